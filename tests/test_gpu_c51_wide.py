"""dq_c51_loss on supports wider than a wave (k_c51_wide, 65..256 atoms) against float64.

The measure, the bar and the discipline are tests/test_gpu_learner_edges.py's: every output
against the float64 oracle relative to its Σ|terms| (oracle/nature_cnn.py cond_ratio at
COND_FLOOR 1e-3 / LAYER_TOL 1e-5, oracle/learner_cases.py c51_checks), NaN-filled outputs with
one spare sample and 64 guard floats behind the mean that must stay NaN, every output finite.
The cases are tests/c51_wide_cases.py's; tests/test_c51_wide_reference_cpu.py asserts their
conditions and the measure's margin and power on the CPU.  Before the wide kernel every case
here was refused with DQ_E_ARG ("num_atoms must be in [2, 64]").
"""
import numpy as np
import pytest
import torch

from oracle import learner_cases as C
from oracle import nature_cnn as ONC
from tests import c51_wide_cases as W
from tests import test_gpu_learner_edges as E

pytestmark = pytest.mark.gpu

_TABLE = W.table()


@pytest.mark.parametrize('name,c,probs', _TABLE, ids=[t[0] for t in _TABLE])
def test_c51_wide_against_float64(name, c, probs):
  E._check('c51 wide %s' % name, E._run_c51(c, probs), c['B'],
           C.c51_checks(W.reference(name, c, probs)))


def test_c51_wide_optional_outputs_may_be_absent():
  """loss_out, priorities_out, mean_loss_out and probs NULL: the gradient alone, bitwise the
  gradient of the call with every output."""
  from dopamine_amd import _lib
  c = W.case(2, 5, 201, 2, 100.0)
  B, A, N = c['B'], c['A'], c['N']
  full = E._run_c51(c, False)
  grad = E._nan(B + 1, A, N)
  ol, tl, act, rew, term, z = E._dev(c, 'ol', 'tl', 'act', 'rew', 'term', 'z')
  p = _lib.ptr
  _lib.call('dq_c51_loss', p(ol), p(tl), p(act), p(rew), p(term), None, p(z), B, A, N,
            float(c['cg']), p(grad), None, None, None, _lib.stream_of(ol.device))
  torch.cuda.synchronize()
  ONC.assert_spare_untouched('grad alone', grad, B)
  assert torch.equal(grad[:B], full['grad'][:B])


def test_c51_wide_greedy_tie_takes_the_first_max():
  """Three 129-atom target rows with Q exactly 0 each and different projections, in four
  orders: the projection 1/N - B grad (zero online logits, uniform weights) is the first
  row's, and far from the others'."""
  c = W.tie_case()
  B, A, N = c['B'], c['A'], c['N']
  ref = C.c51_reference(c, False)
  bufs = E._run_c51(c, False)
  E._check('c51 wide tie', bufs, B, C.c51_checks(ref))
  grad = bufs['grad'][:B].cpu().numpy().astype(np.float64)
  proj = 1.0 / N - B * grad[np.arange(B), c['act']]
  terms = ref['proj_abs'] + 1.0 / N
  ONC.assert_layer_close('c51 wide tie projection', proj, ref['proj'], terms)
  for a in range(1, A):
    other = C.c51_reference(dict(c, tl=c['tl'][:, [a] * A]), False)['proj']
    r = ONC.cond_ratio(proj, other, terms).reshape(B, N).max(1).values
    assert float(r.min()) > 100 * ONC.LAYER_TOL, (a, r)


def test_c51_wide_two_launches_are_bitwise_equal():
  B, A, N = W.DETERMINISM_SHAPE
  c = W.case(B, A, N, 10, 100.0)
  first, second = E._run_c51(c, True), E._run_c51(c, True)
  torch.cuda.synchronize()
  for k in first:
    n = 1 if k == 'mean_loss' else B
    assert torch.equal(first[k][:n], second[k][:n]), k
    assert bool(torch.isfinite(first[k][:n]).all()), k


@pytest.mark.parametrize('N', [257, 1])
def test_c51_atoms_out_of_range_are_refused_before_a_launch(N):
  from dopamine_amd import _lib
  c = dict(W.case(3, 2, 128, 2, 10.0))
  c['N'] = N
  c['ol'] = np.zeros((3, 2, N), np.float32)
  c['tl'] = np.zeros((3, 2, N), np.float32)
  c['z'] = np.linspace(-10, 10, max(N, 2)).astype(np.float32)[:N]
  ol, tl, act, rew, term, z = E._dev(c, 'ol', 'tl', 'act', 'rew', 'term', 'z')
  bufs = E._loss_bufs(3, (2, N))
  p = _lib.ptr
  with pytest.raises(_lib.DQError, match=r'\[2, 256\]'):
    _lib.call('dq_c51_loss', p(ol), p(tl), p(act), p(rew), p(term), None, p(z), 3, 2, N,
              float(c['cg']), p(bufs['grad']), p(bufs['loss']), p(bufs['priorities']),
              p(bufs['mean_loss']), _lib.stream_of(ol.device))
  torch.cuda.synchronize()
  for k, v in bufs.items():
    assert bool(torch.isnan(v).all()), k


def test_c51_one_wave_of_atoms_still_takes_the_narrow_kernel():
  """N = 64, the last atom count of k_c51, beside N = 65, the first of k_c51_wide."""
  for N in (64, 65):
    c = C.c51_case(3, 2, N, 2)
    E._check('c51 N=%d' % N, E._run_c51(c, True), 3, C.c51_checks(C.c51_reference(c, True)))
