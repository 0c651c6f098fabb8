"""dq_c51_loss_double (k_c51_double) and dq_dqn_huber_loss_double (k_dqn_double) against
float64, and bitwise against the plain entries when the select input is the target's.

The measure, the bar and the discipline are tests/test_gpu_learner_edges.py's: every output
against the float64 reference relative to its Σ|terms| (oracle/nature_cnn.py cond_ratio at
COND_FLOOR 1e-3 / LAYER_TOL 1e-5), NaN-filled outputs with one spare sample and 64 guard floats
behind the mean that must stay NaN, every output finite.  The cases and references are
tests/double_dqn_cases.py's; tests/test_double_dqn_reference_cpu.py asserts on the CPU that on
every one of them a kernel taking the target's own greedy action misses the bar by 100 x.
"""
import numpy as np
import pytest
import torch

from oracle import learner_cases as C
from oracle import nature_cnn as ONC
from tests import double_dqn_cases as D
from tests import test_gpu_learner_edges as E

pytestmark = pytest.mark.gpu

_C51 = D.c51_table()
_DQN = D.dqn_table()
_C51_CASES = list({id(t[1]): t for t in _C51}.values())      # each case once (per / uni share)


def _run_c51(c, probs, sl=None):
  """ops.c51_loss with select logits (default the case's) into NaN buffers."""
  from dopamine_amd import ops
  B, A, N = c['B'], c['A'], c['N']
  bufs = E._loss_bufs(B, (A, N))
  ol, tl, act, rew, term, z = E._dev(c, 'ol', 'tl', 'act', 'rew', 'term', 'z')
  sel = tl if sl == 'target' else E._t(c['sl'])
  ops.c51_loss(ol, tl, act, rew, term, z, c['cg'], E._t(c['probs']) if probs else None,
               out=E._views(bufs, B), select_logits=sel)
  return bufs


def _run_dqn(c, sq=None):
  from dopamine_amd import ops
  B, A = c['B'], c['A']
  bufs = dict(grad=E._nan(B + 1, A), loss=E._nan(B + 1), mean_loss=E._nan(1 + 64))
  oq, tq, act, rew, term = E._dev(c, 'oq', 'tq', 'act', 'rew', 'term')
  sel = tq if sq == 'target' else E._t(c['sq'])
  ops.dqn_huber_loss(oq, tq, act, rew, term, c['cg'], out=E._views(bufs, B), select_q=sel)
  return bufs


def _bitwise(what, got, want, B):
  torch.cuda.synchronize()
  for k in want:
    n = 1 if k == 'mean_loss' else B
    assert bool(torch.isfinite(got[k][:n]).all()), (what, k)
    assert torch.equal(got[k][:n], want[k][:n]), (what, k)


# ================================================================================== C51
@pytest.mark.parametrize('name,c,probs', _C51, ids=[t[0] for t in _C51])
def test_c51_double_against_float64(name, c, probs):
  E._check('c51 double %s' % name, _run_c51(c, probs), c['B'],
           C.c51_checks(D.c51_reference(name, c, probs)))


@pytest.mark.parametrize('name,c,probs', _C51_CASES, ids=[t[0][:-4] for t in _C51_CASES])
def test_c51_double_selecting_with_the_target_is_bitwise_the_plain_loss(name, c, probs):
  """select == target: every output bitwise dq_c51_loss's, in the one-wave regime (k_c51) and
  the chunked one (k_c51_wide), with and without probabilities."""
  for pr in (True, False):
    got = _run_c51(c, pr, sl='target')
    E._untouched('c51 double self %s' % name, got, c['B'])
    _bitwise('%s %s' % (name, pr), got, E._run_c51(c, pr), c['B'])


def test_c51_double_greedy_tie_takes_the_first_max():
  """Three select rows with Q exactly 0 each, in four orders, over distinct target rows: the
  projection 1/N - B grad (zero online logits, uniform weights) is target row 0's, and far
  from the other rows'."""
  c = D.c51_tie_case()
  B, A, N = c['B'], c['A'], c['N']
  ref = D.c51_double_reference(c, False)
  bufs = _run_c51(c, False)
  E._check('c51 double tie', bufs, B, C.c51_checks(ref))
  grad = bufs['grad'][:B].cpu().numpy().astype(np.float64)
  proj = 1.0 / N - B * grad[np.arange(B), c['act']]
  terms = ref['proj_abs'] + 1.0 / N
  ONC.assert_layer_close('c51 double tie projection', proj, ref['proj'], terms)
  for a in range(1, A):
    other = C.c51_reference(dict(c, tl=c['tl'][:, [a] * A]), False)['proj']
    r = ONC.cond_ratio(proj, other, terms).reshape(B, N).max(1).values
    assert float(r.min()) > 100 * ONC.LAYER_TOL, (a, r)


def test_c51_double_two_launches_are_bitwise_equal():
  B, A, N = D.DETERMINISM_SHAPE
  c = D.c51_case(B, A, N, 10, 100.0)
  _bitwise('c51 double twice', _run_c51(c, True), _run_c51(c, True), B)


def _call_c51_double(c, bufs, sel, N=None, A=None, mean=True, loss=True):
  from dopamine_amd import _lib
  p = _lib.ptr
  ol, tl, act, rew, term, z = E._dev(c, 'ol', 'tl', 'act', 'rew', 'term', 'z')
  _lib.call('dq_c51_loss_double', p(ol), p(tl), p(tl) if sel else None, p(act), p(rew), p(term),
            None, p(z), c['B'], c['A'] if A is None else A, c['N'] if N is None else N,
            float(c['cg']), p(bufs['grad']), p(bufs['loss']) if loss else None,
            p(bufs['priorities']), p(bufs['mean_loss']) if mean else None,
            _lib.stream_of(ol.device))


@pytest.mark.parametrize('what,kw,msg', [
    ('null select', dict(sel=False), 'null select'),
    ('N=1', dict(N=1), r'\[2, 256\]'),
    ('N=257', dict(N=257), r'\[2, 256\]'),
    ('A=65', dict(A=65), 'num_actions must be <= 64'),
    ('mean without loss', dict(loss=False), 'mean_loss_out needs loss_out')],
    ids=['null-select', 'N1', 'N257', 'A65', 'mean-without-loss'])
def test_c51_double_refusals_write_nothing(what, kw, msg):
  """Refused with the argument-error status before a launch (the sizes are only claimed: the
  buffers are those of the (3, 2, 128) case and nothing may touch them)."""
  from dopamine_amd import _lib
  c = D.c51_case(3, 2, 128, 2, 10.0)
  bufs = E._loss_bufs(3, (2, 128))
  kw = dict(dict(sel=True), **kw)
  with pytest.raises(_lib.DQError, match=msg) as e:
    _call_c51_double(c, bufs, **kw)
  assert 'failed (-1)' in str(e.value)           # DQ_E_ARG, as the plain entry's refusals
  torch.cuda.synchronize()
  for k, v in bufs.items():
    assert bool(torch.isnan(v).all()), (what, k)


# ================================================================================== DQN
@pytest.mark.parametrize('name,c,dyadic', _DQN, ids=[t[0] for t in _DQN])
def test_dqn_double_against_float64(name, c, dyadic):
  ref = D.dqn_double_reference(c)
  bufs = _run_dqn(c)
  E._check('dqn double %s' % name, bufs, c['B'], C.dqn_checks(ref))
  if dyadic:                            # every operation exact (the gradient rounds twice)
    assert np.array_equal(bufs['loss'][:c['B']].cpu().numpy(), ref['loss'])


@pytest.mark.parametrize('name,c,dyadic', _DQN, ids=[t[0] for t in _DQN])
def test_dqn_double_selecting_with_the_target_is_bitwise_the_plain_loss(name, c, dyadic):
  got = _run_dqn(c, sq='target')
  E._untouched('dqn double self %s' % name, got, c['B'])
  _bitwise(name, got, E._run_dqn(c), c['B'])


def test_dqn_double_greedy_tie_takes_the_first_max():
  c = D.dqn_tie_case()
  ref = D.dqn_double_reference(c)
  bufs = _run_dqn(c)
  E._check('dqn double tie', bufs, c['B'], C.dqn_checks(ref))
  assert np.array_equal(bufs['loss'][:c['B']].cpu().numpy(), ref['loss'])   # dyadic: exact


def test_dqn_double_two_launches_are_bitwise_equal():
  c = D.dqn_case(257, 4, False)
  _bitwise('dqn double twice', _run_dqn(c), _run_dqn(c), c['B'])


def test_dqn_double_null_select_is_refused_and_writes_nothing():
  from dopamine_amd import _lib
  p = _lib.ptr
  c = D.dqn_case(7, 64, True)
  B, A = c['B'], c['A']
  bufs = dict(grad=E._nan(B + 1, A), loss=E._nan(B + 1), mean_loss=E._nan(1 + 64))
  oq, tq, act, rew, term = E._dev(c, 'oq', 'tq', 'act', 'rew', 'term')
  with pytest.raises(_lib.DQError, match=r'failed \(-1\): .*null select'):
    _lib.call('dq_dqn_huber_loss_double', p(oq), p(tq), None, p(act), p(rew), p(term), B, A,
              float(c['cg']), p(bufs['grad']), p(bufs['loss']), p(bufs['mean_loss']),
              _lib.stream_of(oq.device))
  torch.cuda.synchronize()
  for k, v in bufs.items():
    assert bool(torch.isnan(v).all()), k
