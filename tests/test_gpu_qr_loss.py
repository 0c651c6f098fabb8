"""dq_qr_loss (k_qr) against float64 at its edges.

The measure, the bar and the discipline are tests/test_gpu_learner_edges.py's: every output
against the float64 reference relative to its Σ|terms| (oracle/nature_cnn.py cond_ratio at
COND_FLOOR 1e-3 / LAYER_TOL 1e-5), NaN-filled outputs with one spare sample and 64 guard floats
behind the mean that must stay NaN, every output finite.  The cases and the reference
(oracle.learner.iqn_loss on reordered rows) are tests/qr_cases.py's;
tests/test_qr_reference_cpu.py asserts on the CPU that the cases have the properties they were
built for and that the same assertion tells eight subtly wrong kernels from the right one.
"""
import numpy as np
import pytest
import torch

from oracle import nature_cnn as ONC
from tests import qr_cases as Q
from tests import test_gpu_learner_edges as E

pytestmark = pytest.mark.gpu

_TABLE = Q.table()


def _run(c, kappa, probs, select='case'):
  """ops.qr_loss into NaN buffers.  select: 'case' (the case's select rows), 'target' (the
  target rows passed as select_q) or None (select_q = NULL)."""
  from dopamine_amd import ops
  B, A, N = c['B'], c['A'], c['N']
  bufs = E._loss_bufs(B, (A, N))
  ol, tl, act, rew, term = E._dev(c, 'ol', 'tl', 'act', 'rew', 'term')
  sel = {'case': lambda: E._t(c['sl']), 'target': lambda: tl, None: lambda: None}[select]()
  ops.qr_loss(ol, tl, act, rew, term, c['cg'], kappa=kappa,
              probs=E._t(c['probs']) if probs else None, out=E._views(bufs, B), select_q=sel)
  return bufs


def _bitwise(what, got, want, B):
  torch.cuda.synchronize()
  for k in want:
    n = 1 if k == 'mean_loss' else B
    assert bool(torch.isfinite(got[k][:n]).all()), (what, k)
    assert torch.equal(got[k][:n], want[k][:n]), (what, k)


@pytest.mark.parametrize('name,c,kappa,probs', _TABLE, ids=[t[0] for t in _TABLE])
def test_qr_loss_against_float64(name, c, kappa, probs):
  E._check('qr %s' % name, _run(c, kappa, probs), c['B'],
           Q.qr_checks(Q.reference(name, c, kappa, probs)))


@pytest.mark.parametrize('kappa', Q.KAPPAS)
def test_qr_loss_dyadic_inputs_with_u_exactly_zero_and_at_both_kinks(kappa):
  """Every operation is exact in fp32 (tests/test_qr_reference_cpu.py: u hits 0 and +-kappa):
  loss and gradient equal float64's bit for bit -- the derivative at u = 0 is 0, at
  |u| = kappa it is the quadratic branch's."""
  c = Q.dyadic_case(kappa)
  B = c['B']
  for probs in (False, True):
    ref = Q.qr_reference(c, kappa, probs)
    bufs = _run(c, kappa, probs)
    E._check('qr dyadic k%g %s' % (kappa, probs), bufs, B, Q.qr_checks(ref))
    assert np.array_equal(bufs['loss'][:B].cpu().numpy().astype(np.float64), ref['loss'])
    if not probs:
      assert np.array_equal(bufs['grad'][:B].cpu().numpy().astype(np.float64), ref['grad'])


def test_qr_loss_greedy_tie_takes_the_first_max():
  """Select rows with exactly equal means (in fp32 and float64, whatever the order of the
  sum) in five orders over distinct target rows, tied across waves and inside one: the
  first index wins, and the result lies at least 100 bars from any other tied row's."""
  c = Q.tie_case()
  B = c['B']
  ref = Q.qr_reference(c, 1.0, True)
  assert list(ref['argmax']) == list(Q.TIE_FIRST)
  bufs = _run(c, 1.0, True)
  E._check('qr tie', bufs, B, Q.qr_checks(ref))
  grad = bufs['grad'][:B].cpu().numpy()
  loss = bufs['loss'][:B].cpu().numpy()
  for b, tied in enumerate(Q.tied_actions(c)):
    for a in tied[1:]:
      sl = c['sl'].copy()
      sl[b, a] += 1.0                     # the reference with that other row taken
      other = Q.qr_reference(c, 1.0, True, sl=sl)
      r = ONC.cond_ratio(grad, other['grad'], ref['grad_abs']).reshape(B, -1).max(1).values
      assert float(r[b]) > 100 * ONC.LAYER_TOL, (b, a, r)
      rl = ONC.cond_ratio(loss, other['loss'], ref['loss_abs'])
      assert float(rl[b]) > 100 * ONC.LAYER_TOL, (b, a, rl)


@pytest.mark.parametrize('B,A,N', Q.SHAPES)
def test_qr_loss_null_select_is_bitwise_selecting_with_the_target(B, A, N):
  c = Q.qr_case(B, A, N, 2)
  for probs in (True, False):
    got = _run(c, 1.0, probs, select=None)
    E._untouched('qr null select', got, B)
    _bitwise('B%d A%d N%d %s' % (B, A, N, probs), got, _run(c, 1.0, probs, select='target'), B)
  ref = Q.qr_reference(c, 1.0, True, sl='target')
  E._check('qr select = target', _run(c, 1.0, True, select=None), B, Q.qr_checks(ref))


def test_qr_loss_two_launches_are_bitwise_equal():
  B, A, N = Q.DETERMINISM_SHAPE
  c = Q.qr_case(B, A, N, 10)
  _bitwise('qr twice', _run(c, 1.0, True), _run(c, 1.0, True), B)
  c = Q.qr_case(513, 2, 8, 10, probs_variant='min512')
  _bitwise('qr twice B513', _run(c, 0.5, True), _run(c, 0.5, True), 513)


def _call(c, bufs, N=None, A=None, kappa=1.0, grad=True, loss=True, mean=True):
  from dopamine_amd import _lib
  p = _lib.ptr
  ol, tl, act, rew, term = E._dev(c, 'ol', 'tl', 'act', 'rew', 'term')
  _lib.call('dq_qr_loss', p(ol), p(tl), None, p(act), p(rew), p(term), None, c['B'],
            c['A'] if A is None else A, c['N'] if N is None else N, float(c['cg']), float(kappa),
            p(bufs['grad']) if grad else None, p(bufs['loss']) if loss else None,
            p(bufs['priorities']), p(bufs['mean_loss']) if mean else None,
            _lib.stream_of(ol.device))


@pytest.mark.parametrize('what,kw,msg', [
    ('N=0', dict(N=0), r'num_quantiles must be in \[1, 256\]'),
    ('N=257', dict(N=257), r'num_quantiles must be in \[1, 256\]'),
    ('A=0', dict(A=0), r'num_actions must be in \[1, 64\]'),
    ('A=65', dict(A=65), r'num_actions must be in \[1, 64\]'),
    ('kappa=0', dict(kappa=0.0), 'kappa must be > 0'),
    ('null grad', dict(grad=False), 'null argument'),
    ('mean without loss', dict(loss=False), 'mean_loss_out needs loss_out')],
    ids=['N0', 'N257', 'A0', 'A65', 'kappa0', 'null-grad', 'mean-without-loss'])
def test_qr_loss_refusals_write_nothing(what, kw, msg):
  """Refused with the argument-error status before a launch (the sizes are only claimed: the
  buffers are those of the (3, 2, 65) case and nothing may touch them)."""
  from dopamine_amd import _lib
  c = Q.qr_case(3, 2, 65, 2)
  bufs = E._loss_bufs(3, (2, 65))
  with pytest.raises(_lib.DQError, match=msg) as e:
    _call(c, bufs, **kw)
  assert 'failed (-1)' in str(e.value)           # DQ_E_ARG
  torch.cuda.synchronize()
  for k, v in bufs.items():
    assert bool(torch.isnan(v).all()), (what, k)


def test_qr_loss_works_without_loss_and_priority_outputs():
  """loss_out, priorities_out and mean_loss_out are optional: the gradient alone is bitwise
  the gradient of the full call."""
  from dopamine_amd import ops
  c = Q.qr_case(5, 3, 7, 2)
  B, A, N = c['B'], c['A'], c['N']
  full = _run(c, 1.0, True)
  ol, tl, act, rew, term = E._dev(c, 'ol', 'tl', 'act', 'rew', 'term')
  g = E._nan(B + 1, A, N)
  ops.qr_loss(ol, tl, act, rew, term, c['cg'], probs=E._t(c['probs']), select_q=E._t(c['sl']),
              out=dict(grad=g[:B], loss=None, priorities=None, mean_loss=None))
  torch.cuda.synchronize()
  assert torch.equal(g[:B], full['grad'][:B]) and bool(torch.isnan(g[B:]).all())
