"""dq_mdqn_loss (k_mdqn) against float64, bitwise against dq_dqn_huber_loss at one action, and
its host refusals.

The measure, the bar and the discipline are tests/test_gpu_learner_edges.py's: every output
against the float64 reference relative to its Σ|terms| (oracle/nature_cnn.py cond_ratio at
COND_FLOOR 1e-3 / LAYER_TOL 1e-5), NaN-filled outputs with one spare sample and 64 guard floats
behind the mean that must stay NaN, every output finite.  The cases and the reference are
tests/munchausen_cases.py's; tests/test_munchausen_reference_cpu.py asserts on the CPU that six
wrong kernels miss the bar by 100 x on the cases built for them.
"""
import pytest
import torch

from oracle import learner_cases as C
from tests import munchausen_cases as M
from tests import test_gpu_learner_edges as E

pytestmark = pytest.mark.gpu

_TABLE = M.table()
_A1 = [(n, c) for n, c, _ in _TABLE if c['A'] == 1]


def _bufs(B, A):
  return dict(grad=E._nan(B + 1, A), loss=E._nan(B + 1), mean_loss=E._nan(1 + 64))


def _run(c):
  """ops.mdqn_loss into NaN buffers."""
  from dopamine_amd import ops
  B, A = c['B'], c['A']
  bufs = _bufs(B, A)
  oq, tq, tqc, act, rew, term = E._dev(c, 'oq', 'tq', 'tqc', 'act', 'rew', 'term')
  ops.mdqn_loss(oq, tq, tqc, act, rew, term, c['cg'], c['tau'], c['alpha'], c['clip'],
                out=E._views(bufs, B))
  return bufs


def _bitwise(what, got, want, B):
  torch.cuda.synchronize()
  for k in want:
    n = 1 if k == 'mean_loss' else B
    assert bool(torch.isfinite(got[k][:n]).all()), (what, k)
    assert torch.equal(got[k][:n], want[k][:n]), (what, k)


@pytest.mark.parametrize('name,c,built_for', _TABLE, ids=[t[0] for t in _TABLE])
def test_mdqn_against_float64(name, c, built_for):
  E._check('mdqn %s' % name, _run(c), c['B'], C.dqn_checks(M.reference(name, c)))


@pytest.mark.parametrize('name,c', _A1, ids=[t[0] for t in _A1])
def test_mdqn_with_one_action_is_bitwise_the_plain_loss(name, c):
  """pi = 1, log pi = 0, exp(0) and log(1) exact, the bonus +0: every output is
  dq_dqn_huber_loss's on (online_q, target_next_q), whatever tau, alpha and the clip."""
  got = _run(c)
  E._untouched('mdqn A=1 %s' % name, got, c['B'])
  _bitwise(name, got, E._run_dqn(c), c['B'])


@pytest.mark.parametrize('B,A', [(257, 4), (3, 129)])
def test_mdqn_two_launches_are_bitwise_equal(B, A):
  c = M.gaussian_case(B, A, 3.0, 1.0, 0.9, -1.0)
  _bitwise('mdqn twice', _run(c), _run(c), B)


def _call(c, bufs, null=None, B=None, A=None, tau=None, alpha=None, clip=None, loss=True):
  from dopamine_amd import _lib
  p = _lib.ptr
  oq, tq, tqc, act, rew, term = E._dev(c, 'oq', 'tq', 'tqc', 'act', 'rew', 'term')
  ptrs = dict(oq=p(oq), tq=p(tq), tqc=p(tqc), act=p(act), rew=p(rew), term=p(term),
              grad=p(bufs['grad']))
  if null is not None:
    ptrs[null] = None
  pick = lambda v, d: float(d) if v is None else v
  _lib.call('dq_mdqn_loss', ptrs['oq'], ptrs['tq'], ptrs['tqc'], ptrs['act'], ptrs['rew'],
            ptrs['term'], c['B'] if B is None else B, c['A'] if A is None else A, float(c['cg']),
            pick(tau, c['tau']), pick(alpha, c['alpha']), pick(clip, c['clip']), ptrs['grad'],
            p(bufs['loss']) if loss else None, p(bufs['mean_loss']), _lib.stream_of(oq.device))


_INF, _NAN = float('inf'), float('nan')
_REFUSALS = ([('null %s' % k, dict(null=k), 'null argument')
              for k in ('oq', 'tq', 'tqc', 'act', 'rew', 'term', 'grad')] + [
    ('B=0', dict(B=0), 'bad sizes'), ('A=0', dict(A=0), 'bad sizes'),
    ('B=-1', dict(B=-1), 'bad sizes'),
    ('tau=0', dict(tau=0.0), 'tau must be'), ('tau<0', dict(tau=-0.03), 'tau must be'),
    ('tau=inf', dict(tau=_INF), 'tau must be'), ('tau=nan', dict(tau=_NAN), 'tau must be'),
    ('alpha<0', dict(alpha=-0.5), 'alpha must be'), ('alpha=inf', dict(alpha=_INF), 'alpha must be'),
    ('alpha=nan', dict(alpha=_NAN), 'alpha must be'),
    ('clip>0', dict(clip=0.25), 'clip_min must be'), ('clip=-inf', dict(clip=-_INF), 'clip_min must be'),
    ('clip=nan', dict(clip=_NAN), 'clip_min must be'),
    ('mean without loss', dict(loss=False), 'mean_loss_out needs loss_out')])


@pytest.mark.parametrize('what,kw,msg', _REFUSALS, ids=[r[0].replace(' ', '-') for r in _REFUSALS])
def test_mdqn_refusals_write_nothing(what, kw, msg):
  """Refused with the argument-error status before a launch: every buffer stays NaN."""
  from dopamine_amd import _lib
  c = M.gaussian_case(7, 64, 3.0, 0.03, 0.9, -1.0)
  bufs = _bufs(c['B'], c['A'])
  with pytest.raises(_lib.DQError, match=msg) as e:
    _call(c, bufs, **kw)
  assert 'failed (-1)' in str(e.value)           # DQ_E_ARG
  torch.cuda.synchronize()
  for k, v in bufs.items():
    assert bool(torch.isnan(v).all()), (what, k)
