"""Inputs and the float64 reference of the Munchausen-DQN loss entry (dq_mdqn_loss) -- TEST
INFRASTRUCTURE ONLY, nothing here touches the GPU.

tests/test_munchausen_reference_cpu.py proves with numpy alone that every case has the property
it was built for and that the measure tells the Munchausen target from six wrong ones;
tests/test_gpu_munchausen_loss.py runs the device kernel on the same inputs.

The reference is the paper's explicit-sum formula (Vieillard, Pietquin, Geist, NeurIPS 2020,
eq. 2) in float64, for a row x:
  m = max_j x_j,  S = Σ_j exp((x_j - m) / τ),  τ log π_j = x_j - m - τ log S,  π_j = exp(τ log π_j / τ)
  V(s')  = Σ_j π'_j (X'_j - τ log π'_j)
  bonus  = α clip(τ log π_a(X), clip_min, 0)
  target = r + bonus + cg V(s') (1 - terminal)
then oracle.learner.dqn_huber's Huber(1), gradient and Σ|terms|, the target's terms being
|r| + |bonus| + cg (|m'| + τ |log S'|) (1 - terminal).  τ, α, clip_min and cg are float32 values
(what the entry point is handed), widened.

The builders start from oracle/learner_cases.py's dqn_case (Gaussian Q, sd 3), rescale its Q to
the case's sd, and add X = Q'(s, .) (`tqc`) from a generator of their own.  `tq` is X' =
Q'(s', .).  Cases and references are built once and shared: treat them as read-only.
"""
import functools

import numpy as np

from oracle import learner as L
from oracle import learner_cases as C

SHAPES = C.DQN_SHAPES + ((5, 2), (33, 18), (2, 65), (64, 3))
SDS = (0.01, 3.0, 1000.0)
TAUS = (0.03, 1.0, 0.001)
ALPHAS = (0.9, 0.0)
CLIPS = (-1.0, -0.125)
HYPER = tuple((a, cl) for a in ALPHAS for cl in CLIPS)
# err = Q(s, a) - target of the built cases: both Huber branches, never 0 (a zero err hides a
# wrong target from the loss to first order)
ERRS = (1.5, -2.0, 0.75, -0.5)


def _with_hyper(c, tau, alpha, clip_min):
  c.update(tau=np.float32(tau), alpha=np.float32(alpha), clip=np.float32(clip_min))
  return c


@functools.lru_cache(maxsize=None)
def gaussian_case(B, A, sd, tau, alpha, clip_min, cg=0.5, all_terminal=False):
  c = C.dqn_case(B, A, cg=cg, all_terminal=all_terminal, dyadic=False)
  for k in ('oq', 'tq'):
    c[k] = (c[k].astype(np.float64) * (sd / 3.0)).astype(np.float32)
  rs = np.random.RandomState(79000 + 5 * B + A)
  c['tqc'] = (rs.randn(B, A) * sd).astype(np.float32)
  c['sd'] = sd
  return _with_hyper(c, tau, alpha, clip_min)


def _row(x, tau):
  """m (B,), S (B,), τ log π (B, A), π (B, A) of the rows of x, in x's dtype."""
  m = x.max(1, keepdims=True)
  S = np.exp((x - m) / tau).sum(1, keepdims=True)
  tlp = x - m - tau * np.log(S)
  return m[:, 0], S[:, 0], tlp, np.exp(tlp / tau)


def mdqn_reference(c, dtype=np.float64):
  """dict(target, loss, grad, mean_loss, grad_abs, loss_abs, bonus, v) of a case, in ``dtype``."""
  xn, xc, oq = (np.asarray(c[k], dtype) for k in ('tq', 'tqc', 'oq'))
  tau, alpha, clip, cg = (dtype(c[k]) for k in ('tau', 'alpha', 'clip', 'cg'))
  B = oq.shape[0]
  rows, act = np.arange(B), np.asarray(c['act'])
  live = 1 - np.asarray(c['term'], dtype)
  rew = np.asarray(c['rew'], dtype)
  mn, sn, tlpn, pin = _row(xn, tau)
  v = (pin * (xn - tlpn)).sum(1)
  bonus = alpha * np.clip(_row(xc, tau)[2][rows, act], clip, 0)
  target = rew + bonus + cg * v * live
  chosen = oq[rows, act]
  err = chosen - target
  a = np.abs(err)
  quad = np.minimum(a, 1.0)
  loss = 0.5 * quad * quad + (a - quad)
  grad = np.zeros_like(oq)
  grad[rows, act] = np.clip(err, -1.0, 1.0) / B
  target_abs = np.abs(rew) + np.abs(bonus) + cg * (np.abs(mn) + tau * np.abs(np.log(sn))) * live
  mag = np.abs(chosen) + target_abs
  grad_abs = np.zeros_like(oq)
  grad_abs[rows, act] = mag / B
  return dict(loss=loss, grad=grad, grad_abs=grad_abs, target=target, mean_loss=loss.mean(),
              loss_abs=L._huber_terms(a, mag, 1.0), bonus=bonus, v=v)


def _set_errs(c):
  """The chosen Q from the case's own target: err runs through ERRS (to float32 rounding)."""
  B = c['B']
  target = mdqn_reference(c)['target']
  c['oq'][np.arange(B), c['act']] = (target + np.array(ERRS)[np.arange(B) % len(ERRS)]).astype(
      np.float32)
  return c


# ------------------------------------------------------------------------------ built cases
def _built(B, A, tau, alpha, clip_min, cg, all_terminal=False):
  c = gaussian_case(B, A, 3.0, tau, alpha, clip_min, cg=cg, all_terminal=all_terminal)
  c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
  if not all_terminal:
    c['term'][B - 1] = 0            # at least one live sample, whatever dqn_case drew
  return c


@functools.lru_cache(maxsize=None)
def tie_case(A, tau):
  """Every row of X and of X' is one dyadic value repeated: S = A, V = x + τ log A and
  τ log π_a = -τ log A exactly in the reals."""
  B = 6
  c = _built(B, A, tau, 0.9, -1.0, 0.5)
  vals = np.array([0.0, 1.5, -2.25, 4.0, -0.5, 3.0], np.float32)
  c['tq'] = np.repeat(vals[:, None], A, axis=1)
  c['tqc'] = np.repeat(vals[::-1, None], A, axis=1).copy()
  return _set_errs(c)


@functools.lru_cache(maxsize=None)
def greedy_case(B, A, lead):
  """tau = 1.  The taken action is the greedy one of X and every other action sits ``lead``
  below it: τ log π_a = -log(1 + (A - 1) e^-lead), below 0 by a visible amount and above the
  clip at -1 (asserted on the CPU), so the bonus is not clipped."""
  c = _built(B, A, 1.0, 0.9, -1.0, 0.5)
  rows = np.arange(B)
  c['act'] = c['tqc'].argmax(1).astype(np.int32)
  best = c['tqc'].max(1)
  c['tqc'][:] = (best - np.float32(lead))[:, None]
  c['tqc'][rows, c['act']] = best
  return _set_errs(c)


@functools.lru_cache(maxsize=None)
def far_case(B, A, tau, alpha, clip_min, cg=0.5, all_terminal=False):
  """A >= 2.  The taken action's X is 50 below the row's best (τ log π_a <= -50: the bonus is
  exactly α clip_min) and its X' is the best of its row by 4 tau (τ log π'_a is close to 0)."""
  assert A >= 2
  c = _built(B, A, tau, alpha, clip_min, cg, all_terminal)
  rows, act = np.arange(B), c['act']
  c['tqc'][rows, act] = c['tqc'].max(1) - np.float32(50.0)
  c['tq'][rows, act] = c['tq'].max(1) + np.float32(4 * tau)
  return _set_errs(c)


def built_table():
  """(id, case, the wrong kernels it is built to expose) -- see the CPU test's variants."""
  out = []
  for A in (2, 8, 65):
    for tau in (1.0, 0.03):
      out.append(('ties-A%d-t%g' % (A, tau), tie_case(A, tau), ('hard_max', 'no_bonus')))
  out.append(('greedy-B5-A3', greedy_case(5, 3, 1.0), ('no_bonus',)))
  out.append(('greedy-B3-A129', greedy_case(3, 129, 6.0), ('no_bonus',)))
  for (B, A), tau, clip_min in (((7, 4), 0.03, -1.0), ((3, 129), 1.0, -0.125),
                                ((33, 18), 0.001, -1.0)):
    out.append(('far-B%d-A%d-t%g-c%g' % (B, A, tau, clip_min), far_case(B, A, tau, 0.9, clip_min),
                ('no_bonus', 'unclipped', 'bonus_from_next')))
  out.append(('far-alpha0', far_case(7, 4, 0.03, 0.0, -1.0), ()))
  out.append(('all-terminal', far_case(7, 64, 0.03, 0.9, -1.0, all_terminal=True),
              ('no_bonus', 'unclipped', 'bonus_from_next', 'bonus_masked')))
  out.append(('gamma0', far_case(257, 4, 0.03, 0.9, -0.125, cg=0.0),
              ('no_bonus', 'unclipped', 'bonus_from_next')))
  out.append(('B513', gaussian_case(513, 2, 3.0, 0.03, 0.9, -1.0), ()))
  return out


def gaussian_table():
  """Every shape at every sd and tau; (alpha, clip_min) rotate through their four pairs so that
  each pair meets each (sd, tau)."""
  out = []
  for si, (B, A) in enumerate(SHAPES):
    for ki, sd in enumerate(SDS):
      for ti, tau in enumerate(TAUS):
        alpha, clip_min = HYPER[(si + ki + ti) % len(HYPER)]
        out.append(('B%d-A%d-sd%g-t%g-a%g-c%g' % (B, A, sd, tau, alpha, clip_min),
                    gaussian_case(B, A, sd, tau, alpha, clip_min), ()))
  return out


def table():
  return gaussian_table() + built_table()


_REFS = {}


def reference(name, c):
  """The float64 reference of a table entry, computed once."""
  if name not in _REFS:
    _REFS[name] = mdqn_reference(c)
  return _REFS[name]
