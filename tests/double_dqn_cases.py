"""Inputs and float64 references of the double-DQN loss entries (dq_c51_loss_double,
dq_dqn_huber_loss_double) -- TEST INFRASTRUCTURE ONLY, nothing here touches the GPU.

tests/test_double_dqn_reference_cpu.py proves with the oracle alone that every case has the
property it was built for and that the measure tells the double target from the plain one;
tests/test_gpu_double_dqn_loss.py runs the device kernels on the same inputs.

The references restate nothing: the double-DQN C51 loss is oracle.learner.c51_loss on target
logits whose every action row is the row of a*_b = first argmax_a Q^S[b, a] (all Q equal, the
reference's own first max takes row 0 = row a*), and the double-DQN Huber loss is
oracle.learner.dqn_huber on target Q whose every entry of row b is T_q[b, a*_b] (the max is
that value).  Q^S comes from oracle.learner.softmax on the select logits.

The builders start from oracle/learner_cases.py's c51_case / dqn_case and add the select
logits / Q from a generator of their own, redrawing a sample's select rows until
  * the select Q's best-minus-second-best margin is at least MARGIN_C51 (1e-3 vmax) /
    MARGIN_DQN (1e-3 of the DQN cases' Q range), and
  * with A >= 2, a* differs from the target network's own greedy action (DQN: the target's
    value at a* is below its maximum, and in the dyadic cases the plain target's err is not
    the mirror image -e of the double target's e, which the even Huber loss could not tell
    apart), so a kernel that ignores the select input is wrong on every sample;
and they make sure that every case but the cold ones (cumulative_gamma = 0, all terminal) holds
a *selection-sensitive* sample -- non-terminal with |r| < vmax: c51_case pins samples 0 and 1
to rewards +-30, which (like terminal ones) project to the same distribution whatever row is
chosen -- by setting the last sample non-terminal with reward 0.4 where there is none (always
for B <= 3).  Cases and references are built once and shared: treat them as read-only.
"""
import functools

import numpy as np

from oracle import learner as L
from oracle import learner_cases as C

VMAXES_WIDE = (10.0, 100.0)
MARGIN_DQN = 1e-3 * 4.0        # the dyadic cases' Q lie in [-4, 4], the Gaussian ones' sd is 3

# (B, A, N).  One kernel serves 2..256 atoms: a row is 1..4 chunks of 64 atoms, wave w of four
# takes actions w, w + 4, .. and keeps its own first-max action's target row.
C51_SHAPES = (
    (1, 1, 2),       # one wave, one atom pair
    (5, 3, 51),      # the usual 51 atoms
    (3, 16, 2),      # two atoms, four actions per wave
    (7, 2, 5),       # N < 8; two of the four waves idle
    (2, 5, 48),      # N % 8 == 0; wave 0 has a second action
    (64, 33, 7),     # nine actions on wave 0, eight on the others
    (33, 64, 64),    # every lane on, sixteen actions per wave
    (65, 17, 51),    # smallest probability at index 64
    (2, 2, 65),      # first atom of a second chunk
    (5, 3, 129),     # one atom into the third chunk
    (3, 17, 201),    # the reference config's wide support
    (2, 64, 256),    # both limits: the full LDS footprint
)
MIN_PROB_LAST = (65, 17, 51)
DETERMINISM_SHAPE = (3, 17, 201)


def select_q(c, dtype=np.float64):
  """Q^S (B, A) of a C51 case's select logits."""
  return (L.softmax(np.asarray(c['sl'], dtype)) * np.asarray(c['z'], dtype)).sum(-1)


def sensitive(c, vmax=None):
  """Samples whose loss depends on which target row is taken: non-terminal, gamma > 0 and (C51)
  the reward inside the support."""
  s = (np.asarray(c['term']) == 0) & (float(c['cg']) != 0.0)
  if vmax is not None:
    s &= np.abs(np.asarray(c['rew'], np.float64)) < vmax
  return s


def _ensure_sensitive(c, vmax, cold):
  B = c['B']
  if cold:
    return
  if B <= 3 or not sensitive(c, vmax).any():
    c['rew'][B - 1], c['term'][B - 1] = 0.4, 0


@functools.lru_cache(maxsize=None)
def c51_case(B, A, N, scale, vmax=C.VMAX, cg=None, all_terminal=False, min_prob_last=False):
  kw = {} if cg is None else dict(cg=cg)
  c = C.c51_case(B, A, N, scale, vmax=vmax, all_terminal=all_terminal, **kw)
  if vmax == 100.0 and B >= 2:
    c['rew'][0], c['rew'][1] = 300.0, -300.0      # two samples outside the wide support too
  if min_prob_last:
    c['probs'][B - 1] = 0.01
  _ensure_sensitive(c, vmax, all_terminal or float(c['cg']) == 0.0)
  rs = np.random.RandomState(77000 + 13 * B + 5 * A + N + scale + int(vmax))
  z8 = c['z'].astype(np.float64)
  tgt_greedy = C.c51_target_q(c).argmax(1)
  sl = np.empty((B, A, N), np.float32)
  for b in range(B):
    for _ in range(100000):
      sl[b] = (rs.randn(A, N) * scale).astype(np.float32)
      q = (L.softmax(sl[b].astype(np.float64)) * z8).sum(-1)
      if C.q_margin(q[None])[0] >= 1e-3 * vmax and (A == 1 or q.argmax() != tgt_greedy[b]):
        break
    else:
      raise AssertionError('no select rows for sample %d of %r' % (b, (B, A, N, scale, vmax)))
  c['sl'] = sl
  c['vmax'] = vmax
  return c


def c51_double_reference(c, probs=True, sl=None, dtype=np.float64, astar=None):
  """oracle.learner.c51_loss with row a* of the target logits broadcast over the actions;
  'argmax' is a* (the oracle's own is 0 on the broadcast rows).  astar: taken as given (the
  agent tests' near ties) instead of the first argmax of the select Q."""
  B, A = c['B'], c['A']
  if astar is None:
    astar = select_q(dict(c, sl=c['sl'] if sl is None else sl), dtype).argmax(1)   # first max
  tl = np.repeat(np.asarray(c['tl'])[np.arange(B), astar][:, None, :], A, axis=1)
  ref = L.c51_loss(c['ol'], tl, c['act'], c['rew'], c['term'], c['z'], c['cg'],
                   c['probs'] if probs else None, dtype=dtype)
  ref['argmax'] = astar
  return ref


def c51_table():
  """(id, case, probs?) of every case the GPU test runs against float64 (the tie case apart)."""
  out = []
  for B, A, N in C51_SHAPES:
    for vmax in (VMAXES_WIDE if N > 64 else (C.VMAX,)):
      for scale in C.SCALES:
        c = c51_case(B, A, N, scale, vmax)
        for probs in (True, False):
          out.append(('B%d-A%d-N%d-x%d-v%d-%s' % (B, A, N, scale, vmax, 'per' if probs else 'uni'),
                      c, probs))
  out.append(('gamma0', c51_case(5, 3, 51, 2, cg=0.0), True))
  out.append(('all-terminal', c51_case(7, 2, 5, 2, all_terminal=True), True))
  out.append(('B513', c51_case(513, 2, 5, 2, min_prob_last=True), True))
  return out


COLD = ('gamma0', 'all-terminal')
_REFS = {}


def c51_reference(name, c, probs):
  """The float64 double reference of a table entry, computed once."""
  if name not in _REFS:
    _REFS[name] = c51_double_reference(c, probs)
  return _REFS[name]


def c51_tie_case():
  """learner_cases.c51_tie_case's rows as SELECT rows (three rows with Q exactly 0 each, in
  four orders); the target rows are distinct Gaussian rows, so the three actions project
  differently and the first index must win.  Zero online logits: proj = 1/N - B grad."""
  c = C.c51_tie_case()
  c['sl'] = c['tl']
  rs = np.random.RandomState(77999)
  c['tl'] = (rs.randn(c['B'], c['A'], c['N']) * 2).astype(np.float32)
  c['vmax'] = 1.0
  return c


# ------------------------------------------------------------------------------------ DQN
def _dqn_astar(sq):
  return np.asarray(sq, np.float64).argmax(1)


@functools.lru_cache(maxsize=None)
def dqn_case(B, A, dyadic=True, cg=0.5, all_terminal=False):
  c = C.dqn_case(B, A, cg=cg, all_terminal=all_terminal, dyadic=dyadic)
  cold = all_terminal or float(cg) == 0.0
  if not cold and (B <= 3 or not sensitive(c).any()):
    c['term'][B - 1] = 0
  rs = np.random.RandomState(78000 + 3 * B + A + (1 if dyadic else 0))
  draw = (lambda: (rs.randint(-16, 17, A) / 4.0).astype(np.float32)) if dyadic else (
      lambda: (rs.randn(A) * 3).astype(np.float32))
  sq = np.empty((B, A), np.float32)
  for b in range(B):
    for _ in range(100000):
      sq[b] = draw()
      a = int(sq[b].astype(np.float64).argmax())
      gap = float(c['tq'][b].max()) - float(c['tq'][b, a])      # plain target - double target, / cg
      # (dyadic: Huber is even, so a plain err = e - cg gap that equals -e would give the
      # double loss by coincidence; such a draw is redrawn too)
      mirror = (dyadic and float(cg) != 0.0 and
                float(cg) * gap == 2 * C.DQN_ERRS[b % len(C.DQN_ERRS)])
      if C.q_margin(sq[b][None])[0] >= MARGIN_DQN and (A == 1 or (gap > 0 and not mirror)):
        break
    else:
      raise AssertionError('no select Q for sample %d of %r' % (b, (B, A, dyadic)))
  c['sq'] = sq
  if dyadic:     # the chosen Q from the DOUBLE target: err runs through DQN_ERRS exactly
    target = dqn_double_reference(c)['target']
    c['oq'][np.arange(B), c['act']] = (
        target + np.array(C.DQN_ERRS)[np.arange(B) % len(C.DQN_ERRS)]).astype(np.float32)
  return c


def dqn_double_reference(c, sq=None, dtype=np.float64, astar=None):
  """oracle.learner.dqn_huber with T_q[b, a*_b] broadcast over row b (its max is that value)."""
  B, A = c['B'], c['A']
  if astar is None:
    astar = _dqn_astar(c['sq'] if sq is None else sq)
  tq = np.repeat(np.asarray(c['tq'])[np.arange(B), astar][:, None], A, axis=1)
  ref = L.dqn_huber(c['oq'], tq, c['act'], c['rew'], c['term'], c['cg'], dtype=dtype)
  ref['argmax'] = astar
  return ref


def dqn_table():
  out = []
  for B, A in C.DQN_SHAPES:
    for dyadic in (True, False):
      out.append(('B%d-A%d-%s' % (B, A, 'dyadic' if dyadic else 'randn'),
                  dqn_case(B, A, dyadic), dyadic))
  out.append(('all-terminal', dqn_case(7, 64, True, all_terminal=True), False))
  out.append(('gamma0', dqn_case(257, 4, True, cg=0.0), False))
  return out


def dqn_tie_case():
  """Equal dyadic select Q at two or three actions per sample, the largest of the row; the
  target values at the tied actions differ, so the first index must win."""
  sq = np.array([[1.0, 2.5, 2.5, 0.25], [3.0, 3.0, 3.0, -1.0], [-2.0, -0.5, -4.0, -0.5],
                 [0.0, -1.0, 0.0, 0.0], [1.5, 0.5, 1.75, 1.75]], np.float32)
  tq = np.array([[4.0, -1.0, 2.0, 3.0], [0.5, 2.0, -3.0, 1.0], [1.0, 3.5, 0.0, -2.5],
                 [-1.5, 2.0, 0.5, 3.0], [2.0, 1.0, -0.5, 3.25]], np.float32)
  B, A = sq.shape
  c = dict(B=B, A=A, sq=sq, tq=tq, oq=np.zeros((B, A), np.float32),
           act=np.array([0, 1, 2, 3, 0], np.int32),
           rew=np.array([0.25, -0.5, 1.0, 0.0, 0.75], np.float32),
           term=np.zeros(B, np.uint8), cg=np.float32(0.5))
  target = dqn_double_reference(c)['target']
  c['oq'][np.arange(B), c['act']] = (target + np.array(C.DQN_ERRS)[:B]).astype(np.float32)
  return c
