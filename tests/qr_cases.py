"""Inputs, float64 reference and fp32 restatement of the quantile-regression loss entry
(dq_qr_loss / k_qr) -- TEST INFRASTRUCTURE ONLY, nothing here touches the GPU.

tests/test_qr_reference_cpu.py proves with the oracle alone that every case has the property it
was built for, that the kernel's documented fp32 summation order stays under the project's bar
and that the measure tells eight subtly wrong kernels from the right one;
tests/test_gpu_qr_loss.py runs the device kernel on the same inputs.

The reference restates nothing: it is oracle.learner.iqn_loss, unchanged, on the rows reordered
to its sample-major layout (row q*B + b), taus set to the midpoints (i + 0.5) / N,
target_qv_action set to the SELECT rows and N' = K = N.  The PER weights (dq_c51_loss's rule),
the priorities sqrt(loss + 1e-10) and their Σ|terms| are added here.

Select rows are redrawn, as tests/double_dqn_cases.py does, until
  * the greedy margin of the select means is at least 1e-3 max(1, max|Q|), and
  * with A >= 2, a* differs from the target rows' own greedy action,
so a kernel that takes the greedy action from the target rows is wrong on every sample.
Cases and references are built once and shared: treat them as read-only.
"""
import functools

import numpy as np

from oracle import learner as L
from oracle import learner_cases as C

SCALES = C.SCALES              # (2, 10)
KAPPAS = C.KAPPAS              # (0.5, 1.0, 2.0)
CG = C.CG

# (B, A, N).  One 256-thread block per sample: thread i owns quantile i, wave w of four takes
# actions w, w + 4, .. (a row is 1..4 chunks of 64 quantiles).
SHAPES = (
    (1, 1, 1),        # the smallest
    (5, 3, 7),        # a partial wave
    (3, 2, 63), (3, 2, 64), (3, 2, 65),    # the wave edge
    (2, 5, 200),      # a wave with two actions; the workload's N
    (2, 64, 256),     # both limits
    (65, 17, 51),     # 2 to 4 target rows per wave; the smallest probability at index 64
    (33, 64, 64),     # sixteen rows per wave
    (513, 2, 8),      # the strided PER minimum
)
MIN_PROB_AT_64 = (65, 17, 51)
STRIDED = (513, 2, 8)          # its variants: the smallest probability at 64 / at 512 / one of 0
DETERMINISM_SHAPE = (2, 5, 200)


def midpoints(N, dtype=np.float64):
  return ((np.arange(N, dtype=dtype) + dtype(0.5)) / dtype(N)).astype(dtype)


def select_means(s, dtype=np.float64):
  return np.asarray(s, dtype).mean(-1)


def margin_floor(q):
  return 1e-3 * max(1.0, float(np.abs(q).max()))


@functools.lru_cache(maxsize=None)
def qr_case(B, A, N, scale, cg=CG, all_terminal=False, probs_variant=None):
  """Gaussian quantile values x scale for the online, target and select outputs (B, A, N),
  rewards x scale / 2, terminal rate 0.3 (sample 0 terminal, sample 1 not, with B >= 2)."""
  rs = np.random.RandomState(91000 + 17 * B + 5 * A + N + scale)
  ol = (rs.randn(B, A, N) * scale).astype(np.float32)
  tl = (rs.randn(B, A, N) * scale).astype(np.float32)
  act = rs.randint(0, A, B).astype(np.int32)
  rew = (rs.randn(B) * scale / 2).astype(np.float32)
  term = (rs.rand(B) < 0.3).astype(np.uint8)
  if B >= 2:
    term[0], term[1] = 1, 0
  else:
    term[0] = 0 if scale == 10 else 1
  if all_terminal:
    term[:] = 1
  probs = rs.uniform(0.05, 2.0, B).astype(np.float32)
  if (B, A, N) == MIN_PROB_AT_64:
    probs[64] = 0.01
  if probs_variant == 'min64':
    probs[64] = 0.01
  elif probs_variant == 'min512':
    probs[512] = 0.01
  elif probs_variant == 'zero':
    probs[300] = 0.0
  else:
    assert probs_variant is None
  tgt_greedy = select_means(tl).argmax(1)
  sl = np.empty((B, A, N), np.float32)
  for b in range(B):
    for _ in range(100000):
      sl[b] = (rs.randn(A, N) * scale).astype(np.float32)
      q = select_means(sl[b])
      if (C.q_margin(q[None])[0] >= margin_floor(q) and
          (A == 1 or q.argmax() != tgt_greedy[b])):
        break
    else:
      raise AssertionError('no select rows for sample %d of %r' % (b, (B, A, N, scale)))
  return dict(B=B, A=A, N=N, ol=ol, tl=tl, sl=sl, act=act, rew=rew, term=term,
              cg=np.float32(cg), probs=probs)


def _rows(x, dtype):
  """(B, A, N) -> oracle.learner.iqn_loss's (N * B, A), row q * B + b."""
  x = np.asarray(x, dtype)
  B, A, N = x.shape
  return np.ascontiguousarray(x.transpose(2, 0, 1)).reshape(N * B, A)


def per_weights(probs, B, dtype=np.float64):
  if probs is None:
    return np.ones(B, dtype)
  w = 1.0 / np.sqrt(np.asarray(probs, dtype) + dtype(1e-10))
  return w / w.max()


def qr_reference(c, kappa=1.0, probs=True, sl=None, dtype=np.float64, astar=None):
  """dict(loss, grad (B, A, N), priorities, mean_loss, weights, argmax and the Σ|terms|
  loss_abs / grad_abs / prio_abs) from oracle.learner.iqn_loss.  sl: other select rows
  ('target': the target rows themselves).  astar: taken as given (the agent tests' near ties)
  -- the select rows are then ones on row a*_b and zeros elsewhere."""
  B, A, N = c['B'], c['A'], c['N']
  sel = c['sl'] if sl is None else (c['tl'] if isinstance(sl, str) else sl)
  if astar is not None:
    sel = np.zeros((B, A, N), dtype)
    sel[np.arange(B), astar] = 1.0
  taus = np.tile(midpoints(N, dtype)[:, None], (1, B)).reshape(-1)
  r = L.iqn_loss(_rows(c['ol'], dtype), _rows(c['tl'], dtype), _rows(sel, dtype), taus, c['act'],
                 c['rew'], c['term'], c['cg'], kappa=dtype(kappa), dtype=dtype)
  w = per_weights(c['probs'] if probs else None, B, dtype)
  back = lambda g: np.asarray(g).reshape(N, B, A).transpose(1, 2, 0)
  loss = r['loss']
  prio = np.sqrt(loss + dtype(1e-10))
  f8 = np.float64
  return dict(loss=loss, grad=back(r['grad']) * w[:, None, None],
              grad_abs=back(r['grad_abs']).astype(f8) * w.astype(f8)[:, None, None],
              loss_abs=r['loss_abs'], priorities=prio,
              prio_abs=r['loss_abs'] / (2 * prio.astype(f8)), weights=w,
              mean_loss=(w * loss).mean(), argmax=r['argmax'])


def qr_checks(ref):
  """name -> (float64 reference, Σ|terms|); mean_loss on the terms of the weighted mean alone
  (the summary kernel is given the loss), as learner_cases.c51_checks."""
  w, loss = np.asarray(ref['weights'], np.float64), np.asarray(ref['loss'], np.float64)
  return dict(grad=(ref['grad'], ref['grad_abs']), loss=(ref['loss'], ref['loss_abs']),
              priorities=(ref['priorities'], ref['prio_abs']),
              mean_loss=(np.reshape(ref['mean_loss'], 1),
                         np.reshape((w * np.abs(loss)).sum() / len(loss), 1)))


def table():
  """(id, case, kappa, probs?) of every case run against float64 (dyadic and tie cases apart)."""
  out = []
  for B, A, N in SHAPES:
    variants = ('min64', 'min512') if (B, A, N) == STRIDED else (None,)
    for scale in SCALES:
      for pv in variants:
        c = qr_case(B, A, N, scale, probs_variant=pv)
        for kappa in KAPPAS:
          for probs in (True, False):
            if not probs and pv == 'min512':
              continue                       # the same inputs as min64 without probabilities
            out.append(('B%d-A%d-N%d-x%d%s-k%g-%s' % (B, A, N, scale, '-' + pv if pv else '',
                                                      kappa, 'per' if probs else 'uni'),
                        c, kappa, probs))
  out.append(('zero-prob', qr_case(513, 2, 8, 2, probs_variant='zero'), 1.0, True))
  for B, A, N in SHAPES:
    out.append(('gamma0-B%d-A%d-N%d' % (B, A, N), qr_case(B, A, N, 2, cg=0.0), 1.0, True))
    out.append(('all-terminal-B%d-A%d-N%d' % (B, A, N), qr_case(B, A, N, 2, all_terminal=True),
                1.0, True))
  return out


_REFS = {}


def reference(name, c, kappa, probs):
  """The float64 reference of a table entry, computed once."""
  if name not in _REFS:
    _REFS[name] = qr_reference(c, kappa, probs)
  return _REFS[name]


def dyadic_case(kappa):
  """Multiples of kappa / 4 (kappa a power of two), gamma 1/2, N = 8 (dyadic midpoints): every
  operation of the loss is exact in fp32, u = y - theta hits 0 and +-kappa; sample 1 is
  terminal; action 1 is greedy by far."""
  B, A, N = 2, 3, 8
  rs = np.random.RandomState(6)
  c = dict(B=B, A=A, N=N, cg=np.float32(0.5))
  c['ol'] = (rs.randint(-8, 9, (B, A, N)) * (kappa / 4.0)).astype(np.float32)
  c['tl'] = (rs.randint(-8, 9, (B, A, N)) * (kappa / 2.0)).astype(np.float32)
  c['sl'] = (rs.randint(-8, 9, (B, A, N)) / 4.0).astype(np.float32)
  c['sl'][:, 1] += 8.0
  c['act'] = np.array([0, 2], np.int32)
  c['rew'] = (np.array([1.0, -0.5]) * kappa).astype(np.float32)
  c['term'] = np.array([0, 1], np.uint8)
  c['probs'] = np.array([0.25, 1.0], np.float32)
  return c


def dyadic_u(c):
  """u[b, j, i] of a case in float64."""
  B = c['B']
  ref = qr_reference(c, 1.0, False)
  gam = np.float64(c['cg']) * (1 - c['term'].astype(np.float64))
  y = c['rew'].astype(np.float64)[:, None] + gam[:, None] * c['tl'].astype(np.float64)[
      np.arange(B), ref['argmax']]
  theta = c['ol'].astype(np.float64)[np.arange(B), c['act']]
  return y[:, :, None] - theta[:, None, :]


# ---- exact ties of the greedy action: small integers, so every partial sum of a row (whatever
# its order) and its mean are exact in fp32 and in float64.  Three rows of mean 2 and three of
# mean 1, in several orders over six actions: ties across waves (actions 0, 1, 2) and inside
# one (actions 1 and 5 are both wave 1's).
TIE_ROWS = ((1.0, 2.0, 3.0, 2.0), (2.0, 2.0, 2.0, 2.0), (0.0, 4.0, 4.0, 0.0),
            (1.0, 1.0, 1.0, 1.0), (0.0, 2.0, 2.0, 0.0), (4.0, 0.0, 0.0, 0.0))
TIE_ORDERS = ((0, 1, 2, 3, 4, 5), (3, 0, 4, 5, 2, 1), (3, 1, 4, 5, 0, 2), (5, 4, 3, 2, 1, 0),
              (3, 2, 4, 5, 1, 0))
TIE_FIRST = (0, 1, 1, 3, 1)       # the first action of mean 2 in each order


def tie_case():
  B, A, N = len(TIE_ORDERS), 6, 4
  rs = np.random.RandomState(91999)
  sl = np.array([[TIE_ROWS[r] for r in order] for order in TIE_ORDERS], np.float32)
  return dict(B=B, A=A, N=N, sl=sl, tl=(rs.randn(B, A, N) * 2).astype(np.float32),
              ol=(rs.randn(B, A, N) * 2).astype(np.float32),
              act=np.array([0, 5, 2, 3, 1], np.int32),
              rew=np.array([0.25, -0.5, 1.0, 0.0, 0.75], np.float32),
              term=np.zeros(B, np.uint8), cg=np.float32(0.5),
              probs=np.array([0.5, 1.0, 0.25, 2.0, 0.125], np.float32))


def tied_actions(c):
  """Per sample, the actions whose select mean equals the largest one."""
  q = select_means(c['sl'])
  return [np.flatnonzero(q[b] == q[b].max()) for b in range(c['B'])]


# ---------------------------------------------------------------------------------------------
# The kernel's arithmetic restated in fp32 numpy, in its documented summation order (DESIGN
# §4.4, the header of k_qr in csrc/qr.hip):
#   row sum     each 64-quantile chunk by the DPP tree (rotations by 8, 4, 2, 1 inside each
#               16-lane row, then (r0 + r1) + (r2 + r3)), the chunks added in chunk order
#   row mean    row sum / N; a* the first maximum
#   j walk      four partial sums, term j into partial j mod 4, each in j order, combined as
#               (p0 + p1) + (p2 + p3) -- for the loss terms and for the gradient terms
#   block sum   the per-quantile sums by the DPP tree per wave, the four waves as
#               ((s0 + s1) + s2) + s3; loss = (sum / N) / kappa
#   mean        k_wmean: lane l adds samples l, l + 64, .. in order, then the xor butterfly
# ``wrong``: one of WRONG, a deliberately wrong kernel.
# ---------------------------------------------------------------------------------------------
WRONG = ('tau_i_over_n', 'indicator_gt', 'terminal_ignored', 'grad_without_1_over_n',
         'last_max', 'per_max_first_64', 'greedy_from_target', 'quantile_major')
f4 = np.float32


def _dpp_sum(x):
  s = x.reshape(x.shape[:-1] + (4, 16))
  for k in (8, 4, 2, 1):
    s = s + np.roll(s, k, axis=-1)
  r = s[..., 0]
  return (r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])


def _chunks(x):
  N = x.shape[-1]
  nch = (N + 63) // 64
  pad = np.zeros(x.shape[:-1] + (nch * 64,), f4)
  pad[..., :N] = x
  return [_dpp_sum(pad[..., 64 * k:64 * k + 64]) for k in range(nch)]


def _row_sum(x):
  parts = _chunks(x)
  tot = parts[0]
  for p in parts[1:]:
    tot = tot + p
  return tot


def _first_max(q, last=False):
  if last:
    return q.shape[1] - 1 - q[:, ::-1].argmax(1)
  return q.argmax(1)


def _wmean(loss, probs):
  B = len(loss)
  if probs is None:
    w = np.ones(B, f4)
  else:
    iw = f4(1) / np.sqrt(probs + f4(1e-10))
    w = iw / iw.max()
  acc = np.zeros(64, f4)
  for b in range(B):
    acc[b % 64] = acc[b % 64] + w[b] * loss[b]
  for o in (32, 16, 8, 4, 2, 1):
    acc = acc + acc[np.arange(64) ^ o]
  return acc[0] / f4(B)


def qr_fp32(c, kappa=1.0, probs=True, sl=None, wrong=None):
  assert wrong is None or wrong in WRONG
  B, A, N = c['B'], c['A'], c['N']
  kappa = f4(kappa)
  view = lambda x: np.asarray(x, f4)
  if wrong == 'quantile_major':
    view = lambda x: np.ascontiguousarray(np.asarray(x, f4).reshape(B, N, A).transpose(0, 2, 1))
  ol, tl = view(c['ol']), view(c['tl'])
  sel = view(c['sl'] if sl is None else (c['tl'] if isinstance(sl, str) else sl))
  if wrong == 'greedy_from_target':
    sel = tl
  rows = np.arange(B)
  q = _row_sum(sel) / f4(N)
  astar = _first_max(q, last=wrong == 'last_max')
  term = np.zeros(B, f4) if wrong == 'terminal_ignored' else c['term'].astype(f4)
  gt = f4(c['cg']) * (f4(1) - term)
  y = c['rew'].astype(f4)[:, None] + gt[:, None] * tl[rows, astar]          # (B, N) over j
  theta = ol[rows, c['act']]                                                # (B, N) over i
  idx = np.arange(N, dtype=f4)
  # |tau_i - 1{u < 0}| without the cancellation near tau = 1: (i + 0.5) / N where u >= 0 and
  # (N - i - 0.5) / N where u < 0, one correctly rounded quotient each
  half = f4(0.0) if wrong == 'tau_i_over_n' else f4(0.5)
  w_pos, w_neg = (idx + half) / f4(N), ((f4(N) - idx) - half) / f4(N)
  hk = f4(0.5) * kappa
  rho = [np.zeros((B, N), f4) for _ in range(4)]
  gs = [np.zeros((B, N), f4) for _ in range(4)]
  for j in range(N):
    u = y[:, j, None] - theta
    au = np.abs(u)
    inner = au <= kappa
    h = np.where(inner, (f4(0.5) * u) * u, kappa * (au - hk))
    neg = (u > 0) if wrong == 'indicator_gt' else (u < 0)
    w = np.where(neg, w_neg[None, :], w_pos[None, :])
    dh = np.where(inner, u, kappa * np.sign(u).astype(f4))
    rho[j & 3] = rho[j & 3] + w * h
    gs[j & 3] = gs[j & 3] + w * dh
  rho = (rho[0] + rho[1]) + (rho[2] + rho[3])
  gs = (gs[0] + gs[1]) + (gs[2] + gs[3])
  pad = np.zeros((B, 256), f4)
  pad[:, :N] = rho
  s = [_dpp_sum(pad[:, 64 * k:64 * k + 64]) for k in range(4)]
  tot = ((s[0] + s[1]) + s[2]) + s[3]
  loss = (tot / f4(N)) / kappa
  prio = np.sqrt(loss + f4(1e-10))
  pr = c['probs'].astype(f4) if probs else None
  if pr is None:
    w_b = np.ones(B, f4)
  else:
    pm = pr[:64].min() if wrong == 'per_max_first_64' else pr.min()
    w_b = (f4(1) / np.sqrt(pr + f4(1e-10))) / (f4(1) / np.sqrt(pm + f4(1e-10)))
  den = (f4(B) * kappa) if wrong == 'grad_without_1_over_n' else ((f4(N) * f4(B)) * kappa)
  gscale = w_b * (f4(-1) / den)
  grad = np.zeros((B, A, N), f4)
  grad[rows, c['act']] = gs * gscale[:, None]
  if wrong == 'quantile_major':     # written back in the layout it was read in
    grad = np.ascontiguousarray(grad.transpose(0, 2, 1)).reshape(B, A, N)
  assert loss.dtype == f4 and grad.dtype == f4 and prio.dtype == f4
  return dict(loss=loss, grad=grad, priorities=prio,
              mean_loss=np.reshape(_wmean(loss, pr), 1), argmax=astar)
