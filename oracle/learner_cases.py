"""The case table of the loss kernels' edge tests -- TEST INFRASTRUCTURE ONLY.

tests/test_learner_reference_cpu.py (the reference against itself, and the tests' power) and
tests/test_gpu_learner_edges.py (the device kernels) build their inputs here, so the
conditions the first asserts on the float64 reference (greedy margins, where the smallest
replay probability sits, exact ties) hold for the inputs the second runs.  Every builder
returns float32 / int32 / uint8 numpy arrays and is deterministic; the CPU test fails if a
condition stops holding.  *_checks() pair every output of a float64 reference with the
Σ|terms| it is measured on (oracle/nature_cnn.py cond_ratio / assert_layer_close).
"""
import numpy as np

from oracle import learner as L

VMAX = 10.0
# on an atom, on the support's edge and far outside it (vmax = 10)
REWARDS = (-30.0, -10.0, -1.0, 0.0, 0.4, 1.0, 2.5, 10.0, 30.0)
CG = np.float32(0.99 ** 3)
SCALES = (2, 10)
MARGIN_C51 = 1e-3 * VMAX      # best - second best target Q
MARGIN_IQN = 1e-3             # best - second best K-mean

# (B, A, N): one wave of one atom pair; the usual 51 atoms; B > 64 with probs and a second row
# per wave (A = 17); every lane on, four rows per wave (A = N = 64); three rows per wave and
# N % 8 != 0 below 8; two atoms at sixteen waves; N < 8; N % 8 == 0
C51_SHAPES = ((1, 1, 2), (5, 3, 51), (65, 17, 51), (33, 64, 64), (64, 33, 7), (3, 16, 2),
              (7, 2, 5), (2, 5, 48))
ZERO_PROB_SHAPE = (64, 33, 7)      # one probability exactly 0, at index 40
MIN_PROB_LAST = (65, 17, 51)       # the smallest probability at index 64


def c51_case(B, A, N, scale, seed=0, cg=CG, all_terminal=False, vmax=VMAX):
  """Inputs of dq_c51_loss: Gaussian logits x scale, rewards from REWARDS, terminal rate 0.3.
  Samples 0 and 1 (B >= 2) are a terminal and a non-terminal one outside the support; with
  B = 1 the sample is terminal at scale 2 and non-terminal at scale 10."""
  rs = np.random.RandomState(1000 * seed + 7 * B + A + N + scale)
  z = L.c51_support(vmax, N, np.float32)
  ol = (rs.randn(B, A, N) * scale).astype(np.float32)
  tl = (rs.randn(B, A, N) * scale).astype(np.float32)
  # a sample whose two best target Q are closer than the margin is drawn again (few atoms at
  # scale 10 saturate the softmax: most rows then sit within rounding of Q = +-vmax)
  for b in range(B):
    for _ in range(100000):
      q = (L.softmax(tl[b].astype(np.float64)) * z.astype(np.float64)).sum(-1)
      if q_margin(q[None])[0] >= MARGIN_C51:
        break
      tl[b] = (rs.randn(A, N) * scale).astype(np.float32)
  act = rs.randint(0, A, B).astype(np.int32)
  rew = rs.choice(REWARDS, B).astype(np.float32)
  term = (rs.rand(B) < 0.3).astype(np.uint8)
  if B >= 2:
    rew[0], term[0] = 30.0, 1
    rew[1], term[1] = -30.0, 0
  else:
    rew[0], term[0] = (30.0, 1) if scale == 2 else (10.0, 0)
  if all_terminal:
    term[:] = 1
  probs = rs.uniform(0.05, 2.0, B).astype(np.float32)
  if (B, A, N) == MIN_PROB_LAST:
    probs[64] = 0.01
  if (B, A, N) == ZERO_PROB_SHAPE:
    probs[40] = 0.0
  return dict(B=B, A=A, N=N, ol=ol, tl=tl, act=act, rew=rew, term=term, z=z, cg=np.float32(cg),
              probs=probs)


def c51_online_case():
  """(B, A, N) = (513, 2, 5) for dq_c51_loss_online (512 threads: the cross-wave minimum):
  the smallest probability sits at index 512."""
  c = c51_case(513, 2, 5, 2)
  c['probs'][512] = 0.01
  return c


def c51_reference(c, probs=True, dtype=np.float64):
  return L.c51_loss(c['ol'], c['tl'], c['act'], c['rew'], c['term'], c['z'], c['cg'],
                    c['probs'] if probs else None, dtype=dtype)


def q_margin(q):
  """best - second best of each row of q (inf with one action)."""
  if q.shape[1] == 1:
    return np.full(q.shape[0], np.inf)
  s = np.sort(np.asarray(q, np.float64), axis=1)
  return s[:, -1] - s[:, -2]


def c51_target_q(c, dtype=np.float64):
  return (L.softmax(np.asarray(c['tl'], dtype)) * np.asarray(c['z'], dtype)).sum(-1)


# ---- exact ties of the greedy action: three atoms on (-1, 0, 1), target rows symmetric about
# the middle atom, so every partial sum of Q = Σ z_i p_i is exact and Q is exactly 0 in fp32
# and in float64 whatever the order of the sum; the three rows project differently
TIE_ROWS = ((0.0, 3.0, 0.0), (3.0, 0.0, 3.0), (0.0, 0.0, 0.0))
TIE_ORDERS = ((0, 1, 2), (2, 0, 1), (1, 2, 0), (2, 1, 0))


def c51_tie_case():
  """One sample per order of TIE_ROWS; zero online logits, so proj = 1/N - B grad."""
  B, A, N = len(TIE_ORDERS), 3, 3
  z = np.array([-1.0, 0.0, 1.0], np.float32)
  tl = np.array([[TIE_ROWS[r] for r in order] for order in TIE_ORDERS], np.float32)
  return dict(B=B, A=A, N=N, ol=np.zeros((B, A, N), np.float32), tl=tl,
              act=np.array([0, 1, 2, 0], np.int32),
              rew=np.array([0.25, 0.25, 0.25, -0.25], np.float32),
              term=np.zeros(B, np.uint8), z=z, cg=np.float32(0.5),
              probs=np.array([0.5, 1.0, 0.25, 2.0], np.float32))


# ---- DQN Huber: small dyadic numbers (every product and sum exact in fp32), the chosen Q set
# so that err = Q - target runs through DQN_ERRS: exactly +1, 0 and -1, and both sides of 1
DQN_SHAPES = ((1, 1), (257, 4), (7, 64), (3, 129))
DQN_ERRS = (1.0, 0.0, -1.0, 0.5, -1.5, 3.0, -0.875, 1.125)


def dqn_case(B, A, cg=0.5, all_terminal=False, dyadic=True, seed=0):
  rs = np.random.RandomState(100 * seed + B + A)
  act = rs.randint(0, A, B).astype(np.int32)
  term = (rs.rand(B) < 0.3).astype(np.uint8)
  if B >= 2:
    term[0], term[1] = 1, 0
  if all_terminal:
    term[:] = 1
  if dyadic:
    oq = (rs.randint(-16, 17, (B, A)) / 4.0).astype(np.float32)
    tq = (rs.randint(-16, 17, (B, A)) / 4.0).astype(np.float32)
    rew = (rs.randint(-8, 9, B) / 4.0).astype(np.float32)
    target = L.dqn_huber(oq, tq, act, rew, term, cg)['target']
    oq[np.arange(B), act] = (target + np.array(DQN_ERRS)[np.arange(B) % len(DQN_ERRS)]).astype(
        np.float32)
  else:
    oq = (rs.randn(B, A) * 3).astype(np.float32)
    tq = (rs.randn(B, A) * 3).astype(np.float32)
    rew = rs.randn(B).astype(np.float32)
  return dict(B=B, A=A, oq=oq, tq=tq, act=act, rew=rew, term=term, cg=np.float32(cg))


def dqn_reference(c, dtype=np.float64):
  return L.dqn_huber(c['oq'], c['tq'], c['act'], c['rew'], c['term'], c['cg'], dtype=dtype)


# ---- IQN: (B, A, N, N', K)
IQN_SHAPES = ((1, 1, 1, 1, 1), (5, 3, 7, 9, 11), (3, 18, 65, 129, 65), (2, 2, 130, 3, 200))
KAPPAS = (0.5, 1.0, 2.0)


def iqn_case(B, A, N, Np, K, seed=0, cg=CG):
  rs = np.random.RandomState(1000 * seed + B + A + N + Np + K)
  return dict(B=B, A=A, N=N, Np=Np, K=K,
              oq=rs.randn(N * B, A).astype(np.float32), tq=rs.randn(Np * B, A).astype(np.float32),
              ta=rs.randn(K * B, A).astype(np.float32), tau=rs.rand(N * B).astype(np.float32),
              act=rs.randint(0, A, B).astype(np.int32), rew=rs.randn(B).astype(np.float32),
              term=(rs.rand(B) < 0.3).astype(np.uint8), cg=np.float32(cg))


def iqn_dyadic_case(kappa):
  """Multiples of 1/4 (times kappa: itself a power of two), gamma 1/2: u = T - theta is exact
  and hits 0 and +-kappa; sample 1 is terminal."""
  B, A, N, Np, K = 2, 3, 9, 8, 4
  rs = np.random.RandomState(5)
  c = dict(B=B, A=A, N=N, Np=Np, K=K, cg=np.float32(0.5))
  c['oq'] = (rs.randint(-8, 9, (N * B, A)) * (kappa / 4.0)).astype(np.float32)
  c['tq'] = (rs.randint(-8, 9, (Np * B, A)) * (kappa / 2.0)).astype(np.float32)
  c['ta'] = (rs.randint(-8, 9, (K * B, A)) / 4.0).astype(np.float32)
  c['ta'][:, 1] += 8.0                       # action 1 is greedy, by far
  c['tau'] = (rs.randint(0, 9, N * B) / 8.0).astype(np.float32)
  c['act'] = np.array([0, 2], np.int32)
  c['rew'] = (np.array([1.0, -0.5]) * kappa).astype(np.float32)
  c['term'] = np.array([0, 1], np.uint8)
  return c


def iqn_tie_case():
  """Columns 1 and 3 of target_qv_action are bit-identical and greedy; their target_qv
  columns differ: the first max takes column 1."""
  c = iqn_case(4, 5, 7, 9, 70, seed=3)
  c['ta'][:, 1] += 4.0
  c['ta'][:, 3] = c['ta'][:, 1]
  c['tq'][:, 3] = c['tq'][:, 1] + 2.0
  return c


def iqn_reference(c, kappa, dtype=np.float64):
  return L.iqn_loss(c['oq'], c['tq'], c['ta'], c['tau'], c['act'], c['rew'], c['term'], c['cg'],
                    kappa=kappa, dtype=dtype)


def iqn_kmean(c, dtype=np.float64):
  return np.asarray(c['ta'], dtype).reshape(c['K'], c['B'], c['A']).mean(0)


# ---- every output of a reference beside the Σ|terms| it is measured on
def c51_checks(ref):
  """name -> (float64 reference, Σ|terms|) for dq_c51_loss's outputs; mean_loss on the
  terms of the weighted mean alone, Σ w |loss| / B (the summary kernel is given the loss)."""
  w, loss = np.asarray(ref['weights'], np.float64), np.asarray(ref['loss'], np.float64)
  return dict(grad=(ref['grad'], ref['grad_abs_proj']), loss=(ref['loss'], ref['loss_abs']),
              priorities=(ref['priorities'], ref['prio_abs']),
              mean_loss=(np.reshape(ref['mean_loss'], 1),
                         np.reshape((w * np.abs(loss)).sum() / len(loss), 1)))


def dqn_checks(ref):
  loss = np.asarray(ref['loss'], np.float64)
  return dict(grad=(ref['grad'], ref['grad_abs']), loss=(ref['loss'], ref['loss_abs']),
              mean_loss=(np.reshape(ref['mean_loss'], 1), np.reshape(np.abs(loss).mean(), 1)))


iqn_checks = dqn_checks


# ---- the fused kernels' synthetic slabs: fc2's k-band partials [n_parts][B][n_out], a bias,
# fc2's weights and the fc1 activation h (about half of it <= 0, some of it exactly 0)
def band_sum(parts, bias):
  """The logits the fused kernels form: the slabs added in band order, then the bias (fp32)."""
  x = parts[0].copy()
  for k in range(1, len(parts)):
    x = x + parts[k]
  return x + bias


# (B, A, N, n_parts, hidden, probs, logits out, fc2_w): every value of n_parts {1, 3, 16},
# hidden {4, 16, 20, 64, 512} (16, 64, 512: d h split four ways; 4, 20: one block per sample),
# A {1, 17, 64} and N {2, 51, 64} at least once, with and without each option
FUSED_ROWS = ((3, 1, 2, 1, 4, True, True, True),
              (5, 17, 51, 3, 20, False, True, True),
              (4, 64, 64, 16, 16, True, False, True),
              (5, 3, 51, 16, 512, True, True, True),
              (3, 17, 64, 3, 64, False, False, True),
              (2, 1, 51, 16, 64, True, False, True),
              (66, 3, 2, 1, 20, True, True, True),
              (3, 64, 51, 3, 4, False, True, False),
              (5, 17, 2, 16, 512, True, False, False),
              (3, 1, 64, 1, 20, False, True, True),
              (4, 17, 51, 1, 16, True, True, True),
              (3, 64, 2, 3, 512, False, False, True),
              (513, 2, 5, 1, 4, True, False, True))
# (B, A, N, n_parts, hidden): atoms on dyadic values (N - 1 divides 2 vmax into a power of two
# times 5), where the exact-target construction below makes the projection exact
EXACT_ROWS = ((3, 1, 2, 1, 4), (513, 2, 5, 3, 4), (4, 17, 17, 16, 20), (3, 64, 33, 3, 512),
              (5, 3, 2, 16, 16))


def fused_case(B, A, N, n_parts, hidden, scale=2, seed=0, exact_target=False):
  """exact_target: one-hot target rows (logit 0 on one atom, -200 elsewhere: the softmax is
  exactly 1 and 0 in fp32 and in float64), rewards that are multiples of 5 and gamma 1/2 on a
  dyadic support: every clipped quotient, hence the projection, is exact in both precisions."""
  rs = np.random.RandomState(1000 * seed + 31 * B + 7 * A + N + n_parts + hidden)
  NO = A * N
  z = L.c51_support(VMAX, N, np.float32)
  sd = scale / np.sqrt(n_parts + 1.0)
  draw = lambda *s: (rs.randn(*s) * sd).astype(np.float32)
  po, bo = draw(n_parts, B, NO), draw(NO)
  if exact_target:
    hot = rs.randint(0, N, (B, A))
    pt = np.zeros((n_parts, B, NO), np.float32)
    pt[0] = np.where(np.arange(N)[None, None, :] == hot[:, :, None], 0.0, -200.0).reshape(B, NO)
    bt = np.zeros(NO, np.float32)
    rew = (rs.randint(-6, 7, B) * 5.0).astype(np.float32)
    cg = np.float32(0.5)
  else:
    pt, bt = draw(n_parts, B, NO), draw(NO)
    for b in range(B):
      for _ in range(100000):
        tlb = band_sum(pt[:, b], bt).reshape(A, N).astype(np.float64)
        if q_margin((L.softmax(tlb) * z.astype(np.float64)).sum(-1)[None])[0] >= MARGIN_C51:
          break
        pt[:, b] = draw(n_parts, NO)
    rew = rs.choice(REWARDS, B).astype(np.float32)
    cg = CG
  term = (rs.rand(B) < 0.3).astype(np.uint8)
  if B >= 2 and not exact_target:
    rew[0], term[0] = 30.0, 1
    rew[1], term[1] = -30.0, 0
  probs = rs.uniform(0.05, 2.0, B).astype(np.float32)
  probs[B - 1] = 0.01                     # the smallest one last (past a wave, past a block)
  h = rs.randn(B, hidden).astype(np.float32)
  h[rs.rand(B, hidden) < 0.1] = 0.0
  return dict(B=B, A=A, N=N, n_parts=n_parts, hidden=hidden, po=po, bo=bo, pt=pt, bt=bt,
              ol=band_sum(po, bo).reshape(B, A, N), tl=band_sum(pt, bt).reshape(B, A, N),
              act=rs.randint(0, A, B).astype(np.int32), rew=rew, term=term, z=z, cg=cg,
              probs=probs, w2=(rs.randn(NO, hidden) * 0.1).astype(np.float32), h=h)


def dh_reference(grad, w2, h, actions):
  """float64 d h = (g . W2[a_b]) (h > 0) on the given logit gradient (B, A, N), and Σ|g||W2|
  (masked alike): only the chosen action's N rows of W2 carry a gradient."""
  B, A, N = grad.shape
  g = np.asarray(grad, np.float64)[np.arange(B), actions]                         # (B, N)
  w = np.asarray(w2, np.float64).reshape(A, N, -1)[actions]                       # (B, N, H)
  keep = np.asarray(h) > 0
  return (np.einsum('bn,bnh->bh', g, w) * keep, np.einsum('bn,bnh->bh', np.abs(g), np.abs(w)) * keep)


# (B, A, n_parts, hidden) of dq_dqn_huber_loss_fused
DQN_FUSED_ROWS = ((3, 1, 1, 4), (5, 64, 3, 20), (4, 64, 16, 512), (2, 1, 16, 512), (130, 4, 3, 20))


def dqn_fused_case(B, A, n_parts, hidden, seed=0):
  rs = np.random.RandomState(1000 * seed + 31 * B + 7 * A + n_parts + hidden)
  draw = lambda *s: (rs.randn(*s) * 3 / np.sqrt(n_parts + 1.0)).astype(np.float32)
  po, bo, pt, bt = draw(n_parts, B, A), draw(A), draw(n_parts, B, A), draw(A)
  term = (rs.rand(B) < 0.3).astype(np.uint8)
  h = rs.randn(B, hidden).astype(np.float32)
  h[rs.rand(B, hidden) < 0.1] = 0.0
  return dict(B=B, A=A, n_parts=n_parts, hidden=hidden, po=po, bo=bo, pt=pt, bt=bt,
              oq=band_sum(po, bo), tq=band_sum(pt, bt), act=rs.randint(0, A, B).astype(np.int32),
              rew=rs.randn(B).astype(np.float32), term=term, cg=np.float32(0.99),
              w2=(rs.randn(A, hidden) * 0.1).astype(np.float32), h=h)
