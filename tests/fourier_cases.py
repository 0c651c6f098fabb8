"""The Fourier-basis Q-network (reference gym_lib.py:135-206) and plain gradient descent,
restated for the tests: a float64 reference, an fp32 numpy restatement in the kernels' order,
the cases, and the measures.  No GPU here.

The definition (steps as the kernels' header lists them):
  x32 = float32(x);  s = (x32 - float32(MIN)) / float32(MAX - MIN)   (float32, no clipping)
  m_f = digits of f + 1 in base order + 1, dimension 0 most significant
        (= itertools.product(range(order + 1), repeat=D) without its first tuple)
  z_f = sum_d m_{f,d} s_d;  arg_f = float32(pi) z_f;  phi_f = cos(arg_f)
  q[b][a] = sum_f phi[b][f] W[a][f];  dW[a][f] = sum_b dq[b][a] phi[b][f]
  SGD: var <- var - lr g (the product rounded, then the difference).
float32(pi), not pi: np.pi enters the reference's TF graph as a float32 constant.
"""
import itertools

import numpy as np

PI32 = np.float32(np.pi)

# (B, D, order, A, input is float64): the edge each one tests is in
# tests/test_gpu_fourier_layers.py's docstring
CASES = ((128, 4, 3, 2, True), (33, 6, 3, 3, False), (1, 1, 1, 1, True), (5, 2, 4, 7, True),
         (3, 3, 6, 5, True), (257, 2, 3, 4, True))

_CARTPOLE = (np.array([-2.4, -5., -np.pi / 12., -np.pi * 2.]),
             np.array([2.4, 5., np.pi / 12., np.pi * 2.]))
_ACROBOT = (np.array([-1., -1., -1., -1., -5., -5.]), np.array([1., 1., 1., 1., 5., 5.]))


def bounds(D):
  """(MIN, MAX) float64 of a D-dimensional box: CartPole's, Acrobot's, or a seeded one."""
  if D == 4:
    return _CARTPOLE
  if D == 6:
    return _ACROBOT
  rs = np.random.RandomState(D)
  lo = -rs.uniform(0.5, 6.0, size=D)
  return lo, lo + rs.uniform(1.0, 12.0, size=D)


def case_id(c):
  return 'B%d-D%d-o%d-A%d' % c[:4]


def n_features(D, order):
  return (order + 1) ** D - 1


def multipliers(D, order):
  """The digit rule, (F, D) int64."""
  base = order + 1
  n = np.arange(1, n_features(D, order) + 1, dtype=np.int64)
  out = np.zeros((len(n), D), dtype=np.int64)
  for d in range(D - 1, -1, -1):
    out[:, d] = n % base
    n = n // base
  return out


def multipliers_product(D, order):
  """gym_lib.py:153-157 as the reference writes it."""
  return np.array(list(itertools.product(range(order + 1), repeat=D))[1:], dtype=np.int64)


def make_inputs(case, seed=0):
  """x (B, D) drawn from 10% outside the box on both sides, W (A, F) Xavier-uniform, dq (B, A)."""
  B, D, order, A, f64 = case
  rs = np.random.RandomState(1000 * B + 10 * D + order + seed)
  lo, hi = bounds(D)
  u = rs.uniform(-0.1, 1.1, size=(B, D))
  u.flat[-1] = 1.1                  # both ends of the range are in every case
  u.flat[0] = -0.1
  x = lo + (hi - lo) * u
  if not f64:
    x = x.astype(np.float32)
  F = n_features(D, order)
  lim = np.sqrt(6.0 / (F + A))
  w = rs.uniform(-lim, lim, size=(A, F)).astype(np.float32)
  dq = rs.standard_normal((B, A)).astype(np.float32)
  return x, w, dq


def scale32(x, lo, hi):
  """Step 2, bitwise what the kernel stores: float32 throughout, MAX - MIN subtracted in
  float64."""
  x32 = np.asarray(x).astype(np.float32)
  lo = np.asarray(lo, np.float64)
  rng = (np.asarray(hi, np.float64) - lo).astype(np.float32)
  s = (x32 - lo.astype(np.float32)) / rng
  assert s.dtype == np.float32
  return s


def phi64(s, D, order):
  """(phi, arg) float64 from a given float32 s: z in float64, arg = float32(pi) z."""
  z = np.asarray(s, np.float64) @ multipliers(D, order).T.astype(np.float64)
  arg = np.float64(PI32) * z
  return np.cos(arg), arg


def reference64(case, x, w, dq):
  """float64 steps 2-7 from the float32 s."""
  B, D, order, A, _ = case
  s = scale32(x, *bounds(D))
  phi, arg = phi64(s, D, order)
  q = phi @ np.asarray(w, np.float64).T
  dw = np.asarray(dq, np.float64).T @ phi
  return dict(s=s, phi=phi, arg=arg, q=q, dw=dw)


def restate32(case, x, w, dq, variant=None):
  """The kernels' arithmetic in numpy float32: z summed in d order, every product and sum
  rounded, the head and the weight gradient summed sequentially (their worst order).
  variant: one of WRONG, a deliberately wrong restatement."""
  B, D, order, A, _ = case
  lo, hi = bounds(D)
  s = scale32(x, lo, hi)
  if variant == 'rescale':            # the MLP's [-1, 1]
    s = np.float32(2.0) * s - np.float32(1.0)
  base = order if variant == 'base' else order + 1
  F = n_features(D, order)
  n = np.arange(1, F + 1, dtype=np.int64) - (1 if variant == 'constant' else 0)
  m = np.zeros((F, D), dtype=np.int64)
  for d in (range(D) if variant == 'digits' else range(D - 1, -1, -1)):
    m[:, d] = n % max(base, 1) if base > 1 else 0
    n = n // max(base, 1) if base > 1 else n
  z = np.zeros((B, F), dtype=np.float32)
  for d in range(D):
    z = z + m[None, :, d].astype(np.float32) * s[:, d:d + 1]
  arg = PI32 * z
  assert arg.dtype == np.float32
  phi = (np.sin(arg) if variant == 'sin' else np.cos(arg)).astype(np.float32)
  w = np.asarray(w, np.float32)
  dq = np.asarray(dq, np.float32)
  q = np.zeros((B, A), dtype=np.float32)
  for f in range(F):
    q = q + phi[:, f:f + 1] * w[None, :, f]
  dw = np.zeros((A, F), dtype=np.float32)
  rows = B - 1 if variant == 'row' else B
  for b in range(rows):
    g = dq[b, :1] if variant == 'action' else dq[b]
    dw = dw + g[:, None] * phi[b][None, :]
  assert q.dtype == dw.dtype == np.float32
  return dict(s=s, phi=phi, arg=arg, q=q, dw=dw)


WRONG = ('digits', 'constant', 'base', 'rescale', 'sin', 'row', 'action')


def phi_bound(D, arg):
  """2 D 2^-24 max(1, |arg|) + 2^-22: the D products, D - 1 sums and the multiplication by
  float32(pi) round once each (2 D roundings, each at most 2^-24 of a partial sum that |arg|
  bounds up to the factor pi, which the slope-1 cosine does not amplify further), and the
  cosine itself gets two ulp of a value at most 1 (2 * 2^-23 = 2^-22)."""
  return 2.0 * D * 2.0 ** -24 * np.maximum(1.0, np.abs(arg)) + 2.0 ** -22


def phi_excess(phi, s, D, order):
  """max of |phi - cos64| / bound over the elements (<= 1 passes), and the worst
  |phi - cos64| / max(1, |arg|)."""
  want, arg = phi64(s, D, order)
  err = np.abs(np.asarray(phi, np.float64) - want)
  return float((err / phi_bound(D, arg)).max()), float((err / np.maximum(1.0, np.abs(arg))).max())


COND_FLOOR = 1e-3      # oracle.nature_cnn's measure, restated for numpy
LAYER_TOL = 1e-5


def cond(got, ref, terms):
  got, ref, terms = (np.asarray(a, np.float64) for a in (got, ref, terms))
  den = np.maximum(np.maximum(terms, COND_FLOOR * np.abs(ref).max()), 1e-300)
  return float((np.abs(got - ref) / den).max())


def head_errors(phi, w, dq, q, dw):
  """(q, dW) on the cond measure against float64 on the given phi."""
  p64, w64, g64 = (np.asarray(a, np.float64) for a in (phi, w, dq))
  return (cond(q, p64 @ w64.T, np.abs(p64) @ np.abs(w64).T),
          cond(dw, g64.T @ p64, np.abs(g64).T @ np.abs(p64)))


def check_restatement(case, r, x, w, dq):
  """Every bar of the layer tests on a restatement's results -> list of the bars it misses."""
  B, D, order, A, _ = case
  missed = []
  s = scale32(x, *bounds(D))
  if not np.array_equal(r['s'].view(np.uint32), s.view(np.uint32)):
    missed.append('s')
  if phi_excess(r['phi'], s, D, order)[0] > 1.0:
    missed.append('phi')
  # the head and the gradient against float64 on the restatement's own features, as the
  # device's are judged on the device's
  if r['q'].shape != (B, A) or r['dw'].shape != (A, n_features(D, order)):
    return missed + ['q', 'dw']
  qe, dwe = head_errors(r['phi'], w, dq, r['q'], r['dw'])
  if qe > LAYER_TOL:
    missed.append('q')
  if dwe > LAYER_TOL:
    missed.append('dw')
  return missed


def sgd32(var, grad, lr):
  """tf.train.GradientDescentOptimizer in float32: the product rounded, then the difference."""
  var, grad = np.asarray(var, np.float32), np.asarray(grad, np.float32)
  out = var - np.float32(lr) * grad
  assert out.dtype == np.float32
  return out


def sgd64(var, grad, lr):
  return np.asarray(var, np.float64) - np.float64(np.float32(lr)) * np.asarray(grad, np.float64)
