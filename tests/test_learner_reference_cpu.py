"""The float64 reference of the loss kernels and its measure, checked without a GPU, over the
case table tests/test_gpu_learner_edges.py runs on the device (oracle/learner_cases.py):

* calibration: the oracle in fp32 (oracle/learner.py at dtype=np.float32 -- the kernels'
  arithmetic restated in numpy) passes the measure (oracle/nature_cnn.py cond_ratio, on the
  Σ|terms| of oracle/learner.py) against float64 with at least 3x to spare, for every output;
* the cases' own conditions hold on the float64 reference for every sample: the greedy
  margins, where the smallest replay probability sits, the exact ties, the exact Huber hits;
* power: each of eight subtly wrong restatements (what a subtly wrong kernel would compute)
  fails the measure on at least one case.
"""
import numpy as np
import pytest

from oracle import learner as L
from oracle import learner_cases as C
from oracle import nature_cnn as ONC

MARGIN = 3.0
f4 = np.float32


def _ratios(got, checks):
  return {k: float(ONC.cond_ratio(np.asarray(got[k], np.float64).reshape(np.shape(ref)), ref,
                                  terms).max())
          for k, (ref, terms) in checks.items()}


def _c51_table():
  """(id, case, probs?) of every C51 case the GPU test runs."""
  out = []
  for B, A, N in C.C51_SHAPES:
    for scale in C.SCALES:
      c = C.c51_case(B, A, N, scale)
      for probs in (True, False):
        out.append(('B%d-A%d-N%d-x%d-%s' % (B, A, N, scale, 'per' if probs else 'uni'), c, probs))
  out.append(('gamma0', C.c51_case(5, 3, 51, 2, cg=0.0), True))
  out.append(('all-terminal', C.c51_case(7, 2, 5, 2, all_terminal=True), True))
  out.append(('online-B513', C.c51_online_case(), True))
  out.append(('tie', C.c51_tie_case(), True))
  return out


def _c51_ratios(got, ref):
  checks = C.c51_checks(ref)
  checks['proj'] = (ref['proj'], ref['proj_abs'])
  return _ratios(got, checks)


# ---------------------------------------------------------------- the fp32 restatements
# L.c51_loss / L.iqn_loss / L.dqn_huber at float32, written out so that one step can be made
# wrong; without a mutation each is bitwise the oracle's (asserted below).
def _c51_f32(c, probs, mut=None):
  ol, tl, z = c['ol'], c['tl'], c['z']
  B, A, N = ol.shape
  rows = np.arange(B)
  term = np.zeros(B, f4) if mut == 'terminal ignored' else c['term'].astype(f4)
  gamma_t = f4(c['cg']) * (1 - term)
  tz = c['rew'][:, None] + gamma_t[:, None] * z[None, :]
  tp = L.softmax(tl)
  q = (tp * z).sum(-1)
  astar = A - 1 - q[:, ::-1].argmax(1) if mut == 'last max' else q.argmax(1)
  p = tp[rows, astar]
  dz = (z[-1] - z[0]) / f4(N) if mut == 'dz over N' else z[1] - z[0]
  clipped = np.clip(tz, z[0], z[-1])[:, None, :]
  quot = np.clip(1 - np.abs(clipped - z[None, :, None]) / dz, 0, 1)           # (B, i, j)
  if mut == 'source atom N-1 dropped':
    quot[:, :, N - 1] = 0
  if mut == 'run cut to 8 terms':
    quot = quot * (np.cumsum(quot > 0, axis=-1) <= 8)
  proj = (quot * p[:, None, :]).sum(-1).astype(f4)
  chosen = ol[rows, c['act']]
  sm = L.softmax(chosen)
  lse = np.log(np.exp(chosen - chosen.max(1, keepdims=True)).sum(1)) + chosen.max(1)
  loss = (proj * (lse[:, None] - chosen)).sum(1)
  if probs:
    w = 1.0 / np.sqrt(c['probs'] + f4(1e-10))
    w = w / (w[:64].max() if mut == 'PER max over 64' else w.max())
  else:
    w = np.ones(B, f4)
  grad = np.zeros_like(ol)
  grad[rows, c['act']] = (w / B)[:, None] * (sm - proj)
  return dict(loss=loss, grad=grad, proj=proj, priorities=np.sqrt(loss + f4(1e-10)),
              mean_loss=(w * loss).mean())


def _iqn_f32(c, kappa, mut=None):
  B, A, N, Np, K = (c[k] for k in ('B', 'A', 'N', 'Np', 'K'))
  rows = np.arange(B)
  astar = c['ta'].reshape(K, B, A).mean(0).argmax(1)
  gam = f4(c['cg']) * (1 - c['term'].astype(f4))
  T = (c['rew'][None, :] + gam[None, :] * c['tq'].reshape(Np, B, A)[:, rows, astar]).T
  theta = c['oq'].reshape(N, B, A)[:, rows, c['act']].T
  tau = c['tau'].reshape(N, B).T
  u = T[:, :, None] - theta[:, None, :]
  au = np.abs(u)
  lin = kappa * au if mut == 'Huber without the half kappa squared' else kappa * (au - 0.5 * kappa)
  hub = np.where(au <= kappa, 0.5 * u * u, lin)
  w = np.abs(tau[:, None, :] - (u < 0).astype(f4))
  loss = (w * hub / kappa).sum(2).mean(1)
  dh = np.where(au <= kappa, u, kappa * np.sign(u))
  dtheta = -(w * dh / (1.0 if mut == 'kappa missing from the gradient' else kappa)).sum(1) / Np / B
  grad = np.zeros_like(c['oq']).reshape(N, B, A)
  grad[:, rows, c['act']] = dtheta.T
  return dict(loss=loss, grad=grad.reshape(N * B, A), mean_loss=loss.mean())


def _iqn_table():
  out = [('B%d-A%d-N%d-Np%d-K%d-k%g' % (sh + (k,)), C.iqn_case(*sh), k)
         for sh in C.IQN_SHAPES for k in C.KAPPAS]
  out += [('dyadic-k%g' % k, C.iqn_dyadic_case(k), k) for k in C.KAPPAS]
  out.append(('tie', C.iqn_tie_case(), 1.0))
  return out


def _dqn_table():
  out = [('B%d-A%d-%s' % (B, A, 'dyadic' if d else 'randn'), C.dqn_case(B, A, dyadic=d))
         for B, A in C.DQN_SHAPES for d in (True, False)]
  out.append(('all-terminal', C.dqn_case(7, 64, all_terminal=True)))
  out.append(('gamma0', C.dqn_case(257, 4, cg=0.0)))
  return out


def test_the_bar_is_the_projects():
  assert ONC.COND_FLOOR == 1e-3 and ONC.LAYER_TOL == 1e-5


def test_restatements_are_the_oracle_in_fp32():
  for name, c, probs in _c51_table():
    a, b = _c51_f32(c, probs), C.c51_reference(c, probs, dtype=f4)
    for k in a:
      assert np.array_equal(a[k], b[k]), (name, k)
  for name, c, kappa in _iqn_table():
    a, b = _iqn_f32(c, kappa), C.iqn_reference(c, kappa, dtype=f4)
    for k in a:
      assert np.array_equal(a[k], b[k]), (name, k)


def test_fp32_oracle_passes_with_margin():
  worst = {}

  def note(kind, name, r):
    for k, v in r.items():
      assert v * MARGIN <= ONC.LAYER_TOL, '%s %s %s: %.3g is not %gx under %g' % (
          kind, name, k, v, MARGIN, ONC.LAYER_TOL)
      worst[kind, k] = max(worst.get((kind, k), 0.0), v)

  for name, c, probs in _c51_table():
    ref = C.c51_reference(c, probs)
    assert np.all(np.isfinite(ref['grad'])) and np.any(ref['grad'] != 0), name
    note('c51', name, _c51_ratios(C.c51_reference(c, probs, dtype=f4), ref))
  for name, c in _dqn_table():
    note('dqn', name, _ratios(C.dqn_reference(c, dtype=f4), C.dqn_checks(C.dqn_reference(c))))
  for name, c, kappa in _iqn_table():
    note('iqn', name, _ratios(C.iqn_reference(c, kappa, dtype=f4),
                              C.iqn_checks(C.iqn_reference(c, kappa))))
  for (kind, k), v in sorted(worst.items()):
    print('fp32 oracle, %s %s: worst ratio %.3g (%.0fx under the bar)' % (
        kind, k, v, ONC.LAYER_TOL / max(v, 1e-300)))


def test_greedy_margins_hold_for_every_sample():
  for name, c, _ in _c51_table():
    if name == 'tie':
      continue
    for dt in (np.float64, f4):
      assert C.q_margin(C.c51_target_q(c, dt)).min() >= 0.99 * C.MARGIN_C51, (name, dt)
    assert C.q_margin(C.c51_target_q(c)).min() >= C.MARGIN_C51, name
    assert np.array_equal(C.c51_reference(c, dtype=f4)['argmax'], C.c51_reference(c)['argmax']), name
  for name, c, kappa in _iqn_table():
    if name == 'tie':
      continue
    assert C.q_margin(C.iqn_kmean(c)).min() >= C.MARGIN_IQN, name


def test_rewards_terminals_and_probabilities_cover_the_edges():
  seen = set()
  for B, A, N in C.C51_SHAPES:
    both = set()
    for scale in C.SCALES:
      c = C.c51_case(B, A, N, scale)
      assert set(c['rew'].tolist()) <= set(f4(r) for r in C.REWARDS)
      seen |= set(c['rew'].tolist())
      out = np.abs(c['rew']) > C.VMAX
      edge = (np.abs(c['rew']) >= C.VMAX) & (c['term'] == 0)     # r + gamma z leaves the support
      both |= ({'terminal'} if np.any(out & (c['term'] == 1)) else set())
      both |= ({'running'} if np.any(edge) else set())
      if B >= 2:
        assert np.any(out & (c['term'] == 1)) and np.any(out & (c['term'] == 0)), (B, A, N)
      if B >= 30:
        assert 0.15 <= c['term'].mean() <= 0.45, (B, A, N, c['term'].mean())
      p = c['probs']
      if (B, A, N) == C.MIN_PROB_LAST:
        assert p.argmin() == 64 and p[64] < 0.5 * np.delete(p, 64).min()
      elif (B, A, N) == C.ZERO_PROB_SHAPE:
        assert p[40] == 0.0 and np.delete(p, 40).min() > 0.04
      else:
        assert p.min() > 0.04
    assert both == {'terminal', 'running'}, (B, A, N)
  assert seen == set(f4(r) for r in C.REWARDS)
  c = C.c51_online_case()
  assert c['B'] == 513 and c['probs'].argmin() >= 512
  # a Tz exactly on an atom and exactly on both edges, with gamma_t = 0 (terminal): r itself
  z = C.c51_case(5, 3, 51, 2)['z']
  assert f4(0.0) in z and z[0] == -10 and z[-1] == 10 and f4(2.5) not in z


def test_c51_tie_rows_are_exact_ties_with_different_projections():
  c = C.c51_tie_case()
  for dt in (f4, np.float64):
    q = C.c51_target_q(c, dt)
    assert q.dtype == dt and np.all(q == 0), q
  ref = C.c51_reference(c)
  assert np.array_equal(ref['argmax'], np.zeros(c['B'], int))
  first = [o[0] for o in C.TIE_ORDERS]
  last = [o[-1] for o in C.TIE_ORDERS]
  assert len(set(first)) >= 2 and all(a != b for a, b in zip(first, last))
  # the projection of any other row of a sample is far from the first one's
  for b in range(c['B']):
    for a in range(1, c['A']):
      alt = dict(c, tl=c['tl'][:, [a] * c['A']])
      other = C.c51_reference(alt)['proj'][b]
      r = ONC.cond_ratio(other, ref['proj'][b], ref['proj_abs'][b]).max()
      assert r > 100 * ONC.LAYER_TOL, (b, a, float(r))


def test_iqn_tie_and_dyadic_cases_hit_what_they_claim():
  c = C.iqn_tie_case()
  assert np.array_equal(c['ta'][:, 1], c['ta'][:, 3]) and not np.array_equal(c['tq'][:, 1], c['tq'][:, 3])
  ref = C.iqn_reference(c, 1.0)
  assert np.all(ref['argmax'] == 1)
  swapped = dict(c, tq=c['tq'][:, [0, 3, 2, 1, 4]])      # what taking column 3 would compute
  bad = C.iqn_reference(swapped, 1.0)
  assert _ratios(bad, C.iqn_checks(ref))['loss'] > 100 * ONC.LAYER_TOL
  for kappa in C.KAPPAS:
    c = C.iqn_dyadic_case(kappa)
    B, N, Np, A = c['B'], c['N'], c['Np'], c['A']
    ref = C.iqn_reference(c, kappa)
    gam = np.float64(c['cg']) * (1 - c['term'])
    T = c['rew'][None] + gam[None] * c['tq'].astype(np.float64).reshape(Np, B, A)[:, np.arange(B), ref['argmax']]
    theta = c['oq'].astype(np.float64).reshape(N, B, A)[:, np.arange(B), c['act']]
    u = T.T[:, :, None] - theta.T[:, None, :]
    assert np.any(u == 0) and np.any(u == kappa) and np.any(u == -kappa), kappa
    assert np.any(np.abs(u) > kappa) and np.any((np.abs(u) < kappa) & (u != 0)), kappa
    # and the fp32 oracle, exact on these inputs up to its last roundings
    assert _ratios(C.iqn_reference(c, kappa, dtype=f4), C.iqn_checks(ref))['grad'] < 1e-6


def test_dqn_dyadic_cases_hit_the_huber_corners():
  for B, A in C.DQN_SHAPES:
    c = C.dqn_case(B, A)
    ref = C.dqn_reference(c)
    err = c['oq'].astype(np.float64)[np.arange(B), c['act']] - ref['target']
    want = np.array(C.DQN_ERRS)[np.arange(B) % len(C.DQN_ERRS)]
    assert np.array_equal(err, want), (B, A)
    got = C.dqn_reference(c, dtype=f4)
    assert np.array_equal(got['loss'], ref['loss'])           # exact in fp32, and err / B rounds once
    assert np.array_equal(got['grad'], ref['grad'].astype(f4))
  errs = set(C.DQN_ERRS)
  assert {0.0, 1.0, -1.0} <= errs and any(0 < abs(e) < 1 for e in errs) and any(abs(e) > 1 for e in errs)


_C51_MUTATIONS = ('source atom N-1 dropped', 'run cut to 8 terms', 'last max', 'PER max over 64',
                  'terminal ignored', 'dz over N')
_IQN_MUTATIONS = ('kappa missing from the gradient', 'Huber without the half kappa squared')


@pytest.mark.parametrize('mut', _C51_MUTATIONS)
def test_a_subtly_wrong_c51_fails(mut):
  failed = []
  for name, c, probs in _c51_table():
    r = _c51_ratios(_c51_f32(c, probs, mut), C.c51_reference(c, probs))
    failed += ['%s %s %.3g' % (name, k, v) for k, v in r.items() if not v <= ONC.LAYER_TOL]
  print('%s: fails %d checks, e.g. %s' % (mut, len(failed), failed[:3]))
  assert failed, mut


@pytest.mark.parametrize('mut', _IQN_MUTATIONS)
def test_a_subtly_wrong_iqn_fails(mut):
  failed = []
  for name, c, kappa in _iqn_table():
    r = _ratios(_iqn_f32(c, kappa, mut), C.iqn_checks(C.iqn_reference(c, kappa)))
    failed += ['%s %s %.3g' % (name, k, v) for k, v in r.items() if not v <= ONC.LAYER_TOL]
  print('%s: fails %d checks, e.g. %s' % (mut, len(failed), failed[:3]))
  assert failed, mut


def test_uncentered_rmsprop_oracle_drops_the_mean_gradient():
  rs = np.random.RandomState(0)
  g = rs.randn(5).astype(f4)
  a = L.TF1CenteredRMSProp(5, 0.01, decay=0.9, momentum=0.9, eps=1e-5, centered=False)
  b = L.TF1CenteredRMSProp(5, 0.01, decay=0.9, momentum=0.9, eps=1e-5)
  va, vb = a.step(np.ones(5, f4), g), b.step(np.ones(5, f4), g)
  ms = f4(1) + (g * g - f4(1)) * f4(1 - f4(0.9))
  assert np.array_equal(va, np.ones(5, f4) - g * f4(0.01) / np.sqrt(ms + f4(1e-5)))
  assert np.all(a.mg == 0) and np.any(b.mg != 0) and not np.array_equal(va, vb)
