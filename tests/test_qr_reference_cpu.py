"""The quantile-regression loss's cases, reference and measure, proved on the CPU alone
(tests/qr_cases.py; the device kernel runs in tests/test_gpu_qr_loss.py).

  * the float64 reference is oracle.learner.iqn_loss on the reordered inputs, exactly;
  * every case has the property it was built for (greedy margins, a* off the target rows' own
    greedy action, where the smallest probability sits, exact ties, u exactly 0 and +-kappa);
  * the kernel's documented fp32 summation order stays under the project's bar (LAYER_TOL 1e-5
    at COND_FLOOR 1e-3, oracle.nature_cnn.cond_ratio) on every case, with margin;
  * eight subtly wrong kernels each miss the same assertion on at least one case;
  * the quantile_*.gin configs parse and bind QuantileAgent's arguments.
"""
import os

import numpy as np
import pytest

from oracle import learner as L
from oracle import learner_cases as C
from oracle import nature_cnn as ONC
from tests import qr_cases as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TABLE = Q.table()
_CASES = list({id(t[1]): t for t in _TABLE}.values())      # each case once


def _worst(got, ref):
  """name -> worst cond_ratio of a result (fp32 restatement or device) against a reference."""
  out = {}
  for k, (r, terms) in Q.qr_checks(ref).items():
    r = np.asarray(r, np.float64)
    g = np.asarray(got[k], np.float64).reshape(r.shape)
    assert np.isfinite(g).all(), k
    out[k] = float(ONC.cond_ratio(g, r, np.asarray(terms, np.float64)).max())
  return out


def _assert_under_bar(what, got, ref):
  """THE assertion of this module (and, through assert_layer_close, of the GPU module)."""
  worst = _worst(got, ref)
  for k, r in worst.items():
    assert r <= ONC.LAYER_TOL, '%s %s: ratio %.3g over %.1g' % (what, k, r, ONC.LAYER_TOL)
  return worst


def test_reference_is_iqn_loss_on_the_reordered_inputs():
  c = Q.qr_case(5, 3, 7, 2)
  B, A, N = c['B'], c['A'], c['N']
  for kappa in Q.KAPPAS:
    ref = Q.qr_reference(c, kappa, probs=False)
    oq = np.empty((N * B, A), np.float32)
    tq = np.empty((N * B, A), np.float32)
    ta = np.empty((N * B, A), np.float32)
    tau = np.empty(N * B, np.float64)
    for q in range(N):
      for b in range(B):
        oq[q * B + b], tq[q * B + b], ta[q * B + b] = c['ol'][b, :, q], c['tl'][b, :, q], c['sl'][b, :, q]
        tau[q * B + b] = (q + 0.5) / N
    r = L.iqn_loss(oq, tq, ta, tau, c['act'], c['rew'], c['term'], c['cg'], kappa=kappa)
    assert np.array_equal(ref['loss'], r['loss'])
    assert np.array_equal(ref['loss_abs'], r['loss_abs'])
    assert np.array_equal(ref['argmax'], r['argmax'])
    for q in range(N):
      for b in range(B):
        assert np.array_equal(ref['grad'][b, :, q], r['grad'][q * B + b])
        assert np.array_equal(ref['grad_abs'][b, :, q], r['grad_abs'][q * B + b])
    # the PER rule and the priorities are dq_c51_loss's
    per = Q.qr_reference(c, kappa, probs=True)
    w = 1.0 / np.sqrt(c['probs'].astype(np.float64) + 1e-10)
    w = w / w.max()
    assert np.array_equal(per['loss'], ref['loss'])
    assert np.array_equal(per['grad'], ref['grad'] * w[:, None, None])
    assert np.array_equal(per['priorities'], np.sqrt(ref['loss'] + 1e-10))
    assert np.array_equal(per['prio_abs'], ref['loss_abs'] / (2 * per['priorities']))
    assert per['mean_loss'] == (w * ref['loss']).mean()


def test_definition_by_hand_on_one_sample():
  """loss_b = sum_i (1/N) sum_j |tau_i - 1{u < 0}| L_kappa(u_bij) / kappa, spelled out."""
  c = Q.qr_case(5, 3, 7, 10)
  N, kappa = c['N'], 2.0
  ref = Q.qr_reference(c, kappa, probs=False)
  for b in range(c['B']):
    a = int(c['sl'][b].astype(np.float64).mean(-1).argmax())
    y = float(c['rew'][b]) + float(c['cg']) * (1 - int(c['term'][b])) * c['tl'][b, a].astype(np.float64)
    th = c['ol'][b, c['act'][b]].astype(np.float64)
    tot = 0.0
    for i in range(N):
      for j in range(N):
        u = y[j] - th[i]
        hub = 0.5 * u * u if abs(u) <= kappa else kappa * (abs(u) - 0.5 * kappa)
        tot += abs((i + 0.5) / N - (1.0 if u < 0 else 0.0)) * hub / kappa / N
    assert abs(tot - ref['loss'][b]) <= 1e-12 * max(1.0, abs(tot))


@pytest.mark.parametrize('name,c,kappa,probs', _CASES, ids=[t[0] for t in _CASES])
def test_cases_have_the_properties_they_were_built_for(name, c, kappa, probs):
  B, A = c['B'], c['A']
  q = Q.select_means(c['sl'])
  assert (C.q_margin(q) >= np.array([Q.margin_floor(q[b]) for b in range(B)])).all()
  ref = Q.qr_reference(c, kappa, probs)
  assert np.array_equal(ref['argmax'], q.argmax(1))
  if A >= 2:
    assert (ref['argmax'] != Q.select_means(c['tl']).argmax(1)).all()
  own = Q.qr_reference(c, kappa, probs, sl='target')
  assert np.array_equal(own['argmax'], Q.select_means(c['tl']).argmax(1))   # S = T: T's own action


def test_smallest_probabilities_sit_where_the_cases_say():
  c = Q.qr_case(*Q.MIN_PROB_AT_64, 2)
  assert int(c['probs'].argmin()) == 64
  B, A, N = Q.STRIDED
  assert int(Q.qr_case(B, A, N, 2, probs_variant='min64')['probs'].argmin()) == 64
  assert int(Q.qr_case(B, A, N, 10, probs_variant='min512')['probs'].argmin()) == 512
  z = Q.qr_case(B, A, N, 2, probs_variant='zero')['probs']
  assert (z == 0).sum() == 1 and z.min() == 0 and int(z.argmin()) >= 256
  assert np.isfinite(Q.qr_reference(Q.qr_case(B, A, N, 2, probs_variant='zero'))['grad']).all()


@pytest.mark.parametrize('kappa', Q.KAPPAS)
def test_dyadic_case_hits_zero_and_both_kinks_and_is_exact_in_fp32(kappa):
  c = Q.dyadic_case(kappa)
  u = Q.dyadic_u(c)
  assert (u == 0).any() and (u == kappa).any() and (u == -kappa).any()
  assert (np.abs(u) > kappa).any() and ((np.abs(u) < kappa) & (u != 0)).any()
  ref = Q.qr_reference(c, kappa, probs=False)
  got = Q.qr_fp32(c, kappa, probs=False)
  assert np.array_equal(got['loss'].astype(np.float64), ref['loss'])
  assert np.array_equal(got['grad'].astype(np.float64), ref['grad'])
  assert (ref['argmax'] == 1).all()


def test_tie_case_ties_exactly_and_the_first_index_is_far_from_the_others():
  c = Q.tie_case()
  B = c['B']
  tied = Q.tied_actions(c)
  q32 = Q._row_sum(c['sl']) / np.float32(c['N'])
  assert np.array_equal(q32.astype(np.float64), Q.select_means(c['sl']))     # exact in both
  assert [int(t[0]) for t in tied] == list(Q.TIE_FIRST) and all(len(t) == 3 for t in tied)
  ref = Q.qr_reference(c, 1.0, False)
  assert list(ref['argmax']) == list(Q.TIE_FIRST)
  _assert_under_bar('tie', Q.qr_fp32(c, 1.0, False), ref)
  for b in range(B):
    for a in tied[b][1:]:
      sl = c['sl'].copy()
      sl[b, a] += 1.0                     # the reference with that other row taken
      other = Q.qr_reference(c, 1.0, False, sl=sl)
      r = ONC.cond_ratio(ref['grad'], other['grad'], ref['grad_abs']).reshape(B, -1).max(1).values
      assert float(r[b]) > 100 * ONC.LAYER_TOL, (b, a, r)


WORST = {}


@pytest.mark.parametrize('name,c,kappa,probs', _TABLE, ids=[t[0] for t in _TABLE])
def test_fp32_restatement_in_the_kernels_order_is_under_the_bar(name, c, kappa, probs):
  worst = _assert_under_bar(name, Q.qr_fp32(c, kappa, probs), Q.reference(name, c, kappa, probs))
  for k, r in worst.items():
    if r > WORST.get(k, (0.0, ''))[0]:
      WORST[k] = (r, name)
  print(name, {k: '%.3g' % v for k, v in worst.items()})


def test_fp32_restatement_keeps_a_threefold_margin():
  """Over the whole table (filled by the test above; computed here when run alone)."""
  if not WORST:
    for name, c, kappa, probs in _TABLE:
      for k, r in _worst(Q.qr_fp32(c, kappa, probs), Q.reference(name, c, kappa, probs)).items():
        if r > WORST.get(k, (0.0, ''))[0]:
          WORST[k] = (r, name)
  print('worst ratios:', {k: ('%.3g' % v[0], v[1]) for k, v in WORST.items()})
  for k, (r, name) in WORST.items():
    assert 3 * r <= ONC.LAYER_TOL, (k, r, name)


def _variant_cases():
  """The table's cases plus the tie case (the only one a last-max rule can miss)."""
  tie = Q.tie_case()
  return [(n, c, k, p, Q.reference(n, c, k, p)) for n, c, k, p in _TABLE if k == 1.0] + [
      ('tie', tie, 1.0, True, Q.qr_reference(tie, 1.0, True))]


@pytest.mark.parametrize('wrong', Q.WRONG)
def test_a_wrong_kernel_misses_the_bar(wrong):
  """Each wrong variant of the fp32 restatement fails _assert_under_bar on at least one case
  (and the right restatement passes every one of them: the tests above)."""
  first = None
  for name, c, kappa, probs, ref in _variant_cases():
    try:
      _assert_under_bar(name, Q.qr_fp32(c, kappa, probs, wrong=wrong), ref)
    except AssertionError:
      got = _worst(Q.qr_fp32(c, kappa, probs, wrong=wrong), ref)
      first = (name, {k: '%.3g' % v for k, v in got.items()})
      break
  print(wrong, 'first failing case:', first)
  assert first is not None, '%s passes every case' % wrong


@pytest.mark.parametrize('config,net,max_steps', [
    ('quantile_cartpole', 'CartpoleRainbowNetwork', 200),
    ('double_quantile_cartpole', 'CartpoleRainbowNetwork', 200),
    ('quantile_acrobot', 'AcrobotRainbowNetwork', 500)])
def test_quantile_configs_parse_and_bind_the_agents_arguments(config, net, max_steps):
  from dopamine_amd import gin_lite
  path = os.path.join(ROOT, 'dopamine_amd', 'agents', 'quantile', 'configs', config + '.gin')
  saved = dict(gin_lite._bindings)
  try:
    gin_lite.clear_config()
    from dopamine_amd.discrete_domains import run_experiment     # registers the references
    gin_lite.parse_config_files_and_bindings([path], [])
    cls, kw = run_experiment._agent_kwargs('quantile')
    assert cls.__name__ == 'QuantileAgent'
    assert kw['num_atoms'] == 200 and kw['kappa'] == 1.0 and 'vmax' not in kw
    assert kw['network'].__name__ == net
    assert kw['update_horizon'] == 3 and kw['replay_scheme'] == 'prioritized'
    assert kw['batch_size'] == 128 and kw['replay_capacity'] == 50000
    assert bool(kw.get('double_dqn', False)) == config.startswith('double')
    assert not any(param == 'vmax' for _, param in gin_lite._bindings)
    assert kw['optimizer'].kwargs['learning_rate'] == 0.09
    assert kw['optimizer'].kwargs['epsilon'] == 0.0003125
    assert gin_lite.query('create_agent')['agent_name'] == 'quantile'
    assert gin_lite.query('Runner')['max_steps_per_episode'] == max_steps
  finally:
    gin_lite.clear_config()
    gin_lite._bindings.update(saved)
