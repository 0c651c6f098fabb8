"""The float64 reference of dq_c51_loss and its measure on supports wider than a wave, checked
without a GPU over the case table tests/test_gpu_c51_wide.py runs on the device
(tests/c51_wide_cases.py), as tests/test_learner_reference_cpu.py does for up to 64 atoms:

* calibration: the oracle in fp32 passes the measure (oracle/nature_cnn.py cond_ratio at
  COND_FLOOR 1e-3 / LAYER_TOL 1e-5, on the Σ|terms| of oracle/learner_cases.py c51_checks)
  against float64 with at least 3x to spare, for every output and for the projection;
* the cases' own conditions: greedy margins, where the smallest probability sits, samples
  outside both supports, the exact ties;
* power: six restatements that each lose one chunk-sized piece of the arithmetic (what a
  kernel that mishandles a row wider than a wave would compute) fail the measure by at least
  100x the bar on at least one case;
* the 201-atom gym config reads into the reference's bindings.
"""
import os

import numpy as np
import pytest

from oracle import learner as L
from oracle import learner_cases as C
from oracle import nature_cnn as ONC
from tests import c51_wide_cases as W

MARGIN = 3.0
POWER = 100.0
f4 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GIN_201 = os.path.join(ROOT, 'dopamine_amd', 'agents', 'rainbow', 'configs', 'c51_cartpole_201.gin')


def _ratios(got, ref):
  checks = C.c51_checks(ref)
  checks['proj'] = (ref['proj'], ref['proj_abs'])
  return {k: float(ONC.cond_ratio(np.asarray(got[k], np.float64).reshape(np.shape(r)), r, t).max())
          for k, (r, t) in checks.items()}


def _table():
  return W.table() + [('tie', W.tie_case(), True)]


# L.c51_loss at float32, written out so that one step can be made wrong; without a mutation it
# is bitwise the oracle's (asserted below).
def _c51_f32(c, probs, mut=None):
  ol, tl, z = c['ol'], c['tl'], c['z']
  B, A, N = ol.shape
  rows = np.arange(B)
  gamma_t = f4(c['cg']) * (1 - c['term'].astype(f4))
  tz = c['rew'][:, None] + gamma_t[:, None] * z[None, :]
  if mut == 'softmax sum over the first 64 atoms':
    e = np.exp(tl - tl.max(axis=-1, keepdims=True))
    tp = e / e[..., :64].sum(axis=-1, keepdims=True)
  else:
    tp = L.softmax(tl)
  q = (tp * z)[..., :64].sum(-1) if mut == 'Q over the first 64 atoms' else (tp * z).sum(-1)
  astar = q[:, :16].argmax(1) if mut == 'greedy over the first 16 actions' else q.argmax(1)
  p = tp[rows, astar]
  dz = z[1] - z[0]
  clipped = np.clip(tz, z[0], z[-1])[:, None, :]
  quot = np.clip(1 - np.abs(clipped - z[None, :, None]) / dz, 0, 1)           # (B, i, j)
  if mut == 'source atoms from 192 on dropped':
    quot[:, :, 192:] = 0
  if mut == 'source atom 64 dropped':
    quot[:, :, 64] = 0
  proj = (quot * p[:, None, :]).sum(-1).astype(f4)
  chosen = ol[rows, c['act']]
  sm = L.softmax(chosen)
  lse = np.log(np.exp(chosen - chosen.max(1, keepdims=True)).sum(1)) + chosen.max(1)
  terms = proj * (lse[:, None] - chosen)
  if mut == 'loss without its last chunk':
    loss = terms[:, :(N - 1) // 64 * 64].sum(1)
  else:
    loss = terms.sum(1)
  if probs:
    w = 1.0 / np.sqrt(c['probs'] + f4(1e-10))
    w = w / w.max()
  else:
    w = np.ones(B, f4)
  grad = np.zeros_like(ol)
  grad[rows, c['act']] = (w / B)[:, None] * (sm - proj)
  return dict(loss=loss, grad=grad, proj=proj, priorities=np.sqrt(loss + f4(1e-10)),
              mean_loss=(w * loss).mean())


def test_the_bar_is_the_projects():
  assert ONC.COND_FLOOR == 1e-3 and ONC.LAYER_TOL == 1e-5


def test_the_table_is_the_issues():
  assert set(n for _, _, n in W.SHAPES) == {65, 128, 129, 201, 255, 256, 70}
  assert all(64 < n <= 256 and a <= 64 for _, a, n in W.SHAPES)
  assert len(W.table()) == len(W.SHAPES) * len(C.SCALES) * len(W.VMAXES) * 2 + 2
  assert W.DETERMINISM_SHAPE in W.SHAPES


def test_restatement_is_the_oracle_in_fp32():
  for name, c, probs in _table():
    a, b = _c51_f32(c, probs), C.c51_reference(c, probs, dtype=f4)
    for k in a:
      assert np.array_equal(a[k], b[k]), (name, k)


def test_fp32_oracle_passes_with_margin():
  worst = {}
  for name, c, probs in _table():
    ref = W.reference(name, c, probs)
    assert np.all(np.isfinite(ref['grad'])) and np.any(ref['grad'] != 0), name
    for k, v in _ratios(C.c51_reference(c, probs, dtype=f4), ref).items():
      assert v * MARGIN <= ONC.LAYER_TOL, '%s %s: %.3g is not %gx under %g' % (
          name, k, v, MARGIN, ONC.LAYER_TOL)
      worst[k] = max(worst.get(k, 0.0), v)
  for k, v in sorted(worst.items()):
    print('fp32 oracle, wide c51 %s: worst ratio %.3g' % (k, v))


def test_greedy_margins_hold_for_every_sample():
  smallest = np.inf
  for name, c, probs in W.table():
    m = C.q_margin(C.c51_target_q(c)).min()
    smallest = min(smallest, m)
    assert m >= C.MARGIN_C51, (name, m)
    assert C.q_margin(C.c51_target_q(c, f4)).min() >= 0.99 * C.MARGIN_C51, name
    assert np.array_equal(C.c51_reference(c, dtype=f4)['argmax'],
                          W.reference(name, c, probs)['argmax']), name
  print('smallest greedy margin %.3g' % smallest)


def test_rewards_terminals_and_probabilities_cover_the_edges():
  for B, A, N in W.SHAPES:
    for scale in C.SCALES:
      for vmax in W.VMAXES:
        c = W.case(B, A, N, scale, vmax)
        assert c['z'][0] == -vmax and c['z'][-1] == vmax and len(c['z']) == N
        if B >= 2:    # a terminal and a running sample outside the support
          assert c['term'][0] == 1 and c['term'][1] == 0
          assert c['rew'][0] > vmax and c['rew'][1] < -vmax
        p = c['probs']
        if (B, A, N) == W.MIN_PROB_LAST:
          assert p.argmin() == 64 and p[64] < 0.5 * np.delete(p, 64).min()
        else:
          assert p.min() > 0.04
  g0 = W.case(5, 3, 129, 2, 10.0, cg=0.0)
  assert g0['cg'] == 0 and np.any(g0['term'] == 0)
  at = W.case(7, 2, 70, 2, 10.0, all_terminal=True)
  assert np.all(at['term'] == 1)


def test_tie_rows_are_exact_ties_with_different_projections():
  c = W.tie_case()
  assert np.array_equal(c['z'], ((np.arange(129) - 64) / 4.0).astype(f4))
  for dt in (f4, np.float64):
    tp = L.softmax(np.asarray(c['tl'], dt))
    assert set(np.unique(tp).tolist()) == {0.0, 0.5, 1.0}
    q = C.c51_target_q(c, dt)
    assert q.dtype == dt and q.shape == (4, 3) and np.all(q == 0), q
  ref = C.c51_reference(c)
  assert np.array_equal(ref['argmax'], np.zeros(c['B'], int))
  first = [o[0] for o in C.TIE_ORDERS]
  last = [o[-1] for o in C.TIE_ORDERS]
  assert len(set(first)) >= 2 and all(a != b for a, b in zip(first, last))
  for b in range(c['B']):
    for a in range(1, c['A']):
      other = C.c51_reference(dict(c, tl=c['tl'][:, [a] * c['A']]))['proj'][b]
      r = ONC.cond_ratio(other, ref['proj'][b], ref['proj_abs'][b]).max()
      assert r > POWER * ONC.LAYER_TOL, (b, a, float(r))


MUTATIONS = ('softmax sum over the first 64 atoms', 'Q over the first 64 atoms',
             'greedy over the first 16 actions', 'source atoms from 192 on dropped',
             'source atom 64 dropped', 'loss without its last chunk')


@pytest.mark.parametrize('mut', MUTATIONS)
def test_a_kernel_that_loses_a_chunk_fails(mut):
  worst, where = 0.0, None
  with np.errstate(all='ignore'):
    for name, c, probs in W.table():
      r = _ratios(_c51_f32(c, probs, mut), W.reference(name, c, probs))
      for k, v in r.items():
        v = np.inf if not np.isfinite(v) else v
        if v > worst:
          worst, where = v, (name, k)
  print('%s: worst ratio %.3g at %s' % (mut, worst, where))
  assert worst >= POWER * ONC.LAYER_TOL, (mut, worst)


def test_gin_201_reads_the_reference_bindings():
  from dopamine_amd import gin_lite
  from dopamine_amd.agents import networks
  from dopamine_amd.discrete_domains import run_experiment
  gin_lite.clear_config()
  try:
    run_experiment.load_gin_configs([GIN_201], [])
    cls, kw = run_experiment._agent_kwargs('rainbow')
    assert cls.__name__ == 'RainbowAgent'
    assert kw['num_atoms'] == 201 and kw['vmax'] == 100.0
    assert kw['network'] is networks.CartpoleRainbowNetwork
    assert kw['observation_shape'] == (4, 1) and kw['stack_size'] == 1
    assert kw['replay_scheme'] == 'uniform' and kw['update_horizon'] == 1
    assert kw['gamma'] == 0.99 and kw['min_replay_history'] == 500
    assert kw['update_period'] == 1 and kw['target_update_period'] == 1
    assert kw['epsilon_train'] == 0.01 and kw['epsilon_eval'] == 0.0
    assert kw['epsilon_fn'] is run_experiment.dqn_agent.identity_epsilon
    assert kw['optimizer'].kwargs['learning_rate'] == 0.00001
    assert kw['optimizer'].kwargs['epsilon'] == 0.00000390625
    assert kw['replay_capacity'] == 50000 and kw['batch_size'] == 128
    assert gin_lite.query('create_gym_environment') == {'environment_name': 'CartPole',
                                                        'version': 'v0'}
    assert gin_lite.query('create_agent') == {'agent_name': 'rainbow'}
  finally:
    gin_lite.clear_config()
