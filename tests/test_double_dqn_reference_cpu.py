"""The double-DQN references and cases of tests/double_dqn_cases.py checked with the oracle
alone (no GPU): the references reduce to oracle.learner's plain ones when the select input is
the target's, every case has the property it was built for, and the measure the GPU test
asserts on (oracle/nature_cnn.py cond_ratio at LAYER_TOL) tells the double target from the
plain one on every selection-sensitive sample -- so a kernel that ignored its select input
would fail tests/test_gpu_double_dqn_loss.py by a wide margin.  Also the public surface that
needs no device: the constructors' double_dqn keyword and the two gin files.
"""
import inspect
import os

import numpy as np
import pytest

from oracle import learner as L
from oracle import learner_cases as C
from oracle import nature_cnn as ONC
from tests import double_dqn_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_C51 = D.c51_table()
_DQN = D.dqn_table()


def _same(a, b):
  assert set(a) == set(b), (sorted(a), sorted(b))
  for k in a:
    assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize('name,c,probs', _C51, ids=[t[0] for t in _C51])
def test_c51_double_reference_with_the_target_as_select_is_the_plain_one(name, c, probs):
  _same(D.c51_double_reference(c, probs, sl=c['tl']), C.c51_reference(c, probs))


@pytest.mark.parametrize('name,c,dyadic', _DQN, ids=[t[0] for t in _DQN])
def test_dqn_double_reference_with_the_target_as_select_is_the_plain_one(name, c, dyadic):
  ref = D.dqn_double_reference(c, sq=c['tq'])
  assert np.array_equal(ref.pop('argmax'), np.asarray(c['tq'], np.float64).argmax(1))
  _same(ref, C.dqn_reference(c))


@pytest.mark.parametrize('name,c,probs', _C51, ids=[t[0] for t in _C51])
def test_c51_case_conditions(name, c, probs):
  B, A, vmax = c['B'], c['A'], c['vmax']
  qs = D.select_q(c)
  assert float(C.q_margin(qs).min()) >= 1e-3 * vmax
  if A >= 2:
    assert not (qs.argmax(1) == C.c51_target_q(c).argmax(1)).any()
  if name not in D.COLD:
    assert D.sensitive(c, vmax).any()
    if B <= 3:
      assert c['term'][B - 1] == 0 and c['rew'][B - 1] == np.float32(0.4)
  if name == 'gamma0':
    assert float(c['cg']) == 0.0
  if name == 'all-terminal':
    assert c['term'].all()
  if name == 'B513' or (B, A, c['N']) == D.MIN_PROB_LAST:
    i = 512 if name == 'B513' else 64
    assert int(c['probs'].argmin()) == i and c['probs'][i] == np.float32(0.01)


def test_c51_table_covers_every_shape_scale_and_support():
  names = [t[0] for t in _C51]
  assert len(set(names)) == len(names)
  for B, A, N in D.C51_SHAPES:
    for scale in C.SCALES:
      for vmax in ((10, 100) if N > 64 else (10,)):
        for p in ('per', 'uni'):
          assert 'B%d-A%d-N%d-x%d-v%d-%s' % (B, A, N, scale, vmax, p) in names


@pytest.mark.parametrize('name,c,probs', _C51, ids=[t[0] for t in _C51])
def test_c51_measure_tells_the_double_target_from_the_plain_one(name, c, probs):
  """Power: on every selection-sensitive sample (A >= 2) the PLAIN reference's gradient
  misses the double reference by at least 100 x LAYER_TOL on grad_abs_proj."""
  if c['A'] < 2 or name in D.COLD:
    return
  ref, plain = D.c51_reference(name, c, probs), C.c51_reference(c, probs)
  r = ONC.cond_ratio(plain['grad'], ref['grad'], ref['grad_abs_proj'])
  r = r.reshape(c['B'], -1).max(1).values.numpy()
  s = D.sensitive(c, c['vmax'])
  print('%s: smallest miss %.3g x LAYER_TOL over %d samples' % (
      name, r[s].min() / ONC.LAYER_TOL, int(s.sum())))
  assert r[s].min() >= 100 * ONC.LAYER_TOL, (name, r[s].min())


@pytest.mark.parametrize('name,c,dyadic', _DQN, ids=[t[0] for t in _DQN])
def test_dqn_case_conditions_and_power(name, c, dyadic):
  B, A = c['B'], c['A']
  assert float(C.q_margin(c['sq']).min()) >= D.MARGIN_DQN
  ref = D.dqn_double_reference(c)
  if A >= 2:
    assert (c['tq'][np.arange(B), ref['argmax']] < c['tq'].max(1)).all()
  if name == 'all-terminal':
    assert c['term'].all()
    return
  if name == 'gamma0':
    assert float(c['cg']) == 0.0
    return
  s = D.sensitive(c)
  assert s.any()
  if dyadic:                       # err runs through DQN_ERRS exactly, on the double target
    err = c['oq'][np.arange(B), c['act']].astype(np.float64) - ref['target']
    assert np.array_equal(err, np.array(C.DQN_ERRS)[np.arange(B) % len(C.DQN_ERRS)])
  if A >= 2:                       # power, on the per-sample loss
    plain = C.dqn_reference(c)
    r = ONC.cond_ratio(plain['loss'], ref['loss'], ref['loss_abs']).numpy()
    assert r[s].min() >= 100 * ONC.LAYER_TOL, (name, r[s].min())


def test_tie_cases_tie_exactly_and_the_tied_actions_differ():
  c = D.c51_tie_case()
  assert np.array_equal(D.select_q(c), np.zeros((c['B'], c['A'])))
  assert np.array_equal(D.select_q(c, np.float32), np.zeros((c['B'], c['A']), np.float32))
  ref = D.c51_double_reference(c, False)
  assert np.array_equal(ref['argmax'], np.zeros(c['B'], np.int64))
  terms = ref['proj_abs'] + 1.0 / c['N']
  for a in range(1, c['A']):
    other = C.c51_reference(dict(c, tl=c['tl'][:, [a] * c['A']]), False)['proj']
    r = ONC.cond_ratio(other, ref['proj'], terms).reshape(c['B'], -1).max(1).values
    assert float(r.min()) > 100 * ONC.LAYER_TOL, (a, r)
  d = D.dqn_tie_case()
  first = d['sq'].argmax(1)
  for b in range(d['B']):
    tied = np.flatnonzero(d['sq'][b] == d['sq'][b].max())
    assert len(tied) >= 2 and tied[0] == first[b]
    assert len(set(d['tq'][b, tied])) == len(tied)       # every tied action a different target


def test_constructors_take_double_dqn():
  from dopamine_amd.agents.dqn.dqn_agent import DQNAgent
  from dopamine_amd.agents.implicit_quantile.implicit_quantile_agent import ImplicitQuantileAgent
  for cls in (DQNAgent, ImplicitQuantileAgent):
    p = inspect.signature(cls.__init__).parameters['double_dqn']
    assert p.default is False, cls


@pytest.mark.parametrize('path,cls,base', [
    ('dqn/configs/double_dqn_acrobot.gin', 'DQNAgent', 'dqn/configs/dqn_acrobot.gin'),
    ('rainbow/configs/double_rainbow_cartpole.gin', 'RainbowAgent',
     'rainbow/configs/rainbow_cartpole.gin')])
def test_gin_files_bind_the_flag_and_nothing_else_new(path, cls, base):
  from dopamine_amd import gin_lite
  from dopamine_amd.discrete_domains import gym_lib, run_experiment  # noqa: F401 (gin names)
  agents = os.path.join(ROOT, 'dopamine_amd', 'agents')
  got = {}
  for f in (path, base):
    gin_lite.clear_config()
    try:
      gin_lite.parse_config_files_and_bindings([os.path.join(agents, f)], [])
      plain = (bool, int, float, str, tuple, list)     # (an optimizer: its class will do)
      got[f] = {k: repr(v) if isinstance(v, plain) else getattr(v, '__name__', type(v).__name__)
                for k, v in gin_lite.query(cls).items()}
    finally:
      gin_lite.clear_config()
  assert got[path].pop('double_dqn') == 'True'
  assert 'double_dqn' not in got[base]
  assert got[path] == got[base]
