"""The classic-control domains without a GPU: the four C51 / Rainbow gym configs as gin_lite
reads them into the agent's arguments, the networks' parameter counts, and Acrobot-v1's
dynamics against known answers and an RK4 step written here from the published equations."""
import math
import os

import numpy as np
import pytest

from dopamine_amd import gin_lite
from dopamine_amd.agents import networks
from dopamine_amd.discrete_domains import gym_lib
from dopamine_amd.discrete_domains import run_experiment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, 'dopamine_amd', 'agents', 'rainbow', 'configs')

# file -> network, observation shape, replay scheme, update horizon, learning rate, epsilon
_GIN = {
    'c51_cartpole.gin': (networks.CartpoleRainbowNetwork, (4, 1), 'uniform', 1, 0.00001,
                         0.00000390625, 'CartPole', 'v0'),
    'rainbow_cartpole.gin': (networks.CartpoleRainbowNetwork, (4, 1), 'prioritized', 3, 0.09,
                             0.0003125, 'CartPole', 'v0'),
    'c51_acrobot.gin': (networks.AcrobotRainbowNetwork, (6, 1), 'uniform', 1, 0.1, 0.0003125,
                        'Acrobot', 'v1'),
    'rainbow_acrobot.gin': (networks.AcrobotRainbowNetwork, (6, 1), 'prioritized', 3, 0.09,
                            0.0003125, 'Acrobot', 'v1'),
}


@pytest.fixture
def clean_gin():
  gin_lite.clear_config()
  yield
  gin_lite.clear_config()


@pytest.mark.parametrize('name', sorted(_GIN))
def test_gin_subset_reads_the_gym_configs(clean_gin, name):
  net, shape, scheme, horizon, lr, eps, env, version = _GIN[name]
  run_experiment.load_gin_configs([os.path.join(CONFIGS, name)], [])
  cls, kw = run_experiment._agent_kwargs('rainbow')
  assert cls.__name__ == 'RainbowAgent'
  assert kw['network'] is net
  assert kw['observation_shape'] == shape
  assert kw['observation_dtype'] is np.float64
  assert kw['stack_size'] == 1
  assert kw['num_atoms'] == 51
  assert kw['replay_scheme'] == scheme
  assert kw['update_horizon'] == horizon
  assert kw['optimizer'].kwargs['learning_rate'] == lr
  assert kw['optimizer'].kwargs['epsilon'] == eps
  assert kw['replay_capacity'] == 50000 and kw['batch_size'] == 128
  assert kw['epsilon_fn'] is run_experiment.dqn_agent.identity_epsilon
  assert gin_lite.query('create_gym_environment') == {'environment_name': env, 'version': version}
  assert gin_lite.query('create_agent') == {'agent_name': 'rainbow'}


def test_acrobot_environment_and_constants():
  env = gym_lib.create_gym_environment('Acrobot', 'v1')
  assert env.action_space.n == 3
  ob = env.reset()
  assert ob.shape == (6,) and ob.dtype == np.float64
  assert env.observation_space.shape == (6,)
  assert 'Acrobot-v1' in gym_lib._ENVS and 'CartPole-v0' in gym_lib._ENVS
  assert gym_lib.ACROBOT_OBSERVATION_SHAPE == (6, 1)
  assert gym_lib.ACROBOT_OBSERVATION_DTYPE is np.float64 and gym_lib.ACROBOT_STACK_SIZE == 1
  assert np.array_equal(gym_lib.ACROBOT_MIN_VALS, [-1, -1, -1, -1, -5, -5])
  assert np.array_equal(gym_lib.ACROBOT_MAX_VALS, [1, 1, 1, 1, 5, 5])
  assert gin_lite._lookup_ref('gym_lib.cartpole_rainbow_network') is networks.CartpoleRainbowNetwork
  assert gin_lite._lookup_ref('gym_lib.acrobot_dqn_network') is networks.AcrobotDQNNetwork
  assert gin_lite._lookup_ref('gym_lib.acrobot_rainbow_network') is networks.AcrobotRainbowNetwork
  assert gin_lite._lookup_ref('gym_lib.cartpole_dqn_network') is networks.CartpoleDQNNetwork
  with pytest.raises(ValueError):
    gym_lib.create_gym_environment('Acrobot', 'v0')


def test_network_parameter_counts():
  mk = lambda cls, *a, **k: cls(*a, device='cpu', **k)
  assert mk(networks.CartpoleRainbowNetwork, 2, num_atoms=51, stack_size=1).fp.count() == 317542
  assert mk(networks.AcrobotRainbowNetwork, 3, num_atoms=51, stack_size=1).fp.count() == 344729
  assert mk(networks.AcrobotDQNNetwork, 3).fp.count() == 267779
  assert mk(networks.CartpoleDQNNetwork, 2).fp.count() == 4 * 512 + 512 + 512 * 512 + 512 + 2 * 512 + 2
  small = mk(networks.AcrobotDQNNetwork, 3, network_size=(24, 24))
  assert small.fp.count() == 6 * 24 + 24 + 24 * 24 + 24 + 3 * 24 + 3
  # logits (B, A, N) / Q (B, A), zero biases, the same init stream as before for config 1
  import torch
  x = torch.zeros(5, 1, 6, 1, dtype=torch.float64)
  assert tuple(mk(networks.AcrobotRainbowNetwork, 3)(x).shape) == (5, 3, 51)
  assert tuple(small(x).shape) == (5, 3)
  assert float(small.fp['fc0_b'].detach().abs().max()) == 0.0
  for cls in (networks.CartpoleDQNNetwork, networks.CartpoleRainbowNetwork,
              networks.AcrobotDQNNetwork, networks.AcrobotRainbowNetwork):
    assert issubclass(cls, networks.BasicDiscreteDomainNetwork)


# ---- Acrobot-v1: the published "book" equations, written here independently
def _deriv(s, a):
  th1, th2, w1, w2 = s
  m1 = m2 = l1 = 1.0
  lc1 = lc2 = 0.5
  I1 = I2 = 1.0
  g = 9.8
  d1 = m1 * lc1 * lc1 + m2 * (l1 * l1 + lc2 * lc2 + 2.0 * l1 * lc2 * np.cos(th2)) + I1 + I2
  d2 = m2 * (lc2 * lc2 + l1 * lc2 * np.cos(th2)) + I2
  phi2 = m2 * lc2 * g * np.cos(th1 + th2 - np.pi / 2.0)
  phi1 = (-m2 * l1 * lc2 * w2 * w2 * np.sin(th2) - 2.0 * m2 * l1 * lc2 * w2 * w1 * np.sin(th2)
          + (m1 * lc1 + m2 * l1) * g * np.cos(th1 - np.pi / 2.0) + phi2)
  a2 = (a + d2 / d1 * phi1 - m2 * l1 * lc2 * w1 * w1 * np.sin(th2) - phi2) / (
      m2 * lc2 * lc2 + I2 - d2 * d2 / d1)
  a1 = -(d2 * a2 + phi1) / d1
  return np.array([w1, w2, a1, a2])


def _rk4_step(s, a, dt=0.2):
  s = np.asarray(s, dtype=np.float64)
  k1 = _deriv(s, a)
  k2 = _deriv(s + 0.5 * dt * k1, a)
  k3 = _deriv(s + 0.5 * dt * k2, a)
  k4 = _deriv(s + dt * k3, a)
  n = s + (dt / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
  for i in (0, 1):
    n[i] = (n[i] + np.pi) % (2.0 * np.pi) - np.pi
  n[2] = np.clip(n[2], -4.0 * np.pi, 4.0 * np.pi)
  n[3] = np.clip(n[3], -9.0 * np.pi, 9.0 * np.pi)
  return n


def _env(state):
  e = gym_lib.AcrobotEnv(seed=0)
  e.reset()
  e.state = np.array(state, dtype=np.float64)
  return e


def test_acrobot_rest_state_stays_at_rest():
  """State 0 under torque 0 is an equilibrium.  The model writes gravity's moment arm as
  cos(theta - pi/2), which is 6.1e-17, not 0, at theta = 0 in float64, so "stays" means to
  within 1e-15 (ten times that residual times g dt)."""
  e = _env([0, 0, 0, 0])
  ob, reward, terminal, _ = e.step(1)
  assert np.allclose(e.state, 0.0, rtol=0, atol=1e-15)
  assert np.allclose(ob, [1, 0, 1, 0, 0, 0], rtol=0, atol=1e-15)
  assert reward == -1.0 and terminal is False


def test_acrobot_mirror_symmetry():
  for s, a in (([0.3, -0.7, 1.1, -2.0], 0), ([1.5, 0.4, -0.2, 0.9], 2), ([-2.0, 2.5, 3.0, 1.0], 1)):
    e, m = _env(s), _env([-v for v in s])
    e.step(a)
    m.step(2 - a)
    assert np.allclose(m.state, -e.state, rtol=0, atol=1e-12)


def test_acrobot_terminal_condition_and_reward():
  # the tip's height is -cos(th1) - cos(th1 + th2): hanging -2, upright +2, terminal above 1
  e = _env([math.pi, 0, 0, 0])          # upright and (unstably) at rest: still above 1 after a step
  ob, reward, terminal, _ = e.step(1)
  assert terminal is True and reward == 0.0
  assert -math.cos(e.state[0]) - math.cos(e.state[0] + e.state[1]) > 1.0
  e = _env([math.pi / 2, 0, 0, 0])      # horizontal: height 0
  ob, reward, terminal, _ = e.step(1)
  assert terminal is False and reward == -1.0
  # exactly the boundary value is not terminal (strict >)
  e = _env([0, 0, 0, 0])
  e.state = np.array([math.pi / 2, math.pi / 2, 0.0, 0.0])     # -cos(pi/2) - cos(pi) = 1 - 6e-17
  assert e._terminal() is False
  e.state = np.array([2.0, 0.0, 0.0, 0.0])                     # -2 cos(2) = 0.83
  assert e._terminal() is False
  e.state = np.array([2.2, 0.0, 0.0, 0.0])                     # -2 cos(2.2) = 1.18
  assert e._terminal() is True


def test_acrobot_velocity_clip_and_angle_wrap():
  def unclipped(state, torque, dt=0.2):
    y = np.asarray(state, dtype=np.float64)
    k1 = _deriv(y, torque)
    k2 = _deriv(y + 0.5 * dt * k1, torque)
    k3 = _deriv(y + 0.5 * dt * k2, torque)
    k4 = _deriv(y + dt * k3, torque)
    return y + (dt / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)

  top = [0.0, 0.0, 4 * math.pi, 9 * math.pi]           # at both caps and speeding up
  raw = unclipped(top, 1.0)
  assert raw[2] > 4 * math.pi and raw[3] > 9 * math.pi and raw[0] > math.pi and raw[1] > math.pi
  e = _env(top)
  e.step(2)
  assert e.state[2] == 4 * math.pi and e.state[3] == 9 * math.pi        # clipped exactly
  assert -math.pi <= e.state[0] <= math.pi and -math.pi <= e.state[1] <= math.pi
  assert np.allclose(e.state, _rk4_step(top, 1.0), rtol=0, atol=1e-12)
  low = [0.0, -1.0, 0.0, -9 * math.pi]                 # the lower cap of the first velocity
  raw = unclipped(low, -1.0)
  assert raw[2] < -4 * math.pi and -9 * math.pi < raw[3] < 9 * math.pi
  e = _env(low)
  e.step(0)
  assert e.state[2] == -4 * math.pi and e.state[3] == raw[3]            # inside: untouched
  # the wrap keeps a value inside [-pi, pi] as it is and brings others in by whole turns
  assert gym_lib._wrap(math.pi, -math.pi, math.pi) == math.pi
  assert gym_lib._wrap(-math.pi, -math.pi, math.pi) == -math.pi
  assert abs(gym_lib._wrap(math.pi + 0.25, -math.pi, math.pi) - (-math.pi + 0.25)) < 1e-15
  assert abs(gym_lib._wrap(-3 * math.pi - 0.5, -math.pi, math.pi) - (math.pi - 0.5)) < 1e-14


def test_acrobot_seeded_resets():
  a, b = gym_lib.AcrobotEnv(seed=7), gym_lib.AcrobotEnv(seed=7)
  for _ in range(3):
    oa, ob = a.reset(), b.reset()
    assert np.array_equal(oa, ob) and np.array_equal(a.state, b.state)
    assert a.state.shape == (4,) and bool((np.abs(a.state) <= 0.1).all())
  c = gym_lib.AcrobotEnv(seed=8)
  assert not np.array_equal(c.reset(), gym_lib.AcrobotEnv(seed=7).reset())
  c.seed(7)
  assert np.array_equal(c.reset(), gym_lib.AcrobotEnv(seed=7).reset())
  want = np.random.RandomState(7).uniform(low=-0.1, high=0.1, size=(4,))
  assert np.array_equal(gym_lib.AcrobotEnv(seed=7).reset()[4:], want[2:])


@pytest.mark.parametrize('state,action', (([0.05, -0.08, 0.02, 0.07], 0),
                                          ([1.2, -2.3, 3.5, -6.0], 2),
                                          ([-2.9, 0.6, -7.0, 11.0], 1)))
def test_acrobot_step_matches_an_independent_rk4(state, action):
  e = _env(state)
  ob, reward, terminal, _ = e.step(action)
  want = _rk4_step(state, (-1.0, 0.0, 1.0)[action])
  assert np.allclose(e.state, want, rtol=0, atol=1e-12)
  assert np.allclose(ob, [np.cos(want[0]), np.sin(want[0]), np.cos(want[1]), np.sin(want[1]),
                          want[2], want[3]], rtol=0, atol=1e-12)
  assert terminal == bool(-np.cos(want[0]) - np.cos(want[0] + want[1]) > 1.0)
  assert reward == (0.0 if terminal else -1.0)
