"""Gym-domain plumbing for the classic-control configs (reference
dopamine/discrete_domains/gym_lib.py).

``gym`` is not installed (third-party, not vendored by the reference), so
CartPole-v0 is restated here from gym's published classic-control model
(gym/envs/classic_control/cartpole.py, the version Dopamine 2.0 used): Euler
integration, tau 0.02 s, force 10 N, masses 1.0 / 0.1 kg, pole half-length
0.5 m; the episode ends when |x| > 2.4 or |theta| > 12 degrees; reward 1 per
step; reset draws the 4 state variables from U(-0.05, 0.05).  As in
``create_gym_environment`` (gym_lib.py:54-72) there is no TimeLimit wrapper: the
Runner's ``max_steps_per_episode`` caps episodes.

Acrobot-v1 likewise (gym/envs/classic_control/acrobot.py): two links of length 1, mass 1,
centre of mass 0.5 and moment of inertia 1 under g = 9.8, the "book" equations of motion,
torque -1 / 0 / +1 on the joint between the links with no noise, one classical Runge-Kutta
step over dt = 0.2, the angles wrapped to [-pi, pi] and the velocities clipped to +-4 pi and
+-9 pi; the episode ends when the tip is above the bar by one link length; reward -1 per
step, 0 on the terminal one; reset draws the 4 state variables from U(-0.1, 0.1).
"""
import math

import numpy as np

from dopamine_amd import gin_lite
from dopamine_amd.agents import networks

CARTPOLE_MIN_VALS = networks.CartpoleDQNNetwork.MIN
CARTPOLE_MAX_VALS = networks.CartpoleDQNNetwork.MAX
CARTPOLE_OBSERVATION_SHAPE = (4, 1)
CARTPOLE_OBSERVATION_DTYPE = np.float64
CARTPOLE_STACK_SIZE = 1
for _n in ('CARTPOLE_OBSERVATION_SHAPE', 'CARTPOLE_OBSERVATION_DTYPE', 'CARTPOLE_STACK_SIZE'):
  gin_lite.constant('gym_lib.' + _n, globals()[_n])

ACROBOT_MIN_VALS = networks.AcrobotDQNNetwork.MIN
ACROBOT_MAX_VALS = networks.AcrobotDQNNetwork.MAX
ACROBOT_OBSERVATION_SHAPE = (6, 1)
ACROBOT_OBSERVATION_DTYPE = np.float64
ACROBOT_STACK_SIZE = 1
for _n in ('ACROBOT_OBSERVATION_SHAPE', 'ACROBOT_OBSERVATION_DTYPE', 'ACROBOT_STACK_SIZE'):
  gin_lite.constant('gym_lib.' + _n, globals()[_n])

# the networks the gin files bind with @gym_lib.<name> (gym_lib.py:113-132, 227-252, 255-273,
# 295-317): the classes themselves
cartpole_dqn_network = gin_lite.register('gym_lib.cartpole_dqn_network',
                                         networks.CartpoleDQNNetwork)
cartpole_rainbow_network = gin_lite.register('gym_lib.cartpole_rainbow_network',
                                             networks.CartpoleRainbowNetwork)
acrobot_dqn_network = gin_lite.register('gym_lib.acrobot_dqn_network', networks.AcrobotDQNNetwork)
acrobot_rainbow_network = gin_lite.register('gym_lib.acrobot_rainbow_network',
                                            networks.AcrobotRainbowNetwork)
# the Fourier-basis networks (gym_lib.py:209-224, 276-292)
cartpole_fourier_dqn_network = gin_lite.register('gym_lib.cartpole_fourier_dqn_network',
                                                 networks.CartpoleFourierDQNNetwork)
acrobot_fourier_dqn_network = gin_lite.register('gym_lib.acrobot_fourier_dqn_network',
                                                networks.AcrobotFourierDQNNetwork)


class Discrete(object):
  def __init__(self, n):
    self.n = n

  def sample(self, rng=np.random):
    return int(rng.randint(self.n))


class Box(object):
  def __init__(self, low, high, dtype=np.float64):
    self.low, self.high, self.dtype = np.asarray(low), np.asarray(high), dtype
    self.shape = self.low.shape


class CartPoleEnv(object):
  """CartPole-v0 dynamics (gym classic control, Euler integrator)."""

  gravity = 9.8
  masscart = 1.0
  masspole = 0.1
  total_mass = masspole + masscart
  length = 0.5                          # half the pole's length
  polemass_length = masspole * length
  force_mag = 10.0
  tau = 0.02
  theta_threshold_radians = 12 * 2 * math.pi / 360
  x_threshold = 2.4

  def __init__(self, seed=None):
    high = np.array([self.x_threshold * 2, np.finfo(np.float32).max,
                     self.theta_threshold_radians * 2, np.finfo(np.float32).max])
    self.action_space = Discrete(2)
    self.observation_space = Box(-high, high)
    self.reward_range = (-float('inf'), float('inf'))
    self.metadata = {'render.modes': []}
    self.np_random = np.random.RandomState(seed)
    self.state = None
    self.steps_beyond_done = None

  def seed(self, seed=None):
    self.np_random = np.random.RandomState(seed)
    return [seed]

  def reset(self):
    self.state = self.np_random.uniform(low=-0.05, high=0.05, size=(4,))
    self.steps_beyond_done = None
    return np.array(self.state)

  def step(self, action):
    assert action in (0, 1), '%r invalid' % (action,)
    x, x_dot, theta, theta_dot = self.state
    force = self.force_mag if action == 1 else -self.force_mag
    costheta, sintheta = math.cos(theta), math.sin(theta)
    temp = (force + self.polemass_length * theta_dot * theta_dot * sintheta) / self.total_mass
    thetaacc = (self.gravity * sintheta - costheta * temp) / (
        self.length * (4.0 / 3.0 - self.masspole * costheta * costheta / self.total_mass))
    xacc = temp - self.polemass_length * thetaacc * costheta / self.total_mass
    x = x + self.tau * x_dot
    x_dot = x_dot + self.tau * xacc
    theta = theta + self.tau * theta_dot
    theta_dot = theta_dot + self.tau * thetaacc
    self.state = (x, x_dot, theta, theta_dot)
    done = bool(x < -self.x_threshold or x > self.x_threshold or
                theta < -self.theta_threshold_radians or theta > self.theta_threshold_radians)
    if not done:
      reward = 1.0
    elif self.steps_beyond_done is None:   # the pole just fell
      self.steps_beyond_done = 0
      reward = 1.0
    else:
      self.steps_beyond_done += 1
      reward = 0.0
    return np.array(self.state), reward, done, {}


class AcrobotEnv(object):
  """Acrobot-v1 dynamics (gym classic control, "book" equations, RK4)."""

  dt = 0.2
  LINK_LENGTH_1 = 1.0
  LINK_LENGTH_2 = 1.0
  LINK_MASS_1 = 1.0
  LINK_MASS_2 = 1.0
  LINK_COM_POS_1 = 0.5
  LINK_COM_POS_2 = 0.5
  LINK_MOI = 1.0
  MAX_VEL_1 = 4 * math.pi
  MAX_VEL_2 = 9 * math.pi
  AVAIL_TORQUE = (-1.0, 0.0, +1.0)
  gravity = 9.8

  def __init__(self, seed=None):
    high = np.array([1.0, 1.0, 1.0, 1.0, self.MAX_VEL_1, self.MAX_VEL_2])
    self.action_space = Discrete(3)
    self.observation_space = Box(-high, high)
    self.reward_range = (-float('inf'), float('inf'))
    self.metadata = {'render.modes': []}
    self.np_random = np.random.RandomState(seed)
    self.state = None

  def seed(self, seed=None):
    self.np_random = np.random.RandomState(seed)
    return [seed]

  def reset(self):
    self.state = self.np_random.uniform(low=-0.1, high=0.1, size=(4,))
    return self._get_ob()

  def _get_ob(self):
    s = self.state
    return np.array([math.cos(s[0]), math.sin(s[0]), math.cos(s[1]), math.sin(s[1]), s[2], s[3]])

  def _terminal(self):
    s = self.state
    return bool(-math.cos(s[0]) - math.cos(s[1] + s[0]) > 1.0)

  def _dsdt(self, s, torque):
    """d/dt of (theta1, theta2, dtheta1, dtheta2) under a constant torque."""
    m1, m2 = self.LINK_MASS_1, self.LINK_MASS_2
    l1, lc1, lc2 = self.LINK_LENGTH_1, self.LINK_COM_POS_1, self.LINK_COM_POS_2
    i1 = i2 = self.LINK_MOI
    g = self.gravity
    theta1, theta2, dtheta1, dtheta2 = s
    d1 = m1 * lc1 ** 2 + m2 * (l1 ** 2 + lc2 ** 2 + 2 * l1 * lc2 * math.cos(theta2)) + i1 + i2
    d2 = m2 * (lc2 ** 2 + l1 * lc2 * math.cos(theta2)) + i2
    phi2 = m2 * lc2 * g * math.cos(theta1 + theta2 - math.pi / 2.)
    phi1 = (-m2 * l1 * lc2 * dtheta2 ** 2 * math.sin(theta2)
            - 2 * m2 * l1 * lc2 * dtheta2 * dtheta1 * math.sin(theta2)
            + (m1 * lc1 + m2 * l1) * g * math.cos(theta1 - math.pi / 2) + phi2)
    ddtheta2 = ((torque + d2 / d1 * phi1 - m2 * l1 * lc2 * dtheta1 ** 2 * math.sin(theta2) - phi2)
                / (m2 * lc2 ** 2 + i2 - d2 ** 2 / d1))
    ddtheta1 = -(d2 * ddtheta2 + phi1) / d1
    return np.array([dtheta1, dtheta2, ddtheta1, ddtheta2])

  def step(self, action):
    assert action in (0, 1, 2), '%r invalid' % (action,)
    torque = self.AVAIL_TORQUE[action]
    y0, dt = np.asarray(self.state, dtype=np.float64), self.dt
    k1 = self._dsdt(y0, torque)
    k2 = self._dsdt(y0 + dt / 2 * k1, torque)
    k3 = self._dsdt(y0 + dt / 2 * k2, torque)
    k4 = self._dsdt(y0 + dt * k3, torque)
    ns = y0 + dt / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
    ns[0] = _wrap(ns[0], -math.pi, math.pi)
    ns[1] = _wrap(ns[1], -math.pi, math.pi)
    ns[2] = min(max(ns[2], -self.MAX_VEL_1), self.MAX_VEL_1)
    ns[3] = min(max(ns[3], -self.MAX_VEL_2), self.MAX_VEL_2)
    self.state = ns
    terminal = self._terminal()
    reward = -1.0 if not terminal else 0.0
    return self._get_ob(), reward, terminal, {}


def _wrap(x, lo, hi):
  """x brought into [lo, hi] by whole periods hi - lo."""
  diff = hi - lo
  while x > hi:
    x = x - diff
  while x < lo:
    x = x + diff
  return x


_ENVS = {'CartPole-v0': CartPoleEnv, 'Acrobot-v1': AcrobotEnv}


@gin_lite.configurable('create_gym_environment')
def create_gym_environment(environment_name=None, version='v0'):
  """gym_lib.py:54-72."""
  assert environment_name is not None
  full_game_name = '{}-{}'.format(environment_name, version)
  if full_game_name not in _ENVS:
    raise ValueError('dopamine_amd provides {} (no gym here); got {}'.format(
        sorted(_ENVS), full_game_name))
  return GymPreprocessing(_ENVS[full_game_name]())


gin_lite.register('gym_lib.create_gym_environment', create_gym_environment)


class GymPreprocessing(object):
  """gym_lib.py:321-372: the Dopamine-facing wrapper (tracks game_over)."""

  def __init__(self, environment, render=False):
    self.environment = environment
    self.game_over = False
    self.render = render

  @property
  def observation_space(self):
    return self.environment.observation_space

  @property
  def action_space(self):
    return self.environment.action_space

  @property
  def reward_range(self):
    return self.environment.reward_range

  @property
  def metadata(self):
    return self.environment.metadata

  def reset(self):
    return self.environment.reset()

  def step(self, action):
    observation, reward, game_over, info = self.environment.step(action)
    self.game_over = game_over
    return observation, reward, game_over, info
