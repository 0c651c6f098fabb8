"""A/B of the classic-control agents' two network paths on one device: the HIP MLP executor
(use_hip_mlp=True) against PyTorch's library GEMMs + autograd (use_hip_mlp=False), with an
A/A pair (a second HIP agent) for the noise floor.

For each of rainbow_cartpole.gin and dqn_cartpole.gin (where the False arm is config 1's
default path) the agents are built from the same seed over the same 3,000-transition
buffer, their graphs are primed, and they alternate, the order reversed every round, over
``--rounds`` rounds of two timed loops, the profiler off and a device synchronise closing
each window:
  learner  gradient steps/s of ``train_gradient_steps`` in windows of at least 0.3 s;
  agent    environment steps/s of ``begin_episode`` / ``step`` against the environment,
           a gradient step every update_period = 4 steps and the batch-1 acting forward
           every step.
Prints every round, then per loop the medians, the spread (max - min) of each arm, the
smallest HIP / PyTorch pair ratio and the A/A difference.
    python tools/gym_mlp_ab.py [--rounds 7] [--configs rainbow_cartpole dqn_cartpole]
--configs also takes dqn_acrobot (the 24-24 MLP with plain gradient descent) and
dqn_acrobot_fourier / dqn_cartpole_fourier (the Fourier-basis networks on fourier.hip),
double_dqn_acrobot / double_rainbow_cartpole (the double-DQN configs: name the plain config
too for the flag's cost in the same session), c51_cartpole_201 / c51_cartpole_201+double and
quantile_cartpole / double_quantile_cartpole / quantile_acrobot (QR-DQN, 200 quantiles) and
dueling_double_dqn_acrobot / dueling_rainbow_cartpole / dueling_quantile_cartpole (the dueling
heads; their parents are double_dqn_acrobot / double_rainbow_cartpole / quantile_cartpole) and
noisy_dqn_acrobot / full_rainbow_cartpole / noisy_quantile_cartpole (the noisy layers; their
parents are dqn_acrobot / dueling_rainbow_cartpole / quantile_cartpole) and mdqn_cartpole /
mdqn_acrobot / dueling_mdqn_acrobot (Munchausen-DQN; their parents are dqn_cartpole / dqn_acrobot).
--profile-arm runs 300 learner steps and 300 agent steps of the HIP arm only, of every config
named (the run to put under a kernel-trace profiler for the per-launch table)."""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dopamine_amd import gin_lite  # noqa: E402
from dopamine_amd.discrete_domains import gym_lib, run_experiment  # noqa: E402

_AGENTS = os.path.join(ROOT, 'dopamine_amd', 'agents')
CONFIGS = {'rainbow_cartpole': (os.path.join(_AGENTS, 'rainbow', 'configs', 'rainbow_cartpole.gin'),
                                'RainbowAgent'),
           'dqn_cartpole': (os.path.join(_AGENTS, 'dqn', 'configs', 'dqn_cartpole.gin'), 'DQNAgent')}
# (measured when named with --configs)
for _n in ('dqn_acrobot', 'dqn_acrobot_fourier', 'dqn_cartpole_fourier'):
  CONFIGS[_n] = (os.path.join(_AGENTS, 'dqn', 'configs', _n + '.gin'), 'DQNAgent')
# the double-DQN configs (run beside dqn_acrobot / rainbow_cartpole for the flag's cost)
CONFIGS['double_dqn_acrobot'] = (os.path.join(_AGENTS, 'dqn', 'configs', 'double_dqn_acrobot.gin'),
                                 'DQNAgent')
CONFIGS['double_rainbow_cartpole'] = (
    os.path.join(_AGENTS, 'rainbow', 'configs', 'double_rainbow_cartpole.gin'), 'RainbowAgent')
# the 201-atom support (the chunked regime of the C51 loss), plain and with the flag bound (a
# third element: extra bindings)
_C201 = os.path.join(_AGENTS, 'rainbow', 'configs', 'c51_cartpole_201.gin')
CONFIGS['c51_cartpole_201'] = (_C201, 'RainbowAgent')
CONFIGS['c51_cartpole_201+double'] = (_C201, 'RainbowAgent', ['RainbowAgent.double_dqn = True'])
# QR-DQN on dq_qr_loss (200 quantiles: MLP outputs of 400 and 600)
for _n in ('quantile_cartpole', 'double_quantile_cartpole', 'quantile_acrobot'):
  CONFIGS[_n] = (os.path.join(_AGENTS, 'quantile', 'configs', _n + '.gin'), 'QuantileAgent')
# (uniform weights: the loss kernel's instantiation without probabilities, for --profile-arm)
CONFIGS['quantile_cartpole+uniform'] = CONFIGS['quantile_cartpole'] + (
    ["QuantileAgent.replay_scheme = 'uniform'"],)
# the dueling heads (dq_dueling_forward / _backward): name the parent config too for the head's
# cost in the same session
CONFIGS['dueling_double_dqn_acrobot'] = (
    os.path.join(_AGENTS, 'dqn', 'configs', 'dueling_double_dqn_acrobot.gin'), 'DQNAgent')
CONFIGS['dueling_rainbow_cartpole'] = (
    os.path.join(_AGENTS, 'rainbow', 'configs', 'dueling_rainbow_cartpole.gin'), 'RainbowAgent')
CONFIGS['dueling_quantile_cartpole'] = (
    os.path.join(_AGENTS, 'quantile', 'configs', 'dueling_quantile_cartpole.gin'), 'QuantileAgent')
# the noisy layers (dq_noisy_draw / _weights / _grads): name the parent config too for the
# noise's cost in the same session
CONFIGS['noisy_dqn_acrobot'] = (
    os.path.join(_AGENTS, 'dqn', 'configs', 'noisy_dqn_acrobot.gin'), 'DQNAgent')
CONFIGS['full_rainbow_cartpole'] = (
    os.path.join(_AGENTS, 'rainbow', 'configs', 'full_rainbow_cartpole.gin'), 'RainbowAgent')
CONFIGS['noisy_quantile_cartpole'] = (
    os.path.join(_AGENTS, 'quantile', 'configs', 'noisy_quantile_cartpole.gin'), 'QuantileAgent')
# Munchausen-DQN (dq_mdqn_loss and the target network's forward on state): name the parent
# config too for the flag's cost in the same session
for _n in ('mdqn_cartpole', 'mdqn_acrobot', 'dueling_mdqn_acrobot'):
  CONFIGS[_n] = (os.path.join(_AGENTS, 'dqn', 'configs', _n + '.gin'), 'DQNAgent')
DEFAULT_CONFIGS = ['rainbow_cartpole', 'dqn_cartpole']


def build(config, hip):
  gin, cls, *extra = CONFIGS[config]
  gin_lite.clear_config()
  run_experiment.load_gin_configs(
      [gin], ['%s.use_hip_mlp = %s' % (cls, bool(hip))] + (extra[0] if extra else []))
  env = gym_lib.create_gym_environment()
  env.environment.seed(0)
  np.random.seed(0)
  random.seed(0)
  agent = run_experiment.create_agent(None, env)
  gin_lite.clear_config()
  assert (agent._mlp is not None) == bool(hip)
  rs = np.random.RandomState(1)
  obs = env.reset()
  for _ in range(3000):
    a = int(rs.randint(agent.num_actions))
    nobs, r, done, _ = env.step(a)
    agent._store_transition(np.asarray(obs).reshape(-1, 1), a, r, done)
    obs = env.reset() if done else nobs
  while not agent.graphs_primed():
    agent.train_gradient_steps(5)
  run_agent_loop(agent, env, 64)            # the interleaved graphs and the acting graph too
  torch.cuda.synchronize()
  return agent, env


def run_learner(agent, n):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  agent.train_gradient_steps(n)
  torch.cuda.synchronize()
  return n / (time.perf_counter() - t0)


def run_agent_loop(agent, env, n):
  """n environment steps as the Runner drives them (episodes capped at 200 steps)."""
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  done, length, action = True, 0, 0
  for _ in range(n):
    if done or length >= 200:
      if not done:
        agent.end_episode(1.0)
      action, length = agent.begin_episode(env.reset()), 0
    obs, r, done, _ = env.step(action)
    length += 1
    if done:
      agent.end_episode(r)
    else:
      action = agent.step(r, obs)
  torch.cuda.synchronize()
  return n / (time.perf_counter() - t0)


def summarize(name, rows):
  """rows: per round {arm: rate}."""
  arms = list(rows[0])
  med = {a: statistics.median(r[a] for r in rows) for a in arms}
  for a in arms:
    v = [r[a] for r in rows]
    print('%s [%s] median %.1f /s  min %.1f  max %.1f  spread %.2f%%' % (
        name, a, med[a], min(v), max(v), 100 * (max(v) - min(v)) / med[a]), flush=True)
  pairs = [r['hip'] / r['torch'] for r in rows]
  aa = [r['hip'] / r['hip2'] for r in rows]
  print('%s hip/torch: median of medians %.4f  smallest pair %.4f  largest pair %.4f' % (
      name, med['hip'] / med['torch'], min(pairs), max(pairs)), flush=True)
  print('%s A/A hip/hip2: median of medians %.4f  pairs %.4f .. %.4f' % (
      name, med['hip'] / med['hip2'], min(aa), max(aa)), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--configs', nargs='*', default=DEFAULT_CONFIGS)
  ap.add_argument('--window', type=float, default=0.3, help='seconds per learner window, at least')
  ap.add_argument('--agent-steps', type=int, default=2000)
  ap.add_argument('--profile-arm', action='store_true')
  args = ap.parse_args()
  torch.cuda.set_device(0)
  if args.profile_arm:
    for config in args.configs:           # (several: their kernels side by side in one trace)
      agent, env = build(config, True)
      print('profile arm %s: %.1f gradient steps/s, %.1f env steps/s' % (
          config, run_learner(agent, 300), run_agent_loop(agent, env, 300)), flush=True)
    return
  for config in args.configs:
    arms = {'hip': build(config, True), 'torch': build(config, False), 'hip2': build(config, True)}
    # learner windows of at least --window seconds on the slowest arm
    n = 200
    slowest = min(run_learner(a, n) for a, _ in arms.values())
    n = max(n, int(slowest * args.window * 1.25))
    print('# %s: learner windows of %d gradient steps, agent windows of %d env steps' % (
        config, n, args.agent_steps), flush=True)
    rows = {'learner': [], 'agent': []}
    for rnd in range(args.rounds):
      order = list(arms) if rnd % 2 == 0 else list(arms)[::-1]
      for loop in ('learner', 'agent'):
        row = {}
        for a in order:
          agent, env = arms[a]
          row[a] = run_learner(agent, n) if loop == 'learner' else run_agent_loop(
              agent, env, args.agent_steps)
          print('%s round %d %s [%s] %.1f /s' % (config, rnd, loop, a, row[a]), flush=True)
        rows[loop].append(row)
    for loop in ('learner', 'agent'):
      summarize('%s %s' % (config, loop), rows[loop])
    for agent, _ in arms.values():
      agent.close()


if __name__ == '__main__':
  main()
