"""Gradient-steps/s for the other single-GPU BASELINE configs, measured like
bench.py (synthetic full 1M-transition buffer in HBM, HIP graph, the reference's
_train_step cadence), for DESIGN.md -- not the bench line:

  config 2: DQN / Pong   -- 6 actions, uniform replay, n = 1, TF1 centered RMSProp, B = 32
  config 5: IQN / Breakout -- 4 actions, n = 3, Adam, B = 64 (quantile-Huber kernel)

    python tools/bench_configs.py [steps] [dqn_pong|iqn_breakout|all] [keyword=0|1 ...]

``rainbow`` (only when named) is config 3, bench.py's agent, for keyword overrides such as
``double_dqn=1`` or ``fused_head=0``.  ``quantile`` (only when named) is QR-DQN on the same
buffer, batch and optimizer schedule: QuantileAgent with 9 actions and 200 quantiles as upstream's
quantile.gin binds it (n = 3, PER, Adam 5e-5 / 3.125e-4), for the loss kernel's cost beside
``rainbow fused_head=0``, the schedule it shares.
"""
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')
import torch  # noqa: E402

import bench  # noqa: E402


def measure(make, actions, steps, warmup=20):
  agent = make()
  import random
  random.seed(0)
  bench.fill_synthetic(agent._replay.memory, actions, seed=1)
  torch.cuda.synchronize()

  agent.train_gradient_steps(warmup)     # = update_period _train_step() calls per step
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  agent.train_gradient_steps(steps)
  torch.cuda.synchronize()
  dt = time.perf_counter() - t0
  agent._replay.memory.sync_rng()
  out = {'steps_per_s': round(steps / dt, 1), 'ms_per_step': round(1e3 * dt / steps, 4),
         'batch': agent._batch_size,
         'hip_cnn': agent._hip is not None or getattr(agent, '_iqn', None) is not None}
  del agent
  gc.collect()
  torch.cuda.empty_cache()
  return out


def build_quantile(device, **kw):
  from dopamine_amd.agents.optimizers import AdamOptimizer
  from dopamine_amd.agents.quantile.quantile_agent import QuantileAgent
  agent = QuantileAgent(num_actions=9, num_atoms=200, kappa=1.0, update_horizon=3, gamma=0.99,
                        replay_scheme='prioritized', min_replay_history=20000, update_period=4,
                        target_update_period=8000,
                        optimizer=AdamOptimizer(learning_rate=0.00005, epsilon=0.0003125),
                        replay_capacity=1_000_000, batch_size=32, device=device, seed=0, **kw)
  agent.keep_gradients = False      # as bench.build_agent
  return agent


def main():
  steps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
  which = sys.argv[2] if len(sys.argv) > 2 else 'all'
  extra = {}
  for a in sys.argv[3:]:            # agent keyword overrides, e.g. pipeline=0
    k, v = a.split('=')
    extra[k] = bool(int(v))
  dev = torch.device('cuda', 0)
  res = {}
  if which in ('all', 'dqn_pong'):
    res['dqn_pong'] = measure(lambda: bench.build_dqn_pong(dev, **extra), 6, steps)
  if which in ('all', 'iqn_breakout'):
    res['iqn_breakout'] = measure(lambda: bench.build_iqn_breakout(dev, **extra), 4,
                                  max(steps // 3, 50))
  if which == 'rainbow':    # config 3, bench.py's own agent: for keyword overrides (double_dqn=1)
    res['rainbow'] = measure(lambda: bench.build_agent(9, 1_000_000, 32, dev, **extra), 9, steps)
  if which == 'quantile':
    res['quantile'] = measure(lambda: build_quantile(dev, **extra), 9, steps)
  print(json.dumps(res))


if __name__ == '__main__':
  main()
