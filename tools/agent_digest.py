"""One sha256 per agent schedule, for comparing two trees (a refactor against its parent): the
digest covers the online and target parameters, every optimizer tensor and the last step's
per-sample loss after STEPS gradient steps that cross target syncs; beside it, the families of
HIP graphs the agent captured on the way (_graph_sets' keys).  The agents, buffers and fills
are tests/test_gpu_agent.py's and tests/test_gpu_gym_agents.py's; only names that every tree
has are used.  Run it in a fresh process per tree and compare the outputs line by line.

    python tools/agent_digest.py [case ...]
"""
import hashlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

STEPS = 18        # gradient steps: 72 training steps, target syncs at 0, 28 and 56


def digest(agent):
  torch.cuda.synchronize()
  ts = [agent.online_convnet.fp.flat, agent.target_convnet.fp.flat]
  ts += [v for _, v in sorted(vars(agent._opt).items()) if isinstance(v, torch.Tensor)]
  ts.append(agent._loss_out['loss'])
  h = hashlib.sha256()
  for t in ts:
    h.update(t.detach().cpu().contiguous().numpy().tobytes())
  fams = sorted({str(k[0] if isinstance(k, tuple) else k) for k in agent._graph_sets})
  return '%s graphs: %s' % (h.hexdigest(), ','.join(fams) or 'none')


def loop(agent, steps=STEPS):
  """The learner loop: chunk graphs where they apply."""
  agent.train_gradient_steps(steps)
  return agent


def per_call(agent, steps=STEPS, add=False):
  """One _train_step per call; add: a transition stored between gradient steps, so every
  step discards a prefetch and runs the non-pipelined graph family."""
  for i in range(steps):
    for _ in range(agent.update_period):
      agent._train_step()
    if add and i % 2 == 0:
      agent._store_transition(np.full(agent.observation_shape, i, np.uint8), 1, 0.5, False)
  return agent


def seed():
  random.seed(5)
  np.random.seed(5)
  torch.manual_seed(5)


def rainbow(**kw):
  from tests.test_gpu_agent import _rainbow
  seed()
  return _rainbow(target_update_period=28, **kw)


def dqn(**kw):
  from dopamine_amd.agents.dqn.dqn_agent import DQNAgent
  from tests.test_gpu_agent import _fill
  seed()
  a = DQNAgent(num_actions=6, replay_capacity=3000, batch_size=32, min_replay_history=100,
               target_update_period=28, **kw)
  _fill(a._replay.memory, 6, 3)
  return a


def iqn(**kw):
  from dopamine_amd.agents.implicit_quantile.implicit_quantile_agent import ImplicitQuantileAgent
  from tests.test_gpu_agent import _fill
  seed()
  a = ImplicitQuantileAgent(num_actions=4, replay_capacity=3000, batch_size=16, num_tau_samples=8,
                            num_tau_prime_samples=8, num_quantile_samples=4,
                            min_replay_history=100, update_horizon=3, replay_scheme='uniform',
                            target_update_period=28, **kw)
  _fill(a._replay.memory, 4, 3)
  return a


def quantile(**kw):
  """A Nature-CNN QuantileAgent (101 quantiles) over tests/test_gpu_agent.py's buffer fill."""
  from dopamine_amd.agents.quantile.quantile_agent import QuantileAgent
  from tests.test_gpu_agent import _fill
  seed()
  a = QuantileAgent(num_actions=4, num_atoms=101, update_horizon=3, replay_capacity=3000,
                    batch_size=32, min_replay_history=100, target_update_period=28, **kw)
  _fill(a._replay.memory, 4, 3)
  return a


def gym(config):
  """A classic-control agent from its gin file (a name of tests/test_gpu_gym_agents.py, or a
  path below dopamine_amd/agents), filled by random-action episodes; it then acts for 120
  steps (per-call gradient steps with adds between them, one target sync)."""
  from tests import test_gpu_gym_agents as G
  path = getattr(G, config, None) or os.path.join(ROOT, 'dopamine_amd', 'agents', config)
  env, agent = G._make(path, [])
  G._fill(env, agent, 1500)
  agent.begin_episode(env.reset())
  for _ in range(120):
    obs, r, done, _ = env.step(agent.action)
    if done:
      agent.end_episode(r)
      agent.begin_episode(env.reset())
    else:
      agent.step(r, obs)
  return agent


def rccl(loop_, **kw):
  """One-rank RCCL group with every collective executed (bench.py --force-dist); a group of
  its own per case, as tests/test_gpu_rccl.py's fixture makes one per test."""
  import torch.distributed as dist
  from dopamine_amd import parallel
  from tests.test_gpu_multirank import _agent, _run
  from tests.test_gpu_rccl import _free_port
  dist.init_process_group('nccl', init_method='tcp://127.0.0.1:%d' % _free_port(), rank=0,
                          world_size=1, device_id=torch.device('cuda', 0))
  parallel.FORCE_COLLECTIVES = True
  try:
    seed()
    agent = _agent(dist.group.WORLD, 0, capacity=3000, **kw)
    _run(agent, loop_, STEPS)
    d = digest(agent)
    agent.close()
  finally:
    parallel.FORCE_COLLECTIVES = False
    torch.cuda.synchronize()
    dist.destroy_process_group()
  return d


CASES = {
    'dqn_loop': lambda: digest(loop(dqn())),                       # the gchunk graphs
    'rainbow_loop': lambda: digest(loop(rainbow())),               # the chunk graphs
    'rainbow_per_call': lambda: digest(per_call(rainbow())),
    'rainbow_per_call_adds': lambda: digest(per_call(rainbow(), add=True)),
    'rainbow_unfused_loop': lambda: digest(loop(rainbow(fused_head=False, ride_replay=False))),
    'rainbow_unfused_per_call': lambda: digest(per_call(rainbow(fused_head=False,
                                                                ride_replay=False))),
    'rainbow_plain_head_loop': lambda: digest(loop(rainbow(fused_head=False))),
    'rainbow_n10_loop': lambda: digest(loop(rainbow_n10())),       # no riders
    'rainbow_eager': lambda: digest(per_call(rainbow(use_hip_graph=False))),
    'rainbow_eager_unpipelined': lambda: digest(per_call(rainbow(use_hip_graph=False,
                                                                 pipeline=False))),
    'iqn_loop': lambda: digest(loop(iqn())),
    'iqn_double_loop': lambda: digest(loop(iqn(double_dqn=True))),
    'iqn_per_call': lambda: digest(per_call(iqn())),
    'c51_acrobot_mlp': lambda: digest(gym('C51_ACROBOT')),
    'rainbow_cartpole_mlp': lambda: digest(gym('RAINBOW_CARTPOLE')),
    'dqn_cartpole_torch': lambda: digest(gym('DQN_CARTPOLE')),
    # QR-DQN (dq_qr_loss): the Nature-CNN schedules and the classic-control configs
    'quantile_loop': lambda: digest(loop(quantile())),
    'quantile_per_call': lambda: digest(per_call(quantile())),
    'quantile_double_loop': lambda: digest(loop(quantile(double_dqn=True))),
    'quantile_cartpole_mlp': lambda: digest(gym('quantile/configs/quantile_cartpole.gin')),
    'double_quantile_cartpole_mlp': lambda: digest(
        gym('quantile/configs/double_quantile_cartpole.gin')),
    'quantile_acrobot_mlp': lambda: digest(gym('quantile/configs/quantile_acrobot.gin')),
    # dueling heads (dq_dueling_forward / _backward): a Nature-CNN schedule and the configs
    'dueling_rainbow_loop': lambda: digest(loop(rainbow(dueling=True))),
    'dueling_rainbow_cartpole_mlp': lambda: digest(
        gym('rainbow/configs/dueling_rainbow_cartpole.gin')),
    'dueling_double_dqn_acrobot_mlp': lambda: digest(
        gym('dqn/configs/dueling_double_dqn_acrobot.gin')),
    'dueling_quantile_cartpole_mlp': lambda: digest(
        gym('quantile/configs/dueling_quantile_cartpole.gin')),
    # noisy layers (dq_noisy_draw / _weights / _grads): the configs
    'full_rainbow_cartpole_mlp': lambda: digest(gym('rainbow/configs/full_rainbow_cartpole.gin')),
    'noisy_dqn_acrobot_mlp': lambda: digest(gym('dqn/configs/noisy_dqn_acrobot.gin')),
    'noisy_quantile_cartpole_mlp': lambda: digest(
        gym('quantile/configs/noisy_quantile_cartpole.gin')),
}
for _zero in (False, True):
  for _native in (True, False):
    for _loop in (False, True):
      CASES['rccl_%s_%s_%s' % ('zero1' if _zero else 'allreduce', 'native' if _native else 'torch',
                               'loop' if _loop else 'per_call')] = (
          lambda z=_zero, n=_native, l=_loop: rccl(l, shard_optimizer=z, native_comm=n))


def rainbow_n10():
  from dopamine_amd.agents.optimizers import AdamOptimizer
  from dopamine_amd.agents.rainbow.rainbow_agent import RainbowAgent
  from tests.test_gpu_agent import _fill
  seed()
  a = RainbowAgent(num_actions=9, update_horizon=10, replay_capacity=3000, batch_size=32,
                   min_replay_history=100, target_update_period=28,
                   optimizer=AdamOptimizer(6.25e-5, epsilon=1.5e-4))
  _fill(a._replay.memory, 9, 3)
  return a


def main():
  torch.cuda.set_device(0)
  for name in sys.argv[1:] or list(CASES):
    print('%-34s %s' % (name, CASES[name]()), flush=True)


if __name__ == '__main__':
  main()
