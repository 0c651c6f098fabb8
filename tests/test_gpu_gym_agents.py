"""The classic-control agents on the HIP MLP executor, made as the Runner makes them.

Each agent is created from its gin file by ``run_experiment.create_agent``, its buffer is
filled with 3,000 random-action transitions from its environment, and it takes 10 gradient
steps through ``_train_step`` (eager steps, then replays of the captured HIP graphs).  Every
step is checked against float64 at the device's parameters of that step:
  * indices (and PER sampling probabilities) bit-exact against the oracle's sampler driven
    from the same host RNG state, and ``random``'s end state.  RainbowAgent keeps a
    prioritized buffer whatever its replay_scheme (rainbow_agent.py:307-337), so c51_acrobot
    (scheme 'uniform') draws through the sum tree's stratified sampler over equal priorities
    too: its oracle is PrioritizedOracle, as the north-star test's C51 case has it;
  * logits / Q, the target network's outputs, per-sample losses (of their scale) and new
    priorities (elementwise) within 1e-5;
  * every parameter gradient, two measures, both printed per tensor:
      rel   max|got - ref| / max|ref| of the tensor (tests/test_gpu_cartpole.py's bar, 1e-5),
      cond  oracle.nature_cnn.cond_ratio, |got - ref| / max(Σ|terms|, 1e-3 max|ref|), its terms
            from layer_reference chained in float64 from the device's parameters (LAYER_TOL);
  * the TF1 Adam update from the device's own state and gradient within 5e-8.

The gradient measure that applies is 'rel': measured first on the PyTorch path
(use_hip_mlp=False, library fp32 GEMMs + autograd, the parent's arithmetic), it stays inside
1e-5 on every tensor at these learning rates of 0.09-0.1, so the fallback to 'cond' is not
taken.  Worst values over the 10 steps and all tensors, MI355X (see GRAD_MEASURE)."""
import os
import pickle
import random

import numpy as np
import pytest
import torch

from oracle import learner as OL
from oracle import nature_cnn as ONC
from oracle import replay as OR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_AGENTS = os.path.join(ROOT, 'dopamine_amd', 'agents')
RAINBOW_CARTPOLE = os.path.join(_AGENTS, 'rainbow', 'configs', 'rainbow_cartpole.gin')
C51_ACROBOT = os.path.join(_AGENTS, 'rainbow', 'configs', 'c51_acrobot.gin')
RAINBOW_ACROBOT = os.path.join(_AGENTS, 'rainbow', 'configs', 'rainbow_acrobot.gin')
DQN_CARTPOLE = os.path.join(_AGENTS, 'dqn', 'configs', 'dqn_cartpole.gin')
TOL = 1e-5
PARAM_ATOL = 5e-8

# The gradient bar.  'rel' is tests/test_gpu_cartpole.py's: 1e-5 of each tensor's largest
# reference gradient.  Measured (worst over the 10 steps and all tensors; rel | cond):
#                     PyTorch path          HIP MLP
#   rainbow_cartpole  1.54e-6 | 4.9e-5      1.25e-6 | 4.2e-5
#   c51_acrobot       3.70e-6 | 1.4e-4      3.78e-6 | 1.5e-4
#   dqn_cartpole      3.87e-7 | 9.9e-6      1.85e-7 | 6.4e-6
# The library path meets 1e-5 on 'rel', so 'rel' is the measure asserted; 'cond' (its terms
# from the float64 chain) is printed beside it for both paths and sits at the same level on
# both.
GRAD_MEASURE = 'rel'


def _rel(got, ref):
  got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
  return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


def _make(gin_file, bindings):
  from dopamine_amd import gin_lite
  from dopamine_amd.discrete_domains import gym_lib, run_experiment
  gin_lite.clear_config()
  run_experiment.load_gin_configs([gin_file], list(bindings))
  env = gym_lib.create_gym_environment()
  env.environment.seed(0)
  np.random.seed(0)
  random.seed(0)
  agent = run_experiment.create_agent(None, env)
  gin_lite.clear_config()
  return env, agent


def _fill(env, agent, n=3000):
  """Random-action episodes into the buffer, stored as the agent stores them."""
  rs = np.random.RandomState(1)
  A, D = agent.num_actions, agent.observation_shape[0]
  obs, steps = env.reset(), 0
  for _ in range(n):
    a = int(rs.randint(A))
    nobs, r, done, _ = env.step(a)
    steps += 1
    done = done or steps >= 200          # Acrobot has no failure state: cap random episodes
    agent._store_transition(np.asarray(obs).reshape(D, 1), a, r, done)
    if done:
      obs, steps = env.reset(), 0
    else:
      obs = nobs


def _oracle(agent, prioritized):
  mem = agent._replay.memory
  mem.sync_rng()
  C, B, D = mem._replay_capacity, agent._batch_size, agent.observation_shape[0]
  cls = OR.PrioritizedOracle if prioritized else OR.ReplayOracle
  orc = cls((D, 1), 1, C, B, update_horizon=agent.update_horizon, gamma=agent.gamma,
            observation_dtype=np.float64)
  orc.observation = mem._frames.cpu().numpy().view(np.float64).reshape(C, D, 1)
  orc.action = mem._actions.cpu().numpy()
  orc.reward = mem._rewards.cpu().numpy()
  orc.terminal = mem._terminals.cpu().numpy()
  orc.add_count = int(mem.add_count)
  orc.invalid_range = OR.invalid_range(orc.cursor(), C, 1, agent.update_horizon)
  if prioritized:
    orc.sum_tree.nodes = mem._tree.cpu().numpy().copy()
    orc.sum_tree.max_recorded_priority = mem.sum_tree.max_recorded_priority
    orc.py_rng = random.Random()
    orc.py_rng.setstate(random.getstate())
  else:
    orc.np_rng = np.random.RandomState()
    orc.np_rng.set_state(np.random.get_state())
  return orc


def _rescale(net, state):
  """The float32 rescaled input the reference computes (gym_lib.py:95-99)."""
  x = np.asarray(state, np.float64).reshape(len(state), -1).astype(np.float32)
  lo = np.asarray(net.MIN, np.float64)
  rng = (np.asarray(net.MAX, np.float64) - lo).astype(np.float32)
  return np.float32(2.0) * ((x - lo.astype(np.float32)) / rng) - np.float32(1.0)


def _layers(net):
  return ['fc%d' % i for i in range(len(net.sizes))] + ['out']


def _params64(net, flat):
  return {n: torch.tensor(flat[o:o + int(np.prod(s))].reshape(s), dtype=torch.float64)
          for n, (o, s) in net.fp.offsets.items()}


def _forward64(net, flat, state):
  """float64 network on the float32 rescaled input: (output, the layers' inputs)."""
  P = _params64(net, flat)
  h = torch.from_numpy(_rescale(net, state)).double()
  ins = []
  for name in _layers(net):
    ins.append(h)
    z = torch.nn.functional.linear(h, P[name + '_w'], P[name + '_b'])
    h = z if name == 'out' else torch.relu(z)
  return h, ins, P


def _backward64(net, P, ins, gout):
  """layer_reference chained from the output layer down: per tensor (gradient, Σ|terms|)."""
  out, dz = {}, torch.from_numpy(np.asarray(gout, np.float64))
  for name, x_in in reversed(list(zip(_layers(net), ins))):
    ref = ONC.layer_reference('fc2', x_in, P[name + '_w'], P[name + '_b'], dz)
    out[name + '_w'] = (ref['dw'].numpy(), ref['dw_abs'].numpy())
    out[name + '_b'] = (ref['db'].numpy(), ref['db_abs'].numpy())
    dz = ref['dx']          # masked by (input > 0): the previous layer's ReLU
  return out


def run_lockstep(gin_file, bindings, steps=10):
  """Drive ``steps`` gradient steps and the float64 oracle in lockstep; returns (agent, errs)."""
  env, agent = _make(gin_file, bindings)
  rainbow = hasattr(agent, '_num_atoms')
  per_loss = rainbow and agent._replay_scheme == 'prioritized'
  agent.enable_trace()
  _fill(env, agent)
  orc = _oracle(agent, rainbow)
  net, B, A = agent.online_convnet, agent._batch_size, agent.num_actions
  offsets = net.fp.offsets
  cg = np.float64(np.float32(agent.cumulative_gamma))
  U = agent._UNROLL
  errs = dict(online=0.0, target=0.0, loss=0.0, priorities=0.0, grad_rel={}, grad_cond={},
              params=0.0)
  for _ in range(steps):
    k = agent._opt_steps % 2
    w = net.fp.flat.detach().cpu().double().numpy().copy()
    tw = agent.target_convnet.fp.flat.detach().cpu().double().numpy().copy()
    opt = agent._opt
    m, v = opt.m.cpu().double().numpy().copy(), opt.v.cpu().double().numpy().copy()
    st = opt.state.cpu().double().numpy()
    before = agent._opt_steps
    for _ in range(agent.update_period):   # one gradient step, the reference's cadence
      agent._train_step()
    assert agent._opt_steps == before + 1
    torch.cuda.synchronize()
    tr = {n: t[U + k].detach().cpu().numpy() for n, t in agent._trace.items()}
    idx = orc.sample_index_batch(B)
    np.testing.assert_array_equal(tr['indices'], idx)
    b = orc.sample_transition_batch(B, indices=idx)
    s, act, rew, ns, term = b[0], b[1], b[2], b[3], b[6]
    np.testing.assert_array_equal(tr['action'], act)
    np.testing.assert_array_equal(tr['reward'], rew)
    np.testing.assert_array_equal(tr['terminal'], term)
    if per_loss:
      np.testing.assert_array_equal(tr['sampling_probabilities'], b[8])
    out, ins, P = _forward64(net, w, s)
    tout, _, _ = _forward64(agent.target_convnet, tw, ns)
    out, tout = out.numpy(), tout.numpy()
    errs['outputs_traced'] = 'online_out' in tr and 'target_out' in tr
    if errs['outputs_traced']:      # (the PyTorch path of the Rainbow agents traces none)
      errs['online'] = max(errs['online'], _rel(tr['online_out'].reshape(out.shape), out))
      errs['target'] = max(errs['target'], _rel(tr['target_out'].reshape(tout.shape), tout))
    if rainbow:
      N = agent._num_atoms
      support = agent._support.cpu().double().numpy()
      ref = OL.c51_loss(out.reshape(B, A, N), tout.reshape(B, A, N), act, rew, term, support, cg,
                        b[8] if per_loss else None, dtype=np.float64)
      errs['priorities'] = max(errs['priorities'], float(
          (np.abs(tr['priorities'] - ref['priorities']) / np.abs(ref['priorities'])).max()))
      gout = ref['grad'].reshape(B, A * N)
    else:
      ref = OL.dqn_huber(out, tout, act, rew, term, cg, dtype=np.float64)
      gout = ref['grad']
    errs['loss'] = max(errs['loss'], _rel(tr['loss'], ref['loss']))
    for name, (g64, terms) in _backward64(net, P, ins, gout).items():
      o, shape = offsets[name]
      got = tr['grad'][o:o + int(np.prod(shape))]
      errs['grad_rel'][name] = max(errs['grad_rel'].get(name, 0.0), _rel(got, g64.reshape(-1)))
      cond = float(ONC.cond_ratio(got, g64.reshape(-1), terms.reshape(-1)).max())
      errs['grad_cond'][name] = max(errs['grad_cond'].get(name, 0.0), cond)
    # float64 TF1 Adam from the device's state with the device's gradient
    g = tr['grad'].astype(np.float64)
    f = lambda x: np.float64(np.float32(x))
    b1, b2, lr, eps = f(opt.b1), f(opt.b2), f(opt.lr), f(opt.eps)
    b1p, b2p = st[2 * k], st[2 * k + 1]
    m += (g - m) * (1 - b1)
    v += (g * g - v) * (1 - b2)
    w -= lr * np.sqrt(1 - b2p) / (1 - b1p) * m / (np.sqrt(v) + eps)
    gw = net.fp.flat.detach().cpu().double().numpy()
    errs['params'] = max(errs['params'], float(np.abs(gw - w).max()))
    if per_loss:      # the next step samples the tree the device wrote
      orc.set_priority(np.asarray(idx, np.int32), tr['priorities'].astype(np.float32))
  # the host RNG stream ends where the oracle's sequential draws leave it
  agent._discard_prefetch()
  agent._replay.memory.sync_rng()
  if rainbow:
    assert random.getstate() == orc.py_rng.getstate()
  else:
    a, b = np.random.get_state(), orc.np_rng.get_state()
    assert np.array_equal(a[1], b[1]) and a[2] == b[2]
  return agent, errs


def _check(name, agent, errs):
  print('gym agent errors', name, errs, flush=True)
  print('gym agent worst gradient: rel %.3g cond %.3g' % (
      max(errs['grad_rel'].values()), max(errs['grad_cond'].values())), flush=True)
  assert errs['outputs_traced']
  assert errs['online'] <= TOL and errs['target'] <= TOL and errs['loss'] <= TOL, errs
  assert errs['priorities'] <= TOL, errs
  if GRAD_MEASURE == 'rel':
    assert max(errs['grad_rel'].values()) <= TOL, errs
  else:
    assert max(errs['grad_cond'].values()) <= ONC.LAYER_TOL, errs
  assert errs['params'] <= PARAM_ATOL, errs
  assert agent._graphs is not None            # the later steps replayed the captured graph


def _uses_hip_mlp(agent):
  from dopamine_amd.mlp import HipMLP
  return (agent._mlp is not None and isinstance(agent._mlp['online'], HipMLP) and
          agent._needs_flat_grad())


def test_rainbow_cartpole_steps_match_float64_oracle():
  """rainbow_cartpole.gin: PER, n = 3, Adam 0.09."""
  agent, errs = run_lockstep(RAINBOW_CARTPOLE, [])
  assert _uses_hip_mlp(agent) and agent.update_horizon == 3
  _check('rainbow_cartpole', agent, errs)


def test_c51_acrobot_steps_match_float64_oracle():
  """c51_acrobot.gin: replay_scheme 'uniform', n = 1, Adam 0.1."""
  agent, errs = run_lockstep(C51_ACROBOT, [])
  assert _uses_hip_mlp(agent) and agent.num_actions == 3 and agent.observation_shape == (6, 1)
  _check('c51_acrobot', agent, errs)


def test_dqn_cartpole_opted_in_steps_match_float64_oracle():
  """dqn_cartpole.gin with use_hip_mlp=True: config 1 on the HIP executor."""
  agent, errs = run_lockstep(DQN_CARTPOLE, ['DQNAgent.use_hip_mlp = True'])
  assert _uses_hip_mlp(agent)
  _check('dqn_cartpole', agent, errs)
  _, default = _make(DQN_CARTPOLE, [])
  assert default._mlp is None                 # config 1's default path is unchanged
  _, off = _make(RAINBOW_CARTPOLE, ['RainbowAgent.use_hip_mlp = False'])
  assert off._mlp is None


@pytest.mark.parametrize('gin_file', (RAINBOW_CARTPOLE, C51_ACROBOT, DQN_CARTPOLE),
                         ids=('rainbow_cartpole', 'c51_acrobot', 'dqn_cartpole'))
def test_acting_forward_matches_float64(gin_file):
  """The batch-1 acting forward (captured graph, float64 state cast in the kernel) gives the
  float64 Q-values within 1e-5 of their scale."""
  bind = ['DQNAgent.use_hip_mlp = True'] if gin_file == DQN_CARTPOLE else []
  env, agent = _make(gin_file, bind)
  assert _uses_hip_mlp(agent)
  net = agent.online_convnet
  with torch.no_grad():     # non-zero biases, as after training
    for n, prm in net.fp.params.items():
      if n.endswith('_b'):
        prm.uniform_(-0.05, 0.1)
  w = net.fp.flat.detach().cpu().double().numpy()
  D = agent.observation_shape[0]
  obs = env.reset()
  for i in range(4):
    agent._reset_state()
    agent._record_observation(obs)
    q = agent._q_values(agent.state).detach().cpu().numpy()
    assert q.shape == (1, agent.num_actions)
    out, _, _ = _forward64(net, w, np.asarray(obs).reshape(1, D))
    if hasattr(agent, '_num_atoms'):
      logits = out.reshape(1, agent.num_actions, agent._num_atoms)
      want = (torch.softmax(logits, -1) * agent._support.cpu().double()).sum(-1).numpy()
    else:
      want = out.numpy()
    assert _rel(q, want) <= TOL, (i, q, want)
    obs, _, _, _ = env.step(i % agent.num_actions)
  assert agent._act is not None and agent._act[3] is not None     # the captured graph served


def test_acrobot_experiment_runs_logs_checkpoints_and_resumes(tmp_path):
  """rainbow_acrobot.gin end to end through train.py, as tests/test_gpu_runner.py does for
  config 1: two short iterations, logs, checkpoints, and a resume that picks them up."""
  from dopamine_amd import gin_lite
  from dopamine_amd.discrete_domains import train
  small = ['Runner.training_steps = 300', 'Runner.evaluation_steps = 100',
           'Runner.max_steps_per_episode = 100', 'RainbowAgent.min_replay_history = 100',
           'WrappedPrioritizedReplayBuffer.replay_capacity = 5000', 'Runner.num_iterations = 2']
  base = str(tmp_path / 'acrobot')
  args = ['--base_dir', base, '--gin_files', RAINBOW_ACROBOT] + sum(
      [['--gin_bindings', b] for b in small], [])
  gin_lite.clear_config()
  runner = train.main(args)
  agent = runner._agent
  assert _uses_hip_mlp(agent) and agent.num_actions == 3
  assert agent.training_steps >= 600 and agent._replay.memory.add_count > 300
  assert agent._opt_steps >= 100 and agent._graph_sets      # trained, on captured graphs
  with open(os.path.join(base, 'logs', 'log_1'), 'rb') as f:
    logs = pickle.load(f)
  it = logs['iteration_1']
  assert it['train_episode_lengths'] and it['eval_episode_lengths']
  assert np.isfinite(it['train_average_return'][0]) and np.isfinite(it['eval_average_return'][0])
  assert bool(torch.isfinite(agent.online_convnet.fp.flat).all())
  ck = os.path.join(base, 'checkpoints')
  for f in ('ckpt.1', 'sentinel_checkpoint_complete.1', 'tf_ckpt-1', 'add_count_ckpt.1.gz'):
    assert os.path.exists(os.path.join(ck, f)), f
  params = agent.online_convnet.fp.flat.detach().cpu().clone()
  steps = agent.training_steps
  gin_lite.clear_config()
  runner2 = train.main(args)
  assert runner2._start_iteration == 2
  a2 = runner2._agent
  assert a2.training_steps == steps
  assert np.array_equal(a2.online_convnet.fp.flat.detach().cpu().numpy(), params.numpy())
  assert int(a2._replay.memory.add_count) == int(agent._replay.memory.add_count)
  gin_lite.clear_config()
