"""DQNAgent / RainbowAgent / QuantileAgent with noisy=True: every gradient step against float64
at the device's parameters AS THEY WERE BEFORE THAT STEP and the noise that step TRACED.

The pattern, the helpers, the bars and the near-tie rule are tests/test_gpu_dueling_agents.py's
(TOL 1e-5, PARAM_ATOL 5e-8, the 'rel' gradient measure).  The agents are made from their gin
files and take 10 gradient steps through ``_train_step`` -- eager steps, then replays of the
captured graphs.  Per step the float64 reference forms each network's effective parameters from
the pre-step mu and sigma and the traced noise of that forward (tests/noisy_cases.py's
weights64), runs the float64 MLP on them (with ``dueling`` the float64 combine on its raw head),
the existing loss references on the outputs, the float64 network backward, and maps dw to
d sigma (grads64).  The traced outputs, the select output, the loss, the priorities, every mu
and sigma gradient and the Adam / SGD update are compared; the traced noise itself against the
generator's restatement at its (role seed, call).  The -pytorch run (use_hip_mlp = False) takes
the networks' torch expression and autograd on noise from the same generators: an independent
statement of the same definition.

Near ties: DD._near_tie_astar as it stands; the count is printed; more than one sample in eight
of any step fails.  That cap was not rehearsed on the CPU (the networks need the device).
"""
import os
import pickle
import random

import numpy as np
import pytest
import torch

from tests import dueling_cases as DC
from tests import fourier_cases as FC
from tests import noisy_cases as NC
from tests import test_gpu_dueling_agents as DA
from tests import test_gpu_fourier_agents as F
from tests import test_gpu_gym_agents as G
from tests import test_gpu_quantile_agents as QA

pytestmark = pytest.mark.gpu

_AGENTS = os.path.join(G.ROOT, 'dopamine_amd', 'agents')
_GIN = {
    'noisy_dqn_acrobot': ('dqn/configs/noisy_dqn_acrobot.gin', []),
    'full_rainbow_cartpole': ('rainbow/configs/full_rainbow_cartpole.gin', []),
    'noisy_quantile_cartpole': ('quantile/configs/noisy_quantile_cartpole.gin', []),
    'full_rainbow_cartpole-pytorch': ('rainbow/configs/full_rainbow_cartpole.gin',
                                      ['RainbowAgent.use_hip_mlp = False']),
}
_CLS = {'noisy_dqn_acrobot': 'DQNAgent', 'full_rainbow_cartpole': 'RainbowAgent',
        'noisy_quantile_cartpole': 'QuantileAgent'}
TOL, PARAM_ATOL = G.TOL, G.PARAM_ATOL


def _geometry(net):
  return (net.D, net.sizes, net.n_out)


def _per_layer(net, flat, part=''):
  out = []
  for n in net.layer_names():
    pair = []
    for s in ('_w', '_b'):
      o, shape = net.fp.offsets[n + part + s]
      pair.append(flat[o:o + int(np.prod(shape))].reshape(shape))
    out.append(tuple(pair))
  return out


def _eff_flat(net, flat, noise):
  """The float64 flat buffer whose mu slots hold the effective parameters on ``noise``."""
  eff = NC.weights64(_geometry(net), _per_layer(net, flat), _per_layer(net, flat, '_sigma'), noise)
  out = np.array(flat, np.float64)
  for n, (w, b, _, _) in zip(net.layer_names(), eff):
    for s, v in (('_w', w), ('_b', b)):
      o, _ = net.fp.offsets[n + s]
      out[o:o + v.size] = v.reshape(-1)
  return out


def _noise_is_call(noise, role, call):
  """The traced noise is the restatement's draw of (role seed, call), in the draw tests' measure."""
  want = NC.normal64(NC.ROLE_SEEDS[role], call, noise.size)
  f = noise.astype(np.float64)
  return bool((np.abs(f * np.abs(f) - want) <= 1e-5 * np.maximum(1.0, np.abs(want))).all())


def run_lockstep(name, steps=10):
  gin, bindings = _GIN[name]
  env, agent = G._make(os.path.join(_AGENTS, gin), bindings)
  kind = DA._kind(agent)
  assert agent.noisy is True and not agent._fused()
  assert agent.online_convnet.noisy and agent.target_convnet.noisy
  double, dueling = agent._double(), agent.dueling
  prioritized = kind != 'dqn'
  per = prioritized and agent._replay_scheme == 'prioritized'
  agent.enable_trace()
  G._fill(env, agent)
  orc = G._oracle(agent, prioritized)
  net, B, A = agent.online_convnet, agent._batch_size, agent.num_actions
  n = getattr(agent, '_num_atoms', None) or 1
  assert net.n_out == (A + int(dueling)) * n
  combine = (lambda h: DA._combine64(h, A, n)) if dueling else (lambda h: h)
  cg = np.float64(np.float32(agent.cumulative_gamma))
  U = agent._UNROLL
  errs = dict(online=0.0, target=0.0, online_next=0.0, loss=0.0, priorities=0.0, grad={},
              params=0.0, near_ties=0)
  online_call, target_call = 0, -1
  for step in range(steps):
    k = agent._opt_steps % 2
    w32 = net.fp.flat.detach().cpu().numpy().copy()          # the parameters BEFORE this step
    w = w32.astype(np.float64)
    tw = agent.target_convnet.fp.flat.detach().cpu().double().numpy().copy()
    opt = agent._opt
    adam = hasattr(opt, 'm')
    if adam:
      m, v = opt.m.cpu().double().numpy().copy(), opt.v.cpu().double().numpy().copy()
      st = opt.state.cpu().double().numpy()
    before = agent._opt_steps
    for _ in range(agent.update_period):
      agent._train_step()
    assert agent._opt_steps == before + 1
    torch.cuda.synchronize()
    tr = {key: t[U + k].detach().cpu().numpy() for key, t in agent._trace.items()}
    idx = orc.sample_index_batch(B)
    np.testing.assert_array_equal(tr['indices'], idx)
    b = orc.sample_transition_batch(B, indices=idx)
    s, act, rew, ns, term = b[0], b[1], b[2], b[3], b[6]
    np.testing.assert_array_equal(tr['action'], act)
    np.testing.assert_array_equal(tr['reward'], rew)
    np.testing.assert_array_equal(tr['terminal'], term)
    if per:
      np.testing.assert_array_equal(tr['sampling_probabilities'], b[8])
    # the noise: the online generator's calls in order (the forward on s, then the select
    # forward on s'); the target generator's a later call than the last step's (a prefetch
    # redone after a target sync has consumed one in between), the first step's call 0
    on, tn = tr['online_noise'], tr['target_noise']
    assert on.shape == tn.shape == (net.noise_numel,)
    assert _noise_is_call(on, 'online', online_call), (step, online_call)
    online_call += 1
    calls_now = int(agent._noise['target'].counter[0].item())
    found = [c for c in range(target_call + 1, calls_now) if _noise_is_call(tn, 'target', c)]
    assert len(found) == 1 and (step > 0 or found == [0]), (step, target_call, calls_now, found)
    target_call = found[0]
    assert not np.array_equal(on, tn)
    if double:
      sn = tr['online_next_noise']
      assert _noise_is_call(sn, 'online', online_call), (step, online_call)
      online_call += 1
      assert not np.array_equal(sn, on) and not np.array_equal(sn, tn)
    else:
      assert 'online_next_noise' not in tr
    assert int(agent._noise['online'].counter[0].item()) == online_call
    head, ctx = F._forward64(net, _eff_flat(net, w, on), s)
    out = combine(head)
    tout = combine(F._forward64(agent.target_convnet, _eff_flat(agent.target_convnet, tw, tn),
                                ns)[0])
    sout = tout
    if double:     # ONLINE parameters on next_state, on noise of its own
      sout = combine(F._forward64(net, _eff_flat(net, w, sn), ns)[0])
      errs['online_next'] = max(errs['online_next'],
                                G._rel(tr['online_next_out'].reshape(sout.shape), sout))
    if 'online_out' in tr and 'target_out' in tr:   # (the Rainbow agents' PyTorch path traces none)
      errs['online'] = max(errs['online'], G._rel(tr['online_out'].reshape(out.shape), out))
      errs['target'] = max(errs['target'], G._rel(tr['target_out'].reshape(tout.shape), tout))
    else:
      assert agent._mlp is None and kind != 'dqn'
    ref, near = DA._loss_reference(agent, kind, out, tout, sout, act, rew, term, cg,
                                   b[8] if per else None, tr['loss'])
    errs['near_ties'] += near
    print('%s step %d: %d near ties of %d samples' % (name, step, near, B), flush=True)
    assert near * 8 <= B, 'step %d: %d of %d samples are near ties' % (step, near, B)
    errs['loss'] = max(errs['loss'], G._rel(tr['loss'], ref['loss']))
    if per:
      errs['priorities'] = max(errs['priorities'], float(
          (np.abs(tr['priorities'] - ref['priorities']) / np.abs(ref['priorities'])).max()))
    dhead = np.asarray(ref['grad'], np.float64).reshape(B, -1)
    if dueling:
      dhead = DC.backward64(dhead.reshape(B, A, n), A, n)[0]
    g64 = F._backward64(net, ctx, dhead)
    dw = [(g64[nm + '_w'], g64[nm + '_b']) for nm in net.layer_names()]
    for nm, (sw, sb, _, _) in zip(net.layer_names(), NC.grads64(_geometry(net), dw, on)):
      g64[nm + '_sigma_w'], g64[nm + '_sigma_b'] = sw, sb
    assert set(g64) == set(net.fp.offsets)
    for pname, ref_g in g64.items():
      o, shape = net.fp.offsets[pname]
      got = tr['grad'][o:o + int(np.prod(shape))]
      errs['grad'][pname] = max(errs['grad'].get(pname, 0.0), G._rel(got, ref_g.reshape(-1)))
    gw = net.fp.flat.detach().cpu().numpy()
    if adam:       # float64 TF1 Adam from the device's state with the device's gradient
      g = tr['grad'].astype(np.float64)
      f = lambda x: np.float64(np.float32(x))
      b1, b2, lr, eps = f(opt.b1), f(opt.b2), f(opt.lr), f(opt.eps)
      b1p, b2p = st[2 * k], st[2 * k + 1]
      m += (g - m) * (1 - b1)
      v += (g * g - v) * (1 - b2)
      w -= lr * np.sqrt(1 - b2p) / (1 - b1p) * m / (np.sqrt(v) + eps)
      errs['params'] = max(errs['params'], float(np.abs(gw.astype(np.float64) - w).max()))
    else:          # plain gradient descent: bitwise float32
      want = FC.sgd32(w32, tr['grad'], opt.lr)
      assert np.array_equal(gw.view(np.uint32), want.view(np.uint32))
    o, shape = net.fp.offsets['fc0_sigma_w']       # the sigmas train
    assert not np.array_equal(gw[o:o + int(np.prod(shape))], w32[o:o + int(np.prod(shape))])
    if per:        # the next step samples the tree the device wrote
      orc.set_priority(np.asarray(idx, np.int32), tr['priorities'].astype(np.float32))
  agent._discard_prefetch()
  agent._replay.memory.sync_rng()
  if prioritized:
    assert random.getstate() == orc.py_rng.getstate()
  else:
    a, b = np.random.get_state(), orc.np_rng.get_state()
    assert np.array_equal(a[1], b[1]) and a[2] == b[2]
  return agent, errs


@pytest.mark.parametrize('name', sorted(_GIN))
def test_noisy_steps_match_float64_at_the_pre_step_parameters_and_traced_noise(name):
  from dopamine_amd import ops
  from dopamine_amd.mlp import HipMLP
  agent, errs = run_lockstep(name)
  print('noisy agent errors', name, errs, flush=True)
  if name.endswith('-pytorch'):
    assert agent._mlp is None and agent._online_next is None
    assert set(agent._noise_bufs) >= {'online', 'online_next', 'target0', 'target1'}
  else:
    exes = [agent._mlp['online']] + agent._mlp['target']
    if agent._double():
      exes.append(agent._online_next)
    assert all(isinstance(e, HipMLP) and e.noisy for e in exes)
    assert agent._mlp['online'].sampler is agent._noise['online']
    assert all(e.sampler is agent._noise['target'] for e in agent._mlp['target'])
  if name == 'noisy_dqn_acrobot':
    assert isinstance(agent._opt, ops.TF1GradientDescent) and not agent._double()
    assert agent.online_convnet.sizes == (24, 24) and agent.online_convnet.n_out == 3
  if name.startswith('full_rainbow_cartpole'):
    assert agent._double() and agent.dueling and agent._replay_scheme == 'prioritized'
    assert agent.update_horizon == 3 and agent.online_convnet.n_out == 3 * 51
  if name == 'noisy_quantile_cartpole':
    assert not agent._double() and agent.online_convnet.n_out == 400
  assert agent.epsilon_train == 0.0 and agent.epsilon_eval == 0.0
  assert errs['online_next'] <= TOL, errs
  assert errs['online'] <= TOL and errs['target'] <= TOL and errs['loss'] <= TOL, errs
  assert errs['priorities'] <= TOL, errs
  assert max(errs['grad'].values()) <= TOL, errs
  assert any('_sigma_' in key for key in errs['grad'])
  assert errs['params'] <= PARAM_ATOL, errs
  assert agent._graphs is not None            # the later steps replayed the captured graph


@pytest.mark.parametrize('name', ['full_rainbow_cartpole', 'noisy_dqn_acrobot'])
def test_per_call_steps_and_learner_loop_are_bitwise_equal(name):
  """2 * _UNROLL + 1 gradient steps one per call (eager, then per-step graphs) and the same
  number through train_gradient_steps: bitwise equal parameters, optimizer state, sum tree and
  noise counters."""
  res = []
  for chunked in (False, True):
    env, a = G._make(os.path.join(_AGENTS, _GIN[name][0]), [])
    G._fill(env, a, 2000)             # past the acrobot config's min_replay_history of 1000
    n = 2 * a._UNROLL + 1
    if chunked:
      a.train_gradient_steps(n)
    else:
      for _ in range(a.update_period * n):
        a._train_step()
    assert a._opt_steps == n and a.noisy
    a._discard_prefetch()
    a._replay.memory.sync_rng()
    torch.cuda.synchronize()
    st = dict(online=a.online_convnet.fp.flat.cpu().numpy(),
              target=a.target_convnet.fp.flat.cpu().numpy(),
              **{'opt_' + key: t.cpu().numpy() for key, t in a._opt_tensors()},
              **{'noise_' + r: s.counter.cpu().numpy() for r, s in a._noise.items()})
    if DA._kind(a) != 'dqn':
      st['tree'] = a._replay.memory.sum_tree.nodes[-1].copy()
    assert st['noise_online'][0] == n * (1 + int(a._double())) and st['noise_target'][0] >= n
    assert st['noise_act'][0] == 0
    res.append(st)
  QA._same(res)
  assert not np.array_equal(res[0]['online'], res[0]['target'])


# ================================================================================== acting
@pytest.mark.parametrize('graph', [True, False], ids=['graph', 'no-graph'])
@pytest.mark.parametrize('name', sorted(_CLS))
def test_acting_draws_fresh_noise_in_training_and_none_in_evaluation(name, graph):
  from dopamine_amd.agents import networks
  from dopamine_amd.mlp import HipMLP
  gin = os.path.join(_AGENTS, _GIN[name][0])
  env, agent = G._make(gin, ['%s.use_hip_graph = %s' % (_CLS[name], graph)])
  assert agent._mlp is not None and agent.noisy and not agent.eval_mode
  net = agent.online_convnet
  obs = env.reset()
  agent._reset_state()
  agent._record_observation(obs)
  q = lambda: agent._q_values(agent.state).detach().clone()
  a, b = q(), q()
  assert a.shape == (1, agent.num_actions) and not torch.equal(a, b)     # fresh noise per call
  calls = int(agent._noise['act'].counter[0].item())
  assert calls >= 2
  # the acting noise is the 'act' generator's last call
  exe = agent._act[True][0]
  torch.cuda.synchronize()
  assert _noise_is_call(exe.acts['noise'].cpu().numpy(), 'act', calls - 1)
  agent.eval_mode = True
  c, d = q(), q()
  assert torch.equal(c, d) and not torch.equal(c, b)
  assert int(agent._noise['act'].counter[0].item()) == calls             # no draw
  # bitwise a plain network's executor on the same mu
  plain = type(net)(agent.num_actions, device='cuda', dueling=agent.dueling,
                    network_size=net.sizes, **({} if net.N is None else {'num_atoms': net.N}))
  assert isinstance(plain, networks.BasicDiscreteDomainNetwork) and not plain.noisy
  plain.fp.flat.copy_(net.fp.flat[:net.mu_numel])
  x = torch.as_tensor(np.asarray(obs, np.float64).reshape(-1), device='cuda')
  want = agent._q_from_output(HipMLP(plain, 1).forward(x))
  assert torch.equal(c, want)
  # back and forth: both executors (and graphs) still serve
  agent.eval_mode = False
  e = q()
  assert not torch.equal(e, a) and not torch.equal(e, b) and not torch.equal(e, c)
  agent.eval_mode = True
  assert torch.equal(q(), c)
  assert sorted(agent._act) == [False, True]
  assert all((v[3] is not None) == graph for v in agent._act.values())
  assert int(agent._noise['act'].counter[0].item()) == calls + 1
  assert agent._noise['online'].counter.tolist() == agent._noise['target'].counter.tolist() == [0, 0]


def test_acting_on_the_pytorch_path():
  gin = os.path.join(_AGENTS, _GIN['full_rainbow_cartpole'][0])
  env, agent = G._make(gin, ['RainbowAgent.use_hip_mlp = False'])
  assert agent._mlp is None and agent.noisy
  agent._reset_state()
  agent._record_observation(env.reset())
  q = lambda: agent._q_values(agent.state).detach().clone()
  a, b = q(), q()
  assert not torch.equal(a, b) and agent._noise['act'].counter.tolist() == [2, 0]
  agent.eval_mode = True
  assert torch.equal(q(), q()) and agent._noise['act'].counter.tolist() == [2, 0]


# ================================================================================== the rest
def test_full_rainbow_experiment_runs_checkpoints_resumes_and_refuses_the_other_kind(tmp_path):
  from dopamine_amd import gin_lite
  from dopamine_amd.discrete_domains import train
  small = ['Runner.training_steps = 400', 'Runner.evaluation_steps = 100',
           'RainbowAgent.min_replay_history = 200', 'Runner.num_iterations = 1',
           'WrappedPrioritizedReplayBuffer.replay_capacity = 5000']
  base = str(tmp_path / 'full_rainbow_cartpole')
  gin = os.path.join(_AGENTS, _GIN['full_rainbow_cartpole'][0])
  args = ['--base_dir', base, '--gin_files', gin] + sum([['--gin_bindings', b] for b in small], [])
  gin_lite.clear_config()
  try:
    runner = train.main(args)
    agent = runner._agent
    assert type(agent).__name__ == 'RainbowAgent' and agent.noisy and agent.dueling
    assert agent._double() and agent.online_convnet.n_out == 153 and agent._mlp is not None
    assert agent.training_steps >= 400 and agent._opt_steps >= 40 and agent._graph_sets
    assert sorted(agent._act) == [False, True]        # trained on noise, evaluated on mu
    assert np.isfinite(agent.mean_loss())
    assert bool(torch.isfinite(agent._loss_out['loss']).all())
    assert bool(torch.isfinite(agent.online_convnet.fp.flat).all())
    with open(os.path.join(base, 'logs', 'log_0'), 'rb') as f:
      it = pickle.load(f)['iteration_0']
    assert it['train_episode_lengths'] and it['eval_episode_lengths']
    assert np.isfinite(it['train_average_return'][0]) and np.isfinite(it['eval_average_return'][0])
    ck = os.path.join(base, 'checkpoints')
    for f in ('ckpt.0', 'sentinel_checkpoint_complete.0', 'tf_ckpt-0', 'add_count_ckpt.0.gz',
              'sum_tree_ckpt.0.gz'):
      assert os.path.exists(os.path.join(ck, f)), f
    params = agent.online_convnet.fp.flat.detach().cpu().clone()
    steps = agent.training_steps
    counters = {r: s.counter.tolist() for r, s in agent._noise.items()}
    assert all(c[0] > 0 and c[1] == 0 for c in counters.values()), counters
    gin_lite.clear_config()
    runner2 = train.main(args)          # resume: a new Runner picks up at iteration 1
    assert runner2._start_iteration == 1
    a2 = runner2._agent
    assert a2.training_steps == steps and a2.noisy
    assert np.array_equal(a2.online_convnet.fp.flat.detach().cpu().numpy(), params.numpy())
    assert int(a2._replay.memory.add_count) == int(agent._replay.memory.add_count)
    # the noise streams continue: the counters are the uninterrupted run's, so the next draw
    # of every role is the one that run makes next
    assert {r: s.counter.tolist() for r, s in a2._noise.items()} == counters
    for r in counters:
      n = agent.online_convnet.noise_numel
      nxt = [x._noise[r].draw(torch.empty(n, device='cuda')).clone() for x in (agent, a2)]
      assert torch.equal(nxt[0], nxt[1])
      assert _noise_is_call(nxt[1].cpu().numpy(), r, counters[r][0])
    # the same checkpoint into a network without the sigmas: unbundle's shape check
    gin_lite.clear_config()
    env, plain = G._make(gin, ['RainbowAgent.noisy = False',
                               'WrappedPrioritizedReplayBuffer.replay_capacity = 5000'])
    assert not plain.noisy and plain._noise is None
    with open(os.path.join(ck, 'ckpt.0'), 'rb') as f:
      bundle = pickle.load(f)
    with pytest.raises(ValueError, match='another network or layout'):
      plain.unbundle(ck, 0, bundle)
  finally:
    gin_lite.clear_config()


def test_noisy_refusals_build_nothing(monkeypatch):
  from dopamine_amd.agents import networks
  from dopamine_amd.agents.dqn.dqn_agent import DQNAgent
  from dopamine_amd.agents.implicit_quantile.implicit_quantile_agent import ImplicitQuantileAgent
  from dopamine_amd.agents.quantile.quantile_agent import QuantileAgent
  from dopamine_amd.agents.rainbow.rainbow_agent import RainbowAgent

  class Group(object):            # a stand-in: construction must not reach a collective
    def __getattr__(self, name):
      raise AssertionError('the process group was used (%s)' % name)

  made = []
  monkeypatch.setattr(DQNAgent, '_build_networks', lambda self: made.append('networks'))
  for cls in (DQNAgent, RainbowAgent, QuantileAgent, ImplicitQuantileAgent):
    monkeypatch.setattr(cls, '_build_replay_buffer', lambda self, staging: made.append('replay'))
  gym = dict(observation_shape=(4, 1), observation_dtype=np.float64, stack_size=1)
  for cls in (DQNAgent, RainbowAgent, QuantileAgent):      # the Nature-CNN networks
    with pytest.raises(ValueError, match='noisy.*Nature CNN'):
      cls(num_actions=4, replay_capacity=3000, batch_size=32, noisy=True)
  with pytest.raises(ValueError, match='Fourier'):
    DQNAgent(num_actions=2, network=networks.CartpoleFourierDQNNetwork, noisy=True, **gym)
  for cls, net in ((DQNAgent, networks.CartpoleDQNNetwork),
                   (RainbowAgent, networks.CartpoleRainbowNetwork)):
    with pytest.raises(ValueError, match='noisy.*process_group'):
      cls(num_actions=2, network=net, noisy=True, process_group=Group(), **gym)
    for bad in (0.0, -0.5):
      with pytest.raises(ValueError, match='noisy_sigma0'):
        cls(num_actions=2, network=net, noisy=True, noisy_sigma0=bad, **gym)
  with pytest.raises(ValueError, match='noisy'):
    ImplicitQuantileAgent(num_actions=4, replay_capacity=3000, batch_size=16, noisy=True)
  assert not made
