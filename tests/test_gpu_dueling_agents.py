"""DQNAgent / RainbowAgent / QuantileAgent with dueling=True: every gradient step against
float64 at the device's parameters AS THEY WERE BEFORE THAT STEP.

The pattern, the helpers, the bars and the near-tie rule are tests/test_gpu_double_dqn_agents.py's
and tests/test_gpu_quantile_agents.py's (TOL 1e-5, PARAM_ATOL 5e-8, the 'rel' gradient
measure).  The classic-control agents are made from their gin files and take 10 gradient steps
through ``_train_step`` -- eager steps, then replays of the captured graphs.  The float64
reference is the raw forward of the pre-step parameters (the last layer has (A + 1) * N
outputs), tests/dueling_cases.py's float64 combine on it, the existing loss references
(tests/double_dqn_cases.py, tests/qr_cases.py) on the combined outputs, the float64 dueling
backward of their gradient, and the float64 network backward fed with that.  Per step the traced
``online_head_out`` (raw), ``online_out`` / ``target_out`` / ``online_next_out`` (combined), the
loss, the priorities, every parameter gradient and the Adam / SGD update are compared.  The
-pytorch run (use_hip_mlp = False) takes the networks' torch expression and autograd: an
independent statement of the same definition.

Near ties: DD._near_tie_astar as it stands; the count is printed; more than one sample in
eight of any step fails.  Seeds are the helpers' fixed ones.
"""
import os
import pickle
import random

import numpy as np
import pytest
import torch

from oracle import learner_cases as C
from oracle import nature_cnn as ONC
from tests import double_dqn_cases as D
from tests import dueling_cases as DC
from tests import fourier_cases as FC
from tests import qr_cases as Q
from tests import test_gpu_agent as TA
from tests import test_gpu_double_dqn_agents as DD
from tests import test_gpu_fourier_agents as F
from tests import test_gpu_gym_agents as G
from tests import test_gpu_quantile_agents as QA

pytestmark = pytest.mark.gpu

_AGENTS = os.path.join(G.ROOT, 'dopamine_amd', 'agents')
_GIN = {
    'dueling_double_dqn_acrobot': ('dqn/configs/dueling_double_dqn_acrobot.gin', []),
    'dueling_rainbow_cartpole': ('rainbow/configs/dueling_rainbow_cartpole.gin', []),
    'dueling_quantile_cartpole': ('quantile/configs/dueling_quantile_cartpole.gin', []),
    'dueling_rainbow_cartpole-pytorch': ('rainbow/configs/dueling_rainbow_cartpole.gin',
                                         ['RainbowAgent.use_hip_mlp = False']),
}
TOL, PARAM_ATOL = G.TOL, G.PARAM_ATOL


def _kind(agent):
  return {'DQNAgent': 'dqn', 'RainbowAgent': 'rainbow', 'QuantileAgent': 'quantile'}[
      type(agent).__name__]


def _combine64(head, A, n):
  """The float64 combined output (B, A * n) of a raw head (B, (A + 1) * n)."""
  return DC.forward64(head, A, n)[0].reshape(len(head), A * n)


def _loss_reference(agent, kind, out, tout, sout, act, rew, term, cg, probs, tr_loss):
  """(float64 loss reference on the combined outputs at the near-tie-resolved a*, near ties)."""
  B, A = agent._batch_size, agent.num_actions
  if kind == 'quantile':
    c = QA._case(B, A, agent._num_atoms, out, tout, sout, act, rew, term, cg, probs)
    return QA._reference(c, agent.kappa, probs is not None, tr_loss)
  if kind == 'rainbow':
    N = agent._num_atoms
    c = dict(B=B, A=A, N=N, ol=out.reshape(B, A, N), tl=tout.reshape(B, A, N),
             sl=sout.reshape(B, A, N), act=act, rew=rew, term=term, cg=cg,
             z=agent._support.cpu().double().numpy(), probs=probs)
    reference = lambda astar: D.c51_double_reference(c, probs is not None, astar=astar)
    qs = D.select_q(c)
  else:
    c = dict(B=B, A=A, oq=out, tq=tout, sq=sout, act=act, rew=rew, term=term, cg=cg)
    reference = lambda astar: D.dqn_double_reference(c, astar=astar)
    qs = np.asarray(sout, np.float64)
  astar, near = DD._near_tie_astar(qs, lambda a: reference(a)['loss'], tr_loss)
  return reference(astar), near


def run_lockstep(name, steps=10):
  gin, bindings = _GIN[name]
  env, agent = G._make(os.path.join(_AGENTS, gin), bindings)
  kind = _kind(agent)
  assert agent.dueling is True and not agent._fused()
  assert agent.online_convnet.dueling and agent.target_convnet.dueling
  double = agent._double()
  prioritized = kind != 'dqn'
  per = prioritized and agent._replay_scheme == 'prioritized'
  agent.enable_trace()
  G._fill(env, agent)
  orc = G._oracle(agent, prioritized)
  net, B, A = agent.online_convnet, agent._batch_size, agent.num_actions
  n = getattr(agent, '_num_atoms', None) or 1
  assert net.n_out == (A + 1) * n
  cg = np.float64(np.float32(agent.cumulative_gamma))
  U = agent._UNROLL
  errs = dict(head=0.0, online=0.0, target=0.0, online_next=0.0, loss=0.0, priorities=0.0,
              grad={}, params=0.0, near_ties=0)
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
    head, ctx = F._forward64(net, w, s)                      # the raw head (B, (A + 1) * n)
    assert head.shape == (B, (A + 1) * n)
    out = _combine64(head, A, n)
    tout = _combine64(F._forward64(agent.target_convnet, tw, ns)[0], A, n)
    sout = tout
    errs['head'] = max(errs['head'], G._rel(tr['online_head_out'].reshape(head.shape), head))
    if double:
      sout = _combine64(F._forward64(net, w, ns)[0], A, n)   # ONLINE parameters on next_state
      errs['online_next'] = max(errs['online_next'],
                                G._rel(tr['online_next_out'].reshape(sout.shape), sout))
    else:
      assert 'online_next_out' not in tr
    if 'online_out' in tr and 'target_out' in tr:   # (the Rainbow agents' PyTorch path traces none)
      errs['online'] = max(errs['online'], G._rel(tr['online_out'].reshape(out.shape), out))
      errs['target'] = max(errs['target'], G._rel(tr['target_out'].reshape(tout.shape), tout))
    else:
      assert agent._mlp is None and kind != 'dqn'
    ref, near = _loss_reference(agent, kind, out, tout, sout, act, rew, term, cg,
                                b[8] if per else None, tr['loss'])
    errs['near_ties'] += near
    print('%s step %d: %d near ties of %d samples' % (name, step, near, B), flush=True)
    assert near * 8 <= B, 'step %d: %d of %d samples are near ties' % (step, near, B)
    errs['loss'] = max(errs['loss'], G._rel(tr['loss'], ref['loss']))
    if per:
      errs['priorities'] = max(errs['priorities'], float(
          (np.abs(tr['priorities'] - ref['priorities']) / np.abs(ref['priorities'])).max()))
    dhead = DC.backward64(ref['grad'].reshape(B, A, n), A, n)[0]
    for pname, g64 in F._backward64(net, ctx, dhead).items():
      o, shape = net.fp.offsets[pname]
      got = tr['grad'][o:o + int(np.prod(shape))]
      errs['grad'][pname] = max(errs['grad'].get(pname, 0.0), G._rel(got, g64.reshape(-1)))
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
      assert not np.array_equal(gw, w32)
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
def test_dueling_steps_match_float64_at_the_pre_step_parameters(name):
  from dopamine_amd import ops
  from dopamine_amd.mlp import HipMLP
  agent, errs = run_lockstep(name)
  print('dueling agent errors', name, errs, flush=True)
  if name.endswith('-pytorch'):
    assert agent._mlp is None and agent._online_next is None
  else:
    exes = [agent._mlp['online']] + agent._mlp['target']
    if agent._double():
      exes.append(agent._online_next)
    assert all(isinstance(e, HipMLP) and e.dueling for e in exes)
  if name == 'dueling_double_dqn_acrobot':
    assert isinstance(agent._opt, ops.TF1GradientDescent) and agent._double()
    assert agent.online_convnet.sizes == (24, 24) and agent.online_convnet.n_out == 4
  if name.startswith('dueling_rainbow_cartpole'):
    assert agent._double() and agent._replay_scheme == 'prioritized' and agent.update_horizon == 3
    assert agent.online_convnet.n_out == 3 * 51
  if name == 'dueling_quantile_cartpole':
    assert not agent._double() and agent.online_convnet.n_out == 600
  assert errs['head'] > 0 and errs['head'] <= TOL, errs
  assert errs['online_next'] <= TOL, errs
  assert errs['online'] <= TOL and errs['target'] <= TOL and errs['loss'] <= TOL, errs
  assert errs['priorities'] <= TOL, errs
  assert max(errs['grad'].values()) <= TOL, errs
  assert errs['params'] <= PARAM_ATOL, errs
  assert agent._graphs is not None            # the later steps replayed the captured graph


@pytest.mark.parametrize('name', ['dueling_rainbow_cartpole', 'dueling_double_dqn_acrobot'])
def test_per_call_steps_and_chunk_graphs_are_bitwise_equal(name):
  """2 * _UNROLL + 1 gradient steps one per call (eager, then per-step graphs) and the same
  number through train_gradient_steps: bitwise equal parameters, optimizer state and sum tree."""
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
    assert a._opt_steps == n and a.dueling
    a._discard_prefetch()
    a._replay.memory.sync_rng()
    torch.cuda.synchronize()
    st = dict(online=a.online_convnet.fp.flat.cpu().numpy(),
              target=a.target_convnet.fp.flat.cpu().numpy(),
              **{'opt_' + key: t.cpu().numpy() for key, t in a._opt_tensors()})
    if _kind(a) != 'dqn':
      st['tree'] = a._replay.memory.sum_tree.nodes[-1].copy()
    res.append(st)
  QA._same(res)
  assert not np.array_equal(res[0]['online'], res[0]['target'])


# ================================================================================== acting
def _q64(agent, kind, out):
  A = agent.num_actions
  if kind == 'dqn':
    return out.reshape(1, A)
  rows = torch.from_numpy(out.reshape(1, A, agent._num_atoms))
  if kind == 'quantile':
    return rows.mean(-1).numpy()
  return (torch.softmax(rows, -1) * agent._support.cpu().double()).sum(-1).numpy()


@pytest.mark.parametrize('graph', [True, False], ids=['graph', 'no-graph'])
@pytest.mark.parametrize('name', ['dueling_double_dqn_acrobot', 'dueling_rainbow_cartpole',
                                  'dueling_quantile_cartpole'])
def test_acting_q_values_match_float64(name, graph):
  gin = os.path.join(_AGENTS, _GIN[name][0])
  cls = {'dueling_double_dqn_acrobot': 'DQNAgent', 'dueling_rainbow_cartpole': 'RainbowAgent',
         'dueling_quantile_cartpole': 'QuantileAgent'}[name]
  env, agent = G._make(gin, ['%s.use_hip_graph = %s' % (cls, graph)])
  kind = _kind(agent)
  assert agent._mlp is not None and agent.dueling
  net = agent.online_convnet
  with torch.no_grad():     # non-zero biases, as after training
    for pname, prm in net.fp.params.items():
      if pname.endswith('_b'):
        prm.uniform_(-0.05, 0.1)
  w = net.fp.flat.detach().cpu().double().numpy()
  D_, A = agent.observation_shape[0], agent.num_actions
  n = getattr(agent, '_num_atoms', None) or 1
  obs = env.reset()
  for i in range(4):
    agent._reset_state()
    agent._record_observation(obs)
    q = agent._q_values(agent.state).detach().cpu().numpy()
    assert q.shape == (1, A)
    head, _ = F._forward64(net, w, np.asarray(obs).reshape(1, D_))
    want = _q64(agent, kind, _combine64(head, A, n))
    assert G._rel(q, want) <= TOL, (i, q, want)
    obs, _, _, _ = env.step(i % A)
  assert agent._act is not None and (agent._act[3] is not None) == graph
  assert agent._act[0].dueling


# ============================================================================== Nature CNN
def _nature(kind, **kw):
  from dopamine_amd.agents.dqn.dqn_agent import DQNAgent
  from dopamine_amd.agents.quantile.quantile_agent import QuantileAgent
  random.seed(5); np.random.seed(5); torch.manual_seed(5)
  if kind == 'rainbow':
    return TA._rainbow(4, dueling=True, **kw)
  if kind == 'quantile':
    a = QuantileAgent(num_actions=4, num_atoms=101, update_horizon=3, replay_capacity=3000,
                      batch_size=32, min_replay_history=100, dueling=True, **kw)
  else:
    a = DQNAgent(num_actions=4, replay_capacity=3000, batch_size=32, min_replay_history=100,
                 dueling=True, **kw)
  TA._fill(a._replay.memory, 4, 3)
  return a


@pytest.mark.parametrize('kind', ['rainbow', 'dqn', 'quantile'])
def test_nature_cnn_dueling_steps(kind):
  """5 steps -- the first, non-pipelined one, 3 eager pipelined ones, then a replay of the
  captured graphs: the traced raw head and combined outputs against oracle/nature_cnn.py's
  float64 forward at the pre-step parameters and the float64 combine; loss, priorities and the
  output gradient against the reference evaluated on the traced outputs."""
  from dopamine_amd.cnn import HipNatureCNN
  a = _nature(kind)
  assert a._hip is not None and a.dueling and a._online_next is None
  assert a.fused_head and a._rides() and not a._fused()
  assert all(isinstance(e, HipNatureCNN) and e.dueling
             for e in [a._hip['online']] + a._hip['target'])
  a.enable_trace()
  B, A, U = a._batch_size, a.num_actions, a._UNROLL
  n = getattr(a, '_num_atoms', None) or 1
  assert a._hip['online'].n_out == (A + 1) * n and B == 32
  assert n == {'rainbow': 51, 'dqn': 1, 'quantile': 101}[kind]
  offsets = a.online_convnet.fp.offsets
  cg = np.float64(np.float32(a.cumulative_gamma))
  per = kind != 'dqn'
  worst = dict(head=0.0, online=0.0, target=0.0)
  fwd = lambda w, x: ONC.forward(ONC.Params64(w, offsets),
                                 ONC.to_input(np.moveaxis(x, 1, -1))).numpy()
  for step in range(5):
    k = a._opt_steps % 2
    w = a.online_convnet.fp.flat.detach().cpu().double().numpy().copy()
    tw = a.target_convnet.fp.flat.detach().cpu().double().numpy().copy()
    for _ in range(a.update_period):
      a._train_step()
    torch.cuda.synchronize()
    assert (a._graphs is not None) == (step >= 3)
    tr = {key: t[U + k].detach().cpu().numpy() for key, t in a._trace.items()}
    with torch.no_grad():
      head = fwd(w, tr['state'])
      thead = fwd(tw, tr['next_state'])
    assert head.shape == (B, (A + 1) * n)
    worst['head'] = max(worst['head'], G._rel(tr['online_head_out'], head))
    worst['online'] = max(worst['online'], G._rel(tr['online_out'], _combine64(head, A, n)))
    worst['target'] = max(worst['target'], G._rel(tr['target_out'], _combine64(thead, A, n)))
    assert tr['online_out'].shape == (B, A * n) and tr['grad_out'].size == B * A * n
    ref, near = _loss_reference(a, kind, tr['online_out'], tr['target_out'], tr['target_out'],
                                tr['action'], tr['reward'], tr['terminal'], cg,
                                tr['sampling_probabilities'] if per else None, tr['loss'])
    what = 'nature dueling %s step %d' % (kind, step)
    print('%s: %d near ties' % (what, near), flush=True)
    assert near * 8 <= B
    checks = {'rainbow': C.c51_checks, 'dqn': C.dqn_checks, 'quantile': Q.qr_checks}[kind](ref)
    checks.pop('mean_loss')
    got = dict(grad=tr['grad_out'], loss=tr['loss'])
    if per:
      got['priorities'] = tr['priorities']
    for key, (r, terms) in checks.items():
      r = np.asarray(r, np.float64)
      ONC.assert_layer_close('%s %s' % (what, key), got[key].reshape(r.shape), r,
                             np.asarray(terms, np.float64))
  print('nature dueling %s worst rel' % kind, worst, flush=True)
  assert max(worst.values()) <= TOL, worst


def test_nature_cnn_dueling_rainbow_schedules_are_bitwise_equal():
  res = []
  for chunked in (False, True):
    a = _nature('rainbow')
    n = 2 * a._UNROLL + 1
    if chunked:      # three eager steps, then chunks of _UNROLL steps, the rest per step
      a.train_gradient_steps(n)
      assert any(isinstance(key, tuple) and key[0] == 'chunk' for key in a._graph_sets)
    else:
      for _ in range(a.update_period * n):
        a._train_step()
    assert a._opt_steps == n and not a._fused() and a.dueling
    res.append(QA._state(a))
  QA._same(res)


def test_fused_paths_refuse_a_dueling_network():
  from dopamine_amd import cnn
  from dopamine_amd.agents import networks
  on = cnn.HipNatureCNN(networks.NatureDQNNetwork(4, dueling=True), 2)
  tg = cnn.HipNatureCNN(networks.NatureDQNNetwork(4, dueling=True, seed=1), 2)
  x = torch.zeros((2, 84, 84, 4), device='cuda')
  with pytest.raises(ValueError, match='dueling'):
    cnn.forward_fused(on, x, tg)
  with pytest.raises(ValueError, match='dueling'):
    cnn.fc2_parts(on)


# ============================================================================== the rest
def test_dueling_rainbow_experiment_runs_checkpoints_resumes_and_refuses_the_other_kind(tmp_path):
  from dopamine_amd import gin_lite
  from dopamine_amd.discrete_domains import train
  small = ['Runner.training_steps = 400', 'Runner.evaluation_steps = 100',
           'RainbowAgent.min_replay_history = 200', 'Runner.num_iterations = 1',
           'WrappedPrioritizedReplayBuffer.replay_capacity = 5000']
  base = str(tmp_path / 'dueling_rainbow_cartpole')
  gin = os.path.join(_AGENTS, _GIN['dueling_rainbow_cartpole'][0])
  args = ['--base_dir', base, '--gin_files', gin] + sum([['--gin_bindings', b] for b in small], [])
  gin_lite.clear_config()
  try:
    runner = train.main(args)
    agent = runner._agent
    assert type(agent).__name__ == 'RainbowAgent' and agent.dueling and agent._double()
    assert agent.online_convnet.n_out == 153 and agent._mlp is not None
    assert agent.training_steps >= 400 and agent._opt_steps >= 40 and agent._graph_sets
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
    gin_lite.clear_config()
    runner2 = train.main(args)          # resume: a new Runner picks up at iteration 1
    assert runner2._start_iteration == 1
    a2 = runner2._agent
    assert a2.training_steps == steps and a2.dueling
    assert np.array_equal(a2.online_convnet.fp.flat.detach().cpu().numpy(), params.numpy())
    assert int(a2._replay.memory.add_count) == int(agent._replay.memory.add_count)
    # the same checkpoint into a network without the value stream: unbundle's shape check
    gin_lite.clear_config()
    env, plain = G._make(gin, ['RainbowAgent.dueling = False',
                               'WrappedPrioritizedReplayBuffer.replay_capacity = 5000'])
    assert not plain.dueling and plain.online_convnet.n_out == 102
    with open(os.path.join(ck, 'ckpt.0'), 'rb') as f:
      bundle = pickle.load(f)
    with pytest.raises(ValueError, match='another network or layout'):
      plain.unbundle(ck, 0, bundle)
  finally:
    gin_lite.clear_config()


def test_dueling_refusals_build_nothing(monkeypatch):
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
  for cls in (DQNAgent, RainbowAgent):
    with pytest.raises(ValueError, match='dueling.*process_group'):
      cls(num_actions=4, replay_capacity=3000, batch_size=32, dueling=True, process_group=Group())
  with pytest.raises(ValueError, match='Fourier'):
    DQNAgent(num_actions=2, network=networks.CartpoleFourierDQNNetwork, dueling=True)
  with pytest.raises(ValueError, match='Fourier'):
    RainbowAgent(num_actions=2, network=networks.CartpoleFourierDQNNetwork, dueling=True)
  with pytest.raises(ValueError, match='dueling'):
    ImplicitQuantileAgent(num_actions=4, replay_capacity=3000, batch_size=16, dueling=True)
  assert not made


def test_hip_mlp_refuses_a_dueling_head_wider_than_1024():
  from dopamine_amd.agents import networks
  from dopamine_amd.mlp import HipMLP
  ok = networks.CartpoleRainbowNetwork(3, num_atoms=256, dueling=True)        # (3 + 1) * 256
  assert HipMLP(ok, 2).n_out == 1024
  wide = networks.CartpoleRainbowNetwork(4, num_atoms=205, dueling=False)     # 820 without,
  assert HipMLP(wide, 2).n_out == 820
  wide = networks.CartpoleRainbowNetwork(4, num_atoms=205, dueling=True)      # 1025 with it
  with pytest.raises(ValueError, match='unsupported geometry.*n_out=1025'):
    HipMLP(wide, 2)
