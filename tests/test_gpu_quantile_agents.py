"""QuantileAgent (QR-DQN on dq_qr_loss): every gradient step against float64 at the device's
parameters AS THEY WERE BEFORE THAT STEP.

The pattern, the helpers, the bars and the near-tie rule are
tests/test_gpu_double_dqn_agents.py's (TOL 1e-5, PARAM_ATOL 5e-8, the 'rel' gradient measure).
The classic-control agents are made from their gin files and take 10 gradient steps through
``_train_step`` -- eager steps, then replays of the captured graphs.  Per step the traced
outputs (``online_next_out`` too with double-DQN targets) are compared with the float64
forward of the pre-step parameters, and loss, priorities, every parameter gradient and the
Adam update with the reference (tests/qr_cases.py: oracle.learner.iqn_loss on reordered rows)
built from the float64 outputs.

Near ties: a sample whose two best float64 select means lie within 1e-5 max(1, max|Q|) may
match either action's reference (the one its traced loss is closer to).  The count is printed;
more than one sample in eight of any step fails.  Seeds are fixed, so the count is
deterministic.

The Nature-CNN agent (A = 4, N = 101, B = 32; stored outputs, then dq_qr_loss: _fused() is
False) is checked on its traced outputs, and per-call steps and train_gradient_steps (chunk
graphs) must leave bitwise equal parameters, Adam state and sum tree.
"""
import os
import pickle
import random

import numpy as np
import pytest
import torch

from oracle import nature_cnn as ONC
from tests import qr_cases as Q
from tests import test_gpu_agent as TA
from tests import test_gpu_double_dqn_agents as DD
from tests import test_gpu_fourier_agents as F
from tests import test_gpu_gym_agents as G

pytestmark = pytest.mark.gpu

_CONFIGS = os.path.join(G.ROOT, 'dopamine_amd', 'agents', 'quantile', 'configs')
_GIN = {
    'quantile_cartpole': ('quantile_cartpole.gin', []),
    'double_quantile_cartpole': ('double_quantile_cartpole.gin', []),
    'quantile_acrobot': ('quantile_acrobot.gin', []),
    'quantile_cartpole-pytorch': ('quantile_cartpole.gin', ['QuantileAgent.use_hip_mlp = False']),
}
TOL, PARAM_ATOL = G.TOL, G.PARAM_ATOL


def _case(B, A, N, out, tout, sout, act, rew, term, cg, probs):
  return dict(B=B, A=A, N=N, ol=np.reshape(out, (B, A, N)), tl=np.reshape(tout, (B, A, N)),
              sl=np.reshape(sout, (B, A, N)), act=act, rew=rew, term=term, cg=cg, probs=probs)


def _reference(c, kappa, per, tr_loss):
  """(float64 reference at the near-tie-resolved a*, number of near ties)."""
  ref_of = lambda astar: Q.qr_reference(c, kappa, per, astar=astar)
  qs = Q.select_means(c['sl'])
  astar, near = DD._near_tie_astar(qs, lambda a: ref_of(a)['loss'], tr_loss)
  return ref_of(astar), near


def run_lockstep(name, steps=10):
  gin, bindings = _GIN[name]
  env, agent = G._make(os.path.join(_CONFIGS, gin), bindings)
  double = name.startswith('double')
  assert type(agent).__name__ == 'QuantileAgent' and agent._double() == double
  per = agent._replay_scheme == 'prioritized'
  agent.enable_trace()
  G._fill(env, agent)
  orc = G._oracle(agent, True)
  net, B, A, N = agent.online_convnet, agent._batch_size, agent.num_actions, agent._num_atoms
  cg = np.float64(np.float32(agent.cumulative_gamma))
  U = agent._UNROLL
  errs = dict(online=0.0, target=0.0, online_next=0.0, loss=0.0, priorities=0.0, grad={},
              params=0.0, near_ties=0)
  for step in range(steps):
    k = agent._opt_steps % 2
    w = net.fp.flat.detach().cpu().double().numpy().copy()    # the parameters BEFORE this step
    tw = agent.target_convnet.fp.flat.detach().cpu().double().numpy().copy()
    opt = agent._opt
    m, v = opt.m.cpu().double().numpy().copy(), opt.v.cpu().double().numpy().copy()
    st = opt.state.cpu().double().numpy()
    before = agent._opt_steps
    for _ in range(agent.update_period):
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
    np.testing.assert_array_equal(tr['sampling_probabilities'], b[8])
    out, ctx = F._forward64(net, w, s)
    tout, _ = F._forward64(agent.target_convnet, tw, ns)
    sout = tout
    if double:
      sout, _ = F._forward64(net, w, ns)                     # ONLINE parameters on next_state
      errs['online_next'] = max(errs['online_next'],
                                G._rel(tr['online_next_out'].reshape(sout.shape), sout))
    else:
      assert 'online_next_out' not in tr
    if 'online_out' in tr and 'target_out' in tr:   # (the PyTorch path traces none)
      errs['online'] = max(errs['online'], G._rel(tr['online_out'].reshape(out.shape), out))
      errs['target'] = max(errs['target'], G._rel(tr['target_out'].reshape(tout.shape), tout))
    else:
      assert agent._mlp is None
    c = _case(B, A, N, out, tout, sout, act, rew, term, cg, b[8] if per else None)
    ref, near = _reference(c, agent.kappa, per, tr['loss'])
    errs['near_ties'] += near
    print('%s step %d: %d near ties of %d samples' % (name, step, near, B), flush=True)
    assert near * 8 <= B, 'step %d: %d of %d samples are near ties' % (step, near, B)
    errs['loss'] = max(errs['loss'], G._rel(tr['loss'], ref['loss']))
    errs['priorities'] = max(errs['priorities'], float(
        (np.abs(tr['priorities'] - ref['priorities']) / np.abs(ref['priorities'])).max()))
    gout = ref['grad'].reshape(B, -1)
    for pname, g64 in F._backward64(net, ctx, gout).items():
      o, shape = net.fp.offsets[pname]
      got = tr['grad'][o:o + int(np.prod(shape))]
      errs['grad'][pname] = max(errs['grad'].get(pname, 0.0), G._rel(got, g64.reshape(-1)))
    # float64 TF1 Adam from the device's state with the device's gradient
    gw = net.fp.flat.detach().cpu().numpy()
    g = tr['grad'].astype(np.float64)
    f = lambda x: np.float64(np.float32(x))
    b1, b2, lr, eps = f(opt.b1), f(opt.b2), f(opt.lr), f(opt.eps)
    b1p, b2p = st[2 * k], st[2 * k + 1]
    m += (g - m) * (1 - b1)
    v += (g * g - v) * (1 - b2)
    w -= lr * np.sqrt(1 - b2p) / (1 - b1p) * m / (np.sqrt(v) + eps)
    errs['params'] = max(errs['params'], float(np.abs(gw.astype(np.float64) - w).max()))
    if per:           # the next step samples the tree the device wrote
      orc.set_priority(np.asarray(idx, np.int32), tr['priorities'].astype(np.float32))
  agent._discard_prefetch()
  agent._replay.memory.sync_rng()
  assert random.getstate() == orc.py_rng.getstate()
  return agent, errs


@pytest.mark.parametrize('name', sorted(_GIN))
def test_quantile_steps_match_float64_at_the_pre_step_parameters(name):
  from dopamine_amd import ops
  agent, errs = run_lockstep(name)
  print('quantile agent errors', name, errs, flush=True)
  assert isinstance(agent._opt, ops.TF1Adam) and agent._num_atoms == 200 and agent.kappa == 1.0
  assert agent._replay_scheme == 'prioritized' and agent.update_horizon == 3
  assert not agent._fused() and not hasattr(agent, '_vmax')
  if name.endswith('-pytorch'):
    assert agent._mlp is None and agent._online_next is None
  else:
    assert (agent._mlp is not None) == (agent.use_hip_mlp is not False)
  if name.startswith('double') and agent._mlp is not None:
    assert type(agent._online_next) is type(agent._mlp['target'][0])
    assert errs['online_next'] > 0
  assert errs['online_next'] <= TOL, errs
  assert errs['online'] <= TOL and errs['target'] <= TOL and errs['loss'] <= TOL, errs
  assert errs['priorities'] <= TOL, errs
  assert max(errs['grad'].values()) <= TOL, errs
  assert errs['params'] <= PARAM_ATOL, errs
  assert agent._graphs is not None            # the later steps replayed the captured graph
  assert np.isfinite(agent.mean_loss())


def _state(a):
  a._discard_prefetch()
  a._replay.memory.sync_rng()
  torch.cuda.synchronize()
  return dict(online=a.online_convnet.fp.flat.cpu().numpy(),
              target=a.target_convnet.fp.flat.cpu().numpy(),
              tree=a._replay.memory.sum_tree.nodes[-1].copy(),
              **{'opt_' + key: t.cpu().numpy() for key, t in a._opt_tensors()})


def _same(res):
  assert set(res[0]) == set(res[1])
  for key in res[0]:
    assert res[0][key].shape == res[1][key].shape and res[0][key].size > 0, key
    assert res[0][key].tobytes() == res[1][key].tobytes(), key


@pytest.mark.parametrize('name', ['quantile_cartpole', 'double_quantile_cartpole'])
def test_per_call_steps_and_chunk_graphs_are_bitwise_equal(name):
  """2 * _UNROLL + 1 gradient steps one per call (eager, then per-step graphs) and the same
  number through train_gradient_steps: bitwise equal parameters, Adam state and sum tree."""
  res = []
  for chunked in (False, True):
    env, a = G._make(os.path.join(_CONFIGS, _GIN[name][0]), [])
    G._fill(env, a, 1000)
    n = 2 * a._UNROLL + 1
    if chunked:
      a.train_gradient_steps(n)
    else:
      for _ in range(a.update_period * n):
        a._train_step()
    assert a._opt_steps == n
    res.append(_state(a))
  _same(res)
  assert not np.array_equal(res[0]['online'], res[0]['target'])


# ============================================================================ Nature CNN
def _nature(**kw):
  from dopamine_amd.agents.quantile.quantile_agent import QuantileAgent
  random.seed(5); np.random.seed(5); torch.manual_seed(5)
  a = QuantileAgent(num_actions=4, num_atoms=101, update_horizon=3, replay_capacity=3000,
                    batch_size=32, min_replay_history=100, **kw)
  TA._fill(a._replay.memory, 4, 3)
  return a


@pytest.mark.parametrize('double', [False, True], ids=['plain', 'double'])
def test_nature_cnn_quantile_steps(double):
  """5 steps -- the first, non-pipelined one, 3 eager pipelined ones, then a replay of the
  captured graphs: the traced outputs against oracle/nature_cnn.py's float64 forward at the
  pre-step parameters; loss, priorities and the output gradient against the reference
  evaluated on the traced outputs."""
  from dopamine_amd.agents import networks
  from dopamine_amd.cnn import HipNatureCNN
  a = _nature(double_dqn=double)
  assert a.network is networks.RainbowNetwork and a._hip is not None
  assert a.fused_head and a._rides() and not a._fused()
  assert isinstance(a._online_next, HipNatureCNN) == double
  assert a.optimizer.kwargs['learning_rate'] == 0.00005 and a.optimizer.kwargs['epsilon'] == 0.0003125
  a.enable_trace()
  B, A, N, U = a._batch_size, a.num_actions, a._num_atoms, a._UNROLL
  offsets = a.online_convnet.fp.offsets
  cg = np.float64(np.float32(a.cumulative_gamma))
  worst = dict(online=0.0, target=0.0, online_next=0.0)
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
    tr = {n: t[U + k].detach().cpu().numpy() for n, t in a._trace.items()}
    with torch.no_grad():
      worst['online'] = max(worst['online'], G._rel(tr['online_out'], fwd(w, tr['state'])))
      worst['target'] = max(worst['target'], G._rel(tr['target_out'], fwd(tw, tr['next_state'])))
      if double:
        worst['online_next'] = max(worst['online_next'],
                                   G._rel(tr['online_next_out'], fwd(w, tr['next_state'])))
    c = _case(B, A, N, tr['online_out'], tr['target_out'],
              tr['online_next_out'] if double else tr['target_out'], tr['action'], tr['reward'],
              tr['terminal'], cg, tr['sampling_probabilities'])
    ref, near = _reference(c, a.kappa, True, tr['loss'])
    what = 'nature quantile %s step %d' % ('double' if double else 'plain', step)
    print('%s: %d near ties' % (what, near), flush=True)
    assert near * 8 <= B
    checks = Q.qr_checks(ref)
    checks.pop('mean_loss')
    got = dict(grad=tr['grad_out'], loss=tr['loss'], priorities=tr['priorities'])
    for key, (r, terms) in checks.items():
      r = np.asarray(r, np.float64)
      ONC.assert_layer_close('%s %s' % (what, key), got[key].reshape(r.shape), r,
                             np.asarray(terms, np.float64))
  print('nature quantile worst rel', worst, flush=True)
  assert max(worst.values()) <= TOL, worst


def test_nature_cnn_quantile_schedules_are_bitwise_equal():
  res = []
  for chunked in (False, True):
    a = _nature()
    n = 2 * a._UNROLL + 1
    if chunked:      # three eager steps, then chunks of _UNROLL steps, the rest per step
      a.train_gradient_steps(n)
      assert any(isinstance(key, tuple) and key[0] == 'chunk' for key in a._graph_sets)
    else:
      for _ in range(a.update_period * n):
        a._train_step()
    assert a._opt_steps == n and not a._fused()
    res.append(_state(a))
  _same(res)


# ============================================================================== the rest
def test_quantile_cartpole_experiment_runs_logs_checkpoints_and_resumes(tmp_path):
  from dopamine_amd import gin_lite
  from dopamine_amd.discrete_domains import train
  small = ['Runner.training_steps = 400', 'Runner.evaluation_steps = 100',
           'QuantileAgent.min_replay_history = 200', 'Runner.num_iterations = 1',
           'WrappedPrioritizedReplayBuffer.replay_capacity = 5000']
  base = str(tmp_path / 'quantile_cartpole')
  args = ['--base_dir', base, '--gin_files', os.path.join(_CONFIGS, 'quantile_cartpole.gin')] + sum(
      [['--gin_bindings', b] for b in small], [])
  gin_lite.clear_config()
  try:
    runner = train.main(args)
    agent = runner._agent
    assert type(agent).__name__ == 'QuantileAgent' and agent._num_atoms == 200
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
    assert a2.training_steps == steps
    assert np.array_equal(a2.online_convnet.fp.flat.detach().cpu().numpy(), params.numpy())
    assert int(a2._replay.memory.add_count) == int(agent._replay.memory.add_count)
  finally:
    gin_lite.clear_config()


def test_quantile_agent_refuses_a_process_group_vmax_and_fourier_networks(monkeypatch):
  from dopamine_amd.agents import networks
  from dopamine_amd.agents.dqn.dqn_agent import DQNAgent
  from dopamine_amd.agents.quantile.quantile_agent import QuantileAgent

  class Group(object):            # a stand-in: construction must not reach a collective
    def __getattr__(self, name):
      raise AssertionError('the process group was used (%s)' % name)

  made = []
  monkeypatch.setattr(DQNAgent, '_build_networks', lambda self: made.append('networks'))
  monkeypatch.setattr(QuantileAgent, '_build_replay_buffer',
                      lambda self, staging: made.append('replay'))
  with pytest.raises(ValueError, match='process_group'):
    QuantileAgent(num_actions=4, replay_capacity=3000, batch_size=32, process_group=Group())
  with pytest.raises(TypeError, match='vmax'):
    QuantileAgent(num_actions=4, replay_capacity=3000, batch_size=32, vmax=10.0)
  with pytest.raises(ValueError, match='Fourier'):
    QuantileAgent(num_actions=2, network=networks.CartpoleFourierDQNNetwork)
  for bad in (0, 257):
    with pytest.raises(ValueError, match='num_atoms'):
      QuantileAgent(num_actions=4, num_atoms=bad)
  with pytest.raises(ValueError, match='kappa'):
    QuantileAgent(num_actions=4, kappa=0.0)
  assert not made
