"""Agents on supports wider than a wave: the 201-atom gym config step by step and end to end,
and a Nature-CNN RainbowAgent with 101 atoms.

The gym agent is made from c51_cartpole_201.gin the way tests/test_gpu_gym_agents.py makes its
agents (its helpers are used), its buffer filled with 3,000 transitions, and it takes 10
gradient steps through ``_train_step`` (eager steps, then replays of the captured HIP graphs).
At every step the device's online and target logits and the batch are read from the trace and
the loss kernel's outputs -- per-sample loss, new priorities, the logit gradient -- are checked
against oracle.learner.c51_loss on those logits with the loss kernels' measure
(oracle/nature_cnn.py cond_ratio at LAYER_TOL on oracle/learner_cases.py c51_checks' Σ|terms|).
The 512 -> 402 output layer is checked once against layer_reference.
"""
import os
import pickle
import random

import numpy as np
import pytest
import torch

from oracle import learner as OL
from oracle import learner_cases as C
from oracle import nature_cnn as ONC
from tests import test_gpu_agent as TA
from tests import test_gpu_gym_agents as G

pytestmark = pytest.mark.gpu

C51_CARTPOLE_201 = os.path.join(G._AGENTS, 'rainbow', 'configs', 'c51_cartpole_201.gin')


def test_c51_cartpole_201_steps_match_float64_oracle():
  env, agent = G._make(C51_CARTPOLE_201, [])
  assert G._uses_hip_mlp(agent)
  assert agent._num_atoms == 201 and agent._vmax == 100.0 and agent._replay_scheme == 'uniform'
  assert agent.update_horizon == 1 and agent.update_period == 1
  agent.enable_trace()
  G._fill(env, agent)
  net, B, A, N = agent.online_convnet, agent._batch_size, agent.num_actions, agent._num_atoms
  assert (B, A, N, net.n_out) == (128, 2, 201, 402)
  support = agent._support.cpu().double().numpy()
  assert support[0] == -100 and support[-1] == 100
  cg = np.float64(np.float32(agent.cumulative_gamma))
  U = agent._UNROLL
  worst = {}
  for step in range(10):
    k = agent._opt_steps % 2
    w = net.fp.flat.detach().cpu().double().numpy().copy()
    before = agent._opt_steps
    agent._train_step()
    assert agent._opt_steps == before + 1
    torch.cuda.synchronize()
    tr = {n: t[U + k].detach().cpu().numpy() for n, t in agent._trace.items()}
    ol = tr['online_out'].astype(np.float64).reshape(B, A, N)
    tl = tr['target_out'].astype(np.float64).reshape(B, A, N)
    ref = OL.c51_loss(ol, tl, tr['action'], tr['reward'], tr['terminal'], support, cg, None,
                      dtype=np.float64)
    checks = C.c51_checks(ref)
    del checks['mean_loss']               # the summary mean is not on the gradient path
    got = dict(grad=tr['grad_out'], loss=tr['loss'], priorities=tr['priorities'])
    for name, (r, terms) in checks.items():
      r = np.asarray(r, np.float64)
      v = ONC.assert_layer_close('c51_cartpole_201 step %d %s' % (step, name),
                                 got[name].reshape(r.shape), r, np.asarray(terms, np.float64))
      worst[name] = max(worst.get(name, 0.0), v)
    if step == 0:
      # the 512 -> 402 output layer alone, as tests/test_gpu_mlp_layers.py checks a layer: the
      # float64 layer on the device's own input to it (the last hidden activation of this
      # step's forward) and the device's own upstream gradient
      mlp = agent._mlp['online']
      assert np.array_equal(mlp.acts['out'].cpu().numpy().reshape(-1), tr['online_out'].reshape(-1))
      P = G._params64(net, w)
      head = ONC.layer_reference('fc2', mlp.acts['h%d' % (len(net.sizes) - 1)], P['out_w'],
                                 P['out_b'], torch.from_numpy(tr['grad_out'].reshape(B, A * N)))
      assert tuple(P['out_w'].shape) == (402, 512)
      ONC.assert_layer_close('head z', tr['online_out'].reshape(B, A * N), head['z'], head['z_abs'])
      for pname, key in (('out_w', 'dw'), ('out_b', 'db')):
        o, shape = net.fp.offsets[pname]
        ONC.assert_layer_close('head ' + pname, tr['grad'][o:o + int(np.prod(shape))],
                               head[key].reshape(-1), head[key + '_abs'].reshape(-1))
  print('c51_cartpole_201 worst ratios over 10 steps', worst, flush=True)
  assert agent._graphs is not None            # the later steps replayed the captured graph
  assert bool(torch.isfinite(net.fp.flat).all())


def test_c51_cartpole_201_experiment_runs_logs_and_checkpoints(tmp_path):
  """c51_cartpole_201.gin through train.py for one short iteration."""
  from dopamine_amd import gin_lite
  from dopamine_amd.discrete_domains import train
  small = ['Runner.training_steps = 300', 'Runner.evaluation_steps = 100',
           'Runner.max_steps_per_episode = 100', 'RainbowAgent.min_replay_history = 100',
           'WrappedPrioritizedReplayBuffer.replay_capacity = 5000', 'Runner.num_iterations = 1']
  base = str(tmp_path / 'cartpole201')
  args = ['--base_dir', base, '--gin_files', C51_CARTPOLE_201] + sum(
      [['--gin_bindings', b] for b in small], [])
  gin_lite.clear_config()
  try:
    runner = train.main(args)
  finally:
    gin_lite.clear_config()
  agent = runner._agent
  assert G._uses_hip_mlp(agent) and agent._num_atoms == 201 and agent._vmax == 100.0
  assert agent.training_steps >= 300 and agent._opt_steps >= 100 and agent._graph_sets
  with open(os.path.join(base, 'logs', 'log_0'), 'rb') as f:
    logs = pickle.load(f)
  it = logs['iteration_0']
  assert it['train_episode_lengths'] and it['eval_episode_lengths']
  assert np.isfinite(it['train_average_return'][0]) and np.isfinite(it['eval_average_return'][0])
  assert bool(torch.isfinite(agent.online_convnet.fp.flat).all())
  ck = os.path.join(base, 'checkpoints')
  for f in ('ckpt.0', 'sentinel_checkpoint_complete.0', 'tf_ckpt-0', 'add_count_ckpt.0.gz'):
    assert os.path.exists(os.path.join(ck, f)), f


def _nature(**kw):
  random.seed(11); np.random.seed(11); torch.manual_seed(11)
  return TA._rainbow(4, num_atoms=101, **kw)


def test_nature_cnn_rainbow_with_101_atoms_steps_on_stored_logits():
  """Above 64 atoms the Nature-CNN RainbowAgent reports _fused() false: one eager step's loss
  matches the float64 oracle on the same batch and weights, and three steps leave bitwise the
  parameters of the same agent constructed with fused_head=False."""
  A, N = 4, 101
  a = _nature(use_hip_graph=False)
  assert a.fused_head and not a._fused()
  w0 = a.online_convnet.fp.flat.detach().cpu().clone()
  tw = a.target_convnet.fp.flat.detach().cpu().clone()
  a._run_train_op()
  torch.cuda.synchronize()
  t = {k: v.detach().cpu() for k, v in a._replay.transition.items()}
  from dopamine_amd.agents.networks import RainbowNetwork
  on = RainbowNetwork(A, num_atoms=N, device='cpu'); on.fp.flat.copy_(w0)
  tg = RainbowNetwork(A, num_atoms=N, device='cpu'); tg.fp.flat.copy_(tw)
  with torch.no_grad():
    tl = tg(t['next_state']).double().numpy().reshape(-1, A, N)
    ol = on(t['state']).double().numpy().reshape(-1, A, N)
  exp = OL.c51_loss(ol, tl, t['action'].numpy(), t['reward'].numpy(), t['terminal'].numpy(),
                    OL.c51_support(10.0, N, np.float32), np.float32(0.99 ** 3),
                    t['sampling_probabilities'].numpy())
  np.testing.assert_allclose(a._loss_out['loss'].cpu().numpy(), exp['loss'], rtol=1e-4, atol=1e-5)
  params = []
  for kw in (dict(), dict(fused_head=False)):
    b = _nature(**kw)
    for _ in range(3):
      b._run_train_op()
    torch.cuda.synchronize()
    assert not b._fused()
    params.append(b.online_convnet.fp.flat.detach().cpu().numpy().copy())
  assert np.array_equal(params[0], params[1])
  assert not np.array_equal(params[0], w0.numpy())
