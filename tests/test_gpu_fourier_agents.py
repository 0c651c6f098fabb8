"""dqn_acrobot, dqn_acrobot_fourier and dqn_cartpole_fourier, made as the Runner makes them.

Written the way tests/test_gpu_gym_agents.py is (its helpers are used here): each agent is
created from its gin file by ``run_experiment.create_agent``, its buffer is filled with 3,000
random-action transitions, and it takes 10 gradient steps through ``_train_step`` (eager
steps, then replays of the captured HIP graphs).  Every step is checked against float64 at the
device's parameters of that step:
  * indices bit-exact against the oracle's sampler driven from the same host RNG state, and
    numpy's RNG end state;
  * Q, the target network's Q, the per-sample losses and every parameter gradient within 1e-5
    of their scale (test_gpu_gym_agents.py's ``rel`` measure and bar).  The float64 chain
    starts from the float32 scaled state, as the reference's graph does.  The reference
    arithmetic in its worst, sequential fp32 order reads 2.8e-6 for Q and 1.3e-6 for dW at
    Acrobot's F = 4,095 and B = 256, and 9.4e-7 / 7.0e-7 at CartPole's, on the CPU with the
    float64 chain taken from the float64 state;
  * the optimizer's update from the device's own gradient: plain gradient descent bitwise
    numpy float32 ``var - float32(lr) * g``, TF1 Adam within 5e-8 of float64.
Beside that: the batch-1 acting forward gives the batch forward's row bitwise, a
bundle_and_checkpoint / unbundle round trip with the stateless optimizer, and the PyTorch path
(use_hip_mlp=False) inside the same bars.

Worst readings over the 10 steps, MI355X: READINGS below."""
import os

import numpy as np
import pytest
import torch

from oracle import learner as OL
from tests import fourier_cases as FC
from tests import test_gpu_gym_agents as G

pytestmark = pytest.mark.gpu

_CONFIGS = os.path.join(G.ROOT, 'dopamine_amd', 'agents', 'dqn', 'configs')
DQN_ACROBOT = os.path.join(_CONFIGS, 'dqn_acrobot.gin')
DQN_ACROBOT_FOURIER = os.path.join(_CONFIGS, 'dqn_acrobot_fourier.gin')
DQN_CARTPOLE_FOURIER = os.path.join(_CONFIGS, 'dqn_cartpole_fourier.gin')
_GIN = {'dqn_acrobot': DQN_ACROBOT, 'dqn_acrobot_fourier': DQN_ACROBOT_FOURIER,
        'dqn_cartpole_fourier': DQN_CARTPOLE_FOURIER}
TOL = G.TOL
PARAM_ATOL = G.PARAM_ATOL

# worst rel over the 10 steps on the MI355X (gradient: the worst tensor); the Adam update of
# dqn_cartpole_fourier 7.5e-9 on both paths, the SGD updates bitwise
READINGS = """
                                     online    target    loss      gradient
  dqn_acrobot           HIP          3.2e-7    3.0e-7    2.4e-7    1.6e-7
                        PyTorch      2.9e-7    3.1e-7    2.3e-7    3.7e-7
  dqn_acrobot_fourier   HIP          2.1e-6    1.7e-6    2.5e-6    3.0e-6
                        PyTorch      2.3e-6    2.0e-6    2.5e-6    2.7e-6
  dqn_cartpole_fourier  HIP          8.3e-7    1.1e-6    8.0e-7    3.7e-7
                        PyTorch      1.2e-6    1.2e-6    1.2e-6    3.8e-7
"""


def _is_fourier(net):
  from dopamine_amd.agents import networks
  return isinstance(net, networks.FourierDQNNetwork)


def _forward64(net, flat, state):
  """(Q float64, what the backward needs) at the flat parameters ``flat``."""
  if not _is_fourier(net):
    out, ins, P = G._forward64(net, flat, state)
    return out.numpy(), (ins, P)
  s = FC.scale32(np.asarray(state).reshape(len(state), -1), net.MIN, net.MAX)
  phi, _ = FC.phi64(s, net.D, net.order)
  o, shape = net.fp.offsets['out_w']
  w = flat[o:o + int(np.prod(shape))].reshape(shape)
  return phi @ w.T, phi


def _backward64(net, ctx, gout):
  """name -> float64 gradient."""
  if not _is_fourier(net):
    ins, P = ctx
    return {k: v[0] for k, v in G._backward64(net, P, ins, gout).items()}
  return {'out_w': np.asarray(gout, np.float64).T @ ctx}


def run_lockstep(name, bindings=(), steps=10):
  env, agent = G._make(_GIN[name], bindings)
  agent.enable_trace()
  G._fill(env, agent)
  orc = G._oracle(agent, False)
  net, B = agent.online_convnet, agent._batch_size
  cg = np.float64(np.float32(agent.cumulative_gamma))
  U = agent._UNROLL
  errs = dict(online=0.0, target=0.0, loss=0.0, grad={}, params=0.0)
  for _ in range(steps):
    k = agent._opt_steps % 2
    w32 = net.fp.flat.detach().cpu().numpy().copy()
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
    tr = {n: t[U + k].detach().cpu().numpy() for n, t in agent._trace.items()}
    idx = orc.sample_index_batch(B)
    np.testing.assert_array_equal(tr['indices'], idx)
    b = orc.sample_transition_batch(B, indices=idx)
    s, act, rew, ns, term = b[0], b[1], b[2], b[3], b[6]
    np.testing.assert_array_equal(tr['action'], act)
    np.testing.assert_array_equal(tr['reward'], rew)
    np.testing.assert_array_equal(tr['terminal'], term)
    out, ctx = _forward64(net, w, s)
    tout, _ = _forward64(agent.target_convnet, tw, ns)
    assert 'online_out' in tr and 'target_out' in tr
    errs['online'] = max(errs['online'], G._rel(tr['online_out'].reshape(out.shape), out))
    errs['target'] = max(errs['target'], G._rel(tr['target_out'].reshape(tout.shape), tout))
    ref = OL.dqn_huber(out, tout, act, rew, term, cg, dtype=np.float64)
    errs['loss'] = max(errs['loss'], G._rel(tr['loss'], ref['loss']))
    for pname, g64 in _backward64(net, ctx, ref['grad']).items():
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
      assert not np.array_equal(gw, w32)                 # it did move
  agent._discard_prefetch()
  agent._replay.memory.sync_rng()
  a, b = np.random.get_state(), orc.np_rng.get_state()
  assert np.array_equal(a[1], b[1]) and a[2] == b[2]
  return env, agent, errs


def _check(name, agent, errs):
  print('fourier agent errors', name, errs, flush=True)
  assert errs['online'] <= TOL and errs['target'] <= TOL and errs['loss'] <= TOL, errs
  assert max(errs['grad'].values()) <= TOL, errs
  assert errs['params'] <= PARAM_ATOL, errs
  assert agent._graphs is not None            # the later steps replayed the captured graph


def _executor(agent):
  from dopamine_amd.fourier import HipFourier
  from dopamine_amd.mlp import HipMLP
  cls = HipFourier if _is_fourier(agent.online_convnet) else HipMLP
  assert agent._mlp is not None and isinstance(agent._mlp['online'], cls)
  assert all(isinstance(t, cls) for t in agent._mlp['target']) and agent._needs_flat_grad()
  return agent._mlp['online']


@pytest.mark.parametrize('name', sorted(_GIN))
def test_steps_match_float64_oracle(name, tmp_path):
  from dopamine_amd import ops
  env, agent, errs = run_lockstep(name)
  exe = _executor(agent)
  net = agent.online_convnet
  if name == 'dqn_acrobot':
    assert net.sizes == (24, 24) and net.fp.count() == 843
  else:
    assert net.fp.count() == {'dqn_acrobot_fourier': 12285, 'dqn_cartpole_fourier': 510}[name]
    assert 'phi' in exe.acts and all('phi' not in t.acts for t in agent._mlp['target'])
  sgd = name != 'dqn_cartpole_fourier'
  assert isinstance(agent._opt, ops.TF1GradientDescent if sgd else ops.TF1Adam)
  assert agent._batch_size == (256 if sgd else 128)
  _check(name, agent, errs)

  # the batch-1 acting forward (captured graph) gives the batch forward's rows bitwise
  B, D = agent._batch_size, agent.observation_shape[0]
  states = agent._replay.memory._frames.cpu().numpy().view(np.float64).reshape(-1, D)[:B].copy()
  batch_q = exe.forward(torch.from_numpy(states).cuda()).detach().cpu().numpy().copy()
  for i in (0, 1, B - 1):
    q = agent._q_values(states[i].reshape(1, D, 1)).detach().cpu().numpy()
    assert q.shape == (1, agent.num_actions)
    assert np.array_equal(q[0].view(np.uint32), batch_q[i].view(np.uint32)), (name, i)
  assert agent._act is not None and agent._act[3] is not None      # the captured graph served
  if _is_fourier(net):
    assert 'phi' not in agent._act[0].acts

  # bundle_and_checkpoint / unbundle with an optimizer that may have no state
  assert (len(list(agent._opt_tensors())) == 0) == sgd
  bundle = agent.bundle_and_checkpoint(str(tmp_path), 0)
  assert bundle is not None and bundle['_opt_steps'] == 10
  _, fresh = G._make(_GIN[name], [])
  assert not torch.equal(fresh.online_convnet.fp.flat, net.fp.flat)
  assert fresh.unbundle(str(tmp_path), 0, bundle)
  assert torch.equal(fresh.online_convnet.fp.flat, net.fp.flat)
  assert torch.equal(fresh.target_convnet.fp.flat, agent.target_convnet.fp.flat)
  assert fresh.training_steps == agent.training_steps and fresh._opt_steps == 10
  assert int(fresh._replay.memory.add_count) == int(agent._replay.memory.add_count)


@pytest.mark.parametrize('name', sorted(_GIN))
def test_pytorch_path_agrees_within_the_same_bars(name):
  _, agent, errs = run_lockstep(name, ['DQNAgent.use_hip_mlp = False'])
  assert agent._mlp is None
  _check(name + ' use_hip_mlp=False', agent, errs)


def test_defaults_and_refusals():
  """None means on for the Fourier networks; the distributional agents refuse them."""
  from dopamine_amd.agents import networks
  from dopamine_amd.agents.rainbow import rainbow_agent
  _, agent = G._make(DQN_CARTPOLE_FOURIER, [])
  assert agent.use_hip_mlp is None and agent._mlp is not None
  with pytest.raises(ValueError, match='Fourier'):
    rainbow_agent.RainbowAgent(num_actions=3, observation_shape=(6, 1),
                               observation_dtype=np.float64, stack_size=1,
                               network=networks.AcrobotFourierDQNNetwork)
