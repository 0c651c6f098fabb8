"""DQNAgent with munchausen=True: every gradient step against float64 at the device's parameters
AS THEY WERE BEFORE THAT STEP.

The classic-control agents are made from their gin files and driven as
tests/test_gpu_double_dqn_agents.py drives its own (the helpers and bars of
tests/test_gpu_gym_agents.py: TOL 1e-5, PARAM_ATOL 5e-8, the 'rel' gradient measure): 10
gradient steps through ``_train_step`` -- eager steps, then replays of the captured graphs.  Per
step the traced ``target_cur_out`` is compared with the float64 forward of the pre-step TARGET
parameters on state, and loss and every parameter gradient with the Munchausen reference
(tests/munchausen_cases.py) built from the float64 outputs.  The soft value and the clipped
log-policy are continuous in the outputs, so no near-tie allowance is needed.

The Nature-CNN agent (stored outputs, then dq_mdqn_loss: _fused() is False) is checked on its
traced outputs, and per-call steps and chunk graphs must leave bitwise equal parameters and
optimizer state.
"""
import os
import random

import numpy as np
import pytest
import torch

from oracle import learner_cases as C
from oracle import nature_cnn as ONC
from tests import dueling_cases as DC
from tests import fourier_cases as FC
from tests import munchausen_cases as M
from tests import test_gpu_agent as TA
from tests import test_gpu_fourier_agents as F
from tests import test_gpu_gym_agents as G

pytestmark = pytest.mark.gpu

_CONFIGS = os.path.join(G.ROOT, 'dopamine_amd', 'agents', 'dqn', 'configs')
_NAMES = ('mdqn_acrobot', 'mdqn_cartpole', 'dueling_mdqn_acrobot')
TOL, PARAM_ATOL = G.TOL, G.PARAM_ATOL


def _case(agent, out, tout, tcur, act, rew, term):
  f = np.float32
  return dict(B=agent._batch_size, A=agent.num_actions, oq=out, tq=tout, tqc=tcur, act=act,
              rew=rew, term=term, cg=f(agent.cumulative_gamma), tau=f(agent.munchausen_tau),
              alpha=f(agent.munchausen_alpha), clip=f(agent.munchausen_clip))


def run_lockstep(name, steps=10):
  env, agent = G._make(os.path.join(_CONFIGS, name + '.gin'), [])
  assert agent.munchausen is True and agent._munchausen() and not agent._double()
  assert (agent.munchausen_tau, agent.munchausen_alpha, agent.munchausen_clip) == (0.03, 0.9, -1.0)
  agent.enable_trace()
  G._fill(env, agent)
  orc = G._oracle(agent, False)
  net, tnet, B, A = agent.online_convnet, agent.target_convnet, agent._batch_size, agent.num_actions
  dueling = agent.dueling
  combine = (lambda h: DC.forward64(h, A, 1)[0].reshape(len(h), A)) if dueling else (lambda h: h)
  U = agent._UNROLL
  errs = dict(online=0.0, target=0.0, target_cur=0.0, loss=0.0, grad_out=0.0, grad={}, params=0.0)
  for step in range(steps):
    k = agent._opt_steps % 2
    w32 = net.fp.flat.detach().cpu().numpy().copy()          # the parameters BEFORE this step
    w = w32.astype(np.float64)
    tw = tnet.fp.flat.detach().cpu().double().numpy().copy()
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
    head, ctx = F._forward64(net, w, s)
    out = combine(head)
    tout = combine(F._forward64(tnet, tw, ns)[0])
    tcur = combine(F._forward64(tnet, tw, s)[0])             # TARGET parameters on state
    assert 'online_next_out' not in tr
    errs['online'] = max(errs['online'], G._rel(tr['online_out'].reshape(out.shape), out))
    errs['target'] = max(errs['target'], G._rel(tr['target_out'].reshape(tout.shape), tout))
    errs['target_cur'] = max(errs['target_cur'],
                             G._rel(tr['target_cur_out'].reshape(tcur.shape), tcur))
    ref = M.mdqn_reference(_case(agent, out, tout, tcur, act, rew, term))
    errs['loss'] = max(errs['loss'], G._rel(tr['loss'], ref['loss']))
    errs['grad_out'] = max(errs['grad_out'], G._rel(tr['grad_out'], ref['grad']))
    dhead = DC.backward64(ref['grad'].reshape(B, A, 1), A, 1)[0] if dueling else ref['grad']
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
  agent._discard_prefetch()
  agent._replay.memory.sync_rng()
  a, b = np.random.get_state(), orc.np_rng.get_state()
  assert np.array_equal(a[1], b[1]) and a[2] == b[2]
  return agent, errs


@pytest.mark.parametrize('name', _NAMES)
def test_munchausen_steps_match_float64_at_the_pre_step_parameters(name):
  from dopamine_amd import ops
  from dopamine_amd.mlp import HipMLP
  agent, errs = run_lockstep(name)
  print('munchausen agent errors', name, errs, flush=True)
  if name == 'mdqn_cartpole':                  # config 1's network keeps its PyTorch path
    assert agent._mlp is None and agent._target_cur is None and not agent.dueling
    assert isinstance(agent._opt, ops.TF1Adam)
  else:
    assert isinstance(agent._target_cur, HipMLP)
    assert type(agent._target_cur) is type(agent._mlp['target'][0])
    assert agent._target_cur.dueling == agent.dueling == (name == 'dueling_mdqn_acrobot')
    assert isinstance(agent._opt, ops.TF1GradientDescent) and agent.online_convnet.sizes == (24, 24)
    assert agent.online_convnet.n_out == (4 if agent.dueling else 3)
  assert not agent._fused() and agent._online_next is None
  assert 0 < errs['target_cur'] <= TOL, errs
  assert errs['online'] <= TOL and errs['target'] <= TOL and errs['loss'] <= TOL, errs
  assert errs['grad_out'] <= TOL, errs
  assert max(errs['grad'].values()) <= TOL, errs
  assert errs['params'] <= PARAM_ATOL, errs
  assert agent._graphs is not None            # the later steps replayed the captured graph


# ============================================================================ Nature CNN
def _nature(**kw):
  from dopamine_amd.agents.dqn.dqn_agent import DQNAgent
  random.seed(5); np.random.seed(5); torch.manual_seed(5)
  a = DQNAgent(num_actions=4, replay_capacity=3000, batch_size=32, min_replay_history=100,
               munchausen=True, **kw)
  TA._fill(a._replay.memory, 4, 3)
  return a


def test_nature_cnn_munchausen_steps():
  """7 steps -- the first, non-pipelined one (nothing is prefetched yet), 3 eager pipelined
  ones, then 3 replays of the captured graphs: target_cur_out against oracle/nature_cnn.py's
  float64 forward of the TARGET parameters on state; loss and the output gradient against the
  Munchausen reference evaluated on the traced outputs."""
  from dopamine_amd.cnn import HipNatureCNN
  a = _nature()
  assert a._hip is not None and isinstance(a._target_cur, HipNatureCNN)
  assert a.fused_head and a._rides() and not a._fused()
  a.enable_trace()
  B, A, U = a._batch_size, a.num_actions, a._UNROLL
  assert (B, A) == (32, 4)
  offsets = a.target_convnet.fp.offsets
  worst = 0.0
  for step in range(7):
    k = a._opt_steps % 2
    tw = a.target_convnet.fp.flat.detach().cpu().double().numpy().copy()
    for _ in range(a.update_period):
      a._train_step()
    torch.cuda.synchronize()
    # captured after the third eager pipelined step: steps 4, 5, 6 replay
    assert (a._graphs is not None) == (step >= 3)
    assert a._eager_steps == {False: 1, True: min(step, 3)}
    tr = {n: t[U + k].detach().cpu().numpy() for n, t in a._trace.items()}
    with torch.no_grad():
      tcur = ONC.forward(ONC.Params64(tw, offsets),
                         ONC.to_input(np.moveaxis(tr['state'], 1, -1))).numpy()
    worst = max(worst, G._rel(tr['target_cur_out'], tcur))
    what = 'nature mdqn step %d' % step
    c = _case(a, tr['online_out'], tr['target_out'], tr['target_cur_out'], tr['action'],
              tr['reward'], tr['terminal'])
    checks = C.dqn_checks(M.mdqn_reference(c))
    checks.pop('mean_loss')
    got = dict(grad=tr['grad_out'], loss=tr['loss'])
    for key, (ref, terms) in checks.items():
      ref = np.asarray(ref, np.float64)
      ONC.assert_layer_close('%s %s' % (what, key), got[key].reshape(ref.shape), ref,
                             np.asarray(terms, np.float64))
  print('nature mdqn target_cur_out worst rel %.3g' % worst, flush=True)
  assert 0 < worst <= TOL


def _state_of(a):
  a._discard_prefetch()
  a._replay.memory.sync_rng()
  torch.cuda.synchronize()
  return dict(online=a.online_convnet.fp.flat.cpu().numpy(),
              target=a.target_convnet.fp.flat.cpu().numpy(),
              **{'opt_' + key: t.cpu().numpy() for key, t in a._opt_tensors()})


def _same(res):
  assert set(res[0]) == set(res[1])
  for key in res[0]:
    assert res[0][key].shape == res[1][key].shape and res[0][key].size > 0, key
    assert res[0][key].tobytes() == res[1][key].tobytes(), key


def test_nature_cnn_munchausen_schedules_are_bitwise_equal():
  """2 * _UNROLL + 1 gradient steps one per call (eager, then per-step graphs) and the same
  number through train_gradient_steps (chunk graphs): bitwise equal parameters and optimizer
  state."""
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
    res.append(_state_of(a))
  _same(res)


@pytest.mark.parametrize('name', ['mdqn_acrobot', 'dueling_mdqn_acrobot'])
def test_per_call_steps_and_the_learner_loop_are_bitwise_equal(name):
  res = []
  for chunked in (False, True):
    env, a = G._make(os.path.join(_CONFIGS, name + '.gin'), [])
    G._fill(env, a, 2000)             # past the acrobot config's min_replay_history of 1000
    n = 2 * a._UNROLL + 1
    if chunked:
      a.train_gradient_steps(n)
    else:
      for _ in range(a.update_period * n):
        a._train_step()
    assert a._opt_steps == n and a._munchausen()
    res.append(_state_of(a))
  _same(res)
  assert not np.array_equal(res[0]['online'], res[0]['target'])


# ============================================================================== the rest
def test_without_the_flag_no_extra_executor_is_built():
  env, a = G._make(os.path.join(_CONFIGS, 'dqn_acrobot.gin'), [])
  assert a.munchausen is False and not a._munchausen() and a._target_cur is None
  assert a._mlp is not None
  a.enable_trace()
  G._fill(env, a, 1200)
  for _ in range(a.update_period):
    a._train_step()
  torch.cuda.synchronize()
  assert a._opt_steps == 1 and 'target_cur_out' not in a._trace
