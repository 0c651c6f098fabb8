"""DQNAgent / RainbowAgent with double_dqn=True: every gradient step against float64 at the
device's parameters AS THEY WERE BEFORE THAT STEP.

The classic-control agents are made from their gin files and driven as
tests/test_gpu_gym_agents.py::run_lockstep drives them (its helpers and bars are used here:
TOL 1e-5, PARAM_ATOL 5e-8, the 'rel' gradient measure): 10 gradient steps through
``_train_step`` -- eager steps, then replays of the captured graphs.  Per step the traced
``online_next_out`` is compared with the float64 forward of the pre-step ONLINE parameters on
next_state, and loss, priorities and every parameter gradient with the double-DQN reference
(tests/double_dqn_cases.py) built from the float64 outputs.  These configs use learning rates
of 0.005 to 0.1 (c51_cartpole_201: 1e-5): a select forward on stale or already-updated
parameters is far outside 1e-5 from the second step on -- the bug this file exists for.

Near ties: a sample whose two best float64 select Q lie within 1e-5 max(1, max|Q|) may match
either action's reference (the one its traced loss is closer to).  The count is printed; more
than one sample in eight of any step fails.  Seeds are fixed, so the count is deterministic:
on the MI355X 1 sample (step 9 of c51_cartpole_201, where max|Q| and so the window are ten
times the other configs') and 0 everywhere else, the Nature-CNN agents included.

The Nature-CNN agents (stored outputs, then the plain loss entry: _fused() is False) are
checked on their traced outputs, and the three schedules -- eager, per-step graphs, chunk
graphs -- must leave bitwise equal parameters, optimizer state and sum tree.
"""
import os
import random

import numpy as np
import pytest
import torch

from oracle import learner as OL
from oracle import learner_cases as C
from oracle import nature_cnn as ONC
from tests import double_dqn_cases as D
from tests import fourier_cases as FC
from tests import test_gpu_agent as TA
from tests import test_gpu_fourier_agents as F
from tests import test_gpu_gym_agents as G

pytestmark = pytest.mark.gpu

_AGENTS = os.path.join(G.ROOT, 'dopamine_amd', 'agents')
_GIN = {
    'double_dqn_acrobot': ('dqn/configs/double_dqn_acrobot.gin', []),
    'double_rainbow_cartpole': ('rainbow/configs/double_rainbow_cartpole.gin', []),
    'c51_cartpole_201+double': ('rainbow/configs/c51_cartpole_201.gin',
                                ['RainbowAgent.double_dqn = True']),
    'dqn_cartpole_fourier+double': ('dqn/configs/dqn_cartpole_fourier.gin',
                                    ['DQNAgent.double_dqn = True']),
    'double_rainbow_cartpole-pytorch': ('rainbow/configs/double_rainbow_cartpole.gin',
                                        ['RainbowAgent.use_hip_mlp = False']),
}
TOL, PARAM_ATOL = G.TOL, G.PARAM_ATOL
NEAR_TIE = 1e-5


def _near_tie_astar(qs, loss_of, traced_loss):
  """(a*, number of near ties): the first argmax of the float64 select Q, but on a sample
  whose two best Q are within NEAR_TIE of each other whichever of the two the traced loss is
  closer to.  loss_of(astar) -> the reference's per-sample loss."""
  B, A = qs.shape
  astar = qs.argmax(1)
  if A == 1:
    return astar, 0
  order = np.argsort(-qs, axis=1, kind='stable')
  gap = qs[np.arange(B), order[:, 0]] - qs[np.arange(B), order[:, 1]]
  near = gap <= NEAR_TIE * max(1.0, float(np.abs(qs).max()))
  if near.any():
    other = np.where(near, order[:, 1], astar)
    l0, l1 = loss_of(astar), loss_of(other)
    astar = np.where(near & (np.abs(traced_loss - l1) < np.abs(traced_loss - l0)), other, astar)
  return astar, int(near.sum())


def run_lockstep(name, steps=10):
  gin, bindings = _GIN[name]
  env, agent = G._make(os.path.join(_AGENTS, gin), bindings)
  assert agent.double_dqn is True and agent._double()
  rainbow = hasattr(agent, '_num_atoms')
  per_loss = rainbow and agent._replay_scheme == 'prioritized'
  agent.enable_trace()
  G._fill(env, agent)
  orc = G._oracle(agent, rainbow)
  net, B, A = agent.online_convnet, agent._batch_size, agent.num_actions
  cg = np.float64(np.float32(agent.cumulative_gamma))
  U = agent._UNROLL
  errs = dict(online=0.0, target=0.0, online_next=0.0, loss=0.0, priorities=0.0, grad={},
              params=0.0, near_ties=0)
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
    out, ctx = F._forward64(net, w, s)
    tout, _ = F._forward64(agent.target_convnet, tw, ns)
    sout, _ = F._forward64(net, w, ns)                       # ONLINE parameters on next_state
    errs['online_next'] = max(errs['online_next'],
                              G._rel(tr['online_next_out'].reshape(sout.shape), sout))
    if 'online_out' in tr and 'target_out' in tr:   # (the Rainbow agents' PyTorch path traces none)
      errs['online'] = max(errs['online'], G._rel(tr['online_out'].reshape(out.shape), out))
      errs['target'] = max(errs['target'], G._rel(tr['target_out'].reshape(tout.shape), tout))
    else:
      assert agent._mlp is None and rainbow
    if rainbow:
      N = agent._num_atoms
      c = dict(B=B, A=A, N=N, ol=out.reshape(B, A, N), tl=tout.reshape(B, A, N),
               sl=sout.reshape(B, A, N), act=act, rew=rew, term=term, cg=cg,
               z=agent._support.cpu().double().numpy(), probs=b[8] if per_loss else None)
      reference = lambda astar: D.c51_double_reference(c, per_loss, astar=astar)
      qs = D.select_q(c)
    else:
      c = dict(B=B, A=A, oq=out, tq=tout, sq=sout, act=act, rew=rew, term=term, cg=cg)
      reference = lambda astar: D.dqn_double_reference(c, astar=astar)
      qs = sout
    astar, near = _near_tie_astar(qs, lambda a: reference(a)['loss'], tr['loss'])
    errs['near_ties'] += near
    print('%s step %d: %d near ties of %d samples' % (name, step, near, B), flush=True)
    assert near * 8 <= B, 'step %d: %d of %d samples are near ties' % (step, near, B)
    ref = reference(astar)
    errs['loss'] = max(errs['loss'], G._rel(tr['loss'], ref['loss']))
    if rainbow:
      errs['priorities'] = max(errs['priorities'], float(
          (np.abs(tr['priorities'] - ref['priorities']) / np.abs(ref['priorities'])).max()))
    gout = ref['grad'].reshape(B, -1)
    for pname, g64 in F._backward64(net, ctx, gout).items():
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
    if per_loss:      # the next step samples the tree the device wrote
      orc.set_priority(np.asarray(idx, np.int32), tr['priorities'].astype(np.float32))
  agent._discard_prefetch()
  agent._replay.memory.sync_rng()
  if rainbow:
    assert random.getstate() == orc.py_rng.getstate()
  else:
    a, b = np.random.get_state(), orc.np_rng.get_state()
    assert np.array_equal(a[1], b[1]) and a[2] == b[2]
  return agent, errs


@pytest.mark.parametrize('name', sorted(_GIN))
def test_double_dqn_steps_match_float64_at_the_pre_step_parameters(name):
  from dopamine_amd import ops
  agent, errs = run_lockstep(name)
  print('double dqn agent errors', name, errs, flush=True)
  if name.endswith('-pytorch'):
    assert agent._mlp is None and agent._online_next is None
  else:
    assert agent._mlp is not None and agent._online_next is not None
    assert type(agent._online_next) is type(agent._mlp['target'][0])
  if name == 'double_dqn_acrobot':
    assert isinstance(agent._opt, ops.TF1GradientDescent) and agent.online_convnet.sizes == (24, 24)
  if name.startswith('double_rainbow_cartpole'):
    assert agent._replay_scheme == 'prioritized' and agent.update_horizon == 3
  if name.startswith('c51_cartpole_201'):
    assert agent._num_atoms == 201
  assert not agent._fused()
  assert errs['online_next'] <= TOL, errs
  assert errs['online'] <= TOL and errs['target'] <= TOL and errs['loss'] <= TOL, errs
  assert errs['priorities'] <= TOL, errs
  assert max(errs['grad'].values()) <= TOL, errs
  assert errs['params'] <= PARAM_ATOL, errs
  assert agent._graphs is not None            # the later steps replayed the captured graph


# ============================================================================ Nature CNN
def _nature(kind, **kw):
  from dopamine_amd.agents.dqn.dqn_agent import DQNAgent
  random.seed(5); np.random.seed(5); torch.manual_seed(5)
  if kind == 'rainbow':
    return TA._rainbow(double_dqn=True, **kw)
  a = DQNAgent(num_actions=6, replay_capacity=3000, batch_size=32, min_replay_history=100,
               double_dqn=True, **kw)
  TA._fill(a._replay.memory, 6, 3)
  return a


@pytest.mark.parametrize('kind', ['dqn', 'rainbow'])
def test_nature_cnn_double_dqn_steps(kind):
  """7 steps -- the first, non-pipelined one (nothing is prefetched yet), 3 eager pipelined
  ones, then 3 replays of the captured graphs: online_next_out against oracle/nature_cnn.py's
  float64 forward at the pre-step parameters; loss, priorities and the output gradient against
  the double reference evaluated on the traced outputs."""
  from dopamine_amd.cnn import HipNatureCNN
  a = _nature(kind)
  assert a._hip is not None and isinstance(a._online_next, HipNatureCNN)
  assert a.fused_head and a._rides() and not a._fused()
  a.enable_trace()
  B, A, U = a._batch_size, a.num_actions, a._UNROLL
  offsets = a.online_convnet.fp.offsets
  cg = np.float64(np.float32(a.cumulative_gamma))
  worst = 0.0
  for step in range(7):
    k = a._opt_steps % 2
    w = a.online_convnet.fp.flat.detach().cpu().double().numpy().copy()
    for _ in range(a.update_period):
      a._train_step()
    torch.cuda.synchronize()
    # captured after the third eager pipelined step: steps 4, 5, 6 replay
    assert (a._graphs is not None) == (step >= 3)
    assert a._eager_steps == {False: 1, True: min(step, 3)}
    tr = {n: t[U + k].detach().cpu().numpy() for n, t in a._trace.items()}
    with torch.no_grad():
      sout = ONC.forward(ONC.Params64(w, offsets),
                         ONC.to_input(np.moveaxis(tr['next_state'], 1, -1))).numpy()
    worst = max(worst, G._rel(tr['online_next_out'], sout))
    what = 'nature %s step %d' % (kind, step)
    if kind == 'rainbow':
      N = a._num_atoms
      c = dict(B=B, A=A, N=N, ol=tr['online_out'].reshape(B, A, N),
               tl=tr['target_out'].reshape(B, A, N), sl=tr['online_next_out'].reshape(B, A, N),
               act=tr['action'], rew=tr['reward'], term=tr['terminal'], cg=cg,
               z=a._support.cpu().numpy(), probs=tr['sampling_probabilities'])
      qs = D.select_q(c)
      astar, near = _near_tie_astar(
          qs, lambda s: D.c51_double_reference(c, True, astar=s)['loss'], tr['loss'])
      checks = C.c51_checks(D.c51_double_reference(c, True, astar=astar))
      checks.pop('mean_loss')
      got = dict(grad=tr['grad_out'], loss=tr['loss'], priorities=tr['priorities'])
    else:
      c = dict(B=B, A=A, oq=tr['online_out'], tq=tr['target_out'], sq=tr['online_next_out'],
               act=tr['action'], rew=tr['reward'], term=tr['terminal'], cg=cg)
      astar, near = _near_tie_astar(
          c['sq'].astype(np.float64), lambda s: D.dqn_double_reference(c, astar=s)['loss'],
          tr['loss'])
      checks = C.dqn_checks(D.dqn_double_reference(c, astar=astar))
      checks.pop('mean_loss')
      got = dict(grad=tr['grad_out'], loss=tr['loss'])
    print('%s: %d near ties' % (what, near), flush=True)
    assert near * 8 <= B
    for key, (ref, terms) in checks.items():
      ref = np.asarray(ref, np.float64)
      ONC.assert_layer_close('%s %s' % (what, key), got[key].reshape(ref.shape), ref,
                             np.asarray(terms, np.float64))
  print('nature %s online_next_out worst rel %.3g' % (kind, worst), flush=True)
  assert worst <= TOL


def test_nature_cnn_double_rainbow_schedules_are_bitwise_equal():
  """2 * _UNROLL + 1 gradient steps one per call (eager, then per-step graphs) and the same
  number through train_gradient_steps (chunk graphs): bitwise equal parameters, optimizer
  state and sum tree."""
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
    assert a._opt_steps == n and not a._fused()
    a._discard_prefetch()
    a._replay.memory.sync_rng()
    torch.cuda.synchronize()
    res.append(dict(online=a.online_convnet.fp.flat.cpu().numpy(),
                    target=a.target_convnet.fp.flat.cpu().numpy(),
                    tree=a._replay.memory.sum_tree.nodes[-1].copy(),
                    **{'opt_' + key: t.cpu().numpy() for key, t in a._opt_tensors()}))
  assert set(res[0]) == set(res[1])
  for key in res[0]:
    assert res[0][key].shape == res[1][key].shape and res[0][key].size > 0, key
    assert res[0][key].tobytes() == res[1][key].tobytes(), key


# ============================================================================== the rest
def test_iqn_double_dqn_builds_no_base_executor():
  from dopamine_amd.agents.implicit_quantile.implicit_quantile_agent import ImplicitQuantileAgent
  for flag in (True, False):
    a = ImplicitQuantileAgent(num_actions=4, replay_capacity=3000, batch_size=16,
                              num_tau_samples=8, num_tau_prime_samples=8, num_quantile_samples=4,
                              min_replay_history=100, replay_scheme='uniform', double_dqn=flag)
    assert a.double_dqn is flag and not a._double() and a._online_next is None
    assert ('online_next' in a._iqn) == flag             # its own path, as before


def test_double_dqn_with_a_process_group_is_refused_before_anything_is_built(monkeypatch):
  from dopamine_amd.agents.dqn.dqn_agent import DQNAgent
  from dopamine_amd.agents.rainbow.rainbow_agent import RainbowAgent

  class Group(object):            # a stand-in: construction must not reach a collective
    def __getattr__(self, name):
      raise AssertionError('the process group was used (%s)' % name)

  made = []
  monkeypatch.setattr(DQNAgent, '_build_networks', lambda self: made.append('networks'))
  for cls in (DQNAgent, RainbowAgent):
    monkeypatch.setattr(cls, '_build_replay_buffer', lambda self, staging: made.append('replay'))
    with pytest.raises(ValueError, match='double_dqn'):
      cls(num_actions=4, replay_capacity=3000, batch_size=32, double_dqn=True,
          process_group=Group())
  assert not made
