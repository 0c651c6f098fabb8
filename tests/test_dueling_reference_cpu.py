"""The dueling head's references (tests/dueling_cases.py) against each other, torch autograd and
the mistakes the bar must reject; the agents' ``dueling`` argument and the three gin files.
No GPU.

The bar is the project's per-layer one (oracle.nature_cnn: LAYER_TOL 1e-5 on |got - ref| over
max(Σ|terms|, COND_FLOOR 1e-3 max|ref|)), the assertion tests/test_gpu_dueling.py makes of the
kernels.
"""
import inspect
import os

import numpy as np
import pytest
import torch

from oracle import nature_cnn as ONC
from tests import dueling_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = DC.all_cases()


def test_the_bars_are_the_projects():
  assert ONC.LAYER_TOL == 1e-5 and ONC.COND_FLOOR == 1e-3


def test_case_table_covers_the_shapes_and_kinds():
  assert len(CASES) == len(DC.SHAPES) * len(DC.KINDS)
  assert {c['kind'] for c in CASES} == set(DC.KINDS)
  assert {(c['A'] == 1, c['N'] == 1) for c in CASES} >= {(True, True), (False, True),
                                                          (False, False)}
  c = CASES[3]
  d = DC.make_case(c['B'], c['A'], c['N'], c['kind'], 7)
  e = DC.make_case(c['B'], c['A'], c['N'], c['kind'], 7)
  assert d['head'].tobytes() == e['head'].tobytes() and d['g'].tobytes() == e['g'].tobytes()
  for c in CASES:      # the sparse gradient: one action's row per sample, the rest exact zeros
    nz = (c['gs'] != 0).any(2)
    assert (nz.sum(1) <= 1).all()
    assert np.array_equal(c['gs'][np.arange(c['B']), c['act']], c['g'][np.arange(c['B']), c['act']])


def _forward_ok(c, wrong=None):
  ref, terms = DC.forward64(c['head'], c['A'], c['N'])
  got = DC.forward32(c['head'], c['A'], c['N'], wrong=wrong)
  ONC.assert_layer_close('forward %s %s' % (DC.case_id(c), wrong), got, ref, terms)


def _backward_ok(c, key, wrong=None):
  ref, terms = DC.backward64(c[key], c['A'], c['N'])
  got = DC.backward32(c[key], c['A'], c['N'], wrong=wrong, act=c['act'])
  ONC.assert_layer_close('backward %s %s %s' % (DC.case_id(c), key, wrong), got, ref, terms)


@pytest.mark.parametrize('c', CASES, ids=DC.case_id)
def test_restatement_meets_the_bar(c):
  _forward_ok(c)
  _backward_ok(c, 'g')
  _backward_ok(c, 'gs')


def _rejected(check):
  n = 0
  for c in CASES:
    try:
      check(c)
    except AssertionError:
      n += 1
  return n


@pytest.mark.parametrize('wrong', DC.FORWARD_WRONG)
def test_the_bar_rejects_a_wrong_forward(wrong):
  n = _rejected(lambda c: _forward_ok(c, wrong))
  print('%s: rejected on %d of %d cases' % (wrong, n, len(CASES)))
  assert n >= 1


@pytest.mark.parametrize('wrong', DC.BACKWARD_WRONG)
def test_the_bar_rejects_a_wrong_backward(wrong):
  # (dval from the taken action only is right on the sparse gradient: g is dense here)
  n = _rejected(lambda c: _backward_ok(c, 'g', wrong))
  print('%s: rejected on %d of %d cases' % (wrong, n, len(CASES)))
  assert n >= 1


@pytest.mark.parametrize('c', CASES, ids=DC.case_id)
def test_backward64_is_autograd_of_forward64(c):
  A, N = c['A'], c['N']
  head = torch.tensor(c['head'], dtype=torch.float64, requires_grad=True)
  adv = head[:, :A * N].reshape(-1, A, N)
  val = head[:, A * N:].reshape(-1, 1, N)
  out = (adv - adv.mean(1, keepdim=True)) + val
  ref, _ = DC.forward64(c['head'], A, N)
  np.testing.assert_allclose(out.detach().numpy(), ref, rtol=1e-14, atol=1e-12)
  for key in ('g', 'gs'):
    head.grad = None
    out.backward(torch.tensor(c[key], dtype=torch.float64), retain_graph=True)
    want, _ = DC.backward64(c[key], A, N)
    scale = max(1.0, float(np.abs(want).max()))
    assert float(np.abs(head.grad.numpy() - want).max()) <= 1e-13 * scale


@pytest.mark.parametrize('c', CASES, ids=DC.case_id)
def test_value_identities(c):
  A, N = c['A'], c['N']
  ref, _ = DC.forward64(c['head'], A, N)
  _, val = DC.split(c['head'].astype(np.float64), A, N)
  scale = max(1.0, float(np.abs(c['head']).max()))
  assert float(np.abs(ref.mean(1) - val).max()) <= 1e-12 * scale    # mean_a out = val
  if A == 1:                                                         # one action: out is val
    assert np.array_equal(ref[:, 0], val)
    got = DC.forward32(c['head'], A, N)
    assert got[:, 0].tobytes() == DC.split(c['head'], A, N)[1].tobytes()
  # the sparse gradient's value-stream gradient is the taken row, bit for bit
  d = DC.backward32(c['gs'], A, N)
  taken = c['gs'][np.arange(c['B']), c['act']]
  assert d[:, A * N:].tobytes() == taken.tobytes()


def test_constructors_take_dueling():
  from dopamine_amd.agents.dqn.dqn_agent import DQNAgent
  from dopamine_amd.agents.quantile.quantile_agent import QuantileAgent
  from dopamine_amd.agents.rainbow.rainbow_agent import RainbowAgent
  params = inspect.signature(DQNAgent.__init__).parameters
  assert params['dueling'].default is False and list(params)[-1] == 'dueling'
  for cls in (RainbowAgent, QuantileAgent):      # passed on through **kwargs
    ps = inspect.signature(cls.__init__).parameters
    assert 'dueling' not in ps and any(p.kind is p.VAR_KEYWORD for p in ps.values()), cls


def _bindings(path):
  """The file's logical content: its lines without comments and blanks."""
  with open(path) as f:
    lines = [line.split('#')[0].rstrip() for line in f]
  return [line for line in lines if line]


@pytest.mark.parametrize('path,cls,base', [
    ('dqn/configs/dueling_double_dqn_acrobot.gin', 'DQNAgent',
     'dqn/configs/double_dqn_acrobot.gin'),
    ('rainbow/configs/dueling_rainbow_cartpole.gin', 'RainbowAgent',
     'rainbow/configs/double_rainbow_cartpole.gin'),
    ('quantile/configs/dueling_quantile_cartpole.gin', 'QuantileAgent',
     'quantile/configs/quantile_cartpole.gin')])
def test_gin_files_parse_and_add_one_binding_to_their_parents(path, cls, base):
  from dopamine_amd import gin_lite
  from dopamine_amd.discrete_domains import gym_lib, run_experiment  # noqa: F401 (gin names)
  agents = os.path.join(ROOT, 'dopamine_amd', 'agents')
  got = {}
  for f in (path, base):
    gin_lite.clear_config()
    try:
      gin_lite.parse_config_files_and_bindings([os.path.join(agents, f)], [])
      plain = (bool, int, float, str, tuple, list)     # (an optimizer: its class will do)
      got[f] = {k: repr(v) if isinstance(v, plain) else getattr(v, '__name__', type(v).__name__)
                for k, v in gin_lite.query(cls).items()}
    finally:
      gin_lite.clear_config()
  assert got[path].pop('dueling') == 'True'
  assert 'dueling' not in got[base]
  assert got[path] == got[base]
  child, parent = _bindings(os.path.join(agents, path)), _bindings(os.path.join(agents, base))
  extra = [line for line in child if line not in parent]
  assert extra == ['%s.dueling = True' % cls]
  assert [line for line in child if line not in extra] == parent
