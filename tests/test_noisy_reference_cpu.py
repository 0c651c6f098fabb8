"""The noisy layers' references (tests/noisy_cases.py) against each other, torch autograd of the
networks' ``head(x, noise)`` and the mistakes the bar must reject; the generator's statistics;
the networks' initialisation; the agents' ``noisy`` argument and the three gin files.  No GPU.

The bar is the project's per-layer one (oracle.nature_cnn: LAYER_TOL 1e-5 on |got - ref| over
max(Σ|terms|, COND_FLOOR 1e-3 max|ref|)), the assertion tests/test_gpu_noisy.py makes of the
kernels.  The generator's statistics are each within 4 standard errors of their expectation on
2^16 draws; rehearsed for these three seeds: the worst is 2.7 standard errors.
"""
import inspect
import math
import os

import numpy as np
import pytest
import torch

from oracle import nature_cnn as ONC
from tests import noisy_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [NC.make_case(g, 0x5EED00 + i) for i, g in enumerate(NC.GEOMETRIES)]
_id = lambda c: NC.geometry_id(c['geometry'])


def test_the_bars_are_the_projects():
  assert ONC.LAYER_TOL == 1e-5 and ONC.COND_FLOOR == 1e-3


def test_hash_is_the_uniform_generators():
  """uniform_of's constants; a draw's top 24 bits are dq_uniform_draw's uniform."""
  assert NC.hash_of(0, 0, 0) == NC.hash_of(0, 0, 0) != NC.hash_of(0, 0, 1) != NC.hash_of(0, 1, 0)
  z = 0xD1B54A32D192ED03            # seed 0, call 0, draw 0: the mixing's input
  z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & NC.MASK
  z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & NC.MASK
  assert NC.hash_of(0, 0, 0) == z ^ (z >> 31)
  assert NC.hash_of(NC.MASK, 3, 5) < 1 << 64


def test_layouts():
  assert NC.layers((6, (5, 7), 3)) == [(6, 5, 0, 6), (5, 7, 11, 16), (7, 3, 23, 30)]
  assert NC.noise_numel((6, (5, 7), 3)) == 33
  assert NC.noise_numel((4, (512, 512), 153)) == 4 + 2 * 1024 + 153


def _weights_ok(c, wrong=None, scale=1.0):
  g = c['geometry']
  sigma = [(w * np.float32(scale), b * np.float32(scale)) for w, b in c['sigma']]
  ref = NC.weights64(g, c['mu'], sigma, c['noise'])
  noise, got_sigma = c['noise'], sigma
  if wrong == 'f_without_sqrt':
    noise = NC.f64(c['normals'], wrong).astype(np.float32)
  if wrong == 'sigma_over_sqrt_q':
    got_sigma = [(w * np.float32(scale), b * np.float32(scale))
                 for w, b in NC.sigma_init(g, wrong=wrong)]
  got = NC.weights32(g, c['mu'], got_sigma, noise, wrong=wrong)
  for l, ((w, b), (rw, rb, tw, tb)) in enumerate(zip(got, ref)):
    ONC.assert_layer_close('w %s layer %d %s' % (_id(c), l, wrong), w, rw, tw)
    ONC.assert_layer_close('b %s layer %d %s' % (_id(c), l, wrong), b, rb, tb)


def _grads_ok(c, wrong=None):
  g = c['geometry']
  ref = NC.grads64(g, c['dw'], c['noise'])
  noise = c['noise']
  if wrong == 'f_without_sqrt':
    noise = NC.f64(c['normals'], wrong).astype(np.float32)
  got = NC.grads32(g, c['dw'], noise, wrong=wrong)
  for l, ((gm_w, gm_b, gs_w, gs_b), (rw, rb, tw, tb)) in enumerate(zip(got, ref)):
    what = '%s layer %d %s' % (_id(c), l, wrong)
    assert np.array_equal(gm_b, c['dw'][l][1])
    ONC.assert_layer_close('d mu_w ' + what, gm_w, c['dw'][l][0].astype(np.float64),
                           np.abs(c['dw'][l][0]).astype(np.float64))
    ONC.assert_layer_close('d sigma_w ' + what, gs_w, rw, tw)
    ONC.assert_layer_close('d sigma_b ' + what, gs_b, rb, tb)


@pytest.mark.parametrize('c', CASES, ids=_id)
def test_restatements_meet_the_bar(c):
  _weights_ok(c)
  _weights_ok(c, scale=100.0)
  _grads_ok(c)


def _rejected(check):
  n = 0
  for c in CASES:
    try:
      check(c)
    except AssertionError:
      n += 1
  return n


@pytest.mark.parametrize('wrong', NC.WEIGHTS_WRONG)
def test_the_bar_rejects_wrong_weights(wrong):
  n = _rejected(lambda c: _weights_ok(c, wrong))
  print('%s: rejected on %d of %d geometries' % (wrong, n, len(CASES)))
  assert n >= 1


@pytest.mark.parametrize('wrong', NC.GRADS_WRONG)
def test_the_bar_rejects_wrong_gradients(wrong):
  n = _rejected(lambda c: _grads_ok(c, wrong))
  print('%s: rejected on %d of %d geometries' % (wrong, n, len(CASES)))
  assert n >= 1


# ------------------------------------------------------------------ the networks
def _net(geometry, **kw):
  from dopamine_amd.agents import networks
  D, sizes, n_out = geometry
  rs = np.random.RandomState(D)
  lo = -rs.uniform(0.5, 6.0, size=D)
  cls = type('Net%d' % D, (networks.BasicDiscreteDomainNetwork,),
             dict(MIN=lo, MAX=lo + rs.uniform(1.0, 12.0, size=D)))
  return cls(n_out, 1, device='cpu', seed=3, network_size=sizes, **kw)


def _per_layer(net, flat, part=''):
  out = []
  for n in net.layer_names():
    pair = []
    for s in ('_w', '_b'):
      o, shape = net.fp.offsets[n + part + s]
      pair.append(flat[o:o + int(np.prod(shape))].reshape(shape))
    out.append(tuple(pair))
  return out


@pytest.mark.parametrize('geometry', [(6, (5, 7), 3), (4, (64, 64), 102), (4, (3,), 2)],
                         ids=NC.geometry_id)
def test_float64_backward_is_autograd_of_the_noisy_head(geometry):
  """head(x, noise) in float32 torch with autograd against the float64 chain: the effective
  parameters (weights64), the float64 MLP on them, its backward, dw -> d sigma (grads64).  The
  measure is the agents' tests': the largest error over the tensor's largest reference value,
  at their 1e-5."""
  net = _net(geometry, noisy=True)
  B = 9
  rs = np.random.RandomState(11)
  with torch.no_grad():
    for n, prm in net.fp.params.items():
      if n.endswith('sigma_b'):       # unequal sigmas, so a transposed or shifted one shows
        prm.mul_(torch.from_numpy(rs.uniform(0.5, 1.5, prm.shape).astype(np.float32)))
  x = rs.uniform(net.MIN, net.MAX, (B, len(net.MIN)))
  noise = NC.f64(NC.normal64(NC.ROLE_SEEDS['online'], 2, net.noise_numel)).astype(np.float32)
  gout = rs.standard_normal((B, net.n_out))
  flat = net.fp.flat.detach().numpy().copy()
  mu, sigma = _per_layer(net, flat), _per_layer(net, flat, '_sigma')
  eff = NC.weights64(geometry, mu, sigma, noise)
  out, ins = NC.mlp64(NC.rescale32(x, net.MIN, net.MAX), eff)
  dw = NC.mlp64_backward(eff, ins, gout)
  ds = NC.grads64(geometry, dw, noise)
  for prm in net.parameters():
    prm.grad = None
  y = net.head(torch.from_numpy(x), torch.from_numpy(noise))
  rel = lambda got, ref: float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))
  assert rel(y.detach().numpy(), out) <= 1e-5
  y.backward(torch.from_numpy(gout.astype(np.float32)))
  for l, n in enumerate(net.layer_names()):
    got = {k: net.fp[n + k].grad.numpy() for k in ('_w', '_b', '_sigma_w', '_sigma_b')}
    assert rel(got['_w'], dw[l][0]) <= 1e-5 and rel(got['_b'], dw[l][1]) <= 1e-5, (n, l)
    assert rel(got['_sigma_w'], ds[l][0]) <= 1e-5, n
    assert rel(got['_sigma_b'], ds[l][1]) <= 1e-5, n
    assert np.abs(ds[l][0]).max() > 0
  # without noise: the mu network, and no gradient reaches a sigma
  mu_only = [(w.astype(np.float64), b.astype(np.float64)) for w, b in mu]
  want, _ = NC.mlp64(NC.rescale32(x, net.MIN, net.MAX), mu_only)
  for prm in net.parameters():
    prm.grad = None
  y0 = net.head(torch.from_numpy(x))
  assert rel(y0.detach().numpy(), want) <= 1e-5
  assert rel(y0.detach().numpy(), out) > 1e-3
  y0.backward(torch.from_numpy(gout.astype(np.float32)))
  assert all(net.fp[n + '_sigma_w'].grad is None for n in net.layer_names())


def test_noisy_composes_with_dueling():
  from dopamine_amd.agents import networks
  net = networks.CartpoleRainbowNetwork(2, num_atoms=51, device='cpu', network_size=(8, 8),
                                        dueling=True, noisy=True)
  assert net.n_out == 153 and net.fp.offsets['out_sigma_w'][1] == (153, 8)
  assert net.noise_numel == 4 + 8 + 8 + 8 + 8 + 153
  noise = torch.from_numpy(NC.f64(NC.normal64(1, 0, net.noise_numel)).astype(np.float32))
  x = torch.zeros(3, 4, dtype=torch.float64)
  out = net(x, noise=noise)
  assert out.shape == (3, 2, 51)
  head = net.head(x, noise)
  assert torch.equal(out, networks.dueling_combine(head, 2, 51))
  assert not torch.equal(out, net(x))
  # both blocks of the last layer share p: one sigma value
  s = net.fp['out_sigma_w'].detach()
  assert float(s.min()) == float(s.max())


@pytest.mark.parametrize('geometry', NC.GEOMETRIES[:5], ids=NC.geometry_id)
def test_initialisation(geometry):
  net = _net(geometry, noisy=True)
  plain = _net(geometry)
  D, sizes, n_out = geometry
  dims = [D] + list(sizes) + [n_out]
  assert net.mu_numel == plain.fp.numel and plain.mu_numel == plain.fp.numel
  assert net.noise_numel == NC.noise_numel(geometry)
  names = list(net.fp.offsets)
  assert names[:len(plain.fp.offsets)] == list(plain.fp.offsets)       # mu first, as the plain
  assert all('_sigma_' in n for n in names[len(plain.fp.offsets):])    # network; then the sigmas
  for n, v in plain.fp.offsets.items():
    assert net.fp.offsets[n] == v
  for l, n in enumerate(net.layer_names()):
    p = dims[l]
    lim = 1.0 / math.sqrt(p)
    for k in ('_w', '_b'):
      t = net.fp[n + k].detach().numpy()
      assert float(np.abs(t).max()) <= lim * (1 + 1e-6), (n, k)
      if t.size >= 64:
        assert float(np.abs(t).max()) > 0.8 * lim and abs(float(t.mean())) < 0.5 * lim
      s = net.fp[n + '_sigma' + k].detach().numpy()
      assert s.shape == t.shape
      assert np.all(s == np.float32(0.5 / math.sqrt(p))), (n, k)
  other = _net(geometry, noisy=True, noisy_sigma0=0.25)
  assert np.all(other.fp['out_sigma_b'].detach().numpy() == np.float32(0.25 / math.sqrt(dims[-2])))
  assert torch.equal(other.fp['fc0_w'], net.fp['fc0_w'])
  with pytest.raises(ValueError, match='noisy_sigma0'):
    _net(geometry, noisy=True, noisy_sigma0=0.0)


def test_noisy_false_is_the_plain_network():
  """noisy=False: the offsets and every draw are those of a network made without the argument
  (tests/test_dueling_networks_cpu.py pins the plain networks' bytes)."""
  from dopamine_amd.agents import networks
  for cls, kw in ((networks.CartpoleRainbowNetwork, dict(num_atoms=51)),
                  (networks.AcrobotDQNNetwork, {}), (networks.CartpoleDQNNetwork, {}),
                  (networks.AcrobotRainbowNetwork, dict(num_atoms=5, dueling=True))):
    a = cls(3, device='cpu', seed=4, network_size=(16, 8), **kw)
    b = cls(3, device='cpu', seed=4, network_size=(16, 8), noisy=False, noisy_sigma0=0.3, **kw)
    assert a.fp.offsets == b.fp.offsets and not b.noisy
    assert a.fp.flat.numpy().tobytes() == b.fp.flat.numpy().tobytes()
    assert not any('sigma' in n for n in b.fp.offsets)
  for cls in (networks.NatureDQNNetwork, networks.RainbowNetwork, networks.FourierDQNNetwork,
              networks.ImplicitQuantileNetwork):
    assert 'noisy' not in inspect.signature(cls.__init__).parameters, cls


# ------------------------------------------------------------------ the generator
@pytest.mark.parametrize('role', sorted(NC.ROLE_SEEDS))
def test_generator_statistics(role):
  """Mean, variance, lag-1 product mean of calls 0 and 1, and the call 0 x call 1 product mean,
  2^16 draws each: all within 4 standard errors (1 / sqrt(N), sqrt(2 / N) for the variance)."""
  seed, N = NC.ROLE_SEEDS[role], 1 << 16
  a, b = NC.normal64(seed, 0, N), NC.normal64(seed, 1, N)
  se = 1.0 / math.sqrt(N)
  worst = 0.0
  for n in (a, b):
    assert np.isfinite(n).all() and float(np.abs(n).min()) > 0
    stats = (n.mean() / se, (n.var() - 1.0) / (math.sqrt(2.0) * se),
             (n[:-1] * n[1:]).mean() * math.sqrt(N - 1.0))
    worst = max(worst, max(abs(float(s)) for s in stats))
  worst = max(worst, abs(float((a * b).mean() / se)))
  print('%s seed %#x: worst %.2f standard errors, smallest |n| %.1e'
        % (role, seed, worst, min(np.abs(a).min(), np.abs(b).min())))
  assert worst <= 4.0
  f = NC.f64(a)
  assert np.allclose(f * np.abs(f), a, rtol=1e-15, atol=0)
  assert not np.array_equal(a, b)


def test_role_seeds_are_the_agents():
  from dopamine_amd.agents.dqn.dqn_agent import DQNAgent
  assert DQNAgent.NOISE_ROLES == ('online', 'target', 'act')
  for i, r in enumerate(DQNAgent.NOISE_ROLES):
    assert NC.ROLE_SEEDS[r] == DQNAgent.NOISE_SEED + i
  assert len(set(NC.ROLE_SEEDS.values())) == 3


# ------------------------------------------------------------------ agents and configs
def test_constructors_take_noisy():
  from dopamine_amd.agents.dqn.dqn_agent import DQNAgent
  from dopamine_amd.agents.quantile.quantile_agent import QuantileAgent
  from dopamine_amd.agents.rainbow.rainbow_agent import RainbowAgent
  params = inspect.signature(DQNAgent.__init__).parameters
  assert params['noisy'].default is False and params['noisy_sigma0'].default == 0.5
  for cls in (RainbowAgent, QuantileAgent):      # passed on through **kwargs
    ps = inspect.signature(cls.__init__).parameters
    assert 'noisy' not in ps and any(p.kind is p.VAR_KEYWORD for p in ps.values()), cls


def _bindings(path):
  """The file's logical content: its lines without comments and blanks."""
  with open(path) as f:
    lines = [line.split('#')[0].rstrip() for line in f]
  return [line for line in lines if line]


@pytest.mark.parametrize('path,cls,base', [
    ('dqn/configs/noisy_dqn_acrobot.gin', 'DQNAgent', 'dqn/configs/dqn_acrobot.gin'),
    ('rainbow/configs/full_rainbow_cartpole.gin', 'RainbowAgent',
     'rainbow/configs/dueling_rainbow_cartpole.gin'),
    ('quantile/configs/noisy_quantile_cartpole.gin', 'QuantileAgent',
     'quantile/configs/quantile_cartpole.gin')])
def test_gin_files_parse_and_add_the_flag_and_the_epsilons_to_their_parents(path, cls, base):
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
  assert got[path].pop('noisy') == 'True' and 'noisy' not in got[base]
  assert float(got[path].pop('epsilon_train')) == 0.0 and float(got[path].pop('epsilon_eval')) == 0.0
  got[base].pop('epsilon_train', None)
  got[base].pop('epsilon_eval', None)
  assert got[path] == got[base]
  child, parent = _bindings(os.path.join(agents, path)), _bindings(os.path.join(agents, base))
  keep = [line for line in parent if '.epsilon_train' not in line and '.epsilon_eval' not in line]
  extra = [line for line in child if line not in keep]
  assert sorted(extra) == sorted(['%s.noisy = True' % cls, '%s.epsilon_train = 0.' % cls,
                                  '%s.epsilon_eval = 0.' % cls])
  assert [line for line in child if line not in extra] == keep
