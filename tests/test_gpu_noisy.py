"""The noisy layers' kernels (dq_noisy_draw / k_noisy_draw, dq_noisy_weights and dq_noisy_grads
/ k_noisy_apply) at their edges, and HipMLP on noisy networks, against tests/noisy_cases.py.

dq_noisy_draw: n = 1, 63, 64, 65 (a wave and its neighbours), 255, 257 (a block and one thread
more: two blocks, so the last-block ticket decides who advances the counter), 65536 (256
blocks) into NaN buffers with 64 guard floats.  f |f| must lie within 1e-5 max(1, |n|) of the
float64 normal of the same (seed, call, index): numpy's own float32 Box-Muller sits at 1.4e-6
of that measure; the device's worst ratio is printed.

dq_noisy_weights / dq_noisy_grads on every geometry (D, sizes, n_out) of NC.GEOMETRIES --
(1, (1,), 1) one element per segment; (4, (3,), 2) and (6, (5, 7), 3) odd widths: rows that
start unaligned, ragged segment ends, slice padding; (4, (64, 64), 102) rainbow_cartpole's
shape at 64 wide; (16, (33, 65, 31, 1), 1024) four layers, D at its cap, p = 1; (6, (1024,),
1024) the widest layers (1024 blocks); (4, (512, 512), 153) the dueling C51 CartPole head --
with sigma at 0.5 / sqrt(p) and at 100 times that: bitwise the float32 restatement from the
device's own noise, and within the project's per-layer bar of float64.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import nature_cnn as ONC
from tests import noisy_cases as NC
from tests import test_gpu_gym_agents as G

pytestmark = pytest.mark.gpu

_NAN = float('nan')
_SEED = NC.ROLE_SEEDS['online']


def _sampler(seed=_SEED):
  from dopamine_amd.mlp import NoiseSampler
  return NoiseSampler(seed, torch.device('cuda', torch.cuda.current_device()))


# ================================================================================ the generator
@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 257, 65536])
def test_draws_match_float64_and_advance_the_counter(n):
  s = _sampler()
  buf = torch.full((n + 64,), _NAN, device='cuda')
  worst = 0.0
  for call in range(3):
    buf.fill_(_NAN)
    s.draw(buf[:n])
    torch.cuda.synchronize()
    assert s.counter.tolist() == [call + 1, 0]
    f = buf[:n].cpu().numpy().astype(np.float64)
    assert bool(torch.isnan(buf[n:]).all()), 'guard floats written'
    assert np.isfinite(f).all()
    want = NC.normal64(_SEED, call, n)
    ratio = np.abs(f * np.abs(f) - want) / (1e-5 * np.maximum(1.0, np.abs(want)))
    worst = max(worst, float(ratio.max()))
    assert np.array_equal(np.sign(f), np.sign(want))
  print('dq_noisy_draw n=%d: worst ratio to the 1e-5 bound %.3g' % (n, worst), flush=True)
  assert worst <= 1.0


def test_graph_replays_draw_what_eager_calls_draw():
  n = 257
  a, b = _sampler(), _sampler()
  out = torch.full((n,), _NAN, device='cuda')
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    a.draw(out)
  torch.cuda.synchronize()
  assert a.counter.tolist() == [0, 0] and bool(torch.isnan(out).all())    # captured, not run
  seen = []
  for call in range(3):
    g.replay()
    eager = b.draw(torch.empty(n, device='cuda'))
    torch.cuda.synchronize()
    assert torch.equal(out, eager), call
    seen.append(out.clone())
  assert a.counter.tolist() == b.counter.tolist() == [3, 0]
  assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


def test_seeds_and_refusals():
  from dopamine_amd import _lib
  outs = [_sampler(seed).draw(torch.empty(300, device='cuda')) for seed in NC.ROLE_SEEDS.values()]
  torch.cuda.synchronize()
  assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
  s = _sampler()
  out = torch.full((8,), _NAN, device='cuda')
  st = _lib.stream_of(out.device)
  seed = ctypes.c_uint64(_SEED)
  for args in ((None, seed, 8, _lib.ptr(out), st), (_lib.ptr(s.counter), seed, 8, None, st),
               (_lib.ptr(s.counter), seed, 0, _lib.ptr(out), st),
               (_lib.ptr(s.counter), seed, -1, _lib.ptr(out), st)):
    assert _lib.lib.dq_noisy_draw(*args) == -1
    assert b'dq_noisy_draw' in _lib.lib.dq_last_error()
  torch.cuda.synchronize()
  assert bool(torch.isnan(out).all()) and s.counter.tolist() == [0, 0]


# ======================================================================== weights and gradients
def _net(geometry, noisy=True, **kw):
  from dopamine_amd.agents import networks
  D, sizes, n_out = geometry
  rs = np.random.RandomState(D)
  lo = -rs.uniform(0.5, 6.0, size=D)
  cls = type('Net%d' % D, (networks.BasicDiscreteDomainNetwork,),
             dict(MIN=lo, MAX=lo + rs.uniform(1.0, 12.0, size=D)))
  return cls(n_out, 1, device='cuda', seed=3, network_size=sizes, noisy=noisy, **kw)


def _per_layer(net, flat, part=''):
  out = []
  for n in net.layer_names():
    pair = []
    for s in ('_w', '_b'):
      o, shape = net.fp.offsets[n + part + s]
      pair.append(flat[o:o + int(np.prod(shape))].reshape(shape))
    out.append(tuple(pair))
  return out


def _covered(net, part=''):
  """Mask over the flat buffer of the layers' own elements of ``part`` (no slice padding)."""
  m = np.zeros(net.fp.numel, bool)
  for n in net.layer_names():
    for s in ('_w', '_b'):
      o, shape = net.fp.offsets[n + part + s]
      m[o:o + int(np.prod(shape))] = True
  return m


class _Case(object):
  """A noisy network, its device noise (call 0 of the online generator) and the structs of
  dq_noisy_weights over a NaN eff buffer with 64 guard floats."""

  def __init__(self, geometry):
    from dopamine_amd.mlp import _params_struct
    self.geometry = geometry
    self.net = net = _net(geometry)
    self.noise = _sampler().draw(torch.full((net.noise_numel + 64,), _NAN, device='cuda')[
        :net.noise_numel])
    self.eff = torch.full((net.mu_numel + 64,), _NAN, device='cuda')
    self.mu = _params_struct(net, net.fp.flat)
    self.sigma = _params_struct(net, net.fp.flat, '_sigma')
    self.effs = _params_struct(net, self.eff)
    self.gmu = _params_struct(net, net.fp.grad)
    self.gsigma = _params_struct(net, net.fp.grad, '_sigma')
    self.base_sigma = [net.fp[n + '_sigma' + s].detach().clone()
                       for n in net.layer_names() for s in ('_w', '_b')]
    torch.cuda.synchronize()
    self.noise_np = self.noise.cpu().numpy()
    want = NC.normal64(_SEED, 0, net.noise_numel)          # (the draw tests' measure)
    f = self.noise_np.astype(np.float64)
    assert (np.abs(f * np.abs(f) - want) <= 1e-5 * np.maximum(1.0, np.abs(want))).all()

  def set_sigma(self, scale):
    i = 0
    with torch.no_grad():
      for n in self.net.layer_names():
        for s in ('_w', '_b'):
          self.net.fp[n + '_sigma' + s].copy_(self.base_sigma[i] * scale)
          i += 1

  def weights(self):
    from dopamine_amd import ops
    self.eff.fill_(_NAN)
    ops.noisy_weights(self.mu, self.sigma, self.noise, self.effs)
    torch.cuda.synchronize()
    return self.eff.cpu().numpy()


@pytest.fixture(scope='module', params=NC.GEOMETRIES, ids=NC.geometry_id)
def case(request):
  return _Case(request.param)


@pytest.mark.parametrize('scale', [1.0, 100.0, 0.0], ids=['sigma', 'sigma-x100', 'sigma-0'])
def test_weights_are_bitwise_the_restatement_and_within_the_bar(case, scale):
  net, g = case.net, case.geometry
  case.set_sigma(scale)
  flat = net.fp.flat.detach().cpu().numpy()
  got = case.weights()
  mask = _covered(net)[:net.mu_numel]
  assert np.isfinite(got[:net.mu_numel][mask]).all()
  assert np.isnan(got[:net.mu_numel][~mask]).all(), 'slice padding written'
  assert np.isnan(got[net.mu_numel:]).all(), 'guard floats written'
  assert np.array_equal(case.weights().view(np.uint32), got.view(np.uint32))     # a second launch
  mu, sigma = _per_layer(net, flat), _per_layer(net, flat, '_sigma')
  eff = _per_layer(net, got)
  if scale == 0.0:
    for (w, b), (mw, mb) in zip(eff, mu):
      assert np.array_equal(w.view(np.uint32), mw.view(np.uint32))
      assert np.array_equal(b.view(np.uint32), mb.view(np.uint32))
    return
  want32 = NC.weights32(g, mu, sigma, case.noise_np)
  want64 = NC.weights64(g, mu, sigma, case.noise_np)
  for l, ((w, b), (w32, b32), (w64, b64, tw, tb)) in enumerate(zip(eff, want32, want64)):
    what = '%s layer %d sigma x%g' % (NC.geometry_id(g), l, scale)
    assert np.array_equal(w.view(np.uint32), w32.view(np.uint32)), what
    assert np.array_equal(b.view(np.uint32), b32.view(np.uint32)), what
    ONC.assert_layer_close('w ' + what, w, w64, tw)
    ONC.assert_layer_close('b ' + what, b, b64, tb)
    assert not np.array_equal(w, mu[l][0])


def test_sigma_gradients_are_bitwise_the_restatement_and_within_the_bar(case):
  from dopamine_amd import ops
  net, g = case.net, case.geometry
  rs = np.random.RandomState(7)
  grad = np.full(net.fp.numel, np.nan, np.float32)
  mask_mu, mask_sigma = _covered(net), _covered(net, '_sigma')
  grad[mask_mu] = rs.standard_normal(int(mask_mu.sum())).astype(np.float32)
  net.fp.grad.copy_(torch.from_numpy(grad))
  res = []
  for _ in range(2):
    net.fp.grad[torch.from_numpy(mask_sigma).cuda()] = _NAN
    ops.noisy_grads(case.mu, case.gmu, case.gsigma, case.noise)
    torch.cuda.synchronize()
    res.append(net.fp.grad.cpu().numpy())
  got = res[0]
  assert np.array_equal(res[1].view(np.uint32), got.view(np.uint32))
  # d mu: as it was
  assert np.array_equal(got[mask_mu].view(np.uint32), grad[mask_mu].view(np.uint32))
  assert np.isfinite(got[mask_sigma]).all()
  assert np.isnan(got[~(mask_mu | mask_sigma)]).all(), 'slice padding written'
  dw = _per_layer(net, grad)
  want32 = NC.grads32(g, dw, case.noise_np)
  want64 = NC.grads64(g, dw, case.noise_np)
  for l, ((sw, sb), w32, (w64, b64, tw, tb)) in enumerate(
      zip(_per_layer(net, got, '_sigma'), want32, want64)):
    what = '%s layer %d' % (NC.geometry_id(g), l)
    assert np.array_equal(sw.view(np.uint32), w32[2].view(np.uint32)), what
    assert np.array_equal(sb.view(np.uint32), w32[3].view(np.uint32)), what
    ONC.assert_layer_close('d sigma_w ' + what, sw, w64, tw)
    ONC.assert_layer_close('d sigma_b ' + what, sb, b64, tb)


def test_wrong_restatement_fails_on_the_device_result(case):
  """The device's (correct) eff against the restatement with the roles swapped: not equal."""
  net, g = case.net, case.geometry
  if all(p == 1 and q == 1 for p, q, _, _ in NC.layers(g)):
    return                                    # one input, one output: there is nothing to swap
  case.set_sigma(1.0)
  flat = net.fp.flat.detach().cpu().numpy()
  got = _per_layer(net, case.weights())
  wrong = NC.weights32(g, _per_layer(net, flat), _per_layer(net, flat, '_sigma'), case.noise_np,
                       wrong='roles_swapped')
  assert any(not np.array_equal(w, ww) for (w, _), (ww, _) in zip(got, wrong))


def test_refusals_leave_the_buffers_untouched():
  from dopamine_amd import _lib
  from dopamine_amd.mlp import _params_struct
  c = _Case((6, (5, 7), 3))
  net = c.net
  st = _lib.stream_of(c.eff.device)
  c.eff.fill_(_NAN)
  net.fp.grad.fill_(_NAN)
  by = ctypes.byref
  noise = _lib.ptr(c.noise)
  null = _params_struct(net, c.eff)
  null.b[1] = None
  odd = _params_struct(net, c.eff)
  odd.w[0] = odd.w[0] + 4
  other = _params_struct(net, c.eff)
  other.width[1] = 8
  big = _params_struct(net, c.eff)
  big.n_out = 1025
  weights = [(by(c.mu), by(c.sigma), None, by(c.effs)), (None, by(c.sigma), noise, by(c.effs)),
             (by(c.mu), None, noise, by(c.effs)), (by(c.mu), by(c.sigma), noise, None),
             (by(c.mu), by(c.sigma), noise, by(c.mu)),          # eff aliases mu
             (by(c.mu), by(c.sigma), noise, by(c.sigma)),       # eff aliases sigma
             (by(c.mu), by(c.sigma), noise, by(null)), (by(c.mu), by(c.sigma), noise, by(odd)),
             (by(c.mu), by(c.sigma), noise, by(other)), (by(big), by(big), noise, by(big))]
  for args in weights:
    assert _lib.lib.dq_noisy_weights(*args, st) == -1, args
    assert b'dq_noisy' in _lib.lib.dq_last_error()
  flat = net.fp.flat.clone()
  grads = [(by(c.mu), by(c.gmu), by(c.gsigma), None), (None, by(c.gmu), by(c.gsigma), noise),
           (by(c.mu), None, by(c.gsigma), noise), (by(c.mu), by(c.gmu), None, noise),
           (by(c.mu), by(c.gmu), by(c.gmu), noise),             # g_sigma aliases g_mu
           (by(c.mu), by(c.gmu), by(null), noise), (by(other), by(c.gmu), by(c.gsigma), noise)]
  for args in grads:
    assert _lib.lib.dq_noisy_grads(*args, st) == -1, args
    assert b'dq_noisy' in _lib.lib.dq_last_error()
  torch.cuda.synchronize()
  assert bool(torch.isnan(c.eff).all()) and bool(torch.isnan(net.fp.grad).all())
  assert torch.equal(net.fp.flat, flat)


# ===================================================================================== HipMLP
_MLP = [((6, (5, 7), 3), {}), ((4, (64, 64), 102), {}),
        ((4, (40, 24), 6), dict(dueling=True))]       # dueling: A = 2, N = 2, (A + 1) * N rows


def _mlp_net(geometry, kw, noisy=True):
  from dopamine_amd.agents import networks
  if not kw:
    return _net(geometry, noisy=noisy)
  return networks.CartpoleRainbowNetwork(2, num_atoms=2, device='cuda', seed=3,
                                         network_size=geometry[1], noisy=noisy, **kw)


@pytest.mark.parametrize('B', [1, 32, 33])
@pytest.mark.parametrize('geometry,kw', _MLP, ids=[NC.geometry_id(g) for g, _ in _MLP])
def test_hip_mlp_on_a_noisy_network_matches_float64(geometry, kw, B):
  from dopamine_amd.mlp import HipMLP
  from tests import dueling_cases as DC
  net = _mlp_net(geometry, kw)
  assert net.n_out == geometry[2] and net.noisy
  with pytest.raises(ValueError, match='NoiseSampler'):
    HipMLP(net, B)
  sampler = _sampler()
  exe = HipMLP(net, B, sampler=sampler)
  rs = np.random.RandomState(B)
  x = rs.uniform(net.MIN, net.MAX, (B, net.D))
  xd = torch.from_numpy(x).cuda()
  net.fp.grad.fill_(_NAN)
  out = exe.forward(xd).clone()
  gout = torch.from_numpy(rs.standard_normal(tuple(out.shape)).astype(np.float32)).cuda()
  exe.backward(gout)
  torch.cuda.synchronize()
  assert sampler.counter.tolist() == [1, 0]
  noise = exe.acts['noise'].cpu().numpy()
  flat = net.fp.flat.detach().cpu().numpy()
  mu, sigma = _per_layer(net, flat), _per_layer(net, flat, '_sigma')
  eff64 = NC.weights64(geometry, mu, sigma, noise)
  # the device's eff is the restatement, bit for bit
  eff_dev = exe.eff.cpu().numpy()
  for (w, b), (w32, b32) in zip(_per_layer(net, eff_dev), NC.weights32(geometry, mu, sigma, noise)):
    assert np.array_equal(w.view(np.uint32), w32.view(np.uint32))
    assert np.array_equal(b.view(np.uint32), b32.view(np.uint32))
  # G's float64 MLP on the float64 eff laid out as the flat buffer
  flat64 = flat.astype(np.float64)
  for n, (w, b, _, _) in zip(net.layer_names(), eff64):
    for s, v in (('_w', w), ('_b', b)):
      o, shape = net.fp.offsets[n + s]
      flat64[o:o + v.size] = v.reshape(-1)
  head, ins, P = G._forward64(net, flat64, x)
  head = head.numpy()
  want, g_head = head, gout.cpu().numpy().astype(np.float64)
  if kw:
    want = DC.forward64(head, 2, 2)[0].reshape(B, -1)
    g_head = DC.backward64(g_head.reshape(B, 2, 2), 2, 2)[0]
  assert G._rel(out.cpu().numpy(), want) <= G.TOL
  grad = net.fp.grad.cpu().numpy()
  b64 = G._backward64(net, P, ins, g_head)
  dw = [(b64[n + '_w'][0], b64[n + '_b'][0]) for n in net.layer_names()]
  ds = NC.grads64(geometry, dw, noise)
  worst = 0.0
  for l, n in enumerate(net.layer_names()):
    for s, ref_mu, ref_sigma in (('_w', dw[l][0], ds[l][0]), ('_b', dw[l][1], ds[l][1])):
      for name, ref in ((n + s, ref_mu), (n + '_sigma' + s, ref_sigma)):
        o, shape = net.fp.offsets[name]
        e = G._rel(grad[o:o + int(np.prod(shape))], ref.reshape(-1))
        worst = max(worst, e)
        assert e <= G.TOL, (name, e)
  mask = _covered(net) | _covered(net, '_sigma')
  assert np.isfinite(grad[mask]).all() and np.isnan(grad[~mask]).all()
  print('HipMLP noisy %s B=%d: worst gradient rel %.3g' % (NC.geometry_id(geometry), B, worst),
        flush=True)
  # fresh noise per forward; noise=False is a plain network's executor on the same mu, bitwise
  out2 = exe.forward(xd).clone()
  assert not torch.equal(out, out2) and sampler.counter.tolist() == [2, 0]
  plain = _mlp_net(geometry, kw, noisy=False)
  assert plain.fp.numel == net.mu_numel
  plain.fp.flat.copy_(net.fp.flat[:net.mu_numel])
  want0 = HipMLP(plain, B).forward(xd)
  got0 = exe.forward(xd, noise=False)
  torch.cuda.synchronize()
  assert torch.equal(got0, want0) and sampler.counter.tolist() == [2, 0]
  assert not torch.equal(got0, out2)
  with pytest.raises(AssertionError, match='noise=True'):
    exe.backward(gout)
