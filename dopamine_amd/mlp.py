"""HIP executor of the classic-control MLPs over a network's flat parameter buffer.

Forward and backward of ``networks.BasicDiscreteDomainNetwork`` (gym_lib.py:75-110: the
rescale to [-1, 1], L ReLU layers, a linear output layer) run as L + 1 and L + 1 launches
on the exact-fp32 matrix cores (dopamine_amd/csrc/mlp.hip) instead of ~15 library launches
and autograd.  The first launch takes the state as the replay hands it over (float64 for
the gym configs) and casts it in the kernel; the backward writes every weight / bias
gradient straight into the flat gradient buffer (plain stores), which the TF1 optimizer
kernel then consumes.
"""
import ctypes

import numpy as np
import torch

from dopamine_amd import _lib
from dopamine_amd import ops


def _params_struct(net, buf, part=''):
  """part '': the layers' weights and biases (a noisy network's mu); '_sigma': its sigmas."""
  fp = net.fp
  L = len(net.sizes)
  s = _lib.MlpParams(in_dim=int(net.D), n_layers=L, n_out=int(net.n_out))
  base = buf.data_ptr()
  names = ['fc%d' % i for i in range(L)] + ['out']
  for i, n in enumerate(names):
    s.w[i] = base + 4 * fp.offsets[n + part + '_w'][0]
    s.b[i] = base + 4 * fp.offsets[n + part + '_b'][0]
  for i, w in enumerate(net.sizes):
    s.width[i] = int(w)
  lo = np.asarray(net.MIN, dtype=np.float64)
  rng = (np.asarray(net.MAX, dtype=np.float64) - lo).astype(np.float32)   # subtracted in float64
  for d in range(int(net.D)):
    s.in_min[d] = float(np.float32(lo[d]))
    s.in_range[d] = float(rng[d])
  return s


class NoiseSampler(object):
  """The noisy layers' generator, the analogue of iqn.TauSampler: call k of a sampler fills a
  buffer with f(n) = sgn(n) sqrt(|n|) of standard normals that are a fixed function of (seed,
  k, index), and the call counter lives on the device (dq_noisy_draw advances it in the
  draw's own launch), so graph replays draw what the same eager calls draw.  ``counter`` is
  two int64: the call count and the launch's block ticket (zero between launches)."""

  def __init__(self, seed, device):
    self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    self.counter = torch.zeros(2, dtype=torch.int64, device=device)

  def draw(self, out):
    return ops.noisy_draw(self.counter, self.seed, out)


class HipMLP(object):
  """Executes a ``BasicDiscreteDomainNetwork``'s parameters (read in place) with the HIP
  kernels.  ``forward`` keeps its activations for ``backward``; use one executor per
  concurrent stream (online vs target).  A dueling network's head is applied here: the last
  layer's (B, n_out = (A + 1) * N) output goes to ``acts['head']``, dq_dueling_forward combines
  it into ``acts['out']`` (B, A * N), which ``forward`` returns and ``backward`` takes the
  gradient of (dq_dueling_backward into ``dhead``, then the MLP's backward on that).
  A noisy network (``net.noisy``) needs a ``sampler`` (NoiseSampler): ``forward`` draws
  ``noise``, materialises the effective parameters into ``eff`` (dq_noisy_weights; the mu
  region's length, laid out as it) and runs the MLP on them; ``backward`` runs on ``eff`` too
  (so the input gradients use the noisy weights), writes dw / db into the flat gradient's mu
  slots and forms the sigma gradients from them (dq_noisy_grads).  ``forward(x, noise=False)``
  is the plain path on mu."""

  def __init__(self, net, batch_size, sampler=None):
    L = len(net.sizes)
    if not (1 <= L <= _lib.MLP_MAX_LAYERS and 1 <= net.D <= _lib.MLP_MAX_IN and
            all(1 <= w <= _lib.MLP_MAX_WIDTH for w in net.sizes) and
            1 <= net.n_out <= _lib.MLP_MAX_WIDTH):
      raise ValueError('HipMLP: unsupported geometry D=%d sizes=%r n_out=%d (D <= 16, 1..4 layers '
                       'of width <= 1024, n_out <= 1024)' % (net.D, net.sizes, net.n_out))
    self.net = net
    self.B = B = int(batch_size)
    self.D, self.n_out = int(net.D), int(net.n_out)
    dev = net.fp.flat.device
    mk = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    self.dueling = bool(getattr(net, 'dueling', False))
    self.acts = dict(x0=mk(B, self.D), out=mk(B, self.n_out))
    if self.dueling:
      self.A, self.N = int(net.A), int(net.N or 1)
      self.acts['head'] = self.acts['out']          # the last layer's raw output
      self.acts['out'] = mk(B, self.A * self.N)     # the combined head
      self.dhead = mk(B, self.n_out)
    self.dacts = {}
    for i, w in enumerate(net.sizes):
      self.acts['h%d' % i] = mk(B, w)
      self.dacts['h%d' % i] = mk(B, w)
    self._p = _params_struct(net, net.fp.flat)
    self._g = _params_struct(net, net.fp.grad)
    self.ws = mk(int(_lib.lib.dq_mlp_workspace_floats(B, ctypes.byref(self._p))) + 64)
    self._a = self._acts_struct(self.acts)
    self._d = self._acts_struct(self.dacts)
    self.noisy = bool(getattr(net, 'noisy', False))
    self.sampler = sampler
    self._noised = False          # the last forward ran on eff
    if self.noisy:
      if sampler is None:
        raise ValueError('HipMLP: a noisy network needs a NoiseSampler')
      self.acts['noise'] = self.noise = mk(net.noise_numel)
      self.eff = torch.zeros(net.mu_numel, dtype=torch.float32, device=dev)
      self._mu = self._p
      self._sigma = _params_struct(net, net.fp.flat, '_sigma')
      self._eff = _params_struct(net, self.eff)
      self._gsigma = _params_struct(net, net.fp.grad, '_sigma')

  @staticmethod
  def _acts_struct(t):
    out = t.get('head', t.get('out'))     # the last layer writes the raw head
    s = _lib.MlpActs(x0=t['x0'].data_ptr() if 'x0' in t else None,
                     out=None if out is None else out.data_ptr())
    for i in range(4):
      if 'h%d' % i in t:
        s.h[i] = t['h%d' % i].data_ptr()
    return s

  def forward(self, x, noise=True):
    """x: the states, B * D contiguous float64 or float32 values (any shape, e.g. the
    gather's (B, 1, D, 1)).  Returns the (B, n_out) output buffer, with a dueling network the
    combined (B, A * N) one (overwritten by the next call).  noise (a noisy network only): True
    -- a fresh draw of the sampler, then the effective parameters; False -- the mu network."""
    assert x.numel() == self.B * self.D and x.is_contiguous(), (tuple(x.shape), self.B, self.D)
    assert x.dtype in (torch.float64, torch.float32), x.dtype
    self._noised = self.noisy and bool(noise)
    if self._noised:
      self.sampler.draw(self.noise)
      ops.noisy_weights(self._mu, self._sigma, self.noise, self._eff)
    self._p = self._eff if self._noised else self._mu if self.noisy else self._p
    _lib.check(_lib.lib.dq_mlp_forward(ctypes.byref(self._p), self.B, x.data_ptr(),
                                       int(x.dtype == torch.float64), ctypes.byref(self._a),
                                       self.ws.data_ptr(), _lib.stream_of(x.device)),
               'dq_mlp_forward')
    if self.dueling:
      ops.dueling_forward(self.acts['head'], self.A, self.N, out=self.acts['out'])
    return self.acts['out']

  def backward(self, dout):
    """dout: d loss / d output of the last ``forward``, shaped as that output.  Writes all
    parameter gradients into net.fp.grad."""
    assert dout.numel() == self.acts['out'].numel() and dout.is_contiguous()
    assert dout.dtype == torch.float32
    assert self._noised or not self.noisy, 'a noisy network trains on forward(x, noise=True)'
    if self.dueling:
      dout = ops.dueling_backward(dout.view(self.B, -1), self.A, self.N, out=self.dhead)
    _lib.check(_lib.lib.dq_mlp_backward(ctypes.byref(self._p), ctypes.byref(self._g), self.B,
                                        ctypes.byref(self._a), dout.data_ptr(),
                                        ctypes.byref(self._d), self.ws.data_ptr(),
                                        _lib.stream_of(dout.device)), 'dq_mlp_backward')
    if self._noised:
      ops.noisy_grads(self._mu, self._g, self._gsigma, self.noise)
    return self.net.fp.grad
