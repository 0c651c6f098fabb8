"""HIP executor of the Fourier-basis Q-networks over a network's flat parameter buffer.

Forward and backward of ``networks.FourierDQNNetwork`` (gym_lib.py:135-206: the scale to
[0, 1], (order + 1)^D - 1 cosine features, a bias-free linear head) run as one launch each
(dopamine_amd/csrc/fourier.hip) instead of a cast, a sub, a div, a GEMM, a mul, a cos and a
GEMM plus autograd.  The launch takes the state as the replay hands it over (float64 for the
gym configs) and casts it in the kernel; the backward writes the head's weight gradient
straight into the flat gradient buffer (plain stores), which the TF1 optimizer kernel then
consumes.  It has ``mlp.HipMLP``'s interface, so the agent drives either.
"""
import ctypes

import numpy as np
import torch

from dopamine_amd import _lib


def _params_struct(net, buf):
  s = _lib.FourierParams(in_dim=int(net.D), order=int(net.order), n_out=int(net.n_out))
  s.w = buf.data_ptr() + 4 * net.fp.offsets['out_w'][0]
  lo = np.asarray(net.MIN, dtype=np.float64)
  rng = (np.asarray(net.MAX, dtype=np.float64) - lo).astype(np.float32)   # subtracted in float64
  for d in range(int(net.D)):
    s.in_min[d] = float(np.float32(lo[d]))
    s.in_range[d] = float(rng[d])
  return s


class HipFourier(object):
  """Executes a ``FourierDQNNetwork``'s parameter (read in place) with the HIP kernels.
  ``forward`` keeps the features for ``backward`` when ``keep`` is set (the online network);
  the target and the batch-1 acting executors keep none.  Use one executor per concurrent
  stream (online vs target)."""

  def __init__(self, net, batch_size, keep=True):
    F = int(_lib.lib.dq_fourier_features(int(net.D), int(net.order)))
    if F == 0 or F != net.F or not 1 <= net.n_out <= _lib.FOURIER_MAX_OUT:
      raise ValueError('HipFourier: unsupported geometry D=%d order=%d n_out=%d (D <= 16, at most '
                       '%d features, n_out <= 64)' % (net.D, net.order, net.n_out,
                                                      _lib.FOURIER_MAX_FEATURES))
    self.net = net
    self.B = B = int(batch_size)
    self.D, self.n_out, self.F = int(net.D), int(net.n_out), F
    dev = net.fp.flat.device
    mk = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    self.acts = dict(out=mk(B, self.n_out))
    if keep:
      self.acts.update(s=mk(B, self.D), phi=mk(B, F))
    self._p = _params_struct(net, net.fp.flat)
    self._g = _params_struct(net, net.fp.grad)
    self._a = _lib.FourierActs(s=self.acts['s'].data_ptr() if keep else None,
                               phi=self.acts['phi'].data_ptr() if keep else None,
                               out=self.acts['out'].data_ptr())

  def forward(self, x):
    """x: the states, B * D contiguous float64 or float32 values (any shape).  Returns the
    (B, n_out) output buffer (overwritten by the next call)."""
    assert x.numel() == self.B * self.D and x.is_contiguous(), (tuple(x.shape), self.B, self.D)
    assert x.dtype in (torch.float64, torch.float32), x.dtype
    _lib.check(_lib.lib.dq_fourier_forward(ctypes.byref(self._p), self.B, x.data_ptr(),
                                           int(x.dtype == torch.float64), ctypes.byref(self._a),
                                           _lib.stream_of(x.device)), 'dq_fourier_forward')
    return self.acts['out']

  def backward(self, dout):
    """dout: (B, n_out) = d loss / d output of the last ``forward``.  Writes the head's weight
    gradient into net.fp.grad."""
    assert dout.numel() == self.B * self.n_out and dout.is_contiguous()
    assert dout.dtype == torch.float32
    _lib.check(_lib.lib.dq_fourier_backward(ctypes.byref(self._p), ctypes.byref(self._g), self.B,
                                            ctypes.byref(self._a), dout.data_ptr(),
                                            _lib.stream_of(dout.device)), 'dq_fourier_backward')
    return self.net.fp.grad
