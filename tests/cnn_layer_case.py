"""One Nature-CNN driven layer by layer through the C ABI, as tests/test_gpu_cnn_layers.py and
tests/bf16_build_child.py (the same drive on the bf16 throughput build, in a process of its
own) use it: every buffer holds one sample more than the batch, NaN before each call (inputs
too: a read past the batch poisons the result), the workspace 64 NaN words more than
dq_cnn_workspace_floats asks for.  The library is whichever dopamine_amd._lib loaded."""
import ctypes
import math

import torch

from oracle import nature_cnn as ONC

NAN = float('nan')
# backward layer index (dq_cnn_backward_layer) -> layer, its input, the d buffer it reads
# (None: dout), the d buffer its input gradient goes to
BACKWARD = ((0, 'fc2', 'h', None, 'h'), (1, 'fc1', 'a3', 'h', 'a3'), (2, 'conv3', 'a2', 'a3', 'a2'),
            (3, 'conv2', 'a1', 'a2', 'a1'), (4, 'conv1', 'x', 'a1', None))
FORWARD = (('conv1', 'x', 'a1'), ('conv2', 'a1', 'a2'), ('conv3', 'a2', 'a3'), ('fc1', 'a3', 'h'),
           ('fc2', 'h', 'out'))
D_NAMES = ('h', 'a3', 'a2', 'a1')


class LayerCase(object):
  """One network with buffers for B + 1 samples, driven through the C ABI at batch B."""

  def __init__(self, B, n_out):
    from dopamine_amd import _lib
    from dopamine_amd.agents.networks import NatureDQNNetwork, RainbowNetwork
    from dopamine_amd.cnn import HipNatureCNN
    torch.manual_seed(100 * B + n_out)
    self.B, self.n_out = B, n_out
    self.net = (RainbowNetwork(18, device='cuda', seed=3) if n_out == 918 else
                NatureDQNNetwork(n_out, device='cuda', seed=3))
    assert self.net.fp.offsets['fc2_w'][1] == (n_out, 512)
    with torch.no_grad():     # non-zero biases so the bias paths are exercised
      for n, prm in self.net.fp.params.items():
        if n.endswith('_b'):
          prm.uniform_(-0.05, 0.1)
    self.hip = h = HipNatureCNN(self.net, B + 1)       # the structs over (B + 1)-sample buffers
    self.need = int(_lib.lib.dq_cnn_workspace_floats(B, n_out))
    self.ws = torch.empty(self.need + 64, device='cuda')
    self.x = torch.full((B + 1, 84, 84, 4), NAN, device='cuda')
    self.x[:B] = torch.rand(B, 84, 84, 4, device='cuda')
    self.dout = torch.full((B + 1, n_out), NAN, device='cuda')
    self.dout[:B] = torch.randn(B, n_out, device='cuda')
    self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    self.fwd = (ctypes.byref(h._p), B, self.x.data_ptr(), ctypes.byref(h._a))
    self.bwd = (ctypes.byref(h._p), ctypes.byref(h._g), B, self.x.data_ptr(), ctypes.byref(h._a),
                self.dout.data_ptr(), ctypes.byref(h._d))
    # the upstream gradient each layer is tested with
    self.dz = {name: torch.randn_like(h.dacts[name][:B]) for name in D_NAMES}
    self._refs = {}
    self.forward()

  def call(self, fn, *args):
    """One C ABI call on a NaN workspace; the guard words must survive it."""
    from dopamine_amd import _lib
    self.ws.fill_(NAN)
    _lib.check(getattr(_lib.lib, fn)(*args), fn)
    torch.cuda.synchronize()
    ONC.assert_guard_untouched('%s workspace' % fn, self.ws, self.need)

  def forward(self):
    for t in self.hip.acts.values():
      t.fill_(NAN)
    self.call('dq_cnn_forward', *self.fwd, self.ws.data_ptr(), self.stream)
    self.acts = dict(self.hip.acts, x=self.x)

  def layer(self, index, part):
    self.call('dq_cnn_backward_layer', *self.bwd, self.ws.data_ptr(), index, part, self.stream)

  def nan_d(self):
    self.net.fp.grad.fill_(NAN)
    for name in D_NAMES:
      self.hip.dacts[name].fill_(NAN)

  def grad_range(self, name):
    o, shape = self.net.fp.offsets[name]
    return o, o + math.prod(shape)

  def reference(self, layer, pad=None):
    """The float64 layer on the device's input to it and this case's upstream gradient
    (computed once per layer, shared by the forward and the backward test)."""
    if pad is None and layer in self._refs:
      return self._refs[layer]
    _, _, src, read, _ = [b for b in BACKWARD if b[1] == layer][0]
    prm = self.net.fp.params
    ref = ONC.layer_reference(layer, self.acts[src][:self.B], prm[layer + '_w'], prm[layer + '_b'],
                              self.upstream(read), pad=pad)
    if pad is None:
      self._refs[layer] = ref
    return ref

  def upstream(self, read):
    return self.dout[:self.B] if read is None else self.dz[read]

  def what(self, text):
    return 'B=%d n_out=%d %s' % (self.B, self.n_out, text)
