"""conv2's input gradient (the four sub-pixel classes of the stride-2 transposed conv) at the
batches where its tiles can go wrong, through the per-layer launch (dq_cnn_backward_layer,
one 8-wave tile per block) and through backward launch 3 of the grouped schedule (two tiles
per 16-wave block):
  B = 1   121 / 110 / 110 / 100 class rows: 4 tiles each, every class's tile count even;
  B = 3   the 11x10 and 10x11 classes have 330 rows = 11 tiles, an odd count: the last
          block's second half recomputes the last tile;
  B = 7   ragged everywhere (847 / 770 / 770 / 700 rows).
Both must be the same bits, match a float64 CPU transposed convolution with the ReLU mask
within the gradient tolerance of tests/test_gpu_cnn.py (5e-5 of the tensor's scale), and
write only their own rows."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

_BATCHES = (1, 3, 7)
_CLASSES = ((0, 0), (0, 1), (1, 0), (1, 1))


class _Case(object):
  """One network with activation buffers for B + 1 samples, driven at batch B: the last
  sample's rows belong to nobody."""

  def __init__(self, B):
    from dopamine_amd.agents.networks import RainbowNetwork
    from dopamine_amd.cnn import HipNatureCNN
    torch.manual_seed(11 + B)
    self.B = B
    self.net = RainbowNetwork(4, device='cuda', seed=5)
    self.hip = HipNatureCNN(self.net, B + 1)
    self.hip.forward(torch.rand(B + 1, 84, 84, 4, device='cuda').permute(0, 3, 1, 2))
    self.da2 = torch.randn_like(self.hip.dacts['a2'])
    self.hip.dacts['a3'].copy_(torch.randn_like(self.hip.dacts['a3']))
    self.dout = torch.zeros_like(self.hip.acts['out'])
    self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

  def run(self, grouped):
    """d a1 (B + 1, 21, 21, 32) after conv2's input gradient at batch B, from a NaN fill."""
    from dopamine_amd import _lib
    h = self.hip
    h.dacts['a2'].copy_(self.da2)
    h.dacts['a1'].fill_(float('nan'))
    args = (ctypes.byref(h._p), ctypes.byref(h._g), self.B, h._x.data_ptr(), ctypes.byref(h._a),
            self.dout.data_ptr(), ctypes.byref(h._d), h.ws.data_ptr())
    if grouped:    # launch 3 alone: conv3's weight-gradient slabs + the paired sub-pixel tiles
      _lib.check(_lib.lib.dq_cnn_backward_groups(*args, 3, 4, self.stream), 'dq_cnn_backward_groups')
    else:
      _lib.check(_lib.lib.dq_cnn_backward_layer(*args, 3, 0, self.stream), 'dq_cnn_backward_layer')
    torch.cuda.synchronize()
    return h.dacts['a1'].clone()

  def reference(self):
    """float64 on the CPU: the gradient of conv2 (TF SAME: pad 1 before, 2 after; stride 2)
    w.r.t. its input for upstream d a2, times (a1 > 0).  NHWC, the first B samples."""
    a1 = self.hip.acts['a1'][:self.B].double().cpu()
    x = a1.permute(0, 3, 1, 2).clone().requires_grad_(True)
    w = self.net.fp.params['conv2_w'].detach().double().cpu()
    y = F.conv2d(F.pad(x, (1, 2, 1, 2)), w, None, stride=2)
    y.backward(self.da2[:self.B].double().cpu().permute(0, 3, 1, 2))
    return x.grad.permute(0, 2, 3, 1) * (a1 > 0)


@pytest.fixture(scope='module', params=_BATCHES)
def case(request):
  c = _Case(request.param)
  c.layer, c.grouped, c.ref = c.run(False), c.run(True), c.reference()
  return c


def test_grouped_equals_per_layer_bitwise(case):
  B = case.B
  assert torch.isfinite(case.layer[:B]).all() and torch.isfinite(case.grouped[:B]).all()
  assert torch.equal(case.layer[:B], case.grouped[:B])


@pytest.mark.parametrize('which', ['layer', 'grouped'])
def test_matches_float64_transposed_conv(case, which):
  got = getattr(case, which)[:case.B].double().cpu()
  assert (case.ref != 0).any() and (case.ref == 0).any()      # the mask keeps and drops
  scale = case.ref.abs().max().item()
  err = (got - case.ref).abs().max().item()
  print('B=%d %s: max err %.3g, scale %.3g' % (case.B, which, err, scale))
  assert err <= 5e-5 * scale, 'max err %.3g vs scale %.3g' % (err, scale)
  for py, px in _CLASSES:     # each class's own rows against its own part of the reference
    e = (got[:, py::2, px::2] - case.ref[:, py::2, px::2]).abs().max().item()
    assert e <= 5e-5 * scale, 'class (%d, %d): max err %.3g vs scale %.3g' % (py, px, e, scale)


@pytest.mark.parametrize('which', ['layer', 'grouped'])
def test_rows_past_the_batch_are_untouched(case, which):
  """Sample B of the buffers is not part of the batch: no tile (the ragged last one, the
  recomputed one of an odd count) may store there -- the NaN fill is still in place."""
  assert torch.isnan(getattr(case, which)[case.B:]).all()


@pytest.mark.parametrize('which', ['layer', 'grouped'])
def test_each_class_writes_only_its_own_rows(case, which):
  """Class (py, px) reads only the taps kh = (py + 1) % 2 + 2 th, kw = (px + 1) % 2 + 2 tw.
  With those taps NaN and the mask open everywhere, whatever that class's tiles store is NaN:
  exactly its own pixels of the B samples turn NaN, every other row keeps the bits of the
  clean run."""
  h, B = case.hip, case.B
  a1_saved = h.acts['a1'].clone()
  w = case.net.fp.params['conv2_w']            # (out, in, kh, kw) view of the flat buffer
  w_saved = w.detach().clone()
  try:
    h.acts['a1'].fill_(1.0)
    clean = case.run(which == 'grouped')
    assert torch.isfinite(clean[:B]).all()
    for py, px in _CLASSES:
      with torch.no_grad():
        w.copy_(w_saved)
        w[:, :, (py + 1) % 2::2, (px + 1) % 2::2] = float('nan')
      got = case.run(which == 'grouped')
      own = torch.zeros(21, 21, dtype=torch.bool, device=got.device)
      own[py::2, px::2] = True
      assert torch.isnan(got[:B][:, own]).all(), (py, px)
      assert torch.equal(got[:B][:, ~own], clean[:B][:, ~own]), (py, px)
      assert torch.isnan(got[B:]).all(), (py, px)
  finally:
    with torch.no_grad():
      w.copy_(w_saved)
    h.acts['a1'].copy_(a1_saved)
