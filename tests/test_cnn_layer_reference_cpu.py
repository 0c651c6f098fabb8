"""The per-layer float64 reference and its measure (oracle/nature_cnn.py layer_reference,
cond_ratio, assert_layer_close), which tests/test_gpu_cnn_layers.py holds every Nature-CNN
layer of the device to, checked here without a GPU:

* calibration: torch's own fp32 CPU convolutions and GEMMs, layer by layer on the GPU tests'
  input distributions at (B, n_out) = (1, 1) and (5, 129), pass the measure with at least
  3x to spare under the bar -- the reference and its Σ|terms| alone stay inside it;
* sensitivity: the same assertion fails on a subtly wrong result (made here on the CPU): a
  flipped SAME padding, a dropped last row of a ragged tile, a dropped tail of the last K
  slice, a column stored one place to the right;
* the guard checks of the GPU tests fail on a buffer without a spare sample and on a
  workspace without guard words.
"""
import pytest
import torch
import torch.nn.functional as F

from dopamine_amd.agents import networks
from oracle import nature_cnn as ONC

MARGIN = 3.0
_PARTS = (('forward', 'z'), ('input grad', 'dx'), ('weight grad', 'dw'), ('bias grad', 'db'))


def _net(n_out, seed=3):
  net = (networks.RainbowNetwork(n_out // 51, device='cpu', seed=seed) if n_out == 918 else
         networks.NatureDQNNetwork(n_out, device='cpu', seed=seed))
  with torch.no_grad():       # non-zero biases, as in tests/test_gpu_cnn.py
    for n, prm in net.fp.params.items():
      if n.endswith('_b'):
        prm.uniform_(-0.05, 0.1)
  return net


def _fp32_layer(layer, x_in, w, b, dz, pad=None):
  """The layer in torch fp32 CPU arithmetic, in layer_reference's layouts."""
  B = x_in.shape[0]
  x = x_in.detach().float().clone()
  w = w.detach().float().clone().requires_grad_(True)
  b = b.detach().float().clone().requires_grad_(True)
  if layer in ONC._CONVS:
    p, stride, ishape, oshape = ONC._CONVS[layer]
    xi = x.reshape((B,) + ishape).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    z = F.conv2d(F.pad(xi, p if pad is None else pad), w, b, stride=stride)
    z.backward(dz.float().reshape((B,) + oshape).permute(0, 3, 1, 2))
    keep = (xi > 0).float()
    return dict(z=z.detach().permute(0, 2, 3, 1),
                dx=(xi.grad * keep).permute(0, 2, 3, 1).reshape(x_in.shape),
                dw=w.grad.permute(0, 2, 3, 1).reshape(-1), db=b.grad)
  xi = x.reshape(B, -1).requires_grad_(True)
  z = F.linear(xi, w, b)
  z.backward(dz.float().reshape(B, -1))
  return dict(z=z.detach(), dx=xi.grad * (xi > 0).float(), dw=w.grad.reshape(-1), db=b.grad)


class _Run(object):
  """fp32 CPU forward of a network, each layer's input kept (as the device keeps its
  activations), and a randn pre-activation gradient per layer."""

  def __init__(self, B, n_out, seed=0):
    torch.manual_seed(seed)
    self.B, self.n_out = B, n_out
    self.net = _net(n_out)
    prm = self.net.fp.params
    self.inputs, self.dz = {}, {}
    a = torch.rand(B, 84, 84, 4)
    for layer in ONC.LAYERS:
      self.inputs[layer] = a
      z = _fp32_layer(layer, a, prm[layer + '_w'], prm[layer + '_b'],
                      self._zero_dz(layer, B, n_out))['z']
      self.dz[layer] = torch.randn(z.shape)
      a = F.relu(z).reshape(B, -1) if layer in ('conv3', 'fc1') else F.relu(z)

  @staticmethod
  def _zero_dz(layer, B, n_out):
    shape = (ONC._CONVS[layer][3] if layer in ONC._CONVS else ((512,) if layer == 'fc1' else (n_out,)))
    return torch.zeros((B,) + tuple(shape))

  def both(self, layer, pad=None):
    prm = self.net.fp.params
    args = (layer, self.inputs[layer], prm[layer + '_w'], prm[layer + '_b'], self.dz[layer])
    return _fp32_layer(*args, pad=pad), ONC.layer_reference(*args)


def _check(what, got, ref, key, tol=ONC.LAYER_TOL):
  want = F.relu(ref['z']) if key == 'z' and what.split()[0] != 'fc2' else ref[key]
  have = F.relu(got['z']) if key == 'z' and what.split()[0] != 'fc2' else got[key]
  return ONC.assert_layer_close(what, have, want, ref[key + '_abs'], tol)


@pytest.fixture(scope='module', params=[(1, 1), (5, 129)], ids=lambda c: 'B%d-n%d' % c)
def run(request):
  return _Run(*request.param)


def test_the_bar_is_the_projects():
  assert ONC.COND_FLOOR == 1e-3 and ONC.LAYER_TOL == 1e-5    # tests/test_gpu_northstar.py


def test_fp32_cpu_arithmetic_passes_with_margin(run):
  for layer in ONC.LAYERS:
    got, ref = run.both(layer)
    for part, key in _PARTS:
      what = '%s %s B=%d n_out=%d (fp32 CPU)' % (layer, part, run.B, run.n_out)
      worst = _check(what, got, ref, key)
      assert worst * MARGIN <= ONC.LAYER_TOL, '%s: %.3g is not %gx under %g' % (
          what, worst, MARGIN, ONC.LAYER_TOL)
      assert bool((ref[key] != 0).any()), what          # the reference is not trivially zero


def test_reference_masks_with_the_given_input(run):
  got, ref = run.both('conv3')
  x = run.inputs['conv3']
  assert bool((x <= 0).any()) and bool((x > 0).any())
  assert bool((ref['dx'][x <= 0] == 0).all()) and bool((ref['dx_abs'][x <= 0] == 0).all())


def test_flipped_conv2_padding_fails(run):
  """conv2's SAME padding taken as 2 before, 1 after: every part that reads a pixel
  position is wrong (the bias gradient reads none)."""
  got, ref = run.both('conv2', pad=(2, 1, 2, 1))
  for part, key in _PARTS[:3]:
    with pytest.raises(AssertionError, match='ratio'):
      _check('conv2 %s, padding flipped' % part, got, ref, key)
  _check('conv2 bias grad, padding flipped', got, ref, 'db')


def test_dropped_last_row_of_a_ragged_tile_fails():
  """M = B * 121 rows with B = 1: the fourth 32-row tile holds 25 rows; its last one (pixel
  120) left zero, in conv3's output and in conv3's input gradient."""
  run = _Run(1, 1)
  got, ref = run.both('conv3')
  for key in ('z', 'dx'):
    bad = dict(got)
    rows = got[key].clone().reshape(121, 64)
    assert bool((F.relu(rows[120]) != 0).any() if key == 'z' else (rows[120] != 0).any())
    rows[120] = 0.0
    bad[key] = rows.reshape(got[key].shape)
    _check('conv3 %s' % key, got, ref, key)
    with pytest.raises(AssertionError, match='ratio'):
      _check('conv3 %s, row 120 dropped' % key, bad, ref, key)


def test_dropped_tail_of_the_second_k_slice_fails():
  """fc2's input gradient at n_out = 918 (K = n_out: one 512-wide slice and a ragged second
  one) with the last 32 entries of K left out."""
  torch.manual_seed(2)
  B = 3
  net = _net(918)
  w, b = net.fp.params['fc2_w'], net.fp.params['fc2_b']
  h = F.relu(torch.randn(B, 512))
  dz = torch.randn(B, 918)
  ref = ONC.layer_reference('fc2', h, w, b, dz)
  got = _fp32_layer('fc2', h, w, b, dz)
  _check('fc2 input grad n_out=918', got, ref, 'dx')
  cut = dz.clone()
  cut[:, 918 - 32:] = 0.0
  bad = _fp32_layer('fc2', h, w, b, cut)
  with pytest.raises(AssertionError, match='ratio'):
    _check('fc2 input grad n_out=918, K tail dropped', bad, ref, 'dx')


def test_a_column_stored_one_place_to_the_right_fails(run):
  for layer, key in (('conv1', 'z'), ('fc1', 'dx'), ('fc2', 'dw')):
    got, ref = run.both(layer)
    cols = got[key].clone().reshape(-1, 512 if key == 'dw' else got[key].shape[-1])
    # (two equal neighbours, e.g. both cut by the ReLU, shift unseen: take a pair that differs)
    c = int((cols[:, 1:] - cols[:, :-1]).abs().amax(0).argmax())
    cols[:, c + 1] = cols[:, c]
    bad = dict(got)
    bad[key] = cols.reshape(got[key].shape)
    with pytest.raises(AssertionError, match='ratio'):
      _check('%s %s, column %d stored at %d' % (layer, key, c, c + 1), bad, ref, key)


def test_a_nan_fails():
  ref = torch.ones(4, dtype=torch.float64)
  got = ref.clone()
  got[2] = float('nan')
  with pytest.raises(AssertionError, match='not finite'):
    ONC.assert_layer_close('nan', got, ref, ref)


def test_guard_checks_fail_without_a_spare_sample_or_guard_words():
  """Host tensors only: what the GPU tests' guard assertions do with a buffer that has no
  room for them (an empty slice is all-NaN vacuously) and with one that was written."""
  B, need = 5, 1000
  nan = float('nan')
  good = torch.full((B + 1, 7), nan)
  good[:B] = 1.0
  ONC.assert_spare_untouched('good', good, B)
  with pytest.raises(AssertionError, match='no spare'):
    ONC.assert_spare_untouched('no spare sample', good[:B], B)
  hit = good.clone()
  hit[B, 3] = 0.0
  with pytest.raises(AssertionError, match='was written'):
    ONC.assert_spare_untouched('written', hit, B)
  ws = torch.full((need + 64,), nan)
  ws[:need] = 2.0
  ONC.assert_guard_untouched('good', ws, need)
  with pytest.raises(AssertionError, match='guard words'):
    ONC.assert_guard_untouched('no guard words', torch.full((need,), nan), need)
  ws[need] = 0.0
  with pytest.raises(AssertionError, match='were written'):
    ONC.assert_guard_untouched('written', ws, need)
