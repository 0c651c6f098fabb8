"""Every Nature-CNN layer of the HIP path against a float64 reference of that layer alone
(oracle/nature_cnn.layer_reference), at the batches and output widths where the code takes
another path:
  (32, 918)  Rainbow with the full 18-action set: fc2's input gradient has K = n_out = 918,
             a second, ragged 512-wide K slice; fc2's weight gradient seven full 128-row
             tiles and a ragged eighth;
  (33, 918)  a second 32-row M tile holding one row in the fc layers; K = B = 33 in the fc
             weight gradients (a second 32-slice holding one row); conv1's split-K chunk of
             1024 (two K slices per slab);
  (5, 129)   two conv2 / conv3 weight-gradient slabs, the second ragged (93 rows), five conv1
             slabs; n_out = 129: a second 128-row tile / fifth 32-column tile with one entry;
  (1, 1)     one-term reductions in the fc weight gradients, one split-K slab, n_out = 1.
Each layer is fed the device's own input to it, so it is judged alone and its ReLU decision
(in > 0) is the one the device's mask epilogue reads.  The measure and the bar are the
north-star test's (|got - ref| / max(Σ|terms|, COND_FLOOR max|ref|) <= 1e-5, element by
element); tests/test_cnn_layer_reference_cpu.py shows fp32 CPU arithmetic passing it with
45x to spare and subtly wrong results failing it.  Every buffer holds one sample more than
the batch, NaN before each call (inputs too: a read past the batch poisons the result), the
workspace 64 NaN words more than dq_cnn_workspace_floats asks for."""
import pytest
import torch
import torch.nn.functional as F

from oracle import nature_cnn as ONC
from tests.cnn_layer_case import BACKWARD as _BACKWARD, FORWARD as _FORWARD, LayerCase as _Case

pytestmark = pytest.mark.gpu

_CASES = ((32, 918), (33, 918), (5, 129), (1, 1))     # product-like first, degenerate last

@pytest.fixture(scope='module', params=_CASES, ids=lambda c: 'B%d-n%d' % c)
def case(request):
  return _Case(*request.param)


def test_forward_layers_match_float64(case):
  B = case.B
  for layer, src, dst in _FORWARD:
    ref = case.reference(layer)
    want = ref['z'] if layer == 'fc2' else F.relu(ref['z'])
    got = case.acts[dst][:B].reshape(want.shape)
    assert bool((want != 0).any())
    ONC.assert_layer_close(case.what('forward %s' % layer), got, want, ref['z_abs'])
    ONC.assert_spare_untouched(case.what(dst), case.acts[dst], B)


@pytest.mark.parametrize('index,layer,src,read,write', _BACKWARD, ids=[b[1] for b in _BACKWARD])
def test_backward_layer_matches_float64(case, index, layer, src, read, write):
  B, h, grad = case.B, case.hip, case.net.fp.grad
  dz, ref = case.upstream(read), case.reference(layer)
  case.nan_d()
  if read is not None:
    h.dacts[read][:B] = dz
  case.layer(index, 1)
  (w0, w1), (b0, b1) = case.grad_range(layer + '_w'), case.grad_range(layer + '_b')
  ONC.assert_layer_close(case.what('%s weight grad' % layer), grad[w0:w1], ref['dw'], ref['dw_abs'])
  ONC.assert_layer_close(case.what('%s bias grad' % layer), grad[b0:b1], ref['db'], ref['db_abs'])
  if write is not None:
    case.layer(index, 0)
    got = h.dacts[write][:B]
    assert bool((ref['dx'] != 0).any()) and bool((ref['dx'] == 0).any())   # the mask keeps and drops
    ONC.assert_layer_close(case.what('%s input grad' % layer), got, ref['dx'].reshape(got.shape),
                           ref['dx_abs'].reshape(got.shape))
  # nothing else was written: the other layers' gradients, the alignment pads, the spare
  # sample of every d buffer, whatever d buffer this layer does not write
  other = torch.ones_like(grad, dtype=torch.bool)
  other[w0:w1] = False
  other[b0:b1] = False
  assert bool(torch.isnan(grad[other]).all()), case.what('%s wrote outside its gradients' % layer)
  assert bool(torch.isfinite(grad[~other]).all())
  for name in ('h', 'a3', 'a2', 'a1'):
    ONC.assert_spare_untouched(case.what('d ' + name), h.dacts[name], B)
    if name == read:
      assert torch.equal(h.dacts[name][:B], dz), case.what('d %s (read only) changed' % name)
    elif name != write:
      assert bool(torch.isnan(h.dacts[name][:B]).all()), case.what('d %s was written' % name)


def test_whole_backward_equals_its_layers_bitwise(case):
  """dq_cnn_backward == the chain of per-layer calls, bit for bit: with the per-layer float64
  checks above this ties the grouped schedule's launches to the reference too."""
  B, h, fp = case.B, case.hip, case.net.fp
  case.nan_d()
  for index, _, _, _, write in _BACKWARD:
    case.layer(index, 1)
    if write is not None:
      case.layer(index, 0)
  parts_g = fp.grad.clone()
  parts_d = {n: h.dacts[n].clone() for n in ('h', 'a3', 'a2', 'a1')}
  case.nan_d()
  case.call('dq_cnn_backward', *case.bwd, case.ws.data_ptr(), case.stream)
  for (name, view), (o, m) in zip(zip(fp.params.keys(), fp.grad_views), fp.segments()):
    assert bool(torch.isfinite(view).all()), case.what(name)
    assert torch.equal(fp.grad[o:o + m], parts_g[o:o + m]), case.what(name)
  for n, t in parts_d.items():
    assert bool(torch.isfinite(t[:B]).all()), case.what('d ' + n)
    assert torch.equal(h.dacts[n][:B], t[:B]), case.what('d ' + n)
    ONC.assert_spare_untouched(case.what('d ' + n), h.dacts[n], B)
    ONC.assert_spare_untouched(case.what('d %s (per layer)' % n), t, B)


def test_wrong_reference_fails_on_the_device_result():
  """The device's (correct) conv2 against a reference with conv2's SAME padding flipped to 2
  before, 1 after: the same assertions fail, without touching a kernel."""
  case = _Case(5, 129)
  B, h = case.B, case.hip
  ref = case.reference('conv2', pad=(2, 1, 2, 1))
  with pytest.raises(AssertionError, match='ratio'):
    ONC.assert_layer_close('forward conv2, padding flipped', case.acts['a2'][:B], F.relu(ref['z']),
                           ref['z_abs'])
  case.nan_d()
  h.dacts['a2'][:B] = case.dz['a2']
  case.layer(3, 1)
  case.layer(3, 0)
  w0, w1 = case.grad_range('conv2_w')
  with pytest.raises(AssertionError, match='ratio'):
    ONC.assert_layer_close('conv2 weight grad, padding flipped', case.net.fp.grad[w0:w1], ref['dw'],
                           ref['dw_abs'])
  with pytest.raises(AssertionError, match='ratio'):
    ONC.assert_layer_close('conv2 input grad, padding flipped', h.dacts['a1'][:B], ref['dx'],
                           ref['dx_abs'])
