"""dq_sgd_tf1 (tf.train.GradientDescentOptimizer: var <- var - lr g) at the edges of its
float4 body and scalar tail: n in 0, 1, 3, 4, 5, 1023, 1024, 1025, guard words around each
buffer, three steps at lr 5e-3.  Each step is bitwise numpy float32 ``var - float32(lr) * g``
(the product rounded, then the difference) and within the optimizer tests' rtol 1e-5 /
atol 1e-7 of float64 from the same float32 state; n = 0 writes nothing.  Buffers that are not
16-byte aligned take the scalar path and give the same bits."""
import numpy as np
import pytest
import torch

from tests import fourier_cases as FC

pytestmark = pytest.mark.gpu

LR = 5e-3
GUARD = 8          # floats on each side (32 bytes: the buffer between them stays 16-byte aligned)
_NAN = float('nan')


def _guarded(values, shift=0):
  """(whole buffer, the view of ``values`` inside it) with NaN guard words around the view."""
  n = len(values)
  buf = torch.full((n + 2 * GUARD + shift,), _NAN, device='cuda')
  view = buf[GUARD + shift:GUARD + shift + n]
  view.copy_(torch.from_numpy(values))
  return buf, view


def _guards_intact(buf, n, shift=0):
  return bool(torch.isnan(buf[:GUARD + shift]).all()) and bool(torch.isnan(buf[GUARD + shift + n:]).all())


@pytest.mark.parametrize('shift', (0, 1), ids=('aligned', 'unaligned'))
@pytest.mark.parametrize('n', (0, 1, 3, 4, 5, 1023, 1024, 1025))
def test_three_steps_are_bitwise_numpy_float32(n, shift):
  from dopamine_amd import ops
  rs = np.random.RandomState(n + 7)
  var = rs.standard_normal(n).astype(np.float32)
  vbuf, v = _guarded(var, shift)
  assert n == 0 or (v.data_ptr() % 16 == 0) == (shift == 0)
  opt = ops.TF1GradientDescent(v, LR)
  for step in range(3):
    g = (rs.standard_normal(n) * 10.0 ** rs.randint(-3, 3, size=n)).astype(np.float32)
    gbuf, gv = _guarded(g, shift)
    opt.step(gv)
    torch.cuda.synchronize()
    got = v.cpu().numpy()
    want = FC.sgd32(var, g, LR)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, step)
    np.testing.assert_allclose(got, FC.sgd64(var, g, LR), rtol=1e-5, atol=1e-7)
    assert _guards_intact(vbuf, n, shift) and _guards_intact(gbuf, n, shift), (n, step)
    assert np.array_equal(gv.cpu().numpy().view(np.uint32), g.view(np.uint32))   # read only
    var = want
  if n:
    flipped = var + np.float32(LR) * g       # a wrong reference fails on the device result
    assert not np.allclose(got, flipped, rtol=1e-5, atol=1e-7)


def test_n_zero_launches_nothing_and_bad_arguments_are_refused():
  from dopamine_amd import _lib
  buf = torch.full((16,), _NAN, device='cuda')
  assert _lib.lib.dq_sgd_tf1(buf.data_ptr(), buf.data_ptr(), 0, LR, None) == 0
  torch.cuda.synchronize()
  assert bool(torch.isnan(buf).all())
  assert _lib.lib.dq_sgd_tf1(None, buf.data_ptr(), 4, LR, None) == -1
  assert _lib.lib.dq_sgd_tf1(buf.data_ptr(), None, 4, LR, None) == -1
  assert _lib.lib.dq_sgd_tf1(buf.data_ptr(), buf.data_ptr(), -1, LR, None) == -1


def test_step_is_captured_in_a_graph():
  """No host synchronisation in step(): it records into a HIP graph, and a replay updates."""
  from dopamine_amd import ops
  rs = np.random.RandomState(3)
  var, g = rs.standard_normal(1025).astype(np.float32), rs.standard_normal(1025).astype(np.float32)
  v, gt = torch.from_numpy(var).cuda(), torch.from_numpy(g).cuda()
  opt = ops.TF1GradientDescent(v, LR)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    opt.step(gt)
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    opt.step(gt)
  graph.replay()
  torch.cuda.synchronize()
  want = FC.sgd32(FC.sgd32(var, g, LR), g, LR)
  assert np.array_equal(v.cpu().numpy().view(np.uint32), want.view(np.uint32))
