"""Every layer of the HIP classic-control MLP (dq_mlp_*) against a float64 reference of that
layer alone (oracle/nature_cnn.layer_reference('fc2', ...): a plain dense layer of any shape),
driven through the C ABI.  Cases (B, D, widths, n_out):
  (128, 4, (512, 512), 102)      rainbow_cartpole's own shape;
  (129, 6, (512, 512), 153)      Acrobot; a last 32-row M tile holding one row; K = B = 129 in
                                 the weight gradients (a third 64-window holding one row);
  (3, 6, (24, 24), 3)            widths below one tile;
  (1, 4, (40, 72), 1)            one-term reductions, widths that are multiples of nothing,
                                 n_out = 1;
  (33, 4, (136,), 2)             one hidden layer, float32 input (x_is_f64 = 0);
  (5, 16, (64, 48, 32, 16), 7)   L = 4, D at its cap.
Each layer is fed the device's own input to it, so it is judged alone and its ReLU decision
(in > 0) is the one the device's mask epilogue reads.  The measure and the bar are the
Nature-CNN layer tests' (|got - ref| / max(Σ|terms|, COND_FLOOR max|ref|) <= LAYER_TOL = 1e-5,
element by element; K here is at most 512).  Biases are non-zero.  Every buffer holds one
sample more than the batch, NaN before each call (inputs too: a read past the batch poisons
the result), the workspace 64 NaN words more than dq_mlp_workspace_floats asks for."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import nature_cnn as ONC

pytestmark = pytest.mark.gpu

_CASES = ((128, 4, (512, 512), 102, True), (129, 6, (512, 512), 153, True),
          (3, 6, (24, 24), 3, True), (1, 4, (40, 72), 1, True), (33, 4, (136,), 2, False),
          (5, 16, (64, 48, 32, 16), 7, True))
_NAN = float('nan')


def _net_class(D):
  from dopamine_amd.agents import networks
  if D == 4:
    return networks.CartpoleRainbowNetwork
  if D == 6:
    return networks.AcrobotRainbowNetwork
  rs = np.random.RandomState(D)
  lo = -rs.uniform(0.5, 6.0, size=D)
  return type('Net%d' % D, (networks.BasicDiscreteDomainNetwork,),
              dict(MIN=lo, MAX=lo + rs.uniform(1.0, 12.0, size=D)))


class _Case(object):
  """One network with buffers for B + 1 samples, driven through the C ABI at batch B."""

  def __init__(self, B, D, widths, n_out, f64):
    from dopamine_amd import _lib
    from dopamine_amd.mlp import HipMLP
    torch.manual_seed(1000 * B + n_out)
    self.B, self.D, self.widths, self.n_out, self.L = B, D, widths, n_out, len(widths)
    cls = _net_class(D)
    # num_actions = n_out, one "atom": the output layer is (n_out, widths[-1])
    self.net = cls(n_out, 1, device='cuda', seed=3, network_size=widths)
    assert self.net.fp.offsets['out_w'][1] == (n_out, widths[-1])
    with torch.no_grad():     # non-zero biases so the bias paths are exercised
      for n, prm in self.net.fp.params.items():
        if n.endswith('_b'):
          prm.uniform_(-0.05, 0.1)
    self.hip = h = HipMLP(self.net, B + 1)       # the structs over (B + 1)-sample buffers
    self.need = int(_lib.lib.dq_mlp_workspace_floats(B, ctypes.byref(h._p)))
    self.ws = torch.empty(self.need + 64, device='cuda')
    lo = torch.tensor(cls.MIN, dtype=torch.float64, device='cuda')
    hi = torch.tensor(cls.MAX, dtype=torch.float64, device='cuda')
    self.x = torch.full((B + 1, D), _NAN, dtype=torch.float64, device='cuda')
    self.x[:B] = lo + (hi - lo) * torch.rand(B, D, dtype=torch.float64, device='cuda')
    if not f64:
      self.x = self.x.float()
    self.f64 = f64
    self.dout = torch.full((B + 1, n_out), _NAN, device='cuda')
    self.dout[:B] = torch.randn(B, n_out, device='cuda')
    self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    self.fwd = (ctypes.byref(h._p), B, self.x.data_ptr(), int(f64), ctypes.byref(h._a))
    self.bwd = (ctypes.byref(h._p), ctypes.byref(h._g), B, ctypes.byref(h._a),
                self.dout.data_ptr(), ctypes.byref(h._d))
    # the upstream gradient each hidden layer is tested with
    self.dz = {k: torch.randn_like(v[:B]) for k, v in h.dacts.items()}
    self._refs = {}
    self.forward()

  def name(self, l):
    return 'fc%d' % l if l < self.L else 'out'

  def src(self, l):
    """The activation layer l reads."""
    return 'x0' if l == 0 else 'h%d' % (l - 1)

  def dst(self, l):
    return 'h%d' % l if l < self.L else 'out'

  def call(self, fn, *args):
    """One C ABI call on a NaN workspace; the guard words must survive it."""
    from dopamine_amd import _lib
    self.ws.fill_(_NAN)
    _lib.check(getattr(_lib.lib, fn)(*args), fn)
    torch.cuda.synchronize()
    ONC.assert_guard_untouched('%s workspace' % fn, self.ws, self.need)

  def forward(self):
    for t in self.hip.acts.values():
      t.fill_(_NAN)
    self.call('dq_mlp_forward', *self.fwd, self.ws.data_ptr(), self.stream)

  def layer(self, index, part):
    self.call('dq_mlp_backward_layer', *self.bwd, self.ws.data_ptr(), index, part, self.stream)

  def nan_d(self):
    self.net.fp.grad.fill_(_NAN)
    for t in self.hip.dacts.values():
      t.fill_(_NAN)

  def grad_range(self, name):
    o, shape = self.net.fp.offsets[name]
    return o, o + math.prod(shape)

  def upstream(self, l):
    return self.dout[:self.B] if l == self.L else self.dz['h%d' % l]

  def reference(self, l):
    """The float64 layer on the device's input to it and this case's upstream gradient
    (computed once per layer, shared by the forward and the backward test)."""
    if l not in self._refs:
      prm = self.net.fp.params
      self._refs[l] = ONC.layer_reference('fc2', self.hip.acts[self.src(l)][:self.B],
                                          prm[self.name(l) + '_w'], prm[self.name(l) + '_b'],
                                          self.upstream(l))
    return self._refs[l]

  def what(self, text):
    return 'B=%d D=%d widths=%r n_out=%d %s' % (self.B, self.D, self.widths, self.n_out, text)


@pytest.fixture(scope='module', params=_CASES, ids=lambda c: 'B%d-D%d-L%d-n%d' % (
    c[0], c[1], len(c[2]), c[3]))
def case(request):
  return _Case(*request.param)


def test_rescaled_input_is_bitwise_the_float32_formula(case):
  """acts.x0 == 2 * ((float32(x) - min) / range) - 1, each step rounded to float32, with
  min = float32(MIN) and range = float32(MAX - MIN), the subtraction done in float64."""
  B, net = case.B, case.net
  x = case.x[:B].cpu().numpy().astype(np.float32)
  lo = np.asarray(net.MIN, dtype=np.float64)
  rng = (np.asarray(net.MAX, dtype=np.float64) - lo).astype(np.float32)
  t = x - lo.astype(np.float32)
  t = t / rng
  want = np.float32(2.0) * t - np.float32(1.0)
  assert want.dtype == np.float32
  got = case.hip.acts['x0'][:B].cpu().numpy()
  assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), case.what('x0')
  assert float(np.abs(want).max()) <= 1.0 + 1e-6
  ONC.assert_spare_untouched(case.what('x0'), case.hip.acts['x0'], B)


def test_forward_layers_match_float64(case):
  B = case.B
  for l in range(case.L + 1):
    ref = case.reference(l)
    want = ref['z'] if l == case.L else F.relu(ref['z'])
    got = case.hip.acts[case.dst(l)][:B]
    assert bool((want != 0).any())
    ONC.assert_layer_close(case.what('forward %s' % case.name(l)), got, want, ref['z_abs'])
    ONC.assert_spare_untouched(case.what(case.dst(l)), case.hip.acts[case.dst(l)], B)
  assert bool(torch.isnan(case.x[B:]).all())


@pytest.mark.parametrize('depth', range(5), ids=lambda d: 'layer_L-%d' % d)
def test_backward_layer_matches_float64(case, depth):
  l = case.L - depth            # the output layer first, as the backward runs
  if l < 0:
    return                      # this case has fewer layers (every case runs depth 0 and 1)
  B, h, grad = case.B, case.hip, case.net.fp.grad
  dz, ref = case.upstream(l), case.reference(l)
  read = None if l == case.L else 'h%d' % l
  write = None if l == 0 else 'h%d' % (l - 1)
  case.nan_d()
  if read is not None:
    h.dacts[read][:B] = dz
  case.layer(l, 1)
  name = case.name(l)
  (w0, w1), (b0, b1) = case.grad_range(name + '_w'), case.grad_range(name + '_b')
  ONC.assert_layer_close(case.what('%s weight grad' % name), grad[w0:w1], ref['dw'], ref['dw_abs'])
  ONC.assert_layer_close(case.what('%s bias grad' % name), grad[b0:b1], ref['db'], ref['db_abs'])
  if write is not None:
    case.layer(l, 0)
    got = h.dacts[write][:B]
    assert bool((ref['dx'] != 0).any()) and bool((ref['dx'] == 0).any())   # the mask keeps and drops
    ONC.assert_layer_close(case.what('%s input grad' % name), got, ref['dx'].reshape(got.shape),
                           ref['dx_abs'].reshape(got.shape))
  # nothing else was written: the other layers' gradients, the alignment pads, the spare
  # sample of every d buffer, whatever d buffer this layer does not write
  other = torch.ones_like(grad, dtype=torch.bool)
  other[w0:w1] = False
  other[b0:b1] = False
  assert bool(torch.isnan(grad[other]).all()), case.what('%s wrote outside its gradients' % name)
  assert bool(torch.isfinite(grad[~other]).all())
  for k in h.dacts:
    ONC.assert_spare_untouched(case.what('d ' + k), h.dacts[k], B)
    if k == read:
      assert torch.equal(h.dacts[k][:B], dz), case.what('d %s (read only) changed' % k)
    elif k != write:
      assert bool(torch.isnan(h.dacts[k][:B]).all()), case.what('d %s was written' % k)


def test_whole_backward_equals_its_layers_bitwise_and_repeats(case):
  """dq_mlp_backward == the chain of per-layer calls, bit for bit (with the per-layer float64
  checks above this ties the grouped launches to the reference too), and a second run of
  the forward and the backward on the same inputs gives the same bits."""
  B, h, fp = case.B, case.hip, case.net.fp
  case.nan_d()
  for l in range(case.L, -1, -1):
    case.layer(l, 1)
    if l > 0:
      case.layer(l, 0)
  parts_g = fp.grad.clone()
  parts_d = {n: t.clone() for n, t in h.dacts.items()}
  acts = {n: t.clone() for n, t in h.acts.items()}
  for _ in range(2):
    case.forward()
    for n, t in acts.items():
      assert torch.equal(h.acts[n][:B], t[:B]), case.what('forward %s differs run to run' % n)
    case.nan_d()
    case.call('dq_mlp_backward', *case.bwd, case.ws.data_ptr(), case.stream)
    for (name, view), (o, m) in zip(zip(fp.params.keys(), fp.grad_views), fp.segments()):
      assert bool(torch.isfinite(view).all()), case.what(name)
      assert torch.equal(fp.grad[o:o + m], parts_g[o:o + m]), case.what(name)
    for n, t in parts_d.items():
      assert bool(torch.isfinite(t[:B]).all()), case.what('d ' + n)
      assert torch.equal(h.dacts[n][:B], t[:B]), case.what('d ' + n)
      ONC.assert_spare_untouched(case.what('d ' + n), h.dacts[n], B)


def test_wrong_reference_fails_on_the_device_result():
  """The device's (correct) result against a reference whose bias is negated: the same
  assertion fails, without touching a kernel."""
  case = _Case(3, 6, (24, 24), 3, True)
  prm = case.net.fp.params
  ref = ONC.layer_reference('fc2', case.hip.acts['h0'][:3], prm['fc1_w'], -prm['fc1_b'],
                            case.dz['h1'])
  with pytest.raises(AssertionError, match='ratio'):
    ONC.assert_layer_close('forward fc1, bias negated', case.hip.acts['h1'][:3], F.relu(ref['z']),
                           ref['z_abs'])


@pytest.mark.parametrize('field,value,message', (('in_dim', 17, b'in_dim must be in 1..16'),
                                                 ('n_layers', 5, b'n_layers must be in 1..4'),
                                                 ('width', 1025, b'width must be in 1..1024')))
def test_host_side_argument_refusals(field, value, message):
  """The supported range is checked on the host before anything touches the device: rc -1
  (DQ_E_ARG) and the message, with null buffers everywhere."""
  from dopamine_amd import _lib
  p = _lib.MlpParams(in_dim=4, n_layers=2, n_out=2)
  p.width[0] = p.width[1] = 512
  if field == 'width':
    p.width[1] = value
  else:
    setattr(p, field, value)
  a = _lib.MlpActs()
  rc = _lib.lib.dq_mlp_forward(ctypes.byref(p), 8, None, 1, ctypes.byref(a), None, None)
  assert rc == -1
  assert message in _lib.lib.dq_last_error()
  rc = _lib.lib.dq_mlp_backward(ctypes.byref(p), ctypes.byref(p), 8, ctypes.byref(a), None,
                                ctypes.byref(a), None, None)
  assert rc == -1
  assert message in _lib.lib.dq_last_error()
  assert _lib.lib.dq_mlp_forward(ctypes.byref(p), 0, None, 1, ctypes.byref(a), None, None) == -1
