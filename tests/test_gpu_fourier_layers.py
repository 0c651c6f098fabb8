"""The two Fourier-basis kernels (dq_fourier_forward / dq_fourier_backward) against float64,
driven through the C ABI.  Cases (B, D, order, A) and the edge each is there for:
  (128, 4, 3, 2)   F = 255    CartPole's own shape; one short of a 256-thread round;
  (33, 6, 3, 3)    F = 4095   Acrobot; 15 full rounds plus one of 255; the largest |arg|;
                              float32 input (x_is_f64 = 0);
  (1, 1, 1, 1)     F = 1      one term everywhere;
  (5, 2, 4, 7)     F = 24     base 5, so digits by division and not shifts; fewer features
                              than a wave; two action passes, the second partial;
  (3, 3, 6, 5)     F = 342    256 + 86 features; B below the slice count;
  (257, 2, 3, 4)   F = 15     uneven batch slices; exactly one full action pass.
States are drawn from 10% outside the box on both sides.  Every buffer holds one sample more
than the batch, NaN before each call (inputs too: a read past the batch poisons the result),
and the spare rows must stay NaN.

The bars:
  s     bitwise the float32 formula (x32 - float32(MIN)) / float32(MAX - MIN).
  phi   |phi - cos(float32(pi) z)| <= 2 D 2^-24 max(1, |arg|) + 2^-22, z formed in float64
        from the device's s.  Derivation: the D products m_d s_d, the D - 1 sums and the
        multiplication by float32(pi) round once each -- 2 D roundings, each at most 2^-24 of
        a partial result that |arg| bounds, which the cosine (slope at most 1) passes on
        unamplified -- and the cosine itself gets two ulp of a value at most 1, 2^-22.  The
        fp32 numpy restatement reads at most 2.4e-7 max(1, |arg|) on these cases on the CPU.
  q, dW oracle.nature_cnn.layer_reference('fc2', ...) with a zero bias on the device's own phi,
        by that file's measure (|got - ref| / max(Σ|terms|, COND_FLOOR max|ref|)) at LAYER_TOL
        = 1e-5; sequential fp32 reads at most 1.8e-7 on the CPU at F = 4,095.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import nature_cnn as ONC
from tests import fourier_cases as FC

pytestmark = pytest.mark.gpu

_NAN = float('nan')


class _Case(object):
  """One head with buffers for B + 1 samples, driven through the C ABI at batch B."""

  def __init__(self, case):
    from dopamine_amd import _lib
    self.case = case
    self.B, self.D, self.order, self.A, self.f64 = B, D, order, A, f64 = case
    self.F = F = FC.n_features(D, order)
    assert int(_lib.lib.dq_fourier_features(D, order)) == F
    x, w, dq = FC.make_inputs(case)
    self.x_np, self.w_np, self.dq_np = x, w, dq
    full = lambda rows, a: torch.cat([torch.from_numpy(a), torch.full(
        (1,) + a.shape[1:], _NAN, dtype=torch.from_numpy(a).dtype)]).cuda()
    self.x, self.dout = full(B, x), full(B, dq)
    # the parameter and its gradient between guard words
    self.w = torch.full((A * F + 128,), _NAN, device='cuda')
    self.w[64:64 + A * F] = torch.from_numpy(w).reshape(-1).cuda()
    self.g = torch.full((A * F + 128,), _NAN, device='cuda')
    self.s = torch.empty(B + 1, D, device='cuda')
    self.phi = torch.empty(B + 1, F, device='cuda')
    self.out = torch.empty(B + 1, A, device='cuda')
    lo, hi = FC.bounds(D)
    rng = (hi - lo).astype(np.float32)
    mk = lambda buf: _lib.FourierParams(in_dim=D, order=order, n_out=A, w=buf.data_ptr() + 256)
    self.p, self.gp = mk(self.w), mk(self.g)
    for st in (self.p, self.gp):
      for d in range(D):
        st.in_min[d] = float(np.float32(lo[d]))
        st.in_range[d] = float(rng[d])
    self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    self.forward()

  def acts(self, s=True, phi=True):
    from dopamine_amd import _lib
    return _lib.FourierActs(s=self.s.data_ptr() if s else None,
                            phi=self.phi.data_ptr() if phi else None, out=self.out.data_ptr())

  def forward(self, s=True, phi=True):
    from dopamine_amd import _lib
    for t in (self.s, self.phi, self.out):
      t.fill_(_NAN)
    a = self.acts(s, phi)
    _lib.check(_lib.lib.dq_fourier_forward(ctypes.byref(self.p), self.B, self.x.data_ptr(),
                                           int(self.f64), ctypes.byref(a), self.stream),
               'dq_fourier_forward')
    torch.cuda.synchronize()

  def backward(self):
    from dopamine_amd import _lib
    self.g.fill_(_NAN)
    a = self.acts()
    _lib.check(_lib.lib.dq_fourier_backward(ctypes.byref(self.p), ctypes.byref(self.gp), self.B,
                                            ctypes.byref(a), self.dout.data_ptr(), self.stream),
               'dq_fourier_backward')
    torch.cuda.synchronize()

  def grad(self):
    return self.g[64:64 + self.A * self.F]

  def reference(self):
    """float64 head on the device's own phi (computed once, left unchanged)."""
    if not hasattr(self, '_ref'):
      w = torch.from_numpy(self.w_np)
      self._ref = ONC.layer_reference('fc2', self.phi[:self.B], w, torch.zeros(self.A),
                                      self.dout[:self.B])
    return self._ref

  def what(self, text):
    return '%s %s' % (FC.case_id(self.case), text)


@pytest.fixture(scope='module', params=FC.CASES, ids=FC.case_id)
def case(request):
  return _Case(request.param)


def test_scaled_input_is_bitwise_the_float32_formula(case):
  want = FC.scale32(case.x_np, *FC.bounds(case.D))
  got = case.s[:case.B].cpu().numpy()
  assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), case.what('s')
  assert float(want.min()) < 0.0 and (want.size == 1 or float(want.max()) > 1.0)   # no clipping
  ONC.assert_spare_untouched(case.what('s'), case.s, case.B)


def test_features_match_float64_cosine(case):
  B = case.B
  phi, s = case.phi[:B].cpu().numpy(), case.s[:B].cpu().numpy()
  assert np.isfinite(phi).all()
  share, per_arg = FC.phi_excess(phi, s, case.D, case.order)
  _, arg = FC.phi64(s, case.D, case.order)
  print('%s: worst share of the bound %.3g, worst error / max(1, |arg|) %.3g, max |arg| %.3g'
        % (case.what('phi'), share, per_arg, np.abs(arg).max()))
  assert share <= 1.0, case.what('phi over its bound')
  ONC.assert_spare_untouched(case.what('phi'), case.phi, B)


def test_head_forward_matches_float64(case):
  ref = case.reference()
  ONC.assert_layer_close(case.what('q'), case.out[:case.B], ref['z'], ref['z_abs'])
  ONC.assert_spare_untouched(case.what('out'), case.out, case.B)
  assert bool(torch.isnan(case.x[case.B:]).all())


def test_weight_gradient_matches_float64(case):
  ref = case.reference()
  case.backward()
  ONC.assert_layer_close(case.what('dW'), case.grad(), ref['dw'], ref['dw_abs'])
  n = case.A * case.F
  assert bool(torch.isnan(case.g[:64]).all()) and bool(torch.isnan(case.g[64 + n:]).all()), \
      case.what('dW wrote outside the gradient')
  assert bool(torch.isnan(case.dout[case.B:]).all())


def test_forward_without_phi_is_bitwise_the_forward_with_it(case):
  B = case.B
  out, s = case.out[:B].clone(), case.s[:B].clone()
  case.forward(phi=False)
  assert bool(torch.isnan(case.phi).all()), case.what('phi written through a null pointer?')
  assert torch.equal(case.out[:B], out) and torch.equal(case.s[:B], s)
  case.forward(s=False, phi=False)
  assert bool(torch.isnan(case.s).all())
  assert torch.equal(case.out[:B], out)
  case.forward()


def test_two_launches_are_bitwise_equal(case):
  B = case.B
  case.backward()
  first = [t.clone() for t in (case.s[:B], case.phi[:B], case.out[:B], case.grad())]
  case.forward()
  case.backward()
  for a, b in zip(first, (case.s[:B], case.phi[:B], case.out[:B], case.grad())):
    assert bool(torch.isfinite(b).all()) and torch.equal(a, b), case.what('differs run to run')


def test_wrong_reference_fails_on_the_device_result():
  """The device's (correct) results against wrong references: the same assertions fail,
  without touching a kernel."""
  c = _Case((5, 2, 4, 7, True))
  s = c.s[:5].cpu().numpy()
  assert FC.phi_excess(c.phi[:5].cpu().numpy(), s[:, ::-1], c.D, c.order)[0] > 1.0
  ref = ONC.layer_reference('fc2', c.phi[:5], -torch.from_numpy(c.w_np), torch.zeros(7),
                            c.dout[:5])
  with pytest.raises(AssertionError, match='ratio'):
    ONC.assert_layer_close('q, weights negated', c.out[:5], ref['z'], ref['z_abs'])
  c.backward()
  wrong = ONC.layer_reference('fc2', c.phi[:4], torch.from_numpy(c.w_np), torch.zeros(7),
                              c.dout[:4])          # the last batch row dropped
  with pytest.raises(AssertionError, match='ratio'):
    ONC.assert_layer_close('dW, a row short', c.grad(), wrong['dw'], wrong['dw_abs'])


_REFUSALS = (
    (dict(in_dim=0), b'in_dim must be in 1..16'), (dict(in_dim=17), b'in_dim must be in 1..16'),
    (dict(order=0), b'order must be >= 1'),
    (dict(in_dim=7, order=3), b'features exceed 16383'),     # 4^7 - 1 = 16383 passes, see below
    (dict(in_dim=16, order=15), b'features exceed 16383'),   # 16^16 overflows 64 bits unchecked
    (dict(n_out=0), b'n_out must be in 1..64'), (dict(n_out=65), b'n_out must be in 1..64'),
    (dict(batch=0), b'batch must be >= 1'))


@pytest.mark.parametrize('change,message', _REFUSALS, ids=lambda v: (
    '-'.join('%s%d' % kv for kv in v.items()) if isinstance(v, dict) else None))
def test_host_side_shape_refusals(change, message):
  """Checked on the host before anything touches the device: DQ_E_ARG and the message from
  both entry points, with null buffers everywhere."""
  from dopamine_amd import _lib
  kw = dict(in_dim=4, order=3, n_out=2, batch=8)
  kw.update(change)
  batch = kw.pop('batch')
  if change == dict(in_dim=7, order=3):
    assert _lib.lib.dq_fourier_features(7, 3) == 16383 == _lib.FOURIER_MAX_FEATURES
    kw['order'] = 4
  p, a = _lib.FourierParams(**kw), _lib.FourierActs()
  if 'n_out' not in change and 'batch' not in change:
    assert _lib.lib.dq_fourier_features(kw['in_dim'], kw['order']) == 0
  rc = _lib.lib.dq_fourier_forward(ctypes.byref(p), batch, None, 1, ctypes.byref(a), None)
  assert rc == -1 and message in _lib.lib.dq_last_error()
  rc = _lib.lib.dq_fourier_backward(ctypes.byref(p), ctypes.byref(p), batch, ctypes.byref(a), None,
                                    None)
  assert rc == -1 and message in _lib.lib.dq_last_error()


def test_null_pointer_refusals():
  from dopamine_amd import _lib
  buf = torch.zeros(2 * 255 + 8 * 255 + 64, device='cuda')
  ptr = buf.data_ptr()
  fwd = lambda p, x, a: _lib.lib.dq_fourier_forward(ctypes.byref(p), 8, x, 0, ctypes.byref(a), None)
  bwd = lambda p, g, a, d: _lib.lib.dq_fourier_backward(ctypes.byref(p), ctypes.byref(g), 8,
                                                        ctypes.byref(a), d, None)
  P = lambda w: _lib.FourierParams(in_dim=4, order=3, n_out=2, w=w)
  A = lambda **k: _lib.FourierActs(**k)
  before = buf.clone()
  for args, msg in (((P(None), ptr, A(out=ptr)), b'null w'), ((P(ptr), None, A(out=ptr)), b'null x'),
                    ((P(ptr), ptr, A()), b'null out')):
    assert fwd(*args) == -1 and msg in _lib.lib.dq_last_error(), msg
  assert bwd(P(ptr), P(ptr), A(out=ptr), ptr) == -1 and b'null phi' in _lib.lib.dq_last_error()
  assert bwd(P(ptr), P(ptr), A(phi=ptr), None) == -1 and b'null dout' in _lib.lib.dq_last_error()
  assert bwd(P(ptr), P(None), A(phi=ptr), ptr) == -1 and b'null g->w' in _lib.lib.dq_last_error()
  torch.cuda.synchronize()
  assert torch.equal(buf, before)
