"""One implicit-quantile head driven through the C ABI, as tests/test_gpu_iqn_head.py and
tests/bf16_build_child.py (the same drive on the bf16 throughput build, in a process of its
own) use it: every R-row buffer holds R + 1 rows and the state B + 1, NaN before each call
(inputs too), the workspace 64 NaN words more than dq_iqn_workspace_floats asks for, the whole
flat gradient buffer NaN before each backward.  The library is whichever dopamine_amd._lib
loaded."""
import ctypes
import math

import torch

from oracle import iqn_head as OIH

NAN = float('nan')
F, H = OIH.F, OIH.H
# forward forms: (emb kept, x stored)
FORMS = {'emb': (True, False), 'emb+x': (True, True), 'x': (False, True)}
GRAD_STAGES = (('dwe', 'emb_w'), ('dbe', 'emb_b'), ('dw1', 'fc1_w'), ('db1', 'fc1_b'),
               ('dw2', 'fc2_w'), ('db2', 'fc2_b'))
SEED = (1 << 63) + 0xC0FFEE1234567        # the top bit set: the seed is unsigned


def _spare(rows, *shape):
  return torch.full((rows + 1,) + shape, NAN, device='cuda')


class HeadCase(object):
  """One head over an ImplicitQuantileNetwork's flat buffers, with activation and gradient
  buffers the test owns, driven through the C ABI; the torso never runs."""

  def __init__(self, B, nq, A, E):
    from dopamine_amd import _lib
    from dopamine_amd.iqn import _head_struct
    self.B, self.nq, self.A, self.E, self.R = B, nq, A, E, B * nq
    self.fused = 128 % nq == 0
    R = self.R
    self.net, state, taus, dq = OIH.make_inputs(B, nq, A, E, device='cuda')
    fp = self.net.fp
    assert fp.offsets['emb_w'][1] == (F, E) and fp.offsets['fc2_w'][1] == (A, H)
    assert all(bool((fp.params[n] != 0).all()) for n in ('emb_b', 'fc1_b', 'fc2_b'))
    self.host = dict(state=state, taus=taus, dq=dq)
    self.state, self.taus, self.dq = _spare(B, F), _spare(R), _spare(R, A)
    self.state[:B], self.taus[:R], self.dq[:R] = state.cuda(), taus.cuda(), dq.cuda()
    self.acts = dict(cos=_spare(R, E), emb=_spare(R, F), x=_spare(R, F), h=_spare(R, H),
                     q=_spare(R, A))
    self.grads = dict(dh=_spare(R, H), dpre=_spare(R, F), dtl=_spare(R, F))
    self.dstate = _spare(B, F)
    self.need = int(_lib.lib.dq_iqn_workspace_floats(B, nq, A, E))
    self.ws = torch.empty(self.need + 64, device='cuda')
    self._p = _head_struct(fp, fp.flat, A, E)
    self._g = _head_struct(fp, fp.grad, A, E)
    self._d = _lib.IqnGrads(**{k: v.data_ptr() for k, v in self.grads.items()})
    self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    self.head = torch.zeros(fp.grad.numel(), dtype=torch.bool, device='cuda')
    for n in OIH.HEAD:
      o, shape = fp.offsets[n]
      self.head[o:o + math.prod(shape)] = True
    self._ran = None

  def what(self, text=''):
    return 'B=%d nq=%d A=%d E=%d %s' % (self.B, self.nq, self.A, self.E, text)

  def call(self, fn, *args):
    """One C ABI call on a NaN workspace; the guard words must survive it."""
    from dopamine_amd import _lib
    self.ws.fill_(NAN)
    _lib.check(getattr(_lib.lib, fn)(*args), fn)
    torch.cuda.synchronize()
    OIH.assert_guard_untouched(self.what(fn + ' workspace'), self.ws, self.need)

  def _acts_struct(self, emb, x):
    from dopamine_amd import _lib
    use = dict(self.acts, emb=self.acts['emb'] if emb else None, x=self.acts['x'] if x else None)
    return _lib.IqnActs(**{k: (v.data_ptr() if v is not None else None) for k, v in use.items()})

  def forward(self, form, taus=True):
    """The forward in one of FORMS on NaN outputs (cos too, unless it comes with the draws:
    taus False).  Returns clones of (cos, emb, x, h, q)."""
    emb, x = FORMS[form]
    for n, t in self.acts.items():
      if n != 'cos' or taus:
        t.fill_(NAN)
    a = self._acts_struct(emb, x)
    self.call('dq_iqn_head_forward', ctypes.byref(self._p), self.B, self.nq, self.state.data_ptr(),
              self.taus.data_ptr() if taus else None, ctypes.byref(a), self.ws.data_ptr(),
              self.stream)
    for n, t in self.acts.items():
      OIH.assert_spare_untouched(self.what('%s (forward %s)' % (n, form)), t, self.R)
      written = bool(torch.isfinite(t[:self.R]).all())
      if n in ('emb', 'x') and not dict(emb=emb, x=x)[n]:
        assert bool(torch.isnan(t[:self.R]).all()), self.what('%s written in form %s' % (n, form))
      else:
        assert written, self.what('%s not finite in form %s' % (n, form))
    return {n: t.clone() for n, t in self.acts.items()}

  def backward(self, x_stored):
    """The backward on NaN gradient buffers (the whole flat gradient, dh, dpre, dtl, d state).
    acts must hold a forward that kept emb (and stored x, if x_stored).  Returns clones."""
    self.net.fp.grad.fill_(NAN)
    for t in list(self.grads.values()) + [self.dstate]:
      t.fill_(NAN)
    a = self._acts_struct(True, x_stored)
    self.call('dq_iqn_head_backward', ctypes.byref(self._p), ctypes.byref(self._g), self.B, self.nq,
              self.state.data_ptr(), ctypes.byref(a), self.dq.data_ptr(), ctypes.byref(self._d),
              self.dstate.data_ptr(), self.ws.data_ptr(), self.stream)
    out = {n: t.clone() for n, t in self.grads.items()}
    out.update(dstate=self.dstate.clone(), grad=self.net.fp.grad.clone())
    return out

  def ran(self):
    """The forward (emb kept, x stored) and the backward (x stored) every test starts from,
    and the float64 reference on their intermediates: run once, left unchanged."""
    if self._ran is None:
      fwd = self.forward('emb+x')
      before = {n: t.clone() for n, t in dict(self.acts, dq=self.dq, state=self.state,
                                              taus=self.taus).items()}
      bwd = self.backward(True)
      for n, t in dict(self.acts, dq=self.dq, state=self.state, taus=self.taus).items():
        rows = self.B if n == 'state' else self.R          # (the spare rows are NaN)
        assert torch.equal(t[:rows], before[n][:rows]), self.what('%s changed by the backward' % n)
        OIH.assert_spare_untouched(self.what(n + ' after the backward'), t, rows)
      R = self.R
      dev = dict(cos=fwd['cos'][:R], emb=fwd['emb'][:R], h=fwd['h'][:R], dh=bwd['dh'][:R],
                 dpre=bwd['dpre'][:R])
      self._dev = {n: t.cpu() for n, t in dev.items()}
      self._ran = (fwd, bwd, self.reference())
    return self._ran

  def reference(self, wrong=()):
    prm = {n: self.net.fp.params[n] for n in OIH.HEAD}
    return OIH.head_reference(self.B, self.nq, self.host['state'], self.host['taus'], prm,
                              self.host['dq'], self._dev, wrong=wrong)

  def grad_of(self, grad, name):
    o, shape = self.net.fp.offsets[name]
    return grad[o:o + math.prod(shape)]

  def device_stages(self):
    """stage -> the device's result of it (device tensors shaped as the reference's)."""
    fwd, bwd, _ = self.ran()
    R, B = self.R, self.B
    out = {n: fwd[n][:R] for n in ('cos', 'emb', 'h', 'q')}
    out.update(dh=bwd['dh'][:R], dpre=bwd['dpre'][:R], dstate=bwd['dstate'][:B])
    if not self.fused:
      out['dtl'] = bwd['dtl'][:R]
    for stage, name in GRAD_STAGES:
      out[stage] = self.grad_of(bwd['grad'], name)
    return out
