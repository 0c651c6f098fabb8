"""Every stage of the implicit-quantile head on the HIP path (dopamine_amd/csrc/iqn.hip:
dq_iqn_head_forward / dq_iqn_head_backward, dq_iqn_tau_cos, dq_uniform_draw) against a float64
reference of that stage alone (oracle/iqn_head.head_reference), the head driven on its own over
a synthetic 7744-wide state, at the (B, nq, A, E) where the code takes another path
(oracle/iqn_head.CASES): the fused b-major dX epilogue (nq | 128) with a ragged last row tile
holding one whole sample, with one sample per tile and with 128; the unfused EpiDx +
k_tile_grad; split-K last slabs of 1 to 8 rows; E = 4 and E = 68; B = 1 and B > 128; A = 1, 3
and 18.  Each stage is fed the device's own input to it, so it is judged alone and its ReLU
decision is the one the device's epilogue reads.  The measure and the bar are the north-star
test's (|got - ref| / max(Σ|terms|, COND_FLOOR max|ref|) <= 1e-5, element by element);
tests/test_iqn_head_reference_cpu.py shows fp32 CPU arithmetic passing it with 3x to spare and
subtly wrong restatements failing it.  Every R-row buffer holds R + 1 rows and the state
B + 1, NaN before each call (inputs too: a read of row R, or of state row B, poisons a result),
the workspace 64 NaN words more than dq_iqn_workspace_floats asks for, the whole flat gradient
buffer NaN before each backward."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import iqn_head as OIH

pytestmark = pytest.mark.gpu

_NAN = float('nan')
F, H = OIH.F, OIH.H
# forward forms: (emb kept, x stored)
_FORMS = {'emb': (True, False), 'emb+x': (True, True), 'x': (False, True)}
_GRAD_STAGES = (('dwe', 'emb_w'), ('dbe', 'emb_b'), ('dw1', 'fc1_w'), ('db1', 'fc1_b'),
                ('dw2', 'fc2_w'), ('db2', 'fc2_b'))
_SEED = (1 << 63) + 0xC0FFEE1234567        # the top bit set: the seed is unsigned


def _spare(rows, *shape):
  return torch.full((rows + 1,) + shape, _NAN, device='cuda')


class _Case(object):
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
    self.ws.fill_(_NAN)
    _lib.check(getattr(_lib.lib, fn)(*args), fn)
    torch.cuda.synchronize()
    OIH.assert_guard_untouched(self.what(fn + ' workspace'), self.ws, self.need)

  def _acts_struct(self, emb, x):
    from dopamine_amd import _lib
    use = dict(self.acts, emb=self.acts['emb'] if emb else None, x=self.acts['x'] if x else None)
    return _lib.IqnActs(**{k: (v.data_ptr() if v is not None else None) for k, v in use.items()})

  def forward(self, form, taus=True):
    """The forward in one of _FORMS on NaN outputs (cos too, unless it comes with the draws:
    taus False).  Returns clones of (cos, emb, x, h, q)."""
    emb, x = _FORMS[form]
    for n, t in self.acts.items():
      if n != 'cos' or taus:
        t.fill_(_NAN)
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
    self.net.fp.grad.fill_(_NAN)
    for t in list(self.grads.values()) + [self.dstate]:
      t.fill_(_NAN)
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
    for stage, name in _GRAD_STAGES:
      out[stage] = self.grad_of(bwd['grad'], name)
    return out


@pytest.fixture(scope='module', params=OIH.CASES, ids=lambda c: 'B%d-nq%d-A%d-E%d' % c)
def case(request):
  return _Case(*request.param)


def test_every_stage_matches_float64(case):
  fwd, bwd, ref = case.ran()
  B, R = case.B, case.R
  state = case.host['state']
  for name, t in (('state', state), ('emb', fwd['emb'][:R]), ('h', fwd['h'][:R])):
    assert bool((t > 0).any()) and bool((t == 0).any()), case.what('%s mask' % name)
  got = case.device_stages()
  assert set(got) == set(OIH.STAGES) - (set(('dtl',)) if case.fused else set())
  for stage in OIH.STAGES:
    if stage in got:
      OIH.assert_stage_close(case.what(), stage, got[stage], ref)
  print('%s: device cos within %.3g of float64' % (
      case.what(), float((got['cos'].cpu().double() - ref['cos']).abs().max())))
  # the stored x is the one fp32 product, and d state is exactly 0 behind the torso's ReLU
  assert torch.equal(fwd['x'][:R].cpu(), ref['x']), case.what('stored x')
  assert bool((bwd['dstate'][:B].cpu()[state == 0] == 0).all()), case.what('d state where state == 0')


def test_forward_forms_agree_bitwise(case):
  fwd, _, ref = case.ran()
  R = case.R
  for form in ('emb', 'x'):
    got = case.forward(form)
    for n in ('cos', 'h', 'q'):
      assert torch.equal(got[n][:R], fwd[n][:R]), case.what('%s of form %s' % (n, form))
    kept = 'emb' if form == 'emb' else 'x'
    assert torch.equal(got[kept][:R], fwd[kept][:R]), case.what('%s of form %s' % (kept, form))
  assert torch.equal(fwd['x'][:R].cpu(), ref['x'])


def test_taus_drawn_with_their_cosines_equal_the_separate_draw(case):
  """dq_iqn_tau_cos + forward(taus NULL) == dq_uniform_draw + forward(those taus), bitwise; the
  draws are uniform_of(seed, counter, r) bit for bit for two consecutive calls."""
  from dopamine_amd import _lib
  fwd, _, _ = case.ran()
  R, E = case.R, case.E
  keep = case.taus.clone()
  seed = ctypes.c_uint64(_SEED)
  try:
    fused_q, sep_q = [], []
    counter = torch.zeros(2, dtype=torch.int64, device='cuda')
    for call in (0, 1):
      case.taus.fill_(_NAN)
      case.acts['cos'].fill_(_NAN)
      _lib.call('dq_iqn_tau_cos', _lib.ptr(counter), seed, R, E, _lib.ptr(case.taus),
                _lib.ptr(case.acts['cos']), case.stream)
      torch.cuda.synchronize()
      assert counter.tolist() == [call + 1, 0], case.what('counter after call %d' % call)
      OIH.assert_spare_untouched(case.what('taus'), case.taus, R)
      OIH.assert_spare_untouched(case.what('cos'), case.acts['cos'], R)
      t = case.taus[:R].cpu().numpy()
      want = OIH.uniform_draws(_SEED, call, R)
      assert np.array_equal(t.view(np.uint32), want.view(np.uint32)), case.what('taus of call %d' % call)
      assert ((t >= 0) & (t < 1)).all()
      got = case.forward('emb', taus=False)
      fused_q.append((t, got['cos'][:R], got['q'][:R]))
    counter = torch.zeros(2, dtype=torch.int64, device='cuda')
    for call in (0, 1):
      case.taus.fill_(_NAN)
      _lib.call('dq_uniform_draw', _lib.ptr(counter), seed, R, _lib.ptr(case.taus), case.stream)
      torch.cuda.synchronize()
      assert counter.tolist() == [call + 1, 0]
      OIH.assert_spare_untouched(case.what('taus (dq_uniform_draw)'), case.taus, R)
      got = case.forward('emb')
      sep_q.append((case.taus[:R].cpu().numpy(), got['cos'][:R], got['q'][:R]))
    for (t0, c0, q0), (t1, c1, q1) in zip(fused_q, sep_q):
      assert np.array_equal(t0.view(np.uint32), t1.view(np.uint32))
      assert torch.equal(c0, c1) and torch.equal(q0, q1)
    assert not np.array_equal(fused_q[0][0], fused_q[1][0])   # the counter is part of the hash
    assert not torch.equal(fused_q[0][2], fwd['q'][:R])       # other taus than the case's
  finally:                      # the case's own taus and activations back, for the other tests
    case.taus.copy_(keep)
    again = case.forward('emb+x')
  for n in ('cos', 'emb', 'x', 'h', 'q'):
    assert torch.equal(again[n][:R], fwd[n][:R]), case.what(n)


def test_backward_forms_agree_bitwise_and_write_nothing_else(case):
  fwd, bwd, ref = case.ran()
  B, R = case.B, case.R
  got = case.device_stages()
  runs = [bwd]
  case.forward('emb+x')
  runs.append(case.backward(True))          # the same backward again: no atomics
  case.forward('emb')
  runs.append(case.backward(False))         # x formed by the loaders
  for i, run in enumerate(runs):
    text = ('', ' (second run)', ' (x from the loaders)')[i]
    grad = run['grad']
    # the torso's gradients and every alignment pad were left alone; every head gradient written
    assert bool(torch.isnan(grad[~case.head]).all()), case.what('wrote outside the head' + text)
    assert bool(torch.isfinite(grad[case.head]).all()), case.what('head gradient' + text)
    assert torch.equal(grad[case.head], bwd['grad'][case.head]), case.what('gradients' + text)
    for n, rows in (('dh', R), ('dpre', R), ('dstate', B)):
      OIH.assert_spare_untouched(case.what('d %s%s' % (n, text)), run[n], rows)
      assert bool(torch.isfinite(run[n][:rows]).all()), case.what(n + text)
      assert torch.equal(run[n][:rows], bwd[n][:rows]), case.what(n + text)
    OIH.assert_spare_untouched(case.what('dtl' + text), run['dtl'], R)
    tiles = (R + 127) // 128
    if case.fused:              # only the dbe partials, one row per 128-row tile
      assert bool(torch.isfinite(run['dtl'][:tiles]).all()), case.what('dbe partials' + text)
      assert bool(torch.isnan(run['dtl'][tiles:]).all()), case.what('dtl past the partials' + text)
      assert torch.equal(run['dtl'][:tiles], bwd['dtl'][:tiles])
    else:
      assert torch.equal(run['dtl'][:R], bwd['dtl'][:R]), case.what('dtl' + text)
  if case.fused:                # the partials sum to dbe (k_colsum adds them in order, in fp32)
    tiles = (R + 127) // 128
    part = bwd['dtl'][:tiles].cpu()
    acc = part[0].clone()
    for t in range(1, tiles):
      acc = acc + part[t]
    assert torch.equal(acc, got['dbe'].cpu()), case.what('dbe from its partials')
  else:
    OIH.assert_stage_close(case.what(), 'dtl', bwd['dtl'][:R], ref)


def test_wrong_reference_fails_on_the_device_result():
  """The device's (correct) result at (17, 8, 18, 64) against the reference with the state row
  taken b-major (r // nq), and with the last q left out of d state: the same assertions fail on
  the stages the mistake reaches, without touching a kernel."""
  case = _Case(17, 8, 18, 64)
  case.ran()
  got = case.device_stages()
  for wrong, failing in (('state_row_b_major', ('h', 'dpre', 'dstate', 'dw1')),
                         ('drop_last_q', ('dstate',))):
    ref = case.reference(wrong=(wrong,))
    for stage in OIH.STAGES:
      if stage not in got:
        continue
      if stage in failing:
        with pytest.raises(AssertionError, match='ratio'):
          OIH.assert_stage_close(case.what(wrong), stage, got[stage], ref)
      else:
        OIH.assert_stage_close(case.what(wrong), stage, got[stage], ref)
