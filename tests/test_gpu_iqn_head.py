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

import numpy as np
import pytest
import torch

from oracle import iqn_head as OIH
from tests.iqn_head_case import NAN as _NAN, SEED as _SEED, HeadCase as _Case

pytestmark = pytest.mark.gpu


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
