"""The rounded-operand references tests/test_gpu_bf16_build.py holds the bf16 throughput build
to (oracle/nature_cnn.bf16_round, layer_reference(round_ops=), oracle/iqn_head.head_reference(
bf16_stages=)), checked here without a GPU on the inputs of that test's cases:

* bf16_round: known answers (ties to even both ways, a carry into the exponent, +-0, a
  representable value, NaN, the overflow to inf) and agreement with torch's .bfloat16() on
  random bit patterns;
* margin: the build's arithmetic emulated on the CPU (operands rounded once, then torch's fp32
  convolutions and GEMMs: exact products, fp32 accumulation) passes the unchanged bar against
  the rounded-operand reference with MARGIN to spare, for every bf16 op of every case
  (measured worst: 1.9e-7 Nature-CNN, conv2 dW at B = 33; 2.4e-7 IQN, dW1 at (27, 5, 3, 64):
  40x under 1e-5);
* power: for every bf16 op of every case, both the UNROUNDED float64 result and the emulation
  with operands truncated instead of rounded FAIL the bar against the rounded-operand
  reference (measured weakest unrounded: conv1 db at B = 33, 3.9e-5; weakest truncated: fc2
  forward at (1, 1), one 512-term row, 3.1e-5), so a device that ran an fp32-exact form, or
  rounded the wrong way, cannot pass assertion (a) -- and assertion (b) has room;
* the subtly wrong restatements still fail with rounded operands: conv2's padding flipped,
  state_row_b_major, drop_last_q;
* the options change nothing by default.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import iqn_head as OIH
from oracle import nature_cnn as ONC
from tests import bf16_build_ops as OPS
from tests.test_cnn_layer_reference_cpu import _Run as _CnnRun, _fp32_layer
from tests.test_iqn_head_reference_cpu import _Run as _IqnRun

MARGIN = 10.0
TOL = ONC.LAYER_TOL
rnd = ONC.bf16_round


def trunc(t):
  """fp32 -> the bf16 below it in magnitude -> fp32: the low 16 bits dropped."""
  return (t.detach().float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def _bits(*words):
  return torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in words],
                      dtype=torch.int32).view(torch.float32)


def _worst(got, ref, key, act=lambda t: t):
  r = ONC.cond_ratio(torch.as_tensor(got).double().reshape(ref[key].shape), act(ref[key]), ref[key + '_abs'])
  return float(r.max())


# ------------------------------------------------------------------------------ bf16_round
def test_bf16_round_known_answers():
  given = _bits(0x3F808000,      # 1 + 2^-8: a tie, the kept mantissa even -> down to 1
                0x3F818000,      # 1 + 3 * 2^-8: a tie, the kept mantissa odd -> up to 1 + 2^-6
                0x3F808001,      # just above the tie -> up
                0x3F807FFF,      # just below the tie -> down
                0x3FFF8000,      # 2 - 2^-8: the tie carries into the exponent -> 2
                0x3FFFFFFF,      # the fp32 below 2 -> 2
                0x00000000, 0x80000000,      # +0, -0
                0x3FC00000,      # 1.5: representable
                0xBF818000,      # the odd tie, negative -> away from 0, to even
                0x7F7FFFFF,      # the largest fp32 -> inf, as .bfloat16()
                0x7F800000, 0xFF800000)      # +-inf
  want = _bits(0x3F800000, 0x3F820000, 0x3F810000, 0x3F800000, 0x40000000, 0x40000000, 0x00000000,
               0x80000000, 0x3FC00000, 0xBF820000, 0x7F800000, 0x7F800000, 0xFF800000)
  got = rnd(given)
  assert got.dtype == torch.float32
  assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (got, want)
  assert torch.equal(got.view(torch.int32), given.bfloat16().float().view(torch.int32))
  nan = rnd(torch.tensor([float('nan'), 1.0]))
  assert bool(torch.isnan(nan[0])) and float(nan[1]) == 1.0
  assert rnd(torch.ones(2, 3, dtype=torch.float64)).shape == (2, 3)


def test_bf16_round_agrees_with_torch_on_random_bit_patterns():
  gen = torch.Generator().manual_seed(5)
  bits = torch.randint(-2 ** 31, 2 ** 31, (1 << 20,), generator=gen, dtype=torch.int64).to(torch.int32)
  x = bits.view(torch.float32)
  got, want = rnd(x), x.bfloat16().float()
  ok = ~torch.isnan(x)
  assert bool(ok.any()) and bool((~ok).any())
  assert torch.equal(got[ok].view(torch.int32), want[ok].view(torch.int32))
  assert bool(torch.isnan(got[~ok]).all())
  assert bool(((got.view(torch.int32) & 0xFFFF) == 0)[ok].all())      # a bf16: 16 low zero bits
  y = torch.randn(1 << 16, generator=gen)
  assert torch.equal(rnd(y), y.bfloat16().float()) and not torch.equal(rnd(y), trunc(y))


# ------------------------------------------------------------------------------ Nature-CNN
@pytest.fixture(scope='module', params=OPS.CNN_CASES, ids=lambda c: 'B%d-n%d' % c)
def cnn(request):
  run = _CnnRun(*request.param)
  prm = run.net.fp.params
  run.args = {layer: (layer, run.inputs[layer], prm[layer + '_w'], prm[layer + '_b'], run.dz[layer])
              for layer in ONC.LAYERS}
  run.rounded = {layer: ONC.layer_reference(*a, round_ops=ONC.ROUND_OPS) for layer, a in run.args.items()}
  return run


def _emulated(args, how):
  layer, x, w, b, dz = args
  return _fp32_layer(layer, how(x), how(w), b, how(dz))


def _act(layer, key):
  return F.relu if key == 'z' and layer != 'fc2' else (lambda t: t)


def test_cnn_options_change_nothing_by_default(cnn):
  for layer in ('conv2', 'fc2'):
    plain, none = ONC.layer_reference(*cnn.args[layer]), ONC.layer_reference(*cnn.args[layer], round_ops=())
    assert all(torch.equal(plain[k], none[k]) for k in plain)
    assert not torch.equal(plain['z'], cnn.rounded[layer]['z'])
    # the ReLU decision is the unrounded input's; the bias is not rounded (a zero input
    # leaves it alone, and it is no bf16)
    _, x, w, b, dz = cnn.args[layer]
    assert bool((x <= 0).any()) and bool((cnn.rounded[layer]['dx'].reshape(x.shape)[x <= 0] == 0).all())
    z0 = ONC.layer_reference(layer, torch.zeros_like(x), w, b, dz, round_ops=ONC.ROUND_OPS)['z']
    assert torch.equal(z0.reshape(-1, b.numel()), b.detach().double().expand(z0.numel() // b.numel(), -1))
    assert not torch.equal(rnd(b), b.detach())


def test_cnn_emulated_build_passes_with_margin(cnn):
  for layer in ONC.LAYERS:
    got, ref = _emulated(cnn.args[layer], rnd), cnn.rounded[layer]
    for key, part in OPS.PARTS:
      if not OPS.cnn_is_bf16(layer, key):
        continue
      worst = _worst(_act(layer, key)(got[key]), ref, key, _act(layer, key))
      print('%s %s B=%d n_out=%d (rounded operands, fp32 CPU): worst ratio %.3g' % (
          layer, part, cnn.B, cnn.n_out, worst))
      assert worst * MARGIN <= TOL, (layer, part, worst)
      assert bool((ref[key] != 0).any())


def test_cnn_unrounded_and_truncated_results_fail(cnn):
  for layer in ONC.LAYERS:
    ref = cnn.rounded[layer]
    exact, cut = ONC.layer_reference(*cnn.args[layer]), _emulated(cnn.args[layer], trunc)
    for key, part in OPS.PARTS:
      if not OPS.cnn_is_bf16(layer, key):
        continue
      act = _act(layer, key)
      fp32, tr = _worst(act(exact[key]), ref, key, act), _worst(act(cut[key]), ref, key, act)
      print('%s %s B=%d n_out=%d: unrounded operands %.3g, truncated operands %.3g' % (
          layer, part, cnn.B, cnn.n_out, fp32, tr))
      # assertion (b) of the GPU test needs room on the real generator: three times the bar
      assert fp32 > 3 * TOL, (layer, part, fp32)
      assert tr > TOL, (layer, part, tr)


def test_flipped_conv2_padding_fails_with_rounded_operands():
  run = _CnnRun(5, 129)
  prm = run.net.fp.params
  args = ('conv2', run.inputs['conv2'], prm['conv2_w'], prm['conv2_b'], run.dz['conv2'])
  got = _emulated(args, rnd)
  ref = ONC.layer_reference(*args, pad=(2, 1, 2, 1), round_ops=ONC.ROUND_OPS)
  for key in ('z', 'dx', 'dw'):
    with pytest.raises(AssertionError, match='ratio'):
      ONC.assert_layer_close('conv2 %s, padding flipped' % key, _act('conv2', key)(got[key]).reshape(ref[key].shape),
                             _act('conv2', key)(ref[key]), ref[key + '_abs'])
  ONC.assert_layer_close('conv2 db, padding flipped', got['db'], ref['db'], ref['db_abs'])


# -------------------------------------------------------------------------------- IQN head
def _emulated_head(run, dev, how):
  """The bf16 stages of the head in fp32 CPU arithmetic on operands rounded by ``how``, each
  on the fp32 head's own input to it (dev)."""
  B, nq = run.shape[:2]
  We, be, W1, b1, W2, b2 = [run.prm[n].detach().float() for n in OIH.HEAD]
  x = run.state.float()[OIH.state_rows(B, nq)] * dev['emb']      # fp32 first, then rounded
  cos, h, dh, dpre, dq = dev['cos'], dev['h'], dev['dh'], dev['dpre'], run.dq.float()
  return dict(emb=torch.relu(how(cos) @ how(We).T + be), h=torch.relu(how(x) @ how(W1).T + b1),
              q=how(h) @ how(W2).T + b2, dh=(how(dq) @ how(W2)) * (h > 0).float(),
              dw1=how(dh).T @ how(x), db1=how(dh).sum(0), dwe=how(dpre).T @ how(cos),
              dbe=how(dpre).sum(0))


@pytest.fixture(scope='module', params=OPS.IQN_CASES, ids=lambda c: 'B%d-nq%d-A%d-E%d' % c)
def iqn(request):
  assert request.param in OIH.CASES
  run = _IqnRun(*request.param)
  B, nq = run.shape[:2]
  run.dev, run.exact = run.both()
  run.bf16 = OPS.iqn_bf16_stages(nq)
  run.rounded = OIH.head_reference(B, nq, run.state, run.taus, run.prm, run.dq, run.dev,
                                   bf16_stages=run.bf16)
  return run


def test_iqn_options_change_nothing_by_default(iqn):
  for stage in OIH.STAGES:
    same = torch.equal(iqn.exact[stage], iqn.rounded[stage])
    assert same == (stage not in iqn.bf16), stage
  assert torch.equal(iqn.exact['x'], iqn.rounded['x'])
  assert set(iqn.bf16) <= set(OIH.GEMM_STAGES)
  assert ('dbe' in iqn.bf16) == (128 % iqn.shape[1] != 0)


def test_iqn_emulated_build_passes_with_margin(iqn):
  got = _emulated_head(iqn, iqn.dev, rnd)
  for stage in iqn.bf16:
    worst = OIH.assert_stage_close(iqn.what(' (rounded operands, fp32 CPU)'), stage, got[stage], iqn.rounded)
    assert worst * MARGIN <= TOL, (stage, worst)
    assert bool((iqn.rounded[stage] != 0).any())


def test_iqn_unrounded_and_truncated_results_fail(iqn):
  cut = _emulated_head(iqn, iqn.dev, trunc)
  for stage in iqn.bf16:
    key = stage
    fp32, tr = _worst(iqn.exact[key], iqn.rounded, key), _worst(cut[key], iqn.rounded, key)
    print('%s %s: unrounded operands %.3g, truncated operands %.3g' % (iqn.what(), stage, fp32, tr))
    assert fp32 > 3 * TOL, (stage, fp32)
    assert tr > TOL, (stage, tr)


@pytest.mark.parametrize('wrong,failing', (('state_row_b_major', ('h', 'dpre', 'dstate', 'dw1')),
                                           ('drop_last_q', ('dstate',))))
def test_wrong_head_references_fail_with_rounded_operands(wrong, failing):
  run = _IqnRun(17, 8, 18, 64)
  B, nq = run.shape[:2]
  dev, _ = run.both()
  bf16 = OPS.iqn_bf16_stages(nq)
  emulated = _emulated_head(run, dev, rnd)
  got = dict(dev, **{stage: emulated[stage] for stage in bf16})   # the other stages in plain fp32
  ref = OIH.head_reference(B, nq, run.state, run.taus, run.prm, run.dq, dev, wrong=(wrong,), bf16_stages=bf16)
  for stage in OIH.STAGES:
    if stage in failing:
      with pytest.raises(AssertionError, match='ratio'):
        OIH.assert_stage_close(run.what(' ref %s:' % wrong), stage, got[stage], ref)
    else:
      OIH.assert_stage_close(run.what(' ref %s:' % wrong), stage, got[stage], ref)
