"""The bf16 throughput build (libdopamine_amd_bf16.so: the product's sources with -DDQ_CNN_X6=1
-DDQ_X6_PAIRS=1, bench.py --full's throughput_mode row) against float64 references on
bf16-ROUNDED OPERANDS, at the project's own fp32 bar.  The build's contract:

  every GEMM that runs on the bf16 matrix instruction computes, with fp32 accumulation, the
  sum of products of its operands each rounded once to bf16 (round to nearest even);
  everything else (bias adds, ReLU masks, epilogues, exact-fp32 tiles, split-K sums) is the
  product's fp32 arithmetic.

bf16 x bf16 products are exact in fp32, so against oracle/nature_cnn.layer_reference(round_ops=)
and oracle/iqn_head.head_reference(bf16_stages=) the device must pass the same measure and
bar as the product does against the unrounded reference (cond_ratio <= LAYER_TOL = 1e-5), not
a loose "bf16 tolerance".  Which op is which (tests/bf16_build_ops.py, read off the tile
template arguments of nature_cnn.hip / iqn.hip):

  op                                              tile                        in this build
  conv1 / conv2 / conv3 / fc1 / fc2 forward       <1,1,8> <1,1,16> <1,1,9>    bf16
                                                  <1,1,16> <1,1,16>
  fc2 dX, fc1 dX, conv3 dX                        <1,1,16>                    bf16
  conv2 dX (four sub-pixel classes)               gemm_op<1,1,8,...>          bf16
  conv3 / conv2 / conv1 dW and db                 <1,1,16>                    bf16; db = Σ of the
                                                                              rounded dz (the
                                                                              ones column)
  fc2 dW|db, fc1 dW|db                            <4,4,1>                     exact fp32
  IQN emb, h (stored x and RowKHad), dW1|db1      gemm_iqn (kIqnX6)           bf16, one product
    (both forms), dWe (narrow <4,2,2>, wide)
  IQN dbe, wide dWe (128 % nq != 0)               ones column of gemm_iqn     bf16: Σ rounded dpre
  IQN dbe, narrow dWe (128 % nq == 0)             EpiDxQ partials + k_colsum  exact fp32
  IQN q, dh                                       gemm<1,1,16>                bf16
  IQN dW2|db2                                     gemm<1,4,4>                 exact fp32
  IQN dX: dpre / dtl / dstate                     kDxX6 = false               exact fp32

Per op, on the arrays the child dumped:
  (a) contract: within LAYER_TOL of the reference -- all GEMM operands rounded for a bf16 op,
      nothing rounded for an exact one;
  (b) power and classification: every bf16 op FAILS the bar against the unrounded reference
      (a build that ran the six products of the split form, or a wrong row of the table, fails
      (a) or (b));
  (c) containment: spare samples, guard words, other layers' gradients and read-only buffers
      untouched; everything written finite.
Within the build, dq_cnn_backward, dq_cnn_backward_groups(0, 7) and a second dq_cnn_backward
equal the chain of dq_cnn_backward_layer calls bit for bit, and FC1 over RowKHad equals FC1
over the stored x bit for bit (as do the backwards on them).

dopamine_amd._build reads DOPAMINE_AMD_LIB at import, so the bf16 library runs in one fresh
child process per network (tests/bf16_build_child.py), started once by a module-scoped fixture
and never retried; a nonzero status or a timeout fails every test that needs it.  A missing
bf16 library FAILS (a skip would hide a bf16 build that no longer compiles).  Measured on the
MI355X (profiles/r13_bf16_contract/): the cnn child runs 3.3 s and the iqn child 2.8 s in all
(python and HIP start-up included; 0.8 s and 0.4 s of it between the first and the last launch);
the timeout of each is 120 s, about 40 times that.  The device's worst ratio to the
rounded-operand reference is 1.6e-7 (IQN dW1), its smallest to the unrounded one 3.3e-5 (conv1
db at B = 33: 14,553 terms average the operands' rounding away; still over three times the bar,
so (b) is asserted there too).  tests/test_bf16_reference_cpu.py checks the measure's margin and power
without a GPU."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import iqn_head as OIH
from oracle import nature_cnn as ONC
from tests import bf16_build_ops as OPS
from tests.cnn_layer_case import BACKWARD, D_NAMES, FORWARD
from tests.iqn_head_case import GRAD_STAGES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CHILD = os.path.join(ROOT, 'tests', 'bf16_build_child.py')
_TIMEOUT = 120.0
_TOL = ONC.LAYER_TOL


def _child(which, tmp):
  """One run of the child on the bf16 library; its dump."""
  from dopamine_amd import _build
  assert os.path.exists(_build.BF16_LIB_PATH), (
      '%s is missing: the bf16 throughput build did not compile' % _build.BF16_LIB_PATH)
  out = str(tmp / ('%s.npz' % which))
  env = dict(os.environ, DOPAMINE_AMD_LIB=_build.BF16_LIB_PATH)
  env.pop('DQ_DIAGNOSTIC_BUILD', None)
  t0 = time.time()
  run = subprocess.run([sys.executable, _CHILD, which, out], cwd=ROOT, env=env, timeout=_TIMEOUT,
                       capture_output=True, text=True)
  print('%sthe %s child ran %.1f s in all' % (run.stdout[-2000:], which, time.time() - t0))
  assert run.returncode == 0, 'the %s child ended with status %d:\n%s' % (which, run.returncode,
                                                                         run.stderr[-4000:])
  return np.load(out, allow_pickle=False)


@pytest.fixture(scope='module')
def cnn_dump(tmp_path_factory):
  return _child('cnn', tmp_path_factory.mktemp('bf16_cnn'))


@pytest.fixture(scope='module')
def iqn_dump(tmp_path_factory):
  return _child('iqn', tmp_path_factory.mktemp('bf16_iqn'))


class _Dump(object):
  """One case's arrays of a child's dump, as torch tensors."""

  def __init__(self, npz, kind, case):
    self.case = case
    self._npz, self._pre = npz, '%s/%s/' % (kind, '-'.join(str(v) for v in case))
    self.cache = {}

  def __getitem__(self, name):
    return torch.from_numpy(self._npz[self._pre + name])

  def what(self, text):
    return '%s%s' % (self._pre, text)


def _worst(got, ref, terms):
  r = ONC.cond_ratio(got, ref, terms)
  return float(r.max()) if r.numel() else 0.0


def _hold(what, bf16, got, rounded, exact, key, act=lambda t: t):
  """Assertions (a) and (b) of one op: ``rounded`` / ``exact`` the reference dicts with and
  without bf16-rounded operands, ``key`` the result, ``act`` the ReLU a forward result passed."""
  assert bool(torch.isfinite(got).all()), '%s: not finite' % what
  shape = exact[key].shape
  got = got.reshape(shape)
  to_rounded = _worst(got, act(rounded[key]), rounded[key + '_abs'])
  to_exact = _worst(got, act(exact[key]), exact[key + '_abs'])
  print('%s [%s]: worst ratio %.3g to the %s reference, %.3g to the other' % (
      what, 'bf16' if bf16 else 'exact fp32', to_rounded if bf16 else to_exact,
      'rounded-operand' if bf16 else 'unrounded', to_exact if bf16 else to_rounded))
  assert bool((exact[key] != 0).any()), what
  failed = []                   # both halves judged, so a wrong build shows which of them it fails
  if not ((to_rounded if bf16 else to_exact) <= _TOL):
    failed.append('(a) ratio %.3g to the %s reference, over %.1g' % (
        to_rounded if bf16 else to_exact, 'rounded-operand' if bf16 else 'unrounded', _TOL))
  if bf16 and to_exact <= _TOL:
    failed.append('(b) ratio %.3g to the UNROUNDED reference is within %.1g: this is no one-product '
                  'bf16 GEMM' % (to_exact, _TOL))
  assert not failed, '%s: %s' % (what, '; '.join(failed))


# ----------------------------------------------------------------------------- Nature-CNN
@pytest.fixture(scope='module', params=OPS.CNN_CASES, ids=lambda c: 'B%d-n%d' % c)
def cnn(request, cnn_dump):
  return _Dump(cnn_dump, 'cnn', request.param)


def _layer_refs(d, layer):
  """(rounded-operand, unrounded) float64 references of one layer on the device's own input
  to it, computed once per case and layer."""
  if layer not in d.cache:
    B = d.case[0]
    _, _, src, read, _ = [b for b in BACKWARD if b[1] == layer][0]
    args = (layer, d[src][:B], d[layer + '_w'], d[layer + '_b'],
            d['dout'][:B] if read is None else d['dz_' + read])
    d.cache[layer] = (ONC.layer_reference(*args, round_ops=ONC.ROUND_OPS),
                      ONC.layer_reference(*args))
  return d.cache[layer]


def test_cnn_forward_layers_hold_the_contract(cnn):
  B = cnn.case[0]
  for layer, src, dst in FORWARD:
    rounded, exact = _layer_refs(cnn, layer)
    _hold(cnn.what('forward %s' % layer), OPS.cnn_is_bf16(layer, 'z'), cnn[dst][:B].double(), rounded,
          exact, 'z', (lambda t: t) if layer == 'fc2' else F.relu)
    ONC.assert_spare_untouched(cnn.what(dst), cnn[dst], B)
  ONC.assert_spare_untouched(cnn.what('x'), cnn['x'], B)


@pytest.mark.parametrize('index,layer,src,read,write', BACKWARD, ids=[b[1] for b in BACKWARD])
def test_cnn_backward_layer_holds_the_contract(cnn, index, layer, src, read, write):
  B = cnn.case[0]
  rounded, exact = _layer_refs(cnn, layer)
  dw, db = cnn[layer + '/dw'], cnn[layer + '/db']
  _hold(cnn.what('%s weight grad' % layer), OPS.cnn_is_bf16(layer, 'dw'), dw, rounded, exact, 'dw')
  _hold(cnn.what('%s bias grad' % layer), OPS.cnn_is_bf16(layer, 'db'), db, rounded, exact, 'db')
  if write is not None:
    assert bool((exact['dx'] != 0).any()) and bool((exact['dx'] == 0).any())   # the mask keeps and drops
    _hold(cnn.what('%s input grad' % layer), OPS.cnn_is_bf16(layer, 'dx'),
          cnn['%s/d_%s' % (layer, write)][:B], rounded, exact, 'dx')
  # nothing else was written: the two (finite) slices account for every non-NaN word of the
  # gradient buffer; the spare sample of every d buffer; whatever d buffer the layer does not write
  assert int(cnn[layer + '/grad_written']) == dw.numel() + db.numel(), cnn.what(
      '%s wrote outside its gradients' % layer)
  for name in D_NAMES:
    buf = cnn['%s/d_%s' % (layer, name)]
    ONC.assert_spare_untouched(cnn.what('%s: d %s' % (layer, name)), buf, B)
    if name == read:
      assert torch.equal(buf[:B], cnn['dz_' + name]), cnn.what('%s: d %s (read only) changed' % (layer, name))
    elif name != write:
      assert bool(torch.isnan(buf[:B]).all()), cnn.what('%s: d %s was written' % (layer, name))


def test_cnn_schedules_agree_bitwise_within_the_build(cnn):
  """gemm() and GemmOp share one cnn_x6 rule: dq_cnn_backward, dq_cnn_backward_groups(0, 7)
  and a second dq_cnn_backward equal the chain of per-layer calls word for word."""
  for name in ('chain_grad_nonfinite', 'chain_pads_written', 'chain_d_nonfinite', 'chain_spare_written',
               'whole_differs_from_chain', 'groups_differs_from_chain', 'again_differs_from_chain'):
    assert int(cnn['sched/' + name]) == 0, cnn.what('%s: %d words' % (name, int(cnn['sched/' + name])))
  guards = cnn['guards']
  assert guards.shape[1] == 64 and guards.shape[0] >= 14
  assert bool(torch.isnan(guards).all()), cnn.what('guard words were written')


# ------------------------------------------------------------------------------ IQN head
@pytest.fixture(scope='module', params=OPS.IQN_CASES, ids=lambda c: 'B%d-nq%d-A%d-E%d' % c)
def iqn(request, iqn_dump):
  assert request.param in OIH.CASES
  return _Dump(iqn_dump, 'iqn', request.param)


def test_iqn_stages_hold_the_contract(iqn):
  B, nq, A, E = iqn.case
  R, fused = B * nq, 128 % nq == 0
  bf16 = OPS.iqn_bf16_stages(nq)
  dev = {n: iqn[n][:R] for n in ('cos', 'emb', 'h', 'dh', 'dpre')}
  args = (B, nq, iqn['state'], iqn['taus'], {n: iqn[n] for n in OIH.HEAD}, iqn['dq'], dev)
  rounded = OIH.head_reference(*args, bf16_stages=bf16)
  exact = OIH.head_reference(*args)
  state = iqn['state']
  for name, t in (('state', state), ('emb', dev['emb']), ('h', dev['h'])):
    assert bool((t > 0).any()) and bool((t == 0).any()), iqn.what('%s mask' % name)
  for stage in OIH.STAGES:
    if stage == 'dtl' and fused:          # not formed: the buffer holds the dbe partials
      continue
    rows = B if stage == 'dstate' else R
    got = iqn[stage] if stage in dict(GRAD_STAGES) else iqn[stage][:rows]
    _hold(iqn.what(stage), stage in bf16, got.double(), rounded, exact, stage)
  # the stored x is the one fp32 product in every build; d state is exactly 0 behind the ReLU
  assert torch.equal(iqn['x'][:R], exact['x']), iqn.what('stored x')
  assert bool((iqn['dstate'][:B][state == 0] == 0).all()), iqn.what('d state where state == 0')


def test_iqn_forms_agree_bitwise_and_nothing_else_is_written(iqn):
  B, nq, A, E = iqn.case
  R, fused = B * nq, 128 % nq == 0
  assert torch.equal(iqn['h_rowkhad'][:R], iqn['h'][:R]), iqn.what('h over RowKHad')
  assert torch.equal(iqn['q_rowkhad'][:R], iqn['q'][:R]), iqn.what('q over RowKHad')
  for name in ('backward_forms_differ', 'inputs_changed_by_backward', 'grad_written_outside_head',
               'grad_head_nonfinite'):
    assert int(iqn[name]) == 0, iqn.what('%s: %d words' % (name, int(iqn[name])))
  for name, rows in (('cos', R), ('emb', R), ('x', R), ('h', R), ('q', R), ('h_rowkhad', R),
                     ('dh', R), ('dpre', R), ('dtl', R), ('dstate', B)):
    OIH.assert_spare_untouched(iqn.what(name), iqn[name], rows)
    if name != 'dtl':
      assert bool(torch.isfinite(iqn[name][:rows]).all()), iqn.what(name)
  tiles = (R + 127) // 128
  dtl = iqn['dtl']
  if fused:                     # only the dbe partials, one row per 128-row tile
    assert bool(torch.isfinite(dtl[:tiles]).all()) and bool(torch.isnan(dtl[tiles:]).all()), iqn.what('dtl')
  else:
    assert bool(torch.isfinite(dtl[:R]).all()), iqn.what('dtl')
  guards = iqn['guards']
  assert guards.shape == (4, 64) and bool(torch.isnan(guards).all()), iqn.what('guard words')
