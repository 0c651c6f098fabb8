"""The stage-by-stage float64 reference of the implicit-quantile head (oracle/iqn_head.py
head_reference) and the measure tests/test_gpu_iqn_head.py holds every stage of the device to
(oracle/nature_cnn.py cond_ratio / assert_layer_close), checked here without a GPU:

* calibration: torch's own fp32 CPU arithmetic of every stage (the d state sum over q taken
  sequentially in q, as the device takes it) passes the measure with at least 3x to spare at
  every (B, nq, A, E) of the GPU test -- the reference and its Σ|terms| alone stay inside it;
* sensitivity: the same assertions fail on a subtly wrong restatement (made here in fp32): the
  state row taken b-major, cosine features from k instead of k + 1, the last q left out of
  d state, the d pre mask as emb >= 0, the last row of a ragged 128-row tile left out of dbe, a
  dropped K tail of the embedding at E = 68, d state without its state > 0 mask -- and only on
  the stages the mistake reaches;
* every ReLU mask (emb > 0, h > 0, state > 0) keeps some and drops some in every case;
* uniform_of, the Python restatement of the device's tau generator.
"""
import numpy as np
import pytest
import torch

from oracle import iqn_head as OIH

MARGIN = 3.0
CASES, F, make_inputs = OIH.CASES, OIH.F, OIH.make_inputs


def _fp32_head(B, nq, state, taus, prm, dq, wrong=()):
  """The head in torch fp32 CPU arithmetic, each stage on the fp32 result before it (as the
  device chains them).  wrong: the deliberately wrong restatements of this file."""
  R, E = B * nq, prm['emb_w'].shape[1]
  state, taus, dq = state.float(), taus.float(), dq.float()
  We, be, W1, b1, W2, b2 = [prm[n].detach().float() for n in OIH.HEAD]
  k = torch.arange(0 if 'cos_from_k' in wrong else 1, E + (0 if 'cos_from_k' in wrong else 1),
                   dtype=torch.float32)
  o = {}
  o['cos'] = cos = torch.cos(taus.reshape(-1, 1) * (k * torch.tensor(np.pi, dtype=torch.float32)))
  kk = 64 if 'emb_k_tail' in wrong else E                    # the third 32-slice holds k = 64 .. 67
  o['emb'] = emb = torch.relu(cos[:, :kk] @ We[:, :kk].T + be)
  r = torch.arange(R)
  rows = r // nq if 'state_row_b_major' in wrong else r % B
  o['x'] = x = state[rows] * emb
  o['h'] = h = torch.relu(x @ W1.T + b1)
  o['q'] = h @ W2.T + b2
  o['dh'] = dh = (dq @ W2) * (h > 0).float()
  o['dw2'], o['db2'] = dq.T @ h, dq.sum(0)
  dx = dh @ W1
  emask = (emb >= 0) if 'dpre_mask_ge' in wrong else (emb > 0)
  zero = torch.zeros(())
  o['dpre'] = dpre = torch.where(emask, dx * state[rows], zero)
  o['dtl'] = dtl = dx * emb
  acc = torch.zeros(B, F)
  for q in range(nq - 1 if 'drop_last_q' in wrong else nq):   # sequentially in q
    acc = acc + (dtl.reshape(B, nq, F)[:, q] if 'state_row_b_major' in wrong else
                 dtl[q * B:(q + 1) * B])
  o['dstate'] = acc if 'no_state_mask' in wrong else torch.where(state > 0, acc, zero)
  o['dw1'], o['db1'] = dh.T @ x, dh.sum(0)
  o['dwe'] = dpre.T @ cos
  o['dbe'] = (dpre[:R - 1] if 'dbe_drop_last_row' in wrong else dpre).sum(0)
  return o


class _Run(object):
  def __init__(self, B, nq, A, E):
    self.shape = (B, nq, A, E)
    self.net, self.state, self.taus, self.dq = make_inputs(B, nq, A, E)
    self.prm = {n: self.net.fp.params[n] for n in OIH.HEAD}

  def both(self, wrong=()):
    """(the fp32 restatement, the float64 reference on that restatement's own intermediates)."""
    B, nq = self.shape[:2]
    got = _fp32_head(B, nq, self.state, self.taus, self.prm, self.dq, wrong)
    ref = OIH.head_reference(B, nq, self.state, self.taus, self.prm, self.dq, got)
    return got, ref

  def what(self, text=''):
    return 'B=%d nq=%d A=%d E=%d%s' % (self.shape + (text,))


@pytest.fixture(scope='module', params=CASES, ids=lambda c: 'B%d-nq%d-A%d-E%d' % c)
def run(request):
  return _Run(*request.param)


def test_the_bar_is_the_projects():
  assert OIH.COND_FLOOR == 1e-3 and OIH.LAYER_TOL == 1e-5    # tests/test_gpu_northstar.py


def test_fp32_cpu_arithmetic_passes_with_margin(run):
  got, ref = run.both()
  assert torch.equal(got['x'], ref['x'])                      # the one-rounding fp32 product
  for stage in OIH.STAGES:
    what = run.what(' (fp32 CPU)')
    worst = OIH.assert_stage_close(what, stage, got[stage], ref)
    assert worst * MARGIN <= OIH.LAYER_TOL, '%s %s: %.3g is not %gx under %g' % (
        what, stage, worst, MARGIN, OIH.LAYER_TOL)
    assert bool((ref[stage] != 0).any()), (what, stage)       # not trivially zero
  print('%s: fp32 cos within %.3g of float64' % (run.what(), float((got['cos'].double() -
                                                                   ref['cos']).abs().max())))


def test_every_mask_keeps_and_drops(run):
  got, ref = run.both()
  for name, t in (('state', run.state), ('emb', got['emb']), ('h', got['h'])):
    assert bool((t > 0).any()) and bool((t == 0).any()), run.what(' ' + name)
  assert bool((run.state >= 0).all())                         # exact zeros, nothing below
  zero = run.state == 0
  assert bool((ref['dstate'][zero] == 0).all()) and bool((ref['dstate_abs'][zero] == 0).all())
  assert bool((ref['dpre'][got['emb'] == 0] == 0).all())
  assert bool((ref['dh'][got['h'] == 0] == 0).all())


# wrong restatement -> (the case it is made at, the stages whose assertion must fail); every
# other stage must still pass: it is judged on the restatement's own input to it
_WRONG = {
    'state_row_b_major': ((17, 8, 18, 64), ('h', 'dpre', 'dstate', 'dw1')),
    'cos_from_k': ((3, 4, 4, 4), ('cos',)),
    'drop_last_q': ((27, 5, 3, 64), ('dstate',)),
    'dpre_mask_ge': ((2, 128, 4, 64), ('dpre',)),
    'dbe_drop_last_row': ((17, 8, 18, 64), ('dbe',)),        # R = 136: row 135, tile 2's 8th
    'emb_k_tail': ((11, 3, 4, 68), ('emb',)),
    'no_state_mask': ((130, 1, 2, 64), ('dstate',)),
}


@pytest.mark.parametrize('wrong', sorted(_WRONG))
def test_wrong_restatement_fails(wrong):
  shape, failing = _WRONG[wrong]
  assert shape in CASES
  run = _Run(*shape)
  got, ref = run.both(wrong=(wrong,))
  if wrong == 'state_row_b_major':
    assert not torch.equal(got['x'], ref['x'])
  for stage in OIH.STAGES:
    what = run.what(' %s:' % wrong)
    if stage in failing:
      with pytest.raises(AssertionError, match='ratio'):
        OIH.assert_stage_close(what, stage, got[stage], ref)
    else:
      OIH.assert_stage_close(what, stage, got[stage], ref)


@pytest.mark.parametrize('wrong', OIH.WRONG)
def test_wrong_reference_fails_on_a_correct_result(wrong):
  """The reference's own wrong restatements (the GPU test holds the device's result to them):
  the correct fp32 head fails on the stages they reach, and passes on the others."""
  run = _Run(17, 8, 18, 64)
  B, nq = run.shape[:2]
  got, _ = run.both()
  ref = OIH.head_reference(B, nq, run.state, run.taus, run.prm, run.dq, got, wrong=(wrong,))
  failing = {'state_row_b_major': ('h', 'dpre', 'dstate', 'dw1'), 'drop_last_q': ('dstate',)}[wrong]
  for stage in OIH.STAGES:
    if stage in failing:
      with pytest.raises(AssertionError, match='ratio'):
        OIH.assert_stage_close(run.what(' ref %s:' % wrong), stage, got[stage], ref)
    else:
      OIH.assert_stage_close(run.what(' ref %s:' % wrong), stage, got[stage], ref)


def test_uniform_of_is_splitmix64_in_wraparound_arithmetic():
  """The Python-integer restatement against numpy uint64 arithmetic (which wraps), seeds with
  the top bit set included; k * 2^-24 with k a 24-bit integer."""
  for seed in (0, 7, 0xC0FFEE1234567, (1 << 64) - 3, 0x9E3779B97F4A7C15):
    for call in (0, 1, 12345):
      i = np.arange(300, dtype=np.uint64)
      with np.errstate(over='ignore'):
        z = (np.uint64(seed) + np.uint64(call) * np.uint64(0x9E3779B97F4A7C15) +
             (i + np.uint64(1)) * np.uint64(0xD1B54A32D192ED03))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
      want = (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
      got = OIH.uniform_draws(seed, call, 300)
      assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
      assert ((got >= 0) & (got < 1)).all()
      k = got.astype(np.float64) * 2.0 ** 24
      assert np.array_equal(k, np.floor(k)) and k.max() < 2 ** 24
  assert not np.array_equal(OIH.uniform_draws(7, 0, 64), OIH.uniform_draws(7, 1, 64))
