"""The loss and optimizer kernels (dopamine_amd/csrc/learner.hip, c51_dev.h) against float64
at their edges: k_c51, k_c51_online, c51_target_block, k_dqn, k_dqn_fused, k_iqn, k_wmean /
k_mean, k_adam* and k_rmsprop.

Every loss output is compared with the float64 oracle (oracle/learner.py) relative to the sum
of the absolute terms its arithmetic adds -- oracle/nature_cnn.py cond_ratio /
assert_layer_close at the project's bar (COND_FLOOR 1e-3, LAYER_TOL 1e-5); the cases are
oracle/learner_cases.py's, whose conditions (greedy margins, where the smallest probability
sits, exact ties) tests/test_learner_reference_cpu.py asserts on the CPU together with the
measure's margin and its power against subtly wrong kernels.  Output buffers are NaN-filled
and carry one spare sample (or 64 guard floats) that must stay NaN; every output must be
finite.  The fused kernels run through the C ABI on synthetic slabs and must be bitwise the
unfused kernel on the logits those slabs sum to.
"""
import numpy as np
import pytest
import torch

from oracle import learner as L
from oracle import learner_cases as C
from oracle import nature_cnn as ONC

pytestmark = pytest.mark.gpu
NAN = float('nan')
f32 = torch.float32


def _t(x, dt=None):
  t = torch.as_tensor(np.ascontiguousarray(x))
  return t.to('cuda', dt if dt is not None else t.dtype)


def _nan(*shape):
  return torch.full(shape, NAN, dtype=f32, device='cuda')


def _dev(c, *names):
  dts = dict(act=torch.int32, term=torch.uint8)
  return [_t(c[n], dts.get(n)) for n in names]


def _loss_bufs(B, grad_shape, mean=True):
  """NaN buffers with one spare sample; the mean (one float) is followed by 64 guard floats."""
  bufs = dict(grad=_nan(B + 1, *grad_shape), loss=_nan(B + 1), priorities=_nan(B + 1))
  if mean:
    bufs['mean_loss'] = _nan(1 + 64)
  return bufs


def _views(bufs, B):
  return {k: (v[:1] if k == 'mean_loss' else v[:B]) for k, v in bufs.items()}


def _untouched(what, bufs, B):
  torch.cuda.synchronize()
  for k, v in bufs.items():
    if k == 'mean_loss':
      ONC.assert_guard_untouched('%s %s' % (what, k), v, 1)
    else:
      ONC.assert_spare_untouched('%s %s' % (what, k), v, B)


def _check(what, bufs, B, checks):
  """Every output in ``checks`` finite and within the bar of its float64 reference on its
  Σ|terms|; the spare sample / guard floats of every buffer still NaN."""
  _untouched(what, bufs, B)
  got = _views(bufs, B)
  for k, (ref, terms) in checks.items():
    ref = np.asarray(ref, np.float64)
    ONC.assert_layer_close('%s %s' % (what, k), got[k].reshape(ref.shape), ref,
                           np.asarray(terms, np.float64))


# =========================================================================== dq_c51_loss
def _run_c51(c, probs):
  from dopamine_amd import ops
  B, A, N = c['B'], c['A'], c['N']
  bufs = _loss_bufs(B, (A, N))
  ol, tl, act, rew, term, z = _dev(c, 'ol', 'tl', 'act', 'rew', 'term', 'z')
  ops.c51_loss(ol, tl, act, rew, term, z, c['cg'], _t(c['probs']) if probs else None,
               out=_views(bufs, B))
  return bufs


@pytest.mark.parametrize('probs', [True, False], ids=['per', 'uniform'])
@pytest.mark.parametrize('scale', C.SCALES)
@pytest.mark.parametrize('B,A,N', C.C51_SHAPES)
def test_c51_loss_against_float64(B, A, N, scale, probs):
  c = C.c51_case(B, A, N, scale)
  ref = C.c51_reference(c, probs)
  _check('c51 B=%d A=%d N=%d x%d %s' % (B, A, N, scale, 'per' if probs else 'uniform'),
         _run_c51(c, probs), B, C.c51_checks(ref))


@pytest.mark.parametrize('name', ['gamma0', 'all-terminal', 'B513'])
def test_c51_loss_cold_branches(name):
  """cumulative_gamma = 0 and an all-terminal batch (the whole-run branch of the projection
  for every sample), and B = 513 with the smallest probability at index 512."""
  c = {'gamma0': lambda: C.c51_case(5, 3, 51, 2, cg=0.0),
       'all-terminal': lambda: C.c51_case(7, 2, 5, 2, all_terminal=True),
       'B513': C.c51_online_case}[name]()
  _check('c51 %s' % name, _run_c51(c, True), c['B'], C.c51_checks(C.c51_reference(c, True)))


def test_c51_greedy_tie_takes_the_first_max():
  """Three target rows with Q exactly 0 each and different projections, in four orders: the
  projection 1/N - B grad / w (zero online logits) is the first row's, and far from the
  others'."""
  c = C.c51_tie_case()
  B, A, N = c['B'], c['A'], c['N']
  ref = C.c51_reference(c, False)
  bufs = _run_c51(c, False)
  _check('c51 tie', bufs, B, C.c51_checks(ref))
  grad = bufs['grad'][:B].cpu().numpy().astype(np.float64)
  proj = 1.0 / N - B * grad[np.arange(B), c['act']]
  terms = ref['proj_abs'] + 1.0 / N
  ONC.assert_layer_close('c51 tie projection', proj, ref['proj'], terms)
  for a in range(1, A):
    other = C.c51_reference(dict(c, tl=c['tl'][:, [a] * A]), False)['proj']
    r = ONC.cond_ratio(proj, other, terms).reshape(B, N).max(1).values
    assert float(r.min()) > 100 * ONC.LAYER_TOL, (a, r)


# =========================================================== fused kernels on synthetic slabs
def _fused_args(c, probs, w2):
  d = dict(po=_t(c['po']), bo=_t(c['bo']), pt=_t(c['pt']), bt=_t(c['bt']))
  d['act'], d['rew'], d['term'] = _dev(c, 'act', 'rew', 'term')
  d['z'] = _t(c['z']) if 'z' in c else None
  d['probs'] = _t(c['probs']) if probs else None
  d['w2'] = _t(c['w2']) if w2 else None
  d['h'] = _t(c['h']) if w2 else None
  return d


def _call_c51_fused(c, d, bufs, dh, ol_out, tl_out, hidden=None, w2=None):
  from dopamine_amd import _lib
  p = _lib.ptr
  B, A, N = c['B'], c['A'], c['N']
  _lib.call('dq_c51_loss_fused', p(d['po']), p(d['bo']), p(d['pt']), p(d['bt']), c['n_parts'],
            p(d['act']), p(d['rew']), p(d['term']), p(d['probs']), p(d['z']), B, A, N,
            float(c['cg']), p(bufs['grad']), p(bufs['loss']), p(bufs['priorities']),
            p(d['w2']) if w2 is None else w2, p(d['h']), p(dh),
            c['hidden'] if hidden is None else hidden, p(ol_out), p(tl_out),
            _lib.stream_of(d['po'].device))


def _call_c51_online(c, d, m, bufs, dh, ol_out, hidden=None, w2=None):
  from dopamine_amd import _lib
  p = _lib.ptr
  B, A, N = c['B'], c['A'], c['N']
  _lib.call('dq_c51_loss_online', p(d['po']), p(d['bo']), c['n_parts'], p(m), p(d['act']),
            p(d['probs']), B, A, N, p(bufs['grad']), p(bufs['loss']), p(bufs['priorities']),
            p(d['w2']) if w2 is None else w2, p(d['h']), p(dh),
            c['hidden'] if hidden is None else hidden, p(ol_out), _lib.stream_of(d['po'].device))


def _check_dh(what, dh, grad, c):
  ref, terms = C.dh_reference(grad.cpu().numpy(), c['w2'], c['h'], c['act'])
  ONC.assert_spare_untouched(what, dh, c['B'])
  ONC.assert_layer_close(what, dh[:c['B']], ref, terms)
  assert bool((dh[:c['B']][_t(c['h']) <= 0] == 0).all()), what


@pytest.mark.parametrize('row', C.FUSED_ROWS, ids=lambda r: 'B%d-A%d-N%d-p%d-H%d' % r[:5])
def test_c51_fused_and_online_on_synthetic_slabs(row):
  """dq_c51_loss_fused: bitwise dq_c51_loss on the logits the slabs sum to (gradient, loss,
  priorities, logits written out); d h against float64 on the device's own gradient.
  dq_c51_loss_online given the float64 projection rounded to fp32: against the float64
  cross-entropy on that m."""
  from dopamine_amd import ops
  B, A, N, n_parts, hidden, probs, logits_out, w2 = row
  c = C.fused_case(B, A, N, n_parts, hidden)
  what = 'fused B=%d A=%d N=%d parts=%d H=%d' % row[:5]
  d = _fused_args(c, probs, w2)
  ol, tl = _t(c['ol']), _t(c['tl'])
  plain = _loss_bufs(B, (A, N), mean=False)
  v = _views(plain, B)
  v['mean_loss'] = _nan(1)
  ops.c51_loss(ol, tl, d['act'], d['rew'], d['term'], d['z'], c['cg'], d['probs'], out=v)
  ref = C.c51_reference(c, probs)
  checks = C.c51_checks(ref)
  checks.pop('mean_loss')
  _check(what + ' (unfused)', plain, B, checks)
  # fused
  bufs = _loss_bufs(B, (A, N), mean=False)
  dh = _nan(B + 1, hidden)
  ol_out = _nan(B + 1, A, N) if logits_out else None
  tl_out = _nan(B + 1, A, N) if logits_out else None
  _call_c51_fused(c, d, bufs, dh, ol_out, tl_out)
  _untouched(what, bufs, B)
  for k in ('grad', 'loss', 'priorities'):
    assert torch.equal(bufs[k][:B], plain[k][:B]), '%s %s: not bitwise the unfused kernel' % (what, k)
  if logits_out:
    for name, out, want in (('online', ol_out, ol), ('target', tl_out, tl)):
      ONC.assert_spare_untouched('%s %s logits' % (what, name), out, B)
      assert torch.equal(out[:B], want), '%s: %s logits' % (what, name)
  if w2:
    _check_dh(what + ' dh', dh, bufs['grad'][:B], c)
  else:
    assert bool(torch.isnan(dh).all()), what
  # online, on the float64 projection rounded to fp32
  m = _nan(B + 1, N)
  m[:B] = _t(ref['proj'].astype(np.float32))
  cref = L.c51_cross_entropy(c['ol'], m[:B].cpu().numpy(), c['act'], c['probs'] if probs else None)
  cchecks = C.c51_checks(cref)
  cchecks.pop('mean_loss')
  obufs = _loss_bufs(B, (A, N), mean=False)
  odh = _nan(B + 1, hidden)
  ool = _nan(B + 1, A, N) if logits_out else None
  _call_c51_online(c, d, m, obufs, odh, ool)
  _check(what + ' (online)', obufs, B, cchecks)
  if logits_out:
    ONC.assert_spare_untouched(what + ' online logits', ool, B)
    assert torch.equal(ool[:B], ol), what
  if w2:
    _check_dh(what + ' online dh', odh, obufs['grad'][:B], c)
  else:
    assert bool(torch.isnan(odh).all()), what


@pytest.mark.parametrize('row', C.EXACT_ROWS, ids=lambda r: 'B%d-A%d-N%d-p%d-H%d' % r)
def test_c51_online_is_bitwise_fused_on_exact_targets(row):
  """One-hot target rows, dyadic rewards, gamma and support: the projection is exact, so the
  float64 projection rounded to fp32 is bit for bit what dq_c51_loss_fused forms inside, and
  dq_c51_loss_online on it must give bitwise its gradient, loss, priorities and d h."""
  B, A, N, n_parts, hidden = row
  c = C.fused_case(B, A, N, n_parts, hidden, exact_target=True)
  what = 'exact B=%d A=%d N=%d parts=%d H=%d' % row
  ref = C.c51_reference(c, True)
  assert np.array_equal(C.c51_reference(c, True, dtype=np.float32)['proj'],
                        ref['proj'].astype(np.float32))
  d = _fused_args(c, True, True)
  bufs, obufs = _loss_bufs(B, (A, N), mean=False), _loss_bufs(B, (A, N), mean=False)
  dh, odh = _nan(B + 1, hidden), _nan(B + 1, hidden)
  m = _nan(B + 1, N)
  m[:B] = _t(ref['proj'].astype(np.float32))
  _call_c51_fused(c, d, bufs, dh, None, None)
  _call_c51_online(c, d, m, obufs, odh, None)
  checks = C.c51_checks(ref)
  checks.pop('mean_loss')
  _check(what, bufs, B, checks)
  _untouched(what + ' online', obufs, B)
  for k in ('grad', 'loss', 'priorities'):
    assert torch.equal(bufs[k][:B], obufs[k][:B]), '%s %s' % (what, k)
  _check_dh(what + ' dh', dh, bufs['grad'][:B], c)
  ONC.assert_spare_untouched(what + ' online dh', odh, B)
  assert torch.equal(dh[:B], odh[:B]), what


@pytest.mark.parametrize('hidden', [6, 10])
def test_c51_fused_and_online_refuse_a_hidden_that_is_no_multiple_of_4(hidden):
  """The W2 rows reach LDS in 16-byte chunks: refused with the header's argument error before
  anything is launched -- and so is an fc2_w, h or dh that is not 16-byte aligned."""
  from dopamine_amd import _lib
  B, A, N = 3, 2, 5
  c = C.fused_case(B, A, N, 3, hidden)
  d = _fused_args(c, True, True)
  m = _t(C.c51_reference(c, True)['proj'].astype(np.float32))
  for call in ('fused', 'online'):
    bufs = _loss_bufs(B, (A, N), mean=False)
    dh = _nan(B + 1, hidden)
    with pytest.raises(_lib.DQError, match='multiple of 4'):
      if call == 'fused':
        _call_c51_fused(c, d, bufs, dh, None, None)
      else:
        _call_c51_online(c, d, m, bufs, dh, None)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(v).all()) for v in list(bufs.values()) + [dh]), call
  # hidden = 8 is fine, a pointer 4 bytes off is not
  c = C.fused_case(B, A, N, 3, 8)
  d = _fused_args(c, True, True)
  for call in ('fused', 'online'):
    bufs = _loss_bufs(B, (A, N), mean=False)
    dh = _nan(B + 1, 8)
    with pytest.raises(_lib.DQError, match='16-byte aligned'):
      if call == 'fused':
        _call_c51_fused(c, d, bufs, dh, None, None, w2=d['w2'].data_ptr() + 4)
      else:
        _call_c51_online(c, d, m, bufs, dh, None, w2=d['w2'].data_ptr() + 4)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(v).all()) for v in list(bufs.values()) + [dh]), call


# ------------------------------------------------------------------------------ DQN fused
def _call_dqn_fused(c, d, grad, loss, dh, oq_out, tq_out, A=None, hidden=None):
  from dopamine_amd import _lib
  p = _lib.ptr
  _lib.call('dq_dqn_huber_loss_fused', p(d['po']), p(d['bo']), p(d['pt']), p(d['bt']),
            c['n_parts'], p(d['act']), p(d['rew']), p(d['term']), c['B'],
            c['A'] if A is None else A, float(c['cg']), p(grad), p(loss), p(d['w2']), p(d['h']),
            p(dh), c['hidden'] if hidden is None else hidden, p(oq_out), p(tq_out),
            _lib.stream_of(grad.device))


@pytest.mark.parametrize('B,A,n_parts,hidden', C.DQN_FUSED_ROWS)
def test_dqn_fused_on_synthetic_slabs(B, A, n_parts, hidden):
  from dopamine_amd import ops
  c = C.dqn_fused_case(B, A, n_parts, hidden)
  what = 'dqn fused B=%d A=%d parts=%d H=%d' % (B, A, n_parts, hidden)
  d = _fused_args(c, False, True)
  oq, tq = _t(c['oq']), _t(c['tq'])
  plain = dict(grad=_nan(B + 1, A), loss=_nan(B + 1), mean_loss=_nan(1 + 64))
  ops.dqn_huber_loss(oq, tq, d['act'], d['rew'], d['term'], c['cg'], out=_views(plain, B))
  _check(what + ' (unfused)', plain, B, C.dqn_checks(C.dqn_reference(c)))
  grad, loss, dh = _nan(B + 1, A), _nan(B + 1), _nan(B + 1, hidden)
  oq_out, tq_out = _nan(B + 1, A), _nan(B + 1, A)
  _call_dqn_fused(c, d, grad, loss, dh, oq_out, tq_out)
  torch.cuda.synchronize()
  for name, buf, want in (('grad', grad, plain['grad'][:B]), ('loss', loss, plain['loss'][:B]),
                          ('Q', oq_out, oq), ("Q'", tq_out, tq)):
    ONC.assert_spare_untouched('%s %s' % (what, name), buf, B)
    assert torch.equal(buf[:B], want), '%s %s: not bitwise the unfused kernel' % (what, name)
  g = grad[:B].cpu().numpy().astype(np.float64)[np.arange(B), c['act']][:, None]
  w = c['w2'].astype(np.float64)[c['act']]
  keep = c['h'] > 0
  ONC.assert_spare_untouched(what + ' dh', dh, B)
  ONC.assert_layer_close(what + ' dh', dh[:B], g * w * keep, np.abs(g) * np.abs(w) * keep)


@pytest.mark.parametrize('A,hidden,msg', [(65, 512, 'num_actions'), (4, 516, 'multiple of 4'),
                                          (4, 6, 'multiple of 4')])
def test_dqn_fused_refusals(A, hidden, msg):
  from dopamine_amd import _lib
  c = C.dqn_fused_case(3, A, 3, hidden)
  d = _fused_args(c, False, True)
  outs = [_nan(4, A), _nan(4), _nan(4, hidden), _nan(4, A), _nan(4, A)]
  with pytest.raises(_lib.DQError, match=msg):
    _call_dqn_fused(c, d, *outs)
  torch.cuda.synchronize()
  assert all(bool(torch.isnan(v).all()) for v in outs)


# ======================================================================= c51_target_block
@pytest.mark.parametrize('name', ['B5-A3', 'B2-A16', 'tie-012', 'tie-210'])
def test_c51_target_block_projection_against_float64(name):
  """The target half riding in the fused forward (cnn.forward_fused_c51): a target network
  with fc2_w zeroed and fc2_b set to the wanted logits has exactly those logits for every
  sample; its m against the float64 projection on proj_abs, reward and terminal varying per
  sample.  The tie cases: three atoms, rows with Q exactly 0 in two orders."""
  from dopamine_amd.agents.networks import RainbowNetwork
  from dopamine_amd.cnn import HipNatureCNN, forward_fused_c51
  if name.startswith('tie'):
    order = [int(ch) for ch in name[4:]]
    c = C.c51_tie_case()
    c['tl'] = np.array([[C.TIE_ROWS[r] for r in order]] * c['B'], np.float32)
  else:
    B, A, scale = {'B5-A3': (5, 3, 2), 'B2-A16': (2, 16, 10)}[name]
    c = C.c51_case(B, A, 51, scale)
    c['tl'] = np.repeat(c['tl'][:1], B, 0)                # the one bias, for every sample
  B, A, N = c['B'], c['A'], c['N']
  ref = C.c51_reference(c, False)
  if name.startswith('tie'):
    assert np.all(C.c51_target_q(c) == 0) and np.all(ref['argmax'] == 0)
  else:
    assert C.q_margin(C.c51_target_q(c)).min() >= C.MARGIN_C51
  on = RainbowNetwork(A, num_atoms=N, device='cuda', seed=1)
  tg = RainbowNetwork(A, num_atoms=N, device='cuda', seed=2)
  with torch.no_grad():
    tg.fp.params['fc2_w'].zero_()
    tg.fp.params['fc2_b'].copy_(_t(c['tl'][0].reshape(-1)))
  ho, ht = HipNatureCNN(on, B), HipNatureCNN(tg, B)
  torch.manual_seed(4)
  x, nx = torch.rand(B, 84, 84, 4, device='cuda'), torch.rand(B, 84, 84, 4, device='cuda')
  ht.forward(nx)                                          # the target's conv1, as the backward leaves it
  rew, term, z = _dev(c, 'rew', 'term', 'z')
  m, tl_out = _nan(B + 1, N), _nan(B + 1, A * N)
  forward_fused_c51(ho, x, ht, rew, term, z, c['cg'], m, target_logits_out=tl_out)
  torch.cuda.synchronize()
  ONC.assert_spare_untouched(name + ' m', m, B)
  ONC.assert_spare_untouched(name + ' target logits', tl_out, B)
  assert torch.equal(tl_out[:B], _t(c['tl'].reshape(B, -1)))
  ONC.assert_layer_close('c51_target_block %s m' % name, m[:B], ref['proj'], ref['proj_abs'])
  if name.startswith('tie'):
    for a in range(1, A):
      other = C.c51_reference(dict(c, tl=c['tl'][:, [a] * A]), False)['proj']
      r = ONC.cond_ratio(m[:B], other, ref['proj_abs']).max(1).values
      assert float(r.min()) > 100 * ONC.LAYER_TOL, (a, r)


# ============================================================================== DQN Huber
def _run_dqn(c):
  from dopamine_amd import ops
  B, A = c['B'], c['A']
  bufs = dict(grad=_nan(B + 1, A), loss=_nan(B + 1), mean_loss=_nan(1 + 64))
  oq, tq, act, rew, term = _dev(c, 'oq', 'tq', 'act', 'rew', 'term')
  ops.dqn_huber_loss(oq, tq, act, rew, term, c['cg'], out=_views(bufs, B))
  return bufs


@pytest.mark.parametrize('dyadic', [True, False], ids=['dyadic', 'randn'])
@pytest.mark.parametrize('B,A', C.DQN_SHAPES)
def test_dqn_huber_against_float64(B, A, dyadic):
  """dyadic: err runs through exactly +1, 0, -1 and both sides of 1, every operation exact."""
  c = C.dqn_case(B, A, dyadic=dyadic)
  ref = C.dqn_reference(c)
  bufs = _run_dqn(c)
  _check('dqn B=%d A=%d %s' % (B, A, 'dyadic' if dyadic else 'randn'), bufs, B, C.dqn_checks(ref))
  if dyadic:                            # (the gradient rounds twice, 1 / B and the product)
    assert np.array_equal(bufs['loss'][:B].cpu().numpy(), ref['loss'])


@pytest.mark.parametrize('name', ['all-terminal', 'gamma0'])
def test_dqn_huber_cold_branches(name):
  c = C.dqn_case(7, 64, all_terminal=True) if name == 'all-terminal' else C.dqn_case(257, 4, cg=0.0)
  _check('dqn %s' % name, _run_dqn(c), c['B'], C.dqn_checks(C.dqn_reference(c)))


# ==================================================================================== IQN
def _run_iqn(c, kappa):
  from dopamine_amd import ops
  B, A, N = c['B'], c['A'], c['N']
  bufs = dict(grad=_nan(N * B + 1, A), loss=_nan(B + 1), mean_loss=_nan(1 + 64))
  oq, tq, ta, tau, act, rew, term = _dev(c, 'oq', 'tq', 'ta', 'tau', 'act', 'rew', 'term')
  ops.iqn_loss(oq, tq, ta, tau, act, rew, term, c['cg'], kappa=kappa,
               out=dict(grad=bufs['grad'][:N * B], loss=bufs['loss'][:B],
                        mean_loss=bufs['mean_loss'][:1]))
  return bufs


def _check_iqn(what, bufs, c, ref):
  B, N = c['B'], c['N']
  torch.cuda.synchronize()
  ONC.assert_spare_untouched(what + ' grad', bufs['grad'], N * B)
  ONC.assert_spare_untouched(what + ' loss', bufs['loss'], B)
  ONC.assert_guard_untouched(what + ' mean_loss', bufs['mean_loss'], 1)
  got = dict(grad=bufs['grad'][:N * B], loss=bufs['loss'][:B], mean_loss=bufs['mean_loss'][:1])
  for k, (r, terms) in C.iqn_checks(ref).items():
    ONC.assert_layer_close('%s %s' % (what, k), got[k], np.asarray(r, np.float64),
                           np.asarray(terms, np.float64))


@pytest.mark.parametrize('kappa', C.KAPPAS)
@pytest.mark.parametrize('B,A,N,Np,K', C.IQN_SHAPES)
def test_iqn_loss_against_float64(B, A, N, Np, K, kappa):
  c = C.iqn_case(B, A, N, Np, K)
  _check_iqn('iqn B=%d A=%d N=%d Np=%d K=%d kappa=%g' % (B, A, N, Np, K, kappa),
             _run_iqn(c, kappa), c, C.iqn_reference(c, kappa))


@pytest.mark.parametrize('kappa', C.KAPPAS)
def test_iqn_loss_on_exact_huber_corners(kappa):
  """Dyadic inputs: u hits 0 and +-kappa exactly (asserted on the CPU)."""
  c = C.iqn_dyadic_case(kappa)
  _check_iqn('iqn dyadic kappa=%g' % kappa, _run_iqn(c, kappa), c, C.iqn_reference(c, kappa))


def test_iqn_greedy_tie_takes_the_first_column():
  c = C.iqn_tie_case()
  ref = C.iqn_reference(c, 1.0)
  bufs = _run_iqn(c, 1.0)
  _check_iqn('iqn tie', bufs, c, ref)
  other = C.iqn_reference(dict(c, tq=c['tq'][:, [0, 3, 2, 1, 4]]), 1.0)     # column 3 taken
  r = ONC.cond_ratio(bufs['loss'][:c['B']], other['loss'], other['loss_abs'])
  assert float(r.min()) > 100 * ONC.LAYER_TOL, r


# ============================================================================= optimizers
class _Guarded(object):
  """n floats (16-byte aligned: the head of an allocation) followed by 64 NaN guard floats."""

  def __init__(self, values):
    self.n = len(values)
    self.buf = _nan(self.n + 64)
    self.buf[:self.n] = _t(np.asarray(values, np.float32))

  def ptr(self, lo=0):
    return self.buf.data_ptr() + 4 * lo

  def get(self):
    return self.buf[:self.n].cpu().numpy()

  def check(self, what):
    ONC.assert_guard_untouched(what, self.buf, self.n)
    assert bool(torch.isfinite(self.buf[:self.n]).all()), what


_ADAM = dict(lr=6.25e-5, b1=0.9, b2=0.999, eps=1.5e-4)


def _adam_call(var, g, m, v, state, slot, lo=0, n=None, bump=None):
  from dopamine_amd import _lib
  n = var.n - lo if n is None else n
  args = (var.ptr(lo), g.ptr(lo), m.ptr(lo), v.ptr(lo), _lib.ptr(state), slot, n, _ADAM['lr'],
          _ADAM['b1'], _ADAM['b2'], _ADAM['eps'])
  if bump is None:
    _lib.call('dq_adam_tf1', *(args + (_lib.stream_of(state.device),)))
  else:
    _lib.call('dq_adam_tf1_part', *(args + (int(bump), _lib.stream_of(state.device))))


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 1025])
def test_adam_small_sizes_against_oracle(n):
  rs = np.random.RandomState(n)
  var0 = (rs.randn(n) * 0.05).astype(np.float32)
  var, m, v = _Guarded(var0), _Guarded(np.zeros(n)), _Guarded(np.zeros(n))
  state = _t(np.array([_ADAM['b1'], _ADAM['b2'], 0, 0], np.float32))
  ref = L.TF1Adam(n, _ADAM['lr'], eps=_ADAM['eps'])
  rvar = var0.copy()
  for step in range(3):
    gv = (rs.randn(n) * 1e-2).astype(np.float32)
    g = _Guarded(gv)
    _adam_call(var, g, m, v, state, step % 2)
    ref.step(rvar, gv)
    torch.cuda.synchronize()
    g.check('adam n=%d grad' % n)
  for name, buf, want in (('var', var, rvar), ('m', m, ref.m), ('v', v, ref.v)):
    buf.check('adam n=%d %s' % (n, name))
    np.testing.assert_allclose(buf.get(), want, rtol=1e-5, atol=1e-7, err_msg=name)
  # three steps: the powers beta^4 sit in slot 1
  np.testing.assert_allclose(state.cpu().numpy()[2:], [ref.b1p, ref.b2p], rtol=1e-6)


def test_adam_parts_equal_one_launch_and_advance_the_powers_once():
  """[0, 512) + [512, 1025) with bump on the second part only == one dq_adam_tf1, bitwise,
  over two steps (both slots); the beta powers advance once per step."""
  n = 1025
  rs = np.random.RandomState(7)
  var0 = (rs.randn(n) * 0.05).astype(np.float32)
  one = [_Guarded(var0), _Guarded(np.zeros(n)), _Guarded(np.zeros(n))]
  two = [_Guarded(var0), _Guarded(np.zeros(n)), _Guarded(np.zeros(n))]
  s0 = np.array([_ADAM['b1'], _ADAM['b2'], NAN, NAN], np.float32)
  st1, st2 = _t(s0), _t(s0)
  b1p, b2p = np.float32(_ADAM['b1']), np.float32(_ADAM['b2'])
  for step in range(2):
    g = _Guarded((rs.randn(n) * 1e-2).astype(np.float32))
    _adam_call(one[0], g, one[1], one[2], st1, step % 2)
    _adam_call(two[0], g, two[1], two[2], st2, step % 2, lo=0, n=512, bump=False)
    mid = st2.clone()
    _adam_call(two[0], g, two[1], two[2], st2, step % 2, lo=512, n=513, bump=True)
    torch.cuda.synchronize()
    b1p, b2p = np.float32(b1p * np.float32(_ADAM['b1'])), np.float32(b2p * np.float32(_ADAM['b2']))
    nxt = 2 * ((step % 2) ^ 1)
    assert torch.equal(mid[2 * (step % 2):][:2], st2[2 * (step % 2):][:2])     # this step's slot
    if step == 0:
      assert bool(torch.isnan(mid[nxt:nxt + 2]).all())          # the part without bump wrote none
    assert np.array_equal(st2.cpu().numpy()[nxt:nxt + 2], [b1p, b2p])
    assert torch.equal(st1, st2)
    for a, b, name in zip(one, two, ('var', 'm', 'v')):
      a.check('adam one %s' % name)
      b.check('adam parts %s' % name)
      assert torch.equal(a.buf[:n], b.buf[:n]), (step, name)


@pytest.mark.parametrize('n', [1, 5, 1025])
@pytest.mark.parametrize('momentum', [0.0, 0.9])
@pytest.mark.parametrize('centered', [True, False], ids=['centered', 'uncentered'])
def test_rmsprop_against_oracle(centered, momentum, n):
  from dopamine_amd import _lib
  rs = np.random.RandomState(n + 1)
  var0 = (rs.randn(n) * 0.05).astype(np.float32)
  var, ms, mg, mom = _Guarded(var0), _Guarded(np.ones(n)), _Guarded(np.zeros(n)), _Guarded(np.zeros(n))
  ref = L.TF1CenteredRMSProp(n, 2.5e-4, decay=0.95, momentum=momentum, eps=1e-5, centered=centered)
  rvar = var0.copy()
  for _ in range(3):
    gv = (rs.randn(n) * 1e-2).astype(np.float32)
    g = _Guarded(gv)
    _lib.call('dq_rmsprop_tf1', var.ptr(), g.ptr(), ms.ptr(), mg.ptr(), mom.ptr(), n, 2.5e-4, 0.95,
              momentum, 1e-5, int(centered), _lib.stream_of(var.buf.device))
    ref.step(rvar, gv)
    torch.cuda.synchronize()
  for name, buf, want in (('var', var, rvar), ('ms', ms, ref.ms), ('mg', mg, ref.mg),
                          ('mom', mom, ref.mom)):
    buf.check('rmsprop %s' % name)
    np.testing.assert_allclose(buf.get(), want, rtol=1e-5, atol=1e-7, err_msg=name)
  if not centered:
    assert bool((mg.buf[:n] == 0).all())                        # never written


def test_optimizers_with_no_elements_write_nothing():
  from dopamine_amd import _lib
  bufs = [_nan(64) for _ in range(5)]
  state = _t(np.array([0.9, 0.999, NAN, NAN], np.float32))
  st = _lib.stream_of(state.device)
  p = _lib.ptr
  _lib.call('dq_rmsprop_tf1', p(bufs[0]), p(bufs[1]), p(bufs[2]), p(bufs[3]), p(bufs[4]), 0, 2.5e-4,
            0.95, 0.0, 1e-5, 1, st)
  _lib.call('dq_adam_tf1', p(bufs[0]), p(bufs[1]), p(bufs[2]), p(bufs[3]), p(state), 0, 0,
            _ADAM['lr'], _ADAM['b1'], _ADAM['b2'], _ADAM['eps'], st)
  _lib.call('dq_adam_tf1_part', p(bufs[0]), p(bufs[1]), p(bufs[2]), p(bufs[3]), p(state), 0, 0,
            _ADAM['lr'], _ADAM['b1'], _ADAM['b2'], _ADAM['eps'], 0, st)
  torch.cuda.synchronize()
  assert all(bool(torch.isnan(b).all()) for b in bufs)
  # an empty Adam step is still a step: the powers of slot 0 stay, slot 1 holds the next ones
  s = state.cpu().numpy()
  assert np.array_equal(s[:2], np.array([0.9, 0.999], np.float32))
  assert np.array_equal(s[2:], np.array([0.9, 0.999], np.float32) ** 2)
