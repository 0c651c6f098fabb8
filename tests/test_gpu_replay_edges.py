"""The replay kernels (dopamine_amd/csrc/replay.hip, replay_dev.h) at their structural edges,
through the drop-in classes and the C ABI, bit for bit against oracle/replay.py, the
reference's long-horizon vectors (tests/golden/replay_horizon.npz) or plain numpy: no
tolerance anywhere.  The shapes are the smallest that reach each branch; the hand-picked
seeds and stores come from tests/replay_edge_cases.py, whose properties
tests/test_replay_edges_reference_cpu.py proves with the oracle alone."""
import random

import numpy as np
import pytest
import torch

from oracle import replay as orc
from tests import replay_edge_cases as ec
from tests.test_oracle_golden import SHAPE_KEYS, shape_case

pytestmark = pytest.mark.gpu

HORIZON = 'replay_horizon.npz'
SCALARS = ['action', 'reward', 'next_action', 'next_reward', 'terminal', 'indices']


def _mods():
  from dopamine_amd import _lib
  from dopamine_amd.replay_memory import circular_replay_buffer as crb
  from dopamine_amd.replay_memory import prioritized_replay_buffer as prb
  return _lib, crb, prb


def _device(store, prioritized=False, B=32, leaves=None, **kw):
  """A device buffer holding ``store`` (load_arrays), as store.oracle() holds it."""
  _, crb, prb = _mods()
  cls = prb.OutOfGraphPrioritizedReplayBuffer if prioritized else crb.OutOfGraphReplayBuffer
  m = cls(store.obs_shape, store.stack, store.C, B, update_horizon=store.n,
          observation_dtype=store.obs_dtype.type, **kw)
  m.load_arrays(torch.from_numpy(store.obs.reshape(store.C, -1).view(np.uint8)),
                torch.from_numpy(store.act), torch.from_numpy(store.rew),
                torch.from_numpy(store.term), add_count=store.add_count)
  if leaves is not None:
    t = orc.SumTree.from_leaves(store.C, leaves)
    m.load_tree_nodes(t.nodes, t.max_recorded_priority)
  return m


def _np_state_equal(a, b):
  a, b = a.get_state(), b.get_state()
  return a[2] == b[2] and np.array_equal(a[1], b[1])


def _cases(kind):
  return ['%s_n%d_s%d' % (kind, n, s) for n in (7, 8, 9, 17, 64, 65, 137) for s in (1, 4)]


# ------------------------------------------------------------------ n-step return, scalars
@pytest.mark.parametrize('name', _cases('uni') + _cases('per'))
def test_horizon_goldens(golden, name):
  """The reference's own batches at update horizons 7 .. 137 (np.sum's pairwise order from
  8 products on; 64 / 65 cross the one-wave trajectory; terminals at step 1, at step n and
  absent; idx + L re-reads; ring wraps), then the scalars of every gather layout."""
  _lib, crb, prb = _mods()
  z = golden(HORIZON)
  m = ec.horizon_meta(z, name)
  rng = random.Random(m['seed']) if m['prioritized'] else np.random.RandomState(m['seed'])
  cls = prb.OutOfGraphPrioritizedReplayBuffer if m['prioritized'] else crb.OutOfGraphReplayBuffer
  mem = cls((2, 2), m['stack'], m['C'], m['B'], update_horizon=m['n'], gamma=float(z['gamma']),
            rng=rng)
  ec.replay_horizon_case(z, name, mem, ec.exact)
  # the last snapshot's batch (every valid index) through the three layouts
  last = int(z[name + '_snaps'][1][-1])
  want = {k: z[name + '_snap_' + k][-last:] for k in SCALARS}
  idx = torch.from_numpy(want['indices'].astype(np.int32)).cuda()
  layouts = [_lib.LAYOUT_RAW, _lib.LAYOUT_F32_NORM] + ([_lib.LAYOUT_F32_NHWC] if m['stack'] == 4 else [])
  for layout in layouts:
    out = mem.sample_device(last, layout=layout, indices=idx)
    for k in SCALARS:
      ec.exact(k, out[k].cpu().numpy(), want[k], '%s layout %d' % (name, layout))


def test_horizon_element_goldens(golden):
  """k_gather_elems' scalar branch at n = 9 and 17 (float64, float16, int32 rewards) and a
  shaped (9,) float32 reward, against the reference's batches."""
  _, crb, _ = _mods()
  z = golden(HORIZON)
  for name in [str(c) for c in z['elem_cases']]:
    pre = 'elem_' + name
    kw, adds, rounds = shape_case(z, pre)
    mem = crb.OutOfGraphReplayBuffer(rng=np.random.RandomState(int(z[pre + '_seed'])), **kw)
    for i in range(adds):
      mem.add(z[pre + '_obs'][i], z[pre + '_act'][i], z[pre + '_rew'][i], z[pre + '_term'][i])
    for r in range(rounds):
      for k, v in zip(SHAPE_KEYS, mem.sample_transition_batch()):
        ec.exact(k, v, z[pre + '_' + k][r], '%s round %d' % (pre, r))
    fixed = [int(i) for i in z[pre + '_fixed_indices']]
    for k, v in zip(SHAPE_KEYS, mem.sample_transition_batch(len(fixed), indices=fixed)):
      ec.exact(k, v, z[pre + '_fixed_' + k], pre + ' fixed')


# --------------------------------------------------------------------------------- gathers
def _gather_store(obs_shape, stack, C, obs_dtype=np.uint8, seed=7):
  st = ec.Store(C=C, stack=stack, n=3, add_count=C + 5, p_term=0.15, seed=seed,
                obs_shape=obs_shape, obs_dtype=obs_dtype)
  st.term[C // 2] = 1             # idx = C/2 - 1: L = 2, the next state is re-read at idx + 2
  flat = st.obs.reshape(-1).view(np.uint8)
  if flat.size >= 256:            # every byte value occurs (every u8_unit input)
    flat[:256] = np.random.RandomState(seed).permutation(256).astype(np.uint8)
  return st


def _batches(st, o):
  """Index batches of B = 1, 2, 33 and C: stacks that wrap below 0, idx + L past C, indices
  that are negative or >= C (taken modulo C), and a next-state whose idx + L != idx + n."""
  C = st.C
  rs = np.random.RandomState(C)
  edge = [0, 1, 2, C - 1, C - 2, -1, -C - 2, C, C + 3, 2 * C + 1]
  cut = [i for i in range(C) if o.nstep(i)[2] != st.n]
  assert cut, 'no trajectory is cut short by a terminal'
  b33 = (edge + cut[:3] + [int(i) for i in rs.randint(0, C, 33)])[:33]
  assert any(o.nstep(i % C)[2] != st.n for i in b33)
  return [[cut[0]], [C - 1, -1], b33, list(range(C))]


GATHER_CASES = (
    # F32_NORM: one block covers 1024 dwords -- obs_bytes 4, 4096 (nd 1024), 4100 (nd 1025)
    [('norm', s, st, C) for s, st, C in [((4,), 5, 70), ((2, 2), 4, 70), ((64, 64), 2, 9),
                                         ((4100,), 1, 9)]] +
    # F32_NHWC: a block column covers 256 dwords, a wave 64 -- nd 1, 63, 64, 65, 256, 257
    [('nhwc', s, 4, C) for s, C in [((2, 2), 70), ((4, 63), 11), ((4, 64), 11), ((4, 65), 11),
                                    ((32, 32), 9), ((4, 257), 9)]] +
    # RAW: byte loop (7, 12 = float32 x 3), 16-byte loop (16, 4096), grid-stride loop
    # (64 blocks x 256 threads x 16 bytes = 262144 < 262160)
    [('raw', s, st, C) for s, st, C in [((7,), 4, 40), ((16,), 3, 20), ((64, 64), 1, 9),
                                        ((262160,), 2, 6)]] +
    [('raw_f32', (3,), 4, 30)])


@pytest.mark.parametrize('layout,obs_shape,stack,C', GATHER_CASES,
                         ids=['%s-%s-s%d' % (c[0], 'x'.join(map(str, c[1])), c[2])
                              for c in GATHER_CASES])
@pytest.mark.parametrize('prioritized', [False, True], ids=['uniform', 'per'])
def test_gather_layout_edges(layout, obs_shape, stack, C, prioritized):
  """stack_at / float32(raw) / 255 and the scalars for every batch, written into slices of
  larger sentinel-filled buffers: nothing outside the slices may change."""
  _lib, _, _ = _mods()
  dt = np.float32 if layout == 'raw_f32' else np.uint8
  st = _gather_store(obs_shape, stack, C, dt)
  o = st.oracle(prioritized)
  leaves = np.random.RandomState(3).uniform(0.1, 2.0, C) if prioritized else None
  if prioritized:
    o.sum_tree = orc.SumTree.from_leaves(C, leaves)
  m = _device(st, prioritized, leaves=leaves)
  code = {'norm': _lib.LAYOUT_F32_NORM, 'nhwc': _lib.LAYOUT_F32_NHWC}.get(layout, _lib.LAYOUT_RAW)
  names = ['state', 'next_state'] + SCALARS + (['sampling_probabilities'] if prioritized else [])
  for idx in _batches(st, o):
    B = len(idx)
    want = o.sample_transition_batch(B, indices=[i % C for i in idx])
    plain = m._alloc_batch(B, code)
    big, out = {}, {}
    for k in names:        # one sentinel row before and one after each output
      t = plain[k]
      nhwc = code == _lib.LAYOUT_F32_NHWC and k.endswith('state')
      rest = tuple((t.permute(0, 2, 3, 1) if nhwc else t).shape[1:])
      row = int(np.prod(rest, dtype=np.int64)) * t.element_size()
      big[k] = torch.full(((B + 2) * row,), 0x5A, dtype=torch.uint8, device='cuda')
      typed = big[k].view(t.dtype).reshape((B + 2,) + rest)[1:B + 1]
      out[k] = typed.permute(0, 3, 1, 2) if nhwc else typed
      assert out[k].shape == t.shape and out[k].stride() == t.stride()
    got = m.sample_device(B, layout=code, out=out,
                          indices=torch.tensor(idx, dtype=torch.int32, device='cuda'))
    torch.cuda.synchronize()
    for k in names:
      edge = big[k].reshape(B + 2, -1)
      assert bool((edge[0] == 0x5A).all()) and bool((edge[-1] == 0x5A).all()), (k, B)
    for k, w in zip(SCALARS, [want[1], want[2], want[4], want[5], want[6], want[7]]):
      ec.exact(k, got[k].cpu().numpy(), w.astype(got[k].cpu().numpy().dtype), 'B %d' % B)
    if prioritized:
      ec.exact('probs', got['sampling_probabilities'].cpu().numpy(), want[8], 'B %d' % B)
    for k, w in (('state', want[0]), ('next_state', want[3])):     # w: (B,) + obs_shape + (S,)
      g = got[k].cpu()
      if code == _lib.LAYOUT_F32_NHWC:
        ec.exact(k, g.permute(0, 2, 3, 1).numpy(), w.astype(np.float32) / np.float32(255), 'B %d' % B)
      elif code == _lib.LAYOUT_F32_NORM:
        ec.exact(k, g.numpy(), np.moveaxis(w, -1, 1).astype(np.float32) / np.float32(255), 'B %d' % B)
      else:
        have = g.numpy().reshape(B, stack, -1).view(np.uint8)
        ec.exact(k, have, np.ascontiguousarray(np.moveaxis(w, -1, 1)).reshape(B, stack, -1).view(np.uint8),
                 'B %d' % B)


def test_gather_refusals():
  _lib, crb, prb = _mods()
  idx = torch.zeros(4, dtype=torch.int32, device='cuda')

  def refused(mem, layout, text, B=4, i=idx):
    with pytest.raises(_lib.DQError) as e:
      mem.sample_device(B, layout=layout, indices=i)
    assert text in str(e.value)

  refused(crb.OutOfGraphReplayBuffer((7,), 1, 10, 4), _lib.LAYOUT_F32_NORM,
          'F32_NORM layout needs obs_bytes % 4 == 0')
  refused(crb.OutOfGraphReplayBuffer((3, 2), 4, 10, 4), _lib.LAYOUT_F32_NHWC,
          'F32_NHWC layout needs obs_bytes % 4 == 0')
  f32 = crb.OutOfGraphReplayBuffer((2, 2), 4, 10, 4, observation_dtype=np.float32)
  for layout, text in ((_lib.LAYOUT_F32_NORM, 'F32_NORM layout needs uint8 observations'),
                       (_lib.LAYOUT_F32_NHWC, 'F32_NHWC layout needs uint8 observations')):
    with pytest.raises(_lib.DQError) as e:
      out = f32._alloc_batch(4, _lib.LAYOUT_RAW)
      f32.sample_device(4, layout=layout, out=out, indices=idx)
    assert text in str(e.value)
  refused(crb.OutOfGraphReplayBuffer((2, 2), 2, 10, 4), _lib.LAYOUT_F32_NHWC,
          'F32_NHWC layout needs stack_size == 4')
  small = crb.OutOfGraphReplayBuffer((1,), 4, 10, 4)
  refused(small, _lib.LAYOUT_RAW, 'batch * 2 * stack too large', B=8192,
          i=torch.zeros(8192, dtype=torch.int32, device='cuda'))
  small.sample_device(8191, layout=_lib.LAYOUT_RAW,
                      indices=torch.zeros(8191, dtype=torch.int32, device='cuda'))   # 65528 slots
  refused(small, 7, 'unknown layout')
  out = small._alloc_batch(4, _lib.LAYOUT_RAW)
  p = _lib.ptr
  with pytest.raises(_lib.DQError) as e:
    _lib.call('dq_replay_gather', small._h, p(idx), 4, _lib.LAYOUT_RAW, p(out['state']),
              p(out['next_state']), p(out['action']), p(out['reward']), p(out['next_action']),
              p(out['next_reward']), p(out['terminal']), p(out['indices']), p(out['reward']),
              small._stream)
  assert 'probs requested from a uniform buffer' in str(e.value)
  # a gather recorded as a rider sums left to right: refused from update_horizon 8 on, by
  # the drop-in class and by the C ABI
  import ctypes
  for n, ok in ((7, True), (8, False)):
    long = crb.OutOfGraphReplayBuffer((2, 2), 4, 40, 4, update_horizon=n)
    out = long._alloc_batch(4, _lib.LAYOUT_F32_NHWC)
    r = _lib.Rider()
    args = (long._h, p(idx), 4, p(out['state']), p(out['next_state']), p(out['action']),
            p(out['reward']), p(out['next_action']), p(out['next_reward']), p(out['terminal']),
            p(out['indices']), None, ctypes.byref(r))
    if ok:
      _lib.call('dq_replay_record_gather_nhwc', *args)
      with long.recording() as riders:
        long.sample_device(4, layout=_lib.LAYOUT_F32_NHWC, indices=idx)
      assert len(riders) == 1
    else:
      with pytest.raises(_lib.DQError, match='a recorded gather needs update_horizon < 8'):
        _lib.call('dq_replay_record_gather_nhwc', *args)
      with long.recording():
        with pytest.raises(ValueError, match='update_horizon < 8'):
          long.sample_device(4, layout=_lib.LAYOUT_F32_NHWC, indices=idx)
  torch.cuda.synchronize()


# --------------------------------------------------------------------- prioritized sampler
def _edge_leaves(C, seed):
  """~30 % zeros, zero runs at both ends, values over 1e-3 .. 1e3 (the descent's
  subtractions round); the padded leaves beyond C stay zero."""
  rs = np.random.RandomState(seed)
  leaves = 10.0 ** rs.uniform(-3, 3, C)
  if C > 16:
    leaves[rs.rand(C) < 0.3] = 0.0
    leaves[:5] = 0.0
    leaves[-7:] = 0.0
  else:
    leaves[0] = 0.0
  return leaves


@pytest.mark.parametrize('C', [2, 1024, 1025, 32768, 32769, 2 ** 20 + 1])
def test_per_sampler_depths(C):
  """Depths 1, 10, 11, 15, 16, 21: the LDS levels alone, one partial 5-level round, one full
  round, a round plus one level, two rounds plus one level; B = 1, 31, 32, 33, 1024 (32
  strata per pass); indices or the reference's error, and random's state, equal the oracle's."""
  _lib, _, _ = _mods()
  st = ec.Store(C=C, stack=1, n=1, add_count=C + C // 3, p_term=0, seed=C % 1000)
  leaves = _edge_leaves(C, C % 1000 + 1)
  m = _device(st, True, leaves=leaves, rng=random.Random(C))
  assert m._depth == {2: 1, 1024: 10, 1025: 11, 32768: 15, 32769: 16, 2 ** 20 + 1: 21}[C]
  o = st.oracle(True, py_rng=random.Random(C))
  o.sum_tree = orc.SumTree.from_leaves(C, leaves)
  for B in (1, 31, 32, 33, 1024):
    try:
      want = o.sample_index_batch(B)
    except RuntimeError as e:
      with pytest.raises(RuntimeError) as got:
        m.sample_index_batch(B)
      assert str(got.value) == str(e)
    else:
      assert m.sample_index_batch(B) == want, B
    assert m._rng.stream.getstate() == o.py_rng.getstate(), B
  with pytest.raises(_lib.DQError, match=r'batch must be in \[1, 1024\]'):
    m.sample_index_batch(1025)


@pytest.mark.parametrize('which', ['error', 'invalid', 'ok'])
def test_per_retry_budget(which):
  """max_sample_attempts = 3, terminals at 1/20, stack 4: the budget runs out on a later
  stratum (the reference's error with its count), on the last invalid stratum (the invalid
  index is returned), or not at all."""
  seed = {'error': ec.RETRY_SEED_ERROR, 'invalid': ec.RETRY_SEED_INVALID, 'ok': ec.RETRY_SEED_OK}[which]
  st, leaves = ec.retry_store(), ec.retry_leaves(600)
  kind, want, o = ec.per_outcome(st, leaves, ec.RETRY_B, seed, ec.RETRY_MAX)
  assert kind == which
  m = _device(st, True, B=ec.RETRY_B, leaves=leaves, rng=random.Random(seed),
              max_sample_attempts=ec.RETRY_MAX)
  if which == 'error':
    with pytest.raises(RuntimeError) as e:
      m.sample_index_batch(ec.RETRY_B)
    assert str(e.value) == want
  else:
    assert m.sample_index_batch(ec.RETRY_B) == want
  assert m._rng.stream.getstate() == o.py_rng.getstate()


def test_per_rewind_restores_entry_cursor():
  st, leaves = ec.retry_store(), ec.retry_leaves(600)
  _lib, _, _ = _mods()
  m = _device(st, True, B=32, leaves=leaves, rng=random.Random(5))
  m.sample_device(32, layout=_lib.LAYOUT_RAW)
  p0 = int(m._read_meta().tape_pos)
  first = m.sample_device(32, layout=_lib.LAYOUT_RAW)['indices'].clone()
  meta = m._read_meta()
  assert int(meta.tape_pos) > p0 and int(meta.reserved[0]) == p0
  m.rewind_last_sample()
  assert int(m._read_meta().tape_pos) == p0
  assert torch.equal(m.sample_device(32, layout=_lib.LAYOUT_RAW)['indices'], first)


# ------------------------------------------------------------------------- uniform sampler
@pytest.mark.parametrize('B', [1, 64, 65, 1024])
def test_uniform_sampler_batches(B):
  st = ec.Store(C=5000, stack=4, n=3, add_count=5000 + 321, p_term=1 / 50., seed=11)
  m = _device(st, B=B, rng=np.random.RandomState(B))
  o = st.oracle(B=B, np_rng=np.random.RandomState(B))
  for _ in range(3):
    assert m.sample_index_batch(B) == o.sample_index_batch(B)
  assert _np_state_equal(m._rng.stream, o.np_rng)


def test_uniform_width_one():
  """max_id - min_id == 1: randint consumes no word.  A valid single index fills the batch;
  an invalid one exhausts max_sample_attempts at once."""
  ok = ec.Store(C=10, stack=1, n=1, add_count=2, p_term=0, seed=1)
  m, o = _device(ok, B=5, rng=np.random.RandomState(1)), ok.oracle(B=5, np_rng=np.random.RandomState(1))
  assert o._id_range() == (0, 1)
  assert m.sample_index_batch(5) == o.sample_index_batch(5) == [0] * 5
  assert _np_state_equal(m._rng.stream, o.np_rng) and _np_state_equal(o.np_rng, np.random.RandomState(1))
  bad = ec.Store(C=2, stack=1, n=1, add_count=2 + 1, p_term=0, seed=1)
  m = _device(bad, B=5, rng=np.random.RandomState(1), max_sample_attempts=9)
  o = bad.oracle(B=5, np_rng=np.random.RandomState(1), max_sample_attempts=9)
  with pytest.raises(RuntimeError) as want:
    o.sample_index_batch(5)
  with pytest.raises(RuntimeError) as got:
    m.sample_index_batch(5)
  assert str(got.value) == str(want.value) and 'Tried 9 times but only sampled 0' in str(got.value)
  assert _np_state_equal(m._rng.stream, np.random.RandomState(1))


@pytest.mark.parametrize('seed,words', [(ec.WINDOW_SEED_LAST_LANE, 64), (ec.WINDOW_SEED_FIRST_LANE, 65)])
def test_uniform_window_boundary(seed, words):
  """Width 33 (heavy mask rejection); the B-th accepted draw is the last word of a 64-word
  window / the first word of the next."""
  st = ec.window_store()
  want, w = ec.uniform_words(st, ec.WINDOW_B, seed)
  assert w == words
  m = _device(st, B=ec.WINDOW_B, rng=np.random.RandomState(seed))
  assert m.sample_index_batch(ec.WINDOW_B) == want
  after = np.random.RandomState(seed)
  after.randint(0, 2 ** 32, size=words, dtype=np.uint32)
  assert _np_state_equal(m._rng.stream, after)


@pytest.mark.parametrize('seed', [ec.ATTEMPTS_SEED_FAILS, ec.ATTEMPTS_SEED_PASSES])
def test_uniform_attempts_budget(seed):
  st = ec.attempts_store()
  want, words = ec.uniform_words(st, ec.ATTEMPTS_B, seed, ec.ATTEMPTS_MAX)
  m = _device(st, B=ec.ATTEMPTS_B, rng=np.random.RandomState(seed), max_sample_attempts=ec.ATTEMPTS_MAX)
  if isinstance(want, str):
    with pytest.raises(RuntimeError) as e:
      m.sample_index_batch(ec.ATTEMPTS_B)
    assert str(e.value) == want
  else:
    assert m.sample_index_batch(ec.ATTEMPTS_B) == want
  after = np.random.RandomState(seed)
  after.randint(0, 2 ** 32, size=words, dtype=np.uint32)
  assert _np_state_equal(m._rng.stream, after)


@pytest.mark.parametrize('B,G', [(32, 2), (16, 5), (128, 8)])
def test_uniform_groups(B, G):
  """groups consecutive batches in one launch == that many oracle calls; the rewind cursor
  is the last group's entry; after sync_rng the numpy stream equals the oracle's."""
  _lib, _, _ = _mods()
  st = ec.Store(C=5000, stack=4, n=3, add_count=5000 + 321, p_term=1 / 50., seed=11)
  done, err, words, o = ec.groups_outcome(st, B, G, seed=B + G, max_attempts=1000)
  assert err is None
  m = _device(st, B=B, rng=np.random.RandomState(B + G))
  out = m.sample_device(B, layout=_lib.LAYOUT_RAW, groups=G)
  meta = m._read_meta()
  assert out['sample_indices'].cpu().tolist() == [i for g in done for i in g]
  assert out['indices'].cpu().tolist() == [i for g in done for i in g]
  assert int(meta.tape_pos) == sum(words) and int(meta.reserved[0]) == sum(words[:-1])
  m.rewind_last_sample()
  assert int(m._read_meta().tape_pos) == sum(words[:-1])
  _lib.call('dq_replay_sample_indices', m._h, B, _lib.ptr(out['sample_indices']), m._stream)
  assert out['sample_indices'][:B].cpu().tolist() == done[-1]
  m.sync_rng()
  assert _np_state_equal(m._rng.stream, o.np_rng)


def test_uniform_groups_failing_group():
  """The third of five groups runs out of attempts: the later groups are zeroed and that
  group's own error is raised; the stream stands where the oracle's stands after its error."""
  _lib, _, _ = _mods()
  st, B, G = ec.attempts_store(), ec.ATTEMPTS_B, ec.GROUPS
  done, err, words, o = ec.groups_outcome(st, B, G, ec.GROUP_SEED_THIRD_FAILS, ec.ATTEMPTS_MAX)
  assert len(done) == 2 and err
  m = _device(st, B=B, rng=np.random.RandomState(ec.GROUP_SEED_THIRD_FAILS),
              max_sample_attempts=ec.ATTEMPTS_MAX)
  out = m.sample_device(B, layout=_lib.LAYOUT_RAW, groups=G)
  got = out['sample_indices'].cpu().tolist()
  assert got[:2 * B] == done[0] + done[1]
  assert got[3 * B:] == [0] * (2 * B)
  meta = m._read_meta()
  assert int(meta.tape_pos) == sum(words) and int(meta.reserved[0]) == sum(words[:2])
  with pytest.raises(RuntimeError) as e:
    m.sync_rng()
  assert str(e.value) == err
  assert _np_state_equal(m._rng.stream, o.np_rng)


# ------------------------------------------------------------------------ sum-tree kernels
def _tree_buffer(C):
  """(device object with _h / _tree / _read_meta, oracle tree) of capacity C, same nodes."""
  _, _, prb = _mods()
  from dopamine_amd.replay_memory import sum_tree
  leaves = np.random.RandomState(C % 977).uniform(0.0, 2.0, C)
  t = orc.SumTree.from_leaves(C, leaves)
  if C == 1:
    dev = sum_tree.SumTree(1)._buf
    dev._tree.copy_(torch.from_numpy(t.nodes))
  else:
    dev = prb.OutOfGraphPrioritizedReplayBuffer((1,), 1, C, 1)
    dev.load_tree_nodes(t.nodes, 1.0)
  t.max_recorded_priority = 1.0
  return dev, t


def _updates(n, depth, C, seed):
  rs = np.random.RandomState(seed)
  idx = rs.randint(0, 2 ** depth, n).astype(np.int32)      # [C, 2^depth): the padded leaves
  idx[::3] = rs.randint(0, min(2 ** depth, 4), len(idx[::3]))   # heavy duplication
  if n > 64:
    idx[64] = idx[63]                                        # a pair across the chunk boundary
  val = rs.uniform(0.0, 3.0, n)
  val[rs.rand(n) < 0.2] = 0.0
  return idx, val


def _set(dev, idx, val, f64):
  _lib, _, _ = _mods()
  d_i = torch.from_numpy(idx).cuda()
  if f64:
    d_v = torch.from_numpy(val.astype(np.float64)).cuda()
    _lib.call('dq_sumtree_set_f64', dev._h, _lib.ptr(d_i), _lib.ptr(d_v), len(idx), dev._stream)
  else:
    d_v = torch.from_numpy(val.astype(np.float32)).cuda()
    _lib.call('dq_sumtree_set', dev._h, _lib.ptr(d_i), _lib.ptr(d_v), len(idx), dev._stream)
  torch.cuda.synchronize()


SET_CASES = [(1, (1, 63, 64, 65, 129)), (2, (1, 63, 64, 65, 128, 129)),
             (2 ** 15, (1, 63, 64, 65, 128, 129)), (2 ** 16, (64, 65, 129)),
             (2 ** 17, (64, 65, 129)), (2 ** 20 + 1, (64, 129))]


@pytest.mark.parametrize('f64', [False, True], ids=['f32', 'f64'])
@pytest.mark.parametrize('C,ns', SET_CASES, ids=['depth%d' % d for d in (0, 1, 15, 16, 17, 21)])
def test_sumtree_set_edges(C, ns, f64):
  """oracle.SumTree.set in order: n across the 64-update chunk, duplicates (one leaf 64
  times; a pair across the chunk boundary), zeros, padded leaves, depths 0 .. 21 (sixteen
  waves own levels w, w + 16: 15 / 16 / 17 cross onto a wave's second level)."""
  dev, t = _tree_buffer(C)
  depth = t.depth
  assert int(np.log2(len(t.nodes) + 1)) - 1 == depth
  for n in ns:
    idx, val = _updates(n, depth, C, n + depth)
    val = val if f64 else val.astype(np.float32)
    _set(dev, idx, np.asarray(val), f64)
    for i, v in zip(idx, val):
      t.set(int(i), v)
    np.testing.assert_array_equal(dev._tree.cpu().numpy(), t.nodes, err_msg='n %d' % n)
    assert float(dev._read_meta().max_recorded_priority) == float(t.max_recorded_priority)
  one = np.full(64, min(3, 2 ** depth - 1), np.int32)     # the longest node_chain
  val = np.random.RandomState(5).uniform(0.0, 9.0, 64)
  val = val if f64 else val.astype(np.float32)
  _set(dev, one, np.asarray(val), f64)
  for i, v in zip(one, val):
    t.set(int(i), v)
  np.testing.assert_array_equal(dev._tree.cpu().numpy(), t.nodes)
  assert float(dev._read_meta().max_recorded_priority) == float(t.max_recorded_priority) > 3.0


@pytest.mark.parametrize('pos', [0, 63, 64])
@pytest.mark.parametrize('kind', ['negative', 'index_below', 'index_above'])
def test_sumtree_set_stops_at_first_bad_update(pos, kind):
  """The updates before the first negative value / bad index are applied, the latched error
  names its position and value, and the updates after it are not applied."""
  _lib, _, _ = _mods()
  C = 1000
  dev, t = _tree_buffer(C)
  idx, val = _updates(100, t.depth, C, pos)
  val = val.astype(np.float32)
  if kind == 'negative':
    val[pos] = -0.25
    val[pos + 3] = -1.0
  else:
    idx[pos] = -3 if kind == 'index_below' else 2 ** t.depth
  _set(dev, idx, val, False)
  for i, v in zip(idx[:pos], val[:pos]):
    t.set(int(i), v)
  np.testing.assert_array_equal(dev._tree.cpu().numpy(), t.nodes)
  meta = dev._read_meta()
  assert int(meta.status_arg) == pos
  assert float(meta.max_recorded_priority) == float(t.max_recorded_priority)
  if kind == 'negative':
    assert int(meta.status) == _lib.ST_NEG_PRIORITY and float(meta.status_value) == -0.25
    with pytest.raises(ValueError, match='Sum tree values should be nonnegative. Got -0.25'):
      dev.sync_rng()
  else:
    assert int(meta.status) == _lib.ST_BAD_INDEX and float(meta.status_value) == float(idx[pos])
    with pytest.raises(IndexError, match='index %d is out of bounds' % idx[pos]):
      dev.sync_rng()
  again = np.arange(5, dtype=np.int32)             # the status was cleared: updates apply again
  _set(dev, again, np.abs(val[:5]), False)
  for i, v in zip(again, np.abs(val[:5])):
    t.set(int(i), v)
  np.testing.assert_array_equal(dev._tree.cpu().numpy(), t.nodes)


@pytest.mark.parametrize('C', [3, 1025, 32769])
def test_sumtree_rebuild_and_get(C):
  _lib, _, prb = _mods()
  leaves = _edge_leaves(C, C)
  t = orc.SumTree.from_leaves(C, leaves)
  m = prb.OutOfGraphPrioritizedReplayBuffer((1,), 1, C, 1)
  m._set_tree_leaves(leaves)
  np.testing.assert_array_equal(m._tree.cpu().numpy(), t.nodes)
  top = 2 ** t.depth
  idx = np.array([0, 1, C - 1, C, top - 1, -1, top, top + 5, -2 ** 31, 2 ** 31 - 1], np.int32)
  want = np.array([t.nodes[top - 1 + i] if 0 <= i < top else 0.0 for i in idx], np.float32)
  got = m.get_priority(torch.from_numpy(idx).cuda()).cpu().numpy()
  ec.exact('get', got, want, 'C %d' % C)


# --------------------------------------------------------------------- add, epsilon-greedy
def test_padded_add_across_the_ring_end():
  """obs_bytes = 7 (no alignment), stack 4: episode starts add 3 zero rows plus the
  transition in one call; some of those calls cross the ring end."""
  _, _, prb = _mods()
  C, S = 11, 4
  rs = np.random.RandomState(2)
  m = prb.OutOfGraphPrioritizedReplayBuffer((7,), S, C, 2, update_horizon=1)
  o = orc.PrioritizedOracle((7,), S, C, 2, update_horizon=1)
  crossed = 0
  for i in range(70):
    obs = rs.randint(0, 256, 7).astype(np.uint8)
    a, r, t = int(rs.randint(0, 5)), np.float32(rs.randn()), int(rs.rand() < 0.3)
    p = np.float32(rs.uniform(0.1, 2.0))
    crossed += o._pad() and o.cursor() + S > C
    m.add(obs, a, r, t, p)
    o.add(obs, a, r, t, p)
    if i % 10 == 9:
      store = m._store
      np.testing.assert_array_equal(store['observation'], o.observation)
      np.testing.assert_array_equal(store['action'], o.action)
      ec.exact('reward', store['reward'], o.reward, 'add %d' % i)
      np.testing.assert_array_equal(store['terminal'], o.terminal)
      np.testing.assert_array_equal(m._tree.cpu().numpy(), o.sum_tree.nodes)
      assert int(m._read_meta().add_count) == o.add_count == int(m.add_count)
  assert crossed >= 2


def _egreedy(m, q, A, eps):
  _lib, _, _ = _mods()
  out = torch.full((1,), -7, dtype=torch.int32, device='cuda')
  _lib.call('dq_replay_egreedy', m._h, _lib.ptr(q), A, float(eps), _lib.ptr(out), m._stream)
  return int(out.item())


@pytest.mark.parametrize('A', [1, 2, 3, 4, 5, 255, 256, 257])
def test_egreedy_matches_python_random(A):
  """random.random() then random.randint(0, A - 1) on the tape (bit-length edges of A),
  epsilon 0 and 1, first maximum on ties, -inf entries; random's state afterwards."""
  st = ec.Store(C=20, stack=1, n=1, add_count=25, p_term=0, seed=1)
  rs = np.random.RandomState(A)
  for eps in (0.0, 1.0, 0.5):
    m = _device(st, True, leaves=np.ones(20), rng=random.Random(A))
    ref = random.Random(A)
    m._rng.rebuild(4096, m._stream)
    for trial in range(40):
      q = rs.randint(-2, 3, A).astype(np.float32)          # ties
      q[rs.rand(A) < 0.3] = -np.inf
      if trial == 0:
        q[:] = -np.inf
      want = ref.randint(0, A - 1) if ref.random() <= eps else int(np.argmax(q))
      assert _egreedy(m, torch.from_numpy(q).cuda(), A, eps) == want, (eps, trial)
    m.sync_rng()
    assert m._rng.stream.getstate() == ref.getstate()


def test_egreedy_tape_ends_mid_redraw():
  """The explore draw's first word is rejected and the tape ends there: -1, nothing consumed."""
  _lib, _, _ = _mods()
  A = 257
  for seed in range(100):
    r = random.Random(seed)
    r.random()
    if r.getrandbits(32) >> (32 - 9) >= A:
      break
  st = ec.Store(C=20, stack=1, n=1, add_count=25, p_term=0, seed=1)
  m = _device(st, True, leaves=np.ones(20), rng=random.Random(seed))
  m._rng.rebuild(64, m._stream)
  _lib.call('dq_replay_set_tape', m._h, 3, m._stream)
  q = torch.zeros(A, device='cuda')
  assert _egreedy(m, q, A, 1.0) == -1
  assert int(m._read_meta().tape_pos) == 0
  _lib.call('dq_replay_set_tape', m._h, 64, m._stream)
  ref = random.Random(seed)
  ref.random()
  assert _egreedy(m, q, A, 1.0) == ref.randint(0, A - 1)
  m.sync_rng()
  assert m._rng.stream.getstate() == ref.getstate()


def test_agent_with_a_long_horizon_trains_without_riders():
  """update_horizon = 10 (data-efficient Rainbow): the gather does not ride in the backward's
  launches (a rider sums left to right), the step runs, and the batch it trains on carries
  the n-step rewards in np.sum's order."""
  from dopamine_amd.agents.optimizers import AdamOptimizer
  from dopamine_amd.agents.rainbow.rainbow_agent import RainbowAgent
  random.seed(3)
  C, n = 600, 10
  a = RainbowAgent(num_actions=4, update_horizon=n, replay_capacity=C, batch_size=32,
                   min_replay_history=100, optimizer=AdamOptimizer(6.25e-5, epsilon=1.5e-4),
                   use_hip_graph=False)
  assert a.ride_replay is False and not a._rides()
  short = RainbowAgent(num_actions=4, update_horizon=7, replay_capacity=C, batch_size=32,
                       min_replay_history=100, use_hip_graph=False)
  assert short.ride_replay is True
  rs = np.random.RandomState(4)
  rew = rs.randn(C).astype(np.float32)
  term = (rs.rand(C) < 0.02).astype(np.uint8)
  mem = a._replay.memory
  mem.load_arrays(torch.from_numpy(rs.randint(0, 256, (C, 84 * 84), dtype=np.uint8)),
                  torch.from_numpy(rs.randint(0, 4, C).astype(np.int32)), torch.from_numpy(rew),
                  torch.from_numpy(term), add_count=C + 77, priorities=rs.uniform(0.1, 2.0, C))
  o = orc.ReplayOracle((1,), 4, C, 32, update_horizon=n)
  o.reward, o.terminal = rew, term
  for _ in range(3):
    a._run_train_op()
    torch.cuda.synchronize()
    t = a._replay.transition
    want = np.array([o.nstep(int(i))[0] for i in t['indices'].cpu().numpy()], np.float32)
    ec.exact('reward', t['reward'].cpu().numpy(), want, 'n = 10')
    assert np.isfinite(a._loss_out['loss'].cpu().numpy()).all()
  assert any(o.nstep(int(i))[2] >= 8 for i in t['indices'].cpu().numpy())
