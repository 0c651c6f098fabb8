"""Inputs shared by tests/test_replay_edges_reference_cpu.py (which proves, with the oracle
alone, that each input has the property it was chosen for) and tests/test_gpu_replay_edges.py
(which runs the device on the same inputs).  Nothing here touches the GPU."""
import random

import numpy as np

from oracle import replay as orc


class Store(object):
  """A whole transition store (what load_arrays takes) plus the buffer geometry."""

  def __init__(self, C, stack, n, add_count, p_term, seed, obs_shape=(1,), obs_dtype=np.uint8):
    rs = np.random.RandomState(seed)
    self.C, self.stack, self.n, self.add_count = C, stack, n, add_count
    self.obs_shape, self.obs_dtype = tuple(obs_shape), np.dtype(obs_dtype)
    if self.obs_dtype == np.uint8:
      self.obs = rs.randint(0, 256, size=(C,) + self.obs_shape).astype(np.uint8)
    else:
      self.obs = rs.randn(*((C,) + self.obs_shape)).astype(obs_dtype)
    self.act = rs.randint(0, 9, size=C).astype(np.int32)
    self.rew = rs.randn(C).astype(np.float32)
    self.term = (rs.rand(C) < p_term).astype(np.uint8) if p_term else np.zeros(C, np.uint8)

  def oracle(self, prioritized=False, B=32, **kw):
    cls = orc.PrioritizedOracle if prioritized else orc.ReplayOracle
    o = cls(self.obs_shape, self.stack, self.C, B, update_horizon=self.n,
            observation_dtype=self.obs_dtype, **kw)
    o.observation, o.action, o.reward, o.terminal = self.obs, self.act, self.rew, self.term
    o.add_count = self.add_count
    o.invalid_range = orc.invalid_range(o.cursor(), self.C, self.stack, self.n)
    return o


def words_between(before, after, limit=1 << 16):
  """How many 32-bit MT19937 words lie between two states of one numpy RandomState stream."""
  twin = np.random.RandomState()
  twin.set_state(before)
  for k in range(limit + 1):
    st = twin.get_state()
    if st[2] == after[2] and np.array_equal(st[1], after[1]):
      return k
    twin.randint(0, 2 ** 32, dtype=np.uint32)
  raise AssertionError('states are more than %d words apart' % limit)


def uniform_words(store, B, seed, max_attempts=1000):
  """(indices or the error text, words consumed) of one oracle sample_index_batch(B)."""
  rng = np.random.RandomState(seed)
  o = store.oracle(False, B, np_rng=rng, max_sample_attempts=max_attempts)
  before = rng.get_state()
  try:
    res = o.sample_index_batch(B)
  except RuntimeError as e:
    res = str(e)
  return res, words_between(before, rng.get_state())


# The uniform sampler evaluates the tape 64 words at a time.  width = max_id - min_id = 33:
# the 6-bit mask rejects almost half of the words.
def window_store():
  return Store(C=39, stack=4, n=3, add_count=39 + 11, p_term=1 / 50., seed=101)


WINDOW_B = 40


def search_window_seeds(limit=4000):
  st, last, first = window_store(), None, None
  for seed in range(limit):
    res, words = uniform_words(st, WINDOW_B, seed)
    if isinstance(res, str):
      continue
    if last is None and words % 64 == 0:
      last = seed
    if first is None and words % 64 == 1 and words > 1:
      first = seed
    if last is not None and first is not None:
      break
  return last, first


# Terminals at 1/5 with stack 4: most draws are invalid, and a small attempts budget runs out.
def attempts_store():
  return Store(C=200, stack=4, n=3, add_count=200 + 77, p_term=1 / 5., seed=102)


ATTEMPTS_B, ATTEMPTS_MAX = 16, 12


def search_attempts_seeds(limit=400):
  """(a seed whose batch fails, a seed whose batch succeeds) under the oracle."""
  st, bad, good = attempts_store(), None, None
  for seed in range(limit):
    res, _ = uniform_words(st, ATTEMPTS_B, seed, ATTEMPTS_MAX)
    if isinstance(res, str) and bad is None:
      bad = seed
    if not isinstance(res, str) and good is None:
      good = seed
    if bad is not None and good is not None:
      break
  return bad, good


GROUPS = 5


def groups_outcome(store, B, G, seed, max_attempts):
  """G consecutive oracle sample_index_batch(B) calls: ([indices per finished group], the
  failing group's error text or None, [words consumed per call], the oracle)."""
  rng = np.random.RandomState(seed)
  o = store.oracle(False, B, np_rng=rng, max_sample_attempts=max_attempts)
  done, words, err = [], [], None
  for _ in range(G):
    before = rng.get_state()
    try:
      done.append(o.sample_index_batch(B))
    except RuntimeError as e:
      err = str(e)
    words.append(words_between(before, rng.get_state()))
    if err:
      break
  return done, err, words, o


def search_group_seed(limit=400):
  """A seed whose first two groups succeed and whose third fails (of GROUPS = 5)."""
  st = attempts_store()
  for seed in range(limit):
    done, err, _, _ = groups_outcome(st, ATTEMPTS_B, GROUPS, seed, ATTEMPTS_MAX)
    if err and len(done) == 2:
      return seed


# Prioritized retry loop (prb:152-170): terminals at 1/20, stack 4, a budget of 3 redraws.
def retry_store():
  return Store(C=600, stack=4, n=3, add_count=600 + 123, p_term=1 / 20., seed=103)


RETRY_B, RETRY_MAX = 32, 3


def retry_leaves(C):
  return np.random.RandomState(104).uniform(0.1, 2.0, C)


def per_outcome(store, leaves, B, seed, max_attempts):
  """('error', text) | ('invalid', indices) | ('ok', indices) of one oracle PER batch."""
  o = store.oracle(True, B, py_rng=random.Random(seed), max_sample_attempts=max_attempts)
  o.sum_tree = orc.SumTree.from_leaves(store.C, leaves)
  try:
    idx = o.sample_index_batch(B)
  except RuntimeError as e:
    return 'error', str(e), o
  kind = 'ok' if all(o.is_valid_transition(i) for i in idx) else 'invalid'
  return kind, idx, o


def search_retry_seeds(limit=3000):
  st, leaves, found = retry_store(), retry_leaves(600), {}
  for seed in range(limit):
    kind = per_outcome(st, leaves, RETRY_B, seed, RETRY_MAX)[0]
    found.setdefault(kind, seed)
    if len(found) == 3:
      break
  return found


# What the searches above found (python -m tests.replay_edge_cases prints them); the CPU test
# asserts that each still has its property.  Window: the B-th accepted draw is word 63 of a
# window (64 words consumed) / word 0 of the next one (65 words consumed).
WINDOW_SEED_LAST_LANE, WINDOW_SEED_FIRST_LANE = 28, 1
ATTEMPTS_SEED_FAILS, ATTEMPTS_SEED_PASSES = 0, 2
RETRY_SEED_ERROR, RETRY_SEED_INVALID, RETRY_SEED_OK = 3, 9, 0
GROUP_SEED_THIRD_FAILS = 17


# --------------------------------------------------------------------------
# tests/golden/replay_horizon.npz (gen_golden.gen_horizon)
# --------------------------------------------------------------------------
HORIZON_KEYS = ['state', 'action', 'reward', 'next_state', 'next_action', 'next_reward',
                'terminal', 'indices']
HORIZON_SNAP_KEYS = ['action', 'reward', 'next_action', 'next_reward', 'terminal', 'indices']
# element cases whose stored reward can show the order of the additions (see gen_golden)
HORIZON_ELEM_ORDER_VISIBLE = ('f64_n9', 'f64_n17')


def horizon_meta(z, name):
  C, n, stack, adds, B, rounds, add_count, seed = [int(x) for x in z[name + '_meta']]
  return dict(C=C, n=n, stack=stack, adds=adds, B=B, rounds=rounds, add_count=add_count,
              seed=seed, prioritized=name.startswith('per'))


def replay_horizon_case(z, name, mem, check):
  """Feeds the case's add stream to ``mem`` (an oracle or a device buffer: same add /
  sample_transition_batch surface).  At every snapshot, at each sampled round and for the
  explicit batch, calls check(key, got, expected, where)."""
  m = horizon_meta(z, name)
  obs, act, rew, term = (z[name + k] for k in ('_obs', '_act', '_rew', '_term'))
  snaps, lens = z[name + '_snaps']
  at = {int(a): i for i, a in enumerate(snaps)}
  offs = np.concatenate([[0], np.cumsum(lens)])
  keys = HORIZON_KEYS + (['probs'] if m['prioritized'] else [])
  for i in range(m['adds']):
    if m['prioritized']:
      mem.add(obs[i], act[i], rew[i], term[i], z[name + '_prio_in'][i])
    else:
      mem.add(obs[i], act[i], rew[i], term[i])
    if i + 1 in at:
      j = at[i + 1]
      idx = [int(x) for x in z[name + '_snap_indices'][offs[j]:offs[j + 1]]]
      batch = mem.sample_transition_batch(batch_size=len(idx), indices=idx)
      for k, v in zip(keys, batch):
        if k in HORIZON_SNAP_KEYS:
          check(k, v, z[name + '_snap_' + k][offs[j]:offs[j + 1]], '%s after %d adds' % (name, i + 1))
  assert int(mem.add_count) == m['add_count']
  for r in range(m['rounds']):
    for k, v in zip(keys, mem.sample_transition_batch()):
      check(k, v, z[name + '_' + k][r], '%s round %d' % (name, r))
  fixed = [int(i) for i in z[name + '_fixed_indices']]
  for k, v in zip(keys, mem.sample_transition_batch(batch_size=len(fixed), indices=fixed)):
    check(k, v, z[name + '_fixed_' + k], name + ' fixed')


def exact(key, got, expected, where):
  got, expected = np.asarray(got), np.asarray(expected)
  assert got.shape == expected.shape, (where, key, got.shape, expected.shape)
  if got.dtype.kind == 'f':     # bit for bit: no tolerance, and the sign of zero counts
    assert got.dtype == expected.dtype, (where, key)
    np.testing.assert_array_equal(got.view('u%d' % got.dtype.itemsize),
                                  expected.view('u%d' % got.dtype.itemsize),
                                  err_msg='%s %s' % (where, key))
  else:
    np.testing.assert_array_equal(got, expected, err_msg='%s %s' % (where, key))


if __name__ == '__main__':
  print('window', search_window_seeds())
  print('attempts', search_attempts_seeds())
  print('retry', search_retry_seeds())
  print('group', search_group_seed())
