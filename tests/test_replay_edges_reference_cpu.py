"""The CPU side of tests/test_gpu_replay_edges.py: the oracle alone against the reference's
own long-horizon vectors, the restated np.sum order against the installed numpy, and proof
that every hand-picked input of the device tests has the property it was picked for.

np.sum(discount[:L] * rewards) (circular_replay_buffer.py:540-541) adds a contiguous 1-D array
of 8 or more elements pairwise.  A left-to-right restatement -- what the oracle and the
kernels did before -- is right below 8 elements only; tests/golden/replay_horizon.npz
(gen_golden.gen_horizon) tells the two orders apart, and this file shows that it does.

Three element cases cannot show the order and are only checked bit for bit: a float16 reward
is the float32 sum rounded to 11 bits and an int32 reward the float64 sum truncated, which
hide a last-bit difference (0 of 80 recorded rewards differ for each), and a shaped (9,)
reward is summed row by row, which IS left to right."""
import random

import numpy as np
import pytest

from oracle import replay as orc
from tests import replay_edge_cases as ec
from tests.test_oracle_golden import SHAPE_KEYS, shape_case

HORIZON = 'replay_horizon.npz'


def _cases(kind):
  return ['%s_n%d_s%d' % (kind, n, s) for n in (7, 8, 9, 17, 64, 65, 137) for s in (1, 4)]


def _oracle(z, name, sum_order=None):
  m = ec.horizon_meta(z, name)
  cls = orc.PrioritizedOracle if m['prioritized'] else orc.ReplayOracle
  py_rng, np_rng = random.Random(m['seed']), np.random.RandomState(m['seed'])
  mem = cls((2, 2), m['stack'], m['C'], m['B'], update_horizon=m['n'], gamma=float(z['gamma']),
            py_rng=py_rng, np_rng=np_rng)
  if sum_order is not None:
    mem.sum_order = sum_order
  return mem


def test_horizon_file_lists_every_case(golden):
  z = golden(HORIZON)
  assert [str(c) for c in z['cases']] == _cases('uni') + _cases('per')
  assert [str(c) for c in z['elem_cases']] == ['f64_n9', 'f64_n17', 'f16_n9', 'f16_n17',
                                               'i32_n9', 'i32_n17', 'shaped_n9']


@pytest.mark.parametrize('name', _cases('uni') + _cases('per'))
def test_oracle_matches_horizon_golden(golden, name):
  z = golden(HORIZON)
  ec.replay_horizon_case(z, name, _oracle(z, name), ec.exact)


@pytest.mark.parametrize('name', _cases('uni') + _cases('per'))
def test_left_to_right_restatement_fails_from_horizon_8(golden, name):
  """The fixture can tell the two orders apart: with the old left-to-right sum at least a
  quarter of the recorded rewards of every n >= 8 case come out wrong, every other element
  still matches, and n = 7 passes whole."""
  z = golden(HORIZON)
  n = ec.horizon_meta(z, name)['n']
  wrong, total = [0], [0]

  def check(key, got, expected, where):
    if key == 'reward' and 'after' in where:
      wrong[0] += int(np.sum(np.asarray(got).view(np.uint32) != expected.view(np.uint32)))
      total[0] += len(expected)
    elif key != 'reward':
      ec.exact(key, got, expected, where)

  ec.replay_horizon_case(z, name, _oracle(z, name, orc.sum_left_to_right), check)
  assert total[0] >= 200
  if n < 8:
    assert wrong[0] == 0
  else:
    assert wrong[0] >= total[0] / 4., (wrong[0], total[0])


@pytest.mark.parametrize('name', _cases('uni') + _cases('per'))
def test_horizon_case_covers_its_edges(golden, name):
  """From the fixture's own data: trajectories with a terminal at the first step, at the
  n-th step and absent; lengths spread over 1..n; a trajectory that wraps the ring end; one
  whose idx + L differs from idx + n (next_action / next_reward re-read)."""
  z = golden(HORIZON)
  m = ec.horizon_meta(z, name)
  C, n = m['C'], m['n']
  o = _oracle(z, name)
  seen = dict(first=0, last=0, absent=0, wraps=0, reread=0)
  lens = set()

  def check(key, got, expected, where):
    if key != 'indices' or 'after' not in where:
      return
    for idx in expected:
      _, term, L = o.nstep(int(idx))
      lens.add(L)
      seen['first'] += term and L == 1
      seen['last'] += term and L == n
      seen['absent'] += not term
      seen['wraps'] += int(idx) + L >= C
      seen['reread'] += L != n

  ec.replay_horizon_case(z, name, o, check)
  assert all(v > 0 for v in seen.values()), seen
  assert min(lens) == 1 and max(lens) == n and len(lens) >= min(n, 12)
  assert seen['absent'] >= 0.2 * sum(z[name + '_snaps'][1])


def test_horizon_element_cases(golden):
  """Scalar float64 / float16 / int32 rewards at n = 9 and 17 and a shaped (9,) float32 one,
  through the oracle; the float64 cases differ from the left-to-right float64 sum in at
  least a quarter of their rewards."""
  z = golden(HORIZON)
  for name in [str(c) for c in z['elem_cases']]:
    pre = 'elem_' + name
    kw, adds, rounds = shape_case(z, pre)
    mem = orc.ReplayOracle(kw['observation_shape'], kw['stack_size'], kw['replay_capacity'],
                           kw['batch_size'], update_horizon=kw['update_horizon'],
                           gamma=kw['gamma'], np_rng=np.random.RandomState(int(z[pre + '_seed'])),
                           action_dtype=kw['action_dtype'], reward_shape=kw['reward_shape'],
                           reward_dtype=kw['reward_dtype'])
    for i in range(adds):
      mem.add(z[pre + '_obs'][i], z[pre + '_act'][i], z[pre + '_rew'][i], z[pre + '_term'][i])
    for r in range(rounds):
      for k, v in zip(SHAPE_KEYS, mem.sample_transition_batch()):
        ec.exact(k, v, z[pre + '_' + k][r], '%s round %d' % (pre, r))
    fixed = [int(i) for i in z[pre + '_fixed_indices']]
    for k, v in zip(SHAPE_KEYS, mem.sample_transition_batch(len(fixed), indices=fixed)):
      ec.exact(k, v, z[pre + '_fixed_' + k], pre + ' fixed')
    if name in ec.HORIZON_ELEM_ORDER_VISIBLE:
      idx = np.concatenate([z[pre + '_indices'].reshape(-1), z[pre + '_fixed_indices']])
      got = np.concatenate([z[pre + '_reward'].reshape(-1), z[pre + '_fixed_reward']])
      l2r = []
      for i in idx:
        _, _, L = mem.nstep(int(i))
        l2r.append(orc.sum_left_to_right(mem.discount[:L] * mem.reward[mem._ring(int(i), L)]))
      l2r = np.array(l2r)
      assert l2r.dtype == np.float64 and got.dtype == np.float64
      assert np.mean(got != l2r) >= 0.25


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_restated_sum_order_is_numpys(dtype):
  """numpy_sum_order against np.sum of the installed numpy for every length 1..300, and the
  left-to-right order against it: equal below 8 elements, different from 8 on."""
  rs = np.random.RandomState(8)
  for L in range(1, 301):
    x = rs.randn(40, L).astype(dtype)
    differ = 0
    for row in x:
      want = np.sum(row)
      assert want.dtype == dtype
      assert orc.numpy_sum_order(row) == want, L
      differ += orc.sum_left_to_right(row) != want
    assert (differ == 0) if L < 8 else (differ > 0), (L, differ)


def test_uniform_window_seeds():
  """The B-th accepted draw falls on the last word of a 64-word window for one seed and on
  the first word of the next window for the other (the oracle's word count)."""
  st = ec.window_store()
  o = st.oracle()
  lo, hi = o._id_range()
  assert hi - lo == 33
  res, words = ec.uniform_words(st, ec.WINDOW_B, ec.WINDOW_SEED_LAST_LANE)
  assert len(res) == ec.WINDOW_B and words == 64
  res, words = ec.uniform_words(st, ec.WINDOW_B, ec.WINDOW_SEED_FIRST_LANE)
  assert len(res) == ec.WINDOW_B and words == 65


def test_uniform_attempts_seeds():
  st = ec.attempts_store()
  res, _ = ec.uniform_words(st, ec.ATTEMPTS_B, ec.ATTEMPTS_SEED_FAILS, ec.ATTEMPTS_MAX)
  assert res == ('Max sample attempts: Tried 12 times but only sampled 9 valid indices. '
                 'Batch size is 16')
  res, _ = ec.uniform_words(st, ec.ATTEMPTS_B, ec.ATTEMPTS_SEED_PASSES, ec.ATTEMPTS_MAX)
  assert len(res) == ec.ATTEMPTS_B


def test_prioritized_retry_seeds():
  """Budget 3: one seed runs out on a later stratum (the reference's error, 25 sampled), one
  on the last invalid stratum (an invalid index is returned), one never runs out."""
  st, leaves = ec.retry_store(), ec.retry_leaves(600)
  kind, text, _ = ec.per_outcome(st, leaves, ec.RETRY_B, ec.RETRY_SEED_ERROR, ec.RETRY_MAX)
  assert kind == 'error' and text == ('Max sample attempts: Tried 3 times but only sampled 25 '
                                      'valid indices. Batch size is 32')
  kind, idx, o = ec.per_outcome(st, leaves, ec.RETRY_B, ec.RETRY_SEED_INVALID, ec.RETRY_MAX)
  assert kind == 'invalid' and sum(not o.is_valid_transition(i) for i in idx) == 1
  assert ec.per_outcome(st, leaves, ec.RETRY_B, ec.RETRY_SEED_OK, ec.RETRY_MAX)[0] == 'ok'


def test_group_seed():
  """Of five consecutive batches the first two succeed and the third runs out of attempts."""
  done, err, words, _ = ec.groups_outcome(ec.attempts_store(), ec.ATTEMPTS_B, ec.GROUPS,
                                          ec.GROUP_SEED_THIRD_FAILS, ec.ATTEMPTS_MAX)
  assert len(done) == 2 and len(words) == 3
  assert err.startswith('Max sample attempts: Tried 12 times but only sampled ')
