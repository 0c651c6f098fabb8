"""Generate golden replay vectors by running the REFERENCE's own code.

Runs only in the build container (needs /root/reference, never on the GPU box).
The reference's replay modules are imported from their files; the only
stand-ins are for non-algorithmic imports that are absent here:
``tensorflow`` (only ``tf.logging.info`` is touched by the code paths used)
and ``gin`` / ``gin.tf`` (``@gin.configurable`` treated as identity).

Outputs: tests/golden/{sumtree,replay_uniform,replay_per,replay_shapes,replay_horizon}.npz
and the two checkpoints -- inputs and
reference outputs only (data, no reference source).

    python tests/golden/gen_golden.py
"""
import importlib.util
import os
import random
import sys
import types

import numpy as np

REF = '/root/reference/dopamine/replay_memory'
OUT = os.path.dirname(os.path.abspath(__file__))


def _load_reference():
  tf = types.ModuleType('tensorflow')
  tf.logging = types.SimpleNamespace(info=lambda *a, **k: None, warning=lambda *a, **k: None)
  gin = types.ModuleType('gin')
  gin.configurable = lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))
  gin_tf = types.ModuleType('gin.tf')
  gin.tf = gin_tf
  for name, mod in (('tensorflow', tf), ('gin', gin), ('gin.tf', gin_tf)):
    sys.modules.setdefault(name, mod)
  pkg = types.ModuleType('dopamine'); pkg.__path__ = []
  sub = types.ModuleType('dopamine.replay_memory'); sub.__path__ = []
  sys.modules.setdefault('dopamine', pkg)
  sys.modules.setdefault('dopamine.replay_memory', sub)
  mods = {}
  for name in ('sum_tree', 'circular_replay_buffer', 'prioritized_replay_buffer'):
    spec = importlib.util.spec_from_file_location('dopamine.replay_memory.' + name,
                                                  os.path.join(REF, name + '.py'))
    m = importlib.util.module_from_spec(spec)
    sys.modules['dopamine.replay_memory.' + name] = m
    setattr(sub, name, m)
    spec.loader.exec_module(m)
    mods[name] = m
  return mods


def _pystate_words():
  st = random.getstate()[1]
  return np.array(st, dtype=np.int64)  # 624 words + position


def gen_sumtree(m):
  st_mod = m['sum_tree']
  out = {}
  rs = np.random.RandomState(7)
  caps = [1, 2, 3, 5, 100, 1000, 1025, 4096]
  out['capacities'] = np.array(caps)
  for c in caps:
    tree = st_mod.SumTree(c)
    nset = 3 * c + 5
    idx = rs.randint(0, c, size=nset).astype(np.int32)
    val = rs.uniform(0.0, 3.0, size=nset).astype(np.float32)
    val[rs.rand(nset) < 0.1] = 0.0
    for i, v in zip(idx, val):
      tree.set(int(i), v)
    out['c%d_set_idx' % c] = idx
    out['c%d_set_val' % c] = val
    out['c%d_nodes' % c] = np.concatenate(tree.nodes)
    out['c%d_maxrec' % c] = np.float64(tree.max_recorded_priority)
    for b in (1, 7, 32):
      random.seed(1000 + c + b)
      out['c%d_strat%d' % (c, b)] = np.array(tree.stratified_sample(b), np.int64)
      out['c%d_strat%d_state' % (c, b)] = _pystate_words()
    random.seed(99 + c)
    out['c%d_single' % c] = np.array([tree.sample() for _ in range(10)], np.int64)
    out['c%d_query' % c] = np.array([tree.sample(query_value=q) for q in (0.0, 0.25, 0.5, 0.999, 1.0)], np.int64)
  np.savez_compressed(os.path.join(OUT, 'sumtree.npz'), **out)


def _stream(rs, n, obs_shape, p_term, nA):
  obs = rs.randint(0, 256, size=(n,) + obs_shape).astype(np.uint8)
  act = rs.randint(0, nA, size=n).astype(np.int32)
  rew = rs.choice(np.array([-1.0, 0.0, 1.0, 0.5], np.float32), size=n)
  term = (rs.rand(n) < p_term).astype(np.uint8)
  return obs, act, rew, term


def gen_replay(m, prioritized):
  crb = m['circular_replay_buffer']
  prb = m['prioritized_replay_buffer']
  out = {}
  cases = [  # (name, capacity, n, stack, adds, gamma, B, rounds)
      ('full_n1', 200, 1, 4, 537, 0.99, 32, 12),
      ('full_n3', 200, 3, 4, 611, 0.99, 32, 12),
      ('part_n3', 300, 3, 4, 90, 0.9, 16, 8),
      ('full_n5_s1', 50, 5, 1, 173, 0.97, 8, 10),
  ]
  out['cases'] = np.array([c[0] for c in cases])
  rs = np.random.RandomState(11 if prioritized else 13)
  for name, C, n, stack, adds, gamma, B, rounds in cases:
    obs_shape = (8, 8)
    obs, act, rew, term = _stream(rs, adds, obs_shape, 0.06, 6)
    cls = prb.OutOfGraphPrioritizedReplayBuffer if prioritized else crb.OutOfGraphReplayBuffer
    mem = cls(observation_shape=obs_shape, stack_size=stack, replay_capacity=C,
              batch_size=B, update_horizon=n, gamma=gamma)
    prio_in = rs.uniform(0.05, 2.0, size=adds).astype(np.float32)
    for i in range(adds):
      if prioritized:
        mem.add(obs[i], act[i], rew[i], term[i], prio_in[i])
      else:
        mem.add(obs[i], act[i], rew[i], term[i])
    meta = np.array([C, n, stack, adds, B, rounds], np.int64)
    pre = '%s_' % name
    out[pre + 'meta'] = meta
    out[pre + 'gamma'] = np.float64(gamma)
    out[pre + 'obs'] = obs
    out[pre + 'act'] = act
    out[pre + 'rew'] = rew
    out[pre + 'term'] = term
    if prioritized:
      out[pre + 'prio_in'] = prio_in
    out[pre + 'add_count'] = np.int64(mem.add_count)
    seed = 4242 + C
    if prioritized:
      random.seed(seed)
    else:
      np.random.seed(seed)
    out[pre + 'seed'] = np.int64(seed)
    keys = ['state', 'action', 'reward', 'next_state', 'next_action', 'next_reward',
            'terminal', 'indices'] + (['probs'] if prioritized else [])
    rows = {k: [] for k in keys}
    upd_idx, upd_val = [], []
    for r in range(rounds):
      batch = mem.sample_transition_batch()
      for k, v in zip(keys, batch):
        rows[k].append(np.array(v))
      if prioritized:
        # set_priority with a few duplicate indices, as the agent would do with
        # sqrt(loss + 1e-10) (rainbow_agent.py:289-290).
        ind = np.array(batch[7], np.int32).copy()
        if B > 2:
          ind[-1] = ind[0]
        pv = rs.uniform(0.01, 3.0, size=B).astype(np.float32)
        mem.set_priority(ind, pv)
        upd_idx.append(ind)
        upd_val.append(pv)
    for k in keys:
      out[pre + k] = np.stack(rows[k])
    if prioritized:
      out[pre + 'upd_idx'] = np.stack(upd_idx)
      out[pre + 'upd_val'] = np.stack(upd_val)
      out[pre + 'nodes'] = np.concatenate(mem.sum_tree.nodes)
      out[pre + 'maxrec'] = np.float64(mem.sum_tree.max_recorded_priority)
      out[pre + 'rng_state'] = _pystate_words()
    else:
      out[pre + 'rng_state'] = np.array(np.random.get_state()[1], np.int64)
      out[pre + 'rng_pos'] = np.int64(np.random.get_state()[2])
    # explicit-index KAT on the final memory (crb:510 `indices` argument)
    fixed = [i for i in range(C) if mem.is_valid_transition(i)][:5]
    out[pre + 'valid_mask'] = np.array([mem.is_valid_transition(i) for i in range(-2, C + 2)], np.uint8)
    fb = mem.sample_transition_batch(batch_size=len(fixed), indices=fixed)
    for k, v in zip(keys, fb):
      out[pre + 'fixed_' + k] = np.array(v)
  fname = 'replay_per.npz' if prioritized else 'replay_uniform.npz'
  np.savez_compressed(os.path.join(OUT, fname), **out)


def gen_checkpoint(m):
  """A checkpoint WRITTEN BY THE REFERENCE's OutOfGraphReplayBuffer.save
  (crb:612-657) for a small wrapped uniform buffer -- its members are all numpy
  arrays, so every file is np.save data (no pickle) -- plus what the reference
  samples after loading it (np.random.seed(13))."""
  import shutil
  crb = m['circular_replay_buffer']
  tf = sys.modules['tensorflow']
  tf.gfile = types.SimpleNamespace(Exists=os.path.exists, Open=open, Remove=os.remove)
  tf.errors = types.SimpleNamespace(NotFoundError=FileNotFoundError)
  kw = dict(observation_shape=(6, 6), stack_size=4, replay_capacity=40, batch_size=4,
            update_horizon=2, gamma=0.9)
  mem = crb.OutOfGraphReplayBuffer(**kw)
  rs = np.random.RandomState(5)
  for i in range(57):
    mem.add(rs.randint(0, 256, (6, 6)).astype(np.uint8), int(rs.randint(0, 5)),
            float(rs.randn()), bool(i % 13 == 12))
  d = os.path.join(OUT, 'ckpt_uniform')
  shutil.rmtree(d, ignore_errors=True)
  os.makedirs(d)
  mem.save(d, 7)
  fresh = crb.OutOfGraphReplayBuffer(**kw)
  fresh.load(d, 7)
  np.random.seed(13)
  batch = fresh.sample_transition_batch(batch_size=4)
  names = [e.name for e in fresh.get_transition_elements(4)]
  np.savez_compressed(os.path.join(OUT, 'ckpt_uniform_expected.npz'),
                      **{n: np.asarray(v) for n, v in zip(names, batch)})


def gen_checkpoint_per(m):
  """A prioritized checkpoint written by the reference's save (crb:612-657 via
  prb:36-252): the `sum_tree` member is the reference's pickled SumTree object.  Plus
  what the reference samples after loading it (random.seed(17)).  The test loads it
  through a restricted unpickler (classes whitelisted, nothing else executes)."""
  import shutil
  prb = m['prioritized_replay_buffer']
  tf = sys.modules['tensorflow']
  tf.gfile = types.SimpleNamespace(Exists=os.path.exists, Open=open, Remove=os.remove)
  tf.errors = types.SimpleNamespace(NotFoundError=FileNotFoundError)
  kw = dict(observation_shape=(6, 6), stack_size=4, replay_capacity=40, batch_size=4,
            update_horizon=3, gamma=0.9)
  mem = prb.OutOfGraphPrioritizedReplayBuffer(**kw)
  rs = np.random.RandomState(6)
  for i in range(61):
    mem.add(rs.randint(0, 256, (6, 6)).astype(np.uint8), int(rs.randint(0, 5)),
            float(rs.randn()), bool(i % 11 == 10), np.float32(rs.uniform(0.1, 2.0)))
  mem.set_priority(np.array([5, 9, 5, 30], np.int32), np.array([0.3, 2.5, 0.7, 1.1], np.float32))
  d = os.path.join(OUT, 'ckpt_per')
  shutil.rmtree(d, ignore_errors=True)
  os.makedirs(d)
  mem.save(d, 3)
  fresh = prb.OutOfGraphPrioritizedReplayBuffer(**kw)
  fresh.load(d, 3)
  random.seed(17)
  batch = fresh.sample_transition_batch(batch_size=4)
  names = [e.name for e in fresh.get_transition_elements(4)]
  out = {n: np.asarray(v) for n, v in zip(names, batch)}
  out['nodes'] = np.concatenate(fresh.sum_tree.nodes)
  out['maxrec'] = np.float64(fresh.sum_tree.max_recorded_priority)
  out['rng_state'] = _pystate_words()
  np.savez_compressed(os.path.join(OUT, 'ckpt_per_expected.npz'), **out)


# (name, capacity, n, stack, adds, gamma, B, rounds, action (shape, dtype), reward (shape, dtype))
SHAPE_CASES = [
    ('a', 40, 1, 2, 97, 0.9, 6, 5, ((2,), 'int8'), ((3,), 'float32')),
    ('b', 40, 3, 2, 101, 0.9, 6, 0, ((), 'int64'), ((3,), 'float64')),
    ('c', 40, 3, 1, 89, 0.95, 5, 4, ((2, 2), 'float32'), ((), 'float64')),
    ('d', 40, 3, 2, 77, 0.9, 5, 4, ((), 'int32'), ((), 'int32')),
    ('e', 40, 1, 2, 66, 0.8, 4, 4, ((), 'uint8'), ((2, 3), 'float16')),
]


def gen_shapes(m):
    """Non-scalar / non-default action and reward elements (crb:96-183, 530-548): sampled
    batches (np.random, rounds > 0), an explicit-index batch over indices whose n-step
    length broadcasts, and for case b one index whose length does not (numpy's error)."""
    out = {'cases': np.array([c[0] for c in SHAPE_CASES])}
    _shape_cases(m, SHAPE_CASES, np.random.RandomState(21), out)
    np.savez_compressed(os.path.join(OUT, 'replay_shapes.npz'), **out)


def _shape_cases(m, cases, rs, out, prefix='', p_term=0.12, rewards=None, patterned=False):
    """The cases of gen_shapes into ``out``; ``rewards(rs, shape, dtype)`` replaces the
    default small-multiple rewards (the long-horizon cases need rewards whose sum depends on
    the order of the additions)."""
    crb = m['circular_replay_buffer']
    for name, C, n, stack, adds, gamma, B, rounds, (ash, adt), (rsh, rdt) in cases:
        mem = crb.OutOfGraphReplayBuffer(observation_shape=(4, 4), stack_size=stack,
                                         replay_capacity=C, batch_size=B, update_horizon=n,
                                         gamma=gamma, action_shape=ash, action_dtype=np.dtype(adt),
                                         reward_shape=rsh, reward_dtype=np.dtype(rdt))
        obs = rs.randint(0, 256, (adds, 4, 4)).astype(np.uint8)
        if patterned:    # frame i = the bytes 16i .. 16i + 15 (mod 256): a small file
            obs = ((16 * np.arange(adds)[:, None, None] + np.arange(16).reshape(4, 4)) % 256).astype(np.uint8)
        act = rs.randint(-3, 100, (adds,) + ash).astype(adt)
        if rewards is None:
            rew = (rs.randint(-4, 5, (adds,) + rsh) * 0.37).astype(rdt)
        else:
            rew = rewards(rs, (adds,) + rsh, rdt)
        term = (rs.rand(adds) < p_term).astype(np.uint8)
        for i in range(adds):
            mem.add(obs[i], act[i], rew[i], term[i])
        pre = prefix + name + '_'
        out[pre + 'meta'] = np.array([C, n, stack, adds, B, rounds], np.int64)
        out[pre + 'gamma'] = np.float64(gamma)
        out[pre + 'obs'], out[pre + 'act'], out[pre + 'rew'], out[pre + 'term'] = obs, act, rew, term
        keys = ['state', 'action', 'reward', 'next_state', 'next_action', 'next_reward',
                'terminal', 'indices']
        np.random.seed(500 + C + n)
        out[pre + 'seed'] = np.int64(500 + C + n)
        rows = {k: [] for k in keys}
        for _ in range(rounds):
            for k, v in zip(keys, mem.sample_transition_batch()):
                rows[k].append(np.array(v))
        for k in keys:
            if rounds:
                out[pre + k] = np.stack(rows[k])
        traj_len = {}
        for i in range(C):
            if mem.is_valid_transition(i):
                t = mem._store['terminal'][[(i + j) % C for j in range(n)]]
                traj_len[i] = int(np.argmax(t.astype(bool))) + 1 if t.any() else n
        m_last = rsh[-1] if rsh else 0
        ok = [i for i, L in sorted(traj_len.items()) if not m_last or L in (m_last, 1)]
        fixed = ok[:B]
        out[pre + 'fixed_indices'] = np.array(fixed, np.int64)
        for k, v in zip(keys, mem.sample_transition_batch(batch_size=len(fixed), indices=fixed)):
            out[pre + 'fixed_' + k] = np.array(v)
        bad = [i for i, L in sorted(traj_len.items()) if m_last and L not in (m_last, 1)]
        if bad:
            try:
                mem.sample_transition_batch(batch_size=1, indices=[bad[0]])
                out[pre + 'bad_error'] = np.array('')
            except ValueError as e:
                out[pre + 'bad_error'] = np.array(str(e))
            out[pre + 'bad_index'] = np.int64(bad[0])


# --------------------------------------------------------------------------
# Long update horizons (replay_horizon.npz): np.sum(discount[:L] * rewards) (crb:540-541)
# adds a contiguous 1-D array of 8 or more elements pairwise, not left to right, so the
# n-step reward's last bits depend on the order from n = 8 on.  Rewards are randn float32
# (the {-1, 0, 0.5, 1} set of gen_replay sums exactly in any order).
# --------------------------------------------------------------------------
HORIZONS = (7, 8, 9, 17, 64, 65, 137)
HORIZON_STACKS = (1, 4)
HORIZON_KEYS = ['state', 'action', 'reward', 'next_state', 'next_action', 'next_reward',
                'terminal', 'indices']
HORIZON_SNAP_KEYS = ['action', 'reward', 'next_action', 'next_reward', 'terminal', 'indices']

# (name, capacity, n, stack, adds, gamma, B, rounds, action (shape, dtype), reward (shape, dtype))
HORIZON_ELEM_CASES = [
    ('f64_n9', 60, 9, 2, 171, 0.99, 16, 4, ((), 'int32'), ((), 'float64')),
    ('f64_n17', 70, 17, 2, 190, 0.99, 16, 4, ((), 'int32'), ((), 'float64')),
    ('f16_n9', 60, 9, 2, 171, 0.99, 16, 4, ((), 'int32'), ((), 'float16')),
    ('f16_n17', 70, 17, 1, 190, 0.99, 16, 4, ((), 'int32'), ((), 'float16')),
    ('i32_n9', 60, 9, 2, 171, 0.99, 16, 4, ((), 'int32'), ((), 'int32')),
    ('i32_n17', 70, 17, 2, 190, 0.99, 16, 4, ((), 'int32'), ((), 'int32')),
    ('shaped_n9', 60, 9, 2, 171, 0.99, 16, 4, ((), 'int32'), ((9,), 'float32')),
]
# the element cases whose stored reward can show the order of the additions: a float16 or
# int32 reward is the float32 / float64 sum rounded to 11 bits / truncated to an integer,
# which hides a last-bit difference, and a shaped reward is summed row by row (left to right)
HORIZON_ELEM_ORDER_VISIBLE = ('f64_n9', 'f64_n17')


def _horizon_rewards(rs, shape, dtype):
  if np.dtype(dtype).kind == 'i':
    return rs.randint(-1000, 1001, shape).astype(dtype)
  return rs.randn(*shape).astype(dtype)


def left_to_right_rewards(store_reward, store_terminal, discount, C, n, indices):
  """The n-step rewards of ``indices`` with the products of crb:540-541 added LEFT TO RIGHT in
  their own type (float32 for a float32 store, numpy's promotion otherwise) -- what the
  goldens of a horizon >= 8 must differ from -- and each trajectory's length."""
  out, lens = [], []
  for idx in indices:
    ring = [(int(idx) + j) % C for j in range(n)]
    t = store_terminal[ring].astype(bool)
    L = int(np.argmax(t)) + 1 if t.any() else n
    prod = discount[:L] * store_reward[ring[:L]]
    acc = prod.dtype.type(0)
    for v in prod:
      acc = prod.dtype.type(acc + v)
    out.append(acc)
    lens.append(L)
  return np.array(out), np.array(lens)


def gen_horizon(m):
  """Uniform and prioritized buffers at update horizons 7 .. 137, stack 1 and 4, (2, 2) uint8
  observations, capacity n + stack + 40: sampled rounds and an explicit-index batch as in
  gen_replay, plus explicit batches over EVERY valid index at several points of the add
  stream (``snap_*``, scalars only), so trajectories of every length, with a terminal at the
  first step, at the last step and absent, wrapping the ring end, are recorded.  Then the
  scalar-reward element cases (float64 / float16 / int32, n = 9 and 17) and one shaped (9,)
  float32 reward, in gen_shapes style."""
  crb = m['circular_replay_buffer']
  prb = m['prioritized_replay_buffer']
  out = {}
  names = []
  for prioritized in (False, True):
    rs = np.random.RandomState(31 if prioritized else 37)
    for n in HORIZONS:
      for stack in HORIZON_STACKS:
        name = '%s_n%d_s%d' % ('per' if prioritized else 'uni', n, stack)
        names.append(name)
        C, B, rounds, gamma = n + stack + 40, 8, 3, 0.99
        adds = 3 * C + 7
        # frame i holds the bytes 4i .. 4i + 3 (mod 256): every frame of a stack differs, and
        # the file stays small
        obs = ((4 * np.arange(adds)[:, None, None] + np.arange(4).reshape(2, 2)) % 256).astype(np.uint8)
        # the terminals are re-drawn (same stream) until the case shows what it is for
        for attempt in range(100):
          act = rs.randint(0, 6, size=adds).astype(np.int32)
          rew = rs.randn(adds).astype(np.float32)
          term = (rs.rand(adds) < 1.0 / (3 * n + 60)).astype(np.uint8)
          # two terminals placed so that, at the last snapshot, one trajectory ends at its
          # first step and one at its n-th
          term[adds - n - 16:adds] = 0
          term[adds - n - 12] = 1
          term[adds - 2] = 1
          prio_in = (rs.randint(1, 41, size=adds) / 20.0).astype(np.float32)
          cls = prb.OutOfGraphPrioritizedReplayBuffer if prioritized else crb.OutOfGraphReplayBuffer
          mem = cls(observation_shape=(2, 2), stack_size=stack, replay_capacity=C, batch_size=B,
                    update_horizon=n, gamma=gamma)
          snaps = sorted(set([C + 3, C + C // 3, 2 * C - 5, 2 * C + 5, adds - 9, adds]))
          keys = HORIZON_KEYS + (['probs'] if prioritized else [])
          snap_rows = {k: [] for k in HORIZON_SNAP_KEYS}
          snap_len, l2r, lens = [], [], []
          for i in range(adds):
            if prioritized:
              mem.add(obs[i], act[i], rew[i], term[i], prio_in[i])
            else:
              mem.add(obs[i], act[i], rew[i], term[i])
            if i + 1 in snaps:
              valid = [j for j in range(C) if mem.is_valid_transition(j)]
              batch = mem.sample_transition_batch(batch_size=len(valid), indices=valid)
              for k, v in zip(keys, batch):
                if k in snap_rows:
                  snap_rows[k].append(np.array(v))
              snap_len.append(len(valid))
              a, b = left_to_right_rewards(mem._store['reward'], mem._store['terminal'],
                                           mem._cumulative_discount_vector, C, n, valid)
              l2r.append(a)
              lens.append(b)
          pre = name + '_'
          seed = 977 + C
          out[pre + 'meta'] = np.array([C, n, stack, adds, B, rounds, int(mem.add_count), seed],
                                       np.int64)
          out[pre + 'obs'], out[pre + 'act'], out[pre + 'rew'], out[pre + 'term'] = obs, act, rew, term
          if prioritized:
            out[pre + 'prio_in'] = prio_in
          out[pre + 'snaps'] = np.array([snaps, snap_len], np.int64)   # add counts, batch sizes
          for k in HORIZON_SNAP_KEYS:
            out[pre + 'snap_' + k] = np.concatenate(snap_rows[k])
          random.seed(seed) if prioritized else np.random.seed(seed)
          rows = {k: [] for k in keys}
          for _ in range(rounds):
            for k, v in zip(keys, mem.sample_transition_batch()):
              rows[k].append(np.array(v))
          for k in keys:
            out[pre + k] = np.stack(rows[k])
          fixed = [i for i in range(C) if mem.is_valid_transition(i)][:5]
          for k, v in zip(keys, mem.sample_transition_batch(batch_size=len(fixed), indices=fixed)):
            out[pre + 'fixed_' + k] = np.array(v)
          # what the fixture must be able to show
          got, l2r, lens = out[pre + 'snap_reward'], np.concatenate(l2r), np.concatenate(lens)
          terms = out[pre + 'snap_terminal'].astype(bool)
          assert got.dtype == np.float32 and l2r.dtype == np.float32
          differ = float(np.mean(got != l2r))
          print('%-14s C %3d  %4d trajectories  L %3d..%3d  no terminal %.2f  differ from '
                'left-to-right %.3f' % (name, C, len(got), lens.min(), lens.max(),
                                        np.mean(~terms), differ))
          assert n >= 8 or differ == 0.0, (name, differ)
          if ((n < 8 or differ >= 0.25) and (terms & (lens == 1)).any() and
              (terms & (lens == n)).any() and np.mean(~terms) >= 0.3 and
              len(set(lens.tolist())) >= min(n, 12)):
            break
        else:
          raise AssertionError(name)
  out['cases'] = np.array(names)
  out['gamma'] = np.float64(0.99)
  out['elem_cases'] = np.array([c[0] for c in HORIZON_ELEM_CASES])
  _shape_cases(m, HORIZON_ELEM_CASES, np.random.RandomState(41), out, prefix='elem_',
               p_term=0.02, rewards=_horizon_rewards, patterned=True)
  for name, C, n, stack, adds, gamma, B, rounds, _, (rsh, rdt) in HORIZON_ELEM_CASES:
    pre = 'elem_' + name + '_'
    # the store after the adds, as the reference pads it (crb:234-260)
    mem = crb.OutOfGraphReplayBuffer(observation_shape=(4, 4), stack_size=stack,
                                     replay_capacity=C, batch_size=B, update_horizon=n,
                                     gamma=gamma, reward_shape=rsh, reward_dtype=np.dtype(rdt))
    for i in range(adds):
      mem.add(out[pre + 'obs'][i], out[pre + 'act'][i], out[pre + 'rew'][i], out[pre + 'term'][i])
    if rsh:
      continue
    idx = np.concatenate([out[pre + 'indices'].reshape(-1), out[pre + 'fixed_indices']])
    got = np.concatenate([out[pre + 'reward'].reshape(-1), out[pre + 'fixed_reward']])
    l2r, _ = left_to_right_rewards(mem._store['reward'], mem._store['terminal'],
                                   mem._cumulative_discount_vector, C, n, idx)
    differ = float(np.mean(got != l2r.astype(rdt)))
    print('elem_%-10s %3d rewards  differ from left-to-right %.3f' % (name, len(got), differ))
    if name in HORIZON_ELEM_ORDER_VISIBLE:
      assert l2r.dtype == np.float64 and differ >= 0.25, (name, differ)
  np.savez_compressed(os.path.join(OUT, 'replay_horizon.npz'), **out)


if __name__ == '__main__':
  mods = _load_reference()
  if sys.argv[1:] == ['ckpt_per']:
    gen_checkpoint_per(mods)
    sys.exit(0)
  if sys.argv[1:] == ['shapes']:
    gen_shapes(mods)
    sys.exit(0)
  if sys.argv[1:] == ['horizon']:
    gen_horizon(mods)
    sys.exit(0)
  gen_sumtree(mods)
  gen_replay(mods, prioritized=False)
  gen_replay(mods, prioritized=True)
  gen_checkpoint(mods)
  gen_checkpoint_per(mods)
  gen_shapes(mods)
  gen_horizon(mods)
  for f in sorted(os.listdir(OUT)):
    if f.endswith('.npz'):
      print(f, os.path.getsize(os.path.join(OUT, f)))
