"""bench.py's command line: a plain run times the headline only (--full adds the rest), and
--dump-outputs writes the learner's state after the last timed step as float .npy files."""
import json
import os

import numpy as np
import pytest


def test_plain_run_is_lean_by_default():
  import bench
  args = bench.parse(['--gpus', '1', '--steps', '7', '--warmup', '3'])
  assert (args.steps, args.warmup) == (7, 3)
  assert args.full is False and args.dump_outputs is None
  args = bench.parse(['--full', '--dump-outputs', 'somewhere'])
  assert args.full is True and args.dump_outputs == 'somewhere'


def test_dump_outputs_writes_one_npy_per_array(tmp_path):
  import bench
  outs = {'a': np.arange(6, dtype=np.float32).reshape(2, 3), 'b': np.float64([1.5, -2.0])}
  d = str(tmp_path / 'new' / 'dir')
  bench.dump_outputs(d, outs)
  assert sorted(os.listdir(d)) == ['a.npy', 'b.npy']
  for k, v in outs.items():
    got = np.load(os.path.join(d, k + '.npy'), allow_pickle=False)
    assert got.dtype == v.dtype
    np.testing.assert_array_equal(got, v)


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_its_outputs(tmp_path, capsys):
  """A plain run at a small buffer: the supplementary fields are null, the step count is the
  one asked for, and the dump holds finite float arrays within the size limit -- the online
  parameters no longer the target's (the steps really ran), the priorities those of the
  dumped loss (sqrt(loss + 1e-10), rainbow_agent.py:289-290)."""
  import bench
  d = str(tmp_path / 'dump')
  bench.main(['--gpus', '1', '--steps', '9', '--warmup', '2', '--capacity', '30000',
              '--dump-outputs', d])
  line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
  assert line['steps'] == 9 and line['warmup'] == 2 and line['full'] is False
  assert line['ms_per_step'] > 0 and line['dtype'] == 'fp32' and line['higher_is_better'] is True
  # value = steps/s of the same window (ms_per_step is rounded to 1e-4 ms, value to 0.01)
  assert abs(line['value'] - 1e3 / line['ms_per_step']) <= (
      line['value'] * 1e-4 / line['ms_per_step'] + 0.01)
  for k in ('roofline', 'cpu_baseline', 'other_configs', 'throughput_mode'):
    assert line[k] is None, k
  outs = {f[:-4]: np.load(os.path.join(d, f), allow_pickle=False) for f in os.listdir(d)}
  assert set(outs) == {'online_params', 'target_params', 'loss', 'priorities',
                       'sampling_probabilities', 'indices'}
  assert sum(a.nbytes for a in outs.values()) <= bench.MAX_DUMP_BYTES
  for k, a in outs.items():
    assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), k
  assert outs['online_params'].shape == outs['target_params'].shape
  assert not np.array_equal(outs['online_params'], outs['target_params'])
  np.testing.assert_allclose(outs['priorities'], np.sqrt(outs['loss'].astype(np.float64) + 1e-10),
                             rtol=1e-6)
  assert ((outs['indices'] >= 0) & (outs['indices'] < 30000)).all()
