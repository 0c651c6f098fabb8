"""The data-parallel exchange's two pure functions: where the sharded range of the flat buffer
starts (ZeRO-1 / peer slices) and how the fc bucket is cut into all-reduce pieces."""
import pytest

from dopamine_amd.agents.dqn.data_parallel import fc_pieces, shard_bounds

# (n, fc_start): fc buckets of 0 floats, fewer than 4 * world for every world above 1, not
# divisible by 4 * world, divisible by all of them, and the Rainbow Nature CNN's
GRID = [(100, 100), (100, 97), (103, 96), (1000, 7), (1024, 0), (1031, 64), (4096 + 96, 96),
        (4_307_635, 78_080)]


@pytest.mark.parametrize('world', [1, 2, 3, 4, 8])
def test_shard_bounds_splits_the_fc_bucket_into_equal_aligned_slices(world):
  for n, fc_start in GRID:
    lo = shard_bounds(n, fc_start, world)
    assert fc_start <= lo <= n
    assert (n - lo) % (4 * world) == 0
    assert lo - fc_start < 4 * world


@pytest.mark.parametrize('pieces', [1, 2, 4])
def test_fc_pieces_tile_the_range_at_multiples_of_four_floats(pieces):
  for lo, hi in [(0, 4), (0, 16), (5, 6), (7, 1000), (96, 4096 + 96), (78_080, 4_307_635),
                 (3, 3 + 4 * pieces), (3, 4 + 4 * pieces)]:
    got = fc_pieces(lo, hi, pieces)
    assert 1 <= len(got) <= pieces
    assert got[0][0] == lo and got[-1][1] == hi
    for (a, b), (c, d) in zip(got, got[1:]):
      assert a < b == c < d
    assert all((a - lo) % 4 == 0 for a, _ in got)
