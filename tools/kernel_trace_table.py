"""Per-kernel launch times of a rocprofv3 --kernel-trace CSV: rows grouped by kernel name, LDS,
grid and block size, with the count, the median and the mean duration in microseconds, sorted by
total time.  Template arguments stay in the name (k_qr<true> / k_qr<false> are two rows).
    python tools/kernel_trace_table.py <..._kernel_trace.csv> [name filter ...]"""
import csv
import re
import statistics
import sys
from collections import defaultdict


def short(name):
  name = re.sub(r'^void ', '', name)
  return re.sub(r'\(.*\)$', '', name)[:92]


def main():
  rows = list(csv.DictReader(open(sys.argv[1])))
  keep = sys.argv[2:]
  agg = defaultdict(list)
  for r in rows:
    name = short(r['Kernel_Name'])
    if keep and not any(k in name for k in keep):
      continue
    key = (name, int(r.get('LDS_Block_Size', 0) or 0), int(r['Grid_Size_X']),
           int(r['Workgroup_Size_X']))
    agg[key].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
  print('%-92s %7s %8s %8s %6s %9s %9s' % ('kernel', 'lds', 'grid', 'wg', 'n', 'median_us',
                                           'mean_us'))
  for (name, lds, grid, wg), d in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
    print('%-92s %7d %8d %8d %6d %9.2f %9.2f' % (name, lds, grid, wg, len(d),
                                                 statistics.median(d), sum(d) / len(d)))


if __name__ == '__main__':
  main()
