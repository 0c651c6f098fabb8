"""Launches dq_mdqn_loss (k_mdqn) and dq_dqn_huber_loss_double (k_dqn_double) on the same
Gaussian inputs, alternating, for a kernel-trace profiler's per-launch table:
    rocprofv3 --kernel-trace --stats -- python tools/mdqn_kernel_probe.py --batch 32 --actions 18
One shape per run, so the two shapes of a kernel do not share a row of the stats.  Prints the
shape and the two mean losses; times nothing itself."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dopamine_amd import ops  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=32)
  ap.add_argument('--actions', type=int, default=18)
  ap.add_argument('--launches', type=int, default=500)
  ap.add_argument('--tau', type=float, default=0.03)
  args = ap.parse_args()
  B, A = args.batch, args.actions
  g = torch.Generator(device='cpu').manual_seed(B * 1000 + A)
  draw = lambda *s: (torch.randn(*s, generator=g) * 3).cuda()
  oq, tq, tqc, sq = draw(B, A), draw(B, A), draw(B, A), draw(B, A)
  act = torch.randint(0, A, (B,), generator=g, dtype=torch.int32).cuda()
  rew = draw(B) / 3
  term = (torch.rand(B, generator=g) < 0.3).to(torch.uint8).cuda()
  out_m = out_d = None
  for _ in range(args.launches):
    out_m = ops.mdqn_loss(oq, tq, tqc, act, rew, term, 0.99, args.tau, 0.9, -1.0, out=out_m)
    out_d = ops.dqn_huber_loss(oq, tq, act, rew, term, 0.99, out=out_d, select_q=sq)
  torch.cuda.synchronize()
  print('B=%d A=%d launches=%d mdqn mean loss %.6f double mean loss %.6f' % (
      B, A, args.launches, float(out_m['mean_loss']), float(out_d['mean_loss'])))


if __name__ == '__main__':
  main()
