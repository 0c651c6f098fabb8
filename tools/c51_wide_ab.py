"""Gradient steps/s of c51_cartpole_201.gin (201 atoms: dq_c51_loss's wide kernel) beside
c51_cartpole.gin (51 atoms: the one-wave kernel) on one device, under tools/gym_mlp_ab.py's
protocol: the agents are built from the same seed over the same 3,000-transition buffer,
their graphs are primed, and they alternate, the order reversed every round, over ``--rounds``
rounds of learner windows of at least ``--window`` seconds, a device synchronise closing each
window.  A second 51-atom agent is the A/A arm (the noise floor).
    python tools/c51_wide_ab.py [--rounds 7]
--profile-arm runs 300 learner steps of the 201-atom agent only (the run to put under a
kernel-trace profiler for k_c51_wide's time per launch at (B, A, N) = (128, 2, 201));
--arms names the arms to run (e.g. ``--arms n51`` for one rate of the 51-atom agent, to set
beside another build's)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools import gym_mlp_ab as ab  # noqa: E402

_CONFIGS = os.path.join(ROOT, 'dopamine_amd', 'agents', 'rainbow', 'configs')
ARMS = {'n51': 'c51_cartpole', 'n201': 'c51_cartpole_201', 'n51b': 'c51_cartpole'}
for _name in set(ARMS.values()):
  ab.CONFIGS[_name] = (os.path.join(_CONFIGS, _name + '.gin'), 'RainbowAgent')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--window', type=float, default=0.3, help='seconds per learner window, at least')
  ap.add_argument('--arms', nargs='*', default=list(ARMS), choices=list(ARMS))
  ap.add_argument('--profile-arm', action='store_true')
  args = ap.parse_args()
  torch.cuda.set_device(0)
  if args.profile_arm:
    agent, _ = ab.build(ARMS['n201'], True)
    print('profile arm: %.1f gradient steps/s' % ab.run_learner(agent, 300), flush=True)
    return
  arms = {a: ab.build(ARMS[a], True)[0] for a in args.arms}
  n = 200
  slowest = min(ab.run_learner(a, n) for a in arms.values())
  n = max(n, int(slowest * args.window * 1.25))
  print('# learner windows of %d gradient steps' % n, flush=True)
  rows = []
  for rnd in range(args.rounds):
    order = list(arms) if rnd % 2 == 0 else list(arms)[::-1]
    row = {a: ab.run_learner(arms[a], n) for a in order}
    for a in order:
      print('round %d [%s] %.1f /s' % (rnd, a, row[a]), flush=True)
    rows.append(row)
  med = {a: statistics.median(r[a] for r in rows) for a in arms}
  for a in arms:
    v = [r[a] for r in rows]
    print('%s [%s] median %.1f /s  min %.1f  max %.1f  spread %.2f%%' % (
        ARMS[a], a, med[a], min(v), max(v), 100 * (max(v) - min(v)) / med[a]), flush=True)
  if 'n51' in arms and 'n201' in arms:
    pairs = [r['n201'] / r['n51'] for r in rows]
    print('201 / 51 atoms: median of medians %.4f  pairs %.4f .. %.4f' % (
        med['n201'] / med['n51'], min(pairs), max(pairs)), flush=True)
  if 'n51' in arms and 'n51b' in arms:
    aa = [r['n51'] / r['n51b'] for r in rows]
    print('A/A 51 / 51: median of medians %.4f  pairs %.4f .. %.4f' % (
        med['n51'] / med['n51b'], min(aa), max(aa)), flush=True)
  for agent in arms.values():
    agent.close()


if __name__ == '__main__':
  main()
