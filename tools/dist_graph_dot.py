"""Dump captured graphs of the learner as Graphviz dot and print their node/edge structure:
which node each kernel waits on, and every edge that crosses from the comm stream's branch
into the main chain.  The agent is the bench's Rainbow learner on a one-rank RCCL group with
every collective executed; --single: the single replica instead (no process group); --dqn: the
single-replica DQN of bench.py's dqn_pong (uniform replay: the chunk-gather graphs).

    python tools/dist_graph_dot.py OUTDIR [--zero 0|1] [--single | --dqn] [--key KEY ...]

KEY names a graph in the agent's _graph_sets after 60 learner-loop steps, as a Python literal:
a chunk key such as "('chunk', 4, 0)" (the default) or "('gchunk', 4, 0, 0, True)", or
FAMILY:PARITY:PART for one captured part of a per-step family, e.g. True:0:0 (PART counts the
parts that were captured, in issue order).  "list" prints the keys captured.  Per KEY it writes
OUTDIR/<key>.dot and OUTDIR/<key>_nodes.txt.  It reads only names that the parent trees have
too (a family through agent._graphs, whose per-parity entry was a bare graph where the step
has one part), so one copy of this file compares two trees.

A diagnostic for DESIGN.md §6 (what the next step's conv1 waits on); not a product path.
"""
import ast
import ctypes
import os
import re
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

_Orig = torch.cuda.CUDAGraph


class _DbgGraph(_Orig):
  """Every graph kept after instantiation (keep_graph), so HIP can print it."""

  def __new__(cls, keep_graph=False):
    return super().__new__(cls, True)

  def __init__(self, keep_graph=False):
    super().__init__(True)


def parse_dot(path):
  """(nodes {id: label}, edges [(a, b)]) from hipGraphDebugDotPrint output."""
  txt = open(path).read()
  nodes, edges = {}, []
  for m in re.finditer(r'"?(\w+)"?\s*\[(.*?)\];', txt, re.S):
    if m.group(1) == 'graph':      # the cluster's own attributes, not a node
      continue
    nodes[m.group(1)] = m.group(2).replace('\\n', ' ')     # every attribute, the label among them
  for m in re.finditer(r'"?(\w+)"?\s*->\s*"?(\w+)"?', txt):
    edges.append((m.group(1), m.group(2)))
  return nodes, edges


def short(label):
  """A node's kind; a kernel node's with its mangled name and launch dimensions."""
  m = re.search(r'([A-Za-z_]\w*)\s*<<<([^>]*)>>>', label.replace('\\', ''))
  if m:
    return 'KERNEL %s<<<%s>>>' % (m.group(1), re.sub(r'\s+', '', m.group(2)))
  m = re.search(r'(k_\w+|\w*[Rr]educe\w*|\w*[Gg]ather\w*|\w*[Cc]opy\w*|MEMCPY|MEMSET|EVENT\w*|'
                r'WAIT\w*|EMPTY|HOST\w*|KERNEL)', label)
  return (m.group(1) if m else label[:40])[:48]


def find_graph(agent, key):
  """The captured graph that KEY (the module docstring) names."""
  if key.split(':')[0] in ('True', 'False'):
    family, parity, part = (ast.literal_eval(x) for x in key.split(':'))
    assert family == agent.pipeline and agent._graphs is not None, (
        'the per-step family %s is not the captured one' % family)
    parts = agent._graphs[parity]
    parts = parts if isinstance(parts, (list, tuple)) else [parts]
    return [g for g in parts if g is not None][part]
  g = agent._graph_sets.get(ast.literal_eval(key))
  assert g is not None, 'no graph %s captured: %s' % (key, list(agent._graph_sets))
  return g


def print_graph(g, stem):
  """Graph g through HIP itself (torch's debug_dump is a no-op on ROCm) into stem.dot, its
  nodes in topological order with what each waits on into stem_nodes.txt and to stdout."""
  hip = ctypes.CDLL('libamdhip64.so')
  hip.hipGraphDebugDotPrint.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint]
  rc = hip.hipGraphDebugDotPrint(ctypes.c_void_p(g.raw_cuda_graph()), (stem + '.dot').encode(), 1)
  assert rc == 0, 'hipGraphDebugDotPrint rc %d' % rc
  list_nodes(stem)


def list_nodes(stem):
  """stem.dot's nodes in topological order -> stem_nodes.txt and stdout."""
  nodes, edges = parse_dot(stem + '.dot')
  preds = defaultdict(list)
  for a, b in edges:
    preds[b].append(a)
  # topological order
  indeg = {n: 0 for n in nodes}
  succ = defaultdict(list)
  for a, b in edges:
    succ[a].append(b)
    indeg[b] = indeg.get(b, 0) + 1
  order, ready = [], [n for n, d in indeg.items() if d == 0]
  while ready:
    n = ready.pop(0)
    order.append(n)
    for s in succ[n]:
      indeg[s] -= 1
      if indeg[s] == 0:
        ready.append(s)
  pos = {n: i for i, n in enumerate(order)}
  with open(stem + '_nodes.txt', 'w') as f:
    f.write('%d nodes, %d edges\n' % (len(nodes), len(edges)))
    for n in order:
      f.write('%4d %-50s <- %s\n' % (pos[n], short(nodes.get(n, '?')),
                                     ', '.join('%d:%s' % (pos.get(p, -1), short(nodes.get(p, '?')))
                                               for p in preds[n])))
  print(open(stem + '_nodes.txt').read())


def main():
  argv = sys.argv[1:]
  out = argv[0] if argv and not argv[0].startswith('--') else 'prof_out/dist_dot'
  zero = int(argv[argv.index('--zero') + 1]) if '--zero' in argv else 0
  single, dqn = '--single' in argv, '--dqn' in argv
  keys = [argv[i + 1] for i, a in enumerate(argv) if a == '--key']
  os.makedirs(out, exist_ok=True)
  torch.cuda.CUDAGraph = _DbgGraph
  from dopamine_amd import parallel
  import bench
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(0)
  if dqn:
    agent = bench.build_dqn_pong(dev)
  elif single:
    agent = bench.build_agent(9, 1_000_000, 32, dev)
  else:
    parallel.FORCE_COLLECTIVES = True
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29541')
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
    agent = bench.build_agent(9, 1_000_000, 32, dev, pg=dist.group.WORLD,
                              **({'shard_optimizer': True} if zero else {}))
  import random
  random.seed(0)
  bench.fill_synthetic(agent._replay.memory, agent.num_actions, seed=1)
  agent.train_gradient_steps(60)
  torch.cuda.synchronize()
  for key in keys or [repr(('chunk', agent._UNROLL, 0))]:
    if key == 'list':
      print('captured: %s' % sorted(str(k) for k in agent._graph_sets))
      continue
    print('== %s' % key)
    print_graph(find_graph(agent, key), os.path.join(out, re.sub(r'\W+', '_', key).strip('_')))
  agent.close()
  if not (single or dqn):
    dist.destroy_process_group()


if __name__ == '__main__':
  main()
