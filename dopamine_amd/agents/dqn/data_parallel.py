"""The collective gradient exchange of data-parallel DQN learners (N > 1): the
bucketed, overlapped all-reduce / ZeRO-1 schedule (``Exchange.split_step``), the replicas'
start (a broadcast) and their check (``replica_report``).  The step's own parts reach it as
callables: nothing here knows the agent.  Communicators and collectives themselves are
``dopamine_amd.parallel``'s.
"""
import os

import torch
import torch.distributed as dist

from dopamine_amd import ops
from dopamine_amd import parallel


def grad_buckets(fp):
  """(fc1 + fc2: final after the backward's head, convs) of a flat gradient buffer."""
  o = fp.offsets['fc1_w'][0]
  return fp.grad[o:], fp.grad[:o]


def shard_bounds(n, fc_start, world):
  """lo: the sharded range [lo, n) of a flat buffer of n floats whose fc bucket starts at
  fc_start -- the fc bucket minus a head of fewer than 4N floats, so that it splits into N
  equal 16-byte-aligned slices; the head joins the conv bucket (all-reduced, replicated
  update)."""
  return fc_start + (n - fc_start) % (4 * world)


def fc_pieces(lo, hi, pieces):
  """[lo, hi) in ``pieces`` ranges, every boundary a multiple of 4 floats."""
  step = -(-(hi - lo) // (4 * pieces)) * 4
  return [(a, min(a + step, hi)) for a in range(lo, hi, step)]


def rank_dir(pg, checkpoint_dir):
  """``checkpoint_dir/rank<r>`` of this process's rank in group pg."""
  return os.path.join(checkpoint_dir, 'rank%d' % dist.get_rank(pg))


class Exchange(object):
  """One learner's end of the process group ``pg``: ``fp`` the online network's flat
  parameters / gradients, ``opt`` their optimizer, ``replica`` every tensor the replica's
  updates depend on.  Collective: every rank constructs it at the same point (the broadcast),
  and likewise calls make_native_comms once after it."""

  def __init__(self, pg, device, fp, opt, replica, shard_optimizer=False, comm_priority=-1):
    self.pg, self.device, self.fp, self.opt = pg, device, fp, opt
    self.world = dist.get_world_size(pg)
    self.shard_optimizer = shard_optimizer
    # the fc bucket's all-reduces (comm_priority -1: a high-priority queue, whose
    # workgroups are dispatched ahead of the main queue's pending ones)
    self.comm = torch.cuda.Stream(device, priority=comm_priority)
    self.comm_opt = torch.cuda.Stream(device)    # ... and the Adam parts behind them
    self.rccl = None
    self.pg_conv = None            # a second communicator for the conv bucket (see split_step)
    self.fc_pending = None         # event: the previous step's fc all-reduce + update are done
    self._next_check = None
    self._broadcast(replica)

  def _broadcast(self, replica):
    """Data-parallel replicas start from group rank 0's networks and optimizer state
    (whatever seed each rank was built with), so the identical all-reduced updates
    keep them bit-identical (parallel.replicas_in_sync)."""
    src = dist.get_process_group_ranks(self.pg)[0]
    for t in replica:
      dist.broadcast(t, src=src, group=self.pg)
    torch.cuda.synchronize(self.device)

  def make_native_comms(self, native_comm, split):
    """The (fc bucket, conv bucket) RcclComm pair for the split schedule (``split``) over
    RCCL, or None (gloo, or a schedule without buckets).  Collective."""
    if not (native_comm and split and dist.get_backend(self.pg) == 'nccl'):
      return
    if not parallel.native_comm_available(self.pg, self.device):
      return             # every rank agreed: torch.distributed's collectives instead
    self.rccl = (parallel.RcclComm(self.pg, self.device), parallel.RcclComm(self.pg, self.device))

  def barrier(self):
    dist.barrier(group=self.pg)

  def destroy(self):
    """Destroys the RCCL communicators (each holds proxy threads and device buffers until
    then); the HIP graphs that captured their collectives must be gone."""
    if self.rccl is not None:
      parallel.forget_capture_probes(self.rccl)
      for c in self.rccl:
        c.destroy()
      self.rccl = None

  # --------------------------------------------------------------- exchange
  def _ar_fc(self, t):
    """The fc bucket's all-reduce (mean), on the current (comm) stream."""
    if self.rccl is not None:
      return self.rccl[0].allreduce_mean_(t)
    return parallel.allreduce_mean_(t, self.pg)

  def _ar_conv(self, t, second):
    """The conv bucket's all-reduce (mean), on the current (main) stream: over the second
    communicator when the fc bucket's may still be in flight on the first."""
    if self.rccl is not None:
      return self.rccl[1].allreduce_mean_(t)
    return parallel.allreduce_mean_(t, self._conv_group() if second else self.pg)

  def _conv_group(self):
    """A second communicator over the same ranks: its all-reduce is not queued behind
    the fc bucket's on the first one's internal stream.  Created on first use, which
    every rank reaches at the same step."""
    if self.pg_conv is None:
      self.pg_conv = dist.new_group(ranks=dist.get_process_group_ranks(self.pg),
                                    backend=dist.get_backend(self.pg))
    return self.pg_conv

  def allreduce_grads(self):
    """The whole flat gradient in one all-reduce (the schedules without buckets)."""
    parallel.allreduce_mean_(self.fp.grad, self.pg)

  def join_fc(self):
    """The main stream waits for a deferred fc all-reduce + update (split_step)."""
    if self.fc_pending is not None:
      torch.cuda.current_stream(self.device).wait_event(self.fc_pending)
      self.fc_pending = None

  def sharded(self):
    """shard_optimizer in effect: N > 1 (or forced collectives) with TF1 Adam."""
    return (self.shard_optimizer and isinstance(self.opt, ops.TF1Adam)
            and (self.world > 1 or parallel.FORCE_COLLECTIVES))

  def shard_bounds(self):
    """(lo, n): the sharded range [lo, n) of the flat buffer (shard_bounds above)."""
    n = self.fp.grad.numel()
    return shard_bounds(n, n - grad_buckets(self.fp)[0].numel(), self.world), n

  def gather_opt_state(self):
    """ZeRO-1: every rank's Adam moments of the sharded range, slice r from rank r (a
    collective: every rank calls it, e.g. from bundle_and_checkpoint)."""
    lo, n = self.shard_bounds()
    torch.cuda.synchronize(self.device)
    for t in (self.opt.m, self.opt.v):
      parallel.all_gather_(t[lo:n], self.pg)
    torch.cuda.synchronize(self.device)

  def split_step(self, head_a, head_b, tail, opt, k=0, defer=False, branch_first=False, pieces=1):
    """head | tail on the main stream with the fc bucket's all-reduce on the comm
    stream beside the tail; with TF1 Adam the fc parameters' update follows their
    all-reduce on the comm stream (hidden under the conv bucket's all-reduce) and
    only the conv parameters' update (which advances the beta powers) is left
    after the join: same arithmetic, split in two launches (dq_adam_tf1_part).
    In the learner-only loop (defer, fused Rainbow head split in head_a | head_b)
    the join moves to the next step, between its conv and fc forward launches: the
    fc all-reduce then runs under this step's tail AND the next step's convs, and
    the conv bucket goes over a second communicator so it does not wait behind it.
    Every launch keeps its inputs: the next step's convs read no fc parameter, its
    fc launches wait for the update, and Adam's beta-power slots alternate (the fc
    part reads slot k while the conv part writes slot 1 - k).
    branch_first: capture the fc bucket's branch before the backward tail instead of after
    it; pieces: the fc bucket's all-reduce pieces (_fc_branch).  The order of the stream
    operations here is the topology of the graph a capture records: keep it."""
    main = torch.cuda.current_stream(self.device)
    fc, conv = grad_buckets(self.fp)
    split_opt = isinstance(self.opt, ops.TF1Adam)
    defer = defer and split_opt and head_a is not None
    grad = self.fp.grad
    o = grad.numel() - fc.numel()
    if head_a is not None:
      head_a()
    self.join_fc()
    head_b()
    ev = torch.cuda.Event()
    ev.record(main)
    # the tail is issued (captured) before the comm branch, so in a captured graph it is the
    # first child of the head's last launch and stays on that launch's hardware queue -- the
    # all-reduce branch takes the other one (a fork to another queue costs ~10 us on the
    # critical path, measured with the branch captured first; branch_first re-measures it)
    if not branch_first:
      tail()
    last, conv, o = self._fc_branch(ev, grad, conv, o, k, split_opt, pieces)
    if branch_first:
      tail()
    if defer:
      self._ar_conv(conv, True)
      self.fc_pending = torch.cuda.Event()
      self.fc_pending.record(last)
    else:
      self._ar_conv(conv, False)
      main.wait_stream(last)
    if split_opt:
      self.opt.step_part(grad, 0, o, slot=k, bump=True)
    else:
      opt()

  def _fc_branch(self, ev, grad, conv, o, k, split_opt, pieces):
    """The fc bucket's exchange and update on the comm stream (forked at event ev, after
    the backward launch that leaves fc1 / fc2's gradients final).  Returns (the stream to
    join, the conv bucket, its end offset)."""
    self.comm.wait_event(ev)
    # The fc bucket as ``pieces`` all-reduces back to back on the comm stream; each
    # piece's Adam part runs on a second stream behind its own all-reduce, under the
    # next piece's (an HBM-bound update beside a link-bound collective).  Elementwise
    # ops: bitwise the one-bucket result.  (Blocking collectives + events rather than
    # async work handles, which graph capture does not survive.)
    last = self.comm
    if self.sharded():
      # ZeRO-1: reduce-scatter the fc bucket, TF1 Adam on this rank's slice only (1/N of
      # the fc update's 112 MB), all-gather the updated parameters -- the same bytes over
      # the links as the all-reduce; the other slices' moments live on their owners
      lo, n = self.shard_bounds()
      S = (n - lo) // self.world
      r = dist.get_rank(self.pg)
      # all three on the comm stream: they are dependent, so a second stream for the
      # update buys no overlap -- and that arrangement (comm -> second stream -> comm) made
      # the captured chunk graphs segfault in hipStreamEndCapture on ROCm 7.2 (DESIGN §6;
      # the repro is tools/capture_fork_repro.py, outside the product)
      with torch.cuda.stream(self.comm):
        if self.rccl is not None:
          self.rccl[0].reduce_scatter_mean_(grad[lo:n])
        else:
          parallel.reduce_scatter_mean_(grad[lo:n], self.pg)
        self.opt.step_part(grad, lo + r * S, lo + (r + 1) * S, slot=k, bump=False)
        if self.rccl is not None:
          self.rccl[0].all_gather_(self.opt.params[lo:n])
        else:
          parallel.all_gather_(self.opt.params[lo:n], self.pg)
      conv, o = grad[:lo], lo                 # the head of the fc bucket joins the conv bucket
    else:
      ranges = fc_pieces(o, grad.numel(), pieces) if split_opt else [(o, grad.numel())]
      # one piece: its update right behind it on the comm stream (measured equal to the
      # second stream at one rank, 6,040 / 6,007 vs 6,027 / 6,014 steps/s, and one queue
      # hop fewer in the captured graphs)
      one = len(ranges) == 1
      for lo, hi in ranges:
        with torch.cuda.stream(self.comm):
          self._ar_fc(grad[lo:hi])
          if split_opt and one:
            self.opt.step_part(grad, lo, hi, slot=k, bump=False)
        if split_opt and not one:
          e = torch.cuda.Event()
          e.record(self.comm)
          self.comm_opt.wait_event(e)
          with torch.cuda.stream(self.comm_opt):
            self.opt.step_part(grad, lo, hi, slot=k, bump=False)
          last = self.comm_opt
    return last, conv, o

  # ---------------------------------------------------------- replica checks
  def captures_collectives(self, split_fused):
    """N > 1 over the learner's own RCCL communicators with the split fused-head schedule
    (``split_fused``): the gradient all-reduces are captured inside the learner loop's chunk
    graphs (gloo's host-side collectives cannot be, torch.distributed's are not)."""
    # (torch.distributed's own collectives are never captured: parallel.collectives_capturable)
    return (dist.get_backend(self.pg) == 'nccl' and self.rccl is not None and split_fused and
            isinstance(self.opt, ops.TF1Adam) and
            parallel.collectives_capturable(self.pg, self.device, self.comm,
                                            sharded=self.sharded(), comms=self.rccl))

  def replica_report(self, named, gather):
    """Collective (every rank of the group calls it at the same point): every tensor of
    ``named`` (name -> tensor; ``gather``: the sharded ranges' moments gathered first,
    gather_opt_state) compared bit for bit with group rank 0's (parallel.replica_report).
    SURVEY 8e: identical updates keep the replicas bit-identical; this is the check that
    they did."""
    self.join_fc()
    torch.cuda.synchronize(self.device)
    if gather:
      self.gather_opt_state()
    return parallel.replica_report(named, self.pg)

  def maybe_check_replicas(self, opt_steps, period, check, report):
    """Every ``period`` gradient steps (0: never), crossed inside a train_gradient_steps
    call, which every rank makes with the same n: check() (collective), then report()'s
    replica_report; a divergence raises on every rank."""
    if not period:
      return
    if self._next_check is None:
      self._next_check = opt_steps + period
    if opt_steps < self._next_check:
      return
    self._next_check = opt_steps + period
    check()
    bad = {k: v['differing'] for k, v in report().items() if not v['in_sync']}
    if bad:
      raise RuntimeError('data-parallel replicas diverged after %d gradient steps: elements '
                         'differing from rank 0, per rank: %r' % (opt_steps, bad))
