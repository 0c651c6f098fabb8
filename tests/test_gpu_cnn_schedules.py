"""Every launch schedule of the grouped Nature-CNN backward (dq_cnn_backward_riders) against
the plain one (dq_cnn_backward) and a separate optimizer step, bit for bit.

The matrix: optimizer {none, TF1 Adam, TF1 RMSProp centered / uncentered} x head_from
{3, 4, 5, 6, 7} x target head {absent, present} x first launch {0, 1}, at (B, n_out) =
(1, 1) -- the floor -- and (33, 129): one full 32-row tile plus a ragged row, and one full
128-row tile of fc2's weight gradient plus a ragged row.  Every case asserts
  * the flat gradient == dq_cnn_backward's on a second executor with the same parameters;
  * with an optimizer, parameters and optimizer state == dq_cnn_backward followed by the
    separate optimizer step, over two steps (both beta-power slots);
  * with a head, the head network holds exactly what its head_from promises (compared with a
    separate executor's forward on the same input) and NaN everywhere else.
Only ``HipNatureCNN.backward`` with valid arguments is called; a combination that would reach
another entry point (no optimizer, no head) carries empty riders, which select
dq_cnn_backward_riders and leave every launch as it is."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (33, 129)]
OPTS = ['none', 'adam', 'rms_centered', 'rms_uncentered']
HEAD_FROMS = [3, 4, 5, 6, 7]
# what the head network holds after a backward with head=, by head_from ('slabs': the fc1
# split-K slabs in its workspace, checked by finishing the forward with forward_with_tail)
PROMISED = {3: ('a1', 'a2', 'a3', 'slabs'), 4: ('a1', 'a2', 'a3'), 5: ('a1', 'a2'), 6: ('a1',),
            7: ()}
HEAD_ACTS = ('a1', 'a2', 'a3', 'h', 'out')


class _Ctx(object):
  """Two online networks with equal parameters (the schedule under test and the reference),
  a target network with two executors (the riding head and its reference), two steps of
  inputs.  Built once per shape; ``reset`` restores the parameters."""

  def __init__(self, B, A):
    from dopamine_amd.agents.networks import NatureDQNNetwork
    from dopamine_amd.cnn import HipNatureCNN
    self.B, self.A = B, A
    self.nets = [NatureDQNNetwork(A, device='cuda', seed=5) for _ in range(2)]
    self.tg = NatureDQNNetwork(A, device='cuda', seed=6)
    gen = torch.Generator(device='cuda').manual_seed(11)
    with torch.no_grad():     # non-zero biases so the bias paths are exercised
      for n, prm in self.tg.fp.params.items():
        if n.endswith('_b'):
          prm.uniform_(-0.05, 0.1, generator=gen)
      for n, prm in self.nets[0].fp.params.items():
        if n.endswith('_b'):
          prm.uniform_(-0.05, 0.1, generator=gen)
    self.p0 = self.nets[0].fp.flat.clone()
    self.hips = [HipNatureCNN(n, B) for n in self.nets]
    self.ht = HipNatureCNN(self.tg, B)
    ht_ref = HipNatureCNN(self.tg, B)
    rnd = lambda *s: torch.rand(*s, device='cuda', generator=gen)
    self.x = [rnd(B, 84, 84, 4) for _ in range(2)]
    self.nx = [rnd(B, 84, 84, 4) for _ in range(2)]
    self.gout = [torch.randn(B, A, device='cuda', generator=gen) for _ in range(2)]
    self.ref_t = []           # the target network's forward on nx[step], computed once
    for nx in self.nx:
      ht_ref.forward(nx)
      self.ref_t.append({k: ht_ref.acts[k].clone() for k in HEAD_ACTS})
    self.mask = torch.zeros_like(self.p0, dtype=torch.bool)   # the parameters, not the pads
    for o, m in self.nets[0].fp.segments():
      self.mask[o:o + m] = True
    torch.cuda.synchronize()

  def reset(self):
    for n in self.nets:
      n.fp.flat.copy_(self.p0)
      n.fp.grad.zero_()

  def make_opts(self, kind):
    from dopamine_amd import ops
    if kind == 'none':
      return [None, None], ()
    if kind == 'adam':
      return ([ops.TF1Adam(n.fp.flat, learning_rate=6.25e-5, epsilon=1.5e-4) for n in self.nets],
              ('params', 'm', 'v', 'state'))
    return ([ops.TF1RMSProp(n.fp.flat, learning_rate=2.5e-4, decay=0.95, momentum=0.1,
                            epsilon=1e-5, centered=kind == 'rms_centered') for n in self.nets],
            ('params', 'ms', 'mg', 'mom'))

  def nan_fill(self):
    """The gradient under test (its parameter views: the alignment pads stay zero, as in the
    reference, so the separate optimizer step reads the same pads) and the head's activations."""
    for v in self.nets[0].fp.grad_views:
      v.fill_(float('nan'))
    for k in HEAD_ACTS:
      self.ht.acts[k].fill_(float('nan'))

  def head_acts(self):
    return {k: self.ht.acts[k].clone() for k in HEAD_ACTS}


_ctx_cache = {}


@pytest.fixture
def ctx(request):
  key = request.param
  if key not in _ctx_cache:
    _ctx_cache.clear()          # one shape's buffers at a time
    _ctx_cache[key] = _Ctx(*key)
  c = _ctx_cache[key]
  c.reset()
  return c


def _riders(first, head_from):
  """One empty rider (kind none) per launch of the schedule from ``first``."""
  from dopamine_amd import _lib
  launches = 6 if head_from >= 5 else 7
  return [_lib.Rider() for _ in range(first, launches)]


def _check_head(c, step, head_from, present):
  """The head network after the backward: exactly what head_from promises, NaN elsewhere."""
  from dopamine_amd.cnn import forward_with_tail
  promised = PROMISED[head_from] if present else ()
  ref = c.ref_t[step]
  for k in HEAD_ACTS:
    if k in promised:
      assert torch.equal(c.ht.acts[k], ref[k]), (head_from, k)
    else:
      assert torch.isnan(c.ht.acts[k]).all(), (head_from, k)
  if 'slabs' in promised:
    forward_with_tail(c.hips[0], c.x[step], c.ht)
    torch.cuda.synchronize()
    assert torch.equal(c.ht.acts['out'], ref['out']), head_from
    assert torch.equal(c.ht.acts['h'], ref['h']), head_from


def _run(c, opt, head_from, present, first, riders):
  c.reset()
  opts, state_names = c.make_opts(opt)
  test, ref = c.hips
  test.store_grads = True
  for step in range(2 if opt != 'none' else 1):
    x, gout = c.x[step], c.gout[step]
    test.forward(x)
    ref.forward(x)
    ref.backward(gout)                                   # dq_cnn_backward
    if opts[1] is not None:
      opts[1].step(c.nets[1].fp.grad, slot=step % 2)
    c.nan_fill()
    if first == 1:
      test.backward(gout, groups=(0, 1))                 # dacts['h'], as the fused losses leave it
    test.backward(gout, groups=(first, 7), head=(c.ht, c.nx[step]) if present else None,
                  head_from=head_from, adam=opts[0], slot=step % 2,
                  riders=_riders(first, head_from) if riders else None)
    torch.cuda.synchronize()
    what = (opt, head_from, present, first, step)
    assert torch.equal(c.nets[0].fp.grad, c.nets[1].fp.grad), what
    for n in state_names:
      a, b = getattr(opts[0], n), getattr(opts[1], n)
      if a.numel() == c.mask.numel():
        a, b = a[c.mask], b[c.mask]
      assert torch.equal(a, b), what + (n,)
    _check_head(c, step, head_from, present)


@pytest.mark.parametrize('head_from', HEAD_FROMS)
@pytest.mark.parametrize('opt', OPTS)
@pytest.mark.parametrize('ctx', SHAPES, indirect=True, ids=lambda s: 'B%d_n%d' % s)
def test_schedule_matrix(ctx, opt, head_from):
  """head {absent, present} x first {0, 1} of one (shape, optimizer, head_from)."""
  for present in (False, True):
    for first in (0, 1):
      # without an optimizer or a head only riders select dq_cnn_backward_riders
      _run(ctx, opt, head_from, present, first, riders=opt == 'none' and not present)


@pytest.mark.parametrize('head_from', HEAD_FROMS)
@pytest.mark.parametrize('ctx', SHAPES, indirect=True, ids=lambda s: 'B%d_n%d' % s)
def test_empty_riders_leave_the_schedule_unchanged(ctx, head_from):
  """One empty rider (kind none) per launch beside the optimizer and the head: the rider
  indexing of every launch, without a replay buffer."""
  _run(ctx, 'adam', head_from, True, 1, riders=True)
  _run(ctx, 'none', head_from, True, 0, riders=True)


@pytest.mark.parametrize('first', [0, 1])
@pytest.mark.parametrize('head_from', [3, 6])
@pytest.mark.parametrize('ctx', SHAPES, indirect=True, ids=lambda s: 'B%d_n%d' % s)
def test_split_backward_equals_single_call(ctx, head_from, first):
  """The data-parallel learner's split -- launches [first, 3), then [3, 7) with the head --
  equals the single call bit for bit: gradient and head network."""
  c = ctx
  test, ref = c.hips
  x, gout, nx = c.x[0], c.gout[0], c.nx[0]
  test.forward(x)
  ref.forward(x)
  ref.backward(gout)
  got = []
  for split in (False, True):
    c.nan_fill()
    if first == 1:
      test.backward(gout, groups=(0, 1))
    if split:
      test.backward(gout, groups=(first, 3))
      test.backward(gout, groups=(3, 7), head=(c.ht, nx), head_from=head_from)
    else:
      test.backward(gout, groups=(first, 7), head=(c.ht, nx), head_from=head_from)
    torch.cuda.synchronize()
    got.append((c.nets[0].fp.grad.clone(), c.head_acts()))
    assert torch.equal(c.nets[0].fp.grad, c.nets[1].fp.grad), split
    _check_head(c, 0, head_from, True)
  assert torch.equal(got[0][0], got[1][0])
  for k in HEAD_ACTS:      # as bits: what is not promised is NaN in both
    assert torch.equal(got[0][1][k].view(torch.int32), got[1][1][k].view(torch.int32)), k
