"""dq_dueling_forward / dq_dueling_backward (k_dueling_fwd / k_dueling_bwd) at their edges.

Shapes (B, A, N) -- one thread per (b, z), 256-thread blocks over B * N:
  (1,1,1)      the minimum of every dimension       (4,3,64)     exactly one block
  (1,2,1)      one sample, DQN head                 (8,2,64)     exactly two blocks
  (32,2,1)     DQN head                             (33,3,65)    a block boundary inside a sample
  (33,3,1)     DQN head, odd batch                  (5,18,51)    several actions
  (128,18,1)   DQN head, wide action set            (32,4,101)   the Nature test agent
  (1,2,51)     one sample                           (128,2,200)  quantile cartpole
  (32,2,51)    cartpole Rainbow                     (3,3,255)    one below the atom limit
                                                    (7,64,256)   both limits
each with four input kinds (tests/dueling_cases.py).  Every launch goes into NaN-filled buffers
with one spare sample, which must stay NaN; every output is finite, within LAYER_TOL of float64
on its Σ|terms| (oracle.nature_cnn.assert_layer_close) and bitwise the fp32 restatement in the
kernel's order; a second launch and a launch replayed from a captured graph are bitwise equal.
"""
import numpy as np
import pytest
import torch

from oracle import nature_cnn as ONC
from tests import dueling_cases as DC

pytestmark = pytest.mark.gpu

CASES = DC.all_cases()
DEV = 'cuda'


def _nan(*shape):
  return torch.full(shape, float('nan'), dtype=torch.float32, device=DEV)


def _call(name, src, B, A, N, dst):
  """The raw entry point: (status, message)."""
  from dopamine_amd import _lib
  rc = getattr(_lib.lib, name)(_lib.ptr(src), B, A, N, _lib.ptr(dst), _lib.stream_of(dst.device))
  return rc, _lib.lib.dq_last_error().decode()


def _forward(c, graph=False):
  """out (B + 1, A * N): the launch at B samples into a NaN-filled buffer."""
  B, A, N = c['B'], c['A'], c['N']
  head = _nan(B + 1, (A + 1) * N)
  head[:B] = torch.from_numpy(c['head']).to(DEV)
  return _launch('dq_dueling_forward', head, B, A, N, _nan(B + 1, A * N), graph)


def _backward(c, key, graph=False):
  B, A, N = c['B'], c['A'], c['N']
  g = _nan(B + 1, A * N)
  g[:B] = torch.from_numpy(c[key]).to(DEV).reshape(B, A * N)
  return _launch('dq_dueling_backward', g, B, A, N, _nan(B + 1, (A + 1) * N), graph)


def _launch(name, src, B, A, N, dst, graph):
  if not graph:
    rc, msg = _call(name, src, B, A, N, dst)
    assert rc == 0, msg
  else:
    rc, msg = _call(name, src, B, A, N, torch.empty_like(dst))    # warm: the code object loaded
    assert rc == 0, msg
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):           # (the entry point launches on the capturing stream)
      rc, msg = _call(name, src, B, A, N, dst)
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst).all()), 'the capture itself wrote'
    g.replay()
  torch.cuda.synchronize()
  return dst


def _bits(t, B):
  return t[:B].cpu().numpy().tobytes()


@pytest.mark.parametrize('c', CASES, ids=DC.case_id)
def test_forward_against_float64_and_the_fp32_restatement(c):
  B, A, N = c['B'], c['A'], c['N']
  what = 'dueling forward %s' % DC.case_id(c)
  out = _forward(c)
  ONC.assert_spare_untouched(what, out, B)
  ref, terms = DC.forward64(c['head'], A, N)
  ONC.assert_layer_close(what, out[:B].reshape(B, A, N), ref, terms)
  assert _bits(out, B) == DC.forward32(c['head'], A, N).tobytes(), what
  assert _bits(_forward(c), B) == _bits(out, B), what + ': a second launch differs'
  if A == 1:
    assert _bits(out, B) == DC.split(c['head'], A, N)[1].tobytes()


@pytest.mark.parametrize('c', CASES, ids=DC.case_id)
def test_backward_against_float64_and_the_fp32_restatement(c):
  B, A, N = c['B'], c['A'], c['N']
  for key in ('g', 'gs'):
    what = 'dueling backward %s %s' % (DC.case_id(c), key)
    d = _backward(c, key)
    ONC.assert_spare_untouched(what, d, B)
    ref, terms = DC.backward64(c[key], A, N)
    ONC.assert_layer_close(what, d[:B], ref, terms)
    assert _bits(d, B) == DC.backward32(c[key], A, N).tobytes(), what
    assert _bits(_backward(c, key), B) == _bits(d, B), what + ': a second launch differs'
  # the sparse gradient (zero off the taken action): dval is the taken row, bit for bit
  taken = c['gs'][np.arange(B), c['act']]
  assert d[:B, A * N:].cpu().numpy().tobytes() == taken.tobytes()


@pytest.mark.parametrize('c', [c for c in CASES if c['kind'] == 'n1'], ids=DC.case_id)
def test_a_captured_launch_is_bitwise_the_plain_one(c):
  B = c['B']
  out = _forward(c, graph=True)
  ONC.assert_spare_untouched('graph forward', out, B)
  assert _bits(out, B) == _bits(_forward(c), B)
  d = _backward(c, 'g', graph=True)
  ONC.assert_spare_untouched('graph backward', d, B)
  assert _bits(d, B) == _bits(_backward(c, 'g'), B)


def test_ops_wrappers_allocate_or_fill_the_outputs():
  from dopamine_amd import ops
  c = DC.make_case(33, 3, 65, 'n1', 5)
  B, A, N = c['B'], c['A'], c['N']
  head = torch.from_numpy(c['head']).to(DEV)
  out = ops.dueling_forward(head, A, N)
  assert tuple(out.shape) == (B, A * N)
  buf = _nan(B, A * N)
  assert ops.dueling_forward(head, A, N, out=buf) is buf
  g = torch.from_numpy(c['g']).to(DEV)
  d = ops.dueling_backward(g, A, N)
  assert tuple(d.shape) == (B, (A + 1) * N)
  torch.cuda.synchronize()
  assert out.cpu().numpy().tobytes() == DC.forward32(c['head'], A, N).tobytes()
  assert buf.cpu().numpy().tobytes() == out.cpu().numpy().tobytes()
  assert d.cpu().numpy().tobytes() == DC.backward32(c['g'], A, N).tobytes()


@pytest.mark.parametrize('entry', ['dq_dueling_forward', 'dq_dueling_backward'])
@pytest.mark.parametrize('what,B,A,N,msg', [
    ('A0', 3, 0, 65, 'num_actions must be in \\[1, 64\\]'),
    ('A65', 3, 65, 65, 'num_actions must be in \\[1, 64\\]'),
    ('N0', 3, 2, 0, 'num_atoms must be in \\[1, 256\\]'),
    ('N257', 3, 2, 257, 'num_atoms must be in \\[1, 256\\]'),
    ('B0', 0, 2, 65, 'bad batch'),
    ('alias', 3, 2, 65, 'may not alias'),
    ('null', 3, 2, 65, 'null argument')])
def test_refusals_return_an_error_and_write_nothing(entry, what, B, A, N, msg):
  """Refused with the argument-error status before a launch (the sizes are only claimed: the
  buffers are those of the (3, 2, 65) case and nothing may touch them)."""
  import re
  src, dst = _nan(4, 3 * 65), _nan(4, 3 * 65)
  if what == 'alias':
    rc, text = _call(entry, dst, B, A, N, dst)
  elif what == 'null':
    rc, text = _call(entry, None, B, A, N, dst)
  else:
    rc, text = _call(entry, src, B, A, N, dst)
  assert rc == -1, (rc, text)                    # DQ_E_ARG
  assert re.search(msg, text), text
  torch.cuda.synchronize()
  assert bool(torch.isnan(src).all()) and bool(torch.isnan(dst).all())
