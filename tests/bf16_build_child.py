"""The child process of tests/test_gpu_bf16_build.py: python bf16_build_child.py {cnn|iqn} OUT.npz

Started with DOPAMINE_AMD_LIB naming the bf16 throughput build (dopamine_amd._build reads it
at import, so that library needs a process of its own).  Drives the C ABI exactly as
tests/test_gpu_cnn_layers.py / tests/test_gpu_iqn_head.py do (the shared LayerCase / HeadCase:
NaN-filled buffers with one spare sample, NaN inputs past the batch, 64 guard words behind the
workspace) and writes what the device computed to OUT.npz; the parent computes the references.
The bitwise comparisons between schedules are made here, on the device, and written as counts
of differing words.  Any failed check or C ABI error ends the process with a nonzero status."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import numpy as np
import pytest
import torch

from tests import bf16_build_ops as OPS

pytestmark = pytest.mark.gpu


def case_id(case):
  return '-'.join(str(v) for v in case)


def _np(t):
  return t.detach().cpu().contiguous().numpy()


def _differ(a, b):
  """How many 32-bit words of two fp32 tensors differ (NaNs compare by their bits)."""
  return int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum())


def _written(t):
  return int((~torch.isnan(t)).sum())


def _guarded(cls):
  class Guarded(cls):
    """The case, keeping the guard words of every call for the parent."""
    guards = None

    def call(self, fn, *args):
      try:
        super(Guarded, self).call(fn, *args)
      finally:
        if self.guards is None:
          self.guards = []
        self.guards.append(_np(self.ws[self.need:]))
  return Guarded


def run_cnn(out):
  from tests.cnn_layer_case import BACKWARD, D_NAMES, LayerCase
  for B, n_out in OPS.CNN_CASES:
    c = _guarded(LayerCase)(B, n_out)
    put = lambda name, t, pre='cnn/%s/' % case_id((B, n_out)): out.__setitem__(pre + name, _np(t))
    fp, h = c.net.fp, c.hip
    for name, prm in fp.params.items():
      put(name, prm)
    for name, t in c.acts.items():                       # x, a1, a2, a3, h, out: B + 1 samples
      put(name, t)
    put('dout', c.dout)
    # every layer's backward on its own upstream gradient, as test_backward_layer_matches_float64
    for index, layer, src, read, write in BACKWARD:
      c.nan_d()
      if read is not None:
        h.dacts[read][:B] = c.dz[read]
        put('dz_' + read, c.dz[read])
      c.layer(index, 1)
      if write is not None:
        c.layer(index, 0)
      (w0, w1), (b0, b1) = c.grad_range(layer + '_w'), c.grad_range(layer + '_b')
      put('%s/dw' % layer, fp.grad[w0:w1])
      put('%s/db' % layer, fp.grad[b0:b1])
      put('%s/grad_written' % layer, torch.tensor(_written(fp.grad)))   # must be the two slices
      for name in D_NAMES:
        put('%s/d_%s' % (layer, name), h.dacts[name])
    # the schedules: the chain of per-layer calls, the whole backward (twice), the 7 groups
    runs = {}
    for how in ('chain', 'whole', 'groups', 'again'):
      c.nan_d()
      if how == 'chain':
        for index, _, _, _, write in BACKWARD:
          c.layer(index, 1)
          if write is not None:
            c.layer(index, 0)
      elif how == 'groups':
        c.call('dq_cnn_backward_groups', *c.bwd, c.ws.data_ptr(), 0, 7, c.stream)
      else:
        c.call('dq_cnn_backward', *c.bwd, c.ws.data_ptr(), c.stream)
      runs[how] = [fp.grad.clone()] + [h.dacts[n].clone() for n in D_NAMES]
    seg = torch.zeros(fp.grad.numel(), dtype=torch.bool, device='cuda')
    for o, m in fp.segments():
      seg[o:o + m] = True
    chain = runs['chain']
    put('sched/chain_grad_nonfinite', torch.tensor(int((~torch.isfinite(chain[0][seg])).sum())))
    put('sched/chain_pads_written', torch.tensor(_written(chain[0][~seg])))
    put('sched/chain_d_nonfinite', torch.tensor(sum(int((~torch.isfinite(t[:B])).sum()) for t in chain[1:])))
    put('sched/chain_spare_written', torch.tensor(sum(_written(t[B:]) for t in chain[1:])))
    for how in ('whole', 'groups', 'again'):
      put('sched/%s_differs_from_chain' % how,
          torch.tensor(sum(_differ(a, b) for a, b in zip(runs[how], chain))))
    put('guards', torch.as_tensor(np.stack(c.guards)))
    del c, runs
    torch.cuda.empty_cache()


def run_iqn(out):
  from oracle import iqn_head as OIH
  from tests.iqn_head_case import GRAD_STAGES, HeadCase
  for case in OPS.IQN_CASES:
    c = _guarded(HeadCase)(*case)
    put = lambda name, t, pre='iqn/%s/' % case_id(case): out.__setitem__(pre + name, _np(t))
    fp, B, R = c.net.fp, c.B, c.R
    for name in OIH.HEAD:
      put(name, fp.params[name])
    for name, t in c.host.items():                       # state, taus, dq
      put(name, t)
    fwd = c.forward('emb+x')                             # FC1 reads the stored x
    for name, t in fwd.items():                          # R + 1 rows each
      put(name, t)
    inputs = dict(c.acts, dq=c.dq, state=c.state, taus=c.taus)
    before = {n: t.clone() for n, t in inputs.items()}
    bwd = c.backward(True)
    put('inputs_changed_by_backward', torch.tensor(sum(_differ(t, before[n]) for n, t in inputs.items())))
    for name in ('dh', 'dpre', 'dtl', 'dstate'):
      put(name, bwd[name])
    for stage, name in GRAD_STAGES:
      put(stage, c.grad_of(bwd['grad'], name))
    put('grad_written_outside_head', torch.tensor(_written(bwd['grad'][~c.head])))
    put('grad_head_nonfinite', torch.tensor(int((~torch.isfinite(bwd['grad'][c.head])).sum())))
    # the other forward form that reaches FC1 (x formed by RowKHad) and the backward on it
    # (dW1 over ColKOnesHad): bitwise the same h, q and gradients
    had = c.forward('emb')
    put('h_rowkhad', had['h'])
    put('q_rowkhad', had['q'])
    bwd2 = c.backward(False)
    put('backward_forms_differ', torch.tensor(sum(_differ(bwd2[n], bwd[n]) for n in bwd)))
    put('guards', torch.as_tensor(np.stack(c.guards)))
    del c, bwd, bwd2, fwd, had
    torch.cuda.empty_cache()


def main(which, path):
  from dopamine_amd import _build, _lib
  assert os.path.realpath(_lib.LIB_PATH) == os.path.realpath(_build.BF16_LIB_PATH), _lib.LIB_PATH
  assert _lib.BUILD_FLAGS == ' '.join(_build.BF16_FLAGS), _lib.BUILD_FLAGS
  t0 = time.time()
  out = {}
  {'cnn': run_cnn, 'iqn': run_iqn}[which](out)
  torch.cuda.synchronize()
  t1 = time.time()
  out['device_seconds'] = np.float64(t1 - t0)
  np.savez(path, **out)
  print('bf16_build_child %s: %.2f s on the device, %.2f s writing %d arrays' % (
      which, t1 - t0, time.time() - t1, len(out)))


if __name__ == '__main__':
  main(sys.argv[1], sys.argv[2])
