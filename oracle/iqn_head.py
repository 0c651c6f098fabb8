"""float64 implicit-quantile head, stage by stage -- TEST INFRASTRUCTURE ONLY.

Only ``tests/`` may import this module.  The quantile head of ImplicitQuantileNetwork
(atari_lib.py:147-199) after the 7744-wide state vector, as dopamine_amd/csrc/iqn.hip lays it
out: R = nq * B quantile rows, row r = q * B + b (tf.tile of the state), so the state row of r
is r % B.  ``head_reference`` restates every stage of the forward and of the backward in
torch-CPU float64, each on the caller's own input to that stage (a device test passes the
device's cos, emb, h, dh and dpre), so each stage is judged alone and every ReLU decision
(emb > 0, h > 0, state > 0) is the one the device's epilogue reads.  Every result comes with the
float64 sum of the absolute values of the terms its reduction adds (suffix ``_abs``), for the
measure of oracle/nature_cnn.py (cond_ratio, assert_layer_close), which this module reuses.
"""
import math

import numpy as np
import torch

from oracle.nature_cnn import (COND_FLOOR, LAYER_TOL, assert_guard_untouched,  # noqa: F401
                               assert_layer_close, assert_spare_untouched, bf16_round, cond_ratio)

F, H = 7744, 512
HEAD = ('emb_w', 'emb_b', 'fc1_w', 'fc1_b', 'fc2_w', 'fc2_b')
# every stage head_reference returns, in the order the device computes them (x, the fp32
# Hadamard product, is compared bit for bit and has no Σ|terms|)
STAGES = ('cos', 'emb', 'h', 'q', 'dh', 'dw2', 'db2', 'dpre', 'dtl', 'dstate', 'dw1', 'db1',
          'dwe', 'dbe')
# deliberately wrong restatements head_reference can make (a test holds a correct result to
# them and expects the assertion to fail)
WRONG = ('state_row_b_major', 'drop_last_q')
# the stages that are one GEMM (or one column of one: db1 and dbe are the products with the
# ones column of dW1's and the wide dWe's second operand), whose operands head_reference can
# round to bf16
GEMM_STAGES = ('emb', 'h', 'q', 'dh', 'dw2', 'db2', 'dw1', 'db1', 'dwe', 'dbe')

# (B, nq, A, E), the smallest shapes that reach each path of iqn.hip (fuse_tile = nq | 128):
#   (1, 1, 1, 64)     R = 1: one-term reductions, one split-K slab everywhere, fused, nq = 1
#   (17, 8, 18, 64)   R = 136, fused: the second 128-row tile holds one whole sample; dW1 slabs
#                     96 + 40, narrow dWe 64 + 64 + 8, dW2 128 + 8; k_colsum over 2 partial rows
#   (2, 128, 4, 64)   R = 256, fused, one sample per row tile
#   (130, 1, 2, 64)   R = 130, fused: 128 samples per tile + 2; B > 128; dWe's last slab 2 rows
#   (27, 5, 3, 64)    R = 135, not fused (EpiDx + k_tile_grad): a ragged second row tile (7 rows),
#                     wide dWe (N = 65) in 5 slabs, the last of 7; A = 3 (ld no multiple of 4)
#   (11, 3, 4, 68)    R = 33, not fused: a second slab of one row in dW1 and the wide dWe; E = 68:
#                     a ragged third K slice of the embedding, dWe with N = 69
#   (3, 4, 4, 4)      R = 12, fused; E = 4: K inside one slice, narrow dWe with N = 4
CASES = ((1, 1, 1, 64), (17, 8, 18, 64), (2, 128, 4, 64), (130, 1, 2, 64), (27, 5, 3, 64),
         (11, 3, 4, 68), (3, 4, 4, 4))


def make_inputs(B, nq, A, E, device='cpu'):
  """An ImplicitQuantileNetwork on ``device`` with non-zero head biases, and one case's
  synthetic inputs (host tensors): a state with exact zeros (relu(randn) / 2: about half),
  taus in [0, 1), a Gaussian d loss / d q.  The same values on every device."""
  from dopamine_amd.agents import networks
  net = networks.ImplicitQuantileNetwork(A, quantile_embedding_dim=E, device=device, seed=3)
  gen = torch.Generator().manual_seed(1000 * B + 10 * nq + A + E)
  with torch.no_grad():
    for n in ('emb_b', 'fc1_b', 'fc2_b'):
      net.fp[n].copy_((torch.rand(net.fp[n].shape, generator=gen) * 0.1 - 0.05).to(device))
  R = B * nq
  state = torch.relu(torch.randn(B, F, generator=gen)) * 0.5
  taus = torch.rand(R, generator=gen)
  dq = torch.randn(R, A, generator=gen) / R
  return net, state, taus, dq


_M64 = (1 << 64) - 1


def uniform_of(seed, call, i):
  """Draw i of call ``call`` of the device's tau generator (iqn.hip uniform_of): a splitmix64
  hash of (seed, call, i) in 64-bit wrap-around arithmetic, its top 24 bits k -> k * 2^-24
  (exact in float32).  Python integers throughout."""
  z = (int(seed) + int(call) * 0x9E3779B97F4A7C15 + (int(i) + 1) * 0xD1B54A32D192ED03) & _M64
  z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
  z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
  z ^= z >> 31
  return (z >> 40) * 2.0 ** -24


def uniform_draws(seed, call, n):
  """uniform_of(seed, call, 0 .. n - 1) as a float32 array."""
  return np.array([uniform_of(seed, call, i) for i in range(n)], dtype=np.float32)


def _f64(t):
  return torch.as_tensor(t).detach().to('cpu', torch.float64)


def _f32(t):
  return torch.as_tensor(t).detach().to('cpu', torch.float32)


def cos_argument(taus, E):
  """The cosine's argument as the reference forms it in float32, (float(k + 1) * float32(pi))
  * tau left to right (atari_lib.py:176-178; oracle/nature_cnn.iqn_forward), (R, E) float32."""
  i_pi = torch.arange(1, E + 1, dtype=torch.float32) * torch.tensor(math.pi, dtype=torch.float32)
  return _f32(taus).reshape(-1, 1) * i_pi


def state_rows(B, nq, wrong=()):
  """The state row of every quantile row r: r % B (``state_row_b_major``: r // nq)."""
  r = torch.arange(B * nq)
  return r // nq if 'state_row_b_major' in wrong else r % B


def _lin(x, w, b):
  return x @ w.T + b


def head_reference(B, nq, state, taus, params, dq, dev, wrong=(), bf16_stages=()):
  """float64 forward and backward of the head, stage by stage.

  state (B, 7744), taus (R,), dq (R, A) = d loss / d q; params: the six head tensors by name
  (HEAD; weights (out, in)); dev: the caller's cos (R, E), emb (R, 7744), h (R, 512), dh
  (R, 512) and dpre (R, 7744) -- the inputs of the stages that follow them.  wrong: names from
  WRONG, a deliberately wrong restatement.  bf16_stages: the stages among GEMM_STAGES whose two
  GEMM operands are rounded once to bf16 (bf16_round) before the float64 arithmetic and in
  the stage's Σ|terms| -- exact products of rounded operands, what a GEMM on the bf16 matrix
  instruction computes; biases and masks are never rounded.  For h the operand x is the fp32
  Hadamard product first, then rounded.

  Returns a dict of float64 tensors, each beside its Σ|terms| (suffix _abs), and ``x``:
    cos            cos64 of the float32 argument; terms = 1
    emb            relu(cos Weᵀ + be)                        on dev cos
    x              float32: the fp32 product state[r % B] · emb of dev emb (no _abs)
    h              relu(x W1ᵀ + b1)                          on that x
    q              h W2ᵀ + b2                                on dev h
    dh             (dq W2) · (h > 0)                         on dev h
    dw2, db2       dqᵀ [h | 1]                               on dev h
    dpre           (emb > 0) ? dx · state[r % B] : 0, dx = dh W1     on dev dh, dev emb
    dtl            d tiled = dx · emb
    dstate         (state > 0) · Σ_q dx[q B + b] · emb[q B + b]
    dw1, db1       dhᵀ [x | 1]                               on dev dh and x
    dwe, dbe       dpreᵀ [cos | 1]                           on dev dpre, dev cos."""
  assert set(wrong) <= set(WRONG), wrong
  assert set(bf16_stages) <= set(GEMM_STAGES), bf16_stages
  R = B * nq

  def ops(stage, *ts):             # the stage's GEMM operands, rounded if the stage is bf16
    return [bf16_round(t).double() if stage in bf16_stages else t for t in ts]
  p = {n: _f64(params[n]) for n in HEAD}
  E = p['emb_w'].shape[1]
  state64, dq = _f64(state), _f64(dq)
  d = {n: _f64(dev[n]) for n in ('cos', 'emb', 'h', 'dh', 'dpre')}
  assert state64.shape == (B, F) and dq.shape[0] == R and d['emb'].shape == (R, F)
  rows = state_rows(B, nq, wrong)
  out = {}
  # ---- forward
  out['cos'] = torch.cos(cos_argument(taus, E).double())
  out['cos_abs'] = torch.ones_like(out['cos'])
  a, w = ops('emb', d['cos'], p['emb_w'])
  out['emb'] = torch.relu(_lin(a, w, p['emb_b']))
  out['emb_abs'] = _lin(a.abs(), w.abs(), p['emb_b'].abs())
  x32 = _f32(state)[rows] * _f32(dev['emb'])            # one fp32 rounding per element
  out['x'] = x32
  x = x32.double()
  a, w = ops('h', x, p['fc1_w'])
  out['h'] = torch.relu(_lin(a, w, p['fc1_b']))
  out['h_abs'] = _lin(a.abs(), w.abs(), p['fc1_b'].abs())
  a, w = ops('q', d['h'], p['fc2_w'])
  out['q'] = _lin(a, w, p['fc2_b'])
  out['q_abs'] = _lin(a.abs(), w.abs(), p['fc2_b'].abs())
  # ---- backward
  hmask = (d['h'] > 0).double()
  a, w = ops('dh', dq, p['fc2_w'])
  out['dh'] = (a @ w) * hmask
  out['dh_abs'] = (a.abs() @ w.abs()) * hmask
  a, w = ops('dw2', dq, d['h'])
  out['dw2'], out['dw2_abs'] = a.T @ w, a.abs().T @ w.abs()
  a, = ops('db2', dq)
  out['db2'], out['db2_abs'] = a.sum(0), a.abs().sum(0)
  dx, dx_abs = d['dh'] @ p['fc1_w'], d['dh'].abs() @ p['fc1_w'].abs()
  emask = (d['emb'] > 0).double()
  out['dpre'] = dx * state64[rows] * emask
  out['dpre_abs'] = dx_abs * state64[rows].abs() * emask
  out['dtl'], out['dtl_abs'] = dx * d['emb'], dx_abs * d['emb'].abs()
  # tf.tile's gradient: the rows of sample b, then the torso's last ReLU
  keep = torch.ones(R, 1, dtype=torch.float64)
  if 'drop_last_q' in wrong:
    keep[torch.arange(R) // B == nq - 1] = 0.0
  smask = (state64 > 0).double()
  zero = torch.zeros(B, F, dtype=torch.float64)
  out['dstate'] = zero.index_add(0, rows, out['dtl'] * keep) * smask
  out['dstate_abs'] = zero.index_add(0, rows, out['dtl_abs'] * keep) * smask
  a, w = ops('dw1', d['dh'], x)
  out['dw1'], out['dw1_abs'] = a.T @ w, a.abs().T @ w.abs()
  a, = ops('db1', d['dh'])
  out['db1'], out['db1_abs'] = a.sum(0), a.abs().sum(0)
  a, w = ops('dwe', d['dpre'], d['cos'])
  out['dwe'], out['dwe_abs'] = a.T @ w, a.abs().T @ w.abs()
  a, = ops('dbe', d['dpre'])
  out['dbe'], out['dbe_abs'] = a.sum(0), a.abs().sum(0)
  return out


def assert_stage_close(what, stage, got, ref, tol=LAYER_TOL):
  """assert_layer_close of one stage of head_reference's dict (shapes as the reference's)."""
  want = ref[stage]
  return assert_layer_close('%s %s' % (what, stage), _f64(got).reshape(want.shape), want,
                            ref[stage + '_abs'], tol)
