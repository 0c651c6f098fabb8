// The dueling head (dq_dueling_forward / k_dueling_fwd, dq_dueling_backward / k_dueling_bwd):
// the combine between a network's last layer and the loss kernels, and its transpose.
// A translation unit of its own, so the other units' code objects stay what they were.
#include "common.h"

namespace dq {

// ---------------------------------------------------------------------------
// Dueling networks (Wang et al., ICML 2016, eq. 9; upstream Dopamine's FullRainbowNetwork).
// head = the last layer's output, (B, (A + 1) * N) row-major; N = 1: the DQN head, N =
// num_atoms: the Rainbow head (logits or quantile values):
//   adv[b, a, z] = head[b, a * N + z]         columns [0, A * N), z fastest
//   val[b, z]    = head[b, A * N + z]         columns [A * N, (A + 1) * N)
// forward   s[b, z]      = ((adv[b, 0, z] + adv[b, 1, z]) + adv[b, 2, z]) + ...
//           m[b, z]      = s[b, z] / A
//           out[b, a, z] = (adv[b, a, z] - m[b, z]) + val[b, z]              (B, A, N)
// backward  g = d loss / d out, (B, A, N)
//           dval[b, z]    = ((g[b, 0, z] + g[b, 1, z]) + g[b, 2, z]) + ...
//           dadv[b, a, z] = g[b, a, z] - dval[b, z] / A
//           dhead = [dadv | dval]                                            (B, (A + 1) * N)
// The fp32 orders (fixed, functions of A alone; tests/dueling_cases.py restates them):
//   sums       sequential in action order, starting from action 0's element (no zero is added)
//   quotient   one correctly rounded division by (float)A, never a reciprocal multiply
//   out        the subtraction first, then the addition of val
// One thread per (b, z) walks the A actions, so a wave's loads and stores run along z.  Each
// pass takes the actions eight at a time: the eight loads are issued together, then consumed
// in order.  The second pass reads the same A elements again (this thread's own, from cache).
// No LDS, no atomics, nothing shared between threads: two launches are bitwise equal.  Thread
// indices past B * N return before any access, and every element of out / dhead is written.
// ---------------------------------------------------------------------------
constexpr int kDuelT = 256, kDuelChunk = 8;
constexpr int kDuelMaxActions = 64, kDuelMaxAtoms = 256;

// v[k] = row[(a0 + k) * N] for a0 + k < A (the others are never read)
__device__ __forceinline__ void duel_load(const float* row, int a0, int A, int N,
                                          float (&v)[kDuelChunk]) {
#pragma unroll
  for (int k = 0; k < kDuelChunk; ++k) v[k] = a0 + k < A ? row[(int64_t)(a0 + k) * N] : 0.0f;
}

// the sequential sum over actions of row[a * N]
__device__ __forceinline__ float duel_sum(const float* row, int A, int N) {
  float s = 0.0f;
  for (int a0 = 0; a0 < A; a0 += kDuelChunk) {
    float v[kDuelChunk];
    duel_load(row, a0, A, N, v);
#pragma unroll
    for (int k = 0; k < kDuelChunk; ++k)
      if (a0 + k < A) s = a0 + k == 0 ? v[k] : __fadd_rn(s, v[k]);
  }
  return s;
}

__global__ __launch_bounds__(kDuelT) void k_dueling_fwd(const float* head, int B, int A, int N,
                                                        float* out) {
  const int64_t i = (int64_t)blockIdx.x * kDuelT + threadIdx.x;
  if (i >= (int64_t)B * N) return;
  const int64_t b = i / N;
  const int z = (int)(i - b * N);
  const float* adv = head + b * (A + 1) * N + z;
  const float val = adv[(int64_t)A * N];
  const float m = __fdiv_rn(duel_sum(adv, A, N), (float)A);
  float* o = out + b * A * N + z;
  for (int a0 = 0; a0 < A; a0 += kDuelChunk) {
    float v[kDuelChunk];
    duel_load(adv, a0, A, N, v);
#pragma unroll
    for (int k = 0; k < kDuelChunk; ++k)
      if (a0 + k < A) o[(int64_t)(a0 + k) * N] = __fadd_rn(__fsub_rn(v[k], m), val);
  }
}

__global__ __launch_bounds__(kDuelT) void k_dueling_bwd(const float* dout, int B, int A, int N,
                                                        float* dhead) {
  const int64_t i = (int64_t)blockIdx.x * kDuelT + threadIdx.x;
  if (i >= (int64_t)B * N) return;
  const int64_t b = i / N;
  const int z = (int)(i - b * N);
  const float* g = dout + b * A * N + z;
  const float dval = duel_sum(g, A, N);
  const float q = __fdiv_rn(dval, (float)A);
  float* d = dhead + b * (A + 1) * N + z;
  for (int a0 = 0; a0 < A; a0 += kDuelChunk) {
    float v[kDuelChunk];
    duel_load(g, a0, A, N, v);
#pragma unroll
    for (int k = 0; k < kDuelChunk; ++k)
      if (a0 + k < A) d[(int64_t)(a0 + k) * N] = __fsub_rn(v[k], q);
  }
  d[(int64_t)A * N] = dval;
}

static int duel_check(const float* in, int32_t batch, int32_t num_actions, int32_t num_atoms,
                      float* out) {
  DQ_CHECK_ARG(in && out, "null argument");
  DQ_CHECK_ARG(num_actions >= 1 && num_actions <= kDuelMaxActions,
               "num_actions must be in [1, 64]");
  DQ_CHECK_ARG(num_atoms >= 1 && num_atoms <= kDuelMaxAtoms, "num_atoms must be in [1, 256]");
  DQ_CHECK_ARG(batch >= 1, "bad batch");
  DQ_CHECK_ARG(batch <= INT32_MAX / kDuelMaxAtoms, "batch * num_atoms must fit 31 bits");
  DQ_CHECK_ARG(in != out, "the output may not alias the input");
  return DQ_OK;
}

static dim3 duel_grid(int32_t batch, int32_t num_atoms) {
  return dim3((unsigned)(((int64_t)batch * num_atoms + kDuelT - 1) / kDuelT));
}

}  // namespace dq

using namespace dq;

extern "C" {

int dq_dueling_forward(const float* head, int32_t batch, int32_t num_actions, int32_t num_atoms,
                       float* out, void* stream) {
  const int rc = duel_check(head, batch, num_actions, num_atoms, out);
  if (rc != DQ_OK) return rc;
  hipLaunchKernelGGL(k_dueling_fwd, duel_grid(batch, num_atoms), dim3(kDuelT), 0,
                     (hipStream_t)stream, head, batch, num_actions, num_atoms, out);
  DQ_CHECK_LAUNCH("k_dueling_fwd");
  return DQ_OK;
}

int dq_dueling_backward(const float* dout, int32_t batch, int32_t num_actions, int32_t num_atoms,
                        float* dhead, void* stream) {
  const int rc = duel_check(dout, batch, num_actions, num_atoms, dhead);
  if (rc != DQ_OK) return rc;
  hipLaunchKernelGGL(k_dueling_bwd, duel_grid(batch, num_atoms), dim3(kDuelT), 0,
                     (hipStream_t)stream, dout, batch, num_actions, num_atoms, dhead);
  DQ_CHECK_LAUNCH("k_dueling_bwd");
  return DQ_OK;
}

}  // extern "C"
