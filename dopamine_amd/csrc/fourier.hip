// The Fourier-basis Q-network (reference gym_lib.py:135-206: FourierBasis,
// fourier_dqn_network; 276-292: the CartPole / Acrobot instances): the observation scaled to
// [0, 1], F = (order + 1)^D - 1 cosine features, a bias-free linear head -- the network's only
// parameter.  The work is ~1M cosines and 6 MFLOP at batch 256 on Acrobot (F = 4,095), launch-
// and latency-bound like the MLPs beside it, and shaped like nothing in mlp.hip: as matrix
// tiles the head is one tile column with a serial K loop over F.  So the forward is ONE launch
// (scale, features, head: a block per sample, the features never leave registers but for the
// copy the backward reads) and the backward ONE launch (the head's weight gradient).
//
// fp32 in every build, in explicit __f*_rn operations; no atomics, no memset, no workspace;
// every reduction has one order, every gradient element is a plain store.
#include "common.h"

namespace dq {
namespace fourier {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kActs = 4;             // outputs accumulated per pass, in registers
constexpr int kAhead = 4;            // features (forward) / batch rows (backward) loaded ahead

struct FwdArgs {
  const void* x;
  const float* w;
  float* s;
  float* phi;
  float* out;
  int32_t D, base, F, A, is_f64;
  uint32_t inv;      // ceil(2^32 / base): n / base == umulhi(n, inv) for n <= 2^14 (see reciprocal)
  float in_min[DQ_FOURIER_MAX_IN], in_range[DQ_FOURIER_MAX_IN];
};

// Feature f of a sample: the digits of f + 1 in base order + 1 are its multipliers, dimension
// 0 the most significant (gym_lib.py:153-157); z = sum_d m_d s_d in d order, phi =
// cos(float32(pi) z) (gym_lib.py:169: np.pi enters the graph as a float32 constant).  cosf
// reduces its argument (|arg| reaches 18 pi on Acrobot).
// The digits come least significant first, by a multiplication (a 32-bit division is ~30
// instructions, and there are D per feature), and without a branch: sr holds s reversed --
// sr[i] = s[D - 1 - i], zero from i = D on -- and f + 1 < base^D leaves n = 0 after D digits,
// so the kD - D steps past the input add 0 * 0 to z and change no bit of it.  (Guarding every
// step with d < D instead cost 32 branches per feature: 13.6 us against 8.4 us per launch at
// batch 256 on Acrobot.)
template <int kD>
__device__ __forceinline__ float feature(int f, int base, uint32_t inv, const float (&sr)[kD]) {
  unsigned n = (unsigned)f + 1u;
  float m[kD];
#pragma unroll
  for (int i = 0; i < kD; ++i) {
    const unsigned q = __umulhi(n, inv);
    m[i] = (float)(n - q * (unsigned)base);
    n = q;
  }
  float z = 0.0f;
#pragma unroll
  for (int i = kD - 1; i >= 0; --i) z = __fadd_rn(z, __fmul_rn(m[i], sr[i]));   // d = 0 first
  return cosf(__fmul_rn(3.14159274101257324f, z));
}

// One block per sample.  Thread t takes features t, t + 256, ... in increasing order and
// accumulates phi W[a][f] for kActs outputs at a time (W read coalesced along f); the block's
// 256 partials per output are summed within each wave, then the four waves in wave order.
// Further passes (A > 4) form the same features again; pass 0 stores them.  kD: 4, 8 or 16,
// the smallest that holds D.
template <int kD>
__global__ __launch_bounds__(kThreads) void k_fourier_fwd(const FwdArgs a) {
  __shared__ float sh_sr[DQ_FOURIER_MAX_IN];
  __shared__ float red[kWaves][kActs];
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  const int64_t b = blockIdx.x;
  if (t < DQ_FOURIER_MAX_IN) {
    if (t < a.D) {
      const int64_t at = b * a.D + t;
      const float xv = a.is_f64 ? (float)((const double*)a.x)[at] : ((const float*)a.x)[at];
      const float v = __fdiv_rn(__fsub_rn(xv, a.in_min[t]), a.in_range[t]);
      if (a.s != nullptr) a.s[at] = v;
      sh_sr[a.D - 1 - t] = v;
    } else {
      sh_sr[t] = 0.0f;
    }
  }
  __syncthreads();
  float s[kD];
#pragma unroll
  for (int i = 0; i < kD; ++i) s[i] = sh_sr[i];

  for (int a0 = 0; a0 < a.A; a0 += kActs) {
    float acc[kActs];
#pragma unroll
    for (int j = 0; j < kActs; ++j) acc[j] = 0.0f;
    // kAhead features' weights are loaded together, ahead of the cosines that use them: one
    // round of global-load latency per kAhead features instead of one per feature (the block
    // is one wave per SIMD, so nothing else hides it)
    for (int f0 = t; f0 < a.F; f0 += kAhead * kThreads) {
      float wv[kAhead][kActs];
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const int f = min(f0 + u * kThreads, a.F - 1);
#pragma unroll
        for (int j = 0; j < kActs; ++j)
          wv[u][j] = a.w[(int64_t)min(a0 + j, a.A - 1) * a.F + f];
      }
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const int f = f0 + u * kThreads;
        if (f < a.F) {
          const float phi = feature<kD>(f, a.base, a.inv, s);
          if (a0 == 0 && a.phi != nullptr) a.phi[b * a.F + f] = phi;
#pragma unroll
          for (int j = 0; j < kActs; ++j)
            if (a0 + j < a.A) acc[j] = __fadd_rn(acc[j], __fmul_rn(phi, wv[u][j]));
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kActs; ++j) {
      const float v = wave_sum(acc[j]);
      if (lane == 0) red[wv][j] = v;
    }
    __syncthreads();
    if (t < kActs && a0 + t < a.A) {
      float v = red[0][t];
#pragma unroll
      for (int q = 1; q < kWaves; ++q) v = __fadd_rn(v, red[q][t]);
      a.out[b * a.A + a0 + t] = v;
    }
    __syncthreads();
  }
}

// The head's weight gradient dW[a][f] = sum_b dout[b][a] phi[b][f]: threads along f (loads and
// stores coalesced), kDwFeat features per block, the batch in kDwSlices interleaved slices (a
// short serial chain per thread: the launch is latency-bound) summed 0..kDwSlices-1 through
// LDS -- k_mlp_dw0's scheme.  kActs outputs per pass, kAhead rows' loads in flight together.
// Measured per launch at Acrobot's (B, F, A) = (256, 4095, 3), back to back in a graph: 64
// features x 4 slices 16.7 us, 32 x 8 9.1, 16 x 16 5.5 (one row loaded at a time); with kAhead
// = 4: 32 x 8 6.5, 16 x 16 4.2, 8 x 32 3.2 us -- 512 blocks, two rounds of loads per thread.
constexpr int kDwFeat = 8;
constexpr int kDwSlices = kThreads / kDwFeat;

struct DwArgs {
  const float* dout;
  const float* phi;
  float* dw;
  int32_t batch, F, A, pad_;
};

__global__ __launch_bounds__(kThreads) void k_fourier_dw(const DwArgs a) {
  __shared__ float red[kDwSlices][kActs][kDwFeat];
  const int t = threadIdx.x, u = t % kDwFeat, w = t / kDwFeat;
  const int f = blockIdx.x * kDwFeat + u;
  for (int a0 = 0; a0 < a.A; a0 += kActs) {
    float acc[kActs];
#pragma unroll
    for (int j = 0; j < kActs; ++j) acc[j] = 0.0f;
    if (f < a.F) {
      for (int r0 = w; r0 < a.batch; r0 += kAhead * kDwSlices) {
        float p[kAhead], g[kAhead][kActs];
#pragma unroll
        for (int v = 0; v < kAhead; ++v) {          // kAhead rows' loads in flight together
          const int64_t r = min(r0 + v * kDwSlices, a.batch - 1);
          p[v] = a.phi[r * a.F + f];
#pragma unroll
          for (int j = 0; j < kActs; ++j) g[v][j] = a.dout[r * a.A + min(a0 + j, a.A - 1)];
        }
#pragma unroll
        for (int v = 0; v < kAhead; ++v)
          if (r0 + v * kDwSlices < a.batch) {
#pragma unroll
            for (int j = 0; j < kActs; ++j)
              if (a0 + j < a.A) acc[j] = __fadd_rn(acc[j], __fmul_rn(g[v][j], p[v]));
          }
      }
    }
#pragma unroll
    for (int j = 0; j < kActs; ++j) red[w][j][u] = acc[j];
    __syncthreads();
    if (t < kActs * kDwFeat) {
      const int j = t / kDwFeat, uu = t % kDwFeat;
      const int ff = blockIdx.x * kDwFeat + uu;
      if (a0 + j < a.A && ff < a.F) {
        float v = red[0][j][uu];
#pragma unroll
        for (int q = 1; q < kDwSlices; ++q) v = __fadd_rn(v, red[q][j][uu]);
        a.dw[(int64_t)(a0 + j) * a.F + ff] = v;
      }
    }
    __syncthreads();
  }
}

// inv = ceil(2^32 / base), 2 <= base <= 2^14.  With e = inv base - 2^32 in [0, base):
// n inv / 2^32 = n / base + n e / (base 2^32), and for n <= 2^14 the second term is below
// 2^-18 while n / base falls short of the next integer by at least 1 / base >= 2^-14, so the
// floor is floor(n / base).
static uint32_t reciprocal(int base) {
  return (uint32_t)((((uint64_t)1 << 32) + (uint64_t)base - 1) / (uint64_t)base);
}

static int features_of(int32_t in_dim, int32_t order) {
  if (in_dim < 1 || in_dim > DQ_FOURIER_MAX_IN || order < 1) return 0;
  int64_t n = 1;
  for (int d = 0; d < in_dim; ++d) {
    n *= (int64_t)order + 1;
    if (n - 1 > DQ_FOURIER_MAX_FEATURES) return 0;
  }
  return (int)(n - 1);
}

static int check_params(const dq_fourier_params* p, int32_t batch) {
  DQ_CHECK_ARG(p != nullptr, "dq_fourier: null params");
  DQ_CHECK_ARG(p->in_dim >= 1 && p->in_dim <= DQ_FOURIER_MAX_IN,
               "dq_fourier: in_dim must be in 1..16");
  DQ_CHECK_ARG(p->order >= 1, "dq_fourier: order must be >= 1");
  DQ_CHECK_ARG(features_of(p->in_dim, p->order) > 0,
               "dq_fourier: (order + 1)^in_dim - 1 features exceed 16383");
  DQ_CHECK_ARG(p->n_out >= 1 && p->n_out <= DQ_FOURIER_MAX_OUT,
               "dq_fourier: n_out must be in 1..64");
  DQ_CHECK_ARG(batch >= 1, "dq_fourier: batch must be >= 1");
  return DQ_OK;
}

}  // namespace fourier
}  // namespace dq

using namespace dq;
using namespace dq::fourier;

extern "C" {

int dq_fourier_features(int32_t in_dim, int32_t order) { return features_of(in_dim, order); }

int dq_fourier_forward(const dq_fourier_params* p, int32_t batch, const void* x, int32_t x_is_f64,
                       dq_fourier_acts* acts, void* stream) {
  if (int rc = check_params(p, batch)) return rc;
  DQ_CHECK_ARG(p->w != nullptr, "dq_fourier_forward: null w");
  DQ_CHECK_ARG(x != nullptr, "dq_fourier_forward: null x");
  DQ_CHECK_ARG(acts != nullptr && acts->out != nullptr, "dq_fourier_forward: null out");
  FwdArgs k = {};
  k.x = x; k.w = p->w; k.s = acts->s; k.phi = acts->phi; k.out = acts->out;
  k.D = p->in_dim; k.base = p->order + 1; k.F = features_of(p->in_dim, p->order);
  k.A = p->n_out; k.is_f64 = x_is_f64 != 0; k.inv = reciprocal(k.base);
  for (int d = 0; d < DQ_FOURIER_MAX_IN; ++d) {
    k.in_min[d] = d < p->in_dim ? p->in_min[d] : 0.0f;
    k.in_range[d] = d < p->in_dim ? p->in_range[d] : 1.0f;
  }
  auto kern = k.D <= 4 ? k_fourier_fwd<4> : k.D <= 8 ? k_fourier_fwd<8> : k_fourier_fwd<16>;
  hipLaunchKernelGGL(kern, dim3((unsigned)batch), dim3(kThreads), 0, (hipStream_t)stream, k);
  DQ_CHECK_LAUNCH("k_fourier_fwd");
  return DQ_OK;
}

int dq_fourier_backward(const dq_fourier_params* p, const dq_fourier_params* g, int32_t batch,
                        const dq_fourier_acts* acts, const float* dout, void* stream) {
  if (int rc = check_params(p, batch)) return rc;
  DQ_CHECK_ARG(g != nullptr && g->w != nullptr, "dq_fourier_backward: null g->w");
  DQ_CHECK_ARG(acts != nullptr && acts->phi != nullptr, "dq_fourier_backward: null phi");
  DQ_CHECK_ARG(dout != nullptr, "dq_fourier_backward: null dout");
  DwArgs k = {};
  k.dout = dout; k.phi = acts->phi; k.dw = g->w;
  k.batch = batch; k.F = features_of(p->in_dim, p->order); k.A = p->n_out;
  hipLaunchKernelGGL(k_fourier_dw, dim3((unsigned)((k.F + kDwFeat - 1) / kDwFeat)), dim3(kThreads),
                     0, (hipStream_t)stream, k);
  DQ_CHECK_LAUNCH("k_fourier_dw");
  return DQ_OK;
}

}  // extern "C"
