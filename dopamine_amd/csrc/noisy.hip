// Factorised-Gaussian noisy layers (dq_noisy_draw / k_noisy_draw, dq_noisy_weights and
// dq_noisy_grads / k_noisy_apply) for the classic-control MLP: the noise generator, the
// effective parameters the MLP kernels then read, and the sigma gradients.
// A translation unit of its own, so the other units' code objects stay what they were.
#include "common.h"

namespace dq {
namespace noisy {

// ---------------------------------------------------------------------------
// NoisyNet (Fortunato et al., ICLR 2018, section 3 (b), eq. 10-11).  A dense layer of p inputs
// and q outputs has parameters mu_w (q, p), mu_b (q), sigma_w (q, p), sigma_b (q) and noise
// f_in (p), f_out (q), f(n) = sgn(n) sqrt(|n|) of standard normals n:
//   e[j, k] = f_out[j] * f_in[k]
//   w[j, k] = mu_w[j, k] + sigma_w[j, k] * e[j, k]        b[j] = mu_b[j] + sigma_b[j] * f_out[j]
//   d sigma_w[j, k] = dw[j, k] * e[j, k]                  d sigma_b[j] = db[j] * f_out[j]
// (d mu = dw, db: dq_mlp_backward writes them straight into the mu slots.)
// The noise buffer of a network is layer-major, [f_in_0 (D) | f_out_0 | f_in_1 | f_out_1 | ...],
// and element i of it is draw i of one generator call.
// The fp32 orders (tests/noisy_cases.py restates them): e is one rounded product, f_out first;
// w = mu + (sigma * e), a rounded product then a rounded sum, never contracted.
// ---------------------------------------------------------------------------

constexpr int kT = 256;          // threads of a block, every kernel here
constexpr int kPer = 4;          // consecutive elements per thread of k_noisy_apply
constexpr int kSegs = 2 * (DQ_MLP_MAX_LAYERS + 1);

// draw i of call `call` of generator `seed`: iqn.hip's uniform_of hash (splitmix64's finaliser
// on seed + call * golden + (i + 1) * 0xD1B5...), all 64 bits returned
__device__ __forceinline__ uint64_t hash_of(uint64_t seed, int64_t call, int64_t i) {
  uint64_t z = seed + (uint64_t)call * 0x9E3779B97F4A7C15ull +
               (uint64_t)(i + 1) * 0xD1B54A32D192ED03ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

// Box-Muller on two 24-bit fields of one hash, then f:
//   u1 = (k1 + 1) * 2^-24 in (0, 1], u2 = k2 * 2^-24 in [0, 1)  (both exact in float32)
//   n  = sqrt(-2 ln u1) * cos(2 pi u2)
// cospif on 2 * u2 (exact) reduces its argument exactly; cosf of the rounded product
// 2 pi u2 would carry that product's rounding (up to 3.7e-7 in the angle) into n.
__device__ __forceinline__ float noise_of(uint64_t seed, int64_t call, int64_t i) {
  const uint64_t z = hash_of(seed, call, i);
  const float u1 = __fmul_rn((float)((uint32_t)(z >> 40) + 1u), 1.0f / 16777216.0f);
  const float u2 = __fmul_rn((float)((uint32_t)(z >> 16) & 0xFFFFFFu), 1.0f / 16777216.0f);
  const float r = sqrt_rn(__fmul_rn(-2.0f, logf(u1)));
  const float n = __fmul_rn(r, cospif(__fmul_rn(2.0f, u2)));
  return copysignf(sqrt_rn(fabsf(n)), n);
}

// out[i] = f(n_i) of call counter[0], i < n; then counter[0] += 1 inside this launch by a
// last-block ticket on counter[1] (zero between launches).  Every thread has consumed its read
// of counter[0] before its block's barrier, a block takes its ticket after that barrier, and
// only the block that takes the last ticket writes counter[0]: no read races the write.
__global__ __launch_bounds__(kT) void k_noisy_draw(int64_t* counter, uint64_t seed, int64_t n,
                                                   float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  const int64_t call = counter[0];
  if (i < n) out[i] = noise_of(seed, call, i);
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    unsigned long long* ticket = (unsigned long long*)(counter + 1);
    if (atomicAdd(ticket, 1ull) == (unsigned long long)gridDim.x - 1) {
      atomicExch(ticket, 0ull);
      counter[0] = call + 1;
    }
  }
}

// One segment = one layer's weight matrix (q * p elements, row j = element / p) or its bias
// (q elements, p = 0).  Blocks [block0, block0 of the next segment) cover it, kT * kPer
// elements each.
struct Seg {
  const float* a;        // weights: mu;     grads: d mu
  const float* s;        // weights: sigma;  grads: unused
  float* o;              // weights: eff;    grads: d sigma
  int32_t n;             // elements
  int32_t p;             // inputs (0: a bias segment)
  int32_t fin, fout;     // offsets of f_in / f_out in the noise buffer
  int32_t block0;
  int32_t pad_;
};

struct Segs {
  Seg seg[kSegs];
  int32_t count;
};

template <bool kGrads>
__device__ __forceinline__ float apply1(float a, float s, float e) {
  return kGrads ? __fmul_rn(a, e) : __fadd_rn(a, __fmul_rn(s, e));
}

// kGrads false: o = a + s * e (the effective parameters); true: o = a * e (the sigma
// gradients).  e = f_out[j] * f_in[k] for a weight, f_out[j] for a bias.  A thread takes kPer
// consecutive elements of its segment: float4 loads and one float4 store where all four lie
// inside the segment (slices start 16-byte aligned), element by element at its ragged end, so
// the slice's padding is never written.  Nothing is shared between threads.
template <bool kGrads>
__global__ __launch_bounds__(kT) void k_noisy_apply(const Segs t, const float* __restrict__ noise) {
  int si = 0;
  for (int i = 1; i < kSegs; ++i)
    if (i < t.count && (int)blockIdx.x >= t.seg[i].block0) si = i;
  const Seg g = t.seg[si];
  const int i0 = (((int)blockIdx.x - g.block0) * kT + (int)threadIdx.x) * kPer;
  if (i0 >= g.n) return;
  const bool bias = g.p == 0;
  int j = bias ? i0 : i0 / g.p;
  int k = bias ? 0 : i0 - j * g.p;
  float e[kPer];
#pragma unroll
  for (int c = 0; c < kPer; ++c) {
    e[c] = 0.0f;
    if (i0 + c < g.n) {
      const float fo = noise[g.fout + j];
      e[c] = bias ? fo : __fmul_rn(fo, noise[g.fin + k]);
    }
    if (bias) {
      ++j;
    } else if (++k == g.p) {
      k = 0;
      ++j;
    }
  }
  if (i0 + kPer <= g.n) {
    const float4 a = *reinterpret_cast<const float4*>(g.a + i0);
    float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!kGrads) s = *reinterpret_cast<const float4*>(g.s + i0);
    *reinterpret_cast<float4*>(g.o + i0) =
        make_float4(apply1<kGrads>(a.x, s.x, e[0]), apply1<kGrads>(a.y, s.y, e[1]),
                    apply1<kGrads>(a.z, s.z, e[2]), apply1<kGrads>(a.w, s.w, e[3]));
    return;
  }
#pragma unroll
  for (int c = 0; c < kPer; ++c)
    if (i0 + c < g.n) g.o[i0 + c] = apply1<kGrads>(g.a[i0 + c], kGrads ? 0.0f : g.s[i0 + c], e[c]);
}

static int check_geometry(const dq_mlp_params* p, const char* what) {
  DQ_CHECK_ARG(p != nullptr, what);
  DQ_CHECK_ARG(p->in_dim >= 1 && p->in_dim <= DQ_MLP_MAX_IN, "dq_noisy: in_dim must be in 1..16");
  DQ_CHECK_ARG(p->n_layers >= 1 && p->n_layers <= DQ_MLP_MAX_LAYERS,
               "dq_noisy: n_layers must be in 1..4");
  for (int l = 0; l < p->n_layers; ++l)
    DQ_CHECK_ARG(p->width[l] >= 1 && p->width[l] <= DQ_MLP_MAX_WIDTH,
                 "dq_noisy: every width must be in 1..1024");
  DQ_CHECK_ARG(p->n_out >= 1 && p->n_out <= DQ_MLP_MAX_WIDTH, "dq_noisy: n_out must be in 1..1024");
  return DQ_OK;
}

static bool same_geometry(const dq_mlp_params* a, const dq_mlp_params* b) {
  if (a->in_dim != b->in_dim || a->n_layers != b->n_layers || a->n_out != b->n_out) return false;
  for (int l = 0; l < a->n_layers; ++l)
    if (a->width[l] != b->width[l]) return false;
  return true;
}

// every pointer set and 16-byte aligned (the flat buffers' slices are; the float4 accesses)
static bool has_ptrs(const dq_mlp_params* p) {
  for (int l = 0; l <= p->n_layers; ++l)
    if (p->w[l] == nullptr || p->b[l] == nullptr || (uintptr_t)p->w[l] % 16 != 0 ||
        (uintptr_t)p->b[l] % 16 != 0)
      return false;
  return true;
}

static bool aliases(const dq_mlp_params* a, const dq_mlp_params* b) {
  for (int l = 0; l <= a->n_layers; ++l)
    for (int m = 0; m <= a->n_layers; ++m)
      if (a->w[l] == b->w[m] || a->b[l] == b->b[m] || a->w[l] == b->b[m] || a->b[l] == b->w[m])
        return true;
  return false;
}

// the segment table of geometry p over (a, s, o) -> the launch's block count
static int build_segs(const dq_mlp_params* p, const dq_mlp_params* a, const dq_mlp_params* s,
                      const dq_mlp_params* o, Segs* t) {
  const int per = kT * kPer;
  int blocks = 0, off = 0, n = 0;
  for (int l = 0; l <= p->n_layers; ++l) {
    const int in = l == 0 ? p->in_dim : p->width[l - 1];
    const int out = l < p->n_layers ? p->width[l] : p->n_out;
    Seg w = {a->w[l], s ? s->w[l] : nullptr, o->w[l], out * in, in, off, off + in, blocks, 0};
    blocks += (w.n + per - 1) / per;
    Seg b = {a->b[l], s ? s->b[l] : nullptr, o->b[l], out, 0, off, off + in, blocks, 0};
    blocks += (b.n + per - 1) / per;
    t->seg[n++] = w;
    t->seg[n++] = b;
    off += in + out;
  }
  t->count = n;
  return blocks;
}

}  // namespace noisy
}  // namespace dq

using namespace dq;
using namespace dq::noisy;

extern "C" {

int dq_noisy_draw(int64_t* counter, uint64_t seed, int64_t n, float* out, void* stream) {
  DQ_CHECK_ARG(counter != nullptr && out != nullptr, "dq_noisy_draw: null argument");
  DQ_CHECK_ARG(n >= 1 && n <= ((int64_t)1 << 31), "dq_noisy_draw: n must be in [1, 2^31]");
  hipLaunchKernelGGL(k_noisy_draw, dim3((unsigned)((n + kT - 1) / kT)), dim3(kT), 0,
                     (hipStream_t)stream, counter, seed, n, out);
  DQ_CHECK_LAUNCH("k_noisy_draw");
  return DQ_OK;
}

int dq_noisy_weights(const dq_mlp_params* mu, const dq_mlp_params* sigma, const float* noise,
                     const dq_mlp_params* eff, void* stream) {
  if (int rc = check_geometry(mu, "dq_noisy_weights: null mu")) return rc;
  DQ_CHECK_ARG(sigma != nullptr && eff != nullptr && noise != nullptr,
               "dq_noisy_weights: null argument");
  DQ_CHECK_ARG(same_geometry(mu, sigma) && same_geometry(mu, eff),
               "dq_noisy_weights: mu, sigma and eff must have one geometry");
  DQ_CHECK_ARG(has_ptrs(mu) && has_ptrs(sigma) && has_ptrs(eff),
               "dq_noisy_weights: null or unaligned parameter pointer");
  DQ_CHECK_ARG(!aliases(eff, mu) && !aliases(eff, sigma),
               "dq_noisy_weights: eff may not alias mu or sigma");
  Segs t = {};
  const int blocks = build_segs(mu, mu, sigma, eff, &t);
  hipLaunchKernelGGL(k_noisy_apply<false>, dim3((unsigned)blocks), dim3(kT), 0,
                     (hipStream_t)stream, t, noise);
  DQ_CHECK_LAUNCH("k_noisy_apply<weights>");
  return DQ_OK;
}

int dq_noisy_grads(const dq_mlp_params* geometry, const dq_mlp_params* g_mu,
                   const dq_mlp_params* g_sigma, const float* noise, void* stream) {
  if (int rc = check_geometry(geometry, "dq_noisy_grads: null geometry")) return rc;
  DQ_CHECK_ARG(g_mu != nullptr && g_sigma != nullptr && noise != nullptr,
               "dq_noisy_grads: null argument");
  DQ_CHECK_ARG(same_geometry(geometry, g_mu) && same_geometry(geometry, g_sigma),
               "dq_noisy_grads: g_mu and g_sigma must have the geometry given");
  DQ_CHECK_ARG(has_ptrs(g_mu) && has_ptrs(g_sigma),
               "dq_noisy_grads: null or unaligned gradient pointer");
  DQ_CHECK_ARG(!aliases(g_sigma, g_mu), "dq_noisy_grads: g_sigma may not alias g_mu");
  Segs t = {};
  const int blocks = build_segs(geometry, g_mu, nullptr, g_sigma, &t);
  hipLaunchKernelGGL(k_noisy_apply<true>, dim3((unsigned)blocks), dim3(kT), 0,
                     (hipStream_t)stream, t, noise);
  DQ_CHECK_LAUNCH("k_noisy_apply<grads>");
  return DQ_OK;
}

}  // extern "C"
