// The classic-control MLP (reference gym_lib.py:75-110, _basic_discrete_domain_network) on the
// exact-fp32 matrix cores: rescale + layer 0 in one VALU launch (K = D <= 16), every other
// layer's forward, input gradient and weight + bias gradient as 32 x 32 output tiles of
// v_mfma_f32_32x32x2_f32 with the 64-wide K window split across the block's four waves.
//
// The whole step is launch-bound (two forwards and a backward at batch 128 are ~67 MFLOP),
// so the tiles are small -- 64 blocks for a 128 x 512 layer, 272 for a 512 x 512 weight
// gradient -- and a layer's dW and dX are groups of ONE launch: the forward is L + 1
// launches, the backward L + 1.  Every reduction has a fixed order (one accumulator chain per
// wave, the four waves summed 0..3), every gradient is written by plain stores: bitwise
// reproducible, no workspace, no memset, no atomics.  The arithmetic is fp32 in every build
// (no bf16 split here: the throughput build's switches do not reach this file).
#include "common.h"

namespace dq {
namespace mlp {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTile = 32;            // output tile (rows = cols)
constexpr int kWin = 64;             // K window staged per round: 16 per wave
constexpr int kPitch = kTile + 1;    // LDS row pitch (odd: conflict-free either way round)
constexpr int kThreads = 256;
constexpr int kWaveK = kWin / (kThreads / 64);         // a wave's share of the window
constexpr int kFetch = kWin * kTile / kThreads;        // elements per thread, window and operand

enum { kFwd = 0, kDx = 1, kDw = 2 };

// C(m, n) = sum_k A(m, k) B(k, n) over generic strides, then the mode's epilogue:
//   kFwd  C = [relu](acc + aux[n])                  A = input (M=B, K), B = W viewed (K, N)
//   kDx   C = aux[m, n] > 0 ? acc : 0               A = dz (B, N_l), B = W (N_l, K_l)
//   kDw   C = acc, and column N: db[m] = sum_k A    A = dz viewed (N_l, B), B = input (B, K_l)
// (the bias gradient is the product with an extra all-ones column of B).
struct MlpOp {
  const float* A;
  const float* B;
  float* C;
  const float* aux;
  float* db;
  int64_t sAm, sAk, sBk, sBn;
  int32_t M, N, K, ldc;
  int32_t mode, relu, a_kc, b_kc;    // a_kc / b_kc: the operand is contiguous along k
  int32_t tiles_n, blocks;
};

struct MlpGroup {
  MlpOp op[2];
  int32_t count, pad_;
};

__device__ __forceinline__ void tile_fetch(const MlpOp& o, int m0, int n0, int k0, int t,
                                           float (&ra)[kFetch], float (&rb)[kFetch]) {
  const int ncols = o.mode == kDw ? o.N + 1 : o.N;
#pragma unroll
  for (int r = 0; r < kFetch; ++r) {
    int i, k;
    if (o.a_kc) { k = t % kWin; i = t / kWin + (kThreads / kWin) * r; }
    else { i = t % kTile; k = t / kTile + (kThreads / kTile) * r; }
    const int gm = m0 + i, gk = k0 + k;
    ra[r] = (gm < o.M && gk < o.K) ? o.A[gm * o.sAm + gk * o.sAk] : 0.0f;
    if (o.b_kc) { k = t % kWin; i = t / kWin + (kThreads / kWin) * r; }
    else { i = t % kTile; k = t / kTile + (kThreads / kTile) * r; }
    const int gn = n0 + i;
    const int gkb = k0 + k;
    float v = 0.0f;
    if (gkb < o.K && gn < ncols) v = gn < o.N ? o.B[gkb * o.sBk + gn * o.sBn] : 1.0f;
    rb[r] = v;
  }
}

__device__ __forceinline__ void tile_stash(const MlpOp& o, int t, const float (&ra)[kFetch],
                                           const float (&rb)[kFetch], float* As, float* Bs) {
#pragma unroll
  for (int r = 0; r < kFetch; ++r) {
    int i, k;
    if (o.a_kc) { k = t % kWin; i = t / kWin + (kThreads / kWin) * r; }
    else { i = t % kTile; k = t / kTile + (kThreads / kTile) * r; }
    As[k * kPitch + i] = ra[r];
    if (o.b_kc) { k = t % kWin; i = t / kWin + (kThreads / kWin) * r; }
    else { i = t % kTile; k = t / kTile + (kThreads / kTile) * r; }
    Bs[k * kPitch + i] = rb[r];
  }
}

__global__ __launch_bounds__(kThreads) void k_mlp_tiles(const MlpGroup g) {
  __shared__ float smem[2 * kWin * kPitch];          // A and B windows; then the 4 waves' tiles
  int blk = blockIdx.x;
  int which = 0;
  if (g.count > 1 && blk >= g.op[0].blocks) { which = 1; blk -= g.op[0].blocks; }
  const MlpOp& o = g.op[which];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int m0 = (blk / o.tiles_n) * kTile, n0 = (blk % o.tiles_n) * kTile;
  float* As = smem;
  float* Bs = smem + kWin * kPitch;

  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
  float ra[kFetch], rb[kFetch];
  tile_fetch(o, m0, n0, 0, t, ra, rb);
  const float* pa = As + (kWaveK * w + (lane >> 5)) * kPitch + (lane & 31);
  const float* pb = Bs + (kWaveK * w + (lane >> 5)) * kPitch + (lane & 31);
  for (int k0 = 0; k0 < o.K; k0 += kWin) {
    tile_stash(o, t, ra, rb, As, Bs);
    __syncthreads();
    if (k0 + kWin < o.K) tile_fetch(o, m0, n0, k0 + kWin, t, ra, rb);
    if (k0 + kWaveK * w < o.K) {                         // wave-uniform: bands past the end are zero
#pragma unroll
      for (int s = 0; s < kWaveK; s += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[s * kPitch], pb[s * kPitch], acc, 0, 0, 0);
    }
    __syncthreads();
  }
  // C/D layout of the 32x32 f32 MFMA: col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
  float* red = smem + w * kTile * kPitch;
#pragma unroll
  for (int e = 0; e < 16; ++e)
    red[((e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)) * kPitch + (lane & 31)] = acc[e];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = t + kThreads * q, row = e >> 5, col = e & 31;
    const float* p = smem + row * kPitch + col;
    float v = p[0];
    v += p[kTile * kPitch];
    v += p[2 * kTile * kPitch];
    v += p[3 * kTile * kPitch];
    const int gm = m0 + row, gn = n0 + col;
    if (gm >= o.M) continue;
    if (o.mode == kFwd) {
      if (gn >= o.N) continue;
      v += o.aux[gn];
      if (o.relu) v = v > 0.0f ? v : 0.0f;
      o.C[(int64_t)gm * o.ldc + gn] = v;
    } else if (o.mode == kDx) {
      if (gn >= o.N) continue;
      const int64_t at = (int64_t)gm * o.ldc + gn;
      o.C[at] = o.aux[at] > 0.0f ? v : 0.0f;
    } else {
      if (gn < o.N) o.C[(int64_t)gm * o.ldc + gn] = v;
      else if (gn == o.N) o.db[gm] = v;
    }
  }
}

// Launch 1 of the forward: cast, rescale (gym_lib.py:104-108) and layer 0, one thread per
// (sample, unit); the unit-0 threads store the rescaled input for layer 0's weight gradient.
struct MlpIn {
  const void* x;
  float* x0;
  const float* w;
  const float* b;
  float* h;
  int32_t batch, D, N, is_f64;
  float in_min[DQ_MLP_MAX_IN], in_range[DQ_MLP_MAX_IN];
};

__global__ __launch_bounds__(kThreads) void k_mlp_layer0(const MlpIn a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)a.batch * a.N) return;
  const int64_t row = i / a.N;
  const int n = (int)(i - row * a.N);
  float acc = a.b[n];
  for (int d = 0; d < a.D; ++d) {
    const int64_t at = row * a.D + d;
    const float xv = a.is_f64 ? (float)((const double*)a.x)[at] : ((const float*)a.x)[at];
    float v = __fsub_rn(xv, a.in_min[d]);
    v = __fdiv_rn(v, a.in_range[d]);
    v = __fsub_rn(__fmul_rn(2.0f, v), 1.0f);
    if (n == 0) a.x0[at] = v;
    acc = __fadd_rn(acc, __fmul_rn(a.w[n * a.D + d], v));
  }
  a.h[i] = acc > 0.0f ? acc : 0.0f;
}

// Last launch of the backward: layer 0's weight (N, D) and bias gradient from dz (B, N) and
// the rescaled input (B, D).  16 units per block, the batch in 16 interleaved slices (a short
// serial chain per thread: the launch is latency-bound) summed 0..15.
constexpr int kDw0Units = 16;
constexpr int kDw0Slices = kThreads / kDw0Units;

struct MlpDw0 {
  const float* dz;
  const float* x0;
  float* dw;
  float* db;
  int32_t batch, D, N, pad_;
};

__global__ __launch_bounds__(kThreads) void k_mlp_dw0(const MlpDw0 a) {
  __shared__ float red[kDw0Slices][DQ_MLP_MAX_IN + 1][kDw0Units];
  const int t = threadIdx.x, u = t % kDw0Units, w = t / kDw0Units;
  const int n = blockIdx.x * kDw0Units + u;
  float s[DQ_MLP_MAX_IN + 1];
#pragma unroll
  for (int d = 0; d <= DQ_MLP_MAX_IN; ++d) s[d] = 0.0f;
  if (n < a.N) {
    for (int r = w; r < a.batch; r += kDw0Slices) {
      const float g = a.dz[(int64_t)r * a.N + n];
      const float* xr = a.x0 + (int64_t)r * a.D;
#pragma unroll
      for (int d = 0; d < DQ_MLP_MAX_IN; ++d)
        if (d < a.D) s[d] = __fadd_rn(s[d], __fmul_rn(g, xr[d]));
      s[DQ_MLP_MAX_IN] += g;
    }
  }
#pragma unroll
  for (int d = 0; d <= DQ_MLP_MAX_IN; ++d) red[w][d][u] = s[d];
  __syncthreads();
  // 16 units x (D + 1) sums, unit-major so that a unit's D weights are stored together
  for (int e = t; e < kDw0Units * (a.D + 1); e += kThreads) {
    const int uu = e / (a.D + 1), d = e - uu * (a.D + 1);
    const int nn = blockIdx.x * kDw0Units + uu;
    if (nn >= a.N) continue;
    const int dd = d < a.D ? d : DQ_MLP_MAX_IN;
    float v = red[0][dd][uu];
#pragma unroll
    for (int q = 1; q < kDw0Slices; ++q) v += red[q][dd][uu];
    if (d < a.D) a.dw[(int64_t)nn * a.D + d] = v;
    else a.db[nn] = v;
  }
}

static int check_params(const dq_mlp_params* p, int32_t batch) {
  DQ_CHECK_ARG(p != nullptr, "dq_mlp: null params");
  DQ_CHECK_ARG(batch >= 1, "dq_mlp: batch must be >= 1");
  DQ_CHECK_ARG(p->in_dim >= 1 && p->in_dim <= DQ_MLP_MAX_IN, "dq_mlp: in_dim must be in 1..16");
  DQ_CHECK_ARG(p->n_layers >= 1 && p->n_layers <= DQ_MLP_MAX_LAYERS,
               "dq_mlp: n_layers must be in 1..4");
  for (int l = 0; l < p->n_layers; ++l)
    DQ_CHECK_ARG(p->width[l] >= 1 && p->width[l] <= DQ_MLP_MAX_WIDTH,
                 "dq_mlp: every width must be in 1..1024");
  DQ_CHECK_ARG(p->n_out >= 1 && p->n_out <= DQ_MLP_MAX_WIDTH, "dq_mlp: n_out must be in 1..1024");
  return DQ_OK;
}

static int check_ptrs(const dq_mlp_params* p, const char* what) {
  for (int l = 0; l <= p->n_layers; ++l)
    DQ_CHECK_ARG(p->w[l] != nullptr && p->b[l] != nullptr, what);
  return DQ_OK;
}

static int check_acts(const dq_mlp_params* p, const dq_mlp_acts* a, bool with_out, const char* what) {
  DQ_CHECK_ARG(a != nullptr, what);
  for (int l = 0; l < p->n_layers; ++l) DQ_CHECK_ARG(a->h[l] != nullptr, what);
  DQ_CHECK_ARG(!with_out || (a->x0 != nullptr && a->out != nullptr), what);
  return DQ_OK;
}

inline int out_dim(const dq_mlp_params* p, int l) { return l < p->n_layers ? p->width[l] : p->n_out; }
inline int in_dim(const dq_mlp_params* p, int l) { return l == 0 ? p->in_dim : p->width[l - 1]; }

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

static void finish(MlpOp& o) {
  const int ncols = o.mode == kDw ? o.N + 1 : o.N;
  o.tiles_n = cdiv(ncols, kTile);
  o.blocks = cdiv(o.M, kTile) * o.tiles_n;
}

// layer l >= 1 forward: out (B, N) = [relu](in (B, K) W^T + b)
static MlpOp op_forward(const dq_mlp_params* p, int32_t batch, const dq_mlp_acts* a, int l) {
  MlpOp o = {};
  const int K = in_dim(p, l), N = out_dim(p, l);
  o.A = a->h[l - 1]; o.sAm = K; o.sAk = 1; o.a_kc = 1;
  o.B = p->w[l]; o.sBk = 1; o.sBn = K; o.b_kc = 1;
  o.C = l < p->n_layers ? a->h[l] : a->out;
  o.aux = p->b[l];
  o.M = batch; o.N = N; o.K = K; o.ldc = N;
  o.mode = kFwd; o.relu = l < p->n_layers;
  finish(o);
  return o;
}

// layer l >= 1 input gradient: d->h[l-1] (B, K_l) = (dz (B, N_l) W (N_l, K_l)) . (h[l-1] > 0)
static MlpOp op_dx(const dq_mlp_params* p, int32_t batch, const dq_mlp_acts* a, const float* dz,
            dq_mlp_acts* d, int l) {
  MlpOp o = {};
  const int K = in_dim(p, l), N = out_dim(p, l);
  o.A = dz; o.sAm = N; o.sAk = 1; o.a_kc = 1;
  o.B = p->w[l]; o.sBk = K; o.sBn = 1; o.b_kc = 0;
  o.C = d->h[l - 1];
  o.aux = a->h[l - 1];
  o.M = batch; o.N = K; o.K = N; o.ldc = K;
  o.mode = kDx;
  finish(o);
  return o;
}

// layer l >= 1 weight + bias gradient: g->w[l] (N_l, K_l) = dz^T in, g->b[l] = dz^T 1
static MlpOp op_dw(const dq_mlp_params* p, const dq_mlp_params* g, int32_t batch, const dq_mlp_acts* a,
            const float* dz, int l) {
  MlpOp o = {};
  const int K = in_dim(p, l), N = out_dim(p, l);
  o.A = dz; o.sAm = 1; o.sAk = N; o.a_kc = 0;
  o.B = a->h[l - 1]; o.sBk = K; o.sBn = 1; o.b_kc = 0;
  o.C = g->w[l];
  o.db = g->b[l];
  o.M = N; o.N = K; o.K = batch; o.ldc = K;
  o.mode = kDw;
  finish(o);
  return o;
}

static int launch_tiles(const MlpOp* ops, int count, hipStream_t s) {
  MlpGroup g = {};
  int blocks = 0;
  for (int i = 0; i < count; ++i) { g.op[i] = ops[i]; blocks += ops[i].blocks; }
  g.count = count;
  hipLaunchKernelGGL(k_mlp_tiles, dim3(blocks), dim3(kThreads), 0, s, g);
  DQ_CHECK_LAUNCH("k_mlp_tiles");
  return DQ_OK;
}

static int launch_dw0(const dq_mlp_params* p, const dq_mlp_params* g, int32_t batch,
               const dq_mlp_acts* a, const float* dz, hipStream_t s) {
  MlpDw0 k = {};
  k.dz = dz; k.x0 = a->x0; k.dw = g->w[0]; k.db = g->b[0];
  k.batch = batch; k.D = p->in_dim; k.N = p->width[0];
  hipLaunchKernelGGL(k_mlp_dw0, dim3(cdiv(k.N, kDw0Units)), dim3(kThreads), 0, s, k);
  DQ_CHECK_LAUNCH("k_mlp_dw0");
  return DQ_OK;
}

static int check_backward(const dq_mlp_params* p, const dq_mlp_params* g, int32_t batch,
                   const dq_mlp_acts* a, const float* dout, const dq_mlp_acts* d) {
  if (int rc = check_params(p, batch)) return rc;
  DQ_CHECK_ARG(g != nullptr, "dq_mlp_backward: null gradient params");
  if (int rc = check_ptrs(p, "dq_mlp_backward: null parameter pointer")) return rc;
  for (int l = 0; l <= p->n_layers; ++l)
    DQ_CHECK_ARG(g->w[l] != nullptr && g->b[l] != nullptr,
                 "dq_mlp_backward: null gradient pointer");
  if (int rc = check_acts(p, a, true, "dq_mlp_backward: null activation pointer")) return rc;
  if (int rc = check_acts(p, d, false, "dq_mlp_backward: null activation-gradient pointer"))
    return rc;
  DQ_CHECK_ARG(dout != nullptr, "dq_mlp_backward: null dout");
  return DQ_OK;
}

}  // namespace mlp
}  // namespace dq

using namespace dq;
using namespace dq::mlp;

extern "C" {

size_t dq_mlp_workspace_floats(int32_t batch, const dq_mlp_params* p) {
  (void)batch;
  (void)p;
  return 0;      // every reduction finishes inside its block
}

int dq_mlp_forward(const dq_mlp_params* p, int32_t batch, const void* x, int32_t x_is_f64,
                   dq_mlp_acts* a, float* ws, void* stream) {
  (void)ws;
  if (int rc = check_params(p, batch)) return rc;
  if (int rc = check_ptrs(p, "dq_mlp_forward: null parameter pointer")) return rc;
  if (int rc = check_acts(p, a, true, "dq_mlp_forward: null activation pointer")) return rc;
  DQ_CHECK_ARG(x != nullptr, "dq_mlp_forward: null input");
  hipStream_t s = (hipStream_t)stream;
  MlpIn k = {};
  k.x = x; k.x0 = a->x0; k.w = p->w[0]; k.b = p->b[0]; k.h = a->h[0];
  k.batch = batch; k.D = p->in_dim; k.N = p->width[0]; k.is_f64 = x_is_f64 != 0;
  for (int d = 0; d < DQ_MLP_MAX_IN; ++d) {
    k.in_min[d] = d < p->in_dim ? p->in_min[d] : 0.0f;
    k.in_range[d] = d < p->in_dim ? p->in_range[d] : 1.0f;
  }
  const int64_t n = (int64_t)batch * k.N;
  DQ_CHECK_ARG((n + kThreads - 1) / kThreads <= 0x7fffffff, "dq_mlp_forward: batch too large");
  hipLaunchKernelGGL(k_mlp_layer0, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads),
                     0, s, k);
  DQ_CHECK_LAUNCH("k_mlp_layer0");
  for (int l = 1; l <= p->n_layers; ++l) {
    MlpOp o = op_forward(p, batch, a, l);
    if (int rc = launch_tiles(&o, 1, s)) return rc;
  }
  return DQ_OK;
}

int dq_mlp_backward(const dq_mlp_params* p, const dq_mlp_params* g, int32_t batch,
                    const dq_mlp_acts* a, const float* dout, dq_mlp_acts* d, float* ws,
                    void* stream) {
  (void)ws;
  if (int rc = check_backward(p, g, batch, a, dout, d)) return rc;
  hipStream_t s = (hipStream_t)stream;
  for (int l = p->n_layers; l >= 1; --l) {
    const float* dz = l == p->n_layers ? dout : d->h[l];
    MlpOp ops[2] = {op_dx(p, batch, a, dz, d, l), op_dw(p, g, batch, a, dz, l)};
    if (int rc = launch_tiles(ops, 2, s)) return rc;
  }
  return launch_dw0(p, g, batch, a, d->h[0], s);
}

int dq_mlp_backward_layer(const dq_mlp_params* p, const dq_mlp_params* g, int32_t batch,
                          const dq_mlp_acts* a, const float* dout, dq_mlp_acts* d, float* ws,
                          int32_t layer, int32_t part, void* stream) {
  (void)ws;
  if (int rc = check_backward(p, g, batch, a, dout, d)) return rc;
  DQ_CHECK_ARG(layer >= 0 && layer <= p->n_layers, "dq_mlp_backward_layer: no such layer");
  DQ_CHECK_ARG(part == 0 || part == 1, "dq_mlp_backward_layer: part must be 0 or 1");
  DQ_CHECK_ARG(!(layer == 0 && part == 0),
               "dq_mlp_backward_layer: layer 0 has no input gradient");
  hipStream_t s = (hipStream_t)stream;
  const float* dz = layer == p->n_layers ? dout : d->h[layer];
  if (layer == 0) return launch_dw0(p, g, batch, a, dz, s);
  MlpOp o = part == 1 ? op_dw(p, g, batch, a, dz, layer) : op_dx(p, batch, a, dz, d, layer);
  return launch_tiles(&o, 1, s);
}

}  // extern "C"
