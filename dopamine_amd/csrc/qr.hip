// QR-DQN's loss (dq_qr_loss / k_qr): fixed-quantile regression on the Rainbow head's layout.
// A translation unit of its own, so learner.hip's code object stays what it was; the row
// pieces (WideRow, fast_sum / fast_min) are c51_dev.h's, the optional summary mean is
// learner.hip's k_wmean, launched from here.
#include "c51_dev.h"

namespace dq {

// mean(w * loss) for summaries, defined in learner.hip
__global__ void k_wmean(const float* loss, const float* probs, int B, float* out);

// ---------------------------------------------------------------------------
// QR-DQN: fixed-quantile regression (Dabney et al., AAAI 2018, eq. 10; upstream Dopamine's
// QuantileAgent).  theta = online output (B, A, N), quantile index last (the Rainbow head's
// layout); T = target output on s'; S = select output (T itself, or the online network on s'
// with double-DQN targets); tau_i = (i + 0.5) / N:
//   a*_b    = first argmax_a (sum_i S[b, a, i]) / N
//   y_bj    = r_b + gamma^n (1 - terminal_b) T[b, a*_b, j]
//   u_bij   = y_bj - theta[b, act_b, i]
//   L_k(u)  = u^2 / 2 if |u| <= kappa else kappa (|u| - kappa / 2)   (derivative 0 at u = 0)
//   loss_b  = sum_i (1/N) sum_j |tau_i - 1{u_bij < 0}| L_k(u_bij) / kappa
//   prio_b  = sqrt(loss_b + 1e-10) of the unweighted loss
//   w_b     = (p_b + 1e-10)^-1/2 / max_b' (p_b' + 1e-10)^-1/2          (1 without probs)
//   grad    = d mean_b(w_b loss_b) / d theta, (B, A, N), zeros off the taken action
// The / kappa is IQN's form (k_iqn); at kappa = 1 it is the paper's.  The PER weight and the
// priority rule are k_c51's.
// One 256-thread block per sample b, arranged as k_c51_double:
//   before the barrier  wave w takes actions w, w + 4, ..: it loads the select row and the raw
//                       target row of an action together (the next action's in flight under
//                       this one's sum), forms the select row's mean, and keeps the target row
//                       of its own first-max action in registers; after its last action it
//                       writes y = r + gamma^n (1 - terminal) T of that row to its slot of s_y
//                       (four candidates, one of them a*'s).  Thread i loads theta_i; the zeros
//                       of the other actions' gradient rows and the strided minimum over all B
//                       probabilities go here too.  No global load follows the barrier.
//   after it            every thread scans the means for a* (first max), thread i < N walks
//                       j = 0 .. N - 1 reading y_j as an LDS broadcast and stores its gradient
//                       element; a second barrier only for the loss's block sum.
// The summation orders (fixed, functions of N alone; tests/qr_cases.py restates them in fp32):
//   row sum    each 64-quantile chunk by fast_sum's tree, the chunks added in chunk order
//   j walk     four partial sums, term j into partial j mod 4, each in j order, combined as
//              (p0 + p1) + (p2 + p3): loss terms w L_k and gradient terms w L_k' alike
//   block sum  fast_sum per wave, the waves as ((s0 + s1) + s2) + s3; loss = (sum / N) / kappa
// The weight |tau_i - 1{u < 0}| is formed without the cancellation near tau = 1: (i + 0.5) / N
// where u >= 0 and (N - i - 0.5) / N where u < 0, one correctly rounded quotient each.
// No atomics, nothing outside the block: two launches are bitwise equal.
// ---------------------------------------------------------------------------
struct QrArgs {
  const float* ol;
  const float* tl;
  const float* sl;
  const int32_t* act;
  const float* rew;
  const uint8_t* term;
  const float* probs;
  int B, A, N;
  float cg, kappa;
  float* grad;
  float* loss_out;
  float* prio_out;
};
constexpr int kQrT = 256, kQrWaves = kQrT / kWave, kQrMaxQuantiles = kC51WideChunks * kWave;
constexpr int kQrMaxActions = 64;
static_assert(kQrMaxQuantiles == kQrT, "one thread per quantile");

template <bool kProbs>
__global__ __launch_bounds__(kQrT) void k_qr(QrArgs a) {
  warm_kernargs<sizeof(QrArgs)>();
  __shared__ __attribute__((aligned(16))) float s_y[kQrWaves * kQrMaxQuantiles];   // candidates
  __shared__ float s_q[kQrMaxActions];   // select means
  __shared__ float s_red[8];             // [0..3] loss partials, [4..7] probability minima
  const int N = a.N, A = a.A, b = blockIdx.x, t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6, nch = (N + kWave - 1) >> 6;
  const bool on = t < N;
  const int ab = a.act[b];
  const float rew_b = a.rew[b], term_b = (float)a.term[b];
  const float pr_b = kProbs ? a.probs[b] : 0.0f;
  const int64_t base = (int64_t)b * A * N;
  const int a0 = min(wave, A - 1);
  WideRow xs = wide_load(a.sl + base + (int64_t)a0 * N, N, lane, 0.0f);
  WideRow xt = wide_load(a.tl + base + (int64_t)a0 * N, N, lane, 0.0f);
  const float theta = a.ol[base + (int64_t)ab * N + min(t, N - 1)];
  if (kProbs) {   // PER: the minimum over all B probabilities (k_c51's weight)
    float pm = a.probs[min(t, a.B - 1)];
    for (int i = t + kQrT; i < a.B; i += kQrT) pm = fminf(pm, a.probs[i]);
    pm = fast_min(pm);
    if (lane == 0) s_red[4 + wave] = pm;
  }
  const float fN = (float)N;
  WideRow bt = xt;  // raw target row of this wave's first-max select action
  float bq = 0.0f;
  for (int act = wave; act < A; act += kQrWaves) {
    // the next action's two rows, in flight under this one's sum (clamped: in bounds)
    const int nx = min(act + kQrWaves, A - 1);
    const WideRow ns = wide_load(a.sl + base + (int64_t)nx * N, N, lane, 0.0f);
    const WideRow nt = wide_load(a.tl + base + (int64_t)nx * N, N, lane, 0.0f);
    const float q = __fdiv_rn(wide_sum(xs, nch), fN);
    if (lane == 0) s_q[act] = q;
    if (act == wave || q > bq) {   // first max within the wave's actions (strict >)
      bq = q;
      bt = xt;
    }
    xs = ns;
    xt = nt;
  }
  if (wave < A) {   // this wave's candidate: y of the kept target row
    const float gt = __fmul_rn(a.cg, __fsub_rn(1.0f, term_b));
#pragma unroll
    for (int c = 0; c < kC51WideChunks; ++c) {
      const int i = lane + c * kWave;
      if (i < N) s_y[wave * kQrMaxQuantiles + i] = __fadd_rn(rew_b, __fmul_rn(gt, bt.v[c]));
    }
  }
  // grad is fully written: zeros on the rows not chosen
  {
    float* g = a.grad + base;
    for (int act = 0; act < A; ++act)
      if (act != ab && on) g[act * N + t] = 0.0f;
  }
  __syncthreads();   // s_y, s_q, s_red[4..7] complete
  float w = 1.0f;
  if (kProbs) {
    const float pm = fminf(fminf(s_red[4], s_red[5]), fminf(s_red[6], s_red[7]));
    const float m = __fdiv_rn(1.0f, sqrt_rn(__fadd_rn(pm, 1e-10f)));
    w = __fdiv_rn(__fdiv_rn(1.0f, sqrt_rn(__fadd_rn(pr_b, 1e-10f))), m);
  }
  int astar = 0;     // greedy select action, first max
  {
    float best = s_q[0];
    for (int act = 1; act < A; ++act) {
      const float qa = s_q[act];
      if (qa > best) {
        best = qa;
        astar = act;
      }
    }
  }
  const float* y = s_y + (astar & (kQrWaves - 1)) * kQrMaxQuantiles;
  const float kappa = a.kappa, hk = __fmul_rn(0.5f, kappa);
  float rho = 0.0f;
  if (on) {
    const float w_pos = __fdiv_rn(__fadd_rn((float)t, 0.5f), fN);
    const float w_neg = __fdiv_rn(__fsub_rn((float)(N - t), 0.5f), fN);
    float r4[4] = {0.0f, 0.0f, 0.0f, 0.0f}, g4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    auto term_of = [&](float yj, float& h, float& dh) {
      const float u = __fsub_rn(yj, theta);
      const float au = fabsf(u);
      const bool inner = au <= kappa;
      const float wq = u < 0.0f ? w_neg : w_pos;
      h = __fmul_rn(wq, inner ? __fmul_rn(__fmul_rn(0.5f, u), u)
                              : __fmul_rn(kappa, __fsub_rn(au, hk)));
      dh = __fmul_rn(wq, inner ? u : (u > 0.0f ? kappa : -kappa));
    };
    int j = 0;
    for (; j + 8 <= N; j += 8) {     // 8 terms' LDS reads in flight, then summed in order
      float hh[8], dd[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) term_of(y[j + k], hh[k], dd[k]);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        r4[k & 3] = __fadd_rn(r4[k & 3], hh[k]);
        g4[k & 3] = __fadd_rn(g4[k & 3], dd[k]);
      }
    }
    for (; j < N; ++j) {
      float h, dh;
      term_of(y[j], h, dh);
      r4[j & 3] = __fadd_rn(r4[j & 3], h);
      g4[j & 3] = __fadd_rn(g4[j & 3], dh);
    }
    rho = __fadd_rn(__fadd_rn(r4[0], r4[1]), __fadd_rn(r4[2], r4[3]));
    const float g = __fadd_rn(__fadd_rn(g4[0], g4[1]), __fadd_rn(g4[2], g4[3]));
    const float gscale =
        __fmul_rn(w, __fdiv_rn(-1.0f, __fmul_rn(__fmul_rn(fN, (float)a.B), kappa)));
    a.grad[base + (int64_t)ab * N + t] = __fmul_rn(g, gscale);
  }
  if (!a.loss_out && !a.prio_out) return;
  const float part = fast_sum(rho);
  if (lane == 0) s_red[wave] = part;
  __syncthreads();
  if (t == 0) {
    const float tot = __fadd_rn(__fadd_rn(__fadd_rn(s_red[0], s_red[1]), s_red[2]), s_red[3]);
    const float loss = __fdiv_rn(__fdiv_rn(tot, fN), kappa);
    if (a.loss_out) a.loss_out[b] = loss;
    if (a.prio_out) a.prio_out[b] = sqrt_rn(__fadd_rn(loss, 1e-10f));
  }
}

}  // namespace dq

using namespace dq;

extern "C" {

int dq_qr_loss(const float* online_q, const float* target_q, const float* select_q,
               const int32_t* actions, const float* rewards, const uint8_t* terminals,
               const float* probs, int32_t batch, int32_t num_actions, int32_t num_quantiles,
               float cumulative_gamma, float kappa, float* grad, float* loss_out,
               float* priorities_out, float* mean_loss_out, void* stream) {
  DQ_CHECK_ARG(online_q && target_q && actions && rewards && terminals && grad, "null argument");
  DQ_CHECK_ARG(num_quantiles >= 1 && num_quantiles <= kQrMaxQuantiles,
               "num_quantiles must be in [1, 256]");
  DQ_CHECK_ARG(num_actions >= 1 && num_actions <= kQrMaxActions,
               "num_actions must be in [1, 64]");
  DQ_CHECK_ARG(batch >= 1, "bad batch");
  DQ_CHECK_ARG(kappa > 0.0f, "kappa must be > 0");
  DQ_CHECK_ARG(!mean_loss_out || loss_out, "mean_loss_out needs loss_out");
  QrArgs a{online_q, target_q, select_q ? select_q : target_q, actions, rewards, terminals,
           probs, batch, num_actions, num_quantiles, cumulative_gamma, kappa, grad, loss_out,
           priorities_out};
  auto kern = probs ? k_qr<true> : k_qr<false>;
  hipLaunchKernelGGL(kern, dim3(batch), dim3(kQrT), 0, (hipStream_t)stream, a);
  DQ_CHECK_LAUNCH("k_qr");
  if (mean_loss_out) {
    hipLaunchKernelGGL(k_wmean, dim3(1), dim3(64), 0, (hipStream_t)stream, loss_out, probs, batch,
                       mean_loss_out);
    DQ_CHECK_LAUNCH("k_wmean");
  }
  return DQ_OK;
}

}  // extern "C"
