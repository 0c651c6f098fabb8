// Munchausen-DQN's loss (dq_mdqn_loss / k_mdqn): Vieillard, Pietquin, Geist, "Munchausen
// Reinforcement Learning", NeurIPS 2020, eq. (2) with the clipped log-policy of section 4 and
// appendix B (the authors' Dopamine agent).  A translation unit of its own, so the other loss
// kernels' code objects stay what they were.
#include <cmath>

#include "common.h"

namespace dq {

// ---------------------------------------------------------------------------
// X' = target Q'(s', .), X = target Q'(s, .), q = online Q(s, a) of the taken action a.  For a
// row x of A values, all in fp32, every operation rounded once and never contracted:
//   m       = max_j x_j
//   e_j     = expf((x_j - m) / tau)                       a rounded difference, a rounded quotient
//   S       = sum_j e_j                                   in the lane order below
//   tls     = tau * logf(S)                               (S >= 1: the maximum's term is exp(0))
// and per sample
//   V       = m' + tls'                                   the soft value of X' (= tau lse(X'/tau))
//   tlp     = (X_a - m) - tls                             tau log pi(a | s), <= 0
//   bonus   = alpha * min(max(tlp, clip_min), 0)
//   target  = (r + bonus) + (cg * V) * (1 - terminal)     the bonus is not masked by terminal
//   err     = q - target, then Huber(1), the gradient and its 1 / B exactly as k_dqn.
// V is the log-sum-exp form of sum_j pi'_j (X'_j - tau log pi'_j): no product of an underflowed
// pi with its log appears, so a row whose gaps are far above tau gives S = 1, V = m', finite.
//
// One block of four waves; wave w takes samples w, w + 4, .., a lane the actions lane,
// lane + 64, ..  A row costs a wave_max and a wave_sum per input instead of 2 A serial
// transcendentals on one thread.  The next sample's first 64 actions and its scalars are loaded
// before this sample's reductions.  The orders (fixed, functions of A and B alone):
//   S      lane l adds its e_j in j order (l, l + 64, ..; a lane past A holds 0), then
//          common.h's wave_sum: v += v[lane ^ o] for o = 32, 16, 8, 4, 2, 1
//   mean   k_dqn's: partial t (of 256) adds loss_b for b = t, t + 256, .. in b order (kept in
//          LDS: 256 % 4 == 0, so slot b % 256 belongs to wave b % 4 alone), each 64 partials by
//          wave_sum, the four sums in wave order from 0, one rounded quotient by B
// No atomics, no workspace, nothing outside the block: two launches are bitwise equal.
// With A = 1: e = exp(0) = 1, S = 1 (the other lanes add +0), log(1) = +0, V = m' = X', tlp = +0,
// bonus = +0, so target, loss, gradient and mean are k_dqn's operation for operation on
// (online_q, target_next_q) -- bitwise, but for the sign of a zero where r is -0.
// ---------------------------------------------------------------------------
struct MdqnArgs {
  const float* oq;
  const float* tn;
  const float* tc;
  const int32_t* act;
  const float* rew;
  const uint8_t* term;
  int B, A;
  float cg, tau, alpha, clip_min;
  float* grad;
  float* loss_out;
  float* mean_out;
};
constexpr int kMdqnT = 256, kMdqnWaves = kMdqnT / kWave;

struct MdqnRow {   // what a wave holds of one sample before its reductions
  float xn, xc;    // X'[b, lane], X[b, lane]  (-inf past A)
  float q, xa, rew, term;
  int ab;
};

__global__ __launch_bounds__(kMdqnT) void k_mdqn(MdqnArgs a) {
  __shared__ float s_part[kMdqnT];
  __shared__ float s_red[kMdqnWaves];
  const int t = threadIdx.x, lane = t & (kWave - 1), wave = t >> 6;
  const int A = a.A, B = a.B;
  const float tau = a.tau;
  const float invB = __fdiv_rn(1.0f, (float)B);
  const bool on = lane < A;
  s_part[lane * kMdqnWaves + wave] = 0.0f;   // this wave's own 64 slots: no barrier needed
  auto load = [&](int b) {
    MdqnRow r;
    const int64_t base = (int64_t)b * A;
    r.xn = on ? a.tn[base + lane] : -INFINITY;
    r.xc = on ? a.tc[base + lane] : -INFINITY;
    r.ab = a.act[b];
    r.q = a.oq[base + r.ab];
    r.xa = a.tc[base + r.ab];
    r.rew = a.rew[b];
    r.term = (float)a.term[b];
    return r;
  };
  MdqnRow cur = load(min(wave, B - 1));
  for (int b = wave; b < B; b += kMdqnWaves) {
    const MdqnRow nxt = load(min(b + kMdqnWaves, B - 1));   // clamped: in bounds
    const int64_t base = (int64_t)b * A;
    float mn = cur.xn, mc = cur.xc;
    for (int j = lane + kWave; j < A; j += kWave) {
      mn = fmaxf(mn, a.tn[base + j]);
      mc = fmaxf(mc, a.tc[base + j]);
    }
    mn = wave_max(mn);
    mc = wave_max(mc);
    float sn = on ? expf(__fdiv_rn(__fsub_rn(cur.xn, mn), tau)) : 0.0f;
    float sc = on ? expf(__fdiv_rn(__fsub_rn(cur.xc, mc), tau)) : 0.0f;
    for (int j = lane + kWave; j < A; j += kWave) {
      sn = __fadd_rn(sn, expf(__fdiv_rn(__fsub_rn(a.tn[base + j], mn), tau)));
      sc = __fadd_rn(sc, expf(__fdiv_rn(__fsub_rn(a.tc[base + j], mc), tau)));
    }
    sn = wave_sum(sn);
    sc = wave_sum(sc);
    // every lane holds the same mn, mc, sn, sc: the rest is computed by all of them
    const float v = __fadd_rn(mn, __fmul_rn(tau, logf(sn)));
    const float tlp = __fsub_rn(__fsub_rn(cur.xa, mc), __fmul_rn(tau, logf(sc)));
    const float bonus = __fmul_rn(a.alpha, fminf(fmaxf(tlp, a.clip_min), 0.0f));
    const float target = __fadd_rn(__fadd_rn(cur.rew, bonus),
                                   __fmul_rn(__fmul_rn(a.cg, v), __fsub_rn(1.0f, cur.term)));
    const float err = __fsub_rn(cur.q, target);   // predictions - labels
    const float ae = fabsf(err);
    const float quad = fminf(ae, 1.0f);
    const float lin = __fsub_rn(ae, quad);
    const float loss = __fadd_rn(__fmul_rn(__fmul_rn(0.5f, quad), quad), lin);
    const float g = __fmul_rn(fminf(fmaxf(err, -1.0f), 1.0f), invB);
    for (int j = lane; j < A; j += kWave) a.grad[base + j] = (j == cur.ab) ? g : 0.0f;
    if (lane == 0) {
      if (a.loss_out) a.loss_out[b] = loss;
      const int slot = b & (kMdqnT - 1);
      s_part[slot] = __fadd_rn(s_part[slot], loss);
    }
    cur = nxt;
  }
  __syncthreads();   // s_part complete
  const float part = wave_sum(s_part[t]);
  if (lane == 0) s_red[wave] = part;
  __syncthreads();
  if (t == 0 && a.mean_out) {
    float tot = 0.0f;
    for (int i = 0; i < kMdqnWaves; ++i) tot = __fadd_rn(tot, s_red[i]);
    a.mean_out[0] = __fdiv_rn(tot, (float)B);
  }
}

}  // namespace dq

using namespace dq;

extern "C" {

int dq_mdqn_loss(const float* online_q, const float* target_next_q, const float* target_cur_q,
                 const int32_t* actions, const float* rewards, const uint8_t* terminals,
                 int32_t batch, int32_t num_actions, float cumulative_gamma, float tau,
                 float alpha, float clip_min, float* grad_q, float* loss_out,
                 float* mean_loss_out, void* stream) {
  DQ_CHECK_ARG(online_q && target_next_q && target_cur_q && actions && rewards && terminals &&
                   grad_q, "null argument");
  DQ_CHECK_ARG(batch >= 1 && num_actions >= 1, "bad sizes");
  DQ_CHECK_ARG(std::isfinite(tau) && tau > 0.0f, "tau must be finite and > 0");
  DQ_CHECK_ARG(std::isfinite(alpha) && alpha >= 0.0f, "alpha must be finite and >= 0");
  DQ_CHECK_ARG(std::isfinite(clip_min) && clip_min <= 0.0f, "clip_min must be finite and <= 0");
  DQ_CHECK_ARG(!mean_loss_out || loss_out, "mean_loss_out needs loss_out");
  MdqnArgs a{online_q, target_next_q, target_cur_q, actions, rewards, terminals, batch,
             num_actions, cumulative_gamma, tau, alpha, clip_min, grad_q, loss_out,
             mean_loss_out};
  hipLaunchKernelGGL(k_mdqn, dim3(1), dim3(kMdqnT), 0, (hipStream_t)stream, a);
  DQ_CHECK_LAUNCH("k_mdqn");
  return DQ_OK;
}

}  // extern "C"
