// The SAC loss head: what SAC.learn computes between the network forwards and the backwards (DRL.py:384-425; SURVEY 3(A),
// row a14), each loss with its gradient in ONE launch, the temperature read from device memory so that a captured step follows it.
//   sac_critic_loss : y = r + (1 - done) gamma (min(q1n, q2n) - alpha logp_next);  loss = mean(w (q1 - y)^2) + mean(w (q2 - y)^2);
//                     td[b] = mean_a |q1 - y|;  dq1 | dq2 for a unit upstream gradient.  discount[b], when given, stands where gamma
//                     does: the gamma^m of an n-step batch
//   sac_actor_loss  : policy_loss = mean(alpha logp - min(q1pi, q2pi)), alpha_loss = -log_alpha mean(logp + target_entropy), and
//                     d logp | dq1pi | dq2pi and d log_alpha for unit upstream gradients
//   sac_bc_loss     : the demonstration term of the actor loss: a masked, optionally Q-filtered mean of (pred - action)^2 or
//                     of -log_prob over the `used` rows it applies to, `used` counted on the device; d pred for a unit upstream gradient
//   sac_cql_penalty : the conservative term of a CQL(H) critic loss: w (gap_1 + gap_2 - 2 tau), gap_i the masked mean over rows
//                     and columns of T logsumexp_m((q_cat - log_w) / T) - q_data; d q_cat (the softmax) | d q_data and d log_weight
//   sac_scale_grads : dst = *scale_dev * src, the backward of either loss for the 0-d upstream gradient autograd hands over
// The two loss kernels are ONE workgroup of 256 threads: B * A is at most 2^20 elements of a few flops each, and one workgroup needs no
// second launch, no atomics and no counters for its sums.  Every thread walks the elements i = tid, tid + 256, ... (row b = i / A), sums
// in double, the wave folds with __shfl_down, the four waves meet in LDS and thread 0 writes the scalars: the same bits on every call.
// Per element the arithmetic is in double from the fp32 inputs and rounded once where a value is stored; the stored fp32 target is the
// one every later term uses, so td and the gradients are those of the returned tensor.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int SAC_MAX_ACTIONS = 16;          // as tanh_gaussian_*
constexpr long long SAC_MAX_ELEMS = 1 << 20;

__device__ __forceinline__ float sac_alpha(const float* __restrict__ log_alpha, float alpha) { return log_alpha ? expf(*log_alpha) : alpha; }

__device__ __forceinline__ float sac_target(float r, float not_done, float gamma, float q1n, float q2n, float al, float nlp) {
  return (float)((double)r + (double)not_done * (double)gamma * ((double)fminf(q1n, q2n) - (double)al * (double)nlp));
}

// the workgroup's sum of s in thread 0 (fixed order: lanes by __shfl_down, then wave 0 + 1, wave 2 + 3); wave_sum: 4 doubles of LDS
__device__ __forceinline__ double block_sum(double s, double* wave_sum) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
  __syncthreads();
  return (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

__global__ void __launch_bounds__(256) sac_critic_loss_kernel(const float* __restrict__ q1, const float* __restrict__ q2, const float* __restrict__ reward,
                                                              const float* __restrict__ done, const float* __restrict__ weights,
                                                              const float* __restrict__ discount, const float* __restrict__ q1n, const float* __restrict__ q2n,
                                                              const float* __restrict__ nlogp, const float* __restrict__ log_alpha, float alpha,
                                                              float gamma_all, float* __restrict__ y, float* __restrict__ td, float* __restrict__ loss,
                                                              float* __restrict__ grads, int B, int A) {
  __shared__ double wave_sum[4];
  const float al = sac_alpha(log_alpha, alpha);
  const int n = B * A;
  const double inv_n = 1.0 / (double)n;
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int b = i / A;
    const float r = reward[b], nd = done ? 1.f - done[b] : 1.f, nlp = nlogp[b];
    const double w = weights ? (double)weights[b] : 1.0;
    const float gamma = discount ? discount[b] : gamma_all;
    const float yi = sac_target(r, nd, gamma, q1n[i], q2n[i], al, nlp);
    const double e1 = (double)q1[i] - (double)yi, e2 = (double)q2[i] - (double)yi;
    acc += w * (e1 * e1 + e2 * e2);
    y[i] = yi;
    if (grads) {
      grads[i] = (float)(2.0 * w * e1 * inv_n);
      grads[n + i] = (float)(2.0 * w * e2 * inv_n);
    }
    if (td && i == b * A) {     // the thread of a row's first element: the row's mean |q1 - y| in fp32
      // In the order of torch's (q1 - y).abs().mean(1) on the device, so that the write-back is the number a caller would have computed
      // from the returned target: P = the largest power of two <= A lanes, lane t sums elements t and t + P, the lanes fold pairwise
      // (offsets 1, 2, 4, 8), times 1 / A.  Slots past P hold +0, which changes no sum of non-negative terms; the indices are
      // compile-time constants after unrolling, so v[] stays in registers.
      int P = 1;
      while (2 * P <= A) P *= 2;
      float v[SAC_MAX_ACTIONS];
#pragma unroll
      for (int t = 0; t < SAC_MAX_ACTIONS; ++t) {
        v[t] = 0.f;
        if (t < P) {
          v[t] = t == 0 ? fabsf(q1[i] - yi) : fabsf(q1[i + t] - sac_target(r, nd, gamma, q1n[i + t], q2n[i + t], al, nlp));
          if (t + P < A) v[t] += fabsf(q1[i + t + P] - sac_target(r, nd, gamma, q1n[i + t + P], q2n[i + t + P], al, nlp));
        }
      }
#pragma unroll
      for (int off = 1; off < SAC_MAX_ACTIONS; off <<= 1) {
#pragma unroll
        for (int t = 0; t < SAC_MAX_ACTIONS; t += 2 * off) v[t] += v[t + off];
      }
      td[b] = v[0] * (1.f / (float)A);
    }
  }
  const double tot = block_sum(acc, wave_sum);
  if (threadIdx.x == 0) loss[0] = (float)(tot * inv_n);
}

__global__ void __launch_bounds__(256) sac_actor_loss_kernel(const float* __restrict__ logp, const float* __restrict__ q1, const float* __restrict__ q2,
                                                             const float* __restrict__ log_alpha, float alpha, int with_temperature,
                                                             float target_entropy, float* __restrict__ losses, float* __restrict__ grads,
                                                             float* __restrict__ dlog_alpha, int B, int A) {
  __shared__ double wave_sum[2][4];
  const float al = sac_alpha(log_alpha, alpha);
  const int n = B * A;
  const double inv_n = 1.0 / (double)n;
  const float g_min = (float)(-inv_n), g_tie = (float)(-0.5 * inv_n), g_logp = (float)((double)al / (double)B);
  double acc = 0.0, ent = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int b = i / A;
    const float lp = logp[b], a1 = q1[i], a2 = q2[i];
    acc += (double)al * (double)lp - (double)fminf(a1, a2);
    if (i == b * A) {
      ent += (double)lp + (double)target_entropy;
      if (grads) grads[b] = g_logp;
    }
    if (grads) {                // torch.minimum's rule: the gradient goes to the smaller one, half to each at a tie
      grads[B + i] = a1 < a2 ? g_min : (a1 == a2 ? g_tie : 0.f);
      grads[B + n + i] = a2 < a1 ? g_min : (a1 == a2 ? g_tie : 0.f);
    }
  }
  const double tot = block_sum(acc, wave_sum[0]);
  const double etot = block_sum(ent, wave_sum[1]);
  if (threadIdx.x == 0) {
    losses[0] = (float)(tot * inv_n);
    if (with_temperature) {
      const double m = etot / (double)B;
      losses[1] = (float)(-(double)*log_alpha * m);
      if (dlog_alpha) dlog_alpha[0] = (float)(-m);
    }
  }
}

// the weight m_b f_b of row b in the demonstration loss: the mask (fp32 weights, or the bytes of a bool tensor) times the Q-filter's
// decision, mean_a min(q1_demo, q2_demo) > mean_a min(q1_pi, q2_pi), strict; both means summed in double over a = 0 .. A - 1
__device__ __forceinline__ double bc_row_weight(const void* __restrict__ mask, int mask_u8, const float* __restrict__ q1d,
                                                const float* __restrict__ q2d, const float* __restrict__ q1p, const float* __restrict__ q2p,
                                                int b, int A) {
  double w = 1.0;
  if (mask) w = mask_u8 ? (double)(static_cast<const unsigned char*>(mask)[b] != 0) : (double)static_cast<const float*>(mask)[b];
  if (q1d) {
    double sd = 0.0, sp = 0.0;
    for (int a = 0; a < A; ++a) {
      const int i = b * A + a;
      sd += (double)fminf(q1d[i], q2d[i]);
      sp += (double)fminf(q1p[i], q2p[i]);
    }
    if (!(sd / (double)A > sp / (double)A)) w = 0.0;
  }
  return w;
}

// The demonstration term: loss = sum_b w_b l_b / used, used = sum_b w_b, w_b = bc_row_weight; l_b = mean_a (pred - action)^2,
// or -pred_b with nll (pred is then the log-density, B values).  thread = rows b = tid, tid + 256, ...; the two sums meet as block_sum
// does, every thread reads them back, and the second walk writes the gradients for a unit upstream gradient, which need 1 / used.
// used == 0 gives loss 0 and zero gradients; a row of weight 0 adds nothing, whatever its l_b.
__global__ void __launch_bounds__(256) sac_bc_loss_kernel(const float* __restrict__ pred, const float* __restrict__ action,
                                                          const void* __restrict__ mask, int mask_u8, const float* __restrict__ q1d,
                                                          const float* __restrict__ q2d, const float* __restrict__ q1p,
                                                          const float* __restrict__ q2p, int nll, float* __restrict__ out,
                                                          float* __restrict__ grads, int B, int A) {
  __shared__ double wave_sum[2][4];
  const double inv_a = 1.0 / (double)A;
  double acc = 0.0, cnt = 0.0;
  for (int b = threadIdx.x; b < B; b += 256) {
    const double w = bc_row_weight(mask, mask_u8, q1d, q2d, q1p, q2p, b, A);
    if (w == 0.0) continue;
    double l;
    if (nll) {
      l = -(double)pred[b];
    } else {
      double s = 0.0;
      for (int a = 0; a < A; ++a) {
        const double d = (double)pred[b * A + a] - (double)action[b * A + a];
        s += d * d;
      }
      l = s * inv_a;
    }
    acc += w * l;
    cnt += w;
  }
  const double tot = block_sum(acc, wave_sum[0]);
  const double used = block_sum(cnt, wave_sum[1]);
  const double inv_used = used > 0.0 ? 1.0 / used : 0.0;
  if (threadIdx.x == 0) {
    out[0] = (float)(tot * inv_used);
    out[1] = (float)used;
  }
  if (!grads) return;
  for (int b = threadIdx.x; b < B; b += 256) {
    const double w = bc_row_weight(mask, mask_u8, q1d, q2d, q1p, q2p, b, A) * inv_used;
    if (nll) {
      grads[b] = w == 0.0 ? 0.f : (float)(-w);
    } else {
      for (int a = 0; a < A; ++a) {
        const int i = b * A + a;
        grads[i] = w == 0.0 ? 0.f : (float)(2.0 * w * inv_a * ((double)pred[i] - (double)action[i]));
      }
    }
  }
}

// The CQL(H) penalty of a twin critic.  For critic i, row b and column c, over the M proposal actions of the row:
//   z_m = q_cat[b][m][c] - log_w[b][m];   lse = T log sum_m exp(z_m / T)   (max-subtracted);   gap_i = sum_{b, c} w_b (lse - q_data) / (used C)
// with w_b the row's mask weight and used = sum_b w_b;  loss = w (gap_1 + gap_2 - 2 tau), tau = 0 outside the Lagrange form, w = the float
// or exp(*log_weight) read here.  thread = items (i, b, c) = tid, tid + 256, ...: the first walk sums the gaps, the sums meet as
// block_sum does, and the second walk writes the gradients for a unit upstream gradient, which need 1 / used:
//   d q_cat = w w_b softmax_m(z / T) / (used C),   d q_data = -w w_b / (used C);   a row of weight 0 gets exact zeros
// used == 0 gives loss 0, weight_loss 0 and zero gradients.  out = [loss, weight_loss, gap_1, gap_2, used].
__device__ __forceinline__ double cql_zt(const float* __restrict__ qc, const float* __restrict__ lw, int m, int C, double T) {
  return ((double)qc[(long long)m * C] - (lw ? (double)lw[m] : 0.0)) / T;
}

__global__ void __launch_bounds__(256) sac_cql_penalty_kernel(const float* __restrict__ q1c, const float* __restrict__ q2c,
                                                              const float* __restrict__ q1d, const float* __restrict__ q2d,
                                                              const float* __restrict__ log_w, const void* __restrict__ mask, int mask_u8,
                                                              const float* __restrict__ log_weight, float weight, float temperature,
                                                              float target_gap, int lagrange, float* __restrict__ out,
                                                              float* __restrict__ grads, float* __restrict__ dlog_weight, int B, int M, int C) {
  __shared__ double wave_sum[3][4];
  const double w = log_weight ? exp((double)*log_weight) : (double)weight, T = (double)temperature;   // in double, as every term here
  const int n = B * C;
  double acc1 = 0.0, acc2 = 0.0, cnt = 0.0;
  for (int it = threadIdx.x; it < 2 * n; it += 256) {
    const int i = it >= n, e = it - i * n, b = e / C, c = e - b * C;
    const double wb = !mask ? 1.0 : (mask_u8 ? (double)(static_cast<const unsigned char*>(mask)[b] != 0) : (double)static_cast<const float*>(mask)[b]);
    if (wb == 0.0) continue;
    const float* __restrict__ qc = (i ? q2c : q1c) + (long long)b * M * C + c;
    const float* __restrict__ lw = log_w ? log_w + (long long)b * M : nullptr;
    double mx = cql_zt(qc, lw, 0, C, T);
    for (int m = 1; m < M; ++m) mx = fmax(mx, cql_zt(qc, lw, m, C, T));
    double S = 0.0;
    for (int m = 0; m < M; ++m) S += exp(cql_zt(qc, lw, m, C, T) - mx);
    const double term = wb * (T * (mx + log(S)) - (double)(i ? q2d : q1d)[e]);
    if (i) acc2 += term; else acc1 += term;
    if (it < n && c == 0) cnt += wb;
  }
  const double tot1 = block_sum(acc1, wave_sum[0]);
  const double tot2 = block_sum(acc2, wave_sum[1]);
  const double used = block_sum(cnt, wave_sum[2]);
  const double inv = used > 0.0 ? 1.0 / (used * (double)C) : 0.0;
  if (threadIdx.x == 0) {
    const double g1 = tot1 * inv, g2 = tot2 * inv;
    const double excess = used > 0.0 ? g1 + g2 - (lagrange ? 2.0 * (double)target_gap : 0.0) : 0.0;
    out[0] = (float)(w * excess);
    out[1] = lagrange ? (float)(-w * excess) : 0.f;
    out[2] = (float)g1;
    out[3] = (float)g2;
    out[4] = (float)used;
    if (dlog_weight) dlog_weight[0] = (float)(-w * excess);
  }
  if (!grads) return;
  const long long ncat = (long long)B * M * C;
  for (int it = threadIdx.x; it < 2 * n; it += 256) {
    const int i = it >= n, e = it - i * n, b = e / C, c = e - b * C;
    const double wb = !mask ? 1.0 : (mask_u8 ? (double)(static_cast<const unsigned char*>(mask)[b] != 0) : (double)static_cast<const float*>(mask)[b]);
    float* __restrict__ gc = grads + i * ncat + (long long)b * M * C + c;
    float* __restrict__ gd = grads + 2 * ncat + (long long)i * n + e;
    const double coef = w * wb * inv;
    if (wb == 0.0 || inv == 0.0) {
      for (int m = 0; m < M; ++m) gc[(long long)m * C] = 0.f;
      *gd = 0.f;
      continue;
    }
    const float* __restrict__ qc = (i ? q2c : q1c) + (long long)b * M * C + c;
    const float* __restrict__ lw = log_w ? log_w + (long long)b * M : nullptr;
    double mx = cql_zt(qc, lw, 0, C, T);
    for (int m = 1; m < M; ++m) mx = fmax(mx, cql_zt(qc, lw, m, C, T));
    double S = 0.0;
    for (int m = 0; m < M; ++m) S += exp(cql_zt(qc, lw, m, C, T) - mx);
    const double cs = coef / S;
    for (int m = 0; m < M; ++m) gc[(long long)m * C] = (float)(cs * exp(cql_zt(qc, lw, m, C, T) - mx));
    *gd = (float)(-coef);
  }
}

__global__ void __launch_bounds__(256) sac_scale_grads_kernel(const float* __restrict__ src, float* __restrict__ dst, long long n,
                                                              const float* __restrict__ scale_dev) {
  const float s = *scale_dev;
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) dst[i] = s * src[i];
}

inline bool al4p(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3) == 0; }

}  // namespace

int sac_critic_loss(const float* q1, const float* q2, const float* reward, const float* done, const float* weights, const float* discount,
                    const float* next_q1, const float* next_q2, const float* next_log_pi, const float* log_alpha, float alpha, float gamma,
                    float* target, float* td, float* loss, float* grads, int B, int A, hipStream_t stream) {
  DGVIT_CHECK_ARG(q1 && q2 && reward && next_q1 && next_q2 && next_log_pi, "sac_critic_loss: q1, q2, reward, next_q1, next_q2 and next_log_pi must not be null");
  DGVIT_CHECK_ARG(target && loss, "sac_critic_loss: target and loss must not be null");
  DGVIT_CHECK_ARG(B >= 1, "sac_critic_loss: B=%d must be at least 1", B);
  DGVIT_CHECK_ARG(A >= 1 && A <= SAC_MAX_ACTIONS, "sac_critic_loss: A=%d must be in [1, %d]", A, SAC_MAX_ACTIONS);
  DGVIT_CHECK_ARG((long long)B * A <= SAC_MAX_ELEMS, "sac_critic_loss: B*A=%lld must be at most %lld", (long long)B * A, SAC_MAX_ELEMS);
  DGVIT_CHECK_ARG(log_alpha || std::isfinite(alpha), "sac_critic_loss: alpha=%g must be finite (or log_alpha given)", (double)alpha);
  DGVIT_CHECK_ARG(discount || std::isfinite(gamma), "sac_critic_loss: gamma=%g must be finite (or discount given)", (double)gamma);
  DGVIT_CHECK_ARG(al4p(q1) && al4p(q2) && al4p(reward) && al4p(done) && al4p(weights) && al4p(discount) && al4p(next_q1) && al4p(next_q2) && al4p(next_log_pi) &&
                      al4p(log_alpha) && al4p(target) && al4p(td) && al4p(loss) && al4p(grads),
                  "sac_critic_loss: pointers must be 4-byte aligned");
  {
    ProfileScope t(PROF_OTHER, 0.0, stream);
    hipLaunchKernelGGL(sac_critic_loss_kernel, dim3(1), dim3(256), 0, stream, q1, q2, reward, done, weights, discount, next_q1, next_q2, next_log_pi,
                       log_alpha, alpha, gamma, target, td, loss, grads, B, A);
  }
  DGVIT_CHECK_LAUNCH("sac_critic_loss");
  return DGVIT_OK;
}

int sac_actor_loss(const float* log_pi, const float* q1_pi, const float* q2_pi, const float* log_alpha, float alpha, int with_temperature,
                   float target_entropy, float* losses, float* grads, float* dlog_alpha, int B, int A, hipStream_t stream) {
  DGVIT_CHECK_ARG(log_pi && q1_pi && q2_pi && losses, "sac_actor_loss: log_pi, q1_pi, q2_pi and losses must not be null");
  DGVIT_CHECK_ARG(B >= 1, "sac_actor_loss: B=%d must be at least 1", B);
  DGVIT_CHECK_ARG(A >= 1 && A <= SAC_MAX_ACTIONS, "sac_actor_loss: A=%d must be in [1, %d]", A, SAC_MAX_ACTIONS);
  DGVIT_CHECK_ARG((long long)B * A <= SAC_MAX_ELEMS, "sac_actor_loss: B*A=%lld must be at most %lld", (long long)B * A, SAC_MAX_ELEMS);
  DGVIT_CHECK_ARG(with_temperature == 0 || with_temperature == 1, "sac_actor_loss: with_temperature=%d must be 0 or 1", with_temperature);
  DGVIT_CHECK_ARG(log_alpha || std::isfinite(alpha), "sac_actor_loss: alpha=%g must be finite (or log_alpha given)", (double)alpha);
  DGVIT_CHECK_ARG(!with_temperature || log_alpha, "sac_actor_loss: the temperature loss needs log_alpha (it is null)");
  DGVIT_CHECK_ARG(!with_temperature || std::isfinite(target_entropy), "sac_actor_loss: target_entropy=%g must be finite", (double)target_entropy);
  DGVIT_CHECK_ARG(al4p(log_pi) && al4p(q1_pi) && al4p(q2_pi) && al4p(log_alpha) && al4p(losses) && al4p(grads) && al4p(dlog_alpha),
                  "sac_actor_loss: pointers must be 4-byte aligned");
  {
    ProfileScope t(PROF_OTHER, 0.0, stream);
    hipLaunchKernelGGL(sac_actor_loss_kernel, dim3(1), dim3(256), 0, stream, log_pi, q1_pi, q2_pi, log_alpha, alpha, with_temperature, target_entropy,
                       losses, grads, dlog_alpha, B, A);
  }
  DGVIT_CHECK_LAUNCH("sac_actor_loss");
  return DGVIT_OK;
}

int sac_bc_loss(const float* pred, const float* action, const void* mask, int mask_u8, const float* q1_demo, const float* q2_demo,
                const float* q1_pi, const float* q2_pi, int nll, float* out, float* grads, int B, int A, hipStream_t stream) {
  DGVIT_CHECK_ARG(pred && out, "sac_bc_loss: pred and out must not be null");
  DGVIT_CHECK_ARG(nll == 0 || nll == 1, "sac_bc_loss: nll=%d must be 0 or 1", nll);
  DGVIT_CHECK_ARG(mask_u8 == 0 || mask_u8 == 1, "sac_bc_loss: mask_u8=%d must be 0 or 1", mask_u8);
  DGVIT_CHECK_ARG(nll || action, "sac_bc_loss: action must not be null (it is only unused with nll=1)");
  DGVIT_CHECK_ARG(B >= 1, "sac_bc_loss: B=%d must be at least 1", B);
  DGVIT_CHECK_ARG(A >= 1 && A <= SAC_MAX_ACTIONS, "sac_bc_loss: A=%d must be in [1, %d]", A, SAC_MAX_ACTIONS);
  DGVIT_CHECK_ARG((long long)B * A <= SAC_MAX_ELEMS, "sac_bc_loss: B*A=%lld must be at most %lld", (long long)B * A, SAC_MAX_ELEMS);
  DGVIT_CHECK_ARG(!nll || A == 1, "sac_bc_loss: nll=1 takes one log-density per row, A=%d must be 1", A);
  const int nq = (q1_demo != nullptr) + (q2_demo != nullptr) + (q1_pi != nullptr) + (q2_pi != nullptr);
  DGVIT_CHECK_ARG(nq == 0 || nq == 4, "sac_bc_loss: the filter needs q1_demo, q2_demo, q1_pi and q2_pi together (%d of 4 given)", nq);
  DGVIT_CHECK_ARG(!nll || nq == 0, "sac_bc_loss: the Q-filter belongs to the squared-error loss, not to nll=1");
  DGVIT_CHECK_ARG(al4p(pred) && al4p(action) && (mask_u8 || al4p(mask)) && al4p(q1_demo) && al4p(q2_demo) && al4p(q1_pi) && al4p(q2_pi) &&
                      al4p(out) && al4p(grads),
                  "sac_bc_loss: pointers must be 4-byte aligned");
  {
    ProfileScope t(PROF_OTHER, 0.0, stream);
    hipLaunchKernelGGL(sac_bc_loss_kernel, dim3(1), dim3(256), 0, stream, pred, action, mask, mask_u8, q1_demo, q2_demo, q1_pi, q2_pi, nll, out,
                       grads, B, A);
  }
  DGVIT_CHECK_LAUNCH("sac_bc_loss");
  return DGVIT_OK;
}

int sac_cql_penalty(const float* q1_cat, const float* q2_cat, const float* q1_data, const float* q2_data, const float* log_w, const void* mask,
                    int mask_u8, const float* log_weight, float weight, float temperature, float target_gap, int lagrange, float* out,
                    float* grads, float* dlog_weight, int B, int M, int C, hipStream_t stream) {
  DGVIT_CHECK_ARG(q1_cat && q2_cat && q1_data && q2_data && out, "sac_cql_penalty: q1_cat, q2_cat, q1_data, q2_data and out must not be null");
  DGVIT_CHECK_ARG(mask_u8 == 0 || mask_u8 == 1, "sac_cql_penalty: mask_u8=%d must be 0 or 1", mask_u8);
  DGVIT_CHECK_ARG(lagrange == 0 || lagrange == 1, "sac_cql_penalty: lagrange=%d must be 0 or 1", lagrange);
  DGVIT_CHECK_ARG(B >= 1, "sac_cql_penalty: B=%d must be at least 1", B);
  DGVIT_CHECK_ARG(M >= 1, "sac_cql_penalty: M=%d must be at least 1", M);
  DGVIT_CHECK_ARG(C >= 1 && C <= SAC_MAX_ACTIONS, "sac_cql_penalty: C=%d must be in [1, %d]", C, SAC_MAX_ACTIONS);
  DGVIT_CHECK_ARG((long long)B * ((long long)M + 1) * C <= SAC_MAX_ELEMS, "sac_cql_penalty: B*(M+1)*C=%lld must be at most %lld",
                  (long long)B * ((long long)M + 1) * C, SAC_MAX_ELEMS);
  DGVIT_CHECK_ARG(std::isfinite(temperature) && temperature > 0.f, "sac_cql_penalty: temperature=%g must be finite and positive", (double)temperature);
  DGVIT_CHECK_ARG(log_weight || std::isfinite(weight), "sac_cql_penalty: weight=%g must be finite (or log_weight given)", (double)weight);
  DGVIT_CHECK_ARG(!lagrange || log_weight, "sac_cql_penalty: the Lagrange form needs log_weight (it is null)");
  DGVIT_CHECK_ARG(!lagrange || std::isfinite(target_gap), "sac_cql_penalty: target_gap=%g must be finite", (double)target_gap);
  DGVIT_CHECK_ARG(lagrange || !dlog_weight, "sac_cql_penalty: dlog_weight belongs to the Lagrange form (lagrange=0)");
  DGVIT_CHECK_ARG(al4p(q1_cat) && al4p(q2_cat) && al4p(q1_data) && al4p(q2_data) && al4p(log_w) && (mask_u8 || al4p(mask)) && al4p(log_weight) &&
                      al4p(out) && al4p(grads) && al4p(dlog_weight),
                  "sac_cql_penalty: pointers must be 4-byte aligned");
  {
    ProfileScope t(PROF_OTHER, 0.0, stream);
    hipLaunchKernelGGL(sac_cql_penalty_kernel, dim3(1), dim3(256), 0, stream, q1_cat, q2_cat, q1_data, q2_data, log_w, mask, mask_u8, log_weight,
                       weight, temperature, target_gap, lagrange, out, grads, dlog_weight, B, M, C);
  }
  DGVIT_CHECK_LAUNCH("sac_cql_penalty");
  return DGVIT_OK;
}

int sac_scale_grads(const float* src, float* dst, long long n, const float* scale_dev, hipStream_t stream) {
  DGVIT_CHECK_ARG(src && dst && scale_dev, "sac_scale_grads: src, dst and scale_dev must not be null");
  DGVIT_CHECK_ARG(n >= 1 && n <= 3 * SAC_MAX_ELEMS, "sac_scale_grads: n=%lld must be in [1, %lld]", n, 3 * SAC_MAX_ELEMS);
  DGVIT_CHECK_ARG(al4p(src) && al4p(dst) && al4p(scale_dev), "sac_scale_grads: pointers must be 4-byte aligned");
  long long blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  {
    ProfileScope t(PROF_OTHER, 0.0, stream);
    hipLaunchKernelGGL(sac_scale_grads_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, src, dst, n, scale_dev);
  }
  DGVIT_CHECK_LAUNCH("sac_scale_grads");
  return DGVIT_OK;
}
