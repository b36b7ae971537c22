// extern "C" surface of libdgvit_hip.so (include/dgvit_hip.h) outside the encoders: errors, events, and the operator-level exports
// (GEMM, norms, attention, embedding, dropout, optimiser, heads, replay staging, depth preprocessing).
#include <stdarg.h>
#include <stdio.h>

#include "schedule.h"

// ---------------------------------------------------------------------------------------------- errors
static thread_local char g_err[512] = "";

int dgvit_set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// ---------------------------------------------------------------------------------------------- misc exports
extern "C" int dgvit_abi_version(void) { return DGVIT_ABI_VERSION; }
extern "C" int dgvit_config_size(void) { return (int)sizeof(dgvit_config); }
extern "C" const char* dgvit_last_error(void) { return g_err; }
extern "C" int dgvit_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return -1;
  return n;
}

extern "C" int dgvit_event_create(void** event) {
  DGVIT_CHECK_ARG(event, "dgvit_event_create: null pointer");
  hipEvent_t e;
  HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  *event = (void*)e;
  return DGVIT_OK;
}
extern "C" int dgvit_event_destroy(void* event) {
  if (event) HIP_TRY(hipEventDestroy((hipEvent_t)event));
  return DGVIT_OK;
}
extern "C" int dgvit_stream_wait_event(void* stream, void* event) {
  DGVIT_CHECK_ARG(event, "dgvit_stream_wait_event: null event");
  HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0));
  return DGVIT_OK;
}

// ---------------------------------------------------------------------------------------------- head Linears
extern "C" int dgvit_linear_forward(const float* x, const float* wt, const float* b, float* y, int M, int N, int K, int act,
                                    void* stream) {
  DGVIT_CHECK_ARG(act == 0 || act == 1, "linear: act must be 0 (identity) or 1 (relu)");
  DGVIT_CHECK_ARG(x && wt && y && M > 0 && N > 0 && K > 0, "linear: bad arguments");
  GemmParams p = gp(x, K, wt, K, y, N, M, N, K);
  p.bias = b;
  return gemm_f32(GEMM_NT, act ? EPI_RELU : EPI_STORE, p, 1, (hipStream_t)stream);
}

extern "C" long long dgvit_linear_backward_scratch_floats(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return -1;
  return al4((long long)M * N) + al4((long long)colsum_blocks(M) * N) + wgrad_scratch(N, K, M);
}

extern "C" int dgvit_linear_backward(const float* dy, const float* x, const float* wt, const float* y, float* dx, float* dw,
                                     float* db, float* scratch, long long scratch_floats, int M, int N, int K, int act,
                                     void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DGVIT_CHECK_ARG(act == 0 || act == 1, "linear: act must be 0 (identity) or 1 (relu)");
  DGVIT_CHECK_ARG(dy && x && wt && dw && scratch && M > 0 && N > 0 && K > 0, "linear_backward: bad arguments");
  DGVIT_CHECK_ARG(act == 0 || y, "linear_backward: relu needs the forward output");
  const long long need = dgvit_linear_backward_scratch_floats(M, N, K);
  if (scratch_floats < need) return dgvit_set_error(DGVIT_ERR_WORKSPACE, "linear_backward scratch %lld < %lld floats", scratch_floats, need);
  float* dpre = scratch;
  float* part = scratch + al4((long long)M * N);
  float* slabs = part + al4((long long)colsum_blocks(M) * N);
  const float* g = dy;
  if (act == 1) {
    TRY(relu_bwd(dy, y, dpre, (long long)M * N, st));
    g = dpre;
  }
  TRY(wgrad(g, N, x, K, dw, db, N, K, M, slabs, wgrad_scratch(N, K, M), st));
  if (dx) {
    GemmParams p = gp(g, N, wt, K, dx, K, M, K, N);
    TRY(gemm_f32(GEMM_NN, EPI_STORE, p, 1, st));
  }
  return DGVIT_OK;
}

// ---------------------------------------------------------------------------------------------- fused MLP heads
extern "C" int dgvit_mlp_head_forward(const dgvit_mlp_desc* desc, const float* const* in, const float* const* params, float* h1,
                                      float* h2, float* y, void* stream) {
  return mlp_head_forward(desc, in, params, h1, h2, y, (hipStream_t)stream);
}
extern "C" long long dgvit_mlp_head_backward_scratch_floats(const dgvit_mlp_desc* desc) { return mlp_head_backward_scratch(desc); }
extern "C" int dgvit_mlp_head_backward(const dgvit_mlp_desc* desc, const float* const* in, const float* const* params, const float* h1,
                                       const float* h2, const float* const* dy, float* const* din, float* const* dparams, float* scratch,
                                       long long scratch_floats, void* stream) {
  return mlp_head_backward(desc, in, params, h1, h2, dy, din, dparams, scratch, scratch_floats, (hipStream_t)stream);
}
extern "C" int dgvit_mlp_head_forward_shared(const dgvit_mlp_desc* desc, const int* share, const float* const* in, const float* const* params,
                                             float* h1, float* h2, float* y, void* stream) {
  return mlp_head_forward_shared(desc, share, in, params, h1, h2, y, (hipStream_t)stream);
}
extern "C" long long dgvit_mlp_head_backward_shared_scratch_floats(const dgvit_mlp_desc* desc, const int* share) {
  return mlp_head_backward_shared_scratch(desc, share);
}
extern "C" int dgvit_mlp_head_backward_shared(const dgvit_mlp_desc* desc, const int* share, const float* const* in, const float* const* params,
                                              const float* h1, const float* h2, const float* const* dy, float* const* din,
                                              float* const* dparams, float* scratch, long long scratch_floats, void* stream) {
  return mlp_head_backward_shared(desc, share, in, params, h1, h2, dy, din, dparams, scratch, scratch_floats, (hipStream_t)stream);
}

extern "C" int dgvit_tanh_gaussian_forward(const float* mean, const float* log_std_raw, const float* eps, const float* scale,
                                           const float* bias, int scale_n, float ls_min, float ls_max, float* action, float* log_prob,
                                           float* tanh_mean, int B, int A, void* stream) {
  return tanh_gaussian_forward(mean, log_std_raw, eps, scale, bias, scale_n, ls_min, ls_max, action, log_prob, tanh_mean, B, A, (hipStream_t)stream);
}
extern "C" int dgvit_tanh_gaussian_backward(const float* mean, const float* log_std_raw, const float* eps, const float* scale, int scale_n,
                                            float ls_min, float ls_max, const float* d_action, const float* d_log_prob,
                                            const float* d_tanh_mean, float* dmean, float* dlog_std_raw, int B, int A, void* stream) {
  return tanh_gaussian_backward(mean, log_std_raw, eps, scale, scale_n, ls_min, ls_max, d_action, d_log_prob, d_tanh_mean, dmean, dlog_std_raw, B, A,
                                (hipStream_t)stream);
}
extern "C" int dgvit_tanh_gaussian_log_prob(const float* mean, const float* log_std_raw, const float* action, const float* scale,
                                            const float* bias, int scale_n, float ls_min, float ls_max, float* log_prob, int B, int A,
                                            void* stream) {
  return tanh_gaussian_log_prob(mean, log_std_raw, action, scale, bias, scale_n, ls_min, ls_max, log_prob, B, A, (hipStream_t)stream);
}
extern "C" int dgvit_tanh_gaussian_log_prob_backward(const float* mean, const float* log_std_raw, const float* action, const float* scale,
                                                     const float* bias, int scale_n, float ls_min, float ls_max, const float* d_log_prob,
                                                     float* dmean, float* dlog_std_raw, int B, int A, void* stream) {
  return tanh_gaussian_log_prob_backward(mean, log_std_raw, action, scale, bias, scale_n, ls_min, ls_max, d_log_prob, dmean, dlog_std_raw, B, A,
                                         (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------- operator exports
extern "C" long long dgvit_gemm_scratch_floats(int layout, int M, int N, int K) {
  if (layout != GEMM_TN) {   // in-launch split-K: arrival counters (one per tile) + partial tiles; 0 when the shape is not split
    const GemmSplitPlan pl = gemm_split_plan(layout, M, N, K);
    return pl.nsplit > 1 ? al4(pl.tiles) + al4(pl.slab_floats) : 0;
  }
  return wgrad_scratch(M, N, K);
}

extern "C" int dgvit_gemm(int layout, int epilogue, const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M,
                          int N, int K, const float* bias, const float* res, int ldr, float* C2, int ldc2, const float* aux,
                          int ldaux, float* scratch, long long scratch_floats, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (layout == GEMM_TN) {
    DGVIT_CHECK_ARG(epilogue == EPI_STORE && !bias && !res, "gemm: layout TN supports the plain epilogue only");
    DGVIT_CHECK_ARG(ldc == N, "gemm: layout TN writes a dense C (ldc == N)");
    DGVIT_CHECK_ARG(scratch, "gemm: layout TN needs scratch");
    return wgrad(A, lda, B, ldb, C, nullptr, M, N, K, scratch, scratch_floats, st);
  }
  DGVIT_CHECK_ARG(layout == GEMM_NT || layout == GEMM_NN, "gemm: bad layout %d", layout);
  DGVIT_CHECK_ARG((epilogue >= EPI_STORE && epilogue <= EPI_DRELU) || epilogue == EPI_GELU2D || epilogue == EPI_DMUL || epilogue == EPI_GELU,
                  "gemm: bad epilogue %d", epilogue);
  DGVIT_CHECK_ARG((epilogue != EPI_GELU2 && epilogue != EPI_GELU2D) || C2, "gemm: epilogue %d needs C2", epilogue);
  DGVIT_CHECK_ARG((epilogue != EPI_DGELU && epilogue != EPI_DRELU && epilogue != EPI_DMUL) || aux, "gemm: epilogue needs aux");
  GemmParams p = gp(A, lda, B, ldb, C, ldc, M, N, K);
  p.bias = bias; p.res = res; p.ldr = ldr; p.C2 = C2; p.ldc2 = ldc2; p.aux = aux; p.ldaux = ldaux;
  const GemmSplitPlan pl = gemm_split_plan(layout, M, N, K);
  if (pl.nsplit > 1 && scratch && scratch_floats >= al4(pl.tiles) + al4(pl.slab_floats)) {
    p.counters = reinterpret_cast<int*>(scratch); p.counter_capacity = pl.tiles;
    p.slabs = scratch + al4(pl.tiles); p.slab_capacity = scratch_floats - al4(pl.tiles);
    TRY(zero_fill(scratch, (long long)sizeof(int) * pl.tiles, st));
  }
  return gemm_f32(layout, epilogue, p, 1, st);
}

extern "C" int dgvit_layernorm_forward(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                                       int rows, int D, void* stream) {
  return layernorm_fwd(x, gamma, beta, y, mean, rstd, rows, D, 1e-5f, 1, (hipStream_t)stream);
}
extern "C" long long dgvit_layernorm_backward_scratch_floats(int rows, int D) {
  if (rows <= 0 || D <= 0) return -1;
  return (long long)layernorm_bwd_blocks(rows) * 2 * D;
}
extern "C" int dgvit_layernorm_backward(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                                        const float* dres, float* dx, float* dgamma, float* dbeta, float* scratch,
                                        long long scratch_floats, int rows, int D, void* stream) {
  if (scratch_floats < dgvit_layernorm_backward_scratch_floats(rows, D))
    return dgvit_set_error(DGVIT_ERR_WORKSPACE, "layernorm_backward: scratch too small");
  return layernorm_bwd(dy, x, mean, rstd, gamma, dres, dx, dgamma, dbeta, scratch, rows, D, 1, (hipStream_t)stream);
}
extern "C" int dgvit_rmsnorm_forward(const float* x, long long ldx, const float* g, float* y, int rows, int D, void* stream) {
  return rmsnorm_fwd(x, ldx, g, y, rows, D, (hipStream_t)stream);
}
extern "C" long long dgvit_rmsnorm_backward_scratch_floats(int rows, int D) {
  if (rows <= 0 || D <= 0) return -1;
  return (long long)rmsnorm_bwd_blocks(rows) * D;
}
extern "C" int dgvit_rmsnorm_backward(const float* dy, const float* x, long long ldx, const float* g, float* dx, long long lddx,
                                      float* dg, float* scratch, long long scratch_floats, int rows, int D, void* stream) {
  if (scratch_floats < dgvit_rmsnorm_backward_scratch_floats(rows, D))
    return dgvit_set_error(DGVIT_ERR_WORKSPACE, "rmsnorm_backward: scratch too small");
  return rmsnorm_bwd(dy, x, ldx, g, dx, lddx, dg, scratch, rows, D, (hipStream_t)stream);
}
extern "C" int dgvit_attention_forward(const float* qkv, float* out, float* lse, int B, int N, int H, int dh, void* stream) {
  return attention_fwd(qkv, out, lse, B, N, H, dh, N, (hipStream_t)stream);
}
extern "C" int dgvit_attention_backward(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv,
                                        int B, int N, int H, int dh, void* stream) {
  return attention_bwd(qkv, out, dout, lse, dqkv, B, N, H, dh, N, (hipStream_t)stream);
}
extern "C" int dgvit_attention_forward_tiled(const float* qkv, float* out, float* lse, int B, int N, int H, int dh, int nq, void* stream) {
  return attention_fwd_tiled(qkv, out, lse, B, N, H, dh, nq, (hipStream_t)stream);
}
extern "C" int dgvit_attention_backward_tiled(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, float* scratch,
                                              long long scratch_floats, int B, int N, int H, int dh, int nq, void* stream) {
  return attention_bwd_tiled(qkv, out, dout, lse, dqkv, scratch, scratch_floats, B, N, H, dh, nq, (hipStream_t)stream);
}
extern "C" long long dgvit_attention_backward_tiled_scratch_floats(int B, int N, int H) {
  if (B <= 0 || N <= 0 || H <= 0) return -1;
  return attention_bwd_tiled_scratch(B, N, H);
}
// the last block's attention with K and V folded into token 0's query (last_block.hip)
extern "C" long long dgvit_goal_attention_scratch_floats(int B, int H, int D) {
  if (B <= 0 || H <= 0 || D <= 0) return -1;
  return 2ll * B * H * D;
}
extern "C" int dgvit_goal_attention_forward(const float* xn, const float* wqkv, const float* q, long long ldq, float* o, long long ldo, float* u,
                                            float* r, float* p, int B, int N, int H, int dh, int D, void* stream) {
  return goal_attention_fwd(xn, wqkv, q, ldq, o, ldo, u, r, (long long)H * D, p, B, N, H, dh, D, (hipStream_t)stream);
}
extern "C" int dgvit_goal_attention_backward(const float* xn, const float* wqkv, const float* q, long long ldq, const float* dout, long long lddo,
                                             const float* u, const float* r, const float* p, float* dq, long long lddq, float* dxn, float* dwkv,
                                             float* scratch, long long scratch_floats, int B, int N, int H, int dh, int D, void* stream) {
  const long long hd = (long long)H * D;
  if (!scratch || scratch_floats < dgvit_goal_attention_scratch_floats(B, H, D) || dgvit_goal_attention_scratch_floats(B, H, D) < 0)
    return dgvit_set_error(DGVIT_ERR_WORKSPACE, "goal_attention_backward: scratch too small");
  float* du = scratch;
  float* dr = scratch + (long long)B * hd;
  int rc = goal_attention_bwd_data(xn, wqkv, dout, lddo, u, hd, p, du, dr, hd, dq, lddq, dxn, B, N, H, dh, D, (hipStream_t)stream);
  if (rc) return rc;
  return goal_attention_wgrad(q, ldq, dout, lddo, du, hd, r, hd, dwkv, B, H, dh, D, (hipStream_t)stream);
}
extern "C" int dgvit_patchify(const float* img, float* patches, int B, int ih, int iw, int ph, int pw, void* stream) {
  return patchify(img, patches, B, ih, iw, ph, pw, (hipStream_t)stream);
}
extern "C" int dgvit_dropout(float* x, long long n, unsigned long long seed, float keep, void* stream) {
  return dropout_inplace(x, n, seed, nullptr, keep, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------- optimiser step
extern "C" int dgvit_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                               float eps, float weight_decay, long long step, const long long* step_dev, void* stream) {
  return adam_step(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, step_dev, (hipStream_t)stream);
}
extern "C" int dgvit_soft_update(float* target, const float* source, long long n, float tau, void* stream) {
  return soft_update(target, source, n, tau, (hipStream_t)stream);
}
extern "C" int dgvit_grad_sqnorm_partials(const float* g, long long n, double* partials, int accumulate, void* stream) {
  return grad_sqnorm_partials(g, n, partials, accumulate, (hipStream_t)stream);
}
extern "C" int dgvit_grad_clip_coef(const double* partials, float max_norm, float* out, void* stream) {
  return grad_clip_coef(partials, max_norm, out, (hipStream_t)stream);
}
extern "C" int dgvit_adam_step_scaled(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                                      float eps, float weight_decay, long long step, const long long* step_dev,
                                      const float* grad_scale_dev, void* stream) {
  return adam_step_scaled(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, step_dev, grad_scale_dev, (hipStream_t)stream);
}
extern "C" int dgvit_scale_by_device_scalar(float* x, long long n, const float* scale_dev, void* stream) {
  return scale_by_device_scalar(x, n, scale_dev, (hipStream_t)stream);
}
extern "C" int dgvit_adam_step_groups(float* p, const float* g, float* m, float* v, long long n, const long long* seg_end4,
                                      const unsigned char* seg_group, int nseg, const float* group_hyper, int ngroups, float* lr_out,
                                      float beta1, float beta2, float eps, int decoupled, long long step, long long sched_step,
                                      const long long* step_dev, int sched_kind, long long warmup_steps, long long total_steps,
                                      float final_ratio, const float* grad_scale_dev, void* stream) {
  return adam_step_groups(p, g, m, v, n, seg_end4, seg_group, nseg, group_hyper, ngroups, lr_out, beta1, beta2, eps, decoupled, step, sched_step,
                          step_dev, sched_kind, warmup_steps, total_steps, final_ratio, grad_scale_dev, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------- SAC loss head (sac_loss.hip)
extern "C" int dgvit_sac_critic_loss(const float* q1, const float* q2, const float* reward, const float* done, const float* weights,
                                     const float* next_q1, const float* next_q2, const float* next_log_pi, const float* log_alpha, float alpha,
                                     float gamma, float* target, float* td, float* loss, float* grads, int B, int A, void* stream) {
  return sac_critic_loss(q1, q2, reward, done, weights, nullptr, next_q1, next_q2, next_log_pi, log_alpha, alpha, gamma, target, td, loss, grads,
                         B, A, (hipStream_t)stream);
}
extern "C" int dgvit_sac_critic_loss_v2(const float* q1, const float* q2, const float* reward, const float* done, const float* weights,
                                        const float* discount, const float* next_q1, const float* next_q2, const float* next_log_pi,
                                        const float* log_alpha, float alpha, float gamma, float* target, float* td, float* loss, float* grads,
                                        int B, int A, void* stream) {
  return sac_critic_loss(q1, q2, reward, done, weights, discount, next_q1, next_q2, next_log_pi, log_alpha, alpha, gamma, target, td, loss,
                         grads, B, A, (hipStream_t)stream);
}
extern "C" int dgvit_sac_actor_loss(const float* log_pi, const float* q1_pi, const float* q2_pi, const float* log_alpha, float alpha,
                                    int with_temperature, float target_entropy, float* losses, float* grads, float* dlog_alpha, int B, int A,
                                    void* stream) {
  return sac_actor_loss(log_pi, q1_pi, q2_pi, log_alpha, alpha, with_temperature, target_entropy, losses, grads, dlog_alpha, B, A,
                        (hipStream_t)stream);
}
extern "C" int dgvit_sac_scale_grads(const float* src, float* dst, long long n, const float* scale_dev, void* stream) {
  return sac_scale_grads(src, dst, n, scale_dev, (hipStream_t)stream);
}
extern "C" int dgvit_sac_bc_loss(const float* pred, const float* action, const void* mask, int mask_u8, const float* q1_demo,
                                 const float* q2_demo, const float* q1_pi, const float* q2_pi, int nll, float* out, float* grads, int B, int A,
                                 void* stream) {
  return sac_bc_loss(pred, action, mask, mask_u8, q1_demo, q2_demo, q1_pi, q2_pi, nll, out, grads, B, A, (hipStream_t)stream);
}
extern "C" int dgvit_sac_cql_penalty(const float* q1_cat, const float* q2_cat, const float* q1_data, const float* q2_data, const float* log_w,
                                     const void* mask, int mask_u8, const float* log_weight, float weight, float temperature, float target_gap,
                                     int lagrange, float* out, float* grads, float* dlog_weight, int B, int M, int C, void* stream) {
  return sac_cql_penalty(q1_cat, q2_cat, q1_data, q2_data, log_w, mask, mask_u8, log_weight, weight, temperature, target_gap, lagrange, out, grads,
                         dlog_weight, B, M, C, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------- replay staging
extern "C" int dgvit_gather_rows(const float* src, const long long* idx, float* out, long long nsel, long long row_floats,
                                 long long nrows, void* stream) {
  return gather_rows(src, idx, out, nsel, row_floats, nrows, (hipStream_t)stream);
}
extern "C" int dgvit_gather_shift_frames(const float* src, const long long* idx, float* out, int* shifts_out, long long nsel, int H, int W,
                                         long long row_floats, long long nrows, int pad, int stream_id, unsigned long long seed,
                                         const unsigned long long* seed_dev, void* stream) {
  return gather_shift_frames(src, idx, out, shifts_out, nsel, H, W, row_floats, nrows, pad, stream_id, seed, seed_dev, (hipStream_t)stream);
}
// the ring with uint8 frame storage (replay_ring.hip)
extern "C" int dgvit_quantize_rows_u8(const float* src, long long src_ld, unsigned char* ring, long long n, long long cols,
                                      long long row_bytes, long long nrows, long long start, void* stream) {
  return quantize_rows_u8(src, src_ld, ring, n, cols, row_bytes, nrows, start, (hipStream_t)stream);
}
extern "C" int dgvit_gather_rows_u8(const unsigned char* ring, const long long* idx, float* out, long long nsel, long long cols,
                                    long long row_bytes, long long row_floats, long long nrows, void* stream) {
  return gather_rows_u8(ring, idx, out, nsel, cols, row_bytes, row_floats, nrows, (hipStream_t)stream);
}
extern "C" int dgvit_gather_shift_frames_u8(const unsigned char* ring, const long long* idx, float* out, int* shifts_out, long long nsel, int H,
                                            int W, long long row_bytes, long long row_floats, long long nrows, int pad, int stream_id,
                                            unsigned long long seed, const unsigned long long* seed_dev, void* stream) {
  return gather_shift_frames_u8(ring, idx, out, shifts_out, nsel, H, W, row_bytes, row_floats, nrows, pad, stream_id, seed, seed_dev,
                                (hipStream_t)stream);
}
// episode flags and the n-step walk (replay_ring.hip)
extern "C" int dgvit_ring_mark(unsigned char* flags, long long nrows, long long start, long long n, void* stream) {
  return ring_mark(flags, nrows, start, n, (hipStream_t)stream);
}
extern "C" int dgvit_nstep_walk(const float* rew, long long rew_ld, const float* done, long long done_ld, const unsigned char* flags,
                                const float* next_small, long long small_ld, const long long* idx, long long nsel, long long nrows, int n,
                                double gamma, float* ret_out, float* done_out, float* discount_out, float* next_small_out, int* steps_out,
                                long long* tail_out, void* stream) {
  return nstep_walk(rew, rew_ld, done, done_ld, flags, next_small, small_ld, idx, nsel, nrows, n, gamma, ret_out, done_out, discount_out,
                    next_small_out, steps_out, tail_out, (hipStream_t)stream);
}
// the ring of E parallel environments (replay_ring.hip)
extern "C" int dgvit_ring_store_frames(const void* src0, int src0_u8, long long src0_ld, const void* src1, int src1_u8, long long src1_ld,
                                       void* ring0, void* ring1, int ring_u8, long long ring_ld, long long n, long long cols,
                                       long long nrows, long long start, void* stream) {
  return ring_store_frames(src0, src0_u8, src0_ld, src1, src1_u8, src1_ld, ring0, ring1, ring_u8, ring_ld, n, cols, nrows, start,
                           (hipStream_t)stream);
}
extern "C" int dgvit_ring_store_small(dgvit_small_fields fields, unsigned char* flags, const void* episode_end, int end_f32, long long n,
                                      long long nrows, long long start, void* stream) {
  return ring_store_small(fields, flags, episode_end, end_f32, n, nrows, start, (hipStream_t)stream);
}
extern "C" int dgvit_nstep_walk_strided(const float* rew, long long rew_ld, const float* done, long long done_ld, const unsigned char* flags,
                                        const float* next_small, long long small_ld, const long long* idx, long long nsel, long long nrows,
                                        long long stride, int n, double gamma, float* ret_out, float* done_out, float* discount_out,
                                        float* next_small_out, int* steps_out, long long* tail_out, void* stream) {
  return nstep_walk_strided(rew, rew_ld, done, done_ld, flags, next_small, small_ld, idx, nsel, nrows, stride, n, gamma, ret_out, done_out,
                            discount_out, next_small_out, steps_out, tail_out, (hipStream_t)stream);
}
// the ring that stores each frame once (replay_ring.hip)
extern "C" int dgvit_ring_plan_next(int* next_row, long long* state, int* moves, const float* done, long long done_ld,
                                    const unsigned char* flags, long long n, long long nrows, long long start, long long envs, long long pool,
                                    void* stream) {
  return ring_plan_next(next_row, state, moves, done, done_ld, flags, n, nrows, start, envs, pool, (hipStream_t)stream);
}
extern "C" int dgvit_ring_store_frames_shared(const void* src0, int src0_u8, long long src0_ld, const void* src1, int src1_u8,
                                              long long src1_ld, void* arena, const int* moves, int ring_u8, long long ring_ld, long long n,
                                              long long cols, long long nrows, long long start, long long envs, long long pool, void* stream) {
  return ring_store_frames_shared(src0, src0_u8, src0_ld, src1, src1_u8, src1_ld, arena, moves, ring_u8, ring_ld, n, cols, nrows, start, envs,
                                  pool, (hipStream_t)stream);
}
extern "C" int dgvit_ring_next_rows(const int* next_row, const long long* idx, long long* out, long long nsel, long long nrows, void* stream) {
  return ring_next_rows(next_row, idx, out, nsel, nrows, (hipStream_t)stream);
}
// frame stacks at sample time and on the acting side (replay_ring.hip)
extern "C" int dgvit_ring_stack_rows(const long long* idx, const long long* tail, const unsigned char* flags, const float* done,
                                     long long done_ld, const int* next_row, long long* obs_rows, long long* next_rows, long long nsel,
                                     long long nrows, long long envs, int frames, int full, long long arena_rows, void* stream) {
  return ring_stack_rows(idx, tail, flags, done, done_ld, next_row, obs_rows, next_rows, nsel, nrows, envs, frames, full, arena_rows,
                         (hipStream_t)stream);
}
extern "C" int dgvit_gather_stack_frames(const void* src0, const void* src1, const long long* rows, float* out, long long nsel, long long cols,
                                         int frames, int ring_u8, long long ring_ld, long long row_floats, long long nrows0, long long nrows1,
                                         void* stream) {
  return gather_stack_frames(src0, src1, rows, out, nsel, cols, frames, ring_u8, ring_ld, row_floats, nrows0, nrows1, (hipStream_t)stream);
}
extern "C" int dgvit_gather_shift_stack_frames(const void* src0, const void* src1, const long long* rows, float* out, int* shifts_out,
                                               long long nsel, int H, int W, int frames, int ring_u8, long long ring_ld, long long row_floats,
                                               long long nrows0, long long nrows1, int pad, int stream_id, unsigned long long seed,
                                               const unsigned long long* seed_dev, void* stream) {
  return gather_shift_stack_frames(src0, src1, rows, out, shifts_out, nsel, H, W, frames, ring_u8, ring_ld, row_floats, nrows0, nrows1, pad,
                                   stream_id, seed, seed_dev, (hipStream_t)stream);
}
extern "C" int dgvit_frame_stack_push(float* stack, const float* frame, long long frame_ld, const unsigned char* reset, int reset_all,
                                      long long envs, long long cols, int frames, void* stream) {
  return frame_stack_push(stack, frame, frame_ld, reset, reset_all, envs, cols, frames, (hipStream_t)stream);
}
// the ring as a file (replay_ring.hip, replay.hip)
extern "C" int dgvit_ring_export(dgvit_ring_view ring, void* out, long long out_bytes, long long cols, long long nrows, long long oldest,
                                 long long a0, long long n, void* stream) {
  return ring_export(ring, out, out_bytes, cols, nrows, oldest, a0, n, (hipStream_t)stream);
}
extern "C" int dgvit_per_set_leaves(float* tree, long long capacity, long long first, long long count, const float* leaves, void* stream) {
  return per_set_leaves(tree, capacity, first, count, leaves, (hipStream_t)stream);
}
// prioritized replay (replay.hip)
extern "C" long long dgvit_per_tree_floats(long long capacity) { return per_tree_floats(capacity); }
extern "C" int dgvit_per_init(float* tree, long long capacity, void* stream) { return per_init(tree, capacity, (hipStream_t)stream); }
extern "C" int dgvit_per_set_range(float* tree, long long capacity, long long first, long long count, void* stream) {
  return per_set_range(tree, capacity, first, count, (hipStream_t)stream);
}
extern "C" int dgvit_per_update(float* tree, long long capacity, long long stored, const long long* idx, const float* prio, long long n,
                                float alpha, float eps, void* stream) {
  return per_update(tree, capacity, stored, idx, prio, n, alpha, eps, (hipStream_t)stream);
}
extern "C" int dgvit_per_sample(const float* tree, long long capacity, const float* uniforms, long long n, int stratified, float beta,
                                long long* idx_out, float* weights_out, void* stream) {
  return per_sample(tree, capacity, uniforms, n, stratified, beta, idx_out, weights_out, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------- SURVEY 8(f4)
extern "C" long long dgvit_depth_preprocess_scratch_floats(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return -1;
  return 2 * al4((long long)B * H * W) + al4(depth_normalize_scratch_floats(B));
}
extern "C" int dgvit_depth_normalize_u8(const float* depth, float* out, float* scratch, long long scratch_floats, int B, int H, int W,
                                        void* stream) {
  DGVIT_CHECK_ARG(scratch && scratch_floats >= depth_normalize_scratch_floats(B), "dgvit_depth_normalize_u8: scratch too small");
  return depth_normalize_u8(depth, out, scratch, B, H, W, (hipStream_t)stream);
}
extern "C" int dgvit_noise_clip(const float* img, const float* noise, float* out, long long n, float noise_level, unsigned long long seed,
                                void* stream) {
  return noise_clip(img, noise, out, n, noise_level, seed, (hipStream_t)stream);
}
extern "C" int dgvit_gaussian_blur(const float* img, float* out, float* tmp, int B, int H, int W, int ksize, int row0, int row1,
                                   void* stream) {
  return gaussian_blur_band(img, out, tmp, B, H, W, ksize, row0, row1, (hipStream_t)stream);
}
extern "C" int dgvit_resize_bilinear(const float* img, float* out, int B, int Hs, int Ws, int Hd, int Wd, float scale, void* stream) {
  return resize_bilinear(img, out, B, Hs, Ws, Hd, Wd, scale, (hipStream_t)stream);
}
// listener_callback (env_lab.py:420-434) + the resize of step() / reset() (:295-299): depth (B, H, W) -> state (B, out_h, out_w) in [0, 1]
extern "C" int dgvit_depth_to_state(const float* depth, const float* noise, float noise_level, unsigned long long seed, float* state,
                                    float* scratch, long long scratch_floats, int B, int H, int W, int out_h, int out_w, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DGVIT_CHECK_ARG(depth && state && scratch && B > 0 && H > 0 && W > 0 && out_h > 0 && out_w > 0, "dgvit_depth_to_state: bad arguments");
  DGVIT_CHECK_ARG(((long long)H * W) % 4 == 0, "dgvit_depth_to_state: H * W must be a multiple of 4");
  const long long n = (long long)B * H * W;
  if (scratch_floats < dgvit_depth_preprocess_scratch_floats(B, H, W))
    return dgvit_set_error(DGVIT_ERR_WORKSPACE, "dgvit_depth_to_state: scratch %lld < %lld floats", scratch_floats,
                           dgvit_depth_preprocess_scratch_floats(B, H, W));
  float* a = scratch;
  float* b = scratch + al4(n);
  float* part = b + al4(n);
  TRY(depth_normalize_u8(depth, a, part, B, H, W, st));              // :424-426
  TRY(noise_clip(a, noise, a, n, noise_level, seed, st));             // add_nose :86-88
  TRY(gaussian_blur_band(a, a, b, B, H, W, 5, 0, H, st));             // add_nose :89   (b = horizontal pass, a = result)
  const int bh = H / 5, y1 = H / 2 - bh / 2;                          // get_center_band :33-39
  TRY(gaussian_blur_band(a, a, b, B, H, W, 11, y1, y1 + bh, st));     // blurring :69-76
  return resize_bilinear(a, state, B, H, W, out_h, out_w, 1.0f / 255.0f, st);   // :295, :299
}
