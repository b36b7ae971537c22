// The diagnostic library's knobs and the entry points of include/dgvit_hip_diag.h (libdgvit_hip_diag.so only).
#define DGVIT_KNOB_DEFINE   // knobs.h: this translation unit defines every knob with its default
#include "../../include/dgvit_hip_diag.h"
#include "schedule.h"
#include "bf16.h"

#ifndef DGVIT_DIAG
#error "diag_api.hip belongs to the diagnostic library only (-DDGVIT_DIAG)"
#endif

long long g_gemm_persist_launches = 0;

extern "C" void dgvit_set_gemm_tile(int tile) { g_gemm_tile_hint = tile; }
extern "C" void dgvit_set_grouped_reduce(int on) { g_group_reduce = on ? 1 : 0; }
extern "C" void dgvit_set_conv_gather(int on) { g_conv_gather = on ? 1 : 0; }
extern "C" void dgvit_set_ln_fusion(int on) { g_ln_fusion = on ? 1 : 0; }
extern "C" void dgvit_set_gemm_split(int on) { g_gemm_split = on ? 1 : 0; }
extern "C" void dgvit_set_gemm_stamps(long long* stamps, int workgroups) {
  g_gemm_stamps = stamps;
  g_gemm_stamp_capacity = stamps ? workgroups : 0;
}
extern "C" long long dgvit_gemm_persistent_launches(void) { return g_gemm_persist_launches; }
extern "C" void dgvit_set_gemm_persistent(int mode, int workgroups) {
  g_gemm_persist = mode < 0 ? 0 : (mode > 2 ? 2 : mode);
  g_gemm_persist_grid = workgroups > 0 ? workgroups : 0;
}
extern "C" void dgvit_set_gemm_diagnostics(int on) { g_gemm_diag = on & 0x3FFFFF; }
extern "C" void dgvit_set_gemm_lds_pad(int bytes) { g_gemm_lds_pad = bytes > 0 ? bytes : 0; }
extern "C" void dgvit_set_small_batch_path(int on, int max_rows) {
  g_small_path = on ? 1 : 0;
  if (max_rows > 0) g_small_path_max_rows = max_rows;
}
extern "C" void dgvit_set_block_path(int on, int max_rows) {
  g_block_path = on < 0 ? 0 : (on > 2 ? 2 : on);
  g_block_path_max_rows = max_rows > 0 ? max_rows : g_block_path_max_rows_default;
}
extern "C" void dgvit_set_block_stamps(long long* stamps) { g_block_stamps = stamps; }
extern "C" void dgvit_set_block_stamp_layer(int layer) { g_block_stamp_layer = layer; }
extern "C" void dgvit_set_gelu_grad_store(int on) { g_gelu_grad_store = on ? 1 : 0; }
extern "C" void dgvit_set_block_fuse(int bits) { g_block_fuse = bits & 3; }
extern "C" void dgvit_set_gemm_bf16_tile(int tile) { g_gemm_bf16_tile_hint = tile; }
extern "C" void dgvit_set_gemm_bf16_mfma16(int on) { g_gemm_bf16_m16 = on ? 1 : 0; }
extern "C" void dgvit_set_attention_bwd_single_pass(int on) { g_attn_bwd64 = on ? 1 : 0; }
extern "C" void dgvit_set_attention_single_query(int on) { g_attn_q1 = on ? 1 : 0; }
extern "C" void dgvit_set_last_block_fold(int on) { g_last_block_fold = on ? 1 : 0; }
extern "C" void dgvit_set_attention_bf16_tiled_waves(int waves) { g_attn_bf16_tiled_waves = waves == 8 ? 8 : waves == 4 ? 4 : g_attn_bf16_tiled_waves_default; }
extern "C" void dgvit_set_attention_bf16_long(int bits) { g_attn_bf16_long = bits < 0 ? g_attn_bf16_long_default : (bits & 3); }
extern "C" void dgvit_set_gemm_wgrad_slice_major(int on) { g_gemm_zfold = on ? 1 : 0; }
extern "C" int dgvit_attention_forward_queries(const float* qkv, float* out, float* lse, int B, int N, int H, int dh, int nq, void* stream) {
  return attention_fwd(qkv, out, lse, B, N, H, dh, nq, (hipStream_t)stream);
}
extern "C" int dgvit_attention_backward_queries(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv,
                                                int B, int N, int H, int dh, int nq, void* stream) {
  return attention_bwd(qkv, out, dout, lse, dqkv, B, N, H, dh, nq, (hipStream_t)stream);
}
extern "C" int dgvit_attention_forward_bf16_queries(const unsigned short* qkv, unsigned short* out, float* lse, int B, int N, int H, int dh,
                                                    int nq, void* stream) {
  return attention_fwd_bf16((const bf16_t*)qkv, (bf16_t*)out, lse, B, N, H, dh, nq, (hipStream_t)stream);
}
// ---- the fp32 attention kernels with the site-0 mask of one layer (tests/test_gpu_attention_fp32_matrix.py): in the product only the
// encoder reaches the DROP instantiations
namespace {
int check_attn_layer(const char* what, int layer) {   // check_layer_site of encoder_bf16.hip, for the one site these entries have
  DGVIT_CHECK_ARG(layer >= 0 && layer < (1 << 22), "%s: layer=%d outside [0, 2^22)", what, layer);
  return DGVIT_OK;
}
}  // namespace
extern "C" int dgvit_attention_forward_drop(const float* qkv, float* out, float* lse, int B, int N, int H, int dh, int nq, float keep,
                                            unsigned long long seed, const unsigned long long* seed_dev, int layer, void* stream) {
  TRY(check_attn_layer("dgvit_attention_forward_drop", layer));
  DGVIT_CHECK_ARG(keep > 0.f && keep <= 1.f, "dgvit_attention_forward_drop: keep=%g outside (0, 1]", (double)keep);
  const LayerDrop drop{keep, drop_tag(layer, DROP_ATTN), seed, seed_dev};
  return attention_fwd(qkv, out, lse, B, N, H, dh, nq, (hipStream_t)stream, &drop);
}
extern "C" int dgvit_attention_backward_drop(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int B,
                                             int N, int H, int dh, int nq, float keep, unsigned long long seed,
                                             const unsigned long long* seed_dev, int layer, void* stream) {
  TRY(check_attn_layer("dgvit_attention_backward_drop", layer));
  DGVIT_CHECK_ARG(keep > 0.f && keep <= 1.f, "dgvit_attention_backward_drop: keep=%g outside (0, 1]", (double)keep);
  const LayerDrop drop{keep, drop_tag(layer, DROP_ATTN), seed, seed_dev};
  return attention_bwd(qkv, out, dout, lse, dqkv, B, N, H, dh, nq, (hipStream_t)stream, &drop);
}
extern "C" int dgvit_attention_forward_tiled_drop(const float* qkv, float* out, float* lse, int B, int N, int H, int dh, int nq, float keep,
                                                  unsigned long long seed, const unsigned long long* seed_dev, int layer, void* stream) {
  TRY(check_attn_layer("dgvit_attention_forward_tiled_drop", layer));
  DGVIT_CHECK_ARG(keep > 0.f && keep <= 1.f, "dgvit_attention_forward_tiled_drop: keep=%g outside (0, 1]", (double)keep);
  const LayerDrop drop{keep, drop_tag(layer, DROP_ATTN), seed, seed_dev};
  return attention_fwd_tiled(qkv, out, lse, B, N, H, dh, nq, (hipStream_t)stream, &drop);
}
extern "C" int dgvit_attention_backward_tiled_drop(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv,
                                                   float* scratch, long long scratch_floats, int B, int N, int H, int dh, int nq,
                                                   float keep, unsigned long long seed, const unsigned long long* seed_dev, int layer,
                                                   void* stream) {
  TRY(check_attn_layer("dgvit_attention_backward_tiled_drop", layer));
  DGVIT_CHECK_ARG(keep > 0.f && keep <= 1.f, "dgvit_attention_backward_tiled_drop: keep=%g outside (0, 1]", (double)keep);
  const LayerDrop drop{keep, drop_tag(layer, DROP_ATTN), seed, seed_dev};
  return attention_bwd_tiled(qkv, out, dout, lse, dqkv, scratch, scratch_floats, B, N, H, dh, nq, (hipStream_t)stream, &drop);
}
extern "C" void dgvit_set_gemm_bf16_group_m(int rows) { g_gemm_bf16_group_m = rows > 0 ? rows : g_gemm_bf16_group_m_default; }
extern "C" void dgvit_set_gemm_bf16_stamps(long long* stamps) { g_gemm_bf16_stamps = stamps; }
extern "C" void dgvit_set_gemm_bf16_l2_budget_kb(int kb) { g_gemm_bf16_l2_budget_kb = kb > 0 ? kb : 0; }

// ---- the row kernels with every argument the encoder schedules use (tests/test_gpu_row_kernels.py); the product ABI fixes row_step = 1,
// both parameter gradients and a direct reduction
extern "C" int dgvit_diag_layernorm_forward(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                                            int rows, int D, int row_step, void* stream) {
  return layernorm_fwd(x, gamma, beta, y, mean, rstd, rows, D, 1e-5f, row_step, (hipStream_t)stream);
}
extern "C" int dgvit_diag_layernorm_backward(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                                             const float* dres, float* dx, float* dgamma, float* dbeta, float* scratch,
                                             long long scratch_floats, int rows, int D, int row_step, int grouped, void* stream) {
  if (rows <= 0 || D <= 0 || scratch_floats < (long long)layernorm_bwd_blocks(rows) * 2 * D)
    return dgvit_set_error(DGVIT_ERR_WORKSPACE, "diag_layernorm_backward: scratch too small");
  DGVIT_CHECK_ARG(row_step >= 1, "diag_layernorm_backward: bad row step");
  hipStream_t st = (hipStream_t)stream;
  if (!grouped) return layernorm_bwd(dy, x, mean, rstd, gamma, dres, dx, dgamma, dbeta, scratch, rows, D, row_step, st);
  ReduceGroup grp;     // as a layer of dgvit_got_backward queues it: the reduction runs in the group's flush
  reduce_group_init(grp);
  TRY(layernorm_bwd(dy, x, mean, rstd, gamma, dres, dx, dgamma, dbeta, scratch, rows, D, row_step, st, &grp));
  return reduce_group_flush(grp, st);
}
// the dispatch of encoder_bf16.hip: no delta -> layernorm_fwd_bf16; delta with xout and statistics -> add_layernorm_fwd_bf16 (the
// training schedule and the pruned last block); delta2, or delta without xout / statistics -> add2_layernorm_fwd_bf16 (the no-grad
// schedule: contiguous rows, no statistics)
extern "C" int dgvit_diag_layernorm_forward_bf16(const float* x, const unsigned short* delta, const unsigned short* delta2, float* xout,
                                                 const float* gamma, const float* beta, unsigned short* y, float* mean, float* rstd,
                                                 int rows, int D, int row_step, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DGVIT_CHECK_ARG(row_step >= 1 && (mean == nullptr) == (rstd == nullptr), "diag_layernorm_forward_bf16: bad row step, or one of mean / rstd without the other");
  DGVIT_CHECK_ARG(delta || (!delta2 && !xout), "diag_layernorm_forward_bf16: delta2 / xout without delta");
  if (!delta) return layernorm_fwd_bf16(x, gamma, beta, y, mean, rstd, rows, D, 1e-5f, row_step, st);
  if (!delta2 && xout && mean) return add_layernorm_fwd_bf16(x, delta, xout, gamma, beta, y, mean, rstd, rows, D, 1e-5f, row_step, st);
  DGVIT_CHECK_ARG(row_step == 1 && !mean, "diag_layernorm_forward_bf16: the joint form has contiguous rows and no statistics");
  return add2_layernorm_fwd_bf16(x, delta, delta2, xout, gamma, beta, y, rows, D, 1e-5f, st);
}
extern "C" int dgvit_diag_layernorm_backward_bf16(const unsigned short* dy, const float* x, const float* mean, const float* rstd,
                                                  const float* gamma, const float* dres, float* dx, unsigned short* dxb, float* dgamma,
                                                  float* dbeta, float* scratch, long long scratch_floats, int rows, int D, int row_step,
                                                  void* stream) {
  if (rows <= 0 || D <= 0 || scratch_floats < (long long)layernorm_bwd_blocks(rows) * 2 * D)
    return dgvit_set_error(DGVIT_ERR_WORKSPACE, "diag_layernorm_backward_bf16: scratch too small");
  DGVIT_CHECK_ARG(row_step >= 1, "diag_layernorm_backward_bf16: bad row step");
  return layernorm_bwd_bf16(dy, x, mean, rstd, gamma, dres, dx, dxb, dgamma, dbeta, scratch, rows, D, row_step, (hipStream_t)stream);
}
extern "C" int dgvit_diag_residual_add_bf16(const float* x, const unsigned short* delta, float* xout, int rows, int D, int row_step,
                                            void* stream) {
  DGVIT_CHECK_ARG(row_step >= 1, "diag_residual_add_bf16: bad row step");
  return residual_add_bf16(x, delta, xout, rows, D, row_step, (hipStream_t)stream);
}
extern "C" int dgvit_diag_transpose_cast_f32_bf16(const float* src, unsigned short* dst, int rows, int cols, void* stream) {
  return transpose_cast_f32_bf16(src, dst, rows, cols, (hipStream_t)stream);
}
extern "C" long long dgvit_diag_colsum_scratch_floats(int rows, int cols) {
  if (rows <= 0 || cols <= 0) return -1;
  return (long long)colsum_blocks(rows) * cols;
}
extern "C" int dgvit_diag_colsum(const float* a, long long lda, float* out, float* scratch, long long scratch_floats, int rows, int cols,
                                 int rgrp, void* stream) {
  if (rows <= 0 || cols <= 0 || scratch_floats < (long long)colsum_blocks(rows) * cols)
    return dgvit_set_error(DGVIT_ERR_WORKSPACE, "diag_colsum: scratch too small");
  DGVIT_CHECK_ARG(lda >= cols && rgrp >= 0, "diag_colsum: lda=%lld < cols=%d, or a negative row group", lda, cols);
  return colsum(a, lda, out, scratch, rows, cols, rgrp, (hipStream_t)stream);
}
