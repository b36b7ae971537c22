// The diagnostic library's knobs and the entry points of include/dgvit_hip_diag.h (libdgvit_hip_diag.so only).
#define DGVIT_KNOB_DEFINE   // knobs.h: this translation unit defines every knob with its default
#include "../../include/dgvit_hip_diag.h"
#include "schedule.h"

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
extern "C" void dgvit_set_gemm_bf16_group_m(int rows) { g_gemm_bf16_group_m = rows > 0 ? rows : g_gemm_bf16_group_m_default; }
extern "C" void dgvit_set_gemm_bf16_stamps(long long* stamps) { g_gemm_bf16_stamps = stamps; }
extern "C" void dgvit_set_gemm_bf16_l2_budget_kb(int kb) { g_gemm_bf16_l2_budget_kb = kb > 0 ? kb : 0; }
