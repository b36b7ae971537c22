// Host-side pieces shared by the translation units of the C ABI (api.hip, encoder.hip, encoder_bf16.hip, cnn_api.hip, diag_api.hip):
// the fp32 weight-gradient GEMM, the encoder's dimensions and parameter slots, and the schedule steps that the fp32 and
// the bf16 encoder have in common.  Internal: not installed.
#pragma once
#include <algorithm>

#include "../../include/dgvit_hip.h"
#include "common.h"
#include "kernels.h"

inline long long al4(long long n) { return (n + 3) & ~3ll; }

// Schedule options travel with every call in dgvit_config.flags (the forward and its backward see the same value, whatever thread
// runs them); A/B and diagnostic knobs are compile-time constants in the product build (knobs.h).
inline bool dense_last_block(const dgvit_config* c) { return (c->flags & DGVIT_FLAG_DENSE_LAST_BLOCK) != 0; }
inline bool wgrad_overlap(const dgvit_config* c) { return (c->flags & DGVIT_FLAG_WGRAD_OVERLAP) != 0; }
inline bool long_sequence(const dgvit_config* c) { return (c->flags & DGVIT_FLAG_LONG_SEQUENCE) != 0; }

// ---------------------------------------------------------------------------------------------- fp32 GEMM helpers
inline GemmParams gp(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K) {
  GemmParams p = {};
  p.A = A; p.lda = lda; p.B = B; p.ldb = ldb; p.C = C; p.ldc = ldc;
  p.M = M; p.N = N; p.K = K; p.kchunk = (K + 31) / 32 * 32;
  return p;
}

// split-K plan for weight gradients: tiles x splits ~ 2 workgroups per CU (all co-resident, one balanced wave)
inline int wgrad_splits(int M, int N, int K) {
  const int bt = (M >= 128 && N >= 128) ? 128 : 64;  // must mirror pick_tile's automatic TN choice
  const long long tiles = (long long)((M + bt - 1) / bt) * ((N + bt - 1) / bt);
  long long s = 512 / tiles;
  const long long maxs = ((long long)K + 255) / 256;  // at least 8 k-tiles per split (64-bit: K + 255 wraps for K near 2^31)
  if (s > maxs) s = maxs;
  if (s > 256) s = 256;
  if (s < 1) s = 1;
  return (int)s;
}

inline long long wgrad_slab(int M, int N) { return al4((long long)M * N + M); }
inline long long wgrad_scratch(int M, int N, int K) { return (long long)wgrad_splits(M, N, K) * wgrad_slab(M, N); }

// dW (M x N) = A^T B with A (K x M, lda), B (K x N, ldb); optional db (M) = column sums of A (fused in the kernel);
// dW == nullptr: the weight is frozen (its requires_grad is off): only the bias gradient, if wanted, is computed.
// grp != null: the slab reduction is queued there and `scratch` must stay untouched until the caller has flushed the group.
inline int wgrad(const float* A, int lda, const float* B, int ldb, float* dW, float* db, int M, int N, int K, float* scratch,
                 long long scratch_floats, hipStream_t st, ReduceGroup* grp = nullptr) {
  if (!dW) {
    if (!db) return DGVIT_OK;
    if (scratch_floats < (long long)colsum_blocks(K) * M) return dgvit_set_error(DGVIT_ERR_WORKSPACE, "wgrad: scratch too small for the bias gradient");
    return colsum(A, lda, db, scratch, K, M, 0, st);
  }
  const int ns = wgrad_splits(M, N, K);
  const long long slab = wgrad_slab(M, N);
  if (scratch_floats < ns * slab) return dgvit_set_error(DGVIT_ERR_WORKSPACE, "wgrad: scratch %lld < %lld floats", scratch_floats, ns * slab);
  GemmParams p = gp(A, lda, B, ldb, scratch, N, M, N, K);
  const int kt = (K + 31) / 32;
  p.kchunk = ((kt + ns - 1) / ns) * 32;
  p.slab_stride = slab;
  p.colsum = db ? 1 : 0;
  const int ns_eff = (K + p.kchunk - 1) / p.kchunk;
  TRY(gemm_f32(GEMM_TN, EPI_SPLITK, p, ns_eff, st));
  const long long mn = (long long)M * N;
  ReduceGroup local;
  if (!grp) reduce_group_init(local);
  ReduceGroup& g = grp ? *grp : local;
  if (db && mn % 4 == 0) {
    TRY(reduce_group_add(g, scratch, dW, mn, db, mn + M, ns_eff, slab, st));
  } else {
    TRY(reduce_group_add(g, scratch, dW, mn, nullptr, mn, ns_eff, slab, st));
    if (db) TRY(reduce_group_add(g, scratch + mn, db, M, nullptr, M, ns_eff, slab, st));
  }
  return grp ? DGVIT_OK : reduce_group_flush(local, st);
}

// scratch of the in-launch split-K GEMMs (gemm.hip): fp32 partial tiles + one arrival counter per output tile
struct SplitNeed {
  long long slab = 0;
  long long tiles = 0;
  void take(const GemmSplitPlan& pl) {
    if (pl.nsplit > 1) {
      slab = std::max(slab, pl.slab_floats);
      tiles = std::max<long long>(tiles, pl.tiles);
    }
  }
  void add(int layout, long long M, int N, int K) {
    if (M > 0) take(gemm_split_plan(layout, (int)M, N, K));
  }
  void add_gather(long long M, int N, int K) {     // A gathered from an image (fixed 64 x 64 x 32 tile)
    if (M > 0) take(gemm_split_plan_gather((int)M, N, K));
  }
};
struct SplitBuf {
  int* counters = nullptr; float* slabs = nullptr; long long slab_cap = 0; int ncounters = 0;
  void attach(GemmParams& p) const {
    p.counters = counters; p.slabs = slabs; p.slab_capacity = slab_cap; p.counter_capacity = ncounters;
  }
};

// ---------------------------------------------------------------------------------------------- encoder dimensions and parameters
struct Dims {
  int B, P, N, D, I, M, L, H, dh, pd, pool_mean;
  int proj;       // 0: heads == 1 and dim_head == dim -- the reference's Attention has no output projection (to_out = nn.Identity(), GoalFormer.py:56,66-69)
  int tiled;      // DGVIT_FLAG_LONG_SEQUENCE and N > 288: the attention runs on the K / V-tiled kernels (attention_long.hip, attention_bf16_long.hip)
  long long T;
};

inline int make_dims(const dgvit_config* c, int batch, Dims& d) {
  DGVIT_CHECK_ARG(c, "null config");
  DGVIT_CHECK_ARG(batch > 0, "batch must be positive");
  DGVIT_CHECK_ARG(c->patch_h > 0 && c->patch_w > 0 && c->image_h > 0 && c->image_w > 0 && c->image_h % c->patch_h == 0 &&
                      c->image_w % c->patch_w == 0,
                  "Image dimensions must be divisible by the patch size.");
  DGVIT_CHECK_ARG(c->dim > 0 && c->dim % 4 == 0 && c->dim <= 1024, "dim=%d must be a multiple of 4 and <= 1024", c->dim);
  DGVIT_CHECK_ARG(c->depth > 0 && c->heads > 0 && c->mlp_dim > 0 && c->mlp_dim % 4 == 0, "bad depth/heads/mlp_dim");
  DGVIT_CHECK_ARG(c->dim_head == 64 || c->dim_head == 32, "dim_head=%d unsupported (64 or 32)", c->dim_head);
  d.B = batch;
  d.P = (c->image_h / c->patch_h) * (c->image_w / c->patch_w);
  d.N = d.P + 1;
  d.D = c->dim; d.H = c->heads; d.dh = c->dim_head; d.I = d.H * d.dh; d.M = c->mlp_dim; d.L = c->depth;
  d.pd = c->patch_h * c->patch_w;
  d.pool_mean = c->pool_mean ? 1 : 0;
  d.proj = !(d.H == 1 && d.dh == d.D);
  d.T = (long long)batch * d.N;
  DGVIT_CHECK_ARG(d.N <= 288 || long_sequence(c),
                  "tokens N=%d exceeds the fused-attention limit (288); set DGVIT_FLAG_LONG_SEQUENCE in dgvit_config.flags "
                  "(GoT.set_schedule(long_sequence=True)) for the K/V-tiled attention", d.N);
  // (N <= 288 keeps the fused kernels with the flag set too: bit-identical results; the small-batch block path (N <= 128) and the
  //  one-query kernel (N <= 64) are never reached by a tiled shape)
  d.tiled = long_sequence(c) && d.N > 288;
  DGVIT_CHECK_ARG(d.T < (1ll << 31) && d.T * (long long)(3 * d.I > d.M ? 3 * d.I : d.M) < (1ll << 40), "batch too large");
  return DGVIT_OK;
}

// The last block's K / V fold (last_block.hip): gemm_layer and backward_layer both ask here, so a forward and its backward
// cannot disagree.  `last` = the block is the pruned (token-0) last one; `maps` = an attention-maps call (always no-grad: the backward
// never sees one).  u and r (du and dr) live behind q (dq) in the frame's own N x 3I region of the qkv (dqkv) buffer, p in the lse slot.
// `wqkv` = the block's to_qkv.weight: the head-batched products read it with 16-byte loads.  `save` = the forward keeps its activations
// for a backward: a no-grad forward keeps the K / V GEMM, so that its features stay bit-identical to those of a maps call
// (dgvit_got_forward_maps, rows = DGVIT_MAPS_GOAL: tests/test_gpu_attention_maps.py), which needs K for its probabilities.
inline bool last_block_fold(const Dims& d, bool last, bool ldrop, bool maps, bool save, const float* wqkv) {
  KNOB_IF(g_last_block_fold) {
    return last && save && !ldrop && !d.tiled && !maps && al16(wqkv) && goal_attention_supports(d.N, d.D, d.H, d.dh) &&
           goal_pool_lds_bytes(d.N, d.D, d.H) <= GOAL_POOL_LDS_BUDGET && d.I + 2ll * d.H * d.D <= 3ll * d.N * d.I;
  }
  return false;
}

enum { P_POS = 0, P_PW = 1, P_PB = 2, P_RMS = 3, P_L0 = 4 };
enum { L_LN1W = 0, L_LN1B, L_QKV, L_OUTW, L_OUTB, L_LN2W, L_LN2B, L_FC1W, L_FC1B, L_FC2W, L_FC2B };
// the to_out slots of the parameter table are unused (may be NULL) when the attention has no output projection
inline bool no_projection_slot(const Dims& d, int i) {
  if (d.proj || i < P_L0) return false;
  const int j = (i - P_L0) % DGVIT_PARAMS_PER_LAYER;
  return j == L_OUTW || j == L_OUTB;
}

// gradient-ready events (dgvit_grad_events): recorded on the caller's stream where a group of parameter gradients is final
inline int check_events(const dgvit_grad_events* ev, int depth) {
  if (!ev) return DGVIT_OK;
  DGVIT_CHECK_ARG(ev->n_layers == depth, "dgvit_grad_events: n_layers %d != depth %d", ev->n_layers, depth);
  DGVIT_CHECK_ARG(ev->layer, "dgvit_grad_events: layer table is null");
  return DGVIT_OK;
}
inline int mark_ready(void* event, hipStream_t st) {
  if (event) HIP_TRY(hipEventRecord((hipEvent_t)event, st));
  return DGVIT_OK;
}

// ---------------------------------------------------------------------------------------------- encoder steps of both schedules
// pool: x[:, 0] (cls slot = goal token) or the token mean into `pooled` (GoalFormer.py:167), then RMSNorm (:170)
inline int pool_rmsnorm_fwd(const Dims& d, const float* x, float* pooled, const float* rms_g, float* feat, hipStream_t st) {
  if (d.pool_mean) {
    TRY(avgpool(x, pooled, d.B, d.N, d.D, st));
    return rmsnorm_fwd(pooled, d.D, rms_g, feat, d.B, d.D, st);
  }
  return rmsnorm_fwd(x, (long long)d.N * d.D, rms_g, feat, d.B, d.D, st);
}

// Head backward: dx (T, D) = the gradient of the last layer's output xl (or of the pooled token mean) through the RMSNorm; every
// token row other than token 0 gets zero gradient.  `dpool` is (B, D) scratch for the gradient of the pooled vector.
inline int head_bwd(const Dims& d, const float* dfeat, const float* xl, const float* pooled, const float* rms_g, float* drms_g, float* dx,
                    float* dpool, float* part, const dgvit_grad_events* events, hipStream_t st) {
  if (d.pool_mean) {
    // feat = RMSNorm(mean_tokens(x)): gradient of the pooled vector, then broadcast / N
    TRY(rmsnorm_bwd(dfeat, pooled, d.D, rms_g, dpool, d.D, drms_g, part, d.B, d.D, st));
    TRY(mean_bwd(dpool, dx, d.B, d.N, d.D, st));
  } else {
    TRY(zero_fill(dx, (long long)sizeof(float) * d.T * d.D, st));
    TRY(rmsnorm_bwd(dfeat, xl, (long long)d.N * d.D, rms_g, dx, (long long)d.N * d.D, drms_g, part, d.B, d.D, st));
  }
  if (events) TRY(mark_ready(events->head, st));
  return DGVIT_OK;
}

// Gradient with respect to the frame: dimg = unpatchify(dpatch W_pe), dpatch (B * P, D) the packed patch rows of the token-assembly
// gradient.  ONE NN GEMM whose epilogue stores straight into the (B, H, W) image (EPI_UNPATCH, the inverse of the forward's patch
// gather): no (B * P, pd) buffer, no permutation pass.  Not split (no counters): the launch is thousands of tiles at training batches,
// and a split would need scratch the size queries do not have.
inline int image_grad(const dgvit_config* c, const Dims& d, const float* dpatch, const float* wpe, float* dimg, hipStream_t st) {
  GemmParams p = gp(dpatch, d.D, wpe, d.pd, dimg, d.pd, d.B * d.P, d.pd, d.D);
  p.g_wi = c->image_w; p.g_hw = c->image_h * c->image_w; p.g_ph = c->patch_h; p.g_pw = c->patch_w;
  p.g_gw = c->image_w / c->patch_w; p.g_P = d.P;
  return gemm_f32(GEMM_NN, EPI_UNPATCH, p, 1, st);
}

// Token-assembly backward, x0 = dropout(cat(goal, patches W^T + b) + pos), in fp32: dx (T, D) = d x0 on entry (the emb-dropout is
// applied in place), then dgoal, dpos and -- when wanted -- the patch-embedding gradients and dimg.  `dpatch` is (B * P, D) scratch
// for the packed patch rows.  The patch-weight gradient reads the fp32 patch rows `patches`, or with `img` set, `img32` after this
// step has patchified the frame into it (the bf16 schedule keeps bf16 patches only).
inline int token_assembly_bwd(const dgvit_config* c, const Dims& d, const float* const* params, float* const* grads, float* dx, float* dgoal,
                              float* dimg, float* dpatch, const float* patches, const float* img, float* img32, float* part, float* slabs,
                              long long slab_floats, float keep, unsigned long long seed, const unsigned long long* seed_dev, hipStream_t st) {
  if (keep < 1.f) TRY(dropout_inplace(dx, d.T * d.D, seed, seed_dev, keep, st));
  if (dgoal)
    HIP_TRY(hipMemcpy2DAsync(dgoal, sizeof(float) * d.D, dx, sizeof(float) * d.N * d.D, sizeof(float) * d.D, d.B,
                             hipMemcpyDeviceToDevice, st));
  if (grads[P_POS]) TRY(colsum(dx, (long long)d.N * d.D, grads[P_POS], part, d.B, d.N * d.D, 0, st));  // dpos = sum over frames
  const bool patch_grads = grads[P_PW] || grads[P_PB];
  if (!patch_grads && !dimg) return DGVIT_OK;
  // patch rows of dx0 (token rows 1..P of every frame) packed densely, then dW_pe = dx_patch^T patches, db_pe = column sums
  HIP_TRY(hipMemcpy2DAsync(dpatch, sizeof(float) * d.P * d.D, dx + d.D, sizeof(float) * d.N * d.D, sizeof(float) * d.P * d.D, d.B,
                           hipMemcpyDeviceToDevice, st));
  if (patch_grads) {
    if (img) {
      TRY(patchify(img, img32, d.B, c->image_h, c->image_w, c->patch_h, c->patch_w, st));
      patches = img32;
    }
    TRY(wgrad(dpatch, d.D, patches, d.pd, grads[P_PW], grads[P_PB], d.D, d.pd, d.B * d.P, slabs, slab_floats, st));
  }
  if (dimg) TRY(image_grad(c, d, dpatch, params[P_PW], dimg, st));   // (whether or not W_pe / b_pe are frozen)
  return DGVIT_OK;
}
