// The bf16 encoder (BASELINE config 5): weight packing, dgvit_got_forward_bf16, every dgvit_got_backward_bf16* entry point and the
// operator-level exports of the bf16 kernels.
#include "bf16.h"
#include "schedule.h"

// ---------------------------------------------------------------------------------------------- bf16 configuration
// BASELINE config 5 (224x224, ViT-Base variant, bf16): bf16 storage for GEMM operands (LayerNorm output, qkv,
// attention output, MLP hidden, branch outputs, weights, and in backward their gradients), fp32 residual stream and its
// gradient / LayerNorm statistics / biases / softmax / parameter gradients, fp32 accumulation on
// v_mfma_f32_32x32x16_bf16.  Same schedule as dgvit_got_forward / dgvit_got_backward (GoalFormer.py:156-171).

namespace {

inline long long al128(long long bytes) { return (bytes + 255) & ~255ll; }
inline int up8(long long n) { return (int)((n + 7) & ~7ll); }

// The patch GEMM needs K and both row strides % 8 == 0 (gemm_bf16): patch rows and patch-weight rows have ldp = up8(pd) elements with a
// zero tail.  ldp == pd for every patch area that is a multiple of 8: nothing differs from the unpadded layout there.
inline int patch_ld(const Dims& d) { return up8(d.pd); }

// bf16 weight arena (elements): patch weight (D rows of ldp), then per layer to_qkv, to_out, fc1, fc2 in the reference's (out, in)
// layouts, followed by their transposes (in, out) -- the B operands of the data-gradient GEMMs dX = dY W
struct Wp {
  long long patch, layer0, qkv, out, fc1, fc2, qkvT, outT, fc1T, fc2T, layer_elems, total;
};
Wp make_wp(const Dims& d) {
  Wp w;
  long long o = 0;
  w.patch = o; o += al4((long long)d.D * patch_ld(d));
  long long l = 0;
  w.qkv = l; l += (long long)3 * d.I * d.D;
  w.out = l; l += (long long)d.D * d.I;
  w.fc1 = l; l += (long long)d.M * d.D;
  w.fc2 = l; l += (long long)d.D * d.M;
  w.qkvT = l; l += (long long)3 * d.I * d.D;
  w.outT = l; l += (long long)d.D * d.I;
  w.fc1T = l; l += (long long)d.M * d.D;
  w.fc2T = l; l += (long long)d.D * d.M;
  w.layer0 = o; w.layer_elems = al4(l);
  o += w.layer_elems * d.L;
  w.total = o;
  return w;
}

// activation workspace in BYTES.  save: every layer keeps what backward needs; else the layers share one block.
struct Wsb {
  long long patches, xa, xb, pooled, delta, layer0, layer_stride, total;
  long long ln, qkv, ao, lse, xmid, ln2, h1, a1, xout, mean1, rstd1, mean2, rstd2, layer_bytes;   // relative to the layer base
};
Wsb make_wsb(const Dims& d, int save) {
  Wsb w;
  long long o = 0;
  w.patches = o; o += al128((long long)d.B * d.P * patch_ld(d) * 2);
  w.xa = o; o += al128(d.T * d.D * 4);
  w.xb = o; o += al128(d.T * d.D * 4);
  w.pooled = o; o += al128((long long)d.B * d.D * 4);
  w.delta = o; o += al128(d.T * d.D * 2);   // bf16 branch output (attention / feed-forward) before it joins the fp32 residual stream
  long long l = 0;
  w.ln = l; l += al128(d.T * d.D * 2);
  w.qkv = l; l += al128(d.T * 3 * d.I * 2);
  w.ao = l; l += al128(d.T * d.I * 2);
  w.lse = l; l += al128((long long)d.B * d.H * d.N * 4);
  w.xmid = l; l += al128(d.T * d.D * 4);
  w.a1 = l; l += al128(d.T * d.M * 2);
  w.ln2 = w.ln; w.h1 = w.xout = w.mean1 = w.rstd1 = w.mean2 = w.rstd2 = -1;
  if (save) {
    w.ln2 = l; l += al128(d.T * d.D * 2);
    w.h1 = l; l += al128(d.T * d.M * 2);      // pre-GELU hidden (GELU' in backward)
    w.xout = l; l += al128(d.T * d.D * 4);    // the layer's output = the next layer's residual input
    w.mean1 = l; l += al128(d.T * 4);
    w.rstd1 = l; l += al128(d.T * 4);
    w.mean2 = l; l += al128(d.T * 4);
    w.rstd2 = l; l += al128(d.T * 4);
  }
  w.layer0 = o; w.layer_bytes = l;
  w.layer_stride = save ? l : 0;
  o += save ? l * d.L : l;
  w.total = o;
  return w;
}

int check_bf16_dims(const Dims& d) {
  DGVIT_CHECK_ARG(d.dh == 64, "bf16 path: dim_head=%d unsupported (64)", d.dh);
  DGVIT_CHECK_ARG(d.proj, "bf16 path: heads == 1 with dim_head == dim (attention without output projection) runs on the fp32 path only");
  DGVIT_CHECK_ARG(d.D % 8 == 0 && d.M % 8 == 0, "bf16 path: dim and mlp_dim must be multiples of 8");
  return DGVIT_OK;
}

GemmBf16Params gpb(const bf16_t* A, int lda, const bf16_t* B, int ldb, void* C, int ldc, int M, int N, int K) {
  GemmBf16Params p = {};
  p.A = A; p.lda = lda; p.B = B; p.ldb = ldb; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K;
  return p;
}

// split-K plan of a weight gradient dW (Mo x Ko) = sum over Tp token columns: about one virtual tile per CU
struct SplitPlan { int splits, kchunk; long long slab; };
SplitPlan wgrad_bf16_plan(int Mo, int Ko, int Tp) {
  const long long tiles = (long long)((Mo + 255) / 256) * ((Ko + 255) / 256);
  long long s = 256 / tiles;
  if (s < 1) s = 1;
  const long long maxs = ((long long)Tp + 511) / 512;   // at least 16 k-tiles per slice (64-bit: Tp + 511 wraps for Tp near 2^31)
  if (s > maxs) s = maxs;
  SplitPlan pl;
  pl.kchunk = (int)((((Tp + s - 1) / s) + 31) / 32 * 32);
  pl.splits = (int)(((long long)Tp + pl.kchunk - 1) / pl.kchunk);
  pl.slab = al4((long long)Mo * Ko);
  return pl;
}
long long wgrad_bf16_scratch(int Mo, int Ko, int Tp) {
  const SplitPlan pl = wgrad_bf16_plan(Mo, Ko, Tp);
  return pl.splits > 1 ? pl.splits * pl.slab : 0;
}
// dW (Mo x Ko, fp32) = dY^T X straight from the token-major bf16 activations dY (T x Mo, row stride ldy), X (T x Ko, ldx):
// the TN layout of the ring GEMM (transposed LDS reads), split over tokens
int wgrad_bf16_tn(const bf16_t* dY, int ldy, const bf16_t* X, int ldx, float* dW, int Mo, int Ko, int T, float* slabs, long long slab_floats,
                  hipStream_t st) {
  const SplitPlan pl = wgrad_bf16_plan(Mo, Ko, T);
  GemmBf16Params p = gpb(dY, ldy, X, ldx, dW, Ko, Mo, Ko, T);
  p.tn = 1;
  if (pl.splits == 1) return gemm_bf16(BEPI_F32_PLAIN, p, st);
  if (slab_floats < pl.splits * pl.slab)
    return dgvit_set_error(DGVIT_ERR_WORKSPACE, "wgrad_bf16: slabs %lld < %lld floats", slab_floats, pl.splits * pl.slab);
  p.C = slabs;
  p.ksplit = pl.splits; p.kchunk = pl.kchunk; p.slab_stride = pl.slab;
  TRY(gemm_bf16(BEPI_F32_PLAIN, p, st));
  return reduce_slabs(slabs, dW, (long long)Mo * Ko, pl.splits, pl.slab, st);
}

// backward scratch in BYTES
struct Bsb {
  long long dxa, dxb, dxh, dln, dqkv, dao, dh1, slabs, part, delta, patches32, total;
  long long slab_floats;
};
Bsb make_bsb(const Dims& d) {
  Bsb s;
  long long o = 0;
  s.dxa = o; o += al128(d.T * d.D * 4);
  s.dxb = o; o += al128(d.T * d.D * 4);
  s.dxh = o; o += al128(d.T * d.D * 2);
  s.dln = o; o += al128(d.T * d.D * 2);
  s.dqkv = o; o += al128(d.T * 3 * d.I * 2);
  s.dao = o; o += al128(d.T * d.I * 2);
  s.dh1 = o; o += al128(d.T * d.M * 2);
  const long long widest = std::max<long long>(std::max(3 * d.I, d.M), d.D);
  const int Ti = (int)d.T;
  long long sl = wgrad_bf16_scratch(3 * d.I, d.D, Ti);
  sl = std::max(sl, wgrad_bf16_scratch(d.D, d.I, Ti));
  sl = std::max(sl, wgrad_bf16_scratch(d.M, d.D, Ti));
  sl = std::max(sl, wgrad_bf16_scratch(d.D, d.M, Ti));
  sl = std::max(sl, wgrad_scratch(d.D, d.pd, d.B * d.P));   // fp32 patch-embedding weight gradient
  s.slab_floats = sl;
  s.slabs = o; o += al128(sl * 4);
  long long part = (long long)layernorm_bwd_blocks((int)d.T) * 2 * d.D;
  part = std::max(part, (long long)colsum_blocks(d.B) * d.N * d.D);
  part = std::max(part, (long long)rmsnorm_bwd_blocks(d.B) * d.D);
  part = std::max(part, (long long)colsum_bf16_blocks((int)d.T) * widest);   // bias-gradient partials
  s.part = o; o += al128(part * 4);
  s.delta = o; o += al128((long long)d.B * d.H * d.N * 4);   // rowsum(dO o O) of the attention backward
  s.patches32 = o; o += al128((long long)d.B * d.P * d.pd * 4);
  s.total = o;
  return s;
}

}  // namespace

extern "C" long long dgvit_got_bf16_weight_elems(const dgvit_config* cfg) {
  Dims d;
  if (make_dims(cfg, 1, d) || check_bf16_dims(d)) return -1;
  return make_wp(d).total;
}

extern "C" long long dgvit_got_bf16_workspace_bytes(const dgvit_config* cfg, int batch, int save) {
  Dims d;
  if (make_dims(cfg, batch, d) || check_bf16_dims(d)) return -1;
  return make_wsb(d, save).total;
}

extern "C" long long dgvit_got_bf16_backward_scratch_bytes(const dgvit_config* cfg, int batch) {
  Dims d;
  if (make_dims(cfg, batch, d) || check_bf16_dims(d)) return -1;
  return make_bsb(d).total;
}

extern "C" int dgvit_got_pack_weights_bf16(const dgvit_config* cfg, const float* const* params, unsigned short* wpack,
                                           long long wpack_elems, int with_transposes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  Dims d;
  TRY(make_dims(cfg, 1, d));
  TRY(check_bf16_dims(d));
  DGVIT_CHECK_ARG(params && wpack, "dgvit_got_pack_weights_bf16: null pointer");
  const Wp w = make_wp(d);
  if (wpack_elems < w.total) return dgvit_set_error(DGVIT_ERR_WORKSPACE, "bf16 weight arena %lld < %lld elements", wpack_elems, w.total);
  CastBatch cb;     // the straight copies of all layers go out as one launch (49 segments at depth 12)
  cast_batch_init(cb);
  const int ldp = patch_ld(d);
  if (ldp == d.pd) TRY(cast_batch_add(cb, params[P_PW], wpack + w.patch, (long long)d.D * d.pd, st));
  else TRY(cast_f32_bf16_rows(params[P_PW], wpack + w.patch, d.D, d.pd, ldp, st));   // rows padded to ldp, tail zeroed
  for (int i = 0; i < d.L; ++i) {
    const float* const* lp = params + P_L0 + DGVIT_PARAMS_PER_LAYER * i;
    bf16_t* lw = wpack + w.layer0 + w.layer_elems * i;
    TRY(cast_batch_add(cb, lp[L_QKV], lw + w.qkv, (long long)3 * d.I * d.D, st));
    TRY(cast_batch_add(cb, lp[L_OUTW], lw + w.out, (long long)d.D * d.I, st));
    TRY(cast_batch_add(cb, lp[L_FC1W], lw + w.fc1, (long long)d.M * d.D, st));
    TRY(cast_batch_add(cb, lp[L_FC2W], lw + w.fc2, (long long)d.D * d.M, st));
  }
  TRY(cast_batch_flush(cb, st));
  for (int i = 0; i < d.L; ++i) {
    const float* const* lp = params + P_L0 + DGVIT_PARAMS_PER_LAYER * i;
    bf16_t* lw = wpack + w.layer0 + w.layer_elems * i;
    if (!with_transposes) continue;
    TRY(transpose_cast_f32_bf16(lp[L_QKV], lw + w.qkvT, 3 * d.I, d.D, st));   // (3I, D) -> (D, 3I)
    TRY(transpose_cast_f32_bf16(lp[L_OUTW], lw + w.outT, d.D, d.I, st));      // (D, I)  -> (I, D)
    TRY(transpose_cast_f32_bf16(lp[L_FC1W], lw + w.fc1T, d.M, d.D, st));      // (M, D)  -> (D, M)
    TRY(transpose_cast_f32_bf16(lp[L_FC2W], lw + w.fc2T, d.D, d.M, st));      // (D, M)  -> (M, D)
  }
  return DGVIT_OK;
}

// ---------------------------------------------------------------------------------------------- forward
namespace {

// one bf16 forward call: what its steps share
struct FwdB {
  const dgvit_config* cfg;
  Dims d;
  Wsb w;
  Wp wp;
  const float* const* params;
  const bf16_t* wpack;
  unsigned char* ws;
  int save;
  hipStream_t st;
  float* maps = nullptr;   // attention maps (dgvit_got_forward_maps_bf16); null in every other call
  int maps_rows = DGVIT_MAPS_GOAL;
  // transformer-internal dropout (the mask table of common.h): lkeep < 1 applies the four sites of every block
  float lkeep = 1.f;
  unsigned long long seed = 0;
  const unsigned long long* seed_dev = nullptr;
  bool ldrop() const { return lkeep < 1.f; }
  LayerDrop site(int layer, int s) const { return LayerDrop{lkeep, drop_tag(layer, s), seed, seed_dev}; }
  float* f32(unsigned char* base, long long off) const { return save ? (float*)(base + off) : (float*)nullptr; }
};

// token assembly into x: patch embedding, goal token, positional embedding, dropout (GoalFormer.py:137-139,157,160-163)
int token_assembly_bf16(const FwdB& f, const float* img, const float* goal, float keep, unsigned long long seed,
                        const unsigned long long* seed_dev, float* x) {
  const Dims& d = f.d;
  const dgvit_config* cfg = f.cfg;
  hipStream_t st = f.st;
  bf16_t* patches = (bf16_t*)(f.ws + f.w.patches);
  const int ldp = patch_ld(d);
  TRY(patchify_bf16(img, patches, ldp, d.B, cfg->image_h, cfg->image_w, cfg->patch_h, cfg->patch_w, st));
  {
    GemmBf16Params p = gpb(patches, ldp, f.wpack + f.wp.patch, ldp, x, d.D, d.B * d.P, d.D, ldp);
    p.bias = f.params[P_PB];
    p.res = f.params[P_POS]; p.ldr = d.D; p.res_mod = d.P;
    p.c_rgrp = d.P;
    TRY(gemm_bf16(BEPI_F32, p, st));
  }
  TRY(goal_row(goal, f.params[P_POS], x, d.B, d.N, d.D, st));
  if (keep < 1.f) TRY(dropout_inplace(x, d.T * d.D, seed, seed_dev, keep, st));
  return DGVIT_OK;
}

// One block; x advances to its output.  The branch outputs (to_out, fc2: GoalFormer.py:82,49) are stored bf16 like every other GEMM
// output and join the fp32 residual stream inside the LayerNorm kernel of the next sub-block (x = attn(..) + x; x = ff(..) + x,
// :103-104): the GEMM epilogues then have no fp32 residual read on their critical path.  Block 0 normalises its input here; every
// later block gets its LN1 from the previous block's residual add.
int layer_fwd_bf16(const FwdB& f, int i, float*& x) {
  const Dims& d = f.d;
  const Wsb& w = f.w;
  const Wp& wp = f.wp;
  unsigned char* ws = f.ws;
  const int save = f.save;
  hipStream_t st = f.st;
  const int T = (int)d.T;
  const float* const* lp = f.params + P_L0 + DGVIT_PARAMS_PER_LAYER * i;
  const bf16_t* lw = f.wpack + wp.layer0 + wp.layer_elems * i;
  unsigned char* lb = ws + w.layer0 + w.layer_stride * i;
  bf16_t* ln = (bf16_t*)(lb + w.ln);
  bf16_t* ln2 = (bf16_t*)(lb + w.ln2);
  bf16_t* qkv = (bf16_t*)(lb + w.qkv);
  bf16_t* ao = (bf16_t*)(lb + w.ao);
  float* xmid = (float*)(lb + w.xmid);
  bf16_t* a1 = (bf16_t*)(lb + w.a1);
  bf16_t* delta = (bf16_t*)(ws + w.delta);
  if (i == 0) TRY(layernorm_fwd_bf16(x, lp[L_LN1W], lp[L_LN1B], ln, f.f32(lb, w.mean1), f.f32(lb, w.rstd1), T, d.D, 1e-5f, 1, st));
  // inference: the last block only needs token 0 downstream of K/V (see gemm_layer in encoder.hip); training keeps it dense
  const bool dense = dense_last_block(f.cfg) || (f.maps && f.maps_rows == DGVIT_MAPS_ALL);   // (maps of every row: see encoder.hip)
  const bool last = !dense && !save && !d.pool_mean && i == d.L - 1;
  const int tok = last ? d.B : T, rs = last ? d.N : 1;
  float* xo = save ? (float*)(lb + w.xout) : (x == (float*)(ws + w.xa) ? (float*)(ws + w.xb) : (float*)(ws + w.xa));
  if (!last) {
    GemmBf16Params p = gpb(ln, d.D, lw + wp.qkv, d.D, qkv, 3 * d.I, T, 3 * d.I, d.D);
    TRY(gemm_bf16(BEPI_BF16, p, st));
  } else {
    GemmBf16Params kv = gpb(ln, d.D, lw + wp.qkv + (long long)d.I * d.D, d.D, qkv + d.I, 3 * d.I, T, 2 * d.I, d.D);
    TRY(gemm_bf16(BEPI_BF16, kv, st));
    GemmBf16Params q = gpb(ln, rs * d.D, lw + wp.qkv, d.D, qkv, rs * 3 * d.I, tok, d.I, d.D);
    TRY(gemm_bf16(BEPI_BF16, q, st));
  }
  float* lse = f.maps ? (float*)(lb + w.lse) : f.f32(lb, w.lse);   // (the no-grad layout has the slot too)
  // with dropout every attention call takes the K / V-tiled kernels (any N): they carry the mask, the fused ones do not
  if (f.ldrop()) TRY(attention_fwd_bf16_tiled_drop(qkv, ao, lse, d.B, d.N, d.H, d.dh, last ? 1 : d.N, f.site(i, DROP_ATTN), st));
  else if (d.tiled) TRY(attention_fwd_bf16_tiled(qkv, ao, lse, d.B, d.N, d.H, d.dh, last ? 1 : d.N, st));
  else TRY(attention_fwd_bf16(qkv, ao, lse, d.B, d.N, d.H, d.dh, last ? 1 : d.N, st));
  if (f.maps) {   // before the shared qkv / lse are overwritten by the next layer
    const long long per_head = f.maps_rows == DGVIT_MAPS_ALL ? (long long)d.N * d.N : d.N;
    TRY(attention_probs_bf16(qkv, lse, f.maps + (long long)i * d.H * per_head, (long long)d.L * d.H * per_head, d.B, d.N, d.H, d.dh,
                             f.maps_rows, st));
  }
  {
    GemmBf16Params p = gpb(ao, rs * d.I, lw + wp.out, d.I, delta, rs * d.D, tok, d.D, d.I);
    p.bias = lp[L_OUTB];
    TRY(gemm_bf16(BEPI_BF16, p, st));
  }
  if (f.ldrop()) TRY(drop_rows_bf16(delta, (long long)rs * d.D, delta, (long long)rs * d.D, tok, d.D, rs, f.site(i, DROP_OUT), st));
  // xmid = x + to_out(..);  ln2 = LN2(xmid).  No-grad passes do not store xmid in the blocks that have a successor: the feed-forward
  // output goes to the (free again) attention-output buffer and both branch outputs join the stream in ONE pass below,
  // (x + d_attn) + d_ff in the order of the two-step schedule: identical results, 22 instead of 24 bytes per element and block
  const bool joint = !save && i + 1 < d.L && d.I >= d.D;     // (the attention-output buffer holds T x I elements)
  if (joint)
    TRY(add2_layernorm_fwd_bf16(x, delta, nullptr, nullptr, lp[L_LN2W], lp[L_LN2B], ln2, T, d.D, 1e-5f, st));
  else
    TRY(add_layernorm_fwd_bf16(x, delta, xmid, lp[L_LN2W], lp[L_LN2B], ln2, f.f32(lb, w.mean2), f.f32(lb, w.rstd2), tok, d.D, 1e-5f, rs, st));
  {
    GemmBf16Params p = gpb(ln2, rs * d.D, lw + wp.fc1, d.D, a1, d.M, tok, d.M, d.D);
    p.bias = lp[L_FC1B];
    if (save) {
      p.C2 = (bf16_t*)(lb + w.h1); p.ldc2 = d.M;
      TRY(gemm_bf16(BEPI_GELU2_BF16, p, st));
    } else {
      TRY(gemm_bf16(BEPI_GELU_BF16, p, st));
    }
  }
  if (f.ldrop()) TRY(drop_rows_bf16(a1, d.M, a1, d.M, tok, d.M, rs, f.site(i, DROP_HIDDEN), st));   // (the pre-activation h1 stays as it is)
  {
    bf16_t* ff = joint ? ao : delta;
    GemmBf16Params p = gpb(a1, d.M, lw + wp.fc2, d.M, ff, rs * d.D, tok, d.D, d.M);
    p.bias = lp[L_FC2B];
    TRY(gemm_bf16(BEPI_BF16, p, st));
    if (f.ldrop()) TRY(drop_rows_bf16(ff, (long long)rs * d.D, ff, (long long)rs * d.D, tok, d.D, rs, f.site(i, DROP_FF), st));
  }
  // xo = xmid + ff(..), and the next block's LN1 of it
  if (joint) {
    unsigned char* nb = ws + w.layer0 + w.layer_stride * (i + 1);
    TRY(add2_layernorm_fwd_bf16(x, delta, ao, xo, lp[DGVIT_PARAMS_PER_LAYER + L_LN1W], lp[DGVIT_PARAMS_PER_LAYER + L_LN1B],
                                (bf16_t*)(nb + w.ln), T, d.D, 1e-5f, st));
  } else if (i + 1 < d.L) {
    unsigned char* nb = ws + w.layer0 + w.layer_stride * (i + 1);
    TRY(add_layernorm_fwd_bf16(xmid, delta, xo, lp[DGVIT_PARAMS_PER_LAYER + L_LN1W], lp[DGVIT_PARAMS_PER_LAYER + L_LN1B],
                               (bf16_t*)(nb + w.ln), f.f32(nb, w.mean1), f.f32(nb, w.rstd1), T, d.D, 1e-5f, 1, st));
  } else {
    TRY(residual_add_bf16(xmid, delta, xo, tok, d.D, rs, st));
  }
  x = xo;
  return DGVIT_OK;
}

}  // namespace

namespace {
int got_forward_bf16(FwdB& f, const float* img, const float* goal, float* feat, const void* workspace, long long ws_bytes, int batch, float keep,
                     unsigned long long seed, const unsigned long long* seed_dev) {
  const dgvit_config* cfg = f.cfg;
  const float* const* params = f.params;
  const unsigned short* wpack = f.wpack;
  const int save = f.save;
  const Dims& d = f.d;
  TRY(make_dims(cfg, batch, f.d));
  TRY(check_bf16_dims(d));
  DGVIT_CHECK_ARG(params && wpack && img && goal && feat && workspace, "dgvit_got_forward_bf16: null pointer");
  DGVIT_CHECK_ARG(keep > 0.f && keep <= 1.f, "dropout_keep must be in (0, 1]");
  DGVIT_CHECK_ARG(f.lkeep > 0.f && f.lkeep <= 1.f, "layer_keep=%g must be in (0, 1]", (double)f.lkeep);
  f.seed = seed; f.seed_dev = seed_dev;
  f.w = make_wsb(d, save);
  f.wp = make_wp(d);
  if (ws_bytes < f.w.total) return dgvit_set_error(DGVIT_ERR_WORKSPACE, "bf16 forward workspace %lld < %lld bytes", ws_bytes, f.w.total);
  DGVIT_CHECK_ARG((uintptr_t)workspace % 256 == 0 && (uintptr_t)wpack % 16 == 0, "bf16 path: workspace must be 256-byte aligned");
  for (int i = 0; i < P_L0 + DGVIT_PARAMS_PER_LAYER * d.L; ++i) DGVIT_CHECK_ARG(params[i], "parameter %d is null", i);
  float* x = (float*)(f.ws + f.w.xa);
  TRY(token_assembly_bf16(f, img, goal, keep, seed, seed_dev, x));
  for (int i = 0; i < d.L; ++i) TRY(layer_fwd_bf16(f, i, x));
  return pool_rmsnorm_fwd(d, x, (float*)(f.ws + f.w.pooled), params[P_RMS], feat, f.st);
}
}  // namespace

extern "C" int dgvit_got_forward_bf16_v2(const dgvit_config* cfg, const float* const* params, const unsigned short* wpack,
                                         const float* img, const float* goal, float* feat, void* workspace, long long ws_bytes,
                                         int batch, int save, float keep, float layer_keep, unsigned long long seed,
                                         const unsigned long long* seed_dev, void* stream) {
  FwdB f = {cfg, {}, {}, {}, params, wpack, (unsigned char*)workspace, save, (hipStream_t)stream};
  f.lkeep = layer_keep;
  return got_forward_bf16(f, img, goal, feat, workspace, ws_bytes, batch, keep, seed, seed_dev);
}

extern "C" int dgvit_got_forward_bf16(const dgvit_config* cfg, const float* const* params, const unsigned short* wpack,
                                      const float* img, const float* goal, float* feat, void* workspace, long long ws_bytes,
                                      int batch, int save, float keep, unsigned long long seed,
                                      const unsigned long long* seed_dev, void* stream) {
  return dgvit_got_forward_bf16_v2(cfg, params, wpack, img, goal, feat, workspace, ws_bytes, batch, save, keep, 1.f, seed, seed_dev, stream);
}

// the no-grad bf16 forward with each layer's attention probabilities (include/dgvit_hip.h: Attention maps)
extern "C" int dgvit_got_forward_maps_bf16(const dgvit_config* cfg, const float* const* params, const unsigned short* wpack, const float* img,
                                           const float* goal, float* feat, float* maps, int rows, void* workspace, long long ws_bytes, int batch,
                                           float keep, unsigned long long seed, const unsigned long long* seed_dev, void* stream) {
  return dgvit_got_forward_maps_bf16_v2(cfg, params, wpack, img, goal, feat, maps, rows, workspace, ws_bytes, batch, keep, 1.f, seed, seed_dev,
                                        stream);
}

// ... with the transformer-internal dropout: the maps are read from q, k and the undropped lse, so they are the probabilities before the mask
extern "C" int dgvit_got_forward_maps_bf16_v2(const dgvit_config* cfg, const float* const* params, const unsigned short* wpack, const float* img,
                                              const float* goal, float* feat, float* maps, int rows, void* workspace, long long ws_bytes,
                                              int batch, float keep, float layer_keep, unsigned long long seed,
                                              const unsigned long long* seed_dev, void* stream) {
  Dims d;
  TRY(make_dims(cfg, batch, d));
  TRY(check_bf16_dims(d));
  DGVIT_CHECK_ARG(maps, "dgvit_got_forward_maps_bf16: null maps pointer");
  DGVIT_CHECK_ARG(rows == DGVIT_MAPS_GOAL || rows == DGVIT_MAPS_ALL, "dgvit_got_forward_maps_bf16: rows=%d must be DGVIT_MAPS_GOAL (0) or DGVIT_MAPS_ALL (1)", rows);
  FwdB f = {cfg, {}, {}, {}, params, wpack, (unsigned char*)workspace, 0, (hipStream_t)stream};
  f.maps = maps;
  f.maps_rows = rows;
  f.lkeep = layer_keep;
  return got_forward_bf16(f, img, goal, feat, workspace, ws_bytes, batch, keep, seed, seed_dev);
}

// Gradient of dgvit_got_forward_bf16 (save_for_backward = 1).  Data-gradient GEMMs take the transposed weight copies of
// the arena as B operand; weight-gradient GEMMs contract over tokens, so both operands are first transposed to
// token-contiguous bf16 copies (zero padded to a multiple of 8 tokens) and the product is split over tokens into fp32
// slabs that a fixed-order reduction sums (deterministic).  Bias gradients are the row sums of the transposed dY.
extern "C" int dgvit_got_backward_bf16(const dgvit_config* cfg, const float* const* params, const unsigned short* wpack,
                                       float* const* grads, const float* dfeat, float* dgoal, const float* img,
                                       const void* workspace, long long ws_bytes, void* scratch, long long scratch_bytes, int batch,
                                       float keep, unsigned long long seed, const unsigned long long* seed_dev, void* stream) {
  return dgvit_got_backward_bf16_v2_ev(cfg, params, wpack, grads, dfeat, dgoal, nullptr, img, workspace, ws_bytes, scratch, scratch_bytes, batch,
                                       keep, seed, seed_dev, stream, nullptr);
}

extern "C" int dgvit_got_backward_bf16_ev(const dgvit_config* cfg, const float* const* params, const unsigned short* wpack,
                                          float* const* grads, const float* dfeat, float* dgoal, const float* img,
                                          const void* workspace, long long ws_bytes, void* scratch, long long scratch_bytes, int batch,
                                          float keep, unsigned long long seed, const unsigned long long* seed_dev, void* stream,
                                          const dgvit_grad_events* events) {
  return dgvit_got_backward_bf16_v2_ev(cfg, params, wpack, grads, dfeat, dgoal, nullptr, img, workspace, ws_bytes, scratch, scratch_bytes, batch,
                                       keep, seed, seed_dev, stream, events);
}

extern "C" int dgvit_got_backward_bf16_v2(const dgvit_config* cfg, const float* const* params, const unsigned short* wpack,
                                          float* const* grads, const float* dfeat, float* dgoal, float* dimg, const float* img,
                                          const void* workspace, long long ws_bytes, void* scratch, long long scratch_bytes, int batch,
                                          float keep, unsigned long long seed, const unsigned long long* seed_dev, void* stream) {
  return dgvit_got_backward_bf16_v2_ev(cfg, params, wpack, grads, dfeat, dgoal, dimg, img, workspace, ws_bytes, scratch, scratch_bytes, batch,
                                       keep, seed, seed_dev, stream, nullptr);
}

extern "C" int dgvit_got_backward_bf16_v2_ev(const dgvit_config* cfg, const float* const* params, const unsigned short* wpack,
                                             float* const* grads, const float* dfeat, float* dgoal, float* dimg, const float* img,
                                             const void* workspace, long long ws_bytes, void* scratch, long long scratch_bytes, int batch,
                                             float keep, unsigned long long seed, const unsigned long long* seed_dev, void* stream,
                                             const dgvit_grad_events* events) {
  return dgvit_got_backward_bf16_v3_ev(cfg, params, wpack, grads, dfeat, dgoal, dimg, img, workspace, ws_bytes, scratch, scratch_bytes, batch,
                                       keep, 1.f, seed, seed_dev, stream, events);
}

extern "C" int dgvit_got_backward_bf16_v3(const dgvit_config* cfg, const float* const* params, const unsigned short* wpack,
                                          float* const* grads, const float* dfeat, float* dgoal, float* dimg, const float* img,
                                          const void* workspace, long long ws_bytes, void* scratch, long long scratch_bytes, int batch,
                                          float keep, float layer_keep, unsigned long long seed, const unsigned long long* seed_dev,
                                          void* stream) {
  return dgvit_got_backward_bf16_v3_ev(cfg, params, wpack, grads, dfeat, dgoal, dimg, img, workspace, ws_bytes, scratch, scratch_bytes, batch,
                                       keep, layer_keep, seed, seed_dev, stream, nullptr);
}

// ---------------------------------------------------------------------------------------------- backward
namespace {

// one bf16 backward call: what its steps share
struct BwdB {
  Dims d;
  Wsb w;
  Wp wp;
  Bsb s;
  const float* const* params;
  const bf16_t* wpack;
  float* const* grads;
  const unsigned char* ws;
  unsigned char* sc;
  hipStream_t st;
  const dgvit_grad_events* events;
  // transformer-internal dropout: the forward's keep and seed (nothing is stored: every mask is regenerated)
  float lkeep;
  unsigned long long seed;
  const unsigned long long* seed_dev;
  bool ldrop() const { return lkeep < 1.f; }
  LayerDrop site(int layer, int s) const { return LayerDrop{lkeep, drop_tag(layer, s), seed, seed_dev}; }
  // dW (no x ni) and optionally db (no) from dY (T x no, row stride ldy) and X (T x ni, row stride ldx)
  int wgrad(const bf16_t* dY, int ldy, const bf16_t* X, int ldx, float* dW, float* db, int no, int ni) const {
    if (db) TRY(colsum_bf16(dY, ldy, db, (float*)(sc + s.part), (int)d.T, no, st));
    if (!dW) return DGVIT_OK;
    return wgrad_bf16_tn(dY, ldy, X, ldx, dW, no, ni, (int)d.T, (float*)(sc + s.slabs), s.slab_floats, st);
  }
};

// Gradient of one block: dx / dxh (the gradient of the block's output, fp32 and its bf16 copy) become the gradient of its input
int layer_bwd_bf16(const BwdB& b, int i) {
  const Dims& d = b.d;
  const Wsb& w = b.w;
  const Wp& wp = b.wp;
  const Bsb& s = b.s;
  const unsigned char* ws = b.ws;
  unsigned char* sc = b.sc;
  hipStream_t st = b.st;
  const int T = (int)d.T;
  float* dx = (float*)(sc + s.dxa);      // gradient of the residual stream entering the current op (fp32)
  float* dx2 = (float*)(sc + s.dxb);
  bf16_t* dxh = (bf16_t*)(sc + s.dxh);   // its bf16 copy: A operand of the data-gradient GEMMs, source of the transposed dY
  bf16_t* dln = (bf16_t*)(sc + s.dln);
  bf16_t* dqkv = (bf16_t*)(sc + s.dqkv);
  bf16_t* dao = (bf16_t*)(sc + s.dao);
  bf16_t* dh1 = (bf16_t*)(sc + s.dh1);
  float* part = (float*)(sc + s.part);
  const float* const* lp = b.params + P_L0 + DGVIT_PARAMS_PER_LAYER * i;
  float* const* lg = b.grads + P_L0 + DGVIT_PARAMS_PER_LAYER * i;
  const bf16_t* lw = b.wpack + wp.layer0 + wp.layer_elems * i;
  const unsigned char* lb = ws + w.layer0 + w.layer_stride * i;
  const float* xin = i == 0 ? (const float*)(ws + w.xa) : (const float*)(ws + w.layer0 + w.layer_stride * (i - 1) + w.xout);
  const bf16_t* ln1 = (const bf16_t*)(lb + w.ln);
  const bf16_t* ln2 = (const bf16_t*)(lb + w.ln2);
  const bf16_t* qkv = (const bf16_t*)(lb + w.qkv);
  const bf16_t* ao = (const bf16_t*)(lb + w.ao);
  const bf16_t* h1 = (const bf16_t*)(lb + w.h1);
  const bf16_t* a1 = (const bf16_t*)(lb + w.a1);
  const float* xmid = (const float*)(lb + w.xmid);
  // With dropout the gradient of a branch OUTPUT (fc2, to_out) is dxh o mask / keep: a masked bf16 copy feeds the branch's weight- and
  // data-gradient GEMMs, the residual path keeps dx.  The copy lives in dln, which is free at both points (it is written next by the
  // data-gradient GEMM that follows the copy's last reader); everything runs on the one stream `st`, in order.
  const bool ldrop = b.ldrop();
  // ---- feed-forward branch: xout = xmid + fc2(gelu(fc1(ln2)))        (dx / dxh = d xout)
  const bf16_t* dff = dxh;
  if (ldrop) {
    TRY(drop_rows_bf16(dxh, d.D, dln, d.D, T, d.D, 1, b.site(i, DROP_FF), st));
    dff = dln;
  }
  TRY(b.wgrad(dff, d.D, a1, d.M, lg[L_FC2W], lg[L_FC2B], d.D, d.M));   // (a1 is the masked hidden: the forward dropped it in place)
  {
    GemmBf16Params p = gpb(dff, d.D, lw + wp.fc2T, d.D, dh1, d.M, T, d.M, d.D);   // dh1 = (dx W2) * gelu'(h1)
    p.aux = h1; p.ldaux = d.M;
    TRY(gemm_bf16(BEPI_DGELU_BF16, p, st));
  }
  if (ldrop) TRY(drop_rows_bf16(dh1, d.M, dh1, d.M, T, d.M, 1, b.site(i, DROP_HIDDEN), st));
  TRY(b.wgrad(dh1, d.M, ln2, d.D, lg[L_FC1W], lg[L_FC1B], d.M, d.D));
  {
    GemmBf16Params p = gpb(dh1, d.M, lw + wp.fc1T, d.M, dln, d.D, T, d.D, d.M);     // dln2 = dh1 W1
    TRY(gemm_bf16(BEPI_BF16, p, st));
  }
  TRY(layernorm_bwd_bf16(dln, xmid, (const float*)(lb + w.mean2), (const float*)(lb + w.rstd2), lp[L_LN2W], dx, dx2, dxh, lg[L_LN2W],
                         lg[L_LN2B], part, T, d.D, 1, st));
  // ---- attention branch: xmid = xin + to_out(attn(to_qkv(ln1)))      (dx2 / dxh = d xmid)
  const bf16_t* dat = dxh;
  if (ldrop) {
    TRY(drop_rows_bf16(dxh, d.D, dln, d.D, T, d.D, 1, b.site(i, DROP_OUT), st));
    dat = dln;
  }
  TRY(b.wgrad(dat, d.D, ao, d.I, lg[L_OUTW], lg[L_OUTB], d.D, d.I));
  {
    GemmBf16Params p = gpb(dat, d.D, lw + wp.outT, d.D, dao, d.I, T, d.I, d.D);     // dao = dxmid Wo
    TRY(gemm_bf16(BEPI_BF16, p, st));
  }
  if (ldrop)
    TRY(attention_bwd_bf16_tiled_drop(qkv, ao, dao, (const float*)(lb + w.lse), dqkv, (float*)(sc + s.delta), d.B, d.N, d.H, d.dh,
                                      b.site(i, DROP_ATTN), st));
  else if (d.tiled) TRY(attention_bwd_bf16_tiled(qkv, ao, dao, (const float*)(lb + w.lse), dqkv, (float*)(sc + s.delta), d.B, d.N, d.H, d.dh, st));
  else TRY(attention_bwd_bf16(qkv, ao, dao, (const float*)(lb + w.lse), dqkv, (float*)(sc + s.delta), d.B, d.N, d.H, d.dh, st));
  TRY(b.wgrad(dqkv, 3 * d.I, ln1, d.D, lg[L_QKV], nullptr, 3 * d.I, d.D));
  {
    GemmBf16Params p = gpb(dqkv, 3 * d.I, lw + wp.qkvT, 3 * d.I, dln, d.D, T, d.D, 3 * d.I);   // dln1 = dqkv Wqkv
    TRY(gemm_bf16(BEPI_BF16, p, st));
  }
  TRY(layernorm_bwd_bf16(dln, xin, (const float*)(lb + w.mean1), (const float*)(lb + w.rstd1), lp[L_LN1W], dx2, dx, dxh, lg[L_LN1W],
                         lg[L_LN1B], part, T, d.D, 1, st));
  if (b.events) TRY(mark_ready(b.events->layer[i], st));
  return DGVIT_OK;
}

}  // namespace


extern "C" int dgvit_got_backward_bf16_v3_ev(const dgvit_config* cfg, const float* const* params, const unsigned short* wpack,
                                             float* const* grads, const float* dfeat, float* dgoal, float* dimg, const float* img,
                                             const void* workspace, long long ws_bytes, void* scratch, long long scratch_bytes, int batch,
                                             float keep, float layer_keep, unsigned long long seed, const unsigned long long* seed_dev,
                                             void* stream, const dgvit_grad_events* events) {
  hipStream_t st = (hipStream_t)stream;
  BwdB b = {{}, {}, {}, {}, params, wpack, grads, (const unsigned char*)workspace, (unsigned char*)scratch, st, events, layer_keep, seed, seed_dev};
  DGVIT_CHECK_ARG(layer_keep > 0.f && layer_keep <= 1.f, "layer_keep=%g must be in (0, 1]", (double)layer_keep);
  const Dims& d = b.d;
  TRY(make_dims(cfg, batch, b.d));
  TRY(check_bf16_dims(d));
  DGVIT_CHECK_ARG(params && wpack && grads && dfeat && img && workspace && scratch, "dgvit_got_backward_bf16: null pointer");
  TRY(check_events(events, cfg->depth));
  b.w = make_wsb(d, 1);
  b.wp = make_wp(d);
  b.s = make_bsb(d);
  const Wsb& w = b.w;
  const Bsb& s = b.s;
  if (ws_bytes < w.total) return dgvit_set_error(DGVIT_ERR_WORKSPACE, "bf16 backward workspace %lld < %lld bytes", ws_bytes, w.total);
  if (scratch_bytes < s.total) return dgvit_set_error(DGVIT_ERR_WORKSPACE, "bf16 backward scratch %lld < %lld bytes", scratch_bytes, s.total);
  DGVIT_CHECK_ARG((uintptr_t)workspace % 256 == 0 && (uintptr_t)scratch % 256 == 0, "bf16 path: workspace / scratch must be 256-byte aligned");
  const int np = P_L0 + DGVIT_PARAMS_PER_LAYER * d.L;
  for (int i = 0; i < np; ++i) DGVIT_CHECK_ARG(params[i], "parameter %d is null", i);   // grads[i] == NULL: frozen parameter
  const unsigned char* ws = b.ws;
  unsigned char* sc = b.sc;
  float* dx = (float*)(sc + s.dxa);
  float* dx2 = (float*)(sc + s.dxb);
  float* part = (float*)(sc + s.part);

  // RMSNorm on token 0 (or the token mean) of the last layer's output
  const float* xl = (const float*)(ws + w.layer0 + w.layer_stride * (d.L - 1) + w.xout);
  TRY(head_bwd(d, dfeat, xl, (const float*)(ws + w.pooled), params[P_RMS], grads[P_RMS], dx, dx2, part, events, st));
  TRY(cast_f32_bf16(dx, (bf16_t*)(sc + s.dxh), d.T * d.D, st));
  for (int i = d.L - 1; i >= 0; --i) TRY(layer_bwd_bf16(b, i));
  // token assembly: fp32, as dgvit_got_backward; the patch-weight gradient reads the frame patchified in fp32, the frame gradient
  // takes the fp32 master patch weight
  return token_assembly_bwd(cfg, d, params, grads, dx, dgoal, dimg, dx2, nullptr, img, (float*)(sc + s.patches32), part,
                            (float*)(sc + s.slabs), s.slab_floats, keep, seed, seed_dev, st);
}

// operator-level exports of the bf16 kernels (parity tests, benches)
extern "C" int dgvit_cast_f32_bf16(const float* src, unsigned short* dst, long long n, void* stream) {
  return cast_f32_bf16(src, dst, n, (hipStream_t)stream);
}
extern "C" int dgvit_gemm_bf16(int epilogue, const unsigned short* A, int lda, const unsigned short* B, int ldb, void* C, int ldc,
                               int M, int N, int K, const float* bias, const float* res, int ldr, unsigned short* C2, int ldc2,
                               const unsigned short* aux, int ldaux, void* stream) {
  DGVIT_CHECK_ARG(A && B && C, "dgvit_gemm_bf16: null pointer");
  GemmBf16Params p = gpb(A, lda, B, ldb, C, ldc, M, N, K);
  p.bias = bias; p.res = res; p.ldr = ldr; p.C2 = C2; p.ldc2 = ldc2; p.aux = aux; p.ldaux = ldaux;
  DGVIT_CHECK_ARG(epilogue != BEPI_DGELU_BF16 || aux, "dgvit_gemm_bf16: epilogue 3 needs aux");
  return gemm_bf16(epilogue, p, (hipStream_t)stream);
}
extern "C" long long dgvit_wgrad_bf16_scratch_floats(int Mo, int Ko, int T) {
  return wgrad_bf16_scratch(Mo, Ko, T) + (long long)colsum_bf16_blocks(T) * Mo;
}
extern "C" int dgvit_wgrad_bf16(const unsigned short* dY, const unsigned short* X, float* dW, float* db, float* scratch,
                                long long scratch_floats, int T, int Mo, int Ko, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DGVIT_CHECK_ARG(dY && X && dW && T > 0 && Mo > 0 && Ko > 0 && Mo % 8 == 0 && Ko % 8 == 0, "dgvit_wgrad_bf16: bad arguments");
  // scratch layout: [split-K slabs | bias-gradient partials]
  const long long nsl = wgrad_bf16_scratch(Mo, Ko, T), npart = db ? (long long)colsum_bf16_blocks(T) * Mo : 0;
  if (scratch_floats < nsl + npart) return dgvit_set_error(DGVIT_ERR_WORKSPACE, "dgvit_wgrad_bf16: scratch %lld < %lld floats", scratch_floats, nsl + npart);
  DGVIT_CHECK_ARG(scratch || nsl + npart == 0, "dgvit_wgrad_bf16: null scratch");
  if (db) TRY(colsum_bf16(dY, Mo, db, scratch + nsl, T, Mo, st));
  return wgrad_bf16_tn(dY, Mo, X, Ko, dW, Mo, Ko, T, scratch, nsl, st);
}
extern "C" int dgvit_layernorm_forward_bf16(const float* x, const float* gamma, const float* beta, unsigned short* y, float* mean,
                                            float* rstd, int rows, int D, void* stream) {
  return layernorm_fwd_bf16(x, gamma, beta, y, mean, rstd, rows, D, 1e-5f, 1, (hipStream_t)stream);
}
extern "C" int dgvit_attention_backward_bf16(const unsigned short* qkv, const unsigned short* out, const unsigned short* dout,
                                             const float* lse, unsigned short* dqkv, float* delta, int B, int N, int H, int dh,
                                             void* stream) {
  return attention_bwd_bf16(qkv, out, dout, lse, dqkv, delta, B, N, H, dh, (hipStream_t)stream);
}
extern "C" int dgvit_attention_forward_bf16(const unsigned short* qkv, unsigned short* out, float* lse, int B, int N, int H, int dh,
                                            void* stream) {
  return attention_fwd_bf16(qkv, out, lse, B, N, H, dh, N, (hipStream_t)stream);
}
extern "C" int dgvit_attention_forward_bf16_tiled(const unsigned short* qkv, unsigned short* out, float* lse, int B, int N, int H, int dh,
                                                  int nq, void* stream) {
  return attention_fwd_bf16_tiled(qkv, out, lse, B, N, H, dh, nq, (hipStream_t)stream);
}
extern "C" int dgvit_attention_backward_bf16_tiled(const unsigned short* qkv, const unsigned short* out, const unsigned short* dout,
                                                   const float* lse, unsigned short* dqkv, float* delta, int B, int N, int H, int dh,
                                                   void* stream) {
  return attention_bwd_bf16_tiled(qkv, out, dout, lse, dqkv, delta, B, N, H, dh, (hipStream_t)stream);
}
namespace {
int check_layer_site(const char* what, int layer, int site_lo, int site) {
  DGVIT_CHECK_ARG(layer >= 0 && layer < (1 << 22), "%s: layer=%d outside [0, 2^22)", what, layer);
  DGVIT_CHECK_ARG(site >= site_lo && site <= DROP_FF, "%s: site=%d outside [%d, 3]", what, site, site_lo);
  return DGVIT_OK;
}
}  // namespace
extern "C" int dgvit_attention_forward_bf16_tiled_drop(const unsigned short* qkv, unsigned short* out, float* lse, int B, int N, int H, int dh,
                                                       int nq, float keep, unsigned long long seed, const unsigned long long* seed_dev,
                                                       int layer, void* stream) {
  TRY(check_layer_site("dgvit_attention_forward_bf16_tiled_drop", layer, DROP_ATTN, DROP_ATTN));
  return attention_fwd_bf16_tiled_drop(qkv, out, lse, B, N, H, dh, nq, LayerDrop{keep, drop_tag(layer, DROP_ATTN), seed, seed_dev},
                                       (hipStream_t)stream);
}
extern "C" int dgvit_attention_backward_bf16_tiled_drop(const unsigned short* qkv, const unsigned short* out, const unsigned short* dout,
                                                        const float* lse, unsigned short* dqkv, float* delta, int B, int N, int H, int dh,
                                                        float keep, unsigned long long seed, const unsigned long long* seed_dev, int layer,
                                                        void* stream) {
  TRY(check_layer_site("dgvit_attention_backward_bf16_tiled_drop", layer, DROP_ATTN, DROP_ATTN));
  return attention_bwd_bf16_tiled_drop(qkv, out, dout, lse, dqkv, delta, B, N, H, dh, LayerDrop{keep, drop_tag(layer, DROP_ATTN), seed, seed_dev},
                                       (hipStream_t)stream);
}
extern "C" int dgvit_drop_rows_bf16(const unsigned short* src, long long lds, unsigned short* dst, long long ldd, long long rows, int width,
                                    int rs, float keep, unsigned long long seed, const unsigned long long* seed_dev, int layer, int site,
                                    void* stream) {
  TRY(check_layer_site("dgvit_drop_rows_bf16", layer, DROP_OUT, site));
  return drop_rows_bf16(src, lds, dst, ldd, rows, width, rs, LayerDrop{keep, drop_tag(layer, site), seed, seed_dev}, (hipStream_t)stream);
}
