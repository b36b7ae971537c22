// The fp32 encoder (GoalFormer.py:156-171): workspace carve-ups, dgvit_got_forward[_v2] and every dgvit_got_backward* entry point.
#include <mutex>

#include "schedule.h"

// ---------------------------------------------------------------------------------------------- helper stream
// dgvit_got_backward forks every weight-gradient GEMM (+ its slab reduction) onto one internal non-blocking
// stream and joins it back with events, so the wgrad workgroups fill the tail / prologue bubbles of the
// data-gradient kernels on the caller's stream.  All ordering is event based (capturable into a hipGraph);
// the helper stream and a ring of events are created on first use and live for the process.
namespace {
struct Side {
  hipStream_t stream = nullptr;
  hipEvent_t ring[32];
  unsigned next = 0;
  bool ready = false;
};
Side g_side;
std::mutex g_side_mu;

int side_init() {
  std::lock_guard<std::mutex> lk(g_side_mu);
  if (g_side.ready) return DGVIT_OK;
  if (hipStreamCreateWithFlags(&g_side.stream, hipStreamNonBlocking) != hipSuccess)
    return dgvit_set_error(DGVIT_ERR_HIP, "cannot create the helper stream");
  for (auto& e : g_side.ring)
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
      return dgvit_set_error(DGVIT_ERR_HIP, "cannot create helper events");
  g_side.ready = true;
  return DGVIT_OK;
}
// `to` waits for everything enqueued on `from` so far
int chain(hipStream_t from, hipStream_t to) {
  hipEvent_t e = g_side.ring[g_side.next++ % 32];
  if (hipEventRecord(e, from) != hipSuccess || hipStreamWaitEvent(to, e, 0) != hipSuccess)
    return dgvit_set_error(DGVIT_ERR_HIP, "event fork/join failed");
  return DGVIT_OK;
}
}  // namespace

namespace {

SplitNeed forward_split_need(const Dims& d) {
  SplitNeed n;
  const int T = (int)d.T;
  n.add(GEMM_NT, (long long)d.B * d.P, d.D, d.pd);
  n.add_gather((long long)d.B * d.P, d.D, d.pd);
  n.add(GEMM_NT, T, 3 * d.I, d.D); n.add(GEMM_NT, T, 2 * d.I, d.D); n.add(GEMM_NT, d.B, d.I, d.D);
  for (int tok : {T, d.B}) {
    n.add(GEMM_NT, tok, d.D, d.I); n.add(GEMM_NT, tok, d.M, d.D); n.add(GEMM_NT, tok, d.D, d.M);
  }
  return n;
}
SplitNeed backward_split_need(const Dims& d) {
  SplitNeed n;
  const int T = (int)d.T;
  for (int tok : {T, d.B}) {
    n.add(GEMM_NN, tok, d.M, d.D); n.add(GEMM_NN, tok, d.D, d.M); n.add(GEMM_NN, tok, d.I, d.D); n.add(GEMM_NN, tok, d.D, d.I);
  }
  n.add(GEMM_NN, T, d.D, 3 * d.I); n.add(GEMM_NN, T, d.D, 2 * d.I);
  return n;
}

// activation workspace carve-up (floats); `save` keeps per-layer buffers distinct
struct Ws {
  long long patches, x0, pooled, layer0, layer_stride, layer_floats, total;
  long long sk_counters, sk_slabs, sk_ncounters, sk_slab_floats;   // in-launch split-K scratch (0 floats when no GEMM splits)
  long long bp_counters, bp_slabs, bp_ncounters;                    // combine scratch of the two-launch small-batch blocks (block.hip; inference only)
  // per-layer offsets relative to the layer base
  long long mean1, rstd1, ln1, qkv, ao, lse, xmid, mean2, rstd2, ln2, h1, a1, xout;
};

// no-grad forwards of a few frames take the two-launch blocks of block.hip.  Where they win, measured against the seven-launch GEMM
// schedule as captured single-launch graphs of policy.sample() (tools/small_batch_ab.py, profiles/r04_*_small_batch_ab.txt): while the
// attention kernel's workgroups (frames x heads x query tiles) fit the chip one per CU -- 0.68-0.76 of the GEMM schedule's time at D = 64
// for 1-16 frames, 0.75-0.89 at D = 128 for 1-32 frames; parity at 32 frames of the shipped model, slower beyond -- and, at D = 256, where
// a workgroup's projections (contraction over 256 on ONE CU) outweigh the saved launches, for a single frame only (0.95; 1.1-1.5 beyond).
bool block_path_eligible(const Dims& d) {
  if (!d.proj || d.T > g_block_path_max_rows || !block_path_supports(d.B, d.N, d.D, d.H, d.dh, d.M)) return false;
  KNOB_IF(g_block_path == 2) return true;      // diagnostic build: every supported shape (tests of ragged row tiles, many frames)
  const long long items = (long long)d.B * d.H * ((d.N + 31) / 32);
  return d.D <= 128 ? items <= 256 : items <= 16;
}

Ws make_ws(const Dims& d, int save) {
  Ws w;
  long long o = 0;
  w.patches = o; o += al4((long long)d.B * d.P * d.pd);
  w.x0 = o; o += al4(d.T * d.D);
  w.pooled = o; o += al4((long long)d.B * d.D);   // token mean (pool='mean' only)
  const SplitNeed sn = forward_split_need(d);
  w.sk_ncounters = sn.tiles; w.sk_slab_floats = sn.slab;
  w.sk_counters = o; o += al4(sn.tiles);
  // (the small-batch blocks' arrival counters sit right behind the split-K ones: ONE memset zeroes both)
  w.bp_counters = o; w.bp_ncounters = 0;
  const bool blocks = !save && block_path_eligible(d);
  if (blocks) {
    w.bp_ncounters = block_path_counters(d.B, d.N);
    o += al4(w.bp_ncounters);
  }
  w.sk_slabs = o; o += al4(sn.slab);
  w.bp_slabs = o;
  if (blocks) o += al4(block_path_slab_floats(d.B, d.N, d.D, d.H, d.M));
  long long l = 0;
  w.mean1 = l; l += al4(d.T);
  w.rstd1 = l; l += al4(d.T);
  w.ln1 = l; l += al4(d.T * d.D);
  w.qkv = l; l += al4(d.T * 3 * d.I);
  w.ao = l; l += al4(d.T * d.I);
  w.lse = l; l += al4((long long)d.B * d.H * d.N);   // base-2 log-sum-exp of every attention row
  w.xmid = l; l += al4(d.T * d.D);
  w.mean2 = l; l += al4(d.T);
  w.rstd2 = l; l += al4(d.T);
  w.ln2 = l; l += al4(d.T * d.D);
  w.h1 = l; l += al4(d.T * d.M);
  w.a1 = l; l += al4(d.T * d.M);
  w.xout = l; l += al4(d.T * d.D);
  w.layer0 = o;
  w.layer_floats = l;
  if (save) {
    w.layer_stride = l;
    o += l * d.L;
  } else {
    // inference: one shared set of temporaries; odd layers write their output into one extra
    // residual-stream buffer placed right behind it, even layers into the shared `xout`
    w.layer_stride = 0;
    long long region = l + al4(d.T * d.D);
#ifdef DGVIT_DIAG
    if (frame_path_supports(d.B, d.N, d.D, d.H, d.dh, d.M)) region = std::max(region, al4(frame_path_scratch_floats(d.B, d.N, d.D, d.H, d.M)));
#endif
    o += region;
  }
  w.total = o;
  return w;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- encoder
extern "C" long long dgvit_got_workspace_floats(const dgvit_config* cfg, int batch, int save) {
  Dims d;
  if (make_dims(cfg, batch, d)) return -1;
  return make_ws(d, save).total;
}

namespace {
struct Bs {  // backward scratch carve-up
  long long dxa, dxb, dln, dqkv, dao, dh1, dm1, dm3, part, part_ln2, part_ln1, slabs, total, slabs_floats;
  long long delta, delta_floats;   // the tiled attention backward's rowsum(dO o O) (0 floats unless Dims::tiled)
  long long sl_fc2, sl_fc1, sl_out, sl_qkv, n_fc2, n_fc1, n_out, n_qkv;   // a layer's four weight gradients keep separate slab regions
  long long sk_counters, sk_slabs, sk_ncounters, sk_slab_floats;          // in-launch split-K scratch of the data-gradient GEMMs
};
Bs make_bs(const Dims& d) {
  Bs s;
  long long o = 0;
  s.dxa = o; o += al4(d.T * d.D);
  s.dxb = o; o += al4(d.T * d.D);
  s.dln = o; o += al4(d.T * d.D);
  s.dqkv = o; o += al4(d.T * 3 * d.I);
  s.dao = o; o += al4(d.T * d.I);
  s.dh1 = o; o += al4(d.T * d.M);
  // transformer dropout (layer keep < 1): dx o m / keep of the to_out (site 1) and fc2 (site 3) branches, the A operand of their data and
  // weight gradients.  Two regions: the helper stream may still read one while the caller's stream writes the other.
  s.dm1 = o; o += al4(d.T * d.D);
  s.dm3 = o; o += al4(d.T * d.D);
  // reduction partials: LN (blocks*2*D), colsum (blocks*max width), rms, dpos (blocks * N*D)
  long long part = (long long)layernorm_bwd_blocks((int)d.T) * 2 * d.D;
  const long long widest = (long long)(d.M > 3 * d.I ? d.M : 3 * d.I);
  const long long cs = (long long)colsum_blocks((int)d.T) * widest;
  if (cs > part) part = cs;
  const long long dp = (long long)colsum_blocks(d.B) * d.N * d.D;
  if (dp > part) part = dp;
  const long long rp = (long long)rmsnorm_bwd_blocks(d.B) * d.D;
  if (rp > part) part = rp;
  s.part = o; o += al4(part);
  // the two LayerNorm backward passes of a layer keep their dgamma / dbeta partials until the layer's ONE grouped reduction
  const long long lnp = al4((long long)layernorm_bwd_blocks((int)d.T) * 2 * d.D);
  s.part_ln2 = o; o += lnp;
  s.part_ln1 = o; o += lnp;
  // ... and so do its four split-K weight gradients (the last block's to_qkv gradient is two GEMMs: Q rows, K/V rows)
  s.n_fc2 = wgrad_scratch(d.D, d.M, (int)d.T);
  s.n_fc1 = wgrad_scratch(d.M, d.D, (int)d.T);
  s.n_out = wgrad_scratch(d.D, d.I, (int)d.T);
  s.n_qkv = std::max(wgrad_scratch(3 * d.I, d.D, (int)d.T), wgrad_scratch(d.I, d.D, d.B) + wgrad_scratch(2 * d.I, d.D, (int)d.T));
  s.sl_fc2 = 0; s.sl_fc1 = s.n_fc2; s.sl_out = s.sl_fc1 + s.n_fc1; s.sl_qkv = s.sl_out + s.n_out;
  long long sl = s.sl_qkv + s.n_qkv;
  sl = std::max(sl, wgrad_scratch(d.D, d.pd, d.B * d.P));
  s.slabs = o; s.slabs_floats = sl; o += sl;
  const SplitNeed sn = backward_split_need(d);
  s.sk_ncounters = sn.tiles; s.sk_slab_floats = sn.slab;
  s.sk_counters = o; o += al4(sn.tiles);
  s.sk_slabs = o; o += al4(sn.slab);
  s.delta = o; s.delta_floats = d.tiled ? attention_bwd_tiled_scratch(d.B, d.N, d.H) : 0; o += al4(s.delta_floats);
  s.total = o;
  return s;
}
}  // namespace

extern "C" long long dgvit_got_backward_scratch_floats(const dgvit_config* cfg, int batch) {
  Dims d;
  if (make_dims(cfg, batch, d)) return -1;
  return make_bs(d).total;
}

// does a training forward (save != 0) and its backward fold K and V of the pruned last block into token 0's query for this
// configuration (schedule.h last_block_fold)?  1 / 0, negative on a bad configuration.  `maps` != 0: a dgvit_got_forward_maps call
// (always no-grad: never folds, like every other no-grad forward).  16-byte aligned weights assumed.
extern "C" int dgvit_got_last_block_folds(const dgvit_config* cfg, int batch, float lkeep, int maps) {
  Dims d;
  if (make_dims(cfg, batch, d)) return -1;
  alignas(16) static const float aligned = 0.f;
  return last_block_fold(d, !dense_last_block(cfg) && !d.pool_mean, lkeep < 1.f, maps != 0, maps == 0, &aligned) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------- forward
namespace {

// one forward call: what its steps share
struct Fwd {
  const dgvit_config* cfg;
  Dims d;
  Ws w;
  const float* const* params;
  float* ws;
  SplitBuf sk;
  int save;
  float lkeep;
  bool ldrop;   // transformer dropout (GoalFormer.py:47,49,68,78): the GEMM schedule only -- the block and frame paths do not apply it
  unsigned long long seed;
  const unsigned long long* seed_dev;
  hipStream_t st;
  float* maps = nullptr;   // attention maps (dgvit_got_forward_maps): (B, L, H, N) or (B, L, H, N, N); null in every other call
  int maps_rows = DGVIT_MAPS_GOAL;
  LayerDrop site(int layer, int s) const { return LayerDrop{lkeep, drop_tag(layer, s), seed, seed_dev}; }
  // the last block runs dense under the flag, and for maps of every query row (rows other than 0 do not exist in the token-0 block)
  bool dense_last() const { return dense_last_block(cfg) || (maps && maps_rows == DGVIT_MAPS_ALL); }
};

// Inference: the patch rearrangement (GoalFormer.py:138) happens inside the GEMM's A-tile loader -- depth patches go from the
// image straight into the LDS tiles, no (B * P, pd) copy in HBM.  Training keeps the copy: the weight gradient reads it.
int patch_gather_inv(const dgvit_config* cfg) { return 65536 / cfg->patch_w + 1; }
bool patch_gather(const dgvit_config* cfg, const Dims& d, const float* img, const float* wpe, int save) {
  const int inv = patch_gather_inv(cfg);
  bool gather = !save && cfg->patch_w % 4 == 0 && cfg->image_w % 4 == 0 && ((uintptr_t)img & 15) == 0 && ((uintptr_t)wpe & 15) == 0 &&
                (long long)d.pd * inv < (1ll << 31) && (long long)d.B * cfg->image_h * cfg->image_w < (1ll << 29);
  for (int k = 0; gather && k < d.pd; ++k) gather = (int)(((unsigned)k * (unsigned)inv) >> 16) == k / cfg->patch_w;   // exact k / pw
  return gather;
}

// Token assembly into x0: patch embedding (GoalFormer.py:137-139,157) + goal token, positional embedding, dropout (:160-163).
// fused_first: the first small-batch block zeroes the counters and assembles the goal row and emb-dropout itself.
int token_assembly(const Fwd& f, const float* img, const float* goal, float keep, bool gather, bool fused_first) {
  const Dims& d = f.d;
  const Ws& w = f.w;
  const dgvit_config* cfg = f.cfg;
  float* ws = f.ws;
  hipStream_t st = f.st;
  float* patches = ws + w.patches;
  float* x = ws + w.x0;
  // arrival counters of the split GEMMs and of the small-batch blocks (adjacent): every user leaves them zero again
  if (!fused_first && (w.sk_slab_floats > 0 || w.bp_ncounters > 0))
    TRY(zero_fill(ws + w.sk_counters, (long long)sizeof(int) * (w.bp_counters - w.sk_counters + w.bp_ncounters), st));
  if (!gather) TRY(patchify(img, patches, d.B, cfg->image_h, cfg->image_w, cfg->patch_h, cfg->patch_w, st));
  {
    GemmParams p = gp(patches, d.pd, f.params[P_PW], d.pd, x, d.D, d.B * d.P, d.D, d.pd);
    p.bias = f.params[P_PB];
    p.res = f.params[P_POS]; p.ldr = d.D; p.res_mod = d.P;  // + pos_embedding[1 + patch]
    p.c_rgrp = d.P;                                         // row (b, patch) -> token row b*N + 1 + patch
    if (gather) {
      p.g_img = img; p.g_img_floats = (long long)d.B * cfg->image_h * cfg->image_w;
      p.g_wi = cfg->image_w; p.g_hw = cfg->image_h * cfg->image_w; p.g_ph = cfg->patch_h; p.g_pw = cfg->patch_w;
      p.g_gw = cfg->image_w / cfg->patch_w; p.g_P = d.P; p.g_inv = patch_gather_inv(cfg);
    }
    f.sk.attach(p);
    TRY(gemm_f32(GEMM_NT, EPI_STORE, p, 1, st));
  }
  if (!fused_first) {
    TRY(goal_row(goal, f.params[P_POS], x, d.B, d.N, d.D, st));
    if (keep < 1.f) TRY(dropout_inplace(x, d.T * d.D, f.seed, f.seed_dev, keep, st));
  }
  return DGVIT_OK;
}

// Small no-grad batches (SAC.choose_action on one frame, the target passes of learn() on a few frames): two launches per block, the
// sums over heads / hidden chunks taken inside the launches (block.hip), the LayerNorms in their combine steps.  The pruned last
// block's MLP kernel also applies the final RMSNorm to the pooled rows (g_block_fuse bit 1; GoalFormer.py:167-170).
int block_path_forward(const Fwd& f, const float* goal, float keep, bool fused_first, float* x, float* feat) {
  const Dims& d = f.d;
  const Ws& w = f.w;
  const float* const* params = f.params;
  float* ws = f.ws;
  int* counters = reinterpret_cast<int*>(ws + w.bp_counters);       // (zeroed by token_assembly, or by the first attention kernel)
  float* lb = ws + w.layer0;
  BlockFirst first = {};
  first.goal = goal; first.pos0 = params[P_POS]; first.xres = lb + w.xmid;   // (xmid: free in this path) the assembled, dropped-out token rows
  first.keep = keep; first.seed = f.seed; first.seed_dev = f.seed_dev;
  bool feat_done = false;
  for (int i = 0; i < d.L; ++i) {
    const float* const* lp = params + P_L0 + DGVIT_PARAMS_PER_LAYER * i;
    float* xo = !(i & 1) ? lb + w.xout : ws + w.layer0 + w.layer_floats;
    const bool last = !dense_last_block(f.cfg) && !d.pool_mean && i == d.L - 1;
    const float* next_ln[2] = {nullptr, nullptr};
    if (i + 1 < d.L) {
      next_ln[0] = params[P_L0 + DGVIT_PARAMS_PER_LAYER * (i + 1) + L_LN1W];
      next_ln[1] = params[P_L0 + DGVIT_PARAMS_PER_LAYER * (i + 1) + L_LN1B];
    }
    DGVIT_DIAG_ONLY(g_block_stamp_now = g_block_stamp_layer < 0 || g_block_stamp_layer == i;)
    // (block 0 normalises its input inside the attention kernel; later blocks read the rows the previous MLP kernel normalised)
    TRY(block_path_layer(x, i == 0 ? nullptr : lb + w.ln1, xo, lb + w.ln1, lp, i + 1 < d.L ? next_ln : nullptr, last ? 1 : 0, ws + w.bp_slabs,
                         counters, i == 0 && fused_first ? &first : nullptr, last && (g_block_fuse & 2) ? params[P_RMS] : nullptr, last ? feat : nullptr, d.B, d.N,
                         d.D, d.H, d.dh, d.M, f.st));
    feat_done = last && (g_block_fuse & 2);
    x = xo;
  }
  if (feat_done) return DGVIT_OK;
  return pool_rmsnorm_fwd(d, x, ws + w.pooled, params[P_RMS], feat, f.st);
}

// One block of the GEMM schedule: x = attn(LN(x)) + x; x = ff(LN(x)) + x   (GoalFormer.py:103-104).  x advances to the block's output.
int gemm_layer(const Fwd& f, int i, float*& x) {
  const Dims& d = f.d;
  const Ws& w = f.w;
  const float* const* params = f.params;
  float* ws = f.ws;
  const int save = f.save;
  const bool ldrop = f.ldrop;
  hipStream_t st = f.st;
  const SplitBuf& sk = f.sk;
  const int T = (int)d.T;
  // (with transformer dropout the branch is masked after its GEMM, before the residual add: the LayerNorms run as kernels of their own)
  const bool ln_fused = g_ln_fusion && d.D == 64 && g_gemm_tile_hint == 0 && !ldrop;   // (the automatic tile for N = 64 is 64 wide)
  const float* const* lp = params + P_L0 + DGVIT_PARAMS_PER_LAYER * i;
  float* lb = ws + w.layer0 + w.layer_stride * i;
  float* xo = (save || !(i & 1)) ? lb + w.xout : ws + w.layer0 + w.layer_floats;
  // The output only reads token 0 of the last block (GoalFormer.py:167): there, K and V are needed for every
  // token but Q, the attention output, to_out and the whole feed-forward only for row b*N of each frame.
  // `tok` = rows processed, `rs` = row step (in token rows) of those rows inside the (T, .) buffers.
  const bool last = !f.dense_last() && !d.pool_mean && i == d.L - 1;
  const int tok = last ? d.B : T, rs = last ? d.N : 1;
  // ... and with to_qkv bias-free, K and V fold into token 0's query: no K / V GEMM at all (last_block.hip)
  const bool fold = last_block_fold(d, last, ldrop, f.maps != nullptr, save != 0, lp[L_QKV]);
  // x = attn(LN(x)) + x   (GoalFormer.py:103, 36-37, 71-82)
  // D <= 64 (the shipped model): a 64-wide GEMM tile holds whole rows of the residual stream, so each LayerNorm runs inside the
  // epilogue of the GEMM that produces its input (to_out -> LN2, fc2 -> the next block's LN1; bit-identical to the LayerNorm
  // kernel).  Only the first block's LN1 is a launch of its own: 8 -> 1 LayerNorm launches in the shipped 4-block encoder.
  if (!(ln_fused && i > 0))
    TRY(layernorm_fwd(x, lp[L_LN1W], lp[L_LN1B], lb + w.ln1, lb + w.mean1, lb + w.rstd1, T, d.D, 1e-5f, 1, st));
  if (!last) {
    GemmParams p = gp(lb + w.ln1, d.D, lp[L_QKV], d.D, lb + w.qkv, 3 * d.I, T, 3 * d.I, d.D);
    sk.attach(p);
    TRY(gemm_f32(GEMM_NT, EPI_STORE, p, 1, st));
  } else {
    if (!fold) {
      GemmParams kv = gp(lb + w.ln1, d.D, lp[L_QKV] + (long long)d.I * d.D, d.D, lb + w.qkv + d.I, 3 * d.I, T, 2 * d.I, d.D);
      sk.attach(kv);
      TRY(gemm_f32(GEMM_NT, EPI_STORE, kv, 1, st));
    }
    GemmParams q = gp(lb + w.ln1, rs * d.D, lp[L_QKV], d.D, lb + w.qkv, rs * 3 * d.I, tok, d.I, d.D);
    sk.attach(q);
    TRY(gemm_f32(GEMM_NT, EPI_STORE, q, 1, st));
  }
  const LayerDrop dr_attn = f.site(i, DROP_ATTN);
  float* lse = save || f.maps ? lb + w.lse : nullptr;   // (a maps call reads the row statistics back)
  if (fold) {
    // u, r behind q in the frame's rows of the qkv slot; the probabilities (B, H, N) in the lse slot
    float* u = lb + w.qkv + d.I;
    TRY(goal_attention_fwd(lb + w.ln1, lp[L_QKV], lb + w.qkv, (long long)rs * 3 * d.I, lb + w.ao, (long long)rs * d.I, u, u + (long long)d.H * d.D,
                           3ll * d.N * d.I, lse, d.B, d.N, d.H, d.dh, d.D, st));
  } else if (d.tiled)
    TRY(attention_fwd_tiled(lb + w.qkv, lb + w.ao, lse, d.B, d.N, d.H, d.dh, last ? 1 : d.N, st, ldrop ? &dr_attn : nullptr));
  else
    TRY(attention_fwd(lb + w.qkv, lb + w.ao, lse, d.B, d.N, d.H, d.dh, last ? 1 : d.N, st, ldrop ? &dr_attn : nullptr));
  if (f.maps) {   // this layer's probabilities, before the next layer overwrites the shared qkv / lse of a no-grad pass
    const long long per_head = f.maps_rows == DGVIT_MAPS_ALL ? (long long)d.N * d.N : d.N;
    TRY(attention_probs(lb + w.qkv, lse, f.maps + (long long)i * d.H * per_head, (long long)d.L * d.H * per_head, d.B, d.N, d.H, d.dh,
                        f.maps_rows, st));
  }
  if (!d.proj) {
    // to_out = nn.Identity() (GoalFormer.py:56,66-69): the head's output IS the branch output (I == D): xmid = attn + x (:103)
    TRY(add_rows(lb + w.ao, (long long)rs * d.I, x, (long long)rs * d.D, lb + w.xmid, (long long)rs * d.D, tok, d.D, st));
  } else {
    GemmParams p = gp(lb + w.ao, rs * d.I, lp[L_OUTW], d.I, lb + w.xmid, rs * d.D, tok, d.D, d.I);
    p.bias = lp[L_OUTB]; p.res = ldrop ? nullptr : x; p.ldr = rs * d.D;
    if (ln_fused) {
      p.ln_g = lp[L_LN2W]; p.ln_b = lp[L_LN2B]; p.ln_y = lb + w.ln2; p.ln_ld = (long long)rs * d.D;
      p.ln_mean = lb + w.mean2; p.ln_rstd = lb + w.rstd2; p.ln_eps = 1e-5f;
    }
    sk.attach(p);
    TRY(gemm_f32(GEMM_NT, EPI_STORE, p, 1, st));
    // xmid = x + m o (ao Wo^T + b) / keep   (site 1)
    if (ldrop) TRY(drop_rows(lb + w.xmid, (long long)rs * d.D, lb + w.xmid, (long long)rs * d.D, x, (long long)rs * d.D, tok, d.D, rs,
                             f.site(i, DROP_OUT), st));
  }
  // x = ff(LN(x)) + x     (GoalFormer.py:104, 42-50)
  if (!ln_fused || !d.proj) TRY(layernorm_fwd(lb + w.xmid, lp[L_LN2W], lp[L_LN2B], lb + w.ln2, lb + w.mean2, lb + w.rstd2, tok, d.D, 1e-5f, rs, st));
  {
    // training: a1 = gelu(t) for fc2 and the weight gradient, and -- in the h1 slot -- gelu'(t), the factor the data gradient of fc2
    // multiplies by (the erf form already holds its exponential; the backward epilogue then evaluates nothing).  No-grad passes
    // store a1 only: the pre-activation (210 MB per layer at C3) is never written.
    GemmParams p = gp(lb + w.ln2, rs * d.D, lp[L_FC1W], d.D, save ? lb + w.h1 : lb + w.a1, d.M, tok, d.M, d.D);   // h1 / a1 are dense (tok, M)
    p.bias = lp[L_FC1B];
    if (save) { p.C2 = lb + w.a1; p.ldc2 = d.M; }
    sk.attach(p);
    TRY(gemm_f32(GEMM_NT, save ? (g_gelu_grad_store || ldrop ? EPI_GELU2D : EPI_GELU2) : EPI_GELU, p, 1, st));
    // site 2: gelu(t) o m / keep, and the same factor folded into the stored gelu'(t) (the backward's EPI_DMUL and fc2's weight
    // gradient then need nothing more)
    if (ldrop) {
      TRY(drop_rows(lb + w.a1, d.M, lb + w.a1, d.M, nullptr, 0, tok, d.M, rs, f.site(i, DROP_HIDDEN), st));
      if (save) TRY(drop_rows(lb + w.h1, d.M, lb + w.h1, d.M, nullptr, 0, tok, d.M, rs, f.site(i, DROP_HIDDEN), st));
    }
  }
  {
    GemmParams p = gp(lb + w.a1, d.M, lp[L_FC2W], d.M, xo, rs * d.D, tok, d.D, d.M);
    p.bias = lp[L_FC2B]; p.res = ldrop ? nullptr : lb + w.xmid; p.ldr = rs * d.D;
    if (ln_fused && i + 1 < d.L) {   // the next block's LN1 (this block is never the pruned last one: all T rows)
      const float* const* ln = params + P_L0 + DGVIT_PARAMS_PER_LAYER * (i + 1);
      float* nb = ws + w.layer0 + w.layer_stride * (i + 1);
      p.ln_g = ln[L_LN1W]; p.ln_b = ln[L_LN1B]; p.ln_y = nb + w.ln1; p.ln_ld = d.D;
      p.ln_mean = nb + w.mean1; p.ln_rstd = nb + w.rstd1; p.ln_eps = 1e-5f;
    }
    sk.attach(p);
    TRY(gemm_f32(GEMM_NT, EPI_STORE, p, 1, st));
    // xout = xmid + m o (a1 W2^T + b) / keep   (site 3)
    if (ldrop) TRY(drop_rows(xo, (long long)rs * d.D, xo, (long long)rs * d.D, lb + w.xmid, (long long)rs * d.D, tok, d.D, rs,
                             f.site(i, DROP_FF), st));
  }
  x = xo;
  return DGVIT_OK;
}

}  // namespace

extern "C" int dgvit_got_forward(const dgvit_config* cfg, const float* const* params, const float* img, const float* goal,
                                 float* feat, float* ws, long long ws_floats, int batch, int save, float keep,
                                 unsigned long long seed, const unsigned long long* seed_dev, void* stream) {
  return dgvit_got_forward_v2(cfg, params, img, goal, feat, ws, ws_floats, batch, save, keep, 1.f, seed, seed_dev, stream);
}

namespace {
int got_forward(Fwd& f, const float* img, const float* goal, float* feat, long long ws_floats, int batch, float keep) {
  const dgvit_config* cfg = f.cfg;
  const float* const* params = f.params;
  float* ws = f.ws;
  const int save = f.save;
  const float lkeep = f.lkeep;
  const Dims& d = f.d;
  TRY(make_dims(cfg, batch, f.d));
  DGVIT_CHECK_ARG(params && img && goal && feat && ws, "dgvit_got_forward: null pointer");
  DGVIT_CHECK_ARG(keep > 0.f && keep <= 1.f, "dropout_keep must be in (0, 1]");
  DGVIT_CHECK_ARG(lkeep > 0.f && lkeep <= 1.f, "layer_dropout_keep must be in (0, 1]");
  f.w = make_ws(d, save);
  const Ws& w = f.w;
  if (ws_floats < w.total) return dgvit_set_error(DGVIT_ERR_WORKSPACE, "forward workspace %lld < %lld floats", ws_floats, w.total);
  for (int i = 0; i < P_L0 + DGVIT_PARAMS_PER_LAYER * d.L; ++i) DGVIT_CHECK_ARG(params[i] || no_projection_slot(d, i), "parameter %d is null", i);
  if (w.sk_slab_floats > 0) {
    f.sk.counters = reinterpret_cast<int*>(ws + w.sk_counters); f.sk.ncounters = (int)w.sk_ncounters;
    f.sk.slabs = ws + w.sk_slabs; f.sk.slab_cap = w.sk_slab_floats;
  }

  // Which path runs: the two-launch small-batch blocks, (diagnostic build) the per-frame path, or the GEMM schedule
  const bool use_blocks = !save && !f.ldrop && !f.maps && g_block_path && !g_small_path && w.bp_ncounters > 0;
  const bool gather = patch_gather(cfg, d, img, params[P_PW], save);
  // ... with the loader gather no GEMM of this call splits, so nothing needs the counters before the first block's attention kernel,
  // which can then zero them itself AND assemble the token rows (goal row, emb-dropout): three launches fewer.  Built, parity-tested
  // and NOT the default (g_block_fuse bit 0, diagnostic build): in one process, graphed sample() of the shipped actor, it measures
  // +14 us for one frame, -3 us for two, +4 us for eight (profiles/r04_c_block_fuse_ab.txt) -- the three launches it removes were not
  // on the critical path the way the in-kernel work that replaces them is.  The RMSNorm fusion (bit 1) is worth 2 us everywhere and stays.
  const bool fused_first = use_blocks && gather && (g_block_fuse & 1);
  TRY(token_assembly(f, img, goal, keep, gather, fused_first));
  float* x = ws + w.x0;
#ifdef DGVIT_DIAG   // (measured slower than the schedule below, DESIGN 3.7: not in the product library)
  if (!save && !f.ldrop && !f.maps && g_small_path && !d.pool_mean && d.proj && d.T <= g_small_path_max_rows && frame_path_supports(d.B, d.N, d.D, d.H, d.dh, d.M))
    return frame_path_forward(x, params, d.L, ws + w.layer0, feat, d.B, d.N, d.D, d.H, d.dh, d.M, f.st);
#endif
  if (use_blocks) return block_path_forward(f, goal, keep, fused_first, x, feat);
  for (int i = 0; i < d.L; ++i) TRY(gemm_layer(f, i, x));
  return pool_rmsnorm_fwd(d, x, ws + w.pooled, params[P_RMS], feat, f.st);
}
}  // namespace

extern "C" int dgvit_got_forward_v2(const dgvit_config* cfg, const float* const* params, const float* img, const float* goal,
                                    float* feat, float* ws, long long ws_floats, int batch, int save, float keep, float lkeep,
                                    unsigned long long seed, const unsigned long long* seed_dev, void* stream) {
  Fwd f = {cfg, {}, {}, params, ws, {}, save, lkeep, lkeep < 1.f, seed, seed_dev, (hipStream_t)stream};
  return got_forward(f, img, goal, feat, ws_floats, batch, keep);
}

// the no-grad forward with each layer's attention probabilities (include/dgvit_hip.h: Attention maps)
extern "C" int dgvit_got_forward_maps(const dgvit_config* cfg, const float* const* params, const float* img, const float* goal, float* feat,
                                      float* maps, int rows, float* ws, long long ws_floats, int batch, float keep, float lkeep,
                                      unsigned long long seed, const unsigned long long* seed_dev, void* stream) {
  Dims d;
  TRY(make_dims(cfg, batch, d));
  DGVIT_CHECK_ARG(maps, "dgvit_got_forward_maps: null maps pointer");
  DGVIT_CHECK_ARG(rows == DGVIT_MAPS_GOAL || rows == DGVIT_MAPS_ALL, "dgvit_got_forward_maps: rows=%d must be DGVIT_MAPS_GOAL (0) or DGVIT_MAPS_ALL (1)", rows);
  Fwd f = {cfg, {}, {}, params, ws, {}, 0, lkeep, lkeep < 1.f, seed, seed_dev, (hipStream_t)stream};
  f.maps = maps;
  f.maps_rows = rows;
  return got_forward(f, img, goal, feat, ws_floats, batch, keep);
}

// ---------------------------------------------------------------------------------------------- backward
namespace {

// one backward call: what its steps share
struct Bwd {
  const dgvit_config* cfg;
  Dims d;
  Ws w;
  Bs s;
  const float* const* params;
  float* const* grads;
  const float* ws;
  float* scratch;
  SplitBuf sk;   // the data-gradient GEMMs all run on the caller's stream, one after the other: one counter / slab region serves them
  float lkeep;
  bool ldrop;    // the masks of dgvit_got_forward_v2, regenerated from the same seed
  unsigned long long seed;
  const unsigned long long* seed_dev;
  hipStream_t st;
  // weight gradients run on the helper stream `sw` (== st without DGVIT_FLAG_WGRAD_OVERLAP)
  hipStream_t sw;
  const dgvit_grad_events* events;
  LayerDrop site(int layer, int s) const { return LayerDrop{lkeep, drop_tag(layer, s), seed, seed_dev}; }
  int fork() const { return sw == st ? DGVIT_OK : chain(st, sw); }
  int join() const { return sw == st ? DGVIT_OK : chain(sw, st); }
};

// Gradient of one block: dx (the gradient of the block's output) becomes the gradient of its input; the block's parameter gradients
// are final in stream order when this returns.
int backward_layer(const Bwd& b, int i) {
  const Dims& d = b.d;
  const Ws& w = b.w;
  const Bs& s = b.s;
  const float* ws = b.ws;
  float* scratch = b.scratch;
  const bool ldrop = b.ldrop;
  hipStream_t st = b.st, sw = b.sw;
  const SplitBuf& sk = b.sk;
  const int T = (int)d.T;
  float* dx = scratch + s.dxa;    // gradient of the residual stream entering the current op
  float* dx2 = scratch + s.dxb;
  float* dln = scratch + s.dln;
  float* dqkv = scratch + s.dqkv;
  float* dao = scratch + s.dao;
  float* dh1 = scratch + s.dh1;
  float* slabs = scratch + s.slabs;
  const float* const* lp = b.params + P_L0 + DGVIT_PARAMS_PER_LAYER * i;
  float* const* lg = b.grads + P_L0 + DGVIT_PARAMS_PER_LAYER * i;
  const float* lb = ws + w.layer0 + w.layer_stride * i;
  const float* xin = i == 0 ? ws + w.x0 : ws + w.layer0 + w.layer_stride * (i - 1) + w.xout;
  const bool last = !dense_last_block(b.cfg) && !d.pool_mean && i == d.L - 1;   // see gemm_layer: only rows b*N carry gradient here
  const int tok = last ? d.B : T, rs = last ? d.N : 1;
  const bool fold = last_block_fold(d, last, ldrop, false, true, lp[L_QKV]);
  // ---- feed-forward branch: xout = fc2(gelu(fc1(ln2))) + xmid
  // (helper-stream kernels are ordered among themselves, so the slab scratch is reused safely; a `join` before
  //  a main-stream kernel that overwrites a buffer makes sure the wgrads that read it have finished)
  // (every weight gradient of the layer writes its split-K slabs into a region of its own; their fixed-order sums and the
  //  two LayerNorm parameter-gradient sums are ONE grouped launch at the end of the layer instead of six)
  ReduceGroup grp;
  reduce_group_init(grp);
  ReduceGroup* gq = g_group_reduce ? &grp : nullptr;   // null: every reduction is launched where it is produced
  // (site 3: the branch sees dx o m / keep; the residual path keeps dx)
  const float* dff = dx;
  if (ldrop) {
    TRY(drop_rows(dx, (long long)rs * d.D, scratch + s.dm3, (long long)rs * d.D, nullptr, 0, tok, d.D, rs, b.site(i, DROP_FF), st));
    dff = scratch + s.dm3;
  }
  TRY(b.fork());
  TRY(wgrad(dff, rs * d.D, lb + w.a1, d.M, lg[L_FC2W], lg[L_FC2B], d.D, d.M, tok, slabs + s.sl_fc2, s.n_fc2, sw, gq));
  {
    GemmParams p = gp(dff, rs * d.D, lp[L_FC2W], d.M, dh1, d.M, tok, d.M, d.D);
    p.aux = lb + w.h1; p.ldaux = d.M;             // (the h1 slot holds gelu'(pre-activation), written by the forward)
    sk.attach(p);
    TRY(gemm_f32(GEMM_NN, g_gelu_grad_store || ldrop ? EPI_DMUL : EPI_DGELU, p, 1, st));   // dh1 = (dx W2) * gelu'(h1)   [previous layer's wgrads joined below]
  }
  TRY(b.fork());
  TRY(wgrad(dh1, d.M, lb + w.ln2, rs * d.D, lg[L_FC1W], lg[L_FC1B], d.M, d.D, tok, slabs + s.sl_fc1, s.n_fc1, sw, gq));
  {
    GemmParams p = gp(dh1, d.M, lp[L_FC1W], d.D, dln, rs * d.D, tok, d.D, d.M);
    sk.attach(p);
    TRY(gemm_f32(GEMM_NN, EPI_STORE, p, 1, st));  // dln2 = dh1 W1
  }
  if (last) TRY(zero_fill(dx2, (long long)sizeof(float) * d.T * d.D, st));   // rows other than b*N get no gradient
  TRY(layernorm_bwd(dln, lb + w.xmid, lb + w.mean2, lb + w.rstd2, lp[L_LN2W], dx, dx2, lg[L_LN2W], lg[L_LN2B], scratch + s.part_ln2, tok, d.D,
                    rs, st, gq));
  // ---- attention branch: xmid = to_out(attn(to_qkv(ln1))) + xin       (dx2 = d xmid)
  if (d.proj) {
    const float* dat = dx2;   // (site 1, as site 3 above)
    if (ldrop) {
      TRY(drop_rows(dx2, (long long)rs * d.D, scratch + s.dm1, (long long)rs * d.D, nullptr, 0, tok, d.D, rs, b.site(i, DROP_OUT), st));
      dat = scratch + s.dm1;
    }
    TRY(b.fork());
    TRY(wgrad(dat, rs * d.D, lb + w.ao, rs * d.I, lg[L_OUTW], lg[L_OUTB], d.D, d.I, tok, slabs + s.sl_out, s.n_out, sw, gq));
    GemmParams p = gp(dat, rs * d.D, lp[L_OUTW], d.I, dao, rs * d.I, tok, d.I, d.D);
    sk.attach(p);
    TRY(gemm_f32(GEMM_NN, EPI_STORE, p, 1, st));  // dao = dxmid Wo
  }
  // (no output projection: the gradient of the attention output is the residual-stream gradient itself, I == D)
  const LayerDrop dr_attn = b.site(i, DROP_ATTN);
  const float* dout = d.proj ? dao : dx2;
  const long long fs_fold = 3ll * d.N * d.I;            // (fold) frame stride of u, r in the qkv slot and of du, dr in dqkv, all behind q / dq
  float* du = dqkv + d.I;
  if (fold)   // dr, du, dq (into the Q columns of dqkv) and EVERY row of dln1 (what dkv W_kv was); W_q^T dq comes on top below
    TRY(goal_attention_bwd_data(lb + w.ln1, lp[L_QKV], dout, (long long)rs * d.I, lb + w.qkv + d.I, fs_fold, lb + w.lse, du,
                                du + (long long)d.H * d.D, fs_fold, dqkv, (long long)rs * 3 * d.I, dln, d.B, d.N, d.H, d.dh, d.D, st));
  else if (d.tiled)
    TRY(attention_bwd_tiled(lb + w.qkv, lb + w.ao, dout, lb + w.lse, dqkv, scratch + s.delta, s.delta_floats, d.B, d.N, d.H,
                            d.dh, last ? 1 : d.N, st, ldrop ? &dr_attn : nullptr));
  else
    TRY(attention_bwd(lb + w.qkv, lb + w.ao, dout, lb + w.lse, dqkv, d.B, d.N, d.H, d.dh, last ? 1 : d.N, st,
                      ldrop ? &dr_attn : nullptr));
  TRY(b.fork());
  if (!last) {
    TRY(wgrad(dqkv, 3 * d.I, lb + w.ln1, d.D, lg[L_QKV], nullptr, 3 * d.I, d.D, T, slabs + s.sl_qkv, s.n_qkv, sw, gq));
    GemmParams p = gp(dqkv, 3 * d.I, lp[L_QKV], d.D, dln, d.D, T, d.D, 3 * d.I);
    sk.attach(p);
    TRY(gemm_f32(GEMM_NN, EPI_STORE, p, 1, st));  // dln1 = dqkv Wqkv
  } else {
    // dWq from the token-0 rows, dWk/dWv from all rows; dln1 = dkv Wkv (+ dq Wq on the token-0 rows)
    const long long nq_slabs = wgrad_scratch(d.I, d.D, tok);
    TRY(wgrad(dqkv, rs * 3 * d.I, lb + w.ln1, rs * d.D, lg[L_QKV], nullptr, d.I, d.D, tok, slabs + s.sl_qkv, nq_slabs, sw, gq));
    float* dwkv = lg[L_QKV] ? lg[L_QKV] + (long long)d.I * d.D : nullptr;
    if (fold) {   // dW_k = sum_b q du^T, dW_v = sum_b do r^T: one launch, straight into rows I..3I (no slabs)
      TRY(goal_attention_wgrad(lb + w.qkv, (long long)rs * 3 * d.I, dout, (long long)rs * d.I, du, fs_fold, lb + w.qkv + d.I + (long long)d.H * d.D,
                               fs_fold, dwkv, d.B, d.H, d.dh, d.D, sw));
    } else {
      TRY(wgrad(dqkv + d.I, 3 * d.I, lb + w.ln1, d.D, dwkv, nullptr, 2 * d.I, d.D, T, slabs + s.sl_qkv + nq_slabs, s.n_qkv - nq_slabs, sw, gq));
      GemmParams kv = gp(dqkv + d.I, 3 * d.I, lp[L_QKV] + (long long)d.I * d.D, d.D, dln, d.D, T, d.D, 2 * d.I);
      sk.attach(kv);
      TRY(gemm_f32(GEMM_NN, EPI_STORE, kv, 1, st));
    }
    GemmParams q = gp(dqkv, rs * 3 * d.I, lp[L_QKV], d.D, dln, rs * d.D, tok, d.D, d.I);
    q.res = dln; q.ldr = rs * d.D;
    sk.attach(q);
    TRY(gemm_f32(GEMM_NN, EPI_STORE, q, 1, st));
  }
  // dx, dh1, dx2 and dqkv are overwritten from here on (this LayerNorm backward and the next layer): wait for the
  // helper stream.  Only this layer's last wgrad (qkv) can still be running; it overlapped the dln1 GEMM above.
  TRY(b.join());
  TRY(layernorm_bwd(dln, xin, lb + w.mean1, lb + w.rstd1, lp[L_LN1W], dx2, dx, lg[L_LN1W], lg[L_LN1B], scratch + s.part_ln1, T, d.D, 1, st, gq));
  // the layer's grouped reduction: behind the weight gradients on the helper stream (it also reads this stream's LayerNorm
  // partials, hence the fork), and the caller's stream waits for it before the slab / partial regions are written again
  TRY(b.fork());
  TRY(reduce_group_flush(grp, sw));
  TRY(b.join());
  if (b.events) TRY(mark_ready(b.events->layer[i], st));    // every gradient of block i is final in stream order
  return DGVIT_OK;
}

}  // namespace

extern "C" int dgvit_got_backward(const dgvit_config* cfg, const float* const* params, float* const* grads, const float* dfeat,
                                  float* dgoal, const float* ws, long long ws_floats, float* scratch, long long scratch_floats,
                                  int batch, float keep, unsigned long long seed, const unsigned long long* seed_dev,
                                  void* stream) {
  return dgvit_got_backward_v2_ev(cfg, params, grads, dfeat, dgoal, ws, ws_floats, scratch, scratch_floats, batch, keep, 1.f, seed, seed_dev,
                                  stream, nullptr);
}

extern "C" int dgvit_got_backward_ev(const dgvit_config* cfg, const float* const* params, float* const* grads, const float* dfeat,
                                     float* dgoal, const float* ws, long long ws_floats, float* scratch, long long scratch_floats,
                                     int batch, float keep, unsigned long long seed, const unsigned long long* seed_dev,
                                     void* stream, const dgvit_grad_events* events) {
  return dgvit_got_backward_v2_ev(cfg, params, grads, dfeat, dgoal, ws, ws_floats, scratch, scratch_floats, batch, keep, 1.f, seed, seed_dev,
                                  stream, events);
}

extern "C" int dgvit_got_backward_v2(const dgvit_config* cfg, const float* const* params, float* const* grads, const float* dfeat,
                                     float* dgoal, const float* ws, long long ws_floats, float* scratch, long long scratch_floats,
                                     int batch, float keep, float lkeep, unsigned long long seed, const unsigned long long* seed_dev,
                                     void* stream) {
  return dgvit_got_backward_v3_ev(cfg, params, grads, dfeat, dgoal, nullptr, ws, ws_floats, scratch, scratch_floats, batch, keep, lkeep, seed,
                                  seed_dev, stream, nullptr);
}

extern "C" int dgvit_got_backward_v2_ev(const dgvit_config* cfg, const float* const* params, float* const* grads, const float* dfeat,
                                        float* dgoal, const float* ws, long long ws_floats, float* scratch, long long scratch_floats,
                                        int batch, float keep, float lkeep, unsigned long long seed, const unsigned long long* seed_dev,
                                        void* stream, const dgvit_grad_events* events) {
  return dgvit_got_backward_v3_ev(cfg, params, grads, dfeat, dgoal, nullptr, ws, ws_floats, scratch, scratch_floats, batch, keep, lkeep, seed,
                                  seed_dev, stream, events);
}

extern "C" int dgvit_got_backward_v3(const dgvit_config* cfg, const float* const* params, float* const* grads, const float* dfeat,
                                     float* dgoal, float* dimg, const float* ws, long long ws_floats, float* scratch, long long scratch_floats,
                                     int batch, float keep, float lkeep, unsigned long long seed, const unsigned long long* seed_dev,
                                     void* stream) {
  return dgvit_got_backward_v3_ev(cfg, params, grads, dfeat, dgoal, dimg, ws, ws_floats, scratch, scratch_floats, batch, keep, lkeep, seed,
                                  seed_dev, stream, nullptr);
}

extern "C" int dgvit_got_backward_v3_ev(const dgvit_config* cfg, const float* const* params, float* const* grads, const float* dfeat,
                                        float* dgoal, float* dimg, const float* ws, long long ws_floats, float* scratch, long long scratch_floats,
                                        int batch, float keep, float lkeep, unsigned long long seed, const unsigned long long* seed_dev,
                                        void* stream, const dgvit_grad_events* events) {
  hipStream_t st = (hipStream_t)stream;
  Bwd b = {cfg, {}, {}, {}, params, grads, ws, scratch, {}, lkeep, lkeep < 1.f, seed, seed_dev, st, st, events};
  const Dims& d = b.d;
  TRY(make_dims(cfg, batch, b.d));
  DGVIT_CHECK_ARG(params && grads && dfeat && ws && scratch, "dgvit_got_backward: null pointer");
  DGVIT_CHECK_ARG(keep > 0.f && keep <= 1.f, "dropout_keep must be in (0, 1]");
  DGVIT_CHECK_ARG(lkeep > 0.f && lkeep <= 1.f, "layer_dropout_keep must be in (0, 1]");
  TRY(check_events(events, cfg->depth));
  b.w = make_ws(d, 1);
  b.s = make_bs(d);
  const Ws& w = b.w;
  const Bs& s = b.s;
  if (ws_floats < w.total) return dgvit_set_error(DGVIT_ERR_WORKSPACE, "backward workspace %lld < %lld floats", ws_floats, w.total);
  if (scratch_floats < s.total) return dgvit_set_error(DGVIT_ERR_WORKSPACE, "backward scratch %lld < %lld floats", scratch_floats, s.total);
  const int np = P_L0 + DGVIT_PARAMS_PER_LAYER * d.L;
  for (int i = 0; i < np; ++i) DGVIT_CHECK_ARG(params[i] || no_projection_slot(d, i), "parameter %d is null", i);   // grads[i] == NULL: frozen parameter, its gradient is skipped
  float* dx = scratch + s.dxa;
  float* dln = scratch + s.dln;
  float* part = scratch + s.part;

  if (s.sk_slab_floats > 0) {
    b.sk.counters = reinterpret_cast<int*>(scratch + s.sk_counters); b.sk.ncounters = (int)s.sk_ncounters;
    b.sk.slabs = scratch + s.sk_slabs; b.sk.slab_cap = s.sk_slab_floats;
    TRY(zero_fill(b.sk.counters, (long long)sizeof(int) * s.sk_ncounters, st));
  }
  if (wgrad_overlap(cfg)) {
    TRY(side_init());
    b.sw = g_side.stream;
    TRY(chain(st, b.sw));   // helper starts after everything already queued by the caller
  }
  const float* xl = ws + w.layer0 + w.layer_stride * (d.L - 1) + w.xout;
  TRY(head_bwd(d, dfeat, xl, ws + w.pooled, params[P_RMS], grads[P_RMS], dx, dln, part, events, st));
  for (int i = d.L - 1; i >= 0; --i) TRY(backward_layer(b, i));
  return token_assembly_bwd(cfg, d, params, grads, dx, dgoal, dimg, dln, ws + w.patches, nullptr, nullptr, part, scratch + s.slabs,
                            s.slabs_floats, keep, seed, seed_dev, st);
}
