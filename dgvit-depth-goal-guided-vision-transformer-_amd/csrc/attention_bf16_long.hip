// Multi-head self-attention for any token count, bf16 storage / fp32 softmax and accumulation on v_mfma_f32_32x32x16_bf16: K and V
// (in the backward also Q and dO) are streamed through LDS in 64-row tiles instead of being held whole, so N is not bounded by the
// 160 KB LDS (attention_bf16.hip keeps a whole (frame, head) and stops at N = 288).  Layouts, LDS images and the per-tile arithmetic
// are those of attention_bf16.hip (attention_bf16_tiles.h): qkv (B, N, 3*H*64) bf16, out (B, N, H*64) bf16, lse (B, H, N) fp32 in
// base-2 units, scores computed TRANSPOSED so that a lane owns one query.
//
// Workgroup = NW waves = one block of 32 NW rows (queries in the forward and the dQ pass, keys in the dK / dV pass) of one (frame,
// head); the other operand is walked in 64-row tiles through a DOUBLE-BUFFERED pair of LDS stages: the first 256 threads issue the
// global loads of tile t+1 into registers (two rows x 16 bytes per matrix and thread), the waves compute on tile t, the registers go
// to the other stage, one barrier.  A 64-row tile is exactly the key pair (kt, kt+1) that one attn_key_tiles<2> call of the fused
// kernels consumes, with <1> for an odd last tile, in the same order: the arithmetic per query is the fused kernel's.
//   forward  (wave = query tile):  stage = K row image + V row image (read transposed by tr_frag) = 16 KB; only query tiles < nq are
//                                  computed (nq = 1: one wave computes, all of them stage)
//   backward (1) dQ   (wave = query tile):  stage = K rows + V rows + K transposed (64 x 72 elements) = 25 KB; also writes
//                                  delta = rowsum(dO o O) of its rows to the scratch
//            (2) dK/dV (wave = key tile):   stage = Q rows + dO rows + both transposed + the lse / delta slices = 34.5 KB
// Every output element is written by exactly one lane of one workgroup, accumulated in a fixed order: no atomics, deterministic,
// and a frame's results do not depend on the other frames of the batch.  Every global offset is 64-bit.
#include "bf16.h"
#include "kernels.h"
#include "attention_bf16_tiles.h"

namespace {

constexpr int LK = 64;                 // rows of one streamed tile
constexpr int TILE = LK * 128;         // bytes of its row image
constexpr int VS = LK + 8;             // row stride of its transposed image in elements: 144 bytes = 16 x 9 (conflict-free ds_read_b128)
constexpr int TILE_T = 64 * VS * 2;    // bytes of the transposed image
constexpr int FETCHERS = 256;          // threads that move a tile: 32 row pairs x 8 chunks

// One 64-row tile of a 64-wide per-head column block in registers: thread f < 256 holds the 16-byte chunk f & 7 of the rows 2p and
// 2p + 1, p = f >> 3 (the pair that one 32-bit word of the transposed image interleaves).  Rows >= N are zero.
struct TileRegs {
  u32x4_t v0, v1;
  __device__ __forceinline__ void fetch(const bf16_t* src, long long ld, int row0, int N, int tid) {
    const int r = row0 + 2 * (tid >> 3), dc = tid & 7;
    const bool ok0 = r < N, ok1 = r + 1 < N;
    v0 = *reinterpret_cast<const u32x4_t*>(src + (ok0 ? r : 0) * ld + dc * 8);
    v1 = *reinterpret_cast<const u32x4_t*>(src + (ok1 ? r + 1 : 0) * ld + dc * 8);
    if (!ok0) v0 = u32x4_t{0u, 0u, 0u, 0u};
    if (!ok1) v1 = u32x4_t{0u, 0u, 0u, 0u};
  }
  // row image; chunk swizzle (row >> 1) & 7 (ds_read_b128 fragments) or, TR, ((row >> 1) & 1) << 2 (tr_frag).  row >> 1 = p.
  template <bool TR>
  __device__ __forceinline__ void stash_rows(unsigned char* img, int tid) const {
    const int p = tid >> 3, dc = tid & 7, pc = TR ? dc ^ ((p & 1) << 2) : dc ^ (p & 7);
    *reinterpret_cast<u32x4_t*>(img + (2 * p) * 128 + pc * 16) = v0;
    *reinterpret_cast<u32x4_t*>(img + (2 * p + 1) * 128 + pc * 16) = v1;
  }
  __device__ __forceinline__ void stash_transposed(bf16_t* img, int tid) const { put_transposed(img, VS, 2 * (tid >> 3), tid & 7, v0, v1); }
};

// ------------------------------------------------------------------------------------ forward
// grid: (B * H) * ceil(nq / (32 NW)) workgroups, block index = item * nqb + query block
// DROP: the attention-dropout mask on the probabilities that feed P V (attn_key_tiles); l, m and the stored lse stay undropped.  The
// mask row is the absolute query row, so nq = 1 draws the bits of the dense call's row 0.
template <int NW, bool DROP>
__device__ __forceinline__ void attn_fwd_bf16_tiled_body(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, float* __restrict__ lse, int N,
                                                         int H, float scale, int nq, const LayerDrop& drop) {
  constexpr int DH = 64, LQ = 32 * NW, STAGE = 2 * TILE;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, h = lane >> 5;
  const int nqb = (nq + LQ - 1) / LQ;
  const int item = blockIdx.x / nqb, qb = blockIdx.x % nqb;
  const int b = item / H, hd = item % H;
  const int I = H * DH;
  const long long ld = 3ll * I;
  const bf16_t* base = qkv + (long long)b * N * ld + hd * DH;
  const float sc = scale * DGVIT_LOG2E;
  const int q = qb * LQ + wave * 32 + li;
  const bool active = qb * LQ + wave * 32 < nq;   // wave-uniform: this wave's query tile holds a needed row
  const bool fetcher = tid < FETCHERS;            // wave-uniform
  const int nkt = (N + 31) / 32, ntile = (N + LK - 1) / LK;
  const unsigned fsw = (unsigned)((li >> 1) & 7);

  bf16x8 qf[4];
  load_frags(qf, base + (long long)(q < nq ? q : 0) * ld, h);
  RowDrop rd = {};
  if constexpr (DROP)
    rd = RowDrop{(((long long)b * H + hd) * N + (q < nq ? q : 0)) * ((N + 3) / 4), drop_seed(drop), drop.tag, drop.keep, 1.0f / drop.keep};
  TileRegs kr, vr;
  if (fetcher) {
    kr.fetch(base + I, ld, 0, N, tid);
    vr.fetch(base + 2 * I, ld, 0, N, tid);
    kr.stash_rows<false>(smem, tid);
    vr.stash_rows<true>(smem + TILE, tid);
  }
  __syncthreads();

  float m = -INFINITY, l = 0.f;
  f32x16 o[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    o[0][r] = 0.f;
    o[1][r] = 0.f;
  }
#pragma unroll 1
  for (int t = 0; t < ntile; ++t) {
    if (fetcher && t + 1 < ntile) {   // in flight during the compute below
      kr.fetch(base + I, ld, (t + 1) * LK, N, tid);
      vr.fetch(base + 2 * I, ld, (t + 1) * LK, N, tid);
    }
    const unsigned char* Ks = smem + (t & 1) * STAGE;
    const unsigned char* Vs = Ks + TILE;
    if (active) {
      const int kt = 2 * t;
      if (kt + 2 <= nkt) attn_key_tiles<2, DROP>(Ks, Vs, qf, m, l, o, sc, kt, nkt, N, li, h, lane, fsw, t * LK, &rd);
      else attn_key_tiles<1, DROP>(Ks, Vs, qf, m, l, o, sc, kt, nkt, N, li, h, lane, fsw, t * LK, &rd);
    }
    if (fetcher && t + 1 < ntile) {
      unsigned char* nxt = smem + ((t + 1) & 1) * STAGE;   // last read in trip t - 1, before the barrier that ended it
      kr.stash_rows<false>(nxt, tid);
      vr.stash_rows<true>(nxt + TILE, tid);
    }
    __syncthreads();
  }
  if (active && q < nq) {
    store_T_bf16(o, out + ((long long)b * N + q) * I + hd * DH, h, 1.f / l);
    if (lse && h == 0) lse[((long long)b * H + hd) * N + q] = m + __builtin_amdgcn_logf(l);   // base-2 log-sum-exp
  }
}
template <int NW>
__global__ void __launch_bounds__(64 * NW) attn_fwd_bf16_tiled_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                                      float* __restrict__ lse, int N, int H, float scale, int nq) {
  attn_fwd_bf16_tiled_body<NW, false>(qkv, out, lse, N, H, scale, nq, LayerDrop{});
}
template <int NW>
__global__ void __launch_bounds__(64 * NW) attn_fwd_bf16_tiled_drop_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                                           float* __restrict__ lse, int N, int H, float scale, int nq,
                                                                           const LayerDrop drop) {
  attn_fwd_bf16_tiled_body<NW, true>(qkv, out, lse, N, H, scale, nq, drop);
}

// ------------------------------------------------------------------------------------ backward (1): dQ, delta
// grid: (B * H) * ceil(N / (32 NW)) workgroups; the arithmetic per (query tile, key tile) is attn_bwd_dq_bf16_kernel's
// DROP: dS = P o (mask / keep o dP - delta) scale; the register layout is the forward's (one Philox block per four registers), and
// delta = rowsum(dO o O) needs no mask: O is the dropped output.
template <int NW>
__global__ void __launch_bounds__(64 * NW) attn_bwd_dq_bf16_tiled_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ o_fwd,
                                                                         const bf16_t* __restrict__ d_out, const float* __restrict__ lse,
                                                                         bf16_t* __restrict__ dqkv, float* __restrict__ delta, int N,
                                                                         int H, float scale) {
  constexpr bool DROP = false;
  const LayerDrop drop = {};
#include "attention_bf16_dq_body.h"
}
template <int NW>
__global__ void __launch_bounds__(64 * NW) attn_bwd_dq_bf16_tiled_drop_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ o_fwd,
                                                                              const bf16_t* __restrict__ d_out, const float* __restrict__ lse,
                                                                              bf16_t* __restrict__ dqkv, float* __restrict__ delta, int N,
                                                                              int H, float scale, const LayerDrop drop) {
  constexpr bool DROP = true;
#include "attention_bf16_dq_body.h"
}

// ------------------------------------------------------------------------------------ backward (2): dK, dV
// grid: (B * H) * ceil(N / (32 NW)) workgroups; the arithmetic per (key tile, query tile) is attn_bwd_dkv_bf16_kernel's
// DROP: dV += dO^T (P o mask / keep), dS as in the dQ kernel.  Here the key sits on the lane and the queries in the registers, so every
// register is another mask row; the four lanes of a quad (keys 4j .. 4j+3) share the Philox blocks of four queries between them.
template <int NW>
__global__ void __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) attn_bwd_dkv_bf16_tiled_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ d_out,
                                                                          const float* __restrict__ lse, const float* __restrict__ delta,
                                                                          bf16_t* __restrict__ dqkv, int N, int H, float scale) {
  constexpr bool DROP = false;
  const LayerDrop drop = {};
#include "attention_bf16_dkv_body.h"
}
template <int NW>
__global__ void __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) attn_bwd_dkv_bf16_tiled_drop_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ d_out,
                                                                               const float* __restrict__ lse, const float* __restrict__ delta,
                                                                               bf16_t* __restrict__ dqkv, int N, int H, float scale,
                                                                               const LayerDrop drop) {
  constexpr bool DROP = true;
#include "attention_bf16_dkv_body.h"
}

constexpr int LDS_FWD = 2 * (2 * TILE);                             // 32 KB
constexpr int LDS_DQ = 2 * (2 * TILE + TILE_T);                     // 50 KB
constexpr int LDS_DKV = 2 * (2 * TILE + 2 * TILE_T + 2 * LK * 4);   // 69 KB: above the default 64 KB limit

// workgroups of a launch: a grid of 2^31 or more is refused
int tiled_grid(const char* what, int B, int H, int rows, int block, long long& grid) {
  grid = (long long)B * H * ((rows + block - 1) / block);
  DGVIT_CHECK_ARG(grid < (1ll << 31), "%s: B*H*blocks = %lld workgroups, the limit is 2^31 - 1", what, grid);
  return DGVIT_OK;
}

template <int NW>
int launch_fwd(const bf16_t* qkv, bf16_t* out, float* lse, int B, int N, int H, int dh, int nq, const LayerDrop* drop, hipStream_t st) {
  long long grid;
  TRY(tiled_grid("attention_fwd_bf16_tiled", B, H, nq, 32 * NW, grid));
  const float scale = 1.0f / sqrtf((float)dh);
  {
    ProfileScope t(PROF_ATTN_FWD, 4.0 * (double)nq * N * dh * H * B, st);
    if (drop)
      hipLaunchKernelGGL((attn_fwd_bf16_tiled_drop_kernel<NW>), dim3((unsigned)grid), dim3(64 * NW), LDS_FWD, st, qkv, out, lse, N, H, scale, nq, *drop);
    else
      hipLaunchKernelGGL((attn_fwd_bf16_tiled_kernel<NW>), dim3((unsigned)grid), dim3(64 * NW), LDS_FWD, st, qkv, out, lse, N, H, scale, nq);
  }
  DGVIT_CHECK_LAUNCH("attention_fwd_bf16_tiled");
  return DGVIT_OK;
}

template <int NW>
int launch_bwd(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse, bf16_t* dqkv, float* delta, int B, int N, int H,
               int dh, const LayerDrop* drop, hipStream_t st) {
  long long grid;
  TRY(tiled_grid("attention_bwd_bf16_tiled", B, H, N, 32 * NW, grid));
  const float scale = 1.0f / sqrtf((float)dh);
  if (drop) {
    TRY(allow_dynamic_lds<attn_bwd_dkv_bf16_tiled_drop_kernel<NW>>(LDS_DKV, "attention_bwd_bf16_tiled_drop"));
    {
      ProfileScope t(PROF_ATTN_BWD, 10.0 * (double)N * N * dh * H * B, st);
      hipLaunchKernelGGL((attn_bwd_dq_bf16_tiled_drop_kernel<NW>), dim3((unsigned)grid), dim3(64 * NW), LDS_DQ, st, qkv, out, dout, lse, dqkv, delta,
                         N, H, scale, *drop);
      hipLaunchKernelGGL((attn_bwd_dkv_bf16_tiled_drop_kernel<NW>), dim3((unsigned)grid), dim3(64 * NW), LDS_DKV, st, qkv, dout, lse,
                         (const float*)delta, dqkv, N, H, scale, *drop);
    }
    DGVIT_CHECK_LAUNCH("attention_bwd_bf16_tiled_drop");
    return DGVIT_OK;
  }
  TRY(allow_dynamic_lds<attn_bwd_dkv_bf16_tiled_kernel<NW>>(LDS_DKV, "attention_bwd_bf16_tiled"));
  {
    ProfileScope t(PROF_ATTN_BWD, 10.0 * (double)N * N * dh * H * B, st);   // 2.5 x forward
    hipLaunchKernelGGL((attn_bwd_dq_bf16_tiled_kernel<NW>), dim3((unsigned)grid), dim3(64 * NW), LDS_DQ, st, qkv, out, dout, lse, dqkv, delta, N, H,
                       scale);
    hipLaunchKernelGGL((attn_bwd_dkv_bf16_tiled_kernel<NW>), dim3((unsigned)grid), dim3(64 * NW), LDS_DKV, st, qkv, dout, lse, (const float*)delta,
                       dqkv, N, H, scale);
  }
  DGVIT_CHECK_LAUNCH("attention_bwd_bf16_tiled");
  return DGVIT_OK;
}

}  // namespace

namespace {
int fwd_tiled(const bf16_t* qkv, bf16_t* out, float* lse, int B, int N, int H, int dh, int nq, const LayerDrop* drop, hipStream_t st) {
  DGVIT_CHECK_ARG(N >= 1, "attention_fwd_bf16_tiled: tokens N=%d must be at least 1", N);
  DGVIT_CHECK_ARG(dh == 64, "attention_fwd_bf16_tiled: dim_head=%d unsupported (64)", dh);
  DGVIT_CHECK_ARG(nq >= 1 && nq <= N, "attention_fwd_bf16_tiled: query rows nq=%d outside [1, %d]", nq, N);
  DGVIT_CHECK_ARG(qkv && out, "attention_fwd_bf16_tiled: null pointer (qkv=%p, out=%p)", (const void*)qkv, (const void*)out);
  DGVIT_CHECK_ARG(B > 0 && H > 0, "attention_fwd_bf16_tiled: batch B=%d and heads H=%d must be positive", B, H);
#ifdef DGVIT_DIAG
  if (g_attn_bf16_tiled_waves == 8) return launch_fwd<8>(qkv, out, lse, B, N, H, dh, nq, drop, st);
  return launch_fwd<4>(qkv, out, lse, B, N, H, dh, nq, drop, st);
#else
  return launch_fwd<g_attn_bf16_tiled_waves>(qkv, out, lse, B, N, H, dh, nq, drop, st);
#endif
}
int check_drop(const char* what, const LayerDrop& drop) {
  DGVIT_CHECK_ARG(drop.keep > 0.f && drop.keep <= 1.f, "%s: keep=%g must be in (0, 1]", what, (double)drop.keep);
  return DGVIT_OK;
}
}  // namespace

int attention_fwd_bf16_tiled(const bf16_t* qkv, bf16_t* out, float* lse, int B, int N, int H, int dh, int nq, hipStream_t st) {
  return fwd_tiled(qkv, out, lse, B, N, H, dh, nq, nullptr, st);
}
int attention_fwd_bf16_tiled_drop(const bf16_t* qkv, bf16_t* out, float* lse, int B, int N, int H, int dh, int nq, const LayerDrop& drop,
                                  hipStream_t st) {
  TRY(check_drop("attention_fwd_bf16_tiled_drop", drop));
  return fwd_tiled(qkv, out, lse, B, N, H, dh, nq, drop.keep < 1.f ? &drop : nullptr, st);
}

// dqkv (B, N, 3I) bf16 = gradient of the attention core; delta: B*H*N floats of scratch (written in full: rowsum(dO o O) of every row)
namespace {
int bwd_tiled(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse, bf16_t* dqkv, float* delta, int B, int N, int H, int dh,
              const LayerDrop* drop, hipStream_t st) {
  DGVIT_CHECK_ARG(N >= 1, "attention_bwd_bf16_tiled: tokens N=%d must be at least 1", N);
  DGVIT_CHECK_ARG(dh == 64, "attention_bwd_bf16_tiled: dim_head=%d unsupported (64)", dh);
  DGVIT_CHECK_ARG(qkv && out && dout && lse && dqkv && delta,
                  "attention_bwd_bf16_tiled: null pointer (qkv=%p, out=%p, dout=%p, lse=%p, dqkv=%p, delta=%p)", (const void*)qkv,
                  (const void*)out, (const void*)dout, (const void*)lse, (const void*)dqkv, (const void*)delta);
  DGVIT_CHECK_ARG(B > 0 && H > 0, "attention_bwd_bf16_tiled: batch B=%d and heads H=%d must be positive", B, H);
#ifdef DGVIT_DIAG
  if (g_attn_bf16_tiled_waves == 8) return launch_bwd<8>(qkv, out, dout, lse, dqkv, delta, B, N, H, dh, drop, st);
  return launch_bwd<4>(qkv, out, dout, lse, dqkv, delta, B, N, H, dh, drop, st);
#else
  return launch_bwd<g_attn_bf16_tiled_waves>(qkv, out, dout, lse, dqkv, delta, B, N, H, dh, drop, st);
#endif
}
}  // namespace

int attention_bwd_bf16_tiled(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse, bf16_t* dqkv, float* delta, int B,
                             int N, int H, int dh, hipStream_t st) {
  return bwd_tiled(qkv, out, dout, lse, dqkv, delta, B, N, H, dh, nullptr, st);
}
int attention_bwd_bf16_tiled_drop(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse, bf16_t* dqkv, float* delta,
                                  int B, int N, int H, int dh, const LayerDrop& drop, hipStream_t st) {
  TRY(check_drop("attention_bwd_bf16_tiled_drop", drop));
  return bwd_tiled(qkv, out, dout, lse, dqkv, delta, B, N, H, dh, drop.keep < 1.f ? &drop : nullptr, st);
}
