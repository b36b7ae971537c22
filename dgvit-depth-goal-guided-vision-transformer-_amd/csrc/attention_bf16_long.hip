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
template <int NW>
__global__ void __launch_bounds__(64 * NW) attn_fwd_bf16_tiled_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                                      float* __restrict__ lse, int N, int H, float scale, int nq) {
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
      if (kt + 2 <= nkt) attn_key_tiles<2>(Ks, Vs, qf, m, l, o, sc, kt, nkt, N, li, h, lane, fsw, t * LK);
      else attn_key_tiles<1>(Ks, Vs, qf, m, l, o, sc, kt, nkt, N, li, h, lane, fsw, t * LK);
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

// ------------------------------------------------------------------------------------ backward (1): dQ, delta
// grid: (B * H) * ceil(N / (32 NW)) workgroups; the arithmetic per (query tile, key tile) is attn_bwd_dq_bf16_kernel's
template <int NW>
__global__ void __launch_bounds__(64 * NW) attn_bwd_dq_bf16_tiled_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ o_fwd,
                                                                         const bf16_t* __restrict__ d_out, const float* __restrict__ lse,
                                                                         bf16_t* __restrict__ dqkv, float* __restrict__ delta, int N,
                                                                         int H, float scale) {
  constexpr int DH = 64, LQ = 32 * NW, STAGE = 2 * TILE + TILE_T;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, h = lane >> 5;
  const int nqb = (N + LQ - 1) / LQ;
  const int item = blockIdx.x / nqb, qb = blockIdx.x % nqb;
  const int b = item / H, hd = item % H;
  const int I = H * DH;
  const long long ld = 3ll * I;
  const bf16_t* base = qkv + (long long)b * N * ld + hd * DH;
  const float sc = scale * DGVIT_LOG2E;
  const int q = qb * LQ + wave * 32 + li, qc = q < N ? q : 0;
  const bool active = qb * LQ + wave * 32 < N;
  const bool fetcher = tid < FETCHERS;
  const int nkt = (N + 31) / 32, ntile = (N + LK - 1) / LK;

  bf16x8 qf[4], dof[4];
  float dl = 0.f;
  {
    bf16x8 of[4];
    load_frags(qf, base + qc * ld, h);
    load_frags(dof, d_out + ((long long)b * N + qc) * I + hd * DH, h);
    load_frags(of, o_fwd + ((long long)b * N + qc) * I + hd * DH, h);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) dl += (float)dof[s][j] * (float)of[s][j];
    dl += __shfl_xor(dl, 32, 64);
  }
  const float lq = lse[((long long)b * H + hd) * N + qc];
  if (active && q < N && h == 0) delta[((long long)b * H + hd) * N + q] = dl;

  TileRegs kr, vr;
  auto fetch = [&](int t) {
    kr.fetch(base + I, ld, t * LK, N, tid);
    vr.fetch(base + 2 * I, ld, t * LK, N, tid);
  };
  auto stash = [&](int t) {
    unsigned char* st = smem + (t & 1) * STAGE;
    kr.stash_rows<false>(st, tid);
    vr.stash_rows<false>(st + TILE, tid);
    kr.stash_transposed(reinterpret_cast<bf16_t*>(st + 2 * TILE), tid);
  };
  if (fetcher) {
    fetch(0);
    stash(0);
  }
  __syncthreads();

  f32x16 dq[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    dq[0][r] = 0.f;
    dq[1][r] = 0.f;
  }
#pragma unroll 1
  for (int t = 0; t < ntile; ++t) {
    if (fetcher && t + 1 < ntile) fetch(t + 1);
    const unsigned char* Ks = smem + (t & 1) * STAGE;
    const unsigned char* Vs = Ks + TILE;
    const bf16_t* Kt = reinterpret_cast<const bf16_t*>(Ks + 2 * TILE);
    if (active) {
#pragma unroll 1
      for (int sub = 0; sub < 2; ++sub) {
        const int kt = 2 * t + sub;
        if (kt >= nkt) break;   // wave-uniform: an odd last tile
        f32x16 s0, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s0[r] = 0.f;
          dp[r] = 0.f;
        }
        mfma_rows(s0, Ks, sub * 32, li, h, qf);
        mfma_rows(dp, Vs, sub * 32, li, h, dof);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kt * 32 + acc_row(r, h);
          const float pr = key < N ? __builtin_amdgcn_exp2f(s0[r] * sc - lq) : 0.f;
          s0[r] = pr * (dp[r] - dl) * scale;   // dS^T
        }
        mfma_transposed(dq, Kt, VS, sub * 32, li, h, s0);
      }
    }
    if (fetcher && t + 1 < ntile) stash(t + 1);
    __syncthreads();
  }
  if (active && q < N) store_T_bf16(dq, dqkv + ((long long)b * N + q) * ld + hd * DH, h, 1.f);
}

// ------------------------------------------------------------------------------------ backward (2): dK, dV
// grid: (B * H) * ceil(N / (32 NW)) workgroups; the arithmetic per (key tile, query tile) is attn_bwd_dkv_bf16_kernel's
template <int NW>
__global__ void __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) attn_bwd_dkv_bf16_tiled_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ d_out,
                                                                          const float* __restrict__ lse, const float* __restrict__ delta,
                                                                          bf16_t* __restrict__ dqkv, int N, int H, float scale) {
  constexpr int DH = 64, LQ = 32 * NW, STAGE = 2 * TILE + 2 * TILE_T + 2 * LK * 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, h = lane >> 5;
  const int nkb = (N + LQ - 1) / LQ;
  const int item = blockIdx.x / nkb, kb = blockIdx.x % nkb;
  const int b = item / H, hd = item % H;
  const int I = H * DH;
  const long long ld = 3ll * I;
  const bf16_t* base = qkv + (long long)b * N * ld + hd * DH;
  const bf16_t* dob = d_out + (long long)b * N * I + hd * DH;
  const float* lbase = lse + ((long long)b * H + hd) * N;
  const float* dbase = delta + ((long long)b * H + hd) * N;
  const float sc = scale * DGVIT_LOG2E;
  const int key = kb * LQ + wave * 32 + li, kc = key < N ? key : 0;
  const bool kvalid = key < N;
  const bool active = kb * LQ + wave * 32 < N;   // wave-uniform: this wave's key tile holds a real key
  const bool fetcher = tid < FETCHERS;
  const int nqt = (N + 31) / 32, ntile = (N + LK - 1) / LK;

  bf16x8 kf[4], vf[4];
  load_frags(kf, base + I + kc * ld, h);
  load_frags(vf, base + 2 * I + kc * ld, h);
  // the row statistics of a query tile travel with its Q / dO rows: the first 64 threads load one each
  TileRegs qr, dor;
  float ls = 0.f, ds = 0.f;
  auto fetch = [&](int t) {
    qr.fetch(base, ld, t * LK, N, tid);
    dor.fetch(dob, (long long)I, t * LK, N, tid);
    if (tid < LK) {
      const int r = t * LK + tid;
      ls = r < N ? lbase[r] : 0.f;
      ds = r < N ? dbase[r] : 0.f;
    }
  };
  auto stash = [&](int t) {
    unsigned char* st = smem + (t & 1) * STAGE;
    qr.stash_rows<false>(st, tid);
    dor.stash_rows<false>(st + TILE, tid);
    qr.stash_transposed(reinterpret_cast<bf16_t*>(st + 2 * TILE), tid);
    dor.stash_transposed(reinterpret_cast<bf16_t*>(st + 2 * TILE + TILE_T), tid);
    if (tid < LK) {
      float* stat = reinterpret_cast<float*>(st + 2 * TILE + 2 * TILE_T);
      stat[tid] = ls;
      stat[LK + tid] = ds;
    }
  };
  if (fetcher) {
    fetch(0);
    stash(0);
  }
  __syncthreads();

  f32x16 dk[2], dv[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    dk[0][r] = 0.f; dk[1][r] = 0.f; dv[0][r] = 0.f; dv[1][r] = 0.f;
  }
#pragma unroll 1
  for (int t = 0; t < ntile; ++t) {
    if (fetcher && t + 1 < ntile) fetch(t + 1);
    const unsigned char* Qs = smem + (t & 1) * STAGE;
    const unsigned char* Os = Qs + TILE;                                     // dO rows
    const bf16_t* Qt = reinterpret_cast<const bf16_t*>(Qs + 2 * TILE);
    const bf16_t* Ot = reinterpret_cast<const bf16_t*>(Qs + 2 * TILE + TILE_T);   // dO transposed
    const float* lse_s = reinterpret_cast<const float*>(Qs + 2 * TILE + 2 * TILE_T);
    const float* del_s = lse_s + LK;
    if (active) {
#pragma unroll 1
      for (int sub = 0; sub < 2; ++sub) {
        const int qt = 2 * t + sub;
        if (qt >= nqt) break;   // wave-uniform: an odd last tile
        f32x16 s0, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s0[r] = 0.f;
          dp[r] = 0.f;
        }
        mfma_rows(s0, Qs, sub * 32, li, h, kf);     // S[query][key]: queries in the registers, key on the lane
        mfma_rows(dp, Os, sub * 32, li, h, vf);     // dP = dO V^T
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int ql = sub * 32 + 8 * g + 4 * h, q0 = t * LK + ql;   // registers 4g .. 4g+3 hold queries q0 .. q0+3
          const fx4 l4 = *reinterpret_cast<const fx4*>(lse_s + ql), d4 = *reinterpret_cast<const fx4*>(del_s + ql);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int r = 4 * g + i;
            const float pr = (kvalid && q0 + i < N) ? __builtin_amdgcn_exp2f(s0[r] * sc - l4[i]) : 0.f;
            s0[r] = pr;                                // P
            dp[r] = pr * (dp[r] - d4[i]) * scale;      // dS
          }
        }
        mfma_transposed(dv, Ot, VS, sub * 32, li, h, s0);   // dV^T += dO^T P
        mfma_transposed(dk, Qt, VS, sub * 32, li, h, dp);   // dK^T += Q^T dS
      }
    }
    if (fetcher && t + 1 < ntile) stash(t + 1);
    __syncthreads();
  }
  if (active && kvalid) {
    store_T_bf16(dk, dqkv + ((long long)b * N + key) * ld + I + hd * DH, h, 1.f);
    store_T_bf16(dv, dqkv + ((long long)b * N + key) * ld + 2 * I + hd * DH, h, 1.f);
  }
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
int launch_fwd(const bf16_t* qkv, bf16_t* out, float* lse, int B, int N, int H, int dh, int nq, hipStream_t st) {
  long long grid;
  TRY(tiled_grid("attention_fwd_bf16_tiled", B, H, nq, 32 * NW, grid));
  const float scale = 1.0f / sqrtf((float)dh);
  {
    ProfileScope t(PROF_ATTN_FWD, 4.0 * (double)nq * N * dh * H * B, st);
    hipLaunchKernelGGL((attn_fwd_bf16_tiled_kernel<NW>), dim3((unsigned)grid), dim3(64 * NW), LDS_FWD, st, qkv, out, lse, N, H, scale, nq);
  }
  DGVIT_CHECK_LAUNCH("attention_fwd_bf16_tiled");
  return DGVIT_OK;
}

template <int NW>
int launch_bwd(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse, bf16_t* dqkv, float* delta, int B, int N, int H,
               int dh, hipStream_t st) {
  long long grid;
  TRY(tiled_grid("attention_bwd_bf16_tiled", B, H, N, 32 * NW, grid));
  TRY(allow_dynamic_lds<attn_bwd_dkv_bf16_tiled_kernel<NW>>(LDS_DKV, "attention_bwd_bf16_tiled"));
  const float scale = 1.0f / sqrtf((float)dh);
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

int attention_fwd_bf16_tiled(const bf16_t* qkv, bf16_t* out, float* lse, int B, int N, int H, int dh, int nq, hipStream_t st) {
  DGVIT_CHECK_ARG(N >= 1, "attention_fwd_bf16_tiled: tokens N=%d must be at least 1", N);
  DGVIT_CHECK_ARG(dh == 64, "attention_fwd_bf16_tiled: dim_head=%d unsupported (64)", dh);
  DGVIT_CHECK_ARG(nq >= 1 && nq <= N, "attention_fwd_bf16_tiled: query rows nq=%d outside [1, %d]", nq, N);
  DGVIT_CHECK_ARG(qkv && out, "attention_fwd_bf16_tiled: null pointer (qkv=%p, out=%p)", (const void*)qkv, (const void*)out);
  DGVIT_CHECK_ARG(B > 0 && H > 0, "attention_fwd_bf16_tiled: batch B=%d and heads H=%d must be positive", B, H);
#ifdef DGVIT_DIAG
  if (g_attn_bf16_tiled_waves == 8) return launch_fwd<8>(qkv, out, lse, B, N, H, dh, nq, st);
  return launch_fwd<4>(qkv, out, lse, B, N, H, dh, nq, st);
#else
  return launch_fwd<g_attn_bf16_tiled_waves>(qkv, out, lse, B, N, H, dh, nq, st);
#endif
}

// dqkv (B, N, 3I) bf16 = gradient of the attention core; delta: B*H*N floats of scratch (written in full: rowsum(dO o O) of every row)
int attention_bwd_bf16_tiled(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse, bf16_t* dqkv, float* delta, int B,
                             int N, int H, int dh, hipStream_t st) {
  DGVIT_CHECK_ARG(N >= 1, "attention_bwd_bf16_tiled: tokens N=%d must be at least 1", N);
  DGVIT_CHECK_ARG(dh == 64, "attention_bwd_bf16_tiled: dim_head=%d unsupported (64)", dh);
  DGVIT_CHECK_ARG(qkv && out && dout && lse && dqkv && delta,
                  "attention_bwd_bf16_tiled: null pointer (qkv=%p, out=%p, dout=%p, lse=%p, dqkv=%p, delta=%p)", (const void*)qkv,
                  (const void*)out, (const void*)dout, (const void*)lse, (const void*)dqkv, (const void*)delta);
  DGVIT_CHECK_ARG(B > 0 && H > 0, "attention_bwd_bf16_tiled: batch B=%d and heads H=%d must be positive", B, H);
#ifdef DGVIT_DIAG
  if (g_attn_bf16_tiled_waves == 8) return launch_bwd<8>(qkv, out, dout, lse, dqkv, delta, B, N, H, dh, st);
  return launch_bwd<4>(qkv, out, dout, lse, dqkv, delta, B, N, H, dh, st);
#else
  return launch_bwd<g_attn_bf16_tiled_waves>(qkv, out, dout, lse, dqkv, delta, B, N, H, dh, st);
#endif
}
