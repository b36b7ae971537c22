// fp32 GEMM on the gfx950 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 in, fp32 accumulate).
//
// This is the dominant kernel of the DGViT hot path: every Linear of the encoder
// (GoalFormer.py:43,46,64,67,139 and the head Linears of got_sac_network.py) and both of its
// gradients run through it.  One kernel template covers the three operand layouts
//   NT  Y  = X W^T      (forward)         A k-contiguous, B k-contiguous
//   NN  dX = dY W       (data gradient)   A k-contiguous, B n-contiguous
//   TN  dW = dY^T X     (weight gradient) A m-contiguous, B n-contiguous, split over K = tokens
// without any transposed copy in HBM:
//   * a k-contiguous operand is staged as LDS[row][BK+4] and read back with one ds_read_b128 per
//     32-row MFMA tile and 8-deep k-group (lane (i, h) takes k = 8g + 4h .. +3; the +4 pad makes the
//     16-lane b128 groups hit 16 distinct 16-byte bank slots);
//   * an m/n-contiguous operand is staged as LDS[k][R+4]; a wave's 32-row MFMA tiles are interleaved over its rows (frag_mc) so
//     that one ds_read_b64 per k-row feeds two tiles (256 B/clk; ds_read_b32 runs at 128 B/clk and made the TN / NN forms
//     12 % / 6 % slower than NT on large problems);
//   both read paths feed MFMA step s of k-group g with k = 8g + 4h + s, so the contraction order is the
//   same permutation for A and B whatever their layouts.
// Global->LDS staging is register-staged and double-buffered in LDS: tile t+1 is fetched to VGPRs
// before the MFMAs of tile t issue and written to the other LDS buffer after them (one barrier per
// k-tile).  Four waves (2x2) per workgroup, each owning a (BM/2)x(BN/2) block of 32x32 accumulators.
// Epilogue: the accumulators (column on the lane, rows in registers) are transposed through the now idle
// staging LDS so that every global access of the epilogue -- C, residual, GELU input/output -- is a
// 16-byte-per-lane, 512-byte-per-row coalesced float4; bias / residual / GELU / GELU' / ReLU are applied
// on the way out.  The weight-gradient form also sums its A tiles over k (= the bias gradient) for free.
// In other files: the tile primitives (TileCfg, Fetch, frag / frag_mc, sched_pattern) in gemm_tile.h, the diagnostic-only pipelined
// persistent kernel in gemm_pipe.h, the slab reductions that follow the split-K weight gradients in gemm_reduce.hip.
#include <algorithm>

#include "common.h"
#include "gemm_tile.h"

namespace {

// diagnostic stamps (dgvit_set_gemm_stamps): wave 0 of every workgroup records the shader clock at four points and where it ran
__device__ __forceinline__ void stamp(const GemmParams& p, int slot, int tid) {
#ifdef DGVIT_DIAG
  if (p.stamps && tid == 0 && (int)blockIdx.x < p.stamp_capacity) {
    long long* s = p.stamps + (long long)blockIdx.x * 16;
    s[slot] = __builtin_readcyclecounter();
    if (slot == 0) {
      s[4] = wall_clock64();
      s[5] = (long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);   // HW_ID, XCC_ID
    }
    if (slot == 3) s[6] = wall_clock64();
  }
#endif
}
// timing / A-B diagnostics of the per-tile kernel exist in the diagnostic build only (knobs.h)
#ifdef DGVIT_DIAG
#define DIAG_BIT(p, b) ((p).diag & (b))
#define DIAG_STAMPS(p) ((p).stamps != nullptr)
#else
#define DIAG_BIT(p, b) 0
#define DIAG_STAMPS(p) false
#endif

// EPI_UNPATCH: image offset of element (m, k) of the (B * P, ph * pw) patch matrix -- the address the patch gather (Fetch::plan_gather) reads
// it from, so the store is that loader's inverse.  Patches do not overlap: every pixel is written exactly once, no atomics.
__device__ __forceinline__ long long unpatch_off(const GemmParams& p, int m, int k) {
  const int b = m / p.g_P, pi = m - b * p.g_P, py = pi / p.g_gw, px = pi - py * p.g_gw;
  const int i = k / p.g_pw, j = k - i * p.g_pw;
  return (long long)b * p.g_hw + (long long)(py * p.g_ph + i) * p.g_wi + px * p.g_pw + j;
}

template <class T, int LAYOUT, int VEC, int EPI, bool GATHER = false>
__global__ void __launch_bounds__(T::NT, T::MINB) gemm_f32_kernel(const GemmParams p) {
  constexpr int BM = T::BM, BN = T::BN, BK = T::BK, NT = T::NT;
  constexpr bool AKC = LAYOUT != GEMM_TN;
  constexpr bool BKC = LAYOUT == GEMM_NT;
  // EPI_GELU2D / EPI_DMUL: the training forward stores gelu'(pre-activation) INSTEAD of the pre-activation (C) beside gelu (C2) -- the
  // erf form already holds exp(-x^2 / 2), the derivative costs two more FMAs there -- and the data-gradient GEMM multiplies by that
  // stored factor instead of evaluating erf and exp per element in its epilogue (same values, bit for bit)
  constexpr bool TWO_OUT = EPI == EPI_GELU2 || EPI == EPI_GELU2D;
  constexpr bool ACT_GRAD = EPI == EPI_DGELU || EPI == EPI_DMUL;
  // Direct-epilogue output stores of the two-output forward (fc1: gelu + gelu') and of the gelu'-scaled data gradient are NON-TEMPORAL: 10 MB
  // of output per round of tiles streamed through each 4 MB L2 and evicted the A panels the column tiles share -- fc1 forward read 121.6 MB per
  // launch for 28 MB of operands, the fc2 data gradient 346 for 238 (rocprofv3 FETCH_SIZE by launch, profiles/r04_g_gemm_traffic_by_launch.txt);
  // with aux 2 (no L2 allocation) 43.2 and 263.5 MB.  Step time unchanged (12.52 vs 12.53 ms interleaved with the bit on every direct epilogue).
  constexpr bool NT_STORES = TWO_OUT || ACT_GRAD;
  constexpr int WM = BM / T::WVM, WN = BN / T::WVN, TM = WM / 32, TN = WN / 32;
  static_assert(WM % 32 == 0 && WN % 32 == 0 && BM <= NT, "bad wave layout");
  constexpr int A_TILE = AKC ? BM * (BK + 4) : BK * (BM + 4);
  constexpr int B_TILE = BKC ? BN * (BK + 4) : BK * (BN + 4);
  constexpr int STAGE = A_TILE + B_TILE;
  using FA = Fetch<BM, BK, AKC, VEC, NT, GATHER>;
  using FB = Fetch<BN, BK, BKC, VEC, NT>;

  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, h = lane >> 5;
  const int wm = wave / T::WVN, wn = wave % T::WVN;

  const int tiles_n = (p.N + BN - 1) / BN, tiles_m = (p.M + BM - 1) / BM;
  // In-launch split-K (forward / data-gradient forms): tiles >= p.split_from are cut into p.nsplit k-slices, one workgroup
  // each; the slices leave fp32 partial tiles in `p.slabs`, draw a ticket from the tile's counter, and the LAST arriver sums
  // the slices in slice order (deterministic) and runs the normal epilogue.  Two uses: GEMMs with far fewer tiles than the
  // chip has workgroup slots (small batches: T = 65 ... 2080 rows, K = 2048), and the last partial round of a large grid
  // (25600 x 256 outputs = 1600 tiles = 6.25 per CU: the 64 left-over tiles become 256 quarter-tiles).
  int tile, zs = 0, nz = 1;
  // Weight gradients (EPI_SPLITK): (tile, k-slice) pairs in ONE grid dimension, k-slice major, each XCD a contiguous chunk of that order.
  // An XCD then works on a few k-slices of EVERY output tile: the rows of dY and X in those slices are read once, by the one L2 that serves
  // all their tiles.  (Round 1-3 gave an XCD a few tiles and ALL their k-slices -- grid (tiles, 1, slices), XCD = blockIdx.x % 8: every XCD
  // streamed the whole of X, and the tiles sharing a dY block sat on one XCD but in different slices' dispatch order: 532 MB read per
  // fc1 / fc2 weight-gradient launch for 236 MB of operands, rocprofv3 FETCH_SIZE by launch, profiles/r04_g_gemm_traffic_by_launch.txt.)
  int zslice = blockIdx.z;
  if (EPI == EPI_SPLITK && p.zsplit > 1) {
    const int ntile = tiles_m * tiles_n, w = xcd_remap(blockIdx.x, ntile * p.zsplit);
    zslice = w / ntile;
    tile = w - zslice * ntile;
  } else if (EPI != EPI_SPLITK && p.nsplit > 1 && (int)blockIdx.x >= p.split_from) {
    const int r = (int)blockIdx.x - p.split_from;
    tile = p.split_from + r / p.nsplit;
    zs = r % p.nsplit;
    nz = p.nsplit;
  } else {
    tile = xcd_remap(blockIdx.x, EPI != EPI_SPLITK && p.nsplit > 1 ? p.split_from : tiles_m * tiles_n);
  }
  const int m0 = (tile / tiles_n) * BM, n0 = (tile % tiles_n) * BN;
  const int kbeg = nz > 1 ? zs * p.kchunk_split : zslice * p.kchunk;
  const int kend = min(p.K, kbeg + (nz > 1 ? p.kchunk_split : p.kchunk));
  const int nk = kend > kbeg ? (kend - kbeg + BK - 1) / BK : 0;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float bsum = 0.f;  // TN only: column sum of this block's A rows (bias gradient), threads < BM of n-tile 0
  const bool do_colsum = EPI == EPI_SPLITK && p.colsum && n0 == 0 && tid < BM;

  float4 ra[FA::NV], rb[FB::NV];
  const int klim = kend - kbeg;
  stamp(p, 0, tid);

  // epilogue geometry: accumulator (col = lane&31, row = (r&3) + 8*(r>>2) + 4*h) -> LDS C image [rows][BN+4] -> float4 row pieces
  // Only ONE tile carries the rarely used epilogue forms, so that they do not inflate (and push into scratch memory) every other
  // instantiation: the element-wise path for outputs that cannot take float4 accesses (odd N / ldc, unaligned C: the host sends
  // those to 64 x 64 x 32, pick_tile) and the fused LayerNorm of a 64-wide output row.
  constexpr bool ELEMWISE = BM == 64 && BN == 64 && BK == 32;
  constexpr bool LN_OK = EPI == EPI_STORE && BN == 64 && VEC == 4 && !GATHER && LAYOUT != GEMM_TN;
  const bool evec = !ELEMWISE || p.evec;
  constexpr int CS = BN + 4;
  constexpr int NCHUNK = (BM * CS <= 2 * STAGE) ? 1 : T::WVM;   // whole tile at once, or one wave-row of the tile at a time
  constexpr int CROWS = BM / NCHUNK;
  static_assert(CROWS * CS <= 2 * STAGE && (NCHUNK == 1 || CROWS == WM), "epilogue C image does not fit the staging LDS");
  constexpr int C4 = BN / 4, RPP = NT / C4;
  const int cc = (tid % C4) * 4, rr0 = tid / C4;
  const int n = n0 + cc;
  // The bias row piece is fetched BEFORE the main loop (4 registers): at the epilogue it would be a dependent round trip of
  // several thousand cycles under load, paid by every tile.
  // which epilogue (uniform over the launch except for split tiles): see "direct epilogue" below
  constexpr bool DIRECT_OK = LAYOUT != GEMM_TN && VEC == 4 && !GATHER && EPI != EPI_SPLITK && EPI != EPI_UNPATCH && (BKC || TN <= 2);
  const bool direct = DIRECT_OK && nz == 1 && evec && p.c_rgrp == 0 && p.res_mod == 0 && (!TWO_OUT || p.ldc2 == p.ldc) && !DIAG_BIT(p, 8) &&
                      !(LN_OK && p.ln_y);   // (the fused LayerNorm reduces over the 16 lanes that hold a row of the LDS image)
  int dcol[TN];     // direct epilogue: this lane's column(s) inside the tile
  float dbias[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    dcol[j] = wn * WN + (BKC ? j * 32 + li : li * TN + j);
    dbias[j] = 0.f;
  }
  float bias4[4] = {0.f, 0.f, 0.f, 0.f};
  if ((EPI == EPI_STORE || TWO_OUT || EPI == EPI_RELU || EPI == EPI_GELU) && p.bias) {
    if (direct) {
#pragma unroll
      for (int j = 0; j < TN; ++j) dbias[j] = p.bias[min(n0 + dcol[j], p.N - 1)];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (n + e < p.N) bias4[e] = p.bias[n + e];
    }
  }

  // LDS -> fragments of one 8-deep k-group; MFMAs of one k-group
  auto load_frags = [&](float (&fa)[TM][4], float (&fb)[TN][4], const float* la, const float* lb, int g) {
    if constexpr (AKC) {
#pragma unroll
      for (int i = 0; i < TM; ++i) frag<BM, BK, true>(fa[i], la, wm * WM + i * 32 + li, g, h);
    } else {
      frag_mc<BM, TM>(fa, la, wm * WM, li, g, h);
    }
    if constexpr (BKC) {
#pragma unroll
      for (int j = 0; j < TN; ++j) frag<BN, BK, true>(fb[j], lb, wn * WN + j * 32 + li, g, h);
    } else {
      frag_mc<BN, TN>(fb, lb, wn * WN, li, g, h);
    }
  };
  auto do_mfma = [&](const float (&fa)[TM][4], const float (&fb)[TN][4]) {
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][s4], fb[j][s4], acc[i][j], 0, 0, 0);
  };
  auto mma_group = [&](const float* la, const float* lb, int g) {
    float fa[TM][4], fb[TN][4];
    load_frags(fa, fb, la, lb, g);
    do_mfma(fa, fb);
  };

  if (VEC == 4) {
    // Software pipeline (2 LDS buffers, 1 register set, 1 barrier per k-tile):
    //   iteration t:  LDS[t+1] <- registers (tile t+1, fetched during iteration t-1)
    //                 registers <- global tile t+2         (in flight for a whole iteration)
    //                 MFMAs on LDS[t]
    // the fetch is branch-free (hardware range check), so loads, LDS writes and MFMAs share one basic block.
    typename FA::Plan pa;
    typename FB::Plan pb;
    if constexpr (GATHER) FA::plan_gather(pa, p, m0, kbeg, tid);
    else FA::plan(pa, p.A, p.lda, m0, p.M, kbeg, p.K, tid);
    FB::plan(pb, p.B, p.ldb, n0, p.N, kbeg, p.K, tid);
    // prologue: the fetches of k-tiles 0 AND 1 are in flight together (one exposed round trip per output tile instead of two;
    // with K = 256 a tile has only 8-16 k-tiles to amortise it over)
    {
      float4 ra0[FA::NV], rb0[FB::NV];
      FA::run4(ra0, pa, 0, klim);
      FB::run4(rb0, pb, 0, klim);
      FA::run4(ra, pa, 1, klim);
      FB::run4(rb, pb, 1, klim);
      FA::stash(ra0, smem, tid);
      FB::stash(rb0, smem + A_TILE, tid);
    }
    __syncthreads();
    stamp(p, 1, tid);
    if (DIAG_BIT(p, 1)) __builtin_amdgcn_s_setprio(2);   // A/B knob: main-loop waves ahead of the prologue / epilogue waves they share a SIMD with
    for (int kt = 0; kt < nk; ++kt) {
      const float* la = smem + (kt & 1) * STAGE;
      const float* lb = la + A_TILE;
      float* wa = smem + ((kt + 1) & 1) * STAGE;
      // program order = wanted issue order where LDS reads and writes may alias for the compiler:
      // fragments of k-group 0, then the next tile's LDS writes, then the k-groups (each prefetching the next)
      float fa[2][TM][4], fb[2][TN][4];
      load_frags(fa[0], fb[0], la, lb, 0);
      FA::stash(ra, wa, tid);
      FB::stash(rb, wa + A_TILE, tid);
      FA::run4(ra, pa, kt + 2, klim);
      FB::run4(rb, pb, kt + 2, klim);
#pragma unroll
      for (int g = 0; g < BK / 8; ++g) {
        if (g + 1 < BK / 8) load_frags(fa[(g + 1) & 1], fb[(g + 1) & 1], la, lb, g + 1);
        do_mfma(fa[g & 1], fb[g & 1]);
      }
      sched_pattern<4 * TM * TN, FA::NV + FB::NV, (AKC ? TM : (TM == 1 ? 2 : 4)) + (BKC ? TN : (TN == 1 ? 2 : 4)), BK / 8>();
      if (EPI == EPI_SPLITK && do_colsum) {
#pragma unroll 8
        for (int kk = 0; kk < BK; ++kk) bsum += la[kk * (BM + 4) + tid];
      }
      __syncthreads();
    }
    if (DIAG_BIT(p, 1)) __builtin_amdgcn_s_setprio(0);
  } else {
    FA::run(ra, p.A, p.lda, m0, p.M, kbeg, kend, tid);
    FB::run(rb, p.B, p.ldb, n0, p.N, kbeg, kend, tid);
    FA::stash(ra, smem, tid);
    FB::stash(rb, smem + A_TILE, tid);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const float* la = smem + (kt & 1) * STAGE;
      const float* lb = la + A_TILE;
      const bool more = kt + 1 < nk;
      if (more) {
        FA::run(ra, p.A, p.lda, m0, p.M, kbeg + (kt + 1) * BK, kend, tid);
        FB::run(rb, p.B, p.ldb, n0, p.N, kbeg + (kt + 1) * BK, kend, tid);
      }
#pragma unroll
      for (int g = 0; g < BK / 8; ++g) mma_group(la, lb, g);
      if (EPI == EPI_SPLITK && do_colsum) {
#pragma unroll 8
        for (int kk = 0; kk < BK; ++kk) bsum += la[kk * (BM + 4) + tid];
      }
      if (more) {
        float* wa = smem + ((kt + 1) & 1) * STAGE;
        FA::stash(ra, wa, tid);
        FB::stash(rb, wa + A_TILE, tid);
      }
      __syncthreads();
    }
  }

  stamp(p, 2, tid);
  if (DIAG_BIT(p, 2)) {   // diagnostic (dgvit_set_gemm_diagnostics(2)): main loop only - what would a free epilogue be worth?
    float sacc = 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc += acc[i][j][r];
    if (sacc == 1.2345678e33f) p.C[0] = sacc;
    return;
  }
  // ---- direct epilogue (NT / NN forms, whole-K tiles, vector-aligned outputs, plain row mapping) ---------------------------------
  // The accumulators go to global memory straight from registers: a lane's 4-byte (NT: one column per MFMA tile) or 8-byte (NN: its
  // two adjacent columns) pieces, 128 / 256 contiguous bytes per half-wave, through a buffer descriptor whose range check drops the
  // rows past M (columns past N get an out-of-range offset) - no LDS image, no barrier, no branch.  Side inputs (residual /
  // activation-gradient operand) of the whole wave tile are requested first and folded in before the first store.  Against the LDS
  // image path below (kept for split tiles, the row-remapped patch embedding and unaligned callers): QKV 113 -> 116-122 TFLOP/s.
  if constexpr (DIRECT_OK) {
    if (direct) {
      constexpr int CW = BKC ? 1 : TN;
      auto tile_rsrc = [&](const float* base, int ld) {
        long long bytes = ((long long)(p.M - 1 - m0) * ld + (p.N - n0)) * 4;   // tile origin .. end of the matrix
        if (bytes > 0x7FFFFFFFll) bytes = 0x7FFFFFFFll;
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base + (long long)m0 * ld + n0), 0, (int)bytes, 0x00020000);
      };
      // byte offset of accumulator element r of MFMA tile (i, j) in that window; everything in the VGPR operand (the scalar offset of
      // a buffer instruction is not range-checked)
      auto eoff = [&](int i, int j, int r, int ld) -> unsigned {
        const unsigned rowpart = (unsigned)((wm * WM + i * 32 + (r & 3) + 8 * (r >> 2)) * ld * 4);   // uniform
        return n0 + dcol[j] < p.N ? rowpart + (unsigned)((4 * h * ld + dcol[j]) * 4) : DGVIT_OOB;
      };
      constexpr bool HAS_SIDE = EPI == EPI_STORE || ACT_GRAD || EPI == EPI_DRELU;
      const bool use_side = HAS_SIDE && (EPI == EPI_STORE ? p.res != nullptr : true);
      if (HAS_SIDE && use_side) {
        const float* sb = EPI == EPI_STORE ? p.res : p.aux;
        const int sld = EPI == EPI_STORE ? p.ldr : p.ldaux;
        const __amdgpu_buffer_rsrc_t sr = tile_rsrc(sb, sld);
        float side[TM][16][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if constexpr (CW == 2) {
              // one 8-byte load for the lane's two adjacent columns.  The result is bit-cast as a WHOLE vector: casting the two
              // dwords to float one by one is what this toolchain narrows to a one-dword load (the equality tests
              // against the LDS-image epilogue and the pipelined kernel, which use 4-byte loads, would catch it)
              typedef float f32x2v __attribute__((ext_vector_type(2)));
              const f32x2v v2 = __builtin_bit_cast(f32x2v, __builtin_amdgcn_raw_buffer_load_b64(sr, eoff(i, 0, r, sld), 0, 0));
              side[i][r][0] = v2[0];
              side[i][r][1] = v2[1];
            } else {
#pragma unroll
              for (int j = 0; j < TN; ++j)
                side[i][r][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(sr, eoff(i, j, r, sld), 0, 0));
            }
          }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float sv = side[i][r][j];
              if (EPI == EPI_STORE) acc[i][j][r] += sv;                     // residual first, bias below: the order of the LDS path
              else if (EPI == EPI_DGELU) acc[i][j][r] *= gelu_erf_grad(sv);
              else if (EPI == EPI_DMUL) acc[i][j][r] *= sv;
              else acc[i][j][r] = sv > 0.f ? acc[i][j][r] : 0.f;
            }
      }
      // output stores: ordinary, or non-temporal (aux 2: no allocation in the L2) for NT_STORES epilogues -- and for every direct epilogue under
      // diagnostic bit 16 of dgvit_set_gemm_diagnostics
      auto st32 = [&](unsigned v, __amdgpu_buffer_rsrc_t rs, unsigned off) {
        if (NT_STORES || DIAG_BIT(p, 16)) __builtin_amdgcn_raw_buffer_store_b32(v, rs, off, 0, 2);
        else __builtin_amdgcn_raw_buffer_store_b32(v, rs, off, 0, 0);
      };
      auto st64 = [&](u32x2 v, __amdgpu_buffer_rsrc_t rs, unsigned off) {
        if (NT_STORES || DIAG_BIT(p, 16)) __builtin_amdgcn_raw_buffer_store_b64(v, rs, off, 0, 2);
        else __builtin_amdgcn_raw_buffer_store_b64(v, rs, off, 0, 0);
      };
      const __amdgpu_buffer_rsrc_t cr = tile_rsrc(p.C, p.ldc);
      __amdgpu_buffer_rsrc_t c2r = cr;
      if (TWO_OUT) c2r = tile_rsrc(p.C2, p.ldc2);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v[TN];
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            v[j] = acc[i][j][r];
            if (EPI == EPI_STORE || TWO_OUT) v[j] += dbias[j];
            else if (EPI == EPI_RELU) v[j] = fmaxf(v[j] + dbias[j], 0.f);
            else if (EPI == EPI_GELU) v[j] = gelu_erf(v[j] + dbias[j]);
          }
          if constexpr (CW == 1) {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
              if constexpr (EPI == EPI_GELU2D) {
                float gl, gd;
                gelu_erf_both(v[j], gl, gd);
                st32(__builtin_bit_cast(unsigned, gd), cr, eoff(i, j, r, p.ldc));
                st32(__builtin_bit_cast(unsigned, gl), c2r, eoff(i, j, r, p.ldc));
              } else {
                st32(__builtin_bit_cast(unsigned, v[j]), cr, eoff(i, j, r, p.ldc));
                if (EPI == EPI_GELU2)
                  st32(__builtin_bit_cast(unsigned, gelu_erf(v[j])), c2r, eoff(i, j, r, p.ldc));
              }
            }
          } else {
            u32x2 w;
            if constexpr (EPI == EPI_GELU2D) {
              float gl0, gd0, gl1, gd1;
              gelu_erf_both(v[0], gl0, gd0);
              gelu_erf_both(v[1], gl1, gd1);
              w[0] = __builtin_bit_cast(unsigned, gd0);
              w[1] = __builtin_bit_cast(unsigned, gd1);
              st64(w, cr, eoff(i, 0, r, p.ldc));
              w[0] = __builtin_bit_cast(unsigned, gl0);
              w[1] = __builtin_bit_cast(unsigned, gl1);
              st64(w, c2r, eoff(i, 0, r, p.ldc));
              continue;
            }
            w[0] = __builtin_bit_cast(unsigned, v[0]);
            w[1] = __builtin_bit_cast(unsigned, v[1]);
            st64(w, cr, eoff(i, 0, r, p.ldc));
            if (EPI == EPI_GELU2) {
              w[0] = __builtin_bit_cast(unsigned, gelu_erf(v[0]));
              w[1] = __builtin_bit_cast(unsigned, gelu_erf(v[1]));
              st64(w, c2r, eoff(i, 0, r, p.ldc));
            }
          }
        }
      stamp(p, 3, tid);
      if (DIAG_STAMPS(p)) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        stamp(p, 7, tid);
      }
      return;
    }
  }
  // ---- epilogue ------------------------------------------------------------------------------------
  float* Cz = p.C;
  if (EPI == EPI_SPLITK) {
    Cz += (long long)zslice * p.slab_stride;
    if (p.colsum && n0 == 0 && tid < BM && m0 + tid < p.M) Cz[(long long)p.M * p.N + m0 + tid] = bsum;
  }
  // Fused LayerNorm of a finished output row (p.ln_y; launch checks N == BN, so the BN / 4 lanes tid % C4 of a wave hold the row).
  // The arithmetic and its order are those of layernorm_fwd_kernel (float4 partial sums, xor butterfly; the butterfly steps that kernel
  // takes over lanes holding nothing add zeros), so the result is bit-identical to running that kernel on C afterwards.
  auto ln_piece = [&](int m, const float (&v)[4]) {
    if constexpr (LN_OK) {
      float s = (v[0] + v[1]) + (v[2] + v[3]);
#pragma unroll
      for (int o = C4 / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      const float mu = s / (float)p.N;
      const float a = v[0] - mu, b = v[1] - mu, c = v[2] - mu, d = v[3] - mu;
      float q = (a * a + b * b) + (c * c + d * d);
#pragma unroll
      for (int o = C4 / 2; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
      const float rsd = rsqrtf(q / (float)p.N + p.ln_eps);
      const float4 g = *reinterpret_cast<const float4*>(p.ln_g + n), be = *reinterpret_cast<const float4*>(p.ln_b + n);
      *reinterpret_cast<float4*>(p.ln_y + (long long)m * p.ln_ld + n) =
          make_float4((v[0] - mu) * rsd * g.x + be.x, (v[1] - mu) * rsd * g.y + be.y, (v[2] - mu) * rsd * g.z + be.z, (v[3] - mu) * rsd * g.w + be.w);
      if (cc == 0) {
        p.ln_mean[m] = mu;
        p.ln_rstd[m] = rsd;
      }
    }
  };
  // one output row piece (row m, columns n .. n+3, v = the k-complete sums): fused epilogue arithmetic and the global stores
  auto finish = [&](int m, float (&v)[4]) {
    if constexpr (EPI == EPI_UNPATCH) {   // (scalar path: a piece may cross a patch row when pw % 4 != 0)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (n + e < p.N) Cz[unpatch_off(p, m, n + e)] = v[e];
      return;
    }
    float w2[4];
    long long crow = m;
    if (EPI == EPI_STORE && p.c_rgrp > 0) crow = (long long)m + m / p.c_rgrp + 1;
    float* cptr = Cz + crow * p.ldc + n;
    if (EPI == EPI_STORE) {
      if (p.res) {
        const long long rrow = p.res_mod > 0 ? (long long)(m % p.res_mod) + 1 : (long long)m;
        const float* rp = p.res + rrow * p.ldr + n;
        if (evec) {
          const float4 q = *reinterpret_cast<const float4*>(rp);
          v[0] += q.x; v[1] += q.y; v[2] += q.z; v[3] += q.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (n + e < p.N) v[e] += rp[e];
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += bias4[e];
    } else if (TWO_OUT) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] += bias4[e];
        if constexpr (EPI == EPI_GELU2D) gelu_erf_both(v[e], w2[e], v[e]);
        else w2[e] = gelu_erf(v[e]);
      }
    } else if (EPI == EPI_RELU) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e] + bias4[e], 0.f);
    } else if (EPI == EPI_GELU) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = gelu_erf(v[e] + bias4[e]);
    } else if (ACT_GRAD || EPI == EPI_DRELU) {
      const float* ap = p.aux + (long long)m * p.ldaux + n;
      float a4[4] = {0.f, 0.f, 0.f, 0.f};
      if (evec) {
        const float4 q = *reinterpret_cast<const float4*>(ap);
        a4[0] = q.x; a4[1] = q.y; a4[2] = q.z; a4[3] = q.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (n + e < p.N) a4[e] = ap[e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = EPI == EPI_DGELU ? v[e] * gelu_erf_grad(a4[e]) : (EPI == EPI_DMUL ? v[e] * a4[e] : (a4[e] > 0.f ? v[e] : 0.f));
    }
    if (evec) {
      *reinterpret_cast<float4*>(cptr) = make_float4(v[0], v[1], v[2], v[3]);
      if (TWO_OUT) *reinterpret_cast<float4*>(p.C2 + (long long)m * p.ldc2 + n) = make_float4(w2[0], w2[1], w2[2], w2[3]);
      if (LN_OK && p.ln_y) ln_piece(m, v);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (n + e < p.N) {
          cptr[e] = v[e];
          if (TWO_OUT) p.C2[(long long)m * p.ldc2 + n + e] = w2[e];
        }
    }
  };
  // k-slice of a split tile: the raw partial sums go to this slice's dense [BM][BN] slab
  float* slab = nullptr;
  if (EPI != EPI_SPLITK && nz > 1) slab = p.slabs + ((long long)(tile - p.split_from) * nz + zs) * (BM * BN);
  // ---- vector fast path (p.evec: every shape of the encoder).  Stamps showed the per-piece `finish` below spending 12-18 k
  // cycles per chunk: a conditional side-input load inside the piece loop makes the compiler wait vmcnt(0) at the merge point
  // of every piece, and on gfx9 that also waits for the PREVIOUS piece's store - a serial chain of loaded-memory round trips
  // (~4 k cycles each), a third of a K = 256 tile's life.  Here the side inputs (residual / activation-gradient operand) of
  // every piece are fetched first, with row indices clamped instead of branched on, so nothing is in flight behind a store;
  // then each chunk is LDS reads -> arithmetic -> stores back to back, no wait in between.
  constexpr int NP = CROWS / RPP;                       // row pieces per thread and chunk
  static_assert(CROWS % RPP == 0, "epilogue row pieces");
  constexpr bool HAS_SIDE = EPI == EPI_STORE || ACT_GRAD || EPI == EPI_DRELU;
  constexpr bool SIDE_ALL = NCHUNK == 1 && NP <= 4;     // one chunk whose side inputs fit in 16 registers: fetch them before the C image barrier
                                                        // (two-chunk tiles take the direct epilogue on the hot path; prefetching both chunks here spilled)
  const bool fast = evec && !slab;
  const bool nvalid = n < p.N;
  const int nc = nvalid ? n : 0;
  const bool use_side = HAS_SIDE && (EPI == EPI_STORE ? p.res != nullptr : true);
  float4 side[HAS_SIDE ? (SIDE_ALL ? NCHUNK * NP : NP) : 1];
#pragma unroll
  for (auto& sv : side) sv = make_float4(0.f, 0.f, 0.f, 0.f);   // (defined on every path: undefined values here were spilled to scratch)
  auto load_side = [&](int ch, float4* dst) {
#pragma unroll
    for (int it = 0; it < NP; ++it) {
      const int m = min(m0 + ch * CROWS + rr0 + it * RPP, p.M - 1);
      const float* sp;
      if (EPI == EPI_STORE) {
        const long long rrow = p.res_mod > 0 ? (long long)(m % p.res_mod) + 1 : (long long)m;
        sp = p.res + rrow * p.ldr + nc;
      } else {
        sp = p.aux + (long long)m * p.ldaux + nc;
      }
      dst[it] = *reinterpret_cast<const float4*>(sp);
    }
  };
  if (HAS_SIDE && SIDE_ALL && fast && use_side) {
#pragma unroll
    for (int ch = 0; ch < NCHUNK; ++ch) load_side(ch, side + ch * NP);
  }
#pragma unroll
  for (int ch = 0; ch < NCHUNK; ++ch) {
    if (NCHUNK == 1 || wm == ch) {
      const int rbase = NCHUNK == 1 ? wm * WM : 0;
      // (an m/n-contiguous operand's tiles are interleaved, see frag_mc: tile-row rt of tile i is row TM * rt + i, and likewise
      //  for columns, where a lane's TN values are adjacent and leave as one vector write)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rt = (r & 3) + 8 * (r >> 2) + 4 * h;
          float* crow = smem + (rbase + (AKC ? i * 32 + rt : rt * TM + i)) * CS + wn * WN;
          if constexpr (BKC || TN == 1) {
#pragma unroll
            for (int j = 0; j < TN; ++j) crow[j * 32 + li] = acc[i][j][r];
          } else {
            typedef float cvec_t __attribute__((ext_vector_type(TN)));
            cvec_t v;
#pragma unroll
            for (int j = 0; j < TN; ++j) v[j] = acc[i][j][r];
            *reinterpret_cast<cvec_t*>(crow + li * TN) = v;
          }
        }
    }
    __syncthreads();
    stamp(p, 8 + 2 * ch, tid);       // chunk's C image in LDS
    if (slab) {
      // write-through (sc1) stores: the partial tile leaves this XCD's L2 at once, so no release fence (an L2 write-back of
      // every dirty line the other workgroups' C stores left there) is needed before the ticket
      const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(slab, 0, BM * BN * 4, 0x00020000);
      for (int rr = rr0; rr < CROWS; rr += RPP) {
        const float4 t = *reinterpret_cast<const float4*>(smem + rr * CS + cc);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, t), srs, (unsigned)(((ch * CROWS + rr) * BN + cc) * 4), 0, 16);
      }
    } else if (fast) {
      if (HAS_SIDE && !SIDE_ALL && use_side) load_side(ch, side);   // big tiles: per chunk (waits for the previous chunk's stores)
      float4* sd = side + (HAS_SIDE && SIDE_ALL ? ch * NP : 0);
      if (EPI == EPI_DGELU) {   // operand -> gelu'(operand) in place, piece by piece (keeps the erf temporaries of one piece live)
#pragma unroll
        for (int it = 0; it < NP; ++it)
          sd[it] = make_float4(gelu_erf_grad(sd[it].x), gelu_erf_grad(sd[it].y), gelu_erf_grad(sd[it].z), gelu_erf_grad(sd[it].w));
      }
      // one-chunk tiles read all their row pieces first; two-chunk tiles (whose hot path is the direct epilogue above) read them
      // one by one: the batch of NP = 4 pieces beside 4 side inputs did not fit the register budget of 5 workgroups per CU
      constexpr bool T_FIRST = NCHUNK == 1;
      float4 t[T_FIRST ? NP : 1];
      if constexpr (T_FIRST) {
#pragma unroll
        for (int it = 0; it < NP; ++it) t[it] = *reinterpret_cast<const float4*>(smem + (rr0 + it * RPP) * CS + cc);
      }
#pragma unroll
      for (int it = 0; it < NP; ++it) {
        const int m = m0 + ch * CROWS + rr0 + it * RPP;
        if constexpr (!T_FIRST) t[0] = *reinterpret_cast<const float4*>(smem + (rr0 + it * RPP) * CS + cc);
        const float4 tv = t[T_FIRST ? it : 0];
        float v[4] = {tv.x, tv.y, tv.z, tv.w}, w2[4];
        if (EPI == EPI_STORE) {
          if (use_side) { v[0] += sd[it].x; v[1] += sd[it].y; v[2] += sd[it].z; v[3] += sd[it].w; }   // same order as `finish`: residual, then bias
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += bias4[e];
        } else if (TWO_OUT) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[e] += bias4[e];
            if constexpr (EPI == EPI_GELU2D) gelu_erf_both(v[e], w2[e], v[e]);
            else w2[e] = gelu_erf(v[e]);
          }
        } else if (EPI == EPI_RELU) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e] + bias4[e], 0.f);
        } else if (EPI == EPI_GELU) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = gelu_erf(v[e] + bias4[e]);
        } else if (ACT_GRAD || EPI == EPI_DRELU) {
          const float a4[4] = {sd[it].x, sd[it].y, sd[it].z, sd[it].w};
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = ACT_GRAD ? v[e] * a4[e] : (a4[e] > 0.f ? v[e] : 0.f);
        }
        if (EPI == EPI_UNPATCH && m < p.M && nvalid) {
          // pw % 4 == 0 (gemm_f32 sets evec only then): the four columns n .. n+3 are adjacent pixels of one image row
          *reinterpret_cast<float4*>(Cz + unpatch_off(p, m, n)) = make_float4(v[0], v[1], v[2], v[3]);
        } else if (EPI != EPI_UNPATCH && m < p.M && nvalid) {
          long long crow = m;
          if (EPI == EPI_STORE && p.c_rgrp > 0) crow = (long long)m + m / p.c_rgrp + 1;
          int ncol = n;
          if (DIAG_BIT(p, 4)) {   // diagnostic: every tile stores over tile 0 (the same instructions, no HBM write stream; results garbage)
            crow = m - m0;
            ncol = cc;
          }
          *reinterpret_cast<float4*>(Cz + crow * p.ldc + ncol) = make_float4(v[0], v[1], v[2], v[3]);   // (non-temporal stores measured the same: +-1 %)
          if (TWO_OUT) *reinterpret_cast<float4*>(p.C2 + crow * p.ldc2 + ncol) = make_float4(w2[0], w2[1], w2[2], w2[3]);
          if (LN_OK && p.ln_y) ln_piece(m, v);
        }
      }
    } else if (ELEMWISE && n < p.N) {
      // element-wise path (unaligned / odd-N callers): one piece at a time through `finish`
      for (int it = 0; it < CROWS / RPP; ++it) {
        const int rr = rr0 + it * RPP;
        const int m = m0 + ch * CROWS + rr;
        if (m < p.M) {
          const float4 t = *reinterpret_cast<const float4*>(smem + rr * CS + cc);
          float v[4] = {t.x, t.y, t.z, t.w};
          finish(m, v);
        }
      }
    }
    stamp(p, 9 + 2 * ch, tid);       // chunk's stores issued
    if (ch + 1 < NCHUNK) __syncthreads();
  }
  stamp(p, 3, tid);                                                 // stores issued
  if (DIAG_STAMPS(p)) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // diagnostic run only: the last stamp sees them drained
    stamp(p, 7, tid);
  }
  if (EPI != EPI_SPLITK && nz > 1) {
    // publish the slab, take a ticket (cdna_hip_programming.md Guideline 16, recipe R1): write-through payload, every storing
    // wave drains its stores, barrier, ONE lane adds to the tile's counter; the last arriver acquires (agent scope) before
    // anybody reads the other slices.  Placement independent: nothing assumes which CU / XCD ran which slice.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int* flag = reinterpret_cast<int*>(smem);
    if (tid == 0) {
      const int ticket = __hip_atomic_fetch_add(p.counters + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = ticket == nz - 1;
      if (last) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(p.counters + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // clean for the next launch
      }
      *flag = last;
    }
    __syncthreads();
    if (!*flag) return;
    if (n < p.N) {
      const float* s0 = p.slabs + (long long)(tile - p.split_from) * nz * (BM * BN);
      for (int rr = rr0; rr < BM; rr += RPP) {
        const int m = m0 + rr;
        if (m >= p.M) break;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        const float* sp = s0 + rr * BN + cc;
        for (int z0 = 0; z0 < nz; z0 += 8) {   // 8 slice loads in flight, then added in slice order: bit-reproducible
          float4 t[8];
#pragma unroll
          for (int u = 0; u < 8; ++u)
            t[u] = z0 + u < nz ? *reinterpret_cast<const float4*>(sp + (long long)(z0 + u) * (BM * BN)) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            v[0] += t[u].x; v[1] += t[u].y; v[2] += t[u].z; v[3] += t[u].w;
          }
        }
        finish(m, v);
      }
    }
  }
}

// ---- in-launch split-K policy -------------------------------------------------------------------------------------------
// (a) few tiles, long K (small batches: T = 65 ... 2080 rows against K = 2048): every tile is cut so that the grid fills the chip;
// (b) a big grid whose last partial round would leave most CUs idle (tiles mod 256 <= 128: measured at 25600 x 256 x 2048,
//     1600 tiles = 6.25 per CU run 12 % longer than 1536 tiles): only the left-over tiles are cut, into 256 / r slices.
// A slice keeps at least 4 k-tiles.  Returns nsplit <= 1 for "do not split".
inline GemmSplitPlan split_plan(int M, int N, int K, int BM, int BN, int BK, int wg_per_cu) {
  GemmSplitPlan pl = {};
  const long long tiles = (long long)((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  pl.tiles = (int)tiles;
  pl.nsplit = 1;
  pl.split_from = (int)tiles;
  const int KT = (K + BK - 1) / BK, cus = 256, slots = cus * wg_per_cu;
  if (KT < 8 || tiles <= 0) return pl;
  int S = 1;
  long long from = tiles;
  if (tiles * 2 <= slots) {
    S = (int)std::min<long long>(KT / 4, slots / tiles);
    from = 0;
  } else if (tiles > slots) {
    const long long r = tiles % cus;
    if (r > 0 && r <= cus / 2) {
      S = (int)std::min<long long>(KT / 4, cus / r);
      from = tiles - r;
    }
  }
  if (S < 2) return pl;
  const int kt_per = (KT + S - 1) / S;
  S = (KT + kt_per - 1) / kt_per;          // no empty slices
  if (S < 2) return pl;
  pl.nsplit = S;
  pl.split_from = (int)from;
  pl.kchunk = kt_per * BK;
  pl.slab_floats = (tiles - from) * S * (long long)BM * BN;
  return pl;
}

}  // namespace

#include "gemm_pipe.h"   // diagnostic build: gemm_f32_pipe_kernel and launch_persistent; empty in the product

namespace {

// the tallest / widest tile of DGVIT_TILES: gemm_f32's leading-dimension checks bound a tile's 32-bit row offsets with it
#define DGVIT_MAX_TILE_ROWS 128

template <class T, int LAYOUT, int VEC, int EPI, bool GATHER = false>
int launch(const GemmParams& p0, int nsplit, hipStream_t stream) {
  constexpr int BM = T::BM, BN = T::BN, BK = T::BK;
  static_assert(BM <= DGVIT_MAX_TILE_ROWS && BN <= DGVIT_MAX_TILE_ROWS, "raise DGVIT_MAX_TILE_ROWS: gemm_f32's leading-dimension checks depend on it");
  constexpr bool AKC = LAYOUT != GEMM_TN;
  constexpr bool BKC = LAYOUT == GEMM_NT;
  constexpr int A_TILE = AKC ? BM * (BK + 4) : BK * (BM + 4);
  constexpr int B_TILE = BKC ? BN * (BK + 4) : BK * (BN + 4);
  constexpr size_t lds = 2 * (A_TILE + B_TILE) * sizeof(float);
  auto kern = gemm_f32_kernel<T, LAYOUT, VEC, EPI, GATHER>;
  TRY((allow_dynamic_lds<gemm_f32_kernel<T, LAYOUT, VEC, EPI, GATHER>>(160 * 1024, "gemm")));
  GemmParams p = p0;
  if (p.ln_y) {   // fused LayerNorm: the whole output row must sit in this tile's LDS image, vector path
    DGVIT_CHECK_ARG(EPI == EPI_STORE && VEC == 4 && !GATHER && LAYOUT != GEMM_TN && p.evec && p.N == BN && BN == 64 && p.c_rgrp == 0,
                    "gemm: fused LayerNorm needs the vector EPI_STORE path, a 64-wide tile and N == 64, got tile width %d, N = %d", BN, p.N);
    DGVIT_CHECK_ARG(p.ln_g && p.ln_b && p.ln_mean && p.ln_rstd && p.ln_ld % 4 == 0 && al16(p.ln_g) && al16(p.ln_b) && al16(p.ln_y),
                    "gemm: fused LayerNorm operands must be present and 16-byte aligned");
  }
  p.stamps = g_gemm_stamps;
  p.stamp_capacity = g_gemm_stamp_capacity;
  p.diag = g_gemm_diag;
  const long long tiles = (long long)((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN);
  DGVIT_CHECK_ARG(tiles > 0 && tiles < (1ll << 31), "gemm: bad tile count %lld", tiles);
  long long blocks = tiles;
  p.nsplit = 1;
  p.split_from = (int)tiles;
  if (EPI != EPI_SPLITK && VEC == 4 && p.counters && p.slabs && p.evec && g_gemm_split) {   // (the gather loader takes k-slices too)
    const int occ = (int)std::min<size_t>(8, (160 * 1024) / lds);
    const GemmSplitPlan pl = split_plan(p.M, p.N, p.K, BM, BN, BK, occ);
    if (pl.nsplit > 1 && pl.slab_floats <= p.slab_capacity && tiles <= p.counter_capacity) {
      p.nsplit = pl.nsplit; p.split_from = pl.split_from; p.kchunk_split = pl.kchunk;
      blocks = pl.split_from + (tiles - pl.split_from) * pl.nsplit;
    }
  }
#ifdef DGVIT_DIAG
  if constexpr (VEC == 4 && !GATHER && EPI != EPI_SPLITK && EPI != EPI_UNPATCH && LAYOUT != GEMM_TN) {
    // whole tiles only, vector epilogue, plain row mapping: the persistent kernel (tile loop in the workgroup, next tile's fetch
    // under the epilogue) when a resident slot gets several tiles
    constexpr bool TWO_OUT = EPI == EPI_GELU2 || EPI == EPI_GELU2D;   // as in the kernel: C2 is addressed with C's stride
    if (g_gemm_persist && (p.nsplit == 1 || g_gemm_persist == 2) && nsplit == 1 && p.evec && p.c_rgrp == 0 && p.res_mod == 0 &&
        (!TWO_OUT || p.ldc2 == p.ldc) && g_gemm_lds_pad == 0 && !p.ln_y) {
      bool taken = false;
      const int rc = launch_persistent<T, LAYOUT, EPI>(p0, stream, &taken);
      if (rc != DGVIT_OK || taken) return rc;
    }
  }
#endif
  dim3 grid((unsigned)blocks, 1, (unsigned)nsplit);
  p.zsplit = 0;
  if (EPI == EPI_SPLITK && nsplit > 1 && g_gemm_zfold && blocks * nsplit < (1ll << 31)) {   // k-slices folded into blockIdx.x (see the kernel)
    p.zsplit = nsplit;
    grid = dim3((unsigned)(blocks * nsplit), 1, 1);
  }
  {
    ProfileScope t(PROF_GEMM, 2.0 * p.M * p.N * p.K, stream);
    hipLaunchKernelGGL(kern, grid, dim3(T::NT), lds + (size_t)g_gemm_lds_pad, stream, p);
  }
  DGVIT_CHECK_LAUNCH("gemm_f32_kernel");
  return DGVIT_OK;
}

// tile_hint = BM*1000000 + BN*1000 + BK (e.g. 128128032), 0 = automatic
#define DGVIT_TILES(X) X(128, 128, 32) X(128, 128, 16) X(64, 64, 32) X(64, 64, 64) X(128, 64, 32) X(64, 128, 32) X(64, 128, 16) X(64, 64, 16)

// measured on MI355X at T = 25600 token rows (tools/gemm_shapes_bench.py, profiles/r01_b_gemm_tiles.txt):
// weight gradients (long K, split over tokens) like the 128x128 tile; forward / data-gradient GEMMs are
// tile-quantisation and prologue bound, so they take small tiles: wide outputs 64x128x16, narrow 64x64x32
inline int auto_tile(int layout, int M, int N) {
  if (layout == GEMM_TN) return (M >= 128 && N >= 128) ? 128128032 : 64064032;
  // (round 4 re-run of the table, profiles/r04_c_gemm_tiles.txt: the choices stand, except the data gradient of to_out -- NN, N = 512,
  //  K = 256 -- which gains 5 % on the wide tile)
  if (layout == GEMM_NN && N >= 512) return 64128016;
  return N >= 1024 ? 64128016 : 64064032;
}

template <int LAYOUT, int EPI>
int pick_tile(const GemmParams& p, int nsplit, bool vec4, int tile_hint, hipStream_t stream) {
  if constexpr (LAYOUT == GEMM_NT && (EPI == EPI_STORE || EPI == EPI_RELU)) {
    if (p.g_img) return launch<TileCfg<64, 64, 32>, LAYOUT, 4, EPI, true>(p, nsplit, stream);   // patch / window gather in the A loader
  }
  if constexpr (EPI == EPI_UNPATCH) {   // the one tile that carries both the float4 and the element-wise image stores
    return vec4 ? launch<TileCfg<64, 64, 32>, LAYOUT, 4, EPI>(p, nsplit, stream) : launch<TileCfg<64, 64, 32>, LAYOUT, 1, EPI>(p, nsplit, stream);
  } else {
    if (!vec4) return launch<TileCfg<64, 64, 32>, LAYOUT, 1, EPI>(p, nsplit, stream);
    int choice = tile_hint;
    if (choice == 64) choice = 64064032;
    if (choice == 128) choice = 128128032;
    if (choice == 0) choice = auto_tile(LAYOUT, p.M, p.N);
    if (!p.evec) choice = 64064032;   // the one tile that carries the element-wise epilogue (odd N / ldc, unaligned outputs)
#define X(BM_, BN_, BK_) \
    if (choice == BM_ * 1000000 + BN_ * 1000 + BK_) return launch<TileCfg<BM_, BN_, BK_>, LAYOUT, 4, EPI>(p, nsplit, stream);
    DGVIT_TILES(X)
#undef X
    return dgvit_set_error(DGVIT_ERR_ARG, "gemm: unknown tile %d", choice);
  }
}


}  // namespace


// the same for a GEMM whose A operand is gathered from an image (patch embedding, implicit-GEMM convolutions): always the 64 x 64 x 32 tile
GemmSplitPlan gemm_split_plan_gather(int M, int N, int K) {
  GemmSplitPlan none = {};
  none.nsplit = 1;
  if (M <= 0 || N <= 0 || K <= 0) return none;
  const size_t lds = 2 * (size_t)(64 * (32 + 4) + 64 * (32 + 4)) * sizeof(float);
  return split_plan(M, N, K, 64, 64, 32, (int)std::min<size_t>(8, (160 * 1024) / lds));
}

GemmSplitPlan gemm_split_plan(int layout, int M, int N, int K) {
  GemmSplitPlan none = {};
  none.nsplit = 1;
  if (layout == GEMM_TN || M <= 0 || N <= 0 || K <= 0) return none;
  const int c = auto_tile(layout, M, N);
  const int BM = c / 1000000, BN = (c / 1000) % 1000, BK = c % 1000;
  const bool akc = true, bkc = layout == GEMM_NT;
  const size_t lds = 2 * (size_t)((akc ? BM * (BK + 4) : BK * (BM + 4)) + (bkc ? BN * (BK + 4) : BK * (BN + 4))) * sizeof(float);
  return split_plan(M, N, K, BM, BN, BK, (int)std::min<size_t>(8, (160 * 1024) / lds));
}

int gemm_f32(int layout, int epi, const GemmParams& p, int nsplit, hipStream_t stream) {
  DGVIT_CHECK_ARG((p.A || p.g_img) && p.B && p.C, "gemm: null operand");
  DGVIT_CHECK_ARG(!p.g_img || (layout == GEMM_NT && (epi == EPI_STORE || epi == EPI_RELU) && p.g_pw % 4 == 0 && p.g_wi % 4 == 0 && p.g_xs % 4 == 0 &&
                               al16(p.g_img) && al16(p.B) && p.ldb % 4 == 0 && p.K % 4 == 0 && p.K == (p.g_kh ? p.g_kh : p.g_ph) * p.g_pw &&
                               (long long)p.K * p.g_inv < (1ll << 32)),
                  "gemm: patch gather needs the NT / store form, patch and image widths that are multiples of 4 and 16-byte aligned operands");
  DGVIT_CHECK_ARG(p.M > 0 && p.N > 0 && p.K > 0, "gemm: empty problem M=%d N=%d K=%d", p.M, p.N, p.K);
  DGVIT_CHECK_ARG(nsplit >= 1 && p.kchunk > 0 && p.kchunk % 32 == 0, "gemm: kchunk must be a positive multiple of 32");
  DGVIT_CHECK_ARG((long long)p.kchunk * nsplit >= p.K, "gemm: split does not cover K");
  // float4 staging needs 16-byte aligned bases, leading dims that are multiples of 4 and a
  // contiguous extent that is a multiple of 4; anything else takes the scalar-load 64x64 variant.
  bool vec4 = al16(p.A) && al16(p.B) && p.lda % 4 == 0 && p.ldb % 4 == 0;
  if (layout == GEMM_NT) vec4 = vec4 && p.K % 4 == 0;
  if (layout == GEMM_NN) vec4 = vec4 && p.K % 4 == 0 && p.N % 4 == 0;
  if (layout == GEMM_TN) vec4 = vec4 && p.M % 4 == 0 && p.N % 4 == 0;
  DGVIT_CHECK_ARG(p.a_kgrp == 0, "gemm: a_kgrp is no longer supported (gather the rows first)");
  // 32-bit byte offsets inside a descriptor window of at most 2 GiB: a tile's DGVIT_MAX_TILE_ROWS rows of an operand must fit
  constexpr long long ROW_BYTES = 4ll * DGVIT_MAX_TILE_ROWS;
  DGVIT_CHECK_ARG(p.lda * ROW_BYTES < 0x7FFFFFFFll && p.ldb * ROW_BYTES < 0x7FFFFFFFll, "gemm: leading dimension too large");
  // ... and so must the rows of C / residual / C2 / aux that the direct epilogue addresses the same way.  Conservative: strides this
  // large are refused whatever M is and also where the LDS-image or element-wise epilogue (64-bit addresses) would run.
  DGVIT_CHECK_ARG(p.ldc * ROW_BYTES < 0x7FFFFFFFll && (!p.res || p.ldr * ROW_BYTES < 0x7FFFFFFFll) &&
                      (!p.C2 || p.ldc2 * ROW_BYTES < 0x7FFFFFFFll) && (!p.aux || p.ldaux * ROW_BYTES < 0x7FFFFFFFll),
                  "gemm: output leading dimension too large");
  DGVIT_CHECK_ARG(layout == GEMM_NT || (long long)p.kchunk * p.ldb * 4 < 0x7FFFFFFFll, "gemm: k-chunk x ldb exceeds the 2 GiB descriptor window");
  DGVIT_CHECK_ARG(layout != GEMM_TN || (long long)p.kchunk * p.lda * 4 < 0x7FFFFFFFll, "gemm: k-chunk x lda exceeds the 2 GiB descriptor window");
  GemmParams q = p;
  q.evec = p.N % 4 == 0 && p.ldc % 4 == 0 && al16(p.C) && (!p.res || (p.ldr % 4 == 0 && al16(p.res))) &&
           (!p.C2 || (p.ldc2 % 4 == 0 && al16(p.C2))) && (!p.aux || (p.ldaux % 4 == 0 && al16(p.aux))) &&
           (epi != EPI_SPLITK || p.slab_stride % 4 == 0);
  if (epi == EPI_UNPATCH) {
    DGVIT_CHECK_ARG(layout == GEMM_NN && !p.g_img && !p.bias && !p.res && !p.counters && p.g_P > 0 && p.g_gw > 0 && p.g_pw > 0 && p.g_ph > 0 &&
                        p.N == p.g_ph * p.g_pw && p.M % p.g_P == 0 && p.g_P % p.g_gw == 0 && p.g_wi == p.g_gw * p.g_pw &&
                        (long long)p.g_hw == (long long)(p.g_P / p.g_gw) * p.g_ph * p.g_wi,
                    "gemm: the unpatch epilogue needs the NN form, no bias / residual / split and a consistent patch geometry");
    q.evec = p.g_pw % 4 == 0 && al16(p.C);   // float4 stores stay inside one patch row (image width = gw * pw: every row start aligned)
  }
  const int th = g_gemm_tile_hint;
#define CASE(L, E) \
  if (layout == L && epi == E) return pick_tile<L, E>(q, nsplit, vec4, th, stream);
  CASE(GEMM_NT, EPI_STORE)
  CASE(GEMM_NT, EPI_GELU2)
  CASE(GEMM_NT, EPI_GELU2D)
  CASE(GEMM_NT, EPI_GELU)
  CASE(GEMM_NT, EPI_RELU)
  CASE(GEMM_NN, EPI_STORE)
  CASE(GEMM_NN, EPI_DGELU)
  CASE(GEMM_NN, EPI_DMUL)
  CASE(GEMM_NN, EPI_DRELU)
  CASE(GEMM_NN, EPI_UNPATCH)
  CASE(GEMM_TN, EPI_SPLITK)
#undef CASE
  return dgvit_set_error(DGVIT_ERR_ARG, "gemm: unsupported layout/epilogue %d/%d", layout, epi);
}
