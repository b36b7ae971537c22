// Tile primitives of the fp32 MFMA GEMM (gemm.hip) and of its diagnostic pipelined variant (gemm_pipe.h): the tile configuration, the
// XCD-contiguous tile order, the global -> register -> LDS loader `Fetch` (with the patch / window gather), the LDS -> MFMA operand
// fragments and the instruction-order pattern of the main loop.  The layouts are described at the top of gemm.hip.
#pragma once
#include "common.h"

namespace {

// BM x BN output tile, BK-deep k-tiles, WVM x WVN waves (each owning a (BM/WVM) x (BN/WVN) block of 32x32 accumulators).
// 2x2 waves everywhere: two-wave workgroups (1x2 / 2x1) measured 10-45 % slower and eight-wave ones (128x128 as 2x4,
// 256x128x16 as 4x2) hit the same 83 % in-CU ceiling as 2x2 (tools/gemm_fill_probe.py, round 1)
template <int BM_, int BN_, int BK_, int WVM_ = 2, int WVN_ = 2>
struct TileCfg {
  static constexpr int BM = BM_, BN = BN_, BK = BK_, WVM = WVM_, WVN = WVN_, NT = 64 * WVM_ * WVN_;
  // workgroups per CU the two LDS stages allow (<= 32 KB each: 5, the occupancy the K = 256 shapes are tuned at); the register
  // allocator is held to it, so an epilogue variant cannot silently cost a resident workgroup
  static constexpr int LDS_BYTES = 2 * (BM_ + BN_) * (BK_ + 4) * 4;
  static constexpr int MINB = LDS_BYTES * 5 <= 160 * 1024 ? 5 : 2;
};

__device__ __forceinline__ int xcd_remap(int id, int n) {
  // Blocks are dealt round-robin over the 8 XCDs; give each XCD a contiguous chunk of the tile grid so
  // that the column tiles sharing an A row-panel hit the same L2 (speed only, bijective for any n).
  const int q = n >> 3, r = n & 7, xcd = id & 7, loc = id >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
}

// ---- global -> register tile fetch ---------------------------------------------------------------
// KC: tile is R rows x BK k (k contiguous in memory).  MC: tile is BK k-rows x R (row index contiguous).
// VEC == 4: 16-byte buffer loads through a per-workgroup resource descriptor; rows/columns/k outside the
// matrix are dropped by the hardware range check (offset >= num_records reads 0), so the fetch is
// branch-free and can be scheduled among the MFMAs.  VEC == 1: scalar loads with explicit predicates
// (odd leading dimensions / unaligned bases; small head and odd-patch GEMMs only).
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
#define DGVIT_OOB 0xFFFFFFF0u

template <int R, int BK, bool KC, int VEC, int NT, bool GATHER = false>
struct Fetch {
  static_assert(!GATHER || (KC && VEC == 4), "the patch gather is a k-contiguous float4 fetch");
  static_assert(R * BK / 4 % NT == 0, "tile must split evenly over the workgroup's threads");
  static constexpr int NV = R * BK / 4 / NT;  // float4 slots per thread
  static constexpr int PER_ROW = KC ? BK / 4 : R / 4;

  // --- VEC == 4 ---------------------------------------------------------------------------------
  struct Plan {
    __amdgpu_buffer_rsrc_t rsrc;
    unsigned off[NV];   // byte offset of slot i at the block's first k-tile
    int kc[NV];         // KC: k offset of the slot inside a tile; MC: k row of the slot inside a tile
    unsigned bad[NV];   // MC: all ones when the slot's columns lie outside the matrix (OR-ed into the offset: no branch), else 0
    unsigned kstep;     // bytes to advance per k-tile
    int g_wi, g_pw, g_inv, g_shift;   // GATHER: image row pitch, window-row floats, 2^shift / pw + 1, shift
    int g_k0;                         // GATHER: first k of this workgroup's k-range (a k-slice of a split tile starts past 0)
  };

  // GATHER: A is never materialised.  Row m of the patch matrix starts at pixel (b, hy * ph, wx * xs) of the image; element k of
  // the row is p1 = k / pw image rows further down and p2 = k % pw floats to the right (k / pw by multiply-shift; dgvit_api checks
  // that it is exact for every k < K).  Non-overlapping patches (xs = pw) and the strided 5x5 windows of the NHWC convolutions
  // (xs = stride * C, pw = KW * C) are the same arithmetic.  The descriptor covers the whole image buffer.
  __device__ static __forceinline__ void plan_gather(Plan& pl, const GemmParams& p, int r0, int kbeg, int tid) {
    pl.g_k0 = kbeg;
    long long bytes = p.g_img_floats * 4;
    if (bytes > 0x7FFFFFFFll) bytes = 0x7FFFFFFFll;
    pl.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.g_img), 0, (int)bytes, 0x00020000);
    pl.kstep = 0;
    pl.g_wi = p.g_wi; pl.g_pw = p.g_pw; pl.g_inv = p.g_inv; pl.g_shift = p.g_shift ? p.g_shift : 16;
    const int xs = p.g_xs ? p.g_xs : p.g_pw;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int f = tid + i * NT;
      const int a = f / PER_ROW, c = (f % PER_ROW) * 4;
      const int m = r0 + a;
      const int b = m / p.g_P, pi = m - b * p.g_P, hy = pi / p.g_gw, wx = pi - hy * p.g_gw;
      pl.off[i] = ((unsigned)b * (unsigned)p.g_hw + (unsigned)(hy * p.g_ph) * (unsigned)p.g_wi + (unsigned)(wx * xs)) * 4u;
      pl.kc[i] = c;
      pl.bad[i] = m < p.M ? 0u : 0xFFFFFFFFu;
    }
  }

  __device__ static __forceinline__ void plan(Plan& pl, const float* base, int ld, int r0, int rmax, int kbeg, int ktotal,
                                              int tid) {
    // resource base = first element this workgroup can touch; num_records = bytes from there to the end of the matrix
    long long first, last;
    if (KC) {
      first = (long long)r0 * ld + kbeg;
      last = (long long)(rmax - 1) * ld + ktotal;       // one past the last valid element
    } else {
      first = (long long)kbeg * ld + r0;
      last = (long long)(ktotal - 1) * ld + rmax;
    }
    long long bytes = (last - first) * 4;
    if (bytes > 0x7FFFFFFFll) bytes = 0x7FFFFFFFll;
    if (bytes < 0) bytes = 0;
    pl.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base + first), 0, (int)bytes, 0x00020000);
    pl.kstep = KC ? BK * 4u : (unsigned)BK * (unsigned)ld * 4u;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int f = tid + i * NT;
      const int a = f / PER_ROW, c = (f % PER_ROW) * 4;
      if (KC) {
        pl.off[i] = ((unsigned)a * (unsigned)ld + (unsigned)c) * 4u;
        pl.kc[i] = c;
        pl.bad[i] = 0u;  // rows past rmax fall outside num_records
      } else {
        pl.off[i] = ((unsigned)a * (unsigned)ld + (unsigned)c) * 4u;
        pl.kc[i] = a;
        pl.bad[i] = r0 + c < rmax ? 0u : 0xFFFFFFFFu;
      }
    }
  }

  // fetch k-tile number `t` (k0 = kbeg + t*BK); klim = kend - kbeg
  __device__ static __forceinline__ void run4(float4 (&reg)[NV], const Plan& pl, int t, int klim) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      unsigned at;
      if constexpr (GATHER) {
        const unsigned k = (unsigned)(pl.g_k0 + t * BK + pl.kc[i]), p1 = (k * (unsigned)pl.g_inv) >> pl.g_shift, p2 = k - p1 * (unsigned)pl.g_pw;
        at = (pl.off[i] + (p1 * (unsigned)pl.g_wi + p2) * 4u) | pl.bad[i];
      } else {
        at = (pl.off[i] + (unsigned)t * pl.kstep) | pl.bad[i];   // num_records <= 0x7FFFFFFF: all ones is out of range
      }
      const unsigned o = t * BK + pl.kc[i] < klim ? at : DGVIT_OOB;
      reg[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(pl.rsrc, o, 0, 0));
    }
  }

  // --- VEC == 1 ---------------------------------------------------------------------------------
  __device__ static __forceinline__ void run(float4 (&reg)[NV], const float* __restrict__ base, int ld, int r0,
                                             int rmax, int k0, int kend, int tid) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int f = tid + i * NT;
      const int a = f / PER_ROW, c = (f % PER_ROW) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (KC) {
        const int row = r0 + a, k = k0 + c;
        if (row < rmax) {
          const float* src = base + (long long)row * ld + k;
          if (k + 0 < kend) v.x = src[0];
          if (k + 1 < kend) v.y = src[1];
          if (k + 2 < kend) v.z = src[2];
          if (k + 3 < kend) v.w = src[3];
        }
      } else {
        const int k = k0 + a, col = r0 + c;
        if (k < kend) {
          const float* src = base + (long long)k * ld + col;
          if (col + 0 < rmax) v.x = src[0];
          if (col + 1 < rmax) v.y = src[1];
          if (col + 2 < rmax) v.z = src[2];
          if (col + 3 < rmax) v.w = src[3];
        }
      }
      reg[i] = v;
    }
  }

  __device__ static __forceinline__ void stash(const float4 (&reg)[NV], float* lds, int tid) {
    constexpr int STRIDE = KC ? BK + 4 : R + 4;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int f = tid + i * NT;
      const int a = f / PER_ROW, c = (f % PER_ROW) * 4;
      *reinterpret_cast<float4*>(lds + a * STRIDE + c) = reg[i];
    }
  }
};

// ---- LDS -> MFMA operand fragments for one 8-deep k-group -----------------------------------------
template <int R, int BK, bool KC>
__device__ __forceinline__ void frag(float (&out)[4], const float* lds, int row, int g, int h) {
  if (KC) {
    const float4 v = *reinterpret_cast<const float4*>(lds + row * (BK + 4) + 8 * g + 4 * h);
    out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
  } else {
    const float* p = lds + (8 * g + 4 * h) * (R + 4) + row;
#pragma unroll
    for (int s = 0; s < 4; ++s) out[s] = p[s * (R + 4)];
  }
}

// m/n-contiguous operand, the wave's NTILE 32-row MFMA tiles INTERLEAVED: lane i of tile t owns row base + NTILE * i + t, so the
// NTILE values a lane needs from one k-row are adjacent in LDS and come in with one ds_read_b64 / b128 (256 B/clk) instead of NTILE
// ds_read_b32 (128 B/clk).  The permutation of the tile's rows is undone where the accumulators are written out.
template <int R, int NTILE>
__device__ __forceinline__ void frag_mc(float (&out)[NTILE][4], const float* lds, int base, int li, int g, int h) {
  typedef float vec_t __attribute__((ext_vector_type(NTILE == 1 ? 1 : NTILE == 2 ? 2 : 4)));
  static_assert(NTILE == 1 || NTILE == 2 || NTILE == 4, "frag_mc: tiles per wave");
  const float* p = lds + (8 * g + 4 * h) * (R + 4) + base + NTILE * li;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if constexpr (NTILE == 1) {
      out[0][s] = p[s * (R + 4)];
    } else {
      // volatile: keeps LLVM from pairing two of these into one ds_read2_b64, which runs at half the rate of two ds_read_b64
      typedef __attribute__((address_space(3))) const volatile vec_t lds_vec_t;
      const vec_t v = *(lds_vec_t*)(p + s * (R + 4));
#pragma unroll
      for (int t = 0; t < NTILE; ++t) out[t][s] = v[t];
    }
  }
}

// ---- instruction-order hints for the pipelined main loop -----------------------------------------------
// One k-tile = NG k-groups of MF MFMAs.  The LDS writes of the next tile (NW ds_write_b128) and the fetch of
// the tile after it (NW buffer loads) are spread one per MFMA over the first k-group; the fragments of
// k-group g+1 are read while k-group g's MFMAs run.  (LLVM SchedGroupMask: MFMA 0x8, VMEM read 0x20,
// DS read 0x100, DS write 0x200.)
#define SGB(mask, n) __builtin_amdgcn_sched_group_barrier(mask, n, 0)
constexpr int cdiv_c(int a, int b) { return (a + b - 1) / b; }
// m-th of H MFMAs, each followed by its share of NI instructions of kind MASK
template <int m, int H, int NI, int MASK>
__device__ __forceinline__ void spread() {
  if constexpr (m < H) {
    SGB(0x8, 1);
    constexpr int c = cdiv_c((m + 1) * NI, H) - cdiv_c(m * NI, H);
    if constexpr (c > 0) SGB(MASK, c);
    spread<m + 1, H, NI, MASK>();
  }
}
template <int MF, int NW, int RPG, int NG>
__device__ __forceinline__ void sched_pattern() {
  static_assert(MF >= 2 && MF % 2 == 0, "sched_pattern: MFMAs per k-group");
  SGB(0x100, RPG);                       // fragments of k-group 0
  spread<0, MF / 2, NW, 0x200>();        // first half of k-group 0: LDS writes of the next tile
  if constexpr (NG > 1) SGB(0x100, RPG); // fragments of k-group 1
  spread<0, MF / 2, NW, 0x20>();         // second half: global fetch of the tile after next
  if constexpr (NG > 1) { if constexpr (NG > 2) SGB(0x100, RPG); SGB(0x8, MF); }
  if constexpr (NG > 2) { if constexpr (NG > 3) SGB(0x100, RPG); SGB(0x8, MF); }
  if constexpr (NG > 3) { if constexpr (NG > 4) SGB(0x100, RPG); SGB(0x8, MF); }
  if constexpr (NG > 4) { if constexpr (NG > 5) SGB(0x100, RPG); SGB(0x8, MF); }
  if constexpr (NG > 5) { if constexpr (NG > 6) SGB(0x100, RPG); SGB(0x8, MF); }
  if constexpr (NG > 6) { if constexpr (NG > 7) SGB(0x100, RPG); SGB(0x8, MF); }
  if constexpr (NG > 7) { SGB(0x8, MF); }
}
#undef SGB

}  // namespace
