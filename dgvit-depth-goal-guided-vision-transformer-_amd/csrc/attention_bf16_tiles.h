// Register / LDS helpers shared by the fused bf16 attention kernels (attention_bf16.hip, N <= 288) and the K / V-tiled ones
// (attention_bf16_long.hip, any N): the 32x32 accumulator layout, the LDS images and their fragment reads, the online-softmax step
// and the transposed stores.  The image layouts are described in the header of attention_bf16.hip.
#pragma once
#include "bf16.h"

namespace {

#define DGVIT_LOG2E 1.4426950408889634f
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
__device__ __forceinline__ int vt_pos(int key) {
  const int w = key & 15;
  return (key & ~15) | (((w >> 2) & 1) << 3) | ((w >> 3) << 2) | (w & 3);
}

// transposed fragment of a row-major [token][64] image (128-byte rows, chunk c of row r stored at c ^ (((r >> 1) & 1) << 2)):
// A[row = feature 32 dt + (lane & 31)][k = the 8 tokens 16 s + 8 (j >> 2) + 4 h + (j & 3)] of token tile `t0` -- the order
// in which a 32x32 accumulator's registers 8s .. 8s+7 present their rows (see the header).  Two ds_read_b64_tr_b16: per
// 16-lane group the hardware reads 4 tokens x 16 features and hands lane i feature i; the swizzle puts the four token rows
// on four different 64-byte bank groups.  EXEC must be all ones (uniform control flow only around this).
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* img, int t0, int dt, int s, int lane) {
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  const int w = lane & 15, q = w >> 2, p = w & 3, cb = (lane >> 4) & 1, h = lane >> 5;
  const int c = ((dt ^ ((q >> 1) & 1)) << 2) | (2 * cb + (p >> 1));
  const unsigned char* a = img + (t0 + 16 * s + 4 * h + q) * 128 + c * 16 + (p & 1) * 8;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)a);
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(a + 8 * 128));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// One key tile of the online softmax on a transposed score tile (a lane owns one query: 16 of its 32 keys in s0, the other 16 in the
// lane 32 away).  In: raw scores q.k; out: s0 = un-normalised probabilities exp2(score * sc - m), l and o brought to the running
// maximum m.  The kernel is bound by exactly this VALU work (MFMA-busy 0.15), so: the scale is folded into the exponent's fma
// (max of the raw scores, scaled once per row); keys >= N are masked in the last tile only; and the accumulator rescale is DEFERRED
// (cdna_hip_programming.md T13): m only moves when some query's tile maximum exceeds it by more than 2^DEFER in probability, so
// after the first tile the 32-register multiply of o almost never runs.  Probabilities then reach 2^DEFER instead of 1 -- the same
// relative precision in bf16, sums in fp32; the normalisation by l at the end is exact either way.
#define DGVIT_ATTN_DEFER 4.0f
template <int NT>
__device__ __forceinline__ void softmax_step(f32x16 (&s0)[NT], float& m, float& l, f32x16 (&o)[2], float sc, int kt, int nkt, int N, int h) {
  if (kt + NT == nkt && (N & 31)) {   // uniform: only the last tile has keys past N
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if ((nkt - 1) * 32 + acc_row(r, h) >= N) s0[NT - 1][r] = -INFINITY;
  }
  float mt = s0[0][0];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) mt = fmaxf(mt, s0[t][r]);
  mt = fmaxf(mt, __shfl_xor(mt, 32, 64)) * sc;         // (sc > 0; every tile holds at least one real key: finite)
  float alpha = 1.f;
  if (!__all(mt - m <= DGVIT_ATTN_DEFER)) {            // wave-uniform; always taken in the first tile (m = -inf)
    const float mn = fmaxf(m, mt);
    alpha = __builtin_amdgcn_exp2f(m - mn);            // first tile: exp2(-inf) = 0 (l and o are 0 there)
    m = mn;
    if (kt > 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        o[0][r] *= alpha;
        o[1][r] *= alpha;
      }
    }
  }
  float ts = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float pr = __builtin_amdgcn_exp2f(fmaf(s0[t][r], sc, -m));
      s0[t][r] = pr;
      ts += pr;
    }
  ts += __shfl_xor(ts, 32, 64);
  l = l * alpha + ts;
}

// The attention-dropout mask (site 0 of the table in common.h) of one row of the (b, h, q, k) probabilities, as the K / V-tiled kernels
// apply it: g0 = the float4 group of the row's key 0, ((b*H + h)*N + q) * ceil(N/4); group g0 + k/4 gives the keys k .. k+3.
struct RowDrop {
  long long g0;
  unsigned long long seed;
  uint32_t tag;
  float keep, inv;
  // the four factors (1/keep or 0) of keys 4 k4 .. 4 k4 + 3
  __device__ __forceinline__ void factors(int k4, float (&f)[4]) const {
    const uint4 r = drop_bits(g0 + k4, seed, tag);
    f[0] = drop_factor(r.x, keep, inv); f[1] = drop_factor(r.y, keep, inv); f[2] = drop_factor(r.z, keep, inv); f[3] = drop_factor(r.w, keep, inv);
  }
};

// NT (1 or 2) key tiles of one query tile: S^T = K Q^T (independent accumulator chains), the softmax step over all of them, O^T += V^T P^T.
// The images start at key row0 (a multiple of 32; 0: the whole head is in LDS): key tile kt is at image row kt * 32 - row0.
// DROP: the un-normalised probabilities are multiplied by mask / keep before they are rounded to bf16 (l and m stay undropped); registers
// 4g .. 4g+3 hold four consecutive keys aligned to 4 (acc_row), so one Philox block covers them.  Straight-line code: EXEC stays all ones.
template <int NT, bool DROP = false>
__device__ __forceinline__ void attn_key_tiles(const unsigned char* Ks, const unsigned char* Vs, const bf16x8 (&qf)[4], float& m, float& l, f32x16 (&o)[2],
                                               float sc, int kt, int nkt, int N, int li, int h, int lane, unsigned fsw, int row0 = 0,
                                               const RowDrop* rd = nullptr) {
  f32x16 s0[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) s0[t][r] = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(Ks + ((kt + t) * 32 - row0 + li) * 128 + (((2 * s + h) ^ fsw) * 16));
      s0[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qf[s], s0[t], 0, 0, 0);
    }
  softmax_step<NT>(s0, m, l, o, sc, kt, nkt, N, h);
  if constexpr (DROP) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float f[4];
        rd->factors((kt + t) * 8 + 2 * g + h, f);
#pragma unroll
        for (int i = 0; i < 4; ++i) s0[t][4 * g + i] *= f[i];
      }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    bf16x8 pf[2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) pf[s][j] = (__bf16)s0[t][8 * s + j];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(Vs, (kt + t) * 32 - row0, dt, s, lane), pf[s], o[dt], 0, 0, 0);
  }
}

// rows [0, N) of a 64-wide per-head column block -> LDS row image [NP][128 B], chunks swizzled by ((row >> 1) & 7).
// (staging loops request all of a thread's 16-byte loads before the first LDS write: a load-store-load-store loop would
//  serialise one memory round trip per chunk)
template <int NTHR>
__device__ __forceinline__ void stage_rows(unsigned char* img, const bf16_t* src, long long ld, int N, int NP, int tid) {
  constexpr int CH = 4;
  for (int f0 = tid; f0 < NP * 8; f0 += CH * NTHR) {
    u32x4_t v[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int f = f0 + j * NTHR, row = f >> 3, pc = f & 7;
      const bool ok = f < NP * 8 && row < N;
      v[j] = *reinterpret_cast<const u32x4_t*>(src + (ok ? row : 0) * ld + (pc ^ ((row >> 1) & 7)) * 8);
      if (!ok) v[j] = u32x4_t{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int f = f0 + j * NTHR;
      if (f < NP * 8) *reinterpret_cast<u32x4_t*>(img + (f >> 3) * 128 + (f & 7) * 16) = v[j];
    }
  }
}
// features 8 dc .. 8 dc + 7 of the rows `row` (even) and row + 1 -> the transposed image img[d][vt_pos(row)], row stride VS elements
__device__ __forceinline__ void put_transposed(bf16_t* img, int VS, int row, int dc, const u32x4_t& v0, const u32x4_t& v1) {
  unsigned* dst = reinterpret_cast<unsigned*>(img + (dc * 8) * VS + vt_pos(row));
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    dst[(2 * i) * (VS / 2)] = (v0[i] & 0xFFFFu) | (v1[i] << 16);
    dst[(2 * i + 1) * (VS / 2)] = (v0[i] >> 16) | (v1[i] & 0xFFFF0000u);
  }
}
// the same block transposed: img[d][vt_pos(row)], row stride VS elements (see the header of attention_bf16.hip)
template <int NTHR>
__device__ __forceinline__ void stage_transposed(bf16_t* img, const bf16_t* src, long long ld, int N, int NP, int VS, int tid) {
  constexpr int CH = 2;
  const int total = (NP / 2) * 8;
  for (int f0 = tid; f0 < total; f0 += CH * NTHR) {
    u32x4_t v0[CH], v1[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int f = f0 + j * NTHR, row = (f >> 3) * 2, dc = f & 7;
      const bool ok0 = f < total && row < N, ok1 = f < total && row + 1 < N;
      v0[j] = *reinterpret_cast<const u32x4_t*>(src + (ok0 ? row : 0) * ld + dc * 8);
      v1[j] = *reinterpret_cast<const u32x4_t*>(src + (ok1 ? row + 1 : 0) * ld + dc * 8);
      if (!ok0) v0[j] = u32x4_t{0u, 0u, 0u, 0u};
      if (!ok1) v1[j] = u32x4_t{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int f = f0 + j * NTHR, row = (f >> 3) * 2, dc = f & 7;
      if (f < total) {
        unsigned* dst = reinterpret_cast<unsigned*>(img + (dc * 8) * VS + vt_pos(row));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          dst[(2 * i) * (VS / 2)] = (v0[j][i] & 0xFFFFu) | (v1[j][i] << 16);
          dst[(2 * i + 1) * (VS / 2)] = (v0[j][i] >> 16) | (v1[j][i] & 0xFFFF0000u);
        }
      }
    }
  }
}

// acc += rows(img, tile base row `row0`) . frags   (A = 32 image rows x 64 deep, B = per-lane fragments)
__device__ __forceinline__ void mfma_rows(f32x16& acc, const unsigned char* img, int row0, int li, int h, const bf16x8 (&fb)[4]) {
  const unsigned fsw = (unsigned)((li >> 1) & 7);
  const unsigned char* rp = img + (row0 + li) * 128;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(rp + (((2 * s + h) ^ fsw) * 16));
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, fb[s], acc, 0, 0, 0);
  }
}
// acc[dt] += transposed(img)[d tile dt][32 contraction rows from `pos0`] . bf16(x)   (x = 32x32 fp32 tile, rows contracted)
__device__ __forceinline__ void mfma_transposed(f32x16 (&acc)[2], const bf16_t* img, int VS, int pos0, int li, int h, const f32x16& x) {
  bf16x8 xf[2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) xf[s][j] = (__bf16)x[8 * s + j];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(img + (dt * 32 + li) * VS + pos0 + 16 * s + 8 * h);
      acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, xf[s], acc[dt], 0, 0, 0);
    }
}
__device__ __forceinline__ void load_frags(bf16x8 (&f)[4], const bf16_t* rowptr, int h) {
#pragma unroll
  for (int s = 0; s < 4; ++s) f[s] = *reinterpret_cast<const bf16x8*>(rowptr + 16 * s + 8 * h);
}
// transposed accumulator pair (rows = d, token on the lane) -> bf16 row `rowptr` (64 wide)
__device__ __forceinline__ void store_T_bf16(const f32x16 (&o)[2], bf16_t* rowptr, int h, float mul) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      fx4 v = {o[dt][4 * c] * mul, o[dt][4 * c + 1] * mul, o[dt][4 * c + 2] * mul, o[dt][4 * c + 3] * mul};
      *reinterpret_cast<bf16x4*>(rowptr + dt * 32 + 8 * c + 4 * h) = __builtin_convertvector(v, bf16x4);
    }
}

}  // namespace
