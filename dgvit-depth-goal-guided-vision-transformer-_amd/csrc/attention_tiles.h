// Register / LDS helpers shared by the fused attention kernels (attention.hip, N <= 288) and the K / V-tiled ones
// (attention_long.hip, any N): the 32x32 accumulator layout, per-lane row fragments, LDS staging and transposed stores.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
// softmax runs in base 2: the query is pre-scaled by scale*log2(e), so exp(x - max) = exp2(s' - max') on v_exp_f32
#define DGVIT_LOG2E 1.4426950408889634f

// Stage rows [0, nrows) of two DH-wide per-head column blocks into LDS images [NP][SK], zero padding rows.
// Every loop trip issues 2*CH float4 loads per thread before it writes LDS (a one-load-per-trip loop would
// serialise a memory round trip per float4).  Out-of-range rows read row 0 and are zeroed by a multiply.
template <int DH, int SK, int NTHR>
__device__ __forceinline__ void stage_pair(float* dstA, const float* srcA, long long ldA, float* dstB, const float* srcB,
                                           long long ldB, int nrows, int NP, int tid) {
  constexpr int C4 = DH / 4, CH = 8;   // 16 float4 in flight per thread: N <= 64 (and N <= 128 with 4 waves) stage in ONE trip
  const int total = NP * C4;
  for (int f0 = tid; f0 < total; f0 += NTHR * CH) {
    float4 va[CH], vb[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int f = f0 + j * NTHR;
      const int row = f / C4, c = (f % C4) * 4;
      const int rr = (f < total && row < nrows) ? row : 0;
      va[j] = *reinterpret_cast<const float4*>(srcA + rr * ldA + c);
      vb[j] = *reinterpret_cast<const float4*>(srcB + rr * ldB + c);
    }
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int f = f0 + j * NTHR;
      const int row = f / C4, c = (f % C4) * 4;
      if (f < total) {
        const float k = row < nrows ? 1.f : 0.f;   // (a float4 ?: would be lowered through scratch memory)
        *reinterpret_cast<float4*>(dstA + row * SK + c) = make_float4(va[j].x * k, va[j].y * k, va[j].z * k, va[j].w * k);
        *reinterpret_cast<float4*>(dstB + row * SK + c) = make_float4(vb[j].x * k, vb[j].y * k, vb[j].z * k, vb[j].w * k);
      }
    }
  }
}

// B-operand style fragments of one row (lane owns a row): elements [8g + 4h .. +3], g = 0..DH/8.
// `rowptr` must point at a readable row (callers clamp the row index); invalid rows are zeroed by a select.
template <int DH>
__device__ __forceinline__ void row_frags(float4 (&f)[DH / 8], const float* rowptr, bool valid, int h, float mul) {
  const float m = valid ? mul : 0.f;
#pragma unroll
  for (int g = 0; g < DH / 8; ++g) {
    const float4 v = *reinterpret_cast<const float4*>(rowptr + 8 * g + 4 * h);
    f[g] = make_float4(v.x * m, v.y * m, v.z * m, v.w * m);
  }
}

// acc += rowsA(LDS image, rows base+li) . fragsB   over the DH-deep contraction
template <int DH, int SK>
__device__ __forceinline__ void mfma_rows_x_frags(f32x16& acc, const float* img, int row, int h, const float4 (&fb)[DH / 8]) {
#pragma unroll
  for (int g = 0; g < DH / 8; ++g) {
    const float4 a = *reinterpret_cast<const float4*>(img + row * SK + 8 * g + 4 * h);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, fb[g].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, fb[g].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, fb[g].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, fb[g].w, acc, 0, 0, 0);
  }
}

// transposed accumulator tile (rows = d, cols = token on the lane) -> global row `tok`, 16-byte pieces along d
template <int DH>
__device__ __forceinline__ void store_T(const f32x16 (&o)[DH / 32], float* rowptr, int h, float mul) {
#pragma unroll
  for (int dt = 0; dt < DH / 32; ++dt)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float4 v = make_float4(o[dt][4 * c] * mul, o[dt][4 * c + 1] * mul, o[dt][4 * c + 2] * mul, o[dt][4 * c + 3] * mul);
      *reinterpret_cast<float4*>(rowptr + dt * 32 + 8 * c + 4 * h) = v;
    }
}

template <int DT>
__device__ __forceinline__ void zero_tiles(f32x16 (&t)[DT]) {
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) t[dt][r] = 0.f;
}

}  // namespace
