// Multi-head self-attention for any token count, fp32 on v_mfma_f32_32x32x2_f32: K and V (and, in the backward, Q and dO) are streamed
// through LDS in 64-row tiles instead of being held whole, so N is not bounded by the 160 KB LDS (attention.hip keeps all of K and V of
// one (frame, head) and stops at N = 288).  Same conventions as attention.hip: q / k / v read straight out of the (B, N, 3*H*dh) to_qkv
// output, the output written in the merged-head (B, N, H*dh) layout, scores computed TRANSPOSED (S^T = K Q^T: a lane owns one query
// column, the accumulator registers hold keys), softmax in base 2 with the query pre-scaled by scale*log2(e), lse (B, H, N) in base-2
// units.
//
// Workgroup = 4 waves = one 128-row block (queries in the forward and the dQ pass, keys in the dK / dV pass) of one (frame, head); the
// other operand is walked in 64-row tiles through a DOUBLE-BUFFERED LDS image pair: every thread issues the global loads of tile t+1
// into registers, the waves compute on tile t, the registers go to the other image, one barrier.  A 64-row tile is exactly the key pair
// (kt, kt+1) one trip of attention.hip's general kernels consumes, in the same order: the arithmetic is the same, trip by trip.
//   forward  (wave = query tile):  online softmax across the key tiles, writes out and lse; only query tiles < nq are computed (nq = 1:
//                                  one wave per workgroup computes, the others only help stage K / V)
//   backward (1) dQ   (wave = query tile):  P^T = exp2(S^T - lse), dP^T = V dO^T, dS^T = P^T o (dP^T - delta) * scale, dQ^T += K^T dS^T;
//                                  also writes delta = rowsum(dO o O) of its rows to the scratch
//            (2) dK/dV (wave = key tile):   Q / dO / lse / delta tiles of the queries < nq streamed; P = exp2(S - lse), dP = dO V^T,
//                                  dV^T += dO^T P, dK^T += Q^T dS
// Every output element is written by exactly one lane of one workgroup, accumulated in a fixed order: no atomics, deterministic,
// and a frame's results do not depend on the other frames of the batch.
// LDS: 2 stages x (K, V) x 64 x (dh + 4) floats = 68 KB at dim_head 64 (+ 1 KB of lse / delta in the dK/dV pass): two workgroups
// (8 waves) per CU.
#include "common.h"
#include "kernels.h"
#include "attention_tiles.h"

namespace {

constexpr int LQ = 128;   // rows of the workgroup's own block (4 waves x 32)
constexpr int LK = 64;    // rows of one streamed tile

// one 64-row tile of two DH-wide column blocks: PER float4 per thread and matrix, loaded into registers (fetch) and written to an LDS
// image pair later (stash).  Rows >= nrows read row 0 and are zeroed by a multiply.
template <int DH>
struct TilePair {
  static constexpr int C4 = DH / 4, PER = LK * C4 / 256, SK = DH + 4;
  float4 a[PER], b[PER];
  __device__ __forceinline__ void fetch(const float* srcA, long long ldA, const float* srcB, long long ldB, int row0, int nrows, int tid) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int f = tid + j * 256, row = row0 + f / C4, c = (f % C4) * 4;
      const int rr = row < nrows ? row : 0;
      a[j] = *reinterpret_cast<const float4*>(srcA + rr * ldA + c);
      b[j] = *reinterpret_cast<const float4*>(srcB + rr * ldB + c);
    }
  }
  __device__ __forceinline__ void stash(float* dstA, float* dstB, int row0, int nrows, int tid) const {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int f = tid + j * 256, row = f / C4, c = (f % C4) * 4;
      const float k = row0 + row < nrows ? 1.f : 0.f;   // (a float4 ?: would be lowered through scratch memory)
      *reinterpret_cast<float4*>(dstA + row * SK + c) = make_float4(a[j].x * k, a[j].y * k, a[j].z * k, a[j].w * k);
      *reinterpret_cast<float4*>(dstB + row * SK + c) = make_float4(b[j].x * k, b[j].y * k, b[j].z * k, b[j].w * k);
    }
  }
};

// P^T (forward) or dP^T (dQ pass) o m / keep for the two 32-key halves of a 64-key tile (the general kernels' float4 groups: registers 4g .. 4g+3, one Philox call each)
__device__ __forceinline__ void drop_keys(f32x16& t0, f32x16& t1, bool two, int k00, int N, long long row4, const LayerDrop& drop, int h) {
  const unsigned long long sd = drop_seed(drop);
  const float inv = 1.0f / drop.keep;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int k0 = k00 + 8 * g + 4 * h;
    if (k0 < N) {
      const uint4 rb = drop_bits(row4 + k0 / 4, sd, drop.tag);
      t0[4 * g] *= drop_factor(rb.x, drop.keep, inv); t0[4 * g + 1] *= drop_factor(rb.y, drop.keep, inv);
      t0[4 * g + 2] *= drop_factor(rb.z, drop.keep, inv); t0[4 * g + 3] *= drop_factor(rb.w, drop.keep, inv);
    }
    if (two && k0 + 32 < N) {
      const uint4 rb = drop_bits(row4 + (k0 + 32) / 4, sd, drop.tag);
      t1[4 * g] *= drop_factor(rb.x, drop.keep, inv); t1[4 * g + 1] *= drop_factor(rb.y, drop.keep, inv);
      t1[4 * g + 2] *= drop_factor(rb.z, drop.keep, inv); t1[4 * g + 3] *= drop_factor(rb.w, drop.keep, inv);
    }
  }
}

// ------------------------------------------------------------------------------------ forward
// grid: (B * H) * ceil(nq / 128) workgroups, block index = item * nqb + query block
template <int DH, bool DROP>
__global__ void __launch_bounds__(256, 2) attn_fwd_tiled_kernel(const float* __restrict__ qkv, float* __restrict__ out, float* __restrict__ lse,
                                                                int N, int H, float scale, int nq, const LayerDrop drop) {
  constexpr int SK = DH + 4, DT = DH / 32, STAGE = 2 * LK * SK;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, h = lane >> 5;
  const int nqb = (nq + LQ - 1) / LQ;
  const int item = blockIdx.x / nqb, qb = blockIdx.x % nqb;
  const int b = item / H, hd = item % H;
  const int I = H * DH;
  const long long ld = 3ll * I;
  const float* base = qkv + (long long)b * N * ld + hd * DH;
  const float qscale = scale * DGVIT_LOG2E;
  const int q = qb * LQ + wave * 32 + li;
  const bool active = qb * LQ + wave * 32 < nq;   // wave-uniform: this wave's query tile holds a needed row
  const int nkt = (N + LK - 1) / LK;

  float4 qf[DH / 8];
  if (active) row_frags<DH>(qf, base + (q < nq ? q : 0) * ld, q < nq, h, qscale);
  TilePair<DH> tp;
  tp.fetch(base + I, ld, base + 2 * I, ld, 0, N, tid);
  tp.stash(smem, smem + LK * SK, 0, N, tid);
  __syncthreads();

  float m = -INFINITY, l = 0.f;
  f32x16 o[DT];
  zero_tiles<DT>(o);
#pragma unroll 1
  for (int t = 0; t < nkt; ++t) {
    if (t + 1 < nkt) tp.fetch(base + I, ld, base + 2 * I, ld, (t + 1) * LK, N, tid);   // in flight during the compute below
    const float* Ks = smem + (t & 1) * STAGE;
    const float* Vs = Ks + LK * SK;
    const int k00 = t * LK;
    if (active) {
      const bool two = k00 + 32 < N;   // wave-uniform
      f32x16 s0, s1;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s0[r] = 0.f;
        s1[r] = 0.f;
      }
      mfma_rows_x_frags<DH, SK>(s0, Ks, li, h, qf);
      if (two) mfma_rows_x_frags<DH, SK>(s1, Ks, 32 + li, h, qf);
      float mt = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = k00 + acc_row(r, h);
        const float v0 = key < N ? s0[r] : -INFINITY;
        const float v1 = (two && key + 32 < N) ? s1[r] : -INFINITY;
        s0[r] = v0;
        s1[r] = v1;
        mt = fmaxf(mt, fmaxf(v0, v1));
      }
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
      const float mn = fmaxf(m, mt);                       // every tile holds at least one real key: mn is finite
      const float alpha = __builtin_amdgcn_exp2f(m - mn);  // first tile: exp2(-inf) = 0
      float ts = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p0 = __builtin_amdgcn_exp2f(s0[r] - mn), p1 = __builtin_amdgcn_exp2f(s1[r] - mn);
        s0[r] = p0;
        s1[r] = p1;
        ts += p0 + p1;
      }
      ts += __shfl_xor(ts, 32, 64);
      l = l * alpha + ts;
      m = mn;
      if constexpr (DROP) drop_keys(s0, s1, two, k00, N, (((long long)b * H + hd) * N + q) * ((N + 3) / 4), drop, h);
      if (t > 0) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (k00 + acc_row(r, 0) >= N) continue;   // both keys of the step are padding (P = 0): wave-uniform skip
        const float* vrow = Vs + acc_row(r, h) * SK + li;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[dt * 32], s0[r], o[dt], 0, 0, 0);
      }
      if (two) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (k00 + 32 + acc_row(r, 0) >= N) continue;
          const float* vrow = Vs + (32 + acc_row(r, h)) * SK + li;
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[dt * 32], s1[r], o[dt], 0, 0, 0);
        }
      }
    }
    if (t + 1 < nkt) {
      float* nxt = smem + ((t + 1) & 1) * STAGE;   // last read in trip t - 1, before the barrier that ended it
      tp.stash(nxt, nxt + LK * SK, (t + 1) * LK, N, tid);
    }
    __syncthreads();
  }
  if (active && q < nq) {
    store_T<DH>(o, out + ((long long)b * N + q) * I + hd * DH, h, 1.f / l);
    if (lse && h == 0) lse[((long long)b * H + hd) * N + q] = m + __builtin_amdgcn_logf(l);   // base-2 log-sum-exp
  }
}

// ------------------------------------------------------------------------------------ backward (1): dQ, delta
template <int DH, bool DROP>
__global__ void __launch_bounds__(256, 2) attn_bwd_dq_tiled_kernel(const float* __restrict__ qkv, const float* __restrict__ o_fwd,
                                                                   const float* __restrict__ d_out, const float* __restrict__ lse,
                                                                   float* __restrict__ dqkv, float* __restrict__ delta_out, int N, int H,
                                                                   float scale, int nq, const LayerDrop drop) {
  constexpr int SK = DH + 4, DT = DH / 32, STAGE = 2 * LK * SK;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, h = lane >> 5;
  const int nqb = (nq + LQ - 1) / LQ;
  const int item = blockIdx.x / nqb, qb = blockIdx.x % nqb;
  const int b = item / H, hd = item % H;
  const int I = H * DH;
  const long long ld = 3ll * I;
  const float* base = qkv + (long long)b * N * ld + hd * DH;
  const float qscale = scale * DGVIT_LOG2E;
  const int q = qb * LQ + wave * 32 + li;
  const bool active = qb * LQ + wave * 32 < nq;
  const bool qv = q < nq;
  const int qc = qv ? q : 0;
  const int nkt = (N + LK - 1) / LK;

  float4 qf[DH / 8], dof[DH / 8];
  float delta = 0.f, lq = 0.f;
  if (active) {   // per-lane fragments of the query row, delta = rowsum(dO o O), lse of the row
    float4 of[DH / 8];
    row_frags<DH>(qf, base + qc * ld, qv, h, qscale);
    row_frags<DH>(dof, d_out + ((long long)b * N + qc) * I + hd * DH, qv, h, 1.f);
    row_frags<DH>(of, o_fwd + ((long long)b * N + qc) * I + hd * DH, qv, h, 1.f);
    lq = qv ? lse[((long long)b * H + hd) * N + qc] : 0.f;
    float d = 0.f;
#pragma unroll
    for (int g = 0; g < DH / 8; ++g) d += (dof[g].x * of[g].x + dof[g].y * of[g].y) + (dof[g].z * of[g].z + dof[g].w * of[g].w);
    delta = d + __shfl_xor(d, 32, 64);
    if (qv && h == 0) delta_out[((long long)b * H + hd) * N + q] = delta;
  }
  TilePair<DH> tp;
  tp.fetch(base + I, ld, base + 2 * I, ld, 0, N, tid);
  tp.stash(smem, smem + LK * SK, 0, N, tid);
  __syncthreads();

  f32x16 dq[DT];
  zero_tiles<DT>(dq);
#pragma unroll 1
  for (int t = 0; t < nkt; ++t) {
    if (t + 1 < nkt) tp.fetch(base + I, ld, base + 2 * I, ld, (t + 1) * LK, N, tid);
    const float* X = smem + (t & 1) * STAGE;   // K
    const float* Y = X + LK * SK;              // V
    const int k00 = t * LK;
    if (active) {
      const bool two = k00 + 32 < N;
      f32x16 s0, s1, dp0, dp1;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s0[r] = 0.f; s1[r] = 0.f; dp0[r] = 0.f; dp1[r] = 0.f;
      }
      mfma_rows_x_frags<DH, SK>(s0, X, li, h, qf);     // S^T (base-2 scaled)
      mfma_rows_x_frags<DH, SK>(dp0, Y, li, h, dof);   // dP^T[key][q] = sum_d V[key][d] dO[q][d]
      if (two) {
        mfma_rows_x_frags<DH, SK>(s1, X, 32 + li, h, qf);
        mfma_rows_x_frags<DH, SK>(dp1, Y, 32 + li, h, dof);
      }
      if constexpr (DROP) drop_keys(dp0, dp1, two, k00, N, (((long long)b * H + hd) * N + q) * ((N + 3) / 4), drop, h);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = k00 + acc_row(r, h);
        const float p0 = key < N ? __builtin_amdgcn_exp2f(s0[r] - lq) : 0.f;
        const float p1 = (two && key + 32 < N) ? __builtin_amdgcn_exp2f(s1[r] - lq) : 0.f;
        s0[r] = p0 * (dp0[r] - delta) * scale;                   // dS^T
        s1[r] = p1 * (dp1[r] - delta) * scale;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float* krow = X + acc_row(r, h) * SK + li;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) dq[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(krow[dt * 32], s0[r], dq[dt], 0, 0, 0);
      }
      if (two) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float* krow = X + (32 + acc_row(r, h)) * SK + li;
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) dq[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(krow[dt * 32], s1[r], dq[dt], 0, 0, 0);
        }
      }
    }
    if (t + 1 < nkt) {
      float* nxt = smem + ((t + 1) & 1) * STAGE;
      tp.stash(nxt, nxt + LK * SK, (t + 1) * LK, N, tid);
    }
    __syncthreads();
  }
  if (active && qv) store_T<DH>(dq, dqkv + ((long long)b * N + q) * ld + hd * DH, h, 1.f);
}

// ------------------------------------------------------------------------------------ backward (2): dK, dV
// grid: (B * H) * ceil(N / 128) workgroups; queries < nq are streamed (rows >= nq are zero in the images and masked: no gradient)
template <int DH, bool DROP>
__global__ void __launch_bounds__(256, 2) attn_bwd_dkv_tiled_kernel(const float* __restrict__ qkv, const float* __restrict__ d_out,
                                                                    const float* __restrict__ lse, const float* __restrict__ delta,
                                                                    float* __restrict__ dqkv, int N, int H, float scale, int nq,
                                                                    const LayerDrop drop) {
  constexpr int SK = DH + 4, DT = DH / 32, STAGE = 2 * LK * SK + 2 * LK;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, h = lane >> 5;
  const int nkb = (N + LQ - 1) / LQ;
  const int item = blockIdx.x / nkb, kb = blockIdx.x % nkb;
  const int b = item / H, hd = item % H;
  const int I = H * DH;
  const long long ld = 3ll * I;
  const float* base = qkv + (long long)b * N * ld + hd * DH;
  const float* dobase = d_out + (long long)b * N * I + hd * DH;
  const float* lbase = lse + ((long long)b * H + hd) * N;
  const float* dbase = delta + ((long long)b * H + hd) * N;
  const float qscale = scale * DGVIT_LOG2E;
  const int key = kb * LQ + wave * 32 + li;
  const bool active = kb * LQ + wave * 32 < N;   // wave-uniform: this wave's key tile holds a real key
  const bool kv = key < N;
  const int nqt = (nq + LK - 1) / LK;

  float4 kf[DH / 8], vf[DH / 8];
  if (active) {
    const int kc = kv ? key : 0;
    row_frags<DH>(kf, base + I + kc * ld, kv, h, 1.f);
    row_frags<DH>(vf, base + 2 * I + kc * ld, kv, h, 1.f);
  }
  // the row statistics of a query tile travel with its Q / dO rows: wave 0's lanes load one each
  TilePair<DH> tp;
  float ls = 0.f, ds = 0.f;
  auto fetch = [&](int t) {
    tp.fetch(base, ld, dobase, (long long)I, t * LK, nq, tid);
    if (tid < LK) {
      const int r = t * LK + tid;
      ls = r < nq ? lbase[r] : 0.f;
      ds = r < nq ? dbase[r] : 0.f;
    }
  };
  auto stash = [&](int t) {
    float* X = smem + (t & 1) * STAGE;
    tp.stash(X, X + LK * SK, t * LK, nq, tid);
    if (tid < LK) {
      X[2 * LK * SK + tid] = ls;
      X[2 * LK * SK + LK + tid] = ds;
    }
  };
  fetch(0);
  stash(0);
  __syncthreads();

  f32x16 dk[DT], dv[DT];
  zero_tiles<DT>(dk);
  zero_tiles<DT>(dv);
#pragma unroll 1
  for (int t = 0; t < nqt; ++t) {
    if (t + 1 < nqt) fetch(t + 1);
    const float* X = smem + (t & 1) * STAGE;   // Q
    const float* Y = X + LK * SK;              // dO
    const float* lse_s = Y + LK * SK;
    const float* del_s = lse_s + LK;
    if (active) {
#pragma unroll 1
      for (int sub = 0; sub < 2; ++sub) {
        const int q0 = t * LK + sub * 32;
        if (q0 >= nq) break;   // wave-uniform
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s[r] = 0.f;
          dp[r] = 0.f;
        }
        mfma_rows_x_frags<DH, SK>(s, X, sub * 32 + li, h, kf);   // S[q][key]
        mfma_rows_x_frags<DH, SK>(dp, Y, sub * 32 + li, h, vf);  // dP[q][key]
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ql = sub * 32 + acc_row(r, h), q = t * LK + ql;
          const float pv = (kv && q < nq) ? __builtin_amdgcn_exp2f(s[r] * qscale - lse_s[ql]) : 0.f;
          float mk = 1.f;   // (the lane owns a key and the registers hold queries: one Philox call per register, word key % 4)
          if constexpr (DROP) {
            if (kv && q < nq) {
              const uint4 rb = drop_bits((((long long)b * H + hd) * N + q) * ((N + 3) / 4) + key / 4, drop_seed(drop), drop.tag);
              const int w = key & 3;
              mk = drop_factor(w == 0 ? rb.x : w == 1 ? rb.y : w == 2 ? rb.z : rb.w, drop.keep, 1.0f / drop.keep);
            }
          }
          const float dsv = DROP ? pv * (dp[r] * mk - del_s[ql]) * scale : pv * (dp[r] - del_s[ql]) * scale;
          const float pd = DROP ? pv * mk : pv;
          const float* dorow = Y + ql * SK + li;
          const float* qrow = X + ql * SK + li;
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            dv[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(dorow[dt * 32], pd, dv[dt], 0, 0, 0);
            dk[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(qrow[dt * 32], dsv, dk[dt], 0, 0, 0);
          }
        }
      }
    }
    if (t + 1 < nqt) stash(t + 1);
    __syncthreads();
  }
  if (active && kv) {
    float* g = dqkv + ((long long)b * N + key) * ld + hd * DH;
    store_T<DH>(dk, g + I, h, 1.f);
    store_T<DH>(dv, g + 2 * I, h, 1.f);
  }
}

template <int DH, bool DROP>
int launch_fwd_tiled(const float* qkv, float* out, float* lse, int B, int N, int H, float scale, int nq, const LayerDrop& drop,
                     hipStream_t stream) {
  constexpr size_t lds = (size_t)2 * 2 * LK * (DH + 4) * sizeof(float);
  auto kern = attn_fwd_tiled_kernel<DH, DROP>;
  TRY((allow_dynamic_lds<attn_fwd_tiled_kernel<DH, DROP>>((int)lds, "attention_fwd_tiled")));
  const long long grid = (long long)B * H * ((nq + LQ - 1) / LQ);
  {
    ProfileScope t(PROF_ATTN_FWD, 4.0 * B * H * (double)nq * N * DH, stream);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), lds, stream, qkv, out, lse, N, H, scale, nq, drop);
  }
  DGVIT_CHECK_LAUNCH("attention_fwd_tiled");
  return DGVIT_OK;
}

template <int DH, bool DROP>
int launch_bwd_tiled(const float* qkv, const float* o, const float* dout, const float* lse, float* dqkv, float* delta, int B, int N, int H,
                     float scale, int nq, const LayerDrop& drop, hipStream_t stream) {
  constexpr size_t lds_dq = (size_t)2 * 2 * LK * (DH + 4) * sizeof(float);
  constexpr size_t lds_dkv = (size_t)2 * (2 * LK * (DH + 4) + 2 * LK) * sizeof(float);
  auto kdq = attn_bwd_dq_tiled_kernel<DH, DROP>;
  auto kdkv = attn_bwd_dkv_tiled_kernel<DH, DROP>;
  TRY((allow_dynamic_lds<attn_bwd_dq_tiled_kernel<DH, DROP>>((int)lds_dq, "attention_bwd_tiled")));
  TRY((allow_dynamic_lds<attn_bwd_dkv_tiled_kernel<DH, DROP>>((int)lds_dkv, "attention_bwd_tiled")));
  const long long gq = (long long)B * H * ((nq + LQ - 1) / LQ), gk = (long long)B * H * ((N + LQ - 1) / LQ);
  {
    ProfileScope t(PROF_ATTN_BWD, 8.0 * B * H * (double)nq * N * DH, stream);
    hipLaunchKernelGGL(kdq, dim3((unsigned)gq), dim3(256), lds_dq, stream, qkv, o, dout, lse, dqkv, delta, N, H, scale, nq, drop);
    hipLaunchKernelGGL(kdkv, dim3((unsigned)gk), dim3(256), lds_dkv, stream, qkv, dout, lse, (const float*)delta, dqkv, N, H, scale, nq, drop);
  }
  DGVIT_CHECK_LAUNCH("attention_bwd_tiled");
  return DGVIT_OK;
}

int check_tiled(const char* what, const float* qkv, int B, int N, int H, int dh, int nq) {
  DGVIT_CHECK_ARG(qkv && B > 0 && N > 0 && H > 0, "%s: bad arguments", what);
  DGVIT_CHECK_ARG(dh == 64 || dh == 32, "%s: unsupported dim_head=%d (64 or 32)", what, dh);
  DGVIT_CHECK_ARG(nq >= 1 && nq <= N, "%s: bad query count", what);
  // grid sizes (work-items of a launch < 2^32) and the row offsets (row * 3 * H * dh) of one frame in int
  DGVIT_CHECK_ARG((long long)B * H * ((N + LQ - 1) / LQ) < (1ll << 24) && (long long)N * 3 * H * dh < (1ll << 31), "%s: B*H*N too large", what);
  return DGVIT_OK;
}

}  // namespace

int attention_fwd_tiled(const float* qkv, float* out, float* lse, int B, int N, int H, int dh, int nq, hipStream_t stream, const LayerDrop* drop) {
  TRY(check_tiled("attention_fwd_tiled", qkv, B, N, H, dh, nq));
  DGVIT_CHECK_ARG(out, "attention_fwd_tiled: bad arguments");
  const float scale = 1.0f / sqrtf((float)dh);
  if (drop && drop->keep < 1.f) {
    DGVIT_CHECK_ARG(drop->keep > 0.f, "attention_fwd_tiled: dropout keep must be in (0, 1]");
    if (dh == 64) return launch_fwd_tiled<64, true>(qkv, out, lse, B, N, H, scale, nq, *drop, stream);
    return launch_fwd_tiled<32, true>(qkv, out, lse, B, N, H, scale, nq, *drop, stream);
  }
  const LayerDrop none = {1.f, 0u, 0ull, nullptr};
  if (dh == 64) return launch_fwd_tiled<64, false>(qkv, out, lse, B, N, H, scale, nq, none, stream);
  return launch_fwd_tiled<32, false>(qkv, out, lse, B, N, H, scale, nq, none, stream);
}

long long attention_bwd_tiled_scratch(int B, int N, int H) { return (long long)B * H * N; }

int attention_bwd_tiled(const float* qkv, const float* o, const float* dout, const float* lse, float* dqkv, float* scratch,
                        long long scratch_floats, int B, int N, int H, int dh, int nq, hipStream_t stream, const LayerDrop* drop) {
  TRY(check_tiled("attention_bwd_tiled", qkv, B, N, H, dh, nq));
  DGVIT_CHECK_ARG(o && dout && lse && dqkv && scratch, "attention_bwd_tiled: bad arguments");
  if (scratch_floats < attention_bwd_tiled_scratch(B, N, H))
    return dgvit_set_error(DGVIT_ERR_WORKSPACE, "attention_bwd_tiled: scratch %lld < %lld floats", scratch_floats, attention_bwd_tiled_scratch(B, N, H));
  const float scale = 1.0f / sqrtf((float)dh);
  if (drop && drop->keep < 1.f) {
    DGVIT_CHECK_ARG(drop->keep > 0.f, "attention_bwd_tiled: dropout keep must be in (0, 1]");
    if (dh == 64) return launch_bwd_tiled<64, true>(qkv, o, dout, lse, dqkv, scratch, B, N, H, scale, nq, *drop, stream);
    return launch_bwd_tiled<32, true>(qkv, o, dout, lse, dqkv, scratch, B, N, H, scale, nq, *drop, stream);
  }
  const LayerDrop none = {1.f, 0u, 0ull, nullptr};
  if (dh == 64) return launch_bwd_tiled<64, false>(qkv, o, dout, lse, dqkv, scratch, B, N, H, scale, nq, none, stream);
  return launch_bwd_tiled<32, false>(qkv, o, dout, lse, dqkv, scratch, B, N, H, scale, nq, none, stream);
}
