// The last transformer block with K and V folded into token 0's query.
//
// The head reads token 0 of the last block only (GoalFormer.py:167), and to_qkv has no bias, so with xn = LN1(x), W_k,h / W_v,h the
// head's dh x D row blocks of to_qkv.weight and s = dh^-1/2:
//     u_h = W_k,h^T q_h                  score_t = s q_h . k_t = s u_h . xn_t
//     p   = softmax_t(score)             r_h = sum_t p_t xn_t             o_h = W_v,h r_h  ( = sum_t p_t v_t )
// K and V never exist.  What touches every token is ONE pass over xn per direction (goal_pool_*: a frame's N x D rows staged in LDS
// once, shared by all heads); what touches the weights is a B-row, head-batched product (head_proj_*).  Backward, given do_h:
//     dr_h = W_v,h^T do_h                g_t = dr_h . xn_t,  c = sum_t p_t g_t,  da_t = p_t (g_t - c)
//     du_h = s sum_t da_t xn_t           dxn_t = sum_h (p_h,t dr_h + s da_h,t u_h)            dq_h = W_k,h du_h
//     dW_k,h = sum_b q_h du_h^T          dW_v,h = sum_b do_h r_h^T
// Every sum runs in a fixed order on plain FMAs (no atomics): two runs give the same bits.  Row offsets are 64-bit.
#include <math.h>

#include <algorithm>

#include "kernels.h"

#define DGVIT_LOG2E 1.4426950408889634f

namespace {

constexpr int GP_WAVES = 4;          // waves per goal_pool workgroup; each takes heads wave, wave + 4, ...
constexpr int GP_J = 4;              // float4 column chunks a lane may hold at most: D <= 4 * 64 * GP_J = 1024
constexpr int HP_FRAMES = 16;        // frames per head_proj workgroup
constexpr int HP_CHUNK = 256;        // floats of D a head_proj_t workgroup stages per step
constexpr int WG_ROWS = 8;           // weight rows per head_proj_wgrad workgroup

__device__ __forceinline__ float fma4(const float4 a, const float4 b, float acc) {   // one fixed-order chain
  acc = fmaf(a.x, b.x, acc);
  acc = fmaf(a.y, b.y, acc);
  acc = fmaf(a.z, b.z, acc);
  return fmaf(a.w, b.w, acc);
}
__device__ __forceinline__ void axpy4(float a, const float4 x, float4& acc) {
  acc.x = fmaf(a, x.x, acc.x);
  acc.y = fmaf(a, x.y, acc.y);
  acc.z = fmaf(a, x.z, acc.z);
  acc.w = fmaf(a, x.w, acc.w);
}

__device__ __forceinline__ void fma4v(const float4 a, const float4 b, float4& acc) {   // four independent chains
  acc.x = fmaf(a.x, b.x, acc.x);
  acc.y = fmaf(a.y, b.y, acc.y);
  acc.z = fmaf(a.z, b.z, acc.z);
  acc.w = fmaf(a.w, b.w, acc.w);
}
__device__ __forceinline__ float4 add4(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float hsum4(const float4 a) { return (a.x + a.y) + (a.z + a.w); }

// sum_t w[t] * xs[t][c] for this lane's float4 columns c = lane + 64 j: four chains over t (t mod 4 while four rows remain, the tail on
// chain 0), combined pairwise -- a fixed order whose rounding error grows like sqrt(N / 4), not sqrt(N)
template <int J>
__device__ __forceinline__ void pool_rows(const float* __restrict__ w, const float4* __restrict__ xs4, int N, int D4, int lane, float4 (&out)[J]) {
  float4 acc[4][J];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int j = 0; j < J; ++j) acc[k][j] = make_float4(0.f, 0.f, 0.f, 0.f);
  int t = 0;
  for (; t + 3 < N; t += 4) {
    const float4 wv = *reinterpret_cast<const float4*>(w + t);
    const float wk[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int c = lane + 64 * j;
        if (c < D4) axpy4(wk[k], xs4[(t + k) * D4 + c], acc[k][j]);
      }
  }
  for (; t < N; ++t) {
    const float wt = w[t];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int c = lane + 64 * j;
      if (c < D4) axpy4(wt, xs4[t * D4 + c], acc[0][j]);
    }
  }
#pragma unroll
  for (int j = 0; j < J; ++j) out[j] = add4(add4(acc[0][j], acc[1][j]), add4(acc[2][j], acc[3][j]));
}

// stage a frame's N x D rows (contiguous) into LDS with 16-byte loads
__device__ __forceinline__ void stage_frame(const float* __restrict__ xn, float4* __restrict__ xs4, int b, int N, int D) {
  const float4* src = reinterpret_cast<const float4*>(xn + (long long)b * N * D);
  const int n4 = N * (D >> 2);
  for (int i = threadIdx.x; i < n4; i += blockDim.x) xs4[i] = src[i];
}

// ------------------------------------------------------------------------------------------------ the pass over xn, forward
// grid B, 256 threads, LDS (N * D + GP_WAVES * NP) floats, NP = N rounded up to 4.  u, r: head h of frame b at b * fs + h * D.
// p (B, H, N) may be null (not kept).  J = float4 column chunks per lane: D <= 256 J.
template <int J>
__global__ void __launch_bounds__(64 * GP_WAVES) goal_pool_fwd_kernel(const float* __restrict__ xn, const float* __restrict__ u, long long fs_u,
                                                                      float* __restrict__ r, long long fs_r, float* __restrict__ p, int N,
                                                                      int D, int H, float qscale) {
  extern __shared__ float4 gp_smem[];
  float4* xs4 = gp_smem;
  const int b = blockIdx.x, D4 = D >> 2, NP = (N + 3) & ~3;
  float* sc = reinterpret_cast<float*>(gp_smem) + (long long)N * D + (threadIdx.x >> 6) * NP;   // this wave's scores, then probabilities
  stage_frame(xn, xs4, b, N, D);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (int h = threadIdx.x >> 6; h < H; h += GP_WAVES) {       // (wave-uniform; no workgroup barrier below)
    const float4* uh = reinterpret_cast<const float4*>(u + (long long)b * fs_u + (long long)h * D);
    float4 uf[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int c = lane + 64 * j;
      uf[j] = c < D4 ? uh[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int t = 0; t < N; ++t) {
      float part = 0.f;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int c = lane + 64 * j;
        if (c < D4) part = fma4(uf[j], xs4[t * D4 + c], part);
      }
      part = wave_sum(part);
      if (lane == 0) sc[t] = part * qscale;                    // base-2 scaled score
    }
    __builtin_amdgcn_wave_barrier();                           // (LDS accesses of a wave complete in order: its lanes see sc[])
    float m = -INFINITY;
    for (int t = lane; t < N; t += 64) m = fmaxf(m, sc[t]);
    m = wave_max(m);
    float l = 0.f;
    for (int t = lane; t < N; t += 64) {
      const float e = __builtin_amdgcn_exp2f(sc[t] - m);
      sc[t] = e;
      l += e;
    }
    l = wave_sum(l);
    const float inv = 1.f / l;
    for (int t = lane; t < N; t += 64) {
      const float pt = sc[t] * inv;
      sc[t] = pt;
      if (p) p[((long long)b * H + h) * N + t] = pt;
    }
    __builtin_amdgcn_wave_barrier();
    float4 acc[J];
    pool_rows<J>(sc, xs4, N, D4, lane, acc);
    float4* rh = reinterpret_cast<float4*>(r + (long long)b * fs_r + (long long)h * D);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int c = lane + 64 * j;
      if (c < D4) rh[c] = acc[j];
    }
  }
}

// ------------------------------------------------------------------------------------------------ the pass over xn, backward
// grid B, 256 threads, LDS (N * D + 2 * H * NP) floats.  Reads p (B, H, N), u and dr (head h of frame b at b * fs + h * D); writes du
// (same layout as dr) and EVERY row of dxn (B, N, D): dxn_t = sum_h (p_h,t dr_h + s da_h,t u_h), heads in ascending order.
template <int J>
__global__ void __launch_bounds__(64 * GP_WAVES) goal_pool_bwd_kernel(const float* __restrict__ xn, const float* __restrict__ p,
                                                                      const float* __restrict__ u, long long fs_u, const float* __restrict__ dr,
                                                                      float* __restrict__ du, long long fs_d, float* __restrict__ dxn, int N,
                                                                      int D, int H, float scale) {
  extern __shared__ float4 gp_smem[];
  float4* xs4 = gp_smem;
  const int b = blockIdx.x, D4 = D >> 2, NP = (N + 3) & ~3;
  float* ps = reinterpret_cast<float*>(gp_smem) + (long long)N * D;   // p[h][t]
  float* das = ps + H * NP;                                           // g[h][t], then s * da[h][t]
  stage_frame(xn, xs4, b, N, D);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (int h = threadIdx.x >> 6; h < H; h += GP_WAVES) {
    const float4* drh = reinterpret_cast<const float4*>(dr + (long long)b * fs_d + (long long)h * D);
    float4 df[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int c = lane + 64 * j;
      df[j] = c < D4 ? drh[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float* dh_ = das + h * NP;
    float* ph_ = ps + h * NP;
    for (int t = 0; t < N; ++t) {
      float part = 0.f;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int c = lane + 64 * j;
        if (c < D4) part = fma4(df[j], xs4[t * D4 + c], part);
      }
      part = wave_sum(part);
      if (lane == 0) dh_[t] = part;                                   // g_t
    }
    __builtin_amdgcn_wave_barrier();
    float cpart = 0.f;
    for (int t = lane; t < N; t += 64) {
      const float pt = p[((long long)b * H + h) * N + t];
      ph_[t] = pt;
      cpart = fmaf(pt, dh_[t], cpart);
    }
    const float cs = wave_sum(cpart);
    for (int t = lane; t < N; t += 64) dh_[t] = scale * (ph_[t] * (dh_[t] - cs));
    __builtin_amdgcn_wave_barrier();
    float4 acc[J];
    pool_rows<J>(dh_, xs4, N, D4, lane, acc);
    float4* duh = reinterpret_cast<float4*>(du + (long long)b * fs_d + (long long)h * D);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int c = lane + 64 * j;
      if (c < D4) duh[c] = acc[j];
    }
  }
  __syncthreads();
  // dxn: an item = 4 token rows x one float4 column; dr_h and u_h of the frame come through the caches (H * D floats each)
  const float4* dr4 = reinterpret_cast<const float4*>(dr + (long long)b * fs_d);
  const float4* u4 = reinterpret_cast<const float4*>(u + (long long)b * fs_u);
  float4* out4 = reinterpret_cast<float4*>(dxn + (long long)b * N * D);
  const int items = ((N + 3) >> 2) * D4;
  for (int it = threadIdx.x; it < items; it += blockDim.x) {
    const int t0 = (it / D4) * 4, c = it % D4;
    float4 acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int h = 0; h < H; ++h) {
      const float4 dv = dr4[h * D4 + c], uv = u4[h * D4 + c];
      const float4 pv = *reinterpret_cast<const float4*>(ps + h * NP + t0);      // (rows >= N of the padded tail are never stored)
      const float4 av = *reinterpret_cast<const float4*>(das + h * NP + t0);
      axpy4(pv.x, dv, acc[0]); axpy4(av.x, uv, acc[0]);
      axpy4(pv.y, dv, acc[1]); axpy4(av.y, uv, acc[1]);
      axpy4(pv.z, dv, acc[2]); axpy4(av.z, uv, acc[2]);
      axpy4(pv.w, dv, acc[3]); axpy4(av.w, uv, acc[3]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (t0 + k < N) out4[(t0 + k) * D4 + c] = acc[k];
  }
}

// ------------------------------------------------------------------------------------------------ head-batched products with the weights
// NN (M = B, N = D, K = dh per head): out[b][h][d] = sum_k in[b * ld_in + h * DH + k] * W[(h * DH + k) * D + d]
// (u from q and W_k; dr from do and W_v).  grid (ceil(B / 16), H), 256 threads; a thread owns output column d for 16 frames.
template <int DH>
__global__ void __launch_bounds__(256) head_proj_kernel(const float* __restrict__ in, long long ld_in, const float* __restrict__ W,
                                                        float* __restrict__ out, long long fs_out, int B, int D) {
  __shared__ float4 in_s[HP_FRAMES][DH / 4];
  const int b0 = blockIdx.x * HP_FRAMES, h = blockIdx.y;
  for (int i = threadIdx.x; i < HP_FRAMES * (DH / 4); i += 256) {
    const int f = i / (DH / 4), k4 = i % (DH / 4);
    in_s[f][k4] = b0 + f < B ? *reinterpret_cast<const float4*>(in + (long long)(b0 + f) * ld_in + h * DH + 4 * k4) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  for (int d = threadIdx.x; d < D; d += 256) {
    float4 acc[HP_FRAMES];                    // four chains over k (k mod 4), combined pairwise at the end
#pragma unroll
    for (int f = 0; f < HP_FRAMES; ++f) acc[f] = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* wp = W + (long long)h * DH * D + d;
#pragma unroll 2
    for (int k4 = 0; k4 < DH / 4; ++k4) {
      const float4 w = make_float4(wp[(long long)(4 * k4) * D], wp[(long long)(4 * k4 + 1) * D], wp[(long long)(4 * k4 + 2) * D],
                                   wp[(long long)(4 * k4 + 3) * D]);
#pragma unroll
      for (int f = 0; f < HP_FRAMES; ++f) fma4v(in_s[f][k4], w, acc[f]);
    }
#pragma unroll
    for (int f = 0; f < HP_FRAMES; ++f)
      if (b0 + f < B) out[(long long)(b0 + f) * fs_out + (long long)h * D + d] = hsum4(acc[f]);
  }
}

// NT (M = B, N = dh per head, K = D): out[b * ld_out + h * DH + j] = sum_d in[b][h][d] * W[(h * DH + j) * D + d]
// (o from r and W_v; dq from du and W_k).  grid (ceil(B / 16), H), 256 threads; thread (j, frame group) owns 16 * DH / 256 frames.
template <int DH>
__global__ void __launch_bounds__(256) head_proj_t_kernel(const float* __restrict__ in, long long fs_in, const float* __restrict__ W,
                                                          float* __restrict__ out, long long ld_out, int B, int D) {
  constexpr int FPT = HP_FRAMES * DH / 256;                 // frames per thread: 4 (dh 64) or 2 (dh 32)
  __shared__ float4 in_s[HP_FRAMES][HP_CHUNK / 4];
  const int b0 = blockIdx.x * HP_FRAMES, h = blockIdx.y;
  const int j = threadIdx.x % DH, f0 = (threadIdx.x / DH) * FPT;
  const float* wrow = W + ((long long)h * DH + j) * D;
  float4 acc[FPT][4];                         // sixteen chains over d (float4 column mod 4 x component), combined pairwise at the end
#pragma unroll
  for (int i = 0; i < FPT; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[i][k] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int d0 = 0; d0 < D; d0 += HP_CHUNK) {
    const int dc4 = (D - d0 < HP_CHUNK ? D - d0 : HP_CHUNK) >> 2;
    __syncthreads();
    for (int i = threadIdx.x; i < HP_FRAMES * dc4; i += 256) {
      const int f = i / dc4, c = i % dc4;
      in_s[f][c] = b0 + f < B ? *reinterpret_cast<const float4*>(in + (long long)(b0 + f) * fs_in + (long long)h * D + d0 + 4 * c)
                              : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    int c = 0;
    for (; c + 3 < dc4; c += 4) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float4 w = *reinterpret_cast<const float4*>(wrow + d0 + 4 * (c + k));
#pragma unroll
        for (int i = 0; i < FPT; ++i) fma4v(in_s[f0 + i][c + k], w, acc[i][k]);
      }
    }
    for (; c < dc4; ++c) {
      const float4 w = *reinterpret_cast<const float4*>(wrow + d0 + 4 * c);
#pragma unroll
      for (int i = 0; i < FPT; ++i) fma4v(in_s[f0 + i][c], w, acc[i][0]);
    }
  }
#pragma unroll
  for (int i = 0; i < FPT; ++i)
    if (b0 + f0 + i < B)
      out[(long long)(b0 + f0 + i) * ld_out + h * DH + j] = hsum4(add4(add4(acc[i][0], acc[i][1]), add4(acc[i][2], acc[i][3])));
}

// TN over the B frames, the K and the V row block in one launch (blockIdx.z):
//   dW[(z * I + h * DH + j) * D + d] = sum_b A_z[b * ld_z + h * DH + j] * X_z[b * fs_z + h * D + d]     A_0 = q, X_0 = du; A_1 = do, X_1 = r
// grid ((DH / 8) * ceil(D / 256), H, 2), 256 threads: 8 weight rows x 256 columns per workgroup; wave w sums its contiguous quarter of
// the frames in ascending order, then wave 0 adds the four partial sums in wave order.  Overwrites dW.
template <int DH>
__global__ void __launch_bounds__(256) head_proj_wgrad_kernel(const float* __restrict__ q, long long ld_q, const float* __restrict__ du,
                                                              long long fs_du, const float* __restrict__ dout, long long ld_do,
                                                              const float* __restrict__ r, long long fs_r, float* __restrict__ dW, int B,
                                                              int D, int H, int vec) {
  __shared__ float4 red[3][WG_ROWS][64];
  constexpr int RT = DH / WG_ROWS;
  const int z = blockIdx.z, h = blockIdx.y, rt = blockIdx.x % RT, cb = blockIdx.x / RT;
  const float* A = z ? dout : q;
  const long long lda = z ? ld_do : ld_q;
  const float* X = z ? r : du;
  const long long fsx = z ? fs_r : fs_du;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = cb * 64 + lane, D4 = D >> 2;
  const bool valid = c < D4;
  const int chunk = (B + 3) >> 2;
  const int bb = wave * chunk, be = bb + chunk < B ? bb + chunk : B;
  float4 acc[WG_ROWS];
#pragma unroll
  for (int i = 0; i < WG_ROWS; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (valid) {
    for (int b = bb; b < be; ++b) {
      const float4 x = *reinterpret_cast<const float4*>(X + (long long)b * fsx + (long long)h * D + 4 * c);
      const float* ap = A + (long long)b * lda + h * DH + rt * WG_ROWS;
      const float4 a0 = *reinterpret_cast<const float4*>(ap), a1 = *reinterpret_cast<const float4*>(ap + 4);
      axpy4(a0.x, x, acc[0]); axpy4(a0.y, x, acc[1]); axpy4(a0.z, x, acc[2]); axpy4(a0.w, x, acc[3]);
      axpy4(a1.x, x, acc[4]); axpy4(a1.y, x, acc[5]); axpy4(a1.z, x, acc[6]); axpy4(a1.w, x, acc[7]);
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int i = 0; i < WG_ROWS; ++i) red[wave - 1][i][lane] = acc[i];
  }
  __syncthreads();
  if (wave == 0 && valid) {
    const long long I = (long long)H * DH;
    float* o = dW + (z * I + (long long)h * DH + rt * WG_ROWS) * D + 4 * c;
#pragma unroll
    for (int i = 0; i < WG_ROWS; ++i) {
      float4 s = acc[i];
#pragma unroll
      for (int w = 0; w < 3; ++w) {
        const float4 v = red[w][i][lane];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
      }
      float* oi = o + (long long)i * D;
      if (vec) *reinterpret_cast<float4*>(oi) = s;
      else { oi[0] = s.x; oi[1] = s.y; oi[2] = s.z; oi[3] = s.w; }   // (a gradient tensor that is not 16-byte aligned)
    }
  }
}

template <int J>
int launch_pool_fwd(const float* xn, const float* u, long long fs_u, float* r, long long fs_r, float* p, int B, int N, int D, int H, float scale,
                    hipStream_t st) {
  auto kern = goal_pool_fwd_kernel<J>;
  TRY(allow_dynamic_lds<goal_pool_fwd_kernel<J>>((int)GOAL_POOL_LDS_MAX, "goal_pool_fwd"));
  const long long np = (N + 3) & ~3;
  const size_t lds = (size_t)((long long)N * D + GP_WAVES * np) * sizeof(float);
  {
    ProfileScope t(PROF_ATTN_FWD, 4.0 * B * H * (double)N * D, st);
    hipLaunchKernelGGL(kern, dim3(B), dim3(64 * GP_WAVES), lds, st, xn, u, fs_u, r, fs_r, p, N, D, H, scale * DGVIT_LOG2E);
  }
  DGVIT_CHECK_LAUNCH("goal_pool_fwd");
  return DGVIT_OK;
}

template <int J>
int launch_pool_bwd(const float* xn, const float* p, const float* u, long long fs_u, const float* dr, float* du, long long fs_d, float* dxn,
                    int B, int N, int D, int H, float scale, hipStream_t st) {
  auto kern = goal_pool_bwd_kernel<J>;
  TRY(allow_dynamic_lds<goal_pool_bwd_kernel<J>>((int)GOAL_POOL_LDS_MAX, "goal_pool_bwd"));
  const long long np = (N + 3) & ~3;
  const size_t lds = (size_t)((long long)N * D + 2ll * H * np) * sizeof(float);
  {
    ProfileScope t(PROF_ATTN_BWD, 8.0 * B * H * (double)N * D, st);
    hipLaunchKernelGGL(kern, dim3(B), dim3(64 * GP_WAVES), lds, st, xn, p, u, fs_u, dr, du, fs_d, dxn, N, D, H, scale);
  }
  DGVIT_CHECK_LAUNCH("goal_pool_bwd");
  return DGVIT_OK;
}

}  // namespace

// LDS bytes a goal_pool workgroup needs for a frame of N x D (the larger of the forward's and the backward's)
long long goal_pool_lds_bytes(int N, int D, int H) {
  const long long np = (N + 3) & ~3;
  const long long extra = std::max<long long>(GP_WAVES, 2ll * H) * np;
  return ((long long)N * D + extra) * (long long)sizeof(float);
}

bool goal_attention_supports(int N, int D, int H, int dh) {
  return N >= 1 && H >= 1 && D >= 4 && D % 4 == 0 && D <= 256 * GP_J && (dh == 32 || dh == 64) && goal_pool_lds_bytes(N, D, H) <= GOAL_POOL_LDS_MAX;
}

#define GOAL_CHECK_SHAPE(name)                                                                                                       \
  DGVIT_CHECK_ARG(B > 0 && goal_attention_supports(N, D, H, dh),                                                                    \
                  name ": unsupported shape B=%d N=%d H=%d dim_head=%d dim=%d (dim_head 32 or 64, dim a multiple of 4 up to 1024, "  \
                       "N * dim floats within %d KB of LDS)", B, N, H, dh, D, (int)(GOAL_POOL_LDS_MAX / 1024))

int head_proj(const float* in, long long ld_in, const float* W, float* out, long long fs_out, int B, int H, int dh, int D, hipStream_t st) {
  DGVIT_CHECK_ARG(in && W && out && al16(in) && ld_in % 4 == 0, "head_proj: bad arguments");
  const dim3 grid((B + HP_FRAMES - 1) / HP_FRAMES, H);
  {
    ProfileScope t(PROF_OTHER, 2.0 * B * H * (double)dh * D, st);
    if (dh == 64) hipLaunchKernelGGL(head_proj_kernel<64>, grid, dim3(256), 0, st, in, ld_in, W, out, fs_out, B, D);
    else hipLaunchKernelGGL(head_proj_kernel<32>, grid, dim3(256), 0, st, in, ld_in, W, out, fs_out, B, D);
  }
  DGVIT_CHECK_LAUNCH("head_proj");
  return DGVIT_OK;
}

int head_proj_t(const float* in, long long fs_in, const float* W, float* out, long long ld_out, int B, int H, int dh, int D, hipStream_t st) {
  DGVIT_CHECK_ARG(in && W && out && al16(in) && al16(W) && fs_in % 4 == 0, "head_proj_t: bad arguments");
  const dim3 grid((B + HP_FRAMES - 1) / HP_FRAMES, H);
  {
    ProfileScope t(PROF_OTHER, 2.0 * B * H * (double)dh * D, st);
    if (dh == 64) hipLaunchKernelGGL(head_proj_t_kernel<64>, grid, dim3(256), 0, st, in, fs_in, W, out, ld_out, B, D);
    else hipLaunchKernelGGL(head_proj_t_kernel<32>, grid, dim3(256), 0, st, in, fs_in, W, out, ld_out, B, D);
  }
  DGVIT_CHECK_LAUNCH("head_proj_t");
  return DGVIT_OK;
}

int goal_pool_fwd(const float* xn, const float* u, long long fs_u, float* r, long long fs_r, float* p, int B, int N, int D, int H,
                  float scale, hipStream_t st) {
  DGVIT_CHECK_ARG(xn && u && r && al16(xn) && al16(u) && al16(r) && fs_u % 4 == 0 && fs_r % 4 == 0, "goal_pool_fwd: bad arguments");
  if (D <= 256) return launch_pool_fwd<1>(xn, u, fs_u, r, fs_r, p, B, N, D, H, scale, st);
  if (D <= 512) return launch_pool_fwd<2>(xn, u, fs_u, r, fs_r, p, B, N, D, H, scale, st);
  return launch_pool_fwd<GP_J>(xn, u, fs_u, r, fs_r, p, B, N, D, H, scale, st);
}

int goal_pool_bwd(const float* xn, const float* p, const float* u, long long fs_u, const float* dr, float* du, long long fs_d, float* dxn,
                  int B, int N, int D, int H, float scale, hipStream_t st) {
  DGVIT_CHECK_ARG(xn && p && u && dr && du && dxn && al16(xn) && al16(u) && al16(dr) && al16(du) && al16(dxn) && fs_u % 4 == 0 && fs_d % 4 == 0,
                  "goal_pool_bwd: bad arguments");
  if (D <= 256) return launch_pool_bwd<1>(xn, p, u, fs_u, dr, du, fs_d, dxn, B, N, D, H, scale, st);
  if (D <= 512) return launch_pool_bwd<2>(xn, p, u, fs_u, dr, du, fs_d, dxn, B, N, D, H, scale, st);
  return launch_pool_bwd<GP_J>(xn, p, u, fs_u, dr, du, fs_d, dxn, B, N, D, H, scale, st);
}

// o = attention of token 0's query over K = xn W_k^T, V = xn W_v^T, without K or V: q (B rows at ldq, I) -> u, r (head h of frame b at
// b * fs_ur + h * D), p (B, H, N) or null, o (B rows at ldo, I).  wqkv = to_qkv.weight (3I, D).
int goal_attention_fwd(const float* xn, const float* wqkv, const float* q, long long ldq, float* o, long long ldo, float* u, float* r,
                       long long fs_ur, float* p, int B, int N, int H, int dh, int D, hipStream_t st) {
  GOAL_CHECK_SHAPE("goal_attention_fwd");
  DGVIT_CHECK_ARG(wqkv && al16(wqkv) && o, "goal_attention_fwd: bad arguments");
  const long long I = (long long)H * dh;
  const float scale = 1.0f / sqrtf((float)dh);
  TRY(head_proj(q, ldq, wqkv + I * D, u, fs_ur, B, H, dh, D, st));
  TRY(goal_pool_fwd(xn, u, fs_ur, r, fs_ur, p, B, N, D, H, scale, st));
  return head_proj_t(r, fs_ur, wqkv + 2 * I * D, o, ldo, B, H, dh, D, st);
}

// the data gradients: dout (B rows at lddo, I) -> dr, du (head h of frame b at b * fs_d + h * D), dq (B rows at lddq, I) and every row
// of dxn (B, N, D) (without W_q^T dq: the caller's token-0 GEMM adds it)
int goal_attention_bwd_data(const float* xn, const float* wqkv, const float* dout, long long lddo, const float* u, long long fs_ur,
                            const float* p, float* du, float* dr, long long fs_d, float* dq, long long lddq, float* dxn, int B, int N, int H,
                            int dh, int D, hipStream_t st) {
  GOAL_CHECK_SHAPE("goal_attention_bwd");
  DGVIT_CHECK_ARG(wqkv && al16(wqkv) && dq, "goal_attention_bwd: bad arguments");
  const long long I = (long long)H * dh;
  const float scale = 1.0f / sqrtf((float)dh);
  TRY(head_proj(dout, lddo, wqkv + 2 * I * D, dr, fs_d, B, H, dh, D, st));
  TRY(goal_pool_bwd(xn, p, u, fs_ur, dr, du, fs_d, dxn, B, N, D, H, scale, st));
  return head_proj_t(du, fs_d, wqkv + I * D, dq, lddq, B, H, dh, D, st);
}

// dW_k, dW_v -> dwkv (2I, D), overwritten (rows I..3I of the to_qkv gradient); dwkv == nullptr: the weight is frozen, nothing runs
int goal_attention_wgrad(const float* q, long long ldq, const float* dout, long long lddo, const float* du, long long fs_d, const float* r,
                         long long fs_ur, float* dwkv, int B, int H, int dh, int D, hipStream_t st) {
  if (!dwkv) return DGVIT_OK;
  DGVIT_CHECK_ARG(q && dout && du && r && B > 0 && H > 0 && (dh == 32 || dh == 64) && D > 0 && D % 4 == 0, "goal_attention_wgrad: bad arguments");
  DGVIT_CHECK_ARG(al16(q) && al16(dout) && al16(du) && al16(r) && ldq % 4 == 0 && lddo % 4 == 0 && fs_d % 4 == 0 && fs_ur % 4 == 0,
                  "goal_attention_wgrad: operands must be 16-byte aligned");
  const dim3 grid((dh / WG_ROWS) * ((D + 255) / 256), H, 2);
  {
    ProfileScope t(PROF_OTHER, 4.0 * B * H * (double)dh * D, st);
    if (dh == 64) hipLaunchKernelGGL(head_proj_wgrad_kernel<64>, grid, dim3(256), 0, st, q, ldq, du, fs_d, dout, lddo, r, fs_ur, dwkv, B, D, H, al16(dwkv) ? 1 : 0);
    else hipLaunchKernelGGL(head_proj_wgrad_kernel<32>, grid, dim3(256), 0, st, q, ldq, du, fs_d, dout, lddo, r, fs_ur, dwkv, B, D, H, al16(dwkv) ? 1 : 0);
  }
  DGVIT_CHECK_LAUNCH("head_proj_wgrad");
  return DGVIT_OK;
}
