// Attention maps: the softmax probabilities of one layer's attention (GoalFormer.py:77, taken before the dropout site :78), recomputed
// from the layer's (B, N, 3*H*dh) qkv buffer and the base-2 log-sum-exp (B, H, N) that every attention forward writes when it gets a
// pointer (fused, pipelined, one-query, K/V-tiled and the bf16 kernels alike):
//     P[q][k] = exp2(q.k * dh^-1/2 * log2(e) - lse[q])
// One pass, no reductions: the row statistics are the forward's own.  Two kernels, each for fp32 and for bf16 qkv (bf16 values are
// widened exactly; products and sums stay fp32, as in attention_bf16.hip's scores):
//   goal row  (query 0 of every (frame, head)): one wave per (frame, head), q0 staged in registers once, lane = key, key blocks of 64
//             for any N.  Reads K once (B*N*I elements per layer); stores N floats per (frame, head).
//   all rows: one workgroup per (frame, head, block of 32*NW queries), one wave per 32-query tile.  S^T = K Q^T on
//             v_mfma_f32_32x32x2_f32 in attention.hip's layout (lane = query column, accumulator registers = keys; K fragments read
//             straight from global memory, where every query block of the head finds them in cache), key tiles of 32 for any N, then
//             the exp2 epilogue goes through a per-wave LDS transpose so that 32 lanes store 128 contiguous bytes of one probability row.
//             Bound by its output, N*N floats per (frame, head): non-temporal stores keep the map stream from evicting the operands.
#include "attention_tiles.h"
#include "bf16.h"
#include "kernels.h"

namespace {

__device__ __forceinline__ float4 load4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 load4(const bf16_t* p) {   // four bf16 -> fp32 (exact)
  const uint2 u = *reinterpret_cast<const uint2*>(p);
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                     __uint_as_float(u.y & 0xffff0000u));
}
__device__ __forceinline__ float dot4(const float4 a, const float4 b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }

// probs[b * frame_stride + hd * N + k] = P[query 0][k] of (frame b, head hd)
template <int DH, typename T>
__global__ void __launch_bounds__(256) attn_probs_goal_kernel(const T* __restrict__ qkv, const float* __restrict__ lse,
                                                              float* __restrict__ probs, long long frame_stride, int N, int H, float qscale,
                                                              int items) {
  const int lane = threadIdx.x & 63, item = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= items) return;                                // (wave-uniform; no barriers in this kernel)
  const int b = item / H, hd = item - b * H, I = H * DH;
  const long long ld = 3ll * I;
  const T* base = qkv + (long long)b * N * ld + hd * DH;
  float4 q[DH / 4];                                         // q0 pre-scaled (every lane loads the same row: one request)
#pragma unroll
  for (int i = 0; i < DH / 4; ++i) {
    const float4 v = load4(base + 4 * i);
    q[i] = make_float4(v.x * qscale, v.y * qscale, v.z * qscale, v.w * qscale);
  }
  const float l0 = lse[(long long)item * N];
  float* out = probs + (long long)b * frame_stride + (long long)hd * N;
  for (int k0 = 0; k0 < N; k0 += 64) {
    const int key = k0 + lane;
    const T* krow = base + I + (long long)(key < N ? key : 0) * ld;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < DH / 4; ++i) s += dot4(q[i], load4(krow + 4 * i));
    if (key < N) __builtin_nontemporal_store(__builtin_amdgcn_exp2f(s - l0), out + key);
  }
}

// probs[b * frame_stride + (hd * N + q) * N + k] = P[q][k] of (frame b, head hd); blockDim = 64 * NW, NW <= 4
template <int DH, typename T>
__global__ void __launch_bounds__(256) attn_probs_all_kernel(const T* __restrict__ qkv, const float* __restrict__ lse,
                                                             float* __restrict__ probs, long long frame_stride, int N, int H, float qscale,
                                                             int nqb) {
  __shared__ float tile[4][32][33];                         // per wave: one 32 x 32 probability tile, [query][key] (+1: bank spread)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, h = lane >> 5;
  const int nw = blockDim.x >> 6;
  const int item = blockIdx.x / nqb, qb = blockIdx.x - item * nqb;
  const int b = item / H, hd = item - b * H, I = H * DH;
  const long long ld = 3ll * I;
  const T* base = qkv + (long long)b * N * ld + hd * DH;
  const int q0 = (qb * nw + wave) * 32, q = q0 + li;        // (a wave past the last query still takes part in the barriers)
  const bool qv = q < N;
  float4 qf[DH / 8];                                        // B-operand fragments of the lane's query row (row_frags' layout)
  {
    const T* qrow = base + (long long)(qv ? q : 0) * ld;
    const float m = qv ? qscale : 0.f;
#pragma unroll
    for (int g = 0; g < DH / 8; ++g) {
      const float4 v = load4(qrow + 8 * g + 4 * h);
      qf[g] = make_float4(v.x * m, v.y * m, v.z * m, v.w * m);
    }
  }
  const float lq = qv ? lse[(long long)item * N + q] : 0.f;
  float* out = probs + (long long)b * frame_stride + (long long)hd * N * N;
  float(*tw)[33] = tile[wave];
  const int nkt = (N + 31) / 32;
  for (int kt = 0; kt < nkt; ++kt) {
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
    const int key = kt * 32 + li;
    const T* krow = base + I + (long long)(key < N ? key : 0) * ld;
#pragma unroll
    for (int g = 0; g < DH / 8; ++g) {
      const float4 a = load4(krow + 8 * g + 4 * h);
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, qf[g].x, s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, qf[g].y, s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, qf[g].z, s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, qf[g].w, s, 0, 0, 0);
    }
    // s[r] = S^T[key kt*32 + acc_row(r, h)][query q0 + li]
#pragma unroll
    for (int r = 0; r < 16; ++r) tw[li][acc_row(r, h)] = __builtin_amdgcn_exp2f(s[r] - lq);
    __syncthreads();
    // half h of the wave stores rows 2 it + h: 32 lanes, 32 consecutive keys of one row
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int row = 2 * it + h, qr = q0 + row, kc = kt * 32 + li;
      if (qr < N && kc < N) __builtin_nontemporal_store(tw[row][li], out + (long long)qr * N + kc);
    }
    __syncthreads();
  }
}

template <int DH, typename T>
int launch_probs(const T* qkv, const float* lse, float* probs, long long frame_stride, int B, int N, int H, int rows, hipStream_t st) {
  const float qscale = 1.0f / sqrtf((float)DH) * DGVIT_LOG2E;   // (the attention kernels' scale * log2(e))
  const long long items = (long long)B * H;
  if (rows == DGVIT_MAPS_GOAL) {
    hipLaunchKernelGGL((attn_probs_goal_kernel<DH, T>), dim3((unsigned)((items + 3) / 4)), dim3(256), 0, st, qkv, lse, probs, frame_stride, N,
                       H, qscale, (int)items);
  } else {
    const int nqt = (N + 31) / 32, nw = nqt < 4 ? nqt : 4, nqb = (nqt + nw - 1) / nw;   // one wave per 32-query tile, <= 4 per workgroup
    DGVIT_CHECK_ARG(items * nqb < (1ll << 31), "attention maps: B*H*query blocks too large");
    hipLaunchKernelGGL((attn_probs_all_kernel<DH, T>), dim3((unsigned)(items * nqb)), dim3(64 * nw), 0, st, qkv, lse, probs, frame_stride, N,
                       H, qscale, nqb);
  }
  DGVIT_CHECK_LAUNCH("attention_probs");
  return DGVIT_OK;
}

int check_probs(const void* qkv, const float* lse, const float* probs, int B, int N, int H, int dh, int rows) {
  DGVIT_CHECK_ARG(qkv && lse && probs && B > 0 && N > 0 && H > 0, "attention maps: bad arguments");
  DGVIT_CHECK_ARG((long long)B * H < (1ll << 31), "attention maps: B*H too large");
  DGVIT_CHECK_ARG(rows == DGVIT_MAPS_GOAL || rows == DGVIT_MAPS_ALL, "attention maps: rows=%d must be DGVIT_MAPS_GOAL (0) or DGVIT_MAPS_ALL (1)", rows);
  return DGVIT_OK;
}

}  // namespace

int attention_probs(const float* qkv, const float* lse, float* probs, long long frame_stride, int B, int N, int H, int dh, int rows,
                    hipStream_t st) {
  TRY(check_probs(qkv, lse, probs, B, N, H, dh, rows));
  DGVIT_CHECK_ARG(dh == 64 || dh == 32, "attention maps: dim_head=%d unsupported (64 or 32)", dh);
  return dh == 64 ? launch_probs<64>(qkv, lse, probs, frame_stride, B, N, H, rows, st)
                  : launch_probs<32>(qkv, lse, probs, frame_stride, B, N, H, rows, st);
}

int attention_probs_bf16(const bf16_t* qkv, const float* lse, float* probs, long long frame_stride, int B, int N, int H, int dh, int rows,
                         hipStream_t st) {
  TRY(check_probs(qkv, lse, probs, B, N, H, dh, rows));
  DGVIT_CHECK_ARG(dh == 64, "attention maps (bf16): dim_head=%d unsupported (64)", dh);
  return launch_probs<64>(qkv, lse, probs, frame_stride, B, N, H, rows, st);
}

extern "C" int dgvit_attention_probs(const float* qkv, const float* lse, float* probs, int B, int N, int H, int dh, int rows, void* stream) {
  const long long frame = (long long)H * N * (rows == DGVIT_MAPS_ALL ? N : 1);
  return attention_probs(qkv, lse, probs, frame, B, N, H, dh, rows, (hipStream_t)stream);
}

extern "C" int dgvit_attention_probs_bf16(const unsigned short* qkv, const float* lse, float* probs, int B, int N, int H, int dh, int rows,
                                          void* stream) {
  const long long frame = (long long)H * N * (rows == DGVIT_MAPS_ALL ? N : 1);
  return attention_probs_bf16(qkv, lse, probs, frame, B, N, H, dh, rows, (hipStream_t)stream);
}
