// The replay ring's storage kernels (replay.DeviceReplayBuffer; the priority tree over the ring's slots is replay.hip).  A field is a
// (nrows, row) matrix; a frame field is fp32 (row = al4(H*W) floats) or, DESIGN 3.30, uint8 (row = al16(H*W) BYTES: the reference's frames
// are k/255 with k in 0..255, env_lab.py:420-434, and the fp32 frame is restored inside the gather).
//   gather_rows             : out[i] = src[idx[i]]                                          (replay sampling)
//   gather_rows_u8          : out[i][c] = (float)ring[idx[i]][c] / 255.0f
//   quantize_rows_u8        : ring[(start + i) % nrows][c] = q(src[i][c]),  q(x) = (uint8) rintf(fminf(fmaxf(x * 255, 0), 255)); an
//                             exported entry point that the Python package no longer calls
//   gather_shift_frames     : the gather with the DrQ random shift (replicate-pad by `pad`, crop at a per-sample offset) folded in
//   gather_shift_frames_u8  : the same kernel template over a byte ring: one draw, one set of clamps
//   ring_mark               : the per-slot episode flags after a store: the written slots forget their marks, the newest one is the HEAD
//   nstep_walk              : the n-step return of each sampled slot: a walk along the ring that stops at done, at a flag or after n slots,
//                             one wave per sample, the rewards summed in double in ascending order
//   ring_store_frames       : both frame fields of n slots -- add, add_batch (n may cross the ring's end) or one vector step of E
//                             environments -- from device memory, fp32 or uint8 source, either ring
//   ring_store_small        : their five small fields and, for one step, its marks (HEAD | END per environment) in one launch
//   nstep_walk_strided      : nstep_walk along one environment's slots, (i + k E) mod nrows
//   ring_plan_next          : the ring that stores each frame once: which arena row holds each slot's next_obs after a store,
//                             the FIFO of the terminal pool, and the store's move list -- one wave, 64 rows a round
//   ring_store_frames_shared: the obs rows, the moves into the pool and the pending rows of that store in one launch
//   ring_next_rows          : out[i] = next_row[idx[i]], the index tensor of the next_obs gather over the arena
//   ring_export             : the store path's mirror: ages [a0, a0 + n) of the ring, every field, the END bits and the
//                             leaves packed densely, field-major, into one device buffer -- the chunk of a save_transitions file
//   ring_stack_rows         : frame stacks at sample time: the n-step walk backward -- for each sampled slot the rows of its
//                             K newest frames inside its episode, one wave per sample, for obs and for next_obs
//   gather_stack_frames     : out[i][p][c] = frame c of sample i at pixel p, the channel-last (B, H, W, K) stack, from a row table; the last
//                             channel may come from a second matrix (next_obs); fp32 or byte ring
//   gather_shift_stack_frames: the same with ONE random shift per sample applied to all K channels, the draw of gather_shift_frames
//   frame_stack_push        : the acting side's stack (replay.FrameStack): every pixel's K channels move down by one, the new frame on top
// The dequantisation is the correctly rounded DIVISION: k * (1.0f / 255.0f) alone differs from numpy's and CPU torch's uint8 -> float / 255
// in 126 of the 256 codes (dequant_u8 below repairs it with one Newton step).  One dword (4 pixels) of a byte ring per thread, one float4 of
// the fp32 side: 256-B and 1-KiB wave accesses.  Columns at or beyond `cols` of every row written (ring or out) are zeros, whatever the
// other side holds there.
#include <math.h>

#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace {

// a sampled index as a ring row: clamp instead of faulting on a bad index
__device__ __forceinline__ long long ring_row(long long s, long long nrows) { return s < 0 ? 0 : (s >= nrows ? nrows - 1 : s); }

// fl(k / 255) for k in 0..255 without the division's v_rcp_f32 and ten-instruction expansion, four times per thread: q = fl(k * fl(1/255))
// is within an ulp, r = k - 255 q is exact in one fma, and q + r * fl(1/255) rounds to the quotient -- the last step of the division's
// own expansion.  Equal to (float)k / 255.0f on all 256 codes: tests/test_replay_u8_host.py restates the three operations in exact
// rational arithmetic, tests/test_gpu_replay_u8.py compares every code on the device.
__device__ __forceinline__ float dequant_u8(uint32_t k) {
  constexpr float RINV = 0x1.010102p-8f;   // fl(1 / 255) = 0x3b808081
  const float x = (float)k, q = x * RINV;
  return fmaf(fmaf(-q, 255.0f, x), RINV, q);
}

// rintf rounds half to even; fmaxf(NaN, 0) = 0, so NaN stores 0; -0 and -inf store 0, +inf stores 255
__device__ __forceinline__ uint32_t quant_u8(float x) { return (uint32_t)rintf(fminf(fmaxf(x * 255.0f, 0.0f), 255.0f)); }

// out[i][:] = src[idx[i]][:] for rows of `row4` float4
__global__ void __launch_bounds__(256) gather_rows_kernel(const float* __restrict__ src, const long long* __restrict__ idx,
                                                          float* __restrict__ out, long long total4, int row4, long long nrows) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const long long r = i / row4;
  const int c = (int)(i % row4);
  const long long s = ring_row(idx[r], nrows);
  reinterpret_cast<float4*>(out)[i] = reinterpret_cast<const float4*>(src)[s * row4 + c];
}

// thread = one float4 of an output row; the ring dword behind it exists whenever 4c < cols (row_bytes >= al4(cols))
__global__ void __launch_bounds__(256) gather_rows_u8_kernel(const unsigned char* __restrict__ ring, const long long* __restrict__ idx,
                                                             float* __restrict__ out, long long total4, int out4, int cols,
                                                             long long row_bytes, long long nrows) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const long long r = i / out4;
  const int c = (int)(i - r * out4), p0 = 4 * c;
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (p0 < cols) {
    const long long s = ring_row(idx[r], nrows);
    const uint32_t w = *reinterpret_cast<const uint32_t*>(ring + s * row_bytes + p0);
    o.x = dequant_u8(w & 255u);
    if (p0 + 1 < cols) o.y = dequant_u8((w >> 8) & 255u);
    if (p0 + 2 < cols) o.z = dequant_u8((w >> 16) & 255u);
    if (p0 + 3 < cols) o.w = dequant_u8(w >> 24);
  }
  reinterpret_cast<float4*>(out)[i] = o;
}

// thread = one dword of a ring row.  VEC: src rows are 16-byte aligned (src_ld % 4 == 0 and an aligned base), a whole group is one float4.
// This is the fp32 -> uint8 case of ring_store_frames_kernel<true> below for one field, and is kept beside it: launched in its place
// (gridDim.y = 1) that kernel took 10.3 us where this one takes 9.8 us on 512 rows of 128 x 160
template <bool VEC>
__global__ void __launch_bounds__(256) quantize_rows_u8_kernel(const float* __restrict__ src, long long src_ld, uint32_t* __restrict__ ring,
                                                               long long total4, int row4, int cols, long long nrows, long long start) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const long long r = i / row4;
  const int c = (int)(i - r * row4), p0 = 4 * c;
  long long d = start + r;      // start < nrows and r < n <= nrows: one subtraction wraps the ring
  if (d >= nrows) d -= nrows;
  const float* __restrict__ s = src + r * src_ld + p0;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (VEC && p0 + 4 <= cols) {
    const float4 t = *reinterpret_cast<const float4*>(s);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (p0 + e < cols) v[e] = s[e];
  }
  ring[d * row4 + c] = quant_u8(v[0]) | (quant_u8(v[1]) << 8) | (quant_u8(v[2]) << 16) | (quant_u8(v[3]) << 24);   // q(0) = 0: the padding
}

// The row stride of the shifted gather's source, in elements: a byte ring's is an argument; the fp32 ring's is the output's, 4 * row4, and
// an argument of its own would only grow that kernel's kernarg segment.
struct row4_stride {};
template <typename T>
using src_stride = std::conditional_t<std::is_same_v<T, float>, row4_stride, long long>;

// the (dy, dx) of sample r in [-pad, pad]^2: one Philox draw per sample and tag, shared by the single-frame and the stacked shifted gather
__device__ __forceinline__ void shift_draw(long long r, int pad, uint32_t tag, unsigned long long seed,
                                           const unsigned long long* __restrict__ seed_dev, int& dy, int& dx) {
  dy = 0, dx = 0;
  if (pad > 0) {
    if (seed_dev) seed = *seed_dev;   // graph-capturable form, as dropout_kernel
    const uint4 rb = drop_bits(r, seed, tag);
    const uint32_t span = 2u * (uint32_t)pad + 1u;
    dy = (int)__umulhi(rb.x, span) - pad;
    dx = (int)__umulhi(rb.y, span) - pad;
  }
}

// out[i][y][x] = fp32(src[idx[i]][clamp(y + dy_i)][clamp(x + dx_i)]): the gather with a per-sample integer shift in [-pad, pad]^2
// (F.pad(mode="replicate", pad) then a crop at (pad + dy, pad + dx)); columns H*W .. 4 * row4 of out are written as zeros.  T = float or
// unsigned char is the ring's element; the draw does not depend on it, so one seed gives both rings one shift table.
// blockIdx.x is the sample, so its index, seed and Philox draw are wave-uniform (scalar unit); blockIdx.y * 256 + threadIdx.x is the
// float4 group of the output row.  A group may straddle image rows (W % 4 != 0): y and x advance per element.
template <typename T>
__global__ void __launch_bounds__(256) gather_shift_frames_kernel(const T* __restrict__ src, const long long* __restrict__ idx,
                                                                  float* __restrict__ out, int* __restrict__ shifts_out, int row4,
                                                                  src_stride<T> ld, long long nrows, int H, int W, int pad, uint32_t tag,
                                                                  unsigned long long seed,
                                                                  const unsigned long long* __restrict__ seed_dev) {
  const int c = (int)blockIdx.y * 256 + (int)threadIdx.x;
  if (c >= row4) return;
  const long long r = blockIdx.x;
  const long long s = ring_row(idx ? idx[r] : r, nrows);
  int dy, dx;
  shift_draw(r, pad, tag, seed, seed_dev, dy, dx);
  if (shifts_out && c == 0) {
    shifts_out[2 * r] = dy;
    shifts_out[2 * r + 1] = dx;
  }
  const T* __restrict__ frame;
  if constexpr (std::is_same_v<T, float>) frame = src + s * (4ll * row4);
  else frame = src + s * ld;
  const unsigned p0 = 4u * (unsigned)c;
  int y = (int)(p0 / (unsigned)W), x = (int)(p0 - (unsigned)y * (unsigned)W);
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int sy = min(max(y + dy, 0), H - 1), sx = min(max(x + dx, 0), W - 1);
    // the source pixel is always inside the frame (clamped; H * W <= 2^25): loaded unconditionally, no branch per element; y >= H are the
    // padding columns behind the frame.  Each element type keeps its kernel's own line, conversion and index width: through a shared
    // conversion helper the fp32 instantiation grows by 5 instructions
    if constexpr (std::is_same_v<T, float>) {
      const float t = frame[(long long)sy * W + sx];
      v[e] = y < H ? t : 0.f;
    } else {
      const uint32_t t = frame[sy * W + sx];
      v[e] = y < H ? dequant_u8(t) : 0.f;
    }
    if (++x == W) { x = 0; ++y; }
  }
  reinterpret_cast<float4*>(out)[r * row4 + c] = make_float4(v[0], v[1], v[2], v[3]);
}

// Episode flags, one byte per slot.  END: the slot's transition is the last of its episode; HEAD: the slot is the newest one
// written, its ring successor is the oldest slot or an unwritten one.  A walk stops behind any slot whose byte is not zero.
constexpr unsigned char RING_END = 1, RING_HEAD = 2;
constexpr int NSTEP_MAX = 64;   // one lane per visited slot

// thread j < n: slot (start + j) % nrows forgets its marks, the last one becomes the HEAD; thread n: the slot before `start` is no longer
// the newest and keeps only its END -- unless the store covered the whole ring, in which case that slot has just been written
__global__ void __launch_bounds__(256) ring_mark_kernel(unsigned char* __restrict__ flags, long long nrows, long long start, long long n) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j < n) {
    long long d = start + j;    // start < nrows and j < n <= nrows: one subtraction wraps the ring
    if (d >= nrows) d -= nrows;
    flags[d] = j == n - 1 ? RING_HEAD : 0;
  } else if (j == n && n < nrows) {
    const long long p = start > 0 ? start - 1 : nrows - 1;
    flags[p] &= RING_END;
  }
}

// One wave per sample (4 per workgroup), as per_sample_kernel.  Lane k < n loads rew, done and flags of slot s_k = (i + k) mod nrows, so
// the walk is one memory round trip; the ballot of the stop predicate gives m, the slots visited; the sum runs over lanes < m in ascending
// order in double, every lane the same arithmetic; then the lanes copy the next_small row of the last slot.  Every slot index is reduced
// mod nrows and i is clamped: nothing here can address outside the ring.  No atomics: the result is a function of the ring and idx[b].
// the walk of wave w once lane k knows its slot s = s_k < nrows: shared by the two kernels below, which differ in s_k alone
__device__ __forceinline__ void nstep_walk_from(long long s, long long w, int lane, const float* __restrict__ rew, long long rew_ld,
                                                const float* __restrict__ done, long long done_ld, const unsigned char* __restrict__ flags,
                                                const float4* __restrict__ next_small, int small4, int n, double gamma,
                                                float* __restrict__ ret_out, float* __restrict__ done_out, float* __restrict__ discount_out,
                                                float4* __restrict__ next_small_out, int* __restrict__ steps_out,
                                                long long* __restrict__ tail_out) {
  const bool active = lane < n;
  const float r = active ? rew[s * rew_ld] : 0.f;
  const float d = active ? done[s * done_ld] : 0.f;
  const unsigned f = active ? (unsigned)flags[s] : 0u;
  const unsigned long long stop = __ballot(active && (d != 0.f || f != 0u || lane == n - 1));   // lane n - 1 always stops: never empty
  const int m = __ffsll((long long)stop);
  double acc = 0.0, g = 1.0;
  for (int k = 0; k < m; ++k) {     // m is wave-uniform
    acc += g * (double)__shfl(r, k, 64);
    g *= gamma;
  }
  const long long tail = __shfl(s, m - 1, 64);
  const float dm = __shfl(d, m - 1, 64);
  if (lane == 0) {
    ret_out[w] = (float)acc;
    done_out[w] = dm;
    discount_out[w] = (float)g;
    steps_out[w] = m;
    tail_out[w] = tail;
  }
  for (int c = lane; c < small4; c += 64) next_small_out[w * small4 + c] = next_small[tail * small4 + c];
}

__global__ void __launch_bounds__(256) nstep_walk_kernel(const float* __restrict__ rew, long long rew_ld, const float* __restrict__ done,
                                                         long long done_ld, const unsigned char* __restrict__ flags,
                                                         const float4* __restrict__ next_small, int small4, const long long* __restrict__ idx,
                                                         long long nsel, long long nrows, int n, double gamma, float* __restrict__ ret_out,
                                                         float* __restrict__ done_out, float* __restrict__ discount_out,
                                                         float4* __restrict__ next_small_out, int* __restrict__ steps_out,
                                                         long long* __restrict__ tail_out) {
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= nsel) return;       // wave-uniform
  long long s = ring_row(idx[w], nrows) + lane;
  if (nrows >= NSTEP_MAX) {    // s < 2 nrows: one subtraction wraps the ring
    if (s >= nrows) s -= nrows;
  } else {
    s = (long long)((unsigned)s % (unsigned)nrows);   // a ring shorter than the walk: s < 128
  }
  nstep_walk_from(s, w, lane, rew, rew_ld, done, done_ld, flags, next_small, small4, n, gamma, ret_out, done_out, discount_out, next_small_out,
                  steps_out, tail_out);
}

// The walk in a ring of `stride` parallel environments: s_k = (i + k * stride) mod nrows.  i < nrows and k * stride <=
// 63 * stride, so where 63 * stride <= nrows (wave-uniform: a ring of at least 63 steps) one subtraction wraps; a shorter ring, down to
// nrows == stride where every lane visits slot i, takes the 64-bit remainder.  stride == 1 gives nstep_walk_kernel's slots.
__global__ void __launch_bounds__(256) nstep_walk_strided_kernel(const float* __restrict__ rew, long long rew_ld,
                                                                 const float* __restrict__ done, long long done_ld,
                                                                 const unsigned char* __restrict__ flags,
                                                                 const float4* __restrict__ next_small, int small4,
                                                                 const long long* __restrict__ idx, long long nsel, long long nrows,
                                                                 long long stride, int n, double gamma, float* __restrict__ ret_out,
                                                                 float* __restrict__ done_out, float* __restrict__ discount_out,
                                                                 float4* __restrict__ next_small_out, int* __restrict__ steps_out,
                                                                 long long* __restrict__ tail_out) {
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= nsel) return;       // wave-uniform
  long long s = ring_row(idx[w], nrows) + lane * stride;   // stride <= nrows < 2^56 (launcher): no overflow
  if ((NSTEP_MAX - 1) * stride <= nrows) {
    if (s >= nrows) s -= nrows;
  } else {
    s = (long long)((unsigned long long)s % (unsigned long long)nrows);
  }
  nstep_walk_from(s, w, lane, rew, rew_ld, done, done_ld, flags, next_small, small4, n, gamma, ret_out, done_out, discount_out, next_small_out,
                  steps_out, tail_out);
}

// One frame field of ring_store_frames: where its rows come from.  vec: whole groups may be read at once (16-byte aligned fp32 rows,
// 4-byte aligned uint8 rows); otherwise element by element.
struct frame_src {
  const void* p;
  long long ld;   // elements between rows
  int u8, vec;
};

// Both frame fields of a vector step in one launch: blockIdx.y is the field, so its source, element type and alignment are
// wave-uniform; thread = one group of 4 pixels of a ring row, a float4 of an fp32 ring or a dword of a byte ring.  Pixels at or beyond
// `cols` are never read and are written as zeros (q(0) = 0).  start + r wraps as in quantize_rows_u8_kernel.
template <bool RING_U8>
__global__ void __launch_bounds__(256) ring_store_frames_kernel(frame_src s0, frame_src s1, void* __restrict__ ring0, void* __restrict__ ring1,
                                                                long long total4, int row4, int cols, long long nrows, long long start) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const frame_src s = blockIdx.y == 0 ? s0 : s1;
  void* __restrict__ ring = blockIdx.y == 0 ? ring0 : ring1;
  const long long r = i / row4;
  const int c = (int)(i - r * row4), p0 = 4 * c;
  long long d = start + r;      // start < nrows and r < n <= nrows: one subtraction wraps the ring
  if (d >= nrows) d -= nrows;
  const bool whole = s.vec && p0 + 4 <= cols;
  if (RING_U8 && s.u8) {        // codes as they are
    const unsigned char* __restrict__ b = static_cast<const unsigned char*>(s.p) + r * s.ld + p0;
    uint32_t w = 0;
    if (whole) {
      w = *reinterpret_cast<const uint32_t*>(b);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (p0 + e < cols) w |= (uint32_t)b[e] << (8 * e);
    }
    static_cast<uint32_t*>(ring)[d * row4 + c] = w;
    return;
  }
  const float* __restrict__ f = static_cast<const float*>(s.p) + r * s.ld + p0;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (whole) {
    const float4 t = *reinterpret_cast<const float4*>(f);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (p0 + e < cols) v[e] = f[e];
  }
  if (RING_U8)
    static_cast<uint32_t*>(ring)[d * row4 + c] = quant_u8(v[0]) | (quant_u8(v[1]) << 8) | (quant_u8(v[2]) << 16) | (quant_u8(v[3]) << 24);
  else
    static_cast<float4*>(ring)[d * row4 + c] = make_float4(v[0], v[1], v[2], v[3]);
}

// The five small fields of a vector step and its marks in one launch.  Threads 0 .. n * tot4 - 1: one float4 of a ring row each, the
// fields' rows side by side (tot4 = sum of ring_ld[f] / 4; the loop over the fields is unrolled, so the by-value struct is never indexed
// with a register).  With flags, threads n * tot4 + j: j < n marks written slot j, n <= j < 2n takes HEAD from slot j - n of the step
// before -- other slots than the written ones, since n divides nrows and n < nrows there.  Sources are read element by element: a
// (n, 2) tensor has 8-byte rows.
__global__ void __launch_bounds__(256) ring_store_small_kernel(dgvit_small_fields p, int tot4, unsigned char* __restrict__ flags,
                                                               const void* __restrict__ episode_end, int end_f32, long long n,
                                                               long long nrows, long long start) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long cells = n * tot4;
  if (i < cells) {
    const long long r = i / tot4;
    int j = (int)(i - r * tot4);
    long long d = start + r;
    if (d >= nrows) d -= nrows;
#pragma unroll
    for (int f = 0; f < DGVIT_SMALL_FIELDS; ++f) {
      const int w4 = p.ring_ld[f] >> 2;
      if (j >= 0 && j < w4) {
        const float* __restrict__ s = p.src[f] + r * p.src_ld[f] + 4 * j;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (4 * j + e < p.cols[f]) v[e] = s[e];
        reinterpret_cast<float4*>(p.ring[f])[d * w4 + j] = make_float4(v[0], v[1], v[2], v[3]);
      }
      j -= w4;
    }
    return;
  }
  if (!flags) return;
  const long long j = i - cells;
  if (j < n) {
    long long d = start + j;
    if (d >= nrows) d -= nrows;
    bool end = false;
    if (episode_end)
      end = end_f32 ? static_cast<const float*>(episode_end)[j] != 0.f : static_cast<const unsigned char*>(episode_end)[j] != 0;
    flags[d] = RING_HEAD | (end ? RING_END : 0);
  } else if (j < 2 * n && n < nrows) {
    long long d = start - 2 * n + j;    // start - n + (j - n) > -nrows
    if (d < 0) d += nrows;
    flags[d] &= RING_END;
  }
}

// ---- the ring that stores each frame once: one frame arena of nrows + E + P rows -- the obs ring, one pending row per lane
// (the next_obs of the lane's newest transition) and a FIFO pool of P rows for the next_obs of transitions that ended an episode.
// next_row[s] is the arena row that holds slot s's next_obs (-1: never written); state = {head, tail, lost}, counters that only grow.

// The bookkeeping of a store of n slots at `start`, ONE wave.  Per round of 64 rows lane k takes row 64 r + k: it loads what its row depends on -- next_row of the slot it overwrites, and next_row, done and flags of its lane predecessor p =
// (s - E) mod nrows -- then every lane runs the same 64 steps of integer arithmetic on the ballots (the FIFO: a freed entry advances
// head, a terminal predecessor takes entry tail % P or, pool full, is lost), keeps the outcome of its own row, and writes it.  Nothing a
// row loads is written by another row of the same launch: next_row[s] is written by row j itself and by row j + E (whose predecessor it
// is), next_row[p] of a row j < E lies outside the store -- unless the store covers the whole ring: such a predecessor is one of the
// call's own last rows, already overwritten, and does not count; done and flags are the ring's, final since dgvit_ring_store_small.
// Row j leaves next_row[s] to row j + E where there is one.
__global__ void __launch_bounds__(64) ring_plan_next_kernel(int* __restrict__ next_row, long long* __restrict__ state, int* __restrict__ moves,
                                                            const float* __restrict__ done, long long done_ld,
                                                            const unsigned char* __restrict__ flags, long long n, long long nrows,
                                                            long long start, long long E, long long P) {
  const int lane = threadIdx.x;
  long long head = state[0], tail = state[1], lost = state[2];
  long long slot_of_tail = tail % P;   // the pool entry the next allocation takes
  const long long pool = nrows + E;
  for (long long base = 0; base < n; base += 64) {   // wave-uniform
    const long long j = base + lane;
    const bool live = j < n;
    long long s = 0, p = 0;
    bool frees = false, has_pred = false, terminal = false;
    if (live) {
      s = start + j;
      if (s >= nrows) s -= nrows;
      p = s - E;
      if (p < 0) p += nrows;
      frees = next_row[s] >= pool;
      has_pred = nrows > E && (j >= E || (n < nrows && next_row[p] >= 0));
      terminal = has_pred && (done[p * done_ld] != 0.f || (flags[p] & RING_END) != 0);
    }
    const unsigned long long fmask = __ballot(frees), tmask = __ballot(terminal);
    long long mine = -1;               // the pool entry of this lane's predecessor; -2: lost
    const int rows = (int)(n - base < 64 ? n - base : 64);
    for (int k = 0; k < rows; ++k) {   // the same arithmetic in every lane
      if ((fmask >> k) & 1) ++head;
      if ((tmask >> k) & 1) {
        long long got = -2;
        if (tail - head < P) {
          got = slot_of_tail;
          ++tail;
          if (++slot_of_tail == P) slot_of_tail = 0;
        } else {
          ++lost;
        }
        if (k == lane) mine = got;
      }
    }
    if (live) {
      if (j + E >= n) next_row[s] = (int)(nrows + s % E);   // the lane's pending row
      moves[j] = mine >= 0 ? (int)(pool + mine) : -1;
      if (has_pred) next_row[p] = terminal ? (mine >= 0 ? (int)(pool + mine) : (int)p) : (int)s;
    }
  }
  if (lane == 0) {
    state[0] = head;
    state[1] = tail;
    state[2] = lost;
  }
}

// one group of 4 pixels, row r of a source into group `at` of the arena: the three conversions of ring_store_frames_kernel, which keeps
// its own copy -- the two-matrix ring's kernels are not touched by the shared ring
template <bool RING_U8>
__device__ __forceinline__ void store_group(const frame_src& s, long long r, int c, int cols, void* __restrict__ arena, long long at) {
  const int p0 = 4 * c;
  const bool whole = s.vec && p0 + 4 <= cols;
  if (RING_U8 && s.u8) {        // codes as they are
    const unsigned char* __restrict__ b = static_cast<const unsigned char*>(s.p) + r * s.ld + p0;
    uint32_t w = 0;
    if (whole) {
      w = *reinterpret_cast<const uint32_t*>(b);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (p0 + e < cols) w |= (uint32_t)b[e] << (8 * e);
    }
    static_cast<uint32_t*>(arena)[at] = w;
    return;
  }
  const float* __restrict__ f = static_cast<const float*>(s.p) + r * s.ld + p0;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (whole) {
    const float4 t = *reinterpret_cast<const float4*>(f);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (p0 + e < cols) v[e] = f[e];
  }
  if (RING_U8)
    static_cast<uint32_t*>(arena)[at] = quant_u8(v[0]) | (quant_u8(v[1]) << 8) | (quant_u8(v[2]) << 16) | (quant_u8(v[3]) << 24);
  else
    static_cast<float4*>(arena)[at] = make_float4(v[0], v[1], v[2], v[3]);
}

// The frames of a store into the arena, after its bookkeeping.  blockIdx.y == 0: the obs rows into the ring, as ring_store_frames.
// blockIdx.y == 1, thread = group c of row r: the move of row r (the next_obs of r's terminal predecessor into its pool row -- out of the
// lane's pending row for r < E, out of the call's own next_obs row r - E otherwise) and then, for r < E, the next_obs of the lane's LAST
// row of the call into the pending row.  The read of a pending group and the write over it are this one thread's, in this order; pool rows
// are written by moves alone and no two moves of a launch share one (ring_plan_next_kernel); sources are never written.
template <bool RING_U8>
__global__ void __launch_bounds__(256) ring_store_frames_shared_kernel(frame_src s0, frame_src s1, void* __restrict__ arena,
                                                                       const int* __restrict__ moves, long long total4, int row4, int cols,
                                                                       long long nrows, long long start, long long n, long long E,
                                                                       long long arena_rows) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const long long r = i / row4;
  const int c = (int)(i - r * row4);
  if (blockIdx.y == 0) {
    long long d = start + r;    // start < nrows and r < n <= nrows: one subtraction wraps the ring
    if (d >= nrows) d -= nrows;
    store_group<RING_U8>(s0, r, c, cols, arena, d * row4 + c);
    return;
  }
  const long long m = moves[r];
  const bool move = m >= nrows + E && m < arena_rows;   // a pool row, whatever the table holds
  if (r >= E) {
    if (move) store_group<RING_U8>(s1, r - E, c, cols, arena, m * row4 + c);
    return;
  }
  const long long pending = (nrows + r) * row4 + c;     // E divides start: row r < E is lane r
  if (move) {
    if (RING_U8) static_cast<uint32_t*>(arena)[m * row4 + c] = static_cast<const uint32_t*>(arena)[pending];
    else static_cast<float4*>(arena)[m * row4 + c] = static_cast<const float4*>(arena)[pending];
  }
  store_group<RING_U8>(s1, r + (n - 1 - r) / E * E, c, cols, arena, pending);
}

// out[i] = next_row[idx[i]], the arena row of the slot's next_obs; a slot never written gives itself, a row of zeros
__global__ void __launch_bounds__(256) ring_next_rows_kernel(const int* __restrict__ next_row, const long long* __restrict__ idx,
                                                             long long* __restrict__ out, long long nsel, long long nrows) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nsel) return;
  const long long s = ring_row(idx[i], nrows);
  const long long r = next_row[s];
  out[i] = r < 0 ? s : r;
}

// ---- the ring as a file: ages [a0, a0 + n) packed field-major into one device buffer, the chunk that leaves in one
// device -> host copy.  Block b of the buffer starts at off[b], a multiple of 16 bytes: obs, next_obs, the five small fields, the n END
// bytes and, with a tree, the n leaves.
struct export_args {
  const unsigned char* obs;       // the obs matrix; the arena of a shared ring
  const unsigned char* next_obs;  // the next_obs matrix; the arena again
  const int* next_row;            // null: a two-matrix ring
  const float* small[DGVIT_SMALL_FIELDS];
  const unsigned char* flags;     // null: episodes were never tracked
  const float* leaves;            // null: no tree
  long long off[DGVIT_SMALL_FIELDS + 4];
  long long ring_bytes;           // bytes between two frame rows of the ring
  long long dense_bytes;          // bytes of a frame row in the buffer: cols * itemsize
  long long next_rows;            // rows of next_obs
  int small_cols[DGVIT_SMALL_FIELDS];
  int small_ld[DGVIT_SMALL_FIELDS];
};

// blockIdx.y is the block of the buffer, so everything that depends on it is wave-uniform.  y < 2, thread = one V (16, 4 or 1 bytes) of a
// dense frame row: ring rows are 16-byte aligned and dense rows a multiple of sizeof(V) behind a 16-byte aligned block, so both sides of
// the copy are aligned; the bytes are the ring's, no conversion.  next_obs of a shared ring is read at next_row[slot], at the slot's own
// obs row where the table names no arena row.  y >= 2, thread = one float of a small field, one END byte or one leaf.  Slot of row r is
// first + r, first < nrows and r < n <= nrows: one subtraction wraps the ring.  Every offset is 64-bit.
template <typename V>
__global__ void __launch_bounds__(256) ring_export_kernel(const export_args p, unsigned char* __restrict__ out, long long n, int units,
                                                          long long nrows, long long first) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int y = (int)blockIdx.y;
  if (y < 2) {
    if (i >= n * units) return;
    const long long r = i / units;
    const long long c = i - r * units;
    long long s = first + r;
    if (s >= nrows) s -= nrows;
    const unsigned char* __restrict__ src = p.obs + s * p.ring_bytes;
    if (y == 1) {
      long long q = s;
      if (p.next_row) {
        const long long t = p.next_row[s];
        if (t >= 0 && t < p.next_rows) q = t;
      }
      src = p.next_obs + q * p.ring_bytes;
    }
    unsigned char* __restrict__ dst = out + (y == 0 ? p.off[0] : p.off[1]) + r * p.dense_bytes;
    reinterpret_cast<V*>(dst)[c] = reinterpret_cast<const V*>(src)[c];
    return;
  }
#pragma unroll
  for (int f = 0; f < DGVIT_SMALL_FIELDS; ++f) {   // unrolled: the by-value struct is never indexed with a register
    if (y == 2 + f) {
      const int cols = p.small_cols[f];
      if (i >= n * cols) return;
      const long long r = i / cols;
      const long long c = i - r * cols;
      long long s = first + r;
      if (s >= nrows) s -= nrows;
      reinterpret_cast<float*>(out + p.off[2 + f])[i] = p.small[f][s * p.small_ld[f] + c];
      return;
    }
  }
  if (i >= n) return;
  long long s = first + i;
  if (s >= nrows) s -= nrows;
  if (y == 2 + DGVIT_SMALL_FIELDS) out[p.off[2 + DGVIT_SMALL_FIELDS] + i] = p.flags ? (unsigned char)(p.flags[s] & RING_END) : (unsigned char)0;
  else reinterpret_cast<float*>(out + p.off[3 + DGVIT_SMALL_FIELDS])[i] = p.leaves[s];
}

// ---- frame stacks at sample time: the K newest frames of a slot's episode, channel-last, built from the single frames the
// ring holds.  The n-step walk goes forward along an episode; this is the same walk backward.
constexpr int STACK_MAX = 16;   // one lane per predecessor; a 128 x 160 stack of 16 is 1.3 MB a sample

// Lane k < K of the wave learns p = pred_k = (s - k E) mod nrows, its flags and its done in one round trip; pred_k (k >= 1) is linked iff
// k E < nrows, it lies at or behind slot 0 only in a full ring, and neither a flag nor done stops a walk behind it.  Returns d, the number
// of consecutive linked predecessors from k = 1 (wave-uniform, 0 <= d <= K - 1).  Lanes that are not linked keep p = s, which nothing
// selects: every p is a slot of the ring.
__device__ __forceinline__ int stack_walk_from(long long s, int lane, int K, long long nrows, long long E, bool full,
                                               const float* __restrict__ done, long long done_ld, const unsigned char* __restrict__ flags,
                                               long long& p) {
  p = s;
  bool linked = false;
  if (lane >= 1 && lane < K) {
    const long long back = lane * E;   // E <= nrows < 2^56 (launcher): no overflow
    if (back < nrows) {
      const long long q = s - back;    // > -nrows: one addition wraps the ring
      if (q >= 0 || full) {
        p = q < 0 ? q + nrows : q;
        linked = flags[p] == 0 && done[p * done_ld] == 0.f;
      }
    }
  }
  const unsigned long long stop = __ballot(lane >= 1 && !linked);   // lanes K .. 63 always stop: never empty, and bit 0 is never set
  return __ffsll((long long)stop) - 2;
}

// One wave per sample (4 per workgroup), as nstep_walk_kernel.  obs_rows[b][c] = pred_min(K-1-c, d) of s = clamp(idx[b]); next_rows[b][c]
// = pred^t_min(K-2-c, d_t) for c < K - 1, rows of the obs matrix, and next_rows[b][K-1] the row of t's next_obs in ITS matrix: t itself,
// or next_row[t] of a shared ring (t where the table names no arena row, as ring_next_rows_kernel).  t = tail[b] with a second walk, or
// t = s and d_t = d without `tail`.  No atomics: a function of the ring and idx[b].
__global__ void __launch_bounds__(256) ring_stack_rows_kernel(const long long* __restrict__ idx, const long long* __restrict__ tail,
                                                              const unsigned char* __restrict__ flags, const float* __restrict__ done,
                                                              long long done_ld, const int* __restrict__ next_row,
                                                              long long* __restrict__ obs_rows, long long* __restrict__ next_rows,
                                                              long long nsel, long long nrows, long long E, int K, int full,
                                                              long long arena_rows) {
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= nsel) return;       // wave-uniform
  const long long s = ring_row(idx[w], nrows);
  long long p;
  const int d = stack_walk_from(s, lane, K, nrows, E, full != 0, done, done_ld, flags, p);
  const long long orow = __shfl(p, min(max(K - 1 - lane, 0), d), 64);
  long long t = s, pt = p;
  int dt = d;
  if (tail) {                  // wave-uniform: the n-step sample's next_obs stack ends at the walk's tail
    t = ring_row(tail[w], nrows);
    dt = stack_walk_from(t, lane, K, nrows, E, full != 0, done, done_ld, flags, pt);
  }
  long long nrow = __shfl(pt, min(max(K - 2 - lane, 0), dt), 64);
  if (lane == K - 1) {
    nrow = t;
    if (next_row) {
      const long long r = next_row[t];
      if (r >= 0 && r < arena_rows) nrow = r;
    }
  }
  if (lane < K) {
    obs_rows[w * K + lane] = orow;
    next_rows[w * K + lane] = nrow;
  }
}

// out[r][p][c] = fp32(src_c[rows[r][c]][p]), src_c = src1 for c == K - 1 and src0 before: the (H W, K) channel-last stack of sample r.
// blockIdx.x is the sample, so its K rows are wave-uniform (scalar loads); thread = one group of 4 pixels: ONE float4 (fp32 ring) or ONE
// dword (byte ring) of each of the K source frames, then the group's 4 K contiguous output floats as K float4s -- K is a template
// argument so that the transposition is register renaming.  The 256 groups of a workgroup are 1024 K contiguous output floats, so the
// float4s go through LDS (4 K KiB) and leave in output order: store j of the workgroup is 256 consecutive float4s, 4 KiB, where a
// thread storing its own K float4s would stride 16 K bytes (both forms were measured: DESIGN 3.43).  Pixels at or beyond
// `cols` are zeros, whatever the ring holds there, and so is every float4 of a group at or beyond `groups` (a row_floats longer than
// al4(cols K): that LDS was never written and is not read); float4s at or beyond out4 = row_floats / 4 belong to the next sample and
// are not written.  The grid covers out4, not groups: a group whose float4s all lie beyond out4 has nothing to store.  Every row is
// clamped to its matrix.
template <typename T, int K>
__global__ void __launch_bounds__(256) gather_stack_frames_kernel(const T* __restrict__ src0, const T* __restrict__ src1,
                                                                  const long long* __restrict__ rows, float* __restrict__ out, int groups,
                                                                  int cols, long long ld, int out4, long long nrows0, long long nrows1) {
  __shared__ float4 stage[256 * K];
  const int g = (int)blockIdx.y * 256 + (int)threadIdx.x;
  const long long r = blockIdx.x;
  if (g < groups) {
    const int p0 = 4 * g;
    float v[K][4];
#pragma unroll
    for (int c = 0; c < K; ++c) {
      const long long s = ring_row(rows[r * K + c], c == K - 1 ? nrows1 : nrows0);
      const T* __restrict__ frame = (c == K - 1 ? src1 : src0) + s * ld + p0;
      if constexpr (std::is_same_v<T, float>) {
        const float4 t = *reinterpret_cast<const float4*>(frame);
        v[c][0] = t.x, v[c][1] = t.y, v[c][2] = t.z, v[c][3] = t.w;
      } else {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(frame);
        v[c][0] = dequant_u8(w & 255u), v[c][1] = dequant_u8((w >> 8) & 255u), v[c][2] = dequant_u8((w >> 16) & 255u),
        v[c][3] = dequant_u8(w >> 24);
      }
#pragma unroll
      for (int e = 1; e < 4; ++e)   // p0 < cols: element 0 is always a pixel
        if (p0 + e >= cols) v[c][e] = 0.f;
    }
    float4* __restrict__ mine = stage + (int)threadIdx.x * K;
#pragma unroll
    for (int j = 0; j < K; ++j)     // element q = 4 j + t of the group is pixel q / K, channel q % K
      mine[j] = make_float4(v[(4 * j) % K][(4 * j) / K], v[(4 * j + 1) % K][(4 * j + 1) / K], v[(4 * j + 2) % K][(4 * j + 2) / K],
                            v[(4 * j + 3) % K][(4 * j + 3) / K]);
  }
  __syncthreads();                  // every thread of the workgroup arrives: nobody has returned
  const int base = (int)blockIdx.y * 256 * K;   // < out4 + 4096 <= 2^25 + 2^12
  float4* __restrict__ o = reinterpret_cast<float4*>(out) + r * out4 + base;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const int i = j * 256 + (int)threadIdx.x;   // float4 i of the workgroup was formed by its thread i / K
    if (base + i < out4) o[i] = (int)blockIdx.y * 256 + i / K < groups ? stage[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// The stacked gather with the random shift: gather_shift_frames_kernel's launch shape, draw (shift_draw: the same r, tag and seed, so the
// shift table is the unstacked call's) and clamps, ONE (dy, dx) per sample for all K channels.  Thread = one float4 of the output row;
// its 4 elements advance channel first, then x, then y, and each reads its own frame's row from the table (K <= 16 rows, cached).
template <typename T>
__global__ void __launch_bounds__(256) gather_shift_stack_kernel(const T* __restrict__ src0, const T* __restrict__ src1,
                                                                 const long long* __restrict__ rows, float* __restrict__ out,
                                                                 int* __restrict__ shifts_out, int out4, long long ld, long long nrows0,
                                                                 long long nrows1, int H, int W, int K, int pad, uint32_t tag,
                                                                 unsigned long long seed, const unsigned long long* __restrict__ seed_dev) {
  const int c4 = (int)blockIdx.y * 256 + (int)threadIdx.x;
  if (c4 >= out4) return;
  const long long r = blockIdx.x;
  int dy, dx;
  shift_draw(r, pad, tag, seed, seed_dev, dy, dx);
  if (shifts_out && c4 == 0) {
    shifts_out[2 * r] = dy;
    shifts_out[2 * r + 1] = dx;
  }
  const unsigned q0 = 4u * (unsigned)c4, px = q0 / (unsigned)K;   // H * W * K <= 2^27 (launcher)
  int ch = (int)(q0 - px * (unsigned)K), y = (int)(px / (unsigned)W), x = (int)(px - (unsigned)y * (unsigned)W);
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int sy = min(max(y + dy, 0), H - 1), sx = min(max(x + dx, 0), W - 1);
    const bool last = ch == K - 1;
    const long long s = ring_row(rows[r * K + ch], last ? nrows1 : nrows0);
    const T* __restrict__ frame = (last ? src1 : src0) + s * ld;
    // the source pixel is always inside its frame (clamped), so it is loaded unconditionally; y >= H are the padding columns
    if constexpr (std::is_same_v<T, float>) {
      const float t = frame[(long long)sy * W + sx];
      v[e] = y < H ? t : 0.f;
    } else {
      const uint32_t t = frame[sy * W + sx];
      v[e] = y < H ? dequant_u8(t) : 0.f;
    }
    if (++ch == K) {
      ch = 0;
      if (++x == W) { x = 0; ++y; }
    }
  }
  reinterpret_cast<float4*>(out)[r * out4 + c4] = make_float4(v[0], v[1], v[2], v[3]);
}

// The acting side (replay.FrameStack): stack is (E, cols, K) fp32, channel K - 1 the newest.  Thread = one pixel of one environment: it
// alone reads and writes that pixel's K channels, in ascending order, so the update in place is safe.  An environment with reset[e] != 0
// (or every one, reset_all) has all K channels filled with the new frame, Gym's FrameStack at reset.
__global__ void __launch_bounds__(256) frame_stack_push_kernel(float* __restrict__ stack, const float* __restrict__ frame, long long frame_ld,
                                                               const unsigned char* __restrict__ reset, int reset_all, long long total,
                                                               int cols, int K) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long e = i / cols;
  const int p = (int)(i - e * cols);
  const float v = frame[e * frame_ld + p];
  const bool fill = reset_all || (reset && reset[e] != 0);
  float* px = stack + i * K;      // not __restrict__-qualified reads: channel c + 1 is read before channel c is written
  for (int c = 0; c + 1 < K; ++c) px[c] = fill ? v : px[c + 1];
  px[K - 1] = v;
}

// both shifted gathers: `name` is the entry point's, `ld` the source's row stride in elements (an fp32 ring's is row_floats)
template <typename T>
int launch_gather_shift(const char* name, const T* src, const long long* idx, float* out, int* shifts_out, long long nsel, int H, int W,
                        long long ld, long long row_floats, long long nrows, int pad, int stream_id, unsigned long long seed,
                        const unsigned long long* seed_dev, hipStream_t stream) {
  constexpr bool BYTES = !std::is_same_v<T, float>;
  const char* what = BYTES ? "ring" : "src";
  DGVIT_CHECK_ARG(src && out, "%s: %s and out must not be null", name, what);
  DGVIT_CHECK_ARG(nsel > 0 && nsel < (1ll << 24) && nrows > 0, "%s: nsel=%lld must be in [1, 2^24) and nrows=%lld positive", name, nsel,
                  nrows);   // one workgroup column per sample: 256 * nsel threads along x
  DGVIT_CHECK_ARG(H > 0 && W > 0, "%s: frame H=%d W=%d must be positive", name, H, W);
  const long long cols = (long long)H * W;
  if constexpr (BYTES)
    DGVIT_CHECK_ARG(ld % 16 == 0 && ld >= cols, "%s: row_bytes=%lld must be a multiple of 16 and at least H*W=%lld", name, ld, cols);
  DGVIT_CHECK_ARG(row_floats % 4 == 0 && row_floats >= cols && row_floats <= (1ll << 25),
                  "%s: row_floats=%lld must be a multiple of 4, at least H*W=%lld and at most 2^25", name, row_floats, cols);
  DGVIT_CHECK_ARG(pad >= 0 && pad < H && pad < W, "%s: pad=%d must be in [0, min(H, W)) = [0, %d)", name, pad, H < W ? H : W);
  DGVIT_CHECK_ARG(stream_id >= 0 && stream_id < DGVIT_SHIFT_STREAMS, "%s: stream_id=%d must be in [0, %d)", name, stream_id, DGVIT_SHIFT_STREAMS);
  DGVIT_CHECK_ARG(al16(src) && al16(out), "%s: %s and out must be 16-byte aligned", name, what);
  const int row4 = (int)(row_floats / 4);
  src_stride<T> stride{};
  if constexpr (BYTES) stride = ld;
  hipLaunchKernelGGL(gather_shift_frames_kernel<T>, dim3((unsigned)nsel, (unsigned)((row4 + 255) / 256)), dim3(256), 0, stream, src, idx, out,
                     shifts_out, row4, stride, nrows, H, W, pad, shift_tag(stream_id), seed, seed_dev);
  DGVIT_CHECK_LAUNCH(name);
  return DGVIT_OK;
}

inline bool al4p(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3) == 0; }
inline bool al8p(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7) == 0; }

// the slots of a store, n from `start` on: what ring_mark and the three store entry points ask of them
int check_slots(const char* name, long long n, long long nrows, long long start) {
  DGVIT_CHECK_ARG(n > 0 && nrows > 0 && n <= nrows, "%s: n=%lld must be in [1, nrows] and nrows=%lld positive", name, n, nrows);
  DGVIT_CHECK_ARG(start >= 0 && start < nrows, "%s: start=%lld must be in [0, nrows) = [0, %lld)", name, start, nrows);
  return DGVIT_OK;
}

// the lanes and the pool of a shared ring, and a store's place in them: what ring_plan_next and ring_store_frames_shared ask alike
int check_shared(const char* name, long long n, long long nrows, long long start, long long envs, long long pool) {
  if (const int rc = check_slots(name, n, nrows, start)) return rc;
  DGVIT_CHECK_ARG(envs >= 1 && envs <= nrows && nrows % envs == 0, "%s: envs=%lld must be in [1, nrows] and divide nrows=%lld", name, envs, nrows);
  DGVIT_CHECK_ARG(n % envs == 0 && start % envs == 0, "%s: n=%lld and start=%lld must be multiples of envs=%lld", name, n, start, envs);
  DGVIT_CHECK_ARG(pool >= 1 && pool <= nrows, "%s: pool=%lld must be in [1, nrows] = [1, %lld]", name, pool, nrows);
  DGVIT_CHECK_ARG(nrows + envs + pool < (1ll << 31), "%s: the arena's nrows + envs + pool = %lld rows must be below 2^31", name,
                  nrows + envs + pool);
  return DGVIT_OK;
}

// What ring_store_frames and ring_store_frames_shared ask alike, in the one order of both: the sources, the slots (`shared`: check_shared
// with envs and pool, else check_slots) and the ring's rows.  The entry point's own pointers come in as `set` and `aligned`, and as the
// words it has for them in the two messages, `theirs` and `their_alignment`.
int check_frame_store(const char* name, bool shared, const void* src0, int src0_u8, long long src0_ld, const void* src1, int src1_u8,
                      long long src1_ld, bool set, const char* theirs, bool aligned, const char* their_alignment, int ring_u8,
                      long long ring_ld, long long n, long long cols, long long nrows, long long start, long long envs, long long pool) {
  DGVIT_CHECK_ARG(src0 && src1 && set, "%s: src0, src1, %s must not be null", name, theirs);
  DGVIT_CHECK_ARG((src0_u8 | src1_u8 | ring_u8) >> 1 == 0, "%s: src0_u8=%d, src1_u8=%d and ring_u8=%d must be 0 or 1", name, src0_u8, src1_u8,
                  ring_u8);
  DGVIT_CHECK_ARG(ring_u8 || !(src0_u8 || src1_u8), "%s: uint8 sources (src0_u8=%d, src1_u8=%d) need a uint8 ring", name, src0_u8, src1_u8);
  if (const int rc = shared ? check_shared(name, n, nrows, start, envs, pool) : check_slots(name, n, nrows, start)) return rc;
  DGVIT_CHECK_ARG(cols > 0 && cols <= (1ll << 25), "%s: cols=%lld must be in [1, 2^25]", name, cols);
  DGVIT_CHECK_ARG(ring_ld % (ring_u8 ? 16 : 4) == 0 && ring_ld >= cols && ring_ld <= (1ll << 26),
                  "%s: ring_ld=%lld must be a multiple of %d, at least cols=%lld and at most 2^26", name, ring_ld, ring_u8 ? 16 : 4, cols);
  DGVIT_CHECK_ARG(src0_ld >= cols && src1_ld >= cols, "%s: src0_ld=%lld and src1_ld=%lld must be at least cols=%lld", name, src0_ld, src1_ld,
                  cols);
  DGVIT_CHECK_ARG(aligned && (src0_u8 || al4p(src0)) && (src1_u8 || al4p(src1)), "%s: %s and fp32 sources 4-byte aligned", name,
                  their_alignment);
  DGVIT_CHECK_ARG((n * (ring_ld / 4) + 255) / 256 < (1ll << 31), "%s: n=%lld rows of ring_ld=%lld are more than one launch covers", name, n,
                  ring_ld);
  return DGVIT_OK;
}

// a frame field's rows as the two store kernels read them: whole groups of 4 pixels at once where the rows' alignment allows it
frame_src make_frame_src(const void* p, int u8, long long ld) {
  const bool vec = u8 ? (ld % 4 == 0 && al4p(p)) : (ld % 4 == 0 && al16(p));
  return frame_src{p, ld, u8, (int)vec};
}

// both walks: `name` is the entry point's, `stride` null for nstep_walk, whose kernel has no such argument
int launch_nstep_walk(const char* name, const float* rew, long long rew_ld, const float* done, long long done_ld, const unsigned char* flags,
                      const float* next_small, long long small_ld, const long long* idx, long long nsel, long long nrows,
                      const long long* stride, int n, double gamma, float* ret_out, float* done_out, float* discount_out,
                      float* next_small_out, int* steps_out, long long* tail_out, hipStream_t stream) {
  DGVIT_CHECK_ARG(rew && done && flags && next_small && idx, "%s: rew, done, flags, next_small and idx must not be null", name);
  DGVIT_CHECK_ARG(ret_out && done_out && discount_out && next_small_out && steps_out && tail_out,
                  "%s: ret_out, done_out, discount_out, next_small_out, steps_out and tail_out must not be null", name);
  DGVIT_CHECK_ARG(nsel > 0 && nsel < (1ll << 31) && nrows > 0, "%s: nsel=%lld must be in [1, 2^31) and nrows=%lld positive", name, nsel, nrows);
  if (stride) {
    DGVIT_CHECK_ARG(nrows < (1ll << 56), "%s: nrows=%lld must be below 2^56", name, nrows);   // lane * stride cannot overflow
    DGVIT_CHECK_ARG(*stride >= 1 && *stride <= nrows, "%s: stride=%lld must be in [1, nrows] = [1, %lld]", name, *stride, nrows);
  }
  DGVIT_CHECK_ARG(n >= 1 && n <= NSTEP_MAX, "%s: n=%d must be in [1, %d]", name, n, NSTEP_MAX);
  DGVIT_CHECK_ARG(gamma >= 0.0 && gamma <= 1.0, "%s: gamma=%g must be in [0, 1]", name, gamma);   // a NaN fails both comparisons
  DGVIT_CHECK_ARG(rew_ld > 0 && done_ld > 0, "%s: rew_ld=%lld and done_ld=%lld must be positive", name, rew_ld, done_ld);
  DGVIT_CHECK_ARG(small_ld > 0 && small_ld % 4 == 0 && small_ld <= (1ll << 20), "%s: small_ld=%lld must be a positive multiple of 4, at most 2^20",
                  name, small_ld);
  DGVIT_CHECK_ARG(al16(next_small) && al16(next_small_out), "%s: next_small and next_small_out must be 16-byte aligned", name);
  DGVIT_CHECK_ARG(al4p(rew) && al4p(done) && al4p(ret_out) && al4p(done_out) && al4p(discount_out) && al4p(steps_out) && al8p(idx) &&
                      al8p(tail_out),
                  "%s: float and int32 pointers must be 4-byte aligned, idx and tail_out 8-byte aligned", name);
  const dim3 grid((unsigned)((nsel + 3) / 4));
  const float4* small = reinterpret_cast<const float4*>(next_small);
  float4* small_out = reinterpret_cast<float4*>(next_small_out);
  if (stride)
    hipLaunchKernelGGL(nstep_walk_strided_kernel, grid, dim3(256), 0, stream, rew, rew_ld, done, done_ld, flags, small, (int)(small_ld / 4), idx,
                       nsel, nrows, *stride, n, gamma, ret_out, done_out, discount_out, small_out, steps_out, tail_out);
  else
    hipLaunchKernelGGL(nstep_walk_kernel, grid, dim3(256), 0, stream, rew, rew_ld, done, done_ld, flags, small, (int)(small_ld / 4), idx, nsel,
                       nrows, n, gamma, ret_out, done_out, discount_out, small_out, steps_out, tail_out);
  DGVIT_CHECK_LAUNCH(name);
  return DGVIT_OK;
}

}  // namespace

int gather_rows(const float* src, const long long* idx, float* out, long long nsel, long long row_floats, long long nrows,
                hipStream_t stream) {
  DGVIT_CHECK_ARG(src && idx && out && nsel > 0 && nrows > 0, "gather_rows: bad arguments");
  DGVIT_CHECK_ARG(row_floats > 0 && row_floats % 4 == 0 && row_floats / 4 < (1ll << 31), "gather_rows: row length must be a multiple of 4 floats");
  const long long total4 = nsel * (row_floats / 4);
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, stream, src, idx, out, total4,
                     (int)(row_floats / 4), nrows);
  DGVIT_CHECK_LAUNCH("gather_rows");
  return DGVIT_OK;
}

int gather_shift_frames(const float* src, const long long* idx, float* out, int* shifts_out, long long nsel, int H, int W,
                        long long row_floats, long long nrows, int pad, int stream_id, unsigned long long seed,
                        const unsigned long long* seed_dev, hipStream_t stream) {
  return launch_gather_shift("gather_shift_frames", src, idx, out, shifts_out, nsel, H, W, row_floats, row_floats, nrows, pad, stream_id, seed,
                             seed_dev, stream);
}

int gather_shift_frames_u8(const unsigned char* ring, const long long* idx, float* out, int* shifts_out, long long nsel, int H, int W,
                           long long row_bytes, long long row_floats, long long nrows, int pad, int stream_id, unsigned long long seed,
                           const unsigned long long* seed_dev, hipStream_t stream) {
  return launch_gather_shift("gather_shift_frames_u8", ring, idx, out, shifts_out, nsel, H, W, row_bytes, row_floats, nrows, pad, stream_id,
                             seed, seed_dev, stream);
}

int quantize_rows_u8(const float* src, long long src_ld, unsigned char* ring, long long n, long long cols, long long row_bytes,
                     long long nrows, long long start, hipStream_t stream) {
  DGVIT_CHECK_ARG(src && ring, "quantize_rows_u8: src and ring must not be null");
  if (const int rc = check_slots("quantize_rows_u8", n, nrows, start)) return rc;
  DGVIT_CHECK_ARG(cols > 0 && cols <= (1ll << 25), "quantize_rows_u8: cols=%lld must be in [1, 2^25]", cols);
  DGVIT_CHECK_ARG(row_bytes % 16 == 0 && row_bytes >= cols && row_bytes <= (1ll << 26),
                  "quantize_rows_u8: row_bytes=%lld must be a multiple of 16, at least cols=%lld and at most 2^26", row_bytes, cols);
  DGVIT_CHECK_ARG(src_ld >= cols, "quantize_rows_u8: src_ld=%lld must be at least cols=%lld", src_ld, cols);
  DGVIT_CHECK_ARG(al4p(src) && al16(ring), "quantize_rows_u8: src must be 4-byte and ring 16-byte aligned");
  const int row4 = (int)(row_bytes / 4);
  const long long total4 = n * row4, blocks = (total4 + 255) / 256;
  DGVIT_CHECK_ARG(blocks < (1ll << 31), "quantize_rows_u8: n=%lld rows of row_bytes=%lld are more than one launch covers", n, row_bytes);
  uint32_t* ring4 = reinterpret_cast<uint32_t*>(ring);
  if (src_ld % 4 == 0 && al16(src))
    hipLaunchKernelGGL(quantize_rows_u8_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, src, src_ld, ring4, total4, row4, (int)cols,
                       nrows, start);
  else
    hipLaunchKernelGGL(quantize_rows_u8_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, src, src_ld, ring4, total4, row4, (int)cols,
                       nrows, start);
  DGVIT_CHECK_LAUNCH("quantize_rows_u8");
  return DGVIT_OK;
}

int gather_rows_u8(const unsigned char* ring, const long long* idx, float* out, long long nsel, long long cols, long long row_bytes,
                   long long row_floats, long long nrows, hipStream_t stream) {
  DGVIT_CHECK_ARG(ring && idx && out, "gather_rows_u8: ring, idx and out must not be null");
  DGVIT_CHECK_ARG(nsel > 0 && nrows > 0, "gather_rows_u8: nsel=%lld and nrows=%lld must be positive", nsel, nrows);
  DGVIT_CHECK_ARG(cols > 0 && cols <= (1ll << 25), "gather_rows_u8: cols=%lld must be in [1, 2^25]", cols);
  DGVIT_CHECK_ARG(row_bytes % 16 == 0 && row_bytes >= cols, "gather_rows_u8: row_bytes=%lld must be a multiple of 16 and at least cols=%lld",
                  row_bytes, cols);
  DGVIT_CHECK_ARG(row_floats % 4 == 0 && row_floats >= cols && row_floats <= (1ll << 26),
                  "gather_rows_u8: row_floats=%lld must be a multiple of 4, at least cols=%lld and at most 2^26", row_floats, cols);
  DGVIT_CHECK_ARG(al16(ring) && al16(out), "gather_rows_u8: ring and out must be 16-byte aligned");
  const int out4 = (int)(row_floats / 4);
  const long long total4 = nsel * out4, blocks = (total4 + 255) / 256;
  DGVIT_CHECK_ARG(blocks < (1ll << 31), "gather_rows_u8: nsel=%lld rows of row_floats=%lld are more than one launch covers", nsel, row_floats);
  hipLaunchKernelGGL(gather_rows_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, ring, idx, out, total4, out4, (int)cols, row_bytes,
                     nrows);
  DGVIT_CHECK_LAUNCH("gather_rows_u8");
  return DGVIT_OK;
}

int ring_mark(unsigned char* flags, long long nrows, long long start, long long n, hipStream_t stream) {
  DGVIT_CHECK_ARG(flags, "ring_mark: flags must not be null");
  if (const int rc = check_slots("ring_mark", n, nrows, start)) return rc;
  const long long blocks = (n + 1 + 255) / 256;
  DGVIT_CHECK_ARG(blocks < (1ll << 31), "ring_mark: n=%lld slots are more than one launch covers", n);
  hipLaunchKernelGGL(ring_mark_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, flags, nrows, start, n);
  DGVIT_CHECK_LAUNCH("ring_mark");
  return DGVIT_OK;
}

int nstep_walk(const float* rew, long long rew_ld, const float* done, long long done_ld, const unsigned char* flags, const float* next_small,
               long long small_ld, const long long* idx, long long nsel, long long nrows, int n, double gamma, float* ret_out, float* done_out,
               float* discount_out, float* next_small_out, int* steps_out, long long* tail_out, hipStream_t stream) {
  return launch_nstep_walk("nstep_walk", rew, rew_ld, done, done_ld, flags, next_small, small_ld, idx, nsel, nrows, nullptr, n, gamma, ret_out,
                           done_out, discount_out, next_small_out, steps_out, tail_out, stream);
}

int ring_store_frames(const void* src0, int src0_u8, long long src0_ld, const void* src1, int src1_u8, long long src1_ld, void* ring0,
                      void* ring1, int ring_u8, long long ring_ld, long long n, long long cols, long long nrows, long long start,
                      hipStream_t stream) {
  // the two spliced messages read "ring_store_frames: src0, src1, ring0 and ring1 must not be null" and "ring_store_frames: the rings must
  // be 16-byte and fp32 sources 4-byte aligned" (tests/test_vec_replay_host.py matches them)
  if (const int rc = check_frame_store("ring_store_frames", false, src0, src0_u8, src0_ld, src1, src1_u8, src1_ld, ring0 && ring1,
                                       "ring0 and ring1", al16(ring0) && al16(ring1), "the rings must be 16-byte", ring_u8, ring_ld, n, cols,
                                       nrows, start, 0, 0))
    return rc;
  const int row4 = (int)(ring_ld / 4);   // groups of 4 pixels per ring row, a dword of bytes or a float4
  const long long total4 = n * row4, blocks = (total4 + 255) / 256;
  const frame_src s0 = make_frame_src(src0, src0_u8, src0_ld), s1 = make_frame_src(src1, src1_u8, src1_ld);
  if (ring_u8)
    hipLaunchKernelGGL(ring_store_frames_kernel<true>, dim3((unsigned)blocks, 2), dim3(256), 0, stream, s0, s1, ring0, ring1, total4, row4,
                       (int)cols, nrows, start);
  else
    hipLaunchKernelGGL(ring_store_frames_kernel<false>, dim3((unsigned)blocks, 2), dim3(256), 0, stream, s0, s1, ring0, ring1, total4, row4,
                       (int)cols, nrows, start);
  DGVIT_CHECK_LAUNCH("ring_store_frames");
  return DGVIT_OK;
}

int ring_store_small(const dgvit_small_fields& fields, unsigned char* flags, const void* episode_end, int end_f32, long long n,
                     long long nrows, long long start, hipStream_t stream) {
  if (const int rc = check_slots("ring_store_small", n, nrows, start)) return rc;
  // only the marks touch the previous step's slots, which are other slots than the written ones when n divides nrows
  DGVIT_CHECK_ARG(!flags || nrows % n == 0, "ring_store_small: n=%lld must divide nrows=%lld when flags are given", n, nrows);
  DGVIT_CHECK_ARG(end_f32 == 0 || end_f32 == 1, "ring_store_small: end_f32=%d must be 0 or 1", end_f32);
  DGVIT_CHECK_ARG(!episode_end || flags, "ring_store_small: episode_end without flags: the flags must not be null when ends are given");
  DGVIT_CHECK_ARG(!episode_end || !end_f32 || al4p(episode_end), "ring_store_small: an fp32 episode_end must be 4-byte aligned");
  long long tot4 = 0;
  for (int f = 0; f < DGVIT_SMALL_FIELDS; ++f) {
    DGVIT_CHECK_ARG(fields.src[f] && fields.ring[f], "ring_store_small: src[%d] and ring[%d] must not be null", f, f);
    DGVIT_CHECK_ARG(fields.cols[f] >= 1 && fields.ring_ld[f] % 4 == 0 && fields.ring_ld[f] >= fields.cols[f] && fields.ring_ld[f] <= (1 << 20),
                    "ring_store_small: cols[%d]=%d must be at least 1 and ring_ld[%d]=%d a multiple of 4, at least cols and at most 2^20", f,
                    fields.cols[f], f, fields.ring_ld[f]);
    DGVIT_CHECK_ARG(fields.src_ld[f] >= fields.cols[f], "ring_store_small: src_ld[%d]=%lld must be at least cols[%d]=%d", f, fields.src_ld[f], f,
                    fields.cols[f]);
    DGVIT_CHECK_ARG(al4p(fields.src[f]) && al16(fields.ring[f]), "ring_store_small: src[%d] must be 4-byte and ring[%d] 16-byte aligned", f, f);
    tot4 += fields.ring_ld[f] / 4;
  }
  const long long threads = n * tot4 + (flags ? 2 * n : 0), blocks = (threads + 255) / 256;
  DGVIT_CHECK_ARG(blocks < (1ll << 31), "ring_store_small: n=%lld slots are more than one launch covers", n);
  hipLaunchKernelGGL(ring_store_small_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, fields, (int)tot4, flags, episode_end, end_f32, n,
                     nrows, start);
  DGVIT_CHECK_LAUNCH("ring_store_small");
  return DGVIT_OK;
}

int ring_plan_next(int* next_row, long long* state, int* moves, const float* done, long long done_ld, const unsigned char* flags, long long n,
                   long long nrows, long long start, long long envs, long long pool, hipStream_t stream) {
  DGVIT_CHECK_ARG(next_row && state && moves && done && flags, "ring_plan_next: next_row, state, moves, done and flags must not be null");
  if (const int rc = check_shared("ring_plan_next", n, nrows, start, envs, pool)) return rc;
  DGVIT_CHECK_ARG(done_ld > 0, "ring_plan_next: done_ld=%lld must be positive", done_ld);
  DGVIT_CHECK_ARG(al4p(next_row) && al4p(moves) && al4p(done) && al8p(state),
                  "ring_plan_next: next_row, moves and done must be 4-byte aligned, state 8-byte aligned");
  hipLaunchKernelGGL(ring_plan_next_kernel, dim3(1), dim3(64), 0, stream, next_row, state, moves, done, done_ld, flags, n, nrows, start, envs,
                     pool);
  DGVIT_CHECK_LAUNCH("ring_plan_next");
  return DGVIT_OK;
}

int ring_store_frames_shared(const void* src0, int src0_u8, long long src0_ld, const void* src1, int src1_u8, long long src1_ld, void* arena,
                             const int* moves, int ring_u8, long long ring_ld, long long n, long long cols, long long nrows, long long start,
                             long long envs, long long pool, hipStream_t stream) {
  // the two spliced messages read "ring_store_frames_shared: src0, src1, arena and moves must not be null" and "ring_store_frames_shared:
  // the arena must be 16-byte, moves and fp32 sources 4-byte aligned" (tests/test_shared_next_host.py matches them)
  if (const int rc = check_frame_store("ring_store_frames_shared", true, src0, src0_u8, src0_ld, src1, src1_u8, src1_ld, arena && moves,
                                       "arena and moves", al16(arena) && al4p(moves), "the arena must be 16-byte, moves", ring_u8, ring_ld, n,
                                       cols, nrows, start, envs, pool))
    return rc;
  const int row4 = (int)(ring_ld / 4);   // groups of 4 pixels per arena row, a dword of bytes or a float4
  const long long total4 = n * row4, blocks = (total4 + 255) / 256;
  const frame_src s0 = make_frame_src(src0, src0_u8, src0_ld), s1 = make_frame_src(src1, src1_u8, src1_ld);
  if (ring_u8)
    hipLaunchKernelGGL(ring_store_frames_shared_kernel<true>, dim3((unsigned)blocks, 2), dim3(256), 0, stream, s0, s1, arena, moves, total4, row4,
                       (int)cols, nrows, start, n, envs, nrows + envs + pool);
  else
    hipLaunchKernelGGL(ring_store_frames_shared_kernel<false>, dim3((unsigned)blocks, 2), dim3(256), 0, stream, s0, s1, arena, moves, total4,
                       row4, (int)cols, nrows, start, n, envs, nrows + envs + pool);
  DGVIT_CHECK_LAUNCH("ring_store_frames_shared");
  return DGVIT_OK;
}

int ring_next_rows(const int* next_row, const long long* idx, long long* out, long long nsel, long long nrows, hipStream_t stream) {
  DGVIT_CHECK_ARG(next_row && idx && out, "ring_next_rows: next_row, idx and out must not be null");
  DGVIT_CHECK_ARG(nsel > 0 && nsel < (1ll << 31) && nrows > 0, "ring_next_rows: nsel=%lld must be in [1, 2^31) and nrows=%lld positive", nsel,
                  nrows);
  DGVIT_CHECK_ARG(al4p(next_row) && al8p(idx) && al8p(out), "ring_next_rows: next_row must be 4-byte, idx and out 8-byte aligned");
  hipLaunchKernelGGL(ring_next_rows_kernel, dim3((unsigned)((nsel + 255) / 256)), dim3(256), 0, stream, next_row, idx, out, nsel, nrows);
  DGVIT_CHECK_LAUNCH("ring_next_rows");
  return DGVIT_OK;
}

int ring_export(const dgvit_ring_view& ring, void* out, long long out_bytes, long long cols, long long nrows, long long oldest, long long a0,
                long long n, hipStream_t stream) {
  DGVIT_CHECK_ARG(ring.obs && ring.next_obs && out, "ring_export: obs, next_obs and out must not be null");
  DGVIT_CHECK_ARG(ring.frame_u8 == 0 || ring.frame_u8 == 1, "ring_export: frame_u8=%d must be 0 or 1", ring.frame_u8);
  DGVIT_CHECK_ARG(nrows > 0 && n >= 1 && n <= nrows, "ring_export: n=%lld must be in [1, nrows] and nrows=%lld positive", n, nrows);
  DGVIT_CHECK_ARG(a0 >= 0 && a0 <= nrows - n, "ring_export: ages a0=%lld .. a0 + n=%lld must lie inside the ring's [0, nrows=%lld]", a0, a0 + n,
                  nrows);
  DGVIT_CHECK_ARG(oldest >= 0 && oldest < nrows, "ring_export: oldest=%lld must be in [0, nrows) = [0, %lld)", oldest, nrows);
  DGVIT_CHECK_ARG(cols > 0 && cols <= (1ll << 25), "ring_export: cols=%lld must be in [1, 2^25]", cols);
  DGVIT_CHECK_ARG(ring.frame_ld % (ring.frame_u8 ? 16 : 4) == 0 && ring.frame_ld >= cols && ring.frame_ld <= (1ll << 26),
                  "ring_export: frame_ld=%lld must be a multiple of %d, at least cols=%lld and at most 2^26", ring.frame_ld,
                  ring.frame_u8 ? 16 : 4, cols);
  if (ring.next_row)
    DGVIT_CHECK_ARG(ring.next_rows >= nrows && ring.next_rows < (1ll << 31) && al4p(ring.next_row),
                    "ring_export: next_rows=%lld of a shared ring must be in [nrows, 2^31) and next_row 4-byte aligned", ring.next_rows);
  else
    DGVIT_CHECK_ARG(ring.next_rows == nrows, "ring_export: next_rows=%lld must be nrows=%lld without next_row", ring.next_rows, nrows);
  DGVIT_CHECK_ARG(al16(ring.obs) && al16(ring.next_obs), "ring_export: obs and next_obs must be 16-byte aligned");
  DGVIT_CHECK_ARG(al16(out), "ring_export: out, the chunk, must be 16-byte aligned");
  DGVIT_CHECK_ARG(!ring.leaves || al4p(ring.leaves), "ring_export: leaves must be 4-byte aligned");
  export_args p{};
  p.obs = static_cast<const unsigned char*>(ring.obs);
  p.next_obs = static_cast<const unsigned char*>(ring.next_obs);
  p.next_row = ring.next_row;
  p.flags = ring.flags;
  p.leaves = ring.leaves;
  const long long item = ring.frame_u8 ? 1 : 4;
  p.ring_bytes = ring.frame_ld * item;
  p.dense_bytes = cols * item;
  p.next_rows = ring.next_rows;
  const auto pad16 = [](long long b) { return (b + 15) & ~15ll; };
  long long off = 0, most = n;
  p.off[0] = off, off = pad16(off + n * p.dense_bytes);
  p.off[1] = off, off = pad16(off + n * p.dense_bytes);
  for (int f = 0; f < DGVIT_SMALL_FIELDS; ++f) {
    DGVIT_CHECK_ARG(ring.small[f], "ring_export: small[%d] must not be null", f);
    DGVIT_CHECK_ARG(ring.small_cols[f] >= 1 && ring.small_ld[f] >= ring.small_cols[f] && ring.small_ld[f] <= (1 << 20),
                    "ring_export: small_cols[%d]=%d must be at least 1 and small_ld[%d]=%d at least that and at most 2^20", f,
                    ring.small_cols[f], f, ring.small_ld[f]);
    DGVIT_CHECK_ARG(al4p(ring.small[f]), "ring_export: small[%d] must be 4-byte aligned", f);
    p.small[f] = ring.small[f], p.small_cols[f] = ring.small_cols[f], p.small_ld[f] = ring.small_ld[f];
    p.off[2 + f] = off, off = pad16(off + n * 4ll * ring.small_cols[f]);
    if (n * ring.small_cols[f] > most) most = n * ring.small_cols[f];
  }
  p.off[2 + DGVIT_SMALL_FIELDS] = off, off = pad16(off + n);
  p.off[3 + DGVIT_SMALL_FIELDS] = off;
  if (ring.leaves) off = pad16(off + 4 * n);
  DGVIT_CHECK_ARG(out_bytes >= off, "ring_export: out_bytes=%lld is less than the %lld bytes of n=%lld transitions", out_bytes, off, n);
  const int vec = p.dense_bytes % 16 == 0 ? 16 : (p.dense_bytes % 4 == 0 ? 4 : 1);
  const int units = (int)(p.dense_bytes / vec);
  if (n * units > most) most = n * units;
  const long long blocks = (most + 255) / 256;
  DGVIT_CHECK_ARG(blocks < (1ll << 31), "ring_export: n=%lld rows of cols=%lld are more than one launch covers", n, cols);
  const dim3 grid((unsigned)blocks, ring.leaves ? 4 + DGVIT_SMALL_FIELDS : 3 + DGVIT_SMALL_FIELDS);
  long long first = oldest + a0;   // oldest < nrows and a0 < nrows
  if (first >= nrows) first -= nrows;
  unsigned char* o = static_cast<unsigned char*>(out);
  {
    ProfileScope ps(PROF_OTHER, 0.0, stream);
    if (vec == 16) hipLaunchKernelGGL(ring_export_kernel<uint4>, grid, dim3(256), 0, stream, p, o, n, units, nrows, first);
    else if (vec == 4) hipLaunchKernelGGL(ring_export_kernel<uint32_t>, grid, dim3(256), 0, stream, p, o, n, units, nrows, first);
    else hipLaunchKernelGGL(ring_export_kernel<unsigned char>, grid, dim3(256), 0, stream, p, o, n, units, nrows, first);
  }
  DGVIT_CHECK_LAUNCH("ring_export");
  return DGVIT_OK;
}

int nstep_walk_strided(const float* rew, long long rew_ld, const float* done, long long done_ld, const unsigned char* flags,
                       const float* next_small, long long small_ld, const long long* idx, long long nsel, long long nrows, long long stride,
                       int n, double gamma, float* ret_out, float* done_out, float* discount_out, float* next_small_out, int* steps_out,
                       long long* tail_out, hipStream_t stream) {
  return launch_nstep_walk("nstep_walk_strided", rew, rew_ld, done, done_ld, flags, next_small, small_ld, idx, nsel, nrows, &stride, n, gamma,
                           ret_out, done_out, discount_out, next_small_out, steps_out, tail_out, stream);
}

namespace {

// the row table, the two sources and the output of both stacked gathers: what they ask alike -> cols * frames in *out_cols
int check_stack(const char* name, const void* src0, const void* src1, const long long* rows, const float* out, long long nsel, long long cols,
                int frames, int ring_u8, long long ring_ld, long long row_floats, long long nrows0, long long nrows1) {
  DGVIT_CHECK_ARG(src0 && src1 && rows && out, "%s: src0, src1, rows and out must not be null", name);
  DGVIT_CHECK_ARG(nsel > 0 && nsel < (1ll << 24), "%s: nsel=%lld must be in [1, 2^24)", name, nsel);   // one workgroup column per sample
  DGVIT_CHECK_ARG(nrows0 > 0 && nrows1 > 0, "%s: nrows0=%lld and nrows1=%lld must be positive", name, nrows0, nrows1);
  DGVIT_CHECK_ARG(frames >= 1 && frames <= STACK_MAX, "%s: frames=%d must be in [1, %d]", name, frames, STACK_MAX);
  DGVIT_CHECK_ARG(ring_u8 == 0 || ring_u8 == 1, "%s: ring_u8=%d must be 0 or 1", name, ring_u8);
  DGVIT_CHECK_ARG(cols > 0 && cols * frames <= (1ll << 27), "%s: cols=%lld must be positive and cols * frames=%lld at most 2^27", name, cols,
                  cols * frames);   // 32-bit element indices inside a row
  DGVIT_CHECK_ARG(ring_ld % (ring_u8 ? 16 : 4) == 0 && ring_ld >= cols && ring_ld <= (1ll << 26),
                  "%s: ring_ld=%lld must be a multiple of %d, at least cols=%lld and at most 2^26", name, ring_ld, ring_u8 ? 16 : 4, cols);
  DGVIT_CHECK_ARG(row_floats % 4 == 0 && row_floats >= cols * frames && row_floats <= (1ll << 27) + 4,
                  "%s: row_floats=%lld must be a multiple of 4 and at least cols * frames=%lld", name, row_floats, cols * frames);
  DGVIT_CHECK_ARG(al16(src0) && al16(src1) && al16(out) && al8p(rows), "%s: src0, src1 and out must be 16-byte aligned, rows 8-byte aligned",
                  name);
  return DGVIT_OK;
}

template <typename T, int K>
void launch_gather_stack_k(const void* src0, const void* src1, const long long* rows, float* out, long long nsel, int groups, int cols,
                           long long ld, int out4, long long nrows0, long long nrows1, hipStream_t stream) {
  hipLaunchKernelGGL((gather_stack_frames_kernel<T, K>), dim3((unsigned)nsel, (unsigned)((out4 + 256 * K - 1) / (256 * K))), dim3(256), 0,
                     stream, static_cast<const T*>(src0), static_cast<const T*>(src1), rows, out, groups, cols, ld, out4, nrows0, nrows1);
}

template <typename T>
void launch_gather_stack(int frames, const void* src0, const void* src1, const long long* rows, float* out, long long nsel, int groups,
                         int cols, long long ld, int out4, long long nrows0, long long nrows1, hipStream_t stream) {
#define DGVIT_STACK_CASE(K) \
  case K: return launch_gather_stack_k<T, K>(src0, src1, rows, out, nsel, groups, cols, ld, out4, nrows0, nrows1, stream)
  switch (frames) {
    DGVIT_STACK_CASE(1); DGVIT_STACK_CASE(2); DGVIT_STACK_CASE(3); DGVIT_STACK_CASE(4); DGVIT_STACK_CASE(5); DGVIT_STACK_CASE(6);
    DGVIT_STACK_CASE(7); DGVIT_STACK_CASE(8); DGVIT_STACK_CASE(9); DGVIT_STACK_CASE(10); DGVIT_STACK_CASE(11); DGVIT_STACK_CASE(12);
    DGVIT_STACK_CASE(13); DGVIT_STACK_CASE(14); DGVIT_STACK_CASE(15); DGVIT_STACK_CASE(16);
  }
#undef DGVIT_STACK_CASE
}

}  // namespace

int ring_stack_rows(const long long* idx, const long long* tail, const unsigned char* flags, const float* done, long long done_ld,
                    const int* next_row, long long* obs_rows, long long* next_rows, long long nsel, long long nrows, long long envs, int frames,
                    int full, long long arena_rows, hipStream_t stream) {
  DGVIT_CHECK_ARG(idx && flags && done && obs_rows && next_rows, "ring_stack_rows: idx, flags, done, obs_rows and next_rows must not be null");
  DGVIT_CHECK_ARG(nsel > 0 && nsel < (1ll << 31), "ring_stack_rows: nsel=%lld must be in [1, 2^31)", nsel);
  DGVIT_CHECK_ARG(nrows > 0 && nrows < (1ll << 56), "ring_stack_rows: nrows=%lld must be in [1, 2^56)", nrows);   // lane * envs cannot overflow
  DGVIT_CHECK_ARG(envs >= 1 && envs <= nrows && nrows % envs == 0, "ring_stack_rows: envs=%lld must be in [1, nrows] and divide nrows=%lld", envs,
                  nrows);
  DGVIT_CHECK_ARG(frames >= 1 && frames <= STACK_MAX, "ring_stack_rows: frames=%d must be in [1, %d]", frames, STACK_MAX);
  DGVIT_CHECK_ARG(full == 0 || full == 1, "ring_stack_rows: full=%d must be 0 or 1", full);
  DGVIT_CHECK_ARG(done_ld > 0, "ring_stack_rows: done_ld=%lld must be positive", done_ld);
  DGVIT_CHECK_ARG(next_row ? arena_rows >= nrows && arena_rows < (1ll << 31) : arena_rows == nrows,
                  "ring_stack_rows: arena_rows=%lld must be in [nrows, 2^31) with next_row and nrows=%lld without", arena_rows, nrows);
  DGVIT_CHECK_ARG(al8p(idx) && al8p(tail) && al8p(obs_rows) && al8p(next_rows) && al4p(done) && al4p(next_row),
                  "ring_stack_rows: idx, tail, obs_rows and next_rows must be 8-byte aligned, done and next_row 4-byte aligned");
  hipLaunchKernelGGL(ring_stack_rows_kernel, dim3((unsigned)((nsel + 3) / 4)), dim3(256), 0, stream, idx, tail, flags, done, done_ld, next_row,
                     obs_rows, next_rows, nsel, nrows, envs, frames, full, arena_rows);
  DGVIT_CHECK_LAUNCH("ring_stack_rows");
  return DGVIT_OK;
}

int gather_stack_frames(const void* src0, const void* src1, const long long* rows, float* out, long long nsel, long long cols, int frames,
                        int ring_u8, long long ring_ld, long long row_floats, long long nrows0, long long nrows1, hipStream_t stream) {
  if (const int rc = check_stack("gather_stack_frames", src0, src1, rows, out, nsel, cols, frames, ring_u8, ring_ld, row_floats, nrows0, nrows1))
    return rc;
  const int groups = (int)((cols + 3) / 4), out4 = (int)(row_floats / 4);
  if (ring_u8)
    launch_gather_stack<unsigned char>(frames, src0, src1, rows, out, nsel, groups, (int)cols, ring_ld, out4, nrows0, nrows1, stream);
  else
    launch_gather_stack<float>(frames, src0, src1, rows, out, nsel, groups, (int)cols, ring_ld, out4, nrows0, nrows1, stream);
  DGVIT_CHECK_LAUNCH("gather_stack_frames");
  return DGVIT_OK;
}

int gather_shift_stack_frames(const void* src0, const void* src1, const long long* rows, float* out, int* shifts_out, long long nsel, int H,
                              int W, int frames, int ring_u8, long long ring_ld, long long row_floats, long long nrows0, long long nrows1,
                              int pad, int stream_id, unsigned long long seed, const unsigned long long* seed_dev, hipStream_t stream) {
  const char* name = "gather_shift_stack_frames";
  DGVIT_CHECK_ARG(H > 0 && W > 0, "%s: frame H=%d W=%d must be positive", name, H, W);
  const long long cols = (long long)H * W;
  if (const int rc = check_stack(name, src0, src1, rows, out, nsel, cols, frames, ring_u8, ring_ld, row_floats, nrows0, nrows1)) return rc;
  DGVIT_CHECK_ARG(pad >= 0 && pad < H && pad < W, "%s: pad=%d must be in [0, min(H, W)) = [0, %d)", name, pad, H < W ? H : W);
  DGVIT_CHECK_ARG(stream_id >= 0 && stream_id < DGVIT_SHIFT_STREAMS, "%s: stream_id=%d must be in [0, %d)", name, stream_id, DGVIT_SHIFT_STREAMS);
  DGVIT_CHECK_ARG(al4p(shifts_out) && al8p(seed_dev), "%s: shifts_out must be 4-byte and seed_dev 8-byte aligned", name);
  const int out4 = (int)(row_floats / 4);
  const dim3 grid((unsigned)nsel, (unsigned)((out4 + 255) / 256));
  if (ring_u8)
    hipLaunchKernelGGL(gather_shift_stack_kernel<unsigned char>, grid, dim3(256), 0, stream, static_cast<const unsigned char*>(src0),
                       static_cast<const unsigned char*>(src1), rows, out, shifts_out, out4, ring_ld, nrows0, nrows1, H, W, frames, pad,
                       shift_tag(stream_id), seed, seed_dev);
  else
    hipLaunchKernelGGL(gather_shift_stack_kernel<float>, grid, dim3(256), 0, stream, static_cast<const float*>(src0),
                       static_cast<const float*>(src1), rows, out, shifts_out, out4, ring_ld, nrows0, nrows1, H, W, frames, pad,
                       shift_tag(stream_id), seed, seed_dev);
  DGVIT_CHECK_LAUNCH(name);
  return DGVIT_OK;
}

int frame_stack_push(float* stack, const float* frame, long long frame_ld, const unsigned char* reset, int reset_all, long long envs,
                     long long cols, int frames, hipStream_t stream) {
  DGVIT_CHECK_ARG(stack && frame, "frame_stack_push: stack and frame must not be null");
  DGVIT_CHECK_ARG(envs >= 1 && envs < (1ll << 24), "frame_stack_push: envs=%lld must be in [1, 2^24)", envs);
  DGVIT_CHECK_ARG(frames >= 1 && frames <= STACK_MAX, "frame_stack_push: frames=%d must be in [1, %d]", frames, STACK_MAX);
  DGVIT_CHECK_ARG(cols > 0 && cols * frames <= (1ll << 27), "frame_stack_push: cols=%lld must be positive and cols * frames=%lld at most 2^27",
                  cols, cols * frames);
  DGVIT_CHECK_ARG(frame_ld >= cols, "frame_stack_push: frame_ld=%lld must be at least cols=%lld", frame_ld, cols);
  DGVIT_CHECK_ARG(reset_all == 0 || reset_all == 1, "frame_stack_push: reset_all=%d must be 0 or 1", reset_all);
  DGVIT_CHECK_ARG(al4p(stack) && al4p(frame), "frame_stack_push: stack and frame must be 4-byte aligned");
  const long long total = envs * cols, blocks = (total + 255) / 256;
  DGVIT_CHECK_ARG(blocks < (1ll << 31), "frame_stack_push: envs=%lld frames of cols=%lld are more than one launch covers", envs, cols);
  hipLaunchKernelGGL(frame_stack_push_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, stack, frame, frame_ld, reset, reset_all, total,
                     (int)cols, frames);
  DGVIT_CHECK_LAUNCH("frame_stack_push");
  return DGVIT_OK;
}
