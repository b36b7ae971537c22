// Deterministic fixed-order reductions of fp32 slabs: the split-K partials of the weight-gradient GEMMs and the per-workgroup column
// partials of LayerNorm, the heads, the bf16 encoder and the CNN stack.  Several independent jobs share ONE launch (ReduceGroup,
// common.h); every sum is taken in a fixed order, so results are bit-identical from run to run.
#include <algorithm>

#include "common.h"

namespace {

// out1[0..n1) , out2[0..n-n1)  <-  sum over slabs of slab[z][0..n), for up to DGVIT_REDUCE_JOBS independent jobs in ONE launch
// (a transformer layer's four split-K weight gradients + its two LayerNorm parameter-gradient partials).
// 256 threads = CW float4 columns x GS slab groups (CW * GS = 256; jobs with few columns and many slabs -- LayerNorm partials --
// take CW = 16, GS = 16): group y sums slabs y, y+GS, y+2GS, ... with 4 loads in flight, then the GS partial sums are combined
// through LDS in a fixed (tree) order: deterministic for a given (nslab, GS).
__global__ void __launch_bounds__(256) reduce_group_kernel(const ReduceGroup g) {
  __shared__ float4 part[256];
  int j = 0;
#pragma unroll
  for (int t = 1; t < DGVIT_REDUCE_JOBS; ++t)
    if (t < g.njobs && (int)blockIdx.x >= g.first_block[t]) j = t;
  const ReduceJob job = g.job[j];
  const int cwl = job.cw_log, CW = 1 << cwl, GS = 256 >> cwl;
  const int tx = threadIdx.x & (CW - 1), ty = threadIdx.x >> cwl;
  const long long i = (long long)((int)blockIdx.x - g.first_block[j]) * CW + tx;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < job.n4) {
    const float4* src = reinterpret_cast<const float4*>(job.slabs) + i;
    const long long st4 = job.stride4;
    int z = ty;
    for (; z + 3 * GS < job.nslab; z += 4 * GS) {
      const float4 a = src[(z + 0 * GS) * st4], b = src[(z + 1 * GS) * st4], c = src[(z + 2 * GS) * st4], d = src[(z + 3 * GS) * st4];
      s.x += (a.x + b.x) + (c.x + d.x);
      s.y += (a.y + b.y) + (c.y + d.y);
      s.z += (a.z + b.z) + (c.z + d.z);
      s.w += (a.w + b.w) + (c.w + d.w);
    }
    for (; z < job.nslab; z += GS) {
      const float4 a = src[z * st4];
      s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w;
    }
  }
  part[ty * CW + tx] = s;
  __syncthreads();
  for (int half = GS >> 1; half >= 1; half >>= 1) {   // fixed pairing: (y, y + half)
    if (ty < half) {
      const float4 a = part[ty * CW + tx], b = part[(ty + half) * CW + tx];
      part[ty * CW + tx] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
    __syncthreads();
  }
  if (ty == 0 && i < job.n4) {
    const float4 r = part[tx];
    if (i < job.n14) reinterpret_cast<float4*>(job.out1)[i] = r;
    else reinterpret_cast<float4*>(job.out2)[i - job.n14] = r;
  }
}

__global__ void __launch_bounds__(256) reduce_slabs_scalar_kernel(const float* __restrict__ slabs, float* __restrict__ out1,
                                                                  float* __restrict__ out2, long long n, long long n1, int nslab,
                                                                  long long stride) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int z = 0; z < nslab; ++z) s += slabs[z * stride + i];
  if (i < n1) out1[i] = s;
  else out2[i - n1] = s;
}

// n 32-bit words at p <- 0: 16-byte stores over the aligned body, word stores over the (at most three) words before and behind it
__global__ void __launch_bounds__(256) zero_words_kernel(unsigned* __restrict__ p, long long n) {
  const long long head = min(n, (long long)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2));
  const long long n4 = (n - head) >> 2;
  uint4* body = reinterpret_cast<uint4*>(p + head);
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) body[i] = make_uint4(0u, 0u, 0u, 0u);
  if (blockIdx.x == 0) {
    const long long tail0 = head + 4 * n4;
    if (threadIdx.x < head) p[threadIdx.x] = 0u;
    if (tail0 + threadIdx.x < n) p[tail0 + threadIdx.x] = 0u;      // n - tail0 <= 3
  }
}

}  // namespace

int zero_fill(void* p, long long bytes, hipStream_t stream) {
  if (bytes == 0) return DGVIT_OK;
  DGVIT_CHECK_ARG(p && bytes > 0 && bytes % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 3) == 0, "zero_fill: needs whole, aligned 32-bit words");
  const long long n = bytes / 4, blocks = (n / 4 + 255) / 256;
  hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)std::min<long long>(std::max<long long>(blocks, 1), 4096)), dim3(256), 0, stream,
                     reinterpret_cast<unsigned*>(p), n);
  DGVIT_CHECK_LAUNCH("zero_fill");
  return DGVIT_OK;
}

// ---- grouped deterministic reductions ----------------------------------------------------------------------------------
void reduce_group_init(ReduceGroup& g) { g.njobs = 0; g.first_block[0] = 0; }

// launch every queued job as ONE kernel (no-op when empty)
int reduce_group_flush(ReduceGroup& g, hipStream_t stream) {
  if (g.njobs == 0) return DGVIT_OK;
  {
    ProfileScope t(PROF_OTHER, 0.0, stream);
    hipLaunchKernelGGL(reduce_group_kernel, dim3((unsigned)g.first_block[g.njobs]), dim3(256), 0, stream, g);
  }
  g.njobs = 0;
  DGVIT_CHECK_LAUNCH("reduce_group");
  return DGVIT_OK;
}

// queue: out1 gets the first n1 sums, out2 (may be null when n1 == n) the remaining n - n1, of nslab slabs slab_stride floats apart.
// Jobs that cannot take the float4 path (odd sizes / alignment: tiny head Linears) run at once on the scalar kernel.
int reduce_group_add(ReduceGroup& g, const float* slabs, float* out1, long long n1, float* out2, long long n, int nslab,
                     long long slab_stride, hipStream_t stream) {
  DGVIT_CHECK_ARG(slabs && out1 && n > 0 && n1 > 0 && n1 <= n && nslab >= 1 && (n1 == n || out2), "reduce_slabs: bad arguments");
  if (!(n % 4 == 0 && n1 % 4 == 0 && slab_stride % 4 == 0 && al16(slabs) && al16(out1) && (n1 == n || al16(out2)))) {
    {
      ProfileScope t(PROF_OTHER, 0.0, stream);
      hipLaunchKernelGGL(reduce_slabs_scalar_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, slabs, out1, out2, n, n1,
                         nslab, slab_stride);
    }
    DGVIT_CHECK_LAUNCH("reduce_slabs");
    return DGVIT_OK;
  }
  if (g.njobs == DGVIT_REDUCE_JOBS) TRY(reduce_group_flush(g, stream));
  ReduceJob& job = g.job[g.njobs];
  job.slabs = slabs; job.out1 = out1; job.out2 = out2;
  job.n4 = n / 4; job.n14 = n1 / 4; job.nslab = nslab; job.stride4 = slab_stride / 4;
  job.cw_log = (job.n4 <= 1024 && nslab >= 64) ? 4 : 6;   // few columns, many slabs: 16 slab groups per block
  const long long blocks = (job.n4 + (1 << job.cw_log) - 1) >> job.cw_log;
  DGVIT_CHECK_ARG(blocks + g.first_block[g.njobs] < (1ll << 30), "reduce_slabs: too many blocks");
  g.first_block[g.njobs + 1] = g.first_block[g.njobs] + (int)blocks;
  ++g.njobs;
  return DGVIT_OK;
}

// out1 gets the first n1 sums, out2 (may be null when n1 == n) the remaining n - n1
int reduce_slabs2(const float* slabs, float* out1, long long n1, float* out2, long long n, int nslab, long long slab_stride,
                  hipStream_t stream) {
  ReduceGroup g;
  reduce_group_init(g);
  TRY(reduce_group_add(g, slabs, out1, n1, out2, n, nslab, slab_stride, stream));
  return reduce_group_flush(g, stream);
}

int reduce_slabs(const float* slabs, float* out, long long n, int nslab, long long slab_stride, hipStream_t stream) {
  return reduce_slabs2(slabs, out, n, nullptr, n, nslab, slab_stride, stream);
}
