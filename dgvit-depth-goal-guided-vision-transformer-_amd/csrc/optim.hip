// Optimiser-side kernels for the step AFTER the hot path: the reference runs
// torch.optim.Adam over ~70 tensors per network (DRL.py:401-403,412-414) and a per-parameter Python loop for the
// Polyak target update (utils.py:31-33).  Here both are one HBM-bound pass over a flat fp32 buffer.
//   adam_step   : torch.optim.Adam semantics (bias-corrected, eps added to sqrt(v_hat), optional L2 weight decay)
//   soft_update : target <- target * (1 - tau) + source * tau
// Algorithmic bytes: Adam 28 B/parameter (read p,g,m,v; write p,m,v), soft update 12 B/parameter.
// Gradient-norm clipping (torch.nn.utils.clip_grad_norm_, attention_imitating.py:45-67) between the backward and Adam:
//   grad_sqnorm_partials   : per-workgroup sums of g*g over a flat gradient buffer, in double (4 B/parameter, one read)
//   grad_clip_coef         : partials -> total norm and the clamped coefficient max_norm / (norm + 1e-6), both left on the device
//   adam_step_scaled       : adam_step with the gradient multiplied by that device-side coefficient as it is read (still 28 B/parameter)
//   scale_by_device_scalar : x <- x * *scale, the in-place form for a stand-alone clip (8 B/parameter)
// Parameter groups and learning-rate schedules (torch.optim.AdamW, warm-up + cosine / linear decay):
//   adam_step_groups       : the step over one run whose elements belong to groups with their own (lr, weight decay), L2 or decoupled
//                            decay, the schedule factor computed on the device -- still one launch and 28 B/parameter
#include "common.h"
#include "kernels.h"

namespace {

// a * b rounded to fp32 on its own.  HIP's __fmul_rn is a plain product that the compiler may contract into a following add; with
// contraction switched off for this expression the product keeps its own rounding wherever the function is inlined.
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// SCALED: every gradient element is first multiplied by *grad_scale_dev (the clip coefficient of grad_clip_coef_kernel) and rounded to
// fp32 on its own -- mul_rounded: never contracted into the weight-decay FMA -- so the step is bit-identical to an unscaled step on a
// gradient buffer that was multiplied by the same scalar beforehand.  SCALED = false is the kernel as it always was.
template <bool SCALED>
__global__ void __launch_bounds__(256) adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, long long n4, float lr_c, float beta1, float beta2,
                                                   float inv_sqrt_bc2, float eps, float wd, float lr,
                                                   const long long* __restrict__ step_dev, const float* __restrict__ grad_scale_dev) {
  float gscale = 1.f;
  if (SCALED) gscale = *grad_scale_dev;
  if (step_dev) {   // graph-capturable form: bias corrections from the device-side step counter
    const float t = (float)*step_dev;
    lr_c = lr / (1.f - powf(beta1, t));
    inv_sqrt_bc2 = rsqrtf(1.f - powf(beta2, t));
  }
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv0 = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float pe[4] = {pv.x, pv.y, pv.z, pv.w}, ge[4] = {gv0.x, gv0.y, gv0.z, gv0.w};
    float me[4] = {mv.x, mv.y, mv.z, mv.w}, ve[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (SCALED) ge[e] = mul_rounded(gscale, ge[e]);
      const float gg = ge[e] + wd * pe[e];
      me[e] = beta1 * me[e] + (1.f - beta1) * gg;
      ve[e] = beta2 * ve[e] + (1.f - beta2) * gg * gg;
      pe[e] -= lr_c * me[e] / (sqrtf(ve[e]) * inv_sqrt_bc2 + eps);
    }
    reinterpret_cast<float4*>(p)[i] = make_float4(pe[0], pe[1], pe[2], pe[3]);
    reinterpret_cast<float4*>(m)[i] = make_float4(me[0], me[1], me[2], me[3]);
    reinterpret_cast<float4*>(v)[i] = make_float4(ve[0], ve[1], ve[2], ve[3]);
  }
}

// Parameter groups and a device-side learning-rate schedule in the same single pass.  The run [0, n4) is cut into nseg
// segments (seg_end4: ascending ends in float4 units, seg_group: the group of each); a group is (lr, weight_decay).  Every workgroup
// stages both segment tables and the per-group constants into LDS once; a lane then keeps a cursor k into the segment table: its index
// only grows along the grid-stride walk, so the cursor only moves forward -- one LDS read (a broadcast: a wave's 64 consecutive float4s
// nearly always share a segment) while the lane stays inside its segment, a binary search over the REMAINING segments when it left it.
// The four global loads of an iteration are issued before the lookup, so the LDS round trips wait under the HBM latency.  Which element
// gets which group depends on i alone: the result does not depend on the grid.
//   f      : the schedule factor, by thread 0 in double from the number of steps already taken, rounded to fp32 once
//   lr_t   : lr * f (one fp32 product); bias corrections ALWAYS by the device formula of adam_kernel's step_dev branch, from
//            t = *step_dev or the host's step: an eager and a captured step run the same instructions on the same values
//   L2     : adam_kernel's lines with the group's wd and lr_c            DECOUPLED : p *= 1 - lr_t * wd first, moments from the raw g
constexpr int ADAM_MAX_SEGMENTS = 2048, ADAM_MAX_GROUPS = 256;
template <bool SCALED, bool DECOUPLED>
__global__ void __launch_bounds__(256) adam_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, long long n4, const long long* __restrict__ seg_end4,
                                                          const unsigned char* __restrict__ seg_group, int nseg,
                                                          const float* __restrict__ group_hyper, int ngroups, float* __restrict__ lr_out,
                                                          float beta1, float beta2, float eps, long long step, long long sched_step,
                                                          const long long* __restrict__ step_dev, int sched_kind, long long warmup_steps,
                                                          long long total_steps, float final_ratio,
                                                          const float* __restrict__ grad_scale_dev) {
  __shared__ long long s_end[ADAM_MAX_SEGMENTS];
  __shared__ unsigned char s_grp[ADAM_MAX_SEGMENTS];
  // L2: lr_c, wd      DECOUPLED: lr_c, 1 - lr_t * wd.  20480 bytes of LDS in all: eight workgroups per CU, the whole grid resident
  __shared__ float s_lrc[ADAM_MAX_GROUPS], s_wd[ADAM_MAX_GROUPS];
  float gscale = 1.f;
  if (SCALED) gscale = *grad_scale_dev;
  const long long t_dev = step_dev ? *step_dev : step;
  if (threadIdx.x == 0) {
    const long long s = (step_dev ? t_dev : sched_step) - 1;   // steps already taken
    double f;
    if (s < warmup_steps) {
      f = (double)(s + 1) / (double)warmup_steps;
    } else {
      const long long span = total_steps - warmup_steps;
      double q = (double)(s - warmup_steps) / (double)(span > 1 ? span : 1);
      q = q < 1.0 ? q : 1.0;
      const double r = (double)final_ratio;
      f = sched_kind == 1 ? r + (1.0 - r) * 0.5 * (1.0 + cospi(q)) : sched_kind == 2 ? r + (1.0 - r) * (1.0 - q) : 1.0;
    }
    s_lrc[0] = (float)f;   // (handed to the workgroup through a slot that is filled for good after the next barrier)
  }
  for (int k = threadIdx.x; k < nseg; k += 256) {
    s_end[k] = seg_end4[k];
    const int gr = seg_group[k];
    s_grp[k] = (unsigned char)(gr < ngroups ? gr : ngroups - 1);   // (a table that breaks its contract still indexes inside the LDS)
  }
  __syncthreads();
  const float f = s_lrc[0];
  __syncthreads();
  const float t = (float)t_dev;
  const float bc1 = 1.f - powf(beta1, t);
  const float inv_sqrt_bc2 = rsqrtf(1.f - powf(beta2, t));
  if ((int)threadIdx.x < ngroups) {
    const float lr_t = mul_rounded(group_hyper[2 * threadIdx.x], f);
    const float wd = group_hyper[2 * threadIdx.x + 1];
    s_lrc[threadIdx.x] = lr_t / bc1;
    s_wd[threadIdx.x] = DECOUPLED ? (float)(1.0 - (double)lr_t * (double)wd) : wd;
    if (lr_out && blockIdx.x == 0) lr_out[threadIdx.x] = lr_t;
  }
  __syncthreads();
  const long long stride = (long long)gridDim.x * 256;
  int k = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv0 = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    if (i >= s_end[k]) {   // left the segment: the first one that ends beyond i, among those after k
      int lo = k + 1, hi = nseg - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (i < s_end[mid]) hi = mid; else lo = mid + 1;
      }
      k = lo < nseg ? lo : nseg - 1;
    }
    const int gr = s_grp[k];
    const float lr_c = s_lrc[gr], wd = s_wd[gr];
    float pe[4] = {pv.x, pv.y, pv.z, pv.w}, ge[4] = {gv0.x, gv0.y, gv0.z, gv0.w};
    float me[4] = {mv.x, mv.y, mv.z, mv.w}, ve[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (SCALED) ge[e] = mul_rounded(gscale, ge[e]);
      float gg;
      if (DECOUPLED) {
        pe[e] = mul_rounded(pe[e], wd);
        gg = ge[e];
      } else {
        gg = ge[e] + wd * pe[e];
      }
      me[e] = beta1 * me[e] + (1.f - beta1) * gg;
      ve[e] = beta2 * ve[e] + (1.f - beta2) * gg * gg;
      pe[e] -= lr_c * me[e] / (sqrtf(ve[e]) * inv_sqrt_bc2 + eps);
    }
    reinterpret_cast<float4*>(p)[i] = make_float4(pe[0], pe[1], pe[2], pe[3]);
    reinterpret_cast<float4*>(m)[i] = make_float4(me[0], me[1], me[2], me[3]);
    reinterpret_cast<float4*>(v)[i] = make_float4(ve[0], ve[1], ve[2], ve[3]);
  }
}

__global__ void __launch_bounds__(256) soft_update_kernel(float* __restrict__ tgt, const float* __restrict__ src, long long n4,
                                                          float tau) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    float4 t = reinterpret_cast<float4*>(tgt)[i];
    const float4 s = reinterpret_cast<const float4*>(src)[i];
    t.x = t.x * (1.f - tau) + s.x * tau;
    t.y = t.y * (1.f - tau) + s.y * tau;
    t.z = t.z * (1.f - tau) + s.z * tau;
    t.w = t.w * (1.f - tau) + s.w * tau;
    reinterpret_cast<float4*>(tgt)[i] = t;
  }
}

// Sum of g*g over a flat buffer, one partial per workgroup.  The grid is ALWAYS DGVIT_GRAD_NORM_PARTIALS workgroups, so which elements
// a lane sums -- and with that the result, bit for bit -- depends on n alone, never on the device.  Accumulation is in double: the pass
// is HBM-bound at 4 B/element, the fp64 FMAs ride along, and the rounding of a lane's sum does not grow with the elements it walks.
// Four float4 loads are in flight per lane (latency, not issue rate, bounds a streaming read); the four of a round go into four
// accumulators in a fixed order.  Workgroup b owns partials[b]: a plain store (or, accumulating, its own earlier value plus the sum,
// ordered by the stream) -- no atomics, no counters, nothing to zero beforehand.
__global__ void __launch_bounds__(256) grad_sqnorm_partials_kernel(const float* __restrict__ g, long long n4, double* __restrict__ partials,
                                                                   int accumulate) {
  __shared__ double wave_sum[4];
  const long long stride = (long long)DGVIT_GRAD_NORM_PARTIALS * 256;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {
    float4 q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) q[u] = reinterpret_cast<const float4*>(g)[i + u * stride];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc[u] = fma((double)q[u].x, (double)q[u].x, acc[u]);
      acc[u] = fma((double)q[u].y, (double)q[u].y, acc[u]);
      acc[u] = fma((double)q[u].z, (double)q[u].z, acc[u]);
      acc[u] = fma((double)q[u].w, (double)q[u].w, acc[u]);
    }
  }
  for (; i < n4; i += stride) {
    const float4 q = reinterpret_cast<const float4*>(g)[i];
    acc[0] = fma((double)q.x, (double)q.x, acc[0]);
    acc[0] = fma((double)q.y, (double)q.y, acc[0]);
    acc[0] = fma((double)q.z, (double)q.z, acc[0]);
    acc[0] = fma((double)q.w, (double)q.w, acc[0]);
  }
  double s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double tot = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
    partials[blockIdx.x] = accumulate ? partials[blockIdx.x] + tot : tot;
  }
}

// One workgroup: the partials summed in a fixed order in double, then torch.nn.utils.clip_grad_norm_'s arithmetic in fp32:
//   clip_coef = max_norm / (total_norm + 1e-6), which torch evaluates as (total_norm + 1e-6).reciprocal() * max_norm (Tensor.__rtruediv__),
//   then clamp(max=1.0).  A NaN norm keeps a NaN coefficient as torch.clamp does (fminf would return 1); an infinite norm gives 0.
__global__ void __launch_bounds__(256) grad_clip_coef_kernel(const double* __restrict__ partials, float max_norm, float* __restrict__ out) {
  __shared__ double wave_sum[4];
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < DGVIT_GRAD_NORM_PARTIALS / 256; ++k) s += partials[k * 256 + threadIdx.x];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt((wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]));
    const float coef = mul_rounded(__fdiv_rn(1.f, __fadd_rn(norm, 1e-6f)), max_norm);
    out[0] = norm;
    out[1] = coef > 1.f ? 1.f : coef;
  }
}
static_assert(DGVIT_GRAD_NORM_PARTIALS % 256 == 0 && DGVIT_GRAD_NORM_PARTIALS >= 512 && DGVIT_GRAD_NORM_PARTIALS <= 2048,
              "grad_clip_coef_kernel reads DGVIT_GRAD_NORM_PARTIALS / 256 partials per thread");

__global__ void __launch_bounds__(256) scale_by_device_scalar_kernel(float* __restrict__ x, long long n4, const float* __restrict__ scale_dev) {
  const float s = *scale_dev;
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    float4 t = reinterpret_cast<float4*>(x)[i];
    t.x = mul_rounded(s, t.x);
    t.y = mul_rounded(s, t.y);
    t.z = mul_rounded(s, t.z);
    t.w = mul_rounded(s, t.w);
    reinterpret_cast<float4*>(x)[i] = t;
  }
}

inline unsigned grid_for(long long n4) {
  long long b = (n4 + 255) / 256;
  if (b > 2048) b = 2048;  // 8 workgroups per CU, grid-stride beyond
  return (unsigned)(b < 1 ? 1 : b);
}

}  // namespace

// n must be a multiple of 4 and the buffers 16-byte aligned (the flat buffers of dgvit_amd.optim are)
int adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
              float weight_decay, long long step, const long long* step_dev, hipStream_t stream) {
  DGVIT_CHECK_ARG(p && g && m && v && n > 0 && n % 4 == 0, "adam_step: n must be a positive multiple of 4");
  DGVIT_CHECK_ARG(al16(p) && al16(g) && al16(m) && al16(v), "adam_step: buffers must be 16-byte aligned");
  DGVIT_CHECK_ARG((step >= 1 || step_dev) && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "adam_step: bad hyper-parameters");
  const double bc1 = 1.0 - pow((double)beta1, (double)(step >= 1 ? step : 1));
  const double bc2 = 1.0 - pow((double)beta2, (double)(step >= 1 ? step : 1));
  {
    ProfileScope t(PROF_OTHER, 0.0, stream);
    hipLaunchKernelGGL(adam_kernel<false>, dim3(grid_for(n / 4)), dim3(256), 0, stream, p, g, m, v, n / 4, (float)(lr / bc1), beta1, beta2,
                       (float)(1.0 / sqrt(bc2)), eps, weight_decay, lr, step_dev, (const float*)nullptr);
  }
  DGVIT_CHECK_LAUNCH("adam_step");
  return DGVIT_OK;
}

// adam_step on the gradient g * *grad_scale_dev (a device scalar, read when the kernel runs): the clipped step without a clipped copy
int adam_step_scaled(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
                     float weight_decay, long long step, const long long* step_dev, const float* grad_scale_dev, hipStream_t stream) {
  DGVIT_CHECK_ARG(p && g && m && v, "adam_step_scaled: p, g, m and v must not be null");
  DGVIT_CHECK_ARG(grad_scale_dev, "adam_step_scaled: grad_scale_dev must not be null (the unscaled step is adam_step)");
  DGVIT_CHECK_ARG(n > 0 && n % 4 == 0, "adam_step_scaled: n=%lld must be a positive multiple of 4", n);
  DGVIT_CHECK_ARG(al16(p) && al16(g) && al16(m) && al16(v), "adam_step_scaled: buffers must be 16-byte aligned");
  DGVIT_CHECK_ARG((reinterpret_cast<uintptr_t>(grad_scale_dev) & 3) == 0, "adam_step_scaled: grad_scale_dev must be 4-byte aligned");
  DGVIT_CHECK_ARG((step >= 1 || step_dev) && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "adam_step_scaled: bad hyper-parameters");
  const double bc1 = 1.0 - pow((double)beta1, (double)(step >= 1 ? step : 1));
  const double bc2 = 1.0 - pow((double)beta2, (double)(step >= 1 ? step : 1));
  {
    ProfileScope t(PROF_OTHER, 0.0, stream);
    hipLaunchKernelGGL(adam_kernel<true>, dim3(grid_for(n / 4)), dim3(256), 0, stream, p, g, m, v, n / 4, (float)(lr / bc1), beta1, beta2,
                       (float)(1.0 / sqrt(bc2)), eps, weight_decay, lr, step_dev, grad_scale_dev);
  }
  DGVIT_CHECK_LAUNCH("adam_step_scaled");
  return DGVIT_OK;
}

// Adam / AdamW over one run with parameter groups and a learning-rate schedule evaluated on the device (adam_groups_kernel above).
// Everything is refused here, before any launch, that the kernel could not survive or would silently misread.
int adam_step_groups(float* p, const float* g, float* m, float* v, long long n, const long long* seg_end4, const unsigned char* seg_group,
                     int nseg, const float* group_hyper, int ngroups, float* lr_out, float beta1, float beta2, float eps, int decoupled,
                     long long step, long long sched_step, const long long* step_dev, int sched_kind, long long warmup_steps,
                     long long total_steps, float final_ratio, const float* grad_scale_dev, hipStream_t stream) {
  DGVIT_CHECK_ARG(p && g && m && v, "adam_step_groups: p, g, m and v must not be null");
  DGVIT_CHECK_ARG(seg_end4 && seg_group, "adam_step_groups: seg_end4 and seg_group must not be null");
  DGVIT_CHECK_ARG(group_hyper, "adam_step_groups: group_hyper must not be null");
  DGVIT_CHECK_ARG(n > 0 && n % 4 == 0, "adam_step_groups: n=%lld must be a positive multiple of 4", n);
  DGVIT_CHECK_ARG(al16(p) && al16(g) && al16(m) && al16(v), "adam_step_groups: p, g, m and v must be 16-byte aligned");
  DGVIT_CHECK_ARG((reinterpret_cast<uintptr_t>(seg_end4) & 7) == 0, "adam_step_groups: seg_end4 must be 8-byte aligned");
  DGVIT_CHECK_ARG((reinterpret_cast<uintptr_t>(group_hyper) & 3) == 0, "adam_step_groups: group_hyper must be 4-byte aligned");
  DGVIT_CHECK_ARG((reinterpret_cast<uintptr_t>(lr_out) & 3) == 0, "adam_step_groups: lr_out must be 4-byte aligned");
  DGVIT_CHECK_ARG((reinterpret_cast<uintptr_t>(grad_scale_dev) & 3) == 0, "adam_step_groups: grad_scale_dev must be 4-byte aligned");
  DGVIT_CHECK_ARG((reinterpret_cast<uintptr_t>(step_dev) & 7) == 0, "adam_step_groups: step_dev must be 8-byte aligned");
  DGVIT_CHECK_ARG(nseg >= 1 && nseg <= ADAM_MAX_SEGMENTS, "adam_step_groups: nseg=%d must be in 1..%d", nseg, ADAM_MAX_SEGMENTS);
  DGVIT_CHECK_ARG(ngroups >= 1 && ngroups <= ADAM_MAX_GROUPS, "adam_step_groups: ngroups=%d must be in 1..%d", ngroups, ADAM_MAX_GROUPS);
  DGVIT_CHECK_ARG(beta1 >= 0.f && beta1 < 1.f, "adam_step_groups: beta1=%g must be in [0, 1)", (double)beta1);
  DGVIT_CHECK_ARG(beta2 >= 0.f && beta2 < 1.f, "adam_step_groups: beta2=%g must be in [0, 1)", (double)beta2);
  DGVIT_CHECK_ARG(step_dev || step >= 1, "adam_step_groups: step=%lld must be at least 1 without step_dev", step);
  DGVIT_CHECK_ARG(step_dev || sched_step >= 1, "adam_step_groups: sched_step=%lld must be at least 1 without step_dev", sched_step);
  DGVIT_CHECK_ARG(sched_kind >= 0 && sched_kind <= 2, "adam_step_groups: sched_kind=%d must be 0 (constant), 1 (cosine) or 2 (linear)", sched_kind);
  DGVIT_CHECK_ARG(warmup_steps >= 0, "adam_step_groups: warmup_steps=%lld must not be negative", warmup_steps);
  DGVIT_CHECK_ARG(sched_kind == 0 || total_steps >= warmup_steps, "adam_step_groups: total_steps=%lld must not be below warmup_steps=%lld",
                  total_steps, warmup_steps);
  DGVIT_CHECK_ARG(std::isfinite(final_ratio) && final_ratio >= 0.f && final_ratio <= 1.f, "adam_step_groups: final_ratio=%g must be in [0, 1]",
                  (double)final_ratio);
  {
    ProfileScope t(PROF_OTHER, 0.0, stream);
    auto kernel = grad_scale_dev ? (decoupled ? adam_groups_kernel<true, true> : adam_groups_kernel<true, false>)
                                 : (decoupled ? adam_groups_kernel<false, true> : adam_groups_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(grid_for(n / 4)), dim3(256), 0, stream, p, g, m, v, n / 4, seg_end4, seg_group, nseg, group_hyper, ngroups,
                       lr_out, beta1, beta2, eps, step, sched_step, step_dev, sched_kind, warmup_steps, total_steps, final_ratio,
                       grad_scale_dev);
  }
  DGVIT_CHECK_LAUNCH("adam_step_groups");
  return DGVIT_OK;
}

int grad_sqnorm_partials(const float* g, long long n, double* partials, int accumulate, hipStream_t stream) {
  DGVIT_CHECK_ARG(g && partials, "grad_sqnorm_partials: g and partials must not be null");
  DGVIT_CHECK_ARG(n > 0 && n % 4 == 0, "grad_sqnorm_partials: n=%lld must be a positive multiple of 4", n);
  DGVIT_CHECK_ARG(al16(g) && al16(partials), "grad_sqnorm_partials: g and partials must be 16-byte aligned");
  {
    ProfileScope t(PROF_OTHER, 0.0, stream);
    hipLaunchKernelGGL(grad_sqnorm_partials_kernel, dim3(DGVIT_GRAD_NORM_PARTIALS), dim3(256), 0, stream, g, n / 4, partials, accumulate);
  }
  DGVIT_CHECK_LAUNCH("grad_sqnorm_partials");
  return DGVIT_OK;
}

int grad_clip_coef(const double* partials, float max_norm, float* out, hipStream_t stream) {
  DGVIT_CHECK_ARG(partials && out, "grad_clip_coef: partials and out must not be null");
  DGVIT_CHECK_ARG(std::isfinite(max_norm) && max_norm > 0.f, "grad_clip_coef: max_norm=%g must be finite and greater than 0", (double)max_norm);
  DGVIT_CHECK_ARG(al16(partials), "grad_clip_coef: partials must be 16-byte aligned");
  DGVIT_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 3) == 0, "grad_clip_coef: out must be 4-byte aligned");
  {
    ProfileScope t(PROF_OTHER, 0.0, stream);
    hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(256), 0, stream, partials, max_norm, out);
  }
  DGVIT_CHECK_LAUNCH("grad_clip_coef");
  return DGVIT_OK;
}

int scale_by_device_scalar(float* x, long long n, const float* scale_dev, hipStream_t stream) {
  DGVIT_CHECK_ARG(x && scale_dev, "scale_by_device_scalar: x and scale_dev must not be null");
  DGVIT_CHECK_ARG(n > 0 && n % 4 == 0, "scale_by_device_scalar: n=%lld must be a positive multiple of 4", n);
  DGVIT_CHECK_ARG(al16(x), "scale_by_device_scalar: x must be 16-byte aligned");
  DGVIT_CHECK_ARG((reinterpret_cast<uintptr_t>(scale_dev) & 3) == 0, "scale_by_device_scalar: scale_dev must be 4-byte aligned");
  {
    ProfileScope t(PROF_OTHER, 0.0, stream);
    hipLaunchKernelGGL(scale_by_device_scalar_kernel, dim3(grid_for(n / 4)), dim3(256), 0, stream, x, n / 4, scale_dev);
  }
  DGVIT_CHECK_LAUNCH("scale_by_device_scalar");
  return DGVIT_OK;
}

int soft_update(float* target, const float* source, long long n, float tau, hipStream_t stream) {
  DGVIT_CHECK_ARG(target && source && n > 0 && n % 4 == 0, "soft_update: n must be a positive multiple of 4");
  DGVIT_CHECK_ARG(al16(target) && al16(source), "soft_update: buffers must be 16-byte aligned");
  hipLaunchKernelGGL(soft_update_kernel, dim3(grid_for(n / 4)), dim3(256), 0, stream, target, source, n / 4, tau);
  DGVIT_CHECK_LAUNCH("soft_update");
  return DGVIT_OK;
}
