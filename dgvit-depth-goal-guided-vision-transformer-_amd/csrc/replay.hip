// Prioritized experience replay on the device (proportional PER, Schaul et al. 2016): a radix-64 sum / min tree over the
// ring's slots in ONE fp32 buffer, so that a wave64 handles one sample and one wave instruction reads the 64 children of a node.
//   per_init      : sums 0, mins +inf, max leaf 1
//   per_set_range : leaves [first, first + count) <- the max leaf (a newly stored transition), ancestors rebuilt
//   per_set_leaves: leaves [first, first + count) <- given values, clamped as a leaf is; ancestors rebuilt as per_set_range's
//   per_update    : leaf[idx[j]] <- clamp((|prio[j]| + eps)^alpha, 2^-64, 2^64), ancestors rebuilt
//   per_sample    : u[j] -> (leaf index, importance weight (p_min / leaf)^beta) by a descent from the top block
//
// Layout (floats): [0, 64) header, word 0 = the running max leaf, word 1 = its value when the running update began; then for each
// level l = 0 .. L-1 pad64(n_l) sums followed by pad64(n_l) mins, n_0 = capacity, n_l = ceil(n_{l-1} / 64), the last level the first
// with n_l <= 64 (the top block: there is no separate root).  Padding and never-written slots hold sum 0 and min +inf.
//
// A parent is ALWAYS recomputed from its 64 children with the same xor butterfly (never updated by a delta): its value is a pure function
// of its children, two waves that rebuild the same parent write the same bits, fp32 drift cannot accumulate and there is no float atomic
// anywhere.  Level 1 takes its min from the children's SUMS (a stored leaf is >= 2^-64, so sum > 0 <=> stored), which is what lets the
// same pass write the leaf's own min word without a race between the waves of one parent.
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int PER_MAX_LEVELS = 4;                 // 64^4 = 2^24 slots
constexpr long long PER_MAX_CAPACITY = 1ll << 24;
constexpr int PER_HEADER = 64;
constexpr float PER_LEAF_MIN = 0x1p-64f, PER_LEAF_MAX = 0x1p64f;

struct PerTree {
  int levels;
  int n[PER_MAX_LEVELS];          // entries of level l
  int pad[PER_MAX_LEVELS];        // ... padded to a multiple of 64: the level's mins start `pad` floats behind its sums
  long long off[PER_MAX_LEVELS];  // float offset of the level's sums
  long long total;                // floats of the whole buffer
};

bool per_layout(long long capacity, PerTree& t) {
  if (capacity < 1 || capacity > PER_MAX_CAPACITY) return false;
  t = PerTree{};
  long long n = capacity, off = PER_HEADER;
  for (int l = 0; l < PER_MAX_LEVELS; ++l) {
    t.n[l] = (int)n;
    t.pad[l] = (int)((n + 63) / 64 * 64);
    t.off[l] = off;
    off += 2ll * t.pad[l];
    t.levels = l + 1;
    if (n <= 64) break;
    n = (n + 63) / 64;
  }
  t.total = off;
  return true;
}

__device__ __forceinline__ float wave_sum(float v) {   // the fixed order every parent is summed in; all 64 lanes hold the result
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// one float4 per thread over the whole buffer; every region boundary is a multiple of 64 floats, so a group never straddles two
__global__ void __launch_bounds__(256) per_init_kernel(float4* __restrict__ tree, const PerTree t) {
  const long long i4 = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long i = 4 * i4;
  if (i >= t.total) return;
  float v = 0.f;
#pragma unroll
  for (int l = 0; l < PER_MAX_LEVELS; ++l)
    if (l < t.levels && i >= t.off[l] + t.pad[l] && i < t.off[l] + 2ll * t.pad[l]) v = INFINITY;
  tree[i4] = make_float4(i == 0 ? 1.f : v, v, v, v);
}

__global__ void __launch_bounds__(256) per_set_leaves_kernel(float* __restrict__ tree, long long off0, int pad0, long long first, long long count) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= count) return;
  const float v = tree[0];
  tree[off0 + first + k] = v;
  tree[off0 + pad0 + first + k] = v;
}

// leaf first + k <- leaves[k], clamped as per_max_kernel clamps (a NaN becomes the smallest leaf); its min word is its sum
__global__ void __launch_bounds__(256) per_write_leaves_kernel(float* __restrict__ tree, long long off0, int pad0, long long first, long long count,
                                                               const float* __restrict__ leaves) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= count) return;
  const float v = fminf(fmaxf(leaves[k], PER_LEAF_MIN), PER_LEAF_MAX);
  tree[off0 + first + k] = v;
  tree[off0 + pad0 + first + k] = v;
}

// One wave per parent of level `level` >= 1 (4 per workgroup): lane c reads child c, the wave reduces sum and min in the fixed order.
// idx == null: the parents lo .. lo + cnt - 1 (per_set_range).  Otherwise wave j rebuilds the ancestor of leaf idx[j] (per_update; an
// index outside [0, stored) is skipped) and, at level 1, stores that leaf's min word, which is its sum.
__global__ void __launch_bounds__(256) per_rebuild_kernel(float* __restrict__ tree, int level, long long coff, int cpad, long long poff, int ppad,
                                                          long long lo, long long cnt, const long long* __restrict__ idx, long long stored) {
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= cnt) return;       // wave-uniform
  long long p = lo + w, leaf = -1;
  if (idx) {
    leaf = idx[w];
    if (leaf < 0 || leaf >= stored) return;
    p = leaf >> (6 * level);
  }
  const long long c = 64 * p + lane;   // < cpad: p < ceil(n_child / 64)
  const float s = tree[coff + c];
  const float m = level == 1 ? (s > 0.f ? s : INFINITY) : tree[coff + cpad + c];
  if (level == 1 && c == leaf) tree[coff + cpad + c] = s;
  const float ps = wave_sum(s), pm = wave_min(m);
  if (lane == 0) {
    tree[poff + p] = ps;
    tree[poff + ppad + p] = pm;
  }
}

__device__ __forceinline__ bool per_valid(long long j, long long n, const long long* __restrict__ idx, long long stored, long long& i) {
  i = j < n ? idx[j] : -1;
  return i >= 0 && i < stored;
}

// pass 1 of an update: the addressed leaves to 0 (so that the largest NEW value wins pass 2, whatever the old one was), and the max leaf
// as it stands now into header word 1 for the non-finite priorities of pass 2
__global__ void __launch_bounds__(256) per_zero_kernel(float* __restrict__ tree, long long off0, const long long* __restrict__ idx, long long n,
                                                       long long stored) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j == 0) tree[1] = tree[0];
  long long i;
  if (per_valid(j, n, idx, stored, i)) tree[off0 + i] = 0.f;
}

// pass 2: integer max on the float bits (monotone for positive floats), one more per wave on the running max leaf
__global__ void __launch_bounds__(256) per_max_kernel(float* __restrict__ tree, long long off0, const long long* __restrict__ idx,
                                                      const float* __restrict__ prio, long long n, long long stored, float alpha, float eps) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  const float start_max = tree[1];
  long long i;
  const bool valid = per_valid(j, n, idx, stored, i);
  float v = 0.f;
  if (valid) {
    const float p = prio[j];
    if (isfinite(p)) {
      const float x = fabsf(p) + eps;
      v = alpha == 1.f ? x : powf(x, alpha);
      v = fminf(fmaxf(v, PER_LEAF_MIN), PER_LEAF_MAX);
    } else {
      v = start_max;
    }
    atomicMax(reinterpret_cast<int*>(tree + off0 + i), __float_as_int(v));
  }
  const float wm = wave_max(v);
  if ((threadIdx.x & 63) == 0 && wm > start_max) atomicMax(reinterpret_cast<int*>(tree), __float_as_int(wm));
}

// a one-level tree has no rebuild pass to store the leaves' min words
__global__ void __launch_bounds__(256) per_leaf_min_kernel(float* __restrict__ tree, long long off0, int pad0, const long long* __restrict__ idx,
                                                           long long n, long long stored) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  long long i;
  if (per_valid(j, n, idx, stored, i)) tree[off0 + pad0 + i] = tree[off0 + i];
}

// One wave per sample.  At each level lane c holds child c's sum and the wave an inclusive prefix (6 fixed __shfl_up steps); the chosen
// child is the first with child > 0 and prefix > residual, else (rounding between a parent and the prefix of its children, or u == 1) the
// last child with a nonzero sum.  Padding and unwritten slots have sum 0 and are never chosen; an all-zero tree gives index 0, weight 1.
__global__ void __launch_bounds__(256) per_sample_kernel(const float* __restrict__ tree, const PerTree t, const float* __restrict__ uniforms,
                                                         long long n, int stratified, float beta, long long* __restrict__ idx_out,
                                                         float* __restrict__ weights_out) {
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= n) return;       // wave-uniform
  const int top = t.levels - 1;
  long long toff = t.off[0];
#pragma unroll
  for (int l = 1; l < PER_MAX_LEVELS; ++l)
    if (l == top) toff = t.off[l];
  const float total = wave_sum(tree[toff + lane]);
  const float p_min = wave_min(tree[toff + 64 + lane]);   // the top block is 64 wide
  const float u = fminf(fmaxf(uniforms[w], 0.f), 1.f);    // (a NaN becomes 0)
  float mass = stratified ? ((float)w + u) / (float)n * total : u * total;
  long long b = 0;
  float leaf = 0.f;
  bool dead = false;
#pragma unroll
  for (int l = PER_MAX_LEVELS - 1; l >= 0; --l) {
    if (l > top || dead) continue;
    const float child = tree[t.off[l] + 64 * b + lane];   // 64 b + lane < pad_l: b is a node of level l + 1 (or 0 at the top)
    float pre = child;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float up = __shfl_up(pre, d, 64);
      if (lane >= d) pre += up;
    }
    const unsigned long long hit = __ballot(child > 0.f && pre > mass);
    const unsigned long long nonzero = __ballot(child > 0.f);
    if (nonzero == 0ull) {
      dead = true;
      continue;
    }
    const int c = hit ? __ffsll((long long)hit) - 1 : 63 - __clzll((long long)nonzero);
    const float before = __shfl(pre, c > 0 ? c - 1 : 0, 64);
    mass = fmaxf(mass - (c > 0 ? before : 0.f), 0.f);
    leaf = __shfl(child, c, 64);
    b = 64 * b + c;
  }
  if (lane == 0) {
    idx_out[w] = dead ? 0 : b;
    weights_out[w] = (dead || beta == 0.f) ? 1.f : powf(p_min / leaf, beta);
  }
}

inline unsigned blocks(long long items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

}  // namespace

long long per_tree_floats(long long capacity) {
  PerTree t;
  return per_layout(capacity, t) ? t.total : -1;
}

#define PER_CHECK_TREE(name)                                                                                                        \
  PerTree t;                                                                                                                        \
  DGVIT_CHECK_ARG(tree, name ": tree must not be null");                                                                            \
  DGVIT_CHECK_ARG(per_layout(capacity, t), name ": capacity=%lld must be in [1, 2^24]", capacity);                                  \
  DGVIT_CHECK_ARG(al16(tree), name ": tree must be 16-byte aligned")

int per_init(float* tree, long long capacity, hipStream_t stream) {
  PER_CHECK_TREE("per_init");
  {
    ProfileScope ps(PROF_OTHER, 0.0, stream);
    hipLaunchKernelGGL(per_init_kernel, dim3(blocks(t.total / 4, 256)), dim3(256), 0, stream, reinterpret_cast<float4*>(tree), t);
  }
  DGVIT_CHECK_LAUNCH("per_init");
  return DGVIT_OK;
}

// the ancestors of leaves [first, first + count): a contiguous range of leaves has a contiguous range of ancestors at every level
static void per_rebuild_range(float* tree, const PerTree& t, long long first, long long count, hipStream_t stream) {
  long long lo = first, hi = first + count - 1;
  for (int l = 1; l < t.levels; ++l) {
    lo >>= 6;
    hi >>= 6;
    hipLaunchKernelGGL(per_rebuild_kernel, dim3(blocks(hi - lo + 1, 4)), dim3(256), 0, stream, tree, l, t.off[l - 1], t.pad[l - 1], t.off[l],
                       t.pad[l], lo, hi - lo + 1, (const long long*)nullptr, 0ll);
  }
}

int per_set_range(float* tree, long long capacity, long long first, long long count, hipStream_t stream) {
  PER_CHECK_TREE("per_set_range");
  DGVIT_CHECK_ARG(first >= 0 && count >= 1 && first < capacity && count <= capacity - first,
                  "per_set_range: first=%lld count=%lld must be a non-empty range inside [0, capacity=%lld)", first, count, capacity);
  {
    ProfileScope ps(PROF_OTHER, 0.0, stream);
    hipLaunchKernelGGL(per_set_leaves_kernel, dim3(blocks(count, 256)), dim3(256), 0, stream, tree, t.off[0], t.pad[0], first, count);
    per_rebuild_range(tree, t, first, count, stream);
  }
  DGVIT_CHECK_LAUNCH("per_set_range");
  return DGVIT_OK;
}

int per_set_leaves(float* tree, long long capacity, long long first, long long count, const float* leaves, hipStream_t stream) {
  PER_CHECK_TREE("per_set_leaves");
  DGVIT_CHECK_ARG(leaves, "per_set_leaves: leaves must not be null");
  DGVIT_CHECK_ARG(first >= 0 && count >= 1 && first < capacity && count <= capacity - first,
                  "per_set_leaves: first=%lld count=%lld must be a non-empty range inside [0, capacity=%lld)", first, count, capacity);
  DGVIT_CHECK_ARG((reinterpret_cast<uintptr_t>(leaves) & 3) == 0, "per_set_leaves: leaves must be 4-byte aligned");
  {
    ProfileScope ps(PROF_OTHER, 0.0, stream);
    hipLaunchKernelGGL(per_write_leaves_kernel, dim3(blocks(count, 256)), dim3(256), 0, stream, tree, t.off[0], t.pad[0], first, count, leaves);
    per_rebuild_range(tree, t, first, count, stream);
  }
  DGVIT_CHECK_LAUNCH("per_set_leaves");
  return DGVIT_OK;
}

int per_update(float* tree, long long capacity, long long stored, const long long* idx, const float* prio, long long n, float alpha, float eps,
               hipStream_t stream) {
  PER_CHECK_TREE("per_update");
  DGVIT_CHECK_ARG(idx && prio, "per_update: idx and prio must not be null");
  DGVIT_CHECK_ARG(stored >= 0 && stored <= capacity, "per_update: stored=%lld must be in [0, capacity=%lld]", stored, capacity);
  DGVIT_CHECK_ARG(n >= 1 && n < (1ll << 24), "per_update: n=%lld must be in [1, 2^24)", n);
  DGVIT_CHECK_ARG(alpha >= 0.f && alpha <= 1.f, "per_update: alpha=%g must be in [0, 1]", (double)alpha);
  DGVIT_CHECK_ARG(eps >= 0.f && std::isfinite(eps), "per_update: eps=%g must be finite and not negative", (double)eps);
  {
    ProfileScope ps(PROF_OTHER, 0.0, stream);
    hipLaunchKernelGGL(per_zero_kernel, dim3(blocks(n, 256)), dim3(256), 0, stream, tree, t.off[0], idx, n, stored);
    hipLaunchKernelGGL(per_max_kernel, dim3(blocks(n, 256)), dim3(256), 0, stream, tree, t.off[0], idx, prio, n, stored, alpha, eps);
    if (t.levels == 1)
      hipLaunchKernelGGL(per_leaf_min_kernel, dim3(blocks(n, 256)), dim3(256), 0, stream, tree, t.off[0], t.pad[0], idx, n, stored);
    for (int l = 1; l < t.levels; ++l)
      hipLaunchKernelGGL(per_rebuild_kernel, dim3(blocks(n, 4)), dim3(256), 0, stream, tree, l, t.off[l - 1], t.pad[l - 1], t.off[l], t.pad[l],
                         0ll, n, idx, stored);
  }
  DGVIT_CHECK_LAUNCH("per_update");
  return DGVIT_OK;
}

int per_sample(const float* tree, long long capacity, const float* uniforms, long long n, int stratified, float beta, long long* idx_out,
               float* weights_out, hipStream_t stream) {
  PER_CHECK_TREE("per_sample");
  DGVIT_CHECK_ARG(uniforms && idx_out && weights_out, "per_sample: uniforms, idx_out and weights_out must not be null");
  DGVIT_CHECK_ARG(n >= 1 && n < (1ll << 24), "per_sample: n=%lld must be in [1, 2^24)", n);
  DGVIT_CHECK_ARG(stratified == 0 || stratified == 1, "per_sample: stratified=%d must be 0 or 1", stratified);
  DGVIT_CHECK_ARG(beta >= 0.f && beta <= 1.f, "per_sample: beta=%g must be in [0, 1]", (double)beta);
  {
    ProfileScope ps(PROF_OTHER, 0.0, stream);
    hipLaunchKernelGGL(per_sample_kernel, dim3(blocks(n, 4)), dim3(256), 0, stream, tree, t, uniforms, n, stratified, beta, idx_out, weights_out);
  }
  DGVIT_CHECK_LAUNCH("per_sample");
  return DGVIT_OK;
}
