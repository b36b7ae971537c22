// The host side of a kernel launch, in one place: error propagation, the per-device one-time state (dynamic-LDS opt-in, CU count) and
// the live-profile bracket.  The launches themselves (hipLaunchKernelGGL) stay in the launchers, readable where they are.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

#include "../../include/dgvit_hip.h"

int dgvit_set_error(int code, const char* fmt, ...);   // thread-local message, returns `code` (api.hip)

#define TRY(expr)          \
  do {                     \
    int rc_ = (expr);      \
    if (rc_) return rc_;   \
  } while (0)

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) return dgvit_set_error(DGVIT_ERR_HIP, #expr ": %s", hipGetErrorString(e_)); \
  } while (0)

// Kernel attributes (the dynamic-LDS limit above 64 KB) are per DEVICE: a flag per device ordinal, set on the first launch on
// that device (a process-wide `static bool` would leave a second GPU of a single-process host without the attribute).
// Racing threads may both set the attribute: harmless, it is idempotent.
struct DeviceOnce {
  std::atomic<unsigned long long> done{0};
  unsigned long long pending() const {    // 0: already done on the current device, else the device's bit for mark()
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const unsigned long long bit = 1ull << (dev & 63);
    return (done.load(std::memory_order_relaxed) & bit) ? 0ull : bit;
  }
  void mark(unsigned long long bit) { done.fetch_or(bit, std::memory_order_relaxed); }
};

// Raise the dynamic-LDS limit of every kernel named, once per device (one DeviceOnce per instantiation, i.e. per kernel group).
//   * `bytes` is the most any launch of these kernels will ever ask for, never the current call's size: the attribute is set once.
//   * kernels that one launcher chooses between are named in ONE call, so that whichever variant runs first (the warm-up before a
//     graph capture) raises them all: hipFuncSetAttribute is not a stream operation and must not first happen inside a capture.
template <auto... Kerns>
int allow_dynamic_lds(int bytes, const char* what) {
  static DeviceOnce once;
  if (const unsigned long long bit = once.pending()) {
    for (const void* k : {reinterpret_cast<const void*>(Kerns)...}) {
      const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
      if (e != hipSuccess)
        return dgvit_set_error(DGVIT_ERR_HIP, "%s: cannot raise the dynamic LDS limit to %d bytes: %s", what, bytes, hipGetErrorString(e));
    }
    once.mark(bit);
  }
  return DGVIT_OK;
}

// Compute units of the current device (the grid of a persistent kernel), queried once per device ordinal.  A failed query gives 256
// and is not cached: the next call asks again.  Racing threads may both query: they store the same value.
inline int device_cus() {
  static std::atomic<int> cus[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  std::atomic<int>& slot = cus[dev & 63];
  int n = slot.load(std::memory_order_relaxed);
  if (n == 0) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess || prop.multiProcessorCount <= 0) return 256;
    n = prop.multiProcessorCount;
    slot.store(n, std::memory_order_relaxed);
  }
  return n;
}

// live timing hooks (profile.hip); slot < 0 = not recording
int profile_begin(int kind, double work, hipStream_t st);
void profile_end(int slot, hipStream_t st);
enum { PROF_GEMM = 0, PROF_ATTN_FWD = 1, PROF_ATTN_BWD = 2, PROF_OTHER = 3 };

// The bracket around the launches of one profiled operation: opened after the argument checks and the LDS opt-in, closed (end of its
// block) before DGVIT_CHECK_LAUNCH.  A begun slot always gets its end event, whatever path leaves the block.  on = false: no bracket.
class ProfileScope {
 public:
  ProfileScope(int kind, double work, hipStream_t st, bool on = true) : slot_(on ? profile_begin(kind, work, st) : -1), st_(st) {}
  ~ProfileScope() { profile_end(slot_, st_); }
  ProfileScope(const ProfileScope&) = delete;
  ProfileScope& operator=(const ProfileScope&) = delete;

 private:
  const int slot_;
  const hipStream_t st_;
};
