// Helpers of the one-wavefront-per-list kernels (loss.hip, task_loss.hip, pairwise.hip, uq.hip): the list-length cap,
// wave-level synchronisation, the f64 wave sum, and the host-side dynamic-LDS opt-in and argument check.  Everything lives
// in an unnamed namespace: each translation unit gets its own copy.
#pragma once
#include "rr_common.h"

namespace {

constexpr int kMaxLen = 8192;
static_assert(kMaxLen <= 65536, "ranking_metrics_kernel keeps list positions in 16 bits");

__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ inline double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <typename Kern>
int set_lds(Kern k, size_t bytes) {
  if (bytes > 65536) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                            static_cast<int>(bytes)) != hipSuccess)
      return RR_ERR_LAUNCH;
  }
  return RR_OK;
}

inline bool list_args_ok(const void* a, const void* t, const int32_t* seg, int Q, int max_len) {
  return a && t && seg && Q >= 0 && max_len >= 0;
}

}  // namespace
