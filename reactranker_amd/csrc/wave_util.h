// Helpers of the one-wavefront-per-list kernels (loss.hip, task_loss.hip, pairwise.hip, uq.hip): the list-length cap,
// wave-level synchronisation, the f64 wave sum, and on the host side the dynamic-LDS opt-in, the argument check and the one
// launch of a "one workgroup per query" kernel (launch_per_query).  Everything lives in an unnamed namespace: each
// translation unit gets its own copy.
#pragma once
#include <atomic>

#include "rr_common.h"

// How many launches have opted in to more than 64 KiB of dynamic LDS (set_lds below); defined in loss.hip and read by
// rr_lds_opt_ins().  The HIP runtime of today launches such a kernel without the opt-in as well, so a kernel or a template
// instantiation that misses it computes the same numbers: this count is the one place where the tests can see it.
extern __attribute__((visibility("hidden"))) std::atomic<long long> rr_lds_opt_in_count;   // not an export

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
    rr_lds_opt_in_count.fetch_add(1, std::memory_order_relaxed);
  }
  return RR_OK;
}

inline bool list_args_ok(const void* a, const void* t, const int32_t* seg, int Q, int max_len) {
  return a && t && seg && Q >= 0 && max_len >= 0;
}

// words per staged array of a window whose longest list has max_len candidates (a window of empty lists still gets one)
inline int list_words(int max_len) { return max_len > 0 ? max_len : 1; }

// The launch of a "one workgroup per query" kernel: Q workgroups of `threads` threads, each with L * bytes_per_cand bytes of
// dynamic LDS.  L is the kernel's words per staged array - list_words(max_len) unless the kernel pads its arrays - and the
// caller passes it among `args` as well, wherever the kernel takes it.  Q == 0 launches nothing and is no error.
template <typename Kern, typename... Args>
int launch_per_query(Kern kern, int Q, int L, size_t bytes_per_cand, int threads, hipStream_t s, Args... args) {
  if (Q == 0) return RR_OK;
  const size_t lds = static_cast<size_t>(L) * bytes_per_cand;
  if (set_lds(kern, lds) != RR_OK) return RR_ERR_LAUNCH;
  kern<<<Q, threads, lds, s>>>(args...);
  return rr_launch_status();
}

}  // namespace
