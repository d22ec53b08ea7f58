// Helpers of the per-list kernels - one wavefront per list (loss.hip, task_loss.hip, pairwise.hip, lambdarank.hip, uq.hip) or one
// workgroup of one or four (approx_ndcg.hip, rank_corr.hip, calibration.hip): the list-length cap, wave-level synchronisation,
// the plain staging of a list (stage_list) and the fixed-order sum of a 256-thread workgroup (block_sum), which every
// partial-producing and finishing kernel of loss.hip and pairwise.hip goes through;
// on the host side the dynamic-LDS opt-in, the argument check, the words per staged array (list_words, list_words4), the wave
// knob of the one-or-four-wave kernels (WaveKnob), the blocks knob of the grid-strided embedding kernels (BlocksKnob) and the
// one launch of a "one workgroup per query" kernel (launch_per_query, launch_per_query_bytes, launch_list, launch_waves).
// The wave reductions and the ordering rule are in rr_common.h.  Everything lives in an unnamed namespace: each translation
// unit gets its own copy.
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

// The fixed-order sum of a 256-thread workgroup, one value per thread and row: v[r] goes through shared memory as
// red[t] += red[t + o] for o = 128, 64, ..., 1 with a barrier after each step, and comes back as the sum in thread 0 alone.
// This order is a contract: fixed_sum (loss_list.h) replays it on one wave and the tests assert its bits, so it is not to be
// replaced by wave shuffles.  Every thread of the workgroup must call it; rows are summed side by side in one tree.
template <typename T, int ROWS>
__device__ inline void block_sum(T (&v)[ROWS]) {
  __shared__ T red[ROWS][256];
  const int t = threadIdx.x;
#pragma unroll
  for (int r = 0; r < ROWS; ++r) red[r][t] = v[r];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int r = 0; r < ROWS; ++r) red[r][t] += red[r][t + o];
    }
    __syncthreads();
  }
  if (t == 0) {
#pragma unroll
    for (int r = 0; r < ROWS; ++r) v[r] = red[r][0];
  }
}

template <typename T>
__device__ inline T block_sum(T v) {
  T a[1] = {v};
  block_sum(a);
  return a[0];
}

// stages a query's strided score column and its targets into LDS as they are
__device__ inline void stage_list(float* s, float* t, const float* __restrict__ score, int64_t sstride,
                                  const float* __restrict__ targets, int off, int C, int lane) {
  for (int i = lane; i < C; i += RR_WAVE) {
    s[i] = score[static_cast<int64_t>(off + i) * sstride];
    t[i] = targets[off + i];
  }
  wave_sync();
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

// the same rounded up to whole float4s, for the kernels that walk a list four candidates at a time (16-byte LDS reads)
inline int list_words4(int max_len) { return max_len > 4 ? (max_len + 3) & ~3 : 4; }

// The wave count of a kernel that gives a query one wavefront while the window's longest list has at most 64 candidates and
// four above: 0 = by max_len, 1 or 4 = pinned.  One instance per entry-point family, a plain process-wide word that every
// launch reads: set() is for the bench tools and the tests, and is not safe against launches or setters on other threads.
struct WaveKnob {
  int waves = 0;
  int set(int w) {
    RR_CHECK_ARG(w == 0 || w == 1 || w == 4);
    waves = w;
    return RR_OK;
  }
  int pick(int max_len) const { return waves != 0 ? waves : (max_len <= RR_WAVE ? 1 : 4); }
};

// The workgroup count of a grid-strided entry-point family (kcenter, cluster, moments, resample): 0 = automatic by the file's own
// grid rule, else pinned.  A process-wide word that every launch reads (relaxed); set() is for the bench tools and the tests.
struct BlocksKnob {
  std::atomic<int> blocks{0};
  int get() const { return blocks.load(std::memory_order_relaxed); }
  int set(int b, int max) {
    RR_CHECK_ARG(b >= 0 && b <= max);
    blocks.store(b, std::memory_order_relaxed);
    return RR_OK;
  }
};

// The launch of a "one workgroup per query" kernel: Q workgroups of `threads` threads, each with `lds` bytes of dynamic LDS.
// Q == 0 launches nothing and is no error.
template <typename Kern, typename... Args>
int launch_per_query_bytes(Kern kern, int Q, size_t lds, int threads, hipStream_t s, Args... args) {
  if (Q == 0) return RR_OK;
  if (set_lds(kern, lds) != RR_OK) return RR_ERR_LAUNCH;
  kern<<<Q, threads, lds, s>>>(args...);
  return rr_launch_status();
}

// The same with L * bytes_per_cand bytes.  L is the kernel's words per staged array - list_words(max_len) unless the kernel
// pads its arrays - and the caller passes it among `args` as well, wherever the kernel takes it.
template <typename Kern, typename... Args>
int launch_per_query(Kern kern, int Q, int L, size_t bytes_per_cand, int threads, hipStream_t s, Args... args) {
  return launch_per_query_bytes(kern, Q, static_cast<size_t>(L) * bytes_per_cand, threads, s, args...);
}

// The host body of a one-wave kernel that takes (score, sstride, targets, seg_off, L, rest...): the list-length cap, the words
// per staged array and the launch
template <typename Kern, typename... Rest>
int launch_list(Kern kern, size_t bytes_per_cand, const float* score, int64_t sstride, const float* targets,
                const int32_t* seg_off, int Q, int max_len, hipStream_t s, Rest... rest) {
  if (max_len > kMaxLen) return RR_ERR_UNSUPPORTED;
  const int L = list_words(max_len);
  return launch_per_query(kern, Q, L, bytes_per_cand, RR_WAVE, s, score, sstride, targets, seg_off, L, rest...);
}

// The one-wave or the four-wave instantiation of a kernel, `waves` (1 or 4) wavefronts per query
template <typename Kern, typename... Args>
int launch_waves(Kern kern1, Kern kern4, int waves, int Q, size_t lds, hipStream_t s, Args... args) {
  return launch_per_query_bytes(waves == 1 ? kern1 : kern4, Q, lds, waves * RR_WAVE, s, args...);
}

}  // namespace
