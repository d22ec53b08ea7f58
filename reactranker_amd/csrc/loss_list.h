// Per-list device code shared by the loss translation units (loss.hip, task_loss.hip): one 64-lane wavefront owns one list
// staged in LDS; only wave-level synchronisation.  Everything lives in an unnamed namespace: each translation unit
// gets its own copy, and moving the code here changed no operation or order (the losses keep their bits).
#pragma once
#include "rr_common.h"

namespace {

constexpr int kMaxLen = 8192;
static_assert(kMaxLen <= 65536, "ranking_metrics_kernel keeps list positions in 16 bits");

__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

struct ListView {
  float* s;       // scores (as given)
  float* t;       // targets
  float* ss;      // scores sorted by target, descending
  int32_t* perm;  // perm[j] = original position of sorted element j
  float* aux;     // scratch (fd values)
};

__device__ inline ListView carve(float* sm, int L) {
  ListView v;
  v.s = sm;
  v.t = sm + L;
  v.ss = sm + 2 * L;
  v.perm = reinterpret_cast<int32_t*>(sm + 3 * L);
  v.aux = sm + 4 * L;
  return v;
}

// rank by target, descending, ties by original index (stable); scatters s into ss / perm.
__device__ inline void rank_sort(const ListView& v, int C, int lane) {
  for (int i = lane; i < C; i += RR_WAVE) {
    const float ti = v.t[i];
    int r = 0;
    for (int j = 0; j < C; ++j) {
      const float tj = v.t[j];
      r += (tj > ti || (tj == ti && j < i)) ? 1 : 0;
    }
    v.ss[r] = v.s[i];
    v.perm[r] = i;
  }
  wave_sync();
}

__device__ inline float list_max(const float* a, int C, int lane) {
  float m = -INFINITY;
  for (int i = lane; i < C; i += RR_WAVE) m = fmaxf(m, a[i]);
  return rr_wave_max(m);
}

// fd[j] = log(sum_{i>=j} exp(x[i] - m)) + m for the C values in x (LogCumsumExp.forward,
// train/loss.py:28-34).  Each lane owns the contiguous chunk [lo, hi).
__device__ inline void logcumsumexp_rev(const float* x, float* fd, int C, int lane, float m) {
  const int E = (C + RR_WAVE - 1) / RR_WAVE;
  const int lo = min(lane * E, C), hi = min(lo + E, C);
  float local = 0.f;
  for (int j = hi - 1; j >= lo; --j) local += expf(x[j] - m);
  // suffix sums over lanes without subtraction: scan the lane-reversed values
  const float rev = __shfl(local, RR_WAVE - 1 - lane, RR_WAVE);
  const float incl_rev = rr_wave_incl_scan(rev, lane);
  const float suffix_incl = __shfl(incl_rev, RR_WAVE - 1 - lane, RR_WAVE);   // sum over lanes >= lane
  const float nxt = __shfl_down(suffix_incl, 1, RR_WAVE);
  float run = (lane == RR_WAVE - 1) ? 0.f : nxt;                             // sum over lanes > lane, no subtraction
  for (int j = hi - 1; j >= lo; --j) {
    run += expf(x[j] - m);
    fd[j] = logf(run) + m;
  }
  wave_sync();
}

// cs[j] = sum_{i<=j} v(i), v(i) = exp(-fd[i]); returned through out[] (may alias nothing else).
__device__ inline void cumsum_exp_neg(const float* fd, float* out, int C, int lane) {
  const int E = (C + RR_WAVE - 1) / RR_WAVE;
  const int lo = min(lane * E, C), hi = min(lo + E, C);
  float local = 0.f;
  for (int j = lo; j < hi; ++j) local += expf(-fd[j]);
  const float incl = rr_wave_incl_scan(local, lane);
  const float prev = __shfl_up(incl, 1, RR_WAVE);
  float run = lane == 0 ? 0.f : prev;
  for (int j = lo; j < hi; ++j) {
    run += expf(-fd[j]);
    out[j] = run;
  }
  wave_sync();
}

// ---------------------------------------------------------------- softmax helpers
__device__ inline void softmax_stats(const float* a, int C, int lane, float* mx, float* sum) {
  const float m = list_max(a, C, lane);
  float s = 0.f;
  for (int i = lane; i < C; i += RR_WAVE) s += expf(a[i] - m);
  *mx = m;
  *sum = rr_wave_sum(s);
}

__device__ inline float sgnf(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }   // torch.abs' gradient

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
