// The sorted list of the searches (csrc/knn.hip; csrc/tanimoto.hip, section 4l), the one copy of it: the k
// best (distance, index) pairs of a query row under the total order (d ascending, then n ascending), one slot per lane of a
// wavefront, and the kernels that merge the per-split partial results of a row.  The order is total (n is unique), so a list does
// not depend on the order in which candidates were offered: the same bits for every split count, no atomics.
// Everything lives in an unnamed namespace: each translation unit gets its own copy.
#pragma once
#include "rr_common.h"

namespace {

constexpr int KN_NT = 256;                        // threads of a search kernel and of the merge kernels (4 waves)
constexpr int KN_PAD = 0x7fffffff;                // index of an empty slot inside the kernels (N <= 2^31 - 1: above every row)

__device__ __forceinline__ bool kn_less(float d1, int i1, float d2, int i2) { return d1 < d2 || (d1 == d2 && i1 < i2); }
__device__ __forceinline__ float kn_lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ int kn_lane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }

// the sorted list (ld, li), one slot per lane: candidate (d, n) takes its place, everything behind it moves one lane up
__device__ __forceinline__ void kn_insert(float& ld, int& li, float d, int n, int lane) {
  const bool mine_less = kn_less(ld, li, d, n);
  const float ud = __shfl_up(ld, 1, 64);
  const int ui = __shfl_up(li, 1, 64);
  const bool up_less = lane == 0 || kn_less(ud, ui, d, n);
  if (!mine_less) {
    ld = up_less ? d : ud;
    li = up_less ? n : ui;
  }
}

// one candidate per lane: those below the list's slot km1 are inserted, lowest lane first (all 64 lanes active)
__device__ __forceinline__ void kn_offer(float& ld, int& li, float d, int n, bool valid, int km1, int lane) {
  float td = kn_lane_f(ld, km1);
  int ti = kn_lane_i(li, km1);
  uint64_t mask = __ballot(valid && kn_less(d, n, td, ti));
  while (mask != 0) {                             // (uniform)
    const int src = __builtin_amdgcn_readfirstlane(__builtin_ctzll(mask));
    mask &= mask - 1;
    const float cd = kn_lane_f(d, src);
    const int cn = kn_lane_i(n, src);
    if (kn_less(cd, cn, td, ti)) {
      kn_insert(ld, li, cd, cn, lane);
      td = kn_lane_f(ld, km1);
      ti = kn_lane_i(li, km1);
    }
  }
}

// one thread per row: the S partial counts of a row, in split order (S == 0: zeros)
__global__ void __launch_bounds__(KN_NT) knn_count_merge_kernel(const int32_t* part, int64_t M, int S, int32_t* out) {
  const int64_t m = static_cast<int64_t>(blockIdx.x) * KN_NT + threadIdx.x;
  if (m >= M) return;
  int c = 0;
  for (int s = 0; s < S; ++s) c += part[m * S + s];
  out[m] = c;
}

// one wave per row: the S partial lists of a row -> the row's result (S == 0: all padding)
__global__ void __launch_bounds__(KN_NT) knn_merge_kernel(const float* part_d, const int32_t* part_i, int64_t M, int S, int k,
                                                          float* out_d, int32_t* out_i) {
  const int lane = threadIdx.x & 63;
  const int64_t m = static_cast<int64_t>(blockIdx.x) * (KN_NT / 64) + (threadIdx.x >> 6);
  if (m >= M) return;                             // (uniform per wave)
  float ld = __builtin_inff();
  int li = KN_PAD;
  for (int s = 0; s < S; ++s) {
    const int64_t o = (m * S + s) * k + (lane < k ? lane : 0);
    const float d = part_d[o];
    const int n = part_i[o];
    kn_offer(ld, li, d, n, lane < k && n != KN_PAD, k - 1, lane);
  }
  if (lane < k) {
    out_d[m * k + lane] = ld;
    out_i[m * k + lane] = li == KN_PAD ? -1 : li;
  }
}

}  // namespace
