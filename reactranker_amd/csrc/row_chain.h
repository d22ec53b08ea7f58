// The shared header of the row-streaming embedding kernels (csrc/kcenter.hip, csrc/cluster.hip, csrc/moments.hip, csrc/knn.hip;
// DESIGN sections 4g, 4h, 4j and 4k).  The one copy of
//   the row load (rr_load4) and the finite rule (rr_finite, kc_row_finite, kc_row_finite_any);
//   the difference chain of kcenter and cluster:
//     d(i, c) = sum_h (x[i,h] - x[c,h])^2 in f32: columns in groups of four, lane l of the wave owns the groups g with g % 64 == l
//     (ascending, columns inside a group ascending), acc = acc + t * t with t = x[i,h] - x[c,h], the 64 chains joined by the
//     butterfly xor 32, 16, 8, 4, 2, 1.  tests/selection_ref.py (chain32) restates it in numpy;
//   the round scaffold of those two (RowPair, rc_join_waves, rc_block_best, rc_pad_kernel) and its host shell (rc_grid,
//   rc_dispatch).  The blocks knob (BlocksKnob) is wave_util.h's, next to WaveKnob.
// NG = groups a lane owns (1 .. 4: H <= 1024, a row in 4 NG registers); the *_any forms are the loop for wider rows, which read
// both rows group by group.  VEC: 16-byte loads (pointer 16-byte aligned and ld % 4 == 0), else 4-byte loads - the same values
// either way.
#pragma once
#include <type_traits>

#include "wave_util.h"

constexpr int RC_NT = 256;                        // threads of a pass kernel (4 waves: 4 rows per workgroup and grid pass)
constexpr int RC_WAVES = RC_NT / 64;
constexpr int RC_MAX_BLOCKS = 4096;
constexpr int RC_MAX_NG = 4;                      // register path up to H = 256 * RC_MAX_NG
constexpr int RC_AUTO_BLOCKS = RR_NUM_CU * 4;     // 16 waves per CU: measured best or within 4 % of it from P = 10^4 to 10^6

typedef const __attribute__((address_space(1))) f32x4* rr_gptr4;

// columns c .. c + 3 of a row (c % 4 == 0), every load unconditional: the address of a column at or past `width` is clamped to a
// valid one; what such an element holds is unspecified and is masked where it is used
template <bool VEC>
__device__ __forceinline__ f32x4 rr_load4(const float* row, int c, int width) {
  f32x4 v;
  if (VEC) {
    v = *(rr_gptr4)(row + (c < width ? c : 0));   // (VEC: ld % 4 == 0, so the group lies inside the row's pitch)
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = row[c + e < width ? c + e : 0];
  }
  return v;
}

template <int NG, bool VEC>
__device__ __forceinline__ void kc_load_row(const float* row, int lane, int H, f32x4 (&v)[NG]) {
#pragma unroll
  for (int j = 0; j < NG; ++j) {
    const int c = 4 * (lane + 64 * j);
    v[j] = c < H ? rr_load4<VEC>(row, c, H) : f32x4(0.f);
  }
}

__device__ __forceinline__ float kc_step(float acc, float a, float b, bool on) {
  float t = a - b;
  t = on ? t : 0.f;                               // (acc >= 0, so acc + 0 is acc: a masked column is a skipped one)
  return acc + t * t;
}

template <int NG>
__device__ __forceinline__ float kc_dist(const f32x4 (&a)[NG], const f32x4 (&b)[NG], int lane, int H) {
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < NG; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = kc_step(acc, a[j][e], b[j][e], 4 * (lane + 64 * j) + e < H);
  return rr_wave_sum(acc);
}

// any width: the same chain with both rows read group by group
template <bool VEC>
__device__ __forceinline__ float kc_dist_any(const float* row, const float* centre, int lane, int H) {
  float acc = 0.f;
  for (int g0 = 0; 4 * g0 < H; g0 += 64) {        // (uniform)
    const int c = 4 * (g0 + lane);
    if (c < H) {
      const f32x4 a = rr_load4<VEC>(row, c, H), b = rr_load4<VEC>(centre, c, H);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = kc_step(acc, a[e], b[e], c + e < H);
    }
  }
  return rr_wave_sum(acc);
}

// THE finite rule of the embedding ops: neither a NaN nor an infinity
__device__ __forceinline__ bool rr_finite(float v) { return fabsf(v) < __builtin_inff(); }

template <int NG>
__device__ __forceinline__ bool kc_row_finite(const f32x4 (&a)[NG], int lane, int H) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < NG; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) ok = ok && (4 * (lane + 64 * j) + e >= H || rr_finite(a[j][e]));
  return __all(ok);
}

template <bool VEC>
__device__ __forceinline__ bool kc_row_finite_any(const float* row, int lane, int H) {
  bool ok = true;
  for (int g0 = 0; 4 * g0 < H; g0 += 64) {
    const int c = 4 * (g0 + lane);
    if (c < H) {
      const f32x4 a = rr_load4<VEC>(row, c, H);
#pragma unroll
      for (int e = 0; e < 4; ++e) ok = ok && (c + e >= H || rr_finite(a[e]));
    }
  }
  return __all(ok);
}

// ---- the round scaffold: a pass kernel leaves one (key, index) pair per workgroup, the next launch reduces them to the winner
template <typename K>
struct __attribute__((aligned(8))) RowPair { K k; int32_t i; };   // i < 0: no candidate

// The join of the four waves' (bk, bi) (each wave-uniform) through LDS, valid in every thread: the last step of the reduction
// of the previous launch's pairs to the winner.  All RC_NT threads call; `s_w` is touched by nobody else; one barrier.  `wave`
// is the caller's readfirstlane(threadIdx.x >> 6), here and below: formed again inside, it costs kc_pass_kernel<0, true> two
// SGPRs.  The scan in front of it stays in the two kernels, see there.
template <typename K>
__device__ __forceinline__ void rc_join_waves(K& bk, int& bi, int wave, RowPair<K> (&s_w)[RC_WAVES]) {
  if ((threadIdx.x & 63) == 0) { s_w[wave].k = bk; s_w[wave].i = bi; }
  __syncthreads();
  bk = s_w[0].k; bi = s_w[0].i;
#pragma unroll
  for (int w = 1; w < RC_WAVES; ++w)
    if (rr_first_max_replaces(s_w[w].k, s_w[w].i, bk, bi)) { bk = s_w[w].k; bi = s_w[w].i; }
}

// The workgroup's best pair from the four waves' (bk, bi) (each wave-uniform): thread 0 hands it to put(key, index), which says
// where it goes.  All RC_NT threads call; one barrier.
template <typename K, class Put>
__device__ __forceinline__ void rc_block_best(K bk, int bi, int wave, RowPair<K> (&s_w)[RC_WAVES], Put put) {
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) { s_w[wave].k = bk; s_w[wave].i = bi; }
  __syncthreads();
  if (tid == 0) {
    bk = s_w[0].k; bi = s_w[0].i;
#pragma unroll
    for (int w = 1; w < RC_WAVES; ++w)
      if (rr_first_max_replaces(s_w[w].k, s_w[w].i, bk, bi)) { bk = s_w[w].k; bi = s_w[w].i; }
    put(bk, bi);
  }
}

// an empty pool: every slot of the picks / centres (and of the gain, where there is one) is padding
template <bool GAIN>
__global__ void __launch_bounds__(RC_NT) rc_pad_kernel(int32_t* idx, float* gain, int n) {
  for (int k = blockIdx.x * RC_NT + threadIdx.x; k < n; k += gridDim.x * RC_NT) {
    idx[k] = -1;
    if (GAIN) gain[k] = -1.0f;
  }
}

// ---- the host shell
// workgroups of a pass over P rows; automatic: two rows per wave and launch at least, 16 waves per CU at most
inline int rc_grid(int blocks, int64_t P) {            // blocks: the entry's BlocksKnob value
  int64_t b = blocks;
  if (b == 0) {
    b = (P + 2 * RC_WAVES - 1) / (2 * RC_WAVES);
    if (b > RC_AUTO_BLOCKS) b = RC_AUTO_BLOCKS;
    if (b < 1) b = 1;
  }
  return static_cast<int>(b);
}

// f(std::bool_constant<VEC>) for a run-time `vec`
template <class F>
inline void rr_vec_dispatch(bool vec, F f) {
  if (vec) f(std::true_type{});
  else f(std::false_type{});
}

// (H, pointer, ld) -> the NG and VEC template arguments: f(std::integral_constant<int, NG>, std::bool_constant<VEC>)
template <class F>
inline void rc_dispatch(int H, const float* x, int64_t ld, F f) {
  const int ng = ((H + 3) / 4 + 63) / 64;
  rr_vec_dispatch(rr_vec4_ok(x, ld), [&](auto vec) {
    switch (ng <= RC_MAX_NG ? ng : 0) {
      case 1: f(std::integral_constant<int, 1>{}, vec); break;
      case 2: f(std::integral_constant<int, 2>{}, vec); break;
      case 3: f(std::integral_constant<int, 3>{}, vec); break;
      case 4: f(std::integral_constant<int, 4>{}, vec); break;
      default: f(std::integral_constant<int, 0>{}, vec); break;
    }
  });
}
