// The difference chain of the row-streaming kernels (csrc/kcenter.hip, csrc/cluster.hip; DESIGN sections 4h and 4k), the one
// copy of it:
//   d(i, c) = sum_h (x[i,h] - x[c,h])^2 in f32: columns in groups of four, lane l of the wave owns the groups g with g % 64 == l
//   (ascending, columns inside a group ascending), acc = acc + t * t with t = x[i,h] - x[c,h], the 64 chains joined by the
//   butterfly xor 32, 16, 8, 4, 2, 1.
// and the row loads that feed it.  NG = groups a lane owns (1 .. 4: H <= 1024, a row in 4 NG registers); the *_any forms are the
// loop for wider rows, which read both rows group by group.  VEC: 16-byte loads (pointer 16-byte aligned and ld % 4 == 0), else
// 4-byte loads - the same values either way.  tests/selection_ref.py (chain32) restates the chain in numpy.
#pragma once
#include "rr_common.h"

typedef const __attribute__((address_space(1))) f32x4* kc_gptr4;

// columns c .. c + 3 of a row (c % 4 == 0, c < H); elements at or past H hold anything and are masked where they are used
template <bool VEC>
__device__ __forceinline__ f32x4 kc_load4(const float* row, int c, int H) {
  f32x4 v;
  if (VEC) {
    v = *(kc_gptr4)(row + c);                     // (VEC: ld % 4 == 0, so the group lies inside the row's pitch)
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = row[c + e < H ? c + e : c];
  }
  return v;
}

template <int NG, bool VEC>
__device__ __forceinline__ void kc_load_row(const float* row, int lane, int H, f32x4 (&v)[NG]) {
#pragma unroll
  for (int j = 0; j < NG; ++j) {
    const int c = 4 * (lane + 64 * j);
    v[j] = c < H ? kc_load4<VEC>(row, c, H) : f32x4(0.f);
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
      const f32x4 a = kc_load4<VEC>(row, c, H), b = kc_load4<VEC>(centre, c, H);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = kc_step(acc, a[e], b[e], c + e < H);
    }
  }
  return rr_wave_sum(acc);
}

__device__ __forceinline__ bool kc_finite(float v) { return fabsf(v) < __builtin_inff(); }

template <int NG>
__device__ __forceinline__ bool kc_row_finite(const f32x4 (&a)[NG], int lane, int H) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < NG; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) ok = ok && (4 * (lane + 64 * j) + e >= H || kc_finite(a[j][e]));
  return __all(ok);
}

template <bool VEC>
__device__ __forceinline__ bool kc_row_finite_any(const float* row, int lane, int H) {
  bool ok = true;
  for (int g0 = 0; 4 * g0 < H; g0 += 64) {
    const int c = 4 * (g0 + lane);
    if (c < H) {
      const f32x4 a = kc_load4<VEC>(row, c, H);
#pragma unroll
      for (int e = 0; e < 4; ++e) ok = ok && (c + e >= H || kc_finite(a[e]));
    }
  }
  return __all(ok);
}
