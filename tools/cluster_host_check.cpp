// Host side of the radius-count and sphere-exclusion entry points under the host sanitizers: the argument checks, the split and
// blocks settings and the workspace sizing of csrc/knn.hip (rr_radius_count_*) and csrc/cluster.hip over edge and very large
// shapes.  Every call returns before a launch, so no GPU is needed and nothing sanitized runs on one.  From the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         reactranker_amd/csrc/knn.hip reactranker_amd/csrc/cluster.hip tools/cluster_host_check.cpp \
//         -o /tmp/cluster_host_check && /tmp/cluster_host_check
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstddef>
#include "../include/reactranker_hip.h"
int main() {
  float* F = reinterpret_cast<float*>(4096);
  int32_t* I = reinterpret_cast<int32_t*>(4096);
  int bad = 0;
  auto expect = [&](int got, int want, int line) { if (got != want) { std::printf("line %d: %d != %d\n", line, got, want); ++bad; } };
  const size_t big = static_cast<size_t>(1) << 40;
  const float nan = std::nanf(""), inf = INFINITY;
  const long long MAXR = 2147483647LL;
  size_t need = 0;

  // ---- rr_radius_count_*
  expect(rr_radius_count_workspace_bytes(4, 100, &need), RR_OK, __LINE__);
  expect(rr_radius_count_workspace_bytes(4, 100, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_radius_count_workspace_bytes(-1, 100, &need), RR_ERR_ARG, __LINE__);
  expect(rr_radius_count_workspace_bytes(4, -1, &need), RR_ERR_ARG, __LINE__);
  expect(rr_radius_count_workspace_bytes(MAXR + 1, 4, &need), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_radius_count_workspace_bytes(4, MAXR + 1, &need), RR_ERR_UNSUPPORTED, __LINE__);
  for (int64_t M : {0LL, 1LL, 63LL, 64LL, 65LL, 1000000LL, MAXR})
    for (int64_t N : {0LL, 1LL, 127LL, 128LL, 129LL, 1000000LL, MAXR})
      for (int s : {0, 1, 2, 7, 1024}) {
        expect(rr_knn_set_splits(s), RR_OK, __LINE__);
        size_t got = 0;
        expect(rr_radius_count_workspace_bytes(M, N, &got), RR_OK, __LINE__);
        if (got < static_cast<size_t>(M) * 4 + static_cast<size_t>(N) * 4) { std::printf("too small\n"); ++bad; }
        // (the size is checked before M == 0 returns)
        expect(rr_radius_count_f32(F, 8, M, F, 8, N, 8, 1.0f, nullptr, nullptr, nullptr, I, F, got - 1, nullptr), RR_ERR_WORKSPACE, __LINE__);
        expect(rr_radius_count_f32(F, 8, M, F, 8, N, 8, 1.0f, I, I, F, I, F, 0, nullptr), RR_ERR_WORKSPACE, __LINE__);
      }
  expect(rr_knn_set_splits(0), RR_OK, __LINE__);
  expect(rr_radius_count_f32(nullptr, 8, 4, F, 8, 9, 8, 1.0f, nullptr, nullptr, nullptr, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_radius_count_f32(F, 8, 4, nullptr, 8, 9, 8, 1.0f, nullptr, nullptr, nullptr, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_radius_count_f32(F, 8, 4, F, 8, 9, 8, 1.0f, nullptr, nullptr, nullptr, nullptr, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_radius_count_f32(F, 8, 4, F, 8, 9, 8, 1.0f, nullptr, nullptr, nullptr, I, nullptr, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_radius_count_f32(F, 8, 4, F, 8, 9, 8, 1.0f, I, nullptr, nullptr, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_radius_count_f32(F, 8, 4, F, 8, 9, 8, 1.0f, nullptr, I, nullptr, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_radius_count_f32(F, 8, -1, F, 8, 9, 8, 1.0f, nullptr, nullptr, nullptr, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_radius_count_f32(F, 8, 4, F, 8, -1, 8, 1.0f, nullptr, nullptr, nullptr, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_radius_count_f32(F, 8, 4, F, 8, 9, 0, 1.0f, nullptr, nullptr, nullptr, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_radius_count_f32(F, 7, 4, F, 8, 9, 8, 1.0f, nullptr, nullptr, nullptr, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_radius_count_f32(F, 8, 4, F, 7, 9, 8, 1.0f, nullptr, nullptr, nullptr, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_radius_count_f32(F, 8, 4, F, 8, 9, 8, nan, nullptr, nullptr, nullptr, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_radius_count_f32(F, 8, 4, F, 8, 9, 8, -1.0f, nullptr, nullptr, nullptr, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_radius_count_f32(F, 8, 4, F, 8, 9, 8, -inf, nullptr, nullptr, nullptr, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_radius_count_f32(F, 8, MAXR + 1, F, 8, 9, 8, 1.0f, nullptr, nullptr, nullptr, I, F, big, nullptr), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_radius_count_f32(F, 8, 4, F, 8, MAXR + 1, 8, 1.0f, nullptr, nullptr, nullptr, I, F, big, nullptr), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_radius_count_f32(F, 8, 0, F, 8, 9, 8, inf, nullptr, nullptr, nullptr, I, F, big, nullptr), RR_OK, __LINE__);
  expect(rr_radius_count_f32(F, 8, 0, F, 8, MAXR, 8, 0.0f, I, I, F, I, F, big, nullptr), RR_OK, __LINE__);

  // ---- rr_sphere_exclusion_*
  expect(rr_sphere_exclusion_workspace_bytes(100, &need), RR_OK, __LINE__);
  expect(rr_sphere_exclusion_workspace_bytes(100, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_sphere_exclusion_workspace_bytes(-1, &need), RR_ERR_ARG, __LINE__);
  expect(rr_sphere_exclusion_workspace_bytes(MAXR + 1, &need), RR_ERR_UNSUPPORTED, __LINE__);
  for (int64_t P : {0LL, 1LL, 3LL, 4LL, 5LL, 255LL, 256LL, 257LL, 1000000LL, MAXR})
    for (int n : {0, 1, 64, RR_SPHERE_EXCLUSION_MAX_ROUNDS})
      for (int b : {0, 1, 2, 3, 4096}) {
        expect(rr_sphere_exclusion_set_blocks(b), RR_OK, __LINE__);
        expect(rr_sphere_exclusion_blocks(), b, __LINE__);
        size_t got = 0;
        expect(rr_sphere_exclusion_workspace_bytes(P, &got), RR_OK, __LINE__);
        if (got < 2 * 4097 * 8) { std::printf("too small\n"); ++bad; }
        if (b == 0) need = got;
        if (got != need) { std::printf("the workspace moved with the blocks setting\n"); ++bad; }
        for (int first : {0, 1, 2147483647 - RR_SPHERE_EXCLUSION_MAX_ROUNDS}) {
          expect(rr_sphere_exclusion_f32(F, 8, P, 8, 1.0f, nullptr, first, n, I, I, F, got - 1, nullptr), RR_ERR_WORKSPACE, __LINE__);
          expect(rr_sphere_exclusion_f32(F, 8, P, 8, inf, I, first, n, I, I, F, 0, nullptr), RR_ERR_WORKSPACE, __LINE__);
        }
      }
  expect(rr_sphere_exclusion_set_blocks(-1), RR_ERR_ARG, __LINE__);
  expect(rr_sphere_exclusion_set_blocks(4097), RR_ERR_ARG, __LINE__);
  expect(rr_sphere_exclusion_blocks(), 4096, __LINE__);
  expect(rr_sphere_exclusion_set_blocks(0), RR_OK, __LINE__);
  expect(rr_sphere_exclusion_f32(nullptr, 8, 4, 8, 1.0f, nullptr, 0, 3, I, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_sphere_exclusion_f32(F, 8, 4, 8, 1.0f, nullptr, 0, 3, nullptr, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_sphere_exclusion_f32(F, 8, 4, 8, 1.0f, nullptr, 0, 3, I, nullptr, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_sphere_exclusion_f32(F, 8, 4, 8, 1.0f, nullptr, 0, 3, I, I, nullptr, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_sphere_exclusion_f32(F, 8, -1, 8, 1.0f, nullptr, 0, 3, I, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_sphere_exclusion_f32(F, 8, 4, 8, 1.0f, nullptr, -1, 3, I, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_sphere_exclusion_f32(F, 8, 4, 8, 1.0f, nullptr, 0, -1, I, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_sphere_exclusion_f32(F, 8, 4, 0, 1.0f, nullptr, 0, 3, I, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_sphere_exclusion_f32(F, 7, 4, 8, 1.0f, nullptr, 0, 3, I, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_sphere_exclusion_f32(F, 8, 4, 8, nan, nullptr, 0, 3, I, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_sphere_exclusion_f32(F, 8, 4, 8, -1.0f, nullptr, 0, 3, I, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_sphere_exclusion_f32(F, 8, 4, 8, -inf, nullptr, 0, 3, I, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_sphere_exclusion_f32(F, 8, 4, 8, 1.0f, nullptr, 0, RR_SPHERE_EXCLUSION_MAX_ROUNDS + 1, I, I, F, big, nullptr), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_sphere_exclusion_f32(F, 8, MAXR + 1, 8, 1.0f, nullptr, 0, 3, I, I, F, big, nullptr), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_sphere_exclusion_f32(F, 8, 4, 8, 1.0f, nullptr, 2147483647, 1, I, I, F, big, nullptr), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_sphere_exclusion_f32(F, 8, 4, 8, 1.0f, nullptr, 2147483645, 3, I, I, F, big, nullptr), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_sphere_exclusion_f32(F, 8, 0, 8, inf, nullptr, 0, 0, I, I, F, big, nullptr), RR_OK, __LINE__);
  expect(rr_sphere_exclusion_f32(F, 8, 0, 8, 0.0f, I, 2147483647, 0, I, I, F, big, nullptr), RR_OK, __LINE__);
  // (first_round > 0 with no rounds to run launches nothing either, whatever P is)
  expect(rr_sphere_exclusion_f32(F, 8, MAXR, 8, 1.0f, nullptr, 5, 0, I, I, F, big, nullptr), RR_OK, __LINE__);
  std::printf("%s\n", bad ? "FAILED" : "host checks clean");
  return bad != 0;
}
