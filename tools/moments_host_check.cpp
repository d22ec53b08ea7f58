// Host side of the moments / projection entry points under the host sanitizers: the argument checks, the limits, the blocks
// setting, the chunk function and the workspace sizing of csrc/moments.hip over edge and very large shapes.  Every call returns
// before a launch, so no GPU is needed and nothing sanitized runs on one.  Built as tools/knn_host_check.cpp says, from the
// repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         reactranker_amd/csrc/moments.hip tools/moments_host_check.cpp -o /tmp/moments_host_check && /tmp/moments_host_check
#include <cstdio>
#include <cstdint>
#include <cstddef>
#include "../include/reactranker_hip.h"
int main() {
  float* F = reinterpret_cast<float*>(4096);
  double* D = reinterpret_cast<double*>(4096);
  int64_t* L = reinterpret_cast<int64_t*>(4096);
  int bad = 0;
  auto expect = [&](int got, int want, int line) { if (got != want) { std::printf("line %d: %d != %d\n", line, got, want); ++bad; } };
  const size_t big = static_cast<size_t>(1) << 40;
  size_t need = 0;
  expect(rr_moments_workspace_bytes(100, 8, &need), RR_OK, __LINE__);
  expect(rr_moments_workspace_bytes(100, 8, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_moments_workspace_bytes(-1, 8, &need), RR_ERR_ARG, __LINE__);
  expect(rr_moments_workspace_bytes(100, 0, &need), RR_ERR_ARG, __LINE__);
  expect(rr_moments_workspace_bytes(100, RR_MOMENTS_MAX_H + 1, &need), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_moments_workspace_bytes(2147483648LL, 8, &need), RR_ERR_UNSUPPORTED, __LINE__);
  for (int64_t N : {0LL, 1LL, 3LL, 4LL, 5LL, 1023LL, 1024LL, 1025LL, 2048LL, 2049LL, 65536LL, 65537LL, 1000000LL, 6400000LL, 2147483646LL, 2147483647LL})
    for (int H : {1, 3, 63, 64, 65, 300, 322, 600, 1023, RR_MOMENTS_MAX_H}) {
      const int chunks = rr_moments_chunks(N, H);
      const int64_t hp = (H + 63) / 64 * 64;
      int64_t want = (N + 1023) / 1024;
      if (want > 64) want = 64;
      if (want > (int64_t(1) << 28) / (8 * hp * hp)) want = (int64_t(1) << 28) / (8 * hp * hp);
      if (want < 1) want = 1;
      expect(chunks, static_cast<int>(want), __LINE__);
      for (int b : {0, 1, 3, 4096}) {
        expect(rr_moments_set_blocks(b), RR_OK, __LINE__);
        expect(rr_moments_blocks(), b, __LINE__);
        size_t got = 0;
        expect(rr_moments_workspace_bytes(N, H, &got), RR_OK, __LINE__);
        const size_t least = static_cast<size_t>(N) + static_cast<size_t>(chunks) * (8 + hp * 8 + hp * hp * 8);
        if (got < least || got > least + 4 * 256) { std::printf("N %lld H %d: workspace %zu, expected %zu .. + 1024\n", (long long)N, H, got, least); ++bad; }
        if (b == 0) need = got;
        if (got != need) { std::printf("the workspace moved with the blocks setting\n"); ++bad; }
        expect(rr_col_moments_f64(F, H, N, H, D, D, L, F, got - 1, nullptr), RR_ERR_WORKSPACE, __LINE__);
        expect(rr_col_moments_f64(F, H + 5, N, H, D, D, L, F, 0, nullptr), RR_ERR_WORKSPACE, __LINE__);
      }
    }
  expect(rr_moments_chunks(5, RR_MOMENTS_MAX_H + 1), 0, __LINE__);
  expect(rr_moments_chunks(-1, 8), 0, __LINE__);
  expect(rr_moments_chunks(5, 0), 0, __LINE__);
  expect(rr_moments_set_blocks(-1), RR_ERR_ARG, __LINE__);
  expect(rr_moments_set_blocks(4097), RR_ERR_ARG, __LINE__);
  expect(rr_moments_blocks(), 4096, __LINE__);
  expect(rr_moments_set_blocks(0), RR_OK, __LINE__);
  expect(rr_col_moments_f64(nullptr, 8, 4, 8, D, D, L, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_col_moments_f64(F, 8, 4, 8, nullptr, D, L, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_col_moments_f64(F, 8, 4, 8, D, nullptr, L, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_col_moments_f64(F, 8, 4, 8, D, D, nullptr, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_col_moments_f64(F, 8, 4, 8, D, D, L, nullptr, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_col_moments_f64(F, 8, -1, 8, D, D, L, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_col_moments_f64(F, 8, 4, 0, D, D, L, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_col_moments_f64(F, 7, 4, 8, D, D, L, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_col_moments_f64(F, 2000, 4, RR_MOMENTS_MAX_H + 1, D, D, L, F, big, nullptr), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_col_moments_f64(F, 2000, 4, RR_MOMENTS_MAX_H + 1, D, D, L, F, 0, nullptr), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_col_moments_f64(F, 8, 2147483648LL, 8, D, D, L, F, big, nullptr), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_center_project_f32(nullptr, 8, 4, 8, F, F, 4, F, F, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_center_project_f32(F, 8, 4, 8, F, nullptr, 4, F, F, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_center_project_f32(F, 8, 4, 8, F, F, 4, nullptr, nullptr, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_center_project_f32(F, 8, -1, 8, F, F, 4, F, F, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_center_project_f32(F, 8, 4, 0, F, F, 4, F, F, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_center_project_f32(F, 7, 4, 8, F, F, 4, F, F, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_center_project_f32(F, 8, 4, 8, F, F, 0, F, F, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_center_project_f32(F, 8, 4, 8, F, F, 9, F, F, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_center_project_f32(F, 8, 2147483648LL, 8, F, F, 4, F, F, nullptr), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_center_project_f32(F, 8, 0, 8, nullptr, F, 8, nullptr, F, nullptr), RR_OK, __LINE__);
  expect(rr_center_project_f32(F, 1024, 0, 1024, F, F, 1024, F, nullptr, nullptr), RR_OK, __LINE__);
  std::printf("%s\n", bad ? "FAILED" : "host checks clean");
  return bad != 0;
}
