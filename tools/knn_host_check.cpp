// Host side of the nearest-neighbour entry points under the host sanitizers: the argument checks, the split setting and the
// workspace sizing of csrc/knn.hip over tile-edge and very large shapes.  Every call returns before a launch, so no GPU is
// needed and nothing sanitized runs on one.  From the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         reactranker_amd/csrc/knn.hip tools/knn_host_check.cpp -o /tmp/knn_host_check && /tmp/knn_host_check
#include <cstdio>
#include <cstdint>
#include <cstddef>
#include "../include/reactranker_hip.h"
int main() {
  float* P = reinterpret_cast<float*>(4096);
  int32_t* I = reinterpret_cast<int32_t*>(4096);
  int bad = 0;
  auto expect = [&](int got, int want, int line) { if (got != want) { std::printf("line %d: %d != %d\n", line, got, want); ++bad; } };
  size_t need = 0;
  expect(rr_knn_workspace_bytes(4, 100, 3, &need), RR_OK, __LINE__);
  expect(rr_knn_workspace_bytes(4, 100, 3, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_knn_workspace_bytes(-1, 100, 3, &need), RR_ERR_ARG, __LINE__);
  expect(rr_knn_workspace_bytes(4, 100, 65, &need), RR_ERR_UNSUPPORTED, __LINE__);
  for (int64_t M : {0LL, 1LL, 63LL, 64LL, 65LL, 4096LL, 100000LL})
    for (int64_t N : {0LL, 1LL, 127LL, 128LL, 129LL, 1000000LL, 2147483647LL})
      for (int k : {1, 2, 63, 64})
        for (int s : {0, 1, 2, 7, 1024}) {
          expect(rr_knn_set_splits(s), RR_OK, __LINE__);
          expect(rr_knn_workspace_bytes(M, N, k, &need), RR_OK, __LINE__);
          if (need < static_cast<size_t>(M) * 4 + static_cast<size_t>(N) * 4) { std::printf("too small\n"); ++bad; }
          expect(rr_knn_f32(P, 8, M, P, 8, N, 8, k, nullptr, nullptr, nullptr, P, I, P, need - 1, nullptr), RR_ERR_WORKSPACE, __LINE__);
        }
  expect(rr_knn_set_splits(-1), RR_ERR_ARG, __LINE__);
  expect(rr_knn_set_splits(1025), RR_ERR_ARG, __LINE__);
  expect(rr_knn_set_splits(0), RR_OK, __LINE__);
  expect(rr_knn_f32(nullptr, 8, 4, P, 8, 100, 8, 3, nullptr, nullptr, nullptr, P, I, P, 1 << 20, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_knn_f32(P, 8, 4, P, 8, 100, 8, 3, I, nullptr, nullptr, P, I, P, 1 << 20, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_knn_f32(P, 7, 4, P, 8, 100, 8, 3, nullptr, nullptr, nullptr, P, I, P, 1 << 20, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_knn_f32(P, 8, 4, P, 8, 100, 8, 65, nullptr, nullptr, nullptr, P, I, P, 1 << 20, nullptr), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_knn_f32(P, 8, 0, P, 8, 100, 8, 3, nullptr, nullptr, nullptr, P, I, P, 1 << 20, nullptr), RR_OK, __LINE__);
  expect(rr_row_sqnorm_f32(P, 7, 4, 8, P, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_row_sqnorm_f32(P, 8, 0, 8, P, nullptr), RR_OK, __LINE__);
  int a, b, c; rr_knn_geometry(&a, &b, &c); rr_knn_geometry(nullptr, nullptr, nullptr);
  std::printf("%s (%d %d %d)\n", bad ? "FAILED" : "host checks clean", a, b, c);
  return bad != 0;
}
