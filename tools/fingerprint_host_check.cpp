// Host side of the fingerprint and Tanimoto entry points under the host sanitizers: the argument checks, the limits, the split
// setting and the workspace sizing of csrc/fingerprint.hip and csrc/tanimoto.hip.  Every call returns before a launch, so no GPU
// is needed and nothing sanitized runs on one.  From the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         reactranker_amd/csrc/fingerprint.hip reactranker_amd/csrc/tanimoto.hip tools/fingerprint_host_check.cpp \
//         -o /tmp/fingerprint_host_check && /tmp/fingerprint_host_check
#include <cstdio>
#include <cstdint>
#include <cstddef>
#include "../include/reactranker_hip.h"
int main() {
  float* P = reinterpret_cast<float*>(4096);
  int32_t* I = reinterpret_cast<int32_t*>(4096);
  uint32_t* U = reinterpret_cast<uint32_t*>(4096);
  int bad = 0;
  auto expect = [&](int got, int want, int line) { if (got != want) { std::printf("line %d: %d != %d\n", line, got, want); ++bad; } };
  size_t need = 0;
  // ---- the fingerprint
  expect(rr_circular_fp_workspace_bytes(10, 20, &need), RR_OK, __LINE__);
  expect(rr_circular_fp_workspace_bytes(10, 20, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_circular_fp_workspace_bytes(0, 20, &need), RR_ERR_ARG, __LINE__);
  expect(rr_circular_fp_workspace_bytes(10, 1LL << 31, &need), RR_ERR_UNSUPPORTED, __LINE__);
  auto fp = [&](int radius, int bits, uint32_t* bo, int64_t ldb, int32_t* co, int64_t ldc, int64_t M, size_t bytes) {
    return rr_circular_fp_u32(P, 64, 61, P, 84, 22, I, 6, I, I, 1000, 2000, M, radius, bits, bo, ldb, co, ldc, P, bytes, nullptr);
  };
  for (int64_t nA : {1LL, 2LL, 257LL, 100000LL, 2147483647LL})
    for (int64_t nB : {1LL, 3LL, 2147483647LL}) {
      expect(rr_circular_fp_workspace_bytes(nA, nB, &need), RR_OK, __LINE__);
      if (need < static_cast<size_t>(nA) * 12 + static_cast<size_t>(nB) * 4) { std::printf("too small\n"); ++bad; }
      expect(rr_circular_fp_u32(P, 64, 61, P, 84, 22, I, 6, I, I, nA, nB, 5, 2, 2048, U, 64, nullptr, 0, P, need - 1, nullptr),
             RR_ERR_WORKSPACE, __LINE__);
    }
  expect(fp(2, 2048, U, 64, I, 2048, 0, 1 << 20), RR_OK, __LINE__);                    // M == 0: nothing to launch
  expect(fp(2, 2048, nullptr, 0, nullptr, 0, 5, 1 << 20), RR_ERR_ARG, __LINE__);
  expect(fp(-1, 2048, U, 64, nullptr, 0, 5, 1 << 20), RR_ERR_ARG, __LINE__);
  expect(fp(9, 2048, U, 64, nullptr, 0, 5, 1 << 20), RR_ERR_UNSUPPORTED, __LINE__);
  expect(fp(2, 0, U, 64, nullptr, 0, 5, 1 << 20), RR_ERR_ARG, __LINE__);
  expect(fp(2, 16, U, 64, nullptr, 0, 5, 1 << 20), RR_ERR_ARG, __LINE__);
  expect(fp(2, 2080 + 16, U, 128, nullptr, 0, 5, 1 << 20), RR_ERR_ARG, __LINE__);
  expect(fp(2, 8192 + 32, U, 512, nullptr, 0, 5, 1 << 20), RR_ERR_UNSUPPORTED, __LINE__);
  expect(fp(2, 2048, U, 63, nullptr, 0, 5, 1 << 20), RR_ERR_ARG, __LINE__);
  expect(fp(2, 2048, nullptr, 0, I, 2047, 5, 1 << 20), RR_ERR_ARG, __LINE__);
  expect(fp(2, 2048, U, 64, nullptr, 0, -1, 1 << 20), RR_ERR_ARG, __LINE__);
  expect(fp(2, 2048, U, 64, nullptr, 0, 5, 16), RR_ERR_WORKSPACE, __LINE__);
  expect(rr_circular_fp_u32(nullptr, 64, 61, P, 84, 22, I, 6, I, I, 10, 20, 5, 2, 64, U, 2, nullptr, 0, P, 1 << 20, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_circular_fp_u32(P, 60, 61, P, 84, 22, I, 6, I, I, 10, 20, 5, 2, 64, U, 2, nullptr, 0, P, 1 << 20, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_circular_fp_u32(P, 64, 61, P, 84, 22, I, 0, I, I, 10, 20, 5, 2, 64, U, 2, nullptr, 0, P, 1 << 20, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_circular_fp_u32(P, 64, 61, P, 84, 22, I, 6, I, nullptr, 10, 20, 5, 2, 64, U, 2, nullptr, 0, P, 1 << 20, nullptr), RR_ERR_ARG, __LINE__);
  // ---- the search
  expect(rr_tanimoto_knn_workspace_bytes(4, 100, 3, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_tanimoto_knn_workspace_bytes(-1, 100, 3, &need), RR_ERR_ARG, __LINE__);
  expect(rr_tanimoto_knn_workspace_bytes(4, 100, 65, &need), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_tanimoto_count_workspace_bytes(4, 1LL << 31, &need), RR_ERR_UNSUPPORTED, __LINE__);
  for (int64_t M : {0LL, 1LL, 63LL, 64LL, 65LL, 4096LL, 100000LL})
    for (int64_t N : {0LL, 1LL, 127LL, 128LL, 129LL, 1000000LL, 2147483647LL})
      for (int s : {0, 1, 2, 7, 1024}) {
        expect(rr_tanimoto_set_splits(s), RR_OK, __LINE__);
        for (int k : {1, 2, 63, 64}) {
          expect(rr_tanimoto_knn_workspace_bytes(M, N, k, &need), RR_OK, __LINE__);
          if (need < static_cast<size_t>(M) * 4 + static_cast<size_t>(N) * 4) { std::printf("too small\n"); ++bad; }
          expect(rr_tanimoto_knn_u32(U, 8, M, U, 8, N, 8, k, nullptr, nullptr, nullptr, P, I, P, need - 1, nullptr), RR_ERR_WORKSPACE, __LINE__);
        }
        expect(rr_tanimoto_count_workspace_bytes(M, N, &need), RR_OK, __LINE__);
        expect(rr_tanimoto_count_u32(U, 8, M, U, 8, N, 8, 0.5f, nullptr, nullptr, nullptr, I, P, need - 1, nullptr), RR_ERR_WORKSPACE, __LINE__);
      }
  expect(rr_tanimoto_set_splits(-1), RR_ERR_ARG, __LINE__);
  expect(rr_tanimoto_set_splits(1025), RR_ERR_ARG, __LINE__);
  expect(rr_tanimoto_set_splits(0), RR_OK, __LINE__);
  expect(rr_tanimoto_splits(), 0, __LINE__);
  expect(rr_tanimoto_knn_u32(nullptr, 8, 4, U, 8, 100, 8, 3, nullptr, nullptr, nullptr, P, I, P, 1 << 20, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_tanimoto_knn_u32(U, 8, 4, U, 8, 100, 8, 3, I, nullptr, nullptr, P, I, P, 1 << 20, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_tanimoto_knn_u32(U, 7, 4, U, 8, 100, 8, 3, nullptr, nullptr, nullptr, P, I, P, 1 << 20, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_tanimoto_knn_u32(U, 8, 4, U, 8, 100, 0, 3, nullptr, nullptr, nullptr, P, I, P, 1 << 20, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_tanimoto_knn_u32(U, 8, 4, U, 8, 100, 8, 65, nullptr, nullptr, nullptr, P, I, P, 1 << 20, nullptr), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_tanimoto_knn_u32(U, 300, 4, U, 300, 100, 257, 3, nullptr, nullptr, nullptr, P, I, P, 1 << 20, nullptr), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_tanimoto_knn_u32(U, 8, 0, U, 8, 100, 8, 3, nullptr, nullptr, nullptr, P, I, P, 1 << 20, nullptr), RR_OK, __LINE__);
  expect(rr_tanimoto_count_u32(U, 8, 4, U, 8, 100, 8, -0.5f, nullptr, nullptr, nullptr, I, P, 1 << 20, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_tanimoto_count_u32(U, 8, 4, U, 8, 100, 8, 0.0f / 0.0f, nullptr, nullptr, nullptr, I, P, 1 << 20, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_tanimoto_count_u32(U, 8, 4, U, 8, 100, 8, 0.5f, nullptr, nullptr, nullptr, nullptr, P, 1 << 20, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_tanimoto_count_u32(U, 8, 0, U, 8, 100, 8, 0.5f, nullptr, nullptr, nullptr, I, P, 1 << 20, nullptr), RR_OK, __LINE__);
  expect(rr_row_popcount_u32(U, 7, 4, 8, I, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_row_popcount_u32(U, 8, 0, 8, I, nullptr), RR_OK, __LINE__);
  int a, b, c, d; rr_tanimoto_geometry(&a, &b, &c, &d); rr_tanimoto_geometry(nullptr, nullptr, nullptr, nullptr);
  std::printf("%s (%d %d %d %d)\n", bad ? "FAILED" : "host checks clean", a, b, c, d);
  return bad != 0;
}
