// Host side of the k-center entry points under the host sanitizers: the argument checks, the blocks setting and the workspace
// sizing of csrc/kcenter.hip over edge and very large shapes.  Every call returns before a launch, so no GPU is needed and
// nothing sanitized runs on one.  From the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         reactranker_amd/csrc/kcenter.hip tools/kcenter_host_check.cpp -o /tmp/kcenter_host_check && /tmp/kcenter_host_check
#include <cstdio>
#include <cstdint>
#include <cstddef>
#include "../include/reactranker_hip.h"
int main() {
  float* F = reinterpret_cast<float*>(4096);
  int32_t* I = reinterpret_cast<int32_t*>(4096);
  int bad = 0;
  auto expect = [&](int got, int want, int line) { if (got != want) { std::printf("line %d: %d != %d\n", line, got, want); ++bad; } };
  size_t need = 0;
  expect(rr_kcenter_workspace_bytes(100, 5, &need), RR_OK, __LINE__);
  expect(rr_kcenter_workspace_bytes(100, 5, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_kcenter_workspace_bytes(-1, 5, &need), RR_ERR_ARG, __LINE__);
  expect(rr_kcenter_workspace_bytes(100, -1, &need), RR_ERR_ARG, __LINE__);
  expect(rr_kcenter_workspace_bytes(100, RR_KCENTER_MAX_PICKS + 1, &need), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_kcenter_workspace_bytes(2147483648LL, 5, &need), RR_ERR_UNSUPPORTED, __LINE__);
  for (int64_t P : {0LL, 1LL, 3LL, 4LL, 5LL, 255LL, 256LL, 257LL, 1000000LL, 2147483647LL})
    for (int n : {0, 1, 64, RR_KCENTER_MAX_PICKS})
      for (int b : {0, 1, 2, 3, 4096}) {
        expect(rr_kcenter_set_blocks(b), RR_OK, __LINE__);
        expect(rr_kcenter_blocks(), b, __LINE__);
        size_t got = 0;
        expect(rr_kcenter_workspace_bytes(P, n, &got), RR_OK, __LINE__);
        if (got < static_cast<size_t>(P) + 2 * 4096 * 8) { std::printf("too small\n"); ++bad; }
        if (b == 0) need = got;
        if (got != need) { std::printf("the workspace moved with the blocks setting\n"); ++bad; }
        expect(rr_kcenter_f32(F, 8, P, 8, n, nullptr, nullptr, I, F, F, I, F, got - 1, nullptr), RR_ERR_WORKSPACE, __LINE__);
        expect(rr_kcenter_f32(F, 8, P, 8, n, F, F, I, F, F, I, F, 0, nullptr), RR_ERR_WORKSPACE, __LINE__);
      }
  expect(rr_kcenter_set_blocks(-1), RR_ERR_ARG, __LINE__);
  expect(rr_kcenter_set_blocks(4097), RR_ERR_ARG, __LINE__);
  expect(rr_kcenter_blocks(), 4096, __LINE__);
  expect(rr_kcenter_set_blocks(0), RR_OK, __LINE__);
  const size_t big = static_cast<size_t>(1) << 40;
  expect(rr_kcenter_f32(nullptr, 8, 4, 8, 3, nullptr, nullptr, I, F, F, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_kcenter_f32(F, 8, 4, 8, 3, nullptr, nullptr, nullptr, F, F, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_kcenter_f32(F, 8, 4, 8, 3, nullptr, nullptr, I, nullptr, F, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_kcenter_f32(F, 8, 4, 8, 3, nullptr, nullptr, I, F, nullptr, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_kcenter_f32(F, 8, 4, 8, 3, nullptr, nullptr, I, F, F, nullptr, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_kcenter_f32(F, 8, 4, 8, 3, nullptr, nullptr, I, F, F, I, nullptr, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_kcenter_f32(F, 8, -1, 8, 3, nullptr, nullptr, I, F, F, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_kcenter_f32(F, 8, 4, 8, -1, nullptr, nullptr, I, F, F, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_kcenter_f32(F, 8, 4, 0, 3, nullptr, nullptr, I, F, F, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_kcenter_f32(F, 7, 4, 8, 3, nullptr, nullptr, I, F, F, I, F, big, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_kcenter_f32(F, 8, 4, 8, RR_KCENTER_MAX_PICKS + 1, nullptr, nullptr, I, F, F, I, F, big, nullptr), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_kcenter_f32(F, 8, 2147483648LL, 8, 3, nullptr, nullptr, I, F, F, I, F, big, nullptr), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_kcenter_f32(F, 8, 0, 8, 0, nullptr, nullptr, I, F, F, I, F, big, nullptr), RR_OK, __LINE__);
  std::printf("%s\n", bad ? "FAILED" : "host checks clean");
  return bad != 0;
}
