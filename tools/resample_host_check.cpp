// Host side of the resampling entry points under the host sanitizers: every argument check and limit of csrc/resample.hip, the
// blocks setting, and rr_resample_draw_host against values of the numpy restatement (tests/resample_ref.py: draws).  Every call
// returns before a launch, so no GPU is needed and nothing sanitized runs on one.  From the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         reactranker_amd/csrc/resample.hip tools/resample_host_check.cpp -o /tmp/resample_host_check && /tmp/resample_host_check
#include <cstdio>
#include <cstdint>
#include <cstddef>
#include "../include/reactranker_hip.h"

// {seed, j, draw(seed, j)} as tests/resample_ref.py computes them: R.draws(seed, np.array([j], np.uint64))
struct Draw { uint64_t seed, j; uint32_t want; };
static const Draw kDraws[] = {
  {0ull, 0ull, 3793791033u},
  {0ull, 1ull, 2065550767u},
  {0ull, 2ull, 1853398634u},
  {0ull, 3ull, 2713282036u},
  {0ull, 6ull, 4169906344u},
  {0ull, 7ull, 1917616620u},
  {0ull, 1000ull, 1130446259u},
  {0ull, 1001ull, 4038254861u},
  {0ull, 4294967294ull, 3226589675u},
  {0ull, 4294967295ull, 1821355342u},
  {0ull, 4294967296ull, 1886314076u},
  {0ull, 4294967297ull, 4242315804u},
  {0ull, 51539607552ull, 2012101383u},
  {0ull, 51539607557ull, 2971764266u},
  {0ull, 9223372036854775805ull, 525097139u},
  {0ull, 9223372036854775806ull, 316749650u},
  {1ull, 0ull, 3220144176u},
  {1ull, 1ull, 3720533874u},
  {1ull, 2ull, 1599417572u},
  {1ull, 3ull, 2196941383u},
  {1ull, 6ull, 4097900091u},
  {1ull, 7ull, 1657249068u},
  {1ull, 1000ull, 611859646u},
  {1ull, 1001ull, 3900158593u},
  {1ull, 4294967294ull, 1719527551u},
  {1ull, 4294967295ull, 1143469552u},
  {1ull, 4294967296ull, 4009265247u},
  {1ull, 4294967297ull, 955681581u},
  {1ull, 51539607552ull, 757364612u},
  {1ull, 51539607557ull, 1705207220u},
  {1ull, 9223372036854775805ull, 3178380992u},
  {1ull, 9223372036854775806ull, 1573062258u},
  {12345ull, 0ull, 2142698583u},
  {12345ull, 1ull, 2530309496u},
  {12345ull, 2ull, 1967658477u},
  {12345ull, 3ull, 3698615870u},
  {12345ull, 6ull, 4228702624u},
  {12345ull, 7ull, 1112809779u},
  {12345ull, 1000ull, 953220783u},
  {12345ull, 1001ull, 2558322848u},
  {12345ull, 4294967294ull, 202876740u},
  {12345ull, 4294967295ull, 2141781629u},
  {12345ull, 4294967296ull, 2995784519u},
  {12345ull, 4294967297ull, 1612971852u},
  {12345ull, 51539607552ull, 958998659u},
  {12345ull, 51539607557ull, 1825611836u},
  {12345ull, 9223372036854775805ull, 2014901024u},
  {12345ull, 9223372036854775806ull, 563310565u},
  {9223372036854775815ull, 0ull, 2247841145u},
  {9223372036854775815ull, 1ull, 3908802957u},
  {9223372036854775815ull, 2ull, 584409960u},
  {9223372036854775815ull, 3ull, 1713942444u},
  {9223372036854775815ull, 6ull, 2975164736u},
  {9223372036854775815ull, 7ull, 1034385471u},
  {9223372036854775815ull, 1000ull, 2252243956u},
  {9223372036854775815ull, 1001ull, 3776329989u},
  {9223372036854775815ull, 4294967294ull, 207540573u},
  {9223372036854775815ull, 4294967295ull, 1774472314u},
  {9223372036854775815ull, 4294967296ull, 3290129319u},
  {9223372036854775815ull, 4294967297ull, 4077288658u},
  {9223372036854775815ull, 51539607552ull, 1698545037u},
  {9223372036854775815ull, 51539607557ull, 1683207424u},
  {9223372036854775815ull, 9223372036854775805ull, 2293823394u},
  {9223372036854775815ull, 9223372036854775806ull, 2493984432u},
  {18446744073709551615ull, 0ull, 2776070187u},
  {18446744073709551615ull, 1ull, 3307904858u},
  {18446744073709551615ull, 2ull, 3028624451u},
  {18446744073709551615ull, 3ull, 2162528446u},
  {18446744073709551615ull, 6ull, 122719827u},
  {18446744073709551615ull, 7ull, 3055007431u},
  {18446744073709551615ull, 1000ull, 2742374257u},
  {18446744073709551615ull, 1001ull, 793120447u},
  {18446744073709551615ull, 4294967294ull, 1989947570u},
  {18446744073709551615ull, 4294967295ull, 3678239583u},
  {18446744073709551615ull, 4294967296ull, 3409600629u},
  {18446744073709551615ull, 4294967297ull, 1440277390u},
  {18446744073709551615ull, 51539607552ull, 234952645u},
  {18446744073709551615ull, 51539607557ull, 1755133500u},
  {18446744073709551615ull, 9223372036854775805ull, 3296384835u},
  {18446744073709551615ull, 9223372036854775806ull, 4094759220u},
};

int main() {
  double* D = reinterpret_cast<double*>(4096);
  int32_t* I = reinterpret_cast<int32_t*>(4096);
  int bad = 0;
  auto expect = [&](int got, int want, int line) { if (got != want) { std::printf("line %d: %d != %d\n", line, got, want); ++bad; } };
  const int B0 = RR_RESAMPLE_BOOTSTRAP, SF = RR_RESAMPLE_SIGNFLIP;
  // arguments
  expect(rr_resample_means_f64(nullptr, 8, 100, 8, B0, 1, 0, 5, D, I, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_resample_means_f64(D, 8, 100, 8, B0, 1, 0, 5, nullptr, I, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_resample_means_f64(D, 8, -1, 8, B0, 1, 0, 5, D, I, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_resample_means_f64(D, 8, 100, 8, B0, 1, 0, -1, D, I, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_resample_means_f64(D, 8, 100, 8, B0, 1, -1, 5, D, I, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_resample_means_f64(D, 8, 100, 0, B0, 1, 0, 5, D, I, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_resample_means_f64(D, 8, 100, -4, SF, 1, 0, 5, D, I, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_resample_means_f64(D, 7, 100, 8, SF, 1, 0, 5, D, I, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_resample_means_f64(D, 8, 100, 8, 2, 1, 0, 5, D, I, nullptr), RR_ERR_ARG, __LINE__);
  expect(rr_resample_means_f64(D, 8, 100, 8, -1, 1, 0, 5, D, I, nullptr), RR_ERR_ARG, __LINE__);
  // limits
  expect(rr_resample_means_f64(D, 33, 100, RR_RESAMPLE_MAX_COLS + 1, B0, 1, 0, 5, D, I, nullptr), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_resample_means_f64(D, 8, (1LL << 20) + 1, 8, B0, 1, 0, 5, D, I, nullptr), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_resample_means_f64(D, 8, 4, 8, B0, 1, (1LL << 61) - 5, 5, D, I, nullptr), RR_ERR_UNSUPPORTED, __LINE__);       // == 2^63
  expect(rr_resample_means_f64(D, 8, 3, 8, SF, 1, 1LL << 62, 1LL << 62, D, I, nullptr), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_resample_means_f64(D, 8, 3, 8, SF, 1, INT64_MAX, INT64_MAX, D, I, nullptr), RR_ERR_UNSUPPORTED, __LINE__);
  expect(rr_resample_means_f64(D, 8, 1LL << 20, 8, B0, 1, 1LL << 43, 1, D, I, nullptr), RR_ERR_UNSUPPORTED, __LINE__);
  // B == 0 launches nothing: right below every limit, with and without counts, without a table when Q == 0
  for (int mode : {B0, SF})
    for (int64_t Q : {0LL, 1LL, 2LL, 63LL, 64LL, 65LL, 1LL << 20})
      for (int M : {1, 3, 16, RR_RESAMPLE_MAX_COLS})
        for (int b : {0, 1, 7, 4096}) {
          expect(rr_resample_set_blocks(b), RR_OK, __LINE__);
          expect(rr_resample_blocks(), b, __LINE__);
          const int64_t Qe = (Q + 1) & ~1LL;
          const int64_t b0 = Qe ? (INT64_MAX / Qe) : INT64_MAX;       // the largest start: b0 * Qe < 2^63
          expect(rr_resample_means_f64(Q ? D : nullptr, M, Q, M, mode, 1, b0, 0, D, b ? I : nullptr, nullptr), RR_OK, __LINE__);
          if (Qe) expect(rr_resample_means_f64(D, M, Q, M, mode, 1, b0, 1, D, I, nullptr), RR_ERR_UNSUPPORTED, __LINE__);
        }
  expect(rr_resample_set_blocks(-1), RR_ERR_ARG, __LINE__);
  expect(rr_resample_set_blocks(4097), RR_ERR_ARG, __LINE__);
  expect(rr_resample_blocks(), 4096, __LINE__);
  expect(rr_resample_set_blocks(0), RR_OK, __LINE__);
  // the draw stream
  int n = 0;
  for (const Draw& d : kDraws) {
    const uint32_t got = rr_resample_draw_host(d.seed, d.j);
    if (got != d.want) { std::printf("draw(%llu, %llu) = %u, want %u\n", (unsigned long long)d.seed, (unsigned long long)d.j, got, d.want); ++bad; }
    ++n;
  }
  std::printf("%d draws checked\n", n);
  std::printf("%s\n", bad ? "FAILED" : "host checks clean");
  return bad != 0;
}
