// Per-query rank correlation: Kendall's tau-b, Spearman's rho, the reciprocal rank and the top-1 regret of
// every list of a window in one launch (rr_rank_correlation_f32).  A definition of this library, not a port.
//
// Definitions.  A pair (i, j) is ORDERED in a key only where > or < holds; where neither holds it is TIED in that key, so a NaN
// is tied with everything: it changes values and never addresses.  Over the C (C - 1) / 2 unordered pairs of a list
//   P  ordered the same way in score and target      D  ordered in both, the opposite way
//   X  tied in score only                            Y  tied in target only
//   tau-b = (P - D) / sqrt((P + D + X) (P + D + Y))
// Spearman's rho is Pearson's r of the tie-averaged ranks.  With
//   a_i = 2 (1 + #{s_j > s_i}) + #{j != i : neither < nor >} - (C + 1)  =  #{s_j > s_i} - #{s_j < s_i}
// the centred, doubled tie-averaged rank of i by score - an integer, summing to 0 over the list - and b_i the same on the targets
//   rho = sum a_i b_i / sqrt(sum a_i^2 sum b_i^2).
// The first maximum of a key is the lowest position that no other candidate is greater than (rank 0 of the stable descending
// order, ties by list position: rr_ranking_metrics_f32's `order`); the reciprocal rank is 1 / (1 + stable descending score
// rank of the target's first maximum) and the regret is t[first maximum of t] - t[first maximum of s].
// Every count and each of the three Spearman sums is accumulated as an integer: a lane's 32-bit pair counters hold at most
// 8191 per candidate, and the 64-bit sums at most C^3 = 5.5e11 at C = 8192, exact in int64 and in a double.  Only the final
// quotients and square roots are float64 - IEEE operations, the build has no fast-math and -ffp-contract=off - formed by ONE
// thread from the reduced integers, so the one-wave and four-wave forms write identical bits.  tau-b and rho are NaN where a key
// is constant (a zero denominator, as scipy), so for C < 2; a list of one has reciprocal rank 1, regret 0 and counts 0; an
// empty list writes NaN to stats 0..3 and 0 to stats 4..7.
//
// One workgroup owns one query: one wavefront when the window's longest list has at most 64 candidates, four above.  Thread =
// candidate i, strided over the workgroup; a thread walks ALL j of the list from LDS, four at a time (16-byte broadcast
// reads), and one pass yields #greater and #less of i in both keys and its concordant and discordant partners - the pair
// classes doubled, halved after the reduction.  The stable rank is needed for one candidate only (the target's first maximum)
// and is counted by the whole workgroup after the pass.  Phases, the barriers between them and outside every loop:
//   1  stage s and t
//   2  the pass over all pairs; per thread seven int64 sums and the two first maxima
//   3  the workgroup's reduction in a fixed order (wave shuffles, then the four waves' partials from LDS)
//   4  the score rank of the target's first maximum, reduced likewise; thread 0 writes the eight statistics
// LDS: s and t, 8 bytes per candidate, and 320 bytes of cross-wave scratch - just over 64 KiB at 8,192 candidates.  No atomics,
// no store to an address that depends on a comparison.
#include "wave_util.h"

namespace {

WaveKnob g_knob;                     // rr_rank_correlation_set_waves

constexpr int kSums = 9;             // 2P, 2D, 2X, 2Y, sum ab, sum aa, sum bb, first maximum of t, first maximum of s
constexpr int kScratch = 4 * (kSums + 1) * sizeof(long long);      // four waves' partials of phase 3 and of phase 4

struct PairCounts {
  int gs, ls, gt, lt, conc, disc;
};

__device__ inline void count_pair(float sj, float tj, float si, float ti, PairCounts& n) {
  const bool sg = sj > si, sl = sj < si, tg = tj > ti, tl = tj < ti;
  n.gs += sg ? 1 : 0;
  n.ls += sl ? 1 : 0;
  n.gt += tg ? 1 : 0;
  n.lt += tl ? 1 : 0;
  n.conc += ((sg && tg) || (sl && tl)) ? 1 : 0;
  n.disc += ((sg && tl) || (sl && tg)) ? 1 : 0;
}

template <int NW>
__global__ void __launch_bounds__(NW * RR_WAVE) rank_corr_kernel(const float* __restrict__ score, int64_t sstride,
                                                                  const float* __restrict__ targets,
                                                                  const int32_t* __restrict__ seg_off, int L,
                                                                  double* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int NT = NW * RR_WAVE;
  const int q = blockIdx.x, tid = threadIdx.x;
  const int off = seg_off[q], C = seg_off[q + 1] - off;
  double* st = stats + static_cast<int64_t>(q) * RR_RANK_CORR_NSTATS;
  if (C <= 0) {                                                    // workgroup-uniform, before any barrier
    if (tid < RR_RANK_CORR_NSTATS) st[tid] = tid < 4 ? static_cast<double>(NAN) : 0.0;
    return;
  }
  float* s = sm;
  float* t = sm + L;
  long long* red = reinterpret_cast<long long*>(sm + 2 * L);       // L % 4 == 0: 32-byte aligned
  long long* red2 = red + 4 * kSums;

  for (int i = tid; i < C; i += NT) {
    s[i] = score[static_cast<int64_t>(off + i) * sstride];
    t[i] = targets[off + i];
  }
  __syncthreads();

  long long v[kSums] = {0, 0, 0, 0, 0, 0, 0, C, C};
  const int C4 = C & ~3;
  for (int i = tid; i < C; i += NT) {
    const float si = s[i], ti = t[i];
    PairCounts n{};
    for (int j = 0; j < C4; j += 4) {
      const float4 s4 = *reinterpret_cast<const float4*>(s + j);
      const float4 t4 = *reinterpret_cast<const float4*>(t + j);
      count_pair(s4.x, t4.x, si, ti, n);
      count_pair(s4.y, t4.y, si, ti, n);
      count_pair(s4.z, t4.z, si, ti, n);
      count_pair(s4.w, t4.w, si, ti, n);
    }
    for (int j = C4; j < C; ++j) count_pair(s[j], t[j], si, ti, n);
    const int both = n.conc + n.disc;                              // the partners ordered in both keys
    v[0] += n.conc;
    v[1] += n.disc;
    v[2] += n.gt + n.lt - both;                                    // ordered in the target, tied in the score
    v[3] += n.gs + n.ls - both;
    const long long a = n.gs - n.ls, b = n.gt - n.lt;
    v[4] += a * b;
    v[5] += a * a;
    v[6] += b * b;
    if (n.gt == 0 && i < v[7]) v[7] = i;                           // nothing greater: a maximum (or a NaN)
    if (n.gs == 0 && i < v[8]) v[8] = i;
  }

#pragma unroll
  for (int k = 0; k < kSums; ++k) v[k] = k < 7 ? rr_wave_sum(v[k]) : rr_wave_min(v[k]);
  if constexpr (NW > 1) {
    if ((tid & (RR_WAVE - 1)) == 0) {
#pragma unroll
      for (int k = 0; k < kSums; ++k) red[(tid / RR_WAVE) * kSums + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kSums; ++k) {
      const long long w0 = red[k], w1 = red[kSums + k], w2 = red[2 * kSums + k], w3 = red[3 * kSums + k];
      if (k < 7) {
        v[k] = (w0 + w1) + (w2 + w3);
      } else {
        const long long lo = w0 < w1 ? w0 : w1, hi = w2 < w3 ? w2 : w3;
        v[k] = lo < hi ? lo : hi;
      }
    }
  }

  // every list of C >= 1 has a candidate that nothing is greater than, so both positions are below C
  const int it = static_cast<int>(v[7]), is = static_cast<int>(v[8]);
  const float sx = s[it];
  long long rank = 0;
  for (int j = tid; j < C; j += NT) rank += rr_precedes(s[j], j, sx, it) ? 1 : 0;
  rank = rr_wave_sum(rank);
  if constexpr (NW > 1) {
    if ((tid & (RR_WAVE - 1)) == 0) red2[tid / RR_WAVE] = rank;
    __syncthreads();
    rank = (red2[0] + red2[1]) + (red2[2] + red2[3]);
  }

  if (tid == 0) {
    const double P = static_cast<double>(v[0] / 2), D = static_cast<double>(v[1] / 2);
    const double X = static_cast<double>(v[2] / 2), Y = static_cast<double>(v[3] / 2);
    const double dt = (P + D + X) * (P + D + Y);                   // < 2^53: exact
    const double dr = static_cast<double>(v[5]) * static_cast<double>(v[6]);
    st[0] = dt > 0.0 ? (P - D) / sqrt(dt) : static_cast<double>(NAN);
    st[1] = dr > 0.0 ? static_cast<double>(v[4]) / sqrt(dr) : static_cast<double>(NAN);
    st[2] = 1.0 / (1.0 + static_cast<double>(rank));
    st[3] = static_cast<double>(t[it]) - static_cast<double>(t[is]);
    st[4] = P;
    st[5] = D;
    st[6] = X;
    st[7] = Y;
  }
}

}  // namespace

extern "C" {

int rr_rank_correlation_waves(void) { return g_knob.waves; }
int rr_rank_correlation_set_waves(int waves) { return g_knob.set(waves); }

int rr_rank_correlation_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q,
                            int max_len, double* stats, rr_stream_t stream) {
  RR_CHECK_ARG(list_args_ok(score, targets, seg_off, Q, max_len) && score_stride >= 1 && stats);
  if (max_len > kMaxLen) return RR_ERR_UNSUPPORTED;
  const int L = list_words4(max_len);
  return launch_waves(rank_corr_kernel<1>, rank_corr_kernel<4>, g_knob.pick(max_len), Q, L * 2 * sizeof(float) + kScratch,
                      static_cast<hipStream_t>(stream), score, score_stride, targets, seg_off, L, stats);
}

}  // extern "C"
