// LambdaRank: RankNet's pair cost with every pair weighted by the |delta NDCG| of swapping the two candidates in the
// current predicted order.  It is a definition of this library, not a port: the reference trainer has no
// such loss.
//
// One 64-lane wavefront owns one query, staged in LDS in the list kernels' five-array layout (carve, loss_list.h):
//   s, t        the scores and targets as given
//   D           the discount of every candidate at its predicted rank, 1 / log2(1 + r_i) for r_i <= k, else 0
//   gn          its gain over the ideal DCG, exp(t_i - max t) / maxDCG
//   lam         the candidate's lambda until the query's pair count is known (RankNet's scratch)
// Both rankings are counting passes (rank_sort's rule: descending, ties by list position); nothing is scattered by rank,
// so no comparison outcome can move a store.  The O(C) quantities - gains, discounts, maxDCG - are evaluated in double and
// stored as floats; a pair's weight, cost and lambda are float expressions; the sums over a candidate's pairs and over the
// query are accumulated in double (a lane adds up to 2^20 terms of a list of 8192) and rounded once.  The weights are
// constants: no gradient flows through them.  Only wave-level synchronisation, no float atomics; per-query partials
// [2 * Q] (loss as a float, ordered pairs as an int32 - RankNet's layout) are finished by finish_counted (loss_list.h, the
// finish RankNet and ApproxNDCG share), in a second launch (fwd) or by the workgroup that arrives last (step), so the bits
// are the same on every run and in both forms.
#include "loss_list.h"

namespace {

// Ranks, discounts and normalised gains of the staged query; returns the number of pairs with t_i > t_j (wave-uniform).
__device__ inline int lambdarank_prepare(const float* s, const float* t, float* D, float* gn, int C, int k, int lane) {
  const float tmax = list_max(t, C, lane);
  double dcg = 0.0;
  int npos = 0;
  for (int i = lane; i < C; i += RR_WAVE) {
    const float si = s[i], ti = t[i];
    int rp = 0, rt = 0;                                             // 0-based ranks by score and by target
    for (int j = 0; j < C; ++j) {
      const float sj = s[j], tj = t[j];
      rp += rr_precedes(sj, j, si, i) ? 1 : 0;
      rt += rr_precedes(tj, j, ti, i) ? 1 : 0;
      npos += (ti > tj) ? 1 : 0;
    }
    const double g = exp(static_cast<double>(ti) - static_cast<double>(tmax));
    D[i] = rp < k ? static_cast<float>(1.0 / log2(static_cast<double>(rp) + 2.0)) : 0.f;
    // the ideal position of a candidate is its target rank (tied targets have equal gains): no sort
    if (rt < k) dcg += g / log2(static_cast<double>(rt) + 2.0);
    gn[i] = static_cast<float>(g);
  }
  dcg = rr_wave_sum(dcg);                                           // >= 1: the best target has gain 1 at position 1
  npos = rr_wave_sum(npos);
  for (int i = lane; i < C; i += RR_WAVE) gn[i] = static_cast<float>(static_cast<double>(gn[i]) / dcg);
  wave_sync();
  return npos;
}

// sum_{i != j} w_ij C_ij (LOSS; the wave's sum, valid in every lane) and lam[i] = sum_j w_ij lambda_ij (GRAD).  One
// exponential per pair serves the cost and the lambda: with y the margin in the pair's favoured direction and e =
// exp(-|y|), softplus(-y) = max(-y, 0) + log1p(e) and sigmoid(-y) = y >= 0 ? e / (1 + e) : 1 / (1 + e).  A pair of weight
// zero (equal gains, or both below the truncation) is skipped before any transcendental.
template <bool LOSS, bool GRAD>
__device__ inline double lambdarank_pairs(const float* s, const float* t, const float* D, const float* gn, float* lam, int C,
                                          float sigma, int lane) {
  double acc = 0.0;
  for (int i = lane; i < C; i += RR_WAVE) {
    const float si = s[i], ti = t[i], Di = D[i], gi = gn[i];
    double li = 0.0;
    for (int j = 0; j < C; ++j) {
      const float tj = t[j];
      const float w = fabsf(gi - gn[j]) * fabsf(Di - D[j]);
      if (ti != tj && w > 0.f) {
        const bool up = ti > tj;
        const float x = sigma * (si - s[j]);
        const float y = up ? x : -x;
        const float e = expf(-fabsf(y));
        if constexpr (LOSS) acc += static_cast<double>(w * (fmaxf(-y, 0.f) + log1pf(e)));
        if constexpr (GRAD) {
          const float p = 1.0f / (1.0f + e);
          const float sg = y >= 0.f ? e * p : p;
          li += static_cast<double>(w * (up ? -sigma * sg : sigma * sg));
        }
      }
    }
    if constexpr (GRAD) lam[i] = static_cast<float>(li);
  }
  return LOSS ? rr_wave_sum(acc) : 0.0;
}

// MODE 0: forward (partial).  MODE 1: backward (dscore = gloss[0] * d loss_sum / d score).  MODE 2: step - both, for the
// upstream gradient `scale`, and the last workgroup to arrive finishes loss = scale * loss_sum and the pair count.
template <int MODE>
__global__ void __launch_bounds__(RR_WAVE) lambdarank_kernel(const float* __restrict__ score, int64_t sstride,
                                                             const float* __restrict__ targets,
                                                             const int32_t* __restrict__ seg_off, int L, float sigma,
                                                             int ndcg_k, float* __restrict__ partial,
                                                             const float* __restrict__ gloss, float scale,
                                                             float* __restrict__ dscore, int64_t dstride,
                                                             float* __restrict__ loss, int64_t* __restrict__ pairs,
                                                             unsigned int* __restrict__ counter) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int q = blockIdx.x, lane = threadIdx.x;
  const int off = seg_off[q], C = seg_off[q + 1] - off;
  int tot = 0;
  double acc = 0.0;
  if (C > 0) {
    const ListView v = carve(sm, L);
    float* D = v.ss;
    float* gn = reinterpret_cast<float*>(v.perm);
    float* lam = v.aux;
    for (int i = lane; i < C; i += RR_WAVE) {
      v.s[i] = score[static_cast<int64_t>(off + i) * sstride];
      v.t[i] = targets[off + i];
    }
    wave_sync();
    const int k = (ndcg_k == 0 || ndcg_k > C) ? C : ndcg_k;
    tot = lambdarank_prepare(v.s, v.t, D, gn, C, k, lane);
    if (tot > 0) acc = lambdarank_pairs<MODE != 1, MODE != 0>(v.s, v.t, D, gn, lam, C, sigma, lane);
    if constexpr (MODE != 0) {
      // w and C are symmetric in (i, j), so d (sum_ij w_ij C_ij) / d s_i = 2 * lam_i; a pair-less query writes zeros
      const float g = (MODE == 1 ? gloss[0] : scale) * 2.0f;
      for (int i = lane; i < C; i += RR_WAVE) dscore[static_cast<int64_t>(off + i) * dstride] = tot > 0 ? g * lam[i] : 0.f;
    }
  }
  if constexpr (MODE != 1) {
    if (lane == 0) {
      partial[2 * q] = tot > 0 ? static_cast<float>(acc) : 0.f;
      reinterpret_cast<int32_t*>(partial)[2 * q + 1] = 2 * tot;     // ordered pairs, as RankNet counts them
    }
  }
  if constexpr (MODE == 2) {
    const int n = gridDim.x;
    if (arrive_last(n, counter, lane)) {
      finish_counted(partial, n, scale, loss, pairs, lane);
      if (lane == 0) *counter = 0u;
    }
  }
}

inline bool lambdarank_args_ok(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q,
                               int max_len, float sigma, int ndcg_k) {
  return list_args_ok(score, targets, seg_off, Q, max_len) && score_stride >= 1 && sigma > 0.f && ndcg_k >= 0;
}

template <int MODE>
int lambdarank_launch(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q, int max_len,
                      float sigma, int ndcg_k, float* partial, const float* gloss, float scale, float* dscore,
                      int64_t dscore_stride, float* loss, int64_t* pairs, unsigned int* counter, hipStream_t s) {
  const int L = list_words(max_len);
  return launch_per_query(lambdarank_kernel<MODE>, Q, L, 5 * sizeof(float), RR_WAVE, s, score, score_stride, targets, seg_off, L,
                          sigma, ndcg_k, partial, gloss, scale, dscore, dscore_stride, loss, pairs, counter);
}

}  // namespace

extern "C" {

int rr_lambdarank_fwd_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q,
                          int max_len, float sigma, int ndcg_k, float* loss_sum, int64_t* pairs, float* partial,
                          rr_stream_t stream) {
  RR_CHECK_ARG(lambdarank_args_ok(score, score_stride, targets, seg_off, Q, max_len, sigma, ndcg_k) && loss_sum && pairs && partial);
  if (max_len > kMaxLen) return RR_ERR_UNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int st = lambdarank_launch<0>(score, score_stride, targets, seg_off, Q, max_len, sigma, ndcg_k, partial, nullptr, 0.f,
                                      nullptr, 1, nullptr, nullptr, nullptr, s);
  if (st != RR_OK) return st;
  finish_counted_kernel<<<1, RR_WAVE, 0, s>>>(partial, Q, 1.0f, loss_sum, pairs);
  return rr_launch_status();
}

int rr_lambdarank_bwd_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q,
                          int max_len, float sigma, int ndcg_k, const float* gloss, float* dscore, int64_t dscore_stride,
                          rr_stream_t stream) {
  RR_CHECK_ARG(lambdarank_args_ok(score, score_stride, targets, seg_off, Q, max_len, sigma, ndcg_k) && gloss && dscore &&
               dscore_stride >= 1);
  if (max_len > kMaxLen) return RR_ERR_UNSUPPORTED;
  return lambdarank_launch<1>(score, score_stride, targets, seg_off, Q, max_len, sigma, ndcg_k, nullptr, gloss, 0.f, dscore,
                              dscore_stride, nullptr, nullptr, nullptr, static_cast<hipStream_t>(stream));
}

int rr_lambdarank_step_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q,
                           int max_len, float sigma, int ndcg_k, float scale, float* loss, int64_t* pairs, float* partial,
                           unsigned int* counter, float* dscore, int64_t dscore_stride, rr_stream_t stream) {
  RR_CHECK_ARG(lambdarank_args_ok(score, score_stride, targets, seg_off, Q, max_len, sigma, ndcg_k) && loss && pairs && partial &&
               counter && dscore && dscore_stride >= 1);
  if (max_len > kMaxLen) return RR_ERR_UNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (Q == 0) {                                          // nothing to rank: the zero loss and pair count of the forward entry
    finish_counted_kernel<<<1, RR_WAVE, 0, s>>>(partial, 0, scale, loss, pairs);
    return rr_launch_status();
  }
  return lambdarank_launch<2>(score, score_stride, targets, seg_off, Q, max_len, sigma, ndcg_k, partial, nullptr, scale, dscore,
                              dscore_stride, loss, pairs, counter, s);
}

}  // extern "C"
