// Soft ranks and ApproxNDCG: every hard rank is replaced by the differentiable
//   r_i = 1 + sum_{j != i} sigmoid((s_j - s_i) / T)
// and NDCG - gains exp(target), the metric ranking_metrics reports - is written on those ranks, so the loss is one minus a
// smooth NDCG and its gradient flows through the ranks.  A definition of this library, not a port; the formulas are in
// include/reactranker_hip.h (rr_soft_rank_fwd_f32, rr_approx_ndcg_fwd_f32).
//
// One workgroup owns one query: one wavefront when the window's longest list has at most 64 candidates, four (256 threads,
// one per SIMD of the CU) above that.  Thread = candidate i, strided over the workgroup; a thread walks ALL j of its own
// candidates, four at a time (16-byte LDS broadcast reads), so no per-candidate sum is ever shared between threads and the
// workgroup barriers stand between the phases only, outside every data-dependent loop:
//   1  stage s and t                                                    s, t
//   2  r_i and the target rank of i (a counting pass, as LambdaRank)    g_i, psi(r_i), psi'(r_i)
//   3  maxDCG; G_i = g_i / maxDCG, loss_q, a_i = -G_i psi'(r_i)         a_i over psi'
//   4  d / d s_k = (1 / T) sum_j sigmoid'(u_kj) (a_j - a_k)
// Five arrays of L words: 20 bytes per candidate, all 160 KiB of a CU at 8,192 candidates.  The cross-wave sums therefore
// have no LDS of their own: they borrow the head of an array that is not live at that point (block_reduce).
// Arithmetic: a pair's margin, its one expf and the sigmoid or its derivative in the e = exp(-|u|) form are float32; the sums
// over j, the O(C) quantities (gain, log2, gate, psi', maxDCG - each stored once as a float) and the loss sum are float64.
// No float atomics and no store behind a comparison: ties, NaNs and unranked queries change values, never addresses.
// The per-query partials [2 * Q] (loss as a float, ranked as an int32) are finished by finish_counted (loss_list.h, the finish
// RankNet and LambdaRank share) in a second launch (fwd) or by the workgroup that arrives last (step): the same bits on every
// run and in both forms.
#include "loss_list.h"

namespace {

enum Mode { RANK_FWD, RANK_BWD, NDCG_FWD, NDCG_BWD, NDCG_STEP, NDCG_A };

constexpr bool is_ndcg(int mode) { return mode >= NDCG_FWD; }
constexpr int lds_arrays(int mode) { return mode == RANK_FWD ? 1 : (mode == RANK_BWD ? 2 : 5); }

WaveKnob g_knob;                     // rr_approx_ndcg_set_waves

struct SumF64 {
  __device__ static double wave(double v) { return rr_wave_sum(v); }
  __device__ static double join(double a, double b) { return a + b; }
};
struct MaxF64 {
  __device__ static double wave(double v) { return rr_wave_max(v); }
  __device__ static double join(double a, double b) { return fmax(a, b); }
};

// The workgroup's reduction of v in a fixed order, valid in every thread.  `red` is NW doubles of LDS that no thread uses
// for anything else between the first barrier and the last.  Reached by every thread of the workgroup; one wave needs
// neither the scratch nor a barrier.
template <typename Op, int NW>
__device__ inline double block_reduce(double v, double* red, int tid) {
  v = Op::wave(v);
  if constexpr (NW > 1) {
    __syncthreads();
    if ((tid & (RR_WAVE - 1)) == 0) red[tid / RR_WAVE] = v;
    __syncthreads();
    v = Op::join(Op::join(red[0], red[1]), Op::join(red[2], red[3]));
    __syncthreads();
  }
  return v;
}

// sigmoid(u) from e = exp(-|u|): 1 / (1 + e) for u >= 0, e / (1 + e) below
__device__ inline float sigmoid_e(float u) {
  const float e = expf(-fabsf(u));
  const float p = 1.0f / (1.0f + e);
  return u >= 0.f ? p : e * p;
}

// sigmoid'(u) = e / (1 + e)^2 (even in u).  Not sigmoid (1 - sigmoid): 1 - sigmoid cancels for large |u| / small T.
__device__ inline float dsigmoid_e(float u) {
  const float e = expf(-fabsf(u));
  const float d = 1.0f + e;
  return e / (d * d);
}

// r_i of candidate i over the staged scores and, with RT, the 0-based rank of its target (descending, ties by position).
template <bool RT>
__device__ inline double soft_rank_of(const float* s, const float* t, int C, int i, float inv_t, int* rt_out) {
  const float si = s[i];
  const float ti = RT ? t[i] : 0.f;
  const int C4 = C & ~3;
  double r = 1.0;
  int rt = 0;
  for (int j = 0; j < C4; j += 4) {
    const float4 s4 = *reinterpret_cast<const float4*>(s + j);
    float f0 = sigmoid_e((s4.x - si) * inv_t);
    float f1 = sigmoid_e((s4.y - si) * inv_t);
    float f2 = sigmoid_e((s4.z - si) * inv_t);
    float f3 = sigmoid_e((s4.w - si) * inv_t);
    f0 = j == i ? 0.f : f0;
    f1 = j + 1 == i ? 0.f : f1;
    f2 = j + 2 == i ? 0.f : f2;
    f3 = j + 3 == i ? 0.f : f3;
    r += (static_cast<double>(f0) + static_cast<double>(f1)) + (static_cast<double>(f2) + static_cast<double>(f3));
    if constexpr (RT) {                                            // rr_precedes, written out: the call costs NDCG_A two SGPRs
      const float4 t4 = *reinterpret_cast<const float4*>(t + j);
      rt += (t4.x > ti || (t4.x == ti && j < i)) ? 1 : 0;
      rt += (t4.y > ti || (t4.y == ti && j + 1 < i)) ? 1 : 0;
      rt += (t4.z > ti || (t4.z == ti && j + 2 < i)) ? 1 : 0;
      rt += (t4.w > ti || (t4.w == ti && j + 3 < i)) ? 1 : 0;
    }
  }
  for (int j = C4; j < C; ++j) {
    const float f = sigmoid_e((s[j] - si) * inv_t);
    r += j == i ? 0.0 : static_cast<double>(f);
    if constexpr (RT) rt += rr_precedes(t[j], j, ti, i) ? 1 : 0;
  }
  if constexpr (RT) *rt_out = rt;
  return r;
}

// sum_j sigmoid'(u_kj) (a_j - a_k); the j == k term is zero by itself.  The caller divides by T.
__device__ inline double rank_grad_of(const float* s, const float* a, int C, int k, float inv_t) {
  const float sk = s[k], ak = a[k];
  const int C4 = C & ~3;
  double acc = 0.0;
  for (int j = 0; j < C4; j += 4) {
    const float4 s4 = *reinterpret_cast<const float4*>(s + j);
    const float4 a4 = *reinterpret_cast<const float4*>(a + j);
    const float f0 = dsigmoid_e((s4.x - sk) * inv_t) * (a4.x - ak);
    const float f1 = dsigmoid_e((s4.y - sk) * inv_t) * (a4.y - ak);
    const float f2 = dsigmoid_e((s4.z - sk) * inv_t) * (a4.z - ak);
    const float f3 = dsigmoid_e((s4.w - sk) * inv_t) * (a4.w - ak);
    acc += (static_cast<double>(f0) + static_cast<double>(f1)) + (static_cast<double>(f2) + static_cast<double>(f3));
  }
  for (int j = C4; j < C; ++j) acc += static_cast<double>(dsigmoid_e((s[j] - sk) * inv_t) * (a[j] - ak));
  return acc;
}

// psi(r) = gate(r) / log2(1 + r) and its derivative; gate(r) = sigmoid(k + 1/2 - r) when the NDCG is truncated inside the
// list, else 1.  r >= 1, so log2(1 + r) >= 1.
__device__ inline void psi_of(double r, int k, bool gated, double* psi, double* dpsi) {
  const double l2 = log2(1.0 + r);
  const double dl2 = 1.0 / ((1.0 + r) * 0.69314718055994530942);
  double sg = 1.0, dsg = 0.0;
  if (gated) {
    const double z = static_cast<double>(k) + 0.5 - r;
    const double e = exp(-fabs(z));
    const double d = 1.0 + e;
    sg = z >= 0.0 ? 1.0 / d : e / d;
    dsg = e / (d * d);
  }
  *psi = sg / l2;
  *dpsi = -dsg / l2 - sg * dl2 / (l2 * l2);                        // d gate / d r = -sigmoid'(z)
}

struct ApproxArgs {
  const float* score;      // [M] with stride sstride
  int64_t sstride;
  const float* targets;    // NDCG modes
  const int32_t* seg_off;
  int L;                   // words per LDS array: a multiple of 4, >= 8, >= the longest list
  float temperature;
  int ndcg_k;
  const float* up;         // RANK_BWD: d L / d rank, stride ustride.  NDCG_BWD: gloss[1]
  int64_t ustride;
  float scale;             // NDCG_STEP: the upstream gradient, and the factor of the loss
  float* out;              // RANK_FWD: rank.  RANK_BWD, NDCG_BWD, NDCG_STEP: dscore.  NDCG_A: a.  Stride ostride
  int64_t ostride;
  float* partial;          // NDCG_FWD, NDCG_STEP: [2 * Q]
  float* loss;             // NDCG_STEP
  int64_t* ranked;
  unsigned int* counter;
};

template <int MODE, int NW>
__global__ void __launch_bounds__(NW * RR_WAVE) approx_ndcg_kernel(const ApproxArgs p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int NT = NW * RR_WAVE;
  constexpr bool GRAD = MODE == RANK_BWD || MODE == NDCG_BWD || MODE == NDCG_STEP;
  const int q = blockIdx.x, tid = threadIdx.x;
  const int off = p.seg_off[q], C = p.seg_off[q + 1] - off;
  const float inv_t = 1.0f / p.temperature;
  float* s = sm;
  float* t = sm + p.L;                                             // RANK_BWD: the upstream gradient
  float* gn = sm + 2 * p.L;
  float* psi = sm + 3 * p.L;
  float* a = is_ndcg(MODE) ? sm + 4 * p.L : t;

  for (int i = tid; i < C; i += NT) {
    s[i] = p.score[static_cast<int64_t>(off + i) * p.sstride];
    if constexpr (is_ndcg(MODE)) t[i] = p.targets[off + i];
    if constexpr (MODE == RANK_BWD) t[i] = p.up[static_cast<int64_t>(off + i) * p.ustride];
  }
  __syncthreads();

  if constexpr (MODE == RANK_FWD) {
    for (int i = tid; i < C; i += NT)
      p.out[static_cast<int64_t>(off + i) * p.ostride] = static_cast<float>(soft_rank_of<false>(s, nullptr, C, i, inv_t, nullptr));
  }

  bool ranked = false;
  double loss_q = 0.0;
  if constexpr (is_ndcg(MODE)) {
    // ranked: some t_i > t_j (RankNet's pairs_q > 0).  The scratch of the two reductions is the head of `a`, not yet written.
    double hi = -INFINITY, lo = -INFINITY;
    for (int i = tid; i < C; i += NT) {
      hi = fmax(hi, static_cast<double>(t[i]));
      lo = fmax(lo, -static_cast<double>(t[i]));
    }
    hi = block_reduce<MaxF64, NW>(hi, reinterpret_cast<double*>(a), tid);
    lo = block_reduce<MaxF64, NW>(lo, reinterpret_cast<double*>(a), tid);
    ranked = hi > -lo;                                             // workgroup-uniform
    if (ranked) {
      const int k = (p.ndcg_k == 0 || p.ndcg_k > C) ? C : p.ndcg_k;
      const bool gated = k < C;
      double dcg = 0.0;
      for (int i = tid; i < C; i += NT) {
        int rt;
        const double r = soft_rank_of<true>(s, t, C, i, inv_t, &rt);
        const double g = exp(static_cast<double>(t[i]) - hi);
        // the ideal position of a candidate is its target rank (tied targets have equal gains): no sort
        dcg += rt < k ? g / log2(static_cast<double>(rt) + 2.0) : 0.0;
        double ps, dps;
        psi_of(r, k, gated, &ps, &dps);
        gn[i] = static_cast<float>(g);
        psi[i] = static_cast<float>(ps);
        a[i] = static_cast<float>(dps);
      }
      // the targets are dead once every thread is past the loop above, which the reduction's first barrier says
      dcg = block_reduce<SumF64, NW>(dcg, reinterpret_cast<double*>(t), tid);   // >= 1: the best target has gain 1 at position 1
      double dot = 0.0;
      for (int i = tid; i < C; i += NT) {
        const double G = static_cast<double>(gn[i]) / dcg;
        dot += G * static_cast<double>(psi[i]);
        a[i] = static_cast<float>(-G * static_cast<double>(a[i]));
      }
      loss_q = 1.0 - block_reduce<SumF64, NW>(dot, reinterpret_cast<double*>(t), tid);
      __syncthreads();                                             // a is complete before any thread walks it
    }
    if constexpr (MODE == NDCG_A) {
      for (int i = tid; i < C; i += NT) p.out[static_cast<int64_t>(off + i) * p.ostride] = ranked ? a[i] : 0.f;
    }
  }

  if constexpr (GRAD) {
    const float g = MODE == NDCG_BWD ? p.up[0] : (MODE == NDCG_STEP ? p.scale : 1.0f);
    for (int k = tid; k < C; k += NT) {
      float d = 0.f;                                               // an unranked query writes zeros
      if (MODE == RANK_BWD || ranked) {
        const double acc = rank_grad_of(s, a, C, k, inv_t);
        d = static_cast<float>(static_cast<double>(g) * (acc / static_cast<double>(p.temperature)));
      }
      p.out[static_cast<int64_t>(off + k) * p.ostride] = d;
    }
  }

  if constexpr (MODE == NDCG_FWD || MODE == NDCG_STEP) {
    if (tid == 0) {
      p.partial[2 * q] = ranked ? static_cast<float>(loss_q) : 0.f;
      reinterpret_cast<int32_t*>(p.partial)[2 * q + 1] = ranked ? 1 : 0;
    }
  }
  if constexpr (MODE == NDCG_STEP) {
    // the first wave alone draws the ticket: its lane 0 wrote this query's partial, which is all the finish reads
    if (tid < RR_WAVE) {
      const int n = gridDim.x;
      if (arrive_last(n, p.counter, tid)) {
        finish_counted(p.partial, n, p.scale, p.loss, p.ranked, tid);
        if (tid == 0) *p.counter = 0u;
      }
    }
  }
}

// positive and finite, and so is its float32 reciprocal, which the kernels multiply the margins by: below 1 / FLT_MAX
// (2.94e-39, inside the subnormals) the reciprocal is inf and a tie's 0 * inf would be NaN
inline bool temperature_ok(float temperature) {
  return temperature > 0.f && temperature < INFINITY && 1.0f / temperature < INFINITY;
}

template <int MODE>
int approx_launch(ApproxArgs a, int Q, int max_len, hipStream_t s) {
  a.L = max_len > 8 ? list_words4(max_len) : 8;                    // float4 reads; 4 doubles of reduction scratch
  return launch_waves(approx_ndcg_kernel<MODE, 1>, approx_ndcg_kernel<MODE, 4>, g_knob.pick(max_len), Q,
                      a.L * lds_arrays(MODE) * sizeof(float), s, a);
}

inline bool rank_args_ok(const float* score, int64_t score_stride, const int32_t* seg_off, int Q, int max_len, float temperature) {
  return score && seg_off && score_stride >= 1 && Q >= 0 && max_len >= 0 && temperature_ok(temperature);
}

inline bool ndcg_args_ok(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q, int max_len,
                         float temperature, int ndcg_k) {
  return list_args_ok(score, targets, seg_off, Q, max_len) && score_stride >= 1 && temperature_ok(temperature) && ndcg_k >= 0;
}

inline ApproxArgs ndcg_args(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, float temperature,
                            int ndcg_k) {
  ApproxArgs a{};
  a.score = score;
  a.sstride = score_stride;
  a.targets = targets;
  a.seg_off = seg_off;
  a.temperature = temperature;
  a.ndcg_k = ndcg_k;
  a.ustride = a.ostride = 1;
  return a;
}

}  // namespace

extern "C" {

int rr_approx_ndcg_waves(void) { return g_knob.waves; }
int rr_approx_ndcg_set_waves(int waves) { return g_knob.set(waves); }

int rr_soft_rank_fwd_f32(const float* score, int64_t score_stride, const int32_t* seg_off, int Q, int max_len, float temperature,
                         float* rank, int64_t rank_stride, rr_stream_t stream) {
  RR_CHECK_ARG(rank_args_ok(score, score_stride, seg_off, Q, max_len, temperature) && rank && rank_stride >= 1);
  if (max_len > kMaxLen) return RR_ERR_UNSUPPORTED;
  ApproxArgs a = ndcg_args(score, score_stride, nullptr, seg_off, temperature, 0);
  a.out = rank;
  a.ostride = rank_stride;
  return approx_launch<RANK_FWD>(a, Q, max_len, static_cast<hipStream_t>(stream));
}

int rr_soft_rank_bwd_f32(const float* score, int64_t score_stride, const int32_t* seg_off, int Q, int max_len, float temperature,
                         const float* drank, int64_t drank_stride, float* dscore, int64_t dscore_stride, rr_stream_t stream) {
  RR_CHECK_ARG(rank_args_ok(score, score_stride, seg_off, Q, max_len, temperature) && drank && drank_stride >= 1 && dscore &&
               dscore_stride >= 1);
  if (max_len > kMaxLen) return RR_ERR_UNSUPPORTED;
  ApproxArgs a = ndcg_args(score, score_stride, nullptr, seg_off, temperature, 0);
  a.up = drank;
  a.ustride = drank_stride;
  a.out = dscore;
  a.ostride = dscore_stride;
  return approx_launch<RANK_BWD>(a, Q, max_len, static_cast<hipStream_t>(stream));
}

int rr_approx_ndcg_fwd_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q,
                           int max_len, float temperature, int ndcg_k, float* loss_sum, int64_t* ranked, float* partial,
                           rr_stream_t stream) {
  RR_CHECK_ARG(ndcg_args_ok(score, score_stride, targets, seg_off, Q, max_len, temperature, ndcg_k) && loss_sum && ranked && partial);
  if (max_len > kMaxLen) return RR_ERR_UNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  ApproxArgs a = ndcg_args(score, score_stride, targets, seg_off, temperature, ndcg_k);
  a.partial = partial;
  const int st = approx_launch<NDCG_FWD>(a, Q, max_len, s);
  if (st != RR_OK) return st;
  finish_counted_kernel<<<1, RR_WAVE, 0, s>>>(partial, Q, 1.0f, loss_sum, ranked);
  return rr_launch_status();
}

int rr_approx_ndcg_bwd_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q,
                           int max_len, float temperature, int ndcg_k, const float* gloss, float* dscore, int64_t dscore_stride,
                           rr_stream_t stream) {
  RR_CHECK_ARG(ndcg_args_ok(score, score_stride, targets, seg_off, Q, max_len, temperature, ndcg_k) && gloss && dscore &&
               dscore_stride >= 1);
  if (max_len > kMaxLen) return RR_ERR_UNSUPPORTED;
  ApproxArgs a = ndcg_args(score, score_stride, targets, seg_off, temperature, ndcg_k);
  a.up = gloss;
  a.out = dscore;
  a.ostride = dscore_stride;
  return approx_launch<NDCG_BWD>(a, Q, max_len, static_cast<hipStream_t>(stream));
}

int rr_approx_ndcg_step_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q,
                            int max_len, float temperature, int ndcg_k, float scale, float* loss, int64_t* ranked, float* partial,
                            unsigned int* counter, float* dscore, int64_t dscore_stride, rr_stream_t stream) {
  RR_CHECK_ARG(ndcg_args_ok(score, score_stride, targets, seg_off, Q, max_len, temperature, ndcg_k) && loss && ranked && partial &&
               counter && dscore && dscore_stride >= 1);
  if (max_len > kMaxLen) return RR_ERR_UNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (Q == 0) {                                          // nothing to rank: the zero loss and count of the forward entry
    finish_counted_kernel<<<1, RR_WAVE, 0, s>>>(partial, 0, scale, loss, ranked);
    return rr_launch_status();
  }
  ApproxArgs a = ndcg_args(score, score_stride, targets, seg_off, temperature, ndcg_k);
  a.scale = scale;
  a.partial = partial;
  a.loss = loss;
  a.ranked = ranked;
  a.counter = counter;
  a.out = dscore;
  a.ostride = dscore_stride;
  return approx_launch<NDCG_STEP>(a, Q, max_len, s);
}

int rr_approx_ndcg_ranks_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q,
                             int max_len, float temperature, int ndcg_k, float* a_out, int64_t a_stride, rr_stream_t stream) {
  RR_CHECK_ARG(ndcg_args_ok(score, score_stride, targets, seg_off, Q, max_len, temperature, ndcg_k) && a_out && a_stride >= 1);
  if (max_len > kMaxLen) return RR_ERR_UNSUPPORTED;
  ApproxArgs a = ndcg_args(score, score_stride, targets, seg_off, temperature, ndcg_k);
  a.out = a_out;
  a.ostride = a_stride;
  return approx_launch<NDCG_A>(a, Q, max_len, static_cast<hipStream_t>(stream));
}

}  // extern "C"
