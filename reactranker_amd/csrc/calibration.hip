// Probabilistic calibration of a predicted (mean, std) and the per-list calibration and prediction sets of a top-1
// probability.  Definitions of this library, not ports.
//
// rr_gauss_calibration_f64: is sigma the right SIZE?  One row per thread, everything in f64:
//   sigma = sigma_scale * std,  z = (target - mean) / sigma,  pit = 0.5 erfc(-z / sqrt 2),
//   crps = sigma (z (2 pit - 1) + 2 phi(z) - 1 / sqrt pi),  bin = min(n_bins - 1, (int)floor(pit * n_bins)).
// A row whose mean or target is not finite or whose std is not finite and positive is counted as invalid and adds nothing
// else.  Structured as rr_uq_calibration_f64 (uq.hip): a block of RR_UQ_CAL_BLOCK rows reduces its eight sums in a fixed order
// (the wave tree, then the four waves in order) and counts its histogram with integer LDS adds - a block holds at most 256
// rows, exact in an int and in a double - into partial[block * (8 + n_bins) ...]; a second launch of one workgroup, thread v
// for value v, adds the blocks' partials in block order.  No floating-point atomics: run-to-run identical bits.
//
// rr_top1_sets_f32: one workgroup owns one list - one wavefront when the window's longest list has at most 64 candidates,
// four above.  Candidate j is AHEAD of i where p_j > p_i, or p_j == p_i and j < i (the stable descending order, ties by list
// position: rr_ranking_metrics_f32's `order`);  rank_i = 1 + #ahead,  before_i = the f64 sum of p_j over the candidates ahead
// of i, ONE chain of IEEE additions in ascending j (a candidate that is not ahead adds +0.0, which changes no bit of a
// non-negative sum),  in_set_i = before_i <= tau.  Thread = candidate i, strided over the workgroup; a thread walks ALL j of
// the list's p in LDS, four at a time (16-byte broadcast reads), and the chain of a candidate lives in one thread, so the
// one-wave and four-wave forms give the same bits.  Phases, every barrier outside every loop:
//   1  stage p (padded with -inf, which is ahead of nothing, to a multiple of four); each thread keeps the first maximum of
//      the targets it reads, and the workgroup reduces it to the true top
//   2  the walk; rank, before and in_set go to global memory; the thread that owns the true top leaves its rank, before
//      and in_set in LDS; per thread the number of candidates in the set and the lowest position of rank 1
//   3  those two integers reduced over the workgroup (wave shuffles, then the four waves' partials from LDS)
//   4  thread 0 forms the Brier score and the mass, two f64 chains in ascending i, and writes the nine statistics
// A comparison with a NaN is false, so a NaN in p is ahead of nothing and has nothing ahead; it and a negative p change
// values and never an address: every store goes to position off + i of a thread's own candidate or to the query's own
// statistics, and the two positions read back (the true top, the predicted top) are reduced from positions below C.
// LDS: p, 4 bytes per candidate (targets are read once, in phase 1, and not kept), and 96 bytes of scratch.
#include "wave_util.h"

namespace {

// ---------------------------------------------------------------- rr_gauss_calibration_f64
constexpr int kCalBlock = RR_UQ_CAL_BLOCK;
constexpr int kCalWaves = kCalBlock / RR_WAVE;
constexpr int kNSums = RR_GAUSS_CAL_NSUMS;
constexpr int kMaxBins = RR_GAUSS_CAL_MAX_BINS;
static_assert(kCalBlock % RR_WAVE == 0, "the calibration block is whole wavefronts");
static_assert(kCalBlock >= kNSums + kMaxBins, "one thread of the finishing workgroup per value");

constexpr double kSqrt2 = 1.41421356237309504880;         // sqrt 2
constexpr double kInvSqrt2Pi = 0.39894228040143267794;    // 1 / sqrt(2 pi)
constexpr double kInvSqrtPi = 0.56418958354775628695;     // 1 / sqrt pi

__global__ void __launch_bounds__(kCalBlock) gauss_partial_kernel(const float* __restrict__ mean, const float* __restrict__ sd,
                                                                  const float* __restrict__ target, int64_t n,
                                                                  double sigma_scale, int n_bins, double* __restrict__ partial) {
  __shared__ double red[kCalWaves][kNSums];
  __shared__ int hist[kMaxBins];
  const int tid = threadIdx.x;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kCalBlock + tid;
  if (tid < kMaxBins) hist[tid] = 0;
  __syncthreads();
  double v[kNSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (i < n) {
    const float mf = mean[i], sf = sd[i], tf = target[i];
    if (isfinite(mf) && isfinite(tf) && isfinite(sf) && sf > 0.f) {
      const double sigma = sigma_scale * static_cast<double>(sf);
      const double err = static_cast<double>(tf) - static_cast<double>(mf);
      const double z = err / sigma;
      const double pit = 0.5 * erfc(-z / kSqrt2);
      const double pdf = kInvSqrt2Pi * exp(-0.5 * (z * z));
      v[0] = 1.0;
      v[2] = z;
      v[3] = z * z;
      v[4] = log(sigma);
      v[5] = sigma * sigma;
      v[6] = err * err;
      v[7] = sigma * (z * (2.0 * pit - 1.0) + 2.0 * pdf - kInvSqrtPi);
      // pit lies in [0, 1]; a NaN (a sigma that the scale underflowed to zero) goes to bin 0: the index stays in range
      const double fb = floor(pit * static_cast<double>(n_bins));
      const int b = fb >= 1.0 ? (fb < static_cast<double>(n_bins) ? static_cast<int>(fb) : n_bins - 1) : 0;
      atomicAdd(&hist[b], 1);
    } else {
      v[1] = 1.0;
    }
  }
#pragma unroll
  for (int k = 0; k < kNSums; ++k) v[k] = rr_wave_sum(v[k]);
  if ((tid & (RR_WAVE - 1)) == 0) {
#pragma unroll
    for (int k = 0; k < kNSums; ++k) red[tid / RR_WAVE][k] = v[k];
  }
  __syncthreads();
  double* out = partial + static_cast<int64_t>(blockIdx.x) * (kNSums + n_bins);
  if (tid < kNSums) {
    double s = 0.0;
    for (int w = 0; w < kCalWaves; ++w) s += red[w][tid];
    out[tid] = s;
  } else if (tid < kNSums + n_bins) {
    out[tid] = static_cast<double>(hist[tid - kNSums]);
  }
}

__global__ void __launch_bounds__(kCalBlock) gauss_finish_kernel(const double* __restrict__ partial, int nb, int nv,
                                                                 double* __restrict__ out) {
  const int v = threadIdx.x;
  if (v >= nv) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += partial[static_cast<int64_t>(b) * nv + v];
  out[v] = s;
}

// ---------------------------------------------------------------- rr_top1_sets_f32
WaveKnob g_knob;                       // rr_top1_sets_set_waves

constexpr int kTopScratch = 96;        // the true top's (before, rank, in_set) and four waves' partials of two reductions

__device__ inline void walk_step(float pj, int j, float pi, int i, int& ahead, double& before) {
  const bool a = rr_precedes(pj, j, pi, i);
  ahead += a ? 1 : 0;
  before += a ? static_cast<double>(pj) : 0.0;
}

template <int NW>
__global__ void __launch_bounds__(NW * RR_WAVE) top1_sets_kernel(const float* __restrict__ prob, int64_t pstride,
                                                                  const float* __restrict__ targets,
                                                                  const int32_t* __restrict__ seg_off, int L, double tau,
                                                                  int32_t* __restrict__ rank, double* __restrict__ before,
                                                                  uint8_t* __restrict__ in_set, double* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int NT = NW * RR_WAVE;
  const int q = blockIdx.x, tid = threadIdx.x, wave = tid / RR_WAVE;
  const int off = seg_off[q], C = seg_off[q + 1] - off;
  double* st = stats + static_cast<int64_t>(q) * RR_TOP1_NSTATS;
  if (C <= 0 || C > L) {                                           // workgroup-uniform, before any barrier
    if (tid < RR_TOP1_NSTATS) st[tid] = tid < 6 ? static_cast<double>(NAN) : 0.0;
    return;
  }
  float* p = sm;                                                   // L % 4 == 0: the scratch stays 16-byte aligned
  double* top_before = reinterpret_cast<double*>(sm + L);          // written by the thread that owns the true top
  int* top_rank = reinterpret_cast<int*>(top_before + 1);
  int* top_in = top_rank + 1;
  float* red_v = reinterpret_cast<float*>(top_in + 1);             // [4] first maximum of the targets, per wave
  int* red_i = reinterpret_cast<int*>(red_v + 4);                  // [4]
  int* red_n = red_i + 4;                                          // [4] candidates in the set
  int* red_f = red_n + 4;                                          // [4] lowest position of rank 1

  const int C4 = (C + 3) & ~3;                                     // <= L
  float bt = -INFINITY;
  int bti = -1;
  for (int i = tid; i < C4; i += NT) {
    p[i] = i < C ? prob[static_cast<int64_t>(off + i) * pstride] : -INFINITY;
    if (i < C) {
      const float ti = targets[off + i];
      if (bti < 0 || ti > bt) { bt = ti; bti = i; }                // i grows: a later equal value never replaces
    }
  }
  rr_wave_first_max(bt, bti);
  if ((tid & (RR_WAVE - 1)) == 0) {
    red_v[wave] = bt;
    red_i[wave] = bti;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < NW; ++w) {                                   // the waves in order; wave 0 always holds candidate 0
    const float ov = red_v[w];
    const int oi = red_i[w];
    if (w == 0 || (oi >= 0 && (ov > bt || (ov == bt && oi < bti)))) { bt = ov; bti = oi; }
  }
  const int it = bti;                                              // the true top, in [0, C)

  int n_in = 0, first = C;
  for (int i = tid; i < C; i += NT) {
    const float pi = p[i];
    int ahead = 0;
    double b = 0.0;
    for (int j = 0; j < C4; j += 4) {
      const float4 p4 = *reinterpret_cast<const float4*>(p + j);
      walk_step(p4.x, j, pi, i, ahead, b);
      walk_step(p4.y, j + 1, pi, i, ahead, b);
      walk_step(p4.z, j + 2, pi, i, ahead, b);
      walk_step(p4.w, j + 3, pi, i, ahead, b);
    }
    const bool in = b <= tau;
    rank[off + i] = ahead + 1;
    before[off + i] = b;
    in_set[off + i] = in ? 1 : 0;
    n_in += in ? 1 : 0;
    if (ahead == 0 && i < first) first = i;
    if (i == it) {
      *top_before = b;
      *top_rank = ahead + 1;
      *top_in = in ? 1 : 0;
    }
  }
  n_in = rr_wave_sum(n_in);
  first = rr_wave_min(first);
  if ((tid & (RR_WAVE - 1)) == 0) {
    red_n[wave] = n_in;
    red_f[wave] = first;
  }
  __syncthreads();

  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      n_in += red_n[w];
      first = red_f[w] < first ? red_f[w] : first;
    }
    // the candidate with the largest p that is not a NaN has nothing ahead, so a list of C >= 1 has a rank 1; a list of
    // NaNs only has C of them and the lowest position is taken
    const int is = first < C ? first : C - 1;
    double brier = 0.0, mass = 0.0;
    for (int i = 0; i < C; ++i) {
      const double pi = static_cast<double>(p[i]);
      const double d = pi - (i == it ? 1.0 : 0.0);
      brier += d * d;
      mass += pi;
    }
    st[0] = is == it ? 1.0 : 0.0;
    st[1] = static_cast<double>(p[is]);
    st[2] = static_cast<double>(p[it]);
    st[3] = static_cast<double>(*top_rank);
    st[4] = brier;
    st[5] = *top_before;
    st[6] = static_cast<double>(n_in);
    st[7] = static_cast<double>(*top_in);
    st[8] = mass;
  }
}

}  // namespace

extern "C" {

int rr_gauss_calibration_f64(const float* mean, const float* std_dev, const float* target, int64_t n, double sigma_scale,
                             int n_bins, void* workspace, size_t workspace_bytes, double* out, rr_stream_t stream) {
  RR_CHECK_ARG(mean && std_dev && target && workspace && out && n >= 1);
  RR_CHECK_ARG(n_bins >= 1 && n_bins <= kMaxBins);
  RR_CHECK_ARG(sigma_scale > 0.0 && sigma_scale <= 1.7976931348623157e308);     // positive and finite (a NaN fails both)
  const int64_t nb = (n + kCalBlock - 1) / kCalBlock;
  if (nb > INT32_MAX) return RR_ERR_UNSUPPORTED;
  const int nv = kNSums + n_bins;
  if (static_cast<uint64_t>(nb) * nv * sizeof(double) > workspace_bytes) return RR_ERR_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* partial = static_cast<double*>(workspace);
  gauss_partial_kernel<<<static_cast<int>(nb), kCalBlock, 0, s>>>(mean, std_dev, target, n, sigma_scale, n_bins, partial);
  gauss_finish_kernel<<<1, kCalBlock, 0, s>>>(partial, static_cast<int>(nb), nv, out);
  return rr_launch_status();
}

int rr_top1_sets_waves(void) { return g_knob.waves; }
int rr_top1_sets_set_waves(int waves) { return g_knob.set(waves); }

int rr_top1_sets_f32(const float* p, int64_t p_stride, const float* targets, const int32_t* seg_off, int Q, int max_len,
                     double tau, int32_t* rank, double* before, uint8_t* in_set, double* stats, rr_stream_t stream) {
  RR_CHECK_ARG(list_args_ok(p, targets, seg_off, Q, max_len) && p_stride >= 1 && rank && before && in_set && stats);
  RR_CHECK_ARG(tau >= 0.0);                                        // (a NaN fails; +inf passes: every candidate is in the set)
  if (max_len > kMaxLen) return RR_ERR_UNSUPPORTED;
  const int L = list_words4(max_len);
  return launch_waves(top1_sets_kernel<1>, top1_sets_kernel<4>, g_knob.pick(max_len), Q, L * sizeof(float) + kTopScratch,
                      static_cast<hipStream_t>(stream), p, p_stride, targets, seg_off, L, tau, rank, before, in_set, stats);
}

}  // extern "C"
