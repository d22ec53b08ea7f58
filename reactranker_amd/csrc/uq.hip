// Uncertainty of a trained ranker from T score samples (MC-dropout passes or ensemble members), and the calibration of an
// uncertainty against the error it should track.
//
// rr_mc_sample_stats_f32: one 64-lane wavefront owns one list, like ranking_metrics_kernel (loss.hip).  Each sample of the
// list is staged once in LDS and ranked with the same O(C^2/64) stable counting pass (descending, ties by list position);
// lane l owns candidates l, l+64, ... for every sample, so its rank sums and top-1 counts live in LDS words no other lane
// writes.  Mean and standard deviation are f64 sums in sample order; every reduction has a fixed order and there are no
// atomics, so two runs give the same bits.
//
// rr_analytic_rank_stats_f32: the same statistics from ONE forward of a distributional head, analytically under independent
// Gaussians.  p_top1_i and mean_rank_i need the whole list but not each other, so the grid is (query, block of candidates)
// and lane = candidate i; every workgroup stages mu_j, 1/sigma_j, sigma_j^2 of its list in LDS (decoded from the head's
// columns in f64, rounded once) and walks it as LDS broadcasts.  FOUR waves (256 candidates) share one staged list: at
// kMaxLen the list takes 96 of the CU's 160 KiB, so one workgroup fits per CU, and with a single wave in it three of the
// CU's four SIMDs would idle as soon as a batch has more long lists than there are CUs; the four waves also pay the
// staging pass once.  Waves past the list's end leave after staging.  The per-query numbers come from a second launch,
// one wave per query, over the rounded f32 outputs - fixed order, no atomics.
//
// rr_uq_calibration_f64: tie-averaged ranks and the descending-uncertainty positions come from binary searches over the
// two stable ascending orders (torch.sort on the device), one row per thread; block partials go to the workspace and a
// one-block second launch sums them in block order.
#include "wave_util.h"

namespace {

constexpr int kCalBlock = RR_UQ_CAL_BLOCK;
static_assert(kCalBlock % RR_WAVE == 0, "the calibration block is whole wavefronts");

__global__ void __launch_bounds__(RR_WAVE) mc_stats_kernel(const float* __restrict__ samples, int64_t sstride, int T,
                                                           const float* __restrict__ targets,
                                                           const int32_t* __restrict__ seg_off, int L,
                                                           float* __restrict__ mean, float* __restrict__ sd,
                                                           float* __restrict__ p_top1, float* __restrict__ mean_rank,
                                                           double* __restrict__ qstats) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int q = blockIdx.x, lane = threadIdx.x;
  const int off = seg_off[q], C = seg_off[q + 1] - off;
  double* qs = qstats + static_cast<int64_t>(q) * RR_UQ_NQSTATS;
  if (C <= 0 || C > L) {                                     // empty list: zeros; a list longer than max_len: NaN
    if (lane < RR_UQ_NQSTATS) qs[lane] = C <= 0 ? 0.0 : NAN;
    return;
  }
  float* s = sm;                                             // the current sample of the list
  uint32_t* rsum = reinterpret_cast<uint32_t*>(sm + L);      // sum over samples of the 0-based rank
  uint32_t* top1 = rsum + L;                                 // samples in which the candidate is the first maximum
  for (int i = lane; i < C; i += RR_WAVE) {
    rsum[i] = 0u;
    top1[i] = 0u;
  }
  for (int t = 0; t < T; ++t) {
    const float* x = samples + static_cast<int64_t>(t) * sstride + off;
    for (int i = lane; i < C; i += RR_WAVE) s[i] = x[i];
    wave_sync();
    for (int i = lane; i < C; i += RR_WAVE) {                 // stable descending rank (ranking_metrics_kernel's rule)
      const float si = s[i];
      int r = 0;
      for (int j = 0; j < C; ++j) r += rr_precedes(s[j], j, si, i) ? 1 : 0;
      rsum[i] += static_cast<uint32_t>(r);
      top1[i] += r == 0 ? 1u : 0u;
    }
    wave_sync();                                             // every read of s is done before the next sample lands
  }
  const double Td = static_cast<double>(T);
  double ent = 0.0, sdsum = 0.0;
  float bm = -INFINITY, bt = -INFINITY;
  int bmi = -1, bti = -1;
  for (int i = lane; i < C; i += RR_WAVE) {
    const float* x = samples + off + i;
    double acc = 0.0;
    for (int t = 0; t < T; ++t) acc += static_cast<double>(x[static_cast<int64_t>(t) * sstride]);
    const double m = acc / Td;
    double ss = 0.0;
    for (int t = 0; t < T; ++t) {
      const double d = static_cast<double>(x[static_cast<int64_t>(t) * sstride]) - m;
      ss += d * d;
    }
    const float mf = static_cast<float>(m), sf = static_cast<float>(sqrt(ss / (Td - 1.0)));
    const uint32_t c1 = top1[i];
    const double p = static_cast<double>(c1) / Td;
    mean[off + i] = mf;
    sd[off + i] = sf;
    p_top1[off + i] = static_cast<float>(p);
    mean_rank[off + i] = static_cast<float>((static_cast<double>(rsum[i]) + Td) / Td);   // 1-based
    if (c1 > 0u) ent -= p * log(p);
    sdsum += static_cast<double>(sf);
    if (bmi < 0 || mf > bm) { bm = mf; bmi = i; }            // i grows: a later equal value never replaces
    const float ti = targets[off + i];
    if (bti < 0 || ti > bt) { bt = ti; bti = i; }
  }
  ent = rr_wave_sum(ent);
  sdsum = rr_wave_sum(sdsum);
  rr_wave_first_max(bm, bmi);
  rr_wave_first_max(bt, bti);
  if (lane == 0) {
    qs[0] = ent;
    qs[1] = static_cast<double>(top1[bti]) / Td;
    qs[2] = static_cast<double>(top1[bmi]) / Td;
    qs[3] = sdsum / static_cast<double>(C);
  }
}

// ---------------------------------------------------------------- analytic (single-forward) statistics
constexpr int kAnaWaves = 4;
constexpr int kAnaBlock = kAnaWaves * RR_WAVE;                 // candidates per workgroup
constexpr int kAnaMaxNodes = RR_UQ_MAX_NODES;
constexpr float kRsqrt2 = 0.70710678f;

struct Moments {
  float mu, sigma, inv_sigma, var, ale, epi;
};

// Row `row` of the head's output -> predictive mean and variance (include/reactranker_hip.h: rr_moment_kind).  The variance
// is formed in f64 and each derived number is rounded once.
__device__ inline Moments decode_moments(const float* __restrict__ row, int kind) {
  Moments m;
  m.mu = row[0];
  double var, ale = 0.0, epi = 0.0;
  if (kind == RR_MOMENT_NIG) {
    const double v = row[1], am1 = static_cast<double>(row[2]) - 1.0, beta = row[3];
    ale = beta / am1;
    epi = beta / (v * am1);
    var = ale + epi;
  } else if (kind == RR_MOMENT_LOG_VARIANCE) {
    var = exp(static_cast<double>(row[1]));
  } else {
    var = row[1];
  }
  const double sd = sqrt(var);
  m.sigma = static_cast<float>(sd);
  m.inv_sigma = static_cast<float>(1.0 / sd);
  m.var = static_cast<float>(var);
  m.ale = static_cast<float>(sqrt(ale));
  m.epi = static_cast<float>(sqrt(epi));
  return m;
}

// Phi(z) = 0.5 erfcf(-z / sqrt 2), one erfcf per call; `neg_z` is -z
__device__ inline float phi_neg(float neg_z) { return 0.5f * erfcf(neg_z * kRsqrt2); }

__global__ void __launch_bounds__(kAnaBlock) analytic_rank_kernel(const float* __restrict__ out, int64_t ld, int kind,
                                                                  const int32_t* __restrict__ seg_off, int L,
                                                                  const double* __restrict__ nodes,
                                                                  const double* __restrict__ weights, int n_nodes,
                                                                  float* __restrict__ mean, float* __restrict__ sd,
                                                                  float* __restrict__ p_top1, float* __restrict__ mean_rank,
                                                                  float* __restrict__ ale_sd, float* __restrict__ epi_sd) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int q = blockIdx.x, base = blockIdx.y * kAnaBlock, tid = threadIdx.x;
  const int off = seg_off[q], C = seg_off[q + 1] - off;
  if (C <= 0 || C > L || base >= C) return;                   // the same for the whole workgroup
  float* mu = sm;                                             // L is a multiple of 4: the three arrays stay 16-byte aligned
  float* inv = sm + L;
  float* s2 = sm + 2 * L;
  const float* rows = out + static_cast<int64_t>(off) * ld;
  for (int j = tid; j < C; j += kAnaBlock) {
    const Moments m = decode_moments(rows + static_cast<int64_t>(j) * ld, kind);
    mu[j] = m.mu;
    inv[j] = m.inv_sigma;
    s2[j] = m.var;
  }
  __syncthreads();
  if (base + (tid & ~(RR_WAVE - 1)) >= C) return;              // a whole wave past the list's end
  const bool live = base + tid < C;
  const int i = live ? base + tid : C - 1;                    // idle lanes of the last wave redo C - 1 and store nothing
  const Moments me = decode_moments(rows + static_cast<int64_t>(i) * ld, kind);
  const int C4 = C & ~3;

  // expected rank: one pass over j, Phi of the margin of j over i; f64 sum, rounded once
  double rank = 1.0;
  for (int j = 0; j < C4; j += 4) {
    const float4 m4 = *reinterpret_cast<const float4*>(mu + j);
    const float4 v4 = *reinterpret_cast<const float4*>(s2 + j);
    float f0 = phi_neg((me.mu - m4.x) / sqrtf(me.var + v4.x));
    float f1 = phi_neg((me.mu - m4.y) / sqrtf(me.var + v4.y));
    float f2 = phi_neg((me.mu - m4.z) / sqrtf(me.var + v4.z));
    float f3 = phi_neg((me.mu - m4.w) / sqrtf(me.var + v4.w));
    f0 = j == i ? 0.f : f0;
    f1 = j + 1 == i ? 0.f : f1;
    f2 = j + 2 == i ? 0.f : f2;
    f3 = j + 3 == i ? 0.f : f3;
    rank += (static_cast<double>(f0) + static_cast<double>(f1)) + (static_cast<double>(f2) + static_cast<double>(f3));
  }
  for (int j = C4; j < C; ++j) {
    const float f = phi_neg((me.mu - mu[j]) / sqrtf(me.var + s2[j]));
    rank += j == i ? 0.0 : static_cast<double>(f);
  }

  // top-1 probability: Gauss-Hermite over candidate i's own score, the product over its rivals in f64
  double acc = 0.0;
  for (int n = 0; n < n_nodes; ++n) {
    const float t = me.mu + me.sigma * static_cast<float>(nodes[n]);
    double prod = 1.0;
    for (int j = 0; j < C4; j += 4) {
      const float4 m4 = *reinterpret_cast<const float4*>(mu + j);
      const float4 r4 = *reinterpret_cast<const float4*>(inv + j);
      float f0 = phi_neg((m4.x - t) * r4.x);
      float f1 = phi_neg((m4.y - t) * r4.y);
      float f2 = phi_neg((m4.z - t) * r4.z);
      float f3 = phi_neg((m4.w - t) * r4.w);
      f0 = j == i ? 1.f : f0;
      f1 = j + 1 == i ? 1.f : f1;
      f2 = j + 2 == i ? 1.f : f2;
      f3 = j + 3 == i ? 1.f : f3;
      prod *= (static_cast<double>(f0) * static_cast<double>(f1)) * (static_cast<double>(f2) * static_cast<double>(f3));
    }
    for (int j = C4; j < C; ++j) {
      const float f = phi_neg((mu[j] - t) * inv[j]);
      prod *= j == i ? 1.0 : static_cast<double>(f);
    }
    acc += weights[n] * prod;
  }
  if (!live) return;
  mean[off + i] = me.mu;
  sd[off + i] = me.sigma;
  p_top1[off + i] = static_cast<float>(acc);
  mean_rank[off + i] = static_cast<float>(rank);
  if (ale_sd) ale_sd[off + i] = me.ale;
  if (epi_sd) epi_sd[off + i] = me.epi;
}

// qstats and mass of query q from the rounded f32 outputs: lane-strided f64 partials, then the wave tree
__global__ void __launch_bounds__(RR_WAVE) analytic_qstats_kernel(const float* __restrict__ targets,
                                                                  const int32_t* __restrict__ seg_off, int L,
                                                                  const float* __restrict__ mean, const float* __restrict__ sd,
                                                                  const float* __restrict__ p_top1, double* __restrict__ qstats,
                                                                  double* __restrict__ mass) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const int off = seg_off[q], C = seg_off[q + 1] - off;
  double* qs = qstats + static_cast<int64_t>(q) * RR_UQ_NQSTATS;
  if (C <= 0 || C > L) {                                      // empty list: zeros; a list longer than max_len: NaN
    if (lane < RR_UQ_NQSTATS) qs[lane] = C <= 0 ? 0.0 : NAN;
    if (lane == 0) mass[q] = C <= 0 ? 0.0 : NAN;
    return;
  }
  double ent = 0.0, sdsum = 0.0, psum = 0.0;
  float bm = -INFINITY, bt = -INFINITY;
  int bmi = -1, bti = -1;
  for (int i = lane; i < C; i += RR_WAVE) {
    const double p = static_cast<double>(p_top1[off + i]);
    if (p > 0.0) ent -= p * log(p);
    psum += p;
    sdsum += static_cast<double>(sd[off + i]);
    const float mf = mean[off + i], ti = targets[off + i];
    if (bmi < 0 || mf > bm) { bm = mf; bmi = i; }
    if (bti < 0 || ti > bt) { bt = ti; bti = i; }
  }
  ent = rr_wave_sum(ent);
  sdsum = rr_wave_sum(sdsum);
  psum = rr_wave_sum(psum);
  rr_wave_first_max(bm, bmi);
  rr_wave_first_max(bt, bti);
  if (lane == 0) {
    qs[0] = ent;
    qs[1] = static_cast<double>(p_top1[off + bti]);
    qs[2] = static_cast<double>(p_top1[off + bmi]);
    qs[3] = sdsum / static_cast<double>(C);
    mass[q] = psum;
  }
}

// ---------------------------------------------------------------- calibration
// key(p) = x[order[p]] is ascending in p.  Order entries outside [0, n) are clamped: a wrong order gives wrong numbers,
// never a read outside x.
__device__ inline float key_at(const float* x, const int64_t* order, int64_t n, int64_t p) {
  int64_t j = order[p];
  j = j < 0 ? 0 : (j >= n ? n - 1 : j);
  return x[j];
}
__device__ inline int64_t first_not_below(const float* x, const int64_t* order, int64_t n, float v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (key_at(x, order, n, mid) < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ inline int64_t first_above(const float* x, const int64_t* order, int64_t n, float v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (!(v < key_at(x, order, n, mid))) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// inside a tie group [lo, hi) of a stable order the row indices ascend: the number of them below i
__device__ inline int64_t index_rank(const int64_t* order, int64_t lo, int64_t hi, int64_t i) {
  const int64_t base = lo;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (order[mid] < i) lo = mid + 1; else hi = mid;
  }
  return lo - base;
}

__device__ inline int64_t removed_rows(double f, int64_t n) {       // k = floor(f * n), kept in [0, n - 1]
  int64_t k = static_cast<int64_t>(floor(f * static_cast<double>(n)));
  return k < 0 ? 0 : (k > n - 1 ? n - 1 : k);
}

// sum of v over the block in a fixed order (wave trees, then the waves in order); the result is valid in thread 0
__device__ inline double block_sum(double v, double* red) {
  const int lane = threadIdx.x & (RR_WAVE - 1), w = threadIdx.x / RR_WAVE;
  v = rr_wave_sum(v);
  if (lane == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int k = 0; k < kCalBlock / RR_WAVE; ++k) s += red[k];
  __syncthreads();                                           // red is reused by the next call
  return s;
}

// partial[b * nv + v], nv = 3 + 2 * n_frac: sum d_e d_u, sum d_e^2, sum d_u^2 (d = 2 * (average rank - (n + 1) / 2)), then
// per fraction the sum of |e| and of e^2 over the rows that stay
__global__ void __launch_bounds__(kCalBlock) calib_partial_kernel(const float* __restrict__ err, const float* __restrict__ unc,
                                                                  const int64_t* __restrict__ order_err,
                                                                  const int64_t* __restrict__ order_unc, int64_t n,
                                                                  const double* __restrict__ fractions, int n_frac,
                                                                  double* __restrict__ partial) {
  __shared__ double red[kCalBlock / RR_WAVE];
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kCalBlock + threadIdx.x;
  double de = 0.0, du = 0.0, e = 0.0;
  int64_t dpos = -1;                                          // position in the stable DESCENDING order of unc
  if (i < n) {
    const float ev = err[i], uv = unc[i];
    const int64_t ae = first_not_below(err, order_err, n, ev), be = first_above(err, order_err, n, ev);
    const int64_t au = first_not_below(unc, order_unc, n, uv), bu = first_above(unc, order_unc, n, uv);
    de = static_cast<double>(ae + be - n);
    du = static_cast<double>(au + bu - n);
    // rows above the tie group come first, then the group in row order
    dpos = (n - bu) + index_rank(order_unc, au, bu, i);
    e = fabs(static_cast<double>(ev));
  }
  const int nv = 3 + 2 * n_frac;
  double* out = partial + static_cast<int64_t>(blockIdx.x) * nv;
  double v;
  v = block_sum(de * du, red);
  if (threadIdx.x == 0) out[0] = v;
  v = block_sum(de * de, red);
  if (threadIdx.x == 0) out[1] = v;
  v = block_sum(du * du, red);
  if (threadIdx.x == 0) out[2] = v;
  for (int f = 0; f < n_frac; ++f) {
    const bool keep = dpos >= removed_rows(fractions[f], n);
    v = block_sum(keep ? e : 0.0, red);
    if (threadIdx.x == 0) out[3 + 2 * f] = v;
    v = block_sum(keep ? e * e : 0.0, red);
    if (threadIdx.x == 0) out[4 + 2 * f] = v;
  }
}

__global__ void __launch_bounds__(kCalBlock) calib_finish_kernel(const double* __restrict__ partial, int nb, int64_t n,
                                                                 const double* __restrict__ fractions, int n_frac,
                                                                 double* __restrict__ out) {
  __shared__ double red[kCalBlock / RR_WAVE];
  const int nv = 3 + 2 * n_frac;
  double tot[2];
  double sxy = 0.0, sxx = 0.0;
  for (int v = 0; v < nv; ++v) {
    double acc = 0.0;
    for (int b = threadIdx.x; b < nb; b += kCalBlock) acc += partial[static_cast<int64_t>(b) * nv + v];
    const double s = block_sum(acc, red);
    if (threadIdx.x != 0) continue;
    if (v == 0) sxy = s;
    else if (v == 1) sxx = s;
    else if (v == 2) {
      double rho = NAN;                                       // a constant rank vector has no correlation
      if (sxx > 0.0 && s > 0.0) rho = fmin(1.0, fmax(-1.0, sxy / sqrt(sxx * s)));
      out[0] = rho;
    } else {
      tot[(v - 3) & 1] = s;
      if (((v - 3) & 1) == 1) {
        const int f = (v - 3) / 2;
        const double kept = static_cast<double>(n - removed_rows(fractions[f], n));
        out[1 + 3 * f] = kept;
        out[2 + 3 * f] = tot[0] / kept;
        out[3 + 3 * f] = sqrt(tot[1] / kept);
      }
    }
  }
}

}  // namespace

extern "C" {

int rr_mc_sample_stats_f32(const float* samples, int64_t sample_stride, int T, const float* targets, const int32_t* seg_off,
                           int Q, int max_len, float* mean, float* std_dev, float* p_top1, float* mean_rank, double* qstats,
                           rr_stream_t stream) {
  RR_CHECK_ARG(samples && targets && seg_off && mean && std_dev && p_top1 && mean_rank && qstats);
  RR_CHECK_ARG(T >= 2 && Q >= 0 && max_len >= 0 && sample_stride >= 1 && sample_stride >= max_len);
  if (max_len > kMaxLen) return RR_ERR_UNSUPPORTED;
  if (static_cast<int64_t>(T) * max_len > static_cast<int64_t>(UINT32_MAX)) return RR_ERR_UNSUPPORTED;   // u32 rank sums
  const int L = list_words(max_len);
  return launch_per_query(mc_stats_kernel, Q, L, sizeof(float) + 2 * sizeof(uint32_t), RR_WAVE, static_cast<hipStream_t>(stream),
                          samples, sample_stride, T, targets, seg_off, L, mean, std_dev, p_top1, mean_rank, qstats);
}

int rr_analytic_rank_stats_f32(const float* out, int64_t ld, int kind, const float* targets, const int32_t* seg_off, int Q,
                               int max_len, const double* nodes, const double* weights, int n_nodes, float* mean,
                               float* std_dev, float* p_top1, float* mean_rank, float* aleatoric_std, float* epistemic_std,
                               double* qstats, double* mass, rr_stream_t stream) {
  RR_CHECK_ARG(out && targets && seg_off && nodes && weights && mean && std_dev && p_top1 && mean_rank && qstats && mass);
  RR_CHECK_ARG(Q >= 0 && max_len >= 0 && n_nodes >= 1 && n_nodes <= kAnaMaxNodes);
  RR_CHECK_ARG(kind == RR_MOMENT_GAUSSIAN || kind == RR_MOMENT_LOG_VARIANCE || kind == RR_MOMENT_NIG);
  RR_CHECK_ARG(ld >= (kind == RR_MOMENT_NIG ? 4 : 2));
  if (max_len > kMaxLen) return RR_ERR_UNSUPPORTED;
  if (Q == 0) return RR_OK;
  const int L = list_words4(max_len);
  const size_t lds = static_cast<size_t>(L) * 3 * sizeof(float);
  if (set_lds(analytic_rank_kernel, lds) != RR_OK) return RR_ERR_LAUNCH;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(Q, (L + kAnaBlock - 1) / kAnaBlock);
  analytic_rank_kernel<<<grid, kAnaBlock, lds, s>>>(out, ld, kind, seg_off, L, nodes, weights, n_nodes, mean, std_dev, p_top1,
                                                    mean_rank, kind == RR_MOMENT_NIG ? aleatoric_std : nullptr,
                                                    kind == RR_MOMENT_NIG ? epistemic_std : nullptr);
  if (rr_launch_status() != RR_OK) return RR_ERR_LAUNCH;
  analytic_qstats_kernel<<<Q, RR_WAVE, 0, s>>>(targets, seg_off, L, mean, std_dev, p_top1, qstats, mass);
  return rr_launch_status();
}

int rr_uq_calibration_f64(const float* err, const float* unc, const int64_t* order_err, const int64_t* order_unc, int64_t n,
                          const double* fractions, int n_frac, void* workspace, size_t workspace_bytes, double* out,
                          rr_stream_t stream) {
  RR_CHECK_ARG(err && unc && order_err && order_unc && out && workspace && n >= 1 && n_frac >= 0);
  RR_CHECK_ARG(n_frac == 0 || fractions);
  const int64_t nb = (n + kCalBlock - 1) / kCalBlock;
  if (nb > INT32_MAX) return RR_ERR_UNSUPPORTED;
  const int nv = 3 + 2 * n_frac;
  if (static_cast<uint64_t>(nb) * nv * sizeof(double) > workspace_bytes) return RR_ERR_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* partial = static_cast<double*>(workspace);
  calib_partial_kernel<<<static_cast<int>(nb), kCalBlock, 0, s>>>(err, unc, order_err, order_unc, n, fractions, n_frac, partial);
  calib_finish_kernel<<<1, kCalBlock, 0, s>>>(partial, static_cast<int>(nb), n, fractions, n_frac, out);
  return rr_launch_status();
}

}  // extern "C"
