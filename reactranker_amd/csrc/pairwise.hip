// The pairwise trainer's remaining pieces (reference train/train_pairwise.py:6-78, 176-338; train/eval.py:15-73, 180-273;
// models/ranknet_baseline.py): the C x C Beta-density KL loss (BetaNet) and the C x C evidential pair loss per query with
// their gradients, the pairwise accuracy / cross-entropy evaluation, the baseline pair model's loss and accuracy on [B, 2]
// outputs, and the row combine  p1_h + p2_h - 2 r_h  that feeds its difference encoder.
//
// The C x C kernels follow ranknet_fwd_kernel / ranknet_bwd_kernel (loss.hip): one 64-lane wavefront owns one query, the
// per-candidate values are staged in LDS (12 bytes per candidate: one double, one float), a lane owns row k and walks j,
// and writes the gradient of its own rows straight to global memory.  Entry (k, j) and entry (j, k) are both seen from row
// k in the same j loop, so no lane writes another lane's row, there are no atomics and every sum has a fixed order: two
// runs give the same bits.  The per-entry arithmetic is double: BetaNet cancels lgamma values near 360 (alpha0 = 100), and
// float32 there sits 0.5e-5 .. 2.3e-5 from the exact value.  Per-query partials are doubles, summed by one block in a
// fixed order.
#include "wave_util.h"

namespace {

__device__ inline double sigmoid_d(double x) { return x >= 0.0 ? 1.0 / (1.0 + exp(-x)) : exp(x) / (1.0 + exp(x)); }

// ln Gamma(x) and (DG) digamma(x), x > 0, in double: recurrence up to x >= 10, then the Stirling series (the first omitted
// term is below 3e-14 there).  Double-precision siblings of lgammaf / digamma_f (loss.hip), which stay as they are.
template <bool DG>
__device__ inline void lgamma_digamma(double x, double* lg, double* dg) {
  double prod = 1.0, rsum = 0.0;
  while (x < 10.0) {
    prod *= x;
    if (DG) rsum += 1.0 / x;
    x += 1.0;
  }
  const double lx = log(x), r = 1.0 / x, f = r * r;
  *lg = (x - 0.5) * lx - x + 0.91893853320467274178 +
        r * (1.0 / 12 - f * (1.0 / 360 - f * (1.0 / 1260 - f * (1.0 / 1680 - f * (1.0 / 1188))))) - log(prod);
  if (DG)
    *dg = lx - 0.5 * r - f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (1.0 / 132))))) - rsum;
}

// ---------------------------------------------------------------- BetaNet (train_pairwise.py:189-226)
// Entry (i, j): x1 = tau_j / (tau_i + tau_j), x2 = tau_i / (tau_i + tau_j), aT = a0 x1, bT = a0 x2, aP = a0 pi_j / (pi_i + pi_j),
// bP = a0 pi_i / (pi_i + pi_j);  lt, lp = ln Beta-density of (aT, bT), (aP, bP) at x1;  entry = exp(lt) (lt - lp).
// aT + bT = aP + bP = a0, so lgamma(a + b) drops out of lt - lp:
//   lt - lp = (aT - aP) ln x1 + (bT - bP) ln x2 - lgamma(aT) - lgamma(bT) + lgamma(aP) + lgamma(bP).
struct BetaEntry {
  double w, diff, h, ap_scale;   // exp(lt), lt - lp, d lp / d aP (with bP = a0 - aP), a0 pi_j / (pi_i + pi_j)^2
};

template <bool GRAD>
__device__ inline BetaEntry beta_entry(double tau_i, double pi_i, double tau_j, double pi_j, double a0, double lg_a0) {
  const double st = tau_i + tau_j, sp = pi_i + pi_j;
  const double x1 = tau_j / st, x2 = tau_i / st;
  const double lx1 = log(x1), lx2 = log(x2);
  const double aT = a0 * x1, bT = a0 * x2, aP = a0 * (pi_j / sp), bP = a0 * (pi_i / sp);
  double lg_aT, lg_bT, lg_aP, lg_bP, dg_aP = 0.0, dg_bP = 0.0, unused;
  lgamma_digamma<false>(aT, &lg_aT, &unused);
  lgamma_digamma<false>(bT, &lg_bT, &unused);
  lgamma_digamma<GRAD>(aP, &lg_aP, &dg_aP);
  lgamma_digamma<GRAD>(bP, &lg_bP, &dg_bP);
  BetaEntry e;
  const double lt = (aT - 1.0) * lx1 + (bT - 1.0) * lx2 - (lg_aT + lg_bT - lg_a0);
  e.w = exp(lt);
  e.diff = (aT - aP) * lx1 + (bT - bP) * lx2 - (lg_aT + lg_bT) + (lg_aP + lg_bP);
  e.h = (lx1 - lx2) - (dg_aP - dg_bP);
  e.ap_scale = a0 * pi_j / (sp * sp);
  return e;
}

// LDS: double pi[L] | float t[L]
__global__ void __launch_bounds__(RR_WAVE) betanet_fwd_kernel(const float* __restrict__ score, int64_t sstride,
                                                              const float* __restrict__ targets,
                                                              const int32_t* __restrict__ seg_off, int L, float alpha0,
                                                              double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double smd[];
  const int q = blockIdx.x, lane = threadIdx.x;
  const int off = seg_off[q], C = seg_off[q + 1] - off;
  if (C <= 0) {
    if (lane == 0) partial[q] = 0.0;
    return;
  }
  double* pi = smd;
  float* t = reinterpret_cast<float*>(smd + L);
  for (int i = lane; i < C; i += RR_WAVE) {
    pi[i] = sigmoid_d(static_cast<double>(score[static_cast<int64_t>(off + i) * sstride]));
    t[i] = targets[off + i];
  }
  wave_sync();
  const double a0 = alpha0;
  double lg_a0, unused;
  lgamma_digamma<false>(a0, &lg_a0, &unused);
  double acc = 0.0;
  for (int k = lane; k < C; k += RR_WAVE) {
    const double tau_k = sigmoid_d(static_cast<double>(t[k])), pi_k = pi[k];
    double row = 0.0;
    for (int j = 0; j < C; ++j) {
      const BetaEntry e = beta_entry<false>(tau_k, pi_k, sigmoid_d(static_cast<double>(t[j])), pi[j], a0, lg_a0);
      row += e.w * e.diff;
    }
    acc += row;
  }
  acc = rr_wave_sum(acc);
  if (lane == 0) partial[q] = acc;
}

// The entry is symmetric under (i <-> j): x1 <-> x2, aT <-> bT, aP <-> bP leave lt and lp as they are.  So entry (j, k)
// contributes to d / d s_k exactly what entry (k, j) does, and the gradient of s_k is twice the row-k sum below; the
// diagonal entry does not depend on the scores (aP = bP = a0 / 2).
//   d entry / d aP = -w h,  d aP / d pi_i = -a0 pi_j / (pi_i + pi_j)^2,  d pi / d s = pi (1 - pi).
__global__ void __launch_bounds__(RR_WAVE) betanet_bwd_kernel(const float* __restrict__ score, int64_t sstride,
                                                              const float* __restrict__ targets,
                                                              const int32_t* __restrict__ seg_off, int L, float alpha0,
                                                              const float* __restrict__ gloss,
                                                              float* __restrict__ dscore, int64_t dstride) {
  extern __shared__ __attribute__((aligned(16))) double smd[];
  const int q = blockIdx.x, lane = threadIdx.x;
  const int off = seg_off[q], C = seg_off[q + 1] - off;
  if (C <= 0) return;
  double* pi = smd;
  float* t = reinterpret_cast<float*>(smd + L);
  for (int i = lane; i < C; i += RR_WAVE) {
    pi[i] = sigmoid_d(static_cast<double>(score[static_cast<int64_t>(off + i) * sstride]));
    t[i] = targets[off + i];
  }
  wave_sync();
  const double a0 = alpha0, g = gloss[0];
  double lg_a0, unused;
  lgamma_digamma<false>(a0, &lg_a0, &unused);
  for (int k = lane; k < C; k += RR_WAVE) {
    const double tau_k = sigmoid_d(static_cast<double>(t[k])), pi_k = pi[k];
    double row = 0.0;
    for (int j = 0; j < C; ++j) {
      if (j == k) continue;
      const BetaEntry e = beta_entry<true>(tau_k, pi_k, sigmoid_d(static_cast<double>(t[j])), pi[j], a0, lg_a0);
      row += e.w * e.h * e.ap_scale;
    }
    const double one_minus = sigmoid_d(-static_cast<double>(score[static_cast<int64_t>(off + k) * sstride]));
    dscore[static_cast<int64_t>(off + k) * dstride] = static_cast<float>(g * 2.0 * row * pi_k * one_minus);
  }
}

// ---------------------------------------------------------------- BetaNet_envidential (train_pairwise.py:276-307)
// Entry (i, j): T1 = tau_j / (tau_i + tau_j), T2 = 1 - T1 likewise, P1 = p_j / S, P2 = p_i / S, S = p_i + p_j (raw scores as
// evidence);  entry = (T1 - P1)^2 + (T2 - P2)^2 + (P1 (1 - P1) + P2 (1 - P2)) / (S + 1) + coef * 2 |ln(T1 / P1) (p_j - 1)|
// (both penalty terms of the reference use the first component, :302-307).  Not symmetric: row k adds d entry(k, j) / d p_i
// and d entry(j, k) / d p_j.
// LDS: double tau[L] | float p[L]
__device__ inline double sgn_d(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }

template <bool BWD>
__global__ void __launch_bounds__(RR_WAVE) beta_evi_kernel(const float* __restrict__ score, int64_t sstride,
                                                           const float* __restrict__ targets,
                                                           const int32_t* __restrict__ seg_off, int L, float coef_f,
                                                           double* __restrict__ partial, const float* __restrict__ gloss,
                                                           float* __restrict__ dscore, int64_t dstride) {
  extern __shared__ __attribute__((aligned(16))) double smd[];
  const int q = blockIdx.x, lane = threadIdx.x;
  const int off = seg_off[q], C = seg_off[q + 1] - off;
  if (C <= 0) {
    if (!BWD && lane == 0) partial[q] = 0.0;
    return;
  }
  double* tau = smd;
  float* p = reinterpret_cast<float*>(smd + L);
  for (int i = lane; i < C; i += RR_WAVE) {
    tau[i] = sigmoid_d(static_cast<double>(targets[off + i]));
    p[i] = score[static_cast<int64_t>(off + i) * sstride];
  }
  wave_sync();
  const double coef = coef_f;
  double acc = 0.0;
  for (int k = lane; k < C; k += RR_WAVE) {
    const double tau_k = tau[k], pk = p[k];
    double row = 0.0;
    for (int j = 0; j < C; ++j) {
      const double tau_j = tau[j], pj = p[j];
      const double st = tau_k + tau_j, S = pk + pj;
      const double T1 = tau_j / st, T2 = tau_k / st, P1 = pj / S, P2 = pk / S;
      const double c1 = log(T1 / P1);
      if (!BWD) {
        const double e1 = T1 - P1, e2 = T2 - P2;
        row += (e1 * e1 + e2 * e2) + (P1 * (1.0 - P1) + P2 * (1.0 - P2)) / (S + 1.0) + coef * (2.0 * fabs(c1 * (pj - 1.0)));
      } else {
        const double S1 = S + 1.0;
        const double dvs = -2.0 * P1 * P2 / (S1 * S1);                       // d var / d S at fixed P1
        // entry (k, j), k in the i role: d P1 / d p_i = -P1 / S
        const double sg1 = sgn_d(c1 * (pj - 1.0));
        const double g1 = -4.0 * (T1 - P1) + 2.0 * (1.0 - 2.0 * P1) / S1 - coef * 2.0 * sg1 * (pj - 1.0) / P1;
        // entry (j, k), k in the j role: its first component is (T2, P2); d P2 / d p_k = P1 / S, and p_k enters the penalty
        const double c2 = log(T2 / P2);
        const double sg2 = sgn_d(c2 * (pk - 1.0));
        const double g2 = -4.0 * (T2 - P2) + 2.0 * (1.0 - 2.0 * P2) / S1 - coef * 2.0 * sg2 * (pk - 1.0) / P2;
        row += (g1 * (-P1 / S) + dvs) + (g2 * (P1 / S) + dvs + coef * 2.0 * sg2 * c2);
      }
    }
    if (BWD)
      dscore[static_cast<int64_t>(off + k) * dstride] = static_cast<float>(static_cast<double>(gloss[0]) * row);
    else
      acc += row;
  }
  if (!BWD) {
    acc = rr_wave_sum(acc);
    if (lane == 0) partial[q] = acc;
  }
}

// loss_sum = sum of the per-query partials, pairs = sum of C^2 - C: one block, fixed order
__global__ void __launch_bounds__(256) finish_sq_kernel(const double* __restrict__ partial, const int32_t* __restrict__ seg_off,
                                                        int Q, float* __restrict__ loss_sum, int64_t* __restrict__ pairs) {
  double acc = 0.0;
  long long np = 0;
  for (int i = threadIdx.x; i < Q; i += 256) {
    acc += partial[i];
    const long long c = seg_off[i + 1] - seg_off[i];
    if (c > 0) np += c * c - c;
  }
  acc = block_sum(acc);                                             // two types, so two trees: each in block_sum's order
  np = block_sum(np);
  if (threadIdx.x == 0) {
    loss_sum[0] = static_cast<float>(acc);
    pairs[0] = np;
  }
}

// ---------------------------------------------------------------- pairwise_acc + eval_cross_entropy_loss (eval.py:15-73, 180-224)
// qstats[q] = { npos, sum_ij |[s_i > s_j] - [t_i > t_j]|, sum over t_i != t_j of C_ij, unused }.
// C_ij = 0.5 (1 - S_ij) x - logsigmoid(-x), x = sigma (s_i - s_j), S_ij = sign(t_i - t_j): log(1 + e^x) for S = 1 and
// x + log(1 + e^x) for S = -1 (the code as written, eval.py:56).
// LDS: float s[L] | float t[L]
__global__ void __launch_bounds__(RR_WAVE) pairwise_eval_kernel(const float* __restrict__ score, int64_t sstride,
                                                                const float* __restrict__ targets,
                                                                const int32_t* __restrict__ seg_off, int L, float sigma,
                                                                double* __restrict__ qstats) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int q = blockIdx.x, lane = threadIdx.x;
  const int off = seg_off[q], C = seg_off[q + 1] - off;
  if (C <= 0) {
    if (lane < 4) qstats[4 * static_cast<int64_t>(q) + lane] = 0.0;
    return;
  }
  float* s = sm;
  float* t = sm + L;
  stage_list(s, t, score, sstride, targets, off, C, lane);
  int npos = 0, mism = 0;
  double ce = 0.0;
  for (int i = lane; i < C; i += RR_WAVE) {
    const float ti = t[i], si = s[i];
    for (int j = 0; j < C; ++j) {
      const bool tp = ti > t[j], sp = si > s[j];
      npos += tp ? 1 : 0;
      mism += (tp != sp) ? 1 : 0;
      if (ti != t[j]) {
        const double x = static_cast<double>(sigma * (si - s[j]));
        const double softplus = (x > 0.0 ? x : 0.0) + log1p(exp(-fabs(x)));
        ce += tp ? softplus : x + softplus;
      }
    }
  }
  npos = rr_wave_sum(npos);
  mism = rr_wave_sum(mism);
  ce = rr_wave_sum(ce);
  if (lane == 0) {
    double* o = qstats + 4 * static_cast<int64_t>(q);
    o[0] = npos;
    o[1] = mism;
    o[2] = ce;
    o[3] = 0.0;
  }
}

// out = { sum over queries with npos > 0 of 1 - mism / (2 npos), number of those queries, sum of ce, sum of 2 npos }
__global__ void __launch_bounds__(256) finish_eval_kernel(const double* __restrict__ qstats, int Q, double* __restrict__ out) {
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < Q; i += 256) {
    const double* o = qstats + 4 * static_cast<int64_t>(i);
    if (o[0] > 0.0) {
      a[0] += 1.0 - o[1] / (2.0 * o[0]);
      a[1] += 1.0;
      a[2] += o[2];
      a[3] += 2.0 * o[0];
    }
  }
  block_sum(a);
  if (threadIdx.x == 0)
    for (int u = 0; u < 4; ++u) out[u] = a[u];
}

// ---------------------------------------------------------------- baseline pair loop (train_pairwise.py:27-59, eval.py:246-266)
constexpr int kPairBlock = 256;   // block_sum's workgroup
inline int pair_blocks(int64_t n) { return rr_grid_for(n, kPairBlock, 1024); }

// loss = mean_b sum_k (softmax(t_b)_k - y_bk / (y_b0 + y_b1))^2
__global__ void __launch_bounds__(kPairBlock) pair_mse_fwd_kernel(const float* __restrict__ y, int64_t ldy,
                                                                  const float* __restrict__ tg, int64_t ldt, int64_t B,
                                                                  double* __restrict__ partial) {
  double acc = 0.0;
  for (int64_t b = static_cast<int64_t>(blockIdx.x) * kPairBlock + threadIdx.x; b < B;
       b += static_cast<int64_t>(gridDim.x) * kPairBlock) {
    const double y0 = y[b * ldy], y1 = y[b * ldy + 1], t0 = tg[b * ldt], t1 = tg[b * ldt + 1];
    const double tp0 = 1.0 / (1.0 + exp(t1 - t0)), tp1 = 1.0 / (1.0 + exp(t0 - t1));
    const double S = y0 + y1, e0 = tp0 - y0 / S, e1 = tp1 - y1 / S;
    acc += e0 * e0 + e1 * e1;
  }
  acc = block_sum(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(256) finish_scale_kernel(const double* __restrict__ partial, int n, double scale,
                                                           float* __restrict__ out) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
  acc = block_sum(acc);
  if (threadIdx.x == 0) out[0] = static_cast<float>(acc * scale);
}

// d pp_k / d y_m = (delta_km - pp_k) / S
__global__ void __launch_bounds__(kPairBlock) pair_mse_bwd_kernel(const float* __restrict__ y, int64_t ldy,
                                                                  const float* __restrict__ tg, int64_t ldt, int64_t B,
                                                                  const float* __restrict__ gloss, float* __restrict__ dy,
                                                                  int64_t ldd) {
  const double g = static_cast<double>(gloss[0]) / static_cast<double>(B);
  for (int64_t b = static_cast<int64_t>(blockIdx.x) * kPairBlock + threadIdx.x; b < B;
       b += static_cast<int64_t>(gridDim.x) * kPairBlock) {
    const double y0 = y[b * ldy], y1 = y[b * ldy + 1], t0 = tg[b * ldt], t1 = tg[b * ldt + 1];
    const double tp0 = 1.0 / (1.0 + exp(t1 - t0)), tp1 = 1.0 / (1.0 + exp(t0 - t1));
    const double S = y0 + y1, p0 = y0 / S, p1 = y1 / S;
    const double d0 = 2.0 * (p0 - tp0), d1 = 2.0 * (p1 - tp1);
    const double common = (d0 * p0 + d1 * p1) / S;
    dy[b * ldd] = static_cast<float>(g * (d0 / S - common));
    dy[b * ldd + 1] = static_cast<float>(g * (d1 / S - common));
  }
}

// acc = 1 - sum_b |[y_b0 > y_b1] - [tp_b0 > tp_b1]| / B with tp = exp(t) / sum exp(t) in float32 as the reference forms it
__global__ void __launch_bounds__(256) pair_acc_kernel(const float* __restrict__ y, int64_t ldy, const float* __restrict__ tg,
                                                       int64_t ldt, int64_t B, float* __restrict__ acc) {
  int miss = 0;
  for (int64_t b = threadIdx.x; b < B; b += 256) {
    const float e0 = expf(tg[b * ldt]), e1 = expf(tg[b * ldt + 1]), es = e0 + e1;
    const bool tp = (e0 / es) > (e1 / es), pp = y[b * ldy] > y[b * ldy + 1];
    miss += (tp != pp) ? 1 : 0;
  }
  miss = block_sum(miss);
  if (threadIdx.x == 0) acc[0] = 1.0f - static_cast<float>(miss) / static_cast<float>(B);
}

// out[row] = h1[i1[row]] + h2[i2[row]] - 2 hr[ir[row]]; a null index array is the identity.  One 16-byte lane per 4 columns.
__global__ void __launch_bounds__(256) pair_combine_kernel(const float* __restrict__ hr, const float* __restrict__ h1,
                                                           const float* __restrict__ h2, int64_t ld,
                                                           const int32_t* __restrict__ ir, const int32_t* __restrict__ i1,
                                                           const int32_t* __restrict__ i2, int64_t n_rows, int H4,
                                                           float* __restrict__ out, int64_t ld_out) {
  const int64_t total = n_rows * H4;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; e < total;
       e += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t row = e / H4;
    const int c = static_cast<int>(e - row * H4) * 4;
    const int64_t rr = ir ? ir[row] : row, r1 = i1 ? i1[row] : row, r2 = i2 ? i2[row] : row;
    const f32x4 a = *reinterpret_cast<const f32x4*>(h1 + r1 * ld + c);
    const f32x4 b = *reinterpret_cast<const f32x4*>(h2 + r2 * ld + c);
    const f32x4 r = *reinterpret_cast<const f32x4*>(hr + rr * ld + c);
    // (p1 - r) + (p2 - r): the reference's order of operations (ranknet_baseline.py:57-61)
    *reinterpret_cast<f32x4*>(out + row * ld_out + c) = (a - r) + (b - r);
  }
}

// the C x C kernels stage one double and one float per candidate (12 bytes)
constexpr size_t kSqBytes = sizeof(double) + sizeof(float);

// the second launch of their forward entry points; st: the status of the first, which a failure passes through
int finish_sq(int st, const double* partial, const int32_t* seg_off, int Q, float* loss_sum, int64_t* pairs, hipStream_t s) {
  if (st != RR_OK) return st;
  finish_sq_kernel<<<1, 256, 0, s>>>(partial, seg_off, Q, loss_sum, pairs);
  return rr_launch_status();
}

}  // namespace

extern "C" {

int rr_betanet_fwd_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q,
                       int max_len, float alpha0, float* loss_sum, int64_t* pairs, double* partial, rr_stream_t stream) {
  RR_CHECK_ARG(list_args_ok(score, targets, seg_off, Q, max_len) && loss_sum && pairs && partial && score_stride >= 1 &&
               alpha0 > 0.f);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int st = launch_list(betanet_fwd_kernel, kSqBytes, score, score_stride, targets, seg_off, Q, max_len, s, alpha0, partial);
  return finish_sq(st, partial, seg_off, Q, loss_sum, pairs, s);
}

int rr_betanet_bwd_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q,
                       int max_len, float alpha0, const float* gloss, float* dscore, int64_t dscore_stride,
                       rr_stream_t stream) {
  RR_CHECK_ARG(list_args_ok(score, targets, seg_off, Q, max_len) && gloss && dscore && score_stride >= 1 &&
               dscore_stride >= 1 && alpha0 > 0.f);
  return launch_list(betanet_bwd_kernel, kSqBytes, score, score_stride, targets, seg_off, Q, max_len,
                     static_cast<hipStream_t>(stream), alpha0, gloss, dscore, dscore_stride);
}

int rr_beta_evidential_fwd_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off,
                               int Q, int max_len, float coef, float* loss_sum, int64_t* pairs, double* partial,
                               rr_stream_t stream) {
  RR_CHECK_ARG(list_args_ok(score, targets, seg_off, Q, max_len) && loss_sum && pairs && partial && score_stride >= 1);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int st = launch_list(beta_evi_kernel<false>, kSqBytes, score, score_stride, targets, seg_off, Q, max_len, s, coef, partial,
                             nullptr, nullptr, 0);
  return finish_sq(st, partial, seg_off, Q, loss_sum, pairs, s);
}

int rr_beta_evidential_bwd_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off,
                               int Q, int max_len, float coef, const float* gloss, float* dscore, int64_t dscore_stride,
                               rr_stream_t stream) {
  RR_CHECK_ARG(list_args_ok(score, targets, seg_off, Q, max_len) && gloss && dscore && score_stride >= 1 &&
               dscore_stride >= 1);
  return launch_list(beta_evi_kernel<true>, kSqBytes, score, score_stride, targets, seg_off, Q, max_len,
                     static_cast<hipStream_t>(stream), coef, nullptr, gloss, dscore, dscore_stride);
}

int rr_pairwise_eval_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q,
                         int max_len, float sigma, double* qstats, double* out, rr_stream_t stream) {
  RR_CHECK_ARG(list_args_ok(score, targets, seg_off, Q, max_len) && qstats && out && score_stride >= 1);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int st = launch_list(pairwise_eval_kernel, 2 * sizeof(float), score, score_stride, targets, seg_off, Q, max_len, s, sigma, qstats);
  if (st != RR_OK) return st;
  finish_eval_kernel<<<1, 256, 0, s>>>(qstats, Q, out);
  return rr_launch_status();
}

int64_t rr_pair_partial_count(int64_t B) { return pair_blocks(B); }

int rr_pair_softmax_mse_fwd_f32(const float* y, int64_t ldy, const float* targets, int64_t ldt, int64_t B, float* loss,
                                double* partial, rr_stream_t stream) {
  RR_CHECK_ARG(y && targets && loss && partial && B >= 0 && ldy >= 2 && ldt >= 2);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nb = pair_blocks(B);
  pair_mse_fwd_kernel<<<nb, kPairBlock, 0, s>>>(y, ldy, targets, ldt, B, partial);
  finish_scale_kernel<<<1, 256, 0, s>>>(partial, nb, B > 0 ? 1.0 / static_cast<double>(B) : NAN, loss);
  return rr_launch_status();
}

int rr_pair_softmax_mse_bwd_f32(const float* y, int64_t ldy, const float* targets, int64_t ldt, int64_t B,
                                const float* gloss, float* dy, int64_t ldd, rr_stream_t stream) {
  RR_CHECK_ARG(y && targets && gloss && dy && B >= 0 && ldy >= 2 && ldt >= 2 && ldd >= 2);
  if (B == 0) return RR_OK;
  pair_mse_bwd_kernel<<<pair_blocks(B), kPairBlock, 0, static_cast<hipStream_t>(stream)>>>(y, ldy, targets, ldt, B, gloss, dy,
                                                                                           ldd);
  return rr_launch_status();
}

int rr_pair_acc_f32(const float* y, int64_t ldy, const float* targets, int64_t ldt, int64_t B, float* acc,
                    rr_stream_t stream) {
  RR_CHECK_ARG(y && targets && acc && B >= 1 && ldy >= 2 && ldt >= 2);
  pair_acc_kernel<<<1, 256, 0, static_cast<hipStream_t>(stream)>>>(y, ldy, targets, ldt, B, acc);
  return rr_launch_status();
}

int rr_pair_combine_f32(const float* hr, const float* h1, const float* h2, int64_t ld, const int32_t* ir, const int32_t* i1,
                        const int32_t* i2, int64_t n_rows, int H, float* out, int64_t ld_out, rr_stream_t stream) {
  RR_CHECK_ARG(hr && h1 && h2 && out && n_rows >= 0 && H >= 1 && ld >= H && ld_out >= H);
  if (H % 4 != 0 || ld % 4 != 0 || ld_out % 4 != 0 || !rr_aligned16(hr) || !rr_aligned16(h1) || !rr_aligned16(h2) ||
      !rr_aligned16(out))
    return RR_ERR_ALIGN;
  if (n_rows == 0) return RR_OK;
  const int H4 = H / 4;
  pair_combine_kernel<<<rr_grid_for(n_rows * H4, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(hr, h1, h2, ld, ir, i1, i2,
                                                                                                  n_rows, H4, out, ld_out);
  return rr_launch_status();
}

}  // extern "C"
