// Per-query ranking losses: ListMLE, ListNet, evidential UC-Listwise, RankNet, plus the
// pointwise MSE / Gaussian NLL and the standalone LogCumsumExp op.
//
// One 64-lane wavefront owns one list (a query's candidates).  The list is staged in LDS
// (up to 5 * max_len floats), ranked by target with an O(C^2/64) counting pass, and reduced /
// scanned with wave shuffles; lists longer than 64 give each lane a contiguous chunk.
// Only wave-level synchronisation is used (no workgroup barrier), so waves of different
// list lengths never wait on each other.  Per-query partials are finished by a fixed-order
// second kernel: no float atomics, results are run-to-run identical.
//
// The nine list losses share ONE kernel shell, list_loss_kernel<K>: stage the list, build its term (loss_list.h, where each
// loss formula is written once with its normalisers - the composite step of task_loss.hip builds the same terms), write the
// partial and / or hand the term an emit that stores the gradient, finish; and one host body, list_launch<K>.  RankNet keeps
// its own pair loops (ranknet_fwd_kernel, ranknet_bwd_kernel).  The four pointwise losses share pointwise_kernel<K, BWD> over
// point_row<K> (loss_list.h), and every workgroup-wide sum is block_sum (wave_util.h).
//
// The reference evaluates these losses as a Python loop of ~10 tiny ATen ops per query
// (train/loss.py:86-97, 338-347, 504-554; train/train_pairwise.py:99-137).
#include "loss_list.h"

std::atomic<long long> rr_lds_opt_in_count{0};

namespace {

// ---------------------------------------------------------------- the shell of the nine list losses: ListMLE, ListNet,
// UC-Listwise, MLEDis, ListNet-Gauss, ListNet-lognorm, ListNet-evidential, ListNet-uq, Dirichlet-uq (ListLoss<K>, loss_list.h)
struct VarIn {            // up to three per-candidate inputs, each read at x[k][row * st[k]]
  const float* x[3];
  int64_t st[3];
};

struct VarOut {           // their gradients, written at d[k][row * st]
  float* d[3];
  int64_t st;
};

// kForward: partial[q] = the query's loss.  kBackward: the gradients of the finished loss, times *gloss.  kStep: both in one
// launch - the loss AND d loss / d input for an upstream gradient of one (what `loss.backward()` feeds a loss that is the
// root of the graph; gloss == nullptr stands for it): the reference's trainer step (train_listwise.py:287-288) then needs
// no second loss kernel, no separate reduction launch and no host-created gradient.  Same operations in the same order as
// the other two modes, and the partials are summed by the last-arriving workgroup (finish_last, loss_list.h), so the bits
// are those of the two-kernel path.
enum ListMode : int { kForward = 0, kBackward = 1, kStep = 2 };

struct ListArgs {
  VarIn in;
  const float* targets;
  const int32_t* seg_off;
  int L, Q;
  float coef, inv_total;  // the penalty coefficient of the UQ losses; ListNet's 1 / candidates of the window
  int mode;
  float* partial;
  const float* gloss;
  VarOut out;
  float scale;            // kStep: loss = scale * the sum of the partials
  float* loss;
  unsigned int* counter;
};

template <int K>
__global__ void __launch_bounds__(RR_WAVE) list_loss_kernel(ListArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  using Loss = ListLoss<K>;
  const int q = blockIdx.x, lane = threadIdx.x;
  const int off = a.seg_off[q], C = a.seg_off[q + 1] - off;
  if (C <= 0) {                                                     // an empty query adds nothing (still counted in Q)
    if (a.mode != kBackward && lane == 0) a.partial[q] = 0.f;
  } else {
    const ListView v = carve(sm, a.L);
    for (int i = lane; i < C; i += RR_WAVE) {
      const int64_t r = off + i;
#pragma unroll
      for (int k = 0; k < Loss::kInputs; ++k) v.col(k)[i] = a.in.x[k][r * a.in.st[k]];
      v.t[i] = a.targets[r];
    }
    wave_sync();
    const ListNorm n{C, a.Q, a.inv_total, a.coef};
    const auto term = Loss::term(v, n, lane);
    if (a.mode != kBackward) {
      const auto acc = term.forward();
      if (lane == 0) a.partial[q] = Loss::partial(acc, n);
    }
    if (a.mode != kForward) {
      const float g = Loss::grad_scale(a.gloss ? a.gloss[0] : 1.0f, n);
      term.gradient(g, [&](int i, auto... gs) {
        int k = 0;
        ((a.out.d[k++][static_cast<int64_t>(off + i) * a.out.st] = gs), ...);
      });
    }
  }
  if (a.mode == kStep) {
    float sum[1];
    if (finish_last(a.partial, a.Q, a.counter, lane, sum)) a.loss[0] = sum[0] * a.scale;
  }
}

// ---------------------------------------------------------------- RankNet
__global__ void __launch_bounds__(RR_WAVE) ranknet_fwd_kernel(const float* __restrict__ score, int64_t sstride,
                                                              const float* __restrict__ targets,
                                                              const int32_t* __restrict__ seg_off, int L, float sigma,
                                                              float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int q = blockIdx.x, lane = threadIdx.x;
  const int off = seg_off[q], C = seg_off[q + 1] - off;
  if (C <= 0) {
    if (lane == 0) {
      partial[2 * q] = 0.f;
      reinterpret_cast<int32_t*>(partial)[2 * q + 1] = 0;
    }
    return;
  }
  float* s = sm;
  float* t = sm + L;
  stage_list(s, t, score, sstride, targets, off, C, lane);
  // The pair costs are float32; their sum is kept in double: a lane adds C * C / 64 of them (a million at C = 8192), and a
  // float32 running sum of ~1e6 rounds every further cost of ~1 to 1/16 - 6.5e-4 of the loss at 8192, 1e-4 at 5462.
  double acc = 0.0;
  int npos = 0;
  for (int i = lane; i < C; i += RR_WAVE) {
    const float ti = t[i], si = s[i];
    for (int j = 0; j < C; ++j) {
      const float rel = ti - t[j];
      const float x = sigma * (si - s[j]);
      if (rel > 0.f) {
        ++npos;
        acc += static_cast<double>(logf(1.0f + expf(-x)));         // C_pos, train_pairwise.py:119 (naive, may be inf)
      } else if (rel < 0.f) {
        acc += static_cast<double>(logf(1.0f + expf(x)));          // C_neg, train_pairwise.py:120
      }
    }
  }
  const int tot = rr_wave_sum(npos);
  acc = rr_wave_sum(acc);
  if (lane == 0) {
    partial[2 * q] = tot > 0 ? static_cast<float>(acc) : 0.f;      // pair-less queries are skipped, :103-104
    reinterpret_cast<int32_t*>(partial)[2 * q + 1] = 2 * tot;      // num_pairs, train_pairwise.py:106
  }
}

// backward kept separate so lambdas never alias the staged scores
__global__ void __launch_bounds__(RR_WAVE) ranknet_bwd_kernel(const float* __restrict__ score, int64_t sstride,
                                                              const float* __restrict__ targets,
                                                              const int32_t* __restrict__ seg_off, int L, float sigma,
                                                              int mode, const float* __restrict__ gloss,
                                                              float* __restrict__ dscore, int64_t dstride) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int q = blockIdx.x, lane = threadIdx.x;
  const int off = seg_off[q], C = seg_off[q + 1] - off;
  if (C <= 0) return;
  float* s = sm;
  float* t = sm + L;
  float* lamv = sm + 2 * L;
  stage_list(s, t, score, sstride, targets, off, C, lane);
  int npos = 0;
  for (int i = lane; i < C; i += RR_WAVE) {
    const float ti = t[i], si = s[i];
    double lam = 0.0;                                              // (float32 terms summed in double, as the forward does:
    for (int j = 0; j < C; ++j) {                                  // a float32 row sum is 1.4e-5 of the largest lambda off at 8192)
      const float rel = ti - t[j];
      const float x = sigma * (si - s[j]);
      if (rel > 0.f) {
        ++npos;
        lam += static_cast<double>(-sigma / (1.0f + expf(x)));     // train_pairwise.py:126,128
      } else if (rel < 0.f) {
        lam += static_cast<double>(sigma / (1.0f + expf(-x)));     // train_pairwise.py:127,128
      }
    }
    lamv[i] = static_cast<float>(lam);
  }
  const int tot = rr_wave_sum(npos);
  // C_ij is symmetric, so d(sum_ij C_ij)/ds_i = 2 * lambda_i (mode 0); mode 1 = accelerate_grad's row sum
  const float g = tot > 0 ? gloss[0] * (mode == 0 ? 2.0f : 1.0f) : 0.f;
  for (int i = lane; i < C; i += RR_WAVE) dscore[static_cast<int64_t>(off + i) * dstride] = g * lamv[i];
}

// ---------------------------------------------------------------- final fixed-order reductions
__global__ void __launch_bounds__(256) reduce_scale_kernel(const float* __restrict__ partial, int64_t n, int64_t step,
                                                           float scale, float* __restrict__ out) {
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += 256) acc += partial[i * step];
  acc = block_sum(acc);
  if (threadIdx.x == 0) out[0] = acc * scale;
}

// ---------------------------------------------------------------- pointwise losses: MSE, Gaussian NLL, Lognorm, exp-MSE
// (rows: point_row<K>, loss_list.h).  Grid-stride; the forward leaves one partial per workgroup, the backward scales the
// rows' gradients by *gloss / n
template <int K, bool BWD>
__global__ void __launch_bounds__(256) pointwise_kernel(const float* __restrict__ x, const float* __restrict__ var,
                                                        int64_t stride, const float* __restrict__ targets, int64_t n,
                                                        float* __restrict__ partial, const float* __restrict__ gloss,
                                                        float* __restrict__ dx, float* __restrict__ dvar, int64_t dstride) {
  float g = 0.f, acc = 0.f;
  if constexpr (BWD) g = gloss[0] / static_cast<float>(n);
  const int64_t gs = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += gs) {
    float v = 0.f;
    if constexpr (point_has_var(K)) v = var[i * stride];
    const PointRow r = point_row<K>(x[i * stride], targets[i], v, g);
    if constexpr (BWD) {
      dx[i * dstride] = r.dmean;
      if constexpr (point_has_var(K)) dvar[i * dstride] = r.dvar;
    } else {
      acc += r.value;
    }
  }
  if constexpr (!BWD) {
    acc = block_sum(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
  }
}

// ---------------------------------------------------------------- ranking metrics (eval.py:475-555)
__global__ void __launch_bounds__(RR_WAVE) ranking_metrics_kernel(const float* __restrict__ score, int64_t sstride,
                                                                  const float* __restrict__ targets,
                                                                  const int32_t* __restrict__ seg_off, int L,
                                                                  double ratio, double ndcg_cut,
                                                                  int32_t* __restrict__ order,
                                                                  double* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int q = blockIdx.x, lane = threadIdx.x;
  const int off = seg_off[q], C = seg_off[q + 1] - off;
  double* st = stats + static_cast<int64_t>(q) * RR_RANKING_NSTATS;
  if (C <= 0) {
    if (lane < RR_RANKING_NSTATS) st[lane] = 0.0;
    return;
  }
  float* s = sm;
  float* t = sm + L;
  uint16_t* po = reinterpret_cast<uint16_t*>(sm + 2 * L);    // predicted order (list positions < 8192 fit 16 bits)
  uint16_t* to = po + L;                                     // target order
  uint16_t* pr = to + L;                                     // predicted rank of every candidate (inverse of po)
  uint16_t* tr = pr + L;                                     // target rank of every candidate (inverse of to)
  stage_list(s, t, score, sstride, targets, off, C, lane);
  for (int i = lane; i < C; i += RR_WAVE) {                   // stable descending ranks of both keys
    const float si = s[i], ti = t[i];
    int rp = 0, rt = 0;
    for (int j = 0; j < C; ++j) {
      const float sj = s[j], tj = t[j];
      rp += rr_precedes(sj, j, si, i) ? 1 : 0;
      rt += rr_precedes(tj, j, ti, i) ? 1 : 0;
    }
    po[rp] = static_cast<uint16_t>(i);
    to[rt] = static_cast<uint16_t>(i);
    pr[i] = static_cast<uint16_t>(rp);
    tr[i] = static_cast<uint16_t>(rt);
  }
  wave_sync();
  for (int r = lane; r < C; r += RR_WAVE) order[off + r] = po[r];
  int len25 = static_cast<int>(rint(static_cast<double>(C) * 0.25));   // python round(): half to even (:522)
  if (len25 < 1) len25 = 1;
  // recall@25%: predicted top-len25 that are in the target top-len25
  int hits = 0, hit0 = 0;
  for (int i = lane; i < len25; i += RR_WAVE) {
    const int pi = po[i];
    int in = 0;
    for (int j = 0; j < len25; ++j) in |= (to[j] == pi) ? 1 : 0;
    hits += in;
    if (i == 0) hit0 = in;
  }
  hits = rr_wave_sum(hits);
  hit0 = rr_wave_sum(hit0);
  // DCG sums with exp gains (compute_NDCG) over the first len25 / all positions, and exp2 gains over the first 10
  double d25 = 0, i25 = 0, dall = 0, iall = 0, d10 = 0, i10 = 0;
  for (int i = lane; i < C; i += RR_WAVE) {
    const double disc = log2(static_cast<double>(i) + 2.0);
    const double gp = exp(static_cast<double>(t[po[i]])), gt = exp(static_cast<double>(t[to[i]]));
    dall += gp / disc;
    iall += gt / disc;
    if (i < len25) { d25 += gp / disc; i25 += gt / disc; }
    if (i < 10) {
      d10 += (exp2(static_cast<double>(t[po[i]])) - 1.0) / disc;
      i10 += (exp2(static_cast<double>(t[to[i]])) - 1.0) / disc;
    }
  }
  d25 = rr_wave_sum(d25); i25 = rr_wave_sum(i25);
  dall = rr_wave_sum(dall); iall = rr_wave_sum(iall);
  d10 = rr_wave_sum(d10); i10 = rr_wave_sum(i10);
  // evaluate_top_scores (eval.py:76-177) at its `ratio`: cut = python round(C * ratio), at least 1 (:144-146);
  // recall of the predicted top-cut in the target top-cut (:147-151) and the TARGET's first maximum looked up in the
  // predicted top-cut (:156-159).  The first maximum (list.index(max)) is rank 0 of the stable descending order.
  int lenr = static_cast<int>(rint(static_cast<double>(C) * ratio));
  if (lenr < 1) lenr = 1;
  if (lenr > C) lenr = C;
  int hitr = 0;
  for (int i = lane; i < lenr; i += RR_WAVE) {
    const int pi = po[i];
    int in = 0;
    for (int j = 0; j < lenr; ++j) in |= (to[j] == pi) ? 1 : 0;
    hitr += in;
  }
  hitr = rr_wave_sum(hitr);
  // calculate_ndcg (eval.py:329-457): KL(softmax(targets) || softmax(scores)) with un-shifted f32 exponentials
  // (:401-404: an overflowing exp gives inf / inf = NaN there and here), and NDCG over the first ceil(C * cut)
  // positions of the TARGET order with rank-derived gains C + 1 - predicted rank (:406-425, cal_NDCG :309-325).
  double se_t = 0, se_s = 0;
  for (int i = lane; i < C; i += RR_WAVE) {
    se_t += static_cast<double>(expf(t[i]));
    se_s += static_cast<double>(expf(s[i]));
  }
  se_t = rr_wave_sum(se_t); se_s = rr_wave_sum(se_s);
  int ncut = static_cast<int>(ceil(static_cast<double>(C) * ndcg_cut));
  if (ncut > C) ncut = C;
  double kl = 0, dcut = 0, icut = 0;
  for (int i = lane; i < C; i += RR_WAVE) {
    const double P = static_cast<double>(expf(t[i])) / se_t, Qd = static_cast<double>(expf(s[i])) / se_s;
    kl += P * log(P / Qd);
    if (i < ncut) {
      // the reference ranks the predictions AFTER putting them in target order (:406-411), so a stable sort breaks
      // tied predictions by target rank, not by list position
      const int cand = to[i];
      const float sc = s[cand];
      int rank = 0;
      for (int j = 0; j < C; ++j) rank += rr_precedes(s[j], tr[j], sc, i) ? 1 : 0;
      const double disc = log2(static_cast<double>(i) + 2.0);
      dcut += static_cast<double>(C - rank) / disc;
      icut += static_cast<double>(C - i) / disc;
    }
  }
  kl = rr_wave_sum(kl); dcut = rr_wave_sum(dcut); icut = rr_wave_sum(icut);
  if (lane == 0) {
    st[8] = (pr[to[0]] < lenr) ? 1.0 : 0.0;
    st[9] = dcut / icut;
    st[10] = kl;
    st[11] = static_cast<double>(hitr) / static_cast<double>(lenr);
    const double p0 = exp(static_cast<double>(t[po[0]])), t0 = exp(static_cast<double>(t[to[0]]));
    double p2 = p0, t2 = t0;                                  // NDCG2: nested lists -> no discount (:543)
    if (C > 1) { p2 += exp(static_cast<double>(t[po[1]])); t2 += exp(static_cast<double>(t[to[1]])); }
    st[0] = (po[0] == to[0]) ? 1.0 : 0.0;
    st[1] = hit0 ? 1.0 : 0.0;
    st[2] = static_cast<double>(hits) / static_cast<double>(len25);
    st[3] = p0 / t0;
    st[4] = p2 / t2;
    st[5] = d25 / i25;
    st[6] = dall / iall;
    st[7] = d10 / i10;
  }
}

// ---------------------------------------------------------------- standalone LogCumsumExp
__global__ void __launch_bounds__(RR_WAVE) lce_fwd_kernel(const float* __restrict__ x, int n, float* __restrict__ y) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int lane = threadIdx.x;
  float* xs = sm;
  float* fd = sm + n;
  for (int i = lane; i < n; i += RR_WAVE) xs[i] = x[i];
  wave_sync();
  const float m = list_max(xs, n, lane);
  logcumsumexp_rev(xs, fd, n, lane, m);
  for (int i = lane; i < n; i += RR_WAVE) y[i] = fd[i];
}

__global__ void __launch_bounds__(RR_WAVE) lce_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                          const float* __restrict__ gy, int n, float* __restrict__ gx) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int lane = threadIdx.x;
  float* fd = sm;
  float* cs = sm + n;
  for (int i = lane; i < n; i += RR_WAVE) fd[i] = y[i];
  wave_sync();
  lce_backward(x, fd, cs, n, lane, [&](int i, float w) { gx[i] = gy[i] * w; });
}

// ---------------------------------------------------------------- evidential_loss_new (train/loss.py:402-437)
// NIG negative log-likelihood + lam * (|t - mu| (2 v + alpha) - eps) of parameter row i against target j.  Elementwise form:
// j = i.  Cross form (parameters [M, 1] against targets [M], what torch broadcasting makes of the trainer's call): all M x M
// pairs.  The device has lgammaf but no digamma: digamma_f below.
__device__ inline float digamma_f(float xf) {
  // recurrence psi(x) = psi(x + 1) - 1 / x up to x >= 6, then the asymptotic series; NaN for x <= 0 (alpha > 1 here)
  double x = xf, r = 0.0;
  if (!(x > 0.0)) return x == 0.0 ? -INFINITY : NAN;
  while (x < 6.0) {
    r -= 1.0 / x;
    x += 1.0;
  }
  const double f = 1.0 / (x * x);
  const double tail = f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (1.0 / 132)))));
  return static_cast<float>(r + log(x) - 0.5 / x - tail);
}

struct NigRow {
  float mu, v, a, b, omega, ap, lw, k;   // omega = 2 b (1 + v), ap = a + 1/2, lw = lam (2 v + a), k = target-free terms
  float cv, ca, cb;                      // target-free parts of d/dv, d/dalpha, d/dbeta
};

__device__ inline NigRow nig_row(float mu, float v, float a, float b, float lam, float eps, bool grads) {
  NigRow r;
  r.mu = mu; r.v = v; r.a = a; r.b = b;
  r.omega = 2.0f * b * (1.0f + v);
  r.ap = a + 0.5f;
  r.lw = lam * (2.0f * v + a);
  const float lo = logf(r.omega);
  r.k = 0.5f * logf(3.14159274101257324f / v) - a * lo + lgammaf(a) - lgammaf(r.ap) - lam * eps;   // float32(np.pi)
  r.cv = r.ca = r.cb = 0.f;
  if (grads) {
    r.cv = -0.5f / v - a / (1.0f + v);
    r.ca = -lo + (digamma_f(a) - digamma_f(r.ap));
    r.cb = -a / b;
  }
  return r;
}

__device__ inline float nig_loss(const NigRow& r, float t) {
  const float d = t - r.mu;
  return r.k + (r.ap * logf(r.v * d * d + r.omega) + r.lw * fabsf(d));
}

struct NigGrad {
  float mu, v, a, b;
};

__device__ inline void nig_grad_add(const NigRow& r, float t, float lam, NigGrad& g) {
  const float d = t - r.mu, ad = fabsf(d);
  const float qv = r.v * d * d + r.omega;
  g.mu += -2.0f * r.ap * r.v * d / qv - r.lw * sgnf(d);
  g.v += r.cv + (r.ap * (d * d + 2.0f * r.b) / qv + 2.0f * lam * ad);
  g.a += r.ca + (logf(qv) + lam * ad);
  g.b += r.cb + 2.0f * r.ap * (1.0f + r.v) / qv;
}

struct NigIn {
  const float* x[4];   // mu, v, alpha, beta
  int64_t st[4];
};

struct NigOut {
  float* d[4];
  int64_t st;
};

__device__ inline NigRow nig_load(const NigIn& in, int64_t i, float lam, float eps, bool grads) {
  return nig_row(in.x[0][i * in.st[0]], in.x[1][i * in.st[1]], in.x[2][i * in.st[2]], in.x[3][i * in.st[3]], lam, eps, grads);
}

// elementwise form: grid-stride, one partial per workgroup (pointwise_kernel's layout)
__global__ void __launch_bounds__(256) nig_elem_kernel(NigIn in, const float* __restrict__ targets, int64_t n, float lam,
                                                       float eps, int bwd, float* __restrict__ partial,
                                                       const float* __restrict__ gloss, NigOut out) {
  float acc = 0.f;
  const float g = bwd ? gloss[0] / static_cast<float>(n) : 0.f;
  const int64_t gs = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += gs) {
    const NigRow r = nig_load(in, i, lam, eps, bwd != 0);
    if (!bwd) {
      acc += nig_loss(r, targets[i]);
    } else {
      NigGrad d{0.f, 0.f, 0.f, 0.f};
      nig_grad_add(r, targets[i], lam, d);
      out.d[0][i * out.st] = g * d.mu;
      out.d[1][i * out.st] = g * d.v;
      out.d[2][i * out.st] = g * d.a;
      out.d[3][i * out.st] = g * d.b;
    }
  }
  if (bwd) return;                                                  // (uniform: no thread reaches the barriers below)
  acc = block_sum(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// cross form: a workgroup owns kNigRows parameter rows (lane = row) and its four waves split the targets, which stream
// through LDS in tiles of kNigTile; each wave takes a fixed quarter of every tile and the four per-row sums are added in
// wave order, so partial[i] (the row's sum over all M targets) has the same bits on every run
constexpr int kNigRows = RR_WAVE;
constexpr int kNigTile = 1024;

__global__ void __launch_bounds__(256) nig_cross_kernel(NigIn in, const float* __restrict__ targets, int64_t M, float lam,
                                                        float eps, int bwd, float* __restrict__ partial,
                                                        const float* __restrict__ gloss, NigOut out) {
  __shared__ float tile[kNigTile];
  __shared__ float red[4][4][kNigRows];
  const int lane = threadIdx.x % RR_WAVE, wave = threadIdx.x / RR_WAVE;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kNigRows + lane;
  const bool live = row < M;
  NigRow r{};
  if (live) r = nig_load(in, row, lam, eps, bwd != 0);
  float acc = 0.f;
  NigGrad d{0.f, 0.f, 0.f, 0.f};
  constexpr int part = kNigTile / 4;
  for (int64_t t0 = 0; t0 < M; t0 += kNigTile) {
    const int n = static_cast<int>(M - t0 < kNigTile ? M - t0 : kNigTile);
    __syncthreads();                                                // the previous tile is consumed
    for (int j = threadIdx.x; j < n; j += 256) tile[j] = targets[t0 + j];
    __syncthreads();
    if (live) {
      const int lo = wave * part, hi = min(lo + part, n);
      if (!bwd) {
        for (int j = lo; j < hi; ++j) acc += nig_loss(r, tile[j]);
      } else {
        for (int j = lo; j < hi; ++j) nig_grad_add(r, tile[j], lam, d);
      }
    }
  }
  red[0][wave][lane] = bwd ? d.mu : acc;
  red[1][wave][lane] = d.v;
  red[2][wave][lane] = d.a;
  red[3][wave][lane] = d.b;
  __syncthreads();
  if (wave != 0 || !live) return;
  float s[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = (red[k][0][lane] + red[k][1][lane]) + (red[k][2][lane] + red[k][3][lane]);
  if (!bwd) {
    partial[row] = s[0];
    return;
  }
  const float g = gloss[0] / (static_cast<float>(M) * static_cast<float>(M));
#pragma unroll
  for (int k = 0; k < 4; ++k) out.d[k][row * out.st] = g * s[k];
}

__global__ void __launch_bounds__(256) digamma_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ y) {
  const int64_t gs = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += gs) y[i] = digamma_f(x[i]);
}

int pointwise_blocks(int64_t n) {
  int64_t b = (n + 255) / 256;
  if (b < 1) b = 1;
  if (b > 1024) b = 1024;
  return static_cast<int>(b);
}

// the second launch of a forward entry point, and all of a step entry point that has no query: loss = scale * the sum of
// partial[n] in reduce_scale_kernel's fixed order.  st: the status of the launch before it, which a failure passes through
int finish_mean(int st, const float* partial, int n, float scale, float* loss, hipStream_t s) {
  if (st != RR_OK) return st;
  reduce_scale_kernel<<<1, 256, 0, s>>>(partial, n, 1, scale, loss);
  return rr_launch_status();
}

inline float inv_count(int64_t n) { return n > 0 ? 1.0f / static_cast<float>(n) : 0.f; }

inline bool strides_ok(const VarIn& in, int nin) {
  for (int k = 0; k < nin; ++k)
    if (!in.x[k] || in.st[k] < 1) return false;
  return true;
}

inline bool outs_ok(const VarOut& o, int nout) {
  for (int k = 0; k < nout; ++k)
    if (!o.d[k]) return false;
  return o.st >= 1;
}

// The host body of the 21 list entry points: argument check, list-length cap, launch, finish.  total: ListNet's candidate
// count (the other losses pass 0), coef: the UQ losses' penalty coefficient.  kForward needs loss and partial, kBackward
// gloss and out, kStep all but gloss.
template <int K>
int list_launch(int mode, const VarIn& in, const float* targets, const int32_t* seg_off, int Q, int max_len, int64_t total,
                float coef, float* loss, float* partial, unsigned int* counter, const float* gloss, const VarOut& out,
                rr_stream_t stream) {
  using Loss = ListLoss<K>;
  RR_CHECK_ARG(list_args_ok(in.x[0], targets, seg_off, Q, max_len) && strides_ok(in, Loss::kInputs) && total >= 0);
  RR_CHECK_ARG(mode == kBackward ? gloss != nullptr : loss && partial);
  RR_CHECK_ARG(mode == kForward || outs_ok(out, Loss::kInputs));
  RR_CHECK_ARG(mode != kStep || counter);
  if (max_len > kMaxLen) return RR_ERR_UNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // no candidate to rank: no gradient to write, and a step is the empty mean of the forward entry point.  (The forward still
  // launches for ListNet's total == 0: it owes the caller its Q zero partials.)
  const bool nothing = Q == 0 || (K == kListNet && total == 0);
  if (nothing && mode == kBackward) return RR_OK;
  if (nothing && mode == kStep) return finish_mean(RR_OK, partial, 0, 0.f, loss, s);
  const float scale = Loss::finish_scale(inv_count(Q), inv_count(total));
  const ListArgs a{in,   targets, seg_off, list_words(max_len), Q,    coef,   inv_count(total),
                   mode, partial, gloss,   out,                 scale, loss,  counter};
  const int st = launch_per_query(list_loss_kernel<K>, Q, a.L, Loss::kWords * sizeof(float), RR_WAVE, s, a);
  return mode == kForward ? finish_mean(st, partial, Q, scale, loss, s) : st;
}

inline VarIn cols(const float* x0, int64_t st0, const float* x1 = nullptr, int64_t st1 = 1, const float* x2 = nullptr,
                  int64_t st2 = 1) {
  return VarIn{{x0, x1, x2}, {st0, st1, st2}};
}

// The host body of the eight pointwise entry points.  The mean of nothing is NaN in the forward (torch.mean); the backward of
// nothing launches nothing.
template <int K, bool BWD>
int pointwise_launch(const float* x, const float* var, int64_t stride, const float* targets, int64_t n, float* loss,
                     float* partial, const float* gloss, float* dx, float* dvar, int64_t dstride, rr_stream_t stream) {
  RR_CHECK_ARG(x && (var || !point_has_var(K)) && targets && n >= 0 && stride >= 1);
  RR_CHECK_ARG(BWD ? gloss && dx && (dvar || !point_has_var(K)) && dstride >= 1 : loss && partial);
  if (BWD && n == 0) return RR_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nb = pointwise_blocks(n);
  pointwise_kernel<K, BWD><<<nb, 256, 0, s>>>(x, var, stride, targets, n, partial, gloss, dx, dvar, dstride);
  if (!BWD) reduce_scale_kernel<<<1, 256, 0, s>>>(partial, nb, 1, n > 0 ? 1.0f / static_cast<float>(n) : NAN, loss);
  return rr_launch_status();
}

int nig_launch(const NigIn& in, const float* targets, int64_t n, int cross, float lam, float eps, float* loss, float* partial,
               const float* gloss, const NigOut& out, rr_stream_t stream) {
  for (int k = 0; k < 4; ++k)
    if (!in.x[k] || in.st[k] < 1) return RR_ERR_ARG;
  if (!targets || n < 0 || (cross != 0 && cross != 1)) return RR_ERR_ARG;
  const int bwd = gloss != nullptr;
  if (bwd) {
    for (int k = 0; k < 4; ++k)
      if (!out.d[k]) return RR_ERR_ARG;
    if (out.st < 1) return RR_ERR_ARG;
    if (n == 0) return RR_OK;
  } else if (!loss || !partial) {
    return RR_ERR_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  int nb = 0;
  float scale = NAN;                                                 // torch.mean of nothing
  if (cross) {
    nb = static_cast<int>((n + kNigRows - 1) / kNigRows);
    if (n > 0) scale = 1.0f / (static_cast<float>(n) * static_cast<float>(n));
    if (nb > 0) nig_cross_kernel<<<nb, 256, 0, s>>>(in, targets, n, lam, eps, bwd, partial, gloss, out);
    if (!bwd) reduce_scale_kernel<<<1, 256, 0, s>>>(partial, n, 1, scale, loss);
  } else {
    nb = pointwise_blocks(n);
    if (n > 0) scale = 1.0f / static_cast<float>(n);
    nig_elem_kernel<<<nb, 256, 0, s>>>(in, targets, n, lam, eps, bwd, partial, gloss, out);
    if (!bwd) reduce_scale_kernel<<<1, 256, 0, s>>>(partial, nb, 1, scale, loss);
  }
  return rr_launch_status();
}

}  // namespace

extern "C" {

long long rr_lds_opt_ins(void) { return rr_lds_opt_in_count.load(std::memory_order_relaxed); }

// ---------------------------------------------------------------- the list losses: thin wrappers over list_launch<K>
int rr_listmle_fwd_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q,
                       int max_len, float* loss, float* partial, rr_stream_t stream) {
  return list_launch<kListMle>(kForward, cols(score, score_stride), targets, seg_off, Q, max_len, 0, 0.f, loss, partial, nullptr,
                               nullptr, VarOut{}, stream);
}

int rr_listmle_bwd_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q,
                       int max_len, const float* gloss, float* dscore, int64_t dscore_stride, rr_stream_t stream) {
  return list_launch<kListMle>(kBackward, cols(score, score_stride), targets, seg_off, Q, max_len, 0, 0.f, nullptr, nullptr,
                               nullptr, gloss, VarOut{{dscore}, dscore_stride}, stream);
}

int rr_listmle_step_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q, int max_len,
                        float* loss, float* partial, unsigned int* counter, float* dscore, int64_t dscore_stride,
                        rr_stream_t stream) {
  return list_launch<kListMle>(kStep, cols(score, score_stride), targets, seg_off, Q, max_len, 0, 0.f, loss, partial, counter,
                               nullptr, VarOut{{dscore}, dscore_stride}, stream);
}

int rr_listnet_fwd_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q,
                       int max_len, int64_t total, float* loss, float* partial, rr_stream_t stream) {
  return list_launch<kListNet>(kForward, cols(score, score_stride), targets, seg_off, Q, max_len, total, 0.f, loss, partial,
                               nullptr, nullptr, VarOut{}, stream);
}

int rr_listnet_bwd_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q,
                       int max_len, int64_t total, const float* gloss, float* dscore, int64_t dscore_stride,
                       rr_stream_t stream) {
  return list_launch<kListNet>(kBackward, cols(score, score_stride), targets, seg_off, Q, max_len, total, 0.f, nullptr, nullptr,
                               nullptr, gloss, VarOut{{dscore}, dscore_stride}, stream);
}

int rr_listnet_step_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q, int max_len,
                        int64_t total, float* loss, float* partial, unsigned int* counter, float* dscore, int64_t dscore_stride,
                        rr_stream_t stream) {
  return list_launch<kListNet>(kStep, cols(score, score_stride), targets, seg_off, Q, max_len, total, 0.f, loss, partial, counter,
                               nullptr, VarOut{{dscore}, dscore_stride}, stream);
}

int rr_evidential_ranking_fwd_f32(const float* mu, const float* var, int64_t stride, const float* targets,
                                  const int32_t* seg_off, int Q, int max_len, float* loss, float* partial,
                                  rr_stream_t stream) {
  return list_launch<kUcListwise>(kForward, cols(mu, stride, var, stride), targets, seg_off, Q, max_len, 0, 0.f, loss, partial,
                                  nullptr, nullptr, VarOut{}, stream);
}

int rr_evidential_ranking_bwd_f32(const float* mu, const float* var, int64_t stride, const float* targets,
                                  const int32_t* seg_off, int Q, int max_len, const float* gloss, float* dmu,
                                  float* dvar, int64_t dstride, rr_stream_t stream) {
  return list_launch<kUcListwise>(kBackward, cols(mu, stride, var, stride), targets, seg_off, Q, max_len, 0, 0.f, nullptr, nullptr,
                                  nullptr, gloss, VarOut{{dmu, dvar}, dstride}, stream);
}

int rr_evidential_ranking_step_f32(const float* mu, const float* var, int64_t stride, const float* targets, const int32_t* seg_off,
                                   int Q, int max_len, float* loss, float* partial, unsigned int* counter, float* dmu, float* dvar,
                                   int64_t dstride, rr_stream_t stream) {
  return list_launch<kUcListwise>(kStep, cols(mu, stride, var, stride), targets, seg_off, Q, max_len, 0, 0.f, loss, partial,
                                  counter, nullptr, VarOut{{dmu, dvar}, dstride}, stream);
}

#define RR_VAR2(NAME, K)                                                                                                        \
  int rr_##NAME##_fwd_f32(const float* mean, int64_t mean_stride, const float* var, int64_t var_stride, const float* targets,  \
                          const int32_t* seg_off, int Q, int max_len, float* loss, float* partial, rr_stream_t stream) {      \
    return list_launch<K>(kForward, cols(mean, mean_stride, var, var_stride), targets, seg_off, Q, max_len, 0, 0.f, loss,       \
                          partial, nullptr, nullptr, VarOut{}, stream);                                                        \
  }                                                                                                                              \
  int rr_##NAME##_bwd_f32(const float* mean, int64_t mean_stride, const float* var, int64_t var_stride, const float* targets,  \
                          const int32_t* seg_off, int Q, int max_len, const float* gloss, float* dmean, float* dvar,           \
                          int64_t dstride, rr_stream_t stream) {                                                               \
    return list_launch<K>(kBackward, cols(mean, mean_stride, var, var_stride), targets, seg_off, Q, max_len, 0, 0.f, nullptr,   \
                          nullptr, nullptr, gloss, VarOut{{dmean, dvar}, dstride}, stream);                                    \
  }

RR_VAR2(mledis, kMleDis)
RR_VAR2(listnet_gauss, kListnetGauss)
RR_VAR2(listnet_lognorm, kListnetLognorm)
#undef RR_VAR2

int rr_listnet_evidential_fwd_f32(const float* mean, int64_t mean_stride, const float* v, int64_t v_stride, const float* alpha,
                                  int64_t alpha_stride, const float* targets, const int32_t* seg_off, int Q, int max_len,
                                  float* loss, float* partial, rr_stream_t stream) {
  return list_launch<kListnetEvid>(kForward, cols(mean, mean_stride, v, v_stride, alpha, alpha_stride), targets, seg_off, Q,
                                   max_len, 0, 0.f, loss, partial, nullptr, nullptr, VarOut{}, stream);
}

int rr_listnet_evidential_bwd_f32(const float* mean, int64_t mean_stride, const float* v, int64_t v_stride, const float* alpha,
                                  int64_t alpha_stride, const float* targets, const int32_t* seg_off, int Q, int max_len,
                                  const float* gloss, float* dmean, float* dv, float* dalpha, int64_t dstride,
                                  rr_stream_t stream) {
  return list_launch<kListnetEvid>(kBackward, cols(mean, mean_stride, v, v_stride, alpha, alpha_stride), targets, seg_off, Q,
                                   max_len, 0, 0.f, nullptr, nullptr, nullptr, gloss, VarOut{{dmean, dv, dalpha}, dstride}, stream);
}

#define RR_VAR1(NAME, K)                                                                                                        \
  int rr_##NAME##_fwd_f32(const float* x, int64_t stride, const float* targets, const int32_t* seg_off, int Q, int max_len,     \
                          float coef, float* loss, float* partial, rr_stream_t stream) {                                       \
    return list_launch<K>(kForward, cols(x, stride), targets, seg_off, Q, max_len, 0, coef, loss, partial, nullptr, nullptr,    \
                          VarOut{}, stream);                                                                                   \
  }                                                                                                                              \
  int rr_##NAME##_bwd_f32(const float* x, int64_t stride, const float* targets, const int32_t* seg_off, int Q, int max_len,     \
                          float coef, const float* gloss, float* dx, int64_t dstride, rr_stream_t stream) {                    \
    return list_launch<K>(kBackward, cols(x, stride), targets, seg_off, Q, max_len, 0, coef, nullptr, nullptr, nullptr, gloss,  \
                          VarOut{{dx}, dstride}, stream);                                                                      \
  }

RR_VAR1(listnet_uq, kListnetUq)
RR_VAR1(dirichlet_uq, kDirichletUq)
#undef RR_VAR1

int rr_ranknet_fwd_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q,
                       int max_len, float sigma, float* loss_sum, int64_t* pairs, float* partial,
                       rr_stream_t stream) {
  RR_CHECK_ARG(list_args_ok(score, targets, seg_off, Q, max_len) && loss_sum && pairs && partial && score_stride >= 1);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int st = launch_list(ranknet_fwd_kernel, 2 * sizeof(float), score, score_stride, targets, seg_off, Q, max_len, s, sigma, partial);
  if (st != RR_OK) return st;
  finish_counted_kernel<<<1, RR_WAVE, 0, s>>>(partial, Q, 1.0f, loss_sum, pairs);
  return rr_launch_status();
}

int rr_ranknet_bwd_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q,
                       int max_len, float sigma, int mode, const float* gloss, float* dscore, int64_t dscore_stride,
                       rr_stream_t stream) {
  RR_CHECK_ARG(list_args_ok(score, targets, seg_off, Q, max_len) && gloss && dscore && score_stride >= 1 &&
               dscore_stride >= 1 && (mode == 0 || mode == 1));
  return launch_list(ranknet_bwd_kernel, 3 * sizeof(float), score, score_stride, targets, seg_off, Q, max_len,
                     static_cast<hipStream_t>(stream), sigma, mode, gloss, dscore, dscore_stride);
}

int64_t rr_pointwise_partial_count(int64_t n) { return pointwise_blocks(n); }

int rr_mse_fwd_f32(const float* pred, int64_t stride, const float* targets, int64_t n, float* loss, float* partial,
                   rr_stream_t stream) {
  return pointwise_launch<kPointMse, false>(pred, nullptr, stride, targets, n, loss, partial, nullptr, nullptr, nullptr, 1, stream);
}

int rr_mse_bwd_f32(const float* pred, int64_t stride, const float* targets, int64_t n, const float* gloss,
                   float* dpred, int64_t dstride, rr_stream_t stream) {
  return pointwise_launch<kPointMse, true>(pred, nullptr, stride, targets, n, nullptr, nullptr, gloss, dpred, nullptr, dstride, stream);
}

int rr_gauss_nll_fwd_f32(const float* mean, const float* var, int64_t stride, const float* targets, int64_t n,
                         float* loss, float* partial, rr_stream_t stream) {
  return pointwise_launch<kPointGauss, false>(mean, var, stride, targets, n, loss, partial, nullptr, nullptr, nullptr, 1, stream);
}

int rr_gauss_nll_bwd_f32(const float* mean, const float* var, int64_t stride, const float* targets, int64_t n,
                         const float* gloss, float* dmean, float* dvar, int64_t dstride, rr_stream_t stream) {
  return pointwise_launch<kPointGauss, true>(mean, var, stride, targets, n, nullptr, nullptr, gloss, dmean, dvar, dstride, stream);
}

int rr_lognorm_fwd_f32(const float* score, const float* var, int64_t stride, const float* targets, int64_t n, float* loss,
                       float* partial, rr_stream_t stream) {
  return pointwise_launch<kPointLognorm, false>(score, var, stride, targets, n, loss, partial, nullptr, nullptr, nullptr, 1, stream);
}

int rr_lognorm_bwd_f32(const float* score, const float* var, int64_t stride, const float* targets, int64_t n, const float* gloss,
                       float* dscore, float* dvar, int64_t dstride, rr_stream_t stream) {
  return pointwise_launch<kPointLognorm, true>(score, var, stride, targets, n, nullptr, nullptr, gloss, dscore, dvar, dstride, stream);
}

int rr_exp_mse_fwd_f32(const float* pred, int64_t stride, const float* targets, int64_t n, float* loss, float* partial,
                       rr_stream_t stream) {
  return pointwise_launch<kPointExpMse, false>(pred, nullptr, stride, targets, n, loss, partial, nullptr, nullptr, nullptr, 1, stream);
}

int rr_exp_mse_bwd_f32(const float* pred, int64_t stride, const float* targets, int64_t n, const float* gloss, float* dpred,
                       int64_t dstride, rr_stream_t stream) {
  return pointwise_launch<kPointExpMse, true>(pred, nullptr, stride, targets, n, nullptr, nullptr, gloss, dpred, nullptr, dstride, stream);
}

int rr_ranking_metrics_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off,
                           int Q, int max_len, double ratio, double ndcg_cut, int32_t* order, double* stats,
                           rr_stream_t stream) {
  RR_CHECK_ARG(list_args_ok(score, targets, seg_off, Q, max_len) && order && stats && score_stride >= 1);
  RR_CHECK_ARG(ratio >= 0.0 && ratio <= 1.0 && ndcg_cut >= 0.0 && ndcg_cut <= 1.0);
  return launch_list(ranking_metrics_kernel, 2 * sizeof(float) + 4 * sizeof(uint16_t), score, score_stride, targets, seg_off, Q,
                     max_len, static_cast<hipStream_t>(stream), ratio, ndcg_cut, order, stats);
}

int rr_logcumsumexp_fwd_f32(const float* x, int n, float* y, rr_stream_t stream) {
  RR_CHECK_ARG(x && y && n >= 0);
  if (n > kMaxLen) return RR_ERR_UNSUPPORTED;
  if (n == 0) return RR_OK;
  const size_t lds = 2u * n * sizeof(float);
  if (set_lds(lce_fwd_kernel, lds) != RR_OK) return RR_ERR_LAUNCH;
  lce_fwd_kernel<<<1, RR_WAVE, lds, static_cast<hipStream_t>(stream)>>>(x, n, y);
  return rr_launch_status();
}

int rr_logcumsumexp_bwd_f32(const float* x, const float* y, const float* gy, int n, float* gx, rr_stream_t stream) {
  RR_CHECK_ARG(x && y && gy && gx && n >= 0);
  if (n > kMaxLen) return RR_ERR_UNSUPPORTED;
  if (n == 0) return RR_OK;
  const size_t lds = 2u * n * sizeof(float);
  if (set_lds(lce_bwd_kernel, lds) != RR_OK) return RR_ERR_LAUNCH;
  lce_bwd_kernel<<<1, RR_WAVE, lds, static_cast<hipStream_t>(stream)>>>(x, y, gy, n, gx);
  return rr_launch_status();
}

// ---------------------------------------------------------------- evidential_loss_new
int rr_nig_fwd_f32(const float* mu, int64_t mu_stride, const float* v, int64_t v_stride, const float* alpha, int64_t alpha_stride,
                   const float* beta, int64_t beta_stride, const float* targets, int64_t n, int cross, float lam, float epsilon,
                   float* loss, float* partial, rr_stream_t stream) {
  const NigIn in{{mu, v, alpha, beta}, {mu_stride, v_stride, alpha_stride, beta_stride}};
  return nig_launch(in, targets, n, cross, lam, epsilon, loss, partial, nullptr, NigOut{}, stream);
}

int rr_nig_bwd_f32(const float* mu, int64_t mu_stride, const float* v, int64_t v_stride, const float* alpha, int64_t alpha_stride,
                   const float* beta, int64_t beta_stride, const float* targets, int64_t n, int cross, float lam,
                   const float* gloss, float* dmu, float* dv, float* dalpha, float* dbeta, int64_t dstride, rr_stream_t stream) {
  if (!gloss) return RR_ERR_ARG;
  const NigIn in{{mu, v, alpha, beta}, {mu_stride, v_stride, alpha_stride, beta_stride}};
  return nig_launch(in, targets, n, cross, lam, 0.f, nullptr, nullptr, gloss, NigOut{{dmu, dv, dalpha, dbeta}, dstride}, stream);
}

int rr_digamma_f32(const float* x, int64_t n, float* y, rr_stream_t stream) {
  RR_CHECK_ARG(x && y && n >= 0);
  if (n == 0) return RR_OK;
  digamma_kernel<<<pointwise_blocks(n), 256, 0, static_cast<hipStream_t>(stream)>>>(x, n, y);
  return rr_launch_status();
}

}  // extern "C"
