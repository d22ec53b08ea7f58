// The per-list loss terms, each defined ONCE for every kernel that evaluates it (loss.hip: list_loss_kernel, one shell over
// the nine list losses; task_loss.hip: the composite one-launch step).  One 64-lane wavefront owns one list staged in LDS;
// only wave-level synchronisation.
//
// A term is a small struct built over the staged list (its constructor does the work forward and gradient share: ranking,
// softmax statistics, scans) with
//   forward()          the list's UN-NORMALISED wave sum (UqTerm: two sums), valid in every lane;
//   gradient(g, emit)  calls emit(row, g0[, g1[, g2]]) once per candidate - row is the candidate's position in the list as
//                      staged, g0.. the gradient of its input columns for the caller's scale g.
// The kernel shell owns the rest: where the list lies in LDS (the term takes pointers), any transform of its inputs, and
// every normaliser (1 / C, 1 / Q, 1 / total, the upstream gradient).  No term divides by a count.
// Next to each term, ListLoss<K> holds what list_loss_kernel needs to know of the loss: kInputs input columns, kWords staged
// words per candidate, term() the term over the staged list, partial() the query's loss from forward(), grad_scale() the g of
// gradient() and finish_scale() what the sum of the partials is multiplied with.  The normalisers differ between the losses
// on purpose, and in bits: they are the reference's expressions, not to be aligned.
// The library is built with -ffp-contract=off and no fast-math, so an expression has the same bits in every kernel it is
// inlined into.
#pragma once
#include "wave_util.h"

namespace {

struct ListView {
  float* s;       // scores (as given): input column 0
  float* t;       // targets
  float* ss;      // scores sorted by target, descending (ListMLE); input column 1 of the losses that have one
  int32_t* perm;  // perm[j] = original position of sorted element j (ListMLE, MLEDis); input column 2 (ListNet-evidential)
  float* aux;     // scratch (fd values)
  __device__ float* col(int k) const { return k == 0 ? s : k == 1 ? ss : reinterpret_cast<float*>(perm); }   // input column k
};

// the one LDS layout of the list kernels: five arrays of L words, of which a kernel allocates the leading ones it uses
__device__ inline ListView carve(float* sm, int L) {
  ListView v;
  v.s = sm;
  v.t = sm + L;
  v.ss = sm + 2 * L;
  v.perm = reinterpret_cast<int32_t*>(sm + 3 * L);
  v.aux = sm + 4 * L;
  return v;
}

// rank by target, descending, ties by original index (stable); scatters s into ss / perm.
__device__ inline void rank_sort(const ListView& v, int C, int lane) {
  for (int i = lane; i < C; i += RR_WAVE) {
    const float ti = v.t[i];
    int r = 0;
    for (int j = 0; j < C; ++j) r += rr_precedes(v.t[j], j, ti, i) ? 1 : 0;
    v.ss[r] = v.s[i];
    v.perm[r] = i;
  }
  wave_sync();
}

__device__ inline float list_max(const float* a, int C, int lane) {
  float m = -INFINITY;
  for (int i = lane; i < C; i += RR_WAVE) m = fmaxf(m, a[i]);
  return rr_wave_max(m);
}

// fd[j] = log(sum_{i>=j} exp(x[i] - m)) + m for the C values in x (LogCumsumExp.forward,
// train/loss.py:28-34).  Each lane owns the contiguous chunk [lo, hi); fd may be x (a lane reads [j] before it writes [j]).
__device__ inline void logcumsumexp_rev(const float* x, float* fd, int C, int lane, float m) {
  const int E = (C + RR_WAVE - 1) / RR_WAVE;
  const int lo = min(lane * E, C), hi = min(lo + E, C);
  float local = 0.f;
  for (int j = hi - 1; j >= lo; --j) local += expf(x[j] - m);
  // suffix sums over lanes without subtraction: scan the lane-reversed values
  const float rev = __shfl(local, RR_WAVE - 1 - lane, RR_WAVE);
  const float incl_rev = rr_wave_incl_scan(rev, lane);
  const float suffix_incl = __shfl(incl_rev, RR_WAVE - 1 - lane, RR_WAVE);   // sum over lanes >= lane
  const float nxt = __shfl_down(suffix_incl, 1, RR_WAVE);
  float run = (lane == RR_WAVE - 1) ? 0.f : nxt;                             // sum over lanes > lane, no subtraction
  for (int j = hi - 1; j >= lo; --j) {
    run += expf(x[j] - m);
    fd[j] = logf(run) + m;
  }
  wave_sync();
}

// cs[j] = sum_{i<=j} v(i), v(i) = exp(-fd[i]); returned through out[], which may be fd itself (same chunks as above).
__device__ inline void cumsum_exp_neg(const float* fd, float* out, int C, int lane) {
  const int E = (C + RR_WAVE - 1) / RR_WAVE;
  const int lo = min(lane * E, C), hi = min(lo + E, C);
  float local = 0.f;
  for (int j = lo; j < hi; ++j) local += expf(-fd[j]);
  const float incl = rr_wave_incl_scan(local, lane);
  const float prev = __shfl_up(incl, 1, RR_WAVE);
  float run = lane == 0 ? 0.f : prev;
  for (int j = lo; j < hi; ++j) {
    run += expf(-fd[j]);
    out[j] = run;
  }
  wave_sync();
}

// LogCumsumExp.backward for an upstream gradient of ones: emit(j, exp(x[j]) * cs[j]); it keeps the un-shifted exp(x)
// (loss.py:59).  x may be global memory; cs is LDS scratch and may be fd.
template <typename Emit>
__device__ inline void lce_backward(const float* x, const float* fd, float* cs, int C, int lane, Emit emit) {
  cumsum_exp_neg(fd, cs, C, lane);
  for (int j = lane; j < C; j += RR_WAVE) emit(j, expf(x[j]) * cs[j]);
}

__device__ inline void softmax_stats(const float* a, int C, int lane, float* mx, float* sum) {
  const float m = list_max(a, C, lane);
  float s = 0.f;
  for (int i = lane; i < C; i += RR_WAVE) s += expf(a[i] - m);
  *mx = m;
  *sum = rr_wave_sum(s);
}

enum ListLossKind : int {
  kListMle, kListNet, kUcListwise, kMleDis, kListnetGauss, kListnetLognorm, kListnetEvid, kListnetUq, kDirichletUq
};

// what a list loss's normalisers are made of: the list's length, the window's query count, 1 / its candidate count
// (ListNet alone) and the penalty coefficient (the UQ losses alone)
struct ListNorm {
  int C, Q;
  float inv_total, coef;
};

// The normalisers most losses share: a mean over the list (in partial()), then a mean over the queries.  gl: the upstream gradient
struct PerQueryMean {
  __device__ static float grad_scale(float gl, const ListNorm& n) { return gl / (static_cast<float>(n.C) * static_cast<float>(n.Q)); }
  static float finish_scale(float inv_queries, float /*inv_total*/) { return inv_queries; }
};

template <int K>
struct ListLoss;

__device__ inline float sgnf(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }   // torch.abs' gradient

// softmax of a staged list: p(i) = exp(a[i] - max) / sum
struct Softmax {
  const float* a;
  float m, z;
  __device__ Softmax(const float* a_, int C, int lane) : a(a_) { softmax_stats(a, C, lane, &m, &z); }
  __device__ float operator()(int i) const { return expf(a[i] - m) / z; }
  __device__ float total(int C, int lane) const {                  // sum_i p(i) as float32 adds it (not exactly one)
    float s = 0.f;
    for (int i = lane; i < C; i += RR_WAVE) s += (*this)(i);
    return rr_wave_sum(s);
  }
};

// ---------------------------------------------------------------- ListMLE (train/loss.py:64-99)
// sum_j (fd_j - ss_j) over the list sorted by target.  Needs all five arrays of v; forward() before gradient(), which
// overwrites fd with its cumulative sum.
struct ListMleTerm {
  ListView v;
  int C, lane;
  __device__ ListMleTerm(const ListView& v_, int C_, int lane_) : v(v_), C(C_), lane(lane_) {
    rank_sort(v, C, lane);
    const float m = list_max(v.ss, C, lane);
    logcumsumexp_rev(v.ss, v.aux, C, lane, m);
  }
  __device__ float forward() const {
    float acc = 0.f;
    for (int i = lane; i < C; i += RR_WAVE) acc += v.aux[i] - v.ss[i];
    return rr_wave_sum(acc);
  }
  template <typename Emit>
  __device__ void gradient(float g, Emit emit) const {
    lce_backward(v.ss, v.aux, v.aux, C, lane, [&](int j, float w) { emit(v.perm[j], g * w - g); });   // "- g": d(-sorted_item)
  }
};

template <>
struct ListLoss<kListMle> : PerQueryMean {
  static constexpr int kInputs = 1, kWords = 5;
  __device__ static ListMleTerm term(const ListView& v, const ListNorm& n, int lane) { return ListMleTerm(v, n.C, lane); }
  __device__ static float partial(float acc, const ListNorm& n) { return acc / static_cast<float>(n.C); }   // torch.mean, loss.py:94
};

// ---------------------------------------------------------------- ListNet top-1 (train/loss.py:317-352)
struct ListNetTerm {
  Softmax ps, pt;
  int C, lane;
  __device__ ListNetTerm(const float* s, const float* t, int C_, int lane_) : ps(s, C_, lane_), pt(t, C_, lane_), C(C_), lane(lane_) {}
  __device__ float forward() const {
    float acc = 0.f;
    for (int i = lane; i < C; i += RR_WAVE) {
      const float pred = logf(ps(i));                               // torch.log(F.softmax(item)), loss.py:339
      const float targ = pt(i);                                     // loss.py:341
      acc += -targ * pred;                                          // loss.py:343
    }
    return rr_wave_sum(acc);
  }
  template <typename Emit>
  __device__ void gradient(float g, Emit emit) const {
    const float tsum = pt.total(C, lane);
    for (int i = lane; i < C; i += RR_WAVE) emit(i, g * (ps(i) * tsum - pt(i)));
  }
};

// ONE mean over all candidates (loss.py:347): the partial is the raw sum, 1 / total scales the gradient and the finish
template <>
struct ListLoss<kListNet> {
  static constexpr int kInputs = 1, kWords = 2;
  __device__ static ListNetTerm term(const ListView& v, const ListNorm& n, int lane) { return ListNetTerm(v.s, v.t, n.C, lane); }
  __device__ static float partial(float acc, const ListNorm&) { return acc; }
  __device__ static float grad_scale(float gl, const ListNorm& n) { return gl * n.inv_total; }
  static float finish_scale(float /*inv_queries*/, float inv_total) { return inv_total; }
};

// ---------------------------------------------------------------- evidential UC-Listwise (train/loss.py:477-556)
// emit(row, d / d mu, d / d var)
struct UcListwiseTerm {
  const float *s, *t, *vv;
  Softmax ps, pt;
  int C, lane;
  __device__ UcListwiseTerm(const float* s_, const float* vv_, const float* t_, int C_, int lane_)
      : s(s_), t(t_), vv(vv_), ps(s_, C_, lane_), pt(t_, C_, lane_), C(C_), lane(lane_) {}
  __device__ float forward() const {
    const float two_pi = 2.0f * 3.141592653f;                       // loss.py:543 (truncated pi)
    float acc = 0.f;
    for (int i = lane; i < C; i += RR_WAVE) {
      const float lp = logf(ps(i));
      const float lt = logf(pt(i));
      const float d = lt - lp;
      const float unc = 0.5f * (d * d) / vv[i] + 0.5f * logf(two_pi * vv[i]);   // loss.py:541-543
      const float pen = fabsf(s[i] - t[i]);                                       // loss.py:545
      acc += -lt + unc + pen;                                                      // loss.py:549
    }
    return rr_wave_sum(acc);
  }
  template <typename Emit>
  __device__ void gradient(float g, Emit emit) const {
    float csum = 0.f;
    for (int i = lane; i < C; i += RR_WAVE) {
      const float lp = logf(ps(i));
      const float lt = logf(pt(i));
      csum += -(lt - lp) / vv[i];
    }
    csum = rr_wave_sum(csum);
    for (int i = lane; i < C; i += RR_WAVE) {
      const float p = ps(i);
      const float lp = logf(p);
      const float lt = logf(pt(i));
      const float d = lt - lp;
      const float c = -d / vv[i];
      emit(i, g * (c - p * csum + sgnf(s[i] - t[i])), g * (-0.5f * d * d / (vv[i] * vv[i]) + 0.5f / vv[i]));
    }
  }
};

template <>
struct ListLoss<kUcListwise> : PerQueryMean {
  static constexpr int kInputs = 2, kWords = 3;
  __device__ static UcListwiseTerm term(const ListView& v, const ListNorm& n, int lane) {
    return UcListwiseTerm(v.s, v.ss, v.t, n.C, lane);
  }
  __device__ static float partial(float acc, const ListNorm& n) { return acc / static_cast<float>(n.C); }
};

// ---------------------------------------------------------------- the listwise variants (train/loss.py:102-141, 187-314,
// 355-399, 440-474).  The C x C pair sums of MLEDis, ListNet-Gauss and ListNet-lognorm are factorised into per-element terms
// (DESIGN section 2), so a list costs O(C) - except MLEDis' gradient and the target ranking, O(C^2 / 64).

// MLEDisLoss: sorted by target (descending, stable); a_j = s_j + v_j / 2, F_j = log sum_{i>=j} exp(a_i);
// sum_j log sum_{i>=j} exp(s_i - s_j + (v_i + v_j) / 2) = sum_j (F_j - s_j + v_j / 2).  x0, x1, t are read; perm and F are
// written.  The sorted a_j go where the targets were, which are not read again - or, with KEEP_T (a caller that still needs
// them), to F, where F_j replaces them in place; gradient() then adds a_k up again (the same bits, a few more registers).
// emit(row, d / d s, d / d v)
template <bool KEEP_T>
struct MleDisTerm {
  const float *x0, *x1;
  const int32_t* perm;
  const float *sa, *F;
  int C, lane;
  __device__ MleDisTerm(float* x0_, const float* x1_, float* t, int32_t* perm_, float* F_, int C_, int lane_)
      : x0(x0_), x1(x1_), perm(perm_), sa(KEEP_T ? F_ : t), F(F_), C(C_), lane(lane_) {
    const ListView lv{x0_, t, F_, perm_, nullptr};                  // the sorted scores are scratch, overwritten below
    rank_sort(lv, C, lane);
    float* sa_ = KEEP_T ? F_ : t;
    for (int r = lane; r < C; r += RR_WAVE) sa_[r] = a(perm_[r]);
    wave_sync();
    const float m = list_max(sa_, C, lane);
    logcumsumexp_rev(sa_, F_, C, lane, m);
  }
  __device__ float a(int p) const { return x0[p] + 0.5f * x1[p]; }
  __device__ float forward() const {
    float acc = 0.f;
    for (int r = lane; r < C; r += RR_WAVE) {
      const int p = perm[r];
      acc += F[r] + (0.5f * x1[p] - x0[p]);
    }
    return rr_wave_sum(acc);
  }
  template <typename Emit>
  __device__ void gradient(float g, Emit emit) const {
    // d / d a_k = g sum_{j<=k} exp(a_k - F_j): every term is <= 1, so the pair form cannot overflow
    for (int k = lane; k < C; k += RR_WAVE) {
      const float ak = KEEP_T ? a(perm[k]) : sa[k];
      float G = 0.f;
      for (int j = 0; j <= k; ++j) G += expf(ak - F[j]);
      emit(perm[k], g * (G - 1.0f), g * 0.5f * (G + 1.0f));
    }
  }
};

// the variants multiply with the rounded 1 / C where ListMLE and UC-Listwise divide by C
struct VariantMean : PerQueryMean {
  __device__ static float partial(float acc, const ListNorm& n) { return acc * (1.0f / static_cast<float>(n.C)); }
};

template <>
struct ListLoss<kMleDis> : VariantMean {
  static constexpr int kInputs = 2, kWords = 5;   // x0, t, x1, perm, F
  __device__ static MleDisTerm<false> term(const ListView& v, const ListNorm& n, int lane) {
    return MleDisTerm<false>(v.s, v.ss, v.t, v.perm, v.aux, n.C, lane);
  }
};

// Listnet_For_Gauss: log sum_j exp(s_j - s_i + (v_i + v_j) / 2) = LSE_j(s_j + v_j / 2) - s_i + v_i / 2.  emit(row, d / d s, d / d v)
struct ListNetGaussTerm {
  const float *x0, *x1;
  Softmax pt;
  float lse;
  int C, lane;
  __device__ ListNetGaussTerm(const float* x0_, const float* x1_, const float* t, int C_, int lane_)
      : x0(x0_), x1(x1_), pt(t, C_, lane_), C(C_), lane(lane_) {
    float ma = -INFINITY;
    for (int i = lane; i < C; i += RR_WAVE) ma = fmaxf(ma, x0[i] + 0.5f * x1[i]);
    ma = rr_wave_max(ma);
    float za = 0.f;
    for (int i = lane; i < C; i += RR_WAVE) za += expf(x0[i] + 0.5f * x1[i] - ma);
    za = rr_wave_sum(za);
    lse = ma + logf(za);
  }
  __device__ float forward() const {
    float acc = 0.f;
    for (int i = lane; i < C; i += RR_WAVE) acc += pt(i) * (lse + (0.5f * x1[i] - x0[i]));
    return rr_wave_sum(acc);
  }
  template <typename Emit>
  __device__ void gradient(float g, Emit emit) const {
    const float tsum = pt.total(C, lane);
    for (int k = lane; k < C; k += RR_WAVE) {
      const float pk = expf(x0[k] + 0.5f * x1[k] - lse), tk = pt(k);
      emit(k, g * (tsum * pk - tk), g * 0.5f * (tsum * pk + tk));
    }
  }
};

template <>
struct ListLoss<kListnetGauss> : VariantMean {
  static constexpr int kInputs = 2, kWords = 3;
  __device__ static ListNetGaussTerm term(const ListView& v, const ListNorm& n, int lane) {
    return ListNetGaussTerm(v.s, v.ss, v.t, n.C, lane);
  }
};

// Listnetlognorm: log sum_j (s_j / s_i) exp((v_i + v_j) / 2) = log(W / s_i) + (v_i + mv) / 2, W = sum_j s_j exp((v_j - mv) / 2):
// the sign of W / s_i is the sign of the reference's sum, so log() of a negative one is NaN here as there.
// emit(row, d / d s, d / d v)
struct ListNetLognormTerm {
  const float *x0, *x1;
  Softmax pt;
  float mv, W;
  int C, lane;
  __device__ ListNetLognormTerm(const float* x0_, const float* x1_, const float* t, int C_, int lane_)
      : x0(x0_), x1(x1_), pt(t, C_, lane_), C(C_), lane(lane_) {
    mv = list_max(x1, C, lane);
    float w = 0.f;
    for (int i = lane; i < C; i += RR_WAVE) w += x0[i] * expf(0.5f * (x1[i] - mv));
    W = rr_wave_sum(w);
  }
  __device__ float forward() const {
    float acc = 0.f;
    for (int i = lane; i < C; i += RR_WAVE) acc += pt(i) * (logf(W / x0[i]) + 0.5f * (x1[i] + mv));
    return rr_wave_sum(acc);
  }
  template <typename Emit>
  __device__ void gradient(float g, Emit emit) const {
    const float tsum = pt.total(C, lane);
    for (int k = lane; k < C; k += RR_WAVE) {
      const float ek = expf(0.5f * (x1[k] - mv)), tk = pt(k);
      emit(k, g * (tsum * ek / W - tk / x0[k]), g * 0.5f * (tsum * x0[k] * ek / W + tk));
    }
  }
};

template <>
struct ListLoss<kListnetLognorm> : VariantMean {
  static constexpr int kInputs = 2, kWords = 3;
  __device__ static ListNetLognormTerm term(const ListView& v, const ListNorm& n, int lane) {
    return ListNetLognormTerm(v.s, v.ss, v.t, n.C, lane);
  }
};

// Listnet_For_evidential: forward() is sum_i softmax(t)_i * log_softmax(s)_i * (2 v_i + alpha_i); the loss is its NEGATIVE
// mean (the caller's sign, with its normaliser), and gradient() is the gradient of that loss.  emit(row, d / d s, d / d v, d / d alpha)
struct ListNetEvidTerm {
  const float *x0, *x1, *x2;
  Softmax ps, pt;
  float lz;
  int C, lane;
  __device__ ListNetEvidTerm(const float* x0_, const float* x1_, const float* x2_, const float* t, int C_, int lane_)
      : x0(x0_), x1(x1_), x2(x2_), ps(x0_, C_, lane_), pt(t, C_, lane_), C(C_), lane(lane_) {
    lz = logf(ps.z);
  }
  __device__ float forward() const {
    float acc = 0.f;
    for (int i = lane; i < C; i += RR_WAVE) acc += pt(i) * ((x0[i] - ps.m) - lz) * (2.0f * x1[i] + x2[i]);
    return rr_wave_sum(acc);
  }
  template <typename Emit>
  __device__ void gradient(float g, Emit emit) const {
    float wsum = 0.f;
    for (int i = lane; i < C; i += RR_WAVE) wsum += pt(i) * (2.0f * x1[i] + x2[i]);
    wsum = rr_wave_sum(wsum);
    for (int k = lane; k < C; k += RR_WAVE) {
      const float tk = pt(k), lsk = (x0[k] - ps.m) - lz, pk = ps(k);
      emit(k, -g * (tk * (2.0f * x1[k] + x2[k]) - pk * wsum), -g * 2.0f * tk * lsk, -g * tk * lsk);
    }
  }
};

template <>
struct ListLoss<kListnetEvid> : PerQueryMean {
  static constexpr int kInputs = 3, kWords = 4;
  __device__ static ListNetEvidTerm term(const ListView& v, const ListNorm& n, int lane) {
    return ListNetEvidTerm(v.s, v.ss, v.col(2), v.t, n.C, lane);
  }
  __device__ static float partial(float acc, const ListNorm& n) { return -(acc * (1.0f / static_cast<float>(n.C))); }
};

// Listnet_with_uq (DIRICHLET false): p = s / sum(s); KL(softmax(t) || p) / C + coef * mean_i |log(softmax(t)_i / p_i) (s_i - 1)|
// Dirichlet_uq (true): p = a / S, S = sum(a); mean_i (p_i - sm_i)^2 + p_i (1 - p_i) / (S + 1) + coef * |log(sm_i / p_i) (a_i - 1)|
// forward() returns the two sums apart (the caller forms acc / C + coef * (pen / C)); emit(row, d / d x)
struct UqSums {
  float acc, pen;
};

template <bool DIRICHLET>
struct UqTerm {
  const float* x0;
  Softmax pt;
  float coef, S;
  int C, lane;
  __device__ UqTerm(const float* x0_, const float* t, float coef_, int C_, int lane_)
      : x0(x0_), pt(t, C_, lane_), coef(coef_), C(C_), lane(lane_) {
    float s = 0.f;
    for (int i = lane; i < C; i += RR_WAVE) s += x0[i];
    S = rr_wave_sum(s);
  }
  __device__ UqSums forward() const {
    float acc = 0.f, pen = 0.f;
    for (int i = lane; i < C; i += RR_WAVE) {
      const float p = x0[i] / S, tk = pt(i);
      pen += fabsf(logf(tk / p) * (x0[i] - 1.0f));
      if constexpr (!DIRICHLET) {
        acc += (tk > 0.f ? tk * logf(tk) : 0.f) - tk * logf(p);        // KLDivLoss: xlogy(t, t) - t * input
      } else {
        const float e = p - tk;
        acc += e * e + p * (1.0f - p) / (S + 1.0f);
      }
    }
    return UqSums{rr_wave_sum(acc), rr_wave_sum(pen)};
  }
  template <typename Emit>
  __device__ void gradient(float g, Emit emit) const {
    if constexpr (!DIRICHLET) {
      const float tsum = pt.total(C, lane);
      float U = 0.f;                                                // sum_i sgn(r_i) (s_i - 1)
      for (int i = lane; i < C; i += RR_WAVE) {
        const float p = x0[i] / S;
        U += sgnf(logf(pt(i) / p) * (x0[i] - 1.0f)) * (x0[i] - 1.0f);
      }
      U = rr_wave_sum(U);
      for (int k = lane; k < C; k += RR_WAVE) {
        const float sk = x0[k], p = sk / S, tk = pt(k), c = logf(tk / p), sg = sgnf(c * (sk - 1.0f));
        emit(k, g * ((tsum / S - tk / sk) + coef * (sg * c - sg * (sk - 1.0f) / sk + U / S)));
      }
    } else {
      float up = 0.f, w = 0.f;                                      // sum_i u_i p_i and d L / d S at fixed p
      const float S1 = S + 1.0f;
      auto u_of = [&](float ai, float p, float tk, float sg) {
        return 2.0f * (p - tk) + (1.0f - 2.0f * p) / S1 - coef * sg * (ai - 1.0f) / p;
      };
      for (int i = lane; i < C; i += RR_WAVE) {
        const float ai = x0[i], p = ai / S, tk = pt(i), sg = sgnf(logf(tk / p) * (ai - 1.0f));
        up += u_of(ai, p, tk, sg) * p;
        w -= p * (1.0f - p) / (S1 * S1);
      }
      up = rr_wave_sum(up);
      w = rr_wave_sum(w);
      for (int k = lane; k < C; k += RR_WAVE) {
        const float ak = x0[k], p = ak / S, tk = pt(k), c = logf(tk / p), sg = sgnf(c * (ak - 1.0f));
        const float u = u_of(ak, p, tk, sg);
        emit(k, g * ((u - up) / S + w + coef * sg * c));
      }
    }
  }
};

template <bool DIRICHLET>
struct UqLoss : PerQueryMean {
  static constexpr int kInputs = 1, kWords = 2;
  __device__ static UqTerm<DIRICHLET> term(const ListView& v, const ListNorm& n, int lane) {
    return UqTerm<DIRICHLET>(v.s, v.t, n.coef, n.C, lane);
  }
  __device__ static float partial(const UqSums& acc, const ListNorm& n) {
    const float invC = 1.0f / static_cast<float>(n.C);
    return acc.acc * invC + n.coef * (acc.pen * invC);
  }
};
template <> struct ListLoss<kListnetUq> : UqLoss<false> {};
template <> struct ListLoss<kDirichletUq> : UqLoss<true> {};

// ---------------------------------------------------------------- pointwise rows: MSE and Gaussian NLL (train/loss.py:144-162),
// Lognorm (train/loss.py:165-184) and the regression_exploss expression mean((exp(t) - exp(o))^2) (train/train_listwise.py:274-279)
// One row's value and its gradients for the caller's scale g (a forward-only caller passes anything and ignores them, a
// backward-only caller ignores the value: the compiler drops what is unused).
struct PointRow {
  float value, dmean, dvar;
};

enum PointKind : int { kPointMse, kPointGauss, kPointLognorm, kPointExpMse };
constexpr bool point_has_var(int K) { return K == kPointGauss || K == kPointLognorm; }

// x: the mean (MSE, Gauss), the score (Lognorm) or the prediction (exp-MSE); v is read by the kinds that have a variance
__device__ inline float half_log_2pi() { return 0.5f * logf(2.0f * 3.14159274101257324f); }   // float32(np.pi), loss.py:152,159,176,180

template <int K>
__device__ inline PointRow point_row(float x, float targ, float v, float g) {
  if constexpr (K == kPointGauss) {
    const float d = x - targ;
    return PointRow{half_log_2pi() + 0.5f * logf(v) + (d * d) / (2.0f * v), g * d / v, g * (0.5f / v - (d * d) / (2.0f * v * v))};
  } else if constexpr (K == kPointLognorm) {
    const float e = logf(x) - targ;
    return PointRow{half_log_2pi() + 0.5f * logf(v * (x * x)) + (e * e) / (2.0f * v), g * (1.0f / x + e / (v * x)),
                    g * (0.5f / v - (e * e) / (2.0f * v * v))};
  } else if constexpr (K == kPointExpMse) {
    const float es = expf(x), e = expf(targ) - es;
    return PointRow{e * e, g * (-2.0f * es * e), 0.f};
  } else {
    const float d = x - targ;
    return PointRow{d * d, g * 2.0f * d, 0.f};
  }
}

// ---------------------------------------------------------------- the last-arriver finish of the one-launch "step" kernels
// fixed-order sum of n floats on one wave: reduce_scale_kernel's order (256 strided accumulators, then block_sum's halving tree),
// lane l playing threads l, l + 64, l + 128, l + 192; the result is valid in lane 0.  step: the distance between two values.
__device__ inline float fixed_sum(const float* p, int n, int lane, int step = 1) {
  float a[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    float acc = 0.f;
    for (int i = lane + 64 * u; i < n; i += 256) acc += p[i * step];
    a[u] = acc;
  }
  float r = (a[0] + a[2]) + (a[1] + a[3]);                           // tree steps o = 128 and o = 64
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) r += __shfl_down(r, o, RR_WAVE);  // red[t] += red[t + o] for t < o
  return r;
}

// Every workgroup (one wave) of an n-workgroup launch calls this after it wrote its entries of partial[ROWS][n].  Each
// draws a ticket; the one that draws the last sums every row in fixed_sum's order - so a loss has the bits of the two-kernel
// path (partials, then reduce_scale_kernel) and the same bits on every run - and re-arms the counter, one device word the
// caller keeps.  The ticket is tested modulo n, so a word an earlier launch left at any multiple of n serves like a zero
// one.  True in lane 0 of the finishing wave alone, where sum[] is valid.
// arrive_last is the ticket alone: true in every lane of the wave that arrives last, which then owes the counter its zero.
__device__ inline bool arrive_last(int n, unsigned int* counter, int lane) {
  __threadfence();                                                   // release: this workgroup's partials
  unsigned int ticket = 0u;
  if (lane == 0) ticket = atomicAdd(counter, 1u);
  ticket = __shfl(ticket, 0, RR_WAVE);
  if (ticket % static_cast<unsigned int>(n) != static_cast<unsigned int>(n) - 1u) return false;
  __threadfence();                                                   // acquire: every other workgroup's partials
  return true;
}

template <int ROWS>
__device__ inline bool finish_last(const float* partial, int n, unsigned int* counter, int lane, float (&sum)[ROWS]) {
  if (!arrive_last(n, counter, lane)) return false;
#pragma unroll
  for (int r = 0; r < ROWS; ++r) sum[r] = fixed_sum(partial + r * n, n, lane);
  if (lane == 0) *counter = 0u;
  return lane == 0;
}

// The finish of the losses that carry a count (RankNet, LambdaRank: ordered pairs; ApproxNDCG: ranked queries).  Their
// per-query partials are [2 * n]: the query's loss as a float, its count as an int32.  loss = scale * the sum of the float
// halves in fixed_sum's order, count = the exact sum of the int32 halves; n == 0 gives +0.0f and 0.  One wave: the second
// launch of a forward entry point (finish_counted_kernel), or the wave that arrive_last picks in a step kernel.
__device__ inline void finish_counted(const float* partial, int n, float scale, float* loss, int64_t* count, int lane) {
  const float sum = fixed_sum(partial, n, lane, 2);
  long long np = 0;
  for (int i = lane; i < n; i += RR_WAVE) np += reinterpret_cast<const int32_t*>(partial)[2 * i + 1];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) np += __shfl_xor(np, o, RR_WAVE);
  if (lane == 0) {
    loss[0] = n > 0 ? sum * scale : 0.f;
    count[0] = np;
  }
}

__global__ void __launch_bounds__(RR_WAVE) finish_counted_kernel(const float* __restrict__ partial, int n, float scale,
                                                                 float* __restrict__ loss, int64_t* __restrict__ count) {
  finish_counted(partial, n, scale, loss, count, threadIdx.x);
}

}  // namespace
