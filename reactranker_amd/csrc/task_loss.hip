// A composite task type's loss and d loss / d out in ONE launch (rr_task_loss_step_f32).
//
// The trainer's composite task types (train/train_listwise.py:196-285 of the reference) sum a per-list term and a
// per-candidate term over column slices of the head's [M, n_cols] output.  Every row of that output belongs to exactly one
// query, so the query's wavefront - which already holds the list in LDS for the list term (loss_list.h) - also evaluates
// the pointwise term of its own candidates and writes every column of its rows of d loss / d out, for an upstream gradient
// of one.  The two terms keep separate per-query partials (partial[0:Q] list, partial[Q:2Q] point) and separate
// normalisers (n_queries, n_cands: the counts of this process' step, or of the whole data-parallel step); the workgroup
// that draws the last ticket sums both rows in a fixed order, so the loss has the same bits on every run.
//
// List terms restate the per-list arithmetic of loss.hip (listmle_step_kernel, listnet_kernel, listwise_variant_kernel);
// the point terms restate pointwise_fwd_kernel / pointwise_bwd_kernel.
#include "loss_list.h"

namespace {

// staged floats per candidate
constexpr int task_lds(int LT) {
  return LT == RR_LIST_MLE || LT == RR_LIST_MLEDIS ? 5 : LT == RR_LIST_LISTNET_GAUSS ? 3 : LT == RR_LIST_NONE ? 0 : 2;
}
constexpr bool list_reads_col1(int LT) { return LT == RR_LIST_MLEDIS || LT == RR_LIST_LISTNET_GAUSS; }

struct TaskArgs {
  const float* out;
  int64_t ld_out;
  int n_cols;
  const float* targets;
  const int32_t* seg_off;
  int L, Q;
  float coef;
  float inv_queries, inv_cands;
  float* loss;
  float* terms;
  float* dout;
  int64_t ld_dout;
  float* partial;
  unsigned int* counter;
};

// fixed-order sum of n floats on one wave: reduce_scale_kernel's order (256 strided accumulators, then its halving tree),
// lane l playing threads l, l + 64, l + 128, l + 192; the result is valid in lane 0
__device__ inline float fixed_sum(const float* p, int n, int lane) {
  float a[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    float acc = 0.f;
    for (int i = lane + 64 * u; i < n; i += 256) acc += p[i];
    a[u] = acc;
  }
  float r = (a[0] + a[2]) + (a[1] + a[3]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) r += __shfl_down(r, o, RR_WAVE);
  return r;
}

template <int LT, int PT>
__global__ void __launch_bounds__(RR_WAVE) task_step_kernel(TaskArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int q = blockIdx.x, lane = threadIdx.x;
  const int L = a.L, Q = a.Q;
  const int off = a.seg_off[q], C = a.seg_off[q + 1] - off;
  float list_part = 0.f, point_acc = 0.f;

  if (C > 0) {
    float* x0 = sm;               // column 0
    float* t = sm + L;            // targets: kept intact until the rows are written (the point term reads them)
    if constexpr (LT != RR_LIST_NONE) {
      for (int i = lane; i < C; i += RR_WAVE) {
        x0[i] = a.out[static_cast<int64_t>(off + i) * a.ld_out];
        t[i] = a.targets[off + i];
      }
      wave_sync();
    }
    const float half_log_2pi = 0.5f * logf(2.0f * 3.14159274101257324f);   // float32(np.pi), loss.py:152,159
    // Writes row i of the query: column 0 gets the list term's gradient gl0 plus the point term's, column 1 gl1 plus the
    // point term's, every further column zero; adds the row's point term to point_acc.  Called once per row.
    auto finish_row = [&](int i, float gl0, float gl1) {
      const int64_t r = off + i;
      float gp0 = 0.f, gp1 = 0.f;
      if constexpr (PT != RR_POINT_NONE) {
        const float mean = LT != RR_LIST_NONE ? x0[i] : a.out[r * a.ld_out];
        const float targ = LT != RR_LIST_NONE ? t[i] : a.targets[r];
        const float d = mean - targ;
        if constexpr (PT == RR_POINT_GAUSS) {
          const float v = a.out[r * a.ld_out + 1];                  // the raw column 1 (GaussDisLoss takes its log)
          point_acc += half_log_2pi + 0.5f * logf(v) + (d * d) / (2.0f * v);
          gp0 = a.inv_cands * d / v;
          gp1 = a.inv_cands * (0.5f / v - (d * d) / (2.0f * v * v));
        } else {
          point_acc += d * d;
          gp0 = a.inv_cands * 2.0f * d;
        }
      }
      float* row = a.dout + r * a.ld_dout;
      row[0] = gl0 + gp0;
      if (a.n_cols > 1) row[1] = gl1 + gp1;
      for (int c = 2; c < a.n_cols; ++c) row[c] = 0.f;
    };
    const float invC = 1.0f / static_cast<float>(C);
    const float g = a.inv_queries * invC;                           // d / d (a per-query mean's element), mean over queries

    if constexpr (LT == RR_LIST_NONE) {
      for (int i = lane; i < C; i += RR_WAVE) finish_row(i, 0.f, 0.f);
    } else if constexpr (LT == RR_LIST_MLE) {
      ListView v = carve(sm, L);
      rank_sort(v, C, lane);
      const float m = list_max(v.ss, C, lane);
      logcumsumexp_rev(v.ss, v.aux, C, lane, m);
      float acc = 0.f;
      for (int i = lane; i < C; i += RR_WAVE) acc += v.aux[i] - v.ss[i];
      list_part = rr_wave_sum(acc) * invC;                          // torch.mean, loss.py:94
      cumsum_exp_neg(v.aux, v.aux, C, lane);                        // in place (each lane reads fd[j] before it writes [j])
      for (int j = lane; j < C; j += RR_WAVE) finish_row(v.perm[j], g * (expf(v.ss[j]) * v.aux[j]) - g, 0.f);
    } else if constexpr (LT == RR_LIST_MLEDIS) {
      // listwise_variant_kernel<kMleDis> with variance = exp(column 1), the transform the trainer applies (:196-202)
      float* x1 = sm + 2 * L;
      int32_t* perm = reinterpret_cast<int32_t*>(sm + 3 * L);
      float* F = sm + 4 * L;
      for (int i = lane; i < C; i += RR_WAVE) x1[i] = expf(a.out[static_cast<int64_t>(off + i) * a.ld_out + 1]);
      ListView lv;
      lv.s = x0;
      lv.t = t;
      lv.perm = perm;
      lv.ss = F;                                                    // sorted scores: scratch, overwritten below
      lv.aux = nullptr;
      rank_sort(lv, C, lane);
      for (int r = lane; r < C; r += RR_WAVE) {
        const int p = perm[r];
        F[r] = x0[p] + 0.5f * x1[p];                                // sorted a_j = s_j + v_j / 2
      }
      wave_sync();
      const float m = list_max(F, C, lane);
      logcumsumexp_rev(F, F, C, lane, m);                           // in place: F_j = log sum_{i>=j} exp(a_i)
      float acc = 0.f;
      for (int r = lane; r < C; r += RR_WAVE) {
        const int p = perm[r];
        acc += F[r] + (0.5f * x1[p] - x0[p]);
      }
      list_part = rr_wave_sum(acc) * invC;
      for (int k = lane; k < C; k += RR_WAVE) {
        const int p = perm[k];
        const float ak = x0[p] + 0.5f * x1[p];
        float G = 0.f;
        for (int j = 0; j <= k; ++j) G += expf(ak - F[j]);
        // d / d out[:, 1] carries exp'(out[:, 1]) = the staged variance
        finish_row(p, g * (G - 1.0f), (g * 0.5f * (G + 1.0f)) * x1[p]);
      }
    } else {
      float mt, zt;                                                 // softmax of the query's targets
      softmax_stats(t, C, lane, &mt, &zt);
      auto smt = [&](int i) { return expf(t[i] - mt) / zt; };
      float tsum = 0.f;
      for (int i = lane; i < C; i += RR_WAVE) tsum += smt(i);
      tsum = rr_wave_sum(tsum);
      if constexpr (LT == RR_LIST_LISTNET) {
        float ms, zs;
        softmax_stats(x0, C, lane, &ms, &zs);
        float acc = 0.f;
        for (int i = lane; i < C; i += RR_WAVE) acc += -smt(i) * logf(expf(x0[i] - ms) / zs);   // loss.py:339-343
        list_part = rr_wave_sum(acc);                               // ONE mean over all candidates (loss.py:347)
        for (int i = lane; i < C; i += RR_WAVE) finish_row(i, a.inv_cands * ((expf(x0[i] - ms) / zs) * tsum - smt(i)), 0.f);
      } else if constexpr (LT == RR_LIST_LISTNET_GAUSS) {
        float* x1 = sm + 2 * L;
        for (int i = lane; i < C; i += RR_WAVE) x1[i] = a.out[static_cast<int64_t>(off + i) * a.ld_out + 1];
        wave_sync();
        float ma = -INFINITY;
        for (int i = lane; i < C; i += RR_WAVE) ma = fmaxf(ma, x0[i] + 0.5f * x1[i]);
        ma = rr_wave_max(ma);
        float za = 0.f;
        for (int i = lane; i < C; i += RR_WAVE) za += expf(x0[i] + 0.5f * x1[i] - ma);
        za = rr_wave_sum(za);
        const float lse = ma + logf(za);
        float acc = 0.f;
        for (int i = lane; i < C; i += RR_WAVE) acc += smt(i) * (lse + (0.5f * x1[i] - x0[i]));
        list_part = rr_wave_sum(acc) * invC;
        for (int k = lane; k < C; k += RR_WAVE) {
          const float pk = expf(x0[k] + 0.5f * x1[k] - lse), tk = smt(k);
          finish_row(k, g * (tsum * pk - tk), g * 0.5f * (tsum * pk + tk));
        }
      } else {
        // RR_LIST_LISTNET_UQ / RR_LIST_DIRICHLET_UQ: see listwise_variant_kernel
        const float coef = a.coef;
        float S = 0.f;
        for (int i = lane; i < C; i += RR_WAVE) S += x0[i];
        S = rr_wave_sum(S);
        float acc = 0.f, pen = 0.f;
        for (int i = lane; i < C; i += RR_WAVE) {
          const float p = x0[i] / S, tk = smt(i);
          pen += fabsf(logf(tk / p) * (x0[i] - 1.0f));
          if constexpr (LT == RR_LIST_LISTNET_UQ) {
            acc += (tk > 0.f ? tk * logf(tk) : 0.f) - tk * logf(p);          // KLDivLoss: xlogy(t, t) - t * input
          } else {
            const float e = p - tk;
            acc += e * e + p * (1.0f - p) / (S + 1.0f);
          }
        }
        acc = rr_wave_sum(acc);
        pen = rr_wave_sum(pen);
        list_part = acc * invC + coef * (pen * invC);
        if constexpr (LT == RR_LIST_LISTNET_UQ) {
          float U = 0.f;                                            // sum_i sgn(r_i) (s_i - 1)
          for (int i = lane; i < C; i += RR_WAVE) {
            const float p = x0[i] / S;
            U += sgnf(logf(smt(i) / p) * (x0[i] - 1.0f)) * (x0[i] - 1.0f);
          }
          U = rr_wave_sum(U);
          for (int k = lane; k < C; k += RR_WAVE) {
            const float sk = x0[k], p = sk / S, tk = smt(k), c = logf(tk / p), sg = sgnf(c * (sk - 1.0f));
            finish_row(k, g * ((tsum / S - tk / sk) + coef * (sg * c - sg * (sk - 1.0f) / sk + U / S)), 0.f);
          }
        } else {
          float up = 0.f, w = 0.f;                                  // sum_i u_i p_i and d L / d S at fixed p
          const float S1 = S + 1.0f;
          for (int i = lane; i < C; i += RR_WAVE) {
            const float ai = x0[i], p = ai / S, tk = smt(i), sg = sgnf(logf(tk / p) * (ai - 1.0f));
            const float u = 2.0f * (p - tk) + (1.0f - 2.0f * p) / S1 - coef * sg * (ai - 1.0f) / p;
            up += u * p;
            w -= p * (1.0f - p) / (S1 * S1);
          }
          up = rr_wave_sum(up);
          w = rr_wave_sum(w);
          for (int k = lane; k < C; k += RR_WAVE) {
            const float ak = x0[k], p = ak / S, tk = smt(k), c = logf(tk / p), sg = sgnf(c * (ak - 1.0f));
            const float u = 2.0f * (p - tk) + (1.0f - 2.0f * p) / S1 - coef * sg * (ak - 1.0f) / p;
            finish_row(k, g * ((u - up) / S + w + coef * sg * c), 0.f);
          }
        }
      }
    }
    if constexpr (PT != RR_POINT_NONE) point_acc = rr_wave_sum(point_acc);
  }
  if (lane == 0) {                                                  // an empty query adds zero to both terms
    a.partial[q] = list_part;
    a.partial[Q + q] = point_acc;
  }

  // the last-arriving workgroup sums both rows of `partial` (finish_last of loss.hip: release fence, ticket, acquire fence,
  // one wave, fixed tree).  The ticket is tested modulo Q, so a word that an earlier launch left at a multiple of Q still
  // lets this launch finish; the finisher re-arms it with zero.
  __threadfence();                                                  // release: this workgroup's partials
  unsigned int ticket = 0u;
  if (lane == 0) ticket = atomicAdd(a.counter, 1u);
  ticket = __shfl(ticket, 0, RR_WAVE);
  if (ticket % static_cast<unsigned int>(Q) != static_cast<unsigned int>(Q) - 1u) return;
  __threadfence();                                                  // acquire: every other workgroup's partials
  const float s_list = fixed_sum(a.partial, Q, lane);
  const float s_point = fixed_sum(a.partial + Q, Q, lane);
  if (lane == 0) {
    const float list_scale = LT == RR_LIST_LISTNET ? a.inv_cands : a.inv_queries;
    const float t0 = LT != RR_LIST_NONE ? s_list * list_scale : 0.f;
    const float t1 = PT != RR_POINT_NONE ? s_point * a.inv_cands : 0.f;
    a.loss[0] = t0 + t1;
    if (a.terms) {
      a.terms[0] = t0;
      a.terms[1] = t1;
    }
    *a.counter = 0u;
  }
}

// Q == 0: nothing to rank, the loss is the empty sum
__global__ void task_empty_kernel(float* loss, float* terms) {
  loss[0] = 0.f;
  if (terms) terms[0] = terms[1] = 0.f;
}

template <int LT, int PT>
int task_launch(const TaskArgs& a, hipStream_t s) {
  const size_t lds = static_cast<size_t>(task_lds(LT) > 0 ? task_lds(LT) : 1) * a.L * sizeof(float);
  if (set_lds(task_step_kernel<LT, PT>, lds) != RR_OK) return RR_ERR_LAUNCH;
  task_step_kernel<LT, PT><<<a.Q, RR_WAVE, lds, s>>>(a);
  return rr_launch_status();
}

template <int LT>
int task_launch_point(int pt, const TaskArgs& a, hipStream_t s) {
  switch (pt) {
    case RR_POINT_NONE:
      if constexpr (LT == RR_LIST_NONE) return RR_ERR_ARG; else return task_launch<LT, RR_POINT_NONE>(a, s);
    case RR_POINT_MSE: return task_launch<LT, RR_POINT_MSE>(a, s);
    case RR_POINT_GAUSS: return task_launch<LT, RR_POINT_GAUSS>(a, s);
  }
  return RR_ERR_ARG;
}

}  // namespace

extern "C" {

size_t rr_abi_task_loss_size(void) { return sizeof(rr_task_loss_args); }

int rr_task_loss_step_f32(const rr_task_loss_args* p, rr_stream_t stream) {
  RR_CHECK_ARG(p != nullptr);
  RR_CHECK_ARG(p->list_term >= RR_LIST_NONE && p->list_term <= RR_LIST_DIRICHLET_UQ);
  RR_CHECK_ARG(p->point_term >= RR_POINT_NONE && p->point_term <= RR_POINT_GAUSS);
  RR_CHECK_ARG(p->list_term != RR_LIST_NONE || p->point_term != RR_POINT_NONE);
  RR_CHECK_ARG(list_args_ok(p->out, p->targets, p->seg_off, p->Q, p->max_len) && p->loss && p->dout && p->partial && p->counter);
  const int need = (list_reads_col1(p->list_term) || p->point_term == RR_POINT_GAUSS) ? 2 : 1;
  RR_CHECK_ARG(p->n_cols >= need && p->ld_out >= p->n_cols && p->ld_dout >= p->n_cols);
  RR_CHECK_ARG(p->n_queries >= 0 && p->n_cands >= 0);
  if (p->max_len > kMaxLen) return RR_ERR_UNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (p->Q == 0) {
    task_empty_kernel<<<1, 1, 0, s>>>(p->loss, p->terms);
    return rr_launch_status();
  }
  TaskArgs a;
  a.out = p->out;
  a.ld_out = p->ld_out;
  a.n_cols = p->n_cols;
  a.targets = p->targets;
  a.seg_off = p->seg_off;
  a.L = p->max_len > 0 ? p->max_len : 1;
  a.Q = p->Q;
  a.coef = p->coef;
  a.inv_queries = p->n_queries > 0 ? 1.0f / static_cast<float>(p->n_queries) : 0.f;
  a.inv_cands = p->n_cands > 0 ? 1.0f / static_cast<float>(p->n_cands) : 0.f;
  a.loss = p->loss;
  a.terms = p->terms;
  a.dout = p->dout;
  a.ld_dout = p->ld_dout;
  a.partial = p->partial;
  a.counter = p->counter;
  switch (p->list_term) {
    case RR_LIST_NONE: return task_launch_point<RR_LIST_NONE>(p->point_term, a, s);
    case RR_LIST_MLE: return task_launch_point<RR_LIST_MLE>(p->point_term, a, s);
    case RR_LIST_LISTNET: return task_launch_point<RR_LIST_LISTNET>(p->point_term, a, s);
    case RR_LIST_MLEDIS: return task_launch_point<RR_LIST_MLEDIS>(p->point_term, a, s);
    case RR_LIST_LISTNET_GAUSS: return task_launch_point<RR_LIST_LISTNET_GAUSS>(p->point_term, a, s);
    case RR_LIST_LISTNET_UQ: return task_launch_point<RR_LIST_LISTNET_UQ>(p->point_term, a, s);
    case RR_LIST_DIRICHLET_UQ: return task_launch_point<RR_LIST_DIRICHLET_UQ>(p->point_term, a, s);
  }
  return RR_ERR_ARG;
}

}  // extern "C"
