// A composite task type's loss and d loss / d out in ONE launch (rr_task_loss_step_f32).
//
// The trainer's composite task types (train/train_listwise.py:196-285 of the reference) sum a per-list term and a
// per-candidate term over column slices of the head's [M, n_cols] output.  Every row of that output belongs to exactly one
// query, so the query's wavefront - which already holds the list in LDS for the list term - also evaluates the pointwise
// term of its own candidates and writes every column of its rows of d loss / d out, for an upstream gradient of one.  The
// two terms keep separate per-query partials (partial[0:Q] list, partial[Q:2Q] point) and separate normalisers (n_queries,
// n_cands: the counts of this process' step, or of the whole data-parallel step); the workgroup that draws the last ticket
// sums both rows in a fixed order, so the loss has the same bits on every run.
//
// The kernel is a shell over loss_list.h: it builds the SAME list term the standalone kernels of loss.hip build, and its
// rows go through the same point_row; what is its own are the normalisers, the exp() on column 1 for MLEDis, and the emit
// that adds the point term's gradient and writes whole rows.
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

template <int LT, int PT>
__global__ void __launch_bounds__(RR_WAVE) task_step_kernel(TaskArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int q = blockIdx.x, lane = threadIdx.x;
  const int L = a.L, Q = a.Q;
  const int off = a.seg_off[q], C = a.seg_off[q + 1] - off;
  float list_part = 0.f, point_acc = 0.f;

  if (C > 0) {
    float* x0 = sm;               // column 0
    float* t = sm + L;            // targets: no term overwrites them (the point term reads them as the rows are written)
    if constexpr (LT != RR_LIST_NONE) {
      for (int i = lane; i < C; i += RR_WAVE) {
        x0[i] = a.out[static_cast<int64_t>(off + i) * a.ld_out];
        t[i] = a.targets[off + i];
      }
      wave_sync();
    }
    // Writes row i of the query: column 0 gets the list term's gradient gl0 plus the point term's, column 1 gl1 plus the
    // point term's, every further column zero; adds the row's point term to point_acc.  Called once per row.
    auto finish_row = [&](int i, float gl0, float gl1 = 0.f) {
      const int64_t r = off + i;
      PointRow p{0.f, 0.f, 0.f};
      if constexpr (PT != RR_POINT_NONE) {
        const float mean = LT != RR_LIST_NONE ? x0[i] : a.out[r * a.ld_out];
        const float targ = LT != RR_LIST_NONE ? t[i] : a.targets[r];
        if constexpr (PT == RR_POINT_GAUSS) {
          p = point_row<kPointGauss>(mean, targ, a.out[r * a.ld_out + 1], a.inv_cands);   // the raw column 1 (GaussDisLoss takes its log)
        } else {
          p = point_row<kPointMse>(mean, targ, 0.f, a.inv_cands);
        }
        point_acc += p.value;
      }
      float* row = a.dout + r * a.ld_dout;
      row[0] = gl0 + p.dmean;
      if (a.n_cols > 1) row[1] = gl1 + p.dvar;
      for (int c = 2; c < a.n_cols; ++c) row[c] = 0.f;
    };
    const float invC = 1.0f / static_cast<float>(C);
    const float g = a.inv_queries * invC;                           // d / d (a per-query mean's element), mean over queries

    if constexpr (LT == RR_LIST_NONE) {
      for (int i = lane; i < C; i += RR_WAVE) finish_row(i, 0.f);
    } else if constexpr (LT == RR_LIST_MLE) {
      const ListMleTerm term(carve(sm, L), C, lane);
      list_part = term.forward() * invC;                            // torch.mean, loss.py:94
      term.gradient(g, finish_row);
    } else if constexpr (LT == RR_LIST_LISTNET) {
      const ListNetTerm term(x0, t, C, lane);
      list_part = term.forward();                                   // ONE mean over all candidates (loss.py:347)
      term.gradient(a.inv_cands, finish_row);
    } else if constexpr (LT == RR_LIST_MLEDIS) {
      // variance = exp(column 1), the transform the trainer applies (:196-202); d / d out[:, 1] carries exp'(out[:, 1]) =
      // the staged variance
      float* x1 = sm + 2 * L;
      for (int i = lane; i < C; i += RR_WAVE) x1[i] = expf(a.out[static_cast<int64_t>(off + i) * a.ld_out + 1]);
      const MleDisTerm<true> term(x0, x1, t, reinterpret_cast<int32_t*>(sm + 3 * L), sm + 4 * L, C, lane);
      list_part = term.forward() * invC;
      term.gradient(g, [&](int p, float g0, float g1) { finish_row(p, g0, g1 * x1[p]); });
    } else if constexpr (LT == RR_LIST_LISTNET_GAUSS) {
      float* x1 = sm + 2 * L;
      for (int i = lane; i < C; i += RR_WAVE) x1[i] = a.out[static_cast<int64_t>(off + i) * a.ld_out + 1];
      wave_sync();
      const ListNetGaussTerm term(x0, x1, t, C, lane);
      list_part = term.forward() * invC;
      term.gradient(g, finish_row);
    } else {
      const UqTerm<LT == RR_LIST_DIRICHLET_UQ> term(x0, t, a.coef, C, lane);
      const UqSums s = term.forward();
      list_part = s.acc * invC + a.coef * (s.pen * invC);
      term.gradient(g, finish_row);
    }
    if constexpr (PT != RR_POINT_NONE) point_acc = rr_wave_sum(point_acc);
  }
  if (lane == 0) {                                                  // an empty query adds zero to both terms
    a.partial[q] = list_part;
    a.partial[Q + q] = point_acc;
  }

  float sum[2];
  if (finish_last(a.partial, Q, a.counter, lane, sum)) {
    const float list_scale = LT == RR_LIST_LISTNET ? a.inv_cands : a.inv_queries;
    const float t0 = LT != RR_LIST_NONE ? sum[0] * list_scale : 0.f;
    const float t1 = PT != RR_POINT_NONE ? sum[1] * a.inv_cands : 0.f;
    a.loss[0] = t0 + t1;
    if (a.terms) {
      a.terms[0] = t0;
      a.terms[1] = t1;
    }
  }
}

// Q == 0: nothing to rank, the loss is the empty sum
__global__ void task_empty_kernel(float* loss, float* terms) {
  loss[0] = 0.f;
  if (terms) terms[0] = terms[1] = 0.f;
}

template <int LT, int PT>
int task_launch(const TaskArgs& a, hipStream_t s) {
  constexpr size_t bytes = (task_lds(LT) > 0 ? task_lds(LT) : 1) * sizeof(float);
  return launch_per_query(task_step_kernel<LT, PT>, a.Q, a.L, bytes, RR_WAVE, s, a);
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
  a.L = list_words(p->max_len);
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
