// Sphere-exclusion (Taylor-Butina / leader) clustering over reaction embeddings.  A definition of this
// library, not a port; include/reactranker_hip.h states it.
//
//   round t: the centre c is the row with labels == -1 that is largest under the total order (key descending, index ascending);
//            every row i with labels[i] == -1 and d(i, c) <= r2 gets labels[i] = t.  d is rr_kcenter_f32's difference chain
//            (row_chain.h), so d(c, c) = 0 and the centre joins its own cluster.
//
// se_pass_kernel<NG, VEC> is the only kernel of a clustering; its launches run back to back on the caller's stream, as
// csrc/kcenter.hip's do:
//   the initial launch (first_round == 0 only) writes labels (-2 for a row that holds a non-finite value, else -1: the one extra
//                  read of the pool) and scores round 0;
//   the launch of round t reduces the grid's (key, index) pairs of the launch before it to the winner c (EVERY workgroup does,
//                  redundantly: the order is total, so all agree; workgroup 0 writes the centre), keeps c's columns in
//                  registers, and streams the rows still at -1: distance to c, the label, and - for a row that stays at -1 -
//                  the workgroup's candidate for round t + 1.
// A workgroup leaves one pair per launch in the workspace (two arrays, used alternately; slot 0 of an array holds how many
// pairs follow, so a call that continues another one need not run the same grid), so a launch only ever reads what the launch
// before it wrote: the kernel boundary is the only synchronisation, nothing inside a launch waits for or signals another
// workgroup, and there are no atomics.
// One wave per row, rows grid-strided as in kcenter.hip.  A wave first reads the labels of its next 64 rows (one per lane),
// then visits only those still at -1, two rows in flight: a row that is assigned already costs four bytes, not its columns.
#include "row_chain.h"

namespace {

BlocksKnob g_blocks;

typedef RowPair<int32_t> SePair;                  // (key, index); slot 0 of an array: k = pairs that follow

struct SeParams {
  const float* x; int64_t ld; int64_t P; int H;
  float r2;
  const int32_t* key;                             // [P] or null (every key equal)
  int32_t* labels;
  int32_t* centre;                                // where this launch's centre goes (null: the initial launch)
  const SePair* prev; SePair* out;                // [1 + pairs] each (workspace)
  int t;                                          // the round this launch assigns; the initial launch assigns none
};

template <int NG, bool VEC>
__global__ void __launch_bounds__(RC_NT) se_pass_kernel(const SeParams p) {
  __shared__ SePair s_prev[RC_WAVES], s_out[RC_WAVES];
  constexpr int NR = NG > 0 ? NG : 1;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = p.H;
  const bool init = p.centre == nullptr;
  const bool keyed = p.key != nullptr;

  int c = -1;                                     // the centre of round t
  f32x4 cv[NR];
  const float* crow = p.x;
  if (!init) {
    // The scan stays here, as in kc_pass_kernel: inside one helper with the join it moves the registers of the NG == 0 kernels
    // (profiles/embedding_shared_ab.txt).
    int bk = 0, bi = -1;
    // (a workspace that no launch of this entry wrote - a call with first_round > 0 on fresh memory - must not become an
    // address: the count is held to the array and an index past the pool counts as none)
    const int n_prev = min(max(p.prev[0].k, 0), RC_MAX_BLOCKS);
    for (int k = tid; k < n_prev; k += RC_NT) {
      const SePair q = p.prev[1 + k];
      if (q.i < p.P && rr_first_max_replaces(q.k, q.i, bk, bi)) { bk = q.k; bi = q.i; }
    }
    rr_wave_first_max(bk, bi);
    rc_join_waves(bk, bi, wave, s_prev);
    c = __builtin_amdgcn_readfirstlane(bi);
    if (blockIdx.x == 0 && tid == 0) *p.centre = c;
    if (c < 0) {                                  // no row is at -1, so none will be: nothing changes, no candidate
      if (tid == 0) {
        p.out[1 + blockIdx.x].k = 0; p.out[1 + blockIdx.x].i = -1;
        if (blockIdx.x == 0) { p.out[0].k = static_cast<int32_t>(gridDim.x); p.out[0].i = 0; }
      }
      return;
    }
    crow = p.x + static_cast<int64_t>(c) * p.ld;
    if (NG > 0) kc_load_row<NR, VEC>(crow, lane, H, cv);
  }

  int best_k = 0, best_i = -1;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * RC_WAVES;
  const int64_t first = static_cast<int64_t>(blockIdx.x) * RC_WAVES + wave;

  // one row that is at -1 (or, in the initial launch, any row): `a` holds its columns (NG > 0); uniform per wave
  auto row_pass = [&](int64_t r, const f32x4 (&a)[NR], int k) {
    const float* row = p.x + r * p.ld;
    bool stays;
    if (init) {
      stays = NG > 0 ? kc_row_finite<NR>(a, lane, H) : kc_row_finite_any<VEC>(row, lane, H);
      if (lane == 0) p.labels[r] = stays ? -1 : -2;
    } else {
      const float d = NG > 0 ? kc_dist<NR>(a, cv, lane, H) : kc_dist_any<VEC>(row, crow, lane, H);
      stays = !(d <= p.r2);
      if (!stays && lane == 0) p.labels[r] = p.t;
    }
    if (stays && rr_first_max_replaces(k, static_cast<int>(r), best_k, best_i)) { best_k = k; best_i = static_cast<int>(r); }
  };

  for (int64_t base = first; base < p.P; base += 64 * stride) {   // (uniform per wave)
    const int64_t mine = base + lane * stride;
    const bool live = mine < p.P && (init || p.labels[mine] == -1);
    const int kv = (live && keyed) ? p.key[mine] : 0;
    uint64_t mask = __ballot(live);
    while (mask != 0) {                           // (uniform)
      const int j0 = __builtin_amdgcn_readfirstlane(__builtin_ctzll(mask));
      mask &= mask - 1;
      const bool two = mask != 0;
      const int j1 = two ? __builtin_amdgcn_readfirstlane(__builtin_ctzll(mask)) : j0;
      mask &= mask - 1;                           // (0 & anything is 0)
      const int64_t r0 = base + j0 * stride, r1 = base + j1 * stride;
      f32x4 a0[NR], a1[NR];
      if (NG > 0) {
        kc_load_row<NR, VEC>(p.x + r0 * p.ld, lane, H, a0);
        kc_load_row<NR, VEC>(p.x + r1 * p.ld, lane, H, a1);
      }
      row_pass(r0, a0, __builtin_amdgcn_readlane(kv, j0));
      if (two) row_pass(r1, a1, __builtin_amdgcn_readlane(kv, j1));
    }
  }

  rc_block_best(best_k, best_i, wave, s_out, [&](int bk, int bi) {
    p.out[1 + blockIdx.x].k = bk;
    p.out[1 + blockIdx.x].i = bi;
    if (blockIdx.x == 0) { p.out[0].k = static_cast<int32_t>(gridDim.x); p.out[0].i = 0; }
  });
}

// the workspace: two pair arrays sized for the largest grid (so the size does not depend on the blocks setting), each behind
// its count slot
constexpr size_t SE_PAIRS_BYTES = static_cast<size_t>(RC_MAX_BLOCKS + 1) * sizeof(SePair);
constexpr size_t SE_WORKSPACE = 2 * SE_PAIRS_BYTES;

}  // namespace

extern "C" {

int rr_sphere_exclusion_blocks(void) { return g_blocks.get(); }
int rr_sphere_exclusion_set_blocks(int blocks) { return g_blocks.set(blocks, RC_MAX_BLOCKS); }

int rr_sphere_exclusion_workspace_bytes(int64_t P, size_t* bytes) {
  RR_CHECK_ARG(bytes && P >= 0);
  if (P > 0x7fffffffLL) return RR_ERR_UNSUPPORTED;
  *bytes = SE_WORKSPACE;
  return RR_OK;
}

int rr_sphere_exclusion_f32(const float* x, int64_t ld, int64_t P, int H, float r2, const int32_t* key, int first_round,
                            int n_rounds, int32_t* labels, int32_t* centres, void* workspace, size_t workspace_bytes,
                            rr_stream_t stream) {
  RR_CHECK_ARG(x && labels && centres && workspace);
  RR_CHECK_ARG(P >= 0 && first_round >= 0 && n_rounds >= 0 && H >= 1 && ld >= H);
  RR_CHECK_ARG(r2 >= 0.f);                        // (false for a NaN)
  if (n_rounds > RR_SPHERE_EXCLUSION_MAX_ROUNDS || P > 0x7fffffffLL || first_round > 0x7fffffff - n_rounds) return RR_ERR_UNSUPPORTED;
  if (workspace_bytes < SE_WORKSPACE) return RR_ERR_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (P == 0) {
    if (n_rounds == 0) return RR_OK;
    rc_pad_kernel<false><<<rr_grid_for(n_rounds, RC_NT, 64), RC_NT, 0, s>>>(centres, nullptr, n_rounds);
    return rr_launch_status();
  }
  char* ws = static_cast<char*>(workspace);
  SePair* pairs[2] = {reinterpret_cast<SePair*>(ws), reinterpret_cast<SePair*>(ws + SE_PAIRS_BYTES)};
  SeParams p;
  p.x = x; p.ld = ld; p.P = P; p.H = H; p.r2 = r2; p.key = key; p.labels = labels;
  const int grid = rc_grid(g_blocks.get(), P);
  // launch j = -1 is the initial one; the launch of round t reads pairs[t & 1] and writes pairs[(t + 1) & 1]
  for (int j = first_round == 0 ? -1 : 0; j < n_rounds; ++j) {
    const int t = first_round + (j < 0 ? 0 : j);
    p.t = t;
    p.centre = j < 0 ? nullptr : centres + j;
    p.prev = pairs[t & 1];
    p.out = j < 0 ? pairs[0] : pairs[(t + 1) & 1];
    rc_dispatch(H, x, ld, [&](auto ng, auto vec) {
      se_pass_kernel<decltype(ng)::value, decltype(vec)::value><<<grid, RC_NT, 0, s>>>(p);
    });
    const int st = rr_launch_status();
    if (st != RR_OK) return st;
  }
  return RR_OK;
}

}  // extern "C"
