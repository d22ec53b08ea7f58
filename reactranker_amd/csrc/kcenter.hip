// Greedy k-center selection over reaction embeddings.  A definition of this library, not a port;
// include/reactranker_hip.h states it.
//
//   d(i, c) = sum_h (x[i,h] - x[c,h])^2 in f32 by the fixed chain: columns in groups of four, lane l of the wave owns the groups
//   g with g % 64 == l (ascending, columns inside a group ascending), acc = acc + t * t with t = x[i,h] - x[c,h], the 64 chains
//   joined by the butterfly xor 32, 16, 8, 4, 2, 1.  The chain, the row loads and the round scaffold (the join of the four
//   waves, the workgroup's best pair, the grid rule, the NG / VEC dispatch) live in row_chain.h (csrc/cluster.hip shares them).
//
// kc_pass_kernel<NG, VEC> is the only kernel of a selection; n_pick + 1 launches of it run back to back on the caller's stream:
//   launch 0       writes min_dist / assign / the eligibility bytes (the one extra read of the pool: it finds the rows that hold
//                  a non-finite value) and scores round 0;
//   launch t >= 1  reduces the grid's pairs of launch t - 1 to the winner c of round t - 1 (EVERY workgroup does, redundantly:
//                  the order is total, so all agree; workgroup 0 writes picks[t-1] / gain[t-1]), keeps c's columns in registers,
//                  and streams the pool once: distance to c, min / assign update, the new score, the workgroup's argmax.
// A workgroup leaves one (score, index) pair per launch in the workspace (two arrays, used alternately), so a launch only ever
// reads what the launch before it wrote: the kernel boundary is the only synchronisation, nothing inside a launch waits for or
// signals another workgroup, and there are no atomics.  One wave per row, rows grid-strided, two rows in flight per wave.
// NG = groups a lane owns (1 .. 4: H <= 1024, the centre in 4 NG registers); NG == 0 is the loop for wider rows, which re-reads
// the centre's columns (L1 / L2 hits).  VEC: 16-byte loads (pointer 16-byte aligned and ld % 4 == 0), else 4-byte loads.
#include "row_chain.h"

namespace {

BlocksKnob g_blocks;

typedef RowPair<float> KcPair;                    // (score, index)

struct KcParams {
  const float* x; int64_t ld; int64_t P; int H;
  const float* init_dist; const float* weight;
  int32_t* picks; float* gain; float* min_dist; int32_t* assign;
  uint8_t* elig;                                  // [P] 1: may still be picked (workspace)
  const KcPair* prev; KcPair* out;                // [gridDim.x] each (workspace)
  int t;                                          // the round this launch scores; 0: the initial pass
  int last;                                       // launch n_pick: nothing is scored
};

template <int NG, bool VEC>
__global__ void __launch_bounds__(RC_NT) kc_pass_kernel(const KcParams p) {
  __shared__ KcPair s_prev[RC_WAVES], s_out[RC_WAVES];
  constexpr int NR = NG > 0 ? NG : 1;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = p.H, t = p.t;
  const bool weighted = p.weight != nullptr;

  int c = -1;                                     // the centre: the winner of round t - 1
  f32x4 cv[NR];
  const float* crow = p.x;
  if (t > 0) {
    // The scan over the grid's pairs stays here (and in se_pass_kernel, which adds its count slot and index guard): as one
    // helper with the join it cost the NG == 3 kernels, at the SGPR cap, up to 38 instructions and measured 0.4 - 1.5 % on
    // weighted picks at H = 600 (profiles/embedding_shared_ab.txt).
    float bs = 0.f;
    int bi = -1;
    for (int k = tid; k < static_cast<int>(gridDim.x); k += RC_NT) {
      const KcPair q = p.prev[k];
      if (rr_first_max_replaces(q.k, q.i, bs, bi)) { bs = q.k; bi = q.i; }
    }
    rr_wave_first_max(bs, bi);
    rc_join_waves(bs, bi, wave, s_prev);
    c = __builtin_amdgcn_readfirstlane(bi);
    if (blockIdx.x == 0 && tid == 0) {
      p.picks[t - 1] = c;
      p.gain[t - 1] = c >= 0 ? bs : -1.0f;
    }
    if (c < 0) {                                  // nothing was eligible, so nothing will be: no update, no candidate
      if (tid == 0 && !p.last) { p.out[blockIdx.x].k = 0.f; p.out[blockIdx.x].i = -1; }
      return;
    }
    crow = p.x + static_cast<int64_t>(c) * p.ld;
    if (NG > 0) kc_load_row<NR, VEC>(crow, lane, H, cv);
  }

  float best_s = 0.f;
  int best_i = -1;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * RC_WAVES;
  const int64_t first = static_cast<int64_t>(blockIdx.x) * RC_WAVES + wave;

  // one row: `a` holds its columns (NG > 0); every lane leaves with the same values
  auto row_pass = [&](int64_t r, const f32x4 (&a)[NR], float md_in, float w, int e_in) {
    const float* row = p.x + r * p.ld;
    float md;
    int e;
    if (t == 0) {
      const bool fin = NG > 0 ? kc_row_finite<NR>(a, lane, H) : kc_row_finite_any<VEC>(row, lane, H);
      md = fin ? md_in : __builtin_nanf("");
      e = (md == md) && (!weighted || (w > 0.f && w < __builtin_inff()));
      if (lane == 0) {
        p.min_dist[r] = md;
        p.assign[r] = -1;
        p.elig[r] = static_cast<uint8_t>(e);
      }
    } else {
      const float d = NG > 0 ? kc_dist<NR>(a, cv, lane, H) : kc_dist_any<VEC>(row, crow, lane, H);
      md = md_in;
      e = e_in;
      if (d < md) {                               // (false for a NaN on either side)
        md = d;
        if (lane == 0) {
          p.min_dist[r] = d;
          p.assign[r] = t - 1;
        }
      }
      if (r == c) {
        e = 0;
        if (lane == 0) p.elig[r] = 0;
      }
    }
    if (e && !p.last) {
      const float s = weighted ? w * md : md;
      if (rr_first_max_replaces(s, static_cast<int>(r), best_s, best_i)) { best_s = s; best_i = static_cast<int>(r); }
    }
  };

  for (int64_t r0 = first; r0 < p.P; r0 += 2 * stride) {   // (uniform per wave)
    const int64_t r1 = r0 + stride;
    const bool two = r1 < p.P;
    const int64_t q1 = two ? r1 : r0;
    f32x4 a0[NR], a1[NR];
    if (NG > 0) {
      kc_load_row<NR, VEC>(p.x + r0 * p.ld, lane, H, a0);
      kc_load_row<NR, VEC>(p.x + q1 * p.ld, lane, H, a1);
    }
    float m0, m1;
    int e0 = 1, e1 = 1;
    if (t == 0) {
      m0 = p.init_dist ? p.init_dist[r0] : __builtin_inff();
      m1 = p.init_dist ? p.init_dist[q1] : __builtin_inff();
    } else {
      m0 = p.min_dist[r0];
      m1 = p.min_dist[q1];
      e0 = p.elig[r0];
      e1 = p.elig[q1];
    }
    const float w0 = weighted ? p.weight[r0] : 1.f, w1 = weighted ? p.weight[q1] : 1.f;
    row_pass(r0, a0, m0, w0, e0);
    if (two) row_pass(r1, a1, m1, w1, e1);
  }

  if (p.last) return;
  rc_block_best(best_s, best_i, wave, s_out, [&](float bs, int bi) {
    p.out[blockIdx.x].k = bs;
    p.out[blockIdx.x].i = bi;
  });
}

// the workspace: two pair arrays sized for the largest grid (so the size does not depend on the blocks setting), then elig [P]
constexpr size_t KC_PAIRS_BYTES = static_cast<size_t>(RC_MAX_BLOCKS) * sizeof(KcPair);
inline size_t kc_workspace(int64_t P) { return 2 * KC_PAIRS_BYTES + rr_round256(static_cast<size_t>(P)); }

}  // namespace

extern "C" {

int rr_kcenter_blocks(void) { return g_blocks.get(); }
int rr_kcenter_set_blocks(int blocks) { return g_blocks.set(blocks, RC_MAX_BLOCKS); }

int rr_kcenter_workspace_bytes(int64_t P, int n_pick, size_t* bytes) {
  RR_CHECK_ARG(bytes && P >= 0 && n_pick >= 0);
  if (n_pick > RR_KCENTER_MAX_PICKS || P > 0x7fffffffLL) return RR_ERR_UNSUPPORTED;
  *bytes = kc_workspace(P);
  return RR_OK;
}

int rr_kcenter_f32(const float* x, int64_t ld, int64_t P, int H, int n_pick, const float* init_dist, const float* weight,
                   int32_t* picks, float* gain, float* min_dist, int32_t* assign, void* workspace, size_t workspace_bytes,
                   rr_stream_t stream) {
  RR_CHECK_ARG(x && picks && gain && min_dist && assign && workspace);
  RR_CHECK_ARG(P >= 0 && n_pick >= 0 && H >= 1 && ld >= H);
  if (n_pick > RR_KCENTER_MAX_PICKS || P > 0x7fffffffLL) return RR_ERR_UNSUPPORTED;
  if (workspace_bytes < kc_workspace(P)) return RR_ERR_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (P == 0) {
    if (n_pick == 0) return RR_OK;
    rc_pad_kernel<true><<<rr_grid_for(n_pick, RC_NT, 64), RC_NT, 0, s>>>(picks, gain, n_pick);
    return rr_launch_status();
  }
  char* ws = static_cast<char*>(workspace);
  KcPair* pairs[2] = {reinterpret_cast<KcPair*>(ws), reinterpret_cast<KcPair*>(ws + KC_PAIRS_BYTES)};
  KcParams p;
  p.x = x; p.ld = ld; p.P = P; p.H = H;
  p.init_dist = init_dist; p.weight = weight;
  p.picks = picks; p.gain = gain; p.min_dist = min_dist; p.assign = assign;
  p.elig = reinterpret_cast<uint8_t*>(ws + 2 * KC_PAIRS_BYTES);
  const int grid = rc_grid(g_blocks.get(), P);
  for (int t = 0; t <= n_pick; ++t) {
    p.t = t;
    p.last = t == n_pick;
    p.prev = pairs[(t + 1) & 1];
    p.out = pairs[t & 1];
    rc_dispatch(H, x, ld, [&](auto ng, auto vec) {
      kc_pass_kernel<decltype(ng)::value, decltype(vec)::value><<<grid, RC_NT, 0, s>>>(p);
    });
    const int st = rr_launch_status();
    if (st != RR_OK) return st;
  }
  return RR_OK;
}

}  // extern "C"
