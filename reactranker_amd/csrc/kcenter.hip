// Greedy k-center selection over reaction embeddings.  A definition of this library, not a port;
// include/reactranker_hip.h states it.
//
//   d(i, c) = sum_h (x[i,h] - x[c,h])^2 in f32 by the fixed chain: columns in groups of four, lane l of the wave owns the groups
//   g with g % 64 == l (ascending, columns inside a group ascending), acc = acc + t * t with t = x[i,h] - x[c,h], the 64 chains
//   joined by the butterfly xor 32, 16, 8, 4, 2, 1.  The chain and the row loads live in row_chain.h (csrc/cluster.hip shares them).
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
#include "rr_common.h"
#include "row_chain.h"

#include <atomic>

namespace {

constexpr int KC_NT = 256;                        // threads (4 waves: 4 rows per workgroup and grid pass)
constexpr int KC_WAVES = KC_NT / 64;
constexpr int KC_MAX_BLOCKS = 4096;
constexpr int KC_MAX_NG = 4;                      // register path up to H = 256 * KC_MAX_NG
constexpr int KC_AUTO_BLOCKS = RR_NUM_CU * 4;     // 16 waves per CU: measured best or within 4 % of it from P = 10^4 to 10^6

std::atomic<int> g_blocks{0};

struct __attribute__((aligned(8))) KcPair { float s; int32_t i; };   // i < 0: no eligible row

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
__global__ void __launch_bounds__(KC_NT) kc_pass_kernel(const KcParams p) {
  __shared__ KcPair s_prev[KC_WAVES], s_out[KC_WAVES];
  constexpr int NR = NG > 0 ? NG : 1;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = p.H, t = p.t;
  const bool weighted = p.weight != nullptr;

  int c = -1;                                     // the centre: the winner of round t - 1
  f32x4 cv[NR];
  const float* crow = p.x;
  if (t > 0) {
    float bs = 0.f;
    int bi = -1;
    for (int k = tid; k < static_cast<int>(gridDim.x); k += KC_NT) {
      const KcPair q = p.prev[k];
      if (rr_first_max_replaces(q.s, q.i, bs, bi)) { bs = q.s; bi = q.i; }
    }
    rr_wave_first_max(bs, bi);
    if (lane == 0) { s_prev[wave].s = bs; s_prev[wave].i = bi; }
    __syncthreads();
    bs = s_prev[0].s; bi = s_prev[0].i;
#pragma unroll
    for (int w = 1; w < KC_WAVES; ++w)
      if (rr_first_max_replaces(s_prev[w].s, s_prev[w].i, bs, bi)) { bs = s_prev[w].s; bi = s_prev[w].i; }
    c = __builtin_amdgcn_readfirstlane(bi);
    if (blockIdx.x == 0 && tid == 0) {
      p.picks[t - 1] = c;
      p.gain[t - 1] = c >= 0 ? bs : -1.0f;
    }
    if (c < 0) {                                  // nothing was eligible, so nothing will be: no update, no candidate
      if (tid == 0 && !p.last) { p.out[blockIdx.x].s = 0.f; p.out[blockIdx.x].i = -1; }
      return;
    }
    crow = p.x + static_cast<int64_t>(c) * p.ld;
    if (NG > 0) kc_load_row<NR, VEC>(crow, lane, H, cv);
  }

  float best_s = 0.f;
  int best_i = -1;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * KC_WAVES;
  const int64_t first = static_cast<int64_t>(blockIdx.x) * KC_WAVES + wave;

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
  if (lane == 0) { s_out[wave].s = best_s; s_out[wave].i = best_i; }
  __syncthreads();
  if (tid == 0) {
    float bs = s_out[0].s;
    int bi = s_out[0].i;
#pragma unroll
    for (int w = 1; w < KC_WAVES; ++w)
      if (rr_first_max_replaces(s_out[w].s, s_out[w].i, bs, bi)) { bs = s_out[w].s; bi = s_out[w].i; }
    p.out[blockIdx.x].s = bs;
    p.out[blockIdx.x].i = bi;
  }
}

// P == 0: every slot of picks / gain is padding
__global__ void __launch_bounds__(KC_NT) kc_pad_kernel(int32_t* picks, float* gain, int n) {
  for (int k = blockIdx.x * KC_NT + threadIdx.x; k < n; k += gridDim.x * KC_NT) {
    picks[k] = -1;
    gain[k] = -1.0f;
  }
}

inline size_t kc_round(size_t b) { return (b + 255) & ~static_cast<size_t>(255); }

// the workspace: two pair arrays sized for the largest grid (so the size does not depend on the blocks setting), then elig [P]
constexpr size_t KC_PAIRS_BYTES = static_cast<size_t>(KC_MAX_BLOCKS) * sizeof(KcPair);
inline size_t kc_workspace(int64_t P) { return 2 * KC_PAIRS_BYTES + kc_round(static_cast<size_t>(P)); }

int kc_grid(int64_t P) {
  int64_t b = g_blocks.load(std::memory_order_relaxed);
  if (b == 0) {                                   // automatic: two rows per wave and launch at least, 16 waves per CU at most
    b = (P + 2 * KC_WAVES - 1) / (2 * KC_WAVES);
    if (b > KC_AUTO_BLOCKS) b = KC_AUTO_BLOCKS;
    if (b < 1) b = 1;
  }
  return static_cast<int>(b);
}

template <int NG>
void kc_launch(bool vec, int grid, hipStream_t s, const KcParams& p) {
  if (vec) kc_pass_kernel<NG, true><<<grid, KC_NT, 0, s>>>(p);
  else kc_pass_kernel<NG, false><<<grid, KC_NT, 0, s>>>(p);
}

}  // namespace

extern "C" {

int rr_kcenter_blocks(void) { return g_blocks.load(std::memory_order_relaxed); }

int rr_kcenter_set_blocks(int blocks) {
  RR_CHECK_ARG(blocks >= 0 && blocks <= KC_MAX_BLOCKS);
  g_blocks.store(blocks, std::memory_order_relaxed);
  return RR_OK;
}

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
    kc_pad_kernel<<<rr_grid_for(n_pick, KC_NT, 64), KC_NT, 0, s>>>(picks, gain, n_pick);
    return rr_launch_status();
  }
  char* ws = static_cast<char*>(workspace);
  KcPair* pairs[2] = {reinterpret_cast<KcPair*>(ws), reinterpret_cast<KcPair*>(ws + KC_PAIRS_BYTES)};
  KcParams p;
  p.x = x; p.ld = ld; p.P = P; p.H = H;
  p.init_dist = init_dist; p.weight = weight;
  p.picks = picks; p.gain = gain; p.min_dist = min_dist; p.assign = assign;
  p.elig = reinterpret_cast<uint8_t*>(ws + 2 * KC_PAIRS_BYTES);
  const int grid = kc_grid(P);
  const bool vec = rr_aligned16(x) && (ld % 4 == 0);
  const int groups = (H + 3) / 4, ng = (groups + 63) / 64;
  for (int t = 0; t <= n_pick; ++t) {
    p.t = t;
    p.last = t == n_pick;
    p.prev = pairs[(t + 1) & 1];
    p.out = pairs[t & 1];
    switch (ng <= KC_MAX_NG ? ng : 0) {
      case 1: kc_launch<1>(vec, grid, s, p); break;
      case 2: kc_launch<2>(vec, grid, s, p); break;
      case 3: kc_launch<3>(vec, grid, s, p); break;
      case 4: kc_launch<4>(vec, grid, s, p); break;
      default: kc_launch<0>(vec, grid, s, p); break;
    }
    const int st = rr_launch_status();
    if (st != RR_OK) return st;
  }
  return RR_OK;
}

}  // extern "C"
