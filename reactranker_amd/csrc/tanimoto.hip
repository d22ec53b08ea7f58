// Tanimoto search on bit rows.  A definition of this library.  For query row m and bank row n of W words:
//   c = popcount(q & b)      u = |q| + |b| - c      d(m, n) = u == 0 ? 0 : (float)(u - c) / (float)u     one correctly rounded f32
// division of exact integers (u <= 32 W <= 8192); per query row the k bank rows smallest under knn's total order (d ascending,
// then n ascending) among the rows that are not excluded (same non-negative group id), or the number of rows with d <= radius.
//
// tn_tile_kernel: grid = row tiles x bank splits, four waves.  A workgroup owns TN_ROWS = 64 query rows and walks its contiguous
// range of the bank in tiles of TN_BANK = 128 rows.  Wave w serves the query rows 16 w .. 16 w + 15 with lane = candidate: a lane
// holds the words of bank rows n0 + lane and n0 + 64 + lane, TN_WC = 16 at a time, in registers (fetched one chunk ahead, straight
// from global memory: 16-byte loads where pointer and pitch allow, 4-byte loads otherwise), so no LDS read ever has lanes on
// different addresses.  The query words are the same for all lanes of a wave: they are staged in LDS, a panel of TN_QP = 64
// words per row (once per workgroup when W <= 64, else once per panel and tile), and read as broadcasts.  Per word and candidate:
// one v_and, one v_bcnt that also accumulates.  After a tile's last chunk the 2 x 16 sums of a lane are exactly the candidates
// kn_offer wants (lane = candidate, two halves): no LDS distance tile.  The count form keeps one integer per row and lane and
// sums the lanes at the end.  Splits, the partial results [M, S, k] / [M, S] and their merge are knn's (topk_list.h): the same
// bits for every split count.
// row_popcount_kernel: one wave per row; lane l sums popcount over the words l, l + 64, ...; the lanes are summed (integers).
#include "row_chain.h"
#include "topk_list.h"

namespace {

constexpr int TN_ROWS = 64;                       // query rows per workgroup
constexpr int TN_BANK = 128;                      // bank rows per tile (two per lane)
constexpr int TN_WC = 16;                         // words of a bank row a lane holds at a time
constexpr int TN_QP = 64;                         // words per query row staged in LDS (a panel)
constexpr int TN_PCH = TN_QP / TN_WC;             // chunks per panel
constexpr int TN_MAX_SPLITS = 1024;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) u32x4* tn_gptr4;

std::atomic<int> g_tn_splits{0};

struct TnParams {
  const uint32_t* q; int64_t ld_q; int64_t M;
  const uint32_t* b; int64_t ld_b; int64_t N;
  int W, S;
  const int32_t* qg; const int32_t* bg;
  const int32_t* qp; const int32_t* bp;           // popcounts per row
  int k; float radius;
  float* out_d; int32_t* out_i; int32_t* out_c;   // S == 1: the result
  float* part_d; int32_t* part_i; int32_t* part_c;   // S > 1: [M, S, k] / [M, S]
};

// words c .. c + 3 of a row (c % 4 == 0); words at or past W, and rows that do not exist, are 0.  Every load is unconditional on a
// clamped address (VEC: ld % 4 == 0, so the group lies inside the row's pitch).
template <bool VEC>
__device__ __forceinline__ u32x4 tn_load4(const uint32_t* row, int c, int W, bool row_ok) {
  u32x4 v;
  if (VEC) {
    v = *(tn_gptr4)(row + (c < W ? c : 0));
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = row[c + e < W ? c + e : 0];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = (row_ok && c + e < W) ? v[e] : 0u;
  return v;
}

// THE distance of the search and of the count, from exact integers
__device__ __forceinline__ float tn_dist(int qp, int bp, int c) {
  const int u = qp + bp - c;
  return u == 0 ? 0.f : __fdiv_rn(static_cast<float>(u - c), static_cast<float>(u));
}

template <bool QV, bool BV, bool COUNT>
__global__ void __launch_bounds__(KN_NT, 2) tn_tile_kernel(const TnParams P) {
  __shared__ __attribute__((aligned(16))) uint32_t qs[TN_ROWS * TN_QP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int W = P.W, km1 = P.k - 1;
  const int64_t m0 = static_cast<int64_t>(blockIdx.x) * TN_ROWS;
  const int64_t T = (P.N + TN_BANK - 1) / TN_BANK;
  const int64_t t0 = static_cast<int64_t>(blockIdx.y) * T / P.S, t1 = (static_cast<int64_t>(blockIdx.y) + 1) * T / P.S;
  const int nch = (W + TN_WC - 1) / TN_WC;
  const bool panels = nch > TN_PCH;               // the query rows do not fit one panel: restage per panel and tile
  const int64_t total = (t1 - t0) * nch;

  // lane r < 16: popcount and group of query row 16 wave + r
  int qpv = 0, qgv = -1;
  {
    const int64_t m = m0 + 16 * wave + (lane & 15);
    qpv = P.qp[m < P.M ? m : 0];
    if (P.qg != nullptr) qgv = P.qg[m < P.M ? m : 0];
  }
  float ld[COUNT ? 1 : 16];
  int li[16];                                     // the lists' indices; the count form keeps its counts here
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    if (!COUNT) ld[r] = __builtin_inff();
    li[r] = COUNT ? 0 : KN_PAD;
  }

  // the query panel that starts at word w0: thread -> (row, 4 words), four rows per thread
  auto stage_q = [&](int w0) {
    const int srow = tid >> 4, c4 = (tid & 15) * 4;
#pragma unroll
    for (int u = 0; u < TN_ROWS / 16; ++u) {
      const int64_t m = m0 + srow + 16 * u;
      const bool ok = m < P.M;
      const u32x4 v = tn_load4<QV>(P.q + (ok ? m : 0) * P.ld_q, w0 + c4, W, ok);
      *reinterpret_cast<u32x4*>(qs + (srow + 16 * u) * TN_QP + c4) = v;
    }
  };

  // the bank chunk in flight: this lane's two rows, TN_WC words each
  u32x4 nxt[2][TN_WC / 4], cur[2][TN_WC / 4];
  auto fetch = [&](int64_t tile, int ch) {
    const int64_t n0 = (t0 + tile) * TN_BANK;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t n = n0 + lane + 64 * h;
      const bool ok = n < P.N;
      const uint32_t* row = P.b + (ok ? n : 0) * P.ld_b;
#pragma unroll
      for (int j = 0; j < TN_WC / 4; ++j) nxt[h][j] = tn_load4<BV>(row, ch * TN_WC + 4 * j, W, ok);
    }
  };

  int acc[16][2];
  int cn[2], cg[2], cbp[2];                       // this lane's two candidates of the tile in flight
  bool cin[2];
  if (total > 0) fetch(0, 0);
  int ch = 0;
  int64_t tile = 0;
  for (int64_t it = 0; it < total; ++it) {
    if (ch % TN_PCH == 0 && (panels || it == 0)) {   // (uniform)
      __syncthreads();                            // every wave has read the panel before
      stage_q(ch * TN_WC);
      __syncthreads();
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int j = 0; j < TN_WC / 4; ++j) cur[h][j] = nxt[h][j];
    if (it + 1 < total) {                         // (uniform)
      const bool wrap = ch + 1 == nch;
      fetch(wrap ? tile + 1 : tile, wrap ? 0 : ch + 1);
    }
    if (ch == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r][0] = acc[r][1] = 0;
      const int64_t n0 = (t0 + tile) * TN_BANK;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int64_t n = n0 + lane + 64 * h;
        cin[h] = n < P.N;
        cn[h] = static_cast<int>(cin[h] ? n : 0);
        cbp[h] = P.bp[cn[h]];
        cg[h] = (P.bg != nullptr) ? P.bg[cn[h]] : -1;
      }
    }
    const uint32_t* qc = qs + (16 * wave) * TN_QP + (ch % TN_PCH) * TN_WC;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
      for (int j = 0; j < TN_WC / 4; ++j) {
        const u32x4 qw = *reinterpret_cast<const u32x4*>(qc + r * TN_QP + 4 * j);   // (one address per wave: a broadcast)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[r][0] += __popc(qw[e] & cur[0][j][e]);
          acc[r][1] += __popc(qw[e] & cur[1][j][e]);
        }
      }
    }
    if (++ch < nch) continue;
    ch = 0;
    ++tile;
    // ---- the tile is complete: this wave's 16 rows against its 128 candidates, lane = candidate (two halves)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int g = kn_lane_i(qgv, r);
      const int qp = kn_lane_i(qpv, r);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float d = tn_dist(qp, cbp[h], acc[r][h]);
        const bool valid = cin[h] && !(g >= 0 && g == cg[h]);
        if (COUNT) li[r] += (valid && d <= P.radius) ? 1 : 0;
        else kn_offer(ld[COUNT ? 0 : r], li[r], d, cn[h], valid, km1, lane);
      }
    }
  }

  // ---- the result (one split) or this split's partial result
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t m = m0 + 16 * wave + r;
    if (COUNT) {
      const int c = rr_wave_sum(li[r]);
      if (m < P.M && lane == 0) {
        if (P.S == 1) P.out_c[m] = c;
        else P.part_c[m * P.S + blockIdx.y] = c;
      }
    } else if (m < P.M && lane < P.k) {
      if (P.S == 1) {
        P.out_d[m * P.k + lane] = ld[COUNT ? 0 : r];
        P.out_i[m * P.k + lane] = li[r] == KN_PAD ? -1 : li[r];
      } else {
        const int64_t o = (m * P.S + blockIdx.y) * P.k + lane;
        P.part_d[o] = ld[COUNT ? 0 : r];
        P.part_i[o] = li[r];
      }
    }
  }
}

__global__ void __launch_bounds__(KN_NT) row_popcount_kernel(const uint32_t* x, int64_t ld, int64_t rows, int W, int32_t* out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * (KN_NT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;                          // (uniform per wave)
  const uint32_t* row = x + r * ld;
  int s = 0;
  for (int w = lane; w < W; w += 64) s += __popc(row[w]);
  s = rr_wave_sum(s);
  if (lane == 0) out[r] = s;
}

// the split count a search of this shape runs with (knn's rule)
int tn_splits(int64_t M, int64_t N) {
  const int64_t T = (N + TN_BANK - 1) / TN_BANK;
  if (T <= 1 || M <= 0) return 1;
  int64_t S = g_tn_splits.load(std::memory_order_relaxed);
  if (S == 0) {                                   // automatic: two workgroups per CU, at least four bank tiles per split
    const int64_t row_tiles = (M + TN_ROWS - 1) / TN_ROWS;
    S = (2 * RR_NUM_CU + row_tiles - 1) / row_tiles;
    if (S > T / 4) S = T / 4;
    if (S < 1) S = 1;
  }
  if (S > TN_MAX_SPLITS) S = TN_MAX_SPLITS;
  if (S > T) S = T;
  return static_cast<int>(S);
}

// the workspace of both entries: the popcounts, then the partial results
struct TnLayout { size_t qp, bp, part, total; };
TnLayout tn_layout(int64_t M, int64_t N, size_t part_bytes) {
  TnLayout L;
  size_t o = 0;
  L.qp = o; o += rr_round256(static_cast<size_t>(M) * 4);
  L.bp = o; o += rr_round256(static_cast<size_t>(N) * 4);
  L.part = o; o += part_bytes;
  L.total = o > 256 ? o : 256;
  return L;
}
inline size_t tn_part(int64_t M, int S, int words) { return S > 1 ? rr_round256(static_cast<size_t>(M) * S * words * 4) : 0; }

int popcount_launch(const uint32_t* x, int64_t ld, int64_t rows, int W, int32_t* out, hipStream_t s) {
  const int64_t blocks = (rows + KN_NT / 64 - 1) / (KN_NT / 64);
  if (blocks > 0x7fffffffLL) return RR_ERR_UNSUPPORTED;
  row_popcount_kernel<<<static_cast<unsigned>(blocks), KN_NT, 0, s>>>(x, ld, rows, W, out);
  return rr_launch_status();
}

struct TnArgs {
  const uint32_t* q; int64_t ld_q; int64_t M;
  const uint32_t* bank; int64_t ld_b; int64_t N;
  int W;
  const int32_t* q_group; const int32_t* b_group; const int32_t* bank_popcount;
  void* workspace; size_t workspace_bytes;
  hipStream_t s;
};

// The host side of both entries: the checks, the splits, the workspace, the empty bank, the popcounts, the tile launch and the
// merge.  COUNT: the radius count (one word per row and split), else the search (two arrays of k words).
template <bool COUNT>
int tn_run(TnParams& P, const TnArgs& a, bool args_ok, bool supported) {
  RR_CHECK_ARG(args_ok && a.q && a.bank && a.workspace);
  RR_CHECK_ARG((a.q_group == nullptr) == (a.b_group == nullptr));
  RR_CHECK_ARG(a.M >= 0 && a.N >= 0 && a.W >= 1 && a.ld_q >= a.W && a.ld_b >= a.W);
  if (!supported || a.W > RR_TANIMOTO_MAX_WORDS || a.N > 0x7fffffffLL) return RR_ERR_UNSUPPORTED;
  const int S = tn_splits(a.M, a.N);
  const int words = COUNT ? 1 : P.k;
  const size_t each = tn_part(a.M, S, words);
  const TnLayout L = tn_layout(a.M, a.N, (COUNT ? 1 : 2) * each);
  if (a.workspace_bytes < L.total) return RR_ERR_WORKSPACE;
  if (a.M == 0) return RR_OK;
  const int merge_rows = COUNT ? KN_NT : KN_NT / 64;
  const int64_t row_tiles = (a.M + TN_ROWS - 1) / TN_ROWS, merge_blocks = (a.M + merge_rows - 1) / merge_rows;
  if (merge_blocks > 0x7fffffffLL) return RR_ERR_UNSUPPORTED;
  char* ws = static_cast<char*>(a.workspace);
  auto merge = [&](int splits) {
    if (COUNT)
      knn_count_merge_kernel<<<static_cast<unsigned>(merge_blocks), KN_NT, 0, a.s>>>(P.part_c, a.M, splits, P.out_c);
    else
      knn_merge_kernel<<<static_cast<unsigned>(merge_blocks), KN_NT, 0, a.s>>>(P.part_d, P.part_i, a.M, splits, P.k, P.out_d, P.out_i);
  };
  P.part_d = reinterpret_cast<float*>(ws + L.part);
  P.part_i = reinterpret_cast<int32_t*>(ws + L.part + each);
  P.part_c = reinterpret_cast<int32_t*>(ws + L.part);
  if (a.N == 0) {                                 // the merge of nothing writes the padding / the zeros
    merge(0);
    return rr_launch_status();
  }
  P.q = a.q; P.ld_q = a.ld_q; P.M = a.M;
  P.b = a.bank; P.ld_b = a.ld_b; P.N = a.N;
  P.W = a.W; P.S = S;
  P.qg = a.q_group; P.bg = a.b_group;
  int32_t* qp = reinterpret_cast<int32_t*>(ws + L.qp);
  int st = popcount_launch(a.q, a.ld_q, a.M, a.W, qp, a.s);
  if (st != RR_OK) return st;
  P.qp = qp;
  P.bp = a.bank_popcount;
  if (!a.bank_popcount) {
    int32_t* bp = reinterpret_cast<int32_t*>(ws + L.bp);
    st = popcount_launch(a.bank, a.ld_b, a.N, a.W, bp, a.s);
    if (st != RR_OK) return st;
    P.bp = bp;
  }
  const dim3 grid(static_cast<unsigned>(row_tiles), static_cast<unsigned>(S));
  rr_vec_dispatch(rr_vec4_ok(a.q, a.ld_q), [&](auto qv) {
    rr_vec_dispatch(rr_vec4_ok(a.bank, a.ld_b), [&](auto bv) {
      tn_tile_kernel<decltype(qv)::value, decltype(bv)::value, COUNT><<<grid, KN_NT, 0, a.s>>>(P);
    });
  });
  st = rr_launch_status();
  if (st != RR_OK || S == 1) return st;
  merge(S);
  return rr_launch_status();
}

}  // namespace

extern "C" {

void rr_tanimoto_geometry(int* row_tile, int* bank_tile, int* max_k, int* max_words) {
  if (row_tile) *row_tile = TN_ROWS;
  if (bank_tile) *bank_tile = TN_BANK;
  if (max_k) *max_k = RR_KNN_MAX_K;
  if (max_words) *max_words = RR_TANIMOTO_MAX_WORDS;
}

int rr_tanimoto_splits(void) { return g_tn_splits.load(std::memory_order_relaxed); }

int rr_tanimoto_set_splits(int splits) {
  RR_CHECK_ARG(splits >= 0 && splits <= TN_MAX_SPLITS);
  g_tn_splits.store(splits, std::memory_order_relaxed);
  return RR_OK;
}

int rr_row_popcount_u32(const uint32_t* x, int64_t ld, int64_t rows, int W, int32_t* out, rr_stream_t stream) {
  RR_CHECK_ARG(x && out && rows >= 0 && W >= 1 && ld >= W);
  if (rows == 0) return RR_OK;
  return popcount_launch(x, ld, rows, W, out, static_cast<hipStream_t>(stream));
}

int rr_tanimoto_knn_workspace_bytes(int64_t M, int64_t N, int k, size_t* bytes) {
  RR_CHECK_ARG(bytes && M >= 0 && N >= 0 && k >= 1);
  if (k > RR_KNN_MAX_K || N > 0x7fffffffLL) return RR_ERR_UNSUPPORTED;
  *bytes = tn_layout(M, N, 2 * tn_part(M, tn_splits(M, N), k)).total;
  return RR_OK;
}

int rr_tanimoto_knn_u32(const uint32_t* q, int64_t ld_q, int64_t M, const uint32_t* bank, int64_t ld_b, int64_t N, int W, int k,
                        const int32_t* q_group, const int32_t* b_group, const int32_t* bank_popcount, float* dist, int32_t* idx,
                        void* workspace, size_t workspace_bytes, rr_stream_t stream) {
  const TnArgs a{q, ld_q, M, bank, ld_b, N, W, q_group, b_group, bank_popcount, workspace, workspace_bytes,
                 static_cast<hipStream_t>(stream)};
  TnParams P{};
  P.k = k;
  P.out_d = dist; P.out_i = idx;
  return tn_run<false>(P, a, dist && idx && k >= 1, k <= RR_KNN_MAX_K);
}

int rr_tanimoto_count_workspace_bytes(int64_t M, int64_t N, size_t* bytes) {
  RR_CHECK_ARG(bytes && M >= 0 && N >= 0);
  if (M > 0x7fffffffLL || N > 0x7fffffffLL) return RR_ERR_UNSUPPORTED;
  *bytes = tn_layout(M, N, tn_part(M, tn_splits(M, N), 1)).total;
  return RR_OK;
}

int rr_tanimoto_count_u32(const uint32_t* q, int64_t ld_q, int64_t M, const uint32_t* bank, int64_t ld_b, int64_t N, int W,
                          float radius, const int32_t* q_group, const int32_t* b_group, const int32_t* bank_popcount,
                          int32_t* count, void* workspace, size_t workspace_bytes, rr_stream_t stream) {
  const TnArgs a{q, ld_q, M, bank, ld_b, N, W, q_group, b_group, bank_popcount, workspace, workspace_bytes,
                 static_cast<hipStream_t>(stream)};
  TnParams P{};
  P.k = 1;
  P.radius = radius;
  P.out_c = count;
  return tn_run<true>(P, a, count && radius >= 0.f, M <= 0x7fffffffLL);   // (radius >= 0 is false for a NaN)
}

}  // extern "C"
