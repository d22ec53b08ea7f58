// Nearest-neighbour search over reaction embeddings.  A definition of this library, not a port.
//
//   d(m, n) = max(0, (qn[m] + bn[n]) - 2 * dot(m, n))     qn, bn = squared row norms, dot = q[m,:] . bank[n,:], all f32
// and, per query row m, the k bank rows that are smallest under the total order (d ascending, then n ascending) among the rows
// that are not excluded (same non-negative group id, or a NaN distance).  The [M, N] distance matrix is never written.
//
// knn_tile_kernel: grid = row tiles x bank splits, four waves.  A workgroup owns KN_ROWS = 64 query rows and walks its
// contiguous range of the bank in tiles of KN_BANK = 128 rows; both operands stream through LDS in chunks of KN_KC = 64
// columns (fetched into registers one chunk ahead, behind the MFMAs of the chunk before; k-tiles of 16 that lie wholly past H
// are skipped), so H is any value.  Wave w owns the
// bank rows 32 w .. 32 w + 31 of a tile against all 64 query rows: 2 x 4 accumulators of v_mfma_f32_16x16x4_f32
//   A operand  bank[n0 + 32 w + 16 a + (lane & 15)][16 t + 4 (lane >> 4) + j]     one 16-byte LDS read per k-tile, element j ->
//   B operand  q[m0 + 16 b + (lane & 15)][16 t + 4 (lane >> 4) + j]               instruction j
//   C / D      lane holds bank rows 32 w + 16 a + 4 (lane >> 4) + e, e = 0..3, of query row 16 b + (lane & 15)
// The chain of dot(m, n): k-tiles of 16 ascending, inside a tile h = 16 t + 4 qd + j with j = 0..3 outer (one instruction each)
// and qd = 0..3 inside the instruction; columns from H to the next multiple of 16 are zeros.  It depends on the two rows and H only.
// After a tile's MFMAs the distances go to an LDS tile [64][128] (it reuses the staging buffers); wave w then serves the query rows 16 w .. 16 w + 15: a row's
// list of the 64 best so far lives in registers, one slot per lane, sorted.  A tile's 128 candidates are compared against the
// row's k-th best (one readlane, one ballot per half); only survivors are inserted (compare and shift by one lane).
// With more than one split a workgroup writes its rows' lists to the workspace [M, S, k] and knn_merge_kernel (one wave per
// row) merges them under the same order; with one split the lists are the result.  The order is total (n is unique), so the
// result does not depend on the order of insertion: no atomics, run-to-run identical, the same bits for every split count.
//
// kn_walk is the one copy of that walk (staging, chunking, the k-tile skip, the split of the bank); knn_tile_kernel gives it the
// list epilogue above, knn_count_kernel (rr_radius_count_f32, DESIGN section 4k: neighbours within a radius) a counting one
// that needs neither the LDS distance tile nor a list.  Both form the distance through kn_dist.
// kn_run is the one copy of the host side of both entries (checks, splits, workspace, the empty bank, norms, tile launch, merge).
// The sorted list (kn_less, kn_insert, kn_offer, KN_PAD) and the two merge kernels are topk_list.h's, shared with csrc/tanimoto.hip.
//
// row_sqnorm_kernel: one wave per row; lane l sums x[h]^2 over h = l, l + 64, ... ascending (product rounded, then added), the
// 64 partial sums are joined by the butterfly xor 32, 16, 8, 4, 2, 1.  4-byte loads only (a wave reads 256 contiguous bytes).
#include "row_chain.h"
#include "topk_list.h"

namespace {

constexpr int KN_ROWS = 64;                       // query rows per workgroup
constexpr int KN_BANK = 128;                      // bank rows per tile
constexpr int KN_KC = 64;                         // columns staged per chunk
constexpr int KN_SP = KN_KC + 4;                  // pitch of the staged operands (== 4 mod 32: 16 rows x 16 bytes hit 64 banks)
constexpr int KN_DP = KN_BANK + 4;                // pitch of the distance tile
constexpr int KN_RPP = KN_NT / (KN_KC / 4);       // rows of a chunk the 256 threads stage per pass (16 bytes per thread)
constexpr int KN_QU = KN_ROWS / KN_RPP, KN_BU = KN_BANK / KN_RPP;   // passes per chunk: query tile, bank tile
constexpr int KN_STAGE = (KN_ROWS + KN_BANK) * KN_SP, KN_DT = KN_ROWS * KN_DP;
constexpr int KN_LDS = KN_STAGE > KN_DT ? KN_STAGE : KN_DT;        // the distance tile reuses the staging buffers
constexpr int KN_MAX_SPLITS = 1024;

std::atomic<int> g_splits{0};

// what the tile walk reads, and what both epilogues need next to it
struct KnWalk {
  const float* q; int64_t ld_q; int64_t M;
  const float* b; int64_t ld_b; int64_t N;
  int H, S;
  const int32_t* qg; const int32_t* bg;
  const float* qn; const float* bn;
};

struct KnnParams : KnWalk {
  int k;
  float* out_d; int32_t* out_i;                   // S == 1: the result
  float* part_d; int32_t* part_i;                 // S > 1: [M, S, k]
};

struct KnCountParams : KnWalk {
  float r2;
  int32_t* out;                                   // S == 1: the result
  int32_t* part;                                  // S > 1: [M, S]
};

// four consecutive elements of a row from column c (c % 4 == 0): row_chain.h's load with elements at or past `width`, and rows
// that do not exist, replaced by 0
template <bool VEC>
__device__ __forceinline__ f32x4 kn_load4(const float* row, int c, int width, bool row_ok) {
  f32x4 v = rr_load4<VEC>(row, c, width);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = (row_ok && c + e < width) ? v[e] : 0.f;
  return v;
}

// The tile walk, the one copy of it: the workgroup's 64 query rows against its contiguous range of bank tiles, both operands
// staged through `smem` (KN_STAGE floats) chunk by chunk.  tile_begin(n0) runs at a tile's first chunk (what the epilogue wants
// loaded early), tile_end(acc, n0) after its last MFMA with the dot products of the tile that starts at bank row n0; the walk
// passes a barrier before it touches `smem` again, so tile_end may use it between barriers of its own.
template <bool QV, bool BV, class Begin, class End>
__device__ __forceinline__ void kn_walk(const KnWalk& P, float* smem, Begin tile_begin, End tile_end) {
  float* const qs = smem;
  float* const bs = smem + KN_ROWS * KN_SP;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, qd = lane >> 4;
  const int H = P.H;
  const int64_t m0 = static_cast<int64_t>(blockIdx.x) * KN_ROWS;
  const int64_t T = (P.N + KN_BANK - 1) / KN_BANK;
  const int64_t t0 = static_cast<int64_t>(blockIdx.y) * T / P.S, t1 = (static_cast<int64_t>(blockIdx.y) + 1) * T / P.S;
  const int nch = (H + KN_KC - 1) / KN_KC;
  const int64_t total = (t1 - t0) * nch;

  // staging: thread -> (row, 4 columns) of the chunk; KN_QU pieces of q and KN_BU of the bank per thread
  const int srow = tid / (KN_KC / 4), sc4 = (tid % (KN_KC / 4)) * 4;
  f32x4 qv[KN_QU], bv[KN_BU];
  auto fetch = [&](int64_t it) {
    const int64_t tile = it / nch;
    const int c = static_cast<int>(it - tile * nch) * KN_KC + sc4;
    const int64_t n0 = (t0 + tile) * KN_BANK;
#pragma unroll
    for (int u = 0; u < KN_QU; ++u) {
      const int64_t m = m0 + srow + KN_RPP * u;
      const bool ok = m < P.M;
      qv[u] = kn_load4<QV>(P.q + (ok ? m : 0) * P.ld_q, c, H, ok);
    }
#pragma unroll
    for (int u = 0; u < KN_BU; ++u) {
      const int64_t n = n0 + srow + KN_RPP * u;
      const bool ok = n < P.N;
      bv[u] = kn_load4<BV>(P.b + (ok ? n : 0) * P.ld_b, c, H, ok);
    }
  };

  f32x4 acc[2][4];
  if (total > 0) fetch(0);
  int ch = 0;
  int64_t n0 = t0 * KN_BANK;
  for (int64_t it = 0; it < total; ++it) {
    __syncthreads();                              // the chunk before this one has been read by every wave
#pragma unroll
    for (int u = 0; u < KN_QU; ++u) *reinterpret_cast<f32x4*>(qs + (srow + KN_RPP * u) * KN_SP + sc4) = qv[u];
#pragma unroll
    for (int u = 0; u < KN_BU; ++u) *reinterpret_cast<f32x4*>(bs + (srow + KN_RPP * u) * KN_SP + sc4) = bv[u];
    __syncthreads();
    if (it + 1 < total) fetch(it + 1);            // (uniform)
    if (ch == 0) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f32x4(0.f);
      tile_begin(n0);
    }
    const int nt = (H - ch * KN_KC + 15) / 16;    // k-tiles of this chunk that hold anything (uniform)
#pragma unroll
    for (int t = 0; t < KN_KC / 16; ++t) {
      if (t >= nt) break;
      f32x4 af[2], bf[4];
#pragma unroll
      for (int a = 0; a < 2; ++a) af[a] = *reinterpret_cast<const f32x4*>(bs + (32 * wave + 16 * a + l15) * KN_SP + 16 * t + 4 * qd);
#pragma unroll
      for (int b = 0; b < 4; ++b) bf[b] = *reinterpret_cast<const f32x4*>(qs + (16 * b + l15) * KN_SP + 16 * t + 4 * qd);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[a][j], bf[b][j], acc[a][b], 0, 0, 0);
    }
    if (++ch < nch) continue;
    ch = 0;
    tile_end(acc, n0);
    n0 += KN_BANK;
  }
}

// this lane's bank norms of the tile that starts at n0: bank rows 32 w + 16 a + 4 (lane >> 4) + e
__device__ __forceinline__ void kn_tile_norms(const KnWalk& P, int64_t n0, int wave, int qd, float (&bnv)[2][4]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t n = n0 + 32 * wave + 16 * a + 4 * qd + e;
      bnv[a][e] = P.bn[n < P.N ? n : 0];
    }
}

// THE distance of the search and of the count, from a finished dot product (a NaN stays a NaN: it is excluded by the caller)
__device__ __forceinline__ float kn_dist(float qn, float bn, float dot) {
  const float v = (qn + bn) - 2.0f * dot;
  return v < 0.f ? 0.f : v;
}

template <bool QV, bool BV>
__global__ void __launch_bounds__(KN_NT, 2) knn_tile_kernel(const KnnParams P) {
  __shared__ __attribute__((aligned(16))) float smem[KN_LDS];
  float* const dt = smem;                         // between a tile's last MFMA and the next tile's first chunk
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, qd = lane >> 4;
  const int km1 = P.k - 1;
  const int64_t m0 = static_cast<int64_t>(blockIdx.x) * KN_ROWS;

  // the lists of this wave's 16 query rows
  float ld[16];
  int li[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    ld[r] = __builtin_inff();
    li[r] = KN_PAD;
  }
  float qnv[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int64_t m = m0 + 16 * b + l15;
    qnv[b] = P.qn[m < P.M ? m : 0];
  }
  int qgv = -1;                                   // lane r < 16: the group of query row 16 wave + r
  if (P.qg != nullptr) {
    const int64_t m = m0 + 16 * wave + l15;
    qgv = P.qg[m < P.M ? m : 0];
  }
  float bnv[2][4];                                // this lane's bank norms and the candidates' groups of the tile in flight,
  int cn[2], cg[2];                               // loaded at the tile's first chunk, used after its last
  bool cin[2];

  auto tile_begin = [&](int64_t n0) {
    kn_tile_norms(P, n0, wave, qd, bnv);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t n = n0 + lane + 64 * h;
      cin[h] = n < P.N;
      cn[h] = static_cast<int>(cin[h] ? n : 0);
      cg[h] = (P.bg != nullptr) ? P.bg[cn[h]] : -1;
    }
  };
  auto tile_end = [&](const f32x4 (&acc)[2][4], int64_t) {
    // ---- the tile is complete: distances -> LDS (over the staging buffers, once every wave has read its last operands)
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int col = 32 * wave + 16 * a + 4 * qd;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        f32x4 d;
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = kn_dist(qnv[b], bnv[a][e], acc[a][b][e]);
        *reinterpret_cast<f32x4*>(dt + (16 * b + l15) * KN_DP + col) = d;
      }
    }
    __syncthreads();
    // ---- selection: this wave's 16 rows against the tile's 128 candidates, lane = candidate (two halves)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int g = kn_lane_i(qgv, r);
      const float* drow = dt + (16 * wave + r) * KN_DP;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float d = drow[lane + 64 * h];
        const bool valid = cin[h] && d == d && !(g >= 0 && g == cg[h]);
        kn_offer(ld[r], li[r], d, cn[h], valid, km1, lane);
      }
    }
  };
  kn_walk<QV, BV>(P, smem, tile_begin, tile_end);

  // ---- the lists: the result (one split) or this split's partial lists
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t m = m0 + 16 * wave + r;
    if (m < P.M && lane < P.k) {
      if (P.S == 1) {
        P.out_d[m * P.k + lane] = ld[r];
        P.out_i[m * P.k + lane] = li[r] == KN_PAD ? -1 : li[r];
      } else {
        const int64_t o = (m * P.S + blockIdx.y) * P.k + lane;
        P.part_d[o] = ld[r];
        P.part_i[o] = li[r];
      }
    }
  }
}

// Neighbours within a radius: the same walk with a cheaper epilogue - no LDS distance tile, no list.  A lane compares the 32
// distances it holds after a tile (bank rows 32 w + 16 a + 4 (lane >> 4) + e of query row 16 b + (lane & 15)) against r2 and keeps
// one integer per b; after the walk the four lane >> 4 groups are summed by two shuffles and the four waves through LDS, in wave
// order.  One split: the counts are the result; more: this split's column of the partial counts [M, S].
template <bool QV, bool BV>
__global__ void __launch_bounds__(KN_NT, 2) knn_count_kernel(const KnCountParams P) {
  __shared__ __attribute__((aligned(16))) float smem[KN_STAGE];
  __shared__ int s_cnt[KN_NT / 64][KN_ROWS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, qd = lane >> 4;
  const int64_t m0 = static_cast<int64_t>(blockIdx.x) * KN_ROWS;
  const float r2 = P.r2;

  float qnv[4];
  int qgv[4], cnt[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int64_t m = m0 + 16 * b + l15;
    qnv[b] = P.qn[m < P.M ? m : 0];
    qgv[b] = (P.qg != nullptr) ? P.qg[m < P.M ? m : 0] : -1;
    cnt[b] = 0;
  }
  float bnv[2][4];                                // this lane's bank norms, groups and row bounds of the tile in flight
  int bgv[2][4];
  bool bin[2][4];

  auto tile_begin = [&](int64_t n0) {
    kn_tile_norms(P, n0, wave, qd, bnv);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t n = n0 + 32 * wave + 16 * a + 4 * qd + e;
        bin[a][e] = n < P.N;
        bgv[a][e] = (P.bg != nullptr) ? P.bg[bin[a][e] ? n : 0] : -1;
      }
  };
  auto tile_end = [&](const f32x4 (&acc)[2][4], int64_t) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = kn_dist(qnv[b], bnv[a][e], acc[a][b][e]);
          const bool in = bin[a][e] && d <= r2 && !(qgv[b] >= 0 && qgv[b] == bgv[a][e]);   // (d <= r2 is false for a NaN)
          cnt[b] += in ? 1 : 0;
        }
  };
  kn_walk<QV, BV>(P, smem, tile_begin, tile_end);

#pragma unroll
  for (int b = 0; b < 4; ++b) {
    cnt[b] += __shfl_xor(cnt[b], 16, 64);
    cnt[b] += __shfl_xor(cnt[b], 32, 64);
    if (qd == 0) s_cnt[wave][16 * b + l15] = cnt[b];
  }
  __syncthreads();
  const int64_t m = m0 + tid;
  if (tid < KN_ROWS && m < P.M) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < KN_NT / 64; ++w) c += s_cnt[w][tid];
    if (P.S == 1) P.out[m] = c;
    else P.part[m * P.S + blockIdx.y] = c;
  }
}

__global__ void __launch_bounds__(KN_NT) row_sqnorm_kernel(const float* x, int64_t ld, int64_t rows, int H, float* out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * (KN_NT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;                          // (uniform per wave)
  const float* row = x + r * ld;
  float s = 0.f;
  for (int h = lane; h < H; h += 64) {
    const float v = row[h];
    s += v * v;
  }
  s = rr_wave_sum(s);
  if (lane == 0) out[r] = s;
}

// the split count a search of this shape runs with
int kn_splits(int64_t M, int64_t N) {
  const int64_t T = (N + KN_BANK - 1) / KN_BANK;
  if (T <= 1 || M <= 0) return 1;
  int64_t S = g_splits.load(std::memory_order_relaxed);
  if (S == 0) {                                   // automatic: two workgroups per CU, at least four bank tiles per split
    const int64_t row_tiles = (M + KN_ROWS - 1) / KN_ROWS;
    S = (2 * RR_NUM_CU + row_tiles - 1) / row_tiles;
    if (S > T / 4) S = T / 4;
    if (S < 1) S = 1;
  }
  if (S > KN_MAX_SPLITS) S = KN_MAX_SPLITS;
  if (S > T) S = T;
  return static_cast<int>(S);
}

// the workspace of both entries: the norms, then the caller's partial-result area
struct KnLayout { size_t qn, bn, part, total; };
KnLayout kn_layout(int64_t M, int64_t N, size_t part_bytes) {
  KnLayout L;
  size_t o = 0;
  L.qn = o; o += rr_round256(static_cast<size_t>(M) * 4);
  L.bn = o; o += rr_round256(static_cast<size_t>(N) * 4);
  L.part = o; o += part_bytes;
  L.total = o > 256 ? o : 256;
  return L;
}
// one partial-result array [M, S, words] of 4-byte values; a single split writes the result itself
inline size_t kn_part(int64_t M, int S, int words) { return S > 1 ? rr_round256(static_cast<size_t>(M) * S * words * 4) : 0; }

int sqnorm_launch(const float* x, int64_t ld, int64_t rows, int H, float* out, hipStream_t s) {
  const int64_t blocks = (rows + KN_NT / 64 - 1) / (KN_NT / 64);
  if (blocks > 0x7fffffffLL) return RR_ERR_UNSUPPORTED;
  row_sqnorm_kernel<<<static_cast<unsigned>(blocks), KN_NT, 0, s>>>(x, ld, rows, H, out);
  return rr_launch_status();
}

// what both entries take from the C ABI, as given
struct KnArgs {
  const float* q; int64_t ld_q; int64_t M;
  const float* bank; int64_t ld_b; int64_t N;
  int H;
  const int32_t* q_group; const int32_t* b_group; const float* bank_sqnorm;
  void* workspace; size_t workspace_bytes;
  hipStream_t s;
};

// what an entry adds: its checks of what only it takes, and its partial results - `arrays` arrays of [M, S, words] (kn_part)
// behind the norms, merged by a kernel with merge_rows rows per workgroup
struct KnEntry {
  bool args_ok, supported;
  int arrays, words, merge_rows;
};

// the walk's operands, with the norms both entries need: the query norms go to `qn`, the bank norms to `bn` unless the caller has them
int kn_prepare(KnWalk& W, const KnArgs& a, int S, float* qn, float* bn) {
  W.q = a.q; W.ld_q = a.ld_q; W.M = a.M;
  W.b = a.bank; W.ld_b = a.ld_b; W.N = a.N;
  W.H = a.H; W.S = S;
  W.qg = a.q_group; W.bg = a.b_group;
  int st = sqnorm_launch(a.q, a.ld_q, a.M, a.H, qn, a.s);
  if (st != RR_OK) return st;
  W.qn = qn;
  W.bn = a.bank_sqnorm;
  if (!a.bank_sqnorm) {
    st = sqnorm_launch(a.bank, a.ld_b, a.N, a.H, bn, a.s);
    W.bn = bn;
  }
  return st;
}

// The host side of both entries.  tile(QV, BV, grid, part, each) launches the entry's tile kernel - `part` the first of its
// partial-result arrays, `each` the bytes of one -, merge(part, each, S, blocks) its merge kernel; S == 0 (and no arrays) when the
// bank is empty: the merge of nothing writes the padding.
template <class Params, class Tile, class Merge>
int kn_run(Params& P, const KnArgs& a, const KnEntry& e, Tile tile, Merge merge) {
  RR_CHECK_ARG(e.args_ok && a.q && a.bank && a.workspace);
  RR_CHECK_ARG((a.q_group == nullptr) == (a.b_group == nullptr));
  RR_CHECK_ARG(a.M >= 0 && a.N >= 0 && a.H >= 1 && a.ld_q >= a.H && a.ld_b >= a.H);
  if (!e.supported) return RR_ERR_UNSUPPORTED;
  const int S = kn_splits(a.M, a.N);
  const size_t each = kn_part(a.M, S, e.words);
  const KnLayout L = kn_layout(a.M, a.N, e.arrays * each);
  if (a.workspace_bytes < L.total) return RR_ERR_WORKSPACE;
  if (a.M == 0) return RR_OK;
  const int64_t row_tiles = (a.M + KN_ROWS - 1) / KN_ROWS, merge_blocks = (a.M + e.merge_rows - 1) / e.merge_rows;
  if (merge_blocks > 0x7fffffffLL) return RR_ERR_UNSUPPORTED;
  if (a.N == 0) {
    merge(nullptr, 0, 0, static_cast<unsigned>(merge_blocks));
    return rr_launch_status();
  }
  char* ws = static_cast<char*>(a.workspace);
  int st = kn_prepare(P, a, S, reinterpret_cast<float*>(ws + L.qn), reinterpret_cast<float*>(ws + L.bn));
  if (st != RR_OK) return st;
  const dim3 grid(static_cast<unsigned>(row_tiles), static_cast<unsigned>(S));
  rr_vec_dispatch(rr_vec4_ok(a.q, a.ld_q), [&](auto qv) {
    rr_vec_dispatch(rr_vec4_ok(a.bank, a.ld_b), [&](auto bv) { tile(qv, bv, grid, ws + L.part, each); });
  });
  st = rr_launch_status();
  if (st != RR_OK || S == 1) return st;
  merge(ws + L.part, each, S, static_cast<unsigned>(merge_blocks));
  return rr_launch_status();
}

}  // namespace

extern "C" {

void rr_knn_geometry(int* row_tile, int* bank_tile, int* max_k) {
  if (row_tile) *row_tile = KN_ROWS;
  if (bank_tile) *bank_tile = KN_BANK;
  if (max_k) *max_k = RR_KNN_MAX_K;
}

int rr_knn_splits(void) { return g_splits.load(std::memory_order_relaxed); }

int rr_knn_set_splits(int splits) {
  RR_CHECK_ARG(splits >= 0 && splits <= KN_MAX_SPLITS);
  g_splits.store(splits, std::memory_order_relaxed);
  return RR_OK;
}

int rr_row_sqnorm_f32(const float* x, int64_t ld, int64_t rows, int H, float* out, rr_stream_t stream) {
  RR_CHECK_ARG(x && out && rows >= 0 && H >= 1 && ld >= H);
  if (rows == 0) return RR_OK;
  return sqnorm_launch(x, ld, rows, H, out, static_cast<hipStream_t>(stream));
}

int rr_knn_workspace_bytes(int64_t M, int64_t N, int k, size_t* bytes) {
  RR_CHECK_ARG(bytes && M >= 0 && N >= 0 && k >= 1);
  if (k > RR_KNN_MAX_K || N > 0x7fffffffLL) return RR_ERR_UNSUPPORTED;
  *bytes = kn_layout(M, N, 2 * kn_part(M, kn_splits(M, N), k)).total;
  return RR_OK;
}

int rr_knn_f32(const float* q, int64_t ld_q, int64_t M, const float* bank, int64_t ld_b, int64_t N, int H, int k,
               const int32_t* q_group, const int32_t* b_group, const float* bank_sqnorm, float* dist, int32_t* idx,
               void* workspace, size_t workspace_bytes, rr_stream_t stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const KnArgs a{q, ld_q, M, bank, ld_b, N, H, q_group, b_group, bank_sqnorm, workspace, workspace_bytes, s};
  KnEntry e;
  e.args_ok = dist && idx && k >= 1;
  e.supported = k <= RR_KNN_MAX_K && N <= 0x7fffffffLL;
  e.arrays = 2; e.words = k;                      // the lists: distances, then indices
  e.merge_rows = KN_NT / 64;                      // one wave per row
  KnnParams P;
  P.k = k;
  P.out_d = dist; P.out_i = idx;
  return kn_run(
      P, a, e,
      [&](auto qv, auto bv, dim3 grid, char* part, size_t each) {
        P.part_d = reinterpret_cast<float*>(part);
        P.part_i = reinterpret_cast<int32_t*>(part + each);
        knn_tile_kernel<decltype(qv)::value, decltype(bv)::value><<<grid, KN_NT, 0, s>>>(P);
      },
      [&](const char* part, size_t each, int S, unsigned blocks) {
        knn_merge_kernel<<<blocks, KN_NT, 0, s>>>(reinterpret_cast<const float*>(part), reinterpret_cast<const int32_t*>(part + each),
                                                  M, S, k, dist, idx);
      });
}

int rr_radius_count_workspace_bytes(int64_t M, int64_t N, size_t* bytes) {
  RR_CHECK_ARG(bytes && M >= 0 && N >= 0);
  if (M > 0x7fffffffLL || N > 0x7fffffffLL) return RR_ERR_UNSUPPORTED;
  *bytes = kn_layout(M, N, kn_part(M, kn_splits(M, N), 1)).total;
  return RR_OK;
}

int rr_radius_count_f32(const float* q, int64_t ld_q, int64_t M, const float* bank, int64_t ld_b, int64_t N, int H, float r2,
                        const int32_t* q_group, const int32_t* b_group, const float* bank_sqnorm, int32_t* count,
                        void* workspace, size_t workspace_bytes, rr_stream_t stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const KnArgs a{q, ld_q, M, bank, ld_b, N, H, q_group, b_group, bank_sqnorm, workspace, workspace_bytes, s};
  KnEntry e;
  e.args_ok = count && r2 >= 0.f;                 // (false for a NaN)
  e.supported = M <= 0x7fffffffLL && N <= 0x7fffffffLL;
  e.arrays = 1; e.words = 1;                      // one count per row and split
  e.merge_rows = KN_NT;                           // one thread per row
  KnCountParams P;
  P.r2 = r2;
  P.out = count;
  return kn_run(
      P, a, e,
      [&](auto qv, auto bv, dim3 grid, char* part, size_t) {
        P.part = reinterpret_cast<int32_t*>(part);
        knn_count_kernel<decltype(qv)::value, decltype(bv)::value><<<grid, KN_NT, 0, s>>>(P);
      },
      [&](const char* part, size_t, int S, unsigned blocks) {
        knn_count_merge_kernel<<<blocks, KN_NT, 0, s>>>(reinterpret_cast<const int32_t*>(part), M, S, count);
      });
}

}  // extern "C"
