// A Gaussian model of the embedding space: second moments of the rows of a matrix in f64, and the centred
// projection with a fused row norm that Mahalanobis distances, whitening and PCA scores are.  A definition of this library, not
// a port; include/reactranker_hip.h states both.
//
// rr_col_moments_f64: five launches on the caller's stream, no atomics, nothing that depends on an order of arrival.
//   mo_flag_kernel     one wavefront per row (rows grid-strided): flags[n] = 1 when every value of row n is finite, else 0 (the
//                      finite rule and the row load are row_chain.h's, shared with kcenter.hip and cluster.hip; the loop
//                      over the row is written out here, see the kernel)
//   mo_colsum_kernel   grid = 64-column blocks x chunks.  A thread owns four columns and the rows q, q + 16, ... of its chunk
//                      (q = 0..15); the 16 partial sums of a column are added in ascending q.  Block 0 also counts the chunk's rows.
//   mo_mean_kernel     mean[h] = (0.0 + chunk sums ascending) / n_used, n_used = the chunks' row counts added up
//   mo_scatter_kernel  grid = 64 x 64 macro tiles on or below the diagonal x chunks, four waves, each a 32 x 32 quarter = 2 x 2
//                      accumulators of v_mfma_f64_16x16x4_f64.  32 rows of the chunk at a time are centred in f64
//                      (c = (double)x - mean, exact zeros for a flagged row, a row past the chunk or a column past H) and staged in
//                      LDS; one instruction takes four consecutive rows:
//                        A operand  c[r + (lane >> 4)][i0 + (lane & 15)]      B operand  c[r + (lane >> 4)][j0 + (lane & 15)]
//                        C / D      lane holds rows i0 + (lane >> 4) + 4 e, e = 0..3, of column j0 + (lane & 15)      (the f64 map)
//                      16 x 16 tiles above the diagonal or wholly past H issue nothing.  The chunk's tile goes to its slab.
//   mo_finish_kernel   scatter[i][j] = scatter[j][i] = 0.0 + slab_0[i][j] + slab_1[i][j] + ... for j <= i
// The chunking is a function of N and H only (mo_chunks), so neither the grid of the strided kernels (the blocks setting) nor
// the pitch nor the alignment reaches a bit of the result.
//
// rr_center_project_f32: one launch.  A workgroup owns 64 rows (tiles grid-strided), wave w the rows 16 w .. 16 w + 15.  R is
// walked in groups of 64 columns, H in chunks of 64: the centred rows (x - center rounded in f32) and the chunk of W (transposed)
// stream through LDS, 4 accumulators of v_mfma_f32_16x16x4_f32 per wave:
//   A operand  W[16 t + 4 (lane >> 4) + j][r0 + 16 b + (lane & 15)]      B operand  xc[n0 + 16 w + (lane & 15)][16 t + 4 (lane >> 4) + j]
//   C / D      lane holds columns r0 + 16 b + 4 (lane >> 4) + e, e = 0..3, of row n0 + 16 w + (lane & 15)
// - knn's chain over h.  A lane keeps the running sum of y^2 over its columns (r ascending); the four lanes of a row are joined
// by the butterfly xor 32, 16.
#include "row_chain.h"

namespace {

constexpr int MO_NT = 256;                        // threads (4 waves) of every kernel here
constexpr int MO_WAVES = MO_NT / 64;
constexpr int MO_MAX_BLOCKS = 4096;
constexpr int MO_AUTO_BLOCKS = RR_NUM_CU * 4;
constexpr int MO_TILE = 64;                       // macro tile of the scatter; H is rounded up to it inside the workspace
constexpr int MO_ROWS = 32;                       // rows centred and staged per step
constexpr int MO_CP = 2 * MO_TILE + 16;           // pitch of the staged rows in doubles: 4 rows x 16 lanes x 8 bytes hit 64 banks
constexpr int MO_QL = 16;                         // row lanes of the column sums
constexpr int MO_MAX_CHUNKS = 64;
constexpr int64_t MO_CHUNK_ROWS = 1024;
constexpr size_t MO_SLAB_BUDGET = static_cast<size_t>(256) << 20;

constexpr int CP_ROWS = 64;                       // rows per workgroup
constexpr int CP_KC = 64;                         // columns of x / rows of W staged per chunk
constexpr int CP_RC = 64;                         // columns of W per group
constexpr int CP_SP = CP_KC + 4;                  // pitch of the staged operands (knn.hip: KN_SP)

BlocksKnob g_blocks;

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

inline int mo_hp(int H) { return (H + MO_TILE - 1) / MO_TILE * MO_TILE; }

// the chunk count: a function of N and H only
inline int mo_chunks(int64_t N, int H) {
  const size_t slab = static_cast<size_t>(mo_hp(H)) * mo_hp(H) * sizeof(double);
  int64_t c = (N + MO_CHUNK_ROWS - 1) / MO_CHUNK_ROWS;
  if (c > MO_MAX_CHUNKS) c = MO_MAX_CHUNKS;
  const int64_t fit = static_cast<int64_t>(MO_SLAB_BUDGET / slab);
  if (c > fit) c = fit;
  if (c < 1) c = 1;
  return static_cast<int>(c);
}
inline int64_t mo_chunk_rows(int64_t N, int chunks) { return (N + chunks - 1) / chunks; }

struct MoLayout { size_t flags, cnt, colsum, slabs, total; };
inline MoLayout mo_layout(int64_t N, int H) {
  const int chunks = mo_chunks(N, H);
  const size_t hp = static_cast<size_t>(mo_hp(H));
  MoLayout L;
  size_t o = 0;
  L.flags = o; o += rr_round256(static_cast<size_t>(N));
  L.cnt = o; o += rr_round256(static_cast<size_t>(chunks) * sizeof(long long));
  L.colsum = o; o += rr_round256(static_cast<size_t>(chunks) * hp * sizeof(double));
  L.slabs = o; o += rr_round256(static_cast<size_t>(chunks) * hp * hp * sizeof(double));
  L.total = o;
  return L;
}

template <bool VEC>
__global__ void __launch_bounds__(MO_NT) mo_flag_kernel(const float* x, int64_t ld, int64_t N, int H, uint8_t* flags) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * MO_WAVES;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * MO_WAVES + (threadIdx.x >> 6); r < N; r += stride) {   // (uniform per wave)
    // row_chain.h's kc_row_finite_any(row, lane, H), written out: as a call it changes this kernel's registers (next_free_vgpr
    // 15 -> 16 without VEC, next_free_sgpr 36 -> 32 with it) and measured 2.6 % on the moments of 10^5 x 600
    // (profiles/embedding_shared_ab.txt).  The load and the rule are the shared ones.
    const float* row = x + r * ld;
    bool ok = true;
    for (int g0 = 0; 4 * g0 < H; g0 += 64) {
      const int c = 4 * (g0 + lane);
      if (c < H) {
        const f32x4 v = rr_load4<VEC>(row, c, H);
#pragma unroll
        for (int e = 0; e < 4; ++e) ok = ok && (c + e >= H || rr_finite(v[e]));
      }
    }
    ok = __all(ok);
    if (lane == 0) flags[r] = static_cast<uint8_t>(ok);
  }
}

// grid (hp / 64, chunks): sums[chunk][col] over the chunk's flagged rows, cnt[chunk] = how many there are
template <bool VEC>
__global__ void __launch_bounds__(MO_NT) mo_colsum_kernel(const float* x, int64_t ld, int64_t N, int H, int hp, int64_t rows_per_chunk,
                                                          const uint8_t* flags, double* sums, long long* cnt) {
  __shared__ double part[MO_QL][MO_TILE];
  __shared__ long long pcnt[MO_QL];
  const int tid = threadIdx.x, q = tid >> 4, c4 = (tid & 15) * 4;
  const int col = blockIdx.x * MO_TILE + c4;
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rows_per_chunk;
  const int64_t r1 = r0 + rows_per_chunk < N ? r0 + rows_per_chunk : N;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  long long n = 0;
  for (int64_t r = r0 + q; r < r1; r += MO_QL) {
    const bool on = flags[r] != 0;
    const f32x4 v = rr_load4<VEC>(x + r * ld, col, H);
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = s[e] + ((on && col + e < H) ? static_cast<double>(v[e]) : 0.0);
    n += on ? 1 : 0;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) part[q][c4 + e] = s[e];
  if (c4 == 0) pcnt[q] = n;
  __syncthreads();
  if (tid < MO_TILE) {
    double t = part[0][tid];
#pragma unroll
    for (int k = 1; k < MO_QL; ++k) t = t + part[k][tid];
    sums[static_cast<size_t>(blockIdx.y) * hp + blockIdx.x * MO_TILE + tid] = t;
  }
  if (blockIdx.x == 0 && tid == 0) {
    long long t = 0;
    for (int k = 0; k < MO_QL; ++k) t += pcnt[k];
    cnt[blockIdx.y] = t;
  }
}

__global__ void __launch_bounds__(MO_NT) mo_mean_kernel(const double* sums, const long long* cnt, int chunks, int H, int hp,
                                                        double* mean, long long* n_used) {
  long long n = 0;
  for (int c = 0; c < chunks; ++c) n += cnt[c];
  for (int h = blockIdx.x * MO_NT + threadIdx.x; h < H; h += gridDim.x * MO_NT) {
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s = s + sums[static_cast<size_t>(c) * hp + h];
    mean[h] = n > 0 ? s / static_cast<double>(n) : 0.0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *n_used = n;
}

// grid (macro tiles on or below the diagonal, chunks)
template <bool VEC>
__global__ void __launch_bounds__(MO_NT) mo_scatter_kernel(const float* x, int64_t ld, int64_t N, int H, int hp, int64_t rows_per_chunk,
                                                           const uint8_t* flags, const double* mean, double* slabs) {
  __shared__ __attribute__((aligned(16))) double cs[MO_ROWS * MO_CP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, qd = lane >> 4;
  int ib = 0, jb = static_cast<int>(blockIdx.x);  // macro tile (ib, jb), jb <= ib, rows of the triangle in order
  while (jb > ib) { jb -= ib + 1; ++ib; }
  const int i0 = ib * MO_TILE, j0 = jb * MO_TILE;
  const int wi = wave >> 1, wj = wave & 1;
  bool on[2][2];                                  // (uniform) the 16 x 16 tiles of this wave that lie on or below the diagonal and inside H
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int ti = i0 + 32 * wi + 16 * a, tj = j0 + 32 * wj + 16 * b;
      on[a][b] = tj <= ti && ti < H;
    }
  // staging: thread -> four columns of the 128 staged ones (64 of the i block, then 64 of the j block), rows srow + 8 u
  const int sc = (tid & 31) * 4, srow = tid >> 5;
  const int gcol = sc < MO_TILE ? i0 + sc : j0 + sc - MO_TILE;
  double m4[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) m4[e] = mean[gcol + e < H ? gcol + e : 0];
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rows_per_chunk;
  const int64_t r1 = r0 + rows_per_chunk < N ? r0 + rows_per_chunk : N;
  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f64x4(0.0);
  for (int64_t r = r0; r < r1; r += MO_ROWS) {    // (uniform)
    __syncthreads();                              // the rows staged before these have been read by every wave
#pragma unroll
    for (int u = 0; u < MO_ROWS / 8; ++u) {
      const int64_t row = r + srow + 8 * u;
      const bool ok = row < r1 && flags[row < r1 ? row : r0] != 0;
      const f32x4 v = rr_load4<VEC>(x + (row < r1 ? row : r0) * ld, gcol, H);
      double c[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) c[e] = (ok && gcol + e < H) ? static_cast<double>(v[e]) - m4[e] : 0.0;
      double* dst = cs + (srow + 8 * u) * MO_CP + sc;
      *reinterpret_cast<f64x2*>(dst) = f64x2{c[0], c[1]};
      *reinterpret_cast<f64x2*>(dst + 2) = f64x2{c[2], c[3]};
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < MO_ROWS / 4; ++s) {
      if (r + 4 * s >= r1) break;                 // (uniform) the groups of four past the chunk's end hold zeros only
      const double* rowp = cs + (4 * s + qd) * MO_CP;
      double af[2], bf[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) af[a] = rowp[32 * wi + 16 * a + l15];
#pragma unroll
      for (int b = 0; b < 2; ++b) bf[b] = rowp[MO_TILE + 32 * wj + 16 * b + l15];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
          if (on[a][b]) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[a], bf[b], acc[a][b], 0, 0, 0);
    }
  }
  double* slab = slabs + static_cast<size_t>(blockIdx.y) * hp * hp;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      if (!on[a][b]) continue;
      const int i = i0 + 32 * wi + 16 * a + qd, j = j0 + 32 * wj + 16 * b + l15;   // (i + 12 < hp, j < hp: inside the slab)
#pragma unroll
      for (int e = 0; e < 4; ++e) slab[static_cast<size_t>(i + 4 * e) * hp + j] = acc[a][b][e];
    }
}

__global__ void __launch_bounds__(MO_NT) mo_finish_kernel(const double* slabs, int chunks, int H, int hp, double* scatter) {
  const int64_t total = static_cast<int64_t>(H) * H, stride = static_cast<int64_t>(gridDim.x) * MO_NT;
  const size_t slab = static_cast<size_t>(hp) * hp;
  for (int64_t k = static_cast<int64_t>(blockIdx.x) * MO_NT + threadIdx.x; k < total; k += stride) {
    const int i = static_cast<int>(k / H), j = static_cast<int>(k - static_cast<int64_t>(i) * H);
    if (j > i) continue;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s = s + slabs[c * slab + static_cast<size_t>(i) * hp + j];
    scatter[static_cast<size_t>(i) * H + j] = s;
    scatter[static_cast<size_t>(j) * H + i] = s;
  }
}

struct CpParams {
  const float* x; int64_t ld; int64_t N; int H, R;
  const float* center; const float* W;
  float* y; float* sq;
};

template <bool VEC>
__global__ void __launch_bounds__(MO_NT) cp_kernel(const CpParams P) {
  __shared__ __attribute__((aligned(16))) float xs[CP_ROWS * CP_SP];
  __shared__ __attribute__((aligned(16))) float wt[CP_RC * CP_SP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, qd = lane >> 4;
  const int H = P.H, R = P.R;
  const int xrow = tid >> 4, xc4 = (tid & 15) * 4;                  // staging of x: 16 rows per pass, four passes
  const int wr = tid & 63, wh = tid >> 6;                           // staging of W: column wr of the group, rows wh + 4 u
  const int64_t tiles = (P.N + CP_ROWS - 1) / CP_ROWS;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // (uniform)
    const int64_t n0 = tile * CP_ROWS;
    const int64_t n = n0 + 16 * wave + l15;                         // the row whose results this lane holds
    float sqacc = 0.f;
    for (int r0 = 0; r0 < R; r0 += CP_RC) {
      const int nb = (R - r0 + 15) / 16 < 4 ? (R - r0 + 15) / 16 : 4;   // 16-column tiles of this group that hold anything (uniform)
      f32x4 acc[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[b] = f32x4(0.f);
      for (int h0 = 0; h0 < H; h0 += CP_KC) {
        __syncthreads();                          // the chunk before this one has been read by every wave
        const int c = h0 + xc4;
        float ce[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) ce[e] = P.center != nullptr ? P.center[c + e < H ? c + e : 0] : 0.f;
#pragma unroll
        for (int u = 0; u < CP_ROWS / 16; ++u) {
          const int64_t m = n0 + xrow + 16 * u;
          const bool ok = m < P.N;
          f32x4 v = rr_load4<VEC>(P.x + (ok ? m : 0) * P.ld, c, H);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = (ok && c + e < H) ? v[e] - ce[e] : 0.f;
          *reinterpret_cast<f32x4*>(xs + (xrow + 16 * u) * CP_SP + xc4) = v;
        }
#pragma unroll
        for (int u = 0; u < CP_KC / 4; ++u) {
          const int h = h0 + wh + 4 * u, r = r0 + wr;
          const bool in = h < H && r < R;
          const float w = P.W[in ? static_cast<int64_t>(h) * R + r : 0];
          wt[wr * CP_SP + wh + 4 * u] = in ? w : 0.f;
        }
        __syncthreads();
        const int nt = (H - h0 + 15) / 16;        // k-tiles of this chunk that hold anything (uniform)
#pragma unroll
        for (int t = 0; t < CP_KC / 16; ++t) {
          if (t >= nt) break;
          const f32x4 bf = *reinterpret_cast<const f32x4*>(xs + (16 * wave + l15) * CP_SP + 16 * t + 4 * qd);
          f32x4 af[4];
#pragma unroll
          for (int b = 0; b < 4; ++b) af[b] = *reinterpret_cast<const f32x4*>(wt + (16 * b + l15) * CP_SP + 16 * t + 4 * qd);
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int b = 0; b < 4; ++b)
              if (b < nb) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[b][j], bf[j], acc[b], 0, 0, 0);
        }
      }
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = r0 + 16 * b + 4 * qd + e;
          if (r < R) {
            const float v = acc[b][e];
            if (P.y != nullptr && n < P.N) P.y[n * R + r] = v;
            sqacc = sqacc + v * v;
          }
        }
    }
    sqacc = sqacc + __shfl_xor(sqacc, 32, 64);
    sqacc = sqacc + __shfl_xor(sqacc, 16, 64);
    if (P.sq != nullptr && qd == 0 && n < P.N) P.sq[n] = sqacc;
  }
}

// workgroups of a grid-strided launch over `items` workgroups' worth of work
inline int mo_grid(int64_t items) {
  int64_t b = g_blocks.get();
  if (b == 0) b = items < MO_AUTO_BLOCKS ? items : MO_AUTO_BLOCKS;
  if (b < 1) b = 1;
  return static_cast<int>(b);
}

}  // namespace

extern "C" {

int rr_moments_blocks(void) { return g_blocks.get(); }
int rr_moments_set_blocks(int blocks) { return g_blocks.set(blocks, MO_MAX_BLOCKS); }

int rr_moments_chunks(int64_t N, int H) {
  if (N < 0 || H < 1 || H > RR_MOMENTS_MAX_H) return 0;
  return mo_chunks(N, H);
}

int rr_moments_workspace_bytes(int64_t N, int H, size_t* bytes) {
  RR_CHECK_ARG(bytes && N >= 0 && H >= 1);
  if (H > RR_MOMENTS_MAX_H || N > 0x7fffffffLL) return RR_ERR_UNSUPPORTED;
  *bytes = mo_layout(N, H).total;
  return RR_OK;
}

int rr_col_moments_f64(const float* x, int64_t ld, int64_t N, int H, double* mean, double* scatter, int64_t* n_used,
                       void* workspace, size_t workspace_bytes, rr_stream_t stream) {
  RR_CHECK_ARG(x && mean && scatter && n_used && workspace);
  RR_CHECK_ARG(N >= 0 && H >= 1 && ld >= H);
  if (H > RR_MOMENTS_MAX_H || N > 0x7fffffffLL) return RR_ERR_UNSUPPORTED;
  const MoLayout L = mo_layout(N, H);
  if (workspace_bytes < L.total) return RR_ERR_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  uint8_t* flags = reinterpret_cast<uint8_t*>(ws + L.flags);
  long long* cnt = reinterpret_cast<long long*>(ws + L.cnt);
  double* sums = reinterpret_cast<double*>(ws + L.colsum);
  double* slabs = reinterpret_cast<double*>(ws + L.slabs);
  const int chunks = mo_chunks(N, H), hp = mo_hp(H), T = hp / MO_TILE;
  const int64_t rpc = mo_chunk_rows(N, chunks);
  const bool vec = rr_vec4_ok(x, ld);
  int st;
  if (N > 0) {
    const int grid = mo_grid((N + MO_WAVES - 1) / MO_WAVES);
    rr_vec_dispatch(vec, [&](auto v) { mo_flag_kernel<decltype(v)::value><<<grid, MO_NT, 0, s>>>(x, ld, N, H, flags); });
    if ((st = rr_launch_status()) != RR_OK) return st;
  }
  const dim3 gsum(static_cast<unsigned>(T), static_cast<unsigned>(chunks));
  rr_vec_dispatch(vec, [&](auto v) { mo_colsum_kernel<decltype(v)::value><<<gsum, MO_NT, 0, s>>>(x, ld, N, H, hp, rpc, flags, sums, cnt); });
  if ((st = rr_launch_status()) != RR_OK) return st;
  mo_mean_kernel<<<mo_grid((H + MO_NT - 1) / MO_NT), MO_NT, 0, s>>>(sums, cnt, chunks, H, hp, mean, reinterpret_cast<long long*>(n_used));
  if ((st = rr_launch_status()) != RR_OK) return st;
  const dim3 gsc(static_cast<unsigned>(T * (T + 1) / 2), static_cast<unsigned>(chunks));
  rr_vec_dispatch(vec, [&](auto v) { mo_scatter_kernel<decltype(v)::value><<<gsc, MO_NT, 0, s>>>(x, ld, N, H, hp, rpc, flags, mean, slabs); });
  if ((st = rr_launch_status()) != RR_OK) return st;
  mo_finish_kernel<<<mo_grid((static_cast<int64_t>(H) * H + MO_NT - 1) / MO_NT), MO_NT, 0, s>>>(slabs, chunks, H, hp, scatter);
  return rr_launch_status();
}

int rr_center_project_f32(const float* x, int64_t ld, int64_t N, int H, const float* center, const float* W, int R, float* y,
                          float* sq, rr_stream_t stream) {
  RR_CHECK_ARG(x && W && (y || sq));
  RR_CHECK_ARG(N >= 0 && H >= 1 && ld >= H && R >= 1 && R <= H);
  if (N > 0x7fffffffLL) return RR_ERR_UNSUPPORTED;
  if (N == 0) return RR_OK;
  CpParams P;
  P.x = x; P.ld = ld; P.N = N; P.H = H; P.R = R;
  P.center = center; P.W = W; P.y = y; P.sq = sq;
  const int grid = mo_grid((N + CP_ROWS - 1) / CP_ROWS);
  hipStream_t s = static_cast<hipStream_t>(stream);
  rr_vec_dispatch(rr_vec4_ok(x, ld), [&](auto v) { cp_kernel<decltype(v)::value><<<grid, MO_NT, 0, s>>>(P); });
  return rr_launch_status();
}

}  // extern "C"
