// Weight gradients of the dense layers (rr_linear_wgrad_f32): dW = dZ^T * [X1|X2], dbias = colsum(dZ), split over M-chunks
// into partial slabs and finished by a fixed-order reduction.  wgrad_kernel is the scalar-load form, wgrad_fast_kernel the
// exact-f32 matrix core, wgrad_split_kernel the bf16 / f16 matrix core through operand term splits (linear_common.h).
#include "linear_common.h"

namespace {

// ======================================================================== weight gradient
constexpr int WT = 5;               // 5x5 MFMA tiles (80 x 80) per wave
constexpr int WBN = 160;            // workgroup output tile: 160 (n) x 160 (k), 2x2 waves
constexpr int WLD = 176;            // LDS row stride (== 16 mod 32 -> ds_read_b32 conflict-free)
constexpr int WMT = 16;             // rows of M per staged tile

struct WgradParams {
  rr_wgrad_args a;
  int k1p;              // segment-2 start column in the extended X (k1 rounded up to 4)
  int kext;             // k1p + k2 + 1 (last column = ones -> dbias)
  int nblk_n, nblk_k;   // output tiles
  int64_t rows_per_chunk;
  int nchunks;
  int flags;            // F_A1_VEC (x1), F_A2_VEC (x2), F_SUB_VEC, F_MASK_VEC (mask), F_EPI_VEC (dy)
  int64_t slab;         // floats per partial slab = N*(k1+k2) + N
};

// The work of a workgroup: output tile (nb, kb) of one M-chunk, rows [mbeg, mend).
// XCD-aware mapping: workgroups are dealt round-robin over the 8 XCDs (id % 8 share an L2), so the
// nblk_n * nblk_k output tiles of ONE M-chunk get consecutive slots of one XCD: the second reader
// of every dZ / X row hits that XCD's L2 instead of HBM (speed only; any placement is correct).
// Two calls: the caller returns in between when chunk >= P.nchunks (a padding workgroup of the grid); with that early return
// inside one function the kernels lose the known bits of nb / kb and come out with other registers.
struct WgradWork { int nb, kb; int64_t mbeg, mend; };
__device__ __forceinline__ int wgrad_chunk(const WgradParams& P) {
  const int nt = P.nblk_n * P.nblk_k;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  return (slot / nt) * 8 + xcd;
}
template <int KB>                     // columns per k-block
__device__ __forceinline__ WgradWork wgrad_work(const WgradParams& P, int chunk) {
  WgradWork w;
  const int nt = P.nblk_n * P.nblk_k;
  const int tile = static_cast<int>(blockIdx.x >> 3) % nt;
  const int bn = tile / P.nblk_k, bk = tile % P.nblk_k;
  w.nb = bn * WBN;
  w.kb = bk * KB;
  w.mbeg = static_cast<int64_t>(chunk) * P.rows_per_chunk;
  w.mend = w.mbeg + P.rows_per_chunk;
  if (w.mend > P.a.M) w.mend = P.a.M;
  return w;
}

// The extended X of one row, written once: [ x1 (k1 columns, then dead pad columns up to k1p) | x2 (k2) | ones ], kext
// columns.  wgrad_x_chunk is the 16-byte chunk that starts at extended column kx (kx % 4 == 0); wgrad_x_column is the
// inverse for one column.  All three loaders and the slab store take the layout from these two.
enum : int { X_NONE = 0, X_SEG1 = 1, X_SEG2 = 2, X_ONES = 3 };
struct WgradXChunk {
  int kind;             // X_NONE: dead pad columns or past kext, the chunk reads as zero
  int col;              // first column inside the segment's source (x1 / x1_sub, or x2)
  int nv;               // leading elements that come from the source; the others are zero ...
  int one;              // ... except this one, the ones column (bias gradient); -1: not in this chunk
};
__device__ __forceinline__ WgradXChunk wgrad_x_chunk(const WgradParams& P, int kx) {
  const rr_wgrad_args& a = P.a;
  WgradXChunk c = {X_NONE, 0, 4, -1};
  if (kx < a.k1) {
    c.kind = X_SEG1; c.col = kx; c.nv = min(4, a.k1 - kx);
  } else if (kx >= P.k1p && kx < P.kext) {
    const int c2 = kx - P.k1p;
    if (c2 < a.k2) {
      c.kind = X_SEG2; c.col = c2; c.nv = min(4, a.k2 - c2);
      if (a.k2 - c2 < 4) c.one = a.k2 - c2;             // the ones column shares this chunk (k2 % 4 != 0)
    } else {
      c.kind = X_ONES; c.nv = 0; c.one = 0;             // c2 == k2 (k2 % 4 == 0): the chunk is {1, 0, 0, 0}
    }
  }
  return c;
}
// column of dw that extended column kx lands in; -1: dead pad column (or past kext), -2: the ones column (dbias)
__device__ __forceinline__ int wgrad_x_column(const WgradParams& P, int kx) {
  const rr_wgrad_args& a = P.a;
  int col = -1;
  if (kx < a.k1) col = kx;
  else if (kx >= P.k1p && kx < P.k1p + a.k2) col = a.k1 + (kx - P.k1p);
  else if (kx == P.k1p + a.k2) col = -2;
  return col;
}

// Row m of a direct operand, or row j = idx[m] of a gathered one; a negative index is "no row" (nullptr: reads as zero).
__device__ __forceinline__ const float* wgrad_row(const float* base, int64_t ld, int64_t m, bool gathered, int32_t j) {
  if (!gathered) return base + m * ld;
  return j >= 0 ? base + static_cast<int64_t>(j) * ld : nullptr;
}

// A partial chunk of the extended X, element by element: the first nv elements are x (- the subtract source), the ones
// element is 1 in a row inside the M-chunk, everything else 0.
template <bool HAS_SUB>
__device__ __forceinline__ f32x4 wgrad_patch_x(f32x4 xv, f32x4 xs, int nv, int one, bool row_ok) {
  f32x4 x;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float u = e < nv ? xv[e] : 0.f;
    if (HAS_SUB) u -= e < nv ? xs[e] : 0.f;
    if (e == one) u = row_ok ? 1.0f : 0.f;
    x[e] = u;
  }
  return x;
}

template <int NJ>
__device__ __forceinline__ void wgrad_zero_acc(f32x4 (&acc)[WT][NJ]) {
#pragma unroll
  for (int i = 0; i < WT; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4(0.f);
}

// A wave's WT x NJ accumulator tiles into the partial slab [chunk][ N*K (dw, row-major) | N (dbias) ]; (nb + wn, kb + wk) is the
// wave's corner in (n, extended k).  D[i = n][j = k]: lane -> n = .. + fq*4 + e, k = .. + fr
template <int NJ>
__device__ __forceinline__ void wgrad_store_slab(const WgradParams& P, int chunk, int nb, int kb, int wn, int wk, int fr, int fq,
                                                 const f32x4 (&acc)[WT][NJ]) {
  const rr_wgrad_args& a = P.a;
  const int K = a.k1 + a.k2;
  float* slab = static_cast<float*>(a.workspace) + static_cast<int64_t>(chunk) * P.slab;
#pragma unroll
  for (int i = 0; i < WT; ++i) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int kreal = wgrad_x_column(P, kb + wk + j * 16 + fr);
      if (kreal == -1) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = nb + wn + i * 16 + fq * 4 + e;
        if (n >= a.N) continue;
        if (kreal >= 0) slab[static_cast<int64_t>(n) * K + kreal] = acc[i][j][e];
        else slab[static_cast<int64_t>(a.N) * K + n] = acc[i][j][e];
      }
    }
  }
}

__global__ void __launch_bounds__(THREADS) wgrad_kernel(const WgradParams P) {
  __shared__ __attribute__((aligned(16))) float lds[2][2 * WMT * WLD];
  const rr_wgrad_args& a = P.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk = wgrad_chunk(P);
  if (chunk >= P.nchunks) return;
  const WgradWork w = wgrad_work<WBN>(P, chunk);
  const int nb = w.nb, kb = w.kb;
  const int64_t mbeg = w.mbeg, mend = w.mend;
  const int flags = P.flags;

  // staging: 2 tiles x 16 rows x 40 float4 = 1280 chunks, 5 per thread
  auto load_chunk_z = [&](int64_t mrow, int col) -> f32x4 {       // dZ[mrow][nb+col .. +3]
    f32x4 v = f32x4(0.f);
    const int n = nb + col;
    if (mrow >= mend || n >= a.N) return v;
    v = load_chunk(a.dy + mrow * a.ld_dy, n, a.N, flags & F_EPI_VEC);
    if (a.mask) v = apply_mask(v, load_chunk(a.mask + mrow * a.ld_mask, n, a.N, flags & F_MASK_VEC), a.mask_scale);
    return v;
  };
  auto load_chunk_x = [&](int64_t mrow, int col) -> f32x4 {       // X_ext[mrow][kb+col .. +3]
    f32x4 v = f32x4(0.f);
    const WgradXChunk c = wgrad_x_chunk(P, kb + col);
    if (mrow >= mend || c.kind == X_NONE) return v;
    if (c.kind == X_SEG1) {
      const float* p = wgrad_row(a.x1, a.ldx1, mrow, a.x1_idx != nullptr, a.x1_idx ? a.x1_idx[mrow] : 0);
      v = load_chunk(p, c.col, a.k1, flags & F_A1_VEC);
      if (a.x1_sub) {
        const float* sp = wgrad_row(a.x1_sub, a.ldx1_sub, mrow, a.x1_sub_idx != nullptr, a.x1_sub_idx ? a.x1_sub_idx[mrow] : 0);
        v = v - load_chunk(sp, c.col, a.k1, flags & F_SUB_VEC);
      }
    } else if (c.kind == X_SEG2) {
      v = load_chunk(a.x2 + mrow * a.ldx2, c.col, a.k2, flags & F_A2_VEC);
    }
    if (c.one >= 0) v[c.one] = 1.0f;             // the ones column (bias gradient) sits right after segment 2
    return v;
  };
  constexpr int CH = 5;
  auto load_tiles = [&](int64_t mt, f32x4 (&r)[CH]) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int f = i * THREADS + tid;           // 0 .. 1279
      const int which = f >= 640 ? 1 : 0;
      const int g = f - which * 640;
      const int row = g / 40, col = (g - row * 40) * 4;
      r[i] = which ? load_chunk_x(mt + row, col) : load_chunk_z(mt + row, col);
    }
  };
  auto store_tiles = [&](int buf, const f32x4 (&r)[CH]) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int f = i * THREADS + tid;
      const int which = f >= 640 ? 1 : 0;
      const int g = f - which * 640;
      const int row = g / 40, col = (g - row * 40) * 4;
      *reinterpret_cast<f32x4*>(&lds[buf][which * WMT * WLD + row * WLD + col]) = r[i];
    }
  };

  f32x4 acc[WT][WT];
  wgrad_zero_acc(acc);

  const int wn = (wave >> 1) * (WT * 16), wk = (wave & 1) * (WT * 16);   // wave's corner inside the 160x160 tile
  const int fr = lane & 15, fq = lane >> 4;

  f32x4 r[CH];
  const int64_t ntiles = (mend > mbeg) ? (mend - mbeg + WMT - 1) / WMT : 0;
  if (ntiles > 0) {
    load_tiles(mbeg, r);
    store_tiles(0, r);
  }
  __syncthreads();
  for (int64_t t = 0; t < ntiles; ++t) {
    const int cur = static_cast<int>(t & 1);
    const bool more = t + 1 < ntiles;
    if (more) load_tiles(mbeg + (t + 1) * WMT, r);
    const float* Zs = lds[cur];
    const float* Xs = lds[cur] + WMT * WLD;
#pragma unroll
    for (int kk = 0; kk < WMT / 4; ++kk) {
      float zf[WT], xf[WT];
      const int row = kk * 4 + fq;
#pragma unroll
      for (int i = 0; i < WT; ++i) {
        zf[i] = Zs[row * WLD + wn + i * 16 + fr];
        xf[i] = Xs[row * WLD + wk + i * 16 + fr];
      }
#pragma unroll
      for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(zf[i], xf[j], acc[i][j], 0, 0, 0);
    }
    if (more) store_tiles(cur ^ 1, r);
    __syncthreads();
  }

  wgrad_store_slab(P, chunk, nb, kb, wn, wk, fr, fq, acc);
}

// ------------------------------------------------------------------------ wgrad fast path
// Hot case: every operand 16-byte addressable, N % 4 == 0.  A 16-row tile is 640 dZ chunks +
// 16 * (k-block width / 4) X chunks of 16 bytes; thread t owns dZ chunks {t, t+256, t+512 (t<128)}
// and up to three X chunks, so every slot's role is known before the loop.
//
// The loop is VALU-bound if the loader is written naively (per-tile 64-bit address products,
// per-element bounds selects: ~500 VALU + ~300 SALU instructions per tile against 100 MFMAs, measured
// 61 % matrix-pipe duty).  So all per-tile work that can be hoisted is hoisted:
//  * every streamed operand is a per-slot POINTER that advances by 16 rows per tile (one 64-bit add);
//  * a slot that must read as zero (column block tail, k-block tail, unused slot) points at a zero
//    chunk with stride 0 — no validity select in the loop; the ones column (bias gradient) is a
//    constant {1,0,0,0} chunk when it starts a chunk (k2 % 4 == 0);
//  * gathered rows cost one v_mad_u64_u32 (index x row pitch + column pointer) and one select
//    (index < 0 -> zero chunk); indices are fetched one tile ahead from an advancing pointer;
//  * rows past the end of the M-chunk exist only in its last tile, which takes a separate
//    instantiation of the issue code (selects to the zero chunk); the steady state has none;
//  * partial 16-byte chunks (k1 % 4 or k2 % 4 != 0) are patched per element only under a uniform flag.
// What remains per tile: the loads, the pointer bumps, the ReLU-mask select and the subtraction.
__device__ __attribute__((aligned(16))) const float rr_one_chunk[4] = {1.f, 0.f, 0.f, 0.f};

#ifdef RR_TRACE_LOOP                  // per-tile stamps of wgrad_fast_kernel's loop (t: the tile), next to its RR_STAMPs
#define RR_LSTAMP(q)                                                                                      \
    do {                                                                                                   \
      if (rr_trace_buf && (threadIdx.x & 63) == 0 && blockIdx.x < 2 && t < 48)                             \
        rr_trace_buf[4096 * 8 + ((blockIdx.x * 4 + (threadIdx.x >> 6)) * 48 + t) * 8 + (q)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#else
#define RR_LSTAMP(q)
#endif

template <bool HAS_MASK, bool HAS_SUB, int WTK>
__global__ void __launch_bounds__(THREADS, 2) wgrad_fast_kernel(const WgradParams P) {
  constexpr int KB = 32 * WTK;                          // columns per k-block (160 / 128 / 96)
  constexpr int XC = KB / 4;                            // 16-byte X chunks per row
  constexpr int S = 3;                                  // slots per operand per thread
  __shared__ __attribute__((aligned(16))) float lds[2][2 * WMT * WLD + 4];   // + one dump chunk for unused staging slots
  const rr_wgrad_args& a = P.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk = wgrad_chunk(P);
  if (chunk >= P.nchunks) return;
  RR_STAMP(0);
  const WgradWork w = wgrad_work<KB>(P, chunk);
  const int nb = w.nb, kb = w.kb;
  const int64_t mbeg = w.mbeg, mend = w.mend;
  const int nrows = static_cast<int>(mend - mbeg);      // rows of this M-chunk (> 0: chunk < nchunks)
  const int ntiles = (nrows + WMT - 1) / WMT;
  const float* const zero = rr_zero_chunk;
  const bool partial = (a.k1 & 3) != 0 || (a.k2 & 3) != 0;

  // ---- slot roles (loop invariant)
  int zrow[S], zoff[S], xrow[S], xoff[S], nval[S], onee[S];
  const float* pz[S];                                   // dZ chunk of this slot in the current tile (advances)
  const float* pm[S];                                   // ReLU-mask chunk
  const float* px[S];                                   // X chunk (direct) or column pointer into row 0 (gather)
  const float* ps[S];                                   // subtract source, same two forms
  const int32_t* pi[S];                                 // gather index of the slot's row, one tile ahead
  const int32_t* pj[S];
  int gi[S], gj[S];                                     // -1 for gathered slots (index offset mask), 0 otherwise
  uint32_t zstep[S], mstep[S], xstep[S], sstep[S];      // bytes per tile (0 for constant chunks); 16 rows * pitch < 4 GiB
  bool sgather[S];
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const int g = tid + i * THREADS;
    // dZ
    const bool zuse = g < WMT * 40;
    zrow[i] = zuse ? g / 40 : 0;
    const int zcol = zuse ? (g - zrow[i] * 40) * 4 : 0;
    zoff[i] = (zuse ? zrow[i] * WLD + zcol : 2 * WMT * WLD) / 4;      // in 16-byte units: the store is a ds_write_b128
    const bool zok = zuse && (nb + zcol < a.N);
    pz[i] = zok ? a.dy + (mbeg + zrow[i]) * a.ld_dy + nb + zcol : zero;
    zstep[i] = zok ? static_cast<uint32_t>(WMT * 4 * a.ld_dy) : 0u;
    pm[i] = zero;
    mstep[i] = 0;
    if (HAS_MASK && zok) {
      pm[i] = a.mask + (mbeg + zrow[i]) * a.ld_mask + nb + zcol;
      mstep[i] = static_cast<uint32_t>(WMT * 4 * a.ld_mask);
    }
    // X
    const bool xuse = g < WMT * XC;
    xrow[i] = xuse ? g / XC : 0;
    const int xc0 = xuse ? (g - xrow[i] * XC) * 4 : 0;
    xoff[i] = (xuse ? WMT * WLD + xrow[i] * WLD + xc0 : 2 * WMT * WLD) / 4;
    const WgradXChunk c = wgrad_x_chunk(P, kb + xc0);   // the slot's chunk of the extended X
    const int kind = xuse ? c.kind : X_NONE;
    px[i] = zero; ps[i] = zero; xstep[i] = 0; sstep[i] = 0; sgather[i] = false;
    pi[i] = reinterpret_cast<const int32_t*>(rr_zero_chunk); pj[i] = pi[i];   // non-gather slots read index 0
    gi[i] = 0; gj[i] = 0;
    nval[i] = xuse ? c.nv : 4; onee[i] = xuse ? c.one : -1;
    if (kind == X_SEG1) {
      if (a.x1_idx) {
        px[i] = a.x1 + c.col;
        pi[i] = a.x1_idx + mbeg + xrow[i];
        gi[i] = -1;
      } else {
        px[i] = a.x1 + (mbeg + xrow[i]) * a.ldx1 + c.col;
        xstep[i] = static_cast<uint32_t>(WMT * 4 * a.ldx1);
      }
      if (HAS_SUB) {
        if (a.x1_sub_idx) {
          sgather[i] = true;
          ps[i] = a.x1_sub + c.col;
          pj[i] = a.x1_sub_idx + mbeg + xrow[i];
          gj[i] = -1;
        } else {
          ps[i] = a.x1_sub + (mbeg + xrow[i]) * a.ldx1_sub + c.col;
          sstep[i] = static_cast<uint32_t>(WMT * 4 * a.ldx1_sub);
        }
      }
    } else if (kind == X_SEG2) {
      px[i] = a.x2 + (mbeg + xrow[i]) * a.ldx2 + c.col;
      xstep[i] = static_cast<uint32_t>(WMT * 4 * a.ldx2);
    } else if (kind == X_ONES) {
      px[i] = rr_one_chunk;
    }
  }

  f32x4 zv[S], zm[S], xv[S], xs[S];
  bool xrv[S];                                          // the X slot's row is inside the M-chunk (latched at issue)
  int32_t ia[S], is[S];
#pragma unroll
  for (int i = 0; i < S; ++i) { ia[i] = 0; is[i] = 0; xrv[i] = true; }

  // indices for the tile whose first row is `r0` (relative to mbeg); rows past the chunk read the last row's index
  auto fetch_idx = [&](int r0) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < S; ++i) {
      const int over = r0 + xrow[i] - (nrows - 1);      // > 0: past the end -> step back to the last row
      const int off = r0 - (over > 0 ? over : 0);
      ia[i] = ldgi(pi[i] + (off & gi[i]));              // direct slots always read index 0 (>= 0, adds 0 rows)
      if (HAS_SUB) is[i] = ldgi(pj[i] + (off & gj[i]));
    }
  };
  // rows_left < 16 only in the last tile of the M-chunk: those rows read the zero chunk.  No branches: every
  // load is issued, the pointer is what gets selected (a load under a per-lane branch makes hipcc wait at the join)
  auto issue = [&](int rows_left) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < S; ++i) {
      const bool zr = zrow[i] < rows_left;
      zv[i] = ldg4(zr ? pz[i] : zero);
      if (HAS_MASK) zm[i] = ldg4(zr ? pm[i] : zero);
      pz[i] = reinterpret_cast<const float*>(reinterpret_cast<const char*>(pz[i]) + zstep[i]);
      if (HAS_MASK) pm[i] = reinterpret_cast<const float*>(reinterpret_cast<const char*>(pm[i]) + mstep[i]);
      const bool xr = xrow[i] < rows_left;
      xrv[i] = xr;
      const float* p = px[i] + static_cast<uint64_t>(static_cast<uint32_t>(ia[i])) * static_cast<uint32_t>(a.ldx1);
      xv[i] = ldg4((xr && ia[i] >= 0) ? p : zero);
      px[i] = reinterpret_cast<const float*>(reinterpret_cast<const char*>(px[i]) + xstep[i]);
      if (HAS_SUB) {
        const float* q = ps[i] + static_cast<uint64_t>(static_cast<uint32_t>(is[i])) * static_cast<uint32_t>(a.ldx1_sub);
        xs[i] = ldg4((xr && is[i] >= 0) ? q : zero);
        ps[i] = reinterpret_cast<const float*>(reinterpret_cast<const char*>(ps[i]) + sstep[i]);
      }
    }
  };
  auto commit = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < S; ++i) {
      reinterpret_cast<f32x4*>(lds[buf])[zoff[i]] = HAS_MASK ? apply_mask(zv[i], zm[i], a.mask_scale) : zv[i];
      f32x4 x = xv[i];
      if (HAS_SUB) x = xv[i] - xs[i];
      // k1 % 4 or k2 % 4 != 0: patch the chunk per element
      if (partial) x = wgrad_patch_x<HAS_SUB>(xv[i], HAS_SUB ? xs[i] : xv[i], nval[i], onee[i], xrv[i]);
      reinterpret_cast<f32x4*>(lds[buf])[xoff[i]] = x;
    }
  };

  f32x4 acc[WT][WTK];
  wgrad_zero_acc(acc);

  const int wn = (wave >> 1) * (WT * 16), wk = (wave & 1) * (WTK * 16);
  const int fr = lane & 15, fq = lane >> 4;
  // tile 0
  fetch_idx(0);
  issue(nrows);
  fetch_idx(WMT);
  commit(0);
  __syncthreads();
  RR_STAMP(1);
  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    const bool more = t + 1 < ntiles;
    RR_LSTAMP(0);
    if (more) {
      const int left = nrows - (t + 1) * WMT;           // rows of tile t+1 (uses the indices fetched one tile ago)
      issue(left);
      fetch_idx((t + 2) * WMT);
    }
    RR_LSTAMP(1);
    const float* Zs = lds[cur];
    const float* Xs = lds[cur] + WMT * WLD;
#pragma unroll
    for (int kk = 0; kk < WMT / 4; ++kk) {
      float zf[WT], xf[WTK];
      const int row = kk * 4 + fq;
#pragma unroll
      for (int i = 0; i < WT; ++i) zf[i] = Zs[row * WLD + wn + i * 16 + fr];
#pragma unroll
      for (int j = 0; j < WTK; ++j) xf[j] = Xs[row * WLD + wk + j * 16 + fr];
#pragma unroll
      for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WTK; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(zf[i], xf[j], acc[i][j], 0, 0, 0);
    }
    RR_LSTAMP(2);
#ifdef RR_TRACE_LOOP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    RR_LSTAMP(3);
#endif
    if (more) commit(cur ^ 1);
    RR_LSTAMP(4);
    __syncthreads();
    RR_LSTAMP(5);
  }

  RR_STAMP(2);
  wgrad_store_slab(P, chunk, nb, kb, wn, wk, fr, fq, acc);
#ifdef RR_TRACE
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  RR_STAMP(3);
#endif
}

// ------------------------------------------------------------------------ weight gradient, split path
// dW = dZ^T X on the bf16 matrix core with the three-term operand split of linear_split_kernel: here BOTH operands are
// activations, so each staged element is split once per workgroup when it is written to LDS (row-major bf16 term
// images [term][32 rows of M][columns]), and the MFMA operands - 8 consecutive rows of M for one column - come out of
// ds_read_b64_tr_b16, the transposing LDS read (a 16-lane group reads 4 rows x 16 columns and each lane receives one
// column).  Output tile, M-chunking, slab layout and the fixed-order reduction are those of wgrad_fast_kernel.
// Loader: thread t owns row t/8 of the 32-row tile and the 16-byte chunks (t%8) + 8 i of that row: one row pointer
// per operand, one gather index per tile.  One LDS stage of 60 KB (two workgroups per CU overlap each other's
// staging with MFMA); image rows are 64 (mod 128) bytes apart so the 8-byte term stores are conflict-free, and the
// 32-byte column blocks of rows 8-15 / 24-31 are swapped pairwise (XOR 32) so that the two row quads a 32-lane half
// reads in one transposed read (rows r..r+3 and r+8..r+11) fall on different banks.
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4* rr_lds_s16x4;

__device__ __forceinline__ u32x4 tr_read8(const unsigned char* p, int rowbytes) {     // rows r..r+3 and r+4..r+7
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((rr_lds_s16x4)(p));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((rr_lds_s16x4)(p + 4 * rowbytes));
  u32x4 r;
  r.x = __builtin_bit_cast(uint2, lo).x; r.y = __builtin_bit_cast(uint2, lo).y;
  r.z = __builtin_bit_cast(uint2, hi).x; r.w = __builtin_bit_cast(uint2, hi).y;
  return r;
}

// c += z * x over the term images of one 16x16 tile and 32 rows of M (z[0] / x[0]: the leading terms), smallest terms first:
// the six products of three bf16 terms, or the three of two f16 terms
template <bool F16>
__device__ __forceinline__ f32x4 mfma_terms(const u32x4 (&z)[F16 ? 2 : 3], const u32x4 (&x)[F16 ? 2 : 3], f32x4 c) {
  if constexpr (F16) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(as_f16x8(z[1]), as_f16x8(x[0]), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(as_f16x8(z[0]), as_f16x8(x[1]), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(as_f16x8(z[0]), as_f16x8(x[0]), c, 0, 0, 0);
  } else {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(z[2]), as_bf16x8(x[0]), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(z[1]), as_bf16x8(x[1]), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(z[0]), as_bf16x8(x[2]), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(z[1]), as_bf16x8(x[0]), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(z[0]), as_bf16x8(x[1]), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(z[0]), as_bf16x8(x[0]), c, 0, 0, 0);
  }
  return c;
}

constexpr int SMT = 32;             // rows of M per staged tile on the split path

template <bool HAS_MASK, bool HAS_SUB, int WTK, bool F16 = false>
__global__ void __launch_bounds__(THREADS, 2) wgrad_split_kernel(const WgradParams P) {
  constexpr int KB = 32 * WTK;                          // columns per k-block (160 / 128 / 96)
  constexpr int ZRB = 320;                              // bytes per row of a dZ term image (160 bf16)
  constexpr int XRB = WTK == 3 ? 192 : 320;             // X term image (WTK 4: 256 bytes of data + 64 of pad)
  constexpr int ZIMG = SMT * ZRB, XIMG = SMT * XRB;
  constexpr int TERMS = F16 ? 2 : 3;                    // three bf16 terms, or two f16 terms of the scaled operands (rr_wgrad_args.split = 2)
  __shared__ __attribute__((aligned(16))) unsigned char lds[TERMS * ZIMG + TERMS * XIMG];
  const rr_wgrad_args& a = P.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float zs = 1.f, xsc = 1.f, izs = 1.f, ixs = 1.f;     // F16: operand scales from the caller's bounds (uniform) and their inverses
  if (F16) {
    const float bz = (a.dy_amax ? rr_amax_read(a.dy_amax) : 0.f) * (HAS_MASK ? fabsf(a.mask_scale) : 1.f);
    const int ez = rr_f16_exp(bz);
    const float bx = fmaxf((a.x1_amax ? rr_amax_read(a.x1_amax) : 0.f) + (a.x1_sub_amax ? rr_amax_read(a.x1_sub_amax) : 0.f),
                           a.x2_amax ? rr_amax_read(a.x2_amax) : 0.f);
    const int ex = rr_f16_exp(fmaxf(bx, 1.0f));         // (the ones column of the extended X)
    zs = rr_pow2(14 - ez); izs = rr_pow2(ez - 14);
    xsc = rr_pow2(14 - ex); ixs = rr_pow2(ex - 14);
    if (!(bz < 2.5e33f)) zs = __builtin_nanf("");       // an infinite / > 2^110 element: no scale fits, the gradient is NaN
    if (!(bx < 2.5e33f)) xsc = __builtin_nanf("");
  }
  const int chunk = wgrad_chunk(P);
  if (chunk >= P.nchunks) return;
  const WgradWork w = wgrad_work<KB>(P, chunk);
  const int nb = w.nb, kb = w.kb;
  const int64_t mbeg = w.mbeg, mend = w.mend;
  const int nrows = static_cast<int>(mend - mbeg);
  const int ntiles = (nrows + SMT - 1) / SMT;
  const float* const zero = rr_zero_chunk;

  // ---- loader role: row r of the tile, chunks g + 8 i
  const int r = tid >> 3, g = tid & 7;
  const int xr = ((r >> 3) & 1) << 5;                   // column-block swap of this row in the images
  bool zok[5];
  int xcode[WTK];                                       // per chunk: column | kind << 16 | valid elements << 18 | (ones element + 1) << 21
  bool partial = false;
#pragma unroll
  for (int i = 0; i < 5; ++i) zok[i] = nb + 4 * (g + 8 * i) < a.N;
#pragma unroll
  for (int i = 0; i < WTK; ++i) {
    const WgradXChunk c = wgrad_x_chunk(P, kb + 4 * (g + 8 * i));
    if (c.nv != 4 || c.one >= 0) partial = true;
    xcode[i] = c.col | (c.kind << 16) | (c.nv << 18) | ((c.one + 1) << 21);
  }
  partial = __any(partial);

  f32x4 zv[5], zm[5], xv[WTK], xs[WTK];
  bool m_ok = false;                                    // this thread's row of the tile in flight is inside the M-chunk
  int32_t ia = 0, is = 0;                               // gather indices of the NEXT tile's row
  auto fetch_idx = [&](int t) {                         // rows past the chunk read the last row's index (never used)
    int rr = t * SMT + r;
    if (rr > nrows - 1) rr = nrows - 1;
    ia = a.x1_idx ? ldgi(a.x1_idx + mbeg + rr) : 0;
    if (HAS_SUB) is = a.x1_sub_idx ? ldgi(a.x1_sub_idx + mbeg + rr) : 0;
  };
  auto issue = [&](int t) {                             // every load is issued; the address is what gets selected
    const int rr = t * SMT + r;
    m_ok = rr < nrows;
    const int64_t m = mbeg + (m_ok ? rr : 0);
    const float* zp = a.dy + m * a.ld_dy + nb + 4 * g;
    const float* mp = HAS_MASK ? a.mask + m * a.ld_mask + nb + 4 * g : zero;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      zv[i] = ldg4((m_ok && zok[i]) ? zp + 32 * i : zero);
      if (HAS_MASK) zm[i] = ldg4((m_ok && zok[i]) ? mp + 32 * i : zero);
    }
    const float* p1 = nullptr;
    const float* ps = nullptr;
    if (a.k1 > 0) {
      p1 = wgrad_row(a.x1, a.ldx1, m, a.x1_idx != nullptr, ia);
      if (HAS_SUB) ps = wgrad_row(a.x1_sub, a.ldx1_sub, m, a.x1_sub_idx != nullptr, is);
    }
    const float* p2 = a.k2 > 0 ? a.x2 + m * a.ldx2 : nullptr;
#pragma unroll
    for (int i = 0; i < WTK; ++i) {
      const int kind = (xcode[i] >> 16) & 3, col = xcode[i] & 0xffff;
      const float* src = kind == X_SEG1 ? p1 : (kind == X_SEG2 ? p2 : nullptr);
      xv[i] = ldg4((m_ok && src != nullptr) ? src + col : zero);
      if (HAS_SUB) xs[i] = ldg4((m_ok && ps != nullptr && kind == X_SEG1) ? ps + col : zero);
    }
  };
  auto put = [&](unsigned char* img, int imgbytes, int rowbytes, int chunk8, f32x4 v, float sc) {   // split + one 8-byte store per term
    uint32_t lo[3], hi[3];
    if constexpr (F16) {
      split_pair_h(v.x, v.y, sc, lo[0], lo[1]);
      split_pair_h(v.z, v.w, sc, hi[0], hi[1]);
    } else {
      split_pair(v.x, v.y, lo[0], lo[1], lo[2]);
      split_pair(v.z, v.w, hi[0], hi[1], hi[2]);
    }
    unsigned char* d = img + r * rowbytes + ((chunk8 * 8) ^ xr);
#pragma unroll
    for (int k = 0; k < TERMS; ++k) *reinterpret_cast<uint2*>(d + k * imgbytes) = make_uint2(lo[k], hi[k]);
  };
  auto commit = [&]() {
#pragma unroll
    for (int i = 0; i < 5; ++i) put(lds, ZIMG, ZRB, g + 8 * i, HAS_MASK ? apply_mask(zv[i], zm[i], a.mask_scale) : zv[i], zs);
#pragma unroll
    for (int i = 0; i < WTK; ++i) {
      f32x4 x = xv[i];
      if (HAS_SUB) x = xv[i] - xs[i];
      // k1 % 4 or k2 % 4 != 0, or the ones column: patch per element
      if (partial) x = wgrad_patch_x<HAS_SUB>(xv[i], HAS_SUB ? xs[i] : xv[i], (xcode[i] >> 18) & 7, ((xcode[i] >> 21) & 7) - 1, m_ok);
      put(lds + TERMS * ZIMG, XIMG, XRB, g + 8 * i, x, xsc);
    }
  };

  f32x4 acc[WT][WTK];
  wgrad_zero_acc(acc);

  const int wn = (wave >> 1) * (WT * 16), wk = (wave & 1) * (WTK * 16);
  const int fr = lane & 15, fq = lane >> 4;
  // transposed-read role: lane 4q+p of 16-lane group fq supplies row 8 fq + q, columns 4p..4p+3 of the 16-column block
  const int tq = fr >> 2, tp = fr & 3;
  const int trow = 8 * fq + tq;
  const int txr = (fq & 1) << 5;
  const unsigned char* const zbase = lds + trow * ZRB + 8 * tp;
  const unsigned char* const xbase = lds + TERMS * ZIMG + trow * XRB + 8 * tp;

  fetch_idx(0);
  issue(0);
  fetch_idx(1);
  for (int t = 0; t < ntiles; ++t) {
    commit();                                           // waits for the tile's loads; splits; writes the term images
    __syncthreads();
    if (t + 1 < ntiles) {
      issue(t + 1);
      fetch_idx(t + 2);
    }
    // The X terms of a group of k-tiles stay in registers across the five n-tiles (36 / 24 registers); holding all
    // WTK at once (what common-subexpression elimination makes of the plain double loop) spills next to the 100
    // accumulators and the next tile's chunks in flight.
    constexpr int JH = WTK <= 3 ? WTK : 3;
#pragma unroll
    for (int j0 = 0; j0 < WTK; j0 += JH) {
      asm volatile("" ::: "memory");                    // the second group RE-READS the dZ terms (no CSE across groups)
      u32x4 xt[JH][TERMS];
#pragma unroll
      for (int jj = 0; jj < JH; ++jj) {
        if (j0 + jj < WTK) {
          const int xc = ((wk + 16 * (j0 + jj)) * 2) ^ txr;
#pragma unroll
          for (int k = 0; k < TERMS; ++k) xt[jj][k] = tr_read8(xbase + k * XIMG + xc, XRB);
        }
      }
#pragma unroll
      for (int i = 0; i < WT; ++i) {
        const int zc = ((wn + 16 * i) * 2) ^ txr;
        u32x4 zt[TERMS];
#pragma unroll
        for (int k = 0; k < TERMS; ++k) zt[k] = tr_read8(zbase + k * ZIMG + zc, ZRB);
#pragma unroll
        for (int jj = 0; jj < JH; ++jj)
          if (j0 + jj < WTK) acc[i][j0 + jj] = mfma_terms<F16>(zt, xt[jj], acc[i][j0 + jj]);
      }
    }
    __syncthreads();                                    // every wave is done with the images before the next commit
  }

  if (F16) {                                            // back from the scaled operands (two exact powers of two)
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
      for (int j = 0; j < WTK; ++j) acc[i][j] = (acc[i][j] * izs) * ixs;
  }
  wgrad_store_slab(P, chunk, nb, kb, wn, wk, fr, fq, acc);
}

// fixed-order sum of the chunk slabs into dw / dbias.  64 elements per workgroup; the chunk range is cut in four
// quarters (one per wave) of 8-deep independent loads - a thread walking all ~128 slabs alone keeps too few bytes in flight
// (32 us for 46 MB) - and the quarters are added in a fixed order through LDS: deterministic, no atomics.
__global__ void __launch_bounds__(THREADS) wgrad_reduce_kernel(const float* __restrict__ ws, int nchunks, int64_t slab,
                                                               int N, int K, float* __restrict__ dw, int64_t ld_dw,
                                                               float* __restrict__ dbias, int accumulate) {
  __shared__ float part[4][64];
  const int el = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int64_t e = static_cast<int64_t>(blockIdx.x) * 64 + el;
  const int per = (nchunks + 3) / 4;
  const int c0 = q * per;
  int c1 = c0 + per;
  if (c1 > nchunks) c1 = nchunks;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (e < slab) {
    int c = c0;
    for (; c + 8 <= c1; c += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) s[u] += ws[static_cast<int64_t>(c + u) * slab + e];
    }
    for (; c < c1; ++c) s[0] += ws[static_cast<int64_t>(c) * slab + e];
  }
  part[q][el] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  __syncthreads();
  if (q != 0 || e >= slab) return;
  const float t = (part[0][el] + part[1][el]) + (part[2][el] + part[3][el]);
  const int64_t nk = static_cast<int64_t>(N) * K;
  if (e < nk) {
    const int64_t n = e / K, k = e - n * K;
    float* d = dw + n * ld_dw + k;
    *d = accumulate ? *d + t : t;
  } else if (dbias) {
    float* d = dbias + (e - nk);
    *d = accumulate ? *d + t : t;
  }
}

int64_t wgrad_want_chunks(int64_t M, int N, int kext) {
  const int tiles = ((N + WBN - 1) / WBN) * ((kext + WBN - 1) / WBN);
  // One round of workgroups (2 fit per CU: a 513th would wait a whole round).  Chunk c runs on XCD c % 8
  // (XCD-aware mapping), so the chunk count is a multiple of 8: otherwise some XCDs get one more chunk than their
  // 64 slots hold.  Round 1 ran 384 here (the masked / subtracting loader held ~250 VGPRs and starved the dX chain on
  // the main stream); with the mask applied by the dX GEMM (dZ side output) the kernels are leaner and the full
  // 512 wins: step -1.1 % (same-box A/B: 448 -0.6 %, 320 +2.4 %), this kernel alone -20...-29 %.
#ifndef RR_WGRAD_WGS
#define RR_WGRAD_WGS 512
#endif
  int64_t want = RR_WGRAD_WGS / tiles;
  if (want >= 8) want -= want % 8;
  const int64_t maxc = (M + 63) / 64;
  if (want > maxc) want = maxc;
  if (want < 1) want = 1;
  return want;
}

void wgrad_plan(int64_t M, int N, int k1, int k2, WgradParams* P, int mt = WMT) {
  P->k1p = (k1 + 3) & ~3;                         // segment 2 (and the ones column) start 16-byte aligned
  P->kext = P->k1p + k2 + 1;
  P->nblk_n = (N + WBN - 1) / WBN;
  P->nblk_k = (P->kext + WBN - 1) / WBN;
  const int64_t want = wgrad_want_chunks(M, N, P->kext);
  int64_t rpc = (M + want - 1) / want;
  rpc = (rpc + mt - 1) / mt * mt;
  if (rpc < mt) rpc = mt;
  P->rows_per_chunk = rpc;
  P->nchunks = static_cast<int>((M + rpc - 1) / rpc);
  if (P->nchunks < 1) P->nchunks = 1;
  P->slab = static_cast<int64_t>(N) * (k1 + k2) + N;
}

// One launch of the instantiation an argument set picks: the (mask, sub, wtk) choice written once for both kernel families and
// both arithmetic forms.  FORM: rr_wgrad_args.split - 0 = wgrad_fast_kernel, 1 / 2 = wgrad_split_kernel in three bf16 / two f16 terms.
template <int FORM, bool MASK, bool SUB, int WTK>
void wgrad_launch_one(const WgradParams& P, dim3 grid, hipStream_t s) {
  if constexpr (FORM == 0) wgrad_fast_kernel<MASK, SUB, WTK><<<grid, THREADS, 0, s>>>(P);
  else wgrad_split_kernel<MASK, SUB, WTK, FORM == 2><<<grid, THREADS, 0, s>>>(P);
}
template <int FORM, bool MASK, bool SUB>
void wgrad_launch_wtk(const WgradParams& P, dim3 grid, hipStream_t s, int wtk) {
  if (wtk == 3) wgrad_launch_one<FORM, MASK, SUB, 3>(P, grid, s);
  else if (wtk == 4) wgrad_launch_one<FORM, MASK, SUB, 4>(P, grid, s);
  else wgrad_launch_one<FORM, MASK, SUB, 5>(P, grid, s);
}
template <int FORM>
void wgrad_launch(const WgradParams& P, dim3 grid, hipStream_t s, int wtk) {
  if (P.a.mask && P.a.x1_sub) wgrad_launch_wtk<FORM, true, true>(P, grid, s, wtk);
  else if (P.a.mask) wgrad_launch_wtk<FORM, true, false>(P, grid, s, wtk);
  else if (P.a.x1_sub) wgrad_launch_wtk<FORM, false, true>(P, grid, s, wtk);
  else wgrad_launch_wtk<FORM, false, false>(P, grid, s, wtk);
}
}  // namespace

extern "C" {

#ifdef RR_TRACE
int rr_trace_set_wgrad(unsigned long long* buf) { return rr_trace_set_unit(buf); }
#endif

size_t rr_linear_wgrad_workspace_bytes(int64_t M, int N, int K) {
  if (M < 0 || N < 1 || K < 1) return 0;
  // upper bound over every [k1|k2] split of K: the chunk count is largest for the narrowest extended K
  const int64_t nc = wgrad_want_chunks(M, N, K + 1);
  return static_cast<size_t>(nc) * (static_cast<size_t>(N) * K + N) * sizeof(float);
}

int rr_linear_wgrad_f32(const rr_wgrad_args* args, rr_stream_t stream) {
  RR_CHECK_ARG(args);
  const rr_wgrad_args& a = *args;
  RR_CHECK_ARG(a.M >= 0 && a.N >= 1 && a.k1 >= 0 && a.k2 >= 0 && a.k1 + a.k2 >= 1);
  RR_CHECK_ARG(a.dy && a.dw && a.workspace && a.ld_dy >= a.N && a.ld_dw >= a.k1 + a.k2);
  RR_CHECK_ARG(a.k1 == 0 || (a.x1 && a.ldx1 >= a.k1));
  RR_CHECK_ARG(a.k2 == 0 || (a.x2 && a.ldx2 >= a.k2));
  RR_CHECK_ARG(!a.x1_sub || (a.k1 > 0 && a.ldx1_sub >= a.k1));
  RR_CHECK_ARG(!a.mask || a.ld_mask >= a.N);
  const int K = a.k1 + a.k2;
  WgradParams P;
  P.a = a;
  RR_CHECK_ARG(a.split >= 0 && a.split <= 2);
  RR_CHECK_ARG(a.split != 2 || (a.dy_amax && (a.k1 == 0 || a.x1_amax) && (a.k2 == 0 || a.x2_amax) && (!a.x1_sub || a.x1_sub_amax)));
  wgrad_plan(a.M, a.N, a.k1, a.k2, &P, a.split ? SMT : WMT);
  if (a.workspace_bytes < static_cast<size_t>(P.nchunks) * static_cast<size_t>(P.slab) * sizeof(float))
    return RR_ERR_WORKSPACE;
  P.flags = 0;
  if (a.k1 > 0 && vec_ok(a.x1, a.ldx1)) P.flags |= F_A1_VEC;
  if (a.k2 > 0 && vec_ok(a.x2, a.ldx2)) P.flags |= F_A2_VEC;
  if (a.x1_sub && vec_ok(a.x1_sub, a.ldx1_sub)) P.flags |= F_SUB_VEC;
  if (a.mask && vec_ok(a.mask, a.ld_mask)) P.flags |= F_MASK_VEC;
  if (vec_ok(a.dy, a.ld_dy)) P.flags |= F_EPI_VEC;
  hipStream_t s = static_cast<hipStream_t>(stream);
  dim3 grid(static_cast<unsigned>(P.nblk_n * P.nblk_k * ((P.nchunks + 7) / 8) * 8));
  bool fast = (P.flags & F_EPI_VEC) != 0 && (a.N % 4 == 0) && a.M < (int64_t(1) << 31);
  const int64_t max_pitch = int64_t(1) << 25;          // 16 rows * pitch * 4 bytes must fit the kernel's 32-bit pointer steps
  if (a.ld_dy >= max_pitch || a.ld_mask >= max_pitch || a.ldx1 >= max_pitch || a.ldx1_sub >= max_pitch || a.ldx2 >= max_pitch)
    fast = false;
  if (a.mask && !(P.flags & F_MASK_VEC)) fast = false;
  if (a.k1 > 0 && !(P.flags & F_A1_VEC)) fast = false;
  if (a.k2 > 0 && !(P.flags & F_A2_VEC)) fast = false;
  if (a.x1_sub && !(P.flags & F_SUB_VEC)) fast = false;
  if (fast) {
    // narrowest k-block (96 / 128 / 160 columns) that still covers kext with nblk_k blocks
    const int per_blk = (P.kext + P.nblk_k - 1) / P.nblk_k;
    const int wtk = per_blk <= 96 ? 3 : (per_blk <= 128 ? 4 : 5);
    if (a.split == 2) wgrad_launch<2>(P, grid, s, wtk);   // (a request: the scalar-load geometry below stays on f32)
    else if (a.split == 1) wgrad_launch<1>(P, grid, s, wtk);
    else wgrad_launch<0>(P, grid, s, wtk);
  } else {
    wgrad_kernel<<<grid, THREADS, 0, s>>>(P);
  }
  const int64_t total = P.slab;
  wgrad_reduce_kernel<<<static_cast<unsigned>((total + 63) / 64), THREADS, 0, s>>>(
      static_cast<const float*>(a.workspace), P.nchunks, P.slab, a.N, K, a.dw, a.ld_dw, a.dbias, a.accumulate);
  return rr_launch_status();
}

}  // extern "C"
