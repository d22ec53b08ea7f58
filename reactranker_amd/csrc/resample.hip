// Resampled column means of a per-query statistics table: the bootstrap over queries and the paired
// sign-flip randomisation test.  A definition of this library, not a port; include/reactranker_hip.h states it.
//
//   resample b, position i -> draw j = b * Qe + i of the stream in rr_common.h (Qe = Q rounded up to even, so every resample
//   starts on a 64-bit word); bootstrap: v = x[(draw * Q) >> 32, c]; sign flip: v = +-x[i, c] by bit 31 of the draw.  Lane l of
//   the wave owns the positions with i % 64 == l, ascending: acc = acc + v and n = n + 1 unless v is a NaN; the 64 chains are
//   joined by the butterfly xor 32, 16, 8, 4, 2, 1; mean = acc / n.
//
// rs_kernel<NC, VEC, MODE> is the only kernel: one launch, one wave per resample, resamples grid-strided, 256 threads.  A wave
// walks its resample 128 positions at a time: lane l makes word l of the 64 words those positions use (two draws per word,
// the halves handed to the owning lanes by four ds_bpermute), then gathers two whole rows per lane - both in flight before
// either is added - into NC register accumulators.  Columns go in groups of NC (4, 8 or 16, the narrowest that holds M, 16
// for wider tables: M = 32 at Q = 2^20 must not spill), a group's walk regenerating its draws - the table sits in L2 or
// the Infinity Cache and the gather, not the generator, is what a walk waits for.  VEC: 16-byte loads (x 16-byte aligned and
// ld even) for the column pairs that lie below M, 8-byte loads otherwise: nothing at or past column M is ever read.
// No LDS, no atomics, no workspace: every (resample, column) is summed and written by one wave, so the bits cannot depend on
// the grid.
#include "wave_util.h"

namespace {

constexpr int RS_NT = 256;                        // threads (4 waves: 4 resamples per workgroup and grid pass)
constexpr int RS_WAVES = RS_NT / 64;
constexpr int RS_MAX_BLOCKS = 4096;
constexpr int64_t RS_MAX_Q = 1 << 20;             // row() = (draw * Q) >> 32 is uniform to 2.4e-4 relative up to here (header)
constexpr int RS_MAX_NC = 16;

BlocksKnob g_blocks;                             // (wave_util.h: the storage only; rs_grid is this file's own rule)

struct RsParams {
  const double* x; int64_t ld; int64_t Q; int M;
  uint64_t mixed_seed;                            // rr_mix64(seed)
  uint64_t b0, Qe;
  int64_t B;
  double* mean; int32_t* count;
};

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(1))) f64x2* rs_gptr2;
typedef const __attribute__((address_space(1))) double* rs_gptr1;

// columns c0 .. c0 + NC - 1 of a row, as far as they lie below M (c0 and NC even; the rest hold anything and are never added)
template <int NC, bool VEC>
__device__ __forceinline__ void rs_load(const double* row, int c0, int M, double (&v)[NC]) {
#pragma unroll
  for (int c = 0; c < NC; c += 2) {
    v[c] = 0.0;
    v[c + 1] = 0.0;
    if (c0 + c < M) {                             // (uniform)
      if (VEC && c0 + c + 1 < M) {                // (an odd M's last column is read alone: nothing past column M - 1 is touched)
        const f64x2 t = *(rs_gptr2)(row + c0 + c);
        v[c] = t[0];
        v[c + 1] = t[1];
      } else {
        v[c] = *(rs_gptr1)(row + c0 + c);
        if (c0 + c + 1 < M) v[c + 1] = *(rs_gptr1)(row + c0 + c + 1);
      }
    }
  }
}

template <int NC>
__device__ __forceinline__ void rs_add(double (&acc)[NC], int (&n)[NC], const double (&v)[NC], double sign, bool valid, int c0,
                                       int M) {
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const bool on = valid && c0 + c < M && v[c] == v[c];
    acc[c] = on ? acc[c] + sign * v[c] : acc[c];  // (sign is +-1: the product is exact)
    n[c] += on ? 1 : 0;
  }
}

template <int NC, bool VEC, int MODE>
__global__ void __launch_bounds__(RS_NT) rs_kernel(const RsParams p) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t Q = p.Q;
  const int M = p.M;
  const int half = lane >> 1;
  const bool odd = (lane & 1) != 0;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * RS_WAVES;
  for (int64_t k = static_cast<int64_t>(blockIdx.x) * RS_WAVES + wave; k < p.B; k += stride) {   // (uniform per wave)
    const uint64_t word0 = ((p.b0 + static_cast<uint64_t>(k)) * p.Qe) >> 1;                     // (b * Qe is even)
    for (int c0 = 0; c0 < M; c0 += NC) {
      double acc[NC];
      int n[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) { acc[c] = 0.0; n[c] = 0; }
      for (int64_t i0 = 0; i0 < Q; i0 += 128) {
        // the 64 words of positions i0 .. i0 + 127: lane l makes word l; position i0 + l reads word l / 2, i0 + 64 + l word 32 + l / 2
        const uint64_t w = rr_resample_word(p.mixed_seed, word0 + static_cast<uint64_t>(i0 >> 1) + static_cast<uint64_t>(lane));
        const int hi = static_cast<int>(static_cast<uint32_t>(w >> 32)), lo = static_cast<int>(static_cast<uint32_t>(w));
        const int ha = __shfl(hi, half, 64), la = __shfl(lo, half, 64);
        const int hb = __shfl(hi, 32 + half, 64), lb = __shfl(lo, 32 + half, 64);
        const uint32_t da = static_cast<uint32_t>(odd ? la : ha), db = static_cast<uint32_t>(odd ? lb : hb);
        const int64_t ia = i0 + lane, ib = ia + 64;
        const bool va = ia < Q, vb = ib < Q;
        int64_t ra, rb;
        double sa = 1.0, sb = 1.0;
        if (MODE == RR_RESAMPLE_BOOTSTRAP) {
          ra = static_cast<int64_t>((static_cast<uint64_t>(da) * static_cast<uint64_t>(Q)) >> 32);   // < Q
          rb = static_cast<int64_t>((static_cast<uint64_t>(db) * static_cast<uint64_t>(Q)) >> 32);
        } else {
          ra = va ? ia : 0;                       // (Q > 0 inside this loop: row 0 exists; an invalid position adds nothing)
          rb = vb ? ib : 0;
          sa = (da >> 31) ? -1.0 : 1.0;
          sb = (db >> 31) ? -1.0 : 1.0;
        }
        double xa[NC], xb[NC];
        rs_load<NC, VEC>(p.x + ra * p.ld, c0, M, xa);
        rs_load<NC, VEC>(p.x + rb * p.ld, c0, M, xb);
        rs_add<NC>(acc, n, xa, sa, va, c0, M);
        rs_add<NC>(acc, n, xb, sb, vb, c0, M);
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        acc[c] = rr_wave_sum(acc[c]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) n[c] += __shfl_xor(n[c], off, 64);
      }
      if (lane == 0) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          if (c0 + c < M) {
            const int64_t o = k * M + c0 + c;
            p.mean[o] = n[c] > 0 ? acc[c] / static_cast<double>(n[c]) : __builtin_nan("");
            if (p.count) p.count[o] = n[c];
          }
        }
      }
    }
  }
}

// Workgroups of a launch.  Measured (tools/resample_bench.py, profiles/resample_bench.txt): a table that fits a CU's 32 KiB L1
// runs fastest with one resample per wave; a larger one is gathered faster by FEWER resident waves (not profiled; the likely
// cause: a lane's row spans two or three 128-byte lines that its ten loads should find in L1, and every further wave on the CU
// pushes them out) - two workgroups per CU while the table fits an XCD's 4 MiB L2 (1.91 against 2.54 ms at 10^4 x 20), one
// per CU beyond (33 against 46 ms at 10^5 x 20); the sign flip, which walks the rows in order, takes three workgroups per two
// CUs there (22.9 against 24.6 ms).
int rs_grid(int64_t B, int64_t table_bytes, int mode) {
  int64_t b = g_blocks.get();
  if (b == 0) {
    const int64_t beyond_l2 = mode == RR_RESAMPLE_SIGNFLIP ? 3 * RR_NUM_CU / 2 : RR_NUM_CU;
    const int64_t cap = table_bytes <= (32 << 10) ? RS_MAX_BLOCKS : table_bytes <= (4 << 20) ? 2 * RR_NUM_CU : beyond_l2;
    b = (B + RS_WAVES - 1) / RS_WAVES;            // one resample per wave, up to the cap; the grid strides beyond
    if (b > cap) b = cap;
    if (b < 1) b = 1;
  }
  return static_cast<int>(b);
}

template <int NC, bool VEC>
void rs_launch_mode(int mode, int grid, hipStream_t s, const RsParams& p) {
  if (mode == RR_RESAMPLE_BOOTSTRAP) rs_kernel<NC, VEC, RR_RESAMPLE_BOOTSTRAP><<<grid, RS_NT, 0, s>>>(p);
  else rs_kernel<NC, VEC, RR_RESAMPLE_SIGNFLIP><<<grid, RS_NT, 0, s>>>(p);
}

template <int NC>
void rs_launch(bool vec, int mode, int grid, hipStream_t s, const RsParams& p) {
  if (vec) rs_launch_mode<NC, true>(mode, grid, s, p);
  else rs_launch_mode<NC, false>(mode, grid, s, p);
}

}  // namespace

extern "C" {

int rr_resample_blocks(void) { return g_blocks.get(); }
int rr_resample_set_blocks(int blocks) { return g_blocks.set(blocks, RS_MAX_BLOCKS); }

uint32_t rr_resample_draw_host(uint64_t seed, uint64_t j) { return rr_resample_draw(seed, j); }

int rr_resample_means_f64(const double* x, int64_t ld, int64_t Q, int M, int mode, uint64_t seed, int64_t b0, int64_t B,
                          double* mean, int32_t* count, rr_stream_t stream) {
  RR_CHECK_ARG(mean && Q >= 0 && B >= 0 && b0 >= 0 && M >= 1 && ld >= M);
  RR_CHECK_ARG(x || Q == 0);
  RR_CHECK_ARG(mode == RR_RESAMPLE_BOOTSTRAP || mode == RR_RESAMPLE_SIGNFLIP);
  if (M > RR_RESAMPLE_MAX_COLS || Q > RS_MAX_Q) return RR_ERR_UNSUPPORTED;
  const uint64_t Qe = (static_cast<uint64_t>(Q) + 1) & ~static_cast<uint64_t>(1);
  const uint64_t last = static_cast<uint64_t>(b0) + static_cast<uint64_t>(B);                    // (both below 2^63: no wrap)
  if (Qe > 0 && last > (static_cast<uint64_t>(1) << 63) / Qe) return RR_ERR_UNSUPPORTED;         // (b0 + B) * Qe <= 2^63 ...
  if (Qe > 0 && last * Qe >= (static_cast<uint64_t>(1) << 63)) return RR_ERR_UNSUPPORTED;        // ... and not equal to it
  if (B == 0) return RR_OK;                       // nothing to fill
  RsParams p;
  p.x = x; p.ld = ld; p.Q = Q; p.M = M;
  p.mixed_seed = rr_mix64(seed);
  p.b0 = static_cast<uint64_t>(b0); p.Qe = Qe; p.B = B;
  p.mean = mean; p.count = count;
  const int grid = rs_grid(B, Q * static_cast<int64_t>(M) * 8, mode);
  const bool vec = rr_aligned16(x) && (ld % 2 == 0);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (M <= 4) rs_launch<4>(vec, mode, grid, s, p);
  else if (M <= 8) rs_launch<8>(vec, mode, grid, s, p);
  else rs_launch<RS_MAX_NC>(vec, mode, grid, s, p);
  return rr_launch_status();
}

}  // extern "C"
