// Atom / bond attributions: the adjoint of a layer's FIRST linear map fused with the product by the layer's
// input and a per-row reduction over column segments (rr_input_attribution_f32), and the per-molecule finish that turns the
// per-row terms into atom, bond and molecule numbers (rr_attribution_reduce_f32).  Definitions of this library, not ports.
//
// rr_input_attribution_f32
//   dX[m,k]   = sum_n dz[m,n] * w[n,k]  (+ add[add_idx[m], k])            m < M, k < K <= 128, n < N
//   attr[m,s] (+)= alpha * sum_{k in segment s} x[m,k] * dX[m,k]
//   dx[m,k]   (+)= alpha * dX[m,k]
// A workgroup of four waves owns AT_ROWS = 128 rows: wave v owns the two 16-row tiles 32 v, 32 v + 16 and ALL column tiles of
// them (K <= 128: at most 8 tiles of 16, 2 x 8 accumulators of 4 registers), so a row is finished inside one wave and the
// dense gradient never has to leave the registers.  The contraction runs on v_mfma_f32_16x16x4_f32 (exact f32, one rounding
// per product, the chain of an output element in ascending n-tile, then j, then q with n = 16 t + 4 q + j):
//   A operand  w[n][16 kt + (lane & 15)]      from an LDS image of a chunk of AT_NC = 32 rows of w, staged once per workgroup
//                                             and zero-filled past N and past K (pitch == 4 mod 16: the four row groups of a
//                                             read land on four different 16-bank groups)
//   B operand  dz[m0 + (lane & 15)][n]        one 16-byte load per lane and n-tile, straight from global memory (each dz
//                                             element is read exactly once by exactly one lane), element j -> instruction j
// Both operands of chunk c + 1 are fetched into registers, with unconditional loads, while the MFMAs of chunk c run.
//   C / D      lane holds columns 16 kt + 4 (lane >> 4) + e, e = 0..3, of row m0 + (lane & 15)
// Epilogue per lane: + add, the dx store, and the segment sums over its own 4 KT elements in ascending column; the four lanes
// of a row (lane >> 4 = 0..3) are then combined with two butterfly steps (xor 16, xor 32).  Every order is fixed by (N, K,
// segments) alone, so a row's bits do not depend on M, on its position in a tile or on the launch before it; no atomics.
// Pad bytes: dz past N, x past K and w past K / N are never MULTIPLIED in - lanes select 0.0f instead of loading or using
// them - so a NaN between the logical width and the pitch of an operand cannot reach a result.
//
// rr_attribution_reduce_f32: one wavefront per molecule (plus, in workgroup 0, the padding atom 0 / bond 0), lane = atom,
// strided.  atom[a] is one f32 chain (own term, then the outgoing bonds' source-atom terms in a2b column order), bond and
// bond_sym one f32 operation each, mol_total one f64 chain in ascending atom order: bit-reproducible, no atomics.
#include "rr_common.h"

namespace {

constexpr int AT_WAVES = 4;
constexpr int AT_RT = 2;                          // 16-row tiles per wave
constexpr int AT_ROWS = AT_WAVES * AT_RT * 16;    // rows per workgroup
constexpr int AT_NC = 32;                         // rows of w (contraction indices) staged per chunk
constexpr int AT_NT = AT_NC / 16;                 // n-tiles per chunk
constexpr int AT_MAX_K = RR_ATTR_MAX_K;
constexpr int AT_MAX_SEG = RR_ATTR_MAX_SEG;

struct AttrParams {
  const float* dz;  int64_t ld_dz;
  const float* w;   int64_t ld_w;
  const float* x;   int64_t ld_x;
  const float* add; int64_t ld_add;
  const int32_t* add_idx;
  int64_t M;
  int N, K;
  int n_seg;
  int seg_end[AT_MAX_SEG];
  float alpha;
  int accumulate;
  float* attr; int64_t ld_attr;
  float* dx;   int64_t ld_dx;
  int dz_vec, x_vec;                              // rows of dz / x can be read in 16-byte chunks
};

typedef const __attribute__((address_space(1))) f32x4* at_gptr4;
__device__ __forceinline__ f32x4 at_ldg4(const float* p) { return *(at_gptr4)(p); }

// four consecutive elements of a row starting at column c (c % 4 == 0); elements at or past `width` read as 0
__device__ __forceinline__ f32x4 at_load4(const float* row, int c, int width, bool vec) {
  f32x4 v = f32x4(0.f);
  if (c >= width) return v;
  if (vec) {
    v = at_ldg4(row + c);                         // (ld % 4 == 0 and ld >= width: the chunk lies inside the row's pitch)
    if (c + 1 >= width) v.y = 0.f;
    if (c + 2 >= width) v.z = 0.f;
    if (c + 3 >= width) v.w = 0.f;
  } else {
    v.x = row[c];
    if (c + 1 < width) v.y = row[c + 1];
    if (c + 2 < width) v.z = row[c + 2];
    if (c + 3 < width) v.w = row[c + 3];
  }
  return v;
}

// the same four elements with every load unconditional (an index past the width is clamped to a valid one and the value
// replaced by 0): the prefetch of the next chunk must not sit under a branch, whose join would wait for it
template <bool VEC>
__device__ __forceinline__ f32x4 at_load4_flat(const float* row, int c, int width) {
  f32x4 v;
  if (VEC) {
    v = at_ldg4(row + (c < width ? c : 0));       // (VEC: ld % 4 == 0, so columns 0..3 lie inside the pitch)
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = row[c + e < width ? c + e : 0];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = c + e < width ? v[e] : 0.f;
  return v;
}

template <int KT, bool DZV>
__global__ void __launch_bounds__(64 * AT_WAVES, 2) input_attribution_kernel(const AttrParams P) {
  constexpr int KP = KT * 16;                     // padded column count
  constexpr int PITCH = KP + 4;                   // == 4 (mod 16)
  constexpr int CNT = AT_NC * KP / (64 * AT_WAVES);   // elements of a w chunk per thread (= KP / 4)
  __shared__ float wsm[AT_NC * PITCH];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const int N = P.N, K = P.K;
  const int64_t m0 = static_cast<int64_t>(blockIdx.x) * AT_ROWS + wave * (AT_RT * 16);

  f32x4 acc[AT_RT][KT];
#pragma unroll
  for (int r = 0; r < AT_RT; ++r)
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) acc[r][kt] = f32x4(0.f);

  const float* dzrow[AT_RT];
  bool row_ok[AT_RT];
#pragma unroll
  for (int r = 0; r < AT_RT; ++r) {
    const int64_t m = m0 + r * 16 + l15;
    row_ok[r] = m < P.M;
    dzrow[r] = P.dz + (row_ok[r] ? m : 0) * P.ld_dz;    // (a row past M reads row 0 and is replaced by zeros)
  }

  // chunk n0 in flight: this thread's CNT elements of w[n0 .. n0 + AT_NC) x [0, KP) (zero past N and past K) and this lane's
  // dz fragments, tile t = elements n = n0 + 16 t + 4 q + j.  Fetched one chunk ahead, behind the MFMAs of the chunk before.
  float wv[CNT];
  f32x4 dzn[AT_RT][AT_NT];
  auto fetch = [&](int n0) {
#pragma unroll
    for (int u = 0; u < CNT; ++u) {
      const int i = tid + u * (64 * AT_WAVES);
      const int nn = i / KP, k = i - nn * KP;
      const int n = n0 + nn;
      const bool in = n < N && k < K;
      const float v = P.w[in ? static_cast<int64_t>(n) * P.ld_w + k : 0];
      wv[u] = in ? v : 0.f;
    }
#pragma unroll
    for (int r = 0; r < AT_RT; ++r)
#pragma unroll
      for (int t = 0; t < AT_NT; ++t) {
        const f32x4 v = at_load4_flat<DZV>(dzrow[r], n0 + 16 * t + 4 * q, N);
        dzn[r][t] = row_ok[r] ? v : f32x4(0.f);
      }
  };
  fetch(0);
  for (int n0 = 0; n0 < N; n0 += AT_NC) {
    __syncthreads();                              // the chunk before this one has been read by every wave
#pragma unroll
    for (int u = 0; u < CNT; ++u) {
      const int i = tid + u * (64 * AT_WAVES);
      const int nn = i / KP, k = i - nn * KP;
      wsm[nn * PITCH + k] = wv[u];
    }
    f32x4 dzf[AT_RT][AT_NT];
#pragma unroll
    for (int r = 0; r < AT_RT; ++r)
#pragma unroll
      for (int t = 0; t < AT_NT; ++t) dzf[r][t] = dzn[r][t];
    __syncthreads();
    fetch(n0 + AT_NC);                            // (past the last chunk: clamped addresses, zeros, never used)
    const int nt = (N - n0 + 15) / 16;            // n-tiles of this chunk that hold anything (uniform)
#pragma unroll
    for (int t = 0; t < AT_NT; ++t) {
      if (t < nt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float* wr = wsm + (16 * t + 4 * q + j) * PITCH + l15;
#pragma unroll
          for (int kt = 0; kt < KT; ++kt) {
            const float a = wr[16 * kt];
#pragma unroll
            for (int r = 0; r < AT_RT; ++r) acc[r][kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, dzf[r][t][j], acc[r][kt], 0, 0, 0);
          }
        }
      }
    }
  }

  // ---- epilogue: acc[r][kt][e] = dX[m0 + 16 r + l15][16 kt + 4 q + e]
#pragma unroll
  for (int r = 0; r < AT_RT; ++r) {
    const int64_t m = m0 + r * 16 + l15;
    const bool ok = row_ok[r];
    const float* addrow = nullptr;
    if (P.add != nullptr && ok) addrow = P.add + static_cast<int64_t>(P.add_idx[m]) * P.ld_add;
    const float* xrow = (P.x != nullptr && ok) ? P.x + m * P.ld_x : nullptr;
    float* dxrow = (P.dx != nullptr && ok) ? P.dx + m * P.ld_dx : nullptr;
    float seg[AT_MAX_SEG] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      const int k = 16 * kt + 4 * q;
      f32x4 v = acc[r][kt];
      if (addrow != nullptr) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k + e < K) v[e] = v[e] + addrow[k + e];
      }
      if (dxrow != nullptr) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (k + e < K) {
            const float o = P.alpha * v[e];
            dxrow[k + e] = P.accumulate ? dxrow[k + e] + o : o;
          }
        }
      }
      if (xrow != nullptr) {
        const f32x4 xv = at_load4(xrow, k, K, P.x_vec != 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int kk = k + e;
          const float pr = kk < K ? xv[e] * v[e] : 0.f;
          int lo = 0;
#pragma unroll
          for (int s = 0; s < AT_MAX_SEG; ++s) {
            if (s < P.n_seg) {
              const int hi = P.seg_end[s];
              seg[s] += (kk >= lo && kk < hi) ? pr : 0.f;
              lo = hi;
            }
          }
        }
      }
    }
    if (P.attr != nullptr) {                      // (uniform; rows past M take part in the shuffles with zeros)
#pragma unroll
      for (int s = 0; s < AT_MAX_SEG; ++s) {
        if (s < P.n_seg) {
          float t = seg[s];
          t += __shfl_xor(t, 16, 64);
          t += __shfl_xor(t, 32, 64);
          if (ok && q == 0) {
            float* o = P.attr + m * P.ld_attr + s;
            const float val = P.alpha * t;
            *o = P.accumulate ? *o + val : val;
          }
        }
      }
    }
  }
}

template <int KT>
int launch_attr(const AttrParams& P, hipStream_t s) {
  const int64_t blocks = (P.M + AT_ROWS - 1) / AT_ROWS;
  if (blocks > 0x7fffffffLL) return RR_ERR_UNSUPPORTED;
  if (P.dz_vec) input_attribution_kernel<KT, true><<<static_cast<unsigned>(blocks), 64 * AT_WAVES, 0, s>>>(P);
  else input_attribution_kernel<KT, false><<<static_cast<unsigned>(blocks), 64 * AT_WAVES, 0, s>>>(P);
  return rr_launch_status();
}

// ---------------------------------------------------------------- the finish
struct ReduceParams {
  const float* attr_fa; int64_t ld_fa;
  const float* attr_fb; int64_t ld_fb;
  const int32_t* a2b; const int32_t* b2revb; const int32_t* a_scope;
  int64_t nA, nB, M;
  int K;
  float* atom; float* bond; float* bond_sym; double* mol_total;
};

// atom a: its number, its outgoing bonds' numbers (written here: a directed bond leaves exactly one atom) -> the f64 term
// (double)atom[a] + bond[b_0] + bond[b_1] + ... over the real entries of a2b[a, :] in column order
__device__ __forceinline__ double reduce_atom(const ReduceParams& P, int64_t a) {
  float s = P.attr_fa[a * P.ld_fa];
  const int32_t* row = P.a2b + a * P.K;
  for (int k = 0; k < P.K; ++k) {
    int32_t b = row[k];
    b = (b >= 0 && b < P.nB) ? b : 0;             // (a corrupt table changes values, never an address)
    int32_t o = P.b2revb[b];
    o = (o >= 0 && o < P.nB) ? o : 0;
    s += P.attr_fb[o * P.ld_fb];
  }
  P.atom[a] = s;
  double c = static_cast<double>(s);
  for (int k = 0; k < P.K; ++k) {
    int32_t b = row[k];
    if (b <= 0 || b >= P.nB) continue;            // padding entry
    int32_t o = P.b2revb[b];
    o = (o >= 0 && o < P.nB) ? o : 0;
    int32_t ro = P.b2revb[o];
    ro = (ro >= 0 && ro < P.nB) ? ro : 0;
    const float bo = P.attr_fb[o * P.ld_fb + 1];
    P.bond[o] = bo;
    P.bond_sym[o] = bo + P.attr_fb[ro * P.ld_fb + 1];
    c += static_cast<double>(bo);
  }
  return c;
}

__global__ void __launch_bounds__(RR_WAVE) attribution_reduce_kernel(const ReduceParams P) {
  const int lane = threadIdx.x;
  const int64_t mol = blockIdx.x;
  if (mol == 0 && lane == 0) {                    // the padding rows: atom 0 reads bond 0 K times, bond 0 is its own reverse
    float s = P.attr_fa[0];
    for (int k = 0; k < P.K; ++k) s += P.attr_fb[0];
    P.atom[0] = s;
    const float b0 = P.attr_fb[1];
    P.bond[0] = b0;
    P.bond_sym[0] = b0 + b0;
  }
  if (mol >= P.M) return;
  int64_t start = P.a_scope[2 * mol], size = P.a_scope[2 * mol + 1];
  if (start < 1 || size < 0 || start + size > P.nA) size = 0;
  double total = 0.0;
  for (int64_t base = 0; base < size; base += RR_WAVE) {      // (uniform trip count)
    const int64_t i = base + lane;
    double c = 0.0;
    if (i < size) c = reduce_atom(P, start + i);
    const int cnt = static_cast<int>(size - base < RR_WAVE ? size - base : RR_WAVE);
    for (int j = 0; j < cnt; ++j) total += __shfl(c, j, RR_WAVE);   // ascending atom order, the same chain in every lane
  }
  if (lane == 0) P.mol_total[mol] = total;
}

}  // namespace

extern "C" {

int rr_input_attribution_max_k(void) { return AT_MAX_K; }

int rr_input_attribution_f32(const float* dz, int64_t ld_dz, const float* w, int64_t ld_w, const float* x, int64_t ld_x,
                             const float* add, int64_t ld_add, const int32_t* add_idx, int64_t M, int N, int K,
                             const int32_t* seg_end, int n_seg, float alpha, int accumulate, float* attr, int64_t ld_attr,
                             float* dx, int64_t ld_dx, rr_stream_t stream) {
  RR_CHECK_ARG(dz && w && M >= 0 && N >= 1 && K >= 1);
  RR_CHECK_ARG(attr || dx);
  RR_CHECK_ARG(accumulate == 0 || accumulate == 1);
  if (K > AT_MAX_K) return RR_ERR_UNSUPPORTED;
  RR_CHECK_ARG(ld_dz >= N && ld_w >= K);
  RR_CHECK_ARG((add == nullptr) == (add_idx == nullptr));
  RR_CHECK_ARG(!add || ld_add >= K);
  RR_CHECK_ARG(!dx || ld_dx >= K);
  AttrParams P;
  P.n_seg = 0;
  for (int s = 0; s < AT_MAX_SEG; ++s) P.seg_end[s] = K;
  if (attr) {
    RR_CHECK_ARG(x && ld_x >= K && seg_end && n_seg >= 1 && n_seg <= AT_MAX_SEG && ld_attr >= n_seg);
    int prev = 0;
    for (int s = 0; s < n_seg; ++s) {
      RR_CHECK_ARG(seg_end[s] > prev);
      prev = seg_end[s];
      P.seg_end[s] = seg_end[s];
    }
    RR_CHECK_ARG(prev == K);
    P.n_seg = n_seg;
  }
  if (M == 0) return RR_OK;
  P.dz = dz; P.ld_dz = ld_dz;
  P.w = w; P.ld_w = ld_w;
  P.x = attr ? x : nullptr; P.ld_x = ld_x;
  P.add = add; P.ld_add = ld_add; P.add_idx = add_idx;
  P.M = M; P.N = N; P.K = K;
  P.alpha = alpha; P.accumulate = accumulate;
  P.attr = attr; P.ld_attr = ld_attr;
  P.dx = dx; P.ld_dx = ld_dx;
  P.dz_vec = rr_vec4_ok(dz, ld_dz) ? 1 : 0;
  P.x_vec = (P.x && rr_vec4_ok(P.x, ld_x)) ? 1 : 0;    // (no attributions: x is not read)
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int kt = (K + 15) / 16;
  if (kt <= 1) return launch_attr<1>(P, s);
  if (kt <= 2) return launch_attr<2>(P, s);
  if (kt <= 4) return launch_attr<4>(P, s);
  if (kt <= 6) return launch_attr<6>(P, s);
  return launch_attr<8>(P, s);
}

int rr_attribution_reduce_f32(const float* attr_fa, int64_t ld_fa, const float* attr_fb, int64_t ld_fb, const int32_t* a2b,
                              const int32_t* b2revb, const int32_t* a_scope, int64_t nA, int64_t nB, int64_t M, int K,
                              float* atom, float* bond, float* bond_sym, double* mol_total, rr_stream_t stream) {
  RR_CHECK_ARG(attr_fa && attr_fb && a2b && b2revb && atom && bond && bond_sym);
  RR_CHECK_ARG(nA >= 1 && nB >= 1 && M >= 0 && K >= 1 && ld_fa >= 1 && ld_fb >= 2);
  RR_CHECK_ARG(M == 0 || (a_scope && mol_total));
  if (nB > 0x7fffffffLL || M > 0x7fffffffLL) return RR_ERR_UNSUPPORTED;
  ReduceParams P;
  P.attr_fa = attr_fa; P.ld_fa = ld_fa;
  P.attr_fb = attr_fb; P.ld_fb = ld_fb;
  P.a2b = a2b; P.b2revb = b2revb; P.a_scope = a_scope;
  P.nA = nA; P.nB = nB; P.M = M; P.K = K;
  P.atom = atom; P.bond = bond; P.bond_sym = bond_sym; P.mol_total = mol_total;
  const unsigned grid = static_cast<unsigned>(M > 0 ? M : 1);
  attribution_reduce_kernel<<<grid, RR_WAVE, 0, static_cast<hipStream_t>(stream)>>>(P);
  return rr_launch_status();
}

}  // extern "C"
