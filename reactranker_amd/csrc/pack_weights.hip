// Weight layouts of rr_linear_f32: the zero-padded f32 panels (w_packed = 1), the bf16 / f16 term images of the split
// path (w_packed = 2 / 3), and the magnitude bound (rr_amax_f32) the two-f16-term form scales its operands by.
#include "linear_common.h"

namespace {

// one weight into the zero-padded f32 layout of the fast path (grid-stride over blockIdx.x)
__device__ __forceinline__ void pack_plain_desc(const rr_pack_desc& q) {
  const int k1p = r16(q.k1), ldd = r16(q.k1) + r16(q.k2);
  const int64_t total = static_cast<int64_t>(q.rows) * ldd;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += stride) {
    const int r = static_cast<int>(e / ldd), c = static_cast<int>(e - static_cast<int64_t>(r) * ldd);
    int lc = -1;
    if (c < q.k1) lc = c;
    else if (c >= k1p && c - k1p < q.k2) lc = q.k1 + (c - k1p);
    float v = 0.f;
    if (lc >= 0)
      v = q.transpose ? q.src[static_cast<int64_t>(lc) * q.ld_src + q.c0 + r] : q.src[static_cast<int64_t>(r) * q.ld_src + q.c0 + lc];
    q.dst[e] = v;
  }
}
// dst = zero-padded packed copy of a weight (or of its transpose) for the fast path
__global__ void __launch_bounds__(256) pack_weight_kernel(const float* __restrict__ src, int64_t ld_src, int transpose,
                                                          int rows, int c0, int k1, int k2, float* __restrict__ dst) {
  pack_plain_desc(rr_pack_desc{src, ld_src, transpose, rows, c0, k1, k2, dst, 0});
}
// the same for up to RR_MAX_PACK weights in ONE launch (blockIdx.y = weight): a training step re-packs ~10 weights
// for its forward and ~10 transposes for its backward, each a 2-5 us kernel with a launch boundary around it
constexpr int RR_MAX_PACK_DEV = RR_MAX_PACK;
struct PackMany {
  rr_pack_desc d[RR_MAX_PACK_DEV];
};
__global__ void __launch_bounds__(256) pack_weights_kernel(const PackMany P) {
  const rr_pack_desc& q = P.d[blockIdx.y];
  if (q.split) return;                                 // pack_split_kernel's
  pack_plain_desc(q);
}

constexpr int PACK_SCALE_BLOCKS = 16;
// weight terms of the split path: dst = [k-step][column tile][term 0..2][lane 0..63][8 bf16], the LDS image of a k-step
__device__ __forceinline__ void split_one(float x, uint16_t& t0, uint16_t& t1, uint16_t& t2) {
  uint32_t p0, p1, p2;
  split_pair(x, 0.f, p0, p1, p2);
  t0 = static_cast<uint16_t>(p0 & 0xffffu);
  t1 = static_cast<uint16_t>(p1 & 0xffffu);
  t2 = static_cast<uint16_t>(p2 & 0xffffu);
}
__host__ __device__ constexpr int split_nt(int N) { return N <= 64 ? 4 : (N <= 160 ? 10 : (N <= 304 ? 19 : 38)); }

__device__ __forceinline__ void pack_split_elem(const rr_pack_desc& q, int64_t e, float S) {
  const int nt = split_nt(q.rows);
  const int t1 = r32(q.k1) / SK;
  const int el = static_cast<int>(e & 7), lane = static_cast<int>((e >> 3) & 63);
  const int64_t blk = e >> 9;                          // (s * nt + j)
  const int j = static_cast<int>(blk % nt), s = static_cast<int>(blk / nt);
  const int n = j * 16 + (lane & 15);
  const int kk = (s < t1 ? s : s - t1) * SK + (lane >> 4) * 8 + el;
  int lc = -1;
  if (s < t1) {
    if (kk < q.k1) lc = kk;
  } else if (kk < q.k2) {
    lc = q.k1 + kk;
  }
  float v = 0.f;
  if (lc >= 0 && n < q.rows)
    v = q.transpose ? q.src[static_cast<int64_t>(lc) * q.ld_src + q.c0 + n] : q.src[static_cast<int64_t>(n) * q.ld_src + q.c0 + lc];
  if (q.split == 2) {                                  // two f16 terms of S * L (S from pack_scale_kernel's partial maxima)
    v *= S;
    _Float16* d = reinterpret_cast<_Float16*>(q.dst) + blk * 2 * 512 + lane * 8 + el;
    const _Float16 h = static_cast<_Float16>(v);
    d[0] = h;
    d[512] = static_cast<_Float16>(v - static_cast<float>(h));
    return;
  }
  uint16_t* d = reinterpret_cast<uint16_t*>(q.dst) + blk * 3 * 512 + lane * 8 + el;
  split_one(v, d[0], d[512], d[1024]);
}

// split = 2: largest magnitude of each weight, as PACK_SCALE_BLOCKS partial maxima behind its last image (floats 4 .. of the
// trailer; pack_split_kernel folds them into S = the power of two with 2^14 <= S max|L| < 2^15 and stores S at float 0)
__global__ void __launch_bounds__(1024) pack_scale_kernel(const PackMany P) {
  const rr_pack_desc& q = P.d[blockIdx.y];
  if (q.split != 2) return;
  __shared__ float part[16];
  const int K = q.k1 + q.k2;
  const int64_t total = static_cast<int64_t>(q.rows) * K;
  auto val = [&](int64_t e) -> float {                  // consecutive threads read consecutive memory in either orientation
    const int n = q.transpose ? static_cast<int>(e % q.rows) : static_cast<int>(e / K);
    const int lc = q.transpose ? static_cast<int>(e / q.rows) : static_cast<int>(e % K);
    return fabsf(q.transpose ? q.src[static_cast<int64_t>(lc) * q.ld_src + q.c0 + n] : q.src[static_cast<int64_t>(n) * q.ld_src + q.c0 + lc]);
  };
  float m4[4] = {0.f, 0.f, 0.f, 0.f};
  constexpr int64_t ST = 1024 * PACK_SCALE_BLOCKS;
  int64_t e = static_cast<int64_t>(blockIdx.x) * 1024 + threadIdx.x;
  for (; e + 3 * ST < total; e += 4 * ST) {
#pragma unroll
    for (int u = 0; u < 4; ++u) m4[u] = fmaxf(m4[u], val(e + u * ST));
  }
  for (; e < total; e += ST) m4[0] = fmaxf(m4[0], val(e));
  float m = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
  m = rr_wave_max(m);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 1; i < 16; ++i) m = fmaxf(m, part[i]);
    const int64_t nblk = static_cast<int64_t>((r32(q.k1) + r32(q.k2)) / SK) * split_nt(q.rows);
    q.dst[nblk * 512 + 4 + blockIdx.x] = m;
  }
}

// (one launch packs EVERY weight of a pass: the f32 panels of the FFN head as well - blockIdx.y picks the weight, its
// `split` the layout; a second launch for the plain ones cost a ~7 us kernel + a launch boundary in front of every forward)
__global__ void __launch_bounds__(256) pack_split_kernel(const PackMany P) {
  const rr_pack_desc& q = P.d[blockIdx.y];
  if (!q.split) {
    pack_plain_desc(q);
    return;
  }
  const int64_t total = static_cast<int64_t>((r32(q.k1) + r32(q.k2)) / SK) * split_nt(q.rows) * 512;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  float S = 1.f;
  if (q.split == 2) {                                  // fold pack_scale_kernel's partial maxima; thread 0 leaves S for the GEMM
    const int64_t nblk = total / 512;
    const float* part = q.dst + nblk * 512 + 4;
    float m = part[0];
#pragma unroll
    for (int i = 1; i < PACK_SCALE_BLOCKS; ++i) m = fmaxf(m, part[i]);
    S = rr_pow2(14 - rr_f16_exp(m));
    if (blockIdx.x == 0 && threadIdx.x == 0) q.dst[nblk * 512] = S;
  }
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += stride) pack_split_elem(q, e, S);
}

// largest magnitude of a [rows, per_row (x 4 when VEC)] block, maxed into the magnitude slot `out` (non-negative floats order
// like their bit patterns; a NaN fails every comparison and is skipped)
template <bool VEC>
__global__ void __launch_bounds__(256) amax_kernel(const float* __restrict__ x, int64_t total, int per_row, int64_t ld, int tail,
                                                   float* __restrict__ out) {
  __shared__ float part[4];
  float m[4] = {0.f, 0.f, 0.f, 0.f};
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
  const bool dense = VEC ? ld == 4 * static_cast<int64_t>(per_row) : ld == per_row;
  auto at = [&](int64_t e) -> int64_t { return dense ? e * (VEC ? 4 : 1) : (e / per_row) * ld + (e % per_row) * (VEC ? 4 : 1); };
  // VEC with cols % 4 != 0 (rows are 16-byte aligned, the last chunk of a row holds padding): its tail elements do not count
  auto ldv = [&](int64_t e) -> f32x4 {
    f32x4 v = ldg4(x + at(e));
    if (tail != 0 && (e % per_row) == per_row - 1) {
      if (tail < 2) v.y = 0.f;
      if (tail < 3) v.z = 0.f;
      v.w = 0.f;
    }
    return v;
  };
  int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  for (; e + 3 * stride < total; e += 4 * stride) {      // four independent loads in flight per thread
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (VEC) {
        const f32x4 v = ldv(e + u * stride);
        m[u] = fmaxf(fmaxf(m[u], fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
      } else {
        m[u] = fmaxf(m[u], fabsf(x[at(e + u * stride)]));
      }
    }
  }
  for (; e < total; e += stride) {
    if (VEC) {
      const f32x4 v = ldv(e);
      m[0] = fmaxf(fmaxf(m[0], fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    } else {
      m[0] = fmaxf(m[0], fabsf(x[at(e)]));
    }
  }
  float r = fmaxf(fmaxf(m[0], m[1]), fmaxf(m[2], m[3]));
  r = rr_wave_max(r);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    rr_amax_put(out, fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3])));
  }
}
}  // namespace

extern "C" {

int rr_pack_weight_f32(const float* src, int64_t ld_src, int transpose, int rows, int c0, int k1, int k2, float* dst,
                       rr_stream_t stream) {
  RR_CHECK_ARG(src && dst && rows >= 1 && c0 >= 0 && k1 >= 0 && k2 >= 0 && k1 + k2 >= 1 && ld_src >= 1);
  const int64_t total = static_cast<int64_t>(rows) * (r16(k1) + r16(k2));
  pack_weight_kernel<<<rr_grid_for(total, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(src, ld_src, transpose, rows,
                                                                                           c0, k1, k2, dst);
  return rr_launch_status();
}

int rr_pack_weights_f32(const rr_pack_desc* descs, int n, rr_stream_t stream) {
  RR_CHECK_ARG(descs && n >= 0 && n <= RR_MAX_PACK);
  if (n == 0) return RR_OK;
  PackMany P;
  int64_t biggest = 0, biggest_split = 0;
  for (int i = 0; i < n; ++i) {
    const rr_pack_desc& q = descs[i];
    RR_CHECK_ARG(q.src && q.dst && q.rows >= 1 && q.c0 >= 0 && q.k1 >= 0 && q.k2 >= 0 && q.k1 + q.k2 >= 1 && q.ld_src >= 1);
    RR_CHECK_ARG(q.split == 0 || ((q.split == 1 || q.split == 2) && q.rows <= 608 && rr_aligned16(q.dst)));
    P.d[i] = q;
    const int64_t total = q.split ? static_cast<int64_t>((r32(q.k1) + r32(q.k2)) / SK) * split_nt(q.rows) * 512
                                  : static_cast<int64_t>(q.rows) * (r16(q.k1) + r16(q.k2));
    if (total > (q.split ? biggest_split : biggest)) (q.split ? biggest_split : biggest) = total;
  }
  for (int i = n; i < RR_MAX_PACK; ++i) P.d[i] = descs[0];
  if (biggest_split > 0) {                             // split weights present: ONE launch packs both layouts
    bool any_f16 = false;
    for (int i = 0; i < n; ++i) any_f16 = any_f16 || descs[i].split == 2;
    if (any_f16) pack_scale_kernel<<<dim3(PACK_SCALE_BLOCKS, static_cast<unsigned>(n)), 1024, 0, static_cast<hipStream_t>(stream)>>>(P);
    const int64_t work = biggest_split > biggest ? biggest_split : biggest;
    dim3 grid(static_cast<unsigned>(rr_grid_for(work, 256, 64)), static_cast<unsigned>(n));
    pack_split_kernel<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(P);
  } else if (biggest > 0) {
    dim3 grid(static_cast<unsigned>(rr_grid_for(biggest, 256, 64)), static_cast<unsigned>(n));
    pack_weights_kernel<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(P);
  }
  return rr_launch_status();
}

int rr_amax_f32(const float* x, int64_t rows, int cols, int64_t ld, float* amax, rr_stream_t stream) {
  RR_CHECK_ARG(x && amax && rows >= 0 && cols >= 1 && ld >= cols);
  if (rows == 0) return RR_OK;
  const bool vec = vec_ok(x, ld) && (cols + 3) / 4 * 4 <= ld;
  const int64_t per_row = vec ? (cols + 3) / 4 : cols;
  const int64_t total = rows * per_row;
  const unsigned grid = static_cast<unsigned>(rr_grid_for((total + 3) / 4, 256, 1024));
  if (vec) amax_kernel<true><<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(x, total, static_cast<int>(per_row), ld, cols % 4, amax);
  else amax_kernel<false><<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(x, total, static_cast<int>(per_row), ld, 0, amax);
  return rr_launch_status();
}

int64_t rr_packed_weight_ld(int k1, int k2) { return r16(k1) + r16(k2); }

size_t rr_split_weight_bytes(int rows, int k1, int k2) {
  if (rows < 1 || rows > 608 || k1 < 0 || k2 < 0 || k1 + k2 < 1) return 0;
  return static_cast<size_t>((r32(k1) + r32(k2)) / SK) * split_nt(rows) * 3 * 1024;
}

}  // extern "C"
