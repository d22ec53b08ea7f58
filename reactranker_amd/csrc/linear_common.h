// What more than one of linear.hip, linear_split.hip, wgrad.hip and pack_weights.hip needs: tile constants, LinearParams,
// the loaders, the trace stamps, the zero chunks and the operand term splits.  Everything sits in an anonymous namespace:
// each unit has its own copy (of the 4 KiB zero row as well).
#pragma once
#include "rr_common.h"

namespace {

constexpr int BM = 64;      // rows per workgroup
constexpr int BK = 16;      // k-tile
constexpr int THREADS = 256;

enum : int {
  F_A1_VEC = 1, F_A2_VEC = 2, F_SUB_VEC = 4, F_MASK_VEC = 8, F_W1_VEC = 16, F_W2_VEC = 32, F_EPI_VEC = 64, F_PRE_VEC = 128
};

__host__ __device__ constexpr int r16(int k) { return (k + 15) & ~15; }

struct LinearParams {
  rr_linear_args a;
  int w_k1_off;         // column of W where segment 2 starts (k1, or r16(k1) for packed weights)
  int t1, t2;           // k-tiles of segment 1 / 2
  int flags;
  uint32_t drop_thr;
  float keep_scale;
  int persist;          // linear_split_kernel: one workgroup per CU walks row blocks blockIdx.x, + gridDim.x, ... (see there)
  // linear_split_kernel, balanced last round of a one-block-per-workgroup launch (see there): workgroups [0, bal_full) run
  // full blocks of 3 x 64 rows, the ones behind them share the remaining 64-row units, bal_base or bal_base + 1 (the
  // first bal_rem of them) each.  bal_base = bal_rem = 0: every workgroup runs a full block
  int bal_full, bal_base, bal_rem;
};

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
// Loads whose address is known to be GLOBAL memory.  A pointer that went through a select with a __device__
// constant (the zero / ones chunks) is a generic pointer to hipcc, which then emits flat_load (counted on lgkmcnt
// as well as vmcnt); these keep the weight-gradient loader on global_load (42 flat_load -> 0 in its ISA).
typedef const __attribute__((address_space(1))) f32x4* rr_gptr4;
typedef const __attribute__((address_space(1))) int32_t* rr_gptri;
__device__ __forceinline__ f32x4 ldg4(const float* p) { return *(rr_gptr4)(p); }
__device__ __forceinline__ int32_t ldgi(const int32_t* p) { return *(rr_gptri)(p); }
typedef const __attribute__((address_space(1))) uint8_t* rr_gptrb;
__device__ __forceinline__ uint32_t ldgb(const uint8_t* p) { return *(rr_gptrb)(p); }
// bytes per row of a packed sign mask over N columns: 40 per block of up to 304 columns (2 halves x 20: 19 tile bytes + pad)
__host__ __device__ constexpr int64_t mask_bits_row(int N) { return 40 * ((N + 303) / 304); }

// LDS-DMA: 16 bytes per lane, global -> LDS at (wave-uniform byte address lds_dst) + lane * 16, no VGPR
// destination.  Written as asm so that hipcc does not track it: its own bookkeeping treats an LDS-DMA in
// flight as a may-alias LDS write and drains it (vmcnt(0)) in front of the next ds_read as soon as the
// kernel has a second __shared__ object, which serialises the panel fetch with the MFMA block.  The caller
// waits for it explicitly (rr_wait_vm0) before the barrier that publishes the buffer.
__device__ __forceinline__ void rr_glds16(const float* gsrc, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_dst)
               : "memory");
}
__device__ __forceinline__ void rr_wait_vm0() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ uint32_t rr_lds_addr(const float* p) {
  return static_cast<uint32_t>(reinterpret_cast<uintptr_t>((const __attribute__((address_space(3))) float*)p));
}

// 4 consecutive floats p[k..k+3] of a row with `ks` valid columns; columns >= ks read as 0.
__device__ __forceinline__ f32x4 load_chunk(const float* p, int k, int ks, bool vec) {
  f32x4 v = f32x4(0.f);
  if (p == nullptr || k >= ks) return v;
  if (vec) {
    v = ld4(p + k);
    if (k + 3 >= ks) {
      if (k + 1 >= ks) v.y = 0.f;
      if (k + 2 >= ks) v.z = 0.f;
      v.w = 0.f;
    }
  } else {
    v.x = p[k];
    if (k + 1 < ks) v.y = p[k + 1];
    if (k + 2 < ks) v.z = p[k + 2];
    if (k + 3 < ks) v.w = p[k + 3];
  }
  return v;
}

__device__ __forceinline__ f32x4 apply_mask(f32x4 v, f32x4 mk, float scale) {
  v.x = mk.x > 0.f ? v.x * scale : 0.f;
  v.y = mk.y > 0.f ? v.y * scale : 0.f;
  v.z = mk.z > 0.f ? v.z * scale : 0.f;
  v.w = mk.w > 0.f ? v.w * scale : 0.f;
  return v;
}

#ifdef RR_TRACE
__device__ unsigned long long* rr_trace_buf = nullptr;
#define RR_STAMP(slot)                                                                                   \
  do {                                                                                                   \
    if (rr_trace_buf && threadIdx.x == 0 && blockIdx.y == 0) {                                           \
      rr_trace_buf[static_cast<size_t>(blockIdx.x) * 8 + (slot)] = __builtin_amdgcn_s_memrealtime();     \
      if ((slot) == 1) rr_trace_buf[static_cast<size_t>(blockIdx.x) * 8 + 5] = __builtin_amdgcn_s_memtime(); \
      if ((slot) == 2) rr_trace_buf[static_cast<size_t>(blockIdx.x) * 8 + 6] = __builtin_amdgcn_s_memtime(); \
    }                                                                                                    \
  } while (0)
inline int rr_trace_set_unit(unsigned long long* buf) {   // this unit's copy
  return hipMemcpyToSymbol(HIP_SYMBOL(rr_trace_buf), &buf, sizeof(buf)) == hipSuccess ? 0 : 1;
}
#else
#define RR_STAMP(slot)
#endif

__device__ __attribute__((aligned(16))) const float rr_zero_chunk[4] = {0.f, 0.f, 0.f, 0.f};
// a whole row of zeros (4 KiB): "no row" for loaders that walk a row with a wave-uniform column offset
constexpr int RR_ZERO_ROW = 1024;
__device__ __attribute__((aligned(16))) const float rr_zero_row[RR_ZERO_ROW] = {0.f};

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int SK = 32;                    // k per step

__host__ __device__ constexpr int r32(int k) { return (k + 31) & ~31; }

__device__ __forceinline__ uint32_t cvt_pk_bf16(float lo, float hi) {
  uint32_t r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
// exact three-term split of two floats (packed bf16 pairs, low half = x)
__device__ __forceinline__ void split_pair(float x, float y, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
  p0 = cvt_pk_bf16(x, y);
  float rx = x - __uint_as_float(p0 << 16), ry = y - __uint_as_float(p0 & 0xffff0000u);
  p1 = cvt_pk_bf16(rx, ry);
  rx -= __uint_as_float(p1 << 16);
  ry -= __uint_as_float(p1 & 0xffff0000u);
  p2 = cvt_pk_bf16(rx, ry);
}
__device__ __forceinline__ bf16x8 as_bf16x8(u32x4 v) { return __builtin_bit_cast(bf16x8, v); }
// Two-term f16 form (w_packed = 3): S x = h + l with h = f16(S x), l = f16(S x - h) (round to nearest even; the remainder
// is exact in f32), 22 significant bits of every operand, and  x w = h_x h_w + (h_x l_w + l_x h_w) + terms below
// 2^-22 |x w|: three v_mfma_f32_16x16x32_f16 per k-step instead of six bf16 ones.  S is a power of two that puts the
// tensor's largest magnitude below 2^15 (f16 has 5 exponent bits: the caller supplies the bound).
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f16x8 as_f16x8(u32x4 v) { return __builtin_bit_cast(f16x8, v); }
// the power of two S with 2^14 <= S * bound < 2^15 (bounds outside 2^+-110, zero included, are clamped: nothing to protect
// below, garbage in above), and its inverse
__host__ __device__ __forceinline__ int rr_f16_exp(float bound) {
  uint32_t u;
  __builtin_memcpy(&u, &bound, 4);
  int e = static_cast<int>((u >> 23) & 0xffu) - 127;     // bound < 2^(e+1)
  return e < -110 ? -110 : (e > 110 ? 110 : e);
}
// |v| folded into a running maximum; a wave's maximum into a device float (one atomic per wave, and only while it can
// still raise the slot: a stale read costs an atomic, never a result)
__device__ __forceinline__ float rr_amax4(float m, f32x4 v) {
  return fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
}
// A wave's maximum into a word of LDS (the workgroup's running maximum; the device float gets ONE atomic per workgroup at
// the end of the kernel).  Nothing here touches global memory: a load of the slot at this point would be waited for with
// vmcnt behind every store the epilogue has just issued - loads and stores retire in issue order - and drain the store
// queue at each row block (measured: the GEMM twice as slow); an atomic per wave and block is 4,464 atomics on one address.
__device__ __forceinline__ void rr_amax_commit_wave(float m, unsigned int* lds_word) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(lds_word, __float_as_uint(m));
}
__device__ __forceinline__ float rr_pow2(int e) { return __uint_as_float(static_cast<uint32_t>(127 + e) << 23); }
__device__ __forceinline__ void split_pair_h(float x, float y, float S, uint32_t& p0, uint32_t& p1) {
  const f32x2 v = {x * S, y * S};
  const f16x2 h = __builtin_convertvector(v, f16x2);
  p0 = __builtin_bit_cast(uint32_t, h);
  const f32x2 r = v - __builtin_convertvector(h, f32x2);
  p1 = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, f16x2));
}

inline bool vec_ok(const float* p, int64_t ld) { return p && rr_aligned16(p) && (ld % 4 == 0); }

// rr_linear_f32's arguments as the kernels take them (linear.hip and linear_split.hip each build their own: the type is
// distinct per unit); k-tiles of BK columns - the split dispatcher recounts them in k-steps of SK
inline LinearParams linear_params(const rr_linear_args& a) {
  LinearParams P;
  P.a = a;
  P.w_k1_off = a.w_packed ? r16(a.k1) : a.k1;         // (packed rows are r16(k1) + r16(k2) floats: with k2 = 0 this is the row pitch)
  P.t1 = (a.k1 + BK - 1) / BK;
  P.t2 = (a.k2 + BK - 1) / BK;
  P.flags = 0;
  P.persist = 0;
  P.bal_full = P.bal_base = P.bal_rem = 0;
  if (a.k1 > 0 && vec_ok(a.a1, a.lda1)) P.flags |= F_A1_VEC;
  if (a.k2 > 0 && vec_ok(a.a2, a.lda2)) P.flags |= F_A2_VEC;
  if (a.a1_sub && vec_ok(a.a1_sub, a.lda1_sub)) P.flags |= F_SUB_VEC;
  if (a.a_mask && vec_ok(a.a_mask, a.ld_mask)) P.flags |= F_MASK_VEC;
  if (vec_ok(a.w, a.ldw)) {
    P.flags |= F_W1_VEC;
    if (a.k1 % 4 == 0) P.flags |= F_W2_VEC;
  }
  if (a.w_packed) P.flags |= F_W1_VEC | F_W2_VEC;     // the generic kernel reads packed weights too: segment 2 starts at column r16(k1)
  if (a.N % 4 == 0 && vec_ok(a.c, a.ldc) && (!a.bias || rr_aligned16(a.bias)) &&
      (!a.residual || vec_ok(a.residual, a.ldr)))
    P.flags |= F_EPI_VEC;
  if (a.c_pre && vec_ok(a.c_pre, a.ld_pre)) P.flags |= F_PRE_VEC;
  P.drop_thr = rr_drop_threshold(a.drop_p);
  P.keep_scale = 1.0f / (1.0f - a.drop_p);
  return P;
}
}  // namespace

// Calls between the units: hidden (not part of the library's C ABI), public C types only (LinearParams is distinct per unit).
// linear_split.hip: the split forms of an rr_linear_f32 request that passed its checks (two_f16: w_packed == 3)
extern "C" __attribute__((visibility("hidden"))) int rr_linear_split_launch(const rr_linear_args* args, int two_f16, rr_stream_t stream);
#ifdef RR_TRACE                       // rr_debug_set_trace sets every stamping unit's copy of rr_trace_buf
extern "C" __attribute__((visibility("hidden"))) int rr_trace_set_linear_split(unsigned long long* buf);
extern "C" __attribute__((visibility("hidden"))) int rr_trace_set_wgrad(unsigned long long* buf);
#endif
