// Dense layers of the D-MPNN path: f32 GEMMs with fused prologues / epilogues, in two arithmetic forms -
//   * linear_fast_kernel (here) / wgrad_fast_kernel (wgrad.hip): every product on the exact-f32 matrix core (v_mfma_f32_16x16x4_f32);
//     the FFN head, shapes off the fast path, and every GEMM under RR_PLAN_F32_GEMM;
//   * linear_split_kernel (linear_split.hip) / wgrad_split_kernel (wgrad.hip): the encoder's GEMMs on the bf16 matrix core through
//     exact three-term operand splits (x = x0 + x1 + x2 in bf16, six products per f32 multiply, f32 accumulation).
//
//   rr_linear_f32        C = dropout(act(residual + bias + [A1|A2] * W^T))   (forward, and dX with W^T)
//   rr_linear_wgrad_f32  dW = dZ^T * [X1|X2],  dbias = colsum(dZ)            (weight gradients)
//
// Both fuse the reference's surrounding ATen ops into the operand load / epilogue:
// row gather + subtract (a_message[b2a] - message[b2revb], models/mpn.py:91-92), the
// concat of two sources (models/mpn.py:103, 208, 217), ReLU/dropout backward masks, bias,
// residual add, ReLU and dropout (models/mpn.py:94-97).
//
// Geometry (forward): workgroup = 4 waves = 64 rows of A x up to 304 output columns
// (19 MFMA tiles of 16), so the streamed / gathered operand A leaves HBM exactly once and
// the small weight matrix is served from L2.  K is walked in 16-wide tiles, double
// buffered in LDS (47 KB -> 3 workgroups per CU), one barrier per tile.  The MFMA is fed
// with W as its "A" operand and the activations as "B", so a lane's 4 accumulator
// registers are 4 consecutive output columns of one row: the epilogue is 16-byte loads and
// stores.  LDS rows are 64 B with the four 16-byte chunks XOR-swizzled so that
// ds_read_b128 fragment reads are bank-conflict free.
//
// The f32 MFMA is bit-for-bit an fmaf chain; the split path drops no operand bit (its omitted cross terms lie below
// 2^-26 |x w| per product) and measures at or below the f32 chain's error against f64 (tests/test_gpu_split.py,
// tests/test_gpu_headline_kernels.py).  Results differ from the CPU reference by summation order.
#include "linear_common.h"

namespace {

__device__ __forceinline__ int swz(int row, int kq) { return kq ^ ((0 - (row >> 2)) & 3); }

// MODE: 0 plain / concat, 1 = A1 minus a second (optionally gathered) source, 2 = ReLU-backward mask on A
template <int NT, int MODE>
__global__ void __launch_bounds__(THREADS) linear_kernel(const LinearParams P) {
  constexpr int BN = 16 * NT;
  constexpr int B_ITERS = (BN * 4 + THREADS - 1) / THREADS;     // float4 chunks of the W tile per thread
  __shared__ __attribute__((aligned(16))) float lds[2][(BM + BN) * BK];

  const rr_linear_args& a = P.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m0 = static_cast<int64_t>(blockIdx.x) * BM;
  const int n0 = blockIdx.y * BN;
  const int flags = P.flags;

  // ---- this thread's staging assignment: one 16-byte chunk of A, B_ITERS chunks of W per k-tile
  const int srow = tid >> 2, skq = tid & 3;
  const int64_t sm = m0 + srow;
  const float* rowp1 = nullptr;
  const float* rowp2 = nullptr;
  const float* subp = nullptr;
  const float* maskp = nullptr;
  if (sm < a.M) {
    if (a.k1 > 0) {
      if (a.a1_idx) {
        const int32_t j = a.a1_idx[sm];
        if (j >= 0) rowp1 = a.a1 + static_cast<int64_t>(j) * a.lda1;
      } else {
        rowp1 = a.a1 + sm * a.lda1;
      }
      if (MODE == 1 && a.a1_sub) {
        if (a.a1_sub_idx) {
          const int32_t j = a.a1_sub_idx[sm];
          if (j >= 0) subp = a.a1_sub + static_cast<int64_t>(j) * a.lda1_sub;
        } else {
          subp = a.a1_sub + sm * a.lda1_sub;
        }
      }
    }
    if (a.k2 > 0) rowp2 = a.a2 + sm * a.lda2;
    if (MODE == 2) maskp = a.a_mask + sm * a.ld_mask;
  }
  const int ktot = a.k1 + a.k2;
  (void)ktot;

  auto load_a = [&](int kt) -> f32x4 {
    f32x4 v;
    if (kt < P.t1) {
      const int k = kt * BK + skq * 4;
      v = load_chunk(rowp1, k, a.k1, flags & F_A1_VEC);
      if (MODE == 1) v = v - load_chunk(subp, k, a.k1, flags & F_SUB_VEC);
      if (MODE == 2) v = apply_mask(v, load_chunk(maskp, k, a.k1, flags & F_MASK_VEC), a.mask_scale);
    } else {
      const int k = (kt - P.t1) * BK + skq * 4;
      v = load_chunk(rowp2, k, a.k2, flags & F_A2_VEC);
    }
    return v;
  };
  auto load_w = [&](int kt, int it) -> f32x4 {
    const int f = it * THREADS + tid;            // chunk id inside the W tile
    const int wr = f >> 2;                       // tile row (output column), kq == skq
    const int n = n0 + wr;
    if (wr >= BN || n >= a.N) return f32x4(0.f);
    const float* wp = a.w + static_cast<int64_t>(n) * a.ldw;
    if (kt < P.t1) return load_chunk(wp, kt * BK + skq * 4, a.k1, flags & F_W1_VEC);
    return load_chunk(wp + P.w_k1_off, (kt - P.t1) * BK + skq * 4, a.k2, flags & F_W2_VEC);
  };
  auto store_tile = [&](int buf, const f32x4& ra, const f32x4 (&rb)[B_ITERS]) {
    float* As = lds[buf];
    float* Bs = lds[buf] + BM * BK;
    *reinterpret_cast<f32x4*>(As + srow * BK + 4 * swz(srow, skq)) = ra;
#pragma unroll
    for (int it = 0; it < B_ITERS; ++it) {
      const int wr = (it * THREADS + tid) >> 2;
      if (wr < BN) *reinterpret_cast<f32x4*>(Bs + wr * BK + 4 * swz(wr, skq)) = rb[it];
    }
  };

  f32x4 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) acc[i] = f32x4(0.f);

  const int nk = P.t1 + P.t2;
  f32x4 ra;
  f32x4 rb[B_ITERS];
  ra = load_a(0);
#pragma unroll
  for (int it = 0; it < B_ITERS; ++it) rb[it] = load_w(0, it);
  store_tile(0, ra, rb);
  __syncthreads();

  const int fr = lane & 15, fkq = lane >> 4;
  const int a_off = (wave * 16 + fr) * BK + 4 * swz(fr, fkq);
  const int b_off = fr * BK + 4 * swz(fr, fkq);

  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nk;
    if (more) {                                   // next tile's global loads fly during the MFMAs
      ra = load_a(kt + 1);
#pragma unroll
      for (int it = 0; it < B_ITERS; ++it) rb[it] = load_w(kt + 1, it);
    }
    const float* As = lds[cur];
    const float* Bs = lds[cur] + BM * BK;
    const f32x4 af = ld4(As + a_off);
    constexpr int G = 5;                          // column tiles per group: MFMA dependency distance >= 4
#pragma unroll
    for (int t0 = 0; t0 < NT; t0 += G) {
      f32x4 wf[G];
#pragma unroll
      for (int g = 0; g < G; ++g)
        if (t0 + g < NT) wf[g] = ld4(Bs + (t0 + g) * 16 * BK + b_off);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int g = 0; g < G; ++g)
          if (t0 + g < NT) acc[t0 + g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[g][j], af[j], acc[t0 + g], 0, 0, 0);
      }
    }
    if (more) store_tile(cur ^ 1, ra, rb);
    __syncthreads();
  }

  // ---- epilogue: lane holds C[m][n .. n+3] per tile: m = row (lane&15), n = tile*16 + (lane>>4)*4
  const int64_t m = m0 + wave * 16 + fr;
  if (m >= a.M) return;
  const int nq = fkq * 4;
  float* crow = a.c + m * a.ldc;
  const float* rrow = nullptr;
  if (a.residual) {
    const int64_t rr = a.residual_idx ? static_cast<int64_t>(a.residual_idx[m]) : m;
    if (rr >= 0) rrow = a.residual + rr * a.ldr;
  }
  const bool evec = flags & F_EPI_VEC;
#pragma unroll
  for (int tc = 0; tc < NT; ++tc) {
    const int n = n0 + tc * 16 + nq;
    if (n >= a.N) continue;
    f32x4 v = acc[tc];
    if (evec) {
      if (a.bias) v = v + ld4(a.bias + n);
      if (rrow) v = v + ld4(rrow + n);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (n + e < a.N) {
          if (a.bias) v[e] += a.bias[n + e];
          if (rrow) v[e] += rrow[n + e];
        }
      }
    }
    if (a.c_pre) {
      float* prow = a.c_pre + m * a.ld_pre;
      if (evec && (flags & F_PRE_VEC)) {
        *reinterpret_cast<f32x4*>(prow + n) = v;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (n + e < a.N) prow[n + e] = v[e];
      }
    }
    if (a.act == RR_ACT_RELU) {
      v.x = fmaxf(v.x, 0.f);
      v.y = fmaxf(v.y, 0.f);
      v.z = fmaxf(v.z, 0.f);
      v.w = fmaxf(v.w, 0.f);
    }
    if (P.drop_thr != 0u) {
      const uint64_t base = static_cast<uint64_t>(m) * static_cast<uint64_t>(a.N) + static_cast<uint64_t>(n);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = rr_keep(a.drop_seed, base + e, P.drop_thr) ? v[e] * P.keep_scale : 0.f;
    }
    if (evec) {
      *reinterpret_cast<f32x4*>(crow + n) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (n + e < a.N) crow[n + e] = v[e];
    }
  }
}

// ------------------------------------------------------------------------ fast path
// Same math as linear_kernel, for the hot case: every A source 16-byte addressable and W in
// the packed layout of rr_pack_weight_f32 ([N][r16(k1) + r16(k2)], zero padded).  The loader
// is straight-line code: the W panel of a k-tile goes global -> LDS by LDS-DMA (global_load_lds,
// no VGPR round trip, no ds_write; row index clamped, pad columns are zeros, the XOR swizzle of
// the LDS image is applied to the per-lane source address), A chunks are loaded
// unconditionally from (valid ? row + k : dummy), and every
// fix-up (tail columns, invalid rows, the subtraction / ReLU mask of MODE 1 / 2) happens when
// the registers are written to LDS, i.e. AFTER the k-tile's MFMAs.  Nothing uses a loaded
// value before that point, so the compiler keeps all loads of tile t+1 in flight across the
// whole MFMA block of tile t (the generic kernel waits on each load as it is issued).
template <int NT, int MODE>
__global__ void __launch_bounds__(THREADS, 3) linear_fast_kernel(const LinearParams P) {
  constexpr int BN = 16 * NT;
  __shared__ __attribute__((aligned(16))) float lds[2][(BM + BN) * BK];
  __shared__ __attribute__((aligned(16))) float bias_s[BN];

  const rr_linear_args& a = P.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m0 = static_cast<int64_t>(blockIdx.x) * BM;
  const int n0 = blockIdx.y * BN;
  RR_STAMP(0);
#ifdef RR_TRACE
  if (rr_trace_buf && threadIdx.x == 0 && blockIdx.y == 0) {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    rr_trace_buf[static_cast<size_t>(blockIdx.x) * 8 + 4] = (static_cast<unsigned long long>(xcc) << 32) | hw;
  }
#endif

  const int srow = tid >> 2, skq = tid & 3;
  const int64_t sm = m0 + srow;
  const float* const dummy = a.w;                     // any valid, 16-byte aligned address
  const float* rowp1 = nullptr;
  const float* rowp2 = nullptr;
  const float* subp = nullptr;                        // MODE 1: subtract source, MODE 2: mask source
  {
    // both gather indices are loaded before either is used (one memory round trip, not two): the loads are
    // unconditional from a selected address, the row pointers are derived afterwards
    const bool in_m = sm < a.M;
    const int64_t smc = in_m ? sm : 0;
    const bool g1 = a.k1 > 0 && a.a1_idx != nullptr;
    const bool g2 = MODE == 1 && a.k1 > 0 && a.a1_sub != nullptr && a.a1_sub_idx != nullptr;
    const int32_t* const izero = reinterpret_cast<const int32_t*>(rr_zero_chunk);
    const int32_t j1 = *(g1 ? a.a1_idx + smc : izero);
    const int32_t j2 = *(g2 ? a.a1_sub_idx + smc : izero);
    if (in_m) {
      if (a.k1 > 0) {
        if (g1) {
          if (j1 >= 0) rowp1 = a.a1 + static_cast<int64_t>(j1) * a.lda1;
        } else {
          rowp1 = a.a1 + sm * a.lda1;
        }
        if (MODE == 1 && a.a1_sub) {
          if (g2) {
            if (j2 >= 0) subp = a.a1_sub + static_cast<int64_t>(j2) * a.lda1_sub;
          } else {
            subp = a.a1_sub + sm * a.lda1_sub;
          }
        }
        if (MODE == 2) subp = a.a_mask + sm * a.ld_mask;
      }
      if (a.k2 > 0) rowp2 = a.a2 + sm * a.lda2;
    }
  }
  float* dzrow = nullptr;                             // MODE 2 side output: dz_out (+)= masked operand
  if (MODE == 2 && a.dz_out && sm < a.M && blockIdx.y == 0) dzrow = a.dz_out + sm * a.ld_dz;
  // W panel by LDS-DMA: wave-instruction j fills column tile j (16 rows x 4 chunks = 1 KiB, lane-linear
  // in LDS); the XOR swizzle of the LDS image goes on each lane's SOURCE column chunk.
  constexpr int G_ITERS = (NT + 3) / 4;
  const int uwave = __builtin_amdgcn_readfirstlane(wave) & 3;
  const float* wsrc[G_ITERS];
#pragma unroll
  for (int it = 0; it < G_ITERS; ++it) {
    const int wr = (it * 4 + uwave) * 16 + (lane >> 2);
    int n = n0 + wr;
    if (n > a.N - 1) n = a.N - 1;
    wsrc[it] = a.w + static_cast<int64_t>(n) * a.ldw + 4 * swz(wr, lane & 3);
  }
  const int k1p = r16(a.k1);

  f32x4 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) acc[i] = f32x4(0.f);

  const int nk = P.t1 + P.t2;
  f32x4 ra, rs, rc;

  auto issue = [&](int kt) {                          // pure loads, no arithmetic on the results
    const bool seg1 = kt < P.t1;
    const int kl = (seg1 ? kt : kt - P.t1) * BK + skq * 4;
    const float* p = seg1 ? rowp1 : rowp2;
    const int ks = seg1 ? a.k1 : a.k2;
    ra = ld4((p != nullptr && kl < ks) ? p + kl : dummy);
    if (MODE != 0) rs = ld4((seg1 && subp != nullptr && kl < ks) ? subp + kl : dummy);
    if (MODE == 2) {
      if (a.dz_accumulate) rc = ld4((dzrow != nullptr && kl < ks) ? dzrow + kl : dummy);
    }
    const int kw = seg1 ? kt * BK : k1p + (kt - P.t1) * BK;
    float* Bd = lds[kt & 1] + BM * BK;
#pragma unroll
    for (int it = 0; it < G_ITERS; ++it) {
      const int j = it * 4 + uwave;
      if (j < NT) rr_glds16(wsrc[it] + kw, rr_lds_addr(Bd + j * 16 * BK));
    }
  };
  auto commit = [&](int kt, int buf) {                // fix-ups + LDS stores (first use of the loads)
    const bool seg1 = kt < P.t1;
    const int kl = (seg1 ? kt : kt - P.t1) * BK + skq * 4;
    const float* p = seg1 ? rowp1 : rowp2;
    const int ks = seg1 ? a.k1 : a.k2;
    const bool ok = (p != nullptr);
    f32x4 v;
    v.x = (ok && kl + 0 < ks) ? ra.x : 0.f;
    v.y = (ok && kl + 1 < ks) ? ra.y : 0.f;
    v.z = (ok && kl + 2 < ks) ? ra.z : 0.f;
    v.w = (ok && kl + 3 < ks) ? ra.w : 0.f;
    if (MODE == 1) {
      const bool oks = seg1 && (subp != nullptr);
      v.x -= (oks && kl + 0 < ks) ? rs.x : 0.f;
      v.y -= (oks && kl + 1 < ks) ? rs.y : 0.f;
      v.z -= (oks && kl + 2 < ks) ? rs.z : 0.f;
      v.w -= (oks && kl + 3 < ks) ? rs.w : 0.f;
    }
    if (MODE == 2) {
      const bool oks = seg1 && (subp != nullptr);
      v.x = (oks && kl + 0 < ks && rs.x > 0.f) ? v.x * a.mask_scale : 0.f;
      v.y = (oks && kl + 1 < ks && rs.y > 0.f) ? v.y * a.mask_scale : 0.f;
      v.z = (oks && kl + 2 < ks && rs.z > 0.f) ? v.z * a.mask_scale : 0.f;
      v.w = (oks && kl + 3 < ks && rs.w > 0.f) ? v.w * a.mask_scale : 0.f;
      if (dzrow != nullptr && kl < ks)                  // k1 % 4 == 0: the chunk is whole
        *reinterpret_cast<f32x4*>(dzrow + kl) = a.dz_accumulate ? v + rc : v;
    }
    float* As = lds[buf];
    *reinterpret_cast<f32x4*>(As + srow * BK + 4 * swz(srow, skq)) = v;
  };

  if (tid < BN / 4) {                                  // bias slice of this column block -> LDS (read in the epilogue)
    const int n = n0 + tid * 4;
    *reinterpret_cast<f32x4*>(bias_s + tid * 4) = ld4((a.bias && n < a.N) ? a.bias + n : dummy);
  }
  issue(0);
  commit(0, 0);
  rr_wait_vm0();                                       // the LDS-DMA of the first W panel
  __syncthreads();
  RR_STAMP(1);

  const int fr = lane & 15, fkq = lane >> 4;
  const int a_off = (wave * 16 + fr) * BK + 4 * swz(fr, fkq);
  const int b_off = fr * BK + 4 * swz(fr, fkq);

  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nk;
    if (more) issue(kt + 1);
    const float* As = lds[cur];
    const float* Bs = lds[cur] + BM * BK;
    const f32x4 af = ld4(As + a_off);
    constexpr int G = 5;
#pragma unroll
    for (int t0 = 0; t0 < NT; t0 += G) {
      f32x4 wf[G];
#pragma unroll
      for (int g = 0; g < G; ++g)
        if (t0 + g < NT) wf[g] = ld4(Bs + (t0 + g) * 16 * BK + b_off);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int g = 0; g < G; ++g)
          if (t0 + g < NT) acc[t0 + g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[g][j], af[j], acc[t0 + g], 0, 0, 0);
      }
    }
    if (more) commit(kt + 1, cur ^ 1);
    rr_wait_vm0();                                     // W panel of tile kt+1 has landed in LDS
    __syncthreads();
  }

  // ---- epilogue (vector form only: the fast path requires F_EPI_VEC).
  // vmcnt retires loads and stores in issue order, so a wait for a load that was issued after a
  // store also waits for that store's write acknowledge.  The tile loop is therefore kept free of
  // path-dependent memory operations (unconditional loads from a safe address, selects instead of
  // branches, bias from LDS) and the residual chunks run D tiles ahead in a register ring: a store
  // is only ever waited for D tiles after it was issued, instead of one write round trip per tile.
  RR_STAMP(2);
  const int64_t m = m0 + wave * 16 + fr;
  const bool row_ok = m < a.M;
  const int64_t mc = row_ok ? m : a.M - 1;
  const int nq = fkq * 4;
  float* crow = a.c + mc * a.ldc;
  const float* rrow = nullptr;
  if (a.residual) {
    const int64_t rr = a.residual_idx ? static_cast<int64_t>(a.residual_idx[mc]) : mc;
    if (rr >= 0) rrow = a.residual + rr * a.ldr;
  }
  const bool has_bias = a.bias != nullptr;
  const bool relu = a.act == RR_ACT_RELU;
  auto finish = [&](f32x4 v, int n) -> f32x4 {         // activation + dropout + store of one chunk; returns what was stored
    if (relu) {
      v.x = fmaxf(v.x, 0.f);
      v.y = fmaxf(v.y, 0.f);
      v.z = fmaxf(v.z, 0.f);
      v.w = fmaxf(v.w, 0.f);
    }
    if (P.drop_thr != 0u) {
      // N % 4 == 0 and n % 4 == 0 on this path: the 4 elements are one aligned group of the mask stream
      const uint64_t base = static_cast<uint64_t>(m) * static_cast<uint64_t>(a.N) + static_cast<uint64_t>(n);
      const uint32_t w = rr_hash_group(a.drop_seed, base >> 2);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = rr_hash_lane(w, e) >= P.drop_thr ? v[e] * P.keep_scale : 0.f;
    }
    if (row_ok && n < a.N) *reinterpret_cast<f32x4*>(crow + n) = v;
    return v;
  };
  float* prow = a.c_pre ? a.c_pre + mc * a.ld_pre : nullptr;   // pre-activation side output (W_i layers)
  // Optional third output: partial[blockIdx.x, n] = sum over this workgroup's 64 rows of w[m] * C[m, n] (the padding
  // row's adjoint, see rr_linear_args.colsum_partial).  A lane holds 4 columns of ONE row per tile, the 16 rows of a
  // wave sit in the 16 lanes of a DPP row: four row_shr adds leave the 16-row sum in lane 15 of every row, which
  // parks it in the (now idle) k-loop LDS; after the tile loop 76 threads add the four waves' slices in wave order.
  const bool cs_on = a.colsum_partial != nullptr;
  const float wrow = (cs_on && row_ok) ? a.colsum_w[mc] : 0.f;
  float* const cs_lds = &lds[0][0];                    // [4 waves][BN]
  {
    const bool res_ok = rrow != nullptr;
    const float* rbase = res_ok ? rrow : dummy;
    constexpr int D = 4;
    f32x4 ring[D + 1];
    auto ldres = [&](int tc) {
      const int n = n0 + tc * 16 + nq;
      return ld4(rbase + (n < a.N ? n : 0));
    };
#pragma unroll
    for (int t = 0; t < D; ++t)
      if (t < NT) ring[t] = ldres(t);
#pragma unroll
    for (int tc = 0; tc < NT; ++tc) {
      const int n = n0 + tc * 16 + nq;
      const f32x4 b = *reinterpret_cast<const f32x4*>(bias_s + tc * 16 + nq);
      f32x4 v = acc[tc];
      const f32x4 vb = v + b;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = has_bias ? vb[e] : v[e];
      const f32x4 vr = v + ring[tc % (D + 1)];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = res_ok ? vr[e] : v[e];
      if (tc + D < NT) ring[(tc + D) % (D + 1)] = ldres(tc + D);
      if (prow != nullptr && row_ok && n < a.N) *reinterpret_cast<f32x4*>(prow + n) = v;
      const f32x4 stored = finish(v, n);
      if (cs_on) {
        f32x4 t = stored * wrow;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float x = t[e];
          x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x111, 0xf, 0xf, true));   // row_shr:1
          x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x112, 0xf, 0xf, true));   // row_shr:2
          x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x114, 0xf, 0xf, true));   // row_shr:4
          x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x118, 0xf, 0xf, true));   // row_shr:8
          t[e] = x;
        }
        if (fr == 15) *reinterpret_cast<f32x4*>(cs_lds + wave * BN + tc * 16 + nq) = t;
      }
    }
  }
  if (cs_on) {
    __syncthreads();
    if (tid < BN / 4) {
      const int n = n0 + tid * 4;
      const f32x4 s01 = ld4(cs_lds + tid * 4) + ld4(cs_lds + BN + tid * 4);
      const f32x4 s23 = ld4(cs_lds + 2 * BN + tid * 4) + ld4(cs_lds + 3 * BN + tid * 4);
      if (n < a.N) *reinterpret_cast<f32x4*>(a.colsum_partial + static_cast<int64_t>(blockIdx.x) * a.ld_partial + n) = s01 + s23;
    }
  }
#ifdef RR_TRACE
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  RR_STAMP(3);
#endif
}

template <int NT>
int launch_linear(const LinearParams& P, hipStream_t s, bool fast) {
  const rr_linear_args& a = P.a;
  dim3 grid(static_cast<unsigned>((a.M + BM - 1) / BM), static_cast<unsigned>((a.N + 16 * NT - 1) / (16 * NT)));
  if (fast) {
    if (a.a_mask) linear_fast_kernel<NT, 2><<<grid, THREADS, 0, s>>>(P);
    else if (a.a1_sub) linear_fast_kernel<NT, 1><<<grid, THREADS, 0, s>>>(P);
    else linear_fast_kernel<NT, 0><<<grid, THREADS, 0, s>>>(P);
  } else {
    if (a.a_mask) linear_kernel<NT, 2><<<grid, THREADS, 0, s>>>(P);
    else if (a.a1_sub) linear_kernel<NT, 1><<<grid, THREADS, 0, s>>>(P);
    else linear_kernel<NT, 0><<<grid, THREADS, 0, s>>>(P);
  }
  return rr_launch_status();
}

// C[m, n] = bias[n] + sum_k A[m, k] * W[n, k] for a handful of output columns (the FFN's last layer: N = task_num <= 8,
// models/base_model.py:57): 16 lanes per row, the row in registers, a shuffle tree per output.  The MFMA kernels spend a
// 64-column tile (and ~20 us of fixed cost at one row per molecule) on these one or two columns.
constexpr int RD_MAXK = 1024;                 // 16 lanes x 4 floats x 16 chunks
__global__ void __launch_bounds__(256) linear_rowdot_kernel(const float* __restrict__ a, int64_t lda, int k,
                                                            const float* __restrict__ w, int64_t ldw,
                                                            const float* __restrict__ bias, int64_t M, int N,
                                                            float* __restrict__ c, int64_t ldc) {
  const int l16 = threadIdx.x & 15;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 16 + (threadIdx.x >> 4);
  const bool live = row < M;
  const float* ar = a + (live ? row : 0) * lda;
  f32x4 x[RD_MAXK / 64];
  const int nch = (k + 63) / 64;
#pragma unroll
  for (int i = 0; i < RD_MAXK / 64; ++i) {
    const int kk = i * 64 + l16 * 4;
    x[i] = (i < nch && kk < k) ? *reinterpret_cast<const f32x4*>(ar + kk) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int n = 0; n < N; ++n) {
    const float* wr = w + static_cast<int64_t>(n) * ldw;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < RD_MAXK / 64; ++i) {
      const int kk = i * 64 + l16 * 4;
      if (i < nch && kk < k) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + kk);
        acc += x[i][0] * wv[0];
        acc += x[i][1] * wv[1];
        acc += x[i][2] * wv[2];
        acc += x[i][3] * wv[3];
      }
    }
    acc += __shfl_xor(acc, 8, 16);
    acc += __shfl_xor(acc, 4, 16);
    acc += __shfl_xor(acc, 2, 16);
    acc += __shfl_xor(acc, 1, 16);
    if (live && l16 == 0) c[row * ldc + n] = acc + (bias ? bias[n] : 0.f);
  }
}

}  // namespace

extern "C" {

#ifdef RR_TRACE
int rr_debug_set_trace(unsigned long long* buf) {   // one copy of rr_trace_buf per unit that stamps
  return rr_trace_set_unit(buf) | rr_trace_set_linear_split(buf) | rr_trace_set_wgrad(buf);
}
#endif

int rr_linear_f32(const rr_linear_args* args, rr_stream_t stream) {
  RR_CHECK_ARG(args);
  const rr_linear_args& a = *args;
  RR_CHECK_ARG(a.M >= 0 && a.N >= 1 && a.k1 >= 0 && a.k2 >= 0 && a.k1 + a.k2 >= 1);
  RR_CHECK_ARG(a.w && a.c && a.ldc >= a.N);
  RR_CHECK_ARG(a.w_packed >= 0 && a.w_packed <= 3);
  RR_CHECK_ARG(a.w_packed >= 2 ? rr_aligned16(a.w)
                               : (a.w_packed ? (a.ldw == r16(a.k1) + r16(a.k2) && rr_aligned16(a.w)) : (a.ldw >= a.k1 + a.k2)));
  RR_CHECK_ARG(a.k1 == 0 || (a.a1 && a.lda1 >= a.k1));
  RR_CHECK_ARG(a.k2 == 0 || (a.a2 && a.lda2 >= a.k2));
  RR_CHECK_ARG(!a.a1_sub || (a.k1 > 0 && a.lda1_sub >= a.k1));
  RR_CHECK_ARG(!a.a_mask || (a.k2 == 0 && !a.a1_sub && !a.a1_idx && a.ld_mask >= a.k1));
  RR_CHECK_ARG(!a.residual || a.ldr >= a.N);
  RR_CHECK_ARG(!a.c_pre || a.ld_pre >= a.N);
  RR_CHECK_ARG(!a.dz_out || ((a.a_mask || a.a_mask_bits) && a.ld_dz >= a.k1));
  RR_CHECK_ARG(!a.a_mask_bits || (a.w_packed >= 2 && a.k2 == 0 && !a.a1_sub && !a.a1_idx && a.k1 % 4 == 0));
  RR_CHECK_ARG(!a.mask_bits_out || (a.w_packed >= 2 && a.N % 4 == 0));
  RR_CHECK_ARG(a.act == RR_ACT_NONE || a.act == RR_ACT_RELU);
  RR_CHECK_ARG((!a.c_amax_out && !a.dz_amax_out) || a.w_packed == 3);      // (the two-f16-term kernels' epilogues only)
  RR_CHECK_ARG(!a.dz_amax_out || a.dz_out);
  RR_CHECK_ARG(a.drop_p >= 0.f && a.drop_p < 1.f);
  RR_CHECK_ARG(a.M < (int64_t(1) << 31) * BM);
  if (a.M == 0) return RR_OK;

  const LinearParams P = linear_params(a);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // a handful of output columns off one plain operand, nothing fused (the FFN's last layer): the row-dot kernel
  if (a.N <= 8 && a.w_packed == 1 && a.k2 == 0 && a.k1 % 4 == 0 && a.k1 <= RD_MAXK && (P.flags & F_A1_VEC) && !a.a1_idx && !a.a1_sub &&
      !a.a_mask && !a.a_mask_bits && !a.residual && a.act == RR_ACT_NONE && a.drop_p == 0.f && !a.c_pre && !a.dz_out &&
      !a.colsum_partial && !a.mask_bits_out && !getenv("RR_NO_ROWDOT")) {
    linear_rowdot_kernel<<<static_cast<unsigned>((a.M + 15) / 16), 256, 0, s>>>(a.a1, a.lda1, a.k1, a.w, P.w_k1_off, a.bias, a.M,
                                                                               a.N, a.c, a.ldc);
    return rr_launch_status();
  }
  // fast path: packed W, every present A source 16-byte addressable, vector epilogue
  bool fast = a.w_packed && (P.flags & F_EPI_VEC) && (!a.c_pre || (P.flags & F_PRE_VEC));
  if (a.k1 > 0 && !(P.flags & F_A1_VEC)) fast = false;
  if (a.k2 > 0 && !(P.flags & F_A2_VEC)) fast = false;
  if (a.a1_sub && !(P.flags & F_SUB_VEC)) fast = false;
  if (a.a_mask && !(P.flags & F_MASK_VEC)) fast = false;
  if (a.dz_out) {                                     // side output only exists on the straight-line path
    if (!fast || a.k1 % 4 != 0 || !vec_ok(a.dz_out, a.ld_dz)) return RR_ERR_ALIGN;
  }
  if (a.colsum_partial) {                             // likewise the weighted column-sum side output
    RR_CHECK_ARG(a.colsum_w && a.ld_partial >= a.N);
    if (!fast || !vec_ok(a.colsum_partial, a.ld_partial)) return RR_ERR_ALIGN;
  }
  if (a.w_packed >= 2) {                              // split terms (three bf16 / two f16) only exist in the straight-line geometry
    if (!fast || a.N > 608 || a.M >= (int64_t(1) << 31) * 128) return RR_ERR_ALIGN;
    if (a.dz_accumulate) return RR_ERR_UNSUPPORTED;
    if (a.w_packed == 3) RR_CHECK_ARG((a.k1 == 0 || a.a1_amax) && (a.k2 == 0 || a.a2_amax) && (!a.a1_sub || a.a1_sub_amax));
    return rr_linear_split_launch(args, a.w_packed == 3, stream);      // linear_split.hip
  }
  // Few rows (the FFN head: one row per molecule, 64 row blocks): cut the columns into 64-wide blocks as well, so the
  // launch covers the chip (5 x 64 workgroups at N = 300 instead of 64) - each element's k-order, hence its value, is
  // the same in every geometry.
  if (a.N <= 64 || a.M <= 8192) return launch_linear<4>(P, s, fast);
  if (a.N <= 160) return launch_linear<10>(P, s, fast);
  return launch_linear<19>(P, s, fast);
}

int64_t rr_mask_bits_row_bytes(int N) { return N < 1 ? 0 : mask_bits_row(N); }

int64_t rr_linear_colsum_rows(int64_t M) { return M <= 0 ? 0 : (M + BM - 1) / BM; }

}  // extern "C"
