// The split forward GEMM of rr_linear_f32 (w_packed = 2 / 3): linear_split_kernel and its dispatch.  linear.hip checks the
// request and enters through rr_linear_split_launch.
#include "linear_common.h"
#include <atomic>
#include <type_traits>

namespace {

// ------------------------------------------------------------------------ split path (3 x bf16 terms, 6 products)
// The same GEMM on the bf16 matrix core without giving up f32 accuracy.  Every f32 operand is written EXACTLY as
// the sum of three bf16 terms, x = x0 + x1 + x2 (x0 = bf16(x), x1 = bf16(x - x0), x2 = x - x0 - x1: the two
// remainders are exact in f32 and the last one has at most 8 significant bits left), and
//     x * w  =  x0 w0 + (x0 w1 + x1 w0) + (x0 w2 + x1 w1 + x2 w0)  +  terms below 2^-24 |x w|
// is accumulated in f32 by six v_mfma_f32_16x16x32_bf16 per 32-deep k-step, smallest terms first.  bf16 x bf16
// products are exact in f32, and the sum of a k-step is rounded once instead of after every fmaf, so the error
// against an f64 GEMM is at or BELOW that of the f32 MFMA chain (tests/test_gpu_split.py measures both).  Six bf16
// MFMAs cost 6/16 of the f32 MFMA's cycles for the same k: the kernel moves from MFMA-bound to HBM-bound.
// Fused tail: where the LAST k-step has at most 16 live columns (K = 300: 12; also 12 ... 16 past any multiple of 32, and the
// second segment of 61 | 300) its six products are issued as three MFMAs, two products side by side in the 32 k-slots of one
// instruction: 57 instead of 60 MFMAs per tile and row block at K = 300 (mfma_block).  It is a compile-time property of the
// instantiation - the template flag TF, picked by the host in launch_split_tail, with the last step peeled out of the k-loop -
// because any branch that joins in front of the epilogue with the 76 accumulators live makes hipcc spill hundreds of
// registers.  Three-bf16-term form of <19,19,MODE 0 / 1 / 3,12,EPI 0 / 1> only.  On by default (launch_split_tail;
// measured in profiles/tail_fuse_ab.txt): RR_NO_TAIL_FUSE=1 launches the unfused twins.
//
// Geometry: workgroup = 12 waves x 16 rows = 192 rows x up to 304 output columns; the activation operand goes
// global -> registers (each lane loads the 8 consecutive k of ITS row that the MFMA layout hands it, fixes them up
// - gather / subtract / ReLU mask - and splits them: every element is converted exactly once); the weight terms
// are pre-split by rr_pack_weights (w_packed = 2) into the exact LDS image of a k-step (per column tile and term:
// 64 lanes x 16 B, lane-linear) and stream L2 -> LDS by LDS-DMA, double buffered (2 x 57 KB: one workgroup per CU).
// N > 304 (H = 600): two column blocks of 19 tiles (blockIdx.y), each streaming its own tiles of the image.
#ifndef RR_EPI_MODE
#define RR_EPI_MODE 1
#endif

// The two conditions host and kernel share.  Lean loader: both segments (plus one k-step of slack for the prefetch) fit
// inside rr_zero_row.  Persistent form: the instantiations that carry it (the host adds the per-launch part, launch_split_epi).
__host__ __device__ constexpr bool split_lean(int k1, int k2) { return k1 + SK <= RR_ZERO_ROW && k2 + SK <= RR_ZERO_ROW; }
__host__ __device__ constexpr bool split_can_persist(int NTP, int NT, int MODE, int WAVES, int EPI) {
  return MODE == 0 && WAVES == 12 && NT == NTP && EPI == 0;
}

// Balanced last round (see the kernel): the other one-column-block instantiations of the 12-wave geometry that the model launches.
// The generic-loader twins EPI 2 / 3 (K > 992: no configuration of the model) stay as they were: <19,19,1,12,3> has no register
// to spare for it (waves without rows cost it spilled registers inside the k-loop).
__host__ __device__ constexpr bool split_balanced(int NTP, int NT, int MODE, int WAVES, int EPI, bool F16) {
  return WAVES == 12 && NT == NTP && EPI < 2 && !F16 && !split_can_persist(NTP, NT, MODE, WAVES, EPI);
}

// Fused tail (see mfma_block): the instantiations of the one-column-block 12-wave geometry that the model launches at H = 300
// carry a twin (TF) whose LAST k-step issues three MFMAs per tile instead of six; the host picks it when that step has at most
// 16 live columns (split_tail_live).
__host__ __device__ constexpr bool split_tail_fusable(int NTP, int NT, int MODE, int WAVES, int EPI, bool F16) {
  return WAVES == 12 && NT == NTP && MODE != 2 && EPI < 2 && !F16;
}
// live columns of the last k-step (it belongs to segment 2 when there is one)
__host__ __device__ constexpr int split_tail_live(int k1, int k2) { return k2 > 0 ? k2 - (r32(k2) - SK) : k1 - (r32(k1) - SK); }

// NTP: column tiles of the packed weight image; NT: column tiles of ONE workgroup (blockIdx.y picks tiles y * NT ...);
// WAVES: 16-row groups per workgroup.  Instantiated: <19, 19, 12 waves> - one workgroup per CU (114 KB of LDS) covers all
// columns of 192 rows - and <10, 10, 8> / <4, 4, 8> for narrow layers.  Cutting the 19 tiles into 10 + 9 (<19, 10, 8>:
// 60 KB, <= 128 registers, TWO workgroups per CU whose store epilogues and MFMA loops overlap) was measured and lost:
// both halves load and split the operand rows, 320 vs 236 us on the masked dX GEMM (profiles/r02_experiments.txt).
// EPI: 0 = accumulator-layout epilogue, 1 = row-contiguous epilogue through LDS (12-wave geometry; chosen per launch,
// see launch_split_one: separate instantiations keep each epilogue's registers out of the other's kernel)
// TF: the last k-step is the fused tail (chosen per launch, launch_split_tail): 0 = no, 1 / 2 = yes, for an odd / even number
// of k-steps (the peeled step's operand slot is a compile-time property as well: see the k-loop)
template <int NTP, int NT, int MODE, int WAVES, int EPI = 0, bool F16 = false, int TF = 0>
__global__ void __launch_bounds__(64 * WAVES, WAVES == 8 ? 4 : 3) linear_split_kernel(const LinearParams P) {
  static_assert(TF == 0 || split_tail_fusable(NTP, NT, MODE, WAVES, EPI, F16), "no fused tail for this instantiation");
  constexpr int BN = 16 * NT;
  constexpr int TERMS = F16 ? 2 : 3;                   // operand terms: three bf16 or two f16
  constexpr int PANEL = NT * TERMS * 1024;             // bytes of one k-step's weight image in LDS
  constexpr int SRC_PANEL = NTP * TERMS * 1024;            // ... and in the packed weights
  constexpr int S_THREADS = 64 * WAVES;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // LDS layout.  k-loop: two weight images [0, 2 * PANEL).  Epilogue of the 12-wave geometry (RS_EPI): the images' space
  // becomes twelve wave-private transposition regions of 8 rows x 77 float4 (the 77th is padding: rows 1232 bytes apart
  // keep the eight lanes of a ds_write_b128 group on different banks), followed by the column-sum / sign-bit staging and
  // the bias slice.  The 8-wave geometries keep bias and staging where they were.
  constexpr bool RS_EPI = WAVES == 12;
  constexpr int RS = 77, REGION = 8 * RS * 16;         // bytes per wave and pass
  constexpr int CS_OFF = RS_EPI ? (WAVES * REGION > 2 * PANEL ? WAVES * REGION : 2 * PANEL) : 0;
  constexpr int BIAS_OFF = RS_EPI ? CS_OFF + WAVES * BN * 4 : 2 * PANEL;
  float* const bias_s = reinterpret_cast<float*>(smem + BIAS_OFF);
  constexpr int PF_OFF = BIAS_OFF + BN * 4;            // persistent form: 2 KiB per wave for the next block's step-0 operand chunks
  // Two column blocks (N > 304: <38, 19, ...>): a 1-D grid in which ids i and i + 8 are the two column blocks of ONE row block.
  // Workgroup ids are dealt to the 8 XCDs round-robin, so the pair lands on one XCD within a few dispatches of each other and the
  // second one finds the operand rows in that XCD's L2 (a (rows, 2) grid ran all first column blocks before any second one: every
  // operand row left HBM twice).
  constexpr bool PAIR = NTP == 2 * NT;
  const unsigned int bx = PAIR ? (((blockIdx.x >> 4) << 3) + (blockIdx.x & 7u)) : blockIdx.x;
  // (BALANCED, SHORT: see "Balanced last round" below.  Those launches have one column block: by = 0 folds the column-block
  // arithmetic away, scalar registers the epilogue needs)
  constexpr bool BALANCED = split_balanced(NTP, NT, MODE, WAVES, EPI, F16);
  constexpr bool SHORT = BALANCED || split_can_persist(NTP, NT, MODE, WAVES, EPI);
  const unsigned int by = PAIR ? ((blockIdx.x >> 3) & 1u) : (BALANCED ? 0u : blockIdx.y);
  if (PAIR && static_cast<int64_t>(bx) * (16 * WAVES) >= P.a.M) return;   // (uniform: the grid is padded to whole groups of 16 ids)
  const int t0 = by * NT;                              // first column tile of this workgroup
  const int nth = NTP - t0 < NT ? NTP - t0 : NT;       // its column tiles (the last workgroup of a row block may have fewer)
  const bool full = nth == NT;
  const int n0 = t0 * 16;

  const rr_linear_args& a = P.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fkq = lane >> 4;
  // two-term f16 form: the operand scale from the caller's bounds (uniform: scalar loads), the weight's from its image
  float xs = 1.f, ixs = 1.f, iws = 1.f;
  if (F16) {
    float b1 = (a.a1_amax ? rr_amax_read(a.a1_amax) : 0.f) + (a.a1_sub_amax ? rr_amax_read(a.a1_sub_amax) : 0.f);
    if (MODE == 2 || MODE == 3) b1 *= fabsf(a.mask_scale);
    const float b2 = a.a2_amax ? rr_amax_read(a.a2_amax) : 0.f;
    const float bound = fmaxf(b1, b2);
    const int e = rr_f16_exp(bound);
    xs = bound < 2.5e33f ? rr_pow2(14 - e) : __builtin_nanf("");   // an infinite / > 2^110 element: no scale fits, every output is NaN
    ixs = rr_pow2(e - 14);
    iws = 1.0f / a.w[static_cast<int64_t>(P.t1 + P.t2) * (SRC_PANEL / 4)];   // (a power of two: exact)
  }
  RR_STAMP(0);
#ifdef RR_TRACE
  if (rr_trace_buf && threadIdx.x == 0 && by == 0) {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    rr_trace_buf[static_cast<size_t>(bx) * 8 + 4] = (static_cast<unsigned long long>(xcc) << 32) | hw;
  }
#endif
#ifdef RR_SPLIT_STAGGER
  // experiment: de-phase the workgroups of the first round (equal work + simultaneous start = every CU in its store
  // epilogue at the same time); later workgroups start when an earlier one retires and inherit the offsets
  if (WAVES == 12 && gridDim.x > 256 && blockIdx.x < 256) {
    const int ph = (blockIdx.x >> 3) & 3;
    for (int i = 0; i < ph * RR_SPLIT_STAGGER; ++i) __builtin_amdgcn_s_sleep(127);
  }
#endif
  // Persistent form (plain-operand GEMMs of the 12-wave geometry, chosen by the host: P.persist): gridDim.x = one workgroup
  // per CU, each owning a CONTIGUOUS range of rows - an equal share of the 64-row units, so every CU finishes at the same
  // time - and walking it in blocks of up to 12 waves x 16 rows; the last block of a range has 4 or 8 active waves (one or
  // two per SIMD instead of three: it takes 1/3 or 2/3 of a full block's time, where the one-block-per-workgroup launch
  // pays a whole second round for it).  The k-loop's software pipeline (operand chunks two steps ahead, weight image one
  // step ahead) continues across the block boundary: the last step of a block issues the NEXT block's first weight image
  // (the weights do not depend on the rows), the step before it fetches the next block's step-0 operand chunks, so a
  // block's ~5 us of dependent loads before its first MFMA run under the previous block's last MFMA blocks.  Same values,
  // same order per element: bit-identical to the one-block form.  Rows are counted in groups of 16 (one wave's rows).
  constexpr bool CAN_PERSIST = split_can_persist(NTP, NT, MODE, WAVES, EPI);
  const bool persist = CAN_PERSIST && P.persist != 0;
  // Balanced last round (the other instantiations of the one-workgroup-per-CU geometry, chosen by the host: P.bal_*): still one
  // block per workgroup, but the row blocks behind the last whole round of full ones are cut so that every CU gets an equal
  // share of their 64-row units - blocks of 4 or 8 active waves, where a grid of full blocks ends with a few CUs running
  // twelve waves and the rest idle.  SHORT: the instantiations in which a wave may be without rows (uwave >= nw): it issues
  // its loads - the weight image is dealt over ALL waves, and every wave keeps the same vmcnt sequence - and nothing else.
  // The block's rows travel to the epilogue in ONE scalar register, blk = first 64-row unit << 2 | units (1 .. 3; the host
  // keeps the unit count below 2^29), where the grid of full blocks needed none: these kernels have no scalar to spare.
  // the workgroup's running maxima of |C| / |dz_out| (rr_linear_args.c_amax_out / dz_amax_out): two words behind everything else
  unsigned int* const amx = reinterpret_cast<unsigned int*>(smem + PF_OFF + (CAN_PERSIST ? WAVES * 2048 : 0));
  if (F16 && tid == 0) { amx[0] = 0u; amx[1] = 0u; }    // (the prologue's barrier orders this before any use)
  int64_t g_cur = static_cast<int64_t>(bx) * WAVES;                    // first 16-row group of the current block
  int64_t g_end = g_cur + WAVES;                                        // end of this workgroup's range
  if (persist) {
    const int64_t units = (a.M + 63) / 64, G = gridDim.x;
    const int64_t base = units / G, rem = units % G, p = blockIdx.x;
    g_cur = 4 * (p * base + (p < rem ? p : rem));
    g_end = g_cur + 4 * (base + (p < rem ? 1 : 0));
  }
  int blk = 0;
  if (BALANCED) {
    int u0 = static_cast<int>(blockIdx.x) * (WAVES / 4), nu = WAVES / 4;
    if ((P.bal_base | P.bal_rem) != 0 && static_cast<int>(blockIdx.x) >= P.bal_full) {
      const int q = static_cast<int>(blockIdx.x) - P.bal_full;          // larger tail blocks first
      u0 = P.bal_full * (WAVES / 4) + q * P.bal_base + (q < P.bal_rem ? q : P.bal_rem);
      nu = P.bal_base + (q < P.bal_rem ? 1 : 0);
    }
    blk = (u0 << 2) | nu;
    g_cur = 4 * static_cast<int64_t>(u0);
    g_end = g_cur + 4 * nu;
  }
  int nw = g_end - g_cur < WAVES ? static_cast<int>(g_end - g_cur) : WAVES;   // active waves of the current block (uniform)
  int64_t m0 = g_cur * 16;
  int64_t m = m0 + wave * 16 + fr;
  bool row_ok = wave < nw && m < a.M;
  int64_t mc = row_ok ? m : a.M - 1;
  const float* const dummy = a.w;                      // any valid, 16-byte aligned GLOBAL address (keeps the loads global_load)
  const float* rowp1 = nullptr;
  const float* rowp2 = nullptr;
  const float* subp = nullptr;                         // MODE 1: subtract source, MODE 2: mask source
  const uint8_t* bitrow = nullptr;                     // MODE 3: the mask as one bit per element (rr_linear_args.a_mask_bits)
  {
    const bool g1 = a.k1 > 0 && a.a1_idx != nullptr;
    const bool g2 = MODE == 1 && a.k1 > 0 && a.a1_sub != nullptr && a.a1_sub_idx != nullptr;
    const int32_t j1 = g1 ? ldgi(a.a1_idx + mc) : 0;
    const int32_t j2 = g2 ? ldgi(a.a1_sub_idx + mc) : 0;
    if (row_ok) {
      if (a.k1 > 0) {
        if (g1) {
          if (j1 >= 0) rowp1 = a.a1 + static_cast<int64_t>(j1) * a.lda1;
        } else {
          rowp1 = a.a1 + m * a.lda1;
        }
        if (MODE == 1 && a.a1_sub) {
          if (g2) {
            if (j2 >= 0) subp = a.a1_sub + static_cast<int64_t>(j2) * a.lda1_sub;
          } else {
            subp = a.a1_sub + m * a.lda1_sub;
          }
        }
        if (MODE == 2) subp = a.a_mask + m * a.ld_mask;
        if (MODE == 3) bitrow = a.a_mask_bits + m * mask_bits_row(a.k1);
      }
      if (a.k2 > 0) rowp2 = a.a2 + m * a.lda2;
    }
  }
  float dz_am = 0.f;                                   // largest |dz_out| this lane stored (rr_linear_args.dz_amax_out)
  float* dzrow = nullptr;                              // MODE 2 side output: dz_out (+)= masked operand
  if ((MODE == 2 || MODE == 3) && a.dz_out && row_ok && by == 0) dzrow = a.dz_out + m * a.ld_dz;

  const int uwave = __builtin_amdgcn_readfirstlane(wave);
  const float* const wlane = a.w + t0 * (TERMS * 256) + lane * 4;   // this workgroup's tiles of a step; 16 B per lane inside a 1 KiB block
  const uint32_t lds0 = rr_lds_addr(reinterpret_cast<const float*>(smem));

  f32x4 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) acc[i] = f32x4(0.f);

  const int nk = P.t1 + P.t2;
  // operand chunks in flight: two k-steps (slot = step & 1), so a load has two MFMA blocks to land; the weight image one
  f32x4 ra[WAVES == 12 ? 2 : 1][2], rs[WAVES == 12 ? 2 : 1][2];
  uint32_t rb[2] = {0u, 0u};                           // MODE 3: the 8 mask bits of a step's chunk pair
  u32x4 x0, x1, x2;                                    // the three bf16 terms of the current step's operand

  // Interior k-steps (all 32 columns of the step inside the segment) of MODE 0 / 1 take a leaner path: the lane's row
  // pointers are resolved ONCE (a missing row points at a row of zeros), a step adds its wave-uniform column offset, and
  // fixup() needs no per-element selects.  ~27 of the ~90 vector instructions of a k-step; same loaded values, same
  // arithmetic.  The last step of a segment (partial: K = 300 ends inside it) keeps the select form below.
#ifndef RR_SPLIT_NO_FASTX
  constexpr bool FASTX = (MODE == 0 || MODE == 1);
#else
  constexpr bool FASTX = false;
#endif
  // an interior step reads columns [s*SK, (s+1)*SK) <= k of its row - or of rr_zero_row when the row is missing: the
  // segment (plus one step of slack for the prefetch) must fit inside that array
  static_assert(RR_ZERO_ROW % SK == 0 && RR_ZERO_ROW >= 2 * SK, "rr_zero_row must hold whole k-steps");
  // (the EPI 0 / 1 instantiations of the 12-wave geometry are only launched with segments that fit - launch_split_one sends
  // longer ones to their twins EPI 2 / 3, which keep the generic loader - so their select-per-element loader is dead code:
  // fewer live scalars and pointers in kernels that have none to spare.  Measured on
  // the persistent form <19,19,0,12,0>: 12 -> 2 spilled registers, -3 ... -5 % per launch at 71k rows, -0.7 % on the step)
  constexpr bool LEAN_ONLY = FASTX && WAVES == 12 && EPI < 2;
  const bool fastx_ok = FASTX && (LEAN_ONLY || split_lean(a.k1, a.k2));
  const float* xb1 = (rowp1 != nullptr ? rowp1 : rr_zero_row) + fkq * 8;
  const float* xb2 = (rowp2 != nullptr ? rowp2 : rr_zero_row) + fkq * 8;
  const float* const sb1 = (subp != nullptr ? subp : rr_zero_row) + fkq * 8;
  const float* xb1n = xb1;                             // persistent form: the NEXT row block's operand rows
  const float* xb2n = xb2;
  bool has_next = false, wrapped = false;              // wrapped: this block was entered from the previous block's pipeline
  auto next_rows = [&](int64_t g, int nwn) {           // MODE 0 only: plain or index-gathered segment 1, plain segment 2
    const int64_t mm = (g + wave) * 16 + fr;
    const bool ok = wave < nwn && mm < a.M;
    const int64_t mmc = ok ? mm : a.M - 1;
    const bool g1 = a.k1 > 0 && a.a1_idx != nullptr;
    const int32_t j1 = g1 ? ldgi(a.a1_idx + mmc) : 0;
    const float* r1 = nullptr;
    const float* r2 = nullptr;
    if (ok) {
      if (a.k1 > 0) {
        if (g1) {
          if (j1 >= 0) r1 = a.a1 + static_cast<int64_t>(j1) * a.lda1;
        } else {
          r1 = a.a1 + mm * a.lda1;
        }
      }
      if (a.k2 > 0) r2 = a.a2 + mm * a.lda2;
    }
    xb1n = (r1 != nullptr ? r1 : rr_zero_row) + fkq * 8;
    xb2n = (r2 != nullptr ? r2 : rr_zero_row) + fkq * 8;
  };
  auto interior = [&](int s) -> bool {                 // (wave-uniform)
    if (!fastx_ok) return false;
    return s < P.t1 ? (s + 1) * SK <= a.k1 : (s - P.t1 + 1) * SK <= a.k2;
  };
  auto issue_x = [&](int s, int slot, bool nextblk = false) {   // pure loads (unconditional, from a selected address)
    if (FASTX && fastx_ok) {
      const bool s1 = s < P.t1;
      const int off = (s1 ? s : s - P.t1) * SK;          // wave-uniform
      const float* p = (s1 ? (nextblk ? xb1n : xb1) : (nextblk ? xb2n : xb2)) + off;
      const float* q = (MODE == 1 && s1) ? sb1 + off : rr_zero_row;   // (segment 2 has no subtract source: zeros, the count of loads per step stays NX)
      if (interior(s)) {
        ra[slot][0] = ldg4(p);
        ra[slot][1] = ldg4(p + 4);
        if (MODE == 1) {
          rs[slot][0] = ldg4(q);
          rs[slot][1] = ldg4(q + 4);
        }
      } else {                                         // last step of a segment: chunks past its end read zeros
        int fq = fkq;                                  // (opaque: these selects are per-lane loop invariants - left alone they are
        if (CAN_PERSIST) asm volatile("" : "+v"(fq));  // hoisted out of the block loop, kept live across the k-loop and spilled)
        const int kl = off + fq * 8, ks = s1 ? a.k1 : a.k2;
        ra[slot][0] = ldg4(kl < ks ? p : rr_zero_row);
        ra[slot][1] = ldg4(kl + 4 < ks ? p + 4 : rr_zero_row);
        if (MODE == 1) {
          rs[slot][0] = ldg4(kl < ks ? q : rr_zero_row);
          rs[slot][1] = ldg4(kl + 4 < ks ? q + 4 : rr_zero_row);
        }
      }
      return;
    }
    const bool seg1 = s < P.t1;
    const int kl = (seg1 ? s : s - P.t1) * SK + fkq * 8;
    const float* p = seg1 ? rowp1 : rowp2;
    const int ks = seg1 ? a.k1 : a.k2;
    ra[slot][0] = ldg4((p != nullptr && kl < ks) ? p + kl : dummy);
    ra[slot][1] = ldg4((p != nullptr && kl + 4 < ks) ? p + kl + 4 : dummy);
    if (MODE == 1 || MODE == 2) {
      const bool oks = seg1 && subp != nullptr;
      rs[slot][0] = ldg4((oks && kl < ks) ? subp + kl : dummy);
      rs[slot][1] = ldg4((oks && kl + 4 < ks) ? subp + kl + 4 : dummy);
    }
    if (MODE == 3) {                                   // byte (column block, half tile, tile) holds k = kl .. kl+7, bit e <-> kl + e
      const int tc = 2 * s + (fkq >> 1);
      const int y = tc / 19;
      const uint8_t* q = bitrow + y * 40 + (fkq & 1) * 20 + (tc - 19 * y);
      rb[slot] = ldgb((seg1 && bitrow != nullptr && kl < ks) ? q : reinterpret_cast<const uint8_t*>(dummy));
    }
  };
  auto issue_w = [&](int s) {                          // weight image of step s: NT * 3 LDS-DMA blocks of 1 KiB over the waves
    int so = s;                                        // (opaque in the TF twins: with the last step peeled, hipcc hoists the per-lane
    if (TF != 0) asm volatile("" : "+s"(so));          // addresses of the constant steps out of the block loop and spills them, 34 registers)
    const float* src = wlane + static_cast<int64_t>(so) * (SRC_PANEL / 4);
    const uint32_t dst = lds0 + (s & 1) * PANEL;
#pragma unroll
    for (int b0 = 0; b0 < NT * TERMS; b0 += WAVES) {
      const int b = b0 + uwave;
      if (b < nth * TERMS) rr_glds16(src + b * 256, dst + b * 1024);
    }
  };
  auto split8 = [&](const f32x4& v0, const f32x4& v1) {
    uint32_t t0, t1, t2;
    if (F16) {
      split_pair_h(v0.x, v0.y, xs, t0, t1); x0.x = t0; x1.x = t1;
      split_pair_h(v0.z, v0.w, xs, t0, t1); x0.y = t0; x1.y = t1;
      split_pair_h(v1.x, v1.y, xs, t0, t1); x0.z = t0; x1.z = t1;
      split_pair_h(v1.z, v1.w, xs, t0, t1); x0.w = t0; x1.w = t1;
      return;
    }
    split_pair(v0.x, v0.y, t0, t1, t2); x0.x = t0; x1.x = t1; x2.x = t2;
    split_pair(v0.z, v0.w, t0, t1, t2); x0.y = t0; x1.y = t1; x2.y = t2;
    split_pair(v1.x, v1.y, t0, t1, t2); x0.z = t0; x1.z = t1; x2.z = t2;
    split_pair(v1.z, v1.w, t0, t1, t2); x0.w = t0; x1.w = t1; x2.w = t2;
  };
  auto fixup = [&](int s, int slot) {                  // first use of the loads: selects, mask / subtract, split
    if (SHORT && uwave >= nw) return;                   // (its loads are still issued: every wave keeps the same vmcnt sequence)
    if (FASTX && fastx_ok) {
      f32x4 v0 = ra[slot][0], v1 = ra[slot][1];
      f32x4 u0 = f32x4(0.f), u1 = f32x4(0.f);
      if (MODE == 1) { u0 = rs[slot][0]; u1 = rs[slot][1]; }
      const bool s1 = s < P.t1;
      const int ks = s1 ? a.k1 : a.k2;
      if (!interior(s) && (ks & 3) != 0) {             // a 16-byte chunk that straddles the segment's end: per element
        const int kl = (s1 ? s : s - P.t1) * SK + fkq * 8;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v0[e] = kl + e < ks ? v0[e] : 0.f;
          v1[e] = kl + 4 + e < ks ? v1[e] : 0.f;
          if (MODE == 1) {
            u0[e] = kl + e < ks ? u0[e] : 0.f;
            u1[e] = kl + 4 + e < ks ? u1[e] : 0.f;
          }
        }
      }
      if (MODE == 1) {
        v0 = v0 - u0;
        v1 = v1 - u1;
      }
      split8(v0, v1);
      return;
    }
    const bool seg1 = s < P.t1;
    const int kl = (seg1 ? s : s - P.t1) * SK + fkq * 8;
    const float* p = seg1 ? rowp1 : rowp2;
    const int ks = seg1 ? a.k1 : a.k2;
    const bool ok = (p != nullptr);
    f32x4 v0, v1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v0[e] = (ok && kl + e < ks) ? ra[slot][0][e] : 0.f;
      v1[e] = (ok && kl + 4 + e < ks) ? ra[slot][1][e] : 0.f;
    }
    if (MODE == 1) {
      const bool oks = seg1 && (subp != nullptr);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v0[e] -= (oks && kl + e < ks) ? rs[slot][0][e] : 0.f;
        v1[e] -= (oks && kl + 4 + e < ks) ? rs[slot][1][e] : 0.f;
      }
    }
    if (MODE == 2) {
      const bool oks = seg1 && (subp != nullptr);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v0[e] = (oks && kl + e < ks && rs[slot][0][e] > 0.f) ? v0[e] * a.mask_scale : 0.f;
        v1[e] = (oks && kl + 4 + e < ks && rs[slot][1][e] > 0.f) ? v1[e] * a.mask_scale : 0.f;
      }
    }
    if (MODE == 3) {
      const bool oks = seg1 && (bitrow != nullptr);
      const uint32_t bits = rb[slot];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v0[e] = (oks && kl + e < ks && ((bits >> e) & 1u)) ? v0[e] * a.mask_scale : 0.f;
        v1[e] = (oks && kl + 4 + e < ks && ((bits >> (4 + e)) & 1u)) ? v1[e] * a.mask_scale : 0.f;
      }
    }
    split8(v0, v1);
    if (MODE == 2 || MODE == 3) {                      // side output (k1 % 4 == 0: chunks are whole).  Stored HERE, after the
      if (dzrow != nullptr && seg1) {                  // step's load wait: the store then has the whole next MFMA block to retire
        if (kl < ks) { *reinterpret_cast<f32x4*>(dzrow + kl) = v0; if (F16) dz_am = rr_amax4(dz_am, v0); }
        if (kl + 4 < ks) { *reinterpret_cast<f32x4*>(dzrow + kl + 4) = v1; if (F16) dz_am = rr_amax4(dz_am, v1); }
      }
    }
  };
  // Fused tail.  K = 300 is 9.4 k-steps: the last one has 12 live columns, all of them in the k-slots of lanes 0-31 (a lane
  // holds k = (lane >> 4) * 8 ...), and lanes 32-63 of all six operands hold zeros.  An MFMA sums over its 32 k-slots
  // whatever they hold, so with the first operand [w_a (k 0..15) | w_b (k 0..15)] and the second [x_c (k 0..15) | x_d (k 0..15)]
  // ONE instruction adds w_a x_c + w_b x_d, and a last step with at most 16 live columns needs three MFMAs per tile,
  //     c += [w2|w1].[x0|x1]      c += [w0|w1].[x2|x0]      c += [w0|w0].[x1|x0]        (smallest terms first, as in every step)
  // instead of six: 57 instead of 60 MFMAs per tile and row block at K = 300.  The two products of an instruction are summed
  // unrounded where the six-MFMA step rounds after each: the last bits may differ from the unfused kernel's (the error
  // against f64 cannot grow).  Neither operand has another layout for it: the weight operand is a ds_read_b128 of the same
  // image with another per-lane address - lanes 0-31 their own slot of term a's block, lanes 32-63 slot lane - 32 of term
  // b's - and the activation operand is one v_permlane32_swap per register, 12 per wave and step, reused over all tiles.
  // FUSED is a compile-time argument of the peeled last step: a uniform branch here (live <= 16) makes every 12-wave
  // instantiation spill 200-300 registers - the 76 accumulators cross the join.
  auto mfma_block = [&](int s, auto fused) {
    if (SHORT && uwave >= nw) return;                   // (uniform) a wave without rows in a short last block: no MFMAs, no LDS reads
    if constexpr (decltype(fused)::value) {
      auto halves = [](const u32x4& lo, const u32x4& hi) {   // [lo lanes 0-31 | hi lanes 0-31]
        u32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = __builtin_amdgcn_permlane32_swap(lo[e], hi[e], false, false)[0];
        return as_bf16x8(r);
      };
      const bf16x8 g1 = halves(x0, x1), g2 = halves(x2, x0), g3 = halves(x1, x0);
      const u32x4* const Wc = reinterpret_cast<const u32x4*>(smem + (s & 1) * PANEL) + (lane & 31);   // [w0|w0]
      const u32x4* const Wb = Wc + (lane & 32) * 2;                                                   // [w0|w1]
      const u32x4* const Wa = Wc + 128 - (lane & 32) * 2;                                             // [w2|w1]
      u32x4 wa = Wa[0], wb = Wb[0], wc = Wc[0];
      __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const bf16x8 f1 = as_bf16x8(wa), f2 = as_bf16x8(wb), f3 = as_bf16x8(wc);
        if (j + 1 < NT) {
          wa = Wa[(j + 1) * 192];
          wb = Wb[(j + 1) * 192];
          wc = Wc[(j + 1) * 192];
        }
        f32x4 c = acc[j];
        if (j + 1 == NT && NT != NTP && !full) continue;  // (uniform) the narrower last column block has no tile NT-1
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f1, g1, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f2, g2, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f3, g3, c, 0, 0, 0);
        acc[j] = c;
        if (j + 1 < NT) __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
      }
      return;
    }
    const u32x4* Ws = reinterpret_cast<const u32x4*>(smem + (s & 1) * PANEL) + lane;
    if constexpr (F16) {
      const f16x8 h0 = as_f16x8(x0), h1 = as_f16x8(x1);
      u32x4 wa = Ws[0], wb = Ws[64];
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const f16x8 w0 = as_f16x8(wa), w1 = as_f16x8(wb);
        if (j + 1 < NT) {
          wa = Ws[((j + 1) * 2 + 0) * 64];
          wb = Ws[((j + 1) * 2 + 1) * 64];
        }
        f32x4 c = acc[j];
        if (j + 1 == NT && NT != NTP && !full) continue;
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1, h0, c, 0, 0, 0);   // smallest terms first
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0, h1, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0, h0, c, 0, 0, 0);
        acc[j] = c;
        if (j + 1 < NT) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
      }
      return;
    }
    const bf16x8 b0 = as_bf16x8(x0), b1 = as_bf16x8(x1), b2 = as_bf16x8(x2);
    // the three weight terms of tile j+1 are read while the six MFMAs of tile j run (pinned with sched_group_barrier:
    // left alone, the scheduler issues each ds_read right in front of its first use and waits for it)
    u32x4 wa = Ws[0], wb = Ws[64], wc = Ws[128];
    __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const bf16x8 w0 = as_bf16x8(wa), w1 = as_bf16x8(wb), w2 = as_bf16x8(wc);
      if (j + 1 < NT) {
        wa = Ws[((j + 1) * 3 + 0) * 64];
        wb = Ws[((j + 1) * 3 + 1) * 64];
        wc = Ws[((j + 1) * 3 + 2) * 64];
      }
      f32x4 c = acc[j];
      if (j + 1 == NT && NT != NTP && !full) continue;  // (uniform) the narrower last column block has no tile NT-1
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2, b0, c, 0, 0, 0);   // smallest terms first
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, b1, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, b2, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, b0, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, b1, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, b0, c, 0, 0, 0);
      acc[j] = c;
      if (j + 1 < NT) __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
    }
  };
  // one k-step with compile-time slots.  vmcnt retires in issue order: the operand loads of step s+2 are issued AFTER the
  // weight image of step s+1, so "all but the youngest NX" = image landed, step s+1's chunks landed, step s+2's in flight.
  constexpr int NX = MODE == 0 ? 2 : (MODE == 3 ? 3 : 4);   // vector-memory instructions of one issue_x
  constexpr bool DEEP = WAVES == 12;                   // the 8-wave geometries (several workgroups per CU, <= 128 registers): one step ahead
  // Waves of the second half ("late") split their operand at the START of the step that consumes it, the first half at
  // the END of the step before: between two barriers every wave runs the same program, so without this all three waves of
  // a SIMD finish their MFMA blocks together and then run their ~150 VALU instructions of fixup() together, matrix pipe
  // idle (measured: 79 k shader cycles per 10 k-steps against 54.7 k of MFMA issue).  De-phased, one half's VALU runs
  // beside the other half's MFMAs.  Same values in the same order: only WHEN a wave converts its operand changes.
#ifdef RR_SPLIT_NO_LATE
  const bool late = false;
#else
  const bool late = DEEP && uwave >= WAVES / 2;
#endif
  // persistent form: step 0 of the NEXT row block, fetched by LDS-DMA into this wave's 2 KiB (lane-linear 16-byte slots:
  // chunk pair A | B) - no register crosses the store epilogue for it.  Same addresses as issue_x(0, .) would read.
  auto prefetch_next0 = [&]() {
    next_rows(g_cur + nw, g_end - (g_cur + nw) < WAVES ? static_cast<int>(g_end - (g_cur + nw)) : WAVES);   // (recomputed at the block switch: not live across the k-loop)
    const bool s1 = 0 < P.t1;
    const float* p = s1 ? xb1n : xb2n;
    const uint32_t dst = lds0 + PF_OFF + uwave * 2048;
    if (interior(0)) {
      rr_glds16(p, dst);
      rr_glds16(p + 4, dst + 1024);
    } else {
      int fq = fkq;
      asm volatile("" : "+v"(fq));                     // (see issue_x)
      const int kl = fq * 8, ks = s1 ? a.k1 : a.k2;
      rr_glds16(kl < ks ? p : rr_zero_row, dst);
      rr_glds16(kl + 4 < ks ? p + 4 : rr_zero_row, dst + 1024);
    }
  };
  // (last: the peeled last step of a TF instantiation, s == nk - 1 - its MFMA block is the fused one)
  auto step = [&](int s, int slot, auto last) {
    constexpr bool LAST = decltype(last)::value;
    const bool more = !LAST && s + 1 < nk, more2 = !LAST && s + 2 < nk;
    const bool wrap = CAN_PERSIST && has_next;         // (uniform) the pipeline runs on into the next row block; nk is even
    // (step 0 of a block entered through the wrap below finds its operand already split by EVERY wave: one register
    // set - x0..x2 - crosses the store epilogue instead of two)
    if (late && !(CAN_PERSIST && s == 0 && wrapped)) fixup(s, DEEP ? slot : 0);
    if (more) issue_w(s + 1);
    else if (wrap) issue_w(0);                         // next block's first image: buffer 0, last read in step nk - 2
    if (DEEP) {
      if (more2) issue_x(s + 2, slot);
      else if (wrap && more) prefetch_next0();         // s = nk - 2: the next block's step-0 chunks go to LDS, not to registers
    } else {
      if (more) issue_x(s + 1, 0);
    }
    mfma_block(s, last);
    if (DEEP && (more2 || (wrap && more))) {           // (the two prefetch DMAs stand in for an issue_x: same count)
      if (NX == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      else if (NX == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
      rr_wait_vm0();
    }
    if (more && !late) fixup(s + 1, DEEP ? slot ^ 1 : 0);
    __syncthreads();
  };

  if (tid < BN / 4) {
    const int n = n0 + tid * 4;
    *reinterpret_cast<f32x4*>(bias_s + tid * 4) = ldg4((a.bias && n < a.N) ? a.bias + n : dummy);
  }
  issue_w(0);
  issue_x(0, 0);
  if (DEEP && nk > 1) issue_x(1, 1);
  rr_wait_vm0();
  if (!late) fixup(0, 0);
  __syncthreads();
  RR_STAMP(1);

  for (;;) {                                            // one pass per row block (a single pass unless persistent)
  if (CAN_PERSIST) {
    has_next = persist && g_cur + nw < g_end;
  }
  if constexpr (TF != 0) {                              // the last step peeled out of the pairs: its MFMA block is another.  Its
    int s = 0;                                          // slot (nk odd / even) is the instantiation's too: a branch on nk here joins
    for (; s + (TF == 1 ? 1 : 2) < nk; s += 2) {        // in front of the epilogue and costs 140 ... 280 spilled registers
      step(s, 0, std::false_type{});
      step(s + 1, 1, std::false_type{});
    }
    if constexpr (TF == 1) {
      step(s, 0, std::true_type{});
    } else {
      step(s, 0, std::false_type{});
      step(s + 1, 1, std::true_type{});
    }
  } else {
    for (int s = 0; s < nk; s += 2) {
      step(s, 0, std::false_type{});
      if (s + 1 < nk) step(s + 1, 1, std::false_type{});
    }
  }
  RR_STAMP(2);

  // ---- epilogue: the accumulator layout is that of linear_fast_kernel (a lane holds 4 consecutive columns of one row)
  // (persistent form: the lane id goes through an opaque asm per row block, so the epilogue's lane-derived offsets and
  // addresses are recomputed here - a few VALU instructions - instead of being hoisted out of the block loop, kept live
  // across the k-loop and spilled: 70 spilled registers / +60 MB of scratch writes per launch without this)
  if (F16) {                                           // back from the scaled operands: two exact powers of two (one product
#pragma unroll                                          // of them could leave the f32 exponent range where the result does not)
    for (int i = 0; i < NT; ++i) acc[i] = (acc[i] * ixs) * iws;
  }
  int lane_o = threadIdx.x;
#ifndef RR_PERSIST_HOIST
  if (CAN_PERSIST) asm volatile("" : "+v"(lane_o));
#endif
  const int tid = lane_o, lane = lane_o & 63, wave = lane_o >> 6;
  const int fr = lane & 15, fkq = lane >> 4;
  // this block's rows, from the (uniform) block index: nothing row-specific is carried through the k-loop in registers
  int blk_o = blk;
  if (BALANCED) asm volatile("" : "+s"(blk_o));        // (decoded HERE, not ahead of the k-loop)
  const int64_t gb = BALANCED ? 4 * static_cast<int64_t>(blk_o >> 2) : g_cur;   // first 16-row group and active waves of this block
  const int nwb = BALANCED ? 4 * (blk_o & 3) : nw;
  const int64_t m0 = gb * 16;
  const int64_t m = m0 + wave * 16 + fr;
  const bool row_ok = wave < nwb && m < a.M;
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
  float c_am = 0.f;                                    // largest |C| this lane stored (rr_linear_args.c_amax_out)
  auto finish = [&](f32x4 v, int n) -> f32x4 {
    if (relu) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
    }
    if (P.drop_thr != 0u) {
      const uint64_t base = static_cast<uint64_t>(m) * static_cast<uint64_t>(a.N) + static_cast<uint64_t>(n);
      const uint32_t w = rr_hash_group(a.drop_seed, base >> 2);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = rr_hash_lane(w, e) >= P.drop_thr ? v[e] * P.keep_scale : 0.f;
    }
    if (row_ok && n < a.N) {
      *reinterpret_cast<f32x4*>(crow + n) = v;
      if (F16) c_am = rr_amax4(c_am, v);
    }
    return v;
  };
  float* prow = a.c_pre ? a.c_pre + mc * a.ld_pre : nullptr;
  // optional fourth output: sign bits of what was stored (the mask a later dX GEMM needs: 1 bit instead of 4 bytes).
  // A lane holds 4 columns of a tile; lanes fkq and fkq^1 (16 lanes apart) make a byte = 8 consecutive columns, the
  // even one collects its 19 bytes in 5 registers and stores them once.
  const bool mb_on = a.mask_bits_out != nullptr;
  uint32_t mb[5] = {0u, 0u, 0u, 0u, 0u};
  const bool cs_on = a.colsum_partial != nullptr;
  const float wrow = (cs_on && row_ok) ? a.colsum_w[mc] : 0.f;
  float* const cs_lds = reinterpret_cast<float*>(smem + CS_OFF);    // [waves][BN] (8-wave geometries: the now idle weight image)
  // ---- row-contiguous epilogue (12-wave geometry).  In the accumulator layout a 16-lane group holds 16 ROWS x 16 bytes:
  // every global_load / global_store of the epilogue touches 64 different 128-byte lines for 1 KiB of payload, and the
  // address coalescer - not HBM - sets its time (measured: 10.8 us per 192-row block for the plain store epilogue, 21 us
  // with the residual read; a de-phased start of the workgroups changed nothing).  So the tile goes through LDS once: the
  // accumulators are written in their own layout, read back lane-linear (a lane = 4 consecutive columns of a row, 64 lanes
  // = 1 KiB of consecutive memory where ldc == N) and everything after the GEMM - bias, residual, ReLU, dropout, second
  // output, sign bits, the store - happens in that layout with fully coalesced accesses.  Same operations in the same
  // order per element, so the stored values are those of the accumulator-layout epilogue bit for bit.  The weighted
  // column sums (dX GEMMs: no bias / residual / activation) are taken from the accumulators before the transposition;
  // the rare combination of column sums WITH epilogue arithmetic keeps the accumulator-layout code below.
  const bool plain_epi = !has_bias && a.residual == nullptr && !relu && P.drop_thr == 0u && prow == nullptr && !mb_on;
  // (a wave without rows of a balanced launch has nothing to finish, store or sum: it goes on to the barriers below.  The
  // persistent form walks both epilogues with row_ok false, as it did)
  const bool idle = BALANCED && uwave >= nwb;
  bool done = idle;
  if (!idle && RS_EPI && (EPI & 1) == 1 && (!cs_on || plain_epi)) {
    done = true;
    if (cs_on) {
#pragma unroll
      for (int tc = 0; tc < NT; ++tc) {
        f32x4 t = acc[tc] * wrow;
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
    unsigned char* const region = smem + uwave * REGION;
    unsigned char* const bits_s = smem + CS_OFF + uwave * 640;       // [16 rows][40 bytes] (never together with column sums)
    if (mb_on) {                                                     // the two pad bytes of a row stay zero
#pragma unroll
      for (int d = lane; d < 160; d += 64) reinterpret_cast<uint32_t*>(bits_s)[d] = 0u;
    }
    const int nqv = (a.N - n0) / 4 < 4 * NT ? (a.N - n0) / 4 : 4 * NT;   // valid float4 columns of this column block
    const int64_t mw = m0 + uwave * 16;
    const bool res_on = a.residual != nullptr;
    constexpr int NI = (8 * 76 + 63) / 64;                           // lane-linear float4 reads per pass (76 per row, 8 rows)
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      if ((fr >> 3) == pass) {
#pragma unroll
        for (int tc = 0; tc < NT; ++tc)
          *reinterpret_cast<f32x4*>(region + (((fr & 7) * RS + tc * 4 + fkq) << 4)) = acc[tc];
      }
      // (wave-private region: a wave's LDS operations execute in order, no barrier)
      // lane-linear reads in groups of RG: the group's residual chunks are in flight together, then the group is finished
      // (all NI at once would need 40 registers next to the 76 accumulators that stay live until pass 1 is written)
      constexpr int RG = 2;
#pragma unroll
      for (int i0 = 0; i0 < NI; i0 += RG) {
        asm volatile("" ::: "memory");
        f32x4 rres[RG];
#pragma unroll
        for (int u = 0; u < RG; ++u) {
          const int i = i0 + u;
          if (i < NI && res_on) {
            const int q = (64 * i) / 76, rem = (64 * i) % 76;
            const bool wrap = rem + lane >= 76;
            const int r = q + (wrap ? 1 : 0), c4 = rem + lane - (wrap ? 76 : 0);
            const int64_t mm = mw + pass * 8 + r;
            const bool ok = (64 * i + lane < 8 * 76) && c4 < nqv && mm < a.M;
            const int64_t mmc = ok ? mm : 0;
            const int64_t rr = a.residual_idx ? static_cast<int64_t>(ldgi(a.residual_idx + mmc)) : mmc;
            rres[u] = ldg4((ok && rr >= 0) ? a.residual + rr * a.ldr + n0 + 4 * c4 : rr_zero_chunk);
          }
        }
#pragma unroll
        for (int u = 0; u < RG; ++u) {
          const int i = i0 + u;
          if (i >= NI) continue;
          const int q = (64 * i) / 76, rem = (64 * i) % 76;
          const bool wrap = rem + lane >= 76;
          const int r = q + (wrap ? 1 : 0), c4 = rem + lane - (wrap ? 76 : 0);
          const int64_t mm = mw + pass * 8 + r;
          const bool ok = (64 * i + lane < 8 * 76) && c4 < nqv && mm < a.M;
          const int n = n0 + 4 * c4;
          f32x4 v = *reinterpret_cast<const f32x4*>(region + ((r * RS + c4) << 4));
          if (has_bias) v = v + *reinterpret_cast<const f32x4*>(bias_s + 4 * (c4 < 4 * NT ? c4 : 0));
          if (res_on) v = v + rres[u];
          if (prow != nullptr && ok) *reinterpret_cast<f32x4*>(a.c_pre + mm * a.ld_pre + n) = v;
          if (relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
          }
          if (P.drop_thr != 0u) {
            const uint64_t base = static_cast<uint64_t>(mm) * static_cast<uint64_t>(a.N) + static_cast<uint64_t>(n);
            const uint32_t w = rr_hash_group(a.drop_seed, base >> 2);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = rr_hash_lane(w, e) >= P.drop_thr ? v[e] * P.keep_scale : 0.f;
          }
          if (ok) {
            *reinterpret_cast<f32x4*>(a.c + mm * a.ldc + n) = v;
            if (F16) c_am = rr_amax4(c_am, v);
          }
          if (mb_on) {                                               // lanes l, l^1 hold the two halves of 8 consecutive columns
            uint32_t nib = (v.x > 0.f ? 1u : 0u) | (v.y > 0.f ? 2u : 0u) | (v.z > 0.f ? 4u : 0u) | (v.w > 0.f ? 8u : 0u);
            if (c4 >= nqv) nib = 0u;                                  // columns past N: zero bits
            const uint32_t other = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute((lane ^ 1) << 2, static_cast<int>(nib)));
            const int j = c4 >> 1;                                   // columns 8j .. 8j+7: tile j/2, half j&1
            if ((c4 & 1) == 0 && 64 * i + lane < 8 * 76 && c4 < 4 * NT)
              bits_s[(pass * 8 + r) * 40 + (j & 1) * 20 + (j >> 1)] = static_cast<uint8_t>(nib | (other << 4));
          }
        }
      }
    }
    if (mb_on) {                                                     // 16 rows x 10 dwords, coalesced
      const int64_t rowb = mask_bits_row(a.N);
#pragma unroll
      for (int d = lane; d < 160; d += 64) {
        const int r = d / 10, w = d - 10 * r;
        if (mw + r < a.M)
          *reinterpret_cast<uint32_t*>(a.mask_bits_out + (mw + r) * rowb + by * 40 + 4 * w) = reinterpret_cast<const uint32_t*>(bits_s)[d];
      }
    }
  }
  if (!done) {
    // (with RR_EPI_MODE 1 the 12-wave forward forms that carry a residual take the row-contiguous epilogue above: this
    // instantiation then never sees one, and its register ring is not needed)
    constexpr bool MAY_RES = !(RR_EPI_MODE == 1 && WAVES == 12 && (MODE == 0 || MODE == 1) && (EPI & 1) == 0);
    const bool res_ok = MAY_RES && rrow != nullptr;
    const float* rbase = res_ok ? rrow : dummy;
    constexpr int D = MAY_RES ? 4 : 0;
    f32x4 ring[D + 1];
    auto ldres = [&](int tc) {
      const int n = n0 + tc * 16 + nq;
      return ldg4(rbase + ((res_ok && n < a.N) ? n : 0));
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
      if (MAY_RES) {
        const f32x4 vr = v + ring[tc % (D + 1)];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = res_ok ? vr[e] : v[e];
        if (tc + D < NT) ring[(tc + D) % (D + 1)] = ldres(tc + D);
      }
      if (prow != nullptr && row_ok && n < a.N) *reinterpret_cast<f32x4*>(prow + n) = v;
      const f32x4 stored = finish(v, n);
      if (mb_on) {
        const uint32_t nib = (stored.x > 0.f ? 1u : 0u) | (stored.y > 0.f ? 2u : 0u) | (stored.z > 0.f ? 4u : 0u) | (stored.w > 0.f ? 8u : 0u);
        const uint32_t other = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute((lane ^ 16) << 2, static_cast<int>(nib)));
        if (NT == 19) {
          mb[tc >> 2] |= (nib | (other << 4)) << (8 * (tc & 3));
        } else if (row_ok && (fkq & 1) == 0 && (full || tc + 1 < NT)) {       // narrow column blocks: one byte store per tile
          const int tg = t0 + tc;
          a.mask_bits_out[m * mask_bits_row(a.N) + (tg / 19) * 40 + (fkq >> 1) * 20 + (tg % 19)] =
              static_cast<uint8_t>(nib | (other << 4));
        }
      }
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
  if (!done && NT == 19 && mb_on && row_ok && (fkq & 1) == 0) {
    uint32_t* d = reinterpret_cast<uint32_t*>(a.mask_bits_out + m * mask_bits_row(a.N) + by * 40 + (fkq >> 1) * 20);
#pragma unroll
    for (int i = 0; i < 5; ++i) d[i] = mb[i];
  }
  // (the magnitude outputs exist in the two-f16-term instantiations only: the three-term kernels keep their registers)
  if (F16 && a.c_amax_out != nullptr) rr_amax_commit_wave(c_am, amx);
  if (F16 && (MODE == 2 || MODE == 3) && a.dz_amax_out != nullptr && by == 0) {
    rr_amax_commit_wave(dz_am, amx + 1);
    dz_am = 0.f;
  }
  if (cs_on) {                                         // one partial row per 64 rows (rr_linear_colsum_rows) = per 4 waves
    __syncthreads();
    static_assert(WAVES % 4 == 0 && (WAVES / 4) * (BN / 4) <= S_THREADS, "colsum slices");
    if (tid < (WAVES / 4) * (BN / 4)) {
      const int h = tid / (BN / 4);
      const int q = tid - h * (BN / 4);
      const int n = n0 + q * 4;
      const float* base = cs_lds + h * 4 * BN + q * 4;
      const f32x4 s01 = ld4(base) + ld4(base + BN);
      const f32x4 s23 = ld4(base + 2 * BN) + ld4(base + 3 * BN);
      if (n < a.N && h * 4 < nwb && m0 + h * 64 < a.M)    // (one partial row per 64-row unit; a short last block owns fewer)
        *reinterpret_cast<f32x4*>(a.colsum_partial + (gb / 4 + h) * a.ld_partial + n) = s01 + s23;
    }
  }
  if (!(CAN_PERSIST && has_next)) break;
  // next row block: its step-0 operand is split (early waves) or loaded (late waves), its step-1 chunks are in flight, its
  // first weight image is in LDS buffer 0 - the state the prologue leaves behind
  if (cs_on) __syncthreads();                          // the column-sum staging of this block has been read
  wrapped = true;
  g_cur += nw;
  nw = g_end - g_cur < WAVES ? static_cast<int>(g_end - g_cur) : WAVES;
  next_rows(g_cur, nw);
  xb1 = xb1n;
  xb2 = xb2n;
  if (nk > 1) issue_x(1, 1);                           // step 1: one MFMA block to land instead of two
  {
    const unsigned char* pf = smem + PF_OFF + uwave * 2048 + lane * 16;
    ra[0][0] = *reinterpret_cast<const f32x4*>(pf);
    ra[0][1] = *reinterpret_cast<const f32x4*>(pf + 1024);
  }
  fixup(0, 0);                                         // every wave (step 0 of a wrapped block skips the late split)
#pragma unroll
  for (int i = 0; i < NT; ++i) acc[i] = f32x4(0.f);
  }
  if (F16 && (a.c_amax_out != nullptr || a.dz_amax_out != nullptr)) {  // (uniform) one atomic per workgroup and output
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned int vc = amx[0], vd = amx[1];
      if (a.c_amax_out != nullptr) rr_amax_put(a.c_amax_out, __uint_as_float(vc));
      if (a.dz_amax_out != nullptr) rr_amax_put(a.dz_amax_out, __uint_as_float(vd));
    }
  }
#ifdef RR_TRACE
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  RR_STAMP(3);
#endif
}

// the device's compute units, asked for once per device (unknown: a count no launch exceeds, so nothing is shared out by it)
inline int split_cus(int dev) {
  static std::atomic<int> n_cu[64];
  int cus = (dev >= 0 && dev < 64) ? n_cu[dev].load(std::memory_order_relaxed) : 0;
  if (cus == 0) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 1 << 30;
    if (dev >= 0 && dev < 64) n_cu[dev].store(cus, std::memory_order_relaxed);
  }
  return cus;
}
// RR_EPI_MODE (A/B knob): 0 = accumulator-layout epilogue everywhere, 1 = row-contiguous where the epilogue READS (a
// residual), 2 = row-contiguous everywhere it applies.  Measured (profiles/r03_experiments.txt): with a residual read
// 223 -> 196 us per isolated 139k-row launch; store-only epilogues do not gain and pay the LDS round trip; inside a
// training step (kernels of three streams interleaved on the chip) the difference is within the noise.
template <int NTP, int NT, int MODE, int WAVES, int EPI, bool F16, int TF = 0>
int launch_split_epi(const LinearParams& P, hipStream_t s) {
  // k-loop: two weight images + the bias slice; the 12-wave geometry's epilogue needs 12 transposition regions of
  // 8 x 77 float4, the column-sum / sign-bit staging and the bias slice (linear_split_kernel, "LDS layout")
  constexpr int panel2 = 2 * NT * (F16 ? 2 : 3) * 1024, bn4 = 16 * NT * 4;
  constexpr bool can_persist = split_can_persist(NTP, NT, MODE, WAVES, EPI);
  constexpr int smem = (WAVES == 12 ? ((12 * 8 * 77 * 16 > panel2 ? 12 * 8 * 77 * 16 : panel2) + 13 * bn4) : panel2 + bn4) +
                       (can_persist ? WAVES * 2048 : 0) + 16;  // + the persistent form's operand prefetch slots + the two magnitude words
  // > 64 KiB of LDS has to be asked for once per kernel AND per device (the attribute lives with the device's code
  // object); atomics because two host threads may launch the same instantiation at once (setting it twice is harmless)
  static std::atomic<uint64_t> configured{0};          // bit d: done on device d (devices >= 64 set it every launch)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return RR_ERR_LAUNCH;
  if (dev < 0 || dev >= 64 || !((configured.load(std::memory_order_acquire) >> dev) & 1u)) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&linear_split_kernel<NTP, NT, MODE, WAVES, EPI, F16, TF>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess)
      return RR_ERR_LAUNCH;
    if (dev >= 0 && dev < 64) configured.fetch_or(uint64_t(1) << dev, std::memory_order_release);
  }
  const int64_t nblk = (P.a.M + 16 * WAVES - 1) / (16 * WAVES);
  // (the balanced instantiations carry a block's first 64-row unit in 29 bits: 2^27 blocks of 3 units, 2.5e10 rows)
  if (split_balanced(NTP, NT, MODE, WAVES, EPI, F16) && nblk >= (int64_t(1) << 27)) return RR_ERR_UNSUPPORTED;
  // Persistent form (see the kernel): plain-operand GEMMs of the one-workgroup-per-CU geometry with more row blocks than
  // CUs, an even number of k-steps (the pipeline's two slots / two image buffers keep their parity across the block
  // boundary) and interior steps on the lean loader.  RR_NO_PERSIST (A/B knob) keeps one workgroup per row block.
  const int cus = split_cus(dev);
  if (can_persist) {
    const int nk = P.t1 + P.t2;
    if (nblk > cus && nk >= 2 && nk % 2 == 0 && split_lean(P.a.k1, P.a.k2) && !getenv("RR_NO_PERSIST")) {
      LinearParams Q = P;
      Q.persist = 1;
      // every CU an equal share of the 64-row units (the granularity of the column-sum partials)
      const dim3 grid(static_cast<unsigned>(cus), 1);
      linear_split_kernel<NTP, NT, MODE, WAVES, EPI, F16, TF><<<grid, 64 * WAVES, smem, s>>>(Q);
      return rr_launch_status();
    }
  }
  // Balanced last round (see the kernel and split_balanced): with
  // U 64-row units, the whole rounds of full blocks - F = floor(U / (3 cus)) * cus workgroups of 3 units, lowest ids, so they
  // are dispatched first - are followed by tail workgroups that share the remaining T = U - 3 F units the way the
  // persistent form shares all of them: T / cus each, the first T % cus one more, none without units.  Taken where it
  // shortens the longest tail block (T <= 2 cus: blocks of 4 or 8 waves instead of 12); with T > 2 cus some tail block has 3
  // units either way and the grid of full blocks stays.  RR_NO_BALANCED_TAIL (A/B knob) keeps that grid everywhere.
  if (split_balanced(NTP, NT, MODE, WAVES, EPI, F16) && nblk > cus && !getenv("RR_NO_BALANCED_TAIL") &&
      !(MODE >= 2 && getenv("RR_NO_BALANCED_TAIL_DX"))) {
    const int64_t units = (P.a.M + 63) / 64;
    const int64_t full = units / (3 * static_cast<int64_t>(cus)) * cus, tail = units - 3 * full;
    if (tail > 0 && tail <= 2 * static_cast<int64_t>(cus)) {
      LinearParams Q = P;
      Q.bal_full = static_cast<int>(full);
      Q.bal_base = static_cast<int>(tail / cus);
      Q.bal_rem = static_cast<int>(tail % cus);
      const dim3 grid(static_cast<unsigned>(full + (Q.bal_base > 0 ? cus : Q.bal_rem)), 1);
      linear_split_kernel<NTP, NT, MODE, WAVES, EPI, F16, TF><<<grid, 64 * WAVES, smem, s>>>(Q);
      return rr_launch_status();
    }
  }
  // (two column blocks: ids i, i + 8 of a 1-D grid are one row block's pair - see the kernel)
  const dim3 grid = NTP == 2 * NT ? dim3(static_cast<unsigned>((nblk + 7) / 8 * 16), 1)
                                  : dim3(static_cast<unsigned>(nblk), static_cast<unsigned>((NTP + NT - 1) / NT));
  linear_split_kernel<NTP, NT, MODE, WAVES, EPI, F16, TF><<<grid, 64 * WAVES, smem, s>>>(P);
  return rr_launch_status();
}
// Fused tail (see the kernel's mfma_block): the TF twin where the instantiation has one and the last k-step has at most 16
// live columns (K = 300: 12; not K = 83, 61 or 600).  Knobs, read per launch: RR_NO_TAIL_FUSE keeps the six-MFMA step
// everywhere, RR_TAIL_FUSE asks for the twins where SPLIT_TAIL_FUSE_DEFAULT does not.
constexpr bool SPLIT_TAIL_FUSE_DEFAULT = true;           // (every twin's per-launch gain is measured: profiles/tail_fuse_ab.txt section 3)
std::atomic<int64_t> split_tail_launches{0};             // rr_linear_split_tail_launches
template <int NTP, int NT, int MODE, int WAVES, int EPI, bool F16>
int launch_split_tail(const LinearParams& P, hipStream_t s) {
  if constexpr (split_tail_fusable(NTP, NT, MODE, WAVES, EPI, F16)) {
    if (split_tail_live(P.a.k1, P.a.k2) <= 16 && !getenv("RR_NO_TAIL_FUSE") && (SPLIT_TAIL_FUSE_DEFAULT || getenv("RR_TAIL_FUSE"))) {
      split_tail_launches.fetch_add(1, std::memory_order_relaxed);
      return (P.t1 + P.t2) % 2 != 0 ? launch_split_epi<NTP, NT, MODE, WAVES, EPI, F16, 1>(P, s) : launch_split_epi<NTP, NT, MODE, WAVES, EPI, F16, 2>(P, s);
    }
  }
  return launch_split_epi<NTP, NT, MODE, WAVES, EPI, F16>(P, s);
}
template <int NTP, int NT, int MODE, int WAVES, bool F16>
int launch_split_one(const LinearParams& P, hipStream_t s) {
  if (WAVES == 12 && (MODE == 0 || MODE == 1)) {       // (the dX forms, MODE 2 / 3, never carry a residual)
    const bool rs = RR_EPI_MODE == 2 || (RR_EPI_MODE == 1 && P.a.residual != nullptr);
    // EPI 0 / 1: the epilogue (accumulator layout / row-contiguous) with the lean loader only; segments past the zero row
    // (K > 992: no configuration of the model) go to the twins EPI 2 / 3, which keep the generic loader
    const bool lean = split_lean(P.a.k1, P.a.k2);
    constexpr int E1 = (WAVES == 12 && (MODE == 0 || MODE == 1)) ? 1 : 0, G = (WAVES == 12 && (MODE == 0 || MODE == 1)) ? 2 : 0;
    if (!lean) return rs ? launch_split_epi<NTP, NT, MODE, WAVES, G + E1, F16>(P, s) : launch_split_epi<NTP, NT, MODE, WAVES, G, F16>(P, s);
    if (rs) return launch_split_tail<NTP, NT, MODE, WAVES, E1, F16>(P, s);
  }
  return launch_split_tail<NTP, NT, MODE, WAVES, 0, F16>(P, s);
}
template <int NTP, int NT, int WAVES, bool F16>
int launch_split(const LinearParams& P, hipStream_t s) {
  if (P.a.a_mask_bits) return launch_split_one<NTP, NT, 3, WAVES, F16>(P, s);
  if (P.a.a_mask) return launch_split_one<NTP, NT, 2, WAVES, F16>(P, s);
  if (P.a.a1_sub) return launch_split_one<NTP, NT, 1, WAVES, F16>(P, s);
  return launch_split_one<NTP, NT, 0, WAVES, F16>(P, s);
}
// the geometry <NTP, NT, WAVES> by N and M, the same for both arithmetic forms
template <bool F16>
int launch_split_geometry(const LinearParams& P, hipStream_t s) {
  const rr_linear_args& a = P.a;
  if (a.N <= 64) return launch_split<4, 4, 8, F16>(P, s);
  if (a.N <= 160) return launch_split<10, 10, 8, F16>(P, s);
  // few rows (the distinct reactants of a shared-prefix step: ~2 k bonds): 192-row workgroups would leave most CUs idle,
  // so the 19 column tiles are cut into blocks of 5 (5 + 5 + 5 + 4) as well - same weight image, same k order
  if (a.N <= 304 && a.M <= 8192) return launch_split<19, 5, 8, F16>(P, s);
  if (a.N <= 304) return launch_split<19, 19, 12, F16>(P, s);
  return launch_split<38, 19, 12, F16>(P, s);           // two column blocks of 19 tiles (H = 600)
}
}  // namespace

extern "C" {

#ifdef RR_TRACE
int rr_trace_set_linear_split(unsigned long long* buf) { return rr_trace_set_unit(buf); }
#endif

int64_t rr_linear_split_tail_launches(void) { return split_tail_launches.load(std::memory_order_relaxed); }

// rr_linear_f32 (linear.hip) has checked the request; k-tiles are k-steps of SK here
int rr_linear_split_launch(const rr_linear_args* args, int two_f16, rr_stream_t stream) {
  LinearParams P = linear_params(*args);
  P.t1 = r32(P.a.k1) / SK;
  P.t2 = r32(P.a.k2) / SK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return two_f16 ? launch_split_geometry<true>(P, s) : launch_split_geometry<false>(P, s);
}

}  // extern "C"
