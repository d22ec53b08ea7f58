/*
 * reactranker_hip.h — C-ABI of the MI355X-native ReactRanker hot path (gfx950 / CDNA4).
 *
 * The reference (IannLiu/ReactRanker) has no FFI layer: its boundary is Python call
 * signatures over stock ATen ops.  Each entry point below replaces one ATen op *site* of
 * the reference's D-MPNN encoder / ranking-loss path (cited per function, paths relative
 * to the reference root).  The host-side mirror (the reactranker_amd package) binds these with
 * ctypes and re-exposes the reference's own names (build_model, MPN, MPNDiff, FFN,
 * MLEloss, ListnetLoss, evidential_ranking, index_select_ND, LogCumsumExp, BatchMolGraph).
 *
 * Conventions
 *   - plain pointers + sizes only; every `float*`/`int32_t*` is DEVICE memory unless the
 *     parameter is documented as host; pointers are borrowed, never retained.
 *   - all floating point is fp32; all indices are int32 (the reference uses int64).
 *   - `stream` is a hipStream_t passed as void*; work is enqueued, never synchronised.
 *   - return value: RR_OK (0) or a negative rr_status; nothing is thrown; re-entrant across streams.
 *     rr_strerror() names a status.  State the library keeps between calls, all of it created lazily and
 *     mutex-guarded: the two non-blocking HIP streams per device that the step plans run their side chains on
 *     (csrc/plan.hip), the one-time shared-memory attribute of the large-LDS kernels, and the RCCL entry points
 *     resolved by the first rr_comm_* call.  No results, tensors or workspaces are retained.
 *   - a row index < 0 in any gather table means "skip" (contributes zero); the reference's
 *     padding index 0 is an ordinary row (row 0 = the padding row of BatchMolGraph,
 *     features/featurization.py:255-264) and is gathered like any other.
 *   - reductions are deterministic: sums run in a fixed order without float atomics; the only atomics are integer
 *     maxima of non-negative floats' bit patterns (the magnitude slots of the two-f16-term GEMMs, rr_amax_f32), which are
 *     exact and order-independent.  Results are run-to-run bit-identical.
 */
#ifndef REACTRANKER_HIP_H
#define REACTRANKER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* rr_stream_t;

typedef enum rr_status {
  RR_OK = 0,
  RR_ERR_ARG = -1,          /* null pointer / negative size / inconsistent shapes */
  RR_ERR_ALIGN = -2,        /* pointer or leading dimension not aligned as required */
  RR_ERR_LAUNCH = -3,       /* hipLaunch / hipGetLastError failed */
  RR_ERR_UNSUPPORTED = -4,  /* size outside the supported range (documented per call) */
  RR_ERR_WORKSPACE = -5     /* workspace too small */
} rr_status;

const char* rr_strerror(int status);
int rr_version(void);               /* ABI version, bumped on any signature change */
/* sizeof(rr_linear_args) / sizeof(rr_wgrad_args) as compiled, so a binding can verify its struct layout. */
void rr_abi_struct_sizes(size_t* linear_args, size_t* wgrad_args);
size_t rr_abi_gather_epi_size(void);   /* sizeof(rr_gather_epi) as compiled */

/* ------------------------------------------------------------------ gathers -------- */

/* out[r, 0:H] = sum_{k<K, idx[r*K+k] >= 0} src[idx[r*K+k], 0:H]
 * Replaces index_select_ND(...).sum(dim=1)  (utils.py:176-193 + models/mpn.py:89-90,
 * 101-102, 201-209, 215-216) without materialising the [n_out, K, H] tensor.  The same
 * kernel run on the transposed tables is the backward of every gather-sum. */
int rr_gather_sum_f32(const float* src, int64_t n_src, int64_t ld_src,
                      const int32_t* idx, int64_t n_out, int K, int H,
                      float* out, int64_t ld_out, rr_stream_t stream);

/* rr_gather_sum_f32 whose output row 0 is instead the fixed-order sum of `n_partial` partial rows
 * (row0_partial[i, 0:H], i ascending): the padding row's adjoint delivered by rr_linear_args.colsum_partial.
 * The one wavefront that owns row 0 does the sum while the others gather - no extra pass, no extra launch. */
int rr_gather_sum_padrow_f32(const float* src, int64_t n_src, int64_t ld_src,
                             const int32_t* idx, int64_t n_out, int K, int H,
                             const float* row0_partial, int64_t n_partial, int64_t ld_partial,
                             float* out, int64_t ld_out, rr_stream_t stream);
/* Both of the above in one entry point (row0_partial may be NULL), plus an optional magnitude output:
 * max |out| maxed into the magnitude slot amax_out - see rr_gather_epi.amax_out. */
int rr_gather_sum_amax_f32(const float* src, int64_t n_src, int64_t ld_src, const int32_t* idx, int64_t n_out, int K,
                           int H, const float* row0_partial, int64_t n_partial, int64_t ld_partial, float* out,
                           int64_t ld_out, float* amax_out, rr_stream_t stream);

/* out[r, 0:H] = sum_{j in [offsets[r], offsets[r+1])} src[idx[j], 0:H]   (CSR form, offsets has n_out+1 entries)
 * The adjoint of index_select_ND (utils.py:176-193) for a GENERIC index tensor: autograd's index_select
 * backward is a scatter-add; here the sources of every destination row are listed (sorted by destination, stable)
 * and summed in that fixed order - no atomics, and no pad width to learn with a device->host sync. */
/* out[r, 0:H] = sum_k (mask[j, :] > 0 ? src[j, :] * scale : 0), j = idx[r*K+k] >= 0 (src and mask share n_src / ld_src):
 * rr_relu_bwd_f32 followed by rr_gather_sum_f32 in one pass, bit-identical to the sequence.  The shared-prefix reactant
 * pass (train_listwise.py:188: every candidate carries its query's reactant) sums each distinct bond's gradient over
 * its copies this way. */
int rr_gather_sum_masked_f32(const float* src, const float* mask, int64_t n_src, int64_t ld_src,
                             const int32_t* idx, int64_t n_out, int K, int H, float scale,
                             float* out, int64_t ld_out, rr_stream_t stream);
/* The same sum when the mask is dropout_j(y[r]) - the copies of a shared row, each with its own dropout mask, as
 * rr_gather_dropout_f32(y, ..., drop_p, drop_seed) produced them:
 *   out[r, c] = sum_k ( kept(drop_seed, j * H + c) && y[r, c] > 0 ? src[j, c] * scale : 0 ),  j = idx[r*K+k] >= 0
 * Equal to rr_gather_sum_masked_f32 on the materialised copies bit for bit, without reading them (ABI revision 5).
 * Needs H % 4 == 0 and 16-byte aligned rows (RR_ERR_ALIGN otherwise). */
int rr_gather_sum_dropmask_f32(const float* src, int64_t n_src, int64_t ld_src, const float* y, int64_t ld_y,
                               const int32_t* idx, int64_t n_out, int K, int H, float drop_p, uint64_t drop_seed,
                               float scale, float* out, int64_t ld_out, rr_stream_t stream);

/* rr_gather_sum_epi_f32 without a mask or addends into an intermediate [n_mid, H], then rr_gather_sum_dropmask_f32 over that
 * intermediate - in one pass that never stores the intermediate (additive to ABI revision 8):
 *   inner(j, c) = ((0 + src[in_idx[j*Ki + 0], c]) + src[in_idx[j*Ki + 1], c]) + ...      negative entry: the +0.0 chunk
 *   out[u, c]   = ((0 + t(j_0)) + t(j_1)) + ...,   j_t = out_idx[u*Ko + t]
 *   t(j)        = (j >= 0 && kept(drop_seed, j * H + c) && y[u, c] > 0) ? inner(j, c) * scale : 0
 * The same additions and products in the same order as the two launches, so the result equals theirs bit for bit.  The
 * shared-prefix reactant backward forms d message of every copy only to sum it over the copies: this removes the write and the
 * read of that [copies, H] tensor.  in_idx is [n_mid, Ki] with values < n_src, out_idx is [n_out, Ko] with values < n_mid,
 * y is [n_out, ld_y].
 * row0_partial (may be NULL): as in rr_gather_sum_padrow_f32, intermediate row 0 is the fixed-order sum of the n_partial
 * partial rows instead of a gather.  PRECONDITION with row0_partial: intermediate row 0 is named by OUTPUT ROW 0 ONLY
 * (the packer's transposed copy table starts with the row [0, -1, ...] and lists copy row 0 nowhere else); any other output
 * row that names it gets the gathered row 0, not the partials' sum.  Needs n_out >= 1.
 * Writes out[u, 0:H] for every u < n_out and nothing else: columns H .. ld_out of a pitched `out` keep what they held.  No
 * scratch.  Needs H % 4 == 0 and 16-byte aligned pointers and pitches (RR_ERR_ALIGN otherwise). */
int rr_gather2_sum_dropmask_f32(const float* src, int64_t n_src, int64_t ld_src, const int32_t* in_idx, int64_t n_mid, int Ki,
                                const float* row0_partial, int64_t n_partial, int64_t ld_partial,
                                const float* y, int64_t ld_y, const int32_t* out_idx, int64_t n_out, int Ko, int H,
                                float drop_p, uint64_t drop_seed, float scale, float* out, int64_t ld_out,
                                rr_stream_t stream);

/* rr_gather_dropout_f32(y, map, ..., drop_p, drop_seed) into copies [n_map, H], then rr_gather_sum_f32 over the copies -
 * without reading (or needing) the copies (additive to ABI revision 8):
 *   out[a, c] = ((0 + v(j_0)) + v(j_1)) + ...,   j_k = idx[a*K + k]
 *   v(j)      = j < 0 ? +0 : ( kept(drop_seed, j * H + c) ? y[map[j], c] / (1 - drop_p) : 0 )       (map[j] < 0: the zero row)
 * Every v(j) is bit for bit the element rr_gather_dropout_f32 stores in row j, so the sum equals rr_gather_sum_f32's over the
 * materialised tensor.  Row 0 is an ordinary row.  map is [n_map] with values < n_y, idx is [n_out, K] with values < n_map.
 * In the shared-prefix reactant forward the first per-copy layer's atom sums could be formed from the distinct bonds'
 * activations this way.  The step plans do NOT use it: at the headline shape it takes 52 us stand-alone against 44 us of
 * rr_gather_sum_f32 over the copies, which rr_gather_dropout_amax_f32 has to write anyway for the GEMM and the weight gradient
 * (profiles/prefix_fuse_ab.txt).  It is kept as a tested library entry for callers that do not materialise the copies.
 * Writes out[a, 0:H] for every a < n_out and nothing else: pad columns of a pitched `out` keep what they held.  No scratch.
 * Needs H % 4 == 0 and 16-byte aligned pointers and pitches (RR_ERR_ALIGN otherwise). */
int rr_gather_sum_dropsrc_f32(const float* y, int64_t n_y, int64_t ld_y, const int32_t* map, int64_t n_map,
                              const int32_t* idx, int64_t n_out, int K, int H, float drop_p, uint64_t drop_seed,
                              float* out, int64_t ld_out, rr_stream_t stream);

/* The sum over idx of a tensor that is itself a sum of n_srcs tensors of one shape (ABI revision 8):
 *   out[r, :] = sum_{k<K, j = idx[r*K+k] >= 0} ( ((srcs[0][j, :] + srcs[1][j, :]) + srcs[2][j, :]) + ... )
 * In the shared-prefix reactant backward a copy's d input is the sum of the dZ of every per-copy layer (models/mpn.py:94-97)
 * and only its sum over the copies is needed: this replaces n_srcs - 1 rr_axpby_f32 passes over [n_src, H] plus a one-source
 * gather by one pass that reads every addend once.  Same additions, same order: bit-identical to that sequence.
 * 1 <= n_srcs <= RR_MAX_GATHER_SRCS; `srcs` is a HOST array of device pointers, all [n_src, ld_src].  H % 4 == 0 and 16-byte
 * aligned rows (RR_ERR_ALIGN otherwise - callers then run the sequence above). */
#define RR_MAX_GATHER_SRCS 4
int rr_gather_sum_multi_f32(const float* const* srcs, int n_srcs, int64_t n_src, int64_t ld_src,
                            const int32_t* idx, int64_t n_out, int K, int H,
                            float* out, int64_t ld_out, rr_stream_t stream);

/* Gather-sum with a fused epilogue - the form the backward chain uses (ABI revision 4):
 *   out[r, :] = M_r( sum_{k<K, idx[r*K+k] >= 0} src[idx[r*K+k], :] )  +  sum_{j<n_adds} adds[j][r, :]
 *   M_r(g)[c] = g[c]                                   without a mask
 *             = (mask[r, c] > 0) ? g[c] * mask_scale : 0   with `mask` ([n_out, ld_mask] f32) or `mask_bits` (the sign-bit
 *               image rr_linear_args.mask_bits_out wrote for that activation: rr_mask_bits_row_bytes(H) bytes per row;
 *               preferred when both are given - 1/32 of the bytes)
 * The adjoint of a message-passing layer never needs the gathered gradient as such: d message is consumed masked by the
 * ReLU / dropout pattern of the layer below (dZ = d message * (y > 0) / (1 - p), models/mpn.py:94-97) and the gradient of
 * the residual `input` (:94) is the sum of every iteration's dZ.  With the mask and the sum applied here, by the HBM-bound
 * kernel that produces the gradient, the dX GEMM downstream reads dZ as a plain operand (no mask, no dZ side output
 * written from inside its k-loop) and rr_relu_bwd_sum_f32's extra pass disappears.  The addends are summed in order
 * starting from zero and the masked gather is added last - the order of rr_relu_bwd_sum_f32 - so the result equals the
 * separate-kernel sequence bit for bit.  row0_partial (may be NULL) as in rr_gather_sum_padrow_f32; the epilogue applies
 * to row 0 as well.  Requires H % 4 == 0 and 16-byte aligned rows everywhere (RR_ERR_ALIGN otherwise); `epi` is a HOST
 * struct of device pointers. */
#define RR_MAX_GATHER_ADDS 15
typedef struct rr_gather_epi {
  const float* mask;        int64_t ld_mask;
  const uint8_t* mask_bits;
  float mask_scale;
  int n_adds;               int64_t ld_add;      /* every addend is [n_out, ld_add] */
  const float* adds[RR_MAX_GATHER_ADDS];
  float* amax_out;          /* optional: max |out| maxed into this magnitude slot (RR_AMAX_FLOATS floats, see rr_amax_f32) - the
                               bound a two-f16-term GEMM needs of this result (rr_linear_args.a1_amax) without a pass over it */
} rr_gather_epi;
int rr_gather_sum_epi_f32(const float* src, int64_t n_src, int64_t ld_src,
                          const int32_t* idx, int64_t n_out, int K, int H,
                          const float* row0_partial, int64_t n_partial, int64_t ld_partial,
                          const rr_gather_epi* epi, float* out, int64_t ld_out, rr_stream_t stream);

int rr_gather_sum_csr_f32(const float* src, int64_t n_src, int64_t ld_src,
                          const int32_t* offsets, const int32_t* idx, int64_t n_out, int H,
                          float* out, int64_t ld_out, rr_stream_t stream);

/* f_bonds[b, :] = [ f_atoms[b2a[b], 0:atom_fdim] | fbond[b, 0:bond_fdim] | zeros up to ld_out ]
 * The reference stores a directed bond's feature row as its source atom's features followed by the bond's own
 * (features/featurization.py:198-199), i.e. 61 of the 83 columns repeat f_atoms.  A packed step therefore ships only the
 * bond columns (reactranker_amd/shards.py) and this kernel rebuilds the [n_bonds, ld_out] array in HBM.  b2a values must
 * lie in [0, n_atoms). */
int rr_build_fbonds_f32(const float* f_atoms, int64_t n_atoms, int64_t ld_fa, int atom_fdim, const int32_t* b2a,
                        const float* fbond, int64_t ld_fbb, int bond_fdim, int64_t n_bonds,
                        float* out, int64_t ld_out, rr_stream_t stream);

/* out[r] = (ia[r] >= 0 ? a[ia[r]] : 0) - (im[r] >= 0 ? m[im[r]] : 0)
 * Replaces  message = a_message[b2a] - message[b2revb]  (models/mpn.py:91-92); with the
 * transposed tables (b2t, b2revb) it is that line's backward. */
int rr_gather_diff_f32(const float* a, int64_t n_a, int64_t ld_a, const int32_t* ia,
                       const float* m, int64_t n_m, int64_t ld_m, const int32_t* im,
                       int64_t n_out, int H, float* out, int64_t ld_out, rr_stream_t stream);

/* out[r, c] = keep(seed, r*H + c) ? src[idx[r], c] / (1 - p) : 0     (idx[r] < 0 -> 0)
 * Expands rows shared by several destinations and applies each destination's own dropout mask: the
 * message after the first W_h of a de-duplicated reactant (same mask stream as rr_linear_f32's epilogue). */
int rr_gather_dropout_f32(const float* src, int64_t n_src, int64_t ld_src, const int32_t* idx, int64_t n_out, int H,
                          float drop_p, uint64_t drop_seed, float* out, int64_t ld_out, rr_stream_t stream);
/* The same with a magnitude output (see rr_gather_epi.amax_out): max |out| maxed into the slot amax_out (may be NULL). */
int rr_gather_dropout_amax_f32(const float* src, int64_t n_src, int64_t ld_src, const int32_t* idx, int64_t n_out, int H,
                               float drop_p, uint64_t drop_seed, float* out, int64_t ld_out, float* amax_out,
                               rr_stream_t stream);

/* out[0:H] (+)= sum_r w[r] * x[r, 0:H]   (w == NULL -> all ones).
 * Backward of the padding row: the reference gathers row 0 (K - deg(a)) times per atom
 * (features/featurization.py:286), so d_src[0] = sum_a npad[a] * d_out[a].  Also used for
 * bias gradients.  workspace: rr_colsum_workspace_bytes(n, H) bytes. */
size_t rr_colsum_workspace_bytes(int64_t n, int H);
int rr_weighted_colsum_f32(const float* x, int64_t n, int64_t ld, const float* w, int H,
                           float* out, int accumulate, void* workspace, size_t workspace_bytes,
                           rr_stream_t stream);

/* ------------------------------------------------------------------ dense layers --- */

typedef enum rr_act { RR_ACT_NONE = 0, RR_ACT_RELU = 1 } rr_act;

/* C[m, n] = dropout(act(residual[m,n] + bias[n] + sum_k A[m,k] * W[n,k]))
 *
 * A is the concatenation [A1 | A2] (k1 + k2 columns, either may be 0 wide):
 *   A1 row m = (a1_idx ? a1[a1_idx[m]] : a1[m])  -  (a1_sub ? a1_sub[a1_sub_idx ? a1_sub_idx[m] : m] : 0)
 *   A2 row m = a2[m]
 * and, if a_mask != NULL, every A element is multiplied by (a_mask[m,k] > 0) * mask_scale
 * (ReLU/dropout backward fused into the operand load; requires k2 == 0).
 *
 * One call replaces, at the reference's sites:
 *   W_i(f_bonds) + relu                         models/mpn.py:80-81, 194-195
 *   a_message[b2a] - message[b2revb]; W_h; input + .; relu; dropout   models/mpn.py:91-97
 *   cat([f_atoms, a_message]); W_o; relu; dropout                     models/mpn.py:103-105, 217-219
 *   cat(nei_a_message, nei_f_bonds).sum; W_h; ...                     models/mpn.py:208-213
 *   FFN Linear/ReLU/Dropout chain                                     models/base_model.py:32-60
 * and their input-gradient GEMMs (dX = dZ * W  ==  same call with w = W^T).
 *
 * Arithmetic: fp32 operands and results, fp32 accumulation.  Two kernels serve the call: with w_packed = 1 every
 * product runs on the f32 MFMA (v_mfma_f32_16x16x4_f32, bit for bit an fmaf chain); with w_packed = 2 (weights
 * packed as three exact bf16 terms by rr_pack_weights_f32 / rr_pack_weight_f32 with split = 1) each f32 operand is
 * written EXACTLY as three bf16 terms and the six products down to 2^-18 |x w| are accumulated in f32 by
 * v_mfma_f32_16x16x32_bf16 - no operand bit is dropped, what is omitted lies below 2^-26 |x w| per product, and the
 * measured error against f64 is at or below the f32-MFMA kernel's.  Differences in kind on
 * that path: an infinite operand, or a finite |x| >= 3.3962e38, turns its output row into NaN (the f32 MFMA gives
 * +-inf).  With w_packed = 3 each operand is scaled by a power of two S that puts its tensor's largest magnitude (the
 * caller's a*_amax bounds; the weight's own, found by the packer) just below 2^15 and written as TWO f16 terms,
 * S x = h + l, h = f16(S x), l = f16(S x - h) (round to nearest even; the remainder is exact): 22 significant bits of
 * every element that is within 2^-18 of its tensor's largest, an absolute error below 2^-40 of that largest otherwise;
 * the three products h h, h l, l h are accumulated in f32 by v_mfma_f32_16x16x32_f16 and the result is scaled back
 * (exactly).  Omitted: l l, below 2^-22 |x w|.  Measured against f64 on N(0,1) operands, K = 300: mean error
 * 2.6e-8 of sum |x||w| (three bf16 terms 1.6e-8, the f32 MFMA chain 2.0e-8), maximum below the f32 chain's
 * (tools/f16_gemm_bench.py).  Dropout keep-mask = rr_dropout_keep(seed, m*N + n).
 * `residual` may alias `c` (in-place accumulate).  Vector loads need 16-byte aligned base
 * pointers and leading dimensions that are multiples of 4; otherwise a scalar path runs. */
typedef struct rr_linear_args {
  int64_t M;
  int N;
  const float* a1;       int64_t lda1;      int k1;   const int32_t* a1_idx;
  const float* a1_sub;   int64_t lda1_sub;            const int32_t* a1_sub_idx;
  const float* a2;       int64_t lda2;      int k2;
  const float* a_mask;   int64_t ld_mask;   float mask_scale;
  float* dz_out;         int64_t ld_dz;     int dz_accumulate;  /* with a_mask: also materialise the masked operand,
                                                       dz_out[m,k] (+)= A[m,k] — e.g. d_input += dZ of every
                                                       message-passing step (the residual `input +` of mpn.py:95).
                                                       Needs k1 % 4 == 0 and 16-byte aligned rows. */
  const float* w;        int64_t ldw;               /* [N, k1+k2] row-major (nn.Linear.weight), or */
  int w_packed;                                     /* 1: the zero-padded layout of rr_pack_weight_f32;
                                                       2: the three-bf16-term images of rr_pack_weights_f32
                                                          (rr_pack_desc.split = 1): f32 result on the bf16 matrix core;
                                                       3: its two-f16-term images (rr_pack_desc.split = 2): 22 significant
                                                          bits per operand, half the matrix instructions (see below) */
  const float* bias;                                /* [N] or NULL */
  const float* residual; int64_t ldr;               /* [M, N] or NULL */
  const int32_t* residual_idx;                      /* optional: row m adds residual[residual_idx[m]] (shared `input`
                                                       of a de-duplicated reactant, models/mpn.py:95) */
  int act;                                          /* rr_act */
  float drop_p;          uint64_t drop_seed;        /* drop_p == 0 -> no dropout */
  float* c;              int64_t ldc;
  float* c_pre;          int64_t ld_pre;            /* optional second output: the pre-activation value
                                                       (input = W_i(f_bonds) next to message = relu(input),
                                                       models/mpn.py:80-81) */
  const float* colsum_w;                            /* optional third output (fast path only): per-row weights w[M] ... */
  float* colsum_partial; int64_t ld_partial;        /* ... and partial[rr_linear_colsum_rows(M), ld_partial >= N]:
                                                       partial[i, n] = sum over the 64 rows of row block i of w[m]*C[m,n].
                                                       The padding row's adjoint (a2b is right-padded with bond 0,
                                                       features/featurization.py:286, so row 0 of a gathered source
                                                       receives sum_a npad[a] * d_out[a]) falls out of the GEMM that
                                                       produces d_out instead of a separate pass over it; the partial
                                                       rows are summed, in order, by rr_gather_sum_padrow_f32. */
  uint8_t* mask_bits_out;                           /* optional fourth output (w_packed = 2, N % 4 == 0): the sign of every
                                                       stored element, 1 bit each, rr_mask_bits_row_bytes(N) bytes per row:
                                                       per block of up to 304 columns 2 x 20 bytes - byte 20*h + t holds
                                                       columns 16*t + 8*h .. + 7 (bit e = column + e).  Bytes 19 and 39
                                                       of a 40-byte block and the bytes of the 16-column tiles past N stand
                                                       for no column: they are unspecified (not necessarily written) and
                                                       never read.  What a later
                                                       dX GEMM needs of this activation (a_mask > 0), at 1/32 of the bytes */
  const uint8_t* a_mask_bits;                       /* alternative to a_mask (w_packed >= 2, k2 = 0, k1 % 4 == 0): such a bit
                                                       image over the k1 columns of A; a_mask is then not read */
  const float* a1_amax;                             /* w_packed = 3 only (required there for every operand present): DEVICE */
  const float* a1_sub_amax;                         /* magnitude slots (RR_AMAX_FLOATS floats each, see rr_amax_f32) whose maximum */
  const float* a2_amax;                             /* is >= max |x| over the elements of a1 / a1_sub / a2 this call can read (a
                                                       bound that is too large costs low-end precision, one that is too small
                                                       overflows f16) */
  float* c_amax_out;                                /* optional outputs (w_packed = 3): max |C| stored, and the same for dz_out, */
  float* dz_amax_out;                               /* maxed into a magnitude slot - the bound the NEXT GEMM needs of this one's
                                                       result without a pass over it (zero the slot first) */
} rr_linear_args;

int rr_linear_f32(const rr_linear_args* args, rr_stream_t stream);
int64_t rr_mask_bits_row_bytes(int N);
/* Row blocks (= partial rows written through colsum_partial) of an M-row call. */
int64_t rr_linear_colsum_rows(int64_t M);
/* Launches of the split GEMM's fused-tail kernels (w_packed = 2, last k-step with at most 16 live columns) this process has
 * made: which kernel a request took cannot be told from its result, so tests and tools read this counter around a call. */
int64_t rr_linear_split_tail_launches(void);

/* Packed weight layout for the straight-line fast path of rr_linear_f32:
 *   dst[r, 0:k1] = L[r, 0:k1];  dst[r, r16(k1) : r16(k1)+k2] = L[r, k1:k1+k2];  zeros elsewhere;
 *   row stride rr_packed_weight_ld(k1,k2) = r16(k1) + r16(k2), r16 = round up to 16;
 *   L[r, c] = src[r*ld_src + c0 + c]            (transpose = 0: a column slice of the weight)
 *           = src[c*ld_src + c0 + r]            (transpose = 1: its transpose, for dX = dZ * W)
 * Weights change every optimizer step, so the mirror re-packs them once per forward. */
int64_t rr_packed_weight_ld(int k1, int k2);
int rr_pack_weight_f32(const float* src, int64_t ld_src, int transpose, int rows, int c0, int k1, int k2,
                       float* dst, rr_stream_t stream);

/* rr_pack_weight_f32 for up to RR_MAX_PACK weights in one launch (`descs` is a HOST array). */
#define RR_MAX_PACK 24
typedef struct rr_pack_desc {
  const float* src;  int64_t ld_src;  int transpose, rows, c0, k1, k2;
  float* dst;
  int split;         /* 0: the f32 layout above.  1: dst (rr_split_weight_bytes(rows, k1, k2) bytes, 16-byte aligned,
                        rows <= 608) receives every element of L as three bf16 terms t0 + t1 + t2 == L[r, c] EXACTLY
                        (t0 = bf16(x), t1 = bf16(x - t0), t2 = x - t0 - t1), laid out as the LDS image of each
                        32-deep k-step of rr_linear_f32's w_packed = 2 path:
                        [k-step][16-column tile][term][lane 0..63][8 bf16], lane = (k-group of 8) * 16 + column.
                        2: the same buffer receives TWO f16 terms of S * L[r, c] per element (same layout with two terms
                        per tile), S = the power of two with 2^14 <= S * max |L| < 2^15, stored as one float right after
                        the last k-step's image (rr_linear_f32, w_packed = 3, reads it there).  The bytes of dst behind
                        that float (the buffer is sized for three terms) are unspecified: scratch of the packing
                        launch, never read by rr_linear_f32 */
} rr_pack_desc;
int rr_pack_weights_f32(const rr_pack_desc* descs, int n, rr_stream_t stream);
size_t rr_split_weight_bytes(int rows, int k1, int k2);

/* dW[n, k] (+)= sum_m dZ[m,n] * X[m,k],   dbias[n] (+)= sum_m dZ[m,n]
 * dZ[m,n] = dy[m,n] * (mask ? (mask[m,n] > 0) * mask_scale : 1);  X = [X1 | X2] described
 * exactly like A above.  Weight gradients of every nn.Linear on the path; the sum over the
 * M rows is split across workgroups and finished by a fixed-order second pass.
 * workspace: rr_linear_wgrad_workspace_bytes(M, N, k1+k2). */
typedef struct rr_wgrad_args {
  int64_t M;
  int N;
  const float* dy;       int64_t ld_dy;
  const float* mask;     int64_t ld_mask;   float mask_scale;
  const float* x1;       int64_t ldx1;      int k1;   const int32_t* x1_idx;
  const float* x1_sub;   int64_t ldx1_sub;            const int32_t* x1_sub_idx;
  const float* x2;       int64_t ldx2;      int k2;
  float* dw;             int64_t ld_dw;             /* [N, k1+k2] */
  float* dbias;                                     /* [N] or NULL */
  int accumulate;                                   /* 0: overwrite, 1: add into dw/dbias */
  void* workspace;       size_t workspace_bytes;
  int split;                                        /* 1: three-bf16-term operands on the bf16 matrix core (f32-equivalent
                                                       accuracy, see rr_pack_desc.split) where the geometry allows vector
                                                       loads (16-byte aligned rows, N % 4 == 0); the f32 path otherwise.
                                                       2: two-f16-term operands (rr_linear_args.w_packed = 3), which needs */
  const float* dy_amax;                             /* ... the magnitude slots of dy, x1, x1_sub, x2 (as rr_linear_args.a1_amax) */
  const float* x1_amax;
  const float* x1_sub_amax;
  const float* x2_amax;
} rr_wgrad_args;

size_t rr_linear_wgrad_workspace_bytes(int64_t M, int N, int K);
int rr_linear_wgrad_f32(const rr_wgrad_args* args, rr_stream_t stream);

/* A magnitude slot: RR_AMAX_LANES floats RR_AMAX_STRIDE floats apart (RR_AMAX_FLOATS floats in all, device memory) whose
 * MAXIMUM is the bound - a producer's workgroups max their values into different lanes, because atomics on one busy address
 * serialise (~5 ns each).  Zero the RR_AMAX_FLOATS floats before the first producer; every kernel only ever raises them.
 * rr_amax_f32: slot = max(slot, max over the [rows, cols] block of |x[r * ld + c]|)  (NaN elements are skipped).
 * The operand bounds of the two-f16-term GEMMs (rr_linear_args.a1_amax, rr_wgrad_args.dy_amax). */
#define RR_AMAX_LANES 16
#define RR_AMAX_STRIDE 32
#define RR_AMAX_FLOATS (RR_AMAX_LANES * RR_AMAX_STRIDE)
int rr_amax_f32(const float* x, int64_t rows, int cols, int64_t ld, float* amax, rr_stream_t stream);

/* ------------------------------------------------------------------ elementwise ---- */

/* 1 iff element `index` is kept by dropout stream `seed` at rate p (host + device agree). */
int rr_dropout_keep_host(uint64_t seed, uint64_t index, float p);

/* out[i] = keep(seed, i) ? x[i] / (1 - p) : 0   — nn.Dropout in training mode with the counter-based
 * mask stream; the same call on a gradient is its backward.  (FFN input dropout, models/base_model.py:32-36.) */
int rr_dropout_f32(const float* x, int64_t n, float p, uint64_t seed, float* out, rr_stream_t stream);

/* dz = dy * (y > 0) * scale (dz may be NULL when only the accumulation is wanted);  if acc != NULL: acc += dz.   (ReLU + inverted-dropout backward;
 * y is the layer's stored post-dropout output, so y > 0 <=> kept and active.) */
int rr_relu_bwd_f32(const float* dy, const float* y, float scale, float* dz, float* acc,
                    int64_t n, rr_stream_t stream);

/* out = sum_{k<n_adds} adds[k] + dy * (y > 0) * scale.  `adds` is a HOST array of n_adds (<= 15) device pointers.
 * The gradient of a residual read by several layers: `input` of models/mpn.py:80 enters every message-passing
 * iteration (:94), so d input = sum_it dZ_it + relu'(input) * d message_0 - formed in one pass over memory from
 * the per-iteration dZ buffers the input-gradient GEMMs write (rr_linear_args.dz_out). */
int rr_relu_bwd_sum_f32(const float* dy, const float* y, float scale, const float* const* adds, int n_adds,
                        float* out, int64_t n, rr_stream_t stream);

/* out = alpha * a + beta * b   (b may be NULL).  diff = p_h - r_h (models/base_model.py:168). */
int rr_axpby_f32(float alpha, const float* a, float beta, const float* b, float* out,
                 int64_t n, rr_stream_t stream);

/* Adam update of up to RR_MAX_ADAM tensors in ONE launch (ABI revision 6) - the optimizer the reference builds
 * (train/utils.py:100-113: torch.optim.Adam, lr 1e-4, weight_decay 0; betas / eps torch's defaults), per element:
 *   g' = g + weight_decay * p;  m = m + (g' - m) * (1 - beta1);  v = beta2 * v + (1 - beta2) * g' * g'
 *   p -= (lr / (1 - beta1^step)) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * i.e. torch's own formula (fused_adam_utils.cuh: scalars in double, each element rounded to f32 once), with `step` the
 * 1-based count of this update.  `descs` is a HOST array;
 * a tensor with g == NULL is skipped.  torch's multi-tensor kernel walks 64k-element chunks, ~20 workgroups for this
 * model's 0.8 M parameters (45 us on MI355X); here a workgroup takes 1024 elements. */
#define RR_MAX_ADAM 64
typedef struct rr_adam_tensor { float* p; const float* g; float* m; float* v; int64_t n; } rr_adam_tensor;
int rr_adam_step_f32(const rr_adam_tensor* descs, int n_tensors, int64_t step, double lr, double beta1, double beta2, double eps,
                     double weight_decay, rr_stream_t stream);

/* FFN output heads (models/base_model.py:61-106), applied to raw[M, N] -> out[M, N]. */
typedef enum rr_head {
  RR_HEAD_IDENTITY = 0,            /* 'no_softplus', 'with_softplus' with task_num==1, ... */
  RR_HEAD_SOFTPLUS = 1,            /* 'listnet_with_softplus' */
  RR_HEAD_SOFTPLUS_PLUS1 = 2,      /* 'listnet_with_uncertainty', 'evidential' */
  RR_HEAD_EVIDENTIAL_RANKING = 3,  /* [score, softplus(u)+1e-6] interleaved (:91-98) */
  RR_HEAD_GAUSSIAN_SOFTPLUS = 4,   /* [mu, softplus(v)] (:71-82) */
  RR_HEAD_LOGNORM_SOFTPLUS = 5,    /* [softplus(mu)+1e-6, softplus(v)+1e-6] (:83-90) */
  RR_HEAD_EVIDENTIAL4_SOFTPLUS = 6 /* [mu, sp+1e-6, sp+1e-6+1, sp+1e-6] (:61-70) */
} rr_head;
int rr_head_fwd_f32(const float* raw, int64_t M, int N, int head, float* out, rr_stream_t stream);
int rr_head_bwd_f32(const float* dout, const float* raw, int64_t M, int N, int head, float* draw,
                    rr_stream_t stream);

/* ------------------------------------------------------------------ readout -------- */

/* out[m, 0:H] = mean over atoms [start, start+size) of x;  out[m, H:H+F] = feat[m, 0:F];
 * then inverted dropout (stream seed, index m*(H+F)+c) if drop_p > 0.
 * a_scope is [M,2] = (start, size) as BatchMolGraph.a_scope (featurization.py:276);
 * size == 0 gives a zero row (cached_zero_vector, models/mpn.py:226-227).
 * Columns H+F .. ld_out-1 of a row of out (the pad of a pitched output) are unspecified: not written here, and no result of
 * a kernel that reads the rows with k = H+F depends on them.
 * Replaces the per-molecule narrow/sum/div/stack loop + cat (models/mpn.py:224-238). */
int rr_segment_mean_fwd_f32(const float* x, int64_t ldx, const int32_t* a_scope, int64_t M, int H,
                            const float* feat, int F, float drop_p, uint64_t drop_seed,
                            float* out, int64_t ld_out, rr_stream_t stream);
/* dx[a, 0:H] = dout[mol(a), 0:H] * keep/(1-p) / size(mol(a));  atom2mol[a] < 0 -> zero row. */
int rr_segment_mean_bwd_f32(const float* dout, int64_t ld_dout, const int32_t* a_scope,
                            const int32_t* atom2mol, int64_t n_atoms, int H, int F,
                            float drop_p, uint64_t drop_seed,
                            float* dx, int64_t ldx, rr_stream_t stream);

/* The same followed by the ReLU / dropout backward of the layer that produced the readout's input:
 *   dx[a, c] = (mask[a, c] > 0) ? dx[a, c] * mask_scale : 0      (mask / mask_bits as in rr_gather_epi; one of them required)
 * so the two dX GEMMs of W_o's column blocks (models/mpn.py:217-219) read a plain operand.  H % 4 == 0 and aligned rows. */
int rr_segment_mean_bwd_masked_f32(const float* dout, int64_t ld_dout, const int32_t* a_scope,
                                   const int32_t* atom2mol, int64_t n_atoms, int H, int F,
                                   float drop_p, uint64_t drop_seed,
                                   const float* mask, int64_t ld_mask, const uint8_t* mask_bits, float mask_scale,
                                   float* dx, int64_t ldx, rr_stream_t stream);
/* The same with a magnitude output (see rr_gather_epi.amax_out): max |dx| maxed into the slot amax_out (may be NULL). */
int rr_segment_mean_bwd_masked_amax_f32(const float* dout, int64_t ld_dout, const int32_t* a_scope,
                                        const int32_t* atom2mol, int64_t n_atoms, int H, int F, float drop_p,
                                        uint64_t drop_seed, const float* mask, int64_t ld_mask, const uint8_t* mask_bits,
                                        float mask_scale, float* dx, int64_t ldx, float* amax_out, rr_stream_t stream);

/* ------------------------------------------------------------------ ranking losses - */
/* Lists are described by seg_off[Q+1] (prefix sums of the reference's `scope` list);
 * max_len = longest list (host value, sizes the LDS staging; supported up to 8192).
 * score/targets/var elements are read at p[i * stride].  `loss` is one float on the device.
 * `gloss` is the upstream gradient (one float on the device). */

/* ListMLE: MLEloss + LogCumsumExp (train/loss.py:9-99). Ties in targets break by index. */
int rr_listmle_fwd_f32(const float* score, int64_t score_stride, const float* targets,
                       const int32_t* seg_off, int Q, int max_len,
                       float* loss, float* partial /* [Q] */, rr_stream_t stream);
int rr_listmle_bwd_f32(const float* score, int64_t score_stride, const float* targets,
                       const int32_t* seg_off, int Q, int max_len, const float* gloss,
                       float* dscore, int64_t dscore_stride, rr_stream_t stream);

/* Fused loss + gradient ("step") forms, ABI revision 8: ONE launch writes `loss` AND d loss / d score for an upstream
 * gradient of one - what `loss.backward()` feeds a loss that is the root of the graph (train/train_listwise.py:287-288) -
 * so a training step needs no second loss kernel, no separate reduction launch and no device-side gradient seed.  `loss`,
 * `partial` and `dscore` hold the bits rr_*_fwd_f32 / rr_*_bwd_f32 (with *gloss == 1.0f) write: same operations in the same
 * order, the per-query partials summed in the same fixed order by the workgroup that finishes last.  `counter` is ONE
 * device word per concurrent launch that the caller keeps.  PRECONDITION: it is zero (or a multiple of Q: the ticket is
 * tested modulo Q) when the launch starts; the kernel leaves it at zero. */
int rr_listmle_step_f32(const float* score, int64_t score_stride, const float* targets,
                        const int32_t* seg_off, int Q, int max_len, float* loss, float* partial /* [Q] */,
                        unsigned int* counter, float* dscore, int64_t dscore_stride, rr_stream_t stream);
int rr_listnet_step_f32(const float* score, int64_t score_stride, const float* targets,
                        const int32_t* seg_off, int Q, int max_len, int64_t total, float* loss, float* partial,
                        unsigned int* counter, float* dscore, int64_t dscore_stride, rr_stream_t stream);
int rr_evidential_ranking_step_f32(const float* mu, const float* var, int64_t stride, const float* targets,
                                   const int32_t* seg_off, int Q, int max_len, float* loss, float* partial,
                                   unsigned int* counter, float* dmu, float* dvar, int64_t dstride, rr_stream_t stream);

/* A composite task type's loss and its gradient in ONE launch (additive: two new symbols, the ABI revision stays 8; a
 * library without them fails a binding's symbol lookup, and rr_abi_task_loss_size() checks the struct layout).  The trainer's composite task types
 * (train/train_listwise.py:196-285) add a per-list term and a per-candidate term over column slices of the head's output
 * `out` [M, n_cols] (row stride ld_out, M = seg_off[Q]).  rr_task_loss_step_f32 writes loss = list term + point term and
 * d loss / d out [M, n_cols] (row stride ld_dout; EVERY column of every row, exact zeros where the task reads none) for an
 * upstream gradient of one.  One wavefront per query evaluates the list term on the staged list and the point term of the
 * query's own candidates.
 *   list term    reads                                   averaged over
 *   MLE          column 0                                n_queries (mean over a list, then over lists)
 *   LISTNET      column 0                                n_cands   (one mean over all candidates)
 *   MLEDIS       column 0, variance = exp(column 1)      n_queries (the transform of the mledis_gaussian branch, :196-202;
 *                                                                   d / d column 1 carries the factor exp(column 1))
 *   LISTNET_GAUSS column 0, variance = column 1          n_queries
 *   LISTNET_UQ / DIRICHLET_UQ  column 0, `coef`          n_queries (coef: the annealing coefficient)
 *   point term   MSE: column 0;  GAUSS: mean = column 0, variance = the raw column 1      n_cands
 * n_queries / n_cands are the counts to divide by: Q and M for one process, the whole step's counts for a shard of a
 * data-parallel step (the shards' losses and gradients then add up to the unsharded ones).  A count of 0 scales by 0.
 * `partial` is a [2, Q] workspace (list row, point row); the workgroup that finishes last sums both rows in a fixed order,
 * so the loss has the same bits on every run.  `terms` (or NULL) receives the two terms; loss == terms[0] + terms[1]
 * exactly.  `counter`: ONE device word per concurrent launch that the caller keeps.  PRECONDITION: it is zero (or a
 * multiple of Q: the ticket is tested modulo Q) when the launch starts; the kernel leaves it at zero.  An empty query
 * adds zero and still counts; max_len > 8192 -> RR_ERR_UNSUPPORTED, nothing is launched; Q == 0 writes a zero loss. */
enum { RR_LIST_NONE = 0, RR_LIST_MLE = 1, RR_LIST_LISTNET = 2, RR_LIST_MLEDIS = 3, RR_LIST_LISTNET_GAUSS = 4,
       RR_LIST_LISTNET_UQ = 5, RR_LIST_DIRICHLET_UQ = 6 };
enum { RR_POINT_NONE = 0, RR_POINT_MSE = 1, RR_POINT_GAUSS = 2 };
typedef struct rr_task_loss_args {
  int list_term, point_term;          /* RR_LIST_*, RR_POINT_*: not both NONE */
  const float* out;  int64_t ld_out;  /* [M, n_cols], row stride ld_out >= n_cols (a column slice of a wider tensor is fine) */
  int n_cols;
  const float* targets;               /* [M] */
  const int32_t* seg_off;             /* [Q + 1] */
  int Q, max_len;
  float coef;
  int64_t n_queries, n_cands;
  float* loss;                        /* one float */
  float* terms;                       /* [2] or NULL */
  float* dout;  int64_t ld_dout;      /* [M, n_cols], row stride ld_dout >= n_cols */
  float* partial;                     /* [2, Q] */
  unsigned int* counter;
} rr_task_loss_args;
size_t rr_abi_task_loss_size(void);
int rr_task_loss_step_f32(const rr_task_loss_args* args, rr_stream_t stream);

/* ListNet top-1, one global mean over all candidates (train/loss.py:327-352). */
int rr_listnet_fwd_f32(const float* score, int64_t score_stride, const float* targets,
                       const int32_t* seg_off, int Q, int max_len, int64_t total /* = seg_off[Q] */,
                       float* loss, float* partial, rr_stream_t stream);
int rr_listnet_bwd_f32(const float* score, int64_t score_stride, const float* targets,
                       const int32_t* seg_off, int Q, int max_len, int64_t total, const float* gloss,
                       float* dscore, int64_t dscore_stride, rr_stream_t stream);

/* UC-Listwise evidential_ranking live branch (train/loss.py:526-556): mu/var are the two
 * columns of the [M,2] model output. */
int rr_evidential_ranking_fwd_f32(const float* mu, const float* var, int64_t stride,
                                  const float* targets, const int32_t* seg_off, int Q, int max_len,
                                  float* loss, float* partial, rr_stream_t stream);
int rr_evidential_ranking_bwd_f32(const float* mu, const float* var, int64_t stride,
                                  const float* targets, const int32_t* seg_off, int Q, int max_len,
                                  const float* gloss, float* dmu, float* dvar, int64_t dstride,
                                  rr_stream_t stream);

/* RankNet pairwise logistic, 'sum_session' (train/train_pairwise.py:99-122):
 * loss_sum = sum over queries with >= 1 positive pair of sum_ij pos*log(1+e^{-s d}) + neg*log(1+e^{s d});
 * pairs = total ordered pairs of those queries (:106).  partial is [2*Q] floats. */
int rr_ranknet_fwd_f32(const float* score, int64_t score_stride, const float* targets,
                       const int32_t* seg_off, int Q, int max_len, float sigma,
                       float* loss_sum, int64_t* pairs, float* partial, rr_stream_t stream);
/* mode 0: dscore = gloss * d(loss_sum)/d(score)   (what autograd gives 'sum_session')
 * mode 1: dscore = gloss * lambda_i, the 'accelerate_grad' row sums (train_pairwise.py:125-133) */
int rr_ranknet_bwd_f32(const float* score, int64_t score_stride, const float* targets,
                       const int32_t* seg_off, int Q, int max_len, float sigma, int mode,
                       const float* gloss, float* dscore, int64_t dscore_stride, rr_stream_t stream);

/* LambdaRank (additive: three new symbols, the ABI revision stays 8): RankNet's pair cost with every pair weighted by the
 * |delta NDCG| of swapping the two candidates in the current predicted order.  It is this library's own definition (the
 * reference trainer has none).  Per query, with k = C for ndcg_k == 0 and min(ndcg_k, C) otherwise:
 *   r_i     1-based rank of i by score, descending, ties by list position (rr_ranking_metrics_f32's `order`)
 *   D_i     1 / log2(1 + r_i) for r_i <= k, else 0
 *   g_i     exp(t_i - max_j t_j)                                  (compute_NDCG's gains; the shift cancels below)
 *   maxDCG  sum_{p = 1..k} g_(p) / log2(1 + p), g_(p) the p-th largest gain
 *   w_ij    |g_i - g_j| |D_i - D_j| / maxDCG                      (constants: no gradient flows through them)
 *   C_ij    softplus(-sigma (s_i - s_j)) for t_i > t_j, softplus(sigma (s_i - s_j)) for t_i < t_j, 0 for t_i == t_j, with
 *           the stable softplus(x) = max(x, 0) + log1p(exp(-|x|))
 *   loss_sum = sum over queries and ordered pairs i != j of w_ij C_ij;  pairs = sum over queries of 2 #{(i, j): t_i > t_j},
 * RankNet's count.  A query without a pair (empty, one candidate, all targets equal) adds 0 to both, and every gradient
 * entry it owns is WRITTEN as 0 (dscore may be uninitialised memory).  partial is [2 * Q] (loss as a float, pairs as an
 * int32), finished in a fixed order: run-to-run identical bits, no float atomics.  LDS 20 * max_len bytes.
 *   fwd   loss_sum and pairs.
 *   bwd   dscore = gloss[0] * d loss_sum / d score.
 *   step  one launch: loss = scale * loss_sum, pairs, and dscore = scale * d loss_sum / d score - the bits of fwd followed
 *         by bwd with *gloss == scale.  `scale` is a host value (a trainer passes 1 / the window's pair count, so the losses
 *         and gradients of the shards of a window add up).  `counter` as for rr_listmle_step_f32: ONE device word per
 *         concurrent launch, zero (or a multiple of Q) when the launch starts, left at zero.
 * Status: RR_ERR_ARG for a null pointer, a stride < 1, Q < 0, sigma <= 0 or ndcg_k < 0; max_len > 8192 ->
 * RR_ERR_UNSUPPORTED, nothing is launched; Q == 0 writes a zero loss and zero pairs (fwd, step) or launches nothing (bwd). */
int rr_lambdarank_fwd_f32(const float* score, int64_t score_stride, const float* targets,
                          const int32_t* seg_off, int Q, int max_len, float sigma, int ndcg_k,
                          float* loss_sum, int64_t* pairs, float* partial /* [2*Q] */, rr_stream_t stream);
int rr_lambdarank_bwd_f32(const float* score, int64_t score_stride, const float* targets,
                          const int32_t* seg_off, int Q, int max_len, float sigma, int ndcg_k,
                          const float* gloss, float* dscore, int64_t dscore_stride, rr_stream_t stream);
int rr_lambdarank_step_f32(const float* score, int64_t score_stride, const float* targets,
                           const int32_t* seg_off, int Q, int max_len, float sigma, int ndcg_k, float scale,
                           float* loss, int64_t* pairs, float* partial /* [2*Q] */, unsigned int* counter,
                           float* dscore, int64_t dscore_stride, rr_stream_t stream);

/* Soft ranks and ApproxNDCG (additive: eight new symbols, the ABI revision stays 8).  This library's own definitions (the
 * reference trainer has neither).  For one query of C candidates with float32 scores s and a temperature T > 0, in score units
 * (a T that is large against the spread of the scores blurs every rank towards (C + 1) / 2):
 *   u_ij    (s_j - s_i) / T
 *   r_i     1 + sum_{j != i} sigmoid(u_ij)                         the soft rank; ties get equal ranks, sum_i r_i = C (C + 1) / 2
 *   d L / d s_k = (1 / T) sum_{j != k} sigmoid'(u_kj) (a_j - a_k)   for an upstream gradient a_i = d L / d r_i (sigmoid' is even);
 *                                                                  it sums to zero over the query
 * ApproxNDCG writes NDCG on the soft ranks.  With targets t, k = C for ndcg_k == 0 and min(ndcg_k, C) otherwise:
 *   g_i     exp(t_i - max_j t_j)                                   (rr_lambdarank_fwd_f32's gains and maxDCG)
 *   maxDCG  sum_{p = 1..k} g_(p) / log2(1 + p), g_(p) the p-th largest gain
 *   G_i     g_i / maxDCG
 *   psi(r)  1 / log2(1 + r)                                        for ndcg_k == 0 or ndcg_k >= C
 *           sigmoid(k + 1/2 - r) / log2(1 + r)                     for 0 < ndcg_k < C: a smooth gate, one rank wide and fixed
 *   loss_q  1 - sum_i G_i psi(r_i),   a_i = -G_i psi'(r_i),   and d loss_q / d s follows from the soft-rank formula.
 * A query is RANKED when some t_i > t_j (RankNet's pairs_q > 0).  An unranked query (empty, one candidate, all targets equal)
 * adds 0 to the loss and to `ranked`, and every gradient entry it owns is WRITTEN as 0 (dscore may be uninitialised memory).
 * Arithmetic: per pair, in float32, the margin, one expf, e = exp(-|u|), sigmoid = 1 / (1 + e) or e / (1 + e) by the sign of u
 * and sigmoid' = e / (1 + e)^2; the sums over j, every O(C) quantity (gain, maxDCG, log2, gate, psi' - stored once as a
 * float) and the loss sum in float64.  One workgroup per query: one wavefront for max_len <= 64, four above.  partial is
 * [2 * Q] (loss_q as a float, ranked as an int32), finished in a fixed order: run-to-run identical bits, no float atomics.
 * LDS 20 * max_len bytes (soft ranks: 4, their backward: 8).
 *   soft_rank_fwd   rank[i * rank_stride] = r_i.
 *   soft_rank_bwd   dscore = d L / d score for drank = d L / d rank.
 *   fwd     loss_sum = sum_q loss_q, ranked = the number of ranked queries.
 *   bwd     dscore = gloss[0] * d loss_sum / d score.
 *   step    one launch: loss = scale * loss_sum, ranked, and dscore = scale * d loss_sum / d score - the bits of fwd followed by
 *           bwd with *gloss == scale.  `scale` is a host value (a trainer passes 1 / the window's query count, so the losses
 *           and gradients of the shards of a window add up).  `counter` as for rr_listmle_step_f32.
 *   ranks   a[i * a_stride] = a_i, the gradient of loss_sum in the soft ranks (0 for an unranked query).
 *   waves / set_waves   the wave count of the launches that follow: 0 = by max_len as above, 1 or 4 = that count whatever the
 *           length.  One process-wide word that every launch reads, NOT thread-safe: set it from one thread with no launch
 *           of this family in flight on another; it is there for the bench tool and the tests, to time and compare both
 *           forms of one build.  set_waves returns RR_ERR_ARG for anything else.
 * Status: RR_ERR_ARG for a null pointer, a stride < 1, Q < 0, a temperature that is not a positive finite number with a
 * finite float32 reciprocal (the kernels multiply the margins by 1 / T: T >= 2.94e-39 = 1 / FLT_MAX, inside the subnormals) or
 * ndcg_k < 0; max_len > 8192 -> RR_ERR_UNSUPPORTED, nothing is launched; Q == 0 writes a zero loss and count (fwd, step) or
 * launches nothing. */
int rr_soft_rank_fwd_f32(const float* score, int64_t score_stride, const int32_t* seg_off, int Q, int max_len,
                         float temperature, float* rank, int64_t rank_stride, rr_stream_t stream);
int rr_soft_rank_bwd_f32(const float* score, int64_t score_stride, const int32_t* seg_off, int Q, int max_len,
                         float temperature, const float* drank, int64_t drank_stride, float* dscore, int64_t dscore_stride,
                         rr_stream_t stream);
int rr_approx_ndcg_fwd_f32(const float* score, int64_t score_stride, const float* targets,
                           const int32_t* seg_off, int Q, int max_len, float temperature, int ndcg_k,
                           float* loss_sum, int64_t* ranked, float* partial /* [2*Q] */, rr_stream_t stream);
int rr_approx_ndcg_bwd_f32(const float* score, int64_t score_stride, const float* targets,
                           const int32_t* seg_off, int Q, int max_len, float temperature, int ndcg_k,
                           const float* gloss, float* dscore, int64_t dscore_stride, rr_stream_t stream);
int rr_approx_ndcg_step_f32(const float* score, int64_t score_stride, const float* targets,
                            const int32_t* seg_off, int Q, int max_len, float temperature, int ndcg_k, float scale,
                            float* loss, int64_t* ranked, float* partial /* [2*Q] */, unsigned int* counter,
                            float* dscore, int64_t dscore_stride, rr_stream_t stream);
int rr_approx_ndcg_ranks_f32(const float* score, int64_t score_stride, const float* targets,
                             const int32_t* seg_off, int Q, int max_len, float temperature, int ndcg_k,
                             float* a, int64_t a_stride, rr_stream_t stream);
int rr_approx_ndcg_waves(void);
int rr_approx_ndcg_set_waves(int waves);

/* Pointwise: nn.MSELoss (train/train_listwise.py:166-167) and GaussDisLoss (train/loss.py:154-162).
 * partial: rr_pointwise_partial_count(n) floats. */
int64_t rr_pointwise_partial_count(int64_t n);
int rr_mse_fwd_f32(const float* pred, int64_t stride, const float* targets, int64_t n,
                   float* loss, float* partial, rr_stream_t stream);
int rr_mse_bwd_f32(const float* pred, int64_t stride, const float* targets, int64_t n,
                   const float* gloss, float* dpred, int64_t dstride, rr_stream_t stream);
int rr_gauss_nll_fwd_f32(const float* mean, const float* var, int64_t stride, const float* targets,
                         int64_t n, float* loss, float* partial, rr_stream_t stream);
int rr_gauss_nll_bwd_f32(const float* mean, const float* var, int64_t stride, const float* targets,
                         int64_t n, const float* gloss, float* dmean, float* dvar, int64_t dstride,
                         rr_stream_t stream);

/* The reference trainer's remaining losses (train/loss.py:102-141, 165-314, 355-474; train/train_listwise.py:274-279).
 * Same list description as above: seg_off[Q+1], max_len <= 8192 (RR_ERR_UNSUPPORTED above), per-query partials [Q]
 * finished in a fixed order (no float atomics: run-to-run identical bits).  Every per-candidate input has its own
 * element stride (a column view of the model output is read in place); gradients are written at d[i * dstride].
 * `loss` = sum over queries of the query's loss / Q (an empty query adds 0 and still counts).  Backward entries write
 * *gloss times the gradient of that.  Status: RR_ERR_ARG for a null pointer, a stride < 1 or a negative size.
 *
 * MLEDisLoss (:102-141), mean = mu, var = variance; sorted by target (descending, ties by index):
 *   L_q = mean_j log sum_{i>=j} exp(s_i - s_j + (v_i + v_j) / 2)
 * Listnet_For_Gauss (:233-272): L_q = mean_i softmax(t)_i log sum_j exp(s_j - s_i + (v_i + v_j) / 2)
 * Listnetlognorm (:275-314):    L_q = mean_i softmax(t)_i log sum_j (s_j / s_i) exp((v_i + v_j) / 2) */
int rr_mledis_fwd_f32(const float* mean, int64_t mean_stride, const float* var, int64_t var_stride, const float* targets,
                      const int32_t* seg_off, int Q, int max_len, float* loss, float* partial /* [Q] */, rr_stream_t stream);
int rr_mledis_bwd_f32(const float* mean, int64_t mean_stride, const float* var, int64_t var_stride, const float* targets,
                      const int32_t* seg_off, int Q, int max_len, const float* gloss, float* dmean, float* dvar,
                      int64_t dstride, rr_stream_t stream);
int rr_listnet_gauss_fwd_f32(const float* mean, int64_t mean_stride, const float* var, int64_t var_stride,
                             const float* targets, const int32_t* seg_off, int Q, int max_len, float* loss,
                             float* partial /* [Q] */, rr_stream_t stream);
int rr_listnet_gauss_bwd_f32(const float* mean, int64_t mean_stride, const float* var, int64_t var_stride,
                             const float* targets, const int32_t* seg_off, int Q, int max_len, const float* gloss,
                             float* dmean, float* dvar, int64_t dstride, rr_stream_t stream);
int rr_listnet_lognorm_fwd_f32(const float* mean, int64_t mean_stride, const float* var, int64_t var_stride,
                               const float* targets, const int32_t* seg_off, int Q, int max_len, float* loss,
                               float* partial /* [Q] */, rr_stream_t stream);
int rr_listnet_lognorm_bwd_f32(const float* mean, int64_t mean_stride, const float* var, int64_t var_stride,
                               const float* targets, const int32_t* seg_off, int Q, int max_len, const float* gloss,
                               float* dmean, float* dvar, int64_t dstride, rr_stream_t stream);
/* Listnet_For_evidential (:187-230): L_q = -mean_i softmax(t)_i log_softmax(s)_i (2 v_i + alpha_i) */
int rr_listnet_evidential_fwd_f32(const float* mean, int64_t mean_stride, const float* v, int64_t v_stride,
                                  const float* alpha, int64_t alpha_stride, const float* targets, const int32_t* seg_off,
                                  int Q, int max_len, float* loss, float* partial /* [Q] */, rr_stream_t stream);
int rr_listnet_evidential_bwd_f32(const float* mean, int64_t mean_stride, const float* v, int64_t v_stride,
                                  const float* alpha, int64_t alpha_stride, const float* targets, const int32_t* seg_off,
                                  int Q, int max_len, const float* gloss, float* dmean, float* dv, float* dalpha,
                                  int64_t dstride, rr_stream_t stream);
/* Listnet_with_uq (:355-399), p = s / sum(s):
 *   L_q = KLDivLoss_batchmean(log p, softmax(t)) + coef * mean_i |log(softmax(t)_i / p_i) (s_i - 1)|
 * Dirichlet_uq (:440-474), S = sum(a), p = a / S:
 *   L_q = mean_i (p_i - softmax(t)_i)^2 + p_i (1 - p_i) / (S + 1) + coef * |log(softmax(t)_i / p_i) (a_i - 1)|
 * `coef` is the annealing coefficient max_coeff * (epoch / (epochs - 1))^3, computed by the caller. */
int rr_listnet_uq_fwd_f32(const float* score, int64_t stride, const float* targets, const int32_t* seg_off, int Q,
                          int max_len, float coef, float* loss, float* partial /* [Q] */, rr_stream_t stream);
int rr_listnet_uq_bwd_f32(const float* score, int64_t stride, const float* targets, const int32_t* seg_off, int Q,
                          int max_len, float coef, const float* gloss, float* dscore, int64_t dstride, rr_stream_t stream);
int rr_dirichlet_uq_fwd_f32(const float* alpha, int64_t stride, const float* targets, const int32_t* seg_off, int Q,
                            int max_len, float coef, float* loss, float* partial /* [Q] */, rr_stream_t stream);
int rr_dirichlet_uq_bwd_f32(const float* alpha, int64_t stride, const float* targets, const int32_t* seg_off, int Q,
                            int max_len, float coef, const float* gloss, float* dalpha, int64_t dstride, rr_stream_t stream);

/* evidential_loss_new (:402-437), the normal-inverse-gamma NLL plus its regulariser, Omega = 2 beta (1 + v), d = t - mu:
 *   l = log(pi / v) / 2 - alpha log Omega + (alpha + 1/2) log(v d^2 + Omega) + lgamma(alpha) - lgamma(alpha + 1/2)
 *       + lam (|d| (2 v + alpha) - epsilon)
 * cross == 0: the four parameters and targets are n-vectors, l is taken elementwise, loss = mean over n.
 * cross == 1: the parameters are n x 1 columns against n targets (torch broadcasting): l of parameter row i against
 *   target j for all n x n pairs, loss = mean over n^2; any n (the targets stream through LDS in tiles).
 * partial: max(n, 1) floats.  n == 0 gives NaN (torch.mean of nothing).  d/dalpha uses a device digamma. */
int rr_nig_fwd_f32(const float* mu, int64_t mu_stride, const float* v, int64_t v_stride, const float* alpha,
                   int64_t alpha_stride, const float* beta, int64_t beta_stride, const float* targets, int64_t n, int cross,
                   float lam, float epsilon, float* loss, float* partial, rr_stream_t stream);
int rr_nig_bwd_f32(const float* mu, int64_t mu_stride, const float* v, int64_t v_stride, const float* alpha,
                   int64_t alpha_stride, const float* beta, int64_t beta_stride, const float* targets, int64_t n, int cross,
                   float lam, const float* gloss, float* dmu, float* dv, float* dalpha, float* dbeta, int64_t dstride,
                   rr_stream_t stream);
/* The device digamma of the NIG backward, elementwise (x > 0; NaN for x < 0, -inf at 0). */
int rr_digamma_f32(const float* x, int64_t n, float* y, rr_stream_t stream);

/* Lognorm (:165-184): mean of log(2 pi) / 2 + log(var s^2) / 2 + (log s - t)^2 / (2 var), pi as float32; the
 * reference's print of the value is not reproduced.  Exp-MSE: mean((exp(t) - exp(pred))^2), the regression_exploss
 * branch (train/train_listwise.py:274-279).  partial: rr_pointwise_partial_count(n) floats. */
int rr_lognorm_fwd_f32(const float* score, const float* var, int64_t stride, const float* targets, int64_t n,
                       float* loss, float* partial, rr_stream_t stream);
int rr_lognorm_bwd_f32(const float* score, const float* var, int64_t stride, const float* targets, int64_t n,
                       const float* gloss, float* dscore, float* dvar, int64_t dstride, rr_stream_t stream);
int rr_exp_mse_fwd_f32(const float* pred, int64_t stride, const float* targets, int64_t n, float* loss, float* partial,
                       rr_stream_t stream);
int rr_exp_mse_bwd_f32(const float* pred, int64_t stride, const float* targets, int64_t n, const float* gloss,
                       float* dpred, int64_t dstride, rr_stream_t stream);

/* Per-query ranking evaluation on the device - the metric halves of `ranking_metrics` (train/eval.py:475-555),
 * `evaluate_top_scores` (:76-177) and `calculate_ndcg` (:329-457) without the one-forward-per-query loops and the
 * Python lists; same list description as the losses.  ABI revision 6: `ratio`, `ndcg_cut`, 12 statistics per query.
 *   order[off_q + r] = position (inside its list) of the candidate ranked r-th by score, descending, ties
 *                      keeping the original order (python's stable sorted(..., reverse=True), :516-519)
 *   stats[q*RR_RANKING_NSTATS + 0..11], float64:
 *     0..6  ranking_metrics: top-1 hit, PREDICTED top-1 in the target top-25%, recall@25%, NDCG1, NDCG2, NDCG25%,
 *           NDCG_all (:521-546; exp gains, compute_NDCG :460-472, python round() for the 25% cut, NDCG2 without
 *           discount exactly as the reference computes it)
 *     7     NDCG@10 with exp2 gains of `targets` taken as relevance grades (metrics.py:54-71)
 *     8     evaluate_top_scores' third value: the TARGET's top-1 (first maximum, :133) in the predicted
 *           top-round(C*ratio) (:144-146, :156-159) - not the same quantity as stat 1
 *     9     calculate_ndcg's NDCG: gains C + 1 - predicted rank over the first ceil(C*ndcg_cut) positions of the
 *           target order (:406-425, cal_NDCG :309-325); ties by position (the reference's torch.sort leaves them open)
 *     10    calculate_ndcg's KL(softmax(targets) || softmax(score)) with un-shifted f32 exponentials (:401-404)
 *     11    evaluate_top_scores' second value: share of the predicted top-round(C*ratio) inside the target
 *           top-round(C*ratio) (:147-151); equals stat 2 at ratio = 0.25
 *   evaluate_top_scores' first value (first-maximum top-1, :133-136) is stat 0.
 * 0 <= ratio, ndcg_cut <= 1.  The trainer-level numbers are the means over queries. */
#define RR_RANKING_NSTATS 12
int rr_ranking_metrics_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off,
                           int Q, int max_len, double ratio, double ndcg_cut, int32_t* order, double* stats,
                           rr_stream_t stream);

/* Per-query rank correlation on the device (additive: three new symbols, the ABI revision stays 8): the scale-free
 * agreement of a whole predicted order with a continuous target.  This library's own definition (the reference has none).
 * Same list description as rr_ranking_metrics_f32: seg_off[Q+1], max_len <= 8192.
 *   stats[q*RR_RANK_CORR_NSTATS + 0..7], float64:
 *     0  Kendall tau-b = (P - D) / sqrt((P + D + X) (P + D + Y))
 *     1  Spearman rho on tie-averaged ranks
 *     2  reciprocal rank: 1 / (1 + predicted rank of the target's first maximum); ranks are the stable descending order, ties
 *        by list position (rr_ranking_metrics_f32's `order`)
 *     3  top-1 regret: t[first maximum of t] - t[first maximum of s] (>= 0: targets are "higher is better" here)
 *     4  P = concordant pairs        5  D = discordant pairs
 *     6  X = pairs tied in score only        7  Y = pairs tied in target only
 *   (pairs tied in both keys: C (C - 1) / 2 minus the sum of stats 4..7)
 * A pair (i, j) is ordered in a key only where > or < holds; where neither holds it is tied in that key.  A NaN is therefore
 * tied with everything: it changes values and never addresses.  The first maximum of a key is the lowest position that no
 * candidate is greater than.  Spearman: a_i = 2 (1 + #{s_j > s_i}) + #{j != i : neither < nor >} - (C + 1), the centred,
 * doubled tie-averaged rank - an integer, sum_i a_i = 0 - b_i the same on the targets, and
 *   rho = sum a_i b_i / sqrt(sum a_i^2 sum b_i^2).
 * Every count and each of the three Spearman sums is accumulated as an integer (at most C^3 = 5.5e11 at C = 8192: exact in
 * int64 and in a double; a lane's 32-bit pair counter holds at most 2^20 per candidate pass); only the final quotients and
 * square roots are float64, IEEE operations of one thread, so the values are run-to-run identical and the same in the
 * one-wave and four-wave forms.  tau-b and rho are NaN where a key is constant (a zero denominator, as scipy), so for C < 2.  A
 * list of one has reciprocal rank 1, regret 0 and counts 0; an empty list writes NaN to stats 0..3 and 0 to stats 4..7.
 * One workgroup per query: one wavefront for max_len <= 64, four above.  LDS 8 * max_len + 320 bytes.  No atomics.
 *   waves / set_waves   as rr_approx_ndcg_waves / rr_approx_ndcg_set_waves: 0 = by max_len, 1 or 4 = pinned; one
 *           process-wide word, NOT thread-safe, for the bench tool and the tests; RR_ERR_ARG for anything else.
 * Status: RR_ERR_ARG for a null pointer, score_stride < 1 or Q < 0; max_len > 8192 -> RR_ERR_UNSUPPORTED, nothing is launched;
 * Q == 0 launches nothing and returns RR_OK. */
#define RR_RANK_CORR_NSTATS 8
int rr_rank_correlation_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off,
                            int Q, int max_len, double* stats, rr_stream_t stream);
int rr_rank_correlation_waves(void);
int rr_rank_correlation_set_waves(int waves);

/* Per-candidate and per-query statistics of T >= 2 score samples of ragged lists: MC-dropout passes or ensemble members
 * (the reference's deleted run_mc_model / run_ensemble_model, SURVEY.md:35-41; this is a definition of its own, not a port).
 * Same list description as rr_ranking_metrics_f32: seg_off[Q+1], max_len <= 8192.  Sample t of candidate i (0 <= i < M =
 * seg_off[Q]) is samples[t * sample_stride + i]; sample_stride >= M.  Per candidate (length M, f32):
 *   mean       f64 sum in sample order / T, rounded once
 *   std_dev    two-pass, unbiased (ddof = 1, torch.std): sqrt(sum_t (x_t - mean_f64)^2 / (T - 1)) in f64, rounded once
 *   p_top1     share of the samples in which the candidate is its list's first maximum
 *   mean_rank  mean 1-based rank; ranks are the stable descending order, ties by list position (the rule of
 *              rr_ranking_metrics_f32's `order`), so rank 1 is the first maximum
 * qstats[q*RR_UQ_NQSTATS + 0..3], float64:
 *   0  entropy -sum p ln p of p_top1 over the list (natural log, p = 0 terms left out)
 *   1  p_top1 of the TARGET's first maximum
 *   2  p_top1 of the first maximum of `mean` (agreement of the mean ranking with the samples)
 *   3  mean of std_dev over the list
 * An empty list writes zeros.  One wavefront per list; LDS (4 + 8) * max_len bytes (96 KiB at 8192).  No atomics: the bits
 * are run-to-run identical.  Status: RR_ERR_ARG for T < 2, a null pointer, a negative size or sample_stride < max_len;
 * RR_ERR_UNSUPPORTED for max_len > 8192 or T * max_len >= 2^32 (32-bit rank sums). */
#define RR_UQ_NQSTATS 4
int rr_mc_sample_stats_f32(const float* samples, int64_t sample_stride, int T, const float* targets, const int32_t* seg_off,
                           int Q, int max_len, float* mean, float* std_dev, float* p_top1, float* mean_rank, double* qstats,
                           rr_stream_t stream);

/* The same per-candidate and per-query statistics from ONE eval-mode forward of a distributional head: candidate i of a
 * list of C scores N(mu_i, sigma_i^2), independently of the others, and everything follows analytically - no samples.  This
 * is a definition of its own (the reference has no such code).  Row i of `out` (leading dimension ld, f32) is decoded by
 * `kind` (rr_moment_kind), the variance in f64:
 *   RR_MOMENT_GAUSSIAN      mu = col 0, var = col 1             (heads 3 and 4)
 *   RR_MOMENT_LOG_VARIANCE  mu = col 0, var = exp(col 1)        (what mledis_gaussian's list term assumes)
 *   RR_MOMENT_NIG           cols mu, v, alpha, beta (head 6): aleatoric = beta / (alpha - 1), epistemic = beta / (v (alpha - 1)),
 *                           var = aleatoric + epistemic - the moment-matched Gaussian of the Student-t predictive
 * Per candidate (length M = seg_off[Q], f32):
 *   mean       the bits of column 0
 *   std_dev    sigma = sqrt(var), rounded once
 *   mean_rank  1 + sum_{j != i} Phi((mu_j - mu_i) / sqrt(sigma_i^2 + sigma_j^2)): the exact expected 1-based descending rank
 *   p_top1     sum_n w_n prod_{j != i} Phi((mu_i + sigma_i x_n - mu_j) / sigma_j) over the n_nodes probabilists' Gauss-Hermite
 *              nodes x_n with weights w_n normalised to sum 1 (numpy.polynomial.hermite_e.hermegauss), two f64 DEVICE arrays;
 *              1 <= n_nodes <= RR_UQ_MAX_NODES
 *   aleatoric_std, epistemic_std   sqrt of the two NIG variances; written for RR_MOMENT_NIG only, either may be NULL
 * Arithmetic: per pair everything is f32 - the margin and ONE erfcf, Phi(z) = 0.5f * erfcf(-z * 0.70710678f); the product over
 * j for one node, the sum over the nodes and the rank sum are f64, each rounded once.
 * qstats[q*RR_UQ_NQSTATS + 0..3] (f64) has the meanings listed at rr_mc_sample_stats_f32, formed in f64 from the rounded f32
 * outputs; mass[q] (f64) = sum_i p_top1_i.  mass is the quadrature's own diagnostic and is NOT normalised away: it is 1 when
 * the rule resolves the integrand, and it drifts when one candidate's sigma is far larger than a rival's (the integrand
 * then has a step much narrower than the node spacing).  Measured with the f64 restatement (tests/analytic_uq_ref.py):
 * variances within a factor 11 of each other (0.05 .. 0.55), lists of 2 .. 300, 32 nodes: |mass - 1| <= 2.3e-4 and p within
 * 1.5e-4 of the 128-node value; one candidate with 10x its rival's variance, 32 nodes: p error 1.7e-4; with 100x: 9e-3 at 32
 * nodes, 1.1e-3 at 128.
 * An empty list writes zeros to its qstats and mass; a list of one candidate gives p = 1 and rank 1.  A non-finite mean or
 * a non-positive variance moves no store (nothing is scattered by rank); what is written for that list is unspecified and
 * its std_dev is not a positive finite number, which is what a caller checks.
 * Grid (query, block of 256 candidates), lane = candidate; every workgroup stages mu_j, 1/sigma_j, sigma_j^2 of its list in
 * LDS, 12 * max_len bytes (96 KiB at 8192); a second launch, one wavefront per query, writes qstats and mass.  No atomics:
 * the bits are run-to-run identical.  Status: RR_ERR_ARG for a null required pointer, n_nodes outside [1, 128], an unknown
 * kind, ld below the kind's column count (2, 2, 4) or a negative size; RR_ERR_UNSUPPORTED for max_len > 8192. */
typedef enum rr_moment_kind { RR_MOMENT_GAUSSIAN = 0, RR_MOMENT_LOG_VARIANCE = 1, RR_MOMENT_NIG = 2 } rr_moment_kind;
#define RR_UQ_MAX_NODES 128
int rr_analytic_rank_stats_f32(const float* out, int64_t ld, int kind, const float* targets, const int32_t* seg_off, int Q,
                               int max_len, const double* nodes, const double* weights, int n_nodes, float* mean,
                               float* std_dev, float* p_top1, float* mean_rank, float* aleatoric_std, float* epistemic_std,
                               double* qstats, double* mass, rr_stream_t stream);

/* Does the uncertainty track the error?  err[n], unc[n] (f32, n >= 1) with their stable ascending orders order_err /
 * order_unc (int64 row indices, ties in row order: torch.sort(stable=True) on the device - sorting stays torch plumbing).
 * fractions[n_frac] (f64, device), each in [0, 1).  out[1 + 3 * n_frac] (f64, device):
 *   out[0]            Spearman rho: the Pearson correlation of the tie-averaged ranks of err and unc (scipy.stats.spearmanr);
 *                     NaN when either rank vector is constant
 *   out[1 + 3f ...]   for fraction f, k = floor(f * n): the k most uncertain rows - the first k of the stable DESCENDING
 *                     order of unc (ties by row index) - are removed; kept = n - k, mae = sum |e| / kept,
 *                     rmse = sqrt(sum e^2 / kept) over the rows that remain
 * (the reference's deleted spearman_coef / erro_confidence).  Two launches: per-block partials of RR_UQ_CAL_BLOCK rows into
 * `workspace` (at least ceil(n / RR_UQ_CAL_BLOCK) * (3 + 2 * n_frac) doubles; RR_ERR_WORKSPACE otherwise), then one
 * workgroup sums them in block order - run-to-run identical bits, no atomics. */
#define RR_UQ_CAL_BLOCK 256
int rr_uq_calibration_f64(const float* err, const float* unc, const int64_t* order_err, const int64_t* order_unc, int64_t n,
                          const double* fractions, int n_frac, void* workspace, size_t workspace_bytes, double* out,
                          rr_stream_t stream);

/* Does sigma have the right SIZE?  Pointwise calibration of a predicted (mean, std) against targets (additive: four new
 * symbols with rr_top1_sets_f32 below, the ABI revision stays 8).  This library's own definition (the reference has none).
 * mean[n], std_dev[n], target[n] (f32, device, n >= 1), sigma_scale > 0, 1 <= n_bins <= RR_GAUSS_CAL_MAX_BINS.  A row is
 * VALID when its mean and target are finite and its std_dev is finite and > 0; an invalid row is counted and adds nothing
 * else.  For a valid row, all in f64 (IEEE operations and the device's erfc, exp and log; the build has -ffp-contract=off):
 *   sigma = sigma_scale * std_dev      z = (target - mean) / sigma      pit = 0.5 * erfc(-z / sqrt 2)
 *   phi = exp(-z^2 / 2) / sqrt(2 pi)   crps = sigma * (z * (2 * pit - 1) + 2 * phi - 1 / sqrt pi)   (Gneiting & Raftery 2007)
 *   bin = min(n_bins - 1, (int)floor(pit * n_bins))
 * out[RR_GAUSS_CAL_NSUMS + n_bins] (f64, device), RAW sums over the valid rows - the caller forms the means:
 *   0  n_valid         1  n_invalid        2  sum z        3  sum z^2
 *   4  sum ln sigma    5  sum sigma^2      6  sum (target - mean)^2      7  sum crps
 *   8 ...  the n_bins counts of the PIT histogram, exact integers stored in doubles
 * Two launches, as rr_uq_calibration_f64: per-block partials of RR_UQ_CAL_BLOCK rows into `workspace` (at least
 * ceil(n / RR_UQ_CAL_BLOCK) * (RR_GAUSS_CAL_NSUMS + n_bins) doubles; RR_ERR_WORKSPACE otherwise) - a block's sums in a fixed
 * order, its histogram by integer LDS adds - then one workgroup adds the blocks' partials in block order.  No floating-point
 * atomics: run-to-run identical bits.  Status: RR_ERR_ARG for a null pointer, n < 1, n_bins outside [1, 64] or a sigma_scale
 * that is not positive and finite. */
#define RR_GAUSS_CAL_NSUMS 8
#define RR_GAUSS_CAL_MAX_BINS 64
int rr_gauss_calibration_f64(const float* mean, const float* std_dev, const float* target, int64_t n, double sigma_scale,
                             int n_bins, void* workspace, size_t workspace_bytes, double* out, rr_stream_t stream);

/* Per-list calibration and prediction sets of a top-1 probability.  Same list description as rr_rank_correlation_f32:
 * seg_off[Q+1], max_len <= 8192.  p[M] (f32, element i at p[i * p_stride]: p_top1, non-negative, summing to about 1 per
 * list), targets[M], tau >= 0 (+inf allowed).  For candidate i of a list of C:
 *   AHEAD of i   the candidates j with p_j > p_i, or with p_j == p_i and j < i: the stable descending order, ties by list
 *                position (the rule of rr_ranking_metrics_f32's `order`)
 *   rank[M]      int32: 1 + the number of candidates ahead
 *   before[M]    f64: the sum of p_j over the candidates ahead of i, taken in ASCENDING j - an ordered chain of IEEE
 *                additions, so a definition and not an approximation
 *   in_set[M]    uint8: before_i <= tau
 * Every term is non-negative and rounding is monotone, so `before` is non-decreasing in rank: the set is a prefix of the
 * predicted order, and it holds the candidate of rank 1 (before = 0) for every tau >= 0.
 *   stats[q*RR_TOP1_NSTATS + 0..8], float64; the true top is the first maximum of the targets, the predicted top the
 *   candidate of rank 1:
 *     0  hit: 1 where the predicted top is the true top, else 0
 *     1  confidence: p of the predicted top           2  p of the true top
 *     3  rank of the true top                          4  Brier score sum_i (p_i - [i is the true top])^2, ascending i
 *     5  conformity score E = before of the true top: the probability mass ranked STRICTLY ahead of it
 *     6  set size #{i : in_set_i}                      7  covered: 1 where the true top is in the set, else 0
 *     8  mass sum_i p_i, ascending i
 * covered <=> E <= tau holds exactly: both come from the one stored `before`.  An empty list writes NaN to stats 0..5 and 0
 * to stats 6..8, and so does a list longer than max_len (nothing of it is staged).  A NaN in p is ahead of nothing and has nothing ahead; it and a negative p change values and never an
 * address (a caller checks its p; with several candidates of rank 1 the predicted top is the lowest position).
 * One workgroup per query: one wavefront for max_len <= 64, four above; thread = candidate, strided, and a candidate's chain
 * lives in one thread, so both forms write the same bits.  LDS 4 * max_len + 96 bytes (p only).  No atomics.
 *   waves / set_waves   as rr_rank_correlation_waves / rr_rank_correlation_set_waves: 0 = by max_len, 1 or 4 = pinned; one
 *           process-wide word, NOT thread-safe, for the bench tool and the tests; RR_ERR_ARG for anything else.
 * Status: RR_ERR_ARG for a null pointer, p_stride < 1, Q < 0, or a tau that is negative or a NaN; max_len > 8192 ->
 * RR_ERR_UNSUPPORTED, nothing is launched; Q == 0 launches nothing and returns RR_OK. */
#define RR_TOP1_NSTATS 9
int rr_top1_sets_f32(const float* p, int64_t p_stride, const float* targets, const int32_t* seg_off, int Q, int max_len,
                     double tau, int32_t* rank, double* before, uint8_t* in_set, double* stats, rr_stream_t stream);
int rr_top1_sets_waves(void);
int rr_top1_sets_set_waves(int waves);

/* Atom / bond attributions (additive: three new symbols, the ABI revision stays 8).  This library's own definition.
 * The adjoint of a layer's FIRST linear map, fused with the product by the layer's input and a per-row reduction over column
 * segments, so the dense input gradient need not be written:
 *   dX[m,k]   = sum_n dz[m,n] * w[n,k]  (+ add[add_idx[m], k] when add != NULL)        m < M, k < K, n < N
 *   attr[m,s] (+)= alpha * sum_{k in segment s} x[m,k] * dX[m,k]                        when attr != NULL (x required)
 *   dx[m,k]   (+)= alpha * dX[m,k]                                                      when dx != NULL
 * dz [M,N] (ld_dz), w [N,K] (ld_w: the torch Linear.weight layout; a column window of a wider weight is a pointer offset plus
 * ld_w), x [M,K] (ld_x), add [*,K] (ld_add) indexed through add_idx (int32 [M], device; every entry must name a row of add),
 * attr [M,n_seg] (ld_attr), dx [M,K] (ld_dx); all f32 device memory.  seg_end: HOST array of n_seg <= RR_ATTR_MAX_SEG ascending
 * column ends, the last equal to K (read only when attr != NULL).  accumulate (0 / 1) applies to both outputs.
 * K <= RR_ATTR_MAX_K (RR_ERR_UNSUPPORTED above); N >= 1 is any value; M == 0 returns RR_OK without a launch; any leading
 * dimension >= the logical width is accepted (16-byte loads are used where a pointer and its pitch allow, 4-byte loads
 * otherwise - same values).  The bytes between the logical width and the pitch of an operand never reach a result.
 * Arithmetic: f32 throughout on v_mfma_f32_16x16x4_f32 (one rounding per product); the chain of dX[m,k] runs over n in tiles
 * of 16 ascending, inside a tile n = 16 t + 4 q + j for j = 0..3 (outer), q = 0..3 (inner); then + add; a segment sum is four
 * per-lane chains over the columns 16 kt + 4 q + e (kt, then e ascending; q = 0..3 the lane) joined as (q0 + q1) + (q2 + q3)
 * - no atomics, and a row's bits depend on that row's operands and (N, K, segments) only: not on M, not on the row's position.
 * Status: RR_ERR_ARG for a null dz / w, both outputs null, attr without x or seg_end, add without add_idx (or the reverse),
 * seg_end not strictly ascending or not ending at K, n_seg outside [1, 4], a leading dimension below its width, M < 0,
 * N < 1, K < 1 or accumulate outside {0, 1} - all before any launch.
 *   rr_input_attribution_max_k   RR_ATTR_MAX_K as the library was compiled (the Python layer checks its widths against it) */
#define RR_ATTR_MAX_K 128
#define RR_ATTR_MAX_SEG 4
int rr_input_attribution_f32(const float* dz, int64_t ld_dz, const float* w, int64_t ld_w, const float* x, int64_t ld_x,
                             const float* add, int64_t ld_add, const int32_t* add_idx, int64_t M, int N, int K,
                             const int32_t* seg_end, int n_seg, float alpha, int accumulate, float* attr, int64_t ld_attr,
                             float* dx, int64_t ld_dx, rr_stream_t stream);
int rr_input_attribution_max_k(void);

/* The finish of an attribution: per-row terms -> atom, bond and molecule numbers of one packed graph.
 *   attr_fa [nA] (element a at attr_fa[a * ld_fa]): the atom's own term (the W_o call)
 *   attr_fb [nB,2] (ld_fb >= 2): per directed bond, column 0 the source-atom columns' term, column 1 the bond columns' term
 *   a2b [nA,K] (incoming bonds, right-padded with bond 0), b2revb [nB], a_scope [M,2] (first atom, atom count) - the packer's
 *   atom[a]      = attr_fa[a] + attr_fb[b2revb[a2b[a,0]], 0] + ... + attr_fb[b2revb[a2b[a,K-1]], 0]: one f32 chain in column
 *                  order (the bonds that LEAVE a are the reverses of its incoming ones; a padding entry names bond 0, whose
 *                  row is zero because f_bonds row 0 is)
 *   bond[b]      = attr_fb[b,1]                 bond_sym[b] = bond[b] + bond[b2revb[b]]
 *   mol_total[m] = f64: 0.0 + c_a for the molecule's atoms in ascending order, c_a = (double)atom[a] + (double)bond[b] over the
 *                  real (non-padding) entries of a2b[a,:] in column order, b = b2revb[a2b[a,k]]
 * One wavefront per molecule, lane = atom (strided); workgroup 0 also writes atom 0 / bond 0 (the padding rows).  A directed
 * bond leaves exactly one atom, so every output element is written once.  No atomics: bit-reproducible.  An index outside
 * its table reads row 0 instead (values change, never an address).
 * Status: RR_ERR_ARG for a null pointer (a_scope / mol_total may be null when M == 0), nA < 1, nB < 1, M < 0, K < 1,
 * ld_fa < 1 or ld_fb < 2. */
int rr_attribution_reduce_f32(const float* attr_fa, int64_t ld_fa, const float* attr_fb, int64_t ld_fb, const int32_t* a2b,
                              const int32_t* b2revb, const int32_t* a_scope, int64_t nA, int64_t nB, int64_t M, int K,
                              float* atom, float* bond, float* bond_sym, double* mol_total, rr_stream_t stream);

/* Nearest-neighbour search over reaction embeddings (additive: seven new symbols, the ABI revision stays 8).  This library's
 * own definition.  For query rows q [M,H] (ld_q) and bank rows bank [N,H] (ld_b), all f32 device memory:
 *   d(m,n) = max(0, (qn[m] + bn[n]) - 2 * dot(m,n))                                           all f32
 *   qn[m] = sum_h q[m,h]^2      bn[n] = sum_h bank[n,h]^2      dot(m,n) = sum_h q[m,h] * bank[n,h]
 * A pair (m,n) is EXCLUDED when the group arrays are given and q_group[m] == b_group[n] >= 0 (int32 device arrays, both NULL
 * or both given; a negative id never matches), or when d(m,n) is a NaN.  For every row m the k non-excluded bank rows that are
 * smallest under the total order (d ascending, then n ascending): dist [M,k] f32 ascending, idx [M,k] int32, both dense.  When
 * fewer than k rows qualify the remaining slots hold dist = +inf, idx = -1; a bank row whose distance overflowed to +inf is an
 * ordinary candidate (after every finite one, before the padding).  Every element of both outputs is written.  The [M,N]
 * distance matrix is never formed: distances come tile by tile from the matrix core and a sorted list per query row (one
 * wavefront lane per slot, hence RR_KNN_MAX_K = 64) takes them in.
 * Arithmetic: dot on v_mfma_f32_16x16x4_f32 (f32, one rounding per product); its chain runs over h in tiles of 16 ascending,
 * inside a tile h = 16 t + 4 c + j with j = 0..3 outer (one instruction each) and c = 0..3 inside the instruction; the
 * columns from H to the next multiple of 16 enter as zeros.  qn / bn (rr_row_sqnorm_f32, also run inside the search): 64
 * chains, chain l = 0.0f + x[l]^2 + x[l+64]^2 + ... (each square rounded, then added), joined by the butterfly over lane
 * distances 32, 16, 8, 4, 2, 1.  So the bits of d(m,n) depend on row m of q, row n of the bank and H only: not on M, N, the
 * rows' positions, the pitches, the pointers' alignment, the number of bank splits or the grid.  No atomics, nothing depends
 * on an order of arrival: run-to-run identical.
 * Limits: k in [1, RR_KNN_MAX_K] (RR_ERR_UNSUPPORTED above); H >= 1 is any value; N <= 2^31 - 1 (RR_ERR_UNSUPPORTED above);
 * any pitch >= H is accepted (16-byte loads where a pointer and its pitch allow, 4-byte loads otherwise - same values); the
 * bytes between H and the pitch never reach a result.  M == 0 returns RR_OK without a launch; N == 0 writes the padding.
 *   rr_row_sqnorm_f32        out[r] = sum_h x[r,h]^2 by the chain above, so that a bank's norms are computed once and kept
 *   rr_knn_workspace_bytes   bytes of caller-owned scratch one search of this shape needs UNDER THE CURRENT SPLIT SETTING: the
 *                            query norms, the bank norms (used when bank_sqnorm == NULL) and the per-split lists [M, S, k]
 *   rr_knn_f32               the search; bank_sqnorm [N] may be NULL (then computed into the workspace by the same chain);
 *                            nothing is retained after the call's work has run
 *   rr_knn_geometry          query rows per workgroup, bank rows per tile and RR_KNN_MAX_K as the library was compiled
 *   rr_knn_splits / rr_knn_set_splits   how many contiguous ranges the bank is cut into (grid = row tiles x splits, the lists
 *                            of a row merged by a second kernel under the same order): 0 = automatic (two workgroups per CU, at
 *                            least four bank tiles per split), 1 .. 1024 fixed (never more than bank tiles).  The result is the
 *                            same bits for every value; a process-wide word, NOT thread-safe, for the bench tool and the tests.
 * Status, all before any launch: RR_ERR_ARG for a null q / bank / dist / idx / workspace / x / out / bytes, one group array
 * without the other, a negative M, N or rows, H < 1, k < 1, a pitch below H or a split count outside [0, 1024];
 * RR_ERR_UNSUPPORTED as above; RR_ERR_WORKSPACE for a workspace below rr_knn_workspace_bytes. */
#define RR_KNN_MAX_K 64
int rr_row_sqnorm_f32(const float* x, int64_t ld, int64_t rows, int H, float* out, rr_stream_t stream);
int rr_knn_workspace_bytes(int64_t M, int64_t N, int k, size_t* bytes);
int rr_knn_f32(const float* q, int64_t ld_q, int64_t M, const float* bank, int64_t ld_b, int64_t N, int H, int k,
               const int32_t* q_group, const int32_t* b_group, const float* bank_sqnorm, float* dist, int32_t* idx,
               void* workspace, size_t workspace_bytes, rr_stream_t stream);
void rr_knn_geometry(int* row_tile, int* bank_tile, int* max_k);
int rr_knn_splits(void);
int rr_knn_set_splits(int splits);

/* Greedy k-center selection over reaction embeddings (additive: four new symbols, the ABI revision stays 8).  This library's
 * own definition.  For pool rows x [P,H] (ld), f32 device memory, pick n_pick rows one after the other, each the row that lies
 * farthest (optionally times a weight) from everything that init_dist stands for and from every row picked before it.
 * Distance of row i to a centre row c, all f32, every difference, product and sum rounded on its own:
 *   columns are cut into groups of four, group g = columns 4g .. min(4g+3, H-1); lane l of a 64-lane wavefront owns the groups
 *   with g mod 64 == l and walks them ascending, the columns inside a group ascending:
 *     acc = 0.0f;   t = x[i,h] - x[c,h];   acc = acc + t * t
 *   the 64 chains are joined by the butterfly over lane distances 32, 16, 8, 4, 2, 1 (acc = acc + acc of lane ^ distance).
 * So the bits of d(i,c) depend on the two rows and H only: not on P, the rows' positions, ld, the pointer's alignment, the
 * grid or the blocks setting.  (Not knn's |q|^2 + |b|^2 - 2 q.b: the difference form has no cancellation, and d(i,i) = 0.)
 * State: min_dist[i] = init_dist ? init_dist[i] : +inf, but NaN for a row that holds any non-finite value; assign[i] = -1.
 * Row i is ELIGIBLE in a round when it has not been taken, min_dist[i] is not a NaN and, with weights, 0 < weight[i] < +inf;
 * its score is s_i = weight ? weight[i] * min_dist[i] : min_dist[i].  Round t = 0 .. n_pick-1 takes the eligible row i that is
 * largest under the total order (score descending, then i ascending): picks[t] = i, gain[t] = s_i; then every row r whose
 * min_dist is not a NaN and for which d(r,i) < min_dist[r] (strict) gets min_dist[r] = d(r,i), assign[r] = t.  With no eligible
 * row left picks[t] = -1 and gain[t] = -1.0f.  Every element of picks, gain [n_pick] and min_dist, assign [P] is written.  A
 * picked row ends at min_dist = 0, as do its exact duplicates, which stay eligible and are taken last, in index order.
 * How it runs: n_pick + 1 launches of one kernel on `stream`, nothing else - no host synchronisation, no copy to the host, no
 * atomics, nothing that depends on an order of arrival, no workgroup that waits for another.  Launch 0 writes the state (the one
 * extra read of the pool: it finds the non-finite rows) and scores round 0; launch t reads the (score, index) pair every
 * workgroup of launch t-1 left in the workspace, reduces them to the winner in every workgroup alike, keeps the winner's columns
 * in registers (H <= 1024; wider rows re-read them) and streams the pool once: one wavefront per row, rows grid-strided, four
 * rows per workgroup and grid pass (256 threads).  16-byte loads where x and ld allow, 4-byte loads otherwise - same values;
 * the bytes between H and ld never reach a result.
 * Limits: n_pick <= RR_KCENTER_MAX_PICKS and P <= 2^31 - 1 (RR_ERR_UNSUPPORTED above); H >= 1 is any value.  P == 0 writes the
 * padding of picks / gain; n_pick == 0 still writes min_dist / assign.
 *   rr_kcenter_workspace_bytes   bytes of caller-owned scratch: the pairs of two launches at the largest grid plus one byte
 *                                per row; it does not depend on the blocks setting; nothing is retained after the call's work
 *   rr_kcenter_blocks / rr_kcenter_set_blocks   workgroups per launch: 0 = automatic (two rows per wavefront and launch at
 *                                least, 4 workgroups per CU at most), 1 .. 4096 fixed.  The result is the same bits for every
 *                                value; a process-wide word, NOT thread-safe, for the bench tool and the tests.
 * Status, all before any launch: RR_ERR_ARG for a null x / picks / gain / min_dist / assign / workspace / bytes, a negative P
 * or n_pick, H < 1, ld < H or blocks outside [0, 4096]; RR_ERR_UNSUPPORTED as above; RR_ERR_WORKSPACE for a workspace below
 * rr_kcenter_workspace_bytes. */
#define RR_KCENTER_MAX_PICKS 65536
int rr_kcenter_workspace_bytes(int64_t P, int n_pick, size_t* bytes);
int rr_kcenter_f32(const float* x, int64_t ld, int64_t P, int H, int n_pick,
                   const float* init_dist,   /* [P] or NULL (= +inf everywhere) */
                   const float* weight,      /* [P] or NULL (= 1 everywhere)    */
                   int32_t* picks, float* gain,          /* [n_pick] each */
                   float* min_dist, int32_t* assign,     /* [P] each      */
                   void* workspace, size_t workspace_bytes, rr_stream_t stream);
int rr_kcenter_blocks(void);
int rr_kcenter_set_blocks(int blocks);

/* Neighbours within a radius (additive: two new symbols, the ABI revision stays 8).  This library's own definition.  For query
 * rows q [M,H] (ld_q) and bank rows bank [N,H] (ld_b), f32 device memory:
 *   count[m] = #{ n : (m,n) not excluded and d(m,n) <= r2 }                                    int32 [M], every element written
 * d(m,n) is rr_knn_f32's distance, bit for bit - max(0, (qn[m] + bn[n]) - 2 * dot(m,n)) with the same chains on
 * v_mfma_f32_16x16x4_f32 - and the exclusion is rr_knn_f32's: q_group[m] == b_group[n] >= 0 (both arrays or neither), or a NaN
 * distance.  A row compared with itself is counted like any other pair (knn's form leaves a rounding residue there, so at a
 * very small r2 a row may not count itself; give every row its own group id to leave it out for certain).  At r2 = +inf a
 * distance that overflowed to +inf counts and a NaN (inf - inf, a row that holds an infinity) does not.  The tile walk is
 * rr_knn_f32's (one copy of it in csrc/knn.hip); instead of a sorted list every lane compares the distances it holds against r2
 * and keeps integers, summed over the workgroup at the end of the walk.  With more than one bank split the partial counts [M,S]
 * go to the workspace and a second kernel sums them in split order.  No atomics; the same counts for every split count
 * (rr_knn_set_splits governs this entry too), pitch, alignment and position of the rows.
 *   rr_radius_count_workspace_bytes   the query norms, the bank norms and the partial counts UNDER THE CURRENT SPLIT SETTING
 *   rr_radius_count_f32               bank_sqnorm [N] may be NULL, as in rr_knn_f32.  M == 0 returns RR_OK without a launch;
 *                                     N == 0 writes zeros.
 * Status, all before any launch: RR_ERR_ARG for a null q / bank / count / workspace / bytes, one group array without the other,
 * a negative M or N, H < 1, a pitch below H, or an r2 that is a NaN or negative (+inf is allowed); RR_ERR_UNSUPPORTED for M or N
 * above 2^31 - 1; RR_ERR_WORKSPACE for a workspace below rr_radius_count_workspace_bytes. */
int rr_radius_count_workspace_bytes(int64_t M, int64_t N, size_t* bytes);
int rr_radius_count_f32(const float* q, int64_t ld_q, int64_t M, const float* bank, int64_t ld_b, int64_t N, int H, float r2,
                        const int32_t* q_group, const int32_t* b_group, const float* bank_sqnorm, int32_t* count,
                        void* workspace, size_t workspace_bytes, rr_stream_t stream);

/* Sphere-exclusion clustering (Taylor-Butina with a density key, the leader algorithm without one) over reaction embeddings
 * (additive: four new symbols, the ABI revision stays 8).  This library's own definition.  For pool rows x [P,H] (ld), f32
 * device memory, a squared radius r2 >= 0 (+inf allowed) and an optional int32 key per row:
 * Distance: d(i,c) is rr_kcenter_f32's difference chain, bit for bit (one copy of it, csrc/row_chain.h) - NOT knn's distance:
 * the difference form gives d(c,c) = 0, so a centre always joins its own cluster and every non-padding round assigns at least
 * one row.
 * State: labels[i] = -2 for a row that holds any non-finite value (never eligible, never a member), every other row starts at -1.
 * Round t takes the row c with labels == -1 that is largest under the total order (key descending, then index ascending;
 * key == NULL: every key equal, so index order): centres[t - first_round] = c, and every row i with labels[i] == -1 and
 * d(i,c) <= r2 gets labels[i] = t.  With no row at -1 left centres[t - first_round] = -1 and nothing else changes.  The keys are
 * read as given and never updated (Butina uses the initial neighbour counts).
 * What holds afterwards: every member lies within r2 of its centre, and two centres lie farther than r2 apart (both in this
 * chain's f32 arithmetic).  What does NOT: two members of different clusters may lie within r2 of each other.
 * How it runs: launches of one kernel back to back on `stream`, nothing else - no host synchronisation, no copy to the host, no
 * atomics, no workgroup that waits for or signals another.  first_round == 0: one initial launch writes the state (the one extra
 * read of the pool: it finds the non-finite rows) and leaves every workgroup's best (key, index) pair in the workspace; then one
 * launch per round reads the pairs of the launch before it (two arrays, used alternately), reduces them to the winner in every
 * workgroup alike (workgroup 0 writes the centre), keeps the centre's columns in registers (H <= 1024; wider rows re-read them)
 * and streams only the rows still at -1 - the label is read first, then the row: one wavefront per row, rows grid-strided,
 * four rows per workgroup and grid pass (256 threads).  16-byte loads where x and ld allow, 4-byte loads otherwise - same
 * values; the bytes between H and ld never reach a result.
 * first_round > 0 CONTINUES: labels and the workspace must be what the previous call on the same x / ld / P / H / r2 / key left
 * (rounds 0 .. first_round-1 done), so that a caller can run rounds in batches and look at the last centre in between.  The
 * blocks setting may differ between such calls.
 * Results are the same bits for every blocks setting, row pitch, pointer alignment and position of the rows in a larger pool.
 * Limits: n_rounds <= RR_SPHERE_EXCLUSION_MAX_ROUNDS per call, P <= 2^31 - 1 and first_round + n_rounds <= 2^31 - 1
 * (RR_ERR_UNSUPPORTED above); H >= 1 is any value.  P == 0 writes the padding of centres; n_rounds == 0 with first_round == 0
 * still writes labels.
 *   rr_sphere_exclusion_workspace_bytes   the pairs of two launches at the largest grid; independent of the blocks setting
 *   rr_sphere_exclusion_blocks / rr_sphere_exclusion_set_blocks   workgroups per launch: 0 = automatic (rr_kcenter_f32's rule),
 *                                1 .. 4096 fixed; a process-wide word, NOT thread-safe, for the bench tool and the tests.
 * Status, all before any launch: RR_ERR_ARG for a null x / labels / centres / workspace / bytes, a negative P, first_round or
 * n_rounds, H < 1, ld < H, an r2 that is a NaN or negative, or blocks outside [0, 4096]; RR_ERR_UNSUPPORTED as above;
 * RR_ERR_WORKSPACE for a workspace below rr_sphere_exclusion_workspace_bytes. */
#define RR_SPHERE_EXCLUSION_MAX_ROUNDS 65536
int rr_sphere_exclusion_workspace_bytes(int64_t P, size_t* bytes);
int rr_sphere_exclusion_f32(const float* x, int64_t ld, int64_t P, int H, float r2,
                            const int32_t* key,        /* [P] or NULL (= equal keys: index order) */
                            int first_round, int n_rounds,
                            int32_t* labels,           /* [P] state and result */
                            int32_t* centres,          /* [n_rounds]: rounds first_round .. first_round+n_rounds-1 */
                            void* workspace, size_t workspace_bytes, rr_stream_t stream);
int rr_sphere_exclusion_blocks(void);
int rr_sphere_exclusion_set_blocks(int blocks);

/* Resampled column means of a per-query table: bootstrap intervals and paired sign-flip tests (additive: four new symbols, the
 * ABI revision stays 8).  This library's own definition.  x [Q,M] (ld >= M) is f64 device memory, one row per query, one column
 * per statistic (the tables of rr_ranking_metrics_f32 / rr_rank_correlation_f32, or differences of two such tables).
 * The draw stream - splitmix64's finaliser, NOT the dropout hash, whose four elements per first-level word are correlated:
 *   mix64(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^ (z >> 31)    (mod 2^64)
 *   word(seed, n) = mix64(mix64(seed) + (n + 1) * 0x9E3779B97F4A7C15 mod 2^64),   n = 0, 1, 2, ...
 *   draw(seed, j) = high 32 bits of word(seed, j >> 1) for even j, low 32 bits for odd j            (uint64 j)
 *   Qe = Q rounded up to even;  resample b, position i (0 <= i < Q)  ->  j = b * Qe + i              (uint64 arithmetic)
 *   row(b, i)  = (draw * Q) >> 32                        (bootstrap)
 *   sign(b, i) = +1 if bit 31 of draw is 0, else -1      (sign flip)
 * row() is not exactly uniform: a row gets floor or ceil of 2^32 / Q of the 2^32 draw values, a relative non-uniformity of at
 * most Q / 2^32 - hence Q <= 2^20 (2.4e-4 at the limit, 2.3e-5 at 10^5 queries; RR_ERR_UNSUPPORTED above).
 * The sums, all f64, every addition rounded on its own: lane l of a 64-lane wavefront owns the positions i of a resample with
 * i mod 64 == l and walks them ascending; per column c it keeps acc = +0.0 and n = 0:
 *   bootstrap:  v = x[row(b,i), c];  if v is not a NaN:  acc = acc + v,               n = n + 1
 *   sign flip:  v = x[i, c];         if v is not a NaN:  acc = acc + sign(b,i) * v,   n = n + 1
 * the 64 chains are joined by the butterfly over lane distances 32, 16, 8, 4, 2, 1 (acc = acc + acc of lane ^ distance, the
 * same for n);  mean[k,c] = acc / n, NaN when n == 0;  count[k,c] = n.  +-inf entries take part in the sums.  Output row k is
 * resample b = b0 + k, so a caller may cut B into calls and gets the rows of the uncut call bit for bit.  The bits of a result
 * depend on x's values, Q, the column, seed and b only: not on ld, the pointer's alignment, B, where b0 cuts, the grid, the
 * blocks setting or the width of the loads.
 * How it runs: one launch on `stream` (none when B == 0), one wavefront per resample, resamples grid-strided, 256 threads; no
 * atomics, no host synchronisation, no workspace, nothing that depends on an order of arrival.  Every element of mean (and of
 * count when given) is written; Q == 0 gives NaN / 0 everywhere.  16-byte loads where x and ld allow, 8-byte loads otherwise -
 * same values; nothing at or past column M of a row is read.
 *   rr_resample_blocks / rr_resample_set_blocks   workgroups per launch: 0 = automatic (one resample per wavefront up to a
 *                            cap by the table's size Q M 8: 4096 workgroups up to 32 KiB, two per CU up to 4 MiB, beyond that one
 *                            per CU for the bootstrap and three per two CUs for the sign flip - measured),
 *                            1 .. 4096 fixed.  The result is the same bits for every value; a process-wide
 *                            word, NOT thread-safe, for the bench tool and the tests.
 *   rr_resample_draw_host    draw(seed, j) on the host, so a test can hold the stream against its numpy restatement.
 * Status, all before any launch: RR_ERR_ARG for a null x (with Q > 0) or mean, a negative Q, B or b0, M < 1, ld < M, an unknown
 * mode or blocks outside [0, 4096]; RR_ERR_UNSUPPORTED for M > RR_RESAMPLE_MAX_COLS, Q > 2^20 or (b0 + B) * Qe not below 2^63. */
#define RR_RESAMPLE_MAX_COLS 32
#define RR_RESAMPLE_BOOTSTRAP 0
#define RR_RESAMPLE_SIGNFLIP  1
int rr_resample_means_f64(const double* x, int64_t ld, int64_t Q, int M,      /* [Q, M], ld >= M, device */
                          int mode, uint64_t seed, int64_t b0, int64_t B,
                          double* mean,      /* [B, M] */
                          int32_t* count,    /* [B, M] or NULL */
                          rr_stream_t stream);
int rr_resample_blocks(void);
int rr_resample_set_blocks(int blocks);
uint32_t rr_resample_draw_host(uint64_t seed, uint64_t j);

/* A Gaussian model of the embedding space: second moments of the rows of a matrix, and the centred projection with a fused row
 * norm that Mahalanobis distances, whitening and PCA scores are (additive: six new symbols, the ABI revision stays 8).  This
 * library's own definition.
 *
 * rr_col_moments_f64.  x [N,H] (ld >= H) is f32 device memory.  Row n is USED when every one of its H values is finite; a row
 * that holds a NaN or an infinity takes part in nothing below and is not counted.
 *   n_used     = the number of used rows (one int64 on the device)
 *   mean [H]   = column sums of the used rows / n_used, f64;  all +0.0 when n_used == 0
 *   scatter [H,H] = sum over the used rows of c_n c_n^T, c_n[h] = (double)x[n,h] - mean[h] (one rounding), f64, row-major, dense.
 * The caller divides by n_used - ddof.  Every element of the three outputs is written; N == 0 or no used row gives n_used = 0,
 * mean and scatter all +0.0.  scatter is EXACTLY symmetric: only j <= i is computed, scatter[j][i] is a copy.
 * Chunks: the rows are cut into C contiguous chunks of L = ceil(N / C) rows (chunk c = rows c L .. min(N, (c+1) L) - 1) with
 *   C = max(1, min(64, ceil(N / 1024), floor(2^28 / (8 Hp^2)))),  Hp = H rounded up to a multiple of 64
 * (a slab of Hp^2 doubles per chunk, 256 MiB of slabs at most) - a function of N and H only (rr_moments_chunks).
 * The mean's chain, all f64, every addition rounded on its own: inside chunk c, row lane q = 0..15 owns the rows c L + q,
 * c L + q + 16, ... and walks them ascending, acc = +0.0, acc = acc + (double)x[n,h] for a used row (+ 0.0 for another); the 16
 * sums are added in ascending q starting from lane 0's; the chunks' sums are added to +0.0 in ascending c; one division by n_used.
 * The scatter's chain, all f64: inside chunk c the rows are taken four at a time in ascending order (c L .. c L + 3, ...; a row
 * that is not used, or past the chunk's end, enters as exact zeros, which change no bit of a sum), one
 * v_mfma_f64_16x16x4_f64 per group of four rows and 16 x 16 tile, accumulating from +0.0: the matrix core adds the four products
 * c_n[i] c_n[j], n ascending, to the running sum.  The instruction's internal rounding (the ISA documents a fused multiply-add
 * per product, i.e. one rounding per term) was not held against a software chain on the card; tests/test_gpu_moments.py bounds
 * the result for either reading.  The chunks' tiles are added to +0.0 in ascending c.
 * So the bits depend on x's values, N and H only: not on ld, the pointer's alignment, the grid or the blocks setting.  No
 * atomics, nothing depends on an order of arrival: run-to-run identical.  Five launches on `stream` (four when N == 0), no host
 * synchronisation.  16-byte loads where x and ld allow, 4-byte loads otherwise - same values; the bytes between H and ld never
 * reach a result.
 * Limits: H <= RR_MOMENTS_MAX_H and N <= 2^31 - 1 (RR_ERR_UNSUPPORTED above).
 *   rr_moments_workspace_bytes   bytes of caller-owned scratch: one byte per row, the chunks' column sums and row counts and the
 *                                chunks' slabs; it does not depend on the blocks setting; nothing is retained after the call's work
 *   rr_moments_chunks            C of the formula above (0 for arguments the call would refuse)
 *   rr_moments_blocks / rr_moments_set_blocks   workgroups of the grid-strided launches (the row flags, the mean, the finish, and
 *                                rr_center_project_f32's row tiles): 0 = automatic (four per CU at most), 1 .. 4096 fixed.  The
 *                                result is the same bits for every value; a process-wide word, NOT thread-safe, for the bench
 *                                tool and the tests.
 * Status, all before any launch: RR_ERR_ARG for a null x / mean / scatter / n_used / workspace / bytes, a negative N, H < 1,
 * ld < H or blocks outside [0, 4096]; RR_ERR_UNSUPPORTED as above; RR_ERR_WORKSPACE for a workspace below
 * rr_moments_workspace_bytes.
 *
 * rr_center_project_f32.  y[n,r] = sum_h (x[n,h] - center[h]) * W[h,r] and sq[n] = sum_r y[n,r]^2, all f32.  x [N,H] (ld >= H),
 * center [H] or NULL (= zeros), W [H,R] row-major and dense, 1 <= R <= H; y [N,R] dense or NULL, sq [N] or NULL, at least one
 * given.  With y == NULL the [N,R] product is never written: four bytes per row leave the kernel.
 * Arithmetic: t = x[n,h] - center[h] rounded in f32; the dot on v_mfma_f32_16x16x4_f32 by rr_knn_f32's chain over h (tiles of 16
 * ascending, inside a tile h = 16 t + 4 c + j with j = 0..3 outer, one instruction each, and c = 0..3 inside the instruction;
 * the columns from H to the next multiple of 16 enter as zeros).  sq: four chains q = 0..3, chain q owns the columns r with
 * (r mod 16) div 4 == q and walks them ascending, acc = 0.0f, acc = acc + y * y (the square rounded, then added);
 * sq = (chain 0 + chain 2) + (chain 1 + chain 3).  sq is computed from the very y that is written.  So the bits of row n depend
 * on row n of x, center, W, H and R only: not on N, the row's position, ld, the pointer's alignment, the grid or the blocks
 * setting.  A non-finite value in a row propagates by plain IEEE arithmetic: a NaN gives NaN in y and sq; an infinity gives NaN
 * wherever it meets a zero or an infinity of the other sign (a dense W: sq is NaN), else an infinity.  Nothing is special-cased.
 * One launch on `stream` (none when N == 0), no workspace, no atomics.
 * Status, all before any launch: RR_ERR_ARG for a null x or W, y and sq both null, a negative N, H < 1, ld < H or R outside
 * [1, H]; RR_ERR_UNSUPPORTED for N > 2^31 - 1. */
#define RR_MOMENTS_MAX_H 1024
int rr_moments_workspace_bytes(int64_t N, int H, size_t* bytes);
int rr_moments_chunks(int64_t N, int H);
int rr_col_moments_f64(const float* x, int64_t ld, int64_t N, int H,
                       double* mean,        /* [H]    */
                       double* scatter,     /* [H, H] */
                       int64_t* n_used,     /* one value, device */
                       void* workspace, size_t workspace_bytes, rr_stream_t stream);
int rr_moments_blocks(void);
int rr_moments_set_blocks(int blocks);
int rr_center_project_f32(const float* x, int64_t ld, int64_t N, int H,
                          const float* center,   /* [H] or NULL */
                          const float* W, int R, /* [H, R] */
                          float* y,              /* [N, R] or NULL */
                          float* sq,             /* [N] or NULL */
                          rr_stream_t stream);

/* Circular (Morgan-style) fingerprints from the packed graph (additive: two new symbols, the ABI revision stays 8).  This
 * library's own definition: NOT bit-compatible with RDKit's Morgan fingerprints, and without ECFP's duplicate-substructure
 * removal.  All arithmetic on uint32 with wrap-around:
 *   fmix(x):  x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13; x *= 0xc2b2ae35; x ^= x >> 16        (murmur3's finaliser)
 *   step(h, w) = fmix((h ^ w) + 0x9e3779b9)
 *   rowhash(v[0..n)) = fold h = 0; for c ascending: h = step(h, bits(v[c]))     bits = the f32 pattern, -0.0 taken as +0.0
 *   id_0[a] = rowhash(f_atoms[a, 0:atom_fdim])          bh[b] = rowhash(bond_cols[b, 0:bond_fdim])
 *   round r = 1..radius, atom a: m_k = step(bh[b], id_{r-1}[b2a[b]]) over the incoming bonds b = a2b[a,k] != 0 (bond 0 is the
 *     padding bond), S = sum_k m_k, X = xor_k fmix(m_k ^ 0x7f4a7c15), id_r[a] = step(step(step(id_{r-1}[a], r), S), X)
 * Both joins are commutative: the ids do not depend on the numbering of atoms or bonds.  Every (a, r), r = 0..radius, a an atom of
 * molecule m (a_scope[m] = (first atom, atoms); atom 0 is padding and never contributes) contributes j = id_r[a] % num_bits to
 * row m: bits_out [M, num_bits / 32] uint32 (ld_bits in words), bit j in word j >> 5 at position j & 31, and / or counts_out
 * [M, num_bits] int32 (ld_counts).  Either may be NULL, not both.  Every word of a row is written; a molecule without atoms
 * gives a zero row.  bond_cols are the bond-only columns: f_bonds + atom_fdim with f_bonds' pitch, or a [nB, bond_fdim] array.
 * One wavefront per molecule, the ids and the row in LDS, plain stores at the end (molecules above 256 atoms keep their ids in
 * the workspace): no global atomics, and a row depends on its molecule only - not on its position in the batch, the other
 * molecules, the grid or what output and workspace held.  A bond index outside [1, nB) is skipped; a neighbour outside the
 * molecule's own atoms is read as its first atom; a scope outside [1, nA) gives a zero row (values change, never an address).
 * Status, all before any launch: RR_ERR_ARG for a null f_atoms / bond_cols / a2b / b2a / workspace / bytes, a null a_scope with
 * M > 0, both outputs null, nA < 1, nB < 1, M < 0, K < 1, a feature width < 1, a pitch below its width, radius < 0, or num_bits
 * below 32 or not a multiple of 32; RR_ERR_UNSUPPORTED for radius > RR_FP_MAX_RADIUS, num_bits > RR_FP_MAX_BITS or nA, nB, M
 * above 2^31 - 1; RR_ERR_WORKSPACE for a workspace below rr_circular_fp_workspace_bytes.  M == 0 returns RR_OK without a launch. */
#define RR_FP_MAX_RADIUS 8
#define RR_FP_MAX_BITS 8192
int rr_circular_fp_workspace_bytes(int64_t nA, int64_t nB, size_t* bytes);
int rr_circular_fp_u32(const float* f_atoms, int64_t ld_fa, int atom_fdim, const float* bond_cols, int64_t ld_bc, int bond_fdim,
                       const int32_t* a2b, int K, const int32_t* b2a, const int32_t* a_scope, int64_t nA, int64_t nB, int64_t M,
                       int radius, int num_bits, uint32_t* bits_out /* nullable */, int64_t ld_bits,
                       int32_t* counts_out /* nullable */, int64_t ld_counts, void* workspace, size_t workspace_bytes,
                       rr_stream_t stream);

/* Tanimoto search on bit rows (additive: eight new symbols, the ABI revision stays 8).  This library's own definition.  For query
 * rows q [M,W] (ld_q) and bank rows bank [N,W] (ld_b), uint32 words in device memory, pitches in words:
 *   c = popcount(q[m] & bank[n])     u = |q[m]| + |bank[n]| - c     d(m,n) = u == 0 ? 0 : (float)(u - c) / (float)u
 * one correctly rounded f32 division of exact integers: d = 1 - Tanimoto similarity, and two empty rows are at distance 0.
 * Order, group exclusion (q_group[m] == b_group[n] >= 0), padding (dist = +inf, idx = -1) and the bank splits with their merge
 * are rr_knn_f32's (one copy of the list, csrc/topk_list.h): dist [M,k] ascending, ties to the lower bank index; the same bits
 * for every split count, pitch, alignment and position of the rows; no atomics.  16-byte loads where a pointer and its pitch
 * allow, 4-byte loads otherwise; the words between W and the pitch never reach a result.
 *   rr_row_popcount_u32                out[r] = |x[r]|, int32: what the searches take as bank_popcount (NULL: computed into the
 *                                      workspace)
 *   rr_tanimoto_knn_u32                the search; k in [1, RR_KNN_MAX_K]; N == 0 writes the padding; M == 0 launches nothing
 *   rr_tanimoto_count_u32              count[m] = number of non-excluded bank rows with d(m,n) <= radius (radius >= 0, +inf
 *                                      allowed); N == 0 writes zeros
 *   rr_tanimoto_knn_workspace_bytes / rr_tanimoto_count_workspace_bytes   the popcounts and the per-split partial results UNDER
 *                                      THE CURRENT SPLIT SETTING
 *   rr_tanimoto_splits / rr_tanimoto_set_splits   as rr_knn_set_splits: 0 = automatic, 1 .. 1024 fixed; process-wide, NOT
 *                                      thread-safe, for the bench tool and the tests
 *   rr_tanimoto_geometry               query rows per workgroup, bank rows per tile, RR_KNN_MAX_K, RR_TANIMOTO_MAX_WORDS
 * Status, all before any launch: RR_ERR_ARG for a null q / bank / dist / idx / count / workspace / x / out / bytes, one group
 * array without the other, a negative M, N or rows, W < 1, k < 1, a pitch below W, a radius that is negative or a NaN, or a split
 * count outside [0, 1024]; RR_ERR_UNSUPPORTED for k > RR_KNN_MAX_K, W > RR_TANIMOTO_MAX_WORDS or N (count: M or N) above
 * 2^31 - 1; RR_ERR_WORKSPACE for a workspace below the sizer's value. */
#define RR_TANIMOTO_MAX_WORDS 256
int rr_row_popcount_u32(const uint32_t* x, int64_t ld, int64_t rows, int W, int32_t* out, rr_stream_t stream);
int rr_tanimoto_knn_workspace_bytes(int64_t M, int64_t N, int k, size_t* bytes);
int rr_tanimoto_knn_u32(const uint32_t* q, int64_t ld_q, int64_t M, const uint32_t* bank, int64_t ld_b, int64_t N, int W, int k,
                        const int32_t* q_group, const int32_t* b_group, const int32_t* bank_popcount, float* dist, int32_t* idx,
                        void* workspace, size_t workspace_bytes, rr_stream_t stream);
int rr_tanimoto_count_workspace_bytes(int64_t M, int64_t N, size_t* bytes);
int rr_tanimoto_count_u32(const uint32_t* q, int64_t ld_q, int64_t M, const uint32_t* bank, int64_t ld_b, int64_t N, int W,
                          float radius, const int32_t* q_group, const int32_t* b_group, const int32_t* bank_popcount,
                          int32_t* count, void* workspace, size_t workspace_bytes, rr_stream_t stream);
void rr_tanimoto_geometry(int* row_tile, int* bank_tile, int* max_k, int* max_words);
int rr_tanimoto_splits(void);
int rr_tanimoto_set_splits(int splits);

/* How many launches of the one-wavefront-per-list kernels (losses, task step, pairwise, uncertainty) have so far opted in
 * to more than 64 KiB of dynamic LDS, in this process.  A kernel stages up to 20 bytes per candidate, so lists above 3276
 * to 5461 candidates need the opt-in, once per kernel and template instantiation.  Today's HIP runtime launches without it
 * too, so this count is where a missing one shows; the long-list tests read it. */
long long rr_lds_opt_ins(void);

/* LogCumsumExp along dim 0 of a 1-D tensor (train/loss.py:9-61); n <= 8192.
 * backward keeps the reference's un-shifted exp(x) (:59). */
int rr_logcumsumexp_fwd_f32(const float* x, int n, float* y, rr_stream_t stream);
int rr_logcumsumexp_bwd_f32(const float* x, const float* y, const float* gy, int n, float* gx,
                            rr_stream_t stream);

/* ------------------------------------------------------------------ graph packing (HOST) */
/* BatchMolGraph.__init__ (features/featurization.py:246-288) as one native call over
 * concatenated per-molecule arrays; ALL pointers here are HOST memory.
 *   in : mol_atoms[M], mol_bonds[M]               atoms / directed bonds per molecule
 *        f_atoms_cat[sum atoms, atom_fdim], f_bonds_cat[sum bonds, bond_fdim]
 *        b2a_local, b2revb_local [sum bonds]      molecule-local indices
 *        a2b_off[sum atoms + 1], a2b_local[...]   incoming-bond lists (CSR, molecule-local)
 *        K_override: 0 -> K = max(1, max in-degree) (:281); else pad width to use (>= that)
 *   out: sizes via rr_pack_sizes; arrays with the padding row 0 (:255-264):
 *        f_atoms[nA, ld_fa], f_bonds[nB, ld_fb] (rows zero-padded to the given ld),
 *        a2b[nA,K], b2a[nB], b2revb[nB], a2a[nA,K] (= b2a[a2b], :326-327), a_scope[M,2],
 *        and the backward tables: a2b_rev_t[nA,K] (b2revb[a2b], pads -1, row0 = {0,-1..}),
 *        b2t[nB] (target atom b2a[b2revb[b]]; b2t[0] = -1), a2a_t[nA,K] (a2a with pads -1),
 *        npad[nA] (float, K - deg; npad[0] = K), atom2mol[nA] (-1 for the pad row). */
int rr_pack_sizes(const int32_t* mol_atoms, const int32_t* mol_bonds, int64_t M,
                  const int64_t* a2b_off, int K_override,
                  int64_t* nA, int64_t* nB, int32_t* K);
int rr_pack_graphs(const int32_t* mol_atoms, const int32_t* mol_bonds, int64_t M,
                   const float* f_atoms_cat, int atom_fdim, const float* f_bonds_cat, int bond_fdim,
                   const int32_t* b2a_local, const int32_t* b2revb_local,
                   const int64_t* a2b_off, const int32_t* a2b_local, int K,
                   float* f_atoms, int64_t ld_fa, float* f_bonds, int64_t ld_fb,
                   int32_t* a2b, int32_t* b2a, int32_t* b2revb, int32_t* a2a, int32_t* a_scope,
                   int32_t* a2b_rev_t, int32_t* b2t, int32_t* a2a_t, float* npad, int32_t* atom2mol);
/* Backward tables for a batch that already exists as padded arrays (e.g. a reference
 * BatchMolGraph's tensors converted to int32); HOST pointers. */
int rr_derive_tables(const int32_t* a2b, const int32_t* b2a, const int32_t* b2revb,
                     int64_t nA, int64_t nB, int K, const int32_t* a_scope, int64_t M,
                     int32_t* a2a, int32_t* a2b_rev_t, int32_t* b2t, int32_t* a2a_t,
                     float* npad, int32_t* atom2mol);

/* ------------------------------------------------------------------ FFN head as one launch (ABI revision 8) --- */
/* The FFN head (models/base_model.py:32-60) and its input-gradient chain: up to RR_MAX_FFN dependent small GEMMs - one row per
 * molecule - in ONE launch; a workgroup owns 16 rows and walks every stage, the activations stay in LDS between stages
 * (csrc/ffn.hip).  Stage s computes  y = x_s W_s^T (+ bias) [ReLU] [dropout]  on the f32 MFMA with W_s in the packed layout of
 * rr_pack_weights_f32 (split = 0: [n_out][r16(n_in)] zero-padded), writes y to `out` (may be NULL except for the last stage)
 * and hands  x_{s+1} = post_mask ? (post_mask > 0 ? y * mask_scale : 0) : y  to the next stage, which reads its first n_in
 * columns.  rowdot = 1 (last stage only, n_out <= 8, n_in % 4 == 0, plain row-major weight rows of pitch ldw): the 16-lane dot
 * product of the scorer's last Linear.  Results are bit-identical to the same layers issued one by one through
 * rr_linear_f32 (M <= 8192 geometry or not).  Forward chain: stages = the Linear layers, ReLU + dropout on all but the last
 * (rowdot); backward chain: stages = the layers in reverse with their transposed packs, post_mask = the forward layer's
 * output below.  Returns RR_ERR_UNSUPPORTED for shapes it does not take (unaligned rows, n_out % 4 != 0, widths > 1024):
 * issue the layers one by one then. */
#ifndef RR_MAX_FFN
#define RR_MAX_FFN 8
#endif
typedef struct rr_ffn_stage {
  const float* w;  int64_t ldw;       /* packed weight [n_out][ldw], ldw = r16(n_in) (rowdot: any row-major [n_out][ldw >= n_in]) */
  const float* bias;                  /* [n_out] or NULL */
  int n_out, n_in;
  int relu, dropout, rowdot;
  uint64_t drop_seed;                 /* dropout stream of this stage (rate: rr_ffn_chain_args.drop_p; element m * n_out + n) */
  float* out;  int64_t ld_out;        /* y [M, ld_out] or NULL */
  const float* post_mask;  int64_t ld_mask;   /* [M, ld_mask] or NULL */
} rr_ffn_stage;
typedef struct rr_ffn_chain_args {
  int64_t M;
  int n_stages;
  const float* x;  int64_t ldx;       /* input of stage 0: [M, ldx], its first stage[0].n_in columns */
  float drop_p, mask_scale;
  rr_ffn_stage stage[RR_MAX_FFN];
} rr_ffn_chain_args;
size_t rr_abi_ffn_chain_size(void);
int rr_ffn_chain_f32(const rr_ffn_chain_args* args, rr_stream_t stream);

/* ------------------------------------------------------------------ whole-model step plans --- */
/* ReactionModel.forward (models/base_model.py:150-171: encoder on reactants and products, p_h - r_h, diff encoder,
 * readout, FFN + head) and its explicit backward as ONE call each: the host-side orchestration of the per-op entry
 * points above (operand wiring, dropout stream seeds, the weight-gradient / reactant-encoder streams and their events)
 * for hosts that should not - or cannot - issue ~140 launches per training step themselves.  All activations live in ONE
 * caller-provided workspace whose layout is a pure function of (model, step): rr_reaction_backward re-derives every
 * saved address, the library keeps no state between the two calls.  Requirements: H % 4 == 0, 16-byte aligned rows
 * (what the packer produces); other shapes use the per-op entry points.  Device pointers unless noted.
 * A data-parallel step is forward, loss kernel, backward, then ONE all-reduce of the gradient buffers handed to
 * rr_reaction_backward (rr_allreduce_f32 below, or the host's own collective - the Python mirror uses torch.distributed). */
#ifndef RR_MAX_FFN
#define RR_MAX_FFN 8
#endif

typedef struct rr_graph {             /* a packed batch resident in HBM (arrays of rr_pack_graphs / rr_derive_*) */
  int64_t nA, nB, M;
  int K, Kb;
  const float* f_atoms;  int64_t ld_fa;
  const float* f_bonds;  int64_t ld_fb;    /* may be NULL for rr_step.r in RR_STEP_PREFIX mode (only u.f_bonds is read) */
  const int32_t *a2b, *b2a, *b2revb, *a2a, *a_scope, *b2t, *a2a_t, *atom2mol, *b2b_t;
  const float *npad, *npad_b;
  const float* fb_sum;   int64_t ld_fbs;   /* sum_k f_bonds[a2b[a,k]] [nA, ld_fbs] (input-only; needed when diff_depth > 1) */
} rr_graph;

typedef struct rr_linear_w {          /* one nn.Linear: weight [out, in] row-major with row stride ldw, bias [out] or NULL */
  const float* w;
  const float* b;
  int out, in;
  int64_t ldw;
} rr_linear_w;

typedef struct rr_model {
  int H, depth, diff_depth, n_ffn, head;          /* head: rr_head of the FFN output (0 = none) */
  int atom_fdim, bond_fdim;                       /* 61, 83 (= 61 + 22) */
  rr_linear_w enc_wi, enc_wh, enc_wo;             /* MPN     (models/mpn.py:40-59);  enc_wh unused when depth == 1 */
  rr_linear_w dif_wi, dif_wh, dif_wo;             /* MPNDiff (models/mpn.py:161-168) */
  rr_linear_w ffn[RR_MAX_FFN];                    /* FFN Linear layers in order (models/base_model.py:32-57) */
} rr_model;

enum { RR_STEP_PLAIN = 0,    /* encoder(r) on the full reactant batch */
       RR_STEP_DEDUP = 1,    /* dropout inactive: `r` holds the DISTINCT reactants, amap / amap_t map product atoms to them */
       RR_STEP_PREFIX = 2 }; /* train mode: `u` holds the distinct reactants, only the deterministic prefix is shared */
enum { RR_PLAN_NO_SIDE_STREAM = 1, RR_PLAN_NO_AUX_STREAM = 2,
       RR_PLAN_F32_GEMM = 4,         /* encoder GEMMs on the f32 matrix core instead of the three-bf16-term path (w_packed = 2);
                                        forward and backward of a step must agree on it (it changes the workspace layout) */
       RR_PLAN_AUX_BACKWARD = 8,     /* reactant-encoder backward on the aux stream beside the product pass */
       RR_PLAN_TRAIN = 16,           /* a backward WILL follow: rr_reaction_forward also packs the transposed weights of the
                                        input-gradient GEMMs, in the same launch as the forward's packs, so the backward
                                        starts with its first GEMM instead of a pack.  Layout-changing like RR_PLAN_F32_GEMM:
                                        pass the same flags to both calls (ABI revision 6). */
       RR_PLAN_F16X2_GEMM = 32,      /* encoder GEMMs and weight gradients on two f16 terms per operand (w_packed = 3: half the
                                        matrix instructions of the three-bf16-term path, 22 significant bits per operand); the
                                        plan finds every operand's largest magnitude itself (rr_amax_f32, one slot per tensor
                                        in the workspace).  Ignored with RR_PLAN_F32_GEMM; layout-changing (ABI revision 7). */
       RR_PLAN_NO_FFN_CHAIN = 64,    /* the FFN head's layers as separate launches instead of rr_ffn_chain_f32 (same results
                                        bit for bit, same workspace layout: an A/B knob; ABI revision 8) */
       RR_PLAN_TIME = 128,           /* measurement: HIP events on the launch stream around every split-GEMM and gather-sum launch
                                        of this call, collected by rr_plan_timing_take (costs ~5 us of stream time per launch:
                                        not for timed runs; ABI revision 8) */
       RR_PLAN_WGRAD_EARLY = 256 };  /* rr_reaction_backward only: the W_h weight gradient of a message-passing layer is issued in
                                        front of that layer's input-gradient GEMM instead of behind it (both read the same dZ).
                                        Same kernels, same order on the weight-gradient stream, same workspace layout, same bits;
                                        which order is faster depends on the workload (-1.3 % ... +2.4 % on the step over the four
                                        BASELINE configurations, profiles/r05_experiments.txt item 19): a host may time both and
                                        keep the better one, as reactranker_amd.functions.WgradOrder does (ABI revision 8) */

typedef struct rr_step {
  rr_graph p, r, u;
  int mode;
  const int32_t* amap;    const int32_t* amap_t;  int amap_t_cols;    /* RR_STEP_DEDUP */
  const int32_t* bmap;    const int32_t* bmap_t;  int bmap_t_cols;    /* RR_STEP_PREFIX */
  const float* feat;      int F;                  /* add_features [M, F] or NULL */
  float drop_p;           uint64_t seed;          /* dropout rate in effect (0 in eval mode) and the step's stream seed */
  void* workspace;        size_t workspace_bytes; /* >= rr_reaction_workspace_bytes(model, step); kept until backward */
  float* out;                                     /* [M, ffn[n_ffn-1].out] */
} rr_step;

enum { RR_G_ENC_WI = 0, RR_G_ENC_WH, RR_G_ENC_WO, RR_G_DIF_WI, RR_G_DIF_WH, RR_G_DIF_WO, RR_G_FFN0 };
typedef struct rr_grads {             /* gradient buffers, same shapes / row strides as the parameters (dense: ld = in) */
  float* w[RR_G_FFN0 + RR_MAX_FFN];
  float* b[RR_G_FFN0 + RR_MAX_FFN];   /* NULL where the layer has no bias */
} rr_grads;

/* sizeof of the four plan structs as compiled, so a binding can verify its layout. */
void rr_abi_plan_struct_sizes(size_t* graph, size_t* model, size_t* step, size_t* grads);
size_t rr_reaction_workspace_bytes(const rr_model* model, const rr_step* step);
int rr_reaction_forward(const rr_model* model, const rr_step* step, int flags, rr_stream_t stream);
int rr_reaction_backward(const rr_model* model, const rr_step* step, const float* dout, const rr_grads* grads, int flags,
                         rr_stream_t stream);

/* Per-launch durations of the heavy kernels INSIDE a step plan (RR_PLAN_TIME): what bench.py's roofline object is made of, measured
 * on the path `value` is measured on.  One record per rr_linear_f32 launch on the split path (M >= 8192) and per gather-sum launch. */
typedef struct rr_plan_timing {
  int kind;                /* 0 = rr_linear_f32 (split GEMM), 1 = rr_gather_sum_f32 / _padrow / _amax, 2 = rr_gather_sum_epi_f32 */
  int mode;                /* GEMM: 0 plain, 1 subtract operand, 2 f32 mask, 3 sign-bit mask */
  int64_t M;               /* GEMM rows / gather destination rows */
  int64_t n_src;           /* gather: source rows */
  int N, k1, k2;           /* GEMM: columns, segment widths; gather: N = H, k1 = table width K, k2 = addends */
  int residual, c_pre, dz_out, bits_out, bits_in, mask;   /* which optional operands / outputs the launch carried (0 / 1) */
  float us;                /* HIP-event time around the launch on its stream */
} rr_plan_timing;
/* Waits for the recorded launches of this process, copies up to max_n records (oldest first) and forgets them all; returns the count. */
int rr_plan_timing_take(rr_plan_timing* out, int max_n);
/* Which launches carry events under RR_PLAN_TIME: bit k of `kinds` = launches of kind k, bit m of `modes` = GEMMs of mode m (default:
 * all).  Every event pair costs its stream ~5 us and loosens the overlap between the streams: timing ONE kernel key at a time keeps a
 * step within ~1 % of an untimed one, and its durations at what rocprofv3 --kernel-trace reports for the untimed step. */
int rr_plan_timing_select(int kinds, int modes);

/* Where a step keeps an activation inside its workspace (ABI revision 6) - valid from rr_reaction_forward until the
 * workspace is reused; nothing is launched.  For hosts that want the encoder's outputs (atom hiddens, reaction vectors:
 * `return_atom_hiddens` / `vecs` of models/mpn.py:61-108, 224-238) without a second forward, and for tests that need the
 * ReLU gates this arithmetic took.  `flags` as passed to rr_reaction_forward.  *ptr = NULL when the step has no such tensor
 * (e.g. RR_SAVED_R_MSG index 0 in RR_STEP_PREFIX mode, where the first message exists per DISTINCT reactant only). */
enum { RR_SAVED_R_MSG = 0,    /* reactant encoder: message after iteration `index` (0 = relu(W_i f_bonds)) [r.nB, H], post-dropout */
       RR_SAVED_R_H = 1,      /* reactant atom hiddens [r.nA, H] */
       RR_SAVED_P_MSG = 2, RR_SAVED_P_H = 3,            /* the same for the product encoder */
       RR_SAVED_D_MSG = 4,    /* diff encoder: message after iteration `index` [p.nA, H] */
       RR_SAVED_D_HID = 5,    /* diff encoder atom hiddens [p.nA, H] */
       RR_SAVED_VECS = 6,     /* readout + add_features (after the FFN's input dropout) [M, ld] */
       RR_SAVED_FFN_H = 7,    /* FFN hidden layer `index` (1 .. n_ffn-1) [M, ld] */
       RR_SAVED_R_MSG0_U = 8, /* RR_STEP_PREFIX: relu(W_i f_bonds) of the distinct reactants [u.nB, H] */
       RR_SAVED_R_Z1_U = 9 }; /* RR_STEP_PREFIX: their first W_h layer before dropout [u.nB, H] */
int rr_reaction_saved_f32(const rr_model* model, const rr_step* step, int flags, int which, int index,
                          const float** ptr, int64_t* rows, int64_t* ld);

/* ------------------------------------------------------------------ the pairwise trainer's remaining strategies --- */
/* BetaNet and BetaNet_envidential (train/train_pairwise.py:176-338): a C x C loss per query on the first score column, list
 * description as for RankNet above (seg_off[Q+1], max_len <= 8192, RR_ERR_UNSUPPORTED above).  Matrices are oriented as the
 * reference builds them: entry (i, j) takes "alpha" from candidate j and "beta" from candidate i.
 *   BetaNet: tau = sigmoid(t), pi = sigmoid(s); x1 = tau_j / (tau_i + tau_j), x2 = tau_i / (tau_i + tau_j); (aT, bT) = alpha0 (x1, x2);
 *   (aP, bP) = alpha0 (pi_j, pi_i) / (pi_i + pi_j); lt, lp = ln Beta(aT, bT) / Beta(aP, bP) density at x1; entry = exp(lt) (lt - lp).
 *   Evidential: tau = sigmoid(t), p = s (positive); T1, T2, P1, P2 likewise, S = p_i + p_j;
 *   entry = (T1-P1)^2 + (T2-P2)^2 + (P1 (1-P1) + P2 (1-P2)) / (S + 1) + coef * 2 |ln(T1 / P1) (p_j - 1)|.
 * loss_sum = sum over queries and all C x C entries (diagonal included), pairs = sum of C^2 - C.  partial: Q doubles.
 * bwd: dscore = *gloss * d loss_sum / d score, every row written by the lane that owns it (no atomics; run-to-run identical).
 * Entries are evaluated in double.  LDS 12 * max_len bytes.  Status: RR_ERR_ARG for a null pointer, a stride < 1, a negative
 * size or alpha0 <= 0 - checked before any launch. */
int rr_betanet_fwd_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q,
                       int max_len, float alpha0, float* loss_sum, int64_t* pairs, double* partial, rr_stream_t stream);
int rr_betanet_bwd_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q,
                       int max_len, float alpha0, const float* gloss, float* dscore, int64_t dscore_stride,
                       rr_stream_t stream);
int rr_beta_evidential_fwd_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off,
                               int Q, int max_len, float coef, float* loss_sum, int64_t* pairs, double* partial,
                               rr_stream_t stream);
int rr_beta_evidential_bwd_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off,
                               int Q, int max_len, float coef, const float* gloss, float* dscore, int64_t dscore_stride,
                               rr_stream_t stream);
/* pairwise_acc and eval_cross_entropy_loss (train/eval.py:180-224, 15-73) in one pass.  qstats [Q, 4] doubles = { npos = #{t_i > t_j},
 * sum_ij |[s_i > s_j] - [t_i > t_j]|, sum over t_i != t_j of 0.5 (1 - S_ij) x - logsigmoid(-x) with x = sigma (s_i - s_j), 0 };
 * out [4] doubles = { sum over queries with npos > 0 of 1 - mismatches / (2 npos), number of those queries, sum of the
 * cross-entropy terms, sum of 2 npos }: pairwise_acc = out[0] / out[1], eval_cross_entropy_loss = out[2] / out[3]. */
int rr_pairwise_eval_f32(const float* score, int64_t score_stride, const float* targets, const int32_t* seg_off, int Q,
                         int max_len, float sigma, double* qstats, double* out, rr_stream_t stream);
/* The baseline pair loop on [B, 2] outputs y and [B, 2] targets (train_pairwise.py:27-59; row strides ldy, ldt >= 2):
 * loss = mean_b sum_k (softmax(t_b)_k - y_bk / (y_b0 + y_b1))^2; partial: rr_pair_partial_count(B) doubles.
 * rr_pair_acc_f32: 1 - mean_b |[y_b0 > y_b1] - [tp_b0 > tp_b1]| (eval.py:262-266), B >= 1. */
int64_t rr_pair_partial_count(int64_t B);
int rr_pair_softmax_mse_fwd_f32(const float* y, int64_t ldy, const float* targets, int64_t ldt, int64_t B, float* loss,
                                double* partial, rr_stream_t stream);
int rr_pair_softmax_mse_bwd_f32(const float* y, int64_t ldy, const float* targets, int64_t ldt, int64_t B,
                                const float* gloss, float* dy, int64_t ldd, rr_stream_t stream);
int rr_pair_acc_f32(const float* y, int64_t ldy, const float* targets, int64_t ldt, int64_t B, float* acc,
                    rr_stream_t stream);
/* out[row] = (h1[i1[row]] - hr[ir[row]]) + (h2[i2[row]] - hr[ir[row]]) over [n_rows, H]: the input of the pair model's
 * difference encoder (models/ranknet_baseline.py:57-61).  The three sources share the row pitch ld; a NULL index array is
 * the identity.  H % 4 == 0, pitches % 4 == 0 and 16-byte aligned pointers (RR_ERR_ALIGN otherwise). */
int rr_pair_combine_f32(const float* hr, const float* h1, const float* h2, int64_t ld, const int32_t* ir, const int32_t* i1,
                        const int32_t* i2, int64_t n_rows, int H, float* out, int64_t ld_out, rr_stream_t stream);

/* ------------------------------------------------------------------ data-parallel gradient exchange (RCCL) --- */
/* Queries are independent: one process per GPU, whole queries per rank, identical replicas, and ONE sum all-reduce of the
 * gradient buffers per optimizer step (the reference itself is single-process).  `comm` is an RCCL
 * communicator (ncclComm_t): either one the host created with the RCCL it links - pass it as is - or one made by
 * rr_comm_init_rank below.  RCCL is resolved at run time (symbols already in the process first, then librccl.so.1), so this
 * library has no link-time dependency on it; RR_ERR_UNSUPPORTED when no RCCL can be found.
 *   rr_allreduce_f32: buf[0:n] <- scale * sum over ranks of buf[0:n], in place, enqueued on `stream` (the all-reduce, then
 *   one scaling pass unless scale == 1).  With equal shards pass scale = 1 / n_ranks; with ragged shards scale the local
 *   gradient by local_count / global_count first (reactranker_amd.dp.loss_weight names the count per loss) and pass 1.
 *   rr_comm_unique_id: rank 0 fills `id` (RR_COMM_ID_BYTES host bytes) and hands it to the other ranks by any host channel;
 *   rr_comm_init_rank: collective over all ranks, each on its own current device. */
typedef void* rr_comm_t;
#define RR_COMM_ID_BYTES 128
int rr_comm_backend(void);   /* how RCCL was resolved: 0 not found, 1 symbols already in the process, 2 dlopen("librccl.so.1") */
int rr_comm_unique_id(void* id);
int rr_comm_init_rank(rr_comm_t* comm, int n_ranks, const void* id, int rank);
int rr_comm_destroy(rr_comm_t comm);
int rr_allreduce_f32(float* buf, int64_t n, float scale, rr_comm_t comm, rr_stream_t stream);
/* The same result as two collectives (ABI revision 8): reduce-scatter + all-gather, in place, over the largest prefix of the
 * bucket that divides by the communicator's rank count, the remaining < n_ranks elements through an all-reduce; then the
 * scale.  For the 3.16 / 12.1 MB buckets on xGMI's point-to-point links; which form is faster is a
 * measurement for an 8-GPU node - rr_allreduce_f32 stays the default.  With 2 ranks the bits equal rr_allreduce_f32's. */
int rr_allreduce_rsag_f32(float* buf, int64_t n, float scale, rr_comm_t comm, rr_stream_t stream);

/* Bond-to-bond backward table (HOST pointers), derived from the tables above.  The adjoint of
 *   message[b] = a_message[b2a[b]] - message[b2revb[b]],  a_message[a] = sum_k message[a2b[a,k]]   (models/mpn.py:89-92)
 * is  d message[b] = sum of d m_in over the bonds leaving atom target(b), minus d m_in[rev(b)]; rev(b) is one of those
 * bonds, so it is a plain gather-sum over  b2b_t[nB, Kb]  (the bonds leaving target(b) except rev(b); pads -1;
 * Kb >= max(1, K-1); row 0 all -1) - one pass instead of gather-sum + gather-diff.  The padding row's adjoint is the
 * weighted column sum  sum_b npad_b[b] * d m_in[b]  with  npad_b[b] = npad[b2a[b]]  (npad_b[0] = K - 1). */
int rr_derive_bond_tables(const int32_t* a2b_rev_t, const int32_t* b2t, const int32_t* b2revb, const int32_t* b2a,
                          const float* npad, int64_t nA, int64_t nB, int K, int Kb,
                          int32_t* b2b_t, float* npad_b);

#ifdef __cplusplus
}
#endif
#endif /* REACTRANKER_HIP_H */
