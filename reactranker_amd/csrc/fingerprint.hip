// Circular (Morgan-style) fingerprints from the packed graph.  A definition of this library, not a port: the
// bits are NOT RDKit's.  All arithmetic on uint32 with wrap-around:
//   fmix = rr_fmix32 (murmur3's finaliser)      step(h, w) = fmix((h ^ w) + 0x9e3779b9)
//   rowhash(v[0..n)) = fold h = 0, h = step(h, bits(v[c])) for c ascending; bits = the f32 pattern, -0.0 taken as +0.0
//   id_0[a] = rowhash(f_atoms[a, 0:atom_fdim])      bh[b] = rowhash(bond_cols[b, 0:bond_fdim])
//   round r = 1..radius: m_k = step(bh[b], id_{r-1}[b2a[b]]) over the incoming bonds b = a2b[a,k] != 0,
//     S = sum m_k, X = xor fmix(m_k ^ 0x7f4a7c15), id_r[a] = step(step(step(id_{r-1}[a], r), S), X)
//   every (a, r), a an atom of molecule m, sets bit / bumps bin id_r[a] % num_bits of row m.
//
// fp_rowhash_kernel: one thread per row of a feature matrix (atoms, then bonds) -> id_0 [nA] and bh [nB] in the workspace.  A
// row's hash is one serial chain, so a thread walks its own row, four columns per load where pointer and pitch allow.
// fp_mol_kernel: one wavefront (a 64-thread workgroup) per molecule, lane = atom (strided).  The ids of the round before and of
// the round in flight live in LDS (two arrays of FP_STAGE entries); a molecule with more atoms keeps them in two [nA] arrays of
// the workspace instead, indexed by the atom's number in the batch, written with plain stores and read - behind a device-scope
// fence and the workgroup barrier - with loads that bypass the L1.  The row under construction (the bitset and / or the bins)
// lives in LDS as well: features go in with LDS atomics (integer or / add: the order does not matter), and the finished row
// leaves with plain stores that cover every word of it.  No global atomics; nothing is read that this call has not written, so
// the row depends on the molecule alone.  A bond index outside [1, nB) is skipped like the padding bond; a neighbour outside
// the molecule's own atoms is read as its first atom; a scope outside [1, nA) gives a zero row (values change, never an address).
#include "row_chain.h"

namespace {

constexpr int FP_NT = 256;                        // threads of the row-hash pass
constexpr int FP_STAGE = 256;                     // atoms of a molecule whose ids stay in LDS
constexpr uint32_t FP_GOLD = 0x9e3779b9u, FP_XOR = 0x7f4a7c15u;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t fp_step(uint32_t h, uint32_t w) { return rr_fmix32((h ^ w) + FP_GOLD); }
__device__ __forceinline__ uint32_t fp_bits(float v) {
  const uint32_t u = __float_as_uint(v);
  return u == 0x80000000u ? 0u : u;
}

template <bool VEC>
__global__ void __launch_bounds__(FP_NT) fp_rowhash_kernel(const float* x, int64_t ld, int64_t rows, int cols, uint32_t* out) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * FP_NT + threadIdx.x;
  if (r >= rows) return;
  const float* row = x + r * ld;
  uint32_t h = 0;
  for (int c = 0; c < cols; c += 4) {
    const f32x4 v = rr_load4<VEC>(row, c, cols);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c + e < cols) h = fp_step(h, fp_bits(v[e]));
  }
  out[r] = h;
}

struct FpParams {
  const int32_t* a2b; const int32_t* b2a; const int32_t* a_scope;
  int64_t nA, nB;
  int K, radius, num_bits;
  const uint32_t* id0; const uint32_t* bh;        // workspace: the row hashes
  uint32_t* ids_a; uint32_t* ids_b;               // workspace: [nA] each, for the molecules above FP_STAGE atoms
  uint32_t* bits_out; int64_t ld_bits;            // nullable
  int32_t* counts_out; int64_t ld_counts;         // nullable
};

__global__ void __launch_bounds__(64) fp_mol_kernel(const FpParams P) {
  extern __shared__ __attribute__((aligned(16))) uint32_t fp_smem[];
  const int lane = threadIdx.x;
  const int64_t m = blockIdx.x;
  const int W = P.num_bits >> 5;
  uint32_t* const s_bits = fp_smem;                                    // [W]
  uint32_t* const s_cnt = fp_smem + W;                                 // [num_bits] when counts are asked for
  uint32_t* const s_ids = s_cnt + (P.counts_out ? P.num_bits : 0);     // [2][FP_STAGE]
  const bool want_bits = P.bits_out != nullptr, want_cnt = P.counts_out != nullptr;

  int64_t start = P.a_scope[2 * m];
  int64_t n = P.a_scope[2 * m + 1];
  if (start < 1 || n < 0 || start + n > P.nA) n = 0;                   // (uniform)
  const bool staged = n <= FP_STAGE;
  const uint32_t nb = static_cast<uint32_t>(P.num_bits);

  for (int w = lane; w < W; w += 64) s_bits[w] = 0;
  if (want_cnt)
    for (int j = lane; j < P.num_bits; j += 64) s_cnt[j] = 0;
  __syncthreads();

  auto feature = [&](uint32_t id) {
    const uint32_t j = id % nb;
    if (want_bits) atomicOr(&s_bits[j >> 5], 1u << (j & 31));
    if (want_cnt) atomicAdd(&s_cnt[j], 1u);
  };
  // id of atom `a` (its number inside the molecule) in buffer `buf`
  auto get = [&](int buf, int64_t a) -> uint32_t {
    if (staged) return s_ids[buf * FP_STAGE + a];
    const uint32_t* p = (buf ? P.ids_b : P.ids_a) + start + a;
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  auto put = [&](int buf, int64_t a, uint32_t id) {
    if (staged) s_ids[buf * FP_STAGE + a] = id;
    else (buf ? P.ids_b : P.ids_a)[start + a] = id;
  };
  auto round_end = [&]() {
    if (!staged) __threadfence();
    __syncthreads();
  };

  for (int64_t a = lane; a < n; a += 64) {
    const uint32_t id = P.id0[start + a];
    put(0, a, id);
    feature(id);
  }
  round_end();
  for (int r = 1; r <= P.radius; ++r) {
    const int prev = (r - 1) & 1, cur = r & 1;
    for (int64_t a = lane; a < n; a += 64) {
      const int32_t* nbrs = P.a2b + (start + a) * P.K;
      uint32_t S = 0, X = 0;
      for (int k = 0; k < P.K; ++k) {
        const int64_t b = nbrs[k];
        if (b < 1 || b >= P.nB) continue;
        int64_t na = static_cast<int64_t>(P.b2a[b]) - start;
        if (na < 0 || na >= n) na = 0;
        const uint32_t mk = fp_step(P.bh[b], get(prev, na));
        S += mk;
        X ^= rr_fmix32(mk ^ FP_XOR);
      }
      const uint32_t id = fp_step(fp_step(fp_step(get(prev, a), static_cast<uint32_t>(r)), S), X);
      put(cur, a, id);
      feature(id);
    }
    round_end();
  }
  __syncthreads();
  if (want_bits)
    for (int w = lane; w < W; w += 64) P.bits_out[m * P.ld_bits + w] = s_bits[w];
  if (want_cnt)
    for (int j = lane; j < P.num_bits; j += 64) P.counts_out[m * P.ld_counts + j] = static_cast<int32_t>(s_cnt[j]);
}

struct FpLayout { size_t id0, bh, ids_a, ids_b, total; };
FpLayout fp_layout(int64_t nA, int64_t nB) {
  FpLayout L;
  size_t o = 0;
  L.id0 = o; o += rr_round256(static_cast<size_t>(nA) * 4);
  L.bh = o; o += rr_round256(static_cast<size_t>(nB) * 4);
  L.ids_a = o; o += rr_round256(static_cast<size_t>(nA) * 4);
  L.ids_b = o; o += rr_round256(static_cast<size_t>(nA) * 4);
  L.total = o > 256 ? o : 256;
  return L;
}

int fp_rowhash_launch(const float* x, int64_t ld, int64_t rows, int cols, uint32_t* out, hipStream_t s) {
  const int64_t blocks = (rows + FP_NT - 1) / FP_NT;
  rr_vec_dispatch(rr_vec4_ok(x, ld), [&](auto vec) {
    fp_rowhash_kernel<decltype(vec)::value><<<static_cast<unsigned>(blocks), FP_NT, 0, s>>>(x, ld, rows, cols, out);
  });
  return rr_launch_status();
}

}  // namespace

extern "C" {

int rr_circular_fp_workspace_bytes(int64_t nA, int64_t nB, size_t* bytes) {
  RR_CHECK_ARG(bytes && nA >= 1 && nB >= 1);
  if (nA > 0x7fffffffLL || nB > 0x7fffffffLL) return RR_ERR_UNSUPPORTED;
  *bytes = fp_layout(nA, nB).total;
  return RR_OK;
}

int rr_circular_fp_u32(const float* f_atoms, int64_t ld_fa, int atom_fdim, const float* bond_cols, int64_t ld_bc, int bond_fdim,
                       const int32_t* a2b, int K, const int32_t* b2a, const int32_t* a_scope, int64_t nA, int64_t nB, int64_t M,
                       int radius, int num_bits, uint32_t* bits_out, int64_t ld_bits, int32_t* counts_out, int64_t ld_counts,
                       void* workspace, size_t workspace_bytes, rr_stream_t stream) {
  RR_CHECK_ARG(f_atoms && bond_cols && a2b && b2a && workspace && (a_scope || M == 0));
  RR_CHECK_ARG(nA >= 1 && nB >= 1 && M >= 0 && K >= 1 && atom_fdim >= 1 && bond_fdim >= 1);
  RR_CHECK_ARG(ld_fa >= atom_fdim && ld_bc >= bond_fdim);
  RR_CHECK_ARG(radius >= 0 && num_bits >= 32 && num_bits % 32 == 0);
  RR_CHECK_ARG(bits_out || counts_out);
  RR_CHECK_ARG((!bits_out || ld_bits >= num_bits / 32) && (!counts_out || ld_counts >= num_bits));
  if (radius > RR_FP_MAX_RADIUS || num_bits > RR_FP_MAX_BITS) return RR_ERR_UNSUPPORTED;
  if (nA > 0x7fffffffLL || nB > 0x7fffffffLL || M > 0x7fffffffLL) return RR_ERR_UNSUPPORTED;
  const FpLayout L = fp_layout(nA, nB);
  if (workspace_bytes < L.total) return RR_ERR_WORKSPACE;
  if (M == 0) return RR_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  FpParams P;
  P.a2b = a2b; P.b2a = b2a; P.a_scope = a_scope;
  P.nA = nA; P.nB = nB;
  P.K = K; P.radius = radius; P.num_bits = num_bits;
  uint32_t* id0 = reinterpret_cast<uint32_t*>(ws + L.id0);
  uint32_t* bh = reinterpret_cast<uint32_t*>(ws + L.bh);
  P.id0 = id0; P.bh = bh;
  P.ids_a = reinterpret_cast<uint32_t*>(ws + L.ids_a);
  P.ids_b = reinterpret_cast<uint32_t*>(ws + L.ids_b);
  P.bits_out = bits_out; P.ld_bits = ld_bits;
  P.counts_out = counts_out; P.ld_counts = ld_counts;
  int st = fp_rowhash_launch(f_atoms, ld_fa, nA, atom_fdim, id0, s);
  if (st != RR_OK) return st;
  if (radius > 0) {
    st = fp_rowhash_launch(bond_cols, ld_bc, nB, bond_fdim, bh, s);
    if (st != RR_OK) return st;
  }
  const size_t lds = (static_cast<size_t>(num_bits / 32) + (counts_out ? num_bits : 0) + 2 * FP_STAGE) * 4;   // <= 35 KiB
  fp_mol_kernel<<<static_cast<unsigned>(M), 64, lds, s>>>(P);
  return rr_launch_status();
}

}  // extern "C"
