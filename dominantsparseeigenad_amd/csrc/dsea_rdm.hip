// dsea_rdm.hip -- reduced density matrices of a bipartition A | B of the sites (docs/design/21-reduced-density-matrix.md): the
// index-table builders k_rdm_index_sector / k_rdm_index_full, the forward k_rdm_cross (+ k_rdm_cross_reduce or
// k_rdm_cross_reduce_wide), the backward k_rdm_pull, the host arithmetic of the block structure and the launchers.
//
// Site i is bit i of a state.  `sites` lists the LA sites of A in the caller's order: bit k of the A-word a is the bit of site
// sites[k]; B is the other LB = L - LA sites in increasing order and bit k of the B-word b is the bit of site B[k].  In the
// sector of ndown set bits the reduced density matrix is block diagonal in the number m of set bits inside A,
// m = max(0, ndown - LB) .. min(LA, ndown).  Row i of block m is the i-th LA-bit word with m set bits in increasing integer
// order, column j the j-th LB-bit word with ndown - m set bits: dA_m = C(LA, m), dB_m = C(LB, ndown - m), sum_m dA_m dB_m = n.
//   M_m(x)[i, j] = x[rank(dep_A(a_i) | dep_B(b_j))]        cross(x, y)_m = M_m(x) M_m(y)^T        rho_m = cross(psi, psi)_m
// The full 2^L space is one block with dA = 2^LA, dB = 2^LB and rank = identity.
// idx (int32, n entries, block after block, j fastest): idx[off_m + i dB_m + j] = the row of (a_i, b_j) -- a permutation of
// 0 .. n - 1, built once per (sector, sites).  With it the sector and the full space are the same kernels, and a lane's four
// consecutive k of an MFMA block are one 16-byte index load and four gathers.  The block descriptors travel by value.
// One wave is one workgroup in cross and pull: everything that selects the work of a wave derives from blockIdx.
// Nothing here is shared with dsea_sector.hip: the file has its own helpers.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_internal.h"
#include "dsea_device.h"

namespace dsea {

namespace {
typedef double rdm_v4d __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) rdm_i4 {
  int32_t v[4];
};

#define DSEA_RDM_PASCAL (DSEA_SECTOR_MAX_L + 1)
#define DSEA_RDM_TARGET_WAVES 4096 /* cross: split the inner dimension until about this many waves exist (4 per SIMD) */
#define DSEA_RDM_MIN_CHUNK 64      /* ... but give no wave fewer than this many inner indices */
#define DSEA_RDM_WIDE_SPLIT 16     /* chunks per pair from which the second stage takes one wave per output element */

// the work list of k_rdm_cross: block m owns the waves wbase[m] .. wbase[m + 1] - 1 = (tile pair, chunk of the inner dimension),
// chunk fastest; nt = tiles of 16 T rows per side, chunk = inner indices per wave (a multiple of 16), nsplit = chunks
struct RdmCrossPlan {
  int32_t wbase[DSEA_RDM_MAX_BLOCKS + 1];
  int32_t nsplit[DSEA_RDM_MAX_BLOCKS], chunk[DSEA_RDM_MAX_BLOCKS], nt[DSEA_RDM_MAX_BLOCKS];
};
// the work list of k_rdm_pull: block m owns the waves wbase[m] .. = (row tile of 16 TI, column tile of 32), column fastest
struct RdmPullPlan {
  int32_t wbase[DSEA_RDM_MAX_BLOCKS + 1];
  int32_t ntj[DSEA_RDM_MAX_BLOCKS];
};

// Pascal's triangle C[i][j] = C(i, j), 0 <= j <= i <= L, zero above the diagonal, filled by the block
__device__ __forceinline__ void rdm_pascal(uint64_t (*C)[DSEA_RDM_PASCAL], int L) {
  for (int c = threadIdx.x; c < DSEA_RDM_PASCAL * DSEA_RDM_PASCAL; c += blockDim.x) (&C[0][0])[c] = 0;
  __syncthreads();
  for (int i = 0; i <= L; ++i) {
    const int j = threadIdx.x;
    if (j <= i) C[i][j] = (j == 0 || j == i) ? 1 : C[i - 1][j - 1] + C[i - 1][j];
    __syncthreads();
  }
}

// the r-th W-bit word with k set bits in increasing order, every bit j deposited at site pos[j] (greedy from the top bit)
__device__ __forceinline__ uint64_t rdm_unrank_deposit(const uint64_t (*C)[DSEA_RDM_PASCAL], uint64_t r, int W, int k,
                                                       const uint8_t* pos) {
  uint64_t s = 0;
  for (int j = W - 1; j >= 0; --j) {
    const uint64_t below = C[j][k > 0 ? k : 0];      // words of k bits that fit under bit j
    if (k > 0 && r >= below) {
      s |= 1ull << pos[j];
      r -= below;
      --k;
    }
  }
  return s;
}

// idx[off_m + i dB_m + j] = rank(dep_A(a_i) | dep_B(b_j)) through the sector's two rank tables; one entry per thread
__global__ __launch_bounds__(256) void k_rdm_index_sector(RdmSites sites, RdmBlocks blk, int ndown, int Llo,
                                                          const uint32_t* __restrict__ lo_rank,
                                                          const uint32_t* __restrict__ hi_base, int64_t n,
                                                          int32_t* __restrict__ idx) {
  __shared__ uint64_t C[DSEA_RDM_PASCAL][DSEA_RDM_PASCAL];
  __shared__ uint8_t pa[DSEA_RDM_MAX_LA], pb[DSEA_SECTOR_MAX_L];
  __shared__ int32_t boff[DSEA_RDM_MAX_BLOCKS], bdB[DSEA_RDM_MAX_BLOCKS];
  rdm_pascal(C, sites.L);
  if (threadIdx.x < DSEA_RDM_MAX_LA) pa[threadIdx.x] = sites.a[threadIdx.x];
  if (threadIdx.x < DSEA_SECTOR_MAX_L) pb[threadIdx.x] = sites.b[threadIdx.x];
  if (threadIdx.x < DSEA_RDM_MAX_BLOCKS) {
    boff[threadIdx.x] = blk.off[threadIdx.x];
    bdB[threadIdx.x] = blk.dB[threadIdx.x];
  }
  __syncthreads();
  const int LA = sites.LA, LB = sites.L - sites.LA, nblk = blk.nblk;
  const uint64_t lomask = (1ull << Llo) - 1;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    int m = 0;
    while (m + 1 < nblk && e >= boff[m + 1]) ++m;
    const int64_t q = e - boff[m];
    const int64_t i = q / bdB[m], j = q - i * bdB[m];
    const int ka = blk.m0 + m;
    const uint64_t s = rdm_unrank_deposit(C, (uint64_t)i, LA, ka, pa) | rdm_unrank_deposit(C, (uint64_t)j, LB, ndown - ka, pb);
    idx[e] = (int32_t)(hi_base[s >> Llo] + lo_rank[s & lomask]);
  }
}

// the full 2^L space: one block, idx[i 2^LB + j] = dep_A(i) | dep_B(j)  (L <= 30)
__global__ __launch_bounds__(256) void k_rdm_index_full(RdmSites sites, int64_t n, int32_t* __restrict__ idx) {
  __shared__ uint8_t pa[DSEA_RDM_MAX_LA], pb[DSEA_SECTOR_MAX_L];
  if (threadIdx.x < DSEA_RDM_MAX_LA) pa[threadIdx.x] = sites.a[threadIdx.x];
  if (threadIdx.x < DSEA_SECTOR_MAX_L) pb[threadIdx.x] = sites.b[threadIdx.x];
  __syncthreads();
  const int LA = sites.LA, LB = sites.L - sites.LA;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const uint32_t i = (uint32_t)(e >> LB), j = (uint32_t)(e & (((int64_t)1 << LB) - 1));
    uint32_t s = 0;
    for (int k = 0; k < LA; ++k) s |= ((i >> k) & 1u) << pa[k];
    for (int k = 0; k < LB; ++k) s |= ((j >> k) & 1u) << pb[k];
    idx[e] = (int32_t)s;
  }
}

// the four index entries of inner indices k0 .. k0 + 3 of the row that starts at idx[rbase]: one 16-byte load where all four
// lie below kend, else entry by entry with a position past the end replaced by kbeg (never read outside the row)
__device__ __forceinline__ rdm_i4 rdm_load_idx(const int32_t* __restrict__ idx, int rbase, int k0, int kbeg, int kend) {
  rdm_i4 o;
  if (k0 + 4 <= kend) {
    o = *reinterpret_cast<const rdm_i4*>(idx + rbase + k0);
  } else {
#pragma unroll
    for (int s = 0; s < 4; ++s) o.v[s] = idx[rbase + (k0 + s < kend ? k0 + s : kbeg)];
  }
  return o;
}
// the four gathers; 0 for an inner index at or past kend
__device__ __forceinline__ rdm_v4d rdm_gather(const double* __restrict__ v, const rdm_i4& ix, int k0, int kend) {
  rdm_v4d o;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const double t = v[ix.v[s]];
    o[s] = k0 + s < kend ? t : 0.0;
  }
  return o;
}

// Forward, first stage: one wave = one (block m, pair of tiles (ti, tj) of 16 T rows, chunk c of the inner dimension).  It
// forms the (16 T)^2 partial of M_m(x)[rows of ti] M_m(y)[rows of tj]^T over its chunk on v_mfma_f64_16x16x4_f64 and writes it
// to scratch[wave (16 T)^2 ..], row-major.  Fragments come straight from x and y through idx: the k index of the MFMA may be
// permuted (the instruction sums over it), so MFMA step s of a 16-wide block takes k = block + 4 (lane >> 4) + s and a lane's
// four k are four consecutive entries of one row of idx.  Pipeline: the gathers of block b + 1 and the index loads of block
// b + 2 are requested before the MFMAs of block b.  A row past dA_m is clamped to dA_m - 1 (its products are never read back);
// an inner index past the chunk contributes 0.  SYM (x and y the same vector): only pairs tj <= ti exist, and a pair on the
// diagonal uses its A fragments as B fragments.
template <int T, bool SYM>
__global__ __launch_bounds__(64) void k_rdm_cross(RdmBlocks blk, RdmCrossPlan plan, const int32_t* __restrict__ idx,
                                                  const double* __restrict__ x, const double* __restrict__ y,
                                                  double* __restrict__ scratch) {
  const int lane = threadIdx.x, fi = lane & 15, kq = lane >> 4;
  const int w = blockIdx.x;
  int m = 0;
  while (m + 1 < blk.nblk && w >= plan.wbase[m + 1]) ++m;
  const int q = w - plan.wbase[m], ns = plan.nsplit[m], pr = q / ns, c = q - pr * ns;
  int ti, tj;
  if (SYM) {                                   // pr = ti (ti + 1) / 2 + tj, tj <= ti
    ti = (int)((sqrt(8.0 * (double)pr + 1.0) - 1.0) * 0.5);
    while ((int64_t)(ti + 1) * (ti + 2) / 2 <= pr) ++ti;
    while ((int64_t)ti * (ti + 1) / 2 > pr) --ti;
    tj = pr - (int)((int64_t)ti * (ti + 1) / 2);
  } else {
    ti = pr / plan.nt[m];
    tj = pr - ti * plan.nt[m];
  }
  const int dA = blk.dA[m], dB = blk.dB[m], off = blk.off[m];
  const int kbeg = c * plan.chunk[m];
  const int kend = kbeg + plan.chunk[m] < dB ? kbeg + plan.chunk[m] : dB;
  const bool diag = SYM && ti == tj;
  int ra[T], rb[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int rowa = 16 * (T * ti + t) + fi, rowb = 16 * (T * tj + t) + fi;
    ra[t] = off + (rowa < dA ? rowa : dA - 1) * dB;
    rb[t] = off + (rowb < dA ? rowb : dA - 1) * dB;
  }
  rdm_v4d acc[T][T];
#pragma unroll
  for (int tm = 0; tm < T; ++tm)
#pragma unroll
    for (int tn = 0; tn < T; ++tn) acc[tm][tn] = (rdm_v4d){0.0, 0.0, 0.0, 0.0};
  const int nsteps = kend > kbeg ? (kend - kbeg + 15) / 16 : 0;
  if (nsteps > 0) {
    rdm_i4 ia[T], ib[T];
    rdm_v4d fa[T], fb[T], ga[T], gb[T];
    int k0 = kbeg + 4 * kq;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      ia[t] = rdm_load_idx(idx, ra[t], k0, kbeg, kend);
      if (!diag) ib[t] = rdm_load_idx(idx, rb[t], k0, kbeg, kend);
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
      fa[t] = rdm_gather(x, ia[t], k0, kend);
      if (!diag) fb[t] = rdm_gather(y, ib[t], k0, kend);
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
      ia[t] = rdm_load_idx(idx, ra[t], k0 + 16, kbeg, kend);
      if (!diag) ib[t] = rdm_load_idx(idx, rb[t], k0 + 16, kbeg, kend);
    }
    for (int st = 0; st < nsteps; ++st, k0 += 16) {
#pragma unroll
      for (int t = 0; t < T; ++t) {            // block st + 1 (all zero past the chunk)
        ga[t] = rdm_gather(x, ia[t], k0 + 16, kend);
        if (!diag) gb[t] = rdm_gather(y, ib[t], k0 + 16, kend);
      }
#pragma unroll
      for (int t = 0; t < T; ++t) {            // block st + 2
        ia[t] = rdm_load_idx(idx, ra[t], k0 + 32, kbeg, kend);
        if (!diag) ib[t] = rdm_load_idx(idx, rb[t], k0 + 32, kbeg, kend);
      }
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
        for (int tm = 0; tm < T; ++tm)
#pragma unroll
          for (int tn = 0; tn < T; ++tn)
            acc[tm][tn] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[tm][s4], diag ? fa[tn][s4] : fb[tn][s4], acc[tm][tn], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < T; ++t) {
        fa[t] = ga[t];
        if (!diag) fb[t] = gb[t];
      }
    }
  }
  // C/D layout of the instruction: row = (lane >> 4) + 4 reg, col = lane & 15
  constexpr int S = 16 * T;
  double* __restrict__ part = scratch + (int64_t)w * (S * S);
#pragma unroll
  for (int tm = 0; tm < T; ++tm)
#pragma unroll
    for (int tn = 0; tn < T; ++tn)
#pragma unroll
      for (int r = 0; r < 4; ++r) part[(16 * tm + 4 * r + kq) * S + 16 * tn + fi] = acc[tm][tn][r];
}

// Forward, second stage: out_m[i, i'] = the sum over the chunks, in order, of the partial that holds it; one output element
// per thread.  SYM: the element (max(i, i'), min(i, i')) of the lower triangle serves both (i, i') and (i', i).
__global__ __launch_bounds__(256) void k_rdm_cross_reduce(RdmBlocks blk, RdmCrossPlan plan, int T, int sym,
                                                          const double* __restrict__ scratch, int64_t out_len,
                                                          double* __restrict__ out) {
  const int S = 16 * T;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < out_len; e += (int64_t)gridDim.x * 256) {
    int m = 0;
    while (m + 1 < blk.nblk && e >= blk.ooff[m + 1]) ++m;
    const int dA = blk.dA[m];
    const int q = (int)(e - blk.ooff[m]);
    int i = q / dA, i2 = q - i * dA;
    if (sym && i2 > i) {
      const int t = i;
      i = i2;
      i2 = t;
    }
    const int ti = i / S, tj = i2 / S;
    const int64_t pr = sym ? (int64_t)ti * (ti + 1) / 2 + tj : (int64_t)ti * plan.nt[m] + tj;
    const int ns = plan.nsplit[m];
    const double* __restrict__ p = scratch + ((int64_t)plan.wbase[m] + pr * ns) * (S * S) + (i - ti * S) * S + (i2 - tj * S);
    double sum = 0.0;
    for (int c = 0; c < ns; ++c) sum += p[(int64_t)c * (S * S)];
    out[e] = sum;
  }
}

// The same sum where the inner dimension was split many ways (few output elements, DSEA_RDM_WIDE_SPLIT chunks or more): one
// wave per output element, lane l adds chunks l, l + 64, ... in order and wave_sum adds the 64 lanes in its fixed order.
__global__ __launch_bounds__(256) void k_rdm_cross_reduce_wide(RdmBlocks blk, RdmCrossPlan plan, int T, int sym,
                                                               const double* __restrict__ scratch, int64_t out_len,
                                                               double* __restrict__ out) {
  const int S = 16 * T, lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= out_len) return;
  int m = 0;
  while (m + 1 < blk.nblk && e >= blk.ooff[m + 1]) ++m;
  const int dA = blk.dA[m];
  const int q = (int)(e - blk.ooff[m]);
  int i = q / dA, i2 = q - i * dA;
  if (sym && i2 > i) {
    const int t = i;
    i = i2;
    i2 = t;
  }
  const int ti = i / S, tj = i2 / S;
  const int64_t pr = sym ? (int64_t)ti * (ti + 1) / 2 + tj : (int64_t)ti * plan.nt[m] + tj;
  const int ns = plan.nsplit[m];
  const double* __restrict__ p = scratch + ((int64_t)plan.wbase[m] + pr * ns) * (S * S) + (i - ti * S) * S + (i2 - tj * S);
  double sum = 0.0;
  for (int c = lane; c < ns; c += 64) sum += p[(int64_t)c * (S * S)];
  sum = wave_sum(sum);
  if (lane == 0) out[e] = sum;
}

// Backward: out[idx[off_m + i dB_m + j]] = sum_i' G_m[i, i'] y[idx[off_m + i' dB_m + j]]  (transpose: G_m[i', i]).  One wave =
// one (block m, 16 TI rows i, 32 columns j); the whole inner dimension dA_m is finished inside it, on the same MFMA with the
// same k permutation: A fragments are four consecutive entries of a row of G_m (of a column when transposed), B fragments
// gathers of y through four rows of idx (16 consecutive entries each).  idx is a permutation, so every output row is written
// exactly once: no atomics, no second stage.  Rows, columns and inner indices past the block are clamped for the loads; inner
// ones contribute 0 and rows and columns are not stored.
template <int TI>
__global__ __launch_bounds__(64) void k_rdm_pull(RdmBlocks blk, RdmPullPlan plan, const int32_t* __restrict__ idx,
                                                 const double* __restrict__ G, const double* __restrict__ y,
                                                 double* __restrict__ out, int transpose) {
  const int lane = threadIdx.x, fi = lane & 15, kq = lane >> 4;
  const int w = blockIdx.x;
  int m = 0;
  while (m + 1 < blk.nblk && w >= plan.wbase[m + 1]) ++m;
  const int q = w - plan.wbase[m], ti = q / plan.ntj[m], tj = q - ti * plan.ntj[m];
  const int dA = blk.dA[m], dB = blk.dB[m], off = blk.off[m];
  const double* __restrict__ Gm = G + blk.ooff[m];
  int ri[TI], cj[2];
#pragma unroll
  for (int t = 0; t < TI; ++t) {
    const int row = 16 * (TI * ti + t) + fi;
    ri[t] = row < dA ? row : dA - 1;
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int col = 32 * tj + 16 * u + fi;
    cj[u] = off + (col < dB ? col : dB - 1);
  }
  rdm_v4d acc[TI][2];
#pragma unroll
  for (int tm = 0; tm < TI; ++tm)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) acc[tm][tn] = (rdm_v4d){0.0, 0.0, 0.0, 0.0};
  for (int kb = 0; kb < dA; kb += 16) {
    const int k0 = kb + 4 * kq;
    rdm_v4d fa[TI], fb[2];
    int ix[2][4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int kc = k0 + s < dA ? k0 + s : 0;
#pragma unroll
      for (int u = 0; u < 2; ++u) ix[u][s] = idx[cj[u] + kc * dB];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bool ok = k0 + s < dA;
      const int kc = ok ? k0 + s : 0;
#pragma unroll
      for (int t = 0; t < TI; ++t) {
        const double g = transpose ? Gm[(int64_t)kc * dA + ri[t]] : Gm[(int64_t)ri[t] * dA + kc];
        fa[t][s] = ok ? g : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const double v = y[ix[u][s]];
        fb[u][s] = ok ? v : 0.0;
      }
    }
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
      for (int tm = 0; tm < TI; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
          acc[tm][tn] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[tm][s4], fb[tn][s4], acc[tm][tn], 0, 0, 0);
  }
#pragma unroll
  for (int tm = 0; tm < TI; ++tm)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * (TI * ti + tm) + 4 * r + kq, col = 32 * tj + 16 * tn + fi;
        if (row < dA && col < dB) out[idx[off + row * dB + col]] = acc[tm][tn][r];
      }
}

// C(a, b) for 0 <= a <= 40 (exact in 64 bits); 0 outside 0 <= b <= a
uint64_t rdm_binom(int a, int b) {
  if (b < 0 || b > a) return 0;
  if (b > a - b) b = a - b;
  uint64_t c = 1;
  for (int i = 1; i <= b; ++i) c = c * (uint64_t)(a - b + i) / (uint64_t)i;
  return c;
}

// the tile edge 16 T of the forward: `tile` 1 or 2 forces T, 0 takes 2 as soon as a block has more than 16 rows
int rdm_tile(const RdmGeom& g, int tile) {
  if (tile == 1 || tile == 2) return tile;
  for (int m = 0; m < g.blk.nblk; ++m)
    if (g.blk.dA[m] > 16) return 2;
  return 1;
}

// the work list of the forward; false when it would not fit 31 bits
bool rdm_cross_plan(const RdmGeom& g, int T, bool sym, RdmCrossPlan* p) {
  const int S = 16 * T;
  int64_t pairs[DSEA_RDM_MAX_BLOCKS], total = 0;
  for (int m = 0; m < g.blk.nblk; ++m) {
    const int64_t nt = (g.blk.dA[m] + S - 1) / S;
    p->nt[m] = (int32_t)nt;
    pairs[m] = sym ? nt * (nt + 1) / 2 : nt * nt;
    total += pairs[m];
  }
  const int64_t want = (DSEA_RDM_TARGET_WAVES + total - 1) / total;   // chunks per pair that would fill the machine
  int64_t w = 0;
  for (int m = 0; m < DSEA_RDM_MAX_BLOCKS; ++m) {
    if (m >= g.blk.nblk) {
      p->wbase[m + 1] = (int32_t)w;
      p->nsplit[m] = p->chunk[m] = p->nt[m] = 1;
      continue;
    }
    const int64_t dB = g.blk.dB[m];
    int64_t most = (dB + DSEA_RDM_MIN_CHUNK - 1) / DSEA_RDM_MIN_CHUNK;
    if (most > want) most = want;
    const int64_t chunk = ((dB + most - 1) / most + 15) / 16 * 16;
    const int64_t ns = (dB + chunk - 1) / chunk;                       // every chunk holds at least one inner index
    p->wbase[m] = (int32_t)w;
    p->nsplit[m] = (int32_t)ns;
    p->chunk[m] = (int32_t)chunk;
    w += pairs[m] * ns;
    if (w > 0x7FFFFFFFll) return false;
    p->wbase[m + 1] = (int32_t)w;
  }
  return true;
}

void rdm_pull_plan(const RdmGeom& g, int TI, RdmPullPlan* p, int64_t* waves) {
  int64_t w = 0;
  for (int m = 0; m < DSEA_RDM_MAX_BLOCKS; ++m) {
    p->wbase[m] = (int32_t)w;
    p->ntj[m] = 1;
    if (m < g.blk.nblk) {
      const int64_t nti = (g.blk.dA[m] + 16 * TI - 1) / (16 * TI), ntj = ((int64_t)g.blk.dB[m] + 31) / 32;
      p->ntj[m] = (int32_t)ntj;
      w += nti * ntj;
    }
    p->wbase[m + 1] = (int32_t)w;
  }
  *waves = w;                                    // at most n / 32 + 17 (dA / 16 + 1): far below 2^31
}
}  // namespace

// the block structure of (L, ndown, sites); ndown < 0: the full 2^L space.  Host arithmetic only; false for LA outside
// 1 .. min(L - 1, 16), a site out of range or repeated, a sector outside the limits of sector_sizes, the full space with
// L > 30, and a flat output of 2^31 elements or more.
bool rdm_geometry(int L, int ndown, int LA, const int32_t* sites, RdmGeom* g) {
  if (!sites || L < 2 || L > DSEA_SECTOR_MAX_L || LA < 1 || LA > DSEA_RDM_MAX_LA || LA > L - 1) return false;
  uint64_t seen = 0;
  for (int k = 0; k < LA; ++k) {
    if (sites[k] < 0 || sites[k] >= L || ((seen >> sites[k]) & 1ull)) return false;
    seen |= 1ull << sites[k];
  }
  const int LB = L - LA;
  g->L = L;
  g->ndown = ndown;
  g->sites.L = L;
  g->sites.LA = LA;
  for (int k = 0; k < DSEA_RDM_MAX_LA; ++k) g->sites.a[k] = k < LA ? (uint8_t)sites[k] : (uint8_t)0;
  int nbs = 0;
  for (int i = 0; i < DSEA_SECTOR_MAX_L; ++i) g->sites.b[i] = 0;
  for (int i = 0; i < L; ++i)
    if (!((seen >> i) & 1ull)) g->sites.b[nbs++] = (uint8_t)i;
  RdmBlocks& b = g->blk;
  for (int m = 0; m <= DSEA_RDM_MAX_BLOCKS; ++m) b.ooff[m] = 0;
  for (int m = 0; m < DSEA_RDM_MAX_BLOCKS; ++m) {
    b.off[m] = 0;
    b.dA[m] = b.dB[m] = 1;
  }
  int64_t off = 0, ooff = 0;
  if (ndown < 0) {
    if (L > 30) return false;
    b.nblk = 1;
    b.m0 = 0;
    b.dA[0] = 1 << LA;
    b.dB[0] = 1 << LB;
    off = (int64_t)1 << L;
    ooff = (int64_t)b.dA[0] * b.dA[0];
    if (ooff > 0x7FFFFFFFll) return false;
  } else {
    int64_t n, n_lo, n_hi;
    if (!sector_sizes(L, ndown, &n, &n_lo, &n_hi)) return false;
    const int mlo = ndown - LB > 0 ? ndown - LB : 0, mhi = LA < ndown ? LA : ndown;
    b.nblk = mhi - mlo + 1;
    b.m0 = mlo;
    for (int m = mlo; m <= mhi; ++m) {
      const uint64_t dA = rdm_binom(LA, m), dB = rdm_binom(LB, ndown - m);   // dA dB <= n < 2^31
      b.off[m - mlo] = (int32_t)off;
      b.ooff[m - mlo] = (int32_t)ooff;
      b.dA[m - mlo] = (int32_t)dA;
      b.dB[m - mlo] = (int32_t)dB;
      off += (int64_t)(dA * dB);
      ooff += (int64_t)(dA * dA);
      if (ooff > 0x7FFFFFFFll) return false;
    }
    if (off != n) return false;                  // (Vandermonde: cannot happen)
  }
  for (int m = b.nblk; m <= DSEA_RDM_MAX_BLOCKS; ++m) b.ooff[m] = (int32_t)ooff;
  for (int m = b.nblk; m < DSEA_RDM_MAX_BLOCKS; ++m) b.off[m] = (int32_t)(off > 0x7FFFFFFFll ? 0x7FFFFFFFll : off);
  g->n = off;
  g->out_len = ooff;
  return true;
}

// doubles of scratch that launch_rdm_cross may write for this geometry: the largest work list over both tile edges and both
// the symmetric and the general form; -1 when a work list does not fit
int64_t rdm_scratch_doubles(const RdmGeom& g) {
  int64_t most = 0;
  for (int T = 1; T <= 2; ++T)
    for (int sym = 0; sym < 2; ++sym) {
      RdmCrossPlan p;
      if (!rdm_cross_plan(g, T, sym != 0, &p)) return -1;
      const int64_t need = (int64_t)p.wbase[g.blk.nblk] * (256 * T * T);
      if (need > most) most = need;
    }
  return most;
}

int launch_rdm_index(const RdmGeom& g, const uint32_t* lo_rank, const uint32_t* hi_base, int32_t* idx, hipStream_t st) {
  const unsigned grid = (unsigned)ew_blocks(g.n * 8);
  if (g.ndown < 0) {
    hipLaunchKernelGGL(k_rdm_index_full, dim3(grid), dim3(256), 0, st, g.sites, g.n, idx);
  } else {
    if (!lo_rank || !hi_base) return -1;
    hipLaunchKernelGGL(k_rdm_index_sector, dim3(grid), dim3(256), 0, st, g.sites, g.blk, g.ndown, (g.L + 1) / 2, lo_rank, hi_base,
                       g.n, idx);
  }
  return 0;
}

// out (flat, block after block, row-major) = cross(x, y); x == y (the same pointer) takes the symmetric form
int launch_rdm_cross(const RdmGeom& g, const int32_t* idx, const double* x, const double* y, double* out, double* scratch,
                     int tile, hipStream_t st) {
  const int T = rdm_tile(g, tile);
  const bool sym = x == y;
  RdmCrossPlan p;
  if (!rdm_cross_plan(g, T, sym, &p)) return -1;
  const dim3 grid((unsigned)p.wbase[g.blk.nblk]);
  if (T == 1) {
    if (sym) hipLaunchKernelGGL((k_rdm_cross<1, true>), grid, dim3(64), 0, st, g.blk, p, idx, x, y, scratch);
    else hipLaunchKernelGGL((k_rdm_cross<1, false>), grid, dim3(64), 0, st, g.blk, p, idx, x, y, scratch);
  } else {
    if (sym) hipLaunchKernelGGL((k_rdm_cross<2, true>), grid, dim3(64), 0, st, g.blk, p, idx, x, y, scratch);
    else hipLaunchKernelGGL((k_rdm_cross<2, false>), grid, dim3(64), 0, st, g.blk, p, idx, x, y, scratch);
  }
  int most = 1;
  for (int m = 0; m < g.blk.nblk; ++m)
    if (p.nsplit[m] > most) most = p.nsplit[m];
  if (most >= DSEA_RDM_WIDE_SPLIT)               // (then the pairs are few: out_len <= 1024 DSEA_RDM_TARGET_WAVES / DSEA_RDM_WIDE_SPLIT)
    hipLaunchKernelGGL(k_rdm_cross_reduce_wide, dim3((unsigned)((g.out_len + 3) / 4)), dim3(256), 0, st, g.blk, p, T, sym ? 1 : 0,
                       scratch, g.out_len, out);
  else
    hipLaunchKernelGGL(k_rdm_cross_reduce, dim3((unsigned)ew_blocks(g.out_len * 8)), dim3(256), 0, st, g.blk, p, T, sym ? 1 : 0,
                       scratch, g.out_len, out);
  return 0;
}

// out (n) = the slices G_m M_m(y) (transpose: G_m^T M_m(y)) scattered through idx
int launch_rdm_pull(const RdmGeom& g, const int32_t* idx, const double* G, const double* y, double* out, int transpose,
                    hipStream_t st) {
  const int TI = rdm_tile(g, 0);
  RdmPullPlan p;
  int64_t waves;
  rdm_pull_plan(g, TI, &p, &waves);
  if (waves > 0x7FFFFFFFll) return -1;
  if (TI == 1) hipLaunchKernelGGL((k_rdm_pull<1>), dim3((unsigned)waves), dim3(64), 0, st, g.blk, p, idx, G, y, out, transpose);
  else hipLaunchKernelGGL((k_rdm_pull<2>), dim3((unsigned)waves), dim3(64), 0, st, g.blk, p, idx, G, y, out, transpose);
  return 0;
}

}  // namespace dsea
