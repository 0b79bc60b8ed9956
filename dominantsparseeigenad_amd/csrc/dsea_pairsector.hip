// dsea_pairsector.hip -- matrix-free XXZ spins with a coupling on EVERY pair of sites, restricted to one magnetisation sector
// (docs/design/22-pair-sector.md): the mat-vec k_spmv_pairsector, the parameter adjoint in two kernels -- k_pairsector_forms
// (the xy forms, gathers) and k_pairsector_gram (the zz and z forms, a Gram product on the fp64 matrix cores) -- their
// fixed-order second stage k_pairsector_reduce, and the launchers.
//
//   H = sum_{i<j} [ Jxy_ij (X_i X_j + Y_i Y_j) + Jz_ij Z_i Z_j ] + sum_i hz_i Z_i
// on the states s with exactly ndown set bits; rows, bits, states and Lin's two rank tables are those of dsea_sector.hip
// (dsea_sector_build_tables).  With m_ij = (1 << i) | (1 << j):
//   (H x)[r] = ( sum_{i<j} Jz_ij z_i z_j + sum_i hz_i z_i ) x[r] + sum_{i<j : bit_i != bit_j} 2 Jxy_ij x[rank(s_r ^ m_ij)]
// The couplings are one device array [Jxy(P), Jz(P), hz(L)], P = L (L - 1) / 2, pairs in lexicographic order (0,1), (0,2), ...,
// (0,L-1), (1,2), ...: p(i, j) = i (2 L - i - 1) / 2 + (j - i - 1).  The pairs are implicit: no table travels in the kernel
// arguments, every block works the list out into LDS.  Nothing here is shared with dsea_sector.hip: the file has its own helpers.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_internal.h"
#include "dsea_device.h"

namespace dsea {

#define DSEA_PAIR_MAX_PAIRS (DSEA_SECTOR_MAX_L * (DSEA_SECTOR_MAX_L - 1) / 2)      /* 780 */
#define DSEA_PAIR_MAX_PARAMS (2 * DSEA_PAIR_MAX_PAIRS + DSEA_SECTOR_MAX_L)         /* 1600 doubles, 12.8 KB */
#define DSEA_PAIR_CHUNK 8            /* pairs whose table lookups and gathers a thread keeps in flight together */
#define DSEA_PAIR_NO_RANK 0xFFFFFFFFu /* "this pair does not flip this row" (a rank is below 2^31) */
#define DSEA_PAIR_GRAM_BLOCKS 256    /* grid cap of the Gram kernel: it is bound by the matrix pipe, one block per CU feeds it */

struct PairParams {
  int L, Llo, npair;
  int64_t n;
  const double* c;
  const uint64_t* states;
  const uint32_t* lo_rank;
  const uint32_t* hi_base;
};

typedef double pair_v4d __attribute__((ext_vector_type(4)));

// v * (1 - 2 bit), exact: the bit goes into the sign
__device__ __forceinline__ double pair_signed(double v, uint64_t bit) {
  return __longlong_as_double(__double_as_longlong(v) ^ (long long)(bit << 63));
}
__device__ __forceinline__ int pair_index(int i, int j, int L) { return i * (2 * L - i - 1) / 2 + (j - i - 1); }

// The pair list in LDS, GROUPED BY HOW A PAIR MEETS THE SPLIT OF THE RANK TABLES: first the pairs with both sites below Llo,
// then the pairs across the split, then the pairs with both sites at or above Llo (inside a group in lexicographic order).
// Entry = i | j << 8 | p << 16, i < j, p the pair's index in the couplings.  Filled by the block: a thread walks at most L rows
// of the triangle.  With Lhi = L - Llo the groups have Llo (Llo - 1) / 2, Llo Lhi and Lhi (Lhi - 1) / 2 entries.
struct PairGroups {
  int low, across;   // the ends of the first and of the second group (the third ends at npair)
};
__device__ __forceinline__ PairGroups pair_groups(int L, int Llo) {
  PairGroups g;
  g.low = Llo * (Llo - 1) / 2;
  g.across = g.low + Llo * (L - Llo);
  return g;
}
__device__ __forceinline__ void pair_fill_table(uint32_t* tb, int L, int Llo, int npair) {
  const PairGroups g = pair_groups(L, Llo);
  const int Lhi = L - Llo;
  for (int p = threadIdx.x; p < npair; p += blockDim.x) {
    int i = 0, rest = p;
    while (rest >= L - 1 - i) {
      rest -= L - 1 - i;
      ++i;
    }
    const int j = i + 1 + rest;
    int at;
    if (j < Llo)
      at = pair_index(i, j, Llo);
    else if (i < Llo)
      at = g.low + i * Lhi + (j - Llo);
    else
      at = g.across + pair_index(i - Llo, j - Llo, Lhi);
    tb[at] = (uint32_t)i | ((uint32_t)j << 8) | ((uint32_t)p << 16);
  }
}
// an entry of the table as a wave-uniform value: the shifts and the mask built from it are scalar work
__device__ __forceinline__ uint32_t pair_entry(const uint32_t* tb, int k) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)tb[k]); }
__device__ __forceinline__ uint64_t pair_mask(uint32_t e) { return (1ull << (e & 255u)) | (1ull << ((e >> 8) & 255u)); }
// 1 when exactly one of the pair's two bits is set in s
__device__ __forceinline__ uint64_t pair_differ(uint64_t s, uint64_t mask) {
  const uint64_t t = s & mask;
  return (t != 0 && t != mask) ? 1ull : 0ull;
}

// the ranks of the partner rows of the table entries k0 .. k0 + CHUNK - 1 of one group for the row with state s, all table reads
// requested before any is used; DSEA_PAIR_NO_RANK for a pair that does not flip the row (and at or past kend).  hi_own =
// hi_base[s >> Llo] and lo_own = lo_rank[s & lomask] are the row's own two reads (loaded once per row): a pair with both sites
// below Llo keeps the high word (KIND 0: one read of lo_rank), one with both sites at or above Llo keeps the low word (KIND 2:
// one read of hi_base); only a pair across the split (KIND 1) costs two reads.
template <int KIND>
__device__ __forceinline__ void pair_ranks(uint32_t (&rk)[DSEA_PAIR_CHUNK], uint64_t s, bool have, int k0, int kend, int Llo,
                                           uint32_t hi_own, uint32_t lo_own, const uint32_t* tb,
                                           const uint32_t* __restrict__ lo_rank, const uint32_t* __restrict__ hi_base) {
  const uint64_t lomask = (1ull << Llo) - 1;
#pragma unroll
  for (int e = 0; e < DSEA_PAIR_CHUNK; ++e) {
    const bool in = k0 + e < kend;
    const uint64_t mask = in ? pair_mask(pair_entry(tb, k0 + e)) : 0ull;
    const bool on = have && in && pair_differ(s, mask) != 0;
    const uint64_t s2 = s ^ mask;
    rk[e] = DSEA_PAIR_NO_RANK;
    if (on) {
      const uint32_t h = KIND == 0 ? hi_own : hi_base[s2 >> Llo];
      const uint32_t l = KIND == 2 ? lo_own : lo_rank[s2 & lomask];
      rk[e] = h + l;
    }
  }
}
// the gathers of one chunk: v[rank], 0 where the pair does not flip the row
__device__ __forceinline__ void pair_gather(double (&xv)[DSEA_PAIR_CHUNK], const uint32_t (&rk)[DSEA_PAIR_CHUNK],
                                            const double* __restrict__ v) {
#pragma unroll
  for (int e = 0; e < DSEA_PAIR_CHUNK; ++e) {
    xv[e] = 0.0;
    if (rk[e] != DSEA_PAIR_NO_RANK) xv[e] = v[rk[e]];
  }
}
// One group of the table for one row: a uniform loop over its entries in chunks, the table reads of chunk c + 1 issued before
// the gathers of chunk c are consumed; use(entry, mask, v[partner] or 0) once per entry, for every lane.
template <int KIND, class F>
__device__ __forceinline__ void pair_group(int kbeg, int kend, uint64_t s, bool have, int Llo, uint32_t hi_own, uint32_t lo_own,
                                           const uint32_t* tb, const uint32_t* __restrict__ lo_rank,
                                           const uint32_t* __restrict__ hi_base, const double* __restrict__ v, F&& use) {
  uint32_t rkA[DSEA_PAIR_CHUNK], rkB[DSEA_PAIR_CHUNK];
  pair_ranks<KIND>(rkA, s, have, kbeg, kend, Llo, hi_own, lo_own, tb, lo_rank, hi_base);
  for (int k0 = kbeg; k0 < kend; k0 += DSEA_PAIR_CHUNK) {
    double xv[DSEA_PAIR_CHUNK];
    pair_gather(xv, rkA, v);
    pair_ranks<KIND>(rkB, s, have, k0 + DSEA_PAIR_CHUNK, kend, Llo, hi_own, lo_own, tb, lo_rank, hi_base);
#pragma unroll
    for (int e = 0; e < DSEA_PAIR_CHUNK; ++e) {
      if (k0 + e < kend) {                         // (the same for every lane)
        const uint32_t w = pair_entry(tb, k0 + e);
        use(w, pair_mask(w), xv[e]);
      }
      rkA[e] = rkB[e];
    }
  }
}
// the three groups in turn
template <class F>
__device__ __forceinline__ void pair_walk(const PairParams& p, uint64_t s, bool have, const uint32_t* tb,
                                          const double* __restrict__ v, F&& use) {
  const int Llo = p.Llo;
  const PairGroups g = pair_groups(p.L, Llo);
  const uint32_t hi_own = p.hi_base[s >> Llo], lo_own = p.lo_rank[s & ((1ull << Llo) - 1)];
  pair_group<0>(0, g.low, s, have, Llo, hi_own, lo_own, tb, p.lo_rank, p.hi_base, v, use);
  pair_group<1>(g.low, g.across, s, have, Llo, hi_own, lo_own, tb, p.lo_rank, p.hi_base, v, use);
  pair_group<2>(g.across, p.npair, s, have, Llo, hi_own, lo_own, tb, p.lo_rank, p.hi_base, v, use);
}

// y = H x - shift x ; partial x.y per block.  One row per thread: states, x and y are read and written coalesced; a pair whose
// two bits differ in the row costs one or two table reads and one gather of x (pair_walk).  A block walks the row ranges
// blockIdx.x, + gridDim.x, ... of 256 rows.  A row's sums run over the pairs in the order of the table.
__global__ __launch_bounds__(256) void k_spmv_pairsector(PairParams p, const double* __restrict__ x, double* __restrict__ y,
                                                         const double* __restrict__ shift, const double* __restrict__ skip,
                                                         double* __restrict__ P) {
  __shared__ double cp[DSEA_PAIR_MAX_PARAMS];
  __shared__ uint32_t tb[DSEA_PAIR_MAX_PAIRS];
  __shared__ double sm5[5];
  if (skip && skip[0] != 0.0) return;
  const int L = p.L, np = p.npair;
  const int64_t n = p.n;
  for (int c = threadIdx.x; c < 2 * np + L; c += 256) cp[c] = p.c[c];
  pair_fill_table(tb, L, p.Llo, np);
  __syncthreads();
  const double* __restrict__ jxy = cp;
  const double* __restrict__ jzs = cp + np;
  const double* __restrict__ hzs = cp + 2 * np;
  const double s = shift ? shift[0] : 0.0;
  double acc = 0.0;
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;                       // (a thread past the last row reads row n - 1 and writes nothing)
    const uint64_t st = p.states[have ? r : n - 1];
    const double xr = x[have ? r : n - 1];
    double diag = 0.0, sum = 0.0;
    for (int i = 0; i < L; ++i) diag += pair_signed(hzs[i], (st >> i) & 1ull);
    pair_walk(p, st, have, tb, x, [&](uint32_t w, uint64_t mask, double xv) {
      const int t = (int)(w >> 16);
      diag += pair_signed(jzs[t], pair_differ(st, mask));
      sum = fma(2.0 * jxy[t], xv, sum);
    });
    if (have) {
      double v = fma(diag, xr, sum);
      if (shift) v = __dsub_rn(v, __dmul_rn(s, xr));
      y[r] = v;
      acc = fma(xr, v, acc);
    }
  }
  if (P) {
    __syncthreads();
    const double tot = block_sum(acc, sm5);
    if (threadIdx.x == 0) P[blockIdx.x] = tot;
  }
}

// The xy forms: out[p] = sum_{r : bits differ} 2 v1[r] v2[rank(s_r ^ m_p)] for all P pairs in one pass over v1 and v2.  Same
// row walk and the same chunks of lookups and gathers (of v2) as the mat-vec.  Every term is reduced through the wave at once
// (wave_sum, fixed order) and lane 0 adds it to the wave's row of LDS accumulators; the four rows are added in fixed order and
// written to scratch[p * gridDim.x + block].  No atomics.
__global__ __launch_bounds__(256) void k_pairsector_forms(PairParams p, const double* __restrict__ v1,
                                                          const double* __restrict__ v2, double* __restrict__ scratch) {
  __shared__ double accs[4][DSEA_PAIR_MAX_PAIRS];
  __shared__ uint32_t tb[DSEA_PAIR_MAX_PAIRS];
  const int np = p.npair;
  const int64_t n = p.n;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double* __restrict__ mine = accs[wv];
  for (int c = lane; c < np; c += 64) mine[c] = 0.0;   // (afterwards a wave's row is touched by its lane 0 alone)
  pair_fill_table(tb, p.L, p.Llo, np);
  __syncthreads();
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;                       // a thread without a row adds zeros to every form
    const uint64_t st = p.states[have ? r : n - 1];
    const double a = have ? v1[r] : 0.0;
    pair_walk(p, st, have, tb, v2, [&](uint32_t w, uint64_t, double xv) {
      const double tot = wave_sum(2.0 * (a * xv));      // (every lane takes part: the loop is uniform)
      if (lane == 0) mine[w >> 16] += tot;
    });
  }
  __syncthreads();
  for (int c = threadIdx.x; c < np; c += 256)
    scratch[(int64_t)c * gridDim.x + blockIdx.x] = ((accs[0][c] + accs[1][c]) + accs[2][c]) + accs[3][c];
}

// The zz and z forms as ONE Gram product on v_mfma_f64_16x16x4_f64.  With w_r = v1[r] v2[r] and an extra "site" L whose z is 1,
//   G[i][j] = sum_r (w_r z_i(s_r)) z_j(s_r),  0 <= i, j <= L
// holds every zz form (i > j), every z form (row L) and v1.v2 (the corner).  The operands are made in registers from states[r]:
// z_i(s) = 1 - 2 bit_i(s) is a sign flip, so w z is exact, and a site past L reads a clear bit (s < 2^L), which gives the
// column of ones at i = L for nothing (the columns beyond it are computed and never written).  T = ceil((L + 1) / 16) tile
// rows, only the T (T + 1) / 2 tiles on or below the diagonal.  The k index of the instruction is the row and may be permuted
// (the product sums over it): a wave loads 64 rows coalesced, puts (state, w) into its 1 KB of LDS, and step s = 0 .. 15 takes
// the rows 16 (lane >> 4) + s -- one 16-byte LDS read per lane and step, four addresses per wave.  A lane's A operand of tile
// row t is w z_{16 t + (lane & 15)}, its B operand z_{16 t + (lane & 15)}.  The accumulators live over the wave's whole row
// walk; at the end a wave writes the entries below the diagonal to scratch[slot * (4 gridDim.x) + wave], slot = the pair index
// of (j, i) for i < L and P + j for i = L (C/D layout: row = (lane >> 4) + 4 reg, col = lane & 15).  No gathers, no atomics.
template <int T>
__global__ __launch_bounds__(256) void k_pairsector_gram(PairParams p, const double* __restrict__ v1,
                                                         const double* __restrict__ v2, double* __restrict__ scratch) {
  struct __attribute__((aligned(16))) Row {
    uint64_t s;
    double w;
  };
  __shared__ Row stage[4][64];
  constexpr int NT = T * (T + 1) / 2;
  const int L = p.L, np = p.npair;
  const int64_t n = p.n;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, fi = lane & 15, kq = lane >> 4;
  pair_v4d acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = pair_v4d{0.0, 0.0, 0.0, 0.0};
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;                       // a thread without a row contributes w = 0
    Row mine;
    mine.s = p.states[have ? r : n - 1];
    mine.w = have ? v1[r] * v2[r] : 0.0;
    __syncthreads();                               // (the reads of the previous range are done)
    stage[wv][lane] = mine;
    __syncthreads();
#pragma unroll 4
    for (int s = 0; s < 16; ++s) {
      const Row k = stage[wv][16 * kq + s];
      double fa[T], fb[T];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const uint64_t bit = (k.s >> (16 * t + fi)) & 1ull;
        fa[t] = pair_signed(k.w, bit);
        fb[t] = pair_signed(1.0, bit);
      }
      int idx = 0;
#pragma unroll
      for (int tm = 0; tm < T; ++tm)
#pragma unroll
        for (int tn = 0; tn <= tm; ++tn, ++idx) acc[idx] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[tm], fb[tn], acc[idx], 0, 0, 0);
    }
  }
  const int nw = 4 * gridDim.x, gw = 4 * blockIdx.x + wv;
  int idx = 0;
#pragma unroll
  for (int tm = 0; tm < T; ++tm)
#pragma unroll
    for (int tn = 0; tn <= tm; ++tn, ++idx)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = 16 * tm + 4 * reg + kq, col = 16 * tn + fi;
        if (row <= L && col < row) {
          const int slot = row == L ? np + col : pair_index(col, row, L);
          scratch[(int64_t)slot * nw + gw] = acc[idx][reg];
        }
      }
}

// second stage of both: out[t] = the sum of slot t's partials, fixed order; one block per slot
__global__ __launch_bounds__(256) void k_pairsector_reduce(const double* __restrict__ scratch, int count,
                                                           double* __restrict__ out) {
  __shared__ double sm5[5];
  const double tot = sum_partials_block(scratch + (int64_t)blockIdx.x * count, count, sm5);
  if (threadIdx.x == 0) out[blockIdx.x] = tot;
}

// one block per 256 rows up to the cap 2^tune_tile_log2 (6 .. 12, 12 at creation: 4096); beyond it blocks walk row ranges
static inline int pairsector_blocks(const OpDesc& op) {
  int64_t nblk = (op.n + 255) / 256;
  const int64_t cap = (int64_t)1 << op.tune_tile_log2;
  if (nblk > cap) nblk = cap;
  return (int)nblk;
}

// the kernel arguments; false when the descriptor is out of range
static bool pairsector_params(const OpDesc& op, PairParams* p) {
  const PairSectorDesc& d = op.pairsector;
  int64_t n, n_lo, n_hi;
  if (!sector_sizes(d.L, d.ndown, &n, &n_lo, &n_hi) || n != op.n) return false;
  if (op.tune_tile_log2 < 6 || op.tune_tile_log2 > 12 || !d.c || !d.states || !d.lo_rank || !d.hi_base) return false;
  p->L = d.L;
  p->Llo = (d.L + 1) / 2;
  p->npair = d.L * (d.L - 1) / 2;
  p->n = n;
  p->c = d.c;
  p->states = d.states;
  p->lo_rank = d.lo_rank;
  p->hi_base = d.hi_base;
  return true;
}

// doubles that dsea_op_pairsector_forms may write at any grid cap: P slots of per-block partials of the xy kernel (the largest
// cap gives the most blocks), then P + L slots of per-wave partials of the Gram kernel
int64_t pairsector_forms_scratch_doubles(int64_t n, int L) {
  const int64_t rows = (n + 255) / 256, np = (int64_t)L * (L - 1) / 2;
  const int64_t nblk = rows > DSEA_MAX_TFIM_BLOCKS ? DSEA_MAX_TFIM_BLOCKS : rows;
  const int64_t gblk = rows > DSEA_PAIR_GRAM_BLOCKS ? DSEA_PAIR_GRAM_BLOCKS : rows;
  return np * nblk + (np + L) * 4 * gblk;
}

int launch_spmv_pairsector(const OpDesc& op, const double* x, double* y, const double* shift, const double* skip, double* P,
                           hipStream_t st, EventPair* ev) {
  PairParams p;
  if (!pairsector_params(op, &p)) return -1;
  const int nblk = pairsector_blocks(op);
  klaunch(ev, k_spmv_pairsector, nblk, 256, 0, st, p, x, y, shift, skip, P);
  return nblk;
}

int launch_pairsector_forms(const OpDesc& op, const double* v1, const double* v2, double* out, double* scratch, hipStream_t st) {
  PairParams p;
  if (!pairsector_params(op, &p)) return -1;
  const int nblk = pairsector_blocks(op);
  const int gblk = nblk > DSEA_PAIR_GRAM_BLOCKS ? DSEA_PAIR_GRAM_BLOCKS : nblk;
  double* gram = scratch + (int64_t)p.npair * nblk;
  klaunch(nullptr, k_pairsector_forms, nblk, 256, 0, st, p, v1, v2, scratch);
  hipLaunchKernelGGL(k_pairsector_reduce, dim3(p.npair), dim3(256), 0, st, scratch, nblk, out);
  const int T = (p.L + 1 + 15) / 16;
  if (T == 1)
    klaunch(nullptr, k_pairsector_gram<1>, gblk, 256, 0, st, p, v1, v2, gram);
  else if (T == 2)
    klaunch(nullptr, k_pairsector_gram<2>, gblk, 256, 0, st, p, v1, v2, gram);
  else
    klaunch(nullptr, k_pairsector_gram<3>, gblk, 256, 0, st, p, v1, v2, gram);
  hipLaunchKernelGGL(k_pairsector_reduce, dim3(p.npair + p.L), dim3(256), 0, st, gram, 4 * gblk, out + p.npair);
  return 0;
}

}  // namespace dsea
