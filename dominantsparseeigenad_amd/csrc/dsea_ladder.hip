// dsea_ladder.hip -- linear maps between two magnetisation sectors of the same L sites (docs/design/24-dynamics.md): the ladder
// k_sector_ladder<STEP>, its site forms k_sector_ladder_forms<STEP> (+ k_sector_ladder_forms_reduce), the block forms
// k_sector_ladder_block<STEP, R> and k_sector_ladder_block_dots<STEP, R> (docs/design/35-finite-temperature-dynamics.md), and
// their launchers.
//
// Site i is bit i of a state, a set bit is a down spin, z_i(s) = 1 - 2 bit_i(s).  For site weights c (fp64 [L], read through
// their device pointer on every launch) the map takes the source sector (L, ndown_src) to the destination sector
// (L, ndown_src + STEP).  With r' a row of the destination and s' = states_dst[r']:
//   STEP = +1, sigma^-(c):  y[r'] = sum_{i : bit_i(s') = 1} c_i x[rank_src(s' ^ (1 << i))]
//   STEP = -1, sigma^+(c):  y[r'] = sum_{i : bit_i(s') = 0} c_i x[rank_src(s' | (1 << i))]
//   STEP =  0, Z(c):        y[r'] = (sum_i c_i z_i(s')) x[r']
// All three are gathers over the destination rows: no scatter, no atomic.  sigma^+(c) is the transpose of sigma^-(c).
// rank_src(s) = hi_base_src[s >> Llo] + lo_rank_src[s & (2^Llo - 1)], Llo = (L + 1) / 2: the two tables of the SOURCE sector
// (dsea_sector_build_tables).  Flipping one bit changes one of the two words only, so a row loads its own
// hi_base_src[s' >> Llo] and lo_rank_src[s' & lomask] once; a site below Llo then costs one lo_rank read and one gather, a site
// at or above Llo one hi_base read and one gather.  The row's own hi_base_src entry enters a sum only when a low site
// contributes, and then it belongs to a valid source state; the row's own lo_rank_src entry is the rank of the low word among
// the words of its popcount and is always valid.
// The site walk is written once, on a row of R columns (docs/design/38-ladder-parts.md): the single-vector kernels are its
// R = 1 case.  The row access, the sign and the partials of a block come from dsea_block.h, the grid rules from
// dsea_internal.h; nothing is shared with dsea_sector.hip.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_internal.h"
#include "dsea_device.h"
#include "dsea_block.h"

namespace dsea {

namespace {
#define DSEA_LADDER_NO_RANK 0xFFFFFFFFu /* "this site does not contribute to this row" (a rank is below 2^31) */

struct LadderParams {
  int L, Llo;
  int64_t n;                  // rows of the destination
  const double* c;            // the L site weights
  const uint64_t* states;     // of the destination
  const uint32_t* lo_rank;    // of the source
  const uint32_t* hi_base;    // of the source
};

// does site i contribute to the row with state s?  sigma^- arrives at a set bit, sigma^+ at a clear one
template <int STEP>
__device__ __forceinline__ bool ladder_qualifies(uint64_t s, int i) {
  return ((s >> i) & 1ull) == (STEP > 0 ? 1ull : 0ull);
}

// sites whose table lookups and gathers a thread keeps in flight together: R * chunk doubles of gathered rows are live beside
// sum[R] (and acc[R] in the dots)
template <int R>
constexpr int ladder_chunk() {
  return R <= 2 ? 8 : (R == 4 ? 4 : 2);
}

// the source ranks of sites k0 .. k0 + CH - 1 of one group (the low sites 0 .. Llo - 1 or the high sites Llo .. L - 1) for the row
// with state s: one table read per contributing site, all requested before any is used; DSEA_LADDER_NO_RANK for a site that
// does not contribute (and past the group's end).  `word` is the row's word of the group (s >> Llo or s & lomask), `base` the
// first site of the group, `other` the row's own entry of the other table.
template <int STEP, int CH>
__device__ __forceinline__ void ladder_ranks(uint32_t (&rk)[CH], uint64_t s, bool have, int k0, int end, int base, uint32_t word,
                                             uint32_t other, const uint32_t* __restrict__ table) {
#pragma unroll
  for (int e = 0; e < CH; ++e) {
    const int i = k0 + e;
    const bool on = have && i < end && ladder_qualifies<STEP>(s, i);   // (i < 48: the shift is defined)
    rk[e] = DSEA_LADDER_NO_RANK;
    if (on) rk[e] = other + table[word ^ (1u << (i - base))];
  }
}

// one group of sites [base, end) of one row: use(i, X[rank_i, :]) for every site of the group in order (a row of zeros for a
// site that does not contribute).  A contributing site costs one table read and one block_load<R> of the source row; the
// table reads of chunk c + 1 are issued before the gathers of chunk c are consumed.
template <int STEP, int R, typename Use>
__device__ __forceinline__ void ladder_group(uint64_t s, bool have, int base, int end, uint32_t word, uint32_t other,
                                             const uint32_t* __restrict__ table, const double* __restrict__ X, Use use) {
  constexpr int CH = ladder_chunk<R>();
  uint32_t rkA[CH], rkB[CH];
  ladder_ranks<STEP, CH>(rkA, s, have, base, end, base, word, other, table);
  for (int k0 = base; k0 < end; k0 += CH) {
    double xv[CH][R];
#pragma unroll
    for (int e = 0; e < CH; ++e) {
#pragma unroll
      for (int j = 0; j < R; ++j) xv[e][j] = 0.0;
      if (rkA[e] != DSEA_LADDER_NO_RANK) block_load<R>(xv[e], X, (int64_t)rkA[e]);
    }
    ladder_ranks<STEP, CH>(rkB, s, have, k0 + CH, end, base, word, other, table);
#pragma unroll
    for (int e = 0; e < CH; ++e) {
      if (k0 + e < end) use(k0 + e, xv[e]);        // (the same for every lane)
      rkA[e] = rkB[e];
    }
  }
}

// the sites of the row with state st, STEP = +-1: the state's two words, the row's own entry of either table, then the low
// group and the high group
template <int STEP, int R, typename Use>
__device__ __forceinline__ void ladder_sites(const LadderParams& p, uint64_t st, bool have, uint64_t lomask,
                                             const double* __restrict__ X, Use use) {
  const uint32_t sl = (uint32_t)(st & lomask), sh = (uint32_t)(st >> p.Llo);
  const uint32_t own_hi = p.hi_base[sh], own_lo = p.lo_rank[sl];
  ladder_group<STEP, R>(st, have, 0, p.Llo, sl, own_hi, p.lo_rank, X, use);
  ladder_group<STEP, R>(st, have, p.Llo, p.L, sh, own_lo, p.hi_base, X, use);
}

// sum[j] = (S(c) X)[r, j] of the row r (row n - 1 for a thread without a row); a site that does not contribute adds a zero
// product, so every column sees the same operations in the same order whatever R
template <int STEP, int R>
__device__ __forceinline__ void ladder_row(const LadderParams& p, const double (&cw)[DSEA_SECTOR_MAX_L], uint64_t lomask, int64_t r,
                                           bool have, const double* __restrict__ X, double (&sum)[R]) {
  const int64_t rr = have ? r : p.n - 1;
  const uint64_t st = p.states[rr];
  if constexpr (STEP == 0) {
    double xr[R];
    block_load<R>(xr, X, rr);
    double diag = 0.0;
    for (int i = 0; i < p.L; ++i) diag += block_signed(cw[i], (st >> i) & 1ull);
#pragma unroll
    for (int j = 0; j < R; ++j) sum[j] = diag * xr[j];
  } else {
#pragma unroll
    for (int j = 0; j < R; ++j) sum[j] = 0.0;
    ladder_sites<STEP, R>(p, st, have, lomask, X, [&](int i, const double (&xrow)[R]) {
      const double w = cw[i];
#pragma unroll
      for (int j = 0; j < R; ++j) sum[j] = fma(w, xrow[j], sum[j]);
    });
  }
}
}  // namespace

// y = S(c) x.  One destination row per thread: states and y are read and written coalesced.  A block walks the row ranges
// blockIdx.x, + gridDim.x, ... of 256 rows; a thread past the last row reads row n - 1 and writes nothing.
template <int STEP>
__global__ __launch_bounds__(256) void k_sector_ladder(LadderParams p, const double* __restrict__ x, double* __restrict__ y) {
  __shared__ double cw[DSEA_SECTOR_MAX_L];
  const int64_t n = p.n;
  for (int c = threadIdx.x; c < p.L; c += 256) cw[c] = p.c[c];
  __syncthreads();
  const uint64_t lomask = (1ull << p.Llo) - 1;
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;
    double sum[1];
    if constexpr (STEP == 0) {   // Z(c) keeps the row it had, spelled out: docs/design/38-ladder-parts.md, 38.6
      const uint64_t st = p.states[have ? r : n - 1];
      const double xr = x[have ? r : n - 1];
      double diag = 0.0;
      for (int i = 0; i < p.L; ++i) diag += block_signed(cw[i], (st >> i) & 1ull);
      sum[0] = diag * xr;
    } else {
      ladder_row<STEP, 1>(p, cw, lomask, r, have, x, sum);
    }
    if (have) block_store<1>(y, r, sum);
  }
}

// The site forms: out[i] = v1^T (dS/dc_i) v2 for all L sites in one pass, v1 on the destination and v2 on the source:
//   STEP = +-1: sum_{r' : bit_i qualifies} v1[r'] v2[rank_src(...)]        STEP = 0: sum_r z_i v1[r] v2[r]
// The same row walk and the same chunks of lookups and gathers (of v2) as the map.  No per-lane accumulator per site: every
// term is reduced through the wave at once (wave_sum, fixed order) and lane 0 adds it to the wave's row of LDS accumulators; the
// four rows are added in fixed order and written to scratch[i * gridDim.x + block].  No atomics.
template <int STEP>
__global__ __launch_bounds__(256) void k_sector_ladder_forms(LadderParams p, const double* __restrict__ v1,
                                                             const double* __restrict__ v2, double* __restrict__ scratch) {
  __shared__ double accs[4][DSEA_SECTOR_MAX_L];
  const int L = p.L;
  const int64_t n = p.n;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double* __restrict__ mine = accs[wv];
  for (int c = lane; c < L; c += 64) mine[c] = 0.0;       // (afterwards a wave's row is touched by its lane 0 alone)
  __syncthreads();
  const uint64_t lomask = (1ull << p.Llo) - 1;
  auto add = [&](int term, double val) {
    const double tot = wave_sum(val);
    if (lane == 0) mine[term] += tot;
  };
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;                               // a thread without a row adds zeros to every form
    const uint64_t st = p.states[have ? r : n - 1];
    const double a = have ? v1[r] : 0.0;
    if constexpr (STEP == 0) {
      const double d = a * v2[have ? r : n - 1];
      for (int i = 0; i < L; ++i) add(i, block_signed(d, (st >> i) & 1ull));
    } else {
      ladder_sites<STEP, 1>(p, st, have, lomask, v2, [&](int i, const double (&xrow)[1]) { add(i, a * xrow[0]); });
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < L; c += 256)
    scratch[(int64_t)c * gridDim.x + blockIdx.x] = ((accs[0][c] + accs[1][c]) + accs[2][c]) + accs[3][c];
}

// second stage: out[i] = the sum of site i's per-block partials, fixed order; one block per form
__global__ __launch_bounds__(256) void k_sector_ladder_forms_reduce(const double* __restrict__ scratch, int count,
                                                                    double* __restrict__ out) {
  __shared__ double sm5[5];
  const double tot = sum_partials_block(scratch + (int64_t)blockIdx.x * count, count, sm5);
  if (threadIdx.x == 0) out[blockIdx.x] = tot;
}

// ---- the block forms (docs/design/35-finite-temperature-dynamics.md): the map and its column dots on blocks fp64 [n, R]
// row-major, R in {1, 2, 4, 8} (dsea_block.h)

// Y = S(c) X.  The grid, the 256-row ranges and the thread past the last row as in k_sector_ladder, which is this kernel at
// R = 1; column j of Y equals k_sector_ladder on column j of X bit for bit.
template <int STEP, int R>
__global__ __launch_bounds__(256) void k_sector_ladder_block(LadderParams p, const double* __restrict__ X, double* __restrict__ Y) {
  __shared__ double cw[DSEA_SECTOR_MAX_L];
  const int64_t n = p.n;
  for (int c = threadIdx.x; c < p.L; c += 256) cw[c] = p.c[c];
  __syncthreads();
  const uint64_t lomask = (1ull << p.Llo) - 1;
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;
    double sum[R];
    ladder_row<STEP, R>(p, cw, lomask, r, have, X, sum);
    if (have) block_store<R>(Y, r, sum);
  }
}

// The column dots d[j] = sum_r' Lft[r', j] (S(c) X)[r', j] without the product block: the same rows and the same sum[j], the
// row of Lft read after the last chunk's gathers are consumed, one accumulator per column and thread over the rows it walks
// (a thread without a row adds nothing), then block_partials into scratch[j * gridDim.x + block].
// k_sector_ladder_forms_reduce with R blocks closes them.  No atomics.
template <int STEP, int R>
__global__ __launch_bounds__(256) void k_sector_ladder_block_dots(LadderParams p, const double* __restrict__ Lft,
                                                                  const double* __restrict__ X, double* __restrict__ scratch) {
  __shared__ double cw[DSEA_SECTOR_MAX_L];
  __shared__ double sm[R][4];
  const int64_t n = p.n;
  for (int c = threadIdx.x; c < p.L; c += 256) cw[c] = p.c[c];
  __syncthreads();
  const uint64_t lomask = (1ull << p.Llo) - 1;
  double acc[R];
#pragma unroll
  for (int j = 0; j < R; ++j) acc[j] = 0.0;
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;
    double sum[R];
    ladder_row<STEP, R>(p, cw, lomask, r, have, X, sum);
    if (have) {
      double l[R];
      block_load<R>(l, Lft, r);
#pragma unroll
      for (int j = 0; j < R; ++j) acc[j] = fma(l[j], sum[j], acc[j]);
    }
  }
  block_partials<R>(acc, sm, scratch);
}

// the rows of the destination; false when either sector is outside the limits of sector_sizes or step outside -1 .. 1 (host
// arithmetic only)
bool ladder_sizes(int L, int ndown_src, int step, int64_t* n_src, int64_t* n_dst) {
  int64_t n_lo, n_hi;
  if (step < -1 || step > 1) return false;
  return sector_sizes(L, ndown_src, n_src, &n_lo, &n_hi) && sector_sizes(L, ndown_src + step, n_dst, &n_lo, &n_hi);
}

// the kernel arguments (c: the weights, null for the forms); false when an argument is out of range
static bool ladder_params(int L, int ndown_src, int step, int grid_log2, const double* c, const uint64_t* states_dst,
                          const uint32_t* lo_rank_src, const uint32_t* hi_base_src, LadderParams* p) {
  int64_t n_src, n_dst;
  if (!ladder_sizes(L, ndown_src, step, &n_src, &n_dst)) return false;
  if (!ladder_grid_ok(grid_log2)) return false;
  if (!states_dst || !lo_rank_src || !hi_base_src) return false;
  p->L = L;
  p->Llo = (L + 1) / 2;
  p->n = n_dst;
  p->c = c;
  p->states = states_dst;
  p->lo_rank = lo_rank_src;
  p->hi_base = hi_base_src;
  return true;
}

// the one place that turns the run-time step of a launch into the template argument (0 for anything but +-1)
template <class F>
static inline void dispatch_ladder_step(int step, F&& f) {
  dispatch_int<1, -1, 0>(step, f);
}

int launch_sector_ladder(int L, int ndown_src, int step, const double* c, const uint64_t* states_dst, const uint32_t* lo_rank_src,
                         const uint32_t* hi_base_src, const double* x, double* y, int grid_log2, hipStream_t st) {
  LadderParams p;
  if (!c || !ladder_params(L, ndown_src, step, grid_log2, c, states_dst, lo_rank_src, hi_base_src, &p)) return -1;
  const dim3 grid((unsigned)ladder_blocks(p.n, grid_log2));
  dispatch_ladder_step(step, [&](auto s) {
    hipLaunchKernelGGL((k_sector_ladder<decltype(s)::value>), grid, dim3(256), 0, st, p, x, y);
  });
  return 0;
}

int launch_sector_ladder_forms(int L, int ndown_src, int step, const uint64_t* states_dst, const uint32_t* lo_rank_src,
                               const uint32_t* hi_base_src, const double* v1, const double* v2, double* out, double* scratch,
                               int grid_log2, hipStream_t st) {
  LadderParams p;
  if (!ladder_params(L, ndown_src, step, grid_log2, nullptr, states_dst, lo_rank_src, hi_base_src, &p)) return -1;
  const int nblk = ladder_blocks(p.n, grid_log2);
  const dim3 grid((unsigned)nblk);
  dispatch_ladder_step(step, [&](auto s) {
    hipLaunchKernelGGL((k_sector_ladder_forms<decltype(s)::value>), grid, dim3(256), 0, st, p, v1, v2, scratch);
  });
  hipLaunchKernelGGL(k_sector_ladder_forms_reduce, dim3((unsigned)L), dim3(256), 0, st, scratch, nblk, out);
  return 0;
}

int launch_sector_ladder_block(int L, int ndown_src, int step, int R, const double* c, const uint64_t* states_dst,
                               const uint32_t* lo_rank_src, const uint32_t* hi_base_src, const double* X, double* Y, int grid_log2,
                               hipStream_t st) {
  LadderParams p;
  if (!c || !ladder_params(L, ndown_src, step, grid_log2, c, states_dst, lo_rank_src, hi_base_src, &p)) return -1;
  const dim3 grid((unsigned)ladder_blocks(p.n, grid_log2));
  dispatch_ladder_step(step, [&](auto s) {
    dispatch_block_width(R, [&](auto w) {
      hipLaunchKernelGGL((k_sector_ladder_block<decltype(s)::value, decltype(w)::value>), grid, dim3(256), 0, st, p, X, Y);
    });
  });
  return 0;
}

int launch_sector_ladder_block_dots(int L, int ndown_src, int step, int R, const double* c, const uint64_t* states_dst,
                                    const uint32_t* lo_rank_src, const uint32_t* hi_base_src, const double* Lft, const double* X,
                                    double* out, double* scratch, int grid_log2, hipStream_t st) {
  LadderParams p;
  if (!c || !ladder_params(L, ndown_src, step, grid_log2, c, states_dst, lo_rank_src, hi_base_src, &p)) return -1;
  const int nblk = ladder_blocks(p.n, grid_log2);
  const dim3 grid((unsigned)nblk);
  dispatch_ladder_step(step, [&](auto s) {
    dispatch_block_width(R, [&](auto w) {
      hipLaunchKernelGGL((k_sector_ladder_block_dots<decltype(s)::value, decltype(w)::value>), grid, dim3(256), 0, st, p, Lft, X,
                         scratch);
    });
  });
  hipLaunchKernelGGL(k_sector_ladder_forms_reduce, dim3((unsigned)R), dim3(256), 0, st, scratch, nblk, out);
  return 0;
}

}  // namespace dsea
