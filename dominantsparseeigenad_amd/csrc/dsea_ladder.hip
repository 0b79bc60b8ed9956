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
// Nothing here is shared with dsea_sector.hip: the file has its own helpers.  The block forms take the row access and the
// partials of a block from dsea_block.h.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_internal.h"
#include "dsea_device.h"
#include "dsea_block.h"

namespace dsea {

namespace {
#define DSEA_LADDER_CHUNK 8             /* sites whose table lookups and gathers a thread keeps in flight together */
#define DSEA_LADDER_NO_RANK 0xFFFFFFFFu /* "this site does not contribute to this row" (a rank is below 2^31) */

struct LadderParams {
  int L, Llo;
  int64_t n;                  // rows of the destination
  const double* c;            // the L site weights
  const uint64_t* states;     // of the destination
  const uint32_t* lo_rank;    // of the source
  const uint32_t* hi_base;    // of the source
};

// v * (1 - 2 bit), exact: the bit goes into the sign
__device__ __forceinline__ double ladder_signed(double v, uint64_t bit) {
  return __longlong_as_double(__double_as_longlong(v) ^ (long long)(bit << 63));
}
// does site i contribute to the row with state s?  sigma^- arrives at a set bit, sigma^+ at a clear one
template <int STEP>
__device__ __forceinline__ bool ladder_qualifies(uint64_t s, int i) {
  return ((s >> i) & 1ull) == (STEP > 0 ? 1ull : 0ull);
}

// the source ranks of sites k0 .. k0 + CHUNK - 1 of one group (the low sites 0 .. Llo - 1 or the high sites Llo .. L - 1) for the row with
// state s: one table read per contributing site, all requested before any is used; DSEA_LADDER_NO_RANK for a site that does
// not contribute (and past the group's end).  `word` is the row's word of the group (s >> Llo or s & lomask), `base` the
// first site of the group, `other` the row's own entry of the other table.
template <int STEP>
__device__ __forceinline__ void ladder_ranks(uint32_t (&rk)[DSEA_LADDER_CHUNK], uint64_t s, bool have, int k0, int end, int base,
                                             uint32_t word, uint32_t other, const uint32_t* __restrict__ table) {
#pragma unroll
  for (int e = 0; e < DSEA_LADDER_CHUNK; ++e) {
    const int i = k0 + e;
    const bool on = have && i < end && ladder_qualifies<STEP>(s, i);   // (i < 48: the shift is defined)
    rk[e] = DSEA_LADDER_NO_RANK;
    if (on) rk[e] = other + table[word ^ (1u << (i - base))];
  }
}
// the gathers of one chunk: v[rank], 0 where the site does not contribute
__device__ __forceinline__ void ladder_gather(double (&xv)[DSEA_LADDER_CHUNK], const uint32_t (&rk)[DSEA_LADDER_CHUNK],
                                              const double* __restrict__ v) {
#pragma unroll
  for (int e = 0; e < DSEA_LADDER_CHUNK; ++e) {
    xv[e] = 0.0;
    if (rk[e] != DSEA_LADDER_NO_RANK) xv[e] = v[rk[e]];
  }
}

// one group of sites [base, end) of one row: use(i, x[rank_i]) for every site of the group in order (0.0 for a site that does
// not contribute).  The table reads of chunk c + 1 are issued before the gathers of chunk c are consumed.
template <int STEP, typename Use>
__device__ __forceinline__ void ladder_group(uint64_t s, bool have, int base, int end, uint32_t word, uint32_t other,
                                             const uint32_t* __restrict__ table, const double* __restrict__ v, Use use) {
  uint32_t rkA[DSEA_LADDER_CHUNK], rkB[DSEA_LADDER_CHUNK];
  ladder_ranks<STEP>(rkA, s, have, base, end, base, word, other, table);
  for (int k0 = base; k0 < end; k0 += DSEA_LADDER_CHUNK) {
    double xv[DSEA_LADDER_CHUNK];
    ladder_gather(xv, rkA, v);
    ladder_ranks<STEP>(rkB, s, have, k0 + DSEA_LADDER_CHUNK, end, base, word, other, table);
#pragma unroll
    for (int e = 0; e < DSEA_LADDER_CHUNK; ++e) {
      if (k0 + e < end) use(k0 + e, xv[e]);        // (the same for every lane)
      rkA[e] = rkB[e];
    }
  }
}
}  // namespace

// y = S(c) x.  One destination row per thread: states and y are read and written coalesced.  A block walks the row ranges
// blockIdx.x, + gridDim.x, ... of 256 rows; a thread past the last row reads row n - 1 and writes nothing.
template <int STEP>
__global__ __launch_bounds__(256) void k_sector_ladder(LadderParams p, const double* __restrict__ x, double* __restrict__ y) {
  __shared__ double cw[DSEA_SECTOR_MAX_L];
  const int L = p.L, Llo = p.Llo;
  const int64_t n = p.n;
  for (int c = threadIdx.x; c < L; c += 256) cw[c] = p.c[c];
  __syncthreads();
  const uint64_t lomask = (1ull << Llo) - 1;
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;
    const uint64_t st = p.states[have ? r : n - 1];
    double sum = 0.0;
    if constexpr (STEP == 0) {
      const double xr = x[have ? r : n - 1];
      double diag = 0.0;
      for (int i = 0; i < L; ++i) diag += ladder_signed(cw[i], (st >> i) & 1ull);
      sum = diag * xr;
    } else {
      const uint32_t sl = (uint32_t)(st & lomask), sh = (uint32_t)(st >> Llo);
      const uint32_t own_hi = p.hi_base[sh], own_lo = p.lo_rank[sl];
      auto use = [&](int i, double xv) { sum = fma(cw[i], xv, sum); };
      ladder_group<STEP>(st, have, 0, Llo, sl, own_hi, p.lo_rank, x, use);
      ladder_group<STEP>(st, have, Llo, L, sh, own_lo, p.hi_base, x, use);
    }
    if (have) y[r] = sum;
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
  const int L = p.L, Llo = p.Llo;
  const int64_t n = p.n;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double* __restrict__ mine = accs[wv];
  for (int c = lane; c < L; c += 64) mine[c] = 0.0;       // (afterwards a wave's row is touched by its lane 0 alone)
  __syncthreads();
  const uint64_t lomask = (1ull << Llo) - 1;
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
      for (int i = 0; i < L; ++i) add(i, ladder_signed(d, (st >> i) & 1ull));
    } else {
      const uint32_t sl = (uint32_t)(st & lomask), sh = (uint32_t)(st >> Llo);
      const uint32_t own_hi = p.hi_base[sh], own_lo = p.lo_rank[sl];
      auto use = [&](int i, double xv) { add(i, a * xv); };
      ladder_group<STEP>(st, have, 0, Llo, sl, own_hi, p.lo_rank, v2, use);
      ladder_group<STEP>(st, have, Llo, L, sh, own_lo, p.hi_base, v2, use);
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
// row-major, R in {1, 2, 4, 8} (dsea_block.h).  The row walk is that of k_sector_ladder; what changes is that a contributing
// site costs one table read and one block_load<R> of the source row for all R columns.  The helpers are written apart from
// the single-vector ones above (whose chunk is a macro), so that those keep their instructions.
namespace {
// sites in flight per thread: R * chunk doubles of gathered rows are live beside sum[R] (and acc[R] in the dots)
template <int R>
constexpr int ladder_block_chunk() {
  return R <= 2 ? 8 : (R == 4 ? 4 : 2);
}

// ladder_ranks with the chunk as a template argument
template <int STEP, int CH>
__device__ __forceinline__ void ladder_block_ranks(uint32_t (&rk)[CH], uint64_t s, bool have, int k0, int end, int base, uint32_t word,
                                                   uint32_t other, const uint32_t* __restrict__ table) {
#pragma unroll
  for (int e = 0; e < CH; ++e) {
    const int i = k0 + e;
    const bool on = have && i < end && ladder_qualifies<STEP>(s, i);
    rk[e] = DSEA_LADDER_NO_RANK;
    if (on) rk[e] = other + table[word ^ (1u << (i - base))];
  }
}

// one group of sites [base, end) of one row: sum[j] = fma(cw[i], X[rank_i, j], sum[j]) for every site of the group in order
// (X[rank_i, :] = 0 for a site that does not contribute: the single-vector kernel adds the same zero product).  The table
// reads of chunk c + 1 are issued before the gathers of chunk c are consumed.
template <int STEP, int R>
__device__ __forceinline__ void ladder_block_group(uint64_t s, bool have, int base, int end, uint32_t word, uint32_t other,
                                                   const uint32_t* __restrict__ table, const double* __restrict__ X,
                                                   const double (&cw)[DSEA_SECTOR_MAX_L], double (&sum)[R]) {
  constexpr int CH = ladder_block_chunk<R>();
  uint32_t rkA[CH], rkB[CH];
  ladder_block_ranks<STEP, CH>(rkA, s, have, base, end, base, word, other, table);
  for (int k0 = base; k0 < end; k0 += CH) {
    double xv[CH][R];
#pragma unroll
    for (int e = 0; e < CH; ++e) {
#pragma unroll
      for (int j = 0; j < R; ++j) xv[e][j] = 0.0;
      if (rkA[e] != DSEA_LADDER_NO_RANK) block_load<R>(xv[e], X, (int64_t)rkA[e]);
    }
    ladder_block_ranks<STEP, CH>(rkB, s, have, k0 + CH, end, base, word, other, table);
#pragma unroll
    for (int e = 0; e < CH; ++e) {
      if (k0 + e < end) {                          // (the same for every lane)
        const double w = cw[k0 + e];
#pragma unroll
        for (int j = 0; j < R; ++j) sum[j] = fma(w, xv[e][j], sum[j]);
      }
      rkA[e] = rkB[e];
    }
  }
}

// sum[j] = (S(c) X)[r, j] of the row r (row n - 1 for a thread without a row): column j in the operations and the order of
// k_sector_ladder on column j
template <int STEP, int R>
__device__ __forceinline__ void ladder_block_row(const LadderParams& p, const double (&cw)[DSEA_SECTOR_MAX_L], uint64_t lomask,
                                                 int64_t r, bool have, const double* __restrict__ X, double (&sum)[R]) {
  const int64_t rr = have ? r : p.n - 1;
  const uint64_t st = p.states[rr];
  if constexpr (STEP == 0) {
    double xr[R];
    block_load<R>(xr, X, rr);
    double diag = 0.0;
    for (int i = 0; i < p.L; ++i) diag += ladder_signed(cw[i], (st >> i) & 1ull);
#pragma unroll
    for (int j = 0; j < R; ++j) sum[j] = diag * xr[j];
  } else {
#pragma unroll
    for (int j = 0; j < R; ++j) sum[j] = 0.0;
    const uint32_t sl = (uint32_t)(st & lomask), sh = (uint32_t)(st >> p.Llo);
    const uint32_t own_hi = p.hi_base[sh], own_lo = p.lo_rank[sl];
    ladder_block_group<STEP, R>(st, have, 0, p.Llo, sl, own_hi, p.lo_rank, X, cw, sum);
    ladder_block_group<STEP, R>(st, have, p.Llo, p.L, sh, own_lo, p.hi_base, X, cw, sum);
  }
}
}  // namespace

// Y = S(c) X.  The grid, the 256-row ranges and the thread past the last row as in k_sector_ladder; column j of Y equals
// k_sector_ladder on column j of X bit for bit.
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
    ladder_block_row<STEP, R>(p, cw, lomask, r, have, X, sum);
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
    ladder_block_row<STEP, R>(p, cw, lomask, r, have, X, sum);
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

// one block per 256 rows up to the cap 2^grid_log2 (6 .. 12; 0 = 12); beyond it blocks walk row ranges
static inline int ladder_blocks(int64_t n, int grid_log2) {
  int64_t nblk = (n + 255) / 256;
  const int64_t cap = (int64_t)1 << (grid_log2 == 0 ? 12 : grid_log2);
  if (nblk > cap) nblk = cap;
  return (int)nblk;
}

// partials per form that launch_sector_ladder_forms may write at any grid cap: the largest cap gives the most blocks
int64_t ladder_forms_scratch_doubles(int64_t n_dst, int L) {
  int64_t nblk = (n_dst + 255) / 256;
  if (nblk > DSEA_MAX_TFIM_BLOCKS) nblk = DSEA_MAX_TFIM_BLOCKS;
  return (int64_t)L * nblk;
}

// the kernel arguments (c: the weights, null for the forms); false when an argument is out of range
static bool ladder_params(int L, int ndown_src, int step, int grid_log2, const double* c, const uint64_t* states_dst,
                          const uint32_t* lo_rank_src, const uint32_t* hi_base_src, LadderParams* p) {
  int64_t n_src, n_dst;
  if (!ladder_sizes(L, ndown_src, step, &n_src, &n_dst)) return false;
  if (grid_log2 != 0 && (grid_log2 < 6 || grid_log2 > 12)) return false;
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

int launch_sector_ladder(int L, int ndown_src, int step, const double* c, const uint64_t* states_dst, const uint32_t* lo_rank_src,
                         const uint32_t* hi_base_src, const double* x, double* y, int grid_log2, hipStream_t st) {
  LadderParams p;
  if (!c || !ladder_params(L, ndown_src, step, grid_log2, c, states_dst, lo_rank_src, hi_base_src, &p)) return -1;
  const dim3 grid((unsigned)ladder_blocks(p.n, grid_log2));
  if (step > 0) hipLaunchKernelGGL((k_sector_ladder<1>), grid, dim3(256), 0, st, p, x, y);
  else if (step < 0) hipLaunchKernelGGL((k_sector_ladder<-1>), grid, dim3(256), 0, st, p, x, y);
  else hipLaunchKernelGGL((k_sector_ladder<0>), grid, dim3(256), 0, st, p, x, y);
  return 0;
}

int launch_sector_ladder_forms(int L, int ndown_src, int step, const uint64_t* states_dst, const uint32_t* lo_rank_src,
                               const uint32_t* hi_base_src, const double* v1, const double* v2, double* out, double* scratch,
                               int grid_log2, hipStream_t st) {
  LadderParams p;
  if (!ladder_params(L, ndown_src, step, grid_log2, nullptr, states_dst, lo_rank_src, hi_base_src, &p)) return -1;
  const int nblk = ladder_blocks(p.n, grid_log2);
  const dim3 grid((unsigned)nblk);
  if (step > 0) hipLaunchKernelGGL((k_sector_ladder_forms<1>), grid, dim3(256), 0, st, p, v1, v2, scratch);
  else if (step < 0) hipLaunchKernelGGL((k_sector_ladder_forms<-1>), grid, dim3(256), 0, st, p, v1, v2, scratch);
  else hipLaunchKernelGGL((k_sector_ladder_forms<0>), grid, dim3(256), 0, st, p, v1, v2, scratch);
  hipLaunchKernelGGL(k_sector_ladder_forms_reduce, dim3((unsigned)L), dim3(256), 0, st, scratch, nblk, out);
  return 0;
}

// partials that launch_sector_ladder_block_dots may write at any grid cap
int64_t ladder_block_dots_scratch_doubles(int64_t n_dst, int R) {
  int64_t nblk = (n_dst + 255) / 256;
  if (nblk > DSEA_MAX_TFIM_BLOCKS) nblk = DSEA_MAX_TFIM_BLOCKS;
  return (int64_t)R * nblk;
}

// the one place that turns the run-time step of a block launch into the template argument (0 for anything but +-1)
template <class F>
static inline void dispatch_ladder_step(int step, F&& f) {
  dispatch_int<1, -1, 0>(step, f);
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
