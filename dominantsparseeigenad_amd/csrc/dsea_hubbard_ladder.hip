// dsea_hubbard_ladder.hip -- linear maps between two particle-number sectors of the Hubbard space of the same L sites
// (docs/design/25-hubbard-ladder.md): the ladder k_hubbard_ladder<SPECIES, STEP>, its site forms
// k_hubbard_ladder_forms<SPECIES, STEP> (+ k_hubbard_ladder_forms_reduce), the block forms k_hubbard_ladder_block<SPECIES, STEP, R>
// and k_hubbard_ladder_block_dots<SPECIES, STEP, R> (docs/design/37-hubbard-finite-temperature-dynamics.md), and their launchers.
//
// Conventions of docs/design/19-hubbard.md: bit i of the word u is the occupation of (i, up), bit i of d that of (i, dn);
// |u, d> = (prod_{i in u, ascending} c+_{i up}) (prod_{j in d, ascending} c+_{j dn}) |0>; row r = ru * n_dn + rd.  With
// below_i = (1 << i) - 1, par(w) = popcount(w) & 1 and site weights c (fp64 [L], read through their device pointer on every
// launch), SPECIES up (0) takes (nup, ndn) to (nup + STEP, ndn); u' is the up word of the destination row:
//   STEP = +1, sum_i c_i c+_{i up}:  y[ru' n_dn + rd] = sum_{i : bit_i(u') = 1} c_i (-1)^par(u' & below_i) x[rank_src(u' ^ (1 << i)) n_dn + rd]
//   STEP = -1, sum_i c_i c_{i up}:   y[ru' n_dn + rd] = sum_{i : bit_i(u') = 0} c_i (-1)^par(u' & below_i) x[rank_src(u' | (1 << i)) n_dn + rd]
//   STEP =  0, sum_i c_i n_{i up}:   y[r] = (sum_i c_i bit_i(u)) x[r]
// SPECIES dn (1) takes (nup, ndn) to (nup, ndn + STEP); the row stride is n_dn_dst = C(L, ndn + STEP) on the destination and
// n_dn_src = C(L, ndn) in the gather, and every down operator stands right of all nup up operators: g = (-1)^nup for STEP +-1,
//   y[ru n_dn_dst + rd'] = g sum_{i : bit_i(d') qualifies} c_i (-1)^par(d' & below_i) x[ru n_dn_src + rank_src(d' ^ (1 << i))]
// All are gathers over the destination rows: no scatter, no atomic.  Only the word of the moving species is read, from the
// state table of its destination count; rank_src(w) = hi_base_src[w >> Llo] + lo_rank_src[w & (2^Llo - 1)], Llo = (L + 1) / 2,
// are the two tables of its source count (dsea_sector_build_tables).  Flipping one bit changes one of the two words only, so a
// row loads its own hi_base_src[w >> Llo] and lo_rank_src[w & lomask] once; a site below Llo then costs one lo_rank read and
// one gather, a site at or above Llo one hi_base read and one gather.  The sites are walked in ascending order, so
// par(w & below_i) is a running parity: it goes into the sign bit of the weight (exact), and g is its starting value.
// The device helpers are the file's own: nothing is shared with dsea_hubbard.hip, and the site walk differs from that of
// dsea_ladder.hip by the running parity and the row arithmetic.  The block forms take the row access and the partials of a
// block from dsea_block.h; the grid rules are those of both ladder files, in dsea_internal.h (docs/design/38-ladder-parts.md).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_internal.h"
#include "dsea_device.h"
#include "dsea_block.h"

namespace dsea {

namespace {
#define DSEA_HLADDER_CHUNK 8   /* sites whose table lookups and gathers a thread keeps in flight together */
#define DSEA_HLADDER_NO_ROW 0xFFFFFFFFu /* "this site does not contribute to this row" (a row is below 2^31) */

struct HubbardLadderParams {
  int L, Llo;
  uint32_t n_dn_dst, n_dn_src;   // the row strides of the destination and of the source (equal for the up species)
  uint32_t g;                    // the starting parity: nup & 1 for the down species with step +-1, else 0
  int64_t n;                     // rows of the destination
  const double* c;               // the L site weights
  const uint64_t* states;        // of the moving species at its destination count
  const uint32_t* lo_rank;       // of the moving species at its source count
  const uint32_t* hi_base;
};

__device__ __forceinline__ uint32_t hladder_bit(uint64_t w, int i) { return (uint32_t)((w >> i) & 1ull); }
// does site i contribute to the row whose moving word is w?  c+ arrives at an occupied site, c at an empty one
template <int STEP>
__device__ __forceinline__ bool hladder_qualifies(uint64_t w, int i) {
  return hladder_bit(w, i) == (STEP > 0 ? 1u : 0u);
}

// the table reads of sites k0 .. k0 + CHUNK - 1 of one group (the low sites 0 .. Llo - 1 or the high sites Llo .. L - 1) for the
// row with the moving word w: one read per contributing site, requested and NOT used here.  Returns the contributing slots as
// a bit mask; the others (and those past the group's end) issue no load and leave tv as it is.  `word` is the row's word of the
// group (w >> Llo or w & lomask), `base` the first site of the group.
template <int STEP>
__device__ __forceinline__ uint32_t hladder_lookups(uint32_t (&tv)[DSEA_HLADDER_CHUNK], uint64_t w, bool have, int k0, int end,
                                                    int base, uint32_t word, const uint32_t* __restrict__ table) {
  uint32_t on = 0;
#pragma unroll
  for (int e = 0; e < DSEA_HLADDER_CHUNK; ++e) {
    const int i = k0 + e;
    if (have && i < end && hladder_qualifies<STEP>(w, i)) {   // (i < 40: the shifts are defined)
      tv[e] = table[word ^ (1u << (i - base))];
      on |= 1u << e;
    }
  }
  return on;
}
// the partner rows of one chunk from its table reads, DSEA_HLADDER_NO_ROW in the slots that do not contribute (selects, outside
// the predicated loads: one wait for the chunk's table values instead of one per site).  The partner's rank in the moving
// species is other + tv (`other`: the row's own entry of the other table); the up partner keeps rd, the down partner keeps ru:
// row = rank * mul + add with (mul, add) = (n_dn, rd) for the up species and rank + ru * n_dn_src for the down species.
template <int SPECIES>
__device__ __forceinline__ void hladder_rows(uint32_t (&rw)[DSEA_HLADDER_CHUNK], uint32_t on, const uint32_t (&tv)[DSEA_HLADDER_CHUNK],
                                             uint32_t other, uint32_t mul, uint32_t add) {
#pragma unroll
  for (int e = 0; e < DSEA_HLADDER_CHUNK; ++e) {
    const uint32_t rank = other + tv[e];
    rw[e] = (on >> e) & 1u ? (SPECIES == 0 ? rank * mul + add : rank + add) : DSEA_HLADDER_NO_ROW;
  }
}
// the gathers of one chunk: v[row], 0 where the site does not contribute.  A load is issued only for a contributing site,
// where the index is a row of the source.
__device__ __forceinline__ void hladder_gather(double (&xv)[DSEA_HLADDER_CHUNK], const uint32_t (&rw)[DSEA_HLADDER_CHUNK],
                                               const double* __restrict__ v) {
#pragma unroll
  for (int e = 0; e < DSEA_HLADDER_CHUNK; ++e) {
    xv[e] = 0.0;
    if (rw[e] != DSEA_HLADDER_NO_ROW) xv[e] = v[rw[e]];
  }
}

// one group of sites [base, end) of one row: use(i, x[partner_i]) for every site of the group in ascending order (0.0 for a
// site that does not contribute).  The table reads of chunk c + 1 are issued before the gathers of chunk c are consumed.
template <int SPECIES, int STEP, typename Use>
__device__ __forceinline__ void hladder_group(uint64_t w, bool have, int base, int end, uint32_t word, uint32_t other,
                                              uint32_t mul, uint32_t add, const uint32_t* __restrict__ table,
                                              const double* __restrict__ v, Use use) {
  uint32_t tv[DSEA_HLADDER_CHUNK];
  uint32_t on = hladder_lookups<STEP>(tv, w, have, base, end, base, word, table);
  for (int k0 = base; k0 < end; k0 += DSEA_HLADDER_CHUNK) {
    uint32_t rw[DSEA_HLADDER_CHUNK];
    double xv[DSEA_HLADDER_CHUNK];
    hladder_rows<SPECIES>(rw, on, tv, other, mul, add);
    hladder_gather(xv, rw, v);
    on = hladder_lookups<STEP>(tv, w, have, k0 + DSEA_HLADDER_CHUNK, end, base, word, table);
#pragma unroll
    for (int e = 0; e < DSEA_HLADDER_CHUNK; ++e)
      if (k0 + e < end) use(k0 + e, xv[e]);        // (the same for every lane)
  }
}

// (ru, rd) of the row rr by one 32-bit division with the stride of the DESTINATION; the rank of the moving species' word
struct HubbardLadderRow {
  uint32_t ru, rd;
};
__device__ __forceinline__ HubbardLadderRow hladder_row(uint32_t rr, uint32_t n_dn_dst) {
  HubbardLadderRow q;
  q.ru = rr / n_dn_dst;
  q.rd = rr - q.ru * n_dn_dst;
  return q;
}
}  // namespace

// y = S(c) x.  One destination row per thread: x (step 0) and y are read and written coalesced.  A block walks the row ranges
// blockIdx.x, + gridDim.x, ... of 256 rows; a thread past the last row reads row n - 1 and writes nothing.
template <int SPECIES, int STEP>
__global__ __launch_bounds__(256) void k_hubbard_ladder(HubbardLadderParams p, const double* __restrict__ x,
                                                        double* __restrict__ y) {
  __shared__ double cw[DSEA_SECTOR_MAX_L];
  const int L = p.L, Llo = p.Llo;
  const int64_t n = p.n;
  for (int c = threadIdx.x; c < L; c += 256) cw[c] = p.c[c];
  __syncthreads();
  const uint64_t lomask = (1ull << Llo) - 1;
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;
    const uint32_t rr = (uint32_t)(have ? r : n - 1);
    const HubbardLadderRow q = hladder_row(rr, p.n_dn_dst);
    const uint64_t w = p.states[SPECIES == 0 ? q.ru : q.rd];
    double sum = 0.0;
    if constexpr (STEP == 0) {
      const double xr = x[rr];
      double diag = 0.0;
      for (int i = 0; i < L; ++i) diag += hladder_bit(w, i) ? cw[i] : 0.0;
      sum = diag * xr;
    } else {
      const uint32_t wl = (uint32_t)(w & lomask), wh = (uint32_t)(w >> Llo);
      const uint32_t own_hi = p.hi_base[wh], own_lo = p.lo_rank[wl];
      const uint32_t mul = p.n_dn_src, add = SPECIES == 0 ? q.rd : q.ru * p.n_dn_src;
      uint32_t par = p.g;                          // the parity of the particles below the site, times the sector sign
      auto use = [&](int i, double xv) {
        sum = fma(block_signed(cw[i], par), xv, sum);
        par ^= hladder_bit(w, i);
      };
      hladder_group<SPECIES, STEP>(w, have, 0, Llo, wl, own_hi, mul, add, p.lo_rank, x, use);
      hladder_group<SPECIES, STEP>(w, have, Llo, L, wh, own_lo, mul, add, p.hi_base, x, use);
    }
    if (have) y[r] = sum;
  }
}

// The site forms: out[i] = v1^T (dS/dc_i) v2 for all L sites in one pass, v1 on the destination and v2 on the source:
//   STEP = +-1: sum_{rows : bit_i qualifies} (+-) v1[row] v2[partner row]        STEP = 0: sum_r bit_i v1[r] v2[r]
// The same row walk and the same chunks of lookups and gathers (of v2) as the map.  No per-lane accumulator per site: every
// term is reduced through the wave at once (wave_sum, fixed order) and lane 0 adds it to the wave's row of LDS accumulators; the
// four rows are added in fixed order and written to scratch[i * gridDim.x + block].  No atomics.
template <int SPECIES, int STEP>
__global__ __launch_bounds__(256) void k_hubbard_ladder_forms(HubbardLadderParams p, const double* __restrict__ v1,
                                                              const double* __restrict__ v2, double* __restrict__ scratch) {
  __shared__ double accs[4][DSEA_SECTOR_MAX_L];
  const int L = p.L, Llo = p.Llo;
  const int64_t n = p.n;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double* __restrict__ mine = accs[wv];
  for (int c = lane; c < L; c += 64) mine[c] = 0.0;       // (afterwards a wave's row is touched by its lane 0 alone)
  __syncthreads();
  const uint64_t lomask = (1ull << Llo) - 1;
  auto add_form = [&](int term, double val) {
    const double tot = wave_sum(val);
    if (lane == 0) mine[term] += tot;
  };
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;                               // a thread without a row adds zeros to every form
    const uint32_t rr = (uint32_t)(have ? r : n - 1);
    const HubbardLadderRow q = hladder_row(rr, p.n_dn_dst);
    const uint64_t w = p.states[SPECIES == 0 ? q.ru : q.rd];
    const double a = have ? v1[rr] : 0.0;
    if constexpr (STEP == 0) {
      const double d = a * v2[rr];
      for (int i = 0; i < L; ++i) add_form(i, hladder_bit(w, i) ? d : 0.0);
    } else {
      const uint32_t wl = (uint32_t)(w & lomask), wh = (uint32_t)(w >> Llo);
      const uint32_t own_hi = p.hi_base[wh], own_lo = p.lo_rank[wl];
      const uint32_t mul = p.n_dn_src, add = SPECIES == 0 ? q.rd : q.ru * p.n_dn_src;
      uint32_t par = p.g;
      auto use = [&](int i, double xv) {
        add_form(i, a * block_signed(xv, par));
        par ^= hladder_bit(w, i);
      };
      hladder_group<SPECIES, STEP>(w, have, 0, Llo, wl, own_hi, mul, add, p.lo_rank, v2, use);
      hladder_group<SPECIES, STEP>(w, have, Llo, L, wh, own_lo, mul, add, p.hi_base, v2, use);
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < L; c += 256)
    scratch[(int64_t)c * gridDim.x + blockIdx.x] = ((accs[0][c] + accs[1][c]) + accs[2][c]) + accs[3][c];
}

// second stage: out[i] = the sum of site i's per-block partials, fixed order; one block per form
__global__ __launch_bounds__(256) void k_hubbard_ladder_forms_reduce(const double* __restrict__ scratch, int count,
                                                                     double* __restrict__ out) {
  __shared__ double sm5[5];
  const double tot = sum_partials_block(scratch + (int64_t)blockIdx.x * count, count, sm5);
  if (threadIdx.x == 0) out[blockIdx.x] = tot;
}

// ---- the block forms (docs/design/37-hubbard-finite-temperature-dynamics.md): the map and its column dots on blocks fp64
// [n, R] row-major, R in {1, 2, 4, 8} (dsea_block.h).  The row walk is that of k_hubbard_ladder; what changes is that a
// contributing site costs one table read and one block_load<R> of the source row for all R columns.  The block walk
// (hladder_block_rows: the partner row formed inside the predicated table read) and the single-vector walk (hladder_lookups +
// hladder_rows: the selects outside the loads, one wait per chunk) are two schedules, not two spellings of one
// (docs/design/38-ladder-parts.md).
namespace {
// sites in flight per thread: R * chunk doubles of gathered rows are live beside sum[R] (and acc[R] in the dots)
template <int R>
constexpr int hladder_block_chunk() {
  return R <= 2 ? 8 : (R == 4 ? 4 : 2);
}

// the partner rows of sites k0 .. k0 + CH - 1 of one group: hladder_lookups and hladder_rows with the chunk as a template
// argument, DSEA_HLADDER_NO_ROW (and no table read) for a site that does not contribute or lies past the group's end
template <int SPECIES, int STEP, int CH>
__device__ __forceinline__ void hladder_block_rows(uint32_t (&rw)[CH], uint64_t w, bool have, int k0, int end, int base,
                                                   uint32_t word, uint32_t other, uint32_t mul, uint32_t add,
                                                   const uint32_t* __restrict__ table) {
#pragma unroll
  for (int e = 0; e < CH; ++e) {
    const int i = k0 + e;
    const bool on = have && i < end && hladder_qualifies<STEP>(w, i);   // (i < 40: the shifts are defined)
    rw[e] = DSEA_HLADDER_NO_ROW;
    if (on) {
      const uint32_t rank = other + table[word ^ (1u << (i - base))];
      rw[e] = SPECIES == 0 ? rank * mul + add : rank + add;
    }
  }
}

// one group of sites [base, end) of one row: sum[j] = fma(+-cw[i], X[partner_i, j], sum[j]) for every site of the group in
// ascending order (X[partner_i, :] = 0 for a site that does not contribute: the single-vector kernel adds the same zero
// product).  The table reads of chunk c + 1 are issued before the gathers of chunk c are consumed.
template <int SPECIES, int STEP, int R>
__device__ __forceinline__ void hladder_block_group(uint64_t w, bool have, int base, int end, uint32_t word, uint32_t other,
                                                    uint32_t mul, uint32_t add, const uint32_t* __restrict__ table,
                                                    const double* __restrict__ X, const double (&cw)[DSEA_SECTOR_MAX_L],
                                                    uint32_t& par, double (&sum)[R]) {
  constexpr int CH = hladder_block_chunk<R>();
  uint32_t rwA[CH], rwB[CH];
  hladder_block_rows<SPECIES, STEP, CH>(rwA, w, have, base, end, base, word, other, mul, add, table);
  for (int k0 = base; k0 < end; k0 += CH) {
    double xv[CH][R];
#pragma unroll
    for (int e = 0; e < CH; ++e) {
#pragma unroll
      for (int j = 0; j < R; ++j) xv[e][j] = 0.0;
      if (rwA[e] != DSEA_HLADDER_NO_ROW) block_load<R>(xv[e], X, (int64_t)rwA[e]);
    }
    hladder_block_rows<SPECIES, STEP, CH>(rwB, w, have, k0 + CH, end, base, word, other, mul, add, table);
#pragma unroll
    for (int e = 0; e < CH; ++e) {
      if (k0 + e < end) {                          // (the same for every lane)
        const double c = block_signed(cw[k0 + e], par);
#pragma unroll
        for (int j = 0; j < R; ++j) sum[j] = fma(c, xv[e][j], sum[j]);
        par ^= hladder_bit(w, k0 + e);
      }
      rwA[e] = rwB[e];
    }
  }
}

// sum[j] = (S(c) X)[r, j] of the row r (row n - 1 for a thread without a row): column j in the operations and the order of
// k_hubbard_ladder on column j
template <int SPECIES, int STEP, int R>
__device__ __forceinline__ void hladder_block_row(const HubbardLadderParams& p, const double (&cw)[DSEA_SECTOR_MAX_L],
                                                  uint64_t lomask, int64_t r, bool have, const double* __restrict__ X,
                                                  double (&sum)[R]) {
  const uint32_t rr = (uint32_t)(have ? r : p.n - 1);
  const HubbardLadderRow q = hladder_row(rr, p.n_dn_dst);
  const uint64_t w = p.states[SPECIES == 0 ? q.ru : q.rd];
  if constexpr (STEP == 0) {
    double xr[R];
    block_load<R>(xr, X, (int64_t)rr);
    double diag = 0.0;
    for (int i = 0; i < p.L; ++i) diag += hladder_bit(w, i) ? cw[i] : 0.0;
#pragma unroll
    for (int j = 0; j < R; ++j) sum[j] = diag * xr[j];
  } else {
#pragma unroll
    for (int j = 0; j < R; ++j) sum[j] = 0.0;
    const uint32_t wl = (uint32_t)(w & lomask), wh = (uint32_t)(w >> p.Llo);
    const uint32_t own_hi = p.hi_base[wh], own_lo = p.lo_rank[wl];
    const uint32_t mul = p.n_dn_src, add = SPECIES == 0 ? q.rd : q.ru * p.n_dn_src;
    uint32_t par = p.g;                            // the parity of the particles below the site, times the sector sign
    hladder_block_group<SPECIES, STEP, R>(w, have, 0, p.Llo, wl, own_hi, mul, add, p.lo_rank, X, cw, par, sum);
    hladder_block_group<SPECIES, STEP, R>(w, have, p.Llo, p.L, wh, own_lo, mul, add, p.hi_base, X, cw, par, sum);
  }
}
}  // namespace

// Y = S(c) X.  The grid, the 256-row ranges and the thread past the last row as in k_hubbard_ladder; column j of Y equals
// k_hubbard_ladder on column j of X bit for bit.  At STEP = 0 a thread reads its row of X before it writes that row of Y.
template <int SPECIES, int STEP, int R>
__global__ __launch_bounds__(256) void k_hubbard_ladder_block(HubbardLadderParams p, const double* __restrict__ X,
                                                              double* __restrict__ Y) {
  __shared__ double cw[DSEA_SECTOR_MAX_L];
  const int64_t n = p.n;
  for (int c = threadIdx.x; c < p.L; c += 256) cw[c] = p.c[c];
  __syncthreads();
  const uint64_t lomask = (1ull << p.Llo) - 1;
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;
    double sum[R];
    hladder_block_row<SPECIES, STEP, R>(p, cw, lomask, r, have, X, sum);
    if (have) block_store<R>(Y, r, sum);
  }
}

// The column dots d[j] = sum_r' Lft[r', j] (S(c) X)[r', j] without the product block: the same rows and the same sum[j], the
// row of Lft read after the last chunk's gathers are consumed, one accumulator per column and thread over the rows it walks
// (a thread without a row adds nothing), then block_partials into scratch[j * gridDim.x + block].
// k_hubbard_ladder_forms_reduce with R blocks closes them.  No atomics.
template <int SPECIES, int STEP, int R>
__global__ __launch_bounds__(256) void k_hubbard_ladder_block_dots(HubbardLadderParams p, const double* __restrict__ Lft,
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
    hladder_block_row<SPECIES, STEP, R>(p, cw, lomask, r, have, X, sum);
    if (have) {
      double l[R];
      block_load<R>(l, Lft, r);
#pragma unroll
      for (int j = 0; j < R; ++j) acc[j] = fma(l[j], sum[j], acc[j]);
    }
  }
  block_partials<R>(acc, sm, scratch);
}

// the rows and the down strides of the two sectors; false when species is outside {0, 1}, step outside -1 .. 1, or either
// sector outside the limits of hubbard_sizes (host arithmetic only)
bool hubbard_ladder_sizes(int L, int nup_src, int ndn_src, int species, int step, int64_t* n_src, int64_t* n_dst,
                          int64_t* n_dn_src, int64_t* n_dn_dst) {
  int64_t n_up;
  if (species < 0 || species > 1 || step < -1 || step > 1) return false;
  const int nup_dst = nup_src + (species == 0 ? step : 0), ndn_dst = ndn_src + (species == 1 ? step : 0);
  return hubbard_sizes(L, nup_src, ndn_src, n_src, &n_up, n_dn_src) && hubbard_sizes(L, nup_dst, ndn_dst, n_dst, &n_up, n_dn_dst);
}

// the kernel arguments (c: the weights, null for the forms); false when an argument is out of range
static bool hubbard_ladder_params(int L, int nup_src, int ndn_src, int species, int step, int grid_log2, const double* c,
                                  const uint64_t* states_dst, const uint32_t* lo_rank_src, const uint32_t* hi_base_src,
                                  HubbardLadderParams* p) {
  int64_t n_src, n_dst, n_dn_src, n_dn_dst;
  if (!hubbard_ladder_sizes(L, nup_src, ndn_src, species, step, &n_src, &n_dst, &n_dn_src, &n_dn_dst)) return false;
  if (!ladder_grid_ok(grid_log2)) return false;
  if (!states_dst || !lo_rank_src || !hi_base_src) return false;
  p->L = L;
  p->Llo = (L + 1) / 2;
  p->n_dn_dst = (uint32_t)n_dn_dst;
  p->n_dn_src = (uint32_t)n_dn_src;
  p->g = species == 1 && step != 0 ? (uint32_t)(nup_src & 1) : 0u;
  p->n = n_dst;
  p->c = c;
  p->states = states_dst;
  p->lo_rank = lo_rank_src;
  p->hi_base = hi_base_src;
  return true;
}

// the one place that turns the run-time (species, step) of a launch into template arguments: f(int_c<SPECIES>, int_c<STEP>),
// species 1 for anything but 0 and step 0 for anything but +-1 (hubbard_ladder_params has refused those)
template <class F>
static inline void hubbard_ladder_dispatch(int species, int step, F&& f) {
  dispatch_int<0, 1>(species, [&](auto sp) { dispatch_int<1, -1, 0>(step, [&](auto stp) { f(sp, stp); }); });
}

int launch_hubbard_ladder(int L, int nup_src, int ndn_src, int species, int step, const double* c, const uint64_t* states_dst,
                          const uint32_t* lo_rank_src, const uint32_t* hi_base_src, const double* x, double* y, int grid_log2,
                          hipStream_t st) {
  HubbardLadderParams p;
  if (!c || !hubbard_ladder_params(L, nup_src, ndn_src, species, step, grid_log2, c, states_dst, lo_rank_src, hi_base_src, &p))
    return -1;
  const dim3 grid((unsigned)ladder_blocks(p.n, grid_log2));
  hubbard_ladder_dispatch(species, step, [&](auto sp, auto stp) {
    hipLaunchKernelGGL((k_hubbard_ladder<decltype(sp)::value, decltype(stp)::value>), grid, dim3(256), 0, st, p, x, y);
  });
  return 0;
}

int launch_hubbard_ladder_forms(int L, int nup_src, int ndn_src, int species, int step, const uint64_t* states_dst,
                                const uint32_t* lo_rank_src, const uint32_t* hi_base_src, const double* v1, const double* v2,
                                double* out, double* scratch, int grid_log2, hipStream_t st) {
  HubbardLadderParams p;
  if (!hubbard_ladder_params(L, nup_src, ndn_src, species, step, grid_log2, nullptr, states_dst, lo_rank_src, hi_base_src, &p))
    return -1;
  const int nblk = ladder_blocks(p.n, grid_log2);
  const dim3 grid((unsigned)nblk);
  hubbard_ladder_dispatch(species, step, [&](auto sp, auto stp) {
    hipLaunchKernelGGL((k_hubbard_ladder_forms<decltype(sp)::value, decltype(stp)::value>), grid, dim3(256), 0, st, p, v1, v2,
                       scratch);
  });
  hipLaunchKernelGGL(k_hubbard_ladder_forms_reduce, dim3((unsigned)L), dim3(256), 0, st, scratch, nblk, out);
  return 0;
}

int launch_hubbard_ladder_block(int L, int nup_src, int ndn_src, int species, int step, int R, const double* c,
                                const uint64_t* states_dst, const uint32_t* lo_rank_src, const uint32_t* hi_base_src,
                                const double* X, double* Y, int grid_log2, hipStream_t st) {
  HubbardLadderParams p;
  if (!c || !hubbard_ladder_params(L, nup_src, ndn_src, species, step, grid_log2, c, states_dst, lo_rank_src, hi_base_src, &p))
    return -1;
  const dim3 grid((unsigned)ladder_blocks(p.n, grid_log2));
  hubbard_ladder_dispatch(species, step, [&](auto sp, auto stp) {
    dispatch_block_width(R, [&](auto w) {
      hipLaunchKernelGGL((k_hubbard_ladder_block<decltype(sp)::value, decltype(stp)::value, decltype(w)::value>), grid, dim3(256),
                         0, st, p, X, Y);
    });
  });
  return 0;
}

int launch_hubbard_ladder_block_dots(int L, int nup_src, int ndn_src, int species, int step, int R, const double* c,
                                     const uint64_t* states_dst, const uint32_t* lo_rank_src, const uint32_t* hi_base_src,
                                     const double* Lft, const double* X, double* out, double* scratch, int grid_log2,
                                     hipStream_t st) {
  HubbardLadderParams p;
  if (!c || !hubbard_ladder_params(L, nup_src, ndn_src, species, step, grid_log2, c, states_dst, lo_rank_src, hi_base_src, &p))
    return -1;
  const int nblk = ladder_blocks(p.n, grid_log2);
  const dim3 grid((unsigned)nblk);
  hubbard_ladder_dispatch(species, step, [&](auto sp, auto stp) {
    dispatch_block_width(R, [&](auto w) {
      hipLaunchKernelGGL((k_hubbard_ladder_block_dots<decltype(sp)::value, decltype(stp)::value, decltype(w)::value>), grid,
                         dim3(256), 0, st, p, Lft, X, scratch);
    });
  });
  hipLaunchKernelGGL(k_hubbard_ladder_forms_reduce, dim3((unsigned)R), dim3(256), 0, st, scratch, nblk, out);
  return 0;
}

}  // namespace dsea
