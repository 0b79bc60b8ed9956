// dsea_hubbard_current.hip -- the bond current map of the Hubbard sector of dsea_hubbard.hip (docs/design/39-hubbard-current.md):
// the kernel k_hubbard_current<R>, the parameter adjoint k_hubbard_current_forms (+ k_hubbard_current_forms_reduce), the column
// dots k_hubbard_current_block_dots<R> (docs/design/40-finite-temperature-conductivity.md), and their launchers.
//
//   K(w) = sum_t sum_s w_{s t} (c+_{a s} c_{b s} - c+_{b s} c_{a s}),   (a, b) = bond t in the caller's orientation,   J = i K(w)
// real and antisymmetric on the sector (L, nup, ndn) of the operator, in its state order and on its tables.  With the notation
// of dsea_hubbard.hip (m_t, B_t, sgn_t) and o_t(w) = +1 if bit a_t of the word w is set, else -1:
//   (K x)[r] = sum_{t : bit_a(u) != bit_b(u)} w_{up t} o_t(u) sgn_t(u) x[rank_u(u ^ m_t) n_dn + rd]
//            + sum_{t : bit_a(d) != bit_b(d)} w_{dn t} o_t(d) sgn_t(d) x[ru n_dn + rank_d(d ^ m_t)]
// No diagonal, no shift; reversing a bond's orientation flips its sign; a repeated bond counts each time.  The weights are one
// device array [w_up(nb), w_dn(nb)], copied into LDS by every block on every launch.
//
// The row walk is the hop walk of k_spmv_hubbard_block (dsea_hubbard_block.hip) without the row of x and without the diagonal:
// one row per thread, the table reads of chunk c + 1 issued before the gathers of chunk c are consumed, chunks of HcurChunk<R>
// bonds.  The few helpers of that walk are written again here: those of dsea_hubbard_block.hip live in its anonymous namespace,
// and moving them would have to leave every existing symbol byte for byte.  Each product is exact -- the signs go into the sign
// bit of the weight -- and the fma chain of a column runs over the bonds in list order whatever the chunk, so column j of
// Y = K X is the same bits at every R.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_block.h"

namespace dsea {

namespace {
#define DSEA_HCUR_NO_ROW 0xFFFFFFFFu /* "this hop does not move a particle in this row" (a row is below 2^31) */

// bonds per chunk, as HblockChunk<R>: at most 32 gathered doubles in flight per thread
template <int R>
struct HcurChunk {
  static constexpr int value = R == 8 ? 2 : 4;
};

struct HubbardCurrentParams {
  int L, nb, Llo;
  uint32_t n_dn;
  int64_t n;
  const double* w;                       // [w_up(nb), w_dn(nb)]; null for the forms
  const uint64_t* up_states;
  const uint32_t* up_lo;
  const uint32_t* up_hi;
  const uint64_t* dn_states;
  const uint32_t* dn_lo;
  const uint32_t* dn_hi;
  uint16_t tb[DSEA_LATTICE_MAX_BONDS];   // a | b << 8, the caller's order
};

// the bits strictly between the two sites of the bond
__device__ __forceinline__ uint64_t hcur_between(uint32_t e) {
  const uint32_t a = e & 255u, b = e >> 8;
  const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
  return ((1ull << hi) - 1) & ~((1ull << (lo + 1)) - 1);
}
// the sign bit of o_t(w) sgn_t(w): the parity of the particles the hop jumps, xor "bit a of w is clear"
__device__ __forceinline__ uint64_t hcur_negative(uint64_t w, uint32_t e, uint64_t between) {
  return ((uint64_t)__popcll(w & between) ^ (w >> (e & 255u)) ^ 1ull) & 1ull;
}
// the bond table and the between-masks of a block, in LDS
__device__ __forceinline__ void hcur_stage_bonds(const HubbardCurrentParams& p, uint16_t* tb, uint64_t* bm) {
  for (int c = threadIdx.x; c < p.nb; c += 256) {
    const uint16_t e = p.tb[c];
    tb[c] = e;
    bm[c] = hcur_between(e);
  }
}

// the table reads of bonds k0 .. k0 + CH - 1 for the row with words (u, d): slot 2 e is the up hop of bond k0 + e, slot 2 e + 1
// its down hop.  Two table reads per hop that moves a particle, requested and NOT used here.  Returns the slots that move a
// particle as a bit mask; the others (and those past the last bond) issue no load and leave hi and lo as they are.
template <int CH>
__device__ __forceinline__ uint32_t hcur_lookups(uint32_t (&hi)[2 * CH], uint32_t (&lo)[2 * CH], uint64_t u, uint64_t d, bool have,
                                                 int k0, const HubbardCurrentParams& p, const uint16_t* tb) {
  const int Llo = p.Llo;
  const uint64_t lomask = (1ull << Llo) - 1;
  const uint32_t* __restrict__ up_lo = p.up_lo;
  const uint32_t* __restrict__ up_hi = p.up_hi;
  const uint32_t* __restrict__ dn_lo = p.dn_lo;
  const uint32_t* __restrict__ dn_hi = p.dn_hi;
  uint32_t on = 0;
#pragma unroll
  for (int e = 0; e < CH; ++e) {
    const bool in = have && k0 + e < p.nb;
    const uint32_t w = k0 + e < p.nb ? tb[k0 + e] : 0u;
    const uint64_t m = block_mask(w);
    const uint64_t u2 = u ^ m, d2 = d ^ m;
    if (in && block_differ(u, w) != 0) {
      hi[2 * e] = up_hi[u2 >> Llo];
      lo[2 * e] = up_lo[u2 & lomask];
      on |= 1u << (2 * e);
    }
    if (in && block_differ(d, w) != 0) {
      hi[2 * e + 1] = dn_hi[d2 >> Llo];
      lo[2 * e + 1] = dn_lo[d2 & lomask];
      on |= 2u << (2 * e);
    }
  }
  return on;
}
// the partner rows of one chunk from its table reads, DSEA_HCUR_NO_ROW in the slots that move nothing: the up partner keeps rd,
// the down partner keeps ru
template <int CH>
__device__ __forceinline__ void hcur_rows(uint32_t (&rw)[2 * CH], uint32_t on, const uint32_t (&hi)[2 * CH],
                                          const uint32_t (&lo)[2 * CH], uint32_t ru, uint32_t rd, uint32_t n_dn) {
#pragma unroll
  for (int e = 0; e < CH; ++e) {
    rw[2 * e] = (on >> (2 * e)) & 1u ? (hi[2 * e] + lo[2 * e]) * n_dn + rd : DSEA_HCUR_NO_ROW;
    rw[2 * e + 1] = (on >> (2 * e + 1)) & 1u ? ru * n_dn + (hi[2 * e + 1] + lo[2 * e + 1]) : DSEA_HCUR_NO_ROW;
  }
}
// the gathers of one chunk: the partner's row of the block, zeros where the hop moves nothing (no load is issued)
template <int R, int HOPS>
__device__ __forceinline__ void hcur_gather(double (&xv)[HOPS][R], const uint32_t (&rw)[HOPS], const double* __restrict__ v) {
#pragma unroll
  for (int e = 0; e < HOPS; ++e) {
#pragma unroll
    for (int j = 0; j < R; ++j) xv[e][j] = 0.0;
    if (rw[e] != DSEA_HCUR_NO_ROW) block_load<R>(xv[e], v, (int64_t)rw[e]);
  }
}
}  // namespace

// Y = K(w) X for the R columns of a block.  The weights, the bond table and the bonds' between-masks are staged in LDS; one row
// per thread, the row of Y moves coalesced, dn_states[rd] too; up_states[ru] is one address for all lanes that share ru.  Per
// bond in list order sum = fma(+-w_up, x_up partner, sum), fma(+-w_dn, x_dn partner, sum), a hop that moves nothing included with
// the value 0.  A block walks the row ranges blockIdx.x, + gridDim.x, ... of 256 rows.
template <int R>
__global__ __launch_bounds__(256) void k_hubbard_current(HubbardCurrentParams p, const double* __restrict__ x, double* __restrict__ y) {
  __shared__ double wp[2 * DSEA_LATTICE_MAX_BONDS];
  __shared__ uint64_t bm[DSEA_LATTICE_MAX_BONDS];
  __shared__ uint16_t tb[DSEA_LATTICE_MAX_BONDS];
  constexpr int CH = HcurChunk<R>::value;
  constexpr int HOPS = 2 * CH;
  const int nb = p.nb;
  const int64_t n = p.n;
  for (int c = threadIdx.x; c < 2 * nb; c += 256) wp[c] = p.w[c];
  hcur_stage_bonds(p, tb, bm);
  __syncthreads();
  const double* __restrict__ wu = wp;
  const double* __restrict__ wd = wp + nb;
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;                       // (a thread past the last row reads row n - 1 and writes nothing)
    const uint32_t rr = (uint32_t)(have ? r : n - 1);
    const uint32_t ru = rr / p.n_dn, rd = rr - ru * p.n_dn;
    const uint64_t u = p.up_states[ru], d = p.dn_states[rd];
    uint32_t hi[HOPS], lo[HOPS];
    uint32_t on = hcur_lookups<CH>(hi, lo, u, d, have, 0, p, tb);
    double sum[R];
#pragma unroll
    for (int j = 0; j < R; ++j) sum[j] = 0.0;
    for (int k0 = 0; k0 < nb; k0 += CH) {
      uint32_t rw[HOPS];
      double xv[HOPS][R];
      hcur_rows<CH>(rw, on, hi, lo, ru, rd, p.n_dn);
      hcur_gather<R, HOPS>(xv, rw, x);
      on = hcur_lookups<CH>(hi, lo, u, d, have, k0 + CH, p, tb);
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        if (k0 + e < nb) {
          const uint32_t w = tb[k0 + e];
          const uint64_t between = bm[k0 + e];
          // w o sgn: parity ^ (o < 0) goes into the sign bit of the weight
          const double tu = block_signed(wu[k0 + e], hcur_negative(u, w, between));
          const double td = block_signed(wd[k0 + e], hcur_negative(d, w, between));
#pragma unroll
          for (int j = 0; j < R; ++j) {
            sum[j] = fma(tu, xv[2 * e][j], sum[j]);
            sum[j] = fma(td, xv[2 * e + 1][j], sum[j]);
          }
        }
      }
    }
    if (have) block_store<R>(y, r, sum);
  }
}

// The column dots d[j] = sum_r Lft[r, j] (K(w) X)[r, j] without the product block (docs/design/40-finite-temperature-conductivity.md):
// the row walk of k_hubbard_current<R>, written again here so that kernel keeps its instructions -- the same staging, chunks,
// look-ahead and fma chain, so sum[j] is the bits that kernel stores.  The row of Lft is read after the last chunk's gathers are
// consumed; one accumulator per column and thread over the row ranges the block walks (a thread without a row adds nothing), then
// block_partials into scratch[j * gridDim.x + block].  k_hubbard_current_forms_reduce with R blocks closes them.  No atomics.
template <int R>
__global__ __launch_bounds__(256) void k_hubbard_current_block_dots(HubbardCurrentParams p, const double* __restrict__ Lft,
                                                                    const double* __restrict__ x, double* __restrict__ scratch) {
  __shared__ double wp[2 * DSEA_LATTICE_MAX_BONDS];
  __shared__ uint64_t bm[DSEA_LATTICE_MAX_BONDS];
  __shared__ uint16_t tb[DSEA_LATTICE_MAX_BONDS];
  __shared__ double sm[R][4];
  constexpr int CH = HcurChunk<R>::value;
  constexpr int HOPS = 2 * CH;
  const int nb = p.nb;
  const int64_t n = p.n;
  for (int c = threadIdx.x; c < 2 * nb; c += 256) wp[c] = p.w[c];
  hcur_stage_bonds(p, tb, bm);
  __syncthreads();
  const double* __restrict__ wu = wp;
  const double* __restrict__ wd = wp + nb;
  double acc[R];
#pragma unroll
  for (int j = 0; j < R; ++j) acc[j] = 0.0;
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;                       // (a thread past the last row reads row n - 1 and adds nothing)
    const uint32_t rr = (uint32_t)(have ? r : n - 1);
    const uint32_t ru = rr / p.n_dn, rd = rr - ru * p.n_dn;
    const uint64_t u = p.up_states[ru], d = p.dn_states[rd];
    uint32_t hi[HOPS], lo[HOPS];
    uint32_t on = hcur_lookups<CH>(hi, lo, u, d, have, 0, p, tb);
    double sum[R];
#pragma unroll
    for (int j = 0; j < R; ++j) sum[j] = 0.0;
    for (int k0 = 0; k0 < nb; k0 += CH) {
      uint32_t rw[HOPS];
      double xv[HOPS][R];
      hcur_rows<CH>(rw, on, hi, lo, ru, rd, p.n_dn);
      hcur_gather<R, HOPS>(xv, rw, x);
      on = hcur_lookups<CH>(hi, lo, u, d, have, k0 + CH, p, tb);
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        if (k0 + e < nb) {
          const uint32_t w = tb[k0 + e];
          const uint64_t between = bm[k0 + e];
          const double tu = block_signed(wu[k0 + e], hcur_negative(u, w, between));
          const double td = block_signed(wd[k0 + e], hcur_negative(d, w, between));
#pragma unroll
          for (int j = 0; j < R; ++j) {
            sum[j] = fma(tu, xv[2 * e][j], sum[j]);
            sum[j] = fma(td, xv[2 * e + 1][j], sum[j]);
          }
        }
      }
    }
    if (have) {
      double l[R];
      block_load<R>(l, Lft, r);
#pragma unroll
      for (int j = 0; j < R; ++j) acc[j] = fma(l[j], sum[j], acc[j]);
    }
  }
  block_partials<R>(acc, sm, scratch);
}

// The parameter adjoint: out[s nb + t] = v1^T K_{s t} v2 for all 2 nb unit-weight bond maps (s = 0 up, 1 dn) in one pass over v1
// and v2:
//   up, t: sum_r v1[r] o_t(u) sgn_t(u) v2[up partner]          dn, t: sum_r v1[r] o_t(d) sgn_t(d) v2[dn partner]
// Same row walk and the same chunks of lookups and gathers (of v2) as the map at R = 1.  No per-lane accumulator per term: every
// term is reduced through the wave at once (wave_sum, fixed order) and lane 0 adds it to the wave's row of LDS accumulators; the
// four rows are added in fixed order and written to scratch[term * gridDim.x + block].  No atomics.
__global__ __launch_bounds__(256) void k_hubbard_current_forms(HubbardCurrentParams p, const double* __restrict__ v1,
                                                               const double* __restrict__ v2, double* __restrict__ scratch) {
  __shared__ double accs[4][2 * DSEA_LATTICE_MAX_BONDS];
  __shared__ uint64_t bm[DSEA_LATTICE_MAX_BONDS];
  __shared__ uint16_t tb[DSEA_LATTICE_MAX_BONDS];
  constexpr int CH = HcurChunk<1>::value;
  constexpr int HOPS = 2 * CH;
  const int nb = p.nb;
  const int nterm = 2 * nb;
  const int64_t n = p.n;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double* __restrict__ mine = accs[wv];
  for (int c = lane; c < nterm; c += 64) mine[c] = 0.0;   // (afterwards a wave's row is touched by its lane 0 alone)
  hcur_stage_bonds(p, tb, bm);
  __syncthreads();
  auto add = [&](int term, double val) {
    const double tot = wave_sum(val);
    if (lane == 0) mine[term] += tot;
  };
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;                       // a thread without a row adds zeros to every form
    const uint32_t rr = (uint32_t)(have ? r : n - 1);
    const uint32_t ru = rr / p.n_dn, rd = rr - ru * p.n_dn;
    const uint64_t u = p.up_states[ru], d = p.dn_states[rd];
    const double a = have ? v1[rr] : 0.0;
    uint32_t hi[HOPS], lo[HOPS];
    uint32_t on = hcur_lookups<CH>(hi, lo, u, d, have, 0, p, tb);
    for (int k0 = 0; k0 < nb; k0 += CH) {
      uint32_t rw[HOPS];
      double xv[HOPS][1];
      hcur_rows<CH>(rw, on, hi, lo, ru, rd, p.n_dn);
      hcur_gather<1, HOPS>(xv, rw, v2);
      on = hcur_lookups<CH>(hi, lo, u, d, have, k0 + CH, p, tb);
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        if (k0 + e < nb) {                         // (the same for every lane: the wave sums run with all lanes)
          const uint32_t w = tb[k0 + e];
          const uint64_t between = bm[k0 + e];
          add(k0 + e, a * block_signed(xv[2 * e][0], hcur_negative(u, w, between)));
          add(nb + k0 + e, a * block_signed(xv[2 * e + 1][0], hcur_negative(d, w, between)));
        }
      }
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < nterm; c += 256)
    scratch[(int64_t)c * gridDim.x + blockIdx.x] = ((accs[0][c] + accs[1][c]) + accs[2][c]) + accs[3][c];
}

// second stage: out[term] = the sum of the term's per-block partials, fixed order; one block per form
__global__ __launch_bounds__(256) void k_hubbard_current_forms_reduce(const double* __restrict__ scratch, int count,
                                                                      double* __restrict__ out) {
  __shared__ double sm5[5];
  const double tot = sum_partials_block(scratch + (int64_t)blockIdx.x * count, count, sm5);
  if (threadIdx.x == 0) out[blockIdx.x] = tot;
}

// the kernel arguments from the operator's descriptor (its sector, tables and bonds; not its couplings); false when the
// descriptor is out of range
static bool hubbard_current_params(const OpDesc& op, const double* w, HubbardCurrentParams* p) {
  const HubbardDesc& d = op.hubbard;
  int64_t n, n_up, n_dn;
  if (!hubbard_sizes(d.L, d.nup, d.ndn, &n, &n_up, &n_dn) || n != op.n || d.nb < 1 || d.nb > DSEA_LATTICE_MAX_BONDS) return false;
  if (op.tune_tile_log2 < 6 || op.tune_tile_log2 > 12) return false;
  if (!d.up_states || !d.up_lo || !d.up_hi || !d.dn_states || !d.dn_lo || !d.dn_hi) return false;
  for (int t = 0; t < d.nb; ++t)
    if (d.a[t] >= d.L || d.b[t] >= d.L || d.a[t] == d.b[t]) return false;
  p->L = d.L;
  p->nb = d.nb;
  p->Llo = (d.L + 1) / 2;
  p->n_dn = (uint32_t)n_dn;
  p->n = n;
  p->w = w;
  p->up_states = d.up_states;
  p->up_lo = d.up_lo;
  p->up_hi = d.up_hi;
  p->dn_states = d.dn_states;
  p->dn_lo = d.dn_lo;
  p->dn_hi = d.dn_hi;
  block_pack_bonds(p->tb, d.a, d.b, d.nb);
  return true;
}

int launch_hubbard_current(const OpDesc& op, int R, const double* w, const double* X, double* Y, hipStream_t st) {
  HubbardCurrentParams p;
  if (!w || !hubbard_current_params(op, w, &p)) return -1;
  const int nblk = block_blocks(op);
  dispatch_block_width(R, [&](auto r) { klaunch(nullptr, k_hubbard_current<decltype(r)::value>, nblk, 256, 0, st, p, X, Y); });
  return nblk;
}

// block_blocks(op) partials per form: at most ladder_partials(n, 2 nb) doubles of scratch at any grid cap
int launch_hubbard_current_forms(const OpDesc& op, const double* v1, const double* v2, double* out, double* scratch, hipStream_t st) {
  HubbardCurrentParams p;
  if (!hubbard_current_params(op, nullptr, &p)) return -1;
  const int nblk = block_blocks(op);
  klaunch(nullptr, k_hubbard_current_forms, nblk, 256, 0, st, p, v1, v2, scratch);
  klaunch(nullptr, k_hubbard_current_forms_reduce, 2 * p.nb, 256, 0, st, scratch, nblk, out);
  return 0;
}

// block_blocks(op) partials per column: at most ladder_partials(n, R) doubles of scratch at any grid cap; the caller has checked R
int launch_hubbard_current_block_dots(const OpDesc& op, int R, const double* w, const double* Lft, const double* X, double* out,
                                      double* scratch, hipStream_t st) {
  HubbardCurrentParams p;
  if (!w || !hubbard_current_params(op, w, &p)) return -1;
  const int nblk = block_blocks(op);
  dispatch_block_width(R, [&](auto r) {
    klaunch(nullptr, k_hubbard_current_block_dots<decltype(r)::value>, nblk, 256, 0, st, p, Lft, X, scratch);
  });
  klaunch(nullptr, k_hubbard_current_forms_reduce, R, 256, 0, st, scratch, nblk, out);
  return 0;
}

}  // namespace dsea
