// dsea_hubbard_block.hip -- the Hubbard Hamiltonian of dsea_hubbard.hip applied to a BLOCK of R vectors at once, plain and with
// the tail of the basis-free block Lanczos step fused in (docs/design/28-hubbard-finite-temperature.md): the kernel
// k_spmv_hubbard_block<R, LZ> -- the family's row walk with the tail block_spmv_tail of dsea_block.h -- and its launchers.  The
// recurrence kernels and their driver are those of dsea_block_lanczos.hip.  k_cheb_hubbard_block<R, A> and
// k_cheb_hubbard_moments<R, LEFT> (docs/design/34-hubbard-chebyshev.md) hold the same row walk, statement for statement, with the
// Chebyshev tails of dsea_sector_block.hip; the finish kernel and the launch schedule of the moments are in
// dsea_block_moments.hip.
//
// One row per thread: the division r / n_dn, the two state words, the move tests, the two parities, the two table reads of every
// hop that moves a particle and the partner rows are paid once per row and hop slot for all R columns, and every gather is R
// contiguous doubles (R / 2 16-byte loads; one 8-byte load at R = 1).  The per-row arithmetic of a column is that of the
// single-vector mat-vec of dsea_hubbard.hip without a shift, in the same order -- the diagonal over the sites (U, then the fma
// with eps) and then over the bonds (fma(V_t, n_a n_b, diag)); sum = fma(+-t_t, x_up partner, sum), fma(+-t_t, x_dn partner, sum)
// per bond in list order, a hop that moves nothing included with the value 0; then fma(diag, x_r, sum) in the tail -- so column j
// of Y = H X equals the single-vector result bit for bit.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_block.h"

namespace dsea {

namespace {
#define DSEA_HBLOCK_MAX_PARAMS (2 * DSEA_LATTICE_MAX_BONDS + 2 * DSEA_SECTOR_MAX_L)
#define DSEA_HBLOCK_NO_ROW 0xFFFFFFFFu /* "this hop does not move a particle in this row" (a row is below 2^31) */

// bonds per chunk: 2 * value hop slots whose table lookups and gathers a thread keeps in flight together, at most 32 gathered
// doubles: 4 bonds as in the single-vector kernel for R <= 4, 2 bonds at R = 8
template <int R>
struct HblockChunk {
  static constexpr int value = R == 8 ? 2 : 4;
};

struct HubbardBlockParams {
  int L, nb, Llo;
  uint32_t n_dn;
  int64_t n;
  const double* c;
  const uint64_t* up_states;
  const uint32_t* up_lo;
  const uint32_t* up_hi;
  const uint64_t* dn_states;
  const uint32_t* dn_lo;
  const uint32_t* dn_hi;
  uint16_t tb[DSEA_LATTICE_MAX_BONDS];   // a | b << 8, the caller's order
};

__device__ __forceinline__ uint64_t hblock_bit(uint64_t w, uint32_t site) { return (w >> site) & 1ull; }
// the bits strictly between the two sites of the bond
__device__ __forceinline__ uint64_t hblock_between(uint32_t e) {
  const uint32_t a = e & 255u, b = e >> 8;
  const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
  return ((1ull << hi) - 1) & ~((1ull << (lo + 1)) - 1);
}
// the parity of the particles that the hop over bond mask `between` jumps: 1 for a hop amplitude of +t
__device__ __forceinline__ uint64_t hblock_parity(uint64_t w, uint64_t between) { return (uint64_t)(__popcll(w & between) & 1); }
// n_a n_b of the bond, 0 .. 4
__device__ __forceinline__ double hblock_nn(uint64_t u, uint64_t d, uint32_t e) {
  const uint32_t a = e & 255u, b = e >> 8;
  return (double)((hblock_bit(u, a) + hblock_bit(d, a)) * (hblock_bit(u, b) + hblock_bit(d, b)));
}

// the table reads of bonds k0 .. k0 + CH - 1 for the row with words (u, d): slot 2 e is the up hop of bond k0 + e, slot 2 e + 1
// its down hop.  Two table reads per hop that moves a particle, requested and NOT used here (a use next to the read would
// make the compiler wait for every hop in turn).  Returns the slots that move a particle as a bit mask; the others (and those
// past the last bond) issue no load and leave hi and lo as they are.
template <int CH>
__device__ __forceinline__ uint32_t hblock_lookups(uint32_t (&hi)[2 * CH], uint32_t (&lo)[2 * CH], uint64_t u, uint64_t d, bool have,
                                                   int k0, const HubbardBlockParams& p, const uint16_t* tb) {
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
// the partner rows of one chunk from its table reads, DSEA_HBLOCK_NO_ROW in the slots that move nothing: the up partner keeps
// rd, the down partner keeps ru
template <int CH>
__device__ __forceinline__ void hblock_rows(uint32_t (&rw)[2 * CH], uint32_t on, const uint32_t (&hi)[2 * CH],
                                            const uint32_t (&lo)[2 * CH], uint32_t ru, uint32_t rd, uint32_t n_dn) {
#pragma unroll
  for (int e = 0; e < CH; ++e) {
    rw[2 * e] = (on >> (2 * e)) & 1u ? (hi[2 * e] + lo[2 * e]) * n_dn + rd : DSEA_HBLOCK_NO_ROW;
    rw[2 * e + 1] = (on >> (2 * e + 1)) & 1u ? ru * n_dn + (hi[2 * e + 1] + lo[2 * e + 1]) : DSEA_HBLOCK_NO_ROW;
  }
}
// the gathers of one chunk: the partner's row of the block, zeros where the hop moves nothing (no load is issued)
template <int R, int HOPS>
__device__ __forceinline__ void hblock_gather(double (&xv)[HOPS][R], const uint32_t (&rw)[HOPS], const double* __restrict__ v) {
#pragma unroll
  for (int e = 0; e < HOPS; ++e) {
#pragma unroll
    for (int j = 0; j < R; ++j) xv[e][j] = 0.0;
    if (rw[e] != DSEA_HBLOCK_NO_ROW) block_load<R>(xv[e], v, (int64_t)rw[e]);
  }
}
}  // namespace

// Y = H X for the R columns of a block; LZ: the Lanczos step W = H x - y diag(st[0 .. R)) with the partials of x_j . W_j in P.
// The family's row walk, written here because this is its one kernel, then the tail block_spmv_tail: the couplings, the bond
// table and the bonds' between-masks are staged in LDS; one row per thread, the row of X and the row of Y move coalesced,
// dn_states[rd] too; up_states[ru] is one address for all lanes that share ru.  The table reads of chunk c + 1 are issued before
// the gathers of chunk c are consumed.  A block walks the row ranges blockIdx.x, + gridDim.x, ... of 256 rows.
template <int R, bool LZ>
__global__ __launch_bounds__(256) void k_spmv_hubbard_block(HubbardBlockParams p, const double* __restrict__ x, double* __restrict__ y,
                                                            const double* __restrict__ st, int first, double* __restrict__ P) {
  __shared__ double cp[DSEA_HBLOCK_MAX_PARAMS];
  __shared__ uint64_t bm[DSEA_LATTICE_MAX_BONDS];
  __shared__ uint16_t tb[DSEA_LATTICE_MAX_BONDS];
  __shared__ double sm[R][4];
  constexpr int CH = HblockChunk<R>::value;
  constexpr int HOPS = 2 * CH;
  const int L = p.L, nb = p.nb;
  const int64_t n = p.n;
  for (int c = threadIdx.x; c < 2 * nb + 2 * L; c += 256) cp[c] = p.c[c];
  for (int c = threadIdx.x; c < nb; c += 256) {
    const uint16_t e = p.tb[c];
    tb[c] = e;
    bm[c] = hblock_between(e);
  }
  __syncthreads();
  const double* __restrict__ ts = cp;
  const double* __restrict__ Vs = cp + nb;
  const double* __restrict__ Us = cp + 2 * nb;
  const double* __restrict__ es = cp + 2 * nb + L;
  double beta[R], acc[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    beta[j] = 0.0;
    acc[j] = 0.0;
    if constexpr (LZ) beta[j] = st[j];
  }
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;                       // (a thread past the last row reads row n - 1 and writes nothing)
    const uint32_t rr = (uint32_t)(have ? r : n - 1);
    const uint32_t ru = rr / p.n_dn, rd = rr - ru * p.n_dn;
    const uint64_t u = p.up_states[ru], d = p.dn_states[rd];
    double xr[R];
    block_load<R>(xr, x, (int64_t)rr);
    uint32_t hi[HOPS], lo[HOPS];
    uint32_t on = hblock_lookups<CH>(hi, lo, u, d, have, 0, p, tb);
    double diag = 0.0, sum[R];
#pragma unroll
    for (int j = 0; j < R; ++j) sum[j] = 0.0;
    const uint64_t both = u & d;
    for (int i = 0; i < L; ++i) {
      diag += hblock_bit(both, i) ? Us[i] : 0.0;
      diag = fma(es[i], (double)(hblock_bit(u, i) + hblock_bit(d, i)), diag);
    }
    for (int k0 = 0; k0 < nb; k0 += CH) {
      uint32_t rw[HOPS];
      double xv[HOPS][R];
      hblock_rows<CH>(rw, on, hi, lo, ru, rd, p.n_dn);
      hblock_gather<R, HOPS>(xv, rw, x);
      on = hblock_lookups<CH>(hi, lo, u, d, have, k0 + CH, p, tb);
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        if (k0 + e < nb) {
          const uint32_t w = tb[k0 + e];
          const uint64_t between = bm[k0 + e];
          const double tt = ts[k0 + e];
          diag = fma(Vs[k0 + e], hblock_nn(u, d, w), diag);
          // -t sgn = t (-1)^(parity + 1): the sign goes into the sign bit of the coupling
          const double tu = block_signed(tt, hblock_parity(u, between) ^ 1ull);
          const double td = block_signed(tt, hblock_parity(d, between) ^ 1ull);
#pragma unroll
          for (int j = 0; j < R; ++j) {
            sum[j] = fma(tu, xv[2 * e][j], sum[j]);
            sum[j] = fma(td, xv[2 * e + 1][j], sum[j]);
          }
        }
      }
    }
    if (have) block_spmv_tail<R, LZ>(y, first, beta, acc, r, xr, diag, sum);
  }
  if constexpr (LZ) block_partials<R>(acc, sm, P);
}

// One order of the Chebyshev recurrence of f(H) X (docs/design/34-hubbard-chebyshev.md), the Hubbard twin of
// k_cheb_sector_block<R, A>.  The row walk is that of k_spmv_hubbard_block<R, false>, statement for statement (a copy, not a
// shared function: 32-block-kernel-parts.md measured what sharing did to the existing symbols), so w = fma(diag, x_r, sum) has
// the bits of the block mat-vec.  The tail is that of the sector kernel:
//   t = g (w - centre x)                                  g = 1 / halfwidth on the first order, 2 / halfwidth afterwards
//   first:  acc_a = c0_a x + c1_a t                       (old and acc are not read)
//   else:   t = t - old,  acc_a = acc_a + c1_a t
//   out = t
// every product and sum rounded on its own.  The tail touches the thread's own row only, so old == out is allowed (neither is
// __restrict__); x and the accumulators are distinct from every other block.  old and acc are read after the last chunk's
// gathers are consumed.  No atomics, no reductions.
template <int R, int A>
__global__ __launch_bounds__(256) void k_cheb_hubbard_block(HubbardBlockParams p, const double* __restrict__ x, const double* old,
                                                            double* out, ChebAccs<A> ca, double centre, double g, int first) {
  __shared__ double cp[DSEA_HBLOCK_MAX_PARAMS];
  __shared__ uint64_t bm[DSEA_LATTICE_MAX_BONDS];
  __shared__ uint16_t tb[DSEA_LATTICE_MAX_BONDS];
  constexpr int CH = HblockChunk<R>::value;
  constexpr int HOPS = 2 * CH;
  const int L = p.L, nb = p.nb;
  const int64_t n = p.n;
  for (int c = threadIdx.x; c < 2 * nb + 2 * L; c += 256) cp[c] = p.c[c];
  for (int c = threadIdx.x; c < nb; c += 256) {
    const uint16_t e = p.tb[c];
    tb[c] = e;
    bm[c] = hblock_between(e);
  }
  __syncthreads();
  const double* __restrict__ ts = cp;
  const double* __restrict__ Vs = cp + nb;
  const double* __restrict__ Us = cp + 2 * nb;
  const double* __restrict__ es = cp + 2 * nb + L;
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;                       // (a thread past the last row reads row n - 1 and writes nothing)
    const uint32_t rr = (uint32_t)(have ? r : n - 1);
    const uint32_t ru = rr / p.n_dn, rd = rr - ru * p.n_dn;
    const uint64_t u = p.up_states[ru], d = p.dn_states[rd];
    double xr[R];
    block_load<R>(xr, x, (int64_t)rr);
    uint32_t hi[HOPS], lo[HOPS];
    uint32_t on = hblock_lookups<CH>(hi, lo, u, d, have, 0, p, tb);
    double diag = 0.0, sum[R];
#pragma unroll
    for (int j = 0; j < R; ++j) sum[j] = 0.0;
    const uint64_t both = u & d;
    for (int i = 0; i < L; ++i) {
      diag += hblock_bit(both, i) ? Us[i] : 0.0;
      diag = fma(es[i], (double)(hblock_bit(u, i) + hblock_bit(d, i)), diag);
    }
    for (int k0 = 0; k0 < nb; k0 += CH) {
      uint32_t rw[HOPS];
      double xv[HOPS][R];
      hblock_rows<CH>(rw, on, hi, lo, ru, rd, p.n_dn);
      hblock_gather<R, HOPS>(xv, rw, x);
      on = hblock_lookups<CH>(hi, lo, u, d, have, k0 + CH, p, tb);
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        if (k0 + e < nb) {
          const uint32_t w = tb[k0 + e];
          const uint64_t between = bm[k0 + e];
          const double tt = ts[k0 + e];
          diag = fma(Vs[k0 + e], hblock_nn(u, d, w), diag);
          // -t sgn = t (-1)^(parity + 1): the sign goes into the sign bit of the coupling
          const double tu = block_signed(tt, hblock_parity(u, between) ^ 1ull);
          const double td = block_signed(tt, hblock_parity(d, between) ^ 1ull);
#pragma unroll
          for (int j = 0; j < R; ++j) {
            sum[j] = fma(tu, xv[2 * e][j], sum[j]);
            sum[j] = fma(td, xv[2 * e + 1][j], sum[j]);
          }
        }
      }
    }
    if (have) {
      double t[R];
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const double w = fma(diag, xr[j], sum[j]);
        t[j] = __dmul_rn(g, __dsub_rn(w, __dmul_rn(centre, xr[j])));
      }
      if (!first) {
        double ov[R];
        block_load<R>(ov, old, r);
#pragma unroll
        for (int j = 0; j < R; ++j) t[j] = __dsub_rn(t[j], ov[j]);
      }
#pragma unroll
      for (int a = 0; a < A; ++a) {
        double av[R];
        if (first) {
#pragma unroll
          for (int j = 0; j < R; ++j) av[j] = __dadd_rn(__dmul_rn(ca.c0[a], xr[j]), __dmul_rn(ca.c1[a], t[j]));
        } else {
          block_load<R>(av, ca.acc[a], r);
#pragma unroll
          for (int j = 0; j < R; ++j) av[j] = __dadd_rn(av[j], __dmul_rn(ca.c1[a], t[j]));
        }
        block_store<R>(ca.acc[a], r, av);
      }
      block_store<R>(out, r, t);
    }
  }
}

// One order of the Chebyshev recurrence WITH the two reductions of the moments, the Hubbard twin of k_cheb_sector_moments<R,
// LEFT>: the same row walk once more, the recurrence part of the tail above without the accumulator block,
//   t = g (w - centre x),  !first: t = t - old,  out = t
//   LEFT = false:  a_j += x_j x_j,  b_j += x_j t_j          LEFT = true:  a_j += y_j x_j,  b_j += y_j t_j
// by fma into the thread's accumulators; y is the row of the left block, read after the last chunk's gathers are consumed like
// old.  A thread without a row adds nothing.  After the row loop the block's partials go to P[(which R + j) gridDim.x + block],
// which = 0 for a, 1 for b, through one LDS array each (33-chebyshev-moments.md: one array for both would race): no atomics.
// old == out is allowed; x and y are distinct from every written block.
template <int R, bool LEFT>
__global__ __launch_bounds__(256) void k_cheb_hubbard_moments(HubbardBlockParams p, const double* __restrict__ x, const double* old,
                                                              double* out, const double* __restrict__ y, double centre, double g,
                                                              int first, double* __restrict__ P) {
  __shared__ double cp[DSEA_HBLOCK_MAX_PARAMS];
  __shared__ uint64_t bm[DSEA_LATTICE_MAX_BONDS];
  __shared__ uint16_t tb[DSEA_LATTICE_MAX_BONDS];
  __shared__ double sma[R][4];
  __shared__ double smb[R][4];
  constexpr int CH = HblockChunk<R>::value;
  constexpr int HOPS = 2 * CH;
  const int L = p.L, nb = p.nb;
  const int64_t n = p.n;
  for (int c = threadIdx.x; c < 2 * nb + 2 * L; c += 256) cp[c] = p.c[c];
  for (int c = threadIdx.x; c < nb; c += 256) {
    const uint16_t e = p.tb[c];
    tb[c] = e;
    bm[c] = hblock_between(e);
  }
  __syncthreads();
  const double* __restrict__ ts = cp;
  const double* __restrict__ Vs = cp + nb;
  const double* __restrict__ Us = cp + 2 * nb;
  const double* __restrict__ es = cp + 2 * nb + L;
  double acca[R], accb[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    acca[j] = 0.0;
    accb[j] = 0.0;
  }
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;                       // (a thread past the last row reads row n - 1 and writes nothing)
    const uint32_t rr = (uint32_t)(have ? r : n - 1);
    const uint32_t ru = rr / p.n_dn, rd = rr - ru * p.n_dn;
    const uint64_t u = p.up_states[ru], d = p.dn_states[rd];
    double xr[R];
    block_load<R>(xr, x, (int64_t)rr);
    uint32_t hi[HOPS], lo[HOPS];
    uint32_t on = hblock_lookups<CH>(hi, lo, u, d, have, 0, p, tb);
    double diag = 0.0, sum[R];
#pragma unroll
    for (int j = 0; j < R; ++j) sum[j] = 0.0;
    const uint64_t both = u & d;
    for (int i = 0; i < L; ++i) {
      diag += hblock_bit(both, i) ? Us[i] : 0.0;
      diag = fma(es[i], (double)(hblock_bit(u, i) + hblock_bit(d, i)), diag);
    }
    for (int k0 = 0; k0 < nb; k0 += CH) {
      uint32_t rw[HOPS];
      double xv[HOPS][R];
      hblock_rows<CH>(rw, on, hi, lo, ru, rd, p.n_dn);
      hblock_gather<R, HOPS>(xv, rw, x);
      on = hblock_lookups<CH>(hi, lo, u, d, have, k0 + CH, p, tb);
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        if (k0 + e < nb) {
          const uint32_t w = tb[k0 + e];
          const uint64_t between = bm[k0 + e];
          const double tt = ts[k0 + e];
          diag = fma(Vs[k0 + e], hblock_nn(u, d, w), diag);
          // -t sgn = t (-1)^(parity + 1): the sign goes into the sign bit of the coupling
          const double tu = block_signed(tt, hblock_parity(u, between) ^ 1ull);
          const double td = block_signed(tt, hblock_parity(d, between) ^ 1ull);
#pragma unroll
          for (int j = 0; j < R; ++j) {
            sum[j] = fma(tu, xv[2 * e][j], sum[j]);
            sum[j] = fma(td, xv[2 * e + 1][j], sum[j]);
          }
        }
      }
    }
    if (have) {
      double t[R];
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const double w = fma(diag, xr[j], sum[j]);
        t[j] = __dmul_rn(g, __dsub_rn(w, __dmul_rn(centre, xr[j])));
      }
      if (!first) {
        double ov[R];
        block_load<R>(ov, old, r);
#pragma unroll
        for (int j = 0; j < R; ++j) t[j] = __dsub_rn(t[j], ov[j]);
      }
      block_store<R>(out, r, t);
      if constexpr (LEFT) {
        double yv[R];
        block_load<R>(yv, y, r);
#pragma unroll
        for (int j = 0; j < R; ++j) {
          acca[j] = fma(yv[j], xr[j], acca[j]);
          accb[j] = fma(yv[j], t[j], accb[j]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < R; ++j) {
          acca[j] = fma(xr[j], xr[j], acca[j]);
          accb[j] = fma(xr[j], t[j], accb[j]);
        }
      }
    }
  }
  block_partials<R>(acca, sma, P);
  block_partials<R>(accb, smb, P + (int64_t)R * gridDim.x);
}

// the kernel arguments; false when the descriptor is out of range
static bool hubbard_block_params(const OpDesc& op, HubbardBlockParams* p) {
  const HubbardDesc& d = op.hubbard;
  int64_t n, n_up, n_dn;
  if (!hubbard_sizes(d.L, d.nup, d.ndn, &n, &n_up, &n_dn) || n != op.n || d.nb < 1 || d.nb > DSEA_LATTICE_MAX_BONDS) return false;
  if (op.tune_tile_log2 < 6 || op.tune_tile_log2 > 12 || !d.c) return false;
  if (!d.up_states || !d.up_lo || !d.up_hi || !d.dn_states || !d.dn_lo || !d.dn_hi) return false;
  for (int t = 0; t < d.nb; ++t)
    if (d.a[t] >= d.L || d.b[t] >= d.L || d.a[t] == d.b[t]) return false;
  p->L = d.L;
  p->nb = d.nb;
  p->Llo = (d.L + 1) / 2;
  p->n_dn = (uint32_t)n_dn;
  p->n = n;
  p->c = d.c;
  p->up_states = d.up_states;
  p->up_lo = d.up_lo;
  p->up_hi = d.up_hi;
  p->dn_states = d.dn_states;
  p->dn_lo = d.dn_lo;
  p->dn_hi = d.dn_hi;
  block_pack_bonds(p->tb, d.a, d.b, d.nb);
  return true;
}

int launch_hubbard_block_apply(const OpDesc& op, int R, const double* X, double* Y, hipStream_t st) {
  HubbardBlockParams p;
  if (!hubbard_block_params(op, &p)) return -1;
  const int nblk = block_blocks(op);
  dispatch_block_width(R, [&](auto r) {
    klaunch(nullptr, k_spmv_hubbard_block<decltype(r)::value, false>, nblk, 256, 0, st, p, X, Y, nullptr, 1, nullptr);
  });
  return nblk;
}

// ACC[a] = sum_{m < M} coeffs[a * M + m] T_m((H - centre) / halfwidth) X in M - 1 launches of k_cheb_hubbard_block, on the
// schedule of launch_sector_block_chebyshev: order 1 is `first` with x = X and out = U; order 2 reads x = U, old = X and writes
// V; from order 3 on old == out, U and V in turn.  The two coefficients of an order go into its launch by value from the host
// array.  Nothing is read back, no synchronise.
int launch_hubbard_block_chebyshev(const OpDesc& op, int R, int A, int M, double centre, double halfwidth, const double* coeffs,
                                   const double* X, double* U, double* V, double* ACC, hipStream_t st) {
  HubbardBlockParams p;
  if (!hubbard_block_params(op, &p)) return -1;
  const int nblk = block_blocks(op);
  dispatch_block_width(R, [&](auto r) {
    dispatch_int<1, 2>(A, [&](auto na) {
      constexpr int RR = decltype(r)::value, AA = decltype(na)::value;
      ChebAccs<AA> ca;
      for (int a = 0; a < AA; ++a) {
        ca.acc[a] = ACC + (int64_t)a * op.n * RR;
        ca.c0[a] = coeffs[(int64_t)a * M];
      }
      double* const t[2] = {U, V};                 // T_m lives in t[(m - 1) & 1]
      for (int m = 1; m < M; ++m) {
        for (int a = 0; a < AA; ++a) ca.c1[a] = coeffs[(int64_t)a * M + m];
        const double* x = m == 1 ? X : t[m & 1];
        const double* old = m == 2 ? X : t[(m - 1) & 1];
        klaunch(nullptr, k_cheb_hubbard_block<RR, AA>, nblk, 256, 0, st, p, x, old, t[(m - 1) & 1], ca, centre,
                (m == 1 ? 1.0 : 2.0) / halfwidth, m == 1 ? 1 : 0);
      }
    });
  });
  return nblk;
}

// the schedule of block_moments_drive with this file's moments kernel as the step; Y null: self mode
int launch_hubbard_block_moments(const OpDesc& op, int R, int M, double centre, double halfwidth, const double* X, const double* Y,
                                 double* U, double* V, double* MU, double* scratch, hipStream_t st) {
  HubbardBlockParams p;
  if (!hubbard_block_params(op, &p)) return -1;
  const int nblk = block_blocks(op);
  return block_moments_drive(op.n, nblk, R, M, Y != nullptr, X, U, V, MU, scratch, st,
                             [&](const double* x, const double* old, double* out, int first, double* P) {
                               dispatch_block_width(R, [&](auto r) {
                                 dispatch_bool(Y != nullptr, [&](auto left) {
                                   klaunch(nullptr, k_cheb_hubbard_moments<decltype(r)::value, decltype(left)::value>, nblk, 256, 0,
                                           st, p, x, old, out, Y, centre, (first ? 1.0 : 2.0) / halfwidth, first, P);
                                 });
                               });
                             });
}

// the recurrence of block_lanczos_drive with this file's mat-vec as the step
int launch_hubbard_block_lanczos(const OpDesc& op, int R, int k, double* Q, double* W, double* norm2, double* alphas, double* betas,
                                 int32_t* steps, double* scratch, hipStream_t st) {
  HubbardBlockParams p;
  if (!hubbard_block_params(op, &p)) return -1;
  const int nblk = block_blocks(op);
  return block_lanczos_drive(op.n, nblk, R, k, Q, W, norm2, alphas, betas, steps, scratch, st,
                             [&](const double* q, double* w, const double* state, int first, double* PA) {
                               dispatch_block_width(R, [&](auto r) {
                                 klaunch(nullptr, k_spmv_hubbard_block<decltype(r)::value, true>, nblk, 256, 0, st, p, q, w, state,
                                         first, PA);
                               });
                             });
}

}  // namespace dsea
