// dsea_sector_block.hip -- the bond-list sector Hamiltonian of dsea_sector.hip applied to a BLOCK of R vectors at once
// (docs/design/27-finite-temperature.md, 31-chebyshev-propagator.md): k_spmv_sector_block<R, LZ>, k_cheb_sector_block<R, A> and
// their launchers, on the block parts of dsea_block.h.  The block Lanczos recurrence that runs around the LZ kernel is in
// dsea_block_lanczos.hip.  The two kernels hold the same row walk, statement for statement: written once, as a function called
// by both or as a walker that takes the tail, the R = 8 kernels ran 0.5 to 1.4 % slower (docs/design/32-block-kernel-parts.md).
// k_cheb_sector_moments<R, LEFT> (docs/design/33-chebyshev-moments.md) is a third holder of that walk: the Chebyshev order with
// the two dot products of the moments; its finish kernel and launch schedule are in dsea_block_moments.hip.
//
// One row per thread: the row's state word and the two table reads of a flipped bond are paid once for all R columns, and every
// gather is R contiguous doubles (R / 2 16-byte loads; one 8-byte load at R = 1).  The per-row arithmetic of a column is that of
// the single-vector mat-vec of dsea_sector.hip in the same order -- the diagonal accumulated over the sites and then the bonds,
// sum = fma(2 Jxy_t, x_partner, sum) over the bonds in list order, then fma(diag, x_r, sum) -- so column j of Y = H X equals the
// single-vector result bit for bit.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_block.h"

namespace dsea {

namespace {
#define DSEA_SBLOCK_MAX_PARAMS (2 * DSEA_LATTICE_MAX_BONDS + DSEA_SECTOR_MAX_L)
#define DSEA_SBLOCK_NO_RANK 0xFFFFFFFFu /* "this bond does not flip this row" (a rank is below 2^31) */

// bonds whose table lookups and gathers a thread keeps in flight together: 8 as in the single-vector kernel while a chunk's
// gathers fit 32 doubles per thread, 4 at R = 8
template <int R>
struct SblockChunk {
  static constexpr int value = R == 8 ? 4 : 8;
};

struct SectorBlockParams {
  int L, nb, Llo;
  int64_t n;
  const double* c;
  const uint64_t* states;
  const uint32_t* lo_rank;
  const uint32_t* hi_base;
  uint16_t tb[DSEA_LATTICE_MAX_BONDS];   // a | b << 8, the caller's order
};

// the two table values of the partner rows of bonds k0 .. k0 + CH - 1 for the row with state s: two table reads per bond that
// flips the row, all requested before any is used -- the predicated block holds the loads alone, so that the chunk waits once
// and not once per bond.  A bond that does not flip the row (and one past the last bond) gets hi = DSEA_SBLOCK_NO_RANK, lo = 0,
// so that the rank hi + lo, formed outside, is DSEA_SBLOCK_NO_RANK for it.
template <int CH>
__device__ __forceinline__ void sblock_ranks(uint32_t (&hi)[CH], uint32_t (&lo)[CH], uint64_t s, bool have, int k0, int nb, int Llo,
                                             const uint16_t* tb, const uint32_t* __restrict__ lo_rank,
                                             const uint32_t* __restrict__ hi_base) {
  const uint64_t lomask = (1ull << Llo) - 1;
#pragma unroll
  for (int e = 0; e < CH; ++e) {
    const uint32_t w = k0 + e < nb ? tb[k0 + e] : 0u;
    const bool on = have && k0 + e < nb && block_differ(s, w) != 0;
    const uint64_t s2 = s ^ block_mask(w);
    hi[e] = DSEA_SBLOCK_NO_RANK;
    lo[e] = 0u;
    if (on) {
      hi[e] = hi_base[s2 >> Llo];
      lo[e] = lo_rank[s2 & lomask];
    }
  }
}
// the gathers of one chunk: the partner's row of the block, zeros where the bond does not flip the row (no load is issued)
template <int R, int CH>
__device__ __forceinline__ void sblock_gather(double (&xv)[CH][R], const uint32_t (&rk)[CH], const double* __restrict__ v) {
#pragma unroll
  for (int e = 0; e < CH; ++e) {
#pragma unroll
    for (int j = 0; j < R; ++j) xv[e][j] = 0.0;
    if (rk[e] != DSEA_SBLOCK_NO_RANK) block_load<R>(xv[e], v, (int64_t)rk[e]);
  }
}

}  // namespace

// Y = H X for the R columns of a block.  One row per thread: states, the row of X and the row of Y move coalesced; a bond whose
// two bits differ in the row costs two table reads and one gather of the partner's R doubles.  The table reads of chunk c + 1
// are issued before the gathers of chunk c are consumed.  A block walks the row ranges blockIdx.x, + gridDim.x, ... of 256 rows.
// LZ (the Lanczos step, the tail block_spmv_tail): y holds Q_{i-1} on entry and receives W = H x - y diag(beta), beta =
// st[0 .. R) (first: W = H x, y is not read); P receives the per-block partials of x_j . W_j.
template <int R, bool LZ>
__global__ __launch_bounds__(256) void k_spmv_sector_block(SectorBlockParams p, const double* __restrict__ x, double* __restrict__ y,
                                                           const double* __restrict__ st, int first, double* __restrict__ P) {
  constexpr int CH = SblockChunk<R>::value;
  __shared__ double cp[DSEA_SBLOCK_MAX_PARAMS];
  __shared__ uint16_t tb[DSEA_LATTICE_MAX_BONDS];
  __shared__ double sm[R][4];
  const int L = p.L, nb = p.nb, Llo = p.Llo;
  const int64_t n = p.n;
  for (int c = threadIdx.x; c < 2 * nb + L; c += 256) cp[c] = p.c[c];
  for (int c = threadIdx.x; c < nb; c += 256) tb[c] = p.tb[c];
  __syncthreads();
  const double* __restrict__ jxy = cp;
  const double* __restrict__ jzs = cp + nb;
  const double* __restrict__ hzs = cp + 2 * nb;
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
    const int64_t rr = have ? r : n - 1;
    const uint64_t s = p.states[rr];
    double xr[R];
    block_load<R>(xr, x, rr);
    uint32_t rk[CH], hi[CH], lo[CH];
    sblock_ranks<CH>(hi, lo, s, have, 0, nb, Llo, tb, p.lo_rank, p.hi_base);
    double diag = 0.0, sum[R];
#pragma unroll
    for (int j = 0; j < R; ++j) sum[j] = 0.0;
    for (int i = 0; i < L; ++i) diag += block_signed(hzs[i], (s >> i) & 1ull);
    for (int k0 = 0; k0 < nb; k0 += CH) {
      double xv[CH][R];
#pragma unroll
      for (int e = 0; e < CH; ++e) rk[e] = hi[e] + lo[e];
      sblock_gather<R, CH>(xv, rk, x);
      sblock_ranks<CH>(hi, lo, s, have, k0 + CH, nb, Llo, tb, p.lo_rank, p.hi_base);
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        if (k0 + e < nb) {
          diag += block_signed(jzs[k0 + e], block_differ(s, tb[k0 + e]));
          const double c2 = 2.0 * jxy[k0 + e];
#pragma unroll
          for (int j = 0; j < R; ++j) sum[j] = fma(c2, xv[e][j], sum[j]);
        }
      }
    }
    if (have) block_spmv_tail<R, LZ>(y, first, beta, acc, r, xr, diag, sum);
  }
  if constexpr (LZ) block_partials<R>(acc, sm, P);
}

// One order of the Chebyshev recurrence of f(H) X (docs/design/31-chebyshev-propagator.md): with w the row of H x exactly as
// k_spmv_sector_block<R, false> forms it (the same loop, the same operation order, the same bits),
//   t = g (w - centre x)                                  g = 1 / halfwidth on the first order, 2 / halfwidth afterwards
//   first:  acc_a = c0_a x + c1_a t                       (old and acc are not read)
//   else:   t = t - old,  acc_a = acc_a + c1_a t
//   out = t
// every product and sum rounded on its own.  x is T_m, old T_{m-1}, out T_{m+1}; the tail touches the thread's own row only,
// so old == out is allowed (neither is __restrict__); x and the accumulators are distinct from every other block.  old and acc
// are read after the last chunk's gathers are consumed.  No atomics, no reductions.
template <int R, int A>
__global__ __launch_bounds__(256) void k_cheb_sector_block(SectorBlockParams p, const double* __restrict__ x, const double* old,
                                                           double* out, ChebAccs<A> ca, double centre, double g, int first) {
  constexpr int CH = SblockChunk<R>::value;
  __shared__ double cp[DSEA_SBLOCK_MAX_PARAMS];
  __shared__ uint16_t tb[DSEA_LATTICE_MAX_BONDS];
  const int L = p.L, nb = p.nb, Llo = p.Llo;
  const int64_t n = p.n;
  for (int c = threadIdx.x; c < 2 * nb + L; c += 256) cp[c] = p.c[c];
  for (int c = threadIdx.x; c < nb; c += 256) tb[c] = p.tb[c];
  __syncthreads();
  const double* __restrict__ jxy = cp;
  const double* __restrict__ jzs = cp + nb;
  const double* __restrict__ hzs = cp + 2 * nb;
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;                       // (a thread past the last row reads row n - 1 and writes nothing)
    const int64_t rr = have ? r : n - 1;
    const uint64_t s = p.states[rr];
    double xr[R];
    block_load<R>(xr, x, rr);
    uint32_t rk[CH], hi[CH], lo[CH];
    sblock_ranks<CH>(hi, lo, s, have, 0, nb, Llo, tb, p.lo_rank, p.hi_base);
    double diag = 0.0, sum[R];
#pragma unroll
    for (int j = 0; j < R; ++j) sum[j] = 0.0;
    for (int i = 0; i < L; ++i) diag += block_signed(hzs[i], (s >> i) & 1ull);
    for (int k0 = 0; k0 < nb; k0 += CH) {
      double xv[CH][R];
#pragma unroll
      for (int e = 0; e < CH; ++e) rk[e] = hi[e] + lo[e];
      sblock_gather<R, CH>(xv, rk, x);
      sblock_ranks<CH>(hi, lo, s, have, k0 + CH, nb, Llo, tb, p.lo_rank, p.hi_base);
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        if (k0 + e < nb) {
          diag += block_signed(jzs[k0 + e], block_differ(s, tb[k0 + e]));
          const double c2 = 2.0 * jxy[k0 + e];
#pragma unroll
          for (int j = 0; j < R; ++j) sum[j] = fma(c2, xv[e][j], sum[j]);
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

// One order of the Chebyshev recurrence WITH the two reductions of the moments (docs/design/33-chebyshev-moments.md).  The row
// walk is that of k_cheb_sector_block<R, 1>, statement for statement (32-block-kernel-parts.md: sharing it changed the
// existing symbols), and the recurrence part of the tail is its tail without the accumulator block:
//   t = g (w - centre x),  !first: t = t - old,  out = t
//   LEFT = false:  a_j += x_j x_j,  b_j += x_j t_j          LEFT = true:  a_j += y_j x_j,  b_j += y_j t_j
// by fma into the thread's accumulators; y is the row of the left block, read after the last chunk's gathers are consumed like
// old.  A thread without a row adds nothing.  After the row loop the block's partials go to P[(which R + j) gridDim.x + block],
// which = 0 for a, 1 for b: no atomics.  old == out is allowed; x and y are distinct from every written block.
template <int R, bool LEFT>
__global__ __launch_bounds__(256) void k_cheb_sector_moments(SectorBlockParams p, const double* __restrict__ x, const double* old,
                                                             double* out, const double* __restrict__ y, double centre, double g,
                                                             int first, double* __restrict__ P) {
  constexpr int CH = SblockChunk<R>::value;
  __shared__ double cp[DSEA_SBLOCK_MAX_PARAMS];
  __shared__ uint16_t tb[DSEA_LATTICE_MAX_BONDS];
  __shared__ double sma[R][4];
  __shared__ double smb[R][4];
  const int L = p.L, nb = p.nb, Llo = p.Llo;
  const int64_t n = p.n;
  for (int c = threadIdx.x; c < 2 * nb + L; c += 256) cp[c] = p.c[c];
  for (int c = threadIdx.x; c < nb; c += 256) tb[c] = p.tb[c];
  __syncthreads();
  const double* __restrict__ jxy = cp;
  const double* __restrict__ jzs = cp + nb;
  const double* __restrict__ hzs = cp + 2 * nb;
  double acca[R], accb[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    acca[j] = 0.0;
    accb[j] = 0.0;
  }
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;                       // (a thread past the last row reads row n - 1 and writes nothing)
    const int64_t rr = have ? r : n - 1;
    const uint64_t s = p.states[rr];
    double xr[R];
    block_load<R>(xr, x, rr);
    uint32_t rk[CH], hi[CH], lo[CH];
    sblock_ranks<CH>(hi, lo, s, have, 0, nb, Llo, tb, p.lo_rank, p.hi_base);
    double diag = 0.0, sum[R];
#pragma unroll
    for (int j = 0; j < R; ++j) sum[j] = 0.0;
    for (int i = 0; i < L; ++i) diag += block_signed(hzs[i], (s >> i) & 1ull);
    for (int k0 = 0; k0 < nb; k0 += CH) {
      double xv[CH][R];
#pragma unroll
      for (int e = 0; e < CH; ++e) rk[e] = hi[e] + lo[e];
      sblock_gather<R, CH>(xv, rk, x);
      sblock_ranks<CH>(hi, lo, s, have, k0 + CH, nb, Llo, tb, p.lo_rank, p.hi_base);
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        if (k0 + e < nb) {
          diag += block_signed(jzs[k0 + e], block_differ(s, tb[k0 + e]));
          const double c2 = 2.0 * jxy[k0 + e];
#pragma unroll
          for (int j = 0; j < R; ++j) sum[j] = fma(c2, xv[e][j], sum[j]);
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
static bool sector_block_params(const OpDesc& op, SectorBlockParams* p) {
  const SectorDesc& d = op.sector;
  int64_t n, n_lo, n_hi;
  if (!sector_sizes(d.L, d.ndown, &n, &n_lo, &n_hi) || n != op.n || d.nb < 1 || d.nb > DSEA_LATTICE_MAX_BONDS) return false;
  if (op.tune_tile_log2 < 6 || op.tune_tile_log2 > 12 || !d.c || !d.states || !d.lo_rank || !d.hi_base) return false;
  p->L = d.L;
  p->nb = d.nb;
  p->Llo = (d.L + 1) / 2;
  p->n = n;
  p->c = d.c;
  p->states = d.states;
  p->lo_rank = d.lo_rank;
  p->hi_base = d.hi_base;
  block_pack_bonds(p->tb, d.a, d.b, d.nb);
  return true;
}

int launch_sector_block_apply(const OpDesc& op, int R, const double* X, double* Y, hipStream_t st) {
  SectorBlockParams p;
  if (!sector_block_params(op, &p)) return -1;
  const int nblk = block_blocks(op);
  dispatch_block_width(R, [&](auto r) {
    klaunch(nullptr, k_spmv_sector_block<decltype(r)::value, false>, nblk, 256, 0, st, p, X, Y, nullptr, 1, nullptr);
  });
  return nblk;
}

// ACC[a] = sum_{m < M} coeffs[a * M + m] T_m((H - centre) / halfwidth) X in M - 1 launches of k_cheb_sector_block: order 1 is
// `first` with x = X and out = U; order 2 reads x = U, old = X and writes V; from order 3 on old == out, U and V in turn.  The
// two coefficients of an order go into its launch by value from the host array.  Nothing is read back, no synchronise.
int launch_sector_block_chebyshev(const OpDesc& op, int R, int A, int M, double centre, double halfwidth, const double* coeffs,
                                  const double* X, double* U, double* V, double* ACC, hipStream_t st) {
  SectorBlockParams p;
  if (!sector_block_params(op, &p)) return -1;
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
        klaunch(nullptr, k_cheb_sector_block<RR, AA>, nblk, 256, 0, st, p, x, old, t[(m - 1) & 1], ca, centre,
                (m == 1 ? 1.0 : 2.0) / halfwidth, m == 1 ? 1 : 0);
      }
    });
  });
  return nblk;
}

// the schedule of block_moments_drive with this file's moments kernel as the step; Y null: self mode
int launch_sector_block_moments(const OpDesc& op, int R, int M, double centre, double halfwidth, const double* X, const double* Y,
                                double* U, double* V, double* MU, double* scratch, hipStream_t st) {
  SectorBlockParams p;
  if (!sector_block_params(op, &p)) return -1;
  const int nblk = block_blocks(op);
  return block_moments_drive(op.n, nblk, R, M, Y != nullptr, X, U, V, MU, scratch, st,
                             [&](const double* x, const double* old, double* out, int first, double* P) {
                               dispatch_block_width(R, [&](auto r) {
                                 dispatch_bool(Y != nullptr, [&](auto left) {
                                   klaunch(nullptr, k_cheb_sector_moments<decltype(r)::value, decltype(left)::value>, nblk, 256, 0,
                                           st, p, x, old, out, Y, centre, (first ? 1.0 : 2.0) / halfwidth, first, P);
                                 });
                               });
                             });
}

// the recurrence of block_lanczos_drive with this file's mat-vec as the step
int launch_sector_block_lanczos(const OpDesc& op, int R, int k, double* Q, double* W, double* norm2, double* alphas, double* betas,
                                int32_t* steps, double* scratch, hipStream_t st) {
  SectorBlockParams p;
  if (!sector_block_params(op, &p)) return -1;
  const int nblk = block_blocks(op);
  return block_lanczos_drive(op.n, nblk, R, k, Q, W, norm2, alphas, betas, steps, scratch, st,
                             [&](const double* q, double* w, const double* state, int first, double* PA) {
                               dispatch_block_width(R, [&](auto r) {
                                 klaunch(nullptr, k_spmv_sector_block<decltype(r)::value, true>, nblk, 256, 0, st, p, q, w, state,
                                         first, PA);
                               });
                             });
}

}  // namespace dsea
