// dsea_sector_block.hip -- the bond-list sector Hamiltonian of dsea_sector.hip applied to a BLOCK of R vectors at once, and the
// basis-free block Lanczos recurrence built on it (docs/design/27-finite-temperature.md): k_spmv_sector_block<R, LZ>,
// k_sblock_norm<R>, k_sblock_update<R>, k_sblock_finish<R>, and their launchers.  The recurrence kernels know nothing about the
// operator: block_lanczos_drive runs them around a caller's mat-vec step, for this file's kernel and for the Hubbard block
// kernel of dsea_hubbard_block.hip alike.
//
// A block is an fp64 array [n, R], row-major (element (r, j) at r * R + j), 16-byte aligned, R in {1, 2, 4, 8}.  One row per
// thread: the row's state word and the two table reads of a flipped bond are paid once for all R columns, and every gather
// is R contiguous doubles (R / 2 16-byte loads; one 8-byte load at R = 1).  The per-row arithmetic of a column is that of the
// single-vector mat-vec of dsea_sector.hip in the same order -- the diagonal accumulated over the sites and then the bonds,
// sum = fma(2 Jxy_t, x_partner, sum) over the bonds in list order, then fma(diag, x_r, sum) -- so column j of Y = H X equals the
// single-vector result bit for bit.
//
// The recurrence (per column j, all columns in the same launches, nothing read back by the host during a run):
//   start:   norm2_j = |Q_j|^2, beta_0 = sqrt(norm2_j), Q_j /= beta_0
//   step i:  W = H Q_i - Q_{i-1} diag(beta_i)   (W overwrites Q_{i-1}; i = 0: W = H Q_0),  partials of alpha_j = Q_i[:, j] . W[:, j]
//            W -= Q_i diag(alpha),  partials of |W_j|^2
//            alphas[i, j] = alpha_j, betas[i, j] = beta_{i+1} = |W_j|, Q_{i+1} = W / beta_{i+1}
// Column j breaks at the first s = i + 1 with !(beta_s > 1e-13 max(earlier |alpha_j|, |beta_j|)) (the rule of
// dsea_lanczos_status; a start column of norm 0 breaks at s = 0): steps[j] = s, the column is zeroed in both blocks, its later
// alphas and betas (and the breaking beta) are written as 0, and nothing divides by its beta.  The other columns go on.
// Every reduction is wave, block, then the per-block partials summed in index order by every block alike: no atomics, two
// identical calls give identical bits.  The per-column state (beta, scale, alive) lives in the caller's scratch in two copies
// that alternate by step, so that no launch reads a word that another block of the same launch writes.
// Nothing here is shared with dsea_sector.hip: the file has its own helpers.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_internal.h"
#include "dsea_device.h"

namespace dsea {

namespace {
#define DSEA_SBLOCK_MAX_PARAMS (2 * DSEA_LATTICE_MAX_BONDS + DSEA_SECTOR_MAX_L)
#define DSEA_SBLOCK_NO_RANK 0xFFFFFFFFu /* "this bond does not flip this row" (a rank is below 2^31) */
#define DSEA_SBLOCK_STATE 32            /* doubles per copy of the per-column state: beta[8], scale[8], alive[8] */

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

// v * (1 - 2 bit), exact: the bit goes into the sign
__device__ __forceinline__ double sblock_signed(double v, uint64_t bit) {
  return __longlong_as_double(__double_as_longlong(v) ^ (long long)(bit << 63));
}
__device__ __forceinline__ uint64_t sblock_differ(uint64_t s, uint32_t e) { return ((s >> (e & 255u)) ^ (s >> (e >> 8))) & 1ull; }
__device__ __forceinline__ uint64_t sblock_mask(uint32_t e) { return (1ull << (e & 255u)) | (1ull << (e >> 8)); }

// one row of a block: R / 2 16-byte loads or stores (one 8-byte access at R = 1)
template <int R>
__device__ __forceinline__ void sblock_load(double (&v)[R], const double* __restrict__ p, int64_t row) {
  if constexpr (R == 1) {
    v[0] = p[row];
  } else {
    const double2* __restrict__ q = reinterpret_cast<const double2*>(p + row * R);
#pragma unroll
    for (int h = 0; h < R / 2; ++h) {
      const double2 t = q[h];
      v[2 * h] = t.x;
      v[2 * h + 1] = t.y;
    }
  }
}
template <int R>
__device__ __forceinline__ void sblock_store(double* __restrict__ p, int64_t row, const double (&v)[R]) {
  if constexpr (R == 1) {
    p[row] = v[0];
  } else {
    double2* __restrict__ q = reinterpret_cast<double2*>(p + row * R);
#pragma unroll
    for (int h = 0; h < R / 2; ++h) q[h] = make_double2(v[2 * h], v[2 * h + 1]);
  }
}

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
    const bool on = have && k0 + e < nb && sblock_differ(s, w) != 0;
    const uint64_t s2 = s ^ sblock_mask(w);
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
    if (rk[e] != DSEA_SBLOCK_NO_RANK) sblock_load<R>(xv[e], v, (int64_t)rk[e]);
  }
}

// per-block partials of R per-thread sums: wave sums, then the four waves in fixed order; P[j * gridDim.x + block]
template <int R>
__device__ __forceinline__ void sblock_partials(const double (&acc)[R], double (*sm)[4], double* __restrict__ P) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const double t = wave_sum(acc[j]);
    if (lane == 0) sm[j][wv] = t;
  }
  __syncthreads();
  if (threadIdx.x < R) {
    const double* s4 = sm[threadIdx.x];
    P[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = ((s4[0] + s4[1]) + s4[2]) + s4[3];
  }
}
}  // namespace

// Y = H X for the R columns of a block.  One row per thread: states, the row of X and the row of Y move coalesced; a bond whose
// two bits differ in the row costs two table reads and one gather of the partner's R doubles.  The table reads of chunk c + 1
// are issued before the gathers of chunk c are consumed.  A block walks the row ranges blockIdx.x, + gridDim.x, ... of 256 rows.
// LZ (the Lanczos step): y holds Q_{i-1} on entry and receives W = H x - y diag(beta), beta = st[0 .. R) (first: W = H x, y is
// not read); P receives the per-block partials of x_j . W_j.
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
    sblock_load<R>(xr, x, rr);
    uint32_t rk[CH], hi[CH], lo[CH];
    sblock_ranks<CH>(hi, lo, s, have, 0, nb, Llo, tb, p.lo_rank, p.hi_base);
    double diag = 0.0, sum[R];
#pragma unroll
    for (int j = 0; j < R; ++j) sum[j] = 0.0;
    for (int i = 0; i < L; ++i) diag += sblock_signed(hzs[i], (s >> i) & 1ull);
    for (int k0 = 0; k0 < nb; k0 += CH) {
      double xv[CH][R];
#pragma unroll
      for (int e = 0; e < CH; ++e) rk[e] = hi[e] + lo[e];
      sblock_gather<R, CH>(xv, rk, x);
      sblock_ranks<CH>(hi, lo, s, have, k0 + CH, nb, Llo, tb, p.lo_rank, p.hi_base);
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        if (k0 + e < nb) {
          diag += sblock_signed(jzs[k0 + e], sblock_differ(s, tb[k0 + e]));
          const double c2 = 2.0 * jxy[k0 + e];
#pragma unroll
          for (int j = 0; j < R; ++j) sum[j] = fma(c2, xv[e][j], sum[j]);
        }
      }
    }
    if (have) {
      double v[R];
#pragma unroll
      for (int j = 0; j < R; ++j) v[j] = fma(diag, xr[j], sum[j]);
      if constexpr (LZ) {
        if (!first) {
          double old[R];
          sblock_load<R>(old, y, r);
#pragma unroll
          for (int j = 0; j < R; ++j) v[j] = __dsub_rn(v[j], __dmul_rn(beta[j], old[j]));
        }
#pragma unroll
        for (int j = 0; j < R; ++j) acc[j] = fma(xr[j], v[j], acc[j]);
      }
      sblock_store<R>(y, r, v);
    }
  }
  if constexpr (LZ) sblock_partials<R>(acc, sm, P);
}

// the per-accumulator arguments of one Chebyshev order, by value
template <int A>
struct ChebAccs {
  double* acc[A];
  double c0[A], c1[A];
};

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
    sblock_load<R>(xr, x, rr);
    uint32_t rk[CH], hi[CH], lo[CH];
    sblock_ranks<CH>(hi, lo, s, have, 0, nb, Llo, tb, p.lo_rank, p.hi_base);
    double diag = 0.0, sum[R];
#pragma unroll
    for (int j = 0; j < R; ++j) sum[j] = 0.0;
    for (int i = 0; i < L; ++i) diag += sblock_signed(hzs[i], (s >> i) & 1ull);
    for (int k0 = 0; k0 < nb; k0 += CH) {
      double xv[CH][R];
#pragma unroll
      for (int e = 0; e < CH; ++e) rk[e] = hi[e] + lo[e];
      sblock_gather<R, CH>(xv, rk, x);
      sblock_ranks<CH>(hi, lo, s, have, k0 + CH, nb, Llo, tb, p.lo_rank, p.hi_base);
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        if (k0 + e < nb) {
          diag += sblock_signed(jzs[k0 + e], sblock_differ(s, tb[k0 + e]));
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
        sblock_load<R>(ov, old, r);
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
          sblock_load<R>(av, ca.acc[a], r);
#pragma unroll
          for (int j = 0; j < R; ++j) av[j] = __dadd_rn(av[j], __dmul_rn(ca.c1[a], t[j]));
        }
        sblock_store<R>(ca.acc[a], r, av);
      }
      sblock_store<R>(out, r, t);
    }
  }
}

// per-block partials of |q_j|^2 of the start block
template <int R>
__global__ __launch_bounds__(256) void k_sblock_norm(const double* __restrict__ q, int64_t n, double* __restrict__ P) {
  __shared__ double sm[R][4];
  double acc[R];
#pragma unroll
  for (int j = 0; j < R; ++j) acc[j] = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
    double v[R];
    sblock_load<R>(v, q, r);
#pragma unroll
    for (int j = 0; j < R; ++j) acc[j] = fma(v[j], v[j], acc[j]);
  }
  sblock_partials<R>(acc, sm, P);
}

// alpha_j = the sum of the mat-vec's partials PA (every block sums them alike; block 0 stores alphas_row[j]);
// w -= q diag(alpha); per-block partials PB of |w_j|^2
template <int R>
__global__ __launch_bounds__(256) void k_sblock_update(const double* __restrict__ q, double* __restrict__ w, int64_t n,
                                                       const double* __restrict__ PA, int count, double* __restrict__ alphas_row,
                                                       double* __restrict__ PB) {
  __shared__ double sm5[5];
  __shared__ double sm[R][4];
  double alpha[R], acc[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    alpha[j] = sum_partials_block(PA + (int64_t)j * count, count, sm5);
    acc[j] = 0.0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < R; ++j) alphas_row[j] = alpha[j];
  }
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
    double qv[R], wv[R];
    sblock_load<R>(qv, q, r);
    sblock_load<R>(wv, w, r);
#pragma unroll
    for (int j = 0; j < R; ++j) {
      wv[j] = __dsub_rn(wv[j], __dmul_rn(alpha[j], qv[j]));
      acc[j] = fma(wv[j], wv[j], acc[j]);
    }
    sblock_store<R>(w, r, wv);
  }
  sblock_partials<R>(acc, sm, PB);
}

// beta_j = sqrt of the sum of the partials PB; the break decision (the same in every block); w = w / beta for a live column,
// 0 for a broken one -- a column that breaks now is also zeroed in `other` (Q_i; null at the start).  Block 0 stores
// out_row[j] (betas[i, j]; norm2[j] at the start, step = 0), steps[j] and the next copy of the state.  step = i + 1.
template <int R>
__global__ __launch_bounds__(256) void k_sblock_finish(double* __restrict__ w, double* __restrict__ other, int64_t n,
                                                       const double* __restrict__ PB, int count,
                                                       const double* __restrict__ alphas_row, double* __restrict__ out_row,
                                                       const double* __restrict__ st_in, double* __restrict__ st_out,
                                                       int32_t* __restrict__ steps, int step, int k) {
  __shared__ double sm5[5];
  const bool start = step == 0;
  double beta[R];
  bool live[R], now[R];
  bool any_now = false;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const double sumsq = sum_partials_block(PB + (int64_t)j * count, count, sm5);
    const bool alive = start ? true : st_in[2 * R + j] != 0.0;
    double scale = start ? 0.0 : st_in[R + j];
    beta[j] = 0.0;
    now[j] = false;
    if (alive) {
      if (!start) scale = fmax(scale, fabs(alphas_row[j]));
      const double b = sqrt(sumsq);
      if (!(b > DSEA_BREAK_TOL * scale)) {          // (also catches NaN; at the start the scale is 0: a zero column)
        now[j] = true;
      } else {
        beta[j] = b;
        scale = fmax(scale, b);
      }
    }
    live[j] = alive && !now[j];
    any_now |= now[j];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      out_row[j] = start ? sumsq : beta[j];
      st_out[j] = beta[j];
      st_out[R + j] = scale;
      st_out[2 * R + j] = live[j] ? 1.0 : 0.0;
      if (now[j]) steps[j] = step;
      else if (start) steps[j] = k;
    }
  }
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
    double v[R];
    sblock_load<R>(v, w, r);
#pragma unroll
    for (int j = 0; j < R; ++j) v[j] = live[j] ? v[j] / beta[j] : 0.0;
    sblock_store<R>(w, r, v);
    if (any_now && other) {
#pragma unroll
      for (int j = 0; j < R; ++j)
        if (now[j]) other[r * R + j] = 0.0;
    }
  }
}

// one block per 256 rows up to the cap 2^tune_tile_log2 (6 .. 12, 12 at creation: 4096); beyond it blocks walk row ranges
static inline int sector_block_blocks(const OpDesc& op) {
  int64_t nblk = (op.n + 255) / 256;
  const int64_t cap = (int64_t)1 << op.tune_tile_log2;
  if (nblk > cap) nblk = cap;
  return (int)nblk;
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
  for (int t = 0; t < DSEA_LATTICE_MAX_BONDS; ++t)
    p->tb[t] = t < d.nb ? (uint16_t)((uint32_t)d.a[t] | ((uint32_t)d.b[t] << 8)) : (uint16_t)0;
  return true;
}

// the one place that turns the run-time R into the template argument
template <class F>
static inline void dispatch_block_width(int R, F&& f) { dispatch_int<1, 2, 4, 8>(R, f); }

// doubles of scratch a block Lanczos run may touch at any grid cap: two copies of the state, then the two partial arrays
int64_t sector_block_lanczos_scratch_doubles(int64_t n, int R) {
  int64_t nblk = (n + 255) / 256;
  if (nblk > DSEA_MAX_TFIM_BLOCKS) nblk = DSEA_MAX_TFIM_BLOCKS;
  return 2 * DSEA_SBLOCK_STATE + 2 * (int64_t)R * nblk;
}

int launch_sector_block_apply(const OpDesc& op, int R, const double* X, double* Y, hipStream_t st) {
  SectorBlockParams p;
  if (!sector_block_params(op, &p)) return -1;
  const int nblk = sector_block_blocks(op);
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
  const int nblk = sector_block_blocks(op);
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

// The recurrence for any operator: start (norm, finish) and k steps of three launches each -- the caller's mat-vec step, update,
// finish; nothing is read back.  Q and W change roles from step to step.  step(q, w, state, first, PA) launches, on st and with
// nblk blocks, W = H q - w diag(state[0 .. R)) over w (first: W = H q, w not read) and the partials PA[j * nblk + block] of
// q_j . W_j.
int block_lanczos_drive(int64_t n, int nblk, int R, int k, double* Q, double* W, double* norm2, double* alphas, double* betas,
                        int32_t* steps, double* scratch, hipStream_t st, const BlockLanczosStep& step) {
  double* state[2] = {scratch, scratch + DSEA_SBLOCK_STATE};
  double* PA = scratch + 2 * DSEA_SBLOCK_STATE;
  double* PB = PA + (int64_t)R * nblk;
  dispatch_block_width(R, [&](auto r) {
    constexpr int RR = decltype(r)::value;
    klaunch(nullptr, k_sblock_norm<RR>, nblk, 256, 0, st, Q, n, PB);
    klaunch(nullptr, k_sblock_finish<RR>, nblk, 256, 0, st, Q, nullptr, n, PB, nblk, nullptr, norm2, nullptr, state[0], steps, 0, k);
    double* q = Q;
    double* w = W;
    for (int i = 0; i < k; ++i) {
      step(q, w, state[i & 1], i == 0 ? 1 : 0, PA);
      klaunch(nullptr, k_sblock_update<RR>, nblk, 256, 0, st, q, w, n, PA, nblk, alphas + (int64_t)i * RR, PB);
      klaunch(nullptr, k_sblock_finish<RR>, nblk, 256, 0, st, w, q, n, PB, nblk, alphas + (int64_t)i * RR, betas + (int64_t)i * RR,
              state[i & 1], state[(i + 1) & 1], steps, i + 1, k);
      double* t = q;
      q = w;
      w = t;
    }
  });
  return 0;
}

// the recurrence with this file's mat-vec as the step
int launch_sector_block_lanczos(const OpDesc& op, int R, int k, double* Q, double* W, double* norm2, double* alphas, double* betas,
                                int32_t* steps, double* scratch, hipStream_t st) {
  SectorBlockParams p;
  if (!sector_block_params(op, &p)) return -1;
  const int nblk = sector_block_blocks(op);
  return block_lanczos_drive(op.n, nblk, R, k, Q, W, norm2, alphas, betas, steps, scratch, st,
                             [&](const double* q, double* w, const double* state, int first, double* PA) {
                               dispatch_block_width(R, [&](auto r) {
                                 klaunch(nullptr, k_spmv_sector_block<decltype(r)::value, true>, nblk, 256, 0, st, p, q, w, state,
                                         first, PA);
                               });
                             });
}

}  // namespace dsea
