// dsea_hubbard.hip -- matrix-free Hubbard model of spinful fermions on a caller-given bond list at fixed particle numbers
// (N_up, N_dn) (docs/design/19-hubbard.md): the mat-vec k_spmv_hubbard, the parameter adjoint k_hubbard_forms
// (+ k_hubbard_forms_reduce), and their launchers.
//
//   H = sum_t [ -t_t sum_s (c+_{a s} c_{b s} + h.c.) + V_t n_a n_b ] + sum_i U_i n_{i up} n_{i dn} + sum_i eps_i n_i
// with bond t joining sites a_t != b_t and n_i = n_{i up} + n_{i dn}.  Bit i of the word u is the occupation of (i, up), bit i
// of d that of (i, dn); |u, d> = (prod_{i in u, ascending} c+_{i up}) (prod_{j in d, ascending} c+_{j dn}) |0>, so a hop never
// picks up a sign from the other species.  Row r = ru * n_dn + rd, ru the rank of u among the L-bit words of nup set bits in
// increasing integer order, rd likewise for d (down fastest); n = C(L, nup) C(L, ndn) <= 2^31 - 1.  With
// m_t = (1 << a_t) | (1 << b_t), B_t the bits strictly between a_t and b_t, sgn_t(w) = (-1)^popcount(w & B_t):
//   (H x)[r] = diag(u, d) x[r] - sum_{t : bit_a(u) != bit_b(u)} t_t sgn_t(u) x[rank_u(u ^ m_t) n_dn + rd]
//                              - sum_{t : bit_a(d) != bit_b(d)} t_t sgn_t(d) x[ru n_dn + rank_d(d ^ m_t)]
//   diag(u, d) = sum_i U_i bit_i(u) bit_i(d) + sum_i eps_i (bit_i(u) + bit_i(d)) + sum_t V_t n_a n_b
// rank_s(w) = hi_base_s[w >> Llo] + lo_rank_s[w & (2^Llo - 1)], Llo = (L + 1) / 2: Lin's two tables of each species, in the
// layout that dsea_sector_build_tables fills at (L, nup) and (L, ndn).  An up hop gathers x at a distance that is a multiple of
// n_dn: consecutive across the lanes that share ru.  A down hop stays inside the row's own window of n_dn entries.  The
// couplings are one device array [t(nb), V(nb), U(L), eps(L)], copied into LDS by every block on every launch; the bond
// table travels by value in the kernel arguments, in the caller's order.
// Nothing here is shared with dsea_sector.hip or dsea_lattice.hip: the file has its own helpers.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_internal.h"
#include "dsea_device.h"

namespace dsea {

#define DSEA_HUBBARD_MAX_PARAMS (2 * DSEA_LATTICE_MAX_BONDS + 2 * DSEA_SECTOR_MAX_L)
#define DSEA_HUBBARD_CHUNK 4             /* bonds per chunk: 2 * CHUNK hops whose table lookups and gathers are in flight together */
#define DSEA_HUBBARD_HOPS (2 * DSEA_HUBBARD_CHUNK)
#define DSEA_HUBBARD_NO_ROW 0xFFFFFFFFu  /* "this hop does not move a particle in this row" (a row is below 2^31) */

struct HubbardParams {
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

// v * (1 - 2 bit), exact: the bit goes into the sign
__device__ __forceinline__ double hubbard_signed(double v, uint64_t bit) {
  return __longlong_as_double(__double_as_longlong(v) ^ (long long)(bit << 63));
}
__device__ __forceinline__ uint64_t hubbard_bit(uint64_t w, uint32_t site) { return (w >> site) & 1ull; }
__device__ __forceinline__ uint64_t hubbard_moves(uint64_t w, uint32_t e) { return ((w >> (e & 255u)) ^ (w >> (e >> 8))) & 1ull; }
__device__ __forceinline__ uint64_t hubbard_mask(uint32_t e) { return (1ull << (e & 255u)) | (1ull << (e >> 8)); }
// the bits strictly between the two sites of the bond
__device__ __forceinline__ uint64_t hubbard_between(uint32_t e) {
  const uint32_t a = e & 255u, b = e >> 8;
  const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
  return ((1ull << hi) - 1) & ~((1ull << (lo + 1)) - 1);
}
// the parity of the particles that the hop over bond mask `between` jumps: 1 for a hop amplitude of +t, i.e. sgn_t(w) = -1
__device__ __forceinline__ uint64_t hubbard_parity(uint64_t w, uint64_t between) { return (uint64_t)(__popcll(w & between) & 1); }
// n_a n_b of the bond, 0 .. 4
__device__ __forceinline__ double hubbard_nn(uint64_t u, uint64_t d, uint32_t e) {
  const uint32_t a = e & 255u, b = e >> 8;
  return (double)((hubbard_bit(u, a) + hubbard_bit(d, a)) * (hubbard_bit(u, b) + hubbard_bit(d, b)));
}

// the bond table and the sign masks of a block, in LDS
__device__ __forceinline__ void hubbard_stage_bonds(const HubbardParams& p, uint16_t* tb, uint64_t* bm) {
  for (int c = threadIdx.x; c < p.nb; c += 256) {
    const uint16_t e = p.tb[c];
    tb[c] = e;
    bm[c] = hubbard_between(e);
  }
}

// the table reads of bonds k0 .. k0 + CHUNK - 1 for the row with words (u, d): slot 2 e is the up hop of bond k0 + e, slot
// 2 e + 1 its down hop.  Two table reads per hop that moves a particle, requested and NOT used here (a use next to the read
// would make the compiler wait for every hop in turn).  Returns the slots that move a particle as a bit mask; the others (and
// those past the last bond) issue no load and leave hi and lo as they are -- no common default value, which the compiler
// would keep as one register tuple and fill in with a wait per read.
__device__ __forceinline__ uint32_t hubbard_lookups(uint32_t (&hi)[DSEA_HUBBARD_HOPS], uint32_t (&lo)[DSEA_HUBBARD_HOPS],
                                                    uint64_t u, uint64_t d, bool have, int k0, const HubbardParams& p,
                                                    const uint16_t* tb) {
  const int Llo = p.Llo;
  const uint64_t lomask = (1ull << Llo) - 1;
  const uint32_t* __restrict__ up_lo = p.up_lo;
  const uint32_t* __restrict__ up_hi = p.up_hi;
  const uint32_t* __restrict__ dn_lo = p.dn_lo;
  const uint32_t* __restrict__ dn_hi = p.dn_hi;
  uint32_t on = 0;
#pragma unroll
  for (int e = 0; e < DSEA_HUBBARD_CHUNK; ++e) {
    const bool in = have && k0 + e < p.nb;
    const uint32_t w = k0 + e < p.nb ? tb[k0 + e] : 0u;
    const uint64_t m = hubbard_mask(w);
    const uint64_t u2 = u ^ m, d2 = d ^ m;
    if (in && hubbard_moves(u, w) != 0) {
      hi[2 * e] = up_hi[u2 >> Llo];
      lo[2 * e] = up_lo[u2 & lomask];
      on |= 1u << (2 * e);
    }
    if (in && hubbard_moves(d, w) != 0) {
      hi[2 * e + 1] = dn_hi[d2 >> Llo];
      lo[2 * e + 1] = dn_lo[d2 & lomask];
      on |= 2u << (2 * e);
    }
  }
  return on;
}
// the partner rows of one chunk from its table reads, DSEA_HUBBARD_NO_ROW in the slots that move nothing: the up partner keeps
// rd, the down partner keeps ru
__device__ __forceinline__ void hubbard_rows(uint32_t (&rw)[DSEA_HUBBARD_HOPS], uint32_t on, const uint32_t (&hi)[DSEA_HUBBARD_HOPS],
                                             const uint32_t (&lo)[DSEA_HUBBARD_HOPS], uint32_t ru, uint32_t rd, uint32_t n_dn) {
#pragma unroll
  for (int e = 0; e < DSEA_HUBBARD_CHUNK; ++e) {
    rw[2 * e] = (on >> (2 * e)) & 1u ? (hi[2 * e] + lo[2 * e]) * n_dn + rd : DSEA_HUBBARD_NO_ROW;
    rw[2 * e + 1] = (on >> (2 * e + 1)) & 1u ? ru * n_dn + (hi[2 * e + 1] + lo[2 * e + 1]) : DSEA_HUBBARD_NO_ROW;
  }
}
// the gathers of one chunk: v[row], 0 where the hop moves nothing
__device__ __forceinline__ void hubbard_gather(double (&xv)[DSEA_HUBBARD_HOPS], const uint32_t (&rw)[DSEA_HUBBARD_HOPS],
                                               const double* __restrict__ v) {
#pragma unroll
  for (int e = 0; e < DSEA_HUBBARD_HOPS; ++e) {
    xv[e] = 0.0;
    if (rw[e] != DSEA_HUBBARD_NO_ROW) xv[e] = v[rw[e]];
  }
}

// y = H x - shift x ; partial x.y per block.  One row per thread: x and y are read and written coalesced, dn_states[rd] too;
// up_states[ru] is one address for all lanes that share ru.  The table reads of chunk c + 1 are issued before the gathers of
// chunk c are consumed.  A block walks the row ranges blockIdx.x, + gridDim.x, ... of 256 rows.
__global__ __launch_bounds__(256) void k_spmv_hubbard(HubbardParams p, const double* __restrict__ x, double* __restrict__ y,
                                                      const double* __restrict__ shift, const double* __restrict__ skip,
                                                      double* __restrict__ P) {
  __shared__ double cp[DSEA_HUBBARD_MAX_PARAMS];
  __shared__ uint64_t bm[DSEA_LATTICE_MAX_BONDS];
  __shared__ uint16_t tb[DSEA_LATTICE_MAX_BONDS];
  __shared__ double sm5[5];
  if (skip && skip[0] != 0.0) return;
  const int L = p.L, nb = p.nb;
  const int64_t n = p.n;
  for (int c = threadIdx.x; c < 2 * nb + 2 * L; c += 256) cp[c] = p.c[c];
  hubbard_stage_bonds(p, tb, bm);
  __syncthreads();
  const double* __restrict__ ts = cp;
  const double* __restrict__ Vs = cp + nb;
  const double* __restrict__ Us = cp + 2 * nb;
  const double* __restrict__ es = cp + 2 * nb + L;
  const double s = shift ? shift[0] : 0.0;
  double acc = 0.0;
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;                       // (a thread past the last row reads row n - 1 and writes nothing)
    const uint32_t rr = (uint32_t)(have ? r : n - 1);
    const uint32_t ru = rr / p.n_dn, rd = rr - ru * p.n_dn;
    const uint64_t u = p.up_states[ru], d = p.dn_states[rd];
    const double xr = x[rr];
    uint32_t hi[DSEA_HUBBARD_HOPS], lo[DSEA_HUBBARD_HOPS];
    uint32_t on = hubbard_lookups(hi, lo, u, d, have, 0, p, tb);
    double diag = 0.0, sum = 0.0;
    const uint64_t both = u & d;
    for (int i = 0; i < L; ++i) {
      diag += hubbard_bit(both, i) ? Us[i] : 0.0;
      diag = fma(es[i], (double)(hubbard_bit(u, i) + hubbard_bit(d, i)), diag);
    }
    for (int k0 = 0; k0 < nb; k0 += DSEA_HUBBARD_CHUNK) {
      uint32_t rw[DSEA_HUBBARD_HOPS];
      double xv[DSEA_HUBBARD_HOPS];
      hubbard_rows(rw, on, hi, lo, ru, rd, p.n_dn);
      hubbard_gather(xv, rw, x);
      on = hubbard_lookups(hi, lo, u, d, have, k0 + DSEA_HUBBARD_CHUNK, p, tb);
#pragma unroll
      for (int e = 0; e < DSEA_HUBBARD_CHUNK; ++e) {
        if (k0 + e < nb) {
          const uint32_t w = tb[k0 + e];
          const uint64_t between = bm[k0 + e];
          const double tt = ts[k0 + e];
          diag = fma(Vs[k0 + e], hubbard_nn(u, d, w), diag);
          // -t sgn = t (-1)^(parity + 1): the sign goes into the sign bit of the coupling
          sum = fma(hubbard_signed(tt, hubbard_parity(u, between) ^ 1ull), xv[2 * e], sum);
          sum = fma(hubbard_signed(tt, hubbard_parity(d, between) ^ 1ull), xv[2 * e + 1], sum);
        }
      }
    }
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

// The parameter adjoint: all 2 nb + 2 L bilinear forms out[p] = v1^T (dH/dp) v2 in one pass over v1 and v2 (p in the order of
// the couplings: t_t, V_t, U_i, eps_i):
//   t_t: -sum_r v1[r] (sgn_t(u) v2[up partner] + sgn_t(d) v2[dn partner])       V_t: sum_r n_a n_b v1[r] v2[r]
//   U_i: sum_r bit_i(u) bit_i(d) v1[r] v2[r]                                   eps_i: sum_r (bit_i(u) + bit_i(d)) v1[r] v2[r]
// Same row walk and the same chunks of lookups and gathers (of v2) as the mat-vec.  No per-lane accumulator per term: every
// term is reduced through the wave at once (wave_sum, fixed order) and lane 0 adds it to the wave's row of LDS accumulators; the
// four rows are added in fixed order and written to scratch[p * gridDim.x + block].  No atomics.
__global__ __launch_bounds__(256) void k_hubbard_forms(HubbardParams p, const double* __restrict__ v1,
                                                       const double* __restrict__ v2, double* __restrict__ scratch) {
  __shared__ double accs[4][DSEA_HUBBARD_MAX_PARAMS];
  __shared__ uint64_t bm[DSEA_LATTICE_MAX_BONDS];
  __shared__ uint16_t tb[DSEA_LATTICE_MAX_BONDS];
  const int L = p.L, nb = p.nb;
  const int nparam = 2 * nb + 2 * L;
  const int64_t n = p.n;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double* __restrict__ mine = accs[wv];
  for (int c = lane; c < nparam; c += 64) mine[c] = 0.0;   // (afterwards a wave's row is touched by its lane 0 alone)
  hubbard_stage_bonds(p, tb, bm);
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
    const double dd = a * v2[rr];
    uint32_t hi[DSEA_HUBBARD_HOPS], lo[DSEA_HUBBARD_HOPS];
    uint32_t on = hubbard_lookups(hi, lo, u, d, have, 0, p, tb);
    for (int k0 = 0; k0 < nb; k0 += DSEA_HUBBARD_CHUNK) {
      uint32_t rw[DSEA_HUBBARD_HOPS];
      double xv[DSEA_HUBBARD_HOPS];
      hubbard_rows(rw, on, hi, lo, ru, rd, p.n_dn);
      hubbard_gather(xv, rw, v2);
      on = hubbard_lookups(hi, lo, u, d, have, k0 + DSEA_HUBBARD_CHUNK, p, tb);
#pragma unroll
      for (int e = 0; e < DSEA_HUBBARD_CHUNK; ++e) {
        if (k0 + e < nb) {                         // (the same for every lane: the wave sums run with all lanes)
          const uint32_t w = tb[k0 + e];
          const uint64_t between = bm[k0 + e];
          const double hop = hubbard_signed(xv[2 * e], hubbard_parity(u, between) ^ 1ull) +
                             hubbard_signed(xv[2 * e + 1], hubbard_parity(d, between) ^ 1ull);
          add(k0 + e, a * hop);                                  // t_t
          add(nb + k0 + e, hubbard_nn(u, d, w) * dd);            // V_t
        }
      }
    }
    const uint64_t both = u & d;
    for (int i = 0; i < L; ++i) add(2 * nb + i, hubbard_bit(both, i) ? dd : 0.0);                            // U_i
    for (int i = 0; i < L; ++i) add(2 * nb + L + i, (double)(hubbard_bit(u, i) + hubbard_bit(d, i)) * dd);   // eps_i
  }
  __syncthreads();
  for (int c = threadIdx.x; c < nparam; c += 256)
    scratch[(int64_t)c * gridDim.x + blockIdx.x] = ((accs[0][c] + accs[1][c]) + accs[2][c]) + accs[3][c];
}

// second stage: out[p] = the sum of form p's per-block partials, fixed order; one block per form
__global__ __launch_bounds__(256) void k_hubbard_forms_reduce(const double* __restrict__ scratch, int count,
                                                              double* __restrict__ out) {
  __shared__ double sm5[5];
  const double tot = sum_partials_block(scratch + (int64_t)blockIdx.x * count, count, sm5);
  if (threadIdx.x == 0) out[blockIdx.x] = tot;
}

// C(L, k) for 0 <= k <= L <= 40, exact: C(L - k + i, i) after trip i, below C(40, 20) * 40 < 2^63
static uint64_t hubbard_binomial(int L, int k) {
  if (k > L - k) k = L - k;
  uint64_t c = 1;
  for (int i = 1; i <= k; ++i) c = c * (uint64_t)(L - k + i) / (uint64_t)i;
  return c;
}

// n_up = C(L, nup), n_dn = C(L, ndn), n = n_up n_dn; false outside 2 <= L <= 40, 1 <= nup, ndn <= L - 1, n <= 2^31 - 1
// (host arithmetic only)
bool hubbard_sizes(int L, int nup, int ndn, int64_t* n, int64_t* n_up, int64_t* n_dn) {
  if (L < 2 || L > DSEA_SECTOR_MAX_L || nup < 1 || nup > L - 1 || ndn < 1 || ndn > L - 1) return false;
  const uint64_t cu = hubbard_binomial(L, nup), cd = hubbard_binomial(L, ndn);
  if (cu > 0x7FFFFFFFull || cd > 0x7FFFFFFFull || cu * cd > 0x7FFFFFFFull) return false;   // (the product is below 2^62)
  *n = (int64_t)(cu * cd);
  *n_up = (int64_t)cu;
  *n_dn = (int64_t)cd;
  return true;
}

// one block per 256 rows up to the cap 2^tune_tile_log2 (6 .. 12, 12 at creation: 4096); beyond it blocks walk row ranges
static inline int hubbard_blocks(const OpDesc& op) {
  int64_t nblk = (op.n + 255) / 256;
  const int64_t cap = (int64_t)1 << op.tune_tile_log2;
  if (nblk > cap) nblk = cap;
  return (int)nblk;
}

// the kernel arguments; false when the descriptor is out of range
static bool hubbard_params(const OpDesc& op, HubbardParams* p) {
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
  for (int t = 0; t < DSEA_LATTICE_MAX_BONDS; ++t)
    p->tb[t] = t < d.nb ? (uint16_t)((uint32_t)d.a[t] | ((uint32_t)d.b[t] << 8)) : (uint16_t)0;
  return true;
}

// partials per form that dsea_op_hubbard_forms may write at any grid cap: the largest cap gives the most blocks
int64_t hubbard_forms_scratch_doubles(int64_t n, int L, int nb) {
  int64_t nblk = (n + 255) / 256;
  if (nblk > DSEA_MAX_TFIM_BLOCKS) nblk = DSEA_MAX_TFIM_BLOCKS;
  return (int64_t)(2 * nb + 2 * L) * nblk;
}

int launch_spmv_hubbard(const OpDesc& op, const double* x, double* y, const double* shift, const double* skip, double* P,
                        hipStream_t st, EventPair* ev) {
  HubbardParams p;
  if (!hubbard_params(op, &p)) return -1;
  const int nblk = hubbard_blocks(op);
  klaunch(ev, k_spmv_hubbard, nblk, 256, 0, st, p, x, y, shift, skip, P);
  return nblk;
}

int launch_hubbard_forms(const OpDesc& op, const double* v1, const double* v2, double* out, double* scratch, hipStream_t st) {
  HubbardParams p;
  if (!hubbard_params(op, &p)) return -1;
  const int nblk = hubbard_blocks(op);
  klaunch(nullptr, k_hubbard_forms, nblk, 256, 0, st, p, v1, v2, scratch);
  hipLaunchKernelGGL(k_hubbard_forms_reduce, dim3(2 * p.nb + 2 * p.L), dim3(256), 0, st, scratch, nblk, out);
  return 0;
}

}  // namespace dsea
