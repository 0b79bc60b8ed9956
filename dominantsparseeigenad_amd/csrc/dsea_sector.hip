// dsea_sector.hip -- matrix-free XXZ spins on a caller-given bond list, restricted to one magnetisation sector
// (docs/design/18-spin-sector.md): the table builders k_sector_fill_states / k_sector_fill_lo / k_sector_fill_hi, the mat-vec
// k_spmv_sector, the parameter adjoint k_sector_forms (+ k_sector_forms_reduce), and their launchers.
//
//   H = sum_t [ Jxy_t (X_a X_b + Y_a Y_b) + Jz_t Z_a Z_b ] + sum_i hz_i Z_i,  bond t joins sites a_t != b_t,
// on the states s with exactly ndown set bits (site i = bit i of s, z_i(s) = 1 - 2 bit_i(s)).  Row r is the r-th such state in
// increasing integer order, states[r]; n = C(L, ndown) <= 2^31 - 1.  With m_t = (1 << a_t) | (1 << b_t):
//   (H x)[r] = ( sum_t Jz_t zz_t(s_r) + sum_i hz_i z_i(s_r) ) x[r] + sum_{t : bit_a(s_r) != bit_b(s_r)} 2 Jxy_t x[rank(s_r ^ m_t)]
// rank(s) = hi_base[s >> Llo] + lo_rank[s & (2^Llo - 1)], Llo = (L + 1) / 2 (Lin's two tables): lo_rank[p] is the rank of p among
// the Llo-bit patterns of its popcount, hi_base[h] the number of sector states below h << Llo.  s ^ m_t keeps the popcount, so
// the mat-vec needs no validity test.  The couplings are one device array [Jxy(nb), Jz(nb), hz(L)], copied into LDS by every
// block on every launch; the bond table travels by value in the kernel arguments, in the caller's order.
// Nothing here is shared with dsea_lattice.hip: the file has its own helpers.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_internal.h"
#include "dsea_device.h"

namespace dsea {

#define DSEA_SECTOR_MAX_PARAMS (2 * DSEA_LATTICE_MAX_BONDS + DSEA_SECTOR_MAX_L)
#define DSEA_SECTOR_CHUNK 8          /* bonds whose table lookups and gathers a thread keeps in flight together */
#define DSEA_SECTOR_NO_RANK 0xFFFFFFFFu /* "this bond does not flip this row" (a rank is below 2^31) */

struct SectorParams {
  int L, nb, Llo;
  int64_t n;
  const double* c;
  const uint64_t* states;
  const uint32_t* lo_rank;
  const uint32_t* hi_base;
  uint16_t tb[DSEA_LATTICE_MAX_BONDS];   // a | b << 8, the caller's order
};

// v * (1 - 2 bit), exact: the bit goes into the sign
__device__ __forceinline__ double sector_signed(double v, uint64_t bit) {
  return __longlong_as_double(__double_as_longlong(v) ^ (long long)(bit << 63));
}
__device__ __forceinline__ uint64_t sector_differ(uint64_t s, uint32_t e) { return ((s >> (e & 255u)) ^ (s >> (e >> 8))) & 1ull; }
__device__ __forceinline__ uint64_t sector_mask(uint32_t e) { return (1ull << (e & 255u)) | (1ull << (e >> 8)); }

// Pascal's triangle C[i][j] = C(i, j), 0 <= j <= i <= L, zero above the diagonal, filled by the block (L <= 40: C(40, 20) fits 64 bits)
#define DSEA_SECTOR_PASCAL (DSEA_SECTOR_MAX_L + 1)
__device__ __forceinline__ void sector_pascal(uint64_t (*C)[DSEA_SECTOR_PASCAL], int L) {
  for (int c = threadIdx.x; c < DSEA_SECTOR_PASCAL * DSEA_SECTOR_PASCAL; c += blockDim.x) (&C[0][0])[c] = 0;
  __syncthreads();
  for (int i = 0; i <= L; ++i) {
    const int j = threadIdx.x;
    if (j <= i) C[i][j] = (j == 0 || j == i) ? 1 : C[i - 1][j - 1] + C[i - 1][j];
    __syncthreads();
  }
}

// states[r] = the r-th L-bit word with ndown set bits in increasing order: the combinatorial number system, r = sum_i C(p_i, i)
// over the positions p_1 < ... < p_k of the set bits, unranked greedily from the top bit
__global__ __launch_bounds__(256) void k_sector_fill_states(int L, int ndown, int64_t n, uint64_t* __restrict__ states) {
  __shared__ uint64_t C[DSEA_SECTOR_PASCAL][DSEA_SECTOR_PASCAL];
  sector_pascal(C, L);
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
    uint64_t rest = (uint64_t)r, s = 0;
    int k = ndown;
    for (int j = L - 1; j >= 0 && k > 0; --j) {
      const uint64_t below = C[j][k];      // sector words of k bits that fit under bit j
      if (rest >= below) {
        s |= 1ull << j;
        rest -= below;
        --k;
      }
    }
    states[r] = s;
  }
}

// lo_rank[p], 0 <= p < 2^Llo: the rank of p among the Llo-bit words of its popcount
__global__ __launch_bounds__(256) void k_sector_fill_lo(int Llo, uint32_t* __restrict__ lo_rank) {
  __shared__ uint64_t C[DSEA_SECTOR_PASCAL][DSEA_SECTOR_PASCAL];
  sector_pascal(C, Llo);
  const int64_t count = (int64_t)1 << Llo;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < count; p += (int64_t)gridDim.x * 256) {
    uint64_t rank = 0;
    int i = 0;
    for (int j = 0; j < Llo; ++j)
      if ((p >> j) & 1) rank += C[j][++i];
    lo_rank[p] = (uint32_t)rank;
  }
}

// hi_base[h], 0 <= h < 2^Lhi: the number of sector states below h << Llo; 0 for an h that no sector state has.  For every set
// bit j of h, with c set bits of h above it: the words that share those c bits, have bit j clear, and place the other
// ndown - c bits anywhere in the j + Llo positions below.
__global__ __launch_bounds__(256) void k_sector_fill_hi(int L, int ndown, int Llo, uint32_t* __restrict__ hi_base) {
  __shared__ uint64_t C[DSEA_SECTOR_PASCAL][DSEA_SECTOR_PASCAL];
  sector_pascal(C, L);
  const int Lhi = L - Llo;
  const int64_t count = (int64_t)1 << Lhi;
  for (int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x; h < count; h += (int64_t)gridDim.x * 256) {
    const int left = ndown - __popcll((uint64_t)h);     // bits the low part has to hold
    uint64_t base = 0;
    if (left >= 0 && left <= Llo) {
      int c = 0;
      for (int j = Lhi - 1; j >= 0; --j)
        if ((h >> j) & 1) {
          if (ndown - c >= 0) base += C[j + Llo][ndown - c];
          ++c;
        }
    }
    hi_base[h] = (uint32_t)base;
  }
}

// the ranks of the partner rows of bonds k0 .. k0 + CHUNK - 1 for the row with state s: two table reads per bond that flips the
// row, all requested before any is used; DSEA_SECTOR_NO_RANK for a bond that does not flip it (and past the last bond)
__device__ __forceinline__ void sector_ranks(uint32_t (&rk)[DSEA_SECTOR_CHUNK], uint64_t s, bool have, int k0, int nb, int Llo,
                                             const uint16_t* tb, const uint32_t* __restrict__ lo_rank,
                                             const uint32_t* __restrict__ hi_base) {
  const uint64_t lomask = (1ull << Llo) - 1;
#pragma unroll
  for (int e = 0; e < DSEA_SECTOR_CHUNK; ++e) {
    const uint32_t w = k0 + e < nb ? tb[k0 + e] : 0u;
    const bool on = have && k0 + e < nb && sector_differ(s, w) != 0;
    const uint64_t s2 = s ^ sector_mask(w);
    rk[e] = DSEA_SECTOR_NO_RANK;
    if (on) rk[e] = hi_base[s2 >> Llo] + lo_rank[s2 & lomask];
  }
}
// the gathers of one chunk: v[rank], 0 where the bond does not flip the row
__device__ __forceinline__ void sector_gather(double (&xv)[DSEA_SECTOR_CHUNK], const uint32_t (&rk)[DSEA_SECTOR_CHUNK],
                                              const double* __restrict__ v) {
#pragma unroll
  for (int e = 0; e < DSEA_SECTOR_CHUNK; ++e) {
    xv[e] = 0.0;
    if (rk[e] != DSEA_SECTOR_NO_RANK) xv[e] = v[rk[e]];
  }
}

// y = H x - shift x ; partial x.y per block.  One row per thread: states, x and y are read and written coalesced; a bond whose
// two bits differ in the row costs two table reads and one gather of x.  The table reads of chunk c + 1 are issued before the
// gathers of chunk c are consumed.  A block walks the row ranges blockIdx.x, + gridDim.x, ... of 256 rows.
__global__ __launch_bounds__(256) void k_spmv_sector(SectorParams p, const double* __restrict__ x, double* __restrict__ y,
                                                     const double* __restrict__ shift, const double* __restrict__ skip,
                                                     double* __restrict__ P) {
  __shared__ double cp[DSEA_SECTOR_MAX_PARAMS];
  __shared__ uint16_t tb[DSEA_LATTICE_MAX_BONDS];
  __shared__ double sm5[5];
  if (skip && skip[0] != 0.0) return;
  const int L = p.L, nb = p.nb, Llo = p.Llo;
  const int64_t n = p.n;
  for (int c = threadIdx.x; c < 2 * nb + L; c += 256) cp[c] = p.c[c];
  for (int c = threadIdx.x; c < nb; c += 256) tb[c] = p.tb[c];
  __syncthreads();
  const double* __restrict__ jxy = cp;
  const double* __restrict__ jzs = cp + nb;
  const double* __restrict__ hzs = cp + 2 * nb;
  const double s = shift ? shift[0] : 0.0;
  double acc = 0.0;
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;                       // (a thread past the last row reads row n - 1 and writes nothing)
    const uint64_t st = p.states[have ? r : n - 1];
    const double xr = x[have ? r : n - 1];
    uint32_t rkA[DSEA_SECTOR_CHUNK], rkB[DSEA_SECTOR_CHUNK];
    sector_ranks(rkA, st, have, 0, nb, Llo, tb, p.lo_rank, p.hi_base);
    double diag = 0.0, sum = 0.0;
    for (int i = 0; i < L; ++i) diag += sector_signed(hzs[i], (st >> i) & 1ull);
    for (int k0 = 0; k0 < nb; k0 += DSEA_SECTOR_CHUNK) {
      double xv[DSEA_SECTOR_CHUNK];
      sector_gather(xv, rkA, x);
      sector_ranks(rkB, st, have, k0 + DSEA_SECTOR_CHUNK, nb, Llo, tb, p.lo_rank, p.hi_base);
#pragma unroll
      for (int e = 0; e < DSEA_SECTOR_CHUNK; ++e) {
        if (k0 + e < nb) {
          diag += sector_signed(jzs[k0 + e], sector_differ(st, tb[k0 + e]));
          sum = fma(2.0 * jxy[k0 + e], xv[e], sum);
        }
        rkA[e] = rkB[e];
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

// The parameter adjoint: all 2 nb + L bilinear forms out[t] = v1^T (dH/dp_t) v2 in one pass over v1 and v2 (t in the order of
// the couplings: Jxy_t, Jz_t, hz_i):
//   Jxy_t: sum_{r : bits differ} 2 v1[r] v2[rank(s_r ^ m_t)]     Jz_t: sum_r zz_t v1[r] v2[r]     hz_i: sum_r z_i v1[r] v2[r]
// Same row walk and the same chunks of lookups and gathers (of v2) as the mat-vec.  No per-lane accumulator per term: every
// term is reduced through the wave at once (wave_sum, fixed order) and lane 0 adds it to the wave's row of LDS accumulators; the
// four rows are added in fixed order and written to scratch[t * gridDim.x + block].  No atomics.
__global__ __launch_bounds__(256) void k_sector_forms(SectorParams p, const double* __restrict__ v1,
                                                      const double* __restrict__ v2, double* __restrict__ scratch) {
  __shared__ double accs[4][DSEA_SECTOR_MAX_PARAMS];
  __shared__ uint16_t tb[DSEA_LATTICE_MAX_BONDS];
  const int L = p.L, nb = p.nb, Llo = p.Llo;
  const int nparam = 2 * nb + L;
  const int64_t n = p.n;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double* __restrict__ mine = accs[wv];
  for (int c = lane; c < nparam; c += 64) mine[c] = 0.0;   // (afterwards a wave's row is touched by its lane 0 alone)
  for (int c = threadIdx.x; c < nb; c += 256) tb[c] = p.tb[c];
  __syncthreads();
  auto add = [&](int term, double val) {
    const double tot = wave_sum(val);
    if (lane == 0) mine[term] += tot;
  };
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;                       // a thread without a row adds zeros to every form
    const uint64_t st = p.states[have ? r : n - 1];
    const double a = have ? v1[r] : 0.0;
    const double d = a * v2[have ? r : n - 1];
    uint32_t rkA[DSEA_SECTOR_CHUNK], rkB[DSEA_SECTOR_CHUNK];
    sector_ranks(rkA, st, have, 0, nb, Llo, tb, p.lo_rank, p.hi_base);
    for (int k0 = 0; k0 < nb; k0 += DSEA_SECTOR_CHUNK) {
      double xv[DSEA_SECTOR_CHUNK];
      sector_gather(xv, rkA, v2);
      sector_ranks(rkB, st, have, k0 + DSEA_SECTOR_CHUNK, nb, Llo, tb, p.lo_rank, p.hi_base);
#pragma unroll
      for (int e = 0; e < DSEA_SECTOR_CHUNK; ++e) {
        if (k0 + e < nb) {                         // (the same for every lane: the wave sums run with all lanes)
          add(k0 + e, 2.0 * (a * xv[e]));                                         // Jxy_t
          add(nb + k0 + e, sector_signed(d, sector_differ(st, tb[k0 + e])));      // Jz_t
        }
        rkA[e] = rkB[e];
      }
    }
    for (int i = 0; i < L; ++i) add(2 * nb + i, sector_signed(d, (st >> i) & 1ull));   // hz_i
  }
  __syncthreads();
  for (int c = threadIdx.x; c < nparam; c += 256)
    scratch[(int64_t)c * gridDim.x + blockIdx.x] = ((accs[0][c] + accs[1][c]) + accs[2][c]) + accs[3][c];
}

// second stage: out[t] = the sum of term t's per-block partials, fixed order; one block per term
__global__ __launch_bounds__(256) void k_sector_forms_reduce(const double* __restrict__ scratch, int count,
                                                             double* __restrict__ out) {
  __shared__ double sm5[5];
  const double tot = sum_partials_block(scratch + (int64_t)blockIdx.x * count, count, sm5);
  if (threadIdx.x == 0) out[blockIdx.x] = tot;
}

// n = C(L, ndown), 2^Llo, 2^Lhi; false outside 2 <= L <= 40, 1 <= ndown <= L - 1, n <= 2^31 - 1 (host arithmetic only)
bool sector_sizes(int L, int ndown, int64_t* n, int64_t* n_lo, int64_t* n_hi) {
  if (L < 2 || L > DSEA_SECTOR_MAX_L || ndown < 1 || ndown > L - 1) return false;
  uint64_t c = 1;                                  // C(L - k + i, i) after trip i: exact, and below C(40, 20) * 40 < 2^63
  const int k = ndown < L - ndown ? ndown : L - ndown;
  for (int i = 1; i <= k; ++i) c = c * (uint64_t)(L - k + i) / (uint64_t)i;
  if (c > 0x7FFFFFFFull) return false;
  const int Llo = (L + 1) / 2;
  *n = (int64_t)c;
  *n_lo = (int64_t)1 << Llo;
  *n_hi = (int64_t)1 << (L - Llo);
  return true;
}

// one block per 256 rows up to the cap 2^tune_tile_log2 (6 .. 12, 12 at creation: 4096); beyond it blocks walk row ranges
static inline int sector_blocks(const OpDesc& op) {
  int64_t nblk = (op.n + 255) / 256;
  const int64_t cap = (int64_t)1 << op.tune_tile_log2;
  if (nblk > cap) nblk = cap;
  return (int)nblk;
}

// the kernel arguments; false when the descriptor is out of range
static bool sector_params(const OpDesc& op, SectorParams* p) {
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

// partials per form that dsea_op_sector_forms may write at any grid cap: the largest cap gives the most blocks
int64_t sector_forms_scratch_doubles(int64_t n, int L, int nb) {
  int64_t nblk = (n + 255) / 256;
  if (nblk > DSEA_MAX_TFIM_BLOCKS) nblk = DSEA_MAX_TFIM_BLOCKS;
  return (int64_t)(2 * nb + L) * nblk;
}

int launch_sector_build_tables(int L, int ndown, uint64_t* states, uint32_t* lo_rank, uint32_t* hi_base, hipStream_t st) {
  int64_t n, n_lo, n_hi;
  if (!sector_sizes(L, ndown, &n, &n_lo, &n_hi)) return -1;
  const int Llo = (L + 1) / 2;
  hipLaunchKernelGGL(k_sector_fill_states, dim3((unsigned)ew_blocks(n * 8)), dim3(256), 0, st, L, ndown, n, states);
  hipLaunchKernelGGL(k_sector_fill_lo, dim3((unsigned)ew_blocks(n_lo * 8)), dim3(256), 0, st, Llo, lo_rank);
  hipLaunchKernelGGL(k_sector_fill_hi, dim3((unsigned)ew_blocks(n_hi * 8)), dim3(256), 0, st, L, ndown, Llo, hi_base);
  return 0;
}

int launch_spmv_sector(const OpDesc& op, const double* x, double* y, const double* shift, const double* skip, double* P,
                       hipStream_t st, EventPair* ev) {
  SectorParams p;
  if (!sector_params(op, &p)) return -1;
  const int nblk = sector_blocks(op);
  klaunch(ev, k_spmv_sector, nblk, 256, 0, st, p, x, y, shift, skip, P);
  return nblk;
}

int launch_sector_forms(const OpDesc& op, const double* v1, const double* v2, double* out, double* scratch, hipStream_t st) {
  SectorParams p;
  if (!sector_params(op, &p)) return -1;
  const int nblk = sector_blocks(op);
  klaunch(nullptr, k_sector_forms, nblk, 256, 0, st, p, v1, v2, scratch);
  hipLaunchKernelGGL(k_sector_forms_reduce, dim3(2 * p.nb + p.L), dim3(256), 0, st, scratch, nblk, out);
  return 0;
}

}  // namespace dsea
