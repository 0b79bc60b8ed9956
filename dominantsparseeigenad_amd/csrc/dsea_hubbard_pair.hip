// dsea_hubbard_pair.hip -- linear maps between two particle-number sectors of the Hubbard space of the same L sites that move one
// particle of EACH species in one pass (docs/design/41-hubbard-pair-ladder.md): the pair map k_hubbard_pair<SU, SD>, its
// site-pair forms k_hubbard_pair_forms<SU, SD> (+ k_hubbard_pair_forms_reduce), and their launchers.
//
// Conventions of docs/design/19-hubbard.md and of dsea_hubbard_ladder.hip: the words u, d; |u, d> = (prod_{i in u, ascending}
// c+_{i up}) (prod_{j in d, ascending} c+_{j dn}) |0>; row r = ru * n_dn + rd; below_i = (1 << i) - 1, par(w) = popcount(w) & 1.
// With steps (SU, SD) in {+1, -1}^2, A = c+ for SU = +1 and c for SU = -1, B likewise for SD, and a weight matrix W (fp64 [L, L]
// row-major, read through its device pointer on every launch), order 0 is P = sum_ij W_ij A_{i up} B_{j dn} from (nup, ndn) to
// (nup + SU, ndn + SD); (u', d') are the words of the destination row:
//   y[ru' n_dn_dst + rd'] = g sum_{i qualifies in u'} sum_{j qualifies in d'} W_ij (-1)^par(u' & below_i) (-1)^par(d' & below_j)
//                             x[rank_up_src(u' ^ (1 << i)) n_dn_src + rank_dn_src(d' ^ (1 << j))]
// A site qualifies when its bit is set in the destination word for a step of +1 and clear for -1.  g = (-1)^nup_src: the down
// operator passes the nup_src up operators of the source state.  Order 1, sum_ij W_ij B_{j dn} A_{i up}, is the same sum with g
// negated.  The transpose of (SU, SD, order) from src to dst is (-SU, -SD, 1 - order) from dst to src, entry for entry.
// A gather over the destination rows: no scatter, no atomic.  The terms are added i ascending outer, j ascending inner, with
// fma and the sign folded into the weight (block_signed, exact).
//
// The number of qualifying sites of a word is the same for every row (the count of the destination for a step of +1, L minus
// it for -1): md of the down word, mu of the up word, and a row has mu md terms.  A thread resolves its md down partners once
// -- two own-table reads and one table read per qualifying site -- and keeps them as (source rank | sign << 31, site) slots in
// LDS laid out [slot][thread]: a column is private to its thread (no barrier), consecutive lanes hit consecutive banks, and no
// register array is indexed dynamically.  It then walks its up partners; each gives a stripe base rank_up_src n_dn_src and the
// md gathers from that stripe, four in flight, with W_ij from an LDS copy of W.
// The device helpers are the file's own: nothing is shared with dsea_hubbard_ladder.hip but the host rules of dsea_internal.h.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_internal.h"
#include "dsea_device.h"
#include "dsea_block.h"

namespace dsea {

namespace {
#ifndef DSEA_HPAIR_CHUNK            /* (an A/B build may set it: make libdsea_<name>.so EXTRA=-DDSEA_HPAIR_CHUNK=8) */
#define DSEA_HPAIR_CHUNK 4          /* table reads of the site walk, and gathers of a stripe, a thread keeps in flight together */
#endif
#define DSEA_HPAIR_NONE 0xFFFFFFFFu /* "this site does not contribute to this row" (a rank is below 2^31 - 1) */

// one species of a pair map: the state table at its destination count and the two rank tables at its source count
struct HubbardPairSpecies {
  const uint64_t* states;
  const uint32_t* lo_rank;
  const uint32_t* hi_base;
};
struct HubbardPairParams {
  int L, Llo;
  int md;                        // qualifying sites of a down word of the destination: slots of a thread
  uint32_t n_dn_dst, n_dn_src;   // the row strides of the destination and of the source
  uint32_t g;                    // the starting parity: (nup_src + order) & 1
  int64_t n;                     // rows of the destination
  const double* W;               // the L x L weights (null for the forms)
  HubbardPairSpecies up, dn;
};

__device__ __forceinline__ uint32_t hpair_bit(uint64_t w, int i) { return (uint32_t)((w >> i) & 1ull); }
template <int STEP>
__device__ __forceinline__ bool hpair_qualifies(uint64_t w, int i) {
  return hpair_bit(w, i) == (STEP > 0 ? 1u : 0u);
}

// The site walk of one species' word w of a destination row: use(i, on, rank, par) for every site i = 0 .. L - 1 in ascending
// order, the same calls in every lane.  on: the site qualifies; rank: the source rank of w ^ (1 << i) (undefined when !on);
// par: par0 ^ par(w & below_i), a running parity.  rank_src(v) = hi_base[v >> Llo] + lo_rank[v & lomask]: flipping one bit
// changes one of the two words, so the row reads its own two entries once and a site costs one table read, requested a chunk
// at a time before any is used.  A table is read only for a qualifying site, where the index is a word of the source count.
template <int STEP, typename Use>
__device__ __forceinline__ void hpair_walk(uint64_t w, int L, int Llo, const HubbardPairSpecies& sp, uint32_t par0, Use use) {
  const uint32_t wl = (uint32_t)(w & ((1ull << Llo) - 1)), wh = (uint32_t)(w >> Llo);
  const uint32_t own_hi = sp.hi_base[wh], own_lo = sp.lo_rank[wl];
  uint32_t par = par0;
  for (int k0 = 0; k0 < L; k0 += DSEA_HPAIR_CHUNK) {
    uint32_t tv[DSEA_HPAIR_CHUNK];
    uint32_t on = 0;
#pragma unroll
    for (int e = 0; e < DSEA_HPAIR_CHUNK; ++e) {
      const int i = k0 + e;
      tv[e] = 0;
      if (i < L && hpair_qualifies<STEP>(w, i)) {     // (i < 40: the shifts are defined)
        tv[e] = i < Llo ? sp.lo_rank[wl ^ (1u << i)] : sp.hi_base[wh ^ (1u << (i - Llo))];
        on |= 1u << e;
      }
    }
#pragma unroll
    for (int e = 0; e < DSEA_HPAIR_CHUNK; ++e) {
      const int i = k0 + e;
      if (i < L) {                                    // (the same for every lane)
        use(i, ((on >> e) & 1u) != 0, (i < Llo ? own_hi : own_lo) + tv[e], par);
        par ^= hpair_bit(w, i);
      }
    }
  }
}

// (u', d') of the destination row rr by one 32-bit division with the stride of the destination
struct HubbardPairRow {
  uint64_t u, d;
};
__device__ __forceinline__ HubbardPairRow hpair_row(const HubbardPairParams& p, uint32_t rr) {
  const uint32_t ru = rr / p.n_dn_dst, rd = rr - ru * p.n_dn_dst;
  HubbardPairRow q;
  q.u = p.up.states[ru];
  q.d = p.dn.states[rd];
  return q;
}
}  // namespace

// y = P(W) x.  One destination row per thread; a block walks the row ranges blockIdx.x, + gridDim.x, ... of 256 rows; a thread
// past the last row works on row n - 1 (reads only) and writes nothing.  Dynamic LDS: W [L * L] doubles, the slot ranks
// [md][256] uint32, the slot sites [md][256] bytes.
template <int SU, int SD>
__global__ __launch_bounds__(256) void k_hubbard_pair(HubbardPairParams p, const double* __restrict__ x, double* __restrict__ y) {
  extern __shared__ double hpair_lds[];
  const int L = p.L, Llo = p.Llo, md = p.md;
  double* __restrict__ Wl = hpair_lds;
  uint32_t* __restrict__ srank = reinterpret_cast<uint32_t*>(Wl + L * L) + threadIdx.x;
  uint8_t* __restrict__ ssite = reinterpret_cast<uint8_t*>(reinterpret_cast<uint32_t*>(Wl + L * L) + md * 256) + threadIdx.x;
  for (int c = threadIdx.x; c < L * L; c += 256) Wl[c] = p.W[c];
  __syncthreads();
  const int64_t n = p.n;
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;
    const HubbardPairRow q = hpair_row(p, (uint32_t)(have ? r : n - 1));
    int cnt = 0;                                     // (reaches md in every thread)
    hpair_walk<SD>(q.d, L, Llo, p.dn, 0u, [&](int j, bool on, uint32_t rank, uint32_t par) {
      if (on && cnt < md) {
        srank[cnt * 256] = rank | (par << 31);
        ssite[cnt * 256] = (uint8_t)j;
        ++cnt;
      }
    });
    double sum = 0.0;
    hpair_walk<SU>(q.u, L, Llo, p.up, p.g, [&](int i, bool on, uint32_t rank, uint32_t par) {
      if (!on) return;
      const double* __restrict__ xs = x + (int64_t)rank * p.n_dn_src;     // the stripe of this up partner
      const double* __restrict__ wrow = Wl + i * L;
      for (int k0 = 0; k0 < md; k0 += DSEA_HPAIR_CHUNK) {
        uint32_t s[DSEA_HPAIR_CHUNK];
        double xv[DSEA_HPAIR_CHUNK], wv[DSEA_HPAIR_CHUNK];
#pragma unroll
        for (int e = 0; e < DSEA_HPAIR_CHUNK; ++e) {
          if (k0 + e < md) {                          // (the same for every lane)
            s[e] = srank[(k0 + e) * 256];
            wv[e] = wrow[ssite[(k0 + e) * 256]];
            xv[e] = xs[s[e] & 0x7FFFFFFFu];
          }
        }
#pragma unroll
        for (int e = 0; e < DSEA_HPAIR_CHUNK; ++e)
          if (k0 + e < md) sum = fma(block_signed(wv[e], par ^ (s[e] >> 31)), xv[e], sum);
      }
    });
    if (have) y[r] = sum;
  }
}

// The site-pair forms: out[i * L + j] = v1^T (dP/dW_ij) v2 = g sum_{rows : i qualifies in u', j in d'} (+-) v1[row] v2[partner row]
// for all L^2 pairs in one pass, v1 on the destination and v2 on the source.  The same row walk; the down partners of a thread
// are kept for ALL L sites (DSEA_HPAIR_NONE where the site does not qualify), since a form is a sum over the lanes of one site.
// Every term is reduced through the wave at once (wave_sum, fixed order; skipped for a site pair no lane of the wave has), the
// four waves' totals of the up site i are staged and added in fixed order into the block's L^2 accumulators, which go to
// scratch[(i * L + j) * gridDim.x + block] at the end.  No atomics: repeated calls return identical bits.  Dynamic LDS: the
// accumulators [L * L] and the stage [4][L] doubles, the slots [L][256] uint32.  Every barrier is reached by all threads: the
// site walk makes the same calls in every lane.
template <int SU, int SD>
__global__ __launch_bounds__(256) void k_hubbard_pair_forms(HubbardPairParams p, const double* __restrict__ v1,
                                                            const double* __restrict__ v2, double* __restrict__ scratch) {
  extern __shared__ double hpair_lds[];
  const int L = p.L, Llo = p.Llo;
  double* __restrict__ acc = hpair_lds;
  double* __restrict__ stage = acc + L * L;
  uint32_t* __restrict__ slot = reinterpret_cast<uint32_t*>(stage + 4 * L) + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = threadIdx.x; c < L * L; c += 256) acc[c] = 0.0;
  const int64_t n = p.n;
  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < n; row0 += (int64_t)gridDim.x * 256) {
    const int64_t r = row0 + threadIdx.x;
    const bool have = r < n;                          // a thread without a row adds zeros to every form
    const uint32_t rr = (uint32_t)(have ? r : n - 1);
    const HubbardPairRow q = hpair_row(p, rr);
    const double a = have ? v1[rr] : 0.0;
    hpair_walk<SD>(q.d, L, Llo, p.dn, 0u, [&](int j, bool on, uint32_t rank, uint32_t par) {
      slot[j * 256] = on ? rank | (par << 31) : DSEA_HPAIR_NONE;
    });
    hpair_walk<SU>(q.u, L, Llo, p.up, p.g, [&](int i, bool on, uint32_t rank, uint32_t par) {
      const bool any_up = __ballot(on) != 0ull;       // (the same for every lane of the wave)
      const double* __restrict__ xs = v2 + (on ? (int64_t)rank * p.n_dn_src : 0);
      for (int j0 = 0; j0 < L; j0 += DSEA_HPAIR_CHUNK) {
        uint32_t s[DSEA_HPAIR_CHUNK];
        double xv[DSEA_HPAIR_CHUNK];
#pragma unroll
        for (int e = 0; e < DSEA_HPAIR_CHUNK; ++e) {
          s[e] = DSEA_HPAIR_NONE;
          xv[e] = 0.0;
          if (any_up && j0 + e < L) {
            s[e] = on ? slot[(j0 + e) * 256] : DSEA_HPAIR_NONE;
            if (s[e] != DSEA_HPAIR_NONE) xv[e] = xs[s[e] & 0x7FFFFFFFu];
          }
        }
#pragma unroll
        for (int e = 0; e < DSEA_HPAIR_CHUNK; ++e) {
          if (j0 + e < L) {                           // (the same for every lane)
            double tot = 0.0;
            if (__ballot(s[e] != DSEA_HPAIR_NONE) != 0ull)
              tot = wave_sum(a * block_signed(xv[e], (par ^ (s[e] >> 31)) & 1u));
            if (lane == 0) stage[wave * L + j0 + e] = tot;
          }
        }
      }
      __syncthreads();
      for (int j = threadIdx.x; j < L; j += 256)
        acc[i * L + j] += ((stage[j] + stage[L + j]) + stage[2 * L + j]) + stage[3 * L + j];
      __syncthreads();
    });
  }
  __syncthreads();
  for (int c = threadIdx.x; c < L * L; c += 256) scratch[(int64_t)c * gridDim.x + blockIdx.x] = acc[c];
}

// second stage: out[i * L + j] = the sum of the pair's per-block partials, fixed order; one block per form
__global__ __launch_bounds__(256) void k_hubbard_pair_forms_reduce(const double* __restrict__ scratch, int count,
                                                                   double* __restrict__ out) {
  __shared__ double sm5[5];
  const double tot = sum_partials_block(scratch + (int64_t)blockIdx.x * count, count, sm5);
  if (threadIdx.x == 0) out[blockIdx.x] = tot;
}

// the rows and the down strides of the two sectors; false when a step is not +-1, order is outside {0, 1} or either sector is
// outside the limits of hubbard_sizes (host arithmetic only)
bool hubbard_pair_sizes(int L, int nup_src, int ndn_src, int step_up, int step_dn, int order, int64_t* n_src, int64_t* n_dst,
                        int64_t* n_dn_src, int64_t* n_dn_dst) {
  int64_t n_up;
  if ((step_up != 1 && step_up != -1) || (step_dn != 1 && step_dn != -1) || order < 0 || order > 1) return false;
  return hubbard_sizes(L, nup_src, ndn_src, n_src, &n_up, n_dn_src) &&
         hubbard_sizes(L, nup_src + step_up, ndn_src + step_dn, n_dst, &n_up, n_dn_dst);
}

// the kernel arguments (W: the weights, null for the forms); false when an argument is out of range
static bool hubbard_pair_params(int L, int nup_src, int ndn_src, int step_up, int step_dn, int order, int grid_log2,
                                const double* W, const void* const tables[6], HubbardPairParams* p) {
  int64_t n_src, n_dst, n_dn_src, n_dn_dst;
  if (!hubbard_pair_sizes(L, nup_src, ndn_src, step_up, step_dn, order, &n_src, &n_dst, &n_dn_src, &n_dn_dst)) return false;
  if (!ladder_grid_ok(grid_log2)) return false;
  for (int t = 0; t < 6; ++t)
    if (!tables[t]) return false;
  const int ndn_dst = ndn_src + step_dn;
  p->L = L;
  p->Llo = (L + 1) / 2;
  p->md = step_dn > 0 ? ndn_dst : L - ndn_dst;
  p->n_dn_dst = (uint32_t)n_dn_dst;
  p->n_dn_src = (uint32_t)n_dn_src;
  p->g = (uint32_t)((nup_src + order) & 1);
  p->n = n_dst;
  p->W = W;
  p->up.states = static_cast<const uint64_t*>(tables[0]);
  p->up.lo_rank = static_cast<const uint32_t*>(tables[1]);
  p->up.hi_base = static_cast<const uint32_t*>(tables[2]);
  p->dn.states = static_cast<const uint64_t*>(tables[3]);
  p->dn.lo_rank = static_cast<const uint32_t*>(tables[4]);
  p->dn.hi_base = static_cast<const uint32_t*>(tables[5]);
  return true;
}

// the dynamic LDS of the two kernels (at most 62720 and 55040 bytes, at L = 40)
static inline size_t hubbard_pair_apply_lds(const HubbardPairParams& p) {
  return (size_t)p.L * p.L * sizeof(double) + (size_t)p.md * 256 * (sizeof(uint32_t) + sizeof(uint8_t));
}
static inline size_t hubbard_pair_forms_lds(const HubbardPairParams& p) {
  return ((size_t)p.L * p.L + 4 * (size_t)p.L) * sizeof(double) + (size_t)p.L * 256 * sizeof(uint32_t);
}

// the one place that turns the run-time (step_up, step_dn) of a launch into template arguments: f(int_c<SU>, int_c<SD>), -1 for
// anything but +1 (hubbard_pair_params has refused the rest)
template <class F>
static inline void hubbard_pair_dispatch(int step_up, int step_dn, F&& f) {
  dispatch_int<1, -1>(step_up, [&](auto su) { dispatch_int<1, -1>(step_dn, [&](auto sd) { f(su, sd); }); });
}

int launch_hubbard_pair(int L, int nup_src, int ndn_src, int step_up, int step_dn, int order, const double* W,
                        const void* const tables[6], const double* x, double* y, int grid_log2, hipStream_t st) {
  HubbardPairParams p;
  if (!W || !hubbard_pair_params(L, nup_src, ndn_src, step_up, step_dn, order, grid_log2, W, tables, &p)) return -1;
  const dim3 grid((unsigned)ladder_blocks(p.n, grid_log2));
  const size_t lds = hubbard_pair_apply_lds(p);
  hubbard_pair_dispatch(step_up, step_dn, [&](auto su, auto sd) {
    hipLaunchKernelGGL((k_hubbard_pair<decltype(su)::value, decltype(sd)::value>), grid, dim3(256), lds, st, p, x, y);
  });
  return 0;
}

int launch_hubbard_pair_forms(int L, int nup_src, int ndn_src, int step_up, int step_dn, int order,
                              const void* const tables[6], const double* v1, const double* v2, double* out, double* scratch,
                              int grid_log2, hipStream_t st) {
  HubbardPairParams p;
  if (!hubbard_pair_params(L, nup_src, ndn_src, step_up, step_dn, order, grid_log2, nullptr, tables, &p)) return -1;
  const int nblk = ladder_blocks(p.n, grid_log2);
  const dim3 grid((unsigned)nblk);
  const size_t lds = hubbard_pair_forms_lds(p);
  hubbard_pair_dispatch(step_up, step_dn, [&](auto su, auto sd) {
    hipLaunchKernelGGL((k_hubbard_pair_forms<decltype(su)::value, decltype(sd)::value>), grid, dim3(256), lds, st, p, v1, v2,
                       scratch);
  });
  hipLaunchKernelGGL(k_hubbard_pair_forms_reduce, dim3((unsigned)(L * L)), dim3(256), 0, st, scratch, nblk, out);
  return 0;
}

}  // namespace dsea
