// dsea_symsector.hip -- matrix-free XXZ spins on a caller-given bond list in one magnetisation sector, reduced further by a
// lattice-symmetry group G with a real one-dimensional character chi (docs/design/20-symmetry-sector.md): the table builders
// k_symsector_fill_perm / k_symsector_classify / k_symsector_fill_buckets, the mat-vec k_spmv_symsector, the parameter adjoint
// k_symsector_forms (+ k_symsector_forms_reduce), and their launchers.
//
// The Hamiltonian, the bits and the couplings [Jxy(nb), Jz(nb), hz(L)] are those of dsea_sector.hip.  g in G is a permutation
// of the sites, g(s) has bit perm_g[i] set iff s has bit i.  rep(s) = min_g g(s); sigma(s) = sum_{g : g(s) = s} chi(g), which is
// |Stab(s)| or 0.  Row r is the r-th representative with sigma != 0 in increasing integer order, reps[r] = s_r | sigma_r << 48.
// With pbar the couplings averaged over their orbits under G (bond orbits for Jxy and Jz, site orbits for hz) and
// m_t = (1 << a_t) | (1 << b_t):
//   (H x)[r] = ( sum_t Jzbar_t zz_t(s_r) + sum_i hzbar_i z_i(s_r) ) x[r]
//            + sum_{t : bit_a(s_r) != bit_b(s_r)} 2 Jxybar_t chi(g*) sqrt(sigma_j / sigma_r) x[j]
// where g* attains min_g g(s_r ^ m_t) and j is the row of that minimum; the term is dropped when the minimum is no stored
// representative (an orbit with sigma = 0).  g(s ^ m) = g(s) ^ g(m): the |G| images of s_r are formed once per row from
// perm_tab (the image of every byte slice under every g), the hops only XOR the image of the bond mask onto them.
// j is found by a bounded binary search of reps inside [bucket[h], bucket[h + 1]), h = rep >> Llo, Llo = (L + 1) / 2.
// A row belongs to a team of 16 lanes; lane l owns the group elements l, l + 16, ...
// Spin inversion (docs/design/23-spin-inversion.md): an element may also flip every spin, g(s) = perm_g(s) ^ (2^L - 1); the flip
// cancels in g(s ^ m) = g(s) ^ perm_g(m), so only the row's own images and the mean of hz (signed) change.  The bodies of the
// classification, the mat-vec and the forms are written once with a compile-time FLIP flag: the kernels named above instantiate
// them without it, k_symsector_classify_flip / k_spmv_symsector_flip / k_symsector_forms_flip (+ k_symsector_forms_reduce_flip) with.
// Nothing here is shared with dsea_sector.hip: the file has its own helpers.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_internal.h"
#include "dsea_device.h"

namespace dsea {

#define DSEA_SYM_MAX_PARAMS (2 * DSEA_LATTICE_MAX_BONDS + DSEA_SECTOR_MAX_L)
#define DSEA_SYM_TEAM 16                           /* lanes per row: one DPP row */
#define DSEA_SYM_STATE_MASK 0xFFFFFFFFFFFFull      /* reps[r] & mask = s_r, reps[r] >> 48 = sigma_r */
#define DSEA_SYM_FORMS_THREADS 128                 /* k_symsector_forms: 8 teams, so that its accumulators fit LDS beside gmt */

struct SymSectorParams {
  int L, nb, Llo, ng, nsl;                 // nsl = ceil(L / 8) byte slices of a state
  int64_t n;
  const double* c;
  const uint64_t* reps;
  const uint32_t* bucket;
  const uint64_t* perm_tab;                // [ng][nsl][256]
  uint64_t neg[2];                         // bit g: chi(g) = -1
  uint16_t tb[DSEA_LATTICE_MAX_BONDS];     // a | b << 8, the caller's order
  uint16_t orb[DSEA_SYM_MAX_PARAMS];       // orbit id per parameter
};
struct SymOrbits {
  uint16_t orb[DSEA_SYM_MAX_PARAMS];
};
struct SymPerm {
  uint8_t p[DSEA_SECTOR_MAX_L];
};
// Spin inversion (docs/design/23-spin-inversion.md): bit g of flip set when g(s) = perm_g(s) ^ full, full = 2^L - 1; eps[i] in
// {+1, -1, 0}, the sign of site i in the signed orbit mean of hz.  Only the *_flip kernels take it.
struct SymFlip {
  uint32_t flip[4];
  uint64_t full;
  int8_t eps[DSEA_SECTOR_MAX_L];
};
__device__ __forceinline__ uint64_t sym_flip_mask(const SymFlip& f, int g) {
  return ((f.flip[g >> 5] >> (g & 31)) & 1u) ? f.full : 0ull;
}

__device__ __forceinline__ double sym_signed(double v, uint64_t bit) {
  return __longlong_as_double(__double_as_longlong(v) ^ (long long)(bit << 63));
}
__device__ __forceinline__ uint64_t sym_differ(uint64_t s, uint32_t e) { return ((s >> (e & 255u)) ^ (s >> (e >> 8))) & 1ull; }
__device__ __forceinline__ uint64_t sym_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
// the family [f0, f1) of parameter c: Jxy, Jz or hz
__device__ __forceinline__ void sym_family(int c, int nb, int L, int* f0, int* f1) {
  *f0 = c < nb ? 0 : c < 2 * nb ? nb : 2 * nb;
  *f1 = c < nb ? nb : c < 2 * nb ? 2 * nb : 2 * nb + L;
}

// g(s) for the g whose slice tables start at tab: the OR of nsl lookups
__device__ __forceinline__ uint64_t sym_image(const uint64_t* __restrict__ tab, int nsl, uint64_t s) {
  uint64_t im = 0;
#pragma unroll
  for (int sl = 0; sl < (DSEA_SECTOR_MAX_L + 7) / 8; ++sl)
    if (sl < nsl) im |= tab[sl * 256 + (int)((s >> (8 * sl)) & 255ull)];
  return im;
}

// perm_tab[g][sl][byte] = the image under g of the state whose byte slice sl is `byte` and whose other bits are 0; one launch per g
__global__ __launch_bounds__(256) void k_symsector_fill_perm(SymPerm pm, int L, int nsl, uint64_t* __restrict__ out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= nsl * 256) return;
  const int sl = idx >> 8, byte = idx & 255;
  uint64_t v = 0;
  for (int bit = 0; bit < 8; ++bit) {
    const int i = sl * 8 + bit;
    if (i < L && ((byte >> bit) & 1)) v |= 1ull << pm.p[i];
  }
  out[idx] = v;
}

#define DSEA_SYM_PASCAL (DSEA_SECTOR_MAX_L + 1)
// slab[i] = s | sigma << 48 for row first + i of the full sector when its state s is the smallest of its orbit and sigma != 0,
// and 0 otherwise.  The state is unranked in the kernel (the combinatorial number system, as k_sector_fill_states).
// (FLIP: the images of flipped elements are XORed with the full mask)
template <bool FLIP>
__device__ __forceinline__ void sym_classify(const SymFlip& fl, int L, int ndown, int ng, int nsl, uint64_t neg0, uint64_t neg1,
                                             const uint64_t* __restrict__ perm_tab, int64_t first, int64_t count,
                                             uint64_t* __restrict__ slab) {
  __shared__ uint64_t C[DSEA_SYM_PASCAL][DSEA_SYM_PASCAL];
  for (int c = threadIdx.x; c < DSEA_SYM_PASCAL * DSEA_SYM_PASCAL; c += 256) (&C[0][0])[c] = 0;
  __syncthreads();
  for (int i = 0; i <= L; ++i) {
    const int j = threadIdx.x;
    if (j <= i) C[i][j] = (j == 0 || j == i) ? 1 : C[i - 1][j - 1] + C[i - 1][j];
    __syncthreads();
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
    uint64_t rest = (uint64_t)(first + i), s = 0;
    int k = ndown;
    for (int j = L - 1; j >= 0 && k > 0; --j) {
      const uint64_t below = C[j][k];
      if (rest >= below) {
        s |= 1ull << j;
        rest -= below;
        --k;
      }
    }
    bool smallest = true;
    int sigma = 0;
    for (int g = 0; g < ng && smallest; ++g) {
      uint64_t im = sym_image(perm_tab + (int64_t)g * nsl * 256, nsl, s);
      if (FLIP) im ^= sym_flip_mask(fl, g);
      const uint64_t ngb = ((g < 64 ? neg0 >> g : neg1 >> (g - 64)) & 1ull);
      if (im < s) smallest = false;
      if (im == s) sigma += ngb ? -1 : 1;
    }
    slab[i] = (smallest && sigma > 0) ? (s | ((uint64_t)sigma << 48)) : 0ull;
  }
}
__global__ __launch_bounds__(256) void k_symsector_classify(int L, int ndown, int ng, int nsl, uint64_t neg0, uint64_t neg1,
                                                            const uint64_t* __restrict__ perm_tab, int64_t first, int64_t count,
                                                            uint64_t* __restrict__ slab) {
  sym_classify<false>(SymFlip(), L, ndown, ng, nsl, neg0, neg1, perm_tab, first, count, slab);
}
__global__ __launch_bounds__(256) void k_symsector_classify_flip(SymFlip fl, int L, int ndown, int ng, int nsl, uint64_t neg0,
                                                                 uint64_t neg1, const uint64_t* __restrict__ perm_tab,
                                                                 int64_t first, int64_t count, uint64_t* __restrict__ slab) {
  sym_classify<true>(fl, L, ndown, ng, nsl, neg0, neg1, perm_tab, first, count, slab);
}

// bucket[h], 0 <= h <= 2^Lhi: the first row whose state >> Llo is >= h (lower bound in the sorted reps)
__global__ __launch_bounds__(256) void k_symsector_fill_buckets(int Llo, int64_t nh, int64_t n, const uint64_t* __restrict__ reps,
                                                                uint32_t* __restrict__ bucket) {
  for (int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x; h <= nh; h += (int64_t)gridDim.x * 256) {
    const uint64_t target = (uint64_t)h << Llo;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((reps[mid] & DSEA_SYM_STATE_MASK) < target) lo = mid + 1;
      else hi = mid;
    }
    bucket[h] = (uint32_t)lo;
  }
}

// Block prologue shared by the mat-vec and the forms: the bond table, then gp[g][i] = perm_g[i] read back from perm_tab (the
// image of the single bit i), then gmt[t][g] = perm_g[a_t] | perm_g[b_t] << 8 for the ngp = NGL * 16 padded group slots (0 past
// ng).  Ends with a barrier.
__device__ __forceinline__ void sym_stage_group(const SymSectorParams& p, int ngp, uint16_t* tb, uint8_t* gp, uint16_t* gmt) {
  const int L = p.L, nb = p.nb, ng = p.ng, nsl = p.nsl, nt = blockDim.x;
  for (int c = threadIdx.x; c < nb; c += nt) tb[c] = p.tb[c];
  for (int c = threadIdx.x; c < ng * L; c += nt) {
    const int g = c / L, i = c - g * L;
    const uint64_t im = p.perm_tab[((int64_t)g * nsl + (i >> 3)) * 256 + (1 << (i & 7))];
    gp[c] = (uint8_t)(__ffsll((unsigned long long)im) - 1);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < nb * ngp; c += nt) {
    const int t = c / ngp, g = c - t * ngp;
    const uint32_t w = tb[t];
    gmt[c] = g < ng ? (uint16_t)((uint32_t)gp[g * L + (w & 255u)] | ((uint32_t)gp[g * L + (w >> 8)] << 8)) : (uint16_t)0;
  }
  __syncthreads();
}

// The images of the row's state under the lane's NGL group elements (all ones for a slot past ng: its keys never win), and the
// lane's character bits.
template <int NGL, bool FLIP>
__device__ __forceinline__ void sym_images(const SymSectorParams& p, const SymFlip& fl, uint64_t st, int lane16,
                                           uint64_t (&img)[NGL], uint64_t (&ngb)[NGL]) {
#pragma unroll
  for (int k = 0; k < NGL; ++k) {
    const int g = lane16 + DSEA_SYM_TEAM * k;
    img[k] = ~0ull;
    ngb[k] = 0;
    if (g < p.ng) {
      img[k] = sym_image(p.perm_tab + (int64_t)g * p.nsl * 256, p.nsl, st);
      if (FLIP) img[k] ^= sym_flip_mask(fl, g);     // (< 2^L: a padding slot's all-ones image still never wins)
      ngb[k] = (g < 64 ? p.neg[0] >> g : p.neg[1] >> (g - 64)) & 1ull;
    }
  }
}

// One chunk of 16 bonds k0 .. k0 + 15 for the team's row.  Each lane forms, per bond, the minimum over its own group elements of
// key = (g(s_r) ^ g(m_t)) << 1 | (chi(g) < 0); a transposed butterfly over the team (8 + 4 + 2 + 1 exchanges, fixed lanes) leaves
// the team minimum of bond k0 + l in lane l.  The lane then looks its representative up.  Returns true when bond k0 + l flips
// the row and lands on a stored representative: *j its row, *sj its sigma, *neg the sign bit.
template <int NGL>
__device__ __forceinline__ bool sym_hop(const SymSectorParams& p, uint64_t st, const uint64_t (&img)[NGL],
                                        const uint64_t (&ngb)[NGL], int k0, int lane16, const uint16_t* tb, const uint16_t* gmt,
                                        uint32_t* j, uint64_t* sj, uint64_t* neg) {
  const int nb = p.nb, ngp = NGL * DSEA_SYM_TEAM;
  uint64_t key[DSEA_SYM_TEAM];
#pragma unroll
  for (int e = 0; e < DSEA_SYM_TEAM; ++e) {
    const int t = k0 + e < nb ? k0 + e : nb - 1;       // (past the last bond: a key nobody uses)
    uint64_t kmin = ~0ull;
#pragma unroll
    for (int k = 0; k < NGL; ++k) {
      const uint32_t w = gmt[t * ngp + lane16 + DSEA_SYM_TEAM * k];
      const uint64_t gm = (1ull << (w & 255u)) | (1ull << (w >> 8));
      kmin = sym_min(kmin, ((img[k] ^ gm) << 1) | ngb[k]);
    }
    key[e] = kmin;
  }
  const bool b3 = lane16 & 8, b2 = lane16 & 4, b1 = lane16 & 2, b0 = lane16 & 1;
  uint64_t k8[8], k4[4], k2[2];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t keep = b3 ? key[i + 8] : key[i], send = b3 ? key[i] : key[i + 8];
    k8[i] = sym_min(keep, __shfl_xor((unsigned long long)send, 8, DSEA_SYM_TEAM));
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint64_t keep = b2 ? k8[i + 4] : k8[i], send = b2 ? k8[i] : k8[i + 4];
    k4[i] = sym_min(keep, __shfl_xor((unsigned long long)send, 4, DSEA_SYM_TEAM));
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const uint64_t keep = b1 ? k4[i + 2] : k4[i], send = b1 ? k4[i] : k4[i + 2];
    k2[i] = sym_min(keep, __shfl_xor((unsigned long long)send, 2, DSEA_SYM_TEAM));
  }
  const uint64_t keep = b0 ? k2[1] : k2[0], send = b0 ? k2[0] : k2[1];
  const uint64_t best = sym_min(keep, __shfl_xor((unsigned long long)send, 1, DSEA_SYM_TEAM));   // bond k0 + lane16

  const int t = k0 + lane16;
  bool found = false;
  if (t < nb && sym_differ(st, tb[t]) != 0) {
    const uint64_t rep = best >> 1;
    const uint64_t h = rep >> p.Llo;
    uint32_t lo = p.bucket[h];
    const uint32_t end = p.bucket[h + 1];
    uint32_t hi = end;
    for (int it = 0; it <= p.Llo && lo < hi; ++it) {   // (a bucket holds at most 2^Llo rows)
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if ((p.reps[mid] & DSEA_SYM_STATE_MASK) < rep) lo = mid + 1;
      else hi = mid;
    }
    if (lo < end) {
      const uint64_t entry = p.reps[lo];
      if ((entry & DSEA_SYM_STATE_MASK) == rep) {
        found = true;
        *j = lo;
        *sj = entry >> 48;
        *neg = best & 1ull;
      }
    }
  }
  return found;
}

// the team's sum in every lane of the team, fixed order
__device__ __forceinline__ double sym_team_sum(double v) {
  v += __shfl_xor(v, 8, DSEA_SYM_TEAM);
  v += __shfl_xor(v, 4, DSEA_SYM_TEAM);
  v += __shfl_xor(v, 2, DSEA_SYM_TEAM);
  v += __shfl_xor(v, 1, DSEA_SYM_TEAM);
  return v;
}

// y = H x - shift x ; partial x.y per block.  256 threads = 16 teams = 16 rows per range; a block walks the ranges blockIdx.x,
// + gridDim.x, ...  Every block first averages the couplings over their orbits (ascending index order) into LDS.  A team past
// the last row reads row n - 1 and writes nothing.  NGL = group elements per lane (|G| <= 16 NGL).
// FLIP (k_spmv_symsector_flip): the row's images carry the flips and the mean of hz is the signed one, eps_i times the mean of
// eps_j hz_j over the site orbit (0 on an orbit with eps = 0).  Each instantiation is inlined into exactly one kernel, which so
// owns the LDS arrays declared here.
template <int NGL, bool FLIP>
__device__ __forceinline__ void sym_spmv(const SymSectorParams& p, const SymFlip& fl, const double* __restrict__ x,
                                         double* __restrict__ y, const double* __restrict__ shift,
                                         const double* __restrict__ skip, double* __restrict__ P) {
  __shared__ double raw[DSEA_SYM_MAX_PARAMS];
  __shared__ double cp[DSEA_SYM_MAX_PARAMS];
  __shared__ uint16_t orb[DSEA_SYM_MAX_PARAMS];
  __shared__ uint16_t tb[DSEA_LATTICE_MAX_BONDS];
  __shared__ uint8_t gp[DSEA_SYMSECTOR_MAX_GROUP * DSEA_SECTOR_MAX_L];
  __shared__ double sm5[5];
  extern __shared__ __attribute__((aligned(16))) uint16_t gmt[];
  if (skip && skip[0] != 0.0) return;
  const int L = p.L, nb = p.nb, nparam = 2 * nb + L;
  const int64_t n = p.n;
  for (int c = threadIdx.x; c < nparam; c += 256) {
    raw[c] = p.c[c];
    orb[c] = p.orb[c];
  }
  sym_stage_group(p, NGL * DSEA_SYM_TEAM, tb, gp, gmt);      // (its barriers also publish raw and orb)
  for (int c = threadIdx.x; c < nparam; c += 256) {
    int f0, f1, cnt = 0;
    sym_family(c, nb, L, &f0, &f1);
    double sum = 0.0;
    if (FLIP && c >= 2 * nb) {
      for (int m = f0; m < f1; ++m)
        if (orb[m] == orb[c]) {
          sum += (double)fl.eps[m - 2 * nb] * raw[m];
          ++cnt;
        }
      cp[c] = (double)fl.eps[c - 2 * nb] * (sum / (double)cnt);
      continue;
    }
    for (int m = f0; m < f1; ++m)
      if (orb[m] == orb[c]) {
        sum += raw[m];
        ++cnt;
      }
    cp[c] = sum / (double)cnt;
  }
  __syncthreads();
  const double* __restrict__ jxy = cp;
  const double* __restrict__ jzs = cp + nb;
  const double* __restrict__ hzs = cp + 2 * nb;
  const double s = shift ? shift[0] : 0.0;
  const int lane16 = threadIdx.x & (DSEA_SYM_TEAM - 1), team = threadIdx.x >> 4;
  double acc = 0.0;
  for (int64_t row0 = (int64_t)blockIdx.x * 16; row0 < n; row0 += (int64_t)gridDim.x * 16) {
    const int64_t r = row0 + team;
    const bool have = r < n;
    const uint64_t entry = p.reps[have ? r : n - 1];
    const uint64_t st = entry & DSEA_SYM_STATE_MASK;
    const double sr = (double)(entry >> 48);
    const double xr = x[have ? r : n - 1];
    uint64_t img[NGL], ngb[NGL];
    sym_images<NGL, FLIP>(p, fl, st, lane16, img, ngb);
    double diag = 0.0, sum = 0.0;
    for (int k0 = 0; k0 < nb; k0 += DSEA_SYM_TEAM) {
      uint32_t j = 0;
      uint64_t sj = 1, neg = 0;
      const bool hop = sym_hop<NGL>(p, st, img, ngb, k0, lane16, tb, gmt, &j, &sj, &neg);
      const int t = k0 + lane16;
      if (t < nb) diag += sym_signed(jzs[t], sym_differ(st, tb[t]));
      if (hop) sum = fma(sym_signed(2.0 * jxy[t] * sqrt((double)sj / sr), neg), x[j], sum);
    }
    for (int i = lane16; i < L; i += DSEA_SYM_TEAM) diag += sym_signed(hzs[i], (st >> i) & 1ull);
    double v = sym_team_sum(fma(diag, xr, sum));
    if (shift) v = __dsub_rn(v, __dmul_rn(s, xr));
    if (have && lane16 == 0) {
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
template <int NGL>
__global__ __launch_bounds__(256) void k_spmv_symsector(SymSectorParams p, const double* __restrict__ x, double* __restrict__ y,
                                                        const double* __restrict__ shift, const double* __restrict__ skip,
                                                        double* __restrict__ P) {
  sym_spmv<NGL, false>(p, SymFlip(), x, y, shift, skip, P);
}
template <int NGL>
__global__ __launch_bounds__(256) void k_spmv_symsector_flip(SymSectorParams p, SymFlip fl, const double* __restrict__ x,
                                                             double* __restrict__ y, const double* __restrict__ shift,
                                                             const double* __restrict__ skip, double* __restrict__ P) {
  sym_spmv<NGL, true>(p, fl, x, y, shift, skip, P);
}

// The raw forms: raw[t] = v1^T A_t v2 with A_t the coefficient matrix of pbar_t in the row formula,
//   Jxy_t: sum_{r : hop} 2 chi sqrt(sigma_j / sigma_r) v1[r] v2[j]     Jz_t: sum_r zz_t v1[r] v2[r]     hz_i: sum_r z_i v1[r] v2[r]
// Same row walk, 128 threads = 8 teams.  Every (team, term) accumulator in LDS has exactly one owning lane (bond t: lane t mod 16,
// site i: lane i mod 16), so there are no atomics; the 8 rows are added in fixed order into scratch[t * gridDim.x + block].
template <int NGL, bool FLIP>
__device__ __forceinline__ void sym_forms(const SymSectorParams& p, const SymFlip& fl, const double* __restrict__ v1,
                                          const double* __restrict__ v2, double* __restrict__ scratch) {
  constexpr int TEAMS = DSEA_SYM_FORMS_THREADS / DSEA_SYM_TEAM;
  __shared__ double accs[TEAMS][DSEA_SYM_MAX_PARAMS];
  __shared__ uint16_t tb[DSEA_LATTICE_MAX_BONDS];
  __shared__ uint8_t gp[DSEA_SYMSECTOR_MAX_GROUP * DSEA_SECTOR_MAX_L];
  extern __shared__ __attribute__((aligned(16))) uint16_t gmt[];
  const int L = p.L, nb = p.nb, nparam = 2 * nb + L;
  const int64_t n = p.n;
  for (int c = threadIdx.x; c < TEAMS * DSEA_SYM_MAX_PARAMS; c += DSEA_SYM_FORMS_THREADS) (&accs[0][0])[c] = 0.0;
  sym_stage_group(p, NGL * DSEA_SYM_TEAM, tb, gp, gmt);
  const int lane16 = threadIdx.x & (DSEA_SYM_TEAM - 1), team = threadIdx.x >> 4;
  double* __restrict__ mine = accs[team];
  for (int64_t row0 = (int64_t)blockIdx.x * TEAMS; row0 < n; row0 += (int64_t)gridDim.x * TEAMS) {
    const int64_t r = row0 + team;
    const bool have = r < n;                       // a team without a row adds zeros to every form
    const uint64_t entry = p.reps[have ? r : n - 1];
    const uint64_t st = entry & DSEA_SYM_STATE_MASK;
    const double sr = (double)(entry >> 48);
    const double a = have ? v1[r] : 0.0;
    const double d = a * v2[have ? r : n - 1];
    uint64_t img[NGL], ngb[NGL];
    sym_images<NGL, FLIP>(p, fl, st, lane16, img, ngb);
    for (int k0 = 0; k0 < nb; k0 += DSEA_SYM_TEAM) {
      uint32_t j = 0;
      uint64_t sj = 1, neg = 0;
      const bool hop = sym_hop<NGL>(p, st, img, ngb, k0, lane16, tb, gmt, &j, &sj, &neg);
      const int t = k0 + lane16;
      if (t < nb) mine[nb + t] += sym_signed(d, sym_differ(st, tb[t]));
      if (hop) mine[t] += sym_signed(2.0 * sqrt((double)sj / sr), neg) * (a * v2[j]);
    }
    for (int i = lane16; i < L; i += DSEA_SYM_TEAM) mine[2 * nb + i] += sym_signed(d, (st >> i) & 1ull);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < nparam; c += DSEA_SYM_FORMS_THREADS) {
    double tot = accs[0][c];
#pragma unroll
    for (int w = 1; w < TEAMS; ++w) tot += accs[w][c];
    scratch[(int64_t)c * gridDim.x + blockIdx.x] = tot;
  }
}
template <int NGL>
__global__ __launch_bounds__(DSEA_SYM_FORMS_THREADS) void k_symsector_forms(SymSectorParams p, const double* __restrict__ v1,
                                                                            const double* __restrict__ v2,
                                                                            double* __restrict__ scratch) {
  sym_forms<NGL, false>(p, SymFlip(), v1, v2, scratch);
}
template <int NGL>
__global__ __launch_bounds__(DSEA_SYM_FORMS_THREADS) void k_symsector_forms_flip(SymSectorParams p, SymFlip fl,
                                                                                 const double* __restrict__ v1,
                                                                                 const double* __restrict__ v2,
                                                                                 double* __restrict__ scratch) {
  sym_forms<NGL, true>(p, fl, v1, v2, scratch);
}

// second stage: out[t] = the mean over t's orbit of the raw forms (that is S): the per-block partials of every member of the
// orbit, members in ascending order, each summed in fixed order; one block per output, so the members of one orbit get identical
// bits
__global__ __launch_bounds__(256) void k_symsector_forms_reduce(SymOrbits o, int L, int nb, const double* __restrict__ scratch,
                                                                int count, double* __restrict__ out) {
  __shared__ double sm5[5];
  const int c = blockIdx.x;
  int f0, f1, cnt = 0;
  sym_family(c, nb, L, &f0, &f1);
  const uint16_t mine = o.orb[c];
  double tot = 0.0;
  for (int m = f0; m < f1; ++m)
    if (o.orb[m] == mine) {
      tot += sum_partials_block(scratch + (int64_t)m * count, count, sm5);
      ++cnt;
    }
  if (threadIdx.x == 0) out[c] = tot / (double)cnt;
}
// the same with the signed sum for the hz outputs: eps_c / |orbit| times the sum of eps_m raw_m, so the members of an orbit get
// bits that are identical up to the sign and an eps = 0 output is exactly 0.0
__global__ __launch_bounds__(256) void k_symsector_forms_reduce_flip(SymOrbits o, SymFlip fl, int L, int nb,
                                                                     const double* __restrict__ scratch, int count,
                                                                     double* __restrict__ out) {
  __shared__ double sm5[5];
  const int c = blockIdx.x;
  int f0, f1, cnt = 0;
  sym_family(c, nb, L, &f0, &f1);
  const uint16_t mine = o.orb[c];
  const bool site = c >= 2 * nb;
  double tot = 0.0;
  for (int m = f0; m < f1; ++m)
    if (o.orb[m] == mine) {
      const double part = sum_partials_block(scratch + (int64_t)m * count, count, sm5);
      tot += site ? (double)fl.eps[m - 2 * nb] * part : part;
      ++cnt;
    }
  if (threadIdx.x == 0) {
    const double mean = tot / (double)cnt;
    const int e = site ? fl.eps[c - 2 * nb] : 1;
    out[c] = e == 0 ? 0.0 : (double)e * mean;
  }
}

// n_sector = C(L, ndown), the bucket count 2^Lhi + 1 and the words of perm_tab; false outside the limits of sector_sizes or
// 1 <= ng <= DSEA_SYMSECTOR_MAX_GROUP (host arithmetic only)
bool symsector_sizes(int L, int ndown, int ng, int64_t* n_sector, int64_t* n_bucket, int64_t* n_perm) {
  int64_t n, n_lo, n_hi;
  if (!sector_sizes(L, ndown, &n, &n_lo, &n_hi) || ng < 1 || ng > DSEA_SYMSECTOR_MAX_GROUP) return false;
  *n_sector = n;
  *n_bucket = n_hi + 1;
  *n_perm = (int64_t)ng * ((L + 7) / 8) * 256;
  return true;
}

// the flips and the site signs of a handle made by dsea_op_create_symsector_flip
static SymFlip sym_flip(const SymSectorDesc& d) {
  SymFlip fl = {};
  for (int w = 0; w < 4; ++w) fl.flip[w] = d.flip[w];
  fl.full = (1ull << d.L) - 1ull;
  for (int i = 0; i < d.L; ++i) fl.eps[i] = d.eps[i];
  return fl;
}

static inline int sym_ngl(int ng) { return ng <= 16 ? 1 : ng <= 32 ? 2 : ng <= 64 ? 4 : 8; }

// one block per `rows` rows up to the cap 2^tune_tile_log2 (6 .. 12, 12 at creation); beyond it blocks walk row ranges
static inline int sym_blocks(const OpDesc& op, int rows) {
  int64_t nblk = (op.n + rows - 1) / rows;
  const int64_t cap = (int64_t)1 << op.tune_tile_log2;
  if (nblk > cap) nblk = cap;
  return (int)nblk;
}

// the kernel arguments; false when the descriptor is out of range
static bool sym_params(const OpDesc& op, SymSectorParams* p) {
  const SymSectorDesc& d = op.symsector;
  int64_t n_sector, n_bucket, n_perm;
  if (!symsector_sizes(d.L, d.ndown, d.ng, &n_sector, &n_bucket, &n_perm) || op.n < 1 || op.n > n_sector) return false;
  if (d.nb < 1 || d.nb > DSEA_LATTICE_MAX_BONDS || op.tune_tile_log2 < 6 || op.tune_tile_log2 > 12) return false;
  if (!d.c || !d.reps || !d.bucket || !d.perm_tab) return false;
  p->L = d.L;
  p->nb = d.nb;
  p->Llo = (d.L + 1) / 2;
  p->ng = d.ng;
  p->nsl = (d.L + 7) / 8;
  p->n = op.n;
  p->c = d.c;
  p->reps = d.reps;
  p->bucket = d.bucket;
  p->perm_tab = d.perm_tab;
  p->neg[0] = d.neg[0];
  p->neg[1] = d.neg[1];
  for (int t = 0; t < DSEA_LATTICE_MAX_BONDS; ++t)
    p->tb[t] = t < d.nb ? (uint16_t)((uint32_t)d.a[t] | ((uint32_t)d.b[t] << 8)) : (uint16_t)0;
  for (int c = 0; c < DSEA_SYM_MAX_PARAMS; ++c) p->orb[c] = c < 2 * d.nb + d.L ? d.orb[c] : (uint16_t)0;
  return true;
}

// partials per form that dsea_op_symsector_forms may write at any grid cap
int64_t symsector_forms_scratch_doubles(int64_t n, int L, int nb) {
  const int rows = DSEA_SYM_FORMS_THREADS / DSEA_SYM_TEAM;
  int64_t nblk = (n + rows - 1) / rows;
  if (nblk > DSEA_MAX_TFIM_BLOCKS) nblk = DSEA_MAX_TFIM_BLOCKS;
  return (int64_t)(2 * nb + L) * nblk;
}

int launch_symsector_fill_perm(int L, int ng, const int32_t* perms_host, uint64_t* perm_tab, hipStream_t st) {
  const int nsl = (L + 7) / 8;
  for (int g = 0; g < ng; ++g) {
    SymPerm pm;
    for (int i = 0; i < DSEA_SECTOR_MAX_L; ++i) pm.p[i] = i < L ? (uint8_t)perms_host[g * L + i] : (uint8_t)0;
    hipLaunchKernelGGL(k_symsector_fill_perm, dim3(nsl), dim3(256), 0, st, pm, L, nsl, perm_tab + (int64_t)g * nsl * 256);
  }
  return 0;
}

int launch_symsector_classify(int L, int ndown, int ng, const uint64_t neg[2], const uint64_t* perm_tab, int64_t first,
                              int64_t count, uint64_t* slab, hipStream_t st) {
  hipLaunchKernelGGL(k_symsector_classify, dim3((unsigned)ew_blocks(count * 8)), dim3(256), 0, st, L, ndown, ng, (L + 7) / 8,
                     neg[0], neg[1], perm_tab, first, count, slab);
  return 0;
}

int launch_symsector_classify_flip(int L, int ndown, int ng, const uint64_t neg[2], const uint32_t flip[4], const uint64_t* perm_tab,
                                   int64_t first, int64_t count, uint64_t* slab, hipStream_t st) {
  SymFlip fl = {};
  for (int w = 0; w < 4; ++w) fl.flip[w] = flip[w];
  fl.full = (1ull << L) - 1ull;
  hipLaunchKernelGGL(k_symsector_classify_flip, dim3((unsigned)ew_blocks(count * 8)), dim3(256), 0, st, fl, L, ndown, ng,
                     (L + 7) / 8, neg[0], neg[1], perm_tab, first, count, slab);
  return 0;
}

int launch_symsector_fill_buckets(int L, int64_t n_rep, const uint64_t* reps, uint32_t* bucket, hipStream_t st) {
  const int Llo = (L + 1) / 2;
  const int64_t nh = (int64_t)1 << (L - Llo);
  hipLaunchKernelGGL(k_symsector_fill_buckets, dim3((unsigned)ew_blocks((nh + 1) * 8)), dim3(256), 0, st, Llo, nh, n_rep, reps,
                     bucket);
  return 0;
}

int launch_spmv_symsector(const OpDesc& op, const double* x, double* y, const double* shift, const double* skip, double* P,
                          hipStream_t st, EventPair* ev) {
  SymSectorParams p;
  if (!sym_params(op, &p)) return -1;
  const int nblk = sym_blocks(op, 256 / DSEA_SYM_TEAM);
  const bool flipped = op.symsector.has_flip != 0;
  const SymFlip fl = sym_flip(op.symsector);
  dispatch_int<1, 2, 4, 8>(sym_ngl(p.ng), [&](auto ngl) {
    constexpr int NGL = decltype(ngl)::value;
    const size_t lds = (size_t)p.nb * NGL * DSEA_SYM_TEAM * sizeof(uint16_t);
    if (flipped) klaunch(ev, k_spmv_symsector_flip<NGL>, nblk, 256, lds, st, p, fl, x, y, shift, skip, P);
    else klaunch(ev, k_spmv_symsector<NGL>, nblk, 256, lds, st, p, x, y, shift, skip, P);
  });
  return nblk;
}

int launch_symsector_forms(const OpDesc& op, const double* v1, const double* v2, double* out, double* scratch, hipStream_t st) {
  SymSectorParams p;
  if (!sym_params(op, &p)) return -1;
  const int nblk = sym_blocks(op, DSEA_SYM_FORMS_THREADS / DSEA_SYM_TEAM);
  const bool flipped = op.symsector.has_flip != 0;
  const SymFlip fl = sym_flip(op.symsector);
  dispatch_int<1, 2, 4, 8>(sym_ngl(p.ng), [&](auto ngl) {
    constexpr int NGL = decltype(ngl)::value;
    const size_t lds = (size_t)p.nb * NGL * DSEA_SYM_TEAM * sizeof(uint16_t);
    if (flipped) klaunch(nullptr, k_symsector_forms_flip<NGL>, nblk, DSEA_SYM_FORMS_THREADS, lds, st, p, fl, v1, v2, scratch);
    else klaunch(nullptr, k_symsector_forms<NGL>, nblk, DSEA_SYM_FORMS_THREADS, lds, st, p, v1, v2, scratch);
  });
  SymOrbits o;
  for (int c = 0; c < DSEA_SYM_MAX_PARAMS; ++c) o.orb[c] = p.orb[c];
  if (flipped)
    hipLaunchKernelGGL(k_symsector_forms_reduce_flip, dim3(2 * p.nb + p.L), dim3(256), 0, st, o, fl, p.L, p.nb, scratch, nblk, out);
  else
    hipLaunchKernelGGL(k_symsector_forms_reduce, dim3(2 * p.nb + p.L), dim3(256), 0, st, o, p.L, p.nb, scratch, nblk, out);
  return 0;
}

}  // namespace dsea
