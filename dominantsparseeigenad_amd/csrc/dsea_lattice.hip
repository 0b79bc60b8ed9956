// dsea_lattice.hip -- matrix-free XYZ spins on a caller-given bond list (docs/design/16-spin-lattice.md): the mat-vec
// k_spmv_lattice, the parameter adjoint k_lattice_forms (+ k_lattice_forms_reduce), and their launchers.
//
//   H = sum_t [ Jx_t X_a X_b + Jy_t Y_a Y_b + Jz_t Z_a Z_b ] + sum_i [ hx_i X_i + hz_i Z_i ],  bond t joins sites a_t != b_t
// Site i is bit i of the row index s, z_i(s) = 1 - 2 bit_i(s), m_t = (1 << a_t) | (1 << b_t), zz_t = z_a z_b:
//   (H x)[s] = ( sum_t Jz_t zz_t(s) + sum_i hz_i z_i(s) ) x[s] + sum_i hx_i x[s ^ (1 << i)]
//            + sum_t ( Jx_t - Jy_t zz_t(s) ) x[s ^ m_t]
// The couplings are one device array [Jx(nb), Jy(nb), Jz(nb), hx(L), hz(L)]; every block copies it into LDS on every launch
// (wave-uniform broadcast reads afterwards): no host copy, in-place optimiser steps are seen.  The bond table travels by value
// in the kernel arguments, sorted by the host for the tile of this launch: the bonds with both sites inside the tile first,
// then the far ones; every entry carries the caller's bond index, so couplings and forms keep the caller's order.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_internal.h"
#include "dsea_device.h"

namespace dsea {

#define DSEA_LATTICE_MAX_L 62
#define DSEA_LATTICE_MAX_PARAMS (3 * DSEA_LATTICE_MAX_BONDS + 2 * DSEA_LATTICE_MAX_L)

struct LatticeParams {
  int L, nb;
  int n_in;          // tb[0 .. n_in): both sites below the tile's T bits; tb[n_in .. nb): a site at or above T
  const double* c;
  uint32_t tb[DSEA_LATTICE_MAX_BONDS];   // a | b << 8 | (the caller's bond index) << 16
};

// v * (1 - 2 bit), exact: the bit goes into the sign
__device__ __forceinline__ double lattice_signed(double v, uint64_t bit) {
  return __longlong_as_double(__double_as_longlong(v) ^ (long long)(bit << 63));
}
__device__ __forceinline__ double2 lattice_swap_if(double2 v, bool swap) { return swap ? make_double2(v.y, v.x) : v; }

// One off-diagonal term as the kernels use it.  A row pair (i0, i0 | 1) has its partner pair at i0 ^ mask (bit 0 of the mask
// cleared), with the pair's two elements swapped when the term flips site 0.  zz of the pair's first row is
// 1 - 2 (bit_a ^ bit_b)(i0); the second row differs in site 0 only, so its bit is flipped exactly when the bond holds site 0.
// A field term is written as a = b = its site: zz bit 0, never swapped beyond site 0's own flip.
struct LatticeTerm {
  int64_t mask;
  int a, b;
  int idx;       // bond: the caller's bond index; field term: the site
  bool bond;
  bool swap;
};
__device__ __forceinline__ LatticeTerm lattice_bond(uint32_t e) {
  LatticeTerm f;
  f.a = (int)(e & 255u);
  f.b = (int)((e >> 8) & 255u);
  f.idx = (int)(e >> 16);
  f.mask = (((int64_t)1 << f.a) | ((int64_t)1 << f.b)) & ~(int64_t)1;
  f.bond = true;
  f.swap = (f.a == 0) || (f.b == 0);
  return f;
}
// The terms whose partner row lies outside the tile of 2^T rows, numbered k = 0 .. nf - 1:
//   k <  nfx = L - T : field term hx_i, i = T + k
//   k >= nfx         : bond tb[n_in + (k - nfx)] (a site at or above T; the other one anywhere)
__device__ __forceinline__ LatticeTerm lattice_far_term(int k, int nfx, int T, int n_in, const uint32_t* tb) {
  if (k >= nfx) return lattice_bond(tb[n_in + (k - nfx)]);
  LatticeTerm f;
  f.a = f.b = f.idx = T + k;
  f.mask = (int64_t)1 << (T + k);
  f.bond = false;
  f.swap = false;
  return f;
}
__device__ __forceinline__ uint64_t lattice_zz_bit(uint64_t row, int a, int b) { return ((row >> a) ^ (row >> b)) & 1ull; }

// the far pairs of terms k0 .. k0 + CH - 1 of every row pair of this thread: all requested before any is consumed
template <int PER, int CH, int NPAIR>
__device__ __forceinline__ void lattice_far_load(double2 (&buf)[PER][CH], const double* __restrict__ x, int64_t base, int k0,
                                                 int nf, int nfx, int T, int n_in, const uint32_t* tb) {
#pragma unroll
  for (int e = 0; e < CH; ++e) {
    const bool on = k0 + e < nf;
    const int64_t mask = on ? lattice_far_term(k0 + e, nfx, T, n_in, tb).mask : 0;
#pragma unroll
    for (int t = 0; t < PER; ++t) {
      const int lp = t * 256 + threadIdx.x;
      const int64_t i0 = base + 2 * (int64_t)(lp < NPAIR ? lp : 0);
      buf[t][e] = make_double2(0.0, 0.0);
      if (on) buf[t][e] = *reinterpret_cast<const double2*>(x + (i0 ^ mask));
    }
  }
}

// y = H x - shift x ; partial x.y per block.  The tile scheme of the chain mat-vec: a block stages 2^T rows of x in LDS, a
// thread owns PER row pairs; a bond with both sites below T is an LDS read of pair lp ^ (m >> 1), every other bond and the
// L - T high field flips are coalesced 16-byte global reads issued a chunk of terms ahead of their use.
template <int T>
__global__ __launch_bounds__(256) void k_spmv_lattice(LatticeParams p, const double* __restrict__ x, double* __restrict__ y,
                                                      const double* __restrict__ shift, const double* __restrict__ skip,
                                                      double* __restrict__ P) {
  constexpr int TILE = 1 << T;
  constexpr int NPAIR = TILE / 2;
  constexpr int PER = (NPAIR + 255) / 256;
  constexpr int CH = PER >= 8 ? 1 : (PER >= 4 ? 2 : 4);   // far terms per buffer (two buffers): <= 64 VGPRs each
  __shared__ double2 tile2[NPAIR];
  __shared__ double cp[DSEA_LATTICE_MAX_PARAMS];
  __shared__ uint32_t tb[DSEA_LATTICE_MAX_BONDS];
  __shared__ double sm5[5];
  if (skip && skip[0] != 0.0) return;
  const int L = p.L, nb = p.nb, n_in = p.n_in;
  const int64_t ntiles = ((int64_t)1 << L) >> T;
  const int nfx = L - T;                     // (T <= L: the launcher takes the whole vector as the tile when L is smaller)
  const int nf = nfx + (nb - n_in);
  for (int c = threadIdx.x; c < 3 * nb + 2 * L; c += 256) cp[c] = p.c[c];
  for (int c = threadIdx.x; c < nb; c += 256) tb[c] = p.tb[c];
  const double* __restrict__ jxs = cp;
  const double* __restrict__ jys = cp + nb;
  const double* __restrict__ jzs = cp + 2 * nb;
  const double* __restrict__ hxs = cp + 3 * nb;
  const double* __restrict__ hzs = cp + 3 * nb + L;
  const double s = shift ? shift[0] : 0.0;
  double acc = 0.0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base = tile * TILE;
    double ownx[PER], owny[PER];
#pragma unroll
    for (int t = 0; t < PER; ++t) {
      const int lp = t * 256 + threadIdx.x;
      const double2 v = *reinterpret_cast<const double2*>(x + base + 2 * (int64_t)(lp < NPAIR ? lp : 0));
      ownx[t] = v.x;
      owny[t] = v.y;
    }
    __syncthreads();  // the couplings and the bond table are in LDS; the previous tile's LDS reads are done
    double2 bufA[PER][CH], bufB[PER][CH];
    lattice_far_load<PER, CH, NPAIR>(bufA, x, base, 0, nf, nfx, T, n_in, tb);
#pragma unroll
    for (int t = 0; t < PER; ++t) {
      const int lp = t * 256 + threadIdx.x;
      if (lp < NPAIR) tile2[lp] = make_double2(ownx[t], owny[t]);
    }
    __syncthreads();
    double sumx[PER], sumy[PER], dgx[PER], dgy[PER];   // off-diagonal sums and the diagonal of the thread's rows
#pragma unroll
    for (int t = 0; t < PER; ++t) sumx[t] = sumy[t] = dgx[t] = dgy[t] = 0.0;
    // one bond or far field term on every row pair of the thread; pv(t): the partner pair as loaded
    auto term = [&](const LatticeTerm& f, auto&& pv) {
      const double ca = f.bond ? jxs[f.idx] : hxs[f.idx];
      const double cb = f.bond ? jys[f.idx] : 0.0;
      const double cz = f.bond ? jzs[f.idx] : 0.0;
#pragma unroll
      for (int t = 0; t < PER; ++t) {
        const int lp = t * 256 + threadIdx.x;
        const uint64_t r0 = (uint64_t)(base + 2 * (int64_t)(lp < NPAIR ? lp : 0));
        const uint64_t b0 = lattice_zz_bit(r0, f.a, f.b), b1 = b0 ^ (uint64_t)f.swap;
        const double2 v = lattice_swap_if(pv(t), f.swap);
        sumx[t] = fma(ca - lattice_signed(cb, b0), v.x, sumx[t]);
        sumy[t] = fma(ca - lattice_signed(cb, b1), v.y, sumy[t]);
        dgx[t] += lattice_signed(cz, b0);
        dgy[t] += lattice_signed(cz, b1);
      }
    };
    // out-of-tile terms, CH at a time through two buffers: the next chunk is requested before this one is consumed
    auto consume = [&](const double2 (&buf)[PER][CH], int k0) {
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        if (k0 + e < nf) term(lattice_far_term(k0 + e, nfx, T, n_in, tb), [&](int t) { return buf[t][e]; });
      }
    };
    for (int k0 = 0; k0 < nf; k0 += 2 * CH) {
      lattice_far_load<PER, CH, NPAIR>(bufB, x, base, k0 + CH, nf, nfx, T, n_in, tb);   // (past the last term: zeros, no loads)
      consume(bufA, k0);
      lattice_far_load<PER, CH, NPAIR>(bufA, x, base, k0 + 2 * CH, nf, nfx, T, n_in, tb);
      consume(bufB, k0 + CH);
    }
    // bonds inside the tile: LDS pair lp ^ (m >> 1)
#pragma unroll 1
    for (int q = 0; q < n_in; ++q) {
      const LatticeTerm f = lattice_bond(tb[q]);
      const int px = (int)(((1u << f.a) | (1u << f.b)) >> 1);
      term(f, [&](int t) {
        const int lp = t * 256 + threadIdx.x;
        return tile2[(lp < NPAIR ? lp : 0) ^ px];
      });
    }
    // field terms inside the tile (site 0: the other element of the pair) and the hz part of the diagonal
    // (two sites per trip: unrolled over all T the PER * T pair reads in flight cost more registers than the far buffers)
#pragma unroll 2
    for (int i = 0; i < T; ++i) {
      const double hx = hxs[i];
#pragma unroll
      for (int t = 0; t < PER; ++t) {
        const int lp = t * 256 + threadIdx.x;
        const double2 v = lattice_swap_if(tile2[(lp < NPAIR ? lp : 0) ^ ((1 << i) >> 1)], i == 0);
        sumx[t] = fma(hx, v.x, sumx[t]);
        sumy[t] = fma(hx, v.y, sumy[t]);
      }
    }
    for (int i = 0; i < L; ++i) {
      const double hz = hzs[i];
#pragma unroll
      for (int t = 0; t < PER; ++t) {
        const int lp = t * 256 + threadIdx.x;
        const uint64_t r0 = (uint64_t)(base + 2 * (int64_t)(lp < NPAIR ? lp : 0));
        dgx[t] += lattice_signed(hz, (r0 >> i) & 1ull);
        dgy[t] += lattice_signed(hz, ((r0 | 1ull) >> i) & 1ull);
      }
    }
#pragma unroll
    for (int t = 0; t < PER; ++t) {
      const int lp = t * 256 + threadIdx.x;
      if (lp < NPAIR) {
        const int64_t i0 = base + 2 * (int64_t)lp;
        const double2 xv = tile2[lp];
        double2 v;
        v.x = fma(dgx[t], xv.x, sumx[t]);
        v.y = fma(dgy[t], xv.y, sumy[t]);
        if (shift) {
          v.x = __dsub_rn(v.x, __dmul_rn(s, xv.x));
          v.y = __dsub_rn(v.y, __dmul_rn(s, xv.y));
        }
        *reinterpret_cast<double2*>(y + i0) = v;
        acc = fma(xv.x, v.x, acc);
        acc = fma(xv.y, v.y, acc);
      }
    }
  }
  if (P) {
    __syncthreads();
    double tot = block_sum(acc, sm5);
    if (threadIdx.x == 0) P[blockIdx.x] = tot;
  }
}

// The parameter adjoint: all 3 nb + 2 L bilinear forms out[t] = v1^T (dH/dp_t) v2 in one pass over v1 and v2 (t in the order
// of the couplings: Jx_t, Jy_t, Jz_t, hx_i, hz_i):
//   Jz_t: sum_s zz_t v1[s] v2[s]          hz_i: sum_s z_i v1[s] v2[s]          hx_i: sum_s v1[s] v2[s ^ (1 << i)]
//   Jx_t: sum_s v1[s] v2[s ^ m_t]         Jy_t: -sum_s zz_t v1[s] v2[s ^ m_t]
// Same tiling as the mat-vec (v2 staged in LDS, far pairs of v2 a chunk of terms ahead).  No per-lane accumulator per term:
// every term is reduced through the wave at once (wave_sum, fixed order) and lane 0 adds it to the wave's row of LDS
// accumulators; the four rows are added in fixed order and written to scratch[t * gridDim.x + block].  No atomics.
template <int T>
__global__ __launch_bounds__(256) void k_lattice_forms(LatticeParams p, const double* __restrict__ v1,
                                                       const double* __restrict__ v2, double* __restrict__ scratch) {
  constexpr int TILE = 1 << T;
  constexpr int NPAIR = TILE / 2;
  constexpr int PER = (NPAIR + 255) / 256;
  constexpr int CH = PER >= 8 ? 1 : (PER >= 4 ? 2 : 4);
  __shared__ double2 tile2[NPAIR];
  __shared__ double accs[4][DSEA_LATTICE_MAX_PARAMS];
  __shared__ uint32_t tb[DSEA_LATTICE_MAX_BONDS];
  const int L = p.L, nb = p.nb, n_in = p.n_in;
  const int nparam = 3 * nb + 2 * L;
  const int64_t ntiles = ((int64_t)1 << L) >> T;
  const int nfx = L - T;
  const int nf = nfx + (nb - n_in);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double* __restrict__ mine = accs[wv];
  for (int c = lane; c < nparam; c += 64) mine[c] = 0.0;   // (afterwards a wave's row is touched by its lane 0 alone)
  for (int c = threadIdx.x; c < nb; c += 256) tb[c] = p.tb[c];
  __syncthreads();
  auto add = [&](int term, double val) {
    const double tot = wave_sum(val);
    if (lane == 0) mine[term] += tot;
  };
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base = tile * TILE;
    double ax[PER], ay[PER], dx[PER], dy[PER];      // v1 of the thread's rows, and v1[s] v2[s]
    double ownx[PER], owny[PER];
#pragma unroll
    for (int t = 0; t < PER; ++t) {
      const int lp = t * 256 + threadIdx.x;
      const int64_t i0 = base + 2 * (int64_t)(lp < NPAIR ? lp : 0);
      const double2 a = *reinterpret_cast<const double2*>(v1 + i0);
      const double2 o = *reinterpret_cast<const double2*>(v2 + i0);
      const bool have = lp < NPAIR;                         // a thread without a pair adds zeros to every form
      ax[t] = have ? a.x : 0.0;
      ay[t] = have ? a.y : 0.0;
      ownx[t] = o.x;
      owny[t] = o.y;
      dx[t] = ax[t] * o.x;
      dy[t] = ay[t] * o.y;
    }
    double2 bufA[PER][CH], bufB[PER][CH];
    lattice_far_load<PER, CH, NPAIR>(bufA, v2, base, 0, nf, nfx, T, n_in, tb);
    __syncthreads();  // the previous tile's LDS reads are done
#pragma unroll
    for (int t = 0; t < PER; ++t) {
      const int lp = t * 256 + threadIdx.x;
      if (lp < NPAIR) tile2[lp] = make_double2(ownx[t], owny[t]);
    }
    __syncthreads();
    // one bond or far field term: its Jx, Jy and Jz forms (or its hx form); pv(t): the partner pair as loaded
    auto term = [&](const LatticeTerm& f, auto&& pv) {
      double plain = 0.0, with_zz = 0.0, vz = 0.0;
#pragma unroll
      for (int t = 0; t < PER; ++t) {
        const int lp = t * 256 + threadIdx.x;
        const uint64_t r0 = (uint64_t)(base + 2 * (int64_t)(lp < NPAIR ? lp : 0));
        const uint64_t b0 = lattice_zz_bit(r0, f.a, f.b), b1 = b0 ^ (uint64_t)f.swap;
        const double2 v = lattice_swap_if(pv(t), f.swap);
        const double ex = ax[t] * v.x, ey = ay[t] * v.y;
        plain += ex + ey;
        with_zz += lattice_signed(ex, b0) + lattice_signed(ey, b1);
        vz += lattice_signed(dx[t], b0) + lattice_signed(dy[t], b1);
      }
      if (f.bond) {
        add(f.idx, plain);                   // Jx_t
        add(nb + f.idx, -with_zz);           // Jy_t
        add(2 * nb + f.idx, vz);             // Jz_t
      } else {
        add(3 * nb + f.idx, plain);          // hx_i
      }
    };
    auto consume = [&](const double2 (&buf)[PER][CH], int k0) {
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        if (k0 + e < nf) term(lattice_far_term(k0 + e, nfx, T, n_in, tb), [&](int t) { return buf[t][e]; });
      }
    };
    for (int k0 = 0; k0 < nf; k0 += 2 * CH) {
      lattice_far_load<PER, CH, NPAIR>(bufB, v2, base, k0 + CH, nf, nfx, T, n_in, tb);
      consume(bufA, k0);
      lattice_far_load<PER, CH, NPAIR>(bufA, v2, base, k0 + 2 * CH, nf, nfx, T, n_in, tb);
      consume(bufB, k0 + CH);
    }
    // bonds inside the tile
    for (int q = 0; q < n_in; ++q) {
      const LatticeTerm f = lattice_bond(tb[q]);
      const int px = (int)(((1u << f.a) | (1u << f.b)) >> 1);
      term(f, [&](int t) {
        const int lp = t * 256 + threadIdx.x;
        return tile2[(lp < NPAIR ? lp : 0) ^ px];
      });
    }
    // field terms inside the tile
    for (int i = 0; i < T; ++i) {
      double plain = 0.0;
#pragma unroll
      for (int t = 0; t < PER; ++t) {
        const int lp = t * 256 + threadIdx.x;
        const double2 v = lattice_swap_if(tile2[(lp < NPAIR ? lp : 0) ^ ((1 << i) >> 1)], i == 0);
        plain += ax[t] * v.x + ay[t] * v.y;
      }
      add(3 * nb + i, plain);
    }
    // hz_i
    for (int i = 0; i < L; ++i) {
      double vh = 0.0;
#pragma unroll
      for (int t = 0; t < PER; ++t) {
        const int lp = t * 256 + threadIdx.x;
        const uint64_t r0 = (uint64_t)(base + 2 * (int64_t)(lp < NPAIR ? lp : 0));
        vh += lattice_signed(dx[t], (r0 >> i) & 1ull) + lattice_signed(dy[t], ((r0 | 1ull) >> i) & 1ull);
      }
      add(3 * nb + L + i, vh);
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < nparam; c += 256)
    scratch[(int64_t)c * gridDim.x + blockIdx.x] = ((accs[0][c] + accs[1][c]) + accs[2][c]) + accs[3][c];
}

// second stage: out[t] = the sum of term t's per-block partials, fixed order; one block per term
__global__ __launch_bounds__(256) void k_lattice_forms_reduce(const double* __restrict__ scratch, int count,
                                                              double* __restrict__ out) {
  __shared__ double sm5[5];
  const double tot = sum_partials_block(scratch + (int64_t)blockIdx.x * count, count, sm5);
  if (threadIdx.x == 0) out[blockIdx.x] = tot;
}

// log2 of the tile: the TFIM mat-vec's tuning value, the whole vector when it is smaller
static inline int lattice_tile_log2(const OpDesc& op) {
  return op.lattice.L < op.tune_tile_log2 ? op.lattice.L : op.tune_tile_log2;
}
static inline int lattice_blocks(int L, int T) {   // one tile of 2^T rows per block; beyond the cap blocks walk several tiles
  int64_t nb = ((int64_t)1 << L) >> T;
  if (nb > DSEA_MAX_TFIM_BLOCKS) nb = DSEA_MAX_TFIM_BLOCKS;
  return (int)nb;
}

// The kernel arguments for a tile of 2^T rows: the bond table sorted "both sites below T" first, each group in the caller's
// order.  False when L, nb or T is out of range.
static bool lattice_params(const OpDesc& op, int T, LatticeParams* p) {
  const LatticeDesc& d = op.lattice;
  if (d.L < 2 || d.L > DSEA_LATTICE_MAX_L || d.nb < 1 || d.nb > DSEA_LATTICE_MAX_BONDS || T < 2 || T > 12 || T > d.L) return false;
  p->L = d.L;
  p->nb = d.nb;
  p->c = d.c;
  int at = 0;
  for (int far = 0; far < 2; ++far) {
    for (int t = 0; t < d.nb; ++t) {
      const bool is_far = d.a[t] >= T || d.b[t] >= T;
      if ((int)is_far == far) p->tb[at++] = (uint32_t)d.a[t] | ((uint32_t)d.b[t] << 8) | ((uint32_t)t << 16);
    }
    if (!far) p->n_in = at;
  }
  for (; at < DSEA_LATTICE_MAX_BONDS; ++at) p->tb[at] = 0;
  return true;
}

// partials per form that dsea_op_lattice_forms may write at any tile tuning (6 <= T <= 12): the smallest tile gives the most
// blocks
int64_t lattice_forms_scratch_doubles(int L, int nb) {
  return (int64_t)(3 * nb + 2 * L) * lattice_blocks(L, L < 6 ? L : 6);
}

int launch_spmv_lattice(const OpDesc& op, const double* x, double* y, const double* shift, const double* skip, double* P,
                        hipStream_t st, EventPair* ev) {
  LatticeParams p;
  const int T = lattice_tile_log2(op);
  if (!lattice_params(op, T, &p)) return -1;
  const int nblk = lattice_blocks(p.L, T);
  dispatch_int<2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12>(T, [&](auto t) {
    klaunch(ev, k_spmv_lattice<decltype(t)::value>, nblk, 256, 0, st, p, x, y, shift, skip, P);
  });
  return nblk;
}

int launch_lattice_forms(const OpDesc& op, const double* v1, const double* v2, double* out, double* scratch, hipStream_t st) {
  LatticeParams p;
  const int T = lattice_tile_log2(op);
  if (!lattice_params(op, T, &p)) return -1;
  const int nblk = lattice_blocks(p.L, T);
  dispatch_int<2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12>(T, [&](auto t) {
    klaunch(nullptr, k_lattice_forms<decltype(t)::value>, nblk, 256, 0, st, p, v1, v2, scratch);
  });
  hipLaunchKernelGGL(k_lattice_forms_reduce, dim3(3 * p.nb + 2 * p.L), dim3(256), 0, st, scratch, nblk, out);
  return 0;
}

}  // namespace dsea
