// dsea_chain.hip -- the matrix-free XYZ spin chain with per-site couplings (docs/design/14-spin-chain.md): its mat-vec
// k_spmv_chain, the parameter adjoint k_chain_forms (+ k_chain_forms_reduce), and their launchers.
//
//   H = sum_b [ Jx_b X_b X_b+1 + Jy_b Y_b Y_b+1 + Jz_b Z_b Z_b+1 ] + sum_i [ hx_i X_i + hz_i Z_i ],  periodic, L sites
// Site i is bit i of the row index s, z_i(s) = 1 - 2 bit_i(s), bond b joins sites b and (b + 1) mod L, m_b = its two bits:
//   (H x)[s] = ( sum_b Jz_b zz_b(s) + sum_i hz_i z_i(s) ) x[s] + sum_i hx_i x[s ^ (1 << i)]
//            + sum_b ( Jx_b - Jy_b zz_b(s) ) x[s ^ m_b]                                        zz_b = z_b z_b+1
// `couplings` is (5, L) row-major on the device: rows Jx, Jy, Jz, hx, hz.  Every block copies the 5 L numbers into LDS on
// every launch (wave-uniform broadcast reads afterwards): no host copy, in-place optimiser steps are seen.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_internal.h"
#include "dsea_device.h"

namespace dsea {

#define DSEA_CHAIN_MAX_L 62

// bit b of the result = bit_b(s) ^ bit_{(b+1) mod L}(s): zz_b(s) = 1 - 2 * that bit.  (L = 2: bonds 0 and 1 both join sites
// 0 and 1, both bits are set together.)
__device__ __forceinline__ uint64_t chain_bond_word(uint64_t s, int L) {
  return s ^ ((s >> 1) | ((s & 1ull) << (L - 1)));
}
// v * (1 - 2 bit_b(word)), exact: the bit goes into the sign
__device__ __forceinline__ double chain_signed(double v, uint64_t word, int b) {
  return __longlong_as_double(__double_as_longlong(v) ^ (long long)(((word >> b) & 1ull) << 63));
}
__device__ __forceinline__ double2 chain_swap_if(double2 v, bool swap) { return swap ? make_double2(v.y, v.x) : v; }

// The terms whose partner row lies outside the tile of 2^T rows (L > T), numbered k = 0 .. 2 (L - T):
//   k <  L - T : field term hx_i, i = T + k                                     -- the TFIM kernel's far flips
//   k >= L - T : bond b = T - 1 + (k - (L - T)), b = T - 1 .. L - 1:
//       b = T - 1          STRADDLING the tile edge (bits T - 1, T): the pair at (i0 ^ (1 << (T-1))) ^ (1 << T)
//       T <= b <= L - 2    BOTH bits FAR: the pair at i0 ^ (1 << b) ^ (1 << (b+1))
//       b = L - 1          the WRAP bond (bits L - 1 and 0): it flips bit 0, so it is the far pair at i0 ^ (1 << (L-1)) with its
//                          two elements swapped
// (T >= 2, so every mask but the wrap bond's keeps bit 0: the partner of a row pair is a row pair, one 16-byte load.)
// In the mat-vec a term contributes (ca - cb zz_b(s)) * x[partner]: ca = hx_i, cb = 0 for a field term, ca = Jx_b, cb = Jy_b
// for a bond.
struct ChainFarTerm {
  int64_t mask;   // xor mask of the pair's first row (bit 0 cleared)
  int b;          // bond index (its bit of the bond word); 0 for a field term
  int site;       // field term: its site, else -1
  bool swap;
};
__device__ __forceinline__ int chain_far_count(int L, int T) { return L > T ? 2 * (L - T) + 1 : 0; }
__device__ __forceinline__ ChainFarTerm chain_far_term(int k, int L, int T) {
  ChainFarTerm f;
  const int nfx = L - T;
  if (k < nfx) {
    f.site = T + k;
    f.mask = (int64_t)1 << f.site;
    f.b = 0;
    f.swap = false;
  } else {
    const int b = T - 1 + (k - nfx);
    const int b1 = (b + 1 == L) ? 0 : b + 1;
    f.mask = (((int64_t)1 << b) | ((int64_t)1 << b1)) & ~(int64_t)1;
    f.b = b;
    f.site = -1;
    f.swap = (b1 == 0);
  }
  return f;
}

// f(int_c<0>{}), ..., f(int_c<N-1>{}): a loop whose index is a constant in every trip (register arrays stay in registers even
// where the body is too large for the unroller)
template <int I, int N, class F>
__device__ __forceinline__ void chain_static_for(F&& f) {
  if constexpr (I < N) {
    f(int_c<I>{});
    chain_static_for<I + 1, N>(f);
  }
}

// the far pairs of terms k0 .. k0 + CH - 1 of every row pair of this thread: all requested before any is consumed
template <int PER, int CH, int NPAIR>
__device__ __forceinline__ void chain_far_load(double2 (&buf)[PER][CH], const double* __restrict__ x, int64_t base, int k0,
                                               int nf, int L, int T) {
#pragma unroll
  for (int e = 0; e < CH; ++e) {
    const bool on = k0 + e < nf;
    const int64_t mask = on ? chain_far_term(k0 + e, L, T).mask : 0;
#pragma unroll
    for (int t = 0; t < PER; ++t) {
      const int lp = t * 256 + threadIdx.x;
      const int64_t i0 = base + 2 * (int64_t)(lp < NPAIR ? lp : 0);
      buf[t][e] = make_double2(0.0, 0.0);
      if (on) buf[t][e] = *reinterpret_cast<const double2*>(x + (i0 ^ mask));
    }
  }
}

// y = H x - shift x ; partial x.y per block.  The tile scheme of the TFIM mat-vec: a block stages 2^T rows of x in LDS, a
// thread owns PER row pairs; partners with all flipped bits below T are LDS reads, everything else a coalesced 16-byte
// global read issued a chunk of terms ahead of its use.  The four geometric cases of a bond:
//   INSIDE the tile (b + 1 < T, and the wrap bond when T = L)   -- LDS
//   STRADDLING / BOTH FAR / WRAP                                -- chain_far_term above
template <int T>
__global__ __launch_bounds__(256) void k_spmv_chain(ChainParams p, const double* __restrict__ x, double* __restrict__ y,
                                                    const double* __restrict__ shift, const double* __restrict__ skip,
                                                    double* __restrict__ P) {
  constexpr int TILE = 1 << T;
  constexpr int NPAIR = TILE / 2;
  constexpr int PER = (NPAIR + 255) / 256;
  constexpr int CH = PER >= 8 ? 1 : (PER >= 4 ? 2 : 4);   // far terms per buffer (two buffers): <= 64 VGPRs each
  __shared__ double2 tile2[NPAIR];
  __shared__ double cp[5 * DSEA_CHAIN_MAX_L];
  __shared__ double sm5[5];
  if (skip && skip[0] != 0.0) return;
  const int L = p.L;
  const int64_t ntiles = ((int64_t)1 << L) >> T;
  const int nf = chain_far_count(L, T);
  for (int c = threadIdx.x; c < 5 * L; c += 256) cp[c] = p.c[c];
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
    __syncthreads();  // the couplings are in LDS; the previous tile's LDS reads are done
    double2 bufA[PER][CH], bufB[PER][CH];
    chain_far_load<PER, CH, NPAIR>(bufA, x, base, 0, nf, L, T);
#pragma unroll
    for (int t = 0; t < PER; ++t) {
      const int lp = t * 256 + threadIdx.x;
      if (lp < NPAIR) tile2[lp] = make_double2(ownx[t], owny[t]);
    }
    __syncthreads();
    double2 sum[PER];
    uint64_t w0[PER];
#pragma unroll
    for (int t = 0; t < PER; ++t) {
      const int lp = t * 256 + threadIdx.x;
      sum[t] = make_double2(0.0, 0.0);
      w0[t] = chain_bond_word((uint64_t)(base + 2 * (int64_t)(lp < NPAIR ? lp : 0)), L);
    }
    // out-of-tile terms, CH at a time through two buffers: the next chunk is requested before this one is consumed
    auto consume = [&](const double2 (&buf)[PER][CH], int k0) {
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        if (k0 + e < nf) {
          const ChainFarTerm f = chain_far_term(k0 + e, L, T);
          const double ca = f.site >= 0 ? cp[3 * L + f.site] : cp[f.b];
          const double cb = f.site >= 0 ? 0.0 : cp[L + f.b];
#pragma unroll
          for (int t = 0; t < PER; ++t) {
            const uint64_t w1 = w0[t] ^ 1ull ^ (1ull << (L - 1));   // the pair's second row: site 0 flipped
            const double2 pv = chain_swap_if(buf[t][e], f.swap);
            sum[t].x = fma(ca - chain_signed(cb, w0[t], f.b), pv.x, sum[t].x);
            sum[t].y = fma(ca - chain_signed(cb, w1, f.b), pv.y, sum[t].y);
          }
        }
      }
    };
    for (int k0 = 0; k0 < nf; k0 += 2 * CH) {
      chain_far_load<PER, CH, NPAIR>(bufB, x, base, k0 + CH, nf, L, T);       // (past the last term: zeros, no loads)
      consume(bufA, k0);
      chain_far_load<PER, CH, NPAIR>(bufA, x, base, k0 + 2 * CH, nf, L, T);
      consume(bufB, k0 + CH);
    }
    chain_static_for<0, PER>([&](auto tc) {
      constexpr int t = decltype(tc)::value;
      const int lp = t * 256 + threadIdx.x;
      if (lp < NPAIR) {
        const int64_t i0 = base + 2 * (int64_t)lp;
        const uint64_t wa = w0[t], wb = wa ^ 1ull ^ (1ull << (L - 1));
        const double2 xv = tile2[lp];
        double2 in = sum[t];
        // field terms inside the tile (site 0: the other element of the pair)
#pragma unroll
        for (int i = 0; i < T; ++i) {
          const double2 pv = chain_swap_if(tile2[lp ^ ((1 << i) >> 1)], i == 0);
          const double hx = cp[3 * L + i];
          in.x = fma(hx, pv.x, in.x);
          in.y = fma(hx, pv.y, in.y);
        }
        // bonds INSIDE the tile (bits b, b + 1 < T; bond 0 flips bit 0: swapped pair)
#pragma unroll
        for (int b = 0; b + 1 < T; ++b) {
          const double2 pv = chain_swap_if(tile2[lp ^ ((3 << b) >> 1)], b == 0);
          const double jx = cp[b], jy = cp[L + b];
          in.x = fma(jx - chain_signed(jy, wa, b), pv.x, in.x);
          in.y = fma(jx - chain_signed(jy, wb, b), pv.y, in.y);
        }
        // the WRAP bond when the tile is the whole vector (T = L): bits L - 1 and 0, inside the tile, swapped pair
        if (L == T) {
          const double2 pv = chain_swap_if(tile2[lp ^ (1 << (T - 2))], true);
          const double jx = cp[L - 1], jy = cp[2 * L - 1];
          in.x = fma(jx - chain_signed(jy, wa, L - 1), pv.x, in.x);
          in.y = fma(jx - chain_signed(jy, wb, L - 1), pv.y, in.y);
        }
        // diagonal: sum_b Jz_b zz_b + sum_i hz_i z_i
        double dzx = 0.0, dzy = 0.0, dhx = 0.0, dhy = 0.0;
        for (int b = 0; b < L; ++b) {
          const double jz = cp[2 * L + b], hz = cp[4 * L + b];
          dzx += chain_signed(jz, wa, b);
          dzy += chain_signed(jz, wb, b);
          dhx += chain_signed(hz, (uint64_t)i0, b);
          dhy += chain_signed(hz, (uint64_t)i0 | 1ull, b);
        }
        double2 v;
        v.x = fma(dzx + dhx, xv.x, in.x);
        v.y = fma(dzy + dhy, xv.y, in.y);
        if (shift) {
          v.x = __dsub_rn(v.x, __dmul_rn(s, xv.x));
          v.y = __dsub_rn(v.y, __dmul_rn(s, xv.y));
        }
        *reinterpret_cast<double2*>(y + i0) = v;
        acc = fma(xv.x, v.x, acc);
        acc = fma(xv.y, v.y, acc);
      }
    });
  }
  if (P) {
    __syncthreads();
    double tot = block_sum(acc, sm5);
    if (threadIdx.x == 0) P[blockIdx.x] = tot;
  }
}

// The parameter adjoint: all 5 L bilinear forms out[t] = v1^T (dH/dp_t) v2 in one pass over v1 and v2 (t in the order of the
// couplings: Jx_b, Jy_b, Jz_b, hx_i, hz_i):
//   Jz_b: sum_s zz_b v1[s] v2[s]          hz_i: sum_s z_i v1[s] v2[s]          hx_i: sum_s v1[s] v2[s ^ (1 << i)]
//   Jx_b: sum_s v1[s] v2[s ^ m_b]         Jy_b: -sum_s zz_b v1[s] v2[s ^ m_b]
// Same tiling as the mat-vec (v2 staged in LDS, far pairs of v2 a chunk of terms ahead).  No per-lane accumulator per term:
// every term is reduced through the wave at once (wave_sum, fixed order) and lane 0 adds it to the wave's row of LDS
// accumulators; the four rows are added in fixed order and written to scratch[t * gridDim.x + block].  No atomics.
template <int T>
__global__ __launch_bounds__(256) void k_chain_forms(ChainParams p, const double* __restrict__ v1,
                                                     const double* __restrict__ v2, double* __restrict__ scratch) {
  constexpr int TILE = 1 << T;
  constexpr int NPAIR = TILE / 2;
  constexpr int PER = (NPAIR + 255) / 256;
  constexpr int CH = PER >= 8 ? 1 : (PER >= 4 ? 2 : 4);
  __shared__ double2 tile2[NPAIR];
  __shared__ double accs[4][5 * DSEA_CHAIN_MAX_L];
  const int L = p.L;
  const int64_t ntiles = ((int64_t)1 << L) >> T;
  const int nf = chain_far_count(L, T);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double* __restrict__ mine = accs[wv];
  for (int c = lane; c < 5 * L; c += 64) mine[c] = 0.0;   // (afterwards a wave's row is touched by its lane 0 alone)
  __syncthreads();
  auto add = [&](int term, double val) {
    const double tot = wave_sum(val);
    if (lane == 0) mine[term] += tot;
  };
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base = tile * TILE;
    double2 a[PER], own[PER];
    uint64_t w0[PER];
#pragma unroll
    for (int t = 0; t < PER; ++t) {
      const int lp = t * 256 + threadIdx.x;
      const int64_t i0 = base + 2 * (int64_t)(lp < NPAIR ? lp : 0);
      a[t] = *reinterpret_cast<const double2*>(v1 + i0);
      own[t] = *reinterpret_cast<const double2*>(v2 + i0);
      if (lp >= NPAIR) a[t] = make_double2(0.0, 0.0);       // a thread without a pair adds zeros to every form
      w0[t] = chain_bond_word((uint64_t)i0, L);
    }
    double2 bufA[PER][CH], bufB[PER][CH];
    chain_far_load<PER, CH, NPAIR>(bufA, v2, base, 0, nf, L, T);
    __syncthreads();  // the previous tile's LDS reads are done
#pragma unroll
    for (int t = 0; t < PER; ++t) {
      const int lp = t * 256 + threadIdx.x;
      if (lp < NPAIR) tile2[lp] = own[t];
    }
    __syncthreads();
    // out-of-tile terms, through two buffers as in the mat-vec
    auto consume = [&](const double2 (&buf)[PER][CH], int k0) {
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        if (k0 + e < nf) {
          const ChainFarTerm f = chain_far_term(k0 + e, L, T);
          double plain = 0.0, with_zz = 0.0;
#pragma unroll
          for (int t = 0; t < PER; ++t) {
            const uint64_t w1 = w0[t] ^ 1ull ^ (1ull << (L - 1));
            const double2 pv = chain_swap_if(buf[t][e], f.swap);
            const double ex = a[t].x * pv.x, ey = a[t].y * pv.y;
            plain += ex + ey;
            with_zz += chain_signed(ex, w0[t], f.b) + chain_signed(ey, w1, f.b);
          }
          if (f.site >= 0) {
            add(3 * L + f.site, plain);        // hx_i
          } else {
            add(f.b, plain);                   // Jx_b
            add(L + f.b, -with_zz);            // Jy_b
          }
        }
      }
    };
    for (int k0 = 0; k0 < nf; k0 += 2 * CH) {
      chain_far_load<PER, CH, NPAIR>(bufB, v2, base, k0 + CH, nf, L, T);
      consume(bufA, k0);
      chain_far_load<PER, CH, NPAIR>(bufA, v2, base, k0 + 2 * CH, nf, L, T);
      consume(bufB, k0 + CH);
    }
    // field terms inside the tile
    for (int i = 0; i < T; ++i) {
      double plain = 0.0;
#pragma unroll
      for (int t = 0; t < PER; ++t) {
        const int lp = t * 256 + threadIdx.x;
        const double2 pv = chain_swap_if(tile2[(lp < NPAIR ? lp : 0) ^ ((1 << i) >> 1)], i == 0);
        plain += a[t].x * pv.x + a[t].y * pv.y;
      }
      add(3 * L + i, plain);
    }
    // bonds INSIDE the tile, and the WRAP bond when the tile is the whole vector (T = L)
    const int nin = (L == T) ? T : T - 1;
    for (int b = 0; b < nin; ++b) {
      const int px = (b == T - 1) ? (1 << (T - 2)) : ((3 << b) >> 1);
      const bool swap = (b == 0) || (b == T - 1);
      double plain = 0.0, with_zz = 0.0;
#pragma unroll
      for (int t = 0; t < PER; ++t) {
        const int lp = t * 256 + threadIdx.x;
        const uint64_t w1 = w0[t] ^ 1ull ^ (1ull << (L - 1));
        const double2 pv = chain_swap_if(tile2[(lp < NPAIR ? lp : 0) ^ px], swap);
        const double ex = a[t].x * pv.x, ey = a[t].y * pv.y;
        plain += ex + ey;
        with_zz += chain_signed(ex, w0[t], b) + chain_signed(ey, w1, b);
      }
      add(b, plain);
      add(L + b, -with_zz);
    }
    // diagonal families
    for (int b = 0; b < L; ++b) {
      double vz = 0.0, vh = 0.0;
#pragma unroll
      for (int t = 0; t < PER; ++t) {
        const int lp = t * 256 + threadIdx.x;
        const uint64_t i0 = (uint64_t)(base + 2 * (int64_t)(lp < NPAIR ? lp : 0));
        const uint64_t w1 = w0[t] ^ 1ull ^ (1ull << (L - 1));
        const double px = a[t].x * own[t].x, py = a[t].y * own[t].y;
        vz += chain_signed(px, w0[t], b) + chain_signed(py, w1, b);
        vh += chain_signed(px, i0, b) + chain_signed(py, i0 | 1ull, b);
      }
      add(2 * L + b, vz);
      add(4 * L + b, vh);
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 5 * L; c += 256)
    scratch[(int64_t)c * gridDim.x + blockIdx.x] = ((accs[0][c] + accs[1][c]) + accs[2][c]) + accs[3][c];
}

// second stage: out[t] = the sum of term t's per-block partials, fixed order; one block per term
__global__ __launch_bounds__(256) void k_chain_forms_reduce(const double* __restrict__ scratch, int count,
                                                            double* __restrict__ out) {
  __shared__ double sm5[5];
  const double tot = sum_partials_block(scratch + (int64_t)blockIdx.x * count, count, sm5);
  if (threadIdx.x == 0) out[blockIdx.x] = tot;
}

// log2 of the tile: the TFIM mat-vec's tuning value, the whole vector when it is smaller
static inline int chain_tile_log2(const OpDesc& op) {
  return op.chain.L < op.tune_tile_log2 ? op.chain.L : op.tune_tile_log2;
}
static inline int chain_blocks(int L, int T) {   // one tile of 2^T rows per block; beyond the cap blocks walk several tiles
  int64_t nb = ((int64_t)1 << L) >> T;
  if (nb > DSEA_MAX_TFIM_BLOCKS) nb = DSEA_MAX_TFIM_BLOCKS;
  return (int)nb;
}

// partials per form that dsea_op_chain_forms may write at any tile tuning (6 <= T <= 12): the smallest tile gives the most blocks
int64_t chain_forms_scratch_doubles(int L) {
  return (int64_t)5 * L * chain_blocks(L, L < 6 ? L : 6);
}

int launch_spmv_chain(const OpDesc& op, const double* x, double* y, const double* shift, const double* skip, double* P,
                      hipStream_t st, EventPair* ev) {
  const ChainParams& p = op.chain;
  const int T = chain_tile_log2(op);
  if (p.L < 2 || p.L > DSEA_CHAIN_MAX_L || T < 2 || T > 12) return -1;
  const int nb = chain_blocks(p.L, T);
  dispatch_int<2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12>(T, [&](auto t) {
    klaunch(ev, k_spmv_chain<decltype(t)::value>, nb, 256, 0, st, p, x, y, shift, skip, P);
  });
  return nb;
}

int launch_chain_forms(const OpDesc& op, const double* v1, const double* v2, double* out, double* scratch, hipStream_t st) {
  const ChainParams& p = op.chain;
  const int T = chain_tile_log2(op);
  if (p.L < 2 || p.L > DSEA_CHAIN_MAX_L || T < 2 || T > 12) return -1;
  const int nb = chain_blocks(p.L, T);
  dispatch_int<2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12>(T, [&](auto t) {
    klaunch(nullptr, k_chain_forms<decltype(t)::value>, nb, 256, 0, st, p, v1, v2, scratch);
  });
  hipLaunchKernelGGL(k_chain_forms_reduce, dim3(5 * p.L), dim3(256), 0, st, scratch, nb, out);
  return 0;
}

}  // namespace dsea
