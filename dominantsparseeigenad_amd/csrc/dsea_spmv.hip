// dsea_spmv.hip -- the operator kernels: the matrix-free TFIM mat-vec, CSR, sliced ELLPACK and its parameter kernels
// (value refresh, sampled outer product), the 3-point stencil and the symmetric dense form; the fused Lanczos tails that
// ride on a mat-vec (TfimFusedArgs); launch_spmv / launch_tfim_fused, which pick among them.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_internal.h"
#include "dsea_device.h"

namespace dsea {

// ------------------------------------------------------------------------------------------
// operators
// ------------------------------------------------------------------------------------------
// TFIM, matrix-free.  A block stages a tile of 2^T consecutive rows of x in LDS: flips of the low
// T bits are LDS reads, flips of bits T..Lloc-1 are coalesced global reads of other tiles (served
// by L2 / Infinity Cache: the whole vector is 8 MiB at L = 20).
//   y[i] = dscale*d(gi)*x[i] - g * sum_j x[i^(1<<j)] - shift*x[i] ;   partial x.y
// A thread owns PAIR consecutive-row pairs (16-byte LDS and global accesses); the out-of-tile loads of
// all its pairs are issued four bits at a time before any of them is consumed.
//
// FUSED (Lanczos tail, Lanczos.py:69-72,75 in one launch): the input is the un-normalised r,
//   beta = sqrt(sum of the ||r||^2 partials) ; q = r/beta -> Q[i] (+ bf16 shadow) ; u = H q ; partial q.u
// in-tile neighbours use the scaled values, the out-of-tile neighbour sum is scaled once (linearity).
struct TfimFusedArgs {
  const double* nP;      // partials of ||r||^2
  int nCount;
  double* q_out;         // Q[i]
  ShadowRow qs_out;      // shadow row (bf16 or 8-bit) or none
  double* beta_store;    // betas[i-1]
  double* brk;           // breakdown record (see broken()) or null
  int step;              // Lanczos step i (recorded on breakdown)
};

// beta of the fused Lanczos tail + the breakdown decision (identical in every block); returns false to stop
__device__ __forceinline__ bool fused_beta(const TfimFusedArgs& fa, double* sm5, double& beta) {
  if (broken(fa.brk)) return false;
  beta = sqrt(sum_partials_block(fa.nP, fa.nCount, sm5));
  if (blockIdx.x == 0 && threadIdx.x == 0) fa.beta_store[0] = beta;
  if (fa.brk && !(beta > DSEA_BREAK_TOL * fa.brk[1])) {
    if (blockIdx.x == 0 && threadIdx.x == 0) fa.brk[0] = (double)fa.step;
    return false;
  }
  return true;
}

// q = r / beta with beta from the ||r||^2 PARTIALS (every block sums them in its prologue, as the fused operator tails do):
// the normalise-and-store of a Lanczos step whose mat-vec is the caller's code (dsea_lanczos_callable_step) without the
// stand-alone second-stage launch in front of it
__global__ __launch_bounds__(256) void k_scale_store_fused(const double* __restrict__ r, TfimFusedArgs fa, int64_t n) {
  __shared__ double sm5[5];
  const int64_t stride = (int64_t)gridDim.x * 512;
  const int64_t row0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
  double2 v = ld2<true>(r, row0, n);                       // (requested before the partials are waited for)
  double beta = 1.0;
  if (!fused_beta(fa, sm5, beta)) return;
  for (int64_t row = row0; row < n; row += stride) {
    if (row != row0) v = ld2<true>(r, row, n);
    v.x = v.x / beta;
    v.y = v.y / beta;
    st2<true>(fa.q_out, row, n, v);
    st_shadow_x2(fa.qs_out, row, n, v);
  }
}

void launch_scale_store_fused(const double* r, const double* nP, int nCount, double* q, ShadowRow qs, double* beta_store,
                              int64_t n, hipStream_t st) {
  TfimFusedArgs fa = {nP, nCount, q, qs, beta_store, nullptr, 0};
  hipLaunchKernelGGL(k_scale_store_fused, dim3(ew_blocks(n)), dim3(256), 0, st, r, fa, n);
}

template <int T, bool FUSED>
__global__ __launch_bounds__(256) void k_spmv_tfim(TfimParams p, const double* __restrict__ x,
                                                   double* __restrict__ y,
                                                   const double* __restrict__ shift,
                                                   const double* __restrict__ skip,
                                                   double* __restrict__ P, TfimFusedArgs fa) {
  constexpr int TILE = 1 << T;
  constexpr int NPAIR = TILE / 2;                       // T >= 1
  constexpr int PER = (NPAIR + 255) / 256;              // pairs per thread
  // far bits whose loads are issued up front: as many as registers allow (L = 20: all of them either way)
// (measured on MI355X at L = 20, average over the fused + plain launches of a bench step: FB_FUSED 1 / 3 / 5 / 7 / 9
//  -> 14.5 / 13.8 / 13.3 / 13.1 / 17.9 us -- at 9 the fused kernel needs 254 VGPRs and only one block fits a CU.
//  The kernel is NOT latency-bound after all: it sits on the fabric traffic of its cross-XCD reads)
#ifndef DSEA_FB_FUSED
#define DSEA_FB_FUSED 7
#endif
#ifndef DSEA_FB_PLAIN
#define DSEA_FB_PLAIN 9
#endif
  constexpr int FB = PER >= 4 ? (FUSED ? DSEA_FB_FUSED : DSEA_FB_PLAIN) : (PER == 2 ? 12 : 14);
  __shared__ double2 tile2[NPAIR];
  __shared__ double sm5[5];
  if (!FUSED && skip && skip[0] != 0.0) return;
  if (FUSED && broken(fa.brk)) return;
  const uint64_t maskL = (p.L >= 64) ? ~0ull : ((1ull << p.L) - 1ull);
  const int64_t ntiles = ((int64_t)1 << p.L_local) >> T;
  double acc = 0.0;
  double beta = 1.0, g = 0.0, s = 0.0;
  bool first = true;
  // a block walks tiles blockIdx.x, +gridDim.x, ... (the grid is capped so that the per-block partials fit)
  // (round 5: mapping workgroup b to tile (b mod 8) * ntiles / 8 + b / 8 -- every XCD a CONTIGUOUS eighth of the vector instead
  //  of every eighth tile -- was built and measured: 12.65 vs 12.69 us, PMC read 33.8 MB = 4.0 x the vector either way, as the
  //  sub-cube argument of DESIGN.md section 3 says; profiles/r05_tfim_tail_xcd_map.txt.  Not kept.)
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base = tile * TILE;
    // 1. everything that does not depend on a scalar is put in flight first: the block's own rows and the
    //    out-of-tile neighbours of the first FB far bits (they are scaled by 1/beta afterwards -- linearity).  The
    //    kernel is latency-bound (~5 dependent memory round trips of 1.5-2 us when issued one after the other);
    //    issued together they overlap each other, the beta reduction and the LDS staging.
    double2 own[PER];
    double2 fb[PER][FB];
#pragma unroll
    for (int t = 0; t < PER; ++t) {
      const int lp = t * 256 + threadIdx.x;
      const int64_t i0 = base + 2 * (int64_t)(lp < NPAIR ? lp : 0);
      own[t] = *reinterpret_cast<const double2*>(x + i0);
#pragma unroll
      for (int e = 0; e < FB; ++e) {
        fb[t][e] = make_double2(0.0, 0.0);
        if (T + e < p.L_local) fb[t][e] = *reinterpret_cast<const double2*>(x + (i0 ^ ((int64_t)1 << (T + e))));
      }
    }
    if (first) {
      if (FUSED && !fused_beta(fa, sm5, beta)) return;   // the same decision in every block
      g = p.g_dev ? p.g_dev[0] : p.g_const;
      s = shift ? shift[0] : 0.0;
      first = false;
    }
    __syncthreads();  // previous tile's LDS reads are done
#pragma unroll
    for (int t = 0; t < PER; ++t) {
      const int lp = t * 256 + threadIdx.x;
      if (lp < NPAIR) {
        double2 v = own[t];
        if (FUSED) {
          v.x = v.x / beta;
          v.y = v.y / beta;
          *reinterpret_cast<double2*>(fa.q_out + base + 2 * lp) = v;
          st_shadow_x2(fa.qs_out, base + 2 * lp, base + TILE, v);   // (whole pairs: the tile lies inside the vector)
        }
        tile2[lp] = v;
      }
    }
    __syncthreads();
    double2 far[PER];
#pragma unroll
    for (int t = 0; t < PER; ++t) {
      far[t] = make_double2(0.0, 0.0);
#pragma unroll
      for (int e = 0; e < FB; ++e) {   // zero for bits beyond L_local
        far[t].x += fb[t][e].x;
        far[t].y += fb[t][e].y;
      }
    }
    // remaining far bits (L_local > T + FB): four bits per trip, loads first
    int j = T + FB;
    for (; j + 4 <= p.L_local; j += 4) {
      double2 nb[PER][4];
#pragma unroll
      for (int t = 0; t < PER; ++t) {
        const int lp = t * 256 + threadIdx.x;
        const int64_t i0 = base + 2 * (int64_t)(lp < NPAIR ? lp : 0);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          nb[t][e] = *reinterpret_cast<const double2*>(x + (i0 ^ ((int64_t)1 << (j + e))));
      }
#pragma unroll
      for (int t = 0; t < PER; ++t) {
        far[t].x += (nb[t][0].x + nb[t][1].x) + (nb[t][2].x + nb[t][3].x);
        far[t].y += (nb[t][0].y + nb[t][1].y) + (nb[t][2].y + nb[t][3].y);
      }
    }
    for (; j < p.L_local; ++j) {
#pragma unroll
      for (int t = 0; t < PER; ++t) {
        const int lp = t * 256 + threadIdx.x;
        const int64_t i0 = base + 2 * (int64_t)(lp < NPAIR ? lp : 0);
        const double2 nbv = *reinterpret_cast<const double2*>(x + (i0 ^ ((int64_t)1 << j)));
        far[t].x += nbv.x;
        far[t].y += nbv.y;
      }
    }
#pragma unroll
    for (int t = 0; t < PER; ++t) {
      const int lp = t * 256 + threadIdx.x;
      if (lp < NPAIR) {
        const int64_t i0 = base + 2 * (int64_t)lp;
        const double2 xv = tile2[lp];
        double2 sum = make_double2(xv.y, xv.x);  // bit 0: the other element of the pair
#pragma unroll
        for (int jb = 1; jb < T; ++jb) {
          const double2 nbv = tile2[lp ^ (1 << (jb - 1))];
          sum.x += nbv.x;
          sum.y += nbv.y;
        }
        if (FUSED) {
          sum.x += far[t].x / beta;
          sum.y += far[t].y / beta;
        } else {
          sum.x += far[t].x;
          sum.y += far[t].y;
        }
        double2 v;
        v.x = __dsub_rn(__dmul_rn(xv.x, tfim_diag(p, i0, maskL)), __dmul_rn(g, sum.x));
        v.y = __dsub_rn(__dmul_rn(xv.y, tfim_diag(p, i0 + 1, maskL)), __dmul_rn(g, sum.y));
        if (!FUSED && shift) {
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

// n = 1 (L_local = 0): a single row, no neighbours inside the slab
__global__ void k_spmv_tfim_single(TfimParams p, const double* __restrict__ x, double* __restrict__ y,
                                   const double* __restrict__ shift, const double* __restrict__ skip,
                                   double* __restrict__ P) {
  if (skip && skip[0] != 0.0) return;
  const uint64_t maskL = (p.L >= 64) ? ~0ull : ((1ull << p.L) - 1ull);
  const double xi = x[0];
  double v = __dmul_rn(xi, tfim_diag(p, 0, maskL));
  if (shift) v = __dsub_rn(v, __dmul_rn(shift[0], xi));
  y[0] = v;
  if (P) P[0] = xi * v;
}

static inline int tfim_blocks(const TfimParams& p, int T) {   // one tile of 2^T rows per block
  int64_t nb = ((int64_t)1 << p.L_local) >> T;
  if (nb > DSEA_MAX_TFIM_BLOCKS) nb = DSEA_MAX_TFIM_BLOCKS;  // blocks then walk several tiles
  return (int)nb;
}

// The TFIM mat-vec of one tile size, plain or with the Lanczos tail (fa); returns the number of partials or -1
template <bool FUSED>
static int launch_tfim(const OpDesc& op, const double* x, double* y, const double* shift, const double* skip, double* P,
                       const TfimFusedArgs& fa, hipStream_t st, EventPair* ev) {
  const TfimParams& p = op.tfim;
  const int T = p.L_local < op.tune_tile_log2 ? p.L_local : op.tune_tile_log2;
  if (T < 1 || T > 12) return -1;
  const int nb = tfim_blocks(p, T);
  dispatch_int<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12>(T, [&](auto t) {
    klaunch(ev, k_spmv_tfim<decltype(t)::value, FUSED>, nb, 256, 0, st, p, x, y, shift, skip, P, fa);
  });
  return nb;
}

// CSR: G lanes cooperate on one row
template <int G>
__global__ __launch_bounds__(256) void k_spmv_csr(CsrParams p, const double* __restrict__ x,
                                                  double* __restrict__ y,
                                                  const double* __restrict__ shift,
                                                  const double* __restrict__ skip,
                                                  double* __restrict__ P) {
  __shared__ double sm4[4];
  if (skip && skip[0] != 0.0) return;
  const double s = shift ? shift[0] : 0.0;
  const int sub = threadIdx.x % G;
  const int64_t rows_per_block = 256 / G;
  double acc = 0.0;
  for (int64_t row = (int64_t)blockIdx.x * rows_per_block + threadIdx.x / G; row < p.n;
       row += (int64_t)gridDim.x * rows_per_block) {
    const int64_t lo = p.rowptr[row], hi = p.rowptr[row + 1];
    double sum = 0.0;
    for (int64_t e = lo + sub; e < hi; e += G) sum = fma(p.vals[e], x[p.colidx[e]], sum);
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
    if (sub == 0) {
      const double xi = x[row];
      double v = sum;
      if (shift) v = __dsub_rn(v, __dmul_rn(s, xi));
      y[row] = v;
      acc = fma(xi, v, acc);
    }
  }
  if (P) {
    double tot = block_sum(acc, sm4);
    if (threadIdx.x == 0) P[blockIdx.x] = tot;
  }
}

// CSR, streaming form: a block owns CSR_ROWS consecutive rows; their non-zeros are one contiguous range of
// vals / colidx, which the block reads fully coalesced (thread t takes elements t, t+256, ...), multiplies
// with the gathered x and parks in LDS; then one thread per row adds up its segment.  Blocks whose range
// does not fit the LDS buffer (very long rows) fall back to 32 lanes per row inside the same kernel.
#define CSR_ROWS 128
#define CSR_CAP 6144
__global__ __launch_bounds__(256) void k_spmv_csr_stream(CsrParams p, const double* __restrict__ x,
                                                         double* __restrict__ y,
                                                         const double* __restrict__ shift,
                                                         const double* __restrict__ skip,
                                                         double* __restrict__ P) {
  __shared__ double prod[CSR_CAP];
  __shared__ double sm4[4];
  if (skip && skip[0] != 0.0) return;
  const double s = shift ? shift[0] : 0.0;
  double acc = 0.0;
  const int64_t nchunks = (p.n + CSR_ROWS - 1) / CSR_ROWS;
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int64_t r0 = chunk * CSR_ROWS;
    const int64_t r1 = (r0 + CSR_ROWS < p.n) ? r0 + CSR_ROWS : p.n;
    const int64_t e0 = p.rowptr[r0], e1 = p.rowptr[r1];
    __syncthreads();
    if (e1 - e0 <= CSR_CAP) {
      for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) prod[e - e0] = p.vals[e] * x[p.colidx[e]];
      __syncthreads();
      const int64_t row = r0 + threadIdx.x;
      if (threadIdx.x < CSR_ROWS && row < r1) {
        const int lo = (int)(p.rowptr[row] - e0), hi = (int)(p.rowptr[row + 1] - e0);
        double sum = 0.0;
        for (int e = lo; e < hi; ++e) sum += prod[e];
        const double xi = x[row];
        double v = sum;
        if (shift) v = __dsub_rn(v, __dmul_rn(s, xi));
        y[row] = v;
        acc = fma(xi, v, acc);
      }
    } else {
      const int sub = threadIdx.x & 31;
      for (int64_t row = r0 + (threadIdx.x >> 5); row < r1; row += 8) {
        double sum = 0.0;
        for (int64_t e = p.rowptr[row] + sub; e < p.rowptr[row + 1]; e += 32) sum = fma(p.vals[e], x[p.colidx[e]], sum);
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
        if (sub == 0) {
          const double xi = x[row];
          double v = sum;
          if (shift) v = __dsub_rn(v, __dmul_rn(s, xi));
          y[row] = v;
          acc = fma(xi, v, acc);
        }
      }
    }
  }
  if (P) {
    __syncthreads();
    double tot = block_sum(acc, sm4);
    if (threadIdx.x == 0) P[blockIdx.x] = tot;
  }
}

// Sliced ELLPACK (SELL-64): rows are grouped in slices of 64 (one wave), each slice stored column-major
// (element k of lane l at slice_ptr[s] + 64 k + l) and padded to the slice's longest row with (col = own row,
// val = 0).  Matrix loads are perfectly coalesced, and for the banded / structured operators of this domain the
// gather x[col] of a wave hits consecutive addresses as well (lane = row).
//
// k_spmv_sell_r5: the round-5 kernel (lane = row, scalar 8-byte matrix loads, two columns in flight), kept behind
// DSEA_TUNE_SELL_UNROLL = 1 as the "before" arm of tools/kbench_csr.py.  It ran at 0.65 of the HBM peak.
template <bool FUSED>
__global__ __launch_bounds__(256) void k_spmv_sell_r5(SellParams p, const double* __restrict__ x,
                                                   double* __restrict__ y, const double* __restrict__ shift,
                                                   const double* __restrict__ skip, double* __restrict__ P,
                                                   TfimFusedArgs fa) {
  __shared__ double sm5[5];
  if (!FUSED && skip && skip[0] != 0.0) return;
  double beta = 1.0;
  // Lanczos tail: x is the un-normalised r; q = r/beta is stored and used for every gather
  if (FUSED && !fused_beta(fa, sm5, beta)) return;
  const double s = shift ? shift[0] : 0.0;
  const int lane = threadIdx.x & 63;
  double acc = 0.0;
  for (int64_t sl = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); sl < p.nslices; sl += (int64_t)gridDim.x * 4) {
    const int64_t b0 = p.slice_ptr[sl], b1 = p.slice_ptr[sl + 1];
    const int64_t row = sl * 64 + lane;
    double s0 = 0.0, s1 = 0.0;
    int64_t e = b0 + lane;
    for (; e + 64 < b1; e += 128) {
      const double v0 = p.vals[e], v1 = p.vals[e + 64];
      const int c0 = p.colidx[e], c1 = p.colidx[e + 64];
      double x0 = x[c0], x1 = x[c1];
      if (FUSED) {
        x0 = x0 / beta;
        x1 = x1 / beta;
      }
      s0 = fma(v0, x0, s0);
      s1 = fma(v1, x1, s1);
    }
    if (e < b1) {
      double x0 = x[p.colidx[e]];
      if (FUSED) x0 = x0 / beta;
      s0 = fma(p.vals[e], x0, s0);
    }
    if (row < p.n) {
      double xi = x[row];
      if (FUSED) {
        xi = xi / beta;
        fa.q_out[row] = xi;
        st_shadow(fa.qs_out, row, xi);
      }
      double v = s0 + s1;
      if (!FUSED && shift) v = __dsub_rn(v, __dmul_rn(s, xi));
      y[row] = v;
      acc = fma(xi, v, acc);
    }
  }
  if (P) {
    __syncthreads();
    double tot = block_sum(acc, sm5);
    if (threadIdx.x == 0) P[blockIdx.x] = tot;
  }
}

// k_spmv_sell (round 6).  What was measured on MI355X with the 21-nnz/row TFIM matrix at n = 2^20 (tools/kbench_csr.py,
// profiles/r06_kbench_csr.txt; kernel alone, 281 MB algorithmic):
//   * the round-5 kernel: 48.8 us = 5.76 TB/s.  Requesting 4 / 8 columns instead of 2 before the first gather: 48.7 / 47.8 us --
//     the kernel is NOT short of loads in flight (8 waves per SIMD already cover the latency);
//   * non-temporal matrix loads: 52-53 us (worse: the stream then bypasses the path that keeps x's lines next to it);
//   * 16-byte matrix loads (a lane takes two rows of one slice column, half-waves take alternate columns, v_permlane32_swap
//     at the end): bit-identical, 53.6 us -- every gather instruction then touches twice the cache lines at half density;
//   * what it sits on is the FABRIC: besides the 264 MB matrix stream every XCD's L2 re-fetches the parts of x its rows
//     gather from (the matrix-free kernel alone moves 4 x the vector, docs/design/04-kernels.md), ~310 MB at the box's
//     6.8 TB/s read ceiling = 46 us.  The lever that is left is BYTES: k_spmv_sell16 below (16-bit column deltas).
// The fused Lanczos tail divided every gathered element by beta (21 fp64 divisions per row: 65 us against 52 for the plain
// launch); it now uses linearity like the matrix-free tail: u = (A r) / beta, one division per row beside q = r / beta.
template <int MODE>
__device__ __forceinline__ double sell_gather(const SellParams& p, const double* __restrict__ x, int c) {
  if (MODE == 1) {
    const double* base = x;
    int64_t idx = c;
    if (c < 0) {
      base = p.halo_lo;
      idx = (int64_t)c + p.hb;
    } else if ((int64_t)c >= p.n) {
      base = p.halo_hi;
      idx = (int64_t)c - p.n;
    }
    return base[idx];
  }
  if (MODE == 2) return p.xg[c];
  return x[c];
}

// slice handled by wave w of block b in trip t: plain round-robin, or (xcd != 0) XCD-contiguous -- workgroups are dealt
// to the 8 XCDs in turn, so block b works on eighth b % 8 of the slices and that XCD's L2 keeps one eighth of x hot
__device__ __forceinline__ int64_t sell_slice_of(const SellParams& p, int64_t linear) {
  if (!p.xcd) return linear;
  const int64_t nchunk = (p.nslices + 3) / 4;               // chunks of 4 slices (one block)
  const int64_t per = (nchunk + 7) / 8;
  const int64_t chunk = linear >> 2;
  const int64_t mapped = (chunk & 7) * per + (chunk >> 3);
  return mapped < nchunk ? mapped * 4 + (linear & 3) : p.nslices;
}

// sum_k vals[k] x[col k] of this lane's row of slice [b0, b1): even / odd slice columns accumulated separately, in order
template <int MODE, int UN, bool C16, bool NT = false>
__device__ __forceinline__ double sell_row_sum(const SellParams& p, const double* __restrict__ x, int64_t b0, int64_t b1,
                                               int lane) {
  double s0 = 0.0, s1 = 0.0;
  // 16-bit columns: lane j keeps the base of slice column kb + j (one coalesced load per 64 columns); a column's base is
  // then a v_readlane with a wave-uniform index instead of a broadcast load per column (44.8 vs 47.2 us)
  int cbl = 0;
  int kb = -64;
  for (int64_t e0 = b0 + lane; C16 ? (e0 - lane < b1) : (e0 < b1); e0 += 64 * UN) {
    double v[UN], g[UN];
    int c[UN];
    const int k0 = __builtin_amdgcn_readfirstlane((int)((e0 - lane - b0) >> 6));
    if (C16 && (k0 & ~63) != kb) {
      kb = k0 & ~63;
      const int64_t cbi = (b0 >> 6) + kb + lane;
      cbl = cbi < (b1 >> 6) ? p.colbase[cbi] : 0;
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int64_t e = e0 + 64 * u;
      v[u] = 0.0;
      c[u] = 0;
      if (e < b1) {
        v[u] = NT ? __builtin_nontemporal_load(p.vals + e) : p.vals[e];
        const int d16 = C16 ? (int)(NT ? __builtin_nontemporal_load(p.col16 + e) : p.col16[e]) : 0;
        c[u] = C16 ? __builtin_amdgcn_readlane(cbl, (k0 + u) & 63) + d16 : p.colidx[e];
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) g[u] = (e0 + 64 * u < b1) ? sell_gather<MODE>(p, x, c[u]) : 0.0;
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      if (e0 + 64 * u < b1) {
        if (u & 1) s1 = fma(v[u], g[u], s1);
        else s0 = fma(v[u], g[u], s0);
      }
    }
  }
  return s0 + s1;
}

// VALUE-CODED operand (dsea_op_create_sell16v8): the value of an element is vt[code], a table of 256 doubles in LDS, and
// the per-element metadata is PACKED four slice columns to a lane: element (column 4 G + j, lane l) of a slice sits at
// 256 G + 4 l + j of its arrays, so one uint32 holds a lane's four codes and one 8-byte word its four column deltas --
// 2 + 4 memory instructions per four non-zeros of a row instead of 12.  Why that matters: with 3 instead of 10 bytes per
// non-zero the kernel no longer sits on the fabric but on the rate at which the CU's address unit takes per-lane loads
// (measured with one byte / short / gather load per element: 84 MB moved in 34 us against 238 MB in 44 us).
// Same products in the same order as sell_row_sum<0, 8, true>: bit-identical to the fp64-value operand.
__device__ __forceinline__ double sell_row_sum_vc(const SellParams& p, const double* __restrict__ x, int64_t b0, int64_t b1,
                                                  int lane, const double* vt) {
  double s0 = 0.0, s1 = 0.0;
  const int width = (int)((b1 - b0) >> 6);     // a multiple of 4
  const uint32_t* __restrict__ code4 = reinterpret_cast<const uint32_t*>(p.code8 + b0) + lane;
  const uint2* __restrict__ delta4 = reinterpret_cast<const uint2*>(p.col16 + b0) + lane;
  int cbl = 0, kb = -64;
  for (int k0 = 0; k0 < width; k0 += 8) {
    if ((k0 & ~63) != kb) {
      kb = k0 & ~63;
      const int64_t cbi = (b0 >> 6) + kb + lane;
      cbl = cbi < (b1 >> 6) ? p.colbase[cbi] : 0;
    }
    const bool two = k0 + 4 < width;
    const uint32_t cw0 = code4[(k0 >> 2) * 64];
    const uint2 dw0 = delta4[(k0 >> 2) * 64];
    uint32_t cw1 = 0;
    uint2 dw1 = make_uint2(0u, 0u);
    if (two) {
      cw1 = code4[((k0 >> 2) + 1) * 64];
      dw1 = delta4[((k0 >> 2) + 1) * 64];
    }
    int c[8];
    double g[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const uint2 dw = u < 4 ? dw0 : dw1;
      const uint32_t half = (u & 2) ? dw.y : dw.x;
      c[u] = __builtin_amdgcn_readlane(cbl, (k0 + u) & 63) + (int)((half >> (16 * (u & 1))) & 0xffffu);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) g[u] = (u < 4 || two) ? x[c[u]] : 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (u < 4 || two) {
        const double v = vt[((u < 4 ? cw0 : cw1) >> (8 * (u & 3))) & 255u];
        if (u & 1) s1 = fma(v, g[u], s1);
        else s0 = fma(v, g[u], s0);
      }
    }
  }
  return s0 + s1;
}

// fp64 values with the per-element arrays packed TWO slice columns to a lane (dsea_op_create_sell16p2): element (column
// 2 G + j, lane l) of a slice sits at 128 G + 2 l + j -- a lane reads its two values as one 16-byte load and its two column
// deltas as one uint32: 4 instead of 6 memory instructions per two non-zeros of a row (section 12.9: beside the matrix stream
// the kernel sits on the rate at which a CU takes per-lane loads).  Same products in the same order as sell_row_sum<.., 8, true>.
template <int MODE>
__device__ __forceinline__ double sell_row_sum_p2(const SellParams& p, const double* __restrict__ x, int64_t b0, int64_t b1,
                                                  int lane) {
  double s0 = 0.0, s1 = 0.0;
  const int width = (int)((b1 - b0) >> 6);     // even
  const double2* __restrict__ val2 = reinterpret_cast<const double2*>(p.vals + b0) + lane;
  const uint32_t* __restrict__ del2 = reinterpret_cast<const uint32_t*>(p.col16 + b0) + lane;
  int cbl = 0, kb = -64;
  for (int k0 = 0; k0 < width; k0 += 8) {
    if ((k0 & ~63) != kb) {
      kb = k0 & ~63;
      const int64_t cbi = (b0 >> 6) + kb + lane;
      cbl = cbi < (b1 >> 6) ? p.colbase[cbi] : 0;
    }
    double2 v[4];
    uint32_t d[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      v[g] = make_double2(0.0, 0.0);
      d[g] = 0u;
      if (k0 + 2 * g < width) {
        v[g] = val2[((k0 >> 1) + g) * 64];
        d[g] = del2[((k0 >> 1) + g) * 64];
      }
    }
    double gx[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int c = __builtin_amdgcn_readlane(cbl, (k0 + u) & 63) + (int)((d[u >> 1] >> (16 * (u & 1))) & 0xffffu);
      gx[u] = (k0 + (u & ~1) < width) ? sell_gather<MODE>(p, x, c) : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (k0 + (u & ~1) < width) {
        const double vv = (u & 1) ? v[u >> 1].y : v[u >> 1].x;
        if (u & 1) s1 = fma(vv, gx[u], s1);
        else s0 = fma(vv, gx[u], s0);
      }
    }
  }
  return s0 + s1;
}

template <bool FUSED, int MODE, int UN, bool C16, bool NT = false, bool VC = false, bool P2 = false>
__global__ __launch_bounds__(256) void k_spmv_sell(SellParams p, const double* __restrict__ x,
                                                   double* __restrict__ y, const double* __restrict__ shift,
                                                   const double* __restrict__ skip, double* __restrict__ P,
                                                   TfimFusedArgs fa) {
  __shared__ double sm5[5];
  __shared__ double vt[VC ? 256 : 1];
  if (!FUSED && skip && skip[0] != 0.0) return;
  if (VC) {
    vt[threadIdx.x] = p.vtab[threadIdx.x];
    __syncthreads();
  }
  const double s = shift ? shift[0] : 0.0;
  const int lane = threadIdx.x & 63;
  double acc = 0.0, beta = 1.0;
  auto finish = [&](int64_t sl, double v) {
    const int64_t row = sl * 64 + lane;
    if (row < p.n) {
      double xi = x[row];
      if (FUSED) {
        xi = xi / beta;
        v = v / beta;
        fa.q_out[row] = xi;
        st_shadow(fa.qs_out, row, xi);
      }
      if (!FUSED && shift) v = __dsub_rn(v, __dmul_rn(s, xi));
      y[row] = v;
      acc = fma(xi, v, acc);
    }
  };
  const int64_t ntrip = p.xcd ? ((p.nslices + 3) / 4 + 7) / 8 * 8 * 4 : p.nslices;
  const int64_t lin0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  // First trip.  Lanczos tail (x is the un-normalised r; q = r/beta is stored, u = (A r)/beta): by linearity the row sums
  // need no beta, so the wait for the ||r||^2 partials (a block-wide reduction with two barriers) sits BEHIND the matrix
  // stream of the wave's first slice instead of in front of it; nothing has been written when a breakdown returns.
  int64_t sl = lin0 < ntrip ? sell_slice_of(p, lin0) : p.nslices;
  double v0 = 0.0;
  constexpr bool p2 = P2;
  if (sl < p.nslices)
    v0 = VC   ? sell_row_sum_vc(p, x, p.slice_ptr[sl], p.slice_ptr[sl + 1], lane, vt)
         : p2 ? sell_row_sum_p2<MODE>(p, x, p.slice_ptr[sl], p.slice_ptr[sl + 1], lane)
              : sell_row_sum<MODE, UN, C16, NT>(p, x, p.slice_ptr[sl], p.slice_ptr[sl + 1], lane);
  // (measured and dropped, round 6 -- every variant same box, alternated: every WAVE summing the partials itself, after the row
  //  sums 52 -> 59 us, with its loads in front of the matrix stream 52 -> 57-58 us; the block version with its loads in front of
  //  the stream: no change.  With beta a constant the tail takes 49 us, without its q / shadow stores 50 / 51: profiles/r06_kbench_csr.txt)
  if (FUSED && !fused_beta(fa, sm5, beta)) return;
  if (sl < p.nslices) finish(sl, v0);
  for (int64_t lin = lin0 + (int64_t)gridDim.x * 4; lin < ntrip; lin += (int64_t)gridDim.x * 4) {
    sl = sell_slice_of(p, lin);
    if (sl >= p.nslices) continue;
    finish(sl, VC   ? sell_row_sum_vc(p, x, p.slice_ptr[sl], p.slice_ptr[sl + 1], lane, vt)
               : p2 ? sell_row_sum_p2<MODE>(p, x, p.slice_ptr[sl], p.slice_ptr[sl + 1], lane)
                    : sell_row_sum<MODE, UN, C16, NT>(p, x, p.slice_ptr[sl], p.slice_ptr[sl + 1], lane));
  }
  if (P) {
    __syncthreads();
    double tot = block_sum(acc, sm5);
    if (threadIdx.x == 0) P[blockIdx.x] = tot;
  }
}

static inline int sell_blocks(const SellParams& p) {   // four 64-row slices (one per wave) to a block
  int64_t nb = (p.nslices + 3) / 4;
  if (nb > DSEA_MAX_TFIM_BLOCKS) nb = DSEA_MAX_TFIM_BLOCKS;
  if (nb < 1) nb = 1;
  return (int)nb;
}

// The SELL mat-vec: which kernel serves which storage form, plain or with the Lanczos tail (fa).  The fused tail exists
// for mode 0 only (has_fused_tail), so the slab modes are not instantiated for it.  Returns the number of partials.
template <bool FUSED>
static int launch_sell(const OpDesc& op, const double* x, double* y, const double* shift, const double* skip, double* P,
                       const TfimFusedArgs& fa, hipStream_t st, EventPair* ev) {
  const SellParams& p = op.sell;
  const int nb = sell_blocks(p);
  auto go = [&](auto kernel) { klaunch(ev, kernel, nb, 256, 0, st, p, x, y, shift, skip, P, fa); };
  auto pick = [&](auto mode) {
    constexpr int M = decltype(mode)::value;
    if (p.pack2) {
      go(k_spmv_sell<FUSED, M, 8, true, false, false, true>);
    } else if constexpr (M != 0) {
      if (p.col16) go(k_spmv_sell<FUSED, M, 8, true>);
      else go(k_spmv_sell<FUSED, M, 4, false>);
    } else if (p.col16) {
      if (p.code8) go(k_spmv_sell<FUSED, 0, 8, true, false, true>);
      else if (p.nt) go(k_spmv_sell<FUSED, 0, 8, true, true>);
      else go(k_spmv_sell<FUSED, 0, 8, true>);
    } else if (op.tune_sell_unroll == 1) {
      go(k_spmv_sell_r5<FUSED>);
    } else {
      dispatch_int<2, 8, 4>(op.tune_sell_unroll, [&](auto un) { go(k_spmv_sell<FUSED, 0, decltype(un)::value, false>); });
    }
  };
  if constexpr (FUSED) pick(int_c<0>{});
  else dispatch_int<1, 2, 0>(p.mode, pick);
  return nb;
}

// The explicit-matrix operand as a PARAMETER (reference symeig.py:29,56-64,82-84: A-bar = v1 v2^T pushed to the parameters
// of A; for a sparse A whose parameters are its non-zeros that is vals-bar[e] = v1[row(e)] v2[col(e)]).  Both kernels walk
// the SELL copy (coalesced column indices) and address the caller's CSR arrays through rowptr: entry k of row i is CSR
// element rowptr[i] + k.
//   k_sell_update_vals : vals_sell[slice, k, lane] = vals_csr[rowptr[row] + k]        (in-place refresh, padding stays 0)
//   k_sell_sddmm       : out[rowptr[row] + k] (+)= alpha * v1[row] * v2[col]   (SYM: alpha/2 (v1[row] v2[col] + v1[col] v2[row]))
#define SELL_SEG_CAP 2048   /* doubles of LDS per wave at most: CSR segments of 64 rows up to 32 non-zeros per row on average */
// LDS per wave of a launch: the widest slice of the operand if the host said so (dsea_op_set_tuning DSEA_TUNE_SELL_MAX_WIDTH --
// 64 KB per workgroup are two workgroups per CU, and both kernels are latency-bound), else the cap; a segment beyond it takes
// the direct form either way
static inline int sell_seg_cap(const SellParams& p) {
  if (p.max_width <= 0) return SELL_SEG_CAP;
  const int64_t need = ((int64_t)p.max_width * 64 + 63) / 64 * 64;
  return (int)(need < 256 ? 256 : (need > SELL_SEG_CAP ? SELL_SEG_CAP : need));
}
// Both kernels move a slice's values between the SELL order (lane = row, coalesced) and the caller's CSR order, where
// the 64 rows of a slice are ONE contiguous segment [rowptr[r0], rowptr[r0 + 64)): the segment is staged in LDS so that
// both sides are coalesced (measured at L = 20 without the staging: 514 us sddmm / 216 us update -- the per-lane CSR
// accesses are 168 bytes apart).  Segments beyond SELL_SEG_CAP use the direct form.
// Every loop of the two kernels works on EIGHT elements per lane and trip with the loads of a trip issued together: written
// one element per iteration they ran one dependent memory round trip per element (sddmm: two -- column, then gather) at two
// waves per SIMD, 18 us per slice and wave.
__global__ __launch_bounds__(256) void k_sell_update_vals(SellParams p, const int64_t* __restrict__ rowptr,
                                                          const double* __restrict__ vals_csr, double* __restrict__ vals_sell,
                                                          int cap) {
  extern __shared__ double seg_all[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double* __restrict__ segw = seg_all + (int64_t)w * cap;
  for (int64_t sl = (int64_t)blockIdx.x * 4 + w; sl < p.nslices; sl += (int64_t)gridDim.x * 4) {
    const int64_t b0 = p.slice_ptr[sl], b1 = p.slice_ptr[sl + 1];
    const int64_t r0 = sl * 64, r1 = r0 + 64 < p.n ? r0 + 64 : p.n;
    const int64_t row = r0 + lane;
    const int64_t lo0 = rowptr[r0], hi0 = rowptr[r1];
    int64_t lo = 0, len = 0;
    if (row < p.n) {
      lo = rowptr[row];
      len = rowptr[row + 1] - lo;
    }
    const int64_t seglen = hi0 - lo0;
    const bool staged = seglen <= cap;
    if (staged) {
      const double* __restrict__ src = vals_csr + lo0;
      for (int64_t i0 = lane; i0 < seglen; i0 += 512) {
        double t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = i0 + 64 * u < seglen ? src[i0 + 64 * u] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (i0 + 64 * u < seglen) segw[i0 + 64 * u] = t[u];
      }
    }
    // one wave owns seg[w]: the LDS operations of a wave are executed in order; the fence keeps the compiler from moving them
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int64_t width = (b1 - b0) >> 6;
    const int64_t off = lo - lo0;
    for (int64_t k0 = 0; k0 < width; k0 += 8) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t k = k0 + u;
        t[u] = k < len ? (staged ? segw[off + k] : vals_csr[lo + k]) : 0.0;
      }
      if (p.pack2) {      // a lane's two values of a column pair are neighbours: one 16-byte store (widths are even)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          if (k0 + 2 * g < width)
            *reinterpret_cast<double2*>(vals_sell + b0 + 128 * ((k0 >> 1) + g) + 2 * lane) = make_double2(t[2 * g], t[2 * g + 1]);
      } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int64_t k = k0 + u;
          if (k < width) vals_sell[b0 + 64 * k + lane] = t[u];
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// explicit-matrix operand as a parameter: refresh of the SELL copy / sampled outer product, CSR order through rowptr
int launch_sell_update_vals(const OpDesc& op, const int64_t* rowptr, const double* vals_csr, hipStream_t st) {
  const SellParams& p = op.sell;
  const int cap = sell_seg_cap(p);
  hipLaunchKernelGGL(k_sell_update_vals, dim3(sell_blocks(p)), dim3(256), (size_t)cap * 4 * sizeof(double), st, p, rowptr,
                     vals_csr, const_cast<double*>(p.vals), cap);
  return 0;
}

template <int MODE, bool SYM>
__global__ __launch_bounds__(256) void k_sell_sddmm(SellParams p, const int64_t* __restrict__ rowptr,
                                                    const double* __restrict__ v1, const double* __restrict__ v2,
                                                    double alpha, int accumulate, double* __restrict__ out, int cap) {
  extern __shared__ double seg_all[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double* __restrict__ segw = seg_all + (int64_t)w * cap;
  for (int64_t sl = (int64_t)blockIdx.x * 4 + w; sl < p.nslices; sl += (int64_t)gridDim.x * 4) {
    const int64_t b0 = p.slice_ptr[sl], b1 = p.slice_ptr[sl + 1];
    const int64_t r0 = sl * 64, r1 = r0 + 64 < p.n ? r0 + 64 : p.n;
    const int64_t row = r0 + lane;
    const int64_t lo0 = rowptr[r0], hi0 = rowptr[r1];
    int64_t lo = 0, len = 0;
    double a1 = 0.0, a2 = 0.0;
    if (row < p.n) {
      lo = rowptr[row];
      len = rowptr[row + 1] - lo;
      a1 = v1[row];
      if (SYM) a2 = v2[row];
    }
    const int64_t seglen = hi0 - lo0;
    const bool staged = seglen <= cap;
    const int64_t width = (b1 - b0) >> 6;
    const int64_t off = lo - lo0;
    // the columns of trip t + 1 are requested before the gathers of trip t are consumed (one dependent round trip per trip
    // instead of two)
    // default layout (packed by two): one uint32 of deltas per two columns and the slice-column bases held by the lanes
    // (v_readlane with a wave-uniform index), as in sell_row_sum_p2 -- 4 loads per trip instead of 16
    int cbl = 0, kb = -64;
    const uint32_t* __restrict__ del2 = p.pack2 ? reinterpret_cast<const uint32_t*>(p.col16 + b0) + lane : nullptr;
    auto load_cols = [&](int64_t k0, int* c) {
      if (p.pack2) {
        const int k0i = (int)k0;
        if ((k0i & ~63) != kb) {
          kb = k0i & ~63;
          const int64_t cbi = (b0 >> 6) + kb + lane;
          cbl = cbi < (b1 >> 6) ? p.colbase[cbi] : 0;
        }
        uint32_t d[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) d[g] = k0i + 2 * g < (int)width ? del2[((k0i >> 1) + g) * 64] : 0u;
#pragma unroll
        for (int u = 0; u < 8; ++u)
          c[u] = __builtin_amdgcn_readlane(cbl, (k0i + u) & 63) + (int)((d[u >> 1] >> (16 * (u & 1))) & 0xffffu);
        return;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t k = k0 + u;
        c[u] = 0;
        if (k < len) {
          const int64_t e = b0 + 64 * k + lane;
          // (packed layouts: the 16-bit deltas sit two / four slice columns to a lane, see sell_row_sum_p2 / _vc)
          const int64_t e16 = p.code8   ? ((e & ~(int64_t)255) | ((e & 63) << 2) | ((e >> 6) & 3))
                              : p.pack2 ? ((e & ~(int64_t)127) | ((e & 63) << 1) | ((e >> 6) & 1))
                                        : e;
          c[u] = p.col16 ? p.colbase[e >> 6] + (int)p.col16[e16] : p.colidx[e];
        }
      }
    };
    int c[8], cn[8];
    load_cols(0, c);
    for (int64_t k0 = 0; k0 < width; k0 += 8) {
      double g2[8], g1[8];
      if (k0 + 8 < width) load_cols(k0 + 8, cn);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        g2[u] = g1[u] = 0.0;
        if (k0 + u < len) {
          g2[u] = sell_gather<MODE>(p, v2, c[u]);
          if (SYM) g1[u] = sell_gather<MODE>(p, v1, c[u]);
        }
      }
      double old[8];
      if (!staged && accumulate) {
#pragma unroll
        for (int u = 0; u < 8; ++u) old[u] = k0 + u < len ? out[lo + k0 + u] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t k = k0 + u;
        if (k < len) {
          double g = __dmul_rn(a1, g2[u]);
          if (SYM) g = __dmul_rn(0.5, __dadd_rn(g, __dmul_rn(g1[u], a2)));
          g = __dmul_rn(alpha, g);
          if (staged) segw[off + k] = g;
          else out[lo + k] = accumulate ? __dadd_rn(old[u], g) : g;
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) c[u] = cn[u];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (staged) {
      double* __restrict__ dst = out + lo0;
      for (int64_t i0 = lane; i0 < seglen; i0 += 512) {
        double t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = (accumulate && i0 + 64 * u < seglen) ? dst[i0 + 64 * u] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int64_t i = i0 + 64 * u;
          if (i < seglen) dst[i] = accumulate ? __dadd_rn(t[u], segw[i]) : segw[i];
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// the same on a plain CSR operand: G lanes per row
template <bool SYM>
__global__ __launch_bounds__(256) void k_csr_sddmm(CsrParams p, const double* __restrict__ v1, const double* __restrict__ v2,
                                                   double alpha, int accumulate, double* __restrict__ out) {
  constexpr int G = 8;
  const int sub = threadIdx.x % G;
  const int64_t rows_per_block = 256 / G;
  for (int64_t row = (int64_t)blockIdx.x * rows_per_block + threadIdx.x / G; row < p.n;
       row += (int64_t)gridDim.x * rows_per_block) {
    const int64_t lo = p.rowptr[row], hi = p.rowptr[row + 1];
    const double a1 = v1[row], a2 = SYM ? v2[row] : 0.0;
    for (int64_t e = lo + sub; e < hi; e += G) {
      const int c = p.colidx[e];
      double g = __dmul_rn(a1, v2[c]);
      if (SYM) g = __dmul_rn(0.5, __dadd_rn(g, __dmul_rn(v1[c], a2)));
      g = __dmul_rn(alpha, g);
      out[e] = accumulate ? __dadd_rn(out[e], g) : g;
    }
  }
}

int launch_sddmm(const OpDesc& op, const int64_t* rowptr, const double* v1, const double* v2, double alpha, int accumulate,
                 bool sym, double* out, hipStream_t st) {
  if (op.kind == OP_SELL) {
    const SellParams& p = op.sell;
    if (sym && p.mode != 0) return -1;                    // (the slab driver issues two one-sided launches instead)
    const int cap = sell_seg_cap(p);
    auto go = [&](auto kernel) {
      klaunch(nullptr, kernel, sell_blocks(p), 256, (size_t)cap * 4 * sizeof(double), st, p, rowptr, v1, v2, alpha,
              accumulate, out, cap);
    };
    if (sym) go(k_sell_sddmm<0, true>);
    else dispatch_int<0, 1, 2>(p.mode, [&](auto mode) { go(k_sell_sddmm<decltype(mode)::value, false>); });
    return 0;
  }
  if (op.kind == OP_CSR) {
    const CsrParams& p = op.csr;
    int64_t nb = (p.n + 31) / 32;
    if (nb > DSEA_MAX_EW_BLOCKS) nb = DSEA_MAX_EW_BLOCKS;
    if (nb < 1) nb = 1;
    dispatch_bool(sym, [&](auto s) {
      klaunch(nullptr, k_csr_sddmm<decltype(s)::value>, (unsigned)nb, 256, 0, st, p, v1, v2, alpha, accumulate, out);
    });
    return 0;
  }
  return -1;
}

// 3-point stencil + diagonal (stencil_row, schrodinger1D.py:18-27).
// Geometry ("canonical tile"): a block of 256 threads works on tiles of 512 consecutive rows, thread t on the row
// pair (2t, 2t+1) of the tile -- 16-byte accesses; the two outer neighbours are scalar loads (L1 hits).  With
// one tile per block (n <= 2^21, see ew_blocks) P[tile] is the x.y partial of exactly that tile: the geometry
// the persistent single-launch CG (k_cg_persist_stencil) reproduces bit for bit.

template <bool FUSED>
__global__ __launch_bounds__(256) void k_spmv_stencil3(Stencil3Params p, const double* __restrict__ x,
                                                       double* __restrict__ y,
                                                       const double* __restrict__ shift,
                                                       const double* __restrict__ skip,
                                                       double* __restrict__ P, TfimFusedArgs fa) {
  __shared__ double sm5[5];
  if (!FUSED && skip && skip[0] != 0.0) return;
  double beta = 1.0;
  if (FUSED && !fused_beta(fa, sm5, beta)) return;
  const double s = shift ? shift[0] : 0.0;
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 512;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2; i < p.n; i += stride) {
    double2 xv = ld2<true>(x, i, p.n);
    double dn = (i > 0) ? x[i - 1] : (p.halo_lo ? p.halo_lo[0] : 0.0);
    double up = (i + 2 < p.n) ? x[i + 2] : ((i + 2 == p.n && p.halo_hi) ? p.halo_hi[0] : 0.0);
    if (i + 1 == p.n) up = 0.0;  // odd n: the pair's second row does not exist (its neighbour value is unused)
    const bool has1 = i + 1 < p.n;
    double up0 = has1 ? xv.y : (p.halo_hi ? p.halo_hi[0] : 0.0);  // upper neighbour of row i
    if (FUSED) {  // the same divisions the separate scale kernel would have done: bit-identical q, u
      xv.x = xv.x / beta;
      if (has1) {
        xv.y = xv.y / beta;
        up0 = xv.y;
      }
      if (i > 0) dn = dn / beta;
      if (i + 2 < p.n) up = up / beta;
      st2<true>(fa.q_out, i, p.n, xv);
      st_shadow_x2(fa.qs_out, i, p.n, xv);
    }
    double2 v, Vv = ld2<true>(p.V, i, p.n);
    v.x = stencil_row(p.coef, Vv.x, xv.x, up0, dn);
    v.y = has1 ? stencil_row(p.coef, Vv.y, xv.y, up, xv.x) : 0.0;
    if (!FUSED && shift) {
      v.x = __dsub_rn(v.x, __dmul_rn(s, xv.x));
      v.y = __dsub_rn(v.y, __dmul_rn(s, xv.y));
    }
    st2<true>(y, i, p.n, v);
    acc = fma(xv.x, v.x, acc);
    acc = fma(xv.y, v.y, acc);
  }
  if (P) {
    __syncthreads();
    double tot = block_sum(acc, sm5);
    if (threadIdx.x == 0) P[blockIdx.x] = tot;
  }
}

// ------------------------------------------------------------------------------------------
// Dense SYMMETRIC operand (DominantSymeig, reference symeig.py:15-31 / Lanczos.py:46-49 applies torch.matmul(A, v):
// a GEMV that streams all n^2 elements).  y = A x reading only the UPPER triangle: the matrix is cut into 64 x 64
// tiles, tile (I, J), I <= J, is loaded once (coalesced 16-byte loads along its rows, staged in LDS) and used twice:
//     y_I += A_IJ x_J            (row part)              y_J += A_IJ^T x_I   (column part, I < J)
// Every tile writes its two 64-element results to their own slots of a partial buffer, P2[a][b-block]: slot
// (J, I-block) <- row part, slot (I, J-block) <- column part -- each slot is written exactly once per call, so there
// are no atomics and no zero-fill; k_symv_reduce adds the nb slots of a row in fixed order (deterministic), applies
// the optional shift and leaves the x.y partials.  Bytes: n^2/2 * 8 matrix + 2 * n^2/64 * 8 partials (3 %).
// ------------------------------------------------------------------------------------------
// T = double or float: the MATRIX may be stored in fp32 (reference Lanczos.py:47: the dense path follows A.dtype);
// it is widened on load, vectors and all arithmetic stay fp64 -- no promoted fp64 copy of the matrix is ever made.
// (Two row-streaming variants without the LDS tile -- a block owning 64 rows x 512 columns, waves streaming 16 rows
//  each, 1-2 KB contiguous runs -- were measured at 1.5-2.4 TB/s, i.e. SLOWER than this one-tile-per-block form:
//  many small independent blocks keep more loads in flight than a few long-running ones.)
template <typename T>
__global__ __launch_bounds__(256) void k_symv_upper(SymDenseParams p, const double* __restrict__ x,
                                                    const double* __restrict__ skip) {
  typedef typename std::conditional<sizeof(T) == 8, double2, float2>::type pair_t;
  const T* __restrict__ Am = static_cast<const T*>(p.A);
  __shared__ double tileA[64][65];
  __shared__ double xsI[64], xsJ[64];
  if (skip && skip[0] != 0.0) return;
  const int I = blockIdx.y, J = blockIdx.x;
  if (J < I) return;
  const int t = threadIdx.x;
  const int64_t r0 = (int64_t)I * 64, c0 = (int64_t)J * 64;
  const int c2 = t & 31;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int r = (t >> 5) + 8 * m;
    const int64_t gr = r0 + r, gc = c0 + 2 * c2;
    double vx = 0.0, vy = 0.0;
    if (gr < p.n) {
      const T* __restrict__ src = Am + gr * p.lda + gc;
      if (gc + 1 < p.n) {
        const pair_t pv = *reinterpret_cast<const pair_t*>(src);
        vx = (double)pv.x;
        vy = (double)pv.y;
      } else if (gc < p.n) {
        vx = (double)src[0];
      }
    }
    tileA[r][2 * c2] = vx;
    tileA[r][2 * c2 + 1] = vy;
  }
  if (t < 64) {
    xsI[t] = (r0 + t < p.n) ? x[r0 + t] : 0.0;
    xsJ[t] = (c0 + t < p.n) ? x[c0 + t] : 0.0;
  }
  __syncthreads();
  if (I == J) {   // diagonal tile: only its upper part is data; mirror it
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const int e = t + 256 * m;
      const int r = e >> 6, c = e & 63;
      if (r > c) tileA[r][c] = tileA[c][r];
    }
    __syncthreads();
  }
  const int rr = t >> 2, q = t & 3;
  double s1 = 0.0;
#pragma unroll
  for (int k2 = 0; k2 < 16; ++k2) s1 = fma(tileA[rr][16 * q + k2], xsJ[16 * q + k2], s1);
  s1 += __shfl_xor(s1, 1, 64);
  s1 += __shfl_xor(s1, 2, 64);
  if (q == 0) p.work[(int64_t)J * p.npad + r0 + rr] = s1;
  if (I < J) {
    double s2 = 0.0;
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) s2 = fma(tileA[16 * q + k2][rr], xsI[16 * q + k2], s2);
    s2 += __shfl_xor(s2, 1, 64);
    s2 += __shfl_xor(s2, 2, 64);
    if (q == 0) p.work[(int64_t)I * p.npad + c0 + rr] = s2;
  }
}

// y = sum_a P2[a][:] - shift x ; partial x.y.  One block per 64-row block-row: lane = row, the four waves split the
// nb slots (independent loads, four accumulators each: the slot reads are pipelined instead of forming one serial
// chain) and are combined in fixed order through LDS.
__global__ __launch_bounds__(256) void k_symv_reduce(SymDenseParams p, const double* __restrict__ x,
                                                     double* __restrict__ y, const double* __restrict__ shift,
                                                     const double* __restrict__ skip, double* __restrict__ P) {
  __shared__ double part[4][64];
  __shared__ double sm4[4];
  if (skip && skip[0] != 0.0) return;
  const double s = shift ? shift[0] : 0.0;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double acc = 0.0;
  for (int Ib = blockIdx.x; Ib < p.nb; Ib += gridDim.x) {
    const int64_t i = (int64_t)Ib * 64 + lane;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
    int a = wv;
    for (; a + 12 < p.nb; a += 16) {
      v0 += p.work[(int64_t)a * p.npad + i];
      v1 += p.work[(int64_t)(a + 4) * p.npad + i];
      v2 += p.work[(int64_t)(a + 8) * p.npad + i];
      v3 += p.work[(int64_t)(a + 12) * p.npad + i];
    }
    for (; a < p.nb; a += 4) v0 += p.work[(int64_t)a * p.npad + i];
    __syncthreads();
    part[wv][lane] = (v0 + v1) + (v2 + v3);
    __syncthreads();
    if (wv == 0 && i < p.n) {
      double v = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
      const double xi = x[i];
      if (shift) v = __dsub_rn(v, __dmul_rn(s, xi));
      y[i] = v;
      acc = fma(xi, v, acc);
    }
  }
  __syncthreads();
  const double tot = block_sum(acc, sm4);
  if (P && threadIdx.x == 0) P[blockIdx.x] = tot;
}

// returns the number of partials written (0 when P == nullptr)
int launch_spmv(const OpDesc& op, const double* x, double* y, const double* shift, const double* skip,
                double* P, hipStream_t st, EventPair* ev) {
  const TfimFusedArgs plain = {nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0};
  switch (op.kind) {
    case OP_TFIM: {
      if (op.tfim.L_local == 0) {
        klaunch(ev, k_spmv_tfim_single, 1, 1, 0, st, op.tfim, x, y, shift, skip, P);
        return 1;
      }
      return launch_tfim<false>(op, x, y, shift, skip, P, plain, st, ev);
    }
    case OP_CSR: {
      const CsrParams& p = op.csr;
      const double avg = p.n > 0 ? (double)p.nnz / (double)p.n : 1.0;
      if (op.tune_csr_group == 0 && avg >= 4.0 && avg * CSR_ROWS <= CSR_CAP) {
        // typical sparse operators (a few to ~48 non-zeros per row): coalesced streaming form
        int64_t nbs = (p.n + CSR_ROWS - 1) / CSR_ROWS;
        if (nbs > DSEA_MAX_TFIM_BLOCKS) nbs = DSEA_MAX_TFIM_BLOCKS;
        klaunch(ev, k_spmv_csr_stream, (unsigned)nbs, 256, 0, st, p, x, y, shift, skip, P);
        return (int)nbs;
      }
      int G = 4;
      while (G < 64 && G < avg) G *= 2;
      if (op.tune_csr_group) G = op.tune_csr_group;
      const int64_t rows_per_block = 256 / G;
      int64_t nb = (p.n + rows_per_block - 1) / rows_per_block;
      if (nb > DSEA_MAX_EW_BLOCKS) nb = DSEA_MAX_EW_BLOCKS;
      if (nb < 1) nb = 1;
      dispatch_int<4, 8, 16, 32, 64>(G, [&](auto group) {
        klaunch(ev, k_spmv_csr<decltype(group)::value>, (unsigned)nb, 256, 0, st, p, x, y, shift, skip, P);
      });
      return (int)nb;
    }
    case OP_SELL:
      return launch_sell<false>(op, x, y, shift, skip, P, plain, st, ev);
    case OP_SYMDENSE: {
      const SymDenseParams& p = op.symdense;
      if (p.elem == 4)
        klaunch(ev, k_symv_upper<float>, dim3(p.nb, p.nb), 256, 0, st, p, x, skip);
      else
        klaunch(ev, k_symv_upper<double>, dim3(p.nb, p.nb), 256, 0, st, p, x, skip);
      int64_t nbr = p.nb;
      if (nbr > DSEA_MAX_EW_BLOCKS) nbr = DSEA_MAX_EW_BLOCKS;
      hipLaunchKernelGGL(k_symv_reduce, dim3((unsigned)nbr), dim3(256), 0, st, p, x, y, shift, skip, P);
      return (int)nbr;
    }
    case OP_DENSE:
    case OP_TRANSFER: {
      // GEMM-shaped operands: rocBLAS (dsea_krylov.hip); the shift / x.y tail is one streaming kernel
      if (blas_apply(op, x, y, st) != 0) return -1;
      if (!shift && !P) return 0;
      const int nbk = launch_shift_dot_partials(x, y, shift, skip, op.n, P, st);   // P may be null
      return P ? nbk : 0;
    }
    case OP_STENCIL3: {
      const int nb = tile_blocks(op.st3.n);
      klaunch(ev, k_spmv_stencil3<false>, nb, 256, 0, st, op.st3, x, y, shift, skip, P, plain);
      return nb;
    }
    case OP_CHAIN:
      return launch_spmv_chain(op, x, y, shift, skip, P, st, ev);
    case OP_LATTICE:
      return launch_spmv_lattice(op, x, y, shift, skip, P, st, ev);
    case OP_SECTOR:
      return launch_spmv_sector(op, x, y, shift, skip, P, st, ev);
    case OP_HUBBARD:
      return launch_spmv_hubbard(op, x, y, shift, skip, P, st, ev);
    case OP_SYMSECTOR:
      return launch_spmv_symsector(op, x, y, shift, skip, P, st, ev);
    case OP_PAIRSECTOR:
      return launch_spmv_pairsector(op, x, y, shift, skip, P, st, ev);
  }
  return -1;
}

// Fused Lanczos tail (beta from the ||r||^2 partials, q = r/beta -> Q[i] (+shadow), u = A q, alpha partials)
// for the operator kinds that have one; returns the number of alpha partials or -1 (caller falls back to the
// unfused sequence scale_store + mat-vec + finalize).
int launch_tfim_fused(const OpDesc& op, const double* r, const double* nP, int nCount, double* q_out, double* y,
                      double* beta_store, double* P, hipStream_t st, EventPair* ev, ShadowRow qs_out, double* brk,
                      int step) {
  if (!has_fused_tail(op)) return -1;
  const TfimFusedArgs fa = {nP, nCount, q_out, qs_out, beta_store, brk, step};
  switch (op.kind) {
    case OP_SELL: return launch_sell<true>(op, r, y, nullptr, nullptr, P, fa, st, ev);
    case OP_TFIM: return launch_tfim<true>(op, r, y, nullptr, nullptr, P, fa, st, ev);
    default: {   // OP_STENCIL3
      const int nb = tile_blocks(op.st3.n);
      klaunch(ev, k_spmv_stencil3<true>, nb, 256, 0, st, op.st3, r, y, nullptr, nullptr, P, fa);
      return nb;
    }
  }
}

}  // namespace dsea
