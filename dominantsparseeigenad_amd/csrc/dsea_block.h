// dsea_block.h -- what a block kernel needs whatever the operator (docs/design/32-block-kernel-parts.md): the row access and
// the partials of a block, the helpers of the a | b << 8 bond table, the tail of the plain and the Lanczos-step mat-vec, the
// accumulator arguments of the Chebyshev kernels, and the host rules of the launchers (grid, width dispatch, bond table).  Used by dsea_sector_block.hip, dsea_hubbard_block.hip,
// dsea_block_lanczos.hip and dsea_block_moments.hip.
//
// A block is an fp64 array [n, R], row-major (element (r, j) at r * R + j), 16-byte aligned, R in {1, 2, 4, 8}.  A family's
// mat-vec kernel forms, one row per thread, diag and sum[j] of the row of H x and hands them to block_spmv_tail after the last
// chunk's gathers are consumed.  The tail is a function of its operands alone: a tail object that carried the output pointer
// cost the Hubbard kernels two registers.
#ifndef DSEA_BLOCK_H
#define DSEA_BLOCK_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_internal.h"
#include "dsea_device.h"

#define DSEA_SBLOCK_STATE 32 /* doubles per copy of the per-column Lanczos state: beta[8], scale[8], alive[8] */

namespace dsea {

// v * (1 - 2 bit), exact: the bit goes into the sign
__device__ __forceinline__ double block_signed(double v, uint64_t bit) {
  return __longlong_as_double(__double_as_longlong(v) ^ (long long)(bit << 63));
}
// a bond table entry e = a | b << 8 against a state word: whether the two sites' bits differ, and the mask that flips both
__device__ __forceinline__ uint64_t block_differ(uint64_t s, uint32_t e) { return ((s >> (e & 255u)) ^ (s >> (e >> 8))) & 1ull; }
__device__ __forceinline__ uint64_t block_mask(uint32_t e) { return (1ull << (e & 255u)) | (1ull << (e >> 8)); }

// one row of a block: R / 2 16-byte loads or stores (one 8-byte access at R = 1)
template <int R>
__device__ __forceinline__ void block_load(double (&v)[R], const double* __restrict__ p, int64_t row) {
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
__device__ __forceinline__ void block_store(double* __restrict__ p, int64_t row, const double (&v)[R]) {
  if constexpr (R == 1) {
    p[row] = v[0];
  } else {
    double2* __restrict__ q = reinterpret_cast<double2*>(p + row * R);
#pragma unroll
    for (int h = 0; h < R / 2; ++h) q[h] = make_double2(v[2 * h], v[2 * h + 1]);
  }
}

// per-block partials of R per-thread sums: wave sums, then the four waves in fixed order; P[j * gridDim.x + block]
template <int R>
__device__ __forceinline__ void block_partials(const double (&acc)[R], double (*sm)[4], double* __restrict__ P) {
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

// The tail of Y = H X, and with LZ that of the Lanczos step: y holds Q_{i-1} on entry and receives W = H x - y diag(beta) (first:
// W = H x, y is not read); acc gathers the thread's part of x_j . W_j.  The kernel sets beta = st[0 .. R) and acc = 0 before its
// row loop and closes the step with block_partials(acc, ...) after it.
template <int R, bool LZ>
__device__ __forceinline__ void block_spmv_tail(double* __restrict__ y, int first, const double (&beta)[R], double (&acc)[R], int64_t r,
                                                const double (&xr)[R], double diag, const double (&sum)[R]) {
  double v[R];
#pragma unroll
  for (int j = 0; j < R; ++j) v[j] = fma(diag, xr[j], sum[j]);
  if constexpr (LZ) {
    if (!first) {
      double old[R];
      block_load<R>(old, y, r);
#pragma unroll
      for (int j = 0; j < R; ++j) v[j] = __dsub_rn(v[j], __dmul_rn(beta[j], old[j]));
    }
#pragma unroll
    for (int j = 0; j < R; ++j) acc[j] = fma(xr[j], v[j], acc[j]);
  }
  block_store<R>(y, r, v);
}

// the per-accumulator arguments of one Chebyshev order, by value
template <int A>
struct ChebAccs {
  double* acc[A];
  double c0[A], c1[A];
};

// one block per 256 rows up to the cap 2^tune_tile_log2 (6 .. 12, 12 at creation: 4096); beyond it blocks walk row ranges
inline int block_blocks(const OpDesc& op) {
  int64_t nblk = (op.n + 255) / 256;
  const int64_t cap = (int64_t)1 << op.tune_tile_log2;
  if (nblk > cap) nblk = cap;
  return (int)nblk;
}

// the one place that turns the run-time R into the template argument
template <class F>
inline void dispatch_block_width(int R, F&& f) { dispatch_int<1, 2, 4, 8>(R, f); }

// the bond table of the kernel arguments: a | b << 8 in the caller's order, 0 past the last bond
inline void block_pack_bonds(uint16_t (&tb)[DSEA_LATTICE_MAX_BONDS], const uint8_t* a, const uint8_t* b, int nb) {
  for (int t = 0; t < DSEA_LATTICE_MAX_BONDS; ++t) tb[t] = t < nb ? (uint16_t)((uint32_t)a[t] | ((uint32_t)b[t] << 8)) : (uint16_t)0;
}

}  // namespace dsea

#endif
