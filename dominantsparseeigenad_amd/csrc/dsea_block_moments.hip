// dsea_block_moments.hip -- Chebyshev moments of a block (docs/design/33-chebyshev-moments.md): k_cheb_moments_finish<R>, the
// driver block_moments_drive and its scratch size.  Nothing here knows the operator: the driver runs the finish kernel after a
// caller's step, the moments kernel of dsea_sector_block.hip, which performs one order of the recurrence
//   T_1 X = s X,  T_{m+1} X = 2 s T_m X - T_{m-1} X,   s = (H - centre) / halfwidth
// and leaves the per-block partials of a_j = l_j . x_j and b_j = l_j . t_j (x = T_{m-1} X, t = T_m X; l = x in self mode, the
// left block in left mode) in P[(which R + j) nblk + block].
//
// Self mode: with T_a T_b = (T_{a+b} + T_{|a-b|}) / 2 and H symmetric,
//   a = <T_{m-1} x | T_{m-1} x> = (mu_{2m-2} + mu_0) / 2,   b = <T_{m-1} x | T_m x> = (mu_{2m-1} + mu_1) / 2
// so order m yields mu_{2m-2} = 2 a - mu_0 and mu_{2m-1} = 2 b - mu_1 (the doubling is exact, the subtraction rounds once), and
// M moments take ceil(M / 2) orders.  Left mode: order m yields mu_m = b; M moments take M - 1 orders.
// Every reduction is wave, block, then the per-block partials summed in index order: no atomics, identical calls give
// identical bits.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_block.h"

namespace dsea {

// One block.  The sums of the 2 R partial rows of order m >= 1 into the moment rows of MU [M, R]; mu_0 and mu_1 are read back
// from the rows that order 1 wrote (the stream orders the launches).  A row past M - 1 is not written.
template <int R>
__global__ __launch_bounds__(256) void k_cheb_moments_finish(const double* __restrict__ P, int count, double* MU, int m, int M,
                                                             int left) {
  __shared__ double sm5[5];
  double a[R], b[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    a[j] = sum_partials_block(P + (int64_t)j * count, count, sm5);
    b[j] = sum_partials_block(P + (int64_t)(R + j) * count, count, sm5);
  }
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    if (m == 1) {
      MU[j] = a[j];
      MU[R + j] = b[j];
    } else if (left) {
      if (m < M) MU[(int64_t)m * R + j] = b[j];
    } else {
      const int64_t even = 2 * (int64_t)m - 2;
      if (even < M) MU[even * R + j] = __dsub_rn(__dmul_rn(2.0, a[j]), MU[j]);
      if (even + 1 < M) MU[(even + 1) * R + j] = __dsub_rn(__dmul_rn(2.0, b[j]), MU[R + j]);
    }
  }
}

// doubles of scratch a moments run may touch at any grid cap: the two partial arrays of one order
int64_t block_moments_scratch_doubles(int64_t n, int R) {
  int64_t nblk = (n + 255) / 256;
  if (nblk > DSEA_MAX_TFIM_BLOCKS) nblk = DSEA_MAX_TFIM_BLOCKS;
  return 2 * (int64_t)R * nblk;
}

// The schedule for any operator: K = ceil(M / 2) orders in self mode, M - 1 in left mode, each the caller's step and one finish
// launch; nothing is read back.  Order 1 is `first` with x = X and out = U; order 2 reads x = U, old = X and writes V; from
// order 3 on old == out, U and V in turn.  On return T_K X is in U for odd K and in V for even K, T_{K-1} X in the other work
// block (X itself for K = 1).  step(x, old, out, first, P) launches, on st and with nblk blocks, one order with its partials in
// P[(which R + j) nblk + block].
int block_moments_drive(int64_t n, int nblk, int R, int M, bool left, const double* X, double* U, double* V, double* MU,
                        double* scratch, hipStream_t st, const BlockMomentsStep& step) {
  (void)n;
  const int K = left ? M - 1 : (M + 1) / 2;
  double* const t[2] = {U, V};                     // T_m lives in t[(m - 1) & 1]
  dispatch_block_width(R, [&](auto r) {
    constexpr int RR = decltype(r)::value;
    for (int m = 1; m <= K; ++m) {
      const double* x = m == 1 ? X : t[m & 1];
      const double* old = m == 2 ? X : t[(m - 1) & 1];
      step(x, old, t[(m - 1) & 1], m == 1 ? 1 : 0, scratch);
      klaunch(nullptr, k_cheb_moments_finish<RR>, 1, 256, 0, st, scratch, nblk, MU, m, M, left ? 1 : 0);
    }
  });
  return 0;
}

}  // namespace dsea
