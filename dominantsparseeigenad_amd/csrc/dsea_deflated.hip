// dsea_deflated.hip -- gfx950 kernels of the lowest-nev eigenpairs (docs/design/13-lowest-eigenpairs.md).
//
//   * block Ritz combine: Y[c] = sum_{j<k} S[c*lds + j] Q[j] for c < m in ONE pass over the basis (m accumulators per
//     row in registers).  Per row, each column is accumulated with exactly the operations and in exactly the order of
//     k_axpy_norm<RPL, 1> (tiled form: descending j, one fma per vector) / k_axpy_norm_split<W, 1> (small-n form: chunks
//     of four vectors dealt to W waves, wave partials summed in wave order): every column is bit-identical to
//     dsea_ritz_combine with that column of S.  The tiled form's rows per lane only change which wave owns a row, not
//     the row's arithmetic, so it is capped by m to bound the accumulator registers.
//   * block projection: out = v - Psi (Psi^T v), the m dot products as per-block partials, summed in the prologue of
//     the apply pass (every block sums the same partials in the same order).
//   * deflated CG (A - shift I) y = P b on range(P), P = I - Psi Psi^T: the update pass folds the m dot products
//     Psi^T r into its partial sums, the re-projection pass applies them and produces the partial ||P r||^2 from the
//     projected vector; the direction pass is the streaming CG's own (k_cg_direction_fused).
//
// Vector stores only; nothing here is shared with an existing entry point's code path.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_internal.h"
#include "dsea_device.h"

namespace dsea {

// ------------------------------------------------------------------------------------------
// block Ritz combine, tiled form (n beyond the split regime)
// ------------------------------------------------------------------------------------------
template <int RPL, int M, bool GUARD>
__device__ __forceinline__ void ritzb_tile(const double* __restrict__ Q, int64_t ldq, int k, int64_t n, int64_t base,
                                           int lane, const double* __restrict__ S, int64_t lds,
                                           double* __restrict__ Y, int64_t ldy) {
  constexpr int NP = RPL / 2;
  double2 w[M][NP];
#pragma unroll
  for (int c = 0; c < M; ++c)
#pragma unroll
    for (int t = 0; t < NP; ++t) w[c][t] = make_double2(0.0, 0.0);
  // descending j, as axpy_tile (the dots pass that precedes a Ritz combine streamed Q ascending)
#pragma unroll 2
  for (int jj = 0; jj < k; ++jj) {
    const int j = k - 1 - jj;
    const double* __restrict__ qj = Q + (int64_t)j * ldq;
    double cj[M];
#pragma unroll
    for (int c = 0; c < M; ++c) cj[c] = S[(int64_t)c * lds + j];
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      const int64_t row = base + t * 128 + lane * 2;
      const double2 q = ld2_stream<GUARD>(qj, row, n);
#pragma unroll
      for (int c = 0; c < M; ++c) {
        w[c][t].x = fma(cj[c], q.x, w[c][t].x);
        w[c][t].y = fma(cj[c], q.y, w[c][t].y);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < M; ++c)
#pragma unroll
    for (int t = 0; t < NP; ++t) st2<GUARD>(Y + (int64_t)c * ldy, base + t * 128 + lane * 2, n, w[c][t]);
}

template <int RPL, int M>
__global__ __launch_bounds__(256) void k_ritz_block(const double* __restrict__ Q, int64_t ldq, int k, int64_t n,
                                                    const double* __restrict__ S, int64_t lds, double* __restrict__ Y,
                                                    int64_t ldy, int nw, int64_t ntiles) {
  const int lane = threadIdx.x & 63;
  const int64_t widx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (widx >= nw) return;
  constexpr int64_t TILE = 64 * RPL;
  for (int64_t tile = widx; tile < ntiles; tile += nw) {
    const int64_t base = tile * TILE;
    if (base + TILE <= n)
      ritzb_tile<RPL, M, false>(Q, ldq, k, n, base, lane, S, lds, Y, ldy);
    else
      ritzb_tile<RPL, M, true>(Q, ldq, k, n, base, lane, S, lds, Y, ldy);
  }
}

// small-n form: W waves share one 128-row tile, chunk c of four basis vectors goes to wave c mod W (k_axpy_norm_split)
template <int W>
__global__ __launch_bounds__(W * 64) void k_ritz_block_split(const double* __restrict__ Q, int64_t ldq, int k,
                                                             int64_t n, const double* __restrict__ S, int64_t lds,
                                                             int m, double* __restrict__ Y, int64_t ldy) {
  __shared__ double2 part[W][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 128 + lane * 2;
  double2 w[DSEA_MAX_NEV];
#pragma unroll
  for (int c = 0; c < DSEA_MAX_NEV; ++c) w[c] = make_double2(0.0, 0.0);
  const int nchunks = (k + 3) / 4;
  for (int cc = wv; cc < nchunks; cc += W) {
    const int j = 4 * cc;
    double2 q[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      q[v] = make_double2(0.0, 0.0);
      if (j + v < k) q[v] = ld2_stream<true>(Q + (int64_t)(j + v) * ldq, row, n);
    }
#pragma unroll
    for (int c = 0; c < DSEA_MAX_NEV; ++c) {
      if (c < m) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const double cj = (j + v < k) ? S[(int64_t)c * lds + j + v] : 0.0;
          w[c].x = fma(cj, q[v].x, w[c].x);
          w[c].y = fma(cj, q[v].y, w[c].y);
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < DSEA_MAX_NEV; ++c) {
    if (c < m) {
      part[wv][lane] = w[c];
      __syncthreads();
      if (wv == 0) {
        double2 tot = part[0][lane];
#pragma unroll
        for (int k2 = 1; k2 < W; ++k2) {
          tot.x += part[k2][lane].x;
          tot.y += part[k2][lane].y;
        }
        st2<true>(Y + (int64_t)c * ldy, row, n, tot);
      }
      __syncthreads();
    }
  }
}

void launch_ritz_block(const TileGeom& g, const double* Q, int64_t ldq, int64_t n, int k, const double* S, int64_t lds,
                       int m, double* Y, int64_t ldy, hipStream_t st) {
  if (g.split_w) {
    dispatch_split_w(g.split_w, [&](auto w) {
      constexpr int W = decltype(w)::value;
      klaunch(nullptr, k_ritz_block_split<W>, (unsigned)g.ntiles, W * 64, 0, st, Q, ldq, k, n, S, lds, m, Y, ldy);
    });
    return;
  }
  dispatch_int<1, 2, 3, 4, 5, 6, 7, 8>(m, [&](auto cols) {
    constexpr int M = decltype(cols)::value;
    // accumulator registers: M * RPL doubles per lane, kept at <= 32
    constexpr int CAP = M <= 2 ? 16 : (M <= 4 ? 8 : 4);
    dispatch_rpl(g.rpl < CAP ? g.rpl : CAP, [&](auto rpl) {
      constexpr int RPL = decltype(rpl)::value;
      if constexpr (RPL <= CAP) {
        int64_t ntiles = (n + 64 * RPL - 1) / (64 * RPL);
        if (ntiles < 1) ntiles = 1;
        const int nw = (int)(ntiles < DSEA_MAX_WAVE_TILES ? ntiles : DSEA_MAX_WAVE_TILES);
        klaunch(nullptr, k_ritz_block<RPL, M>, (nw + 3) / 4, 256, 0, st, Q, ldq, k, n, S, lds, Y, ldy, nw, ntiles);
      }
    });
  });
}

// ------------------------------------------------------------------------------------------
// block projection and the deflated CG passes
// ------------------------------------------------------------------------------------------
static inline int dfl_blocks(int64_t n) {   // one 512-row tile per block up to 2^21 rows, then a capped grid stride
  const int64_t nt = (n + 511) / 512;
  if (nt <= DSEA_PERSIST_MAX_TILES) return (int)(nt < 1 ? 1 : nt);
  int64_t nb = (n + 2047) / 2048;
  if (nb > DSEA_MAX_EW_BLOCKS) nb = DSEA_MAX_EW_BLOCKS;
  return (int)nb;
}

// the m per-block partials of psi_j . v -> P[j * pstride + block]
__device__ __forceinline__ void dfl_flush_dots(const double (&acc)[DSEA_MAX_NEV], int m, double* __restrict__ P,
                                               int pstride, double (*sm)[4]) {
#pragma unroll
  for (int j = 0; j < DSEA_MAX_NEV; ++j) {
    if (j < m) {
      const double t = block_sum(acc[j], sm[j]);
      if (threadIdx.x == 0) P[(int64_t)j * pstride + blockIdx.x] = t;
    }
  }
}

__device__ __forceinline__ void dfl_acc_dots(double (&acc)[DSEA_MAX_NEV], const double* __restrict__ Psi, int64_t ldpsi,
                                             int m, int64_t row, int64_t n, double2 v) {
#pragma unroll
  for (int j = 0; j < DSEA_MAX_NEV; ++j) {
    if (j < m) {
      const double2 p = ld2<true>(Psi + (int64_t)j * ldpsi, row, n);
      acc[j] = fma(p.x, v.x, acc[j]);
      acc[j] = fma(p.y, v.y, acc[j]);
    }
  }
}

// partial psi_j . v ;  with r != null first r = b - (Ax - shift x) (shift, x nullable) and the dots of that r
__global__ __launch_bounds__(256) void k_dfl_dots(const double* __restrict__ v, const double* __restrict__ Psi,
                                                  int64_t ldpsi, int m, int64_t n, double* __restrict__ P, int pstride,
                                                  const double* __restrict__ Ax, const double* __restrict__ x,
                                                  const double* __restrict__ shift, double* __restrict__ r) {
  __shared__ double sm[DSEA_MAX_NEV][4];
  double acc[DSEA_MAX_NEV];
#pragma unroll
  for (int j = 0; j < DSEA_MAX_NEV; ++j) acc[j] = 0.0;
  const double s = shift ? shift[0] : 0.0;
  const int64_t stride = (int64_t)gridDim.x * 512;
  for (int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2; row < n; row += stride) {
    double2 vv = ld2<true>(v, row, n);
    if (r) {   // v = b here
      double2 a = ld2<true>(Ax, row, n);
      if (shift) {
        const double2 xv = ld2<true>(x, row, n);
        a.x = __dsub_rn(a.x, __dmul_rn(s, xv.x));
        a.y = __dsub_rn(a.y, __dmul_rn(s, xv.y));
      }
      vv.x = __dsub_rn(vv.x, a.x);
      vv.y = __dsub_rn(vv.y, a.y);
      st2<true>(r, row, n, vv);
    }
    dfl_acc_dots(acc, Psi, ldpsi, m, row, n, vv);
  }
  __syncthreads();
  dfl_flush_dots(acc, m, P, pstride, sm);
}

// c_j = sum of the partials ; out = v - sum_j c_j psi_j ; optional: coef_out[j] = c_j, copy = out, partial ||out||^2.
// done (nullable): a no-op once the CG stop flag is set.
__global__ __launch_bounds__(256) void k_dfl_apply(const double* __restrict__ v, double* __restrict__ out,
                                                   const double* __restrict__ Psi, int64_t ldpsi, int m,
                                                   const double* __restrict__ P, int count, int pstride,
                                                   double* __restrict__ coef_out, double* __restrict__ copy,
                                                   double* __restrict__ rP, const double* __restrict__ done,
                                                   int64_t n) {
  __shared__ double sm5[5];
  __shared__ double sm4[4];
  if (done && done[0] != 0.0) return;
  double c[DSEA_MAX_NEV];
#pragma unroll
  for (int j = 0; j < DSEA_MAX_NEV; ++j) c[j] = (j < m) ? sum_partials_block(P + (int64_t)j * pstride, count, sm5) : 0.0;
  if (coef_out && blockIdx.x == 0 && threadIdx.x < m) {
#pragma unroll
    for (int j = 0; j < DSEA_MAX_NEV; ++j)
      if (j == (int)threadIdx.x) coef_out[j] = c[j];
  }
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 512;
  for (int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2; row < n; row += stride) {
    double2 w = make_double2(0.0, 0.0);
#pragma unroll
    for (int j = 0; j < DSEA_MAX_NEV; ++j) {
      if (j < m) {
        const double2 p = ld2<true>(Psi + (int64_t)j * ldpsi, row, n);
        w.x = fma(c[j], p.x, w.x);
        w.y = fma(c[j], p.y, w.y);
      }
    }
    double2 vv = ld2<true>(v, row, n);
    vv.x = __dsub_rn(vv.x, w.x);
    vv.y = __dsub_rn(vv.y, w.y);
    st2<true>(out, row, n, vv);
    if (copy) st2<true>(copy, row, n, vv);
    acc = fma(vv.x, vv.x, acc);
    acc = fma(vv.y, vv.y, acc);
  }
  if (rP) {
    __syncthreads();
    const double t = block_sum(acc, sm4);
    if (threadIdx.x == 0) rP[blockIdx.x] = t;
  }
}

// x += alpha d ; r -= alpha A'd ; partial psi_j . r  (alpha = rr / d.A'd, d.A'd summed from dP in the prologue)
__global__ __launch_bounds__(256) void k_dfl_update(double* __restrict__ x, double* __restrict__ r,
                                                    const double* __restrict__ d, const double* __restrict__ Ad,
                                                    const double* __restrict__ state, int parity,
                                                    const double* __restrict__ dP, int dCount,
                                                    const double* __restrict__ Psi, int64_t ldpsi, int m, int64_t n,
                                                    double* __restrict__ P, int pstride) {
  __shared__ double sm5[5];
  __shared__ double sm[DSEA_MAX_NEV][4];
  if (state[DSEA_CG_DONE] != 0.0) return;
  const double dAd = sum_partials_block(dP, dCount, sm5);
  const double alpha = state[parity ? DSEA_CG_RRNEW : DSEA_CG_RR] / dAd;
  double acc[DSEA_MAX_NEV];
#pragma unroll
  for (int j = 0; j < DSEA_MAX_NEV; ++j) acc[j] = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 512;
  for (int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2; row < n; row += stride) {
    double2 xv = ld2<true>(x, row, n), rv = ld2<true>(r, row, n);
    const double2 dv = ld2<true>(d, row, n), av = ld2<true>(Ad, row, n);
    xv.x = __dadd_rn(xv.x, __dmul_rn(alpha, dv.x));
    xv.y = __dadd_rn(xv.y, __dmul_rn(alpha, dv.y));
    rv.x = __dsub_rn(rv.x, __dmul_rn(alpha, av.x));
    rv.y = __dsub_rn(rv.y, __dmul_rn(alpha, av.y));
    st2<true>(x, row, n, xv);
    st2<true>(r, row, n, rv);
    dfl_acc_dots(acc, Psi, ldpsi, m, row, n, rv);
  }
  __syncthreads();
  dfl_flush_dots(acc, m, P, pstride, sm);
}

// after a (re)start: state[RR] = ||r||^2 from the partials, the stop flag on ||r|| < eps; iterations kept if keep_iters
__global__ __launch_bounds__(256) void k_dfl_init_check(double* __restrict__ state, const double* __restrict__ rP,
                                                        int count, double eps, int keep_iters) {
  __shared__ double sm5[5];
  const double rr = sum_partials_block(rP, count, sm5);
  if (threadIdx.x == 0) {
    const double it = keep_iters ? state[DSEA_CG_ITERS] : 0.0;
    for (int i = 0; i < DSEA_CG_STATE_LEN; ++i) state[i] = 0.0;
    const double rn = sqrt(rr);
    state[DSEA_CG_RR] = rr;
    state[DSEA_CG_RESNORM] = rn;
    state[DSEA_CG_DONE] = (rn < eps) ? 1.0 : 0.0;
    state[DSEA_CG_ITERS] = it;
  }
}

void launch_block_project(const double* v, const double* Psi, int64_t ldpsi, int m, double* out, double* coef_out,
                          int64_t n, double* P, int pstride, hipStream_t st) {
  const int nb = dfl_blocks(n);
  hipLaunchKernelGGL(k_dfl_dots, dim3(nb), dim3(256), 0, st, v, Psi, ldpsi, m, n, P, pstride, (const double*)nullptr,
                     (const double*)nullptr, (const double*)nullptr, (double*)nullptr);
  hipLaunchKernelGGL(k_dfl_apply, dim3(nb), dim3(256), 0, st, v, out, Psi, ldpsi, m, (const double*)P, nb, pstride,
                     coef_out, (double*)nullptr, (double*)nullptr, (const double*)nullptr, n);
}

void launch_dfl_restart(const double* b, const double* Ax, const double* x, const double* shift, const double* Psi,
                        int64_t ldpsi, int m, double* r, double* d, double* state, double eps, int keep_iters, int64_t n,
                        double* P, int pstride, double* rP, hipStream_t st) {
  const int nb = dfl_blocks(n);
  hipLaunchKernelGGL(k_dfl_dots, dim3(nb), dim3(256), 0, st, b, Psi, ldpsi, m, n, P, pstride, Ax, x, shift, r);
  hipLaunchKernelGGL(k_dfl_apply, dim3(nb), dim3(256), 0, st, (const double*)r, r, Psi, ldpsi, m, (const double*)P, nb,
                     pstride, (double*)nullptr, d, rP, (const double*)nullptr, n);
  hipLaunchKernelGGL(k_dfl_init_check, dim3(1), dim3(256), 0, st, state, (const double*)rP, nb, eps, keep_iters);
}

int launch_dfl_update(double* x, double* r, const double* d, const double* Ad, const double* state, int parity,
                      const double* dP, int dCount, const double* Psi, int64_t ldpsi, int m, int64_t n, double* P,
                      int pstride, hipStream_t st) {
  const int nb = dfl_blocks(n);
  hipLaunchKernelGGL(k_dfl_update, dim3(nb), dim3(256), 0, st, x, r, d, Ad, state, parity, dP, dCount, Psi, ldpsi, m, n,
                     P, pstride);
  return nb;
}

int launch_dfl_reproject(double* r, const double* Psi, int64_t ldpsi, int m, const double* P, int count, int pstride,
                         double* rP, const double* done, int64_t n, hipStream_t st) {
  const int nb = dfl_blocks(n);
  hipLaunchKernelGGL(k_dfl_apply, dim3(nb), dim3(256), 0, st, (const double*)r, r, Psi, ldpsi, m, P, count, pstride,
                     (double*)nullptr, (double*)nullptr, rP, done, n);
  return nb;
}

}  // namespace dsea
