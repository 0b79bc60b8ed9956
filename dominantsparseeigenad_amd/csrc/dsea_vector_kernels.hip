// dsea_vector_kernels.hip -- the elementwise vector kernels of the Lanczos and CG / PCG drivers (grid-stride, double2,
// most with a fused reduction whose second stage is deterministic), each above its launcher.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_internal.h"
#include "dsea_device.h"

namespace dsea {

// ------------------------------------------------------------------------------------------
// streaming elementwise kernels with a fused reduction (grid-stride, double2)
// ------------------------------------------------------------------------------------------

// Generic two-vector reduction kernels.  Each block writes one partial (P[blockIdx.x]).
__global__ __launch_bounds__(256) void k_dot(const double* __restrict__ x, const double* __restrict__ y,
                                             int64_t n, double* __restrict__ P) {
  __shared__ double sm4[4];
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 512;
  for (int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2; row < n; row += stride) {
    double2 a = ld2<true>(x, row, n), b = ld2<true>(y, row, n);
    acc = fma(a.x, b.x, acc);
    acc = fma(a.y, b.y, acc);
  }
  double t = block_sum(acc, sm4);
  if (threadIdx.x == 0) P[blockIdx.x] = t;
}

int launch_dot_partials(const double* x, const double* y, int64_t n, double* P, hipStream_t st) {
  const int nb = ew_blocks(n);
  hipLaunchKernelGGL(k_dot, dim3(nb), dim3(256), 0, st, x, y, n, P);
  return nb;
}

void launch_dot(const double* x, const double* y, int64_t n, double* P, double* out, hipStream_t st) {
  const int nb = launch_dot_partials(x, y, n, P, st);
  launch_finalize1(P, nb, out, st);
}

// y -= shift*x ; partial x.y
__global__ __launch_bounds__(256) void k_shift_dot(const double* __restrict__ x, double* __restrict__ y,
                                                   const double* __restrict__ shift,
                                                   const double* __restrict__ skip, int64_t n,
                                                   double* __restrict__ P) {
  __shared__ double sm4[4];
  if (skip && skip[0] != 0.0) return;
  const double s = shift ? shift[0] : 0.0;
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 512;
  for (int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2; row < n; row += stride) {
    double2 a = ld2<true>(x, row, n), b = ld2<true>(y, row, n);
    b.x = __dsub_rn(b.x, __dmul_rn(s, a.x));
    b.y = __dsub_rn(b.y, __dmul_rn(s, a.y));
    st2<true>(y, row, n, b);
    acc = fma(a.x, b.x, acc);
    acc = fma(a.y, b.y, acc);
  }
  double t = block_sum(acc, sm4);
  if (P && threadIdx.x == 0) P[blockIdx.x] = t;
}

// y -= shift x with the x.y partials LEFT UNSUMMED (the consumer folds the second stage into its prologue); returns their count
int launch_shift_dot_partials(const double* x, double* y, const double* shift, const double* skip, int64_t n, double* P,
                              hipStream_t st) {
  const int nb = ew_blocks(n);
  hipLaunchKernelGGL(k_shift_dot, dim3(nb), dim3(256), 0, st, x, y, shift, skip, n, P);
  return nb;
}

void launch_shift_dot(const double* x, double* y, const double* shift, const double* skip, int64_t n,
                      double* P, double* out, hipStream_t st) {
  const int nb = launch_shift_dot_partials(x, y, shift, skip, n, P, st);
  launch_finalize_slot(P, nb, out, skip, st);
}

// y += (a_host * a_dev) x
__global__ __launch_bounds__(256) void k_axpy(double a_host, const double* __restrict__ a_dev,
                                              const double* __restrict__ x, double* __restrict__ y,
                                              int64_t n) {
  const double a = a_host * (a_dev ? a_dev[0] : 1.0);
  const int64_t stride = (int64_t)gridDim.x * 512;
  for (int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2; row < n; row += stride) {
    double2 xv = ld2<true>(x, row, n), yv = ld2<true>(y, row, n);
    yv.x = fma(a, xv.x, yv.x);
    yv.y = fma(a, xv.y, yv.y);
    st2<true>(y, row, n, yv);
  }
}

void launch_axpy(double a_host, const double* a_dev, const double* x, double* y, int64_t n,
                 hipStream_t st) {
  hipLaunchKernelGGL(k_axpy, dim3(ew_blocks(n)), dim3(256), 0, st, a_host, a_dev, x, y, n);
}

// q = r / sqrt(nrm2) ; beta_out = sqrt(nrm2)
__global__ __launch_bounds__(256) void k_scale_store(const double* __restrict__ r,
                                                     const double* __restrict__ nrm2,
                                                     double* __restrict__ q, double* __restrict__ beta_out,
                                                     int64_t n, ShadowRow qs,
                                                     double* __restrict__ brk, int step) {
  if (broken(brk)) return;
  const double beta = sqrt(nrm2[0]);
  if (beta_out && blockIdx.x == 0 && threadIdx.x == 0) beta_out[0] = beta;
  if (brk && !(beta > DSEA_BREAK_TOL * brk[1])) {  // also catches a NaN beta; same decision in every block
    if (blockIdx.x == 0 && threadIdx.x == 0) brk[0] = (double)step;
    return;
  }
  const int64_t stride = (int64_t)gridDim.x * 512;
  for (int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2; row < n; row += stride) {
    double2 v = ld2<true>(r, row, n);
    v.x = v.x / beta;
    v.y = v.y / beta;
    st2<true>(q, row, n, v);
    st_shadow_x2(qs, row, n, v);
  }
}

void launch_scale_store(const double* r, const double* nrm2, double* q, double* beta_out, int64_t n,
                        hipStream_t st, ShadowRow qs, double* brk, int step) {
  hipLaunchKernelGGL(k_scale_store, dim3(ew_blocks(n)), dim3(256), 0, st, r, nrm2, q, beta_out, n, qs, brk, step);
}

// out = v - (adv) a, adv = *dot (already finalised)
__global__ __launch_bounds__(256) void k_project_apply(const double* __restrict__ v,
                                                       const double* __restrict__ a,
                                                       const double* __restrict__ dot,
                                                       double* __restrict__ out, int64_t n) {
  const double d = dot[0];
  const int64_t stride = (int64_t)gridDim.x * 512;
  for (int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2; row < n; row += stride) {
    double2 vv = ld2<true>(v, row, n), av = ld2<true>(a, row, n);
    vv.x = __dsub_rn(vv.x, __dmul_rn(d, av.x));
    vv.y = __dsub_rn(vv.y, __dmul_rn(d, av.y));
    st2<true>(out, row, n, vv);
  }
}

void launch_project_apply(const double* v, const double* a, const double* dot, double* out, int64_t n,
                          hipStream_t st) {
  hipLaunchKernelGGL(k_project_apply, dim3(ew_blocks(n)), dim3(256), 0, st, v, a, dot, out, n);
}

// ------------------------------------------------------------------------------------------
// row-partitioned mode: remote part of the mat-vec and the normalising tail of a Lanczos step
// ------------------------------------------------------------------------------------------
struct MultiSrc {
  const double* p[6];
  int count;
};

// y += a * (xs[0] + ... + xs[count-1]) - shift * x ; partial x.y
// (TFIM top-bit flips: a = -g, xs = the partner slabs; shift = E0 in the adjoint solve, CG.py:120)
__global__ __launch_bounds__(256) void k_axpy_multi_dot(double a_host, const double* __restrict__ a_dev,
                                                        MultiSrc xs, const double* __restrict__ shift,
                                                        const double* __restrict__ skip,
                                                        const double* __restrict__ x, double* __restrict__ y,
                                                        int64_t n, double* __restrict__ P) {
  __shared__ double sm4[4];
  if (skip && skip[0] != 0.0) return;
  const double a = a_host * (a_dev ? a_dev[0] : 1.0);
  const double s = shift ? shift[0] : 0.0;
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 512;
  for (int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2; row < n; row += stride) {
    double2 yv = ld2<true>(y, row, n), xv = ld2<true>(x, row, n);
    double2 sum = make_double2(0.0, 0.0);
    for (int b = 0; b < xs.count; ++b) {
      double2 t = ld2<true>(xs.p[b], row, n);
      sum.x += t.x;
      sum.y += t.y;
    }
    if (xs.count > 0) {
      yv.x = __dadd_rn(yv.x, __dmul_rn(a, sum.x));
      yv.y = __dadd_rn(yv.y, __dmul_rn(a, sum.y));
    }
    if (shift) {
      yv.x = __dsub_rn(yv.x, __dmul_rn(s, xv.x));
      yv.y = __dsub_rn(yv.y, __dmul_rn(s, xv.y));
    }
    if (xs.count > 0 || shift) st2<true>(y, row, n, yv);
    acc = fma(xv.x, yv.x, acc);
    acc = fma(xv.y, yv.y, acc);
  }
  double t = block_sum(acc, sm4);
  if (threadIdx.x == 0) P[blockIdx.x] = t;
}

void launch_axpy_multi_dot(double a_host, const double* a_dev, const double* const* xs, int count,
                           const double* shift, const double* skip, const double* x, double* y, int64_t n,
                           double* P, double* dot_out, hipStream_t st, const double* pendP, int pendN, double* pendOut) {
  MultiSrc ms;
  ms.count = count;
  for (int b = 0; b < 6; ++b) ms.p[b] = b < count ? xs[b] : nullptr;
  const int nb = ew_blocks(n);
  hipLaunchKernelGGL(k_axpy_multi_dot, dim3(nb), dim3(256), 0, st, a_host, a_dev, ms, shift, skip, x, y, n, P);
  if (pendP) launch_finalize_pair(pendP, pendN, pendOut, P, nb, dot_out, skip, st);
  else launch_finalize_slot(P, nb, dot_out, skip, st);
}

// r = u - alpha q1 - beta q2 (Lanczos.py:61) as a stand-alone pass, written twice: `r` (worked on in place by
// the following dots / correction passes) and `r_copy` (a snapshot the overlapped slab exchange reads from)
__global__ __launch_bounds__(256) void k_form_r(const double* __restrict__ u, const double* __restrict__ q1,
                                                const double* __restrict__ q2, const double* __restrict__ alpha,
                                                const double* __restrict__ beta, double* __restrict__ r,
                                                double* __restrict__ r_copy, int64_t n) {
  const double a = alpha[0];
  const double b = (beta && q2) ? beta[0] : 0.0;
  const int64_t stride = (int64_t)gridDim.x * 512;
  for (int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2; row < n; row += stride) {
    double2 uu = ld2<true>(u, row, n), qa = ld2<true>(q1, row, n);
    double2 qb = make_double2(0.0, 0.0);
    if (q2) qb = ld2<true>(q2, row, n);
    double2 rv;
    rv.x = __dsub_rn(__dsub_rn(uu.x, __dmul_rn(a, qa.x)), __dmul_rn(b, qb.x));
    rv.y = __dsub_rn(__dsub_rn(uu.y, __dmul_rn(a, qa.y)), __dmul_rn(b, qb.y));
    st2<true>(r, row, n, rv);
    if (r_copy) st2<true>(r_copy, row, n, rv);
  }
}

void launch_form_r(const double* u, const double* q1, const double* q2, const double* alpha, const double* beta,
                   double* r, double* r_copy, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_form_r, dim3(ew_blocks(n)), dim3(256), 0, st, u, q1, q2, alpha, beta, r, r_copy, n);
}

// Transposed form of the hypercube exchange (row-partitioned TFIM, P = 2^p ranks): after an all-to-all the
// buffer xT holds, for every source rank s, chunk number `me` of its slab.  Flipping top bit b of the global
// row index maps source rank s to s ^ (1<<b), so the sum over the p top-bit flips is local here:
//     zT[s][m] = sum_{b<p} xT[s ^ (1<<b)][m]
// (a second all-to-all sends zT[s] back to rank s).
__global__ __launch_bounds__(256) void k_hypercube_flipsum(const double* __restrict__ xT, double* __restrict__ zT,
                                                           int P, int p, int64_t chunk) {
  const int64_t total = (int64_t)P * chunk;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
    const int64_t s = e / chunk, m = e - s * chunk;
    double acc = 0.0;
    for (int b = 0; b < p; ++b) acc += xT[(s ^ ((int64_t)1 << b)) * chunk + m];
    zT[e] = acc;
  }
}

void launch_hypercube_flipsum(const double* xT, double* zT, int P, int p, int64_t chunk, hipStream_t st) {
  int64_t nb = ((int64_t)P * chunk + 255) / 256;
  if (nb > DSEA_MAX_EW_BLOCKS) nb = DSEA_MAX_EW_BLOCKS;
  if (nb < 1) nb = 1;
  hipLaunchKernelGGL(k_hypercube_flipsum, dim3((unsigned)nb), dim3(256), 0, st, xT, zT, P, p, chunk);
}

// pair = [||r||^2, r.Ar] (global).  beta = sqrt(pair[0]) ; q = r/beta (+ bf16 shadow) ; u = y/beta ;
// alpha = pair[1]/pair[0]  (= q.Aq by linearity of the mat-vec; Lanczos.py:69-75)
__global__ __launch_bounds__(256) void k_plz_finish(const double* __restrict__ r, const double* __restrict__ y,
                                                    const double* __restrict__ pair, double* __restrict__ q,
                                                    uint16_t* __restrict__ qs, double* __restrict__ u,
                                                    double* __restrict__ alpha_out,
                                                    double* __restrict__ beta_out, int64_t n) {
  const double nrm2 = pair[0];
  const double beta = sqrt(nrm2);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    alpha_out[0] = pair[1] / nrm2;
    if (beta_out) beta_out[0] = beta;
  }
  const int64_t stride = (int64_t)gridDim.x * 512;
  for (int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2; row < n; row += stride) {
    double2 rv = ld2<true>(r, row, n);
    rv.x = rv.x / beta;
    rv.y = rv.y / beta;
    st2<true>(q, row, n, rv);
    if (qs) st_bf16x2(qs, row, n, rv);
    if (u) {        // (u == null: the next dots pass divides y by beta itself -- k_rdots<., ., USCALE>)
      double2 yv = ld2<true>(y, row, n);
      yv.x = yv.x / beta;
      yv.y = yv.y / beta;
      st2<true>(u, row, n, yv);
    }
  }
}

void launch_plz_finish(const double* r, const double* y, const double* pair, double* q, uint16_t* qs, double* u,
                       double* alpha_out, double* beta_out, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_plz_finish, dim3(ew_blocks(n)), dim3(256), 0, st, r, y, pair, q, qs, u, alpha_out,
                     beta_out, n);
}

// k_plz_finish of step i and k_form_r of step i + 1 in ONE pass (the overlapped row-partitioned step, where the
// three-term vector must exist as a stand-alone snapshot before the dots pass): q = r/beta (+ shadow), u = y/beta is NOT
// stored, r' = u - alpha q - beta q_prev written over r and into r_copy.  The same rounded operations in the same order
// as the two kernels it replaces -- bit-identical -- with three vector passes and a launch fewer per step.
__global__ __launch_bounds__(256) void k_plz_finish_form(double* __restrict__ r, const double* __restrict__ y,
                                                         const double* __restrict__ pair, double* __restrict__ q,
                                                         uint16_t* __restrict__ qs, const double* __restrict__ qprev,
                                                         double* __restrict__ alpha_out, double* __restrict__ beta_out,
                                                         double* __restrict__ r_copy, int64_t n) {
  const double nrm2 = pair[0];
  const double beta = sqrt(nrm2);
  const double a = pair[1] / nrm2;
  const double b = qprev ? beta : 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    alpha_out[0] = a;
    if (beta_out) beta_out[0] = beta;
  }
  const int64_t stride = (int64_t)gridDim.x * 512;
  for (int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2; row < n; row += stride) {
    double2 rv = ld2<true>(r, row, n), yv = ld2<true>(y, row, n);
    double2 qb = make_double2(0.0, 0.0);
    if (qprev) qb = ld2<true>(qprev, row, n);
    rv.x = rv.x / beta;
    rv.y = rv.y / beta;
    yv.x = yv.x / beta;
    yv.y = yv.y / beta;
    st2<true>(q, row, n, rv);
    if (qs) st_bf16x2(qs, row, n, rv);
    double2 nv;
    nv.x = __dsub_rn(__dsub_rn(yv.x, __dmul_rn(a, rv.x)), __dmul_rn(b, qb.x));
    nv.y = __dsub_rn(__dsub_rn(yv.y, __dmul_rn(a, rv.y)), __dmul_rn(b, qb.y));
    st2<true>(r, row, n, nv);
    if (r_copy) st2<true>(r_copy, row, n, nv);
  }
}

void launch_plz_finish_form(double* r, const double* y, const double* pair, double* q, uint16_t* qs, const double* qprev,
                            double* alpha_out, double* beta_out, double* r_copy, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_plz_finish_form, dim3(ew_blocks(n)), dim3(256), 0, st, r, y, pair, q, qs, qprev, alpha_out, beta_out,
                     r_copy, n);
}

// ------------------------------------------------------------------------------------------
// Basis-free ("two-pass") Lanczos: the three-term recurrence WITHOUT re-orthogonalisation and without a stored
// basis (an option the reference lacks; it keeps all k vectors and re-orthogonalises against them, Lanczos.py:49,66).
//   r = u - alpha q1 - beta q2 ; partial ||r||^2 ; second pass only: psi += s1 * q1  (Ritz vector accumulated
//   while the recurrence is replayed -- same kernels, same order, hence bit-identical q_j in both passes)
// alpha arrives as the mat-vec's per-block partials (summed here, stored once), as in k_rdots.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_three_term(const double* __restrict__ u, const double* __restrict__ q1,
                                                    const double* __restrict__ q2, const double* __restrict__ aP,
                                                    int aCount, double* __restrict__ a_store,
                                                    const double* __restrict__ beta, double* __restrict__ r,
                                                    double* __restrict__ P, double* __restrict__ psi,
                                                    const double* __restrict__ s1, int64_t n,
                                                    double* __restrict__ brk) {
  __shared__ double sm5[5];
  if (broken(brk)) return;
  const double a = sum_partials_block(aP, aCount, sm5);
  const double b = (beta && q2) ? beta[0] : 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a_store[0] = a;
    if (brk) brk[1] = fmax(brk[1], fmax(fabs(a), fabs(b)));
  }
  const double sc = s1 ? s1[0] : 0.0;
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 512;
  for (int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2; row < n; row += stride) {
    const double2 uu = ld2<true>(u, row, n), qa = ld2<true>(q1, row, n);
    double2 qb = make_double2(0.0, 0.0);
    if (q2) qb = ld2<true>(q2, row, n);
    double2 rv;
    rv.x = __dsub_rn(__dsub_rn(uu.x, __dmul_rn(a, qa.x)), __dmul_rn(b, qb.x));
    rv.y = __dsub_rn(__dsub_rn(uu.y, __dmul_rn(a, qa.y)), __dmul_rn(b, qb.y));
    st2<true>(r, row, n, rv);
    acc = fma(rv.x, rv.x, acc);
    acc = fma(rv.y, rv.y, acc);
    if (psi) {
      double2 pv = ld2<true>(psi, row, n);
      pv.x = fma(sc, qa.x, pv.x);
      pv.y = fma(sc, qa.y, pv.y);
      st2<true>(psi, row, n, pv);
    }
  }
  __syncthreads();
  const double t = block_sum(acc, sm5);
  if (threadIdx.x == 0) P[blockIdx.x] = t;
}

int launch_three_term(const double* u, const double* q1, const double* q2, const double* aP, int aCount,
                      double* a_store, const double* beta, double* r, double* P, double* psi, const double* s1,
                      int64_t n, double* brk, hipStream_t st) {
  const int nb = ew_blocks(n);
  hipLaunchKernelGGL(k_three_term, dim3(nb), dim3(256), 0, st, u, q1, q2, aP, aCount, a_store, beta, r, P, psi, s1, n,
                     brk);
  return nb;
}

// ------------------------------------------------------------------------------------------
// CG kernels (CG.py:24-41)
// ------------------------------------------------------------------------------------------
// r = b - Ax0 ; d = r ; partial r.r
__global__ __launch_bounds__(256) void k_cg_init(const double* __restrict__ b,
                                                 const double* __restrict__ Ax0, double* __restrict__ r,
                                                 double* __restrict__ d, int64_t n,
                                                 double* __restrict__ P) {
  __shared__ double sm4[4];
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 512;
  for (int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2; row < n; row += stride) {
    double2 bv = ld2<true>(b, row, n), av = ld2<true>(Ax0, row, n);
    bv.x -= av.x;
    bv.y -= av.y;
    st2<true>(r, row, n, bv);
    st2<true>(d, row, n, bv);
    acc = fma(bv.x, bv.x, acc);
    acc = fma(bv.y, bv.y, acc);
  }
  double t = block_sum(acc, sm4);
  if (threadIdx.x == 0) P[blockIdx.x] = t;
}

__global__ void k_cg_state_clear(double* __restrict__ state) {
  if (threadIdx.x < DSEA_CG_STATE_LEN) state[threadIdx.x] = 0.0;
}

void launch_cg_init(const double* b, const double* Ax0, double* r, double* d, double* state, int64_t n,
                    double* P, hipStream_t st) {
  const int nb = tile_blocks(n);
  hipLaunchKernelGGL(k_cg_state_clear, dim3(1), dim3(64), 0, st, state);
  hipLaunchKernelGGL(k_cg_init, dim3(nb), dim3(256), 0, st, b, Ax0, r, d, n, P);
  launch_finalize1(P, nb, state + DSEA_CG_RR, st);
}

__global__ void k_cg_init_check(double* __restrict__ state, double eps) {
  const double rn = sqrt(state[DSEA_CG_RR]);
  state[DSEA_CG_RESNORM] = rn;
  state[DSEA_CG_DONE] = (rn < eps) ? 1.0 : 0.0;
  state[DSEA_CG_ITERS] = 0.0;
}

void launch_cg_init_check(double* state, double eps, hipStream_t st) {
  hipLaunchKernelGGL(k_cg_init_check, dim3(1), dim3(1), 0, st, state, eps);
}

// x += alpha d ; r -= alpha Ad ; partial r.r          alpha = rr / dAd
__global__ __launch_bounds__(256) void k_cg_update(double* __restrict__ x, double* __restrict__ r,
                                                   const double* __restrict__ d,
                                                   const double* __restrict__ Ad,
                                                   const double* __restrict__ state, int64_t n,
                                                   double* __restrict__ P) {
  __shared__ double sm4[4];
  if (state[DSEA_CG_DONE] != 0.0) return;
  const double alpha = state[DSEA_CG_RR] / state[DSEA_CG_DAD];
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 512;
  for (int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2; row < n; row += stride) {
    double2 xv = ld2<true>(x, row, n), rv = ld2<true>(r, row, n);
    double2 dv = ld2<true>(d, row, n), av = ld2<true>(Ad, row, n);
    xv.x = __dadd_rn(xv.x, __dmul_rn(alpha, dv.x));
    xv.y = __dadd_rn(xv.y, __dmul_rn(alpha, dv.y));
    rv.x = __dsub_rn(rv.x, __dmul_rn(alpha, av.x));
    rv.y = __dsub_rn(rv.y, __dmul_rn(alpha, av.y));
    st2<true>(x, row, n, xv);
    st2<true>(r, row, n, rv);
    acc = fma(rv.x, rv.x, acc);
    acc = fma(rv.y, rv.y, acc);
  }
  double t = block_sum(acc, sm4);
  if (threadIdx.x == 0) P[blockIdx.x] = t;
}

// stage 2 of the update's reduction; leaves the local sum in state[RRNEW] unless done
__global__ __launch_bounds__(256) void k_cg_finalize_rrnew(const double* __restrict__ P, int count,
                                                           double* __restrict__ state) {
  __shared__ double sm4[4];
  if (state[DSEA_CG_DONE] != 0.0) return;
  double acc = 0.0;
  for (int b = threadIdx.x; b < count; b += 256) acc += P[b];
  double t = block_sum(acc, sm4);
  if (threadIdx.x == 0) state[DSEA_CG_RRNEW] = t;
}

void launch_cg_update(double* x, double* r, const double* d, const double* Ad, double* state, int64_t n,
                      double* P, hipStream_t st) {
  const int nb = ew_blocks(n);
  hipLaunchKernelGGL(k_cg_update, dim3(nb), dim3(256), 0, st, x, r, d, Ad, (const double*)state, n, P);
  hipLaunchKernelGGL(k_cg_finalize_rrnew, dim3(1), dim3(256), 0, st, (const double*)P, nb, state);
}

// same for d.Ad -> state[DAD]
__global__ __launch_bounds__(256) void k_cg_finalize_slot(const double* __restrict__ P, int count,
                                                          double* __restrict__ out,
                                                          const double* __restrict__ skip) {
  __shared__ double sm4[4];
  if (skip && skip[0] != 0.0) return;
  double acc = 0.0;
  for (int b = threadIdx.x; b < count; b += 256) acc += P[b];
  double t = block_sum(acc, sm4);
  if (threadIdx.x == 0) out[0] = t;
}

void launch_finalize_slot(const double* P, int count, double* out, const double* skip, hipStream_t st) {
  hipLaunchKernelGGL(k_cg_finalize_slot, dim3(1), dim3(256), 0, st, P, count, out, skip);
}

__global__ void k_cg_check(double* __restrict__ state, double eps) {
  if (state[DSEA_CG_DONE] != 0.0) return;
  const double rr_new = state[DSEA_CG_RRNEW];
  const double rn = sqrt(rr_new);
  state[DSEA_CG_ITERS] += 1.0;
  state[DSEA_CG_RESNORM] = rn;
  if (rn < eps) {
    state[DSEA_CG_DONE] = 1.0;
  } else {
    state[DSEA_CG_BETA] = rr_new / state[DSEA_CG_RR];
    state[DSEA_CG_RR] = rr_new;
  }
}

void launch_cg_check(double* state, double eps, hipStream_t st) {
  hipLaunchKernelGGL(k_cg_check, dim3(1), dim3(1), 0, st, state, eps);
}

// d = r + beta d
__global__ __launch_bounds__(256) void k_cg_direction(const double* __restrict__ r, double* __restrict__ d,
                                                      const double* __restrict__ state, int64_t n) {
  if (state[DSEA_CG_DONE] != 0.0) return;
  const double beta = state[DSEA_CG_BETA];
  const int64_t stride = (int64_t)gridDim.x * 512;
  for (int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2; row < n; row += stride) {
    double2 rv = ld2<true>(r, row, n), dv = ld2<true>(d, row, n);
    dv.x = __dadd_rn(rv.x, __dmul_rn(beta, dv.x));
    dv.y = __dadd_rn(rv.y, __dmul_rn(beta, dv.y));
    st2<true>(d, row, n, dv);
  }
}

void launch_cg_direction(const double* r, double* d, const double* state, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_cg_direction, dim3(ew_blocks(n)), dim3(256), 0, st, r, d, state, n);
}

// CG with the scalar stages folded into the consumers (3 launches per iteration: mat-vec, update,
// direction).  rr lives in two ping-pong slots of state: cur = parity ? RRNEW : RR.
__global__ __launch_bounds__(256) void k_cg_update_fused(double* __restrict__ x, double* __restrict__ r,
                                                         const double* __restrict__ d,
                                                         const double* __restrict__ Ad,
                                                         const double* __restrict__ state, int parity,
                                                         const double* __restrict__ dP, int dCount,
                                                         int64_t n, double* __restrict__ P) {
  __shared__ double sm5[5];
  // the first tile's rows are requested before the stop flag and the partial sums are waited for (one memory round
  // trip for the prologue instead of two in a row; up to 2^21 rows a block has exactly one tile)
  const int64_t stride = (int64_t)gridDim.x * 512;
  const int64_t row0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
  double2 xv = ld2<true>(x, row0, n), rv = ld2<true>(r, row0, n);
  double2 dv = ld2<true>(d, row0, n), av = ld2<true>(Ad, row0, n);
  if (state[DSEA_CG_DONE] != 0.0) return;
  const double dAd = sum_partials_block(dP, dCount, sm5);
  const double alpha = state[parity ? DSEA_CG_RRNEW : DSEA_CG_RR] / dAd;
  double acc = 0.0;
  for (int64_t row = row0; row < n; row += stride) {
    if (row != row0) {
      xv = ld2<true>(x, row, n);
      rv = ld2<true>(r, row, n);
      dv = ld2<true>(d, row, n);
      av = ld2<true>(Ad, row, n);
    }
    xv.x = __dadd_rn(xv.x, __dmul_rn(alpha, dv.x));
    xv.y = __dadd_rn(xv.y, __dmul_rn(alpha, dv.y));
    rv.x = __dsub_rn(rv.x, __dmul_rn(alpha, av.x));
    rv.y = __dsub_rn(rv.y, __dmul_rn(alpha, av.y));
    st2<true>(x, row, n, xv);
    st2<true>(r, row, n, rv);
    acc = fma(rv.x, rv.x, acc);
    acc = fma(rv.y, rv.y, acc);
  }
  __syncthreads();
  double t = block_sum(acc, sm5);
  if (threadIdx.x == 0) P[blockIdx.x] = t;
}

int launch_cg_update_fused(double* x, double* r, const double* d, const double* Ad, const double* state,
                           int parity, const double* dP, int dCount, int64_t n, double* P, hipStream_t st) {
  const int nb = tile_blocks(n);
  hipLaunchKernelGGL(k_cg_update_fused, dim3(nb), dim3(256), 0, st, x, r, d, Ad, state, parity, dP, dCount, n, P);
  return nb;
}

__global__ __launch_bounds__(256) void k_cg_direction_fused(const double* __restrict__ r,
                                                            double* __restrict__ d,
                                                            double* __restrict__ state, int parity,
                                                            const double* __restrict__ rP, int rCount,
                                                            double eps, int64_t n) {
  __shared__ double sm5[5];
  const int64_t stride = (int64_t)gridDim.x * 512;
  const int64_t row0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
  double2 rv = ld2<true>(r, row0, n), dv = ld2<true>(d, row0, n);       // (requested first, see k_cg_update_fused)
  if (state[DSEA_CG_DONE] != 0.0) return;
  const double rr_new = sum_partials_block(rP, rCount, sm5);
  const double rr = state[parity ? DSEA_CG_RRNEW : DSEA_CG_RR];
  const double rn = sqrt(rr_new);
  const bool conv = rn < eps;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    state[DSEA_CG_ITERS] += 1.0;
    state[DSEA_CG_RESNORM] = rn;
    if (conv) state[DSEA_CG_DONE] = 1.0;
    else state[parity ? DSEA_CG_RR : DSEA_CG_RRNEW] = rr_new;
  }
  if (conv) return;
  const double beta = rr_new / rr;
  for (int64_t row = row0; row < n; row += stride) {
    if (row != row0) {
      rv = ld2<true>(r, row, n);
      dv = ld2<true>(d, row, n);
    }
    dv.x = __dadd_rn(rv.x, __dmul_rn(beta, dv.x));
    dv.y = __dadd_rn(rv.y, __dmul_rn(beta, dv.y));
    st2<true>(d, row, n, dv);
  }
}

void launch_cg_direction_fused(const double* r, double* d, double* state, int parity, const double* rP,
                               int rCount, double eps, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_cg_direction_fused, dim3(tile_blocks(n)), dim3(256), 0, st, r, d, state, parity, rP, rCount,
                     eps, n);
}

// ------------------------------------------------------------------------------------------
// One-reduction CG of the row-partitioned driver (dsea_pop_cg_run, csrc/dsea_partitioned.hip): the Chronopoulos-Gear
// recurrences of dsea_cg_persist_tfim_big.hip <., MERGED = true> as stream kernels -- w = A'r once per iteration,
// gamma = r.r and delta = r.w reduced TOGETHER (one all-reduce per iteration instead of two), s = A'p carried by
// s <- w + beta s.  Same rounded elementwise operations, in the same order, as that kernel.
//   p <- r + beta p ; s <- w + beta s ; x <- x + alpha p ; r <- r - alpha s ; partial r.r
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pcg_update(double* __restrict__ x, double* __restrict__ r,
                                                    double* __restrict__ p, double* __restrict__ s,
                                                    const double* __restrict__ w,
                                                    const double* __restrict__ state, int64_t n,
                                                    double* __restrict__ P) {
  __shared__ double sm4[4];
  if (state[DSEA_CG_DONE] != 0.0) return;
  const double alpha = state[DSEA_CG_ALPHA], beta = state[DSEA_CG_BETA];
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 512;
  for (int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2; row < n; row += stride) {
    double2 xv = ld2<true>(x, row, n), rv = ld2<true>(r, row, n), pv = ld2<true>(p, row, n);
    double2 sv = ld2<true>(s, row, n), wv = ld2<true>(w, row, n);
    pv.x = __dadd_rn(rv.x, __dmul_rn(beta, pv.x));
    pv.y = __dadd_rn(rv.y, __dmul_rn(beta, pv.y));
    sv.x = __dadd_rn(wv.x, __dmul_rn(beta, sv.x));
    sv.y = __dadd_rn(wv.y, __dmul_rn(beta, sv.y));
    xv.x = __dadd_rn(xv.x, __dmul_rn(alpha, pv.x));
    xv.y = __dadd_rn(xv.y, __dmul_rn(alpha, pv.y));
    rv.x = __dsub_rn(rv.x, __dmul_rn(alpha, sv.x));
    rv.y = __dsub_rn(rv.y, __dmul_rn(alpha, sv.y));
    st2<true>(p, row, n, pv);
    st2<true>(s, row, n, sv);
    st2<true>(x, row, n, xv);
    st2<true>(r, row, n, rv);
    acc = fma(rv.x, rv.x, acc);
    acc = fma(rv.y, rv.y, acc);
  }
  double t = block_sum(acc, sm4);
  if (threadIdx.x == 0) P[blockIdx.x] = t;
}

// returns the number of r.r partials left in P (NOT summed: the caller closes them together with the mat-vec's dot)
int launch_pcg_update(double* x, double* r, double* p, double* s, const double* w, const double* state, int64_t n,
                      double* P, hipStream_t st) {
  const int nb = ew_blocks(n);
  hipLaunchKernelGGL(k_pcg_update, dim3(nb), dim3(256), 0, st, x, r, p, s, w, state, n, P);
  return nb;
}

// first = 1: gamma = state[RR] (all-reduced r.r of the start residual), delta = pair[1] -> alpha = gamma / delta, beta = 0
// first = 0: (gamma', delta) = pair (all-reduced): stopping test, beta = gamma'/gamma, alpha = gamma' / (delta - beta gamma'/alpha)
__global__ void k_pcg_scalars(double* __restrict__ state, const double* __restrict__ pair, double eps, int first) {
  if (state[DSEA_CG_DONE] != 0.0) return;
  if (first) {
    state[DSEA_CG_ALPHA] = state[DSEA_CG_RR] / pair[1];
    state[DSEA_CG_BETA] = 0.0;
    return;
  }
  const double gam2 = pair[0], del2 = pair[1];
  const double rn = sqrt(gam2);
  state[DSEA_CG_ITERS] += 1.0;
  state[DSEA_CG_RESNORM] = rn;
  if (rn < eps) {
    state[DSEA_CG_RR] = gam2;
    state[DSEA_CG_DONE] = 1.0;
  } else {
    const double gam = state[DSEA_CG_RR], alpha = state[DSEA_CG_ALPHA];
    const double beta = gam2 / gam;
    state[DSEA_CG_BETA] = beta;
    state[DSEA_CG_ALPHA] = gam2 / (del2 - beta * gam2 / alpha);
    state[DSEA_CG_RR] = gam2;
  }
}

void launch_pcg_scalars(double* state, const double* pair, double eps, int first, hipStream_t st) {
  hipLaunchKernelGGL(k_pcg_scalars, dim3(1), dim3(1), 0, st, state, pair, eps, first);
}

}  // namespace dsea
