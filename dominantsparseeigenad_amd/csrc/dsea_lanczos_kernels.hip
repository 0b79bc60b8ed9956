// dsea_lanczos_kernels.hip -- gfx950 (MI355X, CDNA4) kernels of the dominant-eigenpair hot path: the Lanczos dots and
// correction passes over the Krylov basis, their second-stage reductions, the bf16 shadow pass, the partial
// re-orthogonalisation's estimate and the bandwidth probes, each family above its launcher.
//
// Everything here is bandwidth-bound fp64 vector work (no MFMA): the Krylov basis is streamed
// from HBM with 16-byte coalesced loads (one wave reads 1 KiB per instruction), partial sums are
// reduced inside a wave with cross-lane shuffles, across waves through LDS, and across workgroups
// by a deterministic second stage (no atomics: the reference is bitwise repeatable and so is this).
//
// Geometry of the basis-streaming kernels (the dominant pair, reference Lanczos.py:66):
//   a wave owns a tile of 64*RPL consecutive rows and keeps its piece of r in registers
//   (RPL doubles per lane, as RPL/2 double2); it then walks j = 0..i-1 over the basis vectors
//   Q[j] (vector-contiguous, stride ldq) reading the same rows of each -- every byte of the basis
//   is read exactly once per pass, r is read once and written once.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_internal.h"
#include "dsea_device.h"

namespace dsea {

// ------------------------------------------------------------------------------------------
// stage-2 reductions (deterministic)
// ------------------------------------------------------------------------------------------
// out[0] = sum_{b<count} partials[b]
__global__ __launch_bounds__(256) void k_finalize1(const double* __restrict__ partials, int count,
                                                   double* __restrict__ out) {
  __shared__ double sm4[4];
  double acc = 0.0;
  for (int b = threadIdx.x; b < count; b += 256) acc += partials[b];
  double t = block_sum(acc, sm4);
  if (threadIdx.x == 0) out[0] = t;
}

void launch_finalize1(const double* P, int count, double* out, hipStream_t st) {
  hipLaunchKernelGGL(k_finalize1, dim3(1), dim3(256), 0, st, P, count, out);
}

// two independent sums in ONE launch (block 0: outA[0] = sum PA, block 1: outB[0] = sum PB), each in the order of
// k_finalize1 / k_cg_finalize_slot -- the row-partitioned step closes ||r||^2 and r.Ar together before their all-reduce
__global__ __launch_bounds__(256) void k_finalize_pair(const double* __restrict__ PA, int na, double* __restrict__ outA,
                                                       const double* __restrict__ PB, int nb, double* __restrict__ outB,
                                                       const double* __restrict__ skipB) {
  __shared__ double sm4[4];
  const bool second = blockIdx.x == 1;
  if (second && skipB && skipB[0] != 0.0) return;
  const double* __restrict__ P = second ? PB : PA;
  const int count = second ? nb : na;
  double acc = 0.0;
  for (int b = threadIdx.x; b < count; b += 256) acc += P[b];
  double t = block_sum(acc, sm4);
  if (threadIdx.x == 0) (second ? outB : outA)[0] = t;
}

void launch_finalize_pair(const double* PA, int na, double* outA, const double* PB, int nb, double* outB,
                          const double* skipB, hipStream_t st) {
  hipLaunchKernelGGL(k_finalize_pair, dim3(2), dim3(256), 0, st, PA, na, outA, PB, nb, outB, skipB);
}

// c[j] = sum_{w<nw} P[j*pstride + w]   (one 256-thread block per j, 4 independent loads in flight per lane)
template <bool GATE>
__global__ __launch_bounds__(256) void k_finalize_multi(const double* __restrict__ P, int64_t pstride,
                                                        int nw, double* __restrict__ c,
                                                        const double* __restrict__ brk,
                                                        const double* __restrict__ gate) {
  __shared__ double sm4[4];
  // (the gate is requested together with the break record: one round trip before a gated launch returns, not two)
  const double gate0 = GATE ? gate[0] : 1.0;
  if (broken(brk)) return;
  if (GATE && gate0 == 0.0) return;     // partial re-orthogonalisation: the dots pass did not run on this step
  const int j = blockIdx.x;
  const double* __restrict__ row = P + (int64_t)j * pstride;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int w = threadIdx.x;
  for (; w + 768 < nw; w += 1024) {
    a0 += row[w];
    a1 += row[w + 256];
    a2 += row[w + 512];
    a3 += row[w + 768];
  }
  for (; w < nw; w += 256) a0 += row[w];
  double t = block_sum((a0 + a1) + (a2 + a3), sm4);
  if (threadIdx.x == 0) c[j] = t;
}

// ------------------------------------------------------------------------------------------
// Lanczos phase 1: r = u - alpha q1 - beta q2 ; partial c[j] = Q[j].r     (Lanczos.py:61,66)
// ------------------------------------------------------------------------------------------
template <int NP>
struct RdotsPre {   // the first tile's rows of u, q_{i-1}, q_{i-2}, requested before any scalar is waited for
  double2 uu[NP], qa[NP], qb[NP];
};

// USCALE: u is given UN-SCALED and divided by `usc` on the fly (row-partitioned library step: u = y / beta of
// k_plz_finish is formed here instead of being stored and re-read -- the same IEEE division, bit-identical)
template <int RPL, bool GUARD, bool PRE, bool USCALE = false>
__device__ __forceinline__ void rdots_tile(const double* __restrict__ Q, int64_t ldq, int i, int ii, int64_t n,
                                           int64_t base, int lane, const double* __restrict__ u,
                                           double a, double b, double* __restrict__ r,
                                           double* __restrict__ sP, bool accumulate, bool want_rr,
                                           const RdotsPre<RPL / 2>& pre, double usc = 1.0) {
  // sP: this wave's row of i + 1 partial sums in LDS.  They are NOT stored to global memory inside the loop: on
  // gfx9 loads and stores share the in-order vmcnt counter, so a store issued between two trips makes the next
  // trip's loads wait for the store's acknowledgement from L2 (measured: 12.6 us of a 273 us pass at i = 199 for the
  // 200 eight-byte stores of a wave).  LDS traffic is counted separately (lgkmcnt); the row is flushed once, after the
  // last tile, by k_rdots.
  constexpr int NP = RPL / 2;
  double2 rv[NP];
  const double* __restrict__ q1 = Q + (int64_t)(i - 1) * ldq;
  const double* __restrict__ q2 = (i >= 2) ? Q + (int64_t)(i - 2) * ldq : nullptr;
#pragma unroll
  for (int t = 0; t < NP; ++t) {
    const int64_t row = base + t * 128 + lane * 2;
    double2 uu, qa, qb;
    if (PRE) {
      uu = pre.uu[t];
      qa = pre.qa[t];
      qb = pre.qb[t];
    } else {
      uu = ld2<GUARD>(u, row, n);
      qa = ld2<GUARD>(q1, row, n);
      qb = make_double2(0.0, 0.0);
      if (q2) qb = ld2<GUARD>(q2, row, n);
    }
    if (USCALE) {
      uu.x = uu.x / usc;
      uu.y = uu.y / usc;
    }
    // (u - alpha*q) - beta*q' with each product rounded on its own, as the torch expression does
    rv[t].x = __dsub_rn(__dsub_rn(uu.x, __dmul_rn(a, qa.x)), __dmul_rn(b, qb.x));
    rv[t].y = __dsub_rn(__dsub_rn(uu.y, __dmul_rn(a, qa.y)), __dmul_rn(b, qb.y));
  }
  // (r is written at the END of the tile, from the registers it stays in: stores issued here would sit in front of
  // the first basis loads in the in-order vmcnt accounting and delay them by a store acknowledgement)
  if (want_rr) {  // ||r||^2 before the correction, as pseudo-vector i (scale for the low-precision test)
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      acc = fma(rv[t].x, rv[t].x, acc);
      acc = fma(rv[t].y, rv[t].y, acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) sP[i] = accumulate ? (sP[i] + acc) : acc;
  }
  // four basis vectors per trip: 4*NP independent 16-byte loads in flight per lane, and one
  // transposed butterfly (7 shuffles instead of 24) leaves the four totals in lanes 0/16/32/48.
  // Direction alternates with the step parity (each c_j is an independent dot product, so the results do
  // not depend on it): the pass starts on the vectors the previous pass touched last, which are the ones
  // still resident in the 256 MiB Infinity Cache.
  // (ii = number of basis vectors dotted: i, or 0 on a step the partial re-orthogonalisation skips)
  const int nchunks = ii / 4;
  const bool rev = (i & 1) != 0;
  auto single = [&](int j) {
    const double* __restrict__ qj = Q + (int64_t)j * ldq;
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      double2 q = ld2_stream<GUARD>(qj, base + t * 128 + lane * 2, n);
      acc = fma(q.x, rv[t].x, acc);
      acc = fma(q.y, rv[t].y, acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) sP[j] = accumulate ? (sP[j] + acc) : acc;
  };
  if (rev)
    for (int j = ii - 1; j >= 4 * nchunks; --j) single(j);
  for (int cc = 0; cc < nchunks; ++cc) {
    const int j = 4 * (rev ? nchunks - 1 - cc : cc);
    const double* __restrict__ qj = Q + (int64_t)j * ldq;
    double2 q[4][NP];
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
      for (int t = 0; t < NP; ++t) q[v][t] = ld2_stream<GUARD>(qj + (int64_t)v * ldq, base + t * 128 + lane * 2, n);
    double acc[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      acc[v] = 0.0;
#pragma unroll
      for (int t = 0; t < NP; ++t) {
        acc[v] = fma(q[v][t].x, rv[t].x, acc[v]);
        acc[v] = fma(q[v][t].y, rv[t].y, acc[v]);
      }
    }
    // (four totals without the LDS crossbar: wave_sum4_rows leaves the total of vector j + v in lane 16 v + 15)
    const double bsum = wave_sum4_rows(acc[0], acc[1], acc[2], acc[3]);
    if ((lane & 15) == 15) {
      const int idx = j + (lane >> 4);
      sP[idx] = accumulate ? (sP[idx] + bsum) : bsum;
    }
  }
  if (!rev)
    for (int j = 4 * nchunks; j < ii; ++j) single(j);
#pragma unroll
  for (int t = 0; t < NP; ++t) st2<GUARD>(r, base + t * 128 + lane * 2, n, rv[t]);
}

// SEL: the partial re-orthogonalisation's gate compiled in (sel != null); the default instantiation carries none of it
template <int RPL, bool SEL = false, bool USCALE = false>
__global__ __launch_bounds__(256) void k_rdots(const double* __restrict__ Q, int64_t ldq, int i,
                                               int64_t n, const double* __restrict__ u,
                                               const double* __restrict__ alpha,
                                               const double* __restrict__ beta, double* __restrict__ r,
                                               double* __restrict__ P, int64_t pstride, int nw,
                                               int64_t ntiles, const double* __restrict__ aP, int aCount,
                                               double* __restrict__ a_store, int want_rr,
                                               double* __restrict__ brk, const double* __restrict__ sel,
                                               int sel_exit, const double* __restrict__ uscale) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;                                                     // 4, 2 or 1 waves per block
  if (SEL && sel_exit && sel[0] == 0.0) return;      // partial re-orthogonalisation: nothing to do on this step
  const int64_t widx = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6);
  constexpr int64_t TILE = 64 * RPL;
  extern __shared__ double rdots_lds[];                                                // [wpb waves][i + 1]
  double* __restrict__ sP = rdots_lds + (threadIdx.x >> 6) * (i + 1);
  const int cnt = i + (want_rr ? 1 : 0);
  // The first tile's rows of u, q, q' are requested HERE, before the break record and the alpha partials are waited
  // for: three dependent memory round trips of the prologue become one.
  RdotsPre<RPL / 2> pre;
  const bool pre_ok = widx < nw && widx * TILE + TILE <= n;
  if (pre_ok) {
    const double* __restrict__ q1 = Q + (int64_t)(i - 1) * ldq;
    const double* __restrict__ q2 = (i >= 2) ? Q + (int64_t)(i - 2) * ldq : nullptr;
#pragma unroll
    for (int t = 0; t < RPL / 2; ++t) {
      const int64_t row = widx * TILE + t * 128 + lane * 2;
      pre.uu[t] = ld2<false>(u, row, n);
      pre.qa[t] = ld2<false>(q1, row, n);
      pre.qb[t] = make_double2(0.0, 0.0);
      if (q2) pre.qb[t] = ld2<false>(q2, row, n);
    }
  }
  if (broken(brk)) return;                                                             // (uniform over the block)
  if (widx < nw) {
    // alpha_{i-1}: either finalised already (phase API) or still as the mat-vec's per-block partials
    double a;
    if (aCount > 0) {
      a = sum_partials_wave(aP, aCount, lane);
      if (widx == 0 && lane == 0) a_store[0] = a;
    } else {
      a = alpha[0];
    }
    const double b = beta ? beta[0] : 0.0;
    const double usc = USCALE ? uscale[0] : 1.0;
    // (read by the tail kernel of this step -- a later launch -- only)
    if (brk && widx == 0 && lane == 0) brk[1] = fmax(brk[1], fmax(fabs(a), fabs(b)));
    // partial re-orthogonalisation (dsea_ws_set_partial_reorth): sel[0] == 0 = this step is not re-orthogonalised -- the
    // three-term update and ||r||^2 (row i of P) only; the coefficient rows of P are then NOT written
    const int ii = (SEL && sel[0] == 0.0) ? 0 : i;
    bool first = true;
    for (int64_t tile = widx; tile < ntiles; tile += nw) {
      const int64_t base = tile * TILE;
      if (first && pre_ok)
        rdots_tile<RPL, false, true, USCALE>(Q, ldq, i, ii, n, base, lane, u, a, b, r, sP, false, want_rr != 0, pre, usc);
      else if (base + TILE <= n)
        rdots_tile<RPL, false, false, USCALE>(Q, ldq, i, ii, n, base, lane, u, a, b, r, sP, !first, want_rr != 0, pre, usc);
      else
        rdots_tile<RPL, true, false, USCALE>(Q, ldq, i, ii, n, base, lane, u, a, b, r, sP, !first, want_rr != 0, pre, usc);
      first = false;
    }
  } else {
    for (int idx = lane; idx < cnt; idx += 64) sP[idx] = 0.0;                          // a wave without tiles adds zeros
  }
  // The block's waves are combined in LDS (fixed order w0 + w1 + ...) and ONE partial per block and basis vector is
  // stored: a quarter of the scattered 8-byte stores at the end of the kernel and a quarter of the values the
  // second stage (k_finalize_multi) has to sum.
  __syncthreads();
  const int row0 = (SEL && sel[0] == 0.0) ? i : 0;      // (a skipped step flushes its ||r||^2 row only)
  for (int idx = row0 + threadIdx.x; idx < cnt; idx += blockDim.x) {
    double t = rdots_lds[idx];
    for (int w = 1; w < wpb; ++w) t += rdots_lds[w * (i + 1) + idx];
    P[(int64_t)idx * pstride + blockIdx.x] = t;
  }
}

// ------------------------------------------------------------------------------------------
// Lanczos phase 2: r -= sum_j c[j] Q[j] ; partial ||r||^2          (Lanczos.py:66,69)
// MODE 0: as above.  MODE 1 (Ritz vector, Lanczos.py:99): out = sum_j c[j] Q[j], no norm.
// ------------------------------------------------------------------------------------------
template <int RPL, bool GUARD, int MODE>
__device__ __forceinline__ double axpy_tile(const double* __restrict__ Q, int64_t ldq, int i, int64_t n,
                                            int64_t base, int lane, const double* __restrict__ c,
                                            double* __restrict__ r) {   // i = number of vectors combined
  constexpr int NP = RPL / 2;
  double2 w[NP];
#pragma unroll
  for (int t = 0; t < NP; ++t) w[t] = make_double2(0.0, 0.0);
  // Descending j: the dots pass (ascending) has just streamed Q[0..i-1], so the most recently read
  // vectors are the ones still resident in the 256 MiB Infinity Cache; walking back over them first
  // turns the tail of pass 1 into hits of pass 2 (and leaves Q[0..] resident for the next dots pass).
#pragma unroll 4
  for (int jj = 0; jj < i; ++jj) {
    const int j = i - 1 - jj;
    const double* __restrict__ qj = Q + (int64_t)j * ldq;
    const double cj = c[j];
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      const int64_t row = base + t * 128 + lane * 2;
      double2 q = ld2_stream<GUARD>(qj, row, n);
      w[t].x = fma(cj, q.x, w[t].x);
      w[t].y = fma(cj, q.y, w[t].y);
    }
  }
  double acc = 0.0;
#pragma unroll
  for (int t = 0; t < NP; ++t) {
    const int64_t row = base + t * 128 + lane * 2;
    if (MODE == 0) {
      double2 rv = ld2<GUARD>(r, row, n);
      rv.x -= w[t].x;
      rv.y -= w[t].y;
      st2<GUARD>(r, row, n, rv);
      acc = fma(rv.x, rv.x, acc);
      acc = fma(rv.y, rv.y, acc);
    } else {
      st2<GUARD>(r, row, n, w[t]);
    }
  }
  return acc;
}

template <int RPL, int MODE, bool SEL = false>
__global__ __launch_bounds__(256) void k_axpy_norm(const double* __restrict__ Q, int64_t ldq, int i,
                                                   int64_t n, const double* __restrict__ c,
                                                   double* __restrict__ r, double* __restrict__ P,
                                                   int nw, int64_t ntiles, const double* __restrict__ brk,
                                                   const double* __restrict__ sel) {
  const int lane = threadIdx.x & 63;
  const int64_t widx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (widx >= nw) return;
  const double sel0 = SEL ? sel[0] : 1.0;      // (requested together with the break record)
  if (broken(brk)) return;
  // (SEL is a template parameter: the check, compiled into the default instantiation, cost the fp64 pass 5 % -- 231 -> 244 us
  // at n = 2^20, i = 199 -- through nothing but a different register allocation)
  if (SEL && sel0 == 0.0) {
    // partial re-orthogonalisation: no correction on this step; ||r||^2 is the dots pass's own c[i], handed on in the
    // partial-sum layout the consumer expects (first partial = the value, the others 0)
    if (MODE == 0 && lane == 0) P[widx] = (widx == 0) ? c[i] : 0.0;
    return;
  }
  constexpr int64_t TILE = 64 * RPL;
  double acc = 0.0;
  for (int64_t tile = widx; tile < ntiles; tile += nw) {
    const int64_t base = tile * TILE;
    if (base + TILE <= n)
      acc += axpy_tile<RPL, false, MODE>(Q, ldq, i, n, base, lane, c, r);
    else
      acc += axpy_tile<RPL, true, MODE>(Q, ldq, i, n, base, lane, c, r);
  }
  if (MODE == 0) {
    acc = wave_sum(acc);
    if (lane == 0) P[widx] = acc;
  }
}

// ------------------------------------------------------------------------------------------
// Small-n form of the two passes ("split"): with fewer than ~1000 row tiles a wave that walks all i basis
// vectors alone is bound by the latency of its serial trips, not by bandwidth.  Here a block of W waves shares
// ONE row tile of 128 rows (2 per lane) and splits the basis vectors between its waves in chunks of four
// (chunk c -> wave c mod W).  Dots: every c_j is still produced by exactly one wave (same partial layout).
// Correction: the W partial sums of a tile are combined through LDS in wave order -- deterministic.
// ------------------------------------------------------------------------------------------
template <int W, int NT, bool SEL = false>
__global__ __launch_bounds__(W * 64) void k_rdots_split(const double* __restrict__ Q, int64_t ldq, int i,
                                                        int64_t n, const double* __restrict__ u,
                                                        const double* __restrict__ alpha,
                                                        const double* __restrict__ beta, double* __restrict__ r,
                                                        double* __restrict__ P, int64_t pstride,
                                                        const double* __restrict__ aP, int aCount,
                                                        double* __restrict__ a_store, int want_rr,
                                                        double* __restrict__ brk, const double* __restrict__ sel,
                                                        int sel_exit) {
  if (SEL && sel_exit && sel[0] == 0.0) return;      // partial re-orthogonalisation: nothing to do on this step
  // NT = 128-row sub-tiles per block (NT = 2 beyond 640 tiles: twice the loads in flight per wave trip, half the partials
  // for the second stage).  Requesting a wave's first chunk ahead of the alpha partials was measured and is SLOWER
  // (config 3: 24.8 -> 28.3 us per launch), and forcing 64 VGPRs (two 1024-thread blocks per CU) gains nothing.
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t tile = blockIdx.x;
  const int64_t row = tile * (128 * NT) + lane * 2;
  // (the tile's rows of u, q, q' are requested before the break record and the alpha partials are waited for)
  const double* __restrict__ q1 = Q + (int64_t)(i - 1) * ldq;
  double2 uu[NT], qa[NT], qb[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    uu[t] = ld2<true>(u, row + 128 * t, n);
    qa[t] = ld2<true>(q1, row + 128 * t, n);
    qb[t] = make_double2(0.0, 0.0);
    if (i >= 2) qb[t] = ld2<true>(Q + (int64_t)(i - 2) * ldq, row + 128 * t, n);
  }
  if (broken(brk)) return;
  double a;
  if (aCount > 0) {
    a = sum_partials_wave(aP, aCount, lane);
    if (tile == 0 && wv == 0 && lane == 0) a_store[0] = a;
  } else {
    a = alpha[0];
  }
  const double b = beta ? beta[0] : 0.0;
  if (brk && tile == 0 && wv == 0 && lane == 0) brk[1] = fmax(brk[1], fmax(fabs(a), fabs(b)));
  double2 rv[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    rv[t].x = __dsub_rn(__dsub_rn(uu[t].x, __dmul_rn(a, qa[t].x)), __dmul_rn(b, qb[t].x));
    rv[t].y = __dsub_rn(__dsub_rn(uu[t].y, __dmul_rn(a, qa[t].y)), __dmul_rn(b, qb[t].y));
  }
  // The tile's i (+1) partial sums are collected in LDS and flushed once, r is written at the end from its
  // registers: no global store sits between the trips of a wave (see rdots_tile).
  extern __shared__ double split_lds[];     // [i + 1]
  if (wv == 0 && want_rr) {
    double p = fma(rv[0].x, rv[0].x, rv[0].y * rv[0].y);
#pragma unroll
    for (int t = 1; t < NT; ++t) p += fma(rv[t].x, rv[t].x, rv[t].y * rv[t].y);
    const double acc = wave_sum(p);
    if (lane == 0) split_lds[i] = acc;
  }
  const int ii = (SEL && sel[0] == 0.0) ? 0 : i;     // partial re-orthogonalisation: see k_rdots
  const int nchunks = (ii + 3) / 4;
  for (int cc = wv; cc < nchunks; cc += W) {
    const int j = 4 * cc;
    double2 q[4][NT];
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        q[v][t] = make_double2(0.0, 0.0);
        if (j + v < ii) q[v][t] = ld2_stream<true>(Q + (int64_t)(j + v) * ldq, row + 128 * t, n);
      }
    double acc[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      acc[v] = fma(q[v][0].x, rv[0].x, q[v][0].y * rv[0].y);
#pragma unroll
      for (int t = 1; t < NT; ++t) acc[v] += fma(q[v][t].x, rv[t].x, q[v][t].y * rv[t].y);
    }
    const double bsum = wave_sum4_rows(acc[0], acc[1], acc[2], acc[3]);
    const int jj = j + (lane >> 4);
    if ((lane & 15) == 15 && jj < ii) split_lds[jj] = bsum;
  }
  if (wv == 0) {
#pragma unroll
    for (int t = 0; t < NT; ++t) st2<true>(r, row + 128 * t, n, rv[t]);
  }
  __syncthreads();
  const int cnt = i + (want_rr ? 1 : 0);
  for (int idx = (ii != i ? i : 0) + threadIdx.x; idx < cnt; idx += W * 64) P[(int64_t)idx * pstride + tile] = split_lds[idx];
}

// MODE 0: r -= sum_j c_j Q_j, partial ||r||^2 ; MODE 1: out = sum_j c_j Q_j (Ritz vector)
template <int W, int MODE, bool SEL = false>
__global__ __launch_bounds__(W * 64) void k_axpy_norm_split(const double* __restrict__ Q, int64_t ldq, int i,
                                                            int64_t n, const double* __restrict__ c,
                                                            double* __restrict__ r, double* __restrict__ P,
                                                            const double* __restrict__ brk,
                                                            const double* __restrict__ sel) {
  __shared__ double2 part[W][64];
  const double sel0 = SEL ? sel[0] : 1.0;
  if (broken(brk)) return;
  if (SEL && sel0 == 0.0) {                     // partial re-orthogonalisation: see k_axpy_norm
    if (MODE == 0 && threadIdx.x == 0) P[blockIdx.x] = (blockIdx.x == 0) ? c[i] : 0.0;
    return;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t tile = blockIdx.x;
  const int64_t row = tile * 128 + lane * 2;
  double2 w = make_double2(0.0, 0.0);
  const int nchunks = (i + 3) / 4;
  for (int cc = wv; cc < nchunks; cc += W) {
    const int j = 4 * cc;
    double2 q[4];
    double cj[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      q[v] = make_double2(0.0, 0.0);
      cj[v] = 0.0;
      if (j + v < i) {
        q[v] = ld2_stream<true>(Q + (int64_t)(j + v) * ldq, row, n);
        cj[v] = c[j + v];
      }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      w.x = fma(cj[v], q[v].x, w.x);
      w.y = fma(cj[v], q[v].y, w.y);
    }
  }
  part[wv][lane] = w;
  __syncthreads();
  if (wv == 0) {
    double2 tot = part[0][lane];
#pragma unroll
    for (int k2 = 1; k2 < W; ++k2) {
      tot.x += part[k2][lane].x;
      tot.y += part[k2][lane].y;
    }
    if (MODE == 0) {
      double2 rv = ld2<true>(r, row, n);
      rv.x -= tot.x;
      rv.y -= tot.y;
      st2<true>(r, row, n, rv);
      double acc = wave_sum(fma(rv.x, rv.x, rv.y * rv.y));
      if (lane == 0) P[tile] = acc;
    } else {
      st2<true>(r, row, n, tot);
    }
  }
}

// dots pass, wave-owned form: one row of i + 1 partial sums per wave in LDS (see rdots_tile); 64 KiB of dynamic LDS hold
// 4 waves up to i = 2047, 2 waves up to 4095, 1 wave up to 8191 (dsea_ws_create caps kmax at DSEA_MAX_KRYLOV = 8000)
static inline int rdots_waves_per_block(int i) { return (i + 1) <= 2048 ? 4 : ((i + 1) <= 4096 ? 2 : 1); }

// partials per basis vector the dots pass of step i leaves in P (row stride g.pstride)
int rdots_partial_count(const TileGeom& g, int i) {
  if (g.split_w) return (int)((g.ntiles + g.dots_nt - 1) / g.dots_nt);
  const int wpb = rdots_waves_per_block(i);
  return (g.nw + wpb - 1) / wpb;
}

void launch_rdots(const TileGeom& g, const double* Q, int64_t ldq, int64_t n, int i, const double* u,
                  const double* alpha, const double* beta, double* r, double* P, double* c_out,
                  hipStream_t st, EventPair* ev, const double* aP, int aCount, double* a_store, bool want_rr,
                  double* brk, const double* sel, bool sel_exit, const double* uscale) {
  // (uscale: wave-owned geometry without the partial re-orthogonalisation gate only -- callers check rdots_uscale_ok)
  const int wr = want_rr ? 1 : 0;
  const int count = rdots_partial_count(g, i);
  if (g.split_w) {
    const size_t lds = (size_t)(i + 1) * sizeof(double);     // the tile's partial sums (see k_rdots_split)
    auto go = [&](auto w, auto nt) {
      dispatch_bool(sel != nullptr, [&](auto s) {
        constexpr int W = decltype(w)::value;
        constexpr bool SEL = decltype(s)::value;
        klaunch(ev, k_rdots_split<W, decltype(nt)::value, SEL>, count, W * 64, lds, st, Q, ldq, i, n, u, alpha, beta, r,
                P, g.pstride, aP, aCount, a_store, wr, brk, sel, SEL && sel_exit ? 1 : 0);
      });
    };
    if (g.dots_nt == 2) go(int_c<16>{}, int_c<2>{});
    else dispatch_split_w(g.dots_w, [&](auto w) { go(w, int_c<1>{}); });
  } else {
    const int wpb = rdots_waves_per_block(i);
    const size_t lds = (size_t)wpb * (i + 1) * sizeof(double);
    // the instantiations: plain, SEL (partial re-orthogonalisation gate), USCALE (without the gate only)
    dispatch_int<1, 2, 0>(sel ? 1 : (uscale ? 2 : 0), [&](auto variant) {
      dispatch_rpl(g.rpl, [&](auto rpl) {
        constexpr bool SEL = decltype(variant)::value == 1, USCALE = decltype(variant)::value == 2;
        klaunch(ev, k_rdots<decltype(rpl)::value, SEL, USCALE>, count, 64 * wpb, lds, st, Q, ldq, i, n, u, alpha, beta, r,
                P, g.pstride, g.nw, g.ntiles, aP, aCount, a_store, wr, brk, sel, !USCALE && sel_exit ? 1 : 0,
                USCALE ? uscale : nullptr);
      });
    });
  }
  // want_rr: one more row of partials (||r||^2) -> c_out[i]
  // (c_out null: the caller's next kernel sums the partial rows it needs itself -- rdots_partial_count of them)
  if (c_out)
    dispatch_bool(sel_exit, [&](auto gate) {
      constexpr bool GATE = decltype(gate)::value;
      klaunch(nullptr, k_finalize_multi<GATE>, want_rr ? i + 1 : i, 256, 0, st, P, g.pstride, count, c_out, brk,
              GATE ? sel : nullptr);
    });
}

// r -= Q[0..i) c with the partial ||r||^2 (MODE 0: the correction pass), or out = Q[0..k) s (MODE 1: the Ritz combine,
// which has no gate and no partials)
template <int MODE>
static void launch_axpy_family(const TileGeom& g, const double* Q, int64_t ldq, int64_t n, int i, const double* c,
                               double* r, double* P, hipStream_t st, EventPair* ev, const double* brk,
                               const double* sel) {
  auto go = [&](auto s) {
    constexpr bool SEL = decltype(s)::value;
    if (g.split_w)
      dispatch_split_w(g.split_w, [&](auto w) {
        constexpr int W = decltype(w)::value;
        klaunch(ev, k_axpy_norm_split<W, MODE, SEL>, (unsigned)g.ntiles, W * 64, 0, st, Q, ldq, i, n, c, r, P, brk, sel);
      });
    else
      dispatch_rpl(g.rpl, [&](auto rpl) {
        klaunch(ev, k_axpy_norm<decltype(rpl)::value, MODE, SEL>, (g.nw + 3) / 4, 256, 0, st, Q, ldq, i, n, c, r, P, g.nw,
                g.ntiles, brk, sel);
      });
  };
  if constexpr (MODE == 0) dispatch_bool(sel != nullptr, go);
  else go(std::false_type{});
}

void launch_axpy_norm(const TileGeom& g, const double* Q, int64_t ldq, int64_t n, int i, const double* c,
                      double* r, double* P, double* nrm2_out, hipStream_t st, EventPair* ev, const double* brk,
                      const double* sel) {
  launch_axpy_family<0>(g, Q, ldq, n, i, c, r, P, st, ev, brk, sel);
  if (nrm2_out) launch_finalize1(P, g.nw, nrm2_out, st);  // null: the consumer sums the g.nw partials itself
}

void launch_ritz(const TileGeom& g, const double* Q, int64_t ldq, int64_t n, int k, const double* s,
                 double* out, hipStream_t st) {
  launch_axpy_family<1>(g, Q, ldq, n, k, s, out, nullptr, st, nullptr, nullptr, nullptr);
}

// ------------------------------------------------------------------------------------------
// Lanczos phase 2 reading a bf16 SHADOW of the basis (storage precision only; all arithmetic is fp64).
//
// Why this is exact to working precision: with full re-orthogonalisation every step the coefficients
// c_j = q_j . r are pure rounding residue, max_j |c_j| ~ 1e-16..1e-15 ||r|| (measured on every golden
// case, also at k = n), so the correction  sum_j c_j q_j  sits at the last bit of r.  Reading q_j with a
// relative error of 2^-9 perturbs r by <= 2^-9 max|c_j| ~ 1e-18 ||r||, far below the fp64 rounding of the
// subtraction itself; the next step's dots (always from the fp64 basis) re-measure orthogonality exactly.
// The kernel checks the premise on the device: if max_j |c_j| > tau ||r|| it takes the fp64 basis instead.
// The pass then moves 2 bytes per basis element instead of 8.
//
// Geometry: a lane owns RPS groups of 8 consecutive rows (one 16-byte shadow load each); a wave tile is
// 512*RPS rows.  j runs downwards (most recently streamed vectors first).

// w[e] += cj * (shadow value e of h), fp64 arithmetic
__device__ __forceinline__ void fma_shadow8(double (&w)[8], double cj, uint4 h) {
  w[0] = fma(cj, bf16lo_to_f64(h.x), w[0]);
  w[1] = fma(cj, bf16hi_to_f64(h.x), w[1]);
  w[2] = fma(cj, bf16lo_to_f64(h.y), w[2]);
  w[3] = fma(cj, bf16hi_to_f64(h.y), w[3]);
  w[4] = fma(cj, bf16lo_to_f64(h.z), w[4]);
  w[5] = fma(cj, bf16hi_to_f64(h.z), w[5]);
  w[6] = fma(cj, bf16lo_to_f64(h.w), w[6]);
  w[7] = fma(cj, bf16hi_to_f64(h.w), w[7]);
}
template <int RPS, bool GUARD>
__device__ __forceinline__ double axpy_lp_tile(const double* __restrict__ Q, int64_t ldq,
                                               const uint16_t* __restrict__ Qs, int64_t lds, int i,
                                               int64_t n, int64_t base, int lane,
                                               const double* __restrict__ c, bool use_lp,
                                               double* __restrict__ r) {
  double w[RPS][8];
#pragma unroll
  for (int s = 0; s < RPS; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) w[s][e] = 0.0;
  if (use_lp) {
    // Round 6, one bounded attempt at the 0.78 -> 0.83 the round-5 verdict asked for (profiles/r06_axpy_norm_lp_attempts.txt, same
    // box, alternated): unroll 4 / 8 / 16 = 37.2 / 38.3 / 40.1 us -- the pass is not short of loads in flight; requesting the
    // wave's rows of r (and its first four shadow rows) before the premise is waited for, as k_rdots does with its prologue:
    // 37 -> 104 us in both variants (the compiler no longer pipelines the eight loads of a trip).  Left as it was.
#ifndef DSEA_LP_UNROLL
#define DSEA_LP_UNROLL 4
#endif
#pragma unroll DSEA_LP_UNROLL
    for (int jj = 0; jj < i; ++jj) {
      const int j = i - 1 - jj;
      const uint16_t* __restrict__ qj = Qs + (int64_t)j * lds;
      const double cj = c[j];
#pragma unroll
      for (int s = 0; s < RPS; ++s) {
        const int64_t row = base + s * 512 + lane * 8;
        uint4 h;
        if (!GUARD || row + 8 <= n) {
          h = ld_u4_stream(qj + row);
        } else {
          uint32_t t[4] = {0u, 0u, 0u, 0u};
          for (int e = 0; e < 8; ++e)
            if (row + e < n) t[e >> 1] |= (uint32_t)qj[row + e] << ((e & 1) * 16);
          h = make_uint4(t[0], t[1], t[2], t[3]);
        }
        fma_shadow8(w[s], cj, h);
      }
    }
  } else {
    for (int jj = 0; jj < i; ++jj) {
      const int j = i - 1 - jj;
      const double* __restrict__ qj = Q + (int64_t)j * ldq;
      const double cj = c[j];
#pragma unroll
      for (int s = 0; s < RPS; ++s) {
        const int64_t row = base + s * 512 + lane * 8;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          double2 q = ld2_stream<GUARD>(qj, row + 2 * t, n);
          w[s][2 * t] = fma(cj, q.x, w[s][2 * t]);
          w[s][2 * t + 1] = fma(cj, q.y, w[s][2 * t + 1]);
        }
      }
    }
  }
  double acc = 0.0;
#pragma unroll
  for (int s = 0; s < RPS; ++s) {
    const int64_t row = base + s * 512 + lane * 8;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      double2 rv = ld2<GUARD>(r, row + 2 * t, n);
      rv.x -= w[s][2 * t];
      rv.y -= w[s][2 * t + 1];
      st2<GUARD>(r, row + 2 * t, n, rv);
      acc = fma(rv.x, rv.x, acc);
      acc = fma(rv.y, rv.y, acc);
    }
  }
  return acc;
}

template <int RPS>
__global__ __launch_bounds__(256) void k_axpy_norm_lp(const double* __restrict__ Q, int64_t ldq,
                                                      const uint16_t* __restrict__ Qs, int64_t lds, int i,
                                                      int64_t n, const double* __restrict__ c, double tau2,
                                                      double* __restrict__ r, double* __restrict__ P, int nw,
                                                      int64_t ntiles, double* __restrict__ lp_count,
                                                      const double* __restrict__ brk) {
  const int lane = threadIdx.x & 63;
  const int64_t widx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (widx >= nw) return;
  if (broken(brk)) return;
  // premise check, identical in every wave: max_j c_j^2 <= tau^2 ||r||^2   (c[i] = ||r||^2 from the dots pass)
  double m = 0.0;
  for (int b = lane; b < i; b += 64) {
    const double v = c[b];
    m = fmax(m, v * v);
  }
  m = wave_max(m);
  const bool use_lp = m <= tau2 * c[i];
  if (widx == 0 && lane == 0 && lp_count) lp_count[use_lp ? 0 : 1] += 1.0;
  constexpr int64_t TILE = 512 * RPS;
  double acc = 0.0;
  for (int64_t tile = widx; tile < ntiles; tile += nw) {
    const int64_t base = tile * TILE;
    if (base + TILE <= n)
      acc += axpy_lp_tile<RPS, false>(Q, ldq, Qs, lds, i, n, base, lane, c, use_lp, r);
    else
      acc += axpy_lp_tile<RPS, true>(Q, ldq, Qs, lds, i, n, base, lane, c, use_lp, r);
  }
  acc = wave_sum(acc);
  if (lane == 0) P[widx] = acc;
}

// Small-n ("split") form of the shadow pass: a block of W waves shares ONE tile of 512 rows (a lane owns 8 rows =
// one 16-byte shadow load) and splits the basis vectors between its waves in chunks of four; the W partial sums are
// combined through LDS in wave order (deterministic), wave 0 applies them.  Same premise check and fp64 fallback
// as k_axpy_norm_lp.  BASELINE config 3 (N = 1e5, k = 300): the correction pass streams 60 MB instead of 240 MB.
template <int W>
__global__ __launch_bounds__(W * 64) void k_axpy_norm_lp_split(const double* __restrict__ Q, int64_t ldq,
                                                               const uint16_t* __restrict__ Qs, int64_t lds, int i,
                                                               int64_t n, const double* __restrict__ c, double tau2,
                                                               double* __restrict__ r, double* __restrict__ P,
                                                               double* __restrict__ lp_count,
                                                               const double* __restrict__ brk) {
  __shared__ double part[W][8][64];
  if (broken(brk)) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t tile = blockIdx.x;
  const int64_t row = tile * 512 + lane * 8;
  double m = 0.0;
  for (int b = lane; b < i; b += 64) {
    const double v = c[b];
    m = fmax(m, v * v);
  }
  m = wave_max(m);
  const bool use_lp = m <= tau2 * c[i];
  if (tile == 0 && threadIdx.x == 0 && lp_count) lp_count[use_lp ? 0 : 1] += 1.0;
  const bool full = row + 8 <= n;
  double w[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) w[e] = 0.0;
  // LPV basis vectors per trip: with W = 16 waves and 8 loads of 16 bytes in flight per lane a wave needs one or two
  // trips for i <= 300 (the pass is a chain of dependent round trips, not a bandwidth problem, at these sizes:
  // 4 vectors per trip on 8 waves measured 17.2 us at N = 1e5, i ~ 150, for 30 MB of shadow)
  constexpr int LPV = 8;
  const int nchunks = (i + LPV - 1) / LPV;
  for (int cc = wv; cc < nchunks; cc += W) {
    const int j0 = LPV * cc;
    if (use_lp) {
      uint4 h[LPV];
      double cj[LPV];
#pragma unroll
      for (int v = 0; v < LPV; ++v) {
        h[v] = make_uint4(0u, 0u, 0u, 0u);
        cj[v] = 0.0;
        if (j0 + v < i) {
          cj[v] = c[j0 + v];
          const uint16_t* __restrict__ qj = Qs + (int64_t)(j0 + v) * lds;
          if (full) {
            h[v] = ld_u4_stream(qj + row);
          } else {
            uint32_t t4[4] = {0u, 0u, 0u, 0u};
            for (int e = 0; e < 8; ++e)
              if (row + e < n) t4[e >> 1] |= (uint32_t)qj[row + e] << ((e & 1) * 16);
            h[v] = make_uint4(t4[0], t4[1], t4[2], t4[3]);
          }
        }
      }
#pragma unroll
      for (int v = 0; v < LPV; ++v) fma_shadow8(w, cj[v], h[v]);
    } else {
      for (int v = 0; v < LPV; ++v) {
        if (j0 + v >= i) break;
        const double* __restrict__ qj = Q + (int64_t)(j0 + v) * ldq;
        const double cj = c[j0 + v];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const double2 q = ld2_stream<true>(qj, row + 2 * t, n);
          w[2 * t] = fma(cj, q.x, w[2 * t]);
          w[2 * t + 1] = fma(cj, q.y, w[2 * t + 1]);
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) part[wv][e][lane] = w[e];
  __syncthreads();
  if (wv == 0) {
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      double tx = part[0][2 * t][lane], ty = part[0][2 * t + 1][lane];
#pragma unroll
      for (int k2 = 1; k2 < W; ++k2) {
        tx += part[k2][2 * t][lane];
        ty += part[k2][2 * t + 1][lane];
      }
      double2 rv = ld2<true>(r, row + 2 * t, n);
      rv.x -= tx;
      rv.y -= ty;
      st2<true>(r, row + 2 * t, n, rv);
      acc = fma(rv.x, rv.x, acc);
      acc = fma(rv.y, rv.y, acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) P[tile] = acc;
  }
}

// returns the number of partials written
int launch_axpy_norm_lp(int64_t n, int rps, const double* Q, int64_t ldq, const uint16_t* Qs, int64_t lds, int i,
                        const double* c, double tau, double* r, double* P, double* lp_count, hipStream_t st,
                        EventPair* ev, const double* brk) {
  if (rps == 0) {   // small-n split form: one block of 16 waves per 512-row tile
    const int64_t nt = (n + 511) / 512;
    klaunch(ev, k_axpy_norm_lp_split<16>, (unsigned)nt, 1024, 0, st, Q, ldq, Qs, lds, i, n, c, tau * tau, r, P, lp_count, brk);
    return (int)nt;
  }
  const int64_t tile = 512 * (int64_t)rps;
  int64_t ntiles = (n + tile - 1) / tile;
  if (ntiles < 1) ntiles = 1;
  const int nw = (int)(ntiles < DSEA_MAX_WAVE_TILES ? ntiles : DSEA_MAX_WAVE_TILES);
  dispatch_int<1, 2>(rps, [&](auto rows) {
    klaunch(ev, k_axpy_norm_lp<decltype(rows)::value>, (nw + 3) / 4, 256, 0, st, Q, ldq, Qs, lds, i, n, c, tau * tau, r, P,
            nw, ntiles, lp_count, brk);
  });
  return nw;
}

// ------------------------------------------------------------------------------------------
// The same pass reading an 8-BIT shadow of the basis: one e5m2 code of q * S per element (S a power of two fixed per run,
// f64_to_e5m2 in dsea_device.h), wave-owned geometry only (n >= 2^20 rows).  docs/design/15-shadow8.md has the argument:
// the error  sum_j c_j (dec(code_j) / S - q_j)  is a combination of storage-rounding noise vectors, uncorrelated with every
// basis vector, of norm ~0.07 sqrt(sum c_j^2) -- below the rounding already committed when u - alpha q - beta q' was formed.
// The premise is the bf16 pass's, against a bound 2^-6 times tighter (the ratio of the two codes' relative errors).
//
// Arithmetic: the correction only has to be known to three digits, so it is accumulated in fp32,
//   w_k = sum_j chat_j dec(code_jk),  chat_j = float(c_j / (S sqrt(c[i]))),      then ONE fp64 step  r_k -= double(w_k) sqrt(c[i]);
// under the premise |chat_j S| <= tau8, so nothing overflows, and products that flush are below 1e-38 ||r||.  Two packed
// converts and two packed FMAs per four elements keep the pass on memory at twice the bf16 pass's element rate.
// ||r||^2 partials come from the updated r in fp64.
//
// Geometry: a lane owns RPS groups of 16 consecutive rows (one 16-byte load each); a wave tile is 1024*RPS rows; j runs
// downwards.  The fp64 fallback walks the same tile as eight 128-row slices (a lane owns one double2 of each).
typedef float dsea_v2f __attribute__((ext_vector_type(2)));
// w[0..3] += ch * (the four e5m2 codes of word x)
__device__ __forceinline__ void fma_e5m2x4(dsea_v2f& w01, dsea_v2f& w23, dsea_v2f ch, uint32_t x) {
  w01 = __builtin_elementwise_fma(ch, __builtin_amdgcn_cvt_pk_f32_bf8((int)x, false), w01);
  w23 = __builtin_elementwise_fma(ch, __builtin_amdgcn_cvt_pk_f32_bf8((int)x, true), w23);
}
template <int RPS, bool GUARD>
__device__ __forceinline__ double axpy_lp8_tile(const uint8_t* __restrict__ Qs8, int64_t ld8, int i, int64_t n, int64_t base,
                                                int lane, const double* __restrict__ c, double cs, double rnorm,
                                                double* __restrict__ r) {
  dsea_v2f w[RPS][8];
#pragma unroll
  for (int s = 0; s < RPS; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) w[s][e] = (dsea_v2f)(0.0f);
  // (no prologue prefetch of r or of the first rows: see the note in axpy_lp_tile; unroll 8 = eight 16-byte loads in flight
  //  per lane at RPS = 1, what the bf16 pass has at its measured optimum)
#ifndef DSEA_LP8_UNROLL
#define DSEA_LP8_UNROLL 8
#endif
#pragma unroll DSEA_LP8_UNROLL
  for (int jj = 0; jj < i; ++jj) {
    const int j = i - 1 - jj;
    const uint8_t* __restrict__ qj = Qs8 + (int64_t)j * ld8;
    const float chf = (float)(c[j] * cs);
    const dsea_v2f ch = (dsea_v2f)(chf);
#pragma unroll
    for (int s = 0; s < RPS; ++s) {
      const int64_t row = base + s * 1024 + lane * 16;
      uint4 h;
      if (!GUARD || row + 16 <= n) {
        h = ld_u4_stream(qj + row);
      } else {
        uint32_t t[4] = {0u, 0u, 0u, 0u};   // rows >= n: code 0 = +0.0
        for (int e = 0; e < 16; ++e)
          if (row + e < n) t[e >> 2] |= (uint32_t)qj[row + e] << ((e & 3) * 8);
        h = make_uint4(t[0], t[1], t[2], t[3]);
      }
      fma_e5m2x4(w[s][0], w[s][1], ch, h.x);
      fma_e5m2x4(w[s][2], w[s][3], ch, h.y);
      fma_e5m2x4(w[s][4], w[s][5], ch, h.z);
      fma_e5m2x4(w[s][6], w[s][7], ch, h.w);
    }
  }
  double acc = 0.0;
#pragma unroll
  for (int s = 0; s < RPS; ++s) {
    const int64_t row = base + s * 1024 + lane * 16;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      double2 rv = ld2<GUARD>(r, row + 2 * t, n);
      rv.x = fma(-(double)w[s][t].x, rnorm, rv.x);
      rv.y = fma(-(double)w[s][t].y, rnorm, rv.y);
      st2<GUARD>(r, row + 2 * t, n, rv);
      acc = fma(rv.x, rv.x, acc);
      acc = fma(rv.y, rv.y, acc);
    }
  }
  return acc;
}
// the fp64 fallback of the 8-bit pass over one 1024*RPS-row tile
template <int RPS, bool GUARD>
__device__ __forceinline__ double axpy_lp8_tile_fp64(const double* __restrict__ Q, int64_t ldq, int i, int64_t n, int64_t base,
                                                     int lane, const double* __restrict__ c, double* __restrict__ r) {
  double2 w[RPS * 8];
#pragma unroll
  for (int t = 0; t < RPS * 8; ++t) w[t] = make_double2(0.0, 0.0);
  for (int jj = 0; jj < i; ++jj) {
    const int j = i - 1 - jj;
    const double* __restrict__ qj = Q + (int64_t)j * ldq;
    const double cj = c[j];
#pragma unroll
    for (int t = 0; t < RPS * 8; ++t) {
      const double2 q = ld2_stream<GUARD>(qj, base + t * 128 + lane * 2, n);
      w[t].x = fma(cj, q.x, w[t].x);
      w[t].y = fma(cj, q.y, w[t].y);
    }
  }
  double acc = 0.0;
#pragma unroll
  for (int t = 0; t < RPS * 8; ++t) {
    const int64_t row = base + t * 128 + lane * 2;
    double2 rv = ld2<GUARD>(r, row, n);
    rv.x -= w[t].x;
    rv.y -= w[t].y;
    st2<GUARD>(r, row, n, rv);
    acc = fma(rv.x, rv.x, acc);
    acc = fma(rv.y, rv.y, acc);
  }
  return acc;
}

template <int RPS>
__global__ __launch_bounds__(256) void k_axpy_norm_lp8(const double* __restrict__ Q, int64_t ldq,
                                                       const uint8_t* __restrict__ Qs8, int64_t ld8, double scale, int i,
                                                       int64_t n, const double* __restrict__ c, double tau2,
                                                       double* __restrict__ r, double* __restrict__ P, int nw,
                                                       int64_t ntiles, double* __restrict__ lp_count,
                                                       const double* __restrict__ brk) {
  const int lane = threadIdx.x & 63;
  const int64_t widx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (widx >= nw) return;
  if (broken(brk)) return;
  // premise check, identical in every wave: max_j c_j^2 <= tau8^2 ||r||^2   (c[i] = ||r||^2 from the dots pass)
  double m = 0.0;
  for (int b = lane; b < i; b += 64) {
    const double v = c[b];
    m = fmax(m, v * v);
  }
  m = wave_max(m);
  const double rr = c[i];
  const bool use_lp = m <= tau2 * rr;
  if (widx == 0 && lane == 0 && lp_count) lp_count[use_lp ? 0 : 1] += 1.0;
  const double rnorm = sqrt(rr);
  const double cs = rnorm > 0.0 ? 1.0 / (scale * rnorm) : 0.0;   // (r = 0: the premise holds only with c = 0)
  constexpr int64_t TILE = 1024 * RPS;
  double acc = 0.0;
  for (int64_t tile = widx; tile < ntiles; tile += nw) {
    const int64_t base = tile * TILE;
    const bool whole = base + TILE <= n;
    if (use_lp)
      acc += whole ? axpy_lp8_tile<RPS, false>(Qs8, ld8, i, n, base, lane, c, cs, rnorm, r)
                   : axpy_lp8_tile<RPS, true>(Qs8, ld8, i, n, base, lane, c, cs, rnorm, r);
    else
      acc += whole ? axpy_lp8_tile_fp64<RPS, false>(Q, ldq, i, n, base, lane, c, r)
                   : axpy_lp8_tile_fp64<RPS, true>(Q, ldq, i, n, base, lane, c, r);
  }
  acc = wave_sum(acc);
  if (lane == 0) P[widx] = acc;
}

// returns the number of partials written
int launch_axpy_norm_lp8(int64_t n, const double* Q, int64_t ldq, const uint8_t* Qs8, int64_t ld8, double scale, int i,
                         const double* c, double tau, double* r, double* P, double* lp_count, hipStream_t st,
                         EventPair* ev, const double* brk) {
#ifndef DSEA_LP8_RPS
#define DSEA_LP8_RPS 1   /* 2^20 rows: 1024 tiles, one wave per SIMD */
#endif
  constexpr int RPS = DSEA_LP8_RPS;
  const int64_t tile = 1024 * (int64_t)RPS;
  int64_t ntiles = (n + tile - 1) / tile;
  if (ntiles < 1) ntiles = 1;
  const int nw = (int)(ntiles < DSEA_MAX_WAVE_TILES ? ntiles : DSEA_MAX_WAVE_TILES);
  klaunch(ev, k_axpy_norm_lp8<RPS>, (nw + 3) / 4, 256, 0, st, Q, ldq, Qs8, ld8, scale, i, n, c, tau * tau, r, P, nw, ntiles,
          lp_count, brk);
  return nw;
}

// ------------------------------------------------------------------------------------------
// Partial re-orthogonalisation (Simon 1984; an OPTION -- the reference re-orthogonalises on every step, Lanczos.py:66).
// omega_{i,k} estimates q_i . q_k from the scalars of the recurrence alone:
//   beta_{i-1} omega_{i,k} = beta_k omega_{i-1,k+1} + (alpha_k - alpha_{i-1}) omega_{i-1,k} + beta_{k-1} omega_{i-1,k-1}
//                            - beta_{i-2} omega_{i-2,k}  (+ a rounding term of the size of eps ||A||),   omega_{j,j} = 1
// One block per step; when max_k |omega_{i,k}| exceeds delta (default 1e-10) this step AND the next one are re-orthogonalised
// against the whole basis and their estimates restart at the rounding level.  om: two rows of `ld` doubles (row i & 1
// is overwritten in place: new[k] needs the old row only at the same k).
// state: [0] re-orthogonalise the next step too  [1] running estimate of ||A||  [2] number of re-orthogonalised steps
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pro_update(const double* __restrict__ alphas, const double* __restrict__ betas,
                                                    const double* __restrict__ rrP, int rrCount,
                                                    double* __restrict__ rr_store, double* __restrict__ om, int ld,
                                                    double* __restrict__ flag, double* __restrict__ state, int i,
                                                    double eps1, double delta, const double* __restrict__ brk) {
  __shared__ double smax[256];
  __shared__ double sm5[5];
  // ||r_i||^2 before any correction: the dots kernel's per-block partials, summed here (no second-stage launch); the
  // total is stored for the correction kernel, which hands it on as ||r||^2 on a step that is not re-orthogonalised.
  // (Everything that does not depend on another load is requested before the break record is looked at: the kernel is a
  // chain of dependent round trips, nothing else.)
  const double a = alphas[i - 1];
  const double bprev = (i >= 2) ? betas[i - 2] : 0.0;
  const double anorm_prev = state[1];
  const double rr = sum_partials_block(rrP, rrCount, sm5);
  if (broken(brk)) return;
  if (threadIdx.x == 0) rr_store[0] = rr;
  const double bcur = sqrt(rr);                            // = beta_{i-1} to rounding
  const double anorm = fmax(anorm_prev, fabs(a) + bcur + bprev);
  double* __restrict__ o1 = om + (size_t)((i - 1) & 1) * ld;   // omega_{i-1, .}
  double* __restrict__ o2 = om + (size_t)(i & 1) * ld;         // omega_{i-2, .}  -> omega_{i, .}
  double mx = 0.0;
  for (int k = threadIdx.x; k <= i - 1; k += 256) {
    double v;
    if (k == i - 1) {
      v = eps1 * anorm / bcur;
    } else {
      const double w1k = o1[k];
      const double w1p = (k + 1 == i - 1) ? 1.0 : o1[k + 1];
      const double w1m = (k > 0) ? o1[k - 1] : 0.0;
      const double w2k = (k == i - 2) ? 1.0 : o2[k];
      double t = betas[k] * w1p + (alphas[k] - a) * w1k - bprev * w2k;
      if (k > 0) t += betas[k - 1] * w1m;
      const double d = eps1 * ((betas[k] + bcur) + anorm);
      v = (t + copysign(d, t)) / bcur;
    }
    mx = fmax(mx, fabs(v));
    // (o2[k] is only read by this thread at this k; the neighbours come from the other row)
    o2[k] = v;
  }
  smax[threadIdx.x] = mx;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + s]);
    __syncthreads();
  }
  mx = smax[0];
  const bool forced = state[0] != 0.0;
  const bool trig = !(mx <= delta);                       // also true for NaN
  __syncthreads();                                        // everybody has read state[0]
  if (trig || forced) {
    for (int k = threadIdx.x; k <= i - 1; k += 256) o2[k] = eps1;
  }
  if (threadIdx.x == 0) {
    flag[0] = (trig || forced) ? 1.0 : 0.0;
    state[0] = trig ? 1.0 : 0.0;
    state[1] = anorm;
    if (trig || forced) state[2] += 1.0;
  }
}

void launch_pro_update(const double* alphas, const double* betas, const double* rrP, int rrCount, double* rr_store,
                       double* om, int ld, double* flag, double* state, int i, double eps1, double delta,
                       const double* brk, hipStream_t st) {
  hipLaunchKernelGGL(k_pro_update, dim3(1), dim3(256), 0, st, alphas, betas, rrP, rrCount, rr_store, om, ld, flag, state,
                     i, eps1, delta, brk);
}

// ------------------------------------------------------------------------------------------
// Measurement probes (bench.py "measured_ceilings"): what THIS box streams with nothing else to do.
// A block walks tiles of 4096 doubles: 8 non-temporal 16-byte loads in flight per lane, no dependence between trips.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_probe_read(const double* __restrict__ x, int64_t n, double* __restrict__ P) {
  __shared__ double sm4[4];
  double acc = 0.0;
  for (int64_t base = (int64_t)blockIdx.x * 4096; base < n; base += (int64_t)gridDim.x * 4096) {
    double2 v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = ld2_stream<true>(x, base + t * 512 + threadIdx.x * 2, n);
#pragma unroll
    for (int t = 0; t < 8; ++t) acc += v[t].x + v[t].y;
  }
  const double tot = block_sum(acc, sm4);
  if (threadIdx.x == 0) P[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void k_probe_copy(const double* __restrict__ x, double* __restrict__ y, int64_t n) {
  for (int64_t base = (int64_t)blockIdx.x * 4096; base < n; base += (int64_t)gridDim.x * 4096) {
    double2 v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = ld2_stream<true>(x, base + t * 512 + threadIdx.x * 2, n);
#pragma unroll
    for (int t = 0; t < 8; ++t) st2<true>(y, base + t * 512 + threadIdx.x * 2, n, v[t]);
  }
}

void launch_probe(const double* x, double* y, int64_t n, double* P, int nP, hipStream_t st) {
  int64_t tiles = (n + 4095) / 4096;
  const int grid = (int)(tiles < nP ? tiles : nP);
  if (y)
    hipLaunchKernelGGL(k_probe_copy, dim3(grid), dim3(256), 0, st, x, y, n);
  else
    hipLaunchKernelGGL(k_probe_read, dim3(grid), dim3(256), 0, st, x, n, P);
}

}  // namespace dsea
