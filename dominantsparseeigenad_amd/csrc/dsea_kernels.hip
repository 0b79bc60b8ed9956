// dsea_kernels.hip -- gfx950 (MI355X, CDNA4) kernels of the dominant-eigenpair hot path.
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
#include <hip/hip_ext.h>
#include <stdint.h>

#include <type_traits>

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

// q = r / sqrt(nrm2) ; beta_out = sqrt(nrm2)
__global__ __launch_bounds__(256) void k_scale_store(const double* __restrict__ r,
                                                     const double* __restrict__ nrm2,
                                                     double* __restrict__ q, double* __restrict__ beta_out,
                                                     int64_t n, uint16_t* __restrict__ qs,
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
    if (qs) st_bf16x2(qs, row, n, v);
  }
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

__global__ void k_cg_init_check(double* __restrict__ state, double eps) {
  const double rn = sqrt(state[DSEA_CG_RR]);
  state[DSEA_CG_RESNORM] = rn;
  state[DSEA_CG_DONE] = (rn < eps) ? 1.0 : 0.0;
  state[DSEA_CG_ITERS] = 0.0;
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
  uint16_t* qs_out;      // bf16 shadow row or null
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
    if (fa.qs_out) st_bf16x2(fa.qs_out, row, n, v);
  }
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
          if (fa.qs_out)
            *reinterpret_cast<uint32_t*>(fa.qs_out + base + 2 * lp) =
                (uint32_t)f64_to_bf16(v.x) | ((uint32_t)f64_to_bf16(v.y) << 16);
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
        if (fa.qs_out) fa.qs_out[row] = f64_to_bf16(xi);
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
        if (fa.qs_out) fa.qs_out[row] = f64_to_bf16(xi);
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
      if (fa.qs_out) st_bf16x2(fa.qs_out, i, p.n, xv);
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

// ------------------------------------------------------------------------------------------
// Persistent single-launch CG for the 3-point stencil on SMALL vectors (BASELINE config 3: N = 1e5, 0.8 MB per
// vector).  There the three launches per iteration of the streaming form cost ~13 us for ~1 us of memory
// traffic.  Here the whole solve is ONE launch of G workgroups x 1024 threads that keep x, r, d and V in
// REGISTERS for the entire solve (row pairs, the canonical tile geometry of the streaming kernels); per
// iteration only
//   * the per-tile partials of d.Ad and r.r                      (one 8-byte value per 512 rows)
//   * the two edge elements of r of every workgroup              (halo of the next mat-vec: d' = r + beta d)
// cross workgroups, as data-tagged granules (cdna_hip_programming.md Guideline 16, form R2: the data is the
// flag -- {epoch tag, 32 payload bits} written by ONE relaxed agent-scope 8-byte store, polled with relaxed
// agent-scope loads; no fences, no separate flags, state zeroed by the launcher before every launch).
// Every workgroup reads ALL tile partials and sums them in exactly the order the streaming kernels use
// (sum_partials_block / k_finalize1), all elementwise updates use the same rounded operations, and a tile
// partial is the same function of the tile's rows: the iterates are BIT-IDENTICAL to the 3-launch form
// (tests/test_gpu_persistent.py) and identical on every workgroup, so all take the same exit.
// Reference: CG.py:24-41 with A' = A - shift (CG.py:120).
// ------------------------------------------------------------------------------------------
struct PersistArgs {
  Stencil3Params p;
  const double* shift;
  const double* b;
  double* x;        // in: start vector, out: solution
  double* state;    // DSEA_CG_* (written by workgroup 0 at the end)
  double eps;
  long long maxiter;
  unsigned long long* comm;  // granules: [2*ntiles] phase A | [2*ntiles] phase C | [4*G] r edges | [4*G] x edges ; zeroed per launch
  int ntiles;
  int lose_peer;   // test hook (dsea_ws_set_fault_injection): the last workgroup exits at once
};

// shared scratch behind the d-with-halo array: wave partials of up to 4 sub-rounds, the broadcast slots
struct PersistSm {
  double red[4][16];
  double bcast[8];   // [0] total  [1] left edge  [2] right edge  [3] fail flag
};

// All 1024 threads call this.  Threads 0..255 fetch the `count` tile partials of phase `base` (spinning until every
// granule carries `epoch`) and sum them in the order of sum_partials_block (two_acc) or k_finalize1 (!two_acc);
// thread 256 / 320 fetch the neighbour workgroups' edge values when `edges`.  Returns the total in every thread;
// el / er receive the edges.  `fail` is set (in every thread) if a peer did not show up in time.
template <int NVB>
__device__ __forceinline__ double persist_gather(gran_u64* base, int count, unsigned epoch, bool two_acc,
                                                 gran_u64* edge_base, bool edges, int g, int G, PersistSm* sm, double& el,
                                                 double& er, bool& fail) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long t0 = wall_clock64();
  // edge pollers: two lanes of waves that do not poll tile partials (NVB >= 2), else two lanes of the polling waves
  constexpr int EL = NVB >= 2 ? 256 : 0, ER = NVB >= 2 ? 320 : 64;
  if (NVB == 1 && edges && (tid == EL || tid == ER)) {
    const bool left = tid == EL;
    const int peer = left ? g - 1 : g + 1;
    double v = 0.0;
    if (peer >= 0 && peer < G) {
      gran_u64* src = edge_base + (peer * 2 + (left ? 1 : 0)) * 2;   // left neighbour's LAST row / right one's FIRST
      if (!granule_wait(src, epoch, v, t0, DSEA_GRANULE_TIMEOUT_TICKS)) sm->bcast[3] = 1.0;
    }
    sm->bcast[left ? 1 : 2] = v;
  }
  if (tid < 256) {
    gran_u64* src[4];
    bool on[4];
    double pv[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int idx = tid + 256 * m;
      src[m] = base + 2 * idx;
      on[m] = idx < count;
    }
    if (!granule_wait_all(src, on, epoch, pv, t0, DSEA_GRANULE_TIMEOUT_TICKS)) sm->bcast[3] = 1.0;
    double acc;
    if (two_acc) {
      const double a0 = (0.0 + pv[0]) + pv[2], a1 = (0.0 + pv[1]) + pv[3];
      acc = a0 + a1;
    } else {
      acc = (((0.0 + pv[0]) + pv[1]) + pv[2]) + pv[3];
    }
    acc = wave_sum(acc);
    if (lane == 0) sm->red[0][wave] = acc;
  } else if (NVB >= 2 && edges && (tid == EL || tid == ER)) {
    const bool left = tid == EL;
    const int peer = left ? g - 1 : g + 1;
    double v = 0.0;
    if (peer >= 0 && peer < G) {
      gran_u64* src = edge_base + (peer * 2 + (left ? 1 : 0)) * 2;   // left neighbour's LAST row / right one's FIRST
      if (!granule_wait(src, epoch, v, t0, DSEA_GRANULE_TIMEOUT_TICKS)) sm->bcast[3] = 1.0;
    }
    sm->bcast[left ? 1 : 2] = v;
  }
  __syncthreads();
  const double tot = ((sm->red[0][0] + sm->red[0][1]) + sm->red[0][2]) + sm->red[0][3];
  el = sm->bcast[1];
  er = sm->bcast[2];
  fail = sm->bcast[3] != 0.0;
  __syncthreads();   // red / bcast may be rewritten by the next phase
  return tot;
}

// NVB = "virtual blocks" of 256 threads per workgroup (a virtual block reproduces one block of the streaming kernels)
template <int PPT, int NVB>
__global__ __launch_bounds__(256 * NVB) void k_cg_persist_stencil(PersistArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int TPW = NVB * PPT;        // tiles per workgroup
  constexpr int ROWS = TPW * 512;
  double* dsm = lds;                    // dsm[1] left halo, dsm[2 + local row] (pairs 16-byte aligned), dsm[2 + ROWS] right halo
  PersistSm* sm = reinterpret_cast<PersistSm*>(lds + ROWS + 4);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, vb = tid >> 8, t = tid & 255;
  const int g = blockIdx.x, G = gridDim.x;
  if (a.lose_peer && G > 1 && g == G - 1) return;
  const int64_t n = a.p.n;
  gran_u64* commA = (gran_u64*)a.comm;
  gran_u64* commC = commA + 2 * (int64_t)a.ntiles;
  gran_u64* commE = commC + 2 * (int64_t)a.ntiles;
  // The start-up exchange of the x edges has its OWN slots: that phase waits for the two neighbours only, so a fast
  // workgroup may be a whole phase ahead of a neighbour that has not read its x edge yet -- were the r edges of the
  // next phase written to the same granules, that neighbour would wait for an epoch that is gone (seen as a timeout
  // when the pollers' back-off sleep was lengthened in an experiment).  All later phases are separated by an
  // all-to-all dependency (every workgroup needs every tile partial), which is what makes slot reuse safe there.
  gran_u64* commX = commE + 4 * (int64_t)gridDim.x;
  const double coef = a.p.coef;
  const bool has_shift = a.shift != nullptr;
  const double s = has_shift ? a.shift[0] : 0.0;
  if (tid == 0) sm->bcast[3] = 0.0;
  __syncthreads();

  // my row pairs: sub-round q -> tile g*TPW + NVB q + vb, rows (tile*512 + 2t, +1)
  int lrow[PPT];
  int tile[PPT];
  bool v0[PPT], v1[PPT];   // row exists
  double2 xv[PPT], rv[PPT], dv[PPT], Vv[PPT];
#pragma unroll
  for (int q = 0; q < PPT; ++q) {
    tile[q] = g * TPW + NVB * q + vb;
    lrow[q] = (NVB * q + vb) * 512 + 2 * t;
    const int64_t i = (int64_t)tile[q] * 512 + 2 * t;
    v0[q] = i < n;
    v1[q] = i + 1 < n;
    xv[q] = ld2<true>(a.x, i, n);
    Vv[q] = ld2<true>(a.p.V, i, n);
  }
  // y = A' w for the vector currently in dsm (halos included); returns the pair of my sub-round q
  auto apply = [&](int q, double2 w) -> double2 {
    const double dn = dsm[lrow[q] + 1];       // element before the pair
    const double up = dsm[lrow[q] + 4];       // element after the pair
    double2 y;
    y.x = v0[q] ? stencil_row(coef, Vv[q].x, w.x, v1[q] ? w.y : 0.0, dn) : 0.0;
    y.y = v1[q] ? stencil_row(coef, Vv[q].y, w.y, up, w.x) : 0.0;
    if (has_shift) {
      y.x = __dsub_rn(y.x, __dmul_rn(s, w.x));
      y.y = __dsub_rn(y.y, __dmul_rn(s, w.y));
    }
    return y;
  };
  auto stage = [&](const double2* w, double hl, double hr) {   // w with halos -> dsm
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PPT; ++q) *reinterpret_cast<double2*>(dsm + 2 + lrow[q]) = w[q];
    if (tid == 0) {
      dsm[1] = hl;
      dsm[2 + ROWS] = hr;
    }
    __syncthreads();
  };
  // per-tile partial sum_t (a.x b.x + a.y b.y) of sub-round q published under `epoch` in `dst`
  auto publish_tiles = [&](gran_u64* dst, unsigned epoch, const double2* u, const double2* w) {
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
      double acc = 0.0;
      acc = fma(u[q].x, w[q].x, acc);
      acc = fma(u[q].y, w[q].y, acc);
      acc = wave_sum(acc);
      if (lane == 0) sm->red[q][wave] = acc;
    }
    __syncthreads();
    if (t == 0) {
#pragma unroll
      for (int q = 0; q < PPT; ++q)
        if (tile[q] < a.ntiles) {
          const double tot = ((sm->red[q][4 * vb] + sm->red[q][4 * vb + 1]) + sm->red[q][4 * vb + 2]) + sm->red[q][4 * vb + 3];
          granule_put(dst + 2 * tile[q], epoch, tot);
        }
    }
    __syncthreads();
  };
  auto publish_edges = [&](unsigned epoch, const double2* w) {
    if (tid == 0) granule_put(commE + (g * 2 + 0) * 2, epoch, w[0].x);
    if (tid == 256 * NVB - 1) granule_put(commE + (g * 2 + 1) * 2, epoch, w[PPT - 1].y);
  };

  double el, er;
  bool fail;
  unsigned epoch = 1;
  // ---- r = b - A' x0 ; d = r ; rr = r.r                                          (CG.py:26-30)
  if (tid == 0) granule_put(commX + (g * 2 + 0) * 2, epoch, xv[0].x);
  if (tid == 256 * NVB - 1) granule_put(commX + (g * 2 + 1) * 2, epoch, xv[PPT - 1].y);
  {
    double dummy = persist_gather<NVB>(commA, 0, epoch, true, commX, true, g, G, sm, el, er, fail);
    (void)dummy;
  }
  if (fail) {
    if (g == 0 && tid == 0) a.state[DSEA_CG_DONE] = -1.0;
    return;
  }
  stage(xv, el, er);
#pragma unroll
  for (int q = 0; q < PPT; ++q) {
    const double2 Ax = apply(q, xv[q]);
    const double2 bv = ld2<true>(a.b, (int64_t)tile[q] * 512 + 2 * t, n);
    rv[q].x = __dsub_rn(bv.x, Ax.x);
    rv[q].y = __dsub_rn(bv.y, Ax.y);
    dv[q] = rv[q];
  }
  epoch = 2;
  publish_edges(epoch, rv);
  publish_tiles(commC, epoch, rv, rv);
  double rr = persist_gather<NVB>(commC, a.ntiles, epoch, false, commE, true, g, G, sm, el, er, fail);
  double dL = el, dR = er;   // d = r: the neighbours' edge d values
  double rn = sqrt(rr);
  long long iters = 0;
  bool done = rn < a.eps;
  // ---- iterations                                                                  (CG.py:31-40)
  while (!done && !fail && iters < a.maxiter) {
    stage(dv, dL, dR);
    double2 Ad[PPT];
#pragma unroll
    for (int q = 0; q < PPT; ++q) Ad[q] = apply(q, dv[q]);
    ++epoch;
    publish_tiles(commA, epoch, dv, Ad);
    const double dAd = persist_gather<NVB>(commA, a.ntiles, epoch, true, commE, false, g, G, sm, el, er, fail);
    if (fail) break;
    const double alpha = rr / dAd;
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
      xv[q].x = __dadd_rn(xv[q].x, __dmul_rn(alpha, dv[q].x));
      xv[q].y = __dadd_rn(xv[q].y, __dmul_rn(alpha, dv[q].y));
      rv[q].x = __dsub_rn(rv[q].x, __dmul_rn(alpha, Ad[q].x));
      rv[q].y = __dsub_rn(rv[q].y, __dmul_rn(alpha, Ad[q].y));
    }
    ++epoch;
    publish_edges(epoch, rv);
    publish_tiles(commC, epoch, rv, rv);
    const double rr_new = persist_gather<NVB>(commC, a.ntiles, epoch, true, commE, true, g, G, sm, el, er, fail);
    if (fail) break;
    ++iters;
    rn = sqrt(rr_new);
    if (rn < a.eps) {
      done = true;
      break;
    }
    const double beta = rr_new / rr;
    rr = rr_new;
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
      dv[q].x = __dadd_rn(rv[q].x, __dmul_rn(beta, dv[q].x));
      dv[q].y = __dadd_rn(rv[q].y, __dmul_rn(beta, dv[q].y));
    }
    dL = __dadd_rn(el, __dmul_rn(beta, dL));   // the neighbours' edge elements of d, updated as they update them
    dR = __dadd_rn(er, __dmul_rn(beta, dR));
  }
#pragma unroll
  for (int q = 0; q < PPT; ++q) st2<true>(a.x, (int64_t)tile[q] * 512 + 2 * t, n, xv[q]);
  if (g == 0 && tid == 0) {
    a.state[DSEA_CG_RR] = rr;
    a.state[DSEA_CG_RESNORM] = rn;
    a.state[DSEA_CG_ITERS] = (double)iters;
    a.state[DSEA_CG_DONE] = fail ? -1.0 : (done ? 1.0 : 0.0);
  }
}

// ------------------------------------------------------------------------------------------
// ONE grid-wide exchange per iteration: the same persistent solve with the two reductions of an iteration MERGED
// (Chronopoulos & Gear's arrangement of CG: s = A p is carried by a recurrence, w = A r is the mat-vec, and
// gamma = r.r, delta = r.Ar are reduced together).  The mat-vec's own neighbour exchange rides on the same
// exchange: w = A r is first formed with zero halos, the missing cross terms of delta are added from the
// published edge elements (2 coef r_last(g) r_first(g+1) per workgroup boundary), and the two edge rows of w are
// completed once the neighbours' edges have arrived.
//     p = r + beta p ; s = w + beta s ; x += alpha p ; r -= alpha s ; w = A' r ;
//     gamma' = r.r , delta = r.w   <- the ONE exchange ;  beta' = gamma'/gamma ; alpha' = gamma'/(delta - beta' gamma'/alpha)
// Mathematically the iteration of CG.py:31-40; NOT its rounding sequence (the search direction's image is
// updated by recurrence instead of being recomputed), so this form is an OPTION (dsea_ws_set_persist mode >= 100),
// never the default: iterates agree with the reference's to rounding-error growth, not bit for bit.
// Exchange: every workgroup publishes {gamma_g, delta_g, first r, last r} under the epoch into the slot set of the
// epoch's PARITY -- with one exchange per iteration a fast workgroup may publish epoch e+1 while a slow one still
// reads epoch e; it cannot reach e+2 before everyone has published e+1, i.e. has finished reading e.
// Every workgroup reads all 4 G values and sums them in the same fixed order: identical scalars everywhere.
// ------------------------------------------------------------------------------------------
struct PersistSmM {
  double red[2][16];
  double bcast[8];      // [0] gamma [1] delta [2] left edge [3] right edge [4] fail
  double vals[4 * 256];
};

template <int PPT, int NVB>
__global__ __launch_bounds__(256 * NVB) void k_cg_persist_stencil_merged(PersistArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int TPW = NVB * PPT;
  constexpr int ROWS = TPW * 512;
  constexpr int NWAVES = 4 * NVB;
  double* dsm = lds;
  PersistSmM* sm = reinterpret_cast<PersistSmM*>(lds + ROWS + 4);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, vb = tid >> 8, t = tid & 255;
  const int g = blockIdx.x, G = gridDim.x;
  if (a.lose_peer && G > 1 && g == G - 1) return;
  const int64_t n = a.p.n;
  gran_u64* commS = (gran_u64*)a.comm;                       // [2 parities][G][4 values][2 granules]
  gran_u64* commX = commS + 16 * (int64_t)G;             // x edges of the start-up: [G][2][2]
  const double coef = a.p.coef;
  const bool has_shift = a.shift != nullptr;
  const double sh = has_shift ? a.shift[0] : 0.0;
  if (tid == 0) sm->bcast[4] = 0.0;
  __syncthreads();

  int lrow[PPT];
  int tile[PPT];
  bool v0[PPT], v1[PPT];
  double2 xv[PPT], rv[PPT], pv[PPT], sv[PPT], wv[PPT], Vv[PPT];
#pragma unroll
  for (int q = 0; q < PPT; ++q) {
    tile[q] = g * TPW + NVB * q + vb;
    lrow[q] = (NVB * q + vb) * 512 + 2 * t;
    const int64_t i = (int64_t)tile[q] * 512 + 2 * t;
    v0[q] = i < n;
    v1[q] = i + 1 < n;
    xv[q] = ld2<true>(a.x, i, n);
    Vv[q] = ld2<true>(a.p.V, i, n);
    pv[q] = make_double2(0.0, 0.0);
    sv[q] = make_double2(0.0, 0.0);
  }
  auto apply = [&](int q, double2 w) -> double2 {
    const double dn = dsm[lrow[q] + 1];
    const double up = dsm[lrow[q] + 4];
    double2 y;
    y.x = v0[q] ? stencil_row(coef, Vv[q].x, w.x, v1[q] ? w.y : 0.0, dn) : 0.0;
    y.y = v1[q] ? stencil_row(coef, Vv[q].y, w.y, up, w.x) : 0.0;
    if (has_shift) {
      y.x = __dsub_rn(y.x, __dmul_rn(sh, w.x));
      y.y = __dsub_rn(y.y, __dmul_rn(sh, w.y));
    }
    return y;
  };
  auto stage = [&](const double2* w, double hl, double hr) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PPT; ++q) *reinterpret_cast<double2*>(dsm + 2 + lrow[q]) = w[q];
    if (tid == 0) {
      dsm[1] = hl;
      dsm[2 + ROWS] = hr;
    }
    __syncthreads();
  };

  // ---- start-up: x edges to the two neighbours (slots of their own), r = b - A' x0           (CG.py:26-27)
  if (tid == 0) granule_put(commX + (g * 2 + 0) * 2, 1u, xv[0].x);
  if (tid == 256 * NVB - 1) granule_put(commX + (g * 2 + 1) * 2, 1u, xv[PPT - 1].y);
  if (tid == 0 || tid == 64) {
    const bool left = tid == 0;
    const int peer = left ? g - 1 : g + 1;
    double v = 0.0;
    if (peer >= 0 && peer < G) {
      if (!granule_wait(commX + (peer * 2 + (left ? 1 : 0)) * 2, 1u, v, wall_clock64(), DSEA_GRANULE_TIMEOUT_TICKS))
        sm->bcast[4] = 1.0;
    }
    sm->bcast[left ? 2 : 3] = v;
  }
  __syncthreads();
  bool fail = sm->bcast[4] != 0.0;
  if (fail) {
    if (g == 0 && tid == 0) a.state[DSEA_CG_DONE] = -1.0;
    return;
  }
  stage(xv, sm->bcast[2], sm->bcast[3]);
#pragma unroll
  for (int q = 0; q < PPT; ++q) {
    const double2 Ax = apply(q, xv[q]);
    const double2 bv = ld2<true>(a.b, (int64_t)tile[q] * 512 + 2 * t, n);
    rv[q].x = __dsub_rn(bv.x, Ax.x);
    rv[q].y = __dsub_rn(bv.y, Ax.y);
  }

  // w = A' r and the merged reduction of (gamma, delta): the ONE exchange of an iteration
  unsigned epoch = 1;
  double gamma = 0.0, delta = 0.0;
  auto exchange = [&]() {
    ++epoch;
    stage(rv, 0.0, 0.0);                       // zero halos: the cross terms come from the published edges
    double ga = 0.0, da = 0.0;
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
      wv[q] = apply(q, rv[q]);
      ga = fma(rv[q].x, rv[q].x, ga);
      ga = fma(rv[q].y, rv[q].y, ga);
      da = fma(rv[q].x, wv[q].x, da);
      da = fma(rv[q].y, wv[q].y, da);
    }
    ga = wave_sum(ga);
    da = wave_sum(da);
    if (lane == 0) {
      sm->red[0][wave] = ga;
      sm->red[1][wave] = da;
    }
    __syncthreads();
    gran_u64* slot = commS + (int64_t)(epoch & 1u) * 8 * G;
    if (tid < 4) {
      double v;
      if (tid < 2) {
        v = 0.0;
        for (int k2 = 0; k2 < NWAVES; ++k2) v += sm->red[tid][k2];
      } else if (tid == 2) {
        v = dsm[2];                // first row of this workgroup
      } else {
        v = dsm[2 + ROWS - 1];     // last row
      }
      granule_put(slot + ((int64_t)g * 4 + tid) * 2, epoch, v);
    }
    // gather all 4 G values (threads 0..255, up to four each)
    if (tid < 256) {
      const long long t0 = wall_clock64();
      bool ok = true;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int idx = tid + 256 * m;
        if (idx < 4 * G) {
          double v = 0.0;
          ok &= granule_wait(slot + (int64_t)idx * 2, epoch, v, t0, DSEA_GRANULE_TIMEOUT_TICKS);
          sm->vals[idx] = v;
        }
      }
      if (!ok) sm->bcast[4] = 1.0;
    }
    __syncthreads();
    // wave 0: gamma ; wave 1: delta incl. the cross terms of the workgroup boundaries (fixed order)
    if (wave < 2) {
      double acc = 0.0;
      for (int gg = lane; gg < G; gg += 64) {
        double v = sm->vals[gg * 4 + wave];
        if (wave == 1 && gg + 1 < G) v = fma(2.0 * coef * sm->vals[gg * 4 + 3], sm->vals[(gg + 1) * 4 + 2], v);
        acc += v;
      }
      acc = wave_sum(acc);
      if (lane == 0) sm->bcast[wave] = acc;
    }
    if (tid == 128) {
      sm->bcast[2] = g > 0 ? sm->vals[(g - 1) * 4 + 3] : 0.0;
      sm->bcast[3] = g + 1 < G ? sm->vals[(g + 1) * 4 + 2] : 0.0;
    }
    __syncthreads();
    gamma = sm->bcast[0];
    delta = sm->bcast[1];
    fail = sm->bcast[4] != 0.0;
    // the two edge rows of w receive their neighbours
    if (tid == 0 && v0[0]) wv[0].x = fma(coef, sm->bcast[2], wv[0].x);
    if (tid == 256 * NVB - 1 && v1[PPT - 1]) wv[PPT - 1].y = fma(coef, sm->bcast[3], wv[PPT - 1].y);
  };

  exchange();
  double rn = sqrt(gamma);
  long long iters = 0;
  bool done = rn < a.eps;
  double alpha = gamma / delta, beta = 0.0;
  while (!done && !fail && iters < a.maxiter) {
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
      pv[q].x = fma(beta, pv[q].x, rv[q].x);
      pv[q].y = fma(beta, pv[q].y, rv[q].y);
      sv[q].x = fma(beta, sv[q].x, wv[q].x);
      sv[q].y = fma(beta, sv[q].y, wv[q].y);
      xv[q].x = fma(alpha, pv[q].x, xv[q].x);
      xv[q].y = fma(alpha, pv[q].y, xv[q].y);
      rv[q].x = fma(-alpha, sv[q].x, rv[q].x);
      rv[q].y = fma(-alpha, sv[q].y, rv[q].y);
    }
    const double gamma_old = gamma;
    exchange();
    if (fail) break;
    ++iters;
    rn = sqrt(gamma);
    if (rn < a.eps) {
      done = true;
      break;
    }
    beta = gamma / gamma_old;
    alpha = gamma / (delta - beta * gamma / alpha);
  }
#pragma unroll
  for (int q = 0; q < PPT; ++q) st2<true>(a.x, (int64_t)tile[q] * 512 + 2 * t, n, xv[q]);
  if (g == 0 && tid == 0) {
    a.state[DSEA_CG_RR] = gamma;
    a.state[DSEA_CG_RESNORM] = rn;
    a.state[DSEA_CG_ITERS] = (double)iters;
    a.state[DSEA_CG_DONE] = fail ? -1.0 : (done ? 1.0 : 0.0);
  }
}

// ------------------------------------------------------------------------------------------
// host-side launch wrappers (called from dsea_capi.hip)
// ------------------------------------------------------------------------------------------
// (tuning knobs live in the operator descriptor: OpDesc::tune_tile_log2, OpDesc::tune_csr_group)

static inline int ew_blocks(int64_t n) {
  int64_t nb = (n + 2047) / 2048;  // 256 threads x double2 x 4 iterations
  if (nb < 1) nb = 1;
  if (nb > DSEA_MAX_EW_BLOCKS) nb = DSEA_MAX_EW_BLOCKS;
  return (int)nb;
}
// Kernels with a fused reduction in the CG loop: up to DSEA_PERSIST_MAX_TILES tiles of 512 rows (n <= 2^21) one
// block per tile, so that P[tile] is a function of the tile alone (the "canonical tile" partial the persistent CG
// kernel reproduces); beyond that the capped grid-stride form.
static inline int tile_blocks(int64_t n) {
  const int64_t nt = (n + 511) / 512;
  return nt <= DSEA_PERSIST_MAX_TILES ? (int)(nt < 1 ? 1 : nt) : ew_blocks(n);
}

// the grid rules of the operator kernels, each stated once
static inline int sell_blocks(const SellParams& p) {   // four 64-row slices (one per wave) to a block
  int64_t nb = (p.nslices + 3) / 4;
  if (nb > DSEA_MAX_TFIM_BLOCKS) nb = DSEA_MAX_TFIM_BLOCKS;
  if (nb < 1) nb = 1;
  return (int)nb;
}
static inline int tfim_blocks(const TfimParams& p, int T) {   // one tile of 2^T rows per block
  int64_t nb = ((int64_t)1 << p.L_local) >> T;
  if (nb > DSEA_MAX_TFIM_BLOCKS) nb = DSEA_MAX_TFIM_BLOCKS;  // blocks then walk several tiles
  return (int)nb;
}
// dots pass, wave-owned form: one row of i + 1 partial sums per wave in LDS (see rdots_tile); 64 KiB of dynamic LDS hold
// 4 waves up to i = 2047, 2 waves up to 4095, 1 wave up to 8191 (dsea_ws_create caps kmax at DSEA_MAX_KRYLOV = 8000)
static inline int rdots_waves_per_block(int i) { return (i + 1) <= 2048 ? 4 : ((i + 1) <= 4096 ? 2 : 1); }

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

void launch_finalize1(const double* P, int count, double* out, hipStream_t st) {
  hipLaunchKernelGGL(k_finalize1, dim3(1), dim3(256), 0, st, P, count, out);
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

// partials per basis vector the dots pass of step i leaves in P (row stride g.pstride)
int rdots_partial_count(const TileGeom& g, int i) {
  if (g.split_w) return (int)((g.ntiles + g.dots_nt - 1) / g.dots_nt);
  const int wpb = rdots_waves_per_block(i);
  return (g.nw + wpb - 1) / wpb;
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

void launch_ritz(const TileGeom& g, const double* Q, int64_t ldq, int64_t n, int k, const double* s,
                 double* out, hipStream_t st) {
  launch_axpy_family<1>(g, Q, ldq, n, k, s, out, nullptr, st, nullptr, nullptr, nullptr);
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

void launch_dot(const double* x, const double* y, int64_t n, double* P, double* out, hipStream_t st) {
  const int nb = ew_blocks(n);
  hipLaunchKernelGGL(k_dot, dim3(nb), dim3(256), 0, st, x, y, n, P);
  launch_finalize1(P, nb, out, st);
}

void launch_shift_dot(const double* x, double* y, const double* shift, const double* skip, int64_t n,
                      double* P, double* out, hipStream_t st) {
  const int nb = ew_blocks(n);
  hipLaunchKernelGGL(k_shift_dot, dim3(nb), dim3(256), 0, st, x, y, shift, skip, n, P);
  hipLaunchKernelGGL(k_cg_finalize_slot, dim3(1), dim3(256), 0, st, (const double*)P, nb, out, skip);
}

// y -= shift x with the x.y partials LEFT UNSUMMED (the consumer folds the second stage into its prologue); returns their count
int launch_shift_dot_partials(const double* x, double* y, const double* shift, const double* skip, int64_t n, double* P,
                              hipStream_t st) {
  const int nb = ew_blocks(n);
  hipLaunchKernelGGL(k_shift_dot, dim3(nb), dim3(256), 0, st, x, y, shift, skip, n, P);
  return nb;
}

void launch_axpy(double a_host, const double* a_dev, const double* x, double* y, int64_t n,
                 hipStream_t st) {
  hipLaunchKernelGGL(k_axpy, dim3(ew_blocks(n)), dim3(256), 0, st, a_host, a_dev, x, y, n);
}

void launch_scale_store_fused(const double* r, const double* nP, int nCount, double* q, uint16_t* qs, double* beta_store,
                              int64_t n, hipStream_t st) {
  TfimFusedArgs fa = {nP, nCount, q, qs, beta_store, nullptr, 0};
  hipLaunchKernelGGL(k_scale_store_fused, dim3(ew_blocks(n)), dim3(256), 0, st, r, fa, n);
}

int launch_dot_partials(const double* x, const double* y, int64_t n, double* P, hipStream_t st) {
  const int nb = ew_blocks(n);
  hipLaunchKernelGGL(k_dot, dim3(nb), dim3(256), 0, st, x, y, n, P);
  return nb;
}

void launch_scale_store(const double* r, const double* nrm2, double* q, double* beta_out, int64_t n,
                        hipStream_t st, uint16_t* qs, double* brk, int step) {
  hipLaunchKernelGGL(k_scale_store, dim3(ew_blocks(n)), dim3(256), 0, st, r, nrm2, q, beta_out, n, qs, brk, step);
}

void launch_project_apply(const double* v, const double* a, const double* dot, double* out, int64_t n,
                          hipStream_t st) {
  hipLaunchKernelGGL(k_project_apply, dim3(ew_blocks(n)), dim3(256), 0, st, v, a, dot, out, n);
}

void launch_cg_init(const double* b, const double* Ax0, double* r, double* d, double* state, int64_t n,
                    double* P, hipStream_t st) {
  const int nb = tile_blocks(n);
  hipLaunchKernelGGL(k_cg_state_clear, dim3(1), dim3(64), 0, st, state);
  hipLaunchKernelGGL(k_cg_init, dim3(nb), dim3(256), 0, st, b, Ax0, r, d, n, P);
  launch_finalize1(P, nb, state + DSEA_CG_RR, st);
}

void launch_cg_init_check(double* state, double eps, hipStream_t st) {
  hipLaunchKernelGGL(k_cg_init_check, dim3(1), dim3(1), 0, st, state, eps);
}

void launch_cg_update(double* x, double* r, const double* d, const double* Ad, double* state, int64_t n,
                      double* P, hipStream_t st) {
  const int nb = ew_blocks(n);
  hipLaunchKernelGGL(k_cg_update, dim3(nb), dim3(256), 0, st, x, r, d, Ad, (const double*)state, n, P);
  hipLaunchKernelGGL(k_cg_finalize_rrnew, dim3(1), dim3(256), 0, st, (const double*)P, nb, state);
}

// returns the number of r.r partials left in P (NOT summed: the caller closes them together with the mat-vec's dot)
int launch_pcg_update(double* x, double* r, double* p, double* s, const double* w, const double* state, int64_t n,
                      double* P, hipStream_t st) {
  const int nb = ew_blocks(n);
  hipLaunchKernelGGL(k_pcg_update, dim3(nb), dim3(256), 0, st, x, r, p, s, w, state, n, P);
  return nb;
}

void launch_pcg_scalars(double* state, const double* pair, double eps, int first, hipStream_t st) {
  hipLaunchKernelGGL(k_pcg_scalars, dim3(1), dim3(1), 0, st, state, pair, eps, first);
}

void launch_cg_check(double* state, double eps, hipStream_t st) {
  hipLaunchKernelGGL(k_cg_check, dim3(1), dim3(1), 0, st, state, eps);
}

void launch_cg_direction(const double* r, double* d, const double* state, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_cg_direction, dim3(ew_blocks(n)), dim3(256), 0, st, r, d, state, n);
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
      const int nbk = ew_blocks(op.n);
      hipLaunchKernelGGL(k_shift_dot, dim3(nbk), dim3(256), 0, st, x, y, shift, skip, op.n, P);   // P may be null
      return P ? nbk : 0;
    }
    case OP_STENCIL3: {
      const int nb = tile_blocks(op.st3.n);
      klaunch(ev, k_spmv_stencil3<false>, nb, 256, 0, st, op.st3, x, y, shift, skip, P, plain);
      return nb;
    }
  }
  return -1;
}

// Fused Lanczos tail (beta from the ||r||^2 partials, q = r/beta -> Q[i] (+shadow), u = A q, alpha partials)
// for the operator kinds that have one; returns the number of alpha partials or -1 (caller falls back to the
// unfused sequence scale_store + mat-vec + finalize).
int launch_tfim_fused(const OpDesc& op, const double* r, const double* nP, int nCount, double* q_out, double* y,
                      double* beta_store, double* P, hipStream_t st, EventPair* ev, uint16_t* qs_out, double* brk,
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

// explicit-matrix operand as a parameter: refresh of the SELL copy / sampled outer product, CSR order through rowptr
int launch_sell_update_vals(const OpDesc& op, const int64_t* rowptr, const double* vals_csr, hipStream_t st) {
  const SellParams& p = op.sell;
  const int cap = sell_seg_cap(p);
  hipLaunchKernelGGL(k_sell_update_vals, dim3(sell_blocks(p)), dim3(256), (size_t)cap * 4 * sizeof(double), st, p, rowptr,
                     vals_csr, const_cast<double*>(p.vals), cap);
  return 0;
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

int launch_cg_update_fused(double* x, double* r, const double* d, const double* Ad, const double* state,
                           int parity, const double* dP, int dCount, int64_t n, double* P, hipStream_t st) {
  const int nb = tile_blocks(n);
  hipLaunchKernelGGL(k_cg_update_fused, dim3(nb), dim3(256), 0, st, x, r, d, Ad, state, parity, dP, dCount, n, P);
  return nb;
}

void launch_cg_direction_fused(const double* r, double* d, double* state, int parity, const double* rP,
                               int rCount, double eps, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_cg_direction_fused, dim3(tile_blocks(n)), dim3(256), 0, st, r, d, state, parity, rP, rCount,
                     eps, n);
}

void launch_axpy_multi_dot(double a_host, const double* a_dev, const double* const* xs, int count,
                           const double* shift, const double* skip, const double* x, double* y, int64_t n,
                           double* P, double* dot_out, hipStream_t st, const double* pendP, int pendN, double* pendOut) {
  MultiSrc ms;
  ms.count = count;
  for (int b = 0; b < 6; ++b) ms.p[b] = b < count ? xs[b] : nullptr;
  const int nb = ew_blocks(n);
  hipLaunchKernelGGL(k_axpy_multi_dot, dim3(nb), dim3(256), 0, st, a_host, a_dev, ms, shift, skip, x, y, n, P);
  if (pendP)
    hipLaunchKernelGGL(k_finalize_pair, dim3(2), dim3(256), 0, st, pendP, pendN, pendOut, (const double*)P, nb, dot_out, skip);
  else
    hipLaunchKernelGGL(k_cg_finalize_slot, dim3(1), dim3(256), 0, st, (const double*)P, nb, dot_out, skip);
}

void launch_form_r(const double* u, const double* q1, const double* q2, const double* alpha, const double* beta,
                   double* r, double* r_copy, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_form_r, dim3(ew_blocks(n)), dim3(256), 0, st, u, q1, q2, alpha, beta, r, r_copy, n);
}

void launch_hypercube_flipsum(const double* xT, double* zT, int P, int p, int64_t chunk, hipStream_t st) {
  int64_t nb = ((int64_t)P * chunk + 255) / 256;
  if (nb > DSEA_MAX_EW_BLOCKS) nb = DSEA_MAX_EW_BLOCKS;
  if (nb < 1) nb = 1;
  hipLaunchKernelGGL(k_hypercube_flipsum, dim3((unsigned)nb), dim3(256), 0, st, xT, zT, P, p, chunk);
}

void launch_plz_finish(const double* r, const double* y, const double* pair, double* q, uint16_t* qs, double* u,
                       double* alpha_out, double* beta_out, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_plz_finish, dim3(ew_blocks(n)), dim3(256), 0, st, r, y, pair, q, qs, u, alpha_out,
                     beta_out, n);
}

void launch_plz_finish_form(double* r, const double* y, const double* pair, double* q, uint16_t* qs, const double* qprev,
                            double* alpha_out, double* beta_out, double* r_copy, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_plz_finish_form, dim3(ew_blocks(n)), dim3(256), 0, st, r, y, pair, q, qs, qprev, alpha_out, beta_out,
                     r_copy, n);
}

void launch_finalize_pair(const double* PA, int na, double* outA, const double* PB, int nb, double* outB,
                          const double* skipB, hipStream_t st) {
  hipLaunchKernelGGL(k_finalize_pair, dim3(2), dim3(256), 0, st, PA, na, outA, PB, nb, outB, skipB);
}

int launch_three_term(const double* u, const double* q1, const double* q2, const double* aP, int aCount,
                      double* a_store, const double* beta, double* r, double* P, double* psi, const double* s1,
                      int64_t n, double* brk, hipStream_t st) {
  const int nb = ew_blocks(n);
  hipLaunchKernelGGL(k_three_term, dim3(nb), dim3(256), 0, st, u, q1, q2, aP, aCount, a_store, beta, r, P, psi, s1, n,
                     brk);
  return nb;
}

void launch_finalize_slot(const double* P, int count, double* out, const double* skip, hipStream_t st) {
  hipLaunchKernelGGL(k_cg_finalize_slot, dim3(1), dim3(256), 0, st, P, count, out, skip);
}

// The persistent kernels' workgroups spin on each other: all G must be resident at the same time.  At most one
// workgroup per CU of THIS device (256 on an MI355X in SPX mode, 32 per partition in CPX mode) guarantees that on an
// otherwise idle device when the kernel's registers and LDS admit one workgroup per CU; a launcher that cannot show
// that from its geometry passes the kernel for the occupancy query.  (A device shared with other work is caught by the
// bounded waits -> DSEA_ERR_TIMEOUT.)
int device_cu_count() {
  static thread_local int cu_dev = -1, cu_count = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return -1;
  if (dev != cu_dev) {
    if (hipDeviceGetAttribute(&cu_count, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return -1;
    cu_dev = dev;
  }
  return cu_count;
}
int persist_resident(int G, const void* kernel, int threads, size_t dyn_lds) {
  const int cus = device_cu_count();
  if (cus < 0) return -2;
  if (G > cus) return -1;
  if (kernel) {
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, threads, dyn_lds) != hipSuccess) return -2;
    if (occ < 1) return -1;
  }
  return 0;
}

// Persistent CG (see k_cg_persist_stencil).  Returns 0 if launched, -1 if the problem is outside its envelope
// (then the caller runs the streaming 3-launch form), -2 on a HIP error.  `comm` must hold persist_comm_bytes().
size_t persist_comm_bytes(int64_t n) {
  const int64_t nt = (n + 511) / 512;
  return (size_t)(4 * nt + 20 * 256) * sizeof(unsigned long long);   // (the merged form needs 20 G <= 20 * 256)
}
int launch_cg_persist(const OpDesc& op, const double* shift, const double* b, double* x, double* state, double eps,
                      int64_t maxiter, void* comm, int ppt_override, hipStream_t st, int lose_peer) {
  // mode >= 100: the merged-reduction form (one exchange per iteration, k_cg_persist_stencil_merged) with the
  // geometry code mode - 100
  const bool merged = ppt_override >= 100;
  if (merged) ppt_override -= 100;
  if (op.kind != OP_STENCIL3 || op.st3.halo_lo || op.st3.halo_hi) return -1;
  const int64_t n = op.st3.n;
  const int64_t nt = (n + 511) / 512;
  if (nt > DSEA_PERSIST_CG_MAX_TILES) return -1;
  // Geometry: ppt row pairs per thread, nvb virtual blocks of 256 threads per workgroup.  Override codes (tuning knob
  // dsea_ws_set_persist): 1 / 2 = ppt with nvb = 4; 21 / 22 = ppt 1 / 2 with nvb = 2; 11 / 12 = ppt 1 / 2 with nvb = 1.
  // Measured on MI355X, 1000 fixed iterations, nvb = 4: N = 1e5: 6.1 us / iteration with 1 pair (49 workgroups),
  // 7.4 with 2; N = 2e4: 5.1 vs 6.8; streaming form 10.6 / 9.8.
  int ppt, nvb = 4;
  switch (ppt_override) {
    case 1: case 2: ppt = ppt_override; break;
    case 21: case 22: ppt = ppt_override - 20; nvb = 2; break;
    case 11: case 12: ppt = ppt_override - 10; nvb = 1; break;
    default:   // measured (N = 1e5 / 2e4, us per iteration): nvb 4: 6.2 / 5.2, nvb 2: 5.6 / 4.5, nvb 1: 5.8 / 4.2
      if (nt <= 64) { ppt = 1; nvb = 1; }
      else if (nt <= 512) { ppt = 1; nvb = 2; }
      else { ppt = 2; nvb = 2; }
      // merged form, measured (N = 1e5 / 2e4): (ppt, nvb) = (2,1): 3.26 / 2.92, (1,1): 3.87 / 2.60, (1,2): 3.49 / 2.90,
      // (2,2): 3.48 / 2.97, (1,4): 3.87 / 3.65
      if (merged && nt > 64 && nt <= 512) { ppt = 2; nvb = 1; }
      break;
  }
  const int tpw = nvb * ppt;
  const int G = (int)((nt + tpw - 1) / tpw);
  if (G > 256) {
    return -1;
  }
  // one workgroup (<= 1024 threads, <= 70 KB of LDS) always fits a compute unit of its own: no occupancy query
  if (const int rc = persist_resident(G)) return rc;
  const size_t cbytes = merged ? (size_t)(16 + 4) * G * sizeof(unsigned long long)
                               : (size_t)(4 * nt + 8 * G) * sizeof(unsigned long long);
  if (hipMemsetAsync(comm, 0, cbytes, st) != hipSuccess) return -2;
  PersistArgs a;
  a.p = op.st3;
  a.shift = shift;
  a.b = b;
  a.x = x;
  a.state = state;
  a.eps = eps;
  a.maxiter = (long long)maxiter;
  a.comm = static_cast<unsigned long long*>(comm);
  a.ntiles = (int)nt;
  a.lose_peer = lose_peer;
  const size_t lds = (size_t)(tpw * 512 + 4) * sizeof(double) + (merged ? sizeof(PersistSmM) : sizeof(PersistSm));
  dispatch_int<1, 2>(ppt, [&](auto pairs) {
    dispatch_int<4, 2, 1>(nvb, [&](auto blocks) {
      constexpr int P = decltype(pairs)::value, V = decltype(blocks)::value;
      klaunch(nullptr, merged ? k_cg_persist_stencil_merged<P, V> : k_cg_persist_stencil<P, V>, G, 256 * V, lds, st, a);
    });
  });
  return 0;
}

}  // namespace dsea
