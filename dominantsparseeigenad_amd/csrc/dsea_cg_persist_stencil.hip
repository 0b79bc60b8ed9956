// dsea_cg_persist_stencil.hip -- the persistent single-launch CG of the 3-point stencil, in two forms (two exchanges per
// iteration, bit-identical to the streaming kernels; one merged exchange, an option), the residency gate every persistent
// launcher asks, and launch_cg_persist.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_internal.h"
#include "dsea_device.h"

namespace dsea {

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
