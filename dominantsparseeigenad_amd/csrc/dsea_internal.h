// dsea_internal.h -- shared between the kernel files (device code + launchers) and dsea_capi.hip (C ABI).
#ifndef DSEA_INTERNAL_H
#define DSEA_INTERNAL_H

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <type_traits>

#include "../../include/dsea.h"

#define DSEA_MAX_EW_BLOCKS 2048   /* grid cap of the grid-stride streaming kernels            */
#define DSEA_MAX_WAVE_TILES 8192  /* cap on wave tiles (= partial sums per basis vector)      */
#define DSEA_TFIM_TILE_LOG2 11    /* rows of x staged in LDS per block of the TFIM mat-vec    */
#define DSEA_MAX_TFIM_BLOCKS 4096 /* grid cap of the TFIM mat-vec (<= DSEA_MAX_WAVE_TILES partial slots)   */
#define DSEA_PERSIST_MAX_TILES 4096 /* canonical-tile regime of the CG kernels: n <= 2^21 rows               */
#define DSEA_MAX_KRYLOV 8000       /* cap on kmax: the dots pass keeps one LDS row of k partial sums per wave      */
#define DSEA_PERSIST_CG_MAX_TILES 1024 /* persistent single-launch CG: n <= 2^19 rows                       */
#define DSEA_SCALARS 64
#define DSEA_SCAL_BREAK 20    /* scal[20] = breakdown step, scal[21] = running scale (see broken())     */
#define DSEA_SCAL_PRO 40      /* scal[40] = re-orthogonalise this step, [41] = and the next, [42] = ||A|| estimate, [43] = steps re-orthogonalised, [44] = global ||r||^2 (row-partitioned run) */
/* default threshold of the partial re-orthogonalisation on the estimated |q_i . q_k|: the path's stated tolerance.  Simon's
 * classical sqrt(eps) = 1.5e-8 keeps the Ritz VALUES at full accuracy; the corrections that are dropped from T (Q c with
 * |c| up to the threshold) enter the residual of a Ritz VECTOR at first order, so the vector is only good to ~threshold */
#define DSEA_PRO_DELTA_DEFAULT 1e-10
#define DSEA_SCAL_LZ_FAIL 38  /* scal[38] = 1 when the single-launch Lanczos lost a peer workgroup (timeout) */

namespace dsea {

struct TfimParams {
  int L, L_local;
  int64_t row_offset;
  const double* g_dev;
  double g_const;
  double diag_scale;
};
struct CsrParams {
  int64_t n, nnz;
  const int64_t* rowptr;
  const int32_t* colidx;
  const double* vals;
};
struct SellParams {
  int64_t n, nslices;
  const int64_t* slice_ptr;
  const int32_t* colidx;
  const double* vals;
  // row-partitioned slab (dsea_pop_create_csr; all zero for a one-GPU operator): where x[col] is read from
  //   mode 0: x itself;  1: LOCAL columns in [-hb, n + hb): c < 0 -> halo_lo[c + hb], c >= n -> halo_hi[c - n];
  //   2: GLOBAL columns, read from the all-gathered copy xg
  int mode;
  int64_t hb;
  const double* halo_lo;
  const double* halo_hi;
  const double* xg;
  // 16-bit column deltas (dsea_op_create_sell16): column of element e = colbase[e / 64] + col16[e]; colidx unused (null)
  const int32_t* colbase;
  const uint16_t* col16;
  int xcd;   // 1: XCD-contiguous slice map (dsea_op_set_tuning DSEA_TUNE_SELL_XCD_MAP)
  int nt;    // 1: non-temporal matrix loads (DSEA_TUNE_SELL_NT; 16-bit-column operands)
  int max_width;  // hint: no slice is wider than this many slice columns (0 = unknown; DSEA_TUNE_SELL_MAX_WIDTH)
  int pack2;  // 1: fp64 values and 16-bit deltas packed TWO slice columns to a lane (dsea_op_create_sell16p2)
  // value-coded operand (dsea_op_create_sell16v8): value of element e = vtab[code8[e]] (256 doubles); vals unused (null)
  const uint8_t* code8;
  const double* vtab;
};
struct Stencil3Params {
  int64_t n;
  double coef;
  const double* V;
  const double* halo_lo;
  const double* halo_hi;
};
// the operators' row formulas, shared by the streaming and the persistent kernels (bit-compared between them)
__device__ __forceinline__ double tfim_diag(const TfimParams& p, int64_t i, uint64_t maskL) {
  const uint64_t gi = (uint64_t)(p.row_offset + i);
  const uint64_t rot = ((gi << 1) | (gi >> (p.L - 1))) & maskL;
  const int pop = __popcll(gi ^ rot);
  return p.diag_scale * (double)(-(p.L - 2 * pop));
}
// 3-point stencil + diagonal (schrodinger1D.py:18-27)
__device__ __forceinline__ double stencil_row(double coef, double Vi, double xi, double up, double dn) {
  const double lap = __dadd_rn(__dadd_rn(__dmul_rn(-2.0, xi), up), dn);
  return __dadd_rn(__dmul_rn(coef, lap), __dmul_rn(Vi, xi));
}
struct DenseParams {
  int64_t n, lda;
  const double* A;  // row-major n x n
  int transpose;
};
struct TransferParams {
  int D, d;
  const double* B;  // d x D x D row-major: A itself, or its slice-wise transpose (inside the caller's work buffer)
  double* xT;       // D * D      scratch: the transposed input
  double* T;        // d * D * D  scratch: B_k x
  double* Y;        // d * D * D  scratch: (B_k x) B_k^T
  int transpose;
  const double* Bp; // d * Dp * Dp (Dp = D rounded up to a multiple of 64): B zero-padded, in fragment-packed order (dsea_transfer_mfma.hip)
  double* Tp;       // d * Dp * Dp scratch: B_k x, written and read in fragment-packed order
};
struct SymDenseParams {
  int64_t n, lda, npad;
  const void* A;    // row-major, symmetric, fp64 or fp32 (elem); only the upper triangle is read
  double* work;     // nb x npad doubles of per-tile partial results
  int nb;           // 64-row blocks
  int elem;         // bytes per matrix element: 8 or 4
};
// XYZ spin chain with per-site couplings (dsea_chain.hip): c = (5, L) row-major device array, rows Jx, Jy, Jz, hx, hz -- read
// through the pointer on every launch
struct ChainParams {
  int L;
  const double* c;
};
// XYZ spins on a caller-given bond list (dsea_lattice.hip): bond t joins sites a[t] != b[t] (host copies, the caller's order);
// c = [Jx(nb), Jy(nb), Jz(nb), hx(L), hz(L)] on the device -- read through the pointer on every launch
struct LatticeDesc {
  int L, nb;
  const double* c;
  uint8_t a[DSEA_LATTICE_MAX_BONDS], b[DSEA_LATTICE_MAX_BONDS];
};
// XXZ spins on a caller-given bond list in the sector of ndown set bits (dsea_sector.hip): bond t joins sites a[t] != b[t] (host
// copies, the caller's order); c = [Jxy(nb), Jz(nb), hz(L)] on the device -- read through the pointer on every launch; states
// (n words), lo_rank (2^Llo) and hi_base (2^Lhi), Llo = (L + 1) / 2: the caller's device tables (dsea_sector_build_tables)
#define DSEA_SECTOR_MAX_L 40
struct SectorDesc {
  int L, ndown, nb;
  const double* c;
  const uint64_t* states;
  const uint32_t* lo_rank;
  const uint32_t* hi_base;
  uint8_t a[DSEA_LATTICE_MAX_BONDS], b[DSEA_LATTICE_MAX_BONDS];
};
// The Hubbard model on a caller-given bond list at fixed (nup, ndn) (dsea_hubbard.hip): bond t joins sites a[t] != b[t] (host
// copies, the caller's order); c = [t(nb), V(nb), U(L), eps(L)] on the device -- read through the pointer on every launch; per
// species the caller's device tables of dsea_sector_build_tables at (L, nup) and (L, ndn): states (C(L, .) words), lo_rank
// (2^Llo) and hi_base (2^Lhi), Llo = (L + 1) / 2.  The two triples may be the same pointers when nup == ndn.
struct HubbardDesc {
  int L, nup, ndn, nb;
  const double* c;
  const uint64_t* up_states;
  const uint32_t* up_lo;
  const uint32_t* up_hi;
  const uint64_t* dn_states;
  const uint32_t* dn_lo;
  const uint32_t* dn_hi;
  uint8_t a[DSEA_LATTICE_MAX_BONDS], b[DSEA_LATTICE_MAX_BONDS];
};
// XXZ spins in one magnetisation sector reduced by a lattice-symmetry group with a real one-dimensional character
// (dsea_symsector.hip): bonds and couplings as SectorDesc; ng group elements, bit g of neg set when chi(g) = -1; orb[c] the orbit
// id of parameter c (the couplings are averaged over their orbits); reps (n_rep words s | sigma << 48, increasing), bucket
// (2^Lhi + 1) and perm_tab (ng * ceil(L / 8) * 256): the caller's device tables
struct SymSectorDesc {
  int L, ndown, nb, ng;
  const double* c;
  const uint64_t* reps;
  const uint32_t* bucket;
  const uint64_t* perm_tab;
  uint64_t neg[2];
  uint8_t a[DSEA_LATTICE_MAX_BONDS], b[DSEA_LATTICE_MAX_BONDS];
  uint16_t orb[2 * DSEA_LATTICE_MAX_BONDS + DSEA_SECTOR_MAX_L];
  // spin inversion (dsea_op_create_symsector_flip; all zero otherwise): bit g of flip set when g also flips every spin, eps[i] the
  // sign of site i in the signed orbit mean of hz; has_flip selects the *_flip kernels
  int has_flip;
  uint32_t flip[4];
  int8_t eps[DSEA_SECTOR_MAX_L];
};
// XXZ spins with a coupling on every pair of sites in the sector of ndown set bits (dsea_pairsector.hip): the pairs are
// implicit (lexicographic, i < j); c = [Jxy(P), Jz(P), hz(L)], P = L (L - 1) / 2, on the device -- read through the pointer on
// every launch; states, lo_rank, hi_base: the caller's device tables as in SectorDesc
struct PairSectorDesc {
  int L, ndown;
  const double* c;
  const uint64_t* states;
  const uint32_t* lo_rank;
  const uint32_t* hi_base;
};
enum OpKind { OP_TFIM = 1, OP_CSR = 2, OP_STENCIL3 = 3, OP_SELL = 4, OP_DENSE = 5, OP_TRANSFER = 6, OP_SYMDENSE = 7, OP_CHAIN = 8,
              OP_LATTICE = 9, OP_SECTOR = 10, OP_HUBBARD = 11, OP_SYMSECTOR = 12, OP_PAIRSECTOR = 13 };
struct OpDesc {
  OpKind kind;
  int64_t n;
  int tune_tile_log2;  // TFIM, spin chain, spin lattice: log2 rows of x staged in LDS per block (6..12); spin sector, Hubbard, symmetry sector, pair sector: log2 of the grid cap
  int tune_csr_group;  // CSR: lanes per row, 0 = automatic
  int tune_sell_unroll;  // SELL: slice-column pairs in flight per lane {0 = automatic, 2, 4, 6, 8}; 1 = the round-5 kernel (A/B)
  TfimParams tfim;
  CsrParams csr;
  Stencil3Params st3;
  SellParams sell;
  DenseParams dense;
  TransferParams transfer;
  SymDenseParams symdense;
  ChainParams chain;
  LatticeDesc lattice;
  SectorDesc sector;
  HubbardDesc hubbard;
  SymSectorDesc symsector;
  PairSectorDesc pairsector;
};

// One basis row's storage shadow as the writers see it: bf16 (h), e5m2 codes of q * S (b), or neither.  At most one of
// the two pointers is set; a plain bf16 row pointer converts by itself.
struct ShadowRow {
  uint16_t* h;
  uint8_t* b;
  double S;
  ShadowRow(uint16_t* bf16 = nullptr) : h(bf16), b(nullptr), S(0.0) {}
  ShadowRow(uint8_t* e5m2, double scale) : h(nullptr), b(e5m2), S(scale) {}
};

// how the rows of one vector are cut into wave tiles for the basis-streaming kernels
struct TileGeom {
  int rpl;         // rows per lane (2,4,8,16): a wave tile is 64*rpl rows
  int nw;          // waves launched (<= DSEA_MAX_WAVE_TILES); wave w handles tiles w, w+nw, ...
  int64_t ntiles;  // ceil(n / (64*rpl))
  int pstride;     // stride between the partial rows of two basis vectors (>= nw)
  int split_w;     // 0, or W = waves of one block that share a 128-row tile and split the basis (small n)
  int dots_w;      // split form of the dots pass: waves per block ...
  int dots_nt;     // ... and 128-row sub-tiles per block (1 or 2); partial count = ceil(ntiles / dots_nt)
};

// Run-time value -> template argument, the one way every launcher picks an instantiation: f(int_c<V>{}) for the V equal
// to v, the LAST value listed when none is (the `default:` of a switch); dispatch_bool likewise.  In f,
// decltype(arg)::value is the compile-time value.
template <int V>
using int_c = std::integral_constant<int, V>;
template <int V, int... Rest, class F>
inline void dispatch_int(int v, F&& f) {
  if constexpr (sizeof...(Rest) == 0) {
    f(int_c<V>{});
  } else {
    if (v == V) f(int_c<V>{});
    else dispatch_int<Rest...>(v, f);
  }
}
template <class F>
inline void dispatch_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}
// the two ladders of the basis-streaming kernels (TileGeom): rows per lane, and waves per block of the split form
template <class F>
inline void dispatch_rpl(int rpl, F&& f) { dispatch_int<2, 4, 8, 16>(rpl, f); }
template <class F>
inline void dispatch_split_w(int w, F&& f) { dispatch_int<4, 8, 16>(w, f); }

// optional per-launch HIP-event timing of the dominant kernels (bench.py roofline); host objects only
enum ProfKind { PROF_RDOTS = 0, PROF_AXPY = 1, PROF_SPMV = 2, PROF_KINDS = 3 };
struct EventPair {
  hipEvent_t a, b;
  int kind;
};
// Launch, optionally with a start/stop event pair attached to the dispatch itself (hipExtLaunchKernelGGL): the events
// then carry the kernel's own begin/end timestamps, i.e. the same duration a profiler reports.  The arguments are
// converted to the kernel's parameter types here (a bare nullptr or int is fine at the call site).
template <class... Params, class... Args>
inline void klaunch(EventPair* ev, void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t st,
                    Args&&... args) {
  if (ev)
    hipExtLaunchKernelGGL(kernel, grid, block, lds, st, ev->a, ev->b, 0, static_cast<Params>(args)...);
  else
    hipLaunchKernelGGL(kernel, grid, block, lds, st, static_cast<Params>(args)...);
}
struct Profiler {
  EventPair* pairs;
  int capacity, used;
  EventPair* next(int kind) {
    if (used >= capacity) return nullptr;
    pairs[used].kind = kind;
    return &pairs[used++];
  }
};

struct Workspace {
  int64_t n, npad;
  int kmax;
  int rpl_override;
  int split_override;  // -1 automatic, 0 off, 4/8/16 forced
  int persist_override;  // persistent single-launch CG: -1 automatic, 0 off, 1/2/4 = row pairs per thread forced
  int lz_persist;        // single-launch Lanczos for small problems: -1 automatic (on where it applies), 0 off
  int arnoldi_optimistic;  // dsea_arnoldi_extend: 1 = the second Gram-Schmidt pass is not enqueued; a step failing the DGKS test records itself
  int last_cg_form;      // which form the last dsea_cg_run took (DSEA_CG_FORM_*)
  int lose_peer;         // TEST HOOK (dsea_ws_set_fault_injection): the last workgroup of a persistent launch exits at once
  int reorth_passes;     // Gram-Schmidt passes per Lanczos step: 1 (the reference, Lanczos.py:66) or 2 (CGS2 option)
  int partial_reorth;    // 1 = re-orthogonalise only when the omega recurrence says so (option; dsea_ws_set_partial_reorth)
  double pro_delta;      // its threshold on the estimated |q_i . q_k| (DSEA_PRO_DELTA_DEFAULT)
  double* partials;  // DSEA_MAX_WAVE_TILES * max(kmax,1) doubles (also >= DSEA_MAX_EW_BLOCKS)
  double* aux;       // 6 * DSEA_MAX_WAVE_TILES doubles: small partial buffers that must not alias `partials`
  double* coef;      // kmax doubles
  double* coef2;     // second coefficient vector (Arnoldi: DGKS second pass)
  double* zero;      // one device double that is always 0
  double* scal;      // DSEA_SCALARS doubles
  double* vec[4];    // four work vectors of npad doubles
  Profiler* prof;    // null unless dsea_profile_begin was called
  uint16_t* shadow;  // caller-owned bf16 shadow of the basis (k rows x shadow_ld), or null
  int64_t shadow_ld;
  int shadow_rows;
  double lp_tau;     // low-precision pass allowed while max|c_j| <= lp_tau * ||r||
  uint8_t* shadow8;  // caller-owned 8-bit (e5m2) shadow of the basis, or null; never set together with `shadow`
  int64_t shadow8_ld;
  int shadow8_rows;
  double lp8_tau;    // the same premise for the 8-bit pass
  // the shadow row a writer of basis row `row` keeps current (n: rows of the vector)
  ShadowRow shadow_row(int row, int64_t n) const;
  // row-partitioned library driver: dsea_plz_correct leaves its ||r||^2 partials un-summed (defer_norm) and the NEXT
  // dot-closing call of the step sums both in one launch (k_finalize_pair) -- bit-identical, one launch fewer per step
  int callable_na;       // dsea_lanczos_callable_alpha: number of alpha partials left in aux[0..] for the next callable step
  int defer_norm;
  const double* pend_P;
  int pend_count;
  double* pend_out;
  TileGeom geom(int64_t n_rows) const;
  // what the single-launch kernels may borrow for their exchange buffers: the whole partial-sum area ((kmax + 1) rows, see
  // ws_layout) and the first four rows of aux
  size_t partials_bytes() const { return (size_t)DSEA_MAX_WAVE_TILES * (size_t)((kmax < 1 ? 1 : kmax) + 1) * sizeof(double); }
  size_t aux_bytes() const { return (size_t)4 * DSEA_MAX_WAVE_TILES * sizeof(double); }
};

// grid of the grid-stride streaming kernels
inline int ew_blocks(int64_t n) {
  int64_t nb = (n + 2047) / 2048;  // 256 threads x double2 x 4 iterations
  if (nb < 1) nb = 1;
  if (nb > DSEA_MAX_EW_BLOCKS) nb = DSEA_MAX_EW_BLOCKS;
  return (int)nb;
}
// Kernels with a fused reduction in the CG loop: up to DSEA_PERSIST_MAX_TILES tiles of 512 rows (n <= 2^21) one
// block per tile, so that P[tile] is a function of the tile alone (the "canonical tile" partial the persistent CG
// kernel reproduces); beyond that the capped grid-stride form.
inline int tile_blocks(int64_t n) {
  const int64_t nt = (n + 511) / 512;
  return nt <= DSEA_PERSIST_MAX_TILES ? (int)(nt < 1 ? 1 : nt) : ew_blocks(n);
}

void launch_finalize1(const double* P, int count, double* out, hipStream_t st);
int launch_three_term(const double* u, const double* q1, const double* q2, const double* aP, int aCount,
                      double* a_store, const double* beta, double* r, double* P, double* psi, const double* s1,
                      int64_t n, double* brk, hipStream_t st);
void launch_finalize_slot(const double* P, int count, double* out, const double* skip, hipStream_t st);
void launch_rdots(const TileGeom& g, const double* Q, int64_t ldq, int64_t n, int i, const double* u,
                  const double* alpha, const double* beta, double* r, double* P, double* c_out,
                  hipStream_t st, EventPair* ev = nullptr, const double* aP = nullptr, int aCount = 0,
                  double* a_store = nullptr, bool want_rr = false, double* brk = nullptr,
                  const double* sel = nullptr, bool sel_exit = false, const double* uscale = nullptr);
// uscale (u divided by *uscale on the fly) exists for the wave-owned geometry without the partial-reorthogonalisation gate
inline bool rdots_uscale_ok(const TileGeom& g) { return g.split_w == 0; }   // sel: device flag of the partial re-orthogonalisation,
                  // 0 = no basis vectors on this step (three-term update and ||r||^2 only; sel_exit: return at once)
int launch_axpy_norm_lp(int64_t n, int rps, const double* Q, int64_t ldq, const uint16_t* Qs, int64_t lds, int i,
                        const double* c, double tau, double* r, double* P, double* lp_count, hipStream_t st,
                        EventPair* ev = nullptr, const double* brk = nullptr);
// the 8-bit form of the same pass (wave-owned geometry only): Qs8 holds e5m2 codes of q * scale
int launch_axpy_norm_lp8(int64_t n, const double* Q, int64_t ldq, const uint8_t* Qs8, int64_t ld8, double scale, int i,
                         const double* c, double tau, double* r, double* P, double* lp_count, hipStream_t st,
                         EventPair* ev = nullptr, const double* brk = nullptr);
// scale of the 8-bit codes of an n-row run: 2^ceil(log2(n) / 2), at most 2^15 (|q| <= 1 stays below the largest code)
inline double shadow8_scale(int64_t n) {
  int e = 0;
  while (e < 15 && ((int64_t)1 << (2 * e)) < n) ++e;
  return (double)((int64_t)1 << e);
}
int launch_tfim_fused(const OpDesc& op, const double* r, const double* nP, int nCount, double* q_out, double* y,
                      double* beta_store, double* P, hipStream_t st, EventPair* ev = nullptr,
                      ShadowRow qs_out = ShadowRow(), double* brk = nullptr, int step = 0);
int launch_cg_update_fused(double* x, double* r, const double* d, const double* Ad, const double* state,
                           int parity, const double* dP, int dCount, int64_t n, double* P, hipStream_t st);
void launch_cg_direction_fused(const double* r, double* d, double* state, int parity, const double* rP,
                               int rCount, double eps, int64_t n, hipStream_t st);
void launch_axpy_norm(const TileGeom& g, const double* Q, int64_t ldq, int64_t n, int i, const double* c,
                      double* r, double* P, double* nrm2_out, hipStream_t st, EventPair* ev = nullptr,
                      const double* brk = nullptr, const double* sel = nullptr);
void launch_ritz(const TileGeom& g, const double* Q, int64_t ldq, int64_t n, int k, const double* s,
                 double* out, hipStream_t st);
void launch_dot(const double* x, const double* y, int64_t n, double* P, double* out, hipStream_t st);
void launch_pro_update(const double* alphas, const double* betas, const double* rrP, int rrCount, double* rr_store,
                       double* om, int ld, double* flag, double* state, int i, double eps1, double delta,
                       const double* brk, hipStream_t st);
int rdots_partial_count(const TileGeom& g, int i);
void launch_probe(const double* x, double* y, int64_t n, double* P, int nP, hipStream_t st);   // y != null: copy
void launch_shift_dot(const double* x, double* y, const double* shift, const double* skip, int64_t n,
                      double* P, double* out, hipStream_t st);
int launch_shift_dot_partials(const double* x, double* y, const double* shift, const double* skip, int64_t n, double* P,
                              hipStream_t st);
void launch_axpy(double a_host, const double* a_dev, const double* x, double* y, int64_t n, hipStream_t st);
void launch_scale_store(const double* r, const double* nrm2, double* q, double* beta_out, int64_t n,
                        hipStream_t st, ShadowRow qs = ShadowRow(), double* brk = nullptr, int step = 0);
void launch_scale_store_fused(const double* r, const double* nP, int nCount, double* q, ShadowRow qs, double* beta_store,
                              int64_t n, hipStream_t st);
int launch_dot_partials(const double* x, const double* y, int64_t n, double* P, hipStream_t st);
void launch_project_apply(const double* v, const double* a, const double* dot, double* out, int64_t n,
                          hipStream_t st);
void launch_cg_init(const double* b, const double* Ax0, double* r, double* d, double* state, int64_t n,
                    double* P, hipStream_t st);
void launch_cg_init_check(double* state, double eps, hipStream_t st);
void launch_cg_update(double* x, double* r, const double* d, const double* Ad, double* state, int64_t n,
                      double* P, hipStream_t st);
void launch_cg_check(double* state, double eps, hipStream_t st);
int launch_pcg_update(double* x, double* r, double* p, double* s, const double* w, const double* state, int64_t n,
                      double* P, hipStream_t st);
void launch_pcg_scalars(double* state, const double* pair, double eps, int first, hipStream_t st);
void launch_cg_direction(const double* r, double* d, const double* state, int64_t n, hipStream_t st);
void launch_axpy_multi_dot(double a_host, const double* a_dev, const double* const* xs, int count,
                           const double* shift, const double* skip, const double* x, double* y, int64_t n,
                           double* P, double* dot_out, hipStream_t st, const double* pendP = nullptr, int pendN = 0,
                           double* pendOut = nullptr);
void launch_form_r(const double* u, const double* q1, const double* q2, const double* alpha, const double* beta,
                   double* r, double* r_copy, int64_t n, hipStream_t st);
void launch_hypercube_flipsum(const double* xT, double* zT, int P, int p, int64_t chunk, hipStream_t st);
void launch_plz_finish(const double* r, const double* y, const double* pair, double* q, uint16_t* qs, double* u,
                       double* alpha_out, double* beta_out, int64_t n, hipStream_t st);
void launch_plz_finish_form(double* r, const double* y, const double* pair, double* q, uint16_t* qs, const double* qprev,
                            double* alpha_out, double* beta_out, double* r_copy, int64_t n, hipStream_t st);
void launch_finalize_pair(const double* PA, int na, double* outA, const double* PB, int nb, double* outB,
                          const double* skipB, hipStream_t st);
// dsea_deflated.hip (lowest-nev eigenpairs)
void launch_ritz_block(const TileGeom& g, const double* Q, int64_t ldq, int64_t n, int k, const double* S, int64_t lds,
                       int m, double* Y, int64_t ldy, hipStream_t st);
void launch_block_project(const double* v, const double* Psi, int64_t ldpsi, int m, double* out, double* coef_out,
                          int64_t n, double* P, int pstride, hipStream_t st);
void launch_dfl_restart(const double* b, const double* Ax, const double* x, const double* shift, const double* Psi,
                        int64_t ldpsi, int m, double* r, double* d, double* state, double eps, int keep_iters, int64_t n,
                        double* P, int pstride, double* rP, hipStream_t st);
int launch_dfl_update(double* x, double* r, const double* d, const double* Ad, const double* state, int parity,
                      const double* dP, int dCount, const double* Psi, int64_t ldpsi, int m, int64_t n, double* P,
                      int pstride, hipStream_t st);
int launch_dfl_reproject(double* r, const double* Psi, int64_t ldpsi, int m, const double* P, int count, int pstride,
                         double* rP, const double* done, int64_t n, hipStream_t st);
// dsea_krylov.hip
bool blas_available();
int blas_apply(const OpDesc& op, const double* x, double* y, hipStream_t st);
void launch_transpose_sq(const double* in, double* out, int D, int batch, hipStream_t st);
void arnoldi_orth(Workspace& w, int64_t n, const double* u, const double* shift_or_zero, double* V, int64_t ldv, int j,
                  double* hcol, double* brk, double* skip, double* nrm1, double* nrm2, hipStream_t st,
                  bool optimistic = false);
int arnoldi_step(const OpDesc& op, Workspace& w, const double* shift_or_zero, double* V, int64_t ldv, int j,
                 double* hcol, double* brk, double* skip, double* nrm1, double* nrm2, hipStream_t st,
                 bool optimistic = false);
void launch_residual(const double* b, const double* u, double* r, int64_t n, double* P, double* nrm2_out,
                     hipStream_t st);
void launch_gmres_begin(const double* nrm2, double target, double* g, int m, double* state, double* brk,
                        hipStream_t st);
void launch_gmres_givens(double* H, int ldh, int j, double* cs, double* sn, double* g, double target, double* state,
                         double* brk, hipStream_t st);
void launch_gmres_solve(const double* H, int ldh, int m, const double* g, const double* state, double* y,
                        hipStream_t st);
size_t persist_comm_bytes(int64_t n);
// Residency gate of the persistent single-launch kernels, whose workgroups wait on each other: all G must be resident
// at once.  device_cu_count(): CUs of the current device, cached per host thread, -1 on a HIP error.  persist_resident():
// 0 if G workgroups fit one per CU -- and, when `kernel` is given, the occupancy query admits one workgroup of `threads`
// threads and `dyn_lds` bytes of dynamic LDS per CU --, -1 if not (the caller takes the multi-launch kernels), -2 on a
// HIP error.
int device_cu_count();
int persist_resident(int G, const void* kernel = nullptr, int threads = 0, size_t dyn_lds = 0);
int launch_cg_persist(const OpDesc& op, const double* shift, const double* b, double* x, double* state, double eps,
                      int64_t maxiter, void* comm, int ppt_override, hipStream_t st, int lose_peer = 0);
int launch_spmv(const OpDesc& op, const double* x, double* y, const double* shift, const double* skip,
                double* P, hipStream_t st, EventPair* ev = nullptr);
int launch_sell_update_vals(const OpDesc& op, const int64_t* rowptr, const double* vals_csr, hipStream_t st);
int launch_sddmm(const OpDesc& op, const int64_t* rowptr, const double* v1, const double* v2, double alpha, int accumulate,
                 bool sym, double* out, hipStream_t st);
// dsea_chain.hip (XYZ spin chain): the mat-vec of launch_spmv's OP_CHAIN case; the 5 L bilinear forms v1^T (dH/dp) v2 into out
// through per-block partials in the caller's scratch (chain_forms_scratch_doubles(L) doubles); both return -1 when L or the
// tile is out of range
int launch_spmv_chain(const OpDesc& op, const double* x, double* y, const double* shift, const double* skip, double* P,
                      hipStream_t st, EventPair* ev);
int launch_chain_forms(const OpDesc& op, const double* v1, const double* v2, double* out, double* scratch, hipStream_t st);
int64_t chain_forms_scratch_doubles(int L);
// dsea_lattice.hip (XYZ spins on a bond list): the mat-vec of launch_spmv's OP_LATTICE case; the 3 nb + 2 L bilinear forms
// v1^T (dH/dp) v2 into out through per-block partials in the caller's scratch (lattice_forms_scratch_doubles(L, nb) doubles);
// both return -1 when L, nb or the tile is out of range
int launch_spmv_lattice(const OpDesc& op, const double* x, double* y, const double* shift, const double* skip, double* P,
                        hipStream_t st, EventPair* ev);
int launch_lattice_forms(const OpDesc& op, const double* v1, const double* v2, double* out, double* scratch, hipStream_t st);
int64_t lattice_forms_scratch_doubles(int L, int nb);
// dsea_sector.hip (XXZ spins on a bond list in one magnetisation sector): the sizes n = C(L, ndown), 2^Llo, 2^Lhi (false when
// L, ndown or n is out of range); the three table fills; the mat-vec of launch_spmv's OP_SECTOR case; the 2 nb + L bilinear
// forms v1^T (dH/dp) v2 into out through per-block partials in the caller's scratch (sector_forms_scratch_doubles doubles);
// the launchers return -1 when the descriptor is out of range
bool sector_sizes(int L, int ndown, int64_t* n, int64_t* n_lo, int64_t* n_hi);
int launch_sector_build_tables(int L, int ndown, uint64_t* states, uint32_t* lo_rank, uint32_t* hi_base, hipStream_t st);
int launch_spmv_sector(const OpDesc& op, const double* x, double* y, const double* shift, const double* skip, double* P,
                       hipStream_t st, EventPair* ev);
int launch_sector_forms(const OpDesc& op, const double* v1, const double* v2, double* out, double* scratch, hipStream_t st);
int64_t sector_forms_scratch_doubles(int64_t n, int L, int nb);
// dsea_hubbard.hip (the Hubbard model on a bond list at fixed (nup, ndn)): the sizes n_up = C(L, nup), n_dn = C(L, ndn),
// n = n_up n_dn (false when L, nup, ndn or n is out of range); the mat-vec of launch_spmv's OP_HUBBARD case; the 2 nb + 2 L
// bilinear forms v1^T (dH/dp) v2 into out through per-block partials in the caller's scratch (hubbard_forms_scratch_doubles
// doubles); the launchers return -1 when the descriptor is out of range
bool hubbard_sizes(int L, int nup, int ndn, int64_t* n, int64_t* n_up, int64_t* n_dn);
int launch_spmv_hubbard(const OpDesc& op, const double* x, double* y, const double* shift, const double* skip, double* P,
                        hipStream_t st, EventPair* ev);
int launch_hubbard_forms(const OpDesc& op, const double* v1, const double* v2, double* out, double* scratch, hipStream_t st);
int64_t hubbard_forms_scratch_doubles(int64_t n, int L, int nb);
// dsea_symsector.hip (the spin sector reduced by a lattice-symmetry group): the sizes n_sector = C(L, ndown), 2^Lhi + 1 buckets
// and the words of perm_tab (false when L, ndown, n_sector or ng is out of range); the table fills; the mat-vec of launch_spmv's
// OP_SYMSECTOR case; the 2 nb + L orbit-averaged bilinear forms into out through per-block partials in the caller's scratch
// (symsector_forms_scratch_doubles doubles); the op launchers return -1 when the descriptor is out of range
bool symsector_sizes(int L, int ndown, int ng, int64_t* n_sector, int64_t* n_bucket, int64_t* n_perm);
int launch_symsector_fill_perm(int L, int ng, const int32_t* perms_host, uint64_t* perm_tab, hipStream_t st);
int launch_symsector_classify(int L, int ndown, int ng, const uint64_t neg[2], const uint64_t* perm_tab, int64_t first,
                              int64_t count, uint64_t* slab, hipStream_t st);
int launch_symsector_classify_flip(int L, int ndown, int ng, const uint64_t neg[2], const uint32_t flip[4], const uint64_t* perm_tab,
                                   int64_t first, int64_t count, uint64_t* slab, hipStream_t st);
int launch_symsector_fill_buckets(int L, int64_t n_rep, const uint64_t* reps, uint32_t* bucket, hipStream_t st);
int launch_spmv_symsector(const OpDesc& op, const double* x, double* y, const double* shift, const double* skip, double* P,
                          hipStream_t st, EventPair* ev);
int launch_symsector_forms(const OpDesc& op, const double* v1, const double* v2, double* out, double* scratch, hipStream_t st);
int64_t symsector_forms_scratch_doubles(int64_t n, int L, int nb);
// dsea_pairsector.hip (XXZ spins with all-pair couplings in one magnetisation sector, on the tables of dsea_sector.hip): the
// mat-vec of launch_spmv's OP_PAIRSECTOR case; the 2 P + L bilinear forms v1^T (dH/dp) v2 into out (the xy forms by gathers,
// the zz and z forms by a Gram product on the matrix cores) through partials in the caller's scratch
// (pairsector_forms_scratch_doubles doubles); the launchers return -1 when the descriptor is out of range
int launch_spmv_pairsector(const OpDesc& op, const double* x, double* y, const double* shift, const double* skip, double* P,
                           hipStream_t st, EventPair* ev);
int launch_pairsector_forms(const OpDesc& op, const double* v1, const double* v2, double* out, double* scratch, hipStream_t st);
int64_t pairsector_forms_scratch_doubles(int64_t n, int L);
// dsea_rdm.hip (reduced density matrices of a bipartition of the sites, docs/design/21-reduced-density-matrix.md).  RdmSites:
// a[k] the site of bit k of the A-word (the caller's order), b[k] that of the B-word (the other sites, increasing).  RdmBlocks:
// block c holds m0 + c set bits in A; off = its offset into idx, ooff = into the flat output (ooff[nblk] = the output length),
// dA x dB its slice.  rdm_geometry fills them on the host (ndown < 0: the full 2^L space) and is false for every argument the
// ABI refuses; the launchers return -1 when a work list does not fit 31 bits.
#define DSEA_RDM_MAX_LA DSEA_RDM_MAX_SITES      /* (DSEA_RDM_MAX_BLOCKS = DSEA_RDM_MAX_SITES + 1: include/dsea.h) */
struct RdmSites {
  int L, LA;
  uint8_t a[DSEA_RDM_MAX_LA], b[DSEA_SECTOR_MAX_L];
};
struct RdmBlocks {
  int nblk, m0;
  int32_t off[DSEA_RDM_MAX_BLOCKS], dA[DSEA_RDM_MAX_BLOCKS], dB[DSEA_RDM_MAX_BLOCKS], ooff[DSEA_RDM_MAX_BLOCKS + 1];
};
struct RdmGeom {
  int L, ndown;
  int64_t n, out_len;
  RdmSites sites;
  RdmBlocks blk;
};
bool rdm_geometry(int L, int ndown, int LA, const int32_t* sites, RdmGeom* g);
int64_t rdm_scratch_doubles(const RdmGeom& g);
int launch_rdm_index(const RdmGeom& g, const uint32_t* lo_rank, const uint32_t* hi_base, int32_t* idx, hipStream_t st);
int launch_rdm_cross(const RdmGeom& g, const int32_t* idx, const double* x, const double* y, double* out, double* scratch,
                     int tile, hipStream_t st);
int launch_rdm_pull(const RdmGeom& g, const int32_t* idx, const double* G, const double* y, double* out, int transpose,
                    hipStream_t st);
// The two ladder files, dsea_ladder.hip and dsea_hubbard_ladder.hip (docs/design/38-ladder-parts.md), share their host rules,
// stated here once; their launchers and their C entries ask these and nothing else.
// the grid cap of a ladder launch is 2^grid_log2 blocks: 6 .. 12, or 0 for the default 12
inline bool ladder_grid_ok(int grid_log2) { return grid_log2 == 0 || (grid_log2 >= 6 && grid_log2 <= 12); }
// one block per 256 rows up to that cap; beyond it blocks walk row ranges
inline int ladder_blocks(int64_t n, int grid_log2) {
  int64_t nblk = (n + 255) / 256;
  const int64_t cap = (int64_t)1 << (grid_log2 == 0 ? 12 : grid_log2);
  if (nblk > cap) nblk = cap;
  return (int)nblk;
}
// the scratch doubles of a two-stage sum of `terms` values (the L site forms, the R column dots) over the destination rows:
// one partial per term and block at any grid cap -- the largest cap gives the most blocks
inline int64_t ladder_partials(int64_t n_dst, int terms) {
  int64_t nblk = (n_dst + 255) / 256;
  if (nblk > DSEA_MAX_TFIM_BLOCKS) nblk = DSEA_MAX_TFIM_BLOCKS;
  return nblk * terms;
}
// dsea_ladder.hip (linear maps between two magnetisation sectors, docs/design/24-dynamics.md): sigma^-(c) (step +1), Z(c)
// (step 0) and sigma^+(c) (step -1) from the sector (L, ndown_src) to (L, ndown_src + step) as gathers over the destination
// rows, on the state table of the destination and the two rank tables of the source; the L site forms v1^T (dS/dc_i) v2 into
// out through per-block partials in the caller's scratch (ladder_partials(n_dst, L) doubles).  ladder_sizes is false, and
// the launchers return -1, for a step outside -1 .. 1, a sector outside the limits of sector_sizes, a grid_log2 that
// ladder_grid_ok refuses, or a null table.
bool ladder_sizes(int L, int ndown_src, int step, int64_t* n_src, int64_t* n_dst);
int launch_sector_ladder(int L, int ndown_src, int step, const double* c, const uint64_t* states_dst, const uint32_t* lo_rank_src,
                         const uint32_t* hi_base_src, const double* x, double* y, int grid_log2, hipStream_t st);
int launch_sector_ladder_forms(int L, int ndown_src, int step, const uint64_t* states_dst, const uint32_t* lo_rank_src,
                               const uint32_t* hi_base_src, const double* v1, const double* v2, double* out, double* scratch,
                               int grid_log2, hipStream_t st);
// The block forms (docs/design/35-finite-temperature-dynamics.md): Y = S(c) X for a block fp64 [n, R] row-major, R in {1, 2, 4, 8}
// (column j bit for bit launch_sector_ladder on column j), and out[j] = sum_r' Lft[r', j] (S(c) X)[r', j] through per-block partials
// in the caller's scratch (ladder_partials(n_dst, R) doubles).  The same -1 as above; the caller has checked R.
int launch_sector_ladder_block(int L, int ndown_src, int step, int R, const double* c, const uint64_t* states_dst,
                               const uint32_t* lo_rank_src, const uint32_t* hi_base_src, const double* X, double* Y, int grid_log2,
                               hipStream_t st);
int launch_sector_ladder_block_dots(int L, int ndown_src, int step, int R, const double* c, const uint64_t* states_dst,
                                    const uint32_t* lo_rank_src, const uint32_t* hi_base_src, const double* Lft, const double* X,
                                    double* out, double* scratch, int grid_log2, hipStream_t st);
// dsea_hubbard_ladder.hip (linear maps between two particle-number sectors of the Hubbard space,
// docs/design/25-hubbard-ladder.md): sum_i c_i c+_{i s} (step +1), sum_i c_i n_{i s} (step 0) and sum_i c_i c_{i s} (step -1) of the
// species s (0 up, 1 dn) from (L, nup_src, ndn_src) to the sector with that species' count changed by step, as gathers over
// the destination rows, on the state table of the moving species at its destination count and its two rank tables at its source
// count; the L site forms v1^T (dS/dc_i) v2 into out through per-block partials in the caller's scratch
// (ladder_partials(n_dst, L) doubles).  hubbard_ladder_sizes is false, and the launchers return -1, for a species outside
// {0, 1}, a step outside -1 .. 1, a sector outside the limits of hubbard_sizes, a grid_log2 that ladder_grid_ok refuses, or a
// null table.
bool hubbard_ladder_sizes(int L, int nup_src, int ndn_src, int species, int step, int64_t* n_src, int64_t* n_dst,
                          int64_t* n_dn_src, int64_t* n_dn_dst);
int launch_hubbard_ladder(int L, int nup_src, int ndn_src, int species, int step, const double* c, const uint64_t* states_dst,
                          const uint32_t* lo_rank_src, const uint32_t* hi_base_src, const double* x, double* y, int grid_log2,
                          hipStream_t st);
int launch_hubbard_ladder_forms(int L, int nup_src, int ndn_src, int species, int step, const uint64_t* states_dst,
                                const uint32_t* lo_rank_src, const uint32_t* hi_base_src, const double* v1, const double* v2,
                                double* out, double* scratch, int grid_log2, hipStream_t st);
// The block forms (docs/design/37-hubbard-finite-temperature-dynamics.md): Y = S(c) X for a block fp64 [n, R] row-major, R in
// {1, 2, 4, 8} (column j bit for bit launch_hubbard_ladder on column j), and out[j] = sum_r' Lft[r', j] (S(c) X)[r', j] through
// per-block partials in the caller's scratch (ladder_partials(n_dst, R) doubles).  The same -1 as above; the caller has
// checked R.
int launch_hubbard_ladder_block(int L, int nup_src, int ndn_src, int species, int step, int R, const double* c,
                                const uint64_t* states_dst, const uint32_t* lo_rank_src, const uint32_t* hi_base_src,
                                const double* X, double* Y, int grid_log2, hipStream_t st);
int launch_hubbard_ladder_block_dots(int L, int nup_src, int ndn_src, int species, int step, int R, const double* c,
                                     const uint64_t* states_dst, const uint32_t* lo_rank_src, const uint32_t* hi_base_src,
                                     const double* Lft, const double* X, double* out, double* scratch, int grid_log2,
                                     hipStream_t st);
// dsea_hubbard_pair.hip (linear maps that move one particle of each species between two Hubbard sectors,
// docs/design/41-hubbard-pair-ladder.md): sum_ij W_ij A_{i up} B_{j dn} (order 0; order 1 is the down operator left, the negative)
// from (L, nup_src, ndn_src) to (nup_src + step_up, ndn_src + step_dn), A, B = c+ for a step of +1 and c for -1, as a gather
// over the destination rows; W fp64 [L, L] on the device.  tables: for the up and then for the down species, the state table at
// its destination count and lo_rank, hi_base at its source count.  The L^2 site-pair forms v1^T (dP/dW_ij) v2 go into out
// through per-block partials in the caller's scratch (ladder_partials(n_dst, L * L) doubles).  The grid rules are those of the
// ladder files above.  hubbard_pair_sizes is false, and the launchers return -1, for a step that is not +-1, an order outside
// {0, 1}, a sector outside the limits of hubbard_sizes, a grid_log2 that ladder_grid_ok refuses, or a null table.
bool hubbard_pair_sizes(int L, int nup_src, int ndn_src, int step_up, int step_dn, int order, int64_t* n_src, int64_t* n_dst,
                        int64_t* n_dn_src, int64_t* n_dn_dst);
int launch_hubbard_pair(int L, int nup_src, int ndn_src, int step_up, int step_dn, int order, const double* W,
                        const void* const tables[6], const double* x, double* y, int grid_log2, hipStream_t st);
int launch_hubbard_pair_forms(int L, int nup_src, int ndn_src, int step_up, int step_dn, int order,
                              const void* const tables[6], const double* v1, const double* v2, double* out, double* scratch,
                              int grid_log2, hipStream_t st);
// dsea_sector_block.hip (the bond-list sector Hamiltonian on a block of R vectors, docs/design/27-finite-temperature.md): a block is
// fp64 [n, R] row-major, R in {1, 2, 4, 8}.  launch_sector_block_apply: Y = H X (column j bit for bit the single-vector mat-vec).
// launch_sector_block_lanczos: block_lanczos_drive (below) with the file's Lanczos-step kernel as the mat-vec.  The launchers
// return -1 when the descriptor is out of range; the callers check R.
int launch_sector_block_apply(const OpDesc& op, int R, const double* X, double* Y, hipStream_t st);
int launch_sector_block_lanczos(const OpDesc& op, int R, int k, double* Q, double* W, double* norm2, double* alphas, double* betas,
                                int32_t* steps, double* scratch, hipStream_t st);
// launch_sector_block_chebyshev (docs/design/31-chebyshev-propagator.md): ACC[a] = sum_{m < M} coeffs[a * M + m] T_m((H - centre)
// / halfwidth) X, a in [0, A), ACC [A, n, R], in M - 1 launches of k_cheb_sector_block<R, A>; coeffs is a HOST array, U and V are
// work blocks, X is not written, nothing is read back.  The blocks launched, or -1 for a descriptor out of range.
int launch_sector_block_chebyshev(const OpDesc& op, int R, int A, int M, double centre, double halfwidth, const double* coeffs,
                                  const double* X, double* U, double* V, double* ACC, hipStream_t st);
// launch_sector_block_moments (docs/design/33-chebyshev-moments.md): MU[m, j] = l_j . T_m((H - centre) / halfwidth) x_j, m < M,
// l = X for a null Y (self mode, ceil(M / 2) orders) or Y (left mode, M - 1 orders): block_moments_drive (below) with the file's
// k_cheb_sector_moments<R, LEFT> as the step.  Returns 0, or -1 for a descriptor out of range.
int launch_sector_block_moments(const OpDesc& op, int R, int M, double centre, double halfwidth, const double* X, const double* Y,
                                double* U, double* V, double* MU, double* scratch, hipStream_t st);
// dsea_block_moments.hip (the finish kernel and the launch schedule of the Chebyshev moments for any operator): K = ceil(M / 2)
// orders (left: M - 1) on nblk blocks of 256 rows, each the caller's step(x, old, out, first, P) -- one order of the recurrence,
// out = g (H x - centre x) [- old], with the per-block partials of a_j = l_j . x_j and b_j = l_j . out_j in P[(which R + j) nblk
// + block] -- and one launch of k_cheb_moments_finish<R>.  Order 1 is first with x = X, out = U; order 2 x = U, old = X, out = V;
// then old == out, U and V in turn.  ON RETURN T_K X is in U for odd K and in V for even K, and T_{K-1} X in the other work block
// (in X for K = 1), so that a caller can continue the run.  Scratch of block_moments_scratch_doubles(n, R) = 2 R min(4096,
// ceil(n / 256)) doubles (enough for every grid cap).  Nothing is read back, no synchronise, no allocation.  Returns 0.
int64_t block_moments_scratch_doubles(int64_t n, int R);
typedef std::function<void(const double* x, const double* old, double* out, int first, double* P)> BlockMomentsStep;
int block_moments_drive(int64_t n, int nblk, int R, int M, bool left, const double* X, double* U, double* V, double* MU,
                        double* scratch, hipStream_t st, const BlockMomentsStep& step);
// dsea_hubbard_block.hip (the Hubbard Hamiltonian on a block of R vectors, docs/design/28-hubbard-finite-temperature.md): the twins
// of launch_sector_block_apply and launch_sector_block_lanczos for an OP_HUBBARD descriptor; column j of Y = H X is bit for bit
// the single-vector mat-vec without a shift.  -1 when the descriptor is out of range; the callers check R.
int launch_hubbard_block_apply(const OpDesc& op, int R, const double* X, double* Y, hipStream_t st);
int launch_hubbard_block_lanczos(const OpDesc& op, int R, int k, double* Q, double* W, double* norm2, double* alphas, double* betas,
                                 int32_t* steps, double* scratch, hipStream_t st);
// launch_hubbard_block_chebyshev, launch_hubbard_block_moments (docs/design/34-hubbard-chebyshev.md): the twins of
// launch_sector_block_chebyshev and launch_sector_block_moments for an OP_HUBBARD descriptor, on k_cheb_hubbard_block<R, A> and
// k_cheb_hubbard_moments<R, LEFT>, with the same arguments, schedules and return values.
int launch_hubbard_block_chebyshev(const OpDesc& op, int R, int A, int M, double centre, double halfwidth, const double* coeffs,
                                   const double* X, double* U, double* V, double* ACC, hipStream_t st);
int launch_hubbard_block_moments(const OpDesc& op, int R, int M, double centre, double halfwidth, const double* X, const double* Y,
                                 double* U, double* V, double* MU, double* scratch, hipStream_t st);
// dsea_hubbard_current.hip (the bond current map K(w) on the sector of an OP_HUBBARD descriptor,
// docs/design/39-hubbard-current.md): Y = K(w) X for a block fp64 [n, R] row-major, R in {1, 2, 4, 8}, with w = [w_up(nb),
// w_dn(nb)] on the device (column j is the same bits at every R; the callers check R), and the 2 nb forms v1^T K_{s t} v2 into
// out through per-block partials in the caller's scratch (ladder_partials(n, 2 nb) doubles).  The couplings of the descriptor are
// not read.  -1 when the descriptor is out of range.
int launch_hubbard_current(const OpDesc& op, int R, const double* w, const double* X, double* Y, hipStream_t st);
int launch_hubbard_current_forms(const OpDesc& op, const double* v1, const double* v2, double* out, double* scratch, hipStream_t st);
// The column dots (docs/design/40-finite-temperature-conductivity.md): out[j] = sum_r Lft[r, j] (K(w) X)[r, j] through per-block
// partials in the caller's scratch (ladder_partials(n, R) doubles), without the product block; Lft == X is allowed.  0, or -1
// when the descriptor is out of range; the caller has checked R.
int launch_hubbard_current_block_dots(const OpDesc& op, int R, const double* w, const double* Lft, const double* X, double* out,
                                      double* scratch, hipStream_t st);
// dsea_block_lanczos.hip (the basis-free block Lanczos recurrence for any operator; the device parts the block kernels share are
// in dsea_block.h, docs/design/32-block-kernel-parts.md): the start and k steps with the per-column break record on nblk blocks
// of 256 rows, three launches per step, nothing read back.  The mat-vec of a step is the caller's step(q, w, state, first, PA),
// which launches W = H q - w diag(state[0 .. R)) over w (first != 0: W = H q, w is not read) with the partials of q_j . W_j in
// PA[j * nblk + block].  Scratch of block_lanczos_scratch_doubles(n, R) doubles (enough for every grid cap).  Returns 0.
int64_t block_lanczos_scratch_doubles(int64_t n, int R);
typedef std::function<void(const double* q, double* w, const double* state, int first, double* PA)> BlockLanczosStep;
int block_lanczos_drive(int64_t n, int nblk, int R, int k, double* Q, double* W, double* norm2, double* alphas, double* betas,
                        int32_t* steps, double* scratch, hipStream_t st, const BlockLanczosStep& step);
// dsea_cg_persist_tfim_big.hip
bool cg_persist_tfim_big_applicable(const OpDesc& op);
size_t cg_persist_tfim_big_comm_bytes(int64_t n);
int launch_cg_persist_tfim_big(const OpDesc& op, const double* shift, const double* b, double* x, double* state,
                               double eps, int64_t maxiter, void* comm, double* dbuf0, double* dbuf1, hipStream_t st,
                               int lose_peer = 0, bool merged = true);
// dsea_cg_persist_tfim.hip
bool cg_persist_tfim_applicable(const OpDesc& op);
size_t cg_persist_tfim_comm_bytes(int64_t n);
int launch_cg_persist_tfim(const OpDesc& op, const double* shift, const double* b, double* x, double* state, double eps,
                           int64_t maxiter, void* comm, hipStream_t st, int lose_peer = 0);
// dsea_lanczos_persist.hip
bool lanczos_persist_applicable(const OpDesc& op, int64_t n, int k);
size_t lanczos_persist_comm_bytes(int64_t n, int k);
int launch_lanczos_persist(const OpDesc& op, int k, const double* q0, double* Q, int64_t ldq, double* alphas,
                           double* betas, double* brk, double* fail, void* comm, hipStream_t st, int lose_peer = 0);

// dsea_transfer_mfma.hip
bool transfer_mfma_applicable(const OpDesc& op);
int launch_transfer_mfma(const OpDesc& op, const double* x, double* y, hipStream_t st);
void launch_pack_fragments(const double* B, double* Bp, int D, int d, hipStream_t st);
// dsea_lanczos_persist_mid.hip
bool lanczos_persist_mid_applicable(const OpDesc& op, int64_t n, int k);
size_t lanczos_persist_mid_comm_bytes(int64_t n, int k);
int launch_lanczos_persist_mid(const OpDesc& op, int k, const double* q0, double* Q, int64_t ldq, uint16_t* Qs, int64_t lds,
                               double tau, double* alphas, double* betas, double* brk, double* fail, double* lp_count,
                               void* comm, hipStream_t st, int lose_peer = 0);

}  // namespace dsea

// ---- the host layer's one error path (dsea_capi.hip, dsea_partitioned.hip) ----------------------------------------------
#define REQUIRE(cond, code)     \
  do {                          \
    if (!(cond)) return (code); \
  } while (0)
#define DSEA_TRY(call)                \
  do {                                \
    const int rc__ = (call);          \
    if (rc__ != DSEA_OK) return rc__; \
  } while (0)
#define HIP_TRY(call)                                   \
  do {                                                  \
    const hipError_t e__ = (call);                      \
    if (e__ != hipSuccess) return dsea::hip_fail(e__); \
  } while (0)

namespace dsea {
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// records e as this host thread's dsea_last_hip_error() (and clears the runtime's sticky copy); returns DSEA_ERR_HIP
int hip_fail(hipError_t e);
inline int check_launch() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DSEA_OK : hip_fail(e);
}
// dst <- src (device to host) and wait for it
inline int read_to_host(void* dst, const void* src, size_t bytes, hipStream_t st) {
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return DSEA_OK;
}
// The answer of a persistent single-launch launcher: 0 = it ran, -2 = a HIP error (recorded here), anything else = it
// does not apply and the caller goes on with the multi-launch kernels (PERSIST_SKIPPED, not a DSEA status).
constexpr int PERSIST_SKIPPED = 1;
inline int persist_status(int pr) { return pr == -2 ? hip_fail(hipGetLastError()) : pr == 0 ? DSEA_OK : PERSIST_SKIPPED; }
// the operators whose mat-vec kernel also takes the Lanczos step's tail (launch_tfim_fused): both Lanczos entry points
inline bool has_fused_tail(const OpDesc& op) {
  return (op.kind == OP_TFIM && op.tfim.L_local >= 1) || (op.kind == OP_SELL && op.sell.mode == 0) ||
         op.kind == OP_STENCIL3;
}

// Host-side polling of the CG state without draining the stream: the state of chunk j is copied into pinned memory
// behind an event while chunk j + 1 is already enqueued -- the device never waits for the host round trip (the launches
// of a chunk issued after convergence are no-ops on the device: every CG kernel tests the DONE flag).
struct StatePoller {
  double* pinned;        // 2 x DSEA_CG_STATE_LEN doubles of page-locked host memory
  hipEvent_t ev[2];
  bool ok;
};
StatePoller* state_poller();   // per host thread, created on first use, nullptr if the runtime refuses
// The CG polling loop of every driver (dsea_capi.hip).  enqueue(first, count) enqueues iterations [first, first + count)
// (numbered from 0 in this call) and returns a DSEA status.  Chunks of <= poll_every iterations are issued until the
// state copied to hs says DONE or `budget` iterations have been issued; *issued (optional) = how many.
//   sp == nullptr: blocking -- the first chunk is always issued (the caller decides whether to start), the state is read
//                  with a stream synchronisation after every chunk.
//   sp:            pipelined -- the state is snapshot before the first chunk and after each one, and the snapshot of chunk
//                  j is looked at only once chunk j + 1 is enqueued; after convergence at most one chunk of no-ops runs.
int cg_poll(const double* state, double* hs, int64_t budget, int poll_every, StatePoller* sp,
            const std::function<int(int64_t, int64_t)>& enqueue, hipStream_t st, int64_t* issued = nullptr);
// the final host state as a status (DONE < 0: TIMEOUT, DONE != 0: OK, else NOT_CONVERGED) after a check of the launches;
// fills iters_out / resnorm_out (optional)
int cg_result(const double* hs, int64_t* iters_out, double* resnorm_out);
}  // namespace dsea

// the opaque handles of include/dsea.h
struct dsea_op_s {
  dsea::OpDesc d;
};
struct dsea_ws_s {
  dsea::Workspace w;
};
#endif
