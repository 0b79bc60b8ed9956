/*
 * dsea.h -- C ABI of the MI355X-native dominant-eigenpair hot path (libdsea.so).
 *
 * The reference (buwantaiji/DominantSparseEigenAD) is pure Python on torch ops and
 * has no FFI of its own; these entry points are the boundary a maintainer would
 * bind (ctypes stub shown in INTEGRATION.md) to replace, op for op, the torch
 * calls inside the two hot loops:
 *
 *      Lanczos tridiagonalisation      reference DominantSparseEigenAD/Lanczos.py:49-77
 *      Ritz vector                     reference DominantSparseEigenAD/Lanczos.py:98-105
 *      conjugate gradients             reference DominantSparseEigenAD/CG.py:24-41
 *      projections b - (a.b) a         reference CG.py:59,67,122,132 ; symeig.py:27,80
 *      user mat-vec A(v)               reference examples/TFIM/TFIM.py:91-98,
 *                                      examples/schrodinger1D.py:18-27 (+ generic CSR)
 *
 * Conventions
 *   - every function returns an int status: 0 = ok, negative = DSEA_ERR_*; nothing throws;
 *   - all data pointers are DEVICE pointers owned by the caller (PyTorch); the library
 *     allocates no device memory.  The only library-owned objects are the small host-side
 *     handles (dsea_op_t, dsea_ws_t) that carve / describe caller memory;
 *   - vectors are fp64, contiguous, 16-byte aligned (DSEA_ERR_ALIGN otherwise);
 *   - the Krylov basis is stored VECTOR-CONTIGUOUS: vector j starts at Q + j*ldq
 *     (ldq >= n, ldq even).  The reference keeps it (n,k) row-major (Lanczos.py:49);
 *     the host layer hands users the transposed view;
 *   - `stream` is a hipStream_t passed as void*; every function is asynchronous on that
 *     stream unless its comment says it synchronises;
 *   - scalars that feed the next kernel (alpha, beta, CG state) stay on the device: they are
 *     passed as device pointers so that no host round trip sits inside the loops.  In the
 *     row-partitioned multi-GPU mode the caller all-reduces exactly those device scalars
 *     between two phase calls (each phase leaves the LOCAL sum there).
 *   - one workspace per stream; a workspace is not re-entrant; distinct workspaces are
 *     independent.
 */
#ifndef DSEA_H
#define DSEA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSEA_OK 0
#define DSEA_ERR_ARG (-1)       /* null pointer / bad size / bad enum            */
#define DSEA_ERR_ALIGN (-2)     /* pointer not 16-byte aligned or ldq odd        */
#define DSEA_ERR_WORKSPACE (-3) /* workspace too small for (n, k)                */
#define DSEA_ERR_HIP (-4)       /* a HIP runtime call failed (see dsea_last_hip_error) */
#define DSEA_ERR_NOT_CONVERGED (-5) /* dsea_cg_run hit maxiter                   */
#define DSEA_ERR_UNSUPPORTED (-6)
#define DSEA_ERR_TIMEOUT (-8)   /* persistent single-launch solver: a peer workgroup did not arrive (bounded spin) */
#define DSEA_ERR_BREAKDOWN (-7) /* dsea_lanczos_status: the run met beta ~ 0 and stopped itself */

typedef struct dsea_op_s *dsea_op_t; /* operator descriptor (host struct, device pointers inside) */
typedef struct dsea_ws_s *dsea_ws_t; /* workspace descriptor                                     */

int dsea_version(void);
const char *dsea_error_string(int status);
int dsea_last_hip_error(void);

/* ------------------------------------------------------------------ workspace
 * Scratch for partial sums, reorthogonalisation coefficients and four work vectors.
 * dsea_ws_bytes tells the caller how much device memory to provide.  kmax (Krylov vectors the
 * workspace can serve) is capped at 8000: DSEA_ERR_ARG beyond.                                  */
int dsea_ws_bytes(int64_t n, int kmax, size_t *bytes);
int dsea_ws_create(void *device_buffer, size_t bytes, int64_t n, int kmax, dsea_ws_t *out);
int dsea_ws_destroy(dsea_ws_t ws);
/* tuning knob (0 = automatic): rows handled per lane in the basis-streaming kernels {2,4,8,16} */
int dsea_ws_set_rows_per_lane(dsea_ws_t ws, int rpl);
/* tuning knob: small-n "split" form of the basis-streaming kernels -- a block of `waves` waves shares one
 * 128-row tile and splits the basis vectors between its waves.  -1 = automatic (on below ~1.3e5 rows),
 * 0 = off, 4 / 8 / 16 = forced.                                                                          */
int dsea_ws_set_split(dsea_ws_t ws, int waves);
/* Persistent single-launch CG of dsea_cg_run (3-point stencil without halo pointers up to 2^19 rows; full-space matrix-free
 * TFIM at 2^11 ... 2^20 rows): the whole solve is ONE launch.                    design: docs/design/04-kernels.md 3a, 3c, 3e
 *   -1  automatic (on where it applies)          0  off (streaming form: three launches per iteration)
 *   1, 2 / 21, 22 / 11, 12   forced geometry: row pairs per thread in workgroups of 1024 / 512 / 256 threads (stencil)
 *   100 + g   MERGED-REDUCTION form, one grid-wide exchange per iteration (Chronopoulos-Gear recurrences: the same iteration
 *             in exact arithmetic, NOT the rounding sequence of reference CG.py:31-40); never automatic on the stencil
 *   200       TFIM: the TWO-exchange form, iterates bit-identical to the streaming kernels (other operands: as -1)
 * Defaults: stencil -- the reference's recurrences (bit-identical to streaming); TFIM -- the one-exchange form.          */
int dsea_ws_set_persist(dsea_ws_t ws, int mode);
/* which form the LAST dsea_cg_run on this workspace took (a persistent launch that times out is repeated by the caller in
 * the streaming form, whose rounding sequence differs from the one-exchange form's: callers and tests can tell)       */
#define DSEA_CG_FORM_STREAMING 0            /* mat-vec + update + direction launches: CG.py:31-40 in fp64            */
#define DSEA_CG_FORM_PERSISTENT 1           /* one launch, the reference's recurrences (bit-identical to streaming)   */
#define DSEA_CG_FORM_PERSISTENT_MERGED 2    /* one launch, Chronopoulos-Gear recurrences (one exchange per iteration) */
int dsea_cg_last_form(dsea_ws_t ws, int *form);
/* Single-launch Lanczos of dsea_lanczos_run: README-sized problems (TFIM L <= 13, stencil n <= 8192, k <= 512) and the
 * MID-SIZE stencil form (8192 < n <= 131072 rows, k <= 505: BASELINE configs[2]).  Same algorithm and expressions as the
 * multi-launch kernels; partial sums are combined per slab, so T agrees to rounding, not bit for bit.
 *   -1  automatic (on where it is measured to win)    0  off    1  on wherever it applies    2  README-sized form only
 * A lost peer workgroup (bounded spins) makes dsea_lanczos_status return DSEA_ERR_TIMEOUT; the caller repeats the run with
 * the knob off.                                                                  design: docs/design/04-kernels.md 3c, 3d  */
int dsea_ws_set_lanczos_persist(dsea_ws_t ws, int mode);
/* Gram-Schmidt passes per step of dsea_lanczos_run: 1 = the reference (single-pass classical Gram-Schmidt against all
 * previous vectors, Lanczos.py:66), 2 = the pass is repeated on the corrected vector ("CGS2": orthogonality at rounding
 * level even where one pass leaves eps ||u|| / beta) -- an option the reference lacks, never selected automatically. */
int dsea_ws_set_reorth_passes(dsea_ws_t ws, int passes);
/* PARTIAL re-orthogonalisation for dsea_lanczos_run / dsea_pop_lanczos_run (Simon 1984) -- an option the reference lacks
 * (it re-orthogonalises on every step, Lanczos.py:66), never selected automatically.  A step is re-orthogonalised only when
 * the omega recurrence exceeds `delta` (0 = the default 1e-10).  Operators with a fused tail only, multi-launch form, fp64
 * basis; otherwise DSEA_ERR_UNSUPPORTED.  dsea_lanczos_reorth_stats (synchronises): steps re-orthogonalised in the last run
 * and the ||A|| estimate used.                                                  design: docs/design/09-next-rows-f1-f4.md 8.4 */
int dsea_ws_set_partial_reorth(dsea_ws_t ws, int on, double delta);
int dsea_lanczos_reorth_stats(dsea_ws_t ws, int64_t *reorth_steps, double *anorm, void *stream);
/* TEST HOOK for the persistent single-launch forms (Lanczos, TFIM CG): with lose_peer != 0 the last workgroup of such a
 * launch exits at once, so its peers run into their bounded spins -- exercises the DSEA_ERR_TIMEOUT path and the
 * host's fall-back to the multi-launch kernels (a launch then takes the 3 s of the timeout).                      */
int dsea_ws_set_fault_injection(dsea_ws_t ws, int lose_peer);

/* Optional bf16 SHADOW of the Krylov basis (caller-owned, `rows` x `ld` uint16, ld % 8 == 0, 16-byte
 * aligned; null = off).  When registered, dsea_lanczos_run also stores every new basis vector rounded to
 * bf16 and the correction pass  r -= sum_j c_j q_j  (second half of Lanczos.py:66) streams the shadow
 * (2 bytes/element) instead of the fp64 basis.  Arithmetic stays fp64 and the dots pass always reads the
 * fp64 basis.  This is exact to working precision because with full re-orthogonalisation
 * max|c_j| ~ 1e-16..1e-15 ||r|| (the correction lives in the last bit of r); the kernel verifies
 * max|c_j| <= tau ||r|| on the device each step and otherwise reads the fp64 basis.
 * dsea_lanczos_lp_stats (synchronises) reports how many steps of the last run took each path.       */
int dsea_ws_set_shadow(dsea_ws_t ws, void *shadow_bf16, int64_t ld, int rows, double tau);
/* The same with ONE byte per element (caller-owned, `rows` x `ld` uint8, ld % 16 == 0, 16-byte aligned; null = off):
 * code = float8_e5m2(float32(q * S)), S = 2^ceil(log2(n) / 2) (at most 2^15), both roundings to nearest even.  Read by
 * the correction pass of dsea_lanczos_run's multi-launch loop and of dsea_lanczos_axpy_norm from 2^20 rows on (below,
 * and in the single-launch forms, the pass reads the fp64 basis); kept current by dsea_lanczos_run in that regime and by
 * dsea_lanczos_store.  The correction is accumulated in fp32 and applied in one fp64 step; the device-side premise is
 * max|c_j| <= tau8 ||r||.  Registering either shadow un-registers the other: a workspace has at most one.
 * dsea_lanczos_lp_stats counts this pass like the bf16 one.                                                    */
int dsea_ws_set_shadow8(dsea_ws_t ws, void *shadow_e5m2, int64_t ld, int rows, double tau8);
int dsea_lanczos_lp_stats(dsea_ws_t ws, int64_t *lp_steps, int64_t *fp64_steps, void *stream);

/* Per-launch timing of the dominant kernels with HIP events recorded on the launch stream
 * (measurement aid for bench.py's roofline figure; not part of the numerical path).
 * After dsea_profile_begin, dsea_lanczos_run brackets every launch of kind
 *   0 = re-orthogonalisation dots kernel, 1 = re-orthogonalisation axpy kernel, 2 = operator mat-vec
 * with an event pair; dsea_profile_end synchronises and returns launches[3], total_ms[3] (host). */
int dsea_profile_begin(dsea_ws_t ws, int max_records);
int dsea_profile_end(dsea_ws_t ws, int64_t *launches, double *total_ms);

/* ------------------------------------------------------------------ operators
 * An operator is y = A x on a slab of n_local rows.                                   */

/* Transverse-field Ising chain, matrix-free (replaces the gather-table mat-vec of
 * reference examples/TFIM/TFIM.py:39-51,91-98):
 *     y[i] = diag_scale * d(gi) * x[i]  -  g * sum_{j < L_local} x[i ^ (1<<j)],
 *     gi = row_offset + i,  d(gi) = -(L - 2*popcount(gi ^ rotl_L(gi,1))).
 * g is read from the device pointer g_dev when it is non-null (the parameter tensor of the
 * model, TFIM.py / E0.py:95-96), otherwise g_const is used.  diag_scale = 0, g_const = 1 gives
 * dH/dg of TFIM.py:58-65.  Flips of bits >= L_local (row-partitioned runs) are the caller's
 * exchange step.  n_local = 2^L_local.                                                        */
int dsea_op_create_tfim(int L, int L_local, int64_t row_offset, const double *g_dev, double g_const,
                        double diag_scale, dsea_op_t *out);

/* XYZ spin chain with per-site couplings, matrix-free (docs/design/14-spin-chain.md): periodic chain of L sites, site i =
 * bit i of the row index s, z_i(s) = 1 - 2 bit_i(s), bond b joins sites b and (b+1) mod L, m_b = its two bits:
 *     H = sum_b [ Jx_b X_b X_b+1 + Jy_b Y_b Y_b+1 + Jz_b Z_b Z_b+1 ] + sum_i [ hx_i X_i + hz_i Z_i ]
 *     y[s] = ( sum_b Jz_b z_b z_b+1 + sum_i hz_i z_i ) x[s] + sum_i hx_i x[s ^ (1<<i)] + sum_b ( Jx_b - Jy_b z_b z_b+1 ) x[s ^ m_b]
 * couplings_dev: fp64 (5, L) row-major on the device, rows Jx, Jy, Jz, hx, hz; READ THROUGH THE POINTER ON EVERY LAUNCH (no
 * host copy: in-place updates are seen).  2 <= L <= 62 and a non-null pointer are checked before any device work; nothing is
 * launched at creation.  L = 2: bonds 0 and 1 join the same two sites and both count; an open chain is J_{L-1} = 0.
 * n = 2^L.  dsea_op_set_tuning DSEA_TUNE_TFIM_TILE_LOG2 applies.  No fused Lanczos tail, no persistent forms. */
int dsea_op_create_chain(int L, const double *couplings_dev, dsea_op_t *out);
/* The parameter adjoint of dsea_op_create_chain: out5L[t] = v1^T (dH/dp_t) v2 for all 5 L couplings in the order of
 * couplings_dev, in one pass over v1 and v2 (per-block partials in `scratch`, then a fixed-order reduction: no atomics,
 * repeated calls return identical bits).  `scratch`: caller-owned, dsea_op_chain_forms_scratch_doubles(L) doubles (enough
 * for every tile tuning); the library allocates nothing.  v1, v2 16-byte aligned.  DSEA_ERR_ARG for any other operator kind. */
int dsea_op_chain_forms_scratch_doubles(int L, int64_t *out);
int dsea_op_chain_forms(dsea_op_t op, const double *v1, const double *v2, double *out5L, double *scratch, void *stream);

#define DSEA_LATTICE_MAX_BONDS 128 /* most bonds of dsea_op_create_lattice (a 4 x 6 J1-J2 torus has 96, K16 has 120) */
/* XYZ spins on a caller-given bond list, matrix-free (docs/design/16-spin-lattice.md): L sites, site i = bit i of the row
 * index s, z_i(s) = 1 - 2 bit_i(s); bond t joins sites a_t != b_t (bonds_host[2t], bonds_host[2t+1], a HOST array that is
 * copied at creation), m_t = (1<<a_t)|(1<<b_t):
 *     H = sum_t [ Jx_t X_a X_b + Jy_t Y_a Y_b + Jz_t Z_a Z_b ] + sum_i [ hx_i X_i + hz_i Z_i ]
 *     y[s] = ( sum_t Jz_t z_a z_b + sum_i hz_i z_i ) x[s] + sum_i hx_i x[s ^ (1<<i)] + sum_t ( Jx_t - Jy_t z_a z_b ) x[s ^ m_t]
 * (a, b) and (b, a) are the same bond; a repeated bond counts each time it is listed.
 * couplings_dev: fp64 [3 nb + 2 L] on the device in the order Jx(nb), Jy(nb), Jz(nb), hx(L), hz(L); READ THROUGH THE POINTER
 * ON EVERY LAUNCH (no host copy: in-place updates are seen).  Checked on the host before any device work (DSEA_ERR_ARG):
 * 2 <= L <= 62, 1 <= nb <= DSEA_LATTICE_MAX_BONDS, 0 <= a_t, b_t < L, a_t != b_t, non-null pointers.  Nothing is launched and
 * nothing is allocated on the device at creation.  n = 2^L.  dsea_op_set_tuning DSEA_TUNE_TFIM_TILE_LOG2 applies.  No fused
 * Lanczos tail, no persistent forms. */
int dsea_op_create_lattice(int L, int nb, const int32_t *bonds_host, const double *couplings_dev, dsea_op_t *out);
/* The parameter adjoint of dsea_op_create_lattice: out[t] = v1^T (dH/dp_t) v2 for all 3 nb + 2 L couplings in the order of
 * couplings_dev, in one pass over v1 and v2 (per-block partials in `scratch`, then a fixed-order reduction: no atomics,
 * repeated calls return identical bits).  `scratch`: caller-owned, dsea_op_lattice_forms_scratch_doubles(L, nb) =
 * (3 nb + 2 L) * min(4096, 2^max(L-6, 0)) doubles (enough for every tile tuning); the library allocates nothing.  v1, v2
 * 16-byte aligned.  DSEA_ERR_ARG for any other operator kind. */
int dsea_op_lattice_forms_scratch_doubles(int L, int nb, int64_t *out);
int dsea_op_lattice_forms(dsea_op_t op, const double *v1, const double *v2, double *out, double *scratch, void *stream);

/* XXZ spins on a caller-given bond list in ONE MAGNETISATION SECTOR, matrix-free (docs/design/18-spin-sector.md): the sites,
 * bits and bonds of dsea_op_create_lattice,
 *     H = sum_t [ Jxy_t (X_a X_b + Y_a Y_b) + Jz_t Z_a Z_b ] + sum_i hz_i Z_i
 * restricted to the states with exactly ndown set bits.  Row r is the r-th such state IN INCREASING INTEGER ORDER, s_r;
 * n = C(L, ndown):
 *     y[r] = ( sum_t Jz_t z_a z_b + sum_i hz_i z_i ) x[r] + sum_{t : bit_a(s_r) != bit_b(s_r)} 2 Jxy_t x[rank(s_r ^ m_t)]
 *     rank(s) = hi_base[s >> Llo] + lo_rank[s & (2^Llo - 1)],   Llo = (L + 1) / 2,  Lhi = L - Llo
 * dsea_sector_table_sizes: n, n_lo = 2^Llo, n_hi = 2^Lhi.  Host arithmetic only.  DSEA_ERR_ARG outside 2 <= L <= 40,
 * 1 <= ndown <= L - 1, n <= 2^31 - 1 (ranks are 32-bit), and for a null pointer. */
int dsea_sector_table_sizes(int L, int ndown, int64_t *n, int64_t *n_lo, int64_t *n_hi);
/* Fills the caller's three device tables on `stream` (deterministic; once per (L, ndown), the tables hold no couplings):
 * states int64 [n] = s_r (combinatorial unranking, one row per thread); lo_rank int32 [n_lo]: the rank of p among the Llo-bit
 * words of its popcount; hi_base int32 [n_hi]: the number of sector states below h << Llo, 0 for an h no sector state has.
 * The library allocates nothing. */
int dsea_sector_build_tables(int L, int ndown, int64_t *states, int32_t *lo_rank, int32_t *hi_base, void *stream);
/* The operator on filled tables (caller-owned, alive as long as the handle; several handles may share one set).
 * bonds_host: as dsea_op_create_lattice, copied at creation.  couplings_dev: fp64 [2 nb + L] on the device in the order
 * Jxy(nb), Jz(nb), hz(L); READ THROUGH THE POINTER ON EVERY LAUNCH (in-place updates are seen).  Checked on the host before any
 * device work (DSEA_ERR_ARG): the limits of dsea_sector_table_sizes, 1 <= nb <= DSEA_LATTICE_MAX_BONDS, 0 <= a_t, b_t < L,
 * a_t != b_t, non-null pointers.  Nothing is launched or allocated at creation.  For this kind dsea_op_set_tuning
 * DSEA_TUNE_TFIM_TILE_LOG2 = log2 of the most blocks a launch uses (6..12, default 12; beyond the cap blocks walk ranges of
 * 256 rows).  No fused Lanczos tail, no persistent forms, no row-partitioned slabs. */
int dsea_op_create_sector(int L, int ndown, int nb, const int32_t *bonds_host, const double *couplings_dev,
                          const int64_t *states, const int32_t *lo_rank, const int32_t *hi_base, dsea_op_t *out);
/* The parameter adjoint of dsea_op_create_sector: out[t] = v1^T (dH/dp_t) v2 for all 2 nb + L couplings in the order of
 * couplings_dev, in one pass over v1 and v2 (per-block partials in `scratch`, then a fixed-order reduction: no atomics,
 * repeated calls return identical bits).  `scratch`: caller-owned, dsea_op_sector_forms_scratch_doubles(L, ndown, nb) =
 * (2 nb + L) * min(4096, ceil(n / 256)) doubles (enough for every grid cap); the library allocates nothing.  DSEA_ERR_ARG for
 * any other operator kind. */
int dsea_op_sector_forms_scratch_doubles(int L, int ndown, int nb, int64_t *out);
int dsea_op_sector_forms(dsea_op_t op, const double *v1, const double *v2, double *out, double *scratch, void *stream);

/* XXZ spins with a coupling on EVERY PAIR OF SITES in one magnetisation sector, matrix-free (docs/design/22-pair-sector.md):
 *     H = sum_{i<j} [ Jxy_ij (X_i X_j + Y_i Y_j) + Jz_ij Z_i Z_j ] + sum_i hz_i Z_i
 * on the rows, bits and tables of dsea_op_create_sector (dsea_sector_table_sizes / dsea_sector_build_tables; several handles
 * of either kind may share one set).  The pairs are implicit, P = L (L - 1) / 2 of them in lexicographic order (0,1), (0,2),
 * ..., (0,L-1), (1,2), ...: p(i, j) = i (2 L - i - 1) / 2 + (j - i - 1); no bond list and no 128-bond cap.  couplings_dev: fp64
 * [2 P + L] on the device in the order Jxy(P), Jz(P), hz(L); READ THROUGH THE POINTER ON EVERY LAUNCH (in-place updates are
 * seen).  Checked on the host before any device work (DSEA_ERR_ARG): the limits of dsea_sector_table_sizes, non-null
 * pointers.  Nothing is launched or allocated at creation.  DSEA_TUNE_TFIM_TILE_LOG2 as for dsea_op_create_sector.  No fused
 * Lanczos tail, no persistent forms, no row-partitioned slabs. */
int dsea_op_create_pairsector(int L, int ndown, const double *couplings_dev, const int64_t *states, const int32_t *lo_rank,
                              const int32_t *hi_base, dsea_op_t *out);
/* The parameter adjoint of dsea_op_create_pairsector: out[t] = v1^T (dH/dp_t) v2 for all 2 P + L couplings in the order of
 * couplings_dev.  With v1 = v2 = psi these are the two-point correlation matrices <X_i X_j + Y_i Y_j>, <Z_i Z_j> and <Z_i> of
 * psi.  The xy forms come from one pass of gathers, the zz and z forms from a Gram product over the rows on the fp64 matrix
 * cores; partials in `scratch`, then fixed-order reductions: no atomics, repeated calls return identical bits.  `scratch`:
 * caller-owned, dsea_op_pairsector_forms_scratch_doubles(L, ndown) = P min(4096, ceil(n / 256)) + 4 (P + L) min(256,
 * ceil(n / 256)) doubles (enough for every grid cap); the library allocates nothing.  DSEA_ERR_ARG for any other operator
 * kind. */
int dsea_op_pairsector_forms_scratch_doubles(int L, int ndown, int64_t *out);
int dsea_op_pairsector_forms(dsea_op_t op, const double *v1, const double *v2, double *out, double *scratch, void *stream);

/* THE HUBBARD MODEL of spinful fermions on a caller-given bond list at fixed particle numbers (nup, ndn), matrix-free
 * (docs/design/19-hubbard.md): the sites and bonds of dsea_op_create_lattice,
 *     H = sum_t [ -t_t sum_s (c+_{a s} c_{b s} + h.c.) + V_t n_a n_b ] + sum_i U_i n_{i up} n_{i dn} + sum_i eps_i n_i
 * Bit i of the word u is the occupation of (i, up), bit i of d that of (i, dn);
 * |u, d> = (prod_{i in u, ascending} c+_{i up}) (prod_{j in d, ascending} c+_{j dn}) |0>.  Row r = ru * n_dn + rd (down
 * fastest), ru the rank of u among the L-bit words of nup set bits IN INCREASING INTEGER ORDER, rd likewise for d.  With
 * m_t = (1 << a_t) | (1 << b_t) and sgn_t(w) = (-1)^(number of set bits of w strictly between a_t and b_t):
 *     y[r] = diag(u, d) x[r] - sum_{t : bit_a(u) != bit_b(u)} t_t sgn_t(u) x[rank_u(u ^ m_t) n_dn + rd]
 *                            - sum_{t : bit_a(d) != bit_b(d)} t_t sgn_t(d) x[ru n_dn + rank_d(d ^ m_t)]
 *     diag(u, d) = sum_i U_i bit_i(u) bit_i(d) + sum_i eps_i (bit_i(u) + bit_i(d)) + sum_t V_t n_a n_b
 * dsea_hubbard_sizes: n = n_up n_dn, n_up = C(L, nup), n_dn = C(L, ndn).  Host arithmetic only.  DSEA_ERR_ARG outside
 * 2 <= L <= 40, 1 <= nup <= L - 1, 1 <= ndn <= L - 1, n <= 2^31 - 1 (rows are 32-bit), and for a null pointer. */
int dsea_hubbard_sizes(int L, int nup, int ndn, int64_t *n, int64_t *n_up, int64_t *n_dn);
/* The operator on filled tables (caller-owned, alive as long as the handle; several handles may share them).  Each triple
 * (states, lo_rank, hi_base) is what dsea_sector_table_sizes / dsea_sector_build_tables give at (L, nup) and at (L, ndn); the
 * two triples may be the same pointers when nup == ndn.  bonds_host: as dsea_op_create_lattice, copied at creation.
 * couplings_dev: fp64 [2 nb + 2 L] on the device in the order t(nb), V(nb), U(L), eps(L); READ THROUGH THE POINTER ON EVERY
 * LAUNCH (in-place updates are seen).  Checked on the host before any device work (DSEA_ERR_ARG): the limits of
 * dsea_hubbard_sizes, 1 <= nb <= DSEA_LATTICE_MAX_BONDS, 0 <= a_t, b_t < L, a_t != b_t, non-null pointers.  Nothing is
 * launched or allocated at creation.  For this kind dsea_op_set_tuning DSEA_TUNE_TFIM_TILE_LOG2 = log2 of the most blocks a
 * launch uses (6..12, default 12; beyond the cap blocks walk ranges of 256 rows).  No fused Lanczos tail, no persistent
 * forms, no row-partitioned slabs. */
int dsea_op_create_hubbard(int L, int nup, int ndn, int nb, const int32_t *bonds_host, const double *couplings_dev,
                           const int64_t *up_states, const int32_t *up_lo_rank, const int32_t *up_hi_base,
                           const int64_t *dn_states, const int32_t *dn_lo_rank, const int32_t *dn_hi_base, dsea_op_t *out);
/* The parameter adjoint of dsea_op_create_hubbard: out[p] = v1^T (dH/dp) v2 for all 2 nb + 2 L couplings in the order of
 * couplings_dev, in one pass over v1 and v2 (per-block partials in `scratch`, then a fixed-order reduction: no atomics,
 * repeated calls return identical bits).  `scratch`: caller-owned, dsea_op_hubbard_forms_scratch_doubles(L, nup, ndn, nb) =
 * (2 nb + 2 L) * min(4096, ceil(n / 256)) doubles (enough for every grid cap); the library allocates nothing.  DSEA_ERR_ARG
 * for any other operator kind. */
int dsea_op_hubbard_forms_scratch_doubles(int L, int nup, int ndn, int nb, int64_t *out);
int dsea_op_hubbard_forms(dsea_op_t op, const double *v1, const double *v2, double *out, double *scratch, void *stream);

/* XXZ spins of dsea_op_create_sector reduced further by a LATTICE-SYMMETRY GROUP G with a real one-dimensional character chi,
 * matrix-free (docs/design/20-symmetry-sector.md).  g in G is a permutation of the sites: g(s) has bit perm_g[i] set iff s has
 * bit i; chi(g) = +1 or -1.  rep(s) = min_g g(s); sigma(s) = sum_{g : g(s) = s} chi(g) (|Stab(s)| or 0).  Row r is the r-th
 * representative with sigma != 0 IN INCREASING INTEGER ORDER; basis vector |r> = (|G| sigma_r)^(-1/2) sum_g chi(g) |g s_r>.  With
 * pbar the couplings averaged over their orbits under G (bond orbits for Jxy and Jz, site orbits for hz; ascending index order):
 *     y[r] = ( sum_t Jzbar_t z_a z_b + sum_i hzbar_i z_i ) x[r]
 *          + sum_{t : bit_a(s_r) != bit_b(s_r)} 2 Jxybar_t chi(g*) sqrt(sigma_j / sigma_r) x[j]
 * g* attains min_g g(s_r ^ m_t), j is the row of that minimum; the term is dropped when the minimum is no stored row.
 * dsea_symsector_sizes: n_sector = C(L, ndown), n_bucket = 2^Lhi + 1 (Lhi = L - (L + 1) / 2), n_perm = ng ceil(L / 8) 256.
 * Host arithmetic only.  DSEA_ERR_ARG outside the limits of dsea_sector_table_sizes, outside 1 <= ng <=
 * DSEA_SYMSECTOR_MAX_GROUP, and for a null pointer. */
#define DSEA_SYMSECTOR_MAX_GROUP 128 /* most group elements (the space group of the 4 x 4 torus has 128) */
int dsea_symsector_sizes(int L, int ndown, int ng, int64_t *n_sector, int64_t *n_bucket, int64_t *n_perm);
/* perm_tab int64 [n_perm] on the device, filled on `stream`: entry (g, slice, byte) = the image under g of the state whose byte
 * `slice` is `byte` and whose other bits are 0, so g(s) is the OR of ceil(L / 8) entries.  perms_host: int32 [ng * L],
 * perms_host[g * L + i] = the site that g sends site i to; DSEA_ERR_ARG unless every row is a permutation of 0 .. L - 1. */
int dsea_symsector_fill_perm(int L, int ng, const int32_t *perms_host, int64_t *perm_tab, void *stream);
/* Rows [first, first + count) of the full sector (unranked in the kernel): slab[i] = s | sigma << 48 when the state s of row
 * first + i is the smallest of its orbit and sigma != 0, and 0 otherwise.  chars_host: int32 [ng], +1 or -1.  slab: int64
 * [count] on the device.  The non-zero entries of all slabs in order are the table `reps`. */
int dsea_symsector_classify(int L, int ndown, int ng, const int32_t *chars_host, const int64_t *perm_tab, int64_t first,
                            int64_t count, int64_t *slab, void *stream);
/* bucket int32 [n_bucket] on the device: bucket[h] = the first row whose state >> Llo is >= h, Llo = (L + 1) / 2. */
int dsea_symsector_fill_buckets(int L, int64_t n_rep, const int64_t *reps, int32_t *bucket, void *stream);
/* The operator on filled tables (caller-owned, alive as long as the handle; several handles may share one set); n = n_rep rows.
 * bonds_host, couplings_dev: as dsea_op_create_sector (READ THROUGH THE POINTER ON EVERY LAUNCH).  orbits_host: int32
 * [2 nb + L], the orbit id of every parameter (equal ids inside one family = one orbit), 0 <= id < 2 nb + L.  Checked on the
 * host before any device work (DSEA_ERR_ARG): the limits of dsea_symsector_sizes, 1 <= n_rep <= n_sector, the bond rules of
 * dsea_op_create_sector, chars of +-1, orbit ids in range, non-null pointers.  Nothing is launched or allocated at creation.
 * DSEA_TUNE_TFIM_TILE_LOG2 = log2 of the most blocks a launch uses (6..12, default 12; a block takes 16 rows at a time and
 * walks beyond the cap).  No fused Lanczos tail, no persistent forms, no row-partitioned slabs. */
int dsea_op_create_symsector(int L, int ndown, int nb, const int32_t *bonds_host, const double *couplings_dev, int ng,
                             const int32_t *chars_host, const int32_t *orbits_host, int64_t n_rep, const int64_t *reps,
                             const int32_t *bucket, const int64_t *perm_tab, dsea_op_t *out);
/* The parameter adjoint of dsea_op_create_symsector: out = S raw, raw[t] = v1^T A_t v2 with A_t the coefficient matrix of
 * pbar_t in the row formula and S the orbit mean, for all 2 nb + L couplings in one pass (per-block partials in `scratch`, then
 * a fixed-order reduction over the members of each orbit: no atomics, repeated calls return identical bits, the members of an
 * orbit receive identical bits).  `scratch`: caller-owned, dsea_op_symsector_forms_scratch_doubles(n_rep, L, nb) =
 * (2 nb + L) * min(4096, ceil(n_rep / 8)) doubles (enough for every grid cap).  DSEA_ERR_ARG for any other operator kind. */
int dsea_op_symsector_forms_scratch_doubles(int64_t n_rep, int L, int nb, int64_t *out);
int dsea_op_symsector_forms(dsea_op_t op, const double *v1, const double *v2, double *out, double *scratch, void *stream);
/* Spin inversion: a group element may also flip every spin, g(s) = perm_g(s) ^ (flip_g ? 2^L - 1 : 0); composition multiplies
 * the characters and XORs the flips.  rep, sigma, the row order, |r> and the dropped hops are defined as above with this g.
 * flips_host: int32 [ng], 0 or 1.  perm_tab keeps its meaning (the permutation alone); dsea_symsector_sizes, _fill_perm and
 * _fill_buckets serve both kinds.  Jxy and Jz enter through their orbit means as before; hz through the SIGNED mean
 *     hzbar_i = eps_i * mean_{j in the site orbit of i} (eps_j hz_j)
 * site_signs_host: int32 [L], eps_i in {+1, -1, 0}: 0 on an orbit one of whose sites is fixed by a flipped element, otherwise
 * the relative sign sgn(g) = -1 (flipped) / +1 of the elements that carry the orbit's first site to i.
 * dsea_symsector_classify_flip: as dsea_symsector_classify with the flipped images.
 * dsea_op_create_symsector_flip: as dsea_op_create_symsector; dsea_op_symsector_forms works on its handles (the hz outputs of an
 * orbit are then identical up to the sign bit for bit, and exactly 0.0 where eps = 0).  Further host checks (DSEA_ERR_ARG, before
 * any device work): flips of 0 or 1, a set flip only with 2 ndown = L, signs in {-1, 0, +1}. */
int dsea_symsector_classify_flip(int L, int ndown, int ng, const int32_t *chars_host, const int32_t *flips_host,
                                 const int64_t *perm_tab, int64_t first, int64_t count, int64_t *slab, void *stream);
int dsea_op_create_symsector_flip(int L, int ndown, int nb, const int32_t *bonds_host, const double *couplings_dev, int ng,
                                  const int32_t *chars_host, const int32_t *flips_host, const int32_t *site_signs_host,
                                  const int32_t *orbits_host, int64_t n_rep, const int64_t *reps, const int32_t *bucket,
                                  const int64_t *perm_tab, dsea_op_t *out);

/* CSR, caller-owned device arrays: rowptr int64 [n+1], colidx int32 [nnz], vals fp64 [nnz]. */
int dsea_op_create_csr(int64_t n, int64_t nnz, const int64_t *rowptr, const int32_t *colidx,
                       const double *vals, dsea_op_t *out);

/* Sliced ELLPACK with slices of 64 rows (SELL-64), caller-owned device arrays: slice_ptr int64 [nslices+1]
 * (element offsets), and per slice s, column-major blocks: entry k of row 64 s + l at slice_ptr[s] + 64 k + l,
 * padded per slice to its longest row with (colidx = any valid column, vals = 0).  nslices = ceil(n/64).
 * This is the layout the CSR operand of the host layer is converted to: coalesced matrix loads.           */
int dsea_op_create_sell(int64_t n, int64_t nslices, const int64_t *slice_ptr, const int32_t *colidx,
                        const double *vals, dsea_op_t *out);

/* The same layout with 16-BIT COLUMN DELTAS: the column of element e is colbase[e / 64] + coldelta[e] -- one int32 base per
 * 64-element slice column (the smallest column index in it) and a uint16 per element, 10.06 instead of 12 bytes per
 * non-zero.  Valid when every slice column spans fewer than 65536 columns (banded / structured patterns: the 21-nnz/row
 * TFIM matrix does; the host layer checks and falls back to dsea_op_create_sell).  The SELL mat-vec sits on the bytes it
 * moves (docs/design/12-round6.md): fewer bytes is the one lever it has.  colbase: int32 [slice_ptr[nslices] / 64].       */
int dsea_op_create_sell16(int64_t n, int64_t nslices, const int64_t *slice_ptr, const int32_t *colbase,
                          const uint16_t *coldelta, const double *vals, dsea_op_t *out);

/* dsea_op_create_sell16 with the per-element arrays PACKED TWO slice columns to a lane: every slice is padded to an EVEN
 * number of slice columns (slice_ptr counts the padded elements, multiples of 128) and element (slice column 2 G + j, lane l)
 * of the slice starting at slice_ptr[s] sits at slice_ptr[s] + 128 G + 2 l + j of vals[] and coldelta[]; colbase as before.
 * A lane then reads its two values as one 16-byte load and its two deltas as one uint32 -- 4 instead of 6 memory
 * instructions per two non-zeros of a row (beside the matrix stream the kernel sits on the CU's per-lane load rate,
 * docs/design/12-round6.md section 12.9).  Same products in the same order; everything dsea_op_create_sell16 supports
 * (dsea_op_update_vals, dsea_op_sddmm, dsea_op_set_slab) works on it.                                                        */
int dsea_op_create_sell16p2(int64_t n, int64_t nslices, const int64_t *slice_ptr, const int32_t *colbase,
                            const uint16_t *coldelta, const double *vals, dsea_op_t *out);

/* VALUE-CODED SELL-64 for operands whose stored entries take few distinct values (lattice Hamiltonians held as explicit
 * matrices: couplings, fields and a handful of diagonal levels -- the 21-nnz/row TFIM matrix at L = 20 has 11): the value of an
 * element is table256[code], a uint8 per element into 256 doubles (unused entries: anything finite; padding elements code a
 * 0.0), columns as in dsea_op_create_sell16 -- 3.06 instead of 10.06 bytes per non-zero.  The products are formed with the
 * SAME doubles in the same order: the result is bit-identical to dsea_op_create_sell16 on the decoded values.
 * Layout: every slice is padded to a MULTIPLE OF FOUR slice columns (slice_ptr counts the padded elements, multiples of
 * 256), colbase has one entry per slice column as before (a column that is all padding: any valid column), and the two
 * per-element arrays are packed four slice columns to a lane: element (slice column 4 G + j, lane l) of the slice starting
 * at slice_ptr[s] sits at slice_ptr[s] + 256 G + 4 l + j of code[] and coldelta[] -- a lane reads its four codes as one
 * uint32 and its four deltas as one 8-byte word (with 3 bytes per non-zero the kernel sits on the CU's per-lane load rate,
 * not on the fabric: docs/design/12-round6.md).  The table is copied into LDS by every workgroup.
 * Such an operand is READ-ONLY: dsea_op_update_vals and dsea_op_set_slab answer DSEA_ERR_UNSUPPORTED (the host layer
 * re-codes in place, or rebuilds the fp64 layout once the values stop fitting 256 codes); dsea_op_sddmm works.        */
int dsea_op_create_sell16v8(int64_t n, int64_t nslices, const int64_t *slice_ptr, const int32_t *colbase,
                            const uint16_t *coldelta, const uint8_t *code, const double *table256, dsea_op_t *out);

/* 3-point stencil + diagonal (reference examples/schrodinger1D.py:18-27):
 *     y[i] = coef * ((-2 x[i] + x[i+1]) + x[i-1]) + V[i] * x[i],  x[-1] = *halo_lo, x[n] = *halo_hi
 * (null halo pointer = 0, the Dirichlet padding of the reference).                            */
int dsea_op_create_stencil3(int64_t n, double coef, const double *V_dev, const double *halo_lo,
                            const double *halo_hi, dsea_op_t *out);

/* per-operator tuning knobs (measurement aid; nothing process-wide): key DSEA_TUNE_TFIM_TILE_LOG2 = log2 rows of
 * x staged in LDS per block of the TFIM mat-vec (6..12, default 11); DSEA_TUNE_CSR_GROUP = lanes per CSR row
 * (0 = automatic, or 4..64)                                                                                */
#define DSEA_TUNE_TFIM_TILE_LOG2 1
#define DSEA_TUNE_CSR_GROUP 2
/* SELL mat-vec (32-bit columns): slice columns requested per lane before the first gather {0 = automatic (4), 2, 4, 8};
 * 1 = the round-5 kernel kept as the "before" arm of tools/kbench_csr.py                                       */
#define DSEA_TUNE_SELL_UNROLL 3
/* SELL mat-vec: 1 = XCD-contiguous slice map (workgroup b works on eighth b % 8 of the slices), 0 = round-robin (default) */
#define DSEA_TUNE_SELL_XCD_MAP 4
/* SELL mat-vec with 16-bit columns (dsea_op_create_sell16 only; DSEA_ERR_UNSUPPORTED on the packed / value-coded layouts):
 * 1 = non-temporal loads of the matrix stream (values, column deltas), 0 = default policy */
#define DSEA_TUNE_SELL_NT 5
/* SELL operand: a HINT that no slice is wider than `value` slice columns (0 = unknown).  dsea_op_sddmm and dsea_op_update_vals
 * stage a slice's CSR segment in LDS; knowing the widest one they reserve that much instead of 16 KB per wave and more
 * workgroups fit a CU (both are latency-bound).  A wrong hint costs speed, not correctness. */
#define DSEA_TUNE_SELL_MAX_WIDTH 6
int dsea_op_set_tuning(dsea_op_t op, int key, int value);

/* The explicit-matrix operand as a PARAMETER of the primitives.  The reference's contract is that the adjoint of the
 * operator, A-bar = v1 v2^T, is pushed to whatever parameters produced A (reference README.md:88-126, symeig.py:56-64,
 * 82-84; its dense primitive returns exactly that outer product, symeig.py:29).  For a sparse A whose parameters ARE
 * its stored non-zeros the push-forward is the sampled outer product  vals-bar[e] = v1[row(e)] * v2[col(e)].
 * Both calls address the caller's CSR arrays: `rowptr` (int64 [n+1], the array the operator was built from; ignored
 * for a dsea_op_create_csr operand, which has its own) maps entry k of row i of the SELL copy to CSR element
 * rowptr[i] + k -- the order the host layer's conversion keeps.
 *
 * dsea_op_update_vals: the operator's values become vals_csr[0..nnz).  SELL: its value array (caller-owned, handed to
 *     dsea_op_create_sell) is REWRITTEN IN PLACE through that map, padding stays 0; no rebuild of the layout.  CSR: a
 *     device copy into the operator's array unless vals_csr already is that array.
 * dsea_op_sddmm: out[e] = alpha * v1[row(e)] * v2[col(e)]            (flags = 0)
 *     DSEA_SDDMM_ACCUMULATE : out[e] += ...
 *     DSEA_SDDMM_SYMMETRIC  : alpha * (v1[row] v2[col] + v1[col] v2[row]) / 2 -- the adjoint w.r.t. the entries of a matrix
 *                             that is applied as (M + M^T)/2, i.e. of a symmetric operand whose pairs (i,j), (j,i) move together
 *     out: CSR order, nnz doubles.  Deterministic (one writer per element).
 *     On a slab operator (dsea_op_set_slab) v2[col] is read where the mat-vec reads x[col]: the caller has exchanged v2's
 *     halo / gathered copy; DSEA_SDDMM_SYMMETRIC is DSEA_ERR_UNSUPPORTED there (dsea_pop_sddmm does both exchanges).     */
#define DSEA_SDDMM_ACCUMULATE 1
#define DSEA_SDDMM_SYMMETRIC 2
int dsea_op_update_vals(dsea_op_t op, const int64_t *rowptr, const double *vals_csr, void *stream);
int dsea_op_sddmm(dsea_op_t op, const int64_t *rowptr, const double *v1, const double *v2, double alpha, int flags,
                  double *out, void *stream);

/* GEMM-shaped operands of the NON-symmetric primitives (reference eig.py) -- the one place on this path where a matrix core
 * is the right unit.                                                            design: docs/design/09-next-rows-f1-f4.md 8.1
 *   dense   : row-major n x n matrix (eig.py:28-30, DominantEig); transpose != 0 applies A^T.  Hand-written row-streaming
 *             GEMV (HBM-bound); callers that apply A^T repeatedly hand in the transposed matrix.
 *   transfer: MPS transfer matrix of a rank-3 tensor A (d x D x D row-major), dimension D^2, vectors are D x D row-major
 *             (reference examples/TFIM_vumps/general.py:59-66):
 *                 transpose == 0:  y = sum_s A_s x A_s^T        ("Gong",  general.py:59-61)
 *                 transpose != 0:  y = sum_s A_s^T x A_s        ("GongT", general.py:62-64)
 *             Two hand-written fp64 MFMA kernels (csrc/dsea_transfer_mfma.hip; any D, zero-padded to a multiple of 64 inside)
 *             up to D = 768, two rocBLAS GEMMs beyond (bound at run time from the copy already in the process; absent: the
 *             hand-written pair at every size).  DSEA_TRANSFER_MFMA=1 / =0 forces one or the other.
 *             `work`: caller-owned scratch of dsea_op_transfer_work_bytes(D, d); dsea_op_create_transfer fills part of it on
 *             `stream`.  THE TENSOR IS CAPTURED AT CREATION: the hand-written kernels read the fragment-packed copy made
 *             then, the rocBLAS path reads A_dev itself -- A_dev must stay unchanged for the life of the operator, and an
 *             updated tensor needs a new operator.                                                                       */
int dsea_op_create_dense(int64_t n, const double *A_dev, int64_t lda, int transpose, dsea_op_t *out);
/* dense SYMMETRIC operand (reference symeig.py:15-31 DominantSymeig; Lanczos.py:46-49 applies torch.matmul(A, v)):
 * hand-written mat-vec that reads only the UPPER triangle of the row-major matrix -- every 64 x 64 tile is loaded
 * once and used for both its row block and its column block (half the bytes of a GEMV; deterministic, no atomics).
 * The matrix may be fp64 (elem_bytes = 8) or fp32 (elem_bytes = 4: the reference's dense path follows A.dtype,
 * Lanczos.py:47) -- fp32 elements are widened on load, vectors and arithmetic stay fp64, no promoted copy is made.
 * `work`: caller-owned scratch of dsea_op_symdense_work_bytes(n) (per-tile partial results, n^2/8 bytes).  lda even. */
size_t dsea_op_symdense_work_bytes(int64_t n);
int dsea_op_create_symdense(int64_t n, const void *A_dev, int elem_bytes, int64_t lda, double *work, dsea_op_t *out);
size_t dsea_op_transfer_work_bytes(int D, int d);
int dsea_op_create_transfer(int D, int d, const double *A_dev, int transpose, double *work, void *stream,
                            dsea_op_t *out);

/* A SELL operator as the SLAB of a row-partitioned matrix (SURVEY.md 8e "CSR-banded: halo"; no reference counterpart -- the
 * reference is single-device): the operator holds n consecutive rows of a larger matrix and says where x[col] lives when
 * col is not one of its own rows.
 *   halo_width = hb >= 0 : column indices are LOCAL, in [-hb, n + hb): c < 0 reads halo_lo[c + hb] (the last hb elements of the
 *                          previous slab), c >= n reads halo_hi[c - n] (the first hb of the next slab).  A banded matrix
 *                          with half-bandwidth <= hb <= n: one pairwise exchange of hb elements with each neighbour per mat-vec.
 *                          A missing neighbour's pointer may be null (no column points there).
 *   halo_width = -1      : column indices are GLOBAL and x[col] is read from x_gathered (all slabs, rank-major): the
 *                          mat-vec is preceded by an all-gather of x -- the fallback for patterns without a band.
 * The row operand of dsea_spmv (x, y) stays the slab.  dsea_pop_create_csr wraps such an operator with the exchange. */
int dsea_op_set_slab(dsea_op_t op, int64_t halo_width, double *halo_lo, double *halo_hi, double *x_gathered);

int dsea_op_destroy(dsea_op_t op);
int dsea_op_dim(dsea_op_t op, int64_t *n);

/* y = A x - (*shift) x  (shift may be null);  if dot_out != null: *dot_out = x.y (local sum).
 * The Amap(v) of Lanczos.py:54,71 and CG.py:27,31,34,40 (with q.u of Lanczos.py:55,72 / d.Ad of CG.py:31 through dot_out).
 * If skip_flag != null and *skip_flag != 0 the call is a no-op on the device (converged CG). */
int dsea_spmv(dsea_op_t op, dsea_ws_t ws, const double *x, double *y, const double *shift,
              double *dot_out, const double *skip_flag, void *stream);

/* ------------------------------------------------------------------ vector phases (Lanczos)
 * Used one by one in the generic-callable and the multi-GPU modes, and composed by
 * dsea_lanczos_run.                                                                       */

/* out = x.y   (torch.matmul(q, u) of Lanczos.py:55,72 ; the inner products of CG.py:31,37) */
int dsea_dot(dsea_ws_t ws, const double *x, const double *y, int64_t n, double *out, void *stream);

/* y -= (*shift) * x ; *dot_out = x.y      (generic A: turns A(d) into (A - E0) d, CG.py:120)   */
int dsea_shift_dot(dsea_ws_t ws, const double *x, double *y, const double *shift, double *dot_out,
                   const double *skip_flag, int64_t n, void *stream);

/* y += (a_host * (*a_dev)) * x   (a_dev may be null = 1)       (x + alpha d of CG.py:33 for a caller-composed loop) */
int dsea_axpy(dsea_ws_t ws, double a_host, const double *a_dev, const double *x, double *y,
              int64_t n, void *stream);

/* nrm2_out = ||x||^2 (local)   (torch.norm of Lanczos.py:53,69 and CG.py:28,35, before its square root) */
int dsea_nrm2sq(dsea_ws_t ws, const double *x, int64_t n, double *nrm2_out, void *stream);

/* Measurement probe, not part of the path (bench.py "measured_ceilings"; SURVEY.md 8d asks for the box's own streaming
 * ceiling beside the 8 TB/s spec figure): y == NULL streams x[0..n) once through a read-only reduction (per-block sums
 * land in the workspace's partials), otherwise copies x to y; 8 non-temporal 16-byte loads in flight per lane. */
int dsea_probe_stream(dsea_ws_t ws, const double *x, double *y, int64_t n, void *stream);

/* q_out = r / sqrt(*nrm2) ; if beta_out != null: *beta_out = sqrt(*nrm2)   (Lanczos.py:53,69-70,75) */
int dsea_scale_store(dsea_ws_t ws, const double *r, const double *nrm2, double *q_out,
                     double *beta_out, int64_t n, void *stream);

/* Phase 1 of step i (1 <= i < k), Lanczos.py:61 and the first half of :66:
 *     r = u - (*alpha) Q[i-1] - (*beta) Q[i-2]        (beta may be null: 0, the i = 1 case)
 *     c_out[j] = Q[j] . r   for j < i ;  c_out[i] = r . r     (local sums; c_out holds i+1 doubles)   */
int dsea_lanczos_rdots(dsea_ws_t ws, const double *Q, int64_t ldq, int64_t n, int i,
                       const double *u, const double *alpha, const double *beta, double *r,
                       double *c_out, void *stream);

/* Phase 2, second half of Lanczos.py:66 and :69:  r -= sum_j c[j] Q[j] ; *nrm2_out = ||r||^2 (local).
 * If a bf16 shadow of this basis is registered (dsea_ws_set_shadow, rows kept current by dsea_lanczos_store)
 * the pass streams the shadow, subject to the device-side premise max|c_j| <= tau*sqrt(c[i]).            */
int dsea_lanczos_axpy_norm(dsea_ws_t ws, const double *Q, int64_t ldq, int64_t n, int i,
                           const double *c, double *r, double *nrm2_out, void *stream);

/* Phases 1 + 2 of step i under the PARTIAL re-orthogonalisation option (dsea_ws_set_partial_reorth's scheme as a phase call
 * for a caller-supplied mat-vec): r = u - alphas[i-1] Q[i-1] - betas[i-2] Q[i-2]; the omega estimates advance from
 * alphas[0..i-1], betas[0..i-2] (device arrays, as dsea_dot / dsea_lanczos_store leave them) and ||r||; if they ask for it
 * -- decided on the device, no host synchronisation -- r -= Q Q^T r; *nrm2_out = ||r||^2.  i = 1 starts a new run.
 * dsea_lanczos_reorth_stats reports the count.  fp64 basis (a registered bf16 shadow is not used).                  */
int dsea_lanczos_partial_step(dsea_ws_t ws, const double *Q, int64_t ldq, int64_t n, int i, const double *u,
                              const double *alphas, const double *betas, double *r, double *nrm2_out, void *stream);

/* Q[row] = r / sqrt(*nrm2) (and the bf16 shadow row if registered) ; *beta_out = sqrt(*nrm2) (nullable)
 * (Lanczos.py:53,69-70,75 writing into the vector-contiguous basis)                                       */
int dsea_lanczos_store(dsea_ws_t ws, const double *r, const double *nrm2, double *Q, int64_t ldq, int row,
                       double *beta_out, int64_t n, void *stream);

/* One Lanczos step around a CALLER-SUPPLIED mat-vec (reference Lanczos.py:60-75 with Amap a Python function -- the reference's
 * own calling convention, examples/TFIM/E0.py:59-62), as TWO calls per step instead of five phase calls:
 *     dsea_lanczos_callable_alpha(ws, Q[i-1], u, n, NULL)      u = A Q[i-1] is the caller's: leaves the partial sums of
 *                                                              alpha_{i-1} = Q[i-1].u in the workspace (one launch)
 *     dsea_lanczos_callable_step(ws, Q, ldq, n, i, u, alphas, betas, r)
 *          r = u - alpha_{i-1} Q[i-1] - beta_{i-2} Q[i-2] ; c = Q^T r ; r -= Q c ; beta_{i-1} = ||r|| ; Q[i] = r / beta_{i-1}
 *          (and the bf16 shadow row if one is registered); alphas[i-1], betas[i-1] are stored.  Four launches: the two scalar
 *          reductions (alpha, ||r||^2) are summed in the prologues of their consumers, as in dsea_lanczos_run's step.
 * The last alpha has no consumer: pass alpha_out = alphas + (k-1) to the last dsea_lanczos_callable_alpha to have it summed.
 * Always full re-orthogonalisation in one pass (the workspace's partial / CGS2 options apply to dsea_lanczos_run; around a
 * caller's mat-vec they are composed from the phase calls).                                                              */
int dsea_lanczos_callable_alpha(dsea_ws_t ws, const double *q, const double *u, int64_t n, double *alpha_out, void *stream);
int dsea_lanczos_callable_step(dsea_ws_t ws, double *Q, int64_t ldq, int64_t n, int i, const double *u, double *alphas,
                               double *betas, double *r, void *stream);

/* out = sum_{j<k} s[j] Q[j]   (the one needed column of Qk @ eigvecs, Lanczos.py:99-105)      */
int dsea_ritz_combine(dsea_ws_t ws, const double *Q, int64_t ldq, int64_t n, int k,
                      const double *s, double *out, void *stream);

/* out = v - (a.v) a   (CG.py:59,67,122,132 ; symeig.py:27,80); `a_dot_v` (nullable) receives a.v */
int dsea_project_out(dsea_ws_t ws, const double *v, const double *a, double *out, double *a_dot_v,
                     int64_t n, void *stream);

/* ------------------------------------------------------------------ CG phases (CG.py:24-41)
 * state = 8 device doubles: [0] rr  [1] dAd  [2] rr_new  [3] alpha  [4] beta  [5] resnorm
 *                           [6] done (0/1)  [7] iterations                                   */
#define DSEA_CG_RR 0
#define DSEA_CG_DAD 1
#define DSEA_CG_RRNEW 2
#define DSEA_CG_ALPHA 3
#define DSEA_CG_BETA 4
#define DSEA_CG_RESNORM 5
#define DSEA_CG_DONE 6
#define DSEA_CG_ITERS 7
#define DSEA_CG_STATE_LEN 8

/* r = b - Ax0 ; d = r ; state[RR] = r.r (local) ; clears the rest of state               (CG.py:27,30) */
int dsea_cg_init(dsea_ws_t ws, const double *b, const double *Ax0, double *r, double *d,
                 double *state, int64_t n, void *stream);
/* after the caller has made state[RR] global: done = sqrt(rr) < eps                       (CG.py:28-29) */
int dsea_cg_init_check(dsea_ws_t ws, double *state, double eps, void *stream);
/* alpha = rr/dAd ; x += alpha d ; r -= alpha Ad ; state[RRNEW] = r.r (local)              (CG.py:31,33-34) */
int dsea_cg_update(dsea_ws_t ws, double *x, double *r, const double *d, const double *Ad,
                   double *state, int64_t n, void *stream);
/* after state[RRNEW] is global: iterations += 1 ; resnorm = sqrt(rr_new) ; done |= resnorm < eps ;
 * beta = rr_new/rr ; rr = rr_new                                                          (CG.py:35-38) */
int dsea_cg_check(dsea_ws_t ws, double *state, double eps, void *stream);
/* d = r + beta d   (no-op when done)                                                       (CG.py:39) */
int dsea_cg_direction(dsea_ws_t ws, const double *r, double *d, const double *state, int64_t n,
                      void *stream);

/* ONE iteration of CG around a CALLER-SUPPLIED mat-vec (reference CG.py:31-40 with Amap = the user's Python function, the
 * reference's own calling convention): on entry Ad = A d.  Ad -= (*shift) d (shift nullable); alpha = rr / d.Ad;
 * x += alpha d; r -= alpha Ad; the stopping test on ||r||; beta; d = r + beta d -- the three fused launches dsea_cg_run issues
 * per iteration of its streaming form (same kernels, same partial-sum order: bit-identical iterates), in one call instead of
 * dsea_shift_dot + dsea_cg_update + dsea_cg_check + dsea_cg_direction.  `iteration` = 0, 1, 2, ... since dsea_cg_init /
 * dsea_cg_init_check (it selects which of the two rr slots of `state` is current).  No-op on the device once DONE is set. */
int dsea_cg_step(dsea_ws_t ws, double *x, double *r, double *d, double *Ad, const double *shift, double *state, double eps,
                 int64_t iteration, int64_t n, void *stream);

/* ------------------------------------------------------------------ row-partitioned macro phases
 * One Lanczos step of the row-partitioned mode (no reference counterpart) is
 *     dsea_plz_dots            -> caller all-reduces c[0..i]   (i coefficients + ||r||^2)
 *     dsea_plz_correct_matvec  -> caller exchanges r with the partner slabs
 *     dsea_axpy_multi_dot      -> caller all-reduces pair[0..1] = (||r||^2, r.Ar)
 *     dsea_plz_finish
 * i.e. two latency-bound all-reduces and one slab exchange per step.  The mat-vec is applied to the
 * un-normalised r (linearity): beta = sqrt(pair[0]), alpha = pair[1]/pair[0], q = r/beta, u = (A r)/beta.   */

/* r = u - (*alpha) Q[i-1] - (*beta) Q[i-2] (Lanczos.py:61) as a stand-alone pass; r_copy (nullable) receives a
 * second copy -- the snapshot an overlapped slab exchange sends while r is corrected in place.            */
int dsea_lanczos_form_r(dsea_ws_t ws, const double *Q, int64_t ldq, int64_t n, int i, const double *u,
                        const double *alpha, const double *beta, double *r, double *r_copy, void *stream);

/* Top-bit flips of the row-partitioned TFIM mat-vec in TRANSPOSED form (P = 2^p ranks, P >= 4): the caller
 * all-to-alls its slab (chunk c of every rank's slab goes to rank c), calls this on the received buffer
 * xT[P][chunk]:  zT[s][m] = sum_{b<p} xT[s ^ (1<<b)][m],  and all-to-alls zT back (zT[s] to rank s).  Every
 * link then carries 1/P of a slab per phase instead of a whole slab per partner.  (The flips of the top p bits in the
 * gather-table mat-vec of examples/TFIM/TFIM.py:39-51.)                                                   */
int dsea_hypercube_flipsum(const double *xT, double *zT, int P, int64_t chunk, void *stream);

/* r = u - (*alpha) Q[i-1] - (*beta) Q[i-2] ; c_out[j] = Q[j].r (j < i) ; c_out[i] = r.r   (local sums)
 * (Lanczos.py:61 and the inner product of :66, on a slab)                                                 */
int dsea_plz_dots(dsea_ws_t ws, const double *Q, int64_t ldq, int64_t n, int i, const double *u,
                  const double *alpha, const double *beta, double *r, double *c_out, void *stream);
/* row >= 1: r -= sum_{j<row} c[j] Q[j] (bf16 shadow if registered and the premise holds) ; pair_out[0] = ||r||^2
 * (local).  row == 0: only pair_out[0] = r.r.          (the outer product of Lanczos.py:66 and the norm of :69, on a slab) */
int dsea_plz_correct(dsea_ws_t ws, const double *Q, int64_t ldq, int64_t n, int row, const double *c,
                     double *r, double *pair_out, void *stream);
/* the same followed by y = A_local r (Lanczos.py:71 applied to the un-normalised r; operators whose remote part is ADDED after the local one, e.g. TFIM;
 * halo-type operators call dsea_plz_correct, exchange the halo, then dsea_spmv)                            */
int dsea_plz_correct_matvec(dsea_op_t op, dsea_ws_t ws, const double *Q, int64_t ldq, int row,
                            const double *c, double *r, double *y, double *pair_out, void *stream);
/* y += a_host*(*a_dev) * (xs[0] + ... + xs[count-1]) - (*shift) x ; *dot_out = x.y (local).  count <= 6,
 * a_dev / shift / skip_flag nullable.  (remote part of the TFIM mat-vec: a = -g, xs = partner slabs -- the flips of
 * examples/TFIM/TFIM.py:39-51 whose partner row lives on another rank; the dot is Lanczos.py:72 / CG.py:31)   */
int dsea_axpy_multi_dot(dsea_ws_t ws, double a_host, const double *a_dev, const double *const *xs, int count,
                        const double *shift, const double *skip_flag, const double *x, double *y, int64_t n,
                        double *dot_out, void *stream);
/* pair = global (||r||^2, r.Ar): q_out = r/beta (row `row` of the basis; also its bf16 shadow row if registered),
 * u_out = y/beta, *alpha_out = pair[1]/pair[0], *beta_out = beta (nullable)            (Lanczos.py:69-70,72-75) */
int dsea_plz_finish(dsea_ws_t ws, const double *r, const double *y, const double *pair, double *q_out, int row,
                    double *u_out, double *alpha_out, double *beta_out, int64_t n, void *stream);

/* ------------------------------------------------------------------ row-partitioned solvers with the collectives
 * INSIDE the library ("multi-GPU variants taking ncclComm_t / rank / world").
 * No reference counterpart (the reference is single-device).  One process per GPU; every n-vector is this rank's
 * slab of contiguous rows.  The library issues its slab kernels and the RCCL calls back to back on the caller's
 * stream -- no host language between two phases of a step, no host synchronisation inside the Lanczos loop.
 *
 * Communicator.  Two RCCL communicators per rank: one carries the latency-bound all-reduces of the inner products on
 * the solver's stream, the other the bandwidth-bound slab exchange of the mat-vec on a side stream (RCCL orders the
 * operations of ONE communicator even across streams, which would serialise the exchange with the all-reduces it is
 * meant to hide behind).  Either adopt communicators that already exist (ncclComm_t values, e.g. the ones PyTorch's
 * ProcessGroupNCCL holds: torch exposes them) or let the library create its own from two unique ids that the caller
 * distributes (128 bytes each, produced on rank 0).  RCCL is bound at run time from the copy already in the process
 * (DSEA_ERR_UNSUPPORTED if there is none); environment DSEA_RCCL_LIB=<path> binds THAT library instead (RTLD_LOCAL) -- how
 * the tests run this branch with several ranks on one GPU over a stand-in (tests/fake_rccl; docs/design/11-round5.md).  For transports other than RCCL (MPI, gloo in the tests) the caller
 * supplies three blocking callbacks instead; they receive DEVICE pointers and the stream the data was produced on.   */
typedef struct dsea_comm_s *dsea_comm_t;
#define DSEA_COMM_ID_BYTES 128
#define DSEA_ERR_COMM (-9)     /* an RCCL call (or a caller-supplied collective) failed                        */
#define DSEA_ERR_PREMISE (-10) /* overlapped exchange: the premise max|c_j| <= tau ||r|| failed at some step -- results of
                                  this run must be discarded and the run repeated without overlap (identical decision
                                  on every rank: c is replicated)                                               */
int dsea_comm_unique_id(void *id_out /* DSEA_COMM_ID_BYTES */);
int dsea_comm_init_rank(const void *id_coll, const void *id_xchg, int rank, int world, dsea_comm_t *out);
/* adopt existing ncclComm_t values (xchg_comm may equal coll_comm or be null: then exchange and all-reduces share one
 * communicator and are ordered by RCCL); the library never destroys adopted communicators                        */
int dsea_comm_adopt(void *coll_comm, void *xchg_comm, int rank, int world, dsea_comm_t *out);
typedef int (*dsea_allreduce_fn)(void *user, double *buf, int64_t count, void *stream);           /* in-place sum     */
typedef int (*dsea_alltoall_fn)(void *user, const double *send, double *recv, int64_t chunk, void *stream);
typedef int (*dsea_sendrecv_fn)(void *user, const double *send, double *recv, int64_t count, int peer, void *stream);
int dsea_comm_create_callbacks(int rank, int world, dsea_allreduce_fn allreduce, dsea_alltoall_fn alltoall,
                               dsea_sendrecv_fn sendrecv, void *user, dsea_comm_t *out);
int dsea_comm_destroy(dsea_comm_t comm);
/* the collectives themselves, as the solvers issue them (tests, user-side inner products) */
int dsea_comm_allreduce(dsea_comm_t comm, double *buf, int64_t count, void *stream);
int dsea_comm_alltoall(dsea_comm_t comm, const double *send, double *recv, int64_t chunk, void *stream);
/* recv[r * count .. (r+1) * count) = rank r's send[0..count): RCCL -- one group of point-to-point operations on the exchange
 * communicator; callbacks -- world rounds of the pairwise sendrecv callback (round s pairs rank r with (s - r) mod world) */
int dsea_comm_allgather(dsea_comm_t comm, const double *send, double *recv, int64_t count, void *stream);

/* Row-partitioned operator = slab-local operator + communicator + exchange scratch.
 *   tfim     : chain of L sites over world = 2^p ranks, this rank holds rows [rank 2^(L-p), (rank+1) 2^(L-p)).  Low-bit
 *              flips are slab-local (dsea_op_create_tfim with L_local = L - p); the top p bits come from the partner
 *              slabs rank ^ (1<<b): pairwise exchange (p whole slabs) for world = 2, TRANSPOSED form from world = 4 on
 *              (all-to-all, dsea_hypercube_flipsum, all-to-all back: 2 (P-1)/P slabs spread over all links).
 *              `scratch`: caller-owned, dsea_pop_tfim_scratch_doubles(L, world) doubles.  `side_stream` (nullable):
 *              stream for the exchange; with it the exchange runs behind the slab-local work of the step.
 *              flags: DSEA_POP_OVERLAP -- in the Lanczos step the exchange is started on the UN-corrected r before the
 *              dots pass (r - r' = Q c is at the 1e-14 level while |c_j| <~ 1e-15 ||r||); the premise
 *              max|c_j| <= tau ||r|| is checked ON THE DEVICE every step and recorded: dsea_pop_lanczos_status reports
 *              DSEA_ERR_PREMISE after the run instead of a host round trip per step.  In the CG solve the vector is
 *              final when the mat-vec starts, so the side-stream exchange is exact there.
 *              DSEA_POP_PAIRWISE forces the pairwise form at any world size.
 *   stencil3 : dsea_op_create_stencil3 semantics on contiguous slabs; halo2 = two device doubles the exchange fills
 *              (x[-1] from rank-1, x[n] from rank+1; a missing neighbour is the Dirichlet zero).                    */
typedef struct dsea_pop_s *dsea_pop_t;
#define DSEA_POP_OVERLAP 1
#define DSEA_POP_PAIRWISE 2
/* MEASUREMENT ONLY: the slab exchange is not issued and the receive buffers are used as they are -- the numbers are
 * meaningless, the time is that of the same step without its exchange (bench.py: exposed exchange = step - this)  */
#define DSEA_POP_NO_EXCHANGE 4
/* dsea_pop_cg_run: which recurrences.  Default: TFIM -- ONE all-reduce per iteration (Chronopoulos-Gear: r.r and r.A'r
 * reduced together, A'p carried by a recurrence; the same iteration in exact arithmetic, not CG.py:31-40's rounding
 * sequence; what the one-GPU single-launch solver does by default, dsea_ws_set_persist); stencil3 -- the reference's
 * recurrences, two all-reduces per iteration.  The flags force one or the other.                                   */
#define DSEA_POP_CG_REFERENCE 8
#define DSEA_POP_CG_ONE_REDUCTION 16
size_t dsea_pop_tfim_scratch_doubles(int L, int world);
int dsea_pop_create_tfim(int L, dsea_comm_t comm, const double *g_dev, double g_const, double diag_scale,
                         double *scratch, void *side_stream, int flags, double tau, dsea_pop_t *out);
int dsea_pop_create_stencil3(int64_t n_local, double coef, const double *V_dev, double *halo2, dsea_comm_t comm,
                             dsea_pop_t *out);
/*   csr      : explicit sparse matrix in contiguous row slabs of the SAME n_local rows on every rank (the host layer pads
 *              the last slab with empty rows): `local_op` is this rank's SELL operator with its slab description
 *              (dsea_op_set_slab) -- neighbour halo of hb elements per side, or the all-gather fallback.  The pop borrows
 *              local_op's arrays and exchange buffers (the caller keeps them alive) and SNAPSHOTS its descriptor: values
 *              refreshed through dsea_op_update_vals(local_op, ...) are seen (same arrays), a later dsea_op_set_tuning /
 *              dsea_op_set_slab on local_op is not.  Halo-type operator: the exchange
 *              precedes the slab mat-vec (as for stencil3).                                                          */
int dsea_pop_create_csr(dsea_op_t local_op, dsea_comm_t comm, dsea_pop_t *out);
/* the adjoint hook of a row-partitioned explicit matrix (dsea_op_sddmm on slabs): out[e] (+)= alpha v1[row e] v2[col e] for this
 * rank's rows; v2 (and v1 for DSEA_SDDMM_SYMMETRIC) is exchanged like the x of a mat-vec.  rowptr: this slab's CSR row
 * pointers (local element offsets), out: this slab's non-zeros in CSR order.                                          */
int dsea_pop_sddmm(dsea_pop_t pop, const int64_t *rowptr, const double *v1, const double *v2, double alpha, int flags,
                   double *out, void *stream);
int dsea_pop_destroy(dsea_pop_t pop);
int dsea_pop_set_flags(dsea_pop_t pop, int flags);
/* y = (A - (*shift)) x over all ranks (Amap of Lanczos.py:54,71 / CG.py:27,31 and A(v) - E0 v of CG.py:120); if dot_out != null: *dot_out = GLOBAL x.y (all-reduced, identical on every
 * rank); skip_flag as in dsea_spmv.                                                                              */
int dsea_pop_matvec(dsea_pop_t pop, dsea_ws_t ws, const double *x, double *y, const double *shift, double *dot_out,
                    const double *skip_flag, void *stream);
/* out = GLOBAL x.y   (the inner products of Lanczos.py:55,72 and CG.py:31,37 across ranks) */
int dsea_pop_dot(dsea_pop_t pop, dsea_ws_t ws, const double *x, const double *y, int64_t n, double *out, void *stream);
/* k-step Lanczos with full re-orthogonalisation on slabs (reference Lanczos.py:49-77 distributed): per step the
 * macro phases above with TWO all-reduces (coefficients + ||r||^2 ; ||r||^2, r.Ar) and ONE exchange, all issued by
 * the library on `stream` / the side stream.  alphas[k], betas[max(k-1,1)] are replicated bit-identically.  A bf16
 * shadow registered on the workspace is used and kept current.  No host synchronisation inside.                  */
int dsea_pop_lanczos_run(dsea_pop_t pop, dsea_ws_t ws, int k, const double *q0, double *Q, int64_t ldq,
                         double *alphas, double *betas, void *stream);
/* SYNCHRONISES: DSEA_OK, or DSEA_ERR_PREMISE with *step = first step whose overlap premise failed                 */
int dsea_pop_lanczos_status(dsea_pop_t pop, dsea_ws_t ws, int *step, void *stream);
/* CG on (A - (*shift)) x = b on slabs (reference CG.py:24-41 distributed): per iteration one exchange and two scalar
 * all-reduces (reference recurrences) or ONE (DSEA_POP_CG_* above); the stopping test runs on the device on replicated
 * scalars, the host polls every `poll_every` iterations.  SYNCHRONISES before returning.  Work vectors: the workspace's.
 * The one-reduction form carries r AND A'p by recurrences, so its stop is only ACCEPTED after r = b - A'x has been recomputed
 * from x and found below eps (one extra mat-vec + all-reduce per solve); otherwise the recurrences restart from the true
 * residual, and after three such restarts the solve is finished on the reference's recurrences.  resnorm_out then is the
 * TRUE residual norm ||b - A'x||; iters_out counts the iterations of all rounds.                                          */
int dsea_pop_cg_run(dsea_pop_t pop, dsea_ws_t ws, const double *shift, const double *b, double *x, double *state,
                    double eps, int64_t maxiter, int poll_every, int64_t *iters_out, double *resnorm_out, void *stream);

/* ------------------------------------------------------------------ whole solvers (native operator, one GPU)
 * k-step Lanczos with full re-orthogonalisation, entirely on the stream, no host sync.
 *   q0      : start vector (need not be normalised; Lanczos.py:52-53)
 *   Q       : k x ldq basis (output), alphas[k], betas[max(k-1,1)] (outputs, device)            */
int dsea_lanczos_run(dsea_op_t op, dsea_ws_t ws, int k, const double *q0, double *Q, int64_t ldq,
                     double *alphas, double *betas, void *stream);
/* BASIS-FREE Lanczos (an option the reference lacks; it stores all k vectors -- 8 n k bytes, 429 GB at n = 2^28,
 * k = 200 -- and re-orthogonalises against them, Lanczos.py:49,66): the plain three-term recurrence with three
 * rotating vectors Qrot (3 x ldq, caller-owned), NO re-orthogonalisation.  Call once with s = psi = NULL for the
 * tridiagonal (alphas[k], betas[k-1]); after the host has the Ritz coefficients s[k] (device), call again with the
 * same q0: the recurrence is replayed bit-identically and psi = sum_j s[j] q_j is accumulated on the way.  Without
 * re-orthogonalisation converged Ritz values reappear as copies ("ghosts"); the EXTREME eigenpair -- the one the
 * primitives want -- and its residual beta_k |s_k| are unaffected, psi must be normalised by the caller.
 * Operators with a fused Lanczos tail only (matrix-free TFIM, SELL, 3-point stencil).                        */
int dsea_lanczos_run_basisfree(dsea_op_t op, dsea_ws_t ws, int k, const double *q0, double *Qrot, int64_t ldq,
                               double *alphas, double *betas, const double *s, double *psi, void *stream);
/* Breakdown (the reference has no test: Lanczos.py:69-70 divides by beta whatever it is): the run compares every
 * beta_{i-1} ON THE DEVICE with 1e-13 * max_j(|alpha_j|, |beta_j|); at the first one below it records step i,
 * leaves Q[i..], alphas[i..], betas[i..] untouched and turns its remaining launches into no-ops.  This call
 * SYNCHRONISES the stream and returns DSEA_OK, or DSEA_ERR_BREAKDOWN with *break_step = i: the Krylov space of q0
 * has dimension i and the leading i x i block of T holds exact eigenpairs of the operator; DSEA_ERR_TIMEOUT if the
 * single-launch form (dsea_ws_set_lanczos_persist) lost a peer workgroup -- the outputs are then undefined.       */
int dsea_lanczos_status(dsea_ws_t ws, int *break_step, void *stream);

/* ------------------------------------------------------------------ non-symmetric Krylov loops (row f-1)
 * What reference eig.py:29-30,116-117 (ARPACK eigs) and :54-57,137-144 (gmres) do inside SciPy on the host.
 *
 * dsea_arnoldi_extend: Arnoldi factorisation (A - (*shift) I) V_m = V_{m+1} H extended from column j0 to j1
 * (exclusive), entirely on the stream, no host sync:  V = rows of a (>= j1+1) x ldv buffer with V[0..j0] given
 * (orthonormal), H column-major with leading dimension ldh >= j1+1 (columns j0..j1-1 are written in full: h_0..h_j
 * by classical Gram-Schmidt against ALL previous vectors -- so a restarted, non-Hessenberg start block is fine --
 * and h_{j+1,j} = ||w||).  A second Gram-Schmidt pass runs only when the DGKS test asks for it, decided on the
 * device.  An invariant subspace (||w|| <= 1e-13 ||A v_j||) is recorded; dsea_lanczos_status reports the step.  */
int dsea_arnoldi_extend(dsea_op_t op, dsea_ws_t ws, const double *shift, double *V, int64_t ldv, int j0, int j1,
                        double *H, int ldh, void *stream);

/* diagnostics (synchronises): how many steps needed the second Gram-Schmidt pass since the last START of a factorisation:
 * dsea_arnoldi_extend with j0 == 0, dsea_arnoldi_orth with j == 0 and dsea_gmres_begin (so every GMRES cycle) clear the
 * count.  In the optimistic mode a step that fails the test is counted when it is repeated with the pass, not before.  */
int dsea_arnoldi_second_passes(dsea_ws_t ws, int64_t *count, void *stream);

/* OPTIMISTIC second pass (round 4; off by default).  The second Gram-Schmidt pass of dsea_arnoldi_extend is needed rarely
 * (0 of 200 steps on BASELINE configs[3]'s transfer matrix) but its three launches and the two scalar kernels around
 * them are enqueued on every step -- 11 launches, 5 of them returning at once.  With the option on, a step is 6 launches:
 * the DGKS test runs inside the finish kernel, and a step that FAILS it is not finished -- it records itself, every later
 * launch of the run is a no-op, and dsea_arnoldi_status returns DSEA_ERR_SECOND_PASS with *redo_step = that step (the
 * record is cleared by the call).  The caller then repeats the step with the option off -- dsea_arnoldi_extend(..., j, j + 1,
 * ...) -- and continues from j + 1.  Columns of H and vectors of V are bit-identical to the default mode either way.
 * dsea_arnoldi_status SYNCHRONISES: DSEA_OK, DSEA_ERR_BREAKDOWN (*break_step = invariant subspace reached at that step)
 * or DSEA_ERR_SECOND_PASS.  Without the option it reports what dsea_lanczos_status reports for an Arnoldi run.
 * dsea_gmres_cycle / dsea_gmres_step (native operand) honour the option too: a step that fails the test ends the CYCLE
 * early with the columns it has -- a restart, always valid -- and sets state[5] = 1; the caller runs the following
 * cycle(s) with the option off.                                                                                      */
#define DSEA_ERR_SECOND_PASS (-11)
int dsea_ws_set_arnoldi_optimistic(dsea_ws_t ws, int on);
int dsea_arnoldi_status(dsea_ws_t ws, int *break_step, int *redo_step, void *stream);
/* the same record WITHOUT synchronising: enqueues a copy of it into host_record[0] (caller-owned, preferably pinned) on
 * `stream`; the caller waits for its own event and reads: 0 = fine so far, > 0 = invariant subspace at that step, < 0 = step
 * -value - 1 needs its second pass (then dsea_arnoldi_status clears the record as above).  Lets a caller test the stage it
 * has just enqueued while the NEXT stage is already running (krylov.arnoldi_dominant).                                  */
int dsea_arnoldi_status_enqueue(dsea_ws_t ws, double *host_record, void *stream);
/* enqueue (no synchronisation) a clear of the record behind everything issued so far: a caller that stops at a converged
 * stage while a SPECULATIVE stage is still in flight leaves this behind it, so that whatever that stage records (a breakdown,
 * a second-pass request) cannot turn a later continuation (j0 > 0) on the same workspace into no-ops                     */
int dsea_arnoldi_clear_record(dsea_ws_t ws, void *stream);

/* the orthogonalisation of ONE Arnoldi step (one step of what eig.py:29-30,116-117 runs inside ARPACK and :54,57,140,144
 * inside scipy's gmres) when the mat-vec is the caller's code: u = A v_j given, writes column j
 * of H (entries 0..j+1) and V[j+1]; (*shift) v_j is subtracted from u inside the first pass.                    */
int dsea_arnoldi_orth(dsea_ws_t ws, const double *u, const double *shift, double *V, int64_t ldv, int64_t n, int j,
                      double *H, int ldh, void *stream);

/* dsea_gmres_cycle: ONE cycle of restarted GMRES(m) for (A - (*shift) I) x = b (m <= 64): residual, m Arnoldi steps,
 * Givens rotations, back-substitution and the update x += V y -- all on the stream, no host sync inside.  `first`
 * != 0: x is taken as 0 (r0 = b).  `target` = absolute residual bound max(rtol ||b||, atol) (scipy's rule,
 * eig.py:54).  work: dsea_gmres_work_doubles(m) device doubles; V: (m+1) x ldv, zero-initialised once by the caller.
 * state (8 device doubles): [0] residual estimate  [1] converged  [2] columns used  [3] ||r0||  [4] finished early
 * (converged, Krylov space exhausted, or one of the next two)  [5] optimistic mode: a step needed the second pass
 * [6] SINGULAR: (A - shift I) v_j lay in span(V[0..j]) and the rotated column j has an exactly zero diagonal -- no
 * progress is possible from this start.  Column j is not counted ([2] stays j), [1] is NOT set, x receives the update of
 * the j columns before it (none for j = 0: x unchanged) and stays finite.  A caller must not restart on [6]: the next
 * cycle would meet the same column (krylov.gmres raises).
 * The caller reads `state` after the cycle (its one sync) and issues the next cycle if [1] == 0 and [6] == 0.
 * Layout of `work` (ldh = m + 1), readable after a cycle:
 *   H  (m+1) x m column-major at work[0]          column j at work + j*ldh: after the Givens update the upper triangle
 *                                                 R of the rotated H, exact zeros below the diagonal
 *   cs[m] at work + (m+1)*m, sn[m] behind it      the rotations (cs[j], sn[j]) that annihilate h[j+1][j]
 *   g[m+1] behind sn                              the rotated right-hand side; |g[k]| is the residual after k columns
 *   y[m] behind g                                 written by dsea_gmres_end: R y = g over the state[2] columns used,
 *                                                 y[t >= state[2]] = 0                                                  */
size_t dsea_gmres_work_doubles(int m);
/* the three stages of a cycle (the gmres calls of eig.py:54,57,140,144), for operands whose mat-vec is the caller's code
 * (op == NULL, u = A v_j supplied per step; Ax = (A - shift) x supplied to begin, NULL for x = 0); dsea_gmres_cycle
 * composes them for native operators.  dsea_gmres_step repeats the checks of dsea_gmres_begin that concern it: the
 * workspace was created with kmax >= m + 1 (DSEA_ERR_WORKSPACE), V 16-byte aligned and ldv even (DSEA_ERR_ALIGN); a
 * refused call enqueues nothing.                                                                                    */
int dsea_gmres_begin(dsea_ws_t ws, const double *b, const double *Ax, double *V, int64_t ldv, int64_t n, int m,
                     double *work, double target, double *state, void *stream);
int dsea_gmres_step(dsea_op_t op, dsea_ws_t ws, const double *shift, const double *u, double *V, int64_t ldv,
                    int64_t n, int j, int m, double *work, double target, double *state, void *stream);
int dsea_gmres_end(dsea_ws_t ws, const double *V, int64_t ldv, int64_t n, int m, double *work, const double *state,
                   double *x, void *stream);
int dsea_gmres_cycle(dsea_op_t op, dsea_ws_t ws, const double *shift, const double *b, double *x, double *V,
                     int64_t ldv, int m, double *work, double target, double *state, int first, void *stream);

/* CG on (A - (*shift) I) x = b from x (in: start vector, out: solution).  Stops when ||r|| < eps
 * (absolute, CG.py:25) or after maxiter iterations.  The loop runs on the device; the host polls the
 * device-side flag every `poll_every` iterations (0 = default).  SYNCHRONISES the stream before
 * returning.  iters_out / resnorm_out are host pointers (nullable).  state = 8 device doubles.    */
int dsea_cg_run(dsea_op_t op, dsea_ws_t ws, const double *shift, const double *b, double *x,
                double *state, double eps, int64_t maxiter, int poll_every, int64_t *iters_out,
                double *resnorm_out, void *stream);

/* ------------------------------------------------------------------ lowest-nev eigenpairs (docs/design/13-lowest-eigenpairs.md)
 * Psi = the m <= DSEA_MAX_NEV requested eigenvectors, stored as the basis is: row j at Psi + j*ldpsi (ldpsi >= n, even,
 * 16-byte aligned).  P = I - Psi Psi^T.                                                                                 */
#define DSEA_MAX_NEV 8

/* Y[j] = sum_{i<k} S[j*lds + i] Q[i] for j < m, in ONE pass over the basis.  Every column is bit-identical to
 * dsea_ritz_combine with that column of S (same per-row summation order in the tiled and the small-n split form). */
int dsea_ritz_combine_block(dsea_ws_t ws, const double *Q, int64_t ldq, int64_t n, int k, const double *S, int64_t lds,
                            int m, double *Y, int64_t ldy, void *stream);

/* out = v - Psi (Psi^T v) (out may be v); coef_out (nullable, device) receives the m dot products.  Two launches: the m
 * fused dot products, then the apply.  The workspace must have been created with kmax >= m - 1.                     */
int dsea_block_project_out(dsea_ws_t ws, const double *v, const double *Psi, int64_t ldpsi, int m, double *out,
                           double *coef_out, int64_t n, void *stream);

/* Deflated CG: (A - (*shift) I) x = P b with x in range(P), for every operand dsea_cg_run accepts (streaming form only).
 * x (in: start vector, out: solution) is projected on entry; the residual is re-projected every iteration (its m dot
 * products folded into the update pass) and the stop is decided on ||P r|| computed from the projected vector.  A stop is
 * accepted only after the recomputed true residual ||P((A - shift) x - b)|| is below eps, otherwise CG restarts from x.
 * state, iters_out, resnorm_out, poll_every and DSEA_ERR_NOT_CONVERGED as dsea_cg_run; SYNCHRONISES the stream.
 * DSEA_ERR_ARG if m < 1, m > DSEA_MAX_NEV or the workspace was created with kmax < m + 1.                              */
int dsea_cg_run_deflated(dsea_op_t op, dsea_ws_t ws, const double *shift, const double *b, double *x, const double *Psi,
                         int64_t ldpsi, int m, double *state, double eps, int64_t maxiter, int poll_every,
                         int64_t *iters_out, double *resnorm_out, void *stream);

/* The same iteration around a CALLER-SUPPLIED mat-vec (the pattern of dsea_cg_init / dsea_cg_step).
 *   dsea_cg_deflated_init: on entry x is in range(P) (dsea_block_project_out) and Ax = A x; r = P(b - (A - shift) x),
 *       d = r, state cleared, state[RR] = ||r||^2 and the stop flag on ||r|| < eps.  Also the restart that checks a stop.
 *   dsea_cg_deflated_step: on entry Ad = A d.  Ad -= shift d; alpha; x += alpha d; r -= alpha Ad; r = P r; the stop test on
 *       ||r||; d = r + beta d.  `iteration` counts from 0 since the last dsea_cg_deflated_init.  No-op once DONE is set.
 * DSEA_ERR_ARG as dsea_cg_run_deflated.                                                                                  */
int dsea_cg_deflated_init(dsea_ws_t ws, const double *b, const double *x, const double *Ax, const double *shift,
                          const double *Psi, int64_t ldpsi, int m, double *r, double *d, double *state, double eps,
                          int64_t n, void *stream);
int dsea_cg_deflated_step(dsea_ws_t ws, double *x, double *r, double *d, double *Ad, const double *shift,
                          const double *Psi, int64_t ldpsi, int m, double *state, double eps, int64_t iteration,
                          int64_t n, void *stream);

/* ------------------------------------------------------------------ reduced density matrices (docs/design/21-reduced-density-matrix.md)
 * A bipartition A | B of the L sites of a spin operator.  sites_host: int32 [LA], the sites of A in the caller's order,
 * distinct, 1 <= LA <= min(L - 1, 16): bit k of the A-word a is the bit of site sites_host[k]; B is the other LB = L - LA sites
 * in increasing order, bit k of the B-word b the bit of site B[k].  ndown >= 1: vectors of dsea_op_create_sector at (L, ndown)
 * (row r = the r-th state with ndown set bits); the reduced density matrix is block diagonal in the number m of set bits
 * inside A, m = max(0, ndown - LB) .. min(LA, ndown): row i of block m is the i-th LA-bit word with m set bits in increasing
 * integer order, column j the j-th LB-bit word with ndown - m set bits, dA_m = C(LA, m), dB_m = C(LB, ndown - m).  ndown = -1:
 * vectors of the full 2^L space (L <= 30, row = state), one block with dA = 2^LA, dB = 2^LB.
 *     M_m(x)[i, j] = x[row(dep_A(a_i) | dep_B(b_j))]     cross(x, y)_m = M_m(x) M_m(y)^T     rho_m = cross(psi, psi)_m
 * Every function takes the same (L, ndown, LA, sites_host) and refuses, by host arithmetic before any device work
 * (DSEA_ERR_ARG): a site repeated or out of range, LA outside its limits, the limits of dsea_sector_table_sizes, the full
 * space with L > 30, a flat output sum_m dA_m^2 of 2^31 elements or more, a null pointer. */
#define DSEA_RDM_MAX_SITES 16  /* most sites of A (take the complement of a larger A: the same non-zero spectrum) */
#define DSEA_RDM_MAX_BLOCKS 17
/* dsea_rdm_sizes: n (the vector length), nblocks, out_len = sum_m dA_m^2, and blocks [5 * nblocks] (room for
 * 5 * DSEA_RDM_MAX_BLOCKS): per block m, dA_m, dB_m, its offset into idx and its offset into the flat output. */
int dsea_rdm_sizes(int L, int ndown, int LA, const int32_t *sites_host, int64_t *n, int *nblocks, int64_t *blocks,
                   int64_t *out_len);
/* The index table, int32 [n] on the device, filled on `stream` once per (L, ndown, sites): block after block, j fastest,
 * idx[off_m + i dB_m + j] = the row of (a_i, b_j); a permutation of 0 .. n - 1.  The sector form unranks (m, i, j), deposits
 * and ranks through lo_rank / hi_base of dsea_sector_build_tables at (L, ndown); the full-space form (ndown = -1) deposits
 * only.  The library allocates nothing. */
int dsea_rdm_build_index_sector(int L, int ndown, int LA, const int32_t *sites_host, const int32_t *lo_rank,
                                const int32_t *hi_base, int32_t *idx, void *stream);
int dsea_rdm_build_index_full(int L, int LA, const int32_t *sites_host, int32_t *idx, void *stream);
/* dsea_rdm_cross: out [out_len] = cross(x, y), block after block, each block row-major, all blocks in one launch on
 * v_mfma_f64_16x16x4_f64 with the inner dimension split over waves (partial tiles in `scratch`), then a fixed-order reduction:
 * no atomics, repeated calls return identical bits.  x == y (the same pointer): only tiles on or below the diagonal are
 * computed and the result is bitwise symmetric.  `scratch`: caller-owned, dsea_rdm_scratch_doubles doubles (enough for every
 * `tile`).  tile: 0 = the library's choice of the tile edge, 1 = 16, 2 = 32 (measurement aid).  x, y: fp64 [n]. */
int dsea_rdm_scratch_doubles(int L, int ndown, int LA, const int32_t *sites_host, int64_t *out);
int dsea_rdm_cross(int L, int ndown, int LA, const int32_t *sites_host, const int32_t *idx, const double *x, const double *y,
                   double *out, double *scratch, int tile, void *stream);
/* dsea_rdm_pull: the adjoint of cross in one launch.  out[idx[off_m + i dB_m + j]] = sum_i' G_m[i, i'] y[idx[off_m + i' dB_m + j]]
 * (transpose != 0: G_m[i', i]); G [out_len] in the layout of dsea_rdm_cross's output, out fp64 [n], not y.  idx is a
 * permutation, so every element of out is written exactly once: no atomics, no scratch. */
int dsea_rdm_pull(int L, int ndown, int LA, const int32_t *sites_host, const int32_t *idx, const double *G, const double *y,
                  double *out, int transpose, void *stream);

/* ------------------------------------------------------------------ sector ladder maps (docs/design/24-dynamics.md)
 * Linear maps from the sector (L, ndown_src) of dsea_op_create_sector to the sector (L, ndown_src + step) of the same L sites
 * (site i = bit i, a set bit = a down spin, z_i = 1 - 2 bit_i).  weights_dev: fp64 [L] on the device, one weight c_i per site,
 * READ THROUGH THE POINTER ON EVERY LAUNCH.  With r' a row of the destination and s' its state:
 *     step = +1, sigma^-(c):  y[r'] = sum_{i : bit_i(s') = 1} c_i x[rank_src(s' ^ (1 << i))]     (sigma^- sets a bit)
 *     step = -1, sigma^+(c):  y[r'] = sum_{i : bit_i(s') = 0} c_i x[rank_src(s' | (1 << i))]     (sigma^+ clears a bit)
 *     step =  0, Z(c):        y[r'] = (sum_i c_i z_i(s')) x[r']
 * sigma^+- = (X +- iY) / 2 have matrix elements 1, and sigma^+(c) is the transpose of sigma^-(c).  All three are gathers over
 * the destination rows (no atomics).  states_dst: the state table of the DESTINATION sector; lo_rank_src, hi_base_src: the two
 * rank tables of the SOURCE sector (dsea_sector_build_tables at the two sectors; for step = 0 they are one sector's).  x fp64
 * [n_src], y fp64 [n_dst].  grid_log2: log2 of the most blocks of a launch, 6 .. 12, 0 = the default 12.  The library allocates
 * nothing.  Refused by host arithmetic before any device work (DSEA_ERR_ARG): step outside {-1, 0, 1}; either sector outside
 * the limits of dsea_sector_table_sizes (so a destination with ndown = 0 or ndown = L); grid_log2 outside {0, 6 .. 12}; a
 * null pointer; x == y when step != 0. */
int dsea_sector_ladder_apply(int L, int ndown_src, int step, const double *weights_dev, const int64_t *states_dst,
                             const int32_t *lo_rank_src, const int32_t *hi_base_src, const double *x, double *y,
                             int grid_log2 /* 0 = default */, void *stream);
/* dsea_sector_ladder_forms: out [L] on the device, out[i] = v1^T (dS/dc_i) v2 for every site in one pass, v1 fp64 [n_dst] on
 * the destination and v2 fp64 [n_src] on the source: sum_{r' : bit_i qualifies} v1[r'] v2[rank_src(...)] for step = +-1,
 * sum_r z_i v1[r] v2[r] for step = 0.  Wave and block reductions in fixed order into per-block partials in `scratch`, then one
 * block per form: no floating-point atomics, repeated calls return identical bits.  `scratch`: caller-owned,
 * dsea_sector_ladder_forms_scratch_doubles = L * min(4096, ceil(n_dst / 256)) doubles (enough for every grid cap).  The same
 * argument checks as dsea_sector_ladder_apply. */
int dsea_sector_ladder_forms_scratch_doubles(int L, int ndown_src, int step, int64_t *out);
int dsea_sector_ladder_forms(int L, int ndown_src, int step, const int64_t *states_dst, const int32_t *lo_rank_src,
                             const int32_t *hi_base_src, const double *v1, const double *v2, double *out, double *scratch,
                             int grid_log2, void *stream);

/* ------------------------------------------------------------------ Hubbard ladder maps (docs/design/25-hubbard-ladder.md)
 * Linear maps from the Hubbard sector (L, nup_src, ndn_src) of dsea_op_create_hubbard to the sector of the same L sites in which
 * the count of one species (species: 0 up, 1 dn) is changed by step; conventions and row order r = ru * n_dn + rd of
 * dsea_op_create_hubbard.  weights_dev: fp64 [L] on the device, one weight c_i per site, READ THROUGH THE POINTER ON EVERY
 * LAUNCH.  With w' the word of the moving species in a row of the destination, below_i = (1 << i) - 1, par = popcount & 1:
 *     step = +1, sum_i c_i c+_{i s}:  y[row] = g sum_{i : bit_i(w') = 1} c_i (-1)^par(w' & below_i) x[row with rank_src(w' ^ (1 << i))]
 *     step = -1, sum_i c_i c_{i s}:   y[row] = g sum_{i : bit_i(w') = 0} c_i (-1)^par(w' & below_i) x[row with rank_src(w' | (1 << i))]
 *     step =  0, sum_i c_i n_{i s}:   y[row] = (sum_i c_i bit_i(w')) x[row]
 * g = 1 for the up species and (-1)^nup_src for the down species (every down operator stands right of all up operators).  The
 * other species keeps its rank; the row stride is C(L, ndn) of the destination for y and of the source for x.  The map with the
 * two sectors exchanged and step negated is the exact transpose.  All are gathers over the destination rows (no atomics).
 * states_dst: the state table of the MOVING species at its DESTINATION count; lo_rank_src, hi_base_src: its two rank tables at
 * its SOURCE count (dsea_sector_build_tables; for step = 0 they are one count's).  x fp64 [n_src], y fp64 [n_dst].  grid_log2:
 * log2 of the most blocks of a launch, 6 .. 12, 0 = the default 12.  The library allocates nothing.  Refused by host arithmetic
 * before any device work (DSEA_ERR_ARG): species outside {0, 1}; step outside {-1, 0, 1}; the source or the destination
 * outside the limits of dsea_hubbard_sizes (so a destination count of 0 or L); grid_log2 outside {0, 6 .. 12}; a null pointer;
 * x == y when step != 0. */
int dsea_hubbard_ladder_apply(int L, int nup_src, int ndn_src, int species /* 0 up, 1 dn */, int step, const double *weights_dev,
                              const int64_t *states_dst, const int32_t *lo_rank_src, const int32_t *hi_base_src, const double *x,
                              double *y, int grid_log2 /* 0 = default */, void *stream);
/* dsea_hubbard_ladder_forms: out [L] on the device, out[i] = v1^T (dS/dc_i) v2 for every site in one pass, v1 fp64 [n_dst] on
 * the destination and v2 fp64 [n_src] on the source.  Wave and block reductions in fixed order into per-block partials in
 * `scratch`, then one block per form: no floating-point atomics, repeated calls return identical bits.  `scratch`: caller-owned,
 * dsea_hubbard_ladder_forms_scratch_doubles = L * min(4096, ceil(n_dst / 256)) doubles (enough for every grid cap).  The same
 * argument checks as dsea_hubbard_ladder_apply. */
int dsea_hubbard_ladder_forms_scratch_doubles(int L, int nup_src, int ndn_src, int species, int step, int64_t *out);
int dsea_hubbard_ladder_forms(int L, int nup_src, int ndn_src, int species, int step, const int64_t *states_dst,
                              const int32_t *lo_rank_src, const int32_t *hi_base_src, const double *v1, const double *v2,
                              double *out, double *scratch, int grid_log2, void *stream);

/* ------------------------------------------------------------------ Hubbard pair maps (docs/design/41-hubbard-pair-ladder.md)
 * Linear maps from the Hubbard sector (L, nup_src, ndn_src) to (nup_src + step_up, ndn_src + step_dn), step_up and step_dn each
 * +1 or -1: one particle of EACH species moves in one pass.  Conventions and row order of dsea_op_create_hubbard.  With A = c+
 * for step_up = +1 and c for -1, B likewise for step_dn, and weights_dev fp64 [L, L] row-major on the device, READ THROUGH THE
 * POINTER ON EVERY LAUNCH: order 0 is sum_ij W_ij A_{i up} B_{j dn}, order 1 is sum_ij W_ij B_{j dn} A_{i up} (its negative).  With
 * (u', d') the words of a row of the destination, below_i = (1 << i) - 1, par = popcount & 1:
 *     y[ru' n_dn_dst + rd'] = g sum_{i qualifies in u'} sum_{j qualifies in d'} W_ij (-1)^par(u' & below_i) (-1)^par(d' & below_j)
 *                               x[rank_up_src(u' ^ (1 << i)) n_dn_src + rank_dn_src(d' ^ (1 << j))]
 * A site qualifies when its bit is set in the destination word for a step of +1 and clear for -1; g = (-1)^(nup_src + order).
 * The terms are added i ascending outer, j ascending inner.  The map (-step_up, -step_dn, 1 - order) from the destination to
 * the source is the exact transpose.  A gather over the destination rows (no atomics).  The six tables
 * (dsea_sector_build_tables): for the up species and then for the down species, the state table at its DESTINATION count and
 * lo_rank, hi_base at its SOURCE count.  x fp64 [n_src], y fp64 [n_dst].  grid_log2: log2 of the most blocks of a launch,
 * 6 .. 12, 0 = the default 12.  The library allocates nothing.  Refused by host arithmetic before any device work
 * (DSEA_ERR_ARG): a step that is not +1 or -1; order outside {0, 1}; the source or the destination outside the limits of
 * dsea_hubbard_sizes; grid_log2 outside {0, 6 .. 12}; a null pointer; x == y. */
int dsea_hubbard_pair_apply(int L, int nup_src, int ndn_src, int step_up, int step_dn, int order /* 0 up left, 1 dn left */,
                            const double *weights_dev, const int64_t *up_states_dst, const int32_t *up_lo_rank_src,
                            const int32_t *up_hi_base_src, const int64_t *dn_states_dst, const int32_t *dn_lo_rank_src,
                            const int32_t *dn_hi_base_src, const double *x, double *y, int grid_log2 /* 0 = default */,
                            void *stream);
/* dsea_hubbard_pair_forms: out [L, L] on the device, out[i * L + j] = v1^T (dP/dW_ij) v2 for every site pair in one pass, v1 fp64
 * [n_dst] on the destination and v2 fp64 [n_src] on the source.  Wave and block reductions in fixed order into per-block
 * partials in `scratch`, then one block per form: no floating-point atomics, repeated calls return identical bits.  `scratch`:
 * caller-owned, dsea_hubbard_pair_forms_scratch_doubles = L * L * min(4096, ceil(n_dst / 256)) doubles (enough for every grid
 * cap).  The same argument checks as dsea_hubbard_pair_apply. */
int dsea_hubbard_pair_forms_scratch_doubles(int L, int nup_src, int ndn_src, int step_up, int step_dn, int order, int64_t *out);
int dsea_hubbard_pair_forms(int L, int nup_src, int ndn_src, int step_up, int step_dn, int order, const int64_t *up_states_dst,
                            const int32_t *up_lo_rank_src, const int32_t *up_hi_base_src, const int64_t *dn_states_dst,
                            const int32_t *dn_lo_rank_src, const int32_t *dn_hi_base_src, const double *v1, const double *v2,
                            double *out, double *scratch, int grid_log2, void *stream);

/* ------------------------------------------------------------------ block sector mat-vec, block Lanczos (docs/design/27-finite-temperature.md)
 * The operator of dsea_op_create_sector applied to R vectors at once, and the basis-free Lanczos recurrence on it.  A block is fp64
 * [n, R] row-major (element (r, j) at r * R + j), 16-byte aligned (DSEA_ERR_ALIGN otherwise), R in {1, 2, 4, 8}.  The library
 * allocates nothing; every check is host arithmetic before any device work.  DSEA_ERR_ARG: any other operator kind, R outside
 * {1, 2, 4, 8}, k < 1, a null pointer, X == Y, Q == W.  DSEA_TUNE_TFIM_TILE_LOG2 of the handle caps the grid as for its mat-vec.
 * dsea_op_sector_block_apply: Y = H X; column j of Y equals the single-vector mat-vec of column j of X bit for bit.
 * dsea_op_sector_block_lanczos: k steps of the three-term recurrence for every column, WITHOUT a stored basis and without
 * re-orthogonalisation; nothing is read back during the run and the call does not synchronise.  Q [n, R]: the start block, any
 * norms (normalised on the device), overwritten; W [n, R]: work; on return both hold the last two Lanczos blocks.  norm2 [R]:
 * |start column|^2.  alphas [k, R], betas [k, R] row-major: alphas[i, j] = alpha_i, betas[i, j] = beta_{i+1} of column j.  steps
 * [R]: column j breaks at the first s with beta_s <= 1e-13 max(its earlier |alpha|, |beta|) (the rule of dsea_lanczos_status;
 * a start column of norm 0 breaks at s = 0): steps[j] = s, its leading s x s block of T holds exact eigenvalues, the column is
 * zeroed, its entries alphas[i >= s, j] and betas[i >= s - 1, j] are 0, and the other columns go on; steps[j] = k otherwise.
 * Every reduction runs in fixed order (no floating-point atomics): identical calls return identical bits.  scratch:
 * caller-owned, dsea_op_sector_block_lanczos_scratch_doubles(L, ndown, R) = 64 + 2 R min(4096, ceil(n / 256)) doubles (enough
 * for every grid cap).  After k steps Q_k lies in W for odd k and in Q for even k, Q_{k-1} in the other array. */
int dsea_op_sector_block_apply(dsea_op_t op, int R, const double *X, double *Y, void *stream);
int dsea_op_sector_block_lanczos_scratch_doubles(int L, int ndown, int R, int64_t *out);
int dsea_op_sector_block_lanczos(dsea_op_t op, int R, int k, double *Q /* [n,R] in: start block, any norms; overwritten */,
                                 double *W /* [n,R] work */, double *norm2 /* [R] out: |start column|^2 */,
                                 double *alphas /* [k,R] */, double *betas /* [k,R]: betas[i,j] = beta_{i+1} */,
                                 int32_t *steps /* [R]: k, or the break step */, double *scratch, void *stream);

/* ------------------------------------------------------------------ block Hubbard mat-vec, block Lanczos (docs/design/28-hubbard-finite-temperature.md)
 * The operator of dsea_op_create_hubbard applied to R vectors at once, and the same basis-free Lanczos recurrence on it: the twins
 * of the three entries above, with the same blocks (fp64 [n, R] row-major, 16-byte aligned, DSEA_ERR_ALIGN otherwise, R in
 * {1, 2, 4, 8}), the same outputs, break rule and scratch layout.  The library allocates nothing; every check is host
 * arithmetic before any device work.  DSEA_ERR_ARG: any other operator kind, R outside {1, 2, 4, 8}, k < 1, a null pointer,
 * X == Y, Q == W, and in the scratch query (L, nup, ndn) outside the limits of dsea_hubbard_sizes.
 * dsea_op_hubbard_block_apply: Y = H X; column j of Y equals dsea_op_apply without a shift on column j of X bit for bit.
 * dsea_op_hubbard_block_lanczos: as dsea_op_sector_block_lanczos.  scratch: caller-owned,
 * dsea_op_hubbard_block_lanczos_scratch_doubles(L, nup, ndn, R) = 64 + 2 R min(4096, ceil(n / 256)) doubles (enough for every
 * grid cap). */
int dsea_op_hubbard_block_apply(dsea_op_t op, int R, const double *X, double *Y, void *stream);
int dsea_op_hubbard_block_lanczos_scratch_doubles(int L, int nup, int ndn, int R, int64_t *out);
int dsea_op_hubbard_block_lanczos(dsea_op_t op, int R, int k, double *Q /* [n,R] in: start block, any norms; overwritten */,
                                  double *W /* [n,R] work */, double *norm2 /* [R] out: |start column|^2 */,
                                  double *alphas /* [k,R] */, double *betas /* [k,R]: betas[i,j] = beta_{i+1} */,
                                  int32_t *steps /* [R]: k, or the break step */, double *scratch, void *stream);

/* ------------------------------------------------------------------ Chebyshev block propagator (docs/design/31-chebyshev-propagator.md)
 * ACC[a] = f_a(H) X for the operator of dsea_op_create_sector and a block X, without a stored basis: f_a(E) ~=
 * sum_{m < M} coeffs[a * M + m] T_m((E - centre) / halfwidth), a in [0, A), with coeffs[a * M + 0] ALREADY HALVED and the
 * spectrum of H inside [centre - halfwidth, centre + halfwidth] (outside it the polynomials grow without bound).  Blocks as
 * above: fp64 [n, R] row-major, 16-byte aligned (DSEA_ERR_ALIGN otherwise), R in {1, 2, 4, 8}.  coeffs [A, M] is a HOST array:
 * two numbers per accumulator go into each launch by value.  X is never written; U and V are work blocks (on return they hold
 * the last two T_m X); ACC is [A, n, R], one block per accumulator, A in {1, 2}.  M - 1 launches, one fused mat-vec and tail
 * each: T_1 X = (H X - centre X) / halfwidth, T_{m+1} X = (2 / halfwidth)(H T_m X - centre T_m X) - T_{m-1} X, every product and
 * sum rounded on its own (no contraction), so the result equals dsea_op_sector_block_apply followed by separate elementwise
 * operations bit for bit.  No reductions, no atomics: identical calls return identical bits.  Nothing is read back, the call
 * does not synchronise, the library allocates nothing; every check is host arithmetic before any device work.  DSEA_ERR_ARG:
 * any other operator kind, R outside {1, 2, 4, 8}, A outside {1, 2}, M < 2, a null pointer, centre or halfwidth not finite,
 * halfwidth <= 0, any two of X, U, V, ACC, ACC + n R equal. */
int dsea_op_sector_block_chebyshev(dsea_op_t op, int R, int A, int M, double centre, double halfwidth,
                                   const double *coeffs /* host [A,M], c_0 halved */, const double *X /* [n,R] */,
                                   double *U /* [n,R] work */, double *V /* [n,R] work */, double *ACC /* [A,n,R] out */,
                                   void *stream);

/* ------------------------------------------------------------------ Chebyshev block moments (docs/design/33-chebyshev-moments.md)
 * MU[m, j] = l_j . T_m((H - centre) / halfwidth) x_j, m in [0, M), for the operator of dsea_op_create_sector, the columns x_j of a
 * block X and l = X (Y null: self mode) or the columns of a second block Y (left mode), without a stored basis; the spectrum of
 * H must lie inside [centre - halfwidth, centre + halfwidth].  Blocks as above: fp64 [n, R] row-major, 16-byte aligned
 * (DSEA_ERR_ALIGN otherwise), R in {1, 2, 4, 8}.  MU is a DEVICE array [M, R] row-major.  X and Y are never written; U and V are
 * work blocks.  Every order is one launch of the fused mat-vec, recurrence tail and two dot products per column, followed by one
 * one-block launch that sums the per-block partials in index order.  Self mode takes K = ceil(M / 2) orders: order m gives
 * mu_{2m-2} = 2 <T_{m-1} x | T_{m-1} x> - mu_0 and mu_{2m-1} = 2 <T_{m-1} x | T_m x> - mu_1 (the product rule T_a T_b =
 * (T_{a+b} + T_{|a-b|}) / 2; the doubling is exact and the subtraction rounds once).  Left mode takes K = M - 1 orders: order m
 * gives mu_m = y . T_m x.  ON RETURN T_K X is in U for odd K and in V for even K, and T_{K-1} X is in the other work block (for
 * K = 1 it is X itself and V is untouched); they equal the work blocks of dsea_op_sector_block_chebyshev after K orders bit for
 * bit.  No atomics: identical calls return identical bits.  Nothing is read back, the call does not synchronise, the library
 * allocates nothing; every check is host arithmetic before any device work.  scratch: caller-owned,
 * dsea_op_sector_block_moments_scratch_doubles(L, ndown, R) = 2 R min(4096, ceil(n / 256)) doubles (enough for every grid cap).
 * DSEA_ERR_ARG: any other operator kind, R outside {1, 2, 4, 8}, M < 2, a null X, U, V, MU or scratch, centre or halfwidth not
 * finite, halfwidth <= 0, any two of X, Y, U, V equal; in the scratch query (L, ndown) outside the limits of
 * dsea_sector_table_sizes or a null out. */
int dsea_op_sector_block_moments_scratch_doubles(int L, int ndown, int R, int64_t *out);
int dsea_op_sector_block_moments(dsea_op_t op, int R, int M, double centre, double halfwidth, const double *X /* [n,R] */,
                                 const double *Y /* [n,R] left block, or NULL: self mode */, double *U /* [n,R] work */,
                                 double *V /* [n,R] work */, double *MU /* device [M,R] out */, double *scratch, void *stream);

/* ------------------------------------------------------------------ Hubbard Chebyshev propagator and moments (docs/design/34-hubbard-chebyshev.md)
 * The twins of dsea_op_sector_block_chebyshev and of the two moments entries above for the operator of dsea_op_create_hubbard:
 * the same quantities, blocks (fp64 [n, R] row-major, 16-byte aligned, DSEA_ERR_ALIGN otherwise, R in {1, 2, 4, 8}), host coeffs
 * [A, M] with coeffs[a * M + 0] ALREADY HALVED, device MU [M, R], launch schedules and rounding: every order is one launch of
 * the Hubbard block mat-vec with the recurrence tail inside (the moments: with the two dot products per column inside, then one
 * one-block launch that sums the per-block partials in index order), every product and sum of the recurrence rounded on its
 * own, so that ACC, U and V equal dsea_op_hubbard_block_apply followed by separate elementwise operations bit for bit.  The
 * spectrum of H must lie inside [centre - halfwidth, centre + halfwidth].  X and Y are never written; U and V are work blocks.
 * dsea_op_hubbard_block_chebyshev: ACC[a] = sum_{m < M} coeffs[a * M + m] T_m((H - centre) / halfwidth) X, a in [0, A), A in
 * {1, 2}, ACC [A, n, R], in M - 1 launches; on return U and V hold the last two T_m X.  No reductions, no atomics.
 * dsea_op_hubbard_block_moments: MU[m, j] = l_j . T_m((H - centre) / halfwidth) x_j, m in [0, M), l = X (Y null: self mode,
 * K = ceil(M / 2) orders, two moments per order by the product rule) or the columns of Y (left mode, K = M - 1 orders).  ON
 * RETURN T_K X is in U for odd K and in V for even K, and T_{K-1} X is in the other work block (for K = 1 it is X itself and V is
 * untouched); they equal the work blocks of dsea_op_hubbard_block_chebyshev after K orders bit for bit.  No atomics: identical
 * calls return identical bits.  scratch: caller-owned, dsea_op_hubbard_block_moments_scratch_doubles(L, nup, ndn, R) =
 * 2 R min(4096, ceil(n / 256)) doubles (enough for every grid cap).
 * Nothing is read back, the calls do not synchronise, the library allocates nothing; every check is host arithmetic before any
 * device work.  DSEA_ERR_ARG: any other operator kind, R outside {1, 2, 4, 8}, A outside {1, 2}, M < 2, a null coeffs, X, U, V,
 * ACC, MU or scratch, centre or halfwidth not finite, halfwidth <= 0, any two of X, U, V, ACC, ACC + n R equal (propagator), any
 * two of X, Y, U, V equal (moments); in the scratch query (L, nup, ndn) outside the limits of dsea_hubbard_sizes or a null out. */
int dsea_op_hubbard_block_chebyshev(dsea_op_t op, int R, int A, int M, double centre, double halfwidth,
                                    const double *coeffs /* host [A,M], c_0 halved */, const double *X /* [n,R] */,
                                    double *U /* [n,R] work */, double *V /* [n,R] work */, double *ACC /* [A,n,R] out */,
                                    void *stream);
int dsea_op_hubbard_block_moments_scratch_doubles(int L, int nup, int ndn, int R, int64_t *out);
int dsea_op_hubbard_block_moments(dsea_op_t op, int R, int M, double centre, double halfwidth, const double *X /* [n,R] */,
                                  const double *Y /* [n,R] left block, or NULL: self mode */, double *U /* [n,R] work */,
                                  double *V /* [n,R] work */, double *MU /* device [M,R] out */, double *scratch, void *stream);

/* ------------------------------------------------------------------ block sector ladder maps (docs/design/35-finite-temperature-dynamics.md)
 * The maps of dsea_sector_ladder_apply applied to R vectors at once, and their column dots.  The sectors, the step, weights_dev
 * (fp64 [L] on the device, READ THROUGH THE POINTER ON EVERY LAUNCH), the three tables and grid_log2 are those of
 * dsea_sector_ladder_apply.  A block is fp64 [n, R] row-major (element (r, j) at r * R + j), 16-byte aligned (DSEA_ERR_ALIGN
 * otherwise), R in {1, 2, 4, 8}: X and the result of the map are [n_src, R] and [n_dst, R].  A row's table reads are made once
 * for all R columns.
 * dsea_sector_ladder_block_apply: Y = S(c) X; column j of Y equals dsea_sector_ladder_apply on column j of X bit for bit.
 * dsea_sector_ladder_block_dots: out_dev[j] = sum_r' Lft[r', j] (S(c) X)[r', j], Lft [n_dst, R], out_dev fp64 [R] on the device;
 * the product block is never stored.  Wave and block sums in fixed order into per-block partials in `scratch`, then one block
 * per column: no floating-point atomics, repeated calls return identical bits, and column j of a call equals the call with
 * R = 1 on that column.  `scratch`: caller-owned, dsea_sector_ladder_block_dots_scratch_doubles = R * min(4096,
 * ceil(n_dst / 256)) doubles (enough for every grid cap).
 * Nothing is allocated, read back or synchronised.  Refused by host arithmetic before any device work (DSEA_ERR_ARG):
 * everything dsea_sector_ladder_apply refuses; R outside {1, 2, 4, 8}; X == Y when step != 0; a null X, Y, Lft, out_dev, scratch
 * or (in the query) out. */
int dsea_sector_ladder_block_apply(int L, int ndown_src, int step, int R, const double *weights_dev, const int64_t *states_dst,
                                   const int32_t *lo_rank_src, const int32_t *hi_base_src, const double *X /* [n_src,R] */,
                                   double *Y /* [n_dst,R] */, int grid_log2 /* 0 = default */, void *stream);
int dsea_sector_ladder_block_dots_scratch_doubles(int L, int ndown_src, int step, int R, int64_t *out);
int dsea_sector_ladder_block_dots(int L, int ndown_src, int step, int R, const double *weights_dev, const int64_t *states_dst,
                                  const int32_t *lo_rank_src, const int32_t *hi_base_src, const double *Lft /* [n_dst,R] */,
                                  const double *X /* [n_src,R] */, double *out_dev /* [R] */, double *scratch, int grid_log2,
                                  void *stream);

/* ------------------------------------------------------------------ block Hubbard ladder maps (docs/design/37-hubbard-finite-temperature-dynamics.md)
 * The maps of dsea_hubbard_ladder_apply applied to R vectors at once, and their column dots.  The sectors, the species, the step,
 * weights_dev (fp64 [L] on the device, READ THROUGH THE POINTER ON EVERY LAUNCH), the three tables and grid_log2 are those of
 * dsea_hubbard_ladder_apply.  A block is fp64 [n, R] row-major (element (r, j) at r * R + j), 16-byte aligned (DSEA_ERR_ALIGN
 * otherwise; the argument checks come first), R in {1, 2, 4, 8}: X and the result of the map are [n_src, R] and [n_dst, R].  A
 * row's division, state word and table reads are made once for all R columns.
 * dsea_hubbard_ladder_block_apply: Y = S(c) X; column j of Y equals dsea_hubbard_ladder_apply on column j of X bit for bit.
 * dsea_hubbard_ladder_block_dots: out_dev[j] = sum_r' Lft[r', j] (S(c) X)[r', j], Lft [n_dst, R], out_dev fp64 [R] on the device;
 * the product block is never stored.  Wave and block sums in fixed order into per-block partials in `scratch`, then one block
 * per column: no floating-point atomics, repeated calls return identical bits, and column j of a call equals the call with
 * R = 1 on that column.  `scratch`: caller-owned, dsea_hubbard_ladder_block_dots_scratch_doubles = R * min(4096,
 * ceil(n_dst / 256)) doubles (enough for every grid cap).
 * Nothing is allocated, read back or synchronised.  Refused by host arithmetic before any device work (DSEA_ERR_ARG):
 * everything dsea_hubbard_ladder_apply refuses; R outside {1, 2, 4, 8}; X == Y when step != 0 (at step 0 a thread reads its row
 * before it writes it); a null X, Y, Lft, out_dev, scratch or (in the query) out. */
int dsea_hubbard_ladder_block_apply(int L, int nup_src, int ndn_src, int species /* 0 up, 1 dn */, int step, int R,
                                    const double *weights_dev, const int64_t *states_dst, const int32_t *lo_rank_src,
                                    const int32_t *hi_base_src, const double *X /* [n_src,R] */, double *Y /* [n_dst,R] */,
                                    int grid_log2 /* 0 = default */, void *stream);
int dsea_hubbard_ladder_block_dots_scratch_doubles(int L, int nup_src, int ndn_src, int species, int step, int R, int64_t *out);
int dsea_hubbard_ladder_block_dots(int L, int nup_src, int ndn_src, int species, int step, int R, const double *weights_dev,
                                   const int64_t *states_dst, const int32_t *lo_rank_src, const int32_t *hi_base_src,
                                   const double *Lft /* [n_dst,R] */, const double *X /* [n_src,R] */, double *out_dev /* [R] */,
                                   double *scratch, int grid_log2, void *stream);

/* ------------------------------------------------------------------ Hubbard bond current map (docs/design/39-hubbard-current.md)
 * The bond-weighted, real antisymmetric map K(w) = sum_t sum_s w_{s t} (c+_{a s} c_{b s} - c+_{b s} c_{a s}) on the sector of
 * an operator of dsea_op_create_hubbard, (a, b) = bond t in the orientation given at creation; the current operator is J = i K(w).
 * It works on the operator's sector, tables, bond list and grid cap (dsea_op_set_tuning) and does not read its couplings.
 * Reversing a bond flips its sign, a repeated bond counts each time, K(w)^T = -K(w).  weights_dev: fp64 [2 nb] on the device, the
 * up weights then the down weights, READ THROUGH THE POINTER ON EVERY LAUNCH.
 * dsea_op_hubbard_current_apply: Y = K(w) X for a block fp64 [n, R] row-major (element (r, j) at r * R + j), R in {1, 2, 4, 8};
 * blocks with R >= 2 must be 16-byte aligned (DSEA_ERR_ALIGN otherwise; the argument checks come first).  Every product is
 * exact (the signs go into the sign bit of the weight) and column j of Y is the same bits at every R.
 * dsea_op_hubbard_current_forms: out[s * nb + t] = v1^T K_{s t} v2 for all 2 nb unit-weight bond maps (s = 0 up, 1 dn) in one
 * pass: the adjoint of the map in its weights.  Wave and block sums in fixed order into per-block partials in `scratch`, then
 * one block per form: no floating-point atomics, repeated calls return identical bits.  `scratch`: caller-owned,
 * dsea_op_hubbard_current_forms_scratch_doubles = 2 nb * min(4096, ceil(n / 256)) doubles (enough for every grid cap).
 * Nothing is allocated, read back or synchronised.  Refused by host arithmetic before any device work (DSEA_ERR_ARG): an
 * operator of another kind; R outside {1, 2, 4, 8}; X == Y; a null op, weights_dev, X, Y, v1, v2, out, scratch; in the query a
 * sector that dsea_hubbard_sizes refuses or nb outside 1 .. DSEA_LATTICE_MAX_BONDS. */
int dsea_op_hubbard_current_apply(dsea_op_t op, int R, const double *weights_dev /* [2 nb]: up then dn */,
                                  const double *X /* [n,R] */, double *Y /* [n,R] */, void *stream);
int dsea_op_hubbard_current_forms_scratch_doubles(int L, int nup, int ndn, int nb, int64_t *out);
int dsea_op_hubbard_current_forms(dsea_op_t op, const double *v1, const double *v2, double *out /* [2 nb] */,
                                  double *scratch, void *stream);

/* ------------------------------------------------------------------ Hubbard current column dots (docs/design/40-finite-temperature-conductivity.md)
 * out_dev[j] = sum_r Lft[r, j] (K(w) X)[r, j] for the R columns of two blocks fp64 [n, R] row-major of the operator's sector, K(w)
 * the map of the section above with the same weights_dev [2 nb], without the product block K X: the rows of K X are formed as
 * dsea_op_hubbard_current_apply forms them (the same bits) and multiplied into the row of Lft at once.  Wave and block sums in
 * fixed order into per-block partials in `scratch`, then one block per column: no floating-point atomics, repeated calls return
 * identical bits, and column j of an R = 8 call equals the R = 1 call on that column bit for bit.  Lft == X is allowed (both are
 * only read; the result is then 0 up to rounding, K being antisymmetric).  `scratch`: caller-owned,
 * dsea_op_hubbard_current_block_dots_scratch_doubles = R * min(4096, ceil(n / 256)) doubles (enough for every grid cap).
 * Nothing is allocated, read back or synchronised.  Refused by host arithmetic before any device work (DSEA_ERR_ARG): an
 * operator of another kind; R outside {1, 2, 4, 8}; a null op, weights_dev, Lft, X, out_dev or scratch; in the query a sector
 * that dsea_hubbard_sizes refuses, R outside {1, 2, 4, 8} or a null out.  With R >= 2, Lft and X must be 16-byte aligned
 * (DSEA_ERR_ALIGN otherwise; the argument checks come first). */
int dsea_op_hubbard_current_block_dots_scratch_doubles(int L, int nup, int ndn, int R, int64_t *out);
int dsea_op_hubbard_current_block_dots(dsea_op_t op, int R, const double *weights_dev /* [2 nb]: up then dn */,
                                       const double *Lft /* [n,R] */, const double *X /* [n,R] */, double *out_dev /* [R] */,
                                       double *scratch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DSEA_H */
