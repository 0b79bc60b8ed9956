"""numpy reference, input classes, judges, wrong kernels and checks of the block Lanczos stage tests
(tests/test_gpu_block_lanczos_stages.py, proved on the CPU by tests/test_block_lanczos_reference_cpu.py); no GPU.
docs/design/36-block-lanczos-stage-tests.md tells the same story at length.

Only the whole run is exported (dsea_op_sector_block_lanczos, dsea_op_hubbard_block_lanczos), so a stage is isolated by the run
length: the kernels of step i are the same whatever k is, runs of k and k + 1 steps agree bit for bit in their first k rows,
and after k steps Q_k lies in the W array for odd k and in the Q array for even k, Q_{k-1} in the other one (``Run.latest`` /
``Run.previous``).

``Reference(dtype)`` states the run of csrc/dsea_block_lanczos.hip in ``dtype`` with the driver's own buffers -- the two arrays
that change roles, the two copies of the per-column state (beta, scale, alive) that alternate by step:

  start    norm2_j = sum phi_j^2; beta_0 = sqrt(norm2_j); Q_0 = phi / beta_0; a column with not beta_0 > 0 (zero, NaN) breaks at
           s = 0: steps = 0, the column is zeroed.  beta_0 enters the scale AFTER its test, as every beta does
  step i   W = H Q_i - fl(beta_i Q_{i-1}) (product and difference rounded separately; i = 0: W = H Q_0, the other array is
           not read), beta_i from the state copy i & 1; alpha_i = Q_i . W; W' = W - fl(alpha_i Q_i); b = sqrt(sum W'^2);
           scale = max(scale, |alpha_i|); the column breaks at s = i + 1 if not b > 1e-13 scale: steps = s, betas[i] = 0, the
           column is zeroed in both arrays, alphas[i] is kept; otherwise betas[i] = beta_{i+1} = b, scale = max(scale, b),
           Q_{i+1} = W' / b.  A dead column stays zero, its later alphas and betas are 0, nothing divides by its beta

np.longdouble is the high-precision reference, np.float64 the MIRROR (the library is built with -ffp-contract=off and the tail
and the update are written with __dmul_rn / __dsub_rn: numpy rounds the same way), np.float64 with ``order`` an honest fp64
evaluation whose sums run over a random permutation.  The rules a wrong kernel breaks are small methods; MUTANTS overrides them
one at a time.

TWO INPUT CLASSES, TWO VERDICTS

  exact     couplings multiples of 1/4, start columns integer vectors on ``support_rows`` whose squared norm is a power of 4:
            Q_0, H Q_0, alpha_0, W' and sum W'^2 are exact (``Headroom`` asserts it term by term), beta_1 and Q_1 one correctly
            rounded operation each: the k = 1 run equals Reference(np.float64) bit for bit in every output, in any summation
            order, with or without FMA.  Break decisions: an operator with ONE hopping bond, whose invariant subspaces have
            dimension 1 and 2, so that the recurrence stays exact through the break (``BreakData``); the strict boundary of the
            rule; a NaN column; k = n + 2.
  random    synthetic.normal_vector couplings and start blocks, each step judged on the run's own inputs and outputs,
            u = 2^-53: Q_{i+1} bit-equal to ((A - fl(beta_i Q_{i-1})) - fl(alpha_i Q_i)) / beta_{i+1} with A the
            implementation's own block mat-vec of the downloaded Q_i and the downloaded scalars; Q_0 bit-equal to phi /
            sqrt(norm2); |s - sum t| <= (n + 4) u sum |t| for norm2_j, alpha_i and (plus 2 u sum t) beta_{i+1}^2, the terms in
            longdouble from the mirror's vectors.  Verdict: every error / bound <= 1, a failed bit equality counts as inf.
            ``assert_teeth``: both subtracted terms are at least 2^-10 of max |A| in every judged column.

``Checks(impl)`` drives an implementation (``run(case, p, Phi, k) -> Run`` and ``apply(case, p, X)``) through all of this: the
GPU test hands it the library, the CPU test ``HostImpl(Reference(np.float64, order=...))`` (must pass) and ``HostImpl(mutant)``
for each of ``MUTANTS`` (must fail)."""
import functools
import math

import numpy as np

from cg_reference import bit, same, sum_ratio
from matvec_reference import LD, U, worst_ratio

SENTINEL = -7.0
STEPS_SENTINEL = -77
BREAK_TOL = 1e-13                       # DSEA_BREAK_TOL
UNIT = 2.0 ** 16                        # every term of an exact-class sum is a multiple of 1 / UNIT
WIDTHS = (1, 2, 4, 8)
KS = (1, 2, 3, 4)
TEETH = 2.0 ** -10


# ---- launcher geometry (csrc/dsea_block.h block_blocks, csrc/dsea_device.h sum_partials_block) ------------------------------
def block_blocks(n, grid_log2=None):
    """one block per 256 rows up to the cap 2^tune_tile_log2 (12 at creation)"""
    return min((n + 255) // 256, 1 << (12 if grid_log2 is None else grid_log2))


def partial_reads(count, t):
    """what thread t of sum_partials_block reads: (the loop's reads into a0, the loop's reads into a1, the tail read or None)"""
    a0, a1, b = [], [], t
    while b + 256 < count:
        a0.append(b)
        a1.append(b + 256)
        b += 512
    return a0, a1, (b if b < count else None)


def partial_trips(count):
    """(loop trips of thread 0, threads that make as many, threads with a tail read)"""
    trips = [len(partial_reads(count, t)[0]) for t in range(256)]
    return trips[0], sum(1 for v in trips if v == trips[0]), sum(1 for t in range(256) if partial_reads(count, t)[2] is not None)


# ---- cases ------------------------------------------------------------------------------------------------------------------
class Case:
    """one operator geometry: ``kind`` "sector" (fill = ndown) or "hubbard" (fill = (nup, ndn)); ``grid`` the log2 of the grid
    cap or None for the default"""

    def __init__(self, name, kind, L, fill, grid, bonds):
        self.name, self.kind, self.L, self.fill, self.grid = name, kind, int(L), fill, grid
        self.bonds = tuple((int(a), int(b)) for a, b in bonds)
        self.nb = len(self.bonds)
        if kind == "sector":
            self.n, self.nparam = math.comb(L, fill), 2 * self.nb + L
        else:
            self.n, self.nparam = math.comb(L, fill[0]) * math.comb(L, fill[1]), 2 * self.nb + 2 * L
        self.ranges = (self.n + 255) // 256
        self.nblk = block_blocks(self.n, grid)

    def __repr__(self):
        return self.name

    def apply(self, p, X, dtype=np.float64):
        """H X in ``dtype`` by the numpy twins of the block mat-vec"""
        if self.kind == "sector":
            import sector_block_reference as twin
            return twin.apply_block(self.L, self.fill, self.bonds, p, X, dtype)
        import hubbard_block_reference as twin
        return twin.apply_block(self.L, self.fill[0], self.fill[1], self.bonds, p, X, dtype)

    def scratch_doubles(self, R):
        return 64 + 2 * R * min(4096, self.ranges)

    def hoppers(self, t):
        """per row, the number of species whose two bits differ on bond t (sector: 0 or 1; Hubbard: 0, 1 or 2)"""
        a, b = self.bonds[t]
        if self.kind == "sector":
            import sector_reference
            w = np.array(sector_reference.states(self.L, self.fill), dtype=np.int64)
            return (((w >> a) ^ (w >> b)) & 1).astype(np.int64)
        import hubbard_reference
        wu = np.array(hubbard_reference.states(self.L, self.fill[0]), dtype=np.int64)
        wd = np.array(hubbard_reference.states(self.L, self.fill[1]), dtype=np.int64)
        return ((((wu >> a) ^ (wu >> b)) & 1)[:, None] + (((wd >> a) ^ (wd >> b)) & 1)[None, :]).reshape(-1).astype(np.int64)

    def diag_slots(self):
        """the parameters that enter the diagonal only"""
        return range(self.nb, self.nparam)


class Restricted:
    """A case on a row set that H maps into itself, as a small dense matrix: ``apply`` for blocks that vanish on every other row
    (the break and boundary blocks of the exact class, whose mirror would otherwise pay a full mat-vec per step).  The matrix
    comes from the twin's mat-vec of the basis vectors of those rows, which must stay inside the set."""

    def __init__(self, case, p, rows):
        self.name, self.kind, self.n, self.nblk, self.ranges = case.name, case.kind, case.n, case.nblk, case.ranges
        self.rows = np.array(sorted(int(r) for r in rows), dtype=np.int64)
        X = np.zeros((case.n, self.rows.size))
        X[self.rows, np.arange(self.rows.size)] = 1.0
        Y = case.apply(p, X)
        self.M = Y[self.rows]
        assert np.count_nonzero(Y) == np.count_nonzero(self.M), "the row set is not closed under H"

    def __repr__(self):
        return self.name

    def apply(self, p, X, dtype=np.float64):
        X = np.asarray(X, dtype=dtype)
        inside = X[self.rows]
        assert np.count_nonzero(X) == np.count_nonzero(inside), "the block does not vanish outside the row set"
        Y = np.zeros(X.shape, dtype=dtype)
        Y[self.rows] = self.M.astype(dtype) @ inside + dtype(0.0)          # (+ 0: no negative zero out of a sum of products)
        return Y


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case: the smallest geometries that reach each branch (docs/design/36-block-lanczos-stage-tests.md)"""
    import lattice_reference
    import test_gpu_hubbard
    import test_gpu_sector
    from dominantsparseeigenad_amd.operators import ring_bonds
    out = {}

    def sector(name, L=None, ndown=None, grid=None, bonds=None, source=None):
        if L is None:
            L, ndown, grid, bonds = test_gpu_sector.GEOMETRY[source or name]
        out[name] = Case(name, "sector", L, ndown, grid, bonds)

    def hubbard(name, grid=False, source=None):
        L, nup, ndn, g, bonds = test_gpu_hubbard.GEOMETRY[source or name]
        out[name] = Case(name, "hubbard", L, (nup, ndn), g if grid is False else grid, bonds)

    for name in ("L2-1", "L3-1", "L9-4-cap", "L11-5", "L16-8"):
        sector(name)
    sector("L19-9", 19, 9, None, tuple(ring_bonds(19) + lattice_reference.random_bonds(19, 5, 7219)))
    walk = test_gpu_sector.GEOMETRY["L20-10-walk"]
    sector("L20-10-default", walk[0], walk[1], None, walk[3])
    sector("L20-10-walk")
    sector("L21-8", 21, 8, None, tuple(ring_bonds(21) + lattice_reference.random_bonds(21, 3, 7221)))
    sector("L40-2")
    for name in ("L2-1-1", "L3-1-2", "L6-3-3-loops", "L8-4-4-complete", "L10-5-5-walk"):
        hubbard(name)
    hubbard("L10-5-5-default", grid=None, source="L10-5-5-walk")
    hubbard("L40-2-1")
    return out


ALL = ("L2-1", "L3-1", "L9-4-cap", "L11-5", "L16-8", "L19-9", "L20-10-default", "L20-10-walk", "L21-8", "L40-2",
       "L2-1-1", "L3-1-2", "L6-3-3-loops", "L8-4-4-complete", "L10-5-5-walk", "L10-5-5-default", "L40-2-1")
# the three largest (92378, 184756, 184756 rows) run the random class at R = 1 and R = 8 only; L21-8 (203490 rows: the one
# case with a second loop trip of sum_partials_block) runs both classes at R = 1 and R = 8
THIN = ("L19-9", "L20-10-default", "L20-10-walk", "L21-8")
# coupling seeds of the random class for which assert_teeth holds in every column of every judged step (searched on the CPU
# twin, asserted there and on the device)
RANDOM_SEEDS = {"L9-4-cap": 1, "L11-5": 2, "L19-9": 2, "L20-10-default": 1, "L20-10-walk": 1, "L2-1-1": 1, "L40-2-1": 1}


def widths(name, random):
    if name == "L21-8" or (random and name in THIN):
        return (1, 8)
    return WIDTHS


def support_rows(case, count=16):
    """at least ``count`` rows where n allows: 0, n - 1, both sides of the first and the last 256-row edge, of the first
    grid-stride edge of a capped grid, of the edges at partial 256 and 512 (the second accumulator, the reads past 512 of
    sum_partials_block), then rows inward from both ends"""
    n = case.n
    rows = [0, n - 1]
    last = (n - 1) // 256 * 256
    for e in (256, last, case.nblk * 256, 256 * 256, 512 * 256, 768 * 256):
        rows += [e - 1, e]
    for t in range(1, count):
        rows += [t, n - 1 - t]
    seen, out = set(), []
    for r in rows:
        if 0 <= r < n and r not in seen:
            seen.add(r)
            out.append(r)
    return np.array(out[:max(count, 14)], dtype=np.int64)


# ---- a run ------------------------------------------------------------------------------------------------------------------
class Run:
    """the outputs of one run of k steps: norm2 [R], alphas [k, R], betas [k, R], steps [R] and the two arrays Q, W [n, R] as
    the call leaves them"""

    FIELDS = ("norm2", "alphas", "betas", "steps", "Q", "W")

    def __init__(self, norm2, alphas, betas, steps, Q, W):
        self.norm2, self.alphas, self.betas, self.Q, self.W = (np.asarray(a, dtype=np.float64) for a in (norm2, alphas, betas, Q, W))
        self.steps = np.asarray(steps, dtype=np.int64)
        self.k = self.alphas.shape[0]

    def latest(self):
        """Q_k: in the W array for odd k, in the Q array for even k"""
        return self.W if self.k & 1 else self.Q

    def previous(self):
        """Q_{k-1}, in the other array"""
        return self.Q if self.k & 1 else self.W

    def pick(self, cols):
        cols = list(cols)
        return Run(self.norm2[cols], self.alphas[:, cols], self.betas[:, cols], self.steps[cols], self.Q[:, cols], self.W[:, cols])

    def differences(self, other):
        """the names of the outputs that differ from ``other`` in a bit"""
        bad = [f for f in ("norm2", "alphas", "betas", "Q", "W") if not same(getattr(self, f), getattr(other, f))]
        return bad + ([] if np.array_equal(self.steps, other.steps) else ["steps"])


# ---- the reference ----------------------------------------------------------------------------------------------------------
class Reference:
    """The run in ``dtype``.  Arrays in, a new Run out.  ``order`` (a seed) makes every sum run over a random permutation of
    its terms.  The small methods at the top are the rules a wrong kernel breaks."""

    def __init__(self, dtype=np.float64, order=None):
        self.dtype, self.order, self.case = dtype, order, None

    # -- rules
    def reads_old(self, i):
        """whether step i subtracts fl(beta_i Q_{i-1})"""
        return i >= 1

    def beta_copy(self, i):
        """the copy of the alternating state whose beta step i reads: the one the finish of step i - 1 wrote"""
        return i & 1

    def minus(self, r, s, q):
        """r - fl(s q): the product and the difference are rounded separately"""
        return r - s * q

    def alpha_vector(self, q, old):
        """the block the alpha correction uses (``old``: what the W array held before the step)"""
        return q

    def norm2_of(self, sumsq):
        return sumsq

    def col(self, j, R):
        """the column whose alpha and beta column j is updated with"""
        return j

    def row_weights(self, n):
        """how often a row enters a sum (None: once)"""
        return None

    def stored_beta(self, b, beta):
        """betas[i, j]: ``beta`` is b for a live column and 0 for one that breaks now or is dead"""
        return beta

    def zero_other(self):
        """a column that breaks now is also zeroed in the other array"""
        return True

    def divide(self, v, beta, live):
        return v / beta if live else np.zeros_like(v)

    def survivors(self, live, now):
        """the columns whose vector the finish keeps"""
        return live

    def scale_with_alpha(self, scale, a):
        return np.fmax(scale, a)

    def scale_with_beta(self, scale, b):
        return np.fmax(scale, b)

    def beyond(self, b, bar):
        return b > bar

    def steps_at_start(self, k, old):
        return k

    def writes_steps(self, now, alive):
        return now

    # -- helpers
    def arr(self, a):
        return np.array(a, dtype=self.dtype)

    def sum(self, terms):
        w = self.row_weights(terms.size)
        if w is not None:
            terms = terms * w.astype(self.dtype)
        terms = terms[terms != 0]                   # (a zero term changes no sum; NaN stays)
        if self.order is not None:
            terms = terms[np.random.default_rng(self.order + terms.size).permutation(terms.size)]
        return self.dtype(np.sum(terms))

    def colsums(self, T):
        return np.array([self.sum(T[:, j]) for j in range(T.shape[1])], dtype=self.dtype)

    # -- the kernels
    def finish(self, A, w, other, sumsq, alphas_row, out_row, st_in, st_out, steps, step, k):
        """k_sblock_finish: the break decision, the next copy of the state, array w scaled, a column that breaks now zeroed in
        array ``other``"""
        d = self.dtype
        start = step == 0
        R = sumsq.size
        beta, live, now = np.zeros(R, dtype=d), np.zeros(R, dtype=bool), np.zeros(R, dtype=bool)
        for j in range(R):
            alive = True if start else st_in["alive"][j] != 0
            scale = d(0.0) if start else st_in["scale"][j]
            b = d(0.0)
            if alive:
                if not start:
                    scale = self.scale_with_alpha(scale, abs(alphas_row[j]))
                b = np.sqrt(sumsq[j])
                if not self.beyond(b, d(np.float64(BREAK_TOL)) * scale):
                    now[j] = True
                else:
                    beta[j] = b
                    scale = self.scale_with_beta(scale, b)
            live[j] = alive and not now[j]
            out_row[j] = self.norm2_of(sumsq[j]) if start else self.stored_beta(b, beta[j])
            st_out["beta"][j], st_out["scale"][j], st_out["alive"][j] = beta[j], scale, 1.0 if live[j] else 0.0
            if self.writes_steps(now[j], alive):
                steps[j] = step
            elif start:
                steps[j] = self.steps_at_start(k, steps[j])
        keep = self.survivors(live, now)
        for j in range(R):
            A[w][:, j] = self.divide(A[w][:, j], beta[self.col(j, R)], keep[j])
            if now[j] and other is not None and self.zero_other():
                A[other][:, j] = 0.0

    def run(self, case, p, Phi, k, W0=None, steps0=STEPS_SENTINEL):
        """block_lanczos_drive: -> Run (in ``dtype``; HostImpl rounds to float64)"""
        d = self.dtype
        self.case = case
        Phi = self.arr(Phi)
        n, R = Phi.shape
        A = [Phi, np.full((n, R), np.nan, dtype=d) if W0 is None else self.arr(W0)]
        norm2, alphas, betas = np.zeros(R, dtype=d), np.zeros((k, R), dtype=d), np.zeros((k, R), dtype=d)
        steps = np.full(R, steps0, dtype=np.int64)
        state = [{key: np.full(R, np.nan, dtype=d) for key in ("beta", "scale", "alive")} for _ in range(2)]
        with np.errstate(all="ignore"):
            self.finish(A, 0, None, self.colsums(A[0] * A[0]), None, norm2, None, state[0], steps, 0, k)
            q, w = 0, 1
            for i in range(k):
                W = self.arr(case.apply(p, A[q], d))
                if self.reads_old(i):
                    W = self.minus(W, state[self.beta_copy(i)]["beta"][None, :], A[w])
                alphas[i] = self.colsums(A[q] * W)
                use = alphas[i][[self.col(j, R) for j in range(R)]]
                W = self.minus(W, use[None, :], self.alpha_vector(A[q], A[w]))
                A[w] = W
                self.finish(A, w, q, self.colsums(W * W), alphas[i], betas[i], state[i & 1], state[(i + 1) & 1], steps, i + 1, k)
                q, w = w, q
        out = Run.__new__(Run)
        out.norm2, out.alphas, out.betas, out.steps, out.Q, out.W, out.k = norm2, alphas, betas, steps, A[0], A[1], k
        return out


class Headroom(Reference):
    """fp64 evaluation of an exact-class case that asserts the class's premise on the way: every term of every sum is a
    multiple of 1 / UNIT and sum |terms| UNIT < 2^53, so any partial sum in any order, with or without FMA, is exact; and no
    product or difference of the three-term update is rounded (fp64 == longdouble)"""

    def __init__(self):
        super().__init__(np.float64)
        self.largest = 0.0

    def sum(self, terms):
        scaled = terms[np.isfinite(terms)] * UNIT
        assert np.array_equal(scaled, np.rint(scaled)), "a term is no multiple of 2^-16"
        total = float(np.sum(np.abs(scaled)))
        assert total < 2.0 ** 53, "sum of |terms| is %.3g units of 2^-16: not exact in every order" % total
        self.largest = max(self.largest, total)
        Headroom.largest_met = max(Headroom.largest_met, total)
        return super().sum(terms)

    def minus(self, r, s, q):
        out = super().minus(r, s, q)
        with np.errstate(invalid="ignore"):
            rows = np.nonzero((r != 0).any(axis=1) | (q != 0).any(axis=1))[0]      # (NaN != 0: the unread W array counts)
        exact = np.asarray(r[rows], dtype=LD) - np.asarray(s, dtype=LD) * np.asarray(q[rows], dtype=LD)
        ok = np.isfinite(exact)
        assert np.array_equal(np.asarray(out[rows], dtype=LD)[ok], exact[ok]), "a product or a difference of the update is rounded"
        return out


Headroom.largest_met = 0.0


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def exact_couplings(case, seed=1):
    """multiples of 1/4 in [-2, 2]"""
    return np.random.default_rng(3600 + seed + case.nparam).integers(-8, 9, size=case.nparam).astype(np.float64) / 4.0


def exact_block(case, R, seed=2):
    """integer start columns on support_rows whose squared norm is a power of 4: one entry +-2^m, four entries +-1, sixteen
    entries +-1, in turn (the kinds n has room for)"""
    rng = np.random.default_rng(3600 + seed + case.n + R)
    rows = support_rows(case)
    kinds = [1] + ([4] if rows.size >= 4 else []) + ([16] if rows.size >= 16 else [])
    Phi = np.zeros((case.n, R))
    for j in range(R):
        cnt = kinds[(j + seed) % len(kinds)]
        pick = rows[rng.permutation(rows.size)[:cnt]]
        Phi[pick, j] = rng.choice((-1.0, 1.0), size=cnt) * (2.0 ** int(rng.integers(0, 4)) if cnt == 1 else 1.0)
    return Phi


def random_couplings(case):
    from dominantsparseeigenad_amd.synthetic import normal_vector
    return normal_vector(case.nparam, 36000 + RANDOM_SEEDS.get(case.name, 0) + case.nparam).copy()


def random_block(case, R, seed=36100):
    from dominantsparseeigenad_amd.synthetic import normal_vector
    return np.stack([normal_vector(case.n, seed + case.L + j) for j in range(R)], axis=1)


class BreakData:
    """An operator with ONE hopping bond t0 = bonds[0] (every other Jxy / t is 0) and dyadic diagonal couplings chosen so that
    the two states of a pair have the same diagonal (hz_a = hz_b and no Jz on a bond that shares one site with t0; for Hubbard
    eps_a = eps_b, U_a = U_b = 0 and no V on a bond that touches a or b).  A basis state the bond moves in ONE species has one
    partner, one it does not move has none.  Column kinds:
      Z   zero                                                              breaks at s = 0
      U   2 e_r, r without a partner: W' = 0 exactly                         breaks at s = 1
      P   e_r, r with a partner: Q_1 = +-e_r', W' = 0 at the second step      breaks at s = 2
      PP  e_r1 + e_r1' + e_r2 + e_r2' over two pairs: two eigenvectors with energies E1 != E2, Q_0 = +-1/2, beta_1 =
          |E1 - E2| / 2 and Q_1 = +-1/2 exactly (sums of four terms)         breaks at s = 2
      L   a synthetic.normal_vector column: alive through four steps (not exact: judged against a run without its neighbours)
    A kind the geometry has no state for is replaced by Z (``missing``); below 16 rows there is no L."""

    def __init__(self, case, hop=0.75):
        from dominantsparseeigenad_amd.synthetic import normal_vector
        self.case = case
        a, b = case.bonds[0]
        rng = np.random.default_rng(3650 + case.nparam)
        p = rng.integers(-8, 9, size=case.nparam).astype(np.float64) / 4.0
        p[:case.nb] = 0.0
        p[0] = hop
        nb, L = case.nb, case.L
        for t, (x, y) in enumerate(case.bonds):
            shared = len({x, y} & {a, b})
            if (shared == 1) if case.kind == "sector" else (shared >= 1):
                p[nb + t] = 0.0
        if case.kind == "sector":
            p[2 * nb + b] = p[2 * nb + a]
        else:
            p[2 * nb + a] = p[2 * nb + b] = 0.0
            p[2 * nb + L + b] = p[2 * nb + L + a]
        self.p = p
        hoppers = case.hoppers(0)
        order = np.concatenate([support_rows(case), np.arange(min(case.n, 4096))])
        _, first = np.unique(order, return_index=True)
        order = order[np.sort(first)]
        self.free = [int(r) for r in order if hoppers[r] == 0][:4]
        single = [int(r) for r in order if hoppers[r] == 1][:24]
        self.partner, self.diag = {}, {}
        if single:
            X = np.zeros((case.n, len(single)))
            X[single, range(len(single))] = 1.0
            Y = case.apply(p, X)
            for j, r in enumerate(single):
                self.diag[r] = float(Y[r, j])
                (others,) = np.nonzero(np.where(np.arange(case.n) == r, 0.0, Y[:, j]))
                assert others.size == 1
                self.partner[r] = (int(others[0]), float(Y[others[0], j]))
        self.paired = [r for r in single if r in self.partner]
        # two pairs with different energies d + h (h the coupling to the partner), four distinct rows
        self.quads = []
        used = set()
        for r1 in self.paired:
            for r2 in self.paired:
                rows = {r1, self.partner[r1][0], r2, self.partner[r2][0]}
                if len(rows) == 4 and not rows & used and self.diag[r1] + self.partner[r1][1] != self.diag[r2] + self.partner[r2][1]:
                    self.quads.append((r1, self.partner[r1][0], r2, self.partner[r2][0]))
                    used |= rows
                    break
        closed = set(self.free) | set(self.paired) | {self.partner[r][0] for r in self.paired}
        self.fast = Restricted(case, p, closed) if closed else case
        self.live = [normal_vector(case.n, 36500 + j) for j in range(3)]
        # (a live column needs five distinct levels under its feet: from 16 rows on)
        self.missing = [kind for kind, have in (("U", self.free), ("P", self.paired), ("PP", self.quads), ("L", case.n >= 16)) if not have]

    def block(self, kinds):
        """(Phi, the kinds actually used): a kind without a state becomes Z; repeated kinds take different states"""
        n = self.case.n
        Phi = np.zeros((n, len(kinds)))
        seen = {"U": 0, "P": 0, "PP": 0, "L": 0}
        used = []
        for j, kind in enumerate(kinds):
            if kind in self.missing:
                kind = "Z"
            if kind == "U":
                Phi[self.free[seen[kind] % len(self.free)], j] = 2.0
            elif kind == "P":
                Phi[self.paired[(2 * seen[kind]) % len(self.paired)], j] = -1.0 if seen[kind] & 1 else 1.0
            elif kind == "PP":
                Phi[list(self.quads[seen[kind] % len(self.quads)]), j] = 1.0
            elif kind == "L":
                Phi[:, j] = self.live[seen[kind] % len(self.live)]
            if kind != "Z":
                seen[kind] += 1
            used.append(kind)
        return Phi, tuple(used)

    def expected_steps(self, kinds, k):
        return [min(k, {"Z": 0, "U": 1, "P": 2, "PP": 2, "L": k}[kind]) for kind in kinds]


BREAK_BLOCKS = {1: (("Z",), ("U",), ("P",), ("PP",)), 2: (("U", "P"), ("Z", "PP"), ("P", "L")),
                4: (("Z", "U", "P", "L"), ("PP", "L", "U", "P")), 8: (("Z", "U", "P", "PP", "L", "U", "P", "L"),)}
ALL_BREAK = {R: tuple(("Z", "U", "P", "PP")[(j + 1) % 4] for j in range(R)) for R in WIDTHS}


@functools.lru_cache(maxsize=None)
def break_data(name):
    return BreakData(cases()[name])


def strict_inputs(case, which, above):
    return _strict_inputs(case.name, which, above)


@functools.lru_cache(maxsize=None)
def _strict_inputs(name, which, above):
    """One two-level column of the strict boundary (docs/design/36-block-lanczos-stage-tests.md): phi = norm e_r with r a row
    with a partner, the only non-zero diagonal coupling set so that alpha_0 = H_rr = diag, 2 Jxy (Hubbard: t) = c.  beta_1 =
    sqrt(fl(c c)) = c and the scale at the test is max(norm, |diag|).  which: "both" (norm = diag = 1), "beta" (norm = 2: the
    largest earlier quantity is beta_0), "alpha" (diag = 2: it is the current alpha).  c = fl(1e-13 scale), or with ``above``
    the next double: the first must break at s = 1, the second must not (and breaks at s = 2, where W' = 0).
    -> (p, phi (n,), c, the operator restricted to the pair) or None when the geometry has no such row"""
    case, data = cases()[name], break_data(name)
    if not data.paired:
        return None
    r = data.paired[0]
    norm, diag = {"both": (1.0, 1.0), "beta": (2.0, 1.0), "alpha": (1.0, 2.0)}[which]
    c = np.float64(BREAK_TOL) * max(norm, diag)
    if above:
        c = np.nextafter(c, np.inf)
    p = np.zeros(case.nparam)
    p[0] = c / 2.0 if case.kind == "sector" else c
    e = np.zeros((case.n, 1))
    e[r, 0] = 1.0
    for slot in case.diag_slots():              # a diagonal coupling whose coefficient at row r is +-1
        unit = np.zeros(case.nparam)
        unit[slot] = 1.0
        coef = float(case.apply(unit, e)[r, 0])
        if abs(coef) == 1.0:
            p[slot] = diag * coef
            break
    else:
        return None
    fast = Restricted(case, p, (r, data.partner[r][0]))
    assert float(fast.apply(p, e)[r, 0]) == diag
    return p, norm * e[:, 0], float(c), fast


# ---- judges of the random class (on the run's own inputs and outputs; return {name: error / bound}) -------------------------
def _ld(a):
    return np.asarray(a, dtype=LD)


def judge_start(Phi, norm2, Q0):
    n, R = Phi.shape
    with np.errstate(all="ignore"):
        out = {"Q_0": bit(Q0, np.asarray(Phi, dtype=np.float64) / np.sqrt(np.asarray(norm2, dtype=np.float64))[None, :])}
    P = _ld(Phi)
    out["norm2"] = max(sum_ratio(norm2[j], P[:, j] * P[:, j], n) for j in range(R))
    return out


def mirror_step(i, A, Qprev, Qi, alpha, beta):
    """(W, W') of step i in fp64 from the implementation's own A = H Q_i and scalars"""
    W = np.asarray(A, dtype=np.float64)
    if i >= 1:
        W = W - np.asarray(beta, dtype=np.float64)[None, :] * Qprev
    return W, W - np.asarray(alpha, dtype=np.float64)[None, :] * Qi


def teeth(i, A, Qprev, Qi, alpha, beta):
    """per column, the smaller of max |fl(beta_i Q_{i-1})| and max |fl(alpha_i Q_i)| over max |A| (the first at i >= 1 only)"""
    top = np.max(np.abs(A), axis=0)
    out = np.max(np.abs(np.asarray(alpha)[None, :] * Qi), axis=0) / top
    if i >= 1:
        out = np.minimum(out, np.max(np.abs(np.asarray(beta)[None, :] * Qprev), axis=0) / top)
    return out


def assert_teeth(tag, i, A, Qprev, Qi, alpha, beta):
    """the premise of the random class: both subtracted terms are of the size of H Q_i in every column, so a dropped, doubled
    or contracted term moves Q_{i+1} by far more than one rounding"""
    t = teeth(i, A, Qprev, Qi, alpha, beta)
    assert (t >= TEETH).all(), "%s step %d: a subtracted term is only %.3g of max |A| (floor 2^-10)" % (tag, i, float(t.min()))
    return float(t.min())


def judge_step(i, A, Qprev, Qi, Qnext, alpha, beta, beta_next):
    """step i from A = H Q_i (the implementation's own block mat-vec of the downloaded Q_i), the downloaded Q_{i-1}, Q_i,
    Q_{i+1}, alpha_i (alphas[i]), beta_i (betas[i - 1]) and beta_{i+1} (betas[i])"""
    n, R = Qi.shape
    W, W2 = mirror_step(i, A, Qprev, Qi, alpha, beta)
    with np.errstate(all="ignore"):
        out = {"Q_next": bit(Qnext, W2 / np.asarray(beta_next, dtype=np.float64)[None, :])}
    Ql, Wl, W2l = _ld(Qi), _ld(W), _ld(W2)
    out["alpha"] = max(sum_ratio(alpha[j], Ql[:, j] * Wl[:, j], n) for j in range(R))
    worst = 0.0
    for j in range(R):
        T = np.sum(W2l[:, j] * W2l[:, j])
        worst = max(worst, worst_ratio(abs(LD(beta_next[j]) ** 2 - T), float(((n + 4) * U + 2 * U) * T)))
    out["beta"] = worst
    return out


# ---- the checks: one implementation of the run through both classes ---------------------------------------------------------
class Checks:
    """``impl.run(case, p, Phi, k, fast=None) -> Run`` is one run on a W array full of NaN, ``impl.apply(case, p, X)`` one block
    mat-vec (``fast``: the Restricted operator of a block that lives on a few rows, for an implementation on the host).
    Every check raises AssertionError where a verdict fails; ``random`` returns the worst ratio per quantity."""

    def __init__(self, impl, log=print, prove=True):
        self.impl, self.log, self.prove, self.mirror = impl, log, prove, Reference(np.float64)
        self.cases = 0                      # verdicts given
        self.worst = {}                     # quantity -> (worst error / bound of the random class, where)

    # -- verdicts
    def exact(self, tag, got, want, cols=None):
        self.cases += 1
        if cols is not None:
            got = got.pick(cols)
        bad = got.differences(want)
        assert not bad, "%s: %s differ from the fp64 reference (exact class): got steps %s, want %s" % (tag, bad, got.steps, want.steps)

    def ratios(self, tag, res):
        self.cases += 1
        bad = {k: v for k, v in res.items() if not v <= 1.0}
        assert not bad, "%s: %s" % (tag, bad)
        for k, v in res.items():
            if v >= self.worst.get(k, (-1.0, ""))[0]:
                self.worst[k] = (float(v), tag)
        return max(res.values()) if res else 0.0

    def headroom(self, case, p, Phi, k):
        """the fp64 reference of an exact-class run, its premise asserted on the way; with ``prove`` also fp64 == longdouble on
        every output before the first square root (norm2, alpha_0)"""
        want = Headroom().run(case, p, Phi, k)
        if self.prove and case.n <= 1 << 14:
            hi = Reference(LD).run(case, p, Phi, 1)
            assert np.array_equal(_ld(want.norm2), hi.norm2) and np.array_equal(_ld(want.alphas[0]), hi.alphas[0]), case
        return _f64(want)

    # -- exact class
    def first_step(self, case, R):
        """k = 1 on exact data: norm2, Q_0 (the Q array), alphas[0], betas[0], Q_1 (the W array) and steps, bit for bit; at
        small sizes with three different draws"""
        for seed in (2, 3, 4) if case.n <= 4096 else (2,):
            p, Phi = exact_couplings(case, seed), exact_block(case, R, seed)
            want = self.headroom(case, p, Phi, 1)
            self.exact("%s R=%d k=1 seed=%d" % (case, R, seed), self.impl.run(case, p, Phi, 1), want)

    def breaks(self, case, R, ks=KS):
        """blocks whose columns break at s = 0, 1 and 2 beside columns that live, at every run length: the exact columns bit
        for bit in every output; the live ones bit-identical to a run in which their neighbours are zero columns"""
        data = break_data(case.name)
        for kinds in BREAK_BLOCKS[R]:
            Phi, used = data.block(kinds)
            hard = [j for j, kind in enumerate(used) if kind != "L"]
            soft = [j for j, kind in enumerate(used) if kind == "L"]
            for k in ks:
                want = self.headroom(data.fast, data.p, Phi[:, hard], k)
                assert want.steps.tolist() == data.expected_steps([used[j] for j in hard], k), (case, used, k, want.steps)
                got = self.impl.run(case, data.p, Phi, k, fast=data.fast)
                self.exact("%s R=%d k=%d break block %s" % (case, R, k, "-".join(used)), got, want, cols=hard)
                if soft and k == ks[-1]:
                    alone = Phi.copy()
                    alone[:, hard] = 0.0
                    assert got.steps[soft].tolist() == [k] * len(soft), (case, used, got.steps)
                    self.exact("%s R=%d k=%d live columns beside breaking ones" % (case, R, k), got,
                               self.impl.run(case, data.p, alone, k).pick(soft), cols=soft)

    def all_break(self, case, R, k=4):
        """every column breaks: both arrays come back zero, every output finite"""
        data = break_data(case.name)
        Phi, used = data.block(ALL_BREAK[R])
        want = self.headroom(data.fast, data.p, Phi, k)
        got = self.impl.run(case, data.p, Phi, k, fast=data.fast)
        self.exact("%s R=%d k=%d every column breaks (%s)" % (case, R, k, "-".join(used)), got, want)
        assert not got.Q.any() and not got.W.any() and (got.steps < k).all()
        assert all(np.isfinite(a).all() for a in (got.norm2, got.alphas, got.betas))

    def strict(self, case, R):
        """the boundary of ``not beta > 1e-13 scale``, with the scale in beta_0 and alpha_0 alike, in beta_0, in alpha_0: at
        equality the column breaks at s = 1 (betas[0] = 0), one ulp above it does not (betas[0] = c) and breaks at s = 2;
        the column sits in the last column of the block beside zero columns.  Returns False if the geometry has no pair."""
        for which in ("both", "beta", "alpha"):
            for above in (False, True):
                made = strict_inputs(case, which, above)
                if made is None:
                    return False
                p, phi, c, fast = made
                Phi = np.zeros((case.n, R))
                Phi[:, R - 1] = phi
                want = _f64(self.mirror.run(fast, p, Phi, 2))
                assert want.steps[R - 1] == (2 if above else 1) and want.betas[0, R - 1] == (c if above else 0.0), (which, above)
                self.exact("%s R=%d strict boundary, scale in %s, %s" % (case, R, which, "one ulp above" if above else "at equality"),
                           self.impl.run(case, p, Phi, 2, fast=fast), want)
        return True

    def nan_column(self, case, R, k=3):
        """a NaN start column beside live ones: steps = 0, zero in both arrays, alphas and betas 0, norm2 NaN; every other
        column bit-identical to the run in which that column is zero"""
        p, Phi = random_couplings(case), random_block(case, R)
        k = min(k, max(case.n - 1, 1))
        j = R // 2
        clean = Phi.copy()
        clean[:, j] = 0.0
        Phi[:, j] = np.nan
        got, base = self.impl.run(case, p, Phi, k), self.impl.run(case, p, clean, k)
        self.cases += 1
        assert got.steps[j] == 0 and np.isnan(got.norm2[j]) and base.norm2[j] == 0.0 and base.steps[j] == 0
        assert not got.Q[:, j].any() and not got.W[:, j].any() and not got.alphas[:, j].any() and not got.betas[:, j].any()
        others = [c for c in range(R) if c != j]
        bad = got.pick(others).differences(base.pick(others))
        assert not bad, "%s R=%d: a NaN column changed %s of its neighbours" % (case, R, bad)

    def beyond_n(self, case, R):
        """k = n + 2 on random data (n = 2, 3): the Krylov space is exhausted at step n.  The mirror decides the steps; the run
        must agree wherever the float64 and the longdouble reference agree.  After the break the column is zero in both
        arrays, its later alphas and betas are 0, everything is finite."""
        k = case.n + 2
        p, Phi = random_couplings(case), random_block(case, R)
        lo, hi = self.mirror.run(case, p, Phi, k), Reference(LD).run(case, p, Phi, k)
        got = self.impl.run(case, p, Phi, k)
        self.cases += 1
        agree = lo.steps == hi.steps
        assert np.array_equal(got.steps[agree], lo.steps[agree]), (case, R, got.steps, lo.steps, hi.steps)
        assert all(np.isfinite(a).all() for a in (got.norm2, got.alphas, got.betas, got.Q, got.W))
        for j in range(R):
            s = int(got.steps[j])
            if s < k:
                assert not got.Q[:, j].any() and not got.W[:, j].any() and not got.alphas[s:, j].any() and not got.betas[max(s - 1, 0):, j].any()
        return agree

    def exact_class(self, case, R):
        self.first_step(case, R)
        self.breaks(case, R)
        self.all_break(case, R)
        self.strict(case, R)
        self.nan_column(case, R)
        if case.n <= 3:
            self.beyond_n(case, R)

    # -- random class
    def random(self, case, R, kmax=4):
        """runs of k = 1 ... min(kmax, n - 1) steps on one start block: the prefix rule and where Q_k lies, then the start and
        every step judged on the runs' own blocks and scalars"""
        p, Phi = random_couplings(case), random_block(case, R)
        kmax = min(kmax, case.n - 1)
        runs = {k: self.impl.run(case, p, Phi, k) for k in range(1, kmax + 1)}
        for k in range(1, kmax + 1):
            assert runs[k].steps.tolist() == [k] * R, (case, R, k, runs[k].steps)
        for k in range(1, kmax):
            a, b = runs[k], runs[k + 1]
            self.ratios("%s R=%d prefix rule k=%d" % (case, R, k),
                        {"prefix": max(bit(a.norm2, b.norm2), bit(a.alphas, b.alphas[:k]), bit(a.betas, b.betas[:k]),
                                       bit(a.latest(), b.previous()))})
        Qs = [runs[1].previous()] + [runs[k].latest() for k in range(1, kmax + 1)]
        last = runs[kmax]
        worst = self.ratios("%s R=%d start" % (case, R), judge_start(Phi, last.norm2, Qs[0]))
        for i in range(kmax):
            A = self.impl.apply(case, p, Qs[i])
            beta = last.betas[i - 1] if i else None
            assert_teeth("%s R=%d" % (case, R), i, A, Qs[i - 1] if i else None, Qs[i], last.alphas[i], beta)
            res = judge_step(i, A, Qs[i - 1] if i else None, Qs[i], Qs[i + 1], last.alphas[i], beta, last.betas[i])
            worst = max(worst, self.ratios("%s R=%d step %d" % (case, R, i), res))
        self.log("%s R=%d: random class, %d steps, worst error / bound = %.3f" % (case, R, kmax, worst))
        return worst

    def twice(self, case, R, k=3):
        p, Phi = random_couplings(case), random_block(case, R)
        k = min(k, max(case.n - 1, 1))
        a, b = self.impl.run(case, p, Phi, k), self.impl.run(case, p, Phi, k)
        self.cases += 1
        assert not a.differences(b), "%s R=%d: two identical calls differ in %s" % (case, R, a.differences(b))


def _f64(run):
    return Run(run.norm2, run.alphas, run.betas, run.steps, run.Q, run.W)


# ---- wrong kernels: each breaks one rule of Reference -----------------------------------------------------------------------
def _mutant(name, **methods):
    return type(name, (Reference,), methods)


def _fma(self, r, s, q):
    return np.asarray(np.asarray(r, dtype=LD) - np.asarray(s, dtype=LD) * np.asarray(q, dtype=LD), dtype=self.dtype)


def _layout(self, n):
    """(row range, block) of every row"""
    rng = np.arange(n) // 256
    return rng, rng % self.case.nblk


def _drop_last_block(self, n):
    _, blk = _layout(self, n)
    return (blk != self.case.nblk - 1).astype(np.float64)


def _drop_second_accumulator(self, n):
    _, blk = _layout(self, n)
    count = self.case.nblk
    lost = np.zeros(count, dtype=bool)
    for t in range(256):
        lost[partial_reads(count, t)[1]] = True
    return (~lost[blk]).astype(np.float64)


def _drop_past_512(self, n):
    _, blk = _layout(self, n)
    return (blk < 512).astype(np.float64)


def _acc_reset(self, n):
    rng, _ = _layout(self, n)
    return (rng + self.case.nblk >= self.case.ranges).astype(np.float64)


def _idle_threads_add(self, n):
    w = np.ones(n)
    w[n - 1] += self.case.ranges * 256 - n
    return w


def _block_dies(self, live, now):
    return np.zeros_like(live) if now.any() else live


MUTANTS = {
    "the beta term is dropped": _mutant("NoBetaTerm", reads_old=lambda self, i: False),
    "the beta term is applied on the first step": _mutant("BetaTermAtZero", reads_old=lambda self, i: True),
    "beta_i is taken from the other state copy": _mutant("OtherCopy", beta_copy=lambda self, i: (i + 1) & 1),
    "the alpha correction is taken from Q_{i-1}": _mutant("AlphaFromOld", alpha_vector=lambda self, q, old: old),
    "product and difference are contracted into an FMA": _mutant("Contracted", minus=_fma),
    "norm2 reports the root": _mutant("NormRoot", norm2_of=lambda self, sumsq: np.sqrt(sumsq)),
    "column j uses the alpha and beta of column j ^ 1": _mutant("NeighbourColumn", col=lambda self, j, R: j ^ 1 if R > 1 else j),
    "the last block's partial is dropped": _mutant("LastPartial", row_weights=_drop_last_block),
    "the second accumulator of the partial sum is dropped": _mutant("SecondAccumulator", row_weights=_drop_second_accumulator),
    "the partials from 512 on are dropped": _mutant("Past512", row_weights=_drop_past_512),
    "acc is reset on every row range of the walk": _mutant("AccReset", row_weights=_acc_reset),
    "a thread past the last row adds row n - 1 again": _mutant("IdleThreads", row_weights=_idle_threads_add),
    "the breaking beta is stored non-zero": _mutant("BreakingBeta", stored_beta=lambda self, b, beta: b),
    "a breaking column is left alive in the other array": _mutant("OtherKept", zero_other=lambda self: False),
    "a dead column is divided by its zero beta": _mutant("DeadDivided", divide=lambda self, v, beta, live: v / beta),
    "one break zeroes the whole block": _mutant("BlockDies", survivors=_block_dies),
    "the scale lacks the current alpha": _mutant("NoAlphaInScale", scale_with_alpha=lambda self, scale, a: scale),
    "the scale lacks the betas": _mutant("NoBetaInScale", scale_with_beta=lambda self, scale, b: scale),
    ">= in place of >": _mutant("NotStrict", beyond=lambda self, b, bar: b >= bar),
    "steps is not set to k at the start": _mutant("StepsNotSet", steps_at_start=lambda self, k, old: old),
    "steps of a dead column is overwritten later": _mutant("StepsOverwritten", writes_steps=lambda self, now, alive: now or not alive),
}


class HostImpl:
    """a Reference behind the interface Checks drives (what the GPU test's implementation offers around the library)"""

    def __init__(self, ref):
        self.ref = ref

    def run(self, case, p, Phi, k, fast=None):
        if isinstance(fast, Restricted) and np.count_nonzero(Phi) == np.count_nonzero(Phi[fast.rows]):
            case = fast
        return _f64(self.ref.run(case, p, Phi, k))

    def apply(self, case, p, X):
        return np.asarray(case.apply(p, X, np.float64), dtype=np.float64)
