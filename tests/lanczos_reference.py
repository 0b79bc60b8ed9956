"""numpy references, input classes, error bounds, judges and checks of the Lanczos stage tests
(tests/test_gpu_lanczos_stages.py, proved on the CPU by tests/test_lanczos_reference_cpu.py); no GPU, no torch.
docs/design/29-lanczos-stage-tests.md tells the same story at length.

``Reference(dtype)`` evaluates every stage of the symmetric Lanczos step of include/dsea.h (reference Lanczos.py:60-75, 99-105) in
``dtype``: np.longdouble is the high-precision reference, np.float64 the MIRROR (the kernels round every product and difference
of the three-term update separately -- __dmul_rn / __dsub_rn, -ffp-contract=off -- and so does numpy), np.float64 with ``order``
an honest fp64 evaluation whose sums run over a random permutation.  The basis is an array of ROWS (vector j = Q[j], as the
library stores it).

  rdots            r = (u - fl(a q_{i-1})) - fl(b q_{i-2}) (no q_{i-2} term at i = 1 or with b None); c_j = q_j . r (j < i);
                   c_i = r . r from r BEFORE any correction
  axpy_norm        r' = r - sum_{j<i} c_j q_j for the c it is given; nrm2 = r' . r'
  ritz             out = sum_{j<k} s_j q_j
  store            beta = sqrt(nrm2); Q[row] = r / beta  (scale_store: the same into a vector)
  callable_alpha   alpha = q . u
  callable_step    alphas[i-1] = q_{i-1} . u; rdots with it and betas[i-2]; axpy_norm with c = Q r; betas[i-1] = sqrt(r' . r');
                   Q[i] = r' / betas[i-1]
  partial_step     the three-term r and rr = r . r; the omega row of k_pro_update in the kernel's own operation order; on a
                   selected step c = Q r and r' = r - Q^T c, nrm2 = r' . r'; on a skipped one r stays and nrm2 = rr

TWO INPUT CLASSES, TWO VERDICTS

  exact     Q has integer entries in [-2, 2] (no orthonormality: the kernels compute the formula whatever Q is), u integer
            entries in [-4, 4], a = 0.75, b = -1.25, supplied coefficients multiples of 1/2: r is a multiple of 1/4, every term
            of a c_j too, every term of r . r a multiple of 1/16.  Where c is hidden and feeds a sum of squares (callable_step,
            a selected partial_step) Q lives on ``support_rows(n)`` (row 0, row n - 1, both sides of tile edges), so that
            ||r'||^2 stays in range.  ``Headroom`` asserts for every sum of every case that sum |terms| < 2^53 / 16.  beta =
            sqrt(nrm2) and q = r' / beta are single correctly rounded operations that numpy reproduces.  Verdict: EVERY output
            equals Reference(np.float64) bit for bit; for partial_step also anorm, the counter and every decision.
  random    synthetic.normal_vector data, Q orthonormal rows built in longdouble and rounded once (krylov_reference.random_rows),
            u = Q^T g + noise with |g_j| in [1, 2] so that the coefficients are O(1) (the builder asserts it).  Each stage is
            judged on the call's own inputs and outputs, u = 2^-53:
              bit equality with the fp64 mirror     r of rdots / callable_step (with the downloaded alphas[i-1]) / partial_step;
                                                    Q[i] from the downloaded r' and beta; beta = sqrt(nrm2)
              |s - sum t| <= (n + 4) u sum |t|       c_j, c_i, nrm2, alpha (t from the call's own vectors, in longdouble)
              visible c:  |r'_k - (r_k - sum_j c_j q_jk)| <= u |r'_k| + (i + 17) u sum_j |c_j q_jk|      (ritz: without u |out_k|)
              hidden c:   c^ = Q r in longdouble, E_j = (n + 4) u sum_k |q_jk r_k|; the bound gains sum_j E_j |q_jk| and |c_j|
                          becomes |c^_j| + E_j
              fused beta: |beta^2 - sum r'^2| <= ((n + 4) u + 2 u) sum r'^2
            No constant is fitted to a device.  Verdict: every ratio error / bound <= 1 (a bit inequality counts as inf).

``Checks(impl)`` drives an implementation of the stages through all of this: the GPU test hands it the library, the CPU test
``HostImpl(Reference(np.float64, order=...))`` (must pass) and ``HostImpl(mutant)`` for each of ``MUTANTS`` (must fail)."""
import contextlib

import numpy as np

from cg_reference import bit, same, sum_ratio
from matvec_reference import LD, U, worst_ratio

SENTINEL = -7.0
UNIT = 16.0                             # every term of an exact-class sum is a multiple of 1 / UNIT
A_EXACT, B_EXACT = 0.75, -1.25
A_RANDOM, B_RANDOM = 0.6180339887498949, -0.3183098861837907
EPS1 = 64.0 * 2.220446049250313e-16     # k_pro_update's rounding unit of the omega recurrence (2^-46)
TILE, MAX_WAVES = 128, 8192             # rows of a split-form tile (and of a wave tile at rpl 2); DSEA_MAX_WAVE_TILES
KMAX = 8000                             # DSEA_MAX_KRYLOV

SIZES_SPLIT16 = (1, 2, 3, 127, 129, 4097)          # one tile with guarded loads; several tiles with an odd last row
SIZE_SPLIT8 = 32897
SIZES_NT2 = (82049, 82177)                         # 642 / 643 tiles: the last block's second sub-tile holds one row / is empty
SIZES_WAVE = (131202, 262146, 524290, (1 << 20) + 2)      # wave-owned, rpl 2 / 4 / 8 / 16 automatic
SIZES_RPL2_SMALL = (129, 300)                      # set_rows_per_lane(2): one block whose last waves own no tile
SIZE_GRID_STRIDE = (1 << 20) + 129                 # set_rows_per_lane(2): 8194 tiles > 8192 waves
SIZES_FINALIZE = (128 * 800 + 1, 128 * 1800 + 1)   # set_split(16): 801 / 1801 partials per coefficient
STEPS_REV = (1, 2, 3, 4, 5, 7, 8)                  # both parities with and without remainder vectors
STEPS_LDS = (2047, 2048, 4095, 4096, 7999)         # four / two / one waves per block; 64 KiB, 64 KiB and 64 000 bytes of LDS
STEPS_LDS_SPLIT = (2047, 4096)


# ---- launcher geometry (csrc/dsea_capi.hip Workspace::geom, csrc/dsea_lanczos_kernels.hip) ----------------------------------
def geom(n, rpl=0, split=-1):
    """what Workspace::geom selects: dict(rpl, ntiles, nw, split_w, dots_w, dots_nt)"""
    r = rpl
    if r not in (2, 4, 8, 16):
        r = 16 if n >= 64 * 16 * 1024 else 8 if n >= 64 * 8 * 1024 else 4 if n >= 64 * 4 * 1024 else 2
    ntiles = max((n + 64 * r - 1) // (64 * r), 1)
    g = dict(rpl=r, ntiles=ntiles, nw=min(ntiles, MAX_WAVES), split_w=0, dots_w=0, dots_nt=1)
    tiles128 = (n + 127) // 128
    sw = split
    if sw < 0 and rpl == 0:
        sw = 16 if tiles128 <= 256 else 8 if tiles128 <= 1024 else 0
    if sw in (4, 8, 16):
        g.update(split_w=sw, rpl=2, ntiles=tiles128, nw=tiles128, dots_w=sw)
        if split < 0 and tiles128 > 640:
            g.update(dots_w=16, dots_nt=2)
    return g


def rdots_waves_per_block(i):
    return 4 if i + 1 <= 2048 else 2 if i + 1 <= 4096 else 1


def rdots_lds_bytes(n, i, rpl=0, split=-1):
    g = geom(n, rpl, split)
    return (i + 1) * 8 if g["split_w"] else rdots_waves_per_block(i) * (i + 1) * 8


def rdots_partials(n, i, rpl=0, split=-1):
    g = geom(n, rpl, split)
    if g["split_w"]:
        return (g["ntiles"] + g["dots_nt"] - 1) // g["dots_nt"]
    w = rdots_waves_per_block(i)
    return (g["nw"] + w - 1) // w


def finalize_trips(count):
    """(four-accumulator trips of k_finalize_multi's thread 0, tail reads of thread 0)"""
    w, trips = 0, 0
    while w + 768 < count:
        w += 1024
        trips += 1
    return trips, len(range(w, count, 256))


def support_rows(n, count=16):
    """up to ``count`` rows: 0, n - 1, then both sides of the LAST and the FIRST edge of every tile size of the streaming
    kernels (128 ... 1024 rows, 256 for the two-sub-tile block), of the 512-row stride of the elementwise kernels and of the
    grid stride of the capped wave-owned form"""
    rows = [0, n - 1]
    for t in (128, 256, 512, 1024, 2048, MAX_WAVES * 128):
        last = (n - 1) // t * t
        rows += [last - 1, last, t - 1, t]
    seen, out = set(), []
    for r in rows:
        if 0 <= r < n and r not in seen:
            seen.add(r)
            out.append(r)
    return np.array(sorted(out[:count]), dtype=np.int64)


# ---- the stages -------------------------------------------------------------------------------------------------------------
class ProState:
    """what a workspace carries from one dsea_lanczos_partial_step to the next"""

    def __init__(self, rows=KMAX + 1):
        self.om = np.full((2, rows), np.nan)
        self.next_too, self.anorm, self.count = 0.0, 0.0, 0.0


class Reference:
    """Every stage in ``dtype``.  Arrays in, new arrays out (nothing is modified in place).  ``order`` (a seed) makes every sum
    run over a random permutation of its terms.  The small methods at the top are the rules a wrong kernel breaks: MUTANTS
    overrides them one at a time."""

    def __init__(self, dtype=np.float64, order=None):
        self.dtype, self.order = dtype, order

    # -- rules
    def terms3(self, i, a, b):
        """which basis rows enter the three-term update, with which scalar"""
        return [(i - 1, a)] + ([(i - 2, b)] if i >= 2 and b is not None else [])

    def minus(self, r, s, q):
        """r - fl(s q): the product and the difference are rounded separately"""
        return r - s * q

    def dots_see(self, u, r):
        return r

    def dotted(self, i):
        return range(i)

    def slot(self, i, j):
        return j

    def rr_sees(self, r, corrected):
        """the vector whose square is c_i / rr (``corrected()``: r after the correction)"""
        return r

    def sum(self, terms):
        if self.order is not None:
            terms = terms[np.random.default_rng(self.order + terms.size).permutation(terms.size)]
        return self.dtype(np.sum(terms))

    def store(self, old, new):
        """what a kernel leaves in an n-row buffer that held ``old``"""
        return new

    def corrected(self, i):
        return range(i)

    def coef(self, c, j):
        return c[j]

    def norm_sees(self, r, r2):
        return r2

    def beta_of(self, nrm2):
        return np.sqrt(nrm2)

    def q_row(self, row):
        return row

    def writes_alpha(self):
        return True

    def skip_r(self, r, corrected):
        """what a skipped step leaves in r"""
        return r

    def skip_nrm2(self, rr):
        return rr

    def selected(self, trig, forced):
        return trig or forced

    def triggers(self, mx, delta):
        return not (mx <= delta)

    def reset(self, row, i):
        row[:i] = EPS1

    def anorm_of(self, prev, cand):
        return max(prev, cand)

    def counts(self, selected):
        return selected

    def restart(self, st):
        st.next_too, st.anorm, st.count = 0.0, 0.0, 0.0

    # -- helpers
    def arr(self, a):
        return np.array(a, dtype=self.dtype)

    def dot(self, x, y):
        return self.sum(self.arr(x) * self.arr(y))

    def three_term(self, Q, i, u, a, b):
        r = self.arr(u)
        for row, s in self.terms3(i, a, b):
            r = self.minus(r, self.dtype(s), self.arr(Q[row]))
        return r

    def combine(self, Q, i, c):
        """sum_j c_j q_j over the rows the correction uses (an FMA chain in the kernels; here one rounded product and one
        rounded sum per vector, in ``order``)"""
        js = list(self.corrected(i))
        if self.order is not None:
            js = [js[p] for p in np.random.default_rng(self.order + i).permutation(len(js))]
        w = np.zeros(np.shape(Q)[1], dtype=self.dtype)
        for j in js:
            w = w + self.dtype(self.coef(c, j)) * self.arr(Q[j])
        return w

    def dots(self, Q, i, v):
        c = np.zeros(i + 1, dtype=self.dtype)
        for j in self.dotted(i):
            c[self.slot(i, j)] = self.dot(Q[j], v)
        return c

    # -- phases
    def rdots(self, Q, i, u, a, b):
        r = self.three_term(Q, i, u, a, b)
        c = self.dots(Q, i, self.dots_see(self.arr(u), r))
        v = self.rr_sees(r, lambda: r - self.combine(Q, i, c))
        c[i] = self.dot(v, v)
        return self.store(np.full(r.size, SENTINEL, dtype=self.dtype), r), c

    def axpy_norm(self, Q, i, c, r):
        r = self.arr(r)
        r2 = self.store(r, r - self.combine(Q, i, self.arr(c)))
        v = self.norm_sees(r, r2)
        return r2, self.dot(v, v)

    def ritz(self, Q, k, s):
        w = self.combine(Q, k, self.arr(s))
        return self.store(np.full(w.size, SENTINEL, dtype=self.dtype), w)

    def store_row(self, r, nrm2, Q, row, with_beta=True):
        beta = self.beta_of(self.dtype(nrm2))
        Qn = self.arr(Q)
        t = self.q_row(row)
        Qn[t] = self.store(Qn[t], self.arr(r) / beta)
        return Qn, (beta if with_beta else None)

    def scale_store(self, r, nrm2, with_beta=True):
        beta = self.beta_of(self.dtype(nrm2))
        r = self.arr(r)
        return self.store(np.full(r.size, SENTINEL, dtype=self.dtype), r / beta), (beta if with_beta else None)

    def callable_alpha(self, q, u, with_out=True):
        alpha = self.dot(q, u)
        return alpha if with_out else None

    def callable_step(self, Q, i, u, alphas, betas):
        """-> (Q, alphas, betas, r') after dsea_lanczos_callable_alpha(Q[i-1], u, null) + dsea_lanczos_callable_step"""
        Qn, al, be = self.arr(Q), self.arr(alphas), self.arr(betas)
        alpha = self.dot(Q[i - 1], u)
        if self.writes_alpha():
            al[i - 1] = alpha
        r, c = self.rdots(Q, i, u, alpha, be[i - 2] if i >= 2 else None)
        r2, nrm2 = self.axpy_norm(Q, i, c, r)
        be[i - 1] = self.beta_of(nrm2)
        t = self.q_row(i)
        Qn[t] = self.store(Qn[t], r2 / be[i - 1])
        return Qn, al, be, r2

    # -- partial re-orthogonalisation
    def pro_update(self, st, i, alphas, betas, rr, delta):
        """k_pro_update in its own operation order; returns whether step i is re-orthogonalised"""
        d_ = self.dtype
        al, be = self.arr(alphas), self.arr(betas)
        a = al[i - 1]
        bprev = be[i - 2] if i >= 2 else d_(0.0)
        bcur = np.sqrt(d_(rr))
        anorm = d_(self.anorm_of(d_(st.anorm), abs(a) + bcur + bprev))
        o1, o2 = st.om[(i - 1) & 1], st.om[i & 1]
        new = np.zeros(i, dtype=d_)
        with np.errstate(all="ignore"):
            for k in range(i):
                if k == i - 1:
                    new[k] = d_(EPS1) * anorm / bcur
                    continue
                w1k = d_(o1[k])
                w1p = d_(1.0) if k + 1 == i - 1 else d_(o1[k + 1])
                w2k = d_(1.0) if k == i - 2 else d_(o2[k])
                t = be[k] * w1p + (al[k] - a) * w1k - bprev * w2k
                if k > 0:
                    t = t + be[k - 1] * d_(o1[k - 1])
                d = d_(EPS1) * ((be[k] + bcur) + anorm)
                new[k] = (t + np.copysign(d, t)) / bcur
        o2[:i] = new
        mx = max(float(np.max(np.abs(new))), 0.0) if not np.isnan(new).any() else np.nan
        forced = st.next_too != 0.0
        trig = self.triggers(mx, delta)
        sel = self.selected(trig, forced)
        if sel:
            self.reset(o2, i)
        st.next_too = 1.0 if trig else 0.0
        st.anorm = float(anorm)
        if self.counts(sel):
            st.count += 1.0
        return sel

    def partial_step(self, st, Q, i, u, alphas, betas, delta):
        """-> (r or r', nrm2, anorm, counter) of one dsea_lanczos_partial_step on the workspace state ``st``"""
        if i == 1:
            self.restart(st)
        r, c = self.rdots(Q, i, u, self.arr(alphas)[i - 1], self.arr(betas)[i - 2] if i >= 2 else None)
        rr = c[i]
        fix = lambda: self.axpy_norm(Q, i, self.dots(Q, i, r), r)          # noqa: E731
        if self.pro_update(st, i, alphas, betas, rr, delta):
            r2, nrm2 = fix()
        else:
            r2, nrm2 = self.skip_r(r, lambda: fix()[0]), self.skip_nrm2(rr)
        return r2, nrm2, st.anorm, st.count


class Headroom(Reference):
    """fp64 evaluation of an exact-class case that asserts the class's premise on the way: every term of every sum is a
    multiple of 1/16 and sum |terms| 16 < 2^53, so any partial sum in any order is exact; and the FMA chain of the correction
    stays exact too (multiples of 1/4 below 2^51)"""

    def __init__(self):
        super().__init__(np.float64)
        self.largest = 0.0

    def sum(self, terms):
        scaled = terms * UNIT
        assert np.array_equal(scaled, np.rint(scaled)), "a term is no multiple of 1/16"
        total = float(np.sum(np.abs(scaled)))
        assert total < 2.0 ** 53, "sum of |terms| is %.3g units of 1/16: not exact in every order" % total
        self.largest = max(self.largest, total)
        return super().sum(terms)

    def combine(self, Q, i, c):
        c = np.asarray(c, dtype=np.float64)
        cq = np.asarray(c[:i], dtype=np.float64) * 4.0
        assert np.array_equal(cq, np.rint(cq)), "a coefficient is no multiple of 1/4"
        w = np.abs(c[:i]) @ np.abs(np.asarray(Q[:i], dtype=np.float64))        # the chain's partial sums stay below this
        assert float(np.max(w, initial=0.0)) * 4.0 < 2.0 ** 51
        self.largest = max(self.largest, float(np.max(w, initial=0.0)) * 4.0)
        return super().combine(Q, i, c)


def assert_headroom(stage, *args, prove=True):
    """run ``stage`` on an exact-class case through Headroom; with ``prove`` also require fp64 == longdouble on every vector
    output (no elementwise operation rounded).  Returns the fp64 outputs."""
    h = Headroom()
    got = getattr(h, stage)(*args)
    if prove and stage in ("rdots", "axpy_norm", "ritz"):
        want = getattr(Reference(LD), stage)(*args)
        for g, w in zip(got if isinstance(got, tuple) else (got,), want if isinstance(want, tuple) else (want,)):
            assert np.array_equal(np.atleast_1d(g).astype(LD), np.atleast_1d(w)), stage
    assert_headroom.largest = max(assert_headroom.largest, h.largest)
    return got


assert_headroom.largest = 0.0


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def exact_q(rows, n, seed, support=None):
    """integer entries in [-2, 2] (on ``support`` only, if given); no zero row"""
    rng = np.random.default_rng(seed)
    Q = np.zeros((rows, n))
    cols = np.arange(n) if support is None else support
    Q[:, cols] = rng.integers(-2, 3, size=(rows, cols.size)).astype(np.float64)
    for j in range(rows):
        if not Q[j].any():
            Q[j, cols[j % cols.size]] = 1.0
    return Q


def exact_u(n, seed):
    return np.random.default_rng(seed).integers(-4, 5, size=n).astype(np.float64)


def halves(count, seed):
    """non-zero multiples of 1/2 in [-2, 2]"""
    v = np.random.default_rng(seed).integers(-4, 5, size=count).astype(np.float64) / 2.0
    v[v == 0] = 0.5
    return v


def random_q(n, rows, seed=5):
    from krylov_reference import random_rows
    assert rows <= n
    return np.array(random_rows(n, rows, seed))


def random_u(Q, i, seed, noise=1.0):
    """u = sum_{j<i} g_j q_j + noise orthogonal to them, |g_j| in [1, 2]: the coefficients q_j . r of the step are O(1), not rounding residue"""
    from dominantsparseeigenad_amd.synthetic import normal_vector
    n = Q.shape[1]
    rng = np.random.default_rng(seed)
    g = (1.0 + rng.random(i)) * rng.choice((-1.0, 1.0), size=i)
    w = noise * normal_vector(n, seed) / np.sqrt(n)
    w = w - (Q[:i] @ w) @ Q[:i]                 # (to fp64 rounding: the noise carries no coefficient of its own)
    return g @ Q[:i] + w, g


def assert_amplified(Q, i, r, floor=0.25):
    """the premise of the random class: every coefficient of the correction is of the size of ||r||, so a wrong correction
    moves r' by far more than any bound allows"""
    c = np.asarray(Q[:i], dtype=np.float64) @ np.asarray(r, dtype=np.float64)
    big = np.abs(c) >= floor
    assert big.sum() >= max(i - 1, 1), ("coefficients", c)
    return c


def tridiagonal(n, seed):
    """a symmetric tridiagonal operand for the chain: apply(v) in fp64"""
    rng = np.random.default_rng(seed)
    dg, off = 3.0 * rng.standard_normal(n), rng.standard_normal(n - 1)

    def apply(v):
        y = dg * v
        y[:-1] += off * v[1:]
        y[1:] += off * v[:-1]
        return y

    return apply


# ---- judges of the random class (on the call's own inputs and outputs; return {name: error / bound}) -----------------------
MIRROR = Reference(np.float64)


def _ld(a):
    return np.asarray(a, dtype=LD)


def judge_rdots(Q, i, u, a, b, r, c):
    n = u.size
    out = {"r": bit(r, MIRROR.three_term(Q, i, u, a, b))}
    rl = _ld(r)
    for j in range(i):
        out["c_%d" % j] = sum_ratio(c[j], _ld(Q[j]) * rl, n)
    out["rr"] = sum_ratio(c[i], rl * rl, n)
    return out


def correction_bound(Q, i, c_abs, out_abs, extra=0.0):
    """u |out_k| + (i + 17) u sum_j |c_j q_jk| (+ extra): i FMAs, at most 16 per-wave chains combined by 15 additions in the
    split form, one rounded subtraction"""
    return U * out_abs + (i + 17) * U * (c_abs @ np.abs(_ld(Q[:i]))) + extra


def judge_axpy_norm(Q, i, c, r, r2, nrm2):
    n = r.size
    cl, r2l = _ld(c[:i]), _ld(r2)
    want = _ld(r) - cl @ _ld(Q[:i])
    return {"r'": worst_ratio(np.abs(r2l - want), correction_bound(Q, i, np.abs(cl), np.abs(r2l))),
            "nrm2": sum_ratio(nrm2, r2l * r2l, n)}


def judge_ritz(Q, k, s, out):
    sl = _ld(s[:k])
    return {"out": worst_ratio(np.abs(_ld(out) - sl @ _ld(Q[:k])), correction_bound(Q, k, np.abs(sl), 0.0 * np.abs(_ld(out))))}


def judge_store(r, nrm2, Q, row, Qn, beta, with_beta):
    b = np.sqrt(np.float64(nrm2))
    want = np.array(Q, dtype=np.float64)
    want[row] = np.asarray(r, dtype=np.float64) / b
    out = {"Q": bit(Qn, want)}
    if with_beta:
        out["beta"] = bit(beta, b)
    return out


def hidden_bounds(Q, i, r):
    """the correction with the coefficients hidden: (r - Q^T Q r in longdouble, the part of the bound that does not depend on
    the output)"""
    n = r.size
    Ql, rl = _ld(Q[:i]), _ld(r)
    absQ = np.abs(Ql)
    c = Ql @ rl
    E = (n + 4) * U * (absQ @ np.abs(rl))
    return rl - c @ Ql, (i + 17) * U * ((np.abs(c) + E) @ absQ) + E @ absQ


def judge_callable_step(Q, i, u, alphas, betas, Qn, al, be, r2):
    n = u.size
    out = {"alpha": sum_ratio(al[i - 1], _ld(Q[i - 1]) * _ld(u), n)}
    keep = [k for k in range(len(alphas)) if k != i - 1]
    out["other alphas"] = bit(np.asarray(al)[keep], np.asarray(alphas)[keep])
    keep = [k for k in range(len(betas)) if k != i - 1]
    out["other betas"] = bit(np.asarray(be)[keep], np.asarray(betas)[keep])
    r = MIRROR.three_term(Q, i, u, al[i - 1], betas[i - 2] if i >= 2 else None)
    want, fixed = hidden_bounds(Q, i, r)
    r2l = _ld(r2)
    out["r'"] = worst_ratio(np.abs(r2l - want), U * np.abs(r2l) + fixed)
    T = np.sum(r2l * r2l)
    out["beta"] = worst_ratio(abs(LD(be[i - 1]) ** 2 - T), float(((n + 4) * U + 2 * U) * T))
    wantQ = np.array(Q, dtype=np.float64)
    wantQ[i] = np.asarray(r2, dtype=np.float64) / np.float64(be[i - 1])
    out["Q"] = bit(Qn, wantQ)
    return out


def judge_partial_step(Q, i, u, alphas, betas, selected, r2, nrm2):
    """``selected`` is read off the counter; a skipped step's nrm2 is the rr the device summed: the sum bound against r"""
    n = u.size
    r = MIRROR.three_term(Q, i, u, alphas[i - 1], betas[i - 2] if i >= 2 else None)
    r2l = _ld(r2)
    out = {"nrm2": sum_ratio(nrm2, r2l * r2l, n)}
    if selected:
        want, fixed = hidden_bounds(Q, i, r)
        out["r'"] = worst_ratio(np.abs(r2l - want), U * np.abs(r2l) + fixed)
    else:
        out["r"] = bit(r2, r)
    return out


# ---- the checks: one implementation of the stages through both classes ------------------------------------------------------
class Checks:
    """``impl`` has the stage methods of Reference (numpy in, numpy out; the GPU test's implementation makes one library call
    per method), ``setup(rpl=, split=, kmax=)`` (a context manager that selects the kernel geometry; a no-op on the host),
    ``layouts`` (the leading dimensions to cover) and ``partial(n, delta)`` (a context manager yielding an object whose
    ``step(Q, i, u, alphas, betas)`` is one dsea_lanczos_partial_step on one workspace).  Every check raises AssertionError
    where a verdict fails and returns the worst ratio of the random class."""

    def __init__(self, impl, log=print, prove=True):
        self.impl, self.log, self.prove, self.mirror = impl, log, prove, MIRROR
        self.cases = 0                      # verdicts given: one per call in the exact class, one per judged call in the random class

    def headroom(self, stage, *args):
        return assert_headroom(stage, *args, prove=self.prove)

    # -- verdicts
    def exact(self, tag, got, want):
        names = "abcdefgh"
        got = got if isinstance(got, tuple) else (got,)
        want = want if isinstance(want, tuple) else (want,)
        assert len(got) == len(want), tag
        self.cases += 1
        for k, (g, w) in enumerate(zip(got, want)):
            if g is None and w is None:
                continue
            assert g is not None and w is not None and same(g, w), "%s: output %s differs from the fp64 reference in %d of %d places (exact class)" % (
                tag, names[k], int(np.sum(np.atleast_1d(g) != np.atleast_1d(w))) if np.shape(g) == np.shape(w) else -1, np.size(w))

    def ratios(self, tag, res):
        self.cases += 1
        worst = max(res.values()) if res else 0.0
        bad = {k: v for k, v in res.items() if not v <= 1.0}
        assert not bad, "%s: %s" % (tag, bad)
        return float(worst)

    def report(self, tag, worst):
        self.log("%s: exact class bit for bit; random class worst error / bound = %.3f" % (tag, worst))
        return worst

    def layouts(self, n):
        return self.impl.layouts if n <= 4097 else self.impl.layouts[:1]

    # -- phases
    def rdots(self, n, steps=STEPS_REV, random=True, rpl=0, split=-1, kmax=None):
        """exact: every i of ``steps`` with beta and (i <= 2) without; random: the largest i <= n of (5, 3, 2, 1) and i = 1"""
        worst = 0.0
        with self.impl.setup(rpl=rpl, split=split, kmax=kmax):
            for i in steps:
                Q, u = exact_q(i, n, 11 + n + i), exact_u(n, 12 + n + i)
                for b in (B_EXACT, None) if i <= 2 else (B_EXACT,):
                    want = self.headroom("rdots", Q, i, u, A_EXACT, b)
                    for ld in self.layouts(n):
                        self.exact("rdots n=%d i=%d beta=%s ld=%s" % (n, i, b, ld), self.impl.rdots(Q, i, u, A_EXACT, b, ld=ld), want)
            if random:
                for i in sorted({max(k for k in (5, 3, 2, 1) if k <= n), 1}):
                    Q = random_q(n, i)
                    u, _ = random_u(Q, i, 13 + n + i)
                    assert_amplified(Q, i, MIRROR.three_term(Q, i, u, A_RANDOM, B_RANDOM))
                    for b in (B_RANDOM, None) if i == 1 else (B_RANDOM,):
                        r, c = self.impl.rdots(Q, i, u, A_RANDOM, b, ld=self.impl.layouts[-1])
                        worst = max(worst, self.ratios("rdots n=%d i=%d beta=%s" % (n, i, b), judge_rdots(Q, i, u, A_RANDOM, b, r, c)))
        return self.report("rdots n=%d rpl=%d split=%d" % (n, rpl, split), worst)

    def axpy_norm(self, n, steps=(1, 2, 5, 8), random=True, rpl=0, split=-1, kmax=None):
        worst = 0.0
        with self.impl.setup(rpl=rpl, split=split, kmax=kmax):
            for i in steps:
                Q, r = exact_q(i, n, 21 + n + i), exact_u(n, 22 + n + i) / 4.0 + exact_u(n, 23 + n + i)
                c = np.append(halves(i, 24 + n + i), 3.5)             # c[i]: the slot a shifted read would pick up
                want = self.headroom("axpy_norm", Q, i, c, r)
                for ld in self.layouts(n):
                    self.exact("axpy_norm n=%d i=%d ld=%s" % (n, i, ld), self.impl.axpy_norm(Q, i, c, r, ld=ld), want)
            if random:
                i = max(k for k in (5, 3, 2, 1) if k <= n)
                Q = random_q(n, i)
                r, g = random_u(Q, i, 25 + n)
                c = np.append(g * (1.0 + 0.01 * np.arange(i)), 1.5)
                r2, nrm2 = self.impl.axpy_norm(Q, i, c, r, ld=self.impl.layouts[-1])
                worst = self.ratios("axpy_norm n=%d i=%d" % (n, i), judge_axpy_norm(Q, i, c, r, r2, nrm2))
        return self.report("axpy_norm n=%d rpl=%d split=%d" % (n, rpl, split), worst)

    def ritz(self, n, steps=(1, 2, 5, 8), random=True):
        worst = 0.0
        with self.impl.setup():
            for k in steps:
                Q, s = exact_q(k, n, 31 + n + k), np.append(halves(k, 32 + n + k), 3.5)
                want = self.headroom("ritz", Q, k, s)
                for ld in self.layouts(n):
                    self.exact("ritz n=%d k=%d ld=%s" % (n, k, ld), self.impl.ritz(Q, k, s, ld=ld), want)
            if random:
                k = max(t for t in (5, 3, 2, 1) if t <= n)
                Q = random_q(n, k)
                s = np.append(random_u(Q, k, 33 + n)[1], 1.5)
                worst = self.ratios("ritz n=%d k=%d" % (n, k), judge_ritz(Q, k, s, self.impl.ritz(Q, k, s, ld=self.impl.layouts[-1])))
        return self.report("ritz n=%d" % n, worst)

    def store(self, n, random=True):
        """dsea_lanczos_store into rows 0 and 2 of a three-row basis and dsea_scale_store, with and without beta_out.  No sum:
        beta = sqrt(nrm2) and r / beta are single correctly rounded operations (exact class: nrm2 = 6.25 and 3.0)"""
        from dominantsparseeigenad_amd.synthetic import normal_vector
        worst = 0.0
        with self.impl.setup():
            Q0 = np.full((3, n), SENTINEL)
            for nrm2, r in ((6.25, exact_u(n, 41 + n)), (3.0, exact_u(n, 42 + n) / 4.0)):
                for row, with_beta in ((0, True), (2, True), (2, False)):
                    want = self.mirror.store_row(r, nrm2, Q0, row, with_beta)
                    for ld in self.layouts(n):
                        self.exact("store n=%d row=%d nrm2=%r beta_out=%s ld=%s" % (n, row, nrm2, with_beta, ld),
                                   self.impl.store_row(r, nrm2, Q0, row, with_beta, ld=ld), want)
                for with_beta in (True, False):
                    self.exact("scale_store n=%d nrm2=%r beta_out=%s" % (n, nrm2, with_beta), self.impl.scale_store(r, nrm2, with_beta),
                               self.mirror.scale_store(r, nrm2, with_beta))
            if random:
                r = normal_vector(n, 43 + n)
                nrm2 = float(np.dot(r, r)) * 1.0000001
                for with_beta in (True, False):
                    Qn, beta = self.impl.store_row(r, nrm2, Q0, 1, with_beta, ld=self.impl.layouts[-1])
                    worst = max(worst, self.ratios("store n=%d" % n, judge_store(r, nrm2, Q0, 1, Qn, beta, with_beta)))
                    q, beta = self.impl.scale_store(r, nrm2, with_beta)
                    res = {"q": bit(q, r / np.sqrt(nrm2))}
                    if with_beta:
                        res["beta"] = bit(beta, np.sqrt(nrm2))
                    assert with_beta or beta is None
                    worst = max(worst, self.ratios("scale_store n=%d" % n, res))
        return self.report("store n=%d" % n, worst)

    def callable_alpha(self, n, random=True):
        from dominantsparseeigenad_amd.synthetic import normal_vector
        worst = 0.0
        with self.impl.setup():
            q, u = exact_q(1, n, 51 + n)[0], exact_u(n, 52 + n)
            want = self.headroom("callable_alpha", q, u)
            self.exact("callable_alpha n=%d" % n, self.impl.callable_alpha(q, u, True), want)
            assert self.impl.callable_alpha(q, u, False) is None
            if random:
                q, u = normal_vector(n, 53 + n), normal_vector(n, 54 + n)
                alpha = self.impl.callable_alpha(q, u, True)
                worst = self.ratios("callable_alpha n=%d" % n, {"alpha": sum_ratio(alpha, _ld(q) * _ld(u), n)})
        return self.report("callable_alpha n=%d" % n, worst)

    def step_inputs(self, n, i, seed):
        """exact class with a hidden c: Q on support_rows(n) (row i a sentinel), alphas / betas sentinels but betas[i-2]; the
        seed moves on until r' != 0 (at n = 1 most draws break down)"""
        al, be = np.full(i + 2, SENTINEL), np.full(i + 2, SENTINEL)
        if i >= 2:
            be[i - 2] = B_EXACT
        for attempt in range(64):
            Q, u = exact_q(i + 1, n, seed + 1000 * attempt, support_rows(n)), exact_u(n, seed + 1000 * attempt + 1)
            Q[i] = SENTINEL
            with np.errstate(invalid="ignore"):
                if self.mirror.callable_step(Q, i, u, al, be)[2][i - 1] > 0:
                    return Q, u, al, be
        raise AssertionError("no exact callable_step case at n = %d, i = %d" % (n, i))

    def callable_step(self, n, steps=(1, 2, 3, 5, 8), random=True, rpl=0, split=-1):
        worst = 0.0
        with self.impl.setup(rpl=rpl, split=split):
            for i in steps:
                Q, u, al, be = self.step_inputs(n, i, 61 + n + i)
                want = self.headroom("callable_step", Q, i, u, al, be)
                assert want[1][i - 1] != SENTINEL and want[2][i - 1] > 0 and (want[1][i:] == SENTINEL).all(), "the case is degenerate"
                for ld in self.layouts(n):
                    self.exact("callable_step n=%d i=%d ld=%s" % (n, i, ld), self.impl.callable_step(Q, i, u, al, be, ld=ld), want)
            if random:
                # (i < n: at i = n the Krylov space is exhausted and Q[i] = r' / ||r'|| is rounding noise over rounding noise)
                for i in sorted({max(k for k in (5, 3, 2, 1) if k < n), 1}) if n > 1 else ():
                    Q = np.vstack([random_q(n, i), np.full((1, n), SENTINEL)])
                    u, _ = random_u(Q, i, 63 + n + i)
                    al, be = np.full(i + 2, SENTINEL), np.full(i + 2, SENTINEL)
                    if i >= 2:
                        be[i - 2] = B_RANDOM
                    if i >= 2:
                        assert_amplified(Q, i, MIRROR.three_term(Q, i, u, float(np.dot(Q[i - 1], u)), B_RANDOM))
                    got = self.impl.callable_step(Q, i, u, al, be, ld=self.impl.layouts[-1])
                    worst = max(worst, self.ratios("callable_step n=%d i=%d" % (n, i), judge_callable_step(Q, i, u, al, be, *got)))
        return self.report("callable_step n=%d rpl=%d split=%d" % (n, rpl, split), worst)

    def callable_chain(self, n=513, steps=6):
        """six fused steps around a numpy mat-vec; each judged from the implementation's own previous outputs"""
        from dominantsparseeigenad_amd.synthetic import normal_vector
        apply = tridiagonal(n, 7)
        q0 = normal_vector(n, 71)
        Q = np.full((steps + 1, n), SENTINEL)
        Q[0] = q0 / np.sqrt(np.dot(q0, q0))
        al, be = np.full(steps + 1, SENTINEL), np.full(steps + 1, SENTINEL)
        worst = 0.0
        with self.impl.setup():
            for i in range(1, steps + 1):
                u = apply(Q[i - 1].copy())
                got = self.impl.callable_step(Q, i, u, al, be, ld=self.impl.layouts[-1])
                worst = max(worst, self.ratios("chain: callable_step %d" % i, judge_callable_step(Q, i, u, al, be, *got)))
                Q, al, be, _ = got
        G = Q[:steps + 1] @ Q[:steps + 1].T - np.eye(steps + 1)
        assert np.max(np.abs(G)) <= 1e-13, "the chain's basis is not orthonormal"
        return self.report("callable_step chain n=%d" % n, worst)

    # -- partial re-orthogonalisation
    def partial_inputs(self, n, steps, seed):
        """exact class: Q on support_rows(n) (steps + 1 rows), prescribed alphas (multiples of 1/4) and betas (2 ... 4), and per
        step u = a q_{i-1} + b q_{i-2} + s with s in {-1, 0, 1} on the same rows and s = 1 on row n // 2: the three-term r is s
        exactly, ||r|| is of order 1 and the estimates grow by about beta_k / ||r|| per step"""
        rng = np.random.default_rng(seed)
        sup = support_rows(n)
        Q = exact_q(steps + 1, n, seed, sup)
        al = rng.integers(-8, 9, size=steps + 1).astype(np.float64) / 4.0
        be = rng.integers(8, 17, size=steps + 1).astype(np.float64) / 4.0
        us = np.zeros((steps + 1, n))
        cols = np.unique(np.append(sup[:4], n // 2))
        for i in range(1, steps + 1):
            us[i, cols] = rng.integers(-1, 2, size=cols.size)
            us[i, n // 2] = 1.0
            us[i] += al[i - 1] * Q[i - 1] + (be[i - 2] * Q[i - 2] if i >= 2 else 0.0)
        return Q, us, al, be

    def partial_case(self, n, steps):
        """the first seed whose run has a delta with exactly one trigger"""
        for attempt in range(32):
            Q, us, al, be = self.partial_inputs(n, steps, 81 + n + 1000 * attempt)
            found = self.find_single_trigger(Q, us, al, be)
            if found:
                return (Q, us, al, be) + found
        raise AssertionError("no run of %d steps at n = %d has a delta at which exactly one step triggers" % (steps, n))

    def partial_run(self, tag, n, Q, us, al, be, delta, first=1, last=None, session=None, st=None):
        """steps first .. last on one workspace against the fp64 mirror, bit for bit: r, nrm2, anorm, the counter, and so every
        decision.  Returns the pattern of selected steps."""
        last = us.shape[0] - 1 if last is None else last
        pattern = []
        for i in range(first, last + 1):
            before = 0.0 if i == 1 else st.count
            want = self.mirror.partial_step(st, Q[:i], i, us[i], al, be, delta)
            got = session.step(Q[:i], i, us[i], al, be)
            self.exact("%s step %d" % (tag, i), tuple(got), tuple(want))
            pattern.append(st.count > before)
        return pattern

    def find_single_trigger(self, Q, us, al, be):
        """(delta, pattern) at which exactly one step of the run triggers -- that step and the next are selected, no other -- or
        None"""
        free = ProState()
        steps = us.shape[0] - 1
        mx = []
        for i in range(1, steps + 1):
            self.mirror.partial_step(free, Q[:i], i, us[i], al, be, 1e300)
            mx.append(float(np.max(np.abs(free.om[i & 1][:i]))))
        for t in range(1, steps - 2):
            lo = max(mx[:t])
            if not mx[t] > lo:
                continue
            delta = float(np.sqrt(lo * mx[t]))
            st, pat = ProState(), []
            for i in range(1, steps + 1):
                before = st.count
                self.mirror.partial_step(st, Q[:i], i, us[i], al, be, delta)
                pat.append(st.count > before)
            if pat == [k in (t, t + 1) for k in range(steps)]:
                return delta, pat
        return None

    def partial_exact(self, n, steps=9, rpl=0, split=-1):
        """tiny delta (all selected), huge delta (none), one trigger (that step, the next by ``forced``, then skipped again),
        and a second run from i = 1 on the same workspace whose counter and anorm restart"""
        Q, us, al, be, one, want_pat = self.partial_case(n, steps)
        for i in range(1, steps + 1):                      # the premise: every sum exact on both branches
            self.headroom("rdots", Q[:i], i, us[i], al[i - 1], be[i - 2] if i >= 2 else None)
            r = self.mirror.three_term(Q, i, us[i], al[i - 1], be[i - 2] if i >= 2 else None)
            self.headroom("axpy_norm", Q[:i], i, np.append(self.mirror.dots(Q[:i], i, r)[:i], 0.0), r)
        with self.impl.setup(rpl=rpl, split=split):
            for name, delta, want in (("all", 1e-300, [True] * steps), ("none", 1e300, [False] * steps), ("one", one, want_pat)):
                with self.impl.partial(n, delta) as session:
                    st = ProState()
                    tag = "partial_step n=%d delta=%s" % (n, name)
                    pat = self.partial_run(tag, n, Q, us, al, be, delta, session=session, st=st)
                    assert pat == want, (tag, pat)
                    if name != "none":                 # a second run on the same workspace: i = 1 restarts everything
                        pat2 = self.partial_run(tag + " again", n, Q, us, al, be, delta, last=4, session=session, st=st)
                        assert st.count == sum(pat2) and st.count < sum(pat) + sum(pat2), tag
        return 0.0

    def partial_strict(self, n=2):
        """i = 1, alphas[0] = 2, rr = 4: anorm = 4, bcur = 2, the only estimate is 2^-46 4 / 2 = 2^-45 exactly: delta = 2^-45
        skips, the next double below selects"""
        Q = np.zeros((1, n))
        Q[0, 0] = 1.0
        u = 4.0 * Q[0]                                     # r = 2 q_0: a selected step leaves r' = 0, a skipped one r and nrm2 = rr = 4
        al, be = np.array([2.0, SENTINEL]), np.array([SENTINEL, SENTINEL])
        edge = 2.0 ** -45
        with self.impl.setup():
            for delta, sel in ((edge, False), (float(np.nextafter(edge, 0.0)), True)):
                with self.impl.partial(n, delta) as session:
                    st = ProState()
                    want = self.mirror.partial_step(st, Q, 1, u, al, be, delta)
                    got = session.step(Q, 1, u, al, be)
                    self.exact("partial_step strictness delta=%r" % delta, tuple(got), tuple(want))
                    assert got[2] == 4.0 and got[3] == (1.0 if sel else 0.0) and got[1] == (0.0 if sel else 4.0), (delta, got)
        return 0.0

    def partial_random(self, n, steps=5, rpl=0, split=-1):
        """huge delta: every step skipped -- r bit for bit, nrm2 = the device's rr (sum bound), and anorm the running maximum of
        |alpha| + sqrt(nrm2) + beta_prev from the downloaded nrm2, bit for bit.  Tiny delta: every step selected -- r' to the
        hidden-coefficient bound, the counter = steps."""
        steps = min(steps, n)
        Q = random_q(n, steps)
        rng = np.random.default_rng(91 + n)
        al, be = rng.random(steps + 1) - 0.5, 0.25 + 0.25 * rng.random(steps + 1)
        worst = 0.0
        with self.impl.setup(rpl=rpl, split=split):
            for delta, sel in ((1e300, False), (1e-300, True)):
                with self.impl.partial(n, delta) as session:
                    anorm = 0.0
                    for i in range(1, steps + 1):
                        u, _ = random_u(Q, i, 92 + n + i)
                        assert_amplified(Q, i, MIRROR.three_term(Q, i, u, al[i - 1], be[i - 2] if i >= 2 else None), floor=0.5)
                        r2, nrm2, an, count = session.step(Q[:i], i, u, al, be)
                        res = judge_partial_step(Q, i, u, al, be, sel, r2, nrm2)
                        res["counter"] = bit(count, float(i) if sel else 0.0)
                        if not sel:
                            anorm = max(anorm, abs(al[i - 1]) + np.sqrt(np.float64(nrm2)) + (be[i - 2] if i >= 2 else 0.0))
                            res["anorm"] = bit(an, anorm)
                        worst = max(worst, self.ratios("partial_step n=%d i=%d selected=%s" % (n, i, sel), res))
        return self.report("partial_step n=%d rpl=%d split=%d" % (n, rpl, split), worst)

    # -- the same call twice
    def twice(self, n, rpl=0, split=-1):
        i = max(min(5, n - 1), 1)
        Q = np.vstack([random_q(n, i), np.full((1, n), SENTINEL)])
        u, g = random_u(Q, i, 95 + n)
        al, be = np.full(i + 2, SENTINEL), np.full(i + 2, B_RANDOM)
        c = np.append(g, 1.5)
        with self.impl.setup(rpl=rpl, split=split):
            calls = [("rdots", lambda: self.impl.rdots(Q[:i], i, u, A_RANDOM, B_RANDOM)),
                     ("axpy_norm", lambda: self.impl.axpy_norm(Q[:i], i, c, u))]
            if n > 1:                                          # (n = 1: the step breaks down, r' = 0)
                calls.append(("callable_step", lambda: self.impl.callable_step(Q, i, u, al, be)))
            for name, call in calls:
                self.exact("%s n=%d twice" % (name, n), call(), call())
        return 0.0

    def small(self, n, random=True):
        """every check of the split-16 sizes"""
        runs = [lambda: self.rdots(n, random=random), lambda: self.axpy_norm(n, random=random), lambda: self.ritz(n, random=random),
                lambda: self.store(n, random), lambda: self.callable_alpha(n, random), lambda: self.callable_step(n, random=random),
                lambda: self.partial_exact(n), self.partial_strict]
        if random:
            runs += [lambda: self.partial_random(n), lambda: self.twice(n)]
        return max(run() for run in runs)


# ---- wrong kernels: each breaks one rule of Reference -----------------------------------------------------------------------
def _mutant(name, **methods):
    return type(name, (Reference,), methods)


def _fma(self, r, s, q):
    return np.asarray(np.asarray(r, dtype=LD) - LD(s) * np.asarray(q, dtype=LD), dtype=self.dtype)


def _drop_last_from_sum(self, terms):
    return Reference.sum(self, terms[:-1] if terms.size & 1 else terms)


def _drop_last_from_store(self, old, new):
    if new.size & 1:
        new = new.copy()
        new[-1] = old[-1]
    return new


def _drop_one_partial(self, terms):
    """the partial of the last 128-row tile never reaches the sum"""
    return Reference.sum(self, terms[:(terms.size - 1) // TILE * TILE])


def _second_trip_overwrites(self, terms):
    """set_rows_per_lane(2) beyond 8192 tiles: a wave's second tile replaces its first"""
    ntiles = (terms.size + TILE - 1) // TILE
    if ntiles <= MAX_WAVES:
        return Reference.sum(self, terms)
    return Reference.sum(self, terms[(ntiles - MAX_WAVES) * TILE:])


def _skip_corrects(self, r, corrected):
    return corrected()


MUTANTS = {
    "the q(i-2) term is dropped at i >= 2": _mutant("NoSecondTerm", terms3=lambda self, i, a, b: [(i - 1, a)]),
    "the q(i-2) term is applied at i = 1": _mutant(
        "SecondTermAtOne", terms3=lambda self, i, a, b: [(i - 1, a)] + ([(max(i - 2, 0), b)] if b is not None else [])),
    "a and b are exchanged": _mutant(
        "Exchanged", terms3=lambda self, i, a, b: Reference.terms3(self, i, a, b) if i < 2 or b is None else [(i - 1, b), (i - 2, a)]),
    "the three-term update is contracted into FMAs": _mutant("Contracted", minus=_fma),
    "the dots are taken against u": _mutant("DotsSeeU", dots_see=lambda self, u, r: u),
    "the remainder vectors j >= 4 floor(i / 4) are dropped": _mutant("NoRemainder", dotted=lambda self, i: range(4 * (i // 4))),
    "c_j is stored at i - 1 - j on odd i": _mutant("Reversed", slot=lambda self, i, j: i - 1 - j if i & 1 else j),
    "c_i is taken after the correction": _mutant("LateNorm", rr_sees=lambda self, r, corrected: corrected()),
    "the last row of an odd n is dropped from a sum": _mutant("LastRowSum", sum=_drop_last_from_sum),
    "the last row of an odd n is dropped from a store": _mutant("LastRowStore", store=_drop_last_from_store),
    "one partial is dropped": _mutant("PartialDropped", sum=_drop_one_partial),
    "the second grid-stride trip overwrites": _mutant("TripOverwrites", sum=_second_trip_overwrites),
    "the correction runs over i - 1 vectors": _mutant("ShortCorrection", corrected=lambda self, i: range(i - 1)),
    "the correction uses c_{j+1}": _mutant("ShiftedCoefficient", coef=lambda self, c, j: c[j + 1]),
    "nrm2 is taken before the subtraction": _mutant("EarlyNorm", norm_sees=lambda self, r, r2: r),
    "beta without the square root": _mutant("NoRoot", beta_of=lambda self, nrm2: nrm2),
    "Q[i] is written to row i - 1": _mutant("WrongRow", q_row=lambda self, row: max(row - 1, 0)),
    "alphas[i-1] is not written": _mutant("AlphaNotWritten", writes_alpha=lambda self: False),
    "a skipped step corrects anyway": _mutant("SkipCorrects", skip_r=_skip_corrects),
    "a skipped step's nrm2_out is not rr": _mutant("SkipNorm", skip_nrm2=lambda self, rr: np.nextafter(rr, np.inf)),
    "forced is ignored": _mutant("NoForced", selected=lambda self, trig, forced: trig),
    "the trigger is decided with <": _mutant("TriggerNotStrict", triggers=lambda self, mx, delta: not (mx < delta)),
    "the omega row is not reset after a selected step": _mutant("NoReset", reset=lambda self, row, i: None),
    "anorm is not a running maximum": _mutant("NoRunningMax", anorm_of=lambda self, prev, cand: cand),
    "the counter is incremented on skipped steps": _mutant("CountsAll", counts=lambda self, selected: True),
    "no restart at i = 1": _mutant("NoRestart", restart=lambda self, st: None),
}


class HostImpl:
    """a Reference behind the interface Checks drives (what the GPU test's implementation offers around the library)"""

    layouts = ("even",)

    def __init__(self, ref):
        self.ref, self.states = ref, {}

    @staticmethod
    def _f64(out):
        if isinstance(out, tuple):
            return tuple(None if o is None else (np.asarray(o, dtype=np.float64) if np.ndim(o) else float(o)) for o in out)
        return None if out is None else (np.asarray(out, dtype=np.float64) if np.ndim(out) else float(out))

    def __getattr__(self, name):
        fn = getattr(self.ref, name)

        def call(*a, ld=None, **k):
            return self._f64(fn(*a, **k))
        return call

    @contextlib.contextmanager
    def setup(self, rpl=0, split=-1, kmax=None):
        yield

    @contextlib.contextmanager
    def partial(self, n, delta):
        st, ref, f64 = self.states.setdefault(n, ProState()), self.ref, self._f64       # (one workspace per n, as in the GPU test)

        class Session:
            def step(self, Q, i, u, alphas, betas):
                return f64(ref.partial_step(st, Q, i, u, alphas, betas, delta))
        yield Session()
