"""numpy references, input classes, error bounds, judges and checks of the conjugate-gradient stage tests
(tests/test_gpu_cg_stages.py, proved on the CPU by tests/test_cg_reference_cpu.py); no GPU, no torch.
docs/design/26-cg-stage-tests.md tells the same story at length.

``Reference(dtype)`` evaluates every stage of include/dsea.h's CG family (reference CG.py:24-41) in ``dtype``: np.longdouble is
the high-precision reference, np.float64 the MIRROR (the kernels round every elementwise product and sum separately --
__dmul_rn / __dadd_rn, -ffp-contract=off -- and so does numpy), np.float64 with ``order`` an honest fp64 evaluation whose
sums are taken in a random permutation.  state = STATE_LEN numbers indexed by RR ... ITERS (the DSEA_CG_* constants).

TWO INPUT CLASSES, TWO VERDICTS

  exact     vectors are integers in [-4, 4]; Ad = D d with D integer in [1, 4] (so d.Ad' > 0); the shift is 0.375; the current
            rr slot is set to 0.375 (d.Ad'), so alpha = fl(rr / d.Ad') = 0.375 exactly, x' is a multiple of 1/8 and r' of 1/64;
            Psi has integer entries in [-2, 2] (no orthonormality: the kernels compute the formula whatever Psi is).  Every term
            of every sum is then a multiple of 2^-12 and every partial sum, in any order, with or without FMA, is exact as long
            as sum |terms| < 2^53 2^-12: ``Headroom`` asserts exactly that for every sum of every case (and that fp64 and
            longdouble agree bit for bit on everything before beta).  beta = fl(rr_new / rr), sqrt and d' = fl(r' + fl(beta d))
            are single correctly rounded operations that numpy reproduces.  Verdict: EVERY output vector and EVERY state slot
            equals Reference(np.float64) bit for bit.
  random    synthetic.normal_vector entries, Ad = D d with D in [1, 4], Psi orthonormal.  Each stage is judged on the device's
            own inputs and outputs, so the conditioning of a solve never enters.  u = 2^-53.
              (a) elementwise results whose scalars are visible in ``state`` equal the fp64 mirror bit for bit: Ad' = Ad - fl(s d);
                  d' = r' + fl(beta d) with beta = fl(new slot / current slot) from the downloaded slots; RESNORM = sqrt(slot);
                  every output of the unfused phases (the test sets RR, DAD, BETA itself).
              (b) a reduction of n terms t_i (each product exact inside an FMA or rounded once, n - 1 additions in some tree):
                      |sum_dev - sum t_i| <= (n + 4) u sum |t_i|        t_i from the device's own elementwise output
                  (gamma_{n+1} <= (n + 4) u for n u << 1).  Used for rr = r'.r', x.y', a.v, psi_j.v and ||P r||^2.
              (c) alpha = fl(rr / dAd_dev) is formed inside dsea_cg_step / dsea_cg_deflated_step and not stored.  With
                  S = d.Ad' (longdouble, device's Ad'), e_d = (n + 4) u sum |d_i Ad'_i| / |S|: alpha = (rr / S) (1 + eta),
                  |eta| <= e_a = (e_d + u) / (1 - e_d - u).  x'_i = fl(x_i + fl(alpha d_i)) then obeys
                      |x'_i - (x_i + (rr / S) d_i)| <= u |x'_i| + |(rr / S) d_i| (e_a + 2 u)
                  and r' likewise with Ad' in place of d (one rounding of the product, one of the sum, eta).
              (d) out = v - sum_j c_j psi_j with c_j = psi_j.v summed on the device: w_i = sum_j c_j psi_ji is a chain of m FMAs
                  (|w_i - sum| <= (m + 1) u sum_j |c_j psi_ji|), then one rounded subtraction.  With the coefficients visible
                  (coef_out):  |c_j - psi_j.v| <= (n + 4) u sum_i |psi_ji v_i|  and
                      |out_i - (v_i - sum_j c_j psi_ji)| <= u |out_i| + (m + 1) u sum_j |c_j psi_ji|.
                  With the coefficients hidden, and the operand v known only to B_i (|v_dev_i - V_i| <= B_i):
                      E_j = sum_i |psi_ji| B_i + (n + 4) u sum_i |psi_ji| (|V_i| + B_i)            (error of c_j)
                      |out_i - (V - Psi^T Psi V)_i| <= u |out_i| + B_i + sum_j E_j |psi_ji| + (m + 1) u sum_j (|c^_j| + E_j) |psi_ji|
                  For dsea_cg_deflated_init V is the fp64 mirror of b - (Ax - fl(s x)) (B = 0); for dsea_cg_deflated_step V is
                  r - (rr / S) Ad' and B_i = (u |V_i| + |(rr / S) Ad'_i| (e_a + 2 u)) / (1 - u)   (bound (c) without knowing r~).
              (e) psi_j.out follows from (d): psi_j.(V - Psi^T Psi V) = sum_k (delta_jk - G_jk) c^_k with G the Gram matrix of
                  Psi, so |psi_j.out| <= sum_k |G - I|_jk |c^_k| + sum_i |psi_ji| bound_i; and for d' = fl(r' + fl(beta d)):
                  |psi_j.d'| <= (bound of psi_j.r') + |beta| (bound of psi_j.d) + u sum_i |psi_ji| (|d'_i| + |beta d_i|).
            No constant is fitted to a device.  Verdict: every ratio error / bound <= 1 (a bit inequality counts as inf).

``Checks(impl)`` drives an implementation of the eleven entries through all of this: the GPU test hands it the library, the CPU
test ``Reference(np.float64, order=...)`` (must pass) and the ``MUTANTS`` (must each fail)."""
import numpy as np

from matvec_reference import LD, U, eighths, exact_vector, headroom, worst_ratio

RR, DAD, RRNEW, ALPHA, BETA, RESNORM, DONE, ITERS = range(8)
STATE_LEN = 8
MAX_NEV = 8
TILE, PERSIST_MAX_TILES, MAX_EW_BLOCKS = 512, 4096, 2048
SENTINEL = -7.0
SHIFT_EXACT, SHIFT_RANDOM = 0.375, 0.6180339887498949
ALPHA_EXACT = 0.375
UNIT = 2.0 ** 12                       # every term of an exact-class sum is a multiple of 1 / UNIT

SIZES_SMALL = (1, 2, 3, 511, 512, 513, 1025, 2047, 2049, 4097)
SIZES_LARGE = (140001, 300001, (1 << 21) + 3)          # exact class + one random case each
SIZES_PHASE_EXTRA = ((1 << 19) + 2049, (1 << 22) + 5)  # unfused phases only: > 256 partials of k_cg_finalize_rrnew; the 2048-block cap
SIZES = SIZES_SMALL + SIZES_LARGE
MS = (1, 2, 3, 8)


# ---- launcher geometry (csrc/dsea_internal.h, csrc/dsea_deflated.hip) ---------------------------------------------------
def ew_blocks(n):
    return int(min(max((n + 2047) // 2048, 1), MAX_EW_BLOCKS))


def tile_blocks(n):
    nt = (n + TILE - 1) // TILE
    return int(max(nt, 1)) if nt <= PERSIST_MAX_TILES else ew_blocks(n)


dfl_blocks = tile_blocks           # the same rule, written twice in the library


def partial_trips(count):
    """(full double trips of sum_partials_block's loop for thread 0, whether a tail read follows)"""
    b, trips = 0, 0
    while b + 256 < count:
        b += 512
        trips += 1
    return trips, b < count


def edge_rows(n):
    """row 0, row n - 1, both sides of every 512-row tile edge and of every grid-stride trip edge"""
    rows = {0, n - 1}
    for e in range(TILE, n, TILE):
        rows.update((e - 1, e))
    stride = tile_blocks(n) * TILE
    for e in range(stride, n, stride):
        rows.update((e - 1, e))
    return np.array(sorted(r for r in rows if 0 <= r < n), dtype=np.int64)


# ---- the stages ---------------------------------------------------------------------------------------------------------
class Reference:
    """Every stage in ``dtype``.  Vectors in, new vectors out (nothing is modified in place); ``state`` is an array of
    STATE_LEN.  ``order`` (a seed) makes every sum run over a random permutation of its terms.  The small methods at the top
    are the rules a wrong kernel breaks: MUTANTS overrides them one at a time."""

    def __init__(self, dtype=np.float64, order=None):
        self.dtype, self.order = dtype, order

    # -- rules
    def cur(self, parity):
        return RRNEW if parity else RR

    def new(self, parity):
        return RR if parity else RRNEW

    def beta(self, rr_new, rr):
        return rr_new / rr

    def below(self, rn, eps):
        return rn < self.dtype(eps)

    def sum(self, terms):
        if self.order is not None:
            terms = terms[np.random.default_rng(self.order + terms.size).permutation(terms.size)]
        return self.dtype(np.sum(terms))

    def store(self, old, new):
        """what a kernel leaves in an n-row buffer that held ``old``"""
        return new

    def dot_rows(self, Psi):
        return Psi

    def apply_rows(self, Psi):
        return Psi

    def reproject(self, r, Psi):
        return self.block_project(r, Psi)[0]

    def idle(self, state):
        """state after a call that found DONE set"""
        return state.copy()

    # -- helpers
    def arr(self, a):
        return np.array(a, dtype=self.dtype)

    def dot(self, x, y):
        return self.sum(self.arr(x) * self.arr(y))

    # -- vector phases
    def shift_dot(self, x, y, shift, skip=False, dot0=SENTINEL):
        """y' = y - fl(s x), x.y'"""
        x, y = self.arr(x), self.arr(y)
        if skip:
            return y, self.dtype(dot0)
        s = self.dtype(0.0 if shift is None else shift)
        y2 = self.store(y, y - s * x)
        return y2, self.dot(x, y2)

    def project_out(self, v, a):
        """out = v - fl((a.v) a), a.v"""
        v, a = self.arr(v), self.arr(a)
        c = self.dot(a, v)
        return self.store(v, v - c * a), c

    # -- CG phases
    def cg_init(self, b, Ax0, state0=None):
        """r = b - Ax0, d = r, state cleared, RR = r.r   (state0: what the state buffer held before; the call clears it)"""
        r = self.arr(b) - self.arr(Ax0)
        state = np.zeros(STATE_LEN, dtype=self.dtype)
        state[RR] = self.dot(r, r)
        return r, r.copy(), state

    def cg_init_check(self, state, eps):
        s = self.arr(state)
        rn = np.sqrt(s[RR])
        s[RESNORM] = rn
        s[DONE] = 1.0 if self.below(rn, eps) else 0.0
        s[ITERS] = 0.0
        return s

    def cg_update(self, x, r, d, Ad, state):
        x, r, d, Ad, s = self.arr(x), self.arr(r), self.arr(d), self.arr(Ad), self.arr(state)
        if s[DONE] != 0:
            return x, r, self.idle(s)
        alpha = s[RR] / s[DAD]
        x2 = self.store(x, x + alpha * d)
        r2 = self.store(r, r - alpha * Ad)
        s[RRNEW] = self.dot(r2, r2)
        return x2, r2, s

    def cg_check(self, state, eps):
        s = self.arr(state)
        if s[DONE] != 0:
            return self.idle(s)
        rr_new = s[RRNEW]
        rn = np.sqrt(rr_new)
        s[ITERS] += 1.0
        s[RESNORM] = rn
        if self.below(rn, eps):
            s[DONE] = 1.0
        else:
            s[BETA] = self.beta(rr_new, s[RR])
            s[RR] = rr_new
        return s

    def cg_direction(self, r, d, state):
        r, d, s = self.arr(r), self.arr(d), self.arr(state)
        if s[DONE] != 0:
            return d
        return self.store(d, r + s[BETA] * d)

    # -- fused step
    def _tail(self, r2, d, s, eps, parity):
        """the stop test on ||r2||, beta, the direction (k_cg_direction_fused)"""
        rr_new = self.dot(r2, r2)
        rr = s[self.cur(parity)]
        rn = np.sqrt(rr_new)
        s[ITERS] += 1.0
        s[RESNORM] = rn
        if self.below(rn, eps):
            s[DONE] = 1.0
            return d, s
        s[self.new(parity)] = rr_new
        beta = self.beta(rr_new, rr)
        return self.store(d, r2 + beta * d), s

    def cg_step(self, x, r, d, Ad, shift, state, eps, iteration):
        """one dsea_cg_step: Ad' = Ad - s d, alpha from the CURRENT rr slot (RRNEW if iteration is odd, else RR), update,
        stop test, beta, direction; the new rr goes to the OTHER slot"""
        x, r, d, Ad, s = self.arr(x), self.arr(r), self.arr(d), self.arr(Ad), self.arr(state)
        parity = int(iteration) & 1
        if s[DONE] != 0:
            return x, r, d, Ad, self.idle(s)
        Ad2, dAd = self.shift_dot(d, Ad, shift)
        alpha = s[self.cur(parity)] / dAd
        x2 = self.store(x, x + alpha * d)
        r2 = self.store(r, r - alpha * Ad2)
        d2, s = self._tail(r2, d, s, eps, parity)
        return x2, r2, d2, Ad2, s

    # -- deflation
    def block_project(self, v, Psi):
        """out = v - Psi^T (Psi v), and the m coefficients"""
        v, Psi = self.arr(v), self.arr(Psi)
        m = Psi.shape[0]
        coef = np.zeros(m, dtype=self.dtype)
        Pd = self.dot_rows(Psi)
        for j in range(Pd.shape[0]):
            coef[j] = self.dot(Pd[j], v)
        Pa = self.apply_rows(Psi)
        w = np.zeros_like(v)
        for j in range(Pd.shape[0]):
            w = w + coef[j] * Pa[j]
        return self.store(v, v - w), coef

    def deflated_init(self, b, x, Ax, shift, Psi, eps):
        b, x, Ax = self.arr(b), self.arr(x), self.arr(Ax)
        r0 = b - Ax if shift is None else b - (Ax - self.dtype(shift) * x)
        r = self.block_project(r0, Psi)[0]
        s = np.zeros(STATE_LEN, dtype=self.dtype)
        s[RR] = self.dot(r, r)
        s[RESNORM] = np.sqrt(s[RR])
        s[DONE] = 1.0 if self.below(s[RESNORM], eps) else 0.0
        return r, r.copy(), s

    def deflated_step(self, x, r, d, Ad, shift, Psi, state, eps, iteration):
        x, r, d, Ad, s = self.arr(x), self.arr(r), self.arr(d), self.arr(Ad), self.arr(state)
        parity = int(iteration) & 1
        if s[DONE] != 0:
            return x, r, d, Ad, self.idle(s)
        Ad2, dAd = self.shift_dot(d, Ad, shift)
        alpha = s[self.cur(parity)] / dAd
        x2 = self.store(x, x + alpha * d)
        r2 = self.reproject(self.store(r, r - alpha * Ad2), Psi)
        d2, s = self._tail(r2, d, s, eps, parity)
        return x2, r2, d2, Ad2, s


class Headroom(Reference):
    """fp64 evaluation of an exact-class case that asserts the class's premise on the way: every term of every sum is a
    multiple of 2^-12 and sum |terms| 2^12 < 2^53, so any partial sum in any order is exact"""

    def __init__(self):
        super().__init__(np.float64)
        self.largest = 0.0

    def sum(self, terms):
        scaled = terms * UNIT
        assert np.array_equal(scaled, np.rint(scaled)), "a term is no multiple of 2^-12"
        total = float(np.sum(np.abs(scaled)))
        assert total < 2.0 ** 53, "sum of |terms| is %.3g units of 2^-12: not exact in every order" % total
        self.largest = max(self.largest, total)
        return super().sum(terms)

    def block_project(self, v, Psi):
        out, coef = super().block_project(v, Psi)
        w = np.abs(coef) @ np.abs(np.asarray(Psi, dtype=np.float64))          # the FMA chain's partial sums stay below this
        assert float(np.max(w, initial=0.0)) * 64.0 < 2.0 ** 53
        return out, coef


def same(got, want):
    """bit for bit (the sign of a zero included)"""
    got = np.ascontiguousarray(np.atleast_1d(np.asarray(got, dtype=np.float64)))
    want = np.ascontiguousarray(np.atleast_1d(np.asarray(want, dtype=np.float64)))
    return got.shape == want.shape and bool(np.array_equal(got.view(np.int64), want.view(np.int64)))


PRE_BETA = {"shift_dot": (0, 1), "project_out": (0, 1), "cg_init": (0, 1), "cg_update": (0, 1), "cg_step": (0, 1, 3),
            "block_project": (0, 1), "deflated_init": (0, 1), "deflated_step": (0, 1, 3)}


def assert_headroom(stage, *args, prove=True):
    """run ``stage`` (a method name) on an exact-class case through Headroom (every sum of the stage -- all of them precede
    beta -- is exact in any order); with ``prove`` also require fp64 == longdouble bit for bit on every output that precedes
    beta (x', r', Ad', out, the coefficients: no elementwise operation rounded).  Returns the fp64 outputs and the largest
    sum of |terms| met, in units of 2^-12."""
    h = Headroom()
    got = getattr(h, stage)(*args)
    if prove:
        want = getattr(Reference(LD), stage)(*args)
        for i in PRE_BETA[stage]:
            assert np.array_equal(np.atleast_1d(got[i]).astype(LD), np.atleast_1d(want[i])), (stage, i)
    return got, h.largest


# ---- inputs -------------------------------------------------------------------------------------------------------------
def nonzero_head(v, value=3.0):
    if v[0] == 0:
        v[0] = value
    return v


def exact_D(n, seed):
    return np.random.default_rng(seed).integers(1, 5, size=n).astype(np.float64)


def random_D(n, seed):
    return 1.0 + 3.0 * np.random.default_rng(seed).random(n)


def exact_step_inputs(n, seed, shift, iteration, iters0=4.0):
    """(x, r, d, Ad, shift, state, eps, iteration) with alpha = 0.375 exactly; every slot the call must not write is SENTINEL"""
    x, r, d = exact_vector(n, seed), exact_vector(n, seed + 1), nonzero_head(exact_vector(n, seed + 2))
    Ad = exact_D(n, seed + 3) * d
    headroom(n, 4, 16 + 4)
    dAd = float(np.sum(d * (Ad - (shift or 0.0) * d)))
    assert dAd > 0
    state = np.full(STATE_LEN, SENTINEL)
    state[RRNEW if iteration & 1 else RR] = ALPHA_EXACT * dAd
    state[DONE], state[ITERS] = 0.0, iters0
    return x, r, d, Ad, shift, state, 1e-3, iteration


def random_step_inputs(n, seed, shift, iteration, iters0=4.0):
    from dominantsparseeigenad_amd.synthetic import normal_vector
    x, r, d = normal_vector(n, seed), normal_vector(n, seed + 1), normal_vector(n, seed + 2)
    Ad = random_D(n, seed + 3) * d
    state = np.full(STATE_LEN, SENTINEL)
    state[RRNEW if iteration & 1 else RR] = float(np.dot(r, r))
    state[DONE], state[ITERS] = 0.0, iters0
    return x, r, d, Ad, shift, state, 1e-9, iteration


def exact_psi(n, m, seed, rows=None):
    """integer entries in [-2, 2] on ``rows`` (None: every row), no zero row of Psi"""
    rng = np.random.default_rng(seed)
    Psi = np.zeros((m, n))
    rows = np.arange(n) if rows is None else rows
    Psi[:, rows] = rng.integers(-2, 3, size=(m, rows.size)).astype(np.float64)
    for j in range(m):
        if not Psi[j].any():
            Psi[j, rows[j % rows.size]] = 1.0
    return Psi


def exact_psi_for(stage, n, m, seed, make_args, prove=True):
    """the exact-class Psi of a case: support on every row where the headroom assertion allows it, else on ``edge_rows``.
    ``make_args(Psi)`` -> the stage's arguments.  Returns (Psi, 'all' | 'edges')."""
    Psi = exact_psi(n, m, seed)
    try:
        assert_headroom(stage, *make_args(Psi), prove=False)
        support = "all"
    except AssertionError:
        Psi, support = exact_psi(n, m, seed, edge_rows(n)), "edges"
    assert_headroom(stage, *make_args(Psi), prove=prove)
    return Psi, support


def orthonormal_psi(n, m, seed):
    from dominantsparseeigenad_amd.synthetic import normal_vector
    Q, _ = np.linalg.qr(normal_vector(n * m, seed).reshape(n, m))
    return np.ascontiguousarray(Q.T)


def tridiagonal(n, seed):
    """SPD tridiagonal (diagonal in [3, 4], off-diagonal 0.3 N(0, 1) clipped to 1): (apply(v) in fp64, dense matrix)"""
    rng = np.random.default_rng(seed)
    dg, off = 3.0 + rng.random(n), np.clip(0.3 * rng.standard_normal(n - 1), -1.0, 1.0)

    def apply(v):
        y = dg * v
        y[:-1] += off * v[1:]
        y[1:] += off * v[:-1]
        return y

    return apply, np.diag(dg) + np.diag(off, 1) + np.diag(off, -1)


# ---- judges of the random class (all on the call's own inputs and outputs; return {name: error / bound}) ---------------
def bit(got, want):
    return 0.0 if same(got, want) else np.inf


def sum_ratio(value, terms, n):
    """bound (b)"""
    terms = np.asarray(terms, dtype=LD)
    return worst_ratio(abs(LD(value) - np.sum(terms)), float((n + 4) * U * np.sum(np.abs(terms))))


def unchanged(state_in, state_out, slots):
    return bit(np.asarray(state_out)[list(slots)], np.asarray(state_in)[list(slots)])


def judge_shift_dot(x, y, shift, y2, dot):
    s = np.float64(0.0 if shift is None else shift)
    return {"y'": bit(y2, y - s * x), "x.y'": sum_ratio(dot, np.asarray(x, dtype=LD) * np.asarray(y2, dtype=LD), x.size)}


def judge_project_out(v, a, out, c):
    return {"a.v": sum_ratio(c, np.asarray(a, dtype=LD) * np.asarray(v, dtype=LD), v.size), "out": bit(out, v - np.float64(c) * a)}


def judge_cg_init(b, Ax0, r, d, state):
    rl = np.asarray(r, dtype=LD)
    others = [i for i in range(STATE_LEN) if i != RR]
    return {"r": bit(r, b - Ax0), "d": bit(d, r), "RR": sum_ratio(state[RR], rl * rl, b.size),
            "cleared": bit(state[others], np.zeros(len(others)))}


def judge_state(got, want):
    """scalar stages: the whole state against the fp64 mirror"""
    return {"state": bit(got, want)}


def judge_cg_update(x, r, d, Ad, state, x2, r2, state2):
    if state[DONE] != 0:
        return {"x": bit(x2, x), "r": bit(r2, r), "state": bit(state2, state)}
    alpha = np.float64(state[RR]) / np.float64(state[DAD])
    rl = np.asarray(r2, dtype=LD)
    return {"x'": bit(x2, x + alpha * d), "r'": bit(r2, r - alpha * Ad), "RRNEW": sum_ratio(state2[RRNEW], rl * rl, x.size),
            "other slots": unchanged(state, state2, [i for i in range(STATE_LEN) if i != RRNEW])}


def judge_cg_direction(r, d, state, d2):
    return {"d'": bit(d2, d if state[DONE] != 0 else r + np.float64(state[BETA]) * d)}


def alpha_bounds(d, Ad2, rr, n):
    """bound (c): (rr / S in longdouble, e_a + 2 u)"""
    t = np.asarray(d, dtype=LD) * np.asarray(Ad2, dtype=LD)
    S = np.sum(t)
    e_d = (n + 4) * U * np.sum(np.abs(t)) / abs(S)
    e_a = (e_d + U) / (1 - e_d - U)
    return LD(rr) / S, e_a + 2 * U


def judge_tail(tag, out, r2, d, d2, state, state2, eps, parity, n):
    """the stop test, the slots, beta and the direction of a fused step, from the downloaded slots"""
    cur, new = (RRNEW, RR) if parity else (RR, RRNEW)
    rl = np.asarray(r2, dtype=LD)
    T = np.sum(rl * rl)
    out[tag + "ITERS"] = bit(state2[ITERS], state[ITERS] + 1.0)
    keep = [DAD, ALPHA, BETA, cur]
    if state2[DONE] == 0:
        out[tag + "rr_new"] = sum_ratio(state2[new], rl * rl, n)
        out[tag + "RESNORM"] = bit(state2[RESNORM], np.sqrt(np.float64(state2[new])))
        out[tag + "stop"] = 0.0 if not (state2[RESNORM] < eps) else np.inf
        out[tag + "d'"] = bit(d2, r2 + (np.float64(state2[new]) / np.float64(state2[cur])) * d)
    else:
        keep = keep + [new]
        out[tag + "DONE"] = bit(state2[DONE], 1.0)
        out[tag + "stop"] = 0.0 if state2[RESNORM] < eps else np.inf
        out[tag + "RESNORM"] = worst_ratio(abs(LD(state2[RESNORM]) - np.sqrt(T)), float(((n + 4) / 2 + 2) * U * np.sqrt(T)))
        out[tag + "d kept"] = bit(d2, d)
    out[tag + "other slots"] = unchanged(state, state2, keep)
    return out


def judge_cg_step(x, r, d, Ad, shift, state, eps, iteration, x2, r2, d2, Ad2, state2):
    n, parity = x.size, int(iteration) & 1
    if state[DONE] != 0:
        return {"x": bit(x2, x), "r": bit(r2, r), "d": bit(d2, d), "Ad": bit(Ad2, Ad), "state": bit(state2, state)}
    out = {"Ad'": bit(Ad2, Ad - np.float64(0.0 if shift is None else shift) * d)}
    a, e = alpha_bounds(d, Ad2, state[RRNEW if parity else RR], n)
    ad, aA = a * np.asarray(d, dtype=LD), a * np.asarray(Ad2, dtype=LD)
    out["x'"] = worst_ratio(np.abs(x2 - (x + ad)), U * np.abs(x2) + np.abs(ad) * e)
    out["r'"] = worst_ratio(np.abs(r2 - (r - aA)), U * np.abs(r2) + np.abs(aA) * e)
    return judge_tail("", out, r2, d, d2, state, state2, eps, parity, n)


def project_bounds(V, B, Psi):
    """bound (d) with hidden coefficients: (V - Psi^T Psi V, c^, the part of the bound on out that does not depend on out)"""
    n, m = V.size, Psi.shape[0]
    P = np.asarray(Psi, dtype=LD)
    absP = np.abs(P)
    c = P @ V
    E = absP @ B + (n + 4) * U * (absP @ (np.abs(V) + B))
    fixed = B + absP.T @ E + (m + 1) * U * (absP.T @ (np.abs(c) + E))
    return V - P.T @ c, c, fixed


def judge_block_project(v, Psi, out, coef=None):
    n, m = v.size, Psi.shape[0]
    V, P = np.asarray(v, dtype=LD), np.asarray(Psi, dtype=LD)
    if coef is None:
        want, _, fixed = project_bounds(V, np.zeros(n, dtype=LD), Psi)
        return {"out": worst_ratio(np.abs(out - want), U * np.abs(out) + fixed)}
    c = np.asarray(coef, dtype=LD)
    res = {"coef": worst_ratio(np.abs(c - P @ V), (n + 4) * U * (np.abs(P) @ np.abs(V)))}
    res["out"] = worst_ratio(np.abs(out - (V - P.T @ c)), U * np.abs(out) + (m + 1) * U * (np.abs(P).T @ np.abs(c)))
    return res


def psi_dot_bound(Psi, c_hat, bound):
    """bound (e) on |psi_j . out|, out judged to ``bound`` componentwise against V - Psi^T c^"""
    P = np.asarray(Psi, dtype=LD)
    G = P @ P.T - np.eye(P.shape[0], dtype=LD)
    return np.abs(G) @ np.abs(c_hat) + np.abs(P) @ bound


def judge_deflated_init(b, x, Ax, shift, Psi, eps, r, d, state):
    n = b.size
    r0 = b - Ax if shift is None else b - (Ax - np.float64(shift) * x)
    want, c, fixed = project_bounds(np.asarray(r0, dtype=LD), np.zeros(n, dtype=LD), Psi)
    bound = U * np.abs(r) + fixed
    rl = np.asarray(r, dtype=LD)
    others = [DAD, RRNEW, ALPHA, BETA, ITERS]
    res = {"r": worst_ratio(np.abs(r - want), bound), "d": bit(d, r), "RR": sum_ratio(state[RR], rl * rl, n),
           "RESNORM": bit(state[RESNORM], np.sqrt(np.float64(state[RR]))), "DONE": bit(state[DONE], 1.0 if state[RESNORM] < eps else 0.0),
           "cleared": bit(state[others], np.zeros(len(others)))}
    bp = psi_dot_bound(Psi, c, bound)
    res["psi.r"] = worst_ratio(np.abs(np.asarray(Psi, dtype=LD) @ rl), bp)
    return res, bp


def judge_deflated_step(x, r, d, Ad, shift, Psi, state, eps, iteration, x2, r2, d2, Ad2, state2, psi_d_bound=None):
    """returns (ratios, bound on |psi_j . d'| for the next step of a chain or None)"""
    n, parity = x.size, int(iteration) & 1
    if state[DONE] != 0:
        return {"x": bit(x2, x), "r": bit(r2, r), "d": bit(d2, d), "Ad": bit(Ad2, Ad), "state": bit(state2, state)}, None
    out = {"Ad'": bit(Ad2, Ad - np.float64(0.0 if shift is None else shift) * d)}
    a, e = alpha_bounds(d, Ad2, state[RRNEW if parity else RR], n)
    ad, aA = a * np.asarray(d, dtype=LD), a * np.asarray(Ad2, dtype=LD)
    out["x'"] = worst_ratio(np.abs(x2 - (x + ad)), U * np.abs(x2) + np.abs(ad) * e)
    V = r - aA
    B = (U * np.abs(V) + np.abs(aA) * e) / (1 - U)
    want, c, fixed = project_bounds(V, B, Psi)
    bound = U * np.abs(r2) + fixed
    out["r' = P r~"] = worst_ratio(np.abs(r2 - want), bound)
    P = np.asarray(Psi, dtype=LD)
    br = psi_dot_bound(Psi, c, bound)
    out["psi.r'"] = worst_ratio(np.abs(P @ np.asarray(r2, dtype=LD)), br)
    judge_tail("", out, r2, d, d2, state, state2, eps, parity, n)
    bd = None
    if psi_d_bound is not None and state2[DONE] == 0:
        new, cur = (RR, RRNEW) if parity else (RRNEW, RR)
        beta = abs(LD(np.float64(state2[new]) / np.float64(state2[cur])))
        bd = br + beta * psi_d_bound + U * (np.abs(P) @ (np.abs(np.asarray(d2, dtype=LD)) + beta * np.abs(np.asarray(d, dtype=LD))))
        out["psi.d'"] = worst_ratio(np.abs(P @ np.asarray(d2, dtype=LD)), bd)
    return out, bd


# ---- the checks: one implementation of the eleven entries through both classes -----------------------------------------
class Checks:
    """``impl`` has the methods of Reference (numpy in, numpy out: the GPU test's implementation makes one library call per
    method).  Every check raises AssertionError where a verdict fails and returns the worst ratio of the random class."""

    def __init__(self, impl, log=print, prove=True):
        """``prove``: also compare every exact-class case's fp64 reference with longdouble (the CPU test does; the GPU test
        leaves that to the CPU test and keeps the assertion on the sums)"""
        self.impl, self.log, self.prove, self.mirror = impl, log, prove, Reference(np.float64)

    def headroom(self, stage, *args):
        return assert_headroom(stage, *args, prove=self.prove)[0]

    def psi(self, stage, n, m, seed, make_args):
        return exact_psi_for(stage, n, m, seed, make_args, prove=self.prove)

    # -- verdicts
    def exact(self, tag, got, want):
        names = "abcdefgh"
        got = got if isinstance(got, tuple) else (got,)
        want = want if isinstance(want, tuple) else (want,)
        for i, (g, w) in enumerate(zip(got, want)):
            if g is None and w is None:
                continue
            assert same(g, w), "%s: output %s differs from the fp64 reference in %d of %d places (exact class)" % (
                tag, names[i], int(np.sum(np.atleast_1d(g) != np.atleast_1d(w))), np.size(w))

    def ratios(self, tag, res):
        worst = max(res.values()) if res else 0.0
        bad = {k: v for k, v in res.items() if not v <= 1.0}
        assert not bad, "%s: %s" % (tag, bad)
        return float(worst)

    def report(self, tag, worst):
        self.log("%s: exact class bit for bit; random class worst error / bound = %.3f" % (tag, worst))
        return worst

    # -- vector phases
    def shift_dot(self, n, random=True):
        x = exact_vector(n, 11 + n)
        y = exact_D(n, 12 + n) * exact_vector(n, 13 + n)
        worst = 0.0
        for shift in (SHIFT_EXACT, None):
            want = self.headroom("shift_dot", x, y, shift)
            self.exact("shift_dot n=%d shift=%s" % (n, shift), self.impl.shift_dot(x, y, shift), want)
        got = self.impl.shift_dot(x, y, SHIFT_EXACT, skip=True, dot0=SENTINEL)
        self.exact("shift_dot n=%d skip flag" % n, got, (y, SENTINEL))
        if random:
            from dominantsparseeigenad_amd.synthetic import normal_vector
            xr, yr = normal_vector(n, 14 + n), normal_vector(n, 15 + n)
            for shift in (SHIFT_RANDOM, None):
                y2, dot = self.impl.shift_dot(xr, yr, shift)
                worst = max(worst, self.ratios("shift_dot n=%d shift=%s" % (n, shift), judge_shift_dot(xr, yr, shift, y2, dot)))
        return self.report("shift_dot n=%d" % n, worst)

    def project_out(self, n, random=True):
        v = exact_vector(n, 21 + n)
        a = np.random.default_rng(22 + n).integers(-2, 3, size=n).astype(np.float64)
        want = self.headroom("project_out", v, a)
        self.exact("project_out n=%d" % n, self.impl.project_out(v, a), want)
        worst = 0.0
        if random:
            from dominantsparseeigenad_amd.synthetic import normal_vector
            vr, ar = normal_vector(n, 23 + n), normal_vector(n, 24 + n)
            ar = ar / np.sqrt(np.dot(ar, ar))
            out, c = self.impl.project_out(vr, ar)
            worst = self.ratios("project_out n=%d" % n, judge_project_out(vr, ar, out, c))
        return self.report("project_out n=%d" % n, worst)

    # -- unfused CG phases
    def cg_init(self, n, random=True):
        b, Ax0 = exact_vector(n, 31 + n), exact_D(n, 32 + n) * exact_vector(n, 33 + n)
        state0 = np.full(STATE_LEN, SENTINEL)
        want = self.headroom("cg_init", b, Ax0)
        self.exact("cg_init n=%d" % n, self.impl.cg_init(b, Ax0, state0), want)
        worst = 0.0
        if random:
            from dominantsparseeigenad_amd.synthetic import normal_vector
            br, Ar = normal_vector(n, 34 + n), normal_vector(n, 35 + n)
            worst = self.ratios("cg_init n=%d" % n, judge_cg_init(br, Ar, *self.impl.cg_init(br, Ar, state0)))
        return self.report("cg_init n=%d" % n, worst)

    def cg_init_check(self):
        for rr, eps in ((4.0, 2.0), (4.0, np.nextafter(2.0, np.inf)), (0.7310585786300049, 1e-7), (0.0, 1e-7)):
            state = np.full(STATE_LEN, SENTINEL)
            state[RR] = rr
            got = self.impl.cg_init_check(state, eps)
            self.exact("cg_init_check rr=%r eps=%r" % (rr, eps), got, self.mirror.cg_init_check(state, eps))
        state = np.full(STATE_LEN, SENTINEL)
        state[RR] = 4.0
        assert self.impl.cg_init_check(state, 2.0)[DONE] == 0.0, "||r|| = eps is not converged (CG.py:28: <)"
        assert self.impl.cg_init_check(state, np.nextafter(2.0, np.inf))[DONE] == 1.0
        return 0.0

    def cg_update(self, n, random=True):
        x, r, d = exact_vector(n, 41 + n), exact_vector(n, 42 + n), nonzero_head(exact_vector(n, 43 + n))
        Ad = exact_D(n, 44 + n) * d
        state = np.full(STATE_LEN, SENTINEL)
        state[DAD] = float(np.sum(d * Ad))
        state[RR], state[DONE] = ALPHA_EXACT * state[DAD], 0.0
        want = self.headroom("cg_update", x, r, d, Ad, state)
        self.exact("cg_update n=%d" % n, self.impl.cg_update(x, r, d, Ad, state), want)
        done = state.copy()
        done[DONE] = 1.0
        self.exact("cg_update n=%d with DONE set" % n, self.impl.cg_update(x, r, d, Ad, done), (x, r, done))
        worst = 0.0
        if random:
            xr, rr_, dr, Adr, _, st, _, _ = random_step_inputs(n, 45 + n, None, 0)
            st[DAD] = float(np.dot(dr, Adr))
            worst = self.ratios("cg_update n=%d" % n, judge_cg_update(xr, rr_, dr, Adr, st, *self.impl.cg_update(xr, rr_, dr, Adr, st)))
        return self.report("cg_update n=%d" % n, worst)

    def cg_check(self):
        base = np.full(STATE_LEN, SENTINEL)
        base[RR], base[RRNEW], base[DONE], base[ITERS] = 3.0, 1.7, 0.0, 6.0
        cases = [("iterating", base, 1e-7)]
        conv = base.copy()
        conv[RRNEW] = 1e-20
        cases.append(("converged", conv, 1e-7))
        done = base.copy()
        done[DONE] = 1.0
        cases.append(("DONE set", done, 1e-7))
        edge = base.copy()
        edge[RRNEW] = 4.0
        cases += [("||r|| = eps", edge, 2.0), ("||r|| just below eps", edge, float(np.nextafter(2.0, np.inf)))]
        for name, state, eps in cases:
            self.exact("cg_check %s" % name, self.impl.cg_check(state, eps), self.mirror.cg_check(state, eps))
        got = self.impl.cg_check(conv, 1e-7)
        assert got[RR] == 3.0 and got[BETA] == SENTINEL and got[DONE] == 1.0 and got[ITERS] == 7.0, got
        assert self.impl.cg_check(edge, 2.0)[DONE] == 0.0 and self.impl.cg_check(edge, float(np.nextafter(2.0, np.inf)))[DONE] == 1.0
        return 0.0

    def cg_direction(self, n, random=True):
        r, d = eighths(n, 51 + n, span=256) / 8.0, exact_vector(n, 52 + n)
        state = np.full(STATE_LEN, SENTINEL)
        state[BETA], state[DONE] = 0.375, 0.0
        self.exact("cg_direction n=%d" % n, self.impl.cg_direction(r, d, state), self.mirror.cg_direction(r, d, state))
        done = state.copy()
        done[DONE] = 1.0
        self.exact("cg_direction n=%d with DONE set" % n, self.impl.cg_direction(r, d, done), d)
        worst = 0.0
        if random:
            from dominantsparseeigenad_amd.synthetic import normal_vector
            rr_, dr = normal_vector(n, 53 + n), normal_vector(n, 54 + n)
            state[BETA] = 0.8414709848078965
            worst = self.ratios("cg_direction n=%d" % n, judge_cg_direction(rr_, dr, state, self.impl.cg_direction(rr_, dr, state)))
        return self.report("cg_direction n=%d" % n, worst)

    # -- fused step
    def step_combos(self, n):
        """(iteration, shift) of the exact class: all eight up to 4097 rows, four beyond (every iteration, both shifts)"""
        if n <= 4097:
            return [(it, sh) for it in (0, 1, 2, 7) for sh in (SHIFT_EXACT, None)]
        return [(0, SHIFT_EXACT), (1, None), (2, None), (7, SHIFT_EXACT)]

    def cg_step(self, n, random=True):
        worst = 0.0
        for it, shift in self.step_combos(n):
            args = exact_step_inputs(n, 61 + n + it, shift, it)
            want = self.headroom("cg_step", *args)
            tag = "cg_step n=%d iteration=%d shift=%s" % (n, it, shift)
            got = self.impl.cg_step(*args)
            self.exact(tag, got, want)
            new = RR if it & 1 else RRNEW
            assert args[5][new] == SENTINEL and got[4][new] == want[4][new] != SENTINEL and got[4][ITERS] == 5.0, tag
        if random:
            for it, shift in ((0, SHIFT_RANDOM), (1, SHIFT_RANDOM), (2, None)) if n <= 4097 else ((1, SHIFT_RANDOM),):
                args = random_step_inputs(n, 71 + n + it, shift, it)
                worst = max(worst, self.ratios("cg_step n=%d iteration=%d shift=%s" % (n, it, shift),
                                               judge_cg_step(*args, *self.impl.cg_step(*args))))
        return self.report("cg_step n=%d" % n, worst)

    def cg_step_converged_and_done(self, n):
        """r = 0.375 Ad' makes r' = 0: x and r updated, d untouched, DONE = 1, ITERS + 1, the other rr slot not written;
        and with DONE set on entry the whole call is a no-op, Ad included"""
        for it, shift in ((0, SHIFT_EXACT), (1, None)):
            x, _, d, Ad, _, state, eps, _ = exact_step_inputs(n, 81 + n + it, shift, it)
            r = ALPHA_EXACT * (Ad - (shift or 0.0) * d)
            args = (x, r, d, Ad, shift, state, eps, it)
            want = self.headroom("cg_step", *args)
            tag = "cg_step n=%d iteration=%d converged" % (n, it)
            got = self.impl.cg_step(*args)
            self.exact(tag, got, want)
            new = RR if it & 1 else RRNEW
            assert not got[1].any() and same(got[2], d) and got[4][DONE] == 1.0 and got[4][ITERS] == 5.0 and got[4][new] == SENTINEL, tag
            self.ratios(tag, judge_cg_step(*args, *got))
            done = state.copy()
            done[DONE] = 1.0
            args = (x, r, d, Ad, shift, done, eps, it)
            self.exact("cg_step n=%d iteration=%d with DONE set" % (n, it), self.impl.cg_step(*args), (x, r, d, Ad, done))
        return 0.0

    def cg_step_strict(self, step="cg_step", Psi=None):
        """n = 2, rr_new = 4.0 exactly: eps = 2.0 is not a stop, the next double above is"""
        x, r, d, Ad = np.array([1.0, -2.0]), np.array([5.0, 3.0]), np.array([1.0, 1.0]), np.array([8.0, 8.0])
        extra = () if Psi is None else (Psi,)
        for it in (0, 1):
            state = np.full(STATE_LEN, SENTINEL)
            state[RRNEW if it else RR], state[DONE], state[ITERS] = 6.0, 0.0, 0.0
            for eps, done in ((2.0, 0.0), (float(np.nextafter(2.0, np.inf)), 1.0)):
                args = (x, r, d, Ad, None) + extra + (state, eps, it)
                got = getattr(self.impl, step)(*args)
                self.exact("%s strictness eps=%r" % (step, eps), got, getattr(self.mirror, step)(*args))
                assert same(got[1], [2.0, 0.0]) and got[4][RESNORM] == 2.0 and got[4][DONE] == done, (step, eps, got)
        return 0.0

    def cg_step_chain(self, n=513, steps=6):
        """cg_init, cg_init_check and six cg_step calls on an SPD tridiagonal system, the mat-vec done here between calls;
        every step judged from the implementation's own previous outputs"""
        from dominantsparseeigenad_amd.synthetic import normal_vector
        apply, _ = tridiagonal(n, 7)
        b, x = normal_vector(n, 91), normal_vector(n, 92)
        eps = 1e-13
        Ax = apply(x)
        r, d, state = self.impl.cg_init(b, Ax, np.full(STATE_LEN, SENTINEL))
        self.ratios("chain: cg_init", judge_cg_init(b, Ax, r, d, state))
        s2 = self.impl.cg_init_check(state, eps)
        self.exact("chain: cg_init_check", s2, self.mirror.cg_init_check(state, eps))
        state, worst = s2, 0.0
        for it in range(steps):
            args = (x, r, d, apply(d), -0.25, state, eps, it)
            got = self.impl.cg_step(*args)
            worst = max(worst, self.ratios("chain: cg_step %d" % it, judge_cg_step(*args, *got)))
            x, r, d, _, state = got
            assert state[ITERS] == it + 1.0 and state[DONE] == 0.0, (it, state)
        return self.report("cg_step chain n=%d" % n, worst)

    # -- deflation
    def block_project(self, n, m, random=True):
        v = exact_vector(n, 101 + n + m)
        Psi, support = self.psi("block_project", n, m, 102 + n + m, lambda P: (v, P))
        want = self.mirror.block_project(v, Psi)
        tag = "block_project n=%d m=%d (Psi on %s rows)" % (n, m, support)
        self.exact(tag, self.impl.block_project(v, Psi), want)
        self.exact(tag + " in place", self.impl.block_project(v, Psi, inplace=True), want)
        self.exact(tag + " coef_out null", self.impl.block_project(v, Psi, inplace=True, coef=False), (want[0], None))
        worst = 0.0
        if random:
            from dominantsparseeigenad_amd.synthetic import normal_vector
            vr, Pr = normal_vector(n, 103 + n + m), orthonormal_psi(n, m, 104 + n + m)
            out, coef = self.impl.block_project(vr, Pr, inplace=True)
            worst = self.ratios(tag, judge_block_project(vr, Pr, out, coef))
            out, _ = self.impl.block_project(vr, Pr, coef=False)
            worst = max(worst, self.ratios(tag + " coef_out null", judge_block_project(vr, Pr, out)))
        return self.report(tag, worst)

    def deflated_init(self, n, m, random=True):
        b, x = exact_vector(n, 111 + n + m), exact_vector(n, 112 + n + m)
        Ax = exact_D(n, 113 + n + m) * x
        worst, support = 0.0, "all"
        for shift in (SHIFT_EXACT, None):
            Psi, support = self.psi("deflated_init", n, m, 114 + n + m, lambda P: (b, x, Ax, shift, P, 1e-3))
            tag = "deflated_init n=%d m=%d shift=%s (Psi on %s rows)" % (n, m, shift, support)
            want = self.mirror.deflated_init(b, x, Ax, shift, Psi, 1e-3)
            got = self.impl.deflated_init(b, x, Ax, shift, Psi, 1e-3)
            self.exact(tag, got, want)
            assert same(got[1], got[0]), tag
            rn = float(got[2][RESNORM])
            if rn > 0:                      # DONE from eps on both sides of ||r||
                for eps, done in ((rn, 0.0), (float(np.nextafter(rn, np.inf)), 1.0)):
                    got = self.impl.deflated_init(b, x, Ax, shift, Psi, eps)
                    self.exact(tag + " eps=%r" % eps, got, self.mirror.deflated_init(b, x, Ax, shift, Psi, eps))
                    assert got[2][DONE] == done and got[2][ITERS] == 0.0, (tag, eps, got[2])
        if random:
            from dominantsparseeigenad_amd.synthetic import normal_vector
            br, xr = normal_vector(n, 115 + n + m), normal_vector(n, 116 + n + m)
            Axr, Pr = random_D(n, 117 + n + m) * xr, orthonormal_psi(n, m, 118 + n + m)
            for shift in (SHIFT_RANDOM, None):
                res, _ = judge_deflated_init(br, xr, Axr, shift, Pr, 1e-9, *self.impl.deflated_init(br, xr, Axr, shift, Pr, 1e-9))
                worst = max(worst, self.ratios("deflated_init n=%d m=%d shift=%s" % (n, m, shift), res))
        return self.report("deflated_init n=%d m=%d (Psi on %s rows)" % (n, m, support), worst)

    def deflated_step(self, n, m, random=True):
        worst, support = 0.0, "all"
        for it, shift in ((0, SHIFT_EXACT), (1, None)):
            x, r, d, Ad, _, state, eps, _ = exact_step_inputs(n, 121 + n + m + it, shift, it)
            Psi, support = self.psi("deflated_step", n, m, 122 + n + m,
                                         lambda P: (x, r, d, Ad, shift, P, state, eps, it))
            tag = "deflated_step n=%d m=%d iteration=%d shift=%s (Psi on %s rows)" % (n, m, it, shift, support)
            args = (x, r, d, Ad, shift, Psi, state, eps, it)
            want = self.mirror.deflated_step(*args)
            got = self.impl.deflated_step(*args)
            self.exact(tag, got, want)
            new = RR if it & 1 else RRNEW
            assert got[4][new] != SENTINEL and got[4][ITERS] == 5.0 and got[4][DONE] == 0.0, tag
            # converged: r = 0.375 Ad' -> r~ = 0 = P r~; then the same call with DONE set
            rc = ALPHA_EXACT * (Ad - (shift or 0.0) * d)
            args = (x, rc, d, Ad, shift, Psi, state, eps, it)
            got = self.impl.deflated_step(*args)
            self.exact(tag + " converged", got, self.mirror.deflated_step(*args))
            assert not got[1].any() and same(got[2], d) and got[4][DONE] == 1.0 and got[4][ITERS] == 5.0 and got[4][new] == SENTINEL, tag
            done = state.copy()
            done[DONE] = 1.0
            args = (x, r, d, Ad, shift, Psi, done, eps, it)
            self.exact(tag + " with DONE set", self.impl.deflated_step(*args), (x, r, d, Ad, done))
        if random:
            Pr = orthonormal_psi(n, m, 123 + n + m)
            for it, shift in ((0, SHIFT_RANDOM), (1, None)) if n <= 4097 else ((1, SHIFT_RANDOM),):
                x, r, d, Ad, _, state, eps, _ = random_step_inputs(n, 124 + n + m + it, shift, it)
                args = (x, r, d, Ad, shift, Pr, state, eps, it)
                res, _ = judge_deflated_step(*args, *self.impl.deflated_step(*args))
                worst = max(worst, self.ratios("deflated_step n=%d m=%d iteration=%d" % (n, m, it), res))
        return self.report("deflated_step n=%d m=%d (Psi on %s rows)" % (n, m, support), worst)

    def deflated_strict(self):
        """the same two-row case through dsea_cg_deflated_step: Psi = (0, 1) and r~ = (2, 0), which the projection keeps"""
        return self.cg_step_strict("deflated_step", np.array([[0.0, 1.0]]))

    def deflated_chain(self, n=513, m=3, steps=6):
        """block_project (in place), deflated_init and six deflated_step calls, the mat-vec done here; every step judged from
        the implementation's own previous outputs, |Psi r| and |Psi d| held to bound (e) after every step"""
        from dominantsparseeigenad_amd.synthetic import normal_vector
        apply, _ = tridiagonal(n, 8)
        Psi = orthonormal_psi(n, m, 131)
        b, x0 = normal_vector(n, 132), normal_vector(n, 133)
        shift, eps = -0.25, 1e-13
        x, coef = self.impl.block_project(x0, Psi, inplace=True)
        worst = self.ratios("chain: block_project", judge_block_project(x0, Psi, x, coef))
        Ax = apply(x)
        r, d, state = self.impl.deflated_init(b, x, Ax, shift, Psi, eps)
        res, bd = judge_deflated_init(b, x, Ax, shift, Psi, eps, r, d, state)
        worst = max(worst, self.ratios("chain: deflated_init", res))
        for it in range(steps):
            args = (x, r, d, apply(d), shift, Psi, state, eps, it)
            got = self.impl.deflated_step(*args)
            res, bd = judge_deflated_step(*args, *got, psi_d_bound=bd)
            assert "psi.d'" in res and "psi.r'" in res
            worst = max(worst, self.ratios("chain: deflated_step %d" % it, res))
            x, r, d, _, state = got
            assert state[ITERS] == it + 1.0 and state[DONE] == 0.0, (it, state)
        return self.report("deflated_step chain n=%d m=%d" % (n, m), worst)


    def all(self, n, m, random=True):
        """every check that takes a size, and the scalar ones; the worst ratio"""
        runs = [lambda: self.shift_dot(n, random), lambda: self.project_out(n, random), lambda: self.cg_init(n, random),
                self.cg_init_check, lambda: self.cg_update(n, random), self.cg_check, lambda: self.cg_direction(n, random),
                lambda: self.cg_step(n, random), lambda: self.cg_step_converged_and_done(n), self.cg_step_strict,
                lambda: self.block_project(n, m, random), lambda: self.deflated_init(n, m, random),
                lambda: self.deflated_step(n, m, random), self.deflated_strict]
        return max(run() for run in runs)


# ---- wrong kernels: each breaks one rule of Reference ------------------------------------------------------------------
def _mutant(name, **methods):
    return type(name, (Reference,), methods)


def _drop_last_from_sum(self, terms):
    return Reference.sum(self, terms[:-1] if terms.size & 1 else terms)


def _drop_last_from_store(self, old, new):
    if new.size & 1:
        new = new.copy()
        new[-1] = old[-1]
    return new


def _drop_one_block(self, terms):
    """the partial of the last 512-row tile never reaches the sum"""
    last = (terms.size - 1) // TILE * TILE
    return Reference.sum(self, terms[:last])


def _swap_rows(self, Psi):
    Psi = Psi.copy()
    Psi[[0, 1]] = Psi[[1, 0]]
    return Psi


def _check_slot_first(self, state, eps):
    """cg_check with RR overwritten before beta is formed"""
    s = self.arr(state)
    if s[DONE] != 0:
        return s
    rn = np.sqrt(s[RRNEW])
    s[ITERS] += 1.0
    s[RESNORM] = rn
    if rn < eps:
        s[DONE] = 1.0
    else:
        s[RR] = s[RRNEW]
        s[BETA] = s[RRNEW] / s[RR]
    return s


def _stale_beta_tail(self, r2, d, s, eps, parity):
    """the fused tail with beta formed from the new slot BEFORE that slot is updated"""
    stale = s[self.new(parity)]
    d2, s = Reference._tail(self, r2, d, s, eps, parity)
    if s[DONE] == 0:
        d2 = r2 + (stale / s[self.cur(parity)]) * d
    return d2, s


def _idle_counts(self, state):
    s = state.copy()
    s[ITERS] += 1.0
    return s


MUTANTS = {
    "the wrong parity slot is read": _mutant("WrongSlotRead", cur=lambda self, parity: RR if parity else RRNEW),
    "the new rr is written to the current slot": _mutant("WrongSlotWritten", new=lambda self, parity: RRNEW if parity else RR),
    "beta is inverted": _mutant("BetaInverted", beta=lambda self, rr_new, rr: rr / rr_new),
    "beta is formed after RR was overwritten (cg_check)": _mutant("CheckSlotFirst", cg_check=_check_slot_first),
    "beta is formed from the new slot before its update (fused tail)": _mutant("StaleBeta", _tail=_stale_beta_tail),
    "the last row of an odd n is dropped from a sum": _mutant("LastRowSum", sum=_drop_last_from_sum),
    "the last row of an odd n is dropped from a store": _mutant("LastRowStore", store=_drop_last_from_store),
    "one partial block is dropped": _mutant("BlockDropped", sum=_drop_one_block),
    "Psi rows j and j + 1 are swapped in the apply": _mutant("RowsSwapped", apply_rows=_swap_rows),
    "m - 1 rows are used in place of m": _mutant("RowMissing", dot_rows=lambda self, Psi: Psi[:-1]),
    "the re-projection is skipped": _mutant("NoReprojection", reproject=lambda self, r, Psi: r),
    "ITERS is incremented on a no-op": _mutant("IdleCounts", idle=_idle_counts),
    "the stop is decided with <= in place of <": _mutant("StopNotStrict", below=lambda self, rn, eps: rn <= self.dtype(eps)),
}


class HostImpl:
    """a Reference behind the interface Checks drives (what the GPU test's implementation offers around the library)"""

    def __init__(self, ref):
        self.ref = ref

    @staticmethod
    def _f64(out):
        if isinstance(out, tuple):
            return tuple(np.asarray(o, dtype=np.float64) if np.ndim(o) else float(o) for o in out)
        return np.asarray(out, dtype=np.float64)

    def __getattr__(self, name):
        fn = getattr(self.ref, name)
        return lambda *a, **k: self._f64(fn(*a, **k))

    def block_project(self, v, Psi, inplace=False, coef=True):
        out, c = self._f64(self.ref.block_project(v, Psi))
        return out, (c if coef else None)
