"""numpy reference, input classes and operation-counted error bounds of the Arnoldi step and the GMRES cycle
(tests/test_gpu_krylov_stages.py on the device, proved on the CPU by tests/test_krylov_reference_cpu.py); no GPU, no torch.

THE STEP (include/dsea.h dsea_arnoldi_orth / dsea_arnoldi_extend, csrc/dsea_krylov.hip "Arnoldi step scalars"), with V = the
j + 1 given rows -- orthonormal or not: the step is defined by its arithmetic, not by a property of V:
    w  = u - shift v_j                       ww   = ||w||^2
    c1 = V w   (classical Gram-Schmidt)      w1   = w - V^T c1          nrm1 = ||w1||^2
    second pass iff nrm1 < 0.5 ww:           c2   = V w1, w2 = w1 - V^T c2, h = c1 + c2, nrm = ||w2||^2   (else h = c1, nrm = nrm1)
    beta = sqrt(nrm), h[j+1] = beta          dead iff not beta > 1e-13 sqrt(ww);  v_next = w_k / beta unless dead

TWO INPUT CLASSES, TWO VERDICTS (as tests/matvec_reference.py)
  exact     V rows are signed coordinate vectors, u is integer valued, shift = 0.375 = 3/8: every product and every partial sum
            is a multiple of 1/8 far below 2^53 / 8 (``headroom``), nrm a power of 4, so beta = 2^p and w / beta are exact --
            bit equality whatever the summation order.
  random    orthonormal rows built in np.longdouble and rounded once, three kinds of u (``random_step``).  Verdict: the
            componentwise bounds of ``step_bounds``, which count operations (u = 2^-53) and know nothing of the reduction tree.
            Both decisions of the step (second pass, dead) are kept a factor 4 away from their thresholds by the builder.
"""
import functools

import numpy as np

from matvec_reference import LD, U, exact_vector, headroom, worst_ratio  # noqa: F401  (re-exported for the tests)

BREAK_TOL = 1e-13
SHIFT_EXACT, SHIFT_RANDOM = 0.375, 0.6180339887498949
MARGIN = 4.0
# nrm1 <= ww always, so nrm1 / (0.5 ww) <= 2: on the side "no second pass" a factor 4 does not exist; the builder asks for three
# quarters of what does (the device's nrm1 and ww are within ~n u, 1e-10 at the largest n, of the reference's)
MARGIN_NO_SECOND = 1.5
J_LONG = 300                           # at n = 129, kmax = 302: the second trip of the hcol loop (rows beyond 255)
# n of the one-step cases and why (docs/design/17-krylov-stage-tests.md)
STEP_N = (1, 2, 3, 127, 129, 4097, 32898, 82178, 131202, 262146, 524290)
N_CAPPED = (1 << 22) + 2050            # rpl 16, capped grid: exact class only
STEP_J = (0, 1, 15, 16, 17, 40)


def step_js(n):
    """the j of the one-step cases at n: j + 2 <= n (a next vector exists), j <= 2 from n = 262146 up"""
    js = [j for j in STEP_J if j + 2 <= n or (j == 0 and n == 1)]
    return [j for j in js if j <= 2] if n >= 262146 else js


# ---- summation orders (the CPU twin runs the same algorithm under each) ------------------------------------------------
def sum_forward(p):
    acc = p.dtype.type(0)
    if p.size <= 4096:
        for v in p:
            acc = acc + v
        return acc
    return np.cumsum(p)[-1]                      # (sequential, left to right)


def sum_reversed(p):
    return sum_forward(p[::-1])


def sum_pairwise(p):
    p = np.array(p)
    while p.size > 1:
        if p.size % 2:
            p = np.concatenate((p, [p.dtype.type(0)]))
        p = p[0::2] + p[1::2]
    return p[0] if p.size else p.dtype.type(0)


ORDERS = {"forward": sum_forward, "reversed": sum_reversed, "pairwise": sum_pairwise}


class Step:
    pass


def _dots(V, w, summ):
    if summ is None:
        return V @ w
    return np.array([summ(V[t] * w) for t in range(V.shape[0])], dtype=w.dtype)


def _nrm2(w, summ):
    return np.sum(w * w) if summ is None else summ(w * w)


def _combine(V, c, summ):
    """V^T c, terms added in row order (any order of the j + 1 terms is within the bound)"""
    if summ is None:
        return c @ V
    acc = np.zeros(V.shape[1], dtype=c.dtype)
    for t in range(V.shape[0]):
        acc = acc + c[t] * V[t]
    return acc


def arnoldi_step(Vrows, u, shift, dtype=LD, summ=None):
    """one step as specified above, in ``dtype``; Vrows = V[0..j] (j + 1 rows), v_j the last.  ``summ``: None (numpy's own
    sums -- the reference) or one of ORDERS (the CPU twin).  Returns a Step: h[0..j+1], v_next (None when dead), second, dead,
    margin_dgks = nrm1 / (0.5 ww), margin_dead = beta / (1e-13 sqrt(ww)) (inf for ww == 0 == beta: 0 > 0 is false -- dead),
    and the intermediates the bounds need."""
    V = np.asarray(Vrows, dtype=dtype)
    s = Step()
    s.V = V
    s.j = V.shape[0] - 1
    s.w = np.asarray(u, dtype=dtype) - dtype(shift) * V[-1]
    s.ww = _nrm2(s.w, summ)
    s.c1 = _dots(V, s.w, summ)
    s.w1 = s.w - _combine(V, s.c1, summ)
    s.nrm1 = _nrm2(s.w1, summ)
    s.second = bool(s.nrm1 < dtype(0.5) * s.ww)
    s.c2 = np.zeros_like(s.c1)
    s.wk, nrm = s.w1, s.nrm1
    if s.second:
        s.c2 = _dots(V, s.w1, summ)
        s.wk = s.w1 - _combine(V, s.c2, summ)
        nrm = _nrm2(s.wk, summ)
    s.beta = np.sqrt(nrm)
    scale = np.sqrt(s.ww)
    s.dead = not bool(s.beta > dtype(BREAK_TOL) * scale)
    s.h = np.concatenate((s.c1 + s.c2 if s.second else s.c1, [s.beta]))
    s.v_next = None if s.dead else s.wk / s.beta
    s.margin_dgks = float(s.nrm1 / (dtype(0.5) * s.ww)) if s.ww > 0 else np.inf
    s.margin_dead = float(s.beta / (dtype(BREAK_TOL) * scale)) if scale > 0 else (np.inf if s.beta > 0 else 0.0)
    return s


def step_bounds(Vrows, u, shift, ref, u_err=None):
    """Componentwise first-order bounds for a fp64 evaluation of the step (ANY summation order, FMA or not) against the
    longdouble Step ``ref``.  i = j + 1 rows, a = |u| + |shift v_j| >= |w|, |V| = absolute rows, u = 2^-53.  ``u_err``: a
    componentwise bound on the error of the given u itself (the mat-vec bound when u came from the device's mat-vec).

      dw   = 2 u a + u_err                                  w = u - shift v_j: a product and a difference
      dc1  = (n + 4) u |V| a + |V| u_err                    a dot of n terms errs by gamma_n sum |v_t||w^|, w^ <= a (1 + 2u);
                                                            the perturbation dw adds 2 u |V| a; 2 u of slack for second order
      E1   = dw + |V|^T dc1 + (i + 2) u (a + |V|^T |c1|)    w1 = w - sum_t c1_t v_t: i products, i subtractions
      no second pass:  dh_t = dc1_t, E = E1
      second pass:     dc2  = |V| E1 + (n + 2) u |V| (|w1| + E1)              c2 = V w1^, w1^ within E1 of w1
                       dh_t = dc1_t + dc2_t + u (|c1_t| + |c2_t|)             h = c1 + c2: one more rounding
                       E    = E1 + |V|^T dc2 + (i + 2) u (|w1| + E1 + |V|^T (|c2| + dc2))
      dbeta = ||E||_2 + (n / 2 + 3) u (beta + ||E||_2)      | ||w^|| - ||w|| | <= ||E||_2; the sum of squares errs by
                                                            gamma_(n+1) relatively, the root halves it and rounds once
      dv   = E / beta + |w_k| dbeta / beta^2 + 2 u |w_k| / beta     v = w_k / beta: both perturbations and the division
    dv grows with ||w|| / beta: E is proportional to the size of w, beta is what the projection left of it.
    The orthogonality and norm bounds follow from dv:   |V v^ - V v_ref| <= |V| dv (V v_ref is the reference's own loss of
    orthogonality: ~u for orthonormal rows, whatever it is for others),   | ||v^|| - 1 | <= ||dv||_2 + 2 u.
    Returns {"h": [i + 1], "v": [n] or None, "orth": [i] or None, "norm": float or None}."""
    V = np.asarray(Vrows, dtype=np.float64)
    absV = np.abs(V)
    i, n = V.shape
    a = np.abs(np.asarray(u, dtype=np.float64)) + abs(float(shift)) * absV[-1]
    ue = np.zeros(n) if u_err is None else np.asarray(u_err, dtype=np.float64)
    f = lambda x: np.abs(np.asarray(x, dtype=np.float64))     # noqa: E731
    dw = 2 * U * a + ue
    dc1 = (n + 4) * U * (absV @ a) + absV @ ue
    E1 = dw + dc1 @ absV + (i + 2) * U * (a + f(ref.c1) @ absV)
    if ref.second:
        dc2 = absV @ E1 + (n + 2) * U * (absV @ (f(ref.w1) + E1))
        dh = dc1 + dc2 + U * (f(ref.c1) + f(ref.c2))
        E = E1 + dc2 @ absV + (i + 2) * U * (f(ref.w1) + E1 + (f(ref.c2) + dc2) @ absV)
    else:
        dh, E = dc1, E1
    nE = float(np.sqrt(np.sum(E * E)))
    beta = float(ref.beta)
    dbeta = nE + (n / 2 + 3) * U * (beta + nE)
    out = {"h": np.concatenate((dh, [dbeta])), "v": None, "orth": None, "norm": None}
    if not ref.dead:
        wk = f(ref.wk)
        dv = E / beta + wk * dbeta / beta ** 2 + 2 * U * wk / beta
        out["v"] = dv
        out["orth"] = absV @ dv
        out["norm"] = float(np.sqrt(np.sum(dv * dv))) + 2 * U
    return out


def judge_step(Vrows, u, shift, ref, h, v_next, u_err=None):
    """worst error / bound of a fp64 step result (h[0..j+1], v_next) per family"""
    b = step_bounds(Vrows, u, shift, ref, u_err)
    out = {"h": worst_ratio(np.abs(np.asarray(h, dtype=LD) - ref.h), b["h"])}
    if not ref.dead:
        vl = np.asarray(v_next, dtype=LD)
        out["v"] = worst_ratio(np.abs(vl - ref.v_next), b["v"])
        Vl = ref.V if ref.V.dtype == LD else np.asarray(Vrows, dtype=LD)
        out["orth"] = worst_ratio(np.abs(Vl @ vl - Vl @ ref.v_next), b["orth"])
        out["norm"] = worst_ratio(abs(np.sqrt(np.sum(vl * vl)) - 1), b["norm"])
    return out


# ---- the exact class ---------------------------------------------------------------------------------------------------
def _spread(n, count, taken):
    """``count`` distinct rows spread evenly over [0, n), none of them in ``taken`` (the first free row at or after each
    evenly spaced position: tile 0 and the last tile get their share)"""
    out, used = [], set(taken)
    for k in range(count):
        r = (k * n) // count
        while r in used:
            r = (r + 1) % n
        used.add(r)
        out.append(r)
    return np.array(out, dtype=np.int64)


def exact_rows(n, j):
    """coordinates of the j + 1 signed coordinate rows: row 0, row n - 1, rows 127 / 128 on either side of a tile edge, then
    evenly spread ones; ``overlap`` cases reuse row 0's coordinate for row 1 with the opposite sign"""
    first = [r for r in (0, n - 1, 127, 128) if 0 <= r < n]
    first = list(dict.fromkeys(first))
    coords = first[: j + 1]
    if len(coords) < j + 1:
        coords += list(_spread(n, j + 1 - len(coords), coords))
    return np.array(coords, dtype=np.int64)


@functools.lru_cache(maxsize=8)
def exact_step(n, j, kind):
    """Exact-class inputs (V rows [j + 1, n], u, shift, p) of one step.  kinds:
      "plain"    u = integers in [-3, 3] on the V coordinates (|.| >= 1 on v_j's) + 4^p entries of +-1 elsewhere, 4^p > the
                 squares on the coordinates: no second pass, beta = 2^p, v_next = w1 / 2^p exact
      "second"   integers of magnitude 2^p .. 2^p + 3 on the coordinates: nrm1 = 4^p < ww / 2 -- the second pass runs, with
                 c2 = 0 exactly (orthogonal rows)
      "overlap"  (j >= 2) as "second", but row 1 is MINUS row 0's coordinate vector and the +-1 entries number 4^p - w_0^2:
                 c1 = (w_0, -w_0, ...), w1[0] = -w_0, c2 = (-w_0, w_0, 0, ...), h_0 = h_1 = 0, w2[0] = w_0, nrm2 = 4^p.  The
                 only exact case whose c2 is not zero: h = c1 + c2 is checked, not h = c1
      "zero"     u = shift v_j bit for bit: w = 0 exactly (a coordinate vector times 3/8 is exact)
      "dead"     u on the coordinates only: w1 = 0 exactly, beta = 0 <= 1e-13 ||w||
    n - (j + 1) free rows bound p; p is as large as fits (at most 5)."""
    coords = exact_rows(n, j)
    rng = np.random.default_rng(7919 * j + n % 100003 + len(kind))
    signs = rng.choice([-1.0, 1.0], size=j + 1)
    V = np.zeros((j + 1, n))
    V[np.arange(j + 1), coords] = signs
    if kind == "overlap":
        assert j >= 2
        coords = coords.copy()
        coords[1] = coords[0]
        V[1] = -V[0]
    u = np.zeros(n)
    if kind == "zero":
        u = SHIFT_EXACT * V[-1]
        return V, u, SHIFT_EXACT, 0
    w0sq = 16 if kind == "overlap" else 0
    p = exact_p(n, j, kind == "overlap")
    count = 4 ** p - w0sq if kind != "dead" else 0
    if kind in ("second", "overlap"):
        mag = rng.integers(2 ** p + 1, 2 ** p + 4, size=j + 1)
    elif kind == "plain" and 4 ** p < 9 * (j + 1) + 3:       # (+ 3: the shift adds 3/8 to |w| on v_j's coordinate)
        mag = np.ones(j + 1, dtype=np.int64)           # (few free rows: unit entries keep 4^p >= the squares on the rows)
    else:
        mag = rng.integers(1, 4, size=j + 1)
    u[coords] = mag * rng.choice([-1.0, 1.0], size=j + 1)
    if kind == "overlap":
        assert p >= 3 and count > 0
        u[coords[0]] = 4.0
    if count > 0:
        rows = _spread(n, count, coords.tolist())
        u[rows] = rng.choice([-1.0, 1.0], size=count)
    headroom(n, float(np.abs(u).max()) + 1.0, float(np.abs(u).max()) + 1.0)
    for a in (V, u):
        a.setflags(write=False)
    return V, u, SHIFT_EXACT, p


def exact_p(n, j, overlap=False):
    """the largest p <= 5 with 4^p (- 16 for "overlap") entries of +-1 on the rows no coordinate vector takes"""
    free = n - (j + 1) + (1 if overlap else 0)
    w0sq = 16 if overlap else 0
    p = 0
    while p < 5 and 4 ** (p + 1) - w0sq <= free:
        p += 1
    return p


def exact_kinds(n, j):
    """the exact kinds that exist at (n, j): a next vector needs a free row, "plain" 4^p >= j + 2 > j + (11 / 8)^2 (no second pass, shifted or not)"""
    kinds = ["zero", "dead"]
    free = n - (j + 1)
    if free >= 1 and 4 ** exact_p(n, j) >= j + 2:
        kinds.append("plain")
    if free >= 1:
        kinds.append("second")
    if j >= 2 and free + 1 >= 48:          # (j >= 2: v_j is not one of the two overlapping rows, the shift stays off them)
        kinds.append("overlap")
    return kinds


# ---- the random class --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def random_rows_ld(n, rows, seed=5):
    """``rows`` orthonormal rows of length n in longdouble.  Up to n = 4097: normal draws, modified Gram-Schmidt twice.
    Beyond (O(rows^2 n) longdouble work would take longer than the device test may): rows 0..2 are dense normal draws, rows
    3.. are normal draws on DISJOINT supports (row 3 + c lives on the indices = c mod (rows - 3): orthogonal by construction);
    the dense rows are orthogonalised against those -- O(n) each -- and against each other, twice."""
    from dominantsparseeigenad_amd.synthetic import normal_vector
    rows = min(rows, n)
    Q = np.zeros((rows, n), dtype=LD)
    draw = lambda t: np.asarray(normal_vector(n, 1000 * seed + t), dtype=LD)     # noqa: E731
    unit = lambda q: q / np.sqrt(np.sum(q * q))                                  # noqa: E731
    dense = rows if n <= 4097 else min(rows, 3)
    comb = rows - dense
    for c in range(comb):
        Q[dense + c, c::comb] = draw(dense + c)[c::comb]
        Q[dense + c] = unit(Q[dense + c])
    for t in range(dense):
        q = draw(t)
        for _ in range(2):
            for c in range(comb):
                r = Q[dense + c, c::comb]
                q[c::comb] -= np.sum(r * q[c::comb]) * r
            for s_ in range(t):
                q = q - np.sum(Q[s_] * q) * Q[s_]
        Q[t] = unit(q)
    Q.setflags(write=False)
    return Q


@functools.lru_cache(maxsize=4)
def random_rows(n, rows, seed=5):
    """the same rows rounded ONCE to fp64: what the device gets"""
    V = np.asarray(random_rows_ld(n, rows, seed), dtype=np.float64)
    V.setflags(write=False)
    return V


@functools.lru_cache(maxsize=2)
def _rounded_rows_ld(n, rows):
    """the ROUNDED rows widened again: what the longdouble reference works on (converted once per n, not once per step)"""
    return np.asarray(random_rows(n, rows), dtype=LD)


def random_step(n, j, kind, with_shift):
    """Random-class inputs (V rows, u, shift, longdouble Step) of one step.  kinds of u:
      "generic"   a normal vector: no second pass
      "second"    V^T c + 2^-10 z (c, z normal): the first pass cancels ten bits, the second pass runs
      "dead"      2 v_t, t = max(j - 1, 0): exactly representable, and w = 2 v_t - shift v_j lies in the span of the rows
    Asserts both decision margins a factor MARGIN away from 1 (on the side the kind names)."""
    from dominantsparseeigenad_amd.synthetic import normal_vector
    V = long_rows(n, j) if j > max(STEP_J) else random_rows(n, max(STEP_J) + 1 if n < 262146 else 3)[: j + 1]
    assert V.shape[0] == j + 1, (n, j)
    shift = SHIFT_RANDOM if with_shift else 0.0
    z = normal_vector(n, 31 * n % 9973 + j)
    if kind == "generic":
        u = z
    elif kind == "second":
        c = normal_vector(j + 1, 77 + j)
        c = np.sqrt(n) * (np.sign(c) + c)                # |c_t| >= sqrt(n) ~ ||z||: ||w1|| / ||w|| <= 2^-10 at every n, j
        u = c @ V + 2.0 ** -10 * z
    else:
        u = 2.0 * V[max(j - 1, 0)]
    u = np.ascontiguousarray(u, dtype=np.float64)
    Vl = V if j > max(STEP_J) else _rounded_rows_ld(n, max(STEP_J) + 1 if n < 262146 else 3)[: j + 1]
    ref = arnoldi_step(Vl, u, shift, LD)
    want_second, want_dead = kind != "generic", kind == "dead"
    assert ref.second == want_second and ref.dead == want_dead, (n, j, kind, ref.margin_dgks, ref.margin_dead)
    assert (ref.margin_dgks <= 1 / MARGIN) if want_second else (ref.margin_dgks >= MARGIN_NO_SECOND), (n, j, kind, ref.margin_dgks)
    assert (ref.margin_dead <= 1 / MARGIN) if want_dead else (ref.margin_dead >= MARGIN), (n, j, kind, ref.margin_dead)
    return V, u, shift, ref


@functools.lru_cache(maxsize=2)
def long_rows(n, j):
    """j + 1 > n rows cannot be orthonormal, and the step does not ask for it: 8 orthonormal rows, then normal rows scaled by
    2^-20 -- every coefficient beyond row 7 is a distinct non-zero number, the decisions stay those of the 8 rows"""
    from dominantsparseeigenad_amd.synthetic import normal_vector
    tail = np.stack([normal_vector(n, 4000 + t) for t in range(8, j + 1)]) * 2.0 ** -20
    V = np.concatenate((random_rows(n, 8), tail))
    V.setflags(write=False)
    return V


def random_kinds(n, j):
    """a generic u keeps nrm1 / (0.5 ww) ~ 2 (n - j - 1) / n above MARGIN_NO_SECOND only while the rows take a small share of
    it: j + 1 <= 0.15 n; "second" needs a row outside the span, "dead" two rows to choose from or no shift at all"""
    if j > max(STEP_J):
        return ["generic", "second"]
    kinds = []
    if j + 1 <= 0.15 * n:
        kinds.append("generic")
    if n - (j + 1) >= 1:
        kinds.append("second")
    kinds.append("dead")
    return kinds


# ---- a run of steps: the Arnoldi relation --------------------------------------------------------------------------------
def relation_ratio(apply, m_terms, shift, V, H, j0, j1):
    """Arnoldi relation and per-step verdict of a device run, column by column ON THE DEVICE'S OWN V: for j in [j0, j1) the
    longdouble step from (V[0..j], u = A v_j in longdouble) is the reference of column j and of V[j+1]; the device's u carried
    the mat-vec bound (m + 4) u |A||v_j| (tests/matvec_reference.py), handed to ``step_bounds`` as u_err.  Because every
    column is judged from the rows the device itself produced, the bound does NOT grow from step to step: growth factor 1
    (a comparison with an independent host trajectory would need the factor ||A - shift I|| / beta_j per step, which no
    operation count supplies).  The relation residual
        |(A - shift I) v_j - sum_{t <= j+1} H[t, j] v_t|  <=  beta dv + |V|^T dh + u_err-free terms already inside dv, dh
    is reported as well, against  beta_ref * dv + |V[0..j]|^T dh + dbeta |v_next|.
    Returns {"h", "v", "orth", "norm", "relation"} worst ratios over the columns."""
    out = {}
    for j in range(j0, j1):
        rows = V[: j + 1]
        Av, sc = apply(V[j], LD)
        ref = arnoldi_step(rows, Av, shift, LD)
        assert not ref.dead
        u_err = (m_terms + 4) * U * np.asarray(sc, dtype=np.float64)
        hcol = H[j, : j + 2]
        r = judge_step(rows, np.asarray(Av, dtype=np.float64), shift, ref, hcol, V[j + 1], u_err)
        b = step_bounds(rows, np.asarray(Av, dtype=np.float64), shift, ref, u_err)
        res = Av - LD(shift) * np.asarray(V[j], dtype=LD) - np.asarray(hcol, dtype=LD) @ np.asarray(V[: j + 2], dtype=LD)
        bound = float(ref.beta) * b["v"] + b["h"][:-1] @ np.abs(rows) + b["h"][-1] * np.abs(V[j + 1])
        r["relation"] = worst_ratio(np.abs(res), bound)
        for k, v in r.items():
            out[k] = max(out.get(k, 0.0), v)
    return out


# ---- GMRES ---------------------------------------------------------------------------------------------------------------
def gmres_cycle(apply, shift, b, x0, m, target, dtype=LD, summ=None):
    """ONE cycle of GMRES(m) for (A - shift I) x = b as include/dsea.h dsea_gmres_cycle specifies it: r0 = b - (A - shift I) x0
    (x0 None: r0 = b), the Arnoldi steps above, Givens rotations, early finish, back-substitution over the columns used.
    Returns (x, state[7], extras) with state = [residual estimate, converged, columns used, ||r0||, finished early,
    0 (second-pass flag: the reference always runs the pass), singular]; extras: V, the residual estimate after every column."""
    n = b.size
    bd = np.asarray(b, dtype=dtype)
    x = np.zeros(n, dtype=dtype) if x0 is None else np.asarray(x0, dtype=dtype)
    A = lambda v: apply(v, dtype)[0] - dtype(shift) * v     # noqa: E731
    r0 = bd if x0 is None else bd - A(x)
    beta0 = np.sqrt(_nrm2(r0, summ))
    state = [beta0, 0.0, 0.0, beta0, 0.0, 0.0, 0.0]
    hist = []
    if beta0 <= target:
        state[1] = state[4] = 1.0
        return x, state, {"V": None, "history": hist}
    V = np.zeros((m + 1, n), dtype=dtype)
    V[0] = r0 / beta0
    R = np.zeros((m + 1, m), dtype=dtype)
    cs, sn, g = np.zeros(m, dtype=dtype), np.zeros(m, dtype=dtype), np.zeros(m + 1, dtype=dtype)
    g[0] = beta0
    k = 0
    for j in range(m):
        st = arnoldi_step(V[: j + 1], apply(V[j], dtype)[0], shift, dtype, summ)
        h = np.zeros(m + 1, dtype=dtype)
        h[: j + 2] = st.h
        if not st.dead:
            V[j + 1] = st.v_next
        for t in range(j):
            a_, b_ = h[t], h[t + 1]
            h[t], h[t + 1] = cs[t] * a_ + sn[t] * b_, -sn[t] * a_ + cs[t] * b_
        rho = np.hypot(h[j], h[j + 1])
        if rho == 0:
            state[4] = state[6] = 1.0
            break
        cs[j], sn[j] = h[j] / rho, h[j + 1] / rho
        h[j], h[j + 1] = rho, 0
        R[:, j] = h
        g[j + 1], g[j] = -sn[j] * g[j], cs[j] * g[j]
        k = j + 1
        state[0], state[2] = abs(g[j + 1]), float(k)
        hist.append(abs(g[j + 1]))
        if state[0] <= target:
            state[1] = state[4] = 1.0
            break
        if st.dead:
            state[4] = 1.0
            break
    y = np.zeros(m, dtype=dtype)
    for i in range(k - 1, -1, -1):
        y[i] = (g[i] - np.sum(R[i, i + 1:k] * y[i + 1:k])) / R[i, i]
    x = x + y[:k] @ V[:k]
    return x, state, {"V": V, "history": hist, "y": y}


def lstsq_over(apply, shift, b, x0, Vrows):
    """the least-squares minimiser x0 + V^T y of ||b - (A - shift I) x|| over span(Vrows), in longdouble by normal equations
    on a QR-free path: Vrows has at most 8 rows and A - shift I is well conditioned on them (the test matrices are
    2.5 I + noise); returns (x, ||residual||, |x - x0| scale for the bound)"""
    Vl = np.asarray(Vrows, dtype=LD)
    x0l = np.zeros(b.size, dtype=LD) if x0 is None else np.asarray(x0, dtype=LD)
    A = lambda v: apply(v, LD)[0] - LD(shift) * v     # noqa: E731
    r0 = np.asarray(b, dtype=LD) - (A(x0l) if x0 is not None else 0)
    W = np.stack([A(v) for v in Vl])                    # rows (A - shift I) v_t
    # orthonormalise W's rows in longdouble (MGS twice) and project r0: y solves the triangular system
    k = W.shape[0]
    Q, Rm = np.zeros_like(W), np.zeros((k, k), dtype=LD)
    for t in range(k):
        q = W[t].copy()
        for _ in range(2):
            for s in range(t):
                c = np.sum(Q[s] * q)
                Rm[s, t] += c
                q = q - c * Q[s]
        Rm[t, t] = np.sqrt(np.sum(q * q))
        Q[t] = q / Rm[t, t]
    z = Q @ r0
    y = np.zeros(k, dtype=LD)
    for i in range(k - 1, -1, -1):
        y[i] = (z[i] - np.sum(Rm[i, i + 1:] * y[i + 1:])) / Rm[i, i]
    x = x0l + y @ Vl
    res = r0 - y @ W
    return x, np.sqrt(np.sum(res * res)), y, Rm


def gmres_bounds(n, m_terms, k, normA, normb, cond):
    """Normwise first-order bounds of one fp64 cycle with k columns (u = 2^-53).  Every Arnoldi column satisfies its relation
    to (n + k + m_terms + 8) u ||A_s|| (``step_bounds`` summed in the 2-norm: a dot of n terms, k + 1 subtractions, the
    mat-vec), the k Givens rotations and the back-substitution are backward stable with 6 k u and k u (Higham, Accuracy and
    Stability, Lemma 19.8 and Theorem 8.5), so the computed y solves a least-squares problem perturbed by
        eps = (n + m_terms + 8 k + 8) u
    relative to ||A_s|| ||V|| = ||A_s||.  With cond = ||A_s|| / sigma_min(A_s V_k) >= 1 (sigma_min of the longdouble R factor
    ``lstsq_over`` returns, see ``subspace_cond``) the minimiser moves by at most
    2 eps cond^2 ||r0|| / ||A_s|| (Wedin; the squared term covers a residual of the size of r0), and the residual norm by
    eps ||A_s|| ||x - x0|| + eps ||r0|| <= 2 eps cond ||r0||.
    Returns (bound on ||x - x_ls||_2, bound on | state[0] - ||b - A_s x|| |)."""
    eps = (n + m_terms + 8 * k + 8) * U
    return 2 * eps * cond ** 2 * normb / normA, 2 * eps * cond * normb


def three_eigenvalue_matrix(n, seed=3, eigs=(1.0, 2.0, 4.0), weights=None):
    """dense diagonal-plus-rotation matrix with three distinct eigenvalues: A = G diag(e0, e1, e2, e0, e1, e2, ...) G^T with G a
    product of 40 plane rotations by the angle (3/5, 4/5), applied in longdouble and rounded once -- every Krylov space has
    dimension <= 3 up to that rounding.  With ``weights`` (w0, w1, w2) also returns a unit start vector whose squared
    components along the three eigenspaces are the weights: the Lanczos coefficients of the run are then those of the
    three-point measure.  For eigs (-c, 0, c) and weights (e/2, 1 - e, e/2): alpha = 0, beta_0^2 = c^2 e, beta_1^2 = c^2 (1 - e),
    so steps 0 and 1 pass the DGKS test with nrm1 / (0.5 ww) = 2 and 2 (1 - e), and step 2 ends the space."""
    rng = np.random.default_rng(seed)
    group = np.arange(n) % 3
    A = np.diag(np.array(eigs)[group]).astype(LD)
    z = None
    if weights is not None:
        z = np.sqrt(np.array([LD(weights[g]) / LD(np.sum(group == g)) for g in group]))
    c, s_ = LD(3) / 5, LD(4) / 5
    for _ in range(40):
        p, q = rng.choice(n, size=2, replace=False)
        rp, rq = A[p].copy(), A[q].copy()
        A[p], A[q] = c * rp + s_ * rq, -s_ * rp + c * rq
        cp, cq = A[:, p].copy(), A[:, q].copy()
        A[:, p], A[:, q] = c * cp + s_ * cq, -s_ * cp + c * cq
        if z is not None:
            z[p], z[q] = c * z[p] + s_ * z[q], -s_ * z[p] + c * z[q]
    A = np.asarray(A, dtype=np.float64)
    return A if z is None else (A, np.asarray(z, dtype=np.float64))


def dense_noise(n, seed=11, scale=1.0):
    """A = 2.5 I + scale * randn / sqrt(n): the matrix of the GMRES stage tests"""
    return 2.5 * np.eye(n) + scale * np.random.default_rng(seed).standard_normal((n, n)) / np.sqrt(n)


def midcycle_target(n, b):
    """(target, apply) of the "converged in mid-cycle" case: the residual of A = 2.5 I + randn / sqrt(n) falls by ~0.4 per
    column, which leaves no target a factor 2 away from BOTH neighbours; with the noise scaled by 0.4 it falls by ~0.16.  The
    target is the geometric mean of the reference's residuals after columns 2 and 3; the factor 2 is asserted."""
    from matvec_reference import dense_apply
    apply = dense_apply(dense_noise(n, scale=0.4))
    _, _, ex = gmres_cycle(apply, 0.0, b, None, 8, 0.0)
    hist = [float(v) for v in ex["history"]]
    target = float(np.sqrt(hist[1] * hist[2]))
    assert hist[1] >= 2 * target and target >= 2 * hist[2], hist[:4]
    return target, apply


def subspace_cond(normA, Rm):
    """||A_s|| / sigma_min(A_s V_k) from the R factor of ``lstsq_over``"""
    sv = np.linalg.svd(np.asarray(Rm, dtype=np.float64), compute_uv=False)
    return float(normA) / float(sv[-1])
