"""Cases, launcher geometry, verdicts and the tiled numpy twin of the chain and lattice tile-kernel tests and of the Ritz block
width tests (tests/test_gpu_tile_kernels.py, proved on the CPU by tests/test_tile_reference_cpu.py); no GPU, no torch.
docs/design/42-tile-and-width-instantiation-tests.md tells the same story at length.

THE SHAPES (``WHOLE``, ``TILED``, ``WALK``; T = log2 of the rows a block stages in LDS)

    T       how                  L        what it reaches
    7..11   default tuning       T        the whole vector at PER 1, 1, 1, 2, 4; the chain's wrap bond inside the tile
    12      set_tile_log2(12)    12       the whole vector at PER 8
    7..12   set_tile_log2(T)     T + 3    eight tiles; the chain has nf = 7 far terms: buffers 4 + 3, 2 + 2 + 2 + 1, seven singles
    7       set_tile_log2(7)     20       8192 tiles on 4096 blocks (exact class only)

TWO INPUT CLASSES (tests/matvec_reference.py): EXACT -- x integers in [-4, 4], couplings non-zero multiples of 1/8 in [-2, 2],
shift 0.375: every coefficient, product and partial sum is a multiple of 1/64 far below 2^53, so y, y - shift x and x.y do not
depend on the summation order or on FMA and must equal the reference bit for bit; RANDOM -- synthetic.normal_vector data
against np.longdouble with the bounds (m + 4) u (|H||x| + |shift x|) per row and ``dot_bound`` for x.y.

THE OPERATION COUNTS m (the rounded operations that can lie on the way to one row, read off the kernel source)

    k_spmv_chain     a coefficient Jx - (+-Jy) and an FMA per off-diagonal term (2 L terms; a field term's coefficient hx - 0 is
                     exact and counted all the same), 2 L additions for the diagonal (L for the zz sum, L - 1 for the z sum, one
                     to join them), one joining FMA, a product and a difference for the shift:        m = 6 L + 3
    k_spmv_lattice   a coefficient and an FMA per off-diagonal term (L + nb terms), nb + L additions for the diagonal (one
                     accumulator takes the Jz of every bond and the hz of every site), one joining FMA, two operations for the
                     shift:                                                                          m = 3 (L + nb) + 3
    k_*_forms        a form is a sum of n = 2^L products; each product is rounded once (the library is built with
                     -ffp-contract=off) and every path through the lane, wave, block and grid reductions has at most n - 1
                     additions: n rounded operations, inside the (n + 4) u sum |terms| of the issue without the factor two.

THE TWIN composes a row pair (i0, i0 | 1) the way the kernels do: partners with every flipped bit below T from the tile
(pair lp ^ px of the tile's own pairs), the others by ``chain_far_term`` / ``lattice_far_term`` number k (mask with bit 0
cleared, ``swap`` when the term flips site 0, the second row's zz bit flipped when the bond holds site 0), the wrap bond
inside the tile when T = L.  ``MUTANTS`` override one rule each."""
import functools

import numpy as np

import chain_reference
import lattice_reference
import matvec_reference as ref
from matvec_reference import LD, U
from dominantsparseeigenad_amd._lib import LATTICE_MAX_BONDS

SENTINEL = -7.0
SHIFT_EXACT, SHIFT_RANDOM = 0.375, 0.6180339887498949
DEFAULT_TILE_LOG2 = 11                  # dsea_op_set_tuning DSEA_TUNE_TFIM_TILE_LOG2: 6..12, default 11
MAX_BLOCKS = ref.MAX_TFIM_BLOCKS        # DSEA_MAX_TFIM_BLOCKS

# (L, tile tuning or None for the default)
WHOLE = tuple((T, None if T <= DEFAULT_TILE_LOG2 else T) for T in range(7, 13))
TILED = tuple((T + 3, T) for T in range(7, 13))
WALK = (20, 7)
SHAPES = WHOLE + TILED
CHAIN_KINDS = ("random", "jy-only", "open")         # the three kinds of tests/test_gpu_chain.py
LATTICE_KINDS = ("random", "jy-only")               # the two kinds of tests/test_gpu_lattice.py


# ---- launcher geometry (csrc/dsea_chain.hip, csrc/dsea_lattice.hip) ---------------------------------------------------------
def tile_log2(L, tune=None):
    """chain_tile_log2 / lattice_tile_log2: the tuning value, the whole vector when it is smaller"""
    t = DEFAULT_TILE_LOG2 if tune is None else tune
    return L if L < t else t


def blocks(L, T):
    """chain_blocks / lattice_blocks: one tile per block up to the cap"""
    return min((1 << L) >> T, MAX_BLOCKS)


def per(T):
    """row pairs per thread"""
    return ((1 << (T - 1)) + 255) // 256


def ch(T):
    """far terms per buffer"""
    return 1 if per(T) >= 8 else 2 if per(T) >= 4 else 4


def chain_nf(L, T):
    """chain_far_count"""
    return 2 * (L - T) + 1 if L > T else 0


def lattice_table(bonds, T):
    """lattice_params: ([(a, b, the caller's index)] with the bonds below T first, each group in the caller's order; n_in)"""
    inside = [(a, b, t) for t, (a, b) in enumerate(bonds) if a < T and b < T]
    far = [(a, b, t) for t, (a, b) in enumerate(bonds) if not (a < T and b < T)]
    return inside + far, len(inside)


def lattice_nf(L, T, bonds):
    return (L - T) + len(bonds) - lattice_table(bonds, T)[1]


def buffers(nf, T):
    """how many terms each far buffer holds"""
    return [min(ch(T), nf - k0) for k0 in range(0, nf, ch(T))]


def lattice_tiles_of_the_older_suite():
    """the tiles tests/test_gpu_lattice.py runs (its GEOMETRY: L = 2, 3, 5, 6, 7, 9 at 2^6, 13 at the default, 19 at 2^6)"""
    return sorted({tile_log2(L, tune) for L, tune in ((2, None), (3, None), (5, None), (6, 6), (7, 6), (9, 6), (13, None), (19, 6))})


def chain_m(L):
    return 6 * L + 3


def lattice_m(L, nb):
    return 3 * (L + nb) + 3


# ---- the Ritz block launcher (csrc/dsea_deflated.hip launch_ritz_block on Workspace::geom) -----------------------------------
RITZ_SPLIT16 = [(n, k) for n in (1, 3, 129, 4097) for k in (1, 3, 4, 5, 64)]
RITZ_SPLIT8 = [(32897, k) for k in (5, 64)]
RITZ_SPLIT4 = [(129, k) for k in (5, 64)]
RITZ_RPL = [(r, n, k) for r in (2, 4, 8, 16) for n in (129, 300) for k in (1, 2, 5, 64)]
RITZ_WAVE = (131202, 64, (1, 3, 8))


def ritz_cap(m):
    """rows per lane the accumulator registers allow: M * RPL <= 32"""
    return 16 if m <= 2 else 8 if m <= 4 else 4


def ritz_block_form(n, m, rpl=0, split=-1):
    """the instantiation launch_ritz_block runs: ("split", W) or ("wave", RPL, M)"""
    from lanczos_reference import geom
    g = geom(n, rpl, split)
    if g["split_w"]:
        return ("split", g["split_w"])
    return ("wave", min(g["rpl"], ritz_cap(m)), m)


RITZ_INSTANTIATIONS = {("split", w) for w in (4, 8, 16)} | {("wave", r, m) for m in range(1, 9) for r in (2, 4, 8, 16)
                                                            if r <= ritz_cap(m)}


# ---- bond lists and couplings -----------------------------------------------------------------------------------------------
def corner_sites(L, T):
    """the sites whose pairs reach every geometric case of a bond at a tile of 2^T rows"""
    return (0, 1, T - 1, T, T + 1, L - 1) if L > T else (0, 1, L - 2, L - 1)


def cyclic_complete(L, count):
    full = lattice_reference.complete_bonds(L)
    return tuple(full[i % len(full)] for i in range(count))


@functools.lru_cache(maxsize=None)
def lattice_bonds(L, T, cap=False):
    """every pair among ``corner_sites``, 10 random pairs, the first pair again reversed; ``cap``: the complete graph listed
    cyclically up to the most bonds an operator takes"""
    if cap:
        return cyclic_complete(L, LATTICE_MAX_BONDS)
    sites = sorted(set(corner_sites(L, T)))
    pairs = [(a, b) for i, a in enumerate(sites) for b in sites[i + 1:]]
    return tuple(pairs + lattice_reference.random_bonds(L, 10, 7100 + L) + [(pairs[0][1], pairs[0][0])])


def nonzero_eighths(shape, seed):
    v = ref.eighths(shape, seed)
    v[v == 0] = 0.125
    return v


def chain_couplings(L, kind, exact):
    from dominantsparseeigenad_amd.synthetic import normal_vector
    c = nonzero_eighths((5, L), 8000 + L) if exact else normal_vector(5 * L, 8000 + L).reshape(5, L).copy()
    if kind == "jy-only":
        c[[0, 2, 3, 4]] = 0.0
    elif kind == "open":
        c[:3, L - 1] = 0.0
    return c


def chain_flat(c):
    """(5, L) rows Jx, Jy, Jz, hx, hz as the bond list parameter of ``ref.chain_bonds``"""
    return np.ascontiguousarray(c, dtype=np.float64).reshape(-1)


def lattice_couplings(L, bonds, kind, exact):
    from dominantsparseeigenad_amd.synthetic import normal_vector
    nb, count = len(bonds), 3 * len(bonds) + 2 * L
    p = nonzero_eighths(count, 8000 + L + nb) if exact else normal_vector(count, 8000 + L + nb).copy()
    if kind == "jy-only":
        p[:nb] = 0.0
        p[2 * nb:] = 0.0
    return p


TILES = [7, 8, 9, 10, 11, 12]


def assert_tile_cases():
    """the shapes reach what the table says: tile, blocks, PER, CH, nf and the buffers, n_in and the kinds of far bond"""
    assert [L for L, _ in WHOLE] == TILES and [L for L, _ in TILED] == [T + 3 for T in TILES]
    for (L, tune), T in zip(WHOLE, TILES):
        assert tile_log2(L, tune) == T == L and blocks(L, T) == 1 and chain_nf(L, T) == 0
        assert (tune is None) == (T <= 11)                                 # the default tile is 2^11
        bonds = lattice_bonds(L, T)
        assert lattice_table(bonds, T)[1] == len(bonds) and lattice_nf(L, T, bonds) == 0
    assert [per(T) for T in TILES] == [1, 1, 1, 2, 4, 8] and [ch(T) for T in TILES] == [4, 4, 4, 4, 2, 1]
    assert [(1 << (T - 1)) < 256 for T in TILES] == [True, True, False, False, False, False]      # NPAIR < 256 at T = 7, 8
    want_buffers = {4: [4, 3], 2: [2, 2, 2, 1], 1: [1] * 7}
    for (L, tune), T in zip(TILED, TILES):
        assert tile_log2(L, tune) == T == tune and blocks(L, T) == 8
        assert chain_nf(L, T) == 7 and buffers(7, T) == want_buffers[ch(T)]
        bonds = lattice_bonds(L, T)
        table, n_in = lattice_table(bonds, T)
        assert len(bonds) == 15 + 10 + 1 and bonds[-1] == bonds[0][::-1] and 0 < n_in < len(bonds)
        sites = set(corner_sites(L, T))
        assert all((a, b) in bonds for a in sites for b in sites if a < b)
        far = table[n_in:]
        kinds = {(min(a, b) == 0, min(a, b) < T) for a, b, _ in far}         # (holds site 0, one site inside)
        assert kinds == {(True, True), (False, True), (False, False)}
        assert any(0 in (a, b) for a, b, _ in table[:n_in])                  # inside with the site-0 swap
        assert sorted(t for _, _, t in table) == list(range(len(bonds)))
        assert lattice_nf(L, T, bonds) == 3 + len(far)
    cap = lattice_bonds(12, 9, cap=True)
    assert len(cap) == LATTICE_MAX_BONDS and len(set(cap)) == 66 and 0 < lattice_table(cap, 9)[1] < len(cap)
    L, T = WALK
    assert tile_log2(L, T) == 7 and (1 << L) >> T == 8192 and blocks(L, T) == 4096 == ref.MAX_TFIM_BLOCKS
    assert 0 < lattice_table(lattice_bonds(L, T), T)[1] < len(lattice_bonds(L, T))


def assert_ritz_cases():
    """the Ritz block geometries reach all 22 valid (RPL, M) pairs and all three W, by the launcher's rule"""
    reached = set()
    for n, k in RITZ_SPLIT16:
        assert {ritz_block_form(n, m) for m in range(1, 9)} == {("split", 16)}
    for n, k in RITZ_SPLIT8:
        assert {ritz_block_form(n, m) for m in range(1, 9)} == {("split", 8)}
    for n, k in RITZ_SPLIT4:
        assert {ritz_block_form(n, m, split=4) for m in range(1, 9)} == {("split", 4)}
    reached |= {("split", 16), ("split", 8), ("split", 4)}
    for r, n, k in RITZ_RPL:
        for m in range(1, 9):
            form = ritz_block_form(n, m, rpl=r)
            assert form == ("wave", min(r, ritz_cap(m)), m)
            reached.add(form)
    n, k, ms = RITZ_WAVE
    assert [ritz_block_form(n, m) for m in ms] == [("wave", 2, m) for m in ms]
    assert reached == RITZ_INSTANTIATIONS and len(reached) == 22 + 3        # 2 x 4 + 2 x 3 + 4 x 2 pairs with RPL <= CAP(M), three W
    assert [ritz_cap(m) for m in range(1, 9)] == [16, 16, 8, 8, 4, 4, 4, 4]
    ks = {k for _, k in RITZ_SPLIT16}
    assert min((k + 3) // 4 for k in ks) < 16 and any(k % 4 for k in ks) and any(k % 4 == 0 for k in ks)
    assert {k % 2 for _, _, k in RITZ_RPL} == {0, 1}


# ---- cases ------------------------------------------------------------------------------------------------------------------
class Case:
    """inputs and references of one operator at one L, computed once and never written to: the exact class always, the random
    class unless ``random`` is False.  ``bonds`` / ``p_*`` describe the operator as a bond list whatever the family."""

    def __init__(self, family, L, bonds, p_exact, p_random, m, seed, random=True):
        self.family, self.L, self.n, self.m = family, L, 1 << L, m
        self.bonds, self.p_exact, self.p_random = tuple(bonds), p_exact, p_random
        n, nb = self.n, len(bonds)
        self.x = ref.exact_vector(n, seed)
        self.ax, sc = ref.lattice_apply(L, bonds, p_exact)(self.x, np.float64)
        # the row's term count and largest coefficient: L + nb off-diagonal terms of at most 2 cmax, a diagonal of at most
        # (nb + L) cmax, the shift; all of them times max |x| = 4
        cmax = float(np.max(np.abs(p_exact)))
        self.ymax = 4.0 * (2.0 * cmax * (L + nb) + cmax * (nb + L) + SHIFT_EXACT)
        ref.headroom(n, 4, self.ymax)
        assert float(sc.max()) + 4.0 * SHIFT_EXACT <= self.ymax
        self.shifted = self.ax - SHIFT_EXACT * self.x
        for v in (self.ax, self.shifted):
            assert np.array_equal(v * 64.0, np.rint(v * 64.0)), "a row is no multiple of 1/64"
        self.dot = float(np.sum(self.x * self.shifted))
        self.random = random
        if random:
            from dominantsparseeigenad_amd.synthetic import normal_vector
            self.xr = normal_vector(n, seed + 1)
            self.want, self.scale = ref.shifted(ref.lattice_apply(L, bonds, p_random), self.xr, SHIFT_RANDOM, LD)
            self.dot_r = np.sum(np.asarray(self.xr, dtype=LD) * self.want)
        for a in vars(self).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)


@functools.lru_cache(maxsize=8)
def chain_case(L, kind, random=True):
    return Case("chain", L, ref.chain_bonds(L), chain_flat(chain_couplings(L, kind, True)),
                chain_flat(chain_couplings(L, kind, False)), chain_m(L), 100 * L + 7, random)


@functools.lru_cache(maxsize=8)
def lattice_case(L, T, kind, random=True, cap=False):
    bonds = lattice_bonds(L, T, cap)
    return Case("lattice", L, bonds, lattice_couplings(L, bonds, kind, True), lattice_couplings(L, bonds, kind, False),
                lattice_m(L, len(bonds)), 100 * L + 9, random)


def judge(tag, case, run, log=print, classes=("exact", "random")):
    """the whole contract of dsea_spmv on one operator.  ``run(cls, x, shift=None, dot=False, skip=False) -> (y, x.y or
    None)`` makes ONE call with the couplings of class ``cls`` into sentinel-filled outputs.  Raises AssertionError where a
    verdict fails; returns the worst error / bound of the random class."""
    if "exact" in classes:
        y, _ = run("exact", case.x)
        assert np.array_equal(y, case.ax), "%s: y = H x on exact inputs, %d rows differ" % (tag, int(np.sum(y != case.ax)))
        y, d = run("exact", case.x, shift=SHIFT_EXACT, dot=True)
        assert np.array_equal(y, case.shifted), "%s: y = H x - shift x on exact inputs, %d rows differ" % (
            tag, int(np.sum(y != case.shifted)))
        assert d == case.dot, "%s: x.y on exact inputs %r, want %r" % (tag, d, case.dot)
        y, d = run("exact", case.x, shift=SHIFT_EXACT, dot=True, skip=True)
        assert bool((y == SENTINEL).all()) and d == SENTINEL, "%s: the skip flag did not make the call a no-op" % tag
        y, _ = run("exact", case.x, skip=True)
        assert bool((y == SENTINEL).all()), "%s: the skip flag did not make the call a no-op" % tag
    if not case.random or "random" not in classes:
        log("%s: exact" % tag)
        return 0.0
    y, d = run("random", case.xr, shift=SHIFT_RANDOM, dot=True)
    ry = ref.worst_ratio(np.abs(np.asarray(y, dtype=LD) - case.want), ref.matvec_bound(case.m, case.scale))
    rd = ref.worst_ratio(abs(LD(d) - case.dot_r), ref.dot_bound(case.n, case.m, case.xr, case.scale))
    log("%s: exact; random  |y - ref| / bound = %.3f   |x.y - ref| / bound = %.3f" % (tag, ry, rd))
    assert ry <= 1.0 and rd <= 1.0, (tag, ry, rd)
    return max(ry, rd)


# ---- the forms --------------------------------------------------------------------------------------------------------------
def forms_reference(L, bonds, v1, v2, magnitudes=True):
    """(the 3 nb + 2 L forms in longdouble, sum |terms| of each or None); ``bonds`` None: the chain, its (5, L) forms row by
    row"""
    if bonds is None:
        want = chain_reference.forms(L, v1, v2, dtype=LD).reshape(-1)
    else:
        want = lattice_reference.forms(L, bonds, v1, v2, dtype=LD)
    if not magnitudes:
        return want, None
    if bonds is None:
        nb = L
        mag = chain_reference.forms(L, np.abs(v1), np.abs(v2), dtype=LD).reshape(-1)
    else:
        nb = len(bonds)
        mag = lattice_reference.forms(L, bonds, np.abs(v1), np.abs(v2), dtype=LD)
    diag = np.sum(np.abs(np.asarray(v1, dtype=LD) * np.asarray(v2, dtype=LD)))
    terms = np.concatenate((mag[:nb], mag[:nb], np.full(nb, diag), mag[3 * nb:3 * nb + L], np.full(L, diag)))
    return want, terms


def forms_bound(n, terms):
    return (n + 4) * U * np.asarray(terms, dtype=np.float64)


class FormsCase:
    """v1, v2 and the forms of one bond list at one L in both classes (the forms do not depend on the couplings)"""

    def __init__(self, L, bonds, seed, random=True):
        from dominantsparseeigenad_amd.synthetic import normal_vector
        n = 1 << L
        self.L, self.n, self.bonds, self.random = L, n, bonds, random
        self.v1, self.v2 = ref.exact_vector(n, seed), ref.exact_vector(n, seed + 1)
        want, _ = forms_reference(L, bonds, self.v1, self.v2, magnitudes=False)
        assert n * 16.0 < 2.0 ** 50                              # n products of at most 4 x 4: every partial sum is an integer far below 2^53
        self.want = want.astype(np.float64)
        assert np.array_equal(self.want.astype(LD), want)
        if random:
            self.r1, self.r2 = normal_vector(n, seed + 2), normal_vector(n, seed + 3)
            self.want_r, terms_r = forms_reference(L, bonds, self.r1, self.r2)
            self.bound = forms_bound(n, terms_r)
        for a in vars(self).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)


@functools.lru_cache(maxsize=4)
def chain_forms_case(L, random=True):
    return FormsCase(L, None, 300 * L + 1, random)


@functools.lru_cache(maxsize=4)
def lattice_forms_case(L, T, random=True, cap=False):
    return FormsCase(L, lattice_bonds(L, T, cap), 300 * L + 5, random)


# ---- the tiled twin ---------------------------------------------------------------------------------------------------------
MUTANTS = ("straddling-inside", "wrap-unswapped", "second-row-zz", "far-field-T", "far-table-offset", "ragged-last",
           "dot-before-shift")


def mutant_applies(mutant, family, L, T):
    tiled = L > T
    if mutant in ("straddling-inside", "far-field-T", "ragged-last"):
        return tiled
    if mutant == "far-table-offset":
        return tiled and family == "lattice"
    return True


class Term:
    """one off-diagonal term of a row pair: partner pair p ^ pxor (from the tile when ``inside``), elements swapped when
    ``swap``; coefficient ca - cb zz with zz of sites (a, b) (a field term: cb = 0); cz: what it adds to the diagonal"""

    def __init__(self, pxor, inside, swap, ca, cb, a, b, cz=0.0, holds0=None):
        self.pxor, self.inside, self.swap, self.ca, self.cb, self.a, self.b, self.cz = pxor, inside, swap, ca, cb, a, b, cz
        self.holds0 = (a == 0 or b == 0) if holds0 is None else holds0


def _bond_term(a, b, T, ca, cb, cz, mutant, family, wrap=False):
    far = a >= T or b >= T
    straddles = far and (a < T or b < T)
    mask = ((1 << a) | (1 << b)) & ~1
    swap = a == 0 or b == 0
    if mutant == "wrap-unswapped" and (wrap or family == "lattice"):
        swap = False
    inside = not far
    if mutant == "straddling-inside" and straddles and (family == "lattice" or not wrap):
        inside = True
    return Term(mask >> 1, inside, swap, ca, cb, a, b, cz, holds0=(a == 0 or b == 0))


def chain_terms(L, T, c, mutant=None):
    """the off-diagonal terms of k_spmv_chain in the kernel's order (far terms by number, fields and bonds inside the tile, the
    wrap bond when T = L) and the diagonal's (coefficient, a, b) list (b = None: a z term)"""
    c = np.asarray(c).reshape(5, L)
    jx, jy, jz, hx, hz = c
    terms = []
    nfx, nf = L - T, chain_nf(L, T)
    last = nf - 1 if mutant == "ragged-last" else nf
    for k in range(last):
        if k < nfx:
            site = T + k
            if not (mutant == "far-field-T" and site == T):
                terms.append(Term((1 << site) >> 1, False, False, hx[site], 0.0, site, site, holds0=False))
        else:
            b = T - 1 + (k - nfx)
            b1 = 0 if b + 1 == L else b + 1
            terms.append(_bond_term(b, b1, T, jx[b], jy[b], 0.0, mutant, "chain", wrap=(b1 == 0)))
    for i in range(T):
        terms.append(Term((1 << i) >> 1, True, i == 0, hx[i], 0.0, i, i, holds0=False))
    for b in range(T - 1):
        terms.append(_bond_term(b, b + 1, T, jx[b], jy[b], 0.0, mutant, "chain"))
    if L == T:
        t = _bond_term(L - 1, 0, T, jx[L - 1], jy[L - 1], 0.0, mutant, "chain", wrap=True)
        assert t.pxor == 1 << (T - 2) and t.inside
        terms.append(t)
    diag = [(jz[b], b, (b + 1) % L) for b in range(L)] + [(hz[i], i, None) for i in range(L)]
    return terms, diag


def lattice_terms(L, T, bonds, p, mutant=None):
    """the same for k_spmv_lattice: far fields, the far bonds tb[n_in + k - nfx], the inside bonds tb[q], the inside fields; a
    bond's Jz rides on its term"""
    nb = len(bonds)
    p = np.asarray(p)
    jx, jy, jz, hx, hz = p[:nb], p[nb:2 * nb], p[2 * nb:3 * nb], p[3 * nb:3 * nb + L], p[3 * nb + L:]
    tb, n_in = lattice_table(bonds, T)
    nfx = L - T
    nf = nfx + nb - n_in
    terms = []
    last = nf - 1 if mutant == "ragged-last" else nf
    for k in range(last):
        if k < nfx:
            site = T + k
            if not (mutant == "far-field-T" and site == T):
                terms.append(Term((1 << site) >> 1, False, False, hx[site], 0.0, site, site, holds0=False))
        else:
            a, b, t = tb[(0 if mutant == "far-table-offset" else n_in) + k - nfx]
            term = _bond_term(a, b, T, jx[t], jy[t], jz[t], mutant, "lattice")
            term.inside = term.inside and mutant == "straddling-inside"       # a far term is a global read
            terms.append(term)
    for q in range(n_in):
        a, b, t = tb[q]
        terms.append(_bond_term(a, b, T, jx[t], jy[t], jz[t], mutant, "lattice"))
    for i in range(T):
        terms.append(Term((1 << i) >> 1, True, i == 0, hx[i], 0.0, i, i, holds0=False))
    return terms, [(hz[i], i, None) for i in range(L)]


def twin(case, T, cls, x, shift=None, dot=False, skip=False, mutant=None, order=None):
    """one dsea_spmv of the tile kernel at tile 2^T as numpy on row pairs, in fp64; ``order``: a numpy Generator that shuffles
    the terms of every sum (an honest evaluation in another order).  Returns (y, x.y or None)."""
    L, n = case.L, case.n
    if skip:
        return np.full(n, SENTINEL), (SENTINEL if dot else None)
    p = case.p_exact if cls == "exact" else case.p_random
    if case.family == "chain":
        terms, diag = chain_terms(L, T, p, mutant)
    else:
        terms, diag = lattice_terms(L, T, case.bonds, p, mutant)
    if order is not None:
        terms = [terms[i] for i in order.permutation(len(terms))]
        diag = [diag[i] for i in order.permutation(len(diag))]
    x = np.asarray(x, dtype=np.float64)
    X = (x[0::2], x[1::2])
    npair_all, NPAIR = n // 2, 1 << (T - 1)
    pidx = np.arange(npair_all, dtype=np.int64)

    def bit(i, second):
        """bit i of the pair's first / second row"""
        if i == 0:
            return np.full(npair_all, 1 if second else 0, dtype=np.int8)
        return ((pidx >> (i - 1)) & 1).astype(np.int8)

    def zz(a, b, second, holds0):
        if b is None or a == b:
            return (1 - 2 * bit(a, second)).astype(np.float64) if b is None else np.ones(npair_all)
        b0 = bit(a, False) ^ bit(b, False)
        if second and holds0 and mutant != "second-row-zz":
            b0 = b0 ^ 1
        return (1 - 2 * b0).astype(np.float64)

    sums = [np.zeros(npair_all), np.zeros(npair_all)]
    dg = [np.zeros(npair_all), np.zeros(npair_all)]
    for t in terms:
        if t.inside:                                   # pair lp ^ px of the tile's own NPAIR pairs
            partner = (pidx & ~(NPAIR - 1)) | ((pidx ^ t.pxor) & (NPAIR - 1))
        else:
            partner = pidx ^ t.pxor
        for e in (0, 1):
            s = zz(t.a, t.b, e == 1, t.holds0)
            sums[e] = sums[e] + (t.ca - t.cb * s) * X[e ^ int(t.swap)][partner]
            if t.cz != 0.0:
                dg[e] = dg[e] + t.cz * s
    for coef, a, b in diag:
        for e in (0, 1):
            dg[e] = dg[e] + coef * zz(a, b, e == 1, b is not None and (a == 0 or b == 0))
    y = np.empty(n)
    for e in (0, 1):
        y[e::2] = dg[e] * X[e] + sums[e]
    before = y
    if shift is not None:
        y = y - shift * x
    d = None
    if dot:
        prod = x * (before if mutant == "dot-before-shift" else y)
        d = float(np.sum(prod if order is None else prod[order.permutation(n)]))
    return y, d
