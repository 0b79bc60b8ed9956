"""tests/tile_reference.py and the chain / lattice references of tests/matvec_reference.py proved on the CPU (no GPU): the
vectorised references against the Kronecker-product matrices and the per-row formulas; the exact class really is exact; the
tiled twin equals the row formula at every (L, T) of the table and an honest fp64 evaluation in a random order passes every
random-class bound; every mutant of the twin fails a verdict at every tile where its rule applies; the cases reach the
instantiations they claim."""
import numpy as np
import pytest

import chain_reference
import lattice_reference
import matvec_reference as ref
import tile_reference as tr
from dominantsparseeigenad_amd.synthetic import normal_vector

LD = np.longdouble
TABLE = [(L, tr.tile_log2(L, tune)) for L, tune in tr.SHAPES]


def test_the_cases_are_what_the_table_says():
    tr.assert_tile_cases()
    tr.assert_ritz_cases()


# ---- references against matrices and the per-row formulas -------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 3, 7, 10])
@pytest.mark.parametrize("kind", tr.CHAIN_KINDS)
def test_chain_apply_is_the_dense_matrix(L, kind):
    n = 1 << L
    c = tr.chain_couplings(L, kind, True)
    x = ref.exact_vector(n, 5 + L)
    got, _ = ref.chain_apply(L, c)(x, np.float64)
    assert np.array_equal(got, chain_reference.dense(L, c) @ x)          # exact class: bit for bit
    c = tr.chain_couplings(L, kind, False)
    x = normal_vector(n, 6 + L)
    want, scale = ref.chain_apply(L, c)(x, LD)
    got = chain_reference.dense(L, c) @ x
    assert ref.worst_ratio(np.abs(got.astype(LD) - want), ref.matvec_bound(tr.chain_m(L), scale)) <= 1.0


@pytest.mark.parametrize("L,T", [(3, 3), (7, 7), (10, 7), (10, 10)])
@pytest.mark.parametrize("kind", tr.LATTICE_KINDS)
def test_lattice_apply_is_the_dense_matrix(L, T, kind):
    n = 1 << L
    bonds = tr.lattice_bonds(L, T) if L > 3 else ((0, 1), (1, 2), (2, 0), (1, 0))
    p = tr.lattice_couplings(L, bonds, kind, True)
    x = ref.exact_vector(n, 7 + L)
    got, _ = ref.lattice_apply(L, bonds, p)(x, np.float64)
    assert np.array_equal(got, lattice_reference.dense(L, bonds, p) @ x)
    p = tr.lattice_couplings(L, bonds, kind, False)
    x = normal_vector(n, 8 + L)
    want, scale = ref.lattice_apply(L, bonds, p)(x, LD)
    got = lattice_reference.dense(L, bonds, p) @ x
    assert ref.worst_ratio(np.abs(got.astype(LD) - want), ref.matvec_bound(tr.lattice_m(L, len(bonds)), scale)) <= 1.0


def test_the_magnitude_is_abs_H_abs_x():
    """|ca| + |cb| for an off-diagonal coefficient: never below |ca - cb zz|, equal to it where the signs allow"""
    L = 6
    bonds = tr.lattice_bonds(L, L)
    p = tr.lattice_couplings(L, bonds, "random", False)
    x = normal_vector(1 << L, 3)
    _, scale = ref.lattice_apply(L, bonds, p)(x, np.float64)
    nb = len(bonds)
    terms = lattice_reference.dense_terms(L, bonds)
    tight = sum(np.abs(p[t] * terms[t] + p[nb + t] * terms[nb + t]) for t in range(nb))
    tight = tight + sum(abs(p[t]) * np.abs(terms[t]) for t in range(2 * nb, 3 * nb + 2 * L))
    loose = sum(abs(p[t]) * np.abs(terms[t]) for t in range(3 * nb + 2 * L))
    ax = np.abs(x)
    assert np.all(scale >= (tight @ ax) * (1 - 1e-14)) and np.allclose(scale, loose @ ax, rtol=1e-13, atol=0)


@pytest.mark.parametrize("L,T", sorted(set(TABLE)))
def test_references_equal_the_per_row_formulas_at_every_new_shape(L, T):
    n = 1 << L
    for kind in tr.CHAIN_KINDS:
        case = tr.chain_case(L, kind)
        c = tr.chain_couplings(L, kind, True)
        assert np.array_equal(case.ax, chain_reference.apply(L, c, case.x))
        got = chain_reference.apply(L, tr.chain_couplings(L, kind, False), case.xr) - tr.SHIFT_RANDOM * case.xr
        assert ref.worst_ratio(np.abs(got.astype(LD) - case.want), ref.matvec_bound(case.m, case.scale)) <= 1.0
    for kind in tr.LATTICE_KINDS:
        case = tr.lattice_case(L, T, kind)
        assert np.array_equal(case.ax, lattice_reference.apply(L, case.bonds, case.p_exact, case.x))
        got = lattice_reference.apply(L, case.bonds, case.p_random, case.xr) - tr.SHIFT_RANDOM * case.xr
        assert ref.worst_ratio(np.abs(got.astype(LD) - case.want), ref.matvec_bound(case.m, case.scale)) <= 1.0


# ---- headroom: the exact class is exact -------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,T", sorted(set(TABLE)))
def test_exact_class_is_exact_in_any_precision_and_order(L, T):
    """fp64 equals longdouble bit for bit (no operation rounded), and the twin in a shuffled order gives the same bits; Case
    asserts the headroom and the multiples of 1/64 when it is built"""
    cases = [tr.chain_case(L, kind) for kind in tr.CHAIN_KINDS] + [tr.lattice_case(L, T, kind) for kind in tr.LATTICE_KINDS]
    for case in cases:
        wide, _ = ref.shifted(ref.lattice_apply(L, case.bonds, case.p_exact), case.x, tr.SHIFT_EXACT, LD)
        assert np.array_equal(case.shifted.astype(LD), wide)
        assert float(np.sum(np.asarray(case.x, dtype=LD) * wide)) == case.dot
        assert case.ymax * case.n * 4 * 64 < 2.0 ** 50
        y, d = tr.twin(case, T, "exact", case.x, shift=tr.SHIFT_EXACT, dot=True, order=np.random.default_rng(L))
        assert np.array_equal(y, case.shifted) and d == case.dot


def test_forms_references_are_exact_and_bounded():
    for L, bonds in ((9, None), (10, tr.lattice_bonds(10, 7))):
        case = tr.FormsCase(L, bonds, 55)
        if bonds is None:
            plain = chain_reference.forms(L, case.v1, case.v2).reshape(-1)
            honest = chain_reference.forms(L, case.r1, case.r2).reshape(-1)
            H = chain_reference.dense_terms(L)
            dense = np.array([case.r1 @ H[f][i] @ case.r2 for f in range(5) for i in range(L)])
        else:
            plain = lattice_reference.forms(L, bonds, case.v1, case.v2)
            honest = lattice_reference.forms(L, bonds, case.r1, case.r2)
            dense = np.array([case.r1 @ M @ case.r2 for M in lattice_reference.dense_terms(L, bonds)])
        assert np.array_equal(plain, case.want)
        assert ref.worst_ratio(np.abs(honest.astype(LD) - case.want_r), case.bound) <= 1.0
        assert ref.worst_ratio(np.abs(dense.astype(LD) - case.want_r), 2 * case.bound) <= 1.0      # (two sums of n terms each)
        wrong = honest.copy()
        wrong[1] += case.r1[3] * case.r2[5]                                                     # one term too many
        assert ref.worst_ratio(np.abs(wrong.astype(LD) - case.want_r), case.bound) > 1.0


# ---- the tiled twin ---------------------------------------------------------------------------------------------------------
def twin_run(case, T, mutant=None, order=None):
    return lambda cls, x, **kw: tr.twin(case, T, cls, x, mutant=mutant, order=order, **kw)


def table_cases(L, T, random=True):
    return [tr.chain_case(L, kind, random) for kind in tr.CHAIN_KINDS] + [tr.lattice_case(L, T, kind, random)
                                                                            for kind in tr.LATTICE_KINDS]


@pytest.mark.parametrize("L,T", TABLE)
def test_twin_passes_every_verdict(L, T):
    """the kernel's composition in the kernel's order (exact class bit for bit) and, for the random class, in a random order"""
    worst = 0.0
    for case in table_cases(L, T):
        tag = "%s twin L=%d T=%d" % (case.family, L, T)
        worst = max(worst, tr.judge(tag, case, twin_run(case, T), log=lambda s: None))
        worst = max(worst, tr.judge(tag, case, twin_run(case, T, order=np.random.default_rng(100 * L + T)), log=lambda s: None))
    print("L=%d T=%d: honest fp64, worst error / bound %.3f" % (L, T, worst))


def test_twin_at_the_full_bond_table():
    case = tr.lattice_case(12, 9, "random", True, True)
    tr.judge("lattice twin, full table", case, twin_run(case, 9, order=np.random.default_rng(9)))


def test_twin_at_the_whole_vector_tile_4():
    for kind in tr.LATTICE_KINDS:
        case = tr.lattice_case(4, 4, kind)
        tr.judge("lattice twin L=4", case, twin_run(case, 4, order=np.random.default_rng(4)))
    assert tr.lattice_tiles_of_the_older_suite() == [2, 3, 5, 6, 11]


def test_twin_where_blocks_walk_two_tiles():
    L, T = tr.WALK
    for case in (tr.chain_case(L, "random", False), tr.lattice_case(L, T, "random", False)):
        tr.judge("%s twin L=%d T=%d" % (case.family, L, T), case, twin_run(case, T))


@pytest.mark.parametrize("T", tr.TILES)
@pytest.mark.parametrize("mutant", tr.MUTANTS)
def test_every_mutant_fails_at_every_tile(mutant, T):
    """at the smallest shape of the tile where the rule applies (the whole vector if it applies there, and the eight-tile
    shape too), in BOTH classes: the exact verdict and the random bound each reject it"""
    hit = 0
    for L in (T, T + 3):
        for family, case in (("chain", tr.chain_case(L, "random")), ("lattice", tr.lattice_case(L, T, "random"))):
            if not tr.mutant_applies(mutant, family, L, T):
                continue
            hit += 1
            for classes in (("exact",), ("random",)):
                with pytest.raises(AssertionError):
                    tr.judge("mutant", case, twin_run(case, T, mutant), log=lambda s: None, classes=classes)
    assert hit >= (1 if mutant == "far-table-offset" else 2)


def test_mutants_are_named_rules_and_apply_where_claimed():
    assert len(tr.MUTANTS) == 7
    for mutant in tr.MUTANTS:
        for T in tr.TILES:
            assert tr.mutant_applies(mutant, "lattice", T + 3, T)
            assert tr.mutant_applies(mutant, "chain", T + 3, T) == (mutant != "far-table-offset")
            whole = mutant in ("wrap-unswapped", "second-row-zz", "dot-before-shift")
            assert tr.mutant_applies(mutant, "chain", T, T) == whole == tr.mutant_applies(mutant, "lattice", T, T)
