"""Spin inversion in the symmetry sector (docs/design/23-spin-inversion.md): the numpy reference tests/spinflip_reference.py
checked against the dense B^T H B on top of the sector reference, the pinned counts, and the host side of
``SpinSymmetrySectorOperator`` (closure with flips, site signs, builders, validation); no GPU."""
import numpy as np
import pytest
import torch

import sector_reference as sec
import spinflip_reference as ref
import symsector_reference as sym
from dominantsparseeigenad_amd import operators
from dominantsparseeigenad_amd.operators import (SpinSymmetrySectorOperator, ring_bonds, ring_symmetries, spin_inversion,
                                                 symmetry_sector_dim, torus_symmetries)
from dominantsparseeigenad_amd.synthetic import normal_vector


def small_geometry(kind, L, z):
    """(L, ndown, bonds, generators) of the four kinds of group at ring length L"""
    T, R, F = sym.translation(L), sym.reflection(L), ref.flip_generator(L, z)
    nn = sym.ring(L)
    if kind == "F":
        return L, L // 2, nn, [F]
    if kind == "TRF":
        return L, L // 2, nn, [(T, 1), (R, 1), F]
    if kind == "j1j2":          # (the second neighbours of a ring of 4 are listed twice: nearest neighbours only there)
        return L, L // 2, nn + (sym.ring(L, 2) if L > 4 else []), [(T, -1), (R, -1), F]
    if kind == "TF":
        return L, L // 2, nn, [(T, z, True)]
    raise KeyError(kind)


SMALL = [(kind, L, z) for kind in ("F", "TRF", "j1j2", "TF") for L in (4, 6, 8, 10) for z in (1, -1)]


def random_p(case, seed):
    return normal_vector(2 * case.nb + case.L, seed).copy()


@pytest.mark.parametrize("kind,L,z", SMALL)
def test_row_formula_signed_mean_and_forms_against_the_dense_projection(kind, L, z):
    case = ref.Case(*small_geometry(kind, L, z))
    n = case.basis.n
    p = random_p(case, 9500 + L)
    S = case.S()
    assert np.max(np.abs(S - S.T)) < 1e-15
    assert np.max(np.abs(S @ S - S)) < 1e-15
    pbar = case.pbar(p)
    assert np.max(np.abs(pbar - S @ p)) < 1e-15 * np.max(np.abs(p)) * 64
    assert np.max(np.abs(pbar - p)) > 0.0                              # the couplings are not invariant
    if any(case.flips[g] and all(perm[i] == i for i in range(L)) for g, (perm, _) in enumerate(case.group)):
        assert case.eps == (0,) * L and not pbar[2 * case.nb:].any()  # G contains F: no field survives
    if n == 0:
        return
    B = ref.dense_B(case)
    assert np.max(np.abs(B.T @ B - np.eye(n))) < 1e-13
    A = ref.dense_sym(case, p)                                         # the couplings as they are
    scale = np.max(np.abs(sec.dense(case.L, case.ndown, case.bonds, p)))   # (of H: a sector of one row may have A = 0)
    assert np.max(np.abs(A - A.T)) < 1e-13 * scale
    assert np.max(np.abs(ref.dense_sym(case, pbar) - A)) < 1e-13 * scale
    Hbar = sec.dense(case.L, case.ndown, case.bonds, pbar)
    proj = B @ B.T
    assert np.max(np.abs(Hbar @ proj - proj @ Hbar)) < 1e-13 * np.max(np.abs(Hbar))
    for seed in (1, 2):
        x = normal_vector(n, 9600 + seed)
        assert np.max(np.abs(ref.apply(case, p, x) - A @ x)) < 1e-13 * scale * np.linalg.norm(x)
    v1, v2 = normal_vector(n, 9701), normal_vector(n, 9702)
    dense_forms = np.zeros(p.size)
    for t in range(p.size):
        e = np.zeros(p.size)
        e[t] = 1.0
        dense_forms[t] = v1 @ ref.dense_sym(case, e) @ v2
    bound = 1e-13 * np.linalg.norm(v1) * np.linalg.norm(v2) * 4
    assert np.max(np.abs(ref.forms(case, v1, v2) - S @ dense_forms)) < bound


def test_the_staggered_field_survives_the_TF_mean():
    case = ref.Case(*small_geometry("TF", 10, 1))
    assert case.eps == (1, -1) * 5
    nb = case.nb
    p = np.zeros(2 * nb + 10)
    p[2 * nb:] = 0.7 * np.array(case.eps) + 0.3                       # staggered + uniform
    pbar = case.pbar(p)
    assert np.max(np.abs(pbar[2 * nb:] - 0.7 * np.array(case.eps))) < 1e-15


def heisenberg_ring(L):
    return np.concatenate([np.ones(2 * L), np.zeros(L)])


def test_the_quoted_eigenvalues_of_the_heisenberg_ring_12():
    L, bonds = 12, sym.ring(12)
    p = heisenberg_ring(L)
    full = np.linalg.eigvalsh(sec.dense(L, 6, bonds, p))
    assert np.max(np.abs(full[:2] - [-21.54956367, -20.12617361])) < 1e-8
    want = {1: [-21.54956367, -19.10955733], -1: [-20.12617361, -18.27749764]}
    rows = 0
    for z in (1, -1):
        case = ref.Case(L, 6, bonds, [ref.flip_generator(L, z)])
        lam = np.linalg.eigvalsh(ref.dense_sym(case, p))
        assert np.max(np.abs(lam[:2] - want[z])) < 1e-8
        rows += case.basis.n
    assert rows == 924
    assert abs((want[-1][0] - want[1][0]) - (full[1] - full[0])) < 1e-8


@pytest.mark.parametrize("name", list(ref.TABLE))
def test_counts_are_the_pinned_ones(name):
    ng, n_sector, orbits, zero, n = ref.TABLE[name]
    for k, z in enumerate((1, -1)):
        case = ref.case(name, z)
        b = case.basis
        assert (len(case.group), b.n_sector, b.orbits, b.zero_norm, b.n) == (ng, n_sector, orbits, zero[k], n[k])
        assert bool((np.diff(b.reps) > 0).all()) and b.bucket[0] == 0 and b.bucket[-1] == b.n
        assert any(case.flips) and len(case.flips) == ng


def test_the_eight_sectors_of_ring_12():
    got = [symmetry_sector_dim(12, 6, ring_symmetries(12, k, p, z)) for k in (0, "pi") for p in (1, -1) for z in (1, -1)]
    assert got == [35, 15, 9, 21, 29, 11, 13, 27]
    for k in (0, "pi"):
        for p in (1, -1):
            pair = [symmetry_sector_dim(12, 6, ring_symmetries(12, k, p, z)) for z in (1, -1)]
            assert sum(pair) == symmetry_sector_dim(12, 6, ring_symmetries(12, k, p))


def test_the_host_group_signs_and_dimension_are_those_of_the_reference():
    for name in ref.TABLE:
        for z in (1, -1):
            L, ndown, bonds, gens = ref.geometry(name, z)
            case = ref.case(name, z)
            group, flips = operators._close_group(L, gens, flips=True)
            assert tuple(group) == case.group and tuple(flips) == case.flips
            assert operators._close_group(L, gens) == group
            assert operators._orbit_ids(L, bonds, group) == list(case.orbit)
            assert tuple(operators._site_signs(L, group, flips)) == case.eps
            if case.basis.n_sector <= 3432:
                assert symmetry_sector_dim(L, ndown, gens) == case.basis.n
    # without a flipped generator: the closure of before, flips all False, signs all +1
    gens = ring_symmetries(8, "pi", 1)
    group, flips = operators._close_group(8, [g + (False,) for g in gens], flips=True)
    assert group == operators._close_group(8, gens) and flips == [False] * 16
    assert operators._site_signs(8, group, flips) == [1] * 8


def test_the_builders():
    assert ring_symmetries(6) == [((1, 2, 3, 4, 5, 0), 1)]
    assert ring_symmetries(6, "pi", -1) == [((1, 2, 3, 4, 5, 0), -1), ((5, 4, 3, 2, 1, 0), -1)]
    assert torus_symmetries(4, 6, 0, "pi") == [(sym.torus_tx(4, 6), 1), (sym.torus_ty(4, 6), -1)]
    ident = tuple(range(6))
    assert spin_inversion(6, -1) == (ident, -1, True)
    assert ring_symmetries(6, spin_flip=1) == ring_symmetries(6) + [(ident, 1, True)]
    assert ring_symmetries(6, "pi", -1, spin_flip=-1) == ring_symmetries(6, "pi", -1) + [(ident, -1, True)]
    assert torus_symmetries(2, 3, spin_flip=-1) == torus_symmetries(2, 3) + [(ident, -1, True)]
    for bad in (0, 2, "x"):
        with pytest.raises(ValueError):
            ring_symmetries(6, spin_flip=bad)
        with pytest.raises(ValueError):
            torus_symmetries(2, 3, spin_flip=bad)
    with pytest.raises(ValueError):
        spin_inversion(6, 0)


def make(L, bonds, ndown, gens):
    return SpinSymmetrySectorOperator(L, bonds, torch.zeros(2 * len(bonds) + L, dtype=torch.float64), ndown, gens, device="cuda")


def test_validation_errors_come_from_the_host():
    """every one of these is raised before anything touches a device (there is none here)"""
    L = 8
    bonds = ring_bonds(L)
    T = sym.translation(L)
    F = spin_inversion(L, 1)
    with pytest.raises(ValueError, match="ndown = L / 2"):
        make(L, bonds, 3, [(T, 1), F])
    with pytest.raises(ValueError, match="ndown = L / 2"):
        make(7, ring_bonds(7), 3, [(sym.translation(7), 1, True)])
    with pytest.raises(ValueError, match="ndown = L / 2"):
        symmetry_sector_dim(L, 3, [F])
    for bad in (2, -1, 0.5, "yes", None):
        with pytest.raises(ValueError, match="flip"):
            make(L, bonds, 4, [(T, 1, bad)])
    with pytest.raises(ValueError, match="generator is"):
        make(L, bonds, 4, [(T,)])
    with pytest.raises(ValueError, match="generator is"):
        make(L, bonds, 4, [(T, 1, False, 0)])
    with pytest.raises(ValueError, match="consistent"):
        make(L, bonds, 4, [spin_inversion(L, 1), spin_inversion(L, -1)])
    with pytest.raises(ValueError, match="consistent"):
        make(L, bonds, 4, [(T, 1), (T, -1, True), spin_inversion(L, 1)])   # F is reached as T^-1 (T F) with -1
    Lq, gens = 16, list(ref.geometry("torus4x4-c4", 1)[3])
    assert len(operators._close_group(Lq, gens)) == 128                     # the cap counts the flipped elements
    with pytest.raises(ValueError, match="more than 128"):
        make(Lq, sym.square(4, 4), 8, gens + [(sym.square_mirror(4), 1)])   # 256 elements
    with pytest.raises(ValueError, match="permutation"):
        make(L, bonds, 4, [((0, 0, 1, 2, 3, 4, 5, 6), 1, True)])
