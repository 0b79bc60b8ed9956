"""The numpy reference of the lattice-symmetry sector (tests/symsector_reference.py) checked against itself and against the
sector reference, and the host side of ``SpinSymmetrySectorOperator`` (group closure, orbit ids, validation); no GPU."""
import math

import numpy as np
import pytest
import torch

import sector_reference as sec
import symsector_reference as ref
from dominantsparseeigenad_amd import operators
from dominantsparseeigenad_amd.operators import (SpinSymmetrySectorOperator, ring_bonds, ring_symmetries, square_bonds,
                                                 symmetry_sector_dim, torus_symmetries)
from dominantsparseeigenad_amd.synthetic import normal_vector

SMALL = ["ring8-k0", "ring8-kpi-p+1-j1j2", "ring8-k0-p-1", "ring7-k0", "ring12-kpi-p-1"]


def random_p(case, seed):
    return normal_vector(2 * case.nb + case.L, seed).copy()


@pytest.mark.parametrize("name", list(ref.TABLE))
def test_counts_are_the_pinned_ones(name):
    case = ref.case(name)
    b = case.basis
    assert (len(case.group), b.n_sector, b.orbits, b.n, b.zero_norm, b.nontrivial) == ref.TABLE[name][1]
    assert b.n_sector == math.comb(case.L, case.ndown)
    if name in ref.HOPS:
        assert (case.n_hops, case.n_dead) == ref.HOPS[name]
    assert bool((np.diff(b.reps) > 0).all()) and b.bucket[0] == 0 and b.bucket[-1] == b.n


@pytest.mark.parametrize("name", SMALL)
def test_row_formula_is_the_dense_projection(name):
    """route (b) = route (a) to 1e-13, B^T B = 1, H(pbar) commutes with B B^T, B^T H(p) B = B^T H(pbar) B, and the spectrum lies
    in that of the full sector"""
    case = ref.case(name)
    n = case.basis.n
    p = random_p(case, 9100 + case.L)
    B = ref.dense_B(case)
    assert np.max(np.abs(B.T @ B - np.eye(n))) < 1e-13
    A = ref.dense_sym(case, p)
    scale = np.max(np.abs(A))
    assert np.max(np.abs(A - A.T)) < 1e-13 * scale
    assert np.max(np.abs(ref.dense_sym(case, p, symmetrised=False) - A)) < 1e-13 * scale
    for seed in (1, 2):
        x = normal_vector(n, 9200 + seed)
        assert np.max(np.abs(ref.apply(case, p, x) - A @ x)) < 1e-13 * scale * np.linalg.norm(x)
    Hbar = sec.dense(case.L, case.ndown, case.bonds, case.pbar(p))
    proj = B @ B.T
    assert np.max(np.abs(Hbar @ proj - proj @ Hbar)) < 1e-13 * np.max(np.abs(Hbar))
    full = np.linalg.eigvalsh(Hbar)
    for e in np.linalg.eigvalsh(A):
        assert np.min(np.abs(full - e)) < 1e-12 * np.max(np.abs(full))
    # the forms are the derivative of v1^T H_sym(p) v2 with respect to p: H_sym is linear in p
    v1, v2 = normal_vector(n, 9301), normal_vector(n, 9302)
    got = ref.forms(case, v1, v2)
    for t in range(p.size):
        e = np.zeros(p.size)
        e[t] = 1.0
        assert abs(got[t] - v1 @ ref.dense_sym(case, e) @ v2) < 1e-13 * np.linalg.norm(v1) * np.linalg.norm(v2) * 4


@pytest.mark.parametrize("name", list(ref.TABLE))
def test_S_is_a_symmetric_projector(name):
    case = ref.case(name)
    S = ref.symmetrise_matrix(case.orbit)
    assert np.array_equal(S, S.T)
    assert np.max(np.abs(S @ S - S)) < 1e-15
    p = random_p(case, 9400)
    assert np.max(np.abs(ref.symmetrise(case.orbit, p) - S @ p)) < 1e-15 * np.max(np.abs(p)) * 64
    nb = case.nb
    assert case.orbit[:nb] != case.orbit[nb:2 * nb] and [v - case.orbit[nb] for v in case.orbit[nb:2 * nb]] == list(case.orbit[:nb])


@pytest.mark.parametrize("L", [6, 8])
def test_the_four_irreps_of_Z2xZ2_are_complete(L):
    """G = <R, T^(L/2)>: four real one-dimensional irreps, so the four n_rep sum to n_sector and the four spectra together are
    the spectrum of the full sector"""
    ndown = L // 2
    bonds = ref.ring(L) + ref.ring(L, 2)
    half = tuple((i + L // 2) % L for i in range(L))
    coup = np.concatenate([np.ones(L), 0.4 * np.ones(L), np.ones(L), 0.7 * np.ones(L), np.zeros(L)])
    total, spectrum = 0, []
    for cr in (1, -1):
        for ch in (1, -1):
            case = ref.Case(L, ndown, bonds, [(ref.reflection(L), cr), (half, ch)])
            assert len(case.group) == 4
            total += case.basis.n
            if case.basis.n:
                spectrum.extend(np.linalg.eigvalsh(ref.dense_sym(case, coup)))
    assert total == math.comb(L, ndown)
    full = np.linalg.eigvalsh(sec.dense(L, ndown, bonds, coup))
    assert np.max(np.abs(np.sort(spectrum) - full)) < 1e-12 * np.max(np.abs(full))


def test_the_host_group_and_orbits_are_those_of_the_reference():
    for name in ref.TABLE:
        (L, ndown, bonds, gens), want = ref.TABLE[name]
        group = operators._close_group(L, gens)
        assert tuple(group) == ref.close_group(L, gens)
        assert operators._orbit_ids(L, bonds, group) == ref.orbit_ids(L, bonds, ref.close_group(L, gens))
    for name in ("ring8-k0", "ring8-kpi-p+1-j1j2", "ring8-k0-p-1", "ring7-k0", "ring12-kpi-p-1"):
        (L, ndown, bonds, gens), want = ref.TABLE[name]
        assert symmetry_sector_dim(L, ndown, gens) == want[3]


def test_the_builders():
    assert ring_symmetries(6) == [((1, 2, 3, 4, 5, 0), 1)]
    assert ring_symmetries(6, "pi", -1) == [((1, 2, 3, 4, 5, 0), -1), ((5, 4, 3, 2, 1, 0), -1)]
    assert [tuple(g) for g in ring_symmetries(12, "pi", -1)] == [tuple(g) for g in ref.TABLE["ring12-kpi-p-1"][0][3]]
    tx, ty = torus_symmetries(4, 6, 0, "pi")
    assert tx == (ref.torus_tx(4, 6), 1) and ty == (ref.torus_ty(4, 6), -1)
    bonds = {frozenset(b) for b in square_bonds(4, 6)}
    for perm, _ in (tx, ty):
        assert {frozenset((perm[a], perm[b])) for a, b in square_bonds(4, 6)} == bonds
    assert len(operators._close_group(24, [tx, ty])) == 24
    with pytest.raises(ValueError):
        ring_symmetries(6, 1)
    with pytest.raises(ValueError):
        torus_symmetries(4, 4, kx=2)


def make(L, bonds, ndown, gens):
    return SpinSymmetrySectorOperator(L, bonds, torch.zeros(2 * len(bonds) + L, dtype=torch.float64), ndown, gens, device="cuda")


def test_validation_errors_come_from_the_host():
    """every one of these is raised before anything touches a device (there is none here)"""
    L = 8
    bonds = ring_bonds(L)
    T, R = ref.translation(L), ref.reflection(L)
    with pytest.raises(ValueError, match="permutation"):
        make(L, bonds, 4, [((0, 0, 1, 2, 3, 4, 5, 6), 1)])
    with pytest.raises(ValueError, match="permutation"):
        make(L, bonds, 4, [(T[:-1], 1)])
    with pytest.raises(ValueError, match=r"\+1 or -1"):
        make(L, bonds, 4, [(T, 2)])
    with pytest.raises(ValueError, match="consistent"):
        make(7, ring_bonds(7), 3, [(ref.translation(7), -1)])          # T^7 = 1 would carry -1
    with pytest.raises(ValueError, match="more than 128"):
        make(L, [(0, 1), (1, 2), (0, 2), (0, 3), (1, 3), (2, 3), (0, 4)], 4,
             [((1, 0, 2, 3, 4, 5, 6, 7), 1), ((1, 2, 3, 4, 5, 6, 7, 0), 1)])      # the symmetric group S_8
    with pytest.raises(ValueError, match="off the bond list"):
        make(L, bonds[:-1], 4, [(T, 1)])                                  # an open chain is not translation invariant
    with pytest.raises(ValueError, match="twice"):
        make(L, bonds + [(1, 0)], 4, [(T, 1)])
    with pytest.raises(ValueError):
        make(L, bonds, 0, [(T, 1)])
    with pytest.raises(ValueError):
        make(41, ring_bonds(41), 2, [(ref.translation(41), 1)])
    with pytest.raises(ValueError):
        make(36, ring_bonds(36), 18, [(ref.translation(36), 1)])          # n_sector >= 2^31
    assert len(operators._close_group(L, [(T, 1), (R, -1)])) == 16
