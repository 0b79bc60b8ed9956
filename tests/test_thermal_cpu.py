"""The finite-temperature layer without a GPU (docs/design/27-finite-temperature.md): the numpy twin of the basis-free block
recurrence (tests/sector_block_reference.py) against dense linear algebra, ``ThermalEnsemble`` against direct sums over the
spectrum, a closed form for tr H^2, and the argument errors that are raised before any device work."""
import functools
import math
from ctypes import byref, c_int64

import numpy as np
import pytest
import torch

import lattice_reference
import sector_block_reference as twin
import sector_reference as ref
from dominantsparseeigenad_amd import _lib, thermal
from dominantsparseeigenad_amd.operators import ring_bonds
from dominantsparseeigenad_amd.spectral import SpectralMeasure
from dominantsparseeigenad_amd.synthetic import normal_vector
from dominantsparseeigenad_amd.thermal import ThermalEnsemble

F64 = torch.float64
BETAS = np.array([0.0, 0.1, 0.5, 1.0, 2.0])


def model(L, seed):
    """ring + a few random bonds (all distinct), random couplings"""
    bonds = list(ring_bonds(L))
    for bond in lattice_reference.random_bonds(L, 2 * L, seed):
        if len(bonds) < L + 4 and all(set(bond) != set(b) for b in bonds):
            bonds.append(tuple(bond))
    bonds = tuple(bonds)
    return bonds, normal_vector(ref.nparam(L, bonds), seed + 1)


@functools.lru_cache(maxsize=None)
def dense_case(L, ndown, seed):
    bonds, p = model(L, seed)
    H = ref.dense(L, ndown, bonds, p)
    H.setflags(write=False)
    return bonds, p, H


def test_the_twin_applies_the_dense_matrix():
    bonds, p, H = dense_case(8, 4, 9100)
    X = twin.start_block(H.shape[0], 3, 9110)
    for dtype in (np.float64, np.longdouble):
        Y = twin.apply_block(8, 4, bonds, p, X, dtype)
        assert Y.dtype == dtype
        assert np.abs(np.asarray(Y, dtype=np.float64) - H @ X).max() <= 1e-13 * np.abs(H @ X).max()


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble], ids=["float64", "longdouble"])
def test_measures_have_the_moments_of_the_vector(dtype):
    """the k-step measure integrates polynomials of degree < 2 k exactly: m = 0 .. 3 at k = 12, the bar of note 24"""
    bonds, p, H = dense_case(8, 4, 9100)
    Phi = twin.start_block(H.shape[0], 4, 9120) * np.array([1.0, 0.5, 3.0, 1e-3])
    norm_H = np.abs(np.linalg.eigvalsh(H)).max()
    parts = twin.block_measures(8, 4, bonds, p, Phi, 12, dtype)
    assert len(parts) == 4
    for j, (poles, weights) in enumerate(parts):
        phi = Phi[:, j]
        assert len(poles) == 12
        v = phi.copy()
        for m in range(4):
            exact = float(phi @ v)
            got = float((weights * poles ** m).sum())
            assert abs(got - exact) <= 1e-12 * float(phi @ phi) * norm_H ** m, (j, m, got, exact)
            v = H @ v


def test_a_column_in_the_span_of_three_eigenvectors_breaks_at_step_three():
    bonds, p, H = dense_case(8, 4, 9100)
    n = H.shape[0]
    E, V = np.linalg.eigh(H)
    pick, coef = [0, n // 2, n - 1], np.array([0.6, -0.5, 0.7])
    Phi = twin.start_block(n, 2, 9130)
    Phi[:, 0] = V[:, pick] @ coef
    norm2, alphas, betas, steps = twin.block_lanczos(8, 4, bonds, p, Phi, 12)
    assert list(steps) == [3, 12]
    assert np.all(alphas[3:, 0] == 0.0) and np.all(betas[2:, 0] == 0.0)
    assert np.all(betas[:, 1] > 0.0)
    poles, weights = twin.measure(alphas[:, 0], betas[:, 0], steps[0], norm2[0])
    assert np.abs(poles - E[pick]).max() <= 1e-10
    assert np.abs(weights - coef ** 2).max() <= 1e-10
    assert np.isfinite(alphas).all() and np.isfinite(betas).all()


def test_a_zero_column_has_no_steps():
    bonds, p, H = dense_case(8, 4, 9100)
    Phi = twin.start_block(H.shape[0], 2, 9140)
    Phi[:, 1] = 0.0
    norm2, alphas, betas, steps = twin.block_lanczos(8, 4, bonds, p, Phi, 5)
    assert list(steps) == [5, 0] and norm2[1] == 0.0
    assert np.all(alphas[:, 1] == 0.0) and np.all(betas[:, 1] == 0.0)
    assert twin.measure(alphas[:, 1], betas[:, 1], steps[1], norm2[1])[0].size == 0


@functools.lru_cache(maxsize=None)
def exact_ensemble(L, seed):
    bonds, p = model(L, seed)
    entries = twin.exact_entries(L, bonds, p)
    ens = ThermalEnsemble([(SpectralMeasure(poles, weights, len(poles), len(poles)), m) for poles, weights, m in entries])
    return bonds, p, entries, ens


def test_the_ensemble_equals_direct_sums_over_the_spectrum():
    """L = 6, all seven sectors (the two one-state sectors from their closed form): Z, E, C, S, chi from plain sums"""
    L = 6
    bonds, p, entries, ens = exact_ensemble(L, 9200)
    assert [len(e[0]) for e in entries] == [math.comb(L, d) for d in range(L + 1)]
    # the one-state sectors against the full-space diagonal: all z = +1 and all z = -1
    jxy, jz, hz = ref.split(L, bonds, p)
    assert entries[0][0][0] == pytest.approx(jz.sum() + hz.sum(), abs=1e-13)
    assert entries[L][0][0] == pytest.approx(jz.sum() - hz.sum(), abs=1e-13)
    E = np.concatenate([e[0] for e in entries])
    m = np.concatenate([np.full(len(e[0]), e[2]) for e in entries])
    assert E.size == 2 ** L
    for i, beta in enumerate(BETAS):
        w = np.exp(-beta * E)
        Z = w.sum()
        e1, e2 = (w * E).sum() / Z, (w * E * E).sum() / Z
        m1, m2 = (w * m).sum() / Z, (w * m * m).sum() / Z
        want = {"logZ": math.log(Z), "energy": e1, "specific_heat": beta ** 2 * (e2 - e1 ** 2), "entropy": math.log(Z) + beta * e1,
                "susceptibility": beta * (m2 - m1 ** 2)}
        for name, value in want.items():
            got = float(getattr(ens, name)(torch.tensor(BETAS))[i])
            assert abs(got - value) <= 1e-10 * max(1.0, abs(value)), (name, beta, got, value)
            other = float(getattr(twin, name)(entries, BETAS)[i])
            assert abs(other - value) <= 1e-10 * max(1.0, abs(value)), (name, beta, other, value)
    assert float(ens.logZ(0.0)) == pytest.approx(L * math.log(2.0), abs=1e-13)
    assert ens.logZ(torch.tensor(BETAS).reshape(5, 1)).shape == (5, 1)


def test_the_second_moment_has_its_closed_form():
    """tr H^2 / 2^L = sum_t (2 Jxy_t^2 + Jz_t^2) + sum_i hz_i^2 for distinct bonds"""
    L = 8
    bonds, p, entries, ens = exact_ensemble(L, 9300)
    assert len({frozenset(b) for b in bonds}) == len(bonds)
    jxy, jz, hz = ref.split(L, bonds, p)
    want = float((2.0 * jxy ** 2 + jz ** 2).sum() + (hz ** 2).sum())
    assert ens.moment(0) == 2 ** L
    assert abs(ens.moment(2) / 2 ** L - want) <= 1e-12 * want
    assert abs(twin.moment(entries, 2) / 2 ** L - want) <= 1e-12 * want
    assert abs(ens.moment(1) / 2 ** L) <= 1e-12 * twin.coupling_bound(L, bonds, p)     # H is traceless


def test_the_stochastic_twin_reproduces_itself_and_sums_to_the_dimension():
    L, ndown = 8, 4
    bonds, p = model(L, 9300)
    a = twin.trace_measure(L, ndown, bonds, p, R=4, k=10, seed=5, dense_below=0)
    b = twin.trace_measure(L, ndown, bonds, p, R=4, k=10, seed=5, dense_below=0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[0].size == 40 and a[1].sum() == pytest.approx(math.comb(L, ndown), rel=1e-12)


def test_block_pieces():
    assert thermal.block_pieces(1) == [(0, 1)]
    assert thermal.block_pieces(8) == [(0, 8)]
    assert thermal.block_pieces(3) == [(0, 2), (2, 1)]
    assert thermal.block_pieces(13) == [(0, 8), (8, 4), (12, 1)]
    assert thermal.block_pieces(23) == [(0, 8), (8, 8), (16, 4), (20, 2), (22, 1)]
    with pytest.raises(ValueError):
        thermal.block_pieces(0)


def test_host_side_argument_errors():
    one = SpectralMeasure([0.0], [1.0], 1.0, 1)
    with pytest.raises(ValueError):
        ThermalEnsemble([])
    with pytest.raises(ValueError):
        ThermalEnsemble([one])
    with pytest.raises(ValueError):
        ThermalEnsemble([(SpectralMeasure([], [], 0.0, 0), 0.0)])
    with pytest.raises(ValueError):
        ThermalEnsemble([(SpectralMeasure([0.0], [-1.0], 1.0, 1), 0.0)])
    with pytest.raises(ValueError):
        ThermalEnsemble([(one, 0.5)]).logZ(-1.0)

    class NotASector:
        n = 4
    for call in (lambda: thermal.block_lanczos_measures(NotASector(), torch.zeros(4, 2, dtype=F64), 3),
                 lambda: thermal.sector_trace_measure(NotASector())):
        with pytest.raises(ValueError, match="SpinSectorOperator"):
            call()
    with pytest.raises(ValueError):
        thermal.spin_thermodynamics(4, ring_bonds(4), torch.zeros(3, dtype=F64))            # wrong parameter length
    with pytest.raises(ValueError):
        thermal.spin_thermodynamics(4, ring_bonds(4), torch.zeros(12, dtype=F64), sectors=[5])
    with pytest.raises(ValueError):
        thermal.spin_thermodynamics(4, ring_bonds(4), torch.zeros(12, dtype=F64), sectors=[1, 1])


def test_the_abi_refuses_before_any_device_work():
    lib = _lib.load()
    need = c_int64()
    assert lib.dsea_op_sector_block_lanczos_scratch_doubles(12, 6, 8, byref(need)) == 0
    assert need.value == 64 + 2 * 8 * math.ceil(math.comb(12, 6) / 256)
    assert lib.dsea_op_sector_block_lanczos_scratch_doubles(24, 12, 8, byref(need)) == 0
    assert need.value == 64 + 2 * 8 * 4096
    for args in ((12, 6, 3), (12, 6, 0), (12, 6, 16), (12, 0, 8), (41, 20, 8)):
        assert lib.dsea_op_sector_block_lanczos_scratch_doubles(*args, byref(need)) == _lib.ERR_ARG
    assert lib.dsea_op_sector_block_lanczos_scratch_doubles(12, 6, 8, None) == _lib.ERR_ARG
    assert lib.dsea_op_sector_block_apply(None, 8, None, None, None) == _lib.ERR_ARG
    assert lib.dsea_op_sector_block_lanczos(None, 8, 4, None, None, None, None, None, None, None, None) == _lib.ERR_ARG
