"""The finite-temperature layer of the Hubbard model without a GPU (docs/design/28-hubbard-finite-temperature.md): the numpy twin
(tests/hubbard_block_reference.py) against dense linear algebra, the one-species edge matrices against Jordan-Wigner,
``GrandCanonicalEnsemble`` against direct sums over the spectrum of all sectors, the sector bookkeeping of
``hubbard_thermodynamics`` with the device part replaced by the dense reference, and the argument errors that are raised before
any device work."""
import ctypes
import functools
import math
from ctypes import byref, c_int32, c_int64, c_void_p

import numpy as np
import pytest
import torch

import hubbard_block_reference as twin
import hubbard_reference as ref
from dominantsparseeigenad_amd import _lib, operators, thermal
from dominantsparseeigenad_amd.spectral import SpectralMeasure
from dominantsparseeigenad_amd.synthetic import normal_vector
from dominantsparseeigenad_amd.thermal import GrandCanonicalEnsemble

F64 = torch.float64
BETAS = np.array([0.0, 0.25, 1.0, 2.0, 4.0])
MUS = np.array([-1.0, 0.7, 2.5])
ERR_ALIGN = -2     # DSEA_ERR_ALIGN
LOOP4 = ((0, 1), (1, 2), (2, 3), (3, 0), (2, 0))     # a loop 0-1-2, and two bonds written from the higher site: the signs matter


def ring(L):
    return tuple((i, (i + 1) % L) for i in range(L))


@functools.lru_cache(maxsize=None)
def dense_case(L, nup, ndn, seed):
    bonds = ring(L) + ((0, 2),)
    p = normal_vector(ref.nparam(L, bonds), seed)
    H = ref.dense(L, nup, ndn, bonds, p)
    for a in (p, H):
        a.setflags(write=False)
    return bonds, p, H


@pytest.mark.parametrize("L,nup,ndn", [(4, 2, 1), (5, 2, 3)])
def test_the_twin_applies_the_dense_matrix(L, nup, ndn):
    bonds, p, H = dense_case(L, nup, ndn, 9400)
    X = twin.start_block(H.shape[0], 3, 9410)
    for dtype in (np.float64, np.longdouble):
        Y = twin.apply_block(L, nup, ndn, bonds, p, X, dtype)
        assert Y.dtype == dtype
        diff = np.linalg.norm(np.asarray(Y, dtype=np.float64) - H @ X)
        assert diff <= 1e-13 * np.linalg.norm(H @ X), diff


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble], ids=["float64", "longdouble"])
def test_measures_have_the_moments_of_the_vector(dtype):
    """the k-step measure integrates polynomials of degree < 2 k exactly: m = 0 .. 3 at k = 12"""
    L, nup, ndn = 5, 2, 3
    bonds, p, H = dense_case(L, nup, ndn, 9400)
    B = twin.coupling_bound(L, bonds, p)
    assert np.abs(np.linalg.eigvalsh(H)).max() <= B
    Phi = twin.start_block(H.shape[0], 4, 9420) * np.array([1.0, 0.5, 3.0, 1e-3])
    parts = twin.block_measures(L, nup, ndn, bonds, p, Phi, 12, dtype)
    assert len(parts) == 4
    for j, (poles, weights) in enumerate(parts):
        phi = Phi[:, j]
        assert len(poles) == 12
        v = phi.copy()
        for m in range(4):
            exact = float(phi @ v)
            got = float((weights * poles ** m).sum())
            assert abs(got - exact) <= 1e-12 * float(phi @ phi) * B ** m, (j, m, got, exact)
            v = H @ v


def test_a_column_in_the_span_of_three_eigenvectors_breaks_at_step_three():
    L, nup, ndn = 5, 2, 3
    bonds, p, H = dense_case(L, nup, ndn, 9400)
    n = H.shape[0]
    E, V = np.linalg.eigh(H)
    pick, coef = [0, n // 2, n - 1], np.array([0.6, -0.5, 0.7])
    Phi = twin.start_block(n, 2, 9430)
    Phi[:, 0] = V[:, pick] @ coef
    norm2, alphas, betas, steps = twin.block_lanczos(L, nup, ndn, bonds, p, Phi, 12)
    assert list(steps) == [3, 12]
    assert np.all(alphas[3:, 0] == 0.0) and np.all(betas[2:, 0] == 0.0)
    assert np.all(betas[:, 1] > 0.0)
    poles, weights = twin.measure(alphas[:, 0], betas[:, 0], steps[0], norm2[0])
    assert np.abs(poles - E[pick]).max() <= 1e-10
    assert np.abs(weights - coef ** 2).max() <= 1e-10
    assert np.isfinite(alphas).all() and np.isfinite(betas).all()


def test_a_zero_column_has_no_steps():
    L, nup, ndn = 4, 2, 1
    bonds, p, H = dense_case(L, nup, ndn, 9400)
    Phi = twin.start_block(H.shape[0], 2, 9440)
    Phi[:, 1] = 0.0
    norm2, alphas, betas, steps = twin.block_lanczos(L, nup, ndn, bonds, p, Phi, 5)
    assert list(steps) == [5, 0] and norm2[1] == 0.0
    assert np.all(alphas[:, 1] == 0.0) and np.all(betas[:, 1] == 0.0)
    assert twin.measure(alphas[:, 1], betas[:, 1], steps[1], norm2[1])[0].size == 0


EDGES = [(f, m) for f in (0, 4) for m in range(5)] + [(m, f) for m in range(5) for f in (0, 4) if m not in (0, 4)]


@pytest.mark.parametrize("nup,ndn", EDGES)
def test_edge_matrices_against_jordan_wigner(nup, ndn):
    """every sector with a species empty or full at L = 4: the package's and the twin's one-species matrix equal the
    second-quantised Hamiltonian restricted to that sector (the live species orders the rows in both)"""
    L, bonds = 4, LOOP4
    p = normal_vector(ref.nparam(L, bonds), 9500)
    H, leak = ref.dense_jordan_wigner(L, nup, ndn, bonds, p)
    assert leak == 0.0
    count, other = (ndn, nup) if nup in (0, L) else (nup, ndn)
    assert H.shape == (math.comb(L, count),) * 2
    mine = thermal.one_species_matrix(L, bonds, torch.from_numpy(p.copy()), count, other == L).numpy()
    theirs = twin.edge_matrix(L, bonds, p, count, other == L)
    assert np.abs(mine - H).max() <= 1e-13, np.abs(mine - H).max()
    assert np.abs(theirs - H).max() <= 1e-13, np.abs(theirs - H).max()
    if 0 < count < L:
        assert np.abs(H - np.diag(np.diag(H))).max() > 0.0          # (hops are present: the signs were compared)


@functools.lru_cache(maxsize=None)
def exact_model(L, seed):
    """random site-dependent U and eps, random t and V; (bonds, p, the dense spectra of all (L + 1)^2 sectors)"""
    bonds = LOOP4 if L == 4 else ring(L)
    p = normal_vector(ref.nparam(L, bonds), seed)
    p.setflags(write=False)
    return bonds, p, tuple(twin.exact_entries(L, bonds, p))


def as_ensemble(entries):
    return GrandCanonicalEnsemble([(SpectralMeasure(poles, weights, len(poles), len(poles)), nup, ndn)
                                   for poles, weights, nup, ndn in entries])


def direct_sums(entries, beta, mu):
    """the seven functions at one (beta, mu) from plain sums over all eigenstates"""
    E = np.concatenate([e[0] for e in entries])
    N = np.concatenate([np.full(len(e[0]), float(e[2] + e[3])) for e in entries])
    Sz = np.concatenate([np.full(len(e[0]), 0.5 * (e[2] - e[3])) for e in entries])
    K = E - mu * N
    w = np.exp(-beta * K)
    Xi = w.sum()
    mean = lambda a: float((w * a).sum() / Xi)   # noqa: E731
    return {"logZ": math.log(Xi), "energy": mean(E), "density": mean(N),
            "compressibility": beta * (mean(N * N) - mean(N) ** 2),
            "spin_susceptibility": beta * (mean(Sz * Sz) - mean(Sz) ** 2),
            "specific_heat": beta ** 2 * (mean(K * K) - mean(K) ** 2),
            "entropy": math.log(Xi) + beta * (mean(E) - mu * mean(N))}


def test_the_ensemble_equals_direct_sums_over_the_spectrum():
    L = 4
    bonds, p, entries = exact_model(L, 9600)
    assert len(entries) == 25 and sum(len(e[0]) for e in entries) == 4 ** L
    ens = as_ensemble(entries)
    grid_b, grid_m = torch.tensor(BETAS).reshape(5, 1), torch.tensor(MUS).reshape(1, 3)
    for name in ("logZ", "energy", "density", "compressibility", "spin_susceptibility", "specific_heat", "entropy"):
        got = getattr(ens, name)(grid_b, grid_m)
        other = getattr(twin, name)(entries, BETAS, MUS)
        assert got.shape == (5, 3) and got.dtype == F64 and other.shape == (5, 3)
        for i, beta in enumerate(BETAS):
            for j, mu in enumerate(MUS):
                value = direct_sums(entries, beta, mu)[name]
                bar = 1e-10 * max(1.0, abs(value))
                assert abs(float(got[i, j]) - value) <= bar, (name, beta, mu, float(got[i, j]), value)
                assert abs(other[i, j] - value) <= bar, (name, beta, mu, other[i, j], value)
    assert float(ens.logZ(1.0, 0.3)) == pytest.approx(direct_sums(entries, 1.0, 0.3)["logZ"], abs=1e-10)
    assert ens.moment(0) == 4 ** L and twin.moment(entries, 0) == 4 ** L


def test_sectors_of_one_particle_number_are_the_canonical_ensemble():
    """mu only shifts ln Xi by beta mu N; every average is independent of mu and the compressibility vanishes"""
    L = 4
    entries = [e for e in exact_model(L, 9600)[2] if e[2] + e[3] == L]
    ens = as_ensemble(entries)
    beta = torch.tensor(BETAS)
    assert torch.allclose(ens.logZ(beta, 1.5), ens.logZ(beta, 0.0) + beta * 1.5 * L, rtol=0, atol=1e-12)
    for name in ("energy", "spin_susceptibility", "entropy"):
        assert torch.allclose(getattr(ens, name)(beta, 1.5), getattr(ens, name)(beta, 0.0), rtol=0, atol=1e-12), name
    assert torch.allclose(ens.density(beta, 1.5), torch.full((5,), float(L), dtype=F64), rtol=0, atol=1e-12)
    assert float(ens.compressibility(beta, 1.5).abs().max()) <= 1e-12


class _DenseSector:
    """stands in for HubbardOperator where there is no GPU: remembers the sector, and records the order of construction"""
    built = []

    def __init__(self, L, bonds, couplings, nup, ndn, device=None):
        self.args = (int(L), tuple(bonds), couplings.detach().cpu().numpy().copy(), int(nup), int(ndn))
        _DenseSector.built.append((int(nup), int(ndn)))


def _dense_trace_measure(op, R=8, k=100, seed=0, dense_below=256):
    L, bonds, p, nup, ndn = op.args
    poles = np.linalg.eigvalsh(ref.dense(L, nup, ndn, bonds, p))
    return SpectralMeasure(poles, np.ones(len(poles)), float(len(poles)), len(poles))


@pytest.fixture
def host_thermodynamics(monkeypatch):
    """hubbard_thermodynamics with the device part (operator and trace measure of a bulk sector) replaced by dense eigh of the
    reference: the sector loop, the edge sectors, the spin symmetry and the ensemble are the package's own"""
    monkeypatch.setattr(operators, "HubbardOperator", _DenseSector)
    monkeypatch.setattr(thermal, "sector_trace_measure", _dense_trace_measure)
    _DenseSector.built = []

    def run(L, bonds, p, **kw):
        return thermal.hubbard_thermodynamics(L, bonds, torch.from_numpy(np.array(p)), device="cpu", **kw)
    return run


def test_spin_symmetry_on_and_off_agree(host_thermodynamics):
    L = 4
    bonds, p, entries = exact_model(L, 9600)
    off = host_thermodynamics(L, bonds, p, spin_symmetric=False)
    assert sorted(_DenseSector.built) == [(a, b) for a in range(1, L) for b in range(1, L)]
    _DenseSector.built = []
    on = host_thermodynamics(L, bonds, p)
    assert sorted(_DenseSector.built) == [(a, b) for a in range(1, L) for b in range(1, a + 1)]
    assert [(e[1], e[2]) for e in on.entries] == [(a, b) for a in range(L + 1) for b in range(L + 1)]
    grid_b, grid_m = torch.tensor(BETAS).reshape(5, 1), torch.tensor(MUS).reshape(1, 3)
    for name in ("logZ", "energy", "density", "compressibility", "spin_susceptibility", "specific_heat", "entropy"):
        a, b = getattr(on, name)(grid_b, grid_m), getattr(off, name)(grid_b, grid_m)
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), name
        for i, beta in enumerate(BETAS):             # and both are the exact numbers
            for j, mu in enumerate(MUS):
                value = direct_sums(entries, beta, mu)[name]
                assert abs(float(b[i, j]) - value) <= 1e-10 * max(1.0, abs(value)), (name, beta, mu)
    part = host_thermodynamics(L, bonds, p, sectors=[(1, 2), (2, 1), (0, 3), (4, 4)])
    assert [(e[1], e[2]) for e in part.entries] == [(1, 2), (2, 1), (0, 3), (4, 4)]
    assert [len(e[0]) for e in part.entries] == [24, 24, 4, 1]
    assert torch.equal(part.entries[0][0].poles, part.entries[1][0].poles)


def test_the_high_temperature_limit(host_thermodynamics):
    """beta = 0: every one of the 4^L states counts once, whatever mu is"""
    L = 4
    bonds, p, _ = exact_model(L, 9600)
    ens = host_thermodynamics(L, bonds, p)
    mu = torch.tensor(MUS)
    assert float((ens.logZ(0.0, mu) - L * math.log(4.0)).abs().max()) <= 1e-12
    assert float((ens.density(0.0, mu) - L).abs().max()) <= 1e-12
    assert float(ens.spin_susceptibility(0.0, mu).abs().max()) == 0.0
    assert float((ens.entropy(0.0, mu) - L * math.log(4.0)).abs().max()) <= 1e-12


def test_host_side_argument_errors(monkeypatch):
    one = SpectralMeasure([0.0], [1.0], 1.0, 1)
    with pytest.raises(ValueError):
        GrandCanonicalEnsemble([])
    with pytest.raises(ValueError):
        GrandCanonicalEnsemble([one])
    with pytest.raises(ValueError):
        GrandCanonicalEnsemble([(one, 1)])
    with pytest.raises(ValueError):
        GrandCanonicalEnsemble([(SpectralMeasure([], [], 0.0, 0), 1, 1)])
    with pytest.raises(ValueError):
        GrandCanonicalEnsemble([(SpectralMeasure([0.0], [-1.0], 1.0, 1), 1, 1)])
    with pytest.raises(ValueError):
        GrandCanonicalEnsemble([(one, 1, 1)]).logZ(-1.0, 0.0)
    with pytest.raises(ValueError):
        GrandCanonicalEnsemble([(one, 1, 1)]).density(torch.tensor([0.5, -0.5]), 0.0)

    def no_device(*args, **kwargs):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(operators, "HubbardOperator", no_device)
    bonds = ring(4)
    good = torch.zeros(2 * 4 + 2 * 4, dtype=F64)
    with pytest.raises(ValueError):
        thermal.hubbard_thermodynamics(4, bonds, torch.zeros(3, dtype=F64))                       # wrong parameter length
    with pytest.raises(ValueError):
        thermal.hubbard_thermodynamics(4, bonds, good, sectors=[(2, 5)])                          # a sector out of range
    with pytest.raises(ValueError):
        thermal.hubbard_thermodynamics(4, bonds, good, sectors=[(-1, 2)])
    with pytest.raises(ValueError):
        thermal.hubbard_thermodynamics(4, bonds, good, sectors=[(1, 2), (2, 1), (1, 2)])          # a repeated sector
    with pytest.raises(ValueError):
        thermal.hubbard_thermodynamics(4, bonds, good, sectors=[])
    with pytest.raises(ValueError, match=r"\(0, 2\).*edge_dense_max"):
        thermal.hubbard_thermodynamics(4, bonds, good, sectors=[(2, 2), (0, 2)], edge_dense_max=5)
    with pytest.raises(ValueError):
        thermal.hubbard_thermodynamics(4, ((0, 4),), torch.zeros(10, dtype=F64))                  # a bad bond


def test_the_abi_refuses_before_any_device_work():
    """with a handle whose pointers are host dummies: every refused call returns before it could touch them"""
    lib = _lib.load()
    need = c_int64()
    assert lib.dsea_op_hubbard_block_lanczos_scratch_doubles(8, 4, 4, 8, byref(need)) == 0
    assert need.value == 64 + 2 * 8 * math.ceil(math.comb(8, 4) ** 2 / 256)
    assert lib.dsea_op_hubbard_block_lanczos_scratch_doubles(16, 5, 5, 4, byref(need)) == 0
    assert need.value == 64 + 2 * 4 * 4096
    for args in ((8, 4, 4, 3), (8, 4, 4, 0), (8, 4, 4, 16), (8, 0, 4, 8), (8, 4, 8, 8), (41, 20, 1, 8), (18, 9, 9, 8), (1, 1, 1, 8)):
        assert lib.dsea_op_hubbard_block_lanczos_scratch_doubles(*args, byref(need)) == _lib.ERR_ARG, args
    assert lib.dsea_op_hubbard_block_lanczos_scratch_doubles(8, 4, 4, 8, None) == _lib.ERR_ARG

    dummy = (ctypes.c_double * 4096)()
    base = (ctypes.addressof(dummy) + 15) & ~15
    A, B_, odd = c_void_p(base), c_void_p(base + 8192), c_void_p(base + 8)
    flat = (c_int32 * 2)(0, 1)
    h = c_void_p()
    assert lib.dsea_op_create_hubbard(8, 4, 4, 1, flat, A, A, A, A, A, A, A, byref(h)) == 0
    ok = [h, 8, 4, A, B_, A, A, A, A, A, None]      # op, R, k, Q, W, norm2, alphas, betas, steps, scratch, stream

    def lanczos(**change):
        names = ("op", "R", "k", "Q", "W", "norm2", "alphas", "betas", "steps", "scratch", "stream")
        return lib.dsea_op_hubbard_block_lanczos(*[change.get(name, value) for name, value in zip(names, ok)])

    assert lib.dsea_op_hubbard_block_apply(None, 8, A, B_, None) == _lib.ERR_ARG             # null handle
    assert lanczos(op=None) == _lib.ERR_ARG
    for R in (3, 0, 16, -1):
        assert lib.dsea_op_hubbard_block_apply(h, R, A, B_, None) == _lib.ERR_ARG
        assert lanczos(R=R) == _lib.ERR_ARG
    assert lanczos(k=0) == _lib.ERR_ARG and lanczos(k=-2) == _lib.ERR_ARG
    assert lib.dsea_op_hubbard_block_apply(h, 8, A, A, None) == _lib.ERR_ARG                 # X == Y
    assert lanczos(W=A) == _lib.ERR_ARG                                                      # Q == W
    assert lib.dsea_op_hubbard_block_apply(h, 8, None, B_, None) == _lib.ERR_ARG
    assert lib.dsea_op_hubbard_block_apply(h, 8, A, None, None) == _lib.ERR_ARG
    for name in ("Q", "W", "norm2", "alphas", "betas", "steps", "scratch"):
        assert lanczos(**{name: None}) == _lib.ERR_ARG, name
    assert lib.dsea_op_hubbard_block_apply(h, 8, odd, B_, None) == ERR_ALIGN            # a misaligned block
    assert lib.dsea_op_hubbard_block_apply(h, 8, A, odd, None) == ERR_ALIGN
    assert lanczos(Q=odd) == ERR_ALIGN and lanczos(W=odd) == ERR_ALIGN
    # the sector entries refuse this kind, and these entries refuse a sector handle
    assert lib.dsea_op_sector_block_apply(h, 8, A, B_, None) == _lib.ERR_ARG
    assert lib.dsea_op_destroy(h) == 0
    assert lib.dsea_op_create_sector(10, 5, 1, flat, A, A, A, A, byref(h)) == 0
    assert lib.dsea_op_hubbard_block_apply(h, 8, A, B_, None) == _lib.ERR_ARG
    ok[0] = h
    assert lanczos() == _lib.ERR_ARG
    assert lib.dsea_op_destroy(h) == 0
