"""The Chebyshev block propagator without a GPU (docs/design/31-chebyshev-propagator.md): the numpy twin against dense linear
algebra, the coefficient and order functions of the package, the thermal-pure-quantum-state sums with every sector exact against
the full 2^L space, and every argument error that must be raised before any device work.

Bar of the twin checks: max(1e-13, 10 x the twin's own float64-longdouble deviation) ||X||, both measured on the same inputs.
"""
import ctypes
import functools
import math
from ctypes import byref, c_void_p

import numpy as np
import pytest
import torch

import lattice_reference
import sector_cheb_reference as twin
import sector_reference as ref
from dominantsparseeigenad_amd import _lib, chebyshev, thermal
from dominantsparseeigenad_amd.operators import ring_bonds
from dominantsparseeigenad_amd.synthetic import normal_vector

LD = np.longdouble
CASES = {"L8-4": (8, 4, tuple(lattice_reference.random_bonds(8, 12, 3108))), "L6-3": (6, 3, tuple(ring_bonds(6)))}


@functools.lru_cache(maxsize=None)
def case(name):
    """(L, ndown, bonds, couplings, X (n, 3), theta, V, spectral bounds) computed once and never written to"""
    L, ndown, bonds = CASES[name]
    p = normal_vector(ref.nparam(L, bonds), 3100 + L).copy()
    n = math.comb(L, ndown)
    X = np.stack([normal_vector(n, 3150 + L + j) for j in range(3)], axis=1)
    theta, V = np.linalg.eigh(ref.dense(L, ndown, bonds, p))
    spread = theta[-1] - theta[0]
    bounds = (theta[0] - 0.05 * spread, theta[-1] + 0.05 * spread)
    for a in (p, X, theta, V):
        a.setflags(write=False)
    return L, ndown, bonds, p, X, theta, V, bounds


def bar(deviation, X):
    return max(1e-13, 10.0 * deviation) * np.linalg.norm(X)


@pytest.mark.parametrize("tau_h", [0.5, 5.0, 40.0])
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_twin_propagates_like_the_dense_exponential(name, tau_h):
    L, ndown, bonds, p, X, theta, V, bounds = case(name)
    tau = tau_h / (0.5 * (bounds[1] - bounds[0]))
    Y, shift = twin.expm(L, ndown, bonds, p, X, tau, bounds)
    Yl, _ = twin.expm(L, ndown, bonds, p, X, tau, bounds, dtype=LD)
    assert shift == bounds[0]
    want = V @ (np.exp(-tau * (theta - shift))[:, None] * (V.T @ X))
    deviation = float(np.linalg.norm((Y - Yl).astype(np.float64)) / np.linalg.norm(X))
    err = float(np.linalg.norm(Y - want))
    print("%s tau h = %g: |Y - dense| = %.2e, twin fp64 - longdouble %.2e ||X||, bar %.2e" % (name, tau_h, err, deviation, bar(deviation, X)))
    assert err <= bar(deviation, X)


@pytest.mark.parametrize("tau_h", [0.5, 5.0, 40.0])
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_twin_evolves_like_the_dense_cos_and_sin(name, tau_h):
    L, ndown, bonds, p, X, theta, V, bounds = case(name)
    t = tau_h / (0.5 * (bounds[1] - bounds[0]))
    psi = X[:, :1] + 1j * X[:, 1:2]
    got = twin.time_evolve(L, ndown, bonds, p, psi, t, bounds)
    long = twin.time_evolve(L, ndown, bonds, p, psi, t, bounds, dtype=LD)
    want = V @ (np.exp(-1j * t * theta)[:, None] * (V.T @ psi))
    deviation = float(np.linalg.norm((got - long).astype(np.complex128)) / np.linalg.norm(psi))
    err = float(np.linalg.norm(got - want))
    print("%s h t = %g: |psi(t) - dense| = %.2e, twin fp64 - longdouble %.2e ||psi||, bar %.2e"
          % (name, tau_h, err, deviation, bar(deviation, psi)))
    assert err <= bar(deviation, psi)
    real = twin.time_evolve(L, ndown, bonds, p, X[:, :2], t, bounds)               # cos and sin themselves
    want = V @ (np.exp(-1j * t * theta)[:, None] * (V.T @ X[:, :2]))
    assert np.linalg.norm(real - want) <= bar(deviation, X[:, :2])


@pytest.mark.parametrize("x", [0.0, 0.5, 5.0, 40.0])
def test_the_coefficients_of_the_exponential(x):
    M = chebyshev.exp_order(x)
    c = chebyshev.chebyshev_coefficients(lambda s: np.exp(-LD(x) * (s + LD(1))), M)
    assert c.dtype == np.float64 and c.shape == (M,)
    assert M == twin.exp_order(x)
    assert np.abs(c - twin.coefficients(twin.exp_function(x), M)).max() <= 2.3e-16  # (both round longdouble sums of terms <= 1)
    full = chebyshev.chebyshev_coefficients(lambda s: np.exp(-LD(x) * (s + LD(1))), M, nodes=4 * M)
    assert np.abs(c - full).max() <= 4e-16                                         # more nodes change nothing
    assert abs(c.sum() - math.exp(-2.0 * x)) <= 1e-15 * M                          # sum_m c_m T_m(1) = f(1), c_0 halved
    assert abs((c * (-1.0) ** np.arange(M)).sum() - 1.0) <= 1e-15 * M              # f(-1) = 1
    assert np.abs(c).max() <= 1.0
    try:
        from scipy.special import ive
    except ImportError:
        return
    want = 2.0 * (-1.0) ** np.arange(M) * ive(np.arange(M), x)                     # e^{-x} e^{-x s} = e^{-x} sum' 2 (-1)^m I_m(x) T_m(s)
    want[0] /= 2.0
    assert np.abs(c - want).max() <= 1e-15


def test_c0_is_halved():
    c = chebyshev.chebyshev_coefficients(lambda s: 0 * s + LD(3), 4)
    assert abs(c[0] - 3.0) <= 1e-15 and np.abs(c[1:]).max() <= 1e-15
    c = chebyshev.chebyshev_coefficients(lambda s: 2 * s * s - 1 + s, 5)           # T_2 + T_1
    assert np.abs(c - np.array([0.0, 1.0, 1.0, 0.0, 0.0])).max() <= 1e-15


def test_exp_order_is_monotone():
    xs = [0.0, 0.01, 0.1, 0.5, 1.0, 2.0, 5.0, 10.0, 20.0, 40.0, 80.0, 160.0]
    orders = [chebyshev.exp_order(x) for x in xs]
    print("exp_order:", dict(zip(xs, orders)))
    assert orders == sorted(orders) and orders[0] >= 2 and orders[-1] > orders[0]
    assert chebyshev.exp_order(40.0, tol=1e-8) <= chebyshev.exp_order(40.0, tol=1e-15)
    x = 40.0
    M = chebyshev.exp_order(x)
    c = np.abs(chebyshev.chebyshev_coefficients(lambda s: np.exp(-LD(x) * (s + LD(1))), 2 * M))
    assert c[M:].max() < 1e-15 * c.max() <= c[M - 1]                                # the rule itself


def test_a_function_that_vanishes_has_order_two():
    """sin(H t) at t = 0: every coefficient is exactly zero, and the order search must end"""
    zero = lambda s: np.sin(LD(0) * s + LD(0))  # noqa: E731
    assert chebyshev.truncation_order(zero, 24) == 2 and twin.order(zero, 24) == 2
    assert chebyshev.truncation_order(lambda s: 0 * s + LD(1), 24) == 2            # a constant: c_0 alone
    L, ndown, bonds, p, X, _, _, bounds = case("L6-3")
    psi = X[:, :1] + 1j * X[:, 1:2]
    assert np.abs(twin.evolution_coefficients(0.0, bounds) - np.array([[1.0, 0.0], [0.0, 0.0]])).max() <= 1e-18
    got = twin.time_evolve(L, ndown, bonds, p, psi, 0.0, bounds)
    assert np.abs(got - psi).max() <= 4e-16 * np.abs(psi).max()


def test_long_expansions_need_no_quadratic_memory():
    """h t = 300: an expansion of 800 coefficients on 1600 nodes, in rows of 32"""
    import tracemalloc
    w = LD(300)
    tracemalloc.start()
    M = chebyshev.truncation_order(lambda s: np.cos(w * s), 400)
    peak = tracemalloc.get_traced_memory()[1]
    tracemalloc.stop()
    assert 300 < M <= 400
    assert peak < 4 * 2 ** 20                    # (the dense 800 x 1600 longdouble matrix alone would be 20 MB)


BETAS = np.array([0.0, 0.3, 1.0, 2.5, 6.0])


@functools.lru_cache(maxsize=None)
def thermal_case():
    L = 6
    bonds = tuple(ring_bonds(L)) + ((0, 3), (1, 4))
    p = normal_vector(ref.nparam(L, bonds), 3160).copy()
    return L, bonds, p, twin.thermal_correlations(L, bonds, p, BETAS), twin.full_space_correlations(L, bonds, p, BETAS)


@pytest.mark.parametrize("key", ["logZ", "energy", "xy", "zz", "z"])
def test_the_sector_sums_are_the_full_space_thermal_averages(key):
    _, _, _, got, want = thermal_case()
    worst = float((np.abs(got[key] - want[key]) / np.maximum(1.0, np.abs(want[key]))).max())
    print("%s: worst deviation %.2e (bar 1e-10 max(1, |value|))" % (key, worst))
    assert got[key].shape == want[key].shape and worst <= 1e-10


def test_the_diagonals_and_the_infinite_temperature_point():
    L, _, _, got, _ = thermal_case()
    for b in range(len(BETAS)):
        assert np.abs(np.diag(got["zz"][b]) - 1.0).max() <= 1e-14 and np.abs(np.diag(got["xy"][b]) - 2.0).max() <= 1e-14
    off = ~np.eye(L, dtype=bool)
    assert np.abs(got["zz"][0][off]).max() <= 1e-13 and np.abs(got["xy"][0][off]).max() <= 1e-13      # beta = 0: no correlations
    assert abs(got["logZ"][0] - L * math.log(2.0)) <= 1e-13


def test_the_stochastic_twin_tracks_its_longdouble_self():
    """one sampled sector (n = 20 > dense_below) beside exact ones: the fp64 sums against the longdouble sums"""
    L, bonds, p, _, _ = thermal_case()
    got = twin.thermal_correlations(L, bonds, p, BETAS, R=3, seed=5, dense_below=15)
    long = twin.thermal_correlations(L, bonds, p, BETAS, R=3, seed=5, dense_below=15, dtype=LD)
    for key in got:
        assert np.abs(got[key] - long[key].astype(np.float64)).max() <= 1e-12


class _NoOperator:
    n, device = 4, "cpu"


def test_host_side_argument_errors():
    op = _NoOperator()
    X = torch.zeros((4, 2), dtype=torch.float64)
    good = np.array([0.5, 0.25, 0.125])
    for bad in (lambda s: s[:3], lambda s: np.zeros((2, 2))):
        with pytest.raises(ValueError):
            chebyshev.chebyshev_coefficients(bad, 4)
    for call in (lambda: chebyshev.chebyshev_coefficients(np.cos, 0),
                 lambda: chebyshev.chebyshev_coefficients(np.cos, 4, nodes=7),
                 lambda: chebyshev.exp_order(-1.0),
                 lambda: chebyshev.exp_order(float("nan")),
                 lambda: chebyshev.exp_order(1.0, tol=0.0),
                 lambda: chebyshev.spectral_bounds(op),                                     # not a sector operator
                 lambda: chebyshev.chebyshev_apply(op, X, good, (-1.0, 1.0), fused=True),   # no fused kernel for this kind
                 lambda: chebyshev.chebyshev_apply(op, X, good, (-1.0, 1.0)),               # nothing with apply_block
                 lambda: chebyshev.chebyshev_apply(op, X, good[:1], (-1.0, 1.0)),           # M < 2
                 lambda: chebyshev.chebyshev_apply(op, X, np.zeros((2, 2, 3)), (-1.0, 1.0)),
                 lambda: chebyshev.chebyshev_apply(op, X, [0.5, float("inf")], (-1.0, 1.0)),
                 lambda: chebyshev.chebyshev_apply(op, X, good, (1.0, 1.0)),                # empty interval
                 lambda: chebyshev.chebyshev_apply(op, X, good, (-1.0, float("inf"))),
                 lambda: chebyshev.chebyshev_apply(op, X, good, (-1.0,)),
                 lambda: chebyshev.expm_block(op, X, -0.1, (-1.0, 1.0)),
                 lambda: chebyshev.expm_block(op, X, float("nan"), (-1.0, 1.0)),
                 lambda: chebyshev.expm_block(op, X, 1.0, (2.0, 1.0)),
                 lambda: chebyshev.time_evolve(op, X, float("inf"), (-1.0, 1.0)),
                 lambda: chebyshev.time_evolve(op, [1.0, 2.0], 1.0, (-1.0, 1.0)),
                 lambda: chebyshev.time_evolve(op, torch.zeros((2, 2, 2)), 1.0, (-1.0, 1.0))):
        with pytest.raises(ValueError):
            call()

    class _WithBlock(_NoOperator):
        def apply_block(self, X):
            return X

    with pytest.raises(ValueError):                                                      # a block that is not on the device
        chebyshev.chebyshev_apply(_WithBlock(), X, good, (-1.0, 1.0))
    bonds = ring_bonds(6)
    c = torch.zeros(2 * 6 + 6, dtype=torch.float64)
    for betas in ([1.0, 0.5], [-0.1, 1.0], [], [0.0, float("nan")]):
        with pytest.raises(ValueError):
            thermal.thermal_correlations(6, bonds, c, betas)
    for call in (lambda: thermal.thermal_correlations(6, bonds, c[:-1], [0.0, 1.0]),
                 lambda: thermal.thermal_correlations(6, bonds, c, [0.0, 1.0], R=0),
                 lambda: thermal.thermal_correlations(6, bonds, c, [0.0, 1.0], sectors=[1, 1]),
                 lambda: thermal.thermal_correlations(6, bonds, c, [0.0, 1.0], sectors=[7])):
        with pytest.raises(ValueError):
            call()


def test_the_edge_sectors_need_no_device():
    """ndown = 0 and ndown = L alone: host arithmetic only"""
    L, bonds = 6, ring_bonds(6)
    p = normal_vector(2 * 6 + 6, 3170)
    out = thermal.thermal_correlations(L, bonds, torch.from_numpy(p.copy()), [0.0, 0.7], sectors=[0, L])
    jz, hz = p[6:12].sum(), p[12:].sum()
    want = np.logaddexp(-0.7 * (jz + hz), -0.7 * (jz - hz))
    assert abs(float(out.logZ[1]) - want) <= 1e-13 and abs(float(out.logZ[0]) - math.log(2.0)) <= 1e-15
    w = np.exp(-0.7 * (jz + hz) - want)
    assert np.abs(out.z[1].numpy() - (2.0 * w - 1.0)).max() <= 1e-13
    assert torch.equal(out.zz, torch.ones((2, L, L), dtype=torch.float64))
    assert torch.equal(out.xy, (2.0 * torch.eye(L, dtype=torch.float64)).expand(2, L, L))
    assert abs(float(out.energy[1]) - (jz + (2.0 * w - 1.0) * hz)) <= 1e-13


def test_the_abi_refuses_before_any_device_work():
    lib = _lib.load()
    ERR_ARG, ERR_ALIGN = _lib.ERR_ARG, -2
    n, R = math.comb(10, 5), 8
    store = (ctypes.c_double * (6 * n * R + 4))()
    base = ctypes.addressof(store)
    base += -base % 16
    block = lambda i: c_void_p(base + 8 * n * R * i)  # noqa: E731
    X, U, V, ACC = block(0), block(1), block(2), block(3)                                # (ACC spans two blocks)
    odd = c_void_p(base + 8 * n * R * 5 + 8)
    M = 5
    coeffs = (ctypes.c_double * (2 * M))(*([0.5] * (2 * M)))
    flat = (ctypes.c_int32 * 2)(0, 1)
    h, other = c_void_p(), c_void_p()
    assert lib.dsea_op_create_sector(10, 5, 1, flat, X, X, X, X, byref(h)) == 0
    assert lib.dsea_op_create_pairsector(10, 5, X, X, X, X, byref(other)) == 0
    good = [h, R, 2, M, 0.25, 3.0, coeffs, X, U, V, ACC, None]

    def call(**change):
        args = list(good)
        for index, value in change.items():
            args[int(index[1:])] = value
        return lib.dsea_op_sector_block_chebyshev(*args)

    for handle in (other, None):
        assert call(a0=handle) == ERR_ARG
    for bad in (0, 3, 5, 16, -1):
        assert call(a1=bad) == ERR_ARG
    for bad in (0, 3, -1):
        assert call(a2=bad) == ERR_ARG
    for bad in (1, 0, -4):
        assert call(a3=bad) == ERR_ARG
    for slot in (6, 7, 8, 9, 10):
        assert call(**{"a%d" % slot: None}) == ERR_ARG
    for bad in (float("nan"), float("inf")):
        assert call(a4=bad) == ERR_ARG and call(a5=bad) == ERR_ARG
    assert call(a5=0.0) == ERR_ARG and call(a5=-1.0) == ERR_ARG
    assert call(a8=X) == ERR_ARG and call(a9=X) == ERR_ARG and call(a10=X) == ERR_ARG      # X among the written blocks
    assert call(a9=U) == ERR_ARG and call(a10=U) == ERR_ARG and call(a10=V) == ERR_ARG
    assert call(a7=block(4)) == ERR_ARG and call(a8=block(4)) == ERR_ARG                   # the second accumulator
    for slot in (7, 8, 9, 10):
        assert call(**{"a%d" % slot: odd}) == ERR_ALIGN
    assert lib.dsea_op_destroy(h) == 0 and lib.dsea_op_destroy(other) == 0
