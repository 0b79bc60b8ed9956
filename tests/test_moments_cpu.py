"""The Chebyshev moments without a GPU (docs/design/33-chebyshev-moments.md): the numpy twin against dense linear algebra, the
product rule against the plain recurrence, the damping kernels and ``ChebyshevMeasure`` of the package, and every argument error
that must be raised before any device work.

Bar of the twin checks, per column j: max(1e-13, 10 x the twin's own float64-longdouble deviation) ||l_j|| ||x_j||, both measured
on the same inputs (the rule of docs/design/31-chebyshev-propagator.md, section 6).
"""
import ctypes
import functools
import math
from ctypes import byref, c_int64, c_void_p

import numpy as np
import pytest
import torch

import lattice_reference
import sector_moments_reference as twin
import sector_reference as ref
from dominantsparseeigenad_amd import _lib, chebyshev, spectral, thermal
from dominantsparseeigenad_amd.operators import ring_bonds
from dominantsparseeigenad_amd.synthetic import normal_vector

LD = np.longdouble
CASES = {"L8-4": (8, 4, tuple(lattice_reference.random_bonds(8, 12, 3108))), "L6-3": (6, 3, tuple(ring_bonds(6)))}
M = 64


@functools.lru_cache(maxsize=None)
def case(name):
    """(L, ndown, bonds, couplings, X (n, 3), Y (n, 3), theta, V, bounds) computed once and never written to"""
    L, ndown, bonds = CASES[name]
    p = normal_vector(ref.nparam(L, bonds), 3700 + L).copy()
    n = math.comb(L, ndown)
    X = np.stack([normal_vector(n, 3750 + L + j) for j in range(3)], axis=1)
    Y = np.stack([normal_vector(n, 3780 + L + j) for j in range(3)], axis=1)
    theta, V = np.linalg.eigh(ref.dense(L, ndown, bonds, p))
    spread = theta[-1] - theta[0]
    bounds = (theta[0] - 0.05 * spread, theta[-1] + 0.05 * spread)
    for a in (p, X, Y, theta, V):
        a.setflags(write=False)
    return L, ndown, bonds, p, X, Y, theta, V, bounds


def scaled(diff, left, X):
    """max over the orders of |diff[m, j]| / (||l_j|| ||x_j||), per column"""
    return np.abs(np.asarray(diff, dtype=np.float64)).max(axis=0) / (np.linalg.norm(left, axis=0) * np.linalg.norm(X, axis=0))


@pytest.mark.parametrize("mode", ["self", "left"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_twin_gives_the_dense_moments(name, mode):
    L, ndown, bonds, p, X, Y, theta, V, bounds = case(name)
    left = None if mode == "self" else Y
    l = X if left is None else left
    got = twin.moments(L, ndown, bonds, p, X, M, bounds, left)
    long = twin.moments(L, ndown, bonds, p, X, M, bounds, left, dtype=LD)
    want = twin.dense_moments(theta, V, X, M, bounds, left)
    deviation = scaled((got - long).astype(np.float64), l, X)
    err = scaled(got - want, l, X)
    bar = np.maximum(1e-13, 10.0 * deviation)
    print("%s %s: worst |mu - dense| = %.2e, twin fp64 - longdouble %.2e (both / ||l|| ||x||), bar %.2e"
          % (name, mode, err.max(), deviation.max(), bar.min()))
    assert got.shape == (M, 3) and (err <= bar).all()


@pytest.mark.parametrize("count", [2, 3, 4, 5, 64])
@pytest.mark.parametrize("name", sorted(CASES))
def test_doubling_gives_the_moments_of_the_plain_recurrence(name, count):
    """ceil(M / 2) orders with the product rule against M - 1 orders of <x| T_m x>, in the same twin"""
    L, ndown, bonds, p, X, _, _, _, bounds = case(name)
    apply = lambda x: twin.blockref.apply_block(L, ndown, bonds, p, x)  # noqa: E731
    got = twin.recurrence_moments(apply, X, count, bounds)
    want = twin.plain_moments(apply, X, count, bounds)
    long = twin.plain_moments(lambda x: twin.blockref.apply_block(L, ndown, bonds, p, x, LD), X, count, bounds, dtype=LD)
    deviation = np.maximum(scaled((want - long).astype(np.float64), X, X), scaled((got - long).astype(np.float64), X, X))
    assert got.shape == want.shape == (count, 3)
    assert (scaled(got - want, X, X) <= np.maximum(1e-13, 10.0 * deviation)).all()
    assert np.array_equal(got[:2], want[:2])                                       # order 1 is the same arithmetic


@pytest.mark.parametrize("count", [1, 2, 7, 64, 255])
def test_the_jackson_kernel(count):
    g = chebyshev.jackson_kernel(count)
    assert g.dtype == np.float64 and g.shape == (count,) and g[0] == 1.0
    assert (g > 0).all() and (g <= 1).all() and (np.diff(g) < 0).all()
    assert np.abs(g - twin.jackson(count)).max() <= 4e-16
    lz = chebyshev.lorentz_kernel(count, 3.0)
    assert lz[0] == 1.0 and (lz > 0).all() and (np.diff(lz) < 0).all() and np.abs(lz - twin.lorentz(count, 3.0)).max() <= 4e-16


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_jackson_density_is_positive_and_integrates_to_mu0(name):
    _, _, _, _, X, _, theta, V, bounds = case(name)
    mu = twin.dense_moments(theta, V, X[:, :1], M, bounds)[:, 0]                   # a positive measure: <x| . |x>
    measure = chebyshev.ChebyshevMeasure(mu, bounds)
    centre, h = 0.5 * (bounds[0] + bounds[1]), 0.5 * (bounds[1] - bounds[0])
    grid = np.linspace(bounds[0], bounds[1], 2001)
    rho = measure.density(grid).numpy()
    assert rho.shape == grid.shape and rho[0] == 0.0 and rho[-1] == 0.0             # the ends are not strictly inside
    assert rho.min() >= -1e-12 * mu[0] / h
    assert np.abs(rho - twin.density(mu, bounds, grid, twin.jackson(M))).max() <= 1e-12 * mu[0] / h
    assert float(measure.density(bounds[1] + 1.0)) == 0.0 and measure.density(torch.zeros((2, 3))).shape == (2, 3)
    # Chebyshev-Gauss: int f(s) / sqrt(1 - s^2) ds = (pi / N) sum_k f(cos theta_k), exact for polynomials of degree < 2 N
    N = 2 * M
    s = np.cos(math.pi * (np.arange(N) + 0.5) / N)
    for kernel in ("jackson", "lorentz", None, np.linspace(1.0, 0.5, M)):
        rho = measure.density(centre + h * s, kernel).numpy()
        total = (math.pi / N) * float((rho * h * np.sqrt(1.0 - s * s)).sum())
        assert abs(total - mu[0]) <= 1e-12 * mu[0], kernel
    undamped = measure.density(grid[1:-1], None).numpy()
    assert np.abs(undamped - twin.density(mu, bounds, grid[1:-1])).max() <= 1e-11 * mu[0] / h / np.sqrt(1 - 0.999 ** 2)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_trace_of_the_exponential(name):
    _, _, _, _, X, _, theta, V, bounds = case(name)
    mu = twin.dense_moments(theta, V, X[:, :1], M, bounds)[:, 0]
    measure = chebyshev.ChebyshevMeasure(mu, bounds)
    weights = (V.T @ X[:, 0]) ** 2
    h = 0.5 * (bounds[1] - bounds[0])
    for beta in (0.0, 0.3 / h, 5.0 / h):
        assert chebyshev.exp_order(beta * h) <= M
        f = lambda E: np.exp(-LD(beta) * (E - LD(bounds[0])))  # noqa: E731
        want = float((weights * np.exp(-beta * (theta - bounds[0]))).sum())
        got = measure.trace(f)
        assert abs(got - want) <= 1e-12 * mu[0] and abs(got - twin.trace(mu, bounds, f)) <= 1e-13 * mu[0]
        logw = math.log(want) - beta * bounds[0]
        bar = 2e-12 * mu[0] / want                                                      # (the bar of the sum, as a relative error)
        assert abs(measure.logtrace_exp(beta) - logw) <= bar and abs(twin.logtrace_exp(mu, bounds, beta) - logw) <= bar
    assert abs(measure.trace(lambda E: E) - float((weights * theta).sum())) <= 1e-12 * mu[0] * max(abs(bounds[0]), abs(bounds[1]))


def test_measures_shift_and_add():
    a = chebyshev.ChebyshevMeasure([2.0, 0.5, -0.25], (-1.0, 3.0))
    b = chebyshev.ChebyshevMeasure(torch.tensor([1.0, 0.0, 0.25]), (-1.0, 3.0))
    assert len(a) == 3 and a.bounds == (-1.0, 3.0) and a.moments.dtype == torch.float64
    total = a + b
    assert total.bounds == a.bounds and torch.equal(total.moments, torch.tensor([3.0, 0.5, 0.0], dtype=torch.float64))
    moved = a.shifted(1.5)
    assert moved.bounds == (-2.5, 1.5) and torch.equal(moved.moments, a.moments)
    E = torch.linspace(-0.9, 2.9, 7, dtype=torch.float64)
    assert torch.equal(moved.density(E - 1.5), a.density(E))
    assert "3 moments" in repr(a)


class _NoOperator:
    n, device = 4, "cpu"


def test_host_side_argument_errors():
    op = _NoOperator()
    X = torch.zeros((4, 2), dtype=torch.float64)
    good = chebyshev.ChebyshevMeasure([1.0, 0.5, 0.25], (-1.0, 1.0))

    class _WithBlock(_NoOperator):
        def apply_block(self, X):
            return X

    for call in (lambda: chebyshev.chebyshev_moments(op, X, 8, (-1.0, 1.0), fused=True),      # no fused kernel for this kind
                 lambda: chebyshev.chebyshev_moments(op, X, 8, (-1.0, 1.0)),                  # nothing with apply_block
                 lambda: chebyshev.chebyshev_moments(_WithBlock(), X, 8, (-1.0, 1.0), fused=True),
                 lambda: chebyshev.chebyshev_moments(_WithBlock(), X, 8, (-1.0, 1.0)),        # a block that is not on the device
                 lambda: chebyshev.chebyshev_moments(_WithBlock(), X, 1, (-1.0, 1.0)),        # M < 2
                 lambda: chebyshev.chebyshev_moments(_WithBlock(), X, 8, (1.0, 1.0)),         # empty interval
                 lambda: chebyshev.chebyshev_moments(_WithBlock(), X, 8, (-1.0, float("nan"))),
                 lambda: chebyshev.chebyshev_moments(_WithBlock(), X[:, 0], 8, (-1.0, 1.0)),  # not a block
                 lambda: chebyshev.jackson_kernel(0),
                 lambda: chebyshev.lorentz_kernel(0),
                 lambda: chebyshev.lorentz_kernel(4, 0.0),
                 lambda: chebyshev.lorentz_kernel(4, float("inf")),
                 lambda: chebyshev.ChebyshevMeasure([], (-1.0, 1.0)),
                 lambda: chebyshev.ChebyshevMeasure([1.0, float("nan")], (-1.0, 1.0)),
                 lambda: chebyshev.ChebyshevMeasure([1.0, 0.5], (1.0, -1.0)),
                 lambda: chebyshev.ChebyshevMeasure([1.0, 0.5], (0.0,)),
                 lambda: good.density([0.0], "gauss"),
                 lambda: good.density([0.0], [1.0, 0.5]),                                     # factors of another length
                 lambda: good.density([0.0], [1.0, 0.5, float("nan")]),
                 lambda: good.logtrace_exp(-1.0),
                 lambda: good.logtrace_exp(float("inf")),
                 lambda: chebyshev.ChebyshevMeasure([0.0, 0.0], (-1.0, 1.0)).logtrace_exp(1.0),  # an empty measure has no logarithm
                 lambda: good + chebyshev.ChebyshevMeasure([1.0, 0.5, 0.25], (-1.0, 2.0)),
                 lambda: good + chebyshev.ChebyshevMeasure([1.0, 0.5], (-1.0, 1.0)),
                 lambda: spectral.kpm_measure(op, X, 8, (-1.0, 1.0)),                         # a block, not a vector
                 lambda: spectral.kpm_measure(op, [0.0] * 4, 8, (-1.0, 1.0)),
                 lambda: spectral.kpm_measure(op, X[:, 0], 8, (-1.0, 1.0)),                   # nothing with apply_block
                 lambda: spectral.kpm_measure(op, X[:, 0], 8),                                # no bounds for this kind
                 lambda: thermal.sector_density_of_states(op, 8, (-1.0, 1.0))):               # not a sector operator
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        good + 1.0
    bonds = ring_bonds(6)
    c = torch.zeros(2 * 6 + 6, dtype=torch.float64)
    for call in (lambda: thermal.spin_density_of_states(6, bonds, c[:-1], 8),
                 lambda: thermal.spin_density_of_states(6, bonds, c, 1),
                 lambda: thermal.spin_density_of_states(6, bonds, c, 8, sectors=[1, 1]),
                 lambda: thermal.spin_density_of_states(6, bonds, c, 8, sectors=[7]),
                 lambda: thermal.spin_density_of_states(6, bonds, c, 8, sectors=[0]),         # all couplings 0: B = 0, no interval
                 lambda: thermal.spin_density_of_states(6, bonds, c + 1.0, 8, sectors=[0], bounds=(-1.0, 1.0))):  # E outside
        with pytest.raises(ValueError):
            call()


def test_the_edge_sectors_need_no_device():
    """ndown = 0 and ndown = L alone: T_m of two energies on (-B, B) from host arithmetic"""
    L, bonds = 6, ring_bonds(6)
    p = normal_vector(2 * 6 + 6, 3790)
    out = thermal.spin_density_of_states(L, bonds, torch.from_numpy(p.copy()), 16, sectors=[0, L])
    B = 2.0 * np.abs(p[:6]).sum() + np.abs(p[6:]).sum()
    assert out.bounds[0] == -out.bounds[1] and abs(out.bounds[1] - B) <= 4e-16 * B      # (two orders of summing |c|)
    assert len(out) == 16 and float(out.moments[0]) == 2.0
    jz, hz = p[6:12].sum(), p[12:].sum()
    want = twin.spectrum_moments([jz + hz, jz - hz], 16, out.bounds)
    assert np.abs(out.moments.numpy() - want).max() <= 1e-13


def test_the_abi_refuses_before_any_device_work():
    lib = _lib.load()
    ERR_ARG, ERR_ALIGN = _lib.ERR_ARG, -2
    n, R = math.comb(10, 5), 8
    store = (ctypes.c_double * (6 * n * R + 4))()
    base = ctypes.addressof(store)
    base += -base % 16
    block = lambda i: c_void_p(base + 8 * n * R * i)  # noqa: E731
    X, Y, U, V, MU, scratch = (block(i) for i in range(6))
    odd = c_void_p(base + 8 * n * R * 5 + 8)
    flat = (ctypes.c_int32 * 2)(0, 1)
    h, other = c_void_p(), c_void_p()
    assert lib.dsea_op_create_sector(10, 5, 1, flat, X, X, X, X, byref(h)) == 0
    assert lib.dsea_op_create_pairsector(10, 5, X, X, X, X, byref(other)) == 0
    good = [h, R, 5, 0.25, 3.0, X, Y, U, V, MU, scratch, None]

    def call(**change):
        args = list(good)
        for index, value in change.items():
            args[int(index[1:])] = value
        return lib.dsea_op_sector_block_moments(*args)

    for handle in (other, None):
        assert call(a0=handle) == ERR_ARG
    for bad in (0, 3, 5, 16, -1):
        assert call(a1=bad) == ERR_ARG
    for bad in (1, 0, -4):
        assert call(a2=bad) == ERR_ARG
    for slot in (5, 7, 8, 9, 10):                                                        # (a null Y, slot 6, is self mode)
        assert call(**{"a%d" % slot: None}) == ERR_ARG
        assert call(**{"a%d" % slot: None, "a6": None}) == ERR_ARG
    for bad in (float("nan"), float("inf")):
        assert call(a3=bad) == ERR_ARG and call(a4=bad) == ERR_ARG
    assert call(a4=0.0) == ERR_ARG and call(a4=-1.0) == ERR_ARG
    assert call(a6=X) == ERR_ARG and call(a7=X) == ERR_ARG and call(a8=X) == ERR_ARG          # any two of X, Y, U, V
    assert call(a7=Y) == ERR_ARG and call(a8=Y) == ERR_ARG and call(a8=U) == ERR_ARG
    assert call(a6=None, a7=X) == ERR_ARG and call(a6=None, a8=X) == ERR_ARG and call(a6=None, a8=U) == ERR_ARG
    for slot in (5, 6, 7, 8):
        assert call(**{"a%d" % slot: odd}) == ERR_ALIGN
    assert lib.dsea_op_destroy(h) == 0 and lib.dsea_op_destroy(other) == 0


def test_the_scratch_sizes():
    lib = _lib.load()
    need = c_int64()
    assert lib.dsea_op_sector_block_moments_scratch_doubles(10, 5, 8, byref(need)) == 0 and need.value == 2 * 8 * 1
    assert lib.dsea_op_sector_block_moments_scratch_doubles(24, 12, 4, byref(need)) == 0
    assert math.comb(24, 12) > 4096 * 256 and need.value == 2 * 4 * 4096                 # the largest grid, whatever the cap
    assert lib.dsea_op_sector_block_moments_scratch_doubles(16, 8, 1, byref(need)) == 0 and need.value == 2 * ((12870 + 255) // 256)
    for bad in ((10, 5, 3), (10, 11, 8), (1, 0, 8)):
        assert lib.dsea_op_sector_block_moments_scratch_doubles(*bad, byref(need)) == _lib.ERR_ARG
    assert lib.dsea_op_sector_block_moments_scratch_doubles(10, 5, 8, None) == _lib.ERR_ARG
