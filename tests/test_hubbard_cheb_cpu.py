"""The Hubbard Chebyshev layer without a GPU (docs/design/34-hubbard-chebyshev.md): the numpy twin against dense linear algebra, the
product rule against the plain recurrence, ``coupling_bound`` of a Hubbard parameter vector, every refusal of the three new ABI
entries before any device work, their scratch sizes, and the host side of ``hubbard_density_of_states``.

Bar of the twin checks, per column j: max(1e-13, 10 x the twin's own float64-longdouble deviation) ||l_j|| ||x_j||, both measured
on the same inputs (docs/design/33-chebyshev-moments.md, section 6).
"""
import ctypes
import functools
import math
from ctypes import byref, c_int32, c_int64, c_void_p

import numpy as np
import pytest
import torch

import hubbard_cheb_reference as twin
import hubbard_reference as ref
from dominantsparseeigenad_amd import _lib, chebyshev, operators, thermal
from dominantsparseeigenad_amd.synthetic import normal_vector

F64 = torch.float64
LD = np.longdouble
CASES = {"L4-2-2": (4, 2, 2), "L6-3-3": (6, 3, 3)}
M = 64


def ring(L):
    return tuple((i, (i + 1) % L) for i in range(L))


@functools.lru_cache(maxsize=None)
def case(name):
    """(L, nup, ndn, bonds, couplings, X (n, 3), Y (n, 3), theta, V, the rigorous bounds) computed once and never written to"""
    L, nup, ndn = CASES[name]
    bonds = ring(L) + ((2, 0),)
    p = normal_vector(ref.nparam(L, bonds), 3400 + L).copy()
    n = math.comb(L, nup) * math.comb(L, ndn)
    X = np.stack([normal_vector(n, 3450 + L + j) for j in range(3)], axis=1)
    Y = np.stack([normal_vector(n, 3480 + L + j) for j in range(3)], axis=1)
    theta, V = np.linalg.eigh(ref.dense(L, nup, ndn, bonds, p))
    B = twin.coupling_bound(L, bonds, p)
    for a in (p, X, Y, theta, V):
        a.setflags(write=False)
    return L, nup, ndn, bonds, p, X, Y, theta, V, (-B, B)


def scaled(diff, left, X):
    """max over the orders of |diff[m, j]| / (||l_j|| ||x_j||), per column"""
    return np.abs(np.asarray(diff, dtype=np.float64)).max(axis=0) / (np.linalg.norm(left, axis=0) * np.linalg.norm(X, axis=0))


def test_the_cases_are_what_the_issue_names():
    assert case("L4-2-2")[5].shape[0] == 36 and case("L6-3-3")[5].shape[0] == 400


@pytest.mark.parametrize("mode", ["self", "left"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_twin_gives_the_dense_moments(name, mode):
    L, nup, ndn, bonds, p, X, Y, theta, V, bounds = case(name)
    assert bounds[0] <= theta[0] and theta[-1] <= bounds[1]
    left = None if mode == "self" else Y
    l = X if left is None else left
    got = twin.moments(L, nup, ndn, bonds, p, X, M, bounds, left)
    long = twin.moments(L, nup, ndn, bonds, p, X, M, bounds, left, dtype=LD)
    want = twin.dense_moments(theta, V, X, M, bounds, left)
    deviation = scaled((got - long).astype(np.float64), l, X)
    err = scaled(got - want, l, X)
    bar = np.maximum(1e-13, 10.0 * deviation)
    print("%s %s: worst |mu - dense| = %.2e, twin fp64 - longdouble %.2e (both / ||l|| ||x||), bar %.2e"
          % (name, mode, err.max(), deviation.max(), bar.min()))
    assert got.shape == (M, 3) and (err <= bar).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_twin_propagator_gives_the_dense_function(name):
    """e^{-tau (H - a)} X from the recurrence against the eigendecomposition, within 1e-13 per order (the bar of note 31)"""
    L, nup, ndn, bonds, p, X, _, theta, V, bounds = case(name)
    h = 0.5 * (bounds[1] - bounds[0])
    x = 0.3 * h
    order = twin.cheb.exp_order(x)
    coeffs = twin.cheb.coefficients(twin.cheb.exp_function(x), order)
    got = twin.chebyshev_apply(L, nup, ndn, bonds, p, X, coeffs, bounds)
    want = V @ (np.exp(-0.3 * (theta - bounds[0]))[:, None] * (V.T @ X))
    assert np.linalg.norm(got - want) <= 1e-13 * order * np.linalg.norm(X)


@pytest.mark.parametrize("count", [2, 3, 4, 5, 64])
@pytest.mark.parametrize("name", sorted(CASES))
def test_doubling_gives_the_moments_of_the_plain_recurrence(name, count):
    """ceil(M / 2) orders with the product rule against M - 1 orders of <x| T_m x>, in the same twin"""
    L, nup, ndn, bonds, p, X, _, _, _, bounds = case(name)
    got = twin.moments(L, nup, ndn, bonds, p, X, count, bounds)
    want = twin.plain_moments(L, nup, ndn, bonds, p, X, count, bounds)
    long = twin.plain_moments(L, nup, ndn, bonds, p, X, count, bounds, dtype=LD)
    deviation = np.maximum(scaled((want - long).astype(np.float64), X, X), scaled((got - long).astype(np.float64), X, X))
    assert got.shape == want.shape == (count, 3)
    assert (scaled(got - want, X, X) <= np.maximum(1e-13, 10.0 * deviation)).all()
    assert np.array_equal(got[:2], want[:2])                                       # order 1 is the same arithmetic


def bare_operator(L, bonds, p):
    """a ``HubbardOperator`` with what ``coupling_bound`` reads and nothing on a device"""
    op = object.__new__(operators.HubbardOperator)
    op.N, op.nb, op.nparam = L, len(bonds), 2 * len(bonds) + 2 * L
    op._c = torch.from_numpy(np.array(p))
    return op


@pytest.mark.parametrize("name", sorted(CASES))
def test_coupling_bound_of_a_hubbard_operator(name):
    L, nup, ndn, bonds, p, _, _, theta, _, _ = case(name)
    got = chebyshev.coupling_bound(bare_operator(L, bonds, p))
    want = twin.coupling_bound(L, bonds, p)
    assert got is not None and abs(got - want) <= 1e-14 * want
    assert got >= max(abs(theta[0]), abs(theta[-1]))
    assert chebyshev.coupling_bound(object()) is None
    # one family at a time: the weights 2, 4, 1, 2
    nb = len(bonds)
    for first, last, weight in ((0, nb, 2.0), (nb, 2 * nb, 4.0), (2 * nb, 2 * nb + L, 1.0), (2 * nb + L, 2 * nb + 2 * L, 2.0)):
        q = np.zeros_like(p)
        q[first:last] = -1.5
        assert chebyshev.coupling_bound(bare_operator(L, bonds, q)) == weight * 1.5 * (last - first)


def host_blocks(n, R, count):
    store = (ctypes.c_double * (count * n * R + 4))()
    base = ctypes.addressof(store)
    base += -base % 16
    return store, [c_void_p(base + 8 * n * R * i) for i in range(count)], c_void_p(base + 8 * n * R * (count - 1) + 8)


def handles(lib, A):
    flat = (c_int32 * 2)(0, 1)
    h, other = c_void_p(), c_void_p()
    assert lib.dsea_op_create_hubbard(8, 4, 4, 1, flat, A, A, A, A, A, A, A, byref(h)) == 0
    assert lib.dsea_op_create_sector(10, 5, 1, flat, A, A, A, A, byref(other)) == 0
    return h, other


def test_the_propagator_entry_refuses_before_any_device_work():
    lib = _lib.load()
    ERR_ARG, ERR_ALIGN = _lib.ERR_ARG, -2
    n, R = 70 * 70, 8
    store, blocks, odd = host_blocks(n, R, 6)
    X, U, V, ACC = blocks[:4]                                                            # (ACC spans two blocks)
    count = 5
    coeffs = (ctypes.c_double * (2 * count))(*([0.5] * (2 * count)))
    h, other = handles(lib, X)
    good = [h, R, 2, count, 0.25, 3.0, coeffs, X, U, V, ACC, None]

    def call(**change):
        args = list(good)
        for index, value in change.items():
            args[int(index[1:])] = value
        return lib.dsea_op_hubbard_block_chebyshev(*args)

    for handle in (other, None):
        assert call(a0=handle) == ERR_ARG
    assert lib.dsea_op_sector_block_chebyshev(*good) == ERR_ARG                             # and the spin entry refuses this kind
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
    assert call(a7=blocks[4]) == ERR_ARG and call(a8=blocks[4]) == ERR_ARG                 # the second accumulator
    for slot in (7, 8, 9, 10):
        assert call(**{"a%d" % slot: odd}) == ERR_ALIGN
    assert lib.dsea_op_destroy(h) == 0 and lib.dsea_op_destroy(other) == 0


def test_the_moments_entry_refuses_before_any_device_work():
    lib = _lib.load()
    ERR_ARG, ERR_ALIGN = _lib.ERR_ARG, -2
    n, R = 70 * 70, 8
    store, blocks, odd = host_blocks(n, R, 6)
    X, Y, U, V, MU, scratch = blocks
    h, other = handles(lib, X)
    good = [h, R, 5, 0.25, 3.0, X, Y, U, V, MU, scratch, None]

    def call(**change):
        args = list(good)
        for index, value in change.items():
            args[int(index[1:])] = value
        return lib.dsea_op_hubbard_block_moments(*args)

    for handle in (other, None):
        assert call(a0=handle) == ERR_ARG
    assert lib.dsea_op_sector_block_moments(*good) == ERR_ARG
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
    """2 R min(4096, ceil(n / 256)) doubles"""
    lib = _lib.load()
    need = c_int64()
    for L, nup, ndn, R in ((4, 2, 1, 8), (6, 3, 3, 1), (8, 4, 4, 2), (10, 5, 5, 8), (16, 8, 8, 4), (40, 2, 1, 8)):
        n = math.comb(L, nup) * math.comb(L, ndn)
        assert lib.dsea_op_hubbard_block_moments_scratch_doubles(L, nup, ndn, R, byref(need)) == 0
        assert need.value == 2 * R * min(4096, (n + 255) // 256), (L, nup, ndn, R)
    assert math.comb(16, 8) ** 2 > 4096 * 256                                            # the largest grid, whatever the cap
    for bad in ((8, 4, 4, 3), (8, 4, 4, 0), (8, 9, 4, 8), (8, 4, 0, 8), (1, 1, 1, 8), (41, 2, 2, 8)):
        assert lib.dsea_op_hubbard_block_moments_scratch_doubles(*bad, byref(need)) == _lib.ERR_ARG, bad
    assert lib.dsea_op_hubbard_block_moments_scratch_doubles(8, 4, 4, 8, None) == _lib.ERR_ARG


def no_device(*args, **kwargs):
    raise AssertionError("the device was touched")


def test_density_of_states_argument_errors(monkeypatch):
    monkeypatch.setattr(operators, "HubbardOperator", no_device)
    bonds = ring(4)
    good = torch.ones(2 * 4 + 2 * 4, dtype=F64)
    dos = thermal.hubbard_density_of_states
    for bad_M in (1, 0, -3):
        with pytest.raises(ValueError):
            dos(4, bonds, good, bad_M)
    with pytest.raises(ValueError):
        dos(4, bonds, good, 16, R=0)
    with pytest.raises(ValueError):
        dos(1, ((0, 1),), good, 16)                                                       # L out of range
    with pytest.raises(ValueError):
        dos(4, bonds, torch.zeros(3, dtype=F64), 16)                                      # wrong parameter length
    with pytest.raises(ValueError):
        dos(4, ((0, 4),), torch.zeros(10, dtype=F64), 16)                                 # a bad bond
    with pytest.raises(ValueError):
        dos(4, bonds, good, 16, sectors=[(2, 5)])                                         # a sector out of range
    with pytest.raises(ValueError):
        dos(4, bonds, good, 16, sectors=[(-1, 2)])
    with pytest.raises(ValueError):
        dos(4, bonds, good, 16, sectors=[(1, 2), (2, 1), (1, 2)])                         # a repeated sector
    with pytest.raises(ValueError):
        dos(4, bonds, good, 16, sectors=[])
    with pytest.raises(ValueError, match=r"\(0, 2\).*edge_dense_max"):
        dos(4, bonds, good, 16, sectors=[(2, 2), (0, 2)], edge_dense_max=5)
    for bad in ((1.0, 1.0), (2.0, -2.0), (0.0, float("inf")), (1.0,), "ab"):
        with pytest.raises(ValueError):
            dos(4, bonds, good, 16, sectors=[(0, 2)], bounds=bad)
    with pytest.raises(ValueError):
        dos(4, bonds, torch.zeros(16, dtype=F64), 16, sectors=[(0, 2)])                   # B = 0: no default interval
    with pytest.raises(ValueError, match="do not hold the spectrum"):
        dos(4, bonds, good, 16, sectors=[(0, 2)], bounds=(-0.1, 0.1))


def test_an_edge_only_sector_list_needs_no_device(monkeypatch):
    monkeypatch.setattr(operators, "HubbardOperator", no_device)
    L, count = 4, 24
    bonds = ring(L) + ((2, 0),)
    p = normal_vector(ref.nparam(L, bonds), 3490).copy()
    sectors = [(0, 0), (0, 2), (2, 0), (4, 1), (3, 4), (4, 4), (0, 4), (4, 0)]
    got = thermal.hubbard_density_of_states(L, bonds, torch.from_numpy(p), count, sectors=sectors)
    B = twin.coupling_bound(L, bonds, p)
    assert isinstance(got, chebyshev.ChebyshevMeasure) and len(got) == count
    assert got.bounds[0] == -got.bounds[1] and abs(got.bounds[1] - B) <= 1e-14 * B
    theta = np.concatenate([np.linalg.eigvalsh(ref.dense(L, a, b, bonds, p)) for a, b in sectors])
    states = sum(math.comb(L, a) * math.comb(L, b) for a, b in sectors)
    assert theta.size == states == 1 + 6 + 6 + 4 + 4 + 1 + 1 + 1
    want = twin.spectrum_moments(theta, count, got.bounds)
    assert np.abs(got.moments.numpy() - want).max() <= 1e-12 * states and abs(float(got.moments[0]) - states) <= 1e-12 * states
    assert np.abs(got.moments.numpy() - twin.hubbard_moments(L, bonds, p, count, sectors=sectors)).max() <= 1e-12 * states
    off = thermal.hubbard_density_of_states(L, bonds, torch.from_numpy(p), count, sectors=sectors, spin_symmetric=False)
    assert np.abs(off.moments.numpy() - want).max() <= 1e-12 * states
    narrow = thermal.hubbard_density_of_states(L, bonds, torch.from_numpy(p), count, sectors=sectors,
                                               bounds=(theta.min() - 0.5, theta.max() + 0.5))
    assert narrow.bounds == (theta.min() - 0.5, theta.max() + 0.5)
    assert np.abs(narrow.moments.numpy() - twin.spectrum_moments(theta, count, narrow.bounds)).max() <= 1e-12 * states


def test_the_density_of_states_is_exported_under_the_package_name():
    import dominantsparseeigenad_amd as pkg
    assert pkg.hubbard_density_of_states is thermal.hubbard_density_of_states
