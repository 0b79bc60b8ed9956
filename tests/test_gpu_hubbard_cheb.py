"""k_cheb_hubbard_block, k_cheb_hubbard_moments and the layers on them on the GPU (docs/design/34-hubbard-chebyshev.md), at the
geometries of tests/test_gpu_hubbard.py that reach each way the new tail and the reductions can go wrong:

    L4-2-1           n = 24: one partial block, n_dn below a wave       L8-4-4-complete  n = 4900, 28 bonds
    L6-3-3-loops     n = 400 = 256 + 144, a ragged last block;          L10-5-5-walk     n = 63 504, grid capped at 2^6: a block
                     10 bonds, no multiple of a chunk                                    accumulates over four row ranges
    L7-3-2-split     n = 735, 4 bonds: fewer than a chunk at R <= 4     L40-2-1          n = 31 200, state words wider than 32 bits

Random couplings, the rigorous bounds (-B, B) of the coupling bound.  The propagator and the work blocks of the moments must hold
the BITS of the unfused path (``apply_block`` and torch elementwise operations); moments are compared within max(1e-13, 10 x the
twin's float64-longdouble deviation on the same inputs) ||l_j|| ||x_j|| per column.  The longdouble twin runs at the four smaller
geometries; the two larger ones take the widest deviation measured at L8-4-4-complete.
"""
import functools
import importlib.util
import math
import os
from ctypes import byref, c_double, c_int64, c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hubbard_cheb_reference as twin  # noqa: E402
import hubbard_reference as ref  # noqa: E402
import test_gpu_hubbard as base  # noqa: E402
from test_gpu_hubbard import GEOMETRY, couplings  # noqa: E402
from dominantsparseeigenad_amd import _lib, chebyshev, engine, spectral, thermal  # noqa: E402
from dominantsparseeigenad_amd.operators import HubbardOperator, SpinSectorOperator, hubbard_dim, ring_bonds  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402

F64 = torch.float64
LD = np.longdouble
NAMES = ["L4-2-1", "L6-3-3-loops", "L7-3-2-split", "L8-4-4-complete", "L10-5-5-walk", "L40-2-1"]
SMALL = NAMES[:4]
WIDTHS = [1, 2, 4, 8]
ORDERS = [2, 3, 12]             # the propagator: 1, 2 and 11 launches (first; x = U, old = X; old == out in turn)
COUNTS = [2, 3, 4, 5, 40]       # self mode: 1, 2, 2, 3, 20 orders (a row past M - 1 at 3 and 5); left mode: 1, 2, 3, 4, 39
MODES = ["self", "left"]
ERR_ARG, ERR_ALIGN = -1, -2
WORST = {}


def to_dev(a):
    return base.to_dev(a)


@functools.lru_cache(maxsize=None)
def case(name):
    """(couplings, X (n, C), Y (n, C), the rigorous bounds (-B, B)) on the host, C = 13 at L6-3-3-loops and 8 elsewhere, computed
    once and never written to"""
    L, nup, ndn, _, bonds = GEOMETRY[name]
    p = couplings(L, bonds, "random")
    n = hubbard_dim(L, nup, ndn)
    C = 13 if name == "L6-3-3-loops" else 8
    X = np.stack([normal_vector(n, 34000 + 20 * L + j) for j in range(C)], axis=1)
    Y = np.stack([normal_vector(n, 34500 + 20 * L + j) for j in range(C)], axis=1)
    B = twin.coupling_bound(L, bonds, p)
    for a in (X, Y):
        a.setflags(write=False)
    return p, X, Y, (-B, B)


def operator(name):
    return base.operator(name, case(name)[0])


def random_coefficients(A, M, seed=34100):
    return normal_vector(A * M, seed + 50 * A + M).reshape(A, M).copy()


def relnorm(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


@functools.lru_cache(maxsize=None)
def twin_propagator(name, M):
    """the float64 twin's two accumulators (2, n, 8) for ``random_coefficients(2, M)``; row 0 alone serves A = 1 through
    ``random_coefficients(1, M)`` in ``twin_propagator_one``"""
    L, nup, ndn, _, bonds = GEOMETRY[name]
    p, X, _, bounds = case(name)
    return twin.chebyshev_apply(L, nup, ndn, bonds, p, X[:, :8], random_coefficients(2, M), bounds)


@functools.lru_cache(maxsize=None)
def twin_propagator_one(name, M):
    L, nup, ndn, _, bonds = GEOMETRY[name]
    p, X, _, bounds = case(name)
    return twin.chebyshev_apply(L, nup, ndn, bonds, p, X[:, :8], random_coefficients(1, M), bounds)


@functools.lru_cache(maxsize=None)
def twin_case(name, mode):
    """(mu float64 [40, C], deviation [C], scale [C]) of the twin on all C columns: the moments of a shorter run and of fewer
    columns are its leading rows and columns; deviation is |float64 - longdouble| / (||l|| ||x||) where the longdouble twin runs,
    and the widest of L8-4-4-complete in this mode at the two larger geometries"""
    L, nup, ndn, _, bonds = GEOMETRY[name]
    p, X, Y, bounds = case(name)
    left = None if mode == "self" else Y
    mu = twin.moments(L, nup, ndn, bonds, p, X, COUNTS[-1], bounds, left)
    scale = np.linalg.norm(X if left is None else left, axis=0) * np.linalg.norm(X, axis=0)
    if name in SMALL:
        long = twin.moments(L, nup, ndn, bonds, p, X, COUNTS[-1], bounds, left, dtype=LD)
        deviation = np.abs((mu - long).astype(np.float64)).max(axis=0) / scale
    else:
        deviation = np.full(X.shape[1], twin_case("L8-4-4-complete", mode)[1].max())
    mu.setflags(write=False)
    return mu, deviation, scale


def run_propagator(op, X, coeffs, bounds):
    """dsea_op_hubbard_block_chebyshev on device blocks: (ACC [A, n, R], U, V)"""
    lib = _lib.load()
    A, M = coeffs.shape
    n, R = X.shape
    U, V = torch.full_like(X, float("nan")), torch.full_like(X, float("nan"))
    acc = torch.full((A, n, R), float("nan"), dtype=F64, device=X.device)
    host = (c_double * (A * M))(*coeffs.reshape(-1).tolist())
    ptr = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    status = lib.dsea_op_hubbard_block_chebyshev(op.handle, R, A, M, 0.5 * (bounds[0] + bounds[1]), 0.5 * (bounds[1] - bounds[0]),
                                                 host, ptr(X), ptr(U), ptr(V), ptr(acc), engine._stream(X.device))
    assert status == 0, status
    return acc, U, V


def run_moments(op, X, Y, M, bounds):
    """dsea_op_hubbard_block_moments on device blocks: (mu on the host [M, R], U, V)"""
    lib = _lib.load()
    n, R = X.shape
    U, V = torch.full_like(X, float("nan")), torch.full_like(X, float("nan"))
    mu = torch.full((M, R), float("nan"), dtype=F64, device=X.device)
    need = c_int64()
    assert lib.dsea_op_hubbard_block_moments_scratch_doubles(op.N, op.nup, op.ndn, R, byref(need)) == 0
    scratch = torch.full((need.value,), float("nan"), dtype=F64, device=X.device)
    ptr = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    status = lib.dsea_op_hubbard_block_moments(op.handle, R, M, 0.5 * (bounds[0] + bounds[1]), 0.5 * (bounds[1] - bounds[0]), ptr(X),
                                               None if Y is None else ptr(Y), ptr(U), ptr(V), ptr(mu), ptr(scratch),
                                               engine._stream(X.device))
    assert status == 0, status
    return mu.cpu(), U, V


def test_the_geometries_are_what_the_table_says():
    sizes = {name: hubbard_dim(*GEOMETRY[name][:3]) for name in NAMES}
    assert sizes == {"L4-2-1": 24, "L6-3-3-loops": 400, "L7-3-2-split": 735, "L8-4-4-complete": 4900, "L10-5-5-walk": 63504,
                     "L40-2-1": 31200}
    assert len(GEOMETRY["L6-3-3-loops"][4]) == 10 and len(GEOMETRY["L7-3-2-split"][4]) == 4
    assert len(GEOMETRY["L8-4-4-complete"][4]) == 28
    assert GEOMETRY["L10-5-5-walk"][3] == 6 and (63504 + 255) // 256 > 3 * 64        # a block walks four row ranges
    assert GEOMETRY["L4-2-1"][0] == 4 and math.comb(4, 1) < 64


@pytest.mark.parametrize("A", [1, 2])
@pytest.mark.parametrize("R", WIDTHS)
@pytest.mark.parametrize("name", NAMES)
def test_the_propagator_entry_returns_the_bits_of_the_unfused_path(name, R, A):
    _, X, _, bounds = case(name)
    op = operator(name)
    Xd = to_dev(X[:, :R])
    for M in ORDERS:
        c = random_coefficients(A, M)
        got, U, V = run_propagator(op, Xd, c, bounds)
        want = chebyshev.chebyshev_apply(op, Xd, c, bounds, fused=False)
        assert want.shape == (A, op.n, R) and torch.equal(got, want), (name, R, A, M)
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
        again, U2, V2 = run_propagator(op, Xd, c, bounds)
        assert torch.equal(again, got) and torch.equal(U2, U) and (M == 2 or torch.equal(V2, V))   # a repeated call: identical bits
        if M == 2:
            assert bool(torch.isnan(V).all())                                                    # one order: V is not touched
        assert torch.equal(chebyshev.chebyshev_apply(op, Xd, c, bounds), got)                    # None reaches this kernel
        if name in SMALL:
            ref64 = (twin_propagator(name, M) if A == 2 else twin_propagator_one(name, M))[:, :, :R]
            worst = max(relnorm(got[a].cpu().numpy(), ref64[a]) for a in range(A))
            print("%s R = %d A = %d M = %d: against the float64 twin %.2e (bar %.1e)" % (name, R, A, M, worst, 1e-13 * M))
            assert worst <= 1e-13 * M
    assert torch.equal(Xd, to_dev(X[:, :R]))                                                     # X is not written


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("R", WIDTHS)
@pytest.mark.parametrize("name", NAMES)
def test_the_moments_entry_leaves_the_bits_of_the_propagator_in_the_work_blocks(name, R, mode):
    """the contract on return: T_K X in U for odd K, in V for even K, equal to ``chebyshev_apply`` with the coefficient row e_K"""
    _, X, Y, bounds = case(name)
    op = operator(name)
    Xd = to_dev(X[:, :R])
    Yd = to_dev(Y[:, :R]) if mode == "left" else None
    want_mu, deviation, scale = twin_case(name, mode)
    for M in COUNTS:
        K = M - 1 if mode == "left" else (M + 1) // 2
        mu, U, V = run_moments(op, Xd, Yd, M, bounds)
        e = np.zeros(K + 1)
        e[K] = 1.0
        assert torch.equal(U if K % 2 else V, chebyshev.chebyshev_apply(op, Xd, e, bounds)), (name, R, mode, M)
        if K >= 2:
            e = np.zeros(K + 1)
            e[K - 1] = 1.0
            assert torch.equal(V if K % 2 else U, chebyshev.chebyshev_apply(op, Xd, e, bounds)), (name, R, mode, M)
        else:
            assert bool(torch.isnan(V).all())                                                   # one order: V is not touched
        assert mu.shape == (M, R) and bool(torch.isfinite(mu).all())                            # every row below M is written
        again, _, _ = run_moments(op, Xd, Yd, M, bounds)
        assert torch.equal(again, mu), (name, R, mode, M)                                       # a repeated call: identical bits
        err = np.abs(mu.numpy() - want_mu[:M, :R]).max(axis=0) / scale[:R]
        assert (err <= np.maximum(1e-13, 10.0 * deviation[:R])).all(), (name, R, mode, M, err)
    assert torch.equal(Xd, to_dev(X[:, :R])) and (Yd is None or torch.equal(Yd, to_dev(Y[:, :R])))   # X and Y are not written


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,R", [(name, R) for name in NAMES for R in WIDTHS] + [("L6-3-3-loops", 3), ("L6-3-3-loops", 13)])
def test_fused_and_unfused_against_the_float64_twin(name, R, mode):
    """R = 3 and 13 go through the host split"""
    _, X, Y, bounds = case(name)
    op = operator(name)
    Xd = to_dev(X[:, :R])
    Yd = to_dev(Y[:, :R]) if mode == "left" else None
    want, deviation, scale = twin_case(name, mode)
    bar = np.maximum(1e-13, 10.0 * deviation[:R])
    for M in COUNTS:
        fused = chebyshev.chebyshev_moments(op, Xd, M, bounds, left=Yd)                          # None: the Hubbard kernel
        unfused = chebyshev.chebyshev_moments(op, Xd, M, bounds, left=Yd, fused=False)
        assert fused.shape == unfused.shape == (M, R) and fused.dtype == F64 and not fused.is_cuda
        errs = [np.abs(a - b).max(axis=0) / scale[:R] for a, b in ((fused.numpy(), want[:M, :R]), (unfused.numpy(), want[:M, :R]),
                                                                   (fused.numpy(), unfused.numpy()))]
        key = "%s %s" % (name, mode)
        WORST[key] = max(WORST.get(key, 0.0), *(float(e.max()) for e in errs))
        print("%s R = %d M = %d: fused - twin %.2e, unfused - twin %.2e, fused - unfused %.2e, twin deviation %.2e (/ ||l|| ||x||)"
              % (key, R, M, errs[0].max(), errs[1].max(), errs[2].max(), deviation[:R].max()))
        for e in errs:
            assert (e <= bar).all(), (name, R, mode, M, e)
    if R in WIDTHS:                                                                              # the fused path is the C entry
        assert torch.equal(fused, run_moments(op, Xd, Yd, COUNTS[-1], bounds)[0])
    assert torch.equal(Xd, to_dev(X[:, :R]))


@pytest.mark.parametrize("R", [3, 13])
def test_other_widths_of_the_propagator_go_through_the_host_split(R):
    _, X, _, bounds = case("L6-3-3-loops")
    op = operator("L6-3-3-loops")
    Xd = to_dev(X[:, :R])
    for M in (4, 40):
        c = random_coefficients(2, M)
        got = chebyshev.chebyshev_apply(op, Xd, c, bounds)
        assert got.shape == (2, op.n, R)
        assert torch.equal(got, chebyshev.chebyshev_apply(op, Xd, c, bounds, fused=False))
    three = random_coefficients(3, 12)                                                           # three rows: no kernel, the torch path
    assert torch.equal(chebyshev.chebyshev_apply(op, Xd, three, bounds), chebyshev.chebyshev_apply(op, Xd, three, bounds, fused=False))
    assert torch.equal(Xd, to_dev(X[:, :R]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["L6-3-3-loops", "L10-5-5-walk"])
def test_a_column_of_a_wide_block_is_the_one_column_call_bit_for_bit(name, mode):
    """every column has its own accumulators, the same rows per thread and the same order of the partial sums at every width"""
    _, X, Y, bounds = case(name)
    op = operator(name)
    Xd, Yd = to_dev(X[:, :8]), to_dev(Y[:, :8])
    wide = chebyshev.chebyshev_moments(op, Xd, 40, bounds, left=Yd if mode == "left" else None)
    for j in range(8):
        single = chebyshev.chebyshev_moments(op, Xd[:, j:j + 1], 40, bounds, left=Yd[:, j:j + 1] if mode == "left" else None)
        assert torch.equal(single[:, 0], wide[:, j]), (name, mode, j)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["L4-2-1", "L6-3-3-loops", "L10-5-5-walk"])
def test_a_zero_column_has_zero_moments_and_leaves_the_others_alone(name, mode):
    _, X, Y, bounds = case(name)
    op = operator(name)
    Xd, Yd = to_dev(X[:, :8]), (to_dev(Y[:, :8]) if mode == "left" else None)
    full = chebyshev.chebyshev_moments(op, Xd, 40, bounds, left=Yd)
    Xz = Xd.clone()
    Xz[:, 5] = 0.0
    got = chebyshev.chebyshev_moments(op, Xz, 40, bounds, left=Yd)
    assert not bool(got[:, 5].any())
    keep = [0, 1, 2, 3, 4, 6, 7]
    assert torch.equal(got[:, keep], full[:, keep])


@pytest.mark.parametrize("name", NAMES)
def test_left_mode_on_the_block_itself_is_self_mode(name):
    _, X, _, bounds = case(name)
    op = operator(name)
    _, deviation, scale = twin_case(name, "self")
    Xd = to_dev(X[:, :8])
    for M in (5, 40):
        own = chebyshev.chebyshev_moments(op, Xd, M, bounds)
        left = chebyshev.chebyshev_moments(op, Xd, M, bounds, left=Xd.clone())
        assert torch.equal(own[:2], left[:2])                                                   # order 1 is the same arithmetic
        err = (own - left).abs().max(dim=0).values.numpy() / scale[:8]
        assert (err <= np.maximum(1e-13, 10.0 * deviation[:8])).all(), (name, M, err)


@functools.lru_cache(maxsize=None)
def dense_case(name):
    """(L, nup, ndn, bonds, couplings, X (n, 3), Y (n, 3), theta, V, bounds) of L6-3-3-loops, or of the ring L = 4 (2, 2)"""
    if name == "L4-2-2":
        L, nup, ndn, bonds = 4, 2, 2, tuple(ring_bonds(4))
        p = normal_vector(ref.nparam(L, bonds), 34200).copy()
        n = 36
        X = np.stack([normal_vector(n, 34210 + j) for j in range(4)], axis=1)
        Y = np.stack([normal_vector(n, 34220 + j) for j in range(4)], axis=1)
        B = twin.coupling_bound(L, bonds, p)
        bounds = (-B, B)
    else:
        L, nup, ndn, _, bonds = GEOMETRY[name]
        p, X, Y, bounds = case(name)
    theta, V = np.linalg.eigh(ref.dense(L, nup, ndn, bonds, p))
    return L, nup, ndn, bonds, p, X[:, :4], Y[:, :4], theta, V, bounds


def dense_operator(name):
    L, nup, ndn, bonds, p = dense_case(name)[:5]
    return HubbardOperator(L, bonds, to_dev(p), nup, ndn)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["L4-2-2", "L6-3-3-loops"])
def test_fused_moments_against_dense_eigh(name, mode):
    L, nup, ndn, bonds, p, X, Y, theta, V, bounds = dense_case(name)
    X, Y = X[:, :3], Y[:, :3]
    assert bounds[0] <= theta[0] and theta[-1] <= bounds[1]
    op = dense_operator(name)
    left = Y if mode == "left" else None
    got = chebyshev.chebyshev_moments(op, to_dev(X), 64, bounds, left=None if left is None else to_dev(Y)).numpy()
    want = twin.dense_moments(theta, V, X, 64, bounds, left)
    t64 = twin.moments(L, nup, ndn, bonds, p, X, 64, bounds, left)
    tld = twin.moments(L, nup, ndn, bonds, p, X, 64, bounds, left, dtype=LD)
    scale = np.linalg.norm(X if left is None else left, axis=0) * np.linalg.norm(X, axis=0)
    deviation = np.abs((t64 - tld).astype(np.float64)).max(axis=0) / scale
    err = np.abs(got - want).max(axis=0) / scale
    print("%s %s: |mu - dense| = %.2e, twin fp64 - longdouble %.2e (/ ||l|| ||x||)" % (name, mode, err.max(), deviation.max()))
    assert (err <= np.maximum(1e-13, 10.0 * deviation)).all()


def test_kpm_measure_of_a_hubbard_column():
    L, nup, ndn, bonds, p, X, _, theta, V, bounds = dense_case("L6-3-3-loops")
    op = dense_operator("L6-3-3-loops")
    block = chebyshev.chebyshev_moments(op, to_dev(X[:, :1]), 64, bounds)
    measure = spectral.kpm_measure(op, to_dev(X[:, 0]), 64, bounds)
    assert measure.bounds == bounds and torch.equal(measure.moments, block[:, 0])               # the same one-column launch
    want = twin.dense_moments(theta, V, X[:, :1], 64, bounds)[:, 0]
    t64 = twin.moments(L, nup, ndn, bonds, p, X[:, :1], 64, bounds)[:, 0]
    tld = twin.moments(L, nup, ndn, bonds, p, X[:, :1], 64, bounds, dtype=LD)[:, 0]
    norm2 = float(np.linalg.norm(X[:, 0]) ** 2)
    bar = max(1e-13, 10.0 * float(np.abs((t64 - tld).astype(np.float64)).max()) / norm2) * norm2
    assert np.abs(measure.moments.numpy() - want).max() <= bar
    auto = spectral.kpm_measure(op, to_dev(X[:, 0]), 16)                                        # bounds = None: spectral_bounds(op)
    a, b = chebyshev.spectral_bounds(op)
    B = bounds[1]
    assert auto.bounds == (a, b) and -B <= a <= theta[0] and theta[-1] <= b <= B                # cut to the coupling bound


@pytest.mark.parametrize("tau_h", [0.5, 5.0, 40.0])
def test_expm_block_against_dense_eigh(tau_h):
    L, nup, ndn, bonds, p, X, _, theta, V, bounds = dense_case("L6-3-3-loops")
    X = X[:, :3]
    op = dense_operator("L6-3-3-loops")
    h = 0.5 * (bounds[1] - bounds[0])
    tau = tau_h / h
    Y, shift = chebyshev.expm_block(op, to_dev(X), tau, bounds)
    assert shift == bounds[0] and Y.shape == X.shape
    orders = chebyshev.exp_order(tau * h)
    want = V @ (np.exp(-tau * (theta - shift))[:, None] * (V.T @ X))
    err = float(np.linalg.norm(Y.cpu().numpy() - want))
    bar = 1e-13 * orders * np.linalg.norm(X)
    print("L6-3-3-loops tau h = %g: |Y - dense| = %.2e, %d orders, bar %.2e" % (tau_h, err, orders, bar))
    assert err <= bar
    _, coeffs = chebyshev._truncated_expansion(lambda s: np.exp(-LD(tau * h) * (s + LD(1))), chebyshev._order_guess(tau * h), 1e-15)
    assert torch.equal(Y, chebyshev.chebyshev_apply(op, to_dev(X), coeffs, bounds, fused=False))  # the kernel's bits


@pytest.mark.parametrize("ht", [0.5, 5.0, 40.0])
def test_time_evolve_against_dense_eigh(ht):
    L, nup, ndn, bonds, p, X, _, theta, V, bounds = dense_case("L6-3-3-loops")
    op = dense_operator("L6-3-3-loops")
    h = 0.5 * (bounds[1] - bounds[0])
    t = ht / h
    psi = X[:, 0:2] + 1j * X[:, 2:4]
    got = chebyshev.time_evolve(op, to_dev(psi), t, bounds)
    assert got.dtype == torch.complex128 and got.shape == psi.shape
    want = V @ (np.exp(-1j * t * theta)[:, None] * (V.T @ psi))
    orders = twin.cheb.evolution_coefficients(t, bounds).shape[1]
    err = float(np.linalg.norm(got.cpu().numpy() - want))
    bar = 1e-13 * orders * np.linalg.norm(psi)
    norms = np.abs(np.linalg.norm(got.cpu().numpy(), axis=0) - np.linalg.norm(psi, axis=0)).max()
    print("L6-3-3-loops h t = %g: |psi(t) - dense| = %.2e, norm change %.2e, %d orders, bar %.2e" % (ht, err, norms, orders, bar))
    assert err <= bar and norms <= bar
    re = chebyshev.time_evolve(op, to_dev(X[:, 0:2]), t, bounds)
    im = chebyshev.time_evolve(op, to_dev(X[:, 2:4]), t, bounds)
    assert torch.equal(got, torch.complex(re.real - im.imag, re.imag + im.real))


def thermal_model(seed):
    L = 4
    bonds = tuple(ring_bonds(L)) + ((2, 0),)
    return L, bonds, normal_vector(ref.nparam(L, bonds), seed).copy()


def test_hubbard_density_of_states_with_every_sector_exact():
    L, bonds, p = thermal_model(34300)
    M = 64
    got = thermal.hubbard_density_of_states(L, bonds, to_dev(p), M)
    B = twin.coupling_bound(L, bonds, p)
    assert abs(got.bounds[1] - B) <= 1e-14 * B and got.bounds[0] == -got.bounds[1] and len(got) == M
    theta = np.concatenate([np.linalg.eigvalsh(ref.dense(L, a, b, bonds, p)) for a in range(L + 1) for b in range(L + 1)])
    assert theta.size == 4 ** L
    worst = float(np.abs(got.moments.numpy() - twin.spectrum_moments(theta, M, got.bounds)).max())
    print("hubbard_density_of_states L = 4, every sector exact: worst moment deviation %.2e (bar %.2e)" % (worst, 1e-10 * 4 ** L))
    assert worst <= 1e-10 * 4 ** L and abs(float(got.moments[0]) - 256.0) <= 1e-10 * 256


def test_hubbard_density_of_states_with_every_bulk_sector_sampled_against_the_twin():
    L, bonds, p = thermal_model(34310)
    M, R, seed = 64, 4, 7
    got = thermal.hubbard_density_of_states(L, bonds, to_dev(p), M, R=R, seed=seed, dense_below=0)
    want = twin.hubbard_moments(L, bonds, p, M, R=R, seed=seed, dense_below=0, bounds=got.bounds)
    worst = float(np.abs(got.moments.numpy() - want).max())
    print("hubbard_density_of_states L = 4, every bulk sector sampled, R = 4: worst deviation from the twin %.2e (bar %.2e)"
          % (worst, 1e-10 * 4 ** L))
    assert worst <= 1e-10 * 4 ** L and abs(float(got.moments[0]) - 256.0) <= 1e-10 * 256
    off = thermal.hubbard_density_of_states(L, bonds, to_dev(p), M, R=R, seed=seed, dense_below=0, spin_symmetric=False)
    both = twin.hubbard_moments(L, bonds, p, M, R=R, seed=seed, dense_below=0, spin_symmetric=False, bounds=got.bounds)
    assert float(np.abs(off.moments.numpy() - both).max()) <= 1e-10 * 4 ** L


def test_the_abi_refuses_what_the_header_says():
    lib = _lib.load()
    name = "L8-4-4-complete"
    _, X, Y, bounds = case(name)
    op = operator(name)
    n = op.n
    Xd, Yd = to_dev(X), to_dev(Y)
    U, V = torch.zeros_like(Xd), torch.zeros_like(Xd)
    acc = torch.zeros((2, n, 8), dtype=F64, device=Xd.device)
    mu = torch.zeros((5, 8), dtype=F64, device=Xd.device)
    scratch = torch.zeros(2 * 8 * ((n + 255) // 256), dtype=F64, device=Xd.device)
    st = engine._stream(Xd.device)
    ptr = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    host = (c_double * 10)(*([0.5] * 10))
    spin = SpinSectorOperator(8, ring_bonds(8), torch.zeros(2 * 8 + 8, dtype=F64, device=Xd.device), 4)
    odd = torch.empty(n * 8 + 1, dtype=F64, device=Xd.device)[1:]
    assert odd.data_ptr() % 16 == 8
    prop = [op.handle, 8, 2, 5, 0.0, bounds[1], host, ptr(Xd), ptr(U), ptr(V), ptr(acc), st]
    mom = [op.handle, 8, 5, 0.0, bounds[1], ptr(Xd), ptr(Yd), ptr(U), ptr(V), ptr(mu), ptr(scratch), st]

    def call(entry, good, **change):
        args = list(good)
        for index, value in change.items():
            args[int(index[1:])] = value
        return entry(*args)

    cheb_entry, mom_entry = lib.dsea_op_hubbard_block_chebyshev, lib.dsea_op_hubbard_block_moments
    assert call(cheb_entry, prop, a0=spin.handle) == ERR_ARG and call(mom_entry, mom, a0=spin.handle) == ERR_ARG   # OP_SECTOR
    assert lib.dsea_op_sector_block_chebyshev(*prop) == ERR_ARG and lib.dsea_op_sector_block_moments(*mom) == ERR_ARG
    for slot in (7, 8, 9, 10):
        assert call(cheb_entry, prop, **{"a%d" % slot: ptr(odd)}) == ERR_ALIGN
    for slot in (5, 6, 7, 8):
        assert call(mom_entry, mom, **{"a%d" % slot: ptr(odd)}) == ERR_ALIGN
    assert call(cheb_entry, prop, a8=ptr(Xd)) == ERR_ARG and call(cheb_entry, prop, a9=ptr(U)) == ERR_ARG
    assert call(cheb_entry, prop, a10=ptr(V)) == ERR_ARG and call(cheb_entry, prop, a7=ptr(acc[1])) == ERR_ARG
    assert call(mom_entry, mom, a6=ptr(Xd)) == ERR_ARG and call(mom_entry, mom, a7=ptr(Yd)) == ERR_ARG
    assert call(mom_entry, mom, a8=ptr(U)) == ERR_ARG and call(mom_entry, mom, a6=None, a8=ptr(Xd)) == ERR_ARG
    torch.cuda.synchronize()
    assert not bool(U.any()) and not bool(V.any()) and not bool(acc.any()) and not bool(mu.any())   # nothing refused has run
    assert cheb_entry(*prop) == 0 and mom_entry(*mom) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(mu).all()) and float(mu.abs().max()) > 0
    with pytest.raises(ValueError):                                                              # True names the spin entry
        chebyshev.chebyshev_moments(op, Xd, 5, bounds, fused=True)
    with pytest.raises(ValueError):
        chebyshev.chebyshev_apply(op, Xd, [0.5, 0.5], bounds, fused=True)


def test_the_example_runs_and_its_density_integrates_to_the_dimension():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "hubbard", "density_of_states.py")
    spec = importlib.util.spec_from_file_location("hubbard_density_of_states_example", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = ex.main(L=6, nup=3, ndn=3, moments=32)
    assert out["n"] == 400 and out["M"] == 32
    assert abs(out["integral"] - 400.0) <= 1e-10 * 400 and abs(out["mu0"] - 400.0) <= 1e-10 * 400


def test_the_worst_deviations_of_this_run():
    """(printed for docs/design/34-hubbard-chebyshev.md; runs after the comparisons above)"""
    for key in sorted(WORST):
        print("worst of fused, unfused and twin, %s: %.2e ||l|| ||x||" % (key, WORST[key]))
