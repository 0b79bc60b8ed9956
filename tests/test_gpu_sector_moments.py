"""k_cheb_sector_moments, k_cheb_moments_finish and the layers on them on the GPU (docs/design/33-chebyshev-moments.md).

    L8-4         n = 70: one partial block, tail threads   L16-8        n = 12 870: many blocks
    L11-5-ring   n = 462 = 256 + 206, 11 bonds: chunks     L18-9-walk   n = 48 620, grid capped at 2^6: a block accumulates
                 8 + 3 and 4 + 4 + 3                                    over three row ranges
    L8-4-short   3 bonds: fewer than one chunk

All with random Jxy, Jz and non-zero hz (the geometries and inputs of tests/test_gpu_sector_cheb.py).  The work blocks must hold
the BITS of the propagator's; moments are compared within max(1e-13, 10 x the twin's float64-longdouble deviation on the same
inputs) ||l_j|| ||x_j|| per column.
"""
import functools
import importlib.util
import math
import os
from ctypes import byref, c_int64, c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hubbard_reference  # noqa: E402
import lattice_reference  # noqa: E402
import sector_block_reference as blockref  # noqa: E402
import sector_moments_reference as twin  # noqa: E402
import sector_reference as ref  # noqa: E402
from dominantsparseeigenad_amd import _lib, chebyshev, engine, spectral, thermal  # noqa: E402
from dominantsparseeigenad_amd.operators import HubbardOperator, SpinSectorOperator, ring_bonds, ring_momentum_weights  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402

F64 = torch.float64
LD = np.longdouble
GEOMETRY = {
    "L8-4": (8, 4, None, tuple(lattice_reference.random_bonds(8, 12, 3108))),
    "L11-5-ring": (11, 5, None, tuple(ring_bonds(11))),
    "L8-4-short": (8, 4, None, ((0, 5), (2, 3), (7, 1))),
    "L16-8": (16, 8, None, tuple(lattice_reference.random_bonds(16, 24, 3116))),
    "L18-9-walk": (18, 9, 6, tuple(lattice_reference.random_bonds(18, 20, 3118))),
}
NAMES = sorted(GEOMETRY)
COUNTS = [2, 3, 4, 5, 40]       # self mode: 1, 2, 2, 3, 20 orders (a row past M - 1 at 3 and 5); left mode: 1, 2, 3, 4, 39
MODES = ["self", "left"]
WORST = {}


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


def to_dev(a):
    return torch.from_numpy(np.array(a)).to(dev())


@functools.lru_cache(maxsize=None)
def case(name):
    """(couplings, X (n, 13), Y (n, 13), the rigorous bounds (-B, B)) on the host, computed once and never written to"""
    L, ndown, _, bonds = GEOMETRY[name]
    p = normal_vector(ref.nparam(L, bonds), 3200 + L + len(bonds)).copy()
    assert np.abs(p).min() > 0
    n = math.comb(L, ndown)
    X = np.stack([normal_vector(n, 3300 + 20 * L + j) for j in range(13)], axis=1)
    Y = np.stack([normal_vector(n, 3800 + 20 * L + j) for j in range(13)], axis=1)
    B = blockref.coupling_bound(L, bonds, p)
    for a in (p, X, Y):
        a.setflags(write=False)
    return p, X, Y, (-B, B)


def operator(name):
    L, ndown, grid, bonds = GEOMETRY[name]
    op = SpinSectorOperator(L, bonds, to_dev(case(name)[0]), ndown)
    if grid is not None:
        op.set_grid_log2(grid)
    return op


@functools.lru_cache(maxsize=None)
def twin_case(name, mode):
    """(mu float64 [40, C], deviation [C]) of the twin on the first C columns (13 on the ring, 8 elsewhere): the moments of a
    shorter run and of fewer columns are its leading rows and columns; deviation is float64 - longdouble / (||l|| ||x||)"""
    L, ndown, _, bonds = GEOMETRY[name]
    p, X, Y, bounds = case(name)
    C = 13 if name == "L11-5-ring" else 8
    left = None if mode == "self" else Y[:, :C]
    mu = twin.moments(L, ndown, bonds, p, X[:, :C], COUNTS[-1], bounds, left)
    long = twin.moments(L, ndown, bonds, p, X[:, :C], COUNTS[-1], bounds, left, dtype=LD)
    scale = np.linalg.norm(X[:, :C] if left is None else left, axis=0) * np.linalg.norm(X[:, :C], axis=0)
    deviation = np.abs((mu - long).astype(np.float64)).max(axis=0) / scale
    mu.setflags(write=False)
    return mu, deviation, scale


def run_entry(op, X, Y, M, bounds):
    """dsea_op_sector_block_moments on device blocks: (mu on the host [M, R], U, V)"""
    lib = _lib.load()
    n, R = X.shape
    U, V = torch.full_like(X, float("nan")), torch.full_like(X, float("nan"))
    mu = torch.full((M, R), float("nan"), dtype=F64, device=X.device)
    need = c_int64()
    assert lib.dsea_op_sector_block_moments_scratch_doubles(op.N, op.ndown, R, byref(need)) == 0
    scratch = torch.full((need.value,), float("nan"), dtype=F64, device=X.device)
    ptr = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    status = lib.dsea_op_sector_block_moments(op.handle, R, M, 0.5 * (bounds[0] + bounds[1]), 0.5 * (bounds[1] - bounds[0]), ptr(X),
                                              None if Y is None else ptr(Y), ptr(U), ptr(V), ptr(mu), ptr(scratch),
                                              engine._stream(X.device))
    assert status == 0, status
    return mu.cpu(), U, V


def test_the_geometries_are_what_the_table_says():
    sizes = {name: math.comb(g[0], g[1]) for name, g in GEOMETRY.items()}
    assert sizes == {"L8-4": 70, "L11-5-ring": 462, "L8-4-short": 70, "L16-8": 12870, "L18-9-walk": 48620}
    assert len(GEOMETRY["L11-5-ring"][3]) == 11 and len(GEOMETRY["L8-4-short"][3]) == 3
    assert (48620 + 255) // 256 > 2 * 64                       # capped at 2^6 blocks, a block walks three row ranges


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("R", [1, 2, 4, 8])
@pytest.mark.parametrize("name", NAMES)
def test_the_entry_leaves_the_bits_of_the_propagator_in_the_work_blocks(name, R, mode):
    """the contract on return: T_K X in U for odd K, in V for even K, equal to ``chebyshev_apply`` with the coefficient row e_K"""
    _, X, Y, bounds = case(name)
    op = operator(name)
    Xd = to_dev(X[:, :R])
    Yd = to_dev(Y[:, :R]) if mode == "left" else None
    want_mu, deviation, scale = twin_case(name, mode)
    for M in COUNTS:
        K = M - 1 if mode == "left" else (M + 1) // 2
        mu, U, V = run_entry(op, Xd, Yd, M, bounds)
        e = np.zeros(K + 1)
        e[K] = 1.0
        last = chebyshev.chebyshev_apply(op, Xd, e, bounds, fused=True)
        assert torch.equal(U if K % 2 else V, last), (name, R, mode, M)
        if K >= 2:
            e = np.zeros(K + 1)
            e[K - 1] = 1.0
            assert torch.equal(V if K % 2 else U, chebyshev.chebyshev_apply(op, Xd, e, bounds, fused=True)), (name, R, mode, M)
        else:
            assert bool(torch.isnan(V).all())                                                   # one order: V is not touched
        assert mu.shape == (M, R) and bool(torch.isfinite(mu).all())                            # every row below M is written
        again, _, _ = run_entry(op, Xd, Yd, M, bounds)
        assert torch.equal(again, mu), (name, R, mode, M)                                       # a repeated call: identical bits
        err = np.abs(mu.numpy() - want_mu[:M, :R]).max(axis=0) / scale[:R]
        assert (err <= np.maximum(1e-13, 10.0 * deviation[:R])).all(), (name, R, mode, M, err)
    assert torch.equal(Xd, to_dev(X[:, :R])) and (Yd is None or torch.equal(Yd, to_dev(Y[:, :R])))   # X and Y are not written


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,R", [(name, R) for name in NAMES for R in (1, 2, 4, 8)] + [("L11-5-ring", 3), ("L11-5-ring", 13)])
def test_fused_and_unfused_against_the_float64_twin(name, R, mode):
    """R = 3 and 13 go through the host split"""
    _, X, Y, bounds = case(name)
    op = operator(name)
    Xd = to_dev(X[:, :R])
    Yd = to_dev(Y[:, :R]) if mode == "left" else None
    want, deviation, scale = twin_case(name, mode)
    bar = np.maximum(1e-13, 10.0 * deviation[:R])
    for M in COUNTS:
        fused = chebyshev.chebyshev_moments(op, Xd, M, bounds, left=Yd, fused=True)
        unfused = chebyshev.chebyshev_moments(op, Xd, M, bounds, left=Yd, fused=False)
        assert fused.shape == unfused.shape == (M, R) and fused.dtype == F64 and not fused.is_cuda
        assert torch.equal(chebyshev.chebyshev_moments(op, Xd, M, bounds, left=Yd), fused)       # the default is the fused path
        errs = [np.abs(a - b).max(axis=0) / scale[:R] for a, b in ((fused.numpy(), want[:M, :R]), (unfused.numpy(), want[:M, :R]),
                                                                   (fused.numpy(), unfused.numpy()))]
        key = "%s %s" % (name, mode)
        WORST[key] = max(WORST.get(key, 0.0), *(float(e.max()) for e in errs))
        print("%s R = %d M = %d: fused - twin %.2e, unfused - twin %.2e, fused - unfused %.2e, twin deviation %.2e (/ ||l|| ||x||)"
              % (key, R, M, errs[0].max(), errs[1].max(), errs[2].max(), deviation[:R].max()))
        for e in errs:
            assert (e <= bar).all(), (name, R, mode, M, e)
    assert torch.equal(Xd, to_dev(X[:, :R]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["L11-5-ring", "L18-9-walk"])
def test_a_column_of_a_wide_block_against_the_one_column_call(name, mode):
    _, X, Y, bounds = case(name)
    op = operator(name)
    _, deviation, scale = twin_case(name, mode)
    Xd, Yd = to_dev(X[:, :8]), to_dev(Y[:, :8])
    wide = chebyshev.chebyshev_moments(op, Xd, 40, bounds, left=Yd if mode == "left" else None, fused=True)
    same = True
    for j in range(8):
        single = chebyshev.chebyshev_moments(op, Xd[:, j:j + 1], 40, bounds, left=Yd[:, j:j + 1] if mode == "left" else None,
                                             fused=True)
        same = same and torch.equal(single[:, 0], wide[:, j])
        err = float((single[:, 0] - wide[:, j]).abs().max()) / scale[j]
        assert err <= max(1e-13, 10.0 * deviation[j]), (name, mode, j, err)
    print("%s %s: the columns of the R = 8 call %s the R = 1 calls bit for bit" % (name, mode, "equal" if same else "DO NOT equal"))


@functools.lru_cache(maxsize=None)
def dense_case(name):
    L, ndown, _, bonds = GEOMETRY[name]
    return np.linalg.eigh(ref.dense(L, ndown, bonds, case(name)[0]))


@pytest.mark.parametrize("which", ["spectral", "rigorous"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["L8-4", "L11-5-ring"])
def test_fused_moments_against_dense_eigh(name, mode, which):
    L, ndown, _, bonds = GEOMETRY[name]
    p, X, Y, rigorous = case(name)
    X, Y = X[:, :3], Y[:, :3]
    theta, V = dense_case(name)
    op = operator(name)
    bounds = chebyshev.spectral_bounds(op) if which == "spectral" else rigorous
    assert bounds[0] <= theta[0] and theta[-1] <= bounds[1]
    left = Y if mode == "left" else None
    got = chebyshev.chebyshev_moments(op, to_dev(X), 64, bounds, left=None if left is None else to_dev(Y), fused=True).numpy()
    want = twin.dense_moments(theta, V, X, 64, bounds, left)
    t64 = twin.moments(L, ndown, bonds, p, X, 64, bounds, left)
    tld = twin.moments(L, ndown, bonds, p, X, 64, bounds, left, dtype=LD)
    scale = np.linalg.norm(X if left is None else left, axis=0) * np.linalg.norm(X, axis=0)
    deviation = np.abs((t64 - tld).astype(np.float64)).max(axis=0) / scale
    err = np.abs(got - want).max(axis=0) / scale
    print("%s %s %s bounds: |mu - dense| = %.2e, twin fp64 - longdouble %.2e (/ ||l|| ||x||)" % (name, mode, which, err.max(), deviation.max()))
    assert (err <= np.maximum(1e-13, 10.0 * deviation)).all()


@pytest.mark.parametrize("name", NAMES)
def test_left_mode_on_the_block_itself_is_self_mode(name):
    _, X, _, bounds = case(name)
    op = operator(name)
    _, deviation, scale = twin_case(name, "self")
    Xd = to_dev(X[:, :8])
    for M in (5, 40):
        own = chebyshev.chebyshev_moments(op, Xd, M, bounds, fused=True)
        left = chebyshev.chebyshev_moments(op, Xd, M, bounds, left=Xd.clone(), fused=True)
        assert torch.equal(own[:2], left[:2])                                                   # order 1 is the same arithmetic
        err = (own - left).abs().max(dim=0).values.numpy() / scale[:8]
        assert (err <= np.maximum(1e-13, 10.0 * deviation[:8])).all(), (name, M, err)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["L8-4", "L11-5-ring", "L18-9-walk"])
def test_a_zero_column_has_zero_moments_and_leaves_the_others_alone(name, mode):
    _, X, Y, bounds = case(name)
    op = operator(name)
    Xd, Yd = to_dev(X[:, :8]), (to_dev(Y[:, :8]) if mode == "left" else None)
    full = chebyshev.chebyshev_moments(op, Xd, 40, bounds, left=Yd, fused=True)
    Xz = Xd.clone()
    Xz[:, 5] = 0.0
    got = chebyshev.chebyshev_moments(op, Xz, 40, bounds, left=Yd, fused=True)
    assert not bool(got[:, 5].any())
    keep = [0, 1, 2, 3, 4, 6, 7]
    assert torch.equal(got[:, keep], full[:, keep])


def test_moments_on_the_hubbard_operator_run_unfused():
    L, nup, ndn = 4, 2, 2
    bonds = tuple(ring_bonds(L))
    p = normal_vector(hubbard_reference.nparam(L, bonds), 3500).copy()
    op = HubbardOperator(L, bonds, to_dev(p), nup, ndn)
    n = op.n
    assert n == 36
    X = np.stack([normal_vector(n, 3510 + j) for j in range(3)], axis=1)
    theta, V = np.linalg.eigh(hubbard_reference.dense(L, nup, ndn, bonds, p))
    bounds = chebyshev.spectral_bounds(op)
    assert bounds[0] <= theta[0] and theta[-1] <= bounds[1]
    got = chebyshev.chebyshev_moments(op, to_dev(X), 64, bounds).numpy()                        # None: no fused entry for this kind
    err = np.abs(got - twin.dense_moments(theta, V, X, 64, bounds)).max(axis=0) / np.linalg.norm(X, axis=0) ** 2
    print("Hubbard L4 (2, 2): |mu - dense| = %.2e ||x||^2 (bar 1e-13)" % err.max())
    assert (err <= 1e-13).all()
    with pytest.raises(ValueError):
        chebyshev.chebyshev_moments(op, to_dev(X), 64, bounds, fused=True)
    measure = spectral.kpm_measure(op, to_dev(X[:, 0]), 64)                                     # (one column: other column sums)
    assert measure.bounds == bounds and np.abs(measure.moments.numpy() - got[:, 0]).max() <= 1e-13 * np.linalg.norm(X[:, 0]) ** 2


def thermal_model(L, seed):
    bonds = tuple(ring_bonds(L)) + ((0, L // 2), (1, L // 2 + 1))
    return bonds, normal_vector(ref.nparam(L, bonds), seed).copy()


def test_spin_density_of_states_with_every_sector_exact():
    L, M = 8, 64
    bonds, p = thermal_model(L, 3600)
    got = thermal.spin_density_of_states(L, bonds, to_dev(p), M)
    B = blockref.coupling_bound(L, bonds, p)
    assert abs(got.bounds[1] - B) <= 1e-14 * B and got.bounds[0] == -got.bounds[1] and len(got) == M
    theta = np.concatenate([np.linalg.eigvalsh(ref.dense(L, nd, bonds, p)) for nd in range(1, L)]
                           + [[blockref.edge_energy(L, bonds, p, 0)], [blockref.edge_energy(L, bonds, p, L)]])
    assert theta.size == 2 ** L
    worst = float(np.abs(got.moments.numpy() - twin.spectrum_moments(theta, M, got.bounds)).max())
    print("spin_density_of_states L = 8, every sector exact: worst moment deviation %.2e (bar %.2e)" % (worst, 1e-10 * 2 ** L))
    assert worst <= 1e-10 * 2 ** L and abs(float(got.moments[0]) - 2 ** L) <= 1e-10 * 2 ** L


BETAS = [0.3, 1.0, 2.5]


@functools.lru_cache(maxsize=None)
def sampled_density():
    """Couplings of size 0.15, so that beta (E - a) stays moderate for beta <= 2.5 on the interval (a, b) = (-B, B): the moments
    carry absolute errors of eps mu_0, and sum_m c_m mu_m = e^{beta a} Z keeps digits only while e^{-beta (E0 + B)} is well above
    eps.  With couplings of size 1 (B = 37, E0 = -15) the sum is pure rounding at beta = 2.5 in the twin as on the GPU -- the
    limit stated in docs/design/33-chebyshev-moments.md, not a property of the kernel."""
    L, R, seed = 8, 4, 11
    bonds, p = thermal_model(L, 3610)
    p = 0.15 * p
    B = blockref.coupling_bound(L, bonds, p)
    M = max(64, chebyshev.exp_order(BETAS[-1] * B))
    got = thermal.spin_density_of_states(L, bonds, to_dev(p), M, R=R, seed=seed, dense_below=0)
    return L, R, seed, bonds, p, M, got


def test_spin_density_of_states_with_every_sector_sampled_against_the_twin():
    L, R, seed, bonds, p, M, got = sampled_density()
    want = twin.spin_moments(L, bonds, p, M, R=R, seed=seed, dense_below=0, bounds=got.bounds)
    worst = float(np.abs(got.moments.numpy() - want).max())
    print("spin_density_of_states L = 8, every sector sampled, R = 4, M = %d: worst deviation from the twin %.2e (bar %.2e)"
          % (M, worst, 1e-10 * 2 ** L))
    assert worst <= 1e-10 * 2 ** L and abs(float(got.moments[0]) - 2 ** L) <= 1e-10 * 2 ** L


def test_logtrace_exp_against_the_lanczos_ensemble_on_the_same_seeds():
    """ln Z from the moments beside ``spin_thermodynamics`` with k = n on the same start vectors: both estimate
    sum_r <r| e^{-beta H} |r>.  The two twins differ by d (Lanczos without re-orthogonalisation is no exact quadrature at k = n);
    the bar is that of the matching row of docs/design/31-chebyshev-propagator.md, max(1e-10, 10 d)."""
    L, R, seed, bonds, p, M, got = sampled_density()
    assert M >= chebyshev.exp_order(BETAS[-1] * got.bounds[1])
    k = math.comb(L, L // 2)
    lanczos = thermal.spin_thermodynamics(L, bonds, to_dev(p), R=R, k=k, seed=seed, dense_below=0).logZ(torch.tensor(BETAS, dtype=F64))
    lanczos_twin = blockref.logZ(blockref.spin_entries(L, bonds, p, R=R, k=k, seed=seed, dense_below=0), BETAS)
    mu_twin = twin.spin_moments(L, bonds, p, M, R=R, seed=seed, dense_below=0, bounds=got.bounds)
    kpm_twin = np.array([twin.logtrace_exp(mu_twin, got.bounds, beta) for beta in BETAS])
    d = float(np.abs(kpm_twin - lanczos_twin).max())
    value = np.array([got.logtrace_exp(beta) for beta in BETAS])
    deviation = float(np.abs(value - lanczos.numpy()).max())
    bar = max(1e-10, 10.0 * d)
    print("ln Z, Chebyshev moments - Lanczos ensemble: %.2e on the GPU, %.2e between the twins (bar %.2e)" % (deviation, d, bar))
    assert deviation <= bar


def test_kpm_structure_factor_against_the_lanczos_poles():
    """S^{zz}(q = pi, omega) at L = 8: the moments of the KPM measure against sum_j w_j T_m of the poles and weights of
    ``dynamical_structure_factor`` with k = n (the full spectral decomposition of Z_q psi0)"""
    L, ndown, M = 8, 4, 64
    bonds = tuple(ring_bonds(L))
    p = np.concatenate([np.full(L, 1.0), np.full(L, 1.0), normal_vector(L, 3900) * 0.05])
    op = SpinSectorOperator(L, bonds, to_dev(p), ndown)
    theta, V = np.linalg.eigh(ref.dense(L, ndown, bonds, p))
    psi0, E0 = to_dev(V[:, 0]), float(theta[0])
    weights = ring_momentum_weights(L, L // 2)
    lanczos = spectral.dynamical_structure_factor(op, psi0, E0, weights, "zz", k=op.n)
    got = spectral.kpm_structure_factor(op, psi0, E0, weights, "zz", M=M)
    a, b = chebyshev.spectral_bounds(op)
    assert abs(got.bounds[0] - (a - E0)) <= 1e-12 and abs(got.bounds[1] - (b - E0)) <= 1e-12 and len(got) == M
    s = (lanczos.poles.numpy() - 0.5 * (got.bounds[0] + got.bounds[1])) / (0.5 * (got.bounds[1] - got.bounds[0]))
    want = (twin.chebyshev_of(s, M) @ lanczos.weights.numpy().astype(LD)).astype(np.float64)
    worst = float(np.abs(got.moments.numpy() - want).max())
    print("kpm_structure_factor L = 8, q = pi: worst moment deviation %.2e (bar %.2e)" % (worst, 1e-10 * lanczos.norm2))
    assert lanczos.norm2 > 0.1 and worst <= 1e-10 * lanczos.norm2
    other = spectral.kpm_structure_factor(op, psi0, E0, weights, "-", M=16)                     # lands in ndown + 1, on new tables
    assert len(other) == 16 and float(other.moments[0]) > 0


def test_the_example_runs_and_its_density_integrates_to_one():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "spin_lattice", "density_of_states.py")
    spec = importlib.util.spec_from_file_location("spin_lattice_density_of_states", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = ex.main(L=8, moments=64)
    assert out["L"] == 8 and out["M"] == 64 and abs(out["B"] - 24.0) <= 1e-12
    assert abs(out["integral"] - 1.0) <= 1e-10 and abs(out["mu0"] - 256.0) <= 1e-10 * 256
    assert out["norm2_moments"] == pytest.approx(out["norm2_lanczos"], rel=1e-10)
    # every sector is exact at L = 8 in both; M = 64 >= exp_order(0.5 * 24): the two ln Z agree to rounding
    assert np.abs(np.array(out["logZ_moments"]) - np.array(out["logZ_lanczos"])).max() <= 1e-10


def test_the_worst_deviations_of_this_run():
    """(printed for docs/design/33-chebyshev-moments.md; runs after the comparisons above)"""
    for key in sorted(WORST):
        print("worst of fused, unfused and twin, %s: %.2e ||l|| ||x||" % (key, WORST[key]))
