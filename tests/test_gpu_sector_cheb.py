"""k_cheb_sector_block and the layers on it on the GPU (docs/design/31-chebyshev-propagator.md).

    L8-4         n = 70: one partial block              L16-8        n = 12 870: many blocks
    L11-5-ring   n = 462, 11 bonds: chunks 8 + 3 and    L18-9-walk   n = 48 620, grid capped at 2^6: the blocks walk three ranges
                 4 + 4 + 3, the last block partial      L8-4-short   3 bonds: fewer than one chunk

All with random Jxy, Jz and non-zero hz.  The fused kernel must return the BITS of ``apply_block`` followed by separate
elementwise operations; the numpy twin in float64 is met within 1e-13 (relative norm, the bar of one mat-vec, which numpy does
not reproduce bit for bit); the propagators are compared with dense ``eigh`` within max(1e-13, 10 x the twin's
float64-longdouble deviation on the same inputs) ||X||.
"""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hubbard_reference  # noqa: E402
import lattice_reference  # noqa: E402
import sector_block_reference as blockref  # noqa: E402
import sector_cheb_reference as twin  # noqa: E402
import sector_reference as ref  # noqa: E402
from dominantsparseeigenad_amd import chebyshev, thermal  # noqa: E402
from dominantsparseeigenad_amd.operators import HubbardOperator, SpinSectorOperator, ring_bonds  # noqa: E402
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
SMALL = ["L8-4", "L11-5-ring", "L8-4-short"]
ORDERS = [2, 3, 4, 40]          # first only; first and the X-as-old step; the first in-place step; many steps
ONE_APPLICATION = 1e-13


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


def to_dev(a):
    return torch.from_numpy(np.array(a)).to(dev())


@functools.lru_cache(maxsize=None)
def case(name):
    """(couplings, X (n, 13), the rigorous bounds (-B, B)) on the host, computed once and never written to"""
    L, ndown, _, bonds = GEOMETRY[name]
    p = normal_vector(ref.nparam(L, bonds), 3200 + L + len(bonds)).copy()
    assert np.abs(p).min() > 0
    n = math.comb(L, ndown)
    X = np.stack([normal_vector(n, 3300 + 20 * L + j) for j in range(13)], axis=1)
    B = blockref.coupling_bound(L, bonds, p)
    for a in (p, X):
        a.setflags(write=False)
    return p, X, (-B, B)


def operator(name):
    L, ndown, grid, bonds = GEOMETRY[name]
    op = SpinSectorOperator(L, bonds, to_dev(case(name)[0]), ndown)
    if grid is not None:
        op.set_grid_log2(grid)
    return op


def random_coefficients(A, M, seed=3400):
    return normal_vector(A * M, seed + 50 * A + M).reshape(A, M).copy()


def relnorm(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def test_the_geometries_are_what_the_table_says():
    sizes = {name: math.comb(g[0], g[1]) for name, g in GEOMETRY.items()}
    assert sizes == {"L8-4": 70, "L11-5-ring": 462, "L8-4-short": 70, "L16-8": 12870, "L18-9-walk": 48620}
    assert len(GEOMETRY["L11-5-ring"][3]) == 11 and len(GEOMETRY["L8-4-short"][3]) == 3
    assert (48620 + 255) // 256 > 2 * 64                       # capped at 2^6 blocks, a block walks three row ranges


@pytest.mark.parametrize("A", [1, 2])
@pytest.mark.parametrize("R", [1, 2, 4, 8])
@pytest.mark.parametrize("name", NAMES)
def test_the_fused_kernel_returns_the_bits_of_the_unfused_path(name, R, A):
    _, X, bounds = case(name)
    op = operator(name)
    Xd = to_dev(X[:, :R])
    for M in ORDERS:
        c = random_coefficients(A, M)
        got = chebyshev.chebyshev_apply(op, Xd, c, bounds, fused=True)
        want = chebyshev.chebyshev_apply(op, Xd, c, bounds, fused=False)
        assert got.shape == (A, op.n, R) and got.dtype == F64
        assert torch.equal(got, want), (name, R, A, M)
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
        assert torch.equal(chebyshev.chebyshev_apply(op, Xd, c, bounds, fused=True), got)       # a repeated call: identical bits
        assert torch.equal(chebyshev.chebyshev_apply(op, Xd, c, bounds), got)                   # the default is the fused path
        if A == 1:
            assert torch.equal(chebyshev.chebyshev_apply(op, Xd, c[0], bounds), got[0])         # one row: (n, R)
    assert torch.equal(Xd, to_dev(X[:, :R]))                                                    # X is not written


@pytest.mark.parametrize("R", [3, 13])
def test_other_widths_go_through_the_host_split(R):
    _, X, bounds = case("L11-5-ring")
    op = operator("L11-5-ring")
    Xd = to_dev(X[:, :R])
    for M in (4, 40):
        c = random_coefficients(2, M)
        got = chebyshev.chebyshev_apply(op, Xd, c, bounds, fused=True)
        assert got.shape == (2, op.n, R)
        assert torch.equal(got, chebyshev.chebyshev_apply(op, Xd, c, bounds, fused=False))
    assert torch.equal(Xd, to_dev(X[:, :R]))


@pytest.mark.parametrize("name", ["L11-5-ring", "L18-9-walk"])
def test_a_column_of_a_wide_block_is_the_one_column_call(name):
    _, X, bounds = case(name)
    op = operator(name)
    Xd = to_dev(X[:, :8])
    c = random_coefficients(2, 40)
    wide = chebyshev.chebyshev_apply(op, Xd, c, bounds, fused=True)
    for j in range(8):
        single = chebyshev.chebyshev_apply(op, Xd[:, j:j + 1], c, bounds, fused=True)
        assert torch.equal(wide[:, :, j:j + 1], single), (name, j)


@pytest.mark.parametrize("name", NAMES)
def test_against_the_float64_twin(name):
    L, ndown, _, bonds = GEOMETRY[name]
    p, X, bounds = case(name)
    op = operator(name)
    R = 2 if name == "L18-9-walk" else 8
    for M in (4, 40):
        c = random_coefficients(2, M)
        want = twin.chebyshev_apply(L, ndown, bonds, p, X[:, :R], c, bounds)
        for fused in (True, False):
            got = chebyshev.chebyshev_apply(op, to_dev(X[:, :R]), c, bounds, fused=fused).cpu().numpy()
            worst = max(relnorm(got[a], want[a]) for a in range(2))
            print("%s M = %d fused = %s: against the twin %.2e (bar %.0e)" % (name, M, fused, worst, ONE_APPLICATION))
            assert worst <= ONE_APPLICATION


@functools.lru_cache(maxsize=None)
def dense_case(name):
    L, ndown, _, bonds = GEOMETRY[name]
    theta, V = np.linalg.eigh(ref.dense(L, ndown, bonds, case(name)[0]))
    return theta, V


@pytest.mark.parametrize("name", SMALL)
def test_spectral_bounds_hold_the_spectrum(name):
    theta, _ = dense_case(name)
    op = operator(name)
    a, b = chebyshev.spectral_bounds(op)
    B = case(name)[2][1]
    print("%s: spectrum [%.6f, %.6f] inside bounds [%.6f, %.6f], B = %.6f" % (name, theta[0], theta[-1], a, b, B))
    assert a <= theta[0] and theta[-1] <= b and -B <= a < b <= B
    L, ndown, _, bonds = GEOMETRY[name]
    ta, tb = twin.spectral_bounds(L, ndown, bonds, case(name)[0])
    assert abs(a - ta) <= 1e-10 * B and abs(b - tb) <= 1e-10 * B


@pytest.mark.parametrize("tau_h", [0.5, 5.0, 40.0])
@pytest.mark.parametrize("name", ["L8-4", "L11-5-ring"])
def test_expm_block_against_dense_eigh(name, tau_h):
    L, ndown, _, bonds = GEOMETRY[name]
    p, X, _ = case(name)
    X = X[:, :3]
    theta, V = dense_case(name)
    op = operator(name)
    bounds = chebyshev.spectral_bounds(op)
    tau = tau_h / (0.5 * (bounds[1] - bounds[0]))
    Y, shift = chebyshev.expm_block(op, to_dev(X), tau, bounds)
    assert shift == bounds[0] and Y.shape == X.shape
    want = V @ (np.exp(-tau * (theta - shift))[:, None] * (V.T @ X))
    t64, _ = twin.expm(L, ndown, bonds, p, X, tau, bounds)
    tld, _ = twin.expm(L, ndown, bonds, p, X, tau, bounds, dtype=LD)
    deviation = float(np.linalg.norm((t64 - tld).astype(np.float64)) / np.linalg.norm(X))
    bar = max(1e-13, 10.0 * deviation) * np.linalg.norm(X)
    err = float(np.linalg.norm(Y.cpu().numpy() - want))
    print("%s tau h = %g: |Y - dense| = %.2e, twin fp64 - longdouble %.2e ||X||, bar %.2e" % (name, tau_h, err, deviation, bar))
    assert err <= bar
    same, _ = chebyshev.expm_block(op, to_dev(X), 0.0, bounds)                      # tau = 0: a copy
    assert torch.equal(same, to_dev(X))
    if tau_h == 5.0:
        auto, shift2 = chebyshev.expm_block(op, to_dev(X), tau)                     # bounds = None: spectral_bounds(op)
        assert shift2 == shift and torch.equal(auto, Y)


@pytest.mark.parametrize("ht", [0.5, 5.0, 40.0])
@pytest.mark.parametrize("name", ["L8-4", "L11-5-ring"])
def test_time_evolve_against_dense_eigh(name, ht):
    L, ndown, _, bonds = GEOMETRY[name]
    p, X, _ = case(name)
    theta, V = dense_case(name)
    op = operator(name)
    bounds = chebyshev.spectral_bounds(op)
    t = ht / (0.5 * (bounds[1] - bounds[0]))
    psi = X[:, 0:2] + 1j * X[:, 2:4]
    got = chebyshev.time_evolve(op, to_dev(psi), t, bounds)
    assert got.dtype == torch.complex128 and got.shape == psi.shape
    want = V @ (np.exp(-1j * t * theta)[:, None] * (V.T @ psi))
    t64 = twin.time_evolve(L, ndown, bonds, p, psi, t, bounds)
    tld = twin.time_evolve(L, ndown, bonds, p, psi, t, bounds, dtype=LD)
    deviation = float(np.linalg.norm((t64 - tld).astype(np.complex128)) / np.linalg.norm(psi))
    bar = max(1e-13, 10.0 * deviation) * np.linalg.norm(psi)
    err = float(np.linalg.norm(got.cpu().numpy() - want))
    norms = np.abs(np.linalg.norm(got.cpu().numpy(), axis=0) - np.linalg.norm(psi, axis=0)).max()
    print("%s h t = %g: |psi(t) - dense| = %.2e, norm change %.2e, twin fp64 - longdouble %.2e ||psi||, bar %.2e"
          % (name, ht, err, norms, deviation, bar))
    assert err <= bar and norms <= bar
    # a complex state against its real and imaginary parts evolved separately, bit for bit
    re = chebyshev.time_evolve(op, to_dev(X[:, 0:2]), t, bounds)
    im = chebyshev.time_evolve(op, to_dev(X[:, 2:4]), t, bounds)
    assert torch.equal(got, torch.complex(re.real - im.imag, re.imag + im.real))
    vector = chebyshev.time_evolve(op, to_dev(X[:, 0]), t, bounds)                  # (n,) in, (n,) out
    assert vector.shape == (op.n,) and torch.equal(vector, re[:, 0])
    back = chebyshev.time_evolve(op, got, -t, bounds)
    assert float(np.linalg.norm(back.cpu().numpy() - psi)) <= 2.0 * bar


def test_time_zero_is_the_first_point_of_a_time_grid():
    """t = 0, where sin(H t) has no coefficient above zero: the state comes back as it is, with and without bounds; and the
    smallest step next to it, through the kernel, moves the state by no more than ||H|| t"""
    _, X, _ = case("L11-5-ring")
    op = operator("L11-5-ring")
    psi = to_dev(X[:, 0:2] + 1j * X[:, 2:4])
    for bounds in (None, chebyshev.spectral_bounds(op)):
        got = chebyshev.time_evolve(op, psi, 0.0, bounds)
        assert got.dtype == torch.complex128 and torch.equal(got, psi) and got.data_ptr() != psi.data_ptr()
        real = chebyshev.time_evolve(op, to_dev(X[:, 0]), 0.0, bounds)
        assert real.dtype == torch.complex128 and torch.equal(real.real, to_dev(X[:, 0])) and not bool(real.imag.any())
    same, shift = chebyshev.expm_block(op, to_dev(X[:, :3]), 0.0)                # tau = 0 without bounds: no Lanczos run
    assert shift == 0.0 and torch.equal(same, to_dev(X[:, :3]))
    B = case("L11-5-ring")[2][1]
    t = 1e-9 / B
    near = chebyshev.time_evolve(op, psi, t)
    moved = float(torch.linalg.vector_norm(near - psi, dim=0).max())              # |e^{-iHt} psi - psi| <= ||H|| t |psi|, ||H|| <= B
    assert 0 < moved <= B * t * float(torch.linalg.vector_norm(psi, dim=0).max()) + 1e-12
    # the rows of cos and sin at t = 0 through the kernel: [1, 0] and zeros
    rows = np.array([[1.0, 0.0], [0.0, 0.0]])
    assert chebyshev.truncation_order(lambda s: np.sin(0 * s), 24) == 2
    C, S = chebyshev.chebyshev_apply(op, to_dev(X[:, :2]), rows, (-B, B), fused=True)
    assert torch.equal(C, to_dev(X[:, :2])) and not bool(S.any())


def test_expm_block_on_the_hubbard_operator_runs_unfused():
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
    tau = 5.0 / (0.5 * (bounds[1] - bounds[0]))
    Y, shift = chebyshev.expm_block(op, to_dev(X), tau, bounds)
    want = V @ (np.exp(-tau * (theta - shift))[:, None] * (V.T @ X))
    err = float(np.linalg.norm(Y.cpu().numpy() - want))
    print("Hubbard L4 (2, 2): |Y - dense| = %.2e (bar %.2e)" % (err, 1e-13 * np.linalg.norm(X)))
    assert err <= 1e-13 * np.linalg.norm(X)
    with pytest.raises(ValueError):
        chebyshev.chebyshev_apply(op, to_dev(X), [0.5, 0.5], bounds, fused=True)


BETAS = [0.0, 0.3, 1.0, 2.5, 6.0]


def thermal_model(L, seed):
    bonds = tuple(ring_bonds(L)) + ((0, L // 2), (1, L // 2 + 1))
    return bonds, normal_vector(ref.nparam(L, bonds), seed).copy()


@functools.lru_cache(maxsize=None)
def exact_thermal():
    bonds, p = thermal_model(8, 3600)
    return thermal.thermal_correlations(8, bonds, to_dev(p), BETAS), twin.full_space_correlations(8, bonds, p, BETAS)


@pytest.mark.parametrize("key", ["logZ", "energy", "xy", "zz", "z"])
def test_thermal_correlations_with_every_sector_exact(key):
    got, want = exact_thermal()
    value = getattr(got, key).numpy()
    worst = float((np.abs(value - want[key]) / np.maximum(1.0, np.abs(want[key]))).max())
    print("%s at L = 8, every sector exact: worst deviation %.2e (bar 1e-10 max(1, |value|))" % (key, worst))
    assert value.shape == want[key].shape and worst <= 1e-10


@functools.lru_cache(maxsize=None)
def sampled_thermal():
    L, R, seed = 10, 4, 11
    bonds, p = thermal_model(L, 3610)
    got = thermal.thermal_correlations(L, bonds, to_dev(p), BETAS, R=R, seed=seed, dense_below=0)
    want = twin.thermal_correlations(L, bonds, p, BETAS, R=R, seed=seed, dense_below=0)
    return L, R, seed, bonds, p, got, want


@pytest.mark.parametrize("key", ["logZ", "energy", "xy", "zz", "z"])
def test_thermal_correlations_with_every_sector_sampled_against_the_twin(key):
    L, _, _, bonds, p, got, want = sampled_thermal()
    B = blockref.coupling_bound(L, bonds, p)
    bar = 1e-10 * B if key == "energy" else 1e-10                # ln Z 1e-10, E 1e-10 B; the correlators are bounded by 2
    worst = float(np.abs(getattr(got, key).numpy() - want[key]).max())
    print("%s at L = 10, every sector sampled, R = 4: worst deviation from the twin %.2e (bar %.2e)" % (key, worst, bar))
    assert worst <= bar
    if key in ("xy", "zz"):
        d = np.diagonal(getattr(got, key).numpy(), axis1=1, axis2=2)
        assert np.abs(d - (2.0 if key == "xy" else 1.0)).max() <= 1e-12


def test_logZ_against_the_lanczos_ensemble_on_the_same_seeds():
    """ln Z of the thermal pure quantum states beside ``spin_thermodynamics`` with k = n on the same start vectors: both
    estimate sum_r <r| e^{-beta H} |r>.  The two twins differ by d (Lanczos without re-orthogonalisation is no exact
    quadrature at k = n); the bar is that of the basis-free row of tests/test_gpu_thermal.py, max(1e-10, 10 d)."""
    L, R, seed, bonds, p, got, want = sampled_thermal()
    k = math.comb(L, L // 2)
    lanczos = thermal.spin_thermodynamics(L, bonds, to_dev(p), R=R, k=k, seed=seed, dense_below=0).logZ(torch.tensor(BETAS, dtype=F64))
    lanczos_twin = blockref.logZ(blockref.spin_entries(L, bonds, p, R=R, k=k, seed=seed, dense_below=0), BETAS)
    d = float(np.abs(want["logZ"] - lanczos_twin).max())
    deviation = float((got.logZ - lanczos).abs().max())
    bar = max(1e-10, 10.0 * d)
    print("ln Z, thermal pure quantum states - Lanczos ensemble: %.2e on the GPU, %.2e between the twins (bar %.2e)"
          % (deviation, d, bar))
    assert deviation <= bar
