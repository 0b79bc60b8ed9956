"""The finite-temperature optical response of the Hubbard model without a GPU (docs/design/40-finite-temperature-conductivity.md):
the numpy twin of tests/hubbard_current_block_reference.py against dense matrices and against the 4^L Fock space, the identity
K_d - X = d^2 F / d phi^2 against a second difference of the free energy of the complex H(phi), the host matrices of
``thermal``, the dense route of ``hubbard_thermal_conductivity`` on edge sectors, the arithmetic of ``ThermalOpticalResponse`` on
hand-made records, and the argument validation of the two C-ABI entries and of the Python layer, which runs before any device
work."""
import ctypes
import math
from ctypes import byref, c_int32, c_int64, c_void_p

import numpy as np
import pytest
import torch

import hubbard_current_block_reference as twin
import hubbard_current_reference as cref
import hubbard_reference as hub
import lattice_reference
from dominantsparseeigenad_amd import _lib, thermal
from dominantsparseeigenad_amd.synthetic import normal_vector

LD = np.longdouble
RING4 = [(0, 1), (1, 2), (2, 3), (3, 0), (0, 2)]         # the 4-site ring and one diagonal bond
D4 = [1.0, 1.0, 1.0, 1.0, 2.0]


def bonds_for(L):
    """random pairs, plus one pair reversed and one repeated"""
    bonds = lattice_reference.random_bonds(L, L + 2, 70 + L)
    a, b = bonds[0]
    return bonds + [(b, a), bonds[1]]


def couplings(L, bonds, seed):
    """random t, V, U, eps of order one"""
    p = normal_vector(hub.nparam(L, bonds), seed)
    p[:len(bonds)] = 1.0 + 0.3 * p[:len(bonds)]
    return p


def test_twin_dots_are_the_dense_column_sums():
    L, nup, ndn = 5, 2, 3
    bonds = bonds_for(L)
    n = math.comb(L, nup) * math.comb(L, ndn)
    w = normal_vector(2 * len(bonds), 4000).reshape(2, -1)
    X = np.stack([normal_vector(n, 4001 + j) for j in range(3)], axis=1)
    Lft = np.stack([normal_vector(n, 4011 + j) for j in range(3)], axis=1)
    K = cref.dense(L, nup, ndn, bonds, w)
    d64, dld = twin.dots(L, nup, ndn, bonds, w, Lft, X), twin.dots(L, nup, ndn, bonds, w, Lft, X, LD)
    want = np.einsum("rj,rj->j", Lft.astype(LD), K.astype(LD) @ X.astype(LD))
    scale = np.linalg.norm(Lft, axis=0) * np.linalg.norm(K @ X, axis=0)
    assert dld.dtype == LD and d64.dtype == np.float64
    assert np.all(np.abs(dld - want) <= 1e-17 * len(bonds) * scale)
    assert np.all(np.abs(d64 - want.astype(np.float64)) <= 1e-14 * scale)
    assert np.array_equal(twin.apply_block(L, nup, ndn, bonds, w, X)[:, 1], cref.apply(L, nup, ndn, bonds, w, X[:, 1]))
    # antisymmetry: l . K x = -x . K l, and x . K x = 0
    back = twin.dots(L, nup, ndn, bonds, w, X, Lft, LD)
    assert np.all(np.abs(dld + back) <= 1e-17 * len(bonds) * scale)
    assert np.all(np.abs(twin.dots(L, nup, ndn, bonds, w, X, X, LD)) <= 1e-17 * len(bonds) * scale)


@pytest.mark.parametrize("L", [2, 3, 4])
def test_the_host_matrices_are_the_twins(L):
    bonds = bonds_for(L)
    nb = len(bonds)
    w = normal_vector(2 * nb, 4020 + L).reshape(2, nb)
    td2 = normal_vector(nb, 4030 + L)
    for nup in range(L + 1):
        for ndn in range(L + 1):
            K = thermal._dense_hubbard_current_matrix(L, nup, ndn, bonds, torch.from_numpy(w)).numpy()
            want = cref.dense(L, nup, ndn, bonds, w)
            assert K.shape == want.shape == (math.comb(L, nup) * math.comb(L, ndn),) * 2
            assert np.max(np.abs(K - want)) <= 1e-14 * max(1.0, np.max(np.abs(want))), (L, nup, ndn)
            assert np.array_equal(K, -K.T)                                        # antisymmetric bit for bit
            if nup in (0, L) and ndn in (0, L):
                assert not K.any()
            T = thermal._dense_hubbard_diamagnetic_matrix(L, nup, ndn, bonds, torch.from_numpy(td2)).numpy()
            want = twin.dense_diamagnetic(L, nup, ndn, bonds, td2)
            assert np.max(np.abs(T - want)) <= 1e-14 * max(1.0, np.max(np.abs(want))), (L, nup, ndn)
            assert np.array_equal(T, T.T)
    one = thermal._dense_hubbard_current_matrix(L, 1, 1, bonds, torch.from_numpy(w[0]))
    assert torch.equal(one, thermal._dense_hubbard_current_matrix(L, 1, 1, bonds, torch.from_numpy(np.stack([w[0], w[0]]))))
    with pytest.raises(ValueError, match="weights"):
        thermal._dense_hubbard_current_matrix(L, 1, 1, bonds, torch.zeros(3, nb))


@pytest.mark.parametrize("kind", ["charge", "spin"])
def test_sector_sums_are_the_fock_space_trace(kind):
    L = 3
    bonds = [(0, 1), (1, 2), (2, 0), (1, 0)]
    p = couplings(L, bonds, 4040)
    d = [1.0, 1.0, 1.0, -1.0]
    betas, mus, times = [0.0, 0.7, 2.1], [-0.4, 0.9], 0.3 * np.arange(5)
    a, b = twin.thermal(L, bonds, p, d, kind, betas, mus, times), twin.full_space(L, bonds, p, d, kind, betas, mus, times)
    c0 = np.abs(b["C"][:, :, :1])
    assert np.max(np.abs(a["logXi"] - b["logXi"])) <= 1e-10
    assert np.max(np.abs(a["C"] - b["C"]) / c0) <= 1e-10
    assert np.max(np.abs(a["K_d"] - b["K_d"])) <= 1e-10 and np.max(np.abs(a["X"] - b["X"])) <= 1e-10
    assert np.max(np.abs(a["C"][:, :, 0].imag)) <= 1e-14 * c0.max() and c0.min() > 0
    assert np.all(a["X"][0] == 0)                                   # g_0 = 0: no response at infinite temperature


def test_stiffness_is_the_second_derivative_of_the_free_energy():
    """K_d - X against the central second difference of F(phi) at h = 1e-3 within 1e-5: the h^2 F''''/ 12 truncation, the bound of
    docs/design/39-hubbard-current.md section 39.6.  Measured 1.5e-6."""
    L, beta, mu, h = 4, 1.3, 0.4, 1e-3
    p = couplings(L, RING4, 4050)
    out = twin.thermal(L, RING4, p, D4, "charge", [beta], [mu], np.zeros(1))
    F = [twin.free_energy(L, RING4, p, D4, phi, beta, mu) for phi in (-h, 0.0, h)]
    second = (F[0] - 2.0 * F[1] + F[2]) / (h * h)
    want = float(out["K_d"][0, 0] - out["X"][0, 0])
    print("d2F/dphi2 = %.7f   K_d - X = %.7f   |difference| = %.2e" % (second, want, abs(second - want)))
    assert abs(second - want) <= 1e-5
    assert abs(F[1] + out["logXi"][0, 0] / beta) <= 1e-12 * abs(F[1])                             # F(0) = -ln Xi / beta


# ---- argument validation without a device ----------------------------------------------------------------------------------------
ERR_ALIGN = -2     # DSEA_ERR_ALIGN of include/dsea.h


def flat(bonds):
    return (c_int32 * (2 * len(bonds)))(*[s for bond in bonds for s in bond])


def test_c_entry_refuses_bad_arguments_before_any_device_work():
    lib = _lib.load()
    dummy = (ctypes.c_double * 64)()
    base = ctypes.addressof(dummy)
    base += (-base) % 16
    ptr, ptr2, odd = c_void_p(base), c_void_p(base + 64), c_void_p(base + 8)
    h = c_void_p()
    assert lib.dsea_op_create_hubbard(10, 5, 4, 4, flat([(0, 1), (9, 3), (3, 9), (0, 1)]), *([ptr] * 7), byref(h)) == 0
    dots = lib.dsea_op_hubbard_current_block_dots
    assert dots(None, 1, ptr, ptr, ptr2, ptr, ptr, None) == _lib.ERR_ARG                  # no operator
    for R in (0, 3, 5, 6, 7, 9, 16, -1):
        assert dots(h, R, ptr, ptr, ptr2, ptr, ptr, None) == _lib.ERR_ARG, R              # R outside {1, 2, 4, 8}
    for k in range(5):                                                                    # null weights, Lft, X, out, scratch
        args = [ptr, ptr, ptr2, ptr, ptr]
        args[k] = None
        assert dots(h, 2, *args, None) == _lib.ERR_ARG, k
    for R in (2, 4, 8):
        assert dots(h, R, ptr, odd, ptr2, ptr, ptr, None) == ERR_ALIGN                    # blocks of R >= 2 on a 16-byte boundary
        assert dots(h, R, ptr, ptr2, odd, ptr, ptr, None) == ERR_ALIGN
    assert dots(h, 2, ptr, odd, odd, None, ptr, None) == _lib.ERR_ARG                     # the argument checks come first
    assert lib.dsea_op_destroy(h) == 0
    assert lib.dsea_op_create_sector(10, 5, 1, flat([(0, 1)]), ptr, ptr, ptr, ptr, byref(h)) == 0
    assert dots(h, 1, ptr, ptr, ptr2, ptr, ptr, None) == _lib.ERR_ARG                     # an operator of another kind
    assert lib.dsea_op_destroy(h) == 0


def test_the_scratch_query():
    query = _lib.load().dsea_op_hubbard_current_block_dots_scratch_doubles
    need = c_int64()
    for R in (1, 2, 4, 8):
        assert query(6, 3, 3, R, byref(need)) == 0 and need.value == 2 * R                # 400 rows: two blocks
        assert query(2, 1, 1, R, byref(need)) == 0 and need.value == R
        assert query(16, 8, 8, R, byref(need)) == 0 and need.value == 4096 * R            # capped at the largest grid
        assert query(10, 5, 5, R, byref(need)) == 0 and need.value == 249 * R
    for bad in ((1, 1, 1, 1), (41, 2, 2, 1), (10, 0, 5, 1), (10, 5, 10, 1), (18, 9, 9, 1), (10, 5, 5, 0), (10, 5, 5, 3),
                (10, 5, 5, 16), (10, 5, 5, -1)):
        assert query(*bad, byref(need)) == _lib.ERR_ARG, bad
    assert query(6, 3, 3, 8, None) == _lib.ERR_ARG


class FakeOperator:
    """what HubbardCurrent reads of its operator, without tables or a handle"""
    N, nup, ndn, nb, n, bonds, handle = 6, 3, 3, 5, 400, ((0, 1), (1, 2), (2, 3), (3, 4), (4, 5)), None
    device = torch.device("cpu")


def test_block_dots_checks_its_arguments_on_the_host(monkeypatch):
    from dominantsparseeigenad_amd import operators
    from dominantsparseeigenad_amd.operators import HubbardCurrent

    def no_device(*args, **kwargs):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(operators._lib, "load", no_device)
    cur = HubbardCurrent(FakeOperator())
    X = torch.zeros(400, 3, dtype=torch.float64)
    w = torch.zeros(2, 5, dtype=torch.float64)
    for bad in (torch.zeros(4), torch.zeros(2, 4), torch.zeros(3, 5), torch.zeros(5, 2), torch.zeros(5, dtype=torch.complex128)):
        with pytest.raises(ValueError, match="weights"):
            cur.block_dots(bad, X, X)
    for bad in (torch.zeros(400, dtype=torch.float64), torch.zeros(399, 3, dtype=torch.float64), torch.zeros(400, 0, dtype=torch.float64),
                torch.zeros(400, 3, dtype=torch.complex128), torch.zeros(400, 3, dtype=torch.float64, device="meta"), [0.0] * 400):
        with pytest.raises(ValueError):
            cur.block_dots(w, bad, X)
        with pytest.raises(ValueError):
            cur.block_dots(w, X, bad)
    with pytest.raises(ValueError, match="same number of columns"):
        cur.block_dots(w, torch.zeros(400, 2, dtype=torch.float64), X)


def failing(name):
    def fail(*args, **kwargs):
        raise AssertionError("%s ran although the call had to be refused" % name)
    return fail


SECTOR_ROUTINES = ("one_species_matrix", "_dense_sector_matrix", "_dense_pair_dynamics", "_tpq_block_dynamics", "_tpq_states",
                   "_tpq_diamagnetic", "_dense_hubbard_current_matrix", "_dense_hubbard_diamagnetic_matrix")


def test_hubbard_thermal_conductivity_refuses_before_any_sector(monkeypatch):
    from dominantsparseeigenad_amd import operators
    for name in SECTOR_ROUTINES:
        monkeypatch.setattr(thermal, name, failing(name))
    monkeypatch.setattr(operators, "HubbardOperator", failing("HubbardOperator"))
    L, bonds = 4, RING4
    c = torch.ones(2 * 5 + 2 * 4, dtype=torch.float64)
    good = dict(L=L, bonds=bonds, couplings=c, displacements=D4, betas=[0.5, 1.0], mus=[0.0], dt=0.1, steps=3)
    for change in (dict(L=1), dict(L=41), dict(bonds=[(0, 0)]), dict(bonds=[(0, 4)]), dict(couplings=c[:-1]),
                   dict(displacements=D4[:-1]), dict(displacements=torch.zeros(5, dtype=torch.complex128)),
                   dict(displacements=torch.zeros(1, 5)), dict(displacements=[1.0, 1.0, float("inf"), 1.0, 1.0]),
                   dict(betas=[]), dict(betas=[-0.1]), dict(betas=[1.0, 0.5]), dict(betas=[float("nan")]),
                   dict(mus=[]), dict(mus=[float("inf")]), dict(dt=0.0), dict(dt=-1.0), dict(dt=float("inf")), dict(steps=-1),
                   dict(R=0), dict(kind="heat"), dict(sectors=[]), dict(sectors=[(1, 1), (1, 1)]), dict(sectors=[(5, 0)]),
                   dict(sectors=[(0, -1)])):
        with pytest.raises(ValueError):
            thermal.hubbard_thermal_conductivity(**{**good, **change})
    # an edge sector above edge_dense_max rows, listed after sectors that would be computed
    with pytest.raises(ValueError, match="edge_dense_max"):
        thermal.hubbard_thermal_conductivity(**{**good, "sectors": [(2, 2), (0, 0), (0, 2)], "edge_dense_max": 5})
    with pytest.raises(ValueError, match="edge_dense_max"):
        thermal.hubbard_thermal_conductivity(**{**good, "sectors": [(1, 4)], "edge_dense_max": 3})


@pytest.mark.parametrize("kind", ["charge", "spin"])
def test_the_dense_route_on_edge_sectors_needs_no_device(monkeypatch, kind):
    from dominantsparseeigenad_amd import operators
    monkeypatch.setattr(operators, "HubbardOperator", failing("HubbardOperator"))
    L, bonds = 4, RING4
    p = couplings(L, bonds, 4060)
    sectors = [(0, 2), (4, 1), (0, 0), (4, 4), (3, 0), (2, 4), (0, 4), (4, 0), (0, 1)]
    betas, mus, dt, steps = [0.0, 0.6, 1.9], [-0.4, 0.9], 0.3, 6
    got = thermal.hubbard_thermal_conductivity(L, bonds, torch.from_numpy(p), D4, betas, mus, dt, steps, kind=kind, sectors=sectors,
                                               device="cpu")
    want = twin.thermal(L, bonds, p, D4, kind, betas, mus, dt * np.arange(steps + 1), sectors=sectors)
    assert isinstance(got, thermal.ThermalOpticalResponse)
    assert got.correlation.shape == (3, 2, 7) and got.correlation.dtype == torch.complex128
    assert got.diamagnetic.shape == got.logXi.shape == (3, 2) and got.times.tolist() == (dt * np.arange(7)).tolist()
    c0 = np.abs(want["C"][:, :, :1])
    assert np.max(np.abs(got.logXi.numpy() - want["logXi"])) <= 1e-12
    assert np.max(np.abs(got.correlation.numpy() - want["C"]) / c0) <= 1e-12
    assert np.max(np.abs(got.diamagnetic.numpy() - want["K_d"])) <= 1e-12
    assert np.max(np.abs(got.static().numpy() - want["C"][:, :, 0].real)) <= 1e-12 * c0.max()
    # both species frozen alone: one state, no current, no kinetic energy
    frozen = thermal.hubbard_thermal_conductivity(L, bonds, torch.from_numpy(p), D4, betas, mus, dt, steps, kind=kind,
                                                  sectors=[(0, 4), (4, 4)], device="cpu")
    assert not frozen.correlation.abs().max() and not frozen.diamagnetic.abs().max()


# ---- ThermalOpticalResponse on hand-made records ------------------------------------------------------------------------------
def hand_made(betas, eta):
    """C(t) = sum_i a_i e^{-i eps_i t} at every beta (one mu), the same for all: the record of poles eps_i with weights a_i"""
    eps, a = np.array([-1.5, 0.0, 0.8, 2.3]), np.array([0.4, 0.25, 1.1, 0.6])
    dt = 0.05
    K = int(math.ceil(8.5 / (eta * dt)))
    times = dt * torch.arange(K + 1, dtype=torch.float64)
    C = torch.from_numpy((a[None, :] * np.exp(-1j * times.numpy()[:, None] * eps[None, :])).sum(axis=1))
    B = len(betas)
    r = thermal.ThermalOpticalResponse(torch.tensor(betas, dtype=torch.float64), torch.zeros(1, dtype=torch.float64), times,
                                       torch.zeros(B, 1, dtype=torch.float64), C[None, None, :].repeat(B, 1, 1).contiguous(),
                                       torch.full((B, 1), 3.0, dtype=torch.float64))
    return r, eps, a


def test_regular_weight_and_stiffness_on_gaussians():
    """A pole at eps becomes the Gaussian of width eta at omega = eps.  With eta t_K >= 8.5 the record's cut leaves out less
    than e^{-36} / (eta^2 t_K) of a unit pole, and with dt = 0.05 the images of the trapezoid sum sit 2 pi / dt = 125 away: the
    bound 1e-13 * sum a / eta is rounding in the sum over ~700 times."""
    eta, betas = 0.25, [0.0, 0.7, 3.0]
    r, eps, a = hand_made(betas, eta)
    omega = np.linspace(-4.0, 5.0, 901)
    gauss = (a[None, :] * np.exp(-0.5 * ((omega[:, None] - eps[None, :]) / eta) ** 2)).sum(axis=1) / (eta * math.sqrt(2 * math.pi))
    bar = 1e-13 * a.sum() / eta
    S = r.spectrum(omega, eta).numpy()
    assert S.shape == (3, 1, 901) and np.max(np.abs(S - gauss[None, None, :])) <= bar
    sigma = r.regular(omega, eta).numpy()
    g = np.stack([twin.g(beta, omega) for beta in betas])
    assert np.all(g[0] == 0) and g[2][400] == 3.0 and omega[400] == 0.0            # g_0 = 0, g_beta(0) = beta
    assert np.all(sigma[0] == 0)
    assert np.max(np.abs(sigma - math.pi * g[:, None, :] * gauss[None, None, :])) <= math.pi * g.max() * bar
    want = math.pi * g * gauss[None, :]
    h = omega[1] - omega[0]
    trap = h * (want.sum(axis=1) - 0.5 * (want[:, 0] + want[:, -1]))
    weight = r.weight(omega, eta).numpy()
    assert weight.shape == (3, 1) and np.max(np.abs(weight[:, 0] - trap)) <= 9.0 * math.pi * g.max() * bar
    assert np.max(np.abs(r.stiffness(omega, eta).numpy()[:, 0] - (3.0 - trap / math.pi))) <= 9.0 * g.max() * bar
    assert float(r.stiffness(omega, eta)[0, 0]) == 3.0                              # beta = 0: the diamagnetic term alone
    assert np.allclose(r.static().numpy(), a.sum(), rtol=0, atol=1e-15 * a.sum())
    for bad in ([0.0], [0.0, 0.1, 0.3], [0.2, 0.1, 0.0]):
        with pytest.raises(ValueError, match="grid"):
            r.weight(bad, eta)
    with pytest.raises(ValueError, match="eta"):
        r.regular(omega, 0.0)

