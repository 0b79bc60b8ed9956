"""The bond current map of a Hubbard sector without a GPU (docs/design/39-hubbard-current.md): the row formula of
tests/hubbard_current_reference.py against the matrix of the same operator from 2 x 2 Kronecker factors, the stiffness
identities on dense ``eigh`` (open chain, ring against the second difference of E0 under a Peierls phase, closed shell), the
arithmetic of ``OpticalResponse`` on a hand-made measure, and the argument validation of the three C-ABI entries and of the
Python class, which runs before any device work."""
import ctypes
import math
from ctypes import byref, c_int32, c_int64, c_void_p

import numpy as np
import pytest
import torch

import hubbard_current_reference as cref
import lattice_reference
from dominantsparseeigenad_amd import _lib
from dominantsparseeigenad_amd.spectral import OpticalResponse, SpectralMeasure
from dominantsparseeigenad_amd.synthetic import normal_vector


def bonds_for(L):
    """random pairs, plus one pair reversed and one repeated (at L = 2 every pair is (0, 1) or (1, 0))"""
    bonds = lattice_reference.random_bonds(L, L + 2, 70 + L)
    a, b = bonds[0]
    return bonds + [(b, a), bonds[1]]


@pytest.mark.parametrize("L", [2, 3, 4])
def test_the_row_formula_is_the_kronecker_matrix(L):
    bonds = bonds_for(L)
    assert any((b, a) in bonds for a, b in bonds) and len(set(bonds)) < len(bonds)
    w = normal_vector(2 * len(bonds), 3900 + L).reshape(2, len(bonds))
    for nup in range(1, L):
        for ndn in range(1, L):
            K = cref.dense(L, nup, ndn, bonds, w)
            want, leak = cref.dense_jordan_wigner(L, nup, ndn, bonds, w)
            assert K.shape == want.shape == (math.comb(L, nup) * math.comb(L, ndn),) * 2
            err = float(np.max(np.abs(K - want)))
            assert err <= 1e-14 * max(1.0, float(np.max(np.abs(want)))), (L, nup, ndn, err)
            assert leak == 0.0                       # the particle numbers are conserved: exactly nothing leaves the sector
            assert np.array_equal(K, -K.T)           # antisymmetric bit for bit


def test_orientation_repetition_and_the_forms():
    """reversing a bond flips its term, a repeated bond counts twice, a (nb,) vector serves both species, and the forms are
    the derivative of the bilinear map"""
    L, nup, ndn = 5, 2, 3
    n = math.comb(L, nup) * math.comb(L, ndn)
    x, y = normal_vector(n, 3910), normal_vector(n, 3911)
    one = cref.apply(L, nup, ndn, [(1, 3)], [[0.7], [-0.4]], x)
    assert np.array_equal(cref.apply(L, nup, ndn, [(3, 1)], [[0.7], [-0.4]], x), -one)
    twice = cref.apply(L, nup, ndn, [(1, 3), (1, 3)], [[0.7, 0.7], [-0.4, -0.4]], x)
    assert np.max(np.abs(twice - 2.0 * one)) <= 4e-16 * np.max(np.abs(one))      # (up + dn) + up + dn against 2 (up + dn)
    bonds = bonds_for(L)
    w = normal_vector(len(bonds), 3912)
    assert np.array_equal(cref.apply(L, nup, ndn, bonds, w, x), cref.apply(L, nup, ndn, bonds, np.stack([w, w]), x))
    w2 = normal_vector(2 * len(bonds), 3913).reshape(2, -1)
    f = cref.forms(L, nup, ndn, bonds, y, x)
    assert abs(float(np.sum(w2 * f)) - float(y @ cref.apply(L, nup, ndn, bonds, w2, x))) <= 1e-13 * np.abs(w2).sum() * 10
    assert np.max(np.abs(cref.forms(L, nup, ndn, bonds, x, x))) <= 1e-14 * float(x @ x)


# ---- the stiffness identities on dense eigh: L = 6 at (3, 3), n = 400 ---------------------------------------------------------
L6 = 6
CHAIN = [(i, i + 1) for i in range(L6 - 1)]
RING = [(i, (i + 1) % L6) for i in range(L6)]        # d_t = +1 on every bond, (5, 0) included: the minimum image


def uniform(bonds, U):
    nb = len(bonds)
    return np.concatenate([np.ones(nb), np.zeros(nb), U * np.ones(L6), np.zeros(L6)])


def test_open_chain_has_no_stiffness():
    """without a loop the twist is a gauge transformation: E0 does not depend on phi and K_d = 2 I_-1"""
    r = cref.optical(L6, 3, 3, CHAIN, uniform(CHAIN, 4.0), np.ones(len(CHAIN)))
    print("open chain: K_d = %.10f  I_-1 = %.10f  K_d - 2 I_-1 = %.2e" % (r["diamagnetic"], r["inverse_moment"], r["stiffness"]))
    assert r["gap"] > 0.1 and r["dropped_weight"] < 1e-24
    assert abs(r["diamagnetic"] - 5.2437343764) < 1e-9
    assert abs(r["inverse_moment"] - 2.6218671882) < 1e-9
    # the sum over 399 levels of terms up to |K psi0|^2 / gap ~ 25, each rounded to 1e-16 relative, and eigenvectors to 1e-14
    assert abs(r["stiffness"]) < 1e-11


def test_ring_stiffness_is_the_second_derivative_of_the_ground_state_energy():
    p, d = uniform(RING, 4.0), np.ones(len(RING))
    r = cref.optical(L6, 3, 3, RING, p, d)
    h = 1e-3
    E = [float(np.linalg.eigvalsh(cref.dense_peierls(L6, 3, 3, RING, p, d, phi))[0]) for phi in (-h, 0.0, h)]
    fd = (E[0] - 2.0 * E[1] + E[2]) / (h * h)
    print("ring U = 4: stiffness %.8f   second difference at h = 1e-3 %.8f" % (r["stiffness"], fd))
    assert abs(E[1] - r["E0"]) < 1e-12                   # H(0) of the Peierls matrix is the real Hamiltonian
    assert abs(r["stiffness"] - 3.91690) < 1e-5
    assert abs(r["stiffness"] - fd) < 1e-5               # truncation h^2 E''''/12 ~ 1e-6, rounding 4e-15 / h^2 ~ 4e-9
    # the spin twist at half filling of the repulsive ring: the same diamagnetic term, another current
    s = cref.optical(L6, 3, 3, RING, p, d, kind="spin")
    assert s["diamagnetic"] == r["diamagnetic"] and s["inverse_moment"] != r["inverse_moment"]


def test_closed_shell_ring_at_u_zero():
    """U = 0, three particles per species on six sites fill k = 0, +-1: the current commutes with H and annihilates psi0"""
    r = cref.optical(L6, 3, 3, RING, uniform(RING, 0.0), np.ones(len(RING)))
    assert r["gap"] > 1.0
    assert math.sqrt(r["norm2"]) < 1e-12
    assert abs(r["diamagnetic"] - 8.0) < 1e-12 and abs(r["stiffness"] - 8.0) < 1e-12


# ---- OpticalResponse arithmetic ------------------------------------------------------------------------------------------------
def hand_made():
    poles = [-1e-12, 5e-10, 0.5, 2.0, 3.5]
    weights = [0.25, 0.125, 0.75, 1.5, 0.5]
    return SpectralMeasure(poles, weights, sum(weights), 5)


def test_optical_response_arithmetic():
    m = hand_made()
    r = OpticalResponse(m, 4.0)
    I = 0.75 / 0.5 + 1.5 / 2.0 + 0.5 / 3.5
    assert r.floor == 1e-9 and r.dropped_weight == 0.375
    assert abs(r.inverse_moment - I) <= 1e-15 * I
    assert abs(r.stiffness - (4.0 - 2.0 * I)) <= 1e-15 * 4.0
    lhs, rhs = r.f_sum()
    assert abs(lhs - rhs) <= 4e-16 * rhs and rhs == math.pi * 2.0
    assert r.measure is m and r.diamagnetic == 4.0
    # a lower floor keeps the pole at 5e-10; a higher one drops the pole at 0.5 too
    low, high = OpticalResponse(m, 4.0, floor=1e-10), OpticalResponse(m, 4.0, floor=1.0)
    assert low.dropped_weight == 0.25 and abs(low.inverse_moment - (I + 0.125 / 5e-10)) <= 1e-15 * low.inverse_moment
    assert high.dropped_weight == 0.375 + 0.75 and abs(high.inverse_moment - (I - 1.5)) <= 1e-15 * I
    with pytest.raises(ValueError):
        r.regular(1.0, 0.0)
    assert r.regular(torch.zeros(3, 2), 0.1).shape == (3, 2)


def test_the_regular_part_integrates_to_pi_times_the_inverse_moment():
    """trapezoid rule on [-W, W] with step h.  What the cut-off leaves out of the Lorentzian of pole theta with strength
    s = w / theta is s (pi - atan((W - theta) / eta) - atan((W + theta) / eta)) <= s eta (1 / (W - theta) + 1 / (W + theta))
    (pi / 2 - atan x <= 1 / x).  The composite trapezoid rule errs by at most (h^2 / 8) * the total variation of f'; f' of
    s eta / (x^2 + eta^2) runs 0 -> max -> -max -> 0 with max = s 3 sqrt(3) / (8 eta^2), so the variation is 4 max."""
    r = OpticalResponse(hand_made(), 4.0)
    eta, W, h = 0.02, 400.0, 1e-3
    omega = torch.linspace(-W, W, int(round(2 * W / h)) + 1, dtype=torch.float64)
    sigma = r.regular(omega, eta).numpy()
    step = float(omega[1] - omega[0])
    integral = step * (sigma.sum() - 0.5 * (sigma[0] + sigma[-1]))
    strengths = {0.5: 0.75 / 0.5, 2.0: 1.5 / 2.0, 3.5: 0.5 / 3.5}
    tail = sum(s * eta * (1.0 / (W - th) + 1.0 / (W + th)) for th, s in strengths.items())
    quad = sum((step * step / 8.0) * 4.0 * s * 3.0 * math.sqrt(3.0) / (8.0 * eta * eta) for s in strengths.values())
    err = abs(integral - math.pi * r.inverse_moment)
    print("integral of sigma_reg = %.8f   pi I_-1 = %.8f   |difference| = %.2e (tail bound %.2e + quadrature bound %.2e)"
          % (integral, math.pi * r.inverse_moment, err, tail, quad))
    assert err <= tail + quad + 1e-12
    # and at a pole the Lorentzian has its height: pi s / (pi eta), the other poles at least 1.5 away add less than s eta / 1.5^2
    peak = float(r.regular(2.0, eta))
    assert abs(peak - strengths[2.0] / eta) <= eta * sum(strengths.values()) / 1.5 ** 2


# ---- argument validation without a device ----------------------------------------------------------------------------------------
ERR_ALIGN = -2     # DSEA_ERR_ALIGN of include/dsea.h


def flat(bonds):
    return (c_int32 * (2 * len(bonds)))(*[s for bond in bonds for s in bond])


def test_c_entries_refuse_bad_arguments_before_any_device_work():
    lib = _lib.load()
    dummy = (ctypes.c_double * 64)()
    base = ctypes.addressof(dummy)
    base += (-base) % 16
    ptr, ptr2, odd = c_void_p(base), c_void_p(base + 64), c_void_p(base + 8)
    h = c_void_p()
    assert lib.dsea_op_create_hubbard(10, 5, 4, 4, flat([(0, 1), (9, 3), (3, 9), (0, 1)]), *([ptr] * 7), byref(h)) == 0
    apply, forms = lib.dsea_op_hubbard_current_apply, lib.dsea_op_hubbard_current_forms
    assert apply(None, 1, ptr, ptr, ptr2, None) == _lib.ERR_ARG                  # no operator
    for R in (0, 3, 5, 6, 7, 9, 16, -1):
        assert apply(h, R, ptr, ptr, ptr2, None) == _lib.ERR_ARG, R              # R outside {1, 2, 4, 8}
    for args in ((None, ptr, ptr2), (ptr, None, ptr2), (ptr, ptr, None)):
        assert apply(h, 2, *args, None) == _lib.ERR_ARG                          # null weights, X, Y
    assert apply(h, 1, ptr, ptr2, ptr2, None) == _lib.ERR_ARG                    # X == Y
    for R in (2, 4, 8):
        assert apply(h, R, ptr, odd, ptr2, None) == ERR_ALIGN               # blocks of R >= 2 on a 16-byte boundary
        assert apply(h, R, ptr, ptr2, odd, None) == ERR_ALIGN
    assert apply(h, 2, ptr, odd, odd, None) == _lib.ERR_ARG                      # the argument checks come first
    for args in ((None, ptr, ptr, ptr), (ptr, None, ptr, ptr), (ptr, ptr, None, ptr), (ptr, ptr, ptr, None)):
        assert forms(h, *args, None) == _lib.ERR_ARG                             # null v1, v2, out, scratch
    assert forms(None, ptr, ptr, ptr, ptr, None) == _lib.ERR_ARG
    assert lib.dsea_op_destroy(h) == 0
    # an operator of another kind
    assert lib.dsea_op_create_sector(10, 5, 1, flat([(0, 1)]), ptr, ptr, ptr, ptr, byref(h)) == 0
    assert apply(h, 1, ptr, ptr, ptr2, None) == _lib.ERR_ARG
    assert forms(h, ptr, ptr, ptr, ptr, None) == _lib.ERR_ARG
    assert lib.dsea_op_destroy(h) == 0


def test_the_scratch_query():
    lib = _lib.load()
    query = lib.dsea_op_hubbard_current_forms_scratch_doubles
    need = c_int64()
    assert query(6, 3, 3, 10, byref(need)) == 0 and need.value == 20 * 2                   # 400 rows: two blocks
    assert query(2, 1, 1, 1, byref(need)) == 0 and need.value == 2
    assert query(16, 8, 8, 3, byref(need)) == 0 and need.value == 6 * 4096                 # capped at the largest grid
    assert query(10, 5, 5, _lib.LATTICE_MAX_BONDS, byref(need)) == 0 and need.value == 2 * _lib.LATTICE_MAX_BONDS * 249
    for bad in ((1, 1, 1, 1), (41, 2, 2, 1), (10, 0, 5, 1), (10, 5, 10, 1), (18, 9, 9, 1), (10, 5, 5, 0),
                (10, 5, 5, _lib.LATTICE_MAX_BONDS + 1)):
        assert query(*bad, byref(need)) == _lib.ERR_ARG, bad
    assert query(6, 3, 3, 10, None) == _lib.ERR_ARG


class FakeOperator:
    """what HubbardCurrent reads of its operator, without tables or a handle"""
    N, nup, ndn, nb, n, bonds, handle = 6, 3, 3, 5, 400, tuple(CHAIN), None
    device = torch.device("cpu")


def test_python_argument_checks_raise_value_error(monkeypatch):
    from dominantsparseeigenad_amd import operators
    from dominantsparseeigenad_amd.operators import HubbardCurrent

    def no_device(*args, **kwargs):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(operators._lib, "load", no_device)
    with pytest.raises(ValueError, match="HubbardOperator"):
        HubbardCurrent(object())
    cur = HubbardCurrent(FakeOperator())
    assert cur.nb == 5 and cur.n == 400 and cur.bonds == tuple(CHAIN)
    x = torch.zeros(400, dtype=torch.float64)
    for w in (torch.zeros(4), torch.zeros(2, 4), torch.zeros(3, 5), torch.zeros(5, 2), torch.zeros(5, dtype=torch.complex128)):
        with pytest.raises(ValueError, match="weights"):
            cur(w, x)
        with pytest.raises(ValueError, match="weights"):
            cur.apply_block(w, x.reshape(-1, 1))
    w = torch.zeros(2, 5, dtype=torch.float64)
    for bad in (torch.zeros(399, dtype=torch.float64), torch.zeros(400, 1, dtype=torch.float64), [0.0] * 400,
                torch.zeros(400, dtype=torch.complex128), torch.zeros(400, dtype=torch.float64, device="meta")):
        with pytest.raises(ValueError):
            cur(w, bad)
        with pytest.raises(ValueError):
            cur.forms(x, bad)
        with pytest.raises(ValueError):
            cur.forms(bad, x)
    for bad in (x, torch.zeros(399, 2, dtype=torch.float64), torch.zeros(400, 0, dtype=torch.float64),
                torch.zeros(400, 2, dtype=torch.complex128), torch.zeros(400, 2, dtype=torch.float64, device="meta")):
        with pytest.raises(ValueError):
            cur.apply_block(w, bad)
    assert tuple(cur._weights(torch.ones(5)).shape) == (2, 5)


def test_optical_conductivity_refuses_bad_arguments():
    from dominantsparseeigenad_amd.spectral import optical_conductivity
    with pytest.raises(ValueError, match="HubbardOperator"):
        optical_conductivity(FakeOperator(), torch.zeros(400), 0.0, torch.ones(5))
