"""The Hubbard model at fixed (nup, ndn) without a GPU (docs/design/19-hubbard.md): the row formula of
tests/hubbard_reference.py against the Jordan-Wigner matrix of the same Hamiltonian, two closed forms (the two-site problem,
free fermions on a lattice with loops), the bilinear forms against differences of the linear map, the pure-Python helpers, and
the argument validation of the Python class and of the new C-ABI entry points, which runs before any device work."""
import ctypes
import math
from ctypes import byref, c_int32, c_int64, c_void_p

import numpy as np
import pytest

import hubbard_reference as ref
import lattice_reference
from dominantsparseeigenad_amd import _lib
from dominantsparseeigenad_amd.synthetic import normal_vector

# six sites, ten bonds: the hexagon, its three diagonals and one chord -- odd and even loops, so the hop signs cannot all be +1
LOOP_BONDS = ((0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (0, 3), (1, 4), (2, 5), (0, 2))


def bonds_for(L):
    """random pairs, plus one pair reversed and one repeated (at L = 2 every pair is (0, 1) or (1, 0))"""
    bonds = lattice_reference.random_bonds(L, L + 2, 70 + L)
    a, b = bonds[0]
    return bonds + [(b, a), bonds[1]]


@pytest.mark.parametrize("L", [2, 3, 4])
def test_the_row_formula_is_the_jordan_wigner_matrix(L):
    bonds = bonds_for(L)
    p = normal_vector(ref.nparam(L, bonds), 2100 + L)
    for nup in range(1, L):
        for ndn in range(1, L):
            H = ref.dense(L, nup, ndn, bonds, p)
            want, leak = ref.dense_jordan_wigner(L, nup, ndn, bonds, p)
            assert H.shape == want.shape == (math.comb(L, nup) * math.comb(L, ndn),) * 2
            err = float(np.max(np.abs(H - want)))
            assert err <= 1e-14 * max(1.0, float(np.max(np.abs(want)))), (L, nup, ndn, err)
            assert leak == 0.0                       # the particle numbers are conserved: exactly nothing leaves the sector
            assert np.array_equal(H, H.T)            # symmetric bit for bit


def test_two_sites_closed_form():
    """one up and one down fermion on two sites: E0 = (U - sqrt(U^2 + 16 t^2)) / 2"""
    t = 0.7
    for U in (0.0, 1.0, 4.0, -2.0):
        p = np.array([t, 0.0, U, U, 0.0, 0.0])
        E0 = np.linalg.eigvalsh(ref.dense(2, 1, 1, [(0, 1)], p))[0]
        assert abs(E0 - 0.5 * (U - math.sqrt(U * U + 16.0 * t * t))) <= 1e-14 * max(1.0, abs(E0))


def free_fermion_parameter():
    nb, L = len(LOOP_BONDS), 6
    p = np.zeros(2 * nb + 2 * L)
    p[:nb] = 1.0 + 0.3 * normal_vector(nb, 2200)
    p[2 * nb + L:] = 0.5 * normal_vector(L, 2201)
    return p


def free_fermion_energy(p, nup, ndn):
    """U = V = 0: the sum of the lowest nup plus the lowest ndn levels of the one-particle matrix -t_ab + eps_a delta_ab"""
    nb, L = len(LOOP_BONDS), 6
    h = np.diag(p[2 * nb + L:])
    for k, (a, b) in enumerate(LOOP_BONDS):
        h[a, b] -= p[k]
        h[b, a] -= p[k]
    lam = np.linalg.eigvalsh(h)
    return float(lam[:nup].sum() + lam[:ndn].sum())


@pytest.mark.parametrize("nup,ndn", [(3, 2), (2, 4), (1, 1), (5, 3)])
def test_free_fermions_on_a_lattice_with_loops(nup, ndn):
    p = free_fermion_parameter()
    E0 = np.linalg.eigvalsh(ref.dense(6, nup, ndn, LOOP_BONDS, p))[0]
    want = free_fermion_energy(p, nup, ndn)
    assert abs(E0 - want) <= 1e-12 * abs(want), (E0, want)


@pytest.mark.parametrize("L,nup,ndn", [(2, 1, 1), (4, 2, 1), (5, 2, 3), (6, 3, 3)])
def test_forms_are_the_differences_of_apply(L, nup, ndn):
    """H is linear in the parameters: H[p + e_q] x - H[p] x = (dH/dp_q) x up to rounding"""
    bonds = bonds_for(L)
    n = math.comb(L, nup) * math.comb(L, ndn)
    p = normal_vector(ref.nparam(L, bonds), 2300 + L)
    v1, v2 = normal_vector(n, 2400 + L), normal_vector(n, 2500 + L)
    got = ref.forms(L, nup, ndn, bonds, v1, v2)
    base = ref.apply(L, nup, ndn, bonds, p, v2)
    scale = np.linalg.norm(v1) * np.linalg.norm(v2) * (np.abs(p).sum() + 1.0)
    for q in range(p.size):
        e = np.zeros(p.size)
        e[q] = 1.0
        want = v1 @ (ref.apply(L, nup, ndn, bonds, p + e, v2) - base)
        assert abs(got[q] - want) <= 1e-13 * scale, (q, got[q], want)
    assert abs(v1 @ base - np.sum(p * got)) <= 1e-13 * scale


def test_hubbard_dim():
    from dominantsparseeigenad_amd.operators import hubbard_dim
    for L in range(1, 9):
        for nup in range(L + 1):
            for ndn in range(L + 1):
                assert hubbard_dim(L, nup, ndn) == math.comb(L, nup) * math.comb(L, ndn)
    assert hubbard_dim(10, 5, 5) == 63504 and hubbard_dim(16, 8, 8) == 165636900 and hubbard_dim(16, 5, 5) == 19079424
    with pytest.raises(ValueError):
        hubbard_dim(4, 5, 1)
    with pytest.raises(ValueError):
        hubbard_dim(4, 1, -1)


def test_hubbard_sizes_without_a_device():
    lib = _lib.load()
    n, n_up, n_dn = c_int64(), c_int64(), c_int64()
    for L, nup, ndn in ((2, 1, 1), (7, 3, 2), (9, 5, 3), (16, 8, 8), (40, 2, 1), (40, 1, 2), (17, 8, 9)):
        assert lib.dsea_hubbard_sizes(L, nup, ndn, byref(n), byref(n_up), byref(n_dn)) == 0, (L, nup, ndn)
        cu, cd = math.comb(L, nup), math.comb(L, ndn)
        assert (n.value, n_up.value, n_dn.value) == (cu * cd, cu, cd), (L, nup, ndn)
    assert math.comb(16, 8) ** 2 == 165636900 and math.comb(17, 8) ** 2 == 590976100 <= 2 ** 31 - 1 < math.comb(18, 9) ** 2
    for L, nup, ndn in ((1, 1, 1), (41, 2, 2), (8, 0, 3), (8, 3, 0), (8, 8, 3), (8, 3, 8), (8, -1, 3), (18, 9, 9), (40, 20, 1),
                        (40, 1, 20), (34, 17, 17)):
        assert lib.dsea_hubbard_sizes(L, nup, ndn, byref(n), byref(n_up), byref(n_dn)) == _lib.ERR_ARG, (L, nup, ndn)
    assert lib.dsea_hubbard_sizes(8, 4, 4, None, byref(n_up), byref(n_dn)) == _lib.ERR_ARG
    assert lib.dsea_hubbard_sizes(8, 4, 4, byref(n), None, byref(n_dn)) == _lib.ERR_ARG
    assert lib.dsea_hubbard_sizes(8, 4, 4, byref(n), byref(n_up), None) == _lib.ERR_ARG
    cnt = c_int64()
    assert lib.dsea_op_hubbard_forms_scratch_doubles(16, 5, 5, 32, byref(cnt)) == 0
    assert cnt.value == (2 * 32 + 2 * 16) * 4096
    assert lib.dsea_op_hubbard_forms_scratch_doubles(7, 3, 2, 4, byref(cnt)) == 0 and cnt.value == (2 * 4 + 2 * 7) * 3
    assert lib.dsea_op_hubbard_forms_scratch_doubles(18, 9, 9, 4, byref(cnt)) == _lib.ERR_ARG
    assert lib.dsea_op_hubbard_forms_scratch_doubles(7, 3, 2, 129, byref(cnt)) == _lib.ERR_ARG
    assert lib.dsea_op_hubbard_forms_scratch_doubles(7, 3, 2, 0, byref(cnt)) == _lib.ERR_ARG
    assert lib.dsea_op_hubbard_forms_scratch_doubles(7, 3, 2, 4, None) == _lib.ERR_ARG


def flat(bonds):
    return (c_int32 * (2 * len(bonds)))(*[s for b in bonds for s in b])


def test_create_hubbard_validates_before_any_device_work():
    lib = _lib.load()
    cap = _lib.LATTICE_MAX_BONDS
    h = c_void_p()
    dummy = (ctypes.c_double * (2 * (cap + 1) + 80))()
    ptr = ctypes.cast(dummy, c_void_p)
    good = [(0, 1), (9, 3), (3, 9), (0, 1)]
    names = ("c", "us", "ul", "uh", "ds", "dl", "dh")

    def create(L, nup, ndn, nb, bonds, out=byref(h), **null):
        args = [None if k in null else ptr for k in names]
        return lib.dsea_op_create_hubbard(L, nup, ndn, nb, bonds, *args, out)

    assert create(1, 1, 1, 1, flat([(0, 1)])) == -1                    # L < 2
    assert create(41, 2, 2, 1, flat([(0, 1)])) == -1                   # L > 40
    assert create(10, 0, 5, 4, flat(good)) == -1                       # nup < 1
    assert create(10, 5, 10, 4, flat(good)) == -1                      # ndn > L - 1
    assert create(18, 9, 9, 4, flat(good)) == -1                       # n > 2^31 - 1
    assert create(10, 5, 5, 0, flat(good)) == -1                       # nb < 1
    many = [(i % 9, 9) for i in range(cap + 1)]
    assert create(10, 5, 5, cap + 1, flat(many)) == -1                 # nb above the cap
    assert create(10, 5, 5, 2, flat([(0, 1), (2, 10)])) == -1          # site out of range
    assert create(10, 5, 5, 2, flat([(0, 1), (-1, 2)])) == -1
    assert create(10, 5, 5, 2, flat([(0, 1), (4, 4)])) == -1           # a == b
    assert create(10, 5, 5, 4, None) == -1                             # null pointers, one at a time
    for k in names:
        assert create(10, 5, 5, 4, flat(good), **{k: True}) == -1, k
    assert create(10, 5, 5, 4, flat(good), out=None) == -1
    assert create(10, 5, 5, cap, flat(many[:cap])) == 0                # the cap itself is accepted
    assert lib.dsea_op_destroy(h) == 0
    assert create(10, 5, 4, 4, flat(good)) == 0                        # nothing is launched at creation
    n = c_int64()
    assert lib.dsea_op_dim(h, byref(n)) == 0 and n.value == 252 * 210
    assert lib.dsea_op_set_tuning(h, _lib.TUNE_TFIM_TILE_LOG2, 6) == 0        # this kind: log2 of the grid cap
    assert lib.dsea_op_set_tuning(h, _lib.TUNE_TFIM_TILE_LOG2, 13) == -1
    # the forms refuse null operands on the host; they refuse other kinds, and the other forms refuse this kind
    assert lib.dsea_op_hubbard_forms(h, None, None, None, None, None) == -1
    assert lib.dsea_op_hubbard_forms(None, ptr, ptr, ptr, ptr, None) == -1
    assert lib.dsea_op_sector_forms(h, ptr, ptr, ptr, ptr, None) == _lib.ERR_ARG
    assert lib.dsea_op_lattice_forms(h, ptr, ptr, ptr, ptr, None) == _lib.ERR_ARG
    assert lib.dsea_op_destroy(h) == 0
    assert lib.dsea_op_create_sector(10, 5, 1, flat([(0, 1)]), ptr, ptr, ptr, ptr, byref(h)) == 0
    assert lib.dsea_op_hubbard_forms(h, ptr, ptr, ptr, ptr, None) == _lib.ERR_ARG
    assert lib.dsea_op_destroy(h) == 0


@pytest.mark.parametrize("L,nup,ndn", [(1, 1, 1), (41, 20, 1), (0, 0, 0), (8, 0, 4), (8, 4, 0), (8, 8, 4), (8, 4, 8), (8, -1, 4),
                                       (8, 4, 9), (18, 9, 9), (40, 20, 20)])
def test_python_argument_checks_fire_before_the_device(L, nup, ndn, monkeypatch):
    """no GPU here: a check that came after the first device call would raise something else than ValueError"""
    import torch
    from dominantsparseeigenad_amd import operators

    def no_device(*args, **kwargs):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(operators._lib, "load", no_device)
    monkeypatch.setattr(torch, "empty", no_device)
    with pytest.raises(ValueError):
        operators.HubbardOperator(L, [(0, 1)], torch.zeros(2 + 2 * max(L, 0), dtype=torch.float64), nup, ndn, device="cuda")


def test_python_refuses_bad_bonds_and_a_host_device(monkeypatch):
    """in the order fillings, bonds, device: a bad bond list is refused although the device is a host device too"""
    import torch
    from dominantsparseeigenad_amd import operators
    from dominantsparseeigenad_amd.operators import HubbardOperator
    c = torch.zeros(2 * 2 + 2 * 8, dtype=torch.float64)
    with pytest.raises(ValueError, match="bond"):
        HubbardOperator(8, [(0, 1), (4, 4)], c, 4, 4, device="cpu")
    with pytest.raises(ValueError, match="bond"):
        HubbardOperator(8, [(0, 1), (4, 8)], c, 4, 4, device="cpu")
    with pytest.raises(ValueError, match="len"):
        HubbardOperator(8, [], c, 4, 4, device="cpu")
    with pytest.raises(ValueError, match="len"):
        HubbardOperator(8, [(0, 1)] * 129, c, 4, 4, device="cpu")
    with pytest.raises(ValueError, match="nup"):
        HubbardOperator(8, [(0, 1), (4, 4)], c, 0, 4, device="cpu")       # the fillings come before the bonds
    with pytest.raises(ValueError, match="device"):
        HubbardOperator(8, [(0, 1), (4, 5)], c, 4, 4, device="cpu")
