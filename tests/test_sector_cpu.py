"""XXZ spins in one magnetisation sector without a GPU (docs/design/18-spin-sector.md): the sector-native numpy reference of
tests/sector_reference.py against the full-space reference restricted to the sector (the identity the whole feature rests on:
the lattice Hamiltonian with Jx = Jy = Jxy and hx = 0 conserves the number of set bits), the pure-Python helpers, and the
argument validation of the Python class and of the new C-ABI entry points, which runs before any device work."""
import ctypes
import math
from ctypes import byref, c_int32, c_int64, c_void_p

import numpy as np
import pytest

import lattice_reference
import sector_reference as ref
from dominantsparseeigenad_amd import _lib
from dominantsparseeigenad_amd.synthetic import normal_vector

SIZES = list(range(2, 9))


def bonds_for(L):
    """random pairs, plus one pair reversed and one repeated (at L = 2 every pair is (0, 1) or (1, 0))"""
    bonds = lattice_reference.random_bonds(L, L + 2, 60 + L)
    a, b = bonds[0]
    return bonds + [(b, a), bonds[1]]


@pytest.mark.parametrize("L", SIZES)
def test_sector_reference_is_the_restricted_lattice_matrix(L):
    bonds = bonds_for(L)
    p = normal_vector(ref.nparam(L, bonds), 1100 + L)
    full = lattice_reference.dense(L, bonds, ref.full_parameter(L, bonds, p))
    p_exact = np.round(p * 1024.0) / 1024.0
    exact = lattice_reference.dense(L, bonds, ref.full_parameter(L, bonds, p_exact))
    for ndown in range(1, L):
        st = np.array(ref.states(L, ndown), dtype=np.int64)
        H = ref.dense(L, ndown, bonds, p)
        assert H.shape == (math.comb(L, ndown),) * 2
        assert np.max(np.abs(H - full[st][:, st])) <= 1e-14 * max(1.0, np.max(np.abs(full)))
        # the Hamiltonian conserves the number of set bits: no entry from a sector state to any other state.  (Couplings that
        # are multiples of 2^-10: the full reference adds Jx_t - Jy_t of bonds with equal masks in one running sum, which
        # cancels exactly only when every partial sum is exact.)
        outside = np.setdiff1d(np.arange(1 << L), st)
        assert np.all(exact[st][:, outside] == 0.0)
        assert np.array_equal(ref.dense(L, ndown, bonds, p_exact), exact[st][:, st])
        # apply and forms against the matrix and its linearity in the couplings
        x, v1 = normal_vector(st.size, 1200 + L + ndown), normal_vector(st.size, 1300 + L + ndown)
        assert np.max(np.abs(ref.apply(L, ndown, bonds, p, x) - H @ x)) <= 1e-13 * np.abs(p).sum() * np.max(np.abs(x))
        forms = ref.forms(L, ndown, bonds, v1, x)
        scale = np.linalg.norm(v1) * np.linalg.norm(x) * np.abs(p).sum()
        assert abs(v1 @ (H @ x) - np.sum(p * forms)) <= 1e-13 * scale


def test_sector_dim_and_states():
    from dominantsparseeigenad_amd.operators import sector_dim, sector_states
    for L in range(1, 11):
        for ndown in range(L + 1):
            assert sector_dim(L, ndown) == math.comb(L, ndown)
            got = sector_states(L, ndown)
            want = sorted(s for s in range(1 << L) if bin(s).count("1") == ndown)
            assert got == want
            if 0 < ndown < L:
                assert tuple(got) == ref.states(L, ndown)
    assert sector_dim(24, 12) == 2704156 and sector_dim(40, 20) == 137846528820
    assert sector_states(40, 1) == [1 << i for i in range(40)]
    high = sector_states(40, 2)
    assert len(high) == 780 and high[-1] == (1 << 39) | (1 << 38) and high == sorted(high)
    with pytest.raises(ValueError):
        sector_dim(4, 5)


@pytest.mark.parametrize("L,ndown", [(1, 1), (41, 20), (0, 0), (8, 0), (8, 8), (8, -1), (8, 9), (34, 17), (40, 20)])
def test_python_argument_checks_fire_before_the_device(L, ndown, monkeypatch):
    """no GPU here: a check that came after the first device call would raise something else than ValueError"""
    import torch
    from dominantsparseeigenad_amd import operators

    def no_device(*args, **kwargs):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(operators._lib, "load", no_device)
    monkeypatch.setattr(torch, "empty", no_device)
    with pytest.raises(ValueError):
        operators.SpinSectorOperator(L, [(0, 1)], torch.zeros(2 + max(L, 0), dtype=torch.float64), ndown, device="cuda")


def test_python_refuses_bad_bonds_and_a_host_device():
    import torch
    from dominantsparseeigenad_amd.operators import SpinSectorOperator
    c = torch.zeros(2 * 2 + 8, dtype=torch.float64)
    with pytest.raises(ValueError):
        SpinSectorOperator(8, [(0, 1), (4, 4)], c, 4, device="cuda")
    with pytest.raises(ValueError):
        SpinSectorOperator(8, [(0, 1), (4, 8)], c, 4, device="cuda")
    with pytest.raises(ValueError):
        SpinSectorOperator(8, [], c, 4, device="cuda")
    with pytest.raises(ValueError):
        SpinSectorOperator(8, [(0, 1), (4, 5)], c, 4, device="cpu")


def flat(bonds):
    return (c_int32 * (2 * len(bonds)))(*[s for b in bonds for s in b])


def test_sector_table_sizes_without_a_device():
    lib = _lib.load()
    n, n_lo, n_hi = c_int64(), c_int64(), c_int64()
    for L, ndown in ((2, 1), (7, 3), (24, 12), (32, 16), (40, 2)):
        assert lib.dsea_sector_table_sizes(L, ndown, byref(n), byref(n_lo), byref(n_hi)) == 0
        Llo = (L + 1) // 2
        assert (n.value, n_lo.value, n_hi.value) == (math.comb(L, ndown), 1 << Llo, 1 << (L - Llo)), (L, ndown)
    for L, ndown in ((1, 1), (41, 20), (8, 0), (8, 8), (8, -1), (34, 17), (40, 20), (35, 15)):
        assert lib.dsea_sector_table_sizes(L, ndown, byref(n), byref(n_lo), byref(n_hi)) == _lib.ERR_ARG, (L, ndown)
    assert lib.dsea_sector_table_sizes(33, 16, byref(n), byref(n_lo), byref(n_hi)) == 0      # the largest sector below 2^31
    assert n.value == math.comb(33, 16) == 1166803110 and math.comb(35, 15) > 2 ** 31 - 1
    assert lib.dsea_sector_table_sizes(8, 4, None, byref(n_lo), byref(n_hi)) == _lib.ERR_ARG
    assert lib.dsea_sector_table_sizes(8, 4, byref(n), None, byref(n_hi)) == _lib.ERR_ARG
    assert lib.dsea_sector_table_sizes(8, 4, byref(n), byref(n_lo), None) == _lib.ERR_ARG
    cnt = c_int64()
    assert lib.dsea_op_sector_forms_scratch_doubles(24, 12, 48, byref(cnt)) == 0
    assert cnt.value == (2 * 48 + 24) * 4096
    assert lib.dsea_op_sector_forms_scratch_doubles(7, 3, 4, byref(cnt)) == 0 and cnt.value == 2 * 4 + 7
    assert lib.dsea_op_sector_forms_scratch_doubles(40, 20, 4, byref(cnt)) == _lib.ERR_ARG
    assert lib.dsea_op_sector_forms_scratch_doubles(7, 3, 129, byref(cnt)) == _lib.ERR_ARG
    assert lib.dsea_op_sector_forms_scratch_doubles(7, 3, 4, None) == _lib.ERR_ARG


def test_create_sector_validates_before_any_device_work():
    lib = _lib.load()
    cap = _lib.LATTICE_MAX_BONDS
    h = c_void_p()
    dummy = (ctypes.c_double * (2 * (cap + 1) + 40))()
    ptr = ctypes.cast(dummy, c_void_p)
    good = [(0, 1), (9, 3), (3, 9), (0, 1)]

    def create(L, ndown, nb, bonds, c=ptr, states=ptr, lo=ptr, hi=ptr, out=byref(h)):
        return lib.dsea_op_create_sector(L, ndown, nb, bonds, c, states, lo, hi, out)

    assert create(1, 1, 1, flat([(0, 1)])) == -1                    # L < 2
    assert create(41, 2, 1, flat([(0, 1)])) == -1                   # L > 40
    assert create(10, 0, 4, flat(good)) == -1                       # ndown < 1
    assert create(10, 10, 4, flat(good)) == -1                      # ndown > L - 1
    assert create(34, 17, 4, flat(good)) == -1                      # n > 2^31 - 1
    assert create(40, 20, 4, flat(good)) == -1
    assert create(10, 5, 0, flat(good)) == -1                       # nb < 1
    many = [(i % 9, 9) for i in range(cap + 1)]
    assert create(10, 5, cap + 1, flat(many)) == -1                 # nb above the cap
    assert create(10, 5, 2, flat([(0, 1), (2, 10)])) == -1          # site out of range
    assert create(10, 5, 2, flat([(0, 1), (-1, 2)])) == -1
    assert create(10, 5, 2, flat([(0, 1), (4, 4)])) == -1           # a == b
    assert create(10, 5, 4, None) == -1                             # null pointers, one at a time
    assert create(10, 5, 4, flat(good), c=None) == -1
    assert create(10, 5, 4, flat(good), states=None) == -1
    assert create(10, 5, 4, flat(good), lo=None) == -1
    assert create(10, 5, 4, flat(good), hi=None) == -1
    assert create(10, 5, 4, flat(good), out=None) == -1
    assert create(10, 5, cap, flat(many[:cap])) == 0                # the cap itself is accepted
    assert lib.dsea_op_destroy(h) == 0
    assert create(10, 5, 4, flat(good)) == 0                        # nothing is launched at creation
    n = c_int64()
    assert lib.dsea_op_dim(h, byref(n)) == 0 and n.value == 252
    assert lib.dsea_op_set_tuning(h, _lib.TUNE_TFIM_TILE_LOG2, 6) == 0       # this kind: log2 of the grid cap
    assert lib.dsea_op_set_tuning(h, _lib.TUNE_TFIM_TILE_LOG2, 13) == -1
    # the forms and the table fill refuse null operands on the host; the forms refuse other kinds, and the other forms this kind
    assert lib.dsea_op_sector_forms(h, None, None, None, None, None) == -1
    assert lib.dsea_op_sector_forms(None, ptr, ptr, ptr, ptr, None) == -1
    assert lib.dsea_op_lattice_forms(h, ptr, ptr, ptr, ptr, None) == _lib.ERR_ARG
    assert lib.dsea_op_destroy(h) == 0
    assert lib.dsea_op_create_lattice(10, 1, flat([(0, 1)]), ptr, byref(h)) == 0
    assert lib.dsea_op_sector_forms(h, ptr, ptr, ptr, ptr, None) == _lib.ERR_ARG
    assert lib.dsea_op_destroy(h) == 0
    assert lib.dsea_sector_build_tables(10, 5, None, ptr, ptr, None) == -1
    assert lib.dsea_sector_build_tables(10, 5, ptr, None, ptr, None) == -1
    assert lib.dsea_sector_build_tables(10, 5, ptr, ptr, None, None) == -1
    assert lib.dsea_sector_build_tables(40, 20, ptr, ptr, ptr, None) == -1
