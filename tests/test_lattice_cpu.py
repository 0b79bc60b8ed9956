"""XYZ spins on a bond list without a GPU: the three statements of tests/lattice_reference.py against each other (the row
formula the HIP kernels implement == the Kronecker build; the form sums == v1^T (dH/dp) v2), ring bonds against the chain
reference, the pure-Python bond builders, and the argument validation of the new C-ABI entry points, which runs before any
device work."""
import ctypes
from ctypes import byref, c_int32, c_void_p

import numpy as np
import pytest

import chain_reference
import lattice_reference as ref
from dominantsparseeigenad_amd import _lib
from dominantsparseeigenad_amd.synthetic import normal_vector

SIZES = list(range(2, 9))


def bonds_for(L):
    """random pairs, plus one pair reversed and one repeated (at L = 2 every pair is (0, 1) or (1, 0))"""
    bonds = ref.random_bonds(L, L + 2, 40 + L)
    a, b = bonds[0]
    return bonds + [(b, a), bonds[1]]


def params(L, bonds, seed):
    return normal_vector(ref.nparam(L, bonds), seed)


@pytest.mark.parametrize("L", SIZES)
def test_row_formula_equals_the_kronecker_build(L):
    bonds = bonds_for(L)
    p = params(L, bonds, 100 + L)
    H = ref.dense(L, bonds, p)
    assert np.array_equal(H, H.T)
    x = normal_vector(1 << L, 200 + L)
    y, want = ref.apply(L, bonds, p, x), H @ x
    assert np.max(np.abs(y - want)) <= 1e-14 * np.linalg.norm(H, 1) * np.max(np.abs(x))
    # and column by column: the same matrix, not only the same product
    eye = np.eye(1 << L)
    M = np.stack([ref.apply(L, bonds, p, eye[:, j]) for j in range(1 << L)], axis=1)
    # (an entry is a sum of at most nparam couplings, formed in two orders: twice the bound of a recursive sum)
    assert np.max(np.abs(M - H)) <= 2 * p.size * np.finfo(float).eps * np.abs(p).sum()


@pytest.mark.parametrize("L", SIZES)
def test_ring_bonds_give_the_chain_matrix(L):
    from dominantsparseeigenad_amd.operators import ring_bonds
    bonds = ring_bonds(L)
    assert len(bonds) == L                                     # L = 2: (0, 1) and (1, 0), the double bond
    c = normal_vector(5 * L, 300 + L).reshape(5, L)
    want = chain_reference.dense(L, c)
    got = ref.dense(L, bonds, c.reshape(-1))                   # nb = L: the flat order is the chain's (5, L) row by row
    assert np.max(np.abs(got - want)) <= 1e-15 * max(1.0, np.max(np.abs(want)))
    x = normal_vector(1 << L, 350 + L)
    got_x, want_x = ref.apply(L, bonds, c.reshape(-1), x), chain_reference.apply(L, c, x)
    assert np.max(np.abs(got_x - want_x)) <= 1e-13 * np.abs(c).sum() * np.max(np.abs(x))


@pytest.mark.parametrize("L", SIZES)
def test_forms_equal_the_bilinear_forms_of_the_dense_terms(L):
    bonds = bonds_for(L)
    v1, v2 = normal_vector(1 << L, 400 + L), normal_vector(1 << L, 500 + L)
    got = ref.forms(L, bonds, v1, v2)
    terms = ref.dense_terms(L, bonds)
    assert got.shape == (3 * len(bonds) + 2 * L,) and len(terms) == got.size
    bound = 1e-13 * np.linalg.norm(v1) * np.linalg.norm(v2)
    for t, term in enumerate(terms):
        assert abs(got[t] - v1 @ (term @ v2)) <= bound, t
    # H is linear in the couplings: v1^T H[p] v2 = sum_t p_t forms_t
    p = params(L, bonds, 600 + L)
    scale = np.linalg.norm(v1) * np.linalg.norm(v2) * np.abs(p).sum()
    assert abs(v1 @ ref.apply(L, bonds, p, v2) - np.sum(p * got)) <= 1e-12 * scale


def test_bond_builders():
    from dominantsparseeigenad_amd.operators import ring_bonds, square_bonds
    assert ring_bonds(6, 2) == [(i, (i + 2) % 6) for i in range(6)]
    assert ring_bonds(2) == [(0, 1), (1, 0)]
    sq = square_bonds(3, 3)
    assert len(sq) == 18
    assert all(0 <= a < 9 and 0 <= b < 9 and a != b for a, b in sq)
    # every site of the torus has four neighbours; site = y * Lx + x
    degree = np.zeros(9, dtype=int)
    for a, b in sq:
        degree[a] += 1
        degree[b] += 1
        dx, dy = (b % 3 - a % 3) % 3, (b // 3 - a // 3) % 3
        assert (dx, dy) in ((1, 0), (0, 1))
    assert np.all(degree == 4)
    assert len(square_bonds(3, 3, periodic=(False, False))) == 12
    assert len(square_bonds(4, 5)) == 40 and len(square_bonds(4, 5, periodic=(True, False))) == 36
    # a periodic direction of length 2 lists its bond twice (the TFIM convention)
    assert sorted(tuple(sorted(b)) for b in square_bonds(2, 1)) == [(0, 1), (0, 1)]
    assert square_bonds(2, 1, periodic=(False, False)) == [(0, 1)]
    with pytest.raises(ValueError):
        ring_bonds(4, 4)


def flat(bonds):
    return (c_int32 * (2 * len(bonds)))(*[s for b in bonds for s in b])


def test_create_lattice_validates_before_any_device_work():
    lib = _lib.load()
    assert lib.dsea_version() >= 143
    cap = _lib.LATTICE_MAX_BONDS
    assert cap >= 128
    h = c_void_p()
    dummy = (ctypes.c_double * (3 * (cap + 1) + 2 * 62))()
    ptr = ctypes.cast(dummy, c_void_p)
    good = [(0, 1), (9, 3), (3, 9), (0, 1)]
    assert lib.dsea_op_create_lattice(1, 1, flat([(0, 1)]), ptr, byref(h)) == -1          # L < 2
    assert lib.dsea_op_create_lattice(63, 1, flat([(0, 1)]), ptr, byref(h)) == -1         # L > 62
    assert lib.dsea_op_create_lattice(10, 0, flat(good), ptr, byref(h)) == -1             # nb < 1
    many = [(i % 9, 9) for i in range(cap + 1)]
    assert lib.dsea_op_create_lattice(10, cap + 1, flat(many), ptr, byref(h)) == -1       # nb above the cap
    assert lib.dsea_op_create_lattice(10, 2, flat([(0, 1), (2, 10)]), ptr, byref(h)) == -1   # site out of range
    assert lib.dsea_op_create_lattice(10, 2, flat([(0, 1), (-1, 2)]), ptr, byref(h)) == -1
    assert lib.dsea_op_create_lattice(10, 2, flat([(0, 1), (4, 4)]), ptr, byref(h)) == -1    # a == b
    assert lib.dsea_op_create_lattice(10, 4, None, ptr, byref(h)) == -1                   # no bonds
    assert lib.dsea_op_create_lattice(10, 4, flat(good), None, byref(h)) == -1            # no couplings
    assert lib.dsea_op_create_lattice(10, 4, flat(good), ptr, None) == -1
    assert lib.dsea_op_create_lattice(10, cap, flat(many[:cap]), ptr, byref(h)) == 0      # the cap itself is accepted
    assert lib.dsea_op_destroy(h) == 0
    assert lib.dsea_op_create_lattice(10, 4, flat(good), ptr, byref(h)) == 0              # nothing is launched at creation
    n = ctypes.c_int64()
    assert lib.dsea_op_dim(h, byref(n)) == 0 and n.value == 1024
    assert lib.dsea_op_set_tuning(h, _lib.TUNE_TFIM_TILE_LOG2, 6) == 0
    assert lib.dsea_op_set_tuning(h, _lib.TUNE_TFIM_TILE_LOG2, 5) == -1
    # the forms refuse null operands on the host
    assert lib.dsea_op_lattice_forms(h, None, None, None, None, None) == -1
    assert lib.dsea_op_lattice_forms(None, ptr, ptr, ptr, ptr, None) == -1
    assert lib.dsea_op_destroy(h) == 0


def test_lattice_forms_refuses_other_operator_kinds():
    lib = _lib.load()
    h = c_void_p()
    assert lib.dsea_op_create_tfim(10, 10, 0, None, 1.0, 1.0, byref(h)) == 0
    buf = (ctypes.c_double * 64)()
    ptr = ctypes.cast(buf, c_void_p)
    assert lib.dsea_op_lattice_forms(h, ptr, ptr, ptr, ptr, None) == _lib.ERR_ARG
    assert lib.dsea_op_destroy(h) == 0
    # and the chain's forms refuse a lattice handle
    assert lib.dsea_op_create_lattice(10, 1, flat([(0, 1)]), ptr, byref(h)) == 0
    assert lib.dsea_op_chain_forms(h, ptr, ptr, ptr, ptr, None) == _lib.ERR_ARG
    assert lib.dsea_op_destroy(h) == 0


def test_forms_scratch_size():
    lib = _lib.load()
    need = ctypes.c_int64()
    assert lib.dsea_op_lattice_forms_scratch_doubles(1, 1, byref(need)) == -1
    assert lib.dsea_op_lattice_forms_scratch_doubles(63, 1, byref(need)) == -1
    assert lib.dsea_op_lattice_forms_scratch_doubles(10, 0, byref(need)) == -1
    assert lib.dsea_op_lattice_forms_scratch_doubles(10, _lib.LATTICE_MAX_BONDS + 1, byref(need)) == -1
    assert lib.dsea_op_lattice_forms_scratch_doubles(10, 4, None) == -1
    # (3 nb + 2 L) forms x the most blocks any tile tuning launches: min(4096, 2^max(L - 6, 0))
    for L, nb in ((2, 1), (7, 5), (13, 40), (19, 128), (40, 128)):
        assert lib.dsea_op_lattice_forms_scratch_doubles(L, nb, byref(need)) == 0
        assert need.value == (3 * nb + 2 * L) * min(4096, 2 ** max(L - 6, 0)), (L, nb, need.value)
