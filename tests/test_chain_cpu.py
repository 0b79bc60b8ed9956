"""The XYZ spin chain without a GPU: the three statements of tests/chain_reference.py against each other (the row formula the
HIP kernels implement == the Kronecker build; the form sums == v1^T (dH/dp) v2), the TFIM special case against the oracle,
and the argument validation of the new C-ABI entry points, which runs before any device work."""
import ctypes
from ctypes import byref, c_void_p

import numpy as np
import pytest

import chain_reference as ref
from dominantsparseeigenad_amd import _lib
from dominantsparseeigenad_amd.synthetic import normal_vector

SIZES = list(range(2, 9))


def couplings(L, seed):
    return normal_vector(5 * L, seed).reshape(5, L)


@pytest.mark.parametrize("L", SIZES)
def test_row_formula_equals_the_kronecker_build(L):
    c = couplings(L, 100 + L)
    H = ref.dense(L, c)
    assert np.array_equal(H, H.T)
    x = normal_vector(1 << L, 200 + L)
    y, want = ref.apply(L, c, x), H @ x
    assert np.max(np.abs(y - want)) <= 1e-14 * np.linalg.norm(H, 1) * np.max(np.abs(x))
    # and column by column: the same matrix, not only the same product
    eye = np.eye(1 << L)
    M = np.stack([ref.apply(L, c, eye[:, j]) for j in range(1 << L)], axis=1)
    assert np.max(np.abs(M - H)) <= 1e-15 * max(1.0, np.max(np.abs(H)))


@pytest.mark.parametrize("L", SIZES)
def test_tfim_couplings_give_the_oracle_matrix(L):
    import oracle.operators
    g = 0.7 + 0.1 * L
    want = oracle.operators.TFIMTables(L, g).dense().numpy()
    c = ref.tfim_couplings(L, g)
    assert np.max(np.abs(ref.dense(L, c) - want)) <= 1e-15
    x = normal_vector(1 << L, 300 + L)
    assert np.max(np.abs(ref.apply(L, c, x) - want @ x)) <= 1e-13 * np.max(np.abs(x)) * (L + g * L)


@pytest.mark.parametrize("L", SIZES)
def test_forms_equal_the_bilinear_forms_of_the_dense_terms(L):
    v1, v2 = normal_vector(1 << L, 400 + L), normal_vector(1 << L, 500 + L)
    got = ref.forms(L, v1, v2)
    terms = ref.dense_terms(L)
    bound = 1e-13 * np.linalg.norm(v1) * np.linalg.norm(v2)
    for f in range(5):
        for i in range(L):
            assert abs(got[f, i] - v1 @ (terms[f][i] @ v2)) <= bound, (f, i)
    # H is linear in the couplings: v1^T H[c] v2 = sum_t c_t forms_t
    c = couplings(L, 600 + L)
    assert abs(v1 @ ref.apply(L, c, v2) - np.sum(c * got)) <= 1e-12 * np.linalg.norm(v1) * np.linalg.norm(v2) * np.abs(c).sum()


def test_open_chain_is_a_zero_last_bond():
    L = 5
    c = couplings(L, 700)
    c[:3, L - 1] = 0.0
    H = ref.dense(L, c)
    # no matrix element between rows that differ in sites L-1 and 0 only
    s = np.arange(1 << L)
    assert np.all(H[s, s ^ ((1 << (L - 1)) | 1)] == 0.0)


def test_create_chain_validates_before_any_device_work():
    lib = _lib.load()
    h = c_void_p()
    dummy = (ctypes.c_double * 50)()
    ptr = ctypes.cast(dummy, c_void_p)
    assert lib.dsea_op_create_chain(1, ptr, byref(h)) == -1            # L < 2
    assert lib.dsea_op_create_chain(63, ptr, byref(h)) == -1           # L > 62
    assert lib.dsea_op_create_chain(10, None, byref(h)) == -1          # no couplings
    assert lib.dsea_op_create_chain(10, ptr, None) == -1
    assert lib.dsea_op_create_chain(10, ptr, byref(h)) == 0            # nothing is launched at creation
    n = ctypes.c_int64()
    assert lib.dsea_op_dim(h, byref(n)) == 0 and n.value == 1024
    assert lib.dsea_op_set_tuning(h, _lib.TUNE_TFIM_TILE_LOG2, 6) == 0
    assert lib.dsea_op_set_tuning(h, _lib.TUNE_TFIM_TILE_LOG2, 5) == -1
    # the forms refuse null operands on the host
    assert lib.dsea_op_chain_forms(h, None, None, None, None, None) == -1
    assert lib.dsea_op_destroy(h) == 0


def test_chain_forms_refuses_other_operator_kinds():
    lib = _lib.load()
    h = c_void_p()
    assert lib.dsea_op_create_tfim(10, 10, 0, None, 1.0, 1.0, byref(h)) == 0
    buf = (ctypes.c_double * 64)()
    ptr = ctypes.cast(buf, c_void_p)
    assert lib.dsea_op_chain_forms(h, ptr, ptr, ptr, ptr, None) == _lib.ERR_ARG
    assert lib.dsea_op_destroy(h) == 0


def test_forms_scratch_size():
    lib = _lib.load()
    need = ctypes.c_int64()
    assert lib.dsea_op_chain_forms_scratch_doubles(1, byref(need)) == -1
    assert lib.dsea_op_chain_forms_scratch_doubles(63, byref(need)) == -1
    assert lib.dsea_op_chain_forms_scratch_doubles(10, None) == -1
    # 5 L forms x the most blocks any tile tuning launches (tiles of 2^6 rows, at most 4096 blocks)
    for L, blocks in ((2, 1), (6, 1), (7, 2), (13, 128), (19, 4096), (40, 4096)):
        assert lib.dsea_op_chain_forms_scratch_doubles(L, byref(need)) == 0
        assert need.value == 5 * L * blocks, (L, need.value)
