"""The numpy reference of the reduced density matrix (tests/rdm_reference.py) against the partial trace of the embedded 2^L
vector, the case table of tests/test_gpu_rdm.py against its own description, and the host arithmetic of the C ABI
(dsea_rdm_sizes / dsea_rdm_scratch_doubles: block structure and every refused argument) -- no GPU."""
import math
from ctypes import byref, c_int, c_int32, c_int64

import numpy as np
import pytest

import rdm_reference as ref
from dominantsparseeigenad_amd import _lib
from dominantsparseeigenad_amd.synthetic import normal_vector


@pytest.mark.parametrize("L,ndown,sites", ref.TRACE_CASES)
def test_blocks_are_the_diagonal_blocks_of_the_partial_trace(L, ndown, sites):
    LA = len(sites)
    x = normal_vector(math.comb(L, ndown), 5100 + L)
    x = x / np.linalg.norm(x)
    rho = ref.partial_trace(L, sites, ref.embed(L, ndown, x))
    assert rho.shape == (1 << LA, 1 << LA)
    rest = rho.copy()
    got = ref.cross(L, ndown, sites, x, x)
    worst = 0.0
    for (m, dA, dB), block in zip(ref.blocks(L, ndown, sites), got):
        rows = ref.block_rows(LA, m)
        assert block.shape == (dA, dA) and rows.size == dA
        worst = max(worst, float(np.max(np.abs(rho[np.ix_(rows, rows)] - block))))
        rest[np.ix_(rows, rows)] = 0.0
    print("L = %d, ndown = %d, sites %s: max |block - partial trace| = %.1e" % (L, ndown, sites, worst))
    assert worst < 1e-15                                 # (a few roundings of sums of products of a unit vector)
    assert np.all(rest == 0.0)                           # outside the blocks, and in the blocks no sector state reaches: exactly 0
    assert abs(sum(np.trace(b) for b in got) - 1.0) < 1e-14


@pytest.mark.parametrize("name", list(ref.CASES))
def test_the_cases_are_what_the_table_says(name):
    L, ndown, sites, n, shapes = ref.CASES[name]
    blocks = ref.blocks(L, ndown, sites)
    assert ref.dim(L, ndown) == n
    assert [(dA, dB) for _, dA, dB in blocks] == shapes
    assert sum(dA * dB for _, dA, dB in blocks) == n     # Vandermonde
    assert 1 <= len(sites) <= min(L - 1, 16) and len(set(sites)) == len(sites)


def test_the_table_reaches_what_it_claims():
    c = ref.CASES
    assert c["L7-3-unsorted"][2] != sorted(c["L7-3-unsorted"][2]) and c["L7-3-unsorted"][0] % 2 == 1
    assert ref.blocks(9, 7, c["L9-7-first-m3"][2])[0][0] == 3
    assert all(dB % 16 for _, dB in c["L9-4-one-site"][4])
    assert {15, 20} <= {dA for dA, _ in c["L12-6"][4]}
    assert len(c["L20-1-cap"][2]) == 16 and (16, 1) in c["L20-1-cap"][4]
    assert max(dA for dA, _ in c["L16-8"][4]) == 70
    assert max(dB for _, dB in c["L20-10-two-sites"][4]) == 48620
    assert max(dA for dA, _ in c["L20-10-half"][4]) == 252
    for name in ("L34-2", "L40-2"):
        assert int(ref.words(c[name][0], c[name][1]).max()) >= 1 << 32
    assert max(v[3] for v in c.values()) == 184756


@pytest.mark.parametrize("name", list(ref.CASES))
def test_the_reference_index_table_is_a_permutation(name):
    L, ndown, sites, n, _ = ref.CASES[name]
    idx = ref.index_table(L, ndown, sites)
    assert idx.shape == (n,)
    assert np.array_equal(np.sort(idx), np.arange(n))


def test_a_contiguous_low_subsystem_of_the_full_space_is_a_reshape():
    L, _, sites, n, _ = ref.CASES["full-L10-contiguous"]
    x = normal_vector(n, 5200)
    M = x.reshape(1 << 5, 1 << 5).T                      # state = a + 32 b: rows a, columns b
    assert np.array_equal(ref.slices(L, None, sites, x)[0], M)


def sizes(L, ndown, sites):
    lib = _lib.load()
    arr = (c_int32 * max(len(sites), 1))(*sites)
    n, nblk, out_len, need = c_int64(), c_int(), c_int64(), c_int64()
    table = (c_int64 * (5 * _lib.RDM_MAX_BLOCKS))()
    status = lib.dsea_rdm_sizes(L, -1 if ndown is None else ndown, len(sites), arr, byref(n), byref(nblk), table, byref(out_len))
    status2 = lib.dsea_rdm_scratch_doubles(L, -1 if ndown is None else ndown, len(sites), arr, byref(need))
    assert (status == 0) == (status2 == 0)
    rows = [tuple(table[5 * c + e] for e in range(5)) for c in range(nblk.value)] if status == 0 else []
    return status, n.value, out_len.value, rows, need.value


@pytest.mark.parametrize("name", list(ref.CASES))
def test_the_library_sizes_are_the_reference_blocks(name):
    L, ndown, sites, n, _ = ref.CASES[name]
    status, got_n, out_len, rows, need = sizes(L, ndown, sites)
    assert status == 0 and got_n == n
    blocks = ref.blocks(L, ndown, sites)
    assert [r[:3] for r in rows] == [tuple(b) for b in blocks]
    assert [r[3] for r in rows] == list(np.cumsum([0] + [dA * dB for _, dA, dB in blocks])[:-1])
    assert [r[4] for r in rows] == list(np.cumsum([0] + [dA * dA for _, dA, _ in blocks])[:-1])
    assert out_len == sum(dA * dA for _, dA, _ in blocks)
    assert need >= 256                                   # at least one partial tile


@pytest.mark.parametrize("L,ndown,sites", [
    (8, 4, [0, 0]),                 # a site repeated
    (8, 4, [8]), (8, 4, [-1]),      # a site out of range
    (8, 4, []), (8, 4, list(range(8))), (20, 10, list(range(17))),     # LA outside 1 .. min(L - 1, 16)
    (20, None, list(range(16))),    # a flat output of 2^32 elements
    (34, 17, [0]), (41, 1, [0]), (8, 0, [0]), (8, 8, [0]), (8, -2, [0]),   # the sector limits
    (31, None, [0]),                # the full space beyond L = 30
])
def test_refused_arguments_return_err_arg_from_host_arithmetic(L, ndown, sites):
    assert sizes(L, ndown, sites)[0] == _lib.ERR_ARG
