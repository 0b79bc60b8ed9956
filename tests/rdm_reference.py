"""numpy reference of the reduced density matrix of a bipartition (docs/design/21-reduced-density-matrix.md), written from the
definitions; no GPU, no torch, no library.

Site i is bit i of a state.  ``sites`` lists the LA sites of A in the caller's order: bit k of the A-word a is the bit of site
sites[k].  B is the other LB = L - LA sites in increasing order; bit k of the B-word b is the bit of site B[k].  A sector vector
has one entry per state with ``ndown`` set bits in increasing integer order; ``ndown=None`` is the full 2^L space (row = state).
Block m (m set bits inside A) has row i = the i-th LA-bit word with m set bits in increasing order and column j = the j-th
LB-bit word with ndown - m set bits;

    M_m(x)[i, j] = x[row(dep_A(a_i) | dep_B(b_j))]      cross(x, y)_m = M_m(x) M_m(y)^T      rho_m = cross(psi, psi)_m

    words(W, k)                       the W-bit words with k set bits, increasing (int64 array)
    blocks(L, ndown, sites)           ((m, dA, dB), ...)
    index_blocks(L, ndown, sites)     per block the (dA, dB) array of rows: M_m(x) = x[index]
    index_table(L, ndown, sites)      the same, flattened block after block (j fastest)
    slices / cross / pull             the definitions on those arrays
    embed / partial_trace             the 2^L vector of a sector vector and its dense 2^LA x 2^LA reduced density matrix
"""
import functools
import math

import numpy as np


@functools.lru_cache(maxsize=None)
def words(W, k):
    """the W-bit words with k set bits in increasing integer order"""
    if k < 0 or k > W:
        return _frozen(np.zeros(0, dtype=np.int64))
    if k == 0:
        return _frozen(np.zeros(1, dtype=np.int64))
    if W == k:
        return _frozen(np.array([(1 << W) - 1], dtype=np.int64))
    return _frozen(np.concatenate([words(W - 1, k), words(W - 1, k - 1) | (1 << (W - 1))]))


def _frozen(a):
    a.setflags(write=False)
    return a


def complement(L, sites):
    inside = set(int(s) for s in sites)
    return [i for i in range(L) if i not in inside]


def deposit(w, positions):
    """bit k of every word of w moved to bit positions[k]"""
    w = np.asarray(w, dtype=np.int64)
    out = np.zeros_like(w)
    for k, pos in enumerate(positions):
        out |= ((w >> k) & 1) << int(pos)
    return out


def dim(L, ndown):
    return 1 << L if ndown is None else math.comb(L, ndown)


def blocks(L, ndown, sites):
    LA = len(sites)
    LB = L - LA
    if ndown is None:
        return ((0, 1 << LA, 1 << LB),)
    return tuple((m, math.comb(LA, m), math.comb(LB, ndown - m)) for m in range(max(0, ndown - LB), min(LA, ndown) + 1))


def _key(sites):
    return tuple(int(s) for s in sites)


def index_blocks(L, ndown, sites):
    return _index_blocks(L, ndown, _key(sites))


@functools.lru_cache(maxsize=None)
def _index_blocks(L, ndown, sites):
    LA = len(sites)
    B = complement(L, sites)
    out = []
    if ndown is None:
        a = deposit(np.arange(1 << LA, dtype=np.int64), sites)
        b = deposit(np.arange(1 << (L - LA), dtype=np.int64), B)
        out.append(_frozen(a[:, None] | b[None, :]))
        return tuple(out)
    states = words(L, ndown)
    for m, dA, dB in blocks(L, ndown, sites):
        a = deposit(words(LA, m), sites)
        b = deposit(words(L - LA, ndown - m), B)
        assert a.size == dA and b.size == dB
        s = a[:, None] | b[None, :]
        rows = np.searchsorted(states, s)
        assert np.array_equal(states[rows], s)
        out.append(_frozen(rows.astype(np.int64)))
    return tuple(out)


def index_table(L, ndown, sites):
    return np.concatenate([ix.reshape(-1) for ix in index_blocks(L, ndown, sites)])


def slices(L, ndown, sites, x):
    x = np.asarray(x, dtype=np.float64)
    return [x[ix] for ix in index_blocks(L, ndown, sites)]


def cross(L, ndown, sites, x, y):
    return [a @ b.T for a, b in zip(slices(L, ndown, sites, x), slices(L, ndown, sites, y))]


def cross_abs(L, ndown, sites, x, y):
    """(|M(x)| |M(y)|^T) per block: the scale of the rounding bound of a cross product"""
    return [np.abs(a) @ np.abs(b).T for a, b in zip(slices(L, ndown, sites, x), slices(L, ndown, sites, y))]


def pull(L, ndown, sites, G, y, transpose=False):
    """out with M_m(out) = G_m M_m(y) (G_m^T when transpose); G a list of (dA, dA) arrays"""
    out = np.zeros(dim(L, ndown))
    for ix, g, sl in zip(index_blocks(L, ndown, sites), G, slices(L, ndown, sites, y)):
        out[ix] = (g.T if transpose else g) @ sl
    return out


def pull_abs(L, ndown, sites, G, y, transpose=False):
    out = np.zeros(dim(L, ndown))
    for ix, g, sl in zip(index_blocks(L, ndown, sites), G, slices(L, ndown, sites, y)):
        out[ix] = np.abs(g.T if transpose else g) @ np.abs(sl)
    return out


def embed(L, ndown, x):
    """the sector vector as a vector of the full 2^L space"""
    w = np.zeros(1 << L)
    w[words(L, ndown)] = x
    return w


def partial_trace(L, sites, w):
    """rho_A[a, a'] = sum_b w[dep_A(a) | dep_B(b)] w[dep_A(a') | dep_B(b)] of a 2^L vector, dense 2^LA x 2^LA"""
    (ix,) = index_blocks(L, None, sites)
    M = np.asarray(w, dtype=np.float64)[ix]
    return M @ M.T


def block_rows(LA, m):
    """the rows of block m inside the dense 2^LA x 2^LA matrix: the A-words with m set bits"""
    return words(LA, m)


# The geometries of tests/test_gpu_rdm.py: name -> (L, ndown or None, sites, n, the (dA, dB) of the blocks the row is there for)
CASES = {
    # less than one tile, dB = 1
    "L2-1": (2, 1, [0], 2, [(1, 1), (1, 1)]),
    "L4-2": (4, 2, [0, 1], 6, [(1, 1), (2, 2), (1, 1)]),
    "L5-2": (5, 2, [0, 3], 10, [(1, 3), (2, 3), (1, 1)]),
    # unsorted sites, odd L
    "L7-3-unsorted": (7, 3, [6, 0, 3], 35, [(1, 4), (3, 6), (3, 4), (1, 1)]),
    # the first block is m = 3, not 0
    "L9-7-first-m3": (9, 7, [2, 3, 4, 5, 6], 36, [(10, 1), (5, 4), (1, 6)]),
    # LA = 1: 1 x 1 blocks, inner dimensions 70 and 56, no multiple of 16
    "L9-4-one-site": (9, 4, [0], 126, [(1, 70), (1, 56)]),
    # dA = 15 (one short of a tile) and 20 (one tile plus a ragged one)
    "L12-6": (12, 6, [11, 0, 5, 6, 2, 9], 924, [(1, 1), (6, 6), (15, 15), (20, 20), (15, 15), (6, 6), (1, 1)]),
    # LA at the cap, dA = 16 exactly one tile, dB = 1 and 4
    "L20-1-cap": (20, 1, list(range(16)), 20, [(1, 4), (16, 1)]),
    # dA = dB = 70 in the middle: several tiles both ways, mirrored tiles
    "L16-8": (16, 8, list(range(0, 16, 2)), 12870, [(1, 1), (8, 8), (28, 28), (56, 56), (70, 70), (56, 56), (28, 28), (8, 8),
                                                     (1, 1)]),
    # the split of the inner dimension over many waves, and the reduce
    "L20-10-two-sites": (20, 10, [0, 1], 184756, [(1, 43758), (2, 48620), (1, 43758)]),
    # dA = 252: 16 x 16 tiles of 16 per block, the compute-bound shape
    "L20-10-half": (20, 10, list(range(10)), 184756, [(math.comb(10, m), math.comb(10, m)) for m in range(11)]),
    # states wider than 32 bits
    "L34-2": (34, 2, [33, 0, 17], 561, [(1, 465), (3, 31), (3, 1)]),
    "L40-2": (40, 2, [39, 0, 20], 780, [(1, 666), (3, 37), (3, 1)]),
    # the full space: a single block
    "full-L3": (3, None, [1], 8, [(2, 4)]),
    "full-L6": (6, None, [5, 0, 2], 64, [(8, 8)]),
    "full-L10-contiguous": (10, None, list(range(5)), 1024, [(32, 32)]),
    "full-L12-odd-sites": (12, None, list(range(1, 12, 2)), 4096, [(64, 64)]),
    "full-L14-one-site": (14, None, [13], 16384, [(2, 8192)]),
}

# the seven cases in which the blocks were first checked against the partial trace of the embedded vector
TRACE_CASES = [(4, 2, [0, 1]), (7, 3, [6, 0, 3]), (8, 4, [1, 3, 5, 7]), (9, 4, [0]), (9, 7, [2, 3, 4, 5, 6]),
               (10, 5, [0, 1, 2, 3, 4]), (12, 6, [11, 0, 5, 6, 2, 9])]
