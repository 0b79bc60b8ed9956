"""numpy reference of the XXZ spins with a coupling on every pair of sites in one magnetisation sector
(docs/design/22-pair-sector.md); no GPU, no torch, and nothing of size 2^L, so it also works at L = 40.

    H = sum_{i<j} [Jxy_ij (X_i X_j + Y_i Y_j) + Jz_ij Z_i Z_j] + sum_i hz_i Z_i

restricted to the states with exactly ``ndown`` set bits.  Site i is bit i of the state s, z_i(s) = 1 - 2 bit_i(s); row r is the
r-th such state in increasing integer order.  ``p`` is the flat parameter [Jxy(P), Jz(P), hz(L)], P = L (L - 1) / 2, the pairs in
lexicographic order (0,1), (0,2), ..., (0,L-1), (1,2), ...

    pairs(L), pair_index(L, i, j)       the pair list and p(i, j) = i (2 L - i - 1) / 2 + (j - i - 1)
    states(L, ndown)                    the sorted states, from itertools.combinations
    apply(L, ndown, p, x)               the row formula, row by row from the bits
    forms(L, ndown, v1, v2)             the 2 P + L sums v1^T (dH/dp_t) v2 written out, in the order of p
    dense(L, ndown, p)                  the matrix, for small n
    haldane_shastry(L)                  the parameter of the Haldane-Shastry ring, and its closed-form ground-state energy

Written from the formula alone: it shares no code with tests/sector_reference.py, against which test_pairsector_cpu.py checks
it with the bond list "all pairs".
"""
import functools
import itertools
import math

import numpy as np


def npair(L):
    return L * (L - 1) // 2


def nparam(L):
    return 2 * npair(L) + L


@functools.lru_cache(maxsize=None)
def pairs(L):
    return tuple((i, j) for i in range(L) for j in range(i + 1, L))


def pair_index(L, i, j):
    if i > j:
        i, j = j, i
    return i * (2 * L - i - 1) // 2 + (j - i - 1)


def split(L, p):
    """(Jxy, Jz, hz) views of the flat parameter"""
    P = npair(L)
    p = np.asarray(p, dtype=np.float64).reshape(nparam(L))
    return p[:P], p[P:2 * P], p[2 * P:]


@functools.lru_cache(maxsize=None)
def states(L, ndown):
    """the states as a sorted tuple of Python ints"""
    return tuple(sorted(sum(1 << i for i in sites) for sites in itertools.combinations(range(L), ndown)))


@functools.lru_cache(maxsize=None)
def _geometry(L, ndown):
    """(bits, rows, cols): bits[r, i] = bit i of state r; per pair the rows whose two bits differ and the rows of their partner
    states, found by sorting -- never written to"""
    words = np.array(states(L, ndown), dtype=np.int64)
    bits = np.stack([(words >> i) & 1 for i in range(L)], axis=1)
    rows, cols = [], []
    for i, j in pairs(L):
        r = np.nonzero(bits[:, i] != bits[:, j])[0]
        partner = words[r] ^ ((1 << i) | (1 << j))
        c = np.searchsorted(words, partner)
        assert np.array_equal(words[c], partner)
        for a in (r, c):
            a.setflags(write=False)
        rows.append(r)
        cols.append(c)
    bits.setflags(write=False)
    return bits, tuple(rows), tuple(cols)


def apply(L, ndown, p, x):
    """(H x)[r] = (sum_{i<j} Jz_ij z_i z_j + sum_i hz_i z_i) x[r] + sum_{i<j: bits differ} 2 Jxy_ij x[rank(s_r ^ m_ij)]"""
    jxy, jz, hz = split(L, p)
    x = np.asarray(x, dtype=np.float64)
    bits, rows, cols = _geometry(L, ndown)
    z = 1.0 - 2.0 * bits
    diag = z @ hz
    y = np.zeros(x.size)
    for t, (i, j) in enumerate(pairs(L)):
        diag = diag + jz[t] * (z[:, i] * z[:, j])
        y[rows[t]] += 2.0 * jxy[t] * x[cols[t]]
    return y + diag * x


def forms(L, ndown, v1, v2):
    """out[t] = v1^T (dH/dp_t) v2, shape (2 P + L,)"""
    v1, v2 = np.asarray(v1, dtype=np.float64), np.asarray(v2, dtype=np.float64)
    bits, rows, cols = _geometry(L, ndown)
    z = 1.0 - 2.0 * bits
    P = npair(L)
    out = np.zeros(nparam(L))
    w = v1 * v2
    for t, (i, j) in enumerate(pairs(L)):
        out[t] = np.sum(2.0 * v1[rows[t]] * v2[cols[t]])
        out[P + t] = np.sum(z[:, i] * z[:, j] * w)
    out[2 * P:] = w @ z
    return out


def dense(L, ndown, p):
    n = len(states(L, ndown))
    H = np.zeros((n, n))
    for c in range(n):
        e = np.zeros(n)
        e[c] = 1.0
        H[:, c] = apply(L, ndown, p, e)
    return H


def pack_matrices(L, Jxy, Jz, hz):
    """the flat parameter of two L x L matrices (strict upper triangle read) and a length-L field"""
    Jxy, Jz = np.asarray(Jxy, dtype=np.float64), np.asarray(Jz, dtype=np.float64)
    return np.concatenate([[Jxy[i, j] for i, j in pairs(L)], [Jz[i, j] for i, j in pairs(L)], np.asarray(hz, dtype=np.float64)])


def haldane_shastry(L):
    """(p, E0): Jxy_ij = Jz_ij = (pi / L)^2 / (4 sin^2(pi (i - j) / L)), hz = 0, i.e. H = sum_{i<j} J_ij S_i . S_j with
    J_ij = (pi / L)^2 / sin^2(pi (i - j) / L); ground-state energy of the S^z = 0 sector (L even): -pi^2 (L + 5 / L) / 24"""
    J = np.zeros((L, L))
    for i, j in pairs(L):
        J[i, j] = (math.pi / L) ** 2 / (4.0 * math.sin(math.pi * (i - j) / L) ** 2)
    return pack_matrices(L, J, J, np.zeros(L)), -math.pi ** 2 * (L + 5.0 / L) / 24.0
