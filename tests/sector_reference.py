"""numpy reference of the XXZ spins on a caller-given bond list in one magnetisation sector (docs/design/18-spin-sector.md); no
GPU, no torch, and nothing of size 2^L, so it also works at L = 40.

    H = sum_t [Jxy_t (X_a X_b + Y_a Y_b) + Jz_t Z_a Z_b] + sum_i hz_i Z_i,   bond t joins sites a_t != b_t

restricted to the states with exactly ``ndown`` set bits.  Site i is bit i of the state s, z_i(s) = 1 - 2 bit_i(s); row r is the
r-th such state in increasing integer order.  ``p`` is the flat parameter [Jxy(nb), Jz(nb), hz(L)].

    states(L, ndown)                    the sorted states, from itertools.combinations
    apply(L, ndown, bonds, p, x)        the row formula
    forms(L, ndown, bonds, v1, v2)      the 2 nb + L sums v1^T (dH/dp_t) v2 written out, in the order of p
    dense(L, ndown, bonds, p)           the matrix, for small n
    full_parameter(L, bonds, p)         the same couplings as the parameter of lattice_reference (Jx = Jy = Jxy, hx = 0)
"""
import functools
import itertools

import numpy as np


def nparam(L, bonds):
    return 2 * len(bonds) + L


def split(L, bonds, p):
    """(Jxy, Jz, hz) views of the flat parameter"""
    nb = len(bonds)
    p = np.asarray(p, dtype=np.float64).reshape(nparam(L, bonds))
    return p[:nb], p[nb:2 * nb], p[2 * nb:]


@functools.lru_cache(maxsize=None)
def states(L, ndown):
    """the states as a sorted tuple of Python ints"""
    return tuple(sorted(sum(1 << i for i in sites) for sites in itertools.combinations(range(L), ndown)))


@functools.lru_cache(maxsize=None)
def rank(L, ndown):
    """state -> row, a dictionary"""
    return {s: r for r, s in enumerate(states(L, ndown))}


def _partners(L, ndown, bonds):
    """per bond: (rows whose two bits differ, the rows of their partner states, zz_t as a vector over the rows); computed once
    per (L, ndown, bond list) and never written to"""
    return _partners_cached(L, ndown, tuple((int(a), int(b)) for a, b in bonds))


@functools.lru_cache(maxsize=None)
def _partners_cached(L, ndown, bonds):
    st, rk = states(L, ndown), rank(L, ndown)
    words = np.array(st, dtype=np.int64)
    out = []
    for a, b in bonds:
        m = (1 << a) | (1 << b)
        differ = ((words >> a) ^ (words >> b)) & 1 == 1
        rows = np.nonzero(differ)[0]
        cols = np.array([rk[st[r] ^ m] for r in rows], dtype=np.int64)
        zz = np.where(differ, -1.0, 1.0)
        for arr in (rows, cols, zz):
            arr.setflags(write=False)
        out.append((rows, cols, zz))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _z(L, ndown):
    words = np.array(states(L, ndown), dtype=np.int64)
    out = tuple(1.0 - 2.0 * ((words >> i) & 1) for i in range(L))
    for arr in out:
        arr.setflags(write=False)
    return out


def apply(L, ndown, bonds, p, x):
    """(H x)[r] = (sum_t Jz_t zz_t + sum_i hz_i z_i) x[r] + sum_{t: bits differ} 2 Jxy_t x[rank(s_r ^ m_t)]"""
    jxy, jz, hz = split(L, bonds, p)
    x = np.asarray(x, dtype=np.float64)
    diag = np.zeros(x.size)
    y = np.zeros(x.size)
    for i, z in enumerate(_z(L, ndown)):
        diag += hz[i] * z
    for t, (rows, cols, zz) in enumerate(_partners(L, ndown, bonds)):
        diag += jz[t] * zz
        y[rows] += 2.0 * jxy[t] * x[cols]
    return y + diag * x


def forms(L, ndown, bonds, v1, v2):
    """out[t] = v1^T (dH/dp_t) v2, shape (2 nb + L,)"""
    v1, v2 = np.asarray(v1, dtype=np.float64), np.asarray(v2, dtype=np.float64)
    nb = len(bonds)
    out = np.zeros(nparam(L, bonds))
    for t, (rows, cols, zz) in enumerate(_partners(L, ndown, bonds)):
        out[t] = np.sum(2.0 * v1[rows] * v2[cols])
        out[nb + t] = np.sum(zz * v1 * v2)
    for i, z in enumerate(_z(L, ndown)):
        out[2 * nb + i] = np.sum(z * v1 * v2)
    return out


def dense(L, ndown, bonds, p):
    n = len(states(L, ndown))
    H = np.zeros((n, n))
    for c in range(n):
        e = np.zeros(n)
        e[c] = 1.0
        H[:, c] = apply(L, ndown, bonds, p, e)
    return H


def full_parameter(L, bonds, p):
    """[Jx, Jy, Jz, hx, hz] of lattice_reference with Jx = Jy = Jxy and hx = 0"""
    jxy, jz, hz = split(L, bonds, p)
    return np.concatenate([jxy, jxy, jz, np.zeros(L), hz])
