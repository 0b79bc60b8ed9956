"""numpy reference of the Hubbard model on a caller-given bond list at fixed (nup, ndn) (docs/design/19-hubbard.md); no GPU, no
torch, and nothing of size 4^L, so it also works at L = 40.

    H = sum_t [-t_t sum_s (c+_{a s} c_{b s} + h.c.) + V_t n_a n_b] + sum_i U_i n_{i up} n_{i dn} + sum_i eps_i n_i

Bit i of the word u is the occupation of (i, up), bit i of d that of (i, dn);
|u, d> = (prod_{i in u, ascending} c+_{i up}) (prod_{j in d, ascending} c+_{j dn}) |0>.  Row r = ru * n_dn + rd with ru, rd the
ranks of u, d among the words of their popcount in increasing integer order.  ``p`` is the flat parameter
[t(nb), V(nb), U(L), eps(L)].  With m_t = (1 << a) | (1 << b) and sgn_t(w) = (-1)^popcount(w & bits strictly between a and b):

    (H x)[r] = diag(u, d) x[r] - sum_{t: bits of u differ} t_t sgn_t(u) x[rank_u(u ^ m_t) n_dn + rd]
                               - sum_{t: bits of d differ} t_t sgn_t(d) x[ru n_dn + rank_d(d ^ m_t)]

    states(L, k)                              the sorted L-bit words with k set bits
    apply(L, nup, ndn, bonds, p, x)           the row formula
    forms(L, nup, ndn, bonds, v1, v2)         the 2 nb + 2 L sums v1^T (dH/dp) v2 written out, in the order of p
    dense(L, nup, ndn, bonds, p)              the matrix, for small n
    dense_jordan_wigner(L, nup, ndn, bonds, p)  (H in the sector, the largest |entry| between the sector and the rest) from
                                              2 x 2 Kronecker factors on 2 L modes, mode i = (i, up), mode L + i = (i, dn); L <= 4
    moves(L, nup, ndn, bonds)                 the number of (row, species, distinct bond mask) that move a particle
"""
import functools
import itertools

import numpy as np


def nparam(L, bonds):
    return 2 * len(bonds) + 2 * L


def split(L, bonds, p):
    """(t, V, U, eps) views of the flat parameter"""
    nb = len(bonds)
    p = np.asarray(p, dtype=np.float64).reshape(nparam(L, bonds))
    return p[:nb], p[nb:2 * nb], p[2 * nb:2 * nb + L], p[2 * nb + L:]


@functools.lru_cache(maxsize=None)
def states(L, k):
    """the L-bit words with k set bits as a sorted tuple of Python ints"""
    return tuple(sorted(sum(1 << i for i in sites) for sites in itertools.combinations(range(L), k)))


@functools.lru_cache(maxsize=None)
def rank(L, k):
    """word -> rank, a dictionary"""
    return {s: r for r, s in enumerate(states(L, k))}


def between(a, b):
    lo, hi = min(a, b), max(a, b)
    return ((1 << hi) - 1) & ~((1 << (lo + 1)) - 1)


def _partners(L, k, bonds):
    """per bond, for one species of k particles: (ranks whose two bits differ, the ranks of their partner words, sgn_t of those
    words); computed once per (L, k, bond list) and never written to"""
    return _partners_cached(L, k, tuple((int(a), int(b)) for a, b in bonds))


@functools.lru_cache(maxsize=None)
def _partners_cached(L, k, bonds):
    st, rk = states(L, k), rank(L, k)
    out = []
    for a, b in bonds:
        m, B = (1 << a) | (1 << b), between(a, b)
        rows = np.array([r for r, w in enumerate(st) if ((w >> a) ^ (w >> b)) & 1], dtype=np.int64)
        cols = np.array([rk[st[r] ^ m] for r in rows], dtype=np.int64)
        sgn = np.array([1.0 - 2.0 * (bin(st[r] & B).count("1") & 1) for r in rows], dtype=np.float64)
        for arr in (rows, cols, sgn):
            arr.setflags(write=False)
        out.append((rows, cols, sgn))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _bits(L, k):
    """bits[i][r] = bit i of the r-th word, as float64"""
    words = np.array(states(L, k), dtype=np.int64)
    out = np.array([((words >> i) & 1).astype(np.float64) for i in range(L)])
    out.setflags(write=False)
    return out


def _occupations(L, nup, ndn):
    """(bu, bd): bit i of u and of d over the rows as (L, n_up, n_dn) arrays (views, broadcast)"""
    bu, bd = _bits(L, nup), _bits(L, ndn)
    return bu[:, :, None], bd[:, None, :]


def apply(L, nup, ndn, bonds, p, x):
    t, V, U, eps = split(L, bonds, p)
    n_up, n_dn = len(states(L, nup)), len(states(L, ndn))
    X = np.asarray(x, dtype=np.float64).reshape(n_up, n_dn)
    bu, bd = _occupations(L, nup, ndn)
    occ = bu + bd
    diag = np.zeros((n_up, n_dn))
    for i in range(L):
        diag += U[i] * (bu[i] * bd[i]) + eps[i] * occ[i]
    Y = np.zeros((n_up, n_dn))
    up, dn = _partners(L, nup, bonds), _partners(L, ndn, bonds)
    for k, (a, b) in enumerate(bonds):
        diag += V[k] * (occ[a] * occ[b])
        rows, cols, sgn = up[k]
        Y[rows, :] -= t[k] * sgn[:, None] * X[cols, :]
        rows, cols, sgn = dn[k]
        Y[:, rows] -= t[k] * sgn[None, :] * X[:, cols]
    return (Y + diag * X).reshape(-1)


def forms(L, nup, ndn, bonds, v1, v2):
    """out[p] = v1^T (dH/dp) v2, shape (2 nb + 2 L,)"""
    n_up, n_dn = len(states(L, nup)), len(states(L, ndn))
    A = np.asarray(v1, dtype=np.float64).reshape(n_up, n_dn)
    B = np.asarray(v2, dtype=np.float64).reshape(n_up, n_dn)
    nb = len(bonds)
    bu, bd = _occupations(L, nup, ndn)
    occ = bu + bd
    AB = A * B
    out = np.zeros(nparam(L, bonds))
    up, dn = _partners(L, nup, bonds), _partners(L, ndn, bonds)
    for k, (a, b) in enumerate(bonds):
        rows, cols, sgn = up[k]
        hop = np.sum(A[rows, :] * sgn[:, None] * B[cols, :])
        rows, cols, sgn = dn[k]
        hop += np.sum(A[:, rows] * sgn[None, :] * B[:, cols])
        out[k] = -hop
        out[nb + k] = np.sum(occ[a] * occ[b] * AB)
    for i in range(L):
        out[2 * nb + i] = np.sum(bu[i] * bd[i] * AB)
        out[2 * nb + L + i] = np.sum(occ[i] * AB)
    return out


def dense(L, nup, ndn, bonds, p):
    n = len(states(L, nup)) * len(states(L, ndn))
    H = np.zeros((n, n))
    for c in range(n):
        e = np.zeros(n)
        e[c] = 1.0
        H[:, c] = apply(L, nup, ndn, bonds, p, e)
    return H


def moves(L, nup, ndn, bonds):
    """the number of (row, species, distinct bond mask) in which the mask moves a particle of that species"""
    masks = {(1 << a) | (1 << b) for a, b in bonds}
    n_up, n_dn = len(states(L, nup)), len(states(L, ndn))
    up = sum(sum(1 for w in states(L, nup) if bin(w & m).count("1") == 1) for m in masks)
    dn = sum(sum(1 for w in states(L, ndn) if bin(w & m).count("1") == 1) for m in masks)
    return up * n_dn + dn * n_up


# ---- the same Hamiltonian from second quantisation: Jordan-Wigner on 2 L modes -------------------------------------------
_I2 = np.eye(2)
_Z2 = np.diag([1.0, -1.0])
_LOWER = np.array([[0.0, 1.0], [0.0, 0.0]])      # |0><1|: removes the particle of a mode (index 1 = occupied)


def _annihilator(M, j):
    """c_j on M modes as a 2^M matrix whose index has mode q at bit q: Z on the modes below j, |0><1| on j, 1 above.  The
    Kronecker product lists the factor of the highest bit first."""
    out = np.ones((1, 1))
    for q in range(M - 1, -1, -1):
        out = np.kron(out, _LOWER if q == j else (_Z2 if q < j else _I2))
    return out


def dense_jordan_wigner(L, nup, ndn, bonds, p):
    """(H restricted to the (nup, ndn) sector in the row order above, max |H[sector, rest]|).  With c_j = Z_0 .. Z_{j-1} |0><1|_j
    the state (prod_{modes ascending} c+_j) |0> is the basis vector of the occupation word with sign +1: c+_j acting on a state
    whose occupied modes are all above j meets no Z."""
    assert L <= 4
    t, V, U, eps = split(L, bonds, p)
    M = 2 * L
    c = [_annihilator(M, j) for j in range(M)]
    num = [cj.T @ cj for cj in c]
    H = np.zeros((1 << M, 1 << M))
    for k, (a, b) in enumerate(bonds):
        for off in (0, L):
            hop = c[a + off].T @ c[b + off]
            H -= t[k] * (hop + hop.T)
        H += V[k] * (num[a] + num[a + L]) @ (num[b] + num[b + L])
    for i in range(L):
        H += U[i] * num[i] @ num[i + L] + eps[i] * (num[i] + num[i + L])
    index = np.array([u | (d << L) for u in states(L, nup) for d in states(L, ndn)], dtype=np.int64)
    rest = np.setdiff1d(np.arange(1 << M), index)
    return H[np.ix_(index, index)], float(np.max(np.abs(H[np.ix_(index, rest)])))
