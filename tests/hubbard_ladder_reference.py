"""numpy reference of the site-weighted c / c+ / n maps between two particle-number sectors of the Hubbard space
(docs/design/25-hubbard-ladder.md); no GPU, no torch, and nothing of size 4^L, so it also works at L = 40.  Written from the
row formulas alone, vectorised per species like ``hubbard_reference.apply``.

Conventions of ``hubbard_reference``: bit i of u is (i, up), bit i of d is (i, dn), |u, d> = (prod_{i in u asc} c+_{i up})
(prod_{j in d asc} c+_{j dn}) |0>, row r = ru * n_dn + rd.  ``species`` is UP = 0 or DN = 1, ``step`` in {+1, 0, -1}; the
source is (nup, ndn), the destination has the count of ``species`` changed by ``step``.  With w' the word of the moving species
in a destination row, below_i = (1 << i) - 1 and par = popcount & 1:

    step = +1, sum_i w_i c+_{i s}:  y[row] = g sum_{i : bit_i(w') = 1} w_i (-1)^par(w' & below_i) x[row with rank_src(w' ^ (1 << i))]
    step = -1, sum_i w_i c_{i s}:   y[row] = g sum_{i : bit_i(w') = 0} w_i (-1)^par(w' & below_i) x[row with rank_src(w' | (1 << i))]
    step =  0, sum_i w_i n_{i s}:   y[row] = (sum_i w_i bit_i(w')) x[row]

g = 1 for the up species, (-1)^nup for the down species (every down operator stands right of all nup up operators).

    sizes(L, nup, ndn, species, step)            (n_src, n_dst)
    apply(L, nup, ndn, species, step, w, x)      the row formula
    forms(L, nup, ndn, species, step, v1, v2)    out[i] = v1^T (dS/dw_i) v2, v1 on the destination, v2 on the source
    dense(L, nup, ndn, species, step, w)         the n_dst x n_src matrix, for small n
"""
import functools

import numpy as np

import hubbard_reference as hub

UP, DN = 0, 1


def destination(nup, ndn, species, step):
    """(nup, ndn) of the destination"""
    assert species in (UP, DN) and step in (-1, 0, 1)
    return (nup + step, ndn) if species == UP else (nup, ndn + step)


def sizes(L, nup, ndn, species, step):
    nu, nd = destination(nup, ndn, species, step)
    return len(hub.states(L, nup)) * len(hub.states(L, ndn)), len(hub.states(L, nu)) * len(hub.states(L, nd))


@functools.lru_cache(maxsize=None)
def _partners(L, k_src, step):
    """for one species whose count goes from k_src to k_src + step, per site: step != 0: (ranks of the destination words to which
    the site contributes, ranks of their source words, (-1)^par(w' & below_i)); step = 0: (all ranks, bit_i).  Computed once and
    never written to"""
    words = np.array(hub.states(L, k_src + step), dtype=np.int64)
    out = []
    if step == 0:
        rows = np.arange(len(words))
        for i in range(L):
            bit = ((words >> i) & 1).astype(np.float64)
            bit.setflags(write=False)
            out.append((rows, rows, bit))
        return tuple(out)
    src = np.array(hub.states(L, k_src), dtype=np.int64)
    want = 1 if step > 0 else 0
    for i in range(L):
        rows = np.nonzero((words >> i) & 1 == want)[0]
        partner = words[rows] ^ (1 << i)
        cols = np.searchsorted(src, partner)             # rank_src: the position in the sorted source words
        assert np.array_equal(src[cols], partner)
        below = words[rows] & ((1 << i) - 1)
        par = np.zeros(len(rows), dtype=np.int64)
        for j in range(i):
            par ^= (below >> j) & 1
        sgn = 1.0 - 2.0 * par
        for a in (rows, cols, sgn):
            a.setflags(write=False)
        out.append((rows, cols, sgn))
    return tuple(out)


def _shapes(L, nup, ndn, species, step):
    nu, nd = destination(nup, ndn, species, step)
    return ((len(hub.states(L, nup)), len(hub.states(L, ndn))), (len(hub.states(L, nu)), len(hub.states(L, nd))))


def _sector_sign(nup, species, step):
    return -1.0 if (species == DN and step != 0 and nup % 2 == 1) else 1.0


def apply(L, nup, ndn, species, step, w, x):
    w, x = np.asarray(w, dtype=np.float64), np.asarray(x, dtype=np.float64)
    src, dst = _shapes(L, nup, ndn, species, step)
    assert w.shape == (L,) and x.shape == (src[0] * src[1],)
    X, Y = x.reshape(src), np.zeros(dst)
    g = _sector_sign(nup, species, step)
    for i, (rows, cols, f) in enumerate(_partners(L, nup if species == UP else ndn, step)):
        if species == UP:
            Y[rows, :] += w[i] * f[:, None] * X[cols, :]
        else:
            Y[:, rows] += (g * w[i]) * f[None, :] * X[:, cols]
    return Y.reshape(-1)


def forms(L, nup, ndn, species, step, v1, v2):
    v1, v2 = np.asarray(v1, dtype=np.float64), np.asarray(v2, dtype=np.float64)
    src, dst = _shapes(L, nup, ndn, species, step)
    assert v1.shape == (dst[0] * dst[1],) and v2.shape == (src[0] * src[1],)
    A, B = v1.reshape(dst), v2.reshape(src)
    g = _sector_sign(nup, species, step)
    out = np.zeros(L)
    for i, (rows, cols, f) in enumerate(_partners(L, nup if species == UP else ndn, step)):
        if species == UP:
            out[i] = np.sum(A[rows, :] * f[:, None] * B[cols, :])
        else:
            out[i] = g * np.sum(A[:, rows] * f[None, :] * B[:, cols])
    return out


def dense(L, nup, ndn, species, step, w):
    n_src, n_dst = sizes(L, nup, ndn, species, step)
    S = np.zeros((n_dst, n_src))
    for col in range(n_src):
        e = np.zeros(n_src)
        e[col] = 1.0
        S[:, col] = apply(L, nup, ndn, species, step, w, e)
    return S
