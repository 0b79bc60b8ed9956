"""numpy reference of the site-weighted ladder maps between two magnetisation sectors (docs/design/24-dynamics.md); no GPU, no
torch, and nothing of size 2^L, so it also works at L = 40.  Written from the formulas alone.

Site i is bit i of a state, a set bit is a down spin, z_i(s) = 1 - 2 bit_i(s).  The map takes the sector (L, ndown_src) to
(L, ndown_src + step); with r' a row of the destination and s' its state (rows in increasing integer order,
``sector_reference.states`` / ``rank``):

    step = +1, sigma^-(c):  y[r'] = sum_{i : bit_i(s') = 1} c_i x[rank_src(s' ^ (1 << i))]
    step = -1, sigma^+(c):  y[r'] = sum_{i : bit_i(s') = 0} c_i x[rank_src(s' | (1 << i))]
    step =  0, Z(c):        y[r'] = (sum_i c_i z_i(s')) x[r']

    apply(L, ndown_src, step, c, x)        the row formula
    forms(L, ndown_src, step, v1, v2)      out[i] = v1^T (dS/dc_i) v2, v1 on the destination, v2 on the source
    dense(L, ndown_src, step, c)           the n_dst x n_src matrix, for small n
"""
import functools

import numpy as np

import sector_reference


@functools.lru_cache(maxsize=None)
def _partners(L, ndown_src, step):
    """per site: (destination rows to which the site contributes, the source rows they read); step = 0: (all rows, z_i).
    Computed once per (L, ndown_src, step) and never written to"""
    dst = sector_reference.states(L, ndown_src + step)
    out = []
    if step == 0:
        words = np.array(dst, dtype=np.int64)
        rows = np.arange(len(dst))
        for i in range(L):
            z = 1.0 - 2.0 * ((words >> i) & 1)
            z.setflags(write=False)
            out.append((rows, z))
        return tuple(out)
    words = np.array(dst, dtype=np.int64)
    src = np.array(sector_reference.states(L, ndown_src), dtype=np.int64)
    want = 1 if step > 0 else 0
    for i in range(L):
        rows = np.nonzero((words >> i) & 1 == want)[0]
        partner = words[rows] ^ (1 << i)
        cols = np.searchsorted(src, partner)             # rank_src: the position in the sorted source states
        assert np.array_equal(src[cols], partner)
        for a in (rows, cols):
            a.setflags(write=False)
        out.append((rows, cols))
    return tuple(out)


def sizes(L, ndown_src, step):
    """(n_src, n_dst)"""
    return len(sector_reference.states(L, ndown_src)), len(sector_reference.states(L, ndown_src + step))


def apply(L, ndown_src, step, c, x):
    c, x = np.asarray(c, dtype=np.float64), np.asarray(x, dtype=np.float64)
    n_src, n_dst = sizes(L, ndown_src, step)
    assert c.shape == (L,) and x.shape == (n_src,)
    y = np.zeros(n_dst)
    if step == 0:
        diag = np.zeros(n_dst)
        for i, (_, z) in enumerate(_partners(L, ndown_src, 0)):
            diag += c[i] * z
        return diag * x
    for i, (rows, cols) in enumerate(_partners(L, ndown_src, step)):
        y[rows] += c[i] * x[cols]
    return y


def forms(L, ndown_src, step, v1, v2):
    v1, v2 = np.asarray(v1, dtype=np.float64), np.asarray(v2, dtype=np.float64)
    n_src, n_dst = sizes(L, ndown_src, step)
    assert v1.shape == (n_dst,) and v2.shape == (n_src,)
    out = np.zeros(L)
    for i, (rows, second) in enumerate(_partners(L, ndown_src, step)):
        out[i] = np.sum(second * v1 * v2) if step == 0 else np.sum(v1[rows] * v2[second])
    return out


def dense(L, ndown_src, step, c):
    n_src, n_dst = sizes(L, ndown_src, step)
    S = np.zeros((n_dst, n_src))
    for col in range(n_src):
        e = np.zeros(n_src)
        e[col] = 1.0
        S[:, col] = apply(L, ndown_src, step, c, e)
    return S
