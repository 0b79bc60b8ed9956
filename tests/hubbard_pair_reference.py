"""numpy reference of the maps that move one particle of each species between two particle-number sectors of the Hubbard space
(docs/design/41-hubbard-pair-ladder.md); no GPU, no torch, and nothing of size 4^L, so it also works at L = 40.  Written from
the row formula alone, not by composing the single-species ladders of ``hubbard_ladder_reference``.

Conventions of ``hubbard_reference``: bit i of u is (i, up), bit i of d is (i, dn), |u, d> = (prod_{i in u asc} c+_{i up})
(prod_{j in d asc} c+_{j dn}) |0>, row r = ru * n_dn + rd.  The source is (nup, ndn), the steps (su, sd) are each +1 or -1 and
the destination is (nup + su, ndn + sd).  With A = c+ for su = +1 and c for su = -1, B likewise for sd, and W an (L, L) matrix:

    order 0 (up operator left):   P = sum_ij W_ij A_{i up} B_{j dn}
    order 1 (down operator left): P = sum_ij W_ij B_{j dn} A_{i up}

    y[ru' n_dn_dst + rd'] = g sum_{i qualifies in u'} sum_{j qualifies in d'} W_ij (-1)^par(u' & below_i) (-1)^par(d' & below_j)
                              x[rank_up_src(u' ^ (1 << i)) n_dn_src + rank_dn_src(d' ^ (1 << j))]

(u', d') the words of the destination row, below_i = (1 << i) - 1, par = popcount & 1; a site qualifies when its bit is set in
the destination word for a step of +1 and clear for -1; g = (-1)^(nup + order).

    sizes(L, nup, ndn, su, sd)                         (n_src, n_dst)
    apply(L, nup, ndn, su, sd, order, W, x)            the row formula
    apply_abs(L, nup, ndn, su, sd, W, x)               the same sum with |W_ij|, |x| and no signs: (|P| |x|), for error bounds
    forms(L, nup, ndn, su, sd, order, v1, v2)          out[i, j] = v1^T (dP/dW_ij) v2, v1 on the destination, v2 on the source
    forms_abs(L, nup, ndn, su, sd, v1, v2)             the same sums with |v1|, |v2| and no signs
    dense(L, nup, ndn, su, sd, order, W)               the n_dst x n_src matrix, for small n
    dense_abs(L, nup, ndn, su, sd, W)                  the same with |W| and no signs
"""
import functools

import numpy as np

import hubbard_reference as hub


def _check(su, sd, order=0):
    assert su in (-1, 1) and sd in (-1, 1) and order in (0, 1)


def sizes(L, nup, ndn, su, sd):
    _check(su, sd)
    return (len(hub.states(L, nup)) * len(hub.states(L, ndn)),
            len(hub.states(L, nup + su)) * len(hub.states(L, ndn + sd)))


def _shapes(L, nup, ndn, su, sd):
    return ((len(hub.states(L, nup)), len(hub.states(L, ndn))),
            (len(hub.states(L, nup + su)), len(hub.states(L, ndn + sd))))


@functools.lru_cache(maxsize=None)
def _site_terms(L, k_src, step):
    """for one species whose count goes from k_src to k_src + step, per site i: (ranks of the destination words in which the site
    qualifies, ranks of the source words w' ^ (1 << i), (-1)^par(w' & below_i)).  Computed once and never written to"""
    dst, src = hub.states(L, k_src + step), hub.rank(L, k_src)
    want = 1 if step > 0 else 0
    out = []
    for i in range(L):
        rows = [r for r, w in enumerate(dst) if (w >> i) & 1 == want]
        cols = [src[dst[r] ^ (1 << i)] for r in rows]
        sgn = [1.0 - 2.0 * (bin(dst[r] & ((1 << i) - 1)).count("1") & 1) for r in rows]
        arrs = (np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(sgn, dtype=np.float64))
        for a in arrs:
            a.setflags(write=False)
        out.append(arrs)
    return tuple(out)


def _g(nup, order):
    return -1.0 if (nup + order) % 2 else 1.0


def _weights(L, W):
    W = np.asarray(W, dtype=np.float64)
    assert W.shape == (L, L)
    return W


def _apply(L, nup, ndn, su, sd, g, W, x, signed):
    src, dst = _shapes(L, nup, ndn, su, sd)
    x = np.asarray(x, dtype=np.float64)
    assert x.shape == (src[0] * src[1],)
    X, Y = x.reshape(src), np.zeros(dst)
    up, dn = _site_terms(L, nup, su), _site_terms(L, ndn, sd)
    for i, (ru, cu, fu) in enumerate(up):
        if not len(ru):
            continue
        for j, (rd, cd, fd) in enumerate(dn):
            if not len(rd) or W[i, j] == 0.0:
                continue
            block = X[np.ix_(cu, cd)]
            if signed:
                block = block * fu[:, None] * fd[None, :]
            Y[np.ix_(ru, rd)] += (g * W[i, j]) * block
    return Y.reshape(-1)


def apply(L, nup, ndn, su, sd, order, W, x):
    _check(su, sd, order)
    return _apply(L, nup, ndn, su, sd, _g(nup, order), _weights(L, W), x, True)


def apply_abs(L, nup, ndn, su, sd, W, x):
    _check(su, sd)
    return _apply(L, nup, ndn, su, sd, 1.0, np.abs(_weights(L, W)), np.abs(np.asarray(x, dtype=np.float64)), False)


def _forms(L, nup, ndn, su, sd, g, v1, v2, signed):
    src, dst = _shapes(L, nup, ndn, su, sd)
    v1, v2 = np.asarray(v1, dtype=np.float64), np.asarray(v2, dtype=np.float64)
    assert v1.shape == (dst[0] * dst[1],) and v2.shape == (src[0] * src[1],)
    A, B = v1.reshape(dst), v2.reshape(src)
    up, dn = _site_terms(L, nup, su), _site_terms(L, ndn, sd)
    out = np.zeros((L, L))
    for i, (ru, cu, fu) in enumerate(up):
        for j, (rd, cd, fd) in enumerate(dn):
            if not len(ru) or not len(rd):
                continue
            block = A[np.ix_(ru, rd)] * B[np.ix_(cu, cd)]
            if signed:
                block = block * fu[:, None] * fd[None, :]
            out[i, j] = g * np.sum(block)
    return out


def forms(L, nup, ndn, su, sd, order, v1, v2):
    _check(su, sd, order)
    return _forms(L, nup, ndn, su, sd, _g(nup, order), v1, v2, True)


def forms_abs(L, nup, ndn, su, sd, v1, v2):
    _check(su, sd)
    return _forms(L, nup, ndn, su, sd, 1.0, np.abs(np.asarray(v1, dtype=np.float64)), np.abs(np.asarray(v2, dtype=np.float64)),
                  False)


def _dense(L, nup, ndn, su, sd, g, W, signed):
    src, dst = _shapes(L, nup, ndn, su, sd)
    S = np.zeros((dst[0] * dst[1], src[0] * src[1]))
    up, dn = _site_terms(L, nup, su), _site_terms(L, ndn, sd)
    for i, (ru, cu, fu) in enumerate(up):
        for j, (rd, cd, fd) in enumerate(dn):
            if not len(ru) or not len(rd):
                continue
            rows = (ru[:, None] * dst[1] + rd[None, :]).reshape(-1)
            cols = (cu[:, None] * src[1] + cd[None, :]).reshape(-1)
            val = np.full(len(rows), g * W[i, j])
            if signed:
                val = val * (fu[:, None] * fd[None, :]).reshape(-1)
            S[rows, cols] += val          # (a (row, column) pair fixes (i, j): every entry is written once)
    return S


def dense(L, nup, ndn, su, sd, order, W):
    _check(su, sd, order)
    return _dense(L, nup, ndn, su, sd, _g(nup, order), _weights(L, W), True)


def dense_abs(L, nup, ndn, su, sd, W):
    _check(su, sd)
    return _dense(L, nup, ndn, su, sd, 1.0, np.abs(_weights(L, W)), False)
