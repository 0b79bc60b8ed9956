"""numpy reference of the XYZ spin chain with per-site couplings (docs/design/14-spin-chain.md); no GPU, no torch.

    H = sum_b [Jx_b X_b X_b+1 + Jy_b Y_b Y_b+1 + Jz_b Z_b Z_b+1] + sum_i [hx_i X_i + hz_i Z_i],   periodic, L sites

Site i is bit i of the row index s, z_i(s) = 1 - 2 bit_i(s), bond b joins sites b and (b + 1) mod L.  ``couplings`` is a
(5, L) array, rows Jx, Jy, Jz, hx, hz.  Three independent statements of the same thing:

    dense(L, c)            Kronecker products of Pauli matrices (L <= 10)
    apply(L, c, x)         the vectorised row formula, any L
    forms(L, v1, v2)       the 5 L sums v1^T (dH/dp_t) v2 written out, shape (5, L)
"""
import numpy as np

_X = np.array([[0.0, 1.0], [1.0, 0.0]])
_Z = np.array([[1.0, 0.0], [0.0, -1.0]])
_I = np.eye(2)
# Y = i * _YI with _YI real antisymmetric, so Y (x) Y = -(_YI (x) _YI): real
_YI = np.array([[0.0, -1.0], [1.0, 0.0]])


def _site_product(L, ops):
    """kron over sites L-1 ... 0 (site 0 = the least significant bit = the LAST Kronecker factor); ops: {site: 2x2}.
    Two operators on the same site (L = 2: both bonds sit on sites 0, 1 -- never the same site twice) do not occur."""
    M = np.ones((1, 1))
    for site in range(L - 1, -1, -1):
        M = np.kron(M, ops.get(site, _I))
    return M


def dense_terms(L):
    """the 5 L matrices dH/dp_t, index [family][site or bond]"""
    assert 2 <= L <= 10
    out = [[], [], [], [], []]
    for b in range(L):
        b1 = (b + 1) % L
        out[0].append(_site_product(L, {b: _X, b1: _X}))
        out[1].append(-_site_product(L, {b: _YI, b1: _YI}))
        out[2].append(_site_product(L, {b: _Z, b1: _Z}))
        out[3].append(_site_product(L, {b: _X}))
        out[4].append(_site_product(L, {b: _Z}))
    return out


def dense(L, couplings):
    c = np.asarray(couplings, dtype=np.float64).reshape(5, L)
    terms = dense_terms(L)
    H = np.zeros((1 << L, 1 << L))
    for f in range(5):
        for i in range(L):
            H += c[f, i] * terms[f][i]
    return H


def _z(L, s):
    return [1.0 - 2.0 * ((s >> i) & 1) for i in range(L)]


def _mask(L, b):
    return (1 << b) | (1 << ((b + 1) % L))


def apply(L, couplings, x):
    """(H x)[s] = (sum_b Jz_b zz_b + sum_i hz_i z_i) x[s] + sum_i hx_i x[s ^ (1<<i)] + sum_b (Jx_b - Jy_b zz_b) x[s ^ m_b]"""
    c = np.asarray(couplings, dtype=np.float64).reshape(5, L)
    x = np.asarray(x, dtype=np.float64)
    s = np.arange(1 << L, dtype=np.int64)
    z = _z(L, s)
    diag = np.zeros(1 << L)
    y = np.zeros(1 << L)
    for b in range(L):
        zz = z[b] * z[(b + 1) % L]
        diag += c[2, b] * zz + c[4, b] * z[b]
        y += c[3, b] * x[s ^ (1 << b)]
        y += (c[0, b] - c[1, b] * zz) * x[s ^ _mask(L, b)]
    return y + diag * x


def forms(L, v1, v2, dtype=np.float64):
    """out[t] = v1^T (dH/dp_t) v2, shape (5, L)"""
    v1, v2 = np.asarray(v1, dtype=dtype), np.asarray(v2, dtype=dtype)
    s = np.arange(1 << L, dtype=np.int64)
    z = [zi.astype(dtype) for zi in _z(L, s)]
    out = np.zeros((5, L), dtype=dtype)
    for b in range(L):
        zz = z[b] * z[(b + 1) % L]
        flipped = v2[s ^ _mask(L, b)]
        out[0, b] = np.sum(v1 * flipped)
        out[1, b] = -np.sum(zz * v1 * flipped)
        out[2, b] = np.sum(zz * v1 * v2)
        out[3, b] = np.sum(v1 * v2[s ^ (1 << b)])
        out[4, b] = np.sum(z[b] * v1 * v2)
    return out


def tfim_couplings(L, g):
    c = np.zeros((5, L))
    c[2] = -1.0
    c[3] = -g
    return c
