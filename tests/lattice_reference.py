"""numpy reference of the XYZ spins on a caller-given bond list (docs/design/16-spin-lattice.md); no GPU, no torch.

    H = sum_t [Jx_t X_a X_b + Jy_t Y_a Y_b + Jz_t Z_a Z_b] + sum_i [hx_i X_i + hz_i Z_i],   bond t joins sites a_t != b_t

Site i is bit i of the row index s, z_i(s) = 1 - 2 bit_i(s).  ``bonds`` is a list of nb pairs (a, b); (a, b) and (b, a) are
the same bond, a repeated bond counts each time.  ``p`` is the flat parameter [Jx(nb), Jy(nb), Jz(nb), hx(L), hz(L)].
Three independent statements of the same thing:

    dense(L, bonds, p)          Kronecker products of Pauli matrices (L <= 10)
    apply(L, bonds, p, x)       the vectorised row formula, any L
    forms(L, bonds, v1, v2)     the 3 nb + 2 L sums v1^T (dH/dp_t) v2 written out, in the order of p
"""
import numpy as np

_X = np.array([[0.0, 1.0], [1.0, 0.0]])
_Z = np.array([[1.0, 0.0], [0.0, -1.0]])
_I = np.eye(2)
# Y = i * _YI with _YI real antisymmetric, so Y (x) Y = -(_YI (x) _YI): real
_YI = np.array([[0.0, -1.0], [1.0, 0.0]])


def nparam(L, bonds):
    return 3 * len(bonds) + 2 * L


def split(L, bonds, p):
    """(Jx, Jy, Jz, hx, hz) views of the flat parameter"""
    nb = len(bonds)
    p = np.asarray(p, dtype=np.float64).reshape(nparam(L, bonds))
    return p[:nb], p[nb:2 * nb], p[2 * nb:3 * nb], p[3 * nb:3 * nb + L], p[3 * nb + L:]


def _site_product(L, ops):
    """kron over sites L-1 ... 0 (site 0 = the least significant bit = the LAST Kronecker factor); ops: {site: 2x2}"""
    M = np.ones((1, 1))
    for site in range(L - 1, -1, -1):
        M = np.kron(M, ops.get(site, _I))
    return M


def dense_terms(L, bonds):
    """the 3 nb + 2 L matrices dH/dp_t, in the order of the parameter"""
    assert 2 <= L <= 10
    jx, jy, jz = [], [], []
    for a, b in bonds:
        assert a != b
        jx.append(_site_product(L, {a: _X, b: _X}))
        jy.append(-_site_product(L, {a: _YI, b: _YI}))
        jz.append(_site_product(L, {a: _Z, b: _Z}))
    hx = [_site_product(L, {i: _X}) for i in range(L)]
    hz = [_site_product(L, {i: _Z}) for i in range(L)]
    return jx + jy + jz + hx + hz


def dense(L, bonds, p):
    p = np.asarray(p, dtype=np.float64).reshape(nparam(L, bonds))
    H = np.zeros((1 << L, 1 << L))
    for c, term in zip(p, dense_terms(L, bonds)):
        H += c * term
    return H


def _z(L, s):
    return [1.0 - 2.0 * ((s >> i) & 1) for i in range(L)]


def apply(L, bonds, p, x):
    """(H x)[s] = (sum_t Jz_t zz_t + sum_i hz_i z_i) x[s] + sum_i hx_i x[s ^ (1<<i)] + sum_t (Jx_t - Jy_t zz_t) x[s ^ m_t]"""
    jx, jy, jz, hx, hz = split(L, bonds, p)
    x = np.asarray(x, dtype=np.float64)
    s = np.arange(1 << L, dtype=np.int64)
    z = _z(L, s)
    diag = np.zeros(1 << L)
    y = np.zeros(1 << L)
    for i in range(L):
        diag += hz[i] * z[i]
        y += hx[i] * x[s ^ (1 << i)]
    for t, (a, b) in enumerate(bonds):
        zz = z[a] * z[b]
        diag += jz[t] * zz
        y += (jx[t] - jy[t] * zz) * x[s ^ ((1 << a) | (1 << b))]
    return y + diag * x


def forms(L, bonds, v1, v2, dtype=np.float64):
    """out[t] = v1^T (dH/dp_t) v2, shape (3 nb + 2 L,)"""
    v1, v2 = np.asarray(v1, dtype=dtype), np.asarray(v2, dtype=dtype)
    nb = len(bonds)
    s = np.arange(1 << L, dtype=np.int64)
    z = [zi.astype(dtype) for zi in _z(L, s)]
    out = np.zeros(nparam(L, bonds), dtype=dtype)
    for t, (a, b) in enumerate(bonds):
        zz = z[a] * z[b]
        flipped = v2[s ^ ((1 << a) | (1 << b))]
        out[t] = np.sum(v1 * flipped)
        out[nb + t] = -np.sum(zz * v1 * flipped)
        out[2 * nb + t] = np.sum(zz * v1 * v2)
    for i in range(L):
        out[3 * nb + i] = np.sum(v1 * v2[s ^ (1 << i)])
        out[3 * nb + L + i] = np.sum(z[i] * v1 * v2)
    return out


def random_bonds(L, nb, seed):
    """nb pairs of different sites from a fixed generator (any order of a pair's two sites, repeats possible)"""
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < nb:
        a, b = int(rng.randint(L)), int(rng.randint(L))
        if a != b:
            out.append((a, b))
    return out


def complete_bonds(L):
    return [(a, b) for a in range(L) for b in range(a + 1, L)]
