"""numpy reference of the bond current map of a Hubbard sector (docs/design/39-hubbard-current.md); no GPU, no torch, and nothing
of size 4^L except where said, so it also works at L = 40.

    K(w) = sum_t sum_s w[s, t] (c+_{a s} c_{b s} - c+_{b s} c_{a s}),     (a, b) = bonds[t] in the caller's orientation

in the state order of tests/hubbard_reference.py (row r = ru * n_dn + rd).  ``w`` has shape (2, nb): species 0 = up, 1 = dn.  With
m_t, sgn_t as there and o_t(word) = +1 if bit a_t of the word is set, else -1:

    (K x)[r] = sum_{t: bits of u differ} w[0, t] o_t(u) sgn_t(u) x[rank_u(u ^ m_t) n_dn + rd]
             + sum_{t: bits of d differ} w[1, t] o_t(d) sgn_t(d) x[ru n_dn + rank_d(d ^ m_t)]

    apply(L, nup, ndn, bonds, w, x)              the row formula
    forms(L, nup, ndn, bonds, v1, v2)            the 2 nb sums v1^T K_{s t} v2 written out, shape (2, nb)
    dense(L, nup, ndn, bonds, w)                 the matrix, for small n
    dense_jordan_wigner(L, nup, ndn, bonds, w)   (K in the sector, the largest |entry| between the sector and the rest) from
                                                 2 x 2 Kronecker factors on 2 L modes; L <= 4
    dense_peierls(L, nup, ndn, bonds, p, d, phi) the complex Hamiltonian with every hopping t_t -> t_t exp(i phi d_t) on
                                                 c+_a c_b (and the conjugate on c+_b c_a), for small n
    optical(L, nup, ndn, bonds, p, d, kind)      K_d, I_-1, stiffness, |K psi0|^2 and the gap from dense ``eigh``
"""
import numpy as np

import hubbard_reference as href


def weights(w, nb):
    """(2, nb) float64 from a (2, nb) array or a (nb,) vector used for both species"""
    w = np.asarray(w, dtype=np.float64)
    if w.shape == (nb,):
        w = np.stack([w, w])
    assert w.shape == (2, nb), w.shape
    return w


def _orient(L, k, bonds):
    """per bond, for one species of k particles: o_t of the words that the bond moves, in the order of href._partners' rows"""
    st = href.states(L, k)
    part = href._partners(L, k, bonds)
    return [np.array([1.0 if (st[r] >> a) & 1 else -1.0 for r in part[t][0]]) for t, (a, b) in enumerate(bonds)]


def apply(L, nup, ndn, bonds, w, x):
    w = weights(w, len(bonds))
    n_up, n_dn = len(href.states(L, nup)), len(href.states(L, ndn))
    X = np.asarray(x, dtype=np.float64).reshape(n_up, n_dn)
    Y = np.zeros((n_up, n_dn))
    up, dn = href._partners(L, nup, bonds), href._partners(L, ndn, bonds)
    ou, od = _orient(L, nup, bonds), _orient(L, ndn, bonds)
    for t in range(len(bonds)):
        rows, cols, sgn = up[t]
        Y[rows, :] += w[0, t] * (ou[t] * sgn)[:, None] * X[cols, :]
        rows, cols, sgn = dn[t]
        Y[:, rows] += w[1, t] * (od[t] * sgn)[None, :] * X[:, cols]
    return Y.reshape(-1)


def forms(L, nup, ndn, bonds, v1, v2):
    n_up, n_dn = len(href.states(L, nup)), len(href.states(L, ndn))
    A = np.asarray(v1, dtype=np.float64).reshape(n_up, n_dn)
    B = np.asarray(v2, dtype=np.float64).reshape(n_up, n_dn)
    out = np.zeros((2, len(bonds)))
    up, dn = href._partners(L, nup, bonds), href._partners(L, ndn, bonds)
    ou, od = _orient(L, nup, bonds), _orient(L, ndn, bonds)
    for t in range(len(bonds)):
        rows, cols, sgn = up[t]
        out[0, t] = np.sum(A[rows, :] * (ou[t] * sgn)[:, None] * B[cols, :])
        rows, cols, sgn = dn[t]
        out[1, t] = np.sum(A[:, rows] * (od[t] * sgn)[None, :] * B[:, cols])
    return out


def dense(L, nup, ndn, bonds, w):
    n = len(href.states(L, nup)) * len(href.states(L, ndn))
    K = np.zeros((n, n))
    for c in range(n):
        e = np.zeros(n)
        e[c] = 1.0
        K[:, c] = apply(L, nup, ndn, bonds, w, e)
    return K


def dense_jordan_wigner(L, nup, ndn, bonds, w):
    """(K restricted to the (nup, ndn) sector, max |K[sector, rest]|) with the mode operators of href.dense_jordan_wigner"""
    assert L <= 4
    w = weights(w, len(bonds))
    M = 2 * L
    c = [href._annihilator(M, j) for j in range(M)]
    K = np.zeros((1 << M, 1 << M))
    for t, (a, b) in enumerate(bonds):
        for s, off in enumerate((0, L)):
            hop = c[a + off].T @ c[b + off]              # c+_a c_b
            K += w[s, t] * (hop - hop.T)
    index = np.array([u | (d << L) for u in href.states(L, nup) for d in href.states(L, ndn)], dtype=np.int64)
    rest = np.setdiff1d(np.arange(1 << M), index)
    return K[np.ix_(index, index)], float(np.max(np.abs(K[np.ix_(index, rest)])))


def _hop_matrices(L, nup, ndn, bonds):
    """per bond the real n x n matrix of sum_s c+_{a s} c_{b s} in the sector (one direction only)"""
    n_up, n_dn = len(href.states(L, nup)), len(href.states(L, ndn))
    up, dn = href._partners(L, nup, bonds), href._partners(L, ndn, bonds)
    ou, od = _orient(L, nup, bonds), _orient(L, ndn, bonds)
    out = []
    for t in range(len(bonds)):
        Su, Sd = np.zeros((n_up, n_up)), np.zeros((n_dn, n_dn))
        keep = ou[t] > 0                                 # rows whose word has bit a set: <row| c+_a c_b |partner> = sgn
        Su[up[t][0][keep], up[t][1][keep]] = up[t][2][keep]
        keep = od[t] > 0
        Sd[dn[t][0][keep], dn[t][1][keep]] = dn[t][2][keep]
        out.append(np.kron(Su, np.eye(n_dn)) + np.kron(np.eye(n_up), Sd))
    return out


def dense_peierls(L, nup, ndn, bonds, p, d, phi):
    """H(phi) = H(0) with -t_t sum_s (e^{i phi d_t} c+_{a s} c_{b s} + h.c.) in place of the hopping, complex Hermitian"""
    nb = len(bonds)
    t = href.split(L, bonds, p)[0]
    q = np.array(p, dtype=np.float64)
    q[:nb] = 0.0
    H = href.dense(L, nup, ndn, bonds, q).astype(np.complex128)
    for k, hop in enumerate(_hop_matrices(L, nup, ndn, bonds)):
        z = np.exp(1j * phi * d[k])
        H -= t[k] * (z * hop + np.conj(z) * hop.T)
    return H


def optical(L, nup, ndn, bonds, p, d, kind="charge", floor=1e-9):
    """the dense twin of spectral.optical_conductivity on the ground state of href.dense: a dictionary with E0, gap,
    diamagnetic K_d, inverse_moment I_-1, stiffness K_d - 2 I_-1, norm2 = |K psi0|^2 and dropped_weight"""
    nb = len(bonds)
    d = np.asarray(d, dtype=np.float64)
    t = href.split(L, bonds, p)[0]
    lam, vec = np.linalg.eigh(href.dense(L, nup, ndn, bonds, p))
    psi0 = vec[:, 0]
    wt = t * d
    w = np.stack([wt, wt if kind == "charge" else -wt])
    phi = apply(L, nup, ndn, bonds, w, psi0)
    kinetic = href.forms(L, nup, ndn, bonds, psi0, psi0)[:nb]          # dE0/dt_t = -<c+_a c_b + h.c.>
    K_d = -float(np.sum(t * d * d * kinetic))
    weight = (vec.T @ phi) ** 2
    omega = lam - lam[0]
    keep = omega > floor
    I = float(np.sum(weight[keep] / omega[keep]))
    return {"E0": float(lam[0]), "gap": float(lam[1] - lam[0]), "diamagnetic": K_d, "inverse_moment": I,
            "stiffness": K_d - 2.0 * I, "norm2": float(phi @ phi), "dropped_weight": float(np.sum(weight[~keep]))}
