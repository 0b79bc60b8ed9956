"""numpy twin of the block Hubbard mat-vec, the basis-free block Lanczos recurrence on it and the grand-canonical layer
(docs/design/28-hubbard-finite-temperature.md); no GPU, no torch.  Matrix-free on the partner lists of hubbard_reference.  The
recurrence takes a ``dtype`` (``numpy.float64`` or ``numpy.longdouble``); the k x k eigenproblems and the ensemble sums are
float64.  (The recurrence of sector_block_reference is tied to that module's mat-vec, so it is restated here.)

    coupling_bound(L, bonds, p)                        B = sum_t (2 |t_t| + 4 |V_t|) + sum_i (|U_i| + 2 |eps_i|) >= ||H||_2
    apply_block(L, nup, ndn, bonds, p, X, dtype)       H X column by column, the row formula of hubbard_reference.apply
    block_lanczos(L, nup, ndn, bonds, p, Phi, k)       norm2 [R], alphas [k, R], betas [k, R], steps [R]: the recurrence and the
                                                       break rule of the kernels, no basis, no re-orthogonalisation
    measure, block_measures, start_block, trace_measure    as in sector_block_reference
    edge_matrix(L, bonds, p, count, other_full)        the dense one-species Hamiltonian beside an empty or a full other species
    entries(L, bonds, p, ...)                          [(poles, weights, nup, ndn)] over the sectors, the edge sectors exact
    exact_entries(L, bonds, p)                         the same from dense eigh of every sector
    logZ, energy, density, compressibility, spin_susceptibility, specific_heat, entropy, moment
                                                       of such a list at arrays beta [nb] and mu [nm] -> [nb, nm], direct sums
"""
import math

import numpy as np

import hubbard_reference as ref
from dominantsparseeigenad_amd.synthetic import normal_vector

BREAK_TOL = 1e-13


def coupling_bound(L, bonds, p):
    t, V, U, eps = ref.split(L, bonds, p)
    return float(2.0 * np.abs(t).sum() + 4.0 * np.abs(V).sum() + np.abs(U).sum() + 2.0 * np.abs(eps).sum())


def apply_block(L, nup, ndn, bonds, p, X, dtype=np.float64):
    """H X for X of shape (n, R), in ``dtype``"""
    t, V, U, eps = (a.astype(dtype) for a in ref.split(L, bonds, p))
    n_up, n_dn = len(ref.states(L, nup)), len(ref.states(L, ndn))
    X = np.asarray(X, dtype=dtype)
    R = X.shape[1]
    X3 = X.reshape(n_up, n_dn, R)
    bu, bd = ref._occupations(L, nup, ndn)
    bu, bd = bu.astype(dtype), bd.astype(dtype)
    occ = bu + bd
    diag = np.zeros((n_up, n_dn), dtype=dtype)
    for i in range(L):
        diag += U[i] * (bu[i] * bd[i]) + eps[i] * occ[i]
    Y = np.zeros_like(X3)
    up, dn = ref._partners(L, nup, bonds), ref._partners(L, ndn, bonds)
    for k, (a, b) in enumerate(bonds):
        diag += V[k] * (occ[a] * occ[b])
        rows, cols, sgn = up[k]
        Y[rows] -= (t[k] * sgn.astype(dtype))[:, None, None] * X3[cols]
        rows, cols, sgn = dn[k]
        Y[:, rows] -= (t[k] * sgn.astype(dtype))[None, :, None] * X3[:, cols]
    return (Y + diag[:, :, None] * X3).reshape(n_up * n_dn, R)


def lanczos_recurrence(matvec, Phi, k, dtype=np.float64):
    """The recurrence of the block Lanczos kernels per column on the block mat-vec ``matvec(Q) -> H Q``: start q = phi / |phi|;
    step i: w = H q_i - beta_i q_{i-1}, alpha_i = q_i . w, w -= alpha_i q_i, beta_{i+1} = |w|, q_{i+1} = w / beta_{i+1}.  Column j
    breaks at the first s = i + 1 with not beta_s > 1e-13 max(earlier |alpha|, |beta|) (s = 0: a zero start column): steps[j] = s,
    the column is zeroed, its later coefficients and the breaking beta are 0."""
    Phi = np.asarray(Phi, dtype=dtype)
    n, R = Phi.shape
    alphas, betas = np.zeros((k, R), dtype=dtype), np.zeros((k, R), dtype=dtype)
    steps = np.full(R, k, dtype=np.int64)
    norm2 = np.einsum("rj,rj->j", Phi, Phi)
    beta = np.sqrt(norm2)
    alive = beta > 0
    steps[~alive] = 0
    scale = np.where(alive, beta, dtype(0.0))          # (beta_0 = |phi| counts among the earlier betas, as in k_sblock_finish)
    safe = np.where(alive, beta, dtype(1.0))
    Q = np.where(alive, Phi / safe, dtype(0.0))
    prev = np.zeros_like(Q)
    beta = np.where(alive, beta, dtype(0.0))
    for i in range(k):
        W = matvec(Q)
        if i:
            W = W - prev * beta
        alpha = np.einsum("rj,rj->j", Q, W)
        W = W - Q * alpha
        b = np.sqrt(np.einsum("rj,rj->j", W, W))
        scale = np.where(alive, np.maximum(scale, np.abs(alpha)), scale)
        now = alive & ~(b > dtype(BREAK_TOL) * scale)
        steps[now] = i + 1
        alive = alive & ~now
        scale = np.where(alive, np.maximum(scale, b), scale)
        beta = np.where(alive, b, dtype(0.0))
        alphas[i], betas[i] = alpha, beta
        safe = np.where(alive, b, dtype(1.0))
        nxt = np.where(alive, W / safe, dtype(0.0))
        Q = np.where(now, dtype(0.0), Q)
        prev, Q = Q, nxt
    return norm2, alphas, betas, steps


def block_lanczos(L, nup, ndn, bonds, p, Phi, k, dtype=np.float64):
    return lanczos_recurrence(lambda Q: apply_block(L, nup, ndn, bonds, p, Q, dtype), Phi, k, dtype)


def measure(alphas, betas, steps, norm2):
    """(poles, weights = norm2 S_0j^2) of the leading steps x steps tridiagonal matrix, float64"""
    s = int(steps)
    if s == 0:
        return np.zeros(0), np.zeros(0)
    a = np.asarray(alphas[:s], dtype=np.float64)
    b = np.asarray(betas[:s - 1], dtype=np.float64)
    T = np.diag(a) + np.diag(b, 1) + np.diag(b, -1)
    theta, S = np.linalg.eigh(T)
    return theta, float(norm2) * S[0] ** 2


def block_measures(L, nup, ndn, bonds, p, Phi, k, dtype=np.float64):
    k = min(int(k), np.asarray(Phi).shape[0])
    norm2, alphas, betas, steps = block_lanczos(L, nup, ndn, bonds, p, Phi, k, dtype)
    return [measure(alphas[:, j], betas[:, j], steps[j], norm2[j]) for j in range(len(steps))]


def start_block(n, R, seed):
    return np.stack([normal_vector(n, seed + j) for j in range(R)], axis=1)


def trace_measure(L, nup, ndn, bonds, p, R=8, k=100, seed=0, dense_below=256, dtype=np.float64):
    n = math.comb(L, nup) * math.comb(L, ndn)
    if n <= dense_below:
        return np.linalg.eigvalsh(ref.dense(L, nup, ndn, bonds, p)), np.ones(n)
    parts = block_measures(L, nup, ndn, bonds, p, start_block(n, R, seed), k, dtype)
    poles = np.concatenate([theta for theta, _ in parts])
    weights = np.concatenate([w * (n / (R * w.sum())) if w.size else w for _, w in parts])
    return poles, weights


def edge_matrix(L, bonds, p, count, other_full):
    """The Hamiltonian of one species with ``count`` particles (rows in the order of ``states(L, count)``) while the other
    species is empty (``other_full`` False) or full: hops -t_t (-1)^(own particles strictly between a and b), and the diagonal
    of the full model with every bit of the other species equal to f = 0 or 1."""
    t, V, U, eps = ref.split(L, bonds, p)
    st, rk = ref.states(L, count), ref.rank(L, count)
    f = 1 if other_full else 0
    H = np.zeros((len(st), len(st)))
    for r, w in enumerate(st):
        bit = [(w >> i) & 1 for i in range(L)]
        H[r, r] = sum(U[i] * bit[i] * f + eps[i] * (bit[i] + f) for i in range(L))
        for k, (a, b) in enumerate(bonds):
            H[r, r] += V[k] * (bit[a] + f) * (bit[b] + f)
            if bit[a] != bit[b]:
                sgn = 1.0 - 2.0 * (bin(w & ref.between(a, b)).count("1") & 1)
                H[rk[w ^ ((1 << a) | (1 << b))], r] -= t[k] * sgn
    return H


def entries(L, bonds, p, R=8, k=100, seed=0, dense_below=256, sectors=None, spin_symmetric=True, dtype=np.float64):
    """[(poles, weights, nup, ndn)]: bulk sectors from trace_measure, edge sectors from the eigenvalues of edge_matrix;
    ``spin_symmetric``: the sector (a, b) with a < b takes the measure of (b, a), as hubbard_thermodynamics does"""
    out = []
    sectors = [(a, b) for a in range(L + 1) for b in range(L + 1)] if sectors is None else sectors
    for first, second in sectors:
        nup, ndn = (max(first, second), min(first, second)) if spin_symmetric else (first, second)
        out.append(_sector_entry(L, bonds, p, nup, ndn, R, k, seed, dense_below, dtype) + (first, second))
    return out


def _sector_entry(L, bonds, p, nup, ndn, R, k, seed, dense_below, dtype):
    """(poles, weights) of one sector"""
    if nup in (0, L) and ndn in (0, L):
        return np.array([edge_matrix(L, bonds, p, nup, ndn == L)[0, 0]]), np.ones(1)
    if nup in (0, L) or ndn in (0, L):
        count, other = (ndn, nup) if nup in (0, L) else (nup, ndn)
        poles = np.linalg.eigvalsh(edge_matrix(L, bonds, p, count, other == L))
        return poles, np.ones(len(poles))
    return trace_measure(L, nup, ndn, bonds, p, R, k, seed, dense_below, dtype)


def exact_entries(L, bonds, p):
    """every sector from dense eigh of hubbard_reference.dense (which also takes an empty or a full species)"""
    out = []
    for nup in range(L + 1):
        for ndn in range(L + 1):
            poles = np.linalg.eigvalsh(ref.dense(L, nup, ndn, bonds, p))
            out.append((poles, np.ones(len(poles)), nup, ndn))
    return out


# ---- the grand-canonical functions as direct sums: one (beta, mu) at a time, every pole in turn ----------------------------
def _flat(ents):
    poles = np.concatenate([e[0] for e in ents])
    weights = np.concatenate([e[1] for e in ents])
    N = np.concatenate([np.full(len(e[0]), float(e[2] + e[3])) for e in ents])
    Sz = np.concatenate([np.full(len(e[0]), 0.5 * (e[2] - e[3])) for e in ents])
    return poles, weights, N, Sz


def _grid(ents, beta, mu, fn):
    poles, weights, N, Sz = _flat(ents)
    beta = np.atleast_1d(np.asarray(beta, dtype=np.float64))
    mu = np.atleast_1d(np.asarray(mu, dtype=np.float64))
    out = np.zeros((len(beta), len(mu)))
    for i, b in enumerate(beta):
        for j, m in enumerate(mu):
            K = poles - m * N
            low = K.min()
            terms = weights * np.exp(-b * (K - low))
            total = terms.sum()
            out[i, j] = fn(b, m, poles, N, Sz, K, low, total, terms / total)
    return out


def logZ(ents, beta, mu):
    return _grid(ents, beta, mu, lambda b, m, th, N, Sz, K, low, tot, pr: math.log(tot) - b * low)


def energy(ents, beta, mu):
    return _grid(ents, beta, mu, lambda b, m, th, N, Sz, K, low, tot, pr: float(pr @ th))


def density(ents, beta, mu):
    return _grid(ents, beta, mu, lambda b, m, th, N, Sz, K, low, tot, pr: float(pr @ N))


def compressibility(ents, beta, mu):
    return _grid(ents, beta, mu, lambda b, m, th, N, Sz, K, low, tot, pr: b * float(pr @ (N - pr @ N) ** 2))


def spin_susceptibility(ents, beta, mu):
    return _grid(ents, beta, mu, lambda b, m, th, N, Sz, K, low, tot, pr: b * float(pr @ (Sz - pr @ Sz) ** 2))


def specific_heat(ents, beta, mu):
    return _grid(ents, beta, mu, lambda b, m, th, N, Sz, K, low, tot, pr: b * b * float(pr @ (K - pr @ K) ** 2))


def entropy(ents, beta, mu):
    return _grid(ents, beta, mu,
                 lambda b, m, th, N, Sz, K, low, tot, pr: math.log(tot) - b * low + b * (float(pr @ th) - m * float(pr @ N)))


def moment(ents, power):
    poles, weights, _, _ = _flat(ents)
    return float((weights * poles ** int(power)).sum())
