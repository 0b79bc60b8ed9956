"""numpy twin of the block sector mat-vec, the basis-free block Lanczos recurrence and the finite-temperature layer
(docs/design/27-finite-temperature.md); no GPU, no torch.  Every function takes a ``dtype`` (``numpy.float64`` or
``numpy.longdouble``) for the recurrence; the k x k eigenproblems and the ensemble sums are float64.

    apply_block(L, ndown, bonds, p, X, dtype)     H X column by column, the row formula of sector_reference.apply in ``dtype``
    block_lanczos(L, ndown, bonds, p, Phi, k)     norm2 [R], alphas [k, R], betas [k, R], steps [R]: the recurrence and the break rule
                                                  of the kernels, no basis, no re-orthogonalisation
    measure(alphas, betas, steps, norm2)          (poles, weights) of one column
    block_measures(...)                           the list of them
    trace_measure(L, ndown, bonds, p, R, k, seed, dense_below)    (poles, weights) with sum w f(theta) ~= tr f(H_sector)
    spin_entries(L, bonds, p, ...)                [(poles, weights, m)] over the sectors, the two one-state sectors included
    exact_entries(L, bonds, p)                    the same from dense eigh of every sector
    logZ, energy, specific_heat, entropy, susceptibility, moment    of such a list, at an array of beta
    coupling_bound(L, bonds, p)                   B = sum_t (2 |Jxy_t| + |Jz_t|) + sum_i |hz_i| >= ||H||_2
"""
import math

import numpy as np

import sector_reference as ref
from dominantsparseeigenad_amd.synthetic import normal_vector

BREAK_TOL = 1e-13


def coupling_bound(L, bonds, p):
    jxy, jz, hz = ref.split(L, bonds, p)
    return float(2.0 * np.abs(jxy).sum() + np.abs(jz).sum() + np.abs(hz).sum())


def apply_block(L, ndown, bonds, p, X, dtype=np.float64):
    """H X for X of shape (n, R), in ``dtype``"""
    jxy, jz, hz = (a.astype(dtype) for a in ref.split(L, bonds, p))
    X = np.asarray(X, dtype=dtype)
    diag = np.zeros(X.shape[0], dtype=dtype)
    Y = np.zeros_like(X)
    for i, z in enumerate(ref._z(L, ndown)):
        diag += hz[i] * z.astype(dtype)
    two = dtype(2.0)
    for t, (rows, cols, zz) in enumerate(ref._partners(L, ndown, bonds)):
        diag += jz[t] * zz.astype(dtype)
        Y[rows] += (two * jxy[t]) * X[cols]
    return Y + diag[:, None] * X


def block_lanczos(L, ndown, bonds, p, Phi, k, dtype=np.float64):
    """The recurrence of dsea_op_sector_block_lanczos per column: start q = phi / |phi|; step i: w = H q_i - beta_i q_{i-1},
    alpha_i = q_i . w, w -= alpha_i q_i, beta_{i+1} = |w|, q_{i+1} = w / beta_{i+1}.  Column j breaks at the first s = i + 1 with
    not beta_s > 1e-13 max(earlier |alpha|, |beta|) (s = 0: a zero start column): steps[j] = s, the column is zeroed, its later
    coefficients and the breaking beta are 0."""
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
        W = apply_block(L, ndown, bonds, p, Q, dtype)
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


def block_measures(L, ndown, bonds, p, Phi, k, dtype=np.float64):
    k = min(int(k), np.asarray(Phi).shape[0])
    norm2, alphas, betas, steps = block_lanczos(L, ndown, bonds, p, Phi, k, dtype)
    return [measure(alphas[:, j], betas[:, j], steps[j], norm2[j]) for j in range(len(steps))]


def start_block(n, R, seed):
    return np.stack([normal_vector(n, seed + j) for j in range(R)], axis=1)


def trace_measure(L, ndown, bonds, p, R=8, k=100, seed=0, dense_below=256, dtype=np.float64):
    n = math.comb(L, ndown)
    if n <= dense_below:
        return np.linalg.eigvalsh(ref.dense(L, ndown, bonds, p)), np.ones(n)
    parts = block_measures(L, ndown, bonds, p, start_block(n, R, seed), k, dtype)
    poles = np.concatenate([theta for theta, _ in parts])
    weights = np.concatenate([w * (n / (R * w.sum())) if w.size else w for _, w in parts])
    return poles, weights


def edge_energy(L, bonds, p, ndown):
    """the energy of the one state of the sector ndown = 0 (all z = +1) or ndown = L (all z = -1)"""
    _, jz, hz = ref.split(L, bonds, p)
    return float(jz.sum() + (hz.sum() if ndown == 0 else -hz.sum()))


def spin_entries(L, bonds, p, R=8, k=100, seed=0, dense_below=256, sectors=None, dtype=np.float64):
    out = []
    for ndown in (range(L + 1) if sectors is None else sectors):
        m = 0.5 * L - ndown
        if ndown in (0, L):
            out.append((np.array([edge_energy(L, bonds, p, ndown)]), np.ones(1), m))
        else:
            poles, weights = trace_measure(L, ndown, bonds, p, R, k, seed, dense_below, dtype)
            out.append((poles, weights, m))
    return out


def exact_entries(L, bonds, p):
    return spin_entries(L, bonds, p, dense_below=1 << 62)


def _flat(entries):
    poles = np.concatenate([e[0] for e in entries])
    weights = np.concatenate([e[1] for e in entries])
    m = np.concatenate([np.full(len(e[0]), e[2]) for e in entries])
    return poles, weights, m


def _boltzmann(entries, beta):
    poles, weights, m = _flat(entries)
    beta = np.atleast_1d(np.asarray(beta, dtype=np.float64))
    low = poles.min()
    terms = weights * np.exp(-beta[:, None] * (poles - low))
    total = terms.sum(axis=1)
    return beta, poles, m, low, total, terms / total[:, None]


def logZ(entries, beta):
    beta, _, _, low, total, _ = _boltzmann(entries, beta)
    return np.log(total) - beta * low


def energy(entries, beta):
    _, poles, _, _, _, prob = _boltzmann(entries, beta)
    return prob @ poles


def specific_heat(entries, beta):
    beta, poles, _, _, _, prob = _boltzmann(entries, beta)
    E = prob @ poles
    return beta ** 2 * (prob * (poles[None, :] - E[:, None]) ** 2).sum(axis=1)


def entropy(entries, beta):
    return logZ(entries, beta) + np.atleast_1d(np.asarray(beta, dtype=np.float64)) * energy(entries, beta)


def susceptibility(entries, beta):
    beta, _, m, _, _, prob = _boltzmann(entries, beta)
    mean = prob @ m
    return beta * (prob * (m[None, :] - mean[:, None]) ** 2).sum(axis=1)


def moment(entries, power):
    poles, weights, _ = _flat(entries)
    return float((weights * poles ** int(power)).sum())
