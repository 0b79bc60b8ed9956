"""numpy twin of the Chebyshev block propagator and of the thermal-pure-quantum-state sums built on it
(docs/design/31-chebyshev-propagator.md); no GPU, no torch.  Built on ``sector_block_reference`` (the block mat-vec, the
recurrence that gives the Ritz values) and ``sector_reference`` (partner lists, forms, dense matrices).  Every function that
runs the recurrence takes a ``dtype`` (``numpy.float64`` or ``numpy.longdouble``).

    coefficients(f, M)                       c_0 / 2, c_1, ... by Chebyshev-Gauss quadrature in longdouble, rounded to float64
    order(f, guess, tol), exp_order(x, tol)  the truncation rule
    recurrence(apply, X, coeffs, bounds)     sum_m c_m T_m X on any ``apply``, the operation order of k_cheb_sector_block's tail
    chebyshev_apply(L, ndown, bonds, p, X, coeffs, bounds, dtype)
    expm(...)  time_evolve(...)              (Y, shift) and e^{-iHt} psi
    spectral_bounds(L, ndown, bonds, p)      Ritz values of a one-column run, widened, cut to [-B, B]
    correlations(L, ndown, v)                (xy, zz, z) of one sector vector
    thermal_correlations(L, bonds, p, betas, R, seed, dense_below)   dict of logZ, energy, xy, zz, z
"""
import math

import numpy as np

import sector_block_reference as blockref
import sector_reference as ref

LD = np.longdouble


def coefficients(f, M, nodes=None):
    N = 2 * M if nodes is None else nodes
    assert N >= 2 * M
    pi = 4 * np.arctan(LD(1))
    theta = pi * (np.arange(N, dtype=LD) + LD(0.5)) / LD(N)
    values = np.asarray(f(np.cos(theta)), dtype=LD)
    c = np.array([(LD(2) / LD(N)) * np.sum(values * np.cos(LD(m) * theta)) for m in range(M)], dtype=LD)
    c[0] /= LD(2)
    return c.astype(np.float64)


def order(f, guess, tol=1e-15):
    K = max(8, int(guess))
    while True:
        c = np.abs(coefficients(f, 2 * K))
        if not c.max() > 0:                              # (f vanishes at every node: sin(0 s))
            return 2
        M = max(2, int(np.nonzero(c >= tol * c.max())[0][-1]) + 1)
        if M <= K:
            return M
        K *= 2


def _guess(x):
    return int(x + 9.0 * math.sqrt(x)) + 24


def exp_function(x):
    return lambda s: np.exp(-LD(x) * (s + LD(1)))


def exp_order(x, tol=1e-15):
    return order(exp_function(x), _guess(x), tol)


def recurrence(apply, X, coeffs, bounds, dtype=np.float64):
    """[A, n, R]: acc_a = sum_m coeffs[a, m] T_m((H - centre) / h) X with t = g (H x - centre x), t -= old, acc += c t, each
    product and sum rounded on its own in ``dtype``; ``apply(x)`` is H x"""
    coeffs = np.atleast_2d(np.asarray(coeffs, dtype=np.float64)).astype(dtype)
    a, b = float(bounds[0]), float(bounds[1])
    centre, h = dtype(0.5 * (a + b)), 0.5 * (b - a)
    x, old = np.asarray(X, dtype=dtype), None
    for m in range(1, coeffs.shape[1]):
        g = dtype((1.0 if m == 1 else 2.0) / h)
        t = g * (apply(x) - centre * x)
        if m == 1:
            acc = [c[0] * x + c[1] * t for c in coeffs]
        else:
            t = t - old
            acc = [acc[i] + c[m] * t for i, c in enumerate(coeffs)]
        old, x = x, t
    return np.stack(acc)


def chebyshev_apply(L, ndown, bonds, p, X, coeffs, bounds, dtype=np.float64):
    out = recurrence(lambda x: blockref.apply_block(L, ndown, bonds, p, x, dtype), X, coeffs, bounds, dtype)
    return out[0] if np.ndim(coeffs) == 1 else out


def expm(L, ndown, bonds, p, X, tau, bounds, dtype=np.float64, tol=1e-15):
    """(Y, shift): e^{-tau H} X = e^{-tau shift} Y, shift = bounds[0]"""
    a, b = float(bounds[0]), float(bounds[1])
    if tau == 0:
        return np.array(X, dtype=dtype), a
    x = tau * 0.5 * (b - a)
    return chebyshev_apply(L, ndown, bonds, p, X, coefficients(exp_function(x), exp_order(x, tol)), bounds, dtype), a


def evolution_coefficients(t, bounds, tol=1e-15):
    """[2, M]: cos and sin of H t = h t s + centre t"""
    a, b = float(bounds[0]), float(bounds[1])
    centre, h = 0.5 * (a + b), 0.5 * (b - a)
    w, phase = LD(h * t), LD(centre * t)
    fc, fs = (lambda s: np.cos(w * s + phase)), (lambda s: np.sin(w * s + phase))
    M = max(order(fc, _guess(abs(h * t)), tol), order(fs, _guess(abs(h * t)), tol))
    return np.stack([coefficients(fc, M), coefficients(fs, M)])


def time_evolve(L, ndown, bonds, p, psi, t, bounds, dtype=np.float64, tol=1e-15):
    """e^{-iHt} psi for psi (n, R) real or complex: (C p + S q) + i (C q - S p)"""
    psi = np.asarray(psi)
    R = psi.shape[1]
    block = np.concatenate([psi.real, psi.imag], axis=1) if np.iscomplexobj(psi) else psi
    C, S = chebyshev_apply(L, ndown, bonds, p, block, evolution_coefficients(t, bounds, tol), bounds, dtype)
    if block.shape[1] == R:
        return C - 1j * S
    return (C[:, :R] + S[:, R:]) + 1j * (C[:, R:] - S[:, :R])


def spectral_bounds(L, ndown, bonds, p, k=60, margin=0.05, seed=0):
    n = math.comb(L, ndown)
    k = min(k, n)
    norm2, alphas, betas, steps = blockref.block_lanczos(L, ndown, bonds, p, blockref.start_block(n, 1, seed), k)
    theta, _ = blockref.measure(alphas[:, 0], betas[:, 0], max(1, steps[0]), norm2[0])
    pad = margin * (theta[-1] - theta[0])
    if not pad > 0:
        pad = max(1.0, abs(theta[0])) * margin
    B = blockref.coupling_bound(L, bonds, p)
    return max(theta[0] - pad, -B), min(theta[-1] + pad, B)


def all_pairs(L):
    return tuple((i, j) for i in range(L) for j in range(i + 1, L))


def correlations(L, ndown, v):
    """(xy [L, L], zz [L, L], z [L]) of the sector vector v: v^T (X_i X_j + Y_i Y_j) v, v^T Z_i Z_j v (diagonals 2 v.v and v.v)
    and v^T Z_i v"""
    v = np.asarray(v, dtype=np.float64)
    pairs = all_pairs(L)
    f = ref.forms(L, ndown, pairs, v, v)
    norm2 = float(v @ v)
    xy, zz = 2.0 * norm2 * np.eye(L), norm2 * np.eye(L)
    for t, (i, j) in enumerate(pairs):
        xy[i, j] = xy[j, i] = f[t]
        zz[i, j] = zz[j, i] = f[len(pairs) + t]
    return xy, zz, f[2 * len(pairs):]


def _dense_sector(L, ndown, bonds, p, betas):
    theta, V = np.linalg.eigh(ref.dense(L, ndown, bonds, p))
    parts = [correlations(L, ndown, V[:, j]) for j in range(len(theta))]
    logw = -betas[:, None] * theta[None, :]
    top = logw.max(axis=1)
    w = np.exp(logw - top[:, None])
    prob = w / w.sum(axis=1)[:, None]
    return (top + np.log(w.sum(axis=1)), prob @ theta) + tuple(
        np.einsum("bj,j...->b...", prob, np.stack([q[i] for q in parts])) for i in range(3))


def tpq_sector(L, ndown, bonds, p, betas, Phi, bounds, dtype=np.float64, tol=1e-15):
    """(log weight [B], E [B], xy, zz, z) of one sector from the thermal pure quantum states of the columns of Phi: stepped
    from beta to beta by ``expm`` over half the difference, renormalised, log norms kept aside; column j weighs
    exp(2 log norm_j), the sector (n / R) times their sum"""
    Phi = np.asarray(Phi, dtype=dtype)
    n, R = Phi.shape
    Phi = Phi / np.sqrt(np.einsum("rj,rj->j", Phi, Phi))
    lognorm = np.zeros(R)
    out = [[] for _ in range(5)]
    before = 0.0
    for beta in betas:
        tau = 0.5 * (beta - before)
        before = beta
        Y, shift = expm(L, ndown, bonds, p, Phi, tau, bounds, dtype, tol)
        norms = np.sqrt(np.einsum("rj,rj->j", Y, Y))
        Phi = Y / norms
        lognorm = lognorm + np.log(norms.astype(np.float64)) - tau * shift
        energy = np.einsum("rj,rj->j", Phi, blockref.apply_block(L, ndown, bonds, p, Phi, dtype)).astype(np.float64)
        parts = [correlations(L, ndown, Phi[:, j]) for j in range(R)]
        top = 2.0 * lognorm.max()
        w = np.exp(2.0 * lognorm - top)
        out[0].append(math.log(n / R) + top + math.log(w.sum()))
        out[1].append((w * energy).sum() / w.sum())
        for i in range(3):
            out[2 + i].append(np.einsum("j,j...->...", w, np.stack([q[i] for q in parts])) / w.sum())
    return tuple(np.array(o) for o in out)


def thermal_correlations(L, bonds, p, betas, R=8, seed=0, dense_below=256, dtype=np.float64, tol=1e-15):
    """dict of logZ [B], energy [B], xy [B, L, L], zz [B, L, L], z [B, L] over all sectors, the two one-state sectors included"""
    betas = np.asarray(betas, dtype=np.float64)
    B = len(betas)
    parts = []
    for ndown in range(L + 1):
        if ndown in (0, L):
            e = blockref.edge_energy(L, bonds, p, ndown)
            sign = 1.0 if ndown == 0 else -1.0
            parts.append((-betas * e, np.full(B, e), np.broadcast_to(2.0 * np.eye(L), (B, L, L)), np.ones((B, L, L)),
                          sign * np.ones((B, L))))
            continue
        n = math.comb(L, ndown)
        if n <= dense_below:
            parts.append(_dense_sector(L, ndown, bonds, p, betas))
        else:
            parts.append(tpq_sector(L, ndown, bonds, p, betas, blockref.start_block(n, R, seed),
                                    spectral_bounds(L, ndown, bonds, p, seed=seed), dtype, tol))
    logw = np.stack([q[0] for q in parts])
    top = logw.max(axis=0)
    logZ = top + np.log(np.exp(logw - top).sum(axis=0))
    prob = np.exp(logw - logZ)
    mix = lambda i: sum(prob[s].reshape((B,) + (1,) * (parts[s][i].ndim - 1)) * parts[s][i] for s in range(len(parts)))  # noqa: E731
    return {"logZ": logZ, "energy": mix(1), "xy": mix(2), "zz": mix(3), "z": mix(4)}


def full_space_correlations(L, bonds, p, betas):
    """the same dict from the dense 2^L x 2^L Hamiltonian and dense operators (site i = bit i, Z = +1 on a clear bit):
    tr(e^{-beta H} A) / tr e^{-beta H}"""
    jxy, jz, hz = ref.split(L, bonds, p)
    I2, Z = np.eye(2), np.diag([1.0, -1.0])
    up = np.array([[0.0, 1.0], [0.0, 0.0]])             # |0><1|: clears the bit

    def site(ops):
        out = np.ones((1, 1))
        for i in range(L - 1, -1, -1):                  # (site 0 is the last factor: the lowest bit)
            out = np.kron(out, ops.get(i, I2))
        return out

    def xy_op(i, j):
        flip = site({i: up, j: up.T})
        return 2.0 * (flip + flip.T)

    H = sum(hz[i] * site({i: Z}) for i in range(L))
    for t, (a, b) in enumerate(bonds):
        H = H + jxy[t] * xy_op(a, b) + jz[t] * site({a: Z, b: Z})
    theta, V = np.linalg.eigh(H)
    betas = np.asarray(betas, dtype=np.float64)
    logw = -betas[:, None] * theta[None, :]
    top = logw.max(axis=1)
    w = np.exp(logw - top[:, None])
    prob = w / w.sum(axis=1)[:, None]
    expect = lambda A: prob @ np.einsum("rj,rj->j", V, A @ V)  # noqa: E731
    B = len(betas)
    xy, zz = np.zeros((B, L, L)), np.zeros((B, L, L))
    for i in range(L):
        xy[:, i, i], zz[:, i, i] = 2.0, 1.0
        for j in range(i + 1, L):
            xy[:, i, j] = xy[:, j, i] = expect(xy_op(i, j))
            zz[:, i, j] = zz[:, j, i] = expect(site({i: Z, j: Z}))
    z = np.stack([expect(site({i: Z})) for i in range(L)], axis=1)
    return {"logZ": top + np.log(w.sum(axis=1)), "energy": prob @ theta, "xy": xy, "zz": zz, "z": z}
