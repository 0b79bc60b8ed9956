"""numpy twin of the block Hubbard ladder maps and of the finite-temperature correlation functions built on them
(docs/design/37-hubbard-finite-temperature-dynamics.md); no GPU, no torch.  Thin: built on ``hubbard_ladder_reference`` (the row
formula of the map and its partner lists), ``hubbard_reference`` (the Hamiltonian, the Jordan-Wigner operators),
``hubbard_cheb_reference`` (the Chebyshev recurrences on the Hubbard mat-vec) and ``ladder_block_reference`` (the evolution
coefficients, the windowed transform).  Every function that sums takes a ``dtype`` (``numpy.float64`` or ``numpy.longdouble``).

    apply_block(L, nup, ndn, species, step, w, X, dtype)   S(w) X for X (n_src, R)
    dots(L, nup, ndn, species, step, w, Lft, X, dtype)     d[j] = sum_r Lft[r, j] (S(w) X)[r, j]
    channel_apply / channel_dots / channel_dense           the same for a channel name: "n" and "sz" add both species' step-0 maps
    sampled_pair(...)                                      (log weight [B], C [B, K + 1], orders [B, K + 1]) of one pair from the
                                                           columns of a given start block
    dense_pair(...)                                        (log weight [B], C [B, K + 1]) of one pair from dense eigh
    thermal_dynamics(L, bonds, p, parts, channel, betas, mus, dt, steps, ...)   dict of logXi [B, M], C [B, M, K + 1], orders
    full_space(L, bonds, p, parts, channel, betas, mus, times)                  the same from the 4^L Fock space (L <= 4)
"""
import math

import numpy as np

import hubbard_block_reference as blockref
import hubbard_cheb_reference as hcheb
import hubbard_ladder_reference as ladref
import hubbard_reference as hub
import ladder_block_reference as spin_twin
import sector_cheb_reference as cheb

LD = np.longdouble
UP, DN = ladref.UP, ladref.DN
# channel -> [(species, step, sign)]
CHANNELS = {"c_up": [(UP, -1, 1.0)], "c_dn": [(DN, -1, 1.0)], "cdag_up": [(UP, 1, 1.0)], "cdag_dn": [(DN, 1, 1.0)],
            "n": [(UP, 0, 1.0), (DN, 0, 1.0)], "sz": [(UP, 0, 1.0), (DN, 0, -1.0)]}
spectrum = spin_twin.spectrum


def apply_block(L, nup, ndn, species, step, w, X, dtype=np.float64):
    """S(w) X: ``hubbard_ladder_reference.apply`` column by column in float64, the same row formula on its partner lists in
    ``dtype``"""
    X = np.asarray(X)
    if dtype == np.float64:
        return np.stack([ladref.apply(L, nup, ndn, species, step, w, X[:, j]) for j in range(X.shape[1])], axis=1)
    w, X = np.asarray(w, dtype=dtype), X.astype(dtype)
    src, dst = ladref._shapes(L, nup, ndn, species, step)
    R = X.shape[1]
    assert w.shape == (L,) and X.shape[0] == src[0] * src[1]
    X3, Y = X.reshape(src + (R,)), np.zeros(dst + (R,), dtype=dtype)
    g = dtype(ladref._sector_sign(nup, species, step))
    for i, (rows, cols, f) in enumerate(ladref._partners(L, nup if species == UP else ndn, step)):
        f = f.astype(dtype)
        if species == UP:
            Y[rows] += w[i] * f[:, None, None] * X3[cols]
        else:
            Y[:, rows] += (g * w[i]) * f[None, :, None] * X3[:, cols]
    return Y.reshape(dst[0] * dst[1], R)


def dots(L, nup, ndn, species, step, w, Lft, X, dtype=np.float64):
    return np.einsum("rj,rj->j", np.asarray(Lft).astype(dtype), apply_block(L, nup, ndn, species, step, w, X, dtype))


def destination(L, nup, ndn, channel):
    """(nup, ndn) of the destination of a channel, None when a count would leave 0 .. L"""
    species, step, _ = CHANNELS[channel][0]
    a, b = ladref.destination(nup, ndn, species, step)
    return (a, b) if 0 <= a <= L and 0 <= b <= L else None


def channel_apply(L, nup, ndn, channel, w, X, dtype=np.float64):
    return sum(dtype(sign) * apply_block(L, nup, ndn, species, step, w, X, dtype) for species, step, sign in CHANNELS[channel])


def channel_dots(L, nup, ndn, channel, w, Lft, X, dtype=np.float64):
    return np.einsum("rj,rj->j", np.asarray(Lft).astype(dtype), channel_apply(L, nup, ndn, channel, w, X, dtype))


def channel_dense(L, nup, ndn, channel, w):
    return sum(sign * ladref.dense(L, nup, ndn, species, step, w) for species, step, sign in CHANNELS[channel])


def spectral_bounds(L, nup, ndn, bonds, p, k=60, margin=0.05, seed=0):
    """``chebyshev.spectral_bounds`` on the Hubbard twin"""
    n = math.comb(L, nup) * math.comb(L, ndn)
    k = min(k, n)
    norm2, alphas, betas, steps = blockref.block_lanczos(L, nup, ndn, bonds, p, blockref.start_block(n, 1, seed), k)
    theta, _ = blockref.measure(alphas[:, 0], betas[:, 0], max(1, steps[0]), norm2[0])
    pad = margin * (theta[-1] - theta[0])
    if not pad > 0:
        pad = max(1.0, abs(theta[0])) * margin
    B = blockref.coupling_bound(L, bonds, p)
    return max(theta[0] - pad, -B), min(theta[-1] + pad, B)


def _expm(L, nup, ndn, bonds, p, X, tau, bounds, dtype, tol):
    a, b = float(bounds[0]), float(bounds[1])
    if tau == 0:
        return np.array(X, dtype=dtype), a
    x = tau * 0.5 * (b - a)
    coeffs = cheb.coefficients(cheb.exp_function(x), cheb.exp_order(x, tol))
    return hcheb.chebyshev_apply(L, nup, ndn, bonds, p, X, coeffs, bounds, dtype), a


def _evolve(L, nup, ndn, bonds, p, re, im, dt, bounds, dtype, tol):
    """(re, im) of e^{-iH dt} (re + i im): the (re | im) block through one two-row expansion, as ``chebyshev.time_evolve``"""
    R = re.shape[1]
    C, S = hcheb.chebyshev_apply(L, nup, ndn, bonds, p, np.concatenate([re, im], axis=1),
                                 spin_twin._evolution(dt, tuple(bounds), tol), bounds, dtype)
    return C[:, :R] + S[:, R:], C[:, R:] - S[:, :R]


def sampled_pair(L, nup, ndn, channel, bonds, p, parts, betas, dt, steps, Phi, bounds_src, bounds_dst, weight=None,
                 dtype=np.float64, tol=1e-15):
    """One pair from the columns of ``Phi`` (n_src, R) as thermal pure quantum states: stepped from beta to beta by the
    Chebyshev expansion of e^{-tau H} and renormalised, log norms aside; per real part w of the weights b_0 = Phi, a_0 = A Phi,
    both stepped by dt, C_j(t_k) = <A b_k,j | a_k,j>.  The pair weighs ``weight`` (default n_src / R) times sum_j
    exp(2 log norm_j).  Returns (log weight [B], C [B, K + 1] complex, orders [B, K + 1]): the Chebyshev orders a column has been
    through."""
    Phi = np.asarray(Phi, dtype=dtype)
    n, R = Phi.shape
    weight = n / R if weight is None else weight
    other = destination(L, nup, ndn, channel)
    Phi = Phi / np.sqrt(np.einsum("rj,rj->j", Phi, Phi))
    per_step = max(spin_twin._evolution(dt, tuple(bounds_src), tol).shape[1], spin_twin._evolution(dt, tuple(bounds_dst), tol).shape[1])
    lognorm, before, spent = np.zeros(R), 0.0, 0
    logw, rows, orders = [], [], []
    for beta in betas:
        tau = 0.5 * (beta - before)
        before = beta
        if tau > 0:
            spent += cheb.exp_order(tau * 0.5 * (bounds_src[1] - bounds_src[0]), tol)
        Y, shift = _expm(L, nup, ndn, bonds, p, Phi, tau, bounds_src, dtype, tol)
        norms = np.sqrt(np.einsum("rj,rj->j", Y, Y))
        Phi = Y / norms
        lognorm = lognorm + np.log(norms.astype(np.float64)) - tau * shift
        top = 2.0 * lognorm.max()
        w = np.exp(2.0 * lognorm - top)
        Cj = np.zeros((steps + 1, R), dtype=np.complex128)
        for c in parts:
            b_re, b_im = Phi, np.zeros_like(Phi)
            a_re = channel_apply(L, nup, ndn, channel, c, Phi, dtype)
            a_im = np.zeros_like(a_re)
            for k in range(steps + 1):
                if k:
                    b_re, b_im = _evolve(L, nup, ndn, bonds, p, b_re, b_im, dt, bounds_src, dtype, tol)
                    a_re, a_im = _evolve(L, other[0], other[1], bonds, p, a_re, a_im, dt, bounds_dst, dtype, tol)
                d = lambda l, x: channel_dots(L, nup, ndn, channel, c, l, x, dtype)  # noqa: E731
                Cj[k] += ((d(a_re, b_re) + d(a_im, b_im)) + 1j * (d(a_im, b_re) - d(a_re, b_im))).astype(np.complex128)
        logw.append(math.log(weight) + top + math.log(w.sum()))
        rows.append((Cj * w).sum(axis=1) / w.sum())
        orders.append(spent + per_step * np.arange(steps + 1))
    return np.array(logw), np.array(rows), np.array(orders)


def _is_edge(L, pair):
    return pair[0] in (0, L) or pair[1] in (0, L)


def _spectrum_of(L, nup, ndn, bonds, p):
    """(theta, V) in the row order ru * n_dn + rd: an edge side from ``edge_matrix`` of the species that is not frozen"""
    if nup in (0, L) and ndn in (0, L):
        return np.array([blockref.edge_matrix(L, bonds, p, nup, ndn == L)[0, 0]]), np.ones((1, 1))
    if nup in (0, L) or ndn in (0, L):
        count, other = (ndn, nup) if nup in (0, L) else (nup, ndn)
        return np.linalg.eigh(blockref.edge_matrix(L, bonds, p, count, other == L))
    return np.linalg.eigh(hub.dense(L, nup, ndn, bonds, p))


def dense_pair(L, nup, ndn, channel, bonds, p, parts, betas, times):
    """(log weight [B], C [B, K + 1]) from the spectra of both sides: C(t) = sum_{n, m} p_n sum_parts |<m|A|n>|^2 e^{-i (E_m - E_n) t};
    a destination that does not exist gives C = 0"""
    betas, times = np.asarray(betas, dtype=np.float64), np.asarray(times, dtype=np.float64)
    theta, V = _spectrum_of(L, nup, ndn, bonds, p)
    logw = -betas[:, None] * theta[None, :]
    top = logw.max(axis=1)
    logsum = top + np.log(np.exp(logw - top[:, None]).sum(axis=1))
    other = destination(L, nup, ndn, channel)
    if other is None:
        return logsum, np.zeros((len(betas), len(times)), dtype=np.complex128)
    prob = np.exp(logw - logsum[:, None])
    theta2, V2 = (theta, V) if other == (nup, ndn) else _spectrum_of(L, other[0], other[1], bonds, p)
    W = sum((V2.T @ channel_dense(L, nup, ndn, channel, c) @ V) ** 2 for c in parts)          # [m, n]
    gap = theta2[:, None] - theta[None, :]
    return logsum, np.einsum("bn,mn,kmn->bk", prob, W, np.exp(-1j * times[:, None, None] * gap[None, :, :]))


def combine(out, sectors, betas, mus):
    """(logXi [B, M], C [B, M, K + 1]) of per-source (log weight [B], C [B, K + 1]) with the weights e^{beta mu N_src}"""
    betas, mus = np.asarray(betas, dtype=np.float64), np.asarray(mus, dtype=np.float64)
    N = np.array([a + b for a, b in sectors], dtype=np.float64)
    logw = np.stack([q[0] for q in out])[:, :, None] + betas[None, :, None] * mus[None, None, :] * N[:, None, None]
    top = logw.max(axis=0)
    logXi = top + np.log(np.exp(logw - top).sum(axis=0))
    prob = np.exp(logw - logXi)
    return logXi, sum(prob[s][:, :, None] * out[s][1][:, None, :] for s in range(len(out)))


def thermal_dynamics(L, bonds, p, parts, channel, betas, mus, dt, steps, R=8, seed=0, dense_below=256, sectors=None,
                     dtype=np.float64, tol=1e-15):
    """dict of logXi [B, M], C [B, M, K + 1] (complex) and orders [B, K + 1] (the most Chebyshev orders any sampled column has been
    through, 0 where every pair is dense) over the source pairs; the routes are those of ``thermal.hubbard_thermal_dynamics``"""
    betas = np.asarray(betas, dtype=np.float64)
    times = dt * np.arange(steps + 1)
    sectors = [(a, b) for a in range(L + 1) for b in range(L + 1)] if sectors is None else list(sectors)
    out, orders = [], np.zeros((len(betas), steps + 1))
    rows = lambda pair: math.comb(L, pair[0]) * math.comb(L, pair[1])  # noqa: E731
    for pair in sectors:
        other = destination(L, pair[0], pair[1], channel)
        if other is None or _is_edge(L, pair) or _is_edge(L, other) or max(rows(pair), rows(other)) <= dense_below:
            out.append(dense_pair(L, pair[0], pair[1], channel, bonds, p, parts, betas, times))
            continue
        bounds_src = spectral_bounds(L, pair[0], pair[1], bonds, p, seed=seed)
        bounds_dst = bounds_src if other == pair else spectral_bounds(L, other[0], other[1], bonds, p, seed=seed)
        logw, C, spent = sampled_pair(L, pair[0], pair[1], channel, bonds, p, parts, betas, dt, steps,
                                      blockref.start_block(rows(pair), R, seed), bounds_src, bounds_dst, dtype=dtype, tol=tol)
        out.append((logw, C))
        orders = np.maximum(orders, spent)
    logXi, C = combine(out, sectors, betas, mus)
    return {"logXi": logXi, "C": C, "orders": orders}


def fock_operators(L):
    """the 2 L Jordan-Wigner annihilators of ``hubbard_reference`` (mode i: (i, up), mode L + i: (i, dn)) on the 4^L space"""
    assert L <= 4
    return [hub._annihilator(2 * L, j) for j in range(2 * L)]


def fock_hamiltonian(L, bonds, p):
    """(H, N) on the 4^L space, as ``hubbard_reference.dense_jordan_wigner`` builds H before it restricts it"""
    t, V, U, eps = hub.split(L, bonds, p)
    c = fock_operators(L)
    num = [cj.T @ cj for cj in c]
    H = np.zeros((1 << (2 * L), 1 << (2 * L)))
    for k, (a, b) in enumerate(bonds):
        for off in (0, L):
            hop = c[a + off].T @ c[b + off]
            H -= t[k] * (hop + hop.T)
        H += V[k] * (num[a] + num[a + L]) @ (num[b] + num[b + L])
    for i in range(L):
        H += U[i] * num[i] @ num[i + L] + eps[i] * (num[i] + num[i + L])
    return H, sum(num)


def fock_channel(L, channel, w):
    """A = sum_i w_i O_i of a channel on the 4^L space"""
    c = fock_operators(L)
    site = {"c_up": lambda i: c[i], "c_dn": lambda i: c[L + i], "cdag_up": lambda i: c[i].T, "cdag_dn": lambda i: c[L + i].T,
            "n": lambda i: c[i].T @ c[i] + c[L + i].T @ c[L + i], "sz": lambda i: c[i].T @ c[i] - c[L + i].T @ c[L + i]}[channel]
    return sum(w[i] * site(i) for i in range(L))


def full_space(L, bonds, p, parts, channel, betas, mus, times):
    """(logXi [B, M], C [B, M, K + 1]) = tr[e^{-beta (H - mu N)} e^{iHt} A^T e^{-iHt} A] / Xi over all 4^L states.  H and N
    commute; the eigenvectors of H + x N for an x that lifts the degeneracies between particle numbers are joint ones."""
    H, N = fock_hamiltonian(L, bonds, p)
    x = 0.3819660112501051
    kappa, V = np.linalg.eigh(H + x * N)
    num = np.rint(np.einsum("an,ab,bn->n", V, N, V))
    assert np.abs(V.T @ N @ V - np.diag(num)).max() <= 1e-9
    theta = kappa - x * num
    W = sum((V.T @ fock_channel(L, channel, c) @ V) ** 2 for c in parts)                         # [m, n]
    gap = theta[:, None] - theta[None, :]
    phase = np.exp(-1j * np.asarray(times)[:, None, None] * gap[None, :, :])
    logXi, C = np.zeros((len(betas), len(mus))), np.zeros((len(betas), len(mus), len(times)), dtype=np.complex128)
    for b, beta in enumerate(betas):
        for m, mu in enumerate(mus):
            logw = -beta * (theta - mu * num)
            top = logw.max()
            wgt = np.exp(logw - top)
            logXi[b, m] = top + math.log(wgt.sum())
            C[b, m] = np.einsum("n,mn,kmn->k", wgt / wgt.sum(), W, phase)
    return logXi, C
