"""numpy twin of the block current map of a Hubbard sector, of its column dots and of the finite-temperature optical response
built on them (docs/design/40-finite-temperature-conductivity.md); no GPU, no torch.  Thin: built on ``hubbard_current_reference``
(the row formula of K(w), the Peierls Hamiltonian), ``hubbard_reference`` (the Hamiltonian, the partner lists, the Jordan-Wigner
operators) and ``hubbard_ladder_block_reference`` (the Chebyshev recurrences of the sampled estimator, the 4^L Fock space).  Every
function that sums takes a ``dtype`` (``numpy.float64`` or ``numpy.longdouble``).

    apply_block(L, nup, ndn, bonds, w, X, dtype)          K(w) X for X (n, R)
    dots(L, nup, ndn, bonds, w, Lft, X, dtype)            d[j] = sum_r Lft[r, j] (K(w) X)[r, j]
    current_weights(t, d, kind)                           w (2, nb) = t_t d_t on up, +- t_t d_t on dn
    dense_current / dense_diamagnetic                     K(w) and T_d = sum_t td2_t sum_s (hop_t + h.c.) on sector states, edge
                                                          sectors included
    g(beta, x)                                            (1 - e^{-beta x}) / x, beta at x = 0
    dense_sector(...)                                     (log weight [B], C [B, K + 1], K_d [B], X [B], (theta, p W)) of one sector
    thermal(L, bonds, p, d, kind, betas, mus, times)      dict of logXi, C, K_d, X over the sectors, all by default
    full_space(L, bonds, p, d, kind, betas, mus, times)   the same from the 4^L Fock space by Jordan-Wigner (L <= 4)
    free_energy(L, bonds, p, d, phi, beta, mu)            F(phi) = -ln Xi / beta of the complex H(phi) on the Fock space
    broadened(L, bonds, p, d, kind, betas, mus, omega, eta)   S_eta, sigma_reg, weight and stiffness with exact Gaussians
    sampled_sector(...)                                   (log weight, C, orders, K_d) of one sector from given start vectors
    sampled(L, bonds, p, d, kind, betas, mus, dt, steps, sectors, R, seed, dtype)   the listed sectors sampled and mixed
"""
import math

import numpy as np

import hubbard_current_reference as cref
import hubbard_ladder_block_reference as hlb
import hubbard_reference as hub
import ladder_block_reference as spin_twin
import sector_cheb_reference as cheb

LD = np.longdouble


def apply_block(L, nup, ndn, bonds, w, X, dtype=np.float64):
    """K(w) X: ``hubbard_current_reference.apply`` column by column in float64, the same row formula on its partner lists in
    ``dtype``"""
    X = np.asarray(X)
    w = cref.weights(w, len(bonds))
    if dtype == np.float64:
        return np.stack([cref.apply(L, nup, ndn, bonds, w, X[:, j]) for j in range(X.shape[1])], axis=1)
    n_up, n_dn = len(hub.states(L, nup)), len(hub.states(L, ndn))
    R = X.shape[1]
    w = w.astype(dtype)
    X3, Y = X.astype(dtype).reshape(n_up, n_dn, R), np.zeros((n_up, n_dn, R), dtype=dtype)
    up, dn = hub._partners(L, nup, bonds), hub._partners(L, ndn, bonds)
    ou, od = cref._orient(L, nup, bonds), cref._orient(L, ndn, bonds)
    for t in range(len(bonds)):
        rows, cols, sgn = up[t]
        Y[rows] += w[0, t] * (ou[t] * sgn).astype(dtype)[:, None, None] * X3[cols]
        rows, cols, sgn = dn[t]
        Y[:, rows] += w[1, t] * (od[t] * sgn).astype(dtype)[None, :, None] * X3[:, cols]
    return Y.reshape(n_up * n_dn, R)


def dots(L, nup, ndn, bonds, w, Lft, X, dtype=np.float64):
    return np.einsum("rj,rj->j", np.asarray(Lft).astype(dtype), apply_block(L, nup, ndn, bonds, w, X, dtype))


def current_weights(t, d, kind="charge"):
    wt = np.asarray(t, dtype=np.float64) * np.asarray(d, dtype=np.float64)
    return np.stack([wt, wt if kind == "charge" else -wt])


def dense_current(L, nup, ndn, bonds, w):
    return cref.dense(L, nup, ndn, bonds, w)


def dense_diamagnetic(L, nup, ndn, bonds, td2):
    """T_d: the Hamiltonian of ``hubbard_reference`` with t = -td2 and V = U = eps = 0"""
    p = np.zeros(hub.nparam(L, bonds))
    p[:len(bonds)] = -np.asarray(td2, dtype=np.float64)
    return hub.dense(L, nup, ndn, bonds, p)


def g(beta, x):
    x = np.asarray(x, dtype=np.float64)
    safe = np.where(x == 0, 1.0, x)
    return np.where(x == 0, beta, -np.expm1(-beta * x) / safe)


def _logsumexp(a, axis):
    top = a.max(axis=axis)
    return top + np.log(np.exp(a - np.expand_dims(top, axis)).sum(axis=axis))


def dense_sector(L, nup, ndn, bonds, p, d, kind, betas, times):
    """(log weight [B], C [B, K + 1], K_d [B], X [B], theta, W [m, n]) of the sector from dense ``eigh``"""
    betas, times = np.asarray(betas, dtype=np.float64), np.asarray(times, dtype=np.float64)
    t = hub.split(L, bonds, p)[0]
    d = np.asarray(d, dtype=np.float64)
    theta, V = np.linalg.eigh(hub.dense(L, nup, ndn, bonds, p))
    logw = -betas[:, None] * theta[None, :]
    logsum = _logsumexp(logw, 1)
    prob = np.exp(logw - logsum[:, None])
    W = (V.T @ dense_current(L, nup, ndn, bonds, current_weights(t, d, kind)) @ V) ** 2           # [m, n]
    gap = theta[:, None] - theta[None, :]
    C = np.einsum("bn,mn,kmn->bk", prob, W, np.exp(-1j * times[:, None, None] * gap[None, :, :]))
    kinetic = np.einsum("rn,rs,sn->n", V, dense_diamagnetic(L, nup, ndn, bonds, t * d * d), V)
    X = np.array([np.sum(prob[b][None, :] * W * g(beta, gap)) for b, beta in enumerate(betas)])
    return logsum, C, prob @ kinetic, X, theta, W


def _mix(out, sectors, betas, mus):
    betas, mus = np.asarray(betas, dtype=np.float64), np.asarray(mus, dtype=np.float64)
    N = np.array([a + b for a, b in sectors], dtype=np.float64)
    logw = np.stack([q[0] for q in out])[:, :, None] + betas[None, :, None] * mus[None, None, :] * N[:, None, None]
    logXi = _logsumexp(logw, 0)
    return logXi, np.exp(logw - logXi)


def thermal(L, bonds, p, d, kind, betas, mus, times, sectors=None):
    """dict of logXi [B, M], C [B, M, K + 1], K_d [B, M] and X [B, M], every sector dense"""
    sectors = [(a, b) for a in range(L + 1) for b in range(L + 1)] if sectors is None else list(sectors)
    out = [dense_sector(L, a, b, bonds, p, d, kind, betas, times) for a, b in sectors]
    logXi, prob = _mix(out, sectors, betas, mus)
    return {"logXi": logXi, "C": sum(prob[s][:, :, None] * out[s][1][:, None, :] for s in range(len(out))),
            "K_d": sum(prob[s] * out[s][2][:, None] for s in range(len(out))),
            "X": sum(prob[s] * out[s][3][:, None] for s in range(len(out)))}


def _fock_hops(L, bonds):
    """per bond and species the matrix of c+_{a s} c_{b s} on the 4^L space"""
    c = hlb.fock_operators(L)
    return [[c[a + off].T @ c[b + off] for off in (0, L)] for a, b in bonds]


def full_space(L, bonds, p, d, kind, betas, mus, times):
    """the dict of ``thermal`` from tr over all 4^L states; the joint eigenvectors of H and N as in
    ``hubbard_ladder_block_reference.full_space``"""
    t = hub.split(L, bonds, p)[0]
    d = np.asarray(d, dtype=np.float64)
    w = current_weights(t, d, kind)
    H, N = hlb.fock_hamiltonian(L, bonds, p)
    hops = _fock_hops(L, bonds)
    K = sum(w[s, k] * (hops[k][s] - hops[k][s].T) for k in range(len(bonds)) for s in (0, 1))
    Td = sum(t[k] * d[k] ** 2 * (hops[k][s] + hops[k][s].T) for k in range(len(bonds)) for s in (0, 1))
    x = 0.3819660112501051
    kappa, V = np.linalg.eigh(H + x * N)
    num = np.rint(np.einsum("an,ab,bn->n", V, N, V))
    assert np.abs(V.T @ N @ V - np.diag(num)).max() <= 1e-9
    theta = kappa - x * num
    W = (V.T @ K @ V) ** 2
    kinetic = np.einsum("rn,rs,sn->n", V, Td, V)
    gap = theta[:, None] - theta[None, :]
    phase = np.exp(-1j * np.asarray(times)[:, None, None] * gap[None, :, :])
    shape = (len(betas), len(mus))
    out = {"logXi": np.zeros(shape), "C": np.zeros(shape + (len(times),), dtype=np.complex128), "K_d": np.zeros(shape),
           "X": np.zeros(shape)}
    for b, beta in enumerate(betas):
        for m, mu in enumerate(mus):
            logw = -beta * (theta - mu * num)
            top = logw.max()
            pr = np.exp(logw - top)
            out["logXi"][b, m] = top + math.log(pr.sum())
            pr = pr / pr.sum()
            out["C"][b, m] = np.einsum("n,mn,kmn->k", pr, W, phase)
            out["K_d"][b, m] = pr @ kinetic
            out["X"][b, m] = np.sum(pr[None, :] * W * g(beta, gap))
    return out


def free_energy(L, bonds, p, d, phi, beta, mu):
    """F(phi) = -ln tr e^{-beta (H(phi) - mu N)} / beta on the 4^L space, H(phi) with t_t -> t_t e^{i phi d_t} on c+_a c_b"""
    nb = len(bonds)
    t = hub.split(L, bonds, p)[0]
    q = np.array(p, dtype=np.float64)
    q[:nb] = 0.0
    H0, N = hlb.fock_hamiltonian(L, bonds, q)
    H = H0.astype(np.complex128)
    for k, pair in enumerate(_fock_hops(L, bonds)):
        z = np.exp(1j * phi * d[k])
        for hop in pair:
            H -= t[k] * (z * hop + np.conj(z) * hop.T)
    lam = np.linalg.eigvalsh(H - mu * N)
    top = (-beta * lam).max()
    return -(top + math.log(np.exp(-beta * lam - top).sum())) / beta


def broadened(L, bonds, p, d, kind, betas, mus, omega, eta):
    """dict of S [B, M, W], regular, weight [B, M] and stiffness [B, M] with every delta(omega - (E_m - E_n)) an exact Gaussian
    of width eta, ``weight`` the trapezoid sum over the uniform grid ``omega``"""
    betas, omega = np.asarray(betas, dtype=np.float64), np.asarray(omega, dtype=np.float64)
    sectors = [(a, b) for a in range(L + 1) for b in range(L + 1)]
    out = [dense_sector(L, a, b, bonds, p, d, kind, betas, np.zeros(1)) for a, b in sectors]
    logXi, prob = _mix(out, sectors, betas, mus)
    S = np.zeros((len(betas), len(mus), len(omega)))
    for s, (logsum, _, _, _, theta, W) in enumerate(out):
        gap = (theta[:, None] - theta[None, :]).reshape(-1)
        gauss = np.exp(-0.5 * ((omega[:, None] - gap[None, :]) / eta) ** 2) / (eta * math.sqrt(2.0 * math.pi))   # [W, mn]
        pn = np.exp(-betas[:, None] * theta[None, :] - logsum[:, None])                                          # [B, n]
        per_beta = np.stack([gauss @ (pn[b][None, :] * W).reshape(-1) for b in range(len(betas))])               # [B, W]
        S += prob[s][:, :, None] * per_beta[:, None, :]
    regular = math.pi * np.stack([g(beta, omega) for beta in betas])[:, None, :] * S
    h = omega[1] - omega[0]
    weight = h * (regular.sum(axis=-1) - 0.5 * (regular[..., 0] + regular[..., -1]))
    K_d = sum(prob[s] * out[s][2][:, None] for s in range(len(out)))
    return {"S": S, "regular": regular, "weight": weight, "K_d": K_d, "stiffness": K_d - weight / math.pi}


def sampled_sector(L, nup, ndn, bonds, p, d, kind, betas, dt, steps, Phi, bounds, dtype=np.float64, tol=1e-15):
    """One sector from the columns of ``Phi`` (n, R) as thermal pure quantum states, as
    ``hubbard_ladder_block_reference.sampled_pair`` with A = K(w) and the destination the sector itself: (log weight [B], C [B, K +
    1] complex, orders [B, K + 1], K_d [B]); K_d of column j is -sum_t t_t d_t^2 phi_j^T (dH / dt_t) phi_j"""
    Phi = np.asarray(Phi, dtype=dtype)
    n, R = Phi.shape
    t = hub.split(L, bonds, p)[0]
    d = np.asarray(d, dtype=np.float64)
    w = current_weights(t, d, kind)
    Phi = Phi / np.sqrt(np.einsum("rj,rj->j", Phi, Phi))
    per_step = spin_twin._evolution(dt, tuple(bounds), tol).shape[1]
    lognorm, before, spent = np.zeros(R), 0.0, 0
    logw, rows, orders, kd = [], [], [], []
    hop_w = np.stack([t * d * d, t * d * d])
    for beta in betas:
        tau = 0.5 * (beta - before)
        before = beta
        if tau > 0:
            spent += cheb.exp_order(tau * 0.5 * (bounds[1] - bounds[0]), tol)
        Y, shift = hlb._expm(L, nup, ndn, bonds, p, Phi, tau, bounds, dtype, tol)
        norms = np.sqrt(np.einsum("rj,rj->j", Y, Y))
        Phi = Y / norms
        lognorm = lognorm + np.log(norms.astype(np.float64)) - tau * shift
        top = 2.0 * lognorm.max()
        cw = np.exp(2.0 * lognorm - top)
        b_re, b_im = Phi, np.zeros_like(Phi)
        a_re = apply_block(L, nup, ndn, bonds, w, Phi, dtype)
        a_im = np.zeros_like(a_re)
        Cj = np.zeros((steps + 1, R), dtype=np.complex128)
        for k in range(steps + 1):
            if k:
                b_re, b_im = hlb._evolve(L, nup, ndn, bonds, p, b_re, b_im, dt, bounds, dtype, tol)
                a_re, a_im = hlb._evolve(L, nup, ndn, bonds, p, a_re, a_im, dt, bounds, dtype, tol)
            dd = lambda l, x: dots(L, nup, ndn, bonds, w, l, x, dtype)  # noqa: E731
            Cj[k] = ((dd(a_re, b_re) + dd(a_im, b_im)) + 1j * (dd(a_im, b_re) - dd(a_re, b_im))).astype(np.complex128)
        # <phi| T_d |phi> = sum_t t_t d_t^2 <hop_t + h.c.>
        Td_phi = _hop_apply(L, nup, ndn, bonds, hop_w, Phi, dtype)
        kin = np.einsum("rj,rj->j", Phi, Td_phi).astype(np.float64)
        logw.append(math.log(n / R) + top + math.log(cw.sum()))
        rows.append((Cj * cw).sum(axis=1) / cw.sum())
        kd.append(float((cw * kin).sum() / cw.sum()))
        orders.append(spent + per_step * np.arange(steps + 1))
    return np.array(logw), np.array(rows), np.array(orders), np.array(kd)


def _hop_apply(L, nup, ndn, bonds, hw, X, dtype):
    """sum_t sum_s hw[s, t] (c+_{a s} c_{b s} + h.c.) X in ``dtype``: the partner lists with sgn_t alone"""
    n_up, n_dn = len(hub.states(L, nup)), len(hub.states(L, ndn))
    R = X.shape[1]
    hw = np.asarray(hw).astype(dtype)
    X3, Y = np.asarray(X).astype(dtype).reshape(n_up, n_dn, R), np.zeros((n_up, n_dn, R), dtype=dtype)
    up, dn = hub._partners(L, nup, bonds), hub._partners(L, ndn, bonds)
    for t in range(len(bonds)):
        rows, cols, sgn = up[t]
        Y[rows] += hw[0, t] * sgn.astype(dtype)[:, None, None] * X3[cols]
        rows, cols, sgn = dn[t]
        Y[:, rows] += hw[1, t] * sgn.astype(dtype)[None, :, None] * X3[:, cols]
    return Y.reshape(n_up * n_dn, R)


def sampled(L, bonds, p, d, kind, betas, mus, dt, steps, sectors, R=8, seed=0, dtype=np.float64, tol=1e-15):
    """dict of logXi [B, M], C [B, M, K + 1], K_d [B, M] and orders [B, K + 1] with every listed (bulk) sector sampled on the start
    vectors and the bounds of ``thermal.hubbard_thermal_conductivity``"""
    import hubbard_block_reference as blockref
    out, orders = [], np.zeros((len(betas), steps + 1))
    for a, b in sectors:
        n = math.comb(L, a) * math.comb(L, b)
        bounds = hlb.spectral_bounds(L, a, b, bonds, p, seed=seed)
        logw, C, spent, kd = sampled_sector(L, a, b, bonds, p, d, kind, betas, dt, steps, blockref.start_block(n, R, seed), bounds,
                                            dtype, tol)
        out.append((logw, C.astype(np.complex128), kd))
        orders = np.maximum(orders, spent)
    logXi, prob = _mix(out, sectors, betas, mus)
    return {"logXi": logXi, "C": sum(prob[s][:, :, None] * out[s][1][:, None, :] for s in range(len(out))),
            "K_d": sum(prob[s] * out[s][2][:, None] for s in range(len(out))), "orders": orders}
