"""numpy twin of the block ladder maps and of the finite-temperature correlation functions built on them
(docs/design/35-finite-temperature-dynamics.md); no GPU, no torch.  Built on ``ladder_reference`` (the row formula of the map),
``sector_block_reference`` (the block mat-vec, the start vectors) and ``sector_cheb_reference`` (the imaginary- and real-time
Chebyshev steps).  Every function that sums takes a ``dtype`` (``numpy.float64`` or ``numpy.longdouble``).

    apply_block(L, ndown_src, step, c, X, dtype)          S(c) X for X (n_src, R)
    dots(L, ndown_src, step, c, Lft, X, dtype)            d[j] = sum_r Lft[r, j] (S(c) X)[r, j]
    sampled_pair(...)                                     (log weight [B], C [B, K + 1], orders [B, K + 1]) of one sector pair from the
                                                          columns of a given start block
    dense_pair(...)                                       (log weight [B], C [B, K + 1]) of one sector pair from dense eigh
    thermal_dynamics(L, bonds, p, parts, step, betas, dt, steps, ...)   dict of logZ, C and orders over the source sectors
    spectrum(times, C, omega, eta)                        the windowed trapezoid transform as a direct sum
"""
import functools
import math

import numpy as np

import ladder_reference as ladref
import sector_block_reference as blockref
import sector_cheb_reference as cheb
import sector_reference as ref

LD = np.longdouble


def apply_block(L, ndown_src, step, c, X, dtype=np.float64):
    """S(c) X: ``ladder_reference.apply`` column by column in float64, the same row formula on its partner lists in ``dtype``"""
    X = np.asarray(X)
    if dtype == np.float64:
        return np.stack([ladref.apply(L, ndown_src, step, c, X[:, j]) for j in range(X.shape[1])], axis=1)
    c, X = np.asarray(c, dtype=dtype), X.astype(dtype)
    n_src, n_dst = ladref.sizes(L, ndown_src, step)
    assert c.shape == (L,) and X.shape[0] == n_src
    if step == 0:
        diag = np.zeros(n_dst, dtype=dtype)
        for i, (_, z) in enumerate(ladref._partners(L, ndown_src, 0)):
            diag += c[i] * z.astype(dtype)
        return diag[:, None] * X
    Y = np.zeros((n_dst, X.shape[1]), dtype=dtype)
    for i, (rows, cols) in enumerate(ladref._partners(L, ndown_src, step)):
        Y[rows] += c[i] * X[cols]
    return Y


def dots(L, ndown_src, step, c, Lft, X, dtype=np.float64):
    return np.einsum("rj,rj->j", np.asarray(Lft).astype(dtype), apply_block(L, ndown_src, step, c, X, dtype))


@functools.lru_cache(maxsize=None)
def _evolution(dt, bounds, tol):
    out = cheb.evolution_coefficients(dt, bounds, tol)
    out.setflags(write=False)
    return out


def _evolve(L, ndown, bonds, p, re, im, dt, bounds, dtype, tol):
    """(re, im) of e^{-iH dt} (re + i im): the (re | im) block through one two-row expansion, as ``chebyshev.time_evolve``"""
    R = re.shape[1]
    C, S = cheb.chebyshev_apply(L, ndown, bonds, p, np.concatenate([re, im], axis=1), _evolution(dt, tuple(bounds), tol), bounds, dtype)
    return C[:, :R] + S[:, R:], C[:, R:] - S[:, :R]


def sampled_pair(L, ndown_src, step, bonds, p, parts, betas, dt, steps, Phi, bounds_src, bounds_dst, weight=None,
                 dtype=np.float64, tol=1e-15):
    """One sector pair from the columns of ``Phi`` (n_src, R) as thermal pure quantum states: stepped from beta to beta by
    ``sector_cheb_reference.expm`` and renormalised, log norms aside; per real part c of the weights b_0 = Phi, a_0 = S(c) Phi, both
    stepped by dt, C_j(t_k) = <S(c) b_k,j | a_k,j>.  The pair weighs ``weight`` (default n_src / R) times sum_j exp(2 log norm_j).
    Returns (log weight [B], C [B, K + 1] complex, orders [B, K + 1]): the Chebyshev orders a column has been through."""
    Phi = np.asarray(Phi, dtype=dtype)
    n, R = Phi.shape
    weight = n / R if weight is None else weight
    nd_dst = ndown_src + step
    Phi = Phi / np.sqrt(np.einsum("rj,rj->j", Phi, Phi))
    per_step = max(_evolution(dt, tuple(bounds_src), tol).shape[1], _evolution(dt, tuple(bounds_dst), tol).shape[1])
    lognorm, before, spent = np.zeros(R), 0.0, 0
    logw, rows, orders = [], [], []
    for beta in betas:
        tau = 0.5 * (beta - before)
        before = beta
        if tau > 0:
            spent += cheb.exp_order(tau * 0.5 * (bounds_src[1] - bounds_src[0]), tol)
        Y, shift = cheb.expm(L, ndown_src, bonds, p, Phi, tau, bounds_src, dtype, tol)
        norms = np.sqrt(np.einsum("rj,rj->j", Y, Y))
        Phi = Y / norms
        lognorm = lognorm + np.log(norms.astype(np.float64)) - tau * shift
        top = 2.0 * lognorm.max()
        w = np.exp(2.0 * lognorm - top)
        Cj = np.zeros((steps + 1, R), dtype=np.complex128)
        for c in parts:
            b_re, b_im = Phi, np.zeros_like(Phi)
            a_re = apply_block(L, ndown_src, step, c, Phi, dtype)
            a_im = np.zeros_like(a_re)
            for k in range(steps + 1):
                if k:
                    b_re, b_im = _evolve(L, ndown_src, bonds, p, b_re, b_im, dt, bounds_src, dtype, tol)
                    a_re, a_im = _evolve(L, nd_dst, bonds, p, a_re, a_im, dt, bounds_dst, dtype, tol)
                d = lambda l, x: dots(L, ndown_src, step, c, l, x, dtype)  # noqa: E731
                Cj[k] += ((d(a_re, b_re) + d(a_im, b_im)) + 1j * (d(a_im, b_re) - d(a_re, b_im))).astype(np.complex128)
        logw.append(math.log(weight) + top + math.log(w.sum()))
        rows.append((Cj * w).sum(axis=1) / w.sum())
        orders.append(spent + per_step * np.arange(steps + 1))
    return np.array(logw), np.array(rows), np.array(orders)


def _spectrum_of(L, ndown, bonds, p):
    if ndown in (0, L):
        return np.array([blockref.edge_energy(L, bonds, p, ndown)]), np.ones((1, 1))
    return np.linalg.eigh(ref.dense(L, ndown, bonds, p))


def dense_pair(L, ndown_src, step, bonds, p, parts, betas, times):
    """(log weight [B], C [B, K + 1]) from the spectra of both sides: C(t) = sum_{n, m} p_n sum_parts |<m|S(c)|n>|^2 e^{-i (E_m - E_n) t};
    a destination that does not exist gives C = 0"""
    betas, times = np.asarray(betas, dtype=np.float64), np.asarray(times, dtype=np.float64)
    theta, V = _spectrum_of(L, ndown_src, bonds, p)
    logw = -betas[:, None] * theta[None, :]
    top = logw.max(axis=1)
    logsum = top + np.log(np.exp(logw - top[:, None]).sum(axis=1))
    if not 0 <= ndown_src + step <= L:
        return logsum, np.zeros((len(betas), len(times)), dtype=np.complex128)
    prob = np.exp(logw - logsum[:, None])
    theta2, V2 = (theta, V) if step == 0 else _spectrum_of(L, ndown_src + step, bonds, p)
    W = sum((V2.T @ ladref.dense(L, ndown_src, step, c) @ V) ** 2 for c in parts)          # [m, n]
    gap = theta2[:, None] - theta[None, :]
    return logsum, np.einsum("bn,mn,kmn->bk", prob, W, np.exp(-1j * times[:, None, None] * gap[None, :, :]))


def thermal_dynamics(L, bonds, p, parts, step, betas, dt, steps, R=8, seed=0, dense_below=256, sectors=None, dtype=np.float64,
                     tol=1e-15):
    """dict of logZ [B], C [B, K + 1] (complex) and orders [B, K + 1] (the most Chebyshev orders any sampled column has been through,
    0 where every pair is dense) over the source sectors; the rule for a dense pair is that of ``thermal.thermal_dynamics``"""
    betas = np.asarray(betas, dtype=np.float64)
    times = dt * np.arange(steps + 1)
    out, orders = [], np.zeros((len(betas), steps + 1))
    for nd in (range(L + 1) if sectors is None else sectors):
        other = nd + step
        exists = 0 <= other <= L
        edge = nd in (0, L) or other in (0, L)
        if not exists or edge or max(math.comb(L, nd), math.comb(L, other)) <= dense_below:
            out.append(dense_pair(L, nd, step, bonds, p, parts, betas, times))
            continue
        bounds_src = cheb.spectral_bounds(L, nd, bonds, p, seed=seed)
        bounds_dst = bounds_src if step == 0 else cheb.spectral_bounds(L, other, bonds, p, seed=seed)
        logw, C, spent = sampled_pair(L, nd, step, bonds, p, parts, betas, dt, steps, blockref.start_block(math.comb(L, nd), R, seed),
                                      bounds_src, bounds_dst, dtype=dtype, tol=tol)
        out.append((logw, C))
        orders = np.maximum(orders, spent)
    logw = np.stack([q[0] for q in out])
    top = logw.max(axis=0)
    logZ = top + np.log(np.exp(logw - top).sum(axis=0))
    prob = np.exp(logw - logZ)
    return {"logZ": logZ, "C": sum(prob[s][:, None] * out[s][1] for s in range(len(out))), "orders": orders}


def spectrum(times, C, omega, eta):
    """(1 / pi) Re sum_k w_k e^{i omega t_k} C(t_k) e^{-(eta t_k)^2 / 2}, w_k the trapezoid weights, as a direct double loop over
    omega and k in longdouble; C [K + 1] or [B, K + 1]"""
    t = np.asarray(times, dtype=LD)
    C = np.atleast_2d(np.asarray(C))
    re, im = C.real.astype(LD), C.imag.astype(LD)
    w = np.full(t.size, t[1] - t[0], dtype=LD)
    w[0] = w[-1] = (t[1] - t[0]) / LD(2)
    win = w * np.exp(-(LD(eta) * t) ** 2 / LD(2))
    pi = 4 * np.arctan(LD(1))
    out = np.zeros((C.shape[0], len(omega)), dtype=LD)
    for a, om in enumerate(np.asarray(omega, dtype=LD)):
        out[:, a] = ((np.cos(om * t) * re - np.sin(om * t) * im) * win).sum(axis=1) / pi
    return out.astype(np.float64)
