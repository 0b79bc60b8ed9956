"""numpy twin of the Chebyshev moments and of the kernel polynomial method built on them (docs/design/33-chebyshev-moments.md);
no GPU, no torch.  Built on ``sector_cheb_reference`` (coefficients) and ``sector_block_reference`` (the block mat-vec, the start
vectors).  Every function that runs the recurrence takes a ``dtype`` (``numpy.float64`` or ``numpy.longdouble``).

    recurrence_moments(apply, X, M, bounds, left)   mu [M, R]: the tail's operation order, a and b as plain sums, the doubling
    plain_moments(apply, X, M, bounds)              the same moments from M - 1 orders without the product rule
    moments(L, ndown, bonds, p, X, M, bounds, left) on the sector Hamiltonian
    dense_moments(theta, V, X, M, bounds, left)     sum_i <l|v_i><v_i|x> cos(m arccos s_i) from an eigendecomposition
    jackson(M), lorentz(M, lam), density(mu, bounds, E, g), trace(mu, bounds, f), logtrace_exp(mu, bounds, beta)
    spin_moments(L, bonds, p, M, R, seed, dense_below, bounds)   the moments of all magnetisation sectors on one interval
"""
import math

import numpy as np

import sector_block_reference as blockref
import sector_cheb_reference as cheb
import sector_reference as ref

LD = np.longdouble


def _interval(bounds, dtype):
    a, b = float(bounds[0]), float(bounds[1])
    return dtype(0.5 * (a + b)), 0.5 * (b - a)


def recurrence_moments(apply, X, M, bounds, left=None, dtype=np.float64):
    """mu [M, R]: order m forms t = g (H x - centre x) (- old), a = sum l x, b = sum l t (l = x without ``left``), every product
    and difference rounded on its own in ``dtype``; self mode doubles, mu_{2m-2} = 2 a - mu_0 and mu_{2m-1} = 2 b - mu_1, over
    ceil(M / 2) orders; left mode stores mu_m = b over M - 1 orders"""
    centre, h = _interval(bounds, dtype)
    x, old = np.asarray(X, dtype=dtype), None
    l = None if left is None else np.asarray(left, dtype=dtype)
    mu = np.zeros((M, x.shape[1]), dtype=dtype)
    for m in range(1, M if l is not None else (M + 1) // 2 + 1):
        g = dtype((1.0 if m == 1 else 2.0) / h)
        t = g * (apply(x) - centre * x)
        if m > 1:
            t = t - old
        y = x if l is None else l
        a, b = (y * x).sum(axis=0), (y * t).sum(axis=0)
        if m == 1:
            mu[0], mu[1] = a, b
        elif l is not None:
            mu[m] = b
        else:
            if 2 * m - 2 < M:
                mu[2 * m - 2] = dtype(2) * a - mu[0]
            if 2 * m - 1 < M:
                mu[2 * m - 1] = dtype(2) * b - mu[1]
        old, x = x, t
    return mu


def plain_moments(apply, X, M, bounds, dtype=np.float64):
    """mu_m = <x| T_m x> one order at a time: left mode with the block as its own left block"""
    return recurrence_moments(apply, X, M, bounds, left=X, dtype=dtype)


def moments(L, ndown, bonds, p, X, M, bounds, left=None, dtype=np.float64):
    return recurrence_moments(lambda x: blockref.apply_block(L, ndown, bonds, p, x, dtype), X, M, bounds, left, dtype)


def chebyshev_of(s, M):
    """[M, len s]: T_m(s) = cos(m arccos s) for s in [-1, 1]"""
    s = np.asarray(s, dtype=LD)
    assert np.abs(s).max() <= 1
    return np.cos(np.arange(M, dtype=LD)[:, None] * np.arccos(s)[None, :])


def dense_moments(theta, V, X, M, bounds, left=None):
    """mu [M, R] (float64, summed in longdouble) = sum_i <l_j|v_i> <v_i|x_j> T_m(s_i)"""
    centre, h = _interval(bounds, LD)
    s = (np.asarray(theta, dtype=LD) - centre) / LD(h)
    wx = (V.T @ X).astype(LD)
    wl = wx if left is None else (V.T @ left).astype(LD)
    return (chebyshev_of(s, M) @ (wl * wx)).astype(np.float64)


def spectrum_moments(theta, M, bounds):
    """mu [M] = sum_i T_m(s_i): the moments of a trace"""
    centre, h = _interval(bounds, LD)
    return chebyshev_of((np.asarray(theta, dtype=LD) - centre) / LD(h), M).sum(axis=1).astype(np.float64)


def jackson(M):
    pi = 4 * np.arctan(LD(1))
    return np.array([((M - m + 1) * np.cos(pi * m / (M + 1)) + np.sin(pi * m / (M + 1)) / np.tan(pi / (M + 1))) / (M + 1)
                     for m in range(M)], dtype=LD).astype(np.float64)


def lorentz(M, lam=4.0):
    return np.array([np.sinh(LD(lam) * (1 - LD(m) / M)) / np.sinh(LD(lam)) for m in range(M)], dtype=LD).astype(np.float64)


def density(mu, bounds, E, g=None):
    """[g_0 mu_0 + 2 sum_{m >= 1} g_m mu_m T_m(s)] / (pi h sqrt(1 - s^2)) strictly inside the bounds, 0 outside"""
    mu = np.asarray(mu, dtype=np.float64)
    M = len(mu)
    c = mu * (np.ones(M) if g is None else np.asarray(g))
    c[1:] *= 2.0
    centre, h = _interval(bounds, np.float64)
    s = (np.asarray(E, dtype=np.float64) - centre) / h
    out = np.zeros(s.shape)
    inside = np.abs(s) < 1
    out[inside] = (c @ np.cos(np.arange(M)[:, None] * np.arccos(s[inside])[None, :])) / (math.pi * h * np.sqrt(1 - s[inside] ** 2))
    return out


def trace(mu, bounds, f):
    """sum_m c_m mu_m, c the coefficients of f(centre + h s) with c_0 halved"""
    centre, h = _interval(bounds, LD)
    return float(np.dot(cheb.coefficients(lambda s: f(centre + LD(h) * s), len(mu)), np.asarray(mu, dtype=np.float64)))


def logtrace_exp(mu, bounds, beta):
    _, h = _interval(bounds, LD)
    return math.log(float(np.dot(cheb.coefficients(cheb.exp_function(beta * h), len(mu)), np.asarray(mu, dtype=np.float64)))) \
        - beta * float(bounds[0])


def sector_moments(L, ndown, bonds, p, M, bounds, R=8, seed=0, dense_below=256, dtype=np.float64):
    """mu [M] ~ tr T_m of one sector: exact from ``eigvalsh`` for n <= dense_below, else (n / R) sum_j mu[:, j] / mu[0, j] over
    the start vectors of ``sector_block_reference.start_block``"""
    n = math.comb(L, ndown)
    if n <= dense_below:
        return spectrum_moments(np.linalg.eigvalsh(ref.dense(L, ndown, bonds, p)), M, bounds)
    mu = moments(L, ndown, bonds, p, blockref.start_block(n, R, seed), M, bounds, dtype=dtype)
    return ((n / R) * (mu / mu[0]).sum(axis=1)).astype(np.float64)


def spin_moments(L, bonds, p, M, R=8, seed=0, dense_below=256, bounds=None, dtype=np.float64):
    """mu [M] of all magnetisation sectors on one interval, (-B, B) of the coupling bound by default"""
    if bounds is None:
        B = blockref.coupling_bound(L, bonds, p)
        bounds = (-B, B)
    total = np.zeros(M)
    for ndown in range(L + 1):
        if ndown in (0, L):
            total += spectrum_moments([blockref.edge_energy(L, bonds, p, ndown)], M, bounds)
        else:
            total += sector_moments(L, ndown, bonds, p, M, bounds, R, seed, dense_below, dtype)
    return total
