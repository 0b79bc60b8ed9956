"""numpy twin of the Chebyshev propagator and moments on the Hubbard Hamiltonian (docs/design/34-hubbard-chebyshev.md); no GPU, no
torch.  Thin: the recurrences of ``sector_cheb_reference`` and ``sector_moments_reference`` take the mat-vec as an argument and
are bound here to ``hubbard_block_reference.apply_block``.  Every function that runs a recurrence takes a ``dtype``
(``numpy.float64`` or ``numpy.longdouble``).

    coupling_bound(L, bonds, p)                                  B >= ||H||_2 in every sector (hubbard_block_reference)
    chebyshev_apply(L, nup, ndn, bonds, p, X, coeffs, bounds)    sum_m c_m T_m X, (n, R) for one coefficient row, else (A, n, R)
    moments(L, nup, ndn, bonds, p, X, M, bounds, left)           mu [M, R] with the product rule (self) or order by order (left)
    plain_moments(L, nup, ndn, bonds, p, X, M, bounds)           <x| T_m x> order by order
    dense_moments, spectrum_moments, chebyshev_of                those of sector_moments_reference
    sector_moments(L, nup, ndn, bonds, p, M, bounds, R, seed, dense_below)   mu [M] ~ tr T_m of one sector, edge sectors exact
    hubbard_moments(L, bonds, p, M, R, seed, dense_below, sectors, spin_symmetric, bounds)   all sectors on one interval
"""
import math

import numpy as np

import hubbard_block_reference as blockref
import hubbard_reference as ref
import sector_cheb_reference as cheb
import sector_moments_reference as mom

LD = np.longdouble
coupling_bound = blockref.coupling_bound
dense_moments = mom.dense_moments
spectrum_moments = mom.spectrum_moments
chebyshev_of = mom.chebyshev_of


def matvec(L, nup, ndn, bonds, p, dtype=np.float64):
    return lambda x: blockref.apply_block(L, nup, ndn, bonds, p, x, dtype)


def chebyshev_apply(L, nup, ndn, bonds, p, X, coeffs, bounds, dtype=np.float64):
    out = cheb.recurrence(matvec(L, nup, ndn, bonds, p, dtype), X, coeffs, bounds, dtype)
    return out[0] if np.ndim(coeffs) == 1 else out


def moments(L, nup, ndn, bonds, p, X, M, bounds, left=None, dtype=np.float64):
    return mom.recurrence_moments(matvec(L, nup, ndn, bonds, p, dtype), X, M, bounds, left, dtype)


def plain_moments(L, nup, ndn, bonds, p, X, M, bounds, dtype=np.float64):
    return mom.plain_moments(matvec(L, nup, ndn, bonds, p, dtype), X, M, bounds, dtype)


def sector_moments(L, nup, ndn, bonds, p, M, bounds, R=8, seed=0, dense_below=256, dtype=np.float64):
    """mu [M] ~ tr T_m of the sector (nup, ndn): an edge sector from the eigenvalues of ``edge_matrix`` (the one energy when both
    species are frozen), a bulk sector exact from ``eigvalsh`` for n <= dense_below, else (n / R) sum_j mu[:, j] / mu[0, j] over
    the start vectors of ``hubbard_block_reference.start_block``"""
    if nup in (0, L) and ndn in (0, L):
        return spectrum_moments([blockref.edge_matrix(L, bonds, p, nup, ndn == L)[0, 0]], M, bounds)
    if nup in (0, L) or ndn in (0, L):
        count, other = (ndn, nup) if nup in (0, L) else (nup, ndn)
        return spectrum_moments(np.linalg.eigvalsh(blockref.edge_matrix(L, bonds, p, count, other == L)), M, bounds)
    n = math.comb(L, nup) * math.comb(L, ndn)
    if n <= dense_below:
        return spectrum_moments(np.linalg.eigvalsh(ref.dense(L, nup, ndn, bonds, p)), M, bounds)
    mu = moments(L, nup, ndn, bonds, p, blockref.start_block(n, R, seed), M, bounds, dtype=dtype)
    return ((n / R) * (mu / mu[0]).sum(axis=1)).astype(np.float64)


def hubbard_moments(L, bonds, p, M, R=8, seed=0, dense_below=256, sectors=None, spin_symmetric=True, bounds=None, dtype=np.float64):
    """mu [M] of the listed (nup, ndn) sectors (all by default) on one interval, (-B, B) of the coupling bound by default;
    ``spin_symmetric``: the sector (a, b) with a < b takes the moments of (b, a), as hubbard_density_of_states does"""
    if bounds is None:
        B = coupling_bound(L, bonds, p)
        bounds = (-B, B)
    sectors = [(a, b) for a in range(L + 1) for b in range(L + 1)] if sectors is None else sectors
    total, done = np.zeros(M), {}
    for first, second in sectors:
        key = (max(first, second), min(first, second)) if spin_symmetric else (first, second)
        if key not in done:
            done[key] = sector_moments(L, key[0], key[1], bonds, p, M, bounds, R, seed, dense_below, dtype)
        total += done[key]
    return total
