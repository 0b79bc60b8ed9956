"""Finite temperature by the finite-temperature Lanczos method (docs/design/27-finite-temperature.md for spins,
docs/design/28-hubbard-finite-temperature.md for the Hubbard model).

    tr f(H) in a sector of dimension n  ~=  (n / R) sum_r <r| f(H) |r>     over R random unit vectors r

and every <r| f(H) |r> is the Gauss quadrature sum_j S_{0j}^2 f(theta_j) of the k x k Lanczos matrix T = S diag(theta) S^T of r:
a ``SpectralMeasure``.  The runs keep NO basis and do not re-orthogonalise (the quadrature does not need it): all R vectors go
through the three-term recurrence at once as one [n, R] block, on the block mat-vec of ``SpinSectorOperator`` or of
``HubbardOperator``; the k x k eigenproblems are solved on the host.

    block_lanczos_coefficients(op, Phi, k)  norm2, alphas, betas and steps of the R columns of Phi, basis-free
    block_lanczos_measures(op, Phi, k)      their measures
    sector_trace_measure(op, R, k, seed)    a measure with sum_j w_j f(theta_j) ~= tr f(H_sector); exact for small sectors
    ThermalEnsemble(entries)                ln Z, E, C, S and chi of a list of (measure, m) over a tensor of inverse temperatures
    spin_thermodynamics(L, bonds, couplings, ...)   the ensemble over all magnetisation sectors of a bond-list XXZ model
    sector_density_of_states(op, M, bounds, ...)    the Chebyshev moments of tr T_m(H_sector): a ``chebyshev.ChebyshevMeasure``
    spin_density_of_states(L, bonds, couplings, M)  those of all sectors on one interval (docs/design/33-chebyshev-moments.md)
    GrandCanonicalEnsemble(entries)         ln Xi, <H>, <N>, kappa, chi_s, C and S of a list of (measure, nup, ndn) over (beta, mu)
    hubbard_thermodynamics(L, bonds, couplings, ...)   that ensemble over all (nup, ndn) sectors of a Hubbard model
    hubbard_density_of_states(L, bonds, couplings, M)  the Chebyshev moments of tr T_m over all (nup, ndn) sectors on one interval
                                                       (docs/design/34-hubbard-chebyshev.md)
    thermal_correlations(L, bonds, couplings, betas, ...)   <X_i X_j + Y_i Y_j>, <Z_i Z_j>, <Z_i>, E and ln Z at T > 0 from thermal
                                                       pure quantum states e^{-beta H / 2} |r> (docs/design/31-chebyshev-propagator.md)
    thermal_dynamics(L, bonds, couplings, weights, channel, betas, dt, steps, ...)   C(t) = <A^T(t) A> at T > 0 for A = sum_i c_i Z_i,
                                                       sigma^-_i or sigma^+_i, and its spectrum S(q, omega; T): those states stepped
                                                       in real time, the block ladder map in between
                                                       (docs/design/35-finite-temperature-dynamics.md)
    hubbard_thermal_dynamics(L, bonds, couplings, weights, channel, betas, mus, dt, steps, ...)   the same for the Hubbard model
                                                       and A = sum_i w_i c_{i s}, c+_{i s}, n_i or 2 S^z_i at every (beta, mu): the
                                                       one-particle A(k, omega; T) (docs/design/37-hubbard-finite-temperature-dynamics.md)
    hubbard_thermal_conductivity(L, bonds, couplings, displacements, betas, mus, dt, steps, ...)   <J(t) J> and the diamagnetic
                                                       term K_d of the Hubbard model at every (beta, mu): sigma_reg(omega; T), its
                                                       weight and the thermodynamic stiffness, the block current map and its
                                                       column dots in between (docs/design/40-finite-temperature-conductivity.md)

Plain host float64 numbers: nothing here is differentiable.
"""
from __future__ import annotations

import math
from ctypes import byref, c_int64, c_void_p

import torch

from . import _lib, engine
from ._lib import check
from .spectral import SpectralMeasure

F64 = torch.float64
BLOCK_WIDTHS = (8, 4, 2, 1)


def block_pieces(R):
    """[(first column, width)] of the split of R >= 1 columns into blocks the kernels take: widths 8, 4, 2 and 1, widest first"""
    R = int(R)
    if R < 1:
        raise ValueError("a block needs at least one column, got %d" % R)
    out, first = [], 0
    for w in BLOCK_WIDTHS:
        while R - first >= w:
            out.append((first, w))
            first += w
    return out


def _sector_operator(op, what):
    from .operators import HubbardOperator, SpinSectorOperator
    if not isinstance(op, (SpinSectorOperator, HubbardOperator)):
        raise ValueError("%s works on the bond-list SpinSectorOperator and on the HubbardOperator only, got %s"
                         % (what, type(op).__name__))
    return op


def _block_lanczos_entries(op, lib):
    """(scratch query with the sector's sizes bound, run, the run's name) of the operator's kind: the pair of ABI entries"""
    from .operators import HubbardOperator
    if isinstance(op, HubbardOperator):
        return (lambda w, out: lib.dsea_op_hubbard_block_lanczos_scratch_doubles(op.N, op.nup, op.ndn, w, out),
                lib.dsea_op_hubbard_block_lanczos, "dsea_op_hubbard_block_lanczos")
    return (lambda w, out: lib.dsea_op_sector_block_lanczos_scratch_doubles(op.N, op.ndown, w, out),
            lib.dsea_op_sector_block_lanczos, "dsea_op_sector_block_lanczos")


def _as_block(op, X, what):
    if not torch.is_tensor(X) or X.dim() != 2 or X.shape[0] != op.n or X.shape[1] < 1:
        raise ValueError("%s expects a tensor of shape (%d, R) with R >= 1, got %r"
                         % (what, op.n, tuple(X.shape) if torch.is_tensor(X) else type(X).__name__))
    if not X.is_cuda:
        raise ValueError("%s expects a block on %s, got a %s tensor" % (what, op.device, X.device))
    return X.detach()


def _empty_measure(norm2=0.0):
    return SpectralMeasure(torch.empty(0, dtype=F64), torch.empty(0, dtype=F64), norm2, 0)


def _tridiagonal_measure(alphas, betas, norm2):
    """the measure norm2 sum_j S_{0j}^2 delta(E - theta_j) of the tridiagonal matrix with diagonal alphas (s) and off-diagonal
    betas (s - 1), host tensors"""
    s = alphas.numel()
    T = torch.diag(alphas)
    if s > 1:
        T = T + torch.diag(betas, 1) + torch.diag(betas, -1)
    theta, S = torch.linalg.eigh(T)
    return SpectralMeasure(theta, norm2 * S[0] ** 2, norm2, s)


def block_lanczos_coefficients(op, Phi, k):
    """(norm2 [R], alphas [k, R], betas [k, R], steps [R]) of the basis-free recurrence for the R columns of ``Phi`` as host
    tensors, k cut to n: norm2[j] = |Phi[:, j]|^2, alphas[i, j] = alpha_i and betas[i, j] = beta_{i+1} of column j, steps[j] = k or
    the step at which column j broke (dsea_op_sector_block_lanczos, or dsea_op_hubbard_block_lanczos for a ``HubbardOperator``, in
    blocks of 8, 4, 2 and 1 columns)."""
    op = _sector_operator(op, "block_lanczos_coefficients")
    k = min(int(k), int(op.n))
    if k < 1:
        raise ValueError("the block Lanczos run needs k >= 1")
    Phi = _as_block(op, Phi, "block_lanczos_coefficients")
    lib = _lib.load()
    scratch_doubles, run, name = _block_lanczos_entries(op, lib)
    dev = Phi.device
    out = []
    for first, w in block_pieces(Phi.shape[1]):
        Q = Phi[:, first:first + w].to(F64).clone(memory_format=torch.contiguous_format)   # (overwritten by the run)
        W = torch.empty_like(Q)
        need = c_int64()
        check(scratch_doubles(w, byref(need)), name + "_scratch_doubles")
        scratch = torch.empty(need.value, dtype=F64, device=dev)
        norm2 = torch.empty(w, dtype=F64, device=dev)
        alphas = torch.empty((k, w), dtype=F64, device=dev)
        betas = torch.empty((k, w), dtype=F64, device=dev)
        steps = torch.empty(w, dtype=torch.int32, device=dev)
        check(run(op.handle, w, k, c_void_p(Q.data_ptr()), c_void_p(W.data_ptr()), c_void_p(norm2.data_ptr()),
                  c_void_p(alphas.data_ptr()), c_void_p(betas.data_ptr()), c_void_p(steps.data_ptr()),
                  c_void_p(scratch.data_ptr()), engine._stream(dev)), name)
        out.append((norm2.cpu(), alphas.cpu(), betas.cpu(), steps.cpu()))
    return tuple(torch.cat([piece[i] for piece in out], dim=-1) for i in range(4))


def block_lanczos_measures(op, Phi, k):
    """The spectral measures of the R columns of ``Phi`` (a device tensor (n, R), any R >= 1, any norms) under the
    ``SpinSectorOperator`` or ``HubbardOperator`` ``op``, from min(k, n) steps of the three-term recurrence WITHOUT a stored
    basis and without re-orthogonalisation: memory is two blocks plus scratch whatever k is.  Columns go through the kernels in blocks of 8, 4, 2
    and 1.  A column whose Krylov space is exhausted at step s reports ``steps = s`` (its poles are then exact eigenvalues)
    while the other columns go on; a zero column gives the empty measure.  Returns a list of R ``SpectralMeasure``.  Not
    differentiable: Phi is detached."""
    norm2, alphas, betas, steps = block_lanczos_coefficients(_sector_operator(op, "block_lanczos_measures"), Phi, k)
    out = []
    for j in range(steps.numel()):
        s = int(steps[j])
        if s == 0:
            out.append(_empty_measure(float(norm2[j])))
        else:
            out.append(_tridiagonal_measure(alphas[:s, j].contiguous(), betas[:s - 1, j].contiguous(), float(norm2[j])))
    return out


def _dense_sector_matrix(op):
    """H of the sector as a host matrix: ``op.apply_block`` on the identity columns, eight at a time"""
    n = int(op.n)
    H = torch.empty((n, n), dtype=F64, device=op.device)
    for first in range(0, n, 8):
        w = min(8, n - first)
        X = torch.zeros((n, w), dtype=F64, device=op.device)
        X[first:first + w] = torch.eye(w, dtype=F64, device=op.device)
        H[:, first:first + w] = op.apply_block(X)
    return H.cpu()


def sector_trace_measure(op, R=8, k=100, seed=0, dense_below=256):
    """A ``SpectralMeasure`` with sum_j w_j f(theta_j) ~= tr f(H) over the sector of ``op``, a ``SpinSectorOperator`` or a
    ``HubbardOperator``.

    n <= ``dense_below``: EXACT -- H is formed by ``op.apply_block`` on the identity columns, eight at a time, its eigenvalues
    (``torch.linalg.eigvalsh`` on the host) are the poles and the weights are 1.  Otherwise the R start vectors are
    ``synthetic.normal_vector(n, seed + j)`` (deterministic; the torch generators are not touched), each runs min(k, n)
    basis-free Lanczos steps in one block, and the weights are (n / R) S_{0j}^2: a stochastic estimate whose error is the
    sampling error of R vectors."""
    op = _sector_operator(op, "sector_trace_measure")
    n = int(op.n)
    R, k = int(R), int(k)
    if R < 1 or k < 1:
        raise ValueError("sector_trace_measure needs R >= 1 and k >= 1")
    if n <= int(dense_below):
        poles = torch.linalg.eigvalsh(_dense_sector_matrix(op))
        return SpectralMeasure(poles, torch.ones(n, dtype=F64), float(n), n)
    from .synthetic import normal_vector
    Phi = torch.stack([torch.from_numpy(normal_vector(n, int(seed) + j)) for j in range(R)], dim=1).to(op.device)
    parts = block_lanczos_measures(op, Phi, k)
    poles = torch.cat([m.poles for m in parts])
    weights = torch.cat([m.weights * (n / (R * m.norm2)) for m in parts if len(m)] or [torch.empty(0, dtype=F64)])
    return SpectralMeasure(poles, weights, float(n), sum(m.steps for m in parts))


class ThermalEnsemble:
    """Canonical averages over a list of ``(measure, m)``: ``measure`` a ``SpectralMeasure`` with sum_j w_j f(theta_j) = tr f(H)
    of one sector (``sector_trace_measure``) and ``m`` the magnetisation S^z_total = L / 2 - ndown of that sector.  With
    p_j = w_j exp(-beta theta_j) / Z over all poles of all entries:

        logZ(beta)            ln sum_j w_j exp(-beta theta_j)     (log-sum-exp shifted by the lowest pole)
        energy(beta)          E = sum_j p_j theta_j
        specific_heat(beta)   C = beta^2 sum_j p_j (theta_j - E)^2
        entropy(beta)         S = ln Z + beta E
        susceptibility(beta)  chi = beta sum_j p_j (m_j - <m>)^2
        moment(p)             sum_j w_j theta_j^p = tr H^p

    ``beta`` >= 0 is a number or a tensor; the results are host float64 tensors of its shape.  The variances are sums of squared
    deviations, not differences of two means.  Plain numbers: not differentiable."""

    def __init__(self, entries):
        entries = list(entries)
        if not entries:
            raise ValueError("ThermalEnsemble needs at least one (measure, m) entry")
        poles, weights, ms = [], [], []
        for entry in entries:
            if not (isinstance(entry, (tuple, list)) and len(entry) == 2 and isinstance(entry[0], SpectralMeasure)):
                raise ValueError("every entry must be a (SpectralMeasure, m) pair, got %r" % (entry,))
            measure, m = entry
            poles.append(measure.poles)
            weights.append(measure.weights)
            ms.append(torch.full((len(measure),), float(m), dtype=F64))
        self.entries = [(e[0], float(e[1])) for e in entries]
        self.poles, self.weights, self.m = torch.cat(poles), torch.cat(weights), torch.cat(ms)
        if self.poles.numel() == 0:
            raise ValueError("ThermalEnsemble needs at least one pole")
        if bool((self.weights < 0).any()):
            raise ValueError("the weights of a trace measure must not be negative")
        self.lowest = float(self.poles.min())

    def _boltzmann(self, beta):
        """(beta as a host fp64 tensor, sum_j w_j exp(-beta (theta_j - lowest)) [...], the probabilities p [..., poles])"""
        beta = torch.as_tensor(beta, dtype=F64).detach().cpu()
        if bool((beta < 0).any()):
            raise ValueError("ThermalEnsemble works at inverse temperatures beta >= 0")
        terms = self.weights * torch.exp(-beta.unsqueeze(-1) * (self.poles - self.lowest))
        total = terms.sum(dim=-1)
        return beta, total, terms / total.unsqueeze(-1)

    def logZ(self, beta):
        beta, total, _ = self._boltzmann(beta)
        return torch.log(total) - beta * self.lowest

    def energy(self, beta):
        _, _, p = self._boltzmann(beta)
        return (p * self.poles).sum(dim=-1)

    def specific_heat(self, beta):
        beta, _, p = self._boltzmann(beta)
        E = (p * self.poles).sum(dim=-1)
        return beta ** 2 * (p * (self.poles - E.unsqueeze(-1)) ** 2).sum(dim=-1)

    def entropy(self, beta):
        beta, total, p = self._boltzmann(beta)
        return torch.log(total) - beta * self.lowest + beta * (p * self.poles).sum(dim=-1)

    def susceptibility(self, beta):
        beta, _, p = self._boltzmann(beta)
        mean = (p * self.m).sum(dim=-1)
        return beta * (p * (self.m - mean.unsqueeze(-1)) ** 2).sum(dim=-1)

    def moment(self, p):
        return float((self.weights * self.poles ** int(p)).sum())


def _spin_model(L, bonds, couplings, sectors, device):
    """(L, bonds, couplings, sectors, sum Jz, sum hz, device) of a bond-list XXZ model, checked: the parameter order is
    [Jxy(nb), Jz(nb), hz(L)], ``sectors`` None means ndown = 0 .. L"""
    from .operators import _check_bonds
    L = int(L)
    bonds = _check_bonds(L, bonds)
    nb = len(bonds)
    c = torch.as_tensor(couplings, dtype=F64).detach()
    if tuple(c.shape) != (2 * nb + L,):
        raise ValueError("couplings must have shape (%d,): Jxy(nb), Jz(nb), hz(L)" % (2 * nb + L))
    sectors = list(range(L + 1)) if sectors is None else [int(s) for s in sectors]
    if not sectors or any(not 0 <= s <= L for s in sectors) or len(set(sectors)) != len(sectors):
        raise ValueError("sectors must be distinct values of ndown in 0 .. %d" % L)
    host = c.cpu()
    jz_sum, hz_sum = float(host[nb:2 * nb].sum()), float(host[2 * nb:].sum())
    if device is None:
        device = c.device if c.is_cuda else "cuda"
    return L, bonds, c, sectors, jz_sum, hz_sum, device


def spin_thermodynamics(L, bonds, couplings, R=8, k=100, seed=0, dense_below=256, sectors=None, device=None):
    """The ``ThermalEnsemble`` of H = sum_t [Jxy_t (X_a X_b + Y_a Y_b) + Jz_t Z_a Z_b] + sum_i hz_i Z_i (the Hamiltonian and the
    parameter order [Jxy(nb), Jz(nb), hz(L)] of ``SpinSectorOperator``) over the sectors ndown = 0 .. L, or over the list
    ``sectors``.  Every sector contributes ``sector_trace_measure(op, R, k, seed, dense_below)`` at m = L / 2 - ndown; the two
    one-state sectors ndown = 0 and ndown = L, which the operator refuses, contribute their energy sum_t Jz_t +- sum_i hz_i from
    host arithmetic.  One sector's tables are released before the next sector is built."""
    from .operators import SpinSectorOperator
    L, bonds, c, sectors, jz_sum, hz_sum, device = _spin_model(L, bonds, couplings, sectors, device)
    entries = []
    for ndown in sectors:
        m = 0.5 * L - ndown
        if ndown in (0, L):
            energy = jz_sum + (hz_sum if ndown == 0 else -hz_sum)
            entries.append((SpectralMeasure(torch.tensor([energy], dtype=F64), torch.ones(1, dtype=F64), 1.0, 1), m))
            continue
        op = SpinSectorOperator(L, bonds, c.to(device), ndown, device)
        entries.append((sector_trace_measure(op, R=R, k=k, seed=seed, dense_below=dense_below), m))
        del op
    return ThermalEnsemble(entries)


def _trace_moments(poles, M, centre, h):
    """mu [M] = sum_i T_m((theta_i - centre) / h) = sum_i cos(m arccos s_i) of a host tensor of eigenvalues inside the bounds"""
    s = (poles.to(F64) - centre) / h
    if bool((s.abs() > 1.0).any()):
        raise ValueError("the bounds (%r, %r) do not hold the spectrum [%r, %r]"
                         % (centre - h, centre + h, float(poles.min()), float(poles.max())))
    return torch.cos(torch.arange(M, dtype=F64)[:, None] * torch.acos(s)[None, :]).sum(dim=1)


def sector_density_of_states(op, M, bounds, R=8, seed=0, dense_below=256):
    """A ``chebyshev.ChebyshevMeasure`` with the moments mu_m ~= tr T_m((H - centre) / h) over the sector of ``op``: its density
    is the density of states of the sector, its ``trace(f)`` is tr f(H) (docs/design/33-chebyshev-moments.md).  ``bounds`` must
    hold the spectrum.

    n <= ``dense_below``: EXACT -- mu_m = sum_i T_m(s_i) over the eigenvalues (host ``eigvalsh``) of the matrix formed by
    ``op.apply_block`` on the identity columns.  Otherwise the start vectors and the weight n / R of ``sector_trace_measure``:
    mu_m = (n / R) sum_j <r_j| T_m |r_j> / <r_j|r_j> over r_j = ``synthetic.normal_vector(n, seed + j)``, all R columns in the
    runs of ``chebyshev.chebyshev_moments`` (ceil(M / 2) mat-vecs) -- a stochastic estimate whose error is the sampling error of
    R vectors."""
    from .chebyshev import ChebyshevMeasure, _check_bounds, chebyshev_moments
    op = _sector_operator(op, "sector_density_of_states")
    n, M, R = int(op.n), int(M), int(R)
    if R < 1 or M < 2:
        raise ValueError("sector_density_of_states needs R >= 1 and M >= 2")
    centre, h = _check_bounds(bounds)
    if n <= int(dense_below):
        return ChebyshevMeasure(_trace_moments(torch.linalg.eigvalsh(_dense_sector_matrix(op)), M, centre, h), bounds)
    from .synthetic import normal_vector
    Phi = torch.stack([torch.from_numpy(normal_vector(n, int(seed) + j)) for j in range(R)], dim=1).to(op.device)
    mu = chebyshev_moments(op, Phi, M, bounds)
    return ChebyshevMeasure((n / R) * (mu / mu[0]).sum(dim=1), bounds)


def spin_density_of_states(L, bonds, couplings, M, R=8, seed=0, dense_below=256, sectors=None, bounds=None, device=None):
    """The ``chebyshev.ChebyshevMeasure`` of the whole spectrum of the model of ``spin_thermodynamics`` (all magnetisation
    sectors, or the list ``sectors``): mu_m ~= tr T_m over the 2^L states, so that mu_0 = 2^L, ``density(E) / 2^L`` is the
    normalised density of states and ``logtrace_exp(beta)`` is ln Z.  All sectors are expanded on ONE interval, so their moments
    add: ``bounds``, or by default the rigorous (-B, B) with B = sum_t (2 |Jxy_t| + |Jz_t|) + sum_i |hz_i| >= ||H||.  Every sector
    contributes ``sector_density_of_states(op, M, bounds, R, seed, dense_below)``; ndown = 0 and ndown = L are one state each,
    T_m of their energy sum_t Jz_t +- sum_i hz_i from host arithmetic."""
    from .chebyshev import ChebyshevMeasure, _check_bounds
    from .operators import SpinSectorOperator
    L, bonds, c, sectors, jz_sum, hz_sum, device = _spin_model(L, bonds, couplings, sectors, device)
    M = int(M)
    if M < 2:
        raise ValueError("spin_density_of_states needs M >= 2, got %d" % M)
    if bounds is None:
        nb = len(bonds)
        host = c.cpu().abs()
        B = float(2.0 * host[:nb].sum() + host[nb:].sum())
        bounds = (-B, B)
    centre, h = _check_bounds(bounds)
    total = None
    for ndown in sectors:
        if ndown in (0, L):
            energy = jz_sum + (hz_sum if ndown == 0 else -hz_sum)
            part = ChebyshevMeasure(_trace_moments(torch.tensor([energy], dtype=F64), M, centre, h), bounds)
        else:
            op = SpinSectorOperator(L, bonds, c.to(device), ndown, device)
            part = sector_density_of_states(op, M, bounds, R=R, seed=seed, dense_below=dense_below)
            del op
        total = part if total is None else total + part
    return total


class ThermalCorrelations:
    """What ``thermal_correlations`` returns, host float64 tensors over the B inverse temperatures ``betas``: ``logZ`` [B],
    ``energy`` [B], ``xy`` [B, L, L] = <X_i X_j + Y_i Y_j>, ``zz`` [B, L, L] = <Z_i Z_j> (diagonals 2 and 1) and ``z`` [B, L] =
    <Z_i>."""

    def __init__(self, betas, logZ, energy, xy, zz, z):
        self.betas, self.logZ, self.energy, self.xy, self.zz, self.z = betas, logZ, energy, xy, zz, z


def _dense_sector_correlations(op, betas):
    """(log weight [B], E [B], xy, zz, z) of a sector from its full spectrum: H from ``apply_block`` on identity columns, host
    ``eigh``, and ``correlations(v, v)`` of every eigenvector"""
    n = int(op.n)
    theta, V = torch.linalg.eigh(_dense_sector_matrix(op))
    pair = op.pair_operator()
    Vd = V.to(op.device)
    parts = [pair.correlations(Vd[:, j].contiguous()) for j in range(n)]
    xy, zz, z = (torch.stack([q[i] for q in parts]).cpu() for i in range(3))
    logw = -betas[:, None] * theta[None, :]
    logsum = torch.logsumexp(logw, dim=1)
    prob = torch.exp(logw - logsum[:, None])
    return logsum, prob @ theta, torch.einsum("bj,jkl->bkl", prob, xy), torch.einsum("bj,jkl->bkl", prob, zz), prob @ z


def _tpq_states(op, betas, R, seed, tol, bounds=None):
    """The R canonical thermal pure quantum states of the sector of ``op`` at every beta in turn, as a generator of
    (Phi [n, R] normalised columns on the device, log norms [R] on the host, top, w [R], log weight of the sector): the columns
    r_j = normal_vector(n, seed + j), normalised, are stepped from one beta to the next by ``expm_block`` over half the difference
    and renormalised, the logarithms of their norms kept on the host; column j weighs w_j = exp(2 log norm_j - top) with
    top = 2 max_j log norm_j, and the sector weighs (n / R) e^top sum_j w_j.  ``bounds`` None: ``spectral_bounds(op, seed=seed)``."""
    from .chebyshev import expm_block, spectral_bounds
    from .synthetic import normal_vector
    n = int(op.n)
    Phi = torch.stack([torch.from_numpy(normal_vector(n, int(seed) + j)) for j in range(R)], dim=1).to(op.device)
    Phi = Phi / torch.linalg.vector_norm(Phi, dim=0)
    if bounds is None:
        bounds = spectral_bounds(op, seed=seed)
    lognorm = torch.zeros(R, dtype=F64)
    before = 0.0
    for beta in betas.tolist():
        tau = 0.5 * (beta - before)
        before = beta
        Y, shift = expm_block(op, Phi, tau, bounds, tol)
        norms = torch.linalg.vector_norm(Y, dim=0)
        Phi = Y / norms
        lognorm = lognorm + torch.log(norms.cpu()) - tau * shift
        top = 2.0 * lognorm.max()
        w = torch.exp(2.0 * lognorm - top)
        yield Phi, lognorm, top, w, math.log(n / R) + top + torch.log(w.sum())


def _tpq_sector_correlations(op, betas, R, seed, tol):
    """the same five from the R thermal pure quantum states of ``_tpq_states``: at every beta column j weighs exp(2 log norm_j)
    and the sector weighs (n / R) times their sum"""
    pair = op.pair_operator()
    out = [[] for _ in range(5)]
    for Phi, _, _, w, logweight in _tpq_states(op, betas, R, seed, tol):
        energy = (Phi * op.apply_block(Phi)).sum(dim=0).cpu()
        parts = [pair.correlations(Phi[:, j].contiguous()) for j in range(R)]
        total = w.sum()
        out[0].append(logweight)
        out[1].append((w * energy).sum() / total)
        for i in range(3):
            q = torch.stack([part[i] for part in parts]).cpu()
            out[2 + i].append((w.reshape((R,) + (1,) * (q.dim() - 1)) * q).sum(dim=0) / total)
    return tuple(torch.stack(o) for o in out)


def thermal_correlations(L, bonds, couplings, betas, R=8, seed=0, dense_below=256, sectors=None, tol=1e-15, device=None):
    """Thermal averages that do not commute with H, for the model and the parameter order of ``spin_thermodynamics``, at the
    ascending inverse temperatures ``betas`` >= 0: a ``ThermalCorrelations`` with ``logZ``, ``energy``, ``xy``, ``zz`` and ``z``.

    A sector with n > ``dense_below`` rows is sampled by R canonical thermal pure quantum states |beta, r> = e^{-beta H / 2} |r>
    on the start vectors and with the sector weight n / R of ``sector_trace_measure``: |e^{-beta H / 2} r|^2 estimates what its
    <r| e^{-beta H} |r> estimates.  Each state is stepped from the previous beta by ``chebyshev.expm_block`` (order chosen by
    ``tol``) and renormalised; at every beta it costs one ``apply_block`` for <H> and one ``correlations`` per column.  A
    smaller sector is exact: its full spectrum, and ``correlations(v, v)`` of every eigenvector (at most ``dense_below`` forms
    calls per sector, made once for all betas).  ndown = 0 and ndown = L are one state each: xy = 0 off the diagonal, zz = 1,
    z = +1 or -1, the energy from host arithmetic.  The sectors are combined by a log-sum-exp of their log weights; one
    sector's tables are released before the next is built.  The error of a sampled sector is the sampling error of R
    vectors; it is not estimated."""
    from .operators import SpinSectorOperator, _check_bonds
    L = int(L)
    bonds = _check_bonds(L, bonds)
    nb = len(bonds)
    c = torch.as_tensor(couplings, dtype=F64).detach()
    if tuple(c.shape) != (2 * nb + L,):
        raise ValueError("couplings must have shape (%d,): Jxy(nb), Jz(nb), hz(L)" % (2 * nb + L))
    betas = torch.as_tensor(betas, dtype=F64).detach().cpu().reshape(-1)
    if betas.numel() < 1 or not bool(torch.isfinite(betas).all()) or bool((betas < 0).any()) or bool((betas[1:] < betas[:-1]).any()):
        raise ValueError("betas must be finite, >= 0 and ascending")
    R = int(R)
    if R < 1:
        raise ValueError("thermal_correlations needs R >= 1")
    sectors = list(range(L + 1)) if sectors is None else [int(s) for s in sectors]
    if not sectors or any(not 0 <= s <= L for s in sectors) or len(set(sectors)) != len(sectors):
        raise ValueError("sectors must be distinct values of ndown in 0 .. %d" % L)
    host = c.cpu()
    jz_sum, hz_sum = float(host[nb:2 * nb].sum()), float(host[2 * nb:].sum())
    if device is None:
        device = c.device if c.is_cuda else "cuda"
    B = betas.numel()
    parts = []
    for ndown in sectors:
        if ndown in (0, L):
            sign = 1.0 if ndown == 0 else -1.0
            one = torch.ones((B, L, L), dtype=F64)
            parts.append((-betas * (jz_sum + sign * hz_sum), torch.full((B,), jz_sum + sign * hz_sum, dtype=F64),
                          2.0 * torch.eye(L, dtype=F64).expand(B, L, L), one, sign * torch.ones((B, L), dtype=F64)))
            continue
        op = SpinSectorOperator(L, bonds, c.to(device), ndown, device)
        if op.n <= int(dense_below):
            parts.append(_dense_sector_correlations(op, betas))
        else:
            parts.append(_tpq_sector_correlations(op, betas, R, seed, tol))
        del op
    logw = torch.stack([p[0] for p in parts])                              # [sectors, B]
    logZ = torch.logsumexp(logw, dim=0)
    prob = torch.exp(logw - logZ)
    mix = lambda i: sum(prob[s].reshape((B,) + (1,) * (parts[s][i].dim() - 1)) * parts[s][i] for s in range(len(parts)))  # noqa: E731
    return ThermalCorrelations(betas, logZ, mix(1), mix(2), mix(3), mix(4))


class ThermalDynamics:
    """What ``thermal_dynamics`` returns, host tensors: ``betas`` [B], ``times`` [K + 1] with t_k = k dt, ``logZ`` [B] and
    ``correlation`` [B, K + 1] (complex128), C(t_k) = tr[e^{-beta H} A^T(t_k) A] / Z at every beta."""

    def __init__(self, betas, times, logZ, correlation):
        self.betas, self.times, self.logZ, self.correlation = betas, times, logZ, correlation

    def static(self):
        """C(0).real [B]: the equal-time correlation <A^T A>"""
        return self.correlation[:, 0].real.clone()

    def spectrum(self, omega, eta):
        """S(omega) [B, len omega] = (1 / pi) Re sum_k w_k e^{i omega t_k} C(t_k) e^{-(eta t_k)^2 / 2} with the trapezoid weights
        w_k = dt (dt / 2 at both ends): (1 / 2 pi) int dt e^{i omega t} C(t) e^{-(eta t)^2 / 2} over all times, folded onto t >= 0
        with C(-t) = C(t)^* (which holds in the exact trace), so that a pole of C at the excitation energy eps becomes a
        Gaussian of width ``eta`` at omega = eps.  THE CALLER picks dt and K: eta t_K >= 8, so that the window has decayed where
        the record ends, and pi / dt well above the band width, so that the trapezoid sum does not alias."""
        return _windowed_spectrum(self.times, self.correlation, omega, eta)


def _windowed_spectrum(times, correlation, omega, eta):
    """the Gaussian-windowed transform of ``ThermalDynamics.spectrum`` for a record ``correlation`` [rows, K + 1] at ``times``:
    [rows, len omega]"""
    eta = float(eta)
    if not (eta > 0 and math.isfinite(eta)):
        raise ValueError("spectrum needs a finite eta > 0, got %r" % (eta,))
    K = times.numel() - 1
    if K < 1:
        raise ValueError("spectrum needs at least one time step")
    omega = torch.as_tensor(omega, dtype=F64).detach().cpu().reshape(-1)
    t = times
    w = torch.full((K + 1,), float(t[1] - t[0]), dtype=F64)
    w[0] = w[-1] = 0.5 * float(t[1] - t[0])
    window = w * torch.exp(-0.5 * (eta * t) ** 2)
    phase = torch.exp(torch.complex(torch.zeros(omega.numel(), K + 1, dtype=F64), omega[:, None] * t[None, :]))
    return (torch.einsum("wk,bk->bw", phase * window, correlation).real / math.pi).contiguous()


def _dense_ladder_matrix(L, ndown_src, step, c):
    """the n_dst x n_src host matrix of sum_i c_i O_i from the sector (L, ndown_src) to (L, ndown_src + step), from
    ``sector_states`` (edge sectors included): sigma^- arrives at a set bit, sigma^+ at a clear one, Z is diagonal"""
    from .operators import sector_states
    src, dst = sector_states(L, ndown_src), sector_states(L, ndown_src + step)
    A = torch.zeros((len(dst), len(src)), dtype=F64)
    c = c.tolist()
    if step == 0:
        for r, s in enumerate(dst):
            A[r, r] = sum(c[i] * (1 - 2 * ((s >> i) & 1)) for i in range(L))
        return A
    rank = {s: r for r, s in enumerate(src)}
    want = 1 if step > 0 else 0
    for r, s in enumerate(dst):
        for i in range(L):
            if (s >> i) & 1 == want:
                A[r, rank[s ^ (1 << i)]] = c[i]
    return A


def _dense_pair_dynamics(spec_src, spec_dst, maps, betas, times):
    """(log weight [B], C [B, K + 1]) of a sector pair from the full spectra (theta, V) of its two sides and the host matrices
    ``maps`` of the real parts of A: C(t) = sum_{n, m} p_n sum_parts |<m|A|n>|^2 e^{-i (E_m - E_n) t}, p_n = e^{-beta E_n} / Z_src.
    ``spec_dst`` None: the destination does not exist, C = 0."""
    theta, V = spec_src
    logw = -betas[:, None] * theta[None, :]
    logsum = torch.logsumexp(logw, dim=1)
    if spec_dst is None:
        return logsum, torch.zeros((betas.numel(), times.numel()), dtype=torch.complex128)
    prob = torch.exp(logw - logsum[:, None])
    theta2, V2 = spec_dst
    W = sum((V2.t() @ A @ V) ** 2 for A in maps)                                  # [m, n]
    unit = lambda e: torch.exp(torch.complex(torch.zeros(times.numel(), e.numel(), dtype=F64), times[:, None] * e[None, :]))  # noqa: E731
    G = unit(-theta2) @ W.to(torch.complex128)                                    # [k, n] = sum_m e^{-i E_m t_k} W[m, n]
    return logsum, torch.einsum("bn,kn->bk", prob.to(torch.complex128), unit(theta) * G)


def _tpq_block_dynamics(src, dst, apply, dots, parts, betas, dt, steps, R, seed, tol):
    """(log weights [B], C [B, K + 1]) of a sector pair from the thermal pure quantum states of ``_tpq_states`` on ``src``, for a
    map given as ``apply(c, X)`` (the block A X on the device) and ``dots(c, Lft, X)`` (the host column dots of Lft with A X):
    per beta and per real part c of the weights, b_0 = Phi and a_0 = A Phi are stepped by ``time_evolve`` over dt on the source
    and on the destination, and at every step two ``dots`` calls on the (re | im) blocks give
    C_j(t_k) = <A b_k,j | a_k,j> = [d(a_re, b_re) + d(a_im, b_im)] + i [d(a_im, b_re) - d(a_re, b_im)]"""
    from .chebyshev import spectral_bounds, time_evolve
    bounds_src = spectral_bounds(src, seed=seed)
    bounds_dst = bounds_src if dst is src else spectral_bounds(dst, seed=seed)
    logweights, rows = [], []
    for Phi, _, _, w, logweight in _tpq_states(src, betas, R, seed, tol, bounds_src):
        Cj = torch.zeros((steps + 1, R), dtype=torch.complex128)
        for c in parts:
            b = torch.complex(Phi, torch.zeros_like(Phi))
            a0 = apply(c, Phi)
            a = torch.complex(a0, torch.zeros_like(a0))
            for k in range(steps + 1):
                if k:
                    b = time_evolve(src, b, dt, bounds_src, tol)
                    a = time_evolve(dst, a, dt, bounds_dst, tol)
                bb = torch.cat([b.real, b.imag], dim=1)
                d1 = dots(c, torch.cat([a.real, a.imag], dim=1), bb)
                d2 = dots(c, torch.cat([a.imag, a.real], dim=1), bb)
                Cj[k] += torch.complex(d1[:R] + d1[R:], d2[:R] - d2[R:])
        logweights.append(logweight)
        rows.append((Cj * w).sum(dim=1) / w.sum())
    return torch.stack(logweights), torch.stack(rows)


def _tpq_pair_dynamics(src, dst, lad, parts, betas, dt, steps, R, seed, tol):
    """``_tpq_block_dynamics`` for one ladder: ``lad.apply_block`` and ``lad.block_dots``"""
    parts = [c.to(lad.device) for c in parts]
    return _tpq_block_dynamics(src, dst, lad.apply_block, lambda c, Lft, X: lad.block_dots(c, Lft, X).cpu(), parts, betas, dt,
                               steps, R, seed, tol)


def thermal_dynamics(L, bonds, couplings, weights, channel, betas, dt, steps, R=8, seed=0, dense_below=256, sectors=None,
                     tol=1e-15, device=None):
    """The finite-temperature correlation function of A = sum_i c_i O_i for the model and the parameter order of
    ``spin_thermodynamics`` (docs/design/35-finite-temperature-dynamics.md): a ``ThermalDynamics`` with

        C(t_k) = (1 / Z) sum_sectors tr_src[ e^{-beta H} e^{i H t_k} A^T e^{-i H' t_k} A ],    t_k = k dt,  k = 0 .. steps

    at the ascending inverse temperatures ``betas`` >= 0.  ``channel`` "zz", "-" or "+": O = Z, sigma^- or sigma^+ (the channels
    of ``spectral.dynamical_structure_factor``), which take the source sector ndown to ndown, ndown + 1 or ndown - 1 with the
    Hamiltonian H'.  ``weights``: a real vector [L], a ``(re, im)`` pair (``ring_momentum_weights``) or a complex tensor; for
    complex weights the result is the sum of the correlation functions of the real and of the imaginary part -- all matrices are
    real, so the cross terms cancel in the exact trace, and dropping them removes an estimator of zero.  ``sectors`` lists the
    SOURCE sectors (default 0 .. L): Z is the sum over them, and a source whose destination does not exist contributes to Z only.

    A sector pair with more than ``dense_below`` rows on either side is sampled by the R thermal pure quantum states of
    ``thermal_correlations`` on the source (same start vectors ``normal_vector(n, seed + j)``, same stepping in beta, same
    weights): a_0 = A |beta, j> by ``SpinSectorLadder.apply_block``, both sides stepped by ``chebyshev.time_evolve`` over dt on one
    ``spectral_bounds`` interval per sector, and C_j(t_k) = <A b_k,j | a_k,j> by two ``block_dots`` calls per step.  A smaller
    pair, and every pair with an edge sector (ndown = 0 or L) on one side, is exact on the host: the full spectra of both sides
    and the matrix of A from ``operators.sector_states``.  One pair of operators is alive at a time.  The error of a sampled
    pair is the sampling error of R vectors; it is not estimated.  Plain numbers: not differentiable."""
    from .operators import SpinSectorLadder, SpinSectorOperator
    from .spectral import _spin_step, _weight_parts
    step = _spin_step(channel)
    L, bonds, c, sectors, jz_sum, hz_sum, device = _spin_model(L, bonds, couplings, sectors, device)
    parts = [p.detach().cpu() for p in _weight_parts(weights)]
    if any(tuple(p.shape) != (L,) or not bool(torch.isfinite(p).all()) for p in parts):
        raise ValueError("weights must be %d finite site weights: a real vector, a (re, im) pair or a complex tensor" % L)
    betas = torch.as_tensor(betas, dtype=F64).detach().cpu().reshape(-1)
    if betas.numel() < 1 or not bool(torch.isfinite(betas).all()) or bool((betas < 0).any()) or bool((betas[1:] < betas[:-1]).any()):
        raise ValueError("betas must be finite, >= 0 and ascending")
    dt, steps, R = float(dt), int(steps), int(R)
    if not (dt > 0 and math.isfinite(dt)):
        raise ValueError("thermal_dynamics needs a finite dt > 0, got %r" % (dt,))
    if steps < 0:
        raise ValueError("thermal_dynamics needs steps >= 0, got %d" % steps)
    if R < 1:
        raise ValueError("thermal_dynamics needs R >= 1")
    times = dt * torch.arange(steps + 1, dtype=F64)
    on_device = [None]

    def operator(ndown):
        if on_device[0] is None:
            on_device[0] = c.to(device)
        return SpinSectorOperator(L, bonds, on_device[0], ndown, device)

    def spectrum(ndown, op):
        """(theta, V) of a side of a dense pair: the closed energy of an edge sector, host ``eigh`` otherwise"""
        if ndown in (0, L):
            return torch.tensor([jz_sum + (hz_sum if ndown == 0 else -hz_sum)], dtype=F64), torch.ones((1, 1), dtype=F64)
        return torch.linalg.eigh(_dense_sector_matrix(op))

    out = []
    for ndown in sectors:
        other = ndown + step
        if not 0 <= other <= L:
            out.append(_dense_pair_dynamics(spectrum(ndown, None), None, (), betas, times))
            continue
        edge = ndown in (0, L) or other in (0, L)
        src = None if ndown in (0, L) else operator(ndown)
        dst = src if step == 0 else (None if other in (0, L) else operator(other))
        if edge or max(math.comb(L, ndown), math.comb(L, other)) <= int(dense_below):
            spec_src = spectrum(ndown, src)
            spec_dst = spec_src if step == 0 else spectrum(other, dst)
            maps = [_dense_ladder_matrix(L, ndown, step, p) for p in parts]
            out.append(_dense_pair_dynamics(spec_src, spec_dst, maps, betas, times))
        else:
            lad = SpinSectorLadder(src, dst)
            out.append(_tpq_pair_dynamics(src, dst, lad, parts, betas, dt, steps, R, seed, tol))
            del lad
        del src, dst
    logw = torch.stack([p[0] for p in out])                                 # [sectors, B]
    logZ = torch.logsumexp(logw, dim=0)
    prob = torch.exp(logw - logZ)
    correlation = sum(prob[s][:, None] * out[s][1] for s in range(len(out)))
    return ThermalDynamics(betas, times, logZ, correlation)


class GrandCanonicalEnsemble:
    """Grand-canonical averages over a list of ``(measure, nup, ndn)``: ``measure`` a ``SpectralMeasure`` with
    sum_j w_j f(theta_j) = tr f(H) of the sector with ``nup`` up and ``ndn`` down particles (``sector_trace_measure`` on a
    ``HubbardOperator``).  Per pole N = nup + ndn, Sz = (nup - ndn) / 2 and K = theta - mu N; with
    p_j = w_j exp(-beta K_j) / Xi over all poles of all entries:

        logZ(beta, mu)                 ln Xi = ln sum_j w_j exp(-beta K_j)     (log-sum-exp shifted by the lowest K per (beta, mu))
        energy(beta, mu)               <H> = sum_j p_j theta_j
        density(beta, mu)              <N> = sum_j p_j N_j
        compressibility(beta, mu)      beta sum_j p_j (N_j - <N>)^2 = d<N> / d mu
        spin_susceptibility(beta, mu)  beta sum_j p_j (Sz_j - <Sz>)^2
        specific_heat(beta, mu)        beta^2 sum_j p_j (K_j - <K>)^2: the specific heat at FIXED mu, not at fixed <N>
        entropy(beta, mu)              ln Xi + beta (<H> - mu <N>)
        moment(p)                      sum_j w_j theta_j^p = tr H^p

    ``beta`` >= 0 and ``mu`` are numbers or tensors that broadcast against each other; the results are host float64 tensors of
    the broadcast shape.  The variances are sums of squared deviations, not differences of two means.  A list of sectors that all
    share N is the canonical ensemble: mu then only shifts ln Xi by beta mu N.  Plain numbers: not differentiable."""

    def __init__(self, entries):
        entries = list(entries)
        if not entries:
            raise ValueError("GrandCanonicalEnsemble needs at least one (measure, nup, ndn) entry")
        poles, weights, ns, szs = [], [], [], []
        for entry in entries:
            if not (isinstance(entry, (tuple, list)) and len(entry) == 3 and isinstance(entry[0], SpectralMeasure)):
                raise ValueError("every entry must be a (SpectralMeasure, nup, ndn) triple, got %r" % (entry,))
            measure, nup, ndn = entry
            poles.append(measure.poles)
            weights.append(measure.weights)
            ns.append(torch.full((len(measure),), float(nup) + float(ndn), dtype=F64))
            szs.append(torch.full((len(measure),), 0.5 * (float(nup) - float(ndn)), dtype=F64))
        self.entries = [(e[0], int(e[1]), int(e[2])) for e in entries]
        self.poles, self.weights = torch.cat(poles), torch.cat(weights)
        self.N, self.Sz = torch.cat(ns), torch.cat(szs)
        if self.poles.numel() == 0:
            raise ValueError("GrandCanonicalEnsemble needs at least one pole")
        if bool((self.weights < 0).any()):
            raise ValueError("the weights of a trace measure must not be negative")

    def _boltzmann(self, beta, mu):
        """(beta [...], mu [...], K [..., poles], its lowest value [...], sum_j w_j exp(-beta (K_j - lowest)) [...], p [..., poles])"""
        beta = torch.as_tensor(beta, dtype=F64).detach().cpu()
        mu = torch.as_tensor(mu, dtype=F64).detach().cpu()
        if bool((beta < 0).any()):
            raise ValueError("GrandCanonicalEnsemble works at inverse temperatures beta >= 0")
        beta, mu = torch.broadcast_tensors(beta, mu)
        K = self.poles - mu.unsqueeze(-1) * self.N
        lowest = K.min(dim=-1).values
        terms = self.weights * torch.exp(-beta.unsqueeze(-1) * (K - lowest.unsqueeze(-1)))
        total = terms.sum(dim=-1)
        return beta, mu, K, lowest, total, terms / total.unsqueeze(-1)

    @staticmethod
    def _variance(p, values):
        mean = (p * values).sum(dim=-1)
        return (p * (values - mean.unsqueeze(-1)) ** 2).sum(dim=-1)

    def logZ(self, beta, mu):
        beta, _, _, lowest, total, _ = self._boltzmann(beta, mu)
        return torch.log(total) - beta * lowest

    def energy(self, beta, mu):
        p = self._boltzmann(beta, mu)[-1]
        return (p * self.poles).sum(dim=-1)

    def density(self, beta, mu):
        p = self._boltzmann(beta, mu)[-1]
        return (p * self.N).sum(dim=-1)

    def compressibility(self, beta, mu):
        beta, _, _, _, _, p = self._boltzmann(beta, mu)
        return beta * self._variance(p, self.N)

    def spin_susceptibility(self, beta, mu):
        beta, _, _, _, _, p = self._boltzmann(beta, mu)
        return beta * self._variance(p, self.Sz)

    def specific_heat(self, beta, mu):
        """beta^2 (<K^2> - <K>^2) with K = H - mu N: the specific heat at fixed chemical potential"""
        beta, _, K, _, _, p = self._boltzmann(beta, mu)
        return beta ** 2 * self._variance(p, K)

    def entropy(self, beta, mu):
        beta, _, K, lowest, total, p = self._boltzmann(beta, mu)
        return torch.log(total) - beta * lowest + beta * (p * K).sum(dim=-1)

    def moment(self, p):
        return float((self.weights * self.poles ** int(p)).sum())


def one_species_matrix(L, bonds, couplings, count, other_full):
    """The dense Hamiltonian (host float64, rows in the order of ``sector_states(L, count)``) that one species of the Hubbard
    model of ``HubbardOperator`` sees when it has ``count`` particles and the OTHER species is empty (``other_full`` False) or
    full: the in-species hops -t_t (-1)^(particles strictly between a_t and b_t), and the diagonal of the full model with the
    other species' bits all 0 or all 1.  ``couplings`` = [t(nb), V(nb), U(L), eps(L)] as a host tensor."""
    from .operators import sector_states
    nb = len(bonds)
    c = torch.as_tensor(couplings, dtype=F64).detach().cpu()
    t, V, U, eps = c[:nb], c[nb:2 * nb], c[2 * nb:2 * nb + L], c[2 * nb + L:]
    states = torch.tensor(sector_states(L, count), dtype=torch.int64)
    n = states.numel()
    f = 1 if other_full else 0
    occ = [((states >> i) & 1) + f for i in range(L)]
    diag = torch.zeros(n, dtype=F64)
    for i in range(L):
        diag = diag + U[i] * (((states >> i) & 1) * f).to(F64) + eps[i] * occ[i].to(F64)
    H = torch.zeros((n, n), dtype=F64)
    rows = torch.arange(n)
    for k, (a, b) in enumerate(bonds):
        diag = diag + V[k] * (occ[a] * occ[b]).to(F64)
        lo, hi = min(a, b), max(a, b)
        moves = (((states >> a) ^ (states >> b)) & 1).bool()
        src = rows[moves]
        w = states[moves]
        jumped = torch.zeros_like(w)
        for i in range(lo + 1, hi):
            jumped = jumped + ((w >> i) & 1)
        amp = -t[k] * (1.0 - 2.0 * (jumped & 1).to(F64))
        dst = torch.searchsorted(states, w ^ ((1 << a) | (1 << b)))
        H.index_put_((dst, src), amp, accumulate=True)
    H[rows, rows] += diag
    return H


def _hubbard_model(what, L, bonds, couplings, sectors, edge_dense_max, device):
    """The argument checks that ``hubbard_thermodynamics`` and ``hubbard_density_of_states`` share (``ValueError`` in the name of
    ``what``, before any sector is computed): (L, bonds, couplings, sectors, device) as ``_hubbard_sector_sweep`` takes them"""
    from .operators import _check_bonds
    L = int(L)
    if not 2 <= L <= _lib.SECTOR_MAX_L:
        raise ValueError("%s needs 2 <= L <= %d, got %d" % (what, _lib.SECTOR_MAX_L, L))
    bonds = _check_bonds(L, bonds)
    nb = len(bonds)
    c = torch.as_tensor(couplings, dtype=F64).detach()
    if tuple(c.shape) != (2 * nb + 2 * L,):
        raise ValueError("couplings must have shape (%d,): t(nb), V(nb), U(L), eps(L)" % (2 * nb + 2 * L))
    if sectors is None:
        sectors = [(a, b) for a in range(L + 1) for b in range(L + 1)]
    else:
        sectors = [(int(a), int(b)) for a, b in sectors]
    if not sectors or any(not (0 <= a <= L and 0 <= b <= L) for a, b in sectors) or len(set(sectors)) != len(sectors):
        raise ValueError("sectors must be distinct pairs (nup, ndn) with both counts in 0 .. %d" % L)
    for nup, ndn in sectors:                                    # (refused before any sector is computed)
        if (nup in (0, L)) != (ndn in (0, L)):
            n = math.comb(L, ndn if nup in (0, L) else nup)
            if n > int(edge_dense_max):
                raise ValueError("the edge sector (nup, ndn) = (%d, %d) has a one-species dimension of %d, above edge_dense_max = %d"
                                 % (nup, ndn, n, int(edge_dense_max)))
    if device is None:
        device = c.device if c.is_cuda else "cuda"
    return L, bonds, c, sectors, device


def _hubbard_sector_sweep(L, bonds, c, sectors, device, spin_symmetric, exact, bulk):
    """The sector bookkeeping that ``hubbard_thermodynamics`` and ``hubbard_density_of_states`` share, on the checked arguments
    of ``_hubbard_model``: [(value, nup, ndn)] over the sectors in the caller's order.  An edge sector -- a species empty or
    full -- gives ``exact(poles)`` with the host float64 eigenvalues of ``one_species_matrix`` (both species frozen: the one
    energy); a bulk sector gives ``bulk(op)`` of its ``HubbardOperator``, which is released before the next is built.
    ``spin_symmetric``: (a, b) and (b, a) share the value computed for nup >= ndn."""
    from .operators import HubbardOperator
    host = c.cpu()
    on_device = None

    def value(nup, ndn):
        nonlocal on_device
        frozen = [s for s in (nup, ndn) if s in (0, L)]
        if len(frozen) == 2:
            return exact(one_species_matrix(L, bonds, host, nup, ndn == L).reshape(1))
        if frozen:
            count, other = (ndn, nup) if nup in (0, L) else (nup, ndn)
            return exact(torch.linalg.eigvalsh(one_species_matrix(L, bonds, host, count, other == L)))
        if on_device is None:
            on_device = c.to(device)
        op = HubbardOperator(L, bonds, on_device, nup, ndn, device)
        out = bulk(op)
        del op
        return out

    entries, done = [], {}
    for nup, ndn in sectors:
        key = (max(nup, ndn), min(nup, ndn)) if spin_symmetric else (nup, ndn)
        if key not in done:
            done[key] = value(*key)
        entries.append((done[key], nup, ndn))
    return entries


def hubbard_thermodynamics(L, bonds, couplings, R=8, k=100, seed=0, dense_below=256, sectors=None, spin_symmetric=True,
                           edge_dense_max=4096, device=None):
    """The ``GrandCanonicalEnsemble`` of the Hubbard model of ``HubbardOperator`` (its Hamiltonian and its parameter order
    [t(nb), V(nb), U(L), eps(L)]) over all sectors (nup, ndn) in {0 .. L}^2, or over the list ``sectors`` of distinct pairs.

    A bulk sector, 1 <= nup, ndn <= L - 1, contributes ``sector_trace_measure(op, R, k, seed, dense_below)`` of its
    ``HubbardOperator``; one sector's operator and tables are released before the next is built.  An edge sector -- a species
    empty or full, which the operator refuses -- is always exact: the other species sees ``one_species_matrix``, whose
    eigenvalues (host ``eigvalsh``) enter with weight 1; a one-species dimension above ``edge_dense_max`` raises ``ValueError``;
    both species frozen is one state from host arithmetic.  ``spin_symmetric=True``: H has no spin-dependent term, so the
    sectors (a, b) and (b, a) share a spectrum; only nup >= ndn is computed and the measure is entered for both."""
    model = _hubbard_model("hubbard_thermodynamics", L, bonds, couplings, sectors, edge_dense_max, device)
    return GrandCanonicalEnsemble(_hubbard_sector_sweep(
        *model, spin_symmetric,
        lambda poles: SpectralMeasure(poles, torch.ones(poles.numel(), dtype=F64), float(poles.numel()), poles.numel()),
        lambda op: sector_trace_measure(op, R=R, k=k, seed=seed, dense_below=dense_below)))


def hubbard_density_of_states(L, bonds, couplings, M, R=8, seed=0, dense_below=256, sectors=None, spin_symmetric=True,
                              edge_dense_max=4096, bounds=None, device=None):
    """The ``chebyshev.ChebyshevMeasure`` of the spectrum of the model of ``hubbard_thermodynamics`` over all sectors (nup, ndn)
    in {0 .. L}^2, or over the list ``sectors``: mu_m ~= tr T_m over the listed sectors, so that over all of them mu_0 = 4^L,
    ``density(E) / 4^L`` is the normalised density of states and ``logtrace_exp(beta)`` is ln Z at zero chemical potential
    (docs/design/34-hubbard-chebyshev.md).  All sectors are expanded on ONE interval, so their moments add: ``bounds``, or by
    default the rigorous (-B, B) with B = sum_t (2 |t_t| + 4 |V_t|) + sum_i (|U_i| + 2 |eps_i|) >= ||H|| in every sector.  A bulk
    sector contributes ``sector_density_of_states(op, M, bounds, R, seed, dense_below)`` of its ``HubbardOperator``, on the fused
    Hubbard moments kernel; an edge sector is exact, sum_i T_m of the eigenvalues of ``one_species_matrix`` or of the one frozen
    state.  The sectors, their refusals (``ValueError`` before any sector is computed) and ``spin_symmetric`` are those of
    ``hubbard_thermodynamics``."""
    from .chebyshev import ChebyshevMeasure, _check_bounds
    M = int(M)
    if M < 2 or int(R) < 1:
        raise ValueError("hubbard_density_of_states needs M >= 2 and R >= 1, got %d and %d" % (M, int(R)))
    model = _hubbard_model("hubbard_density_of_states", L, bonds, couplings, sectors, edge_dense_max, device)
    if bounds is None:
        L, nb = model[0], len(model[1])
        host = model[2].cpu().abs()
        B = float(2.0 * host[:nb].sum() + 4.0 * host[nb:2 * nb].sum() + host[2 * nb:2 * nb + L].sum() + 2.0 * host[2 * nb + L:].sum())
        bounds = (-B, B)
    centre, h = _check_bounds(bounds)
    entries = _hubbard_sector_sweep(
        *model, spin_symmetric,
        lambda poles: ChebyshevMeasure(_trace_moments(poles, M, centre, h), bounds),
        lambda op: sector_density_of_states(op, M, bounds, R=R, seed=seed, dense_below=dense_below))
    total = entries[0][0]
    for part, _, _ in entries[1:]:
        total = total + part
    return total


class HubbardThermalDynamics:
    """What ``hubbard_thermal_dynamics`` returns, host tensors: ``betas`` [B], ``mus`` [M], ``times`` [K + 1] with t_k = k dt,
    ``logXi`` [B, M] and ``correlation`` [B, M, K + 1] (complex128), C(t_k; beta, mu) = tr[e^{-beta (H - mu N)} A^T(t_k) A] / Xi."""

    def __init__(self, betas, mus, times, logXi, correlation):
        self.betas, self.mus, self.times, self.logXi, self.correlation = betas, mus, times, logXi, correlation

    def static(self):
        """C(0).real [B, M]: the equal-time correlation <A^T A>"""
        return self.correlation[:, :, 0].real.clone()

    def spectrum(self, omega, eta, reflected=False):
        """[B, M, len omega]: the Gaussian-windowed transform of ``ThermalDynamics.spectrum`` at every (beta, mu), with the same
        duties of the caller towards dt and K.  ``reflected=True`` evaluates it at -omega, which places a removal channel at
        omega = E_n - E_m <= 0 of the added-particle axis: ``cdag.spectrum(omega, eta) + c.spectrum(omega, eta, reflected=True)``
        is the one-particle A(omega), as ``SpectralMeasure.reflected`` gives it at T = 0."""
        omega = torch.as_tensor(omega, dtype=F64).detach().cpu().reshape(-1)
        B, M, K1 = self.correlation.shape
        flat = _windowed_spectrum(self.times, self.correlation.reshape(B * M, K1), -omega if reflected else omega, eta)
        return flat.reshape(B, M, -1)


def _dense_hubbard_ladder_matrix(L, nup_src, ndn_src, species, step, w):
    """the n_dst x n_src host matrix of sum_i w_i c+_{i s} (step +1), c_{i s} (step -1) or n_{i s} (step 0) of the species
    ``species`` ("up" or "dn") from the sector (nup_src, ndn_src), rows r = ru * n_dn + rd on ``sector_states`` of both species
    (edge sectors included): the running parity of the moving species' word below the site, and the sector sign (-1)^nup_src
    of a down operator with step +-1 (it stands right of all up operators)"""
    from .operators import sector_states
    count = nup_src if species == "up" else ndn_src
    src, dst = sector_states(L, count), sector_states(L, count + step)
    A = torch.zeros((len(dst), len(src)), dtype=F64)
    w = w.tolist()
    if step == 0:
        for r, word in enumerate(dst):
            A[r, r] = sum(w[i] * ((word >> i) & 1) for i in range(L))
    else:
        rank = {word: r for r, word in enumerate(src)}
        want = 1 if step > 0 else 0
        for r, word in enumerate(dst):
            for i in range(L):
                if (word >> i) & 1 == want:
                    A[r, rank[word ^ (1 << i)]] = w[i] * (1 - 2 * (bin(word & ((1 << i) - 1)).count("1") & 1))
    if species == "up":
        return torch.kron(A, torch.eye(math.comb(L, ndn_src), dtype=F64))
    g = -1.0 if step != 0 and nup_src & 1 else 1.0
    return torch.kron(torch.eye(math.comb(L, nup_src), dtype=F64), g * A)


def hubbard_thermal_dynamics(L, bonds, couplings, weights, channel, betas, mus, dt, steps, R=8, seed=0, dense_below=256,
                             sectors=None, edge_dense_max=4096, tol=1e-15, device=None):
    """The finite-temperature correlation function of A = sum_i w_i O_i for the Hubbard model and the parameter order
    [t(nb), V(nb), U(L), eps(L)] of ``hubbard_thermodynamics`` (docs/design/37-hubbard-finite-temperature-dynamics.md): a
    ``HubbardThermalDynamics`` with

        C(t_k; beta, mu) = (1 / Xi) sum_src e^{beta mu N_src} tr_src[ e^{-beta H} e^{i H t_k} A^T e^{-i H' t_k} A ],
        Xi = sum_src e^{beta mu N_src} tr e^{-beta H},    t_k = k dt,  k = 0 .. steps

    at the ascending inverse temperatures ``betas`` >= 0 and the chemical potentials ``mus``.  ``channel`` is one of
    ``spectral.hubbard_spectral_function``: "c_up", "c_dn", "cdag_up", "cdag_dn" (one particle of that species less or more, the
    Hamiltonian H' of the destination), "n" and "sz" (O_i = n_{i up} +- n_{i dn}, H' = H).  ``weights``: a real vector [L], a
    ``(re, im)`` pair (``ring_momentum_weights``) or a complex tensor; for complex weights the result is the sum of the
    correlation functions of the real and of the imaginary part (all matrices are real, so the cross terms cancel in the exact
    trace).  ``sectors`` lists the SOURCE pairs (nup, ndn), default all (L + 1)^2.  A sector's trace does not depend on mu: every
    mu comes from one sweep over the sectors, combined by a log-sum-exp of log weight + beta mu N_src.

    A source whose destination does not exist (the count would leave 0 .. L) contributes to Xi only.  A pair whose two sides
    are bulk (1 <= nup, ndn <= L - 1) with more than ``dense_below`` rows on either side is sampled by the R thermal pure
    quantum states of ``thermal_correlations`` on the source (start vectors ``normal_vector(n, seed + j)``): a_0 = A |beta, j> by
    ``HubbardLadder.apply_block``, both sides stepped by ``chebyshev.time_evolve`` over dt on one ``spectral_bounds`` interval per
    sector, C_j(t_k) = <A b_k,j | a_k,j> by ``block_dots`` on the (re | im) blocks; "n" and "sz" apply the step-0 ladders of both
    species and add them with the sign +-1.  A smaller pair, and every pair with an edge side (a species empty or full, which
    ``HubbardOperator`` refuses), is exact on the host: the spectrum of a bulk side from ``apply_block`` on identity columns,
    that of an edge side from ``one_species_matrix`` or the one frozen energy, the matrix of A from ``operators.sector_states``
    with the fermion signs.  AN EDGE SIDE IS NOT ONE STATE: the other side of such a pair has up to L C(L, k) rows, and a pair
    with an edge side and more than ``edge_dense_max`` rows on either side raises ``ValueError`` before any sector is computed.
    One pair of operators is alive at a time; (a, b) and (b, a) are computed separately.  The error of a sampled pair is the
    sampling error of R vectors; it is not estimated.  Plain numbers: not differentiable."""
    from .operators import HubbardLadder, HubbardOperator
    from .spectral import _HUBBARD_CHANNELS, _weight_parts
    what = "hubbard_thermal_dynamics"
    if channel not in _HUBBARD_CHANNELS:
        raise ValueError("channel must be one of %s, got %r" % (", ".join(repr(c) for c in _HUBBARD_CHANNELS), channel))
    species, step = _HUBBARD_CHANNELS[channel]
    sign = -1.0 if channel == "sz" else 1.0
    L, bonds, c, sectors, device = _hubbard_model(what, L, bonds, couplings, sectors, edge_dense_max, device)
    parts = [p.detach().cpu() for p in _weight_parts(weights)]
    if any(tuple(p.shape) != (L,) or not bool(torch.isfinite(p).all()) for p in parts):
        raise ValueError("weights must be %d finite site weights: a real vector, a (re, im) pair or a complex tensor" % L)
    betas = torch.as_tensor(betas, dtype=F64).detach().cpu().reshape(-1)
    if betas.numel() < 1 or not bool(torch.isfinite(betas).all()) or bool((betas < 0).any()) or bool((betas[1:] < betas[:-1]).any()):
        raise ValueError("betas must be finite, >= 0 and ascending")
    mus = torch.as_tensor(mus, dtype=F64).detach().cpu().reshape(-1)
    if mus.numel() < 1 or not bool(torch.isfinite(mus).all()):
        raise ValueError("mus must be at least one finite chemical potential")
    dt, steps, R = float(dt), int(steps), int(R)
    if not (dt > 0 and math.isfinite(dt)):
        raise ValueError("%s needs a finite dt > 0, got %r" % (what, dt))
    if steps < 0:
        raise ValueError("%s needs steps >= 0, got %d" % (what, steps))
    if R < 1:
        raise ValueError("%s needs R >= 1" % what)
    times = dt * torch.arange(steps + 1, dtype=F64)
    host = c.cpu()
    rows = lambda pair: math.comb(L, pair[0]) * math.comb(L, pair[1])           # noqa: E731
    is_edge = lambda pair: pair[0] in (0, L) or pair[1] in (0, L)              # noqa: E731

    def destination(nup, ndn):
        other = (nup + step, ndn) if species == "up" else (nup, ndn + step) if species == "dn" else (nup, ndn)
        return other if 0 <= other[0] <= L and 0 <= other[1] <= L else None

    routes = []
    for pair in sectors:                                         # (refused before any sector is computed)
        other = destination(*pair)
        if other is None:
            routes.append("none")
        elif is_edge(pair) or is_edge(other):
            if max(rows(pair), rows(other)) > int(edge_dense_max):
                raise ValueError("the pair (nup, ndn) = (%d, %d) -> (%d, %d) has an edge side and is exact on the host, but a "
                                 "side of %d rows, above edge_dense_max = %d"
                                 % (pair + other + (max(rows(pair), rows(other)), int(edge_dense_max))))
            routes.append("dense")
        else:
            routes.append("dense" if max(rows(pair), rows(other)) <= int(dense_below) else "sampled")
    on_device = [None]

    def operator(pair):
        if on_device[0] is None:
            on_device[0] = c.to(device)
        return HubbardOperator(L, bonds, on_device[0], pair[0], pair[1], device)

    def spectrum(pair, op):
        """(theta, V) of a side of a dense pair, rows r = ru * n_dn + rd: ``one_species_matrix`` of an edge side (the one energy
        when both species are frozen), host ``eigh`` of the operator's matrix otherwise"""
        nup, ndn = pair
        if nup in (0, L) and ndn in (0, L):
            return one_species_matrix(L, bonds, host, nup, ndn == L).reshape(1), torch.ones((1, 1), dtype=F64)
        if is_edge(pair):
            count, frozen = (ndn, nup) if nup in (0, L) else (nup, ndn)
            return torch.linalg.eigh(one_species_matrix(L, bonds, host, count, frozen == L))
        return torch.linalg.eigh(_dense_sector_matrix(op))

    def matrix(pair, w):
        if step != 0:
            return _dense_hubbard_ladder_matrix(L, pair[0], pair[1], species, step, w)
        return (_dense_hubbard_ladder_matrix(L, pair[0], pair[1], "up", 0, w)
                + sign * _dense_hubbard_ladder_matrix(L, pair[0], pair[1], "dn", 0, w))

    out = []
    for pair, route in zip(sectors, routes):
        other = destination(*pair)
        if route == "none":
            out.append(_dense_pair_dynamics(spectrum(pair, None), None, (), betas, times))
            continue
        src = None if is_edge(pair) else operator(pair)
        dst = src if step == 0 else (None if is_edge(other) else operator(other))
        if route == "dense":
            spec_src = spectrum(pair, src)
            spec_dst = spec_src if step == 0 else spectrum(other, dst)
            out.append(_dense_pair_dynamics(spec_src, spec_dst, [matrix(pair, p) for p in parts], betas, times))
        else:
            if step != 0:
                lads, signs = [HubbardLadder(src, dst, species)], [1.0]
            else:
                lads, signs = [HubbardLadder(src, dst, "up"), HubbardLadder(src, dst, "dn")], [1.0, sign]
            if len(lads) == 1:
                apply = lads[0].apply_block
                dots = lambda w, Lft, X: lads[0].block_dots(w, Lft, X).cpu()                              # noqa: E731
            else:
                apply = lambda w, X: lads[0].apply_block(w, X) + signs[1] * lads[1].apply_block(w, X)      # noqa: E731
                dots = lambda w, Lft, X: (lads[0].block_dots(w, Lft, X)                                    # noqa: E731
                                          + signs[1] * lads[1].block_dots(w, Lft, X)).cpu()
            out.append(_tpq_block_dynamics(src, dst, apply, dots, [p.to(device) for p in parts], betas, dt, steps, R, seed, tol))
            del lads, apply, dots
        del src, dst
    logw = torch.stack([p[0] for p in out])                                 # [sources, B]
    N = torch.tensor([float(a + b) for a, b in sectors], dtype=F64)
    logw = logw[:, :, None] + betas[None, :, None] * mus[None, None, :] * N[:, None, None]      # [sources, B, M]
    logXi = torch.logsumexp(logw, dim=0)
    prob = torch.exp(logw - logXi)
    correlation = sum(prob[s][:, :, None] * out[s][1][:, None, :] for s in range(len(out)))
    return HubbardThermalDynamics(betas, mus, times, logXi, correlation)


# ------------------------------------------------------------------------------------------ finite-temperature conductivity
class ThermalOpticalResponse:
    """What ``hubbard_thermal_conductivity`` returns (docs/design/40-finite-temperature-conductivity.md), host tensors:
    ``betas`` [B], ``mus`` [M], ``times`` [K + 1] with t_k = k dt, ``logXi`` [B, M], ``correlation`` [B, M, K + 1] (complex128),
    C(t_k; beta, mu) = tr[e^{-beta (H - mu N)} K^T(t_k) K] / Xi = <J(t_k) J> for the current J = i K(w), and ``diamagnetic``
    [B, M], K_d = <sum_t t_t d_t^2 sum_s (c+_{a s} c_{b s} + h.c.)>.  No volume factor, e = hbar = 1.  Plain numbers: not
    differentiable."""

    def __init__(self, betas, mus, times, logXi, correlation, diamagnetic):
        self.betas, self.mus, self.times, self.logXi = betas, mus, times, logXi
        self.correlation, self.diamagnetic = correlation, diamagnetic

    def static(self):
        """C(0).real [B, M]: the equal-time value <K^T K> = <J J>"""
        return self.correlation[:, :, 0].real.clone()

    def spectrum(self, omega, eta):
        """S_eta(omega) [B, M, len omega]: the Gaussian-windowed transform of ``ThermalDynamics.spectrum`` of C at every
        (beta, mu), (1 / 2 pi) int dt e^{i omega t} C(t) e^{-(eta t)^2 / 2}: a pair of levels with E_m - E_n = eps becomes a Gaussian
        of width ``eta`` at omega = eps.  THE CALLER picks dt and K: eta t_K >= 8, so that the window has decayed where the record
        ends, and pi / dt well above the band width, so that the trapezoid sum does not alias."""
        omega = torch.as_tensor(omega, dtype=F64).detach().cpu().reshape(-1)
        B, M, K1 = self.correlation.shape
        return _windowed_spectrum(self.times, self.correlation.reshape(B * M, K1), omega, eta).reshape(B, M, -1)

    def regular(self, omega, eta):
        """sigma_reg(omega) [B, M, len omega] = pi g_beta(omega) S_eta(omega), g_beta(omega) = (1 - e^{-beta omega}) / omega (beta at
        omega = 0, 0 at beta = 0), even in omega.  Pairs of levels with E_m = E_n carry the weight beta p_n |K_mn|^2 at omega = 0:
        the part of the Drude weight above the stiffness.  It is NOT separated: the broadened ``regular`` contains it as a
        Gaussian of width ``eta`` around omega = 0, and so do ``weight`` and ``stiffness``."""
        omega = torch.as_tensor(omega, dtype=F64).detach().cpu().reshape(-1)
        x = self.betas[:, None] * omega[None, :]                                        # [B, W]
        safe = torch.where(omega == 0, torch.ones_like(omega), omega)
        g = torch.where(omega[None, :] == 0, self.betas[:, None].expand_as(x), -torch.expm1(-x) / safe[None, :])
        return math.pi * g[:, None, :] * self.spectrum(omega, eta)

    def weight(self, omega, eta):
        """[B, M]: the trapezoid sum of ``regular`` over the caller's uniform ascending grid ``omega`` (at least two points),
        int sigma_reg d omega = pi X.  THE CALLER picks the grid: a spacing well below ``eta`` and a range that covers the band of
        excitations on both sides of omega = 0 by several ``eta`` AND NO MORE: at omega < 0 g_beta = (e^{beta |omega|} - 1) / |omega|
        multiplies S, which is e^{-beta |omega|} small there, and with it the rounding of the transform (about 1e-16 C(0)); a grid
        that reaches beta |omega| = 37 has lost every digit."""
        omega = torch.as_tensor(omega, dtype=F64).detach().cpu().reshape(-1)
        if omega.numel() < 2:
            raise ValueError("weight needs a grid of at least two frequencies")
        step = omega[1:] - omega[:-1]
        h = float(step[0])
        if not (h > 0 and bool(((step - h).abs() <= 1e-9 * abs(h)).all())):
            raise ValueError("weight needs a uniform ascending grid of frequencies")
        sigma = self.regular(omega, eta)
        return h * (sigma.sum(dim=-1) - 0.5 * (sigma[..., 0] + sigma[..., -1]))

    def stiffness(self, omega, eta):
        """[B, M]: K_d - weight / pi, the second derivative d^2 F / d phi^2 of the free energy F = -ln Xi / beta at fixed mu
        under the Peierls twist t_t -> t_t e^{i phi d_t} (the f-sum rule: pi K_d = pi stiffness + int sigma_reg), with the grid
        duties of ``weight``"""
        return self.diamagnetic - self.weight(omega, eta) / math.pi


def _current_weights(w, nb):
    """host float64 (2, nb) from a (2, nb) tensor or a (nb,) vector used for both species"""
    w = torch.as_tensor(w, dtype=F64).detach().cpu()
    if tuple(w.shape) == (nb,):
        w = torch.stack([w, w])
    if tuple(w.shape) != (2, nb):
        raise ValueError("expected bond weights of shape (2, %d) or (%d,), got %r" % (nb, nb, tuple(w.shape)))
    return w


def _one_species_current_matrix(L, bonds, w, count):
    """the host matrix of sum_t w_t (c+_a c_b - c+_b c_a) of one species with ``count`` particles on ``sector_states``: the row
    of a word with differing bits at a_t and b_t holds w_t o_t sgn_t at the column of the word with both flipped (o_t = +1 if
    bit a_t is set, else -1; sgn_t the parity of the particles strictly between).  An empty or full species: 0."""
    from .operators import sector_states
    states = sector_states(L, count)
    rank = {word: r for r, word in enumerate(states)}
    K = torch.zeros((len(states), len(states)), dtype=F64)
    w = w.tolist()
    for t, (a, b) in enumerate(bonds):
        lo, hi = min(a, b), max(a, b)
        between = ((1 << hi) - 1) & ~((1 << (lo + 1)) - 1)
        for r, word in enumerate(states):
            if ((word >> a) ^ (word >> b)) & 1:
                o = 1.0 if (word >> a) & 1 else -1.0
                sgn = -1.0 if bin(word & between).count("1") & 1 else 1.0
                K[r, rank[word ^ ((1 << a) | (1 << b))]] += w[t] * o * sgn
    return K


def _dense_hubbard_current_matrix(L, nup, ndn, bonds, w):
    """the n x n host matrix of K(w) on the sector (nup, ndn), rows r = ru * n_dn + rd on ``operators.sector_states`` of both
    species (edge sectors included): K_up(w_up) x 1 + 1 x K_dn(w_dn), each factor with the sign o_t sgn_t of
    docs/design/39-hubbard-current.md section 39.2; an empty or full species contributes 0.  Equal to -K^T bit for bit."""
    w = _current_weights(w, len(bonds))
    n_up, n_dn = math.comb(L, nup), math.comb(L, ndn)
    return (torch.kron(_one_species_current_matrix(L, bonds, w[0], nup), torch.eye(n_dn, dtype=F64))
            + torch.kron(torch.eye(n_up, dtype=F64), _one_species_current_matrix(L, bonds, w[1], ndn)))


def _dense_hubbard_diamagnetic_matrix(L, nup, ndn, bonds, td2):
    """the n x n host matrix of T_d = sum_t td2_t sum_s (c+_{a s} c_{b s} + h.c.) on the rows of ``_dense_hubbard_current_matrix``:
    T_up x 1 + 1 x T_dn, each factor ``one_species_matrix`` with the couplings [-td2, 0, 0, 0] (V = U = eps = 0, so that
    Hamiltonian is T_d exactly); both species frozen: 0"""
    nb = len(bonds)
    c_d = torch.cat([-torch.as_tensor(td2, dtype=F64).detach().cpu(), torch.zeros(nb + 2 * L, dtype=F64)])
    n_up, n_dn = math.comb(L, nup), math.comb(L, ndn)
    T_up = one_species_matrix(L, bonds, c_d, nup, False)
    T_dn = one_species_matrix(L, bonds, c_d, ndn, False)
    return torch.kron(T_up, torch.eye(n_dn, dtype=F64)) + torch.kron(torch.eye(n_up, dtype=F64), T_dn)


def _tpq_diamagnetic(op, td2, betas, R, seed, tol):
    """K_d [B] of a sampled sector: a pass over ``_tpq_states`` with the seed and the bounds of ``_tpq_block_dynamics`` (hence
    the same states); at every beta column j gives -sum_t td2_t Hadjoint_to_couplingsadjoint(phi_j, phi_j)[t] (the bond kinetic
    energies: dH / dt_t = -(hop_t + h.c.)), weighted by the column weights w_j like ``energy`` in ``_tpq_sector_correlations``"""
    from .chebyshev import spectral_bounds
    nb = td2.numel()
    rows = []
    for Phi, _, _, w, _ in _tpq_states(op, betas, R, seed, tol, spectral_bounds(op, seed=seed)):
        cols = []
        for j in range(R):
            phi = Phi[:, j].contiguous()
            cols.append(-(td2 * op.Hadjoint_to_couplingsadjoint(phi, phi).detach()[:nb].cpu()).sum())
        rows.append((w * torch.stack(cols)).sum() / w.sum())
    return torch.stack(rows)


def hubbard_thermal_conductivity(L, bonds, couplings, displacements, betas, mus, dt, steps, kind="charge", R=8, seed=0,
                                 dense_below=256, sectors=None, edge_dense_max=4096, tol=1e-15, device=None):
    """The finite-temperature optical response of the Hubbard model of ``hubbard_thermodynamics`` (parameter order [t(nb), V(nb),
    U(L), eps(L)]) to a uniform field (docs/design/40-finite-temperature-conductivity.md): a ``ThermalOpticalResponse`` with

        C(t_k; beta, mu) = (1 / Xi) sum_s e^{beta mu N_s} tr_s[ e^{-beta H} e^{i H t_k} K^T e^{-i H t_k} K ] = <J(t_k) J>,   t_k = k dt
        K_d(beta, mu)    = < sum_t t_t d_t^2 sum_s (c+_{a s} c_{b s} + h.c.) >

    at the ascending inverse temperatures ``betas`` >= 0 and the chemical potentials ``mus``, for the current J = i K(w) of
    ``HubbardCurrent`` with w = t_t d_t on both species (``kind="charge"``) or +t_t d_t on up and -t_t d_t on dn
    (``kind="spin"``), the hoppings t_t read from ``couplings[:nb]``.  ``displacements``: a real (nb,) vector d_t, the projection
    of r_b - r_a of bond t on the field direction, on a periodic cluster the MINIMUM IMAGE -- the caller's duty, as in
    ``spectral.optical_conductivity``.  From the result, sigma_reg(omega) = pi g_beta(omega) S(omega) (``regular``), its integral
    (``weight``) and d^2 F / d phi^2 = K_d - weight / pi (``stiffness``).

    ``sectors`` lists the pairs (nup, ndn), default all (L + 1)^2; K keeps both counts, so every sector maps to itself, and
    every mu comes from one sweep, combined by a log-sum-exp of log weight + beta mu N.  An edge sector (a species empty or
    full, which ``HubbardOperator`` refuses) and a bulk sector of at most ``dense_below`` rows are exact on the host: the
    spectrum from ``one_species_matrix`` or from ``apply_block`` on identity columns, K and T_d from ``operators.sector_states``
    with the fermion signs.  An edge sector above ``edge_dense_max`` rows raises ``ValueError`` before any sector is computed.
    A larger bulk sector is sampled by the R thermal pure quantum states of ``thermal_correlations`` (start vectors
    ``normal_vector(n, seed + j)``): a_0 = K |beta, j> by ``HubbardCurrent.apply_block``, both stepped by ``chebyshev.time_evolve``,
    C_j(t_k) = <K b_k,j | a_k,j> by ``HubbardCurrent.block_dots`` on the (re | im) blocks, and K_d from the bond kinetic energies
    of the same states in a second pass.  The error of a sampled sector is the sampling error of R vectors; it is not
    estimated.  Plain numbers: not differentiable."""
    from .operators import HubbardCurrent, HubbardOperator
    what = "hubbard_thermal_conductivity"
    if kind not in ("charge", "spin"):
        raise ValueError("kind must be 'charge' or 'spin', got %r" % (kind,))
    L, bonds, c, sectors, device = _hubbard_model(what, L, bonds, couplings, sectors, edge_dense_max, device)
    nb = len(bonds)
    d = torch.as_tensor(displacements)
    if d.is_complex() or d.dim() != 1 or d.numel() != nb:
        raise ValueError("displacements must be a real vector of %d elements (one per bond), got shape %r" % (nb, tuple(d.shape)))
    d = d.detach().cpu().to(F64)
    if not bool(torch.isfinite(d).all()):
        raise ValueError("displacements must be finite")
    betas = torch.as_tensor(betas, dtype=F64).detach().cpu().reshape(-1)
    if betas.numel() < 1 or not bool(torch.isfinite(betas).all()) or bool((betas < 0).any()) or bool((betas[1:] < betas[:-1]).any()):
        raise ValueError("betas must be finite, >= 0 and ascending")
    mus = torch.as_tensor(mus, dtype=F64).detach().cpu().reshape(-1)
    if mus.numel() < 1 or not bool(torch.isfinite(mus).all()):
        raise ValueError("mus must be at least one finite chemical potential")
    dt, steps, R = float(dt), int(steps), int(R)
    if not (dt > 0 and math.isfinite(dt)):
        raise ValueError("%s needs a finite dt > 0, got %r" % (what, dt))
    if steps < 0:
        raise ValueError("%s needs steps >= 0, got %d" % (what, steps))
    if R < 1:
        raise ValueError("%s needs R >= 1" % what)
    times = dt * torch.arange(steps + 1, dtype=F64)
    host = c.cpu()
    hop = host[:nb]
    wt = hop * d
    w = torch.stack([wt, wt if kind == "charge" else -wt])
    td2 = hop * d * d
    is_edge = lambda pair: pair[0] in (0, L) or pair[1] in (0, L)              # noqa: E731
    rows = lambda pair: math.comb(L, pair[0]) * math.comb(L, pair[1])           # noqa: E731
    on_device = [None]
    out = []
    for pair in sectors:
        nup, ndn = pair
        if is_edge(pair) or rows(pair) <= int(dense_below):
            if nup in (0, L) and ndn in (0, L):
                spec = (one_species_matrix(L, bonds, host, nup, ndn == L).reshape(1), torch.ones((1, 1), dtype=F64))
            elif is_edge(pair):
                count, frozen = (ndn, nup) if nup in (0, L) else (nup, ndn)
                spec = torch.linalg.eigh(one_species_matrix(L, bonds, host, count, frozen == L))
            else:
                if on_device[0] is None:
                    on_device[0] = c.to(device)
                op = HubbardOperator(L, bonds, on_device[0], nup, ndn, device)
                spec = torch.linalg.eigh(_dense_sector_matrix(op))
                del op
            logweight, C = _dense_pair_dynamics(spec, spec, [_dense_hubbard_current_matrix(L, nup, ndn, bonds, w)], betas, times)
            theta, V = spec
            kinetic = torch.einsum("rn,rs,sn->n", V, _dense_hubbard_diamagnetic_matrix(L, nup, ndn, bonds, td2), V)
            prob = torch.exp(-betas[:, None] * theta[None, :] - logweight[:, None])
            out.append((logweight, C, prob @ kinetic))
        else:
            if on_device[0] is None:
                on_device[0] = c.to(device)
            op = HubbardOperator(L, bonds, on_device[0], nup, ndn, device)
            cur = HubbardCurrent(op)
            logweight, C = _tpq_block_dynamics(op, op, cur.apply_block, lambda w_, Lft, X: cur.block_dots(w_, Lft, X).cpu(),
                                               [w.to(device)], betas, dt, steps, R, seed, tol)
            out.append((logweight, C, _tpq_diamagnetic(op, td2, betas, R, seed, tol)))
            del cur, op
    logw = torch.stack([p[0] for p in out])                                 # [sectors, B]
    N = torch.tensor([float(a + b) for a, b in sectors], dtype=F64)
    logw = logw[:, :, None] + betas[None, :, None] * mus[None, None, :] * N[:, None, None]      # [sectors, B, M]
    logXi = torch.logsumexp(logw, dim=0)
    prob = torch.exp(logw - logXi)
    correlation = sum(prob[s][:, :, None] * out[s][1][:, None, :] for s in range(len(out)))
    diamagnetic = sum(prob[s] * out[s][2][:, None] for s in range(len(out)))
    return ThermalOpticalResponse(betas, mus, times, logXi, correlation, diamagnetic)
