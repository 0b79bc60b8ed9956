"""Y = f(H) X for a block X without a stored basis, by a Chebyshev expansion (docs/design/31-chebyshev-propagator.md).

With the spectrum of H inside [a, b], centre = (a + b) / 2, h = (b - a) / 2 and s = (H - centre) / h,

    f(H) X ~= sum_{m < M} c_m T_m(s) X,     T_0 X = X,  T_1 X = s X,  T_{m+1} X = 2 s T_m X - T_{m-1} X

a three-term recurrence with no reductions, whose memory (X, two work blocks, one block per function) does not depend on M.
On a ``SpinSectorOperator`` every order is ONE launch of k_cheb_sector_block, on a ``HubbardOperator`` of k_cheb_hubbard_block
(docs/design/34-hubbard-chebyshev.md): the block mat-vec with the recurrence tail inside.

    chebyshev_coefficients(f, M)            c_0 / 2, c_1, ..., c_{M-1} of f on [-1, 1]
    exp_order(x, tol)                       the order that e^{-x (s + 1)} needs
    spectral_bounds(op, k, margin, seed)    (a, b) from a short Lanczos run, inside the rigorous bound where one is known
    chebyshev_apply(op, X, coeffs, bounds)  sum_m c_m T_m(s) X for one or two coefficient rows
    expm_block(op, X, tau)                  (Y, shift) with e^{-tau H} X = e^{-tau shift} Y
    time_evolve(op, psi, t)                 e^{-i H t} psi

and what the propagated block projects onto (docs/design/33-chebyshev-moments.md): the moments mu_m = <l| T_m(s) |x>, on a
``SpinSectorOperator`` or a ``HubbardOperator`` one launch of k_cheb_sector_moments or k_cheb_hubbard_moments per order with the
two dot products inside, two moments per order when l = x.  They do not depend on f: one run serves every function and the kernel polynomial method's densities.

    chebyshev_moments(op, X, M, bounds)     mu [M, R], optionally against a left block
    jackson_kernel(M), lorentz_kernel(M)    the damping factors g_m
    ChebyshevMeasure(moments, bounds)       density(E), trace(f), logtrace_exp(beta), shifted(E0), +

Plain host float64 numbers and detached blocks: nothing here is differentiable.
"""
from __future__ import annotations

import functools
import math
from ctypes import byref, c_double, c_int64, c_void_p

import numpy as np
import torch

from . import _lib, engine
from ._lib import check
from .thermal import _as_block, _sector_operator, block_lanczos_coefficients, block_pieces

F64 = torch.float64
LD = np.longdouble
FUSED_ACCUMULATORS = (1, 2)
COEFFICIENT_ROWS = 32


def chebyshev_coefficients(f, M, nodes=None):
    """c [M] (float64) with f(s) ~= sum_m c[m] T_m(s) on [-1, 1]; c[0] IS ALREADY HALVED.  Chebyshev-Gauss quadrature on
    ``nodes`` >= 2 M points (default 2 M): c_m = (2 / N) sum_k f(cos theta_k) cos(m theta_k), theta_k = pi (k + 1/2) / N,
    evaluated in ``numpy.longdouble`` and rounded once.  ``f`` takes and returns a longdouble array."""
    M = int(M)
    if M < 1:
        raise ValueError("chebyshev_coefficients needs M >= 1, got %d" % M)
    N = 2 * M if nodes is None else int(nodes)
    if N < 2 * M:
        raise ValueError("chebyshev_coefficients needs at least 2 M = %d nodes, got %d" % (2 * M, N))
    pi = 4 * np.arctan(LD(1))
    theta = pi * (np.arange(N, dtype=LD) + LD(0.5)) / LD(N)
    values = np.asarray(f(np.cos(theta)), dtype=LD)
    if values.shape != (N,):
        raise ValueError("f must map an array of %d nodes to %d values" % (N, N))
    c = np.empty(M, dtype=LD)
    for first in range(0, M, COEFFICIENT_ROWS):           # (a few rows of cos(m theta) at a time: memory O(N), not O(M N))
        m = np.arange(first, min(M, first + COEFFICIENT_ROWS), dtype=LD)
        c[first:first + m.size] = np.cos(m[:, None] * theta[None, :]) @ values
    c *= LD(2) / LD(N)
    c[0] = c[0] / LD(2)
    return c.astype(np.float64)


def _truncated_expansion(f, guess, tol):
    """(M, c): the order of ``truncation_order`` and the leading M coefficients of the long expansion that decided it"""
    if not 0 < float(tol) < 1:
        raise ValueError("the truncation tolerance must lie in (0, 1), got %r" % (tol,))
    K = max(8, int(guess))
    while True:
        c = chebyshev_coefficients(f, 2 * K)
        size = np.abs(c)
        if not size.max() > 0:                            # (f vanishes at every node, sin(0 s) for one: order 2 of zeros)
            return 2, c[:2]
        M = max(2, int(np.nonzero(size >= tol * size.max())[0][-1]) + 1)
        if M <= K:
            return M, c[:M]
        K *= 2


def truncation_order(f, guess, tol=1e-15):
    """The smallest M >= 2 after which every coefficient of an expansion of f twice as long is below tol max|c| (2 for a
    function that vanishes at every node).  ``guess`` is where the search starts; it doubles until the tail of the long
    expansion is small."""
    return _truncated_expansion(f, guess, tol)[0]


def _order_guess(x):
    return int(x + 9.0 * math.sqrt(x)) + 24


def exp_order(x, tol=1e-15):
    """The order M of e^{-x (s + 1)} on s in [-1, 1] (``truncation_order``); x >= 0.  The coefficients are 2 e^{-x} I_m(x) up
    to sign, so M grows like x + O(sqrt(x)) and is monotone in x."""
    x = float(x)
    if not (x >= 0 and math.isfinite(x)):
        raise ValueError("exp_order needs a finite x >= 0, got %r" % (x,))
    return truncation_order(lambda s: np.exp(-LD(x) * (s + LD(1))), _order_guess(x), tol)


def coupling_bound(op):
    """B >= ||H||_2 from the couplings alone: sum_t (2 |Jxy_t| + |Jz_t|) + sum_i |hz_i| of a ``SpinSectorOperator``,
    sum_t (2 |t_t| + 4 |V_t|) + sum_i (|U_i| + 2 |eps_i|) of a ``HubbardOperator`` (a hop has norm 1 per species, n_a n_b <= 4,
    n_up n_dn <= 1, n_i <= 2); None for another operator"""
    from .operators import HubbardOperator, SpinSectorOperator
    if isinstance(op, HubbardOperator):
        t, V, U, eps = op.unpack(op.couplings.detach())
        return float(2.0 * t.abs().sum() + 4.0 * V.abs().sum() + U.abs().sum() + 2.0 * eps.abs().sum())
    if not isinstance(op, SpinSectorOperator):
        return None
    jxy, jz, hz = op.unpack(op.couplings.detach())
    return float(2.0 * jxy.abs().sum() + jz.abs().sum() + hz.abs().sum())


def spectral_bounds(op, k=60, margin=0.05, seed=0):
    """(a, b) that should hold the spectrum of ``op``: the extreme Ritz values theta_min, theta_max of min(k, n) basis-free
    Lanczos steps on ``synthetic.normal_vector(n, seed)``, each widened by margin (theta_max - theta_min), then cut to the
    rigorous [-B, B] of ``coupling_bound`` where the operator has one.  The Ritz values lie INSIDE the spectrum: the margin is
    what covers the distance to its ends, it is not a proof."""
    op = _sector_operator(op, "spectral_bounds")
    if int(k) < 1 or not float(margin) > 0:
        raise ValueError("spectral_bounds needs k >= 1 and margin > 0")
    from .synthetic import normal_vector
    phi = torch.from_numpy(normal_vector(int(op.n), int(seed))).reshape(-1, 1).to(op.device)
    _, alphas, betas, steps = block_lanczos_coefficients(op, phi, k)
    s = max(1, int(steps[0]))
    T = torch.diag(alphas[:s, 0])
    if s > 1:
        T = T + torch.diag(betas[:s - 1, 0], 1) + torch.diag(betas[:s - 1, 0], -1)
    theta = torch.linalg.eigvalsh(T)
    lo, hi = float(theta[0]), float(theta[-1])
    pad = float(margin) * (hi - lo)
    if not pad > 0:                                   # (a one-dimensional Krylov space: any interval around the value does)
        pad = max(1.0, abs(lo)) * float(margin)
    a, b = lo - pad, hi + pad
    B = coupling_bound(op)
    if B is not None and B > 0:
        a, b = max(a, -B), min(b, B)
    return a, b


def _check_bounds(bounds):
    try:
        a, b = (float(v) for v in bounds)
    except (TypeError, ValueError):
        raise ValueError("bounds must be a pair (a, b) of numbers, got %r" % (bounds,)) from None
    if not (math.isfinite(a) and math.isfinite(b) and a < b):
        raise ValueError("bounds must be finite with a < b, got (%r, %r)" % (a, b))
    return 0.5 * (a + b), 0.5 * (b - a)


def _check_coeffs(coeffs):
    c = np.array(coeffs, dtype=np.float64, order="C")
    if c.ndim not in (1, 2) or c.shape[-1] < 2 or c.shape[0] < 1 or not np.isfinite(c).all():
        raise ValueError("coeffs must be finite, of shape (M,) or (A, M) with M >= 2, got shape %r" % (c.shape,))
    return c.reshape(-1, c.shape[-1]), c.ndim == 1


def chebyshev_apply(op, X, coeffs, bounds, fused=None):
    """sum_{m < M} coeffs[..., m] T_m((H - centre) / h) X for a device block X (n, R), any R >= 1, and ``bounds`` = (a, b) =
    (centre - h, centre + h), which must hold the spectrum of H.  ``coeffs`` (M,) returns (n, R); (A, M) returns (A, n, R):
    all A functions share the M - 1 mat-vecs.  c_0 is taken as given (``chebyshev_coefficients`` halves it).

    ``fused=True`` names the spin-sector entry: dsea_op_sector_block_chebyshev, one launch per order, ``SpinSectorOperator`` and
    A in {1, 2} only (``ValueError`` otherwise, for a ``HubbardOperator`` too), the columns in pieces of 8, 4, 2 and 1.
    ``fused=False``: ``op.apply_block`` and torch elementwise operations in exactly the order of the kernel's tail, for any
    operator with ``apply_block``; the two paths return the same bits.  ``None``: fused where an entry exists -- the spin-sector
    one, or for a ``HubbardOperator`` with A in {1, 2} dsea_op_hubbard_block_chebyshev, the same schedule on
    k_cheb_hubbard_block; ``None`` is how a Hubbard operator reaches its kernel.  X is detached and not written."""
    from .operators import HubbardOperator, SpinSectorOperator
    c, single = _check_coeffs(coeffs)
    centre, h = _check_bounds(bounds)
    A, M = c.shape
    can_fuse = isinstance(op, SpinSectorOperator) and A in FUSED_ACCUMULATORS
    if fused is None:
        fused = can_fuse or (isinstance(op, HubbardOperator) and A in FUSED_ACCUMULATORS)
    elif fused and not can_fuse:
        raise ValueError("the fused Chebyshev kernel exists for SpinSectorOperator and 1 or 2 coefficient rows only, got %s and %d"
                         % (type(op).__name__, A))
    if not callable(getattr(op, "apply_block", None)):
        raise ValueError("chebyshev_apply needs an operator with apply_block, got %s" % type(op).__name__)
    X = _as_block(op, X, "chebyshev_apply").to(F64)
    out = _apply_fused(op, X, c, centre, h) if fused else _apply_unfused(op, X, c, centre, h)
    return out[0] if single else out


def _aligned_piece(X, first, w):
    """columns first .. first + w of X as a contiguous block on a 16-byte boundary"""
    piece = X[:, first:first + w].contiguous()
    return piece.clone() if piece.data_ptr() % 16 else piece


def _fused_entries(op, lib):
    """(propagator, its name, scratch query of the moments with the sector's sizes bound, moments, their name): the fused ABI
    entries of the operator's kind"""
    from .operators import HubbardOperator
    if isinstance(op, HubbardOperator):
        return (lib.dsea_op_hubbard_block_chebyshev, "dsea_op_hubbard_block_chebyshev",
                lambda w, out: lib.dsea_op_hubbard_block_moments_scratch_doubles(op.N, op.nup, op.ndn, w, out),
                lib.dsea_op_hubbard_block_moments, "dsea_op_hubbard_block_moments")
    return (lib.dsea_op_sector_block_chebyshev, "dsea_op_sector_block_chebyshev",
            lambda w, out: lib.dsea_op_sector_block_moments_scratch_doubles(op.N, op.ndown, w, out),
            lib.dsea_op_sector_block_moments, "dsea_op_sector_block_moments")


def _apply_fused(op, X, c, centre, h):
    lib = _lib.load()
    run, name = _fused_entries(op, lib)[:2]
    A, M = c.shape
    n, R = X.shape
    host = (c_double * (A * M))(*c.reshape(-1).tolist())
    out = torch.empty((A, n, R), dtype=F64, device=X.device)
    ptr = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    for first, w in block_pieces(R):
        Xp = _aligned_piece(X, first, w)
        U, V = torch.empty_like(Xp), torch.empty_like(Xp)
        acc = torch.empty((A, n, w), dtype=F64, device=X.device)
        check(run(op.handle, w, A, M, centre, h, host, ptr(Xp), ptr(U), ptr(V), ptr(acc), engine._stream(X.device)), name)
        out[:, :, first:first + w] = acc
    return out


def _apply_unfused(op, X, c, centre, h):
    """the recurrence on ``op.apply_block`` with the tail of k_cheb_sector_block as separate elementwise operations, each
    rounded on its own: u = w - centre x, t = g u, (t -= old,) acc += c t"""
    A, M = c.shape
    c = c.tolist()
    x, old = X, None
    for m in range(1, M):
        t = ((1.0 if m == 1 else 2.0) / h) * (op.apply_block(x) - centre * x)
        if m == 1:
            acc = [c[a][0] * x + c[a][1] * t for a in range(A)]
        else:
            t = t - old
            acc = [acc[a] + c[a][m] * t for a in range(A)]
        old, x = x, t
    return torch.stack(acc)


def chebyshev_moments(op, X, M, bounds, left=None, fused=None):
    """mu [M, R] (host float64) with mu[m, j] = <l_j| T_m((H - centre) / h) |x_j> for a device block X (n, R), any R >= 1, M >= 2
    and ``bounds`` = (a, b) = (centre - h, centre + h), which must hold the spectrum of H; l = X unless a second block ``left``
    (n, R) is given (docs/design/33-chebyshev-moments.md).  Without ``left`` the product rule T_a T_b = (T_{a+b} + T_{|a-b|}) / 2
    gives two moments per order, mu_{2m-2} = 2 <T_{m-1} x|T_{m-1} x> - mu_0 and mu_{2m-1} = 2 <T_{m-1} x|T_m x> - mu_1: ceil(M / 2)
    mat-vecs; with ``left`` M - 1.

    ``fused=True`` names the spin-sector entry: dsea_op_sector_block_moments, one launch per order with the dot products inside
    and one small launch that closes them, ``SpinSectorOperator`` only (``ValueError`` otherwise, for a ``HubbardOperator``
    too), the columns in pieces of 8, 4, 2 and 1.  ``fused=False``: ``op.apply_block``, torch elementwise operations in the order
    of the kernel's tail and column sums, for any operator with ``apply_block``.  ``None``: fused where an entry exists -- the
    spin-sector one, or for a ``HubbardOperator`` dsea_op_hubbard_block_moments, the same schedule on k_cheb_hubbard_moments;
    ``None`` is how a Hubbard operator reaches its kernel.  The two paths run the same recurrence bit for bit but sum the dot
    products in different orders: their moments agree to rounding, NOT bit for bit.  X and ``left`` are detached and not
    written."""
    from .operators import HubbardOperator, SpinSectorOperator
    M = int(M)
    if M < 2:
        raise ValueError("chebyshev_moments needs M >= 2, got %d" % M)
    centre, h = _check_bounds(bounds)
    can_fuse = isinstance(op, SpinSectorOperator)
    if fused is None:
        fused = can_fuse or isinstance(op, HubbardOperator)
    elif fused and not can_fuse:
        raise ValueError("the fused moments kernel exists for SpinSectorOperator only, got %s" % type(op).__name__)
    if not callable(getattr(op, "apply_block", None)):
        raise ValueError("chebyshev_moments needs an operator with apply_block, got %s" % type(op).__name__)
    X = _as_block(op, X, "chebyshev_moments").to(F64)
    if left is not None:
        left = _as_block(op, left, "chebyshev_moments").to(F64)
        if left.shape != X.shape:
            raise ValueError("the left block must have the shape %r of X, got %r" % (tuple(X.shape), tuple(left.shape)))
    return (_moments_fused if fused else _moments_unfused)(op, X, left, M, centre, h)


def _moments_fused(op, X, left, M, centre, h):
    lib = _lib.load()
    dev = X.device
    ptr = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    _, _, query, run, name = _fused_entries(op, lib)
    out = []
    for first, w in block_pieces(X.shape[1]):
        Xp = _aligned_piece(X, first, w)
        Yp = None if left is None else _aligned_piece(left, first, w)
        U, V = torch.empty_like(Xp), torch.empty_like(Xp)
        mu = torch.empty((M, w), dtype=F64, device=dev)
        need = c_int64()
        check(query(w, byref(need)), name + "_scratch_doubles")
        scratch = torch.empty(need.value, dtype=F64, device=dev)
        check(run(op.handle, w, M, centre, h, ptr(Xp), None if Yp is None else ptr(Yp), ptr(U), ptr(V), ptr(mu), ptr(scratch),
                  engine._stream(dev)), name)
        out.append(mu.cpu())
    return torch.cat(out, dim=1)


def _moments_unfused(op, X, left, M, centre, h):
    """the orders of k_cheb_sector_moments on ``op.apply_block``: the tail as separate elementwise operations, each rounded on
    its own, the dot products as column sums, and the doubling of k_cheb_moments_finish"""
    mu = torch.empty((M, X.shape[1]), dtype=F64, device=X.device)
    x, old = X, None
    for m in range(1, (M if left is not None else (M + 1) // 2 + 1)):
        t = ((1.0 if m == 1 else 2.0) / h) * (op.apply_block(x) - centre * x)
        if m > 1:
            t = t - old
        l = x if left is None else left
        a, b = (l * x).sum(0), (l * t).sum(0)
        if m == 1:
            mu[0], mu[1] = a, b
        elif left is not None:
            mu[m] = b
        else:
            if 2 * m - 2 < M:
                mu[2 * m - 2] = 2.0 * a - mu[0]
            if 2 * m - 1 < M:
                mu[2 * m - 1] = 2.0 * b - mu[1]
        old, x = x, t
    return mu.cpu()


def jackson_kernel(M):
    """g [M] (float64): the Jackson damping factors g_m = [(M - m + 1) cos(pi m / (M + 1)) + sin(pi m / (M + 1)) cot(pi / (M + 1))]
    / (M + 1) of the kernel polynomial method: g_0 = 1, decreasing, and the damped density of a positive measure is positive
    with the resolution pi h / M"""
    M = int(M)
    if M < 1:
        raise ValueError("jackson_kernel needs M >= 1, got %d" % M)
    pi = 4 * np.arctan(LD(1))
    m = np.arange(M, dtype=LD)
    q = pi / LD(M + 1)
    return (((LD(M + 1) - m) * np.cos(m * q) + np.sin(m * q) / np.tan(q)) / LD(M + 1)).astype(np.float64)


def lorentz_kernel(M, lam=4.0):
    """g [M] (float64): the Lorentz damping factors g_m = sinh(lam (1 - m / M)) / sinh(lam), which turn a pole into a Lorentzian
    of width lam h / M (the kernel for Green's functions)"""
    M, lam = int(M), float(lam)
    if M < 1 or not (lam > 0 and math.isfinite(lam)):
        raise ValueError("lorentz_kernel needs M >= 1 and a finite lam > 0, got %d and %r" % (M, lam))
    m = np.arange(M, dtype=LD)
    return (np.sinh(LD(lam) * (LD(1) - m / LD(M))) / np.sinh(LD(lam))).astype(np.float64)


_KERNELS = {"jackson": jackson_kernel, "lorentz": lorentz_kernel}


class ChebyshevMeasure:
    """A measure on the interval ``bounds`` = (a, b) given by its M Chebyshev moments mu_m = int T_m((E - centre) / h) d mu(E):
    <x| . |x> of one vector (``spectral.kpm_measure``), or a trace (``thermal.sector_density_of_states``).  ``moments`` is a host
    float64 tensor [M].  The sum of two measures on the same interval with the same M adds their moments.  Plain numbers:
    nothing here is differentiable."""

    def __init__(self, moments, bounds):
        self.moments = torch.as_tensor(moments, dtype=F64).detach().cpu().reshape(-1).clone()
        if self.moments.numel() < 1 or not bool(torch.isfinite(self.moments).all()):
            raise ValueError("a ChebyshevMeasure needs at least one moment, all finite")
        self.centre, self.halfwidth = _check_bounds(bounds)
        self.bounds = (float(bounds[0]), float(bounds[1]))

    def __len__(self):
        return self.moments.numel()

    def _damping(self, kernel):
        M = len(self)
        if kernel is None:
            return np.ones(M)
        if isinstance(kernel, str):
            if kernel not in _KERNELS:
                raise ValueError("kernel must be one of %s, None or an array of %d factors, got %r"
                                 % (", ".join(repr(k) for k in sorted(_KERNELS)), M, kernel))
            return _KERNELS[kernel](M)
        g = np.array(kernel, dtype=np.float64)
        if g.shape != (M,) or not np.isfinite(g).all():
            raise ValueError("an array of damping factors must be finite and of shape (%d,), got %r" % (M, g.shape))
        return g

    def density(self, E, kernel="jackson"):
        """[g_0 mu_0 + 2 sum_{m >= 1} g_m mu_m T_m(s)] / (pi h sqrt(1 - s^2)) at the energies ``E`` (any shape) strictly inside
        the bounds, 0 outside; a host float64 tensor of the shape of E.  ``kernel``: "jackson", "lorentz", None (no damping) or
        an array of M factors.  cos(m arccos s) is formed a few orders at a time: host memory is O(len E)."""
        c = self._damping(kernel) * self.moments.numpy()
        c[1:] *= 2.0
        E = np.asarray(torch.as_tensor(E, dtype=F64).detach().cpu().numpy())
        s = (E.reshape(-1) - self.centre) / self.halfwidth
        inside = np.abs(s) < 1.0
        theta = np.arccos(s[inside])
        acc = np.zeros(theta.shape)
        for first in range(0, len(c), COEFFICIENT_ROWS):
            m = np.arange(first, min(len(c), first + COEFFICIENT_ROWS), dtype=np.float64)
            acc += c[first:first + m.size] @ np.cos(m[:, None] * theta[None, :])
        out = np.zeros(s.shape)
        out[inside] = acc / (math.pi * self.halfwidth * np.sqrt(1.0 - s[inside] ** 2))
        return torch.from_numpy(out.reshape(E.shape))

    def _expansion(self, g):
        """sum_m c_m mu_m with the coefficients of g(s) on [-1, 1] (c_0 halved as ``chebyshev_coefficients`` returns it)"""
        return float(np.dot(chebyshev_coefficients(g, len(self)), self.moments.numpy()))

    def trace(self, f):
        """sum_m c_m mu_m with the M Chebyshev coefficients of f on the bounds: the undamped estimate of int f d mu, that is of
        <x| f(H) |x> or tr f(H).  ``f`` takes and returns a ``numpy.longdouble`` array of energies."""
        centre, h = LD(self.centre), LD(self.halfwidth)
        return self._expansion(lambda s: f(centre + h * s))

    def logtrace_exp(self, beta):
        """ln int e^{-beta E} d mu(E) for beta >= 0 as -beta a + ln sum_m c_m mu_m with the coefficients of e^{-beta h (s + 1)},
        which are at most 1 (the shift of ``expm_block``); M should reach ``exp_order(beta h)``"""
        beta = float(beta)
        if not (beta >= 0 and math.isfinite(beta)):
            raise ValueError("logtrace_exp needs a finite beta >= 0, got %r" % (beta,))
        x = LD(beta * self.halfwidth)
        total = self._expansion(lambda s: np.exp(-x * (s + LD(1))))
        if not total > 0:
            raise ValueError("the expansion of e^{-beta H} sums to %r: too few moments for beta h = %g" % (total, float(x)))
        return math.log(total) - beta * self.bounds[0]

    def shifted(self, E0):
        """the same moments on the bounds moved by -E0: the measure as a function of E - E0"""
        return ChebyshevMeasure(self.moments, (self.bounds[0] - float(E0), self.bounds[1] - float(E0)))

    def __add__(self, other):
        if not isinstance(other, ChebyshevMeasure):
            return NotImplemented
        if other.bounds != self.bounds or len(other) != len(self):
            raise ValueError("only measures with the same bounds and the same number of moments add")
        return ChebyshevMeasure(self.moments + other.moments, self.bounds)

    def __repr__(self):
        return "ChebyshevMeasure(%d moments on [%.6g, %.6g], mu_0 = %.6g)" % (len(self), self.bounds[0], self.bounds[1],
                                                                              float(self.moments[0]))


def expm_block(op, X, tau, bounds=None, tol=1e-15):
    """(Y, shift) with e^{-tau H} X = e^{-tau shift} Y for a device block X (n, R) and tau >= 0: the expansion of
    e^{-tau (H - a)} = e^{-tau h (s + 1)} on ``bounds`` = (a, b) (``spectral_bounds(op)`` if None), shift = a, so that every
    coefficient is at most 1 and Y neither overflows nor vanishes with e^{-tau E0}.  The order is ``exp_order(tau h, tol)``,
    and the coefficients are those of the long expansion that decided it.  tau = 0 returns a copy of X with no device work;
    its shift is a where bounds are given and 0 where they are not (every shift is right at tau = 0, and none is worth a
    Lanczos run)."""
    tau = float(tau)
    if not (tau >= 0 and math.isfinite(tau)):
        raise ValueError("expm_block needs a finite tau >= 0, got %r" % (tau,))
    if tau == 0 and bounds is None:
        return _as_block(op, X, "expm_block").to(F64).clone(), 0.0
    if bounds is None:
        bounds = spectral_bounds(op)
    _, h = _check_bounds(bounds)
    a = float(bounds[0])
    if tau == 0:
        return _as_block(op, X, "expm_block").to(F64).clone(), a
    x = LD(tau * h)
    _, coeffs = _truncated_expansion(lambda s: np.exp(-x * (s + LD(1))), _order_guess(tau * h), tol)
    return chebyshev_apply(op, X, coeffs, bounds), a


@functools.lru_cache(maxsize=16)
def _evolution_rows(t, centre, h, tol):
    """[2, M]: the coefficient rows of cos and sin of H t = h t s + centre t.  Kept for the last few (t, interval) pairs: a time
    grid asks for the same rows at every step (``thermal.thermal_dynamics``).  Never written to."""
    w, phase = LD(h * t), LD(centre * t)
    fc = lambda s: np.cos(w * s + phase)  # noqa: E731
    fs = lambda s: np.sin(w * s + phase)  # noqa: E731
    guess = _order_guess(abs(h * t))
    found = [_truncated_expansion(f, guess, tol) for f in (fc, fs)]
    M = max(m for m, _ in found)
    rows = np.zeros((2, M))                     # (the shorter row is padded: its coefficients beyond its own order are below tol)
    for a, (m, c) in enumerate(found):
        rows[a, :m] = c
    rows.setflags(write=False)
    return rows


def time_evolve(op, psi, t, bounds=None, tol=1e-15):
    """e^{-i H t} psi (complex128) for a real or complex device tensor psi of shape (n,) or (n, R) and a real time t.  H is
    real, so the real and the imaginary parts are columns of ONE real block that goes through ONE ``chebyshev_apply`` with
    two coefficient rows, cos and sin of H t = h t s + centre t:  e^{-iHt} (p + i q) = (C p + S q) + i (C q - S p).
    t = 0 returns psi as a complex copy with no device work and no bounds."""
    t = float(t)
    if not math.isfinite(t):
        raise ValueError("time_evolve needs a finite time, got %r" % (t,))
    if not torch.is_tensor(psi) or psi.dim() not in (1, 2):
        raise ValueError("time_evolve expects a tensor of shape (n,) or (n, R)")
    if t == 0:
        _as_block(op, psi.reshape(psi.shape[0], -1), "time_evolve")
        return psi.detach().to(torch.complex128).clone()
    if bounds is None:
        bounds = spectral_bounds(op)
    centre, h = _check_bounds(bounds)
    psi = psi.detach()
    vector = psi.dim() == 1
    block = psi.reshape(psi.shape[0], -1)
    R = block.shape[1]
    if block.is_complex():
        block = torch.cat([block.real, block.imag], dim=1)
    C, S = chebyshev_apply(op, block, _evolution_rows(t, centre, h, float(tol)), bounds)
    if block.shape[1] == R:
        out = torch.complex(C, -S)
    else:
        out = torch.complex(C[:, :R] + S[:, R:], C[:, R:] - S[:, :R])
    return out[:, 0] if vector else out
