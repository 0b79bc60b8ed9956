"""Y = f(H) X for a block X without a stored basis, by a Chebyshev expansion (docs/design/31-chebyshev-propagator.md).

With the spectrum of H inside [a, b], centre = (a + b) / 2, h = (b - a) / 2 and s = (H - centre) / h,

    f(H) X ~= sum_{m < M} c_m T_m(s) X,     T_0 X = X,  T_1 X = s X,  T_{m+1} X = 2 s T_m X - T_{m-1} X

a three-term recurrence with no reductions, whose memory (X, two work blocks, one block per function) does not depend on M.
On a ``SpinSectorOperator`` every order is ONE launch of k_cheb_sector_block: the block mat-vec with the recurrence tail inside.

    chebyshev_coefficients(f, M)            c_0 / 2, c_1, ..., c_{M-1} of f on [-1, 1]
    exp_order(x, tol)                       the order that e^{-x (s + 1)} needs
    spectral_bounds(op, k, margin, seed)    (a, b) from a short Lanczos run, inside the rigorous bound where one is known
    chebyshev_apply(op, X, coeffs, bounds)  sum_m c_m T_m(s) X for one or two coefficient rows
    expm_block(op, X, tau)                  (Y, shift) with e^{-tau H} X = e^{-tau shift} Y
    time_evolve(op, psi, t)                 e^{-i H t} psi

Plain host float64 numbers and detached blocks: nothing here is differentiable.
"""
from __future__ import annotations

import math
from ctypes import c_double, c_void_p

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
    """B = sum_t (2 |Jxy_t| + |Jz_t|) + sum_i |hz_i| >= ||H||_2 of a ``SpinSectorOperator``; None for another operator"""
    from .operators import SpinSectorOperator
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

    ``fused=True``: dsea_op_sector_block_chebyshev, one launch per order, ``SpinSectorOperator`` and A in {1, 2} only
    (``ValueError`` otherwise), the columns in pieces of 8, 4, 2 and 1.  ``fused=False``: ``op.apply_block`` and torch
    elementwise operations in exactly the order of the kernel's tail, for any operator with ``apply_block``; the two paths
    return the same bits.  ``None``: fused where the entry exists.  X is detached and not written."""
    from .operators import SpinSectorOperator
    c, single = _check_coeffs(coeffs)
    centre, h = _check_bounds(bounds)
    A, M = c.shape
    can_fuse = isinstance(op, SpinSectorOperator) and A in FUSED_ACCUMULATORS
    if fused is None:
        fused = can_fuse
    if fused and not can_fuse:
        raise ValueError("the fused Chebyshev kernel exists for SpinSectorOperator and 1 or 2 coefficient rows only, got %s and %d"
                         % (type(op).__name__, A))
    if not callable(getattr(op, "apply_block", None)):
        raise ValueError("chebyshev_apply needs an operator with apply_block, got %s" % type(op).__name__)
    X = _as_block(op, X, "chebyshev_apply").to(F64)
    out = _apply_fused(op, X, c, centre, h) if fused else _apply_unfused(op, X, c, centre, h)
    return out[0] if single else out


def _apply_fused(op, X, c, centre, h):
    lib = _lib.load()
    A, M = c.shape
    n, R = X.shape
    host = (c_double * (A * M))(*c.reshape(-1).tolist())
    out = torch.empty((A, n, R), dtype=F64, device=X.device)
    ptr = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    for first, w in block_pieces(R):
        Xp = X[:, first:first + w].contiguous()
        if Xp.data_ptr() % 16:
            Xp = Xp.clone()
        U, V = torch.empty_like(Xp), torch.empty_like(Xp)
        acc = torch.empty((A, n, w), dtype=F64, device=X.device)
        check(lib.dsea_op_sector_block_chebyshev(op.handle, w, A, M, centre, h, host, ptr(Xp), ptr(U), ptr(V), ptr(acc),
                                                 engine._stream(X.device)), "dsea_op_sector_block_chebyshev")
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
    w, phase = LD(h * t), LD(centre * t)
    fc = lambda s: np.cos(w * s + phase)  # noqa: E731
    fs = lambda s: np.sin(w * s + phase)  # noqa: E731
    guess = _order_guess(abs(h * t))
    found = [_truncated_expansion(f, guess, tol) for f in (fc, fs)]
    M = max(m for m, _ in found)
    rows = np.zeros((2, M))                     # (the shorter row is padded: its coefficients beyond its own order are below tol)
    for a, (m, c) in enumerate(found):
        rows[a, :m] = c
    C, S = chebyshev_apply(op, block, rows, bounds)
    if block.shape[1] == R:
        out = torch.complex(C, -S)
    else:
        out = torch.complex(C[:, :R] + S[:, R:], C[:, R:] - S[:, :R])
    return out[:, 0] if vector else out
