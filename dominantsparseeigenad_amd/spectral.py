"""Zero-temperature spectral functions by the Lanczos continued fraction (docs/design/24-dynamics.md).

    S_O(omega) = sum_n |<n| O |psi0>|^2 delta(omega - (E_n - E_0))

For a vector phi = O psi0 the k-step Lanczos run of H from phi / |phi| gives a k x k tridiagonal matrix T = S diag(theta) S^T,
and the measure sum_j w_j delta(E - theta_j) with w_j = |phi|^2 S_{0j}^2 has the first 2 k moments phi^T H^m phi of the exact
one.  The run is ``engine.lanczos`` on a native operator (full re-orthogonalisation, the kernels of the eigenvalue solvers); the
k x k eigenproblem is solved on the host.

    lanczos_measure(op, phi, k)                                   the measure of phi under the operator ``op``
    SpectralMeasure                                               poles and weights: greens(z), __call__(omega, eta), moment(m)
    dynamical_structure_factor(op0, psi0, E0, weights, channel)   S^{zz}, S^{-}, S^{+} of a sector state through SpinSectorLadder
    hubbard_spectral_function(op0, psi0, E0, weights, channel)    c, c+, charge and spin channels of a Hubbard state (HubbardLadder)
    kpm_measure(op, phi, M), kpm_structure_factor(...)            the same by Chebyshev moments: a ``chebyshev.ChebyshevMeasure``
                                                                  of uniform, chosen resolution (docs/design/33-chebyshev-moments.md)

A ``SpectralMeasure`` holds host float64 tensors and is NOT differentiable: derivatives of poles and weights are out of scope.
Static quantities built on the ladder itself (|sigma^-_q psi0|^2, matrix elements) are differentiable through
``SpinSectorLadder``.
"""
from __future__ import annotations

import math
import warnings

import torch

from . import engine

F64 = torch.float64


class SpectralMeasure:
    """sum_j weights[j] delta(E - poles[j]): ``poles`` and ``weights`` are host float64 tensors of the same length, ``norm2`` =
    |phi|^2 of the vector(s) it was built from (= the sum of the weights up to rounding) and ``steps`` the number of Lanczos
    steps that entered it (fewer than asked for when the Krylov space of phi was exhausted).  The sum of two measures
    concatenates them (``norm2`` and ``steps`` add).  Plain numbers: nothing here is differentiable."""

    def __init__(self, poles, weights, norm2, steps):
        self.poles = torch.as_tensor(poles, dtype=F64).detach().cpu().reshape(-1)
        self.weights = torch.as_tensor(weights, dtype=F64).detach().cpu().reshape(-1)
        if self.poles.numel() != self.weights.numel():
            raise ValueError("poles and weights must have the same length")
        self.norm2 = float(norm2)
        self.steps = int(steps)

    def __len__(self):
        return self.poles.numel()

    def greens(self, z):
        """G(z) = sum_j w_j / (z - theta_j) for a complex tensor (or number) z, on the device of z"""
        z = torch.as_tensor(z).to(torch.complex128)
        poles, weights = self.poles.to(z.device), self.weights.to(z.device)
        return (weights / (z.unsqueeze(-1) - poles)).sum(dim=-1)

    def __call__(self, omega, eta):
        """the Lorentzian-broadened spectral function -Im G(omega + i eta) / pi"""
        omega = torch.as_tensor(omega, dtype=F64)
        return -self.greens(torch.complex(omega, torch.full_like(omega, float(eta)))).imag / math.pi

    def moment(self, m):
        """sum_j w_j theta_j^m as a float"""
        return float((self.weights * self.poles ** int(m)).sum())

    def shifted(self, E0):
        """the same weights at the poles theta - E0"""
        return SpectralMeasure(self.poles - float(E0), self.weights, self.norm2, self.steps)

    def reflected(self):
        """the same weights at the poles -theta: a removal measure in E_n - E0 placed at omega = E0 - E_n"""
        return SpectralMeasure(-self.poles, self.weights, self.norm2, self.steps)

    def __add__(self, other):
        if not isinstance(other, SpectralMeasure):
            return NotImplemented
        return SpectralMeasure(torch.cat([self.poles, other.poles]), torch.cat([self.weights, other.weights]),
                               self.norm2 + other.norm2, self.steps + other.steps)

    def __repr__(self):
        return "SpectralMeasure(%d poles, norm2 = %.6g, steps = %d)" % (len(self), self.norm2, self.steps)


def lanczos_measure(op, phi, k):
    """The spectral measure of the vector ``phi`` under the native symmetric operator ``op`` (``op.handle``, ``op.n``) from
    min(k, n) Lanczos steps with the module defaults of ``engine`` (full re-orthogonalisation).  When the run meets beta ~ 0
    at step s (``engine.last_break``: the Krylov space of phi has dimension s), the tridiagonal matrix is cut there, the
    engine's ``RuntimeWarning`` is not passed on and the measure reports ``steps = s``; its poles are then exact eigenvalues.
    phi = 0 gives the empty measure.  Not differentiable: phi is detached."""
    n = int(op.n)
    phi = phi.detach()
    if phi.dim() != 1 or phi.numel() != n:
        raise ValueError("expected a vector of %d elements, got shape %r" % (n, tuple(phi.shape)))
    k = min(int(k), n)
    if k < 1:
        raise ValueError("lanczos_measure needs k >= 1")
    norm2 = float(torch.dot(phi, phi))
    if not norm2 > 0.0:
        return SpectralMeasure(torch.empty(0, dtype=F64), torch.empty(0, dtype=F64), 0.0, 0)
    q0 = phi / math.sqrt(norm2)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _, _, alphas, betas = engine.lanczos(None, k, n, phi.device, q0, native=op)
        steps = engine.last_break or k
    for w in caught:            # the breakdown is reported as ``steps``; anything else goes on to the caller
        if not (issubclass(w.category, RuntimeWarning) and "Lanczos breakdown" in str(w.message)):
            warnings.warn_explicit(w.message, w.category, w.filename, w.lineno)
    a = alphas[:steps].cpu()
    b = betas[:steps - 1].cpu()
    T = torch.diag(a)
    if steps > 1:
        T = T + torch.diag(b, 1) + torch.diag(b, -1)
    theta, S = torch.linalg.eigh(T)
    return SpectralMeasure(theta, norm2 * S[0] ** 2, norm2, steps)


def _weight_parts(weights):
    """the real site-weight vectors whose measures add up: [c] for a real vector, [re, im] for a (re, im) pair or a complex
    tensor"""
    if torch.is_tensor(weights) and weights.is_complex():
        return [weights.real.to(F64), weights.imag.to(F64)]
    if isinstance(weights, (tuple, list)) and len(weights) == 2 and all(torch.as_tensor(w).dim() == 1 for w in weights):
        return [torch.as_tensor(w, dtype=F64) for w in weights]
    t = torch.as_tensor(weights)
    if t.is_complex():
        return [t.real.to(F64), t.imag.to(F64)]
    return [t.to(F64)]


def _spin_step(channel):
    step = {"zz": 0, "-": 1, "+": -1}.get(channel)
    if step is None:
        raise ValueError("channel must be 'zz', '-' or '+', got %r" % (channel,))
    return step


def _spin_ladder(op0, step, channel, target):
    """(target, ladder) of a spin channel: ``target`` None builds the Hamiltonian of the destination sector from ``op0``"""
    from .operators import SpinSectorLadder, SpinSectorOperator, SpinSectorPairOperator
    if target is None:
        if step == 0:
            target = op0
        else:
            couplings = op0.couplings.detach()
            if hasattr(op0, "bonds"):
                target = SpinSectorOperator(op0.N, op0.bonds, couplings, op0.ndown + step, op0.device)
            else:
                target = SpinSectorPairOperator(op0.N, couplings, op0.ndown + step, op0.device)
    lad = SpinSectorLadder(op0, target)
    if lad.step != step:
        raise ValueError("channel %r needs a target at ndown = %d, got %d" % (channel, op0.ndown + step, target.ndown))
    return target, lad


def dynamical_structure_factor(op0, psi0, E0, weights, channel, k=200, target=None, basis_free=False):
    """The spectral measure of O psi0 as a function of the excitation energy E - E0, for the eigenstate (psi0, E0) of the sector
    operator ``op0`` (``SpinSectorOperator`` or ``SpinSectorPairOperator``) and the site-weighted operator

        channel "zz": O = sum_i c_i Z_i            (stays in the sector; ``target`` = op0)
        channel "-":  O = sum_i c_i sigma^-_i      (lands in ndown + 1)
        channel "+":  O = sum_i c_i sigma^+_i      (lands in ndown - 1)

    in the Pauli convention of the operators (Z = 2 S^z, sigma^+- = S^+-).  ``weights``: a real vector [L], a ``(re, im)``
    pair (``ring_momentum_weights``) or a complex tensor.  For complex weights the result is the sum of the measures of the real
    and of the imaginary part: H is real symmetric, so the cross terms of <a + ib| f(H) |a + ib> cancel.  ``target`` is the
    Hamiltonian of the destination sector; ``None`` builds it from the bonds and couplings of ``op0`` at the new ndown, on new
    tables.  ``k`` Lanczos steps per real vector.  ``basis_free=True`` (bond-list ``SpinSectorOperator`` only): the real and the
    imaginary part run as one block of 1 or 2 columns through ``thermal.block_lanczos_measures`` -- no stored basis, no
    re-orthogonalisation, memory independent of k (docs/design/27-finite-temperature.md).  Plain numbers: not differentiable."""
    from .operators import SpinSectorOperator
    step = _spin_step(channel)
    if basis_free and not (isinstance(op0, SpinSectorOperator) and (target is None or isinstance(target, SpinSectorOperator))):
        raise ValueError("basis_free=True works on the bond-list SpinSectorOperator only")
    target, lad = _spin_ladder(op0, step, channel, target)
    psi0 = psi0.detach()
    if basis_free:
        from .thermal import block_lanczos_measures
        Phi = torch.stack([lad(c, psi0).detach() for c in _weight_parts(weights)], dim=1)
        parts = block_lanczos_measures(target, Phi, k)
        total = parts[0] if len(parts) == 1 else parts[0] + parts[1]
        return total.shifted(float(E0))
    total = None
    for c in _weight_parts(weights):
        part = lanczos_measure(target, lad(c, psi0), k)
        total = part if total is None else total + part
    return total.shifted(float(E0))


_HUBBARD_CHANNELS = {"c_up": ("up", -1), "c_dn": ("dn", -1), "cdag_up": ("up", 1), "cdag_dn": ("dn", 1), "n": (None, 0),
                     "sz": (None, 0)}


def _hubbard_excitation(op0, psi0, channel, target):
    """(target, excited) of a Hubbard channel: ``excited(w)`` is sum_i w_i O_i psi0 in the sector of ``target``; ``target`` None
    builds the Hamiltonian of the destination sector from ``op0``"""
    from .operators import HubbardLadder, HubbardOperator
    if channel not in _HUBBARD_CHANNELS:
        raise ValueError("channel must be one of %s, got %r" % (", ".join(repr(c) for c in _HUBBARD_CHANNELS), channel))
    species, step = _HUBBARD_CHANNELS[channel]
    if target is None:
        if step == 0:
            target = op0
        else:
            nup, ndn = (op0.nup + step, op0.ndn) if species == "up" else (op0.nup, op0.ndn + step)
            target = HubbardOperator(op0.N, op0.bonds, op0.couplings.detach(), nup, ndn, op0.device)
    if step == 0:
        ladders = [HubbardLadder(op0, target, "up"), HubbardLadder(op0, target, "dn")]
        sign = 1.0 if channel == "n" else -1.0
    else:
        ladders = [HubbardLadder(op0, target, species)]
    if ladders[0].step != step:
        raise ValueError("channel %r needs a target with the %s count changed by %d, got (nup, ndn) = (%d, %d)"
                         % (channel, species or "no", step, target.nup, target.ndn))
    psi0 = psi0.detach()

    def excited(w):
        phi = ladders[0](w, psi0)
        return phi + sign * ladders[1](w, psi0) if step == 0 else phi

    return target, excited


def hubbard_spectral_function(op0, psi0, E0, weights, channel, k=200, target=None, basis_free=False):
    """The spectral measure of O psi0 as a function of the excitation energy E - E0, for the eigenstate (psi0, E0) of the
    ``HubbardOperator`` ``op0`` and the site-weighted operator (docs/design/25-hubbard-ladder.md)

        channel "c_up", "c_dn":        O = sum_i w_i c_{i s}        (photoemission; lands in the sector with one s particle less)
        channel "cdag_up", "cdag_dn":  O = sum_i w_i c+_{i s}       (inverse photoemission; one s particle more)
        channel "n":                   O = sum_i w_i (n_{i up} + n_{i dn})     (charge; stays in the sector, ``target`` = op0)
        channel "sz":                  O = sum_i w_i (n_{i up} - n_{i dn})     (2 S^z; stays in the sector)

    ``weights``: a real vector [L], a ``(re, im)`` pair (``ring_momentum_weights``) or a complex tensor.  For complex weights
    the result is the sum of the measures of the real and of the imaginary part: H is real symmetric, so the cross terms of
    <a + ib| f(H) |a + ib> cancel.  ``target`` is the Hamiltonian of the destination sector; ``None`` builds it from the bonds
    and couplings of ``op0`` at the new particle numbers, on new tables.  ``k`` Lanczos steps per real vector.  A removal
    measure comes out in E_n - E0 >= 0 like every other; ``reflected()`` places it at omega = E0 - E_n, so that
    ``cdag + c.reflected()`` is the one-particle spectral function A(omega).  ``basis_free=True``: the real and the imaginary
    part run as one block of 1 or 2 columns through ``thermal.block_lanczos_measures`` -- no stored basis, no
    re-orthogonalisation, memory independent of k (docs/design/28-hubbard-finite-temperature.md).  Plain numbers: not
    differentiable."""
    target, excited = _hubbard_excitation(op0, psi0, channel, target)
    if basis_free:
        from .thermal import block_lanczos_measures
        Phi = torch.stack([excited(w).detach() for w in _weight_parts(weights)], dim=1)
        parts = block_lanczos_measures(target, Phi, k)
        total = parts[0] if len(parts) == 1 else parts[0] + parts[1]
        return total.shifted(float(E0))
    total = None
    for w in _weight_parts(weights):
        part = lanczos_measure(target, excited(w), k)
        total = part if total is None else total + part
    return total.shifted(float(E0))


_HUBBARD_PAIR_CHANNELS = {"pair_add": ((1, 1), "up_left"), "pair_remove": ((-1, -1), "dn_left"), "s_plus": ((1, -1), "up_left"),
                          "s_minus": ((-1, 1), "dn_left")}


def _pair_weight_parts(weights):
    """the real pair weights whose measures add up, each a matrix (L, L) or a vector (L,) (its diagonal): [W] for real weights,
    [re, im] for a (re, im) pair or a complex tensor"""
    if isinstance(weights, (tuple, list)) and len(weights) == 2 and all(torch.is_tensor(w) and w.dim() >= 1 for w in weights):
        return [w.to(F64) for w in weights]
    t = torch.as_tensor(weights)
    if t.is_complex():
        return [t.real.to(F64), t.imag.to(F64)]
    return [t.to(F64)]


def hubbard_pair_spectral_function(op0, psi0, E0, weights, channel, k=200, target=None, basis_free=False):
    """The spectral measure of O psi0 as a function of the excitation energy E - E0, for the eigenstate (psi0, E0) of the
    ``HubbardOperator`` ``op0`` and an operator that moves one particle of each species (``HubbardPairLadder``,
    docs/design/41-hubbard-pair-ladder.md)

        channel "pair_add":     O = Delta+(W) = sum_ij W_ij c+_{i up} c+_{j dn}     (lands in (nup + 1, ndn + 1))
        channel "pair_remove":  O = Delta(W)  = sum_ij W_ij c_{j dn} c_{i up}       (lands in (nup - 1, ndn - 1))
        channel "s_plus":       O = sum_ij W_ij c+_{i up} c_{j dn}                  (S^+(q) for diagonal W; (nup + 1, ndn - 1))
        channel "s_minus":      O = sum_ij W_ij c+_{j dn} c_{i up}                  (its transpose; (nup - 1, ndn + 1))

    ``weights``: a real matrix (L, L), a real vector (L,) for a diagonal one (``ring_momentum_weights``), a ``(re, im)`` pair of
    either, or a complex tensor.  For complex weights the result is the sum of the measures of the real and of the imaginary
    part: H is real symmetric, so the cross terms cancel.  ``target`` is the Hamiltonian of the destination sector; ``None``
    builds it from the bonds and couplings of ``op0`` at the new particle numbers, on new tables.  ``k`` Lanczos steps per real
    vector; ``basis_free=True`` runs the parts as one block through ``thermal.block_lanczos_measures``.  Plain numbers: not
    differentiable."""
    from .operators import HubbardOperator, HubbardPairLadder
    if channel not in _HUBBARD_PAIR_CHANNELS:
        raise ValueError("channel must be one of %s, got %r" % (", ".join(repr(c) for c in _HUBBARD_PAIR_CHANNELS), channel))
    (su, sd), order = _HUBBARD_PAIR_CHANNELS[channel]
    if target is None:
        target = HubbardOperator(op0.N, op0.bonds, op0.couplings.detach(), op0.nup + su, op0.ndn + sd, op0.device)
    lad = HubbardPairLadder(op0, target, order)
    if lad.steps != (su, sd):
        raise ValueError("channel %r needs a target at (nup, ndn) = (%d, %d), got (%d, %d)"
                         % (channel, op0.nup + su, op0.ndn + sd, target.nup, target.ndn))
    psi0 = psi0.detach()
    parts = [lad(W, psi0).detach() for W in _pair_weight_parts(weights)]
    if basis_free:
        from .thermal import block_lanczos_measures
        measures = block_lanczos_measures(target, torch.stack(parts, dim=1), k)
    else:
        measures = [lanczos_measure(target, phi, k) for phi in parts]
    total = measures[0] if len(measures) == 1 else measures[0] + measures[1]
    return total.shifted(float(E0))


def kpm_measure(op, phi, M, bounds=None):
    """The ``chebyshev.ChebyshevMeasure`` of the vector ``phi`` under ``op``: its M moments mu_m = <phi| T_m((H - centre) / h)
    |phi> from ceil(M / 2) mat-vecs without a basis (``chebyshev.chebyshev_moments``; docs/design/33-chebyshev-moments.md), the
    counterpart of ``lanczos_measure`` with a resolution pi h / M that is the same all over ``bounds`` = (a, b).  ``bounds`` must
    hold the spectrum; None takes ``chebyshev.spectral_bounds(op)``.  Not differentiable: phi is detached."""
    from .chebyshev import ChebyshevMeasure, chebyshev_moments, spectral_bounds
    if not torch.is_tensor(phi) or phi.dim() != 1 or phi.numel() != int(op.n):
        raise ValueError("expected a vector of %d elements, got %r"
                         % (int(op.n), tuple(phi.shape) if torch.is_tensor(phi) else type(phi).__name__))
    if bounds is None:
        bounds = spectral_bounds(op)
    return ChebyshevMeasure(chebyshev_moments(op, phi.detach().reshape(-1, 1), M, bounds)[:, 0], bounds)


def kpm_structure_factor(op0, psi0, E0, weights, channel, M=256, target=None, bounds=None):
    """``dynamical_structure_factor`` by the kernel polynomial method: the ``chebyshev.ChebyshevMeasure`` of O psi0 as a function
    of omega = E - E0, from one ladder application and ONE moments run in the destination sector (the real and the imaginary
    part of complex weights are the two columns of one block, and their moments add).  ``op0`` a ``SpinSectorOperator`` with
    the channels "zz", "-", "+", or a ``HubbardOperator`` with the channel names of ``hubbard_spectral_function``; either way
    the moments run on the operator's fused kernel.  ``bounds`` of the TARGET's spectrum; None takes
    ``chebyshev.spectral_bounds(target)``.  Plain numbers: not differentiable."""
    from .chebyshev import ChebyshevMeasure, chebyshev_moments, spectral_bounds
    from .operators import HubbardOperator
    if isinstance(op0, HubbardOperator):
        target, excited = _hubbard_excitation(op0, psi0, channel, target)
    else:
        target, lad = _spin_ladder(op0, _spin_step(channel), channel, target)
        psi0 = psi0.detach()
        excited = lambda c: lad(c, psi0)  # noqa: E731
    Phi = torch.stack([excited(w).detach() for w in _weight_parts(weights)], dim=1)
    if bounds is None:
        bounds = spectral_bounds(target)
    return ChebyshevMeasure(chebyshev_moments(target, Phi, M, bounds).sum(dim=1), bounds).shifted(float(E0))


class OpticalResponse:
    """What ``optical_conductivity`` returns: plain host numbers, not differentiable (docs/design/39-hubbard-current.md).

        measure          the ``SpectralMeasure`` of K(w) psi0 in omega = E_n - E0: sum_j w_j delta(omega - theta_j)
        diamagnetic      K_d = sum_t t_t d_t^2 <c+_a c_b + h.c.>_t summed over the species
        inverse_moment   I_-1 = sum_{theta_j > floor} w_j / theta_j
        dropped_weight   the weight of the poles at or below ``floor``, which I_-1 leaves out (a degenerate ground level, or
                         a current that does not leave the ground state)
        stiffness        K_d - 2 I_-1 = d^2 E0 / d phi^2 under the Peierls twist t_t -> t_t exp(i phi d_t)

    Convention (no volume factor, e = hbar = 1): sigma(omega) = pi stiffness delta(omega) + sigma_reg(omega) on the whole axis,
    so the Drude weight in the usual convention is pi * stiffness, and

        sigma_reg(omega) = pi sum_j (w_j / theta_j) delta(omega - theta_j)        for omega > 0,

    ``regular(omega, eta)`` with every delta a Lorentzian of half width eta.  Then int_0^inf sigma_reg = pi I_-1 and the f-sum
    rule reads  pi stiffness / 2 + pi I_-1 = pi K_d / 2  (``f_sum()`` returns the two sides)."""

    def __init__(self, measure, diamagnetic, floor=1e-9):
        self.measure = measure
        self.diamagnetic = float(diamagnetic)
        self.floor = float(floor)
        keep = measure.poles > self.floor
        self._poles = measure.poles[keep]
        self._strengths = measure.weights[keep] / self._poles
        self.inverse_moment = float(self._strengths.sum())
        self.dropped_weight = float(measure.weights[~keep].sum())
        self.stiffness = self.diamagnetic - 2.0 * self.inverse_moment

    def regular(self, omega, eta):
        """sigma_reg(omega) = pi sum_j (w_j / theta_j) eta / (pi ((omega - theta_j)^2 + eta^2)) over the poles above the floor,
        for a real tensor (or number) omega; a host float64 tensor of the shape of omega"""
        omega = torch.as_tensor(omega, dtype=F64).detach().cpu()
        eta = float(eta)
        if not eta > 0.0:
            raise ValueError("regular needs eta > 0, got %r" % eta)
        diff = omega.unsqueeze(-1) - self._poles
        return (self._strengths * eta / (diff * diff + eta * eta)).sum(dim=-1)

    def f_sum(self):
        """(pi stiffness / 2 + pi I_-1, pi K_d / 2): the two sides of the f-sum rule"""
        return math.pi * self.stiffness / 2.0 + math.pi * self.inverse_moment, math.pi * self.diamagnetic / 2.0

    def __repr__(self):
        return ("OpticalResponse(K_d = %.10g, I_-1 = %.10g, stiffness = %.10g, dropped_weight = %.3g, %d poles)"
                % (self.diamagnetic, self.inverse_moment, self.stiffness, self.dropped_weight, len(self.measure)))


def optical_conductivity(op0, psi0, E0, displacements, kind="charge", k=200, basis_free=False, floor=1e-9):
    """The optical response of the eigenstate (psi0, E0) of the ``HubbardOperator`` ``op0`` to a uniform field, as an
    ``OpticalResponse`` (docs/design/39-hubbard-current.md): the regular part of sigma(omega), its f-sum rule and Kohn's
    stiffness from ONE application of the bond current map (``HubbardCurrent``), one Lanczos measure in the same sector and the
    bond kinetic energies of ``op0.Hadjoint_to_couplingsadjoint``.

    ``displacements``: a real (nb,) vector d_t, the projection of r_b - r_a of bond t = (a, b) of ``op0.bonds`` on the field
    direction.  On a periodic cluster it must be the MINIMUM IMAGE (the bond (L - 1, 0) of a ring has d = +1, not 1 - L): that
    is the caller's duty, the function cannot know the geometry.  The current weights are w[s, t] = t_t d_t for
    ``kind="charge"`` and w[up] = t_t d_t, w[dn] = -t_t d_t for ``kind="spin"``, with the hoppings t_t read from
    ``op0.couplings``; the paramagnetic current is J = i K(w) and the measure is that of K(w) psi0, ``k`` Lanczos steps
    (``lanczos_measure``), or the basis-free recurrence of ``thermal.block_lanczos_measures`` with ``basis_free=True``.  Poles at
    or below ``floor`` are left out of the inverse moment and reported as ``dropped_weight``: with a degenerate ground level
    the stiffness of this formula is not defined.  Plain numbers: not differentiable."""
    from .operators import HubbardCurrent, HubbardOperator
    if not isinstance(op0, HubbardOperator):
        raise ValueError("optical_conductivity works on a HubbardOperator, got %s" % type(op0).__name__)
    if kind not in ("charge", "spin"):
        raise ValueError("kind must be 'charge' or 'spin', got %r" % (kind,))
    d = torch.as_tensor(displacements)
    if d.is_complex() or d.dim() != 1 or d.numel() != op0.nb:
        raise ValueError("displacements must be a real vector of %d elements (one per bond), got shape %r"
                         % (op0.nb, tuple(d.shape)))
    d = d.detach().to(device=op0.device, dtype=F64)
    psi0 = psi0.detach()
    hop = op0.couplings.detach()[:op0.nb]
    wt = hop * d
    cur = HubbardCurrent(op0)
    phi = cur(torch.stack([wt, wt if kind == "charge" else -wt]), psi0).detach()
    if basis_free:
        from .thermal import block_lanczos_measures
        measure = block_lanczos_measures(op0, phi.reshape(-1, 1), k)[0]
    else:
        measure = lanczos_measure(op0, phi, k)
    kinetic = op0.Hadjoint_to_couplingsadjoint(psi0, psi0).detach()[:op0.nb]       # dE0/dt_t = -<c+_a c_b + h.c.>
    diamagnetic = -float((hop * d * d * kinetic).sum())
    return OpticalResponse(measure.shifted(float(E0)), diamagnetic, floor)
