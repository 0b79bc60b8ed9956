"""Density of states and a dynamical structure factor of the Heisenberg ring by the kernel polynomial method
(docs/design/33-chebyshev-moments.md):

    H = J1 sum_i s_i . s_{i+1},   s = (X, Y, Z) Pauli matrices, periodic, L sites

The Chebyshev moments mu_m = tr T_m(H / B) of every magnetisation sector are summed on ONE interval (-B, B), B = 3 J1 L >= ||H||:
exact where the sector is small, R random vectors through ceil(M / 2) orders of the fused moments kernel where it is not.  From
the same moments come

    rho(E) / 2^L             the density of states, Jackson-damped: resolution pi B / M all over the band
    ln Z(beta)               sum_m c_m(beta) mu_m, beside the finite-temperature Lanczos ensemble of ``spin_thermodynamics``
    S^{zz}(q = pi, omega)    of the ground state: ``kpm_structure_factor`` beside the Lanczos poles of
                             ``dynamical_structure_factor`` broadened by the same amount

    python examples/spin_lattice/density_of_states.py [--L 16] [--moments 256] [--R 8] [--seed 0] [--dense-below 256] [--device cuda]

The operators are device operators: the example needs a GPU.  The stochastic sectors carry the sampling error of R vectors.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

F64 = torch.float64


def main(argv=None, L=None, moments=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=16, help="ring length (even)")
    ap.add_argument("--J1", type=float, default=1.0)
    ap.add_argument("--moments", type=int, default=256, help="Chebyshev moments M")
    ap.add_argument("--R", type=int, default=8, help="random vectors per stochastic sector")
    ap.add_argument("--k", type=int, default=100, help="Lanczos steps of the runs shown for comparison")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dense-below", type=int, default=256, help="sectors of at most this dimension are diagonalised exactly")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args([] if argv is None and L is not None else argv)
    if L is not None:
        args.L = L
    if moments is not None:
        args.moments = moments
    import DominantSparseEigenAD.symeig as symeig
    from dominantsparseeigenad_amd.operators import SpinSectorOperator, ring_bonds, ring_momentum_weights
    from dominantsparseeigenad_amd.spectral import dynamical_structure_factor, kpm_structure_factor
    from dominantsparseeigenad_amd.thermal import spin_density_of_states, spin_thermodynamics
    L, J1, M = args.L, args.J1, args.moments
    if L < 4 or L % 2:
        raise SystemExit("--L must be even and at least 4")
    bonds = ring_bonds(L)
    couplings = torch.tensor([J1] * L + [J1] * L + [0.0] * L, dtype=F64)
    common = dict(R=args.R, seed=args.seed, dense_below=args.dense_below, device=args.device)

    dos = spin_density_of_states(L, bonds, couplings, M, **common)
    B = dos.bounds[1]
    N = 2 * M                                        # Chebyshev-Gauss nodes: the integral of the damped density is exact on them
    s = torch.cos(math.pi * (torch.arange(N, dtype=F64) + 0.5) / N)
    rho = dos.density(B * s) / 2 ** L
    integral = float((math.pi / N) * (rho * B * torch.sqrt(1.0 - s * s)).sum())
    print("L = %d  J1 = %.3f  M = %d moments on (-B, B), B = %.4f   mu_0 = %.6f (2^L = %d)" % (L, J1, M, B, float(dos.moments[0]), 2 ** L))
    print("integral of rho = %.12f" % integral)
    E = torch.linspace(-0.95 * B, 0.95 * B, 13, dtype=F64)
    print("      E       rho(E) / 2^L")
    for e, r in zip(E.tolist(), (dos.density(E) / 2 ** L).tolist()):
        print("  %8.3f   %10.6f" % (e, r))

    ens = spin_thermodynamics(L, bonds, couplings, k=args.k, **common)
    betas = [0.05, 0.1, 0.25, 0.5]
    logZ_kpm = [dos.logtrace_exp(beta / J1) for beta in betas]
    logZ_ftlm = ens.logZ(torch.tensor(betas, dtype=F64) / J1).tolist()
    print("   beta J1    ln Z (moments)    ln Z (Lanczos ensemble)")
    for beta, a, b in zip(betas, logZ_kpm, logZ_ftlm):
        print("  %7.3f   %14.8f   %14.8f" % (beta, a, b))

    op = SpinSectorOperator(L, bonds, couplings.to(args.device), L // 2, args.device)
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    torch.manual_seed(0)
    E0, psi0 = symeig.DominantSparseSymeig.apply(op.couplings, min(200, op.dim), op.dim, op.device)
    E0, psi0 = E0.item(), psi0.detach()
    weights = ring_momentum_weights(L, L // 2)
    kpm = kpm_structure_factor(op, psi0, E0, weights, "zz", M=M)
    poles = dynamical_structure_factor(op, psi0, E0, weights, "zz", k=args.k)
    width = math.pi * 0.5 * (kpm.bounds[1] - kpm.bounds[0]) / M          # the resolution of M Jackson-damped moments
    omega = torch.linspace(0.0, 8.0 * J1, 9, dtype=F64)
    print("S^zz(q = pi, omega), E0 = %.8f, |Z_q psi0|^2 = %.6f (moments) %.6f (Lanczos); resolution %.3f"
          % (E0, float(kpm.moments[0]), poles.norm2, width))
    print("    omega      moments      Lanczos poles, Lorentzian of the same width")
    for w, a, b in zip(omega.tolist(), kpm.density(omega).tolist(), poles(omega, width).tolist()):
        print("  %7.3f   %10.6f   %10.6f" % (w, a, b))
    return {"L": L, "M": M, "B": B, "integral": integral, "mu0": float(dos.moments[0]), "logZ_moments": logZ_kpm,
            "logZ_lanczos": logZ_ftlm, "E0": E0, "norm2_moments": float(kpm.moments[0]), "norm2_lanczos": poles.norm2}


if __name__ == "__main__":
    main()
