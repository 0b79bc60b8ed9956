"""Specific heat and uniform susceptibility of the Heisenberg ring at finite temperature (docs/design/27-finite-temperature.md):

    H = J1 sum_i s_i . s_{i+1},   s = (X, Y, Z) Pauli matrices, periodic, L sites

by the finite-temperature Lanczos method: every magnetisation sector contributes a trace measure -- exact (all eigenvalues)
where the sector is small, R random vectors through k basis-free Lanczos steps as one block where it is not -- and
``ThermalEnsemble`` turns the measures into ln Z, E, C, S and chi on a grid of temperatures.

THE PAULI CONVENTION: s = 2 S, so this is J sum S_i . S_{i+1} with J = 4 J1, and the magnetisation m = L / 2 - ndown is S^z_total.
The high-temperature limits printed beside the numbers follow from tr H^2 / 2^L = 3 J1^2 L and tr (S^z)^2 / 2^L = L / 4:

    C / L -> beta^2 3 J1^2          chi / L -> beta / 4          (beta -> 0)

    python examples/spin_lattice/thermodynamics.py [--L 16] [--R 8] [--k 100] [--seed 0] [--dense-below 256] [--device cuda]

The operators are device operators: the example needs a GPU.  The stochastic sectors carry the sampling error of R vectors.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

F64 = torch.float64


def main(argv=None, L=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=16, help="ring length")
    ap.add_argument("--J1", type=float, default=1.0)
    ap.add_argument("--R", type=int, default=8, help="random vectors per stochastic sector")
    ap.add_argument("--k", type=int, default=100, help="Lanczos steps per vector")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dense-below", type=int, default=256, help="sectors of at most this dimension are diagonalised exactly")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args([] if argv is None and L is not None else argv)
    if L is not None:
        args.L = L
    from dominantsparseeigenad_amd.operators import ring_bonds
    from dominantsparseeigenad_amd.thermal import spin_thermodynamics
    L, J1 = args.L, args.J1
    if L < 3:
        raise SystemExit("--L must be at least 3")
    bonds = ring_bonds(L)
    couplings = torch.tensor([J1] * L + [J1] * L + [0.0] * L, dtype=F64)
    ens = spin_thermodynamics(L, bonds, couplings, R=args.R, k=args.k, seed=args.seed, dense_below=args.dense_below,
                              device=args.device)
    T = torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0], dtype=F64) * J1
    beta = 1.0 / T
    C, chi, S = ens.specific_heat(beta) / L, ens.susceptibility(beta) / L, ens.entropy(beta) / L
    c_limit, chi_limit = beta ** 2 * 3.0 * J1 ** 2, beta / 4.0
    print("L = %d  J1 = %.3f  %d poles in %d sectors   tr 1 = %.6g (2^L = %d)   tr H^2 / 2^L = %.8f (3 J1^2 L = %.8f)"
          % (L, J1, ens.poles.numel(), len(ens.entries), ens.moment(0), 2 ** L, ens.moment(2) / 2 ** L, 3.0 * J1 ** 2 * L))
    print("      T       C/L      beta^2 3 J1^2      chi/L      beta/4        S/L")
    for i in range(T.numel()):
        print("  %7.3f  %10.6f  %10.6f    %10.6f  %10.6f  %10.6f" % (T[i], C[i], c_limit[i], chi[i], chi_limit[i], S[i]))
    return {"L": L, "T": T.tolist(), "C": C.tolist(), "chi": chi.tolist(), "S": S.tolist(), "C_limit": c_limit.tolist(),
            "chi_limit": chi_limit.tolist(), "dimension": ens.moment(0), "second_moment": ens.moment(2) / 2 ** L}


if __name__ == "__main__":
    main()
