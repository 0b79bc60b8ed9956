"""Filling, entropy, specific heat and spin susceptibility of the Hubbard ring at finite temperature
(docs/design/28-hubbard-finite-temperature.md):

    H = -t sum_{i, s} (c+_{i s} c_{i+1 s} + h.c.) + U sum_i n_{i up} n_{i dn},   periodic, L sites

in the grand-canonical ensemble by the finite-temperature Lanczos method: every (N_up, N_dn) sector contributes a trace measure
-- exact (all eigenvalues) where the sector is small or a species is empty or full, R random vectors through k basis-free Lanczos
steps as one block where it is not -- and ``GrandCanonicalEnsemble`` turns the measures into ln Xi, <N>, S, C and chi_s on a grid
of temperatures and chemical potentials.

Printed: n(mu) = <N> / L at two temperatures -- at the lower one the Mott plateau at n = 1 around mu = U / 2 --, and S / L, C / L
(at fixed mu) and chi_s / L against T at mu = U / 2.  Exact statements to compare with: S / L -> ln 4 as T -> infinity, and
<N> = L at mu = U / 2 at every temperature on the bipartite ring (even L), by particle-hole symmetry; where sectors are
stochastic the latter holds up to the sampling error of R vectors.

    python examples/hubbard/thermodynamics.py [--L 8] [--U 4] [--R 8] [--k 100] [--seed 0] [--dense-below 256] [--device cuda]

The operators are device operators: the example needs a GPU.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

F64 = torch.float64


def main(argv=None, L=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=8, help="ring length (even: the ring is then bipartite)")
    ap.add_argument("--t", type=float, default=1.0)
    ap.add_argument("--U", type=float, default=4.0)
    ap.add_argument("--R", type=int, default=8, help="random vectors per stochastic sector")
    ap.add_argument("--k", type=int, default=100, help="Lanczos steps per vector")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dense-below", type=int, default=256, help="sectors of at most this dimension are diagonalised exactly")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args([] if argv is None and L is not None else argv)
    if L is not None:
        args.L = L
    from dominantsparseeigenad_amd.operators import ring_bonds
    from dominantsparseeigenad_amd.thermal import hubbard_thermodynamics
    L, t, U = args.L, args.t, args.U
    if L < 3:
        raise SystemExit("--L must be at least 3")
    bonds = ring_bonds(L)
    couplings = torch.tensor([t] * L + [0.0] * L + [U] * L + [0.0] * L, dtype=F64)
    ens = hubbard_thermodynamics(L, bonds, couplings, R=args.R, k=args.k, seed=args.seed, dense_below=args.dense_below,
                                 device=args.device)
    print("L = %d  t = %.3f  U = %.3f  %d poles in %d sectors   tr 1 = %.6g (4^L = %d)"
          % (L, t, U, ens.poles.numel(), len(ens.entries), ens.moment(0), 4 ** L))
    half = 0.5 * U
    mu = half + torch.linspace(-1.0, 1.0, 9, dtype=F64) * (0.5 * U + 2.0 * t)
    T_n = [0.1 * t, 1.0 * t]
    filling = [ens.density(1.0 / T, mu) / L for T in T_n]
    print("      mu      n(T = %.2f)   n(T = %.2f)" % tuple(T_n))
    for i in range(mu.numel()):
        print("  %7.3f   %10.6f   %10.6f" % (mu[i], filling[0][i], filling[1][i]))
    T = torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0], dtype=F64) * t
    beta = 1.0 / T
    S, C, chi = ens.entropy(beta, half) / L, ens.specific_heat(beta, half) / L, ens.spin_susceptibility(beta, half) / L
    N_half = ens.density(beta, half)
    print("  at mu = U / 2 (ln 4 = %.6f):" % math.log(4.0))
    print("      T        S/L         C/L       chi_s/L       <N>")
    for i in range(T.numel()):
        print("  %7.3f  %10.6f  %10.6f  %10.6f  %12.8f" % (T[i], S[i], C[i], chi[i], N_half[i]))
    print("largest |<N> - L| at mu = U / 2: %.3e" % float((N_half - L).abs().max()))
    return {"L": L, "mu": mu.tolist(), "T_n": T_n, "n": [f.tolist() for f in filling], "T": T.tolist(), "S": S.tolist(),
            "C": C.tolist(), "chi_s": chi.tolist(), "N_half": N_half.tolist(), "dimension": ens.moment(0)}


if __name__ == "__main__":
    main()
