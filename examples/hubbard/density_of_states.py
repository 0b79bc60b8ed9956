"""Density of states of the Hubbard ring at fixed filling by the kernel polynomial method (docs/design/34-hubbard-chebyshev.md):

    H = -t sum_{i, s} (c+_{i s} c_{i+1 s} + h.c.) + U sum_i n_{i up} n_{i dn},   periodic, L sites, nup up and ndn down fermions

The Chebyshev moments mu_m = tr T_m(H / B) of the sector are taken on the interval (-B, B), B = 2 t L + U L >= ||H|| from the
couplings alone: exact where the sector is small, R random vectors through ceil(M / 2) orders of the fused Hubbard moments kernel
where it is not.  rho(E) is the Jackson-damped density, with the resolution pi B / M all over the band; its integral on the
Chebyshev-Gauss nodes is mu_0 = n, the dimension of the sector.

    python examples/hubbard/density_of_states.py [--L 8] [--nup 4] [--ndn 4] [--U 4] [--moments 128] [--R 8] [--seed 0]
                                                 [--dense-below 256] [--device cuda]

The operator is a device operator: the example needs a GPU.  A sampled sector carries the sampling error of R vectors.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

F64 = torch.float64


def main(argv=None, L=None, nup=None, ndn=None, moments=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=8, help="ring length")
    ap.add_argument("--nup", type=int, default=4)
    ap.add_argument("--ndn", type=int, default=4)
    ap.add_argument("--t", type=float, default=1.0)
    ap.add_argument("--U", type=float, default=4.0)
    ap.add_argument("--moments", type=int, default=128, help="Chebyshev moments M")
    ap.add_argument("--R", type=int, default=8, help="random vectors of a sampled sector")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dense-below", type=int, default=256, help="a sector of at most this dimension is diagonalised exactly")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args([] if argv is None and L is not None else argv)
    for name, value in (("L", L), ("nup", nup), ("ndn", ndn), ("moments", moments)):
        if value is not None:
            setattr(args, name, value)
    from dominantsparseeigenad_amd.chebyshev import coupling_bound
    from dominantsparseeigenad_amd.operators import HubbardOperator, ring_bonds
    from dominantsparseeigenad_amd.thermal import sector_density_of_states
    L, M = args.L, args.moments
    bonds = ring_bonds(L)
    couplings = torch.tensor([args.t] * L + [0.0] * L + [args.U] * L + [0.0] * L, dtype=F64)
    op = HubbardOperator(L, bonds, couplings.to(args.device), args.nup, args.ndn, args.device)
    B = coupling_bound(op)
    dos = sector_density_of_states(op, M, (-B, B), R=args.R, seed=args.seed, dense_below=args.dense_below)
    n = int(op.n)
    N = 2 * M                                        # Chebyshev-Gauss nodes: the integral of the damped density is exact on them
    s = torch.cos(math.pi * (torch.arange(N, dtype=F64) + 0.5) / N)
    integral = float((math.pi / N) * (dos.density(B * s) * B * torch.sqrt(1.0 - s * s)).sum())
    print("L = %d  (nup, ndn) = (%d, %d)  t = %.3f  U = %.3f  M = %d moments on (-B, B), B = %.4f" % (L, args.nup, args.ndn, args.t,
                                                                                                   args.U, M, B))
    print("n = %d   mu_0 = %.6f   integral of rho = %.6f" % (n, float(dos.moments[0]), integral))
    E = torch.linspace(-0.6 * B, 0.9 * B, 16, dtype=F64)
    print("      E       rho(E) / n")
    for e, r in zip(E.tolist(), (dos.density(E) / n).tolist()):
        print("  %8.3f   %10.6f" % (e, r))
    return {"L": L, "n": n, "M": M, "B": B, "integral": integral, "mu0": float(dos.moments[0])}


if __name__ == "__main__":
    main()
