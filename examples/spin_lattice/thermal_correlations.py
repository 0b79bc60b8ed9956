"""Spin correlations of the Heisenberg ring at finite temperature (docs/design/31-chebyshev-propagator.md):

    H = J1 sum_i s_i . s_{i+1},   s = (X, Y, Z) Pauli matrices, periodic, L sites

from canonical thermal pure quantum states: in every magnetisation sector R random vectors are propagated in imaginary time,
|beta, r> = e^{-beta H / 2} |r>, by a Chebyshev expansion of the exponential -- one fused kernel launch per order, no stored
basis -- and <A>_beta is the weighted mean of <beta, r| A |beta, r>; small sectors are summed exactly over their spectrum.

THE PAULI CONVENTION: s = 2 S, so <S_i . S_j> = <s_i . s_j> / 4 = (xy_ij + zz_ij) / 4.  Printed per temperature:

    the nearest-neighbour <S_i . S_{i+1}> (mean over the ring; -> 0 as T -> infinity, -> E0 / (4 J1 L) as T -> 0) and
    S(q = pi) = (1 / L) sum_ij (-1)^(i - j) <S_i . S_j> through ``ring_structure_factor``, beside its T -> infinity value 3 / 4.

    python examples/spin_lattice/thermal_correlations.py [--L 16] [--R 8] [--seed 0] [--dense-below 256] [--device cuda]

The operators are device operators: the example needs a GPU.  The sampled sectors carry the sampling error of R vectors.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

F64 = torch.float64


def main(argv=None, L=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=16, help="ring length (even, so that q = pi is a momentum of the ring)")
    ap.add_argument("--J1", type=float, default=1.0)
    ap.add_argument("--R", type=int, default=8, help="random vectors per sampled sector")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dense-below", type=int, default=256, help="sectors of at most this dimension are summed exactly")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args([] if argv is None and L is not None else argv)
    if L is not None:
        args.L = L
    from dominantsparseeigenad_amd.operators import ring_bonds, ring_structure_factor
    from dominantsparseeigenad_amd.thermal import thermal_correlations
    L, J1 = args.L, args.J1
    if L < 4 or L % 2:
        raise SystemExit("--L must be even and at least 4")
    bonds = ring_bonds(L)
    couplings = torch.tensor([J1] * L + [J1] * L + [0.0] * L, dtype=F64)
    T = torch.tensor([64.0, 16.0, 4.0, 2.0, 1.0, 0.5, 0.25], dtype=F64) * abs(J1)          # (descending: beta ascends)
    out = thermal_correlations(L, bonds, couplings, 1.0 / T, R=args.R, seed=args.seed, dense_below=args.dense_below,
                               device=args.device)
    SS = (out.xy + out.zz) / 4.0                                                       # <S_i . S_j>, diagonal 3 / 4
    nn = torch.stack([SS[b][torch.arange(L), (torch.arange(L) + 1) % L].mean() for b in range(T.numel())])
    Spi = torch.stack([ring_structure_factor(SS[b])[L // 2] for b in range(T.numel())])
    print("L = %d  J1 = %.3f  R = %d" % (L, J1, args.R))
    print("      T     <S_i.S_i+1>   E/(4 J1 L)      S(pi)    S(pi, T = inf)")
    for b in range(T.numel()):
        print("  %7.3f  %11.6f  %11.6f  %10.6f  %10.6f" % (T[b], nn[b], out.energy[b] / (4.0 * J1 * L), Spi[b], 0.75))
    return {"L": L, "T": T.tolist(), "nn": nn.tolist(), "energy": out.energy.tolist(), "S_pi": Spi.tolist(), "S_pi_limit": 0.75,
            "logZ": out.logZ.tolist()}


if __name__ == "__main__":
    main()
