"""Long-range spin models in their S^z = 0 sector, on the all-pair operator (docs/design/22-pair-sector.md).  Every pair of
sites carries a coupling: L (L - 1) / 2 of them, 190 at the default L = 20 -- more than a bond list holds.

  1. The Haldane-Shastry ring
         H = sum_{i<j} J_ij S_i . S_j,   J_ij = (pi / L)^2 / sin^2(pi (i - j) / L),   S = (X, Y, Z) / 2
     i.e. Jxy_ij = Jz_ij = J_ij / 4 in Pauli matrices.  E0 beside the closed form -pi^2 (L + 5 / L) / 24, and the static zz
     structure factor S(k) = (1 / L) sum_ij cos(2 pi k (i - j) / L) <Z_i Z_j> from ``correlations`` of the ground state.
  2. The open power-law XXZ chain Jxy_ij = 1 / |i - j|^alpha, Jz_ij = delta / |i - j|^alpha: dE0/dalpha by autograd through
     ``power_law_couplings`` (one pass of the parameter-adjoint kernels gives all L (L - 1) + L coupling gradients; the chain
     rule of the power law folds them into one number).

    python examples/spin_lattice/long_range.py [--L 20] [--k 100] [--alpha 2.0] [--delta 1.0] [--device cuda]

The operator is a device operator: the example needs a GPU.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

F64 = torch.float64


def haldane_shastry(L, device):
    """the S^z = 0 operator of the Haldane-Shastry ring"""
    from dominantsparseeigenad_amd.operators import SpinSectorPairOperator
    idx = torch.arange(L, dtype=F64, device=device)
    J = (math.pi / L) ** 2 / (4.0 * torch.sin(math.pi * (idx[:, None] - idx[None, :]) / L) ** 2 + torch.eye(L, dtype=F64, device=device))
    op = SpinSectorPairOperator(L, None, L // 2, device)
    op.couplings = op.pack(J, J, 0.0)
    return op


def power_law(L, alpha, delta, device):
    """the S^z = 0 operator of the open power-law XXZ chain; alpha a tensor that may require grad"""
    from dominantsparseeigenad_amd.operators import SpinSectorPairOperator, power_law_couplings
    M = power_law_couplings(L, alpha)
    op = SpinSectorPairOperator(L, None, L // 2, device)
    op.couplings = op.pack(M, delta * M, 0.0)
    return op


def ground_state(op, k):
    import DominantSparseEigenAD.symeig as symeig
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    torch.manual_seed(0)
    return symeig.DominantSparseSymeig.apply(op.couplings, min(k, op.dim), op.dim, op.device)


def power_law_energy(L, alpha, delta=1.0, device="cuda", k=100):
    """E0(alpha) of the open power-law chain as a float"""
    device = torch.device(device)
    op = power_law(L, torch.tensor(float(alpha), dtype=F64, device=device), delta, device)
    return ground_state(op, k)[0].item()


def main(argv=None, L=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=20, help="number of sites (even)")
    ap.add_argument("--k", type=int, default=100, help="Lanczos steps")
    ap.add_argument("--alpha", type=float, default=2.0, help="exponent of the power-law chain")
    ap.add_argument("--delta", type=float, default=1.0, help="Jz / Jxy of the power-law chain")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args([] if argv is None and L is not None else argv)
    if L is not None:
        args.L = L
    import DominantSparseEigenAD.CG as CG
    from dominantsparseeigenad_amd.operators import ring_structure_factor
    CG.EPS_DEFAULT = 1e-12
    device = torch.device(args.device)
    L = args.L
    # 1. Haldane-Shastry: E0 and the structure factor of the ground state
    op = haldane_shastry(L, device)
    E0, psi = ground_state(op, args.k)
    exact = -math.pi ** 2 * (L + 5.0 / L) / 24.0
    print("Haldane-Shastry ring  L = %d  S^z = 0 (n = %d, %d pairs)   E0 = %.12f   closed form %.12f"
          % (L, op.dim, op.npair, E0.item(), exact))
    xy, zz, z = op.correlations(psi)
    S = ring_structure_factor(zz)
    print("  <Z_0 Z_j>, j = 0 .. L/2: " + " ".join("%+.5f" % c for c in zz[0, :L // 2 + 1].tolist()))
    print("  S_zz(k), k = 0 .. L/2:   " + " ".join("%.5f" % s for s in S[:L // 2 + 1].tolist()))
    # 2. the open power-law chain: dE0/dalpha through the couplings
    alpha = torch.tensor(args.alpha, dtype=F64, device=device, requires_grad=True)
    chain = power_law(L, alpha, args.delta, device)
    E0_chain, _ = ground_state(chain, args.k)
    (dE0,) = torch.autograd.grad(E0_chain, alpha)
    print("open power-law XXZ chain  alpha = %.2f  delta = %.2f   E0 = %.12f   dE0/dalpha = %.10f"
          % (args.alpha, args.delta, E0_chain.item(), dE0.item()))
    return {"L": L, "n": op.dim, "pairs": op.npair, "E0_hs": E0.item(), "E0_hs_exact": exact, "zz": zz.detach().cpu(),
            "z": z.detach().cpu(), "xy": xy.detach().cpu(), "S_zz": S.detach().cpu(), "alpha": args.alpha, "delta": args.delta,
            "E0_chain": E0_chain.item(), "dE0_dalpha": dE0.item()}


if __name__ == "__main__":
    main()
