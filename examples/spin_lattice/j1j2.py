"""The J1-J2 Heisenberg ring on the bond-list operator (docs/design/16-spin-lattice.md):

    H = J1 sum_i s_i . s_{i+1} + J2 sum_i s_i . s_{i+2},   s = (X, Y, Z) Pauli matrices, periodic, L sites

as ``SpinLatticeOperator(L, ring_bonds(L, 1) + ring_bonds(L, 2), couplings)`` -- the second-neighbour bonds are what the
nearest-neighbour chain operator cannot hold.

  1. E0 and the gap E1 - E0 over a few values of J2 / J1 (DominantSparseSymeig, LowestSparseSymeig);
  2. dE0/dJ2 by autograd through the couplings (one pass of the parameter-adjoint kernel gives all 6 L + 2 L coupling
     gradients; the chain rule of ``couplings = J1 * d1 + J2 * d2`` folds them into one number);
  3. the Majumdar-Ghosh point J2 = J1 / 2, where the ground state is a product of singlets and E0 = -1.5 J1 L exactly.

    python examples/spin_lattice/j1j2.py [--L 12] [--k 200] [--device cuda]

The operator is a device operator: the example needs a GPU.  The first excited level of the Heisenberg ring is a triplet, so
the two-level Lanczos run warns that Ritz values 1 and 2 are degenerate: the gap itself (forward only here) is not affected.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

F64 = torch.float64


def directions(L, device):
    """(bonds, d1, d2): couplings = J1 * d1 + J2 * d2 is the Heisenberg J1-J2 ring (Jx = Jy = Jz on every bond, no fields)"""
    from dominantsparseeigenad_amd.operators import ring_bonds
    bonds = ring_bonds(L, 1) + ring_bonds(L, 2)
    near = torch.cat([torch.ones(L, dtype=F64), torch.zeros(L, dtype=F64)])
    nxt = torch.cat([torch.zeros(L, dtype=F64), torch.ones(L, dtype=F64)])
    fields = torch.zeros(2 * L, dtype=F64)
    d1 = torch.cat([near, near, near, fields]).to(device)
    d2 = torch.cat([nxt, nxt, nxt, fields]).to(device)
    return bonds, d1, d2


def model(L, J2, device, J1=1.0):
    """the operator at (J1, J2), with J2 a tensor that may require grad"""
    from dominantsparseeigenad_amd.operators import SpinLatticeOperator
    bonds, d1, d2 = directions(L, device)
    return SpinLatticeOperator(L, bonds, (J1 * d1 + J2 * d2).contiguous(), device)


def ground_energy(op, k):
    import DominantSparseEigenAD.symeig as symeig
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    torch.manual_seed(0)
    E0, _ = symeig.DominantSparseSymeig.apply(op.couplings, k, op.dim, op.device)
    return E0


def energy(L, J2, device="cuda", k=200):
    """E0(J2) at J1 = 1 as a float"""
    device = torch.device(device)
    return ground_energy(model(L, torch.tensor(float(J2), dtype=F64, device=device), device), min(k, 1 << L)).item()


def gap(op, k):
    import DominantSparseEigenAD.symeig as symeig
    symeig.setLowestSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    torch.manual_seed(0)
    vals, _ = symeig.LowestSparseSymeig.apply(op.couplings, k, op.dim, 2, op.device)
    return (vals[1] - vals[0]).item()


def main(argv=None, L=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=12, help="ring length (even)")
    ap.add_argument("--k", type=int, default=200, help="Lanczos steps")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args([] if argv is None and L is not None else argv)
    if L is not None:
        args.L = L
    import DominantSparseEigenAD.CG as CG
    CG.EPS_DEFAULT = 1e-12
    device = torch.device(args.device)
    L, k = args.L, min(args.k, 1 << args.L)
    # 1. E0 and the gap below the Majumdar-Ghosh point (at it the ground state is twofold degenerate: E0 only, see 3.)
    ratios = [0.0, 0.1, 0.2, 0.3, 0.4]
    E0s, gaps = [], []
    for r in ratios:
        op = model(L, torch.tensor(r, dtype=F64, device=device), device)
        E0s.append(ground_energy(op, k).item())
        gaps.append(gap(op, k))
        print("J2/J1 = %.2f   E0 = %.12f   E0/L = %.8f   gap = %.8f" % (r, E0s[-1], E0s[-1] / L, gaps[-1]))
    # 2. dE0/dJ2 by autograd: <psi0| sum_i s_i . s_{i+2} |psi0> (Hellmann-Feynman), through the coupling gradients
    J2 = torch.tensor(0.3, dtype=F64, device=device, requires_grad=True)
    E0 = ground_energy(model(L, J2, device), k)
    (dE0,) = torch.autograd.grad(E0, J2)
    print("dE0/dJ2 at J2/J1 = 0.30: %.10f" % dE0.item())
    # 3. the Majumdar-Ghosh point
    E0_mg = energy(L, 0.5, device, k)
    print("Majumdar-Ghosh point J2 = J1/2: E0 = %.12f   (closed form -1.5 L = %.1f)" % (E0_mg, -1.5 * L))
    return {"J2": ratios, "E0": E0s, "gap": gaps, "J2_grad": 0.3, "dE0_dJ2": dE0.item(), "E0_mg": E0_mg}


if __name__ == "__main__":
    main()
