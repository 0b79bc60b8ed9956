"""The J1-J2 Heisenberg ring in its S^z = 0 sector, on the fixed-magnetisation operator (docs/design/18-spin-sector.md):

    H = J1 sum_i s_i . s_{i+1} + J2 sum_i s_i . s_{i+2},   s = (X, Y, Z) Pauli matrices, periodic, L sites (even)

as ``SpinSectorOperator(L, ring_bonds(L, 1) + ring_bonds(L, 2), couplings, ndown=L // 2)`` with Jxy = Jz on every bond and no
field.  The sector has C(L, L/2) rows instead of 2^L (2.7e6 instead of 1.7e7 at L = 24), and the S^z = +-1 partners of the
triplet are not in it: the first excited level of the sector is a single state, so the gap comes from a two-level run without
the degeneracy warning of examples/spin_lattice/j1j2.py.

  1. E0 and the gap E1 - E0 inside the sector over a few values of J2 / J1 (DominantSparseSymeig, LowestSparseSymeig, nev = 2);
  2. dE0/dJ2 by autograd through the couplings (one pass of the parameter-adjoint kernel gives all 4 L + L coupling gradients;
     the chain rule of ``couplings = J1 * d1 + J2 * d2`` folds them into one number);
  3. the Majumdar-Ghosh point J2 = J1 / 2 at L = 16, where E0 = -1.5 J1 L exactly.

    python examples/spin_lattice/sector.py [--L 24] [--Lmg 16] [--k 200] [--device cuda]

The operator is a device operator: the example needs a GPU.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

F64 = torch.float64


def directions(L, device):
    """(bonds, d1, d2): couplings = J1 * d1 + J2 * d2 is the Heisenberg J1-J2 ring (Jxy = Jz on every bond, no field)"""
    from dominantsparseeigenad_amd.operators import ring_bonds
    bonds = ring_bonds(L, 1) + ring_bonds(L, 2)
    near = torch.cat([torch.ones(L, dtype=F64), torch.zeros(L, dtype=F64)])
    nxt = torch.cat([torch.zeros(L, dtype=F64), torch.ones(L, dtype=F64)])
    field = torch.zeros(L, dtype=F64)
    d1 = torch.cat([near, near, field]).to(device)
    d2 = torch.cat([nxt, nxt, field]).to(device)
    return bonds, d1, d2


def model(L, J2, device, J1=1.0):
    """the S^z = 0 operator at (J1, J2), with J2 a tensor that may require grad"""
    from dominantsparseeigenad_amd.operators import SpinSectorOperator
    bonds, d1, d2 = directions(L, device)
    return SpinSectorOperator(L, bonds, (J1 * d1 + J2 * d2).contiguous(), L // 2, device)


def ground_energy(op, k):
    import DominantSparseEigenAD.symeig as symeig
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    torch.manual_seed(0)
    E0, _ = symeig.DominantSparseSymeig.apply(op.couplings, k, op.dim, op.device)
    return E0


def energy(L, J2, device="cuda", k=200):
    """E0(J2) of the S^z = 0 sector at J1 = 1 as a float"""
    device = torch.device(device)
    op = model(L, torch.tensor(float(J2), dtype=F64, device=device), device)
    return ground_energy(op, min(k, op.dim)).item()


def gap(op, k):
    import DominantSparseEigenAD.symeig as symeig
    symeig.setLowestSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    torch.manual_seed(0)
    vals, _ = symeig.LowestSparseSymeig.apply(op.couplings, k, op.dim, 2, op.device)
    return (vals[1] - vals[0]).item()


def main(argv=None, L=None, L_mg=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=24, help="ring length (even)")
    ap.add_argument("--Lmg", type=int, default=16, help="ring length of the Majumdar-Ghosh check (even)")
    ap.add_argument("--k", type=int, default=200, help="Lanczos steps")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args([] if argv is None and L is not None else argv)
    if L is not None:
        args.L = L
        args.Lmg = min(args.Lmg, L) if L_mg is None else L_mg
    import DominantSparseEigenAD.CG as CG
    CG.EPS_DEFAULT = 1e-12
    device = torch.device(args.device)
    L = args.L
    # 1. E0 and the gap inside the sector, below the Majumdar-Ghosh point (at it the ground state is twofold degenerate)
    ratios = [0.0, 0.2, 0.4]
    E0s, gaps = [], []
    for r in ratios:
        op = model(L, torch.tensor(r, dtype=F64, device=device), device)
        k = min(args.k, op.dim)
        E0s.append(ground_energy(op, k).item())
        gaps.append(gap(op, k))
        print("L = %d  S^z = 0 (n = %d)  J2/J1 = %.2f   E0 = %.12f   E0/L = %.8f   gap = %.8f"
              % (L, op.dim, r, E0s[-1], E0s[-1] / L, gaps[-1]))
    # 2. dE0/dJ2 by autograd: <psi0| sum_i s_i . s_{i+2} |psi0> (Hellmann-Feynman), through the coupling gradients
    J2 = torch.tensor(0.3, dtype=F64, device=device, requires_grad=True)
    op = model(L, J2, device)
    E0 = ground_energy(op, min(args.k, op.dim))
    (dE0,) = torch.autograd.grad(E0, J2)
    print("dE0/dJ2 at J2/J1 = 0.30: %.10f" % dE0.item())
    # 3. the Majumdar-Ghosh point
    E0_mg = energy(args.Lmg, 0.5, device, args.k)
    print("Majumdar-Ghosh point J2 = J1/2, L = %d: E0 = %.12f   (closed form -1.5 L = %.1f)" % (args.Lmg, E0_mg, -1.5 * args.Lmg))
    return {"L": L, "n": op.dim, "J2": ratios, "E0": E0s, "gap": gaps, "J2_grad": 0.3, "dE0_dJ2": dE0.item(),
            "L_mg": args.Lmg, "E0_mg": E0_mg}


if __name__ == "__main__":
    main()
