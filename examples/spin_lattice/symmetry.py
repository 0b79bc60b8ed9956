"""The J1-J2 Heisenberg ring inside momentum / parity sectors (docs/design/20-symmetry-sector.md):

    H = J1 sum_i s_i . s_{i+1} + J2 sum_i s_i . s_{i+2},   s = (X, Y, Z) Pauli matrices, periodic, L sites (even)

as ``SpinSymmetrySectorOperator(L, bonds, couplings, L // 2, ring_symmetries(L, momentum, parity))``: the S^z = 0 sector
reduced further by the translations (momentum k = 0 or pi) and the reflection (parity p = +-1) of the ring.  Each of the four
sectors has about C(L, L/2) / (2 L) rows.

  1. E0 and the gap E1 - E0 inside each of the four (k, p) sectors, beside E0 of the full S^z = 0 sector: the smallest of the
     four is the ground state of the ring;
  2. dE0/dJ2 by autograd through the couplings, in the sector that holds the ground state.

    python examples/spin_lattice/symmetry.py [--L 24] [--J2 0.3] [--k 200] [--device cuda]

The operator is a device operator: the example needs a GPU.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

F64 = torch.float64
SECTORS = [(0, 1), (0, -1), ("pi", 1), ("pi", -1)]


def directions(L, device):
    """(bonds, d1, d2): couplings = J1 * d1 + J2 * d2 is the Heisenberg J1-J2 ring (Jxy = Jz on every bond, no field)"""
    from dominantsparseeigenad_amd.operators import ring_bonds
    bonds = ring_bonds(L, 1) + ring_bonds(L, 2)
    near = torch.cat([torch.ones(L, dtype=F64), torch.zeros(L, dtype=F64)])
    nxt = torch.cat([torch.zeros(L, dtype=F64), torch.ones(L, dtype=F64)])
    field = torch.zeros(L, dtype=F64)
    return bonds, torch.cat([near, near, field]).to(device), torch.cat([nxt, nxt, field]).to(device)


def model(L, J2, momentum, parity, device, J1=1.0):
    """the (momentum, parity) sector of S^z = 0 at (J1, J2), with J2 a tensor that may require grad"""
    from dominantsparseeigenad_amd.operators import SpinSymmetrySectorOperator, ring_symmetries
    bonds, d1, d2 = directions(L, device)
    return SpinSymmetrySectorOperator(L, bonds, (J1 * d1 + J2 * d2).contiguous(), L // 2, ring_symmetries(L, momentum, parity),
                                      device)


def full_model(L, J2, device, J1=1.0):
    from dominantsparseeigenad_amd.operators import SpinSectorOperator
    bonds, d1, d2 = directions(L, device)
    return SpinSectorOperator(L, bonds, (J1 * d1 + J2 * d2).contiguous(), L // 2, device)


def ground_energy(op, k):
    import DominantSparseEigenAD.symeig as symeig
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    torch.manual_seed(0)
    E0, _ = symeig.DominantSparseSymeig.apply(op.couplings, min(k, op.dim), op.dim, op.device)
    return E0


def gap(op, k):
    import DominantSparseEigenAD.symeig as symeig
    symeig.setLowestSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    torch.manual_seed(0)
    vals, _ = symeig.LowestSparseSymeig.apply(op.couplings, min(k, op.dim), op.dim, 2, op.device)
    return (vals[1] - vals[0]).item()


def main(argv=None, L=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=24, help="ring length (even)")
    ap.add_argument("--J2", type=float, default=0.3)
    ap.add_argument("--k", type=int, default=200, help="Lanczos steps")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args([] if argv is None and L is not None else argv)
    if L is not None:
        args.L = L
    import DominantSparseEigenAD.CG as CG
    CG.EPS_DEFAULT = 1e-12
    device = torch.device(args.device)
    L = args.L
    # 1. the four sectors beside the full S^z = 0 sector
    full = full_model(L, torch.tensor(args.J2, dtype=F64, device=device), device)
    E_full = ground_energy(full, args.k).item()
    print("L = %d  J2/J1 = %.2f  full S^z = 0 sector (n = %d): E0 = %.12f" % (L, args.J2, full.dim, E_full))
    rows, E0s, gaps = [], [], []
    for momentum, parity in SECTORS:
        op = model(L, torch.tensor(args.J2, dtype=F64, device=device), momentum, parity, device)
        rows.append(op.dim)
        E0s.append(ground_energy(op, args.k).item())
        gaps.append(gap(op, args.k))
        print("  k = %-2s  p = %+d  (n = %d, 1/%.1f of the sector)   E0 = %.12f   gap = %.8f"
              % (momentum, parity, op.dim, full.dim / op.dim, E0s[-1], gaps[-1]))
    best = min(range(4), key=lambda i: E0s[i])
    # 2. dE0/dJ2 in the ground-state sector: <psi0| sum_i s_i . s_{i+2} |psi0>, through the coupling gradients
    J2 = torch.tensor(args.J2, dtype=F64, device=device, requires_grad=True)
    op = model(L, J2, SECTORS[best][0], SECTORS[best][1], device)
    (dE0,) = torch.autograd.grad(ground_energy(op, args.k), J2)
    print("ground state in k = %s, p = %+d: dE0/dJ2 = %.10f" % (SECTORS[best][0], SECTORS[best][1], dE0.item()))
    return {"L": L, "J2": args.J2, "n_full": full.dim, "E0_full": E_full, "sectors": SECTORS, "n": rows, "E0": E0s, "gap": gaps,
            "ground_sector": SECTORS[best], "dE0_dJ2": dE0.item()}


if __name__ == "__main__":
    main()
