"""The spin gap of the J1-J2 Heisenberg ring as a difference of two dominant eigenpairs (docs/design/23-spin-inversion.md):

    H = J1 sum_i s_i . s_{i+1} + J2 sum_i s_i . s_{i+2},   s = (X, Y, Z) Pauli matrices, periodic, L sites (even)

At S^z = 0 the global spin flip F commutes with H and has the eigenvalue z = (-1)^(L/2 - S) on a state of total spin S, so the
lowest singlet and the lowest triplet lie in different z sectors.  With the translations they are the ground states of

    (k = 0 or pi, z = +-1):   k = 0, z = +1 for the singlet and k = pi, z = -1 for the triplet when L / 2 is even,
                              k = pi, z = -1 and k = 0, z = +1 when L / 2 is odd

(``ring_symmetries(L, momentum, spin_flip=z)``, |G| = 2 L), each about C(L, L/2) / (2 L) rows.  The gap is then
E0(triplet sector) - E0(singlet sector): two ``DominantSparseSymeig`` solves, each differentiable to second order, where the
lowest-two solver is first order only.  Below J2 / J1 = 0.2411 the lowest excitation of the ring is that triplet.

    python examples/spin_lattice/spin_gap.py [--L 20] [--J2 0.1] [--k 200] [--device cuda]

Prints E0 of both sectors, the gap, d gap / dJ2 and d2 gap / dJ2^2 by autograd, and the row counts beside the S^z = 0 sector's.
The operator is a device operator: the example needs a GPU.
"""
import argparse
import math
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
    return bonds, torch.cat([near, near, field]).to(device), torch.cat([nxt, nxt, field]).to(device)


def sectors(L):
    """((momentum, z) of the lowest singlet, (momentum, z) of the lowest triplet)"""
    return ((0, 1), ("pi", -1)) if (L // 2) % 2 == 0 else (("pi", -1), (0, 1))


def model(L, J2, momentum, z, device, J1=1.0):
    """the (momentum, z) sector of S^z = 0 at (J1, J2), with J2 a tensor that may require grad"""
    from dominantsparseeigenad_amd.operators import SpinSymmetrySectorOperator, ring_symmetries
    bonds, d1, d2 = directions(L, device)
    return SpinSymmetrySectorOperator(L, bonds, (J1 * d1 + J2 * d2).contiguous(), L // 2,
                                      ring_symmetries(L, momentum, spin_flip=z), device)


def ground_energy(op, k):
    import DominantSparseEigenAD.symeig as symeig
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    torch.manual_seed(0)
    E0, _ = symeig.DominantSparseSymeig.apply(op.couplings, min(k, op.dim), op.dim, op.device)
    return E0


def main(argv=None, L=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=20, help="ring length (even)")
    ap.add_argument("--J2", type=float, default=0.1)
    ap.add_argument("--k", type=int, default=200, help="Lanczos steps")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args([] if argv is None and L is not None else argv)
    if L is not None:
        args.L = L
    import DominantSparseEigenAD.CG as CG
    CG.EPS_DEFAULT = 1e-12
    device = torch.device(args.device)
    L = args.L
    n_full = math.comb(L, L // 2)
    J2 = torch.tensor(args.J2, dtype=F64, device=device, requires_grad=True)
    E, rows = [], []
    for name, (momentum, z) in zip(("singlet", "triplet"), sectors(L)):
        op = model(L, J2, momentum, z, device)
        E.append(ground_energy(op, args.k))
        rows.append(op.dim)
        print("L = %d  J2/J1 = %.2f  %s sector k = %-2s z = %+d  (n = %d, 1/%.1f of the %d rows of S^z = 0):  E0 = %.12f"
              % (L, args.J2, name, momentum, z, op.dim, n_full / op.dim, n_full, E[-1].item()))
    gap = E[1] - E[0]
    (d1,) = torch.autograd.grad(gap, J2, create_graph=True)
    (d2,) = torch.autograd.grad(d1, J2)
    print("gap = %.10f   d gap / dJ2 = %.10f   d2 gap / dJ2^2 = %.8f" % (gap.item(), d1.item(), d2.item()))
    return {"L": L, "J2": args.J2, "n_full": n_full, "sectors": sectors(L), "n": rows, "E0": [e.item() for e in E],
            "gap": gap.item(), "dgap_dJ2": d1.item(), "d2gap_dJ2": d2.item()}


if __name__ == "__main__":
    main()
