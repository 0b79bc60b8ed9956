"""Entanglement of the ground state of the J1-J2 Heisenberg ring in its S^z = 0 sector (docs/design/21-reduced-density-matrix.md):

    H = J1 sum_i s_i . s_{i+1} + J2 sum_i s_i . s_{i+2},   s = (X, Y, Z) Pauli matrices, periodic, L sites (even)

on ``SpinSectorOperator`` with the reduced density matrices of ``Bipartition``: block diagonal in the number of set bits inside
the subsystem, every block a Gram matrix of a gathered slice of the eigenvector, formed on the fp64 matrix cores.

  1. the Renyi entropy S_2 and the von Neumann entropy S of half the ring (sites 0 .. L/2 - 1) on a grid of J2 / J1;
  2. dS_2/dJ2 by autograd THROUGH THE EIGENVECTOR of DominantSparseSymeig (the adjoint CG), beside a central difference;
  3. the two-site mutual information I(0 : r) = S(0) + S(r) - S(0, r) from three bipartitions per distance.

    python examples/spin_lattice/entanglement.py [--L 24] [--k 200] [--device cuda]

The operator is a device operator: the example needs a GPU.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

F64 = torch.float64


def model(L, J2, device, J1=1.0):
    """the S^z = 0 operator at (J1, J2), with J2 a tensor that may require grad"""
    from dominantsparseeigenad_amd.operators import SpinSectorOperator, ring_bonds
    bonds = ring_bonds(L, 1) + ring_bonds(L, 2)
    near = torch.cat([torch.ones(L, dtype=F64), torch.zeros(L, dtype=F64)])
    nxt = torch.cat([torch.zeros(L, dtype=F64), torch.ones(L, dtype=F64)])
    field = torch.zeros(L, dtype=F64)
    d1 = torch.cat([near, near, field]).to(device)
    d2 = torch.cat([nxt, nxt, field]).to(device)
    return SpinSectorOperator(L, bonds, (J1 * d1 + J2 * d2).contiguous(), L // 2, device)


def ground_state(op, k):
    import DominantSparseEigenAD.symeig as symeig
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    torch.manual_seed(0)
    return symeig.DominantSparseSymeig.apply(op.couplings, min(k, op.dim), op.dim, op.device)


def half_ring_renyi2(L, J2, device="cuda", k=200):
    """S_2 of sites 0 .. L/2 - 1 at J1 = 1 as a float"""
    device = torch.device(device)
    op = model(L, torch.tensor(float(J2), dtype=F64, device=device), device)
    _, psi = ground_state(op, k)
    return op.bipartition(range(L // 2)).renyi2(psi).item()


def main(argv=None, L=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=24, help="ring length (even)")
    ap.add_argument("--k", type=int, default=200, help="Lanczos steps")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args([] if argv is None and L is not None else argv)
    if L is not None:
        args.L = L
    import DominantSparseEigenAD.CG as CG
    CG.EPS_DEFAULT = 1e-12
    device = torch.device(args.device)
    L = args.L
    half = list(range(L // 2))
    # 1. the half-ring entropies below the Majumdar-Ghosh point
    ratios = [0.0, 0.2, 0.4]
    S2s, Ss = [], []
    for r in ratios:
        op = model(L, torch.tensor(r, dtype=F64, device=device), device)
        part = op.bipartition(half)              # (one index table per operator; an optimisation loop would keep it)
        _, psi = ground_state(op, args.k)
        S2s.append(part.renyi2(psi).item())
        Ss.append(part.entropy(psi).item())
        print("L = %d  S^z = 0 (n = %d)  J2/J1 = %.2f   half ring: S2 = %.10f   S = %.10f   (%d blocks, largest %d x %d)"
              % (L, op.dim, r, S2s[-1], Ss[-1], len(part.blocks), max(b[1] for b in part.blocks), max(b[2] for b in part.blocks)))
    # 2. dS2/dJ2 through the eigenvector adjoint, and a central difference
    at, h = 0.3, 1e-4
    J2 = torch.tensor(at, dtype=F64, device=device, requires_grad=True)
    op = model(L, J2, device)
    _, psi = ground_state(op, args.k)
    (dS2,) = torch.autograd.grad(op.bipartition(half).renyi2(psi), J2)
    fd = (half_ring_renyi2(L, at + h, device, args.k) - half_ring_renyi2(L, at - h, device, args.k)) / (2 * h)
    print("dS2/dJ2 at J2/J1 = %.2f: autograd %.9f   central difference %.9f" % (at, dS2.item(), fd))
    # 3. the two-site mutual information of the same state
    psi = psi.detach()
    s0 = op.bipartition([0]).entropy(psi).item()
    info = []
    for r in range(1, L // 2 + 1):
        sr = op.bipartition([r]).entropy(psi).item()
        s0r = op.bipartition([0, r]).entropy(psi).item()
        info.append(s0 + sr - s0r)
        print("I(0 : %d) = %.10f" % (r, info[-1]))
    return {"L": L, "n": op.dim, "J2": ratios, "S2": S2s, "S": Ss, "J2_grad": at, "dS2_dJ2": dS2.item(), "dS2_dJ2_fd": fd,
            "mutual_information": info}


if __name__ == "__main__":
    main()
