"""Excitation gap of the 1-D TFIM, Delta(g) = E1 - E0, and dDelta/dg through LowestSparseSymeig (the two lowest
eigenpairs from one Lanczos run, the derivative from the deflated adjoint; docs/design/13-lowest-eigenpairs.md).

    python examples/TFIM/gap.py [--N 10] [--k 300] [--points 11] [--device cuda] [--check]

--check also evaluates Delta and dDelta/dg by torch.linalg.eigh autograd on the dense matrix (small N) and prints the
largest differences.  The levels must be non-degenerate up to E2: at g < 1 the two lowest levels of a finite chain
approach each other exponentially in N, so the default grid stays in the paramagnetic phase.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from TFIM import TFIM  # noqa: E402


def gap_sparseAD(model, k):
    import DominantSparseEigenAD.symeig as symeig
    symeig.setLowestSparseSymeig(model.H, model.Hadjoint_to_gadjoint)
    vals, _ = symeig.LowestSparseSymeig.apply(model.g, k, model.dim, 2, model.device)
    gap = vals[1] - vals[0]
    dgap, = torch.autograd.grad(gap, model.g)
    return gap.item(), dgap.item()


def gap_torchAD(model):
    model.setHmatrix()
    w, _ = torch.linalg.eigh(model.Hmatrix)
    gap = w[1] - w[0]
    dgap, = torch.autograd.grad(gap, model.g)
    return gap.item(), dgap.item()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=10, help="chain length (10 ... 20)")
    ap.add_argument("--k", type=int, default=300)
    ap.add_argument("--points", type=int, default=11)
    ap.add_argument("--gmin", type=float, default=1.2)
    ap.add_argument("--gmax", type=float, default=2.0)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--check", action="store_true", help="compare with eigh autograd on the dense matrix (N <= 12)")
    args = ap.parse_args(argv)
    import DominantSparseEigenAD.CG as CG
    CG.EPS_DEFAULT = 1e-12
    model = TFIM(args.N, torch.device(args.device))
    k = min(args.k, model.dim)
    rows = []
    print("#        g            gap       dgap/dg" + ("      dense gap  dense dgap/dg" if args.check else ""))
    for gval in np.linspace(args.gmin, args.gmax, num=args.points):
        model.g = torch.tensor([gval], dtype=torch.float64, device=model.device, requires_grad=True)
        torch.manual_seed(0)
        row = [gval, *gap_sparseAD(model, k)]
        if args.check:
            model.g = torch.tensor([gval], dtype=torch.float64, device=model.device, requires_grad=True)
            row += [*gap_torchAD(model)]
        rows.append(row)
        print(" ".join("% .12f" % v for v in row))
    rows = np.array(rows)
    if args.check:
        print("max |gap - dense| = %.3e   max |dgap/dg - dense| = %.3e"
              % (np.abs(rows[:, 1] - rows[:, 3]).max(), np.abs(rows[:, 2] - rows[:, 4]).max()))
        if np.abs(rows[:, 1] - rows[:, 3]).max() > 1e-8 or np.abs(rows[:, 2] - rows[:, 4]).max() > 1e-7:
            sys.exit(1)
    return rows


if __name__ == "__main__":
    main()
