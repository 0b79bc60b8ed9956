"""A disordered XXZ chain with per-site couplings as the parameters (docs/design/14-spin-chain.md):

    H = sum_b [Jx_b X_b X_b+1 + Jy_b Y_b Y_b+1 + Jz_b Z_b Z_b+1] + sum_i [hx_i X_i + hz_i Z_i],   couplings: (5, L)

  1. E0 and dE0/d(couplings) through DominantSparseSymeig;
  2. gap = E1 - E0 and dgap/d(couplings) through LowestSparseSymeig (one Lanczos run, deflated adjoint);
  3. ten optimiser steps that tune the longitudinal field hz (the other couplings stay fixed) to widen the gap.

    python examples/spin_chain/couplings.py [--L 12] [--k 200] [--device cuda] [--steps 10] [--lr 0.05]

On a CUDA device the operator is the matrix-free HIP kernel of ``operators.SpinChainOperator`` and the gradient of all 5 L
couplings is one pass of its parameter-adjoint kernel; on the CPU the same row formula is evaluated with torch ops.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

F64 = torch.float64


class SpinChain(object):
    """model class in the style of examples/TFIM/TFIM.py: ``couplings`` is the parameter, ``H`` the mat-vec,
    ``Hadjoint_to_couplingsadjoint`` the adjoint hook"""

    def __init__(self, L, device=torch.device("cpu")):
        self.N = int(L)
        self.dim = 1 << self.N
        self.device = torch.device(device)
        self._c = None
        self._op = None
        if self.device.type != "cuda":
            s = torch.arange(self.dim, dtype=torch.int64)
            self._s = s
            self._z = [(1 - 2 * ((s >> i) & 1)).to(F64) for i in range(self.N)]
            self._zz = [self._z[b] * self._z[(b + 1) % self.N] for b in range(self.N)]
            self._m = [(1 << b) | (1 << ((b + 1) % self.N)) for b in range(self.N)]

    @property
    def couplings(self):
        return self._c

    @couplings.setter
    def couplings(self, value):
        self._c = value
        if self.device.type == "cuda":
            if self._op is None:
                from dominantsparseeigenad_amd.operators import SpinChainOperator
                self._op = SpinChainOperator(self.N, value, self.device)
            else:
                self._op.couplings = value

    def _apply(self, c, v):
        y = torch.zeros_like(v)
        for b in range(self.N):
            y = y + (c[2, b] * self._zz[b] + c[4, b] * self._z[b]) * v + c[3, b] * v[self._s ^ (1 << b)]
            y = y + (c[0, b] - c[1, b] * self._zz[b]) * v[self._s ^ self._m[b]]
        return y

    def H(self, v):
        if self._op is not None:
            return self._op.H(v)
        return self._apply(self._c, v)

    def Hadjoint_to_couplingsadjoint(self, v1, v2):
        if self._op is not None:
            return self._op.Hadjoint_to_couplingsadjoint(v1, v2)
        rows = [[], [], [], [], []]
        for b in range(self.N):
            flipped = v2[self._s ^ self._m[b]]
            rows[0].append((v1 * flipped).sum())
            rows[1].append(-(self._zz[b] * v1 * flipped).sum())
            rows[2].append((self._zz[b] * v1 * v2).sum())
            rows[3].append((v1 * v2[self._s ^ (1 << b)]).sum())
            rows[4].append((self._z[b] * v1 * v2).sum())
        return torch.stack([torch.stack(r) for r in rows])

    @property
    def _native_methods(self):  # lets setDominantSparseSymeig(model.H, ...) find the native operator
        if self._op is None:
            raise AttributeError("_native_methods")
        return ("H",)

    @property
    def handle(self):
        return self._op.handle

    @property
    def n(self):
        return self.dim


def disordered_xxz(L, seed=0, delta=0.7, disorder=0.3):
    """Jx = Jy = 1 + disorder * noise, Jz = delta + disorder * noise, a weak transverse and a random longitudinal field"""
    rng = np.random.RandomState(seed)
    c = np.zeros((5, L))
    c[0] = c[1] = 1.0 + disorder * rng.uniform(-1, 1, L)
    c[2] = delta + disorder * rng.uniform(-1, 1, L)
    c[3] = 0.2 * rng.uniform(-1, 1, L)
    c[4] = disorder * rng.uniform(-1, 1, L)
    return torch.from_numpy(c)


def ground_state(model, k):
    import DominantSparseEigenAD.symeig as symeig
    symeig.setDominantSparseSymeig(model.H, model.Hadjoint_to_couplingsadjoint)
    E0, _ = symeig.DominantSparseSymeig.apply(model.couplings, k, model.dim, model.device)
    (dE0,) = torch.autograd.grad(E0, model.couplings)
    return E0.item(), dE0


def gap(model, k):
    import DominantSparseEigenAD.symeig as symeig
    symeig.setLowestSparseSymeig(model.H, model.Hadjoint_to_couplingsadjoint)
    vals, _ = symeig.LowestSparseSymeig.apply(model.couplings, k, model.dim, 2, model.device)
    return vals[1] - vals[0]


def main(argv=None, L=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=12, help="chain length")
    ap.add_argument("--k", type=int, default=200, help="Lanczos steps")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    args = ap.parse_args([] if argv is None and L is not None else argv)
    if L is not None:
        args.L = L
    import DominantSparseEigenAD.CG as CG
    CG.EPS_DEFAULT = 1e-12
    device = torch.device(args.device)
    model = SpinChain(args.L, device)
    k = min(args.k, model.dim)
    fixed = disordered_xxz(args.L, args.seed).to(device)
    hz = fixed[4].clone().requires_grad_(True)          # the tuned row

    def bind():
        model.couplings = torch.cat([fixed[:4], hz[None]], dim=0)

    bind()
    torch.manual_seed(0)
    E0, dE0 = ground_state(model, k)
    print("L = %d   E0 = %.12f   max |dE0/dcouplings| = %.6f" % (args.L, E0, dE0.abs().max().item()))
    bind()
    torch.manual_seed(0)
    g = gap(model, k)
    (dgap,) = torch.autograd.grad(g, model.couplings)
    print("gap = %.12f   dgap/dhz = %s" % (g.item(), " ".join("% .4f" % v for v in dgap[4].tolist())))
    opt = torch.optim.Adam([hz], lr=args.lr)
    gaps = []
    for step in range(args.steps):
        opt.zero_grad()
        bind()
        torch.manual_seed(0)
        g = gap(model, k)
        (-g).backward()
        gaps.append(g.item())
        opt.step()
        print("step %2d   gap = %.12f" % (step, gaps[-1]))
    bind()
    torch.manual_seed(0)
    gaps.append(gap(model, k).item())
    print("after %d steps: gap %.12f -> %.12f" % (args.steps, gaps[0], gaps[-1]))
    return {"E0": E0, "dE0": dE0.detach().cpu(), "gaps": gaps}


if __name__ == "__main__":
    main()
