"""The Hubbard ring at half filling on the matrix-free fermion operator (docs/design/19-hubbard.md):

    H = -t sum_{i, s} (c+_{i s} c_{i+1 s} + h.c.) + U sum_i n_{i up} n_{i dn},   periodic, L sites, nup = ndn = L / 2

as ``HubbardOperator(L, ring_bonds(L), couplings, L // 2, L // 2)`` with couplings = [t(nb), V(nb) = 0, U(L), eps(L) = 0].  The
space has C(L, L/2)^2 rows instead of 4^L (63 504 instead of 1 048 576 at L = 10).

  1. E0(U) over a short list of U (DominantSparseSymeig);
  2. the double occupancy per site <n_up n_dn> two ways: as (1 / L) sum_i dE0/dU_i by autograd through the couplings
     (Hellmann-Feynman; one pass of the parameter-adjoint kernel gives all 2 nb + 2 L coupling gradients), and as the U part
     of the bilinear forms psi^T (dH/dU_i) psi of the ground state itself;
  3. d^2 E0 / dU^2 with one U for all sites, by a second backward pass through the same two kernels;
  4. the two-site problem (one bond, one particle of each species), where E0 = (U - sqrt(U^2 + 16 t^2)) / 2.

    python examples/hubbard/ring.py [--L 10] [--k 200] [--device cuda]

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
    """(bonds, dt, dU): couplings = t * dt + U * dU is the Hubbard ring (V = eps = 0).  Two sites are joined by ONE bond (a
    ring of two would list it twice, which doubles t)."""
    from dominantsparseeigenad_amd.operators import ring_bonds
    bonds = ring_bonds(L) if L > 2 else [(0, 1)]
    nb = len(bonds)
    dt = torch.cat([torch.ones(nb, dtype=F64), torch.zeros(nb + 2 * L, dtype=F64)]).to(device)
    dU = torch.cat([torch.zeros(2 * nb, dtype=F64), torch.ones(L, dtype=F64), torch.zeros(L, dtype=F64)]).to(device)
    return bonds, dt, dU


def model(L, couplings_of, device, t=1.0):
    """the half-filled operator whose couplings are ``couplings_of(t * dt, dU)`` (a tensor that may carry a graph)"""
    from dominantsparseeigenad_amd.operators import HubbardOperator
    bonds, dt, dU = directions(L, device)
    return HubbardOperator(L, bonds, couplings_of(t * dt, dU).contiguous(), L // 2, L // 2, device)


def ground_state(op, k):
    import DominantSparseEigenAD.symeig as symeig
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    torch.manual_seed(0)
    return symeig.DominantSparseSymeig.apply(op.couplings, min(k, op.dim), op.dim, op.device)


def energy(L, U, device="cuda", k=200, t=1.0):
    """E0(U) of the half-filled ring as a float"""
    device = torch.device(device)
    op = model(L, lambda hop, dU: hop + float(U) * dU, device, t)
    return ground_state(op, k)[0].item()


def main(argv=None, L=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=10, help="ring length (even)")
    ap.add_argument("--k", type=int, default=200, help="Lanczos steps")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args([] if argv is None and L is not None else argv)
    if L is not None:
        args.L = L
    import DominantSparseEigenAD.CG as CG
    CG.EPS_DEFAULT = 1e-12
    device = torch.device(args.device)
    L = args.L
    # 1. E0 over U
    Us = [1.0, 2.0, 4.0, 8.0]       # (at U = 0 the spectrum is so degenerate that the Krylov space ends after a few steps)
    E0s = [energy(L, U, device, args.k) for U in Us]
    for U, E0 in zip(Us, E0s):
        print("L = %d  nup = ndn = %d  U/t = %.1f   E0 = %.12f   E0/L = %.8f" % (L, L // 2, U, E0, E0 / L))
    # 2. the double occupancy per site: every U_i its own parameter
    U0 = 4.0
    op = model(L, lambda hop, dU: (hop + U0 * dU).requires_grad_(True), device)
    E0, psi = ground_state(op, args.k)
    (grad,) = torch.autograd.grad(E0, op.couplings)
    docc_autograd = op.unpack(grad)[2].mean().item()
    psi = psi.detach()
    docc_forms = op.unpack(op.Hadjoint_to_couplingsadjoint(psi, psi))[2].mean().item()
    print("double occupancy per site at U/t = %.1f: %.12f (autograd, dE0/dU_i)   %.12f (forms of the ground state)"
          % (U0, docc_autograd, docc_forms))
    # 3. one U for all sites: first and second derivative
    U = torch.tensor(U0, dtype=F64, device=device, requires_grad=True)
    op = model(L, lambda hop, dU: hop + U * dU, device)
    E0 = ground_state(op, args.k)[0]
    (d1,) = torch.autograd.grad(E0, U, create_graph=True)
    (d2,) = torch.autograd.grad(d1, U)
    print("dE0/dU = %.10f   d2E0/dU2 = %.10f" % (d1.item(), d2.item()))
    # 4. two sites
    E0_two = energy(2, U0, device, args.k)
    closed = 0.5 * (U0 - math.sqrt(U0 * U0 + 16.0))
    print("two sites, U/t = %.1f: E0 = %.12f   (closed form %.12f)" % (U0, E0_two, closed))
    return {"L": L, "n": op.dim, "U": Us, "E0": E0s, "U_grad": U0, "E0_at_U_grad": E0.item(), "docc_autograd": docc_autograd,
            "docc_forms": docc_forms, "dE0_dU": d1.item(), "d2E0_dU2": d2.item(), "E0_two_site": E0_two,
            "E0_two_site_closed": closed}


if __name__ == "__main__":
    main()
