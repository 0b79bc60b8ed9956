"""Optical conductivity, f-sum rule and charge stiffness of the half-filled Hubbard ring (docs/design/39-hubbard-current.md):

    H = -t sum_{i, s} (c+_{i s} c_{i+1 s} + h.c.) + U sum_i n_{i up} n_{i dn},   L sites, nup = ndn = L / 2

The field runs along the ring, so every bond (i, i + 1) has the displacement d = +1 -- the bond (L - 1, 0) that closes the
ring too: on a periodic cluster the displacement is the minimum image, not 1 - L.  With the current map K(w), w_t = t d_t
(``HubbardCurrent``), ``optical_conductivity`` returns

    sigma(omega) = pi D_s delta(omega) + sigma_reg(omega),   sigma_reg(omega > 0) = pi sum_n |<n| K |0>|^2 / (E_n - E0) delta(omega - (E_n - E0))
    D_s = K_d - 2 I_-1 = d^2 E0 / d phi^2   (Kohn's stiffness; the Drude weight is pi D_s),   K_d = -<kinetic energy>
    f-sum rule:  pi D_s / 2 + int_0^inf sigma_reg = pi K_d / 2

  1. the ring over a short list of U: K_d, I_-1, the stiffness, the optical gap (the lowest pole that carries weight: the
     Mott gap of the finite ring) and sigma_reg on a grid;
  2. the open chain of the same length beside the ring: a twist of a chain is a gauge transformation, so its stiffness is 0
     and all of the f-sum is in the regular part;
  3. the f-sum check of every case.

    python examples/hubbard/optical.py [--L 6] [--k 200] [--eta 0.1] [--device cuda]

On L = 4 m + 2 sites the stiffness is positive and falls with U; on L = 4 m sites with periodic boundaries it is negative.
The operator is a device operator: the example needs a GPU.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

F64 = torch.float64


def model(L, U, periodic, device, t=1.0):
    """(operator, displacements) of the half-filled ring or open chain"""
    from dominantsparseeigenad_amd.operators import HubbardOperator
    bonds = [(i, (i + 1) % L) for i in range(L if periodic else L - 1)]
    nb = len(bonds)
    couplings = torch.cat([t * torch.ones(nb, dtype=F64), torch.zeros(nb, dtype=F64), U * torch.ones(L, dtype=F64),
                           torch.zeros(L, dtype=F64)]).to(device)
    return HubbardOperator(L, bonds, couplings, L // 2, L // 2, device), torch.ones(nb, dtype=F64)


def ground_state(op, k):
    import DominantSparseEigenAD.symeig as symeig
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    torch.manual_seed(0)
    E0, psi = symeig.DominantSparseSymeig.apply(op.couplings, min(k, op.dim), op.dim, op.device)
    return E0.item(), psi.detach()


def response(L, U, periodic, device, k):
    from dominantsparseeigenad_amd.spectral import optical_conductivity
    op, d = model(L, U, periodic, device)
    E0, psi = ground_state(op, k)
    return E0, optical_conductivity(op, psi, E0, d, kind="charge", k=k)


def optical_gap(res, share=1e-6):
    """the lowest pole above the floor that carries more than ``share`` of the weight"""
    m = res.measure
    keep = (m.poles > res.floor) & (m.weights > share * m.norm2)
    return float(m.poles[keep].min()) if bool(keep.any()) else float("nan")


def main(argv=None, L=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=6, help="ring length (even, at least 4)")
    ap.add_argument("--k", type=int, default=200, help="Lanczos steps")
    ap.add_argument("--eta", type=float, default=0.1, help="Lorentzian half width of sigma_reg")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args([] if argv is None and L is not None else argv)
    if L is not None:
        args.L = L
    L = args.L
    if L < 4 or L % 2:
        raise ValueError("the half-filled ring needs an even L >= 4, got %d" % L)
    import DominantSparseEigenAD.CG as CG
    CG.EPS_DEFAULT = 1e-12
    device = torch.device(args.device)
    Us = [1.0, 2.0, 4.0, 8.0]
    omega = torch.linspace(0.0, 12.0, 241, dtype=F64)
    out = {"L": L, "U": Us, "ring": [], "omega": omega, "sigma": []}
    print("half-filled ring, L = %d, nup = ndn = %d, field along the ring (d_t = 1 on every bond)" % (L, L // 2))
    for U in Us:
        E0, res = response(L, U, True, device, args.k)
        lhs, rhs = res.f_sum()
        sigma = res.regular(omega, args.eta)
        peak = float(omega[int(sigma.argmax())])
        print("U/t = %4.1f   E0 = %.10f   K_d = %.8f   I_-1 = %.8f   stiffness = %+.8f   optical gap = %.6f   sigma_reg peaks at "
              "omega = %.2f   f-sum: %.10f = %.10f" % (U, E0, res.diamagnetic, res.inverse_moment, res.stiffness, optical_gap(res),
                                                      peak, lhs, rhs))
        out["ring"].append({"U": U, "E0": E0, "diamagnetic": res.diamagnetic, "inverse_moment": res.inverse_moment,
                            "stiffness": res.stiffness, "gap": optical_gap(res), "dropped_weight": res.dropped_weight,
                            "f_sum": (lhs, rhs)})
        out["sigma"].append(sigma)
    U0 = 4.0
    E0, res = response(L, U0, False, device, args.k)
    lhs, rhs = res.f_sum()
    ring = out["ring"][Us.index(U0)]
    print("open chain at U/t = %.1f: K_d = %.8f   2 I_-1 = %.8f   stiffness = %+.2e   (ring: %+.8f)   f-sum: %.10f = %.10f"
          % (U0, res.diamagnetic, 2.0 * res.inverse_moment, res.stiffness, ring["stiffness"], lhs, rhs))
    out["chain"] = {"U": U0, "E0": E0, "diamagnetic": res.diamagnetic, "inverse_moment": res.inverse_moment,
                    "stiffness": res.stiffness, "gap": optical_gap(res), "dropped_weight": res.dropped_weight, "f_sum": (lhs, rhs)}
    return out


if __name__ == "__main__":
    main()
