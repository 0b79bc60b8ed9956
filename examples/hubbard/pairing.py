"""Pair correlations, total spin and the eta-pairing pole of the Hubbard ring and open chain
(docs/design/41-hubbard-pair-ladder.md):

    H = -t sum_{i, s} (c+_{i s} c_{i+1 s} + h.c.) + U sum_i n_{i up} n_{i dn},   L sites

All three need an operator that moves one particle of each species at once (``HubbardPairLadder``):

  1. the pair correlations P_ab = <Delta+(W_a) Delta(W_b)> of the half-filled ground state against U, for the on-site field
     Delta+ = sum_i c+_{i up} c+_{i dn} (``onsite_pairing``) and the nearest-neighbour singlet field sum_bonds (c+_{a up} c+_{b dn} +
     c+_{b up} c+_{a dn}) / sqrt(2) (``bond_pairing``), on the ring and on the open chain: a repulsive U suppresses the on-site
     pairs, the nearest-neighbour singlets survive;
  2. <S^2> = |S+ psi|^2 + S^z (S^z + 1) of the ground states of several fillings (``total_spin``): a singlet at half filling,
     S = 1/2 with one unpaired particle, S = 1 for the open shell of two particles per species less on L = 4 m + 2 sites;
  3. Yang's eta pairing on the (bipartite) ring: eta+ = sum_i (-1)^i c+_{i up} c+_{i dn} obeys [H, eta+] = U eta+, so the pair
     addition spectrum of this field has ALL its weight in one pole at omega = U, whatever the state it is added to
     (``hubbard_pair_spectral_function``).

    python examples/hubbard/pairing.py [--L 6] [--k 200] [--device cuda]

The operator is a device operator: the example needs a GPU.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

F64 = torch.float64


def model(L, U, periodic, nup, ndn, device, t=1.0):
    from dominantsparseeigenad_amd.operators import HubbardOperator
    bonds = [(i, (i + 1) % L) for i in range(L if periodic else L - 1)]
    nb = len(bonds)
    couplings = torch.cat([t * torch.ones(nb, dtype=F64), torch.zeros(nb, dtype=F64), U * torch.ones(L, dtype=F64),
                           torch.zeros(L, dtype=F64)]).to(device)
    return HubbardOperator(L, bonds, couplings, nup, ndn, device)


def ground_state(op, k):
    import DominantSparseEigenAD.symeig as symeig
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    torch.manual_seed(0)
    E0, psi = symeig.DominantSparseSymeig.apply(op.couplings, min(k, op.dim), op.dim, op.device)
    return E0.item(), psi.detach()


def main(argv=None, L=None):
    from dominantsparseeigenad_amd.operators import bond_pairing, onsite_pairing, pair_correlations, total_spin
    from dominantsparseeigenad_amd.spectral import hubbard_pair_spectral_function
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=6, help="sites (even, at least 6)")
    ap.add_argument("--k", type=int, default=200, help="Lanczos steps")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args([] if argv is None and L is not None else argv)
    if L is not None:
        args.L = L
    L = args.L
    if L < 6 or L % 2:
        raise ValueError("the example needs an even L >= 6, got %d" % L)
    import DominantSparseEigenAD.CG as CG
    CG.EPS_DEFAULT = 1e-12
    device = torch.device(args.device)
    half = L // 2
    Us = [0.0, 2.0, 4.0, 8.0]
    out = {"L": L, "U": Us, "pair": {}, "spin": [], "eta": []}

    print("1. pair correlations of the half-filled ground state, L = %d, (nup, ndn) = (%d, %d)" % (L, half, half))
    for name, periodic in (("ring", True), ("chain", False)):
        rows = []
        for U in Us:
            op = model(L, U, periodic, half, half, device)
            _, psi = ground_state(op, args.k)
            fields = torch.stack([onsite_pairing(L), bond_pairing(L, op.bonds, torch.ones(op.nb, dtype=F64))]).to(device)
            P = pair_correlations(op, psi, fields).cpu()
            rows.append({"U": U, "onsite": float(P[0, 0]), "bond": float(P[1, 1]), "cross": float(P[0, 1])})
            print("   %-5s U/t = %4.1f   <D+_s D_s> = %.8f   <D+_nn D_nn> = %.8f   <D+_s D_nn> = %+.8f"
                  % (name, U, rows[-1]["onsite"], rows[-1]["bond"], rows[-1]["cross"]))
        out["pair"][name] = rows

    U0 = 4.0
    print("2. <S^2> of ring ground states at U/t = %.1f" % U0)
    for nup, ndn in ((half, half), (half - 1, half), (half - 1, half - 1), (1, 2)):
        op = model(L, U0, True, nup, ndn, device)
        _, psi = ground_state(op, args.k)
        s2 = float(total_spin(op, psi))
        out["spin"].append({"nup": nup, "ndn": ndn, "S2": s2})
        print("   (nup, ndn) = (%d, %d)   <S^2> = %.10f" % (nup, ndn, s2))

    print("3. the eta-pairing pole of the ring: pair addition with eta+ = sum_i (-1)^i c+_{i up} c+_{i dn} on (%d, %d)"
          % (half - 1, half - 1))
    eta = onsite_pairing(L, [(-1.0) ** i for i in range(L)])
    for U in (2.0, 4.0):
        op = model(L, U, True, half - 1, half - 1, device)
        E0, psi = ground_state(op, args.k)
        m = hubbard_pair_spectral_function(op, psi, E0, eta, "pair_add", k=min(args.k, 40))
        top = int(m.weights.argmax())
        out["eta"].append({"U": U, "pole": float(m.poles[top]), "weight": float(m.weights[top]), "total": float(m.moment(0))})
        print("   U/t = %4.1f   |eta+ psi0|^2 = %.10f   heaviest pole at omega = %.10f with weight %.10f"
              % (U, out["eta"][-1]["total"], out["eta"][-1]["pole"], out["eta"][-1]["weight"]))
    return out


if __name__ == "__main__":
    main()
