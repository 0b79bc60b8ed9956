"""Dynamical structure factors of the J1-J2 Heisenberg ring at zero temperature (docs/design/24-dynamics.md):

    H = J1 sum_i s_i . s_{i+1} + J2 sum_i s_i . s_{i+2},   s = (X, Y, Z) Pauli matrices, periodic, L sites (even)

    S^{zz}(q, omega) = sum_n |<n| Z_q |0>|^2 delta(omega - (E_n - E_0)),        Z_q = L^{-1/2} sum_j e^{i q j} Z_j
    S^{+-}(q, omega) = sum_n |<n| sigma^-_q |0>|^2 delta(omega - (E_n - E_0)),  sigma^-_q = L^{-1/2} sum_j e^{i q j} sigma^-_j

on the momentum grid q = 2 pi m / L, m = 1 .. L - 1.  The ground state |0> of the S^z = 0 sector comes from
DominantSparseSymeig; Z_q |0> stays in the sector and sigma^-_q |0> lands in the sector with one more down spin
(``SpinSectorLadder``); each spectral function is one ladder application and one Lanczos run per real weight vector
(``dynamical_structure_factor``: the continued fraction).

  1. the lowest pole of both channels per q beside the des Cloizeaux-Pearson lower boundary of the two-spinon continuum.  For
     H = J sum S_i . S_{i+1} with spin-1/2 operators S it is (pi / 2) J |sin q|.  THE PAULI CONVENTION: this Hamiltonian is
     written in s = 2 S, so J = 4 J1 and the boundary is 2 pi J1 |sin q| in the units printed here.  (It is the
     thermodynamic limit at J2 = 0; a finite ring lies above it.)
  2. the first-moment sum rule of S^{zz}: sum_n (E_n - E_0) |<n|Z_q|0>|^2 = -2 sum_bonds J_t |c_a - c_b|^2 <X_a X_b + Y_a Y_b>
     with c_j = e^{i q j} / sqrt(L) (again the Pauli convention: Z = 2 S^z), the right side from ``correlations``;
  3. the equal-time structure factor <0| Z_-q Z_q |0> as the zeroth moment, and both spectral functions broadened by eta on a
     frequency grid.  The ground state is a singlet, so S^{+-} = S^{zz} / 2 (sigma^- = S^-, Z = 2 S^z).

    python examples/spin_lattice/dynamics.py [--L 20] [--J2 0.0] [--k 200] [--eta 0.2] [--device cuda]

The operators are device operators: the example needs a GPU.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

F64 = torch.float64


def model(L, J2, ndown, device, J1=1.0):
    """(operator, bonds, the coupling of every bond) of the J1-J2 ring in the sector of ndown down spins"""
    from dominantsparseeigenad_amd.operators import SpinSectorOperator, ring_bonds
    bonds = ring_bonds(L, 1) + ring_bonds(L, 2)
    J = [J1] * L + [J2] * L
    couplings = torch.tensor(J + J + [0.0] * L, dtype=F64, device=device)
    return SpinSectorOperator(L, bonds, couplings, ndown, device), bonds, J


def f_sum(bonds, J, parts, xy):
    """-2 sum_t J_t |c_a - c_b|^2 <X_a X_b + Y_a Y_b> for c = re + i im"""
    total = 0.0
    for c in parts:
        total += -2.0 * sum(J[t] * float(c[a] - c[b]) ** 2 * float(xy[a, b]) for t, (a, b) in enumerate(bonds))
    return total


def main(argv=None, L=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=20, help="ring length (even)")
    ap.add_argument("--J2", type=float, default=0.0, help="next-nearest-neighbour coupling in units of J1")
    ap.add_argument("--k", type=int, default=200, help="Lanczos steps, for the ground state and per spectral function")
    ap.add_argument("--eta", type=float, default=0.2, help="Lorentzian broadening")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args([] if argv is None and L is not None else argv)
    if L is not None:
        args.L = L
    import DominantSparseEigenAD.CG as CG
    import DominantSparseEigenAD.symeig as symeig
    from dominantsparseeigenad_amd.operators import ring_momentum_weights
    from dominantsparseeigenad_amd.spectral import dynamical_structure_factor
    CG.EPS_DEFAULT = 1e-12
    device = torch.device(args.device)
    L = args.L
    if L % 2 or L < 4:
        raise SystemExit("--L must be even and at least 4")
    op, bonds, J = model(L, args.J2, L // 2, device)
    target, _, _ = model(L, args.J2, L // 2 + 1, device)        # the Hamiltonian of the sector that sigma^-_q lands in
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    torch.manual_seed(0)
    E0, psi0 = symeig.DominantSparseSymeig.apply(op.couplings, min(args.k, op.dim), op.dim, op.device)
    E0, psi0 = E0.item(), psi0.detach()
    xy, _, _ = op.correlations(psi0)
    xy = xy.cpu()
    print("L = %d  J2/J1 = %.2f  S^z = 0 (n = %d), S^z = -1 (n = %d)   E0 = %.12f" % (L, args.J2, op.dim, target.dim, E0))
    print("   q/pi   lowest pole zz   lowest pole +-   2 pi |sin q|   <Z_-q Z_q>   first moment   f-sum rule")
    omega = torch.linspace(0.0, 5.0 * math.pi, 201, dtype=F64)      # (the two-spinon continuum ends at 4 pi J1 |sin(q / 2)|)
    out = {"L": L, "n": op.dim, "E0": E0, "omega": omega.tolist(), "q": [], "gap_zz": [], "gap_pm": [], "dcp": [],
           "first_moment": [], "f_sum": [], "static_zz": [], "S_zz": [], "S_pm": []}
    for m in range(1, L):
        q = 2.0 * math.pi * m / L
        parts = ring_momentum_weights(L, m)
        zz = dynamical_structure_factor(op, psi0, E0, parts, "zz", k=args.k)
        pm = dynamical_structure_factor(op, psi0, E0, parts, "-", k=args.k, target=target)
        # the lowest pole that carries weight (a pole of weight ~ 0 is a direction the run picked up from rounding)
        gap_zz = float(zz.poles[zz.weights > 1e-12 * zz.norm2].min())
        gap_pm = float(pm.poles[pm.weights > 1e-12 * pm.norm2].min())
        dcp = 2.0 * math.pi * abs(math.sin(q))
        first, want = zz.moment(1), f_sum(bonds, J, parts, xy)
        print("  %5.3f   %14.8f   %14.8f   %12.8f   %10.6f   %12.8f   %10.8f"
              % (q / math.pi, gap_zz, gap_pm, dcp, zz.moment(0), first, want))
        for key, val in (("q", q), ("gap_zz", gap_zz), ("gap_pm", gap_pm), ("dcp", dcp), ("first_moment", first),
                         ("f_sum", want), ("static_zz", zz.moment(0))):
            out[key].append(val)
        out["S_zz"].append(zz(omega, args.eta).tolist())
        out["S_pm"].append(pm(omega, args.eta).tolist())
    return out


if __name__ == "__main__":
    main()
