"""The dynamical structure factor of the Heisenberg ring at finite temperature (docs/design/35-finite-temperature-dynamics.md):

    H = J1 sum_i s_i . s_{i+1},   s = (X, Y, Z) Pauli matrices, periodic, L sites
    S^{zz}(q = pi, omega; T) = (1 / 2 pi) int dt e^{i omega t} <A(t) A>_T,    A = (1 / sqrt L) sum_j (-1)^j Z_j

what a neutron sees at the antiferromagnetic wave vector.  In every magnetisation sector R thermal pure quantum states
|beta, r> = e^{-beta H / 2} |r> are stepped in real time, A is applied to the whole block by one block ladder launch, and
<A b(t) | a(t)> is measured at every step by the fused dots kernel; small sectors are summed exactly over their spectrum.  The
record C(t_k), k = 0 .. K, is turned into the spectrum with a Gaussian window of width eta: dt = pi / (4 |J1| L) puts the Nyquist
frequency 4 |J1| L above every excitation energy (the band is narrower than 3 |J1| L), and K dt = 8 / eta lets the window decay.

THE PAULI CONVENTION: s = 2 S, so S^{zz} of spin-1/2 operators is a quarter of what is printed.  Printed per temperature: the
static sum rule C(0) = int d omega S(omega) beside the same number from ``thermal_correlations`` (c^T <Z_i Z_j> c, from the same
thermal states), and the spectrum on a few frequencies.

    python examples/spin_lattice/thermal_dynamics.py [--L 16] [--R 8] [--eta 0.25] [--seed 0] [--dense-below 256] [--device cuda]

The operators are device operators: the example needs a GPU.  The sampled sectors carry the sampling error of R vectors.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

F64 = torch.float64


def main(argv=None, L=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=16, help="ring length (even, so that q = pi is a momentum of the ring)")
    ap.add_argument("--J1", type=float, default=1.0)
    ap.add_argument("--R", type=int, default=8, help="random vectors per sampled sector")
    ap.add_argument("--eta", type=float, default=0.25, help="Gaussian broadening in units of |J1|")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dense-below", type=int, default=256, help="sector pairs of at most this dimension are summed exactly")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args([] if argv is None and L is not None else argv)
    if L is not None:
        args.L = L
    from dominantsparseeigenad_amd.operators import ring_bonds, ring_momentum_weights
    from dominantsparseeigenad_amd.thermal import thermal_correlations, thermal_dynamics
    L, J1 = args.L, args.J1
    if L < 4 or L % 2:
        raise SystemExit("--L must be even and at least 4")
    bonds = ring_bonds(L)
    couplings = torch.tensor([J1] * L + [J1] * L + [0.0] * L, dtype=F64)
    T = torch.tensor([4.0, 1.0, 0.25], dtype=F64) * abs(J1)                             # (descending: beta ascends)
    c, _ = ring_momentum_weights(L, L // 2)                                            # (-1)^j / sqrt(L); the sine part vanishes
    eta = args.eta * abs(J1)
    dt = math.pi / (4.0 * abs(J1) * L)
    K = int(math.ceil(8.0 / (eta * dt)))
    out = thermal_dynamics(L, bonds, couplings, c, "zz", 1.0 / T, dt, K, R=args.R, seed=args.seed, dense_below=args.dense_below,
                           device=args.device)
    corr = thermal_correlations(L, bonds, couplings, 1.0 / T, R=args.R, seed=args.seed, dense_below=args.dense_below,
                                device=args.device)
    static = torch.einsum("i,bij,j->b", c, corr.zz, c)
    # one Nyquist period in 2 K points: the sum over it is the integral of the trapezoid transform, C(0), exactly
    omega = (2.0 * math.pi / dt) * (torch.arange(2 * K, dtype=F64) / (2 * K) - 0.5)
    S = out.spectrum(omega, eta)
    print("L = %d  J1 = %.3f  R = %d  eta = %.3f  dt = %.4f  K = %d" % (L, J1, args.R, eta, dt, K))
    print("      T       C(0)      c^T <ZZ> c   int S d omega")
    d_omega = float(omega[1] - omega[0])
    for b in range(T.numel()):
        print("  %7.3f  %10.6f  %10.6f  %10.6f" % (T[b], out.static()[b], static[b], S[b].sum() * d_omega))
    show = [int(i) for i in torch.nonzero(omega.abs() <= 8.0 * abs(J1)).reshape(-1)[::max(1, K // 40)]]
    print("  omega   " + "  ".join("T = %-7.3f" % t for t in T.tolist()))
    for i in show:
        print("  %6.2f  " % omega[i] + "  ".join("%11.6f" % S[b, i] for b in range(T.numel())))
    return {"L": L, "T": T.tolist(), "static": out.static().tolist(), "static_correlations": static.tolist(), "omega": omega.tolist(),
            "S": S.tolist(), "logZ": out.logZ.tolist(), "dt": dt, "steps": K}


if __name__ == "__main__":
    main()
