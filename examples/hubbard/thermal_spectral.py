"""The one-particle spectral function of the half-filled Hubbard ring at finite temperature
(docs/design/37-hubbard-finite-temperature-dynamics.md):

    H = -t sum_{i, s} (c+_{i s} c_{i+1 s} + h.c.) + U sum_i n_{i up} n_{i dn},   periodic, L sites, mu = U / 2 (half filling)
    A(k, omega; T) = (1 / 2 pi) int dt e^{i omega t} < {c_{k up}(t), c+_{k up}} >_{T, mu},    c_k = (1 / sqrt L) sum_j e^{i k j} c_j (k and -k agree on the ring)

what angle-resolved photoemission (the removal part) and its inverse (the addition part) measure.  Both parts come from
``hubbard_thermal_dynamics``: over all (nup, ndn) sectors R thermal pure quantum states e^{-beta H / 2} |r> are stepped in real
time on both sides of the block ladder map and <A b(t) | a(t)> is measured at every step by the fused dots kernel; small sector
pairs and pairs with an empty or a full species are summed exactly over their spectra.  The addition record is transformed as
it is, the removal record reflected (omega -> -omega), with a Gaussian window of width eta; omega is printed from mu.

Printed per momentum and temperature: int A d omega beside its exact value 1 (the anticommutator), and the momentum
distribution n(k; T) = <c+_k c_k> = C_c(0); then A(k, omega; T) on a few frequencies.

    python examples/hubbard/thermal_spectral.py [--L 6] [--U 4] [--R 8] [--eta 0.25] [--seed 0] [--dense-below 256] [--device cuda]

The operators are device operators: the example needs a GPU.  The sampled pairs carry the sampling error of R vectors.
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
    ap.add_argument("--L", type=int, default=6, help="ring length (even: half filling is L / 2 particles per species)")
    ap.add_argument("--t", type=float, default=1.0)
    ap.add_argument("--U", type=float, default=4.0)
    ap.add_argument("--R", type=int, default=8, help="random vectors per sampled sector pair")
    ap.add_argument("--eta", type=float, default=0.25, help="Gaussian broadening in units of |t|")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dense-below", type=int, default=256, help="sector pairs of at most this dimension are summed exactly")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args([] if argv is None and L is not None else argv)
    if L is not None:
        args.L = L
    from dominantsparseeigenad_amd.operators import ring_bonds, ring_momentum_weights
    from dominantsparseeigenad_amd.thermal import hubbard_thermal_dynamics
    L, t, U = args.L, args.t, args.U
    if L < 4 or L % 2:
        raise SystemExit("--L must be even and at least 4")
    bonds = ring_bonds(L)
    couplings = torch.tensor([t] * L + [0.0] * L + [U] * L + [0.0] * L, dtype=F64)
    T = torch.tensor([2.0, 0.5], dtype=F64) * abs(t)                                   # (descending: beta ascends)
    mu = 0.5 * U
    eta = args.eta * abs(t)
    # the weight of A(k, omega) lies between the lower band edge -2 |t| and the upper Hubbard band's U + 2 |t|, up to thermal and
    # correlation tails: a Nyquist frequency of twice (4 |t| + |U|) keeps every alias outside the window's reach
    dt = math.pi / (2.0 * (4.0 * abs(t) + abs(U)))
    K = int(math.ceil(8.0 / (eta * dt)))
    omega = (2.0 * math.pi / dt) * (torch.arange(2 * K, dtype=F64) / (2 * K) - 0.5)    # one Nyquist period in 2 K points
    d_omega = float(omega[1] - omega[0])
    momenta = [0, L // 4, L // 2]
    common = dict(R=args.R, seed=args.seed, dense_below=args.dense_below, device=args.device)
    print("L = %d  t = %.3f  U = %.3f  mu = %.3f  R = %d  eta = %.3f  dt = %.4f  K = %d" % (L, t, U, mu, args.R, eta, dt, K))
    print("   k / pi      T     int A d omega     n(k; T)")
    spectra, sums, occupations = [], [], []
    for m in momenta:
        weights = ring_momentum_weights(L, m)
        add = hubbard_thermal_dynamics(L, bonds, couplings, weights, "cdag_up", 1.0 / T, [mu], dt, K, **common)
        rem = hubbard_thermal_dynamics(L, bonds, couplings, weights, "c_up", 1.0 / T, [mu], dt, K, **common)
        A = (add.spectrum(omega, eta) + rem.spectrum(omega, eta, reflected=True))[:, 0]             # [T, omega]
        spectra.append(A)
        sums.append((A.sum(dim=1) * d_omega).tolist())
        occupations.append(rem.static()[:, 0].tolist())
        for b in range(T.numel()):
            print("  %7.3f  %6.3f  %12.8f  %12.8f" % (2.0 * m / L, T[b], sums[-1][b], occupations[-1][b]))
    show = [int(i) for i in torch.nonzero((omega - mu).abs() <= 6.0 * abs(t) + 0.5 * abs(U)).reshape(-1)[::max(1, K // 30)]]
    print("  omega - mu  " + "  ".join("k = %.2f pi, T = %-5.2f" % (2.0 * m / L, temp) for m in momenta for temp in T.tolist()))
    for i in show:
        print("  %9.3f   " % (omega[i] - mu) + "  ".join("%19.6f" % spectra[a][b, i] for a in range(len(momenta))
                                                         for b in range(T.numel())))
    return {"L": L, "T": T.tolist(), "mu": mu, "momenta": momenta, "omega": omega.tolist(), "A": [a.tolist() for a in spectra],
            "sum": sums, "n_k": occupations, "dt": dt, "steps": K}


if __name__ == "__main__":
    main()
