"""Timings of the symmetry-sector spin kernels with and without spin inversion on one GPU (docs/design/23-spin-inversion.md) on
the 4 x 6 torus of 20.6: square_bonds(4, 6) (48 bonds), Heisenberg couplings, L = 24, ndown = 12, k = (0, 0).  Two sides in one
process, one after the other, five rounds each:

    flip:     torus_symmetries(4, 6, spin_flip=+1), |G| = 48 (NGL = 4), the *_flip kernels
    no flip:  torus_symmetries(4, 6),               |G| = 24 (NGL = 2), n = 112 800, the kernels of note 20

Reported for each side, median (min - max): n, the table build (host clock to a synchronise), the mat-vec
(k_spmv_symsector_flip / k_spmv_symsector) and the forms pair (forms + reduce) between two events, and forward + backward of
E0 through DominantSparseSymeig (k = 100 Lanczos steps, default re-orthogonalisation and CG tolerance; a fresh operator per
round, the table build outside the clock).  No ratio is required: the script says which side is faster.

    python tools/kbench_spinflip.py [--Lx 4] [--Ly 6] [--k 100] [--reps 50] [--rounds 5] [--out profiles/kbench_spinflip.json]
"""
import argparse
import json
import os
import sys
import time
from ctypes import byref, c_int64

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from dominantsparseeigenad_amd import _lib  # noqa: E402
from dominantsparseeigenad_amd.engine import _ptr, _stream  # noqa: E402
from dominantsparseeigenad_amd.operators import SpinSymmetrySectorOperator, square_bonds, torus_symmetries  # noqa: E402
import dominantsparseeigenad_amd.symeig as symeig  # noqa: E402

F64 = torch.float64


def timed(fn, reps, rounds):
    """median over `rounds` of the mean of `reps` back-to-back calls, in us (after a warm-up round): (median, min, max)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def e0_rounds(make, k, rounds):
    """forward + backward of E0 in ms, one fresh operator per round (after one warm-up round): (median, min, max, E0)"""
    out, E = [], None
    for r in range(rounds + 1):
        op = make()
        symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        E0, _ = symeig.DominantSparseSymeig.apply(op.couplings, min(k, op.dim), op.dim, op.device)
        (g,) = torch.autograd.grad(E0, op.couplings)
        torch.cuda.synchronize()
        if r > 0:
            out.append((time.perf_counter() - t0) * 1e3)
        E = E0.item()
    out.sort()
    return out[len(out) // 2], out[0], out[-1], E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Lx", type=int, default=4)
    ap.add_argument("--Ly", type=int, default=6)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda:0")
    L = args.Lx * args.Ly
    ndown = L // 2
    bonds = square_bonds(args.Lx, args.Ly)
    nb = len(bonds)
    st = _stream(dev)

    def heisenberg(grad):
        p = torch.cat([torch.ones(2 * nb, dtype=F64, device=dev), torch.zeros(L, dtype=F64, device=dev)])   # Jxy = Jz = 1
        return p.requires_grad_(True) if grad else p

    def side(name, gens):
        builds = []
        for _ in range(args.rounds + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            op = SpinSymmetrySectorOperator(L, bonds, heisenberg(False), ndown, gens)
            torch.cuda.synchronize()
            builds.append((time.perf_counter() - t0) * 1e3)
        builds = sorted(builds[1:])
        n = op.n
        gen = torch.Generator(dev).manual_seed(1)
        x = torch.randn(n, dtype=F64, device=dev, generator=gen)
        x2 = torch.randn(n, dtype=F64, device=dev, generator=gen)
        y = torch.empty(n, dtype=F64, device=dev)
        t_mv = timed(lambda: lib.dsea_spmv(op.handle, None, _ptr(x), _ptr(y), None, None, None, st), args.reps, args.rounds)
        cnt = c_int64()
        _lib.check(lib.dsea_op_symsector_forms_scratch_doubles(n, L, nb, byref(cnt)), "scratch")
        scratch = torch.empty(cnt.value, dtype=F64, device=dev)
        out = torch.empty(2 * nb + L, dtype=F64, device=dev)
        t_forms = timed(lambda: lib.dsea_op_symsector_forms(op.handle, _ptr(x), _ptr(x2), _ptr(out), _ptr(scratch), st),
                        max(5, args.reps // 5), args.rounds)
        e0 = e0_rounds(lambda: SpinSymmetrySectorOperator(L, bonds, heisenberg(True), ndown, gens), args.k, args.rounds)
        return {"side": name, "group": op.ng, "flipped_elements": int(sum(op.flips)), "n": n,
                "table_build_ms": (builds[len(builds) // 2], builds[0], builds[-1]), "matvec_us": t_mv, "forms_pair_us": t_forms,
                "e0_forward_backward_ms": e0[:3], "E0": e0[3]}

    flip = side("k = (0, 0), z = +1", torus_symmetries(args.Lx, args.Ly, 0, 0, spin_flip=1))
    plain = side("k = (0, 0), no flip", torus_symmetries(args.Lx, args.Ly, 0, 0))

    def faster(key):
        return flip["side"] if flip[key][0] < plain[key][0] else plain["side"]

    rec = {"L": L, "ndown": ndown, "bonds": nb, "k": args.k, "reps": args.reps, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "sides": [flip, plain],
           "flip_over_plain": {key: flip[key][0] / plain[key][0]
                               for key in ("table_build_ms", "matvec_us", "forms_pair_us", "e0_forward_backward_ms")},
           "faster": {key: faster(key) for key in ("table_build_ms", "matvec_us", "forms_pair_us", "e0_forward_backward_ms")}}
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
