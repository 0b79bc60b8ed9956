"""Timings of the Hubbard bond current kernels on one GPU (docs/design/39-hubbard-current.md) on the 4 x 4 torus,
square_bonds(4, 4) (32 bonds), L = 16, nup = ndn = 5, n = 4368^2 = 19 079 424; kernels alone (C-ABI calls back to back between
two events), median (min - max) of five rounds, one side of a pair after the other in one process:

    (a) k_hubbard_current<1>                         beside k_spmv_hubbard of the same operator (dsea_spmv without a shift): the
                                                     same table reads and gathers, no diagonal.  Bar: the median of the new kernel
                                                     is not above the mat-vec's median by more than the mat-vec's own min - max
                                                     spread in this run.
    (b) k_hubbard_current<8>                         beside eight R = 1 launches on contiguous columns.  Bar: the slowest block
                                                     round is not slower than the fastest eight-launch round.
    (c) k_hubbard_current_forms + reduce (64 forms)  beside 64 R = 1 applies: reported only.

The script reports whether a bar holds; it does not fail when one does not.  GB/s on ALGORITHMIC bytes: 2 * 8 n R for a map (X
read once, Y written once), 2 * 8 n for the forms.

    python tools/kbench_hubbard_current.py [--Lx 4] [--Ly 4] [--nup 5] [--ndn 5] [--reps 20] [--rounds 5] [--out profiles/kbench_hubbard_current.json]
"""
import argparse
import json
import os
import sys
from ctypes import byref, c_int64

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from dominantsparseeigenad_amd import _lib  # noqa: E402
from dominantsparseeigenad_amd.engine import _ptr, _stream  # noqa: E402
from dominantsparseeigenad_amd.operators import HubbardOperator, square_bonds  # noqa: E402

F64 = torch.float64


def timed(fn, reps, rounds):
    """median over `rounds` of the mean of `reps` back-to-back calls, in us (after a warm-up round)"""
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


def row(name, us, nbytes, **extra):
    med, lo, hi = us
    rec = {"kernel": name, "us": med, "us_min": lo, "us_max": hi, "GBps_algorithmic": nbytes / med / 1e3}
    rec.update(extra)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Lx", type=int, default=4)
    ap.add_argument("--Ly", type=int, default=4)
    ap.add_argument("--nup", type=int, default=5)
    ap.add_argument("--ndn", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda:0")
    L = args.Lx * args.Ly
    nup, ndn = args.nup, args.ndn
    bonds = square_bonds(args.Lx, args.Ly)
    nb = len(bonds)
    st = _stream(dev)
    p = torch.cat([torch.ones(nb, dtype=F64), torch.zeros(nb, dtype=F64), 4.0 * torch.ones(L, dtype=F64),
                   torch.zeros(L, dtype=F64)]).to(dev)                                # t = 1, V = 0, U = 4, eps = 0
    op = HubbardOperator(L, bonds, p, nup, ndn)
    cur = op.current()
    n = op.n
    gen = torch.Generator(dev).manual_seed(1)
    w = torch.randn(2 * nb, dtype=F64, device=dev, generator=gen)
    X = torch.randn((n, 8), dtype=F64, device=dev, generator=gen)
    Y = torch.empty((n, 8), dtype=F64, device=dev)
    cols = X.T.contiguous()                              # eight contiguous columns for the R = 1 launches
    ycols = torch.empty_like(cols)
    x, x2, y = cols[0], cols[1], ycols[0]
    mv_bytes = 2 * 8 * n

    def apply(R, src, dst):
        return lambda: lib.dsea_op_hubbard_current_apply(op.handle, R, _ptr(w), _ptr(src), _ptr(dst), st)

    # the kernels agree with each other before anything is timed: column j of the block is the R = 1 result, bit for bit
    _lib.check(apply(8, X, Y)(), "dsea_op_hubbard_current_apply")
    for j in range(8):
        _lib.check(apply(1, cols[j], ycols[j])(), "dsea_op_hubbard_current_apply")
    torch.cuda.synchronize()
    assert torch.equal(Y.T.contiguous(), ycols)
    assert torch.equal(cur(w.reshape(2, nb), x), ycols[0])
    # (a) the map at R = 1 beside the Hamiltonian's mat-vec
    spmv = lambda: lib.dsea_spmv(op.handle, None, _ptr(x), _ptr(y), None, None, None, st)  # noqa: E731
    ta, tb = timed(apply(1, x, y), args.reps, args.rounds), timed(spmv, args.reps, args.rounds)
    pair_a = [row("k_hubbard_current<1> (%d x %d torus, %d bonds, nup = %d, ndn = %d)" % (args.Lx, args.Ly, nb, nup, ndn), ta,
                  mv_bytes), row("k_spmv_hubbard", tb, mv_bytes)]
    # (b) the block of eight beside eight launches
    def eight():
        for j in range(8):
            lib.dsea_op_hubbard_current_apply(op.handle, 1, _ptr(w), _ptr(cols[j]), _ptr(ycols[j]), st)
    reps2 = max(3, args.reps // 4)
    tc, td = timed(apply(8, X, Y), reps2, args.rounds), timed(eight, reps2, args.rounds)
    pair_b = [row("k_hubbard_current<8>", tc, 8 * mv_bytes), row("8 launches of k_hubbard_current<1>", td, 8 * mv_bytes)]
    # (c) all forms beside 2 nb applies
    cnt = c_int64()
    _lib.check(lib.dsea_op_hubbard_current_forms_scratch_doubles(L, nup, ndn, nb, byref(cnt)), "scratch")
    scratch = torch.empty(cnt.value, dtype=F64, device=dev)
    out = torch.empty(2 * nb, dtype=F64, device=dev)
    forms = lambda: lib.dsea_op_hubbard_current_forms(op.handle, _ptr(x), _ptr(x2), _ptr(out), _ptr(scratch), st)  # noqa: E731
    one = apply(1, x, y)

    def applies():
        for _ in range(2 * nb):
            one()
    reps3 = max(2, args.reps // 10)
    te, tf = timed(forms, reps3, args.rounds), timed(applies, reps3, args.rounds)
    pair_c = [row("k_hubbard_current_forms + reduce (%d forms)" % (2 * nb), te, mv_bytes),
              row("%d launches of k_hubbard_current<1>" % (2 * nb), tf, 2 * nb * mv_bytes)]
    spread = pair_a[1]["us_max"] - pair_a[1]["us_min"]
    rec = {"L": L, "nup": nup, "ndn": ndn, "n": n, "bonds": nb, "reps": args.reps, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0),
           "matvec_pair": pair_a, "matvec_spread_us": spread, "current_over_matvec": pair_a[0]["us"] / pair_a[1]["us"],
           "current_median_within_the_matvec_spread_of_the_matvec_median": pair_a[0]["us"] <= pair_a[1]["us"] + spread,
           "block_pair": pair_b, "eight_launches_over_block": pair_b[1]["us"] / pair_b[0]["us"],
           "slowest_block_round_not_slower_than_fastest_eight_launch_round": pair_b[0]["us_max"] <= pair_b[1]["us_min"],
           "forms_pair": pair_c, "applies_over_forms": pair_c[1]["us"] / pair_c[0]["us"],
           "forms_in_applies": pair_c[0]["us"] / pair_a[0]["us"]}
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
