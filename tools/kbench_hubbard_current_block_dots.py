#!/usr/bin/env python3
"""Kernel-alone timings of the column dots of the Hubbard bond current map (docs/design/40-finite-temperature-conductivity.md) on
the 4 x 4 torus (L = 16, 32 bonds), sector nup = ndn = 5 (n = 19 079 424), R = 8 -- the shape of tools/kbench_hubbard_current.py:

    fused     k_hubbard_current_block_dots<8> + k_hubbard_current_forms_reduce (dsea_op_hubbard_current_block_dots)
    unfused   k_hubbard_current<8> (dsea_op_hubbard_current_apply) + the torch product and column sum (Lft * Y).sum(0)
    map       k_hubbard_current<8> alone

Bar: the slowest fused round is not slower than the fastest unfused round.  The ratio of the fused call to the map alone is
reported.  Kernels alone: back-to-back calls between two events, median (min - max) of `rounds` rounds after a warm-up, all
sides one after the other in one process; before anything is timed the fused dots are checked against the unfused ones.
No share of any peak is claimed: no counters are taken here.

    python tools/kbench_hubbard_current_block_dots.py [--Lx 4] [--Ly 4] [--nup 5] [--ndn 5] [--reps 5] [--rounds 5] [--out profiles/kbench_hubbard_current_block_dots.json]
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
    """median, min and max over `rounds` of the mean of `reps` back-to-back calls, in us (after a warm-up round)"""
    for _ in range(2):
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


def row(name, us):
    return {"kernel": name, "us": us[0], "us_min": us[1], "us_max": us[2]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Lx", type=int, default=4)
    ap.add_argument("--Ly", type=int, default=4)
    ap.add_argument("--nup", type=int, default=5)
    ap.add_argument("--ndn", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda:0")
    L, R = args.Lx * args.Ly, 8
    nup, ndn = args.nup, args.ndn
    bonds = square_bonds(args.Lx, args.Ly)
    nb = len(bonds)
    st = _stream(dev)
    p = torch.cat([torch.ones(nb, dtype=F64), torch.zeros(nb, dtype=F64), 4.0 * torch.ones(L, dtype=F64),
                   torch.zeros(L, dtype=F64)]).to(dev)                                # t = 1, V = 0, U = 4, eps = 0
    op = HubbardOperator(L, bonds, p, nup, ndn)
    n = op.n
    gen = torch.Generator(dev).manual_seed(1)
    w = torch.randn(2 * nb, dtype=F64, device=dev, generator=gen)
    X = torch.randn((n, R), dtype=F64, device=dev, generator=gen)
    Lft = torch.randn((n, R), dtype=F64, device=dev, generator=gen)
    Y = torch.empty((n, R), dtype=F64, device=dev)
    cnt = c_int64()
    _lib.check(lib.dsea_op_hubbard_current_block_dots_scratch_doubles(L, nup, ndn, R, byref(cnt)), "scratch")
    scratch = torch.empty(cnt.value, dtype=F64, device=dev)
    out = torch.empty(R, dtype=F64, device=dev)

    fused = lambda: lib.dsea_op_hubbard_current_block_dots(op.handle, R, _ptr(w), _ptr(Lft), _ptr(X), _ptr(out), _ptr(scratch), st)  # noqa: E731
    apply = lambda: lib.dsea_op_hubbard_current_apply(op.handle, R, _ptr(w), _ptr(X), _ptr(Y), st)  # noqa: E731

    def unfused():
        apply()
        return (Lft * Y).sum(0)

    # fused against unfused before anything is timed: the same rows of K X, another order of the column sums
    _lib.check(fused(), "dsea_op_hubbard_current_block_dots")
    want = unfused()
    torch.cuda.synchronize()
    scale = torch.linalg.vector_norm(Lft, dim=0) * torch.linalg.vector_norm(Y, dim=0)
    deviation = float(((out - want).abs() / scale).max())
    assert deviation <= 1e-13, deviation
    tf, tu, tm = timed(fused, args.reps, args.rounds), timed(unfused, args.reps, args.rounds), timed(apply, args.reps, args.rounds)
    rec = {"L": L, "nup": nup, "ndn": ndn, "n": n, "bonds": nb, "R": R, "reps": args.reps, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "fused_against_unfused_relative": deviation,
           "fused": row("k_hubbard_current_block_dots<8> + k_hubbard_current_forms_reduce", tf),
           "unfused": row("k_hubbard_current<8> + torch (Lft * Y).sum(0)", tu),
           "map": row("k_hubbard_current<8>", tm),
           "unfused_over_fused": tu[0] / tf[0], "fused_over_map": tf[0] / tm[0],
           "slowest_fused_round_not_slower_than_fastest_unfused_round": tf[2] <= tu[1]}
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
