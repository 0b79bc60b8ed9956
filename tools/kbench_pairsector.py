"""Timings of the all-pair sector kernels on one GPU (docs/design/22-pair-sector.md): L = 24, ndown = 12, n = 2 704 156, all
276 pairs with Heisenberg power-law couplings Jxy_ij = Jz_ij = 1 / |i - j|^alpha, alpha = 3.  The other side of each pair is the
only way to do the same without the new kind: three ``SpinSectorOperator``s of 92 bonds each on one table set.  One process,
kernels alone (calls back to back between two events, median (min - max) of five rounds after a warm-up, one side after the
other):

    a. k_spmv_pairsector                                        beside three k_spmv_sector calls and the two vector adds;
    b. k_pairsector_forms + k_pairsector_gram + two reduces     beside three k_sector_forms + reduce passes;
    c. one ``correlations(psi)`` call (forms, scratch allocation and the torch indexing), reported only.

The two sides are first checked against each other at 1e-13.  Bar of a and b (the one of docs/design/16 .. 21): the slowest
round of the new kernel is not slower than the fastest round of the composition.  The script reports whether it holds; it does
not fail when it does not.  GB/s on ALGORITHMIC bytes: 8 n (states) + 2 * 8 n (x read once, y written once) for the mat-vec,
8 n + 2 * 8 n for the forms (states, v1, v2 read once) -- the gathers, ndown (L - ndown) per row, are not counted.

    python tools/kbench_pairsector.py [--L 24] [--alpha 3.0] [--reps 20] [--rounds 5] [--out profiles/kbench_pairsector.json]
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
from dominantsparseeigenad_amd.operators import SpinSectorOperator, SpinSectorPairOperator, power_law_couplings  # noqa: E402

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
    ap.add_argument("--L", type=int, default=24)
    ap.add_argument("--alpha", type=float, default=3.0)
    ap.add_argument("--parts", type=int, default=3, help="bond-list operators the pairs are split over")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = _stream(dev)
    L, ndown = args.L, args.L // 2
    pair = SpinSectorPairOperator(L, None, ndown, dev)
    P, n = pair.npair, pair.n
    M = power_law_couplings(L, torch.tensor(args.alpha, dtype=F64, device=dev))
    pair.couplings = pair.pack(M, M, 0.0)
    jxy, jz, hz = pair.unpack(pair.couplings)
    # the composition: `parts` bond-list operators on the pair operator's tables, the field on the first
    size = (P + args.parts - 1) // args.parts
    assert size <= _lib.LATTICE_MAX_BONDS
    parts, slices = [], []
    for k in range(args.parts):
        sl = slice(k * size, min(P, (k + 1) * size))
        bonds = pair.pairs[sl]
        c = torch.cat([jxy[sl], jz[sl], hz if k == 0 else torch.zeros_like(hz)]).contiguous()
        op = SpinSectorOperator(L, bonds, c, ndown, dev)
        op._tables = pair._tables
        op.couplings = c                                 # a new handle, on the shared tables
        parts.append(op)
        slices.append(sl)
    gen = torch.Generator(dev).manual_seed(1)
    x = torch.randn(n, dtype=F64, device=dev, generator=gen)
    x2 = torch.randn(n, dtype=F64, device=dev, generator=gen)
    y = torch.empty(n, dtype=F64, device=dev)
    ys = [torch.empty(n, dtype=F64, device=dev) for _ in parts]
    mv_bytes = 3 * 8 * n
    gathers = ndown * (L - ndown)

    def new_mv():
        lib.dsea_spmv(pair.handle, None, _ptr(x), _ptr(y), None, None, None, st)

    def old_mv():
        for op, yk in zip(parts, ys):
            lib.dsea_spmv(op.handle, None, _ptr(x), _ptr(yk), None, None, None, st)
        for yk in ys[1:]:
            ys[0].add_(yk)

    new_mv()
    old_mv()
    agree_mv = float((y - ys[0]).norm() / ys[0].norm())
    assert agree_mv < 1e-13, agree_mv
    ta = timed(new_mv, args.reps, args.rounds)
    tb = timed(old_mv, args.reps, args.rounds)
    pair_a = [row("k_spmv_pairsector (%d pairs)" % P, ta, mv_bytes, gathers_per_row=gathers),
              row("%d x k_spmv_sector (%d bonds each) + %d vector adds" % (len(parts), size, len(parts) - 1), tb,
                  len(parts) * mv_bytes + (len(parts) - 1) * mv_bytes, agreement=agree_mv)]
    # b. the forms
    cnt = c_int64()
    _lib.check(lib.dsea_op_pairsector_forms_scratch_doubles(L, ndown, byref(cnt)), "scratch")
    scratch = torch.empty(cnt.value, dtype=F64, device=dev)
    out = torch.empty(2 * P + L, dtype=F64, device=dev)
    olds = []
    for op in parts:
        _lib.check(lib.dsea_op_sector_forms_scratch_doubles(L, ndown, op.nb, byref(cnt)), "scratch")
        olds.append((op, torch.empty(cnt.value, dtype=F64, device=dev), torch.empty(op.nparam, dtype=F64, device=dev)))

    def new_forms():
        lib.dsea_op_pairsector_forms(pair.handle, _ptr(x), _ptr(x2), _ptr(out), _ptr(scratch), st)

    def old_forms():
        for op, s, o in olds:
            lib.dsea_op_sector_forms(op.handle, _ptr(x), _ptr(x2), _ptr(o), _ptr(s), st)

    new_forms()
    old_forms()
    theirs = torch.cat([o[:op.nb] for op, _, o in olds] + [o[op.nb:2 * op.nb] for op, _, o in olds] + [olds[0][2][2 * olds[0][0].nb:]])
    agree_forms = float((out - theirs).abs().max() / (x.norm() * x2.norm()))
    assert agree_forms < 1e-13, agree_forms
    reps2 = max(3, args.reps // 4)
    tc = timed(new_forms, reps2, args.rounds)
    td = timed(old_forms, reps2, args.rounds)
    pair_b = [row("k_pairsector_forms + k_pairsector_gram + 2 reduces (%d forms)" % (2 * P + L), tc, 2 * mv_bytes),
              row("%d x (k_sector_forms + reduce)" % len(parts), td, len(parts) * mv_bytes, agreement=agree_forms)]
    # c. one correlations call
    psi = x / x.norm()
    te = timed(lambda: pair.correlations(psi), reps2, args.rounds)
    rec = {"L": L, "ndown": ndown, "n": n, "pairs": P, "alpha": args.alpha, "reps": args.reps, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0),
           "matvec_pair": pair_a,
           "matvec_slowest_new_round_not_slower_than_fastest_composition_round": pair_a[0]["us_max"] <= pair_a[1]["us_min"],
           "matvec_composition_over_new": pair_a[1]["us"] / pair_a[0]["us"],
           "forms_pair": pair_b,
           "forms_slowest_new_round_not_slower_than_fastest_composition_round": pair_b[0]["us_max"] <= pair_b[1]["us_min"],
           "forms_composition_over_new": pair_b[1]["us"] / pair_b[0]["us"],
           "correlations_call_us": {"us": te[0], "us_min": te[1], "us_max": te[2]}}
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
