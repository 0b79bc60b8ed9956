"""Timings of the block Hubbard ladder kernels on one GPU (docs/design/37-hubbard-finite-temperature-dynamics.md): L = 14,
(nup, ndn) = (7, 7) -> (8, 7) (c+ of the up species, n_src = 11 778 624, n_dst = 10 306 296) and (7, 7) -> (7, 7) (n of the up
species), R = 8, random weights; kernels alone (C-ABI calls back to back between two events, median (min - max) of five rounds of
ten runs after a warm-up), in one process.  Each fused result is checked against the unfused one before anything is timed.

    the block map       k_hubbard_ladder_block<0, STEP, 8>, one launch
      against           eight k_hubbard_ladder<0, STEP> launches on contiguous columns (what the parent can do; the column copies
                        in and out are NOT counted)
    the dots            k_hubbard_ladder_block_dots<0, STEP, 8> + k_hubbard_ladder_forms_reduce
      against           k_hubbard_ladder_block<0, STEP, 8> + the torch product and column sum

THE BAR, per case: the slowest fused round is not slower than the fastest round of the unfused form.  GB/s on ALGORITHMIC bytes:
64 n_src (X) + 64 n_dst (Y or Lft); the state words are one per 3432 rows.

    python tools/kbench_hubbard_ladder_block.py [--L 14] [--reps 10] [--rounds 5] [--out profiles/kbench_hubbard_ladder_block.json]
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
from dominantsparseeigenad_amd.operators import HubbardLadder, HubbardOperator, ring_bonds  # noqa: E402

F64 = torch.float64
R = 8


def timed(fn, reps, rounds):
    """(median, min, max) over `rounds` of the mean of `reps` back-to-back calls, in us, after a warm-up round"""
    for _ in range(reps):
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


def row(name, us, nbytes=None):
    med, lo, hi = us
    rec = {"kernel": name, "us": med, "us_min": lo, "us_max": hi}
    if nbytes is not None:
        rec["GBps"] = nbytes / med / 1e3
    return rec


def case(lib, dev, L, nup, ndn, step, reps, rounds):
    st = _stream(dev)
    bonds = ring_bonds(L)
    zero = torch.zeros(2 * len(bonds) + 2 * L, dtype=F64, device=dev)           # (zero couplings: only the tables are used)
    src = HubbardOperator(L, bonds, zero, nup, ndn, dev)
    dst = src if step == 0 else HubbardOperator(L, bonds, zero, nup + step, ndn, dev)
    lad = HubbardLadder(src, dst, "up")
    states, lo_rank, hi_base = lad._tables
    n_src, n_dst = lad.n_src, lad.n_dst
    sector = lad._sector_args()
    gen = torch.Generator(dev).manual_seed(1)
    c = torch.randn(L, dtype=F64, device=dev, generator=gen)
    X = torch.randn((n_src, R), dtype=F64, device=dev, generator=gen)
    Lft = torch.randn((n_dst, R), dtype=F64, device=dev, generator=gen)
    Y = torch.empty((n_dst, R), dtype=F64, device=dev)
    Xc, Yc = X.t().contiguous(), torch.empty((R, n_dst), dtype=F64, device=dev)
    out = torch.empty(R, dtype=F64, device=dev)
    cnt = c_int64()
    _lib.check(lib.dsea_hubbard_ladder_block_dots_scratch_doubles(*sector, R, byref(cnt)), "scratch")
    scratch = torch.empty(cnt.value, dtype=F64, device=dev)
    tabs = (_ptr(c), _ptr(states), _ptr(lo_rank), _ptr(hi_base))

    def block():
        return lib.dsea_hubbard_ladder_block_apply(*sector, R, *tabs, _ptr(X), _ptr(Y), 0, st)

    def columns():
        rc = 0
        for j in range(R):
            rc |= lib.dsea_hubbard_ladder_apply(*sector, *tabs, _ptr(Xc[j]), _ptr(Yc[j]), 0, st)
        return rc

    def dots():
        return lib.dsea_hubbard_ladder_block_dots(*sector, R, *tabs, _ptr(Lft), _ptr(X), _ptr(out), _ptr(scratch), 0, st)

    def dots_unfused():
        rc = block()
        torch.sum(Lft * Y, dim=0, out=unfused)
        return rc

    unfused = torch.empty(R, dtype=F64, device=dev)
    assert block() == 0 and columns() == 0 and dots() == 0 and dots_unfused() == 0
    torch.cuda.synchronize()
    assert torch.equal(Y, Yc.t()), "the block map differs from eight single-vector maps"
    scale = torch.linalg.vector_norm(Lft, dim=0) * torch.linalg.vector_norm(Y, dim=0)
    agree = float(((out - unfused).abs() / scale).max())
    assert agree < 1e-13, agree
    t_block = timed(block, reps, rounds)
    t_cols = timed(columns, reps, rounds)
    t_dots = timed(dots, reps, rounds)
    t_unf = timed(dots_unfused, reps, rounds)
    nbytes = 8 * R * (n_src + n_dst)
    return {"src": [nup, ndn], "dst": [nup + step, ndn], "species": "up", "step": step, "n_src": n_src, "n_dst": n_dst,
            "dots_agreement": agree,
            "kernels": [row("k_hubbard_ladder_block<0, %+d, 8>" % step, t_block, nbytes),
                        row("8 x k_hubbard_ladder<0, %+d> on contiguous columns" % step, t_cols),
                        row("k_hubbard_ladder_block_dots<0, %+d, 8> + reduce" % step, t_dots, nbytes),
                        row("k_hubbard_ladder_block<0, %+d, 8> + torch product and column sum" % step, t_unf)],
            "block_speedup": t_cols[0] / t_block[0], "dots_speedup": t_unf[0] / t_dots[0],
            "block_bar_met": t_block[2] <= t_cols[1], "dots_bar_met": t_dots[2] <= t_unf[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=14)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda:0")
    half = args.L // 2
    rec = {"L": args.L, "R": R, "reps": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "cases": [case(lib, dev, args.L, half, half, step, args.reps, args.rounds) for step in (1, 0)]}
    rec["bar_met"] = all(c["block_bar_met"] and c["dots_bar_met"] for c in rec["cases"])
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
