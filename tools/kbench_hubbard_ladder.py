"""Timings of the Hubbard ladder kernels on one GPU (docs/design/25-hubbard-ladder.md) on the sector of docs/design/19-hubbard.md:
the 4 x 4 torus, L = 16, (nup, ndn) = (5, 5) -> (4, 5) (sum_i w_i c_{i up}) and (5, 5) -> (5, 4) (sum_i w_i c_{i dn}),
n_src = 19 079 424, n_dst = 7 949 760; kernels alone (C-ABI calls back to back between two events, median (min - max) of five
rounds), in one process, per species:

    k_hubbard_ladder<species, -1>                     S(w) x, random weights
    k_hubbard_ladder_forms<species, -1> + reduce      all L site forms
    k_spmv_hubbard of the destination sector          the mat-vec that a spectral function applies k times

REPORTED ONLY, there is no bar: a spectral function applies the ladder once and the Hamiltonian k times.  GB/s on ALGORITHMIC
bytes: 8 n_src (x) + 8 n_dst (y) for the ladder, 8 n_dst (v1) + 8 n_src (v2) for the forms (the state table of the moving species
has C(L, count) words and is not counted), 2 * 8 n_dst for the mat-vec.  They are no share of peak.

    python tools/kbench_hubbard_ladder.py [--Lx 4] [--Ly 4] [--nup 5] [--ndn 5] [--reps 20] [--rounds 5]
                                          [--out profiles/kbench_hubbard_ladder.json]
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
from dominantsparseeigenad_amd.operators import HubbardLadder, HubbardOperator, square_bonds  # noqa: E402

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
    rec = {"kernel": name, "us": med, "us_min": lo, "us_max": hi, "GBps": nbytes / med / 1e3}
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
                   torch.zeros(L, dtype=F64)]).to(dev)                                     # t = 1, U = 4, V = eps = 0
    src = HubbardOperator(L, bonds, p, nup, ndn)
    gen = torch.Generator(dev).manual_seed(1)
    w = torch.randn(L, dtype=F64, device=dev, generator=gen)
    x = torch.randn(src.n, dtype=F64, device=dev, generator=gen)
    reps2 = max(4, args.reps // 5)
    species_rows = []
    for code, species, sector in ((0, "up", (nup - 1, ndn)), (1, "dn", (nup, ndn - 1))):
        dst = HubbardOperator(L, bonds, p, *sector)
        lad = HubbardLadder(src, dst)
        assert (lad.species, lad.step) == (species, -1)
        states, lo_rank, hi_base = lad._tables
        v1 = torch.randn(dst.n, dtype=F64, device=dev, generator=gen)
        y = torch.empty(dst.n, dtype=F64, device=dev)
        y2 = torch.empty(dst.n, dtype=F64, device=dev)
        cnt = c_int64()
        _lib.check(lib.dsea_hubbard_ladder_forms_scratch_doubles(L, nup, ndn, code, -1, byref(cnt)), "scratch")
        scratch = torch.empty(cnt.value, dtype=F64, device=dev)
        out = torch.empty(L, dtype=F64, device=dev)
        apply = lambda: lib.dsea_hubbard_ladder_apply(L, nup, ndn, code, -1, _ptr(w), _ptr(states), _ptr(lo_rank),  # noqa: E731
                                                      _ptr(hi_base), _ptr(x), _ptr(y), 0, st)
        forms = lambda: lib.dsea_hubbard_ladder_forms(L, nup, ndn, code, -1, _ptr(states), _ptr(lo_rank), _ptr(hi_base),  # noqa: E731
                                                      _ptr(v1), _ptr(x), _ptr(out), _ptr(scratch), 0, st)
        spmv = lambda: lib.dsea_spmv(dst.handle, None, _ptr(v1), _ptr(y2), None, None, None, st)  # noqa: E731
        assert apply() == 0 and forms() == 0 and spmv() == 0
        # the two agree with each other before they are timed: v1^T S(w) x = sum_i w_i form_i
        lhs, rhs = float(v1 @ y), float(w @ out)
        agree = abs(lhs - rhs) / float(v1.norm() * y.norm())
        assert agree < 1e-12, agree
        ta = timed(apply, args.reps, args.rounds)
        tf = timed(forms, reps2, args.rounds)
        tm = timed(spmv, args.reps, args.rounds)
        count = nup if species == "up" else ndn
        rows = [row("k_hubbard_ladder<%s, -1> (%d, %d) -> (%d, %d)" % ((species, nup, ndn) + sector), ta, 8 * (dst.n + src.n),
                    gathers_per_row=float(L - count + 1)),
                row("k_hubbard_ladder_forms<%s, -1> + reduce (%d forms)" % (species, L), tf, 8 * (dst.n + src.n)),
                row("k_spmv_hubbard of the destination (%d bonds)" % nb, tm, 2 * 8 * dst.n)]
        species_rows.append({"species": species, "dst": list(sector), "n_dst": dst.n, "agreement": agree, "kernels": rows,
                             "ladder_over_matvec": rows[0]["us"] / rows[2]["us"],
                             "forms_over_matvec": rows[1]["us"] / rows[2]["us"]})
        del dst, lad
    rec = {"L": L, "src": [nup, ndn], "n_src": src.n, "bonds": nb, "reps": args.reps, "forms_reps": reps2, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "species": species_rows}
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
