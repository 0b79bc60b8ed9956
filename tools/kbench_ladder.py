"""Timings of the sector ladder kernels on one GPU (docs/design/24-dynamics.md) on the sector of docs/design/18-spin-sector.md:
the 4 x 6 torus, L = 24, ndown 12 -> 13 (n_src = 2 704 156, n_dst = 2 496 144); kernels alone (C-ABI calls back to back between
two events, median (min - max) of five rounds), in one process:

    k_sector_ladder<+1>                        sigma^-(c) x, random weights
    k_sector_ladder_forms<+1> + reduce         all L site forms
    k_spmv_sector of the destination sector    the Heisenberg mat-vec that a spectral function applies k times
    k_sector_ladder<-1>, <0> and k_sector_ladder_forms<-1>, <0> + reduce: the transposed ladder 13 -> 12 and Z(c) on ndown 12
    (docs/design/38-ladder-parts.md), each checked against its forms like the first pair

REPORTED ONLY, there is no bar: a spectral function applies the ladder once and the Hamiltonian k times.  GB/s on ALGORITHMIC
bytes: 8 n_dst (states) + 8 n_src (x) + 8 n_dst (y) for the ladder, 8 n_dst + 8 n_dst + 8 n_src for the forms, 3 * 8 n_dst for
the mat-vec.

    python tools/kbench_ladder.py [--Lx 4] [--Ly 6] [--reps 50] [--rounds 5] [--out profiles/kbench_ladder.json]
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
from dominantsparseeigenad_amd.operators import SpinSectorLadder, SpinSectorOperator, square_bonds  # noqa: E402

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
    ap.add_argument("--Ly", type=int, default=6)
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
    p = torch.cat([torch.ones(2 * nb, dtype=F64, device=dev), torch.zeros(L, dtype=F64, device=dev)])   # Jxy = Jz = 1, no field
    src = SpinSectorOperator(L, bonds, p, ndown)
    dst = SpinSectorOperator(L, bonds, p, ndown + 1)
    lad = SpinSectorLadder(src, dst)
    states, lo_rank, hi_base = lad._tables
    gen = torch.Generator(dev).manual_seed(1)
    c = torch.randn(L, dtype=F64, device=dev, generator=gen)
    x = torch.randn(src.n, dtype=F64, device=dev, generator=gen)
    v1 = torch.randn(dst.n, dtype=F64, device=dev, generator=gen)
    y = torch.empty(dst.n, dtype=F64, device=dev)
    y2 = torch.empty(dst.n, dtype=F64, device=dev)
    cnt = c_int64()
    _lib.check(lib.dsea_sector_ladder_forms_scratch_doubles(L, ndown, 1, byref(cnt)), "scratch")
    scratch = torch.empty(cnt.value, dtype=F64, device=dev)
    out = torch.empty(L, dtype=F64, device=dev)
    apply = lambda: lib.dsea_sector_ladder_apply(L, ndown, 1, _ptr(c), _ptr(states), _ptr(lo_rank), _ptr(hi_base), _ptr(x),  # noqa: E731
                                                 _ptr(y), 0, st)
    forms = lambda: lib.dsea_sector_ladder_forms(L, ndown, 1, _ptr(states), _ptr(lo_rank), _ptr(hi_base), _ptr(v1), _ptr(x),  # noqa: E731
                                                 _ptr(out), _ptr(scratch), 0, st)
    spmv = lambda: lib.dsea_spmv(dst.handle, None, _ptr(v1), _ptr(y2), None, None, None, st)  # noqa: E731
    assert apply() == 0 and forms() == 0 and spmv() == 0
    # the three agree with each other before they are timed: v1^T S(c) x = sum_i c_i form_i
    lhs, rhs = float(v1 @ y), float(c @ out)
    agree = abs(lhs - rhs) / float(v1.norm() * y.norm())
    assert agree < 1e-12, agree
    reps2 = max(5, args.reps // 5)
    ta = timed(apply, args.reps, args.rounds)
    tf = timed(forms, reps2, args.rounds)
    tm = timed(spmv, args.reps, args.rounds)
    rows = [row("k_sector_ladder<+1> (ndown %d -> %d)" % (ndown, ndown + 1), ta, 8 * (2 * dst.n + src.n),
                gathers_per_row=float(ndown + 1)),
            row("k_sector_ladder_forms<+1> + reduce (%d forms)" % L, tf, 8 * (2 * dst.n + src.n)),
            row("k_spmv_sector of the destination (%d bonds)" % nb, tm, 3 * 8 * dst.n)]
    # the other two steps on the same tables: sigma^+(c) back from ndown + 1, and Z(c) within ndown
    for step, a, b in ((-1, dst, src), (0, src, src)):
        other = lad.T if step < 0 else SpinSectorLadder(src, src)
        tabs = [_ptr(t) for t in other._tables]
        _lib.check(lib.dsea_sector_ladder_forms_scratch_doubles(L, a.ndown, step, byref(cnt)), "scratch")
        assert cnt.value <= scratch.numel()
        xs = torch.randn(a.n, dtype=F64, device=dev, generator=gen)
        vs = torch.randn(b.n, dtype=F64, device=dev, generator=gen)
        ys = torch.empty(b.n, dtype=F64, device=dev)
        apply_s = lambda: lib.dsea_sector_ladder_apply(L, a.ndown, step, _ptr(c), *tabs, _ptr(xs), _ptr(ys), 0, st)  # noqa: E731
        forms_s = lambda: lib.dsea_sector_ladder_forms(L, a.ndown, step, *tabs, _ptr(vs), _ptr(xs), _ptr(out), _ptr(scratch),  # noqa: E731
                                                       0, st)
        assert apply_s() == 0 and forms_s() == 0
        agree_s = abs(float(vs @ ys) - float(c @ out)) / float(vs.norm() * ys.norm())
        assert agree_s < 1e-12, (step, agree_s)
        rows.append(row("k_sector_ladder<%+d> (ndown %d -> %d)" % (step, a.ndown, b.ndown), timed(apply_s, args.reps, args.rounds),
                        8 * (2 * b.n + a.n)))
        rows.append(row("k_sector_ladder_forms<%+d> + reduce (%d forms)" % (step, L), timed(forms_s, reps2, args.rounds),
                        8 * (2 * b.n + a.n)))
    rec = {"L": L, "ndown_src": ndown, "ndown_dst": ndown + 1, "n_src": src.n, "n_dst": dst.n, "bonds": nb, "reps": args.reps,
           "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "agreement": agree, "kernels": rows,
           "ladder_over_matvec": rows[0]["us"] / rows[2]["us"], "forms_over_matvec": rows[1]["us"] / rows[2]["us"]}
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
