"""Timings of the Hubbard pair kernels on one GPU (docs/design/41-hubbard-pair-ladder.md) against what a user had to do before
them, in one process on one device; kernels alone (C-ABI calls back to back between two events, median (min - max) of the
rounds after a warm-up; `reps` calls of the fused apply and reps / 5 of the forms and of the composition per round), on the
ring of L sites with random weights W (L, L):

    fused apply        k_hubbard_pair<SU, SD>: y = sum_ij W_ij A_{i up} B_{j dn} x, one launch
    fused forms        k_hubbard_pair_forms<SU, SD> + reduce: all L^2 site-pair forms, two launches
    composition        sum_i up-ladder(e_i, down-ladder(W[i, :], x)) through dsea_hubbard_ladder_apply: per up site one down
                       ladder into the intermediate sector, one up ladder with a one-hot weight into the destination and one
                       axpy into y -- 3 L launches, every one of them timed

    L = 12  (6, 6) -> (5, 5)      L = 12  (6, 6) -> (7, 5)      L = 14  (7, 7) -> (6, 6)

THE BAR: the fused apply takes less time than the composition at every size (asserted; the two results are compared before
they are timed).  No ratio is fixed in advance.  Gathers per second counts the mu md source reads of a destination row.

    python tools/kbench_hubbard_pair.py [--reps 100] [--rounds 5] [--out profiles/kbench_hubbard_pair.json]
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
from dominantsparseeigenad_amd.operators import HubbardLadder, HubbardOperator, HubbardPairLadder, ring_bonds  # noqa: E402

F64 = torch.float64
SIZES = ((12, (6, 6), (5, 5)), (12, (6, 6), (7, 5)), (14, (7, 7), (6, 6)))


def timed(fn, reps, rounds):
    """median over `rounds` of the mean of `reps` back-to-back calls, in us (after a warm-up round)"""
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


def row(name, us, **extra):
    med, lo, hi = us
    rec = {"kernel": name, "us": med, "us_min": lo, "us_max": hi}
    rec.update(extra)
    return rec


def sector(L, nup, ndn, dev):
    bonds = ring_bonds(L)
    return HubbardOperator(L, bonds, torch.zeros(2 * len(bonds) + 2 * L, dtype=F64, device=dev), nup, ndn)


def measure(L, src_sec, dst_sec, reps, rounds, dev, gen):
    lib = _lib.load()
    st = _stream(dev)
    su, sd = dst_sec[0] - src_sec[0], dst_sec[1] - src_sec[1]
    src, dst, mid = sector(L, *src_sec, dev), sector(L, *dst_sec, dev), sector(L, src_sec[0], dst_sec[1], dev)
    lad = HubbardPairLadder(src, dst)
    down, up = HubbardLadder(src, mid, "dn"), HubbardLadder(mid, dst, "up")
    W = torch.randn((L, L), dtype=F64, device=dev, generator=gen)
    eye = torch.eye(L, dtype=F64, device=dev)
    x = torch.randn(src.n, dtype=F64, device=dev, generator=gen)
    v1 = torch.randn(dst.n, dtype=F64, device=dev, generator=gen)
    y, yc = torch.empty(dst.n, dtype=F64, device=dev), torch.empty(dst.n, dtype=F64, device=dev)
    tmp, part = torch.empty(mid.n, dtype=F64, device=dev), torch.empty(dst.n, dtype=F64, device=dev)
    cnt = c_int64()
    _lib.check(lib.dsea_hubbard_pair_forms_scratch_doubles(*lad._sector_args(), byref(cnt)), "scratch")
    scratch = torch.empty(cnt.value, dtype=F64, device=dev)
    out = torch.empty((L, L), dtype=F64, device=dev)
    tabs = [_ptr(t) for t in lad._tables]
    dtabs, utabs = [_ptr(t) for t in down._tables], [_ptr(t) for t in up._tables]

    def fused():
        return lib.dsea_hubbard_pair_apply(*lad._sector_args(), _ptr(W), *tabs, _ptr(x), _ptr(y), 0, st)

    def forms():
        return lib.dsea_hubbard_pair_forms(*lad._sector_args(), *tabs, _ptr(v1), _ptr(x), _ptr(out), _ptr(scratch), 0, st)

    def composed():
        rc = 0
        yc.zero_()
        for i in range(L):
            rc |= lib.dsea_hubbard_ladder_apply(*down._sector_args(), _ptr(W[i]), *dtabs, _ptr(x), _ptr(tmp), 0, st)
            rc |= lib.dsea_hubbard_ladder_apply(*up._sector_args(), _ptr(eye[i]), *utabs, _ptr(tmp), _ptr(part), 0, st)
            yc.add_(part)
        return rc

    assert fused() == 0 and forms() == 0 and composed() == 0
    agree = float((y - yc).norm() / yc.norm())
    lin = abs(float(v1 @ y) - float((W * out).sum())) / float(v1.norm() * y.norm())
    assert agree < 1e-12 and lin < 1e-12, (agree, lin)
    tf = timed(fused, reps, rounds)
    tq = timed(forms, max(2, reps // 5), rounds)
    tc = timed(composed, max(2, reps // 5), rounds)
    mu = dst_sec[0] if su > 0 else L - dst_sec[0]
    md = dst_sec[1] if sd > 0 else L - dst_sec[1]
    gathers = dst.n * mu * md
    rows = [row("k_hubbard_pair<%+d, %+d>" % (su, sd), tf, gathers_per_s=gathers / tf[0] * 1e6, launches=1),
            row("k_hubbard_pair_forms<%+d, %+d> + reduce (%d forms)" % (su, sd, L * L), tq, gathers_per_s=gathers / tq[0] * 1e6,
                launches=2),
            row("%d x (down ladder, up ladder, axpy) + zero" % L, tc, launches=3 * L + 1)]
    return {"L": L, "src": list(src_sec), "dst": list(dst_sec), "n_src": src.n, "n_dst": dst.n, "n_mid": mid.n,
            "terms_per_row": mu * md, "agreement": agree, "forms_linearity": lin, "kernels": rows,
            "composition_over_fused": tc[0] / tf[0], "forms_over_fused": tq[0] / tf[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kbench_hubbard_pair.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(dev).manual_seed(1)
    sizes = [measure(L, s, d, args.reps, args.rounds, dev, gen) for L, s, d in SIZES]
    rec = {"reps": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "sizes": sizes,
           "bar_met": all(s["composition_over_fused"] > 1.0 for s in sizes)}
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    assert rec["bar_met"], "the fused apply is not faster than the composition at every size"


if __name__ == "__main__":
    main()
