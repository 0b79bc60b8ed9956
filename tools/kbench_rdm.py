"""Timings of the reduced-density-matrix kernels on one GPU (docs/design/21-reduced-density-matrix.md) on a normalised random
vector of the sector L = 24, ndown = 12, n = 2 704 156, for two bipartitions:

    (a) A = sites 0 .. 11   13 blocks, dA_m = dB_m = C(12, m) up to 924: sum_m 2 dA_m^2 dB_m = 4.1e9 flops for the full products
    (b) A = [0, 1]          3 blocks, dA = 1, 2, 1 and dB = 646 646, 705 432, 646 646: a tall-skinny reduction

For each: k_rdm_cross + k_rdm_cross_reduce with x = y (the reduced density matrix: tiles on or below the diagonal only) and with
x != y, at both tile edges, and k_rdm_pull -- calls back to back between two events, median (min - max) of five rounds after a
warm-up round.  Beside each, the torch composition on the same index table, one side of the pair after the other:
``x[idx]``, then one ``torch.matmul`` per block (forward), and ``y[idx]``, one matmul per block, one ``index_copy`` (backward).
The index build is timed too.

Bar of workload (a): the slowest round of the hand-written forward (x = y, the library's tile) is not slower than the fastest
round of the torch composition.  The script reports whether it holds; it does not fail when it does not.  TF/s counts the flops
of the FULL products 2 dA^2 dB on both sides (the symmetric kernel executes about half of them).  GB/s on ALGORITHMIC bytes:
forward 4 n (idx) + 8 n (x) [+ 8 n (y)] + 8 out_len; backward 4 n + 8 n (y) + 8 n (out) + 8 out_len.

    python tools/kbench_rdm.py [--L 24] [--reps 20] [--rounds 5] [--out profiles/kbench_rdm.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from dominantsparseeigenad_amd.operators import Bipartition  # noqa: E402

F64 = torch.float64
FP64_PEAK_TF = 78.6      # AMD's public MI355X data sheet, fp64 vector = matrix; the microarchitecture guide used here gives none


def timed(fn, reps, rounds):
    """median, min, max over `rounds` of the mean of `reps` back-to-back calls, in us (after a warm-up round)"""
    for _ in range(max(2, reps // 4)):
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


def row(name, us, nbytes, flops=None, **extra):
    med, lo, hi = us
    rec = {"kernel": name, "us": med, "us_min": lo, "us_max": hi, "GBps": nbytes / med / 1e3}
    if flops is not None:
        rec["TFps_full_products"] = flops / med / 1e6
        rec["fraction_of_fp64_peak"] = rec["TFps_full_products"] / FP64_PEAK_TF
    rec.update(extra)
    return rec


def workload(name, L, ndown, sites, reps, rounds, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    Bipartition(L, sites, ndown=ndown, device=dev)       # (warm-up: library load, first launch)
    torch.cuda.synchronize()
    a.record()
    part = Bipartition(L, sites, ndown=ndown, device=dev)
    b.record()
    torch.cuda.synchronize()
    build_us = a.elapsed_time(b) * 1e3                    # the rank tables of the sector and the index table
    n, out_len = part.n, part.out_len
    gen = torch.Generator(dev).manual_seed(1)
    x = torch.randn(n, dtype=F64, device=dev, generator=gen)
    x = x / x.norm()
    y = torch.randn(n, dtype=F64, device=dev, generator=gen)
    G = torch.randn(out_len, dtype=F64, device=dev, generator=gen)
    idx = part.idx.to(torch.int64)
    flops = float(sum(2 * dA * dA * dB for _, dA, dB in part.blocks))
    offs = part._idx_off

    def slices(v):
        g = v[idx]
        return [g[o:o + dA * dB].view(dA, dB) for o, (_, dA, dB) in zip(offs, part.blocks)]

    def torch_cross(u, v):
        return [p @ q.T for p, q in zip(slices(u), slices(v))]

    def torch_rdm():
        s = slices(x)
        return [p @ p.T for p in s]

    def torch_pull():
        out = torch.empty(n, dtype=F64, device=dev)
        parts = [g @ s for g, s in zip(part.views(G), slices(y))]
        return out.index_copy_(0, idx, torch.cat([p.reshape(-1) for p in parts]))

    want = torch.cat([t.reshape(-1) for t in torch_rdm()])
    agree_f = float((part._cross_raw(x, x) - want).norm() / want.norm())
    want = torch_pull()
    agree_b = float((part._pull_raw(G, y, False) - want).norm() / want.norm())
    assert agree_f < 1e-12 and agree_b < 1e-12, (agree_f, agree_b)
    fwd_bytes = 4 * n + 8 * n + 8 * out_len
    rows = []
    for tile in (0, 1, 2):
        part.set_tile(tile)
        label = {0: "library's tile", 1: "tile 16", 2: "tile 32"}[tile]
        rows.append(row("k_rdm_cross + reduce, x = y, %s" % label, timed(lambda: part._cross_raw(x, x), reps, rounds), fwd_bytes,
                        flops, tile=tile, symmetric=True))
        if tile:
            rows.append(row("k_rdm_cross + reduce, x != y, %s" % label, timed(lambda: part._cross_raw(x, y), reps, rounds),
                            fwd_bytes + 8 * n, flops, tile=tile, symmetric=False))
    part.set_tile(0)
    rows.append(row("torch: x[idx], one matmul per block (M M^T)", timed(torch_rdm, reps, rounds), fwd_bytes, flops,
                    launches=1 + len(part.blocks), temporaries_bytes=8 * n))
    rows.append(row("torch: x[idx], y[idx], one matmul per block", timed(lambda: torch_cross(x, y), reps, rounds),
                    fwd_bytes + 8 * n, flops, temporaries_bytes=16 * n))
    bwd_bytes = 4 * n + 16 * n + 8 * out_len
    rows.append(row("k_rdm_pull", timed(lambda: part._pull_raw(G, y, False), reps, rounds), bwd_bytes, flops))
    rows.append(row("k_rdm_pull, transposed", timed(lambda: part._pull_raw(G, y, True), reps, rounds), bwd_bytes, flops))
    rows.append(row("torch: y[idx], one matmul per block, index_copy", timed(torch_pull, reps, rounds), bwd_bytes, flops,
                    temporaries_bytes=16 * n))
    ours, theirs = rows[0], [r for r in rows if r["kernel"].startswith("torch: x[idx], one")][0]
    return {"workload": name, "sites": list(sites), "n": n, "out_len": out_len, "blocks": [list(b) for b in part.blocks],
            "flops_full_products": flops, "scratch_bytes": 8 * part._scratch_doubles, "index_bytes": 4 * n,
            "build_us_tables_and_index": build_us, "agreement_forward": agree_f, "agreement_backward": agree_b, "rows": rows,
            "slowest_forward_round_not_slower_than_fastest_torch_round": ours["us_max"] <= theirs["us_min"],
            "torch_over_forward": theirs["us"] / ours["us"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L, ndown = args.L, args.L // 2
    rec = {"L": L, "ndown": ndown, "reps": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "fp64_peak_TF_assumed": FP64_PEAK_TF,
           "a": workload("(a) A = sites 0 .. %d" % (L // 2 - 1), L, ndown, list(range(L // 2)), args.reps, args.rounds, dev),
           "b": workload("(b) A = [0, 1]", L, ndown, [0, 1], args.reps, args.rounds, dev)}
    rec["bar_a_holds"] = rec["a"]["slowest_forward_round_not_slower_than_fastest_torch_round"]
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
