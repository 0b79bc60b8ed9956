"""Timings of the block Hubbard mat-vec and of one basis-free block Lanczos step on one GPU
(docs/design/28-hubbard-finite-temperature.md) on the case of docs/design/19-hubbard.md: the 4 x 4 torus, square_bonds(4, 4) (32
bonds), L = 16, t = 1, U = 4, V = eps = 0, at nup = ndn = 5 (n = 4368^2 = 19 079 424) and at nup = ndn = 4 (n = 1820^2 =
3 312 400); kernels alone (calls back to back between two events, at least --reps of them and at least 200 ms per round; median,
fastest and slowest of five rounds):

    R2, R4, R8    k_spmv_hubbard_block<R> on an [n, R] block   beside R calls of the single-vector mat-vec on R vectors, in
                                                               the same process, after checking that the two agree bit for bit;
    lanczos       one step of dsea_op_hubbard_block_lanczos at R = 8 (three launches; a run of --k steps divided by k, so the
                  two launches of the start are spread over the steps)   beside the R = 8 block mat-vec alone.  Reported only.

Bar, in the form of notes 16, 18 and 27: the slowest R = 8 block round is not slower than the fastest round of eight single
mat-vecs, at both fillings.  The script reports whether it holds and the ratio for every R; it does not fail when it does not.
GB/s on ALGORITHMIC bytes: 8 n + 2 * 8 n R for a block (X read once, Y written once), R * 2 * 8 n for R single mat-vecs (the
count of note 19.6).

Without --step every step of every filling runs in a process of its own under its own time limit, one after the other, and the
first one that fails ends the run; the results are merged into --out.

    python tools/kbench_hubbard_block.py [--Lx 4] [--Ly 4] [--fillings 5 4] [--reps 50] [--rounds 5] [--k 20]
                                         [--out profiles/kbench_hubbard_block.json]
    python tools/kbench_hubbard_block.py --step R8 --fillings 5
"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

STEPS = ("R2", "R4", "R8", "lanczos")
STEP_SECONDS = 240
WINDOW_MS = 200.0


def timed(fn, reps, rounds):
    """median, fastest and slowest over `rounds` of the mean of back-to-back calls, in us (after a warm-up): `reps` calls per
    round, or as many more as it takes to fill WINDOW_MS -- a shorter window measures the clock and the scheduler as much as
    the kernel"""
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(3):
        fn()
    b.record()
    torch.cuda.synchronize()
    reps = max(reps, int(math.ceil(WINDOW_MS / max(a.elapsed_time(b) / 3.0, 1e-3))))
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
    return out[len(out) // 2], out[0], out[-1], reps


def row(name, us, nbytes, **extra):
    med, lo, hi, reps = us
    rec = {"kernel": name, "us": med, "us_min": lo, "us_max": hi, "calls_per_round": reps, "GBps": nbytes / med / 1e3}
    rec.update(extra)
    return rec


def run_step(args):
    import torch
    from ctypes import byref, c_int64
    from dominantsparseeigenad_amd import _lib
    from dominantsparseeigenad_amd.engine import _ptr, _stream
    from dominantsparseeigenad_amd.operators import HubbardOperator, square_bonds
    F64 = torch.float64
    lib = _lib.load()
    dev = torch.device("cuda:0")
    L = args.Lx * args.Ly
    nup = ndn = args.fillings[0]
    bonds = square_bonds(args.Lx, args.Ly)
    nb = len(bonds)
    st = _stream(dev)
    p = torch.cat([torch.ones(nb, dtype=F64), torch.zeros(nb, dtype=F64), 4.0 * torch.ones(L, dtype=F64),
                   torch.zeros(L, dtype=F64)]).to(dev)                                # t = 1, V = 0, U = 4, eps = 0
    op = HubbardOperator(L, bonds, p, nup, ndn)
    n = op.n
    gen = torch.Generator(dev).manual_seed(1)
    R = 8 if args.step == "lanczos" else int(args.step[1:])
    X = torch.randn((n, R), dtype=F64, device=dev, generator=gen)
    Y = torch.empty_like(X)
    block_bytes = 8 * n + 2 * 8 * n * R
    block = lambda: lib.dsea_op_hubbard_block_apply(op.handle, R, _ptr(X), _ptr(Y), st)  # noqa: E731
    rec = {"step": args.step, "L": L, "nup": nup, "ndn": ndn, "n": n, "bonds": nb, "R": R, "reps": args.reps,
           "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    if args.step == "lanczos":
        need = c_int64()
        _lib.check(lib.dsea_op_hubbard_block_lanczos_scratch_doubles(L, nup, ndn, R, byref(need)), "scratch")
        scratch = torch.empty(need.value, dtype=F64, device=dev)
        Q, W = X.clone(), torch.empty_like(X)
        norm2 = torch.empty(R, dtype=F64, device=dev)
        alphas, betas = torch.empty((args.k, R), dtype=F64, device=dev), torch.empty((args.k, R), dtype=F64, device=dev)
        steps = torch.empty(R, dtype=torch.int32, device=dev)
        run = lambda: lib.dsea_op_hubbard_block_lanczos(op.handle, R, args.k, _ptr(Q), _ptr(W), _ptr(norm2), _ptr(alphas),  # noqa: E731
                                                        _ptr(betas), _ptr(steps), _ptr(scratch), st)
        assert run() == 0
        torch.cuda.synchronize()
        assert steps.tolist() == [args.k] * R and bool(torch.isfinite(alphas).all()) and bool(torch.isfinite(betas).all())
        reps = max(2, args.reps // 10)
        t_run = timed(run, reps, args.rounds)
        per_step = tuple(t / args.k for t in t_run[:3]) + (t_run[3],)
        t_block = timed(block, args.reps, args.rounds)
        # per step: the mat-vec (Q read, W read and written), the update (Q, W read, W written), the finish (W read and written)
        step_bytes = 8 * n + 8 * 8 * n * R
        rec["pair"] = [row("one block Lanczos step, R = %d (run of %d steps / %d)" % (R, args.k, args.k), per_step, step_bytes),
                       row("k_spmv_hubbard_block<%d> alone" % R, t_block, block_bytes)]
        rec["step_over_block_matvec"] = per_step[0] / t_block[0]
        return rec
    xs = [X[:, j].contiguous() for j in range(R)]
    ys = [torch.empty(n, dtype=F64, device=dev) for _ in range(R)]

    def singles():
        for j in range(R):
            lib.dsea_spmv(op.handle, None, _ptr(xs[j]), _ptr(ys[j]), None, None, None, st)
    assert block() == 0
    singles()
    torch.cuda.synchronize()
    assert all(torch.equal(Y[:, j], ys[j]) for j in range(R)), "the block columns are not the single-vector results"
    ta, tb = timed(block, args.reps, args.rounds), timed(singles, args.reps, args.rounds)
    rec["pair"] = [row("k_spmv_hubbard_block<%d>" % R, ta, block_bytes),
                   row("%d calls of the single-vector mat-vec" % R, tb, R * 2 * 8 * n)]
    rec["slowest_block_round_not_slower_than_fastest_round_of_singles"] = ta[2] <= tb[1]
    rec["singles_over_block"] = tb[0] / ta[0]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Lx", type=int, default=4)
    ap.add_argument("--Ly", type=int, default=4)
    ap.add_argument("--fillings", type=int, nargs="+", default=[5, 4], help="nup = ndn of every case")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--k", type=int, default=20, help="steps of the timed Lanczos run")
    ap.add_argument("--step", choices=STEPS, default=None, help="run this one step (first filling) in this process")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        print(json.dumps(run_step(args)))
        return 0
    cases = []
    for fill in args.fillings:
        records = []
        for step in STEPS:   # every GPU step: a fresh process under its own time limit; the first failure ends the run
            cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", step, "--Lx",
                   str(args.Lx), "--Ly", str(args.Ly), "--fillings", str(fill), "--reps", str(args.reps), "--rounds",
                   str(args.rounds), "--k", str(args.k)]
            done = subprocess.run(cmd, capture_output=True, text=True)
            if done.returncode != 0:
                sys.stderr.write(done.stdout + done.stderr)
                sys.stderr.write("step %s at filling %d ended with status %d: nothing more is started\n"
                                 % (step, fill, done.returncode))
                return done.returncode
            records.append(json.loads(done.stdout.strip().splitlines()[-1]))
            print("filling %d, %s: %s" % (fill, step, json.dumps(records[-1]["pair"])), flush=True)
        by = {r["step"]: r for r in records}
        case = {key: by["R8"][key] for key in ("L", "nup", "ndn", "n", "bonds", "reps", "rounds", "device")}
        case["steps"] = records
        case["singles_over_block"] = {s: by[s]["singles_over_block"] for s in ("R2", "R4", "R8")}
        case["bar_R8_slowest_block_round_not_slower_than_fastest_round_of_eight_singles"] = \
            by["R8"]["slowest_block_round_not_slower_than_fastest_round_of_singles"]
        cases.append(case)
    rec = {"cases": cases,
           "bar_holds_at_every_filling": all(c["bar_R8_slowest_block_round_not_slower_than_fastest_round_of_eight_singles"]
                                             for c in cases)}
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
