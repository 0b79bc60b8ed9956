"""Timings of one order of the Chebyshev block propagator on one GPU (docs/design/31-chebyshev-propagator.md) on the case of
notes 18.6 and 27.6: the 4 x 6 torus, square_bonds(4, 6) (48 bonds), Heisenberg couplings, L = 24, ndown = 12, n = 2 704 156,
R = 8; kernels alone (calls back to back between two events, median, fastest and slowest of five rounds after a warm-up):

    A1, A2    one order of k_cheb_sector_block<8, A> (a run of --orders launches of dsea_op_sector_block_chebyshev divided by
              their number; the first of them is the `first` form)
              beside the same order as it could be computed before: one k_spmv_sector_block<8> and the tail as separate torch
              elementwise kernels into preallocated blocks (u = w - centre x, t = g u, t -= old, acc_a += c_a t),
              beside the plain block mat-vec alone, in the same process, after checking that ``chebyshev_apply`` returns the same
              bits fused and unfused.

Bar, in the form of notes 16, 18 and 27: the slowest fused round is not slower than the fastest unfused round.  The script
reports whether it holds; it does not fail when it does not.  The order moves 8 n R (1 + 2 A) bytes more than the mat-vec: `old`
read, and every accumulator read and written.

Without --step every step runs in a process of its own under its own time limit, one after the other, and the first one that
fails ends the run; the results are merged into --out.

    python tools/kbench_sector_cheb.py [--Lx 4] [--Ly 6] [--reps 10] [--rounds 5] [--orders 20] [--out profiles/kbench_sector_cheb.json]
    python tools/kbench_sector_cheb.py --step A2
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

STEPS = ("A1", "A2")
STEP_SECONDS = 240


def timed(fn, reps, rounds):
    """median, fastest and slowest over `rounds` of the mean of `reps` back-to-back calls, in us (after a warm-up)"""
    import torch
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


def row(name, us, nbytes):
    med, lo, hi = us
    return {"kernel": name, "us": med, "us_min": lo, "us_max": hi, "GBps": nbytes / med / 1e3}


def run_step(args):
    import numpy as np
    import torch
    from ctypes import c_double
    from dominantsparseeigenad_amd import _lib, chebyshev
    from dominantsparseeigenad_amd.engine import _ptr, _stream
    from dominantsparseeigenad_amd.operators import SpinSectorOperator, square_bonds
    F64 = torch.float64
    lib = _lib.load()
    dev = torch.device("cuda:0")
    L = args.Lx * args.Ly
    ndown = L // 2
    bonds = square_bonds(args.Lx, args.Ly)
    nb = len(bonds)
    st = _stream(dev)
    p = torch.cat([torch.ones(2 * nb, dtype=F64, device=dev), torch.zeros(L, dtype=F64, device=dev)])   # Jxy = Jz = 1, no field
    op = SpinSectorOperator(L, bonds, p, ndown)
    n, R, A, K = op.n, 8, int(args.step[1:]), args.orders
    B = chebyshev.coupling_bound(op)
    centre, h = 0.0, B
    gen = torch.Generator(dev).manual_seed(1)
    X = torch.randn((n, R), dtype=F64, device=dev, generator=gen)
    check = np.cos(np.arange(A * 4, dtype=np.float64) + 1.0).reshape(A, 4)
    assert torch.equal(chebyshev.chebyshev_apply(op, X, check, (-B, B), fused=True),
                       chebyshev.chebyshev_apply(op, X, check, (-B, B), fused=False)), "fused and unfused bits differ"
    U, V, W, T = (torch.empty_like(X) for _ in range(4))
    ACC = torch.zeros((A, n, R), dtype=F64, device=dev)
    M = K + 1
    c = np.cos(np.arange(A * M, dtype=np.float64) + 1.0) / M
    host = (c_double * (A * M))(*c.tolist())
    fused = lambda: lib.dsea_op_sector_block_chebyshev(op.handle, R, A, M, centre, h, host, _ptr(X), _ptr(U), _ptr(V),  # noqa: E731
                                                       _ptr(ACC), st)
    block = lambda: lib.dsea_op_sector_block_apply(op.handle, R, _ptr(X), _ptr(W), st)  # noqa: E731
    g, old = 2.0 / h, U.copy_(X)

    def unfused():                                    # one order, not the first: x = X, old = U, acc read and written
        lib.dsea_op_sector_block_apply(op.handle, R, _ptr(X), _ptr(W), st)
        torch.mul(X, centre, out=T)
        torch.sub(W, T, out=W)
        torch.mul(W, g, out=W)
        torch.sub(W, old, out=V)
        for a in range(A):
            torch.mul(V, float(c[a * M + 2]), out=T)
            ACC[a].add_(T)

    assert fused() == 0 and block() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ACC).all())
    t_run = timed(fused, max(1, args.reps // 2), args.rounds)
    t_fused = tuple(t / K for t in t_run)
    U.copy_(X)
    t_unfused = timed(unfused, args.reps, args.rounds)
    t_block = timed(block, args.reps, args.rounds)
    block_bytes = 8 * n + 2 * 8 * n * R
    order_bytes = block_bytes + 8 * n * R * (1 + 2 * A)
    return {"step": args.step, "L": L, "ndown": ndown, "n": n, "bonds": nb, "R": R, "A": A, "orders": K, "reps": args.reps,
            "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
            "rows": [row("one order of k_cheb_sector_block<%d, %d> (run of %d / %d)" % (R, A, K, K), t_fused, order_bytes),
                     row("one order unfused: k_spmv_sector_block<%d> and %d elementwise kernels" % (R, 4 + 2 * A), t_unfused,
                         order_bytes),
                     row("k_spmv_sector_block<%d> alone" % R, t_block, block_bytes)],
            "slowest_fused_round_not_slower_than_fastest_unfused_round": t_fused[2] <= t_unfused[1],
            "unfused_over_fused": t_unfused[0] / t_fused[0],
            "fused_order_minus_block_matvec_us": t_fused[0] - t_block[0],
            "extra_bytes_per_order": 8 * n * R * (1 + 2 * A)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Lx", type=int, default=4)
    ap.add_argument("--Ly", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--orders", type=int, default=20, help="launches of the timed fused run")
    ap.add_argument("--step", choices=STEPS, default=None, help="run this one step in this process and print its record")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        print(json.dumps(run_step(args)))
        return 0
    records = []
    for step in STEPS:       # every GPU step: a fresh process under its own time limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", step, "--Lx",
               str(args.Lx), "--Ly", str(args.Ly), "--reps", str(args.reps), "--rounds", str(args.rounds), "--orders",
               str(args.orders)]
        done = subprocess.run(cmd, capture_output=True, text=True)
        if done.returncode != 0:
            sys.stderr.write(done.stdout + done.stderr)
            sys.stderr.write("step %s ended with status %d: nothing more is started\n" % (step, done.returncode))
            return done.returncode
        records.append(json.loads(done.stdout.strip().splitlines()[-1]))
    rec = {key: records[0][key] for key in ("L", "ndown", "n", "bonds", "R", "orders", "reps", "rounds", "device")}
    rec["steps"] = records
    rec["bar_slowest_fused_round_not_slower_than_fastest_unfused_round"] = {
        r["step"]: r["slowest_fused_round_not_slower_than_fastest_unfused_round"] for r in records}
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
