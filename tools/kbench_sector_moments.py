"""Timings of one order of the Chebyshev moments on one GPU (docs/design/33-chebyshev-moments.md) on the case of
docs/design/27-finite-temperature.md and 31-chebyshev-propagator.md: the 4 x 6 torus, square_bonds(4, 6) (48 bonds), Heisenberg
couplings, L = 24, ndown = 12, n = 2 704 156, R = 8; kernels alone (calls back to back between two events, median, fastest and
slowest of five rounds after a warm-up), one process per mode:

    self, left    one FUSED order: a run of dsea_op_sector_block_moments over 20 orders (M = 40 in self mode, M = 21 with a left
                  block) divided by 20 -- k_cheb_sector_moments<8, LEFT> and the one-block k_cheb_moments_finish<8> per order;
                  beside one UNFUSED order, what the library could do before this kernel: a run of
                  dsea_op_sector_block_chebyshev with one accumulator over the same 20 orders (k_cheb_sector_block<8, 1>) plus,
                  per order, the column sums (A * B).sum(0) of torch -- two in self mode, three with a left block -- divided by
                  20; and beside k_cheb_sector_block<8, 1> alone, so that the cost of the reductions can be read off.

Before the timing the fused moments are compared with ``chebyshev_moments(..., fused=False)``.  Bar, in the form of notes 16, 18,
27 and 31: the slowest fused round is not slower than the fastest unfused round, in both modes.  The script reports whether it
holds and the ratios; it does not fail when it does not.  No share of peak is claimed: there are no counters here.

Without --step every step runs in a process of its own under its own time limit, one after the other, and the first one that
fails ends the run; the results are merged into --out.

    python tools/kbench_sector_moments.py [--Lx 4] [--Ly 6] [--reps 10] [--rounds 5] [--out profiles/kbench_sector_moments.json]
    python tools/kbench_sector_moments.py --step left
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

STEPS = ("self", "left")
STEP_SECONDS = 240
ORDERS = 20
R = 8


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


def row(name, us):
    med, lo, hi = (t / ORDERS for t in us)
    return {"kernel": name, "us": med, "us_min": lo, "us_max": hi}


def run_step(args):
    import torch
    from ctypes import byref, c_double, c_int64
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
    n = op.n
    left = args.step == "left"
    gen = torch.Generator(dev).manual_seed(1)
    X = torch.randn((n, R), dtype=F64, device=dev, generator=gen)
    Y = torch.randn((n, R), dtype=F64, device=dev, generator=gen) if left else None
    U, V, ACC = torch.empty_like(X), torch.empty_like(X), torch.empty_like(X)
    B = float(3 * nb)                                        # 2 |Jxy| + |Jz| per bond: the rigorous bound
    M = ORDERS + 1 if left else 2 * ORDERS
    need = c_int64()
    _lib.check(lib.dsea_op_sector_block_moments_scratch_doubles(L, ndown, R, byref(need)), "scratch")
    scratch = torch.empty(need.value, dtype=F64, device=dev)
    MU = torch.empty((M, R), dtype=F64, device=dev)
    coeffs = (c_double * (ORDERS + 1))(*([0.5] * (ORDERS + 1)))
    fused = lambda: lib.dsea_op_sector_block_moments(op.handle, R, M, 0.0, B, _ptr(X), _ptr(Y) if left else None, _ptr(U),  # noqa: E731
                                                     _ptr(V), _ptr(MU), _ptr(scratch), st)
    cheb = lambda: lib.dsea_op_sector_block_chebyshev(op.handle, R, 1, ORDERS + 1, 0.0, B, coeffs, _ptr(X), _ptr(U), _ptr(V),  # noqa: E731
                                                      _ptr(ACC), st)
    dots = [(X, U), (U, V)] if not left else [(Y, U), (Y, V), (X, U)]

    def unfused():
        cheb()
        for _ in range(ORDERS):
            for a, b in dots:
                (a * b).sum(0)

    assert fused() == 0 and cheb() == 0
    torch.cuda.synchronize()
    want = chebyshev.chebyshev_moments(op, X, M, (-B, B), left=Y, fused=False)
    deviation = float((MU.cpu() - want).abs().max() / (X.norm(dim=0) * (Y if left else X).norm(dim=0)).max().cpu())
    assert deviation <= 1e-12, deviation
    reps = max(2, args.reps)
    tf, tu, tc = timed(fused, reps, args.rounds), timed(unfused, reps, args.rounds), timed(cheb, reps, args.rounds)
    return {"step": args.step, "L": L, "ndown": ndown, "n": n, "bonds": nb, "R": R, "orders_per_run": ORDERS, "reps": reps,
            "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "fused_minus_unfused_moments": deviation,
            "rows": [row("one fused order: k_cheb_sector_moments<8, %s> + k_cheb_moments_finish<8>" % ("true" if left else "false"), tf),
                     row("one unfused order: k_cheb_sector_block<8, 1> + %d torch column sums" % len(dots), tu),
                     row("k_cheb_sector_block<8, 1> alone", tc)],
            "slowest_fused_round_not_slower_than_fastest_unfused_round": tf[2] <= tu[1],
            "unfused_over_fused": tu[0] / tf[0], "fused_over_cheb_alone": tf[0] / tc[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Lx", type=int, default=4)
    ap.add_argument("--Ly", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10, help="runs of 20 orders per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step", choices=STEPS, default=None, help="run this one step in this process and print its record")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        print(json.dumps(run_step(args)))
        return 0
    records = []
    for step in STEPS:       # every GPU step: a fresh process under its own time limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", step, "--Lx",
               str(args.Lx), "--Ly", str(args.Ly), "--reps", str(args.reps), "--rounds", str(args.rounds)]
        done = subprocess.run(cmd, capture_output=True, text=True)
        if done.returncode != 0:
            sys.stderr.write(done.stdout + done.stderr)
            sys.stderr.write("step %s ended with status %d: nothing more is started\n" % (step, done.returncode))
            return done.returncode
        records.append(json.loads(done.stdout.strip().splitlines()[-1]))
    rec = {key: records[0][key] for key in ("L", "ndown", "n", "bonds", "R", "orders_per_run", "reps", "rounds", "device")}
    rec["steps"] = records
    rec["unfused_over_fused"] = {r["step"]: r["unfused_over_fused"] for r in records}
    rec["fused_over_cheb_alone"] = {r["step"]: r["fused_over_cheb_alone"] for r in records}
    rec["bar_slowest_fused_round_not_slower_than_fastest_unfused_round"] = \
        {r["step"]: r["slowest_fused_round_not_slower_than_fastest_unfused_round"] for r in records}
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
