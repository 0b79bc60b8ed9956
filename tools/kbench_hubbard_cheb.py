"""Timings of one order of the Hubbard Chebyshev kernels on one GPU (docs/design/34-hubbard-chebyshev.md) on the case of
tools/kbench_hubbard_block.py: the 4 x 4 torus, square_bonds(4, 4) (32 bonds), L = 16, t = 1, U = 4, V = eps = 0, nup = ndn = 5
(n = 4368^2 = 19 079 424; --filling 4 gives n = 3 312 400 where the memory for X, Y, U, V, two accumulators and the temporaries
of the torch path does not allow 5), R = 8; kernels alone (runs back to back between two events, median, fastest and slowest of
five rounds of ten runs after a warm-up), one process per mode:

    A1            one FUSED order of the propagator: a run of dsea_op_hubbard_block_chebyshev with one accumulator over 20 orders
                  divided by 20 -- k_cheb_hubbard_block<8, 1>;
    self, left    one FUSED order of the moments: a run of dsea_op_hubbard_block_moments over 20 orders (M = 40 in self mode,
                  M = 21 with a left block) divided by 20 -- k_cheb_hubbard_moments<8, LEFT> and the one-block
                  k_cheb_moments_finish<8> per order;

each beside one UNFUSED order, what the library could do for this operator before these kernels: ``apply_block``
(k_spmv_hubbard_block<8, false>) and the tail as torch elementwise operations in the order of ``chebyshev._apply_unfused`` and
``chebyshev._moments_unfused``, with the accumulator update (A1) or the two column sums (self, left) of every order; and beside
20 calls of k_spmv_hubbard_block<8, false> alone divided by 20, so that the cost of the tail on this row walk can be read off.

Before the timing the fused result is compared with the unfused one: the propagator bit for bit, the moments within 1e-12
||l|| ||x||.  Bar, in the form of notes 16, 18, 27, 31 and 33: the slowest fused round is not slower than the fastest unfused
round, in each of the three modes.  The script reports whether it holds and the ratios; it does not fail when it does not.  The
ratio to the bare mat-vec is reported, not barred.  No share of peak is claimed: there are no counters here.

Without --step every step runs in a process of its own under its own time limit, one after the other, and the first one that
fails ends the run; the results are merged into --out.

    python tools/kbench_hubbard_cheb.py [--filling 5] [--reps 10] [--rounds 5] [--out profiles/kbench_hubbard_cheb.json]
    python tools/kbench_hubbard_cheb.py --step left
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

STEPS = ("A1", "self", "left")
STEP_SECONDS = 420
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
    from dominantsparseeigenad_amd import _lib
    from dominantsparseeigenad_amd.engine import _ptr, _stream
    from dominantsparseeigenad_amd.operators import HubbardOperator, square_bonds
    F64 = torch.float64
    lib = _lib.load()
    dev = torch.device("cuda:0")
    L = args.Lx * args.Ly
    nup = ndn = args.filling
    bonds = square_bonds(args.Lx, args.Ly)
    nb = len(bonds)
    st = _stream(dev)
    p = torch.cat([torch.ones(nb, dtype=F64), torch.zeros(nb, dtype=F64), 4.0 * torch.ones(L, dtype=F64),
                   torch.zeros(L, dtype=F64)]).to(dev)                                # t = 1, V = 0, U = 4, eps = 0
    op = HubbardOperator(L, bonds, p, nup, ndn)
    n = op.n
    B = float(2 * nb + 4 * L)                                # 2 |t| per bond, |U| per site: the rigorous bound
    centre, h = 0.0, B
    left = args.step == "left"
    gen = torch.Generator(dev).manual_seed(1)
    X = torch.randn((n, R), dtype=F64, device=dev, generator=gen)
    Y = torch.randn((n, R), dtype=F64, device=dev, generator=gen) if left else None
    U, V, W = torch.empty_like(X), torch.empty_like(X), torch.empty_like(X)
    bare_once = lambda: lib.dsea_op_hubbard_block_apply(op.handle, R, _ptr(X), _ptr(W), st)  # noqa: E731

    def bare():
        for _ in range(ORDERS):
            bare_once()

    rec = {"step": args.step, "L": L, "nup": nup, "ndn": ndn, "n": n, "bonds": nb, "R": R, "orders_per_run": ORDERS,
           "reps": max(2, args.reps), "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    if args.step == "A1":
        M = ORDERS + 1
        c = [0.5 + 0.01 * m for m in range(M)]
        coeffs = (c_double * M)(*c)
        ACC = torch.empty_like(X)
        fused = lambda: lib.dsea_op_hubbard_block_chebyshev(op.handle, R, 1, M, centre, h, coeffs, _ptr(X), _ptr(U), _ptr(V),  # noqa: E731
                                                            _ptr(ACC), st)
        kept = {}

        def unfused():                                       # chebyshev._apply_unfused with one coefficient row
            x, old = X, None
            for m in range(1, M):
                t = ((1.0 if m == 1 else 2.0) / h) * (op.apply_block(x) - centre * x)
                if m == 1:
                    acc = c[0] * x + c[1] * t
                else:
                    t = t - old
                    acc = acc + c[m] * t
                old, x = x, t
            kept["acc"] = acc

        assert fused() == 0
        unfused()
        torch.cuda.synchronize()
        assert torch.equal(ACC, kept["acc"]), "the fused propagator does not return the bits of the unfused path"
        rec["fused_equals_unfused_bit_for_bit"] = True
        names = ("one fused order: k_cheb_hubbard_block<8, 1>",
                 "one unfused order: k_spmv_hubbard_block<8, false> + the torch tail with one accumulator")
    else:
        M = ORDERS + 1 if left else 2 * ORDERS
        need = c_int64()
        _lib.check(lib.dsea_op_hubbard_block_moments_scratch_doubles(L, nup, ndn, R, byref(need)), "scratch")
        scratch = torch.empty(need.value, dtype=F64, device=dev)
        MU = torch.empty((M, R), dtype=F64, device=dev)
        fused = lambda: lib.dsea_op_hubbard_block_moments(op.handle, R, M, centre, h, _ptr(X), _ptr(Y) if left else None, _ptr(U),  # noqa: E731
                                                          _ptr(V), _ptr(MU), _ptr(scratch), st)
        mu = torch.empty((M, R), dtype=F64, device=dev)

        def unfused():                                       # chebyshev._moments_unfused without its read-back
            x, old = X, None
            for m in range(1, ORDERS + 1):
                t = ((1.0 if m == 1 else 2.0) / h) * (op.apply_block(x) - centre * x)
                if m > 1:
                    t = t - old
                l = Y if left else x
                a, b = (l * x).sum(0), (l * t).sum(0)
                if m == 1:
                    mu[0], mu[1] = a, b
                elif left:
                    mu[m] = b
                else:
                    mu[2 * m - 2] = 2.0 * a - mu[0]
                    mu[2 * m - 1] = 2.0 * b - mu[1]
                old, x = x, t

        assert fused() == 0
        unfused()
        torch.cuda.synchronize()
        deviation = float((MU - mu).abs().max() / (X.norm(dim=0) * (Y if left else X).norm(dim=0)).max())
        assert deviation <= 1e-12, deviation
        rec["fused_minus_unfused_moments"] = deviation
        names = ("one fused order: k_cheb_hubbard_moments<8, %s> + k_cheb_moments_finish<8>" % ("true" if left else "false"),
                 "one unfused order: k_spmv_hubbard_block<8, false> + the torch tail + 2 torch column sums")
    reps = max(2, args.reps)
    tf, tu, tb = timed(fused, reps, args.rounds), timed(unfused, reps, args.rounds), timed(bare, reps, args.rounds)
    rec["rows"] = [row(names[0], tf), row(names[1], tu), row("k_spmv_hubbard_block<8, false> alone", tb)]
    rec["slowest_fused_round_not_slower_than_fastest_unfused_round"] = tf[2] <= tu[1]
    rec["unfused_over_fused"] = tu[0] / tf[0]
    rec["fused_over_bare_matvec"] = tf[0] / tb[0]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Lx", type=int, default=4)
    ap.add_argument("--Ly", type=int, default=4)
    ap.add_argument("--filling", type=int, default=5, help="nup = ndn")
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
               str(args.Lx), "--Ly", str(args.Ly), "--filling", str(args.filling), "--reps", str(args.reps), "--rounds",
               str(args.rounds)]
        done = subprocess.run(cmd, capture_output=True, text=True)
        if done.returncode != 0:
            sys.stderr.write(done.stdout + done.stderr)
            sys.stderr.write("step %s ended with status %d: nothing more is started\n" % (step, done.returncode))
            return done.returncode
        records.append(json.loads(done.stdout.strip().splitlines()[-1]))
        print("%s: %s" % (step, json.dumps(records[-1]["rows"])), flush=True)
    rec = {key: records[0][key] for key in ("L", "nup", "ndn", "n", "bonds", "R", "orders_per_run", "reps", "rounds", "device")}
    rec["steps"] = records
    rec["unfused_over_fused"] = {r["step"]: r["unfused_over_fused"] for r in records}
    rec["fused_over_bare_matvec"] = {r["step"]: r["fused_over_bare_matvec"] for r in records}
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
