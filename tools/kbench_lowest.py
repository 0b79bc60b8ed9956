"""Timings of the lowest-nev eigenpair path on one GPU (docs/design/13-lowest-eigenpairs.md):

    * dsea_ritz_combine_block at n = 2^20, k = 200, m = 1, 2, 4, 8 (bytes = (k + m) 8 n) beside dsea_ritz_combine;
    * deflated CG us per iteration against the streaming dsea_cg_run at TFIM L = 20, m = 1, 2, 4 (fixed iteration count);
    * LowestSparseSymeig forward + backward at L = 20, k = 200, nev = 2 beside DominantSparseSymeig.

    python tools/kbench_lowest.py [--reps 20] [--out profiles/kbench_lowest.json]
"""
import argparse
import json
import os
import sys
import time
from ctypes import byref, c_double, c_int64

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples", "TFIM"))

from dominantsparseeigenad_amd import _lib, engine  # noqa: E402
from dominantsparseeigenad_amd.engine import Workspace, _ptr, _stream  # noqa: E402

F64 = torch.float64


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps        # us


def ritz_rows(reps):
    lib = _lib.load()
    dev = torch.device("cuda:0")
    n, k = 1 << 20, 200
    ldq = engine.round_up(n, 32)
    Q = torch.randn(k, ldq, dtype=F64, device=dev)
    ws = Workspace.get(n, k, dev)
    st = _stream(dev)
    rows = []
    s = torch.randn(k, dtype=F64, device=dev)
    out = torch.empty(n, dtype=F64, device=dev)
    us = timed(lambda: lib.dsea_ritz_combine(ws.handle, _ptr(Q), ldq, n, k, _ptr(s), _ptr(out), st), reps)
    rows.append({"kernel": "dsea_ritz_combine", "n": n, "k": k, "m": 1, "us": us, "GBps": (k + 1) * 8 * n / us / 1e3})
    for m in (1, 2, 4, 8):
        S = torch.randn(m, k, dtype=F64, device=dev)
        Y = torch.empty(m, n, dtype=F64, device=dev)
        us = timed(lambda: lib.dsea_ritz_combine_block(ws.handle, _ptr(Q), ldq, n, k, _ptr(S), k, m, _ptr(Y), n, st), reps)
        rows.append({"kernel": "dsea_ritz_combine_block", "n": n, "k": k, "m": m, "us": us,
                     "GBps": (k + m) * 8 * n / us / 1e3})
    return rows


def cg_rows(iters):
    """fixed iteration count (eps = 0: the stop never fires): us per iteration, the entry / poll cost included"""
    lib = _lib.load()
    from dominantsparseeigenad_amd.operators import TFIMOperator
    dev = torch.device("cuda:0")
    L = 20
    n = 1 << L
    op = TFIMOperator(L, dev, g=torch.tensor([1.0], dtype=F64, device=dev))
    b = torch.randn(n, dtype=F64, device=dev)
    shift = torch.tensor([-30.0], dtype=F64, device=dev)
    rows = []
    ws = Workspace.get(n, 9, dev)
    st = _stream(dev)
    it, res = c_int64(0), c_double(0.0)
    prev = ws.persist_mode
    ws.set_persist(0)                          # the streaming form: the one the deflated CG generalises
    try:
        def run_plain():
            x = torch.zeros(n, dtype=F64, device=dev)
            lib.dsea_cg_run(op.handle, ws.handle, _ptr(shift), _ptr(b), _ptr(x), _ptr(ws.state), 0.0, iters, 16,
                            byref(it), byref(res), st)
        run_plain()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_plain()
        torch.cuda.synchronize()
        base = (time.perf_counter() - t0) * 1e6 / iters
        rows.append({"solver": "dsea_cg_run (streaming)", "L": L, "m": 0, "us_per_iter": base, "ratio": 1.0})
    finally:
        ws.set_persist(prev)
    for m in (1, 2, 4):
        Psi = torch.linalg.qr(torch.randn(n, m, dtype=F64, device=dev))[0].T.contiguous()

        def run_dfl():
            x = torch.zeros(n, dtype=F64, device=dev)
            lib.dsea_cg_run_deflated(op.handle, ws.handle, _ptr(shift), _ptr(b), _ptr(x), _ptr(Psi), n, m, _ptr(ws.state),
                                     0.0, iters, 16, byref(it), byref(res), st)
        run_dfl()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_dfl()
        torch.cuda.synchronize()
        us = (time.perf_counter() - t0) * 1e6 / iters
        rows.append({"solver": "dsea_cg_run_deflated", "L": L, "m": m, "us_per_iter": us, "ratio": us / base})
    return rows


def primitive_rows(reps):
    import dominantsparseeigenad_amd.symeig as symeig
    from TFIM import TFIM
    dev = torch.device("cuda:0")
    L, k = 20, 200
    model = TFIM(L, dev)
    u = torch.randn(model.dim, dtype=F64, device=dev, generator=torch.Generator(dev).manual_seed(1))
    rows = []
    for name in ("DominantSparseSymeig", "LowestSparseSymeig nev=2"):
        times = []
        for _ in range(reps + 1):
            model.g = torch.tensor([1.5], dtype=F64, device=dev, requires_grad=True)
            torch.manual_seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name.startswith("Dominant"):
                symeig.setDominantSparseSymeig(model.H, model.Hadjoint_to_gadjoint)
                e0, psi = symeig.DominantSparseSymeig.apply(model.g, k, model.dim)
                loss = e0 + (psi @ u) ** 2
            else:
                symeig.setLowestSparseSymeig(model.H, model.Hadjoint_to_gadjoint)
                vals, vecs = symeig.LowestSparseSymeig.apply(model.g, k, model.dim, 2)
                loss = vals[1] - vals[0] + (vecs[:, 1] @ u) ** 2
            loss.backward()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        times = sorted(times[1:])
        rows.append({"primitive": name, "L": L, "k": k, "loss": "levels + (psi_j . u)^2, u random",
                     "ms_fwd_bwd_median": times[len(times) // 2], "cg_iters_last_solve": engine.last_cg.iters})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cg-iters", type=int, default=400)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rec = {"ritz_combine_block": ritz_rows(args.reps), "deflated_cg": cg_rows(args.cg_iters),
           "primitives": primitive_rows(max(3, args.reps // 4)), "device": torch.cuda.get_device_name(0)}
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
