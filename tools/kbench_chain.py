"""Timings of the matrix-free XYZ spin-chain kernels on one GPU at L = 20 (docs/design/14-spin-chain.md), each pair in the
same process, kernels alone (dsea_spmv / dsea_op_chain_forms calls back to back between two events):

    1. k_spmv_chain with TFIM couplings                beside k_spmv_tfim;
    2. k_spmv_chain with all five families non-zero    beside the to_csr() operand of the same Hamiltonian (default layout);
    3. k_chain_forms (all 5 L forms, both stages)      beside L calls of the mat-vec.

GB/s on ALGORITHMIC bytes: 2 * 8 n for a mat-vec (x read once, y written once), 2 * 8 n for the forms (v1, v2 read once).

    python tools/kbench_chain.py [--L 20] [--reps 50] [--rounds 5] [--out profiles/kbench_chain.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from dominantsparseeigenad_amd import _lib  # noqa: E402
from dominantsparseeigenad_amd.engine import _ptr, _stream  # noqa: E402
from dominantsparseeigenad_amd.operators import SpinChainOperator, TFIMOperator  # noqa: E402

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
    ap.add_argument("--L", type=int, default=20)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda:0")
    L, n = args.L, 1 << args.L
    st = _stream(dev)
    gen = torch.Generator(dev).manual_seed(1)
    x = torch.randn(n, dtype=F64, device=dev, generator=gen)
    x2 = torch.randn(n, dtype=F64, device=dev, generator=gen)
    y = torch.empty(n, dtype=F64, device=dev)
    mv_bytes = 2 * 8 * n

    def spmv(handle):
        return lambda: lib.dsea_spmv(handle, None, _ptr(x), _ptr(y), None, None, None, st)

    # 1. TFIM couplings beside the TFIM kernel
    tfim = TFIMOperator(L, dev, g=torch.tensor([1.0], dtype=F64, device=dev))
    chain_tfim = SpinChainOperator.tfim(L, 1.0, dev)
    pair1 = [row("k_spmv_tfim", timed(spmv(tfim.handle), args.reps, args.rounds), mv_bytes),
             row("k_spmv_chain (TFIM couplings)", timed(spmv(chain_tfim.handle), args.reps, args.rounds), mv_bytes)]
    # 2. all five families beside the explicit matrix of the same Hamiltonian
    c = torch.randn((5, L), dtype=F64, device=dev, generator=gen)
    chain = SpinChainOperator(L, c)
    csr = chain.to_csr()
    check = float((chain(x) - csr(x)).norm() / chain(x).norm())
    pair2 = [row("k_spmv_chain (five families)", timed(spmv(chain.handle), args.reps, args.rounds), mv_bytes),
             row("to_csr() operand, default layout", timed(spmv(csr.handle), args.reps, args.rounds), mv_bytes,
                 nnz=csr.nnz, coded=bool(getattr(csr, "_coded", False)), col16=bool(csr.col16), agreement=check)]
    # 3. the forms beside L mat-vecs
    from ctypes import byref, c_int64
    cnt = c_int64()
    _lib.check(lib.dsea_op_chain_forms_scratch_doubles(L, byref(cnt)), "scratch")
    scratch = torch.empty(cnt.value, dtype=F64, device=dev)
    out = torch.empty((5, L), dtype=F64, device=dev)
    forms = lambda: lib.dsea_op_chain_forms(chain.handle, _ptr(x), _ptr(x2), _ptr(out), _ptr(scratch), st)  # noqa: E731
    mv = spmv(chain.handle)

    def l_matvecs():
        for _ in range(L):
            mv()
    reps3 = max(5, args.reps // 5)
    pair3 = [row("k_chain_forms + reduce (5 L forms)", timed(forms, reps3, args.rounds), mv_bytes),
             row("L calls of k_spmv_chain", timed(l_matvecs, reps3, args.rounds), L * mv_bytes)]
    rec = {"L": L, "n": n, "reps": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "tfim_pair": pair1, "csr_pair": pair2, "forms_pair": pair3,
           "matrix_free_faster_than_csr": pair2[0]["us"] < pair2[1]["us"]}
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
