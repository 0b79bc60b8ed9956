"""Timings of the matrix-free Hubbard kernels on one GPU (docs/design/19-hubbard.md) on the 4 x 4 torus, square_bonds(4, 4)
(32 bonds), L = 16, nup = ndn = 5, n = 4368^2 = 19 079 424, t = 1, U = 4, V = eps = 0; each pair in the same process, kernels
alone (dsea_spmv / dsea_op_hubbard_forms calls back to back between two events, median of five rounds):

    1. k_spmv_hubbard                                   beside the to_csr() operand of the same matrix (default layout),
                                                        after checking that the two agree;
    2. k_hubbard_forms + reduce (all 2 nb + 2 L forms)  beside (2 nb + 2 L) / 4 calls of the mat-vec (reported only).

Bar of pair 1 (the one of docs/design/16-spin-lattice.md): the slowest matrix-free round is not slower than the fastest CSR
round.  The script reports whether it holds; it does not fail when it does not.  GB/s on ALGORITHMIC bytes: 2 * 8 n (x read
once, y written once) for a mat-vec, 2 * 8 n for the forms (v1, v2 read once) -- no table of n words is streamed.  It also
states the bytes of the tables beside the bytes of the CSR operand.

    python tools/kbench_hubbard.py [--Lx 4] [--Ly 4] [--nup 5] [--ndn 5] [--reps 20] [--rounds 5] [--out profiles/kbench_hubbard.json]
"""
import argparse
import json
import os
import sys
import time
from ctypes import byref, c_int64

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from dominantsparseeigenad_amd import _lib  # noqa: E402
from dominantsparseeigenad_amd.engine import _ptr, _stream  # noqa: E402
from dominantsparseeigenad_amd.operators import HubbardOperator, square_bonds  # noqa: E402

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
    rec = {"kernel": name, "us": med, "us_min": lo, "us_max": hi, "GBps_algorithmic": nbytes / med / 1e3}
    rec.update(extra)
    return rec


def tensor_bytes(tensors):
    return int(sum(t.numel() * t.element_size() for t in tensors if t is not None))


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
                   torch.zeros(L, dtype=F64)]).to(dev)                                # t = 1, V = 0, U = 4, eps = 0
    op = HubbardOperator(L, bonds, p, nup, ndn)
    n = op.n
    gen = torch.Generator(dev).manual_seed(1)
    x = torch.randn(n, dtype=F64, device=dev, generator=gen)
    x2 = torch.randn(n, dtype=F64, device=dev, generator=gen)
    y = torch.empty(n, dtype=F64, device=dev)
    mv_bytes = 2 * 8 * n

    def spmv(handle):
        return lambda: lib.dsea_spmv(handle, None, _ptr(x), _ptr(y), None, None, None, st)

    # 1. the matrix-free kernel beside the explicit matrix of the same Hamiltonian, default layout
    t0 = time.time()
    csr = op.to_csr()
    torch.cuda.synchronize()
    build_s = time.time() - t0
    print("to_csr(): n = %d, nnz = %d, built in %.1f s" % (n, csr.nnz, build_s), flush=True)
    ref = csr(x)
    agree = float((op(x) - ref).norm() / ref.norm())
    assert agree < 1e-13, agree
    moves = (csr.nnz - n) / n                            # gathers of x per row: the hops that move a particle
    ta, tb = timed(spmv(op.handle), args.reps, args.rounds), timed(spmv(csr.handle), args.reps, args.rounds)
    coded = bool(getattr(csr, "_coded", False))
    csr_tensors = list(csr._sell) + ([csr._codes, csr._vtab] if coded else [])
    pair1 = [row("k_spmv_hubbard (%d x %d torus, %d bonds, nup = %d, ndn = %d)" % (args.Lx, args.Ly, nb, nup, ndn), ta, mv_bytes,
                 gathers_per_row=moves),
             row("to_csr() operand, default layout", tb, mv_bytes, nnz=csr.nnz, nnz_per_row=csr.nnz / n, coded=coded,
                 col16=bool(csr.col16), agreement=agree, build_seconds=build_s)]
    # 2. the forms beside (2 nb + 2 L) / 4 mat-vecs
    cnt = c_int64()
    _lib.check(lib.dsea_op_hubbard_forms_scratch_doubles(L, nup, ndn, nb, byref(cnt)), "scratch")
    scratch = torch.empty(cnt.value, dtype=F64, device=dev)
    out = torch.empty(2 * nb + 2 * L, dtype=F64, device=dev)
    forms = lambda: lib.dsea_op_hubbard_forms(op.handle, _ptr(x), _ptr(x2), _ptr(out), _ptr(scratch), st)  # noqa: E731
    mv = spmv(op.handle)
    count = (2 * nb + 2 * L) // 4

    def matvecs():
        for _ in range(count):
            mv()
    reps2 = max(3, args.reps // 5)
    tc, td = timed(forms, reps2, args.rounds), timed(matvecs, reps2, args.rounds)
    pair2 = [row("k_hubbard_forms + reduce (%d forms)" % (2 * nb + 2 * L), tc, mv_bytes),
             row("%d calls of k_spmv_hubbard" % count, td, count * mv_bytes)]
    tables = list(op._up) + ([] if op._dn is op._up else list(op._dn))
    rec = {"L": L, "nup": nup, "ndn": ndn, "n": n, "n_up": op.n_up, "n_dn": op.n_dn, "bonds": nb, "reps": args.reps,
           "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "csr_pair": pair1,
           "slowest_matrix_free_round_not_slower_than_fastest_csr_round": pair1[0]["us_max"] <= pair1[1]["us_min"],
           "csr_over_matrix_free": pair1[1]["us"] / pair1[0]["us"],
           "forms_pair": pair2, "forms_over_matvecs": pair2[0]["us"] / pair2[1]["us"],
           "forms_in_matvecs": pair2[0]["us"] / pair1[0]["us"],
           "table_bytes": {"table_sets": 1 if op._dn is op._up else 2, "total": tensor_bytes(tables)},
           "csr_operand_bytes": tensor_bytes(csr_tensors),
           "csr_arrays_bytes": tensor_bytes([csr.rowptr, csr.colidx, csr._vals_data])}
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
