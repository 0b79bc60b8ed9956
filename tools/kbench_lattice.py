"""Timings of the matrix-free bond-list spin kernels on one GPU at L = 20 (docs/design/16-spin-lattice.md), each pair in the
same process, kernels alone (dsea_spmv / dsea_op_*_forms calls back to back between two events, median of five rounds):

    1. k_spmv_lattice with ring bonds                     beside k_spmv_chain with the same couplings;
    2. k_spmv_lattice on the 4 x 5 torus (Heisenberg      beside the to_csr() operand of the same Hamiltonian (default
       couplings plus random fields)                       layout), after checking that the two agree;
    3. k_lattice_forms (all 3 nb + 2 L forms, both        beside (3 nb + 2 L) / 5 calls of the mat-vec.
       stages)

Requirement of pair 2: the matrix-free kernel is not slower than the CSR operand measured in the same run (no margin beyond
the spread of the rounds).  GB/s on ALGORITHMIC bytes: 2 * 8 n for a mat-vec (x read once, y written once), 2 * 8 n for the
forms (v1, v2 read once).

    python tools/kbench_lattice.py [--L 20] [--reps 50] [--rounds 5] [--out profiles/kbench_lattice.json]
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
from dominantsparseeigenad_amd.operators import SpinChainOperator, SpinLatticeOperator, ring_bonds, square_bonds  # noqa: E402

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


def far_terms(L, bonds, tile_log2):
    """(far field flips, far bonds) of the mat-vec at this tile: the 16-byte global partner reads per row pair"""
    T = min(L, tile_log2)
    return L - T, sum(1 for a, b in bonds if max(a, b) >= T)


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
    tile = 11                                            # DSEA_TFIM_TILE_LOG2, the default of both operators

    def spmv(handle):
        return lambda: lib.dsea_spmv(handle, None, _ptr(x), _ptr(y), None, None, None, st)

    # 1. ring bonds beside the chain kernel, the same couplings (nb = L: the flat order is the chain's (5, L) row by row)
    c = torch.randn(5 * L, dtype=F64, device=dev, generator=gen)
    chain = SpinChainOperator(L, c.reshape(5, L))
    ring = SpinLatticeOperator(L, ring_bonds(L), c)
    agree1 = float((ring(x) - chain(x)).norm() / chain(x).norm())
    ta, tb = timed(spmv(chain.handle), args.reps, args.rounds), timed(spmv(ring.handle), args.reps, args.rounds)
    pair1 = [row("k_spmv_chain", ta, mv_bytes),
             row("k_spmv_lattice (ring bonds)", tb, mv_bytes, agreement=agree1, far_terms=far_terms(L, ring.bonds, tile))]
    # 2. the 4 x (L / 4) torus, Heisenberg couplings plus random fields, beside the explicit matrix of the same Hamiltonian
    bonds = square_bonds(4, L // 4)
    assert 4 * (L // 4) == L, "pair 2 needs L divisible by 4"
    nb = len(bonds)
    p = torch.cat([torch.ones(3 * nb, dtype=F64, device=dev), torch.randn(2 * L, dtype=F64, device=dev, generator=gen)])
    torus = SpinLatticeOperator(L, bonds, p)
    csr = torus.to_csr()
    agree2 = float((torus(x) - csr(x)).norm() / torus(x).norm())
    assert agree2 < 1e-13, agree2
    ta, tb = timed(spmv(torus.handle), args.reps, args.rounds), timed(spmv(csr.handle), args.reps, args.rounds)
    pair2 = [row("k_spmv_lattice (4 x %d torus, %d bonds)" % (L // 4, nb), ta, mv_bytes, far_terms=far_terms(L, bonds, tile)),
             row("to_csr() operand, default layout", tb, mv_bytes,
                 nnz=csr.nnz, nnz_per_row=csr.nnz // n, coded=bool(getattr(csr, "_coded", False)), col16=bool(csr.col16),
                 agreement=agree2)]
    # 3. the forms beside (3 nb + 2 L) / 5 mat-vecs
    cnt = c_int64()
    _lib.check(lib.dsea_op_lattice_forms_scratch_doubles(L, nb, byref(cnt)), "scratch")
    scratch = torch.empty(cnt.value, dtype=F64, device=dev)
    out = torch.empty(3 * nb + 2 * L, dtype=F64, device=dev)
    forms = lambda: lib.dsea_op_lattice_forms(torus.handle, _ptr(x), _ptr(x2), _ptr(out), _ptr(scratch), st)  # noqa: E731
    mv = spmv(torus.handle)
    count = (3 * nb + 2 * L) // 5

    def matvecs():
        for _ in range(count):
            mv()
    reps3 = max(5, args.reps // 5)
    ta, tb = timed(forms, reps3, args.rounds), timed(matvecs, reps3, args.rounds)
    pair3 = [row("k_lattice_forms + reduce (%d forms)" % (3 * nb + 2 * L), ta, mv_bytes),
             row("%d calls of k_spmv_lattice" % count, tb, count * mv_bytes)]
    rec = {"L": L, "n": n, "reps": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "ring_pair": pair1, "lattice_over_chain": pair1[1]["us"] / pair1[0]["us"],
           "csr_pair": pair2, "matrix_free_not_slower_than_csr": pair2[0]["us"] <= pair2[1]["us"],
           "csr_over_matrix_free": pair2[1]["us"] / pair2[0]["us"],
           "forms_pair": pair3, "forms_over_matvecs": pair3[0]["us"] / pair3[1]["us"]}
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
