#!/usr/bin/env python3
"""Headline benchmark: DominantSparseSymeig forward + backward on a TFIM-shaped sparse operator.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--scaling weak|strong] [--dump-outputs DIR] [--full]

A plain run sets up, runs W untimed and K timed steps, writes the outputs of the last timed step if --dump-outputs is
given, and prints the line.  Everything measured or checked beside the timed steps -- live PMC passes, per-kernel events
and the roofline, the option extras, the config-3 / config-4 / sweep / operand figures, the one-GPU anchors, the CPU
baseline, the N > 1 extra points and scaling decomposition, and the N = 1 supervisor that re-measures in a fresh
process -- runs only with --full.

One "step" = one pass of the hot path over synthetic inputs already resident in HBM, through the reference API:
    forward   symeig.DominantSparseSymeig.apply(g, k, dim, device)      (Lanczos, k vectors, full reorth)
    backward  torch.autograd.grad(E0 + psi.t, g)                         (projected CG adjoint solve + hook)

Workloads (what the K timed steps run, i.e. what `value` / `ms_per_step` are quoted on)
    N = 1 (default)   BASELINE.json configs[1]: TFIM L=20 (n = 2^20), k = 200, fp64, g = 1.0.  With --full the same run
                      then times, OUTSIDE the K steps, the two one-GPU anchors of the multi-GPU curves
                      (config.one_gpu_anchors): L = 28, k = 100 (strong) and 2^25 rows, k = 200 (weak).
    N > 1 (default)   STRONG scaling, north_star's curve: TFIM L=28 (n = 2^28) row-partitioned over the N GPUs with
                      k = 100 at every N (the largest k whose basis, 215 GB, fits the one 288 GB GPU of the anchor).
                      With --full, after the timed steps the WEAK point (2^25 rows per GPU, k = 200; N = 8 is
                      BASELINE configs[4]: L = 28 with 53.7 GB of basis + 13.4 GB bf16 shadow per GPU) is timed too and
                      reported as config.weak_scaling_point.
    --scaling weak|strong   time only that one point.
    --gpus N without a launcher starts its own N worker processes (python -m torch.distributed.run) BEFORE any GPU
    call and relays rank 0's JSON line; under torchrun (WORLD_SIZE set) it is a worker.

value = HBM GB/s of the whole job: bytes the step's kernels move (traffic model below; at the headline size checked
against rocprofv3 PMC counters, profiles/r<NN>_pmc_traffic.json) / step time.  It is bounded by N x 8 TB/s.  The figure of
SURVEY.md 8d -- ALGORITHMIC bytes 8 n (k^2 + 12k + 11m + 17) of the reference's algorithm / step time (m = CG
iterations actually run) -- is config.algorithmic_GBs; it may exceed the peak because the correction pass streams a
bf16 storage shadow of the basis.  Prints ONE JSON line (rank 0) as the last line of stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time
from ctypes import c_double, c_int64

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s is the measured copy ceiling
SEED = 12345
# GPU-vs-reference deviation of the adjoint at the reference's hard-coded CG tolerance (eps = 1e-7 absolute,
# CG.py:25), observed over the golden cases of tests/test_gpu_parity.py (asserted there at 2e-8): see DESIGN.md 5
ADJOINT_DEV_EPS7 = "3e-10..1.6e-9 relative (reference's own seed-to-seed spread: 5e-10)"


def algorithmic_bytes(n, k, m):
    """forward 8n(k^2+12k-7), backward 8n(11m+24)."""
    return 8.0 * n * (k * k + 12 * k + 11 * m + 17)


def traffic_model_bytes(n, k, m, shadow_steps, cg_vectors_per_iteration=11.0):
    """HBM bytes one step of THIS implementation moves, as a model: SURVEY 8d's per-phase count with the correction
    pass of ``shadow_steps`` Lanczos steps reading the bf16 shadow (2 instead of 8 bytes per basis element: step i
    saves 6 n i bytes) plus the k shadow rows written once (2 n each).  At L = 20, k = 200, m = 90: 239.3 GB against
    249.9 GB counted by the PMC (the difference is the TFIM mat-vec's cross-XCD re-reads).
    ``cg_vectors_per_iteration``: 11 for the streaming CG; the persistent single-launch CG keeps x, r, d in
    registers and moves only d (one write + the out-of-tile reads, 4 vectors' worth through the fabric): 5."""
    saved = 6.0 * n * sum(range(1, int(shadow_steps) + 1))
    saved += 8.0 * n * m * (11.0 - float(cg_vectors_per_iteration))
    return algorithmic_bytes(n, k, m) - saved + (2.0 * n * k if shadow_steps else 0.0)


def analytic_E0_per_site(L, g):
    """Closed-form ground-state energy per site of the periodic chain (sanity value printed next to the measured
    one): free fermions with the momenta of the even-parity sector, k = (2m+1) pi / L.  For even L this is the set
    used by reference examples/TFIM/E0.py:15-18; for odd L the reference's linspace would pick integer momenta,
    which is not the ground-state sector."""
    ks = (2 * np.arange(L) + 1) * np.pi / L
    return float(-0.5 * (2 * np.sqrt(g * g - 2 * g * np.cos(ks) + 1)).sum() / L)


def reorth_bytes_per_launch(n, k):
    """average algorithmic bytes of one launch of each reorth kernel over steps i = 1..k-1 (SURVEY 8d split):
    pass 1 = 4 + (i+1) vectors, pass 2 = (i+2) vectors of 8n bytes."""
    steps = k - 1
    dots = sum(4 + (i + 1) for i in range(1, k)) / steps * 8.0 * n
    axpy = sum(i + 2 for i in range(1, k)) / steps * 8.0 * n
    return dots, axpy


class PinnedRandn:
    """torch.randn replacement handing out pre-generated DEVICE vectors in call order (q0, dummy, x0, ...),
    so the timed region contains no host RNG / H2D traffic and every step solves the identical problem."""

    def __init__(self, vectors):
        self.vectors, self.i, self._orig = vectors, 0, None

    def __call__(self, *size, dtype=None, device=None, **kw):
        v = self.vectors[self.i % len(self.vectors)]
        self.i += 1
        assert v.numel() == size[0]
        return v

    def __enter__(self):
        self._orig, torch.randn, self.i = torch.randn, self, 0
        return self

    def __exit__(self, *exc):
        torch.randn = self._orig


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(L, k, cg_cap, threads, model=None):
    """The oracle (CPU port of the reference path, torch CPU ops incl. the gather-table mat-vec) on the same
    workload; ``cg_cap`` None = the reference's cap (n iterations, i.e. runs to ||r|| < 1e-7)."""
    import oracle
    from dominantsparseeigenad_amd.synthetic import normal_vector

    n = 1 << L
    torch.set_num_threads(int(threads))
    t_init = 0.0
    if model is None:
        t0 = time.time()
        model = oracle.TFIMTables(L)
        t_init = time.time() - t0
    model.g = torch.tensor([1.0], dtype=torch.float64, requires_grad=True)
    seeds = iter(range(SEED + 10, SEED + 20))
    draws = lambda m, dtype=torch.float64: torch.from_numpy(normal_vector(m, next(seeds))).to(dtype)  # noqa: E731
    t = torch.from_numpy(normal_vector(n, SEED + 1))
    t = t / t.norm()
    stats = []
    f = oracle.make_sparse_dominant_symeig(model.H, model.adjoint_hook, draw=draws, maxiter=cg_cap, stats=stats).apply
    t0 = time.time()
    E0, psi = f(model.g, k, n)
    t_fwd = time.time() - t0
    loss = E0 + psi.matmul(t)
    (gl,) = torch.autograd.grad(loss, model.g)
    dt = time.time() - t0
    m = stats[0]["iters"]
    return model, {"threads": int(threads), "k": k, "cg_iterations": m, "fwd_s": round(t_fwd, 2),
                   "bwd_s": round(dt - t_fwd, 2), "fwd_bwd_s": round(dt, 2), "table_build_s": round(t_init, 2),
                   "GBs": round(algorithmic_bytes(n, k, m) / dt / 1e9, 3), "E0": E0.item(), "dloss_dg": gl.item()}


def measured_ceilings(dev):
    """the box's own streaming ceilings next to the 8 TB/s spec figure, measured with the library's probe
    kernels (dsea_probe_stream: 8 non-temporal 16-byte loads in flight per lane, nothing else to do) on 1 GiB buffers
    (beyond the 256 MiB Infinity Cache): a read-only pass and a copy (bytes read + written); torch's own copy kernel
    beside them.  Best of 5 after 2 warm-ups, HIP events on the current stream."""
    from dominantsparseeigenad_amd import engine, _lib
    lib = _lib.load()
    nel = 1 << 27                                   # 1 GiB of doubles
    a = torch.ones(nel, dtype=torch.float64, device=dev)
    b = torch.empty(nel, dtype=torch.float64, device=dev)
    ws = engine.Workspace.get(4096, 8, dev)         # the probe only borrows its partial-sum buffer
    st = engine._stream(dev)

    def best(fn):
        for _ in range(2):
            fn()
        t = 1e30
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            t = min(t, e0.elapsed_time(e1) * 1e-3)
        return t
    t_read = best(lambda: engine.check(lib.dsea_probe_stream(ws.handle, engine._ptr(a), None, nel, st), "dsea_probe_stream"))
    t_copy = best(lambda: engine.check(lib.dsea_probe_stream(ws.handle, engine._ptr(a), engine._ptr(b), nel, st), "dsea_probe_stream"))
    t_torch = best(lambda: b.copy_(a))
    res = {"read_GBs": round(8.0 * nel / t_read / 1e9, 1), "copy_GBs": round(2 * 8.0 * nel / t_copy / 1e9, 1),
           "torch_copy_GBs": round(2 * 8.0 * nel / t_torch / 1e9, 1),
           "what": "1 GiB buffers: read-only reduction / copy (bytes read + written) by dsea_probe_stream, torch's "
                   "copy_ beside them; best of 5, HIP events"}
    del a, b
    return res


def c3_figures(dev):
    """BASELINE configs[2] in its well-posed restatement: 3-point stencil N = 100000
    (schrodinger1D.py:11-27 semantics), Lanczos k = 300 forward and CG over a FIXED 1000 iterations."""
    from dominantsparseeigenad_amd import engine
    from dominantsparseeigenad_amd.Lanczos import symeigLanczos
    from dominantsparseeigenad_amd.operators import Stencil3Operator
    from dominantsparseeigenad_amd.synthetic import normal_vector
    N, k, iters = 100000, 300, 1000
    x = torch.from_numpy(np.linspace(-1.0, 1.0, num=N, endpoint=False)).to(dev)
    op = Stencil3Operator(N, 2.0 / N, 0.5 * x ** 2)
    q0 = torch.from_numpy(normal_vector(N, 1)).to(dev)
    best_l = best_c = 1e30
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        symeigLanczos(op, k, dev, extreme="min", sparse=True, dim=N, q0=q0)
        torch.cuda.synchronize()
        best_l = min(best_l, time.perf_counter() - t0)
    b = torch.from_numpy(normal_vector(N, 2)).to(dev)
    x0 = torch.from_numpy(normal_vector(N, 3)).to(dev)
    shift = torch.tensor(-1.0, dtype=torch.float64, device=dev)
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        engine.cg(b, x0, native=op, shift=shift, eps=0.0, maxiter=iters, poll_every=iters)
        torch.cuda.synchronize()
        best_c = min(best_c, time.perf_counter() - t0)
    ran = engine.last_cg.iters
    best_m = 1e30
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        engine.cg(b, x0, native=op, shift=shift, eps=0.0, maxiter=iters, poll_every=iters, merged_reductions=True)
        torch.cuda.synchronize()
        best_m = min(best_m, time.perf_counter() - t0)
    return {"workload": "3-point stencil N=100000 (schrodinger1D.py:18-27), Lanczos k=300 forward; CG on (A+1)x=b over "
                        "a fixed %d iterations" % ran,
            "lanczos_k300_ms": round(best_l * 1e3, 3), "lanczos_us_per_step": round(best_l / k * 1e6, 2),
            "lanczos_algorithmic_GBs": round(8.0 * N * (k * k + 12 * k) / best_l / 1e9, 1),
            "cg_us_per_iteration": round(best_c / ran * 1e6, 3),
            "cg_algorithmic_GBs": round(11 * 8.0 * N * ran / best_c / 1e9, 1), "cg_iterations": ran,
            "cg_us_per_iteration_merged_reductions": round(best_m / ran * 1e6, 3),
            "cg_note": "cg_us_per_iteration: persistent single-launch CG with the reference's recurrences (iterates "
                       "bit-identical to CG.py:31-40 evaluated in fp64 on the device, two grid-wide exchanges per "
                       "iteration); merged_reductions: the optional one-exchange form (Chronopoulos-Gear; same iteration "
                       "in exact arithmetic, 6e-14 relative deviation after 40 iterations), off by default"}


def sweep_figures(dev, N=20, k=200, idxs=(25, 50, 75), warm=80):
    """Row f-2 as a driver-timed figure: the reference's SECOND-ORDER workload per coupling (examples/TFIM/E0.py:53-67
    ``E0_sparseAD`` = forward + d/dg + d2/dg2, chiF.py:40-53 ``chiF_sparseAD`` = forward + two derivatives of log F: two
    forward passes and six CG solves per coupling, counted in the kernel trace) at N = 20, k = 200, on the three couplings the
    parity test uses, against the reference's stored curves (tests/golden/ref_datas = its own outputs); cold, and with the previous
    coupling's eigenvector as the start vector of a ``warm``-step Lanczos (an extension the reference lacks)."""
    import importlib.util
    import DominantSparseEigenAD.Lanczos as LZ

    def load(fname, name):
        d = os.path.join(ROOT, "examples", "TFIM")
        if d not in sys.path:
            sys.path.insert(0, d)
        spec = importlib.util.spec_from_file_location(name, os.path.join(d, fname))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    E0m, chim = load("E0.py", "bench_ex_E0"), load("chiF.py", "bench_ex_chiF")
    curE = np.load(os.path.join(ROOT, "tests", "golden", "ref_datas", "E0_N_%d.npz" % N))
    curC = np.load(os.path.join(ROOT, "tests", "golden", "ref_datas", "chiF_N_%d.npz" % N))
    model = E0m.TFIM(N, dev)
    out = {"workload": "TFIM N=%d k=%d: E0, dE0/dg, d2E0/dg2 (E0.py:53-67) and chi_F (chiF.py:40-53) per coupling -- two forward "
                       "passes + six CG solves; couplings g = %s" % (N, k, ", ".join("%.3f" % curE["gs"][i] for i in idxs))}
    for label, kw in (("cold", 0), ("warm_%d" % warm, warm)):
        torch.manual_seed(1)
        dev_max = {"E0": 0.0, "dE0": 0.0, "d2E0": 0.0, "chiF": 0.0}
        prev, times = None, []
        try:
            for idx in idxs:
                g = float(curE["gs"][idx])
                model.g = torch.tensor([g], dtype=torch.float64, device=dev, requires_grad=True)
                kk = k
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if kw and prev is not None:
                    kk, LZ.WARM_START = kw, prev
                e, de, d2e = E0m.E0_sparseAD(model, kk)
                if kw and prev is not None:
                    LZ.WARM_START = prev
                _, psi, c = chim.chiF_sparseAD(model, kk)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
                prev = psi.detach()
                for key, got, want in (("E0", e, curE["E0s"][idx]), ("dE0", de, curE["dE0s"][idx]),
                                       ("d2E0", d2e, curE["d2E0s"][idx]), ("chiF", c, curC["chiFs"][idx])):
                    dev_max[key] = max(dev_max[key], abs(got - want) / abs(want))
        finally:
            LZ.WARM_START = None
        # warm: the first coupling has no predecessor (it runs cold) -- the figure is the mean over the others
        use = times[1:] if kw else times
        out[label] = {"ms_per_coupling": round(sum(use) / len(use) * 1e3, 2), "couplings_timed": len(use),
                      "max_rel_deviation_from_reference_curves": {kk2: float("%.2e" % v) for kk2, v in dev_max.items()}}
    out["note"] = "the stored curves pin results at the 1e-6 ... 1e-5 level (SURVEY 8c: produced with a less converged setting)"
    return out


def _fused_tail_us(pa, ctx):
    """(average us, launches) of the fused Lanczos tail of one step of ``pa``, from HIP events attached to the dispatches (as the
    headline's roofline)"""
    from dominantsparseeigenad_amd import _lib, engine
    lib = _lib.load()
    launches, total_ms = (c_int64 * 3)(), (c_double * 3)()
    ws = engine.Workspace.get(pa.n, pa.k, ctx.dev)
    _lib.check(lib.dsea_profile_begin(ws.handle, 3 * pa.k * 2 + 8), "dsea_profile_begin")
    pa.step()
    pa.barrier()
    _lib.check(lib.dsea_profile_end(ws.handle, launches, total_ms), "dsea_profile_end")
    return (total_ms[2] / launches[2] * 1e3, int(launches[2])) if launches[2] > 0 else (None, 0)


def sell_operand_figures(ctx, args, steps=3):
    """SURVEY 8d C2 (ii) as a driver-observed figure: the headline workload with the operator given as an EXPLICIT matrix
    (21 non-zeros per row, SELL-64 layout, fp64 values + 16-bit column deltas, dsea_op_create_sell16p2) instead of the matrix-free
    kernel; beside it
    the same matrix VALUE-CODED (dsea_op_create_sell16v8: what the host layer picks for a non-parameter operand of few
    distinct values -- this one has 11)"""
    pa = Problem(ctx, 20, 200, False, operator="sell")
    try:
        dt, E0, _ = pa.measure(steps, 1)
        ms = dt / steps * 1e3
        m = pa.cg_iterations()
        n, k = pa.n, pa.k
        operand = 12.0 * 21 * n * (k + m + 1)
        moved = traffic_model_bytes(n, k, m, (k - 1) if pa.use_shadow else 0) + operand
        tail = None
        try:
            us, cnt = _fused_tail_us(pa, ctx)
            if us is not None:
                alg = 12.0 * 21 * n + 8.0 * (n // 64 + 1) + 16.0 * n        # 12 B per non-zero + two vectors
                tail = {"kernel": "k_spmv_sell<fused Lanczos tail>", "avg_launch_us": round(us, 2), "launches": cnt,
                        "algorithmic_bytes_per_launch": alg, "algorithmic_GBs": round(alg / us / 1e3, 1),
                        "frac_of_hbm_peak_on_algorithmic_bytes": round(alg / us / 1e3 / HBM_PEAK_GBS, 4),
                        "columns": ("16-bit deltas" + (", values and deltas packed two slice columns to a lane"
                                                       if getattr(pa.A_operand, "_pack2", False) else ""))
                        if getattr(pa.A_operand, "col16", False) else "int32",
                        "note": "in situ (Infinity Cache swept by the basis passes; also writes q and its bf16 shadow); the kernel "
                                "alone: profiles/r06_kbench_csr.txt"}
        except Exception as exc:  # noqa: BLE001
            tail = "failed: %s: %s" % (type(exc).__name__, exc)
        out = {"workload": pa.describe(), "ms_per_step": round(ms, 3), "steps": steps, "cg_iterations": int(m),
               "fused_tail": tail,
               "bytes_per_step": moved, "GBs": round(moved / (ms * 1e-3) / 1e9, 1),
               "frac_of_hbm_peak": round(moved / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
               "E0_per_site_minus_closed_form": E0.item() / 20 - analytic_E0_per_site(20, 1.0),
               "bytes_note": "the matrix-free step's traffic model + the matrix stream: 12 B per non-zero, 21 per row, in each "
                             "of the %d mat-vecs" % (k + m + 1)}
    finally:
        pa.release()
    try:
        pc = Problem(ctx, 20, 200, False, operator="sell-coded")
        try:
            dt, E0c, _ = pc.measure(steps, 1)
            us, cnt = _fused_tail_us(pc, ctx)
            opv = pc.A_operand
            out["value_coded"] = {
                "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps, "cg_iterations": int(pc.cg_iterations()),
                "fused_tail_avg_launch_us": None if us is None else round(us, 2),
                "distinct_values": int((opv._vtab != 0).sum().item()), "bytes_per_stored_element": 3.0625,
                "E0_equal_to_the_fp64_value_operand": bool(E0c.item() == E0.item()),
                "note": "same matrix, values as 8-bit codes into a 256-entry fp64 table, slices padded 21 -> 24 columns; products "
                        "formed with the same doubles in the same order (bit-identical results); NOT a roofline figure on the "
                        "12 B / non-zero the general layout is priced on -- it moves 3.06"}
        finally:
            pc.release()
    except Exception as exc:  # noqa: BLE001
        out["value_coded"] = "failed: %s: %s" % (type(exc).__name__, exc)
    return out


class _ReferenceStyleTFIM:
    """the mat-vec an UNCHANGED user script hands over (reference examples/TFIM/TFIM.py:39-51,91-98 semantics: a diagonal and an
    (n, L) int64 gather table, torch index ops) -- built here with index arithmetic instead of the reference's numpy bit tables"""

    def __init__(self, L, g, dev):
        n = 1 << L
        idx = torch.arange(n, dtype=torch.int64, device=dev)
        rot = ((idx << 1) | (idx >> (L - 1))) & (n - 1)
        x = idx ^ rot
        pop = torch.zeros_like(x)
        for b in range(L):
            pop += (x >> b) & 1
        self.diag_elements = (-(L - 2 * pop)).to(torch.float64)
        self.flips_basis = idx[:, None] ^ (1 << torch.arange(L, dtype=torch.int64, device=dev))[None, :]
        self.g = g

    def H(self, v):
        return v * self.diag_elements - self.g * v[self.flips_basis].sum(dim=1)          # TFIM.py:96-97


def _kernel_time_of(fn):
    """(wall ms, sum of kernel durations ms) of fn() from torch's profiler (kineto over roctracer), or (wall, None)"""
    under_profiler = any(k.startswith(("ROCPROF", "ROCP_", "ROCTRACER")) for k in os.environ) or \
        "rocprof" in os.environ.get("LD_PRELOAD", "")
    try:
        if under_profiler:       # the whole bench is being traced by rocprofv3: no second tracer inside it
            raise RuntimeError("external profiler attached")
        from torch.profiler import profile, ProfilerActivity
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
        dev_us = 0.0
        for ev in prof.events():
            if getattr(ev, "device_type", None) is not None and "cuda" in str(ev.device_type).lower():
                dev_us += float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0) or 0.0)
        return wall, (dev_us * 1e-3 if dev_us > 0 else None)
    except Exception:  # noqa: BLE001
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, None


def callable_operand_figures(ctx, args, native_ms, steps=3):
    """The reference's ACTUAL calling convention as a driver-observed figure (round-5 verdict, Next 5): the headline workload
    with ``A`` an opaque Python callable (reference examples/TFIM/E0.py:59-62, examples/schrodinger1D.py:69-71, symeig.py:71-75)
    -- what an unchanged user script gets.  The loops cannot see the operator: the mat-vec is the caller's code, every other
    vector operation of a Lanczos step / CG iteration is a phase call of include/dsea.h issued from Python."""
    out = {"native_operand_ms_per_step": round(native_ms, 3)}
    for label, operator in (("lambda_around_native_matvec", "callable-native"), ("reference_style_torch_gather_tables", "callable-tables")):
        pa = Problem(ctx, 20, 200, False, operator=operator)
        try:
            dt, E0, _ = pa.measure(steps, 1)
            ms = dt / steps * 1e3
            m = pa.cg_iterations()
            rec = {"ms_per_step": round(ms, 3), "steps": steps, "vs_native_operand": round(ms / native_ms, 4), "cg_iterations": int(m),
                   "cg_form": str(pa.engine.last_cg.form), "cg_host_polls": int(getattr(pa.engine.last_cg, "polls", -1)),
                   "E0_per_site_minus_closed_form": E0.item() / 20 - analytic_E0_per_site(20, 1.0)}
            out[label] = rec
            if os.environ.get("DSEA_BENCH_INPROCESS_PROFILER", "") != "1":
                # host time outside kernels comes from a kernel trace taken OUTSIDE the driver line (tools/gpu_evidence.sh
                # callable -> profiles/r06_callable_operand_trace.txt); an in-process tracer (torch.profiler over roctracer) in
                # the default run is one more thing that can stall a GPU box, and it is switched off unless asked for
                continue
            # host time outside kernels, forward (k Lanczos steps) and backward (m CG iterations) separately
            k = pa.k
            with PinnedRandn(pa.draws):
                hold = {}

                def fwd():
                    hold["E0"], hold["psi"] = pa.f(pa.g, pa.k, pa.n, pa.dev)

                def bwd():
                    torch.autograd.grad(hold["E0"] + pa.dot(hold["psi"], pa.tvec), pa.g)

                wf, kf = _kernel_time_of(fwd)
                wb, kb = _kernel_time_of(bwd)
            if kf is not None and kb is not None:
                rec["host_us_per_lanczos_step_outside_kernels"] = round(max(wf - kf, 0.0) / k * 1e3, 2)
                rec["host_us_per_cg_iteration_outside_kernels"] = round(max(wb - kb, 0.0) / max(m, 1) * 1e3, 2)
                rec["kernel_ms_forward_backward"] = [round(kf, 3), round(kb, 3)]
                rec["note"] = "wall - sum of kernel durations under torch's profiler (slower than the un-profiled step above)"
            out[label] = rec
        except Exception as exc:  # noqa: BLE001
            out[label] = "failed: %s: %s" % (type(exc).__name__, exc)
        finally:
            pa.release()
    return out


def c4_figures(dev):
    """BASELINE configs[3]: dominant eigen-triple of the MPS transfer matrix at bond dimension D = 512 (n = 262144),
    DominantSparseEig k = 200 (examples/TFIM_vumps/general.py:59-66, eig.py:115-149) -- the one MFMA-shaped operand of the path."""
    import dominantsparseeigenad_amd.eig as eig
    from dominantsparseeigenad_amd.operators import TransferOperator
    from dominantsparseeigenad_amd.synthetic import normal_vector
    D, d, k = 512, 2, 200
    n = D * D
    A = (torch.from_numpy(normal_vector(d * n, 11)).reshape(d, D, D) / D ** 0.5).to(dev).requires_grad_(True)
    Ad = A.detach()
    op, opT = TransferOperator(Ad), TransferOperator(Ad, transpose=True)

    def hook(pieces):                                        # dA of sum_s A_s r A_s^T (general.py:66-76 counterpart)
        gA = torch.zeros_like(Ad)
        for u, v in pieces:
            um, vm = u.reshape(D, D), v.reshape(D, D)
            gA = gA + torch.matmul(torch.matmul(um, Ad), vm.T) + torch.matmul(torch.matmul(um.T, Ad), vm)
        return gA

    v = torch.from_numpy(normal_vector(n, 12)).to(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(20):
        op(v)
    reps = 200
    e0.record()
    for _ in range(reps):
        op(v)
    e1.record()
    torch.cuda.synchronize()
    mv_us = e0.elapsed_time(e1) / reps * 1e3
    eig.setDominantSparseEig(op, opT, hook)
    tv1, tv2 = torch.from_numpy(normal_vector(n, 13)).to(dev), torch.from_numpy(normal_vector(n, 14)).to(dev)
    best_f = best_b = 1e30
    lam = None
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lam, l, r = eig.DominantSparseEig.apply(A, k)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        loss = lam.sum() + (l * tv1).sum() * (r * tv2).sum()
        torch.autograd.grad(loss, A)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        best_f, best_b = min(best_f, t1 - t0), min(best_b, t2 - t1)
    res = float((op(r.detach()) - lam.detach() * r.detach()).norm())
    flops = 4.0 * d * D ** 3                                 # two products of d D^3 multiply-adds
    return {"workload": "MPS transfer matrix D=512, d=2 (n=262144), DominantSparseEig k=200: forward = two Arnoldi solves, "
                        "backward = two GMRES solves",
            "forward_ms": round(best_f * 1e3, 2), "backward_ms": round(best_b * 1e3, 2),
            "matvec_us": round(mv_us, 2), "matvec_TFLOPs_fp64": round(flops / (mv_us * 1e-6) / 1e12, 1),
            "matvec_frac_of_fp64_matrix_peak": round(flops / (mv_us * 1e-6) / 1e12 / 78.6, 3),
            "fp64_matrix_peak_note": "78.6 TFLOP/s = the vendor's dense fp64 matrix figure for MI355X (MI355X_MICROARCH.md has no fp64 "
                                     "row); tools/probes/mfma_f64_probe.hip sustains 70-77 in a pure register loop",
            "matvec_form": "two hand-written v_mfma_f64_16x16x4_f64 kernels on fragment-packed operands "
                           "(csrc/dsea_transfer_mfma.hip); DSEA_TRANSFER_MFMA=0 selects two rocBLAS GEMMs",
            "eigen_residual": res}


def live_pmc_traffic(timeout_s=240):
    """HBM bytes per launch of every kernel of ONE step of the headline workload, from the PMC counters, measured NOW on
    this box: two rocprofv3 passes (FETCH_SIZE, WRITE_SIZE: separate passes, --kernel-trace only, as
    MI355X_MICROARCH.md prescribes) over `bench.py --steps 1 --warmup 1` as CHILD processes.  Must be called before
    this process touches the GPU (a process that has initialised the GPU must not start other programs on this pool).
    Units: KiB -> x 1024; on gfx950 FETCH_SIZE reports half of the bytes of wide coalesced reads -> x 2.
    Returns (dict in the format of profiles/r<NN>_pmc_traffic.json, None) or (None, reason)."""
    import collections
    import csv
    import glob
    import shutil
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    acc = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        outdir = tempfile.mkdtemp(prefix="dsea_pmc_", dir="/tmp")
        cmd = [exe, "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", outdir, "-o", "p", "--",
               sys.executable, os.path.abspath(__file__), "--steps", "1", "--warmup", "1", "--no-cpu-baseline",
               "--no-extras", "--no-anchors", "--no-kernel-events", "--no-live-pmc"]
        env = dict(os.environ, TMPDIR="/tmp", DSEA_BENCH_CHILD="1")
        try:
            proc = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                  text=True, timeout=timeout_s)
        except subprocess.TimeoutExpired:
            shutil.rmtree(outdir, ignore_errors=True)
            return None, "rocprofv3 --pmc %s pass timed out after %d s" % (counter, timeout_s)
        except OSError as exc:
            shutil.rmtree(outdir, ignore_errors=True)
            return None, "rocprofv3 could not be started: %s" % exc
        files = glob.glob(os.path.join(outdir, "**", "*counter_collection.csv"), recursive=True)
        if proc.returncode != 0 or not files:
            shutil.rmtree(outdir, ignore_errors=True)
            return None, "rocprofv3 --pmc %s pass failed (rc %s): %s" % (counter, proc.returncode, proc.stdout[-200:].replace("\n", " "))
        per = collections.defaultdict(lambda: [0, 0.0])
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                if row.get("Counter_Name") != counter:
                    continue
                short = row["Kernel_Name"].split("(")[0].replace("void ", "").replace("dsea::", "").split("<")[0]
                per[short][0] += 1
                per[short][1] += float(row["Counter_Value"])
        acc[counter] = per
        shutil.rmtree(outdir, ignore_errors=True)
    out = {"_method": "live: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE in two separate passes over one warm-up + one timed "
                      "step of this script on this box, child processes started before the timed run; bytes = "
                      "FETCH_SIZE[KiB]*1024*2 (gfx950 wide-read correction) + WRITE_SIZE[KiB]*1024"}
    steps = 2
    for name in sorted(acc["FETCH_SIZE"]):
        if not name.startswith("k_"):
            continue
        nf, fs = acc["FETCH_SIZE"][name]
        nw, wsz = acc["WRITE_SIZE"].get(name, [0, 0.0])
        rd = fs / nf * 1024 * 2
        wr = (wsz / nw * 1024) if nw else 0.0
        out[name] = {"launches": nf, "fetch_bytes_per_launch": rd, "write_bytes_per_launch": wr,
                     "hbm_bytes_per_launch": rd + wr}
    out["_steps_profiled"] = steps
    out["_total_hbm_bytes_per_step"] = sum(v["launches"] * v["hbm_bytes_per_launch"] for kk, v in out.items()
                                           if kk.startswith("k_")) / steps
    out["_commit"] = "live"
    return out, None


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_workers(n):
    """--gpus N without a launcher: start N fresh worker processes (one per GPU) BEFORE this process has touched
    the GPU, relay their output and finish with rank 0's JSON as the last line of stdout."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % n,
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # the workers are SUPERVISORS (tools/bench_watchdog.py): each runs the measuring process as its child, notices a stall
    # and walks the fallback ladder, so a line comes back well inside their budget; the limit here is the last resort
    limit = float(os.environ.get("DSEA_BENCH_BUDGET_S", "1500")) + 240.0
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env, start_new_session=True)
    try:
        stdout, _ = proc.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        import signal
        try:
            os.killpg(proc.pid, signal.SIGKILL)
        except OSError:
            proc.kill()
        stdout, _ = proc.communicate()
        stdout = (stdout or "") + "\nbench.py: the worker group exceeded %.0f s and was killed\n" % limit
    lines = stdout.splitlines()
    final = None
    for line in lines:
        if line.startswith("{") and '"metric"' in line:
            final = line
        else:
            print(line)
    sys.stdout.flush()
    if final is not None:
        print(final, flush=True)
    raise SystemExit(proc.returncode if proc.returncode else (0 if final is not None else 1))


def progress(event, **kw):
    """one line into this rank's progress file (DSEA_BENCH_PROGRESS, set by the supervisor of tools/bench_watchdog.py):
    the supervisor takes a file that stops growing for a stall"""
    path = os.environ.get("DSEA_BENCH_PROGRESS")
    if not path:
        return
    try:
        with open(path, "a") as f:
            f.write(json.dumps(dict(kw, event=event, t=round(time.time(), 3))) + "\n")
    except OSError:
        pass


def _simulated_hang(ctx, where):
    """DRY RUN only (tests of the watchdog on CPU processes): DSEA_BENCH_SIMULATE_HANG is set by the supervisor for the
    stages an injected fault of that kind would hit; rank 0 then stops making progress in its second step"""
    kind = os.environ.get("DSEA_BENCH_SIMULATE_HANG", "")
    if ctx.dry and kind == "crash" and ctx.rank == 1 and where == "step 2":
        raise RuntimeError("simulated failure of rank 1 (dry run)")
    if ctx.dry and kind and ctx.rank == 0 and where == ("extras" if kind == "extras" else "step 2") and kind != "crash":
        print("bench.py: simulated %s hang (dry run, stage %s)" % (os.environ["DSEA_BENCH_SIMULATE_HANG"],
                                                                   os.environ.get("DSEA_BENCH_STAGE", "?")), flush=True)
        while True:
            time.sleep(3600)


# ---------------------------------------------------------------------------------------------- one-GPU anchors
# The multi-GPU lines quote speed-ups against ONE-GPU runs of the same workload ("anchors").  They are measured LIVE by
# the default N = 1 invocation (config.one_gpu_anchors), which also leaves them in ANCHOR_CACHE so that the N = 2, 4, 8
# lines of the same back-to-back sequence on the same node divide by what THAT node measured.  Resolution order of an
# N > 1 line: --anchors-json PATH (an N = 1 line, or a driver record wrapping one under "parsed") > $DSEA_ANCHORS_JSON >
# the cache of this node > the newest committed profiles/r<NN>_bench.json that carries anchors.  No hand-copied constants.
ANCHOR_CACHE = os.path.join(os.environ.get("TMPDIR", "/tmp"), "dsea_one_gpu_anchors.json")
# the anchors and the arithmetic of their correction pass ("shadow": bf16 storage shadow of the basis):
#   weak_2p25_rows_k200     2^25 rows, k = 200, shadow on   (the per-GPU load of BASELINE configs[4]; fits one GPU with it)
#   strong_L28_k100         L = 28, k = 100, fp64 basis     (215 GB basis: the shadow does NOT fit beside it on one GPU)
#   strong_L28_k80_shadow   L = 28, k = 80, shadow on       (172 + 43 GB: the largest round k whose shadow fits one GPU)
ANCHOR_SPECS = (("weak_2p25_rows_k200", 25, 200, 3, "on"), ("strong_L28_k100", 28, 100, 2, "off"),
                ("strong_L28_k80_shadow", 28, 80, 2, "on"))
STRONG_K, STRONG_K_SHADOW_MATCHED = 100, 80


def _commit():
    """the tree's commit: from git where the tree has its history, else the stamp __graft_entry__.build() leaves (.commit
    travels to the GPU box, .git does not)"""
    if os.path.isdir(os.path.join(ROOT, ".git")):
        try:
            out = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
            if out:
                return out
        except OSError:
            pass
    try:
        return open(os.path.join(ROOT, ".commit")).read().strip() or "unknown"
    except OSError:
        return "unknown"


def _anchors_of(path):
    """(anchors dict, description) from a JSON file holding an N = 1 bench line (possibly among other lines, possibly
    wrapped by the driver under "parsed"), or from the node cache written by ``store_anchors``; (None, reason) otherwise"""
    try:
        text = open(path).read()
    except OSError as exc:
        return None, "%s: %s" % (path, exc)
    cands = []
    try:
        cands.append(json.loads(text))
    except ValueError:
        for ln in text.splitlines():
            if ln.startswith("{"):
                try:
                    cands.append(json.loads(ln))
                except ValueError:
                    pass
    for d in reversed(cands):
        if not isinstance(d, dict):
            continue
        d = d.get("parsed", d) if isinstance(d.get("parsed", None), dict) else d
        anchors = d.get("one_gpu_anchors") or d.get("config", {}).get("one_gpu_anchors")
        if isinstance(anchors, dict) and any(isinstance(v, dict) and v.get("ms_per_step") for v in anchors.values()):
            commit = d.get("commit") or d.get("config", {}).get("commit")
            return anchors, "%s%s" % (os.path.relpath(path, ROOT) if path.startswith(ROOT) else path,
                                      " (commit %s)" % commit if commit else "")
    return None, "%s: no one_gpu_anchors with a measured ms_per_step" % path


def load_anchors(args):
    """resolution order documented at ANCHOR_CACHE; returns (anchors or {}, source description)"""
    import glob
    tried = []
    for path in (args.anchors_json, os.environ.get("DSEA_ANCHORS_JSON"), ANCHOR_CACHE):
        if path and os.path.exists(path):
            anchors, src = _anchors_of(path)
            if anchors:
                if path == ANCHOR_CACHE:
                    src = "this node's N = 1 run of the same sequence (%s)" % src
                return anchors, src
            tried.append(src)
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_bench.json")), reverse=True):
        anchors, src = _anchors_of(path)
        if anchors:
            return anchors, "committed %s (another box: the N = 1 line of this sequence re-measures it)" % src
        tried.append(src)
    return {}, "no anchors found (%s)" % "; ".join(tried[-3:])


def store_anchors(anchors):
    try:
        with open(ANCHOR_CACHE, "w") as f:
            json.dump({"one_gpu_anchors": anchors, "commit": _commit(), "host": socket.gethostname(),
                       "unix_time": time.time()}, f)
    except OSError:
        pass


def anchor_ms(anchors, tag, shadow):
    """ms_per_step of anchor ``tag`` IF it ran with the arithmetic asked for (``shadow`` True / False), else None"""
    a = anchors.get(tag)
    if not isinstance(a, dict) or not a.get("ms_per_step"):
        return None
    if bool(a.get("bf16_shadow_of_basis")) != bool(shadow):
        return None
    return float(a["ms_per_step"])


# ---------------------------------------------------------------------------------------------- the workload
class Problem:
    """One TFIM workload behind the reference API: operator, pinned draws, step() = forward + backward.
    ``shadow``: "auto" (on where the bf16 shadow fits beside the basis), "on" (must fit), "off" (all-fp64 correction)."""

    def __init__(self, ctx, L, k, partitioned_path, reorth="full", shadow="auto", operator="matrix-free"):
        from dominantsparseeigenad_amd import engine
        import dominantsparseeigenad_amd.symeig as symeig
        from dominantsparseeigenad_amd.synthetic import normal_vector
        self.engine, self.symeig, self.ctx = engine, symeig, ctx
        world, rank, dev, dry = ctx.world, ctx.rank, ctx.dev, ctx.dry
        self.L, self.k, self.world, self.rank, self.dev, self.dry = L, k, world, rank, dev, dry
        self.partitioned = partitioned_path
        self.reorth = reorth
        self.operator = operator
        self.notes = {}
        p = int(np.log2(world)) if partitioned_path else 0
        self.p, self.Lloc = p, L - p
        self.nloc, self.n = 1 << (L - p), 1 << L
        off = rank * self.nloc if partitioned_path else 0
        # one GPU cannot hold the fp64 basis AND its bf16 shadow at L = 28, k = 100 (215 + 54 GB of 288 GB)
        free_b, total_b = (0, 1 << 62) if dry else torch.cuda.mem_get_info(dev)
        need_shadow = 10.0 * self.nloc * k + 16 * 8.0 * self.nloc
        fits = need_shadow <= 0.92 * total_b / (ctx.ranks_per_device if not dry else 1)
        if reorth in ("none", "partial") or shadow == "off":
            self.use_shadow = False
        elif shadow == "on":
            if not fits:
                raise RuntimeError("--shadow on: basis + bf16 shadow need %.0f GB of %.0f GB" % (need_shadow / 1e9, total_b / 1e9))
            self.use_shadow = True
        else:
            self.use_shadow = fits
        self.shadow_policy = shadow

        def slab(seed):
            return torch.from_numpy(normal_vector(self.nloc, seed, offset=off)).to(dev)

        self.g = torch.tensor([1.0], dtype=torch.float64, device=dev, requires_grad=True)
        self.draws = [slab(SEED + 10 + c) for c in range(3)]  # q0, unused second draw, CG start vector
        tvec = slab(SEED + 1)
        if not partitioned_path:
            from dominantsparseeigenad_amd.operators import TFIMOperator
            self.tvec = tvec / tvec.norm()
            self.op = TFIMOperator(L, dev)
            self.op.g = self.g
            self.A_operand = self.op.H
            if operator in ("sell", "csr", "sell-coded"):
                # explicit matrix (values fixed at the current g); "sell" = the general layout, fp64 values
                self.A_operand = self.op.to_csr(layout="csr" if operator == "csr" else "sell",
                                                values="coded" if operator == "sell-coded" else "plain")
            elif operator == "callable-native":
                # the reference's calling convention (examples/TFIM/E0.py:59-62): an OPAQUE Python callable -- here a lambda
                # around the native mat-vec, so the loops cannot see the operator and every other vector operation is a phase call
                native_H = self.op.H
                self.A_operand = lambda v: native_H(v)
            elif operator == "callable-tables":
                # ... and the reference's own torch mat-vec: gather tables (examples/TFIM/TFIM.py:39-51,91-98) on the device
                self.A_operand = _ReferenceStyleTFIM(L, self.g, dev).H
            elif operator != "matrix-free":
                raise ValueError(operator)
            self.dot = torch.matmul
        else:
            self.op = self._partitioned_operator()
            self.op.force_driver = True
            self.A_operand = self.op.H
            self.dot = self.op.dot
            self.tvec = tvec / self.op.dot(tvec, tvec).sqrt()
        self.last = {}

    def _partitioned_operator(self):
        """The row-partitioned operator on this stack.  The library-side driver (collectives issued by libdsea) needs its
        communicators; if creating them fails on ANY rank the decision to use the Python driver instead is taken
        collectively (an all-reduced flag)."""
        import torch.distributed as dist
        from dominantsparseeigenad_amd import partitioned
        ctx = self.ctx
        backend = comm = None
        if self.dry:   # the torch test double of the slab kernels (test infrastructure; never on the product path)
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from cpu_backend import CpuBackend
            backend = CpuBackend(self.nloc)
        if ctx.staged:   # ranks sharing one GPU: gloo staged through the host (RCCL refuses two ranks on a device)
            comm = partitioned.HostStagedComm()
            if os.environ.get("DSEA_RCCL_LIB") and os.environ.get("DSEA_DRIVER", "") != "python":
                # rehearsal of the RCCL branch: library-owned communicators over the stand-in RCCL of tests/fake_rccl
                # (ids broadcast over the gloo group), cached for the problems of this process
                if getattr(ctx, "stand_in_comm", None) is None:
                    ctx.stand_in_comm = partitioned.NativeComm.own(None, self.dev)
                comm.native_comm = ctx.stand_in_comm
        overlap = True if (self.dry or ctx.staged) else "auto"
        if os.environ.get("DSEA_BENCH_OVERLAP", "") == "off":          # stages 2 and 3 of the watchdog's ladder
            overlap = False

        def make():
            op = partitioned.PartitionedTFIMOperator(self.L, self.g, self.dev, backend=backend, comm=comm, overlap=overlap)
            if os.environ.get("DSEA_BENCH_PAIRWISE", "") == "1" and op.p > 0:
                op.use_pairwise_exchange()
            return op

        failed = torch.zeros(1, dtype=torch.float64, device=ctx.ctrl_dev)
        op = None
        try:
            op = make()
        except Exception as exc:  # noqa: BLE001
            failed[0] = 1.0
            self.notes["partitioned_driver_fallback_reason"] = "%s: %s" % (type(exc).__name__, str(exc)[:160])
        dist.all_reduce(failed)
        if failed.item() > 0:
            os.environ["DSEA_DRIVER"] = "python"
            op = make()
            self.notes["partitioned_driver_fallback"] = "library driver unavailable on %d rank(s): Python driver used" \
                                                        % int(failed.item())
        return op

    def barrier(self):
        if not self.dry:
            torch.cuda.synchronize()
        if self.partitioned:
            import torch.distributed as dist
            dist.barrier()
            if not self.dry:
                torch.cuda.synchronize()

    def activate(self):
        """(re-)bind the module-global primitive to this problem's operator (reference symeig.py:66,87: last set wins)"""
        from dominantsparseeigenad_amd import Lanczos as _LZ
        _LZ.REORTH_DEFAULT = self.reorth
        self.engine.USE_SHADOW = self.use_shadow
        self.symeig.setDominantSparseSymeig(self.A_operand, self.op.Hadjoint_to_gadjoint)
        self.f = self.symeig.DominantSparseSymeig.apply

    def step(self):
        with PinnedRandn(self.draws):
            E0, psi = self.f(self.g, self.k, self.n, self.dev)
            loss = E0 + self.dot(psi, self.tvec)
            (gl,) = torch.autograd.grad(loss, self.g)
        self.last["psi"] = psi.detach()
        return E0, gl

    def eigen_residual(self, E0, psi):
        """||H psi - E0 psi|| over all ranks: the self-check of the distributed run (outside the timed region)"""
        res = self.op.H(psi) - E0.detach() * psi
        return float(self.dot(res, res).sqrt())

    def cg_iterations(self):
        return self.op.last_cg_iters if self.partitioned else self.engine.last_cg.iters

    def first_contact(self):
        """first contact with the collectives of this stack.  The decision to leave the transposed all-to-all form
        is COLLECTIVE (an all-reduced failure flag): a rank-local fallback would leave the others in a collective"""
        if not (self.partitioned and self.op.transposed):
            return
        import torch.distributed as dist
        failed = torch.zeros(1, dtype=torch.float64, device=self.ctx.ctrl_dev)
        try:
            probe = torch.zeros(self.world * 8, dtype=torch.float64, device=self.dev)
            self.op.comm.all_to_all(probe, torch.empty_like(probe))
            if not self.dry:
                torch.cuda.synchronize()
        except Exception as exc:  # noqa: BLE001
            failed[0] = 1.0
            self.notes["distributed_fallback_reason"] = "%s: %s" % (type(exc).__name__, str(exc)[:120])
        dist.all_reduce(failed)
        if failed.item() > 0:
            self.op.use_pairwise_exchange()
            self.notes["distributed_fallback"] = "transposed exchange unavailable on %d rank(s): pairwise slab " \
                                                 "exchange used" % int(failed.item())

    def _self_check(self, E0):
        """the overlapped exchange is verified before anything is timed; if the eigen-residual is not at the level the
        sequential exchange reaches, the run falls back to the sequential exchange"""
        op, notes = self.op, self.notes
        resid = self.eigen_residual(E0, self.last["psi"])
        notes["partitioned_driver"] = getattr(op, "driver", "python")
        notes["slab_exchange"] = ("none (one rank)" if op.p == 0 else
                                  ("transposed all-to-all form" if op.transposed else "pairwise hypercube partners")
                                  + (", overlapped with the dots / correction passes" if op.overlap else ""))
        if op.p > 0 and op.overlap:
            op.overlap = False
            E0s, _ = self.step()
            resid_seq = self.eigen_residual(E0s, self.last["psi"])
            op.overlap = True
            if not (resid <= 10.0 * resid_seq + 1e-9):
                op.overlap = False
                notes["distributed_self_check"] = "overlapped exchange failed its self-check (residual %.2e vs " \
                                                  "%.2e sequential): sequential exchange timed instead" % (resid, resid_seq)
            else:
                notes["distributed_self_check"] = "overlapped exchange verified: eigen-residual %.2e (sequential " \
                                                  "%.2e), %d premise fallbacks" % (resid, resid_seq, op.overlap_fallbacks)
        else:
            notes["distributed_self_check"] = "eigen-residual %.2e" % resid

    def measure(self, steps, warmup):
        """W untimed steps, [distributed self-check], barrier, EXACTLY K timed steps, barrier; returns seconds
        (max over ranks), E0, dloss/dg"""
        self.activate()
        self.first_contact()
        E0 = gl = None
        progress("first contact done", L=self.L, k=self.k)
        for w in range(warmup):
            _simulated_hang(self.ctx, "step %d" % (w + 1))
            E0, gl = self.step()
            if not self.dry:
                torch.cuda.synchronize()
            progress("warm-up step", L=self.L, k=self.k)
        self.barrier()
        if self.partitioned:
            if warmup == 0:
                E0, gl = self.step()
            _simulated_hang(self.ctx, "step 2")
            self._self_check(E0)
            self.barrier()
            progress("self-check done", L=self.L, k=self.k)
        # ---- timed region: exactly K steps, no instrumentation inside
        t0 = time.perf_counter()
        for _ in range(steps):
            E0, gl = self.step()
        self.barrier()
        dt = time.perf_counter() - t0
        progress("timed steps done", L=self.L, k=self.k, steps=steps, seconds=round(dt, 4))
        if self.partitioned:
            import torch.distributed as dist
            tmax = torch.tensor([dt], dtype=torch.float64, device=self.ctx.ctrl_dev)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dt = tmax.item()
        return dt, E0, gl

    def time_steps(self, n):
        """one untimed + n timed steps of the CURRENT settings, max over ranks, ms per step (extras beside the headline)"""
        self.step()
        self.barrier()
        t0 = time.perf_counter()
        for _ in range(n):
            E0, gl = self.step()
        self.barrier()
        dt = time.perf_counter() - t0
        if self.partitioned:
            import torch.distributed as dist
            tmax = torch.tensor([dt], dtype=torch.float64, device=self.ctx.ctrl_dev)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dt = tmax.item()
        return dt / n * 1e3, E0, gl

    def describe(self, scaling=None):
        mode = "row-partitioned over %d GPUs%s" % (self.world, ", %s scaling" % scaling if scaling else "") \
            if self.partitioned else "one GPU"
        return "TFIM L=%d (n=2^%d, %d rows/GPU) DominantSparseSymeig k=%d fwd+bwd, g=1.0, loss=E0+psi.t, " \
               "operand=%s, %s" % (self.L, self.L, self.nloc, self.k, self.operator, mode)

    def release(self):
        """drop the operator and the arena basis (the next problem of this process may need the memory)"""
        self.op = self.A_operand = self.f = None
        self.draws = self.tvec = None
        self.last = {}
        self.engine.BasisArena.release()
        self.engine.Workspace.clear_cache()
        if not self.dry:
            torch.cuda.empty_cache()


DUMP_PSI_MAX = 1 << 22           # psi entries written in full up to this length (32 MB of float64), else a sample of as many
DUMP_SAMPLE_SEED = SEED + 99


def dump_outputs(path, prob, E0, gl):
    """--dump-outputs DIR: what the last timed step returned to its caller, as float64 .npy files -- E0.npy, dloss_dg.npy and
    psi.npy (the eigenvector in global row order; above DUMP_PSI_MAX rows the entries at a fixed, seeded set of DUMP_PSI_MAX
    indices, ascending).  Row-partitioned runs gather the slabs' entries to rank 0 (every rank calls this: collective)."""
    psi = prob.last["psi"]
    n, nloc = prob.n, prob.nloc
    lo = prob.rank * nloc if prob.partitioned else 0
    if n <= DUMP_PSI_MAX:
        part = psi.double().cpu().numpy()
    else:
        idx = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(n, DUMP_PSI_MAX, replace=False))
        mine = idx[(idx >= lo) & (idx < lo + nloc)] - lo
        part = psi[torch.from_numpy(mine).to(psi.device)].double().cpu().numpy()
    parts = [part]
    if prob.partitioned and prob.world > 1:
        import torch.distributed as dist
        parts = [None] * prob.world
        dist.all_gather_object(parts, part)
    if prob.rank != 0:
        return
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "E0.npy"), np.asarray([float(E0.item())], dtype=np.float64))
    np.save(os.path.join(path, "dloss_dg.npy"), gl.detach().double().reshape(-1).cpu().numpy())
    np.save(os.path.join(path, "psi.npy"), np.concatenate(parts).astype(np.float64))


def rank_evidence(ctx):
    """what proves the collectives span N distinct GPUs: every rank's device, gathered to rank 0"""
    import torch.distributed as dist
    mine = {"rank": ctx.rank, "local_rank": ctx.local_rank, "host": socket.gethostname(), "pid": os.getpid()}
    if not ctx.dry:
        pr = torch.cuda.get_device_properties(ctx.dev)
        mine.update(device=pr.name, pci="%04x:%02x:%02x" % (getattr(pr, "pci_domain_id", 0), getattr(pr, "pci_bus_id", 0),
                                                             getattr(pr, "pci_device_id", 0)),
                    uuid=str(getattr(pr, "uuid", "")), hbm_GB=round(pr.total_memory / 1e9, 1))
    gathered = [None] * ctx.world
    dist.all_gather_object(gathered, mine)
    info = {"world_size": dist.get_world_size(), "backend": dist.get_backend(), "ranks": gathered}
    if not ctx.dry:
        try:
            info["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:  # noqa: BLE001
            pass
        info["distinct_devices"] = len({(r["host"], r.get("pci"), r.get("uuid")) for r in gathered})
    return info


# ---------------------------------------------------------------------------------------------- command line
def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--scaling", choices=["weak", "strong"], default=None,
                    help="N > 1: time only this point (default: strong timed, weak reported beside it)")
    ap.add_argument("--L", type=int, default=None, help="chain length (default: by --gpus / --scaling)")
    ap.add_argument("--L-local", type=int, default=None, help="log2 rows per GPU (weak scaling)")
    ap.add_argument("--k", type=int, default=None)
    ap.add_argument("--shadow", choices=["auto", "on", "off"], default="auto",
                    help="bf16 storage shadow of the basis for the correction pass (DESIGN.md 4): auto = on where it fits "
                         "beside the fp64 basis (at L = 28, k = 100 on ONE GPU it does not), on = must fit, off = all-fp64 "
                         "correction pass (the reference's arithmetic)")
    ap.add_argument("--anchors-json", type=str, default=None,
                    help="N > 1: file with the N = 1 line (bench.py --gpus 1 output, or a driver record wrapping it) whose "
                         "config.one_gpu_anchors the speed-ups are quoted against (default: the cache the N = 1 run of this "
                         "sequence left on this node, else the newest committed profiles/r<NN>_bench.json)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample", action="store_true",
                    help="CPU baseline on a bounded sample (k = --cpu-k, CG capped at --cpu-cg-cap) instead of the FULL "
                         "configuration of SURVEY 8d (k as on the GPU, CG to the reference's tolerance: ~30 s of host "
                         "time at L = 20, k = 200 with 8 threads)")
    ap.add_argument("--cpu-k", type=int, default=64)
    ap.add_argument("--cpu-cg-cap", type=int, default=60)
    ap.add_argument("--cpu-threads", type=str, default="8,64",
                    help="comma-separated torch thread counts for the CPU baseline (capped at os.cpu_count(), duplicates "
                         "dropped); every run is listed in cpu_baseline.runs, the best one is reported.  Default 8 and 64 "
                         "(SURVEY 8d asks for more than one count): on the GPU box's 2 x 64-core host the reference's "
                         "torch-CPU gather mat-vec runs the full configuration in 31.5 s with 8 threads, 33.8 s with 64 and "
                         "554 s with all 256")
    ap.add_argument("--no-kernel-events", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the fp64-basis batch and the config-3 figures")
    ap.add_argument("--no-anchors", action="store_true",
                    help="N = 1: skip the live one-GPU anchors of the multi-GPU curves (L = 28 with k = 100 / k = 80 and "
                         "2^25 rows, k = 200: ~60 s and 230 GB of HBM)")
    ap.add_argument("--anchors-only", action="store_true",
                    help="N = 1: one headline step, then the live anchors (no CPU baseline, extras, PMC passes, kernel events)")
    ap.add_argument("--no-live-pmc", action="store_true",
                    help="N = 1 headline run: do not measure roofline.traffic / pmc_* live with two rocprofv3 --pmc child "
                         "passes (~20 s each) before the timed run; the newest committed profiles/r<NN>_pmc_traffic.json is "
                         "quoted instead")
    ap.add_argument("--rpl", type=int, default=0)
    ap.add_argument("--operator", choices=["matrix-free", "sell", "sell-coded", "csr"], default="matrix-free",
                    help="operand form of the TFIM operator at N=1: native matrix-free kernel (headline) or the "
                         "explicit 21-nnz/row matrix in SELL-64 / CSR layout")
    ap.add_argument("--reorth", choices=["full", "none", "partial"], default="full",
                    help="'none': basis-free two-pass Lanczos (no stored basis, no re-orthogonalisation) -- NOT the "
                         "reference's algorithm, reported for what it is; lets k = 200 at L = 28 fit one GPU.  'partial': "
                         "stored basis, re-orthogonalised only on the steps the omega recurrence selects (Simon) -- NOT the "
                         "reference's schedule either, priced with its own bytes")
    ap.add_argument("--force-partitioned", action="store_true",
                    help="run the row-partitioned driver even with one rank (measures its host overhead)")
    ap.add_argument("--dry-run-cpu", action="store_true",
                    help="CONTROL-FLOW CHECK ONLY, no measurement: the multi-rank path of this script (self-launch, "
                         "row-partitioned operator behind the reference API, collective fallback decision, exchange "
                         "self-check, max-over-ranks timing, rank-0 JSON) on CPU processes over gloo with the torch test "
                         "double of the slab kernels (tests/cpu_backend.py).  Without --L / --k the default two-point "
                         "schedule of N > 1 runs at toy sizes.  The line it prints is labelled as a dry run and carries "
                         "no roofline / cpu_baseline.")
    ap.add_argument("--host-staged", action="store_true",
                    help="REHEARSAL, no measurement: the REAL N > 1 branch of this script -- self-launch, row-partitioned "
                         "operator on the HIP slab kernels and the library-side driver, collective fallback decisions, "
                         "overlapped-exchange self-check, strong point + matched extras + weak point, rank evidence, final "
                         "line -- with the N ranks SHARING GPU 0 and the collectives over gloo staged through the host "
                         "(RCCL refuses two ranks on one device), at toy sizes.  It is how a one-GPU box executes the "
                         "P = 2 / 4 / 8 geometry end to end; the line is labelled as a rehearsal.")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step returned to its caller as DIR/<name>.npy "
                         "(float64): E0, dloss_dg and psi -- all of psi up to 2^22 entries, else a fixed, seeded sample of "
                         "2^22 of its entries in ascending index order")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beside the timed steps (live PMC passes, kernel events and "
                         "roofline, option extras, config-3 / config-4 / sweep / operand figures, one-GPU anchors, CPU "
                         "baseline, N > 1 extra points and scaling decomposition, N = 1 supervisor); --anchors-only "
                         "implies it")
    args = ap.parse_args()
    if args.anchors_only:
        args.full = True
        args.steps = args.steps or 1
        args.warmup = 1 if args.warmup is None else args.warmup
        args.no_cpu_baseline = args.no_extras = args.no_live_pmc = args.no_kernel_events = True
    if not args.full:
        args.no_cpu_baseline = args.no_extras = args.no_live_pmc = args.no_kernel_events = args.no_anchors = True
    return args


def init_process(args):
    """process-level state: ranks, device, process group, the live PMC passes (which must run BEFORE this process touches
    the GPU).  Returns a namespace ``ctx``."""
    import types
    ctx = types.SimpleNamespace()
    ctx.dry, ctx.staged = args.dry_run_cpu, args.host_staged
    if ctx.dry and ctx.staged:
        raise SystemExit("--dry-run-cpu and --host-staged exclude each other")
    env_world = os.environ.get("WORLD_SIZE")
    if args.gpus > 1 and env_world is None:
        launch_workers(args.gpus)          # does not return
    if env_world is not None and int(env_world) > 1 and os.environ.get("DSEA_BENCH_CHILD", "") != "1" and \
            os.environ.get("DSEA_BENCH_NO_WATCHDOG", "") != "1":
        # a rank started by the launcher (the driver's torchrun line or launch_workers): supervise a child that does the
        # measuring; this process never touches the GPU                                        (does not return)
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bench_watchdog
        anchors, _src = load_anchors(args)
        describe = {"metric": "DominantSparseSymeig fwd+bwd ms & HBM GB/s (TFIM, fp64)", "unit": "GB/s", "n_gpus": int(env_world),
                    "steps": args.steps, "warmup": args.warmup, "higher_is_better": True, "scaling": args.scaling or "strong",
                    "vs_baseline": None, "dtype": "f64", "data": "synthetic", "config": {"commit": _commit()}}
        bench_watchdog.supervise(os.path.abspath(__file__), sys.argv[1:], anchors, describe)
    ctx.world = int(env_world or "1")
    ctx.rank = int(os.environ.get("RANK", "0"))
    ctx.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != ctx.world:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, ctx.world))
    ctx.p = int(np.log2(ctx.world))
    assert (1 << ctx.p) == ctx.world, "world size must be a power of two"
    ctx.ranks_per_device = ctx.world if ctx.staged else 1
    ctx.live_pmc, ctx.live_pmc_note = None, None
    headline_defaults = (ctx.world == 1 and not ctx.dry and not ctx.staged and not args.force_partitioned and args.L is None
                         and args.L_local is None and args.k is None and args.operator == "matrix-free"
                         and args.reorth == "full" and args.shadow == "auto")
    # never from under a profiler: its preloaded library may already have initialised the GPU in THIS process, and a
    # process that has done so must not start other programs on this pool
    under_profiler = any(kk.startswith(("ROCPROF", "ROCP_", "ROCTRACER", "RPD_")) for kk in os.environ) or \
        "rocprof" in os.environ.get("LD_PRELOAD", "").lower() or "roctracer" in os.environ.get("LD_PRELOAD", "").lower()
    if under_profiler and headline_defaults and not args.no_live_pmc:
        ctx.live_pmc_note = "skipped: running under a profiler (newest committed profiles/r<NN>_pmc_traffic.json quoted)"
    if headline_defaults and not args.no_live_pmc and not under_profiler and not torch.cuda.is_initialized() and \
            os.environ.get("DSEA_BENCH_CHILD", "") != "1":
        # child processes, BEFORE this process initialises the GPU
        t_pmc = time.time()
        ctx.live_pmc, ctx.live_pmc_note = live_pmc_traffic()
        ctx.live_pmc_note = ctx.live_pmc_note or "two rocprofv3 --pmc passes took %.0f s" % (time.time() - t_pmc)
    if ctx.dry:
        ctx.dev = torch.device("cpu")
        torch.set_num_threads(1)
    else:
        assert torch.cuda.is_available(), "bench.py needs the MI355X; there is no CPU fallback for the product path"
        dev_index = 0 if ctx.staged else ctx.local_rank
        torch.cuda.set_device(dev_index)
        ctx.dev = torch.device("cuda", dev_index)
    # control-plane tensors (failure flags, max-over-ranks time): on the host whenever the backend is gloo
    ctx.ctrl_dev = torch.device("cpu") if (ctx.dry or ctx.staged) else ctx.dev
    ctx.partitioned_path = ctx.world > 1 or args.force_partitioned or ctx.dry or ctx.staged
    ctx.evidence = None
    if ctx.partitioned_path:
        import torch.distributed as dist
        if not dist.is_initialized():
            if ctx.world == 1:
                os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                os.environ.setdefault("MASTER_PORT", str(_free_port()))
            if ctx.dry or ctx.staged:
                dist.init_process_group("gloo", rank=ctx.rank, world_size=ctx.world)
            else:
                dist.init_process_group("nccl", rank=ctx.rank, world_size=ctx.world, device_id=ctx.dev)
        ctx.evidence = rank_evidence(ctx)
    progress("process group up", world=ctx.world)
    return ctx


def choose_point(args, ctx):
    """which (L, k) the K timed steps run, and how many of them; returns a namespace ``pt``"""
    import types
    pt = types.SimpleNamespace()
    world, p = ctx.world, ctx.p
    pt.explicit = args.L is not None or args.L_local is not None
    if world == 1:
        pt.scaling = args.scaling or "weak"
    else:
        pt.scaling = args.scaling or ("weak" if pt.explicit else "strong")
    pt.strong = pt.scaling == "strong"
    # toy sizes: the default schedule in a dry run / rehearsal (no measurement is taken from either)
    pt.toy = (ctx.dry or ctx.staged) and not pt.explicit
    if ctx.dry:
        pt.toy_strong, pt.toy_weak, pt.toy_matched_k = (10, 80), (7 + p, 60), 48
    else:                       # rehearsal on the HIP kernels: slabs of >= 2^12 rows at 8 ranks
        pt.toy_strong, pt.toy_weak, pt.toy_matched_k = (15, 80), (12 + p, 60), 48
    if args.L is not None:
        pt.L = args.L
    elif pt.strong:
        pt.L = pt.toy_strong[0] if pt.toy else 28
    elif args.L_local is not None:
        pt.L = args.L_local + p
    elif pt.toy:
        pt.L = pt.toy_weak[0]
    else:
        pt.L = 20 if world == 1 else 25 + p
    if args.k is not None:
        pt.k = args.k
    elif pt.toy:
        pt.k = pt.toy_strong[1] if pt.strong else pt.toy_weak[1]
    else:
        pt.k = STRONG_K if pt.strong else 200
    # default schedule of N > 1: the strong point is timed; the same point with the all-fp64 correction pass, the
    # shadow-matched k and the weak point are reported beside it
    pt.default_schedule = world > 1 and args.scaling is None and not pt.explicit and args.k is None and \
        args.reorth == "full" and args.shadow == "auto"
    pt.nloc, pt.n = 1 << (pt.L - (p if ctx.partitioned_path else 0)), 1 << pt.L
    pt.big = pt.nloc >= (1 << 24)
    pt.steps = args.steps if args.steps is not None else (3 if pt.big else 10)
    pt.warmup = args.warmup if args.warmup is not None else (1 if pt.big else 2)
    return pt


# ---------------------------------------------------------------------------------------------- measurements beside the headline
def kernel_events(args, ctx, pt, prob, lib):
    """per-launch durations of the dominant kernels: the same K steps again, this time with a HIP event pair recorded on
    the launch stream around every reorth / mat-vec launch (the event records cost ~4 % of a step, which is why they are
    kept out of the timed region).  Returns None or dict(launches, total_ms, steps, ms_per_step_instrumented)."""
    from dominantsparseeigenad_amd import _lib, engine
    if args.no_kernel_events or args.reorth != "full" or ctx.dry:
        return None                  # (rank 0's local kernels, also when partitioned)
    launches, total_ms = (c_int64 * 3)(), (c_double * 3)()
    ev_steps = min(pt.steps, 5) if pt.big else pt.steps
    ws = engine.Workspace.get(pt.nloc, pt.k, ctx.dev)
    _lib.check(lib.dsea_profile_begin(ws.handle, 3 * pt.k * ev_steps + 8), "dsea_profile_begin")
    t1 = time.perf_counter()
    for _ in range(ev_steps):
        prob.step()
    prob.barrier()
    dt_instr = time.perf_counter() - t1
    _lib.check(lib.dsea_profile_end(ws.handle, launches, total_ms), "dsea_profile_end")
    return {"launches": [int(v) for v in launches], "total_ms": [float(v) for v in total_ms], "steps": ev_steps,
            "ms_per_step_instrumented": dt_instr / ev_steps * 1e3}


def _rel_dev(a, b):
    return abs(a - b) / abs(b)


def option_extras(args, ctx, pt, prob, E0, gl):
    """the same workload under the options the library offers beside the reference's schedule -- reported beside the
    headline, never as the headline: basis-free two-pass Lanczos, partial re-orthogonalisation, all-fp64 correction pass"""
    from dominantsparseeigenad_amd import Lanczos as _LZ, engine
    out = {}
    if args.no_extras or args.reorth != "full":
        return out
    E0v, glv = E0.item(), float(gl.reshape(-1)[0])
    single = not ctx.partitioned_path
    if single and not pt.big:
        nb = min(pt.steps, 5)
        for tag, mode, note in (
                ("basisfree_two_pass_lanczos", "none",
                 "reorth='none' option: no stored basis, no re-orthogonalisation; not the reference's algorithm"),
                ("partial_reorth_lanczos", "partial",
                 "reorth='partial' option (Simon's partial re-orthogonalisation, threshold 1e-10): same stored basis, "
                 "re-orthogonalised only on the steps the omega recurrence selects; not the reference's schedule "
                 "(Lanczos.py:66 re-orthogonalises on every step), never the headline")):
            _LZ.REORTH_DEFAULT = mode
            try:
                ms, E0x, glx = prob.time_steps(nb)
                rec = {"ms_per_step": round(ms, 4), "E0_rel_dev_vs_full_reorth": _rel_dev(E0x.item(), E0v),
                       "dloss_dg_rel_dev_vs_full_reorth": _rel_dev(float(glx.reshape(-1)[0]), glv), "note": note}
                if mode == "partial":
                    rec.update(steps_reorthogonalised=engine.last_reorth_steps, of=pt.k - 1)
                out[tag] = rec
            except Exception as exc:  # noqa: BLE001
                out[tag] = "failed: %s" % exc
            finally:
                _LZ.REORTH_DEFAULT = "full"
    if ctx.partitioned_path and not ctx.dry and (ctx.world == 1 or os.environ.get("DSEA_BENCH_PARTIAL_EXTRA", "") == "1"):
        # row-partitioned run: the partial re-orthogonalisation option on the library driver (same collective sequence on
        # every rank, one more scalar all-reduce per step).  On more than one rank only on request
        # (DSEA_BENCH_PARTIAL_EXTRA=1): an extra must not be able to cost the line its headline.
        _LZ.REORTH_DEFAULT = "partial"
        try:
            ms, E0x, glx = prob.time_steps(2)
            out["partial_reorth_lanczos"] = {
                "ms_per_step": round(ms, 4), "steps_reorthogonalised": engine.last_reorth_steps, "of": pt.k - 1,
                "E0_rel_dev_vs_full_reorth": _rel_dev(E0x.item(), E0v),
                "dloss_dg_rel_dev_vs_full_reorth": _rel_dev(float(glx.reshape(-1)[0]), glv),
                "note": "reorth='partial' option on the row-partitioned library driver; never the headline"}
        except Exception as exc:  # noqa: BLE001  (e.g. the Python step driver: the option needs the library driver)
            if ctx.rank == 0:
                print("[bench] partial re-orthogonalisation extra skipped: %s" % exc, file=sys.stderr)
        finally:
            _LZ.REORTH_DEFAULT = "full"
    if engine.USE_SHADOW and single:
        # the same step with the all-fp64 correction pass (no bf16 shadow of the basis): the figure to hold against SURVEY
        # 8d's algorithmic bytes
        engine.USE_SHADOW = False
        try:
            ms, _, _ = prob.time_steps(min(pt.steps, 5))
            out["ms_per_step_fp64_basis"] = round(ms, 4)
        finally:
            engine.USE_SHADOW = True
    return out


def _point_record(pw, ms, steps, warmup, E0, scaling):
    m = pw.cg_iterations()
    n, k = pw.n, pw.k
    shadow_steps = (k - 1) if pw.use_shadow else 0
    return {"workload": pw.describe(scaling), "ms_per_step": round(ms, 4), "steps": steps, "warmup": warmup,
            "bf16_shadow_of_basis": bool(pw.use_shadow),
            "GBs": round(traffic_model_bytes(n, k, m, shadow_steps) / (ms * 1e-3) / 1e9, 2),
            "algorithmic_GBs": round(algorithmic_bytes(n, k, m) / (ms * 1e-3) / 1e9, 2), "cg_iterations": int(m),
            "E0_per_site": E0.item() / pw.L, "E0_per_site_closed_form": analytic_E0_per_site(pw.L, 1.0)}


def extra_point(ctx, L, k, shadow, steps, warmup, scaling):
    """one more row-partitioned point of the N > 1 schedule, timed like the headline (W untimed, self-check, K timed, max
    over ranks) -- every rank runs the same code, so an exception is collective"""
    try:
        progress("extra point", L=L, k=k, shadow=shadow, scaling=scaling)
        _simulated_hang(ctx, "extras")
        pw = Problem(ctx, L, k, True, shadow=shadow)
        dt, E0, _ = pw.measure(steps, warmup)
        rec = _point_record(pw, dt / steps * 1e3, steps, warmup, E0, scaling)
        rec.update(pw.notes)
        pw.release()
        return rec
    except Exception as exc:  # noqa: BLE001
        try:
            from dominantsparseeigenad_amd import engine
            engine.BasisArena.release()
            if not ctx.dry:
                torch.cuda.empty_cache()
        except Exception:  # noqa: BLE001
            pass
        return "failed: %s: %s" % (type(exc).__name__, str(exc)[:200])


def multi_gpu_extras(args, ctx, pt, prob, anchors):
    """default schedule of N > 1, after the timed strong point (shadow: auto = on from two GPUs): the SAME point with the
    all-fp64 correction pass, the shadow-matched k, and the weak point.  Returns (strong_fp64, strong_matched, weak)."""
    # (without --full, and in the fallback stages: timed point only)
    if not args.full or not pt.default_schedule or os.environ.get("DSEA_BENCH_REDUCED", "") == "1":
        return None, None, None
    prob.release()
    Ls = pt.L
    sw = (2, 1)
    k_m = pt.toy_matched_k if pt.toy else STRONG_K_SHADOW_MATCHED
    strong_fp64 = extra_point(ctx, Ls, pt.k, "off", sw[0], sw[1], "strong")
    strong_matched = extra_point(ctx, Ls, k_m, "auto", sw[0], sw[1], "strong")
    Lw, kw = pt.toy_weak if pt.toy else (25 + ctx.p, 200)
    weak = extra_point(ctx, Lw, kw, "auto", 2 if pt.toy else 3, 1, "weak")
    if isinstance(weak, dict):
        a = None if pt.toy else anchor_ms(anchors, "weak_2p25_rows_k200", weak["bf16_shadow_of_basis"])
        weak["one_gpu_anchor_ms"] = a
        weak["weak_efficiency_vs_anchor"] = round(a / weak["ms_per_step"], 4) if a else None
    return strong_fp64, strong_matched, weak


def one_gpu_anchors(args, ctx, pt, prob):
    """N = 1, default workload: the live one-GPU anchors of the multi-GPU curves (outside the timed steps), each with the
    arithmetic of its correction pass stated; also left in ANCHOR_CACHE for the N > 1 lines of the same sequence"""
    from dominantsparseeigenad_amd import engine
    default_headline = ctx.world == 1 and not ctx.partitioned_path and not pt.explicit and args.k is None and \
        args.operator == "matrix-free" and args.reorth == "full" and args.shadow == "auto"
    if not default_headline or args.no_anchors or ctx.dry:
        return None
    anchors = {}
    free_b, total_b = torch.cuda.mem_get_info(ctx.dev)
    for tag, La, ka, sa, shadow in ANCHOR_SPECS:
        need = 8.0 * (1 << La) * (ka + 8) * (1.25 if shadow == "on" else 1.0)
        if need > 0.9 * total_b:
            anchors[tag] = "skipped: needs %.0f GB of %.0f GB" % (need / 1e9, total_b / 1e9)
            continue
        try:
            engine.BasisArena.release()
            engine.Workspace.clear_cache()
            torch.cuda.empty_cache()
            pa = Problem(ctx, La, ka, False, shadow=shadow)
            dta, E0a, _ = pa.measure(sa, 1)
            ma = pa.cg_iterations()
            msa = dta / sa * 1e3
            anchors[tag] = {"workload": pa.describe(), "ms_per_step": round(msa, 3), "steps": sa, "warmup": 1,
                            "cg_iterations": int(ma), "bf16_shadow_of_basis": bool(pa.use_shadow),
                            "GBs": round(traffic_model_bytes(1 << La, ka, ma, (ka - 1) if pa.use_shadow else 0) / (msa * 1e-3) / 1e9, 1),
                            "algorithmic_GBs": round(algorithmic_bytes(1 << La, ka, ma) / (msa * 1e-3) / 1e9, 1),
                            "E0_per_site_minus_closed_form": E0a.item() / La - analytic_E0_per_site(La, 1.0)}
            pa.release()
        except Exception as exc:  # noqa: BLE001
            anchors[tag] = "failed: %s: %s" % (type(exc).__name__, str(exc)[:200])
            engine.BasisArena.release()
            torch.cuda.empty_cache()
    prob.activate()          # module-global primitive, shadow flag and reorth default back to the headline problem
    store_anchors(anchors)
    return anchors


# ---------------------------------------------------------------------------------------------- the JSON line
def _metric_name(args, ctx):
    if ctx.dry:
        return "DRY RUN on CPU processes (gloo, torch test double of the slab kernels): control flow of the multi-rank " \
               "bench only, not a measurement"
    if ctx.staged:
        how = ("the library's RCCL calls over the stand-in RCCL of tests/fake_rccl (DSEA_RCCL_LIB), host-side control over gloo"
               if os.environ.get("DSEA_RCCL_LIB") and os.environ.get("DSEA_DRIVER", "") != "python" else
               "collectives over gloo staged through the host")
        return "REHEARSAL, not a measurement: the N > 1 branch on the HIP slab kernels with %d ranks SHARING ONE GPU, " \
               "%s, toy sizes" % (ctx.world, how)
    if args.reorth == "full":
        return "DominantSparseSymeig fwd+bwd ms & HBM GB/s (TFIM, fp64)"
    if args.reorth == "partial":
        return "DominantSparseSymeig fwd+bwd GB/s, partial re-orthogonalisation option (TFIM, fp64; not the reference's " \
               "schedule: it re-orthogonalises on every step)"
    return "DominantSparseSymeig fwd+bwd GB/s, basis-free two-pass Lanczos option (TFIM, fp64; not the reference's " \
           "full-reorthogonalisation algorithm)"


def _priced_bytes(args, pt, m, shadow_steps, cg_persistent, pr_run_steps):
    """(bytes `value` is quoted on, algorithmic bytes, description)"""
    n, k = pt.n, pt.k
    alg = algorithmic_bytes(n, k, m)
    if args.reorth == "none":
        # the basis-free two-pass option is a DIFFERENT algorithm: it is priced with ITS OWN algorithmic bytes, not with
        # SURVEY 8d's full-reorthogonalisation figure (which it does not move).  Per Lanczos step and pass: mat-vec 2 +
        # three-term 4 + scale/store 2 vectors; the second pass also updates psi (2): 18 k vectors in all.
        b = 8.0 * n * (18 * k + 11 * m + 24)
        return b, b, "the OPTION's own bytes (18 k + 11 m + 24 vectors) / step time, all ranks"
    if args.reorth == "partial":
        # the partial re-orthogonalisation option, priced with ITS OWN bytes: every step mat-vec 2 + three-term 4 +
        # scale/store 2 vectors; a re-orthogonalised step i adds the two passes over the basis, (i + 1) + (i + 2) vectors --
        # R such steps, taken as spread evenly (mean i = k / 2); Ritz vector k + 1; backward as SURVEY 8d
        b = 8.0 * n * (8 * k + pr_run_steps * (k + 3) + (k + 1) + 11 * m + 24)
        return b, b, ("the OPTION's own bytes (every Lanczos step mat-vec 2 + three-term 4 + scale/store 2 vectors; each of "
                      "the %d re-orthogonalised steps the two passes over the basis, taken at the mean step index; Ritz "
                      "vector; backward as SURVEY 8d) / step time, all ranks" % pr_run_steps)
    b = traffic_model_bytes(n, k, m, shadow_steps, 5.0 if cg_persistent else 11.0)
    what = ("HBM bytes the step's kernels move (traffic model: SURVEY 8d per-phase count with the correction pass "
            "of %d Lanczos steps reading the bf16 shadow of the basis) / step time, all ranks" % shadow_steps)
    if args.operator != "matrix-free":
        # explicit operand (the 21-nnz/row TFIM matrix, fp64 values + int32 columns): every mat-vec also
        # streams the matrix -- k of them in the forward pass, m + 1 in the adjoint solve
        operand = 12.0 * (pt.L + 1) * n * (k + m + 1)
        b, alg = b + operand, alg + operand
        what += "; plus the explicit operand, 12 B per non-zero (%d per row) in each of the %d mat-vecs" % (pt.L + 1, k + m + 1)
    return b, alg, what


def _roofline(ctx, pt, prob, ev, pmc, lp_stats):
    launches, total_ms = ev["launches"], ev["total_ms"]
    if not (launches[0] > 0 and launches[1] > 0):
        return None
    k, nloc = pt.k, pt.nloc
    dots_b, axpy_b = reorth_bytes_per_launch(nloc, k)
    # the correction pass is priced with the bytes IT reads: bf16 shadow (2 bytes/element) when it is on
    axpy_real = axpy_b if not prob.use_shadow else sum(2.0 * i + 16.0 for i in range(1, k)) / (k - 1) * nloc
    per = {"k_rdots": (dots_b, total_ms[0] / launches[0], launches[0]),
           "k_axpy_norm": (axpy_real, total_ms[1] / launches[1], launches[1])}
    name = max(per, key=lambda kk: per[kk][1] * per[kk][2])
    b, ms, cnt = per[name]
    traffic = None
    if pmc and pt.L == 20 and k == 200:
        traffic = pmc.get(name, {}).get("hbm_bytes_per_launch")
    lp, fb = lp_stats if lp_stats is not None else (launches[1] if prob.use_shadow else 0, 0)
    return {
        "kernel": name, "bound": "hbm", "achieved": round(b / (ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS,
        "unit": "GB/s", "frac": round(b / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "traffic": traffic,
        "traffic_commit": pmc.get("_commit") if (pmc and traffic) else None,
        "avg_launch_ms": round(ms, 5), "launches": int(cnt), "launches_per_step": int(cnt) // max(ev["steps"], 1),
        "algorithmic_bytes_per_launch": b,
        "other": {kk: {"avg_launch_ms": round(v[1], 5), "achieved_GBs": round(v[0] / (v[1] * 1e-3) / 1e9, 1),
                       "bytes_per_launch": v[0]} for kk, v in per.items() if kk != name},
        "spmv_avg_launch_ms": round(total_ms[2] / max(launches[2], 1), 5),
        "measured": "HIP events on the launch stream, %d instrumented steps run right after the timed region (%.3f "
                    "ms/step with events)" % (ev["steps"], ev["ms_per_step_instrumented"]),
        "note": ("k_axpy_norm streams the bf16 shadow of the basis on %d of %d steps (fp64 fallback %d) and is priced with "
                 "the bytes it reads (2 per basis element + r in and out), not with SURVEY 8d's 8 per element"
                 % (lp, lp + fb, fb)) if not ctx.partitioned_path else "rank 0's local kernels in the row-partitioned run"}


def _cpu_baseline_block(args, pt):
    ncpu = os.cpu_count() or 1
    host = "%s, os.cpu_count()=%d" % (_cpu_model(), ncpu)
    want = []
    for t in args.cpu_threads.split(","):
        if t and min(int(t), ncpu) not in want:
            want.append(min(int(t), ncpu))
    want = want or [min(8, ncpu)]
    L, k = pt.L, pt.k
    if args.cpu_sample:
        # bounded sample of the same workload: same L, fewer Lanczos vectors, capped CG
        _, r = cpu_baseline(L, args.cpu_k, args.cpu_cg_cap, want[0])
        return {"value": r["GBs"], "unit": "GB/s", "cores": r["threads"], "kind": "port",
                "sample": "oracle (torch-CPU port of reference Lanczos.py/CG.py/TFIM.H), TFIM L=%d, k=%d Lanczos "
                          "vectors, CG capped at %d iterations (ran %d), fwd+bwd %.1f s, table build %.1f s not "
                          "timed; GB/s of the algorithmic bytes (SURVEY 8d), which is what a CPU run moves; host: %s"
                          % (L, r["k"], args.cpu_cg_cap, r["cg_iterations"], r["fwd_bwd_s"], r["table_build_s"], host)}
    # the FULL configuration (k as on the GPU, CG to the reference's tolerance)
    model, runs = None, []
    for th in want:
        model, r = cpu_baseline(L, k, None, th, model=model)
        runs.append(r)
    best = max(runs, key=lambda r: r["GBs"])
    return {"value": best["GBs"], "unit": "GB/s", "cores": best["threads"], "kind": "port",
            "sample": "oracle (torch-CPU port of reference Lanczos.py/CG.py/TFIM.H incl. the gather-table "
                      "mat-vec) on the FULL workload: TFIM L=%d, k=%d, CG to ||r||<1e-7 (%d iterations): fwd "
                      "%.1f s + bwd %.1f s; GB/s of the algorithmic bytes (SURVEY 8d); host: %s"
                      % (L, k, best["cg_iterations"], best["fwd_s"], best["bwd_s"], host),
            "ms_per_step": round(best["fwd_bwd_s"] * 1e3, 1), "runs": runs}


def _speedups(pt, ms_per_step, prob_shadow, strong_fp64, strong_matched, anchors, anchors_src):
    """config.one_gpu_anchor of an N > 1 line: every speed-up divides LIKE BY LIKE (same k, same arithmetic of the
    correction pass on both sides) and names its arithmetic; a pair whose one-GPU side is missing stays null"""
    canonical = not pt.explicit and not pt.toy
    rec = {"source": anchors_src,
           "live": "the N = 1 line of the same sequence re-measures the anchors (config.one_gpu_anchors) and leaves them "
                   "for the N > 1 lines of that sequence on the same node"}
    if pt.strong:
        k = pt.k
        a_fp64 = anchor_ms(anchors, "strong_L28_k%d" % STRONG_K, False) if canonical and k == STRONG_K else None
        a_m = anchor_ms(anchors, "strong_L28_k%d_shadow" % STRONG_K_SHADOW_MATCHED, True) if canonical else None
        ms_fp64 = strong_fp64["ms_per_step"] if isinstance(strong_fp64, dict) else (None if prob_shadow else ms_per_step)
        ms_m = strong_matched["ms_per_step"] if isinstance(strong_matched, dict) and strong_matched.get("bf16_shadow_of_basis") else None
        rec.update({
            "strong_k%d_fp64_basis_one_gpu_ms" % STRONG_K: a_fp64,
            "strong_k%d_fp64_basis_ms" % STRONG_K: ms_fp64,
            "speedup_vs_one_gpu_fp64_basis": round(a_fp64 / ms_fp64, 4) if (a_fp64 and ms_fp64) else None,
            "speedup_vs_one_gpu_fp64_basis_is": "L = 28, k = %d, all-fp64 correction pass on BOTH sides (the one GPU cannot "
                                                "hold the bf16 shadow beside its 215 GB basis)" % STRONG_K,
            "strong_k%d_shadow_one_gpu_ms" % STRONG_K_SHADOW_MATCHED: a_m,
            "strong_k%d_shadow_ms" % STRONG_K_SHADOW_MATCHED: ms_m,
            "speedup_vs_one_gpu_k%d_shadow" % STRONG_K_SHADOW_MATCHED: round(a_m / ms_m, 4) if (a_m and ms_m) else None,
            "speedup_vs_one_gpu_k%d_shadow_is" % STRONG_K_SHADOW_MATCHED:
                "L = 28, k = %d, bf16 shadow of the basis on BOTH sides (the largest round k at which it fits one GPU)"
                % STRONG_K_SHADOW_MATCHED,
            "timed_point_note": "value / ms_per_step of this line: k = %d with the shadow %s -- NOT divided into the fp64 "
                                "one-GPU anchor" % (k, "on" if prob_shadow else "off")})
    else:
        a = anchor_ms(anchors, "weak_2p25_rows_k200", prob_shadow) if canonical and pt.k == 200 and pt.nloc == (1 << 25) else None
        rec.update({"weak_one_gpu_ms": a, "weak_efficiency": round(a / ms_per_step, 4) if a else None,
                    "weak_efficiency_is": "2^25 rows per GPU, k = 200, bf16 shadow %s on both sides" % ("on" if prob_shadow else "off")})
    return rec


def _supervise_one_gpu(args):
    """N = 1: run the measurement in a CHILD and relay its line; if the child dies (a GPU hang surfaced once in ~20 default runs
    of round 6 as an abort with "HW Exception ... GPU Hang" and an EMPTY stdout -- cause not found, not reproduced in 14 further
    runs, docs/design/12-round6.md 12.8) or stalls, a fresh child measures again without the parts that are not the number
    (live PMC passes, extras).  The line then says so (config.supervisor).  This process never touches the GPU.  Not used under a
    profiler (its preloaded library has initialised the GPU here: no child processes then), without --full, for N > 1
    (tools/bench_watchdog.py supervises those), for the CPU dry run / host-staged rehearsal, or with DSEA_BENCH_NO_WATCHDOG=1."""
    import signal
    import subprocess
    if not args.full or args.gpus != 1 or os.environ.get("WORLD_SIZE") is not None or args.dry_run_cpu or args.host_staged:
        return
    if os.environ.get("DSEA_BENCH_SUPERVISED", "") == "1" or os.environ.get("DSEA_BENCH_NO_WATCHDOG", "") == "1" or \
            os.environ.get("DSEA_BENCH_CHILD", "") == "1":
        return
    if any(kk.startswith(("ROCPROF", "ROCP_", "ROCTRACER", "RPD_")) for kk in os.environ) or \
            "rocprof" in os.environ.get("LD_PRELOAD", "").lower() or "roctracer" in os.environ.get("LD_PRELOAD", "").lower():
        return
    argv = sys.argv[1:]
    plans = [(argv, 1200), (argv + [a for a in ("--no-live-pmc", "--no-extras") if a not in argv], 900)]
    failures = []
    for attempt, (child_argv, limit_s) in enumerate(plans, 1):
        env = dict(os.environ, DSEA_BENCH_SUPERVISED="1")
        proc = subprocess.Popen([sys.executable, os.path.abspath(__file__)] + child_argv, stdout=subprocess.PIPE, text=True, env=env,
                                start_new_session=True)
        try:
            out, _ = proc.communicate(timeout=limit_s)
            rc = proc.returncode
        except subprocess.TimeoutExpired:
            try:
                os.killpg(proc.pid, signal.SIGKILL)
            except (ProcessLookupError, PermissionError):
                pass
            out, _ = proc.communicate()
            rc = "no line after %d s (killed)" % limit_s
        lines = [ln for ln in (out or "").splitlines() if ln.strip()]
        final = lines[-1] if lines and lines[-1].startswith("{") and '"metric"' in lines[-1] else None
        for ln in lines[:-1] if final else lines:          # anything else the child printed goes to stderr: ONE line on stdout
            print(ln, file=sys.stderr)
        if rc == 0 and final is not None:
            if failures:
                try:
                    rec = json.loads(final)
                    rec.setdefault("config", {})["supervisor"] = {
                        "attempt": attempt, "earlier_attempts": failures,
                        "note": "an earlier measuring process died or stalled; this line is from a fresh one" +
                                (" run without the live PMC passes and the extras" if child_argv != argv else "")}
                    final = json.dumps(rec)
                except ValueError:
                    pass
            print(final, flush=True)
            sys.exit(0)
        failures.append("attempt %d: exit %s, %s" % (attempt, rc, "no JSON line" if final is None else "line present"))
        print("bench.py supervisor: %s" % failures[-1], file=sys.stderr, flush=True)
    sys.exit(1)


def main():
    args = parse_args()
    _supervise_one_gpu(args)           # N = 1: returns in the measuring child (and under a profiler); does not return in the parent
    ctx = init_process(args)
    dry, world, rank = ctx.dry, ctx.world, ctx.rank
    from dominantsparseeigenad_amd import _lib, engine
    lib = None if dry else _lib.load()
    pt = choose_point(args, ctx)
    L, k = pt.L, pt.k
    if os.environ.get("DSEA_PLACEMENT_TRIES"):
        engine.BasisArena.PLACEMENT_TRIES = int(os.environ["DSEA_PLACEMENT_TRIES"])

    # ---- the timed point
    prob = Problem(ctx, L, k, ctx.partitioned_path, reorth=args.reorth, shadow=args.shadow, operator=args.operator)
    if args.rpl and not dry:
        engine.Workspace.get(pt.nloc, k, ctx.dev).set_rows_per_lane(args.rpl)
    dt, E0, gl = prob.measure(pt.steps, pt.warmup)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, prob, E0, gl)
    if os.environ.get("DSEA_BENCH_INJECT_ABORT", "") == "1" and os.environ.get("DSEA_BENCH_SUPERVISED", "") == "1" and \
            not args.no_extras:
        os.abort()       # TEST HOOK (tests/test_gpu_bench_contract.py): what a GPU hang does to the measuring process -- SIGABRT, no line
    notes = dict(prob.notes)
    m = prob.cg_iterations()
    ms_per_step = dt / pt.steps * 1e3
    ev = kernel_events(args, ctx, pt, prob, lib)
    lp_stats = engine.lanczos_lp_stats(pt.nloc, ctx.dev) if not ctx.partitioned_path else None
    pr_run_steps = int(engine.last_reorth_steps or 0) if args.reorth == "partial" else None
    extras = option_extras(args, ctx, pt, prob, E0, gl)
    shadow_steps = int(lp_stats[0]) if lp_stats is not None else ((k - 1) if (prob.use_shadow and k > 1) else 0)
    # the adjoint solve runs as one persistent launch for the full-space TFIM operator up to 2^20 rows
    cg_persistent = (not ctx.partitioned_path) and args.operator == "matrix-free" and 11 <= L <= 20 and \
        os.environ.get("DSEA_NO_PERSIST", "") != "1"
    total_bytes, alg_bytes, value_is = _priced_bytes(args, pt, m, shadow_steps, cg_persistent, pr_run_steps)
    value = total_bytes / (ms_per_step * 1e-3) / 1e9
    workload = prob.describe(pt.scaling if world > 1 else None)
    E0_site, gl0 = E0.item() / L, float(gl.reshape(-1)[0].item())
    overlap_fb = prob.op.overlap_fallbacks if ctx.partitioned_path else None
    prob_shadow = bool(prob.use_shadow)
    if rank == 0 and world > 1:
        # the timed point is complete: leave it with the supervisor, so that a stall in what runs BESIDE it (extras, tear-down)
        # cannot cost the number
        progress("provisional_line", line={
            "metric": _metric_name(args, ctx), "value": round(value, 2), "unit": "GB/s", "n_gpus": world, "steps": pt.steps,
            "warmup": pt.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": pt.scaling,
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": dict(notes, workload=workload, value_is=value_is, cg_iterations=int(m), bf16_shadow_of_basis=prob_shadow,
                           E0_per_site=E0_site, E0_per_site_closed_form=analytic_E0_per_site(L, 1.0), dloss_dg=gl0,
                           commit=_commit(), collectives=ctx.evidence, provisional=True)})

    # ---- beside the timed point: N > 1 default schedule / N = 1 anchors
    anchors_in, anchors_src = load_anchors(args) if (world > 1 and args.full) else ({}, None)
    decomposition = None
    if world > 1 and args.full:
        # what bounds this line: collectives on the run's own communicators, exposed exchange per step / iteration,
        # SURVEY 8e's model beside the measurement (tools/bench_multi.py; outside the timed region, collective)
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bench_multi
        canonical = not pt.explicit and not pt.toy
        tag = ("strong_L28_k%d" % STRONG_K if (pt.strong and k == STRONG_K and not prob_shadow) else
               "strong_L28_k%d_shadow" % STRONG_K_SHADOW_MATCHED if (pt.strong and k == STRONG_K_SHADOW_MATCHED and prob_shadow) else
               "weak_2p25_rows_k200" if (not pt.strong and k == 200 and pt.nloc == (1 << 25)) else None)
        a1 = anchor_ms(anchors_in, tag, prob_shadow) if (canonical and tag) else None
        if a1 and not pt.strong:
            a1 = a1 * world          # weak point: T_1 of the N-fold problem (the model divides it by P again)
        progress("scaling decomposition")
        try:
            decomposition = bench_multi.scaling_decomposition(ctx, prob, pt, ms_per_step, m, E0, a1)
        except Exception as exc:  # noqa: BLE001  (every rank runs the same code: the exception is collective)
            decomposition = "failed: %s: %s" % (type(exc).__name__, str(exc)[:200])
        progress("scaling decomposition done")
    strong_fp64, strong_matched, weak_point = multi_gpu_extras(args, ctx, pt, prob, anchors_in)
    anchors = one_gpu_anchors(args, ctx, pt, prob)

    final_line = None
    if rank == 0:
        cfg = {"workload": workload, "value_is": value_is, "cg_iterations": int(m),
               "cg_form": "persistent single launch (x, r, d in registers)" if cg_persistent
               else "streaming (mat-vec, update, direction launches)",
               "traffic_model_bytes_per_step": total_bytes,
               "frac_of_hbm_peak": round(value / (HBM_PEAK_GBS * world), 4),
               "algorithmic_bytes_per_step": alg_bytes,
               "algorithmic_GBs": round(alg_bytes / (ms_per_step * 1e-3) / 1e9, 2),
               "algorithmic_GBs_note": "SURVEY 8d figure: bytes of the REFERENCE's algorithm (all-fp64 basis) / step time; it "
                                       "may exceed the HBM peak because the implementation moves fewer bytes -- not a "
                                       "roofline fraction",
               "ms_at_hbm_peak_for_algorithmic_bytes": round(alg_bytes / (HBM_PEAK_GBS * world * 1e9) * 1e3, 3),
               "bf16_shadow_of_basis": prob_shadow, "shadow_policy": args.shadow,
               "lanczos_reorthogonalisation": args.reorth,
               **({"steps_reorthogonalised": pr_run_steps, "of": k - 1} if pr_run_steps is not None else {}),
               "E0_per_site": E0_site, "E0_per_site_closed_form": analytic_E0_per_site(L, 1.0), "dloss_dg": gl0,
               "adjoint_vs_reference_at_eps1e-7": ADJOINT_DEV_EPS7, "commit": _commit(),
               "basis_placement_probe_us": [round(t, 1) for t in (engine.BasisArena.last_placement or [])]}
        out = {"metric": _metric_name(args, ctx), "value": round(value, 2), "unit": "GB/s", "n_gpus": world,
               "steps": pt.steps, "warmup": pt.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True,
               "scaling": pt.scaling if (world > 1 or ctx.partitioned_path) else "none", "vs_baseline": None, "dtype": "f64",
               "data": "synthetic", "config": cfg}
        cfg.update(notes)
        if os.environ.get("DSEA_BENCH_STAGE"):
            cfg["ladder_stage_env"] = {kk: os.environ[kk] for kk in ("DSEA_BENCH_STAGE", "DSEA_COMM_SINGLE", "DSEA_BENCH_OVERLAP",
                                                                    "DSEA_BENCH_PAIRWISE", "DSEA_DRIVER", "DSEA_BENCH_REDUCED")
                                       if kk in os.environ}
        if ctx.evidence is not None:
            cfg["collectives"] = ctx.evidence
            if ctx.staged:
                cfg["collectives"]["note"] = "rehearsal: all ranks share GPU 0 (distinct_devices = 1 is expected)"
        if world > 1:
            if args.full:
                cfg["one_gpu_anchor"] = _speedups(pt, ms_per_step, prob_shadow, strong_fp64, strong_matched, anchors_in,
                                                  anchors_src)
            if strong_fp64 is not None:
                cfg["strong_point_fp64_basis"] = strong_fp64
            if strong_matched is not None:
                cfg["strong_point_shadow_matched_k"] = strong_matched
            if weak_point is not None:
                cfg["weak_scaling_point"] = weak_point
            if overlap_fb is not None:
                cfg["overlap_premise_fallbacks"] = int(overlap_fb)
            if isinstance(decomposition, dict) and isinstance(strong_fp64, dict):
                # the like-by-like pair the strong point has (all-fp64 correction pass on both sides), same k, same collectives
                a_fp64 = anchor_ms(anchors_in, "strong_L28_k%d" % STRONG_K, False) if (not pt.explicit and not pt.toy) else None
                decomposition["model"]["strong_point_fp64_basis"] = bench_multi.model_entry(
                    a_fp64, strong_fp64["ms_per_step"], world, decomposition["communication_ms_per_step"])
            if args.full:
                cfg["scaling_decomposition"] = decomposition
        if world == 1 and not ctx.partitioned_path:
            cfg["multi_gpu_schedule"] = (
                "bench.py --gpus N (N > 1) times the STRONG point TFIM L=28, k=%d over N GPUs as value/ms_per_step (shadow "
                "auto = on), then the same point with the all-fp64 correction pass, L=28 k=%d with the shadow, and the WEAK "
                "point (2^25 rows/GPU, k=200); config.one_gpu_anchors of this line are their one-GPU sides, each with the "
                "arithmetic of its correction pass -- speed-ups divide like by like only"
                % (STRONG_K, STRONG_K_SHADOW_MATCHED))
        if anchors is not None:
            cfg["one_gpu_anchors"] = anchors
        import glob
        stored = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_pmc_traffic.json")))
        tpath = stored[-1] if stored else ""       # the newest committed round file
        pmc = ctx.live_pmc
        if ctx.live_pmc_note:
            cfg["pmc_live"] = ctx.live_pmc_note
        if pmc is None and os.path.exists(tpath):
            try:
                pmc = json.load(open(tpath))
            except Exception:  # noqa: BLE001
                pmc = None
        if args.full and not ctx.partitioned_path and L == 20 and k == 200 and args.operator == "matrix-free":
            # the traffic model against the counters: bytes that crossed the HBM interface in a profiled run of this step
            if pmc and pmc.get("_total_hbm_bytes_per_step"):
                real = float(pmc["_total_hbm_bytes_per_step"])
                cfg["pmc_hbm_bytes_per_step"] = real
                cfg["pmc_source"] = ("rocprofv3 PMC FETCH_SIZE/WRITE_SIZE measured in THIS run (child processes, same box)"
                                     if pmc.get("_commit") == "live" else
                                     "rocprofv3 PMC FETCH_SIZE/WRITE_SIZE at commit %s (committed file %s)"
                                     % (pmc.get("_commit", "?"), os.path.basename(tpath)))
                cfg["pmc_GBs"] = round(real / (ms_per_step * 1e-3) / 1e9, 2)
                cfg["frac_of_hbm_peak_pmc_traffic"] = round(real / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        for key in ("basisfree_two_pass_lanczos", "partial_reorth_lanczos"):
            if key in extras:
                cfg[key] = extras[key]
        if "ms_per_step_fp64_basis" in extras:
            cfg["ms_per_step_fp64_basis"] = extras["ms_per_step_fp64_basis"]
            cfg["GBs_fp64_basis"] = round(alg_bytes / (extras["ms_per_step_fp64_basis"] * 1e-3) / 1e9, 2)
        if ev is not None:
            roof = _roofline(ctx, pt, prob, ev, pmc, lp_stats)
            if roof is not None:
                out["roofline"] = roof
        if not args.no_extras and world == 1 and not ctx.partitioned_path and not pt.big:
            try:
                progress("extra: measured_ceilings")
                ceil = measured_ceilings(ctx.dev)
                cfg["measured_ceilings"] = ceil
                if "roofline" in out:
                    out["roofline"]["frac_of_measured_read_ceiling"] = round(out["roofline"]["achieved"] / ceil["read_GBs"], 4)
            except Exception as exc:  # noqa: BLE001
                cfg["measured_ceilings"] = "failed: %s" % exc
            try:
                progress("extra: config3")
                cfg["config3"] = c3_figures(ctx.dev)
            except Exception as exc:  # noqa: BLE001
                cfg["config3"] = "failed: %s" % exc
            try:
                progress("extra: config4")
                cfg["config4"] = c4_figures(ctx.dev)
            except Exception as exc:  # noqa: BLE001
                cfg["config4"] = "failed: %s" % exc
            if L == 20 and k == 200 and args.operator == "matrix-free" and args.reorth == "full":
                try:
                    progress("extra: sweep_N20")
                    cfg["sweep_N20"] = sweep_figures(ctx.dev)
                except Exception as exc:  # noqa: BLE001
                    cfg["sweep_N20"] = "failed: %s: %s" % (type(exc).__name__, exc)
                try:
                    progress("extra: operand_sell")
                    cfg["operand_sell"] = sell_operand_figures(ctx, args)
                except Exception as exc:  # noqa: BLE001
                    cfg["operand_sell"] = "failed: %s: %s" % (type(exc).__name__, exc)
                try:
                    progress("extra: callable_operand")
                    cfg["callable_operand"] = callable_operand_figures(ctx, args, ms_per_step)
                except Exception as exc:  # noqa: BLE001
                    cfg["callable_operand"] = "failed: %s: %s" % (type(exc).__name__, exc)
                prob.activate()
        if not args.no_cpu_baseline and world == 1 and not pt.big and not ctx.staged:
            progress("cpu baseline")
            out["cpu_baseline"] = _cpu_baseline_block(args, pt)
        # RCCL / HIP runtime banners go through C stdio: flush them first so the JSON is the last line
        import ctypes
        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:  # noqa: BLE001
            pass
        sys.stdout.flush()
        final_line = json.dumps(out)
    if ctx.partitioned_path:
        import torch.distributed as dist
        dist.barrier()
        prob.release()
        try:
            from dominantsparseeigenad_amd import partitioned
            partitioned.NativeComm.release_all()
            if getattr(ctx, "stand_in_comm", None) is not None:
                ctx.stand_in_comm.close()
        except Exception:  # noqa: BLE001
            pass
        dist.destroy_process_group()
    if final_line is not None:
        print(final_line, flush=True)


if __name__ == "__main__":
    main()
