"""bench.py contract on a small workload: ONE JSON line as the last line of stdout, the required keys, the roofline
and cpu_baseline objects, and the row-partitioned code path (one rank over RCCL)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
from conftest import ROOT  # noqa: E402

REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config"}


def _run(extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--L-local", "14", "--k", "48", "--steps", "2",
           "--warmup", "1", "--cpu-k", "8", "--cpu-cg-cap", "5"] + extra
    # (the N = 1 supervisor of bench.py -- a child measures, the parent relays its line -- has its own test below; the other
    #  cases run the measuring process directly: one interpreter start less per case)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29561")
    env.setdefault("DSEA_BENCH_NO_WATCHDOG", "1")
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.strip().splitlines() if ln.strip()]
    return json.loads(lines[-1])          # the JSON line must be the LAST line


def test_bench_line_single_gpu():
    d = _run(["--full"])
    assert REQUIRED <= set(d) and d["n_gpus"] == 1 and d["dtype"] == "f64" and d["vs_baseline"] is None
    assert d["value"] > 0 and d["ms_per_step"] > 0 and "workload" in d["config"]
    assert abs(d["config"]["E0_per_site"] - d["config"]["E0_per_site_closed_form"]) < 1e-9
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    # the line must survive a peak check: `value` counts bytes the kernels move, a fraction is a fraction, and the
    # dominant kernel's launches fit into the step they belong to
    assert d["value"] <= r["peak"] * d["n_gpus"] and 0 < d["config"]["frac_of_hbm_peak"] <= 1.0
    assert 0 < r["frac"] <= 1.0
    assert r["avg_launch_ms"] * r["launches_per_step"] <= d["ms_per_step"] * 1.1
    assert d["config"]["algorithmic_GBs"] >= d["value"] and "frac_of_hbm_peak_whole_step" not in d["config"]
    assert d["config"]["traffic_model_bytes_per_step"] <= d["config"]["algorithmic_bytes_per_step"]
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and "sample" in c


def test_bench_one_gpu_supervisor_relays_the_line_and_survives_a_dead_measuring_process():
    """N = 1: bench.py measures in a child and relays its ONE line; a child that dies without a line (what the GPU hang of
    round 6 did: SIGABRT, empty stdout) is replaced by a fresh one that measures without the live PMC passes and the extras, and
    the line says so."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--L-local", "14", "--k", "48", "--steps", "2", "--warmup", "1",
           "--full", "--no-cpu-baseline", "--no-anchors"]
    env = {k: v for k, v in os.environ.items() if k != "DSEA_BENCH_NO_WATCHDOG"}
    ok = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert ok.returncode == 0, ok.stderr[-2000:]
    lines = [ln for ln in ok.stdout.strip().splitlines() if ln.strip()]
    assert len(lines) == 1 and "supervisor" not in json.loads(lines[0])["config"] and "config3" in json.loads(lines[0])["config"]
    bad = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(env, DSEA_BENCH_INJECT_ABORT="1"), cwd=ROOT)
    assert bad.returncode == 0, bad.stderr[-2000:]
    lines = [ln for ln in bad.stdout.strip().splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    sup = d["config"]["supervisor"]
    assert sup["attempt"] == 2 and "attempt 1: exit -6" in sup["earlier_attempts"][0] and "config3" not in d["config"]
    assert d["ms_per_step"] > 0 and abs(d["config"]["E0_per_site"] - d["config"]["E0_per_site_closed_form"]) < 1e-9
    assert "attempt 1" in bad.stderr


def test_plain_line_and_dumped_outputs(tmp_path):
    """without --full the line carries the timed point only (nothing measured beside it); --dump-outputs writes what the last
    timed step returned -- E0, dloss/dg, the eigenvector -- as float64, and a second run with the same arguments writes the same"""
    import numpy as np
    dumps = []
    for run in (1, 2):
        out = tmp_path / ("run%d" % run)
        d = _run(["--dump-outputs", str(out)])
        assert REQUIRED <= set(d) and d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0
        assert "roofline" not in d and "cpu_baseline" not in d
        assert not {"config3", "config4", "measured_ceilings", "ms_per_step_fp64_basis", "one_gpu_anchors"} & set(d["config"])
        got = {name: np.load(str(out / (name + ".npy"))) for name in ("E0", "dloss_dg", "psi")}
        assert all(v.dtype == np.float64 for v in got.values()) and got["psi"].shape == (1 << 14,)
        assert abs(got["E0"][0] / 14 - d["config"]["E0_per_site"]) < 1e-12 and got["dloss_dg"][0] == d["config"]["dloss_dg"]
        assert abs(np.linalg.norm(got["psi"]) - 1.0) < 1e-10
        dumps.append(got)
    for name in ("E0", "dloss_dg", "psi"):
        np.testing.assert_allclose(dumps[1][name], dumps[0][name], rtol=0, atol=1e-12)


def test_bench_line_cpu_baseline_forms():
    d = _run(["--full", "--cpu-threads", "4", "--no-extras"])
    assert "FULL workload" in d["cpu_baseline"]["sample"] and "config3" not in d["config"]
    assert d["cpu_baseline"]["runs"][0]["threads"] == 4
    d = _run(["--full", "--cpu-sample", "--no-extras"])
    assert "capped" in d["cpu_baseline"]["sample"]


def test_bench_line_carries_honest_extras():
    """the all-fp64-basis step time next to the headline, and the config-3 figures driver-timed"""
    d = _run(["--full", "--no-cpu-baseline"])
    assert d["config"]["ms_per_step_fp64_basis"] > 0 and d["config"]["bf16_shadow_of_basis"] is True
    c3 = d["config"]["config3"]
    assert c3["cg_iterations"] == 1000 and c3["cg_us_per_iteration"] > 0 and c3["lanczos_k300_ms"] > 0
    # BASELINE configs[3] (transfer matrix D = 512, DominantSparseEig k = 200): the mat-vec on the fp64 matrix cores
    c4 = d["config"]["config4"]
    assert 0 < c4["matvec_us"] < 200 and c4["forward_ms"] > 0 and c4["backward_ms"] > 0 and c4["eigen_residual"] < 1e-10
    assert 0 < c4["matvec_TFLOPs_fp64"] < 80.0               # (dense fp64 MFMA peak of the chip)
    # the box's own copy / read ceilings beside the spec peak; the dominant kernel cannot beat a read-only stream by much
    ceil = d["config"]["measured_ceilings"]
    assert 2000.0 < ceil["copy_GBs"] <= 8000.0 and 2000.0 < ceil["read_GBs"] <= 8000.0
    assert 0.0 < d["roofline"]["frac_of_measured_read_ceiling"] < 1.5


def test_bench_line_of_the_partial_reorthogonalisation_option():
    """--reorth partial: labelled as an option (not the reference's schedule), priced with its own bytes, steps in the line"""
    d = _run(["--reorth", "partial", "--no-cpu-baseline", "--no-extras"])
    assert "partial re-orthogonalisation option" in d["metric"] and "not the reference" in d["metric"]
    c = d["config"]
    assert c["lanczos_reorthogonalisation"] == "partial" and c["bf16_shadow_of_basis"] is False
    assert 0 <= c["steps_reorthogonalised"] <= c["of"] and "OPTION's own bytes" in c["value_is"]
    assert 0.0 < d["value"] <= 8000.0 and d["ms_per_step"] > 0


def test_bench_line_partitioned_path():
    d = _run(["--force-partitioned", "--no-cpu-baseline"])
    assert REQUIRED <= set(d) and d["scaling"] == "weak"
    assert "distributed_self_check" in d["config"]
    assert abs(d["config"]["E0_per_site"] - d["config"]["E0_per_site_closed_form"]) < 1e-9


def test_headline_line_measures_its_pmc_traffic_live():
    """The default N = 1 workload (BASELINE configs[1]) measures roofline.traffic in the run itself: two rocprofv3 --pmc
    child passes (FETCH_SIZE, WRITE_SIZE, separate, --kernel-trace only) started before the process touches the GPU.
    The dominant kernel's HBM traffic equals its algorithmic bytes to a few per cent (no wasted re-reads)."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline",
           "--no-extras", "--no-anchors"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.strip().splitlines() if ln.strip()][-1])
    r, c = d["roofline"], d["config"]
    assert "L=20" in c["workload"] and r["kernel"] == "k_rdots"
    assert r["traffic_commit"] == "live", c.get("pmc_live")
    assert 0.98 * r["algorithmic_bytes_per_launch"] < r["traffic"] < 1.05 * r["algorithmic_bytes_per_launch"]
    assert "THIS run" in c["pmc_source"] and 0.9 < c["pmc_hbm_bytes_per_step"] / c["traffic_model_bytes_per_step"] < 1.15
    assert d["value"] <= 8000.0 and 0 < r["frac"] <= 1.0


def _bench(argv, env=None, timeout=1500):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + argv
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    e.update(env or {})
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=e, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    lines = [ln for ln in out.stdout.strip().splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1 and out.stdout.strip().splitlines()[-1] == lines[0]
    return json.loads(lines[0])


@pytest.mark.parametrize("world", [2, 4, 8])
def test_bench_multi_gpu_branch_rehearsal_on_hip_kernels(world):
    """``bench.py --gpus N --host-staged``: the REAL N > 1 branch of the script (self-launch of N workers, row-partitioned
    operator on the HIP slab kernels with the library-side driver through the callback communicator, collective fallback
    decisions, overlapped-exchange self-check, strong point + fp64 / shadow-matched extras + weak point, rank evidence,
    one final JSON line) with the N ranks sharing the one GPU of this box at toy sizes.  N = 8 is the p = 3 geometry of
    BASELINE configs[4]: transposed exchange with three far bits.  A rehearsal, labelled as such -- no measurement."""
    # N = 8 (eight processes time-slicing one GPU: 82 s with the full schedule) runs the timed strong point only -- the extras
    # beside it (fp64 / shadow-matched / weak points, scaling decomposition) are the same code at N = 2 and N = 4
    reduced = world >= 8
    d = _bench(["--gpus", str(world), "--host-staged", "--steps", "2", "--warmup", "1", "--full"],
               env={"DSEA_BENCH_REDUCED": "1"} if reduced else None)
    assert d["metric"].startswith("REHEARSAL") and d["n_gpus"] == world and d["scaling"] == "strong"
    assert "roofline" not in d or d["roofline"]["frac"] <= 1.0
    cfg = d["config"]
    assert cfg["partitioned_driver"].startswith("library (callbacks"), cfg["partitioned_driver"]
    assert ("transposed" if world >= 4 else "pairwise") in cfg["slab_exchange"] and "overlapped" in cfg["slab_exchange"]
    assert cfg["distributed_self_check"].startswith("overlapped exchange verified"), cfg["distributed_self_check"]
    assert abs(cfg["E0_per_site"] - cfg["E0_per_site_closed_form"]) < 1e-9
    col = cfg["collectives"]
    assert col["world_size"] == world and sorted(r["rank"] for r in col["ranks"]) == list(range(world))
    assert len({r["pid"] for r in col["ranks"]}) == world and col["distinct_devices"] == 1
    assert cfg["fallback_stage"] == 1 and cfg["watchdog"]["stages"][0]["outcome"] == "completed"
    if reduced:
        return
    for key in ("strong_point_fp64_basis", "strong_point_shadow_matched_k", "weak_scaling_point"):
        rec = cfg[key]
        assert isinstance(rec, dict), (key, rec)
        # (toy Krylov dimensions: the shadow-matched k = 48 and the weak point's k = 60 are not converged to 1e-9)
        assert rec["ms_per_step"] > 0 and abs(rec["E0_per_site"] - rec["E0_per_site_closed_form"]) < 1e-6, (key, rec)
        assert rec["partitioned_driver"].startswith("library (callbacks") and "verified" in rec["distributed_self_check"]
    assert cfg["strong_point_fp64_basis"]["bf16_shadow_of_basis"] is False and cfg["bf16_shadow_of_basis"] is True
    sd = cfg["scaling_decomposition"]          # what bounds the line: tools/bench_multi.py
    assert sd["allreduce_us"]["8_bytes"] > 0 and sd["allreduce_us"]["1600_bytes"] > 0 and "library" in sd["allreduce_us"]["through"]
    assert sd["exchange"]["ms_per_matvec"] > 0 and sd["exchange"]["GBs_sent_per_gpu"] > 0
    assert sd["exposed_exchange_ms_per_lanczos_step"] >= 0 and sd["exposed_exchange_ms_per_cg_iteration"] >= 0
    assert sd["lanczos_forward_ms"]["exchange_after_correction"] > 0 and sd["lanczos_forward_ms"]["without_exchange"] > 0
    for key in ("timed_point", "strong_point_fp64_basis"):
        assert "predicted_speedup" in sd["model"][key] and "measured_speedup" in sd["model"][key]
    assert cfg["fallback_stage"] == 1 and cfg["watchdog"]["stages"][0]["outcome"] == "completed"
    anchor = cfg["one_gpu_anchor"]
    assert "speedup_vs_one_gpu" not in anchor and "speedup_vs_one_gpu_fp64_basis" in anchor
    assert "speedup_vs_one_gpu_k80_shadow" in anchor


@pytest.mark.parametrize("mode,word", [("own", "library-owned"), ("adopt", "adopted")])
def test_bench_partitioned_branch_with_library_owned_and_adopted_rccl_communicators(mode, word):
    """DSEA_COMM=own|adopt through bench.py's partitioned branch (one rank over RCCL: the communicator pair is created by
    dsea_comm_unique_id + dsea_comm_init_rank, or adopted from torch's ProcessGroupNCCL) -- the fallback a torch build
    without ProcessGroupNCCL._comm_ptr would take must not be met first on the 8-GPU node."""
    d = _bench(["--force-partitioned", "--L-local", "14", "--k", "48", "--steps", "2", "--warmup", "1",
                "--no-cpu-baseline", "--no-extras"], env={"DSEA_COMM": mode})
    cfg = d["config"]
    assert word in cfg["partitioned_driver"] and cfg["partitioned_driver"].startswith("library (rccl"), cfg["partitioned_driver"]
    assert abs(cfg["E0_per_site"] - cfg["E0_per_site_closed_form"]) < 1e-9


def test_bench_shadow_switch():
    """--shadow off: the all-fp64 correction pass is what is timed and what the line says"""
    d = _bench(["--L-local", "14", "--k", "48", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-extras",
                "--shadow", "off"])
    assert d["config"]["bf16_shadow_of_basis"] is False and d["config"]["shadow_policy"] == "off"
    assert "0 Lanczos steps reading the bf16 shadow" in d["config"]["value_is"]


FAKE_RCCL = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")


@pytest.mark.parametrize("inject,stage,driver", [(None, 1, "library (rccl (library-owned, two communicators"),
                                                 ("exchange", 2, "library (rccl (library-owned, one communicator"),
                                                 ("allreduce", 3, "python")])
def test_bench_watchdog_on_the_rccl_branch_rehearsal(inject, stage, driver):
    """The N > 1 branch of bench.py with the LIBRARY'S OWN RCCL calls executing (DSEA_RCCL_LIB = the stand-in of
    tests/fake_rccl; two ranks sharing the GPU) under the watchdog of tools/bench_watchdog.py.  A hang injected INSIDE the
    stand-in -- in the point-to-point traffic of the second communicator, or in the all-reduce -- is what a dead-locked
    RCCL call would look like: no error, no return.  The supervisors notice the stall, kill both children and start fresh
    ones at the next stage; the line arrives from stage 2 (one communicator) resp. stage 3 (Python driver)."""
    if not os.path.exists(FAKE_RCCL):       # normally shipped in-tree by build(); else build it on the box
        subprocess.run(["make", "-C", os.path.dirname(FAKE_RCCL), "libfake_rccl.so"], capture_output=True, timeout=300)
    assert os.path.exists(FAKE_RCCL), "build() compiles tests/fake_rccl/libfake_rccl.so"
    env = {"DSEA_RCCL_LIB": FAKE_RCCL, "DSEA_BENCH_STALL_S": "8", "DSEA_BENCH_STARTUP_S": "300"}
    if inject:
        env["DSEA_BENCH_INJECT_HANG"] = inject
    d = _bench(["--gpus", "2", "--host-staged", "--steps", "2", "--warmup", "1", "--full"], env=env)
    cfg = d["config"]
    assert cfg["fallback_stage"] == stage, cfg["watchdog"]
    assert cfg["partitioned_driver"].startswith(driver), cfg["partitioned_driver"]
    assert abs(cfg["E0_per_site"] - cfg["E0_per_site_closed_form"]) < 1e-9
    wd = cfg["watchdog"]["stages"]
    assert [r["stage"] for r in wd] == list(range(1, stage + 1)) and wd[-1]["outcome"] == "completed"
    if inject:
        assert "no progress" in cfg["fallback_reason"] and "overlapped" not in cfg["slab_exchange"]
    else:
        assert cfg["fallback_reason"] is None and "overlapped" in cfg["slab_exchange"]
        assert isinstance(cfg["weak_scaling_point"], dict)
