"""world_size 2, 3, 4 and 8 over gloo on CPU: the row-partitioned operators BEHIND THE REFERENCE API
(setDominantSparseSymeig / DominantSparseSymeig.apply / autograd.grad, second order included) against the
reference-generated fixtures and the single-process CPU oracle.  2 ranks: pairwise slab exchange; 4, 8: transposed
all-to-all form; stencil: halo exchange on uneven slabs.  The slab-local numerics come from a torch-CPU test
double (tests/cpu_backend.py); on the GPU box the same driver runs on HipBackend (tests/test_gpu_partitioned.py)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle
from dominantsparseeigenad_amd.synthetic import normal_vector
from helpers import SeedDraws, signed_close, unit

L, K, G = 8, 120, 1.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _case_driver(rank, world, overlap=False, tau=None, replicate="auto"):
    """hand-written forward + backward of partitioned.PartitionedTFIM (no autograd)"""
    from cpu_backend import CpuBackend
    from dominantsparseeigenad_amd import engine
    from dominantsparseeigenad_amd.partitioned import PartitionedTFIM
    p = world.bit_length() - 1
    nloc = 1 << (L - p)
    off = rank * nloc
    g = torch.tensor([G], dtype=torch.float64)
    solver = PartitionedTFIM(L, g, "cpu", backend=CpuBackend(nloc), eps=1e-12)
    solver.overlap = overlap
    solver.op.replicate_cg = replicate
    if tau is not None:
        engine.SHADOW_TAU = tau
    q0 = torch.from_numpy(normal_vector(nloc, 5000, offset=off))
    x0 = torch.from_numpy(normal_vector(nloc, 5002, offset=off))
    t = torch.from_numpy(normal_vector(nloc, 5003, offset=off))
    E0, psi, grad = solver.forward_backward(K, q0, x0, t)
    return (E0.item(), psi.numpy().copy(), grad.item(), solver.last_cg_iters, solver.op.overlap_fallbacks)


def _case_g_rebind(rank, world):
    """op.g = new_tensor (the reference's ``model.g = ...`` pattern) must be SEEN by the slab operator: H with the new g"""
    from cpu_backend import CpuBackend
    from dominantsparseeigenad_amd.partitioned import PartitionedTFIMOperator
    p = world.bit_length() - 1
    nloc = 1 << (L - p)
    off = rank * nloc
    v = torch.from_numpy(normal_vector(nloc, 6000, offset=off))
    op = PartitionedTFIMOperator(L, torch.tensor([1.0], dtype=torch.float64), "cpu", backend=CpuBackend(nloc))
    y1 = op.H(v).clone()
    op.g = torch.tensor([1.7], dtype=torch.float64)
    y2 = op.H(v).clone()
    fresh = PartitionedTFIMOperator(L, torch.tensor([1.7], dtype=torch.float64), "cpu", backend=CpuBackend(nloc))
    y3 = fresh.H(v).clone()
    return (bool(torch.equal(y2, y3)), float((y1 - y2).abs().max()))


def _case_partial_on_python_driver(rank, world):
    """the partial re-orthogonalisation option needs the library driver: the Python step driver says so on every rank (same
    condition everywhere, no collective has been issued yet) instead of silently re-orthogonalising on every step"""
    from cpu_backend import CpuBackend
    from dominantsparseeigenad_amd import engine
    from dominantsparseeigenad_amd.partitioned import PartitionedTFIM
    p = world.bit_length() - 1
    nloc = 1 << (L - p)
    off = rank * nloc
    solver = PartitionedTFIM(L, torch.tensor([G], dtype=torch.float64), "cpu", backend=CpuBackend(nloc), eps=1e-12)
    q0 = torch.from_numpy(normal_vector(nloc, 5000, offset=off))
    x0 = torch.from_numpy(normal_vector(nloc, 5002, offset=off))
    t = torch.from_numpy(normal_vector(nloc, 5003, offset=off))
    engine.PARTIAL_REORTH = 0.0
    try:
        solver.forward_backward(20, q0, x0, t)
        raised = False
    except NotImplementedError as exc:
        raised = "library driver" in str(exc)
    finally:
        engine.PARTIAL_REORTH = None
    E0, _, _ = solver.forward_backward(20, q0, x0, t)          # ... and the operator is usable afterwards
    return (raised, bool(torch.isfinite(E0)))


def _case_api_tfim(rank, world, tag):
    """E0, dE0, d2E0, loss gradient, chi_F through the reference API on a row-partitioned operator"""
    from cpu_backend import CpuBackend
    from helpers import PatchRandn
    import dominantsparseeigenad_amd.symeig as symeig
    from dominantsparseeigenad_amd.partitioned import PartitionedTFIMOperator
    gd = np.load(os.path.join(GOLDEN, "tfim_" + tag + ".npz"))
    Lg, k, g0 = int(gd["L"]), int(gd["k"]), float(gd["g"])
    p = world.bit_length() - 1
    nloc = 1 << (Lg - p)
    off = rank * nloc
    g = torch.tensor([g0], dtype=torch.float64, requires_grad=True)
    op = PartitionedTFIMOperator(Lg, g, "cpu", backend=CpuBackend(nloc))
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_gadjoint)
    f = symeig.DominantSparseSymeig.apply
    tvec = op.slab(unit(1 << Lg, int(gd["seed_t"])))
    out = {}
    with PatchRandn(int(gd["seed_draw_E"]), offset=off) as draws:
        E0, psi = f(g, k, op.dim, "cpu")
        (dE0,) = torch.autograd.grad(E0, g, create_graph=True)
        (d2E0,) = torch.autograd.grad(dE0, g)
        out["ndraw_E"] = draws.count
    out.update(E0=E0.item(), psi=psi.detach().numpy().copy(), dE0=dE0.item(), d2E0=d2E0.item())
    sgn_probe = op.dot(psi.detach(), op.slab(torch.from_numpy(gd["psi"]))).item()
    sgn = 1.0 if sgn_probe > 0 else -1.0
    with PatchRandn(int(gd["seed_draw_E"]), offset=off):
        E0, psi = f(g, k, op.dim, "cpu")
        loss = E0 + op.dot(psi, tvec) * sgn
        (gl,) = torch.autograd.grad(loss, g)
    out.update(loss=loss.item(), dloss=gl.item())
    with PatchRandn(int(gd["seed_draw_E"]), offset=off):
        E0, psi = f(g, k, op.dim, "cpu")
        logF = torch.log(op.dot(psi.detach(), psi))
        (dlogF,) = torch.autograd.grad(logF, g, create_graph=True)
        (d2logF,) = torch.autograd.grad(dlogF, g)
    out["chiF"] = -d2logF.item()
    return out


def _case_api_stencil(rank, world):
    """1-D Schroedinger problem (schrodinger1D.py:64-73 semantics) on uneven slabs with halo exchange"""
    from cpu_backend import CpuBackend
    from helpers import PatchRandn
    import dominantsparseeigenad_amd.symeig as symeig
    from dominantsparseeigenad_amd.partitioned import PartitionedStencil3Operator, stencil_partition
    gd = np.load(os.path.join(GOLDEN, "schrodinger.npz"))
    N, k, h = int(gd["N"]), int(gd["k"]), float(gd["h"])
    rows, off = stencil_partition(N, world, rank)
    xmesh = torch.from_numpy(np.linspace(-1.0, 1.0, num=N, endpoint=False))
    potential = (0.5 * xmesh ** 2)[off:off + rows].clone().requires_grad_(True)
    op = PartitionedStencil3Operator(N, h, potential, "cpu", backend=CpuBackend(rows))
    target = torch.from_numpy(gd["target"])[off:off + rows]
    symeig.setDominantSparseSymeig(op.Hsparse, op.Hadjoint_to_padjoint)
    with PatchRandn(int(gd["seed_draw"]), offset=off):
        E, psi = symeig.DominantSparseSymeig.apply(potential, k, N, "cpu")
        loss = 1.0 - op.dot(psi.abs(), target)
        (gp,) = torch.autograd.grad(loss, potential)
    return dict(E=E.item(), psi=psi.detach().numpy().copy(), loss=loss.item(), grad=gp.numpy().copy(), off=off)


def _csr_case_matrix(kind):
    """the two patterns of the row-partitioned explicit-matrix tests: a banded SPD matrix (halo exchange) and a symmetric
    matrix with far couplings (all-gather fallback); n is not a multiple of 3 or 4 (padded last slab)"""
    import scipy.sparse as sp
    from helpers import banded_spd
    n = 601
    M = banded_spd(n, 7, 31)
    if kind == "scattered":
        rng = np.random.RandomState(32)
        extra = sp.random(n, n, density=0.004, random_state=rng, format="csr") * 0.05
        M = (M + extra + extra.T).tocsr()
        M.sort_indices()
    return M


def _case_api_csr(rank, world, kind):
    """E0, psi and d(E0 + psi.t)/d vals (this rank's non-zeros) through the reference API on PartitionedCSROperator"""
    from cpu_backend import CpuBackend
    from helpers import PatchRandn
    import dominantsparseeigenad_amd.symeig as symeig
    import dominantsparseeigenad_amd.CG as CG
    from dominantsparseeigenad_amd.partitioned import PartitionedCSROperator, csr_partition
    CG.EPS_DEFAULT = 1e-12
    M = _csr_case_matrix(kind)
    n, k = M.shape[0], 150
    nloc, off, real = csr_partition(n, world, rank)
    sub = M[off:off + real]
    vals = torch.from_numpy(sub.data.copy()).requires_grad_(True)
    op = PartitionedCSROperator(torch.from_numpy(sub.indptr.astype("int64")), torch.from_numpy(sub.indices.astype("int64")),
                                vals, n, "cpu", backend=CpuBackend(nloc))
    t_full = torch.zeros(nloc * world, dtype=torch.float64)
    t_full[:n] = unit(n, 8100)
    t = op.slab(t_full)
    symeig.setDominantSparseSymeig(op, op.Aadjoint_to_valsadjoint_symmetric)
    with PatchRandn(8200, offset=off):
        E0, psi = symeig.DominantSparseSymeig.apply(vals, k, op.dim, "cpu")
        loss = E0 + op.dot(psi, t)
        (gv,) = torch.autograd.grad(loss, vals)
    x = op.slab(torch.cat([torch.from_numpy(normal_vector(n, 8300)), torch.zeros(nloc * world - n, dtype=torch.float64)]))
    y = op.H(x.clone())
    return dict(mode=op.mode, hb=op.hb, E=E0.item(), psi=psi.detach().numpy()[:real].copy(), pad=float(psi.detach()[real:].abs().sum()),
                grad=gv.numpy().copy(), y=y.numpy()[:real].copy(), loss=loss.item())


def _worker(rank, world, port, case, args, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        ret[rank] = globals()[case](rank, world, *args)   # results by value, not shm
    finally:
        dist.destroy_process_group()


def _run(world, case, *args):
    from helpers import spawn_collect
    ret = spawn_collect(_worker, (world, _free_port(), case, args), world, port_index=1)
    assert len(ret) == world
    return [ret[r] for r in range(world)]


@pytest.mark.parametrize("world,overlap,tau", [(2, False, None), (4, False, None), (8, False, None),
                                               (2, True, None), (4, True, None), (4, True, 0.0),
                                               (8, True, None), (8, True, 0.0)])
def test_partitioned_matches_single_process_oracle(world, overlap, tau):
    """overlap: the slab exchange of the un-corrected r is started before the dots pass (pairwise form at 2 ranks,
    transposed form from 4) and its premise max|c_j| <= tau ||r|| is checked every step; tau = 0 makes every step
    fail the premise, i.e. exercises the redo-with-the-corrected-r branch."""
    n = 1 << L
    model = oracle.TFIMTables(L)
    model.g = torch.tensor([G], dtype=torch.float64, requires_grad=True)
    # the oracle consumes draws in the order q0, (unused), x0 -> seeds 5000, 5001, 5002
    f = oracle.make_sparse_dominant_symeig(model.H, model.adjoint_hook, draw=SeedDraws(5000), eps=1e-12).apply
    t = torch.from_numpy(normal_vector(n, 5003))
    E_o, psi_o = f(model.g, K, n)
    (g_o,) = torch.autograd.grad(E_o + psi_o.matmul(t), model.g)

    ret = _run(world, "_case_driver", overlap, tau)
    if overlap:
        # n = 256, k = 120: close to the end the Krylov space of the start vector is nearly exhausted and a few steps
        # fail the premise on their own (they take the redo branch, which is what the check is for)
        # (tau = 0: every step whose coefficients are not EXACTLY zero -- all of them but at most one or two)
        assert (K - 3 <= ret[0][4] <= K - 1) if tau == 0.0 else (ret[0][4] < 10), ret[0][4]
    psi = torch.cat([torch.from_numpy(ret[r][1]) for r in range(world)])
    sgn = 1.0 if float(psi @ psi_o.detach()) > 0 else -1.0
    for r in range(world):
        assert ret[r][0] == ret[0][0] and ret[r][2] == ret[0][2]      # replicated scalars are bit-identical
        assert ret[r][3] == ret[0][3]                                    # same CG branch everywhere
    assert abs(ret[0][0] - E_o.item()) < 1e-12 * abs(E_o.item())
    assert float((psi * sgn - psi_o.detach()).abs().max()) < 1e-10
    # the loss used psi with this run's sign; compare with the oracle's gradient for the same sign
    if sgn < 0:
        (g_o,) = torch.autograd.grad(E_o - psi_o.matmul(t), model.g)
    assert abs(ret[0][2] - g_o.item()) < 1e-9 * abs(g_o.item()), (ret[0][2], g_o.item())


@pytest.mark.parametrize("world,tag", [(2, "L10_k300_g1.0"), (4, "L10_k300_g1.0"), (4, "L12_k200_g1.0")])
def test_reference_api_on_partitioned_tfim_matches_reference_fixtures(world, tag):
    """The REFERENCE'S OWN outputs (tests/golden/make_golden.py ran reference symeig.py / CG.py / E0.py:53-67 /
    chiF.py:40-53) reproduced with the vectors cut over ``world`` ranks: same call sequence, same number of RNG
    draws, first and second order."""
    gd = np.load(os.path.join(GOLDEN, "tfim_" + tag + ".npz"))
    ret = _run(world, "_case_api_tfim", tag)
    for r in range(1, world):          # replicated scalars: bit-identical on all ranks
        for key in ("E0", "dE0", "d2E0", "loss", "dloss", "chiF"):
            assert ret[r][key] == ret[0][key], (key, ret[r][key], ret[0][key])
    o = ret[0]
    assert o["ndraw_E"] == int(gd["ndraw_E"])
    psi = np.concatenate([ret[r]["psi"] for r in range(world)])
    assert abs(o["E0"] - float(gd["E0"])) < 1e-10 * abs(float(gd["E0"]))
    assert signed_close(psi, gd["psi"], 1e-10)[0]
    assert abs(o["dE0"] - float(gd["dE0"][0])) < 2e-8 * abs(float(gd["dE0"][0]))     # CG eps = 1e-7 (CG.py:25)
    assert abs(o["d2E0"] - float(gd["d2E0"][0])) < 1e-6 * abs(float(gd["d2E0"][0]))
    assert abs(o["loss"] - float(gd["loss"])) < 1e-10
    assert abs(o["dloss"] - float(gd["dloss"][0])) < 2e-8 * abs(float(gd["dloss"][0]))
    assert abs(o["chiF"] - float(gd["chiF"][0])) < 1e-7 * abs(float(gd["chiF"][0]))


@pytest.mark.parametrize("world", [2, 3])
def test_reference_api_on_partitioned_stencil_matches_reference_fixture(world):
    gd = np.load(os.path.join(GOLDEN, "schrodinger.npz"))
    ret = _run(world, "_case_api_stencil")
    psi = np.concatenate([ret[r]["psi"] for r in range(world)])
    grad = np.concatenate([ret[r]["grad"] for r in range(world)])
    assert abs(ret[0]["E"] - float(gd["E"])) < 1e-10 * abs(float(gd["E"]))
    assert signed_close(psi, gd["psi"], 1e-9)[0]
    assert abs(ret[0]["loss"] - float(gd["loss"])) < 1e-9
    assert np.max(np.abs(grad - gd["grad"])) < 1e-5 * np.max(np.abs(gd["grad"]))   # CG hits the n-iteration cap


@pytest.mark.parametrize("world,kind", [(2, "banded"), (3, "banded"), (4, "banded"), (2, "scattered"), (3, "scattered"),
                                        (4, "scattered")])
def test_reference_api_on_partitioned_csr_matches_dense_eigh(world, kind):
    """row-partitioned explicit matrix (SURVEY 8e "CSR-banded: halo", all-gather fallback otherwise): mat-vec equal to
    scipy's, E0 / psi / d(E0 + psi.t)/d vals (tied-pair adjoint) at 1e-10 against first-order perturbation theory on
    the dense eigh factors; the padding of the last slab stays zero"""
    from helpers import eigh_reference
    M = _csr_case_matrix(kind)
    n = M.shape[0]
    ret = _run(world, "_case_api_csr", kind)
    # (two ranks: the one neighbour IS everybody else, a wide halo; from three on the far couplings need the all-gather)
    assert all(r["mode"] == ("halo" if kind == "banded" or world == 2 else "gather") for r in ret), [r["mode"] for r in ret]
    if kind == "banded":
        assert all(1 <= r["hb"] <= 7 and r["hb"] == ret[0]["hb"] for r in ret)
    y = np.concatenate([r["y"] for r in ret])
    x = normal_vector(n, 8300)
    assert np.max(np.abs(y - M @ x)) < 1e-13 * np.max(np.abs(M @ x))
    psi = torch.from_numpy(np.concatenate([r["psi"] for r in ret]))
    assert all(r["pad"] == 0.0 for r in ret)
    grad = torch.from_numpy(np.concatenate([r["grad"] for r in ret]))
    t = unit(n, 8100)
    E_ref, psi_ref, g_ref = eigh_reference(torch.from_numpy(M.indptr.astype("int64")), torch.from_numpy(M.indices.astype("int64")),
                                           torch.from_numpy(M.data.copy()), n, t, 1.0, 1.0, psi_like=psi, autograd=False)
    for r in ret:
        assert r["E"] == ret[0]["E"] and r["loss"] == ret[0]["loss"]          # replicated scalars: bit-identical
    assert abs(ret[0]["E"] - E_ref.item()) < 1e-12 * abs(E_ref.item())
    assert float((psi - psi_ref).abs().max()) < 1e-9
    err = float((grad - g_ref).abs().max()) / float(g_ref.abs().max())
    assert err < 1e-10, err


@pytest.mark.parametrize("world,launcher,explicit", [(2, "self", True), (4, "torchrun", False), (8, "self", False)])
def test_bench_multi_rank_control_flow_dry_run(world, launcher, explicit):
    """bench.py's multi-rank path end to end on CPU processes (``--dry-run-cpu``: gloo + the torch test double of the
    slab kernels): self-launch of one worker per rank, or under the driver's own launcher line (python -m
    torch.distributed.run ... bench.py --gpus N --steps K --warmup W); row-partitioned operator behind the reference
    API, collective decision on the exchange form, overlapped-exchange self-check, max-over-ranks timing, ONE JSON line
    from rank 0 as the last line of stdout.  Without --L / --k the DEFAULT SCHEDULE of N > 1 runs (toy sizes in a dry
    run): the strong point is timed (value / ms_per_step, scaling "strong"), the weak point is reported beside it, the
    one-GPU anchors and what proves the collectives spanned N ranks are in the line.  No measurement is taken from it."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    tail = [os.path.join(root, "bench.py"), "--gpus", str(world), "--steps", "2", "--warmup", "1", "--dry-run-cpu", "--full"]
    if explicit:
        tail += ["--L", "10", "--k", "60"]
    if launcher == "self":
        cmd = [sys.executable] + tail
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port())] + tail
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and out.stdout.strip().splitlines()[-1] == lines[0]       # one JSON line, and it is the last
    d = json.loads(lines[0])
    assert d["n_gpus"] == world and d["steps"] == 2 and d["warmup"] == 1 and d["metric"].startswith("DRY RUN")
    cfg = d["config"]
    assert ("transposed" if world >= 4 else "pairwise") in cfg["slab_exchange"] and "overlapped" in cfg["slab_exchange"]
    assert cfg["distributed_self_check"].startswith("overlapped exchange verified")
    assert abs(cfg["E0_per_site"] - cfg["E0_per_site_closed_form"]) < 1e-9
    assert "roofline" not in d and "cpu_baseline" not in d
    # what proves the collectives saw N ranks
    col = cfg["collectives"]
    assert col["world_size"] == world and col["backend"] == "gloo"
    assert sorted(r["rank"] for r in col["ranks"]) == list(range(world)) and len({r["pid"] for r in col["ranks"]}) == world
    # what bounds the line (tools/bench_multi.py): collectives on the run's own communicators, exposed exchange, SURVEY 8e's model
    sd = cfg["scaling_decomposition"]
    assert sd["allreduce_us"]["8_bytes"] > 0 and sd["allreduce_us"]["1600_bytes"] > 0
    assert sd["exchange"]["ms_per_matvec"] > 0 and sd["exchange"]["bytes_sent_per_gpu_per_matvec"] > 0
    assert sd["exposed_exchange_ms_per_lanczos_step"] >= 0 and sd["exposed_exchange_ms_per_cg_iteration"] >= 0
    assert sd["lanczos_forward_ms"]["without_exchange"] > 0 and sd["cg_ms_per_iteration"]["as_timed"] > 0
    assert "predicted_speedup" in sd["model"]["timed_point"] and "measured_speedup" in sd["model"]["timed_point"]
    assert cfg["fallback_stage"] == 1 and cfg["fallback_reason"] is None and cfg["watchdog"]["stages"][0]["outcome"] == "completed"
    if explicit:
        assert d["scaling"] == "weak" and "weak_scaling_point" not in cfg
    else:
        assert d["scaling"] == "strong" and "strong scaling" in cfg["workload"]
        wk = cfg["weak_scaling_point"]
        assert "weak scaling" in wk["workload"] and wk["ms_per_step"] > 0
        assert abs(wk["E0_per_site"] - wk["E0_per_site_closed_form"]) < 1e-9
        assert wk["distributed_self_check"].startswith("overlapped exchange verified")
        # the strong point beside itself with the all-fp64 correction pass and at the shadow-matched k; every speed-up
        # field names the arithmetic of BOTH sides and never divides a shadow-off anchor into a shadow-on run
        assert cfg["bf16_shadow_of_basis"] is True
        f64, mk = cfg["strong_point_fp64_basis"], cfg["strong_point_shadow_matched_k"]
        assert f64["bf16_shadow_of_basis"] is False and f64["ms_per_step"] > 0 and "strong scaling" in f64["workload"]
        assert mk["bf16_shadow_of_basis"] is True and mk["ms_per_step"] > 0 and "k=48" in mk["workload"]
        anchor = cfg["one_gpu_anchor"]
        assert "speedup_vs_one_gpu" not in anchor
        assert "speedup_vs_one_gpu_fp64_basis" in anchor and "fp64" in anchor["speedup_vs_one_gpu_fp64_basis_is"] \
            and "BOTH sides" in anchor["speedup_vs_one_gpu_fp64_basis_is"]
        assert "speedup_vs_one_gpu_k80_shadow" in anchor and "shadow" in anchor["speedup_vs_one_gpu_k80_shadow_is"] \
            and "BOTH sides" in anchor["speedup_vs_one_gpu_k80_shadow_is"]
        assert anchor["strong_k100_fp64_basis_ms"] == f64["ms_per_step"] and anchor["strong_k80_shadow_ms"] == mk["ms_per_step"]
        assert anchor["source"] and "NOT divided" in anchor["timed_point_note"]


def test_bench_anchor_resolution_and_like_by_like_speedups(tmp_path):
    """the one-GPU anchors of the N > 1 lines come from an N = 1 line's JSON (a path, a driver record wrapping the line
    under "parsed", the node cache), never from constants in the script; an anchor is only used for a speed-up when the
    arithmetic of its correction pass matches the multi-GPU side"""
    import importlib.util
    import json
    import types
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert not hasattr(bench, "STORED_ANCHORS")
    line = {"metric": "m", "config": {"commit": "abc1234", "one_gpu_anchors": {
        "strong_L28_k100": {"ms_per_step": 5000.0, "bf16_shadow_of_basis": False},
        "strong_L28_k80_shadow": {"ms_per_step": 3000.0, "bf16_shadow_of_basis": True},
        "weak_2p25_rows_k200": {"ms_per_step": 1250.0, "bf16_shadow_of_basis": True}}}}
    raw, wrapped = tmp_path / "line.json", tmp_path / "BENCH_r99.json"
    raw.write_text("some banner\n" + json.dumps(line) + "\n")
    wrapped.write_text(json.dumps({"rc": 0, "parsed": line}))
    for path in (raw, wrapped):
        anchors, src = bench.load_anchors(types.SimpleNamespace(anchors_json=str(path)))
        assert anchors["strong_L28_k100"]["ms_per_step"] == 5000.0 and "abc1234" in src
    assert bench.anchor_ms(anchors, "strong_L28_k100", False) == 5000.0
    assert bench.anchor_ms(anchors, "strong_L28_k100", True) is None          # never a shadow-off anchor for a shadow-on run
    assert bench.anchor_ms(anchors, "strong_L28_k80_shadow", True) == 3000.0
    pt = types.SimpleNamespace(explicit=False, toy=False, strong=True, k=100, nloc=1 << 25)
    rec = bench._speedups(pt, 700.0, True, {"ms_per_step": 1000.0, "bf16_shadow_of_basis": False},
                          {"ms_per_step": 600.0, "bf16_shadow_of_basis": True}, anchors, src)
    assert rec["speedup_vs_one_gpu_fp64_basis"] == 5.0 and rec["speedup_vs_one_gpu_k80_shadow"] == 5.0
    assert not any(key == "speedup_vs_one_gpu" for key in rec)
    # the one-GPU side of a pair missing -> the figure stays null instead of borrowing the other arithmetic
    del anchors["strong_L28_k80_shadow"]
    rec = bench._speedups(pt, 700.0, True, {"ms_per_step": 1000.0, "bf16_shadow_of_basis": False},
                          {"ms_per_step": 600.0, "bf16_shadow_of_basis": True}, anchors, src)
    assert rec["speedup_vs_one_gpu_k80_shadow"] is None and rec["speedup_vs_one_gpu_fp64_basis"] == 5.0


def test_rebinding_g_on_a_partitioned_operator_is_seen():
    ret = _run(2, "_case_g_rebind")
    assert all(same and moved > 1e-3 for same, moved in ret), ret


def test_partial_reorthogonalisation_needs_the_library_driver():
    ret = _run(2, "_case_partial_on_python_driver")
    assert all(r == (True, True) for r in ret), ret


@pytest.mark.parametrize("world", [2, 4])
def test_replicated_cg_equals_partitioned_cg(world):
    """PartitionedTFIMOperator.replicate_cg: the adjoint solve gathered and run on every rank in full (the default at
    two ranks, where a mat-vec would move a whole slab over one link) against the row-partitioned solve: same number
    of iterations, same eigenpair, gradient equal to the CG tolerance; replicated scalars bit-identical on all ranks."""
    part = _run(world, "_case_driver", False, None, False)
    repl = _run(world, "_case_driver", False, None, True)
    for r in range(world):
        assert repl[r][0] == repl[0][0] and repl[r][2] == repl[0][2] and repl[r][3] == repl[0][3]
        assert repl[r][0] == part[r][0] and torch.equal(torch.from_numpy(repl[r][1]), torch.from_numpy(part[r][1]))
    assert repl[0][3] == part[0][3]
    assert abs(repl[0][2] - part[0][2]) < 1e-10 * abs(part[0][2])


@pytest.mark.parametrize("inject,stage", [("exchange", 2), ("allreduce", 3), ("crash", 2), ("extras", 1)])
def test_bench_watchdog_walks_the_fallback_ladder(inject, stage):
    """tools/bench_watchdog.py: every launched rank supervises a child; a child that stops making progress (or dies) is
    killed on ALL ranks together and a fresh one started at the next stage -- library driver with the exchange on its
    own communicator -> one communicator, no overlap -> Python driver, pairwise.  The line still arrives, says which
    stage it came from and why.  A stall AFTER the timed point (in the extras beside it) keeps stage 1's number.
    Dry run: the faults are simulated in bench.py at the stages a real one of that kind would hit."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(DSEA_BENCH_INJECT_HANG=inject, DSEA_BENCH_STALL_S="6", DSEA_BENCH_STARTUP_S="120")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--dry-run-cpu",
           "--full"]
    if inject != "extras":
        cmd += ["--L", "10", "--k", "60"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
    lines = [ln for ln in out.stdout.strip().splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1 and out.stdout.strip().splitlines()[-1] == lines[0]
    d = json.loads(lines[0])
    cfg = d["config"]
    assert d["value"] > 0 and cfg["fallback_stage"] == stage, cfg["watchdog"]
    wd = cfg["watchdog"]["stages"]
    assert [r["stage"] for r in wd] == list(range(1, stage + 1))
    if inject == "extras":
        assert "extras_incomplete" in cfg and cfg["provisional"] is True and "no progress" in wd[0]["outcome"]
        assert cfg["fallback_reason"] is None
    else:
        assert wd[-1]["outcome"] == "completed" and all(r["outcome"] != "completed" for r in wd[:-1])
        assert ("exited with code" if inject == "crash" else "no progress") in cfg["fallback_reason"]
        assert cfg["ladder_stage_env"]["DSEA_BENCH_STAGE"] == str(stage)
    assert abs(cfg["E0_per_site"] - cfg["E0_per_site_closed_form"]) < 1e-9
