"""The block ladder kernels and ``thermal_dynamics`` on the GPU (docs/design/35-finite-temperature-dynamics.md):
k_sector_ladder_block and k_sector_ladder_block_dots on the geometries of tests/test_gpu_ladder.py that reach each path, bit for
bit against the single-vector kernel and within the bar of the numpy twin of tests/ladder_block_reference.py, the argument checks
of the C ABI with the outputs watched, then the assembled correlation function: the sampled route against the twin's estimator on
the same start vectors, the dense route against the full 2^L space, and the static sum rules that tie C(0) to
``thermal_correlations``.

"Bar" is max(1e-13, 10 x the twin's fp64 - longdouble deviation) x the natural scale of the quantity."""
import functools
import importlib.util
import math
import os
from ctypes import byref, c_int64, c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ladder_block_reference as twin  # noqa: E402
import lattice_reference  # noqa: E402
import sector_reference as ref  # noqa: E402
from dominantsparseeigenad_amd import _lib, engine, thermal  # noqa: E402
from dominantsparseeigenad_amd.operators import ring_bonds, ring_momentum_weights  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402
from test_gpu_ladder import GEOMETRY, WEIGHTS, dev, ladder, site_weights, to_dev  # noqa: E402

F64 = torch.float64
LD = np.longdouble
NAMES = ["L3-1-2", "L7-3-4", "L7-4-3", "L7-3-3", "L11-5-6", "L16-8-7", "L16-8-8", "L20-10-11-walk", "L40-2-1", "L40-2-2"]
WIDTHS = [1, 2, 4, 8]
STEP = {"zz": 0, "-": 1, "+": -1}


@functools.lru_cache(maxsize=None)
def blocks(name):
    """(X [n_src, 8], Lft [n_dst, 8]) on the host, computed once per geometry and never written to; column 5 of X is zero"""
    L, a, b, _ = GEOMETRY[name]
    X = np.stack([normal_vector(math.comb(L, a), 9300 + L + j) for j in range(8)], axis=1)
    X[:, 5] = 0.0
    Lft = np.stack([normal_vector(math.comb(L, b), 9320 + L + j) for j in range(8)], axis=1)
    for arr in (X, Lft):
        arr.setflags(write=False)
    return X, Lft


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """(S(c) X in longdouble, the column norms of fp64 twin - longdouble twin, the dots in longdouble, their deviation)"""
    L, a, b, _ = GEOMETRY[name]
    X, Lft = blocks(name)
    c = site_weights(L, kind)
    long = twin.apply_block(L, a, b - a, c, X, LD)
    own = np.linalg.norm((twin.apply_block(L, a, b - a, c, X) - long).astype(np.float64), axis=0)
    d_long = twin.dots(L, a, b - a, c, Lft, X, LD)
    d_own = np.abs((twin.dots(L, a, b - a, c, Lft, X) - d_long).astype(np.float64))
    return long.astype(np.float64), own, d_long.astype(np.float64), d_own


def entry_apply(lad, R, cd, Xd, Yd, grid):
    L, a = lad.L, int(lad.src.ndown)
    states, lo_rank, hi_base = lad._tables
    return _lib.load().dsea_sector_ladder_block_apply(L, a, lad.step, R, c_void_p(cd.data_ptr()), c_void_p(states.data_ptr()),
                                                      c_void_p(lo_rank.data_ptr()), c_void_p(hi_base.data_ptr()),
                                                      c_void_p(Xd.data_ptr()), c_void_p(Yd.data_ptr()), grid or 0, engine._stream(dev()))


def test_the_cases_reach_what_they_are_for():
    sizes = {name: (math.comb(GEOMETRY[name][0], GEOMETRY[name][1]), math.comb(GEOMETRY[name][0], GEOMETRY[name][2])) for name in NAMES}
    assert sizes["L3-1-2"] == (3, 3) and sizes["L11-5-6"][1] == 256 + 206 and sizes["L20-10-11-walk"][1] == 167960
    assert (167960 + 255) // 256 > 1 << GEOMETRY["L20-10-11-walk"][3]                 # blocks walk row ranges
    assert [GEOMETRY[n][2] - GEOMETRY[n][1] for n in NAMES] == [1, 1, -1, 0, 1, -1, 0, 1, -1, 0]
    # sites in flight per width are 8, 8, 4, 2: L = 16 (8 sites per group) runs 1, 1, 2, 4 chunks per group, L = 40 runs 3, 3, 5, 10
    assert (16 + 1) // 2 == 8 and (40 + 1) // 2 == 20


@pytest.mark.parametrize("R", WIDTHS)
@pytest.mark.parametrize("kind", WEIGHTS)
@pytest.mark.parametrize("name", NAMES)
def test_the_block_map_is_the_single_vector_map_column_by_column(name, kind, R):
    L, a, b, grid = GEOMETRY[name]
    lad = ladder(name)
    X, _ = blocks(name)
    first = 8 - R if R < 8 else 0                                   # (the narrower blocks end at column 7; R = 4, 8 hold the zero column)
    cd = to_dev(site_weights(L, kind))
    Xd = to_dev(np.ascontiguousarray(X[:, first:first + R]))
    keep = Xd.clone()
    Yd = torch.full((lad.n_dst * R + 67,), -7.0, dtype=F64, device=dev())
    assert entry_apply(lad, R, cd, Xd, Yd, grid) == 0
    Y = Yd[:lad.n_dst * R].reshape(lad.n_dst, R)
    assert bool((Yd[lad.n_dst * R:] == -7.0).all())                 # nothing is written past the last row
    assert torch.equal(Xd, keep)
    for j in range(R):
        assert torch.equal(Y[:, j], lad(cd, Xd[:, j].contiguous())), (name, kind, R, j)
    again = torch.empty((lad.n_dst, R), dtype=F64, device=dev())
    assert entry_apply(lad, R, cd, Xd, again, grid) == 0 and torch.equal(again, Y)
    if first <= 5:
        assert not bool(Y[:, 5 - first].any())                      # a zero column gives exactly zero
    if R == 8:                                                      # ... and against the twin
        want, own, _, _ = reference(name, kind)
        got = Y.cpu().numpy()
        for j in range(8):
            scale = np.linalg.norm(want[:, j])
            err = np.linalg.norm(got[:, j] - want[:, j])
            assert err <= max(1e-13, 10.0 * own[j] / scale if scale else 0.0) * scale, (name, kind, j, err, scale)


@pytest.mark.parametrize("R", [3, 13])
@pytest.mark.parametrize("name", ["L7-3-4", "L11-5-6", "L16-8-8", "L40-2-1"])
def test_apply_block_takes_any_width(name, R):
    L, a, b, _ = GEOMETRY[name]
    lad = ladder(name)
    cd = to_dev(site_weights(L, "random"))
    Xd = to_dev(np.stack([normal_vector(lad.n_src, 9340 + j) for j in range(R)], axis=1))
    Y = lad.apply_block(cd, Xd)
    assert Y.shape == (lad.n_dst, R) and Y.dtype == F64
    for j in range(R):
        assert torch.equal(Y[:, j], lad(cd, Xd[:, j].contiguous()))
    # the transposed ladder is the transpose: <Yl, S X> = <S^T Yl, X> column by column
    Yl = to_dev(np.stack([normal_vector(lad.n_dst, 9360 + j) for j in range(R)], axis=1))
    back = lad.T.apply_block(cd, Yl)
    assert back.shape == (lad.n_src, R)
    lhs, rhs = (Yl * Y).sum(0), (back * Xd).sum(0)
    scale = torch.linalg.vector_norm(Yl, dim=0) * torch.linalg.vector_norm(Y, dim=0) + \
        torch.linalg.vector_norm(back, dim=0) * torch.linalg.vector_norm(Xd, dim=0)
    assert bool(((lhs - rhs).abs() <= 1e-13 * scale).all())
    # ... and the dots of both against the column sums
    d, dT = lad.block_dots(cd, Yl, Xd), lad.T.block_dots(cd, Xd, Yl)
    assert d.shape == (R,) and bool(((d - lhs).abs() <= 1e-13 * scale).all()) and bool(((dT - rhs).abs() <= 1e-13 * scale).all())


@pytest.mark.parametrize("kind", WEIGHTS)
@pytest.mark.parametrize("name", NAMES)
def test_the_dots(name, kind):
    L, a, b, grid = GEOMETRY[name]
    lad = ladder(name)
    X, Lft = blocks(name)
    want, own, d_want, d_own = reference(name, kind)
    cd, Xd, Ld = to_dev(site_weights(L, kind)), to_dev(X), to_dev(Lft)
    got = lad.block_dots(cd, Ld, Xd)
    assert got.shape == (8,) and got.dtype == F64 and got.device.type == "cuda"
    scale = np.linalg.norm(Lft, axis=0) * np.linalg.norm(want, axis=0)
    bar = np.maximum(1e-13 * scale, 10.0 * d_own)
    err = np.abs(got.cpu().numpy() - d_want)
    print("%s %s: max |dots - longdouble twin| / scale = %.2e" % (name, kind, float((err / np.where(scale > 0, scale, 1.0)).max())))
    assert (err <= bar).all(), (err, bar)
    unfused = (Ld * lad.apply_block(cd, Xd)).sum(0)
    assert (np.abs((got - unfused).cpu().numpy()) <= bar).all()
    assert float(got[5]) == 0.0                                     # the zero column
    assert torch.equal(lad.block_dots(cd, Ld, Xd), got)             # fixed-order sums, no atomics
    for j in (0, 5, 7):                                             # column j of the R = 8 call is the R = 1 call on that column
        assert torch.equal(lad.block_dots(cd, Ld[:, j:j + 1], Xd[:, j:j + 1])[0], got[j])
    if grid is not None:                                            # a walked grid against the default one
        lad.set_grid_log2(0)
        try:
            flat = lad.block_dots(cd, Ld, Xd)
        finally:
            lad.set_grid_log2(grid)
        assert (np.abs((flat - got).cpu().numpy()) <= bar).all()


def test_c_abi_refusals_leave_the_outputs_alone():
    lib = _lib.load()
    name = "L7-3-4"
    L, a, b, _ = GEOMETRY[name]
    lad = ladder(name)
    states, lo_rank, hi_base = (c_void_p(t.data_ptr()) for t in lad._tables)
    X, Lft = blocks(name)
    cd, Xd, Ld = to_dev(site_weights(L, "random")), to_dev(X), to_dev(Lft)
    Yd = torch.full((lad.n_dst * 8 + 2,), -7.0, dtype=F64, device=dev())
    out = torch.full((8,), -7.0, dtype=F64, device=dev())
    need = c_int64()
    assert lib.dsea_sector_ladder_block_dots_scratch_doubles(L, a, b - a, 8, byref(need)) == 0 and need.value == 8
    scratch = torch.full((need.value,), -7.0, dtype=F64, device=dev())
    st = engine._stream(dev())
    P = lambda t, off=0: c_void_p(t.data_ptr() + off)  # noqa: E731
    assert Xd.data_ptr() % 16 == 0 and Yd.data_ptr() % 16 == 0 and Ld.data_ptr() % 16 == 0

    def apply(R=8, step=b - a, X=P(Xd), Y=P(Yd)):
        return lib.dsea_sector_ladder_block_apply(L, a, step, R, P(cd), states, lo_rank, hi_base, X, Y, 0, st)

    def dots(R=8, Lf=P(Ld), X=P(Xd), o=P(out), s=P(scratch)):
        return lib.dsea_sector_ladder_block_dots(L, a, b - a, R, P(cd), states, lo_rank, hi_base, Lf, X, o, s, 0, st)

    ERR_ALIGN = -2
    assert apply(X=P(Xd, 8)) == ERR_ALIGN and apply(Y=P(Yd, 8)) == ERR_ALIGN
    assert dots(X=P(Xd, 8)) == ERR_ALIGN and dots(Lf=P(Ld, 8)) == ERR_ALIGN
    assert apply(Y=P(Xd)) == _lib.ERR_ARG                           # X == Y at step != 0
    for R in (3, 0, 16):
        assert apply(R=R) == _lib.ERR_ARG and dots(R=R) == _lib.ERR_ARG
    assert apply(X=None) == _lib.ERR_ARG and apply(Y=None) == _lib.ERR_ARG
    assert dots(Lf=None) == _lib.ERR_ARG and dots(o=None) == _lib.ERR_ARG and dots(s=None) == _lib.ERR_ARG
    torch.cuda.synchronize()
    for t in (Yd, out, scratch):
        assert bool((t == -7.0).all())                              # nothing refused has run
    assert torch.equal(Xd, to_dev(X))
    # X == Y is allowed at step 0 (a diagonal map): in place
    same = ladder("L7-3-3")
    Xz = to_dev(blocks("L7-3-3")[0])
    want = same.apply_block(cd, Xz)
    assert entry_apply(same, 8, cd, Xz, Xz, None) == 0 and torch.equal(Xz, want)
    with pytest.raises(ValueError):
        lad.apply_block(cd, Xd.cpu())
    with pytest.raises(ValueError):
        lad.block_dots(cd, Ld[:, :4], Xd)                           # (the widths differ)
    with pytest.raises(ValueError):
        ladder("L11-5-6").block_dots(cd[:7], Ld, Xd)                # (blocks of another sector)


# ---- thermal_dynamics
BETAS = [0.0, 0.5, 2.0]


@functools.lru_cache(maxsize=None)
def ring_model(L):
    """a ring with random Jxy, Jz and fields hz, so that no two sectors share a spectrum"""
    bonds = tuple(ring_bonds(L))
    p = normal_vector(ref.nparam(L, bonds), 9380 + L).copy()
    p.setflags(write=False)
    return bonds, p


def weight_parts(L, kind):
    if kind == "real":
        return [normal_vector(L, 9390 + L)]
    re, im = ring_momentum_weights(L, 1)
    return [re.numpy(), im.numpy()]


@pytest.mark.parametrize("kind", ["real", "momentum"])
@pytest.mark.parametrize("channel", ["zz", "-", "+"])
@pytest.mark.parametrize("L", [6, 8])
def test_thermal_dynamics_sampled_against_the_twin(L, channel, kind):
    """dense_below = 0: every pair without an edge sector runs on the thermal pure quantum states, through the block ladder map, time_evolve
    and the fused dots, against the longdouble twin on the same start vectors"""
    bonds, p = ring_model(L)
    parts = weight_parts(L, kind)
    R, seed, dt, steps = 4, 11, 0.3, 8
    weights = torch.from_numpy(parts[0].copy()) if kind == "real" else tuple(torch.from_numpy(q.copy()) for q in parts)
    got = thermal.thermal_dynamics(L, bonds, to_dev(p), weights, channel, BETAS, dt, steps, R=R, seed=seed, dense_below=0)
    want = twin.thermal_dynamics(L, bonds, p, parts, STEP[channel], BETAS, dt, steps, R=R, seed=seed, dense_below=0, dtype=LD)
    assert got.correlation.shape == (3, steps + 1) and got.correlation.dtype == torch.complex128 and got.correlation.device.type == "cpu"
    assert torch.equal(got.times, dt * torch.arange(steps + 1, dtype=F64)) and torch.equal(got.betas, torch.tensor(BETAS, dtype=F64))
    C, ref_C = got.correlation.numpy(), want["C"].astype(np.complex128)
    static = ref_C[:, 0].real
    assert (static > 0).all() and want["orders"][:, 0].min() >= 0 and want["orders"][:, 1:].min() > 0
    bar = 1e-13 * np.maximum(want["orders"], 1.0) * static[:, None]
    err = np.abs(C - ref_C)
    print("L = %d %s %s: worst |C - twin| / (1e-13 orders C(0)) = %.3f (orders up to %d)"
          % (L, channel, kind, float((err / bar).max()), int(want["orders"].max())))
    assert (err <= bar).all()
    # ln Z: the log norms of the imaginary-time steps, the same form of bar on the orders of those steps alone
    assert (np.abs(got.logZ.numpy() - want["logZ"]) <= 1e-13 * np.maximum(want["orders"][:, 0], 10.0)).all()
    assert torch.equal(got.static(), got.correlation[:, 0].real)


@functools.lru_cache(maxsize=None)
def full_space(L):
    bonds, p = ring_model(L)
    theta, V = np.linalg.eigh(lattice_reference.dense(L, bonds, ref.full_parameter(L, bonds, p)))
    return theta, V


@pytest.mark.parametrize("kind", ["real", "momentum"])
@pytest.mark.parametrize("channel", ["zz", "-", "+"])
def test_thermal_dynamics_dense_against_the_full_space(channel, kind):
    """L = 8 at the default dense_below: every pair is dense; against tr[e^{-beta H} e^{iHt} A^+ e^{-iHt} A] / Z over all 2^L states"""
    L = 8
    bonds, p = ring_model(L)
    theta, V = full_space(L)
    parts = weight_parts(L, kind)
    dt, steps = 0.3, 8
    weights = torch.from_numpy(parts[0].copy()) if kind == "real" else torch.complex(*(torch.from_numpy(q.copy()) for q in parts))
    got = thermal.thermal_dynamics(L, bonds, to_dev(p), weights, channel, BETAS, dt, steps)
    lower = np.array([[0.0, 0.0], [1.0, 0.0]])                     # sets the bit: sigma^-
    site = {"zz": np.diag([1.0, -1.0]), "-": lower, "+": lower.T}[channel]
    W = sum((V.T @ sum(c[i] * lattice_reference._site_product(L, {i: site}) for i in range(L)) @ V) ** 2 for c in parts)
    gap = theta[:, None] - theta[None, :]
    for b, beta in enumerate(BETAS):
        w = np.exp(-beta * (theta - theta.min()))
        want = np.array([np.sum(w[None, :] * W * np.exp(-1j * k * dt * gap)) for k in range(steps + 1)]) / w.sum()
        err = np.abs(got.correlation[b].numpy() - want).max()
        print("%s %s beta = %g: |C - full space| / C(0) = %.2e" % (channel, kind, beta, err / want[0].real))
        assert err <= 1e-10 * want[0].real
        assert abs(float(got.logZ[b]) - (math.log(w.sum()) - beta * theta.min())) <= 1e-10


def test_the_static_sum_rules_against_thermal_correlations():
    """C(0) is an equal-time correlator that ``thermal_correlations`` has: with A = sum c_i Z_i, A^T A = sum_ij c_i c_j Z_i Z_j; with
    A = sigma^-(c) and sigma^+(c), A^T A adds up to sum_ij c_i c_j (sigma^+_i sigma^-_j + sigma^-_i sigma^+_j) =
    (1/2) sum_ij c_i c_j (X_i X_j + Y_i Y_j) / 2 off the diagonal and c_i^2 on it, that is c^T xy c / 2 with the diagonal 2 of ``xy``.
    Both are operator identities inside a source sector, so they hold column by column of the SAME thermal pure quantum states:
    same seed, R, betas and dense_below = 0.  zz: all sectors (its only edge pairs are the one-state sectors, exact in both).  The
    ladder channels: the sources 2 .. L - 2, because a pair with an edge sector is exact in ``thermal_dynamics`` while
    ``thermal_correlations`` samples the sectors ndown = 1 and L - 1 at dense_below = 0; with every sector exact (the default
    dense_below) all sources are compared."""
    L, R, seed = 8, 4, 21
    bonds, p = ring_model(L)
    c = torch.from_numpy(normal_vector(L, 9395))
    pd = to_dev(p)
    bar = 1e-12 * L

    def rules(sectors_zz, sectors_pm, dense_below):
        corr = thermal.thermal_correlations(L, bonds, pd, BETAS, R=R, seed=seed, dense_below=dense_below, sectors=sectors_zz)
        zz = thermal.thermal_dynamics(L, bonds, pd, c, "zz", BETAS, 0.3, 0, R=R, seed=seed, dense_below=dense_below, sectors=sectors_zz)
        err = (zz.static() - torch.einsum("i,bij,j->b", c, corr.zz, c)).abs().max()
        assert float((zz.logZ - corr.logZ).abs().max()) <= 1e-12
        corr = thermal.thermal_correlations(L, bonds, pd, BETAS, R=R, seed=seed, dense_below=dense_below, sectors=sectors_pm)
        lo, up = (thermal.thermal_dynamics(L, bonds, pd, c, ch, BETAS, 0.3, 0, R=R, seed=seed, dense_below=dense_below,
                                           sectors=sectors_pm) for ch in ("-", "+"))
        err_pm = (lo.static() + up.static() - 0.5 * torch.einsum("i,bij,j->b", c, corr.xy, c)).abs().max()
        return float(err), float(err_pm)

    sampled = rules(None, list(range(2, L - 1)), 0)
    exact = rules(None, None, 256)
    print("sampled: zz %.2e, -+ %.2e; exact: zz %.2e, -+ %.2e (bar %.2e)" % (sampled + exact + (bar,)))
    assert max(sampled + exact) <= bar


def test_example_thermal_dynamics():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "spin_lattice", "thermal_dynamics.py")
    spec = importlib.util.spec_from_file_location("spin_lattice_thermal_dynamics", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = ex.main(L=8)
    assert out["L"] == 8 and len(out["T"]) == len(out["static"]) == len(out["static_correlations"])
    for a, b in zip(out["static"], out["static_correlations"]):
        assert abs(a - b) <= 1e-10 * abs(b)
    S = np.asarray(out["S"])
    assert S.shape == (len(out["T"]), len(out["omega"])) and np.isfinite(S).all()
    # the integral of S over omega is C(0) (the window is 1 at t = 0), and the broadened spectrum of a positive measure is positive
    d_omega = out["omega"][1] - out["omega"][0]
    assert np.abs(S.sum(axis=1) * d_omega - np.asarray(out["static"])).max() <= 1e-6 * max(out["static"])
    assert S.min() >= -1e-8 * S.max()
