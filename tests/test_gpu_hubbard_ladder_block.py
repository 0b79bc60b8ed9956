"""The block Hubbard ladder kernels and ``hubbard_thermal_dynamics`` on the GPU
(docs/design/37-hubbard-finite-temperature-dynamics.md): k_hubbard_ladder_block and k_hubbard_ladder_block_dots on the 22
geometries of tests/test_gpu_hubbard_ladder.py, bit for bit against the single-vector kernel and within the bar of the numpy
twin of tests/hubbard_ladder_block_reference.py, the argument checks of the C ABI with the outputs watched, then the assembled
correlation function: the sampled route against the twin's estimator on the same start vectors, the dense route against the full
4^L Fock space, and the exact identities (the anticommutator sum rule, <N^2>, constant records of conserved operators).

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

import hubbard_ladder_block_reference as twin  # noqa: E402
import hubbard_reference as hub  # noqa: E402
from dominantsparseeigenad_amd import _lib, engine, thermal  # noqa: E402
from dominantsparseeigenad_amd.operators import ring_bonds, ring_momentum_weights  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402
from test_gpu_hubbard_ladder import GEOMETRY, WEIGHTS, dev, ladder, ref_args, site_weights, step_of, to_dev  # noqa: E402

F64 = torch.float64
LD = np.longdouble
TOL = 1e-10
NAMES = list(GEOMETRY)
WIDTHS = [1, 2, 4, 8]
CHANNELS = ["c_up", "c_dn", "cdag_up", "cdag_dn", "n", "sz"]


def sizes(name):
    L, src, dst, _, _ = GEOMETRY[name]
    return math.comb(L, src[0]) * math.comb(L, src[1]), math.comb(L, dst[0]) * math.comb(L, dst[1])


@functools.lru_cache(maxsize=None)
def blocks(name):
    """(X [n_src, 8], Lft [n_dst, 8]) on the host, computed once per geometry and never written to; column 5 of X is zero"""
    L = GEOMETRY[name][0]
    n_src, n_dst = sizes(name)
    X = np.stack([normal_vector(n_src, 9800 + L + j) for j in range(8)], axis=1)
    X[:, 5] = 0.0
    Lft = np.stack([normal_vector(n_dst, 9820 + L + j) for j in range(8)], axis=1)
    for arr in (X, Lft):
        arr.setflags(write=False)
    return X, Lft


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """(S(w) X in longdouble, the column norms of fp64 twin - longdouble twin, the dots in longdouble, their deviation)"""
    args = ref_args(name)
    X, Lft = blocks(name)
    w = site_weights(args[0], kind)
    long, plain = twin.apply_block(*args, w, X, LD), twin.apply_block(*args, w, X)           # (each once: the dots are their column sums)
    own = np.linalg.norm((plain - long).astype(np.float64), axis=0)
    d_long = np.einsum("rj,rj->j", Lft.astype(LD), long)
    d_own = np.abs((np.einsum("rj,rj->j", Lft, plain) - d_long).astype(np.float64))
    return long.astype(np.float64), own, d_long.astype(np.float64), d_own


def entry_apply(lad, R, wd, Xd, Yd, grid):
    states, lo_rank, hi_base = lad._tables
    return _lib.load().dsea_hubbard_ladder_block_apply(*lad._sector_args(), R, c_void_p(wd.data_ptr()), c_void_p(states.data_ptr()),
                                                       c_void_p(lo_rank.data_ptr()), c_void_p(hi_base.data_ptr()),
                                                       c_void_p(Xd.data_ptr()), c_void_p(Yd.data_ptr()), grid or 0, engine._stream(dev()))


def test_the_cases_reach_what_they_are_for():
    assert len(NAMES) == 22
    assert sizes("L2-11-up0") == (4, 4) and sizes("L7-34-44")[1] == 1225 == 4 * 256 + 201
    assert sizes("L12-55-65-walk")[1] == 731808 and (731808 + 255) // 256 > 1 << GEOMETRY["L12-55-65-walk"][4]      # blocks walk ranges
    need = c_int64()                                                # ... and the scratch of the dots holds every range's partial
    assert _lib.load().dsea_hubbard_ladder_block_dots_scratch_doubles(*ref_args("L12-55-65-walk"), 8, byref(need)) == 0
    assert need.value == 8 * 2859
    assert {(GEOMETRY[n][3], step_of(n)) for n in NAMES} == {(s, k) for s in ("up", "dn") for k in (-1, 0, 1)}
    assert {n for n in NAMES if GEOMETRY[n][3] == "dn" and step_of(n) and GEOMETRY[n][1][0] % 2} == {"L10-55-54", "L40-12-11"}   # g = -1
    # sites in flight per width are 8, 8, 4, 2: L = 16 (8 sites per group) runs 1, 1, 2, 4 chunks per group, L = 40 runs 3, 3, 5, 10;
    # L = 34 and L = 40 have words wider than 32 bits with sites in the high group
    assert (16 + 1) // 2 == 8 and (40 + 1) // 2 == 20 and (34 + 1) // 2 == 17


@pytest.mark.parametrize("R", WIDTHS)
@pytest.mark.parametrize("kind", WEIGHTS)
@pytest.mark.parametrize("name", NAMES)
def test_the_block_map_is_the_single_vector_map_column_by_column(name, kind, R):
    L, grid = GEOMETRY[name][0], GEOMETRY[name][4]
    lad = ladder(name)
    X, _ = blocks(name)
    first = 8 - R if R < 8 else 0                                   # (the narrower blocks end at column 7; R = 4, 8 hold the zero column)
    wd = to_dev(site_weights(L, kind))
    Xd = to_dev(np.ascontiguousarray(X[:, first:first + R]))
    keep = Xd.clone()
    Yd = torch.full((lad.n_dst * R + 67,), -7.0, dtype=F64, device=dev())
    assert entry_apply(lad, R, wd, Xd, Yd, grid) == 0
    Y = Yd[:lad.n_dst * R].reshape(lad.n_dst, R)
    assert bool((Yd[lad.n_dst * R:] == -7.0).all())                 # nothing is written past the last row
    assert torch.equal(Xd, keep)
    for j in range(R):
        assert torch.equal(Y[:, j], lad(wd, Xd[:, j].contiguous())), (name, kind, R, j)
    again = torch.empty((lad.n_dst, R), dtype=F64, device=dev())
    assert entry_apply(lad, R, wd, Xd, again, grid) == 0 and torch.equal(again, Y)
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
@pytest.mark.parametrize("name", ["L3-11-21", "L5-23-22", "L7-34-44", "L10-55-54", "L16-21-31", "L40-12-11", "L7-34-dn0"])
def test_apply_block_takes_any_width(name, R):
    L = GEOMETRY[name][0]
    lad = ladder(name)
    wd = to_dev(site_weights(L, "random"))
    Xd = to_dev(np.stack([normal_vector(lad.n_src, 9840 + j) for j in range(R)], axis=1))
    Y = lad.apply_block(wd, Xd)
    assert Y.shape == (lad.n_dst, R) and Y.dtype == F64
    for j in range(R):
        assert torch.equal(Y[:, j], lad(wd, Xd[:, j].contiguous()))
    # the transposed ladder is the transpose: <Yl, S X> = <S^T Yl, X> column by column
    Yl = to_dev(np.stack([normal_vector(lad.n_dst, 9860 + j) for j in range(R)], axis=1))
    back = lad.T.apply_block(wd, Yl)
    assert back.shape == (lad.n_src, R)
    lhs, rhs = (Yl * Y).sum(0), (back * Xd).sum(0)
    scale = torch.linalg.vector_norm(Yl, dim=0) * torch.linalg.vector_norm(Y, dim=0) + \
        torch.linalg.vector_norm(back, dim=0) * torch.linalg.vector_norm(Xd, dim=0)
    assert bool(((lhs - rhs).abs() <= 1e-13 * scale).all())
    # ... and the dots of both against the column sums
    d, dT = lad.block_dots(wd, Yl, Xd), lad.T.block_dots(wd, Xd, Yl)
    assert d.shape == (R,) and bool(((d - lhs).abs() <= 1e-13 * scale).all()) and bool(((dT - rhs).abs() <= 1e-13 * scale).all())


@pytest.mark.parametrize("kind", WEIGHTS)
@pytest.mark.parametrize("name", NAMES)
def test_the_dots(name, kind):
    L, grid = GEOMETRY[name][0], GEOMETRY[name][4]
    lad = ladder(name)
    X, Lft = blocks(name)
    want, own, d_want, d_own = reference(name, kind)
    wd, Xd, Ld = to_dev(site_weights(L, kind)), to_dev(X), to_dev(Lft)
    got = lad.block_dots(wd, Ld, Xd)
    assert got.shape == (8,) and got.dtype == F64 and got.device.type == "cuda"
    scale = np.linalg.norm(Lft, axis=0) * np.linalg.norm(want, axis=0)
    bar = np.maximum(1e-13 * scale, 10.0 * d_own)
    err = np.abs(got.cpu().numpy() - d_want)
    print("%s %s: max |dots - longdouble twin| / scale = %.2e" % (name, kind, float((err / np.where(scale > 0, scale, 1.0)).max())))
    assert (err <= bar).all(), (err, bar)
    unfused = (Ld * lad.apply_block(wd, Xd)).sum(0)
    assert (np.abs((got - unfused).cpu().numpy()) <= bar).all()
    assert float(got[5]) == 0.0                                     # the zero column
    assert torch.equal(lad.block_dots(wd, Ld, Xd), got)             # fixed-order sums, no atomics
    for j in (0, 5, 7):                                             # column j of the R = 8 call is the R = 1 call on that column
        assert torch.equal(lad.block_dots(wd, Ld[:, j:j + 1], Xd[:, j:j + 1])[0], got[j])
    if grid is not None:                                            # a walked grid against the default one
        lad.set_grid_log2(0)
        try:
            flat = lad.block_dots(wd, Ld, Xd)
        finally:
            lad.set_grid_log2(grid)
        assert (np.abs((flat - got).cpu().numpy()) <= bar).all()


def test_c_abi_refusals_leave_the_outputs_alone():
    lib = _lib.load()
    name = "L7-34-44"
    L = GEOMETRY[name][0]
    lad = ladder(name)
    args = lad._sector_args()
    states, lo_rank, hi_base = (c_void_p(t.data_ptr()) for t in lad._tables)
    X, Lft = blocks(name)
    wd, Xd, Ld = to_dev(site_weights(L, "random")), to_dev(X), to_dev(Lft)
    Yd = torch.full((lad.n_dst * 8 + 2,), -7.0, dtype=F64, device=dev())
    out = torch.full((8,), -7.0, dtype=F64, device=dev())
    need = c_int64()
    assert lib.dsea_hubbard_ladder_block_dots_scratch_doubles(*args, 8, byref(need)) == 0 and need.value == 8 * 5
    scratch = torch.full((need.value,), -7.0, dtype=F64, device=dev())
    st = engine._stream(dev())
    P = lambda t, off=0: c_void_p(t.data_ptr() + off)  # noqa: E731
    assert Xd.data_ptr() % 16 == 0 and Yd.data_ptr() % 16 == 0 and Ld.data_ptr() % 16 == 0

    def apply(R=8, step=args[4], X=P(Xd), Y=P(Yd)):
        return lib.dsea_hubbard_ladder_block_apply(args[0], args[1], args[2], args[3], step, R, P(wd), states, lo_rank, hi_base, X, Y,
                                                   0, st)

    def dots(R=8, Lf=P(Ld), X=P(Xd), o=P(out), s=P(scratch)):
        return lib.dsea_hubbard_ladder_block_dots(*args, R, P(wd), states, lo_rank, hi_base, Lf, X, o, s, 0, st)

    ERR_ALIGN = -2
    assert apply(X=P(Xd, 8)) == ERR_ALIGN and apply(Y=P(Yd, 8)) == ERR_ALIGN
    assert dots(X=P(Xd, 8)) == ERR_ALIGN and dots(Lf=P(Ld, 8)) == ERR_ALIGN
    assert args[4] == 1 and apply(Y=P(Xd)) == _lib.ERR_ARG          # X == Y at step +1 ...
    back = ladder("L3-21-11")                                       # ... and at step -1
    assert back.step == -1
    Xb = to_dev(blocks("L3-21-11")[0])
    keep = Xb.clone()
    assert entry_apply(back, 8, to_dev(site_weights(3, "random")), Xb, Xb, None) == _lib.ERR_ARG and torch.equal(Xb, keep)
    for R in (3, 0, 16):
        assert apply(R=R) == _lib.ERR_ARG and dots(R=R) == _lib.ERR_ARG
    assert apply(X=None) == _lib.ERR_ARG and apply(Y=None) == _lib.ERR_ARG
    assert dots(Lf=None) == _lib.ERR_ARG and dots(X=None) == _lib.ERR_ARG and dots(o=None) == _lib.ERR_ARG and dots(s=None) == _lib.ERR_ARG
    torch.cuda.synchronize()
    for t in (Yd, out, scratch):
        assert bool((t == -7.0).all())                              # nothing refused has run
    assert torch.equal(Xd, to_dev(X))
    # X == Y is allowed at step 0 (a diagonal map): in place, for both species
    for zero in ("L7-34-up0", "L7-34-dn0"):
        same = ladder(zero)
        Xz = to_dev(blocks(zero)[0])
        want = same.apply_block(wd, Xz)
        assert entry_apply(same, 8, wd, Xz, Xz, None) == 0 and torch.equal(Xz, want)
    with pytest.raises(ValueError):
        lad.apply_block(wd, Xd.cpu())
    with pytest.raises(ValueError):
        lad.block_dots(wd, Ld[:, :4], Xd)                           # (the widths differ)
    with pytest.raises(ValueError):
        ladder("L10-55-45").block_dots(wd, Ld, Xd)                  # (blocks and weights of another sector)


# ---- hubbard_thermal_dynamics
BETAS = [0.0, 0.5, 2.0]
MUS = [-0.4, 0.9]


@functools.lru_cache(maxsize=None)
def ring_model(L):
    """a ring with random t, V, U and eps, so that no two sectors share a spectrum"""
    bonds = tuple(ring_bonds(L))
    p = normal_vector(hub.nparam(L, bonds), 9880 + L).copy()
    p.setflags(write=False)
    return bonds, p


def weight_parts(L, kind):
    if kind == "real":
        return [normal_vector(L, 9890 + L)]
    re, im = ring_momentum_weights(L, 1)
    return [re.numpy(), im.numpy()]


def as_weights(parts, complex_tensor=False):
    if len(parts) == 1:
        return torch.from_numpy(parts[0].copy())
    parts = tuple(torch.from_numpy(q.copy()) for q in parts)
    return torch.complex(*parts) if complex_tensor else parts


def bulk(L, pair):
    return 1 <= pair[0] <= L - 1 and 1 <= pair[1] <= L - 1


def bulk_sources(L, channels, candidates):
    """the candidates that are bulk and whose destination is bulk under every channel listed"""
    return [s for s in candidates if bulk(L, s) and all(twin.destination(L, s[0], s[1], ch) is not None
                                                        and bulk(L, twin.destination(L, s[0], s[1], ch)) for ch in channels)]


# a few sources per L, so that the longdouble twin stays quick: both parities of nup (the sign of a down operator), nup != ndn
# both ways, and per channel at least two whose destination is bulk
CANDIDATES = {4: [(1, 1), (2, 2), (3, 2), (2, 3), (1, 3), (3, 1)], 5: [(2, 2), (3, 2), (2, 3), (1, 3), (4, 2), (3, 4)]}


@pytest.mark.parametrize("kind", ["real", "momentum"])
@pytest.mark.parametrize("channel", CHANNELS)
@pytest.mark.parametrize("L", [4, 5])
def test_hubbard_thermal_dynamics_sampled_against_the_twin(L, channel, kind):
    """dense_below = 0 on sources whose destination is bulk: every pair runs on the thermal pure quantum states, through the block ladder
    map, time_evolve and the fused dots, against the longdouble twin on the same start vectors"""
    bonds, p = ring_model(L)
    parts = weight_parts(L, kind)
    sources = bulk_sources(L, [channel], CANDIDATES[L])[:3]
    assert len(sources) >= 2
    R, seed, dt, steps = 4, 11, 0.3, 6
    got = thermal.hubbard_thermal_dynamics(L, bonds, to_dev(p), as_weights(parts), channel, BETAS, MUS, dt, steps, R=R, seed=seed,
                                           dense_below=0, sectors=sources)
    want = twin.thermal_dynamics(L, bonds, p, parts, channel, BETAS, MUS, dt, steps, R=R, seed=seed, dense_below=0, sectors=sources,
                                 dtype=LD)
    assert got.correlation.shape == (3, 2, steps + 1) and got.correlation.dtype == torch.complex128 and got.correlation.device.type == "cpu"
    assert torch.equal(got.times, dt * torch.arange(steps + 1, dtype=F64)) and torch.equal(got.betas, torch.tensor(BETAS, dtype=F64))
    assert torch.equal(got.mus, torch.tensor(MUS, dtype=F64)) and got.logXi.shape == (3, 2)
    C, ref_C = got.correlation.numpy(), want["C"].astype(np.complex128)
    static = ref_C[:, :, 0].real
    assert (static > 0).all() and want["orders"][:, 0].min() >= 0 and want["orders"][:, 1:].min() > 0
    bar = 1e-13 * np.maximum(want["orders"], 1.0)[:, None, :] * static[:, :, None]
    err = np.abs(C - ref_C)
    print("L = %d %s %s %s: worst |C - twin| / (1e-13 orders C(0)) = %.3f (orders up to %d)"
          % (L, channel, kind, sources, float((err / bar).max()), int(want["orders"].max())))
    assert (err <= bar).all()
    # ln Xi: the log norms of the imaginary-time steps, the same form of bar on the orders of those steps alone
    assert (np.abs(got.logXi.numpy() - want["logXi"]) <= 1e-13 * np.maximum(want["orders"][:, :1], 10.0)).all()
    assert torch.equal(got.static(), got.correlation[:, :, 0].real)


@pytest.mark.parametrize("kind", ["real", "momentum"])
@pytest.mark.parametrize("channel", CHANNELS)
def test_hubbard_thermal_dynamics_dense_against_the_full_fock_space(channel, kind):
    """L = 4, all 25 sources at the default dense_below: every pair is dense (at most 36 rows); against
    tr[e^{-beta (H - mu N)} e^{iHt} A^+ e^{-iHt} A] / Xi over all 4^4 states"""
    L = 4
    bonds, p = ring_model(L)
    parts = weight_parts(L, kind)
    dt, steps = 0.3, 6
    got = thermal.hubbard_thermal_dynamics(L, bonds, to_dev(p), as_weights(parts, complex_tensor=True), channel, BETAS, MUS, dt, steps)
    logXi, C = twin.full_space(L, bonds, p, parts, channel, BETAS, MUS, dt * np.arange(steps + 1))
    scale = C[:, :, :1].real
    err = np.abs(got.correlation.numpy() - C) / scale
    print("%s %s: |C - full space| / C(0) = %.2e, |ln Xi - full space| = %.2e"
          % (channel, kind, float(err.max()), float(np.abs(got.logXi.numpy() - logXi).max())))
    assert (scale > 0).all() and (err <= TOL).all()
    assert np.abs(got.logXi.numpy() - logXi).max() <= TOL


@pytest.mark.parametrize("dense_below", [0, 256])
def test_the_exact_identities(dense_below):
    """On one source list and seed, sampled on bulk-only pairs (dense_below = 0) and with every pair dense (256):
    C_cdag(0) + C_c(0) = sum_i |w_i|^2 at every (beta, mu) -- {A, A^T} is that multiple of the identity for each real part of the
    weights, so the rule holds per sampled state, both runs having the states of the same source; channel "n" with unit weights is
    N^2 and "sz" with unit weights (nup - ndn)^2 in every source, constant in time -- per sampled state again, up to the rounding of
    the stepping, 1e-13 per Chebyshev order as everywhere; with every pair dense over all 25 sources <N^2> is the second moment of N
    of ``hubbard_thermodynamics`` on exact sectors."""
    L, R, seed, dt, steps = 5 if dense_below == 0 else 4, 4, 21, 0.3, 3
    bonds, p = ring_model(L)
    pd = to_dev(p)
    if dense_below == 0:
        sources = bulk_sources(L, ["c_up", "cdag_up", "c_dn", "cdag_dn"], [(2, 2), (3, 2), (2, 3)])
        assert len(sources) == 3
    else:
        sources = None
    run = lambda w, ch, k=0: thermal.hubbard_thermal_dynamics(L, bonds, pd, w, ch, BETAS, MUS, dt, k, R=R, seed=seed,  # noqa: E731
                                                              dense_below=dense_below, sectors=sources)
    for kind in ("real", "momentum"):
        parts = weight_parts(L, kind)
        total = float(sum((q ** 2).sum() for q in parts))
        for species in ("up", "dn"):
            add, rem = run(as_weights(parts), "cdag_" + species), run(as_weights(parts), "c_" + species)
            err = float((add.static() + rem.static() - total).abs().max())
            print("dense_below = %d %s %s: |C_cdag(0) + C_c(0) - sum |w|^2| = %.2e" % (dense_below, kind, species, err))
            assert err <= 1e-12 * total
            assert torch.equal(add.logXi, rem.logXi)
    ones = torch.ones(L, dtype=F64)
    orders = twin.thermal_dynamics(L, bonds, p, [np.ones(L)], "n", BETAS, MUS, dt, steps, R=R, seed=seed, dense_below=dense_below,
                                   sectors=sources)["orders"]
    for channel in ("n", "sz"):
        out = run(ones, channel, steps)
        C = out.correlation.numpy()
        bar = 1e-13 * np.maximum(orders, 10.0)[:, None, :] * C[:, :, :1].real
        assert (C[:, :, 0].real > 0).all() and (np.abs(C - C[:, :, :1].real) <= bar).all(), channel
        if dense_below:
            ens = thermal.hubbard_thermodynamics(L, bonds, pd, dense_below=1 << 30)
            for b, beta in enumerate(BETAS):
                for m, mu in enumerate(MUS):
                    logw = torch.log(ens.weights) - beta * (ens.poles - mu * ens.N)
                    prob = torch.exp(logw - torch.logsumexp(logw, dim=0))
                    value = ens.N if channel == "n" else 2.0 * ens.Sz
                    assert abs(float(out.static()[b, m]) - float((prob * value ** 2).sum())) <= TOL * float(out.static()[b, m])
                    assert abs(float(out.logXi[b, m]) - float(ens.logZ(beta, mu))) <= TOL


def test_example_thermal_spectral():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "hubbard", "thermal_spectral.py")
    spec = importlib.util.spec_from_file_location("hubbard_thermal_spectral", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = ex.main(L=4)                                              # every pair is dense: at most 36 rows
    assert out["L"] == 4 and len(out["T"]) == 2 and len(out["momenta"]) == len(out["A"]) == len(out["sum"]) == len(out["n_k"])
    A = np.asarray(out["A"])
    assert A.shape == (len(out["momenta"]), 2, len(out["omega"])) and np.isfinite(A).all()
    # one Nyquist period: the sum over it is the trapezoid transform's C_cdag(0) + C_c(0) = {c_k, c+_k} = 1
    d_omega = out["omega"][1] - out["omega"][0]
    assert np.abs(A.sum(axis=2) * d_omega - 1.0).max() <= 1e-6 and np.abs(np.asarray(out["sum"]) - 1.0).max() <= 1e-6
    assert A.min() >= -1e-9
    n_k = np.asarray(out["n_k"])
    assert ((n_k > 0) & (n_k < 1)).all()
    # half filling at mu = U / 2 on a bipartite ring: n(k) + n(k + pi) = 1
    assert out["momenta"] == [0, 1, 2] and np.abs(n_k[0] + n_k[2] - 1.0).max() <= 1e-10 and np.abs(n_k[1] - 0.5).max() <= 1e-10
