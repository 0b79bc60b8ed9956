"""The block ladder maps and the finite-temperature correlation functions without a GPU
(docs/design/35-finite-temperature-dynamics.md): the numpy twin of tests/ladder_block_reference.py against dense matrices, its
sampled estimator on the unit vectors against its dense C(t) (the assembly, the dropped cross terms of complex weights
included), ``ThermalDynamics.spectrum`` against Gaussians, and everything the library and ``thermal_dynamics`` refuse on the
host before any device work."""
import ctypes
import functools
import math
from ctypes import byref, c_int64, c_void_p

import numpy as np
import pytest
import torch

import ladder_block_reference as twin
import ladder_reference as ladref
import sector_block_reference as blockref
import sector_reference as ref
from dominantsparseeigenad_amd import _lib, thermal
from dominantsparseeigenad_amd.operators import ring_bonds, ring_momentum_weights
from dominantsparseeigenad_amd.synthetic import normal_vector

LD = np.longdouble
STEP = {"zz": 0, "-": 1, "+": -1}


@pytest.mark.parametrize("L,nd,step", [(4, 2, 1), (5, 2, -1), (6, 3, 0), (6, 1, -1), (6, 5, 1), (7, 3, 1)])
def test_the_block_map_and_the_dots_against_the_dense_matrix(L, nd, step):
    n_src, n_dst = ladref.sizes(L, nd, step)
    c = normal_vector(L, 3500 + L)
    X = np.stack([normal_vector(n_src, 3510 + j) for j in range(3)], axis=1)
    Lft = np.stack([normal_vector(n_dst, 3520 + j) for j in range(3)], axis=1)
    S = ladref.dense(L, nd, step, c)
    scale = np.linalg.norm(S, 2) * np.linalg.norm(X, axis=0)
    for dtype in (np.float64, LD):
        Y = twin.apply_block(L, nd, step, c, X, dtype)
        assert Y.shape == (n_dst, 3) and Y.dtype == dtype
        assert (np.linalg.norm((Y - S @ X).astype(np.float64), axis=0) <= 1e-14 * scale).all()
        d = twin.dots(L, nd, step, c, Lft, X, dtype)
        assert d.shape == (3,)
        assert (np.abs(d.astype(np.float64) - (Lft * (S @ X)).sum(axis=0)) <= 1e-14 * scale * np.linalg.norm(Lft, axis=0)).all()
    # the float64 block map IS the single-vector reference, column by column
    assert np.array_equal(twin.apply_block(L, nd, step, c, X)[:, 1], ladref.apply(L, nd, step, c, X[:, 1]))


def ring_case(L):
    bonds = tuple(ring_bonds(L))
    p = normal_vector(ref.nparam(L, bonds), 3530 + L).copy()            # random Jxy, Jz and fields: every sector differs
    return bonds, p


def site_weight_parts(L, kind):
    if kind == "real":
        return [normal_vector(L, 3540 + L)]
    re, im = ring_momentum_weights(L, 1)
    return [re.numpy(), im.numpy()]


def unit_vector_estimator(L, bonds, p, parts, step, betas, dt, steps, dtype):
    """the twin's sampled estimator of every sector pair on the n unit vectors, weight 1 each: tr, with no sampling"""
    B = 1.01 * blockref.coupling_bound(L, bonds, p)
    out = []
    for nd in range(L + 1):
        if not 0 <= nd + step <= L:
            out.append(twin.dense_pair(L, nd, step, bonds, p, parts, betas, dt * np.arange(steps + 1)))
            continue
        n = math.comb(L, nd)
        out.append(twin.sampled_pair(L, nd, step, bonds, p, parts, betas, dt, steps, np.eye(n), (-B, B), (-B, B), weight=1.0,
                                     dtype=dtype)[:2])
    logw = np.stack([q[0] for q in out])
    top = logw.max(axis=0)
    logZ = top + np.log(np.exp(logw - top).sum(axis=0))
    return logZ, sum(np.exp(logw[s] - logZ)[:, None] * out[s][1] for s in range(len(out)))


@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("channel", ["zz", "-", "+"])
@pytest.mark.parametrize("L", [4, 6])
def test_the_sampled_estimator_on_the_unit_vectors_is_the_dense_trace(L, channel, kind):
    bonds, p = ring_case(L)
    parts = site_weight_parts(L, kind)
    betas, dt, steps = np.array([0.0, 1.0]), 0.3, 3
    want = twin.thermal_dynamics(L, bonds, p, parts, STEP[channel], betas, dt, steps, dense_below=1 << 30)
    assert not want["orders"].any()
    logZ, C = unit_vector_estimator(L, bonds, p, parts, STEP[channel], betas, dt, steps, np.float64)
    _, C_long = unit_vector_estimator(L, bonds, p, parts, STEP[channel], betas, dt, steps, LD)
    scale = want["C"][:, 0].real
    assert (scale > 0).all() and np.abs(want["C"][:, 0].imag).max() <= 1e-14 * scale.max()
    own = float((np.abs(C - C_long) / scale[:, None]).max())
    bar = max(1e-13, 10.0 * own)
    err = float((np.abs(C - want["C"]) / scale[:, None]).max())
    print("L = %d %s %s: |estimator - dense| / C(0) = %.2e (fp64 - longdouble %.2e, bar %.2e)" % (L, channel, kind, err, own, bar))
    assert err <= bar
    assert np.abs(logZ - want["logZ"]).max() <= 1e-12


def test_the_dense_trace_against_the_full_space():
    """L = 4: C(t) of the twin against tr[e^{-beta H} e^{iHt} A^T e^{-iHt} A] / Z with 16 x 16 matrices"""
    import lattice_reference
    L = 4
    bonds, p = ring_case(L)
    H = lattice_reference.dense(L, bonds, ref.full_parameter(L, bonds, p))
    theta, V = np.linalg.eigh(H)
    betas, dt, steps = np.array([0.0, 0.8]), 0.4, 3
    lower = np.array([[0.0, 0.0], [1.0, 0.0]])                   # sets the bit: sigma^-
    site = {"zz": np.diag([1.0, -1.0]), "-": lower, "+": lower.T}
    for channel in ("zz", "-", "+"):
        c = normal_vector(L, 3550)
        A = sum(c[i] * lattice_reference._site_product(L, {i: site[channel]}) for i in range(L))
        M = (V.T @ A @ V) ** 2
        got = twin.thermal_dynamics(L, bonds, p, [c], STEP[channel], betas, dt, steps, dense_below=1 << 30)
        for b, beta in enumerate(betas):
            w = np.exp(-beta * (theta - theta.min()))
            for k in range(steps + 1):
                want = np.sum(w[None, :] * M * np.exp(-1j * k * dt * (theta[:, None] - theta[None, :]))) / w.sum()
                assert abs(got["C"][b, k] - want) <= 1e-12 * abs(got["C"][b, 0])
            assert abs(got["logZ"][b] - (np.log(w.sum()) - beta * theta.min())) <= 1e-12


@pytest.mark.parametrize("dt", [0.1, 0.25])
def test_the_spectrum_of_poles_is_a_sum_of_gaussians(dt):
    eta, t_end = 0.2, 40.0
    K = int(round(t_end / dt))
    eps = np.array([-5.0, -3.1, -1.7, 0.2, 1.3, 3.6, 5.0])
    w = 0.5 + np.abs(normal_vector(7, 3561))
    times = dt * np.arange(K + 1)
    C = (w[None, :] * np.exp(-1j * times[:, None] * eps[None, :])).sum(axis=1)
    omega = np.linspace(-7.0, 7.0, 281)
    want = (w[None, :] * np.exp(-0.5 * ((omega[:, None] - eps[None, :]) / eta) ** 2)).sum(axis=1) / (eta * math.sqrt(2.0 * math.pi))
    bar = 1e-12 * w.sum() / (eta * math.sqrt(2.0 * math.pi))
    out = thermal.ThermalDynamics(torch.tensor([0.0, 1.0], dtype=torch.float64), torch.from_numpy(times), torch.zeros(2, dtype=torch.float64),
                                  torch.from_numpy(np.stack([C, 2.0 * C])))
    got = out.spectrum(torch.from_numpy(omega), eta)
    assert got.shape == (2, omega.size) and got.dtype == torch.float64
    err = float(np.abs(got[0].numpy() - want).max())
    direct = float(np.abs(twin.spectrum(times, C, omega, eta)[0] - want).max())
    print("dt = %.2f: |spectrum - Gaussians| = %.2e, the direct sum %.2e (bar %.2e)" % (dt, err, direct, bar))
    assert eta * times[-1] >= 8.0 and math.pi / dt > 7.0 + 5.0          # (the window has decayed; no alias of a pole reaches omega)
    assert direct <= bar and err <= bar
    assert np.abs(got[1].numpy() - 2.0 * want).max() <= 2.0 * bar
    assert torch.equal(out.static(), torch.tensor([float(w.sum()), 2.0 * float(w.sum())], dtype=torch.float64))
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            out.spectrum(omega, bad)


def test_thermal_dynamics_argument_errors_need_no_device():
    L, bonds = 6, ring_bonds(6)
    c = torch.zeros(3 * L, dtype=torch.float64)
    w = torch.ones(L, dtype=torch.float64)
    good = dict(L=L, bonds=bonds, couplings=c, weights=w, channel="zz", betas=[0.0, 1.0], dt=0.1, steps=4)
    nan = torch.tensor([1.0] * (L - 1) + [float("nan")], dtype=torch.float64)
    for bad in (dict(channel="xx"), dict(couplings=c[:-1]), dict(weights=w[:-1]), dict(weights=nan), dict(weights=(w, w[:-1])),
                dict(weights=torch.complex(w, nan)), dict(betas=[1.0, 0.5]), dict(betas=[-0.1, 1.0]), dict(betas=[]),
                dict(betas=[0.0, float("inf")]), dict(dt=0.0), dict(dt=-0.1), dict(dt=float("nan")), dict(dt=float("inf")),
                dict(steps=-1), dict(R=0), dict(sectors=[1, 1]), dict(sectors=[7]), dict(sectors=[]), dict(bonds=[(0, 6)])):
        with pytest.raises(ValueError):
            thermal.thermal_dynamics(**dict(good, **bad))


def test_the_edge_pairs_need_no_device():
    """sources whose pair has only edge sectors (ndown = 0 and L in the zz channel) or no destination: host arithmetic only"""
    L, bonds = 6, tuple(ring_bonds(6))
    p = normal_vector(3 * L, 3570).copy()
    c = normal_vector(L, 3571)
    betas, dt, steps = [0.0, 0.7], 0.25, 5
    out = thermal.thermal_dynamics(L, bonds, torch.from_numpy(p.copy()), torch.from_numpy(c.copy()), "zz", betas, dt, steps, sectors=[0, L])
    want = twin.thermal_dynamics(L, bonds, p, [c], 0, betas, dt, steps, sectors=[0, L])
    assert out.correlation.shape == (2, steps + 1) and out.correlation.dtype == torch.complex128
    assert torch.equal(out.times, dt * torch.arange(steps + 1, dtype=torch.float64))
    assert np.abs(out.logZ.numpy() - want["logZ"]).max() <= 1e-13
    assert np.abs(out.correlation.numpy() - want["C"]).max() <= 1e-13 * c.sum() ** 2
    # (Z(c) is diagonal with the one entry +- sum c in the two sectors: C(t) = (sum c)^2 at every time)
    assert np.abs(out.correlation.numpy() - c.sum() ** 2).max() <= 1e-13 * c.sum() ** 2
    re, im = ring_momentum_weights(L, 2)
    for channel, nd in (("-", L), ("+", 0)):
        out = thermal.thermal_dynamics(L, bonds, torch.from_numpy(p.copy()), (re, im), channel, betas, dt, steps, sectors=[nd])
        want = twin.thermal_dynamics(L, bonds, p, [re.numpy(), im.numpy()], STEP[channel], betas, dt, steps, sectors=[nd])
        assert float(out.correlation.abs().max()) == 0.0 and np.abs(out.logZ.numpy() - want["logZ"]).max() <= 1e-13
        assert torch.equal(out.static(), torch.zeros(2, dtype=torch.float64))


def test_the_host_ladder_matrix_is_the_reference_matrix():
    for L, nd, step in ((4, 2, 1), (5, 2, -1), (6, 3, 0), (6, 0, 1), (6, 1, -1), (6, 6, -1), (6, 5, 1), (6, 0, 0), (6, 6, 0)):
        c = normal_vector(L, 3580 + L)
        got = thermal._dense_ladder_matrix(L, nd, step, torch.from_numpy(c.copy()))
        assert np.array_equal(got.numpy(), ladref.dense(L, nd, step, c)), (L, nd, step)


# ---- the C ABI: every refusal is host arithmetic before any device work (host memory stands in for the blocks)
@functools.lru_cache(maxsize=None)
def host_store():
    store = (ctypes.c_double * 4096)()
    base = ctypes.addressof(store)
    return store, base + (-base % 16)


def abi_calls():
    lib = _lib.load()
    _, base = host_store()
    P = lambda i: c_void_p(base + 256 * i)  # noqa: E731
    good = dict(L=8, nd=4, step=1, R=8, c=P(0), states=P(1), lo=P(2), hi=P(3), X=P(4), Y=P(5), Lft=P(6), out=P(7), scratch=P(8), grid=0)

    def apply(**kw):
        a = dict(good, **kw)
        return lib.dsea_sector_ladder_block_apply(a["L"], a["nd"], a["step"], a["R"], a["c"], a["states"], a["lo"], a["hi"], a["X"],
                                                  a["Y"], a["grid"], None)

    def dots(**kw):
        a = dict(good, **kw)
        return lib.dsea_sector_ladder_block_dots(a["L"], a["nd"], a["step"], a["R"], a["c"], a["states"], a["lo"], a["hi"], a["Lft"],
                                                 a["X"], a["out"], a["scratch"], a["grid"], None)

    return lib, P, c_void_p(base + 256 * 9 + 8), apply, dots


def test_the_abi_refuses_before_any_device_work():
    lib, P, odd, apply, dots = abi_calls()
    null = c_void_p(None)
    # what dsea_sector_ladder_apply refuses (tests/test_gpu_ladder.py), and the widths
    shared = [dict(step=2), dict(step=-2), dict(nd=7, step=1), dict(nd=1, step=-1), dict(nd=0, step=1), dict(nd=8, step=-1),
              dict(L=41, nd=1), dict(L=1, nd=1, step=0), dict(L=36, nd=17), dict(grid=5), dict(grid=13), dict(grid=-1), dict(grid=1),
              dict(states=null), dict(lo=null), dict(hi=null), dict(c=null), dict(X=null),
              dict(R=0), dict(R=3), dict(R=5), dict(R=6), dict(R=16), dict(R=-1)]
    for bad in shared + [dict(Y=null), dict(Y=P(4)), dict(step=-1, Y=P(4))]:
        assert apply(**bad) == _lib.ERR_ARG, bad
    for bad in shared + [dict(Lft=null), dict(out=null), dict(scratch=null)]:
        assert dots(**bad) == _lib.ERR_ARG, bad
    ERR_ALIGN = -2
    for R in (1, 2, 4, 8):
        assert apply(R=R, X=odd) == ERR_ALIGN and apply(R=R, Y=odd) == ERR_ALIGN
        assert dots(R=R, X=odd) == ERR_ALIGN and dots(R=R, Lft=odd) == ERR_ALIGN
    assert apply(R=3, X=odd) == _lib.ERR_ARG                       # (the argument checks come first)
    store, _ = host_store()
    assert not any(store)                                           # nothing was written


def test_the_dots_scratch_sizes():
    lib = _lib.load()
    need = c_int64(-1)
    for bad in ((8, 4, 2, 8), (8, 7, 1, 8), (8, 1, -1, 8), (41, 1, 1, 8), (36, 17, 1, 8), (8, 4, 1, 3), (8, 4, 1, 0), (8, 4, 1, 16)):
        assert lib.dsea_sector_ladder_block_dots_scratch_doubles(*bad, byref(need)) == _lib.ERR_ARG and need.value == -1
    assert lib.dsea_sector_ladder_block_dots_scratch_doubles(8, 4, 1, 8, None) == _lib.ERR_ARG
    for (L, nd, step), n_dst in (((8, 4, 1), 56), ((11, 5, 1), 462), ((20, 10, 1), 167960), ((24, 12, 1), 2496144),
                                 ((24, 12, 0), 2704156), ((24, 12, -1), 2496144)):
        assert math.comb(L, nd + step) == n_dst
        for R in (1, 2, 4, 8):
            assert lib.dsea_sector_ladder_block_dots_scratch_doubles(L, nd, step, R, byref(need)) == 0
            assert need.value == R * min(4096, (n_dst + 255) // 256)


class _Tables:
    """what SpinSectorLadder reads of an operator, with host tensors: enough for the checks that come before the device"""

    def __init__(self, L, ndown):
        self.N, self.ndown, self.device = L, ndown, torch.device("cpu")
        self._tables = (torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))


def test_the_python_block_entries_refuse_on_the_host():
    from dominantsparseeigenad_amd.operators import SpinSectorLadder
    lad = SpinSectorLadder(_Tables(6, 3), _Tables(6, 4))
    assert (lad.n_src, lad.n_dst) == (20, 15)
    c = torch.ones(6, dtype=torch.float64)
    X, Lft = torch.zeros((20, 3), dtype=torch.float64), torch.zeros((15, 3), dtype=torch.float64)
    for call in (lambda: lad.apply_block(c, X[:19]), lambda: lad.apply_block(c, X[:, 0]), lambda: lad.apply_block(c, X[:, :0]),
                 lambda: lad.apply_block(c, [1.0]), lambda: lad.apply_block(c[:5], X), lambda: lad.apply_block(c, X.to(torch.complex128)),
                 lambda: lad.apply_block(torch.complex(c, c), X), lambda: lad.apply_block(c, X.to("meta")),
                 lambda: lad.block_dots(c, X, X), lambda: lad.block_dots(c, Lft[:, :2], X), lambda: lad.block_dots(c, Lft, X[:, 0]),
                 lambda: lad.block_dots(c[:5], Lft, X), lambda: lad.T.apply_block(c, X), lambda: lad.T.block_dots(c, Lft, X)):
        with pytest.raises(ValueError):
            call()
