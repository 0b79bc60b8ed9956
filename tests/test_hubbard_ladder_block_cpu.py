"""The block Hubbard ladder maps and the finite-temperature Hubbard correlation functions without a GPU
(docs/design/37-hubbard-finite-temperature-dynamics.md): the numpy twin of tests/hubbard_ladder_block_reference.py against dense
matrices, its sampled estimator on the unit vectors against its dense C(t) (the assembly over (nup, ndn) with the chemical
potential, the dropped cross terms of complex weights included), its dense C(t; beta, mu) against the full 4^L Fock space, the
host matrix of A with edge sectors, and everything the library and ``hubbard_thermal_dynamics`` refuse on the host before any
device work."""
import ctypes
import functools
import math
from ctypes import byref, c_int64, c_void_p

import numpy as np
import pytest
import torch

import hubbard_ladder_block_reference as twin
import hubbard_ladder_reference as ladref
import hubbard_reference as hub
from dominantsparseeigenad_amd import _lib, thermal
from dominantsparseeigenad_amd.operators import HubbardLadder, ring_bonds, ring_momentum_weights
from dominantsparseeigenad_amd.synthetic import normal_vector

LD = np.longdouble
F64 = torch.float64
UP, DN = ladref.UP, ladref.DN
CHANNELS = ["c_up", "c_dn", "cdag_up", "cdag_dn", "n", "sz"]
NAME = {UP: "up", DN: "dn"}


def test_the_host_ladder_matrix_is_the_reference_matrix():
    cases = ((3, 1, 1, UP, 1), (4, 2, 1, DN, 1), (4, 3, 2, DN, -1), (5, 2, 3, UP, -1), (5, 2, 2, UP, 0), (5, 3, 2, DN, 0),
             (4, 0, 2, DN, -1), (4, 0, 1, DN, -1), (4, 1, 4, UP, 1), (4, 1, 2, UP, -1), (4, 3, 3, DN, 1), (4, 3, 1, UP, 1),
             (4, 0, 0, UP, 1), (4, 4, 4, DN, -1), (4, 0, 4, UP, 0), (4, 3, 0, DN, 0), (4, 4, 2, DN, 0))
    for L, nup, ndn, species, step in cases:
        w = normal_vector(L, 3750 + L)
        got = thermal._dense_hubbard_ladder_matrix(L, nup, ndn, NAME[species], step, torch.from_numpy(w.copy()))
        assert np.array_equal(got.numpy(), ladref.dense(L, nup, ndn, species, step, w)), (L, nup, ndn, species, step)


@pytest.mark.parametrize("L,nup,ndn,species,step", [(3, 1, 1, UP, 1), (4, 2, 1, DN, 1), (4, 3, 2, DN, -1), (5, 2, 3, UP, -1),
                                                    (5, 2, 2, UP, 0), (5, 3, 2, DN, 0), (4, 0, 2, DN, -1), (4, 1, 4, UP, 1)])
def test_the_block_map_and_the_dots_against_the_dense_matrix(L, nup, ndn, species, step):
    n_src, n_dst = ladref.sizes(L, nup, ndn, species, step)
    w = normal_vector(L, 3700 + L)
    X = np.stack([normal_vector(n_src, 3710 + j) for j in range(3)], axis=1)
    Lft = np.stack([normal_vector(n_dst, 3720 + j) for j in range(3)], axis=1)
    S = ladref.dense(L, nup, ndn, species, step, w)
    scale = np.linalg.norm(S, 2) * np.linalg.norm(X, axis=0)
    for dtype in (np.float64, LD):
        Y = twin.apply_block(L, nup, ndn, species, step, w, X, dtype)
        assert Y.shape == (n_dst, 3) and Y.dtype == dtype
        assert (np.linalg.norm((Y - S @ X).astype(np.float64), axis=0) <= 1e-14 * scale).all()
        d = twin.dots(L, nup, ndn, species, step, w, Lft, X, dtype)
        assert d.shape == (3,)
        assert (np.abs(d.astype(np.float64) - (Lft * (S @ X)).sum(axis=0)) <= 1e-14 * scale * np.linalg.norm(Lft, axis=0)).all()
    # the float64 block map IS the single-vector reference, column by column
    assert np.array_equal(twin.apply_block(L, nup, ndn, species, step, w, X)[:, 1], ladref.apply(L, nup, ndn, species, step, w, X[:, 1]))


def ring_case(L):
    bonds = tuple(ring_bonds(L))
    p = normal_vector(hub.nparam(L, bonds), 3730 + L).copy()            # random t, V, U and eps: every sector differs
    return bonds, p


def site_weight_parts(L, kind):
    if kind == "real":
        return [normal_vector(L, 3740 + L)]
    re, im = ring_momentum_weights(L, 1)
    return [re.numpy(), im.numpy()]


def all_pairs(L):
    return [(a, b) for a in range(L + 1) for b in range(L + 1)]


def exact_bounds(L, nup, ndn, bonds, p):
    """the interval ``spectral_bounds`` aims at, from the sector's exact spectrum: its ends widened by 5 % of its width.  The
    rigorous (-B, B) of the coupling bound is several times wider than a sector's spectrum here, and e^{-tau H} expanded on an
    interval whose lower end lies far below the spectrum loses, at the states that carry the trace, the factor e^{tau (E_0 - a)}
    of relative accuracy to the truncation -- in fp64 and in longdouble alike, so that their difference would not show it."""
    theta = twin._spectrum_of(L, nup, ndn, bonds, p)[0]
    pad = 0.05 * (theta[-1] - theta[0])
    if not pad > 0:
        pad = 0.05 * max(1.0, abs(theta[0]))
    return theta[0] - pad, theta[-1] + pad


def unit_vector_estimator(L, bonds, p, parts, channel, betas, mus, dt, steps, dtype):
    """the twin's sampled estimator of every pair on the n unit vectors, weight 1 each: the trace, with no sampling"""
    out = []
    for nup, ndn in all_pairs(L):
        other = twin.destination(L, nup, ndn, channel)
        if other is None:
            out.append(twin.dense_pair(L, nup, ndn, channel, bonds, p, parts, betas, dt * np.arange(steps + 1)))
            continue
        n = math.comb(L, nup) * math.comb(L, ndn)
        out.append(twin.sampled_pair(L, nup, ndn, channel, bonds, p, parts, betas, dt, steps, np.eye(n),
                                     exact_bounds(L, nup, ndn, bonds, p), exact_bounds(L, other[0], other[1], bonds, p),
                                     weight=1.0, dtype=dtype)[:2])
    return twin.combine(out, all_pairs(L), betas, mus)


@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("channel", CHANNELS)
@pytest.mark.parametrize("L", [3, 4])
def test_the_sampled_estimator_on_the_unit_vectors_is_the_dense_trace(L, channel, kind):
    bonds, p = ring_case(L)
    parts = site_weight_parts(L, kind)
    betas, mus, dt, steps = np.array([0.0, 1.0]), np.array([-0.4, 0.9]), 0.3, 2
    want = twin.thermal_dynamics(L, bonds, p, parts, channel, betas, mus, dt, steps, dense_below=1 << 30)
    assert not want["orders"].any()
    logXi, C = unit_vector_estimator(L, bonds, p, parts, channel, betas, mus, dt, steps, np.float64)
    logXi_long, C_long = unit_vector_estimator(L, bonds, p, parts, channel, betas, mus, dt, steps, LD)
    scale = want["C"][:, :, 0].real
    assert (scale > 0).all() and np.abs(want["C"][:, :, 0].imag).max() <= 1e-14 * scale.max()
    own = float((np.abs(C - C_long) / scale[:, :, None]).max())
    bar = max(1e-13, 10.0 * own)
    err = float((np.abs(C - want["C"]) / scale[:, :, None]).max())
    print("L = %d %s %s: |estimator - dense| / C(0) = %.2e (fp64 - longdouble %.2e, bar %.2e)" % (L, channel, kind, err, own, bar))
    assert err <= bar
    # ln Xi: a relative error of Xi, so the same form of bar on the estimator's own fp64 - longdouble deviation
    assert np.abs(logXi - want["logXi"]).max() <= max(1e-13, 10.0 * float(np.abs(logXi - logXi_long).max()))


@pytest.mark.parametrize("channel", CHANNELS)
def test_the_dense_trace_against_the_full_fock_space(channel):
    """L = 3: C(t; beta, mu) of the twin over all 16 sectors against the 64-state space with Jordan-Wigner matrices"""
    L = 3
    bonds, p = ring_case(L)
    betas, mus, dt, steps = np.array([0.0, 0.8]), np.array([-0.5, 0.0, 1.1]), 0.4, 3
    for parts in (site_weight_parts(L, "real"), site_weight_parts(L, "complex")):
        got = twin.thermal_dynamics(L, bonds, p, parts, channel, betas, mus, dt, steps, dense_below=1 << 30)
        logXi, C = twin.full_space(L, bonds, p, parts, channel, betas, mus, dt * np.arange(steps + 1))
        assert got["C"].shape == (2, 3, steps + 1)
        assert np.abs(got["logXi"] - logXi).max() <= 1e-10
        assert (np.abs(got["C"] - C) <= 1e-10 * np.abs(C[:, :, :1])).all()


def test_the_fock_space_restricts_to_the_sector_reference():
    """the operators of ``full_space`` are those of the sector references: H and A between two sectors, in their row order"""
    L = 3
    bonds, p = ring_case(L)
    H, N = twin.fock_hamiltonian(L, bonds, p)
    index = lambda nup, ndn: np.array([u | (d << L) for u in hub.states(L, nup) for d in hub.states(L, ndn)], dtype=np.int64)  # noqa: E731
    assert np.abs(H[np.ix_(index(2, 1), index(2, 1))] - hub.dense(L, 2, 1, bonds, p)).max() <= 1e-14
    assert np.array_equal(np.diag(N)[index(2, 1)], np.full(9, 3.0))
    w = normal_vector(L, 3745)
    for channel, (nup, ndn) in (("c_up", (2, 1)), ("c_dn", (1, 2)), ("cdag_dn", (1, 0)), ("cdag_up", (2, 3)), ("sz", (2, 1))):
        other = twin.destination(L, nup, ndn, channel)
        A = twin.fock_channel(L, channel, w)
        assert np.abs(A[np.ix_(index(*other), index(nup, ndn))] - twin.channel_dense(L, nup, ndn, channel, w)).max() <= 1e-14


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
    good = dict(L=8, nup=4, ndn=3, species=0, step=1, R=8, c=P(0), states=P(1), lo=P(2), hi=P(3), X=P(4), Y=P(5), Lft=P(6), out=P(7),
                scratch=P(8), grid=0)

    def apply(**kw):
        a = dict(good, **kw)
        return lib.dsea_hubbard_ladder_block_apply(a["L"], a["nup"], a["ndn"], a["species"], a["step"], a["R"], a["c"], a["states"],
                                                   a["lo"], a["hi"], a["X"], a["Y"], a["grid"], None)

    def dots(**kw):
        a = dict(good, **kw)
        return lib.dsea_hubbard_ladder_block_dots(a["L"], a["nup"], a["ndn"], a["species"], a["step"], a["R"], a["c"], a["states"],
                                                  a["lo"], a["hi"], a["Lft"], a["X"], a["out"], a["scratch"], a["grid"], None)

    return lib, P, c_void_p(base + 256 * 9 + 8), apply, dots


def test_the_abi_refuses_before_any_device_work():
    lib, P, odd, apply, dots = abi_calls()
    null = c_void_p(None)
    # what dsea_hubbard_ladder_apply refuses (tests/test_gpu_hubbard_ladder.py), and the widths
    shared = [dict(step=2), dict(step=-2), dict(species=2), dict(species=-1), dict(nup=7, step=1), dict(nup=1, step=-1),
              dict(species=1, ndn=7, step=1), dict(species=1, ndn=1, step=-1), dict(nup=0, step=1), dict(nup=8, step=-1), dict(ndn=0),
              dict(ndn=8), dict(L=41, nup=1, ndn=1), dict(L=1, nup=1, ndn=1, step=0), dict(L=36, nup=17, ndn=18), dict(grid=5),
              dict(grid=13), dict(grid=-1), dict(grid=1), dict(states=null), dict(lo=null), dict(hi=null), dict(c=null), dict(X=null),
              dict(R=0), dict(R=3), dict(R=5), dict(R=6), dict(R=16), dict(R=-1)]
    for bad in shared + [dict(Y=null), dict(Y=P(4)), dict(step=-1, Y=P(4)), dict(species=1, Y=P(4))]:
        assert apply(**bad) == _lib.ERR_ARG, bad
    for bad in shared + [dict(Lft=null), dict(out=null), dict(scratch=null)]:
        assert dots(**bad) == _lib.ERR_ARG, bad
    ERR_ALIGN = -2
    for R in (1, 2, 4, 8):
        assert apply(R=R, X=odd) == ERR_ALIGN and apply(R=R, Y=odd) == ERR_ALIGN
        assert dots(R=R, X=odd) == ERR_ALIGN and dots(R=R, Lft=odd) == ERR_ALIGN
        assert apply(R=R, step=0, X=odd, Y=odd) == ERR_ALIGN        # (X == Y passes the argument checks at step 0)
    assert apply(R=3, X=odd) == _lib.ERR_ARG                       # (the argument checks come first)
    store, _ = host_store()
    assert not any(store)                                           # nothing was written


def test_the_dots_scratch_sizes():
    lib = _lib.load()
    need = c_int64(-1)
    for bad in ((8, 4, 3, 0, 2, 8), (8, 7, 3, 0, 1, 8), (8, 1, 3, 0, -1, 8), (8, 4, 7, 1, 1, 8), (8, 4, 3, 2, 1, 8), (41, 1, 1, 0, 1, 8),
                (36, 17, 18, 0, 1, 8), (8, 4, 3, 0, 1, 3), (8, 4, 3, 0, 1, 0), (8, 4, 3, 0, 1, 16)):
        assert lib.dsea_hubbard_ladder_block_dots_scratch_doubles(*bad, byref(need)) == _lib.ERR_ARG and need.value == -1
    assert lib.dsea_hubbard_ladder_block_dots_scratch_doubles(8, 4, 3, 0, 1, 8, None) == _lib.ERR_ARG
    for (L, nup, ndn, species, step), n_dst in (((3, 1, 1, 0, 1), 9), ((7, 3, 4, 0, 1), 1225), ((8, 4, 3, 1, 1), 4900),
                                                ((12, 5, 5, 0, 1), 731808), ((14, 7, 7, 0, 1), 10306296), ((14, 7, 7, 1, 0), 11778624),
                                                ((16, 5, 5, 1, -1), 7949760)):
        assert ladref.destination(nup, ndn, species, step) and math.prod(
            math.comb(L, k) for k in ladref.destination(nup, ndn, species, step)) == n_dst
        for R in (1, 2, 4, 8):
            assert lib.dsea_hubbard_ladder_block_dots_scratch_doubles(L, nup, ndn, species, step, R, byref(need)) == 0
            assert need.value == R * min(4096, (n_dst + 255) // 256)


class _Tables:
    """what HubbardLadder reads of an operator, with host tensors: enough for the checks that come before the device"""

    def __init__(self, L, nup, ndn):
        self.N, self.nup, self.ndn, self.device = L, nup, ndn, torch.device("cpu")
        self._up = self._dn = (torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))


def test_the_python_block_entries_refuse_on_the_host():
    lad = HubbardLadder(_Tables(5, 2, 3), _Tables(5, 3, 3))
    assert (lad.n_src, lad.n_dst) == (100, 100) and lad.species == "up" and lad.step == 1
    down = HubbardLadder(_Tables(5, 2, 3), _Tables(5, 2, 2))
    assert (down.n_src, down.n_dst) == (100, 100)
    other = HubbardLadder(_Tables(6, 3, 3), _Tables(6, 3, 2))
    assert (other.n_src, other.n_dst) == (400, 300)
    w = torch.ones(5, dtype=F64)
    X, Lft = torch.zeros((100, 3), dtype=F64), torch.zeros((100, 3), dtype=F64)
    X6, L6 = torch.zeros((400, 3), dtype=F64), torch.zeros((300, 3), dtype=F64)
    w6 = torch.ones(6, dtype=F64)
    for call in (lambda: lad.apply_block(w, X[:99]), lambda: lad.apply_block(w, X[:, 0]), lambda: lad.apply_block(w, X[:, :0]),
                 lambda: lad.apply_block(w, [1.0]), lambda: lad.apply_block(w[:4], X), lambda: lad.apply_block(w, X.to(torch.complex128)),
                 lambda: lad.apply_block(torch.complex(w, w), X), lambda: lad.apply_block(w, X.to("meta")),
                 lambda: lad.block_dots(w, Lft[:, :2], X), lambda: lad.block_dots(w, Lft, X[:, 0]), lambda: lad.block_dots(w[:4], Lft, X),
                 lambda: lad.block_dots(w, Lft.to(torch.complex128), X), lambda: lad.block_dots(w, Lft.to("meta"), X),
                 lambda: other.block_dots(w6, X6, X6), lambda: other.T.apply_block(w6, X6), lambda: other.T.block_dots(w6, L6, X6),
                 lambda: down.T.apply_block(w, X[:50])):
        with pytest.raises(ValueError):
            call()


def test_hubbard_thermal_dynamics_argument_errors_need_no_device(monkeypatch):
    L, bonds = 4, ring_bonds(4)
    c = torch.zeros(2 * 4 + 2 * L, dtype=F64)
    w = torch.ones(L, dtype=F64)
    good = dict(L=L, bonds=bonds, couplings=c, weights=w, channel="c_up", betas=[0.0, 1.0], mus=[0.0, 0.5], dt=0.1, steps=4)
    nan = torch.tensor([1.0] * (L - 1) + [float("nan")], dtype=F64)
    for bad in (dict(channel="zz"), dict(channel="c"), dict(couplings=c[:-1]), dict(weights=w[:-1]), dict(weights=nan),
                dict(weights=(w, w[:-1])), dict(weights=torch.complex(w, nan)), dict(betas=[1.0, 0.5]), dict(betas=[-0.1, 1.0]),
                dict(betas=[]), dict(betas=[0.0, float("inf")]), dict(mus=[]), dict(mus=[float("nan")]), dict(mus=[0.0, float("inf")]),
                dict(dt=0.0), dict(dt=-0.1), dict(dt=float("nan")), dict(dt=float("inf")), dict(steps=-1), dict(R=0),
                dict(sectors=[(1, 1), (1, 1)]), dict(sectors=[(5, 1)]), dict(sectors=[(1, -1)]), dict(sectors=[]), dict(bonds=[(0, 4)]),
                dict(L=1), dict(L=41)):
        with pytest.raises(ValueError):
            thermal.hubbard_thermal_dynamics(**dict(good, **bad))

    # an edge pair is exact on the host: a side above edge_dense_max is refused BEFORE any sector is computed
    def never(*args, **kwargs):
        raise AssertionError("a sector was computed before the refusal")

    for name in ("_dense_pair_dynamics", "_tpq_block_dynamics", "one_species_matrix", "_dense_sector_matrix"):
        monkeypatch.setattr(thermal, name, never)
    L, bonds = 8, ring_bonds(8)
    c = torch.zeros(2 * 8 + 2 * L, dtype=F64)
    w = torch.ones(L, dtype=F64)
    big = dict(L=L, bonds=bonds, couplings=c, weights=w, betas=[0.0], mus=[0.0], dt=0.1, steps=1, edge_dense_max=100)
    # (1, 4) -> (0, 4): the destination is an edge sector of 70 rows, the source has 8 * 70 = 560
    with pytest.raises(ValueError, match="edge_dense_max"):
        thermal.hubbard_thermal_dynamics(channel="c_up", sectors=[(0, 1), (1, 4)], **big)
    with pytest.raises(ValueError, match="edge_dense_max"):
        thermal.hubbard_thermal_dynamics(channel="cdag_dn", sectors=[(8, 1), (4, 7)], **big)
    with pytest.raises(ValueError, match="edge_dense_max"):
        thermal.hubbard_thermal_dynamics(channel="n", sectors=[(0, 4), (0, 3)], edge_dense_max=60, **{k: v for k, v in big.items()
                                                                                                      if k != "edge_dense_max"})


@pytest.mark.parametrize("channel,sectors", [("c_dn", [(0, 1), (0, 2), (0, 3), (5, 4), (5, 5), (0, 0)]),
                                             ("cdag_up", [(0, 0), (1, 0), (3, 5), (4, 5), (5, 2)]),
                                             ("c_up", [(1, 0), (5, 5), (5, 0), (0, 3)]),
                                             ("n", [(0, 0), (0, 2), (3, 5), (5, 5)]), ("sz", [(0, 3), (2, 0), (5, 1)])])
def test_the_edge_pairs_need_no_device(channel, sectors):
    """sources whose pairs hold edge sectors only (or have no destination): host arithmetic only, against the twin"""
    L, bonds = 5, tuple(ring_bonds(5))
    p = normal_vector(hub.nparam(L, bonds), 3770).copy()
    betas, mus, dt, steps = [0.0, 0.7], [-0.3, 0.6, 1.4], 0.25, 4
    for kind in ("real", "complex"):
        parts = site_weight_parts(L, kind)
        weights = torch.from_numpy(parts[0].copy()) if kind == "real" else torch.complex(*(torch.from_numpy(q.copy()) for q in parts))
        out = thermal.hubbard_thermal_dynamics(L, bonds, torch.from_numpy(p.copy()), weights, channel, betas, mus, dt, steps,
                                               sectors=sectors)
        want = twin.thermal_dynamics(L, bonds, p, parts, channel, betas, mus, dt, steps, sectors=sectors)
        assert out.correlation.shape == (2, 3, steps + 1) and out.correlation.dtype == torch.complex128
        assert out.logXi.shape == (2, 3) and torch.equal(out.mus, torch.tensor(mus, dtype=F64))
        assert torch.equal(out.times, dt * torch.arange(steps + 1, dtype=F64)) and torch.equal(out.betas, torch.tensor(betas, dtype=F64))
        assert np.abs(out.logXi.numpy() - want["logXi"]).max() <= 1e-12
        scale = np.abs(want["C"][:, :, :1])
        assert (scale > 0).all() and (np.abs(out.correlation.numpy() - want["C"]) <= 1e-12 * scale).all()
        assert torch.equal(out.static(), out.correlation[:, :, 0].real)


def test_the_spectrum_is_the_spin_transform_and_reflects():
    dt, K, eta = 0.1, 400, 0.2
    eps = np.array([-3.1, -1.7, 0.2, 1.3, 3.6])
    wgt = 0.5 + np.abs(normal_vector(5, 3780))
    times = dt * np.arange(K + 1)
    C = (wgt[None, :] * np.exp(-1j * times[:, None] * eps[None, :])).sum(axis=1)
    record = torch.from_numpy(np.stack([C, 2.0 * C, 3.0 * C, C.conj(), C, C]).reshape(2, 3, K + 1))
    out = thermal.HubbardThermalDynamics(torch.tensor([0.0, 1.0], dtype=F64), torch.tensor([0.0, 0.5, 1.0], dtype=F64),
                                         torch.from_numpy(times), torch.zeros((2, 3), dtype=F64), record)
    omega = np.linspace(-5.0, 5.0, 201)
    got = out.spectrum(omega, eta)
    assert got.shape == (2, 3, omega.size) and got.dtype == F64
    spin = thermal.ThermalDynamics(out.betas, out.times, torch.zeros(2, dtype=F64), record[:, 0])
    assert torch.equal(got[:, 0], spin.spectrum(omega, eta))
    want = (wgt[None, :] * np.exp(-0.5 * ((omega[:, None] - eps[None, :]) / eta) ** 2)).sum(axis=1) / (eta * math.sqrt(2.0 * math.pi))
    bar = 1e-12 * wgt.sum() / (eta * math.sqrt(2.0 * math.pi))
    assert np.abs(got[0, 0].numpy() - want).max() <= bar and np.abs(got[0, 2].numpy() - 3.0 * want).max() <= 3.0 * bar
    assert torch.equal(out.spectrum(omega, eta, reflected=True), out.spectrum(-omega, eta))
    assert np.abs(out.spectrum(omega, eta, reflected=True)[0, 0].numpy() - want[::-1]).max() <= bar
    assert torch.equal(out.static(), record[:, :, 0].real)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            out.spectrum(omega, bad)
