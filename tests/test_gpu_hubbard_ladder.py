"""The c / c+ / n maps between Hubbard sectors and the spectral functions built on them on the GPU
(docs/design/25-hubbard-ladder.md): k_hubbard_ladder and k_hubbard_ladder_forms against the numpy reference of
tests/hubbard_ladder_reference.py at the smallest sizes that reach each path, then the transpose, autograd against a dense twin
and through DominantSparseSymeig, the argument checks of the C ABI, the measure against the dense Lehmann sum, and the sum rules
of free and interacting rings end to end.

    L  (nup, ndn) src -> dst     n_src -> n_dst        what it reaches
    2  (1,1) -> (1,1) up, dn     4 -> 4                step 0, the smallest sector
    3  (1,1) -> (2,1), back      9 -> 9                the smallest step +-1
    5  (2,3) -> (2,2), back      100 -> 100            down species, the gather runs on the source's stride (C(5, 3) = C(5, 2) = 10:
                                                       the two strides differ from L = 10 on), n_dn < 64: several ru in one wave
    7  (3,4) -> (4,4)            1225 -> 1225          up species, low / high split 4 + 3
    7  (4,3) -> (4,4)            1225 -> 1225          down species behind an even nup
    10 (5,5) -> (4,5), (5,4)     63 504 -> 52 920      n_dn = 252 and 252 -> 210, no multiples of 64: waves straddle ru; down
                                                       species behind an odd nup
    12 (5,5) -> (6,5)            627 264 -> 731 808    2859 row ranges on a grid capped at 64 blocks: blocks walk ranges
    16 (2,1) -> (3,1)            1920 -> 8960          one full chunk of 8 sites in each group
    34 (2,1) -> (3,1)            19 074 -> 203 456     words wider than 32 bits
    40 (1,1) -> (2,1), back      1600 -> 31 200        words wider than 32 bits, three chunks in each group
    40 (1,2) -> (1,1)            31 200 -> 1600        the same for the down species, odd nup
    7, 16, 40                    step 0, both species
"""
import functools
import importlib.util
import math
import os
from ctypes import byref, c_int64, c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hubbard_ladder_reference as ref  # noqa: E402
import hubbard_reference as hub  # noqa: E402
import lattice_reference  # noqa: E402
from helpers import PatchRandn  # noqa: E402
from dominantsparseeigenad_amd import _lib, engine  # noqa: E402
from dominantsparseeigenad_amd.operators import (HubbardLadder, HubbardOperator, one_body_density_matrix, ring_bonds,  # noqa: E402
                                                 ring_momentum_weights)
from dominantsparseeigenad_amd.spectral import SpectralMeasure, hubbard_spectral_function  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402
import dominantsparseeigenad_amd.symeig as symeig  # noqa: E402
import dominantsparseeigenad_amd.CG as CG  # noqa: E402

F64 = torch.float64
TOL = 1e-10
SPECIES = {"up": ref.UP, "dn": ref.DN}

# name -> (L, (nup, ndn) of the source, (nup, ndn) of the destination, species, log2 of the grid cap or None for the default)
GEOMETRY = {
    "L2-11-up0": (2, (1, 1), (1, 1), "up", None),
    "L2-11-dn0": (2, (1, 1), (1, 1), "dn", None),
    "L3-11-21": (3, (1, 1), (2, 1), "up", None),
    "L3-21-11": (3, (2, 1), (1, 1), "up", None),
    "L5-23-22": (5, (2, 3), (2, 2), "dn", None),
    "L5-22-23": (5, (2, 2), (2, 3), "dn", None),
    "L7-34-44": (7, (3, 4), (4, 4), "up", None),
    "L7-43-44": (7, (4, 3), (4, 4), "dn", None),
    "L10-55-45": (10, (5, 5), (4, 5), "up", None),
    "L10-55-54": (10, (5, 5), (5, 4), "dn", None),
    "L12-55-65-walk": (12, (5, 5), (6, 5), "up", 6),
    "L16-21-31": (16, (2, 1), (3, 1), "up", None),
    "L34-21-31": (34, (2, 1), (3, 1), "up", None),
    "L40-11-21": (40, (1, 1), (2, 1), "up", None),
    "L40-21-11": (40, (2, 1), (1, 1), "up", None),
    "L40-12-11": (40, (1, 2), (1, 1), "dn", None),
    "L7-34-up0": (7, (3, 4), (3, 4), "up", None),
    "L7-34-dn0": (7, (3, 4), (3, 4), "dn", None),
    "L16-21-up0": (16, (2, 1), (2, 1), "up", None),
    "L16-21-dn0": (16, (2, 1), (2, 1), "dn", None),
    "L40-12-up0": (40, (1, 2), (1, 2), "up", None),
    "L40-12-dn0": (40, (1, 2), (1, 2), "dn", None),
}
WEIGHTS = ["random", "ones", "top"]


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


def to_dev(a):
    return torch.from_numpy(np.array(a)).to(dev())      # (a copy: the cached case arrays are read-only)


def site_weights(L, kind):
    if kind == "ones":
        return np.ones(L)
    if kind == "top":
        return np.eye(L)[L - 1]
    return normal_vector(L, 9600 + L)


def step_of(name):
    _, (a, b), (c, d), _, _ = GEOMETRY[name]
    return (c - a) + (d - b)


def ref_args(name):
    L, (a, b), _, species, _ = GEOMETRY[name]
    return L, a, b, SPECIES[species], step_of(name)


@functools.lru_cache(maxsize=None)
def sector(L, nup, ndn):
    """one table set per sector for the whole module (zero couplings on a ring: only the tables are used)"""
    bonds = ring_bonds(L) if L > 2 else [(0, 1)]
    return HubbardOperator(L, bonds, torch.zeros(2 * len(bonds) + 2 * L, dtype=F64, device=dev()), nup, ndn)


def ladder(name):
    L, src, dst, species, grid = GEOMETRY[name]
    lad = HubbardLadder(sector(L, *src), sector(L, *dst), species)
    if grid is not None:
        lad.set_grid_log2(grid)
    return lad


@functools.lru_cache(maxsize=None)
def case(name, kind):
    """(w, x, S(w) x) on the host, computed once per case and never written to"""
    args = ref_args(name)
    n_src, _ = ref.sizes(*args)
    w = site_weights(args[0], kind)
    x = normal_vector(n_src, 9700 + args[0] + n_src % 97)
    y = ref.apply(*args, w, x)
    for arr in (w, x, y):
        arr.setflags(write=False)
    return w, x, y


@functools.lru_cache(maxsize=None)
def form_case(name):
    args = ref_args(name)
    n_src, n_dst = ref.sizes(*args)
    v1, v2 = normal_vector(n_dst, 9800 + args[0] + n_dst % 97), normal_vector(n_src, 9900 + args[0] + n_src % 97)
    out = ref.forms(*args, v1, v2)
    for arr in (v1, v2, out):
        arr.setflags(write=False)
    return v1, v2, out


def relnorm(a, b):
    diff, scale = float(np.linalg.norm(np.asarray(a) - np.asarray(b))), float(np.linalg.norm(np.asarray(b)))
    if scale == 0.0:
        return 0.0 if diff == 0.0 else math.inf
    return diff / scale


def test_the_cases_are_what_the_table_says():
    sizes = {name: ref.sizes(*ref_args(name)) for name in GEOMETRY}
    assert [sizes[k] for k in GEOMETRY] == [(4, 4), (4, 4), (9, 9), (9, 9), (100, 100), (100, 100), (1225, 1225), (1225, 1225),
                                            (63504, 52920), (63504, 52920), (627264, 731808), (1920, 8960), (19074, 203456),
                                            (1600, 31200), (31200, 1600), (31200, 1600), (1225, 1225), (1225, 1225), (1920, 1920),
                                            (1920, 1920), (31200, 31200), (31200, 31200)]
    assert [step_of(k) for k in GEOMETRY] == [0, 0, 1, -1, -1, 1, 1, 1, -1, -1, 1, 1, 1, 1, -1, -1, 0, 0, 0, 0, 0, 0]
    # the down stride: 10 -> 10 at L = 5 and 35 -> 35 at L = 7 (several ru in one wave); it changes at L = 10 and L = 40
    assert (math.comb(5, 3), math.comb(5, 2)) == (10, 10) and (math.comb(7, 4), math.comb(7, 3)) == (35, 35)
    assert (math.comb(10, 5), math.comb(10, 4)) == (252, 210) and 252 % 64 and 210 % 64
    assert (math.comb(40, 2), math.comb(40, 1)) == (780, 40)
    assert (7 + 1) // 2 == 4 and 7 - 4 == 3                           # L = 7: sites 0 .. 3 low, 4 .. 6 high
    n = sizes["L12-55-65-walk"][1]
    assert (n + 255) // 256 == 2859 > (1 << GEOMETRY["L12-55-65-walk"][4])      # more row ranges than blocks
    assert (16 + 1) // 2 == 8 and (40 + 1) // 2 == 20                 # one full chunk of 8 per group at L = 16, three at L = 40
    for name in ("L34-21-31", "L40-11-21", "L40-21-11", "L40-12-11", "L40-12-up0", "L40-12-dn0"):
        L, _, (c, d), species, _ = GEOMETRY[name]
        assert max(hub.states(L, c if species == "up" else d)) >= 1 << 32
    # the sector sign of the down species: odd nup at L10, L40 and L7-34, even nup at L5 and L7-43
    assert [GEOMETRY[k][1][0] % 2 for k in ("L5-23-22", "L7-43-44", "L10-55-54", "L40-12-11")] == [0, 0, 1, 1]


@pytest.mark.parametrize("kind", WEIGHTS)
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_apply_against_the_reference(name, kind):
    L, (a, b), _, species, grid = GEOMETRY[name]
    w, x, want = case(name, kind)
    lad = ladder(name)
    assert (lad.L, lad.species, lad.step, lad.n_src, lad.n_dst) == (L, species, step_of(name), x.size, want.size)
    wd, xd = to_dev(w), to_dev(x)
    got = lad(wd, xd)
    assert got.shape == (lad.n_dst,) and got.dtype == F64
    err = relnorm(got.cpu().numpy(), want)
    print("%s %s: |y - ref| / |ref| = %.2e" % (name, kind, err))
    assert err < 1e-13
    # nothing is written past the last row: a longer output filled with a sentinel
    y = torch.full((lad.n_dst + 67,), -7.0, dtype=F64, device=dev())
    states, lo_rank, hi_base = lad._tables
    rc = _lib.load().dsea_hubbard_ladder_apply(L, a, b, SPECIES[species], step_of(name), c_void_p(wd.data_ptr()),
                                               c_void_p(states.data_ptr()), c_void_p(lo_rank.data_ptr()),
                                               c_void_p(hi_base.data_ptr()), c_void_p(xd.data_ptr()), c_void_p(y.data_ptr()),
                                               grid or 0, engine._stream(dev()))
    assert rc == 0
    assert torch.equal(y[:lad.n_dst], got) and bool((y[lad.n_dst:] == -7.0).all())


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_the_transposed_ladder_is_the_transpose(name):
    w, x, _ = case(name, "random")
    lad = ladder(name)
    wd, v2 = to_dev(w), to_dev(x)
    v1 = to_dev(normal_vector(lad.n_dst, 9650 + lad.n_dst % 89))
    Sv2, STv1 = lad(wd, v2), lad.T(wd, v1)
    assert STv1.shape == (lad.n_src,) and lad.T.T is lad
    lhs, rhs = float(v1 @ Sv2), float(STv1 @ v2)
    assert abs(lhs - rhs) <= 1e-13 * float(v1.norm() * Sv2.norm() + STv1.norm() * v2.norm())


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_forms_against_the_reference_sums(name):
    L = GEOMETRY[name][0]
    v1, v2, want = form_case(name)
    lad = ladder(name)
    d1, d2 = to_dev(v1), to_dev(v2)
    got = lad.forms(d1, d2)
    assert got.shape == (L,)
    norms = np.linalg.norm(v1) * np.linalg.norm(v2)
    bound = 1e-13 * norms
    err = float(np.max(np.abs(got.cpu().numpy() - want)))
    print("%s: max |form - ref| = %.2e (bound %.2e)" % (name, err, bound))
    assert err <= bound
    again = lad.forms(d1, d2)
    assert torch.equal(got, again)                       # fixed-order reductions, no atomics
    # S is linear in the weights: v1^T S(w) v2 = sum_i w_i form_i.  Each form is within 1e-13 |v1| |v2| of its sum and the map
    # within 1e-13 |S v2| of its value (the two bounds above), so the two sides differ by at most
    # 1e-13 (|v1| |v2| sum_i |w_i| + |v1| |S v2|)
    w = site_weights(L, "random")
    Sv2 = lad(to_dev(w), d2)
    lhs, rhs = float(d1 @ Sv2), float(np.sum(w * got.cpu().numpy()))
    assert abs(lhs - rhs) <= 1e-13 * (norms * np.abs(w).sum() + np.linalg.norm(v1) * float(Sv2.norm()))


@pytest.mark.parametrize("dst,species", [((2, 3), "up"), ((3, 2), "dn")])
def test_autograd_against_a_dense_twin(dst, species):
    L = 6
    lad = HubbardLadder(sector(L, 3, 3), sector(L, *dst))
    assert (lad.species, lad.step) == (species, -1)
    S = torch.stack([lad.dense(torch.eye(L, dtype=F64, device=dev())[i]) for i in range(L)])       # [L, n_dst, n_src]
    assert S.shape == (L, 300, 400)
    want = np.stack([ref.dense(L, 3, 3, SPECIES[species], -1, np.eye(L)[i]) for i in range(L)])
    assert torch.equal(S, torch.from_numpy(want).to(dev()))
    w0, x0 = to_dev(site_weights(L, "random")), to_dev(normal_vector(400, 9670))
    v = to_dev(normal_vector(L, 9671))

    def grads(apply):
        w, x = w0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
        y = apply(w, x)
        loss = (y * y).sum()
        gw, gx = torch.autograd.grad(loss, (w, x), create_graph=True)
        (hv,) = torch.autograd.grad((gw * v).sum(), w)
        return loss.detach(), gw.detach(), gx.detach(), hv

    native = grads(lad)
    twin = grads(lambda w, x: torch.einsum("i,iab,b->a", w, S, x))
    for what, a, b in zip(("loss", "d/dw", "d/dx", "Hessian-vector product in w"), native, twin):
        err = float((a - b).norm() / b.norm())
        print("%s %s: relative deviation from the dense twin %.2e" % (species, what, err))
        assert err <= TOL


def hubbard_ring_couplings(L, U, eps=None):
    nb = L
    return np.concatenate([np.ones(nb), np.zeros(nb), U * np.ones(L), np.zeros(L) if eps is None else eps])


def test_the_gradient_of_the_momentum_distribution_through_the_eigensolver(monkeypatch):
    """d n_k / dU at U = 4 on the ring L = 6, (3, 3), k = 2 pi 2 / 6 (empty at U = 0), n_k = |c_{k up} psi0|^2 with psi0 from
    DominantSparseSymeig, against the five-point central difference of the dense reference with step h = 1e-3:
        (f(-2h) - 8 f(-h) + 8 f(h) - f(2h)) / (12 h),  truncation h^4 |f^(5)| / 30 (1e-12 / 30 per unit of f^(5)),
        rounding 1.5 delta / h with delta the error of one dense n_k (eigenvector of eigh: eps |H| / gap ~ 1e-14, taken as 1e-12)
    so the difference itself is good to 1.5e-9; the adjoint CG stops at 1e-12.  Tolerance 5e-9 absolute (n_k is of order one)."""
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, m, h = 6, 2, 1e-3
    bonds = ring_bonds(L)
    parts = [t.numpy() for t in ring_momentum_weights(L, m)]

    def dense_nk(U):
        E, V = np.linalg.eigh(hub.dense(L, 3, 3, bonds, hubbard_ring_couplings(L, U)))
        assert E[1] - E[0] > 0.1
        return sum(float(np.sum(ref.apply(L, 3, 3, ref.UP, -1, w, V[:, 0]) ** 2)) for w in parts)

    want = (dense_nk(4 - 2 * h) - 8 * dense_nk(4 - h) + 8 * dense_nk(4 + h) - dense_nk(4 + 2 * h)) / (12 * h)
    U = torch.tensor(4.0, dtype=F64, device=dev(), requires_grad=True)
    p0, dU = to_dev(hubbard_ring_couplings(L, 0.0)), to_dev(hubbard_ring_couplings(L, 1.0) - hubbard_ring_couplings(L, 0.0))
    op = HubbardOperator(L, bonds, p0 + U * dU, 3, 3)
    lad = op.ladder(sector(L, 2, 3))
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(9680):
        _, psi0 = symeig.DominantSparseSymeig.apply(op.couplings, 200, 400)
        n_k = sum((lad(to_dev(w), psi0) ** 2).sum() for w in parts)
        (got,) = torch.autograd.grad(n_k, U)
    value_err = abs(n_k.item() - dense_nk(4.0))
    err = abs(got.item() - want)
    print("n_k = %.12f (|dev| %.2e)   d n_k / dU = %.10f against the central difference %.10f: |dev| = %.2e (bound 5e-9)"
          % (n_k.item(), value_err, got.item(), want, err))
    assert value_err <= TOL and abs(want) > 1e-3
    assert err <= 5e-9


def test_c_abi_argument_errors():
    """every DSEA_ERR_ARG case returns the error from host arithmetic: nothing is launched, the outputs keep their sentinel"""
    lib = _lib.load()
    L = 6
    lad = HubbardLadder(sector(L, 3, 3), sector(L, 2, 3))
    states, lo_rank, hi_base = (c_void_p(t.data_ptr()) for t in lad._tables)
    w = to_dev(site_weights(L, "random"))
    x = to_dev(normal_vector(400, 9680))
    y = torch.full((400,), -7.0, dtype=F64, device=dev())         # (400: long enough for step 0 and +1 as well)
    out = torch.full((L,), -7.0, dtype=F64, device=dev())
    scratch = torch.full((2 * L,), -7.0, dtype=F64, device=dev())
    st = engine._stream(dev())
    P = lambda t: c_void_p(t.data_ptr())                        # noqa: E731
    null = c_void_p(None)
    good = dict(L=L, nup=3, ndn=3, species=0, step=-1, w=P(w), states=states, lo=lo_rank, hi=hi_base, x=P(x), y=P(y), grid=0)

    def apply(**kw):
        a = dict(good, **kw)
        return lib.dsea_hubbard_ladder_apply(a["L"], a["nup"], a["ndn"], a["species"], a["step"], a["w"], a["states"], a["lo"],
                                             a["hi"], a["x"], a["y"], a["grid"], st)

    goodf = dict(L=L, nup=3, ndn=3, species=0, step=-1, states=states, lo=lo_rank, hi=hi_base, v1=P(y), v2=P(x), out=P(out),
                 scratch=P(scratch), grid=0)

    def forms(**kw):
        a = dict(goodf, **kw)
        return lib.dsea_hubbard_ladder_forms(a["L"], a["nup"], a["ndn"], a["species"], a["step"], a["states"], a["lo"], a["hi"],
                                             a["v1"], a["v2"], a["out"], a["scratch"], a["grid"], st)

    shared = [dict(species=2), dict(species=-1), dict(step=2), dict(step=-2),
              dict(nup=5, step=1), dict(nup=1, step=-1), dict(ndn=5, species=1, step=1), dict(ndn=1, species=1, step=-1),
              dict(nup=0, step=1), dict(nup=6, step=-1), dict(ndn=0), dict(ndn=6),
              dict(L=41, nup=1, ndn=1, step=1), dict(L=1, nup=1, ndn=1, step=0), dict(L=18, nup=9, ndn=8, species=1, step=1),
              dict(grid=5), dict(grid=13), dict(grid=-1), dict(grid=1), dict(states=null), dict(lo=null), dict(hi=null)]
    for bad in shared + [dict(w=null), dict(x=null), dict(y=null), dict(y=P(x)), dict(step=1, nup=2, y=P(x))]:
        assert apply(**bad) == _lib.ERR_ARG, bad
    for bad in shared + [dict(v1=null), dict(v2=null), dict(out=null), dict(scratch=null)]:
        assert forms(**bad) == _lib.ERR_ARG, bad
    need = c_int64(-1)
    for bad in ((L, 3, 3, 2, 1), (L, 3, 3, 0, 2), (L, 5, 3, 0, 1), (L, 3, 1, 1, -1), (41, 1, 1, 0, 1), (18, 9, 8, 1, 1)):
        assert lib.dsea_hubbard_ladder_forms_scratch_doubles(*bad, byref(need)) == _lib.ERR_ARG and need.value == -1
    assert lib.dsea_hubbard_ladder_forms_scratch_doubles(L, 3, 3, 0, -1, None) == _lib.ERR_ARG
    torch.cuda.synchronize()
    for t in (y, out, scratch):
        assert bool((t == -7.0).all())
    # x == y is allowed for step 0 (a diagonal map)
    same = ladder("L7-34-dn0")
    wz, xz, want = case("L7-34-dn0", "random")
    buf = to_dev(xz)
    tabs = [c_void_p(t.data_ptr()) for t in same._tables]
    assert lib.dsea_hubbard_ladder_apply(7, 3, 4, 1, 0, P(to_dev(wz)), tabs[0], tabs[1], tabs[2], P(buf), P(buf), 0, st) == 0
    assert relnorm(buf.cpu().numpy(), want) < 1e-13


# ---------------------------------------------------------------------------------------------- the measure and the physics
@functools.lru_cache(maxsize=None)
def lehmann_case():
    """L = 6, (3, 3): a ring plus random bonds with t = 1, V = 0.3, U = 4 and random eps (no symmetry); the ground state of the
    source from dense eigh, on the host"""
    L = 6
    bonds = tuple(ring_bonds(L) + lattice_reference.random_bonds(L, 3, 9690))
    nb = len(bonds)
    p = np.concatenate([np.ones(nb), 0.3 * np.ones(nb), 4.0 * np.ones(L), normal_vector(L, 9691)])
    E, V = np.linalg.eigh(hub.dense(L, 3, 3, bonds, p))
    assert E[1] - E[0] > 1e-3
    return L, bonds, p, E[0], V[:, 0].copy()


CHANNELS = {"c_up": ((2, 3), ref.UP, -1), "c_dn": ((3, 2), ref.DN, -1), "cdag_up": ((4, 3), ref.UP, 1),
            "cdag_dn": ((3, 4), ref.DN, 1), "n": ((3, 3), None, 0), "sz": ((3, 3), None, 0)}


@pytest.mark.parametrize("channel", list(CHANNELS))
def test_the_spectral_function_against_the_dense_lehmann_sum(channel):
    """k = n: G(omega + i eta) at eta = 0.5 on 64 points across the spectrum against sum_n |<n|O|0>|^2 / (z - (E_n - E_0)) from
    dense eigh of the destination sector and the numpy reference of O, for complex site weights (the two real parts add)"""
    L, bonds, p, E0, psi0 = lehmann_case()
    (nu, nd), species, step = CHANNELS[channel]
    En, Vn = np.linalg.eigh(hub.dense(L, nu, nd, bonds, p))
    parts = [t.numpy() for t in ring_momentum_weights(L, 1)]
    z = torch.complex(torch.linspace(float(En[0] - E0), float(En[-1] - E0), 64, dtype=F64), torch.full((64,), 0.5, dtype=F64))
    dense = np.zeros(64, dtype=np.complex128)
    for w in parts:
        if step:
            phi = ref.apply(L, 3, 3, species, step, w, psi0)
        else:
            sign = 1.0 if channel == "n" else -1.0
            phi = ref.apply(L, 3, 3, ref.UP, 0, w, psi0) + sign * ref.apply(L, 3, 3, ref.DN, 0, w, psi0)
        amp = Vn.T @ phi
        dense += np.sum(amp ** 2 / (z.numpy()[:, None] - (En - E0)[None, :]), axis=1)
    dense = torch.from_numpy(dense)
    op0 = HubbardOperator(L, bonds, to_dev(p), 3, 3)
    m = hubbard_spectral_function(op0, to_dev(psi0), E0, tuple(torch.from_numpy(w) for w in parts), channel, k=len(En))
    assert isinstance(m, SpectralMeasure) and 1 <= m.steps <= 2 * len(En)
    err = float((m.greens(z) - dense).abs().max() / dense.abs().max())
    print("%s, k = n = %d (steps = %d): max |G - G_dense| / max |G_dense| = %.2e" % (channel, len(En), m.steps, err))
    assert err <= TOL
    if channel == "c_up":
        target = HubbardOperator(L, bonds, to_dev(p), nu, nd)
        again = hubbard_spectral_function(op0, to_dev(psi0), E0, torch.complex(*(torch.from_numpy(w) for w in parts)), channel,
                                          k=len(En), target=target)
        assert float((again.greens(z) - m.greens(z)).abs().max()) <= TOL * float(dense.abs().max())
        with pytest.raises(ValueError):
            hubbard_spectral_function(op0, to_dev(psi0), E0, parts[0], "cdag_up", target=target)   # a target in the wrong sector
        with pytest.raises(ValueError):
            hubbard_spectral_function(op0, to_dev(psi0), E0, parts[0], "c")


def slater_ground_state(L, N):
    """the ground state of the free ring with N particles of each species (a closed shell) in the row order of the operator:
    the amplitude of |u, d> is det(Phi[sites of u]) det(Phi[sites of d]) with Phi the N lowest orbitals"""
    hop = np.zeros((L, L))
    for a, b in ring_bonds(L):
        hop[a, b] = hop[b, a] = -1.0
    e, phi = np.linalg.eigh(hop)
    assert e[N] - e[N - 1] > 0.5                                   # closed shell
    amp = np.array([np.linalg.det(phi[[i for i in range(L) if (s >> i) & 1], :N]) for s in hub.states(L, N)])
    return 2.0 * float(e[:N].sum()), np.outer(amp, amp).reshape(-1)


def test_free_fermions_every_removal_measure_is_one_pole():
    """Ring L = 10, (5, 5), U = 0: c_{k up} psi0 is an eigenvector of the (4, 5) Hamiltonian at E0 - eps_k, so the removal
    measure is one pole at the excitation energy -eps_k carrying n_k = 1 for an occupied k; an empty k carries nothing (the
    Slater determinant is built in floating point, so "nothing" is rounding: below 1e-24)"""
    L, N = 10, 5
    E0, psi0 = slater_ground_state(L, N)
    assert abs(np.linalg.norm(psi0) - 1.0) < 1e-12
    op0 = HubbardOperator(L, ring_bonds(L), to_dev(hubbard_ring_couplings(L, 0.0)), N, N)
    target = HubbardOperator(L, ring_bonds(L), to_dev(hubbard_ring_couplings(L, 0.0)), N - 1, N)
    psi = to_dev(psi0)
    assert float((op0.H(psi) - E0 * psi).norm()) <= 1e-12
    total = 0.0
    for m in range(L):
        eps = -2.0 * math.cos(2.0 * math.pi * m / L)
        meas = hubbard_spectral_function(op0, psi, E0, ring_momentum_weights(L, m), "c_up", k=12, target=target)
        n_k = meas.moment(0)
        total += n_k
        if eps < 0.0:
            heavy = meas.weights > 1e-10
            assert abs(n_k - 1.0) <= TOL and abs(float(meas.weights[heavy].sum()) - 1.0) <= TOL
            assert float((meas.poles[heavy] + eps).abs().max()) <= TOL
        else:
            assert n_k <= 1e-24
        print("m = %d: eps_k = %+.6f  n_k = %.3e  poles %d" % (m, eps, n_k, len(meas)))
    assert abs(total - N) <= TOL


@functools.lru_cache(maxsize=None)
def interacting_ring():
    """ring L = 8, (4, 4), U = 4: (op, psi0, E0) from DominantSparseSymeig, the four neighbouring sectors' Hamiltonians"""
    L = 8
    p = to_dev(hubbard_ring_couplings(L, 4.0))
    op = HubbardOperator(L, ring_bonds(L), p, 4, 4)
    orig = CG.EPS_DEFAULT
    try:
        CG.EPS_DEFAULT = 1e-12
        symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
        torch.manual_seed(0)
        E0, psi0 = symeig.DominantSparseSymeig.apply(op.couplings, 200, op.dim, op.device)
    finally:
        CG.EPS_DEFAULT = orig
    psi0 = psi0.detach()
    res = float((op.H(psi0) - E0 * psi0).norm())
    print("interacting ring L = 8, (4, 4), U = 4: E0 = %.12f, |H psi0 - E0 psi0| = %.2e" % (float(E0), res))
    assert res <= 1e-8
    targets = {key: HubbardOperator(L, ring_bonds(L), p, *sec)
               for key, sec in (("c_up", (3, 4)), ("cdag_up", (5, 4)), ("c_dn", (4, 3)), ("cdag_dn", (4, 5)))}
    return op, psi0, float(E0), targets


@pytest.mark.parametrize("species", ["up", "dn"])
def test_the_sum_rules_of_the_interacting_ring(species):
    """per k: |c_k psi0|^2 + |c+_k psi0|^2 = <{c_k, c+_k}> = 1 (the zeroth moments of the two measures); sum_k n_k = N_s; and
    n(k) is the Fourier transform of the one-body density matrix"""
    op, psi0, E0, targets = interacting_ring()
    L = op.N
    rho = one_body_density_matrix(op, psi0, species, target=targets["c_" + species]).cpu()
    assert float((rho - rho.T).abs().max()) <= 1e-14 and abs(float(rho.trace()) - 4.0) <= TOL
    auto = one_body_density_matrix(op, psi0, species).cpu()           # target=None builds the tables itself
    assert float((auto - rho).abs().max()) <= 1e-14
    total = worst = 0.0
    for m in range(L):
        parts = ring_momentum_weights(L, m)
        c = hubbard_spectral_function(op, psi0, E0, parts, "c_" + species, k=8, target=targets["c_" + species])
        cdag = hubbard_spectral_function(op, psi0, E0, parts, "cdag_" + species, k=8, target=targets["cdag_" + species])
        A = cdag + c.reflected()
        worst = max(worst, abs(A.moment(0) - 1.0))
        assert abs(A.moment(0) - 1.0) <= TOL, (m, A.moment(0))
        n_k = c.moment(0)
        assert abs(n_k - sum(float(w @ rho @ w) for w in parts)) <= TOL
        assert 0.0 < n_k < 1.0
        total += n_k
    print("%s: worst |m0(c) + m0(c+) - 1| = %.2e   sum_k n_k - 4 = %.2e" % (species, worst, total - 4.0))
    assert abs(total - 4.0) <= TOL


def test_the_f_sum_rule_of_the_charge_channel():
    """the first moment of the "n" (and "sz") measure is -(1/2) sum_t t_t (w_a - w_b)^2 <dH/dt_t>, the prefactor that
    tests/test_hubbard_ladder_cpu.py::test_the_f_sum_rule_prefactor_against_dense_eigh checks against dense eigh, with the
    t forms of ``Hadjoint_to_couplingsadjoint``"""
    op, psi0, E0, _ = interacting_ring()
    L, bonds = op.N, op.bonds
    t_forms = op.Hadjoint_to_couplingsadjoint(psi0, psi0)[:len(bonds)].cpu().numpy()
    worst = 0.0
    for channel in ("n", "sz"):
        for m in range(1, L):
            parts = ring_momentum_weights(L, m)
            meas = hubbard_spectral_function(op, psi0, E0, parts, channel, k=40)
            want = sum(-0.5 * sum((float(w[a]) - float(w[b])) ** 2 * t_forms[k] for k, (a, b) in enumerate(bonds)) for w in parts)
            scale = float((meas.weights * meas.poles.abs()).sum())
            dev_m = abs(meas.moment(1) - want) / scale
            worst = max(worst, dev_m)
            assert dev_m <= TOL, (channel, m, dev_m)
            assert float(meas.poles[meas.weights > 1e-12 * meas.norm2].min()) > -1e-8        # excitation energies
    print("worst f-sum deviation = %.2e" % worst)


def test_example_spectral():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "hubbard", "spectral.py")
    spec = importlib.util.spec_from_file_location("hubbard_spectral", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    orig = CG.EPS_DEFAULT
    try:
        out = ex.main(L=8)
    finally:
        CG.EPS_DEFAULT = orig
    assert out["L"] == 8 and out["n"] == 4900 and len(out["k"]) == 8
    for key in ("n_k", "n_k_rho", "sum_rule", "removal_edge", "addition_edge"):
        assert len(out[key]) == 8 and all(math.isfinite(v) for v in out[key]), key
    for n_k, n_rho, total in zip(out["n_k"], out["n_k_rho"], out["sum_rule"]):
        assert abs(n_k - n_rho) <= 1e-8 and abs(total - 1.0) <= 1e-8
    assert abs(sum(out["n_k"]) - 4.0) <= 1e-8 and out["charge_gap"] > 0.0
    assert np.isfinite(out["A"]).all() and (np.asarray(out["A"]) >= 0.0).all()
