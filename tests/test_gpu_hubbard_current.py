"""The bond current map of a Hubbard sector on the GPU (docs/design/39-hubbard-current.md): k_hubbard_current<R> and
k_hubbard_current_forms against the numpy twin of tests/hubbard_current_reference.py at the shapes of tests/test_gpu_hubbard.py
(the table is copied, not imported), the block form column by column, antisymmetry, the autograd pair against the twin's dense
matrices, and ``optical_conductivity`` end to end against dense ``eigh``.

    L, nup, ndn             n_up x n_dn = n          bonds                           what it reaches
    2,1,1                   2 x 2 = 4                (0,1) (0,1) (1,0)               less than a wave; repeated and reversed bond
    5,2,3                   10 x 10 = 100            random + one reversed, 7        n_dn < 64: many ru in one wave; nup != ndn;
                                                                                     chunks of 4 and of 2 end ragged
    5,2,3 five              100                      the first 5 of them             a ragged second chunk of 4, third chunk of 2
    6,3,3                   20 x 20 = 400            the ten bonds of the loop       two blocks, ragged last block; shared tables
                                                     lattice
    7,3,2                   35 x 21 = 735            (0,6) (5,6) (2,3) (1,4)         odd L (Llo = 4, Lhi = 3); sign masks inside
                                                                                     lo, inside hi, across
    7,3,2 one               735                      (6,0)                           one bond: a single ragged chunk at every R
    8,4,4                   70 x 70 = 4 900          complete graph, 28              n_dn = 70: waves straddle an ru boundary
    9,3,5                   84 x 126 = 10 584        complete graph cycled to 128    full bond table; two different table sets
    10,5,5, grid cap 2^6    252 x 252 = 63 504       24 random                       249 row ranges on 64 blocks: blocks walk
    40,2,1                  780 x 40 = 31 200        ring + 10 random                words and sign masks wider than 32 bits; the
                                                                                     bond (39, 0) spans bits 1 .. 38
"""
import functools
import importlib.util
import math
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hubbard_current_reference as cref  # noqa: E402
import hubbard_reference as href  # noqa: E402
import lattice_reference  # noqa: E402
from helpers import PatchRandn  # noqa: E402
from dominantsparseeigenad_amd import _lib  # noqa: E402
from dominantsparseeigenad_amd.operators import HubbardCurrent, HubbardOperator, hubbard_dim, ring_bonds  # noqa: E402
from dominantsparseeigenad_amd.spectral import OpticalResponse, optical_conductivity  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402
import dominantsparseeigenad_amd.symeig as symeig  # noqa: E402
import dominantsparseeigenad_amd.CG as CG  # noqa: E402

F64 = torch.float64
CAP = _lib.LATTICE_MAX_BONDS
LOOP_BONDS = ((0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (0, 3), (1, 4), (2, 5), (0, 2))


def small_bonds(L):
    """random pairs with one of them listed again reversed; at L = 2 that is (0, 1) more than once"""
    bonds = lattice_reference.random_bonds(L, L + 1, 7500 + L)
    a, b = bonds[0]
    return tuple(bonds + [(b, a)]) if L > 2 else ((0, 1), (0, 1), (1, 0))


def cyclic_complete(L, count):
    full = lattice_reference.complete_bonds(L)
    return tuple(full[i % len(full)] for i in range(count))


def ring_and_random(L):
    return tuple(ring_bonds(L) + lattice_reference.random_bonds(L, 10, 7600 + L))


# name -> (L, nup, ndn, log2 of the grid cap or None for the default, bonds)
GEOMETRY = {
    "L2-1-1": (2, 1, 1, None, small_bonds(2)),
    "L5-2-3": (5, 2, 3, None, small_bonds(5)),
    "L5-2-3-five": (5, 2, 3, None, small_bonds(5)[:5]),
    "L6-3-3-loops": (6, 3, 3, None, LOOP_BONDS),
    "L7-3-2-split": (7, 3, 2, None, ((0, 6), (5, 6), (2, 3), (1, 4))),
    "L7-3-2-one": (7, 3, 2, None, ((6, 0),)),
    "L8-4-4-complete": (8, 4, 4, None, tuple(lattice_reference.complete_bonds(8))),
    "L9-3-5-cap": (9, 3, 5, None, cyclic_complete(9, CAP)),
    "L10-5-5-walk": (10, 5, 5, 6, tuple(lattice_reference.random_bonds(10, 24, 7510))),
    "L40-2-1": (40, 2, 1, None, ring_and_random(40)),
}
LARGER = ["L8-4-4-complete", "L9-3-5-cap", "L10-5-5-walk", "L40-2-1"]
WIDTHS = (1, 2, 3, 4, 8, 11)


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


def to_dev(a):
    return torch.from_numpy(np.array(a)).to(dev())      # (a copy: the cached case arrays are read-only)


def operator(name):
    """the operator of a case: the current map reads its sector, tables, bonds and grid cap, not its couplings"""
    L, nup, ndn, grid, bonds = GEOMETRY[name]
    op = HubbardOperator(L, bonds, torch.zeros(2 * len(bonds) + 2 * L, dtype=F64, device=dev()), nup, ndn)
    if grid is not None:
        op.set_grid_log2(grid)
    return op


@functools.lru_cache(maxsize=None)
def case(name):
    """(w, x, K(w) x) on the host, computed once per case and never written to"""
    L, nup, ndn, _, bonds = GEOMETRY[name]
    nb = len(bonds)
    w = normal_vector(2 * nb, 3000 + L + nb).reshape(2, nb).copy()
    x = normal_vector(hubbard_dim(L, nup, ndn), 3100 + L + nup)
    y = cref.apply(L, nup, ndn, bonds, w, x)
    for a in (w, x, y):
        a.setflags(write=False)
    return w, x, y


@functools.lru_cache(maxsize=None)
def form_case(name):
    L, nup, ndn, _, bonds = GEOMETRY[name]
    n = hubbard_dim(L, nup, ndn)
    v1, v2 = normal_vector(n, 3200 + L + nup), normal_vector(n, 3300 + L + nup)
    out = cref.forms(L, nup, ndn, bonds, v1, v2)
    for a in (v1, v2, out):
        a.setflags(write=False)
    return v1, v2, out


def relnorm(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def test_the_cases_are_what_the_table_says():
    sizes = {name: hubbard_dim(*g[:3]) for name, g in GEOMETRY.items()}
    assert [sizes[k] for k in GEOMETRY] == [4, 100, 100, 400, 735, 735, 4900, 10584, 63504, 31200]
    counts = [len(g[4]) for g in GEOMETRY.values()]
    assert counts == [3, 7, 5, 10, 4, 1, 28, CAP, 24, 50]
    assert {1, 5, 7} <= set(counts)                      # a chunk of 4 and a chunk of 2 both end ragged
    assert GEOMETRY["L2-1-1"][4] == ((0, 1), (0, 1), (1, 0))
    assert any((b, a) in GEOMETRY["L5-2-3"][4] for a, b in GEOMETRY["L5-2-3"][4])
    assert math.comb(5, 3) < 64 and (sizes["L6-3-3-loops"] + 255) // 256 == 2 and sizes["L6-3-3-loops"] % 256 != 0
    assert [href.between(a, b) for a, b in GEOMETRY["L7-3-2-split"][4]] == [0b0111110, 0, 0, 0b0001100]
    assert math.comb(8, 4) % 64 != 0 and len(set(GEOMETRY["L9-3-5-cap"][4])) == 36
    assert (sizes["L10-5-5-walk"] + 255) // 256 == 249 > (1 << GEOMETRY["L10-5-5-walk"][3]) == 64
    assert (39, 0) in GEOMETRY["L40-2-1"][4] and max(href.states(40, 2)) >= 1 << 32 and href.between(39, 0) == (1 << 39) - 2


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_apply_against_the_twin(name):
    L, nup, ndn, _, bonds = GEOMETRY[name]
    w, x, want = case(name)
    cur = operator(name).current()
    assert isinstance(cur, HubbardCurrent) and cur.nb == len(bonds) and cur.n == x.size
    xd = to_dev(x)
    err = relnorm(cur(to_dev(w), xd).cpu().numpy(), want)
    print("%s: |K x - twin| / |twin| = %.2e (bound 1e-13)" % (name, err))
    assert err < 1e-13
    # one species' weights all zero: the other species alone
    for s in (0, 1):
        ws = np.array(w)
        ws[s] = 0.0
        assert relnorm(cur(to_dev(ws), xd).cpu().numpy(), cref.apply(L, nup, ndn, bonds, ws, x)) < 1e-13
    # a (nb,) vector is used for both species
    both = cur(to_dev(w[0]), xd)
    assert torch.equal(both, cur(to_dev(np.stack([w[0], w[0]])), xd))
    assert relnorm(both.cpu().numpy(), cref.apply(L, nup, ndn, bonds, w[0], x)) < 1e-13


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_apply_block_columns_are_the_single_vector_call(name):
    w, x, _ = case(name)
    cur = operator(name).current()
    n = x.size
    wd = to_dev(w)
    X = torch.from_numpy(normal_vector(n * max(WIDTHS), 3400 + n % 89).reshape(n, max(WIDTHS)).copy()).to(dev())
    single = [cur(wd, X[:, j].contiguous()) for j in range(max(WIDTHS))]
    for R in WIDTHS:
        Y = cur.apply_block(wd, X[:, :R])
        assert Y.shape == (n, R) and not Y.requires_grad
        for j in range(R):
            assert torch.equal(Y[:, j], single[j]), (name, R, j)
        assert torch.equal(cur.apply_block(wd, X[:, :R]), Y)


def test_dense_is_antisymmetric_bit_for_bit_and_is_the_twin():
    name = "L6-3-3-loops"
    L, nup, ndn, _, bonds = GEOMETRY[name]
    w = case(name)[0]
    K = operator(name).current().dense(to_dev(w))
    assert K.shape == (400, 400)
    assert torch.equal(K, -K.T)
    want = cref.dense(L, nup, ndn, bonds, w)
    assert float(np.max(np.abs(K.cpu().numpy() - want))) <= 1e-14 * float(np.max(np.abs(want)))


@pytest.mark.parametrize("name", LARGER)
def test_the_map_is_antisymmetric(name):
    w, x, _ = case(name)
    cur = operator(name).current()
    wd, a = to_dev(w), to_dev(x)
    b = torch.from_numpy(normal_vector(x.size, 3500 + x.size % 97)).to(dev())
    Ka, Kb = cur(wd, a), cur(wd, b)
    assert abs(float(a @ Kb) + float(b @ Ka)) <= 1e-13 * float(a.norm() * Kb.norm() + b.norm() * Ka.norm())


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_forms_against_the_twin(name):
    L, nup, ndn, _, bonds = GEOMETRY[name]
    v1, v2, want = form_case(name)
    cur = operator(name).current()
    a, b = to_dev(v1), to_dev(v2)
    got = cur.forms(a, b)
    assert got.shape == (2, len(bonds))
    bound = 1e-13 * np.linalg.norm(v1) * np.linalg.norm(v2)
    err = float(np.max(np.abs(got.cpu().numpy() - want)))
    print("%s: max |form - twin| = %.2e (bound %.2e)" % (name, err, bound))
    assert err <= bound
    assert torch.equal(cur.forms(a, b), got)             # fixed-order reductions, no atomics
    assert float(cur.forms(a, a).abs().max()) <= 1e-13 * np.linalg.norm(v1) ** 2      # v^T K v = 0
    # K is linear in the weights: v1^T K(w) v2 = sum w form, within the two bounds above
    w = case(name)[0]
    Kv2 = cur(to_dev(w), b)
    lhs, rhs = float(a @ Kv2), float(np.sum(w * got.cpu().numpy()))
    assert abs(lhs - rhs) <= 1e-13 * (np.linalg.norm(v1) * np.linalg.norm(v2) * np.abs(w).sum()
                                      + np.linalg.norm(v1) * float(Kv2.norm()))


# ---- autograd at L = 6 (3, 3), analytic from the twin's dense matrices ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def unit_matrices():
    """the 2 nb matrices K_{s t} of the loop lattice as one (2, nb, n, n) host array"""
    L, nup, ndn, _, bonds = GEOMETRY["L6-3-3-loops"]
    nb = len(bonds)
    out = np.zeros((2, nb, 400, 400))
    for s in range(2):
        for t in range(nb):
            e = np.zeros((2, nb))
            e[s, t] = 1.0
            out[s, t] = cref.dense(L, nup, ndn, bonds, e)
    out.setflags(write=False)
    return out


def test_gradients_of_the_squared_norm():
    name = "L6-3-3-loops"
    w, x, _ = case(name)
    Kst = unit_matrices()
    K = np.einsum("st,stij->ij", w, Kst)
    y = K @ x
    units = np.einsum("stij,j->sti", Kst, x)             # K_{s t} x
    gw_ref = 2.0 * units @ y                             # d |K x|^2 / d w_{s t} = 2 (K_{s t} x) . (K x)
    gx_ref = 2.0 * K.T @ y
    v = normal_vector(w.size, 3600).reshape(w.shape)
    hv_ref = 2.0 * units @ (np.einsum("st,sti->i", v, units))        # the Hessian in w is 2 (K_{s t} x) . (K_{s' t'} x)
    cur = operator(name).current()
    wd = to_dev(w).requires_grad_(True)
    xd = to_dev(x).requires_grad_(True)
    out = cur(wd, xd)
    f = out @ out
    gw, gx = torch.autograd.grad(f, (wd, xd), create_graph=True)
    (hv,) = torch.autograd.grad((gw * to_dev(v)).sum(), wd)
    ew = float(np.max(np.abs(gw.detach().cpu().numpy() - gw_ref)) / np.max(np.abs(gw_ref)))
    ex = float(np.max(np.abs(gx.detach().cpu().numpy() - gx_ref)) / np.max(np.abs(gx_ref)))
    eh = float(np.max(np.abs(hv.cpu().numpy() - hv_ref)) / np.max(np.abs(hv_ref)))
    print("d|Kx|^2/dw max err / max = %.2e   d/dx %.2e (bounds 1e-10)   Hessian-vector product in w %.2e (bound 1e-8)"
          % (ew, ex, eh))
    assert gw.shape == (2, 10) and gx.shape == (400,) and hv.shape == (2, 10)
    assert ew < 1e-10 and ex < 1e-10
    assert eh < 1e-8
    # the forms are differentiable too: d (G . forms(v1, v2)) / d v1 = K(G) v2, d / d v2 = -K(G) v1
    v1 = to_dev(form_case(name)[0]).requires_grad_(True)
    v2 = to_dev(form_case(name)[1]).requires_grad_(True)
    g1, g2 = torch.autograd.grad((cur.forms(v1, v2) * to_dev(v)).sum(), (v1, v2))
    KG = np.einsum("st,stij->ij", v, Kst)
    assert relnorm(g1.cpu().numpy(), KG @ form_case(name)[1]) < 1e-13
    assert relnorm(g2.cpu().numpy(), -KG @ form_case(name)[0]) < 1e-13
    # a (nb,) vector of weights keeps its graph: the gradient is the sum over the species
    w1 = to_dev(w[0]).requires_grad_(True)
    out = cur(w1, to_dev(x))
    (g,) = torch.autograd.grad(out @ out, w1)
    K1 = np.einsum("t,stij->ij", w[0], Kst)
    want = 2.0 * (units @ (K1 @ x)).sum(axis=0)
    assert g.shape == (10,) and float(np.max(np.abs(g.cpu().numpy() - want)) / np.max(np.abs(want))) < 1e-10


# ---- end to end: optical_conductivity against dense eigh, L = 6 at (3, 3) -----------------------------------------------------
E2E_L = 6
CHAIN = tuple((i, i + 1) for i in range(E2E_L - 1))
RING = tuple((i, (i + 1) % E2E_L) for i in range(E2E_L))
BOUND = 1e-8         # the project's bound for a second derivative of E0 (tests/test_gpu_hubbard.py, second order in U)


def uniform(bonds, U):
    nb = len(bonds)
    return np.concatenate([np.ones(nb), np.zeros(nb), U * np.ones(E2E_L), np.zeros(E2E_L)])


def solve(bonds, U, seed, monkeypatch):
    """(operator, E0, psi0) of the half-filled cluster from DominantSparseSymeig; at U = 0 the spectrum is so degenerate that
    the Krylov space ends early, which the solver reports as a warning and resolves exactly"""
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    op = HubbardOperator(E2E_L, bonds, to_dev(uniform(bonds, U)), 3, 3)
    assert op.n == 400
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(seed), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        E0, psi = symeig.DominantSparseSymeig.apply(op.couplings, 200, 400)
    return op, E0.item(), psi.detach()


def deviations(res, want):
    return {k: abs(getattr(res, k) - want[k]) for k in ("diamagnetic", "inverse_moment", "stiffness")}


@pytest.mark.parametrize("basis_free", [False, True])
def test_ring_at_u_4_against_dense_eigh(basis_free, monkeypatch):
    want = cref.optical(E2E_L, 3, 3, RING, uniform(RING, 4.0), np.ones(len(RING)))
    op, E0, psi = solve(RING, 4.0, 3700, monkeypatch)
    res = optical_conductivity(op, psi, E0, torch.ones(len(RING), dtype=F64), k=200, basis_free=basis_free)
    assert isinstance(res, OpticalResponse)
    dev_ = deviations(res, want)
    print("ring U = 4, basis_free = %s: E0 err %.2e   K_d = %.10f (err %.2e)   I_-1 = %.10f (err %.2e)   stiffness = %.10f "
          "(err %.2e)   bound 1e-8   dropped weight %.2e   %d poles"
          % (basis_free, abs(E0 - want["E0"]), res.diamagnetic, dev_["diamagnetic"], res.inverse_moment, dev_["inverse_moment"],
             res.stiffness, dev_["stiffness"], res.dropped_weight, len(res.measure)))
    assert abs(res.measure.norm2 - want["norm2"]) <= BOUND
    assert all(v <= BOUND for v in dev_.values()), dev_
    assert res.dropped_weight <= 1e-16
    lhs, rhs = res.f_sum()
    assert abs(lhs - rhs) <= 1e-14 * rhs
    if not basis_free:
        # the spin twist: the same diamagnetic term, the current of the twin's "spin" weights
        spin = optical_conductivity(op, psi, E0, torch.ones(len(RING), dtype=F64), kind="spin", k=200)
        swant = cref.optical(E2E_L, 3, 3, RING, uniform(RING, 4.0), np.ones(len(RING)), kind="spin")
        assert all(v <= BOUND for v in deviations(spin, swant).values())
        with pytest.raises(ValueError):
            optical_conductivity(op, psi, E0, torch.ones(len(RING) + 1, dtype=F64))
        with pytest.raises(ValueError):
            optical_conductivity(op, psi, E0, torch.ones(len(RING), dtype=F64), kind="heat")


def test_open_chain_has_no_stiffness(monkeypatch):
    want = cref.optical(E2E_L, 3, 3, CHAIN, uniform(CHAIN, 4.0), np.ones(len(CHAIN)))
    op, E0, psi = solve(CHAIN, 4.0, 3701, monkeypatch)
    res = optical_conductivity(op, psi, E0, torch.ones(len(CHAIN), dtype=F64), k=200)
    print("open chain U = 4: K_d = %.10f   2 I_-1 = %.10f   stiffness = %.2e (bound 1e-8)   deviations from eigh %s"
          % (res.diamagnetic, 2.0 * res.inverse_moment, res.stiffness, deviations(res, want)))
    assert abs(res.stiffness) <= BOUND
    assert all(v <= BOUND for v in deviations(res, want).values())


def test_closed_shell_ring_carries_no_current(monkeypatch):
    op, E0, psi = solve(RING, 0.0, 3702, monkeypatch)
    res = optical_conductivity(op, psi, E0, torch.ones(len(RING), dtype=F64), k=200)
    print("ring U = 0: E0 = %.12f   |K psi0|^2 = %.2e (bound 1e-20)   K_d = %.12f" % (E0, res.measure.norm2, res.diamagnetic))
    assert abs(E0 + 8.0) <= 1e-12 * 8.0
    assert res.measure.norm2 <= 1e-20
    assert abs(res.diamagnetic - 8.0) <= BOUND and abs(res.stiffness - 8.0) <= BOUND


def test_example_optical():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "hubbard", "optical.py")
    spec = importlib.util.spec_from_file_location("hubbard_optical", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    orig = CG.EPS_DEFAULT
    try:
        out = ex.main(L=4)
    finally:
        CG.EPS_DEFAULT = orig
    assert out["L"] == 4 and len(out["ring"]) == len(out["U"]) == len(out["sigma"])
    for row in out["ring"] + [out["chain"]]:
        assert abs(row["f_sum"][0] - row["f_sum"][1]) <= 1e-13 * abs(row["f_sum"][1])
        assert row["dropped_weight"] <= 1e-12 and row["diamagnetic"] > 0.0 and row["gap"] > 0.0
    gaps = [row["gap"] for row in out["ring"]]
    assert all(a < b for a, b in zip(gaps, gaps[1:]))                  # the Mott gap grows with U
    assert abs(out["chain"]["stiffness"]) <= BOUND
    assert all(float(s.min()) >= 0.0 and s.shape == out["omega"].shape for s in out["sigma"])
    # against dense eigh at the example's U = 4
    ring = [(i, (i + 1) % 4) for i in range(4)]
    p = np.concatenate([np.ones(4), np.zeros(4), 4.0 * np.ones(4), np.zeros(4)])
    want = cref.optical(4, 2, 2, ring, p, np.ones(4))
    got = out["ring"][out["U"].index(4.0)]
    assert all(abs(got[k] - want[k]) <= BOUND for k in ("diamagnetic", "inverse_moment", "stiffness"))
