"""XYZ spins on a caller-given bond list on the GPU (docs/design/16-spin-lattice.md): k_spmv_lattice and k_lattice_forms
against the numpy row formula of tests/lattice_reference.py at the smallest sizes that reach each path of a bond (LDS, far
with one or both bits outside the tile, the site-0 swap, full bond tables, blocks that walk tiles), then the primitives end to
end against torch.linalg.eigh autograd and a closed form.

    L        tile       bonds                                            path
    2 3 5    default    random, (0,1) twice at L = 2, a reversed pair    tile = whole vector
    6        2^6        complete graph, 15 bonds                         everything in LDS, site-0 swaps
    7        2^6        (0,6) (5,6) (2,6) (1,3)                          far with swap; far with one bit inside; LDS
    9        2^6        complete graph, 36 bonds                         both bits far (6,7) (6,8) (7,8) beside the others
    9        2^6        complete graph listed cyclically up to the cap   full tables, repeated bonds
    13       2^11       30 random pairs                                  four tiles, default tuning
    19       2^6        24 random pairs                                  8192 tiles > the 4096-block cap: blocks walk tiles
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import chain_reference  # noqa: E402
import lattice_reference as ref  # noqa: E402
from helpers import PatchRandn, unit  # noqa: E402
from dominantsparseeigenad_amd import _lib, engine  # noqa: E402
from dominantsparseeigenad_amd.engine import Workspace, _ptr, _stream  # noqa: E402
from dominantsparseeigenad_amd.operators import SpinChainOperator, SpinLatticeOperator, ring_bonds, square_bonds  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402
import dominantsparseeigenad_amd.symeig as symeig  # noqa: E402
import dominantsparseeigenad_amd.CG as CG  # noqa: E402

F64 = torch.float64
TOL = 1e-10
CAP = _lib.LATTICE_MAX_BONDS


def small_bonds(L):
    """random pairs with one of them listed again reversed; at L = 2 that is (0, 1) more than once"""
    bonds = ref.random_bonds(L, L + 1, 7000 + L)
    a, b = bonds[0]
    return tuple(bonds + [(b, a)]) if L > 2 else ((0, 1), (0, 1), (1, 0))


def cyclic_complete(L, count):
    full = ref.complete_bonds(L)
    return tuple(full[i % len(full)] for i in range(count))


# name -> (L, tile, bonds)
GEOMETRY = {
    "L2": (2, None, small_bonds(2)),
    "L3": (3, None, small_bonds(3)),
    "L5": (5, None, small_bonds(5)),
    "L6-complete": (6, 6, tuple(ref.complete_bonds(6))),
    "L7-far": (7, 6, ((0, 6), (5, 6), (2, 6), (1, 3))),
    "L9-complete": (9, 6, tuple(ref.complete_bonds(9))),
    "L9-cap": (9, 6, cyclic_complete(9, CAP)),
    "L13-default": (13, None, tuple(ref.random_bonds(13, 30, 7013))),
    "L19-walk": (19, 6, tuple(ref.random_bonds(19, 24, 7019))),
}
KINDS = ["random", "jy-only"]


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


def couplings(L, bonds, kind, seed=8000):
    nb = len(bonds)
    p = normal_vector(ref.nparam(L, bonds), seed + L + nb).copy()
    if kind == "jy-only":
        p[:nb] = 0.0
        p[2 * nb:] = 0.0
    return p


@functools.lru_cache(maxsize=None)
def case(name, kind):
    """(couplings, x, H x) on the host, computed once per case and never written to"""
    L, _, bonds = GEOMETRY[name]
    p = couplings(L, bonds, kind)
    x = normal_vector(1 << L, 8100 + L)
    y = ref.apply(L, bonds, p, x)
    for a in (p, x, y):
        a.setflags(write=False)
    return p, x, y


@functools.lru_cache(maxsize=None)
def form_case(name):
    L, _, bonds = GEOMETRY[name]
    v1, v2 = normal_vector(1 << L, 8200 + L), normal_vector(1 << L, 8300 + L)
    out = ref.forms(L, bonds, v1, v2)
    for a in (v1, v2, out):
        a.setflags(write=False)
    return v1, v2, out


def to_dev(a):
    return torch.from_numpy(np.array(a)).to(dev())      # (a copy: the cached case arrays are read-only)


def operator(L, bonds, p, tile):
    op = SpinLatticeOperator(L, bonds, to_dev(p))
    if tile is not None:
        op.set_tile_log2(tile)
    return op


def relnorm(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def test_the_cases_are_what_the_table_says():
    assert GEOMETRY["L2"][2].count((0, 1)) == 2
    for name in ("L3", "L5"):
        bonds = GEOMETRY[name][2]
        assert any((b, a) in bonds for a, b in bonds)
    assert len(GEOMETRY["L6-complete"][2]) == 15 and len(GEOMETRY["L9-complete"][2]) == 36
    assert len(GEOMETRY["L9-cap"][2]) == CAP and len(set(GEOMETRY["L9-cap"][2])) == 36
    assert len(GEOMETRY["L13-default"][2]) == 30 and len(GEOMETRY["L19-walk"][2]) == 24


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_matvec_against_the_row_formula(name, kind):
    L, tile, bonds = GEOMETRY[name]
    p, x, want = case(name, kind)
    n = 1 << L
    op = operator(L, bonds, p, tile)
    xd = to_dev(x)
    got = op(xd).cpu().numpy()
    err = relnorm(got, want)
    print("%s %s: |y - ref| / |ref| = %.2e" % (name, kind, err))
    assert err < 1e-13
    # the full contract of a kind in launch_spmv: y = H x - shift x, the block partials of x.y, and the skip flag
    lib = _lib.load()
    ws = Workspace.get(n, 8, dev())
    shift = torch.tensor([0.375], dtype=F64, device=dev())
    dot = torch.zeros(1, dtype=F64, device=dev())
    y = torch.empty(n, dtype=F64, device=dev())
    _lib.check(lib.dsea_spmv(op.handle, ws.handle, _ptr(xd), _ptr(y), _ptr(shift), _ptr(dot), None, _stream(dev())), "dsea_spmv")
    shifted = want - 0.375 * x
    err_s = relnorm(y.cpu().numpy(), shifted)
    err_d = abs(dot.item() - float(x @ shifted)) / (np.linalg.norm(x) * np.linalg.norm(shifted))
    print("    with shift: %.2e   x.y from the partials: %.2e" % (err_s, err_d))
    assert err_s < 1e-13
    assert err_d < 1e-13
    flag = torch.ones(1, dtype=F64, device=dev())
    sentinel = torch.full((n,), -7.0, dtype=F64, device=dev())
    _lib.check(lib.dsea_spmv(op.handle, ws.handle, _ptr(xd), _ptr(sentinel), _ptr(shift), None, _ptr(flag), _stream(dev())),
               "dsea_spmv")
    assert bool((sentinel == -7.0).all())


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_forms_against_the_reference_sums(name):
    L, tile, bonds = GEOMETRY[name]
    v1, v2, want = form_case(name)
    op = operator(L, bonds, couplings(L, bonds, "random"), tile)
    a, b = to_dev(v1), to_dev(v2)
    got = op.Hadjoint_to_couplingsadjoint(a, b)
    assert got.shape == (3 * len(bonds) + 2 * L,)
    bound = 1e-13 * np.linalg.norm(v1) * np.linalg.norm(v2)
    err = float(np.max(np.abs(got.cpu().numpy() - want)))
    print("%s: max |form - ref| = %.2e (bound %.2e)" % (name, err, bound))
    assert err <= bound
    again = op.Hadjoint_to_couplingsadjoint(a, b)
    assert torch.equal(got, again)                       # fixed-order reductions, no atomics


def test_matvec_is_symmetric():
    L, tile, bonds = GEOMETRY["L13-default"]
    p, x, _ = case("L13-default", "random")
    op = operator(L, bonds, p, tile)
    v1 = to_dev(x)
    v2 = torch.from_numpy(normal_vector(1 << L, 8400)).to(dev())
    a, b = float(v1 @ op(v2)), float(v2 @ op(v1))
    assert abs(a - b) <= 1e-13 * float(v1.norm() * op(v2).norm() + v2.norm() * op(v1).norm())


def test_ring_bonds_against_the_chain_operator():
    L = 12
    c = normal_vector(5 * L, 8500)
    x = torch.from_numpy(normal_vector(1 << L, 8510)).to(dev())
    x2 = torch.from_numpy(normal_vector(1 << L, 8520)).to(dev())
    chain = SpinChainOperator(L, to_dev(c.reshape(5, L)))
    lat = SpinLatticeOperator(L, ring_bonds(L), to_dev(c))      # nb = L: the flat order is the chain's (5, L) row by row
    want, got = chain(x), lat(x)
    assert float((got - want).norm() / want.norm()) < 1e-13
    fw, fg = chain.Hadjoint_to_couplingsadjoint(x, x2).reshape(-1), lat.Hadjoint_to_couplingsadjoint(x, x2)
    assert float((fg - fw).abs().max()) <= 1e-13 * float(x.norm() * x2.norm())


def test_to_csr_is_the_same_matrix():
    L, _, bonds = GEOMETRY["L9-complete"]
    p, x, want = case("L9-complete", "random")
    op = operator(L, bonds, p, None)
    csr = op.to_csr()
    assert csr.nnz == (1 << L) * (1 + L + 36)
    xd = to_dev(x)
    assert relnorm(csr(xd).cpu().numpy(), want) < 1e-13
    assert float((csr(xd) - op(xd)).norm() / op(xd).norm()) < 1e-13


def test_to_csr_sums_a_repeated_bond_into_one_column():
    L, bonds = 4, ((0, 1), (2, 3), (1, 0), (1, 3))
    p = couplings(L, bonds, "random")
    x = normal_vector(1 << L, 8530)
    want = ref.apply(L, bonds, p, x)
    op = operator(L, bonds, p, None)
    csr = op.to_csr()
    assert csr.nnz == (1 << L) * (1 + L + 3)             # four bonds, three distinct masks
    xd = to_dev(x)
    assert relnorm(csr(xd).cpu().numpy(), want) < 1e-13
    assert relnorm(op(xd).cpu().numpy(), want) < 1e-13


def test_couplings_changed_in_place_are_seen_without_a_new_operator():
    L, tile, bonds = GEOMETRY["L9-complete"]
    p, x, _ = case("L9-complete", "random")
    op = operator(L, bonds, p, tile)
    assert op.bonds == bonds and isinstance(op.bonds, tuple)
    handle = op.handle.value
    xd = to_dev(x)
    op(xd)
    p2 = normal_vector(p.size, 8600)
    with torch.no_grad():
        op.couplings.copy_(torch.from_numpy(p2))
    assert op.handle.value == handle
    assert relnorm(op(xd).cpu().numpy(), ref.apply(L, bonds, p2, x)) < 1e-13
    # pack / unpack: five views of the same storage, in the order of the parameter
    parts = op.unpack(op.couplings)
    assert [t.numel() for t in parts] == [36, 36, 36, L, L]
    assert all(t.data_ptr() == op.couplings.data_ptr() + 8 * off for t, off in zip(parts, (0, 36, 72, 108, 108 + L)))
    assert torch.equal(op.pack(*parts), op.couplings)
    with pytest.raises(ValueError):
        op.couplings = torch.zeros(p.size + 1, dtype=F64, device=dev())
    with pytest.raises(ValueError):
        op.couplings = torch.zeros(p.size, dtype=torch.float32, device=dev())
    with pytest.raises(ValueError):
        SpinLatticeOperator(L, cyclic_complete(L, CAP + 1), torch.zeros(3 * (CAP + 1) + 2 * L, dtype=F64, device=dev()))
    with pytest.raises(ValueError):
        SpinLatticeOperator(L, ((0, 1), (4, 4)), torch.zeros(6 + 2 * L, dtype=F64, device=dev()))


# ---- end to end ------------------------------------------------------------------------------------------------------
def dense_torch(L, bonds, p):
    """the dense matrix as a differentiable function of the flat couplings p (CPU): the row formula, entry by entry"""
    n, nb = 1 << L, len(bonds)
    s = torch.arange(n, dtype=torch.int64)
    z = [(1 - 2 * ((s >> i) & 1)).to(F64) for i in range(L)]
    H = torch.zeros((n, n), dtype=F64)
    for i in range(L):
        H = H.index_put((s, s), p[3 * nb + L + i] * z[i], accumulate=True)
        H = H.index_put((s, s ^ (1 << i)), p[3 * nb + i].expand(n), accumulate=True)
    for t, (a, b) in enumerate(bonds):
        zz = z[a] * z[b]
        H = H.index_put((s, s), p[2 * nb + t] * zz, accumulate=True)
        H = H.index_put((s, s ^ ((1 << a) | (1 << b))), p[t] - p[nb + t] * zz, accumulate=True)
    return H


def test_dense_torch_is_the_reference_matrix():
    L, bonds = 5, small_bonds(5)
    p = couplings(L, bonds, "random")
    assert np.max(np.abs(dense_torch(L, bonds, torch.from_numpy(p)).numpy() - ref.dense(L, bonds, p))) < 1e-14


def test_ground_state_and_its_gradient_against_eigh(monkeypatch):
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, k, seed = 9, 300, 9702
    bonds = square_bonds(3, 3)
    assert len(bonds) == 18
    n = 1 << L
    p0 = torch.from_numpy(normal_vector(3 * 18 + 2 * L, seed).copy())
    u = unit(n, 9200)
    pr = p0.clone().requires_grad_(True)
    lam, U = torch.linalg.eigh(dense_torch(L, bonds, pr))
    assert float(lam[1] - lam[0]) >= 0.02 * float(lam[-1] - lam[0])       # a gap Lanczos resolves with k = 300
    (g_ref,) = torch.autograd.grad(lam[0] + (U[:, 0] @ u) ** 2, pr)
    op = SpinLatticeOperator(L, bonds, p0.to(dev()).requires_grad_(True))
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(9300):
        E0, psi = symeig.DominantSparseSymeig.apply(op.couplings, k, n)
        (g,) = torch.autograd.grad(E0 + (psi @ u.to(dev())) ** 2, op.couplings)
    assert engine.last_cg.converged
    e_err = abs(E0.item() - lam[0].item()) / abs(lam[0].item())
    g_err = float((g.cpu() - g_ref).abs().max()) / float(g_ref.abs().max())
    print("3x3 torus: E0 rel err %.2e   d(E0 + (psi.u)^2)/d couplings: max abs err / max = %.2e" % (e_err, g_err))
    assert g.shape == (3 * 18 + 2 * 9,)
    assert e_err < 1e-12
    assert g_err < TOL


def j1j2_line(L, seed):
    bonds = ring_bonds(L, 1) + ring_bonds(L, 2)
    m = 3 * len(bonds) + 2 * L
    return bonds, torch.from_numpy(normal_vector(m, seed).copy()), torch.from_numpy(normal_vector(m, seed + 18).copy())


def test_second_order_along_a_line_of_couplings(monkeypatch):
    """couplings = p0 + t p1: d^2 E0 / dt^2 through the re-entrant mat-vec / forms pair against eigh double backward, at the
    tolerance of the second-order test of tests/test_gpu_chain.py"""
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, k = 8, 200
    n = 1 << L
    bonds, p0, p1 = j1j2_line(L, 9721)
    tr = torch.tensor(0.0, dtype=F64, requires_grad=True)
    lam, _ = torch.linalg.eigh(dense_torch(L, bonds, p0 + tr * p1))
    (r1,) = torch.autograd.grad(lam[0], tr, create_graph=True)
    (r2,) = torch.autograd.grad(r1, tr)
    t = torch.tensor(0.0, dtype=F64, device=dev(), requires_grad=True)
    op = SpinLatticeOperator(L, bonds, (p0.to(dev()) + t * p1.to(dev())))
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(9400):
        E0, _ = symeig.DominantSparseSymeig.apply(op.couplings, k, n)
        (g1,) = torch.autograd.grad(E0, t, create_graph=True)
        (g2,) = torch.autograd.grad(g1, t)
    e1 = abs(g1.item() - r1.item()) / abs(r1.item())
    e2 = abs(g2.item() - r2.item()) / abs(r2.item())
    print("dE0/dt rel err %.2e   d2E0/dt2 rel err %.2e  (%.6f vs %.6f)" % (e1, e2, g2.item(), r2.item()))
    assert e1 < TOL
    assert e2 < 1e-8


def test_gap_and_its_gradient_through_the_lowest_two_levels(monkeypatch):
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, k = 8, 200
    n = 1 << L
    bonds, p0, _ = j1j2_line(L, 9721)
    pr = p0.clone().requires_grad_(True)
    lam, _ = torch.linalg.eigh(dense_torch(L, bonds, pr))
    spread = float(lam[-1] - lam[0])
    assert float(lam[1] - lam[0]) >= 1e-3 * spread and float(lam[2] - lam[1]) >= 1e-3 * spread
    gap_ref = lam[1] - lam[0]
    (g_ref,) = torch.autograd.grad(gap_ref, pr)
    op = SpinLatticeOperator(L, bonds, p0.to(dev()).requires_grad_(True))
    symeig.setLowestSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(9500):
        vals, _ = symeig.LowestSparseSymeig.apply(op.couplings, k, n, 2)
        gap = vals[1] - vals[0]
        (g,) = torch.autograd.grad(gap, op.couplings)
    gap_err = abs(gap.item() - gap_ref.item()) / abs(gap_ref.item())
    g_err = float((g.cpu() - g_ref).abs().max()) / float(g_ref.abs().max())
    print("gap rel err %.2e   dgap/dcouplings max abs err / max = %.2e" % (gap_err, g_err))
    assert gap_err < TOL
    assert g_err < TOL


def test_majumdar_ghosh_ground_state_energy_is_the_closed_form(monkeypatch):
    """J1-J2 Heisenberg ring at J2 = J1 / 2: E0 = -1.5 L exactly (twofold degenerate: forward only)"""
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, k = 10, 300
    bonds = ring_bonds(L, 1) + ring_bonds(L, 2)
    j = torch.cat([torch.ones(L, dtype=F64), 0.5 * torch.ones(L, dtype=F64)])
    p = torch.cat([j, j, j, torch.zeros(2 * L, dtype=F64)]).to(dev())
    op = SpinLatticeOperator(L, bonds, p)
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(9600):
        E0, _ = symeig.DominantSparseSymeig.apply(op.couplings, k, 1 << L)
    want = -1.5 * L
    assert abs(E0.item() - want) < 1e-12 * abs(want), (E0.item(), want)


def test_example_j1j2():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "spin_lattice", "j1j2.py")
    spec = importlib.util.spec_from_file_location("spin_lattice_j1j2", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    orig = CG.EPS_DEFAULT
    try:
        out = ex.main(L=8)
        h = 1e-4
        fd = (ex.energy(8, 0.3 + h, device=dev()) - ex.energy(8, 0.3 - h, device=dev())) / (2 * h)
    finally:
        CG.EPS_DEFAULT = orig
    print("E0(MG) = %.12f   dE0/dJ2 at 0.3: autograd %.9f   central difference %.9f" % (out["E0_mg"], out["dE0_dJ2"], fd))
    assert abs(out["E0_mg"] + 12.0) < 1e-12 * 12.0
    assert out["J2_grad"] == 0.3
    assert abs(out["dE0_dJ2"] - fd) < 1e-5
    assert len(out["E0"]) == len(out["gap"]) == len(out["J2"])
