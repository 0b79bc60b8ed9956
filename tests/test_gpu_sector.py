"""XXZ spins in one magnetisation sector on the GPU (docs/design/18-spin-sector.md): the table builders, k_spmv_sector and
k_sector_forms against the sector-native numpy reference of tests/sector_reference.py at the smallest sizes that reach each
path, then the merged full-space operator as a cross-check and the primitives end to end against torch.linalg.eigh autograd
and a closed form.

    L, ndown              n         bonds                                        what it reaches
    2,1  3,1  3,2  5,2    2 3 3 10  random, a reversed pair, (0,1) twice at L=2  tiny and odd n, less than one wave
    7,3                   35        (0,6) (5,6) (2,3) (1,4)                      odd L (Llo = 4, Lhi = 3), odd n; bonds inside lo,
                                                                                 inside hi, across the split
    8,4                   70        complete graph, 28                           every split case at once
    9,4                   126       complete graph cycled to the cap, 128        full bond table, repeated bonds
    11,5                  462       20 random                                    two blocks, ragged last block
    16,8                  12 870    24 random                                    many blocks
    20,10                 184 756   24 random                                    722 row ranges on a grid capped at 64 blocks
                                                                                 (the smallest cap): blocks walk ranges
    20,1  20,19           20 20     ring                                         extreme fillings
    34,2  40,1  40,2      561 40 780  ring + 10 random                           states wider than 32 bits
"""
import functools
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lattice_reference  # noqa: E402
import sector_reference as ref  # noqa: E402
from helpers import PatchRandn, unit  # noqa: E402
from dominantsparseeigenad_amd import _lib, engine  # noqa: E402
from dominantsparseeigenad_amd.engine import Workspace, _ptr, _stream  # noqa: E402
from dominantsparseeigenad_amd.operators import (SpinLatticeOperator, SpinSectorOperator, ring_bonds, sector_dim,  # noqa: E402
                                                 sector_states)
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402
import dominantsparseeigenad_amd.symeig as symeig  # noqa: E402
import dominantsparseeigenad_amd.CG as CG  # noqa: E402

F64 = torch.float64
TOL = 1e-10
CAP = _lib.LATTICE_MAX_BONDS


def small_bonds(L):
    """random pairs with one of them listed again reversed; at L = 2 that is (0, 1) more than once"""
    bonds = lattice_reference.random_bonds(L, L + 1, 7100 + L)
    a, b = bonds[0]
    return tuple(bonds + [(b, a)]) if L > 2 else ((0, 1), (0, 1), (1, 0))


def cyclic_complete(L, count):
    full = lattice_reference.complete_bonds(L)
    return tuple(full[i % len(full)] for i in range(count))


def ring_and_random(L):
    return tuple(ring_bonds(L) + lattice_reference.random_bonds(L, 10, 7200 + L))


# name -> (L, ndown, log2 of the grid cap or None for the default, bonds)
GEOMETRY = {
    "L2-1": (2, 1, None, small_bonds(2)),
    "L3-1": (3, 1, None, small_bonds(3)),
    "L3-2": (3, 2, None, small_bonds(3)),
    "L5-2": (5, 2, None, small_bonds(5)),
    "L7-3-split": (7, 3, None, ((0, 6), (5, 6), (2, 3), (1, 4))),
    "L8-4-complete": (8, 4, None, tuple(lattice_reference.complete_bonds(8))),
    "L9-4-cap": (9, 4, None, cyclic_complete(9, CAP)),
    "L11-5": (11, 5, None, tuple(lattice_reference.random_bonds(11, 20, 7111))),
    "L16-8": (16, 8, None, tuple(lattice_reference.random_bonds(16, 24, 7116))),
    "L20-10-walk": (20, 10, 6, tuple(lattice_reference.random_bonds(20, 24, 7120))),
    "L20-1": (20, 1, None, tuple(ring_bonds(20))),
    "L20-19": (20, 19, None, tuple(ring_bonds(20))),
    "L34-2": (34, 2, None, ring_and_random(34)),
    "L40-1": (40, 1, None, ring_and_random(40)),
    "L40-2": (40, 2, None, ring_and_random(40)),
}
KINDS = ["random", "jxy-only"]


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


def couplings(L, bonds, kind, seed=8000):
    nb = len(bonds)
    p = normal_vector(ref.nparam(L, bonds), seed + L + nb).copy()
    if kind == "jxy-only":
        p[nb:] = 0.0
    return p


@functools.lru_cache(maxsize=None)
def case(name, kind):
    """(couplings, x, H x) on the host, computed once per case and never written to"""
    L, ndown, _, bonds = GEOMETRY[name]
    p = couplings(L, bonds, kind)
    x = normal_vector(math.comb(L, ndown), 8100 + L + ndown)
    y = ref.apply(L, ndown, bonds, p, x)
    for a in (p, x, y):
        a.setflags(write=False)
    return p, x, y


@functools.lru_cache(maxsize=None)
def form_case(name):
    L, ndown, _, bonds = GEOMETRY[name]
    n = math.comb(L, ndown)
    v1, v2 = normal_vector(n, 8200 + L + ndown), normal_vector(n, 8300 + L + ndown)
    out = ref.forms(L, ndown, bonds, v1, v2)
    for a in (v1, v2, out):
        a.setflags(write=False)
    return v1, v2, out


def to_dev(a):
    return torch.from_numpy(np.array(a)).to(dev())      # (a copy: the cached case arrays are read-only)


def operator(name, p):
    L, ndown, grid, bonds = GEOMETRY[name]
    op = SpinSectorOperator(L, bonds, to_dev(p), ndown)
    if grid is not None:
        op.set_grid_log2(grid)
    return op


def relnorm(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def test_the_cases_are_what_the_table_says():
    sizes = {name: math.comb(g[0], g[1]) for name, g in GEOMETRY.items()}
    assert [sizes[k] for k in ("L2-1", "L3-1", "L3-2", "L5-2", "L7-3-split", "L8-4-complete", "L9-4-cap", "L11-5", "L16-8",
                               "L20-10-walk", "L20-1", "L20-19", "L34-2", "L40-1", "L40-2")] == \
        [2, 3, 3, 10, 35, 70, 126, 462, 12870, 184756, 20, 20, 561, 40, 780]
    assert GEOMETRY["L2-1"][3].count((0, 1)) == 2
    for name in ("L3-1", "L3-2", "L5-2"):
        bonds = GEOMETRY[name][3]
        assert any((b, a) in bonds for a, b in bonds)
    lo = (7 + 1) // 2                                    # the split of L = 7: sites 0 .. 3 low, 4 .. 6 high
    where = [(a < lo, b < lo) for a, b in GEOMETRY["L7-3-split"][3]]
    assert where == [(True, False), (False, False), (True, True), (True, False)]
    assert len(GEOMETRY["L8-4-complete"][3]) == 28
    assert len(GEOMETRY["L9-4-cap"][3]) == CAP and len(set(GEOMETRY["L9-4-cap"][3])) == 36
    assert len(GEOMETRY["L11-5"][3]) == 20 and len(GEOMETRY["L16-8"][3]) == len(GEOMETRY["L20-10-walk"][3]) == 24
    assert (sizes["L11-5"] + 255) // 256 == 2 and sizes["L11-5"] % 256 != 0
    assert (sizes["L20-10-walk"] + 255) // 256 > (1 << GEOMETRY["L20-10-walk"][2])      # more row ranges than blocks
    for name in ("L34-2", "L40-1", "L40-2"):
        assert len(GEOMETRY[name][3]) == GEOMETRY[name][0] + 10
        assert max(ref.states(GEOMETRY[name][0], GEOMETRY[name][1])) >= 1 << 32


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_tables(name):
    L, ndown, _, bonds = GEOMETRY[name]
    op = operator(name, couplings(L, bonds, "random"))
    n = sector_dim(L, ndown)
    assert op.n == op.dim == n
    states = op.states.cpu()
    assert states.dtype == torch.int64 and states.shape == (n,)
    assert torch.equal(states, torch.tensor(sector_states(L, ndown), dtype=torch.int64))
    # rank(states[r]) == r through the two tables as the kernel reads them, with torch indexing on the downloaded tables
    _, lo_rank, hi_base = (t.cpu() for t in op._tables)
    Llo = (L + 1) // 2
    assert lo_rank.shape == (1 << Llo,) and hi_base.shape == (1 << (L - Llo),)
    rank = hi_base[states >> Llo].to(torch.int64) + lo_rank[states & ((1 << Llo) - 1)].to(torch.int64)
    assert torch.equal(rank, torch.arange(n, dtype=torch.int64))
    assert torch.equal(op.rank(op.states).cpu(), torch.arange(n, dtype=torch.int64))
    # an h that no sector state has carries 0
    used = torch.zeros(1 << (L - Llo), dtype=torch.bool)
    used[states >> Llo] = True
    assert bool((hi_base[~used] == 0).all())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_matvec_against_the_row_formula(name, kind):
    L, ndown, _, bonds = GEOMETRY[name]
    p, x, want = case(name, kind)
    n = x.size
    op = operator(name, p)
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
    L, ndown, _, bonds = GEOMETRY[name]
    v1, v2, want = form_case(name)
    p = couplings(L, bonds, "random")
    op = operator(name, p)
    a, b = to_dev(v1), to_dev(v2)
    got = op.Hadjoint_to_couplingsadjoint(a, b)
    assert got.shape == (2 * len(bonds) + L,)
    norms = np.linalg.norm(v1) * np.linalg.norm(v2)
    bound = 1e-13 * norms
    err = float(np.max(np.abs(got.cpu().numpy() - want)))
    print("%s: max |form - ref| = %.2e (bound %.2e)" % (name, err, bound))
    assert err <= bound
    again = op.Hadjoint_to_couplingsadjoint(a, b)
    assert torch.equal(got, again)                       # fixed-order reductions, no atomics
    # H is linear in the couplings: v1^T H[p] v2 = sum_t p_t form_t.  Each form is within 1e-13 |v1| |v2| of its sum and the
    # mat-vec within 1e-13 |H v2| of its value (the two bounds above), so the two sides differ by at most
    # 1e-13 (|v1| |v2| sum_t |p_t| + |v1| |H v2|)
    Hv2 = op(b)
    lhs, rhs = float(a @ Hv2), float(np.sum(p * got.cpu().numpy()))
    assert abs(lhs - rhs) <= 1e-13 * (norms * np.abs(p).sum() + np.linalg.norm(v1) * float(Hv2.norm()))


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_matvec_is_symmetric(name):
    p, x, _ = case(name, "random")
    op = operator(name, p)
    a = to_dev(x)
    b = torch.from_numpy(normal_vector(x.size, 8400 + x.size % 97)).to(dev())
    Ha, Hb = op(a), op(b)
    assert abs(float(a @ Hb) - float(Ha @ b)) <= 1e-13 * float(a.norm() * Hb.norm() + b.norm() * Ha.norm())


def test_against_the_full_space_operator_and_to_csr():
    """L = 12, ndown = 6: the merged bond-list operator with Jx = Jy = Jxy, hx = 0 maps the sector into itself"""
    L, ndown = 12, 6
    bonds = tuple(lattice_reference.random_bonds(L, 20, 7312)) + ((3, 7), (7, 3))        # (one mask listed twice more)
    p = couplings(L, bonds, "random")
    sec = SpinSectorOperator(L, bonds, to_dev(p), ndown)
    lat = SpinLatticeOperator(L, bonds, to_dev(ref.full_parameter(L, bonds, p)))
    n = sec.n
    assert n == 924
    v = torch.from_numpy(normal_vector(n, 8700)).to(dev())
    w = sec.embed(v)
    assert w.shape == (1 << L,) and float(w.norm()) == float(v.norm()) and torch.equal(sec.restrict(w), v)
    full = lat(w)
    got = sec(v)
    assert float((sec.restrict(full) - got).norm() / got.norm()) < 1e-13
    outside = torch.ones(1 << L, dtype=torch.bool, device=dev())
    outside[sec.states] = False
    assert int(outside.sum()) == (1 << L) - n
    assert bool((full[outside] == 0.0).all())            # exactly: Jx - Jy = 0 bit for bit, and x is 0 off the sector
    csr = sec.to_csr()
    masks = {(1 << a) | (1 << b) for a, b in bonds}
    flips = sum(sum(1 for s in ref.states(L, ndown) if bin(s & m).count("1") == 1) for m in masks)
    assert csr.n == n and csr.nnz == n + flips           # the diagonal, and one entry per (row, distinct mask that flips it)
    assert float((csr(v) - got).norm() / got.norm()) < 1e-13
    assert relnorm(csr(v).cpu().numpy(), ref.apply(L, ndown, bonds, p, v.cpu().numpy())) < 1e-13


def test_couplings_changed_in_place_are_seen_without_a_new_operator():
    name = "L8-4-complete"
    L, ndown, _, bonds = GEOMETRY[name]
    p, x, _ = case(name, "random")
    op = operator(name, p)
    assert op.bonds == bonds and isinstance(op.bonds, tuple)
    handle = op.handle.value
    xd = to_dev(x)
    op(xd)
    delta = normal_vector(p.size, 8600)
    with torch.no_grad():
        op.couplings.add_(torch.from_numpy(delta).to(dev()))
    assert op.handle.value == handle
    assert relnorm(op(xd).cpu().numpy(), ref.apply(L, ndown, bonds, p + delta, x)) < 1e-13
    # pack / unpack: three views of the same storage, in the order of the parameter
    parts = op.unpack(op.couplings)
    assert [t.numel() for t in parts] == [28, 28, L]
    assert all(t.data_ptr() == op.couplings.data_ptr() + 8 * off for t, off in zip(parts, (0, 28, 56)))
    assert torch.equal(op.pack(*parts), op.couplings)
    assert op.pack(1.0, 0.5, 0.0).tolist() == [1.0] * 28 + [0.5] * 28 + [0.0] * L
    # binding another tensor: a new handle on the same tables
    tables = [t.data_ptr() for t in op._tables]
    op.couplings = to_dev(p)
    assert [t.data_ptr() for t in op._tables] == tables
    assert relnorm(op(xd).cpu().numpy(), case(name, "random")[2]) < 1e-13
    with pytest.raises(ValueError):
        op.couplings = torch.zeros(p.size + 1, dtype=F64, device=dev())
    with pytest.raises(ValueError):
        op.couplings = torch.zeros(p.size, dtype=torch.float32, device=dev())
    with pytest.raises(ValueError):
        SpinSectorOperator(L, cyclic_complete(L, CAP + 1), torch.zeros(2 * (CAP + 1) + L, dtype=F64, device=dev()), ndown)
    with pytest.raises(ValueError):
        SpinSectorOperator(L, ((0, 1), (4, 4)), torch.zeros(4 + L, dtype=F64, device=dev()), ndown)
    with pytest.raises(ValueError):
        SpinSectorOperator(34, ((0, 1),), torch.zeros(2 + 34, dtype=F64, device=dev()), 17)


# ---- end to end ------------------------------------------------------------------------------------------------------
E2E_L, E2E_NDOWN = 10, 5
E2E_BONDS = tuple(ring_bonds(E2E_L, 1) + ring_bonds(E2E_L, 2))


def dense_torch(L, ndown, bonds, p):
    """the dense sector matrix as a differentiable function of the flat couplings p (CPU): the row formula, entry by entry"""
    nb = len(bonds)
    n = math.comb(L, ndown)
    r = torch.arange(n, dtype=torch.int64)
    H = torch.zeros((n, n), dtype=F64)
    for i, z in enumerate(ref._z(L, ndown)):
        H = H.index_put((r, r), p[2 * nb + i] * torch.from_numpy(np.array(z)), accumulate=True)
    for t, (rows, cols, zz) in enumerate(ref._partners(L, ndown, bonds)):
        H = H.index_put((r, r), p[nb + t] * torch.from_numpy(np.array(zz)), accumulate=True)
        H = H.index_put((torch.from_numpy(np.array(rows)), torch.from_numpy(np.array(cols))), (2.0 * p[t]).expand(rows.size),
                        accumulate=True)
    return H


def j1j2_point(seed, J2=0.3, noise=0.1):
    """(p0, d2): the J1-J2 Heisenberg ring at J1 = 1 without its J2 part, plus random perturbations of all 2 nb + L couplings
    (no symmetry and no degeneracy left inside the sector); couplings = p0 + J2 d2"""
    L = E2E_L
    near = torch.cat([torch.ones(L, dtype=F64), torch.zeros(L, dtype=F64)])
    nxt = torch.cat([torch.zeros(L, dtype=F64), torch.ones(L, dtype=F64)])
    field = torch.zeros(L, dtype=F64)
    d1, d2 = torch.cat([near, near, field]), torch.cat([nxt, nxt, field])
    p0 = d1 + noise * torch.from_numpy(normal_vector(d1.numel(), seed).copy())
    return p0, d2, J2


def test_dense_torch_is_the_reference_matrix():
    p0, d2, J2 = j1j2_point(9700)
    p = (p0 + J2 * d2).numpy()
    H = dense_torch(E2E_L, E2E_NDOWN, E2E_BONDS, torch.from_numpy(p)).numpy()
    assert H.shape == (252, 252)
    assert np.max(np.abs(H - ref.dense(E2E_L, E2E_NDOWN, E2E_BONDS, p))) < 1e-14


def test_ground_state_and_its_gradient_against_eigh(monkeypatch):
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, ndown, bonds = E2E_L, E2E_NDOWN, E2E_BONDS
    n = k = 252
    p0, d2, J2 = j1j2_point(9702)
    p = p0 + J2 * d2
    u = unit(n, 9200)
    pr = p.clone().requires_grad_(True)
    lam, U = torch.linalg.eigh(dense_torch(L, ndown, bonds, pr))
    (g_ref,) = torch.autograd.grad(lam[0] + (U[:, 0] @ u) ** 2, pr)
    op = SpinSectorOperator(L, bonds, p.to(dev()).requires_grad_(True), ndown)
    assert op.n == n
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(9300):
        E0, psi = symeig.DominantSparseSymeig.apply(op.couplings, k, n)
        (g,) = torch.autograd.grad(E0 + (psi @ u.to(dev())) ** 2, op.couplings)
    assert engine.last_cg.converged
    e_err = abs(E0.item() - lam[0].item()) / abs(lam[0].item())
    g_err = float((g.cpu() - g_ref).abs().max()) / float(g_ref.abs().max())
    print("J1-J2 ring, L = 10, S^z = 0: E0 rel err %.2e   d(E0 + (psi.u)^2)/d couplings: max abs err / max = %.2e" % (e_err, g_err))
    assert g.shape == (2 * 20 + 10,)
    assert e_err < 1e-12
    assert g_err < TOL


def test_gap_and_its_gradient_through_the_lowest_two_levels(monkeypatch):
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, ndown, bonds = E2E_L, E2E_NDOWN, E2E_BONDS
    n = k = 252
    p0, d2, J2 = j1j2_point(9702)
    p = p0 + J2 * d2
    pr = p.clone().requires_grad_(True)
    lam, _ = torch.linalg.eigh(dense_torch(L, ndown, bonds, pr))
    gap_ref = lam[1] - lam[0]
    (g_ref,) = torch.autograd.grad(gap_ref, pr)
    op = SpinSectorOperator(L, bonds, p.to(dev()).requires_grad_(True), ndown)
    symeig.setLowestSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(9500):
        vals, _ = symeig.LowestSparseSymeig.apply(op.couplings, k, n, 2)
        gap = vals[1] - vals[0]
        (g,) = torch.autograd.grad(gap, op.couplings)
    e_err = abs(vals[0].item() - lam[0].item()) / abs(lam[0].item())
    gap_err = abs(gap.item() - gap_ref.item()) / abs(gap_ref.item())
    g_err = float((g.cpu() - g_ref).abs().max()) / float(g_ref.abs().max())
    print("E0 rel err %.2e   gap rel err %.2e   dgap/dcouplings max abs err / max = %.2e" % (e_err, gap_err, g_err))
    assert e_err < 1e-12
    assert gap_err < TOL
    assert g_err < TOL


def test_second_order_in_J2(monkeypatch):
    """couplings = p0 + J2 d2: d^2 E0 / dJ2^2 through the re-entrant mat-vec / forms pair against eigh double backward, at the
    tolerance of the second-order test of tests/test_gpu_lattice.py (1e-8 relative)"""
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, ndown, bonds = E2E_L, E2E_NDOWN, E2E_BONDS
    n = k = 252
    p0, d2, J2 = j1j2_point(9721)
    tr = torch.tensor(J2, dtype=F64, requires_grad=True)
    lam, _ = torch.linalg.eigh(dense_torch(L, ndown, bonds, p0 + tr * d2))
    (r1,) = torch.autograd.grad(lam[0], tr, create_graph=True)
    (r2,) = torch.autograd.grad(r1, tr)
    t = torch.tensor(J2, dtype=F64, device=dev(), requires_grad=True)
    op = SpinSectorOperator(L, bonds, (p0.to(dev()) + t * d2.to(dev())), ndown)
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(9400):
        E0, _ = symeig.DominantSparseSymeig.apply(op.couplings, k, n)
        (g1,) = torch.autograd.grad(E0, t, create_graph=True)
        (g2,) = torch.autograd.grad(g1, t)
    e1 = abs(g1.item() - r1.item()) / abs(r1.item())
    e2 = abs(g2.item() - r2.item()) / abs(r2.item())
    print("dE0/dJ2 rel err %.2e   d2E0/dJ2^2 rel err %.2e  (%.6f vs %.6f)" % (e1, e2, g2.item(), r2.item()))
    assert e1 < TOL
    assert e2 < 1e-8


def test_majumdar_ghosh_ground_state_energy_is_the_closed_form(monkeypatch):
    """J1-J2 Heisenberg ring at J2 = J1 / 2 in S^z = 0: E0 = -1.5 L exactly (twofold degenerate: forward only)"""
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, k = 16, 300
    bonds = ring_bonds(L, 1) + ring_bonds(L, 2)
    j = torch.cat([torch.ones(L, dtype=F64), 0.5 * torch.ones(L, dtype=F64)])
    p = torch.cat([j, j, torch.zeros(L, dtype=F64)]).to(dev())
    op = SpinSectorOperator(L, bonds, p, L // 2)
    assert op.n == 12870
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(9600):
        E0, _ = symeig.DominantSparseSymeig.apply(op.couplings, k, op.n)
    want = -1.5 * L
    assert abs(E0.item() - want) < 1e-12 * abs(want), (E0.item(), want)


def test_example_sector():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "spin_lattice", "sector.py")
    spec = importlib.util.spec_from_file_location("spin_lattice_sector", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    orig = CG.EPS_DEFAULT
    try:
        out = ex.main(L=10, L_mg=8)
        h = 1e-4
        fd = (ex.energy(10, 0.3 + h, device=dev()) - ex.energy(10, 0.3 - h, device=dev())) / (2 * h)
    finally:
        CG.EPS_DEFAULT = orig
    print("E0(MG, L = 8) = %.12f   dE0/dJ2 at 0.3: autograd %.9f   central difference %.9f" % (out["E0_mg"], out["dE0_dJ2"], fd))
    assert out["n"] == 252 and out["L_mg"] == 8
    assert abs(out["E0_mg"] + 12.0) < 1e-12 * 12.0
    assert out["J2_grad"] == 0.3
    assert abs(out["dE0_dJ2"] - fd) < 1e-5
    assert len(out["E0"]) == len(out["gap"]) == len(out["J2"])
    assert all(g > 0.0 for g in out["gap"])
