"""The Hubbard model at fixed (nup, ndn) on the GPU (docs/design/19-hubbard.md): k_spmv_hubbard and k_hubbard_forms against
the numpy reference of tests/hubbard_reference.py at the smallest sizes that reach each path, then the explicit matrix, the
primitives end to end against torch.linalg.eigh autograd, two closed forms and the example.

    L, nup, ndn             n_up x n_dn = n          bonds                           what it reaches
    2,1,1                   2 x 2 = 4                (0,1) (0,1) (1,0)               less than a wave; repeated and reversed bond
    3,1,2  4,2,1  5,2,3     9, 24, 100               random + one reversed           n_dn < 64: many ru in one wave; nup != ndn
    6,3,3                   20 x 20 = 400            the ten bonds of the loop       two blocks, ragged last block; shared tables
                                                     lattice
    7,3,2                   35 x 21 = 735            (0,6) (5,6) (2,3) (1,4)         odd L (Llo = 4, Lhi = 3); sign masks inside
                                                                                     lo, inside hi, across
    8,4,4                   70 x 70 = 4 900          complete graph, 28              n_dn = 70: waves straddle an ru boundary
    9,3,5  9,5,3            84 x 126, 126 x 84       complete graph cycled to 128    full bond table; two different table sets,
                            = 10 584                                                 both orders
    10,5,5, grid cap 2^6    252 x 252 = 63 504       24 random                       249 row ranges on 64 blocks: blocks walk
    12,1,11  12,11,1        144                      ring                            extreme fillings
    34,1,1  40,2,1  40,1,2  1 156, 31 200, 31 200    ring + 10 random                words and sign masks wider than 32 bits; the
                                                                                     bond (39, 0) spans bits 1 .. 38
"""
import functools
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hubbard_reference as ref  # noqa: E402
import lattice_reference  # noqa: E402
from helpers import PatchRandn, unit  # noqa: E402
from dominantsparseeigenad_amd import _lib, engine  # noqa: E402
from dominantsparseeigenad_amd.engine import Workspace, _ptr, _stream  # noqa: E402
from dominantsparseeigenad_amd.operators import HubbardOperator, hubbard_dim, ring_bonds, sector_states  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402
import dominantsparseeigenad_amd.symeig as symeig  # noqa: E402
import dominantsparseeigenad_amd.CG as CG  # noqa: E402

F64 = torch.float64
TOL = 1e-10
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
    "L3-1-2": (3, 1, 2, None, small_bonds(3)),
    "L4-2-1": (4, 2, 1, None, small_bonds(4)),
    "L5-2-3": (5, 2, 3, None, small_bonds(5)),
    "L6-3-3-loops": (6, 3, 3, None, LOOP_BONDS),
    "L7-3-2-split": (7, 3, 2, None, ((0, 6), (5, 6), (2, 3), (1, 4))),
    "L8-4-4-complete": (8, 4, 4, None, tuple(lattice_reference.complete_bonds(8))),
    "L9-3-5-cap": (9, 3, 5, None, cyclic_complete(9, CAP)),
    "L9-5-3-cap": (9, 5, 3, None, cyclic_complete(9, CAP)),
    "L10-5-5-walk": (10, 5, 5, 6, tuple(lattice_reference.random_bonds(10, 24, 7510))),
    "L12-1-11": (12, 1, 11, None, tuple(ring_bonds(12))),
    "L12-11-1": (12, 11, 1, None, tuple(ring_bonds(12))),
    "L34-1-1": (34, 1, 1, None, ring_and_random(34)),
    "L40-2-1": (40, 2, 1, None, ring_and_random(40)),
    "L40-1-2": (40, 1, 2, None, ring_and_random(40)),
}
KINDS = ["random", "hopping-only"]


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


def couplings(L, bonds, kind, seed=8000):
    nb = len(bonds)
    p = normal_vector(ref.nparam(L, bonds), seed + L + nb).copy()
    if kind == "hopping-only":
        p[nb:] = 0.0
    return p


@functools.lru_cache(maxsize=None)
def case(name, kind):
    """(couplings, x, H x) on the host, computed once per case and never written to"""
    L, nup, ndn, _, bonds = GEOMETRY[name]
    p = couplings(L, bonds, kind)
    x = normal_vector(hubbard_dim(L, nup, ndn), 8100 + L + nup)
    y = ref.apply(L, nup, ndn, bonds, p, x)
    for a in (p, x, y):
        a.setflags(write=False)
    return p, x, y


@functools.lru_cache(maxsize=None)
def form_case(name):
    L, nup, ndn, _, bonds = GEOMETRY[name]
    n = hubbard_dim(L, nup, ndn)
    v1, v2 = normal_vector(n, 8200 + L + nup), normal_vector(n, 8300 + L + nup)
    out = ref.forms(L, nup, ndn, bonds, v1, v2)
    for a in (v1, v2, out):
        a.setflags(write=False)
    return v1, v2, out


def to_dev(a):
    return torch.from_numpy(np.array(a)).to(dev())      # (a copy: the cached case arrays are read-only)


def operator(name, p):
    L, nup, ndn, grid, bonds = GEOMETRY[name]
    op = HubbardOperator(L, bonds, to_dev(p), nup, ndn)
    if grid is not None:
        op.set_grid_log2(grid)
    return op


def relnorm(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def test_the_cases_are_what_the_table_says():
    shape = {name: (math.comb(g[0], g[1]), math.comb(g[0], g[2])) for name, g in GEOMETRY.items()}
    assert [shape[k] for k in GEOMETRY] == [(2, 2), (3, 3), (6, 4), (10, 10), (20, 20), (35, 21), (70, 70), (84, 126), (126, 84),
                                            (252, 252), (12, 12), (12, 12), (34, 34), (780, 40), (40, 780)]
    sizes = {name: a * b for name, (a, b) in shape.items()}
    assert [sizes[k] for k in GEOMETRY] == [4, 9, 24, 100, 400, 735, 4900, 10584, 10584, 63504, 144, 144, 1156, 31200, 31200]
    assert all(hubbard_dim(*GEOMETRY[k][:3]) == sizes[k] for k in GEOMETRY)
    assert GEOMETRY["L2-1-1"][4] == ((0, 1), (0, 1), (1, 0))
    for name in ("L3-1-2", "L4-2-1", "L5-2-3"):
        bonds = GEOMETRY[name][4]
        assert any((b, a) in bonds for a, b in bonds)
        assert shape[name][1] < 64 and GEOMETRY[name][1] != GEOMETRY[name][2]
    assert len(GEOMETRY["L6-3-3-loops"][4]) == 10
    assert (sizes["L6-3-3-loops"] + 255) // 256 == 2 and sizes["L6-3-3-loops"] % 256 != 0
    lo = (7 + 1) // 2                                    # the split of L = 7: sites 0 .. 3 low, 4 .. 6 high
    where = [(a < lo, b < lo) for a, b in GEOMETRY["L7-3-2-split"][4]]
    assert where == [(True, False), (False, False), (True, True), (True, False)]
    masks = [ref.between(a, b) for a, b in GEOMETRY["L7-3-2-split"][4]]
    assert masks == [0b0111110, 0, 0, 0b0001100]         # across the split, none, none, inside lo
    assert len(GEOMETRY["L8-4-4-complete"][4]) == 28 and shape["L8-4-4-complete"][1] % 64 != 0
    for name in ("L9-3-5-cap", "L9-5-3-cap"):
        assert len(GEOMETRY[name][4]) == CAP and len(set(GEOMETRY[name][4])) == 36
    assert len(GEOMETRY["L10-5-5-walk"][4]) == 24
    assert (sizes["L10-5-5-walk"] + 255) // 256 == 249 > (1 << GEOMETRY["L10-5-5-walk"][3]) == 64
    for name in ("L34-1-1", "L40-2-1", "L40-1-2"):
        L = GEOMETRY[name][0]
        assert len(GEOMETRY[name][4]) == L + 10 and (L - 1, 0) in GEOMETRY[name][4]
        assert max(ref.states(L, GEOMETRY[name][1])) >= 1 << 32
    assert ref.between(39, 0) == (1 << 39) - 2           # bits 1 .. 38


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_tables(name):
    L, nup, ndn, _, bonds = GEOMETRY[name]
    op = operator(name, couplings(L, bonds, "random"))
    n = hubbard_dim(L, nup, ndn)
    assert op.n == op.dim == n and op.nparam == 2 * len(bonds) + 2 * L
    Llo = (L + 1) // 2
    for tables, count in ((op._up, nup), (op._dn, ndn)):
        states, lo_rank, hi_base = (t.cpu() for t in tables)
        assert states.dtype == torch.int64
        assert torch.equal(states, torch.tensor(sector_states(L, count), dtype=torch.int64))
        assert lo_rank.shape == (1 << Llo,) and hi_base.shape == (1 << (L - Llo),)
        rank = hi_base[states >> Llo].to(torch.int64) + lo_rank[states & ((1 << Llo) - 1)].to(torch.int64)
        assert torch.equal(rank, torch.arange(states.numel(), dtype=torch.int64))
    assert torch.equal(op.up_states.cpu(), torch.tensor(sector_states(L, nup), dtype=torch.int64))
    assert torch.equal(op.dn_states.cpu(), torch.tensor(sector_states(L, ndn), dtype=torch.int64))
    assert (op._up is op._dn) == (nup == ndn)            # one table set serves both species at equal fillings
    rows = torch.arange(n, dtype=torch.int64, device=dev())
    u, d = op.up_states[rows // op.n_dn], op.dn_states[rows % op.n_dn]
    assert torch.equal(op.rank(u, d), rows)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_matvec_against_the_row_formula(name, kind):
    p, x, want = case(name, kind)
    n = x.size
    op = operator(name, p)
    xd = to_dev(x)
    got = op(xd).cpu().numpy()
    err = relnorm(got, want)
    print("%s %s: |y - ref| / |ref| = %.2e (bound 1e-13)" % (name, kind, err))
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
    print("    with shift: %.2e   x.y from the partials: %.2e (bounds 1e-13)" % (err_s, err_d))
    assert err_s < 1e-13
    assert err_d < 1e-13
    flag = torch.ones(1, dtype=F64, device=dev())
    sentinel = torch.full((n,), -7.0, dtype=F64, device=dev())
    _lib.check(lib.dsea_spmv(op.handle, ws.handle, _ptr(xd), _ptr(sentinel), _ptr(shift), None, _ptr(flag), _stream(dev())),
               "dsea_spmv")
    assert bool((sentinel == -7.0).all())


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_forms_against_the_reference_sums(name):
    L, nup, ndn, _, bonds = GEOMETRY[name]
    v1, v2, want = form_case(name)
    p = couplings(L, bonds, "random")
    op = operator(name, p)
    a, b = to_dev(v1), to_dev(v2)
    got = op.Hadjoint_to_couplingsadjoint(a, b)
    assert got.shape == (2 * len(bonds) + 2 * L,)
    norms = np.linalg.norm(v1) * np.linalg.norm(v2)
    bound = 1e-13 * norms
    err = float(np.max(np.abs(got.cpu().numpy() - want)))
    print("%s: max |form - ref| = %.2e (bound %.2e)" % (name, err, bound))
    assert err <= bound
    again = op.Hadjoint_to_couplingsadjoint(a, b)
    assert torch.equal(got, again)                       # fixed-order reductions, no atomics
    # H is linear in the couplings: v1^T H[p] v2 = sum_q p_q form_q.  Each form is within 1e-13 |v1| |v2| of its sum and the
    # mat-vec within 1e-13 |H v2| of its value (the two bounds above), so the two sides differ by at most
    # 1e-13 (|v1| |v2| sum_q |p_q| + |v1| |H v2|)
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


def test_to_csr_is_the_same_matrix():
    """L = 8 at (4, 4) with one mask listed twice more: equal masks are summed into one entry"""
    L, nup, ndn = 8, 4, 4
    bonds = tuple(lattice_reference.random_bonds(L, 12, 7708)) + ((3, 7), (7, 3), (3, 7))
    p = couplings(L, bonds, "random")
    op = HubbardOperator(L, bonds, to_dev(p), nup, ndn)
    n = op.n
    assert n == 4900
    v = torch.from_numpy(normal_vector(n, 8700)).to(dev())
    got = op(v)
    csr = op.to_csr()
    assert csr.n == n and csr.nnz == n + ref.moves(L, nup, ndn, bonds)
    want = ref.apply(L, nup, ndn, bonds, p, v.cpu().numpy())
    e1 = float((csr(v) - got).norm() / got.norm())
    e2 = relnorm(csr(v).cpu().numpy(), want)
    print("to_csr: against the matrix-free result %.2e, against the reference %.2e (bounds 1e-13)" % (e1, e2))
    assert e1 < 1e-13
    assert e2 < 1e-13


def test_couplings_changed_in_place_are_seen_without_a_new_operator():
    name = "L8-4-4-complete"
    L, nup, ndn, _, bonds = GEOMETRY[name]
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
    assert relnorm(op(xd).cpu().numpy(), ref.apply(L, nup, ndn, bonds, p + delta, x)) < 1e-13
    # pack / unpack: four views of the same storage, in the order of the parameter
    parts = op.unpack(op.couplings)
    assert [t.numel() for t in parts] == [28, 28, L, L]
    assert all(t.data_ptr() == op.couplings.data_ptr() + 8 * off for t, off in zip(parts, (0, 28, 56, 56 + L)))
    assert torch.equal(op.pack(*parts), op.couplings)
    assert op.pack(1.0, 0.5, 4.0, 0.0).tolist() == [1.0] * 28 + [0.5] * 28 + [4.0] * L + [0.0] * L
    # binding another tensor: a new handle on the same tables
    tables = [t.data_ptr() for t in op._up + op._dn]
    op.couplings = to_dev(p)
    assert [t.data_ptr() for t in op._up + op._dn] == tables
    assert relnorm(op(xd).cpu().numpy(), case(name, "random")[2]) < 1e-13
    with pytest.raises(ValueError):
        op.couplings = torch.zeros(p.size + 1, dtype=F64, device=dev())
    with pytest.raises(ValueError):
        op.couplings = torch.zeros(p.size, dtype=torch.float32, device=dev())
    with pytest.raises(ValueError):
        HubbardOperator(L, cyclic_complete(L, CAP + 1), torch.zeros(2 * (CAP + 1) + 2 * L, dtype=F64, device=dev()), nup, ndn)
    with pytest.raises(ValueError):
        HubbardOperator(L, ((0, 1), (4, 4)), torch.zeros(4 + 2 * L, dtype=F64, device=dev()), nup, ndn)
    with pytest.raises(ValueError):
        HubbardOperator(18, ((0, 1),), torch.zeros(2 + 36, dtype=F64, device=dev()), 9, 9)
    with pytest.raises(ValueError):
        HubbardOperator(L, ((0, 1),), torch.zeros(2 + 2 * L, dtype=F64, device=dev()), 0, ndn)


# ---- end to end ------------------------------------------------------------------------------------------------------
def one_particle_sum(p, bonds, L, nup, ndn):
    nb = len(bonds)
    h = np.diag(np.array(p[2 * nb + L:]))
    for k, (a, b) in enumerate(bonds):
        h[a, b] -= p[k]
        h[b, a] -= p[k]
    lam = np.linalg.eigvalsh(h)
    return float(lam[:nup].sum() + lam[:ndn].sum())


def test_free_fermions_on_the_device(monkeypatch):
    """U = V = 0 on the six-site lattice with loops at (3, 2): E0 = the lowest 3 plus the lowest 2 one-particle levels"""
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, nup, ndn, bonds = 6, 3, 2, LOOP_BONDS
    nb = len(bonds)
    p = np.zeros(2 * nb + 2 * L)
    p[:nb] = 1.0 + 0.3 * normal_vector(nb, 9100)
    p[2 * nb + L:] = 0.5 * normal_vector(L, 9101)
    op = HubbardOperator(L, bonds, to_dev(p), nup, ndn)
    n = op.n
    assert n == 300
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(9102):
        E0, _ = symeig.DominantSparseSymeig.apply(op.couplings, n, n)
    want = one_particle_sum(p, bonds, L, nup, ndn)
    err = abs(E0.item() - want) / abs(want)
    print("free fermions, six sites with loops, (3, 2): E0 = %.12f, one-particle sum %.12f, rel err %.2e (bound 1e-12)"
          % (E0.item(), want, err))
    assert err < 1e-12


E2E_L, E2E_NUP, E2E_NDN = 6, 3, 3
E2E_BONDS = tuple(ring_bonds(E2E_L, 1) + ring_bonds(E2E_L, 2))


@functools.lru_cache(maxsize=None)
def term_matrices(L, nup, ndn, bonds):
    """the 2 nb + 2 L matrices dH/dp_q as one (nparam, n, n) CPU tensor, from Kronecker products of the species' hop matrices"""
    n_up, n_dn = math.comb(L, nup), math.comb(L, ndn)
    bu, bd = ref._occupations(L, nup, ndn)
    occ = bu + bd
    up, dn = ref._partners(L, nup, bonds), ref._partners(L, ndn, bonds)
    hop, dens = [], []
    for k, (a, b) in enumerate(bonds):
        Su, Sd = np.zeros((n_up, n_up)), np.zeros((n_dn, n_dn))
        Su[up[k][0], up[k][1]] = up[k][2]
        Sd[dn[k][0], dn[k][1]] = dn[k][2]
        hop.append(-(np.kron(Su, np.eye(n_dn)) + np.kron(np.eye(n_up), Sd)))
        dens.append(np.diag((occ[a] * occ[b]).reshape(-1)))
    U = [np.diag((bu[i] * bd[i] * np.ones((n_up, n_dn))).reshape(-1)) for i in range(L)]
    eps = [np.diag((occ[i] * np.ones((n_up, n_dn))).reshape(-1)) for i in range(L)]
    return torch.from_numpy(np.array(hop + dens + U + eps))


def dense_torch(L, nup, ndn, bonds, p):
    """the dense matrix as a differentiable (linear) function of the flat couplings p (CPU)"""
    return torch.einsum("q,qij->ij", p, term_matrices(L, nup, ndn, bonds))


def hubbard_point(seed, U=4.0, noise=0.1):
    """(p0, dU, U): t = 1 on the ring and 0.3 on the next-nearest bonds, V = 0.5 on the ring and 0 beyond, eps = 0, U apart,
    plus random perturbations of all 2 nb + 2 L couplings (no symmetry and no degeneracy left); couplings = p0 + U dU"""
    L = E2E_L
    one, zero = torch.ones(L, dtype=F64), torch.zeros(L, dtype=F64)
    base = torch.cat([one, 0.3 * one, 0.5 * one, zero, zero, zero])
    dU = torch.cat([zero, zero, zero, zero, one, zero])
    p0 = base + noise * torch.from_numpy(normal_vector(base.numel(), seed).copy())
    return p0, dU, U


def test_dense_torch_is_the_reference_matrix_and_the_levels_are_apart():
    for seed in (9702, 9721):
        p0, dU, U = hubbard_point(seed)
        p = (p0 + U * dU).numpy()
        H = dense_torch(E2E_L, E2E_NUP, E2E_NDN, E2E_BONDS, torch.from_numpy(p)).numpy()
        assert H.shape == (400, 400)
        assert np.max(np.abs(H - ref.dense(E2E_L, E2E_NUP, E2E_NDN, E2E_BONDS, p))) < 1e-14 * np.max(np.abs(H))
        lam = np.linalg.eigvalsh(H)
        print("seed %d: E1 - E0 = %.3f   E2 - E1 = %.3f" % (seed, lam[1] - lam[0], lam[2] - lam[1]))
        assert lam[1] - lam[0] > 0.1 and lam[2] - lam[1] > 0.1


def test_ground_state_and_its_gradient_against_eigh(monkeypatch):
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, nup, ndn, bonds = E2E_L, E2E_NUP, E2E_NDN, E2E_BONDS
    n = k = 400
    p0, dU, U = hubbard_point(9702)
    p = p0 + U * dU
    u = unit(n, 9200)
    pr = p.clone().requires_grad_(True)
    lam, vecs = torch.linalg.eigh(dense_torch(L, nup, ndn, bonds, pr))
    assert lam[1] - lam[0] > 0.1 and lam[2] - lam[1] > 0.1
    (g_ref,) = torch.autograd.grad(lam[0] + (vecs[:, 0] @ u) ** 2, pr)
    op = HubbardOperator(L, bonds, p.to(dev()).requires_grad_(True), nup, ndn)
    assert op.n == n
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(9300):
        E0, psi = symeig.DominantSparseSymeig.apply(op.couplings, k, n)
        (g,) = torch.autograd.grad(E0 + (psi @ u.to(dev())) ** 2, op.couplings)
    assert engine.last_cg.converged
    e_err = abs(E0.item() - lam[0].item()) / abs(lam[0].item())
    g_err = float((g.cpu() - g_ref).abs().max()) / float(g_ref.abs().max())
    print("Hubbard ring with next-nearest hops, L = 6, (3, 3): E0 rel err %.2e (bound 1e-12)   d(E0 + (psi.u)^2)/d couplings: "
          "max abs err / max = %.2e (bound 1e-10)" % (e_err, g_err))
    assert g.shape == (36,)
    assert e_err < 1e-12
    assert g_err < TOL


def test_gap_and_its_gradient_through_the_lowest_two_levels(monkeypatch):
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, nup, ndn, bonds = E2E_L, E2E_NUP, E2E_NDN, E2E_BONDS
    n = k = 400
    p0, dU, U = hubbard_point(9702)
    p = p0 + U * dU
    pr = p.clone().requires_grad_(True)
    lam, _ = torch.linalg.eigh(dense_torch(L, nup, ndn, bonds, pr))
    gap_ref = lam[1] - lam[0]
    (g_ref,) = torch.autograd.grad(gap_ref, pr)
    op = HubbardOperator(L, bonds, p.to(dev()).requires_grad_(True), nup, ndn)
    symeig.setLowestSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(9500):
        vals, _ = symeig.LowestSparseSymeig.apply(op.couplings, k, n, 2)
        gap = vals[1] - vals[0]
        (g,) = torch.autograd.grad(gap, op.couplings)
    e_err = abs(vals[0].item() - lam[0].item()) / abs(lam[0].item())
    gap_err = abs(gap.item() - gap_ref.item()) / abs(gap_ref.item())
    g_err = float((g.cpu() - g_ref).abs().max()) / float(g_ref.abs().max())
    print("E0 rel err %.2e (bound 1e-12)   gap rel err %.2e   dgap/dcouplings max abs err / max = %.2e (bounds 1e-10)"
          % (e_err, gap_err, g_err))
    assert e_err < 1e-12
    assert gap_err < TOL
    assert g_err < TOL


def test_second_order_in_U(monkeypatch):
    """couplings = p0 + U dU: d^2 E0 / dU^2 through the re-entrant mat-vec / forms pair against eigh double backward, at the
    tolerances of the second-order tests of tests/test_gpu_sector.py and tests/test_gpu_lattice.py"""
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, nup, ndn, bonds = E2E_L, E2E_NUP, E2E_NDN, E2E_BONDS
    n = k = 400
    p0, dU, U = hubbard_point(9721)
    tr = torch.tensor(U, dtype=F64, requires_grad=True)
    lam, _ = torch.linalg.eigh(dense_torch(L, nup, ndn, bonds, p0 + tr * dU))
    assert lam[1] - lam[0] > 0.1 and lam[2] - lam[1] > 0.1
    (r1,) = torch.autograd.grad(lam[0], tr, create_graph=True)
    (r2,) = torch.autograd.grad(r1, tr)
    t = torch.tensor(U, dtype=F64, device=dev(), requires_grad=True)
    op = HubbardOperator(L, bonds, (p0.to(dev()) + t * dU.to(dev())), nup, ndn)
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(9400):
        E0, _ = symeig.DominantSparseSymeig.apply(op.couplings, k, n)
        (g1,) = torch.autograd.grad(E0, t, create_graph=True)
        (g2,) = torch.autograd.grad(g1, t)
    e1 = abs(g1.item() - r1.item()) / abs(r1.item())
    e2 = abs(g2.item() - r2.item()) / abs(r2.item())
    print("dE0/dU rel err %.2e (bound 1e-10)   d2E0/dU2 rel err %.2e (bound 1e-8)  (%.6f vs %.6f)"
          % (e1, e2, g2.item(), r2.item()))
    assert e1 < TOL
    assert e2 < 1e-8


def test_two_sites_closed_form_through_the_primitive(monkeypatch):
    """one up and one down fermion on two sites at U = 4, t = 1: E0 = (U - sqrt(U^2 + 16 t^2)) / 2 and
    dE0/dU = (1 - U / sqrt(U^2 + 16 t^2)) / 2, the double occupancy"""
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    U0, t0 = 4.0, 1.0
    U = torch.tensor(U0, dtype=F64, device=dev(), requires_grad=True)
    base = torch.tensor([t0, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=F64, device=dev())
    dU = torch.tensor([0.0, 0.0, 1.0, 1.0, 0.0, 0.0], dtype=F64, device=dev())
    op = HubbardOperator(2, [(0, 1)], base + U * dU, 1, 1)
    assert op.n == 4
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(9800):
        E0, _ = symeig.DominantSparseSymeig.apply(op.couplings, 4, 4)
        (g,) = torch.autograd.grad(E0, U)
    root = math.sqrt(U0 * U0 + 16.0 * t0 * t0)
    want, dwant = 0.5 * (U0 - root), 0.5 * (1.0 - U0 / root)
    e_err, g_err = abs(E0.item() - want) / abs(want), abs(g.item() - dwant) / abs(dwant)
    print("two sites: E0 rel err %.2e (bound 1e-12)   dE0/dU rel err %.2e (bound 1e-10)" % (e_err, g_err))
    assert e_err < 1e-12
    assert g_err < TOL


def test_example_ring():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "hubbard", "ring.py")
    spec = importlib.util.spec_from_file_location("hubbard_ring", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    orig = CG.EPS_DEFAULT
    try:
        out = ex.main(L=6)
        two = ex.main(L=2)
        h = 1e-4
        fd = (ex.energy(6, out["U_grad"] + h, device=dev()) - ex.energy(6, out["U_grad"] - h, device=dev())) / (2 * h)
    finally:
        CG.EPS_DEFAULT = orig
    print("L = 6: double occupancy per site %.12f (autograd) %.12f (forms)   dE0/dU %.9f   central difference %.9f   "
          "d2E0/dU2 %.9f" % (out["docc_autograd"], out["docc_forms"], out["dE0_dU"], fd, out["d2E0_dU2"]))
    assert out["n"] == 400 and out["L"] == 6 and two["n"] == 4
    assert len(out["E0"]) == len(out["U"]) and all(a < b for a, b in zip(out["E0"], out["E0"][1:]))   # E0 grows with U
    assert abs(out["docc_autograd"] - out["docc_forms"]) < 1e-10
    assert abs(two["docc_autograd"] - two["docc_forms"]) < 1e-10
    assert abs(out["dE0_dU"] - 6 * out["docc_autograd"]) < 1e-10
    assert abs(out["dE0_dU"] - fd) < 1e-5
    assert out["d2E0_dU2"] < 0.0                                   # E0 is concave in a parameter that enters linearly
    for res in (out, two):
        assert abs(res["E0_two_site"] - res["E0_two_site_closed"]) < 1e-12 * abs(res["E0_two_site_closed"])
    U0 = two["U_grad"]
    assert abs(two["E0_at_U_grad"] - 0.5 * (U0 - math.sqrt(U0 * U0 + 16.0))) < 1e-12 * abs(two["E0_at_U_grad"])
