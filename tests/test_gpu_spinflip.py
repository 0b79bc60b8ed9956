"""Spin inversion in the symmetry sector on the GPU (docs/design/23-spin-inversion.md): k_symsector_classify_flip,
k_spmv_symsector_flip and k_symsector_forms_flip (+ reduce) against the numpy reference of tests/spinflip_reference.py, and the
primitives end to end against torch.linalg.eigh autograd.  Tolerances are those of tests/test_gpu_symsector.py.

    case (z = +1 / -1)   |G|   n_sector   n            what it reaches
    flip-L8              2     70         35 / 35      NGL = 1, the flip alone: every site has eps = 0
    ring8                32    70         7 / 1        NGL = 2, a sector of one row
    ring12-j1j2          48    924        13 / 27      NGL = 4, |G| no multiple of 16, two bond orbits
    ring10-TF            10    252        30 / 22      NGL = 1, the combined element T F: eps = +-1, a staggered field acts
    ring14-TF            14    3432       256 / 236    NGL = 1, 16 full ranges of 16 rows at z = +1
    K16-D16              64    12 870     158 / 212    NGL = 4 with every slot used, 120 bonds: 8 chunks, the last one ragged
    torus4x4-c4          128   12 870     149 / 82     NGL = 8, the cap on |G|
    ring20               80    184 756    2518 / 2234  NGL = 8; with the grid capped at 64 blocks, blocks walk and the last team
                                                       is partial (2518 > 64 * 16, 2518 % 16 != 0)
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sector_reference as sec  # noqa: E402
import spinflip_reference as ref  # noqa: E402
from helpers import PatchRandn, unit  # noqa: E402
from dominantsparseeigenad_amd import _lib, engine  # noqa: E402
from dominantsparseeigenad_amd.engine import Workspace, _ptr, _stream  # noqa: E402
from dominantsparseeigenad_amd.operators import (SpinSectorOperator, SpinSymmetrySectorOperator, ring_bonds,  # noqa: E402
                                                 ring_symmetries, spin_inversion)
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402
import dominantsparseeigenad_amd.symeig as symeig  # noqa: E402
import dominantsparseeigenad_amd.CG as CG  # noqa: E402

F64 = torch.float64
TOL = 1e-10
# (name, z, log2 of the grid cap or None for the default)
CASES = [(name, z, None) for name, z in ref.CASES] + [("ring20", 1, 6)]
IDS = ["%s-z%+d%s" % (name, z, "" if grid is None else "-walk") for name, z, grid in CASES]
KINDS = ["random", "jxy-only"]


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


def couplings(case, kind, seed=8000):
    p = normal_vector(2 * case.nb + case.L, seed + case.L + case.nb).copy()
    if kind == "jxy-only":
        p[case.nb:] = 0.0
    return p


@functools.lru_cache(maxsize=None)
def matvec_case(name, z, kind):
    """(couplings, x, H x) on the host, computed once per case and never written to"""
    case = ref.case(name, z)
    p = couplings(case, kind)
    x = normal_vector(case.basis.n, 8100 + case.L + case.ndown)
    y = ref.apply(case, p, x)
    for a in (p, x, y):
        a.setflags(write=False)
    return p, x, y


@functools.lru_cache(maxsize=None)
def form_case(name, z):
    case = ref.case(name, z)
    n = case.basis.n
    v1, v2 = normal_vector(n, 8200 + case.L + case.ndown), normal_vector(n, 8300 + case.L + case.ndown)
    out = ref.forms(case, v1, v2)
    for a in (v1, v2, out):
        a.setflags(write=False)
    return v1, v2, out


def to_dev(a):
    return torch.from_numpy(np.array(a)).to(dev())      # (a copy: the cached case arrays are read-only)


def operator(name, z, p, grid=None):
    L, ndown, bonds, gens = ref.geometry(name, z)
    op = SpinSymmetrySectorOperator(L, bonds, to_dev(p), ndown, gens)
    if grid is not None:
        op.set_grid_log2(grid)
    return op


def relnorm(a, b):
    """|a - b| / |b|; where the reference is exactly 0 the absolute |a|"""
    scale = np.linalg.norm(np.asarray(b))
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / (scale if scale > 0.0 else 1.0))


def test_the_cases_are_what_the_table_says():
    for name, (ng, n_sector, orbits, zero, n) in ref.TABLE.items():
        for k, z in enumerate((1, -1)):
            b = ref.case(name, z).basis
            assert (len(ref.case(name, z).group), b.n_sector, b.orbits, b.zero_norm, b.n) == (ng, n_sector, orbits, zero[k], n[k])
    ngl = {name: (row[0] + 15) // 16 for name, row in ref.TABLE.items()}
    assert ngl == {"flip-L8": 1, "ring8": 2, "ring12-j1j2": 3, "ring10-TF": 1, "ring14-TF": 1, "K16-D16": 4, "torus4x4-c4": 8,
                   "ring20": 5}                                            # (3 runs as NGL = 4, 5 as NGL = 8)
    walk = ref.case("ring20", 1).basis.n
    assert (walk + 15) // 16 > (1 << 6) and walk % 16 != 0


@pytest.mark.parametrize("name,z", ref.CASES)
def test_tables(name, z):
    case = ref.case(name, z)
    b = case.basis
    op = operator(name, z, couplings(case, "random"))
    assert op.n == op.dim == b.n and op.n_sector == b.n_sector and op.ng == len(case.group)
    assert tuple(op.group) == case.group and tuple(op.orbits) == case.orbit
    assert op.flips == case.flips and all(isinstance(f, bool) for f in op.flips)
    assert tuple(op.site_signs) == case.eps
    assert op.states.dtype == torch.int64 and torch.equal(op.states.cpu(), torch.from_numpy(np.array(b.reps)))
    assert torch.equal(op.norms.cpu(), torch.from_numpy(np.array(b.sigma)))
    reps, bucket, perm_tab = (t.cpu() for t in op._tables)
    assert torch.equal(reps, torch.from_numpy(np.array(b.reps | (b.sigma << 48))))
    assert torch.equal(bucket.to(torch.int64), torch.from_numpy(np.array(b.bucket)))
    assert torch.equal(perm_tab, torch.from_numpy(b.tab.reshape(-1)))      # the permutation alone
    assert torch.equal(op.row_of(op.states).cpu(), torch.arange(b.n, dtype=torch.int64))
    assert op.row_of(torch.tensor([0, (1 << case.L) - 1], dtype=torch.int64)).tolist() == [-1, -1]
    some = op.states[:64]
    assert torch.equal(op._images(some).cpu(), torch.from_numpy(ref.images(b.tab, b.flips, case.L, b.reps[:64])))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,z,grid", CASES, ids=IDS)
def test_matvec_against_the_row_formula(name, z, grid, kind):
    p, x, want = matvec_case(name, z, kind)
    n = x.size
    op = operator(name, z, p, grid)
    xd = to_dev(x)
    got = op(xd)
    err = relnorm(got.cpu().numpy(), want)
    print("%s z=%+d %s: |y - ref| / |ref| = %.2e" % (name, z, kind, err))
    assert err < 1e-13
    assert torch.equal(op(xd), got)                      # no atomics: two calls return identical bits
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


@pytest.mark.parametrize("name,z,grid", CASES, ids=IDS)
def test_forms_against_the_reference_sums(name, z, grid):
    case = ref.case(name, z)
    nb = case.nb
    v1, v2, want = form_case(name, z)
    p = couplings(case, "random")
    op = operator(name, z, p, grid)
    a, b = to_dev(v1), to_dev(v2)
    got = op.Hadjoint_to_couplingsadjoint(a, b)
    assert got.shape == (2 * nb + case.L,)
    norms = np.linalg.norm(v1) * np.linalg.norm(v2)
    bound = 1e-13 * norms
    err = float(np.max(np.abs(got.cpu().numpy() - want)))
    print("%s z=%+d: max |form - ref| = %.2e (bound %.2e)" % (name, z, err, bound))
    assert err <= bound
    assert torch.equal(got, op.Hadjoint_to_couplingsadjoint(a, b))       # fixed-order reductions, no atomics
    swapped = op.Hadjoint_to_couplingsadjoint(b, a)
    assert float((swapped - got).abs().max()) <= bound
    host = got.cpu().numpy()
    for o in set(case.orbit):
        members = [c for c, oc in enumerate(case.orbit) if oc == o]
        if members[0] < 2 * nb:
            assert len({host[c].tobytes() for c in members}) == 1       # bond orbits: identical bits
        else:
            # site orbits: identical up to the sign, bit for bit, and exactly 0.0 where eps = 0
            signs = [case.eps[c - 2 * nb] for c in members]
            if signs[0] == 0:
                assert all(host[c].tobytes() == np.float64(0.0).tobytes() for c in members)
            else:
                assert len({np.float64(e * host[c]).tobytes() for e, c in zip(signs, members)}) == 1
    # H is linear in the couplings: v1^T H[p] v2 = sum_t p_t form_t
    Hv2 = op(b)
    lhs, rhs = float(a @ Hv2), float(np.sum(p * host))
    assert abs(lhs - rhs) <= 1e-13 * (norms * np.abs(p).sum() + np.linalg.norm(v1) * float(Hv2.norm()))


@pytest.mark.parametrize("name,z", ref.CASES)
def test_matvec_is_symmetric_and_sees_the_couplings_through_S(name, z):
    case = ref.case(name, z)
    p, x, _ = matvec_case(name, z, "random")
    op = operator(name, z, p)
    a = to_dev(x)
    b = torch.from_numpy(normal_vector(x.size, 8400 + x.size % 97)).to(dev())
    Ha, Hb = op(a), op(b)
    assert abs(float(a @ Hb) - float(Ha @ b)) <= 1e-13 * float(a.norm() * Hb.norm() + b.norm() * Ha.norm())
    pbar = case.pbar(p)
    assert np.max(np.abs(pbar - p)) > 0.0
    assert float((operator(name, z, pbar)(a) - Ha).norm()) <= 1e-13 * float(Ha.norm())
    assert float((op.symmetrise(op.couplings).cpu() - torch.from_numpy(pbar)).abs().max()) < 1e-14 * np.max(np.abs(p)) * 16


@pytest.mark.parametrize("name,z", [("ring12-j1j2", -1), ("ring10-TF", 1), ("ring10-TF", -1), ("K16-D16", 1), ("torus4x4-c4", -1)])
def test_expand_commutes_with_the_sector_operator(name, z):
    """SpinSectorOperator(pbar).H(expand(x)) = expand(H_sym x): B B^T commutes with H(pbar)"""
    L, ndown, bonds, gens = ref.geometry(name, z)
    case = ref.case(name, z)
    p, x, _ = matvec_case(name, z, "random")
    sym = operator(name, z, p)
    full = SpinSectorOperator(L, bonds, to_dev(case.pbar(p)), ndown)
    xd = to_dev(x)
    w = sym.expand(xd)
    assert w.shape == (full.n,) and abs(float(w.norm()) - float(xd.norm())) < 1e-13 * float(xd.norm())
    lhs, rhs = full(w), sym.expand(sym(xd))
    assert float((lhs - rhs).norm()) < 1e-13 * float(rhs.norm())


@pytest.mark.parametrize("name,z", [("flip-L8", -1), ("ring12-j1j2", 1), ("ring10-TF", -1), ("torus4x4-c4", 1)])
def test_to_csr(name, z):
    p, x, want = matvec_case(name, z, "random")
    op = operator(name, z, p)
    csr = op.to_csr()
    xd = to_dev(x)
    got = op(xd)
    assert csr.n == op.n
    assert float((csr(xd) - got).norm() / got.norm()) < 1e-13
    assert relnorm(csr(xd).cpu().numpy(), want) < 1e-13


@pytest.mark.parametrize("z", [1, -1])
def test_a_staggered_field_acts_in_the_TF_sector(z):
    """hz = staggered field + noise breaks T and F and keeps T F: the dense B^T H(p) B shows that the field acts"""
    name = "ring10-TF"
    case = ref.case(name, z)
    nb = case.nb
    p = couplings(case, "random")
    p[2 * nb:] = 0.8 * np.array([(-1) ** i for i in range(case.L)]) + 0.1 * normal_vector(case.L, 8500)
    x = normal_vector(case.basis.n, 8510)
    A = ref.dense_sym(case, p)
    p0 = p.copy()
    p0[2 * nb:] = 0.0
    want, without = A @ x, ref.dense_sym(case, p0) @ x
    assert np.linalg.norm(want - without) > 0.1 * np.linalg.norm(want)
    got = operator(name, z, p)(to_dev(x)).cpu().numpy()
    assert relnorm(got, want) < 1e-13
    assert relnorm(got, ref.apply(case, p, x)) < 1e-13


def test_a_group_without_flips_takes_the_path_of_before():
    """generators written (perm, char, False) give the bits of the (perm, char) form: the same entry points, the same kernels"""
    L, ndown = 12, 6
    bonds = tuple(ring_bonds(L, 1) + ring_bonds(L, 2))
    gens = ring_symmetries(L, "pi", -1)
    p = to_dev(normal_vector(2 * len(bonds) + L, 8700).copy())
    old = SpinSymmetrySectorOperator(L, bonds, p, ndown, gens)
    new = SpinSymmetrySectorOperator(L, bonds, p, ndown, [g + (False,) for g in gens])
    assert new.group == old.group and new.flips == (False,) * 24 and new.site_signs == (1,) * L
    assert all(torch.equal(a, b) for a, b in zip(old._tables, new._tables))
    x, x2 = to_dev(normal_vector(old.n, 8710)), to_dev(normal_vector(old.n, 8720))
    assert torch.equal(old(x), new(x))
    assert torch.equal(old.Hadjoint_to_couplingsadjoint(x, x2), new.Hadjoint_to_couplingsadjoint(x, x2))
    assert torch.equal(old.symmetrise(p), new.symmetrise(p))


def test_validation_errors():
    L, bonds = 8, ring_bonds(8)
    zeros = torch.zeros(3 * L, dtype=F64, device=dev())
    with pytest.raises(ValueError, match="ndown = L / 2"):
        SpinSymmetrySectorOperator(L, bonds, zeros, 3, [spin_inversion(L, 1)])
    with pytest.raises(ValueError, match="consistent"):
        SpinSymmetrySectorOperator(L, bonds, zeros, 4, [spin_inversion(L, 1), spin_inversion(L, -1)])
    with pytest.raises(ValueError, match="flip"):
        SpinSymmetrySectorOperator(L, bonds, zeros, 4, [(tuple(range(L)), 1, 2)])
    with pytest.raises(ValueError, match="empty"):
        # two sites, one down spin: the single orbit {01, 10} is fixed by R F, whose character is -1
        SpinSymmetrySectorOperator(2, [(0, 1)], torch.zeros(4, dtype=F64, device=dev()), 1, [((1, 0), 1), spin_inversion(2, -1)])


# ---- end to end ------------------------------------------------------------------------------------------------------
E2E_L, E2E_NDOWN = 12, 6
E2E_BONDS = tuple(ring_bonds(E2E_L, 1) + ring_bonds(E2E_L, 2))
E2E_SECTORS = [(k, p, z) for k, p in [(0, 1), (0, -1), ("pi", 1), ("pi", -1)] for z in (1, -1)]


def dense_torch(L, ndown, bonds, p):
    """the dense full-sector matrix as a differentiable function of the flat couplings p (CPU)"""
    nb = len(bonds)
    n = len(sec.states(L, ndown))
    r = torch.arange(n, dtype=torch.int64)
    H = torch.zeros((n, n), dtype=F64)
    for i, z in enumerate(sec._z(L, ndown)):
        H = H.index_put((r, r), p[2 * nb + i] * torch.from_numpy(np.array(z)), accumulate=True)
    for t, (rows, cols, zz) in enumerate(sec._partners(L, ndown, bonds)):
        H = H.index_put((r, r), p[nb + t] * torch.from_numpy(np.array(zz)), accumulate=True)
        H = H.index_put((torch.from_numpy(np.array(rows)), torch.from_numpy(np.array(cols))), (2.0 * p[t]).expand(rows.size),
                        accumulate=True)
    return H


@functools.lru_cache(maxsize=None)
def e2e_case(gens):
    case = ref.Case(E2E_L, E2E_NDOWN, E2E_BONDS, gens)
    return case, torch.from_numpy(ref.dense_B(case))


def sector_gens(sector):
    return tuple(ring_symmetries(E2E_L, *sector))


def dense_sym_torch(gens, p):
    """B^T H(p) B with B constant and p the leaf: the couplings enter as they are, not through their means"""
    _, B = e2e_case(gens)
    return B.T @ dense_torch(E2E_L, E2E_NDOWN, E2E_BONDS, p) @ B


def j1j2_point(seed, J2=0.3, noise=0.1):
    """(p0, d2, J2): couplings = p0 + J2 d2; p0 = the J1 part plus random perturbations of all 2 nb + L couplings, which are
    not invariant under the group"""
    L = E2E_L
    near = torch.cat([torch.ones(L, dtype=F64), torch.zeros(L, dtype=F64)])
    nxt = torch.cat([torch.zeros(L, dtype=F64), torch.ones(L, dtype=F64)])
    field = torch.zeros(L, dtype=F64)
    d1, d2 = torch.cat([near, near, field]), torch.cat([nxt, nxt, field])
    p0 = d1 + noise * torch.from_numpy(normal_vector(d1.numel(), seed).copy())
    return p0, d2, J2


def sym_operator(gens, p):
    return SpinSymmetrySectorOperator(E2E_L, E2E_BONDS, p, E2E_NDOWN, list(gens))


def test_the_e2e_sectors_have_the_pinned_rows():
    assert [e2e_case(sector_gens(s))[0].basis.n for s in E2E_SECTORS] == [35, 15, 9, 21, 29, 11, 13, 27]


@pytest.mark.parametrize("sector", E2E_SECTORS)
def test_ground_state_and_gradient_against_eigh(sector, monkeypatch):
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    gens = sector_gens(sector)
    case, _ = e2e_case(gens)
    n = k = case.basis.n
    p0, d2, J2 = j1j2_point(9702)
    p = p0 + J2 * d2
    u = unit(n, 9200)
    pr = p.clone().requires_grad_(True)
    lam, U = torch.linalg.eigh(dense_sym_torch(gens, pr))
    (g_ref,) = torch.autograd.grad(lam[0] + (U[:, 0] @ u) ** 2, pr)
    op = sym_operator(gens, p.to(dev()).requires_grad_(True))
    assert op.n == n
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(9300):
        E0, psi = symeig.DominantSparseSymeig.apply(op.couplings, k, n)
        (g,) = torch.autograd.grad(E0 + (psi @ u.to(dev())) ** 2, op.couplings)
    assert engine.last_cg.converged
    e_err = abs(E0.item() - lam[0].item()) / abs(lam[0].item())
    g_err = float((g.cpu() - g_ref).abs().max()) / float(g_ref.abs().max())
    print("sector %s, n = %d: E0 rel err %.2e   d(E0 + (psi.u)^2)/d couplings: max abs err / max = %.2e" % (sector, n, e_err, g_err))
    assert g.shape == (2 * 24 + 12,)
    assert e_err < 1e-12
    assert g_err < TOL
    assert not g[2 * 24:].any()                          # G contains F: the field gradient is exactly 0


@pytest.mark.parametrize("sector", E2E_SECTORS)
def test_second_order_in_J2(sector, monkeypatch):
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    gens = sector_gens(sector)
    case, _ = e2e_case(gens)
    n = k = case.basis.n
    p0, d2, J2 = j1j2_point(9721)
    tr = torch.tensor(J2, dtype=F64, requires_grad=True)
    lam, _ = torch.linalg.eigh(dense_sym_torch(gens, p0 + tr * d2))
    (r1,) = torch.autograd.grad(lam[0], tr, create_graph=True)
    (r2,) = torch.autograd.grad(r1, tr)
    t = torch.tensor(J2, dtype=F64, device=dev(), requires_grad=True)
    op = sym_operator(gens, p0.to(dev()) + t * d2.to(dev()))
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(9400):
        E0, _ = symeig.DominantSparseSymeig.apply(op.couplings, k, n)
        (g1,) = torch.autograd.grad(E0, t, create_graph=True)
        (g2,) = torch.autograd.grad(g1, t)
    e1 = abs(g1.item() - r1.item()) / abs(r1.item())
    e2 = abs(g2.item() - r2.item()) / abs(r2.item())
    print("sector %s: dE0/dJ2 rel err %.2e   d2E0/dJ2^2 rel err %.2e  (%.6f vs %.6f)" % (sector, e1, e2, g2.item(), r2.item()))
    assert e1 < TOL
    assert e2 < 1e-8


def flip_gens(z):
    return (spin_inversion(E2E_L, z),)


def gpu_gap(p0, d2, t, seed):
    """E0(z = -1) - E0(z = +1) through two DominantSparseSymeig solves, a function of the device scalar t = J2"""
    E = {}
    for z in (1, -1):
        op = sym_operator(flip_gens(z), p0.to(dev()) + t * d2.to(dev()))
        assert op.n == 462
        symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
        with PatchRandn(seed + z):
            E[z], _ = symeig.DominantSparseSymeig.apply(op.couplings, 300, op.n)
    return E[-1] - E[1]


def test_the_gap_is_that_of_the_full_sector(monkeypatch):
    """clean Heisenberg ring (J2 = 0): the lowest singlet has z = +1, the lowest triplet z = -1"""
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    p0, d2, _ = j1j2_point(0, noise=0.0)
    full = torch.linalg.eigvalsh(dense_torch(E2E_L, E2E_NDOWN, E2E_BONDS, p0))
    want = (full[1] - full[0]).item()
    assert abs(want - 1.42339006) < 1e-8
    gap = gpu_gap(p0, d2, torch.tensor(0.0, dtype=F64, device=dev()), 9900).item()
    print("gap %.10f, E1 - E0 of the full sector %.10f" % (gap, want))
    assert abs(gap - want) < TOL * abs(want)


def test_the_gap_is_differentiable_to_second_order(monkeypatch):
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    p0, d2, J2 = j1j2_point(9731)
    tr = torch.tensor(J2, dtype=F64, requires_grad=True)
    lam = {z: torch.linalg.eigvalsh(dense_sym_torch(flip_gens(z), p0 + tr * d2)) for z in (1, -1)}
    ref_gap = lam[-1][0] - lam[1][0]
    (r1,) = torch.autograd.grad(ref_gap, tr, create_graph=True)
    (r2,) = torch.autograd.grad(r1, tr)
    t = torch.tensor(J2, dtype=F64, device=dev(), requires_grad=True)
    gap = gpu_gap(p0, d2, t, 9910)
    (g1,) = torch.autograd.grad(gap, t, create_graph=True)
    (g2,) = torch.autograd.grad(g1, t)
    e0 = abs(gap.item() - ref_gap.item()) / abs(ref_gap.item())
    e1 = abs(g1.item() - r1.item()) / abs(r1.item())
    e2 = abs(g2.item() - r2.item()) / abs(r2.item())
    print("gap rel err %.2e   dgap/dJ2 rel err %.2e   d2gap/dJ2^2 rel err %.2e  (%.6f vs %.6f)" % (e0, e1, e2, g2.item(), r2.item()))
    assert e0 < TOL
    assert e1 < TOL
    assert e2 < 1e-8


def test_example_spin_gap():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "spin_lattice", "spin_gap.py")
    spec = importlib.util.spec_from_file_location("spin_lattice_spin_gap", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    orig = CG.EPS_DEFAULT
    try:
        out = ex.main(L=12)
    finally:
        CG.EPS_DEFAULT = orig
    p0, d2, _ = j1j2_point(0, noise=0.0)

    def full_sector_gap(J2):
        """(E1 - E0, its J2 derivative) of the full S^z = 0 sector by dense eigh (first order: the spectrum has degenerate
        levels elsewhere, which the second derivative of eigh does not survive)"""
        tr = torch.tensor(J2, dtype=F64, requires_grad=True)
        full = torch.linalg.eigvalsh(dense_torch(E2E_L, E2E_NDOWN, E2E_BONDS, p0 + tr * d2))
        (w1,) = torch.autograd.grad(full[1] - full[0], tr)
        return (full[1] - full[0]).item(), w1.item()

    h = 1e-4
    want, w1 = full_sector_gap(out["J2"])
    w2 = (full_sector_gap(out["J2"] + h)[1] - full_sector_gap(out["J2"] - h)[1]) / (2 * h)     # (error O(h^2))
    print("gap %.9f (%.9f)  dgap/dJ2 %.9f (%.9f)  d2gap/dJ2^2 %.7f (%.7f)" % (out["gap"], want, out["dgap_dJ2"], w1,
                                                                            out["d2gap_dJ2"], w2))
    assert out["n_full"] == 924 and out["n"] == [44, 38]
    assert abs(out["gap"] - want) < TOL * abs(want)
    assert abs(out["dgap_dJ2"] - w1) < TOL * abs(w1)
    assert abs(out["d2gap_dJ2"] - w2) < 1e-5 * abs(w2)
