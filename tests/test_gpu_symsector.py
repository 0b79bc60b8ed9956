"""XXZ spins in a lattice-symmetry sector on the GPU (docs/design/20-symmetry-sector.md): the table builders, k_spmv_symsector and
k_symsector_forms against the numpy reference of tests/symsector_reference.py at the smallest sizes that reach each path, the
fixed-magnetisation operator as a cross-check, and the primitives end to end against torch.linalg.eigh autograd.

    case                     |G|   n_sector  n_rep    what it reaches
    the ten rows of symsector_reference.TABLE            zero-norm orbits, non-trivial stabilisers, dropped hops (pinned counts)
    identity-L11             1     462       462      reduces to SpinSectorOperator (20 random bonds)
    ring7-k0                 7     35        5        |G| < 16: padded group slots
    ring12-kpi-p-1           24    924       40       |G| no multiple of 16
    torus4x4-full            128   12 870    (ref)    the cap on |G|: translations, C4 and a mirror
    K16-D16                  32    12 870    (ref)    120 bonds: 8 chunks of 16, the last one ragged
    ring34-nd2  ring40-nd2   34 80 561 780   (ref)    states wider than 32 bits, 5 byte slices
    ring22-k0-walk           22    705 432   32 066   2005 ranges of 16 rows on a grid capped at 64 blocks: blocks walk
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lattice_reference  # noqa: E402
import sector_reference as sec  # noqa: E402
import symsector_reference as ref  # noqa: E402
from helpers import PatchRandn, unit  # noqa: E402
from dominantsparseeigenad_amd import _lib, engine  # noqa: E402
from dominantsparseeigenad_amd.engine import Workspace, _ptr, _stream  # noqa: E402
from dominantsparseeigenad_amd.operators import (SpinSectorOperator, SpinSymmetrySectorOperator, ring_bonds,  # noqa: E402
                                                 ring_symmetries)
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402
import dominantsparseeigenad_amd.symeig as symeig  # noqa: E402
import dominantsparseeigenad_amd.CG as CG  # noqa: E402

F64 = torch.float64
TOL = 1e-10


def distinct_random_bonds(L, count, seed):
    seen, out = set(), []
    for a, b in lattice_reference.random_bonds(L, 8 * count, seed):
        if frozenset((a, b)) not in seen:
            seen.add(frozenset((a, b)))
            out.append((a, b))
    return tuple(out[:count])


# name -> (L, ndown, log2 of the grid cap or None for the default, bonds, generators)
GEOMETRY = {name: (args[0], args[1], None, args[2], args[3]) for name, (args, _) in ref.TABLE.items()}
GEOMETRY.update({
    "identity-L11": (11, 5, None, distinct_random_bonds(11, 20, 7411), ()),
    "torus4x4-full": (16, 8, None, tuple(ref.square(4, 4)),
                      ((ref.torus_tx(4, 4), 1), (ref.torus_ty(4, 4), 1), (ref.square_rot(4), 1), (ref.square_mirror(4), 1))),
    "K16-D16": (16, 8, None, tuple(lattice_reference.complete_bonds(16)), ((ref.translation(16), 1), (ref.reflection(16), -1))),
    "ring34-nd2": (34, 2, None, tuple(ref.ring(34)), ((ref.translation(34), -1),)),
    "ring40-nd2": (40, 2, None, tuple(ref.ring(40)), ((ref.translation(40), 1), (ref.reflection(40), 1))),
    "ring22-k0-walk": (22, 11, 6) + ref.TABLE["ring22-k0"][0][2:],
})
KINDS = ["random", "jxy-only"]


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def geometry(name):
    L, ndown, _, bonds, gens = GEOMETRY[name]
    return ref.Case(L, ndown, bonds, gens)


def couplings(case, kind, seed=8000):
    p = normal_vector(2 * case.nb + case.L, seed + case.L + case.nb).copy()
    if kind == "jxy-only":
        p[case.nb:] = 0.0
    return p


@functools.lru_cache(maxsize=None)
def matvec_case(name, kind):
    """(couplings, x, H x) on the host, computed once per case and never written to"""
    case = geometry(name)
    p = couplings(case, kind)
    x = normal_vector(case.basis.n, 8100 + case.L + case.ndown)
    y = ref.apply(case, p, x)
    for a in (p, x, y):
        a.setflags(write=False)
    return p, x, y


@functools.lru_cache(maxsize=None)
def form_case(name):
    case = geometry(name)
    n = case.basis.n
    v1, v2 = normal_vector(n, 8200 + case.L + case.ndown), normal_vector(n, 8300 + case.L + case.ndown)
    out = ref.forms(case, v1, v2)
    for a in (v1, v2, out):
        a.setflags(write=False)
    return v1, v2, out


def to_dev(a):
    return torch.from_numpy(np.array(a)).to(dev())      # (a copy: the cached case arrays are read-only)


def operator(name, p):
    L, ndown, grid, bonds, gens = GEOMETRY[name]
    op = SpinSymmetrySectorOperator(L, bonds, to_dev(p), ndown, gens)
    if grid is not None:
        op.set_grid_log2(grid)
    return op


def relnorm(a, b):
    """|a - b| / |b|; where the reference is exactly 0 (a sector all of whose hops are dropped, Jxy only) the absolute |a|"""
    scale = np.linalg.norm(np.asarray(b))
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / (scale if scale > 0.0 else 1.0))


def test_the_cases_are_what_the_table_says():
    for name, (_, want) in ref.TABLE.items():
        case = geometry(name)
        b = case.basis
        assert (len(case.group), b.n_sector, b.orbits, b.n, b.zero_norm, b.nontrivial) == want
    for name, want in ref.HOPS.items():
        assert (geometry(name).n_hops, geometry(name).n_dead) == want
    sizes = {name: (len(geometry(name).group), geometry(name).basis.n_sector) for name in GEOMETRY}
    assert sizes["identity-L11"] == (1, 462) and geometry("identity-L11").basis.n == 462 and geometry("identity-L11").nb == 20
    assert sizes["ring7-k0"][0] < 16 and sizes["ring12-kpi-p-1"][0] % 16 != 0
    assert sizes["torus4x4-full"] == (_lib.SYMSECTOR_MAX_GROUP, 12870)
    assert sizes["K16-D16"] == (32, 12870) and geometry("K16-D16").nb == 120
    assert sizes["ring34-nd2"] == (34, 561) and sizes["ring40-nd2"] == (80, 780)
    for name in ("ring34-nd2", "ring40-nd2"):
        # (the representatives are minima and stay small; the images and the hop candidates are what is wider than 32 bits)
        assert GEOMETRY[name][0] > 32 and (GEOMETRY[name][0] + 7) // 8 == 5
    walk = geometry("ring22-k0-walk").basis.n
    assert (walk + 15) // 16 > (1 << GEOMETRY["ring22-k0-walk"][2]) and walk % 16 != 0


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_tables(name):
    case = geometry(name)
    b = case.basis
    op = operator(name, couplings(case, "random"))
    assert op.n == op.dim == b.n and op.n_sector == b.n_sector and op.ng == len(case.group)
    assert tuple(op.group) == case.group and tuple(op.orbits) == case.orbit
    assert op.states.dtype == torch.int64 and torch.equal(op.states.cpu(), torch.from_numpy(np.array(b.reps)))
    assert torch.equal(op.norms.cpu(), torch.from_numpy(np.array(b.sigma)))
    reps, bucket, perm_tab = (t.cpu() for t in op._tables)
    assert torch.equal(reps, torch.from_numpy(np.array(b.reps | (b.sigma << 48))))
    assert torch.equal(bucket.to(torch.int64), torch.from_numpy(np.array(b.bucket)))
    assert torch.equal(perm_tab, torch.from_numpy(b.tab.reshape(-1)))
    assert torch.equal(op.row_of(op.states).cpu(), torch.arange(b.n, dtype=torch.int64))
    assert op.row_of(torch.tensor([0, (1 << case.L) - 1], dtype=torch.int64)).tolist() == [-1, -1]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_matvec_against_the_row_formula(name, kind):
    p, x, want = matvec_case(name, kind)
    n = x.size
    op = operator(name, p)
    xd = to_dev(x)
    got = op(xd)
    err = relnorm(got.cpu().numpy(), want)
    print("%s %s: |y - ref| / |ref| = %.2e" % (name, kind, err))
    assert err < 1e-13
    assert torch.equal(op(xd), got)                      # no atomics: two calls return identical bits
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
    case = geometry(name)
    v1, v2, want = form_case(name)
    p = couplings(case, "random")
    op = operator(name, p)
    a, b = to_dev(v1), to_dev(v2)
    got = op.Hadjoint_to_couplingsadjoint(a, b)
    assert got.shape == (2 * case.nb + case.L,)
    norms = np.linalg.norm(v1) * np.linalg.norm(v2)
    bound = 1e-13 * norms
    err = float(np.max(np.abs(got.cpu().numpy() - want)))
    print("%s: max |form - ref| = %.2e (bound %.2e)" % (name, err, bound))
    assert err <= bound
    assert torch.equal(got, op.Hadjoint_to_couplingsadjoint(a, b))       # fixed-order reductions, no atomics
    swapped = op.Hadjoint_to_couplingsadjoint(b, a)                      # S raw is symmetric in (v1, v2): the orbit sums are
    assert float((swapped - got).abs().max()) <= bound
    # constant on every orbit, bit for bit: one block per output sums the same partials in the same order
    host = got.cpu().numpy()
    for o in set(case.orbit):
        members = [c for c, oc in enumerate(case.orbit) if oc == o]
        assert len({host[c].tobytes() for c in members}) == 1
    # H is linear in the couplings: v1^T H[p] v2 = sum_t p_t form_t (the bound of tests/test_gpu_sector.py)
    Hv2 = op(b)
    lhs, rhs = float(a @ Hv2), float(np.sum(p * host))
    assert abs(lhs - rhs) <= 1e-13 * (norms * np.abs(p).sum() + np.linalg.norm(v1) * float(Hv2.norm()))


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_matvec_is_symmetric_and_sees_the_couplings_through_S(name):
    case = geometry(name)
    p, x, _ = matvec_case(name, "random")
    op = operator(name, p)
    a = to_dev(x)
    b = torch.from_numpy(normal_vector(x.size, 8400 + x.size % 97)).to(dev())
    Ha, Hb = op(a), op(b)
    assert abs(float(a @ Hb) - float(Ha @ b)) <= 1e-13 * float(a.norm() * Hb.norm() + b.norm() * Ha.norm())
    # the random couplings are not invariant under the group: H(p) x = H(S p) x
    pbar = case.pbar(p)
    assert np.max(np.abs(pbar - p)) > 0.0 or len(case.group) == 1
    assert float((operator(name, pbar)(a) - Ha).norm()) <= 1e-13 * float(Ha.norm())
    assert float((op.symmetrise(op.couplings).cpu() - torch.from_numpy(pbar)).abs().max()) < 1e-14 * np.max(np.abs(p)) * 16


def test_the_identity_group_is_the_sector_operator():
    name = "identity-L11"
    L, ndown, _, bonds, gens = GEOMETRY[name]
    p, x, _ = matvec_case(name, "random")
    sym = operator(name, p)
    full = SpinSectorOperator(L, bonds, to_dev(p), ndown)
    assert sym.n == full.n and torch.equal(sym.states, full.states) and bool((sym.norms == 1).all())
    xd = to_dev(x)
    want = full(xd)
    assert float((sym(xd) - want).norm() / want.norm()) < 1e-13
    v1, v2, _ = form_case(name)
    f_sym = sym.Hadjoint_to_couplingsadjoint(to_dev(v1), to_dev(v2))
    f_full = full.Hadjoint_to_couplingsadjoint(to_dev(v1), to_dev(v2))
    assert float((f_sym - f_full).abs().max()) <= 1e-13 * np.linalg.norm(v1) * np.linalg.norm(v2)


@pytest.mark.parametrize("name", ["ring8-kpi-p+1-j1j2", "ring12-kpi-p-1", "torus4x4-c4", "torus4x4-pipi-nd7", "K16-D16"])
def test_expand_commutes_with_the_sector_operator(name):
    """SpinSectorOperator(pbar).H(expand(x)) = expand(H_sym x): B B^T commutes with H(pbar)"""
    L, ndown, _, bonds, gens = GEOMETRY[name]
    case = geometry(name)
    p, x, _ = matvec_case(name, "random")
    sym = operator(name, p)
    full = SpinSectorOperator(L, bonds, to_dev(case.pbar(p)), ndown)
    xd = to_dev(x)
    w = sym.expand(xd)
    assert w.shape == (full.n,) and abs(float(w.norm()) - float(xd.norm())) < 1e-13 * float(xd.norm())
    lhs, rhs = full(w), sym.expand(sym(xd))
    assert float((lhs - rhs).norm()) < 1e-13 * float(rhs.norm())


@pytest.mark.parametrize("name", ["ring8-k0-p-1", "ring12-kpi-p-1", "torus4x4-c4", "ring40-nd2"])
def test_to_csr(name):
    p, x, want = matvec_case(name, "random")
    op = operator(name, p)
    csr = op.to_csr()
    xd = to_dev(x)
    got = op(xd)
    assert csr.n == op.n
    assert float((csr(xd) - got).norm() / got.norm()) < 1e-13
    assert relnorm(csr(xd).cpu().numpy(), want) < 1e-13


def test_couplings_changed_in_place_are_seen_without_a_new_operator():
    name = "ring8-kpi-p+1-j1j2"
    case = geometry(name)
    p, x, _ = matvec_case(name, "random")
    op = operator(name, p)
    assert op.bonds == case.bonds and isinstance(op.bonds, tuple)
    handle = op.handle.value
    xd = to_dev(x)
    op(xd)
    delta = normal_vector(p.size, 8600)
    with torch.no_grad():
        op.couplings.add_(torch.from_numpy(delta).to(dev()))
    assert op.handle.value == handle
    assert relnorm(op(xd).cpu().numpy(), ref.apply(case, p + delta, x)) < 1e-13
    parts = op.unpack(op.couplings)
    assert [t.numel() for t in parts] == [16, 16, 8]
    assert torch.equal(op.pack(*parts), op.couplings)
    tables = [t.data_ptr() for t in op._tables]
    op.couplings = to_dev(p)
    assert [t.data_ptr() for t in op._tables] == tables
    assert relnorm(op(xd).cpu().numpy(), matvec_case(name, "random")[2]) < 1e-13
    with pytest.raises(ValueError):
        op.couplings = torch.zeros(p.size + 1, dtype=F64, device=dev())
    with pytest.raises(ValueError):
        op.couplings = torch.zeros(p.size, dtype=torch.float32, device=dev())


def test_validation_errors():
    L, bonds = 8, ring_bonds(8)
    zeros = torch.zeros(2 * L + L, dtype=F64, device=dev())
    T = ref.translation(L)
    with pytest.raises(ValueError, match="permutation"):
        SpinSymmetrySectorOperator(L, bonds, zeros, 4, [((0, 0, 1, 2, 3, 4, 5, 6), 1)])
    with pytest.raises(ValueError, match="consistent"):
        SpinSymmetrySectorOperator(7, ring_bonds(7), torch.zeros(21, dtype=F64, device=dev()), 3, [(ref.translation(7), -1)])
    with pytest.raises(ValueError, match="off the bond list"):
        SpinSymmetrySectorOperator(L, bonds[:-1], zeros[:-1], 4, [(T, 1)])
    with pytest.raises(ValueError, match="twice"):
        SpinSymmetrySectorOperator(L, bonds + [(1, 0)], torch.zeros(2 * 9 + L, dtype=F64, device=dev()), 4, [(T, 1)])
    with pytest.raises(ValueError, match="empty"):
        # one down spin on a ring of 4 at k = 0, p = -1: the single orbit is fixed by the reflection about the down site (T R),
        # whose character is -1, so sigma = 0 and no row is left
        SpinSymmetrySectorOperator(4, ring_bonds(4), torch.zeros(12, dtype=F64, device=dev()), 1, ring_symmetries(4, 0, -1))


# ---- end to end ------------------------------------------------------------------------------------------------------
E2E_L, E2E_NDOWN = 12, 6
E2E_BONDS = tuple(ring_bonds(E2E_L, 1) + ring_bonds(E2E_L, 2))
E2E_SECTORS = [(0, 1), (0, -1), ("pi", 1), ("pi", -1)]


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
def e2e_case(sector):
    momentum, parity = sector
    case = ref.Case(E2E_L, E2E_NDOWN, E2E_BONDS, ring_symmetries(E2E_L, momentum, parity))
    return case, torch.from_numpy(ref.dense_B(case))


def dense_sym_torch(sector, p):
    """B^T H(p) B with B constant and p the leaf: the couplings enter as they are, not through their orbit means"""
    _, B = e2e_case(sector)
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


def sym_operator(sector, p):
    return SpinSymmetrySectorOperator(E2E_L, E2E_BONDS, p, E2E_NDOWN, ring_symmetries(E2E_L, *sector))


@pytest.mark.parametrize("sector", E2E_SECTORS)
def test_ground_state_gap_and_gradients_against_eigh(sector, monkeypatch):
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    case, _ = e2e_case(sector)
    n = k = case.basis.n
    p0, d2, J2 = j1j2_point(9702)
    p = p0 + J2 * d2
    u = unit(n, 9200)
    pr = p.clone().requires_grad_(True)
    lam, U = torch.linalg.eigh(dense_sym_torch(sector, pr))
    (g_ref,) = torch.autograd.grad(lam[0] + (U[:, 0] @ u) ** 2, pr, retain_graph=True)
    (gap_ref_g,) = torch.autograd.grad(lam[1] - lam[0], pr)
    op = sym_operator(sector, p.to(dev()).requires_grad_(True))
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
    symeig.setLowestSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(9500):
        vals, _ = symeig.LowestSparseSymeig.apply(op.couplings, k, n, 2)
        gap = vals[1] - vals[0]
        (gg,) = torch.autograd.grad(gap, op.couplings)
    gap_ref = (lam[1] - lam[0]).item()
    gap_err = abs(gap.item() - gap_ref) / abs(gap_ref)
    gg_err = float((gg.cpu() - gap_ref_g).abs().max()) / float(gap_ref_g.abs().max())
    print("    gap rel err %.2e   dgap/dcouplings max abs err / max = %.2e" % (gap_err, gg_err))
    assert gap_err < TOL
    assert gg_err < TOL


@pytest.mark.parametrize("sector", E2E_SECTORS)
def test_second_order_in_J2(sector, monkeypatch):
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    case, _ = e2e_case(sector)
    n = k = case.basis.n
    p0, d2, J2 = j1j2_point(9721)
    tr = torch.tensor(J2, dtype=F64, requires_grad=True)
    lam, _ = torch.linalg.eigh(dense_sym_torch(sector, p0 + tr * d2))
    (r1,) = torch.autograd.grad(lam[0], tr, create_graph=True)
    (r2,) = torch.autograd.grad(r1, tr)
    t = torch.tensor(J2, dtype=F64, device=dev(), requires_grad=True)
    op = sym_operator(sector, p0.to(dev()) + t * d2.to(dev()))
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


def test_the_lowest_sector_is_the_ground_state_of_the_full_sector(monkeypatch):
    """invariant couplings (the clean J1-J2 ring): min over the four sectors of E0 = E0 of SpinSectorOperator, and in that sector
    the sum over the J2 orbit of dE0/dJ2_t = dE0/dJ2 of the full sector"""
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    p0, d2, J2 = j1j2_point(0, noise=0.0)
    p = (p0 + J2 * d2).to(dev())
    full = SpinSectorOperator(E2E_L, E2E_BONDS, p.clone().requires_grad_(True), E2E_NDOWN)
    symeig.setDominantSparseSymeig(full.H, full.Hadjoint_to_couplingsadjoint)
    with PatchRandn(9800):
        E_full, _ = symeig.DominantSparseSymeig.apply(full.couplings, 300, full.n)
        (g_full,) = torch.autograd.grad(E_full, full.couplings)
    best = None
    for sector in E2E_SECTORS:
        op = sym_operator(sector, p.clone().requires_grad_(True))
        symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
        with PatchRandn(9810):
            E0, _ = symeig.DominantSparseSymeig.apply(op.couplings, op.n, op.n)
            (g,) = torch.autograd.grad(E0, op.couplings)
        if best is None or E0.item() < best[0]:
            best = (E0.item(), float(g.cpu() @ d2), sector)
    want_g = float(g_full.cpu() @ d2)
    print("E0: lowest sector %s %.12f, full sector %.12f   dE0/dJ2: %.10f, %.10f" % (best[2], best[0], E_full.item(), best[1], want_g))
    assert abs(best[0] - E_full.item()) < TOL * abs(E_full.item())
    assert abs(best[1] - want_g) < TOL * abs(want_g)


def test_example_symmetry():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "spin_lattice", "symmetry.py")
    spec = importlib.util.spec_from_file_location("spin_lattice_symmetry", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    orig = CG.EPS_DEFAULT
    try:
        out = ex.main(L=12)
        h, (momentum, parity) = 1e-4, out["ground_sector"]
        pair = [ex.ground_energy(ex.model(12, torch.tensor(out["J2"] + s * h, dtype=F64, device=dev()), momentum, parity, dev()),
                                 200).item() for s in (1.0, -1.0)]
    finally:
        CG.EPS_DEFAULT = orig
    fd = (pair[0] - pair[1]) / (2 * h)
    print("ground sector %s: dE0/dJ2 autograd %.9f   central difference %.9f" % (out["ground_sector"], out["dE0_dJ2"], fd))
    assert out["n_full"] == 924 and len(out["E0"]) == len(out["gap"]) == 4
    assert out["n"] == [e2e_case(s)[0].basis.n for s in E2E_SECTORS] and sum(out["n"]) < 924
    assert abs(min(out["E0"]) - out["E0_full"]) < 1e-10 * abs(out["E0_full"])
    assert all(g > 0.0 for g in out["gap"])
    assert abs(out["dE0_dJ2"] - fd) < 1e-5
