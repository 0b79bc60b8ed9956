"""Reduced density matrices on the GPU (docs/design/21-reduced-density-matrix.md): the index-table builders, k_rdm_cross
(+ k_rdm_cross_reduce) and k_rdm_pull against the numpy reference of tests/rdm_reference.py at the smallest shapes that reach
each path (the table ``rdm_reference.CASES``; tests/test_rdm_cpu.py holds it to its description), the autograd pair, every
refused argument, and the entanglement measures end to end against torch.linalg.eigh autograd and closed forms.

    L, ndown, sites                              n            what it reaches
    2,1,[0]  4,2,[0,1]  5,2,[0,3]                2 6 10       less than one tile, dB = 1
    7,3,[6,0,3]                                  35           unsorted sites, odd L
    9,7,[2..6]                                   36           the first block is m = 3 (blocks 10, 5, 1)
    9,4,[0]                                      126          LA = 1: 1 x 1 blocks, dB = 70 and 56, no multiple of 16
    12,6,[11,0,5,6,2,9]                          924          dA = 15 and 20: one short of a tile, one tile plus a ragged one
    20,1,[0..15]                                 20           LA at the cap, dA = 16 exactly one tile, dB = 1 and 4
    16,8,[0,2,..,14]                             12 870       dA = dB = 70: several tiles both ways, mirrored tiles
    20,10,[0,1]                                  184 756      dB = 48 620 and 43 758: the split over ~1300 waves and the reduce
    20,10,[0..9]                                 184 756      dA = 252: 16 x 16 tiles of 16 per block, the compute-bound shape
    34,2,[33,0,17]  40,2,[39,0,20]               561 780      states wider than 32 bits
    full space 3,[1] 6,[5,0,2] 10,[0..4] 12,[1,3,..,11] 14,[13]   8 .. 16 384   one block; contiguous A = a reshape; dA = 64; dB = 8192

The forward runs at both tile edges (16 and 32) in every geometry.  The launchers cap no grid: one wave takes one work item, so
there is no walking case.
"""
import functools
import importlib.util
import math
import os
from ctypes import c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rdm_reference as ref  # noqa: E402
import sector_reference  # noqa: E402
from helpers import PatchRandn  # noqa: E402
from dominantsparseeigenad_amd import _lib, engine  # noqa: E402
from dominantsparseeigenad_amd.engine import _stream  # noqa: E402
from dominantsparseeigenad_amd.operators import (Bipartition, SpinSectorOperator, SpinSymmetrySectorOperator,  # noqa: E402
                                                 ring_bonds, ring_symmetries)
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402
import dominantsparseeigenad_amd.symeig as symeig  # noqa: E402
import dominantsparseeigenad_amd.CG as CG  # noqa: E402

F64 = torch.float64
TOL = 1e-10                      # tests/test_gpu_sector.py: what its own psi-adjoint test meets
U = 2.0 ** -53
LD = np.longdouble
SENTINEL = -7.25
PAD = 300
NAMES = list(ref.CASES)


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


def to_dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64)).to(dev())


@functools.lru_cache(maxsize=None)
def part(name):
    L, ndown, sites, _, _ = ref.CASES[name]
    return Bipartition(L, sites, ndown=ndown, device=dev())


@functools.lru_cache(maxsize=None)
def vectors(name):
    n = ref.CASES[name][3]
    x, y = normal_vector(n, 6100 + n % 89), normal_vector(n, 6200 + n % 89)
    for a in (x, y):
        a.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def cross_case(name, same):
    """(the blocks M(x) M(y)^T in extended precision, rounded to fp64 only for the comparison; the bound (K + 2) 2^-53
    (|M(x)| |M(y)|^T) per block) -- computed once and never written to.  ``same``: y = x."""
    L, ndown, sites, _, _ = ref.CASES[name]
    x, y = vectors(name)
    if same:
        y = x
    want, bound = [], []
    for (m, dA, dB), a, b in zip(ref.blocks(L, ndown, sites), ref.slices(L, ndown, sites, x), ref.slices(L, ndown, sites, y)):
        want.append(a.astype(LD) @ b.astype(LD).T)
        bound.append((dB + 2) * U * (np.abs(a) @ np.abs(b).T))
    return want, bound


@functools.lru_cache(maxsize=None)
def pull_case(name):
    """(G blocks, then per transpose setting the reference vector in extended precision and the bound (dA + 2) 2^-53 |G| |M(y)|)"""
    L, ndown, sites, n, _ = ref.CASES[name]
    _, y = vectors(name)
    blocks = ref.blocks(L, ndown, sites)
    G = [normal_vector(dA * dA, 6300 + m).reshape(dA, dA) for m, dA, _ in blocks]
    out = {}
    for transpose in (False, True):
        want, bound = np.zeros(n, dtype=LD), np.zeros(n)
        for (m, dA, dB), ix, g, sl in zip(blocks, ref.index_blocks(L, ndown, sites), G, ref.slices(L, ndown, sites, y)):
            gg = g.T if transpose else g
            want[ix] = gg.astype(LD) @ sl.astype(LD)
            bound[ix] = (dA + 2) * U * (np.abs(gg) @ np.abs(sl))
        out[transpose] = (want, bound)
    return G, out


def ratio(got, want, bound):
    """the largest |got - want| / bound (0 / 0 = 0: an exact 0 has the bound 0)"""
    err = np.abs(np.asarray(got).astype(LD) - want).astype(np.float64)
    assert np.all(err[bound == 0.0] == 0.0)
    return float(np.max(err[bound > 0.0] / bound[bound > 0.0])) if np.any(bound > 0.0) else 0.0


@pytest.mark.parametrize("name", NAMES)
def test_index_table(name):
    L, ndown, sites, n, _ = ref.CASES[name]
    p = part(name)
    assert p.n == n and p.idx.dtype == torch.int32 and p.idx.shape == (n,)
    assert p.blocks == tuple(ref.blocks(L, ndown, sites))
    assert np.array_equal(p.idx.cpu().numpy().astype(np.int64), ref.index_table(L, ndown, sites))
    if ndown is not None:                                # the same table on an operator's rank tables
        op = SpinSectorOperator(L, ((0, 1),), torch.zeros(2 + L, dtype=F64, device=dev()), ndown)
        assert torch.equal(op.bipartition(sites).idx, p.idx)


@pytest.mark.parametrize("tile", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_cross_against_the_reference(name, tile):
    x, y = vectors(name)
    want, bound = cross_case(name, False)
    p = part(name)
    p.set_tile(tile)
    try:
        got = p.cross(to_dev(x), to_dev(y))
    finally:
        p.set_tile(0)
    assert len(got) == len(want)
    worst = 0.0
    for g, w, b in zip(got, want, bound):
        assert g.shape == w.shape
        worst = max(worst, ratio(g.cpu().numpy(), w, b))
    print("%s tile %d: max |cross - ref| / bound = %.3f" % (name, 16 * tile, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("tile", [0, 1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_rdm_is_symmetric_deterministic_and_has_the_trace(name, tile):
    x, _ = vectors(name)
    want, bound = cross_case(name, True)
    p = part(name)
    xd = to_dev(x)
    p.set_tile(tile)
    try:
        flat = p.rdm_flat(xd)
        again = p.rdm_flat(xd)
    finally:
        p.set_tile(0)
    assert torch.equal(flat, again)                      # fixed-order reduction, no atomics
    blocks = p.views(flat)
    worst, trace, trace_bound = 0.0, LD(0.0), 0.0
    for g, w, b in zip(blocks, want, bound):
        assert torch.equal(g, g.T)                       # bitwise
        worst = max(worst, ratio(g.cpu().numpy(), w, b))
        trace += np.sum(np.diagonal(g.cpu().numpy()).astype(LD))
        trace_bound += float(np.sum(np.diagonal(b)))
    norm2 = np.sum(x.astype(LD) ** 2)
    print("%s tile %d: max |rdm - ref| / bound = %.3f   |Tr rho - |x|^2| / bound = %.3f"
          % (name, 16 * tile, worst, float(abs(trace - norm2)) / trace_bound))
    assert worst <= 1.0
    assert float(abs(trace - norm2)) <= trace_bound


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_pull_against_the_reference(name, transpose):
    _, y = vectors(name)
    G, cases = pull_case(name)
    want, bound = cases[transpose]
    p = part(name)
    got = p.pull([to_dev(g) for g in G], to_dev(y), transpose=transpose)
    assert got.shape == (p.n,)
    worst = ratio(got.cpu().numpy(), want, bound)
    print("%s transpose %s: max |pull - ref| / bound = %.3f" % (name, transpose, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("name", NAMES)
def test_nothing_is_written_beyond_the_documented_lengths(name):
    """every output and scratch buffer is PAD elements longer than documented and filled with a sentinel first"""
    L, ndown, sites, n, _ = ref.CASES[name]
    p = part(name)
    lib = _lib.load()
    x, y = (to_dev(v) for v in vectors(name))
    nd, LA, st = p._nd, len(sites), _stream(dev())

    def ptr(t):
        return c_void_p(t.data_ptr())

    idx = torch.full((n + PAD,), -77, dtype=torch.int32, device=dev())
    if ndown is None:
        _lib.check(lib.dsea_rdm_build_index_full(L, LA, p._sites, ptr(idx), st), "dsea_rdm_build_index_full")
    else:
        op = SpinSectorOperator(L, ((0, 1),), torch.zeros(2 + L, dtype=F64, device=dev()), ndown)
        _lib.check(lib.dsea_rdm_build_index_sector(L, ndown, LA, p._sites, ptr(op._tables[1]), ptr(op._tables[2]), ptr(idx), st),
                   "dsea_rdm_build_index_sector")
    assert torch.equal(idx[:n], p.idx) and bool((idx[n:] == -77).all())
    for tile in (1, 2):
        for b in (y, x):                                 # the general and the symmetric form
            out = torch.full((p.out_len + PAD,), SENTINEL, dtype=F64, device=dev())
            scratch = torch.full((p._scratch_doubles + PAD,), SENTINEL, dtype=F64, device=dev())
            _lib.check(lib.dsea_rdm_cross(L, nd, LA, p._sites, ptr(p.idx), ptr(x), ptr(b), ptr(out), ptr(scratch), tile, st),
                       "dsea_rdm_cross")
            assert bool((out[p.out_len:] == SENTINEL).all()) and bool((scratch[p._scratch_doubles:] == SENTINEL).all())
            assert not bool((out[:p.out_len] == SENTINEL).any())
    G = torch.from_numpy(normal_vector(p.out_len, 6400)).to(dev())
    for transpose in (0, 1):
        out = torch.full((n + PAD,), SENTINEL, dtype=F64, device=dev())
        _lib.check(lib.dsea_rdm_pull(L, nd, LA, p._sites, ptr(p.idx), ptr(G), ptr(y), ptr(out), transpose, st), "dsea_rdm_pull")
        assert bool((out[n:] == SENTINEL).all()) and not bool((out[:n] == SENTINEL).any())


# ---- autograd ----------------------------------------------------------------------------------------------------------
GRAD_NAMES = ["L2-1", "L4-2", "L5-2", "L7-3-unsorted"]


@pytest.mark.parametrize("name", GRAD_NAMES)
def test_gradcheck_and_gradgradcheck(name):
    """cross and pull are bilinear, so central differences are exact to rounding: the default tolerances"""
    p = part(name)
    x, y = vectors(name)
    xd, yd = to_dev(x).requires_grad_(True), to_dev(y).requires_grad_(True)
    for fn, args in ((p.cross, (xd, yd)), (p.rdm, (xd,)), (p.renyi2, (xd,))):
        assert torch.autograd.gradcheck(fn, args)
        assert torch.autograd.gradgradcheck(fn, args)


@pytest.mark.parametrize("name", ["L12-6", "L16-8"])
def test_gradient_of_a_linear_functional_of_rho(name):
    """d/dpsi sum_m <W_m, rho_m> has the slices (W_m + W_m^T) M_m(psi).  The library forms it as the sum of two pulls, each
    within (dA + 2) 2^-53 |W| |M| of its value (the pull bound), and adds them with one more rounding: the bound is
    (dA + 3) 2^-53 (|W| + |W|^T) |M|."""
    L, ndown, sites, n, _ = ref.CASES[name]
    x, _ = vectors(name)
    blocks = ref.blocks(L, ndown, sites)
    W = [normal_vector(dA * dA, 6500 + m).reshape(dA, dA) for m, dA, _ in blocks]
    want, bound = np.zeros(n, dtype=LD), np.zeros(n)
    for (m, dA, dB), ix, w, sl in zip(blocks, ref.index_blocks(L, ndown, sites), W, ref.slices(L, ndown, sites, x)):
        want[ix] = (w + w.T).astype(LD) @ sl.astype(LD)
        bound[ix] = (dA + 3) * U * ((np.abs(w) + np.abs(w.T)) @ np.abs(sl))
    p = part(name)
    xd = to_dev(x).requires_grad_(True)
    loss = sum((to_dev(w) * r).sum() for w, r in zip(W, p.rdm(xd)))
    (g,) = torch.autograd.grad(loss, xd)
    worst = ratio(g.cpu().numpy(), want, bound)
    print("%s: max |grad - (W + W^T) M| / bound = %.3f" % (name, worst))
    assert worst <= 1.0


# ---- errors ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,ndown,sites", [
    (8, 4, [0, 0]), (8, 4, [8]), (8, 4, [-1]),                               # a site repeated, out of range
    (8, 4, []), (8, 4, list(range(8))), (20, 10, list(range(17))),           # LA outside 1 .. min(L - 1, 16)
    (20, None, list(range(16))),                                             # a flat output of 2^32 elements
    (34, 17, [0]), (41, 1, [0]), (8, 0, [0]), (8, 8, [0]),                   # the sector limits
    (31, None, [0]),                                                         # the full space beyond L = 30
])
def test_refused_arguments_raise_value_error(L, ndown, sites):
    with pytest.raises(ValueError):
        Bipartition(L, sites, ndown=ndown, device=dev())


def test_wrong_tensors_raise_value_error():
    p = part("L7-3-unsorted")
    good = to_dev(vectors("L7-3-unsorted")[0])
    with pytest.raises(ValueError):
        p.rdm(good.cpu())
    with pytest.raises(ValueError):
        p.cross(good, good.cpu())
    with pytest.raises(ValueError):
        p.rdm(good[:-1])
    with pytest.raises(ValueError):
        p.cross(good, torch.cat([good, good]))
    with pytest.raises(ValueError):
        p.pull(torch.zeros(p.out_len + 1, dtype=F64, device=dev()), good)
    with pytest.raises(ValueError):
        p.pull(torch.zeros(p.out_len, dtype=F64), good)
    with pytest.raises(ValueError):
        p.rdm(good.to(torch.float32))
    with pytest.raises(ValueError):
        Bipartition(8, [0, 1], ndown=4, device="cpu")


def test_dense_places_the_blocks():
    name = "L7-3-unsorted"
    L, ndown, sites, _, _ = ref.CASES[name]
    x, _ = vectors(name)
    want = ref.partial_trace(L, sites, ref.embed(L, ndown, x))
    got = part(name).dense(to_dev(x)).cpu().numpy()
    assert got.shape == want.shape and np.max(np.abs(got - want)) < 1e-13 * np.max(np.abs(want))
    name = "full-L6"
    L, _, sites, _, _ = ref.CASES[name]
    x, _ = vectors(name)
    want = ref.partial_trace(L, sites, x)
    got = part(name).dense(to_dev(x)).cpu().numpy()
    assert np.max(np.abs(got - want)) < 1e-13 * np.max(np.abs(want))


# ---- end to end ----------------------------------------------------------------------------------------------------------
def ground_state(op, k, seed):
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(seed):
        return symeig.DominantSparseSymeig.apply(op.couplings, k, op.n)


@pytest.mark.filterwarnings("ignore:Lanczos breakdown")
def test_dimers_have_the_entropies_of_their_cut_singlets(monkeypatch):
    """four singlets on (0,1) (2,3) (4,5) (6,7): E0 = -12, gap 4; a cut through c singlets has S_2 = S = c ln 2.  (Four commuting
    bond terms: the sector has five distinct levels, so the Krylov space ends after five steps and the run says so.)"""
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, bonds = 8, ((0, 1), (2, 3), (4, 5), (6, 7))
    p = torch.cat([torch.ones(8, dtype=F64), torch.zeros(8, dtype=F64)]).to(dev())
    op = SpinSectorOperator(L, bonds, p, 4)
    E0, psi = ground_state(op, op.n, 9900)
    assert abs(E0.item() + 12.0) < 1e-12 * 12.0
    for sites, cut in (([0, 1], 0), ([0, 2], 2), ([1, 2], 2), ([0, 2, 4, 6], 4)):
        b = op.bipartition(sites)
        s2, s = b.renyi2(psi).item(), b.entropy(psi).item()
        print("A = %s: S2 = %.3e  S = %.3e  (want %d ln 2)" % (sites, s2, s, cut))
        assert abs(s2 - cut * math.log(2.0)) <= TOL
        assert abs(s - cut * math.log(2.0)) <= TOL


E2E_L, E2E_NDOWN = 10, 5
E2E_BONDS = tuple(ring_bonds(E2E_L, 1) + ring_bonds(E2E_L, 2))


def dense_torch(L, ndown, bonds, p):
    """the dense sector matrix as a differentiable function of the flat couplings p (CPU): the row formula, entry by entry"""
    nb = len(bonds)
    n = math.comb(L, ndown)
    r = torch.arange(n, dtype=torch.int64)
    H = torch.zeros((n, n), dtype=F64)
    for i, z in enumerate(sector_reference._z(L, ndown)):
        H = H.index_put((r, r), p[2 * nb + i] * torch.from_numpy(np.array(z)), accumulate=True)
    for t, (rows, cols, zz) in enumerate(sector_reference._partners(L, ndown, bonds)):
        H = H.index_put((r, r), p[nb + t] * torch.from_numpy(np.array(zz)), accumulate=True)
        H = H.index_put((torch.from_numpy(np.array(rows)), torch.from_numpy(np.array(cols))), (2.0 * p[t]).expand(rows.size),
                        accumulate=True)
    return H


def j1j2_point(seed, J2=0.3, noise=0.1):
    """the couplings of the J1-J2 Heisenberg ring at J1 = 1 plus random perturbations of all 2 nb + L of them (no symmetry and no
    degeneracy left inside the sector)"""
    L = E2E_L
    near = torch.cat([torch.ones(L, dtype=F64), torch.zeros(L, dtype=F64)])
    nxt = torch.cat([torch.zeros(L, dtype=F64), torch.ones(L, dtype=F64)])
    field = torch.zeros(L, dtype=F64)
    d1, d2 = torch.cat([near, near, field]), torch.cat([nxt, nxt, field])
    return d1 + noise * torch.from_numpy(normal_vector(d1.numel(), seed).copy()) + J2 * d2


def dense_entropies(psi, L, ndown, LA, floor=1e-14):
    """(S_2, S, eigenvalues dropped) of the LOW LA sites from the embedded vector with torch alone: state = a + 2^LA b, so the
    2^L vector reshaped to (2^LB, 2^LA) is M^T"""
    states = torch.from_numpy(np.array(sector_reference.states(L, ndown), dtype=np.int64))
    w = torch.zeros(1 << L, dtype=F64).index_put((states,), psi)
    M = w.reshape(1 << (L - LA), 1 << LA)
    rho = M.T @ M
    rho = rho / torch.trace(rho)
    lam = torch.linalg.eigvalsh(rho)
    keep = lam.detach() > floor
    return -torch.log((rho * rho).sum()), -(lam[keep] * torch.log(lam[keep])).sum(), int((~keep).sum())


def test_j1j2_entropies_and_their_gradients_against_eigh(monkeypatch):
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, ndown, bonds = E2E_L, E2E_NDOWN, E2E_BONDS
    n = k = 252
    p = j1j2_point(9702)
    pr = p.clone().requires_grad_(True)
    lam, V = torch.linalg.eigh(dense_torch(L, ndown, bonds, pr))
    s2_ref, s_ref, dropped = dense_entropies(V[:, 0], L, ndown, 5)
    assert dropped == 0
    (g2_ref,) = torch.autograd.grad(s2_ref, pr, retain_graph=True)
    (g_ref,) = torch.autograd.grad(s_ref, pr)
    op = SpinSectorOperator(L, bonds, p.to(dev()).requires_grad_(True), ndown)
    b = op.bipartition([0, 1, 2, 3, 4])
    E0, psi = ground_state(op, k, 9300)
    s2, s = b.renyi2(psi), b.entropy(psi)
    with PatchRandn(9350):
        (g2,) = torch.autograd.grad(s2, op.couplings, retain_graph=True)
    with PatchRandn(9360):
        (g,) = torch.autograd.grad(s, op.couplings)
    assert engine.last_cg.converged
    smallest = float(b.spectrum(psi.detach()).min())
    e = {"S2": abs(s2.item() - s2_ref.item()), "S": abs(s.item() - s_ref.item()),
         "dS2": float((g2.cpu() - g2_ref).abs().max()) / float(g2_ref.abs().max()),
         "dS": float((g.cpu() - g_ref).abs().max()) / float(g_ref.abs().max())}
    print("J1-J2 ring, L = 10, A = 0..4: gap %.3f  S2 = %.6f  S = %.6f  smallest eigenvalue of rho %.1e   errors %s"
          % ((lam[1] - lam[0]).item(), s2.item(), s.item(), smallest, {key: "%.1e" % v for key, v in e.items()}))
    assert g2.shape == g.shape == (2 * 20 + 10,)
    assert abs(E0.item() - lam[0].item()) < 1e-12 * abs(lam[0].item())
    assert smallest > 1e-14                              # nothing is dropped on this side either
    for key, v in e.items():
        assert v < TOL, key


def test_symmetry_sector_state_through_expand(monkeypatch):
    """the clean L = 12 J1-J2 ring: the (k, p) sector that holds the ground state, expanded, has the Renyi entropy of the ground
    state of the full S^z = 0 sector"""
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, ndown = 12, 6
    bonds = tuple(ring_bonds(L, 1) + ring_bonds(L, 2))
    j = torch.cat([torch.ones(L, dtype=F64), 0.3 * torch.ones(L, dtype=F64)])
    p = torch.cat([j, j, torch.zeros(L, dtype=F64)]).to(dev())
    full = SpinSectorOperator(L, bonds, p.clone(), ndown)
    E_full, psi_full = ground_state(full, 300, 9800)
    b = full.bipartition([0, 1, 2, 3, 4, 5])
    want = b.renyi2(psi_full).item()
    best = None
    for sector in [(0, 1), (0, -1), ("pi", 1), ("pi", -1)]:
        op = SpinSymmetrySectorOperator(L, bonds, p.clone(), ndown, ring_symmetries(L, *sector))
        E0, psi = ground_state(op, op.n, 9810)
        if best is None or E0.item() < best[0]:
            best = (E0.item(), b.renyi2(op.expand(psi)).item(), sector)
    print("sector %s: E0 %.12f (full %.12f)   S2 %.12f (full %.12f)" % (best[2], best[0], E_full.item(), best[1], want))
    assert abs(best[0] - E_full.item()) < TOL * abs(E_full.item())
    assert abs(best[1] - want) <= TOL


def test_example_entanglement():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "spin_lattice", "entanglement.py")
    spec = importlib.util.spec_from_file_location("spin_lattice_entanglement", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    orig = CG.EPS_DEFAULT
    try:
        out = ex.main(L=10)
    finally:
        CG.EPS_DEFAULT = orig
    print("dS2/dJ2 at %.2f: autograd %.9f   central difference %.9f   I(0:r) = %s"
          % (out["J2_grad"], out["dS2_dJ2"], out["dS2_dJ2_fd"], ["%.4f" % v for v in out["mutual_information"]]))
    assert out["n"] == 252
    assert len(out["S2"]) == len(out["S"]) == len(out["J2"])
    assert all(0.0 < a <= b + 1e-12 for a, b in zip(out["S2"], out["S"]))       # S_2 <= S
    assert abs(out["dS2_dJ2"] - out["dS2_dJ2_fd"]) < 1e-5
    assert len(out["mutual_information"]) == 5 and all(v >= -1e-10 for v in out["mutual_information"])
