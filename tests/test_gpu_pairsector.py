"""All-pair XXZ couplings in one magnetisation sector on the GPU (docs/design/22-pair-sector.md): k_spmv_pairsector,
k_pairsector_forms and k_pairsector_gram against the bond-list operator on the same tables where that one can hold all pairs
(L <= 16), against the numpy reference of tests/pairsector_reference.py beyond it, then bitwise properties, identities that need
no reference, autograd, and the Haldane-Shastry ring and the power-law chain end to end.

    L, ndown    n        P     what it reaches
    2,1         2        1     the smallest operator: one pair, one Gram tile with 3 live columns
    5,2         10       10    less than one wave, n no multiple of 4
    8,4         70       28    pairs inside the low half, inside the high half and across the split of the rank tables
    15,7        6435     105   L + 1 = 16: exactly one Gram tile; 26 blocks
    16,8        12870    120   L + 1 = 17: the first ragged second tile row
    17,2        136      136   the first L beyond the bond-list cap (128)
    18,9        48620    153   190 row ranges; with the grid capped at 64 blocks they walk
    31,2  32,2  465 496  465 496   L + 1 = 32 and 33: two full tile rows, and the third tile row
    40,1  40,2  40  780  780   the cap of L and P; states wider than 32 bits

Tolerances.  Mat-vec: 1e-13 in the relative norm (the project's value).  A form is a sum of n products in some order, so it
differs from any other order by at most n eps |v1| |v2| (eps = 2^-52; twice that for the xy forms, whose terms carry a factor
2).  Against the device twin the issue's 1e-13 |v1| |v2| is used where it is the smaller of the two.
"""
import functools
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pairsector_reference as ref  # noqa: E402
from helpers import PatchRandn  # noqa: E402
from dominantsparseeigenad_amd import _lib, engine  # noqa: E402
from dominantsparseeigenad_amd.engine import Workspace, _ptr, _stream  # noqa: E402
from dominantsparseeigenad_amd.operators import (SpinSectorOperator, SpinSectorPairOperator, power_law_couplings,  # noqa: E402
                                                 ring_structure_factor)
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402
import dominantsparseeigenad_amd.symeig as symeig  # noqa: E402
import dominantsparseeigenad_amd.CG as CG  # noqa: E402

F64 = torch.float64
EPS = 2.0 ** -52
TWIN = [(2, 1), (5, 2), (8, 4), (15, 7), (16, 8)]
BEYOND = [(17, 2), (18, 9), (31, 2), (32, 2), (40, 1), (40, 2)]


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


def to_dev(a):
    return torch.from_numpy(np.array(a)).to(dev())      # (a copy: the cached arrays are read-only)


def relnorm(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


@functools.lru_cache(maxsize=None)
def inputs(L, ndown):
    """(couplings, x, v1, v2) on the host, drawn once per case and never written to"""
    n = math.comb(L, ndown)
    out = (normal_vector(ref.nparam(L), 11000 + 41 * L + ndown), normal_vector(n, 11100 + 41 * L + ndown),
           normal_vector(n, 11200 + 41 * L + ndown), normal_vector(n, 11300 + 41 * L + ndown))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(L, ndown):
    """(H x, forms(v1, v2)) of the numpy reference, computed once per case and never written to"""
    p, x, v1, v2 = inputs(L, ndown)
    out = (ref.apply(L, ndown, p, x), ref.forms(L, ndown, v1, v2))
    for a in out:
        a.setflags(write=False)
    return out


def form_bounds(L, n, v1, v2):
    """per form: n eps |v1| |v2|, twice that for the xy forms"""
    P = ref.npair(L)
    unit = n * EPS * np.linalg.norm(v1) * np.linalg.norm(v2)
    return np.concatenate([np.full(P, 2.0 * unit), np.full(P + L, unit)])


def full_contract(op, x, want):
    """the contract of a kind in launch_spmv on the host arrays x, want = H x: y = H x - shift x, the block partials of x.y, the
    skip flag; returns the two relative errors"""
    lib = _lib.load()
    n = x.size
    xd = to_dev(x)
    ws = Workspace.get(n, 8, dev())
    shift = torch.tensor([0.375], dtype=F64, device=dev())
    dot = torch.zeros(1, dtype=F64, device=dev())
    y = torch.empty(n, dtype=F64, device=dev())
    _lib.check(lib.dsea_spmv(op.handle, ws.handle, _ptr(xd), _ptr(y), _ptr(shift), _ptr(dot), None, _stream(dev())), "dsea_spmv")
    shifted = want - 0.375 * x
    err_s = relnorm(y.cpu().numpy(), shifted)
    err_d = abs(dot.item() - float(x @ shifted)) / (np.linalg.norm(x) * np.linalg.norm(shifted))
    flag = torch.ones(1, dtype=F64, device=dev())
    sentinel = torch.full((n,), -7.0, dtype=F64, device=dev())
    _lib.check(lib.dsea_spmv(op.handle, ws.handle, _ptr(xd), _ptr(sentinel), _ptr(shift), None, _ptr(flag), _stream(dev())),
               "dsea_spmv")
    assert bool((sentinel == -7.0).all())
    return err_s, err_d


@pytest.mark.parametrize("L,ndown", TWIN)
def test_twin_on_the_device(L, ndown):
    """the bond-list operator with bonds = all pairs: an independent implementation on the same tables, same parameter order"""
    p, x, v1, v2 = inputs(L, ndown)
    n = x.size
    twin = SpinSectorOperator(L, ref.pairs(L), to_dev(p), ndown)
    op = twin.pair_operator(to_dev(p))
    assert op.n == n and op.npair == len(ref.pairs(L)) and op.pairs == ref.pairs(L)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(op._tables, twin._tables))
    xd = to_dev(x)
    want = twin(xd).cpu().numpy()
    err = relnorm(op(xd).cpu().numpy(), want)
    err_s, err_d = full_contract(op, x, want)
    print("L = %d ndown = %d: |y - twin| / |twin| = %.2e   with shift %.2e   x.y from the partials %.2e" % (L, ndown, err, err_s, err_d))
    assert err < 1e-13 and err_s < 1e-13 and err_d < 1e-13
    a, b = to_dev(v1), to_dev(v2)
    got = op.Hadjoint_to_couplingsadjoint(a, b)
    theirs = twin.Hadjoint_to_couplingsadjoint(a, b)
    assert got.shape == theirs.shape == (ref.nparam(L),)
    norms = np.linalg.norm(v1) * np.linalg.norm(v2)
    dev_err = np.abs((got - theirs).cpu().numpy())
    bound = np.minimum(form_bounds(L, n, v1, v2), 1e-13 * norms)
    print("    max |form - twin| / (|v1| |v2|) = %.2e   (n eps = %.2e)" % (dev_err.max() / norms, n * EPS))
    assert np.all(dev_err <= bound)
    assert torch.equal(got, op.Hadjoint_to_couplingsadjoint(a, b))      # fixed-order reductions, no atomics
    assert torch.equal(op(xd), op(xd))


@pytest.mark.parametrize("L,ndown", TWIN + BEYOND)
def test_against_the_numpy_reference(L, ndown):
    p, x, v1, v2 = inputs(L, ndown)
    want_y, want_f = reference(L, ndown)
    n = x.size
    op = SpinSectorPairOperator(L, to_dev(p), ndown)
    assert op.n == n == math.comb(L, ndown) and op.nparam == p.size
    err = relnorm(op(to_dev(x)).cpu().numpy(), want_y)
    err_s, err_d = full_contract(op, x, want_y)
    print("L = %d ndown = %d (n = %d, P = %d): |y - ref| / |ref| = %.2e   with shift %.2e   x.y %.2e"
          % (L, ndown, n, op.npair, err, err_s, err_d))
    assert err < 1e-13 and err_s < 1e-13 and err_d < 1e-13
    a, b = to_dev(v1), to_dev(v2)
    got = op.Hadjoint_to_couplingsadjoint(a, b)
    f_err = np.abs(got.cpu().numpy() - want_f)
    bound = form_bounds(L, n, v1, v2)
    print("    max |form - ref| / bound: xy %.3f   zz %.3f   z %.3f"
          % tuple(float(np.max(f_err[s] / bound[s])) for s in (slice(0, op.npair), slice(op.npair, 2 * op.npair),
                                                              slice(2 * op.npair, None))))
    assert np.all(f_err <= bound)
    assert torch.equal(got, op.Hadjoint_to_couplingsadjoint(a, b))


def test_the_grid_walk_gives_the_same_rows():
    L, ndown = 18, 9
    p, x, v1, v2 = inputs(L, ndown)
    _, want_f = reference(L, ndown)
    n = x.size
    op = SpinSectorPairOperator(L, to_dev(p), ndown)
    xd, a, b = to_dev(x), to_dev(v1), to_dev(v2)
    y, f = op(xd), op.Hadjoint_to_couplingsadjoint(a, b)
    op.set_grid_log2(6)
    assert (n + 255) // 256 == 190 > 64
    assert torch.equal(op(xd), y)                        # a row's sum does not depend on which block computes it
    walked = op.Hadjoint_to_couplingsadjoint(a, b)
    bound = form_bounds(L, n, v1, v2)
    assert np.all(np.abs(walked.cpu().numpy() - want_f) <= bound)
    assert np.all(np.abs((walked - f).cpu().numpy()) <= bound)
    assert torch.equal(walked, op.Hadjoint_to_couplingsadjoint(a, b))
    # the adjoint handle of the backward takes the cap over
    v = xd.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(op.Hadjoint_to_couplingsadjoint(v, b).sum(), v)
    ones = SpinSectorPairOperator(L, torch.ones(op.nparam, dtype=F64, device=dev()), ndown, _tables=op._tables)
    assert float((g - ones(b)).norm() / g.norm()) < 1e-13


def test_correlations_are_bitwise_symmetric_and_satisfy_the_sum_rules():
    L, ndown = 12, 6
    sec = SpinSectorOperator(L, [(0, 1)], torch.zeros(2 + L, dtype=F64, device=dev()), ndown)
    v = to_dev(normal_vector(sec.n, 11500))
    xy, zz, z = sec.correlations(v)
    assert xy.shape == zz.shape == (L, L) and z.shape == (L,)
    assert torch.equal(xy, xy.t()) and torch.equal(zz, zz.t())
    again = sec.correlations(v)
    assert all(torch.equal(s, t) for s, t in zip((xy, zz, z), again))
    vv = float(v @ v)
    assert torch.equal(torch.diagonal(zz), torch.full((L,), vv, dtype=F64, device=dev()))
    assert torch.equal(torch.diagonal(xy), torch.full((L,), 2.0 * vv, dtype=F64, device=dev()))
    # sum_i Z_i = L - 2 ndown on every state of the sector: sum_ij <Z_i Z_j> = (L - 2 ndown)^2 |v|^2, sum_i <Z_i> likewise.
    # L^2 and L entries, each within n eps |v|^2 of its sum
    n, m = sec.n, L - 2 * ndown
    print("sum zz = %.3e   sum z = %.3e   (both 0 at S^z = 0; |v|^2 = %.1f)" % (float(zz.sum()), float(z.sum()), vv))
    assert abs(float(zz.sum()) - m * m * vv) <= L * L * n * EPS * vv
    assert abs(float(z.sum()) - m * vv) <= L * n * EPS * vv
    # and away from S^z = 0, with two different vectors
    L, ndown = 12, 4
    op = SpinSectorPairOperator(L, None, ndown)
    assert float(op.couplings.abs().max()) == 0.0
    a, b = to_dev(normal_vector(op.n, 11501)), to_dev(normal_vector(op.n, 11502))
    xy, zz, z = op.correlations(a, b)
    ab, scale = float(a @ b), float(a.norm() * b.norm())
    m = L - 2 * ndown
    assert abs(float(zz.sum()) - m * m * ab) <= L * L * op.n * EPS * scale
    assert abs(float(z.sum()) - m * ab) <= L * op.n * EPS * scale
    assert torch.equal(torch.diagonal(zz), torch.full((L,), ab, dtype=F64, device=dev()))
    assert torch.equal(xy, xy.t()) and torch.equal(zz, zz.t())
    # the entries are the forms
    f = op.Hadjoint_to_couplingsadjoint(a, b)
    assert zz[3, 7].item() == zz[7, 3].item() == f[op.npair + op.pair_index(3, 7)].item()
    assert xy[0, 11].item() == f[op.pair_index(11, 0)].item() and z[5].item() == f[2 * op.npair + 5].item()


def test_couplings_changed_in_place_are_seen_and_the_surface():
    L, ndown = 8, 4
    p, x, _, _ = inputs(L, ndown)
    op = SpinSectorPairOperator(L, to_dev(p), ndown)
    handle = op.handle.value
    xd = to_dev(x)
    delta = normal_vector(p.size, 11600)
    with torch.no_grad():
        op.couplings.add_(to_dev(delta))
    assert op.handle.value == handle
    assert relnorm(op(xd).cpu().numpy(), ref.apply(L, ndown, p + delta, x)) < 1e-13
    tables = [t.data_ptr() for t in op._tables]
    op.couplings = to_dev(p)                             # binding another tensor: a new handle on the same tables
    assert [t.data_ptr() for t in op._tables] == tables
    assert relnorm(op(xd).cpu().numpy(), reference(L, ndown)[0]) < 1e-13
    # pack of matrices, rank / embed / restrict, to_csr, bipartition
    J = to_dev(normal_vector(L * L, 11601).reshape(L, L))
    packed = op.pack(J, 2.0 * J, 0.5)
    assert np.array_equal(packed.cpu().numpy(), ref.pack_matrices(L, J.cpu().numpy(), 2.0 * J.cpu().numpy(), np.full(L, 0.5)))
    assert torch.equal(op.rank(op.states), torch.arange(op.n, device=dev()))
    assert torch.equal(op.restrict(op.embed(xd)), xd)
    csr = op.to_csr()
    assert csr.n == op.n and float((csr(xd) - op(xd)).norm() / op(xd).norm()) < 1e-13
    part = op.bipartition([0, 1, 2])
    assert abs(sum(float(torch.diagonal(b).sum()) for b in part.rdm(xd / xd.norm())) - 1.0) < 1e-13      # Tr rho = |psi|^2
    with pytest.raises(ValueError):
        op.couplings = torch.zeros(p.size + 1, dtype=F64, device=dev())
    with pytest.raises(ValueError):
        op.couplings = torch.zeros(p.size, dtype=torch.float32, device=dev())
    with pytest.raises(ValueError):
        SpinSectorPairOperator(34, None, 17)


# ---- autograd at (5, 2) ------------------------------------------------------------------------------------------------
def small_operator():
    L, ndown = 5, 2
    p, x, v1, v2 = inputs(L, ndown)
    base = SpinSectorPairOperator(L, to_dev(p), ndown)
    return base, to_dev(p), to_dev(x), to_dev(v1), to_dev(v2)


def test_gradcheck_of_the_matvec_in_the_vector_and_the_couplings():
    base, p, x, _, _ = small_operator()

    def apply(v, c):
        return SpinSectorPairOperator(base.N, c, base.ndown, _tables=base._tables).H(v)

    args = (x.requires_grad_(True), p.requires_grad_(True))
    assert torch.autograd.gradcheck(apply, args)
    assert torch.autograd.gradgradcheck(apply, args)


def test_gradcheck_of_the_forms():
    base, _, _, v1, v2 = small_operator()
    args = (v1.requires_grad_(True), v2.requires_grad_(True))
    assert torch.autograd.gradcheck(base.Hadjoint_to_couplingsadjoint, args)
    assert torch.autograd.gradgradcheck(base.Hadjoint_to_couplingsadjoint, args)


def test_gradcheck_of_the_correlations():
    base, _, _, v1, v2 = small_operator()
    args = (v1.requires_grad_(True), v2.requires_grad_(True))
    assert torch.autograd.gradcheck(base.correlations, args)
    assert torch.autograd.gradgradcheck(base.correlations, args)


# ---- end to end --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [12, 18])
def test_haldane_shastry_ground_state_and_its_gradient(L, monkeypatch):
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    k = 60
    p, want = ref.haldane_shastry(L)
    op = SpinSectorPairOperator(L, to_dev(p).requires_grad_(True), L // 2)
    assert op.n == math.comb(L, L // 2) and (L < 17 or op.npair > _lib.LATTICE_MAX_BONDS)
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(11700 + L):
        E0, psi = symeig.DominantSparseSymeig.apply(op.couplings, k, op.n)
        (g,) = torch.autograd.grad(E0, op.couplings)
    e_err = abs(E0.item() - want) / abs(want)
    hf = op.Hadjoint_to_couplingsadjoint(psi.detach(), psi.detach())       # Hellmann-Feynman
    g_err = float((g - hf).abs().max() / hf.abs().max())
    print("Haldane-Shastry L = %d (n = %d, %d pairs), k = %d: E0 rel err %.2e   |dE0/dp - forms(psi, psi)| / max = %.2e"
          % (L, op.n, op.npair, k, e_err, g_err))
    assert e_err < 1e-10
    assert g_err < 1e-9
    if L == 12:
        twin = SpinSectorOperator(L, ref.pairs(L), to_dev(p).requires_grad_(True), L // 2)
        symeig.setDominantSparseSymeig(twin.H, twin.Hadjoint_to_couplingsadjoint)
        with PatchRandn(11700 + L):
            E0_t, _ = symeig.DominantSparseSymeig.apply(twin.couplings, k, twin.n)
            (g_t,) = torch.autograd.grad(E0_t, twin.couplings)
        t_err = float((g - g_t).abs().max() / g_t.abs().max())
        print("    against the gradient of the all-pairs bond-list twin: %.2e" % t_err)
        assert t_err < 1e-10


def test_derivative_of_a_correlator_through_the_eigenvector(monkeypatch):
    """d <Z_0 Z_{L/2}> / d alpha of the open power-law Heisenberg chain at alpha = 2, L = 10: autograd through
    power_law_couplings, the eigenvector adjoint and correlations, against a central difference with h = 1e-4 (its own
    truncation error (h^2 / 6) f''' is what the tolerance 1e-6 leaves room for)"""
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, ndown, h = 10, 5, 1e-4
    n = k = 252
    base = SpinSectorPairOperator(L, None, ndown)

    def correlator(alpha):
        M = power_law_couplings(L, alpha)
        op = SpinSectorPairOperator(L, base.pack(M, M, 0.0), ndown, _tables=base._tables)
        symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
        with PatchRandn(11800):
            _, psi = symeig.DominantSparseSymeig.apply(op.couplings, k, n)
        return op.correlations(psi)[1][0, L // 2]

    alpha = torch.tensor(2.0, dtype=F64, device=dev(), requires_grad=True)
    c = correlator(alpha)
    (g,) = torch.autograd.grad(c, alpha)
    assert engine.last_cg.converged
    with torch.no_grad():
        fd = (correlator(torch.tensor(2.0 + h, dtype=F64, device=dev())) -
              correlator(torch.tensor(2.0 - h, dtype=F64, device=dev()))).item() / (2 * h)
    err = abs(g.item() - fd) / abs(fd)
    print("<Z_0 Z_5> = %.10f   d/dalpha: autograd %.10f   central difference %.10f   rel %.2e" % (c.item(), g.item(), fd, err))
    assert err < 1e-6


def test_example_long_range():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "spin_lattice", "long_range.py")
    spec = importlib.util.spec_from_file_location("spin_lattice_long_range", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    orig = CG.EPS_DEFAULT
    try:
        out = ex.main(L=12)
        h = 1e-4
        fd = (ex.power_law_energy(12, 2.0 + h, device=dev()) - ex.power_law_energy(12, 2.0 - h, device=dev())) / (2 * h)
    finally:
        CG.EPS_DEFAULT = orig
    print("E0(HS, L = 12) = %.12f (closed form %.12f)   dE0/dalpha: autograd %.9f   central difference %.9f"
          % (out["E0_hs"], out["E0_hs_exact"], out["dE0_dalpha"], fd))
    assert out["n"] == 924 and out["pairs"] == 66
    assert abs(out["E0_hs"] - out["E0_hs_exact"]) < 1e-10 * abs(out["E0_hs_exact"])
    assert abs(out["dE0_dalpha"] - fd) < 1e-5
    zz = out["zz"]
    assert zz.shape == (12, 12) and torch.equal(zz, zz.t())
    assert torch.allclose(out["S_zz"], ring_structure_factor(zz))
    assert abs(out["S_zz"][0].item()) < 1e-10            # sum_i Z_i = 0 in the sector
    assert out["S_zz"][6].item() > out["S_zz"][1].item() > 0.0      # antiferromagnetic: the weight sits at k = pi
