"""The matrix-free XYZ spin chain on the GPU (docs/design/14-spin-chain.md): k_spmv_chain and k_chain_forms against the numpy
row formula of tests/chain_reference.py at the smallest sizes that reach each geometric case of a bond (inside the tile,
straddling its edge, both bits far, the wrap bond), then the primitives end to end against torch.linalg.eigh autograd.

    L          tile       path
    2 3 4 5    default    tile = whole vector, the double bond of L = 2, wrap bond inside the tile
    6          2^6        everything inside the tile
    7          2^6        the straddling and the wrap bond are the only far bonds
    8          2^6        first bond with both bits far (6, 7)
    9          2^6        further both-far bonds
    13         2^11       four tiles, bonds (10,11) and (11,12), wrap (12,0)
    19         2^6        8192 tiles > the 4096-block cap: blocks walk several tiles
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import chain_reference as ref  # noqa: E402
from helpers import PatchRandn, unit  # noqa: E402
from dominantsparseeigenad_amd import _lib, engine  # noqa: E402
from dominantsparseeigenad_amd.engine import Workspace, _ptr, _stream  # noqa: E402
from dominantsparseeigenad_amd.operators import SpinChainOperator, TFIMOperator  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402
import dominantsparseeigenad_amd.symeig as symeig  # noqa: E402
import dominantsparseeigenad_amd.CG as CG  # noqa: E402

F64 = torch.float64
TOL = 1e-10
GEOMETRY = [(2, None), (3, None), (4, None), (5, None), (6, 6), (7, 6), (8, 6), (9, 6), (13, None), (19, 6)]
KINDS = ["random", "jy-only", "open"]


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


def couplings(L, kind):
    c = normal_vector(5 * L, 8000 + L).reshape(5, L).copy()
    if kind == "jy-only":
        c[[0, 2, 3, 4]] = 0.0
    elif kind == "open":
        c[:3, L - 1] = 0.0
    return c


@functools.lru_cache(maxsize=None)
def case(L, kind):
    """(couplings, x, H x) on the host, computed once per case and never written to"""
    c = couplings(L, kind)
    x = normal_vector(1 << L, 8100 + L)
    y = ref.apply(L, c, x)
    for a in (c, x, y):
        a.setflags(write=False)
    return c, x, y


@functools.lru_cache(maxsize=None)
def form_case(L):
    v1, v2 = normal_vector(1 << L, 8200 + L), normal_vector(1 << L, 8300 + L)
    out = ref.forms(L, v1, v2)
    for a in (v1, v2, out):
        a.setflags(write=False)
    return v1, v2, out


def operator(L, c, tile):
    op = SpinChainOperator(L, to_dev(c))
    if tile is not None:
        op.set_tile_log2(tile)
    return op


def to_dev(a):
    return torch.from_numpy(np.array(a)).to(dev())      # (a copy: the cached case arrays are read-only)


def relnorm(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("L,tile", GEOMETRY)
def test_matvec_against_the_row_formula(L, tile, kind):
    c, x, want = case(L, kind)
    n = 1 << L
    op = operator(L, c, tile)
    xd = to_dev(x)
    got = op(xd).cpu().numpy()
    err = relnorm(got, want)
    print("L=%d tile=%s %s: |y - ref| / |ref| = %.2e" % (L, tile, kind, err))
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


@pytest.mark.parametrize("L,tile", GEOMETRY)
def test_forms_against_the_reference_sums(L, tile):
    v1, v2, want = form_case(L)
    op = operator(L, couplings(L, "random"), tile)
    a, b = to_dev(v1), to_dev(v2)
    got = op.Hadjoint_to_couplingsadjoint(a, b)
    assert got.shape == (5, L)
    bound = 1e-13 * np.linalg.norm(v1) * np.linalg.norm(v2)
    err = float(np.max(np.abs(got.cpu().numpy() - want)))
    print("L=%d tile=%s: max |form - ref| = %.2e (bound %.2e)" % (L, tile, err, bound))
    assert err <= bound
    again = op.Hadjoint_to_couplingsadjoint(a, b)
    assert torch.equal(got, again)                       # fixed-order reductions, no atomics


def test_matvec_is_symmetric():
    L = 13
    c, x, _ = case(L, "random")
    op = operator(L, c, None)
    v1 = to_dev(x)
    v2 = torch.from_numpy(normal_vector(1 << L, 8400)).to(dev())
    a, b = float(v1 @ op(v2)), float(v2 @ op(v1))
    assert abs(a - b) <= 1e-13 * float(v1.norm() * op(v2).norm() + v2.norm() * op(v1).norm())


def test_tfim_couplings_against_the_tfim_operator():
    L, g = 12, 0.9
    x = torch.from_numpy(normal_vector(1 << L, 8500)).to(dev())
    want = TFIMOperator(L, dev(), g=torch.tensor([g], dtype=F64, device=dev()))(x)
    got = SpinChainOperator.tfim(L, g, dev())(x)
    assert float((got - want).norm() / want.norm()) < 1e-13


@pytest.mark.parametrize("L", [9, 2])
def test_to_csr_is_the_same_matrix(L):
    c, x, want = case(L, "random")
    op = operator(L, c, None)
    csr = op.to_csr()
    assert csr.nnz == (1 << L) * (2 * L + 1 if L > 2 else 4)        # L = 2: the two bonds share a column, summed
    xd = to_dev(x)
    assert relnorm(csr(xd).cpu().numpy(), want) < 1e-13
    assert float((csr(xd) - op(xd)).norm() / op(xd).norm()) < 1e-13


def test_couplings_changed_in_place_are_seen_without_a_new_operator():
    L = 9
    c, x, _ = case(L, "random")
    op = operator(L, c, 6)
    handle = op.handle.value
    xd = to_dev(x)
    op(xd)
    c2 = normal_vector(5 * L, 8600).reshape(5, L)
    with torch.no_grad():
        op.couplings.copy_(torch.from_numpy(c2))
    assert op.handle.value == handle
    assert relnorm(op(xd).cpu().numpy(), ref.apply(L, c2, x)) < 1e-13
    with pytest.raises(ValueError):
        op.couplings = torch.zeros((5, L + 1), dtype=F64, device=dev())
    with pytest.raises(ValueError):
        op.couplings = torch.zeros((5, L), dtype=torch.float32, device=dev())
    with pytest.raises(ValueError):
        SpinChainOperator(1, torch.zeros((5, 1), dtype=F64, device=dev()))


# ---- end to end ------------------------------------------------------------------------------------------------------
def dense_torch(L, c):
    """the dense matrix as a differentiable function of the (5, L) couplings c (CPU): the row formula, entry by entry"""
    n = 1 << L
    s = torch.arange(n, dtype=torch.int64)
    z = [(1 - 2 * ((s >> i) & 1)).to(F64) for i in range(L)]
    H = torch.zeros((n, n), dtype=F64)
    for b in range(L):
        zz = z[b] * z[(b + 1) % L]
        H = H.index_put((s, s), c[2, b] * zz + c[4, b] * z[b], accumulate=True)
        H = H.index_put((s, s ^ (1 << b)), c[3, b].expand(n), accumulate=True)
        H = H.index_put((s, s ^ ((1 << b) | (1 << ((b + 1) % L)))), c[0, b] - c[1, b] * zz, accumulate=True)
    return H


def test_dense_torch_is_the_reference_matrix():
    L = 5
    c = couplings(L, "random")
    assert np.max(np.abs(dense_torch(L, torch.from_numpy(c)).numpy() - ref.dense(L, c))) < 1e-14


def test_ground_state_and_its_gradient_against_eigh(monkeypatch):
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, k, seed = 10, 300, 9103
    n = 1 << L
    c0 = torch.from_numpy(normal_vector(5 * L, seed).reshape(5, L).copy())
    u = unit(n, 9200)
    cr = c0.clone().requires_grad_(True)
    lam, U = torch.linalg.eigh(dense_torch(L, cr))
    assert float(lam[1] - lam[0]) >= 0.02 * float(lam[-1] - lam[0])       # a gap Lanczos resolves with k = 300
    (g_ref,) = torch.autograd.grad(lam[0] + (U[:, 0] @ u) ** 2, cr)
    op = SpinChainOperator(L, c0.to(dev()).requires_grad_(True))
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(9300):
        E0, psi = symeig.DominantSparseSymeig.apply(op.couplings, k, n)
        (g,) = torch.autograd.grad(E0 + (psi @ u.to(dev())) ** 2, op.couplings)
    assert engine.last_cg.converged
    e_err = abs(E0.item() - lam[0].item()) / abs(lam[0].item())
    g_err = float((g.cpu() - g_ref).abs().max()) / float(g_ref.abs().max())
    print("L=10: E0 rel err %.2e   d(E0 + (psi.u)^2)/d couplings: max abs err / max = %.2e" % (e_err, g_err))
    assert g.shape == (5, L)
    assert e_err < 1e-12
    assert g_err < TOL


def test_second_order_along_a_line_of_couplings(monkeypatch):
    """couplings = c0 + t c1: d^2 E0 / dt^2 through the re-entrant mat-vec / forms pair against eigh double backward, at the
    tolerance of the second-order test of tests/test_gpu_csr_param.py"""
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, k = 8, 200
    n = 1 << L
    c0 = torch.from_numpy(normal_vector(5 * L, 9102).reshape(5, L).copy())
    c1 = torch.from_numpy(normal_vector(5 * L, 9120).reshape(5, L).copy())
    tr = torch.tensor(0.0, dtype=F64, requires_grad=True)
    lam, _ = torch.linalg.eigh(dense_torch(L, c0 + tr * c1))
    (r1,) = torch.autograd.grad(lam[0], tr, create_graph=True)
    (r2,) = torch.autograd.grad(r1, tr)
    t = torch.tensor(0.0, dtype=F64, device=dev(), requires_grad=True)
    op = SpinChainOperator(L, (c0.to(dev()) + t * c1.to(dev())))
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
    c0 = torch.from_numpy(normal_vector(5 * L, 9102).reshape(5, L).copy())
    cr = c0.clone().requires_grad_(True)
    lam, _ = torch.linalg.eigh(dense_torch(L, cr))
    spread = float(lam[-1] - lam[0])
    assert float(lam[1] - lam[0]) >= 1e-3 * spread and float(lam[2] - lam[1]) >= 1e-3 * spread
    gap_ref = lam[1] - lam[0]
    (g_ref,) = torch.autograd.grad(gap_ref, cr)
    op = SpinChainOperator(L, c0.to(dev()).requires_grad_(True))
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


def test_tfim_ground_state_energy_is_the_closed_form(monkeypatch):
    import oracle.operators
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, k = 10, 300
    op = SpinChainOperator.tfim(L, 1.0, dev())
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(9600):
        E0, _ = symeig.DominantSparseSymeig.apply(op.couplings, k, 1 << L)
    want = float(oracle.operators.tfim_analytic_E0(L, 1.0))
    assert abs(E0.item() - want) < 1e-12 * abs(want), (E0.item(), want)


def test_example_widens_the_gap():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "spin_chain", "couplings.py")
    spec = importlib.util.spec_from_file_location("spin_chain_couplings", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    orig = CG.EPS_DEFAULT
    try:
        out = ex.main(L=8)
    finally:
        CG.EPS_DEFAULT = orig
    assert len(out["gaps"]) == 11 and out["dE0"].shape == (5, 8)
    assert out["gaps"][-1] > out["gaps"][0]
