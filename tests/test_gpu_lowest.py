"""The nev lowest eigenpairs on the MI355X (docs/design/13-lowest-eigenpairs.md): the block Ritz combine against
dsea_ritz_combine bit for bit, the block projection and the deflated CG against torch fp64, and the primitives
(LowestSymeig / LowestSparseSymeig) against torch.linalg.eigh autograd.

dsea_block_project_out, dsea_cg_deflated_init and dsea_cg_deflated_step are judged one call at a time (odd n, n below a tile
and above 2^21 rows, m = 1 ... DSEA_MAX_NEV, a padded ldpsi) in tests/test_gpu_cg_stages.py; the deflated tests here go
through the restarting driver."""
import os
import subprocess
import sys
from ctypes import byref, c_double, c_int64

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dominantsparseeigenad_amd import _lib, engine  # noqa: E402
from dominantsparseeigenad_amd.engine import Workspace, _ptr, _stream  # noqa: E402
from dominantsparseeigenad_amd.operators import CSROperator, TFIMOperator  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402
from dominantsparseeigenad_amd.Lanczos import last_lowest  # noqa: E402
import dominantsparseeigenad_amd.symeig as symeig  # noqa: E402
import dominantsparseeigenad_amd.CG as CG  # noqa: E402

F64 = torch.float64
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "examples", "TFIM"))


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


@pytest.fixture
def tight_cg(monkeypatch):
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-13)


def _orthonormal_rows(m, n, seed):
    """(m, ldpsi) device buffer with orthonormal rows"""
    ld = n + (n & 1)
    A = torch.from_numpy(normal_vector(m * n, seed).reshape(n, m))
    Qr, _ = torch.linalg.qr(A)
    buf = torch.zeros((m, ld), dtype=F64)
    buf[:, :n] = Qr.T
    return buf.to(dev()), ld


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.timeout(600, method="thread")
@pytest.mark.parametrize("n", [1000, 4097, (1 << 20) + 37])
@pytest.mark.parametrize("k", [3, 64, 200])
def test_ritz_block_bit_identical_per_column(n, k):
    lib = _lib.load()
    ldq = engine.round_up(n, 32)
    Q = torch.zeros((k, ldq), dtype=F64, device=dev())
    Q[:, :n] = torch.randn(k, n, dtype=F64, device=dev(), generator=torch.Generator(dev()).manual_seed(n + k))
    ws = Workspace.get(n, k, dev())
    st = _stream(dev())
    for m in (1, 2, 5, 8):
        S = torch.from_numpy(normal_vector(m * k, 31 * m + k).reshape(m, k)).to(dev())
        ldy = n + (n & 1)
        Y = torch.full((m, ldy), float("nan"), dtype=F64, device=dev())
        _lib.check(lib.dsea_ritz_combine_block(ws.handle, _ptr(Q), ldq, n, k, _ptr(S), k, m, _ptr(Y), ldy, st),
                   "dsea_ritz_combine_block")
        for j in range(m):
            out = torch.empty(n, dtype=F64, device=dev())
            sj = S[j].contiguous()
            _lib.check(lib.dsea_ritz_combine(ws.handle, _ptr(Q), ldq, n, k, _ptr(sj), _ptr(out), st), "dsea_ritz_combine")
            assert torch.equal(Y[j, :n], out), (m, j)


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("n,m", [(n, m) for n in (1, 3, 1000, 4097, 300001) for m in (1, 3, 8) if m <= n])
def test_block_project_out_vs_torch(n, m):
    lib = _lib.load()
    Psi, ld = _orthonormal_rows(m, n, 500 + n + m)
    v = torch.from_numpy(normal_vector(n, 900 + n)).to(dev())
    ws = Workspace.get(n, m + 1, dev())
    out = torch.empty(n, dtype=F64, device=dev())
    coef = torch.empty(m, dtype=F64, device=dev())
    _lib.check(lib.dsea_block_project_out(ws.handle, _ptr(v), _ptr(Psi), ld, m, _ptr(out), _ptr(coef), n, _stream(dev())),
               "dsea_block_project_out")
    P = Psi[:, :n]
    c_ref = P @ v
    ref = v - P.T @ c_ref
    scale = float(v.norm())
    assert float((coef - c_ref).abs().max()) <= 1e-14 * scale
    assert float((out - ref).abs().max()) <= 1e-14 * scale


def _dense_restricted_solve(H, shift, Psi, b):
    """y in range(P) with P (H - shift) y = P b: eigh of H, the components outside span(Psi) only"""
    w, V = torch.linalg.eigh(H)
    P = torch.eye(H.shape[0], dtype=F64, device=H.device) - Psi.T @ Psi
    rhs = P @ b
    c = V.T @ rhs
    keep = (V.T @ Psi.T).abs().max(dim=1).values < 0.5        # eigenvectors not in span(Psi)
    y = V[:, keep] @ (c[keep] / (w[keep] - shift))
    return P @ y


@pytest.mark.timeout(600, method="thread")
@pytest.mark.parametrize("case", ["tfim-L12", "sell-csr"])
def test_cg_run_deflated_vs_dense_solve(case):
    lib = _lib.load()
    if case == "tfim-L12":
        op = TFIMOperator(12, dev(), g=torch.tensor([1.3], dtype=F64, device=dev()))
        n = 1 << 12
        csr = op.to_csr()
    else:
        import scipy.sparse as sp
        n = 3000
        rng = np.random.RandomState(3)
        M = sp.random(n, n, density=4.0 / n, random_state=rng)
        M = M + M.T + sp.diags(np.concatenate([np.arange(4.0), 10.0 + rng.rand(n - 4)]))
        M = M.tocsr()
        op = CSROperator.from_scipy(M, dev())
        csr = op
    rows = torch.repeat_interleave(torch.arange(n, device=dev()), csr.rowptr[1:] - csr.rowptr[:-1])
    H = torch.zeros((n, n), dtype=F64, device=dev()).index_put((rows, csr.colidx.long()), csr.vals.detach(), accumulate=True)
    w, V = torch.linalg.eigh(H)
    m = 2
    ld = n + (n & 1)
    Psi = torch.zeros((m, ld), dtype=F64, device=dev())
    Psi[:, :n] = V[:, :m].T
    b = torch.from_numpy(normal_vector(n, 77)).to(dev())
    for j in range(m):
        shift = w[j:j + 1].contiguous()
        x = torch.from_numpy(normal_vector(n, 78 + j)).to(dev())
        ws = Workspace.get(n, m + 1, dev())
        it, res = c_int64(0), c_double(0.0)
        rc = lib.dsea_cg_run_deflated(op.handle, ws.handle, _ptr(shift), _ptr(b), _ptr(x), _ptr(Psi), ld, m,
                                      _ptr(ws.state), 1e-12, 4 * n, 16, byref(it), byref(res), _stream(dev()))
        _lib.check(rc, "dsea_cg_run_deflated")
        assert res.value < 1e-12
        ref = _dense_restricted_solve(H, float(w[j]), Psi[:, :n], b)
        assert float((x - ref).norm()) <= 1e-10 * float(ref.norm()), float((x - ref).norm() / ref.norm())
        assert float((Psi[:, :n] @ x).norm()) <= 1e-12 * float(x.norm())


# ------------------------------------------------------------------------------------------------ primitives
def _tfim_dense(L, g0):
    from TFIM import TFIM
    ref = TFIM(L, dev())
    ref.g = torch.tensor([g0], dtype=F64, device=dev(), requires_grad=True)
    ref.setHmatrix()
    return ref


@pytest.mark.timeout(600, method="thread")
@pytest.mark.parametrize("L", [10, 12])
def test_tfim_lowest_native_and_callable_vs_eigh(tight_cg, L):
    from TFIM import TFIM
    k, nev, g0 = 160, 2, 1.3
    n = 1 << L
    u = torch.from_numpy(normal_vector(n, 1234)).to(dev())
    ref = _tfim_dense(L, g0)
    w, V = torch.linalg.eigh(ref.Hmatrix)
    dref, = torch.autograd.grad(w[1] - w[0] + (V[:, 1] @ u) ** 2, ref.g)
    grads = []
    for native in (True, False):
        model = TFIM(L, dev())
        model.g = torch.tensor([g0], dtype=F64, device=dev(), requires_grad=True)
        A = model.H if native else (lambda v, m=model: m.H(v).clone())
        symeig.setLowestSparseSymeig(A, model.Hadjoint_to_gadjoint)
        torch.manual_seed(40 + L)
        vals, vecs = symeig.LowestSparseSymeig.apply(model.g, k, n, nev)
        assert torch.allclose(vals, w[:nev].detach(), rtol=0, atol=1e-9)
        dl, = torch.autograd.grad(vals[1] - vals[0] + (vecs[:, 1] @ u) ** 2, model.g)
        assert abs(dl.item() - dref.item()) < 1e-9 * max(1.0, abs(dref.item())), (native, dl.item(), dref.item())
        grads.append(dl.item())
    assert abs(grads[0] - grads[1]) < 1e-12 * max(1.0, abs(grads[0]))


@pytest.mark.timeout(600, method="thread")
def test_csr_lowest_gradient_wrt_vals(tight_cg):
    import scipy.sparse as sp
    n, k, nev = 4096, 200, 4
    rng = np.random.RandomState(8)
    diags = [np.concatenate([np.arange(5.0), 12.0 + 4.0 * rng.rand(n - 5)])]
    offs = [0]
    for o in range(1, 4):
        band = 0.05 * rng.randn(n - o)
        diags += [band, band]
        offs += [o, -o]
    M = sp.diags(diags, offs, shape=(n, n)).tocsr()
    rowptr = torch.from_numpy(M.indptr.astype("int64")).to(dev())
    colidx = torch.from_numpy(M.indices.astype("int32")).to(dev())
    vals0 = torch.from_numpy(M.data.copy()).to(dev())
    vals = vals0.clone().requires_grad_(True)
    op = CSROperator(rowptr, colidx, vals, n)
    u = torch.from_numpy(normal_vector(n, 55)).to(dev())
    wts = torch.tensor([1.0, -0.5, 0.25, 2.0], dtype=F64, device=dev())

    symeig.setLowestSparseSymeig(op, op.Aadjoint_to_valsadjoint_symmetric)
    torch.manual_seed(3)
    ev, vecs = symeig.LowestSparseSymeig.apply(op.vals, k, n, nev)
    g_lz, = torch.autograd.grad((wts * ev).sum() + ((vecs.T @ u) ** 2).sum(), op.vals)

    rows = torch.repeat_interleave(torch.arange(n, device=dev()), rowptr[1:] - rowptr[:-1])
    vr = vals0.clone().requires_grad_(True)
    Hd = torch.zeros((n, n), dtype=F64, device=dev()).index_put((rows, colidx.long()), vr, accumulate=True)
    w, V = torch.linalg.eigh((Hd + Hd.T) / 2)
    g_ref, = torch.autograd.grad((wts * w[:nev]).sum() + ((V[:, :nev].T @ u) ** 2).sum(), vr)
    assert torch.allclose(ev.detach(), w[:nev].detach(), rtol=0, atol=1e-9)
    assert float((g_lz - g_ref).abs().max()) < 1e-9 * max(1.0, float(g_ref.abs().max()))


@pytest.mark.timeout(600, method="thread")
def test_dense_lowest_symeig_vs_eigh(tight_cg):
    n, k, nev = 2048, 160, 3
    rng = np.random.RandomState(12)
    w0 = np.concatenate([[-4.0, -3.0, -1.5, 0.0], 5.0 + 5.0 * rng.rand(n - 4)])
    U, _ = np.linalg.qr(rng.randn(n, n))
    A0 = torch.from_numpy((U * w0) @ U.T).to(dev())
    A0 = (A0 + A0.T) / 2
    u = torch.from_numpy(normal_vector(n * nev, 19).reshape(n, nev)).to(dev())
    X = A0.clone().requires_grad_(True)
    torch.manual_seed(6)
    ev, vecs = symeig.LowestSymeig.apply((X + X.T) / 2, k, nev)
    ((ev * torch.arange(1, nev + 1, device=dev())).sum() + ((vecs * u).sum(0) ** 2).sum()).backward()
    Xr = A0.clone().requires_grad_(True)
    w, V = torch.linalg.eigh((Xr + Xr.T) / 2)
    ((w[:nev] * torch.arange(1, nev + 1, device=dev())).sum() + ((V[:, :nev] * u).sum(0) ** 2).sum()).backward()
    assert torch.allclose(ev.detach(), w[:nev].detach(), rtol=0, atol=1e-9)
    assert float((X.grad - Xr.grad).abs().max()) < 1e-9


@pytest.mark.timeout(900, method="thread")
def test_headline_tfim_L20_gap(tight_cg):
    from TFIM import TFIM
    L, k, nev, g0, h = 20, 200, 2, 1.5, 1e-4
    n = 1 << L
    model = TFIM(L, dev())

    def forward(gval, grad=False):
        model.g = torch.tensor([gval], dtype=F64, device=dev(), requires_grad=grad)
        symeig.setLowestSparseSymeig(model.H, model.Hadjoint_to_gadjoint)
        torch.manual_seed(2024)
        return symeig.LowestSparseSymeig.apply(model.g, k, n, nev)

    vals, _ = forward(g0, grad=True)
    res = list(last_lowest.ritz_residuals)
    dgap, = torch.autograd.grad(vals[1] - vals[0], model.g)
    model.g = torch.tensor([g0], dtype=F64, device=dev())
    symeig.setDominantSparseSymeig(model.H, model.Hadjoint_to_gadjoint)
    torch.manual_seed(2024)
    e0, _ = symeig.DominantSparseSymeig.apply(model.g, k, n)
    assert torch.equal(vals[0], e0)
    assert max(res) <= 1e-10, res
    with torch.no_grad():
        vp, _ = forward(g0 + h)
        vm, _ = forward(g0 - h)
    fd = ((vp[1] - vp[0]) - (vm[1] - vm[0])).item() / (2 * h)
    assert abs(dgap.item() - fd) <= 1e-6 * abs(fd), (dgap.item(), fd)


@pytest.mark.timeout(600, method="thread")
def test_gap_example_on_device():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "TFIM", "gap.py"), "--N", "10", "--points", "3",
                          "--device", "cuda", "--check"], capture_output=True, text=True, timeout=500, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "max |gap - dense|" in out.stdout
