"""The nev lowest eigenpairs (LowestSymeig / LowestSparseSymeig / lowestLanczos) on host tensors, against torch.linalg.eigh
autograd; argument checks of the new C entries without a device (docs/design/13-lowest-eigenpairs.md)."""
import ctypes
import os
import sys
import warnings
from ctypes import c_double, c_int64, c_void_p

import numpy as np
import pytest
import torch

import DominantSparseEigenAD.CG as CG
import DominantSparseEigenAD.symeig as symeig
from DominantSparseEigenAD.Lanczos import symeigLanczos
from dominantsparseeigenad_amd import _lib
from dominantsparseeigenad_amd.Lanczos import last_lowest, lowestLanczos

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "examples", "TFIM"))


@pytest.fixture
def tight_cg(monkeypatch):
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-13)


def _spectrum_matrix(n, low, seed):
    rng = np.random.RandomState(seed)
    w = np.concatenate([np.asarray(low, dtype=np.float64), 10.0 + 10.0 * rng.rand(n - len(low))])
    U, _ = np.linalg.qr(rng.randn(n, n))
    A = (U * w) @ U.T
    return torch.from_numpy((A + A.T) / 2)


def _loss(vals, vecs, wts, us):
    return (wts * vals).sum() + ((vecs * us).sum(0) ** 2).sum()


def test_dense_lowest_matches_eigh(tight_cg):
    n, k, nev = 300, 120, 4
    A0 = _spectrum_matrix(n, [-3.0, -1.5, 0.0, 1.0, 2.5], 11)
    gen = torch.Generator().manual_seed(3)
    wts = torch.randn(nev, generator=gen, dtype=torch.float64)
    us = torch.randn(n, nev, generator=gen, dtype=torch.float64)

    X = A0.clone().requires_grad_()
    torch.manual_seed(7)
    vals, vecs = symeig.LowestSymeig.apply((X + X.T) / 2, k, nev)
    _loss(vals, vecs, wts, us).backward()

    Xr = A0.clone().requires_grad_()
    w, V = torch.linalg.eigh((Xr + Xr.T) / 2)
    _loss(w[:nev], V[:, :nev], wts, us).backward()

    assert torch.allclose(vals, w[:nev].detach(), rtol=0, atol=1e-9)
    overlap = (vecs.detach() * V[:, :nev].detach()).sum(0).abs()
    assert torch.allclose(overlap, torch.ones(nev, dtype=torch.float64), rtol=0, atol=1e-9)
    assert (X.grad - Xr.grad).abs().max().item() < 1e-9
    assert max(last_lowest.ritz_residuals) < 1e-9
    assert abs(last_lowest.next_eigval - w[nev].item()) < 1e-9


def test_tfim_gap_derivative(tight_cg):
    from TFIM import TFIM
    L, k, nev, g0 = 8, 100, 2, 1.5
    model = TFIM(L)
    model.g = torch.tensor([g0], dtype=torch.float64, requires_grad=True)
    symeig.setLowestSparseSymeig(model.H, model.Hadjoint_to_gadjoint)
    torch.manual_seed(5)
    vals, _ = symeig.LowestSparseSymeig.apply(model.g, k, model.dim, nev)
    gap = vals[1] - vals[0]
    dgap, = torch.autograd.grad(gap, model.g)

    ref = TFIM(L)
    ref.g = torch.tensor([g0], dtype=torch.float64, requires_grad=True)
    ref.setHmatrix()
    w, _ = torch.linalg.eigh(ref.Hmatrix)
    dref, = torch.autograd.grad(w[1] - w[0], ref.g)
    assert abs(gap.item() - (w[1] - w[0]).item()) < 1e-9
    assert abs(dgap.item() - dref.item()) < 1e-8


def test_tfim_eigenvector_loss_matches_eigh(tight_cg):
    """a psi_1-dependent, gauge-invariant loss through the matrix-free primitive (the deflated adjoint solve of pair 1)"""
    from TFIM import TFIM
    L, k, nev, g0 = 8, 120, 2, 1.3
    u = torch.from_numpy(np.random.RandomState(2).randn(1 << L))
    model = TFIM(L)
    model.g = torch.tensor([g0], dtype=torch.float64, requires_grad=True)
    symeig.setLowestSparseSymeig(model.H, model.Hadjoint_to_gadjoint)
    torch.manual_seed(9)
    vals, vecs = symeig.LowestSparseSymeig.apply(model.g, k, model.dim, nev)
    dl, = torch.autograd.grad(vals[1] + (vecs[:, 1] @ u) ** 2, model.g)

    ref = TFIM(L)
    ref.g = torch.tensor([g0], dtype=torch.float64, requires_grad=True)
    ref.setHmatrix()
    w, V = torch.linalg.eigh(ref.Hmatrix)
    dref, = torch.autograd.grad(w[1] + (V[:, 1] @ u) ** 2, ref.g)
    assert abs(dl.item() - dref.item()) < 1e-8 * max(1.0, abs(dref.item()))


def test_nev1_bit_identical_to_symeig_lanczos():
    A = _spectrum_matrix(200, [-2.0, -1.0], 4)
    torch.manual_seed(21)
    e0, v0 = symeigLanczos(A, 80, extreme="min")
    torch.manual_seed(21)
    vals, vecs = lowestLanczos(A, 80, 1)
    assert torch.equal(vals[0], e0)
    assert torch.equal(vecs[:, 0], v0)


def test_degeneracy_warning():
    rng = np.random.RandomState(5)
    n = 24
    w = np.array([0.0, 1.0, 1.0 + 1e-10] + list(3.0 + np.arange(n - 3)))
    U, _ = np.linalg.qr(rng.randn(n, n))
    A = torch.from_numpy((U * w) @ U.T)
    A = (A + A.T) / 2
    torch.manual_seed(0)
    with pytest.warns(RuntimeWarning, match="degenerate"):
        lowestLanczos(A, n, 2)
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        lowestLanczos(A, n, 1)          # lambda_0 < lambda_1 well separated: no warning


def test_argument_errors():
    A = _spectrum_matrix(50, [-1.0, 0.0], 1)
    with pytest.raises(ValueError):
        lowestLanczos(A, 3, 3)          # k < nev + 1
    with pytest.raises(ValueError):
        lowestLanczos(A, 20, 9)         # nev > DSEA_MAX_NEV
    with pytest.raises(NotImplementedError):
        lowestLanczos(A, 20, 2, reorth="none")


def test_second_backward_raises(tight_cg):
    A0 = _spectrum_matrix(60, [-2.0, -1.0, 0.5], 8)
    X = A0.clone().requires_grad_()
    torch.manual_seed(1)
    vals, vecs = symeig.LowestSymeig.apply(X, 40, 2)
    gX, = torch.autograd.grad(vals.sum() + vecs[:, 1].sum() ** 2, X, create_graph=True)
    with pytest.raises(NotImplementedError, match="second derivatives"):
        torch.autograd.grad(gX.sum(), X)


def test_deflated_entries_argument_validation_without_device():
    lib = _lib.load()
    it, res = c_int64(0), c_double(0.0)
    null = c_void_p(None)
    assert lib.dsea_version() >= 141
    for m in (0, 1, 9):
        assert lib.dsea_ritz_combine_block(null, null, 16, 16, 4, null, 4, m, null, 16, null) == -1
        assert lib.dsea_block_project_out(null, null, null, 16, m, null, null, 16, null) == -1
        assert lib.dsea_cg_run_deflated(null, null, null, null, null, null, 16, m, null, 1e-7, 10, 0,
                                        ctypes.byref(it), ctypes.byref(res), null) == -1
        assert lib.dsea_cg_deflated_init(null, null, null, null, null, null, 16, m, null, null, null, 1e-7, 16,
                                         null) == -1
        assert lib.dsea_cg_deflated_step(null, null, null, null, null, null, null, 16, m, null, 1e-7, 0, 16, null) == -1
