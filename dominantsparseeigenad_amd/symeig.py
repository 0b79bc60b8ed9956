"""Dominant symmetric eigen primitives -- API of reference DominantSparseEigenAD/symeig.py.

    DominantSymeig.apply(A, k[, device])                              reference symeig.py:4-31
    setDominantSparseSymeig(A, Aadjoint_to_gadjoint)                  reference symeig.py:33-88
        -> module attribute ``DominantSparseSymeig``; ``.apply(g, k, dim[, device])``

Extensions the reference lacks (the nev lowest eigenpairs, docs/design/13-lowest-eigenpairs.md):

    LowestSymeig.apply(A, k, nev[, device])                           -> (eigvals (nev,), eigvectors (n, nev))
    setLowestSparseSymeig(A, Aadjoint_to_gadjoint)
        -> module attribute ``LowestSparseSymeig``; ``.apply(g, k, dim, nev[, device])``

forward  = Lanczos with full re-orthogonalisation (HIP on CUDA devices, see Lanczos.py)
backward = projected CG solve of (A - lambda I) x = b (HIP on CUDA devices, see CG.py) followed by the
           user's ``Aadjoint_to_gadjoint(v1, v2)`` hook; the backward is built from differentiable
           pieces (torch glue + the re-entrant CG primitive) so second derivatives work as in the
           reference (examples/TFIM/E0.py:63-64, chiF.py:49-52).
"""
from __future__ import annotations

import torch

from .Lanczos import lowestLanczos, symeigLanczos
from . import CG as _CG
from . import engine as _engine
from ._cpu_plumbing import cg_host_deflated
from ._space import space_of


# A loss that does not depend on the eigenvector (dE0/dg of examples/TFIM/E0.py:62-63, the first backward of every
# second-derivative evaluation) reaches the reference's backward with a ZERO grad_eigvector, and the reference then runs
# a complete CG solve of (A - E0) x = 0 from a random start vector (87-180 mat-vecs) whose result is rounding noise of
# size eps/gap added to the gradient (FIX-OK).  With SKIP_ZERO_RHS the primitives ask autograd
# not to materialise unused output gradients, recognise the case without looking at any data and take x = 0 -- the
# exact solution.  OFF by default: the skipped solve is also absent from the graph, so a SECOND derivative then makes
# one solve (and one random draw) fewer than the reference, and the default keeps the reference's behaviour draw for
# draw; sweeps that want the time back switch it on (examples/TFIM/sweep.py).
SKIP_ZERO_RHS = False


def _draw_and_discard(like):
    torch.randn(like.shape[0], device=like.device, dtype=like.dtype)        # CG.py:58 / :121 (RNG parity)


class DominantSymeig(torch.autograd.Function):
    """Smallest eigenvalue / eigenvector of a real symmetric matrix given as a torch.Tensor."""

    @staticmethod
    def forward(ctx, A, k, device=torch.device("cpu")):
        device = A.device if A.is_cuda else torch.device(device)
        eigval, eigvector = symeigLanczos(A.detach(), k, device=device, extreme="min")   # symeig.py:16
        ctx.save_for_backward(A, eigval, eigvector)
        ctx.device = device
        ctx.set_materialize_grads(False)
        return eigval, eigvector

    @staticmethod
    def backward(ctx, grad_eigval, grad_eigvector):
        A, eigval, eigvector = ctx.saved_tensors
        if grad_eigval is None:
            grad_eigval = torch.zeros_like(eigval)
        if grad_eigvector is None:
            if SKIP_ZERO_RHS:
                _draw_and_discard(eigvector)
                return (grad_eigval * eigvector)[:, None] * eigvector, None, None        # symeig.py:29 with lambda0 = 0
            grad_eigvector = torch.zeros_like(eigvector)
        b = grad_eigvector - torch.matmul(eigvector, grad_eigvector) * eigvector         # symeig.py:27
        if A.is_cuda:
            # the shift is applied inside the CG kernels: no A - lambda*I copy, no n x n identity (symeig.py:25)
            lambda0 = _CG.CGSubspaceShifted.apply(A, eigval, b, eigvector)
        else:
            Aprime = A - eigval * torch.eye(A.shape[0], device=A.device, dtype=A.dtype)  # symeig.py:25
            lambda0 = _CG.CGSubspace.apply(Aprime, b, eigvector)                         # symeig.py:28
        grad_A = (grad_eigval * eigvector - lambda0)[:, None] * eigvector                # symeig.py:29
        return grad_A, None, None


def _make_sparse_symeig(A, Aadjoint_to_gadjoint, cg_cls):
    sp = space_of(A)   # one device: plain torch expressions; row-partitioned operator: global inner products

    class DominantSparseSymeig(torch.autograd.Function):
        """Smallest eigenpair of a matrix-free real symmetric operator depending on parameters g."""

        @staticmethod
        def forward(ctx, g, k, dim, device=torch.device("cpu")):
            device = g.device if g.is_cuda else torch.device(device)
            eigval, eigvector = symeigLanczos(A, k, device=device, extreme="min", sparse=True, dim=dim)  # symeig.py:72-73
            ctx.save_for_backward(g, eigval, eigvector)
            ctx.set_materialize_grads(False)
            return eigval, eigvector

        @staticmethod
        def backward(ctx, grad_eigval, grad_eigvector):
            g, eigval, eigvector = ctx.saved_tensors
            if grad_eigval is None:
                grad_eigval = torch.zeros_like(eigval)
            if grad_eigvector is None:
                if SKIP_ZERO_RHS:
                    _draw_and_discard(eigvector)
                    return Aadjoint_to_gadjoint(sp.scale(grad_eigval, eigvector), eigvector), None, None, None
                grad_eigvector = torch.zeros_like(eigvector)
            b = grad_eigvector - sp.scale(sp.dot(eigvector, grad_eigvector), eigvector)  # symeig.py:80
            lambda0 = cg_cls.apply(g, eigval, b, eigvector)                              # symeig.py:81
            v1, v2 = sp.scale(grad_eigval, eigvector) - lambda0, eigvector               # symeig.py:82-83
            grad_g = Aadjoint_to_gadjoint(v1, v2)                                        # symeig.py:84
            return grad_g, None, None, None

    return DominantSparseSymeig


def setDominantSparseSymeig(A, Aadjoint_to_gadjoint):
    """Publish ``DominantSparseSymeig`` as a module attribute (the reference's protocol, symeig.py:66,87).

    ``A`` is the operator as a callable v -> A v -- either plain torch code or one of the native operators
    of ``dominantsparseeigenad_amd.operators`` (then both loops run without any Python in them);
    ``Aadjoint_to_gadjoint(v1, v2)`` maps the adjoint  A-bar = v1 v2^T  to the adjoint of g."""
    global DominantSparseSymeig
    cg_cls = _CG.setCGSubspaceSparse(A, Aadjoint_to_gadjoint)                            # symeig.py:67-69
    DominantSparseSymeig = _make_sparse_symeig(A, Aadjoint_to_gadjoint, cg_cls)
    return DominantSparseSymeig


# --------------------------------------------------------------------------- the nev lowest eigenpairs
class _FirstOrderOnly(torch.autograd.Function):
    """Identity on the gradient a lowest-nev backward returns; differentiating it again raises (out of scope)."""

    @staticmethod
    def forward(ctx, t, anchor):
        return t.clone()        # (anchor: the primitive's input, so that the result is part of a graph that can be walked)

    @staticmethod
    def backward(ctx, grad):
        raise NotImplementedError("second derivatives through LowestSymeig / LowestSparseSymeig are not implemented "
                                  "(the backward of the lowest-nev primitives is first order only)")


def _first_order(t, anchor):
    if torch.is_grad_enabled() and isinstance(t, torch.Tensor) and anchor.requires_grad:
        return _FirstOrderOnly.apply(t, anchor)
    return t


def _psi_buffer(eigvectors):
    """the (m, ldpsi) device buffer of include/dsea.h (rows 16-byte aligned, ldpsi even)"""
    n, m = eigvectors.shape
    buf = torch.zeros((m, n + (n & 1)), dtype=torch.float64, device=eigvectors.device)
    buf[:, :n] = eigvectors.T
    return buf


def _adjoint_solutions(eigvals, eigvectors, grad_eigvectors, solve):
    """x_j of the adjoint (docs/design/13-lowest-eigenpairs.md): the in-span part in closed form plus y_j, the solution of
    (A - lambda_j) y = P psibar_j on range(P) from ``solve(j, rhs)``; a missing psibar gives x = 0 and no solve."""
    m = eigvals.shape[0]
    xs = []
    for j in range(m):
        if grad_eigvectors is None:
            xs.append(None)
            continue
        g = grad_eigvectors[:, j]
        c = torch.matmul(eigvectors.T, g)
        x = solve(j, g)
        for i in range(m):
            if i != j:
                x = x + (c[i] / (eigvals[i] - eigvals[j])) * eigvectors[:, i]
        xs.append(x)
    return xs


def _make_solver(eigvals, eigvectors, native=None, callable_A=None, eps=None):
    """solve(j, b): (A - lambda_j I) y = P b, y in range(P) -- the deflated CG in HIP on the GPU, in torch on the host"""
    eps = _CG.EPS_DEFAULT if eps is None else eps
    n, m = eigvectors.shape
    if eigvectors.is_cuda:
        Psi = _psi_buffer(eigvectors.detach())
        lam = eigvals.detach().to(torch.float64)

        def solve(j, b):
            x0 = torch.zeros(n, dtype=torch.float64, device=b.device)
            kw = dict(native=native) if native is not None else dict(callable_A=callable_A)
            y = _engine.cg_deflated(b.detach().to(torch.float64), x0, Psi, Psi.shape[1], m, shift=lam[j:j + 1], eps=eps,
                                    maxiter=n, **kw)
            return y.to(eigvectors.dtype)
        return solve
    Psi = eigvectors.detach()

    def solve(j, b):
        lam = eigvals[j].detach()
        amap = lambda v: callable_A(v) - lam * v                       # noqa: E731
        return cg_host_deflated(amap, b.detach(), torch.zeros_like(b), Psi, eps, n, _engine.last_cg)
    return solve


class LowestSymeig(torch.autograd.Function):
    """The nev lowest eigenpairs of a real symmetric matrix given as a torch.Tensor (an extension the reference lacks).

    Returns (eigvals (nev,), eigvectors (n, nev)).  The levels must be non-degenerate up to lambda_nev, the first one not
    requested (a RuntimeWarning says when they are not), and a loss must be invariant under psi_j -> -psi_j for every j.
    First order only: a second backward raises NotImplementedError."""

    @staticmethod
    def forward(ctx, A, k, nev, device=torch.device("cpu")):
        device = A.device if A.is_cuda else torch.device(device)
        eigvals, eigvectors = lowestLanczos(A.detach(), k, nev, device=device)
        ctx.save_for_backward(A, eigvals, eigvectors)
        ctx.set_materialize_grads(False)
        return eigvals, eigvectors

    @staticmethod
    def backward(ctx, grad_eigvals, grad_eigvectors):
        A, eigvals, eigvectors = ctx.saved_tensors
        if grad_eigvals is None:
            grad_eigvals = torch.zeros_like(eigvals)
        with torch.no_grad():
            native, amap = None, (lambda v: torch.matmul(A.detach().to(v.dtype), v))
            if A.is_cuda and _engine.DENSE_SYMMETRIC_KERNEL:
                from .operators import dense_symmetric_operand
                native = dense_symmetric_operand(A.detach())   # the shift stays inside the CG kernels
            solve = _make_solver(eigvals, eigvectors, native=native, callable_A=amap)
            xs = _adjoint_solutions(eigvals, eigvectors, grad_eigvectors, solve)
            grad_A = torch.zeros_like(A)
            for j, x in enumerate(xs):
                v1 = grad_eigvals[j] * eigvectors[:, j]
                if x is not None:
                    v1 = v1 - x
                grad_A += v1[:, None] * eigvectors[:, j]
        return _first_order(grad_A, A), None, None, None


def _make_lowest_sparse(A, Aadjoint_to_gadjoint):
    native = _engine.native_of(A)
    if native is not None and getattr(native, "partitioned", False):
        raise NotImplementedError("the lowest-nev eigenpairs are not implemented for row-partitioned operators "
                                  "(PartitionedTFIMOperator / PartitionedCSROperator)")

    class LowestSparseSymeig(torch.autograd.Function):
        """The nev lowest eigenpairs of a matrix-free real symmetric operator depending on parameters g.  Same conditions
        as ``LowestSymeig``; the hook is called once per pair with (lambdabar_j psi_j - x_j, psi_j) and the results are
        summed (the hook is linear)."""

        @staticmethod
        def forward(ctx, g, k, dim, nev, device=torch.device("cpu")):
            device = g.device if g.is_cuda else torch.device(device)
            eigvals, eigvectors = lowestLanczos(A, k, nev, device=device, sparse=True, dim=dim)
            ctx.save_for_backward(g, eigvals, eigvectors)
            ctx.set_materialize_grads(False)
            return eigvals, eigvectors

        @staticmethod
        def backward(ctx, grad_eigvals, grad_eigvectors):
            g, eigvals, eigvectors = ctx.saved_tensors
            if grad_eigvals is None:
                grad_eigvals = torch.zeros_like(eigvals)
            with torch.no_grad():
                solve = _make_solver(eigvals, eigvectors, native=native if eigvectors.is_cuda else None, callable_A=A)
                xs = _adjoint_solutions(eigvals, eigvectors, grad_eigvectors, solve)
                grad_g = None
                for j, x in enumerate(xs):
                    v1 = grad_eigvals[j] * eigvectors[:, j]
                    if x is not None:
                        v1 = v1 - x
                    gj = Aadjoint_to_gadjoint(v1.contiguous(), eigvectors[:, j].contiguous())
                    grad_g = gj if grad_g is None else grad_g + gj
            return _first_order(grad_g, g), None, None, None, None

    return LowestSparseSymeig


def setLowestSparseSymeig(A, Aadjoint_to_gadjoint):
    """Publish ``LowestSparseSymeig`` as a module attribute (the set-then-attribute protocol of setDominantSparseSymeig).

    ``A`` is the operator as a callable v -> A v (plain torch code or a native operator of
    ``dominantsparseeigenad_amd.operators``); ``Aadjoint_to_gadjoint(v1, v2)`` maps A-bar = v1 v2^T to the adjoint of g."""
    global LowestSparseSymeig
    LowestSparseSymeig = _make_lowest_sparse(A, Aadjoint_to_gadjoint)
    return LowestSparseSymeig
