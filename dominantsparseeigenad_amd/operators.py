"""Native (HIP) operators: the user mat-vec ``A(v)`` of the reference as a device kernel.

Each operator is
  * a plain callable ``op(v) -> A v`` on torch tensors, so it can be handed to
    ``setDominantSparseSymeig(A, Aadjoint_to_gadjoint)`` exactly like the Python functions of the
    reference examples (reference examples/TFIM/TFIM.py:91-98, examples/schrodinger1D.py:18-27); the call
    is a differentiable ``torch.autograd.Function`` (backward = the same symmetric kernel), so the
    adjoint hooks built from it stay differentiable for second-order AD;
  * a holder of a C-ABI operator handle (``.handle``), which lets ``Lanczos`` / ``CG_torch`` run the
    whole loop inside libdsea.so without returning to Python per iteration.
"""
from __future__ import annotations

import math
from ctypes import byref, c_int, c_int32, c_int64, c_void_p

import torch

from . import _lib, engine
from ._lib import check

F64 = torch.float64


class _Handle:
    """RAII wrapper of a dsea_op_t."""

    def __init__(self, raw, n, keepalive):
        self.raw, self.n, self.keepalive = raw, int(n), keepalive

    def __del__(self):
        try:
            _lib.load().dsea_op_destroy(self.raw)
        except Exception:
            pass


class _NativeView:
    """minimal (handle, n) pair accepted by engine.* as ``native=``"""

    def __init__(self, h):
        self.handle, self.n = h.raw, h.n
        self._h = h


class _SymmetricApply(torch.autograd.Function):
    """y = M v for a fixed symmetric M given by a handle; dy/dv^T g = M g (re-entrant)."""

    @staticmethod
    def forward(ctx, v, view):
        ctx.view = view
        return engine.spmv(view, v.detach())

    @staticmethod
    def backward(ctx, gy):
        return _SymmetricApply.apply(gy, ctx.view), None


def _cuda_device(name, device, couplings=None, what="operator", index=True):
    """the device of the device object ``name``: ``device``, else the device of the tensor ``couplings``, else "cuda";
    ValueError for a host device.  With ``index``, "cuda" becomes "cuda:<current>", so that tensors on the device compare
    equal (this asks the runtime: host checks that must come first pass ``index=False`` and call again)."""
    if device is None:
        device = couplings.device if torch.is_tensor(couplings) else "cuda"
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("%s is a device %s; use device='cuda'" % (name, what))
    if index and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _csr_regular(cols, vals, n, layout, col16, values):
    """the CSR operand of (n, per) column and value tensors with ``per`` distinct columns in every row, sorted row by row"""
    order = torch.argsort(cols, dim=1)
    cols, vals = torch.gather(cols, 1, order), torch.gather(vals, 1, order)
    rowptr = torch.arange(n + 1, dtype=torch.int64, device=cols.device) * cols.shape[1]
    return CSROperator(rowptr, cols.reshape(-1), vals.reshape(-1).contiguous(), n, layout=layout, col16=col16, values=values)


def _csr_from_coo(rows, cols, vals, n, layout, col16, values):
    """the CSR operand of the entries (rows[k], cols[k], vals[k]), each a list of tensors; no (row, column) is listed twice"""
    rows, cols, vals = torch.cat(rows), torch.cat(cols), torch.cat(vals)
    order = torch.argsort(rows * n + cols)
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=rows.device)
    rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    return CSROperator(rowptr, cols[order], vals[order].contiguous(), n, layout=layout, col16=col16, values=values)


# ------------------------------------------------------------------------------------------ TFIM
class TFIMOperator:
    """H = -sum_i (g sx_i + sz_i sz_{i+1}) on a periodic chain of L sites, dimension 2^L, matrix-free.

    Replaces the index tables of reference examples/TFIM/TFIM.py:39-51 (an (n, L) int64 gather table:
    168 MB and 11.8 s to build at L = 20) by index arithmetic inside the kernel:
        diag_i = -(L - 2 popcount(i xor rotl_L(i,1))),   neighbours  i xor (1 << j).
    Attribute names follow the reference model class: ``N``, ``dim``, ``g``, ``H``, ``pHpg``,
    ``Hadjoint_to_gadjoint``.
    ``L_local`` / ``row_offset`` describe a row slab for the multi-GPU partition (default: all rows).
    """

    _native_methods = ("H", "__call__")

    def __init__(self, N, device=None, g=None, L_local=None, row_offset=0):
        self.N = int(N)
        self.L_local = self.N if L_local is None else int(L_local)
        self.row_offset = int(row_offset)
        self.dim = 1 << self.N
        self.n = 1 << self.L_local
        self.device = _cuda_device("TFIMOperator", device)
        self._g = None
        self._H = None
        lib = _lib.load()
        raw = c_void_p()
        check(lib.dsea_op_create_tfim(self.N, self.L_local, self.row_offset, None, 1.0, 0.0, byref(raw)),
              "dsea_op_create_tfim")
        self._dHdg = _NativeView(_Handle(raw, self.n, None))
        if g is not None:
            self.g = g

    # -- the parameter tensor (reference: ``model.g``, shape (1,), requires_grad; E0.py:95-96)
    @property
    def g(self):
        return self._g

    @g.setter
    def g(self, value):
        if not torch.is_tensor(value):
            value = torch.tensor([float(value)], dtype=F64)
        if value.device != self.device or value.dtype != F64:
            raise ValueError("g must be a float64 tensor on %s" % self.device)
        self._g = value
        lib = _lib.load()
        raw = c_void_p()
        # the kernel reads g through this device pointer: no host sync, and in-place updates of g are seen
        check(lib.dsea_op_create_tfim(self.N, self.L_local, self.row_offset, c_void_p(value.data_ptr()), 0.0, 1.0,
                                      byref(raw)), "dsea_op_create_tfim")
        self._H = _NativeView(_Handle(raw, self.n, value))

    # C-ABI handle of H (what Lanczos / CG use for the in-library loops)
    @property
    def handle(self):
        if self._H is None:
            raise RuntimeError("set the parameter g before using the operator")
        return self._H.handle

    def to_csr(self, layout="sell", col16="auto", values="auto"):
        """The same operator as an explicit device CSR matrix (L + 1 entries per row, int32 columns): the
        "generic sparse operand" form of BASELINE config 2.  Built on the device with index arithmetic."""
        n, L = self.n, self.L_local
        idx = torch.arange(n, dtype=torch.int64, device=self.device)
        gi = idx + self.row_offset
        rot = ((gi << 1) | (gi >> (self.N - 1))) & (self.dim - 1)
        x = gi ^ rot
        pop = torch.zeros_like(x)
        for b in range(self.N):
            pop += (x >> b) & 1
        diag = (-(self.N - 2 * pop)).to(F64)
        cols = torch.empty((n, L + 1), dtype=torch.int64, device=self.device)
        vals = torch.empty((n, L + 1), dtype=F64, device=self.device)
        cols[:, 0], vals[:, 0] = idx, diag
        for j in range(L):
            cols[:, j + 1] = idx ^ (1 << j)
            vals[:, j + 1] = -self._g.detach()
        return _csr_regular(cols, vals, n, layout, col16, values)

    def pHpg(self, v):
        """dH/dg v = -sum_j v[i xor (1<<j)]   (TFIM.py:58-65)"""
        return _SymmetricApply.apply(v, self._dHdg)

    def H(self, v):
        """H v, differentiable in v and in g  (TFIM.py:91-98)"""
        return _TFIMApply.apply(v, self._g, self)

    __call__ = H

    def Hadjoint_to_gadjoint(self, v1, v2):
        """adjoint hook of TFIM.py:100-101:  g-bar = v1^T (dH/dg) v2, shape (1,)"""
        return self.pHpg(v2).matmul(v1)[None]


class _TFIMApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, g, op):
        ctx.op = op
        ctx.save_for_backward(v, g)
        return engine.spmv(op._H, v.detach())

    @staticmethod
    def backward(ctx, gy):
        v, g = ctx.saved_tensors
        op = ctx.op
        gv = _TFIMApply.apply(gy, g, op) if ctx.needs_input_grad[0] else None
        gg = None
        if ctx.needs_input_grad[1]:
            gg = op.pHpg(v).matmul(gy).reshape(g.shape)
        return gv, gg, None


# ------------------------------------------------------------------------------------------ operators linear in a couplings tensor
def _set_tuning(view, log2):
    check(_lib.load().dsea_op_set_tuning(view.handle, _lib.TUNE_TFIM_TILE_LOG2, int(log2)), "dsea_op_set_tuning")
    view.tune_log2 = int(log2)


def _flat_bonds(bonds):
    """the bond list as the flat c_int32 array a0, b0, a1, b1, ... of the create calls"""
    return (c_int32 * (2 * len(bonds)))(*[s for bond in bonds for s in bond])


def _pack(device, values, sizes):
    """coupling families (each a scalar, or ``size`` values) as one contiguous float64 parameter tensor on ``device``"""
    parts = []
    for value, size in zip(values, sizes):
        t = torch.as_tensor(value, dtype=F64).to(device)
        parts.append(t.expand(size) if t.dim() == 0 else t.reshape(size))
    return torch.cat(parts).contiguous()


def _build_sector_tables(L, count, rows, device):
    """(states, lo_rank, hi_base) of the ``rows`` L-bit words with ``count`` set bits, on ``device``: dsea_sector_build_tables"""
    Llo = (L + 1) // 2
    states = torch.empty(rows, dtype=torch.int64, device=device)
    lo_rank = torch.empty(1 << Llo, dtype=torch.int32, device=device)
    hi_base = torch.empty(1 << (L - Llo), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        check(_lib.load().dsea_sector_build_tables(L, count, c_void_p(states.data_ptr()), c_void_p(lo_rank.data_ptr()),
                                                   c_void_p(hi_base.data_ptr()), engine._stream(device)),
              "dsea_sector_build_tables")
    return states, lo_rank, hi_base


def _table_rank(tables, Llo, s):
    """the rank of every word in the int64 device tensor ``s`` among the words of its popcount: the two-table lookup"""
    _, lo_rank, hi_base = tables
    return hi_base[s >> Llo].to(torch.int64) + lo_rank[s & ((1 << Llo) - 1)].to(torch.int64)


def _apply_block(op, X, entry):
    """H X for a device tensor X of shape (n, R) by the block mat-vec ``entry`` of the library, per block of 8, 4, 2 or 1 columns"""
    from .thermal import _as_block, block_pieces
    X = _as_block(op, X, "apply_block")
    apply = getattr(_lib.load(), entry)
    out = []
    for first, w in block_pieces(X.shape[1]):
        Xp = X[:, first:first + w].to(F64).contiguous()
        if Xp.data_ptr() % 16:
            Xp = Xp.clone()
        Yp = torch.empty_like(Xp)
        check(apply(op.handle, w, c_void_p(Xp.data_ptr()), c_void_p(Yp.data_ptr()), engine._stream(Xp.device)), entry)
        out.append(Yp)
    return out[0] if len(out) == 1 else torch.cat(out, dim=1)


class _CouplingsOperator:
    """What the six matrix-free Hamiltonians that are LINEAR in one float64 couplings tensor share
    (docs/design/30-couplings-operator-base.md): the ``couplings`` binding, the handle, the differentiable ``H`` and its adjoint
    hook, and the tuning that a rebinding and an adjoint handle carry over.

    A subclass sets, with host arithmetic first, ``N``, ``n``, ``dim``, ``device`` and whatever its create call reads, then calls
    ``_bind(couplings)``.  It provides
      * ``_families``: the coupling families in the order of the tensor, for the error message;
      * ``_shape``: the shape of the couplings tensor, ``(nparam,)`` unless overridden;
      * ``_create(data) -> (raw, keepalive)``: the library handle whose kernels read the prepared (detached, float64,
        contiguous) tensor ``data`` through its pointer, and what that handle needs alive -- ``data`` itself and the tables;
      * ``_forms_stem`` and ``_forms_sizes``: ``<stem>_forms`` is the library's forms call and ``_forms_sizes`` the integers its
        ``<stem>_forms_scratch_doubles`` takes;
      * ``set_tile_log2`` or ``set_grid_log2`` on ``_set_tune_log2``."""

    _native_methods = ("H", "__call__")

    def _bind(self, couplings):
        self._c = None
        self._H = None
        self._tune_log2 = None
        self.couplings = couplings

    @property
    def _shape(self):
        return (self.nparam,)

    @property
    def couplings(self):
        return self._c

    @couplings.setter
    def couplings(self, value):
        if not torch.is_tensor(value):
            value = torch.as_tensor(value, dtype=F64).to(self.device)
        if value.device != self.device or value.dtype != F64:
            raise ValueError("couplings must be a float64 tensor on %s" % self.device)
        if tuple(value.shape) != self._shape or not value.is_contiguous():
            raise ValueError("couplings must be a contiguous tensor of shape %s: %s" % (self._shape, self._families))
        self._c = value
        self._H = self._view(value)          # the kernels read the couplings through this tensor's pointer
        if self._tune_log2 is not None:
            _set_tuning(self._H, self._tune_log2)

    def _view(self, couplings, like=None):
        """(handle, n) of this Hamiltonian (its geometry and its tables) with the tensor ``couplings`` as couplings; ``like``: a
        view whose tuning the new handle takes over."""
        data = couplings.detach()
        if data.dtype != F64 or not data.is_contiguous():
            data = data.to(F64).contiguous()
        raw, keepalive = self._create(data)
        view = _NativeView(_Handle(raw, self.n, keepalive))
        view.tune_log2 = None
        if like is not None and like.tune_log2 is not None:
            _set_tuning(view, like.tune_log2)
        return view

    def _forms(self, view, v1, v2):
        """all bilinear forms v1^T (dH/dp) v2 in the shape of the couplings (<stem>_forms: one pass, deterministic)"""
        lib = _lib.load()
        v1, v2 = engine.as_vector(v1, view.n), engine.as_vector(v2, view.n)
        need = c_int64()
        sizer = self._forms_stem + "_forms_scratch_doubles"
        check(getattr(lib, sizer)(*self._forms_sizes, byref(need)), sizer)
        scratch = torch.empty(need.value, dtype=F64, device=v1.device)
        out = torch.empty(self._shape, dtype=F64, device=v1.device)
        check(getattr(lib, self._forms_stem + "_forms")(view.handle, c_void_p(v1.data_ptr()), c_void_p(v2.data_ptr()),
                                                        c_void_p(out.data_ptr()), c_void_p(scratch.data_ptr()),
                                                        engine._stream(v1.device)), self._forms_stem + "_forms")
        return out

    def _set_tune_log2(self, log2):
        """the one tuning integer of a handle (DSEA_TUNE_TFIM_TILE_LOG2: the tile of the full-space kernels, the grid cap of the
        sector kernels), kept for the handles of later bindings"""
        _set_tuning(self._H, log2)
        self._tune_log2 = int(log2)

    @property
    def handle(self):
        return self._H.handle

    def H(self, v):
        """H v, differentiable in v and in the couplings"""
        return _CouplingsApply.apply(v, self._c, self, self._H)

    __call__ = H

    def Hadjoint_to_couplingsadjoint(self, v1, v2):
        """adjoint hook: couplings-bar[t] = v1^T (dH/dp_t) v2, in the shape of the couplings"""
        return _CouplingsForms.apply(v1, v2, self, self._H)


class _CouplingsApply(torch.autograd.Function):
    """y = H[c] v of a ``_CouplingsOperator``.  Backward: H[c] gy (symmetric) and the forms(gy, v) -- both re-entrant."""

    @staticmethod
    def forward(ctx, v, c, op, view):
        ctx.op, ctx.view = op, view
        ctx.save_for_backward(v, c)
        return engine.spmv(view, v.detach())

    @staticmethod
    def backward(ctx, gy):
        v, c = ctx.saved_tensors
        gv = _CouplingsApply.apply(gy, c, ctx.op, ctx.view) if ctx.needs_input_grad[0] else None
        gc = _CouplingsForms.apply(gy, v, ctx.op, ctx.view).reshape(c.shape) if ctx.needs_input_grad[1] else None
        return gv, gc, None, None


class _CouplingsForms(torch.autograd.Function):
    """out[t] = v1^T (dH/dp_t) v2 in the shape of the couplings.  H is linear in the couplings, so with the incoming adjoint G as
    couplings the backward is d/dv1 = H[G] v2 and d/dv2 = H[G] v1: the same mat-vec kernel through a second handle on the same
    geometry and tables, which both products share."""

    @staticmethod
    def forward(ctx, v1, v2, op, view):
        ctx.op, ctx.view = op, view
        ctx.save_for_backward(v1, v2)
        return op._forms(view, v1.detach(), v2.detach())

    @staticmethod
    def backward(ctx, G):
        v1, v2 = ctx.saved_tensors
        g1 = g2 = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            G = G.reshape(ctx.op._shape)
            adj = ctx.op._view(G, like=ctx.view)      # the Hamiltonian whose couplings are the adjoint
            if ctx.needs_input_grad[0]:
                g1 = _CouplingsApply.apply(v2, G, ctx.op, adj)
            if ctx.needs_input_grad[1]:
                g2 = _CouplingsApply.apply(v1, G, ctx.op, adj)
        return g1, g2, None, None


# ------------------------------------------------------------------------------------------ XYZ spin chain
class SpinChainOperator(_CouplingsOperator):
    """H = sum_b [Jx_b X_b X_b+1 + Jy_b Y_b Y_b+1 + Jz_b Z_b Z_b+1] + sum_i [hx_i X_i + hz_i Z_i] on a periodic chain of L
    sites, dimension 2^L, matrix-free (docs/design/14-spin-chain.md).  Site i is bit i of the row index, bond b joins sites
    b and (b + 1) mod L; an open chain is J_{L-1} = 0; at L = 2 bonds 0 and 1 join the same two sites and both count.

    ``couplings`` is ONE float64 device tensor of shape (5, L), rows Jx, Jy, Jz, hx, hz -- the parameter (it may require
    grad).  The kernels read it through its device pointer on every launch: in-place optimiser steps are seen, binding another
    tensor rebuilds the handle.  ``H(v)`` is differentiable in v and in ``couplings``;
    ``Hadjoint_to_couplingsadjoint(v1, v2)`` is the hook for ``setDominantSparseSymeig`` / ``setLowestSparseSymeig``: all
    5 L forms v1^T (dH/dp) v2 in one pass.  Both are re-entrant (H is linear in the couplings: the backward of the forms is a
    mat-vec with the incoming (5, L) adjoint as couplings), so second order works as for ``TFIMOperator``.
    Row-partitioned slabs, a fused Lanczos tail and the persistent single-launch forms do not exist for this operator."""

    _families = "rows Jx, Jy, Jz, hx, hz"
    _forms_stem = "dsea_op_chain"

    def __init__(self, L, couplings, device=None):
        self.N = int(L)
        if not 2 <= self.N <= 62:
            raise ValueError("SpinChainOperator needs 2 <= L <= 62, got %d" % self.N)
        self.dim = self.n = 1 << self.N
        self.device = _cuda_device("SpinChainOperator", device, couplings)
        self._forms_sizes = (self.N,)
        self._bind(couplings)

    @property
    def _shape(self):
        return (5, self.N)

    def _create(self, data):
        raw = c_void_p()
        check(_lib.load().dsea_op_create_chain(self.N, c_void_p(data.data_ptr()), byref(raw)), "dsea_op_create_chain")
        return raw, data

    def set_tile_log2(self, tile_log2):
        """log2 of the rows of x a block stages in LDS (6..12; measurement aid, dsea_op_set_tuning)"""
        self._set_tune_log2(tile_log2)

    @classmethod
    def tfim(cls, L, g, device=None):
        """the transverse-field Ising chain of ``TFIMOperator``: Jz = -1, hx = -g"""
        dev = torch.device(device if device is not None else "cuda")
        c = torch.zeros((5, int(L)), dtype=F64, device=dev)
        c[2] = -1.0
        c[3] = -float(g)
        return cls(L, c, dev)

    def to_csr(self, layout="sell", col16="auto", values="auto"):
        """The same matrix as an explicit device CSR operand (2 L + 1 stored entries per row; at L = 2 the two bonds share a
        column and are summed).  Built on the device with index arithmetic."""
        L, n = self.N, self.n
        c = self._c.detach()
        jx, jy, jz, hx, hz = c[0], c[1], c[2], c[3], c[4]
        idx = torch.arange(n, dtype=torch.int64, device=self.device)
        z = [(1 - 2 * ((idx >> i) & 1)).to(F64) for i in range(L)]
        zz = [z[b] * z[(b + 1) % L] for b in range(L)]
        diag = torch.zeros(n, dtype=F64, device=self.device)
        for b in range(L):
            diag = diag + jz[b] * zz[b] + hz[b] * z[b]
        cols, vals = [idx], [diag]
        for i in range(L):
            cols.append(idx ^ (1 << i))
            vals.append(hx[i].expand(n))
        bond = [(jx[b] - jy[b] * zz[b], idx ^ ((1 << b) | (1 << ((b + 1) % L)))) for b in range(L)]
        if L == 2:                                      # bonds 0 and 1: one column, summed
            bond = [(bond[0][0] + bond[1][0], bond[0][1])]
        for v, col in bond:
            cols.append(col)
            vals.append(v)
        return _csr_regular(torch.stack(cols, dim=1), torch.stack(vals, dim=1), n, layout, col16, values)


# ------------------------------------------------------------------------------------------ XYZ spins on a bond list
def ring_bonds(L, distance=1):
    """the L bonds (i, (i + distance) mod L) of a ring, i = 0 .. L - 1 (pure Python; a ring whose distance wraps onto the same
    pair, L = 2 distance, lists that pair twice -- the TFIM convention)"""
    L, distance = int(L), int(distance)
    if L < 2 or distance % L == 0:
        raise ValueError("ring_bonds needs L >= 2 and a distance that is no multiple of L")
    return [(i, (i + distance) % L) for i in range(L)]


def square_bonds(Lx, Ly, periodic=(True, True)):
    """nearest-neighbour bonds of an Lx x Ly square lattice, site = y * Lx + x: for every site its +x bond, then its +y bond
    (pure Python).  An open direction has no bond across its edge; a periodic direction of length 2 lists its bond twice (the
    TFIM convention); a direction of length 1 has no bonds."""
    Lx, Ly = int(Lx), int(Ly)
    if Lx < 1 or Ly < 1:
        raise ValueError("square_bonds needs Lx, Ly >= 1")
    px, py = bool(periodic[0]), bool(periodic[1])
    bonds = []
    for y in range(Ly):
        for x in range(Lx):
            if Lx > 1 and (x + 1 < Lx or px):
                bonds.append((y * Lx + x, y * Lx + (x + 1) % Lx))
            if Ly > 1 and (y + 1 < Ly or py):
                bonds.append((y * Lx + x, ((y + 1) % Ly) * Lx + x))
    return bonds


def _check_bonds(L, bonds):
    """the bond list as a tuple of int pairs; ValueError for what dsea_op_create_lattice refuses"""
    out = tuple((int(a), int(b)) for a, b in bonds)
    if not 1 <= len(out) <= _lib.LATTICE_MAX_BONDS:
        raise ValueError("SpinLatticeOperator needs 1 <= len(bonds) <= %d, got %d" % (_lib.LATTICE_MAX_BONDS, len(out)))
    for a, b in out:
        if not (0 <= a < L and 0 <= b < L) or a == b:
            raise ValueError("bond (%d, %d): two different sites in 0 .. %d are needed" % (a, b, L - 1))
    return out


class SpinLatticeOperator(_CouplingsOperator):
    """H = sum_t [Jx_t X_a X_b + Jy_t Y_a Y_b + Jz_t Z_a Z_b] + sum_i [hx_i X_i + hz_i Z_i] on L sites, dimension 2^L,
    matrix-free, with bond t joining the sites ``bonds[t] = (a_t, b_t)`` of a caller-given list
    (docs/design/16-spin-lattice.md).  Site i is bit i of the row index; (a, b) and (b, a) are the same bond; a repeated bond
    counts each time it is listed; 1 <= len(bonds) <= 128.  ``ring_bonds`` and ``square_bonds`` build common lists.

    ``couplings`` is ONE contiguous float64 device tensor of length 3 nb + 2 L in the order [Jx(nb), Jy(nb), Jz(nb), hx(L),
    hz(L)] -- the parameter (it may require grad; ``pack`` / ``unpack`` convert).  The kernels read it through its device
    pointer on every launch: in-place optimiser steps are seen, binding another tensor rebuilds the handle.  ``H(v)`` is
    differentiable in v and in ``couplings``; ``Hadjoint_to_couplingsadjoint(v1, v2)`` is the hook for
    ``setDominantSparseSymeig`` / ``setLowestSparseSymeig``: all 3 nb + 2 L forms v1^T (dH/dp) v2 in one pass.  Both are
    re-entrant (H is linear in the couplings: the backward of the forms is a mat-vec with the incoming adjoint as couplings),
    so second order works as for ``SpinChainOperator``.
    Row-partitioned slabs, a fused Lanczos tail and the persistent single-launch forms do not exist for this operator."""

    _families = "Jx(nb), Jy(nb), Jz(nb), hx(L), hz(L)"
    _forms_stem = "dsea_op_lattice"

    def __init__(self, L, bonds, couplings, device=None):
        self.N = int(L)
        if not 2 <= self.N <= 62:
            raise ValueError("SpinLatticeOperator needs 2 <= L <= 62, got %d" % self.N)
        self._bonds = _check_bonds(self.N, bonds)
        self.nb = len(self._bonds)
        self.nparam = 3 * self.nb + 2 * self.N
        self.dim = self.n = 1 << self.N
        self.device = _cuda_device("SpinLatticeOperator", device, couplings)
        self._forms_sizes = (self.N, self.nb)
        self._bind(couplings)

    def _create(self, data):
        raw = c_void_p()
        check(_lib.load().dsea_op_create_lattice(self.N, self.nb, _flat_bonds(self._bonds), c_void_p(data.data_ptr()),
                                                 byref(raw)), "dsea_op_create_lattice")
        return raw, data

    @property
    def bonds(self):
        """the bond list as a tuple of (a, b) pairs, in the order of the couplings (read-only)"""
        return self._bonds

    def set_tile_log2(self, tile_log2):
        """log2 of the rows of x a block stages in LDS (6..12; measurement aid, dsea_op_set_tuning)"""
        self._set_tune_log2(tile_log2)

    def pack(self, Jx, Jy, Jz, hx, hz):
        """the five families (scalars, or one value per bond / per site) as one parameter tensor on the operator's device"""
        return _pack(self.device, (Jx, Jy, Jz, hx, hz), (self.nb, self.nb, self.nb, self.N, self.N))

    def unpack(self, t):
        """views (Jx, Jy, Jz, hx, hz) of a parameter tensor"""
        nb, L = self.nb, self.N
        if tuple(t.shape) != (self.nparam,):
            raise ValueError("expected a tensor of shape (%d,)" % self.nparam)
        return t[:nb], t[nb:2 * nb], t[2 * nb:3 * nb], t[3 * nb:3 * nb + L], t[3 * nb + L:]

    def to_csr(self, layout="sell", col16="auto", values="auto"):
        """The same matrix as an explicit device CSR operand: the diagonal, L field columns and one column per distinct bond
        mask (bonds with equal masks are summed into one stored entry).  Built on the device with index arithmetic."""
        L, n = self.N, self.n
        jx, jy, jz, hx, hz = self.unpack(self._c.detach())
        idx = torch.arange(n, dtype=torch.int64, device=self.device)
        z = [(1 - 2 * ((idx >> i) & 1)).to(F64) for i in range(L)]
        diag = torch.zeros(n, dtype=F64, device=self.device)
        for i in range(L):
            diag = diag + hz[i] * z[i]
        by_mask = {}
        for t, (a, b) in enumerate(self._bonds):
            zz = z[a] * z[b]
            diag = diag + jz[t] * zz
            m = (1 << a) | (1 << b)
            v = jx[t] - jy[t] * zz
            by_mask[m] = by_mask[m] + v if m in by_mask else v
        cols, vals = [idx], [diag]
        for i in range(L):
            cols.append(idx ^ (1 << i))
            vals.append(hx[i].expand(n))
        for m, v in by_mask.items():
            cols.append(idx ^ m)
            vals.append(v)
        return _csr_regular(torch.stack(cols, dim=1), torch.stack(vals, dim=1), n, layout, col16, values)


# ------------------------------------------------------------------------------------------ XXZ spins in one S^z sector
def sector_dim(L, ndown):
    """the dimension C(L, ndown) of the sector of L sites with ndown set bits (pure Python)"""
    L, ndown = int(L), int(ndown)
    if L < 0 or not 0 <= ndown <= L:
        raise ValueError("sector_dim needs 0 <= ndown <= L")
    return math.comb(L, ndown)


def sector_states(L, ndown):
    """the L-bit words with ndown set bits as a list of ints in increasing order: the row order of ``SpinSectorOperator``
    (pure Python, Gosper's next word of the same popcount)"""
    n = sector_dim(L, ndown)
    if int(ndown) == 0:
        return [0]
    out, s = [], (1 << int(ndown)) - 1
    for _ in range(n):
        out.append(s)
        low = s & -s
        ripple = s + low
        s = ripple | (((s ^ ripple) >> 2) // low)
    return out


def _check_sector(L, ndown):
    """(L, ndown, n) as ints; ValueError for what dsea_sector_table_sizes refuses -- host arithmetic only"""
    L, ndown = int(L), int(ndown)
    if not 2 <= L <= _lib.SECTOR_MAX_L:
        raise ValueError("SpinSectorOperator needs 2 <= L <= %d, got %d" % (_lib.SECTOR_MAX_L, L))
    if not 1 <= ndown <= L - 1:
        raise ValueError("SpinSectorOperator needs 1 <= ndown <= L - 1 = %d, got %d" % (L - 1, ndown))
    n = math.comb(L, ndown)
    if n > 2 ** 31 - 1:
        raise ValueError("the sector L = %d, ndown = %d has %d rows; ranks are 32-bit: at most 2^31 - 1" % (L, ndown, n))
    return L, ndown, n


class _SectorRows:
    """What the two operators whose rows are the states of one S^z sector share: they carry ``N``, ``ndown``, ``Llo``, ``device``
    and ``_tables = (states, lo_rank, hi_base)``."""

    @property
    def states(self):
        """states[r] = the basis state of row r (int64 device tensor, increasing)"""
        return self._tables[0]

    def rank(self, s):
        """the row of every state in the int64 device tensor ``s`` (states of the sector only): the two-table lookup"""
        return _table_rank(self._tables, self.Llo, s)

    def embed(self, v):
        """the sector vector v as a vector of the full 2^L space (zero outside the sector); L <= 30"""
        if self.N > 30:
            raise ValueError("embed / restrict need L <= 30")
        w = torch.zeros(1 << self.N, dtype=v.dtype, device=v.device)
        return w.index_put((self.states.to(v.device),), v)

    def restrict(self, w):
        """the sector part of a vector of the full 2^L space; L <= 30"""
        if self.N > 30:
            raise ValueError("embed / restrict need L <= 30")
        return w[self.states.to(w.device)]

    def bipartition(self, sites):
        """the ``Bipartition`` of this sector into the sites ``sites`` and the rest, on the operator's rank tables"""
        return Bipartition(self.N, sites, ndown=self.ndown, device=self.device, _tables=self._tables[1:])

    def ladder(self, dst):
        """the ``SpinSectorLadder`` from this sector to the sector of ``dst`` (ndown + 1, ndown or ndown - 1; ``dst`` may be
        this operator), on the two operators' tables"""
        return SpinSectorLadder(self, dst)


class SpinSectorOperator(_SectorRows, _CouplingsOperator):
    """H = sum_t [Jxy_t (X_a X_b + Y_a Y_b) + Jz_t Z_a Z_b] + sum_i hz_i Z_i on L sites, restricted to the states with exactly
    ``ndown`` set bits (total S^z fixed), matrix-free (docs/design/18-spin-sector.md).  Sites, bits and ``bonds`` are those of
    ``SpinLatticeOperator`` (this is its Hamiltonian with Jx = Jy = Jxy and hx = 0); 2 <= L <= 40, 1 <= ndown <= L - 1 and
    n = C(L, ndown) <= 2^31 - 1.  Row r is the r-th such state in increasing integer order: ``states`` (int64, on the device),
    ``sector_states(L, ndown)`` on the host.

    ``couplings`` is ONE contiguous float64 device tensor of length 2 nb + L in the order [Jxy(nb), Jz(nb), hz(L)] -- the
    parameter (it may require grad; ``pack`` / ``unpack`` convert).  The kernels read it through its device pointer on every
    launch: in-place optimiser steps are seen, binding another tensor makes a new handle on the same tables.  ``H(v)`` is
    differentiable in v and in ``couplings``; ``Hadjoint_to_couplingsadjoint(v1, v2)`` is the hook for
    ``setDominantSparseSymeig`` / ``setLowestSparseSymeig``: all 2 nb + L forms in one pass.  Both are re-entrant (H is linear
    in the couplings), so second order works.  The state table and the two rank tables are built once per operator by the
    library's kernels and kept alive by it.  ``embed`` / ``restrict`` convert to and from the 2^L space (L <= 30)."""

    _families = "Jxy(nb), Jz(nb), hz(L)"
    _forms_stem = "dsea_op_sector"

    def __init__(self, L, bonds, couplings, ndown, device=None):
        self.N, self.ndown, n = _check_sector(L, ndown)
        self._bonds = _check_bonds(self.N, bonds)
        self.nb = len(self._bonds)
        self.nparam = 2 * self.nb + self.N
        self.dim = self.n = n
        self.device = _cuda_device("SpinSectorOperator", device, couplings)
        self.Llo = (self.N + 1) // 2
        self._tables = _build_sector_tables(self.N, self.ndown, n, self.device)
        self._forms_sizes = (self.N, self.ndown, self.nb)
        self._bind(couplings)

    def _create(self, data):
        states, lo_rank, hi_base = self._tables
        raw = c_void_p()
        check(_lib.load().dsea_op_create_sector(self.N, self.ndown, self.nb, _flat_bonds(self._bonds), c_void_p(data.data_ptr()),
                                                c_void_p(states.data_ptr()), c_void_p(lo_rank.data_ptr()),
                                                c_void_p(hi_base.data_ptr()), byref(raw)), "dsea_op_create_sector")
        return raw, (data, self._tables)

    @property
    def bonds(self):
        """the bond list as a tuple of (a, b) pairs, in the order of the couplings (read-only)"""
        return self._bonds

    def set_grid_log2(self, grid_log2):
        """log2 of the most blocks a launch uses (6..12, default 12; measurement aid, dsea_op_set_tuning)"""
        self._set_tune_log2(grid_log2)

    def pack(self, Jxy, Jz, hz):
        """the three families (scalars, or one value per bond / per site) as one parameter tensor on the operator's device"""
        return _pack(self.device, (Jxy, Jz, hz), (self.nb, self.nb, self.N))

    def unpack(self, t):
        """views (Jxy, Jz, hz) of a parameter tensor"""
        nb = self.nb
        if tuple(t.shape) != (self.nparam,):
            raise ValueError("expected a tensor of shape (%d,)" % self.nparam)
        return t[:nb], t[nb:2 * nb], t[2 * nb:]

    def apply_block(self, X):
        """H X for a device tensor X of shape (n, R), any R >= 1: all columns in one pass over the rows per block of 8, 4, 2 or
        1 columns (dsea_op_sector_block_apply, docs/design/27-finite-temperature.md); column j equals ``H(X[:, j])`` bit for bit.
        Plain, not differentiable: X is detached."""
        return _apply_block(self, X, "dsea_op_sector_block_apply")

    def pair_operator(self, couplings=None):
        """the ``SpinSectorPairOperator`` of this sector on the operator's tables; ``couplings=None``: zeros, the correlator
        of a state of this (or any other) Hamiltonian of the sector"""
        return SpinSectorPairOperator(self.N, couplings, self.ndown, device=self.device, _tables=self._tables)

    def correlations(self, psi):
        """(xy, zz, z) of the state psi: <X_i X_j + Y_i Y_j> and <Z_i Z_j> for ALL pairs of sites as L x L matrices, and
        <Z_i> (``SpinSectorPairOperator.correlations``); differentiable in psi"""
        return self.pair_operator().correlations(psi)

    def to_csr(self, layout="sell", col16="auto", values="auto"):
        """The sector matrix as an explicit device CSR operand: the diagonal, and for every distinct bond mask one entry in the
        rows that the mask flips (bonds with equal masks are summed).  Built on the device with index arithmetic."""
        n = self.n
        jxy, jz, hz = self.unpack(self._c.detach())
        s = self.states
        rows = torch.arange(n, dtype=torch.int64, device=self.device)
        z = [(1 - 2 * ((s >> i) & 1)).to(F64) for i in range(self.N)]
        diag = torch.zeros(n, dtype=F64, device=self.device)
        for i in range(self.N):
            diag = diag + hz[i] * z[i]
        by_mask = {}
        for t, (a, b) in enumerate(self._bonds):
            diag = diag + jz[t] * (z[a] * z[b])
            m = (1 << a) | (1 << b)
            by_mask[m] = by_mask[m] + 2.0 * jxy[t] if m in by_mask else 2.0 * jxy[t]
        r_all, c_all, v_all = [rows], [rows], [diag]
        for m, v in by_mask.items():
            a, b = [i for i in range(self.N) if (m >> i) & 1]
            flips = rows[((s >> a) ^ (s >> b)) & 1 == 1]
            r_all.append(flips)
            c_all.append(self.rank(s[flips] ^ m))
            v_all.append(v.expand(flips.numel()))
        return _csr_from_coo(r_all, c_all, v_all, n, layout, col16, values)


# ------------------------------------------------------------------------------------------ all-pair XXZ couplings in one S^z sector
def pair_count(L):
    """P = L (L - 1) / 2, the number of site pairs i < j"""
    L = int(L)
    return L * (L - 1) // 2


def pair_index(L, i, j):
    """the position of the pair {i, j}, i != j, in the lexicographic list (0,1), (0,2), ..., (0,L-1), (1,2), ...:
    p = i (2 L - i - 1) / 2 + (j - i - 1) for i < j (pure Python)"""
    L, i, j = int(L), int(i), int(j)
    if i > j:
        i, j = j, i
    if not 0 <= i < j < L:
        raise ValueError("pair_index needs two different sites in 0 .. L - 1 = %d, got %d and %d" % (L - 1, i, j))
    return i * (2 * L - i - 1) // 2 + (j - i - 1)


def power_law_couplings(L, alpha, periodic=False):
    """the strict upper triangle of 1 / d(i, j)^alpha as an L x L float64 matrix, d = |i - j| on the open chain and
    min(|i - j|, L - |i - j|) on the ring; differentiable in ``alpha`` (a tensor, on whose device the matrix lives); pure torch"""
    L = int(L)
    if L < 2:
        raise ValueError("power_law_couplings needs L >= 2")
    alpha = torch.as_tensor(alpha, dtype=F64) if not torch.is_tensor(alpha) else alpha.to(F64)
    idx = torch.arange(L, device=alpha.device)
    d = (idx[:, None] - idx[None, :]).abs()
    if periodic:
        d = torch.minimum(d, L - d)
    d = d.clamp(min=1).to(F64)                 # (the diagonal is cut off below; 1 keeps its gradient finite)
    return torch.triu(torch.exp(-alpha * torch.log(d)), diagonal=1)


def ring_structure_factor(C):
    """S[k] = (1 / L) sum_ij cos(2 pi k (i - j) / L) C[i, j] for k = 0 .. L - 1, of an L x L correlation matrix; pure torch"""
    if C.dim() != 2 or C.shape[0] != C.shape[1]:
        raise ValueError("ring_structure_factor needs a square matrix")
    L = C.shape[0]
    idx = torch.arange(L, device=C.device)
    diff = (idx[:, None] - idx[None, :]).to(C.dtype)
    k = idx.to(C.dtype)
    phase = torch.cos((2.0 * math.pi / L) * k[:, None, None] * diff[None, :, :])
    return (phase * C[None, :, :]).sum(dim=(1, 2)) / L


class SpinSectorPairOperator(_SectorRows, _CouplingsOperator):
    """H = sum_{i<j} [Jxy_ij (X_i X_j + Y_i Y_j) + Jz_ij Z_i Z_j] + sum_i hz_i Z_i on L sites with a coupling on EVERY pair of
    sites, restricted to the states with exactly ``ndown`` set bits, matrix-free (docs/design/22-pair-sector.md).  Rows, bits,
    ``states``, the two rank tables and the limits are those of ``SpinSectorOperator``: 2 <= L <= 40, 1 <= ndown <= L - 1,
    n = C(L, ndown) <= 2^31 - 1.  There is no bond list and no cap on the number of bonds: long-range models (power-law,
    Haldane-Shastry, all-to-all) fit in one handle at every L.

    ``couplings`` is ONE contiguous float64 device tensor of length 2 P + L, P = L (L - 1) / 2, in the order
    [Jxy(P), Jz(P), hz(L)] with the pairs in lexicographic order (0,1), (0,2), ..., (0,L-1), (1,2), ... (``pairs``,
    ``pair_index``); ``pack`` takes scalars, length-P vectors or L x L matrices (strict upper triangle).  ``None`` = zeros: the
    operator is then the correlator of a state.  The kernels read the tensor through its device pointer on every launch:
    in-place optimiser steps are seen, binding another tensor makes a new handle on the same tables.  ``H(v)`` is differentiable
    in v and in ``couplings``; ``Hadjoint_to_couplingsadjoint(v1, v2)`` gives all 2 P + L forms and is the hook for
    ``setDominantSparseSymeig`` / ``setLowestSparseSymeig``.  Both are re-entrant, so second order works.
    ``correlations(v1, v2)`` arranges the forms as the L x L matrices of v1^T (X_i X_j + Y_i Y_j) v2 and v1^T Z_i Z_j v2 and
    the vector v1^T Z_i v2."""

    _families = "Jxy(P), Jz(P), hz(L)"
    _forms_stem = "dsea_op_pairsector"

    def __init__(self, L, couplings, ndown, device=None, _tables=None):
        self.N, self.ndown, n = _check_sector(L, ndown)
        self.npair = pair_count(self.N)
        self.nparam = 2 * self.npair + self.N
        self.dim = self.n = n
        self.device = _cuda_device("SpinSectorPairOperator", device, couplings, index=False)
        if torch.is_tensor(couplings) and tuple(couplings.shape) != (self.nparam,):
            raise ValueError("couplings must have shape (%d,): Jxy(P), Jz(P), hz(L) with P = %d" % (self.nparam, self.npair))
        self.device = _cuda_device("SpinSectorPairOperator", self.device)
        self.Llo = (self.N + 1) // 2
        if _tables is None:
            _tables = _build_sector_tables(self.N, self.ndown, n, self.device)
        self._tables = tuple(_tables)
        self._pairs = tuple((i, j) for i in range(self.N) for j in range(i + 1, self.N))
        self._upper = None
        self._forms_sizes = (self.N, self.ndown)
        self._bind(torch.zeros(self.nparam, dtype=F64, device=self.device) if couplings is None else couplings)

    def _create(self, data):
        states, lo_rank, hi_base = self._tables
        raw = c_void_p()
        check(_lib.load().dsea_op_create_pairsector(self.N, self.ndown, c_void_p(data.data_ptr()), c_void_p(states.data_ptr()),
                                                    c_void_p(lo_rank.data_ptr()), c_void_p(hi_base.data_ptr()), byref(raw)),
              "dsea_op_create_pairsector")
        return raw, (data, self._tables)

    @property
    def pairs(self):
        """the P pairs (i, j), i < j, as a tuple in the order of the couplings (read-only)"""
        return self._pairs

    def pair_index(self, i, j):
        """the position of the pair {i, j} in ``pairs``"""
        return pair_index(self.N, i, j)

    def _upper_index(self):
        """(rows, columns) of the strict upper triangle in pair order, on the device"""
        if self._upper is None:
            iu = torch.tensor([p[0] for p in self._pairs], dtype=torch.int64, device=self.device)
            ju = torch.tensor([p[1] for p in self._pairs], dtype=torch.int64, device=self.device)
            self._upper = (iu, ju)
        return self._upper

    def set_grid_log2(self, grid_log2):
        """log2 of the most blocks a launch uses (6..12, default 12; measurement aid, dsea_op_set_tuning)"""
        self._set_tune_log2(grid_log2)

    def pack(self, Jxy, Jz, hz):
        """the three families as one parameter tensor on the operator's device.  Jxy and Jz: a scalar, one value per pair, or
        an L x L matrix of which the strict upper triangle is read; hz: a scalar or one value per site.  Differentiable."""
        def per_pair(value):
            t = torch.as_tensor(value, dtype=F64).to(self.device)
            if t.dim() == 2:
                if tuple(t.shape) != (self.N, self.N):
                    raise ValueError("a coupling matrix must have shape (%d, %d)" % (self.N, self.N))
                t = t[self._upper_index()]
            return t
        return _pack(self.device, (per_pair(Jxy), per_pair(Jz), hz), (self.npair, self.npair, self.N))

    def unpack(self, t):
        """views (Jxy, Jz, hz) of a parameter tensor"""
        P = self.npair
        if tuple(t.shape) != (self.nparam,):
            raise ValueError("expected a tensor of shape (%d,)" % self.nparam)
        return t[:P], t[P:2 * P], t[2 * P:]

    def correlations(self, v1, v2=None):
        """(xy, zz, z): xy[i, j] = v1^T (X_i X_j + Y_i Y_j) v2 and zz[i, j] = v1^T Z_i Z_j v2 as symmetric L x L matrices (their
        diagonals are 2 v1.v2 and v1.v2), z[i] = v1^T Z_i v2; ``v2=None``: the expectation values of v1.  One forms call, then
        torch indexing; differentiable in v1 and v2."""
        if v2 is None:
            v2 = v1
        f = self.Hadjoint_to_couplingsadjoint(v1, v2)
        fxy, fzz, z = self.unpack(f)
        index = self._upper_index()
        eye = torch.eye(self.N, dtype=F64, device=f.device) * torch.dot(v1.to(F64), v2.to(F64))
        out = []
        for part, weight in ((fxy, 2.0), (fzz, 1.0)):
            upper = torch.zeros((self.N, self.N), dtype=F64, device=f.device).index_put(index, part)
            out.append(upper + upper.t() + weight * eye)      # (x + 0 and 0 + x: the two triangles carry the same bits)
        return out[0], out[1], z

    def to_csr(self, layout="sell", col16="auto", values="auto"):
        """The sector matrix as an explicit device CSR operand: the diagonal, and for every pair one entry in the rows that
        the pair flips.  Built on the device with index arithmetic."""
        n = self.n
        jxy, jz, hz = self.unpack(self._c.detach())
        s = self.states
        rows = torch.arange(n, dtype=torch.int64, device=self.device)
        z = [(1 - 2 * ((s >> i) & 1)).to(F64) for i in range(self.N)]
        diag = torch.zeros(n, dtype=F64, device=self.device)
        for i in range(self.N):
            diag = diag + hz[i] * z[i]
        r_all, c_all, off = [rows], [rows], []
        for t, (a, b) in enumerate(self._pairs):
            diag = diag + jz[t] * (z[a] * z[b])
            flips = rows[((s >> a) ^ (s >> b)) & 1 == 1]
            r_all.append(flips)
            c_all.append(self.rank(s[flips] ^ ((1 << a) | (1 << b))))
            off.append((2.0 * jxy[t]).expand(flips.numel()))
        return _csr_from_coo(r_all, c_all, [diag] + off, n, layout, col16, values)


# ------------------------------------------------------------------------------------------ ladder maps between two S^z sectors
def ring_momentum_weights(L, m):
    """(cos(2 pi m j / L), sin(2 pi m j / L)) / sqrt(L) for j = 0 .. L - 1 as two float64 host tensors: the real and the
    imaginary part of the site weights of the momentum q = 2 pi m / L on a ring (pure torch, no device)"""
    L, m = int(L), int(m)
    if L < 1:
        raise ValueError("ring_momentum_weights needs L >= 1")
    angle = (2.0 * math.pi / L) * ((m * torch.arange(L, dtype=torch.int64)) % L).to(F64)
    return torch.cos(angle) / math.sqrt(L), torch.sin(angle) / math.sqrt(L)


class _SectorLadderBase:
    """What ``SpinSectorLadder`` and ``HubbardLadder`` share (docs/design/38-ladder-parts.md): the argument checks, the
    transpose and the whole call path into libdsea.  A subclass names its family of C entries, ``_entry`` (``dsea_sector_ladder``
    has the entries ``dsea_sector_ladder_apply``, ``_forms``, ``_forms_scratch_doubles``, ``_block_apply``, ``_block_dots`` and
    ``_block_dots_scratch_doubles``), and their leading integer arguments, ``_sector_args()``; its constructor checks its
    operands (``_pair``), then sets ``step``, ``n_src``, ``n_dst`` and ``_tables`` = (states of dst, lo_rank of src, hi_base of
    src)."""

    _entry = None        # the stem of the family's C entries
    _operand = ()        # the attributes an operand must carry, and what to say when one is missing (% (name, attr))
    _no_operand = None

    def _sector_args(self):
        """the integers that open every C entry of the family"""
        raise NotImplementedError

    def _check_operand(self, name, op):
        """the checks of one operand beyond its attributes (ValueError)"""
        raise NotImplementedError

    def _transpose_args(self):
        """the constructor arguments of ``T`` after (dst, src)"""
        return ()

    def _pair(self, src, dst, _transpose):
        """what both constructors ask of (src, dst) and keep of them; ``_grid`` is one list for the ladder and its transpose"""
        for name, op in (("src", src), ("dst", dst)):
            for attr in self._operand:
                if not hasattr(op, attr):
                    raise ValueError(self._no_operand % (name, attr))
            self._check_operand(name, op)
        if int(src.N) != int(dst.N):
            raise ValueError("the two sectors must have the same number of sites, got L = %d and L = %d" % (src.N, dst.N))
        if torch.device(src.device) != torch.device(dst.device):
            raise ValueError("the two sectors must live on the same device, got %s and %s" % (src.device, dst.device))
        self.src, self.dst = src, dst
        self.L = self.N = int(src.N)
        self.device = torch.device(src.device)
        self._T = _transpose
        self._grid = _transpose._grid if _transpose is not None else [0]

    @property
    def T(self):
        """the ladder dst -> src on the same tables: ``lad.T(c, .)`` is the transpose of ``lad(c, .)``"""
        if self._T is None:
            self._T = type(self)(self.dst, self.src, *self._transpose_args(), _transpose=self)
        return self._T

    def _call(self, entry, *args):
        """one C entry of the family on this ladder's sectors: ``args`` follow the sector arguments; tensors go by pointer"""
        name = "%s_%s" % (self._entry, entry)
        args = [c_void_p(a.data_ptr()) if torch.is_tensor(a) else a for a in args]
        check(getattr(_lib.load(), name)(*self._sector_args(), *args), name)

    def _launch(self, entry, lead, operands):
        """``_call`` of a launching entry: ``lead`` (the width, the weights), the three tables, the operands, grid cap, stream"""
        with torch.cuda.device(self.device):
            self._call(entry, *lead, *self._tables, *operands, self._grid[0], engine._stream(self.device))

    def _scratch(self, entry, *width):
        """the scratch of a two-stage entry, sized by the library (``<entry>_scratch_doubles``)"""
        need = c_int64()
        self._call(entry + "_scratch_doubles", *width, byref(need))
        return torch.empty(need.value, dtype=F64, device=self.device)

    def _apply_raw(self, c, x):
        c, x = engine.as_vector(c, self.L), engine.as_vector(x, self.n_src)
        y = torch.empty(self.n_dst, dtype=F64, device=x.device)
        self._launch("apply", (c,), (x, y))
        return y

    def _forms_raw(self, v1, v2):
        v1, v2 = engine.as_vector(v1, self.n_dst), engine.as_vector(v2, self.n_src)
        out = torch.empty(self.L, dtype=F64, device=v1.device)
        self._launch("forms", (), (v1, v2, out, self._scratch("forms")))
        return out

    def apply_block(self, c, X):
        """sum_i c_i O_i X for a device tensor X of shape (n_src, R), any R >= 1: (n_dst, R), in blocks of 8, 4, 2 and 1 columns
        (the family's ``_block_apply`` entry).  Column j equals ``lad(c, X[:, j])`` bit for bit; what a row needs whatever the
        column -- its state word, its table reads, the Hubbard row's division -- is done once for all columns of a block.
        Detached, not differentiable."""
        from .chebyshev import _aligned_piece
        from .thermal import block_pieces
        c = self._weights(c)
        X = self._block(X, self.n_src, "X")
        c = engine.as_vector(c.detach(), self.L)
        out = []
        for first, w in block_pieces(X.shape[1]):
            Yp = torch.empty((self.n_dst, w), dtype=F64, device=self.device)
            self._launch("block_apply", (w, c), (_aligned_piece(X, first, w), Yp))
            out.append(Yp)
        return out[0] if len(out) == 1 else torch.cat(out, dim=1)

    def block_dots(self, c, Lft, X):
        """d[j] = sum_r Lft[r, j] (sum_i c_i O_i X)[r, j] as a device tensor [R], for Lft (n_dst, R) and X (n_src, R), any R >= 1:
        the column dots of ``Lft`` with ``apply_block(c, X)`` without the product block (the family's ``_block_dots`` entry, in
        blocks of 8, 4, 2 and 1 columns; fixed-order sums, identical calls return identical bits).  Detached, not
        differentiable."""
        from .chebyshev import _aligned_piece
        from .thermal import block_pieces
        c = self._weights(c)
        X = self._block(X, self.n_src, "X")
        Lft = self._block(Lft, self.n_dst, "Lft")
        if Lft.shape[1] != X.shape[1]:
            raise ValueError("Lft and X must have the same number of columns, got %d and %d" % (Lft.shape[1], X.shape[1]))
        c = engine.as_vector(c.detach(), self.L)
        out = torch.empty(X.shape[1], dtype=F64, device=self.device)
        for first, w in block_pieces(X.shape[1]):
            piece = torch.empty(w, dtype=F64, device=self.device)
            self._launch("block_dots", (w, c), (_aligned_piece(Lft, first, w), _aligned_piece(X, first, w), piece,
                                                self._scratch("block_dots", w)))
            out[first:first + w] = piece
        return out

    def set_grid_log2(self, grid_log2):
        """log2 of the most blocks a launch uses (6..12, 0 = the default 12; measurement aid), for the ladder and ``T``"""
        g = int(grid_log2)
        if g != 0 and not 6 <= g <= 12:
            raise ValueError("grid_log2 must be 0 or 6 .. 12, got %d" % g)
        self._grid[0] = g

    def _weights(self, c):
        if not torch.is_tensor(c):
            c = torch.as_tensor(c, dtype=F64)
        if c.dim() != 1 or c.numel() != self.L:
            raise ValueError("expected %d site weights, got shape %r" % (self.L, tuple(c.shape)))
        if c.is_complex():
            raise ValueError("the site weights must be real: apply the real and the imaginary part one after the other")
        if c.dtype != F64 or c.device != self.device:
            c = c.to(device=self.device, dtype=F64)
        return c

    def _vector(self, v, n, what):
        if not torch.is_tensor(v) or v.dim() != 1 or v.numel() != n:
            raise ValueError("%s must be a vector of %d elements, got %s" % (what, n, tuple(v.shape) if torch.is_tensor(v) else type(v)))
        if v.device != self.device:
            raise ValueError("%s must live on %s, got %s" % (what, self.device, v.device))
        return v

    def _block(self, X, n, what):
        if not torch.is_tensor(X) or X.dim() != 2 or X.shape[0] != n or X.shape[1] < 1:
            raise ValueError("%s must be a tensor of shape (%d, R) with R >= 1, got %r"
                             % (what, n, tuple(X.shape) if torch.is_tensor(X) else type(X).__name__))
        if X.device != self.device:
            raise ValueError("%s must live on %s, got %s" % (what, self.device, X.device))
        if X.is_complex():
            raise ValueError("%s must be real: the real and the imaginary part are columns of one real block" % what)
        return X.detach().to(F64)

    def __call__(self, c, x):
        """the vector sum_i c_i O_i x of the destination sector, differentiable in c and in x"""
        return _LadderApply.apply(self._weights(c), self._vector(x, self.n_src, "x"), self)

    def forms(self, v1, v2):
        """out[i] = v1^T O_i v2 for every site i, shape (L,): v1 on the destination, v2 on the source; differentiable"""
        return _LadderForms.apply(self._vector(v1, self.n_dst, "v1"), self._vector(v2, self.n_src, "v2"), self)

    def dense(self, c):
        """the n_dst x n_src matrix of ``lad(c, .)``, by applying the map to the columns of the identity (small sectors)"""
        c = self._weights(c)
        eye = torch.eye(self.n_src, dtype=F64, device=self.device)
        return torch.stack([self(c, eye[j]) for j in range(self.n_src)], dim=1)


class SpinSectorLadder(_SectorLadderBase):
    """The site-weighted ladder operators between two magnetisation sectors of the same L sites, matrix-free
    (docs/design/24-dynamics.md).  ``src`` and ``dst`` are ``SpinSectorOperator`` or ``SpinSectorPairOperator`` objects
    (anything that carries the sector tables: ``N``, ``ndown``, ``device``, ``_tables``) with the same L on the same device and
    ``step = dst.ndown - src.ndown`` in {+1, 0, -1}.  Site i is bit i, a set bit is a down spin, z_i = 1 - 2 bit_i; sigma^+- =
    (X +- iY) / 2 have matrix elements 1, sigma^- sets a bit and sigma^+ clears it.  For site weights c (float64 [L]):

        step = +1:  lad(c, x) = sum_i c_i sigma^-_i x        step = -1:  sum_i c_i sigma^+_i x        step = 0:  sum_i c_i Z_i x

    as a vector of the destination sector (``n_dst`` rows) from one of the source sector (``n_src`` rows).  The object builds no
    tables: it reads the two operators' tables and keeps them alive.  ``lad.T`` is the ladder dst -> src on the same tables and
    ``lad.T(c, .)`` the exact transpose of ``lad(c, .)``.  ``lad.forms(v1, v2)[i] = v1^T (d lad / d c_i) v2`` for all sites in
    one pass (v1 on the destination, v2 on the source; deterministic).  Both are differentiable to any order in c and in the
    vectors: the map is bilinear and each of the two ``autograd.Function``s is the other's derivative.  ``dense(c)`` is the
    n_dst x n_src matrix, a test aid for small sectors.  ``apply_block`` and ``block_dots`` are the map and its column dots on
    blocks of columns (dsea_sector_ladder_block_apply and dsea_sector_ladder_block_dots,
    docs/design/35-finite-temperature-dynamics.md): a row's table reads are made once for all columns of a block.  Every
    argument check is host arithmetic before the device is touched and raises ``ValueError``."""

    _entry = "dsea_sector_ladder"
    _operand = ("N", "ndown", "device", "_tables")
    _no_operand = "%s carries no sector tables (no attribute %r): a SpinSectorOperator or a SpinSectorPairOperator is needed"

    def __init__(self, src, dst, _transpose=None):
        self._pair(src, dst, _transpose)
        step = int(dst.ndown) - int(src.ndown)
        if step not in (-1, 0, 1):
            raise ValueError("a ladder changes ndown by +1, 0 or -1, got %d -> %d" % (src.ndown, dst.ndown))
        self.step = step
        self.n_src, self.n_dst = math.comb(self.L, int(src.ndown)), math.comb(self.L, int(dst.ndown))
        self._tables = (dst._tables[0], src._tables[1], src._tables[2])     # states of dst, rank tables of src: kept alive

    def _check_operand(self, name, op):
        _check_sector(op.N, op.ndown)
        if len(op._tables) != 3:
            raise ValueError("%s._tables must be (states, lo_rank, hi_base)" % name)

    def _sector_args(self):
        return self.L, int(self.src.ndown), self.step


class _LadderApply(torch.autograd.Function):
    """y = S(c) x.  Bilinear: with the cotangent gy, c-bar = forms(gy, x) and x-bar = S(c)^T gy, the transposed ladder on the
    same tables -- both re-entrant."""

    @staticmethod
    def forward(ctx, c, x, lad):
        ctx.lad = lad
        ctx.save_for_backward(c, x)
        return lad._apply_raw(c.detach(), x.detach())

    @staticmethod
    def backward(ctx, gy):
        c, x = ctx.saved_tensors
        gc = _LadderForms.apply(gy, x, ctx.lad).reshape(c.shape) if ctx.needs_input_grad[0] else None
        gx = _LadderApply.apply(c, gy, ctx.lad.T) if ctx.needs_input_grad[1] else None
        return gc, gx, None


class _LadderForms(torch.autograd.Function):
    """out[i] = v1^T (dS/dc_i) v2, shape (L,).  S is linear in the weights, so with the cotangent G as weights
    v1-bar = S(G) v2 and v2-bar = S(G)^T v1."""

    @staticmethod
    def forward(ctx, v1, v2, lad):
        ctx.lad = lad
        ctx.save_for_backward(v1, v2)
        return lad._forms_raw(v1.detach(), v2.detach())

    @staticmethod
    def backward(ctx, G):
        v1, v2 = ctx.saved_tensors
        G = G.reshape(ctx.lad.L)
        g1 = _LadderApply.apply(G, v2, ctx.lad) if ctx.needs_input_grad[0] else None
        g2 = _LadderApply.apply(G, v1, ctx.lad.T) if ctx.needs_input_grad[1] else None
        return g1, g2, None


# ------------------------------------------------------------------------------------------ reduced density matrices
RDM_DENSE_MAX_SITES = 12   # dense(): the 2^LA x 2^LA matrix is for tests and small cases


class Bipartition:
    """The sites ``sites`` (A, in the caller's order) against the rest (B) for the vectors of a spin operator on L sites
    (docs/design/21-reduced-density-matrix.md).  ``ndown`` = the sector of ``SpinSectorOperator`` (row r = the r-th state with
    ndown set bits); ``ndown=None`` = the full 2^L space of ``TFIMOperator`` / ``SpinChainOperator`` / ``SpinLatticeOperator``
    (L <= 30).  1 <= len(sites) <= min(L - 1, 16): for a larger A take the complement, it has the same non-zero spectrum.

    Bit k of the A-word a is the bit of site sites[k]; bit k of the B-word b is the bit of the k-th other site.  In a sector
    the reduced density matrix is block diagonal in the number m of set bits inside A: ``blocks`` is the tuple of
    (m, dA, dB), row i of block m the i-th LA-bit word with m set bits in increasing order, column j the j-th LB-bit word with
    ndown - m set bits.  With M_m(x)[i, j] = x[row(a_i, b_j)]:
        cross(x, y)_m = M_m(x) M_m(y)^T        rdm(psi)_m = cross(psi, psi)_m        (psi as given: Tr rho = |psi|^2)
    ``idx`` (int32, n entries, on the device) holds row(a_i, b_j) block after block, j fastest; it is built once here by the
    library's kernel, so build the object once and reuse it.  Everything is differentiable to any order: the forward
    (k_rdm_cross) and its adjoint (k_rdm_pull) are bilinear and each is the other's derivative.  ``ValueError`` for every
    argument the C ABI refuses."""

    def __init__(self, L, sites, ndown=None, device=None, _tables=None):
        L = int(L)
        sites = [int(s) for s in sites]
        LA = len(sites)
        full = ndown is None
        if full:
            if not 2 <= L <= 30:
                raise ValueError("a Bipartition of the full 2^L space needs 2 <= L <= 30, got %d" % L)
        else:
            L, ndown, _ = _check_sector(L, ndown)
        if not 1 <= LA <= min(L - 1, _lib.RDM_MAX_SITES):
            raise ValueError("a Bipartition needs 1 <= len(sites) <= min(L - 1, %d), got %d" % (_lib.RDM_MAX_SITES, LA))
        if len(set(sites)) != LA or min(sites) < 0 or max(sites) >= L:
            raise ValueError("sites must be distinct and in 0 .. L - 1 = %d, got %r" % (L - 1, sites))
        self.N, self.ndown, self.sites = L, (None if full else ndown), tuple(sites)
        self._nd = -1 if full else ndown
        self._sites = (c_int32 * LA)(*sites)
        self.device = _cuda_device("Bipartition", device, what="object")
        lib = _lib.load()
        n, nblk, out_len = c_int64(), c_int(), c_int64()
        table = (c_int64 * (5 * _lib.RDM_MAX_BLOCKS))()
        status = lib.dsea_rdm_sizes(L, self._nd, LA, self._sites, byref(n), byref(nblk), table, byref(out_len))
        if status == _lib.ERR_ARG:
            raise ValueError("the reduced density matrix of %d sites at L = %d, ndown = %r has 2^31 elements or more"
                             % (LA, L, ndown))
        check(status, "dsea_rdm_sizes")
        self.n = self.dim = n.value
        self.out_len = out_len.value
        rows = [tuple(table[5 * c + e] for e in range(5)) for c in range(nblk.value)]
        self.blocks = tuple((m, dA, dB) for m, dA, dB, _, _ in rows)
        self._idx_off = tuple(r[3] for r in rows)
        self._out_off = tuple(r[4] for r in rows)
        need = c_int64()
        status = lib.dsea_rdm_scratch_doubles(L, self._nd, LA, self._sites, byref(need))
        if status == _lib.ERR_UNSUPPORTED:
            raise ValueError("the work list of this Bipartition does not fit 31 bits")
        check(status, "dsea_rdm_scratch_doubles")
        self._scratch_doubles = need.value
        self.idx = torch.empty(self.n, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            if full:
                check(lib.dsea_rdm_build_index_full(L, LA, self._sites, c_void_p(self.idx.data_ptr()),
                                                    engine._stream(self.device)), "dsea_rdm_build_index_full")
            else:
                if _tables is None:
                    _tables = _build_sector_tables(L, ndown, self.n, self.device)[1:]
                lo_rank, hi_base = _tables
                check(lib.dsea_rdm_build_index_sector(L, ndown, LA, self._sites, c_void_p(lo_rank.data_ptr()),
                                                      c_void_p(hi_base.data_ptr()), c_void_p(self.idx.data_ptr()),
                                                      engine._stream(self.device)), "dsea_rdm_build_index_sector")
        self._tile = 0

    def set_tile(self, tile):
        """the tile edge of the forward: 0 = the library's choice, 1 = 16, 2 = 32 (measurement aid)"""
        if int(tile) not in (0, 1, 2):
            raise ValueError("tile must be 0, 1 or 2")
        self._tile = int(tile)

    # ---- the two kernels on flat tensors
    def _vector(self, v):
        if not torch.is_tensor(v) or not v.is_cuda:
            raise ValueError("Bipartition works on device vectors; got %s" % (v.device if torch.is_tensor(v) else type(v)))
        if v.dim() != 1 or v.numel() != self.n:
            raise ValueError("expected a vector of %d elements, got shape %r" % (self.n, tuple(v.shape)))
        if v.dtype != F64:
            raise ValueError("Bipartition works on float64 vectors, got %s" % v.dtype)
        return engine.as_vector(v, self.n)

    def _flat(self, G):
        if not torch.is_tensor(G) or not G.is_cuda:
            raise ValueError("Bipartition works on device tensors")
        if G.numel() != self.out_len:
            raise ValueError("expected %d elements (the blocks, flat), got %d" % (self.out_len, G.numel()))
        if G.dtype != F64:
            raise ValueError("Bipartition works on float64 tensors, got %s" % G.dtype)
        return G.reshape(-1).contiguous()

    def _cross_raw(self, x, y):
        same = x is y or (x.data_ptr() == y.data_ptr() and x.dtype == y.dtype == F64 and x.is_contiguous() and y.is_contiguous())
        x = self._vector(x)
        y = x if same else self._vector(y)
        out = torch.empty(self.out_len, dtype=F64, device=x.device)
        scratch = torch.empty(self._scratch_doubles, dtype=F64, device=x.device)
        check(_lib.load().dsea_rdm_cross(self.N, self._nd, len(self.sites), self._sites, c_void_p(self.idx.data_ptr()),
                                         c_void_p(x.data_ptr()), c_void_p(y.data_ptr()), c_void_p(out.data_ptr()),
                                         c_void_p(scratch.data_ptr()), self._tile, engine._stream(x.device)), "dsea_rdm_cross")
        return out

    def _pull_raw(self, G, y, transpose):
        G, y = self._flat(G), self._vector(y)
        out = torch.empty(self.n, dtype=F64, device=y.device)
        check(_lib.load().dsea_rdm_pull(self.N, self._nd, len(self.sites), self._sites, c_void_p(self.idx.data_ptr()),
                                        c_void_p(G.data_ptr()), c_void_p(y.data_ptr()), c_void_p(out.data_ptr()),
                                        1 if transpose else 0, engine._stream(y.device)), "dsea_rdm_pull")
        return out

    # ---- the public, differentiable interface
    def views(self, flat):
        """the blocks of a flat tensor of ``out_len`` elements as a tuple of (dA, dA) views"""
        return tuple(flat[o:o + dA * dA].view(dA, dA) for o, (_, dA, _) in zip(self._out_off, self.blocks))

    def flatten(self, blocks):
        """one flat tensor from a sequence of (dA, dA) blocks (the layout ``pull`` takes)"""
        return torch.cat([b.reshape(-1) for b in blocks])

    def cross_flat(self, x, y):
        self._vector(x), self._vector(y)
        return _RdmCross.apply(x, y, self)

    def cross(self, x, y):
        """(M_m(x) M_m(y)^T for every block m): 2-D views into one flat float64 tensor"""
        return self.views(self.cross_flat(x, y))

    def rdm_flat(self, psi):
        return self.cross_flat(psi, psi)

    def rdm(self, psi):
        """the blocks rho_m of the reduced density matrix of psi (bitwise symmetric; Tr rho = |psi|^2)"""
        return self.views(self.rdm_flat(psi))

    def pull(self, G, y, transpose=False):
        """the vector whose slices are G_m M_m(y) (G_m^T when ``transpose``); G flat or a sequence of blocks"""
        if not torch.is_tensor(G):
            G = self.flatten(G)
        self._flat(G), self._vector(y)
        return _RdmPull.apply(G, y, self, bool(transpose))

    def _trace(self, flat):
        return sum(torch.diagonal(b).sum() for b in self.views(flat))

    def renyi2(self, psi):
        """S_2 = -log( sum_m |rho_m|_F^2 / (Tr rho)^2 ): no eigendecomposition, smooth"""
        flat = self.rdm_flat(psi)
        return -torch.log((flat * flat).sum() / self._trace(flat) ** 2)

    def spectrum(self, psi):
        """the eigenvalues of rho (not normalised), block after block, ascending inside a block"""
        return torch.cat([torch.linalg.eigvalsh(b) for b in self.rdm(psi)])

    def entropy(self, psi, floor=1e-14):
        """S = -sum lambda log lambda over the eigenvalues of rho / Tr rho above ``floor``; the others contribute neither value
        nor gradient"""
        lam = self.spectrum(psi)
        lam = lam / lam.sum()
        lam = lam[lam.detach() > floor]
        return -(lam * torch.log(lam)).sum()

    def dense(self, psi):
        """the 2^LA x 2^LA reduced density matrix in the basis of the A-words (len(sites) <= 12): the blocks placed by torch"""
        LA = len(self.sites)
        if LA > RDM_DENSE_MAX_SITES:
            raise ValueError("dense() is for len(sites) <= %d" % RDM_DENSE_MAX_SITES)
        blocks = self.rdm(psi)
        if self.ndown is None:
            return blocks[0]
        out = torch.zeros((1 << LA, 1 << LA), dtype=F64, device=blocks[0].device)
        for (m, _, _), b in zip(self.blocks, blocks):
            rows = torch.tensor([a for a in range(1 << LA) if bin(a).count("1") == m], dtype=torch.int64, device=out.device)
            out = out.index_put((rows[:, None], rows[None, :]), b)
        return out


class _RdmCross(torch.autograd.Function):
    """flat = (M_m(x) M_m(y)^T)_m.  Bilinear: with the cotangent G the slices of x-bar are G M(y) and those of y-bar G^T M(x),
    both pulls -- re-entrant."""

    @staticmethod
    def forward(ctx, x, y, part):
        ctx.part = part
        ctx.save_for_backward(x, y)
        return part._cross_raw(x.detach(), y.detach())

    @staticmethod
    def backward(ctx, G):
        x, y = ctx.saved_tensors
        gx = _RdmPull.apply(G, y, ctx.part, False) if ctx.needs_input_grad[0] else None
        gy = _RdmPull.apply(G, x, ctx.part, True) if ctx.needs_input_grad[1] else None
        return gx, gy, None


class _RdmPull(torch.autograd.Function):
    """out with slices G_m M_m(y) (G_m^T M_m(y) when transposed).  Bilinear in (G, y): with the cotangent w, G-bar =
    cross(w, y) (cross(y, w), its transpose, when transposed) and y-bar = pull of w with the other transpose setting."""

    @staticmethod
    def forward(ctx, G, y, part, transpose):
        ctx.part, ctx.transpose = part, transpose
        ctx.save_for_backward(G, y)
        return part._pull_raw(G.detach(), y.detach(), transpose)

    @staticmethod
    def backward(ctx, w):
        G, y = ctx.saved_tensors
        gG = gy = None
        if ctx.needs_input_grad[0]:
            gG = _RdmCross.apply(y, w, ctx.part) if ctx.transpose else _RdmCross.apply(w, y, ctx.part)
            gG = gG.reshape(G.shape)
        if ctx.needs_input_grad[1]:
            gy = _RdmPull.apply(G, w, ctx.part, not ctx.transpose)
        return gG, gy, None, None


# ------------------------------------------------------------------------------------------ XXZ spins in a lattice-symmetry sector
def spin_inversion(L, char):
    """the generator (identity, char, True) of the global spin flip s -> s ^ (2^L - 1) with character ``char`` = +1 / -1 (it needs
    ndown = L / 2 and hz-free or staggered couplings to be a symmetry; docs/design/23-spin-inversion.md)"""
    if char not in (1, -1):
        raise ValueError("spin_inversion: char is +1 or -1")
    return (tuple(range(int(L))), int(char), True)


def ring_symmetries(L, momentum=0, parity=None, spin_flip=None):
    """generators of the symmetry group of an L-site ring as (perm, char) pairs: the translation i -> i + 1 with character +1
    (momentum 0) or -1 (momentum "pi"), and with ``parity`` = +1 / -1 the reflection i -> L - 1 - i with that character; with
    ``spin_flip`` = +1 / -1 also ``spin_inversion(L, spin_flip)``"""
    L = int(L)
    if spin_flip not in (None, 1, -1):
        raise ValueError("ring_symmetries: spin_flip is None, +1 or -1")
    if momentum not in (0, "pi"):
        raise ValueError("ring_symmetries: momentum is 0 or 'pi' (complex characters are out of scope)")
    if parity not in (None, 1, -1):
        raise ValueError("ring_symmetries: parity is None, +1 or -1")
    gens = [(tuple((i + 1) % L for i in range(L)), 1 if momentum == 0 else -1)]
    if parity is not None:
        gens.append((tuple(L - 1 - i for i in range(L)), int(parity)))
    if spin_flip is not None:
        gens.append(spin_inversion(L, spin_flip))
    return gens


def torus_symmetries(Lx, Ly, kx=0, ky=0, spin_flip=None):
    """generators of the translation group of the Lx x Ly torus of ``square_bonds`` (site = y * Lx + x): the x translation with
    character +1 (kx = 0) or -1 (kx = "pi"), and the y translation likewise; with ``spin_flip`` = +1 / -1 also
    ``spin_inversion(Lx * Ly, spin_flip)``"""
    Lx, Ly = int(Lx), int(Ly)
    if spin_flip not in (None, 1, -1):
        raise ValueError("torus_symmetries: spin_flip is None, +1 or -1")
    if kx not in (0, "pi") or ky not in (0, "pi"):
        raise ValueError("torus_symmetries: kx and ky are 0 or 'pi' (complex characters are out of scope)")
    tx = tuple(y * Lx + (x + 1) % Lx for y in range(Ly) for x in range(Lx))
    ty = tuple(((y + 1) % Ly) * Lx + x for y in range(Ly) for x in range(Lx))
    gens = [(tx, 1 if kx == 0 else -1), (ty, 1 if ky == 0 else -1)]
    if spin_flip is not None:
        gens.append(spin_inversion(Lx * Ly, spin_flip))
    return gens


def _close_group(L, generators, flips=False):
    """the group generated by ``generators`` as a list of (perm, char), the identity first, in breadth-first order; with
    ``flips`` the pair (that list, the list of the elements' flip bits).  A generator is (perm, char) or (perm, char, flip); an
    element is a permutation together with its flip bit, composition multiplies the characters and XORs the flips.  ValueError
    for a generator of another length, a perm that is no permutation of 0 .. L - 1, a flip other than a bool / 0 / 1, a character
    other than +-1 or one that is not consistent, and for more than DSEA_SYMSECTOR_MAX_GROUP elements -- host arithmetic only"""
    gens = []
    for gen in generators:
        gen = tuple(gen)
        if len(gen) not in (2, 3):
            raise ValueError("a generator is (perm, char) or (perm, char, flip)")
        perm, char, flip = gen if len(gen) == 3 else gen + (False,)
        perm = tuple(int(v) for v in perm)
        if sorted(perm) != list(range(L)):
            raise ValueError("a generator's perm must be a permutation of 0 .. %d" % (L - 1))
        if char not in (1, -1):
            raise ValueError("a generator's character must be +1 or -1 (real one-dimensional irreps only)")
        if isinstance(flip, (float, str, bytes)) or not any(flip is v or flip == v for v in (False, True)):
            raise ValueError("a generator's flip must be a bool (or 0 / 1)")
        gens.append(((perm, bool(flip)), int(char)))
    ident = (tuple(range(L)), False)
    chars = {ident: 1}
    order, frontier = [ident], [ident]
    while frontier:
        new = []
        for p in frontier:
            for q, d in gens:
                r = (tuple(q[0][p[0][i]] for i in range(L)), p[1] != q[1])            # p first, then q
                e = chars[p] * d
                if r not in chars:
                    if len(order) >= _lib.SYMSECTOR_MAX_GROUP:
                        raise ValueError("the symmetry group has more than %d elements" % _lib.SYMSECTOR_MAX_GROUP)
                    chars[r] = e
                    order.append(r)
                    new.append(r)
                elif chars[r] != e:
                    raise ValueError("the character is not consistent: one group element is reached with both signs")
        frontier = new
    group = [(p[0], chars[p]) for p in order]
    return (group, [p[1] for p in order]) if flips else group


def _check_flips(L, ndown, flips):
    """ValueError when an element flips the spins outside the sector that the flip maps onto itself"""
    if any(flips) and 2 * ndown != L:
        raise ValueError("a group element with a spin flip needs ndown = L / 2 (got L = %d, ndown = %d)" % (L, ndown))


def _site_signs(L, group, flips):
    """eps_i in {+1, -1, 0} of the signed orbit mean of hz: 0 on a site orbit one of whose sites is fixed by a flipped element,
    otherwise +1 on the orbit's lowest site i0 and sgn(g) = -1 (flipped) / +1 on perm_g[i0] (path independent: two elements that
    carry i0 to the same site with different flips would compose to a flipped element fixing i0)"""
    low = [min(perm[i] for perm, _ in group) for i in range(L)]
    dead = {low[i] for (perm, _), flip in zip(group, flips) if flip for i in range(L) if perm[i] == i}
    eps = [0] * L
    for i0 in range(L):
        if low[i0] == i0 and i0 not in dead:
            for (perm, _), flip in zip(group, flips):
                eps[perm[i0]] = -1 if flip else 1
    return eps


def _orbit_ids(L, bonds, group):
    """orbit id per parameter [Jxy(nb), Jz(nb), hz(L)], numbered by first appearance inside each family; ValueError when a group
    element does not map the bond set onto itself or a pair is listed twice"""
    pairs = [frozenset(b) for b in bonds]
    index = {}
    for t, pair in enumerate(pairs):
        if pair in index:
            raise ValueError("bond (%d, %d) is listed twice: SpinSymmetrySectorOperator refuses repeated bonds" % bonds[t])
        index[pair] = t
    low_b, low_s = list(range(len(bonds))), list(range(L))
    for perm, _ in group:
        for t, (a, b) in enumerate(bonds):
            image = index.get(frozenset((perm[a], perm[b])))
            if image is None:
                raise ValueError("a group element maps bond (%d, %d) off the bond list" % (a, b))
            low_b[t] = min(low_b[t], image)
        for i in range(L):
            low_s[i] = min(low_s[i], perm[i])
    # the smallest image is a canonical label because G is a group; closing it transitively keeps that true for any input
    for low in (low_b, low_s):
        for i in range(len(low)):
            while low[low[i]] != low[i]:
                low[i] = low[low[i]]
    def number(low):
        ids = {}
        return [ids.setdefault(v, len(ids)) for v in low]
    ob, os_ = number(low_b), number(low_s)
    nob = max(ob) + 1
    return ob + [nob + v for v in ob] + [2 * nob + v for v in os_]


def _apply_perm(perm, s):
    t = 0
    for i, to in enumerate(perm):
        if (s >> i) & 1:
            t |= 1 << to
    return t


def symmetry_sector_dim(L, ndown, generators):
    """the number of rows of ``SpinSymmetrySectorOperator``: the orbits of the sector under the generated group whose
    sigma = sum over the stabiliser of chi is not 0 (pure Python, for small L)"""
    L, ndown = int(L), int(ndown)
    group, flips = _close_group(L, generators, flips=True)
    _check_flips(L, ndown, flips)
    full = (1 << L) - 1
    count = 0
    for s in sector_states(L, ndown):
        images = [_apply_perm(perm, s) ^ (full if flip else 0) for (perm, _), flip in zip(group, flips)]
        if min(images) == s and sum(c for (_, c), im in zip(group, images) if im == s) != 0:
            count += 1
    return count


class SpinSymmetrySectorOperator(_CouplingsOperator):
    """The Hamiltonian of ``SpinSectorOperator`` (same bits, bonds and parameter tensor [Jxy(nb), Jz(nb), hz(L)]) restricted
    further to one sector of a lattice-symmetry group G with a real one-dimensional character, matrix-free
    (docs/design/20-symmetry-sector.md).  ``generators`` is a list of (perm, char): perm[i] is the site that site i is sent to,
    char is +1 or -1 (``ring_symmetries`` / ``torus_symmetries`` build the usual ones).  The host closes the group and raises
    ValueError, before anything touches the device, for a perm that is no permutation, an inconsistent character, more than 128
    elements, a group element that does not map the bond set onto itself, and a bond listed twice.

    Row r is the r-th orbit representative (the smallest state of its orbit) with sigma_r = sum over its stabiliser of chi != 0,
    in increasing integer order: ``states`` and ``norms`` on the device.  The matrix is B^T H_sector(p) B with
    |r> = (|G| sigma_r)^(-1/2) sum_g chi(g) |g s_r>, for any couplings: they enter through their orbit means (``symmetrise``).
    ``H(v)`` is differentiable in v and in ``couplings``; ``Hadjoint_to_couplingsadjoint(v1, v2)`` returns all 2 nb + L entries in
    one pass; both are re-entrant (second order works).  The couplings are read through the tensor's pointer on every launch;
    binding another tensor makes a new handle on the same tables.  The hook returns couplings-bar = S raw with
    raw[t] = v1^T A_t v2: H_sym is linear in the couplings and sees them through S, which is symmetric, so with an incoming
    adjoint G as couplings the backward of the forms is d/dv1 = H_sym[G] v2 and d/dv2 = H_sym[G] v1.

    Spin inversion (docs/design/23-spin-inversion.md): a generator may also be (perm, char, flip); with ``flip`` the element acts
    as g(s) = perm(s) ^ (2^L - 1) (``spin_inversion``, or ``spin_flip=`` of the builders).  It needs ndown = L / 2 (ValueError
    otherwise).  ``flips`` holds the flip bit of every element of ``group``; hz then enters through the signed orbit mean with the
    signs ``site_signs``.  Without a flipped generator the operator is exactly the one above."""

    _families = "Jxy(nb), Jz(nb), hz(L)"
    _forms_stem = "dsea_op_symsector"
    SLAB_ROWS = 1 << 26

    def __init__(self, L, bonds, couplings, ndown, generators, device=None):
        self.N, self.ndown, self.n_sector = _check_sector(L, ndown)
        self._bonds = _check_bonds(self.N, bonds)
        self.nb = len(self._bonds)
        self.nparam = 2 * self.nb + self.N
        group, flips = _close_group(self.N, generators, flips=True)
        _check_flips(self.N, self.ndown, flips)
        self._group, self._flips = tuple(group), tuple(flips)
        self.ng = len(self._group)
        self._orbits = tuple(_orbit_ids(self.N, self._bonds, self._group))
        self._site_signs = tuple(_site_signs(self.N, self._group, self._flips))
        self._has_flip = any(self._flips)
        self.device = _cuda_device("SpinSymmetrySectorOperator", device, couplings)
        self.Llo = (self.N + 1) // 2
        self.nsl = (self.N + 7) // 8
        lib = _lib.load()
        stream = engine._stream(self.device)
        chars = (c_int32 * self.ng)(*[c for _, c in self._group])
        perms = (c_int32 * (self.ng * self.N))(*[v for perm, _ in self._group for v in perm])
        perm_tab = torch.empty(self.ng * self.nsl * 256, dtype=torch.int64, device=self.device)
        kept = []
        with torch.cuda.device(self.device):
            check(lib.dsea_symsector_fill_perm(self.N, self.ng, perms, c_void_p(perm_tab.data_ptr()), stream),
                  "dsea_symsector_fill_perm")
            for first in range(0, self.n_sector, self.SLAB_ROWS):
                count = min(self.SLAB_ROWS, self.n_sector - first)
                slab = torch.empty(count, dtype=torch.int64, device=self.device)
                if self._has_flip:
                    flipbits = (c_int32 * self.ng)(*[int(f) for f in self._flips])
                    check(lib.dsea_symsector_classify_flip(self.N, self.ndown, self.ng, chars, flipbits,
                                                           c_void_p(perm_tab.data_ptr()), first, count, c_void_p(slab.data_ptr()),
                                                           stream), "dsea_symsector_classify_flip")
                else:
                    check(lib.dsea_symsector_classify(self.N, self.ndown, self.ng, chars, c_void_p(perm_tab.data_ptr()), first,
                                                      count, c_void_p(slab.data_ptr()), stream), "dsea_symsector_classify")
                kept.append(slab[slab != 0])
            reps = torch.cat(kept).contiguous()
            del kept
            self.dim = self.n = int(reps.numel())
            if self.n < 1:
                raise ValueError("the symmetry sector is empty: every orbit has sigma = 0")
            bucket = torch.empty((1 << (self.N - self.Llo)) + 1, dtype=torch.int32, device=self.device)
            check(lib.dsea_symsector_fill_buckets(self.N, self.n, c_void_p(reps.data_ptr()), c_void_p(bucket.data_ptr()), stream),
                  "dsea_symsector_fill_buckets")
        self._tables = (reps, bucket, perm_tab)
        self._states = reps & ((1 << 48) - 1)
        self._norms = reps >> 48
        self._orbit_index = torch.tensor(self._orbits, dtype=torch.int64, device=self.device)
        self._chars = torch.tensor([c for _, c in self._group], dtype=F64, device=self.device)
        full = (1 << self.N) - 1
        self._flip_masks = torch.tensor([full if f else 0 for f in self._flips], dtype=torch.int64, device=self.device)
        self._param_signs = torch.tensor([1.0] * (2 * self.nb) + [float(e) for e in self._site_signs], dtype=F64,
                                         device=self.device)
        self._sector_tables = None
        self._forms_sizes = (self.n, self.N, self.nb)
        self._bind(couplings)

    def _create(self, data):
        lib = _lib.load()
        flat = _flat_bonds(self._bonds)
        chars = (c_int32 * self.ng)(*[c for _, c in self._group])
        orbits = (c_int32 * self.nparam)(*self._orbits)
        reps, bucket, perm_tab = self._tables
        raw = c_void_p()
        if self._has_flip:
            flips = (c_int32 * self.ng)(*[int(f) for f in self._flips])
            signs = (c_int32 * self.N)(*self._site_signs)
            check(lib.dsea_op_create_symsector_flip(self.N, self.ndown, self.nb, flat, c_void_p(data.data_ptr()), self.ng, chars,
                                                    flips, signs, orbits, self.n, c_void_p(reps.data_ptr()),
                                                    c_void_p(bucket.data_ptr()), c_void_p(perm_tab.data_ptr()), byref(raw)),
                  "dsea_op_create_symsector_flip")
        else:
            check(lib.dsea_op_create_symsector(self.N, self.ndown, self.nb, flat, c_void_p(data.data_ptr()), self.ng, chars,
                                               orbits, self.n, c_void_p(reps.data_ptr()), c_void_p(bucket.data_ptr()),
                                               c_void_p(perm_tab.data_ptr()), byref(raw)), "dsea_op_create_symsector")
        return raw, (data, self._tables)

    @property
    def bonds(self):
        """the bond list as a tuple of (a, b) pairs, in the order of the couplings (read-only)"""
        return self._bonds

    @property
    def group(self):
        """the closed group as a tuple of (perm, char), the identity first"""
        return self._group

    @property
    def flips(self):
        """flips[g]: whether element g of ``group`` also flips every spin (a tuple of bools)"""
        return self._flips

    @property
    def site_signs(self):
        """eps_i in {+1, -1, 0}: the signed orbit mean of hz is eps_i times the mean of eps_j hz_j over the orbit of site i (all +1
        without a flipped element)"""
        return self._site_signs

    @property
    def orbits(self):
        """orbit id per parameter, in the order of the couplings: equal ids = one orbit under the group"""
        return self._orbits

    @property
    def states(self):
        """states[r] = the representative of row r (int64 device tensor, increasing)"""
        return self._states

    @property
    def norms(self):
        """norms[r] = sigma_r, the size of the representative's stabiliser (int64 device tensor)"""
        return self._norms

    def set_grid_log2(self, grid_log2):
        """log2 of the most blocks a launch uses (6..12, default 12; measurement aid, dsea_op_set_tuning)"""
        self._set_tune_log2(grid_log2)

    pack = SpinSectorOperator.pack
    unpack = SpinSectorOperator.unpack

    def symmetrise(self, p):
        """S p: every coupling replaced by the mean over its orbit, for hz under flipped elements the signed mean
        eps_i mean(eps_j hz_j) (torch, differentiable)"""
        if self._has_flip:
            sign = self._param_signs.to(device=p.device, dtype=p.dtype)
            idx = self._orbit_index.to(p.device)
            size = int(idx.max()) + 1
            sums = torch.zeros(size, dtype=p.dtype, device=p.device).index_add(0, idx, sign * p)
            counts = torch.zeros(size, dtype=p.dtype, device=p.device).index_add(0, idx, torch.ones_like(p))
            return sign * (sums / counts)[idx]
        idx = self._orbit_index.to(p.device)
        size = int(idx.max()) + 1
        sums = torch.zeros(size, dtype=p.dtype, device=p.device).index_add(0, idx, p)
        counts = torch.zeros(size, dtype=p.dtype, device=p.device).index_add(0, idx, torch.ones_like(p))
        return (sums / counts)[idx]

    def row_of(self, s):
        """the row of every state in the int64 device tensor ``s``, -1 for a state that is no stored representative"""
        s = torch.as_tensor(s, dtype=torch.int64, device=self.device)
        pos = torch.searchsorted(self._states, s).clamp(max=self.n - 1)
        return torch.where(self._states[pos] == s, pos, torch.full_like(pos, -1))

    def _images(self, s):
        """g(s) for every group element: an (|G|, len(s)) int64 tensor, from perm_tab by torch indexing (and the flips)"""
        tab = self._tables[2].view(self.ng, self.nsl, 256)
        out = torch.zeros((self.ng, s.numel()), dtype=torch.int64, device=self.device)
        for sl in range(self.nsl):
            out |= tab[:, sl, :][:, (s >> (8 * sl)) & 255]
        if self._has_flip:
            out ^= self._flip_masks[:, None]
        return out

    def expand(self, v):
        """B v: the vector in the row order of ``SpinSectorOperator`` (torch indexing; for tests, n_sector <= 2^27)"""
        if self.n_sector > 1 << 27:
            raise ValueError("expand needs n_sector <= 2^27")
        if self._sector_tables is None:
            _, lo_rank, hi_base = _build_sector_tables(self.N, self.ndown, self.n_sector, self.device)
            self._sector_tables = (lo_rank.to(torch.int64), hi_base.to(torch.int64))
        lo_rank, hi_base = self._sector_tables
        coef = v / torch.sqrt(float(self.ng) * self._norms.to(v.dtype))
        images = self._images(self._states)
        w = torch.zeros(self.n_sector, dtype=v.dtype, device=v.device)
        for g in range(self.ng):
            rows = hi_base[images[g] >> self.Llo] + lo_rank[images[g] & ((1 << self.Llo) - 1)]
            w = w.index_add(0, rows, self._chars[g] * coef)
        return w

    def to_csr(self, layout="sell", col16="auto", values="auto"):
        """The symmetry-sector matrix as an explicit device CSR operand (entries that share a row and a column are summed).
        Built on the device with index arithmetic."""
        n = self.n
        jxy, jz, hz = self.unpack(self.symmetrise(self._c.detach()))
        s, sigma = self._states, self._norms.to(F64)
        rows = torch.arange(n, dtype=torch.int64, device=self.device)
        z = [(1 - 2 * ((s >> i) & 1)).to(F64) for i in range(self.N)]
        diag = torch.zeros(n, dtype=F64, device=self.device)
        for i in range(self.N):
            diag = diag + hz[i] * z[i]
        r_all, c_all, v_all = [rows], [rows], []
        for t, (a, b) in enumerate(self._bonds):
            diag = diag + jz[t] * (z[a] * z[b])
            flips = rows[((s >> a) ^ (s >> b)) & 1 == 1]
            images = self._images(s[flips] ^ ((1 << a) | (1 << b)))
            best, which = images.min(dim=0)
            col = self.row_of(best)
            keep = col >= 0
            flips, col, which = flips[keep], col[keep], which[keep]
            r_all.append(flips)
            c_all.append(col)
            v_all.append(2.0 * jxy[t] * self._chars[which] * torch.sqrt(sigma[col] / sigma[flips]))
        key = torch.cat(r_all) * n + torch.cat(c_all)
        uniq, inverse = torch.unique(key, sorted=True, return_inverse=True)
        vals = torch.zeros(uniq.numel(), dtype=F64, device=self.device).index_add(0, inverse, torch.cat([diag] + v_all))
        r_u = torch.div(uniq, n, rounding_mode="floor")
        rowptr = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
        rowptr[1:] = torch.cumsum(torch.bincount(r_u, minlength=n), 0)
        return CSROperator(rowptr, uniq - r_u * n, vals.contiguous(), n, layout=layout, col16=col16, values=values)


# ------------------------------------------------------------------------------------------ Hubbard model at fixed (N_up, N_dn)
def hubbard_dim(L, nup, ndn):
    """the dimension C(L, nup) C(L, ndn) of the Hubbard space of L sites with nup up and ndn down particles (pure Python)"""
    return sector_dim(L, nup) * sector_dim(L, ndn)


def _check_hubbard(L, nup, ndn):
    """(L, nup, ndn, n_up, n_dn) as ints; ValueError for what dsea_hubbard_sizes refuses -- host arithmetic only"""
    L, nup, ndn = int(L), int(nup), int(ndn)
    if not 2 <= L <= _lib.SECTOR_MAX_L:
        raise ValueError("HubbardOperator needs 2 <= L <= %d, got %d" % (_lib.SECTOR_MAX_L, L))
    for name, k in (("nup", nup), ("ndn", ndn)):
        if not 1 <= k <= L - 1:
            raise ValueError("HubbardOperator needs 1 <= %s <= L - 1 = %d, got %d" % (name, L - 1, k))
    n_up, n_dn = math.comb(L, nup), math.comb(L, ndn)
    if n_up * n_dn > 2 ** 31 - 1:
        raise ValueError("L = %d, nup = %d, ndn = %d has %d rows; rows are 32-bit: at most 2^31 - 1" % (L, nup, ndn, n_up * n_dn))
    return L, nup, ndn, n_up, n_dn


class HubbardOperator(_CouplingsOperator):
    """H = sum_t [-t_t sum_s (c+_{a s} c_{b s} + h.c.) + V_t n_a n_b] + sum_i U_i n_{i up} n_{i dn} + sum_i eps_i n_i on L sites
    with exactly ``nup`` up and ``ndn`` down fermions, matrix-free (docs/design/19-hubbard.md).  ``bonds`` follows the rules of
    ``SpinLatticeOperator``; 2 <= L <= 40, 1 <= nup, ndn <= L - 1 and n = C(L, nup) C(L, ndn) <= 2^31 - 1.  Bit i of the word u
    is the occupation of (i, up), bit i of d that of (i, dn); |u, d> = (prod_{i in u, ascending} c+_{i up})
    (prod_{j in d, ascending} c+_{j dn}) |0>.  Row r = ru * n_dn + rd (down fastest) with ru, rd the ranks of u, d among the words
    of their popcount in increasing integer order: ``up_states`` / ``dn_states`` (int64, on the device),
    ``sector_states(L, nup)`` / ``sector_states(L, ndn)`` on the host.

    ``couplings`` is ONE contiguous float64 device tensor of length 2 nb + 2 L in the order [t(nb), V(nb), U(L), eps(L)] -- the
    parameter (it may require grad; ``pack`` / ``unpack`` convert).  The kernels read it through its device pointer on every
    launch: in-place optimiser steps are seen, binding another tensor makes a new handle on the same tables.  ``H(v)`` is
    differentiable in v and in ``couplings``; ``Hadjoint_to_couplingsadjoint(v1, v2)`` is the hook for
    ``setDominantSparseSymeig`` / ``setLowestSparseSymeig``: all 2 nb + 2 L forms in one pass.  Both are re-entrant (H is linear
    in the couplings), so second order works.  The state and rank tables of each species are built once per operator by the
    library's sector-table kernels and kept alive by it; with nup == ndn one set serves both species."""

    _families = "t(nb), V(nb), U(L), eps(L)"
    _forms_stem = "dsea_op_hubbard"

    def __init__(self, L, bonds, couplings, nup, ndn, device=None):
        self.N, self.nup, self.ndn, self.n_up, self.n_dn = _check_hubbard(L, nup, ndn)
        self._bonds = _check_bonds(self.N, bonds)
        self.nb = len(self._bonds)
        self.nparam = 2 * self.nb + 2 * self.N
        self.dim = self.n = self.n_up * self.n_dn
        self.device = _cuda_device("HubbardOperator", device, couplings)
        self.Llo = (self.N + 1) // 2
        self._up = _build_sector_tables(self.N, self.nup, self.n_up, self.device)
        self._dn = self._up if self.ndn == self.nup else _build_sector_tables(self.N, self.ndn, self.n_dn, self.device)
        self._forms_sizes = (self.N, self.nup, self.ndn, self.nb)
        self._bind(couplings)

    def _create(self, data):
        tables = self._up + self._dn
        raw = c_void_p()
        check(_lib.load().dsea_op_create_hubbard(self.N, self.nup, self.ndn, self.nb, _flat_bonds(self._bonds),
                                                 c_void_p(data.data_ptr()), *[c_void_p(t.data_ptr()) for t in tables], byref(raw)),
              "dsea_op_create_hubbard")
        return raw, (data, tables)

    @property
    def bonds(self):
        """the bond list as a tuple of (a, b) pairs, in the order of the couplings (read-only)"""
        return self._bonds

    @property
    def up_states(self):
        """up_states[ru] = the up word of the rows ru * n_dn .. ru * n_dn + n_dn - 1 (int64 device tensor, increasing)"""
        return self._up[0]

    @property
    def dn_states(self):
        """dn_states[rd] = the down word of the rows rd, n_dn + rd, ... (int64 device tensor, increasing)"""
        return self._dn[0]

    def set_grid_log2(self, grid_log2):
        """log2 of the most blocks a launch uses (6..12, default 12; measurement aid, dsea_op_set_tuning)"""
        self._set_tune_log2(grid_log2)

    def pack(self, t, V, U, eps):
        """the four families (scalars, or one value per bond / per site) as one parameter tensor on the operator's device"""
        return _pack(self.device, (t, V, U, eps), (self.nb, self.nb, self.N, self.N))

    def unpack(self, p):
        """views (t, V, U, eps) of a parameter tensor"""
        nb, L = self.nb, self.N
        if tuple(p.shape) != (self.nparam,):
            raise ValueError("expected a tensor of shape (%d,)" % self.nparam)
        return p[:nb], p[nb:2 * nb], p[2 * nb:2 * nb + L], p[2 * nb + L:]

    def apply_block(self, X):
        """H X for a device tensor X of shape (n, R), any R >= 1: all columns in one pass over the rows per block of 8, 4, 2 or
        1 columns (dsea_op_hubbard_block_apply, docs/design/28-hubbard-finite-temperature.md); column j equals ``H(X[:, j])`` bit
        for bit.  Plain, not differentiable: X is detached."""
        return _apply_block(self, X, "dsea_op_hubbard_block_apply")

    def rank(self, u, d):
        """the row of every pair of words in the int64 device tensors ``u`` (nup set bits) and ``d`` (ndn set bits)"""
        return _table_rank(self._up, self.Llo, u) * self.n_dn + _table_rank(self._dn, self.Llo, d)

    def ladder(self, dst, species=None):
        """the site-weighted c+ / c / n maps of one species from this sector into the sector of ``dst`` (``HubbardLadder``)"""
        return HubbardLadder(self, dst, species)

    def current(self):
        """the bond current map K(w) of this sector, on this operator's tables, bonds and grid tuning (``HubbardCurrent``)"""
        return HubbardCurrent(self)

    def to_csr(self, layout="sell", col16="auto", values="auto"):
        """The matrix as an explicit device CSR operand: the diagonal, and one entry per (row, species, distinct bond mask that
        moves a particle of that species in the row); bonds with equal masks are summed.  Built on the device with index
        arithmetic."""
        n, n_dn, L = self.n, self.n_dn, self.N
        t, V, U, eps = self.unpack(self._c.detach())
        rows = torch.arange(n, dtype=torch.int64, device=self.device)
        ru, rd = rows // n_dn, rows % n_dn
        u, d = self.up_states[ru], self.dn_states[rd]
        occ = [((u >> i) & 1) + ((d >> i) & 1) for i in range(L)]
        diag = torch.zeros(n, dtype=F64, device=self.device)
        for i in range(L):
            diag = diag + U[i] * ((u >> i) & (d >> i) & 1).to(F64) + eps[i] * occ[i].to(F64)
        by_mask = {}
        for k, (a, b) in enumerate(self._bonds):
            diag = diag + V[k] * (occ[a] * occ[b]).to(F64)
            m = (1 << a) | (1 << b)
            by_mask[m] = by_mask[m] - t[k] if m in by_mask else -t[k]
        r_all, c_all, v_all = [rows], [rows], [diag]
        for m, amp in by_mask.items():
            lo, hi = [i for i in range(L) if (m >> i) & 1]
            between = ((1 << hi) - 1) & ~((1 << (lo + 1)) - 1)
            for up in (True, False):
                w = u if up else d
                moved = rows[((w >> lo) ^ (w >> hi)) & 1 == 1]
                wm = w[moved]
                partner = _table_rank(self._up if up else self._dn, self.Llo, wm ^ m)
                # sgn = (-1)^popcount(w & between): the parity by folding the word onto its lowest bit
                par = wm & between
                for shift in (32, 16, 8, 4, 2, 1):
                    par = par ^ (par >> shift)
                r_all.append(moved)
                c_all.append(partner * n_dn + rd[moved] if up else ru[moved] * n_dn + partner)
                v_all.append(amp * (1 - 2 * (par & 1)).to(F64))
        return _csr_from_coo(r_all, c_all, v_all, n, layout, col16, values)


# ------------------------------------------------------------------------------------------ bond current of a Hubbard sector
class HubbardCurrent:
    """The bond-weighted current map of the sector of a ``HubbardOperator``, matrix-free (docs/design/39-hubbard-current.md):

        K(w) = sum_t sum_s w[s, t] (c+_{a s} c_{b s} - c+_{b s} c_{a s}),      (a, b) = op.bonds[t] in the caller's orientation

    real and antisymmetric in the state order of the operator; the current operator is J = i K(w).  Reversing a bond flips the
    sign of its term, a repeated bond counts each time.  ``w`` is a real tensor of shape (2, nb), species 0 = up and 1 = dn; a
    (nb,) vector is used for both species (the charge current; ``torch.stack([w, -w])`` is the spin current).  The object works
    on the operator's sector, tables, bond list and grid tuning (``op.set_grid_log2``) and allocates no tables of its own; the
    operator's couplings are not read.

    ``cur(w, x)`` is K(w) x, differentiable to any order in w and in x: the map is bilinear and each of the two
    ``autograd.Function``s is the other's derivative.  ``cur.forms(v1, v2)[s, t] = v1^T K_{s t} v2``, the bond-current matrix
    elements of all 2 nb unit-weight maps in one pass (deterministic: fixed-order sums, no atomics).  There is no second object
    for the transpose: K(w)^T = -K(w) = K(-w), so ``cur.T`` would be ``-cur`` and ``x . K(w) y = -y . K(w) x``.
    ``apply_block(w, X)`` is the map on a block of columns (detached); ``dense(w)`` the n x n matrix, a test aid for small
    sectors.  Every argument check is host arithmetic before the device is touched and raises ``ValueError``."""

    _operand = ("N", "nup", "ndn", "nb", "n", "device", "bonds", "handle")

    def __init__(self, op):
        for attr in self._operand:
            if not hasattr(op, attr):
                raise ValueError("op carries no Hubbard sector (no attribute %r): a HubbardOperator is needed" % attr)
        _check_hubbard(op.N, op.nup, op.ndn)
        self.op = op
        self.L = self.N = int(op.N)
        self.nb = int(op.nb)
        self.n = int(op.n)
        self.device = torch.device(op.device)

    @property
    def bonds(self):
        """the operator's bond list: the orientation (a, b) of bond t is the sign convention of w[:, t]"""
        return self.op.bonds

    def _weights(self, w):
        """the weights as a real float64 (2, nb) tensor on the device; the graph of a tensor input is kept"""
        if not torch.is_tensor(w):
            w = torch.as_tensor(w, dtype=F64)
        if w.is_complex():
            raise ValueError("the bond weights must be real: apply the real and the imaginary part one after the other")
        if tuple(w.shape) not in ((self.nb,), (2, self.nb)):
            raise ValueError("expected bond weights of shape (2, %d) or (%d,), got %r" % (self.nb, self.nb, tuple(w.shape)))
        if w.dtype != F64 or w.device != self.device:
            w = w.to(device=self.device, dtype=F64)
        return torch.stack([w, w]) if w.dim() == 1 else w

    def _vector(self, v, what):
        if not torch.is_tensor(v) or v.dim() != 1 or v.numel() != self.n:
            raise ValueError("%s must be a vector of %d elements, got %s"
                             % (what, self.n, tuple(v.shape) if torch.is_tensor(v) else type(v)))
        if v.device != self.device:
            raise ValueError("%s must live on %s, got %s" % (what, self.device, v.device))
        if v.is_complex():
            raise ValueError("%s must be real: apply the map to the real and the imaginary part one after the other" % what)
        return v

    def _block(self, X, what):
        if not torch.is_tensor(X) or X.dim() != 2 or X.shape[0] != self.n or X.shape[1] < 1:
            raise ValueError("%s must be a tensor of shape (%d, R) with R >= 1, got %r"
                             % (what, self.n, tuple(X.shape) if torch.is_tensor(X) else type(X).__name__))
        if X.device != self.device:
            raise ValueError("%s must live on %s, got %s" % (what, self.device, X.device))
        if X.is_complex():
            raise ValueError("%s must be real: the real and the imaginary part are columns of one real block" % what)
        return X.detach().to(F64)

    def _launch_apply(self, w, R, X, Y):
        with torch.cuda.device(self.device):
            check(_lib.load().dsea_op_hubbard_current_apply(self.op.handle, R, c_void_p(w.data_ptr()), c_void_p(X.data_ptr()),
                                                            c_void_p(Y.data_ptr()), engine._stream(self.device)),
                  "dsea_op_hubbard_current_apply")

    def _apply_raw(self, w, x):
        w, x = engine.as_vector(w.reshape(-1), 2 * self.nb), engine.as_vector(x, self.n)
        y = torch.empty(self.n, dtype=F64, device=self.device)
        self._launch_apply(w, 1, x, y)
        return y

    def _forms_raw(self, v1, v2):
        lib = _lib.load()
        v1, v2 = engine.as_vector(v1, self.n), engine.as_vector(v2, self.n)
        need = c_int64()
        check(lib.dsea_op_hubbard_current_forms_scratch_doubles(self.N, int(self.op.nup), int(self.op.ndn), self.nb, byref(need)),
              "dsea_op_hubbard_current_forms_scratch_doubles")
        scratch = torch.empty(need.value, dtype=F64, device=self.device)
        out = torch.empty((2, self.nb), dtype=F64, device=self.device)
        with torch.cuda.device(self.device):
            check(lib.dsea_op_hubbard_current_forms(self.op.handle, c_void_p(v1.data_ptr()), c_void_p(v2.data_ptr()),
                                                    c_void_p(out.data_ptr()), c_void_p(scratch.data_ptr()),
                                                    engine._stream(self.device)), "dsea_op_hubbard_current_forms")
        return out

    def __call__(self, w, x):
        """the vector K(w) x, differentiable in w and in x"""
        return _CurrentApply.apply(self._weights(w), self._vector(x, "x"), self)

    def forms(self, v1, v2):
        """out[s, t] = v1^T K_{s t} v2 for every species and bond, shape (2, nb); differentiable.  ``forms(v, v)`` is 0."""
        return _CurrentForms.apply(self._vector(v1, "v1"), self._vector(v2, "v2"), self)

    def apply_block(self, w, X):
        """K(w) X for a device tensor X of shape (n, R), any R >= 1, in blocks of 8, 4, 2 and 1 columns
        (dsea_op_hubbard_current_apply).  Column j equals ``cur(w, X[:, j])`` bit for bit; a row's division, state words and
        table reads are made once for all columns of a block.  Detached, not differentiable."""
        from .chebyshev import _aligned_piece
        from .thermal import block_pieces
        w = engine.as_vector(self._weights(w).detach().reshape(-1), 2 * self.nb)
        X = self._block(X, "X")
        out = []
        for first, width in block_pieces(X.shape[1]):
            Yp = torch.empty((self.n, width), dtype=F64, device=self.device)
            self._launch_apply(w, width, _aligned_piece(X, first, width), Yp)
            out.append(Yp)
        return out[0] if len(out) == 1 else torch.cat(out, dim=1)

    def block_dots(self, w, Lft, X):
        """d[j] = sum_r Lft[r, j] (K(w) X)[r, j] as a device tensor [R], for Lft and X of shape (n, R), any R >= 1: the column
        dots of ``Lft`` with ``apply_block(w, X)`` without the product block (dsea_op_hubbard_current_block_dots,
        docs/design/40-finite-temperature-conductivity.md; in blocks of 8, 4, 2 and 1 columns; fixed-order sums, identical calls
        return identical bits).  ``Lft`` may be ``X``: the dots are then 0 up to rounding.  Detached, not differentiable."""
        from .chebyshev import _aligned_piece
        from .thermal import block_pieces
        w = self._weights(w)
        X = self._block(X, "X")
        Lft = self._block(Lft, "Lft")
        if Lft.shape[1] != X.shape[1]:
            raise ValueError("Lft and X must have the same number of columns, got %d and %d" % (Lft.shape[1], X.shape[1]))
        w = engine.as_vector(w.detach().reshape(-1), 2 * self.nb)
        lib = _lib.load()
        out = torch.empty(X.shape[1], dtype=F64, device=self.device)
        for first, width in block_pieces(X.shape[1]):
            need = c_int64()
            check(lib.dsea_op_hubbard_current_block_dots_scratch_doubles(self.N, int(self.op.nup), int(self.op.ndn), width,
                                                                         byref(need)),
                  "dsea_op_hubbard_current_block_dots_scratch_doubles")
            scratch = torch.empty(need.value, dtype=F64, device=self.device)
            piece = torch.empty(width, dtype=F64, device=self.device)
            Lp, Xp = _aligned_piece(Lft, first, width), _aligned_piece(X, first, width)
            with torch.cuda.device(self.device):
                check(lib.dsea_op_hubbard_current_block_dots(self.op.handle, width, c_void_p(w.data_ptr()), c_void_p(Lp.data_ptr()),
                                                             c_void_p(Xp.data_ptr()), c_void_p(piece.data_ptr()),
                                                             c_void_p(scratch.data_ptr()), engine._stream(self.device)),
                      "dsea_op_hubbard_current_block_dots")
            out[first:first + width] = piece
        return out

    def dense(self, w):
        """the n x n matrix of ``cur(w, .)``, by applying the map to the columns of the identity (small sectors)"""
        return self.apply_block(w, torch.eye(self.n, dtype=F64, device=self.device))


class _CurrentApply(torch.autograd.Function):
    """y = K(w) x.  Bilinear and antisymmetric: with the cotangent gy, w-bar = forms(gy, x) and x-bar = K(w)^T gy = -K(w) gy --
    both re-entrant."""

    @staticmethod
    def forward(ctx, w, x, cur):
        ctx.cur = cur
        ctx.save_for_backward(w, x)
        return cur._apply_raw(w.detach(), x.detach())

    @staticmethod
    def backward(ctx, gy):
        w, x = ctx.saved_tensors
        gw = _CurrentForms.apply(gy, x, ctx.cur) if ctx.needs_input_grad[0] else None
        gx = -_CurrentApply.apply(w, gy, ctx.cur) if ctx.needs_input_grad[1] else None
        return gw, gx, None


class _CurrentForms(torch.autograd.Function):
    """out[s, t] = v1^T K_{s t} v2, shape (2, nb).  K is linear in the weights, so with the cotangent G as weights
    v1-bar = K(G) v2 and v2-bar = K(G)^T v1 = -K(G) v1."""

    @staticmethod
    def forward(ctx, v1, v2, cur):
        ctx.cur = cur
        ctx.save_for_backward(v1, v2)
        return cur._forms_raw(v1.detach(), v2.detach())

    @staticmethod
    def backward(ctx, G):
        v1, v2 = ctx.saved_tensors
        G = G.reshape(2, ctx.cur.nb)
        g1 = _CurrentApply.apply(G, v2, ctx.cur) if ctx.needs_input_grad[0] else None
        g2 = -_CurrentApply.apply(G, v1, ctx.cur) if ctx.needs_input_grad[1] else None
        return g1, g2, None


# ------------------------------------------------------------------------------------------ c / c+ between two Hubbard sectors
_HUBBARD_SPECIES = {"up": 0, "dn": 1}


class HubbardLadder(_SectorLadderBase):
    """The site-weighted creation, annihilation and density operators of one species between two particle-number sectors of
    the Hubbard space of the same L sites, matrix-free (docs/design/25-hubbard-ladder.md).  ``src`` and ``dst`` are
    ``HubbardOperator`` objects (anything that carries the species tables: ``N``, ``nup``, ``ndn``, ``device``, ``_up``, ``_dn``)
    with the same L on the same device.  (dst.nup - src.nup, dst.ndn - src.ndn) fixes the species and the step: (+-1, 0) is the
    up species, (0, +-1) the down species; (0, 0) needs ``species="up"`` or ``"dn"``.  With the ordering convention of
    ``HubbardOperator`` and site weights w (float64 [L]):

        step = +1:  lad(w, x) = sum_i w_i c+_{i s} x      step = -1:  sum_i w_i c_{i s} x      step = 0:  sum_i w_i n_{i s} x

    as a vector of the destination sector (``n_dst`` rows) from one of the source sector (``n_src`` rows), fermion signs
    included (a down operator passes all nup up operators).  The object builds no tables: it reads the two operators' tables and
    keeps them alive.  ``lad.T`` is the ladder dst -> src on the same tables and ``lad.T(w, .)`` the exact transpose of
    ``lad(w, .)``.  ``lad.forms(v1, v2)[i] = v1^T (d lad / d w_i) v2`` for all sites in one pass (v1 on the destination, v2 on
    the source; deterministic).  Both are differentiable to any order in w and in the vectors: the map is bilinear and each of
    the two ``autograd.Function``s is the other's derivative.  ``dense(w)`` is the n_dst x n_src matrix, a test aid for small
    sectors.  ``apply_block`` and ``block_dots`` are the map and its column dots on blocks of columns
    (dsea_hubbard_ladder_block_apply and dsea_hubbard_ladder_block_dots,
    docs/design/37-hubbard-finite-temperature-dynamics.md): a row's division, state word and table reads are made once for all
    columns of a block.  Every argument check is host arithmetic before the device is touched and raises ``ValueError``."""

    _entry = "dsea_hubbard_ladder"
    _operand = ("N", "nup", "ndn", "device", "_up", "_dn")
    _no_operand = "%s carries no species tables (no attribute %r): a HubbardOperator is needed"

    def __init__(self, src, dst, species=None, _transpose=None):
        self._pair(src, dst, _transpose)
        if species is not None and species not in _HUBBARD_SPECIES:
            raise ValueError("species must be 'up', 'dn' or None, got %r" % (species,))
        dup, ddn = int(dst.nup) - int(src.nup), int(dst.ndn) - int(src.ndn)
        if (dup, ddn) == (0, 0):
            if species is None:
                raise ValueError("src and dst are the same sector: species='up' or 'dn' picks sum_i w_i n_{i s}")
            step = 0
        elif ddn == 0 and dup in (-1, 1):
            implied, step = "up", dup
        elif dup == 0 and ddn in (-1, 1):
            implied, step = "dn", ddn
        else:
            raise ValueError("a ladder changes the count of one species by +1, 0 or -1, got (nup, ndn) = (%d, %d) -> (%d, %d)"
                             % (src.nup, src.ndn, dst.nup, dst.ndn))
        if step != 0:
            if species is not None and species != implied:
                raise ValueError("species=%r contradicts the sectors (%d, %d) -> (%d, %d), which move the %s species"
                                 % (species, src.nup, src.ndn, dst.nup, dst.ndn, implied))
            species = implied
        self.species, self.step = species, step
        self._species = _HUBBARD_SPECIES[species]
        self.n_src = math.comb(self.L, int(src.nup)) * math.comb(self.L, int(src.ndn))
        self.n_dst = math.comb(self.L, int(dst.nup)) * math.comb(self.L, int(dst.ndn))
        moving_src, moving_dst = (src._up, dst._up) if species == "up" else (src._dn, dst._dn)
        self._tables = (moving_dst[0], moving_src[1], moving_src[2])    # states of dst, rank tables of src: kept alive

    def _check_operand(self, name, op):
        _check_hubbard(op.N, op.nup, op.ndn)
        if len(op._up) != 3 or len(op._dn) != 3:
            raise ValueError("%s._up and %s._dn must be (states, lo_rank, hi_base)" % (name, name))

    def _transpose_args(self):
        return (self.species,)

    def _sector_args(self):
        return self.L, int(self.src.nup), int(self.src.ndn), self._species, self.step


def one_body_density_matrix(op, psi, species, target=None):
    """rho[i, j] = <psi| c+_{i s} c_{j s} |psi> for the species ``"up"`` or ``"dn"`` of the Hubbard sector of ``op``, shape
    (L, L): rho_ij = (c_{i s} psi) . (c_{j s} psi) from L applications of the annihilation ladder with one-hot weights and one
    Gram matrix.  Differentiable in psi (hence through ``DominantSparseSymeig``).  ``target`` carries the tables of the sector
    with one particle of that species less; ``None`` builds them (zero couplings on the bonds of ``op``)."""
    if species not in _HUBBARD_SPECIES:
        raise ValueError("species must be 'up' or 'dn', got %r" % (species,))
    if target is None:
        nup, ndn = (op.nup - 1, op.ndn) if species == "up" else (op.nup, op.ndn - 1)
        _check_hubbard(op.N, nup, ndn)
        target = HubbardOperator(op.N, op.bonds, torch.zeros(op.nparam, dtype=F64, device=op.device), nup, ndn, op.device)
    lad = HubbardLadder(op, target, species)
    if lad.step != -1:
        raise ValueError("one_body_density_matrix needs a target with one %s particle less than op" % species)
    eye = torch.eye(lad.L, dtype=F64, device=lad.device)
    C = torch.stack([lad(eye[i], psi) for i in range(lad.L)])
    return C @ C.T


# ------------------------------------------------------------------------------------------ pair and spin-flip maps between two Hubbard sectors
_PAIR_ORDERS = {"up_left": 0, "dn_left": 1}


class _NotOffered:
    """a method of the base class that a subclass does not have (its C entries do not exist): reading it is an AttributeError"""

    def __set_name__(self, owner, name):
        self._what = "%s has no %s" % (owner.__name__, name)

    def __get__(self, obj, owner=None):
        raise AttributeError(self._what)


class HubbardPairLadder(_SectorLadderBase):
    """The maps that move one particle of EACH species between two particle-number sectors of the Hubbard space of the same L
    sites in one pass, matrix-free (docs/design/41-hubbard-pair-ladder.md).  ``src`` and ``dst`` are ``HubbardOperator`` objects
    (anything that carries the species tables, as for ``HubbardLadder``) with the same L on the same device and
    (dst.nup - src.nup, dst.ndn - src.ndn) one of (+-1, +-1).  With A = c+ where the up count grows and c where it shrinks, B
    likewise for the down species, and a real weight matrix W (L, L) -- an (L,) vector means its diagonal --

        order="up_left":  lad(W, x) = sum_ij W_ij A_{i up} B_{j dn} x        order="dn_left":  sum_ij W_ij B_{j dn} A_{i up} x

    (the second is the negative of the first) as a vector of the destination sector, fermion signs of the ordering convention of
    ``HubbardOperator`` included.  (+1, +1) is the pair creation field, (-1, -1) pair annihilation, (+1, -1) and (-1, +1) the
    spin flips c+_{i up} c_{j dn} and c_{i up} c+_{j dn}.  ``lad.T`` is the map dst -> src with the other order on the same tables
    and ``lad.T(W, .)`` the exact transpose of ``lad(W, .)``: the transpose of sum W_ij c+_{i up} c+_{j dn} is sum W_ij c_{j dn}
    c_{i up}.  ``lad.forms(v1, v2)[i, j] = v1^T (d lad / d W_ij) v2`` for all L^2 site pairs in one pass (v1 on the destination, v2
    on the source; deterministic).  Both are differentiable to any order in W and in the vectors: the map is bilinear and each of
    the two ``autograd.Function``s is the other's derivative.  ``dense(W)`` is the n_dst x n_src matrix, a test aid for small
    sectors.  There are no block forms.  Every argument check is host arithmetic before the device is touched and raises
    ``ValueError``."""

    _entry = "dsea_hubbard_pair"
    _operand = HubbardLadder._operand
    _no_operand = HubbardLadder._no_operand
    apply_block = _NotOffered()
    block_dots = _NotOffered()

    def __init__(self, src, dst, order="up_left", _transpose=None):
        self._pair(src, dst, _transpose)
        if order not in _PAIR_ORDERS:
            raise ValueError("order must be 'up_left' or 'dn_left', got %r" % (order,))
        dup, ddn = int(dst.nup) - int(src.nup), int(dst.ndn) - int(src.ndn)
        if dup not in (-1, 1) or ddn not in (-1, 1):
            raise ValueError("a pair map changes the count of each species by +1 or -1, got (nup, ndn) = (%d, %d) -> (%d, %d)"
                             % (src.nup, src.ndn, dst.nup, dst.ndn))
        self.order, self.steps = order, (dup, ddn)
        self.n_src = math.comb(self.L, int(src.nup)) * math.comb(self.L, int(src.ndn))
        self.n_dst = math.comb(self.L, int(dst.nup)) * math.comb(self.L, int(dst.ndn))
        # per species: states of dst, rank tables of src -- kept alive
        self._tables = (dst._up[0], src._up[1], src._up[2], dst._dn[0], src._dn[1], src._dn[2])

    _check_operand = HubbardLadder._check_operand

    def _transpose_args(self):
        return ("dn_left" if self.order == "up_left" else "up_left",)

    def _sector_args(self):
        return self.L, int(self.src.nup), int(self.src.ndn), self.steps[0], self.steps[1], _PAIR_ORDERS[self.order]

    def _weights(self, W):
        if not torch.is_tensor(W):
            W = torch.as_tensor(W, dtype=F64)
        if W.is_complex():
            raise ValueError("the pair weights must be real: apply the real and the imaginary part one after the other")
        if W.dim() == 1 and W.numel() == self.L:
            W = torch.diag(W)
        if tuple(W.shape) != (self.L, self.L):
            raise ValueError("expected pair weights of shape (%d, %d) or (%d,), got %r" % (self.L, self.L, self.L, tuple(W.shape)))
        if W.dtype != F64 or W.device != self.device:
            W = W.to(device=self.device, dtype=F64)
        return W

    def _apply_raw(self, W, x):
        W, x = engine.as_vector(W.reshape(-1), self.L * self.L), engine.as_vector(x, self.n_src)
        y = torch.empty(self.n_dst, dtype=F64, device=x.device)
        self._launch("apply", (W,), (x, y))
        return y

    def _forms_raw(self, v1, v2):
        v1, v2 = engine.as_vector(v1, self.n_dst), engine.as_vector(v2, self.n_src)
        out = torch.empty((self.L, self.L), dtype=F64, device=v1.device)
        self._launch("forms", (), (v1, v2, out, self._scratch("forms")))
        return out

    def __call__(self, W, x):
        """the vector sum_ij W_ij O_ij x of the destination sector, differentiable in W and in x"""
        return _PairApply.apply(self._weights(W), self._vector(x, self.n_src, "x"), self)

    def forms(self, v1, v2):
        """out[i, j] = v1^T O_ij v2 for every site pair, shape (L, L): v1 on the destination, v2 on the source; differentiable"""
        return _PairForms.apply(self._vector(v1, self.n_dst, "v1"), self._vector(v2, self.n_src, "v2"), self)


class _PairApply(torch.autograd.Function):
    """y = P(W) x.  Bilinear: with the cotangent gy, W-bar = forms(gy, x) and x-bar = P(W)^T gy, the transposed map on the same
    tables -- both re-entrant."""

    @staticmethod
    def forward(ctx, W, x, lad):
        ctx.lad = lad
        ctx.save_for_backward(W, x)
        return lad._apply_raw(W.detach(), x.detach())

    @staticmethod
    def backward(ctx, gy):
        W, x = ctx.saved_tensors
        gW = _PairForms.apply(gy, x, ctx.lad) if ctx.needs_input_grad[0] else None
        gx = _PairApply.apply(W, gy, ctx.lad.T) if ctx.needs_input_grad[1] else None
        return gW, gx, None


class _PairForms(torch.autograd.Function):
    """out[i, j] = v1^T (dP/dW_ij) v2, shape (L, L).  P is linear in the weights, so with the cotangent G as weights
    v1-bar = P(G) v2 and v2-bar = P(G)^T v1."""

    @staticmethod
    def forward(ctx, v1, v2, lad):
        ctx.lad = lad
        ctx.save_for_backward(v1, v2)
        return lad._forms_raw(v1.detach(), v2.detach())

    @staticmethod
    def backward(ctx, G):
        v1, v2 = ctx.saved_tensors
        g1 = _PairApply.apply(G, v2, ctx.lad) if ctx.needs_input_grad[0] else None
        g2 = _PairApply.apply(G, v1, ctx.lad.T) if ctx.needs_input_grad[1] else None
        return g1, g2, None


def onsite_pairing(L, signs=None):
    """the (L, L) weights of the on-site pair field sum_i s_i c+_{i up} c+_{i dn}: diag(signs), the identity for ``signs=None``
    (s-wave); signs = (-1)^i on a bipartite lattice is the eta pair.  A float64 host tensor (pure torch, no device)."""
    L = int(L)
    if L < 1:
        raise ValueError("onsite_pairing needs L >= 1")
    if signs is None:
        return torch.eye(L, dtype=F64)
    s = torch.as_tensor(signs, dtype=F64)
    if tuple(s.shape) != (L,):
        raise ValueError("expected %d signs, got shape %r" % (L, tuple(s.shape)))
    return torch.diag(s)


def bond_pairing(L, bonds, amplitudes):
    """the (L, L) weights of the singlet pair field sum_t amp_t (c+_{a up} c+_{b dn} + c+_{b up} c+_{a dn}) / sqrt(2) over the
    bonds t = (a, b): W_ab = W_ba = amp_t / sqrt(2), summed over bonds that name the same pair.  Equal amplitudes give the
    extended-s field, +1 on the x bonds and -1 on the y bonds of a square lattice the d-wave field.  Differentiable in
    ``amplitudes``; on their device (pure torch)."""
    L = int(L)
    bonds = [(int(a), int(b)) for a, b in bonds]
    for a, b in bonds:
        if not (0 <= a < L and 0 <= b < L) or a == b:
            raise ValueError("a bond joins two different sites of 0 .. %d, got (%d, %d)" % (L - 1, a, b))
    amp = torch.as_tensor(amplitudes)
    if amp.is_complex() or tuple(amp.shape) != (len(bonds),):
        raise ValueError("expected %d real amplitudes (one per bond), got shape %r" % (len(bonds), tuple(amp.shape)))
    amp = amp.to(F64) / math.sqrt(2.0)
    a = torch.tensor([a for a, _ in bonds] + [b for _, b in bonds], dtype=torch.int64, device=amp.device)
    b = torch.tensor([b for _, b in bonds] + [a for a, _ in bonds], dtype=torch.int64, device=amp.device)
    return torch.zeros((L, L), dtype=F64, device=amp.device).index_put((a, b), torch.cat([amp, amp]), accumulate=True)


def _hubbard_target(op, nup, ndn):
    """the sector (nup, ndn) on the bonds of ``op`` with zero couplings: a carrier of tables"""
    _check_hubbard(op.N, nup, ndn)
    return HubbardOperator(op.N, op.bonds, torch.zeros(op.nparam, dtype=F64, device=op.device), nup, ndn, op.device)


def pair_correlations(op, psi, pairings, target=None):
    """P[a, b] = <psi| Delta+(W_a) Delta(W_b) |psi> for the pair fields Delta(W) = sum_ij W_ij c_{j dn} c_{i up}, the transpose of
    Delta+(W) = sum_ij W_ij c+_{i up} c+_{j dn}, of the real (M, L, L) tensor ``pairings`` (``onsite_pairing``, ``bond_pairing``):
    the Gram matrix of the M vectors Delta(W_b) psi, shape (M, M), from M applications of one ``HubbardPairLadder``.
    Differentiable in psi (hence through ``DominantSparseSymeig``) and in the pairings.  ``target`` carries the tables of the
    sector (nup - 1, ndn - 1); ``None`` builds them."""
    if not torch.is_tensor(pairings):
        pairings = torch.as_tensor(pairings, dtype=F64)
    if pairings.dim() != 3 or tuple(pairings.shape[1:]) != (int(op.N), int(op.N)) or pairings.shape[0] < 1:
        raise ValueError("pairings must have shape (M, %d, %d) with M >= 1, got %r" % (op.N, op.N, tuple(pairings.shape)))
    if target is None:
        target = _hubbard_target(op, op.nup - 1, op.ndn - 1)
    lad = HubbardPairLadder(op, target, "dn_left")
    if lad.steps != (-1, -1):
        raise ValueError("pair_correlations needs a target with one particle of each species less than op")
    C = torch.stack([lad(pairings[a], psi) for a in range(pairings.shape[0])])
    return C @ C.T


def total_spin(op, psi, target=None):
    """<psi| S^2 |psi> of a vector of the Hubbard sector of ``op``, a 0-dim tensor differentiable in psi: with S^z = (nup - ndn)
    / 2 and S^+ = sum_i c+_{i up} c_{i dn}, S^2 = S^- S^+ + S^z (S^z + 1) = |S^+ psi|^2 + S^z (S^z + 1).  S^+ psi lives in
    (nup + 1, ndn - 1); when that sector is outside the library's limits (ndn = 1 or nup = L - 1) the other side serves: S^2 =
    |S^- psi|^2 + S^z (S^z - 1) in (nup - 1, ndn + 1).  ``target`` carries the tables of either sector; ``None`` builds them.
    ``ValueError`` when neither sector exists (nup = ndn = 1 at L = 2)."""
    L, nup, ndn = int(op.N), int(op.nup), int(op.ndn)
    sz = 0.5 * (nup - ndn)
    plus_ok = ndn - 1 >= 1 and nup + 1 <= L - 1
    minus_ok = nup - 1 >= 1 and ndn + 1 <= L - 1
    if target is None:
        if not plus_ok and not minus_ok:
            raise ValueError("total_spin: neither (nup + 1, ndn - 1) nor (nup - 1, ndn + 1) is a sector of 1 .. L - 1 particles per "
                             "species for L = %d, (nup, ndn) = (%d, %d)" % (L, nup, ndn))
        target = _hubbard_target(op, nup + 1, ndn - 1) if plus_ok else _hubbard_target(op, nup - 1, ndn + 1)
    raising = (int(target.nup), int(target.ndn)) == (nup + 1, ndn - 1)
    if not raising and (int(target.nup), int(target.ndn)) != (nup - 1, ndn + 1):
        raise ValueError("total_spin needs a target at (nup + 1, ndn - 1) or (nup - 1, ndn + 1), got (%d, %d)"
                         % (target.nup, target.ndn))
    lad = HubbardPairLadder(op, target, "up_left" if raising else "dn_left")
    phi = lad(torch.ones(L, dtype=F64, device=lad.device), psi)
    return phi.dot(phi) + (sz * (sz + 1.0) if raising else sz * (sz - 1.0))


# ------------------------------------------------------------------------------------------ stencil
class Stencil3Operator:
    """H v = coef (-2 v + v_{+1} + v_{-1}) + V o v, Dirichlet ends (reference examples/schrodinger1D.py:18-27
    with coef = -0.5/h^2).  ``potential`` is the parameter tensor (n,), the hook is v1 o v2 (:29-34)."""

    _native_methods = ("H", "__call__", "Hsparse")

    def __init__(self, n, h, potential):
        self.n = int(n)
        self.h = float(h)
        self.coef = -0.5 / self.h ** 2
        self.device = potential.device
        self._H = None
        self.potential = potential

    @property
    def potential(self):
        return self._V

    @potential.setter
    def potential(self, value):
        if value.device.type != "cuda" or value.dtype != F64 or value.numel() != self.n:
            raise ValueError("potential must be a float64 CUDA tensor of %d elements" % self.n)
        self._V = value
        self._Vdata = engine.as_vector(value.detach(), self.n)     # contiguous, 16-byte aligned (pair loads)
        raw = c_void_p()
        check(_lib.load().dsea_op_create_stencil3(self.n, self.coef, c_void_p(self._Vdata.data_ptr()), None, None,
                                                  byref(raw)), "dsea_op_create_stencil3")
        self._H = _NativeView(_Handle(raw, self.n, self._Vdata))

    @property
    def handle(self):
        return self._H.handle

    def H(self, v):
        return _Stencil3Apply.apply(v, self._V, self)

    __call__ = H
    Hsparse = H

    @staticmethod
    def Hadjoint_to_padjoint(v1, v2):
        return v1 * v2


class _Stencil3Apply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, V, op):
        ctx.op = op
        ctx.save_for_backward(v, V)
        return engine.spmv(op._H, v.detach())

    @staticmethod
    def backward(ctx, gy):
        v, V = ctx.saved_tensors
        gv = _Stencil3Apply.apply(gy, V, ctx.op) if ctx.needs_input_grad[0] else None
        gV = gy * v if ctx.needs_input_grad[1] else None
        return gv, gV, None


# ------------------------------------------------------------------------------------------ CSR
def sell_layout(rowptr, colidx, n, col16="auto", pad_cols=1):
    """SELL-64 structure of a CSR pattern (device tensors, torch index ops -- built once per operator):
    returns (slice_ptr int64 [nslices+1], columns, total) with ``columns`` = (int32 [total],) or, when every
    64-element slice column spans fewer than 65536 columns (``col16`` "auto" / True), (colbase int32 [total/64],
    coldelta uint16-as-int16 [total]) -- include/dsea.h dsea_op_create_sell / dsea_op_create_sell16.  Entry k of
    row i sits at slice_ptr[i // 64] + 64 k + i % 64; padding entries carry the smallest real column of their
    slice column (value 0), so gathers stay in range and the 16-bit deltas are not widened by them."""
    dev = rowptr.device
    nsl = (n + 63) // 64
    lens = rowptr[1:] - rowptr[:-1]
    padded = torch.zeros(nsl * 64, dtype=torch.int64, device=dev)
    padded[:n] = lens
    width = padded.view(nsl, 64).max(dim=1).values
    if pad_cols > 1:      # (the value-coded layout packs four slice columns to a lane: widths in multiples of pad_cols)
        width = (width + (pad_cols - 1)) // pad_cols * pad_cols
    slice_ptr = torch.zeros(nsl + 1, dtype=torch.int64, device=dev)
    slice_ptr[1:] = torch.cumsum(width * 64, 0)
    total = int(slice_ptr[-1].item())
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), lens)
    k_in_row = torch.arange(rows.numel(), dtype=torch.int64, device=dev) - rowptr[rows]
    dest = slice_ptr[rows // 64] + k_in_row * 64 + (rows % 64)
    big = torch.iinfo(torch.int32).max
    s_cols = torch.full((max(total, 64),), big, dtype=torch.int32, device=dev)[:total]
    s_cols[dest] = colidx.to(torch.int32)
    blocks = s_cols.view(-1, 64)
    cmin = blocks.min(dim=1, keepdim=True).values
    cmin = torch.where(cmin == big, torch.zeros_like(cmin), cmin)     # (a slice column that is ALL padding: column 0)
    blocks.copy_(torch.where(blocks == big, cmin.expand_as(blocks), blocks))
    span_ok = total > 0 and int((blocks.max(dim=1).values - cmin[:, 0]).max().item()) < 65536
    if col16 is True and not span_ok and total > 0:
        raise ValueError("col16=True: a slice column of this pattern spans 65536 columns or more")
    if total == 0:        # no stored entry at all: keep the arrays addressable (the C ABI refuses null pointers, and torch
        return slice_ptr, (torch.zeros(64, dtype=torch.int32, device=dev),), 0      # reports one for every EMPTY tensor)
    if col16 in ("auto", True) and span_ok:
        delta = blocks - cmin                                        # 0 .. 65535
        delta = torch.where(delta >= 32768, delta - 65536, delta).to(torch.int16)   # the same 16 bits, as torch can hold them
        return slice_ptr, (cmin[:, 0].contiguous(), delta.reshape(-1).contiguous()), total
    return slice_ptr, (s_cols.contiguous(),), total


def sell_positions(rowptr, n, slice_ptr, packed=False):
    """position of every CSR element in the SELL arrays of ``sell_layout`` (int64 [nnz]); ``packed``: in the per-element
    arrays of the value-coded layout (four slice columns to a lane: 256 G + 4 l + j, include/dsea.h dsea_op_create_sell16v8)"""
    lens = rowptr[1:] - rowptr[:-1]
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=rowptr.device), lens)
    k = torch.arange(rows.numel(), dtype=torch.int64, device=rowptr.device) - rowptr[rows]
    if packed:
        return slice_ptr[rows // 64] + (k // 4) * 256 + (rows % 64) * 4 + (k % 4)
    return slice_ptr[rows // 64] + k * 64 + (rows % 64)


def pack2(a):
    """... -> two slice columns to a lane (dsea_op_create_sell16p2; slices hold multiples of 128)"""
    return a.view(-1, 2, 64).permute(0, 2, 1).contiguous().view(-1)


def pack4(a):
    """a per-element SELL array in slice-column-major order -> four slice columns to a lane (slices hold multiples of 256)"""
    return a.view(-1, 4, 64).permute(0, 2, 1).contiguous().view(-1)


def value_codes(data, limit=255):
    """(table float64 [256], codes uint8 [nnz]) with data == table[codes] BIT FOR BIT and table[0] = 0.0 (the padding's
    code), or None when ``data`` takes more than ``limit`` distinct bit patterns.  A strided sample is looked at first, so
    that a matrix of arbitrary values costs one small sort."""
    bits = data.detach().contiguous().view(torch.int64)
    if bits.numel() > (1 << 16):
        step = bits.numel() >> 16
        if torch.unique(bits[::step]).numel() > limit:
            return None
    uniq, inv = torch.unique(bits, return_inverse=True)
    if uniq.numel() > limit:
        return None
    table = torch.zeros(256, dtype=torch.int64, device=data.device)
    table[1:1 + uniq.numel()] = uniq
    return table.view(F64), (inv + 1).to(torch.uint8)


class CSROperator:
    """General sparse symmetric matrix given in CSR (rowptr int64, colidx int32, vals fp64) on the device.

    The mat-vec kernel reads a SELL-64 copy (sliced ELLPACK, slices of one wave = 64 rows, column-major inside a
    slice) built once here on the device with torch index ops: matrix loads become perfectly coalesced and, for
    banded / structured operators, so does the gather of x; where the pattern allows it the columns are stored as
    16-bit deltas (10 instead of 12 bytes per non-zero: the kernel is bound by the bytes it moves).
    ``layout="csr"`` keeps the plain CSR kernel.  ``from_scipy`` / ``from_dense`` build the CSR arrays on the host once.

    THE MATRIX AS A PARAMETER (reference README.md:88-126, symeig.py:56-64,82-84: the adjoint A-bar = v1 v2^T is pushed to
    the parameters that produced A).  ``vals`` may be a leaf tensor with ``requires_grad``:

        op = CSROperator(rowptr, colidx, vals, n)                       # vals: nn.Parameter-like, fp64, on the device
        symeig.setDominantSparseSymeig(op, op.Aadjoint_to_valsadjoint)  # hook: vals-bar[e] = v1[row e] v2[col e]
        E0, psi = symeig.DominantSparseSymeig.apply(op.vals, k, n)
        loss.backward(); optimiser.step()                               # in-place update of vals ...
        E0, psi = symeig.DominantSparseSymeig.apply(op.vals, k, n)      # ... is picked up: the SELL copy is refreshed in
                                                                        #     place (dsea_op_update_vals), no rebuild

    The hooks are differentiable (second order: examples/TFIM/E0.py:63-64 pattern) -- their backward is a mat-vec with
    the incoming gradient as the values of the same pattern.  ``Aadjoint_to_valsadjoint_symmetric`` is the adjoint for a
    matrix whose entry pairs (i,j), (j,i) are tied, i.e. of  vals -> eigh((M + M^T)/2)."""

    _native_methods = ("__call__",)

    def __init__(self, rowptr, colidx, vals, n, layout="sell", col16="auto", values="auto"):
        self.n = int(n)
        self.rowptr = rowptr.to(torch.int64).contiguous()
        self.colidx = colidx.to(torch.int32).contiguous()
        data = vals.detach()
        if data.dtype != F64 or not data.is_contiguous():
            data = data.to(F64).contiguous()
            self._vals = data         # a converted copy: not the caller's storage (no parameter semantics)
        else:
            self._vals = vals         # the caller's tensor: its in-place updates are seen by refresh()
        self._vals_data = data
        self._seen_version = None
        self.nnz = int(data.numel())
        self.device = data.device
        self.layout = layout
        if self.device.type != "cuda":
            raise ValueError("CSROperator is a device operator")
        self._T = None
        raw = c_void_p()
        lib = _lib.load()
        if layout == "sell":
            nsl = (self.n + 63) // 64
            import os as _os
            if values == "auto":
                values = _os.environ.get("DSEA_SELL_VALUES", "auto")      # A/B switch: "plain" | "auto" | "coded"
            if values not in ("auto", "plain", "coded"):
                raise ValueError("values must be 'auto', 'plain' or 'coded'")
            # VALUE CODES (include/dsea.h dsea_op_create_sell16v8): few distinct stored values -> a uint8 per element into a
            # table of 256 doubles, 3 instead of 10 bytes per non-zero, bit-identical products.  Not for a parameter (its
            # values spread with the first optimiser step) unless asked for.
            coded = None
            if values != "plain" and col16 is not False and self.nnz > 0 and (values == "coded" or not vals.requires_grad):
                coded = value_codes(data)
            if coded is not None:
                slice_ptr, cols, total = sell_layout(self.rowptr, self.colidx, self.n, col16, pad_cols=4)
                if len(cols) != 2:
                    coded = None          # (a slice column spans 65536 columns or more: 32-bit columns, fp64 values)
            if values == "coded" and coded is None:
                raise ValueError("values='coded' needs 16-bit columns and at most 255 distinct stored values")
            self._coded = coded is not None
            if self._coded:
                self._vtab = coded[0]
                self._codes = torch.zeros(total, dtype=torch.uint8, device=self.device)
                self._codes[sell_positions(self.rowptr, self.n, slice_ptr, packed=True)] = coded[1]
                cols = (cols[0], pack4(cols[1]))
                check(lib.dsea_op_create_sell16v8(self.n, nsl, c_void_p(slice_ptr.data_ptr()), c_void_p(cols[0].data_ptr()),
                                                  c_void_p(cols[1].data_ptr()), c_void_p(self._codes.data_ptr()),
                                                  c_void_p(self._vtab.data_ptr()), byref(raw)), "dsea_op_create_sell16v8")
                self._sell = (slice_ptr,) + tuple(cols) + (None,)
                keep = self._sell + (self._codes, self._vtab)
            else:
                slice_ptr, cols, total = self._plain_layout(col16)
                s_vals = torch.zeros(max(total, 1), dtype=F64, device=self.device)
                raw = self._create_plain(slice_ptr, cols, s_vals)
                self._sell = (slice_ptr,) + tuple(cols) + (s_vals,)
                keep = self._sell
            self._sell_total = total
            self.col16 = len(cols) == 2
        elif layout == "csr":
            # (a matrix without a stored entry -- e.g. a slab that is all padding: one addressable dummy element per array)
            c_arr = self.colidx if self.nnz else torch.zeros(1, dtype=torch.int32, device=self.device)
            v_arr = data if self.nnz else torch.zeros(1, dtype=F64, device=self.device)
            check(lib.dsea_op_create_csr(self.n, self.nnz, c_void_p(self.rowptr.data_ptr()),
                                         c_void_p(c_arr.data_ptr()), c_void_p(v_arr.data_ptr()),
                                         byref(raw)), "dsea_op_create_csr")
            self.col16 = False
            keep = (self.rowptr, c_arr, v_arr)
        else:
            raise ValueError("layout must be 'sell' or 'csr'")
        self._H = _NativeView(_Handle(raw, self.n, keep))
        import os as _os
        if layout == "sell":
            self._hint_width(raw)
        if layout == "sell" and _os.environ.get("DSEA_SELL_NT", "") == "1" and (getattr(self, "_pack2", False) or self._coded):
            raise ValueError("DSEA_SELL_NT=1 is an A/B switch of the unpacked layout: set DSEA_SELL_PACK2=0 and DSEA_SELL_VALUES=plain")
        if layout == "sell" and _os.environ.get("DSEA_SELL_NT", "") in ("0", "1"):     # A/B switch (tools/gpu_evidence.sh abenv)
            check(lib.dsea_op_set_tuning(raw, _lib.TUNE_SELL_NT, int(_os.environ["DSEA_SELL_NT"])), "dsea_op_set_tuning")
        self._seen_version = None
        if getattr(self, "_coded", False):
            self._seen_version = self.vals._version        # (the codes were just taken from these values)
        else:
            self.refresh()

    def _hint_width(self, raw):
        """tell the library the widest slice (LDS reservation of the parameter kernels: dsea_op_set_tuning DSEA_TUNE_SELL_MAX_WIDTH)"""
        sp = self._sell[0]
        width = int(((sp[1:] - sp[:-1]).max().item()) // 64) if sp.numel() > 1 else 0
        check(_lib.load().dsea_op_set_tuning(raw, _lib.TUNE_SELL_MAX_WIDTH, width), "dsea_op_set_tuning")

    def _plain_layout(self, col16):
        """(slice_ptr, columns, total) of the fp64-value SELL layout: with 16-bit deltas the per-element arrays are packed two
        slice columns to a lane (include/dsea.h dsea_op_create_sell16p2; DSEA_SELL_PACK2=0: the unpacked layout, for A/B)"""
        import os as _os
        self._pack2 = False
        if col16 is not False and _os.environ.get("DSEA_SELL_PACK2", "1") != "0":
            slice_ptr, cols, total = sell_layout(self.rowptr, self.colidx, self.n, col16, pad_cols=2)
            if len(cols) == 2:
                self._pack2 = True
                return slice_ptr, (cols[0], pack2(cols[1])), total
        return sell_layout(self.rowptr, self.colidx, self.n, col16)

    def _create_plain(self, slice_ptr, cols, s_vals):
        """SELL operand with fp64 values on this pattern (16- or 32-bit columns as ``cols`` has them)"""
        raw, lib, nsl = c_void_p(), _lib.load(), (self.n + 63) // 64
        if len(cols) == 2:
            create = lib.dsea_op_create_sell16p2 if getattr(self, "_pack2", False) else lib.dsea_op_create_sell16
            check(create(self.n, nsl, c_void_p(slice_ptr.data_ptr()), c_void_p(cols[0].data_ptr()),
                         c_void_p(cols[1].data_ptr()), c_void_p(s_vals.data_ptr()), byref(raw)),
                  "dsea_op_create_sell16(p2)")
        else:
            check(lib.dsea_op_create_sell(self.n, nsl, c_void_p(slice_ptr.data_ptr()), c_void_p(cols[0].data_ptr()),
                                          c_void_p(s_vals.data_ptr()), byref(raw)), "dsea_op_create_sell")
        return raw

    # -- the parameter tensor (reference: ``model.g`` / ``model.potential``): in-place updates are followed through its version
    #    counter; binding ANOTHER tensor of the same shape (``op.vals = new``) marks the device copy stale as well
    @property
    def vals(self):
        return self._vals

    @vals.setter
    def vals(self, value):
        if value.numel() != self.nnz or value.device != self.device or value.dtype != F64 or not value.is_contiguous():
            raise ValueError("vals must be a contiguous float64 tensor of %d elements on %s" % (self.nnz, self.device))
        self._vals = value
        self._seen_version = None

    # -- structure shared, values replaced (the mat-vec M(G) x of the hooks' backward)
    def with_vals(self, vals):
        """an operator on the SAME pattern with other values (shares the SELL structure; one value array is allocated)"""
        if getattr(self, "_coded", False):      # (the value-coded layout pads and packs differently: a fresh fp64-value operator)
            return CSROperator(self.rowptr, self.colidx, vals.detach().to(F64).contiguous(), self.n, layout=self.layout, values="plain")
        twin = object.__new__(CSROperator)
        twin.__dict__.update({k: v for k, v in self.__dict__.items()
                              if k not in ("_H", "_sell", "_vals", "_vals_data", "_T", "_codes", "_vtab", "_coded")})
        data = vals.detach().to(F64).contiguous()
        twin._vals, twin._vals_data, twin._T = data, data, None
        raw = c_void_p()
        lib = _lib.load()
        if self.layout == "sell":
            s_vals = torch.zeros(max(self._sell_total, 1), dtype=F64, device=self.device)
            st = self._sell
            raw = self._create_plain(st[0], st[1:-1], s_vals)
            self._hint_width(raw)
            twin._sell = st[:-1] + (s_vals,)
            twin._coded = False
            keep = twin._sell
        else:
            check(lib.dsea_op_create_csr(self.n, self.nnz, c_void_p(self.rowptr.data_ptr()), c_void_p(self.colidx.data_ptr()),
                                         c_void_p(data.data_ptr()), byref(raw)), "dsea_op_create_csr")
            keep = (self.rowptr, self.colidx, data)
        twin._H = _NativeView(_Handle(raw, self.n, keep))
        twin._seen_version = None
        twin.refresh()
        return twin

    def refresh(self):
        """make the device operator's values equal ``vals`` as it is now (dsea_op_update_vals: the SELL copy is rewritten
        in place through rowptr, the layout is not rebuilt).  Called automatically when ``vals`` has been modified in
        place since the last look (optimiser step); call it yourself after writing through a view torch cannot see."""
        data = self.vals.detach()
        if self.nnz == 0:                   # nothing stored: nothing to rewrite
            self._seen_version = self.vals._version
            return
        if data.data_ptr() != self._vals_data.data_ptr():
            self._vals_data = data          # (vals re-bound to another tensor of the same shape)
        if getattr(self, "_coded", False):
            self._recode()
            if self._coded:
                self._seen_version = self.vals._version
                return
        check(_lib.load().dsea_op_update_vals(self._H.handle, c_void_p(self.rowptr.data_ptr()),
                                              c_void_p(self._vals_data.data_ptr()), engine._stream(self.device)),
              "dsea_op_update_vals")
        self._seen_version = self.vals._version

    def _recode(self):
        """value-coded operand whose values have changed: new table and codes IN PLACE (the handle stays), or -- once they no
        longer fit 255 codes -- the fp64 layout on the same pattern, built once (the handle changes: ``handle`` is read
        per call; a row-partitioned slab is never value-coded)"""
        coded = value_codes(self._vals_data)
        if coded is not None:
            self._vtab.copy_(coded[0])
            self._codes[sell_positions(self.rowptr, self.n, self._sell[0], packed=True)] = coded[1]
            return
        slice_ptr, cols, total = self._plain_layout(True)
        s_vals = torch.zeros(max(total, 1), dtype=F64, device=self.device)
        raw = self._create_plain(slice_ptr, cols, s_vals)
        self._sell = (slice_ptr,) + tuple(cols) + (s_vals,)
        self._hint_width(raw)
        self._sell_total = total
        self._coded = False
        del self._codes, self._vtab
        self._H = _NativeView(_Handle(raw, self.n, self._sell))

    def _current(self):
        # (plain CSR layout: the kernel reads the registered tensor itself, so only a re-bound ``vals`` needs the copy)
        if self._seen_version is None or (self.layout == "sell" and self._vals._version != self._seen_version):
            self.refresh()
        return self._H

    @classmethod
    def from_scipy(cls, M, device="cuda", layout="sell", col16="auto", values="auto"):
        M = M.tocsr()
        M.sort_indices()
        return cls(torch.from_numpy(M.indptr.astype("int64")).to(device),
                   torch.from_numpy(M.indices.astype("int32")).to(device),
                   torch.from_numpy(M.data.astype("float64")).to(device), M.shape[0], layout=layout, col16=col16, values=values)

    @classmethod
    def from_npz(cls, path, device="cuda", layout="sell"):
        """on-disk sparse symmetric operand: a file written by ``scipy.sparse.save_npz`` (any scipy sparse format)"""
        import scipy.sparse as sp
        return cls.from_scipy(sp.load_npz(path), device, layout=layout)

    @classmethod
    def from_dense(cls, A, device="cuda", layout="sell"):
        import scipy.sparse as sp
        return cls.from_scipy(sp.csr_matrix(A.detach().cpu().numpy()), device, layout=layout)

    @property
    def handle(self):
        return self._current().handle

    def __call__(self, v):
        return _SymmetricApply.apply(v, self._current())

    # -- the adjoint hooks (reference symeig.py:84 calls Aadjoint_to_padjoint(v1, v2) with A-bar = v1 v2^T)
    def Aadjoint_to_valsadjoint(self, v1, v2):
        """vals-bar[e] = v1[row(e)] * v2[col(e)], in the caller's CSR order (dsea_op_sddmm)"""
        return _SampledOuter.apply(v1, v2, self, False)

    def Aadjoint_to_valsadjoint_symmetric(self, v1, v2):
        """vals-bar[e] = (v1[row] v2[col] + v1[col] v2[row]) / 2"""
        return _SampledOuter.apply(v1, v2, self, True)

    def apply_with_vals(self, vals, v, transpose=False):
        """M(vals) v (or M(vals)^T v) on this operator's pattern, differentiable in ``vals`` and ``v``"""
        return _ValsApply.apply(vals, v, self, bool(transpose))

    def sddmm(self, v1, v2, symmetric=False, out=None, alpha=1.0, accumulate=False):
        """raw kernel call (no autograd): out[e] (+)= alpha * v1[row e] * v2[col e]"""
        v1, v2 = engine.as_vector(v1.detach(), self.n), engine.as_vector(v2.detach(), self.n)
        if out is None:
            out = torch.empty(self.nnz, dtype=F64, device=self.device)
        if self.nnz == 0:
            return out
        flags = (_lib.SDDMM_ACCUMULATE if accumulate else 0) | (_lib.SDDMM_SYMMETRIC if symmetric else 0)
        check(_lib.load().dsea_op_sddmm(self._H.handle, c_void_p(self.rowptr.data_ptr()), c_void_p(v1.data_ptr()),
                                        c_void_p(v2.data_ptr()), float(alpha), flags, c_void_p(out.data_ptr()),
                                        engine._stream(self.device)), "dsea_op_sddmm")
        return out

    def transposed(self):
        """(operator of the transposed PATTERN with this operator's values, perm) with vals_T = vals[perm]; built lazily
        (torch sort, once) -- the backward of the hooks needs M(G)^T x for non-symmetric G"""
        if self._T is None:
            n = self.n
            lens = self.rowptr[1:] - self.rowptr[:-1]
            rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=self.device), lens)
            cols = self.colidx.to(torch.int64)
            perm = torch.argsort(cols * n + rows)
            rowptr_t = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
            rowptr_t[1:] = torch.cumsum(torch.bincount(cols, minlength=n), 0)
            opT = CSROperator(rowptr_t, rows[perm].to(torch.int32), self._vals_data[perm], n, layout=self.layout)
            self._T = (opT, perm)
        return self._T


class _SampledOuter(torch.autograd.Function):
    """out[e] = v1[row e] v2[col e]  (sym: the average with v1 <-> v2) on a CSROperator's pattern.
    backward (G = gradient w.r.t. out, itself on the pattern):  v1-bar = M(G) v2,  v2-bar = M(G)^T v1  (sym: both averaged
    with their transposes) -- mat-vecs of the same SELL kernel, differentiable again through _ValsApply."""

    @staticmethod
    def forward(ctx, v1, v2, op, sym):
        ctx.op, ctx.sym = op, sym
        ctx.save_for_backward(v1, v2)
        return op.sddmm(v1, v2, symmetric=sym)

    @staticmethod
    def backward(ctx, G):
        v1, v2 = ctx.saved_tensors
        op, sym = ctx.op, ctx.sym
        g1 = g2 = None
        if ctx.needs_input_grad[0]:
            g1 = _ValsApply.apply(G, v2, op, False)
            if sym:
                g1 = 0.5 * (g1 + _ValsApply.apply(G, v2, op, True))
        if ctx.needs_input_grad[1]:
            g2 = _ValsApply.apply(G, v1, op, True)
            if sym:
                g2 = 0.5 * (g2 + _ValsApply.apply(G, v1, op, False))
        return g1, g2, None, None


class _ValsApply(torch.autograd.Function):
    """y = M(vals) x  /  M(vals)^T x  on a CSROperator's pattern, differentiable in vals and x."""

    @staticmethod
    def forward(ctx, vals, x, op, transpose):
        ctx.op, ctx.transpose = op, transpose
        ctx.save_for_backward(vals, x)
        if transpose:
            opT, perm = op.transposed()
            twin = opT.with_vals(vals.detach()[perm])
        else:
            twin = op.with_vals(vals)
        return engine.spmv(twin._H, engine.as_vector(x.detach(), op.n))

    @staticmethod
    def backward(ctx, gy):
        vals, x = ctx.saved_tensors
        op, tr = ctx.op, ctx.transpose
        gvals = gx = None
        if ctx.needs_input_grad[0]:       # y_r = sum_e vals_e x[col e]  ->  vals-bar_e = gy[row e] x[col e]   (transpose: swapped)
            gvals = _SampledOuter.apply(x, gy, op, False) if tr else _SampledOuter.apply(gy, x, op, False)
        if ctx.needs_input_grad[1]:
            gx = _ValsApply.apply(vals, gy, op, not tr)
        return gvals, gx, None, None


# ------------------------------------------------------------------------------------------ GEMM-shaped operands
class DenseOperator:
    """A dense real matrix (row-major device tensor) as a library operand of the NON-symmetric primitives
    (reference eig.py:28-30 hands the matrix to ARPACK); ``transpose=True`` applies A^T.  The mat-vec is libdsea's
    hand-written row-major GEMV (include/dsea.h: dsea_op_create_dense; HBM-bound, deterministic); for ``transpose=True`` the
    transposed matrix is materialised once so that both orientations stream rows."""

    _native_methods = ("__call__", "matvec")

    def __init__(self, A, transpose=False):
        if A.device.type != "cuda" or A.dim() != 2 or A.shape[0] != A.shape[1]:
            raise ValueError("DenseOperator takes a square CUDA matrix")
        self.transpose = bool(transpose)
        A = A.detach().to(F64)
        self.A = (A.T if self.transpose else A).contiguous()       # the matrix whose ROWS the kernel streams
        self.n = int(A.shape[0])
        self.shape = (self.n, self.n)
        self.device = self.A.device
        raw = c_void_p()
        check(_lib.load().dsea_op_create_dense(self.n, c_void_p(self.A.data_ptr()), self.n, 0, byref(raw)),
              "dsea_op_create_dense")
        self._H = _NativeView(_Handle(raw, self.n, self.A))

    @property
    def handle(self):
        return self._H.handle

    def matvec(self, v):
        return engine.spmv(self._H, v)

    __call__ = matvec


class SymmetricDenseOperator:
    """A dense real SYMMETRIC matrix as a native operand of the symmetric primitives (reference symeig.py:15-31,
    CG.py:43-71 apply ``torch.matmul(A, v)``): hand-written HIP mat-vec that reads only the UPPER triangle, each
    64 x 64 tile once for both its row and its column block -- half the bytes of a GEMV -- and lets the dense
    primitive run its Lanczos / CG loops inside libdsea like the sparse ones (no Python per iteration).

    Handed to ``setDominantSparseSymeig(op, hook)`` it is also the way to get the adjoint of a LARGE dense matrix in
    its lazy rank-1 form: the hook receives (v1, v2) with A-bar = v1 v2^T (reference symeig.py:56-64) and contracts
    them with whatever produced A -- the n x n gradient of ``DominantSymeig`` (symeig.py:29) is never formed."""

    _native_methods = ("__call__", "matvec")

    def __init__(self, A):
        if A.device.type != "cuda" or A.dim() != 2 or A.shape[0] != A.shape[1]:
            raise ValueError("SymmetricDenseOperator takes a square CUDA matrix")
        self.n = int(A.shape[0])
        A = A.detach()
        if A.dtype not in (F64, torch.float32):
            A = A.to(F64)
        if self.n % 2:   # rows are read as element pairs: pad the leading dimension to an even number
            Ap = torch.zeros((self.n, self.n + 1), dtype=A.dtype, device=A.device)
            Ap[:, : self.n] = A
            self.A, lda = Ap, self.n + 1
        else:
            self.A, lda = A.contiguous(), self.n
        if self.A.data_ptr() % 16:
            self.A = self.A.clone()
        self.shape = (self.n, self.n)
        self.device = self.A.device
        lib = _lib.load()
        self._work = torch.empty(lib.dsea_op_symdense_work_bytes(self.n) // 8, dtype=F64, device=self.device)
        raw = c_void_p()
        check(lib.dsea_op_create_symdense(self.n, c_void_p(self.A.data_ptr()), self.A.element_size(), lda,
                                          c_void_p(self._work.data_ptr()), byref(raw)), "dsea_op_create_symdense")
        self._H = _NativeView(_Handle(raw, self.n, (self.A, self._work)))

    @property
    def handle(self):
        return self._H.handle

    def matvec(self, v):
        """A v, differentiable in v (dy/dv^T g = A g: the same symmetric kernel, re-entrant)"""
        return _SymmetricApply.apply(v, self._H)

    __call__ = matvec


def dense_symmetric_operand(A):
    """native operand for a dense symmetric tensor: the upper-triangle kernel where it wins (measured on MI355X:
    n = 6144: 50 vs 74 us, n = 16384: 317 vs 439 us for the rocBLAS GEMV), the library's rocBLAS GEMV operand below
    (n = 4096: 29 vs 21 us -- two launches do not pay off there).  Either way the Lanczos / CG
    loops run inside libdsea."""
    if A.shape[0] >= 6144 or (A.dtype == torch.float32 and A.shape[0] >= 2048):
        return SymmetricDenseOperator(A)      # fp32 matrices are read as fp32: no promoted copy (Lanczos.py:47)
    try:
        return DenseOperator(A)
    except _lib.DseaError as exc:
        # no rocBLAS in this process (dsea_op_create_dense -> DSEA_ERR_UNSUPPORTED on another ROCm stack): the
        # hand-written upper-triangle mat-vec has no such dependency -- still inside the library, no torch arithmetic
        if "unsupported" not in str(exc):
            raise
        return SymmetricDenseOperator(A)


class TransferOperator:
    """MPS transfer matrix of a real rank-3 tensor A (d, D, D) acting on D x D matrices stored as D^2-vectors
    (reference examples/TFIM_vumps/general.py:59-66):

        transpose=False:  r -> sum_s A_s r A_s^T      ("Gong",  the reference's ``fr``)
        transpose=True :  l -> sum_s A_s^T l A_s      ("GongT", the reference's ``fl``)

    applied by libdsea as one strided-batched fp64 GEMM + one GEMM of depth d*D (rocBLAS) -- the explicit D^2 x D^2
    matrix of ``matrix_forward`` (general.py:47-49) would be 550 GB at D = 512."""

    _native_methods = ("__call__", "matvec")

    def __init__(self, A, transpose=False):
        if A.device.type != "cuda" or A.dim() != 3 or A.shape[1] != A.shape[2]:
            raise ValueError("TransferOperator takes a CUDA tensor of shape (d, D, D)")
        # a private fp64 COPY: the operator is a snapshot of A at construction, whatever path applies it (the hand-written
        # kernels read a fragment-packed copy made by dsea_op_create_transfer, the rocBLAS path reads this tensor) -- an
        # in-place update of the caller's tensor is never seen; build a new operator for a new A (general.py:59 does)
        self.A = A.detach().to(F64).clone(memory_format=torch.contiguous_format)
        self.d, self.D = int(A.shape[0]), int(A.shape[1])
        self.n = self.D * self.D
        self.shape = (self.n, self.n)
        self.device = self.A.device
        self.transpose = bool(transpose)
        lib = _lib.load()
        nbytes = lib.dsea_op_transfer_work_bytes(self.D, self.d)
        self._work = torch.empty(nbytes // 8, dtype=F64, device=self.device)
        raw = c_void_p()
        check(lib.dsea_op_create_transfer(self.D, self.d, c_void_p(self.A.data_ptr()), int(self.transpose),
                                          c_void_p(self._work.data_ptr()), engine._stream(self.device), byref(raw)),
              "dsea_op_create_transfer")
        self._H = _NativeView(_Handle(raw, self.n, (self.A, self._work)))

    @property
    def handle(self):
        return self._H.handle

    def matvec(self, v):
        return engine.spmv(self._H, v)

    __call__ = matvec
