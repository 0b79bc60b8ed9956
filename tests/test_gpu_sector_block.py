"""k_spmv_sector_block on the GPU (docs/design/27-finite-temperature.md): the bond-list sector Hamiltonian applied to a block of
R vectors, at the geometries of tests/test_gpu_sector.py that reach each path of the kernel, for every block width.

    L2-1 L3-1 L3-2 L5-2   less than a wave, odd n          L16-8          many blocks
    L7-3-split            odd L                            L20-10-walk    blocks walk row ranges (grid capped at 2^6)
    L9-4-cap              full bond table                  L34-2 L40-2    states wider than 32 bits
    L11-5                 two blocks, ragged

Column j of the block result must equal the single-vector mat-vec ``op.H`` of column j BIT FOR BIT, and lie within 1e-13
(relative norm, the project's bar for one application) of the numpy reference.
"""
import functools
import math
from ctypes import c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sector_reference as ref  # noqa: E402
import test_gpu_sector as base  # noqa: E402
from dominantsparseeigenad_amd import _lib  # noqa: E402
from dominantsparseeigenad_amd.engine import _stream  # noqa: E402
from dominantsparseeigenad_amd.operators import SpinLatticeOperator  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402

F64 = torch.float64
NAMES = ["L2-1", "L3-1", "L3-2", "L5-2", "L7-3-split", "L9-4-cap", "L11-5", "L16-8", "L20-10-walk", "L34-2", "L40-2"]
WIDTHS = [1, 2, 4, 8]
ONE_APPLICATION = 1e-13
ERR_ARG, ERR_ALIGN = -1, -2


@functools.lru_cache(maxsize=None)
def block_case(name, R=8):
    """(couplings, X (n, R), H X from the numpy reference) on the host, computed once per geometry and never written to"""
    L, ndown, _, bonds = base.GEOMETRY[name]
    p = base.couplings(L, bonds, "random")
    n = math.comb(L, ndown)
    X = np.stack([normal_vector(n, 27000 + 10 * L + ndown + j) for j in range(R)], axis=1)
    Y = np.stack([ref.apply(L, ndown, bonds, p, X[:, j]) for j in range(R)], axis=1)
    for a in (p, X, Y):
        a.setflags(write=False)
    return p, X, Y


def test_the_geometries_are_the_ones_of_the_single_vector_tests():
    assert all(name in base.GEOMETRY for name in NAMES)
    assert base.GEOMETRY["L20-10-walk"][2] == 6 and len(base.GEOMETRY["L9-4-cap"][3]) == _lib.LATTICE_MAX_BONDS


@pytest.mark.parametrize("R", WIDTHS)
@pytest.mark.parametrize("name", NAMES)
def test_every_column_is_the_single_vector_mat_vec_bit_for_bit(name, R):
    p, X, Y = block_case(name)
    op = base.operator(name, p)
    Xd = base.to_dev(X[:, :R])
    got = op.apply_block(Xd)
    assert got.shape == (op.n, R) and got.dtype == F64 and got.is_contiguous()
    worst = 0.0
    for j in range(R):
        single = op.H(Xd[:, j].contiguous())
        assert torch.equal(got[:, j], single), (name, R, j)
        worst = max(worst, base.relnorm(got[:, j].cpu().numpy(), Y[:, j]))
    print("%s R = %d: worst column against the numpy reference %.2e (bar %.0e)" % (name, R, worst, ONE_APPLICATION))
    assert worst <= ONE_APPLICATION
    assert torch.equal(op.apply_block(Xd), got)                 # repeated calls: identical bits
    assert torch.equal(Xd, base.to_dev(X[:, :R]))                # the input is not written


@pytest.mark.parametrize("name", ["L5-2", "L11-5"])
@pytest.mark.parametrize("R", [3, 13])
def test_other_widths_go_through_the_host_split(name, R):
    L, ndown, _, bonds = base.GEOMETRY[name]
    p, _, _ = block_case(name)
    op = base.operator(name, p)
    n = op.n
    X = np.stack([normal_vector(n, 27500 + j) for j in range(R)], axis=1)
    Xd = base.to_dev(X)
    got = op.apply_block(Xd)
    assert got.shape == (n, R)
    for j in range(R):
        assert torch.equal(got[:, j], op.H(Xd[:, j].contiguous())), (name, R, j)
        assert base.relnorm(got[:, j].cpu().numpy(), ref.apply(L, ndown, bonds, p, X[:, j])) <= ONE_APPLICATION


def test_views_and_tensors_with_grad_are_taken_as_plain_blocks():
    p, X, _ = block_case("L11-5")
    op = base.operator("L11-5", p)
    Xd = base.to_dev(X)
    want = op.apply_block(Xd)
    assert torch.equal(op.apply_block(Xd[:, 2:6]), want[:, 2:6])                       # a strided view of four columns
    assert torch.equal(op.apply_block(Xd.t().contiguous().t()), want)                  # column-major storage
    leaf = Xd.clone().requires_grad_(True)
    out = op.apply_block(leaf)
    assert not out.requires_grad and torch.equal(out, want)
    for bad in (Xd[:, 0], Xd[:-1], Xd[:, :0], Xd.cpu()):
        with pytest.raises(ValueError):
            op.apply_block(bad)


def test_the_abi_refuses_what_the_header_says():
    lib = _lib.load()
    p, X, _ = block_case("L11-5")
    op = base.operator("L11-5", p)
    n = op.n
    Xd = base.to_dev(X)
    Yd = torch.empty_like(Xd)
    st = _stream(Xd.device)
    ptr = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    assert lib.dsea_op_sector_block_apply(op.handle, 8, ptr(Xd), ptr(Yd), st) == 0
    L, ndown, _, bonds = base.GEOMETRY["L11-5"]
    full = SpinLatticeOperator(L, bonds, torch.zeros(3 * len(bonds) + 2 * L, dtype=F64, device=Xd.device))
    pair = op.pair_operator()
    for handle in (full.handle, pair.handle, None):
        assert lib.dsea_op_sector_block_apply(handle, 8, ptr(Xd), ptr(Yd), st) == ERR_ARG
    for R in (0, 3, 5, 16, -1):
        assert lib.dsea_op_sector_block_apply(op.handle, R, ptr(Xd), ptr(Yd), st) == ERR_ARG
    assert lib.dsea_op_sector_block_apply(op.handle, 8, None, ptr(Yd), st) == ERR_ARG
    assert lib.dsea_op_sector_block_apply(op.handle, 8, ptr(Xd), None, st) == ERR_ARG
    assert lib.dsea_op_sector_block_apply(op.handle, 8, ptr(Xd), ptr(Xd), st) == ERR_ARG
    odd = torch.empty(n * 8 + 1, dtype=F64, device=Xd.device)[1:]
    assert odd.data_ptr() % 16 == 8
    assert lib.dsea_op_sector_block_apply(op.handle, 8, ptr(odd), ptr(Yd), st) == ERR_ALIGN
    assert lib.dsea_op_sector_block_apply(op.handle, 8, ptr(Xd), ptr(odd), st) == ERR_ALIGN
    # the recurrence
    k = 4
    Q, W = Xd.clone(), torch.empty_like(Xd)
    norm2 = torch.empty(8, dtype=F64, device=Xd.device)
    alphas, betas = torch.empty((k, 8), dtype=F64, device=Xd.device), torch.empty((k, 8), dtype=F64, device=Xd.device)
    steps = torch.empty(8, dtype=torch.int32, device=Xd.device)
    scratch = torch.empty(64 + 16 * ((n + 255) // 256), dtype=F64, device=Xd.device)
    good = [op.handle, 8, k, ptr(Q), ptr(W), ptr(norm2), ptr(alphas), ptr(betas), ptr(steps), ptr(scratch), st]

    def call(**change):
        args = list(good)
        for index, value in change.items():
            args[int(index[1:])] = value
        return lib.dsea_op_sector_block_lanczos(*args)

    for handle in (full.handle, pair.handle, None):
        assert call(a0=handle) == ERR_ARG
    for R in (0, 3, 16):
        assert call(a1=R) == ERR_ARG
    for bad_k in (0, -1):
        assert call(a2=bad_k) == ERR_ARG
    for slot in range(3, 10):
        assert call(**{"a%d" % slot: None}) == ERR_ARG
    assert call(a4=ptr(Q)) == ERR_ARG                                                   # Q == W
    assert call(a3=ptr(odd)) == ERR_ALIGN and call(a4=ptr(odd)) == ERR_ALIGN
    torch.cuda.synchronize()
    assert torch.equal(Q, Xd)                                                           # nothing refused has run
    assert call() == 0
    torch.cuda.synchronize()
    assert steps.tolist() == [k] * 8
