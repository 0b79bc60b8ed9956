"""k_spmv_hubbard_block on the GPU (docs/design/28-hubbard-finite-temperature.md): the Hubbard Hamiltonian applied to a block of R
vectors, at the 15 geometries of tests/test_gpu_hubbard.py -- the smallest that reach each path of the row work (n_dn below a
wave, n_dn = 70 straddling an ru boundary, a ragged last block, the full bond table, fewer bonds than a chunk and a bond count
that is no multiple of one, two different table sets in both orders, row ranges walked by a capped grid, words wider than 32
bits) -- for every block width.

Column j of the block result must equal the single-vector mat-vec ``op.H`` of column j BIT FOR BIT, and lie within 1e-13
(relative norm, the project's bar for one application) of the numpy reference.
"""
import functools
from ctypes import c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hubbard_reference as ref  # noqa: E402
import test_gpu_hubbard as base  # noqa: E402
from test_gpu_hubbard import GEOMETRY, couplings, operator  # noqa: E402
from dominantsparseeigenad_amd import _lib  # noqa: E402
from dominantsparseeigenad_amd.engine import _stream  # noqa: E402
from dominantsparseeigenad_amd.operators import SpinSectorOperator, hubbard_dim, ring_bonds  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402

F64 = torch.float64
NAMES = list(GEOMETRY)
WIDTHS = [1, 2, 4, 8]
ONE_APPLICATION = 1e-13
ERR_ARG, ERR_ALIGN = -1, -2


@functools.lru_cache(maxsize=None)
def block_case(name, R=8):
    """(couplings, X (n, R), H X from the numpy reference) on the host, computed once per geometry and never written to"""
    L, nup, ndn, _, bonds = GEOMETRY[name]
    p = couplings(L, bonds, "random")
    n = hubbard_dim(L, nup, ndn)
    X = np.stack([normal_vector(n, 28000 + 10 * L + nup + j) for j in range(R)], axis=1)
    Y = np.stack([ref.apply(L, nup, ndn, bonds, p, X[:, j]) for j in range(R)], axis=1)
    for a in (p, X, Y):
        a.setflags(write=False)
    return p, X, Y


def test_the_geometries_are_the_ones_of_the_single_vector_tests():
    assert len(NAMES) == 15
    assert GEOMETRY["L10-5-5-walk"][3] == 6 and len(GEOMETRY["L9-3-5-cap"][4]) == _lib.LATTICE_MAX_BONDS
    assert len(GEOMETRY["L7-3-2-split"][4]) == 4          # fewer bonds than a chunk of four, two chunks of two
    assert hubbard_dim(*GEOMETRY["L8-4-4-complete"][:3]) == 70 * 70


@pytest.mark.parametrize("R", WIDTHS)
@pytest.mark.parametrize("name", NAMES)
def test_every_column_is_the_single_vector_mat_vec_bit_for_bit(name, R):
    p, X, Y = block_case(name)
    op = operator(name, p)
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


@pytest.mark.parametrize("name", ["L5-2-3", "L8-4-4-complete"])
@pytest.mark.parametrize("R", [3, 13])
def test_other_widths_go_through_the_host_split(name, R):
    L, nup, ndn, _, bonds = GEOMETRY[name]
    p, _, _ = block_case(name)
    op = operator(name, p)
    n = op.n
    X = np.stack([normal_vector(n, 28500 + j) for j in range(R)], axis=1)
    Xd = base.to_dev(X)
    got = op.apply_block(Xd)
    assert got.shape == (n, R)
    for j in range(R):
        assert torch.equal(got[:, j], op.H(Xd[:, j].contiguous())), (name, R, j)
        assert base.relnorm(got[:, j].cpu().numpy(), ref.apply(L, nup, ndn, bonds, p, X[:, j])) <= ONE_APPLICATION


def test_views_and_tensors_with_grad_are_taken_as_plain_blocks():
    p, X, _ = block_case("L8-4-4-complete")
    op = operator("L8-4-4-complete", p)
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
    name = "L8-4-4-complete"
    p, X, _ = block_case(name)
    op = operator(name, p)
    n = op.n
    Xd = base.to_dev(X)
    Yd = torch.empty_like(Xd)
    st = _stream(Xd.device)
    ptr = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    assert lib.dsea_op_hubbard_block_apply(op.handle, 8, ptr(Xd), ptr(Yd), st) == 0
    spin = SpinSectorOperator(8, ring_bonds(8), torch.zeros(2 * 8 + 8, dtype=F64, device=Xd.device), 4)
    for handle in (spin.handle, None):
        assert lib.dsea_op_hubbard_block_apply(handle, 8, ptr(Xd), ptr(Yd), st) == ERR_ARG
    assert lib.dsea_op_sector_block_apply(op.handle, 8, ptr(Xd), ptr(Yd), st) == ERR_ARG
    for R in (0, 3, 5, 16, -1):
        assert lib.dsea_op_hubbard_block_apply(op.handle, R, ptr(Xd), ptr(Yd), st) == ERR_ARG
    assert lib.dsea_op_hubbard_block_apply(op.handle, 8, None, ptr(Yd), st) == ERR_ARG
    assert lib.dsea_op_hubbard_block_apply(op.handle, 8, ptr(Xd), None, st) == ERR_ARG
    assert lib.dsea_op_hubbard_block_apply(op.handle, 8, ptr(Xd), ptr(Xd), st) == ERR_ARG
    odd = torch.empty(n * 8 + 1, dtype=F64, device=Xd.device)[1:]
    assert odd.data_ptr() % 16 == 8
    assert lib.dsea_op_hubbard_block_apply(op.handle, 8, ptr(odd), ptr(Yd), st) == ERR_ALIGN
    assert lib.dsea_op_hubbard_block_apply(op.handle, 8, ptr(Xd), ptr(odd), st) == ERR_ALIGN
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
        return lib.dsea_op_hubbard_block_lanczos(*args)

    for handle in (spin.handle, None):
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
