"""The basis-free block Lanczos recurrence stage by stage (docs/design/36-block-lanczos-stage-tests.md): k_sblock_norm,
k_sblock_update, k_sblock_finish, the LZ instantiations of k_spmv_sector_block and k_spmv_hubbard_block, block_spmv_tail<R, true>,
block_partials and sum_partials_block, through dsea_op_sector_block_lanczos and dsea_op_hubbard_block_lanczos called with ctypes,
one library call per run, everything downloaded and judged by tests/block_lanczos_reference.py -- EXACT inputs bit for bit
(norm2, alphas, betas, steps and both returned blocks; every break decision), RANDOM inputs step by step against the fp64 mirror
and np.longdouble with bounds that count operations.  tests/test_block_lanczos_reference_cpu.py shows without a GPU that the same
``Checks`` reject wrong kernels.

Only the whole run is exported, so a stage is isolated by the run length: runs of k = 1 ... 4 steps on the same start block.

Every call: Q and W sit in buffers with a NaN tail (W is NaN throughout: the first step must not read it), alphas / betas have a
sentinel row behind row k - 1, norm2 and steps sentinels behind entry R - 1, scratch is exactly the queried number of doubles,
NaN, with sentinels behind it.  After the call every tail and sentinel must be unchanged bit for bit."""
from ctypes import byref, c_int64, c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import block_lanczos_reference as ref  # noqa: E402
from block_lanczos_reference import SENTINEL, STEPS_SENTINEL, Checks, Run  # noqa: E402
from test_gpu_cg_stages import Buf, dev, scalars  # noqa: E402
from dominantsparseeigenad_amd import _lib  # noqa: E402
from dominantsparseeigenad_amd.engine import _ptr, _stream  # noqa: E402
from dominantsparseeigenad_amd.operators import HubbardOperator, SpinSectorOperator  # noqa: E402

CASES = ref.cases()
EXACT = [(name, R) for name in ref.ALL for R in ref.widths(name, False)]
RANDOM = [(name, R) for name in ref.ALL for R in ref.widths(name, True)]


class Library:
    """the interface block_lanczos_reference.Checks drives: one library call per ``run`` and per ``apply``"""

    def __init__(self):
        self.lib = _lib.load()
        self.ops = {}

    def operator(self, case, p):
        """one operator per case (the tables are built once); the couplings are rewritten in place"""
        if case.name not in self.ops:
            pd = torch.from_numpy(np.array(p, dtype=np.float64)).to(dev())
            if case.kind == "sector":
                op = SpinSectorOperator(case.L, case.bonds, pd, case.fill)
            else:
                op = HubbardOperator(case.L, case.bonds, pd, case.fill[0], case.fill[1])
            if case.grid is not None:
                op.set_grid_log2(case.grid)
            assert op.n == case.n
            self.ops[case.name] = op
        op = self.ops[case.name]
        with torch.no_grad():
            op.couplings.copy_(torch.from_numpy(np.array(p, dtype=np.float64)))
        return op

    def entries(self, case):
        if case.kind == "sector":
            return (lambda R, out: self.lib.dsea_op_sector_block_lanczos_scratch_doubles(case.L, case.fill, R, out),
                    self.lib.dsea_op_sector_block_lanczos, self.lib.dsea_op_sector_block_apply)
        return (lambda R, out: self.lib.dsea_op_hubbard_block_lanczos_scratch_doubles(case.L, case.fill[0], case.fill[1], R, out),
                self.lib.dsea_op_hubbard_block_lanczos, self.lib.dsea_op_hubbard_block_apply)

    def run(self, case, p, Phi, k, fast=None):
        op = self.operator(case, p)
        n, R = Phi.shape
        query, run, _ = self.entries(case)
        need = c_int64(-1)
        _lib.check(query(R, byref(need)), "scratch_doubles")
        assert need.value == case.scratch_doubles(R)
        Q, W = Buf(np.ascontiguousarray(Phi).reshape(-1)), Buf(np.full(n * R, np.nan))
        norm2, steps = scalars([SENTINEL] * (R + 2)), torch.full((R + 2,), STEPS_SENTINEL, dtype=torch.int32, device=dev())
        alphas, betas = scalars([SENTINEL] * ((k + 1) * R)), scalars([SENTINEL] * ((k + 1) * R))
        scratch = scalars([np.nan] * need.value + [SENTINEL] * 4)
        _lib.check(run(op.handle, R, k, Q.ptr, W.ptr, _ptr(norm2), _ptr(alphas), _ptr(betas), c_void_p(steps.data_ptr()),
                       _ptr(scratch), _stream(dev())), "block_lanczos")
        what = "%s R=%d k=%d" % (case, R, k)
        nh, ah, bh, sh = norm2.cpu().numpy(), alphas.cpu().numpy(), betas.cpu().numpy(), steps.cpu().numpy()
        assert (nh[R:] == SENTINEL).all() and (sh[R:] == STEPS_SENTINEL).all(), "%s: norm2 or steps written behind entry R - 1" % what
        assert (ah[k * R:] == SENTINEL).all() and (bh[k * R:] == SENTINEL).all(), "%s: alphas or betas written behind row k - 1" % what
        assert (scratch[need.value:].cpu().numpy() == SENTINEL).all(), "%s: scratch written behind the queried size" % what
        return Run(nh[:R], ah[:k * R].reshape(k, R), bh[:k * R].reshape(k, R), sh[:R],
                   Q.down(what + " Q").reshape(n, R), W.down(what + " W").reshape(n, R))

    def apply(self, case, p, X):
        op = self.operator(case, p)
        n, R = X.shape
        _, _, apply = self.entries(case)
        Xb, Yb = Buf(np.ascontiguousarray(X).reshape(-1)), Buf(np.full(n * R, SENTINEL))
        _lib.check(apply(op.handle, R, Xb.ptr, Yb.ptr, _stream(dev())), "block_apply")
        Xb.kept("block_apply X")
        return Yb.down("block_apply Y").reshape(n, R)


LIBRARY = []


def checks():
    # (one Library for the file: the operators' tables are built once per case; the longdouble side of the exact class's
    # premise is proved by tests/test_block_lanczos_reference_cpu.py, the assertion on the sums of every case runs here too)
    if not LIBRARY:
        LIBRARY.append(Library())
    return Checks(LIBRARY[0], prove=False)


@pytest.mark.parametrize("name,R", EXACT)
def test_the_first_step_on_exact_data_bit_for_bit(name, R):
    """k = 1: norm2, Q_0 in the Q array, alphas[0], betas[0], Q_1 in the W array and steps equal the fp64 reference in every bit;
    the W array is NaN on entry (the first step must not read the old block)"""
    checks().first_step(CASES[name], R)


@pytest.mark.parametrize("name,R", EXACT)
def test_break_decisions_bit_for_bit(name, R):
    """columns that break at s = 0, 1 and 2 beside live ones at k = 1 ... 4, a block in which
    every column breaks, the strict boundary of the rule with the scale in beta_0, in alpha_0 and in both, a NaN start column,
    and k = n + 2 at n = 2 and 3: steps, norm2, the whole alphas / betas arrays and both blocks"""
    c, case = checks(), CASES[name]
    c.breaks(case, R)
    c.all_break(case, R)
    c.strict(case, R)
    c.nan_column(case, R)
    if case.n <= 3:
        c.beyond_n(case, R)


@pytest.mark.parametrize("name,R", RANDOM)
def test_every_step_on_random_data(name, R):
    """runs of k = 1 ... 4 steps: the prefix rule, where Q_k and Q_{k-1} lie, Q_0 and every Q_{i+1} bit-equal to the mirror on
    the device's own mat-vec and scalars, norm2 / alpha_i / beta_{i+1}^2 within the sum bounds, the teeth of every judged step"""
    c = checks()
    assert c.random(CASES[name], R) <= 1.0
    print("%s R=%d worst error / bound: %s" % (name, R, "  ".join("%s %.4f (%s)" % (k, v[0], v[1].split(" ", 2)[2]) for k, v in c.worst.items())))


@pytest.mark.parametrize("name", ref.ALL)
def test_two_identical_calls_give_identical_bits(name):
    checks().twice(CASES[name], 8 if name in ref.THIN else 4)


def test_the_launch_geometry_the_cases_rely_on():
    """the grids the branch table names, on the Python copy of block_blocks and of sum_partials_block's trips, and the scratch
    size the library reports"""
    lib = checks().impl
    for name, blocks in (("L2-1", 1), ("L11-5", 2), ("L16-8", 51), ("L19-9", 361), ("L20-10-default", 722), ("L20-10-walk", 64),
                         ("L21-8", 795), ("L6-3-3-loops", 2), ("L8-4-4-complete", 20), ("L10-5-5-walk", 64), ("L10-5-5-default", 249)):
        case = CASES[name]
        assert case.nblk == blocks
        need = c_int64(-1)
        _lib.check(lib.entries(case)[0](8, byref(need)), "scratch_doubles")
        assert need.value == 64 + 16 * min(4096, case.ranges)
    assert ref.partial_trips(361) == (1, 105, 151) and ref.partial_trips(722) == (1, 256, 210) and ref.partial_trips(795) == (2, 27, 229)
    assert ref.partial_trips(249) == (0, 256, 249) and ref.partial_trips(257) == (1, 1, 255)
