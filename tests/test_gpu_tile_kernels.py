"""Every tile of the chain and lattice kernels and every width of the Ritz block kernel, one launch at a time through the C ABI
(docs/design/42-tile-and-width-instantiation-tests.md lists which case reaches which instantiation).

k_spmv_chain<T>, k_spmv_lattice<T> (csrc/dsea_chain.hip, csrc/dsea_lattice.hip): one dsea_spmv per call with shift, dot_out and
skip_flag passed explicitly, at T = 7 .. 12 on the whole vector (L = T), on eight tiles (L = T + 3) and, at T = 7, on 8192
tiles (L = 20).  EXACT inputs: y, y - shift x and x.y equal the reference bit for bit.  RANDOM inputs against np.longdouble:

    |y - ref|_row <= (m + 4) u (|H||x| + |shift x|)_row       |x.y - ref| <= (n + m + 4) u sum_row |x| (|H||x| + |shift x|)

with m counted from the kernel source (tests/tile_reference.py): k_spmv_chain rounds a coefficient and an FMA per off-diagonal
term (2 L terms), 2 L additions for the diagonal, one joining FMA and two operations for the shift, m = 6 L + 3;
k_spmv_lattice rounds a coefficient and an FMA per off-diagonal term (L + nb terms), nb + L additions for the diagonal, the
joining FMA and the shift, m = 3 (L + nb) + 3.  No constant is fitted to a device.  The skip call leaves sentinel-filled y
and scalar untouched; x and y sit in buffers with a NaN tail that must survive, and x must come back unchanged.

k_chain_forms<T>, k_lattice_forms<T>: dsea_op_chain_forms / dsea_op_lattice_forms at the same (L, T) with out and scratch 67
elements longer than asked for.  EXACT (v1, v2 integers in [-4, 4]): every form equals the longdouble reference bit for bit.
RANDOM: |form - ref| <= (n + 4) u sum |terms| (a form is a sum of n = 2^L once-rounded products through at most n - 1
additions: n rounded operations, so the factor two the products could claim is not used).  Two calls give identical bits;
the results at two tiles agree within the bound.

k_ritz_block<RPL, M>, k_ritz_block_split<W> (csrc/dsea_deflated.hip): dsea_ritz_combine_block for every m = 1 .. 8 in every
geometry of ``tile_reference.RITZ_*``: (a) column j equals dsea_ritz_combine with row j of S bit for bit; (b) the ritz
verdicts of tests/lanczos_reference.py -- exact class bit for bit against Reference(np.float64), random class within
(k + 17) u sum_j |s_j q_jk| (docs/design/29-lanczos-stage-tests.md)."""
from ctypes import byref, c_int64

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lanczos_reference as lref  # noqa: E402
import matvec_reference as ref  # noqa: E402
import tile_reference as tr  # noqa: E402
from test_gpu_cg_stages import Buf, dev, scalars  # noqa: E402
from test_gpu_lanczos_stages import Basis  # noqa: E402
from dominantsparseeigenad_amd import _lib  # noqa: E402
from dominantsparseeigenad_amd.engine import Workspace, _ptr, _stream  # noqa: E402
from dominantsparseeigenad_amd.operators import SpinChainOperator, SpinLatticeOperator  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402

F64 = torch.float64
LD = np.longdouble
SENTINEL = tr.SENTINEL
EXTRA = 67                      # elements behind what the forms calls are entitled to


def to_dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64)).to(dev())


# ---- the shapes are what the table says -------------------------------------------------------------------------------------
def test_the_cases_are_what_the_table_says():
    tr.assert_tile_cases()


# ---- mat-vec ----------------------------------------------------------------------------------------------------------------
def spmv_runner(handles, n):
    """``run`` of tile_reference.judge: one dsea_spmv on the handle of the class; x and y in NaN-tailed buffers"""
    lib = _lib.load()
    ws = Workspace.get(n, 8, dev())

    def run(cls, x, shift=None, dot=False, skip=False):
        xb, yb = Buf(x), Buf(np.full(n, SENTINEL))
        sh = scalars([shift]) if shift is not None else None
        d = scalars([SENTINEL]) if dot else None
        fl = scalars([1.0]) if skip else None
        _lib.check(lib.dsea_spmv(handles[cls], ws.handle, xb.ptr, yb.ptr, _ptr(sh), _ptr(d), _ptr(fl), _stream(dev())), "dsea_spmv")
        xb.kept("dsea_spmv x")
        if sh is not None:
            assert sh.item() == shift
        return yb.down("dsea_spmv y"), (d.item() if dot else None)

    return run


def chain_ops(L, kind, tune):
    ops = {}
    for cls in ("exact", "random"):
        op = SpinChainOperator(L, to_dev(tr.chain_couplings(L, kind, cls == "exact")))
        if tune is not None:
            op.set_tile_log2(tune)
        ops[cls] = op
    return ops


def lattice_ops(L, bonds, kind, tune):
    ops = {}
    for cls in ("exact", "random"):
        op = SpinLatticeOperator(L, bonds, to_dev(tr.lattice_couplings(L, bonds, kind, cls == "exact")))
        if tune is not None:
            op.set_tile_log2(tune)
        ops[cls] = op
    return ops


def judge_chain(L, tune, kind, random=True):
    case = tr.chain_case(L, kind, random)
    ops = chain_ops(L, kind, tune)
    tag = "chain L=%d T=%d %s" % (L, tr.tile_log2(L, tune), kind)
    return tr.judge(tag, case, spmv_runner({c: o.handle for c, o in ops.items()}, case.n))


def judge_lattice(L, tune, kind, random=True, cap=False):
    T = tr.tile_log2(L, tune)
    case = tr.lattice_case(L, T, kind, random, cap)
    ops = lattice_ops(L, case.bonds, kind, tune)
    tag = "lattice L=%d T=%d nb=%d %s" % (L, T, len(case.bonds), kind)
    return tr.judge(tag, case, spmv_runner({c: o.handle for c, o in ops.items()}, case.n))


@pytest.mark.parametrize("L,tune", tr.SHAPES)
def test_chain_matvec_every_tile(L, tune):
    worst = max(judge_chain(L, tune, kind) for kind in tr.CHAIN_KINDS)
    print("chain L=%d T=%d: worst error / bound %.3f" % (L, tr.tile_log2(L, tune), worst))


@pytest.mark.parametrize("L,tune", tr.SHAPES)
def test_lattice_matvec_every_tile(L, tune):
    worst = max(judge_lattice(L, tune, kind) for kind in tr.LATTICE_KINDS)
    print("lattice L=%d T=%d: worst error / bound %.3f" % (L, tr.tile_log2(L, tune), worst))


def test_lattice_matvec_full_bond_table_at_tile_9():
    print("worst error / bound %.3f" % judge_lattice(12, 9, "random", cap=True))


def test_lattice_whole_vector_at_tile_4():
    """k_spmv_lattice<4> and k_lattice_forms<4>: the one tile below 6 that tests/test_gpu_lattice.py has no case for"""
    assert tr.tile_log2(4) == 4 and 4 not in tr.lattice_tiles_of_the_older_suite()
    for kind in tr.LATTICE_KINDS:
        judge_lattice(4, None, kind)
    lattice_forms(4, None, 4)


def test_chain_matvec_blocks_walk_two_tiles_at_tile_7():
    judge_chain(*tr.WALK, "random", random=False)


def test_lattice_matvec_blocks_walk_two_tiles_at_tile_7():
    judge_lattice(*tr.WALK, "random", random=False)


# ---- forms ------------------------------------------------------------------------------------------------------------------
def forms_call(entry, sizer, sizes, handle, v1, v2, count):
    """one <stem>_forms call into sentinel-guarded out and scratch; twice, with identical bits"""
    lib = _lib.load()
    need = c_int64()
    _lib.check(getattr(lib, sizer)(*sizes, byref(need)), sizer)
    a, b = Buf(v1), Buf(v2)
    got = []
    for _ in range(2):
        out = torch.full((count + EXTRA,), SENTINEL, dtype=F64, device=dev())
        scratch = torch.full((need.value + EXTRA,), SENTINEL, dtype=F64, device=dev())
        _lib.check(getattr(lib, entry)(handle, a.ptr, b.ptr, _ptr(out), _ptr(scratch), _stream(dev())), entry)
        assert bool((out[count:] == SENTINEL).all()), "%s wrote behind its %d forms" % (entry, count)
        assert bool((scratch[need.value:] == SENTINEL).all()), "%s wrote behind its scratch" % entry
        got.append(out[:count].cpu().numpy())
    a.kept(entry + " v1")
    b.kept(entry + " v2")
    assert np.array_equal(got[0].view(np.int64), got[1].view(np.int64)), "%s: two calls differ" % entry
    return got[0]


def judge_forms(tag, case, call):
    """``call(v1, v2) -> forms``; returns (worst error / bound, the random-class forms)"""
    got = call(case.v1, case.v2)
    assert np.array_equal(got, case.want), "%s: %d forms differ on exact inputs" % (tag, int(np.sum(got != case.want)))
    if not case.random:
        print("%s: exact" % tag)
        return 0.0, None
    got = call(case.r1, case.r2)
    worst = ref.worst_ratio(np.abs(np.asarray(got, dtype=LD) - case.want_r), case.bound)
    print("%s: exact; random |form - ref| / bound = %.1e" % (tag, worst))
    assert worst <= 1.0, (tag, worst)
    return worst, got


def chain_forms(L, tune, random=True):
    case = tr.chain_forms_case(L, random)
    op = chain_ops(L, "random", tune)["random"]
    return judge_forms("chain forms L=%d T=%d" % (L, tr.tile_log2(L, tune)), case, lambda v1, v2: forms_call(
        "dsea_op_chain_forms", "dsea_op_chain_forms_scratch_doubles", (L,), op.handle, v1, v2, 5 * L))


def lattice_forms(L, tune, bonds_tile, random=True, cap=False):
    """``bonds_tile``: the tile the bond list was drawn for (the list stays when another tile is tuned in)"""
    case = tr.lattice_forms_case(L, bonds_tile, random, cap)
    bonds = case.bonds
    op = lattice_ops(L, bonds, "random", tune)["random"]
    return judge_forms("lattice forms L=%d T=%d nb=%d" % (L, tr.tile_log2(L, tune), len(bonds)), case, lambda v1, v2: forms_call(
        "dsea_op_lattice_forms", "dsea_op_lattice_forms_scratch_doubles", (L, len(bonds)), op.handle, v1, v2,
        3 * len(bonds) + 2 * L))


def tiles_of(L):
    """the tile tunings of the table at this L, and 2^6 (checked by tests/test_gpu_chain.py) to compare every one with"""
    return [tune for l, tune in tr.SHAPES if l == L] + [6]


def agree_across_tiles(tag, results, bound):
    for i, (ta, a) in enumerate(results):
        for tb, b in results[i + 1:]:
            worst = ref.worst_ratio(np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD)), bound)
            print("%s: tile %s against tile %s, |difference| / bound = %.1e" % (tag, ta, tb, worst))
            assert worst <= 1.0, (tag, ta, tb, worst)


@pytest.mark.parametrize("L", sorted({L for L, _ in tr.SHAPES}))
def test_chain_forms_every_tile(L):
    results = [(tune, chain_forms(L, tune)[1]) for tune in tiles_of(L)]
    agree_across_tiles("chain forms L=%d" % L, results, tr.chain_forms_case(L).bound)


@pytest.mark.parametrize("L", sorted({L for L, _ in tr.SHAPES}))
def test_lattice_forms_every_tile(L):
    tunes = tiles_of(L)
    T0 = tr.tile_log2(L, tunes[-2])                  # the bond list of the smallest tile of the table at this L
    results = [(tune, lattice_forms(L, tune, T0)[1]) for tune in tunes]
    agree_across_tiles("lattice forms L=%d" % L, results, tr.lattice_forms_case(L, T0).bound)


def test_lattice_forms_full_bond_table_at_tile_9():
    results = [(tune, lattice_forms(12, tune, 9, cap=True)[1]) for tune in (9, 12, 6)]
    agree_across_tiles("lattice forms L=12, full table", results, tr.lattice_forms_case(12, 9, cap=True).bound)


def test_chain_forms_blocks_walk_two_tiles_at_tile_7():
    chain_forms(*tr.WALK, random=False)


def test_lattice_forms_blocks_walk_two_tiles_at_tile_7():
    L, T = tr.WALK
    lattice_forms(L, T, T, random=False)


# ---- the Ritz block widths --------------------------------------------------------------------------------------------------
MAX_NEV = 8


def test_the_ritz_cases_reach_every_instantiation():
    tr.assert_ritz_cases()


def nan_bits_kept(got, before, keep, what):
    assert np.array_equal(got.view(np.int64)[keep], before.view(np.int64)[keep]), "%s: the call wrote outside its output" % what


def ritz_block(ws, Q, k, S8, ms, tag):
    """dsea_ritz_combine_block for every m of ``ms`` on rows [0, m) of S8, against dsea_ritz_combine row by row (verdict a);
    returns {m: Y[:m, :n]}"""
    lib, st = _lib.load(), _stream(dev())
    n = Q.shape[1]
    B = Basis(Q[:k], "even")
    single = []
    for j in range(max(ms)):
        sb, ob = scalars(S8[j]), Buf(np.full(n, SENTINEL))
        _lib.check(lib.dsea_ritz_combine(ws.handle, B.ptr, B.ld, n, k, _ptr(sb), ob.ptr, st), "dsea_ritz_combine")
        single.append(ob.down("dsea_ritz_combine out"))
    lds, ldy = k + 3, n + (n & 1) + 2
    out = {}
    for m in ms:
        S = np.full((MAX_NEV, lds), np.nan)
        S[:m, :k] = S8[:m]
        Y = np.full((MAX_NEV + 1, ldy), np.nan)
        Sd, Yd = torch.from_numpy(S).to(dev()), torch.from_numpy(Y).to(dev())
        _lib.check(lib.dsea_ritz_combine_block(ws.handle, B.ptr, B.ld, n, k, _ptr(Sd), lds, m, _ptr(Yd), ldy, st),
                   "dsea_ritz_combine_block")
        got = Yd.cpu().numpy()
        keep = np.ones(Y.shape, dtype=bool)
        keep[:m, :n] = False
        nan_bits_kept(got, Y, keep, "%s m=%d Y" % (tag, m))
        nan_bits_kept(Sd.cpu().numpy(), S, np.ones(S.shape, dtype=bool), "%s m=%d S" % (tag, m))
        assert np.isfinite(got[:m, :n]).all(), "%s m=%d: non-finite output (a read of the padding?)" % (tag, m)
        for j in range(m):
            assert np.array_equal(got[j, :n].view(np.int64), single[j].view(np.int64)), (
                "%s m=%d: column %d differs from dsea_ritz_combine in %d rows" % (tag, m, j, int(np.sum(got[j, :n] != single[j]))))
        out[m] = got[:m, :n].copy()
    B.kept("dsea_ritz_combine_block Q")
    return out


def judge_ritz_block(n, k, ms=tuple(range(1, 9)), rpl=0, split=-1):
    """both classes at one (n, k) in one geometry on a workspace of its own; returns the worst ratio of the random class"""
    ws = Workspace(n, 64, dev())
    tag = "ritz block n=%d k=%d rpl=%d split=%d" % (n, k, rpl, split)
    worst = 0.0
    try:
        ws.set_rows_per_lane(rpl)
        ws.set_split(split)
        Q = lref.exact_q(k, n, 131 + n + k)
        S8 = lref.halves(MAX_NEV * k, 132 + n + k).reshape(MAX_NEV, k)
        got = ritz_block(ws, Q, k, S8, ms, tag + " exact")
        want = [lref.assert_headroom("ritz", Q, k, S8[j]) for j in range(max(ms))]
        for m in ms:
            for j in range(m):
                assert np.array_equal(got[m][j], want[j]), "%s m=%d: column %d differs from the fp64 reference (exact class)" % (tag, m, j)
        Q = normal_vector(k * n, 133 + n + k).reshape(k, n) / np.sqrt(n)
        S8 = normal_vector(MAX_NEV * k, 134 + n + k).reshape(MAX_NEV, k)
        got = ritz_block(ws, Q, k, S8, ms, tag + " random")
        for j in range(max(ms)):                     # (column j has the same bits at every m >= j + 1: verdict a)
            res = lref.judge_ritz(Q, k, S8[j], got[max(ms)][j])
            assert res["out"] <= 1.0, (tag, j, res)
            worst = max(worst, res["out"])
    finally:
        ws.set_rows_per_lane(0)
        ws.set_split(-1)
    print("%s: exact class bit for bit; random class worst error / bound = %.3f" % (tag, worst))
    return worst


@pytest.mark.parametrize("n", sorted({n for n, _ in tr.RITZ_SPLIT16}))
def test_ritz_block_split_16(n):
    for _, k in (c for c in tr.RITZ_SPLIT16 if c[0] == n):
        judge_ritz_block(n, k)


def test_ritz_block_split_8():
    for n, k in tr.RITZ_SPLIT8:
        judge_ritz_block(n, k)


def test_ritz_block_split_4():
    for n, k in tr.RITZ_SPLIT4:
        judge_ritz_block(n, k, split=4)


@pytest.mark.parametrize("r", [2, 4, 8, 16])
def test_ritz_block_every_rows_per_lane_and_width(r):
    for _, n, k in (c for c in tr.RITZ_RPL if c[0] == r):
        judge_ritz_block(n, k, rpl=r)


def test_ritz_block_wave_owned_natural():
    n, k, ms = tr.RITZ_WAVE
    judge_ritz_block(n, k, ms=ms)
