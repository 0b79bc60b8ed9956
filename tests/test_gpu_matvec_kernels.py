"""The operator mat-vec kernels of csrc/dsea_spmv.hip one launch at a time, through dsea_spmv on the C ABI with shift, dot_out
and skip_flag passed explicitly, and their fused Lanczos tails through three steps of dsea_lanczos_run_basisfree -- every
tile, group, unroll, storage form and grid trip that launch_spmv / launch_sell / launch_tfim(_fused) can select
(docs/design/04-kernels.md lists which case reaches which instantiation).

Two input classes (tests/matvec_reference.py): EXACT inputs, where the kernel's y and x.y must equal the numpy reference bit
for bit whatever the summation order, and RANDOM normal inputs against np.longdouble with a bound that counts operations.
Every case also makes the skip_flag call into sentinel-filled outputs, which must come back untouched (include/dsea.h: "a
no-op on the device" -- y and *dot_out alike)."""
import functools
from ctypes import byref, c_int, c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import matvec_reference as ref  # noqa: E402
from dominantsparseeigenad_amd import _lib  # noqa: E402
from dominantsparseeigenad_amd.engine import Workspace, _ptr, _stream, round_up  # noqa: E402
from dominantsparseeigenad_amd.operators import CSROperator, _Handle  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402

F64 = torch.float64
LD = np.longdouble
SENTINEL = -7.0
SHIFT_EXACT, SHIFT_RANDOM = 0.375, 0.6180339887498949
G_EXACT, G_RANDOM = 0.875, 1.0690449676496976
COEF_EXACT, COEF_RANDOM = -1.625, -0.5 / 0.37 ** 2


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


def to_dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))                    # (a copy: cached case arrays are read-only)
    return (t if dtype is None else t.to(dtype)).to(dev())


def tune(handle, key, value, expect=0):
    rc = _lib.load().dsea_op_set_tuning(handle, key, value)
    assert rc == expect, (key, value, rc)


def spmv(handle, n, xd, shift=None, dot=False, skip=False):
    """one dsea_spmv; y and the scalar start as sentinels"""
    lib = _lib.load()
    ws = Workspace.get(n, 8, dev())
    y = torch.full((n,), SENTINEL, dtype=F64, device=dev())
    sh = torch.tensor([shift], dtype=F64, device=dev()) if shift is not None else None
    d = torch.full((1,), SENTINEL, dtype=F64, device=dev()) if dot else None
    fl = torch.ones(1, dtype=F64, device=dev()) if skip else None
    _lib.check(lib.dsea_spmv(handle, ws.handle, _ptr(xd), _ptr(y), _ptr(sh), _ptr(d), _ptr(fl), _stream(dev())), "dsea_spmv")
    return y.cpu().numpy(), (d.item() if dot else None)


class Case:
    """inputs and references of one operator, computed once: the exact class always, the random class unless the shape
    is one of the large ones (exact only)"""

    def __init__(self, n, m, apply_exact, apply_random, seed):
        self.n, self.m = n, m
        self.x = ref.exact_vector(n, seed)
        self.ax, sc = apply_exact(self.x, np.float64)
        ref.headroom(n, 4, float(sc.max()) + 4.0)
        self.shifted = self.ax - SHIFT_EXACT * self.x
        self.dot = float(np.sum(self.x * self.shifted))
        self.random = apply_random is not None
        if self.random:
            self.xr = normal_vector(n, seed + 1)
            self.want, self.scale = ref.shifted(apply_random, self.xr, SHIFT_RANDOM, LD)
            self.dot_r = np.sum(np.asarray(self.xr, dtype=LD) * self.want)
        for a in vars(self).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)


def judge(tag, case, handle_exact, handle_random=None):
    """the whole contract of dsea_spmv on one handle (per input class); returns the worst error / bound of the random class"""
    n = case.n
    xd = to_dev(case.x)
    y, _ = spmv(handle_exact, n, xd)
    assert np.array_equal(y, case.ax), "%s: y = A x on exact inputs, %d rows differ" % (tag, int(np.sum(y != case.ax)))
    y, d = spmv(handle_exact, n, xd, shift=SHIFT_EXACT, dot=True)
    assert np.array_equal(y, case.shifted), "%s: y = A x - shift x on exact inputs, %d rows differ" % (
        tag, int(np.sum(y != case.shifted)))
    assert d == case.dot, "%s: x.y on exact inputs %r, want %r" % (tag, d, case.dot)
    y, d = spmv(handle_exact, n, xd, shift=SHIFT_EXACT, dot=True, skip=True)
    assert bool((y == SENTINEL).all()) and d == SENTINEL, "%s: the skip flag did not make the call a no-op" % tag
    y, d = spmv(handle_exact, n, xd, skip=True)
    assert bool((y == SENTINEL).all())
    if not case.random:
        print("%s: exact" % tag)
        return 0.0
    xr = to_dev(case.xr)
    y, d = spmv(handle_random if handle_random is not None else handle_exact, n, xr, shift=SHIFT_RANDOM, dot=True)
    ry = ref.worst_ratio(np.abs(np.asarray(y, dtype=LD) - case.want), ref.matvec_bound(case.m, case.scale))
    rd = ref.worst_ratio(abs(LD(d) - case.dot_r), ref.dot_bound(n, case.m, case.xr, case.scale))
    print("%s: exact; random  |y - ref| / bound = %.3f   |x.y - ref| / bound = %.3f" % (tag, ry, rd))
    assert ry <= 1.0 and rd <= 1.0, (tag, ry, rd)
    return max(ry, rd)


# ====================================================================================================== TFIM, plain
def tfim_handle(L, L_local, offset, g, diag_scale, g_on_device, tile=None):
    raw = c_void_p()
    gd = torch.tensor([g], dtype=F64, device=dev()) if g_on_device else None
    _lib.check(_lib.load().dsea_op_create_tfim(L, L_local, offset, _ptr(gd), 0.0 if g_on_device else g, diag_scale, byref(raw)),
               "dsea_op_create_tfim")
    h = _Handle(raw, 1 << L_local, gd)
    if tile is not None:
        tune(raw, _lib.TUNE_TFIM_TILE_LOG2, tile)
    return h


# variant -> (g exact, g random, diag_scale, g through the device pointer)
TFIM_VARIANTS = {"g-dev": (G_EXACT, G_RANDOM, 1.0, True), "g-const": (G_EXACT, G_RANDOM, 1.0, False),
                 "dH/dg": (1.0, 1.0, 0.0, False)}


@functools.lru_cache(maxsize=12)
def tfim_case(L, L_local, offset, variant, random=True):
    ge, gr, ds, _ = TFIM_VARIANTS[variant]
    return Case(1 << L_local, L + 1, ref.tfim_apply(L, L_local, offset, ge, ds),
                ref.tfim_apply(L, L_local, offset, gr, ds) if random else None, 100 * L + L_local)


def judge_tfim(L, L_local, offset, variant, tile, random=True):
    ge, gr, ds, on_dev = TFIM_VARIANTS[variant]
    case = tfim_case(L, L_local, offset, variant, random)
    he = tfim_handle(L, L_local, offset, ge, ds, on_dev, tile)
    hr = tfim_handle(L, L_local, offset, gr, ds, on_dev, tile) if random else None
    return judge("tfim L=%d L_local=%d offset=%#x %s tile=%s" % (L, L_local, offset, variant, tile), case, he.raw,
                 hr.raw if hr else None)


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5])
def test_tfim_below_the_smallest_tile(L):
    """T = L_local < 6: the tile is the whole vector"""
    for variant in TFIM_VARIANTS:
        judge_tfim(L, L, 0, variant, None)


def test_tfim_single_row_slab():
    """L_local = 0: k_spmv_tfim_single"""
    for offset in (0, 5, 6):
        for variant in TFIM_VARIANTS:
            judge_tfim(3, 0, offset, variant, None)


@pytest.mark.parametrize("tile", [6, 7, 8, 9, 10, 11, 12])
def test_tfim_every_tile(tile):
    """L = T (one tile, no far bit), T + 1 (one far bit, two tiles) and 14, for every instantiation T = 6..12"""
    worst = 0.0
    for L in sorted({tile, tile + 1, 14}):
        for variant in TFIM_VARIANTS:
            worst = max(worst, judge_tfim(L, L, 0, variant, tile))
    print("tile 2^%d: worst error / bound %.3f" % (tile, worst))


@pytest.mark.parametrize("L,ntiles", [(18, 4096), (19, 8192)])
def test_tfim_blocks_walk_several_tiles(L, ntiles):
    """T = 6: exactly DSEA_MAX_TFIM_BLOCKS tiles, then two tiles per block"""
    assert (1 << L) >> 6 == ntiles and (ntiles > ref.MAX_TFIM_BLOCKS) == (L == 19)
    judge_tfim(L, L, 0, "g-dev", 6)


@pytest.mark.parametrize("L,tile", [(21, 6), (21, 11), (23, 6), (23, 11), (24, 6), (24, 11), (24, 12)])
def test_tfim_far_bit_loops(L, tile):
    """far bits beyond the T + FB requested up front (T + FB = 20 at T = 6 and 11, 21 at T = 12): L = 21 and 23 run the
    one-bit tail loop only, L = 24 the four-bit trip at T = 6 (PER = 1) and T = 11 (PER = 4) and three tail bits at T = 12.
    Exact inputs only: the reference is L XOR-gathers of an integer-valued array."""
    judge_tfim(L, L, 0, "g-dev", tile, random=False)


@pytest.mark.parametrize("rank", [0, 1, 2, 3])
def test_tfim_slab_every_rank(rank):
    for variant in ("g-dev", "dH/dg"):
        judge_tfim(10, 8, rank << 8, variant, None)


SLAB_OFFSETS = {33: [(1 << 32) | (0x15A5A5 << 9), (1 << 32) | (0x0A5A5A << 9) | (1 << 31), 0x1F0F0F << 9],
                62: [(1 << 61) | (0x5A5A5A5A5A5A5 << 9), (1 << 61) | (1 << 60) | (1 << 9), (1 << 60) | (0x2A5A5A5A5A5A5 << 9)]}


@pytest.mark.parametrize("L", [33, 62])
def test_tfim_slab_of_a_long_chain(L):
    """row offsets with the top bits set: the wrap bond of the diagonal (bit L-1 against bit 0, which alternates along the
    slab) and the 64-bit rotate / mask of tfim_diag, against the header's d(gi) in Python integers"""
    for offset in SLAB_OFFSETS[L]:
        assert offset % 512 == 0 and offset >> L == 0
        judge_tfim(L, 9, offset, "g-dev", None)
    assert (SLAB_OFFSETS[L][0] >> (L - 1)) & 1 == 1 and (SLAB_OFFSETS[L][2] >> (L - 1)) & 1 == 0


def test_tfim_creator_limits():
    lib, raw = _lib.load(), c_void_p()
    assert lib.dsea_op_create_tfim(63, 9, 0, None, 1.0, 1.0, byref(raw)) == _lib.ERR_ARG
    assert lib.dsea_op_create_tfim(10, 8, 128, None, 1.0, 1.0, byref(raw)) == _lib.ERR_ARG       # slab not aligned
    assert lib.dsea_op_create_tfim(10, 11, 0, None, 1.0, 1.0, byref(raw)) == _lib.ERR_ARG


# ====================================================================================================== CSR
def csr_operator(name, exact):
    rowptr, cols, n, _ = ref.csr_case(name)
    vals = ref.csr_values(int(rowptr[-1]), 31, exact)
    return CSROperator(to_dev(rowptr), to_dev(cols), to_dev(vals), n, layout="csr"), vals


@functools.lru_cache(maxsize=4)
def csr_reference(name, random=True):
    rowptr, cols, n, m = ref.csr_case(name)
    nnz = int(rowptr[-1])
    return Case(n, m, ref.csr_apply(rowptr, cols, ref.csr_values(nnz, 31, True)),
                ref.csr_apply(rowptr, cols, ref.csr_values(nnz, 31, False)) if random else None, 7 + n)


def judge_csr(name, groups):
    case = csr_reference(name)
    ope, _ = csr_operator(name, True)
    opr, _ = csr_operator(name, False)
    worst = 0.0
    for G in groups:
        for op in (ope, opr):
            tune(op.handle, _lib.TUNE_CSR_GROUP, G)
        worst = max(worst, judge("csr %s G=%d" % (name, G), case, ope.handle, opr.handle))
    return worst


@pytest.mark.parametrize("name", ["avg6-1", "avg6-129", "avg6-1037", "avg2-129", "avg2-1037", "avg60-129"])
def test_csr_every_group(name):
    """automatic (streaming kernel at an average of 6, k_spmv_csr<4> below 4, k_spmv_csr<64> above 48) and every forced G;
    empty rows include the first and the last"""
    rowptr = ref.csr_case(name)[0]
    assert ref.csr_takes_stream(rowptr, 0) == name.startswith("avg6-")
    if not name.endswith("-1"):
        assert rowptr[1] == 0 and rowptr[-1] == rowptr[-2]
    print("worst error / bound %.3f" % judge_csr(name, (0, 4, 8, 16, 32, 64)))


def test_csr_group_kernel_grid_stride():
    rowptr, _, n, _ = ref.csr_case("group-stride")
    assert n > ref.MAX_EW_BLOCKS * (256 // 64)
    judge_csr("group-stride", (64,))


def test_csr_stream_several_chunks_per_block():
    rowptr, _, n, _ = ref.csr_case("stream-trips")
    assert ref.csr_takes_stream(rowptr, 0) and (n + ref.CSR_ROWS - 1) // ref.CSR_ROWS > ref.MAX_TFIM_BLOCKS
    judge_csr("stream-trips", (0,))


def test_csr_stream_long_row_fallback():
    rowptr, _, n, _ = ref.csr_case("long-rows")
    sizes = ref.csr_chunk_sizes(rowptr)
    assert ref.csr_takes_stream(rowptr, 0) and sizes[1] > ref.CSR_CAP and (np.delete(sizes, 1) <= ref.CSR_CAP).all()
    judge_csr("long-rows", (0,))


def test_csr_tuning_refuses_other_groups():
    op, _ = csr_operator("avg6-129", True)
    for G in (1, 2, 3, 12, 128):
        tune(op.handle, _lib.TUNE_CSR_GROUP, G, expect=_lib.ERR_ARG)


# ====================================================================================================== SELL
FORMS = {"sell32": dict(col16=False, values="plain", pad=1), "sell16": dict(col16=True, values="plain", pad=1),
         "sell16p2": dict(col16=True, values="plain", pad=2), "sell16v8": dict(col16=True, values="coded", pad=4)}


def sell_operator(monkeypatch, form, rowptr, cols, vals, n):
    for name in ("DSEA_SELL_NT", "DSEA_SELL_VALUES", "DSEA_SELL_PACK2"):
        monkeypatch.delenv(name, raising=False)
    if form == "sell16":
        monkeypatch.setenv("DSEA_SELL_PACK2", "0")
    f = FORMS[form]
    op = CSROperator(to_dev(rowptr), to_dev(cols), to_dev(vals), n, layout="sell", col16=f["col16"], values=f["values"])
    assert op.col16 == (form != "sell32") and op._coded == (form == "sell16v8")
    assert op._coded or op._pack2 == (form == "sell16p2")
    got = np.diff(op._sell[0].cpu().numpy()) // 64
    assert np.array_equal(got, ref.sell_slice_widths(rowptr, n, f["pad"])), "the slice widths of the device layout"
    return op


def sell_tunings(form):
    """[(label, [(key, value), ...])]: every kernel instantiation the storage form can select, each at both slice maps"""
    out = []
    for xcd in (0, 1):
        if form == "sell32":
            for un in (1, 2, 4, 8):
                out.append(("unroll=%d xcd=%d" % (un, xcd), [(_lib.TUNE_SELL_UNROLL, un), (_lib.TUNE_SELL_XCD_MAP, xcd)]))
        elif form == "sell16":
            for nt in (0, 1):
                out.append(("nt=%d xcd=%d" % (nt, xcd), [(_lib.TUNE_SELL_NT, nt), (_lib.TUNE_SELL_XCD_MAP, xcd)]))
        else:
            out.append(("xcd=%d" % xcd, [(_lib.TUNE_SELL_XCD_MAP, xcd)]))
    return out


@functools.lru_cache(maxsize=4)
def sell_reference(nslices):
    rowptr, cols, n, m = ref.sell_case(nslices)
    nnz = int(rowptr[-1])
    return Case(n, m, ref.csr_apply(rowptr, cols, ref.csr_values(nnz, 41, True)),
                ref.csr_apply(rowptr, cols, ref.csr_values(nnz, 41, False)), 3 + nslices)


def check_sell_geometry(nslices):
    rowptr, cols, n, m = ref.sell_case(nslices)
    assert (n + 63) // 64 == nslices and n % 64 != 0
    assert list(ref.sell_slice_widths(rowptr, n)) == ref.sell_widths(nslices)
    if 30 < nslices < 1000:
        assert set(ref.sell_widths(nslices)) == set(ref.WIDTHS)


@pytest.mark.parametrize("nslices", [1, 5, 37, 129, 4 * ref.MAX_TFIM_BLOCKS + 5])
@pytest.mark.parametrize("form", list(FORMS))
def test_sell_every_form_and_tuning(monkeypatch, form, nslices):
    """ragged slices (widths 0, 1, 3, 8, 9, 63, 64, 65, 130; n no multiple of 64) at slice counts where the XCD map sends
    most lanes out of range (1, 5, 37), a full grid (129) and a second trip of the grid (16389: small widths)"""
    check_sell_geometry(nslices)
    rowptr, cols, n, _ = ref.sell_case(nslices)
    nnz = int(rowptr[-1])
    case = sell_reference(nslices)
    ope = sell_operator(monkeypatch, form, rowptr, cols, ref.csr_values(nnz, 41, True), n)
    opr = sell_operator(monkeypatch, form, rowptr, cols, ref.csr_values(nnz, 41, False), n)
    if form in ("sell16p2", "sell16v8"):
        tune(ope.handle, _lib.TUNE_SELL_NT, 1, expect=_lib.ERR_UNSUPPORTED)
        tune(ope.handle, _lib.TUNE_SELL_NT, 0)
    worst = 0.0
    for label, keys in sell_tunings(form):
        for op in (ope, opr):
            for key, value in keys:
                tune(op.handle, key, value)
        worst = max(worst, judge("%s %d slices %s" % (form, nslices, label), case, ope.handle, opr.handle))
    print("worst error / bound %.3f" % worst)


@pytest.mark.parametrize("lo,hi", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("hb", [3, "n"])
@pytest.mark.parametrize("form", ["sell32", "sell16", "sell16p2"])
def test_sell_slab_with_halos(monkeypatch, form, hb, lo, hi):
    """mode 1: c < 0 reads halo_lo[c + hb], c >= n reads halo_hi[c - n]; a missing neighbour's pointer is null"""
    nslices = 37
    n = ref.sell_case(nslices)[2]
    hb = n if hb == "n" else hb
    rowptr, cols, n, m = ref.slab_pattern(nslices, hb, lo, hi)
    nnz = int(rowptr[-1])
    halos = {True: (ref.exact_vector(hb, 61), ref.exact_vector(hb, 62)), False: (normal_vector(hb, 63), normal_vector(hb, 64))}

    def gather(exact):
        hl, hh = halos[exact]
        nan = np.full(hb, np.nan)
        return lambda x, c: np.concatenate((hl if lo else nan, x, hh if hi else nan))[c.astype(np.int64) + hb]

    case = Case(n, m, ref.csr_apply(rowptr, cols, ref.csr_values(nnz, 43, True), gather(True)),
                ref.csr_apply(rowptr, cols, ref.csr_values(nnz, 43, False), gather(False)), 11 + hb)
    ops, keep = [], []
    for exact in (True, False):
        op = sell_operator(monkeypatch, form, rowptr, cols, ref.csr_values(nnz, 43, exact), n)
        hl, hh = (to_dev(h) for h in halos[exact])
        keep += [hl, hh]
        assert _lib.load().dsea_op_set_slab(op.handle, hb, _ptr(hl if lo else None), _ptr(hh if hi else None), None) == 0
        ops.append(op)
    print("worst error / bound %.3f" % judge("%s slab hb=%d lo=%s hi=%s" % (form, hb, lo, hi), case, ops[0].handle, ops[1].handle))


@pytest.mark.parametrize("form", ["sell32", "sell16", "sell16p2"])
def test_sell_slab_gathered(monkeypatch, form):
    """mode 2: GLOBAL columns, x[col] read from x_gathered (three slabs, this one in the middle)"""
    nslices = 37
    rowptr, _, n, m = ref.sell_case(nslices)
    nnz = int(rowptr[-1])
    cols = np.random.default_rng(71).integers(0, 3 * n, size=nnz).astype(np.int32)
    assert cols.min() < n and cols.max() >= 2 * n
    others = {True: (ref.exact_vector(n, 72), ref.exact_vector(n, 73)), False: (normal_vector(n, 74), normal_vector(n, 75))}

    def gather(exact):
        return lambda x, c: np.concatenate((others[exact][0], x, others[exact][1]))[c]

    case = Case(n, m, ref.csr_apply(rowptr, cols, ref.csr_values(nnz, 44, True), gather(True)),
                ref.csr_apply(rowptr, cols, ref.csr_values(nnz, 44, False), gather(False)), 13)
    ops, keep = [], []
    for exact, x in ((True, case.x), (False, case.xr)):
        op = sell_operator(monkeypatch, form, rowptr, cols, ref.csr_values(nnz, 44, exact), n)
        xg = to_dev(np.concatenate((others[exact][0], x, others[exact][1])))
        keep.append(xg)
        assert _lib.load().dsea_op_set_slab(op.handle, -1, None, None, _ptr(xg)) == 0
        ops.append(op)
    print("worst error / bound %.3f" % judge("%s slab gathered" % form, case, ops[0].handle, ops[1].handle))


def test_sell_value_coded_operand_takes_no_slab(monkeypatch):
    rowptr, cols, n, _ = ref.sell_case(5)
    op = sell_operator(monkeypatch, "sell16v8", rowptr, cols, ref.csr_values(int(rowptr[-1]), 41, True), n)
    buf = torch.zeros(3 * n, dtype=F64, device=dev())
    lib = _lib.load()
    assert lib.dsea_op_set_slab(op.handle, 3, _ptr(buf), _ptr(buf), None) == _lib.ERR_UNSUPPORTED
    assert lib.dsea_op_set_slab(op.handle, -1, None, None, _ptr(buf)) == _lib.ERR_UNSUPPORTED


# ====================================================================================================== stencil
def stencil_handle(n, coef, V, lo, hi):
    raw = c_void_p()
    Vd = to_dev(V)
    lod = torch.tensor([lo], dtype=F64, device=dev()) if lo is not None else None
    hid = torch.tensor([hi], dtype=F64, device=dev()) if hi is not None else None
    _lib.check(_lib.load().dsea_op_create_stencil3(n, coef, _ptr(Vd), _ptr(lod), _ptr(hid), byref(raw)), "dsea_op_create_stencil3")
    return _Handle(raw, n, (Vd, lod, hid))


@pytest.mark.parametrize("halos", ["none", "both", "lo", "hi"])
@pytest.mark.parametrize("n", [1, 2, 3, 511, 512, 513, 1025, (1 << 21) + 3])
def test_stencil(n, halos):
    """pairs, the odd last row, one tile per block up to 4096 tiles and the grid-stride form beyond (2^21 + 3 rows)"""
    lo, hi = halos in ("both", "lo"), halos in ("both", "hi")
    Ve, Vr = ref.eighths(n, 81), normal_vector(n, 82)
    he = stencil_handle(n, COEF_EXACT, Ve, 3.0 if lo else None, -2.0 if hi else None)
    hr = stencil_handle(n, COEF_RANDOM, Vr, 0.7315 if lo else None, -1.4142 if hi else None)
    case = Case(n, 4, ref.stencil_apply(COEF_EXACT, Ve, 3.0 if lo else None, -2.0 if hi else None),
                ref.stencil_apply(COEF_RANDOM, Vr, 0.7315 if lo else None, -1.4142 if hi else None), 5 + n)
    print("worst error / bound %.3f" % judge("stencil n=%d halos=%s" % (n, halos), case, he.raw, hr.raw))


# ====================================================================================================== symmetric dense
def symdense_handle(store, n, lda, elem):
    A = to_dev(store, torch.float32 if elem == 4 else F64)
    lib = _lib.load()
    work = torch.full((lib.dsea_op_symdense_work_bytes(n) // 8,), np.nan, dtype=F64, device=dev())
    raw = c_void_p()
    _lib.check(lib.dsea_op_create_symdense(n, _ptr(A), elem, lda, _ptr(work), byref(raw)), "dsea_op_create_symdense")
    return _Handle(raw, n, (A, work))


@pytest.mark.parametrize("pad", [0, 6])
@pytest.mark.parametrize("elem", [8, 4])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 1000])
def test_symdense(n, elem, pad):
    """fp64 and fp32 elements, ragged n, lda = n and n + 6 (n odd: n + 1 and n + 7, rows are read as element pairs), 16 block
    rows at n = 1000 (both loops of k_symv_reduce).  The lower triangle and the padding columns hold NaN, and so does the
    scratch: no NaN may reach y (the lower triangle is never used, every partial slot is written before it is read)."""
    lda = n + (n & 1) + pad
    assert n != 1000 or (n + 63) // 64 >= 13
    se, Se = ref.symdense_storage(n, lda, 91, True)
    sr, Sr = ref.symdense_storage(n, lda, 92, False)
    assert np.array_equal(Se.astype(np.float32).astype(np.float64), Se) and np.array_equal(Sr.astype(np.float32).astype(np.float64), Sr)
    case = Case(n, n, ref.dense_apply(Se), ref.dense_apply(Sr), 9 + n)
    he, hr = symdense_handle(se, n, lda, elem), symdense_handle(sr, n, lda, elem)
    print("worst error / bound %.3f" % judge("symdense n=%d elem=%d lda=%d" % (n, elem, lda), case, he.raw, hr.raw))
    lib, raw = _lib.load(), c_void_p()
    A = torch.zeros((n, lda + 1), dtype=F64, device=dev())
    assert lib.dsea_op_create_symdense(n, _ptr(A), 8, lda + 1, _ptr(A), byref(raw)) != 0           # odd lda
    assert lib.dsea_op_create_symdense(n, _ptr(A), 8, n - 1, _ptr(A), byref(raw)) == _lib.ERR_ARG  # lda < n


# ====================================================================================================== fused tails
def lanczos3(handle, n, q0):
    """three steps of the basis-free run: plain mat-vec, then the fused tail twice.  Returns (status, break step, Q[3, n],
    alphas[3], betas[2]); every output starts as a sentinel."""
    lib = _lib.load()
    ws = Workspace.get(n, 8, dev())
    before = ws.lanczos_persist_mode
    ws.set_lanczos_persist(0)
    try:
        ldq = round_up(n, 32)
        Q = torch.full((3, ldq), SENTINEL, dtype=F64, device=dev())
        alphas = torch.full((3,), SENTINEL, dtype=F64, device=dev())
        betas = torch.full((2,), SENTINEL, dtype=F64, device=dev())
        qd = to_dev(q0)
        _lib.check(lib.dsea_lanczos_run_basisfree(handle, ws.handle, 3, _ptr(qd), _ptr(Q), ldq, _ptr(alphas), _ptr(betas),
                                                  None, None, _stream(dev())), "dsea_lanczos_run_basisfree")
        step = c_int(0)
        rc = lib.dsea_lanczos_status(ws.handle, byref(step), _stream(dev()))
    finally:
        ws.set_lanczos_persist(before)
    assert bool((Q[:, n:] == SENTINEL).all())
    return rc, step.value, Q[:, :n].cpu().numpy(), alphas.cpu().numpy(), betas.cpu().numpy()


def judge_fused(tag, handle, n, m, apply, seed):
    """the Lanczos relations on the device's own outputs, and the same bits from a second run"""
    q0 = normal_vector(n, seed)
    rc, step, Q, a, b = lanczos3(handle, n, q0)
    assert rc == 0 and step == 0, (tag, rc, step)
    ratios = ref.lanczos_relations(apply, m, q0, Q, a, b)
    worst = max(ratios.values())
    print("%s: %s" % (tag, "  ".join("%s %.3f" % kv for kv in ratios.items())))
    assert worst <= 1.0, (tag, ratios)
    rc2, _, Q2, a2, b2 = lanczos3(handle, n, q0)
    assert rc2 == 0 and np.array_equal(Q, Q2) and np.array_equal(a, a2) and np.array_equal(b, b2), "%s: not deterministic" % tag
    return worst


def judge_breakdown(tag, handle, n, eigenvalue):
    """q0 = the all-ones eigenvector, exact inputs, n a power of 4: r = 0 exactly -> breakdown at step 1, nothing later written"""
    rc, step, Q, a, b = lanczos3(handle, n, np.ones(n))
    assert (rc, step) == (_lib.ERR_BREAKDOWN, 1), (tag, rc, step)
    assert np.array_equal(Q[0], np.full(n, 1.0 / np.sqrt(n))) and a[0] == eigenvalue, tag
    assert (Q[1:] == SENTINEL).all() and (a[1:] == SENTINEL).all() and b[1] == SENTINEL, tag
    assert b[0] == 0.0, tag


FUSED_TFIM = [(14, t) for t in range(6, 13)] + [(19, 11), (19, 12), (20, 11), (20, 12), (22, 11), (23, 11), (19, 6)]


@pytest.mark.parametrize("L,tile", FUSED_TFIM)
def test_fused_tfim(L, tile):
    """k_spmv_tfim<T, true>: every tile at L = 14; T + FB = 18 at T = 11 and 19 at T = 12, so L = 19 / 20 run the one-bit tail
    loop (T = 12, L = 19: no remaining bit), L = 22 the four-bit trip, L = 23 trip and tail; L = 19 at T = 6: 8192 tiles"""
    h = tfim_handle(L, L, 0, G_RANDOM, 1.0, True, tile)
    judge_fused("fused tfim L=%d tile=%d" % (L, tile), h.raw, 1 << L, L + 1, ref.tfim_apply(L, L, 0, G_RANDOM, 1.0), 300 + L)


def test_fused_tfim_slab_and_single_row():
    """a slab (L_local < L) is an operator on its own rows and has the tail; the single-row form has none"""
    h = tfim_handle(10, 8, 3 << 8, G_RANDOM, 1.0, True)
    judge_fused("fused tfim slab", h.raw, 256, 11, ref.tfim_apply(10, 8, 3 << 8, G_RANDOM, 1.0), 333)
    h0 = tfim_handle(3, 0, 5, G_RANDOM, 1.0, True)
    ws = Workspace.get(1, 8, dev())
    buf = torch.zeros(96, dtype=F64, device=dev())
    rc = _lib.load().dsea_lanczos_run_basisfree(h0.raw, ws.handle, 3, _ptr(buf), _ptr(buf[32:]), 32, _ptr(buf[8:]), _ptr(buf[16:]),
                                                None, None, _stream(dev()))
    assert rc == _lib.ERR_UNSUPPORTED


@pytest.mark.parametrize("nslices", [37, 129])
@pytest.mark.parametrize("form", list(FORMS))
def test_fused_sell(monkeypatch, form, nslices):
    """k_spmv_sell<true, 0, ...> and k_spmv_sell_r5<true>: every storage form and tuning on the ragged slices"""
    rowptr, cols, n, m = ref.sell_case(nslices)
    vals = ref.csr_values(int(rowptr[-1]), 41, False)
    op = sell_operator(monkeypatch, form, rowptr, cols, vals, n)
    apply = ref.csr_apply(rowptr, cols, vals)
    worst = 0.0
    for label, keys in sell_tunings(form):
        for key, value in keys:
            tune(op.handle, key, value)
        worst = max(worst, judge_fused("fused %s %d slices %s" % (form, nslices, label), op.handle, n, m, apply, 400 + nslices))
    print("worst error / bound %.3f" % worst)


@pytest.mark.parametrize("n", [513, 1025, (1 << 21) + 3])
def test_fused_stencil(n):
    V = normal_vector(n, 82)
    h = stencil_handle(n, COEF_RANDOM, V, None, None)
    judge_fused("fused stencil n=%d" % n, h.raw, n, 4, ref.stencil_apply(COEF_RANDOM, V), 500)


def test_breakdown_tfim():
    """dH/dg: A 1 = -L 1"""
    h = tfim_handle(12, 12, 0, 1.0, 0.0, False)
    judge_breakdown("tfim", h.raw, 1 << 12, -12.0)


@pytest.mark.parametrize("unroll", [0, 1])
def test_breakdown_sell(monkeypatch, unroll):
    """integer values with constant row sums 5 (k_spmv_sell and the round-5 kernel)"""
    n = 4096
    rowptr, cols = ref.csr_pattern(np.random.default_rng(5).integers(1, 10, size=n), 6, band=300)
    vals = ref.constant_row_sum_values(rowptr, 5.0, 7)
    op = sell_operator(monkeypatch, "sell32", rowptr, cols, vals, n)
    tune(op.handle, _lib.TUNE_SELL_UNROLL, unroll)
    judge_breakdown("sell unroll=%d" % unroll, op.handle, n, 5.0)


def test_breakdown_stencil():
    """V = c inside, c + coef at the two ends: A 1 = c 1"""
    n, c = 1024, 2.5
    V = np.full(n, c)
    V[[0, -1]] = c + COEF_EXACT
    h = stencil_handle(n, COEF_EXACT, V, None, None)
    judge_breakdown("stencil", h.raw, n, c)
