"""The symmetric Lanczos step kernels one library call at a time (docs/design/29-lanczos-stage-tests.md): dsea_lanczos_rdots,
dsea_lanczos_axpy_norm, dsea_ritz_combine, dsea_lanczos_store / dsea_scale_store, dsea_lanczos_callable_alpha,
dsea_lanczos_callable_step and dsea_lanczos_partial_step, each on prepared inputs with everything downloaded and judged by
tests/lanczos_reference.py -- EXACT inputs bit for bit (every output vector and scalar, the partial re-orthogonalisation's
anorm, counter and every decision), RANDOM inputs against np.longdouble with bounds that count operations.
tests/test_lanczos_reference_cpu.py shows without a GPU that the same ``Checks`` reject wrong kernels.

Every vector lives at the start of a buffer two elements longer than n whose tail is NaN; the basis is a (rows + 1, ldq) buffer
with NaN in columns n .. ldq - 1 and one NaN row behind the last row the call may touch, for ldq = n + (n & 1) and for the Python
layer's round_up(n, 32).  After every call the tails and the padding must be unchanged bit for bit, the n rows finite, read-only
operands unchanged, and c_out / alphas / betas must hold their sentinels wherever the call must not write.  Every case runs on
a workspace of its own (no shadow, no geometry override, no partial re-orthogonalisation left behind by another test)."""
import contextlib
from ctypes import byref, c_double, c_int64, c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lanczos_reference as ref  # noqa: E402
from lanczos_reference import SENTINEL, Checks  # noqa: E402
from test_gpu_cg_stages import Buf, dev, scalars  # noqa: E402
from dominantsparseeigenad_amd import _lib  # noqa: E402
from dominantsparseeigenad_amd.engine import Workspace, _ptr, _stream  # noqa: E402

F64 = torch.float64
ERR_ARG, ERR_ALIGN, ERR_WORKSPACE = -1, -2, -3
KMAX_DEFAULT = 16


class Basis:
    """``rows`` basis vectors in a (rows + 1, ldq) device buffer: NaN beyond column n and in the row behind the last"""

    def __init__(self, Q, layout):
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        self.rows, self.n = Q.shape
        self.ld = self.n + (self.n & 1) if layout == "even" else (self.n + 31) // 32 * 32
        self.host = np.full((self.rows + 1, self.ld), np.nan)
        self.host[:self.rows, :self.n] = Q
        self.t = torch.from_numpy(self.host).to(dev())

    @property
    def ptr(self):
        return _ptr(self.t)

    def row_ptr(self, j):
        return c_void_p(self.t.data_ptr() + 8 * j * self.ld)

    def down(self, what):
        got = self.t.cpu().numpy()
        pad = np.ones(got.shape, dtype=bool)
        pad[:self.rows, :self.n] = False
        assert np.array_equal(got.view(np.int64)[pad], self.host.view(np.int64)[pad]), "%s: the call wrote outside the basis rows" % what
        assert np.isfinite(got[:self.rows, :self.n]).all(), "%s: non-finite basis rows (a read past row n - 1?)" % what
        return got[:self.rows, :self.n].copy()

    def kept(self, what):
        assert ref.same(self.down(what), self.host[:self.rows, :self.n]), "%s: the basis was modified" % what


def unchanged(t, host, what):
    assert ref.same(t.cpu().numpy(), np.asarray(host, dtype=np.float64).reshape(-1)), "%s was modified" % what


class Library:
    """the interface lanczos_reference.Checks drives, one library call per method (callable_step: the alpha call first)"""

    layouts = ("even", "pad32")

    def __init__(self):
        self.lib = _lib.load()
        self.cfg = dict(rpl=0, split=-1, kmax=None)
        self.spaces = {}

    def st(self):
        return _stream(dev())

    def ws(self, n):
        """a workspace of this Library alone (Workspace.get caches and other tests leave settings behind): created without a
        shadow; the geometry knobs are set on every use and cleared by ``setup``'s exit"""
        if n not in self.spaces:
            self.spaces[n] = Workspace(n, self.cfg["kmax"] or KMAX_DEFAULT, dev())
        w = self.spaces[n]
        _lib.check(self.lib.dsea_ws_set_shadow(w.handle, c_void_p(None), 0, 0, 0.0), "dsea_ws_set_shadow")
        _lib.check(self.lib.dsea_ws_set_shadow8(w.handle, c_void_p(None), 0, 0, 0.0), "dsea_ws_set_shadow8")
        w.set_rows_per_lane(self.cfg["rpl"])
        w.set_split(self.cfg["split"])
        return w.handle

    @contextlib.contextmanager
    def setup(self, rpl=0, split=-1, kmax=None):
        old = dict(self.cfg)
        self.cfg = dict(rpl=rpl, split=split, kmax=kmax)
        if kmax is not None:
            self.spaces = {}
        try:
            yield
        finally:
            for w in self.spaces.values():
                w.set_rows_per_lane(0)
                w.set_split(-1)
                _lib.check(self.lib.dsea_ws_set_partial_reorth(w.handle, 0, 0.0), "dsea_ws_set_partial_reorth")
            if kmax is not None:                    # (half a gigabyte of partial sums at kmax = 8000: released at once)
                self.spaces = {}
                torch.cuda.empty_cache()
            self.cfg = old

    # -- phases
    def rdots(self, Q, i, u, a, b, ld="even"):
        n = u.size
        B, ub, rb = Basis(Q[:i], ld), Buf(u), Buf(np.full(n, SENTINEL))
        al, be = scalars([a]), (scalars([b]) if b is not None else None)
        c = scalars([SENTINEL] * (i + 3))
        _lib.check(self.lib.dsea_lanczos_rdots(self.ws(n), B.ptr, B.ld, n, i, ub.ptr, _ptr(al), _ptr(be), rb.ptr, _ptr(c), self.st()),
                   "dsea_lanczos_rdots")
        B.kept("dsea_lanczos_rdots Q")
        ub.kept("dsea_lanczos_rdots u")
        unchanged(al, [a], "dsea_lanczos_rdots alpha")
        if b is not None:
            unchanged(be, [b], "dsea_lanczos_rdots beta")
        ch = c.cpu().numpy()
        assert (ch[i + 1:] == SENTINEL).all(), "dsea_lanczos_rdots wrote more than i + 1 coefficients"
        return rb.down("dsea_lanczos_rdots r"), ch[:i + 1].copy()

    def axpy_norm(self, Q, i, c, r, ld="even"):
        n = r.size
        B, rb, cb = Basis(Q[:i], ld), Buf(r), scalars(c)
        out = scalars([SENTINEL, SENTINEL])
        _lib.check(self.lib.dsea_lanczos_axpy_norm(self.ws(n), B.ptr, B.ld, n, i, _ptr(cb), rb.ptr, _ptr(out), self.st()),
                   "dsea_lanczos_axpy_norm")
        B.kept("dsea_lanczos_axpy_norm Q")
        unchanged(cb, c, "dsea_lanczos_axpy_norm c")
        oh = out.cpu().numpy()
        assert oh[1] == SENTINEL, "dsea_lanczos_axpy_norm wrote behind nrm2_out"
        return rb.down("dsea_lanczos_axpy_norm r"), float(oh[0])

    def ritz(self, Q, k, s, ld="even"):
        n = Q.shape[1]
        B, sb, ob = Basis(Q[:k], ld), scalars(s), Buf(np.full(n, SENTINEL))
        _lib.check(self.lib.dsea_ritz_combine(self.ws(n), B.ptr, B.ld, n, k, _ptr(sb), ob.ptr, self.st()), "dsea_ritz_combine")
        B.kept("dsea_ritz_combine Q")
        unchanged(sb, s, "dsea_ritz_combine s")
        return ob.down("dsea_ritz_combine out")

    def store_row(self, r, nrm2, Q, row, with_beta=True, ld="even"):
        n = r.size
        B, rb, nb = Basis(Q, ld), Buf(r), scalars([nrm2])
        bo = scalars([SENTINEL, SENTINEL]) if with_beta else None
        _lib.check(self.lib.dsea_lanczos_store(self.ws(n), rb.ptr, _ptr(nb), B.ptr, B.ld, row, _ptr(bo), n, self.st()), "dsea_lanczos_store")
        rb.kept("dsea_lanczos_store r")
        unchanged(nb, [nrm2], "dsea_lanczos_store nrm2")
        if not with_beta:
            return B.down("dsea_lanczos_store Q"), None
        bh = bo.cpu().numpy()
        assert bh[1] == SENTINEL, "dsea_lanczos_store wrote behind beta_out"
        return B.down("dsea_lanczos_store Q"), float(bh[0])

    def scale_store(self, r, nrm2, with_beta=True):
        n = r.size
        rb, qb, nb = Buf(r), Buf(np.full(n, SENTINEL)), scalars([nrm2])
        bo = scalars([SENTINEL, SENTINEL]) if with_beta else None
        _lib.check(self.lib.dsea_scale_store(self.ws(n), rb.ptr, _ptr(nb), qb.ptr, _ptr(bo), n, self.st()), "dsea_scale_store")
        rb.kept("dsea_scale_store r")
        unchanged(nb, [nrm2], "dsea_scale_store nrm2")
        if not with_beta:
            return qb.down("dsea_scale_store q"), None
        bh = bo.cpu().numpy()
        assert bh[1] == SENTINEL, "dsea_scale_store wrote behind beta_out"
        return qb.down("dsea_scale_store q"), float(bh[0])

    def callable_alpha(self, q, u, with_out=True):
        n = q.size
        qb, ub = Buf(q), Buf(u)
        out = scalars([SENTINEL, SENTINEL]) if with_out else None
        _lib.check(self.lib.dsea_lanczos_callable_alpha(self.ws(n), qb.ptr, ub.ptr, n, _ptr(out), self.st()), "dsea_lanczos_callable_alpha")
        qb.kept("dsea_lanczos_callable_alpha q")
        ub.kept("dsea_lanczos_callable_alpha u")
        if not with_out:
            torch.cuda.synchronize()
            return None
        oh = out.cpu().numpy()
        assert oh[1] == SENTINEL, "dsea_lanczos_callable_alpha wrote behind alpha_out"
        return float(oh[0])

    def callable_step(self, Q, i, u, alphas, betas, ld="even"):
        n = u.size
        B, ub, rb = Basis(Q[:i + 1], ld), Buf(u), Buf(np.full(n, SENTINEL))
        al, be = scalars(alphas), scalars(betas)
        ws = self.ws(n)
        _lib.check(self.lib.dsea_lanczos_callable_alpha(ws, B.row_ptr(i - 1), ub.ptr, n, c_void_p(None), self.st()),
                   "dsea_lanczos_callable_alpha")
        _lib.check(self.lib.dsea_lanczos_callable_step(ws, B.ptr, B.ld, n, i, ub.ptr, _ptr(al), _ptr(be), rb.ptr, self.st()),
                   "dsea_lanczos_callable_step")
        ub.kept("dsea_lanczos_callable_step u")
        Qn = np.array(Q, dtype=np.float64)
        Qn[:i + 1] = B.down("dsea_lanczos_callable_step Q")
        return Qn, al.cpu().numpy(), be.cpu().numpy(), rb.down("dsea_lanczos_callable_step r")

    @contextlib.contextmanager
    def partial(self, n, delta):
        lib, ws, st = self.lib, self.ws(n), self.st()
        _lib.check(lib.dsea_ws_set_partial_reorth(ws, 1, float(delta)), "dsea_ws_set_partial_reorth")

        class Session:
            def step(self, Q, i, u, alphas, betas):
                B, ub, rb = Basis(Q[:i], "pad32" if i & 1 else "even"), Buf(u), Buf(np.full(n, SENTINEL))
                al, be, out = scalars(alphas), scalars(betas), scalars([SENTINEL, SENTINEL])
                _lib.check(lib.dsea_lanczos_partial_step(ws, B.ptr, B.ld, n, i, ub.ptr, _ptr(al), _ptr(be), rb.ptr, _ptr(out), st),
                           "dsea_lanczos_partial_step")
                count, anorm = c_int64(-1), c_double(-1.0)
                _lib.check(lib.dsea_lanczos_reorth_stats(ws, byref(count), byref(anorm), st), "dsea_lanczos_reorth_stats")
                B.kept("dsea_lanczos_partial_step Q")
                ub.kept("dsea_lanczos_partial_step u")
                unchanged(al, alphas, "dsea_lanczos_partial_step alphas")
                unchanged(be, betas, "dsea_lanczos_partial_step betas")
                oh = out.cpu().numpy()
                assert oh[1] == SENTINEL, "dsea_lanczos_partial_step wrote behind nrm2_out"
                return rb.down("dsea_lanczos_partial_step r"), float(oh[0]), float(anorm.value), float(count.value)
        try:
            yield Session()
        finally:
            _lib.check(lib.dsea_ws_set_partial_reorth(ws, 0, 0.0), "dsea_ws_set_partial_reorth")


def checks():
    # (the longdouble side of the exact class's headroom is proved by tests/test_lanczos_reference_cpu.py; the assertion on the
    # sums of every case runs here as well)
    return Checks(Library(), prove=False)


# ------------------------------------------------------------------------------------------------ split form
@pytest.mark.parametrize("n", ref.SIZES_SPLIT16)
def test_every_stage_in_the_split_16_form(n):
    """one tile with guarded loads (n = 1, 2, 3, 127), several tiles with an odd last row (129, 4097): every stage, every step
    parity with and without remainder vectors, i = 1 with beta null and non-null, one and several alpha partials, the partial
    re-orthogonalisation selected / skipped / forced / restarted, and every call twice"""
    assert checks().small(n) <= 1.0


@pytest.mark.parametrize("stage", ["rdots", "axpy_norm", "callable_step"])
def test_the_split_8_form(stage):
    assert getattr(checks(), stage)(ref.SIZE_SPLIT8, steps=(1, 2, 5)) <= 1.0


@pytest.mark.parametrize("n", ref.SIZES_NT2)
@pytest.mark.parametrize("stage", ["rdots", "callable_step"])
def test_two_sub_tiles_per_block_of_the_dots_pass(stage, n):
    """642 tiles: the last block's second sub-tile holds one row; 643 tiles: it is empty"""
    assert getattr(checks(), stage)(n, steps=(1, 2, 5)) <= 1.0


@pytest.mark.parametrize("n", ref.SIZES_FINALIZE)
def test_the_four_accumulator_trips_of_the_second_stage(n):
    """set_split(16) keeps one partial per 128-row tile: 801 (one four-accumulator trip of k_finalize_multi, then the tail) and
    1801 (two trips for the first threads)"""
    assert checks().rdots(n, steps=(3,), split=16) <= 1.0


# ------------------------------------------------------------------------------------------------ wave-owned form
@pytest.mark.parametrize("n", ref.SIZES_WAVE)
@pytest.mark.parametrize("stage", ["rdots", "axpy_norm", "callable_step", "ritz"])
def test_the_wave_owned_form(stage, n):
    """rows per lane 2 / 4 / 8 / 16 as Workspace::geom selects them: the exact class at i <= 5 (all step parities at 131202
    rows) and one random case per stage"""
    steps = {"rdots": ref.STEPS_REV if n == ref.SIZES_WAVE[0] else (1, 2, 5), "axpy_norm": (2, 5), "callable_step": (1, 2, 5), "ritz": (5,)}
    assert getattr(checks(), stage)(n, steps=steps[stage]) <= 1.0


def test_the_wave_owned_form_stores():
    c = checks()
    assert c.store(ref.SIZES_WAVE[0]) <= 1.0 and c.callable_alpha(ref.SIZES_WAVE[0]) <= 1.0


@pytest.mark.parametrize("n", (ref.SIZE_SPLIT8, ref.SIZES_NT2[0]) + ref.SIZES_WAVE)
def test_two_identical_calls_give_identical_outputs(n):
    """rdots, axpy_norm and the fused step twice on the same inputs, bit for bit: one size per geometry (the split-16 sizes and
    the forced two rows per lane repeat their calls inside their own tests)"""
    checks().twice(n)


def test_alpha_from_more_than_64_partials():
    """131203 rows: 65 partials of q.u (sum_partials_wave's two-accumulator trip), an odd last row in the wave-owned form"""
    assert checks().callable_step(ref.SIZES_WAVE[0] + 1, steps=(2, 3)) <= 1.0


@pytest.mark.parametrize("n", ref.SIZES_RPL2_SMALL)
def test_a_block_whose_last_waves_own_no_tile(n):
    """set_rows_per_lane(2) at 129 / 300 rows: two / three wave tiles in one block of four waves (the idle waves add zeros)"""
    c = checks()
    assert c.rdots(n, rpl=2) <= 1.0
    c.partial_exact(n, rpl=2)
    assert c.partial_random(n, rpl=2) <= 1.0
    c.twice(n, rpl=2)


@pytest.mark.parametrize("stage", ["rdots", "axpy_norm"])
def test_the_grid_stride_trip(stage):
    """set_rows_per_lane(2) at 2^20 + 129 rows: 8194 tiles on 8192 waves -- two waves take a second tile (``accumulate``), the
    second of them a one-row tile"""
    assert getattr(checks(), stage)(ref.SIZE_GRID_STRIDE, steps=(5,), rpl=2) <= 1.0


def test_partial_reorthogonalisation_in_the_wave_owned_form():
    c = checks()
    c.partial_exact(ref.SIZES_WAVE[0])
    assert c.partial_random(ref.SIZES_WAVE[0]) <= 1.0


def test_partial_reorthogonalisation_boundary_is_strict():
    checks().partial_strict()


# ------------------------------------------------------------------------------------------------ waves per block, LDS edges
@pytest.mark.parametrize("i", ref.STEPS_LDS)
def test_waves_per_block_of_the_dots_pass_and_the_lds_edges(i):
    """set_rows_per_lane(2) at 300 rows, kmax 8000: four waves per block up to i = 2047 (exactly 64 KiB of LDS), two up to 4095
    (64 KiB again), one beyond (64 000 bytes at i = 7999); exact class, the correction pass over the same i vectors too"""
    assert ref.rdots_lds_bytes(300, i, rpl=2) == {2047: 65536, 2048: 2 * 2049 * 8, 4095: 65536, 4096: 4097 * 8, 7999: 64000}[i]
    c = checks()
    c.rdots(300, steps=(i,), random=False, rpl=2, kmax=ref.KMAX)
    c.axpy_norm(300, steps=(i,), random=False, rpl=2, kmax=ref.KMAX)


@pytest.mark.parametrize("i", ref.STEPS_LDS_SPLIT)
def test_long_recurrences_in_the_split_form(i):
    c = checks()
    c.rdots(129, steps=(i,), random=False, kmax=ref.KMAX)
    c.axpy_norm(129, steps=(i,), random=False, kmax=ref.KMAX)


# ------------------------------------------------------------------------------------------------ a chain
def test_callable_step_chain():
    assert checks().callable_chain() <= 1.0


# ------------------------------------------------------------------------------------------------ return codes
def test_return_codes():
    """refused on the host, before any launch: i = 0, a null required pointer and ldq < n are DSEA_ERR_ARG; i > kmax is
    DSEA_ERR_WORKSPACE; an odd ldq or a pointer at an odd element is DSEA_ERR_ALIGN; dsea_lanczos_callable_step without a
    preceding dsea_lanczos_callable_alpha is DSEA_ERR_ARG.  Every output keeps its sentinel."""
    lib = _lib.load()
    n, i, kmax = 16, 2, 8
    space = Workspace(n, kmax, dev())
    ws, st = space.handle, _stream(dev())
    pool = torch.full((8 * (n + 2),), SENTINEL, dtype=F64, device=dev())
    v = [pool[k * (n + 2):k * (n + 2) + n] for k in range(4)]
    odd = pool[1:1 + n]
    assert odd.data_ptr() % 16 == 8
    Q = torch.full((kmax + 2, n), SENTINEL, dtype=F64, device=dev())
    sc = torch.full((16,), SENTINEL, dtype=F64, device=dev())
    null, p = c_void_p(None), _ptr
    S = p(sc)
    # (function, arguments, positions of the 16-byte-aligned pointers, of the required pointers, of ldq, of i)
    table = [
        ("dsea_lanczos_rdots", [ws, p(Q), n, n, i, p(v[0]), S, S, p(v[1]), S, st], (1, 5, 8), (0, 1, 5, 6, 8, 9), 2, 4),
        ("dsea_lanczos_axpy_norm", [ws, p(Q), n, n, i, S, p(v[1]), S, st], (1, 6), (0, 1, 5, 6, 7), 2, 4),
        ("dsea_lanczos_partial_step", [ws, p(Q), n, n, i, p(v[0]), S, S, p(v[1]), S, st], (1, 5, 8), (0, 1, 5, 6, 7, 8, 9), 2, 4),
        ("dsea_lanczos_store", [ws, p(v[0]), S, p(Q), n, 1, S, n, st], (1, 3), (0, 1, 2, 3), 4, None),
        ("dsea_scale_store", [ws, p(v[0]), S, p(v[1]), S, n, st], (1, 3), (1, 2, 3), None, None),
        ("dsea_lanczos_callable_alpha", [ws, p(v[0]), p(v[1]), n, S, st], (1, 2), (0, 1, 2), None, None),
        ("dsea_lanczos_callable_step", [ws, p(Q), n, n, i, p(v[0]), S, S, p(v[1]), st], (1, 5, 8), (0, 1, 5, 6, 7, 8), 2, 4),
        ("dsea_ritz_combine", [ws, p(Q), n, n, i, S, p(v[1]), st], (1, 6), (0, 1, 5, 6), 2, 4),
    ]
    for name, args, aligned, required, ld_at, i_at in table:
        fn = getattr(lib, name)
        for k in aligned:
            bad = list(args)
            bad[k] = p(odd)
            assert fn(*bad) == ERR_ALIGN, (name, "odd pointer at", k)
        for k in required:
            bad = list(args)
            bad[k] = null
            assert fn(*bad) == ERR_ARG, (name, "null pointer at", k)
        if ld_at is not None:
            bad = list(args)
            bad[ld_at] = n + 1
            assert fn(*bad) == ERR_ALIGN, (name, "odd ldq")
            bad[ld_at] = n - 2
            assert fn(*bad) == ERR_ARG, (name, "ldq < n")
        if i_at is not None:
            bad = list(args)
            bad[i_at] = 0
            assert fn(*bad) == ERR_ARG, (name, "i = 0")
            if name not in ("dsea_lanczos_axpy_norm", "dsea_ritz_combine"):      # (these two keep nothing per vector in the workspace)
                bad[i_at] = kmax + 1
                assert fn(*bad) == ERR_WORKSPACE, (name, "i > kmax")
    # the fused step needs the alpha partials of a dsea_lanczos_callable_alpha on the same workspace: none were left (every
    # call above was refused), and a completed step consumes them
    step = table[6][1]
    assert lib.dsea_lanczos_callable_step(*step) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((pool == SENTINEL).all()) and bool((Q == SENTINEL).all()) and bool((sc == SENTINEL).all()), "a refused call reached the device"
