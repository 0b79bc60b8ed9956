"""The non-symmetric side one library call at a time: the Arnoldi step scalars and the GMRES cycle of csrc/dsea_krylov.hip
through dsea_arnoldi_orth / dsea_arnoldi_extend / dsea_gmres_begin / step / end / cycle on the C ABI (ctypes), every output
sentinel-filled first.  tests/krylov_reference.py holds the plain longdouble reference, the two input classes (EXACT: bit
equality whatever the summation order; RANDOM: operation-counted bounds) and the derivations;
docs/design/17-krylov-stage-tests.md lists which case reaches which kernel branch."""
import ctypes
import functools
from ctypes import byref, c_int, c_int64

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import krylov_reference as kr  # noqa: E402
import matvec_reference as mref  # noqa: E402
from dominantsparseeigenad_amd import _lib, krylov  # noqa: E402
from dominantsparseeigenad_amd.engine import Workspace, _ptr, _stream, round_up  # noqa: E402
from dominantsparseeigenad_amd.operators import DenseOperator, Stencil3Operator  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402

F64 = torch.float64
LD = np.longdouble
SENTINEL = -7.0
ERR_ALIGN, ERR_WORKSPACE = -2, -3


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


def st():
    return _stream(dev())


def to_dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64)).to(dev())


def sentinels(*shape):
    return torch.full(shape, SENTINEL, dtype=F64, device=dev())


def scalar(v):
    return None if v is None else torch.tensor([v], dtype=F64, device=dev())


def second_passes(ws):
    cnt = c_int64(-1)
    _lib.check(_lib.load().dsea_arnoldi_second_passes(ws.handle, byref(cnt), st()))
    return cnt.value


def statuses(ws):
    """(rc, break_step) of dsea_lanczos_status and of dsea_arnoldi_status"""
    lib, a, b, r = _lib.load(), c_int(-5), c_int(-5), c_int(-5)
    rc1 = lib.dsea_lanczos_status(ws.handle, byref(a), st())
    rc2 = lib.dsea_arnoldi_status(ws.handle, byref(b), byref(r), st())
    return (rc1, a.value), (rc2, b.value), r.value


# ====================================================================================== one step, dsea_arnoldi_orth
def orth_step(n, j, Vrows, u, shift, kmax=None):
    """one dsea_arnoldi_orth on hand-made rows; V has j + 3 rows of ldv = round_up(n, 32) + 32 doubles and H j + 3 columns of
    ldh = j + 4, all sentinels except V[0..j][:n].  Returns a dict of what came back and what must not have changed."""
    lib = _lib.load()
    ws = Workspace.get(n, max(kmax or 0, j + 3), dev())
    ldv, ldh = round_up(n, 32) + 32, j + 4
    V = sentinels(j + 3, ldv)
    V[: j + 1, :n] = to_dev(Vrows)
    H = sentinels(j + 3, ldh)
    V0 = V.clone()
    ud, sh = to_dev(u), scalar(shift)
    if j > 0:
        _lib.check(lib.dsea_arnoldi_clear_record(ws.handle, st()))
    before = second_passes(ws) if j > 0 else 0
    _lib.check(lib.dsea_arnoldi_orth(ws.handle, _ptr(ud), _ptr(sh), _ptr(V), ldv, n, j, _ptr(H), ldh, st()), "dsea_arnoldi_orth")
    out = {"count": second_passes(ws) - before, "status": statuses(ws)}
    torch.cuda.synchronize()
    assert torch.equal(V[: j + 1], V0[: j + 1]), "V[0..j] changed"
    assert bool((V[j + 1, n:] == SENTINEL).all()), "the padding of row j + 1 was written"
    assert bool((V[j + 2] == SENTINEL).all()), "a row beyond j + 1 was written"
    assert bool((H[:j] == SENTINEL).all()) and bool((H[j + 1:] == SENTINEL).all()), "another column of H was written"
    assert bool((H[j, j + 2:] == SENTINEL).all()), "hcol beyond j + 1 was written"
    out["h"] = H[j, : j + 2].cpu().numpy()
    out["v"] = V[j + 1, :n].cpu().numpy()
    assert np.isfinite(out["h"]).all() and np.isfinite(out["v"]).all()
    # a following step j + 1: a no-op after a breakdown (checked by the caller through these)
    out["again"] = lambda: _follow(ws, ud, sh, V, ldv, n, j + 1, H, ldh)
    return out


def _follow(ws, ud, sh, V, ldv, n, j, H, ldh):
    Vb, Hb, before = V.clone(), H.clone(), second_passes(ws)
    _lib.check(_lib.load().dsea_arnoldi_orth(ws.handle, _ptr(ud), _ptr(sh), _ptr(V), ldv, n, j, _ptr(H), ldh, st()))
    torch.cuda.synchronize()
    return torch.equal(V, Vb) and torch.equal(H, Hb) and second_passes(ws) == before


def check_dead(tag, n, j, got, ref):
    (rc1, b1), (rc2, b2), redo = got["status"]
    assert rc1 == _lib.ERR_BREAKDOWN and rc2 == _lib.ERR_BREAKDOWN and b1 == b2 == j + 1 and redo == -1, (tag, got["status"])
    assert got["h"][j + 1] <= kr.BREAK_TOL * float(np.sqrt(ref.ww)), (tag, got["h"][j + 1])
    assert bool((got["v"] == SENTINEL).all()), "%s: V[j + 1] written by a dead step" % tag
    assert got["again"](), "%s: the step after a breakdown was not a no-op" % tag


def check_alive(tag, got):
    assert got["status"] == ((0, 0), (0, 0), -1), (tag, got["status"])


def exact_cases(n):
    if n == kr.N_CAPPED:          # 134 MB per row block: one case per branch (exactness of every kind is shown at the other sizes)
        yield from ((0, "plain"), (1, "second"), (2, "overlap"), (2, "zero"))
        return
    for j in kr.step_js(n):
        for kind in kr.exact_kinds(n, j):
            yield j, kind


@pytest.mark.parametrize("n", kr.STEP_N + (kr.N_CAPPED,))
def test_arnoldi_orth_exact_class(n):
    """bit equality with the reference for every exact kind, shifted and unshifted; the exactly-zero case u = shift v_j"""
    ran = 0
    for j, kind in exact_cases(n):
        V, u, shift, p = kr.exact_step(n, j, kind)
        for sh in ((shift,) if n == kr.N_CAPPED and kind != "plain" else (shift, None)):
            if kind == "zero" and sh is None:
                u_ = np.zeros(n)                                     # (u = 0 v_j)
            else:
                u_ = u
            # (fp64 = longdouble on this class, shown by tests/test_krylov_reference_cpu.py: the large sizes skip the conversion)
            ref = kr.arnoldi_step(V, u_, sh or 0.0, LD if n <= 131202 else np.float64)
            tag = "exact n=%d j=%d %s shift=%s" % (n, j, kind, sh)
            got = orth_step(n, j, V, u_, sh)
            assert got["count"] == int(ref.second), (tag, got["count"], ref.second)
            want_h = np.asarray(ref.h, dtype=np.float64)
            assert np.array_equal(got["h"], want_h), (tag, got["h"], want_h)
            if kind == "zero":
                assert not got["h"].any() and got["count"] == 0, tag
            if ref.dead:
                check_dead(tag, n, j, got, ref)
            else:
                check_alive(tag, got)
                assert np.array_equal(got["v"], np.asarray(ref.v_next, dtype=np.float64)), \
                    "%s: %d rows of v_next differ" % (tag, int(np.sum(got["v"] != np.asarray(ref.v_next, dtype=np.float64))))
            ran += 1
    print("n = %d: %d exact steps, all bit-equal" % (n, ran))
    assert ran >= 4


def random_cases(n):
    for j in kr.step_js(n):
        for kind in kr.random_kinds(n, j):
            yield j, kind
    if n == 129:
        for kind in kr.random_kinds(n, kr.J_LONG):
            yield kr.J_LONG, kind


@pytest.mark.parametrize("n", kr.STEP_N)
def test_arnoldi_orth_random_class(n):
    """the operation-counted bounds of krylov_reference.step_bounds on hcol and V[j + 1], decisions equal to the reference's"""
    worst = {}
    for j, kind in random_cases(n):
        for with_shift in ((True,) if j == kr.J_LONG else (False, True)):
            V, u, shift, ref = kr.random_step(n, j, kind, with_shift)
            tag = "random n=%d j=%d %s shift=%s" % (n, j, kind, with_shift)
            got = orth_step(n, j, V, u, shift if with_shift else None, kmax=j + 2 if j == kr.J_LONG else None)
            assert got["count"] == int(ref.second), (tag, got["count"], ref.second)
            if ref.dead:
                check_dead(tag, n, j, got, ref)
                ratios = {"h": kr.worst_ratio(np.abs(np.asarray(got["h"], dtype=LD) - ref.h),
                                              kr.step_bounds(V, u, shift, ref)["h"])}
            else:
                check_alive(tag, got)
                ratios = kr.judge_step(V, u, shift, ref, got["h"], got["v"])
            for fam, r in ratios.items():
                key = "%s/%s" % (kind, fam)
                worst[key] = max(worst.get(key, 0.0), r)
                assert r <= 1.0, (tag, fam, r)
    for key in sorted(worst):
        print("n = %d  %-14s worst error / bound = %.4f" % (n, key, worst[key]))
    assert worst


def test_second_pass_counter_is_cleared_by_every_start():
    """include/dsea.h dsea_arnoldi_second_passes: cleared by dsea_arnoldi_orth(j = 0) and dsea_gmres_begin as by
    dsea_arnoldi_extend(j0 = 0); grows by one per step that ran the pass"""
    n = 129
    V, u, shift, _ = kr.exact_step(n, 2, "second")
    ws = Workspace.get(n, 5, dev())
    a = orth_step(n, 2, V, u, shift)
    b = orth_step(n, 2, V, u, shift)
    assert a["count"] == b["count"] == 1 and second_passes(ws) >= 2
    V0, u0, s0, _ = kr.exact_step(n, 0, "plain")
    assert orth_step(n, 0, V0, u0, s0)["count"] == 0 and second_passes(ws) == 0
    orth_step(n, 2, V, u, shift)
    assert second_passes(ws) == 1
    g = GmresRun(n, 1, dense=kr.dense_noise(n), ws=ws)
    g.begin(normal_vector(n, 3), None, 0.0)
    assert second_passes(ws) == 0


# ====================================================================================== native steps, dsea_arnoldi_extend
class Native:
    """an operand, its reference apply, and dsea_arnoldi_extend into sentinel-filled buffers"""

    def __init__(self, kind, n):
        self.n = n
        if kind == "dense":
            A = kr.dense_noise(n, seed=20 + n % 7)
            self.op, self.apply, self.m = DenseOperator(to_dev(A)), mref.dense_apply(A), n
        else:
            pot = normal_vector(n, 8)
            self.op = Stencil3Operator(n, 0.37, to_dev(pot))
            self.apply, self.m = mref.stencil_apply(self.op.coef, pot), 4
        self.ldv = round_up(n, 32) + 32
        self.ws = Workspace.get(n, 10, dev())

    def buffers(self, rows, start):
        V = sentinels(rows, self.ldv)
        V[: start.shape[0], : self.n] = to_dev(start)
        return V, sentinels(rows - 1, rows)

    def extend(self, V, H, j0, j1, shift=None, optimistic=False):
        lib = _lib.load()
        sh = scalar(shift)
        _lib.check(lib.dsea_ws_set_arnoldi_optimistic(self.ws.handle, 1 if optimistic else 0))
        try:
            _lib.check(lib.dsea_arnoldi_extend(self.op.handle, self.ws.handle, _ptr(sh), _ptr(V), self.ldv, j0, j1, _ptr(H),
                                               H.shape[1], st()), "dsea_arnoldi_extend")
        finally:
            _lib.check(lib.dsea_ws_set_arnoldi_optimistic(self.ws.handle, 0))
        torch.cuda.synchronize()


def unit(v):
    v = np.asarray(v, dtype=LD)
    return np.asarray(v / np.sqrt(np.sum(v * v)), dtype=np.float64)


@pytest.mark.parametrize("kind,n", [("dense", 129), ("dense", 1001), ("stencil3", 131202)])
def test_arnoldi_extend_native(kind, n):
    nat = Native(kind, n)
    v0 = unit(normal_vector(n, 9))[None, :]
    for shift in (None, kr.SHIFT_RANDOM):
        V, H = nat.buffers(6, v0)
        nat.extend(V, H, 0, 4, shift)
        assert statuses(nat.ws) == ((0, 0), (0, 0), -1)
        Vh, Hh = V[:, :n].cpu().numpy(), H.cpu().numpy()
        assert bool((V[5] == SENTINEL).all()) and bool((V[:5, n:] == SENTINEL).all()) and bool((H[4:] == SENTINEL).all())
        for j in range(4):
            assert (Hh[j, j + 2:] == SENTINEL).all()
        r = kr.relation_ratio(nat.apply, nat.m, shift or 0.0, Vh, Hh, 0, 4)
        print("extend %s n=%d shift=%s: " % (kind, n, shift) + "  ".join("%s %.4f" % kv for kv in sorted(r.items())))
        assert max(r.values()) <= 1.0, r
        # 0 -> 2 -> 4 is 0 -> 4
        V2, H2 = nat.buffers(6, v0)
        nat.extend(V2, H2, 0, 2, shift)
        nat.extend(V2, H2, 2, 4, shift)
        assert torch.equal(V2, V) and torch.equal(H2, H)
    # a non-Hessenberg start block: p = 3 arbitrary orthonormal rows, then columns 3 and 4 in full
    start = kr.random_rows(n, 4, seed=9)
    V, H = nat.buffers(7, start)
    lib = _lib.load()
    _lib.check(lib.dsea_arnoldi_clear_record(nat.ws.handle, st()))
    nat.extend(V, H, 3, 5, kr.SHIFT_RANDOM)
    Vh, Hh = V[:, :n].cpu().numpy(), H.cpu().numpy()
    assert (Hh[:3] == SENTINEL).all() and (Hh[5:] == SENTINEL).all() and (Hh[3, 5:] == SENTINEL).all() and (Hh[4, 6:] == SENTINEL).all()
    assert np.array_equal(Vh[:4], start) and bool((V[6] == SENTINEL).all())
    r = kr.relation_ratio(nat.apply, nat.m, kr.SHIFT_RANDOM, Vh, Hh, 3, 5)
    print("extend %s n=%d from a start block of 4 rows: " % (kind, n) + "  ".join("%s %.4f" % kv for kv in sorted(r.items())))
    assert max(r.values()) <= 1.0, r


# ====================================================================================== Arnoldi breakdown, native operand
def test_arnoldi_breakdown_native_three_eigenvalues():
    n = 129
    # eigenvalues (-2, 0, 2), start vector with weights (0.05, 0.9, 0.05) on the eigenspaces: steps 0 and 1 pass the DGKS test
    # (a random start fails it at step 0 already: A v0 is mostly v0), step 2 finds the space exhausted
    A, v0 = kr.three_eigenvalue_matrix(n, eigs=(-2.0, 0.0, 2.0), weights=(0.05, 0.9, 0.05))
    nat = Native("dense", n)
    nat.op, nat.apply = DenseOperator(to_dev(A)), mref.dense_apply(A)
    v0 = unit(v0)[None, :]
    # the reference: alive, alive, dead -- with its margins
    Vr = np.zeros((4, n), dtype=LD)
    Vr[0] = v0[0]
    for j in range(3):
        s = kr.arnoldi_step(Vr[: j + 1], nat.apply(Vr[j], LD)[0], 0.0, LD)
        assert s.dead == (j == 2) and (s.margin_dead <= 1 / kr.MARGIN if j == 2 else s.margin_dead >= kr.MARGIN), (j, s.margin_dead)
        assert s.second == (j == 2) and (s.margin_dgks <= 1 / kr.MARGIN if j == 2 else s.margin_dgks >= kr.MARGIN_NO_SECOND), (j, s.margin_dgks)
        if not s.dead:
            Vr[j + 1] = s.v_next
    lib = _lib.load()
    Vd, Hd = nat.buffers(7, v0)
    nat.extend(Vd, Hd, 0, 5)
    assert statuses(nat.ws) == ((_lib.ERR_BREAKDOWN, 3), (_lib.ERR_BREAKDOWN, 3), -1)
    assert bool((Hd[2, :4] != SENTINEL).all()) and bool((Hd[3:] == SENTINEL).all()) and bool((Vd[3:] == SENTINEL).all())
    Vb, Hb = Vd.clone(), Hd.clone()
    nat.extend(Vd, Hd, 3, 5)
    assert torch.equal(Vd, Vb) and torch.equal(Hd, Hb), "extend after a breakdown was not a no-op"
    Vn, Hn = nat.buffers(7, v0)
    nat.extend(Vn, Hn, 0, 1)
    assert statuses(nat.ws) == ((0, 0), (0, 0), -1), "a new factorisation did not clear the record"
    assert torch.equal(Vn[:2], Vd[:2]) and torch.equal(Hn[0], Hd[0])
    # optimistic mode: step 2 fails the DGKS test first, the redo records the breakdown
    Vo, Ho = nat.buffers(7, v0)
    nat.extend(Vo, Ho, 0, 5, optimistic=True)
    a, b, r = c_int(-5), c_int(-5), c_int(-5)
    assert lib.dsea_arnoldi_status(nat.ws.handle, byref(b), byref(r), st()) == _lib.ERR_SECOND_PASS and r.value == 2 and b.value == 0
    nat.extend(Vo, Ho, 2, 3)
    assert statuses(nat.ws) == ((_lib.ERR_BREAKDOWN, 3), (_lib.ERR_BREAKDOWN, 3), -1)
    assert torch.equal(Vo, Vd) and torch.equal(Ho, Hd)


def test_arnoldi_exactly_zero_step_native():
    """v0 = e_k on a diagonal matrix, shift = A_kk: (A - shift I) v0 == 0 -- the dead branch of k_arnoldi_finish_opt (the
    DGKS test 0 >= 0.5 * 0 passes), record 1 in both modes and no redo"""
    n, k = 300, 7
    d = np.arange(1, n + 1) / 8.0
    nat = Native("dense", n)
    nat.op = DenseOperator(to_dev(np.diag(d)))
    e = np.zeros((1, n))
    e[0, k] = 1.0
    for optimistic in (False, True):
        V, H = nat.buffers(4, e)
        nat.extend(V, H, 0, 2, float(d[k]), optimistic)
        assert statuses(nat.ws) == ((_lib.ERR_BREAKDOWN, 1), (_lib.ERR_BREAKDOWN, 1), -1), optimistic
        assert second_passes(nat.ws) == 0
        assert H[0, :2].cpu().tolist() == [0.0, 0.0] and bool((H[0, 2:] == SENTINEL).all()) and bool((H[1:] == SENTINEL).all())
        assert bool((V[1:] == SENTINEL).all())


# ====================================================================================== GMRES stages
class GmresRun:
    """the staged calls (callable form: u from dsea_spmv on the same dense handle) and the native cycle on one matrix"""

    def __init__(self, n, m, dense, ws=None, kmax=None):
        self.n, self.m, self.A = n, m, dense
        self.op = DenseOperator(to_dev(dense))
        self.apply = mref.dense_apply(dense)
        self.ws = ws or Workspace.get(n, max(m + 2, kmax or 0), dev())
        self.ldv = round_up(n, 32) + 32
        self.lib = _lib.load()
        self.nwork = int(self.lib.dsea_gmres_work_doubles(m))
        self.reset()

    def reset(self):
        self.V = torch.zeros((self.m + 1, self.ldv), dtype=F64, device=dev())
        self.V[:, self.n:] = SENTINEL
        self.work = sentinels(self.nwork + 4)
        self.state = sentinels(8)

    def begin(self, b, Ax, target, expect=0):
        self.b = to_dev(b)
        self.Ax = None if Ax is None else to_dev(Ax)
        rc = self.lib.dsea_gmres_begin(self.ws.handle, _ptr(self.b), _ptr(self.Ax), _ptr(self.V), self.ldv, self.n, self.m,
                                       _ptr(self.work), float(target), _ptr(self.state), st())
        assert rc == expect, rc
        torch.cuda.synchronize()

    def spmv(self, v):
        u = sentinels(self.n)
        _lib.check(self.lib.dsea_spmv(self.op.handle, self.ws.handle, _ptr(v), _ptr(u), None, None, None, st()))
        return u

    def step(self, j, shift, target, native=False):
        sh = scalar(shift)
        u = None if native else self.spmv(self.V[j, : self.n])
        rc = self.lib.dsea_gmres_step(self.op.handle if native else None, self.ws.handle, _ptr(sh), _ptr(u), _ptr(self.V),
                                      self.ldv, self.n, j, self.m, _ptr(self.work), float(target), _ptr(self.state), st())
        assert rc == 0, rc
        torch.cuda.synchronize()

    def end(self, x):
        rc = self.lib.dsea_gmres_end(self.ws.handle, _ptr(self.V), self.ldv, self.n, self.m, _ptr(self.work), _ptr(self.state),
                                     _ptr(x), st())
        assert rc == 0, rc
        torch.cuda.synchronize()

    def staged(self, b, shift, target, x0=None):
        """begin, m steps, end; returns x (device)"""
        self.reset()
        x = torch.zeros(self.n, dtype=F64, device=dev()) if x0 is None else to_dev(x0)
        Ax = None
        if x0 is not None:
            Ax = (self.spmv(x) - (shift or 0.0) * x).cpu().numpy()
        self.begin(b, Ax, target)
        for j in range(self.m):
            self.step(j, shift, target)
        self.end(x)
        return x

    def cycle(self, b, shift, target, x0=None, optimistic=False):
        self.reset()
        x = torch.zeros(self.n, dtype=F64, device=dev()) if x0 is None else to_dev(x0)
        bd, sh = to_dev(b), scalar(shift)
        _lib.check(self.lib.dsea_ws_set_arnoldi_optimistic(self.ws.handle, 1 if optimistic else 0))
        try:
            rc = self.lib.dsea_gmres_cycle(self.op.handle, self.ws.handle, _ptr(sh), _ptr(bd), _ptr(x), _ptr(self.V), self.ldv,
                                           self.m, _ptr(self.work), float(target), _ptr(self.state), int(x0 is None), st())
        finally:
            _lib.check(self.lib.dsea_ws_set_arnoldi_optimistic(self.ws.handle, 0))
        assert rc == 0, rc
        torch.cuda.synchronize()
        return x

    def carve(self):
        """the work layout of include/dsea.h: H (m+1) x m column-major | cs[m] | sn[m] | g[m+1] | y[m]"""
        m, w = self.m, self.work.cpu().numpy()
        assert (w[self.nwork:] == SENTINEL).all(), "written beyond dsea_gmres_work_doubles(m)"
        o = (m + 1) * m
        return w[:o].reshape(m, m + 1), w[o:o + m], w[o + m:o + 2 * m], w[o + 2 * m:o + 3 * m + 1], w[o + 3 * m + 1:o + 4 * m + 1]

    def judge(self, tag, b, shift, x, x0=None, k_expect=None):
        """state[0] against the true residual, x against the longdouble least-squares minimiser over the device's own V[:k];
        the structure of `work`.  Returns the two worst ratios."""
        n, m = self.n, self.m
        state = self.state.cpu().numpy()
        k = int(state[2])
        if k_expect is not None:
            assert k == k_expect, (tag, k)
        shift = shift or 0.0
        Vh = self.V[:, :n].cpu().numpy()
        assert bool((self.V[:, n:] == SENTINEL).all()), "%s: the padding of V was written" % tag
        xh = x.cpu().numpy()
        xl, rl, _, Rm = kr.lstsq_over(self.apply, shift, b, x0, Vh[:k])
        sv = sv_of(self.A, shift)
        nb = float(state[3])
        bx, br = kr.gmres_bounds(n, n, k, float(sv[0]), nb, kr.subspace_cond(sv[0], Rm))
        ex = float(np.sqrt(np.sum((np.asarray(xh, dtype=LD) - xl) ** 2)))
        true = np.asarray(b, dtype=LD) - (self.apply(xh, LD)[0] - LD(shift) * np.asarray(xh, dtype=LD))
        er = abs(float(np.sqrt(np.sum(true * true))) - float(state[0]))
        print("%s: columns %d  |x - x_ls| / bound = %.4f  |state[0] - true residual| / bound = %.4f" % (tag, k, ex / bx, er / br))
        assert ex <= bx and er <= br, (tag, ex / bx, er / br)
        H, cs, sn, g, y = self.carve()
        for j in range(k):
            assert (H[j, j + 1: j + 2] == 0.0).all(), "%s: the rotated H has a sub-diagonal entry" % tag
            assert abs(cs[j] ** 2 + sn[j] ** 2 - 1.0) <= 4 * kr.U, (tag, j, cs[j], sn[j])
        assert (y[k:] == 0.0).all() and np.isfinite(y).all(), tag
        return ex / bx, er / br


@functools.lru_cache(maxsize=None)
def _sv(key, shift):
    return np.linalg.svd(_SV_MATS[key] - shift * np.eye(_SV_MATS[key].shape[0]), compute_uv=False)


_SV_MATS = {}


def sv_of(A, shift):
    key = (A.shape[0], float(A[0, 0]), float(A[-1, -1]))
    _SV_MATS[key] = A
    return _sv(key, float(shift))


GMRES_CASES = [(n, m) for n in (1, 2, 3, 300, 1001) for m in (1, 4, 8) if m <= n]


@pytest.mark.parametrize("n,m", GMRES_CASES)
def test_gmres_begin_and_converged_at_the_start(n, m):
    g = GmresRun(n, m, kr.dense_noise(n))
    b = normal_vector(n, 40 + n)
    x0 = normal_vector(n, 41 + n)
    for Ax in (None, (kr.dense_noise(n) @ x0)):
        r0 = np.asarray(b, dtype=LD) - (0 if Ax is None else np.asarray(Ax, dtype=LD))
        nr = np.sqrt(np.sum(r0 * r0))
        g.reset()
        g.begin(b, Ax, 0.0)
        s = g.state.cpu().numpy()
        bound = (n / 2 + 4) * kr.U * float(nr)        # a difference, n squares summed in any order, a root
        assert s[0] == s[3] and abs(LD(s[0]) - nr) <= bound, (s[0], float(nr))
        assert (s[[1, 2, 4, 5, 6]] == 0.0).all() and s[7] == SENTINEL, s
        v0 = g.V[0, :n].cpu().numpy()
        # v0 = r0^ / ||r0^||: the difference rounds once, the norm as above, the division once
        vb = (n / 2 + 8) * kr.U * np.abs(np.asarray(r0 / nr, dtype=np.float64)) + 2 * kr.U * (
            np.abs(b) + (0 if Ax is None else np.abs(Ax))) / float(nr)
        assert kr.worst_ratio(np.abs(np.asarray(v0, dtype=LD) - r0 / nr), vb) <= 1.0
        assert bool((g.V[1:, :n] == 0.0).all())
        # converged at the start
        g.reset()
        g.begin(b, Ax, 2 * float(nr))
        s = g.state.cpu().numpy()
        assert s[1] == s[4] == 1.0 and s[2] == 0.0 and s[0] == s[3], s
        assert bool((g.V[:, :n] == 0.0).all()), "V[0] written although the cycle started converged"
        Vb, wb = g.V.clone(), g.work.clone()
        for j in range(m):
            g.step(j, None, 2 * float(nr))
        assert torch.equal(g.V, Vb), "a step of a converged cycle wrote V"
        assert torch.equal(g.work, wb), "a step of a converged cycle wrote `work`"
        x = to_dev(x0)
        g.end(x)
        assert np.array_equal(x.cpu().numpy(), x0), "end of a converged cycle changed x"


@pytest.mark.parametrize("n,m", GMRES_CASES)
def test_gmres_full_cycle_staged_and_native(n, m):
    g = GmresRun(n, m, kr.dense_noise(n))
    b = normal_vector(n, 50 + n)
    worst = [0.0, 0.0]
    for shift in (None, kr.SHIFT_RANDOM):
        x = g.staged(b, shift, 0.0)
        s_staged, V_staged, w_staged = g.state.clone(), g.V.clone(), g.work.clone()
        _, ref_state, _ = kr.gmres_cycle(g.apply, shift or 0.0, b, None, m, 0.0)
        k = int(ref_state[2])
        assert k == m or n <= 3
        r = g.judge("gmres n=%d m=%d shift=%s" % (n, m, shift), b, shift, x, k_expect=k)
        worst = [max(a, c) for a, c in zip(worst, r)]
        xn = g.cycle(b, shift, 0.0)
        assert torch.equal(xn, x) and torch.equal(g.state, s_staged) and torch.equal(g.V, V_staged) and torch.equal(g.work, w_staged), \
            "the native cycle differs from the staged sequence"


def test_gmres_converges_in_mid_cycle():
    n, m = 300, 8
    b = normal_vector(n, 5)
    target, apply = kr.midcycle_target(n, b)
    g = GmresRun(n, m, kr.dense_noise(n, scale=0.4))
    for native in (False, True):
        x = g.cycle(b, None, target) if native else g.staged(b, None, target)
        s = g.state.cpu().numpy()
        assert s[2] == 3.0 and s[1] == s[4] == 1.0 and s[5] == s[6] == 0.0, s
        # three columns: steps 0..2 wrote rows 1..3, the step after the converged one is a no-op
        assert bool((g.V[4:, :n] == 0.0).all()) and bool((g.V[3, :n] != 0.0).any())
        g.judge("gmres mid-cycle native=%s" % native, b, None, x, k_expect=3)


def test_gmres_exhausts_the_krylov_space():
    n, m = 300, 8
    A = kr.three_eigenvalue_matrix(n)
    g = GmresRun(n, m, A)
    b = normal_vector(n, 5)
    for native in (False, True):
        x = g.cycle(b, None, 0.0) if native else g.staged(b, None, 0.0)
        s = g.state.cpu().numpy()
        assert s[2] == 3.0 and s[4] == 1.0 and s[1] == 0.0 and s[6] == 0.0, s
        r = np.asarray(b, dtype=LD) - g.apply(x.cpu().numpy(), LD)[0]
        sv = sv_of(A, 0.0)
        _, br = kr.gmres_bounds(n, n, 3, float(sv[0]), float(s[3]), float(sv[0] / sv[-1]))
        rn = float(np.sqrt(np.sum(r * r)))
        print("gmres exhaustion native=%s: true residual %.3e, bound %.3e" % (native, rn, br))
        assert rn <= br + float(s[0])


def test_gmres_restart_from_the_previous_x():
    n, m = 300, 4
    g = GmresRun(n, m, kr.dense_noise(n))
    b = normal_vector(n, 61)
    x1r, s1r, _ = kr.gmres_cycle(g.apply, kr.SHIFT_RANDOM, b, None, m, 0.0)
    x2r, s2r, _ = kr.gmres_cycle(g.apply, kr.SHIFT_RANDOM, b, x1r, m, 0.0)
    sv = sv_of(g.A, kr.SHIFT_RANDOM)
    for native in (False, True):
        x1 = g.cycle(b, kr.SHIFT_RANDOM, 0.0) if native else g.staged(b, kr.SHIFT_RANDOM, 0.0)
        e1 = float(g.state[0])
        x1h = x1.cpu().numpy()
        x2 = g.cycle(b, kr.SHIFT_RANDOM, 0.0, x0=x1h) if native else g.staged(b, kr.SHIFT_RANDOM, 0.0, x0=x1h)
        e2 = float(g.state[0])
        g.judge("gmres restart native=%s" % native, b, kr.SHIFT_RANDOM, x2, x0=x1h, k_expect=m)
        # the estimates against the reference's restarted GMRES: cycle 1 by the cycle bound; cycle 2 starts from an x that
        # differs from the reference's by at most bx, which moves its r0 (and every later residual) by at most ||A_s|| bx
        bx, br = kr.gmres_bounds(n, n, m, float(sv[0]), float(s1r[3]), float(sv[0] / sv[-1]))
        assert abs(e1 - float(s1r[0])) <= br, (e1, float(s1r[0]))
        assert abs(e2 - float(s2r[0])) <= 2 * br + float(sv[0]) * bx, (e2, float(s2r[0]))
        assert e2 < e1


def test_gmres_optimistic_step_ends_the_cycle():
    """the rank-one-plus-1e-6-noise matrix of test_gpu_eig.py at n = 1024: step 1 needs the second pass"""
    rng = np.random.RandomState(78)
    n, m = 1024, 6
    u, v = rng.randn(n), rng.randn(n)
    G = np.outer(u, v + 0.5 * u) / n + 1e-6 * rng.randn(n, n)
    b = rng.randn(n)
    shift = None
    g = GmresRun(n, m, G)
    # the failing step according to the reference, with its margin
    xr, sr, ex = kr.gmres_cycle(g.apply, 0.0, b, None, m, 0.0)
    Vr = ex["V"]
    fail = None
    for j in range(m):
        s = kr.arnoldi_step(Vr[: j + 1], g.apply(Vr[j], LD)[0], 0.0, LD)
        if s.second:
            assert s.margin_dgks <= 1 / kr.MARGIN
            fail = j
            break
        assert s.margin_dgks >= kr.MARGIN_NO_SECOND
    assert fail is not None and fail >= 1
    x = g.cycle(b, shift, 0.0, optimistic=True)
    s = g.state.cpu().numpy()
    assert s[5] == 1.0 and s[4] == 1.0 and s[1] == 0.0 and s[2] == float(fail) and s[6] == 0.0, (s, fail)
    xh = x.cpu().numpy()
    xl, _, _, Rm = kr.lstsq_over(g.apply, 0.0, b, None, g.V[:fail, :n].cpu().numpy())
    sv = sv_of(G, 0.0)
    bx, _ = kr.gmres_bounds(n, n, fail, float(sv[0]), float(s[3]), kr.subspace_cond(sv[0], Rm))
    ex_ = float(np.sqrt(np.sum((np.asarray(xh, dtype=LD) - xl) ** 2)))
    print("gmres optimistic: ended with %d columns, |x - x_ls| / bound = %.4f" % (fail, ex_ / bx))
    assert ex_ <= bx
    lib = _lib.load()
    _lib.check(lib.dsea_arnoldi_clear_record(g.ws.handle, st()))


@pytest.mark.parametrize("n", [3, 300])
def test_gmres_singular_column(n):
    """(A - shift I) v0 == 0 exactly: diagonal A, b = e_k, shift = A_kk.  include/dsea.h state[6]: the column is not counted,
    nothing claims convergence, x stays finite and unchanged; krylov.gmres raises instead of cycling"""
    k = n // 2
    d = np.arange(1, n + 1) / 8.0
    A = np.diag(d)
    e = np.zeros(n)
    e[k] = 1.0
    g = GmresRun(n, min(4, n), A)
    for native in (False, True):
        x = g.cycle(e, float(d[k]), 1e-12) if native else g.staged(e, float(d[k]), 1e-12)
        s = g.state.cpu().numpy()
        assert s[6] == 1.0 and s[4] == 1.0 and s[1] == 0.0 and s[2] == 0.0 and s[0] == 1.0 and s[3] == 1.0, (native, s)
        xh = x.cpu().numpy()
        assert np.isfinite(xh).all() and not xh.any(), "x changed by a cycle that made no progress"
        H, cs, sn, gg, y = g.carve()
        assert not y.any() and np.isfinite(y).all()
    for operand in (g.op, lambda v: g.op(v)):
        with pytest.raises(RuntimeError, match="singular"):
            krylov.gmres(operand, to_dev(e), shift=scalar(float(d[k])))
    # a consistent system on the same matrix is solved
    xs = krylov.gmres(g.op, to_dev(e), shift=scalar(0.0625))
    assert abs(float(xs[k]) - 1.0 / (d[k] - 0.0625)) <= 1e-12 * abs(1.0 / (d[k] - 0.0625))


def test_gmres_refusals_enqueue_nothing():
    n, m = 300, 4
    g = GmresRun(n, m, kr.dense_noise(n))
    lib, ws = g.lib, g.ws
    b, x = to_dev(normal_vector(n, 1)), sentinels(n + 2)
    big = sentinels(n + 2)
    u = sentinels(n + 2)
    sh = None

    def begin(V=None, ldv=None, bb=None, Ax=None, mm=m, wsh=None):
        return lib.dsea_gmres_begin((wsh or ws).handle, _ptr(b) if bb is None else bb, Ax, _ptr(g.V) if V is None else V,
                                    g.ldv if ldv is None else ldv, n, mm, _ptr(g.work), 0.0, _ptr(g.state), st())

    def step(V=None, ldv=None, uu=None, j=0, mm=m, wsh=None, op=None):
        return lib.dsea_gmres_step(op, (wsh or ws).handle, sh, _ptr(u) if uu is None else uu, _ptr(g.V) if V is None else V,
                                   g.ldv if ldv is None else ldv, n, j, mm, _ptr(g.work), 0.0, _ptr(g.state), st())

    def end(V=None, ldv=None, xx=None, mm=m):
        return lib.dsea_gmres_end(ws.handle, _ptr(g.V) if V is None else V, g.ldv if ldv is None else ldv, n, mm, _ptr(g.work),
                                  _ptr(g.state), _ptr(x) if xx is None else xx, st())

    off = lambda t: ctypes.c_void_p(t.data_ptr() + 8)     # noqa: E731
    small = Workspace(n, m, dev())                        # kmax = m < m + 1
    g.reset()
    keep = (g.V.clone(), g.work.clone(), g.state.clone())
    calls = [
        (begin(mm=0), _lib.ERR_ARG), (begin(mm=65), _lib.ERR_ARG), (step(mm=0), _lib.ERR_ARG), (step(mm=65), _lib.ERR_ARG),
        (end(mm=0), _lib.ERR_ARG), (end(mm=65), _lib.ERR_ARG), (step(j=m), _lib.ERR_ARG), (step(j=m + 1), _lib.ERR_ARG),
        (step(j=-1), _lib.ERR_ARG),
        (begin(ldv=g.ldv - 1), ERR_ALIGN), (step(ldv=g.ldv - 1), ERR_ALIGN), (end(ldv=g.ldv - 1), ERR_ALIGN),
        (begin(V=off(g.V)), ERR_ALIGN), (step(V=off(g.V)), ERR_ALIGN), (end(V=off(g.V)), ERR_ALIGN),
        (begin(bb=off(big)), ERR_ALIGN), (begin(Ax=off(big)), ERR_ALIGN), (step(uu=off(big)), ERR_ALIGN),
        (end(xx=off(x)), ERR_ALIGN),
        (begin(wsh=small), ERR_WORKSPACE), (step(wsh=small), ERR_WORKSPACE), (step(wsh=small, op=g.op.handle), ERR_WORKSPACE),
    ]
    for i, (rc, want) in enumerate(calls):
        assert rc == want, (i, rc, want)
    xs = sentinels(n + 2)
    rc = lib.dsea_gmres_cycle(g.op.handle, ws.handle, None, _ptr(b), off(xs), _ptr(g.V), g.ldv, m, _ptr(g.work), 0.0,
                              _ptr(g.state), 1, st())
    assert rc == ERR_ALIGN
    torch.cuda.synchronize()
    assert torch.equal(g.V, keep[0]) and torch.equal(g.work, keep[1]) and torch.equal(g.state, keep[2])
    assert bool((x == SENTINEL).all()) and bool((xs == SENTINEL).all()) and bool((u == SENTINEL).all())
