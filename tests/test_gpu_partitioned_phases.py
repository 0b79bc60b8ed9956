"""The row-partitioned macro phases of include/dsea.h, one by one, in ONE process on the MI355X: dsea_lanczos_form_r,
dsea_hypercube_flipsum, dsea_plz_dots, dsea_plz_correct, dsea_plz_correct_matvec, dsea_axpy_multi_dot, dsea_plz_finish.

Each phase against the plain fp64 expression of the header (tests/partitioned_reference.py, proved on the CPU by
tests/test_partitioned_phase_reference_cpu.py) on ragged slab sizes, with the basis padded by a sentinel that must come back
untouched and never enter a sum.  Tolerances are those of tests/test_gpu_kernels.py: bit-equality where a phase is a sequence
of individually rounded element-wise operations, 1e-13 x operand norms for the reductions, 1e-12 in the form of
test_reorth_pair for the correction pass; the shadow branch of dsea_plz_correct is judged by tests/test_gpu_shadow.py's own
reader bound.  Then the phases composed: P virtual ranks in lockstep against the oracle on the full operator, and phase by
phase against the torch-CPU test double (tests/cpu_backend.py) the CPU-side partitioned suite rests on.

Every error-return case is a host-side argument check of the C ABI (nothing is launched)."""
from contextlib import contextmanager
from ctypes import byref, c_int, c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dominantsparseeigenad_amd import _lib, engine  # noqa: E402
from dominantsparseeigenad_amd.engine import Workspace, _stream, round_up  # noqa: E402
from dominantsparseeigenad_amd.partitioned import HipBackend  # noqa: E402
import partitioned_reference as pr  # noqa: E402
from cpu_backend import CpuBackend  # noqa: E402
from helpers import bf16_bits  # noqa: E402
from partitioned_reference import F64, SENTINEL, padded_basis, ulp_distance, vec  # noqa: E402
from test_gpu_shadow import EPS, LD, ReaderInputs, Registered, lp_stats  # noqa: E402

ERR_ARG, ERR_ALIGN, ERR_WORKSPACE = -1, -2, -3
VSIZES = [1, 2, 3, 63, 65, 129, 1000, 4097, 100000]
BIG = (1 << 22) + 6            # the element-wise grid of 2048 blocks x 2048 rows wraps
A_HOST, A_DEV, SHIFT = -2.0, 0.37, -0.6
ALPHA, BETA = 0.7, -1.3


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


def D(t):
    return t.to(dev())


def P_(t, skip=0):
    """device pointer of a tensor (None: null), optionally ``skip`` doubles further"""
    return c_void_p(t.data_ptr() + 8 * skip) if t is not None else None


def scal(*v):
    return torch.tensor(v, dtype=F64, device=dev())


def guarded(n, init=None):
    """an n-vector followed by four sentinel doubles: (whole buffer, the vector)"""
    buf = torch.full((n + 4,), SENTINEL, dtype=F64, device=dev())
    if init is not None:
        buf[:n] = D(init)
    return buf, buf[:n]


def tail_ok(buf, n):
    return bool((buf[n:] == SENTINEL).all())


def call(name, *args):
    _lib.check(getattr(_lib.load(), name)(*args, _stream(dev())), name)


def ws_of(n, kmax=64):
    return Workspace.get(n, kmax, dev())


@contextmanager
def geometry(ws, kind, value):
    """``dsea_ws_set_rows_per_lane`` / ``dsea_ws_set_split`` forced for the block, automatic again afterwards"""
    try:
        (ws.set_rows_per_lane if kind == "rpl" else ws.set_split)(value)
        yield
    finally:
        ws.set_rows_per_lane(0)
        ws.set_split(-1)


GEOMETRIES = [("rpl", v) for v in (0, 2, 4, 8, 16)] + [("split", v) for v in (4, 8, 16)]


# ------------------------------------------------------------------------------------------------ dsea_lanczos_form_r
FORM_R_CASES = [(1, False, False), (1, True, True), (2, True, True), (2, False, False), (5, True, False), (5, False, True)]


def run_form_r(n, Qd, ldq, ud, i, with_beta, with_copy):
    ab = scal(ALPHA, BETA)
    rbuf, r = guarded(n)
    cbuf, rc = guarded(n)
    call("dsea_lanczos_form_r", ws_of(n).handle, P_(Qd), ldq, n, i, P_(ud), P_(ab), P_(ab, 1) if with_beta else None, P_(r),
         P_(rc) if with_copy else None)
    return rbuf, cbuf


@pytest.mark.parametrize("n", VSIZES + [BIG])
def test_form_r(n):
    """(i, beta given, r_copy given): i = 1 has no q2 whether or not beta is given, a null beta drops the term at i >= 2"""
    cases = FORM_R_CASES if n != BIG else [(2, True, True)]
    Q, ldq = padded_basis(max(c[0] for c in cases), n, 1100 + n % 997)
    u = vec(n, 1200 + n % 997)
    Qd, ud = D(Q), D(u)
    for i, with_beta, with_copy in cases:
        rbuf, cbuf = run_form_r(n, Qd, ldq, ud, i, with_beta, with_copy)
        want = pr.ref_form_r(Q, n, i, u, ALPHA, BETA if with_beta else None)
        assert torch.equal(rbuf[:n].cpu(), want), (i, with_beta, with_copy)
        assert tail_ok(rbuf, n)
        assert torch.equal(cbuf[:n].cpu(), want) if with_copy else tail_ok(cbuf, 0)
        assert tail_ok(cbuf, n)
    assert torch.equal(Qd.cpu(), Q) and torch.equal(ud.cpu(), u)          # inputs and the sentinel padding untouched


# ------------------------------------------------------------------------------------------------ dsea_hypercube_flipsum
@pytest.mark.parametrize("P", [1, 2, 4, 8, 16])
def test_hypercube_flipsum(P):
    """P = 8, chunk = 70001: 560008 elements, beyond 2048 blocks x 256 threads (the grid-stride loop runs); P = 1: zeros"""
    for chunk in (1, 3, 255, 257, 70001):
        x = vec(P * chunk, 2000 + P + chunk)
        xd = D(x)
        zbuf, z = guarded(P * chunk)
        call("dsea_hypercube_flipsum", P_(xd), P_(z), P, chunk)
        want = pr.ref_flipsum(x, P, chunk)
        assert torch.equal(z.cpu(), want), (P, chunk)
        assert tail_ok(zbuf, P * chunk) and torch.equal(xd.cpu(), x)
        if P == 1:
            assert not bool(z.any())


def test_hypercube_flipsum_rejects_bad_arguments():
    lib, st = _lib.load(), _stream(dev())
    x, z = scal(*range(16)), scal(*range(16))
    for P, chunk, a, b in ((3, 4, x, z), (0, 4, x, z), (4, 0, x, z), (4, 4, x, x), (4, 4, None, z)):
        assert lib.dsea_hypercube_flipsum(P_(a), P_(b), P, chunk, st) == ERR_ARG, (P, chunk)
    assert torch.equal(z, scal(*range(16)))


# ------------------------------------------------------------------------------------------------ dsea_plz_dots
def run_plz_dots(ws, n, Qd, ldq, ud, i, with_beta):
    ab = scal(ALPHA, BETA)
    rbuf, r = guarded(n)
    c = torch.full((i + 3,), SENTINEL, dtype=F64, device=dev())
    call("dsea_plz_dots", ws.handle, P_(Qd), ldq, n, i, P_(ud), P_(ab), P_(ab, 1) if with_beta else None, P_(r), P_(c))
    return rbuf, c


def check_plz_dots(n, i, geometries):
    ws = ws_of(n)
    Q, ldq = padded_basis(i, n, 3100 + n % 997 + i)
    u = vec(n, 3200 + n % 997)
    Qd, ud = D(Q), D(u)
    want = pr.ref_form_r(Q, n, i, u, ALPHA, BETA)
    c_ref, rr = Q[:, :n] @ want, float(want @ want)
    tol = 1e-13 * float(want.norm()) * float(Q[:, :n].norm(dim=1).max())
    for idx, (kind, value) in enumerate(geometries):
        with geometry(ws, kind, value):
            rbuf, c = run_plz_dots(ws, n, Qd, ldq, ud, i, i >= 2 or idx % 2 == 0)    # (i = 1: beta is ignored when given)
        label = (n, i, kind, value)
        assert torch.equal(rbuf[:n].cpu(), want), label
        assert tail_ok(rbuf, n), label
        ch = c.cpu()
        assert float((ch[:i] - c_ref).abs().max()) <= tol, label
        assert abs(float(ch[i]) - rr) <= 1e-13 * rr, label
        assert bool((ch[i + 1:] == SENTINEL).all()), label
    assert torch.equal(Qd.cpu(), Q)


@pytest.mark.parametrize("i", [1, 2, 37])
@pytest.mark.parametrize("n", VSIZES)
def test_plz_dots_every_forced_geometry(n, i):
    """r bit-equal to (u - a q1) - b q2, c[:i] = Q r, c[i] = r.r, under every rows-per-lane and every split geometry"""
    check_plz_dots(n, i, GEOMETRIES)


def test_plz_dots_beyond_kmax_is_a_workspace_error():
    n = 129
    ws = Workspace(n, 8, dev())
    Q, ldq = padded_basis(1, n, 5)
    Qd, ud, ab = D(Q), D(vec(n, 6)), scal(ALPHA, BETA)
    rbuf, r = guarded(n)
    c = torch.full((12,), SENTINEL, dtype=F64, device=dev())
    rc = _lib.load().dsea_plz_dots(ws.handle, P_(Qd), ldq, n, 9, P_(ud), P_(ab), P_(ab, 1), P_(r), P_(c), _stream(dev()))
    assert rc == ERR_WORKSPACE
    assert tail_ok(rbuf, 0) and tail_ok(c, 0)


# ------------------------------------------------------------------------------------------------ dsea_plz_correct
def run_plz_correct(ws, n, Qd, ldq, row, cd, r0):
    rbuf, r = guarded(n, r0)
    pair = scal(0.0, SENTINEL)
    call("dsea_plz_correct", ws.handle, P_(Qd) if row else None, ldq, n, row, P_(cd) if row else None, P_(r), P_(pair))
    return rbuf, pair


def check_plz_correct(n, row, geometries):
    ws = ws_of(n)
    Q, ldq = padded_basis(max(row, 1), n, 4100 + n % 997 + row)
    r0, c = vec(n, 4200 + n % 997), vec(max(row, 1), 4300 + row)
    Qd, cd = D(Q), D(c)
    want = pr.ref_correct(Q, n, row, c, r0)
    ww = float(want @ want)
    sub = Q[:row, :n].T @ c[:row] if row else torch.zeros(n, dtype=F64)
    for kind, value in geometries:
        with geometry(ws, kind, value):
            rbuf, pair = run_plz_correct(ws, n, Qd, ldq, row, cd, r0)
        label = (n, row, kind, value)
        got = rbuf[:n].cpu()
        if row == 0:
            assert torch.equal(got, r0), label             # only the norm is taken
        else:
            assert float((got - want).abs().max()) <= 1e-12 * float(r0.abs().max() + sub.abs().max()), label
        assert tail_ok(rbuf, n), label
        assert abs(float(pair[0]) - ww) <= 1e-12 * ww, label
        assert float(pair[1]) == SENTINEL, label           # pair_out[1] belongs to the mat-vec's dot
    assert torch.equal(Qd.cpu(), Q)


@pytest.mark.parametrize("row", [0, 1, 5, 37])
@pytest.mark.parametrize("n", VSIZES)
def test_plz_correct_without_a_shadow(n, row):
    """automatic, forced wave-owned and forced split geometry; row = 0 takes null Q and c and leaves r alone"""
    check_plz_correct(n, row, [("split", -1), ("split", 0), ("split", 16)])


@pytest.mark.parametrize("n,row", [(129, 1), (1000, 5), (4097, 37), (100000, 5)])
def test_plz_correct_with_a_registered_shadow(n, row):
    """A bf16 shadow whose rows are the exact roundings of Q, O(1) coefficients: the shadow formula and the fp64 formula
    differ at the 2^-9 level, so each run shows which branch it took -- and dsea_lanczos_lp_stats counts it.
      * wave-owned geometry, premise holds (tau^2 ||r||^2 = 4 max c_j^2): the shadow reader        -> stats (1, 0)
      * wave-owned geometry, premise fails (tau^2 ||r||^2 = max c_j^2 / 4): fp64 inside the reader -> stats (0, 1)
      * forced split geometry: the fp64 kernels, the reader is not launched                        -> stats (0, 0)
      * a shadow of exactly `row` rows (shadow_rows == row): not used                              -> stats (0, 0)
    Every result against the longdouble evaluation of its own formula within the reader bound of tests/test_gpu_shadow.py,
    (i + 18) 2^-53 S element-wise.  With the production tau and coefficients a thousand times below the premise threshold the
    shadow run must agree with the run without a shadow: each lies within that bound of its own formula and the two formulas
    differ by sum_j |c_j| |Q_j - bf16(Q_j)|, which is computed, not estimated."""
    lib, st = _lib.load(), _stream(dev())
    ws = Workspace.get(n, max(row, 8), dev())
    inp = ReaderInputs(n, row, n % 2 == 1, 9900 + n + row)
    bits = bf16_bits(inp.Q[:, :n].cpu().numpy())
    inp.Qs[:row, :n] = torch.from_numpy(bits.view(np.int16).copy()).to(dev())
    inp.Qs_before = inp.Qs.clone()

    def run(split, shadow_rows, tau):
        r = inp.r0.clone()
        pair = scal(0.0, SENTINEL)
        with geometry(ws, "split", split):
            with Registered(ws, inp.Qs, inp.lds, shadow_rows, tau):
                before = lp_stats(ws)
                _lib.check(lib.dsea_plz_correct(ws.handle, P_(inp.Q), inp.ldq, n, row, P_(inp.c), P_(r), P_(pair), st),
                           "dsea_plz_correct")
                after = lp_stats(ws)
        assert torch.equal(inp.Qs, inp.Qs_before) and float(pair[1]) == SENTINEL
        return r, pair[:1], (after[0] - before[0], after[1] - before[1])

    c = inp.c.cpu().numpy()
    cmax2, rr = float(np.max(c[:row] ** 2)), float(c[row])
    for split, rows, tau, which, stats in ((0, inp.rows, np.sqrt(4.0 * cmax2 / rr), "shadow", (1, 0)),
                                           (0, inp.rows, np.sqrt(0.25 * cmax2 / rr), "fp64", (0, 1)),
                                           (16, inp.rows, 1e6, "fp64", (0, 0)),
                                           (0, row, 1e6, "fp64", (0, 0))):
        r, nrm2, adv = run(split, rows, tau)
        assert adv == stats, (split, rows, tau, adv)
        inp.check(r, nrm2, which, "plz_correct split=%d shadow_rows=%d tau=%.3g" % (split, rows, tau))
    # production threshold, coefficients far below it: shadow and no shadow agree
    inp.c[:row] *= 1e-3 * engine.SHADOW_TAU * float(np.sqrt(rr / cmax2))
    r_sh, n_sh, adv = run(0, inp.rows, engine.SHADOW_TAU)
    assert adv == (1, 0)
    inp.check(r_sh, n_sh, "shadow", "plz_correct below the threshold")
    with geometry(ws, "split", 0):
        rbuf, pair = run_plz_correct(ws, n, inp.Q, inp.ldq, row, inp.c, inp.r0)
    inp.check(rbuf[:n], pair[:1], "fp64", "plz_correct without a shadow")
    ref_sh, S = inp.reference("shadow")
    ref_64, _ = inp.reference("fp64")
    allowed = 2 * (row + 18) * EPS * S + np.abs(ref_sh - ref_64)
    diff = np.abs(r_sh.cpu().numpy().astype(LD) - rbuf[:n].cpu().numpy().astype(LD))
    assert bool(np.all(diff <= allowed))


# ------------------------------------------------------------------------------------------------ dsea_plz_correct_matvec
def tfim_slab():
    be = HipBackend(16, dev())
    be.attach_tfim(6, 4, 32, scal(pr.TFIM_G))
    cpu = CpuBackend(16)
    cpu.attach_tfim(6, 4, 32, torch.tensor([pr.TFIM_G], dtype=F64))
    return be, cpu, 16


def stencil_slab(n=1000):
    V, halo = pr.stencil_potential(n), torch.tensor([0.7, -0.4], dtype=F64)
    be = HipBackend(n, dev())
    be.attach_stencil(n, -0.5 * n * n, D(V), D(halo), True, True)
    cpu = CpuBackend(n)
    cpu.attach_stencil(n, -0.5 * n * n, V, halo, True, True)
    return be, cpu, n


def csr_slab():
    n, hb = 301, 2
    rng = np.random.RandomState(17)
    rowptr = torch.arange(0, 5 * n + 1, 5, dtype=torch.int64)
    cols = (torch.arange(n)[:, None] + torch.arange(-hb, hb + 1)[None, :]).reshape(-1).to(torch.int32)   # local, in [-hb, n + hb)
    vals = torch.from_numpy(rng.randn(5 * n))
    halo = torch.from_numpy(rng.randn(2 * hb))
    be = HipBackend(n, dev())
    be.attach_csr(D(rowptr), D(cols), D(vals), n, hb, D(halo), None)
    cpu = CpuBackend(n)
    cpu.attach_csr(rowptr, cols, vals, n, hb, halo, None)
    return be, cpu, n


@pytest.mark.parametrize("slab", [tfim_slab, stencil_slab, csr_slab])
def test_plz_correct_matvec_is_correct_then_spmv(slab):
    """TFIM slab (L = 6, L_local = 4, row_offset = 32), stencil slab with both halos, CSR slab with hb = 2: bit-identical to
    dsea_plz_correct followed by dsea_spmv on the same handle; y = A_local r also against the test double's slab operator"""
    be, cpu, n = slab()
    lib, st = _lib.load(), _stream(dev())
    be.reserve(8)
    Q, ldq = padded_basis(5, n, 5100 + n)
    r0, c = vec(n, 5200 + n), vec(6, 5300)
    Qd, cd = D(Q), D(c)
    for row in (0, 5):
        rbuf1, r1 = guarded(n, r0)
        ybuf1, y1 = guarded(n)
        pair1 = scal(0.0, SENTINEL)
        be.plz_correct_matvec(Qd, ldq, row, cd, r1, y1, pair1)
        rbuf2, r2 = guarded(n, r0)
        ybuf2, y2 = guarded(n)
        pair2 = scal(0.0, SENTINEL)
        be.plz_correct(Qd, ldq, n, row, cd, r2, pair2)
        _lib.check(lib.dsea_spmv(be.op.handle, None, P_(r2), P_(y2), None, None, None, st), "dsea_spmv")
        assert torch.equal(rbuf1, rbuf2) and torch.equal(ybuf1, ybuf2) and torch.equal(pair1, pair2)
        assert tail_ok(rbuf1, n) and tail_ok(ybuf1, n) and float(pair1[1]) == SENTINEL
        want = pr.ref_correct(Q, n, row, c, r0)
        assert float((r1.cpu() - want).abs().max()) <= 1e-12 * float(r0.abs().max() + 6 * Q[:, :n].abs().max() * c.abs().max())
        y_cpu = torch.zeros(n, dtype=F64)
        rh = r1.cpu()
        cpu._local(rh, y_cpu)
        assert float((y1.cpu() - y_cpu).abs().max()) <= 1e-13 * float(y_cpu.abs().max() + 1.0)
    assert lib.dsea_plz_correct_matvec(be.op.handle, be.ws.handle, P_(Qd), ldq, 5, P_(cd), P_(r1), P_(r1), P_(pair1), st) == ERR_ARG
    assert torch.equal(rbuf1, rbuf2)


# ------------------------------------------------------------------------------------------------ dsea_axpy_multi_dot
def run_axpy_multi_dot(ws, n, xs_d, count, a_dev, shift, skip, xd, y0):
    ybuf, y = guarded(n, y0)
    out = scal(SENTINEL)
    arr = (c_void_p * 6)(*[t.data_ptr() for t in xs_d[:count]])
    call("dsea_axpy_multi_dot", ws.handle, A_HOST, P_(a_dev), arr, count, P_(shift), P_(skip), P_(xd), P_(y), n, P_(out))
    return ybuf, out


def check_axpy_multi_dot(n, counts):
    ws = ws_of(n)
    x, y0 = vec(n, 6100 + n % 997), vec(n, 6200 + n % 997)
    xs = [vec(n, 6300 + 7 * j + n % 997) for j in range(max(counts))]
    xd, xs_d = D(x), [D(t) for t in xs]
    ad, sh, skips = scal(A_DEV), scal(SHIFT), {None: None, 0: scal(0.0), 1: scal(1.0)}
    for count in counts:
        for a_dev in (None, ad):
            for shift in (None, sh):
                for skip in (None, 0, 1):
                    ybuf, out = run_axpy_multi_dot(ws, n, xs_d, count, a_dev, shift, skips[skip], xd, y0)
                    label = (n, count, a_dev is not None, shift is not None, skip)
                    got = ybuf[:n].cpu()
                    assert tail_ok(ybuf, n), label
                    if skip == 1:
                        assert torch.equal(got, y0) and float(out[0]) == SENTINEL, label
                        continue
                    want = pr.ref_axpy_multi(A_HOST, A_DEV if a_dev is not None else None, xs[:count],
                                             SHIFT if shift is not None else None, x, y0)
                    assert torch.equal(got, want), label
                    if count == 0 and shift is None:
                        assert torch.equal(got, y0), label           # nothing is written, only the dot is produced
                    assert abs(float(out[0]) - float(x @ want)) <= 1e-13 * float(x.norm() * want.norm()), label


@pytest.mark.parametrize("n", VSIZES)
def test_axpy_multi_dot(n):
    """sum = ((xs0 + xs1) + ...) ; y = y + a sum ; y = y - s x with a = a_host * a_dev[0], bit for bit; every combination of
    count, a_dev, shift and skip flag"""
    check_axpy_multi_dot(n, (0, 1, 2, 3, 6))


def test_axpy_multi_dot_rejects_bad_arguments():
    lib, st = _lib.load(), _stream(dev())
    n = 130
    ws = ws_of(n)
    x, y0 = D(vec(n, 1)), vec(n, 2)
    xs = [D(vec(n + 2, 10 + j)) for j in range(7)]
    ybuf, y = guarded(n, y0)
    out = scal(SENTINEL)

    def rc(ptrs, count):
        arr = (c_void_p * 8)(*ptrs)
        return lib.dsea_axpy_multi_dot(ws.handle, A_HOST, None, arr, count, None, None, P_(x), P_(y), n, P_(out), st)

    good = [t.data_ptr() for t in xs]
    assert rc(good, 7) == ERR_ARG
    assert rc(good[:2] + [None] + good[3:], 4) == ERR_ARG                       # a null entry
    assert rc(good[:1] + [good[1] + 8] + good[2:], 3) == ERR_ALIGN              # a misaligned entry
    assert lib.dsea_axpy_multi_dot(ws.handle, A_HOST, None, None, 2, None, None, P_(x), P_(y), n, P_(out), st) == ERR_ARG
    assert torch.equal(ybuf[:n].cpu(), y0) and tail_ok(ybuf, n) and float(out[0]) == SENTINEL


# ------------------------------------------------------------------------------------------------ dsea_plz_finish
def run_plz_finish(ws, n, rd, yd, pair, with_beta):
    ldq = round_up(n, 32) + (32 if n % 32 == 0 else 0)
    Qd = torch.full((3, ldq), SENTINEL, dtype=F64, device=dev())
    ubuf, u = guarded(n)
    al, bt = scal(SENTINEL), scal(SENTINEL)
    call("dsea_plz_finish", ws.handle, P_(rd), P_(yd), P_(pair), P_(Qd[1]), 1, P_(u), P_(al), P_(bt) if with_beta else None, n)
    return Qd, ubuf, al, bt


def check_plz_finish(n):
    ws = ws_of(n)
    r, y = vec(n, 7100 + n % 997), vec(n, 7200 + n % 997)
    pair0, pair1 = 1.7 * float(r @ r) + 0.1, -0.3 * float(r @ y) + 0.2
    rd, yd, pair = D(r), D(y), scal(pair0, pair1)
    q, uw, alpha, beta = pr.ref_plz_finish(r, y, pair0, pair1)
    for with_beta in (True, False):
        Qd, ubuf, al, bt = run_plz_finish(ws, n, rd, yd, pair, with_beta)
        Qh = Qd.cpu()
        assert torch.equal(Qh[1, :n], q) and torch.equal(ubuf[:n].cpu(), uw), (n, with_beta)
        assert bool((Qh[1, n:] == SENTINEL).all()) and bool((Qh[0] == SENTINEL).all()) and bool((Qh[2] == SENTINEL).all())
        assert tail_ok(ubuf, n)
        assert float(al[0]) == alpha and float(bt[0]) == (beta if with_beta else SENTINEL), (n, with_beta)
    assert torch.equal(rd.cpu(), r) and torch.equal(yd.cpu(), y) and torch.equal(pair.cpu(), torch.tensor([pair0, pair1], dtype=F64))


@pytest.mark.parametrize("n", VSIZES)
def test_plz_finish(n):
    """q = r / sqrt(pair0) into row 1 of a sentinel-filled basis only, u = y / sqrt(pair0), alpha = pair1 / pair0,
    beta = sqrt(pair0) (nullable): bit for bit"""
    check_plz_finish(n)


# ------------------------------------------------------------------------------------------------ once per phase: 2^22 + 6 rows
@pytest.mark.parametrize("phase", ["dsea_plz_dots", "dsea_plz_correct", "dsea_axpy_multi_dot", "dsea_plz_finish"])
def test_grid_wrap_at_4194310_rows(phase):
    """(dsea_lanczos_form_r has this size in its own list)"""
    if phase == "dsea_plz_dots":
        check_plz_dots(BIG, 2, [("rpl", 0)])
    elif phase == "dsea_plz_correct":
        check_plz_correct(BIG, 2, [("split", -1)])
    elif phase == "dsea_axpy_multi_dot":
        check_axpy_multi_dot(BIG, (2,))
    else:
        check_plz_finish(BIG)


# ------------------------------------------------------------------------------------------------ determinism
def test_every_phase_twice_gives_the_same_bits():
    n, i = 100000, 5
    ws = ws_of(n)
    Q, ldq = padded_basis(i, n, 8100)
    Qd, ud, cd = D(Q), D(vec(n, 8101)), D(vec(i, 8102))
    r0, y0 = vec(n, 8103), vec(n, 8104)
    xs_d = [D(vec(n, 8110 + j)) for j in range(3)]
    xT = D(vec(8 * 12500, 8120))
    pair = scal(float(r0 @ r0), 0.3)

    def flip():
        zbuf, z = guarded(xT.numel())
        call("dsea_hypercube_flipsum", P_(xT), P_(z), 8, 12500)
        return (zbuf,)

    def correct_matvec():
        be, _, m = stencil_slab(n)
        rbuf, r = guarded(m, r0)
        ybuf, y = guarded(m)
        pr2 = scal(0.0, SENTINEL)
        be.reserve(8)
        be.plz_correct_matvec(Qd, ldq, i, cd, r, y, pr2)
        return rbuf, ybuf, pr2

    phases = {"dsea_lanczos_form_r": lambda: run_form_r(n, Qd, ldq, ud, i, True, True),
              "dsea_hypercube_flipsum": flip,
              "dsea_plz_dots": lambda: run_plz_dots(ws, n, Qd, ldq, ud, i, True),
              "dsea_plz_correct": lambda: run_plz_correct(ws, n, Qd, ldq, i, cd, r0),
              "dsea_plz_correct_matvec": correct_matvec,
              "dsea_axpy_multi_dot": lambda: run_axpy_multi_dot(ws, n, xs_d, 3, scal(A_DEV), scal(SHIFT), None, ud, y0),
              "dsea_plz_finish": lambda: run_plz_finish(ws, n, D(r0), D(y0), pair, True)}
    for name, run in phases.items():
        first, second = run(), run()
        for a, b in zip(first, second):
            assert torch.equal(a, b), name


# ------------------------------------------------------------------------------------------------ lockstep: several slabs, one process
def native_lanczos(op, n, k, q0):
    """dsea_lanczos_run on the whole operator: (Q (k, n), alphas, betas) on the host"""
    lib, st = _lib.load(), _stream(dev())
    ws = Workspace.get(n, max(k, 8), dev())
    _lib.check(lib.dsea_ws_set_reorth_passes(ws.handle, 1), "dsea_ws_set_reorth_passes")
    _lib.check(lib.dsea_ws_set_partial_reorth(ws.handle, 0, 0.0), "dsea_ws_set_partial_reorth")
    ws.reorth_passes, ws.partial_reorth = 1, None
    ldq = round_up(n, 32)
    Q = torch.zeros((k, ldq), dtype=F64, device=dev())
    alphas, betas = torch.zeros(k, dtype=F64, device=dev()), torch.zeros(max(k - 1, 1), dtype=F64, device=dev())
    _lib.check(lib.dsea_lanczos_run(op.handle, ws.handle, k, P_(D(q0)), P_(Q), ldq, P_(alphas), P_(betas), st), "dsea_lanczos_run")
    brk = c_int(0)
    lib.dsea_lanczos_status(ws.handle, byref(brk), st)
    return Q[:, :n].cpu(), alphas.cpu(), betas.cpu()


@pytest.mark.parametrize("kind,size,part", pr.lockstep_cases())
def test_lockstep_ranks_match_the_oracle(kind, size, part):
    """The four-phase step composed as the header prescribes for P virtual ranks in this process (host-summed all-reduce,
    torch-copy exchange: pairwise at P = 2 and where a slab has fewer rows than there are ranks, transposed through
    dsea_hypercube_flipsum otherwise): every step against oracle.lanczos_tridiag on the full operator, then 20 iterations of
    the shifted CG against oracle.cg_solve, iterate for iterate.  P = 1 also against dsea_lanczos_run."""
    run = pr.make_lockstep(kind, size, part, lambda m: HipBackend(m, dev()))
    Q, alphas, betas = pr.check_lockstep_lanczos(run, kind, size)
    if run.P == 1:
        k, valid = min(run.n, 30), Q.shape[0]
        Qn, an, bn = native_lanczos(run.bes[0].op, run.n, k, vec(run.n, pr.LANCZOS_SEED))
        scale = float(alphas.abs().max())
        assert float((an[:valid] - alphas).abs().max()) <= pr.TOL * scale
        assert float((bn[:valid - 1] - betas).abs().max()) <= pr.TOL * scale
        head = min(valid, 24)
        assert float((Qn[:head] - Q[:head]).abs().max()) <= pr.TOL
    pr.check_lockstep_cg(run, kind, size)


# ------------------------------------------------------------------------------------------------ contract with the test double
@pytest.mark.parametrize("n", [3, 129, 1000])
def test_the_cpu_test_double_keeps_the_contract_of_the_hip_backend(n):
    """tests/cpu_backend.CpuBackend claims the phase semantics of include/dsea.h; the same inputs go to it and to HipBackend.
    Element-wise outputs: 4 ulp; reductions: 1e-13 x operand norms."""
    hip, cpu = HipBackend(n, dev()), CpuBackend(n)
    hip.reserve(8)
    Q, ldq = padded_basis(6, n, 9100 + n)
    u, r0, y0 = vec(n, 9101 + n), vec(n, 9102 + n), vec(n, 9103 + n)
    a, b, c = torch.tensor([ALPHA], dtype=F64), torch.tensor([BETA], dtype=F64), vec(6, 9104) * 0.1
    qnorm = float(Q[:, :n].norm(dim=1).max())

    def both(method, make_args):
        """call ``method`` on both backends with freshly built arguments; returns the two argument lists (host copies)"""
        outs = []
        for be, to in ((cpu, lambda t: t), (hip, D)):
            args = [to(v.clone()) if torch.is_tensor(v) else ([to(w.clone()) for w in v] if isinstance(v, list) else v)
                    for v in make_args()]
            getattr(be, method)(*args)
            outs.append([v.cpu() if torch.is_tensor(v) else v for v in args])
        return outs

    # form_r and plz_dots: i = 1 ignores beta on BOTH sides; r_copy given and null
    for i, beta, copy in ((1, b, True), (1, None, False), (2, b, True), (5, b, False), (5, None, True)):
        oc, oh = both("form_r", lambda: [Q, ldq, n, i, u, a, beta, torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64) if copy else None])
        assert ulp_distance(oc[7], oh[7]) <= 4 and (not copy or ulp_distance(oc[8], oh[8]) <= 4), ("form_r", i)
        assert torch.equal(oh[0], Q)                        # the sentinel padding came back untouched
        if i == 1:
            assert torch.equal(oc[7], pr.ref_form_r(Q, n, 1, u, ALPHA, None)) and torch.equal(oh[7], oc[7])
        oc, oh = both("plz_dots", lambda: [Q, ldq, n, i, u, a, beta, torch.zeros(n, dtype=F64), torch.zeros(i + 1, dtype=F64)])
        assert ulp_distance(oc[7], oh[7]) <= 4, ("plz_dots", i)
        assert float((oc[8] - oh[8])[:i].abs().max()) <= 1e-13 * float(oc[7].norm()) * qnorm
        assert abs(float(oc[8][i] - oh[8][i])) <= 1e-13 * float(oc[7] @ oc[7])
    # plz_correct: row = 0 leaves r alone on BOTH sides
    for row in (0, 5):
        oc, oh = both("plz_correct", lambda: [Q, ldq, n, row, c, r0, torch.zeros(2, dtype=F64)])
        if row == 0:
            assert torch.equal(oc[5], r0) and torch.equal(oh[5], r0)
        assert float((oc[5] - oh[5]).abs().max()) <= 1e-13 * float(r0.norm() + c.norm() * qnorm)
        assert abs(float(oc[6][0] - oh[6][0])) <= 1e-13 * float(oc[5] @ oc[5])
    # flipsum: the double adds in the header's order
    for P in (1, 4):
        oc, oh = both("flipsum", lambda: [vec(P * n, 9200 + P), torch.zeros(P * n, dtype=F64), P])
        assert ulp_distance(oc[1], oh[1]) <= 4, ("flipsum", P)
    # axpy_multi_dot.  The double adds a*t term by term where the kernel sums the sources first, so 1 ulp cannot be
    # demanded: with positive data (no cancellation: every rounding error is at most half an ulp of the RESULT) the kernel makes
    # three roundings, one of them scaled by a, the double four -- at most 4 ulp apart.  One source: the same operations.
    pos = [vec(n, 9300 + j).abs() + 0.5 for j in range(4)]
    g = torch.tensor([A_DEV], dtype=F64)
    oc, oh = both("axpy_multi_dot", lambda: [3.0, g, pos[:2], None, None, pos[2], pos[3], torch.zeros(1, dtype=F64)])
    assert ulp_distance(oc[6], oh[6]) <= 4
    assert abs(float(oc[7] - oh[7])) <= 1e-13 * float(oc[5].norm() * oc[6].norm())
    sh = torch.tensor([SHIFT], dtype=F64)
    oc, oh = both("axpy_multi_dot", lambda: [A_HOST, g, [u], sh, torch.zeros(1, dtype=F64), r0, y0, torch.zeros(1, dtype=F64)])
    assert ulp_distance(oc[6], oh[6]) <= 4
    assert abs(float(oc[7] - oh[7])) <= 1e-13 * float(oc[5].norm() * oc[6].norm())
    oc, oh = both("axpy_multi_dot", lambda: [A_HOST, g, [u], sh, torch.ones(1, dtype=F64), r0, y0, torch.full((1,), SENTINEL, dtype=F64)])
    for o in (oc, oh):
        assert torch.equal(o[6], y0) and float(o[7]) == SENTINEL
    # plz_finish (q_out is row 2 of a basis)
    pair = torch.tensor([float(r0 @ r0), 0.3], dtype=F64)

    def finish_args():
        return [r0, y0, pair, torch.full((ldq,), SENTINEL, dtype=F64), 2, torch.zeros(n, dtype=F64), torch.zeros(1, dtype=F64),
                torch.zeros(1, dtype=F64)]
    oc, oh = both("plz_finish", finish_args)
    for k_ in (3, 5, 6, 7):
        assert ulp_distance(oc[k_], oh[k_]) <= 4, ("plz_finish", k_)
    assert bool((oh[3][n:] == SENTINEL).all())
    # plz_correct_matvec on a stencil slab with both halos
    V, halo, coef = pr.stencil_potential(n), torch.tensor([0.7, -0.4], dtype=F64), -0.5 * n * n
    cpu.attach_stencil(n, coef, V, halo, True, True)
    keep = (D(V), D(halo))
    hip.attach_stencil(n, coef, keep[0], keep[1], True, True)
    for row in (0, 5):
        oc, oh = both("plz_correct_matvec", lambda: [Q, ldq, row, c, r0, torch.zeros(n, dtype=F64), torch.zeros(2, dtype=F64)])
        assert float((oc[4] - oh[4]).abs().max()) <= 1e-13 * float(r0.norm() + c.norm() * qnorm)
        assert float((oc[5] - oh[5]).abs().max()) <= 1e-13 * (4 * abs(coef) + 1.0) * float(oc[4].abs().max() + 1.0)
        assert abs(float(oc[6][0] - oh[6][0])) <= 1e-13 * float(oc[4] @ oc[4])
