"""The bf16 storage shadow of the Krylov basis (docs/design/05-bf16-shadow.md), tested directly: every READER against a
longdouble evaluation of  r - sum_j c_j bf16_value(Qs[j])  with O(1) coefficients and a shadow that has nothing to do with the
fp64 basis, every WRITER bit for bit against  bf16_bits(the fp64 row it stored)  (tests/helpers.py: plain numpy integers,
pinned against torch in tests/test_shadow_reference_cpu.py).

Tolerances are derived, not measured.  Per row the kernels do i fp64 FMAs and one subtraction, the split form 15 more
additions in wave order: |r_gpu - r_ref| <= (i + 18) 2^-53 S with S = |r| + sum_j |c_j| |qs_j|, asserted element-wise (the
products c_j qs_j are exact in longdouble: 53 x 8 bits).  ||r||^2: 1e-12 relative against the longdouble norm of the kernel's
own output (the bound tests/test_gpu_kernels.py::test_reorth_pair uses for this quantity).  Each test prints its largest
error / bound as a SHADOW-RATIO line.

Not reached from here: the shadow READER of the mid-size single-launch kernel (csrc/dsea_lanczos_persist_mid.hip); its
coefficients exist only inside a run, where they are rounding residue.  Its writer is covered below."""
import ctypes
from ctypes import byref, c_int64, c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dominantsparseeigenad_amd import _lib, engine  # noqa: E402
from dominantsparseeigenad_amd.engine import Workspace, _ptr, _stream, round_up  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402
from helpers import bf16_bits, bf16_chosen_values, bf16_value  # noqa: E402

F64 = torch.float64
LD = np.longdouble
SENTINEL = 0x7FC0            # a bf16 NaN: whatever streams it by mistake turns the result into NaN
EPS = 2.0 ** -53


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


def lp_stats(ws):
    a, b = c_int64(0), c_int64(0)
    _lib.check(_lib.load().dsea_lanczos_lp_stats(ws.handle, byref(a), byref(b), _stream(dev())), "dsea_lanczos_lp_stats")
    return a.value, b.value


def shadow_ld(n, differs):
    return round_up(n, 8) + 8 if differs else round_up(n, 32)


def sentinel_buffer(rows, lds):
    return torch.full((rows, lds), SENTINEL, dtype=torch.int16, device=dev())


def host_u16(t):
    return t.contiguous().cpu().numpy().view(np.uint16)


class Registered:
    """``dsea_ws_set_shadow(ws, Qs, lds, rows, tau)`` for the duration of a with-block"""

    def __init__(self, ws, Qs, lds, rows, tau):
        self.args = (ws, Qs, int(lds), int(rows), float(tau))

    def __enter__(self):
        ws, Qs, lds, rows, tau = self.args
        _lib.check(_lib.load().dsea_ws_set_shadow(ws.handle, _ptr(Qs), lds, rows, tau), "dsea_ws_set_shadow")

    def __exit__(self, *exc):
        _lib.check(_lib.load().dsea_ws_set_shadow(self.args[0].handle, None, 0, 0, 0.0), "dsea_ws_set_shadow")


# ------------------------------------------------------------------------------------------------------------ readers
class ReaderInputs:
    """Q (i x ldq fp64) and Qs (rows x lds bf16) drawn INDEPENDENTLY of each other, rows > i; the padding columns of both and
    the shadow rows >= i hold NaN; O(1) coefficients c[0..i), c[i] = r.r."""

    def __init__(self, n, i, differs, seed):
        gen = torch.Generator(device=dev()).manual_seed(seed)
        self.n, self.i = n, i
        self.ldq, self.lds, self.rows = round_up(n, 32), shadow_ld(n, differs), i + 2
        self.Q = torch.full((i, self.ldq), float("nan"), dtype=F64, device=dev())
        self.Q[:, :n] = torch.randn((i, n), generator=gen, device=dev(), dtype=F64)
        self.Qs = sentinel_buffer(self.rows, self.lds)
        self.Qs[:i, :n] = torch.randn((i, n), generator=gen, device=dev(), dtype=torch.float32).to(torch.bfloat16).view(torch.int16)
        self.r0 = torch.randn(n, generator=gen, device=dev(), dtype=F64)
        self.c = torch.randn(i + 1, generator=gen, device=dev(), dtype=F64)
        self.c[i] = torch.dot(self.r0, self.r0)
        self.Qs_before = self.Qs.clone()

    def reference(self, which):
        """(r_ref, S) in longdouble from the shadow values ("shadow") or from the fp64 basis ("fp64")"""
        r0, c = self.r0.cpu().numpy(), self.c.cpu().numpy()
        acc, S = r0.astype(LD), np.abs(r0).astype(LD)
        for j in range(self.i):
            if which == "shadow":
                v = bf16_value(host_u16(self.Qs_before[j, :self.n])).astype(LD)
            else:
                v = self.Q[j, :self.n].cpu().numpy().astype(LD)
            acc -= LD(c[j]) * v
            S += abs(LD(c[j])) * np.abs(v)
        return acc, S

    def run(self, ws, tau):
        """one dsea_lanczos_axpy_norm on a fresh copy of r with the shadow registered; (r, nrm2, stats advance)"""
        lib = _lib.load()
        r = self.r0.clone()
        nrm2 = torch.zeros(1, dtype=F64, device=dev())
        with Registered(ws, self.Qs, self.lds, self.rows, tau):
            before = lp_stats(ws)
            _lib.check(lib.dsea_lanczos_axpy_norm(ws.handle, _ptr(self.Q), self.ldq, self.n, self.i, _ptr(self.c), _ptr(r),
                                                  _ptr(nrm2), _stream(dev())), "dsea_lanczos_axpy_norm")
            after = lp_stats(ws)
        assert torch.equal(self.Qs, self.Qs_before)          # a reader does not write
        return r, nrm2, (after[0] - before[0], after[1] - before[1])

    def check(self, r, nrm2, which, label):
        r_ref, S = self.reference(which)
        r_gpu = r.cpu().numpy()
        assert np.all(np.isfinite(r_gpu)), "%s: NaN padding or a sentinel row reached the result" % label
        bound = (self.i + 18) * EPS * S                      # element-wise (module docstring)
        err = np.abs(r_gpu.astype(LD) - r_ref)
        ratio_r = float(np.max(err / bound))
        g2 = float(np.sum(r_gpu.astype(LD) ** 2))
        ref2 = float(np.sum(r_ref ** 2))
        got = float(nrm2.item())
        tol_ref = 1e-12 * ref2 + 2.0 * float(np.sqrt(ref2)) * float(np.sqrt(np.sum(bound ** 2)))
        print("SHADOW-RATIO %s n=%d i=%d lds=%d ldq=%d: r %.3f  nrm2/own %.3e  nrm2/ref %.3e"
              % (label, self.n, self.i, self.lds, self.ldq, ratio_r, abs(got - g2) / (1e-12 * g2), abs(got - ref2) / tol_ref))
        rows_off = np.nonzero(err > bound)[0]
        assert rows_off.size == 0, "%s: %d rows beyond (i + 18) 2^-53 S, first %s, worst ratio %.3g" % (
            label, rows_off.size, rows_off[:8], ratio_r)
        assert abs(got - g2) <= 1e-12 * g2, label
        assert abs(got - ref2) <= tol_ref, label


def _forced_split_cases():
    table = [((1, 7, 8, 9), (1, 3, 7, 9, 129)),
             ((511, 512, 513), (1, 8, 9, 129)),
             ((1000, 4097), (1, 9, 127, 128, 129)),          # 16 waves x 8 vectors per sweep
             ((100000,), (1, 9, 129, 201))]
    cases = [(n, i) for ns, iis in table for n in ns for i in iis]
    return [(n, i, idx % 3 != 0) for idx, (n, i) in enumerate(cases)]


@pytest.mark.parametrize("n,i,differs", _forced_split_cases())
def test_split_reader_forced_at_small_n(n, i, differs):
    """k_axpy_norm_lp_split<16> at sizes where the automatic geometry would not stream the shadow: partial octets (n not a
    multiple of 8), partial 512-row tiles, chunk remainders (i not a multiple of 8), fewer chunks than waves and more."""
    ws = Workspace.get(n, max(i, 8), dev())
    ws.set_split(0)
    try:
        inp = ReaderInputs(n, i, differs, 7000 + 13 * n + i)
        r, nrm2, adv = inp.run(ws, 1e6)
        assert adv == (1, 0)
        inp.check(r, nrm2, "shadow", "split-forced")
    finally:
        ws.set_split(-1)


_P20 = 1 << 20
_AUTO = [(n, i) for n in (_P20 - 3, _P20, _P20 + 5, _P20 + 1029) for i in (1, 2, 3, 4, 5, 23)] + \
        [((1 << 18) + 6, i) for i in (1, 9, 129)] + [((1 << 23) + 3 * 1024 + 5, 2)]


@pytest.mark.parametrize("n,i,differs", [(n, i, idx % 2 == 0) for idx, (n, i) in enumerate(_AUTO)])
def test_reader_automatic_geometry(n, i, differs):
    """What the phase API picks by itself: the split form below 2^20 rows (2^18 + 6, 2^20 - 3), k_axpy_norm_lp<2> from 2^20
    rows on -- exact tiles, a partial octet, a partial and a whole extra 1024-row tile, the unroll-4 remainder of the vector
    loop, and more tiles than DSEA_MAX_WAVE_TILES (waves walk two tiles)."""
    ws = Workspace.get(n, max(i, 8), dev())
    inp = ReaderInputs(n, i, differs, 8000 + (n % 9973) + i)
    r, nrm2, adv = inp.run(ws, 1e6)
    assert adv == (1, 0)
    inp.check(r, nrm2, "shadow", "auto")


@pytest.mark.parametrize("n,i,split0", [(4097, 9, True), ((1 << 18) + 6, 9, False), (_P20 + 5, 5, False)])
def test_reader_fallback_decision(n, i, split0):
    """The device-side premise max c_j^2 <= tau^2 ||r||^2 decides between two O(1)-different results (Qs is unrelated to Q):
    tau = 0 and tau^2 ||r||^2 = max c_j^2 / 4 give the fp64 formula on Q, tau^2 ||r||^2 = 4 max c_j^2 the shadow formula;
    dsea_lanczos_lp_stats advances by exactly one on the matching side."""
    ws = Workspace.get(n, max(i, 8), dev())
    if split0:
        ws.set_split(0)
    try:
        inp = ReaderInputs(n, i, True, 9000 + n % 9973)
        c = inp.c.cpu().numpy()
        cmax2, rr = float(np.max(c[:i] ** 2)), float(c[i])
        for tau, which, want in ((0.0, "fp64", (0, 1)), (np.sqrt(0.25 * cmax2 / rr), "fp64", (0, 1)),
                                 (np.sqrt(4.0 * cmax2 / rr), "shadow", (1, 0))):
            r, nrm2, adv = inp.run(ws, tau)
            assert adv == want, (tau, adv)
            inp.check(r, nrm2, which, "decision tau=%.3g" % tau)
    finally:
        ws.set_split(-1)


@pytest.mark.parametrize("n,i,split0", [(100000, 23, True), (_P20 + 5, 23, False)])
def test_reader_is_deterministic(n, i, split0):
    ws = Workspace.get(n, max(i, 8), dev())
    if split0:
        ws.set_split(0)
    try:
        inp = ReaderInputs(n, i, True, 9500 + n % 9973)
        r1, n1, adv1 = inp.run(ws, 1e6)
        r2, n2, adv2 = inp.run(ws, 1e6)
        assert adv1 == adv2 == (1, 0)
        assert torch.equal(r1, r2) and torch.equal(n1, n2)
    finally:
        ws.set_split(-1)


# ------------------------------------------------------------------------------------------------------------ writers
def assert_shadow_rows(Q, Qs, n, written, label):
    """rows in ``written``: Qs[j, :n] == bf16_bits(Q[j, :n]); everything else in the buffer still holds the sentinel"""
    sent = torch.tensor(SENTINEL, dtype=torch.int16, device=Qs.device)
    assert bool((Qs[:, n:] == sent).all()), "%s: a padding column [n, lds) was written" % label
    untouched = [j for j in range(Qs.shape[0]) if j not in set(written)]
    if untouched:
        assert bool((Qs[untouched, :n] == sent).all()), "%s: a row outside %s was written" % (label, list(written)[:4])
    for j in written:
        want = bf16_bits(Q[j, :n].cpu().numpy())
        got = host_u16(Qs[j, :n])
        bad = np.nonzero(want != got)[0]
        assert bad.size == 0, "%s: row %d, %d elements differ, first at column %d: stored 0x%04x, bf16_bits gives 0x%04x" % (
            label, j, bad.size, bad[0], got[bad[0]], want[bad[0]])


def chosen_vector(n, seed):
    """normal draws over 40 binades with the chosen values of tests/helpers.py mixed in (first and last element included)"""
    rng = np.random.RandomState(seed)
    v = rng.randn(n) * np.exp2(rng.randint(-20, 20, size=n).astype(np.float64))
    chosen = bf16_chosen_values()
    m = min(n, 4 * chosen.size)
    pos = rng.permutation(n)[:m]
    if n - 1 not in pos:
        pos[0] = n - 1
    v[pos] = chosen[(seed + np.arange(m)) % chosen.size]
    return v


@pytest.mark.parametrize("call", ["dsea_lanczos_store", "dsea_plz_finish"])
@pytest.mark.parametrize("n", [1, 2, 3, 9, 1000, 4097, (1 << 18) + 7])
def test_phase_call_writers_bit_for_bit(n, call):
    """k_scale_store / k_plz_finish with ||r||^2 = 1 (beta = 1: the chosen values reach the conversion unchanged): ties,
    the two-step rounding, the carry into the exponent, fp32 subnormals, signed zeros; rows 0, 1, rows - 1; a row index at or
    beyond the registered row count leaves the shadow alone."""
    lib, st = _lib.load(), _stream(dev())
    ws = Workspace.get(n, 8, dev())
    rows, ldq = 4, round_up(n, 32)
    one = torch.tensor([1.0, 0.3], dtype=F64, device=dev())             # ||r||^2 (and r.Ar for dsea_plz_finish)
    for case, row in enumerate((0, 1, rows - 1, rows, rows + 1)):
        lds = shadow_ld(n, case % 2 == 0)
        Q = torch.zeros((rows + 2, ldq), dtype=F64, device=dev())
        Qs = sentinel_buffer(rows + 2, lds)
        r = torch.from_numpy(chosen_vector(n, 31 * n + row)).to(dev())
        with Registered(ws, Qs, lds, rows, 1e-12):
            if call == "dsea_lanczos_store":
                _lib.check(lib.dsea_lanczos_store(ws.handle, _ptr(r), _ptr(one), _ptr(Q), ldq, row, None, n, st), call)
            else:
                y = torch.from_numpy(normal_vector(n, 77)).to(dev())
                u, ab = torch.empty(n, dtype=F64, device=dev()), torch.zeros(2, dtype=F64, device=dev())
                _lib.check(lib.dsea_plz_finish(ws.handle, _ptr(r), _ptr(y), _ptr(one), c_void_p(Q[row].data_ptr()), row, _ptr(u),
                                               _ptr(ab), c_void_p(ab.data_ptr() + 8), n, st), call)
        assert_shadow_rows(Q, Qs, n, [row] if row < rows else [], "%s n=%d row=%d lds=%d" % (call, n, row, lds))
        if row < rows:      # the chosen values did reach the shadow: both zeros, a subnormal, the tie that goes down
            got = set(host_u16(Qs[row, :n]).tolist())
            assert n < 1000 or {0x0000, 0x8000, 0x0001, 0x3F80, 0x3F82, 0x4000} <= got


def run_native(op, n, k, differs, persist=-1):
    """dsea_lanczos_run on the test's own Q, Qs (k + 1 rows, k registered) and lds; returns (Q, Qs, stats)"""
    lib, st = _lib.load(), _stream(dev())
    ws = Workspace.get(n, k, dev())
    # full re-orthogonalisation in one pass, whatever an earlier solve left on this cached workspace
    _lib.check(lib.dsea_ws_set_reorth_passes(ws.handle, 1), "dsea_ws_set_reorth_passes")
    _lib.check(lib.dsea_ws_set_partial_reorth(ws.handle, 0, 0.0), "dsea_ws_set_partial_reorth")
    ws.reorth_passes, ws.partial_reorth = 1, None
    ldq, lds = round_up(n, 32), shadow_ld(n, differs)
    Q = torch.zeros((k, ldq), dtype=F64, device=dev())
    Qs = sentinel_buffer(k + 1, lds)
    alphas = torch.empty(k, dtype=F64, device=dev())
    betas = torch.empty(max(k - 1, 1), dtype=F64, device=dev())
    q0 = torch.from_numpy(normal_vector(n, 4300 + k)).to(dev())
    brk = ctypes.c_int(0)
    ws.set_lanczos_persist(persist)
    try:
        with Registered(ws, Qs, lds, k, engine.SHADOW_TAU):
            _lib.check(lib.dsea_lanczos_run(op.handle, ws.handle, k, _ptr(q0), _ptr(Q), ldq, _ptr(alphas), _ptr(betas), st),
                       "dsea_lanczos_run")
            _lib.check(lib.dsea_lanczos_status(ws.handle, byref(brk), st), "dsea_lanczos_status")
            stats = lp_stats(ws)
    finally:
        ws.set_lanczos_persist(-1)
    assert brk.value == 0
    assert bool(torch.isfinite(alphas).all()) and bool(torch.isfinite(betas).all())
    return Q, Qs, stats


def check_native(op, n, k, differs, label, persist=-1, takes_shadow=True):
    Q, Qs, stats = run_native(op, n, k, differs, persist)
    if takes_shadow:
        assert stats == (k - 1, 0), (label, stats)
        assert_shadow_rows(Q, Qs, n, range(k), label)
    else:
        assert stats == (0, 0), (label, stats)
        assert_shadow_rows(Q, Qs, n, [], label)


def tfim(L):
    from dominantsparseeigenad_amd.operators import TFIMOperator
    return TFIMOperator(L, dev(), g=torch.tensor([1.0], dtype=F64, device=dev()))


@pytest.mark.parametrize("L,differs,takes", [(15, False, True), (15, True, True), (14, True, False), (18, True, True),
                                              (20, False, True)])
def test_tfim_run_writes_the_shadow_bit_for_bit(L, differs, takes):
    """launch_scale_store (row 0) and the fused tail of the TFIM mat-vec (rows 1..k-1): L = 15 is the lower edge of the
    n >= 32768 rule (split shadow form), L = 14 must leave a registered shadow alone, L = 18 / 20 the large geometries."""
    check_native(tfim(L), 1 << L, 24, differs, "TFIM L=%d" % L, takes_shadow=takes)


@pytest.mark.parametrize("variant", ["sell16v8", "sell16p2", "sell16", "sell"])
def test_sell_run_writes_the_shadow_bit_for_bit(monkeypatch, variant):
    """the explicit TFIM matrix (L = 15: takes the shadow) in every SELL operand the library builds -- value-coded, 16-bit
    columns packed two to a lane, 16-bit columns, 32-bit columns: the fused tails of their mat-vec kernels"""
    L = 15
    if variant == "sell16":
        monkeypatch.setenv("DSEA_SELL_PACK2", "0")
    op = tfim(L).to_csr(layout="sell", col16=False if variant == "sell" else "auto",
                        values="coded" if variant == "sell16v8" else "plain")
    built = ("sell16v8" if op._coded else "sell16p2" if getattr(op, "_pack2", False) else "sell16" if op.col16 else "sell")
    assert built == variant
    check_native(op, 1 << L, 24, variant in ("sell16p2", "sell"), "TFIM as %s" % variant)


def test_csr_run_writes_the_shadow_bit_for_bit():
    """plain CSR operand (no fused tail: launch_scale_store on every row) at a ragged n"""
    import scipy.sparse as sp
    from dominantsparseeigenad_amd.operators import CSROperator
    n = 40037
    rng = np.random.RandomState(5)
    off = rng.randn(n - 1) * 0.4
    M = sp.diags([rng.rand(n) + 1.0, off, off], [0, 1, -1], format="csr")
    check_native(CSROperator.from_scipy(M, dev(), layout="csr"), n, 24, True, "CSR n=%d" % n)


def stencil(n):
    from dominantsparseeigenad_amd.operators import Stencil3Operator
    x = torch.linspace(-1.0, 1.0, n, dtype=F64, device=dev())
    return Stencil3Operator(n, 1.0, 0.5 * x * x + 0.1 * torch.from_numpy(normal_vector(n, 66)).to(dev()).abs())


@pytest.mark.parametrize("n,k,persist,differs", [(40000, 24, -1, False), (100000, 200, -1, True), (100000, 200, 0, False)])
def test_stencil_run_writes_the_shadow_bit_for_bit(n, k, persist, differs):
    """3-point stencil: the fused tail of the multi-launch step (N = 40000; N = 100000 with the single-launch form off) and the
    writer of the mid-size single-launch kernel (N = 100000, automatic: k = 200 streams most of the basis)."""
    check_native(stencil(n), n, k, differs, "stencil N=%d persist=%d" % (n, persist), persist=persist)


def test_callable_step_writes_the_shadow_bit_for_bit():
    """dsea_lanczos_store (row 0) + dsea_lanczos_callable_step's fused normalise-and-store (rows 1..k-1) around a caller's
    mat-vec at n = 2^20, k = 8, the shadow registered on the workspace directly (engine.lanczos keeps its own to itself)."""
    lib, st = _lib.load(), _stream(dev())
    L, k = 20, 8
    n = 1 << L
    op = tfim(L)
    ws = Workspace.get(n, k, dev())
    ldq, lds = round_up(n, 32), shadow_ld(n, True)
    Q = torch.zeros((k, ldq), dtype=F64, device=dev())
    Qs = sentinel_buffer(k + 1, lds)
    alphas, betas = torch.empty(k, dtype=F64, device=dev()), torch.empty(k - 1, dtype=F64, device=dev())
    q0 = torch.from_numpy(normal_vector(n, 4400)).to(dev())
    nrm2, r = torch.zeros(1, dtype=F64, device=dev()), torch.empty(n, dtype=F64, device=dev())
    with Registered(ws, Qs, lds, k, engine.SHADOW_TAU):
        before = lp_stats(ws)
        _lib.check(lib.dsea_nrm2sq(ws.handle, _ptr(q0), n, _ptr(nrm2), st), "dsea_nrm2sq")
        _lib.check(lib.dsea_lanczos_store(ws.handle, _ptr(q0), _ptr(nrm2), _ptr(Q), ldq, 0, None, n, st), "dsea_lanczos_store")
        u = engine.as_vector(op.H(Q[0, :n]), n)
        _lib.check(lib.dsea_lanczos_callable_alpha(ws.handle, _ptr(Q), _ptr(u), n, None, st), "dsea_lanczos_callable_alpha")
        for i in range(1, k):
            _lib.check(lib.dsea_lanczos_callable_step(ws.handle, _ptr(Q), ldq, n, i, _ptr(u), _ptr(alphas), _ptr(betas), _ptr(r),
                                                      st), "dsea_lanczos_callable_step")
            u = engine.as_vector(op.H(Q[i, :n]), n)
            last = c_void_p(alphas.data_ptr() + 8 * i) if i == k - 1 else None
            _lib.check(lib.dsea_lanczos_callable_alpha(ws.handle, _ptr(Q[i]), _ptr(u), n, last, st), "dsea_lanczos_callable_alpha")
        after = lp_stats(ws)
    assert (after[0] - before[0], after[1] - before[1]) == (k - 1, 0)
    assert bool(torch.isfinite(alphas).all()) and bool(torch.isfinite(betas).all())
    assert_shadow_rows(Q, Qs, n, range(k), "callable step")
