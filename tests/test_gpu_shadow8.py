"""The 8-bit storage shadow of the Krylov basis (docs/design/15-shadow8.md), tested directly like the bf16 one
(tests/test_gpu_shadow.py): the READER k_axpy_norm_lp8 against a longdouble evaluation of  r - sum_j c_j dec(code_j) / S  with
O(1) coefficients and codes that have nothing to do with the fp64 basis, every WRITER bit for bit against
e5m2_bits(the fp64 row it stored * S)  (tests/shadow8_helpers.py, pinned against torch in tests/test_shadow8_reference_cpu.py).

Tolerance of the reader, derived.  With T = sum_j |c_j| |dec(code_j)| / S per row the kernel computes
    chat_j = fl32(c_j cs),  cs = fl64(1 / (S sqrt(c[i])))           relative error <= 2^-24 + 3 2^-53 per term
    w      = i fused fp32 multiply-adds, j downwards                each rounds a partial sum <= T / sqrt(c[i]): <= i 2^-24 in all
    r_k   -= fl64(w) sqrt(c[i])                                     one fp64 FMA: 2^-53 (|r| + T), sqrt and cs: 3 2^-53 T
so |r_gpu - r_ref| <= (i + 1) 2^-24 T (1 + i 2^-24) + 4 2^-53 (|r| + T); the asserted bound is the one the issue states,
    (i + 18) 2^-53 (|r| + T) + (i + 4) 2^-24 T,
whose second term is the fp32 accumulation with a margin of three roundings and whose first term is the bf16 test's.  No
product underflows: |chat_j dec| >= 2^-16 |c_j| / (S sqrt(c[i])) ~ 1e-12 here.  The fp64 fallback is held to the bf16 test's
bound (i + 18) 2^-53 (|r| + sum |c_j| |q_j|).  ||r||^2: 1e-12 relative against the longdouble norm of the kernel's own output."""
import ctypes
from ctypes import byref, c_int64

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dominantsparseeigenad_amd import _lib, engine  # noqa: E402
from dominantsparseeigenad_amd.engine import Workspace, _ptr, _stream, round_up  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402
from shadow8_helpers import e5m2_bits, e5m2_chosen_values, e5m2_value, shadow8_scale  # noqa: E402

F64 = torch.float64
LD = np.longdouble
SENTINEL = 0x7F              # an e5m2 NaN: whatever streams it by mistake turns the result into NaN
SENTINEL16 = 0x7FC0
EPS, EPS32 = 2.0 ** -53, 2.0 ** -24
_P20 = 1 << 20


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


def lp_stats(ws):
    a, b = c_int64(0), c_int64(0)
    _lib.check(_lib.load().dsea_lanczos_lp_stats(ws.handle, byref(a), byref(b), _stream(dev())), "dsea_lanczos_lp_stats")
    return a.value, b.value


def shadow_ld(n, differs):
    return round_up(n, 16) + 16 if differs else round_up(n, 32)


def sentinel_buffer(rows, ld8):
    return torch.full((rows, ld8), SENTINEL, dtype=torch.uint8, device=dev())


class Registered:
    """``dsea_ws_set_shadow8(ws, Qs8, ld8, rows, tau8)`` for the duration of a with-block"""

    def __init__(self, ws, Qs8, ld8, rows, tau):
        self.args = (ws, Qs8, int(ld8), int(rows), float(tau))

    def __enter__(self):
        ws, Qs8, ld8, rows, tau = self.args
        _lib.check(_lib.load().dsea_ws_set_shadow8(ws.handle, _ptr(Qs8), ld8, rows, tau), "dsea_ws_set_shadow8")

    def __exit__(self, *exc):
        _lib.check(_lib.load().dsea_ws_set_shadow8(self.args[0].handle, None, 0, 0, 0.0), "dsea_ws_set_shadow8")


# ------------------------------------------------------------------------------------------------------------ reader
class ReaderInputs:
    """Q (i x ldq fp64) and Qs8 (rows x ld8 codes) drawn INDEPENDENTLY of each other, rows > i; every finite code occurs
    (uniform bytes, the NaN / infinity patterns folded back); the padding columns of both and the shadow rows >= i hold
    NaN; O(1) coefficients c[0..i), c[i] = r.r."""

    def __init__(self, n, i, differs, seed):
        gen = torch.Generator(device=dev()).manual_seed(seed)
        self.n, self.i = n, i
        self.ldq, self.ld8, self.rows = round_up(n, 32), shadow_ld(n, differs), i + 2
        self.Q = torch.full((i, self.ldq), float("nan"), dtype=F64, device=dev())
        self.Q[:, :n] = torch.randn((i, n), generator=gen, device=dev(), dtype=F64)
        codes = torch.randint(0, 256, (i, n), generator=gen, device=dev(), dtype=torch.int32)
        codes = torch.where((codes & 0x7C) == 0x7C, codes ^ 0x40, codes)
        self.Qs8 = sentinel_buffer(self.rows, self.ld8)
        self.Qs8[:i, :n] = codes.to(torch.uint8)
        self.r0 = torch.randn(n, generator=gen, device=dev(), dtype=F64)
        self.c = torch.randn(i + 1, generator=gen, device=dev(), dtype=F64)
        self.c[i] = torch.dot(self.r0, self.r0)
        self.Qs8_before = self.Qs8.clone()

    def reference(self, which):
        """(r_ref, |r| + T, T) in longdouble from the codes ("shadow") or from the fp64 basis ("fp64")"""
        r0, c = self.r0.cpu().numpy(), self.c.cpu().numpy()
        S = shadow8_scale(self.n)
        acc, T = r0.astype(LD), np.zeros(self.n, dtype=LD)
        for j in range(self.i):
            if which == "shadow":
                v = e5m2_value(self.Qs8_before[j, :self.n].cpu().numpy()).astype(LD) / LD(S)
            else:
                v = self.Q[j, :self.n].cpu().numpy().astype(LD)
            acc -= LD(c[j]) * v
            T += abs(LD(c[j])) * np.abs(v)
        return acc, np.abs(r0).astype(LD) + T, T

    def run(self, ws, tau):
        """one dsea_lanczos_axpy_norm on a fresh copy of r with the shadow registered; (r, nrm2, stats advance)"""
        lib = _lib.load()
        r = self.r0.clone()
        nrm2 = torch.zeros(1, dtype=F64, device=dev())
        with Registered(ws, self.Qs8, self.ld8, self.rows, tau):
            before = lp_stats(ws)
            _lib.check(lib.dsea_lanczos_axpy_norm(ws.handle, _ptr(self.Q), self.ldq, self.n, self.i, _ptr(self.c), _ptr(r),
                                                  _ptr(nrm2), _stream(dev())), "dsea_lanczos_axpy_norm")
            after = lp_stats(ws)
        assert torch.equal(self.Qs8, self.Qs8_before)          # a reader does not write
        return r, nrm2, (after[0] - before[0], after[1] - before[1])

    def check(self, r, nrm2, which, label):
        r_ref, S, T = self.reference(which)
        r_gpu = r.cpu().numpy()
        assert np.all(np.isfinite(r_gpu)), "%s: NaN padding or a sentinel row reached the result" % label
        bound = (self.i + 18) * EPS * S                      # element-wise (module docstring)
        if which == "shadow":
            bound = bound + (self.i + 4) * EPS32 * T
        err = np.abs(r_gpu.astype(LD) - r_ref)
        ratio_r = float(np.max(err / bound))
        g2 = float(np.sum(r_gpu.astype(LD) ** 2))
        ref2 = float(np.sum(r_ref ** 2))
        got = float(nrm2.item())
        tol_ref = 1e-12 * ref2 + 2.0 * float(np.sqrt(ref2)) * float(np.sqrt(np.sum(bound ** 2)))
        print("SHADOW8-RATIO %s n=%d i=%d ld8=%d ldq=%d: r %.3f  nrm2/own %.3e  nrm2/ref %.3e"
              % (label, self.n, self.i, self.ld8, self.ldq, ratio_r, abs(got - g2) / (1e-12 * g2), abs(got - ref2) / tol_ref))
        rows_off = np.nonzero(err > bound)[0]
        assert rows_off.size == 0, "%s: %d rows beyond the bound, first %s, worst ratio %.3g" % (
            label, rows_off.size, rows_off[:8], ratio_r)
        assert abs(got - g2) <= 1e-12 * g2, label
        assert abs(got - ref2) <= tol_ref, label


_SIZES = [(n, i) for n in (_P20 - 3, _P20, _P20 + 5, _P20 + 1029) for i in (1, 2, 7, 8, 9, 23)] + [((1 << 23) + 3 * 1024 + 5, 2)]


@pytest.mark.parametrize("n,i,differs", [(n, i, idx % 2 == 0) for idx, (n, i) in enumerate(_SIZES)])
def test_reader(n, i, differs):
    """k_axpy_norm_lp8 through the phase call: partial 16-row groups (n not a multiple of 16), a partial and a whole extra
    1024-row tile, the unroll-8 remainders of the vector loop, more tiles than DSEA_MAX_WAVE_TILES (waves walk two tiles).
    Below 2^20 rows (2^20 - 3) a registered 8-bit shadow is not read: the pass takes the fp64 basis and counts nothing."""
    ws = Workspace.get(n, max(i, 8), dev())
    inp = ReaderInputs(n, i, differs, 18000 + (n % 9973) + i)
    r, nrm2, adv = inp.run(ws, 1e6)
    if n < _P20:
        assert adv == (0, 0)
        inp.check(r, nrm2, "fp64", "below 2^20")
    else:
        assert adv == (1, 0)
        inp.check(r, nrm2, "shadow", "lp8")


def test_reader_fallback_decision():
    """The device-side premise max c_j^2 <= tau8^2 ||r||^2 decides between two O(1)-different results (the codes are unrelated
    to Q): tau8 = 0 and tau8^2 ||r||^2 = max c_j^2 / 4 give the fp64 formula on Q, tau8^2 ||r||^2 = 4 max c_j^2 the shadow
    formula; dsea_lanczos_lp_stats advances by exactly one on the matching side."""
    n, i = _P20 + 5, 5
    ws = Workspace.get(n, 8, dev())
    inp = ReaderInputs(n, i, True, 19000)
    c = inp.c.cpu().numpy()
    cmax2, rr = float(np.max(c[:i] ** 2)), float(c[i])
    for tau, which, want in ((0.0, "fp64", (0, 1)), (np.sqrt(0.25 * cmax2 / rr), "fp64", (0, 1)),
                             (np.sqrt(4.0 * cmax2 / rr), "shadow", (1, 0))):
        r, nrm2, adv = inp.run(ws, tau)
        assert adv == want, (tau, adv)
        inp.check(r, nrm2, which, "decision tau8=%.3g" % tau)


def test_reader_is_deterministic():
    n, i = _P20 + 5, 23
    ws = Workspace.get(n, max(i, 8), dev())
    inp = ReaderInputs(n, i, True, 19500)
    r1, n1, adv1 = inp.run(ws, 1e6)
    r2, n2, adv2 = inp.run(ws, 1e6)
    assert adv1 == adv2 == (1, 0)
    assert torch.equal(r1, r2) and torch.equal(n1, n2)


# ------------------------------------------------------------------------------------------------------------ writers
def assert_shadow_rows(Q, Qs8, n, written, label):
    """rows in ``written``: Qs8[j, :n] == e5m2_bits(Q[j, :n] * S); everything else in the buffer still holds the sentinel"""
    S = shadow8_scale(n)
    assert bool((Qs8[:, n:] == SENTINEL).all()), "%s: a padding column [n, ld8) was written" % label
    untouched = [j for j in range(Qs8.shape[0]) if j not in set(written)]
    if untouched:
        assert bool((Qs8[untouched, :n] == SENTINEL).all()), "%s: a row outside %s was written" % (label, list(written)[:4])
    for j in written:
        want = e5m2_bits(Q[j, :n].cpu().numpy() * S)
        got = Qs8[j, :n].cpu().numpy()
        bad = np.nonzero(want != got)[0]
        assert bad.size == 0, "%s: row %d, %d elements differ, first at column %d: stored 0x%02x, e5m2_bits gives 0x%02x" % (
            label, j, bad.size, bad[0], got[bad[0]], want[bad[0]])


def chosen_vector(n, seed):
    """values / S: normal draws over 40 binades below the largest code with the chosen values of tests/shadow8_helpers.py mixed
    in (first and last element included); the writer multiplies by S again, exactly"""
    rng = np.random.RandomState(seed)
    v = rng.randn(n) * np.exp2(rng.randint(-28, 12, size=n).astype(np.float64))
    chosen = e5m2_chosen_values()
    m = min(n, 4 * chosen.size)
    pos = rng.permutation(n)[:m]
    if n - 1 not in pos:
        pos[0] = n - 1
    v[pos] = chosen[(seed + np.arange(m)) % chosen.size]
    return v / shadow8_scale(n)


@pytest.mark.parametrize("n", [1, 2, 3, 17, 1000, 4097, _P20 + 5])
def test_store_writes_the_codes_bit_for_bit(n):
    """k_scale_store with ||r||^2 = 1 (beta = 1: the chosen values reach the conversion unchanged): ties, the two-step
    rounding, the carry into the exponent, subnormal codes, signed zeros, the largest codes; rows 0, 1, rows - 1; a row index
    at or beyond the registered row count leaves the shadow alone."""
    lib, st = _lib.load(), _stream(dev())
    ws = Workspace.get(n, 8, dev())
    rows, ldq = 4, round_up(n, 32)
    one = torch.tensor([1.0], dtype=F64, device=dev())
    for case, row in enumerate((0, 1, rows - 1, rows, rows + 1)):
        ld8 = shadow_ld(n, case % 2 == 0)
        Q = torch.zeros((rows + 2, ldq), dtype=F64, device=dev())
        Qs8 = sentinel_buffer(rows + 2, ld8)
        r = torch.from_numpy(chosen_vector(n, 31 * n + row)).to(dev())
        with Registered(ws, Qs8, ld8, rows, 1e-13):
            _lib.check(lib.dsea_lanczos_store(ws.handle, _ptr(r), _ptr(one), _ptr(Q), ldq, row, None, n, st), "dsea_lanczos_store")
        assert_shadow_rows(Q, Qs8, n, [row] if row < rows else [], "dsea_lanczos_store n=%d row=%d ld8=%d" % (n, row, ld8))
        if row < rows:      # the chosen values did reach the shadow: both zeros, subnormal codes, a tie, the largest code
            got = set(Qs8[row, :n].cpu().numpy().tolist())
            assert n < 1000 or {0x00, 0x80, 0x01, 0x02, 0x03, 0x04, 0x3C, 0x3E, 0x40, 0x7B, 0xFB} <= got


def test_registering_one_shadow_unregisters_the_other():
    lib, st = _lib.load(), _stream(dev())
    n, rows = 4097, 2
    ws = Workspace.get(n, 8, dev())
    ldq, ld8 = round_up(n, 32), shadow_ld(n, True)
    one = torch.tensor([1.0], dtype=F64, device=dev())
    r = torch.from_numpy(chosen_vector(n, 5)).to(dev())
    for last in ("8", "16"):
        Q = torch.zeros((rows, ldq), dtype=F64, device=dev())
        Qs8 = sentinel_buffer(rows, ld8)
        Qs16 = torch.full((rows, ldq), SENTINEL16, dtype=torch.int16, device=dev())
        try:
            for which in (("16", "8") if last == "8" else ("8", "16")):
                if which == "8":
                    _lib.check(lib.dsea_ws_set_shadow8(ws.handle, _ptr(Qs8), ld8, rows, 1e-13), "dsea_ws_set_shadow8")
                else:
                    _lib.check(lib.dsea_ws_set_shadow(ws.handle, _ptr(Qs16), ldq, rows, 1e-12), "dsea_ws_set_shadow")
            _lib.check(lib.dsea_lanczos_store(ws.handle, _ptr(r), _ptr(one), _ptr(Q), ldq, 1, None, n, st), "dsea_lanczos_store")
        finally:
            _lib.check(lib.dsea_ws_set_shadow8(ws.handle, None, 0, 0, 0.0), "dsea_ws_set_shadow8")
            _lib.check(lib.dsea_ws_set_shadow(ws.handle, None, 0, 0, 0.0), "dsea_ws_set_shadow")
        wrote8 = not bool((Qs8 == SENTINEL).all())
        wrote16 = not bool((Qs16 == SENTINEL16).all())
        assert (wrote8, wrote16) == ((True, False) if last == "8" else (False, True)), (last, wrote8, wrote16)
        if last == "8":
            assert_shadow_rows(Q, Qs8, n, [1], "after bf16 then 8-bit")


def run_native(op, n, k, differs):
    """dsea_lanczos_run on the test's own Q, Qs8 (k + 1 rows, k registered) and ld8; returns (Q, Qs8, stats)"""
    lib, st = _lib.load(), _stream(dev())
    ws = Workspace.get(n, k, dev())
    _lib.check(lib.dsea_ws_set_reorth_passes(ws.handle, 1), "dsea_ws_set_reorth_passes")
    _lib.check(lib.dsea_ws_set_partial_reorth(ws.handle, 0, 0.0), "dsea_ws_set_partial_reorth")
    ws.reorth_passes, ws.partial_reorth = 1, None
    ldq, ld8 = round_up(n, 32), shadow_ld(n, differs)
    Q = torch.zeros((k, ldq), dtype=F64, device=dev())
    Qs8 = sentinel_buffer(k + 1, ld8)
    alphas = torch.empty(k, dtype=F64, device=dev())
    betas = torch.empty(max(k - 1, 1), dtype=F64, device=dev())
    q0 = torch.from_numpy(normal_vector(n, 4300 + k)).to(dev())
    brk = ctypes.c_int(0)
    with Registered(ws, Qs8, ld8, k, engine.shadow8_tau(n)):
        _lib.check(lib.dsea_lanczos_run(op.handle, ws.handle, k, _ptr(q0), _ptr(Q), ldq, _ptr(alphas), _ptr(betas), st),
                   "dsea_lanczos_run")
        _lib.check(lib.dsea_lanczos_status(ws.handle, byref(brk), st), "dsea_lanczos_status")
        stats = lp_stats(ws)
    assert brk.value == 0
    assert bool(torch.isfinite(alphas).all()) and bool(torch.isfinite(betas).all())
    return Q, Qs8, stats


def check_native(op, n, k, differs, label):
    Q, Qs8, stats = run_native(op, n, k, differs)
    assert stats == (k - 1, 0), (label, stats)
    assert_shadow_rows(Q, Qs8, n, range(k), label)


def tfim(L):
    from dominantsparseeigenad_amd.operators import TFIMOperator
    return TFIMOperator(L, dev(), g=torch.tensor([1.0], dtype=F64, device=dev()))


def tridiagonal(n):
    import scipy.sparse as sp
    rng = np.random.RandomState(5)
    off = rng.randn(n - 1) * 0.4
    return sp.diags([rng.rand(n) + 1.0, off, off], [0, 1, -1], format="csr")


def test_tfim_run_writes_the_codes_bit_for_bit():
    """launch_scale_store (row 0) and the fused tail of the TFIM mat-vec (rows 1..k-1)"""
    check_native(tfim(20), _P20, 6, True, "TFIM L=20")


def test_small_run_leaves_a_registered_shadow_alone():
    """below 2^20 rows the run neither reads nor writes an 8-bit shadow: all-fp64 correction, (0, 0) steps counted"""
    Q, Qs8, stats = run_native(tfim(15), 1 << 15, 6, False)
    assert stats == (0, 0)
    assert_shadow_rows(Q, Qs8, 1 << 15, [], "TFIM L=15")


@pytest.mark.parametrize("layout", ["sell", "csr"])
def test_matrix_run_writes_the_codes_bit_for_bit(layout):
    """an explicit matrix at a ragged n: the fused tail of the SELL mat-vec, and plain CSR (no fused tail: launch_scale_store
    on every row)"""
    from dominantsparseeigenad_amd.operators import CSROperator
    n = _P20 + 5
    check_native(CSROperator.from_scipy(tridiagonal(n), dev(), layout=layout), n, 6, layout == "csr", "%s n=%d" % (layout, n))


def test_stencil_run_writes_the_codes_bit_for_bit():
    from dominantsparseeigenad_amd.operators import Stencil3Operator
    n = _P20 + 5
    x = torch.linspace(-1.0, 1.0, n, dtype=F64, device=dev())
    op = Stencil3Operator(n, 1.0, 0.5 * x * x + 0.1 * torch.from_numpy(normal_vector(n, 66)).to(dev()).abs())
    check_native(op, n, 6, False, "stencil N=%d" % n)


# ------------------------------------------------------------------------------------------------------------ end to end
def test_end_to_end_8_bits_vs_16_bits_vs_no_shadow(monkeypatch):
    """TFIM L = 20, k = 40 through engine.lanczos: E0 of the three runs agrees to 1e-13 relative, ||Q Q^T - I||_max of the
    shadow runs stays within twice the shadow-off run's value plus 1e-15, both shadow runs report 39 / 0."""
    L, k = 20, 40
    n = 1 << L
    op = tfim(L)
    q0 = torch.from_numpy(normal_vector(n, 4500)).to(dev())
    out = {}
    for name, use, bits in (("off", False, 8), ("16", True, 16), ("8", True, 8)):
        monkeypatch.setattr(engine, "USE_SHADOW", use)
        monkeypatch.setattr(engine, "SHADOW_BITS", bits)
        Q, ldq, alphas, betas = engine.lanczos(None, k, n, dev(), q0, native=op)
        stats = engine.lanczos_lp_stats(n, dev())
        a, b = alphas.cpu().numpy(), betas.cpu().numpy()
        E0 = float(np.linalg.eigvalsh(np.diag(a) + np.diag(b, 1) + np.diag(b, -1))[0])
        G = Q[:, :n] @ Q[:, :n].T
        orth = float((G - torch.eye(k, dtype=F64, device=dev())).abs().max())
        out[name] = (E0, orth, stats)
        del Q, G
    print("SHADOW8-E2E " + "  ".join("%s: E0 %.15g orth %.2e lp %s" % ((nm,) + out[nm]) for nm in ("off", "16", "8")))
    assert out["off"][2] == (0, 0) and out["16"][2] == (k - 1, 0) and out["8"][2] == (k - 1, 0)
    for nm in ("16", "8"):
        assert abs(out[nm][0] - out["off"][0]) <= 1e-13 * abs(out["off"][0]), nm
        assert out[nm][1] <= 2.0 * out["off"][1] + 1e-15, nm
