"""The conjugate-gradient kernels one library call at a time (docs/design/26-cg-stage-tests.md): dsea_shift_dot, the a_dot_v of
dsea_project_out, the five unfused phases, dsea_cg_step, dsea_block_project_out, dsea_cg_deflated_init and
dsea_cg_deflated_step, each on prepared inputs with everything downloaded and judged by tests/cg_reference.py -- EXACT inputs
bit for bit (every output vector, every state slot), RANDOM inputs against np.longdouble with bounds that count operations.
tests/test_cg_reference_cpu.py shows without a GPU that the same ``Checks`` reject wrong kernels.

Every vector lives at the start of a buffer two elements longer than n whose tail is NaN: after every call the tail must be
unchanged bit for bit and the n rows finite (the ld2<true> / st2<true> guards at odd n).  Psi is an (m, ldpsi) buffer with
ldpsi > n and NaN padding.  State slots a call must not write hold a sentinel and must come back unchanged."""
from ctypes import c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cg_reference as ref  # noqa: E402
from cg_reference import Checks  # noqa: E402
from dominantsparseeigenad_amd import _lib, engine  # noqa: E402
from dominantsparseeigenad_amd.engine import Workspace, _ptr, _stream  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402

F64 = torch.float64
ERR_ARG, ERR_ALIGN = -1, -2
NAN_BITS = np.array([np.nan, np.nan]).view(np.int64)


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


class Buf:
    """an n-row vector at the start of an (n + 2)-element device buffer with a NaN tail"""

    def __init__(self, host):
        host = np.ascontiguousarray(host, dtype=np.float64)
        self.n, self.host = host.size, host
        full = np.full(self.n + 2, np.nan)
        full[:self.n] = host
        self.t = torch.from_numpy(full).to(dev())

    @property
    def ptr(self):
        return _ptr(self.t)

    def down(self, what):
        got = self.t.cpu().numpy()
        assert np.array_equal(got[self.n:].view(np.int64), NAN_BITS), "%s: the call wrote past row n - 1" % what
        assert np.isfinite(got[:self.n]).all(), "%s: non-finite rows (a read past row n - 1?)" % what
        return got[:self.n].copy()

    def kept(self, what):
        assert ref.same(self.down(what), self.host), "%s: a read-only operand was modified" % what


def psi_buf(Psi):
    """(device (m, ldpsi) buffer with NaN beyond column n, ldpsi even and > n)"""
    m, n = Psi.shape
    ld = n + (n & 1) + 2
    full = np.full((m, ld), np.nan)
    full[:, :n] = Psi
    return torch.from_numpy(full).to(dev()), ld


def psi_kept(t, Psi, what):
    got = t.cpu().numpy()
    n = Psi.shape[1]
    assert ref.same(got[:, :n], Psi) and np.isnan(got[:, n:]).all(), "%s: Psi was modified" % what


def scalars(values):
    return torch.from_numpy(np.array(values, dtype=np.float64).reshape(-1)).to(dev())


class Library:
    """the interface cg_reference.Checks drives, one library call per method"""

    def __init__(self):
        self.lib = _lib.load()

    def ws(self, n, m=1):
        return Workspace.get(n, max(8, m + 1), dev()).handle

    def st(self):
        return _stream(dev())

    def shift_dot(self, x, y, shift, skip=False, dot0=ref.SENTINEL):
        n = x.size
        xb, yb = Buf(x), Buf(y)
        sh = scalars([shift]) if shift is not None else None
        dot, flag = scalars([dot0]), (scalars([1.0]) if skip else None)
        _lib.check(self.lib.dsea_shift_dot(self.ws(n), xb.ptr, yb.ptr, _ptr(sh), _ptr(dot), _ptr(flag), n, self.st()), "dsea_shift_dot")
        xb.kept("dsea_shift_dot x")
        return yb.down("dsea_shift_dot y"), dot.item()

    def project_out(self, v, a):
        n = v.size
        vb, ab, ob = Buf(v), Buf(a), Buf(np.full(n, ref.SENTINEL))
        c = scalars([ref.SENTINEL])
        _lib.check(self.lib.dsea_project_out(self.ws(n), vb.ptr, ab.ptr, ob.ptr, _ptr(c), n, self.st()), "dsea_project_out")
        vb.kept("dsea_project_out v")
        ab.kept("dsea_project_out a")
        return ob.down("dsea_project_out out"), c.item()

    def cg_init(self, b, Ax0, state0):
        n = b.size
        bb, ab, rb, db = Buf(b), Buf(Ax0), Buf(np.full(n, ref.SENTINEL)), Buf(np.full(n, ref.SENTINEL))
        s = scalars(state0)
        _lib.check(self.lib.dsea_cg_init(self.ws(n), bb.ptr, ab.ptr, rb.ptr, db.ptr, _ptr(s), n, self.st()), "dsea_cg_init")
        bb.kept("dsea_cg_init b")
        ab.kept("dsea_cg_init Ax0")
        return rb.down("dsea_cg_init r"), db.down("dsea_cg_init d"), s.cpu().numpy()

    def cg_init_check(self, state, eps):
        s = scalars(state)
        _lib.check(self.lib.dsea_cg_init_check(self.ws(8), _ptr(s), float(eps), self.st()), "dsea_cg_init_check")
        return s.cpu().numpy()

    def cg_update(self, x, r, d, Ad, state):
        n = x.size
        xb, rb, db, ab = Buf(x), Buf(r), Buf(d), Buf(Ad)
        s = scalars(state)
        _lib.check(self.lib.dsea_cg_update(self.ws(n), xb.ptr, rb.ptr, db.ptr, ab.ptr, _ptr(s), n, self.st()), "dsea_cg_update")
        db.kept("dsea_cg_update d")
        ab.kept("dsea_cg_update Ad")
        return xb.down("dsea_cg_update x"), rb.down("dsea_cg_update r"), s.cpu().numpy()

    def cg_check(self, state, eps):
        s = scalars(state)
        _lib.check(self.lib.dsea_cg_check(self.ws(8), _ptr(s), float(eps), self.st()), "dsea_cg_check")
        return s.cpu().numpy()

    def cg_direction(self, r, d, state):
        n = r.size
        rb, db = Buf(r), Buf(d)
        s = scalars(state)
        _lib.check(self.lib.dsea_cg_direction(self.ws(n), rb.ptr, db.ptr, _ptr(s), n, self.st()), "dsea_cg_direction")
        rb.kept("dsea_cg_direction r")
        assert ref.same(s.cpu().numpy(), state), "dsea_cg_direction wrote to state"
        return db.down("dsea_cg_direction d")

    def cg_step(self, x, r, d, Ad, shift, state, eps, iteration):
        n = x.size
        xb, rb, db, ab = Buf(x), Buf(r), Buf(d), Buf(Ad)
        s = scalars(state)
        sh = scalars([shift]) if shift is not None else None
        _lib.check(self.lib.dsea_cg_step(self.ws(n), xb.ptr, rb.ptr, db.ptr, ab.ptr, _ptr(sh), _ptr(s), float(eps), int(iteration), n,
                                         self.st()), "dsea_cg_step")
        return (xb.down("dsea_cg_step x"), rb.down("dsea_cg_step r"), db.down("dsea_cg_step d"), ab.down("dsea_cg_step Ad"),
                s.cpu().numpy())

    def block_project(self, v, Psi, inplace=False, coef=True):
        n, m = v.size, Psi.shape[0]
        vb = Buf(v)
        ob = vb if inplace else Buf(np.full(n, ref.SENTINEL))
        P, ld = psi_buf(Psi)
        c = scalars([ref.SENTINEL] * (m + 1)) if coef else None
        _lib.check(self.lib.dsea_block_project_out(self.ws(n, m), vb.ptr, _ptr(P), ld, m, ob.ptr, _ptr(c), n, self.st()),
                   "dsea_block_project_out")
        if not inplace:
            vb.kept("dsea_block_project_out v")
        psi_kept(P, Psi, "dsea_block_project_out")
        if not coef:
            return ob.down("dsea_block_project_out out"), None
        ch = c.cpu().numpy()
        assert ch[m] == ref.SENTINEL, "dsea_block_project_out wrote more than m coefficients"
        return ob.down("dsea_block_project_out out"), ch[:m].copy()

    def deflated_init(self, b, x, Ax, shift, Psi, eps):
        n, m = b.size, Psi.shape[0]
        bb, xb, ab, rb, db = Buf(b), Buf(x), Buf(Ax), Buf(np.full(n, ref.SENTINEL)), Buf(np.full(n, ref.SENTINEL))
        P, ld = psi_buf(Psi)
        s = scalars([ref.SENTINEL] * ref.STATE_LEN)
        sh = scalars([shift]) if shift is not None else None
        _lib.check(self.lib.dsea_cg_deflated_init(self.ws(n, m), bb.ptr, xb.ptr, ab.ptr, _ptr(sh), _ptr(P), ld, m, rb.ptr, db.ptr, _ptr(s),
                                                  float(eps), n, self.st()), "dsea_cg_deflated_init")
        for buf, name in ((bb, "b"), (xb, "x"), (ab, "Ax")):
            buf.kept("dsea_cg_deflated_init " + name)
        psi_kept(P, Psi, "dsea_cg_deflated_init")
        return rb.down("dsea_cg_deflated_init r"), db.down("dsea_cg_deflated_init d"), s.cpu().numpy()

    def deflated_step(self, x, r, d, Ad, shift, Psi, state, eps, iteration):
        n, m = x.size, Psi.shape[0]
        xb, rb, db, ab = Buf(x), Buf(r), Buf(d), Buf(Ad)
        P, ld = psi_buf(Psi)
        s = scalars(state)
        sh = scalars([shift]) if shift is not None else None
        _lib.check(self.lib.dsea_cg_deflated_step(self.ws(n, m), xb.ptr, rb.ptr, db.ptr, ab.ptr, _ptr(sh), _ptr(P), ld, m, _ptr(s),
                                                  float(eps), int(iteration), n, self.st()), "dsea_cg_deflated_step")
        psi_kept(P, Psi, "dsea_cg_deflated_step")
        return (xb.down("dsea_cg_deflated_step x"), rb.down("dsea_cg_deflated_step r"), db.down("dsea_cg_deflated_step d"),
                ab.down("dsea_cg_deflated_step Ad"), s.cpu().numpy())


def checks():
    # (the longdouble side of the exact class's headroom is proved by tests/test_cg_reference_cpu.py; the assertion on the
    # sums of every case runs here as well)
    return Checks(Library(), prove=False)


PHASE_SIZES = ref.SIZES + ref.SIZES_PHASE_EXTRA
NM = [(n, m) for n in ref.SIZES for m in ref.MS if m <= n]


# ------------------------------------------------------------------------------------------------ vector phases
@pytest.mark.parametrize("n", PHASE_SIZES)
def test_shift_dot(n):
    assert checks().shift_dot(n) <= 1.0


@pytest.mark.parametrize("n", PHASE_SIZES)
def test_project_out_with_a_dot_v(n):
    assert checks().project_out(n) <= 1.0


# ------------------------------------------------------------------------------------------------ unfused phases
@pytest.mark.parametrize("n", PHASE_SIZES)
def test_cg_init(n):
    assert checks().cg_init(n) <= 1.0


def test_cg_init_check():
    checks().cg_init_check()


@pytest.mark.parametrize("n", PHASE_SIZES)
def test_cg_update(n):
    assert checks().cg_update(n) <= 1.0


def test_cg_check():
    checks().cg_check()


@pytest.mark.parametrize("n", PHASE_SIZES)
def test_cg_direction(n):
    assert checks().cg_direction(n) <= 1.0


# ------------------------------------------------------------------------------------------------ fused step
@pytest.mark.parametrize("n", ref.SIZES)
def test_cg_step(n):
    assert checks().cg_step(n) <= 1.0


@pytest.mark.parametrize("n", ref.SIZES)
def test_cg_step_converged_and_already_done(n):
    checks().cg_step_converged_and_done(n)


def test_cg_step_stop_is_strict():
    checks().cg_step_strict()


def test_cg_step_chain():
    assert checks().cg_step_chain() <= 1.0


# ------------------------------------------------------------------------------------------------ deflation
@pytest.mark.parametrize("n,m", NM)
def test_block_project_out(n, m):
    assert checks().block_project(n, m, random=(n <= 4097 or m == 3)) <= 1.0


@pytest.mark.parametrize("n,m", NM)
def test_cg_deflated_init(n, m):
    assert checks().deflated_init(n, m, random=(n <= 4097 or m == 3)) <= 1.0


@pytest.mark.parametrize("n,m", NM)
def test_cg_deflated_step(n, m):
    assert checks().deflated_step(n, m, random=(n <= 4097 or m == 3)) <= 1.0


def test_cg_deflated_step_stop_is_strict():
    checks().deflated_strict()


def test_cg_deflated_step_chain():
    assert checks().deflated_chain() <= 1.0


# ------------------------------------------------------------------------------------------------ return codes
def test_return_codes():
    """an odd-offset pointer is DSEA_ERR_ALIGN, a null required pointer or m outside 1 .. DSEA_MAX_NEV DSEA_ERR_ARG (all
    refused on the host, before any launch)"""
    lib = _lib.load()
    n, m = 16, 2
    ws, st = Workspace.get(n, 10, dev()).handle, _stream(dev())
    pool = torch.zeros(8 * (n + 2), dtype=F64, device=dev())
    v = [pool[i * (n + 2):i * (n + 2) + n] for i in range(6)]
    odd = pool[1:1 + n]
    assert odd.data_ptr() % 16 == 8
    Psi = torch.zeros((m, n), dtype=F64, device=dev())
    state, sh, null = torch.zeros(8, dtype=F64, device=dev()), torch.zeros(1, dtype=F64, device=dev()), c_void_p(None)
    p = _ptr
    S, E = p(state), 1e-7
    # (function, arguments, positions of the 16-byte-aligned vector pointers, positions of the required pointers)
    table = [
        ("dsea_shift_dot", [ws, p(v[0]), p(v[1]), p(sh), p(sh), null, n, st], (1, 2), (0, 1, 2, 4)),
        ("dsea_project_out", [ws, p(v[0]), p(v[1]), p(v[2]), p(sh), n, st], (1, 2, 3), (0, 1, 2, 3)),
        ("dsea_cg_init", [ws, p(v[0]), p(v[1]), p(v[2]), p(v[3]), S, n, st], (1, 2, 3, 4), (0, 1, 2, 3, 4, 5)),
        ("dsea_cg_init_check", [ws, S, E, st], (), (1,)),
        ("dsea_cg_update", [ws, p(v[0]), p(v[1]), p(v[2]), p(v[3]), S, n, st], (1, 2, 3, 4), (0, 1, 2, 3, 4, 5)),
        ("dsea_cg_check", [ws, S, E, st], (), (1,)),
        ("dsea_cg_direction", [ws, p(v[0]), p(v[1]), S, n, st], (1, 2), (1, 2, 3)),
        ("dsea_cg_step", [ws, p(v[0]), p(v[1]), p(v[2]), p(v[3]), p(sh), S, E, 0, n, st], (1, 2, 3, 4), (0, 1, 2, 3, 4, 6)),
        ("dsea_block_project_out", [ws, p(v[0]), p(Psi), n, m, p(v[1]), null, n, st], (1, 2, 5), (0, 1, 2, 5)),
        ("dsea_cg_deflated_init", [ws, p(v[0]), p(v[1]), p(v[2]), p(sh), p(Psi), n, m, p(v[3]), p(v[4]), S, E, n, st],
         (1, 2, 3, 5, 8, 9), (0, 1, 2, 3, 5, 8, 9, 10)),
        ("dsea_cg_deflated_step", [ws, p(v[0]), p(v[1]), p(v[2]), p(v[3]), p(sh), p(Psi), n, m, S, E, 0, n, st],
         (1, 2, 3, 4, 6), (0, 1, 2, 3, 4, 6, 9)),
    ]
    m_at = {"dsea_block_project_out": 4, "dsea_cg_deflated_init": 7, "dsea_cg_deflated_step": 8}
    for name, args, aligned, required in table:
        fn = getattr(lib, name)
        for i in aligned:
            bad = list(args)
            bad[i] = p(odd)
            assert fn(*bad) == ERR_ALIGN, (name, "odd pointer at", i)
        for i in required:
            bad = list(args)
            bad[i] = null
            assert fn(*bad) == ERR_ARG, (name, "null pointer at", i)
        if name in m_at:
            for wrong in (0, ref.MAX_NEV + 1):
                bad = list(args)
                bad[m_at[name]] = wrong
                assert fn(*bad) == ERR_ARG, (name, "m =", wrong)
            bad = list(args)
            bad[m_at[name] - 1] = n + 1                       # an odd ldpsi
            assert fn(*bad) == ERR_ALIGN, (name, "odd ldpsi")
    torch.cuda.synchronize()
    assert not pool.any() and not state.any(), "a refused call reached the device"


# ------------------------------------------------------------------------------------------------ one end-to-end link
def test_deflated_cg_around_a_callable_equals_the_native_operand():
    """engine.cg_deflated with callable_A wrapping a CSR operator (dsea_cg_deflated_init / _step around the caller's mat-vec)
    against dsea_cg_run_deflated on the same operator: same iteration count, x to 1e-13 of its scale -- the tolerance of
    test_cg_step_around_a_callable_equals_the_phase_calls_and_the_native_streaming_form for this same kind of difference (the
    d.A'd partials come from different kernels)"""
    import scipy.sparse as sp
    from scipy.linalg import eigh_tridiagonal
    from dominantsparseeigenad_amd.operators import CSROperator
    n, m = 4097, 3
    rng = np.random.RandomState(n)
    dg, off = rng.rand(n) + 3.0, rng.randn(n - 1) * 0.3
    op = CSROperator.from_scipy(sp.diags([dg, off, off], [0, 1, -1], format="csr"), dev(), layout="csr")
    _, V = eigh_tridiagonal(dg, off, select="i", select_range=(0, m - 1))     # Psi spans an invariant subspace: P commutes with A
    ld = n + 1
    Psi = torch.zeros((m, ld), dtype=F64, device=dev())
    Psi[:, :n] = torch.from_numpy(np.ascontiguousarray(V.T)).to(dev())
    b, x0 = torch.from_numpy(normal_vector(n, 9300)).to(dev()), torch.from_numpy(normal_vector(n, 9301)).to(dev())
    shift = torch.tensor([-0.25], dtype=F64, device=dev())                    # A - shift is SPD with a condition number near 2
    xc = engine.cg_deflated(b, x0, Psi, ld, m, callable_A=lambda v: op(v), shift=shift, eps=1e-10, maxiter=400).clone()
    it_c, conv_c = engine.last_cg.iters, engine.last_cg.converged
    xn = engine.cg_deflated(b, x0, Psi, ld, m, native=op, shift=shift, eps=1e-10, maxiter=400)
    assert conv_c and engine.last_cg.converged
    assert engine.last_cg.iters == it_c, (engine.last_cg.iters, it_c)
    scale = float(xn.abs().max())
    assert float((xc - xn).abs().max()) <= 1e-13 * scale, float((xc - xn).abs().max()) / scale
