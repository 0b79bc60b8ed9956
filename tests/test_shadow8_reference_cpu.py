"""The 8-bit basis shadow on the CPU (docs/design/15-shadow8.md).  No GPU, no library call.

1. ``e5m2_bits`` (tests/shadow8_helpers.py: plain numpy integer arithmetic, the definition csrc/dsea_device.h implements)
   equals torch's  x.to(float32).to(float8_e5m2)  bit for bit.
2. The oracle's Lanczos loop with ONLY the correction pass changed to what k_axpy_norm_lp8 computes -- codes of q * S decoded,
   fp32 accumulation of  chat_j dec(code_j)  with chat_j = float32(c_j / (S sqrt(r.r))), one fp64 step  r -= w sqrt(r.r),  the
   premise  max c_j^2 <= SHADOW8_TAU^2 r.r  and the fp64 pass of the oracle otherwise -- against the all-fp64 oracle run of the
   same case.  The oracle alone defines every reference value.  The leading alpha, beta are compared in the runs in which no
   step fell back."""
import numpy as np
import pytest
import torch

from dominantsparseeigenad_amd import engine
from oracle.operators import TFIMTables
from oracle.solvers import lanczos_tridiag, tridiag_matrix
from shadow8_helpers import e5m2_bits, e5m2_chosen_values, e5m2_value, shadow8_scale


def torch_bits(x):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    return t.to(torch.float32).to(torch.float8_e5m2).view(torch.uint8).numpy()


def test_e5m2_bits_equals_torch_on_normal_draws_across_the_range():
    rng = np.random.RandomState(20250)
    x = rng.randn(200000) * np.exp2(rng.randint(-24, 15, size=200000).astype(np.float64))
    x = x[np.abs(x) <= 2.0 ** 15.5]
    assert np.unique(np.frexp(x)[1]).size >= 38
    assert np.array_equal(e5m2_bits(x), torch_bits(x))


def test_e5m2_bits_on_every_tie_and_its_neighbours():
    """midpoints of all adjacent finite codes (subnormal ones included) and the fp64 / fp32 values next to them"""
    codes = np.arange(0x00, 0x7B, dtype=np.uint8)
    lo, hi = e5m2_value(codes), e5m2_value(codes + 1)
    mid = 0.5 * (lo + hi)
    x = np.concatenate([mid, np.nextafter(mid, 0.0), np.nextafter(mid, np.inf),
                        np.nextafter(mid.astype(np.float32), np.float32(0)).astype(np.float64),
                        np.nextafter(mid.astype(np.float32), np.float32(np.inf)).astype(np.float64), lo, hi])
    x = np.concatenate([x, -x])
    assert np.array_equal(e5m2_bits(x), torch_bits(x))
    got = e5m2_bits(mid)
    assert np.array_equal(got, np.where(codes % 2 == 0, codes, codes + 1))       # ties go to the even code


def test_e5m2_bits_on_chosen_values():
    x = e5m2_chosen_values()
    got = e5m2_bits(x)
    assert np.array_equal(got, torch_bits(x))
    half = x.size // 2
    want = {0.0: 0x00, 1.0 + 2.0 ** -3: 0x3C, 1.0 + 3.0 * 2.0 ** -3: 0x3E, 1.0 + 2.0 ** -3 + 2.0 ** -40: 0x3C,
            2.0 - 2.0 ** -23: 0x40, 2.0 ** -14: 0x04, 2.0 ** -16: 0x01, 2.0 ** -15: 0x02, 3.0 * 2.0 ** -16: 0x03,
            2.0 ** -17: 0x00, 2.0 ** -17 + 2.0 ** -40: 0x01, 3.0 * 2.0 ** -17: 0x02, 5.0 * 2.0 ** -17: 0x02, 7.0 * 2.0 ** -17: 0x04,
            1e-300: 0x00, 2.0 ** 15: 0x78, 2.0 ** 15.5: 0x7A, 57344.0: 0x7B}
    for v, b in want.items():
        (idx,) = np.nonzero(x[:half] == v)
        assert idx.size == 1, v
        assert got[idx[0]] == b, (v, hex(got[idx[0]]))
        assert got[half + idx[0]] == (b | 0x80), (v, hex(got[half + idx[0]]))     # the sign bit survives, -0 included


def test_e5m2_value_inverts_e5m2_bits():
    bits = np.arange(0x100, dtype=np.uint16).astype(np.uint8)
    finite = (bits & 0x7C) != 0x7C
    v = e5m2_value(bits[finite])
    assert np.array_equal(e5m2_bits(v), bits[finite])
    t = torch.from_numpy(bits[finite].copy()).view(torch.float8_e5m2).double().numpy()
    assert np.array_equal(v, t) and np.array_equal(np.signbit(v), np.signbit(t))
    assert np.isnan(e5m2_value(np.uint8(0x7F))[0])       # the sentinel of the GPU tests


def test_scale_keeps_unit_vectors_finite():
    for n in (1, 2, 255, 256, 257, 1 << 20, (1 << 20) + 1, 1 << 30, 1 << 31, 1 << 40):
        S = shadow8_scale(n)
        assert S == engine.shadow8_scale(n)
        assert S == 2.0 ** min(15, int(np.ceil(np.log2(n) / 2.0)))
        assert e5m2_bits(np.array([S]))[0] < 0x7C


def test_premise_bound_follows_the_measured_floor():
    """SHADOW8_TAU while it keeps a 4x margin over the sqrt(n) rounding floor of the coefficients, 4x the floor beyond (the CPU
    oracle's 7.3e-15 / 1.5e-14 / 3.1e-14 at L = 16 / 18 / 20 stay a factor 4 below it), never above SHADOW_TAU"""
    assert engine.SHADOW8_TAU == 2.0 ** -6 * engine.SHADOW_TAU
    for n in (1, 256, 4096, 1 << 14):
        assert engine.shadow8_tau(n) == engine.SHADOW8_TAU
    for L, seen in ((16, 7.31e-15), (18, 1.506e-14), (20, 3.07e-14)):
        assert 3.9 * seen <= engine.shadow8_tau(1 << L) <= 4.3 * seen
    assert engine.shadow8_tau(1 << 50) == engine.SHADOW_TAU


# ---------------------------------------------------------------------------------------------------- the simulation
def lanczos_shadow8(apply_A, k, n, draw, tau):
    """oracle.solvers.lanczos_tridiag, statement for statement, except the correction pass (module docstring).
    Returns (Q, alphas, betas, steps that took the fp64 pass)."""
    S = shadow8_scale(n)
    Q = torch.zeros((n, k), dtype=torch.float64)
    codes = np.zeros((k, n), dtype=np.uint8)
    alphas, betas = torch.zeros(k, dtype=torch.float64), torch.zeros(max(k - 1, 0), dtype=torch.float64)
    q = draw(n, torch.float64)
    q = q / torch.norm(q)
    u = apply_A(q)
    alpha = torch.matmul(q, u)
    Q[:, 0] = q
    codes[0] = e5m2_bits(q.numpy() * S)
    alphas[0] = alpha
    beta = 0
    q_prev = draw(n, torch.float64)
    fallback = []
    for i in range(1, k):
        r = u - alpha * q - beta * q_prev
        basis = Q[:, :i]
        c = torch.matmul(basis.T, r)
        rr = float(torch.dot(r, r))
        if float((c * c).max()) <= tau * tau * rr:
            rnorm = np.sqrt(rr)
            chat = (c.numpy() * (1.0 / (S * rnorm))).astype(np.float32)
            w = np.zeros(n, dtype=np.float32)
            for j in range(i - 1, -1, -1):       # fp32 FMA: the product is exact in fp64, one rounding to fp32
                w = (np.float64(chat[j]) * e5m2_value(codes[j]) + w.astype(np.float64)).astype(np.float32)
            r = r - torch.from_numpy(w.astype(np.float64) * rnorm)
        else:
            fallback.append(i)
            r = r - torch.matmul(basis, c)
        q_prev = q
        beta = torch.norm(r)
        q = r / beta
        u = apply_A(q)
        alpha = torch.matmul(q, u)
        alphas[i] = alpha
        betas[i - 1] = beta
        Q[:, i] = q
        codes[i] = e5m2_bits(q.numpy() * S)
    return Q, alphas, betas, fallback


def _case(name):
    if name.startswith("tfim"):
        L, g, k = {"tfim_L10": (10, 1.0, 200), "tfim_L12": (12, 1.0, 200), "tfim_L12_g0.9": (12, 0.9, 300),
                   "tfim_L8": (8, 1.0, 200)}[name]
        op = TFIMTables(L, g=torch.tensor(g, dtype=torch.float64))
        return op.H, 1 << L, k
    gen = torch.Generator().manual_seed(256)
    M = torch.randn((256, 256), generator=gen, dtype=torch.float64)
    M = 0.5 * (M + M.T)
    return (lambda v: torch.matmul(M, v)), 256, 256


def _pinned_draw(seed):
    gen = torch.Generator().manual_seed(seed)
    return lambda n, dtype: torch.randn(n, generator=gen, dtype=dtype)


def _measures(apply_A, Q, alphas, betas):
    evals, Svec = torch.linalg.eigh(tridiag_matrix(alphas, betas))
    psi = torch.matmul(Q, Svec[:, 0])
    k = Q.shape[1]
    orth = float((Q.T @ Q - torch.eye(k, dtype=torch.float64)).abs().max())
    resid = float(torch.norm(apply_A(psi) - evals[0] * psi))
    return float(evals[0]), orth, resid


_REFERENCE = {}


def _reference(name):
    if name not in _REFERENCE:
        apply_A, n, k = _case(name)
        Q, a, b = lanczos_tridiag(apply_A, k, sparse=True, dim=n, draw=_pinned_draw(77))
        _REFERENCE[name] = (Q, a, b, _measures(apply_A, Q, a, b))
    return _REFERENCE[name]


@pytest.mark.parametrize("name", ["tfim_L10", "tfim_L12", "tfim_L12_g0.9", "tfim_L8", "dense256"])
def test_shadow8_correction_is_exact_to_working_precision(name):
    """Bounds as the issue states them; the premise bound is what the engine registers for a run of this size, which at
    these sizes is SHADOW8_TAU itself.  dense256 (k = n) ends on a step whose r is rounding noise (max|c_j| / ||r|| =
    9.4e-14): it must take the fp64 pass, as must steps of L = 8 past its Krylov dimension."""
    apply_A, n, k = _case(name)
    _, a0, b0, (E0, orth0, resid0) = _reference(name)
    Q, a, b, fallback = lanczos_shadow8(apply_A, k, n, _pinned_draw(77), engine.shadow8_tau(n))
    E, orth, resid = _measures(apply_A, Q, a, b)
    m = min(k, 60)
    da = float((a[:m] - a0[:m]).abs().max())
    db = float((b[:m - 1] - b0[:m - 1]).abs().max()) if m > 1 else 0.0
    print("SHADOW8-SIM %s n=%d k=%d: fp64 steps %d (first %s)  E0 rel %.2e  orth %.2e (oracle %.2e)  resid %.2e (oracle %.2e)  "
          "alpha %.2e beta %.2e over %d steps" % (name, n, k, len(fallback), fallback[:1], abs(E - E0) / abs(E0), orth, orth0,
                                                  resid, resid0, da, db, m))
    assert abs(E - E0) <= 1e-13 * abs(E0)
    assert orth <= 2.0 * orth0 + 1e-15
    assert resid <= 2.0 * resid0 + 1e-15
    if not fallback:
        # (a run with fp64 steps has left the regime the premise describes: at L = 8 the Krylov space is exhausted near step
        #  35, beta drops to 1e-5 and the later alpha, beta are set by rounding noise in the oracle's own run as well)
        assert da <= 1e-12 and db <= 1e-12
    assert engine.shadow8_tau(n) == engine.SHADOW8_TAU == 2.0 ** -6 * engine.SHADOW_TAU
    if name == "dense256":
        assert fallback == [255], fallback
    if name == "tfim_L8":
        assert fallback, "k = 200 at L = 8 runs beyond the Krylov dimension: the premise must send steps to the fp64 pass"
    if name in ("tfim_L10", "tfim_L12", "tfim_L12_g0.9"):
        assert len(fallback) == 0, fallback
