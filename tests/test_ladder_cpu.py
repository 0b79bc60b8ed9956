"""The ladder maps between magnetisation sectors and the Lanczos measure without a GPU (docs/design/24-dynamics.md): the numpy
reference of tests/ladder_reference.py against the full-space operators built with Kronecker products, the identities that the
GPU tests rely on (transpose, forms, the norm of sigma^-(c) psi through the correlators, the f-sum rule with its
Pauli-convention prefactor, the singlet relation between the two channels), the continued-fraction algebra in plain numpy, and
the argument checks of the Python layer that need no device."""
import types

import numpy as np
import pytest
import torch

import ladder_reference as ref
import pairsector_reference
import sector_reference
from dominantsparseeigenad_amd.operators import SpinSectorLadder, ring_bonds, ring_momentum_weights
from dominantsparseeigenad_amd.spectral import SpectralMeasure, _weight_parts
from dominantsparseeigenad_amd.synthetic import normal_vector

SIZES = list(range(2, 9))
# sigma^- = (X - iY) / 2 sets a bit (|0> = up -> |1> = down), sigma^+ clears it; index = bit
SITE = {1: np.array([[0.0, 0.0], [1.0, 0.0]]), -1: np.array([[0.0, 1.0], [0.0, 0.0]]), 0: np.diag([1.0, -1.0])}


def admissible(L):
    """every (ndown_src, step) whose two sectors the library accepts: 1 <= ndown <= L - 1 on both sides"""
    return [(nd, step) for nd in range(1, L) for step in (1, 0, -1) if 1 <= nd + step <= L - 1]


def site_operator(L, i, one):
    """the 2^L x 2^L matrix of the one-site matrix ``one`` on site i: site i is bit i, so it is factor L - 1 - i of the product"""
    out = np.ones((1, 1))
    for j in range(L - 1, -1, -1):
        out = np.kron(out, one if j == i else np.eye(2))
    return out


def full_operator(L, step, c):
    return sum(c[i] * site_operator(L, i, SITE[step]) for i in range(L))


def weights(L, seed=0):
    return normal_vector(L, 9000 + L + seed)


def test_the_site_matrices_are_the_pauli_combinations():
    X, Y = np.array([[0.0, 1.0], [1.0, 0.0]]), np.array([[0.0, -1j], [1j, 0.0]])
    assert np.array_equal((X - 1j * Y) / 2, SITE[1]) and np.array_equal((X + 1j * Y) / 2, SITE[-1])


@pytest.mark.parametrize("L", SIZES)
def test_reference_is_the_block_of_the_full_space_operator(L):
    c = weights(L)
    for nd, step in admissible(L):
        full = full_operator(L, step, c)
        src, dst = sector_reference.states(L, nd), sector_reference.states(L, nd + step)
        block = full[np.ix_(dst, src)]
        S = ref.dense(L, nd, step, c)
        assert S.shape == (len(dst), len(src)) == ref.sizes(L, nd, step)[::-1]
        assert np.array_equal(S, block) if step else np.allclose(S, block, rtol=0, atol=1e-14 * np.abs(c).sum())
        # the rest of the columns of the source states is zero: the operator maps the sector into the destination only
        outside = np.ones(1 << L, dtype=bool)
        outside[list(dst)] = False
        assert not full[np.ix_(outside, src)].any()
        x = normal_vector(len(src), 9100 + L + nd)
        y = ref.apply(L, nd, step, c, x)
        assert np.linalg.norm(y - block @ x) <= 1e-14 * np.linalg.norm(block @ x) + 1e-300


@pytest.mark.parametrize("L", SIZES)
def test_sigma_plus_is_the_transpose_of_sigma_minus(L):
    c = weights(L, 1)
    for nd in range(1, L - 1):                   # a = nd -> b = nd + 1
        down = ref.dense(L, nd, 1, c)
        up = ref.dense(L, nd + 1, -1, c)
        assert np.array_equal(up, down.T)
    for nd in range(1, L):
        Z = ref.dense(L, nd, 0, c)
        assert np.array_equal(Z, Z.T) and np.array_equal(Z, np.diag(np.diag(Z)))


@pytest.mark.parametrize("L", SIZES)
def test_forms_are_the_dense_bilinear_forms(L):
    for nd, step in admissible(L):
        n_src, n_dst = ref.sizes(L, nd, step)
        v1, v2 = normal_vector(n_dst, 9200 + L + nd), normal_vector(n_src, 9300 + L + nd)
        got = ref.forms(L, nd, step, v1, v2)
        want = np.array([v1 @ ref.dense(L, nd, step, np.eye(L)[i]) @ v2 for i in range(L)])
        assert np.max(np.abs(got - want)) <= 1e-14 * np.linalg.norm(v1) * np.linalg.norm(v2)


def lowering_norm_from_correlators(c, xy, z):
    """sum_i c_i^2 (1 + <Z_i>) / 2 + sum_{i<j} c_i c_j <X_i X_j + Y_i Y_j> / 2 for a NORMALISED state: sigma^+_i sigma^-_i is
    the projector (1 + Z_i) / 2 on a clear bit and sigma^+_i sigma^-_j + sigma^+_j sigma^-_i = (X_i X_j + Y_i Y_j) / 2"""
    L = len(c)
    total = sum(c[i] ** 2 * (1.0 + z[i]) / 2.0 for i in range(L))
    for i in range(L):
        for j in range(i + 1, L):
            total += c[i] * c[j] * xy[i][j] / 2.0
    return total


@pytest.mark.parametrize("L", [3, 4, 5, 6, 7, 8])
def test_the_norm_of_sigma_minus_psi_from_the_correlators(L):
    c = weights(L, 2)
    for nd in range(1, L - 1):
        n = len(sector_reference.states(L, nd))
        psi = normal_vector(n, 9400 + L + nd)
        psi = psi / np.linalg.norm(psi)
        f = pairsector_reference.forms(L, nd, psi, psi)
        P = pairsector_reference.npair(L)
        xy = np.zeros((L, L))
        for t, (i, j) in enumerate(pairsector_reference.pairs(L)):
            xy[i, j] = f[t]
        z = f[2 * P:]
        phi = ref.apply(L, nd, 1, c, psi)
        assert abs(phi @ phi - lowering_norm_from_correlators(c, xy, z)) <= 1e-13 * np.sum(np.abs(c)) ** 2


def plain_lanczos(H, phi, k):
    """k steps of the textbook recurrence with full re-orthogonalisation; (alphas, betas)"""
    Q = [phi / np.linalg.norm(phi)]
    a, b = [], []
    for i in range(k):
        u = H @ Q[i]
        a.append(Q[i] @ u)
        for q in Q:
            u = u - (q @ u) * q
        for q in Q:
            u = u - (q @ u) * q
        if i + 1 < k:
            b.append(np.linalg.norm(u))
            Q.append(u / b[-1])
    return np.array(a), np.array(b)


def test_the_continued_fraction_reproduces_the_moments():
    """k Lanczos steps make a Gauss quadrature of the measure of phi: exact for polynomials of degree 2 k - 1, so k = 4 gives
    the moments 0 .. 3 (and more)"""
    L, nd = 8, 4
    bonds = ring_bonds(L) + [(0, 3), (2, 6), (1, 5)]
    p = normal_vector(sector_reference.nparam(L, bonds), 9500)
    H = sector_reference.dense(L, nd, bonds, p)
    phi = normal_vector(H.shape[0], 9501)
    a, b = plain_lanczos(H, phi, 4)
    theta, S = np.linalg.eigh(np.diag(a) + np.diag(b, 1) + np.diag(b, -1))
    w = (phi @ phi) * S[0] ** 2
    measure = SpectralMeasure(torch.from_numpy(theta), torch.from_numpy(w), phi @ phi, 4)
    scale = np.linalg.norm(H, 2)
    v = phi.copy()
    for m in range(4):
        exact = phi @ v
        assert abs(np.sum(w * theta ** m) - exact) <= 1e-12 * (phi @ phi) * scale ** m
        assert abs(measure.moment(m) - exact) <= 1e-12 * (phi @ phi) * scale ** m
        v = H @ v
    assert np.all(w >= 0.0)


def heisenberg(L, nd):
    bonds = ring_bonds(L)
    p = np.concatenate([np.ones(L), np.ones(L), np.zeros(L)])
    return bonds, p, sector_reference.dense(L, nd, bonds, p)


def zz_first_moment_from_correlators(bonds, jxy, c, xy_bond):
    """The f-sum rule in the Pauli convention.  For the hermitian A = sum_i c_i Z_i the first moment of its measure is
    sum_n (E_n - E_0) |<n|A|0>|^2 = <[A, [H, A]]> / 2.  Only the XY part of H fails to commute with A.  With
    X_a X_b + Y_a Y_b = 2 (sigma^+_a sigma^-_b + sigma^-_a sigma^+_b) and [Z_a, sigma^+-_a] = +-2 sigma^+-_a:
        [A, sigma^+_a sigma^-_b] = 2 (c_a - c_b) sigma^+_a sigma^-_b,   [A, sigma^-_a sigma^+_b] = -2 (c_a - c_b) sigma^-_a sigma^+_b
        [A, [H, A]] = -sum_t 4 Jxy_t (c_a - c_b)^2 (X_a X_b + Y_a Y_b)
    so the first moment is -2 sum_t Jxy_t (c_a - c_b)^2 <X_a X_b + Y_a Y_b>."""
    return -2.0 * sum(jxy[t] * (c[a] - c[b]) ** 2 * xy_bond[t] for t, (a, b) in enumerate(bonds))


@pytest.mark.parametrize("L", [6, 8])
def test_the_f_sum_rule_prefactor_against_dense_eigh(L):
    nd = L // 2
    bonds, p, H = heisenberg(L, nd)
    E, V = np.linalg.eigh(H)
    psi0 = V[:, 0]
    xy_bond = sector_reference.forms(L, nd, bonds, psi0, psi0)[:len(bonds)]       # <X_a X_b + Y_a Y_b> per bond
    for m in range(1, L):
        re, im = (t.numpy() for t in ring_momentum_weights(L, m))
        total = 0.0
        for c in (re, im):
            amp = V.T @ ref.apply(L, nd, 0, c, psi0)
            first = np.sum((E - E[0]) * amp ** 2)
            want = zz_first_moment_from_correlators(bonds, p[:len(bonds)], c, xy_bond)
            assert abs(first - want) <= 1e-12 * (E[-1] - E[0])
            total += first
        assert total > 0.0


def test_a_singlet_sees_the_same_triplet_in_both_channels():
    """SU(2): for a singlet |0>, <0| S^+_i f(H) S^-_j |0> = 2 <0| S^z_i f(H) S^z_j |0>.  With sigma^- = S^- and Z = 2 S^z the
    measure of sigma^-(c)|0> is half that of Z(c)|0>, at the same excitation energies (the S^z = -1 member of each triplet)."""
    L = 8
    bonds, p, H0 = heisenberg(L, 4)
    _, _, H1 = heisenberg(L, 5)
    E, V = np.linalg.eigh(H0)
    E1, V1 = np.linalg.eigh(H1)
    psi0 = V[:, 0]
    z = (np.linspace(-1.0, 12.0, 40) + 0.5j)[:, None]
    for m in (1, 3, 4):
        c = ring_momentum_weights(L, m)[0].numpy()
        zz = V.T @ ref.apply(L, 4, 0, c, psi0)
        lo = V1.T @ ref.apply(L, 4, 1, c, psi0)
        Gzz = np.sum(zz ** 2 / (z - (E - E[0])), axis=1)
        Glo = np.sum(lo ** 2 / (z - (E1 - E[0])), axis=1)
        assert np.max(np.abs(Glo - Gzz / 2)) <= 1e-10 * np.max(np.abs(Gzz))


def test_spectral_measure_algebra():
    a = SpectralMeasure([0.5, 2.0], [0.25, 0.75], 1.0, 2)
    b = SpectralMeasure([1.0], [2.0], 2.0, 1)
    s = a + b
    assert len(s) == 3 and s.norm2 == 3.0 and s.steps == 3
    assert s.moment(0) == 3.0 and s.moment(1) == 0.125 + 1.5 + 2.0
    z = torch.tensor([0.3 + 0.5j, 4.0 + 0.1j], dtype=torch.complex128)
    want = sum(w / (z - t) for w, t in ((0.25, 0.5), (0.75, 2.0), (2.0, 1.0)))
    assert torch.allclose(s.greens(z), want, rtol=1e-15, atol=0)
    omega = torch.tensor([0.3, 4.0], dtype=torch.float64)
    assert torch.allclose(s(omega, 0.5), -s.greens(torch.complex(omega, torch.full_like(omega, 0.5))).imag / np.pi)
    assert torch.equal(s.shifted(0.5).poles, s.poles - 0.5) and torch.equal(s.shifted(0.5).weights, s.weights)
    assert s.poles.dtype == torch.float64 and s.poles.device.type == "cpu" and not s.weights.requires_grad
    with pytest.raises(ValueError):
        SpectralMeasure([0.0, 1.0], [1.0], 1.0, 1)
    empty = SpectralMeasure([], [], 0.0, 0)
    assert len(empty) == 0 and empty.moment(0) == 0.0 and (empty + a).moment(0) == 1.0


def test_weight_parts():
    re, im = ring_momentum_weights(6, 1)
    assert len(_weight_parts(re)) == 1
    for parts in (_weight_parts((re, im)), _weight_parts(torch.complex(re, im)), _weight_parts([re.numpy(), im.numpy()])):
        assert len(parts) == 2 and torch.equal(parts[0], re) and torch.equal(parts[1], im)
    assert len(_weight_parts([0.5, -0.5])) == 1              # two numbers are a real vector of two sites, not a pair


def test_ring_momentum_weights():
    L = 10
    for m in (0, 1, 5, 9):
        re, im = ring_momentum_weights(L, m)
        assert re.dtype == im.dtype == torch.float64 and re.shape == im.shape == (L,) and re.device.type == "cpu"
        j = np.arange(L)
        # (the plain formula rounds its argument, up to 2 pi 8.1 = 51, to eps 51 = 1.1e-14; the function reduces m j mod L first)
        assert np.allclose(re.numpy(), np.cos(2 * np.pi * m * j / L) / np.sqrt(L), rtol=0, atol=1.2e-14)
        assert np.allclose(im.numpy(), np.sin(2 * np.pi * m * j / L) / np.sqrt(L), rtol=0, atol=1.2e-14)
        exact = {0: 0.0, 5: 0.0}                # sin(pi j m') at m j a multiple of L / 2: the reduced argument keeps it below eps
        if m in exact:
            assert np.max(np.abs(im.numpy())) <= 4e-16
        assert abs(float(re @ re + im @ im) - 1.0) < 1e-14
    with pytest.raises(ValueError):
        ring_momentum_weights(0, 1)


def carrier(L, ndown, device="cpu"):
    """what SpinSectorLadder reads of an operator, without a device"""
    return types.SimpleNamespace(N=L, ndown=ndown, device=torch.device(device), _tables=(None, None, None))


def test_value_errors_that_need_no_device():
    lad = SpinSectorLadder(carrier(8, 4), carrier(8, 5))
    assert (lad.step, lad.L, lad.n_src, lad.n_dst) == (1, 8, 70, 56)
    back = lad.T
    assert (back.step, back.n_src, back.n_dst) == (-1, 56, 70) and back.T is lad
    same = SpinSectorLadder(carrier(8, 4), carrier(8, 4))
    assert same.step == 0 and same.n_src == same.n_dst == 70
    for src, dst in ((carrier(8, 4), carrier(8, 6)),        # two steps
                     (carrier(8, 4), carrier(8, 2)),
                     (carrier(8, 4), carrier(9, 4)),        # another L
                     (carrier(8, 7), carrier(8, 8)),        # a destination with ndown = L
                     (carrier(8, 1), carrier(8, 0)),        # ... and with ndown = 0
                     (carrier(41, 1), carrier(41, 2)),      # L beyond the limit
                     (carrier(36, 17), carrier(36, 18)),    # more than 2^31 - 1 rows
                     (carrier(8, 4), carrier(8, 5, "meta")),     # another device
                     (carrier(8, 4), object())):            # no tables
        with pytest.raises(ValueError):
            SpinSectorLadder(src, dst)
    for g in (1, 5, 13, -1):
        with pytest.raises(ValueError):
            lad.set_grid_log2(g)
    lad.set_grid_log2(6)
    assert back._grid[0] == 6                               # one setting for the ladder and its transpose
    lad.set_grid_log2(0)
    x = torch.zeros(70, dtype=torch.float64)
    for c in (torch.zeros(7, dtype=torch.float64), torch.zeros((8, 1), dtype=torch.float64),
              torch.zeros(8, dtype=torch.complex128)):
        with pytest.raises(ValueError):
            lad(c, x)
    with pytest.raises(ValueError):
        lad(torch.zeros(8, dtype=torch.float64), torch.zeros(56, dtype=torch.float64))      # a vector of the destination
    with pytest.raises(ValueError):
        lad.forms(x, x)                                     # v1 lives on the destination
    with pytest.raises(ValueError):
        lad(torch.zeros(8, dtype=torch.float64), x)         # host tensors: the map is a device kernel, there is no fallback


def test_the_call_path_is_written_once_in_the_base():
    """docs/design/38-ladder-parts.md: the two public classes carry no call path of their own, only the stem of their C entries
    and the integers that open them -- as many as include/dsea.h (through _lib._SIGNATURES) declares before the first pointer."""
    from ctypes import c_int

    from dominantsparseeigenad_amd import _lib
    from dominantsparseeigenad_amd.operators import HubbardLadder, _SectorLadderBase

    shared = ("_apply_raw", "_forms_raw", "apply_block", "block_dots", "T")
    for name in shared:
        assert name in _SectorLadderBase.__dict__, name
        for cls in (SpinSectorLadder, HubbardLadder):
            assert name not in cls.__dict__, (cls.__name__, name)
    cpu = torch.device("cpu")
    hub = [types.SimpleNamespace(N=6, nup=nup, ndn=2, device=cpu, _up=(None,) * 3, _dn=(None,) * 3) for nup in (3, 4)]
    for lad in (SpinSectorLadder(carrier(8, 4), carrier(8, 5)), HubbardLadder(*hub)):
        args = lad._sector_args()
        assert all(type(a) is int for a in args), args
        assert type(lad.T) is type(lad) and lad.T._sector_args()[-1] == -args[-1] and lad.T.T is lad
        for entry, extra in (("apply", 0), ("forms", 0), ("forms_scratch_doubles", 0), ("block_apply", 1), ("block_dots", 1),
                             ("block_dots_scratch_doubles", 1)):                # (the block entries take the width next)
            argtypes = _lib._SIGNATURES["%s_%s" % (lad._entry, entry)][1]
            k = len(args) + extra
            assert argtypes[:k] == [c_int] * k and argtypes[k] is not c_int, (lad._entry, entry)
