"""All-pair XXZ couplings in one magnetisation sector without a GPU (docs/design/22-pair-sector.md): the numpy reference of
tests/pairsector_reference.py against the bond-list references with the bond list "all pairs" (legal up to L = 16, here
L <= 8), the pure-Python and pure-torch helpers against direct sums, the Haldane-Shastry closed form by dense eigh, and the
argument validation of the Python class and of the new C-ABI entry points, which runs before any device work."""
import ctypes
import math
from ctypes import byref, c_int64, c_void_p

import numpy as np
import pytest
import torch

import lattice_reference
import pairsector_reference as ref
import sector_reference
from dominantsparseeigenad_amd import _lib, operators
from dominantsparseeigenad_amd.operators import (SpinSectorPairOperator, pair_count, pair_index, power_law_couplings,
                                                 ring_structure_factor)
from dominantsparseeigenad_amd.synthetic import normal_vector

SIZES = list(range(2, 9))


@pytest.mark.parametrize("L", SIZES)
def test_pair_reference_is_the_bond_list_reference_on_all_pairs(L):
    bonds = lattice_reference.complete_bonds(L)
    assert list(ref.pairs(L)) == bonds and len(bonds) == ref.npair(L) <= 28
    p = normal_vector(ref.nparam(L), 2100 + L)
    full = lattice_reference.dense(L, bonds, sector_reference.full_parameter(L, bonds, p))
    for ndown in range(1, L):
        st = np.array(ref.states(L, ndown), dtype=np.int64)
        assert ref.states(L, ndown) == sector_reference.states(L, ndown)
        n = st.size
        x, v1 = normal_vector(n, 2200 + L + ndown), normal_vector(n, 2300 + L + ndown)
        want = sector_reference.apply(L, ndown, bonds, p, x)
        scale = np.abs(p).sum() * np.max(np.abs(x))
        assert np.max(np.abs(ref.apply(L, ndown, p, x) - want)) <= 1e-13 * scale
        H = ref.dense(L, ndown, p)
        assert np.max(np.abs(H - full[st][:, st])) <= 1e-14 * max(1.0, np.max(np.abs(full)))
        assert np.array_equal(H, H.T)
        got = ref.forms(L, ndown, v1, x)
        bound = 1e-13 * np.linalg.norm(v1) * np.linalg.norm(x)
        assert np.max(np.abs(got - sector_reference.forms(L, ndown, bonds, v1, x))) <= bound
        assert abs(v1 @ (H @ x) - np.sum(p * got)) <= 1e-13 * np.linalg.norm(v1) * np.linalg.norm(x) * np.abs(p).sum()


def test_pair_index_and_count():
    for L in range(2, 41):
        listed = [(i, j) for i in range(L) for j in range(i + 1, L)]
        assert pair_count(L) == len(listed) == ref.npair(L)
        if L <= 12 or L == 40:
            for t, (i, j) in enumerate(listed):
                assert pair_index(L, i, j) == pair_index(L, j, i) == ref.pair_index(L, i, j) == t
    assert pair_count(40) == 780 and pair_count(24) == 276 and pair_count(16) == 120 and pair_count(17) > _lib.LATTICE_MAX_BONDS
    for bad in ((3, 3), (-1, 2), (0, 8), (8, 0)):
        with pytest.raises(ValueError):
            pair_index(8, *bad)


def test_power_law_couplings_against_direct_sums():
    for L, alpha, periodic in ((2, 1.0, False), (7, 2.5, False), (8, 3.0, True), (9, 0.0, True), (40, 1.5, False)):
        got = power_law_couplings(L, alpha, periodic=periodic)
        assert got.shape == (L, L) and got.dtype == torch.float64
        want = np.zeros((L, L))
        for i in range(L):
            for j in range(i + 1, L):
                d = min(j - i, L - (j - i)) if periodic else j - i
                want[i, j] = d ** (-alpha)
        assert np.max(np.abs(got.numpy() - want)) <= 4e-16
        assert bool((torch.tril(got) == 0.0).all())
    # differentiable in alpha: d/dalpha d^-alpha = -log(d) d^-alpha, finite everywhere (the diagonal too)
    a = torch.tensor(2.0, dtype=torch.float64, requires_grad=True)
    M = power_law_couplings(6, a)
    weights = torch.from_numpy(normal_vector(36, 2400).copy()).reshape(6, 6)
    (g,) = torch.autograd.grad((M * weights).sum(), a)
    want = sum(-math.log(j - i) * (j - i) ** -2.0 * weights[i, j].item() for i in range(6) for j in range(i + 1, 6))
    assert math.isfinite(g.item()) and abs(g.item() - want) <= 1e-14 * abs(weights).sum().item()
    with pytest.raises(ValueError):
        power_law_couplings(1, 2.0)


def test_ring_structure_factor_against_direct_sums():
    for L in (2, 5, 8):
        C = normal_vector(L * L, 2500 + L).reshape(L, L)
        got = ring_structure_factor(torch.from_numpy(C.copy()))
        want = np.array([sum(math.cos(2 * math.pi * k * (i - j) / L) * C[i, j] for i in range(L) for j in range(L)) / L
                         for k in range(L)])
        assert got.shape == (L,)
        assert np.max(np.abs(got.numpy() - want)) <= 1e-14 * np.abs(C).sum()
    with pytest.raises(ValueError):
        ring_structure_factor(torch.zeros(3, 4, dtype=torch.float64))


class _HostPairOperator(SpinSectorPairOperator):
    """the host-side plumbing of the class (pack, unpack, pairs) without a device: no tables, no handle"""

    def __init__(self, L, ndown):
        self.N, self.ndown = L, ndown
        self.npair = pair_count(L)
        self.nparam = 2 * self.npair + L
        self.device = torch.device("cpu")
        self._pairs = tuple((i, j) for i in range(L) for j in range(i + 1, L))
        self._upper = None


def test_pack_reads_the_strict_upper_triangle_differentiably():
    L = 6
    op = _HostPairOperator(L, 3)
    P = op.npair
    assert op.pairs == ref.pairs(L) and op.pair_index(4, 2) == ref.pair_index(L, 2, 4)
    A = torch.from_numpy(normal_vector(L * L, 2600).copy()).reshape(L, L).requires_grad_(True)
    B = torch.from_numpy(normal_vector(L * L, 2601).copy()).reshape(L, L)
    hz = torch.from_numpy(normal_vector(L, 2602).copy())
    p = op.pack(A, B, hz)
    assert p.shape == (2 * P + L,)
    assert np.array_equal(p.detach().numpy(), ref.pack_matrices(L, A.detach().numpy(), B.numpy(), hz.numpy()))
    weights = torch.from_numpy(normal_vector(2 * P + L, 2603).copy())
    (g,) = torch.autograd.grad((p * weights).sum(), A)
    want = np.zeros((L, L))
    for t, (i, j) in enumerate(ref.pairs(L)):
        want[i, j] = weights[t].item()
    assert np.array_equal(g.numpy(), want)              # the diagonal and the lower triangle are not read
    # scalars and vectors
    assert op.pack(1.0, 0.5, 0.25).tolist() == [1.0] * P + [0.5] * P + [0.25] * L
    vec = torch.arange(P, dtype=torch.float64)
    assert torch.equal(op.pack(vec, 2.0 * vec, 0.0)[:2 * P], torch.cat([vec, 2.0 * vec]))
    jxy, jz, h = op.unpack(p)
    assert jxy.numel() == jz.numel() == P and h.numel() == L and torch.equal(op.pack(jxy, jz, h), p)
    with pytest.raises(ValueError):
        op.pack(torch.zeros(L, L + 1, dtype=torch.float64), 0.0, 0.0)
    with pytest.raises(ValueError):
        op.unpack(torch.zeros(2 * P + L + 1, dtype=torch.float64))


@pytest.mark.parametrize("L,ndown", [(1, 1), (41, 20), (0, 0), (8, 0), (8, 8), (8, -1), (8, 9), (34, 17), (40, 20)])
def test_python_argument_checks_fire_before_the_device(L, ndown, monkeypatch):
    """no GPU here: a check that came after the first device call would raise something else than ValueError"""

    def no_device(*args, **kwargs):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(operators._lib, "load", no_device)
    monkeypatch.setattr(torch, "empty", no_device)
    monkeypatch.setattr(torch, "zeros", no_device)
    with pytest.raises(ValueError):
        SpinSectorPairOperator(L, None, ndown, device="cuda")


def test_python_refuses_a_wrong_length_before_the_device(monkeypatch):
    def no_device(*args, **kwargs):
        raise AssertionError("the device was touched before the arguments were checked")

    wrong = torch.zeros(2 * 28 + 8 + 1, dtype=torch.float64)       # (made before the patch)
    monkeypatch.setattr(operators._lib, "load", no_device)
    monkeypatch.setattr(torch, "empty", no_device)
    with pytest.raises(ValueError):
        SpinSectorPairOperator(8, wrong, 4, device="cuda")


def test_python_refuses_a_host_device():
    with pytest.raises(ValueError):
        SpinSectorPairOperator(8, torch.zeros(2 * 28 + 8, dtype=torch.float64), 4, device="cpu")
    with pytest.raises(ValueError):
        SpinSectorPairOperator(8, torch.zeros(2 * 28 + 8, dtype=torch.float64), 4)        # a host tensor decides the device


def test_scratch_size_without_a_device():
    lib = _lib.load()
    cnt = c_int64()
    for L, ndown in ((2, 1), (7, 3), (18, 9), (24, 12), (40, 2), (33, 16)):
        assert lib.dsea_op_pairsector_forms_scratch_doubles(L, ndown, byref(cnt)) == 0
        P, rows = L * (L - 1) // 2, (math.comb(L, ndown) + 255) // 256
        assert cnt.value == P * min(4096, rows) + 4 * (P + L) * min(256, rows), (L, ndown)
    for L, ndown in ((1, 1), (41, 20), (8, 0), (8, 8), (8, -1), (34, 17), (40, 20), (35, 15)):
        assert lib.dsea_op_pairsector_forms_scratch_doubles(L, ndown, byref(cnt)) == _lib.ERR_ARG, (L, ndown)
    assert lib.dsea_op_pairsector_forms_scratch_doubles(8, 4, None) == _lib.ERR_ARG


def test_create_pairsector_validates_before_any_device_work():
    lib = _lib.load()
    h = c_void_p()
    dummy = (ctypes.c_double * 1600)()
    ptr = ctypes.cast(dummy, c_void_p)

    def create(L, ndown, c=ptr, states=ptr, lo=ptr, hi=ptr, out=byref(h)):
        return lib.dsea_op_create_pairsector(L, ndown, c, states, lo, hi, out)

    assert create(1, 1) == -1                       # L < 2
    assert create(41, 2) == -1                      # L > 40
    assert create(10, 0) == -1                      # ndown < 1
    assert create(10, 10) == -1                     # ndown > L - 1
    assert create(34, 17) == -1                     # n > 2^31 - 1
    assert create(40, 20) == -1
    assert create(10, 5, c=None) == -1              # null pointers, one at a time
    assert create(10, 5, states=None) == -1
    assert create(10, 5, lo=None) == -1
    assert create(10, 5, hi=None) == -1
    assert create(10, 5, out=None) == -1
    assert create(40, 2) == 0                       # 780 pairs, the cap of L
    assert lib.dsea_op_destroy(h) == 0
    assert create(17, 8) == 0                       # 136 pairs: more than a bond list holds; nothing is launched at creation
    n = c_int64()
    assert lib.dsea_op_dim(h, byref(n)) == 0 and n.value == math.comb(17, 8)
    assert lib.dsea_op_set_tuning(h, _lib.TUNE_TFIM_TILE_LOG2, 6) == 0       # this kind: log2 of the grid cap
    assert lib.dsea_op_set_tuning(h, _lib.TUNE_TFIM_TILE_LOG2, 13) == -1
    # the forms refuse null operands on the host; they refuse other kinds, and the other forms this kind
    assert lib.dsea_op_pairsector_forms(h, None, None, None, None, None) == -1
    assert lib.dsea_op_pairsector_forms(None, ptr, ptr, ptr, ptr, None) == -1
    assert lib.dsea_op_sector_forms(h, ptr, ptr, ptr, ptr, None) == _lib.ERR_ARG
    assert lib.dsea_op_destroy(h) == 0
    bonds = (ctypes.c_int32 * 2)(0, 1)
    assert lib.dsea_op_create_sector(10, 5, 1, bonds, ptr, ptr, ptr, ptr, byref(h)) == 0
    assert lib.dsea_op_pairsector_forms(h, ptr, ptr, ptr, ptr, None) == _lib.ERR_ARG
    assert lib.dsea_op_destroy(h) == 0


@pytest.mark.parametrize("L", [6, 8, 10, 12])
def test_haldane_shastry_closed_form(L):
    """E0 = -pi^2 (L + 5 / L) / 24 in S^z = 0, by dense eigh of the reference matrix; the ground state is simple"""
    p, want = ref.haldane_shastry(L)
    lam = np.linalg.eigvalsh(ref.dense(L, L // 2, p))
    print("L = %d: E0 = %.15f  closed form %.15f  gap %.3f" % (L, lam[0], want, lam[1] - lam[0]))
    assert abs(lam[0] - want) <= 1e-13 * abs(want)
    assert lam[1] - lam[0] > 0.3
