"""The pair and spin-flip maps between Hubbard sectors on the GPU (docs/design/41-hubbard-pair-ladder.md): k_hubbard_pair and
k_hubbard_pair_forms against the numpy reference of tests/hubbard_pair_reference.py at the smallest sizes that reach each path,
the transpose bit for bit, the existing single-species kernels composed, autograd, and the physics end to end.

The error bound of a row is derived, not measured: the kernel adds the m = mu md products of a row with fma, so
|y - y_ref| <= (m + 2) 2^-53 (|P| |x|)_row.  m is the number of terms of a row, the same for every row: nup' ndn' of the
destination when both steps create, with L - nup' (L - ndn') in place of the count of a species whose step annihilates (its
qualifying sites are the empty ones).  A form is a sum over the rows as well: the same bound with the number of rows added to
m, on the sum of |v1| |v2| over the form's terms.

    L      (nup, ndn) src -> dst             n_src -> n_dst          what it reaches
    2..5   every admissible case             up to 100 -> 100        n_dst < 256 (one partial block), nup = ndn (one table set
                                                                     serves both species), every step pair and both orders
    9      (4,3) -> (5,4) (5,2) (3,4) (3,2)  10 584 -> 3024 .. 15 876  odd L (Llo = 5), three chunks of sites, 12 .. 63 blocks
    10     (5,5) -> (6,6) (6,4) (4,6) (4,4)  63 504 -> 44 100        two slot chunks per stripe, strides 252 -> 210, 173 blocks
    10     (5,5) -> (6,6) on 64 blocks       63 504 -> 44 100        173 row ranges on a grid capped at 64 blocks: blocks walk ranges
    40     (1,1) -> (2,2)                    1600 -> 608 400         shifts past bit 31, ten chunks of sites, 1600 forms
    40     (2,2) -> (1,1)                    608 400 -> 1600         39 slots per thread: the largest dynamic LDS (62 720 bytes)
    40     (1,2) -> (2,1)                    31 200 -> 31 200        a spin flip, 39 slots, odd nup behind the down operator
    8      (4,3) -> the four neighbours      against sum_i HubbardLadder(e_i, HubbardLadder(W[i], x)) on the device
"""
import functools
import importlib.util
import math
import os
from ctypes import c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hubbard_pair_reference as ref  # noqa: E402
import hubbard_reference as hub  # noqa: E402
from helpers import PatchRandn  # noqa: E402
from dominantsparseeigenad_amd import _lib, engine  # noqa: E402
from dominantsparseeigenad_amd.chebyshev import coupling_bound  # noqa: E402
from dominantsparseeigenad_amd.operators import (HubbardLadder, HubbardOperator, HubbardPairLadder, bond_pairing,  # noqa: E402
                                                 one_body_density_matrix, onsite_pairing, pair_correlations, ring_bonds,
                                                 total_spin)
from dominantsparseeigenad_amd.spectral import hubbard_pair_spectral_function  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402
import dominantsparseeigenad_amd.symeig as symeig  # noqa: E402
import dominantsparseeigenad_amd.CG as CG  # noqa: E402

F64 = torch.float64
EPS = 2.0 ** -53
STEPS = ((1, 1), (1, -1), (-1, 1), (-1, -1))
ORDERS = ("up_left", "dn_left")


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


def to_dev(a):
    return torch.from_numpy(np.array(a)).to(dev())      # (a copy: the cached case arrays are read-only)


def admissible(L):
    return [(nup, ndn, su, sd) for nup in range(1, L) for ndn in range(1, L) for su, sd in STEPS
            if 1 <= nup + su <= L - 1 and 1 <= ndn + sd <= L - 1]


@functools.lru_cache(maxsize=None)
def sector(L, nup, ndn):
    """one table set per sector for the whole module (zero couplings on a ring: only the tables are used)"""
    bonds = ring_bonds(L) if L > 2 else [(0, 1)]
    return HubbardOperator(L, bonds, torch.zeros(2 * len(bonds) + 2 * L, dtype=F64, device=dev()), nup, ndn)


def pair(L, nup, ndn, su, sd, order=0):
    return HubbardPairLadder(sector(L, nup, ndn), sector(L, nup + su, ndn + sd), ORDERS[order])


def terms(L, nup, ndn, su, sd):
    """the m of the bound: the qualifying sites of the up word times those of the down word of a destination row"""
    nu, nd = nup + su, ndn + sd
    return (nu if su > 0 else L - nu) * (nd if sd > 0 else L - nd)


@functools.lru_cache(maxsize=None)
def case(L, nup, ndn, su, sd):
    """(W, x, v1, P(W) x at order 0, |P| |x|, the forms of (v1, x) at order 0, their absolute sums) on the host, computed once
    per case and never written to; order 1 is the exact negative"""
    n_src, n_dst = ref.sizes(L, nup, ndn, su, sd)
    W = normal_vector(L * L, 9500 + L).reshape(L, L)
    x, v1 = normal_vector(n_src, 9510 + L + n_src % 97), normal_vector(n_dst, 9520 + L + n_dst % 97)
    out = (W, x, v1, ref.apply(L, nup, ndn, su, sd, 0, W, x), ref.apply_abs(L, nup, ndn, su, sd, W, x),
           ref.forms(L, nup, ndn, su, sd, 0, v1, x), ref.forms_abs(L, nup, ndn, su, sd, v1, x))
    for arr in out:
        arr.setflags(write=False)
    return out


def check(L, nup, ndn, su, sd, order, lad=None, label=""):
    """apply and forms of one case against the reference within the derived bounds; the forms twice, bit for bit.  Returns
    (y, forms) on the device."""
    W, x, v1, y_ref, y_abs, f_ref, f_abs = case(L, nup, ndn, su, sd)
    sign = -1.0 if order else 1.0
    lad = lad or pair(L, nup, ndn, su, sd, order)
    assert (lad.L, lad.steps, lad.order, lad.n_src, lad.n_dst) == (L, (su, sd), ORDERS[order], x.size, y_ref.size)
    m = terms(L, nup, ndn, su, sd)
    Wd, xd, v1d = to_dev(W), to_dev(x), to_dev(v1)
    y = lad(Wd, xd)
    assert y.shape == (lad.n_dst,) and y.dtype == F64
    excess = np.abs(y.cpu().numpy() - sign * y_ref) - (m + 2) * EPS * y_abs
    forms = lad.forms(v1d, xd)
    assert forms.shape == (L, L) and torch.equal(forms, lad.forms(v1d, xd))       # fixed-order sums, no atomics
    fexcess = np.abs(forms.cpu().numpy() - sign * f_ref) - (m + lad.n_dst + 2) * EPS * f_abs
    if label:
        ratio = float(np.max(np.abs(y.cpu().numpy() - sign * y_ref) / np.maximum((m + 2) * EPS * y_abs, 1e-300)))
        fratio = float(np.max(np.abs(forms.cpu().numpy() - sign * f_ref) / np.maximum((m + lad.n_dst + 2) * EPS * f_abs, 1e-300)))
        print("%s: worst |y - ref| / bound = %.3f, worst |form - ref| / bound = %.3f (m = %d)" % (label, ratio, fratio, m))
    assert excess.max() <= 0.0, (L, nup, ndn, su, sd, order, float(excess.max()))
    assert fexcess.max() <= 0.0, (L, nup, ndn, su, sd, order, float(fexcess.max()))
    return y, forms


@pytest.mark.parametrize("L", [2, 3, 4, 5])
def test_every_small_case_against_the_reference_and_the_transpose_bit_for_bit(L):
    cases = admissible(L)
    assert len(cases) == {2: 0, 3: 4, 4: 16, 5: 36}[L]
    for nup, ndn, su, sd in cases:
        W = case(L, nup, ndn, su, sd)[0]
        want = ref.dense(L, nup, ndn, su, sd, 0, W)
        for order in (0, 1):
            lad = pair(L, nup, ndn, su, sd, order)
            check(L, nup, ndn, su, sd, order, lad)
            P = lad.dense(to_dev(W))
            assert torch.equal(P, to_dev(-want if order else want))          # each entry is a single +-W_ij
            assert torch.equal(lad.T.dense(to_dev(W)), P.T.contiguous())
    if cases:
        # an (L,) vector of weights means its diagonal
        nup, ndn, su, sd = cases[0]
        lad, x = pair(L, nup, ndn, su, sd), to_dev(case(L, nup, ndn, su, sd)[1])
        w = to_dev(normal_vector(L, 9530))
        assert torch.equal(lad(w, x), lad(torch.diag(w), x))


MEDIUM = [(9, 4, 3), (10, 5, 5)]


@pytest.mark.parametrize("su,sd", STEPS)
@pytest.mark.parametrize("L,nup,ndn", MEDIUM)
def test_more_than_one_chunk_and_more_than_one_block(L, nup, ndn, su, sd):
    order = (su + sd) // 2 % 2                         # both orders are met over the four step pairs
    lad = pair(L, nup, ndn, su, sd, order)
    assert lad.n_dst > 2 * 256 and L > 8 and (L + 1) // 2 == 5
    y, _ = check(L, nup, ndn, su, sd, order, lad, label="L = %d (%d, %d) -> (%d, %d)" % (L, nup, ndn, nup + su, ndn + sd))
    # nothing is written past the last row: a longer output filled with a sentinel, through the C entry
    W, x = case(L, nup, ndn, su, sd)[:2]
    Wd, xd = to_dev(W), to_dev(x)
    out = torch.full((lad.n_dst + 67,), -7.0, dtype=F64, device=dev())
    rc = _lib.load().dsea_hubbard_pair_apply(*lad._sector_args(), c_void_p(Wd.data_ptr()),
                                             *[c_void_p(t.data_ptr()) for t in lad._tables], c_void_p(xd.data_ptr()),
                                             c_void_p(out.data_ptr()), 0, engine._stream(dev()))
    assert rc == 0
    assert torch.equal(out[:lad.n_dst], y) and bool((out[lad.n_dst:] == -7.0).all())
    # <v1, P x> = <P^T v1, x> through the transposed map
    v1 = to_dev(case(L, nup, ndn, su, sd)[2])
    back = lad.T(Wd, v1)
    assert abs(float(v1 @ y) - float(back @ xd)) <= 1e-13 * float(v1.norm() * y.norm() + back.norm() * xd.norm())


def test_the_grid_stride():
    """(5, 5) -> (6, 6) at L = 10: 44 100 rows are 173 ranges of 256 on 64 blocks.  The map is one row per thread whatever the
    grid: the same bits.  The forms sum other partials: within the bound."""
    L, nup, ndn, su, sd = 10, 5, 5, 1, 1
    lad = pair(L, nup, ndn, su, sd)
    assert lad.n_dst == 44100 > 64 * 256
    W, x = case(L, nup, ndn, su, sd)[:2]
    y = lad(to_dev(W), to_dev(x))
    lad.set_grid_log2(6)
    try:
        y6, _ = check(L, nup, ndn, su, sd, 0, lad, label="L = 10 on 64 blocks")
    finally:
        lad.set_grid_log2(0)
    assert torch.equal(y6, y)


@pytest.mark.parametrize("nup,ndn,su,sd", [(1, 1, 1, 1), (2, 2, -1, -1), (1, 2, 1, -1)])
def test_forty_sites(nup, ndn, su, sd):
    L = 40
    assert max(hub.states(L, nup + su)) >= 1 << 32
    check(L, nup, ndn, su, sd, 0, label="L = 40 (%d, %d) -> (%d, %d)" % (nup, ndn, nup + su, ndn + sd))


@pytest.mark.parametrize("su,sd", STEPS)
def test_against_the_single_species_kernels_composed(su, sd):
    """L = 8 from (4, 3): order 0 is the down ladder first, then the up ladder with one-hot weights, summed over the up site.
    Either side is within its bound of the exact result: twice the bound between them."""
    L, nup, ndn = 8, 4, 3
    W, x, _, _, y_abs = case(L, nup, ndn, su, sd)[:5]
    Wd, xd = to_dev(W), to_dev(x)
    down = HubbardLadder(sector(L, nup, ndn), sector(L, nup, ndn + sd), "dn")
    up = HubbardLadder(sector(L, nup, ndn + sd), sector(L, nup + su, ndn + sd), "up")
    eye = torch.eye(L, dtype=F64, device=dev())
    want = sum(up(eye[i], down(Wd[i], xd)) for i in range(L))
    got = pair(L, nup, ndn, su, sd)(Wd, xd)
    m = terms(L, nup, ndn, su, sd)
    excess = np.abs((got - want).cpu().numpy()) - 2 * (m + 2) * EPS * y_abs
    assert excess.max() <= 0.0 and float(got.norm()) > 0.0
    assert torch.equal(pair(L, nup, ndn, su, sd, 1)(Wd, xd), -got)


def test_gradcheck_and_gradgradcheck():
    """L = 4, (2, 2) -> (1, 1) and the spin flip (2, 2) -> (3, 1), with torch's defaults as everywhere in this suite"""
    L = 4
    for su, sd, order in ((-1, -1, 1), (1, -1, 0)):
        lad = pair(L, 2, 2, su, sd, order)
        W = to_dev(normal_vector(L * L, 9540).reshape(L, L)).requires_grad_(True)
        x = to_dev(normal_vector(lad.n_src, 9541)).requires_grad_(True)
        v1 = to_dev(normal_vector(lad.n_dst, 9542)).requires_grad_(True)
        assert torch.autograd.gradcheck(lad, (W, x))
        assert torch.autograd.gradgradcheck(lad, (W, x))
        assert torch.autograd.gradcheck(lad.forms, (v1, x))
        assert torch.autograd.gradgradcheck(lad.forms, (v1, x))


def ring_couplings(L, t, U, eps=None):
    return np.concatenate([t * np.ones(L), np.zeros(L), U * np.ones(L), np.zeros(L) if eps is None else eps])


def five_point(f, U, h):
    return (f(U - 2 * h) - 8 * f(U - h) + 8 * f(U + h) - f(U + 2 * h)) / (12 * h)


def through_the_eigensolver(L, nup, ndn, t, U0, eps, measure, seed):
    """(value, d value / dU) of measure(op, psi0) with psi0 from DominantSparseSymeig at U0"""
    bonds = ring_bonds(L)
    U = torch.tensor(U0, dtype=F64, device=dev(), requires_grad=True)
    p0, dU = to_dev(ring_couplings(L, t, 0.0, eps)), to_dev(ring_couplings(L, 0.0, 1.0))
    op = HubbardOperator(L, bonds, p0 + U * dU, nup, ndn)
    symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
    with PatchRandn(seed):
        _, psi0 = symeig.DominantSparseSymeig.apply(op.couplings, 200, op.dim)
        value = measure(op, psi0)
        (grad,) = torch.autograd.grad(value, U)
    return value.item(), grad.item()


def test_the_gradient_of_the_pair_correlations_through_the_eigensolver(monkeypatch):
    """d/dU of P_00 + P_01 + P_11 / 2 (on-site and nearest-neighbour singlet fields) at U = 4 on the ring L = 6, (3, 3), against
    the five-point central difference of the dense reference with h = 1e-3: the finite-difference tolerance of
    tests/test_gpu_hubbard_ladder.py, 5e-9 absolute, and its reasoning (the values are of order one)."""
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, h = 6, 1e-3
    bonds = ring_bonds(L)
    fields = [onsite_pairing(L).numpy(), bond_pairing(L, bonds, torch.ones(L, dtype=F64)).numpy()]

    def combine(P):
        return P[0, 0] + P[0, 1] + 0.5 * P[1, 1]

    def dense(U):
        E, V = np.linalg.eigh(hub.dense(L, 3, 3, bonds, ring_couplings(L, 1.0, U)))
        assert E[1] - E[0] > 0.1
        C = np.array([ref.apply(L, 3, 3, -1, -1, 1, W, V[:, 0]) for W in fields])
        return float(combine(C @ C.T))

    want = five_point(dense, 4.0, h)
    stack = to_dev(np.stack(fields))
    value, got = through_the_eigensolver(L, 3, 3, 1.0, 4.0, None, lambda op, psi: combine(pair_correlations(op, psi, stack)), 9550)
    print("pair correlations: %.12f (|dev| %.2e)   d/dU = %.10f against the central difference %.10f: |dev| = %.2e (bound 5e-9)"
          % (value, abs(value - dense(4.0)), got, want, abs(got - want)))
    assert abs(value - dense(4.0)) <= 1e-10 and abs(want) > 1e-3
    assert abs(got - want) <= 5e-9


def test_the_gradient_of_the_total_spin_through_the_eigensolver(monkeypatch):
    """ring L = 6 at (2, 3) with random eps (a non-degenerate ground state), t = 1.3, U = 2.5: <S^2> = 3/4 whatever U, since H
    commutes with S; S+ psi0 has norm 1, so the backward pass runs through non-zero vectors and has to cancel.  Against the
    five-point central difference of the dense reference, the same tolerance as above."""
    monkeypatch.setattr(CG, "EPS_DEFAULT", 1e-12)
    L, h, t = 6, 1e-3, 1.3
    eps = 0.3 * normal_vector(L, 9560)

    def dense(U):
        E, V = np.linalg.eigh(hub.dense(L, 2, 3, ring_bonds(L), ring_couplings(L, t, U, eps)))
        assert E[1] - E[0] > 0.05
        phi = ref.apply(L, 2, 3, 1, -1, 0, np.eye(L), V[:, 0])
        return float(phi @ phi) - 0.25

    want = five_point(dense, 2.5, h)
    value, got = through_the_eigensolver(L, 2, 3, t, 2.5, eps, total_spin, 9561)
    print("<S^2> = %.12f   d/dU = %.3e against the central difference %.3e (bound 5e-9)" % (value, got, want))
    assert abs(value - 0.75) <= 1e-10 and abs(dense(2.5) - 0.75) <= 1e-12
    assert abs(got - want) <= 5e-9


# ---------------------------------------------------------------------------------------------- the physics, psi0 from host eigh
def host_ground_state(op):
    """(E, psi0, gap) from a host eigh of the operator's own matrix, op.to_csr() applied to the identity: only rounding remains"""
    csr = op.to_csr()
    eye = torch.eye(op.n, dtype=F64, device=dev())
    H = torch.stack([csr(eye[j]) for j in range(op.n)], dim=1).cpu().numpy()
    assert np.max(np.abs(H - H.T)) <= 1e-15
    E, V = np.linalg.eigh(H)
    return E, to_dev(V[:, 0]), E[1] - E[0]


def ring_operator(L, nup, ndn, t, U):
    return HubbardOperator(L, ring_bonds(L), to_dev(ring_couplings(L, t, U)), nup, ndn)


def test_the_eta_pairing_pole():
    """ring L = 6, t = 1.3, U = 5, eta+ = Delta+(diag (-1)^i) added to the ground state of (2, 2): [H, eta+] = U eta+, so all the
    weight |eta+ psi0|^2 sits in one pole at omega = U, within 64 * 2^-53 * coupling_bound"""
    L, t, U = 6, 1.3, 5.0
    op = ring_operator(L, 2, 2, t, U)
    target = ring_operator(L, 3, 3, t, U)
    E, psi0, _ = host_ground_state(op)
    eta = onsite_pairing(L, (-1.0) ** np.arange(L))
    tol = 64 * EPS * coupling_bound(target)
    want = float(np.sum(ref.apply(L, 2, 2, 1, 1, 0, eta.numpy(), psi0.cpu().numpy()) ** 2))
    for kwargs in (dict(target=target), dict(), dict(target=target, basis_free=True)):
        m = hubbard_pair_spectral_function(op, psi0, E[0], eta, "pair_add", k=20, **kwargs)
        top = int(m.weights.argmax())
        rest = float(m.weights.sum() - m.weights[top])
        print("eta: |eta+ psi0|^2 = %.15f (reference %.15f), pole %.15f, weight elsewhere %.2e (tol %.2e)"
              % (m.moment(0), want, float(m.poles[top]), rest, tol))
        assert want > 0.1 and abs(m.moment(0) - want) <= tol * want
        assert abs(float(m.poles[top]) - U) <= tol and rest <= tol * want
    # the (L,) vector form of the weights and a complex field: the two parts' measures add
    m = hubbard_pair_spectral_function(op, psi0, E[0], torch.complex(eta.diagonal(), 2.0 * eta.diagonal()), "pair_add", k=20,
                                       target=target)
    assert abs(m.moment(0) - 5.0 * want) <= 5.0 * tol * want


@pytest.mark.parametrize("nup,ndn,t,U,want", [(2, 2, 1.3, 5.0, 2.0), (2, 3, 1.3, 2.5, 0.75), (3, 3, 1.0, 4.0, 0.0)])
def test_total_spin_of_ring_ground_states(nup, ndn, t, U, want):
    op = ring_operator(6, nup, ndn, t, U)
    _, psi0, _ = host_ground_state(op)
    s2 = float(total_spin(op, psi0))
    print("(%d, %d): <S^2> = %.16g" % (nup, ndn, s2))
    assert abs(s2 - want) <= 1e-12
    # from the other side: S^2 = |S- psi|^2 + S^z (S^z - 1)
    other = float(total_spin(op, psi0, target=sector(6, nup - 1, ndn + 1)))
    assert abs(other - want) <= 1e-12


def test_total_spin_where_only_one_side_exists():
    """(3, 1) on four sites: S+ psi would live in (4, 0), which is no sector of the library: S- from the other side"""
    L = 4
    op = HubbardOperator(L, ring_bonds(L), to_dev(ring_couplings(L, 1.0, 3.0, 0.2 * normal_vector(L, 9570))), 3, 1)
    _, psi0, gap = host_ground_state(op)
    assert gap > 1e-3
    s2 = float(total_spin(op, psi0))
    assert min(abs(s2 - s * (s + 1)) for s in (1.0, 2.0)) <= 1e-12          # S^z = 1: S is 1 or 2


def test_wick_through_pair_correlations_and_the_density_matrix():
    """U = V = 0 on the open chain L = 6 at (3, 3) with small random eps: P_ab = sum W_a,ij W_b,kl rho_up[i, k] rho_dn[j, l]"""
    L = 6
    bonds = [(i, i + 1) for i in range(L - 1)]
    p = np.concatenate([np.ones(L - 1), np.zeros(L - 1), np.zeros(L), 0.05 * normal_vector(L, 9760)])
    op = HubbardOperator(L, bonds, to_dev(p), 3, 3)
    _, psi0, gap = host_ground_state(op)
    assert gap > 0.5
    fields = to_dev(np.stack([normal_vector(L * L, 9580 + a).reshape(L, L) for a in range(3)]))
    P = pair_correlations(op, psi0, fields)
    up, dn = one_body_density_matrix(op, psi0, "up"), one_body_density_matrix(op, psi0, "dn")
    want = torch.einsum("aij,bkl,ik,jl->ab", fields, fields, up, dn)
    scale = float(fields.flatten(1).norm(dim=1).max()) ** 2
    print("Wick: max |P - rho rho| = %.2e" % float((P - want).abs().max()))
    assert P.shape == (3, 3) and torch.equal(P, P.T) and float((P - want).abs().max()) <= 1e-12 * scale
    again = pair_correlations(op, psi0, fields, target=sector(L, 2, 2))
    assert torch.equal(again, P)


def test_example_pairing():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "hubbard", "pairing.py")
    spec = importlib.util.spec_from_file_location("hubbard_pairing", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    orig = CG.EPS_DEFAULT
    try:
        out = ex.main(L=6)
    finally:
        CG.EPS_DEFAULT = orig
    assert out["L"] == 6 and len(out["U"]) == 4
    for name in ("ring", "chain"):
        onsite = [row["onsite"] for row in out["pair"][name]]
        assert all(math.isfinite(v) and v > 0.0 for v in onsite)
        assert all(a > b for a, b in zip(onsite, onsite[1:]))                 # a repulsive U suppresses the on-site pairs
        assert all(row["bond"] > 0.0 for row in out["pair"][name])
    assert [round(row["S2"], 6) for row in out["spin"]] == [0.0, 0.75, 2.0, 0.75]
    for row in out["eta"]:
        assert abs(row["pole"] - row["U"]) <= 1e-8 and abs(row["weight"] - row["total"]) <= 1e-8 * row["total"]
