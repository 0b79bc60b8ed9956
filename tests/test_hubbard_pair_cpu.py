"""The pair and spin-flip maps between Hubbard sectors without a GPU (docs/design/41-hubbard-pair-ladder.md): the numpy reference
of tests/hubbard_pair_reference.py against the Jordan-Wigner operators on 2 L modes and against compositions of the
single-species ladder reference, the identities the GPU tests rely on (the two orders, the transpose, the forms), the physics
(eta pairing, spin rotation invariance, <S^2> of ground states, Wick's theorem for free fermions), and the argument checks of
the Python layer and of the C ABI that need no device."""
import types
from ctypes import byref, c_int64, c_void_p

import numpy as np
import pytest
import torch

import hubbard_ladder_reference as lad_ref
import hubbard_pair_reference as ref
import hubbard_reference as hub
from hubbard_ladder_reference import DN, UP
from dominantsparseeigenad_amd import _lib
from dominantsparseeigenad_amd.operators import (HubbardPairLadder, bond_pairing, onsite_pairing, pair_correlations, ring_bonds,
                                                 total_spin)
from dominantsparseeigenad_amd.spectral import hubbard_pair_spectral_function
from dominantsparseeigenad_amd.synthetic import normal_vector

EPS = 2.0 ** -53
STEPS = ((1, 1), (1, -1), (-1, 1), (-1, -1))


def admissible(L):
    """every (nup, ndn, su, sd) whose two sectors the library accepts: 1 <= count <= L - 1 on both sides"""
    return [(nup, ndn, su, sd) for nup in range(1, L) for ndn in range(1, L) for su, sd in STEPS
            if 1 <= nup + su <= L - 1 and 1 <= ndn + sd <= L - 1]


def weights(L, seed=0):
    return normal_vector(L * L, 9700 + L + seed).reshape(L, L)


def sector_index(L, nup, ndn):
    """the Jordan-Wigner index u | d << L of every row of the sector, in row order"""
    return np.array([u | (d << L) for u in hub.states(L, nup) for d in hub.states(L, ndn)], dtype=np.int64)


def full_operator(L, su, sd, order, W):
    """sum_ij W_ij A_i B_{L + j} (order 0) or sum_ij W_ij B_{L + j} A_i (order 1) on 2 L modes"""
    M = 2 * L
    c = [hub._annihilator(M, q) for q in range(M)]
    out = np.zeros((1 << M, 1 << M))
    for i in range(L):
        A = c[i].T if su > 0 else c[i]
        for j in range(L):
            B = c[L + j].T if sd > 0 else c[L + j]
            out += W[i, j] * (A @ B if order == 0 else B @ A)
    return out


def test_the_admissible_cases():
    assert [len(admissible(L)) for L in (2, 3, 4, 5)] == [0, 4, 16, 36]


@pytest.mark.parametrize("L", [2, 3, 4])
def test_reference_is_the_block_of_the_jordan_wigner_operator(L):
    W = weights(L)
    worst, cases = 0.0, admissible(L)
    for su, sd in STEPS:
        for order in (0, 1):
            full = full_operator(L, su, sd, order, W)
            for nup, ndn, a, b in cases:
                if (a, b) != (su, sd):
                    continue
                src, dst = sector_index(L, nup, ndn), sector_index(L, nup + su, ndn + sd)
                S = ref.dense(L, nup, ndn, su, sd, order, W)
                assert S.shape == (len(dst), len(src)) == ref.sizes(L, nup, ndn, su, sd)[::-1]
                dev = float(np.max(np.abs(S - full[np.ix_(dst, src)])))
                worst = max(worst, dev)
                assert dev <= 1e-14 * np.abs(W).sum(), (nup, ndn, su, sd, order, dev)
                # the operator maps the source sector into the destination only: exactly zero everywhere else
                rest = np.setdiff1d(np.arange(1 << (2 * L)), dst)
                assert not full[np.ix_(rest, src)].any()
    print("L = %d: %d cases, worst |reference - Jordan-Wigner block| = %.2e" % (L, 2 * len(cases), worst))


@pytest.mark.parametrize("L", [3, 4, 5])
def test_reference_is_the_composition_of_two_single_species_ladders(L):
    """order 0: the down ladder first, from (nup, ndn), then the up ladder from (nup, ndn + sd); order 1 the other way round.
    One (row, column) pair fixes (i, j), so every entry of either side is a single +-W_ij."""
    W = weights(L, 1)
    eye = np.eye(L)
    for nup, ndn, su, sd in admissible(L):
        want0 = sum(lad_ref.dense(L, nup, ndn + sd, UP, su, eye[i]) @ lad_ref.dense(L, nup, ndn, DN, sd, W[i]) for i in range(L))
        want1 = sum(lad_ref.dense(L, nup + su, ndn, DN, sd, W[i]) @ lad_ref.dense(L, nup, ndn, UP, su, eye[i]) for i in range(L))
        for order, want in ((0, want0), (1, want1)):
            got = ref.dense(L, nup, ndn, su, sd, order, W)
            assert np.max(np.abs(got - want)) <= 1e-14 * np.abs(W).sum(), (nup, ndn, su, sd, order)


@pytest.mark.parametrize("L", [3, 4, 5])
def test_the_two_orders_and_the_transpose_are_exact(L):
    W = weights(L, 2)
    for nup, ndn, su, sd in admissible(L):
        P0, P1 = (ref.dense(L, nup, ndn, su, sd, order, W) for order in (0, 1))
        assert P0.any() and np.array_equal(P1, -P0)
        for order, P in ((0, P0), (1, P1)):
            back = ref.dense(L, nup + su, ndn + sd, -su, -sd, 1 - order, W)
            assert np.array_equal(back, P.T)               # bit for bit: the entries are +-W_ij themselves
        assert np.array_equal(np.abs(P0), ref.dense_abs(L, nup, ndn, su, sd, W))


@pytest.mark.parametrize("L", [3, 4])
def test_apply_and_forms_are_the_dense_matrix(L):
    W = weights(L, 3)
    for nup, ndn, su, sd in admissible(L):
        n_src, n_dst = ref.sizes(L, nup, ndn, su, sd)
        v1, v2 = normal_vector(n_dst, 9800 + n_dst), normal_vector(n_src, 9900 + n_src)
        for order in (0, 1):
            P = ref.dense(L, nup, ndn, su, sd, order, W)
            bound = 1e-14 * np.abs(W).sum() * np.linalg.norm(v1) * np.linalg.norm(v2)
            assert np.max(np.abs(ref.apply(L, nup, ndn, su, sd, order, W, v2) - P @ v2)) <= bound
            got = ref.forms(L, nup, ndn, su, sd, order, v1, v2)
            want = np.array([[v1 @ ref.dense(L, nup, ndn, su, sd, order, np.outer(np.eye(L)[i], np.eye(L)[j])) @ v2
                              for j in range(L)] for i in range(L)])
            assert np.max(np.abs(got - want)) <= bound
            assert abs(np.sum(got * W) - v1 @ P @ v2) <= bound
        Pa = ref.dense_abs(L, nup, ndn, su, sd, W)
        assert np.max(np.abs(ref.apply_abs(L, nup, ndn, su, sd, W, v2) - Pa @ np.abs(v2))) <= 1e-14 * np.abs(W).sum() * np.linalg.norm(v2)
        assert np.all(ref.forms_abs(L, nup, ndn, su, sd, v1, v2) >= np.abs(ref.forms(L, nup, ndn, su, sd, 0, v1, v2)))


def ring(L, nup, ndn, t, U):
    bonds = ring_bonds(L)
    p = np.concatenate([t * np.ones(L), np.zeros(L), U * np.ones(L), np.zeros(L)])
    return hub.dense(L, nup, ndn, bonds, p)


@pytest.mark.parametrize("nup,ndn", [(1, 1), (2, 2), (2, 3)])
def test_eta_pairing_on_the_ring(nup, ndn):
    """L = 6 is bipartite: with eta+ = Delta+(diag (-1)^i), [H, eta+] = U eta+ (Yang), through the sector blocks
    H' eta+ - eta+ H = U eta+.  Every entry of the three products is a sum of at most 2 L + 1 terms t or U: the bound."""
    L, t, U = 6, 1.3, 5.0
    eta = ref.dense(L, nup, ndn, 1, 1, 0, np.diag((-1.0) ** np.arange(L)))
    H, Hp = ring(L, nup, ndn, t, U), ring(L, nup + 1, ndn + 1, t, U)
    res = float(np.max(np.abs(Hp @ eta - eta @ H - U * eta)))
    print("(%d, %d): |H' eta+ - eta+ H - U eta+| = %.2e" % (nup, ndn, res))
    assert eta.any() and res <= (4 * L + 2) * EPS * (abs(t) + abs(U))


@pytest.mark.parametrize("L,nup,ndn", [(5, 2, 2), (5, 1, 3), (6, 3, 2)])
def test_the_hamiltonian_commutes_with_the_total_spin(L, nup, ndn):
    """random t, V, U_i and eps_i: every term of H is a spin singlet, so H' S+ = S+ H through the sector blocks"""
    bonds = ring_bonds(L) + [(0, 2)]
    p = normal_vector(hub.nparam(L, bonds), 9750 + L + nup)
    H, Hp = hub.dense(L, nup, ndn, bonds, p), hub.dense(L, nup + 1, ndn - 1, bonds, p)
    Sp = ref.dense(L, nup, ndn, 1, -1, 0, np.eye(L))
    assert Sp.any() and np.max(np.abs(Hp @ Sp - Sp @ H)) <= 64 * EPS * np.abs(p).sum()
    # ... and S- is its transpose, the other order from the other side
    assert np.array_equal(ref.dense(L, nup + 1, ndn - 1, -1, 1, 1, np.eye(L)), Sp.T)


def spin_squared(L, nup, ndn, psi):
    phi = ref.apply(L, nup, ndn, 1, -1, 0, np.eye(L), psi)
    sz = 0.5 * (nup - ndn)
    return phi @ phi + sz * (sz + 1.0)


@pytest.mark.parametrize("nup,ndn,t,U,want", [(2, 2, 1.3, 5.0, 2.0), (2, 3, 1.3, 2.5, 0.75), (3, 3, 1.0, 4.0, 0.0)])
def test_total_spin_of_ring_ground_states(nup, ndn, t, U, want):
    """ring L = 6: an open shell at (2, 2) (Hund: S = 1), one unpaired particle at (2, 3), a singlet at half filling (Lieb)"""
    L = 6
    E, V = np.linalg.eigh(ring(L, nup, ndn, t, U))
    s2 = spin_squared(L, nup, ndn, V[:, 0])
    print("(%d, %d): <S^2> = %.16g" % (nup, ndn, s2))
    assert abs(s2 - want) <= 1e-12


def open_chain_free(L, nup, ndn, seed):
    bonds = [(i, i + 1) for i in range(L - 1)]
    p = np.concatenate([np.ones(L - 1), np.zeros(L - 1), np.zeros(L), 0.05 * normal_vector(L, seed)])
    return bonds, p


def density_matrix(L, nup, ndn, species, psi):
    C = np.array([lad_ref.apply(L, nup, ndn, species, -1, np.eye(L)[i], psi) for i in range(L)])
    return C @ C.T


def test_wick_for_free_fermions():
    """U = V = 0 on the open chain L = 6 at (3, 3): the ground state is a product of two Slater determinants, so
    <Delta(W1) psi | Delta(W2) psi> = sum W1_ij W2_kl rho_up[i, k] rho_dn[j, l]"""
    L, nup, ndn = 6, 3, 3
    bonds, p = open_chain_free(L, nup, ndn, 9760)
    E, V = np.linalg.eigh(hub.dense(L, nup, ndn, bonds, p))
    assert E[1] - E[0] > 0.5
    psi = V[:, 0]
    W1, W2 = weights(L, 4), weights(L, 5)
    got = ref.apply(L, nup, ndn, -1, -1, 1, W1, psi) @ ref.apply(L, nup, ndn, -1, -1, 1, W2, psi)
    up, dn = density_matrix(L, nup, ndn, UP, psi), density_matrix(L, nup, ndn, DN, psi)
    want = np.einsum("ij,kl,ik,jl->", W1, W2, up, dn)
    print("Wick: %.14g against %.14g" % (got, want))
    assert abs(got - want) <= 1e-12 * np.linalg.norm(W1) * np.linalg.norm(W2)


def carrier(L, nup, ndn, device="cpu"):
    """what HubbardPairLadder reads of an operator, without a device"""
    return types.SimpleNamespace(N=L, nup=nup, ndn=ndn, device=torch.device(device), _up=(None, None, None),
                                 _dn=(None, None, None), bonds=((0, 1),), nparam=2 + 2 * L)


def test_value_errors_that_need_no_device():
    lad = HubbardPairLadder(carrier(6, 3, 3), carrier(6, 2, 2))
    assert (lad.order, lad.steps, lad.L, lad.n_src, lad.n_dst) == ("up_left", (-1, -1), 6, 400, 225)
    assert lad._sector_args() == (6, 3, 3, -1, -1, 0) and len(lad._tables) == 6
    back = lad.T
    assert (back.order, back.steps, back.n_src, back.n_dst) == ("dn_left", (1, 1), 225, 400) and back.T is lad
    assert back._sector_args() == (6, 2, 2, 1, 1, 1)
    flip = HubbardPairLadder(carrier(6, 3, 3), carrier(6, 4, 2), order="dn_left")
    assert (flip.order, flip.steps, flip.n_dst, flip.T.order, flip.T.steps) == ("dn_left", (1, -1), 225, "up_left", (-1, 1))
    # no block forms: the C entries do not exist, and neither do the methods
    assert not hasattr(lad, "apply_block") and not hasattr(lad, "block_dots")
    for name in ("apply", "forms", "forms_scratch_doubles"):
        assert "dsea_hubbard_pair_" + name in _lib.EXPORTED_SYMBOLS
    assert not [s for s in _lib.EXPORTED_SYMBOLS if s.startswith("dsea_hubbard_pair_block")]
    for src, dst, order in ((carrier(6, 3, 3), carrier(6, 3, 3), "up_left"),        # the same sector
                            (carrier(6, 3, 3), carrier(6, 2, 3), "up_left"),        # one species only
                            (carrier(6, 3, 3), carrier(6, 3, 4), "up_left"),
                            (carrier(6, 3, 3), carrier(6, 1, 2), "up_left"),        # two steps
                            (carrier(6, 3, 3), carrier(6, 4, 5), "up_left"),
                            (carrier(6, 3, 3), carrier(6, 2, 2), "left"),           # no such order
                            (carrier(6, 3, 3), carrier(6, 2, 2), 0),
                            (carrier(6, 3, 3), carrier(7, 2, 2), "up_left"),        # another L
                            (carrier(6, 5, 3), carrier(6, 6, 2), "up_left"),        # a destination with a full species
                            (carrier(6, 3, 1), carrier(6, 2, 0), "up_left"),        # ... and with an empty one
                            (carrier(41, 1, 1), carrier(41, 2, 2), "up_left"),      # L beyond the limit
                            (carrier(18, 8, 8), carrier(18, 9, 9), "up_left"),      # more than 2^31 - 1 rows
                            (carrier(6, 3, 3), carrier(6, 2, 2, "meta"), "up_left"),     # another device
                            (carrier(6, 3, 3), object(), "up_left")):               # no tables
        with pytest.raises(ValueError):
            HubbardPairLadder(src, dst, order)
    for g in (1, 5, 13, -1):
        with pytest.raises(ValueError):
            lad.set_grid_log2(g)
    lad.set_grid_log2(6)
    assert back._grid[0] == 6                               # one setting for the map and its transpose
    lad.set_grid_log2(0)
    x = torch.zeros(400, dtype=torch.float64)
    good = torch.zeros((6, 6), dtype=torch.float64)
    for W in (torch.zeros(5, dtype=torch.float64), torch.zeros((6, 5), dtype=torch.float64), torch.zeros((5, 5), dtype=torch.float64),
              torch.zeros((1, 6, 6), dtype=torch.float64), torch.zeros((6, 6), dtype=torch.complex128),
              torch.zeros(6, dtype=torch.complex128)):
        with pytest.raises(ValueError):
            lad(W, x)
    with pytest.raises(ValueError):
        lad(good, torch.zeros(225, dtype=torch.float64))    # a vector of the destination
    with pytest.raises(ValueError):
        lad.forms(x, x)                                     # v1 lives on the destination
    for W in (good, torch.zeros(6, dtype=torch.float64)):
        with pytest.raises(ValueError):
            lad(W, x)                                       # host tensors: the map is a device kernel, there is no fallback
    with pytest.raises(ValueError):
        lad.forms(torch.zeros(225, dtype=torch.float64), x)


def test_physics_helpers_without_a_device():
    assert torch.equal(onsite_pairing(4), torch.eye(4, dtype=torch.float64))
    assert torch.equal(onsite_pairing(3, [1, -1, 1]), torch.diag(torch.tensor([1.0, -1.0, 1.0], dtype=torch.float64)))
    amp = torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64, requires_grad=True)
    W = bond_pairing(4, [(0, 1), (1, 2), (1, 0)], amp)
    want = np.zeros((4, 4))
    want[0, 1] = want[1, 0] = 1.5 / np.sqrt(2.0)
    want[1, 2] = want[2, 1] = -2.0 / np.sqrt(2.0)
    assert W.shape == (4, 4) and np.allclose(W.detach().numpy(), want, rtol=0, atol=1e-16)
    W.sum().backward()
    assert np.allclose(amp.grad.numpy(), np.sqrt(2.0), rtol=1e-15)
    for bad in (lambda: onsite_pairing(0), lambda: onsite_pairing(3, [1, 1]), lambda: bond_pairing(3, [(0, 3)], [1.0]),
                lambda: bond_pairing(3, [(1, 1)], [1.0]), lambda: bond_pairing(3, [(0, 1)], [1.0, 2.0])):
        with pytest.raises(ValueError):
            bad()
    op = carrier(6, 3, 3)
    psi = torch.zeros(400, dtype=torch.float64)
    for pairings in (torch.zeros((6, 6), dtype=torch.float64), torch.zeros((2, 6, 5), dtype=torch.float64),
                     torch.zeros((0, 6, 6), dtype=torch.float64)):
        with pytest.raises(ValueError):
            pair_correlations(op, psi, pairings)
    with pytest.raises(ValueError):
        pair_correlations(op, psi, torch.zeros((1, 6, 6), dtype=torch.float64), target=carrier(6, 2, 3))
    with pytest.raises(ValueError, match="neither"):
        total_spin(carrier(2, 1, 1), torch.zeros(4, dtype=torch.float64))
    with pytest.raises(ValueError):
        total_spin(op, psi, target=carrier(6, 2, 2))
    for channel, target in (("pair", None), ("c_up", None), ("pair_add", carrier(6, 2, 2)), ("s_plus", carrier(6, 4, 4))):
        with pytest.raises(ValueError):
            hubbard_pair_spectral_function(op, psi, 0.0, torch.eye(6, dtype=torch.float64), channel, target=target)


def test_c_abi_argument_errors_without_a_device():
    """every refusal is host arithmetic before any device work, so it can be asked for without a device: the pointers that are
    not the point of a case are non-null and never read"""
    lib = _lib.load()
    some = c_void_p(4096)
    null = c_void_p(None)
    tables = ("us", "ul", "uh", "ds", "dl", "dh")
    good = dict(L=6, nup=3, ndn=3, su=-1, sd=-1, order=0, w=some, x=some, y=c_void_p(8192), grid=0, **{t: some for t in tables})

    def apply(**kw):
        a = dict(good, **kw)
        return lib.dsea_hubbard_pair_apply(a["L"], a["nup"], a["ndn"], a["su"], a["sd"], a["order"], a["w"],
                                           *[a[t] for t in tables], a["x"], a["y"], a["grid"], None)

    goodf = dict(L=6, nup=3, ndn=3, su=-1, sd=-1, order=0, v1=some, v2=some, out=some, scratch=some, grid=0,
                 **{t: some for t in tables})

    def forms(**kw):
        a = dict(goodf, **kw)
        return lib.dsea_hubbard_pair_forms(a["L"], a["nup"], a["ndn"], a["su"], a["sd"], a["order"], *[a[t] for t in tables],
                                           a["v1"], a["v2"], a["out"], a["scratch"], a["grid"], None)

    shared = [dict(su=0), dict(sd=0), dict(su=2), dict(sd=-2), dict(order=2), dict(order=-1),
              dict(nup=5, su=1), dict(nup=1), dict(ndn=5, sd=1), dict(ndn=1), dict(nup=0, su=1), dict(nup=6), dict(ndn=0, sd=1),
              dict(ndn=6), dict(L=41, nup=1, ndn=1, su=1, sd=1), dict(L=1, nup=1, ndn=1), dict(L=2, nup=1, ndn=1),
              dict(L=18, nup=8, ndn=8, su=1, sd=1), dict(L=18, nup=9, ndn=9),
              dict(grid=5), dict(grid=13), dict(grid=-1), dict(grid=1)] + [{t: null} for t in tables]
    for bad in shared + [dict(w=null), dict(x=null), dict(y=null), dict(y=some)]:
        assert apply(**bad) == _lib.ERR_ARG, bad
    for bad in shared + [dict(v1=null), dict(v2=null), dict(out=null), dict(scratch=null)]:
        assert forms(**bad) == _lib.ERR_ARG, bad
    need = c_int64(-1)
    for bad in ((6, 3, 3, 0, 1, 0), (6, 3, 3, 1, 2, 0), (6, 3, 3, 1, 1, 2), (6, 5, 3, 1, 1, 0), (6, 3, 1, 1, -1, 0),
                (41, 1, 1, 1, 1, 0), (18, 8, 8, 1, 1, 0)):
        assert lib.dsea_hubbard_pair_forms_scratch_doubles(*bad, byref(need)) == _lib.ERR_ARG and need.value == -1
    assert lib.dsea_hubbard_pair_forms_scratch_doubles(6, 3, 3, 1, 1, 0, None) == _lib.ERR_ARG
    # ... and the sizes: L^2 * min(4096, ceil(n_dst / 256))
    for args, n_dst in (((6, 3, 3, -1, -1, 0), 225), ((12, 6, 6, -1, -1, 1), 792 * 792), ((16, 5, 5, 1, -1, 0), 8008 * 1820),
                        ((40, 1, 1, 1, 1, 0), 780 * 780)):
        assert lib.dsea_hubbard_pair_forms_scratch_doubles(*args, byref(need)) == 0
        assert need.value == args[0] ** 2 * min(4096, (n_dst + 255) // 256)
