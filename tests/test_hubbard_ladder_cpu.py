"""The c / c+ / n maps between Hubbard sectors without a GPU (docs/design/25-hubbard-ladder.md): the numpy reference of
tests/hubbard_ladder_reference.py against the Jordan-Wigner operators on 2 L modes, the identities the GPU tests rely on
(transpose, forms, anticommutators through the sector blocks, free fermions on a ring, the one-body density matrix against the
forms of the Hamiltonian, the f-sum rule of the charge channel with its prefactor), and the argument checks of the Python layer
and of the C ABI that need no device."""
import types
from ctypes import byref, c_int64, c_void_p

import numpy as np
import pytest
import torch

import hubbard_ladder_reference as ref
import hubbard_reference as hub
import lattice_reference
from hubbard_ladder_reference import DN, UP
from dominantsparseeigenad_amd import _lib
from dominantsparseeigenad_amd.operators import HubbardLadder, ring_bonds, ring_momentum_weights
from dominantsparseeigenad_amd.spectral import SpectralMeasure
from dominantsparseeigenad_amd.synthetic import normal_vector


def admissible(L):
    """every (nup, ndn, species, step) whose two sectors the library accepts: 1 <= count <= L - 1 on both sides"""
    out = []
    for nup in range(1, L):
        for ndn in range(1, L):
            for species in (UP, DN):
                for step in (1, 0, -1):
                    nu, nd = ref.destination(nup, ndn, species, step)
                    if 1 <= nu <= L - 1 and 1 <= nd <= L - 1:
                        out.append((nup, ndn, species, step))
    return out


def weights(L, seed=0):
    return normal_vector(L, 9100 + L + seed)


def sector_index(L, nup, ndn):
    """the Jordan-Wigner index u | d << L of every row of the sector, in row order"""
    return np.array([u | (d << L) for u in hub.states(L, nup) for d in hub.states(L, ndn)], dtype=np.int64)


def full_operator(L, species, step, w):
    """sum_i w_i c+_j, c_j or n_j on 2 L modes, j = i for the up species and L + i for the down species"""
    M = 2 * L
    out = np.zeros((1 << M, 1 << M))
    for i in range(L):
        c = hub._annihilator(M, i + (L if species == DN else 0))
        out += w[i] * (c.T if step > 0 else c if step < 0 else c.T @ c)
    return out


def test_the_admissible_cases_are_sixty():
    assert [len(admissible(L)) for L in (2, 3, 4)] == [2, 16, 42]


@pytest.mark.parametrize("L", [2, 3, 4])
def test_reference_is_the_block_of_the_jordan_wigner_operator(L):
    w = weights(L)
    worst = 0.0
    for nup, ndn, species, step in admissible(L):
        full = full_operator(L, species, step, w)
        nu, nd = ref.destination(nup, ndn, species, step)
        src, dst = sector_index(L, nup, ndn), sector_index(L, nu, nd)
        S = ref.dense(L, nup, ndn, species, step, w)
        assert S.shape == (len(dst), len(src)) == ref.sizes(L, nup, ndn, species, step)[::-1]
        dev = float(np.max(np.abs(S - full[np.ix_(dst, src)])))
        worst = max(worst, dev)
        assert dev <= 1e-14 * np.abs(w).sum(), (nup, ndn, species, step, dev)
        # the operator maps the source sector into the destination only: exactly zero everywhere else
        rest = np.setdiff1d(np.arange(1 << (2 * L)), dst)
        assert not full[np.ix_(rest, src)].any()
    print("L = %d: worst |reference - Jordan-Wigner block| = %.2e" % (L, worst))


@pytest.mark.parametrize("L", [2, 3, 4, 5])
def test_creation_is_the_exact_transpose_of_annihilation(L):
    w = weights(L, 1)
    for nup, ndn, species, step in admissible(L):
        S = ref.dense(L, nup, ndn, species, step, w)
        if step == 0:
            assert np.array_equal(S, np.diag(np.diag(S)))
            continue
        nu, nd = ref.destination(nup, ndn, species, step)
        back = ref.dense(L, nu, nd, species, -step, w)
        assert np.array_equal(back, S.T)                  # bit for bit: the entries are +-w_i themselves


@pytest.mark.parametrize("L", [3, 4, 5])
def test_forms_are_the_dense_bilinear_forms(L):
    for nup, ndn, species, step in admissible(L):
        n_src, n_dst = ref.sizes(L, nup, ndn, species, step)
        v1, v2 = normal_vector(n_dst, 9200 + n_dst), normal_vector(n_src, 9300 + n_src)
        got = ref.forms(L, nup, ndn, species, step, v1, v2)
        want = np.array([v1 @ ref.dense(L, nup, ndn, species, step, np.eye(L)[i]) @ v2 for i in range(L)])
        assert np.max(np.abs(got - want)) <= 1e-14 * np.linalg.norm(v1) * np.linalg.norm(v2)


def site(L, nup, ndn, species, step, i):
    return ref.dense(L, nup, ndn, species, step, np.eye(L)[i])


@pytest.mark.parametrize("nup,ndn", [(2, 2), (2, 1), (3, 2)])
def test_the_anticommutators_through_the_sector_blocks(nup, ndn):
    """L = 4.  Same species: c_i c+_j + c+_j c_i = delta_ij on the sector, through (n + 1) and (n - 1).  Different species:
    c_{i up} c+_{j dn} + c+_{j dn} c_{i up} = 0 from (nup, ndn) to (nup - 1, ndn + 1): the down operator acts once behind nup and
    once behind nup - 1 up particles, which is what pins the factor (-1)^nup of the down species."""
    L = 4
    n = ref.sizes(L, nup, ndn, UP, 0)[0]
    for species in (UP, DN):
        k = nup if species == UP else ndn
        if not 2 <= k <= L - 2:
            continue
        up1, dn1 = ref.destination(nup, ndn, species, 1), ref.destination(nup, ndn, species, -1)
        for i in range(L):
            for j in range(L):
                a = site(L, *up1, species, -1, i) @ site(L, nup, ndn, species, 1, j)
                b = site(L, *dn1, species, 1, j) @ site(L, nup, ndn, species, -1, i)
                assert np.array_equal(a + b, np.eye(n) * (i == j))
    if nup >= 2 and ndn <= L - 2:
        for i in range(L):
            for j in range(L):
                a = site(L, nup, ndn + 1, UP, -1, i) @ site(L, nup, ndn, DN, 1, j)
                b = site(L, nup - 1, ndn, DN, 1, j) @ site(L, nup, ndn, UP, -1, i)
                assert a.any() and not (a + b).any()
                # ... and the two annihilators: c_{i up} c_{j dn} + c_{j dn} c_{i up} = 0
                if ndn >= 2:
                    a = site(L, nup, ndn - 1, UP, -1, i) @ site(L, nup, ndn, DN, -1, j)
                    b = site(L, nup - 1, ndn, DN, -1, j) @ site(L, nup, ndn, UP, -1, i)
                    assert a.any() and not (a + b).any()


def free_ring(L, nup, ndn):
    bonds = ring_bonds(L)
    p = np.concatenate([np.ones(L), np.zeros(L), np.zeros(L), np.zeros(L)])
    return bonds, p, hub.dense(L, nup, ndn, bonds, p)


def test_free_fermions_on_a_ring():
    """L = 6, nup = ndn = 3: a closed shell (k = 0, +-pi/3 occupied, eps_k = -2 cos k, gap 2).  c_{k up} psi0 is an eigenvector
    of the (2, 3) Hamiltonian at E0 - eps_k with norm^2 n_k = 1 for an occupied k and vanishes for an empty one;
    |c+_k psi0|^2 = 1 - n_k; sum_k n_k = nup.  The real and the imaginary part of the weights are applied one after the other."""
    L = 6
    _, _, H0 = free_ring(L, 3, 3)
    _, _, Hm = free_ring(L, 2, 3)
    E, V = np.linalg.eigh(H0)
    assert E[1] - E[0] > 1.9
    E0, psi0 = E[0], V[:, 0]
    assert abs(E0 - 2 * (-2.0 - 1.0 - 1.0)) < 1e-12
    total = 0.0
    for m in range(L):
        eps = -2.0 * np.cos(2 * np.pi * m / L)
        occupied = eps < 0.0
        parts = [t.numpy() for t in ring_momentum_weights(L, m)]
        n_k = hole = 0.0
        for w in parts:
            phi = ref.apply(L, 3, 3, UP, -1, w, psi0)
            n_k += phi @ phi
            if occupied:
                assert np.linalg.norm(Hm @ phi - (E0 - eps) * phi) <= 1e-12
            add = ref.apply(L, 3, 3, UP, 1, w, psi0)
            hole += add @ add
        if occupied:
            assert abs(n_k - 1.0) <= 1e-13
        else:
            assert n_k <= 1e-26          # no weight: |c_k psi0| is rounding of the dense eigenvector
        assert abs(hole - (1.0 - n_k)) <= 1e-13
        total += n_k
    assert abs(total - 3.0) <= 1e-12


def density_matrix(L, nup, ndn, species, psi):
    C = np.array([ref.apply(L, nup, ndn, species, -1, np.eye(L)[i], psi) for i in range(L)])
    return C @ C.T


def interacting(L, nup, ndn, seed):
    bonds = tuple(ring_bonds(L) + lattice_reference.random_bonds(L, 3, seed))
    nb = len(bonds)
    p = np.concatenate([np.ones(nb), 0.3 * np.ones(nb), 4.0 * np.ones(L), normal_vector(L, seed + 1)])
    return bonds, p, hub.dense(L, nup, ndn, bonds, p)


@pytest.mark.parametrize("L,nup,ndn", [(5, 2, 3), (5, 3, 2), (4, 2, 2)])
def test_the_one_body_density_matrix_against_the_forms_of_the_hamiltonian(L, nup, ndn):
    """U = 4, V = 0.3, random eps: tr rho_s = N_s, rho symmetric, diag rho_up + diag rho_dn = <n_i> (the eps forms), and
    -2 (rho_up + rho_dn)[a, b] = <dH/dt_t> (the t forms: dH/dt_t = -sum_s (c+_a c_b + h.c.))"""
    bonds, p, H = interacting(L, nup, ndn, 9400 + L + nup)
    _, V = np.linalg.eigh(H)
    psi = V[:, 0]
    up, dn = density_matrix(L, nup, ndn, UP, psi), density_matrix(L, nup, ndn, DN, psi)
    assert abs(np.trace(up) - nup) <= 1e-13 and abs(np.trace(dn) - ndn) <= 1e-13
    assert np.max(np.abs(up - up.T)) <= 1e-15 and np.max(np.abs(dn - dn.T)) <= 1e-15
    forms = hub.forms(L, nup, ndn, bonds, psi, psi)
    nb = len(bonds)
    assert np.max(np.abs(np.diag(up) + np.diag(dn) - forms[2 * nb + L:])) <= 1e-14
    hop = np.array([-2.0 * (up + dn)[a, b] for a, b in bonds])
    assert np.max(np.abs(hop - forms[:nb])) <= 1e-14


def charge_first_moment_from_forms(bonds, t, w, t_forms):
    """The f-sum rule of the charge channel.  For the hermitian A = sum_i w_i n_i the first moment of its measure is
    sum_n (E_n - E_0) |<n|A|0>|^2 = <[A, [H, A]]> / 2, and only the hopping fails to commute with A:
        [A, c+_a c_b] = (w_a - w_b) c+_a c_b
        [A, [H, A]] = sum_t t_t (w_a - w_b)^2 sum_s (c+_{a s} c_{b s} + h.c.) = -sum_t t_t (w_a - w_b)^2 dH/dt_t
    so the first moment is -(1/2) sum_t t_t (w_a - w_b)^2 <dH/dt_t>, with the t forms of ``Hadjoint_to_couplingsadjoint``.  The
    same holds for sum_i w_i (n_{i up} - n_{i dn}): the species enter the double commutator separately."""
    return -0.5 * sum(t[k] * (w[a] - w[b]) ** 2 * t_forms[k] for k, (a, b) in enumerate(bonds))


@pytest.mark.parametrize("channel", ["n", "sz"])
def test_the_f_sum_rule_prefactor_against_dense_eigh(channel):
    L, nup, ndn = 5, 2, 3
    bonds, p, H = interacting(L, nup, ndn, 9450)
    E, V = np.linalg.eigh(H)
    psi0 = V[:, 0]
    nb = len(bonds)
    t_forms = hub.forms(L, nup, ndn, bonds, psi0, psi0)[:nb]
    sign = 1.0 if channel == "n" else -1.0
    for m in range(1, L):
        for w in (t.numpy() for t in ring_momentum_weights(L, m)):
            phi = ref.apply(L, nup, ndn, UP, 0, w, psi0) + sign * ref.apply(L, nup, ndn, DN, 0, w, psi0)
            amp = V.T @ phi
            first = np.sum((E - E[0]) * amp ** 2)
            want = charge_first_moment_from_forms(bonds, p[:nb], w, t_forms)
            assert abs(first - want) <= 1e-12 * (E[-1] - E[0])
            assert first > 0.0


def test_spectral_measure_reflected():
    a = SpectralMeasure([0.5, 2.0], [0.25, 0.75], 1.0, 2)
    r = a.reflected()
    assert torch.equal(r.poles, -a.poles) and torch.equal(r.weights, a.weights) and r.norm2 == 1.0 and r.steps == 2
    assert r.moment(0) == a.moment(0) and r.moment(1) == -a.moment(1) and r.moment(2) == a.moment(2)
    back = r.reflected()
    assert torch.equal(back.poles, a.poles)
    z = torch.tensor([0.3 + 0.5j, -1.0 + 0.1j], dtype=torch.complex128)
    assert torch.allclose(r.greens(z), -a.greens(-z), rtol=1e-15, atol=0)
    # A(omega) = addition + reflected removal is one measure
    b = SpectralMeasure([1.0], [2.0], 2.0, 1)
    s = b + a.reflected()
    assert s.poles.tolist() == [1.0, -0.5, -2.0] and s.moment(0) == 3.0
    assert len(SpectralMeasure([], [], 0.0, 0).reflected()) == 0


def carrier(L, nup, ndn, device="cpu"):
    """what HubbardLadder reads of an operator, without a device"""
    return types.SimpleNamespace(N=L, nup=nup, ndn=ndn, device=torch.device(device), _up=(None, None, None),
                                 _dn=(None, None, None))


def test_value_errors_that_need_no_device():
    lad = HubbardLadder(carrier(6, 3, 3), carrier(6, 2, 3))
    assert (lad.species, lad.step, lad.L, lad.n_src, lad.n_dst) == ("up", -1, 6, 400, 300)
    back = lad.T
    assert (back.species, back.step, back.n_src, back.n_dst) == ("up", 1, 300, 400) and back.T is lad
    dn = HubbardLadder(carrier(6, 3, 3), carrier(6, 3, 4), species="dn")
    assert (dn.species, dn.step, dn.n_dst) == ("dn", 1, 300)
    same = HubbardLadder(carrier(6, 3, 2), carrier(6, 3, 2), species="dn")
    assert (same.species, same.step, same.n_src, same.n_dst) == ("dn", 0, 300, 300)
    assert same.T.species == "dn" and same.T.step == 0
    for src, dst, species in ((carrier(6, 3, 3), carrier(6, 3, 3), None),        # the same sector needs a species
                              (carrier(6, 3, 3), carrier(6, 2, 3), "dn"),        # a species that contradicts the sectors
                              (carrier(6, 3, 3), carrier(6, 3, 2), "up"),
                              (carrier(6, 3, 3), carrier(6, 3, 3), "down"),      # no such species
                              (carrier(6, 3, 3), carrier(6, 2, 2), None),        # both counts change
                              (carrier(6, 3, 3), carrier(6, 4, 2), None),
                              (carrier(6, 3, 3), carrier(6, 1, 3), None),        # two steps
                              (carrier(6, 3, 3), carrier(6, 3, 5), None),
                              (carrier(6, 3, 3), carrier(7, 3, 3), "up"),        # another L
                              (carrier(6, 5, 3), carrier(6, 6, 3), None),        # a destination with a full species
                              (carrier(6, 3, 1), carrier(6, 3, 0), None),        # ... and with an empty one
                              (carrier(41, 1, 1), carrier(41, 2, 1), None),      # L beyond the limit
                              (carrier(18, 9, 8), carrier(18, 9, 9), None),      # more than 2^31 - 1 rows
                              (carrier(6, 3, 3), carrier(6, 2, 3, "meta"), None),     # another device
                              (carrier(6, 3, 3), object(), None)):               # no tables
        with pytest.raises(ValueError):
            HubbardLadder(src, dst, species)
    for g in (1, 5, 13, -1):
        with pytest.raises(ValueError):
            lad.set_grid_log2(g)
    lad.set_grid_log2(6)
    assert back._grid[0] == 6                               # one setting for the ladder and its transpose
    lad.set_grid_log2(0)
    x = torch.zeros(400, dtype=torch.float64)
    for w in (torch.zeros(5, dtype=torch.float64), torch.zeros((6, 1), dtype=torch.float64),
              torch.zeros(6, dtype=torch.complex128)):
        with pytest.raises(ValueError):
            lad(w, x)
    with pytest.raises(ValueError):
        lad(torch.zeros(6, dtype=torch.float64), torch.zeros(300, dtype=torch.float64))     # a vector of the destination
    with pytest.raises(ValueError):
        lad.forms(x, x)                                     # v1 lives on the destination
    with pytest.raises(ValueError):
        lad(torch.zeros(6, dtype=torch.float64), x)         # host tensors: the map is a device kernel, there is no fallback


def test_c_abi_argument_errors_without_a_device():
    """every refusal is host arithmetic before any device work, so it can be asked for without a device: the pointers that are
    not the point of a case are non-null and never read"""
    lib = _lib.load()
    some = c_void_p(4096)
    null = c_void_p(None)
    good = dict(L=6, nup=3, ndn=3, species=0, step=-1, w=some, states=some, lo=some, hi=some, x=some, y=c_void_p(8192), grid=0)

    def apply(**kw):
        a = dict(good, **kw)
        return lib.dsea_hubbard_ladder_apply(a["L"], a["nup"], a["ndn"], a["species"], a["step"], a["w"], a["states"], a["lo"],
                                             a["hi"], a["x"], a["y"], a["grid"], None)

    goodf = dict(L=6, nup=3, ndn=3, species=0, step=-1, states=some, lo=some, hi=some, v1=some, v2=some, out=some, scratch=some,
                 grid=0)

    def forms(**kw):
        a = dict(goodf, **kw)
        return lib.dsea_hubbard_ladder_forms(a["L"], a["nup"], a["ndn"], a["species"], a["step"], a["states"], a["lo"], a["hi"],
                                             a["v1"], a["v2"], a["out"], a["scratch"], a["grid"], None)

    shared = [dict(species=2), dict(species=-1), dict(step=2), dict(step=-2),
              dict(nup=5, step=1), dict(nup=1, step=-1), dict(ndn=5, species=1, step=1), dict(ndn=1, species=1, step=-1),
              dict(nup=0, step=1), dict(nup=6, step=-1), dict(ndn=0), dict(ndn=6),
              dict(L=41, nup=1, ndn=1, step=1), dict(L=1, nup=1, ndn=1, step=0), dict(L=18, nup=9, ndn=8, species=1, step=1),
              dict(L=18, nup=9, ndn=9, step=-1),
              dict(grid=5), dict(grid=13), dict(grid=-1), dict(grid=1), dict(states=null), dict(lo=null), dict(hi=null)]
    for bad in shared + [dict(w=null), dict(x=null), dict(y=null), dict(y=some), dict(step=1, nup=2, y=some)]:
        assert apply(**bad) == _lib.ERR_ARG, bad
    for bad in shared + [dict(v1=null), dict(v2=null), dict(out=null), dict(scratch=null)]:
        assert forms(**bad) == _lib.ERR_ARG, bad
    need = c_int64(-1)
    for bad in ((6, 3, 3, 2, 1), (6, 3, 3, 0, 2), (6, 5, 3, 0, 1), (6, 3, 1, 1, -1), (41, 1, 1, 0, 1), (18, 9, 8, 1, 1)):
        assert lib.dsea_hubbard_ladder_forms_scratch_doubles(*bad, byref(need)) == _lib.ERR_ARG and need.value == -1
    assert lib.dsea_hubbard_ladder_forms_scratch_doubles(6, 3, 3, 0, 1, None) == _lib.ERR_ARG
    # ... and the sizes: L * min(4096, ceil(n_dst / 256))
    for args, n_dst in (((6, 3, 3, 0, -1), 300), ((12, 5, 5, 0, 1), 731808), ((16, 5, 5, 1, -1), 4368 * 1820),
                        ((16, 5, 5, 1, 0), 4368 * 4368)):
        assert lib.dsea_hubbard_ladder_forms_scratch_doubles(*args, byref(need)) == 0
        assert need.value == args[0] * min(4096, (n_dst + 255) // 256)
