"""The ladder maps between magnetisation sectors and the Lanczos measure on the GPU (docs/design/24-dynamics.md):
k_sector_ladder and k_sector_ladder_forms against the numpy reference of tests/ladder_reference.py at the smallest sizes that
reach each path, then the identities that tie them to the existing correlator, autograd against a dense twin, the argument
checks of the C ABI, the spectral measure against dense eigh, and the structure factor of a Heisenberg ring end to end.

    L  src -> dst         n_src -> n_dst       what it reaches
    2  1 -> 1             2 -> 2               step 0, less than one wave
    3  1 -> 2, 2 -> 1     3 -> 3               tiny, odd n, both directions
    5  2 -> 3             10 -> 10             Llo = 3, Lhi = 2
    7  3 -> 4, 4 -> 3     35 -> 35             odd L (Llo = 4), sites on both sides of the split; 3 -> 3: step 0
    11 5 -> 6             462 -> 462           two blocks, ragged last block
    16 8 -> 9, 8 -> 7     12 870 -> 11 440     many blocks, two chunks in each group; 8 -> 8: step 0
    20 10 -> 11           184 756 -> 167 960   657 row ranges on a grid capped at 64 blocks: blocks walk ranges
    20 1 -> 2, 19 -> 18   20 -> 190            extreme fillings
    34 2 -> 3             561 -> 5 984         states wider than 32 bits
    40 1 -> 2, 2 -> 1     40 -> 780, 780 -> 40 states wider than 32 bits, three chunks in each group; 2 -> 2: step 0
"""
import functools
import importlib.util
import math
import os
import warnings
from ctypes import byref, c_int64, c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ladder_reference as ref  # noqa: E402
import lattice_reference  # noqa: E402
import sector_reference  # noqa: E402
from dominantsparseeigenad_amd import _lib, engine  # noqa: E402
from dominantsparseeigenad_amd.operators import (SpinSectorLadder, SpinSectorOperator, SpinSectorPairOperator,  # noqa: E402
                                                 ring_bonds, ring_momentum_weights)
from dominantsparseeigenad_amd.spectral import SpectralMeasure, dynamical_structure_factor, lanczos_measure  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402
import dominantsparseeigenad_amd.symeig as symeig  # noqa: E402
import dominantsparseeigenad_amd.CG as CG  # noqa: E402

F64 = torch.float64
TOL = 1e-10

# name -> (L, ndown of the source, ndown of the destination, log2 of the grid cap or None for the default)
GEOMETRY = {
    "L2-1-1": (2, 1, 1, None),
    "L3-1-2": (3, 1, 2, None),
    "L3-2-1": (3, 2, 1, None),
    "L5-2-3": (5, 2, 3, None),
    "L7-3-4": (7, 3, 4, None),
    "L7-4-3": (7, 4, 3, None),
    "L11-5-6": (11, 5, 6, None),
    "L16-8-9": (16, 8, 9, None),
    "L16-8-7": (16, 8, 7, None),
    "L20-10-11-walk": (20, 10, 11, 6),
    "L20-1-2": (20, 1, 2, None),
    "L20-19-18": (20, 19, 18, None),
    "L34-2-3": (34, 2, 3, None),
    "L40-1-2": (40, 1, 2, None),
    "L40-2-1": (40, 2, 1, None),
    "L7-3-3": (7, 3, 3, None),
    "L16-8-8": (16, 8, 8, None),
    "L40-2-2": (40, 2, 2, None),
}
WEIGHTS = ["random", "ones", "top"]


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


def to_dev(a):
    return torch.from_numpy(np.array(a)).to(dev())      # (a copy: the cached case arrays are read-only)


def site_weights(L, kind):
    if kind == "ones":
        return np.ones(L)
    if kind == "top":
        return np.eye(L)[L - 1]
    return normal_vector(L, 9600 + L)


@functools.lru_cache(maxsize=None)
def sector(L, ndown):
    """one table set per sector for the whole module (zero couplings: only the tables are used)"""
    return SpinSectorPairOperator(L, None, ndown, device=dev())


def ladder(name):
    L, a, b, grid = GEOMETRY[name]
    lad = SpinSectorLadder(sector(L, a), sector(L, b))
    if grid is not None:
        lad.set_grid_log2(grid)
    return lad


@functools.lru_cache(maxsize=None)
def case(name, kind):
    """(c, x, S(c) x) on the host, computed once per case and never written to"""
    L, a, b, _ = GEOMETRY[name]
    c = site_weights(L, kind)
    x = normal_vector(math.comb(L, a), 9700 + L + a)
    y = ref.apply(L, a, b - a, c, x)
    for arr in (c, x, y):
        arr.setflags(write=False)
    return c, x, y


@functools.lru_cache(maxsize=None)
def form_case(name):
    L, a, b, _ = GEOMETRY[name]
    v1, v2 = normal_vector(math.comb(L, b), 9800 + L + b), normal_vector(math.comb(L, a), 9900 + L + a)
    out = ref.forms(L, a, b - a, v1, v2)
    for arr in (v1, v2, out):
        arr.setflags(write=False)
    return v1, v2, out


def relnorm(a, b):
    """|a - b| / |b|; a reference that is exactly zero (Z(1) in a sector with as many up as down spins) must be met exactly"""
    diff, scale = float(np.linalg.norm(np.asarray(a) - np.asarray(b))), float(np.linalg.norm(np.asarray(b)))
    if scale == 0.0:
        return 0.0 if diff == 0.0 else math.inf
    return diff / scale


def test_the_cases_are_what_the_table_says():
    sizes = {name: (math.comb(g[0], g[1]), math.comb(g[0], g[2])) for name, g in GEOMETRY.items()}
    assert [sizes[k] for k in GEOMETRY] == [(2, 2), (3, 3), (3, 3), (10, 10), (35, 35), (35, 35), (462, 462), (12870, 11440),
                                            (12870, 11440), (184756, 167960), (20, 190), (20, 190), (561, 5984), (40, 780),
                                            (780, 40), (35, 35), (12870, 12870), (780, 780)]
    steps = [g[2] - g[1] for g in GEOMETRY.values()]
    assert steps == [0, 1, -1, 1, 1, -1, 1, 1, -1, 1, 1, -1, 1, 1, -1, 0, 0, 0]
    assert (7 + 1) // 2 == 4 and 7 - 4 == 3                       # L = 7: sites 0 .. 3 low, 4 .. 6 high
    n = sizes["L11-5-6"][1]
    assert (n + 255) // 256 == 2 and n % 256 != 0                # two blocks, ragged last block
    n = sizes["L20-10-11-walk"][1]
    assert (n + 255) // 256 == 657 > (1 << GEOMETRY["L20-10-11-walk"][3])      # more row ranges than blocks
    assert (16 + 1) // 2 == 8 and (40 + 1) // 2 == 20            # one full chunk of 8 per group at L = 16, three at L = 40
    for name in ("L34-2-3", "L40-1-2", "L40-2-1", "L40-2-2"):
        L, a, b, _ = GEOMETRY[name]
        assert max(sector_reference.states(L, b)) >= 1 << 32
    # a row sums at most L = 40 products
    assert max(g[0] for g in GEOMETRY.values()) == 40


@pytest.mark.parametrize("kind", WEIGHTS)
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_apply_against_the_reference(name, kind):
    L, a, b, grid = GEOMETRY[name]
    c, x, want = case(name, kind)
    lad = ladder(name)
    assert (lad.L, lad.step, lad.n_src, lad.n_dst) == (L, b - a, x.size, want.size)
    cd, xd = to_dev(c), to_dev(x)
    got = lad(cd, xd)
    assert got.shape == (lad.n_dst,) and got.dtype == F64
    err = relnorm(got.cpu().numpy(), want)
    print("%s %s: |y - ref| / |ref| = %.2e" % (name, kind, err))
    assert err < 1e-13
    # nothing is written past the last row: a longer output filled with a sentinel
    y = torch.full((lad.n_dst + 67,), -7.0, dtype=F64, device=dev())
    states, lo_rank, hi_base = lad._tables
    rc = _lib.load().dsea_sector_ladder_apply(L, a, b - a, c_void_p(cd.data_ptr()), c_void_p(states.data_ptr()),
                                              c_void_p(lo_rank.data_ptr()), c_void_p(hi_base.data_ptr()), c_void_p(xd.data_ptr()),
                                              c_void_p(y.data_ptr()), grid or 0, engine._stream(dev()))
    assert rc == 0
    assert torch.equal(y[:lad.n_dst], got) and bool((y[lad.n_dst:] == -7.0).all())


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_the_transposed_ladder_is_the_transpose(name):
    c, x, _ = case(name, "random")
    lad = ladder(name)
    cd, v2 = to_dev(c), to_dev(x)
    v1 = to_dev(normal_vector(lad.n_dst, 9650 + lad.n_dst % 89))
    Sv2, STv1 = lad(cd, v2), lad.T(cd, v1)
    assert STv1.shape == (lad.n_src,)
    lhs, rhs = float(v1 @ Sv2), float(STv1 @ v2)
    assert abs(lhs - rhs) <= 1e-13 * float(v1.norm() * Sv2.norm() + STv1.norm() * v2.norm())


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_forms_against_the_reference_sums(name):
    L, a, b, _ = GEOMETRY[name]
    v1, v2, want = form_case(name)
    lad = ladder(name)
    d1, d2 = to_dev(v1), to_dev(v2)
    got = lad.forms(d1, d2)
    assert got.shape == (L,)
    norms = np.linalg.norm(v1) * np.linalg.norm(v2)
    bound = 1e-13 * norms
    err = float(np.max(np.abs(got.cpu().numpy() - want)))
    print("%s: max |form - ref| = %.2e (bound %.2e)" % (name, err, bound))
    assert err <= bound
    again = lad.forms(d1, d2)
    assert torch.equal(got, again)                       # fixed-order reductions, no atomics
    # S is linear in the weights: v1^T S(c) v2 = sum_i c_i form_i.  Each form is within 1e-13 |v1| |v2| of its sum and the map
    # within 1e-13 |S v2| of its value (the two bounds above), so the two sides differ by at most
    # 1e-13 (|v1| |v2| sum_i |c_i| + |v1| |S v2|)
    c = site_weights(L, "random")
    Sv2 = lad(to_dev(c), d2)
    lhs, rhs = float(d1 @ Sv2), float(np.sum(c * got.cpu().numpy()))
    assert abs(lhs - rhs) <= 1e-13 * (norms * np.abs(c).sum() + np.linalg.norm(v1) * float(Sv2.norm()))


@pytest.mark.parametrize("L,ndown", [(11, 5), (16, 8)])
def test_the_norm_of_sigma_minus_psi_through_the_correlator(L, ndown):
    """|sigma^-(c) psi|^2 = sum_i c_i^2 (1 + <Z_i>) / 2 + sum_{i<j} c_i c_j <X_i X_j + Y_i Y_j> / 2 for a normalised psi
    (tests/test_ladder_cpu.py checks the identity in numpy), with the correlators of SpinSectorOperator.correlations"""
    bonds = ring_bonds(L)
    src = SpinSectorOperator(L, bonds, torch.zeros(3 * L, dtype=F64, device=dev()), ndown)
    lad = src.ladder(sector(L, ndown + 1))
    psi = to_dev(normal_vector(src.n, 9660 + L))
    psi = psi / psi.norm()
    c = to_dev(site_weights(L, "random"))
    phi = lad(c, psi)
    xy, _, z = src.correlations(psi)
    want = (c * c * (1.0 + z)).sum() / 2.0 + (torch.triu(xy, diagonal=1) * torch.outer(c, c)).sum() / 2.0
    got = torch.dot(phi, phi)
    err = abs(float(got - want)) / float(got)
    print("L = %d: | |phi|^2 - correlators | / |phi|^2 = %.2e" % (L, err))
    assert err <= TOL


def test_autograd_against_a_dense_twin():
    L = 8
    lad = ladder_8()
    S = torch.stack([lad.dense(torch.eye(L, dtype=F64, device=dev())[i]) for i in range(L)])       # [L, n_dst, n_src]
    assert S.shape == (L, 56, 70)
    assert torch.equal(S, torch.from_numpy(np.stack([ref.dense(L, 4, 1, np.eye(L)[i]) for i in range(L)])).to(dev()))
    c0, x0 = to_dev(site_weights(L, "random")), to_dev(normal_vector(70, 9670))
    v = to_dev(normal_vector(L, 9671))

    def grads(apply):
        c, x = c0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
        y = apply(c, x)
        loss = (y * y).sum()
        gc, gx = torch.autograd.grad(loss, (c, x), create_graph=True)
        (hv,) = torch.autograd.grad((gc * v).sum(), c)
        return loss.detach(), gc.detach(), gx.detach(), hv

    native = grads(lad)
    twin = grads(lambda c, x: torch.einsum("i,iab,b->a", c, S, x))
    for what, a, b in zip(("loss", "d/dc", "d/dx", "Hessian-vector product in c"), native, twin):
        err = float((a - b).norm() / b.norm())
        print("%s: relative deviation from the dense twin %.2e" % (what, err))
        assert err <= TOL


def ladder_8():
    return SpinSectorLadder(sector(8, 4), sector(8, 5))


def test_c_abi_argument_errors():
    """every DSEA_ERR_ARG case returns the error from host arithmetic: nothing is launched, the outputs keep their sentinel"""
    lib = _lib.load()
    L, nd, step = 8, 4, 1
    lad = ladder_8()
    states, lo_rank, hi_base = (c_void_p(t.data_ptr()) for t in lad._tables)
    c = to_dev(site_weights(L, "random"))
    x = to_dev(normal_vector(70, 9680))
    y = torch.full((70,), -7.0, dtype=F64, device=dev())          # (70: long enough for step 0 as well)
    out = torch.full((L,), -7.0, dtype=F64, device=dev())
    scratch = torch.full((L,), -7.0, dtype=F64, device=dev())
    st = engine._stream(dev())
    P = lambda t: c_void_p(t.data_ptr())                        # noqa: E731
    null = c_void_p(None)
    good = dict(L=L, nd=nd, step=step, c=P(c), states=states, lo=lo_rank, hi=hi_base, x=P(x), y=P(y), grid=0)

    def apply(**kw):
        a = dict(good, **kw)
        return lib.dsea_sector_ladder_apply(a["L"], a["nd"], a["step"], a["c"], a["states"], a["lo"], a["hi"], a["x"], a["y"],
                                            a["grid"], st)

    goodf = dict(L=L, nd=nd, step=step, states=states, lo=lo_rank, hi=hi_base, v1=P(y), v2=P(x), out=P(out), scratch=P(scratch),
                 grid=0)

    def forms(**kw):
        a = dict(goodf, **kw)
        return lib.dsea_sector_ladder_forms(a["L"], a["nd"], a["step"], a["states"], a["lo"], a["hi"], a["v1"], a["v2"], a["out"],
                                            a["scratch"], a["grid"], st)

    shared = [dict(step=2), dict(step=-2), dict(nd=7, step=1), dict(nd=1, step=-1), dict(nd=0, step=1), dict(nd=8, step=-1),
              dict(L=41, nd=1), dict(L=1, nd=1, step=0), dict(L=36, nd=17), dict(grid=5), dict(grid=13), dict(grid=-1),
              dict(grid=1), dict(states=null), dict(lo=null), dict(hi=null)]
    for bad in shared + [dict(c=null), dict(x=null), dict(y=null), dict(y=P(x)), dict(step=-1, y=P(x))]:
        assert apply(**bad) == _lib.ERR_ARG, bad
    for bad in shared + [dict(v1=null), dict(v2=null), dict(out=null), dict(scratch=null)]:
        assert forms(**bad) == _lib.ERR_ARG, bad
    need = c_int64(-1)
    for bad in ((L, nd, 2), (L, 7, 1), (L, 1, -1), (41, 1, 1), (36, 17, 1)):
        assert lib.dsea_sector_ladder_forms_scratch_doubles(*bad, byref(need)) == _lib.ERR_ARG and need.value == -1
    assert lib.dsea_sector_ladder_forms_scratch_doubles(L, nd, step, None) == _lib.ERR_ARG
    torch.cuda.synchronize()
    for t in (y, out, scratch):
        assert bool((t == -7.0).all())
    # ... and the sizes: L * min(4096, ceil(n_dst / 256))
    for (l, a, s), n_dst in (((8, 4, 1), 56), ((20, 10, 1), 167960), ((24, 12, 1), 2496144), ((24, 12, 0), 2704156)):
        assert lib.dsea_sector_ladder_forms_scratch_doubles(l, a, s, byref(need)) == 0
        assert need.value == l * min(4096, (n_dst + 255) // 256)
    # x == y is allowed for step 0 (a diagonal map)
    same = ladder("L7-3-3")
    cz, xz, want = case("L7-3-3", "random")
    buf = to_dev(xz)
    tabs = [c_void_p(t.data_ptr()) for t in same._tables]
    assert lib.dsea_sector_ladder_apply(7, 3, 0, P(to_dev(cz)), tabs[0], tabs[1], tabs[2], P(buf), P(buf), 0, st) == 0
    assert relnorm(buf.cpu().numpy(), want) < 1e-13


@functools.lru_cache(maxsize=None)
def measure_case():
    """L = 8, a ring with random couplings plus random bonds and random fields (no symmetry), ndown 4 -> 5: the dense
    matrices of both sectors, the ground state of the source, on the host"""
    L = 8
    bonds = tuple(ring_bonds(L) + lattice_reference.random_bonds(L, 6, 9690))
    p = normal_vector(sector_reference.nparam(L, bonds), 9691)
    H0, H1 = sector_reference.dense(L, 4, bonds, p), sector_reference.dense(L, 5, bonds, p)
    _, V0 = np.linalg.eigh(H0)
    E1, V1 = np.linalg.eigh(H1)
    c = site_weights(L, "random")
    phi = ref.apply(L, 4, 1, c, V0[:, 0])
    return L, bonds, p, c, V0[:, 0].copy(), H1, E1, V1, phi


def measure_setup():
    L, bonds, p, c, psi0, H1, E1, V1, phi_ref = measure_case()
    assert H1.shape == (56, 56)
    src = SpinSectorOperator(L, bonds, to_dev(p), 4)
    target = SpinSectorOperator(L, bonds, to_dev(p), 5)
    phi = src.ladder(target)(to_dev(c), to_dev(psi0))
    assert relnorm(phi.cpu().numpy(), phi_ref) < 1e-13
    return target, phi


def test_the_measure_with_all_steps_against_dense_eigh():
    """k = n: G(omega + i eta) at eta = 0.5 on 64 points across the spectrum against sum_n |<n|phi>|^2 / (z - E_n).  The
    sensitivity of G to a pole shift is at most |phi|^2 / eta^2, so eigenvalue errors of order eps |H| leave a wide margin
    below TOL max|G|."""
    _, _, _, _, _, H1, E1, V1, phi_ref = measure_case()
    target, phi = measure_setup()
    m = lanczos_measure(target, phi, 56)
    assert isinstance(m, SpectralMeasure) and 1 <= m.steps <= 56 and len(m) == m.steps
    assert m.poles.device.type == "cpu" and m.poles.dtype == torch.float64
    z = torch.complex(torch.linspace(float(E1[0]), float(E1[-1]), 64, dtype=F64), torch.full((64,), 0.5, dtype=F64))
    amp = V1.T @ phi_ref
    dense = torch.from_numpy(np.sum(amp ** 2 / (z.numpy()[:, None] - E1[None, :]), axis=1))
    got = m.greens(z)
    err = float((got - dense).abs().max() / dense.abs().max())
    print("k = n = 56 (steps = %d): max |G - G_dense| / max |G_dense| = %.2e" % (m.steps, err))
    assert err <= TOL
    assert torch.allclose(m(z.real, 0.5), -got.imag / math.pi, rtol=1e-15, atol=0)
    assert float(m.greens(z.to(dev())).cpu().sub(got).abs().max()) <= 1e-14 * float(got.abs().max())


def test_the_measure_with_few_steps_reproduces_the_moments():
    _, _, _, _, _, H1, _, _, phi_ref = measure_case()
    target, phi = measure_setup()
    m = lanczos_measure(target, phi, 12)
    assert m.steps == 12 and len(m) == 12
    norm2 = float(phi_ref @ phi_ref)
    scale = np.linalg.norm(H1, 2)
    v = phi_ref.copy()
    for k in range(4):
        exact = float(phi_ref @ v)
        err = abs(m.moment(k) - exact)
        print("moment %d: |measure - phi^T H^%d phi| = %.2e (bound %.2e)" % (k, k, err, 1e-12 * norm2 * scale ** k))
        assert err <= 1e-12 * norm2 * scale ** k
        v = H1 @ v
    assert abs(float(m.weights.sum()) - norm2) <= 1e-12 * norm2 and abs(m.norm2 - norm2) <= 1e-12 * norm2
    assert bool((m.weights >= 0.0).all())
    # a vector of zeros has the empty measure, and more steps than rows are cut to n
    empty = lanczos_measure(target, torch.zeros(56, dtype=F64, device=dev()), 12)
    assert len(empty) == 0 and empty.steps == 0 and empty.norm2 == 0.0
    assert float(empty.greens(torch.tensor([1.0 + 0.5j])).abs()) == 0.0
    assert lanczos_measure(target, phi, 500).steps <= 56


def test_the_measure_is_cut_at_a_breakdown():
    """phi in the span of three eigenvectors: the Krylov space has dimension 3, the run stops itself there
    (``engine.last_break``), the measure is cut at the break, reports it as ``steps`` and passes no RuntimeWarning on; its
    poles are then the three eigenvalues and its weights the squared coefficients"""
    _, _, _, _, _, _, E1, V1, _ = measure_case()
    target, _ = measure_setup()
    pick, coef = [3, 20, 41], np.array([0.5, -1.25, 2.0])
    phi = to_dev(V1[:, pick] @ coef)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m = lanczos_measure(target, phi, 12)
    print("breakdown: steps = %d, poles %s, weights %s" % (m.steps, m.poles.tolist(), m.weights.tolist()))
    assert m.steps < 12 and len(m) == m.steps
    heavy = m.weights > 1e-10 * m.norm2
    assert int(heavy.sum()) == 3
    assert np.max(np.abs(m.poles[heavy].numpy() - E1[pick])) <= TOL * np.abs(E1).max()
    assert np.max(np.abs(m.weights[heavy].numpy() - coef ** 2)) <= TOL * m.norm2
    assert abs(m.norm2 - float(coef @ coef)) <= 1e-12 * m.norm2


def zz_first_moment_from_correlators(bonds, jxy, c, xy):
    """The f-sum rule in the Pauli convention.  For the hermitian A = sum_i c_i Z_i the first moment of its measure is
    sum_n (E_n - E_0) |<n|A|0>|^2 = <[A, [H, A]]> / 2, and only the XY part of H fails to commute with A.  With
    X_a X_b + Y_a Y_b = 2 (sigma^+_a sigma^-_b + sigma^-_a sigma^+_b) and [Z_a, sigma^+-_a] = +-2 sigma^+-_a:
        [A, sigma^+_a sigma^-_b] = 2 (c_a - c_b) sigma^+_a sigma^-_b,   [A, sigma^-_a sigma^+_b] = -2 (c_a - c_b) sigma^-_a sigma^+_b
        [A, [H, A]] = -sum_t 4 Jxy_t (c_a - c_b)^2 (X_a X_b + Y_a Y_b)
    so the first moment is -2 sum_t Jxy_t (c_a - c_b)^2 <X_a X_b + Y_a Y_b>: the prefactor 2 that
    tests/test_ladder_cpu.py::test_the_f_sum_rule_prefactor_against_dense_eigh checks against dense eigh."""
    return -2.0 * sum(jxy[t] * (c[a] - c[b]) ** 2 * xy[a][b] for t, (a, b) in enumerate(bonds))


def test_structure_factor_of_the_heisenberg_ring():
    """L = 10, ndown = 5, psi0 and E0 from DominantSparseSymeig, every q = 2 pi m / L with m != 0.  The ground state is a singlet,
    so the "-" channel (in ndown = 6) and the "zz" channel (in ndown = 5) see the same triplet: with sigma^- = S^- and Z = 2 S^z,
    G_-(z) = G_zz(z) / 2 (checked in numpy by tests/test_ladder_cpu.py).  The zz first moment obeys the f-sum rule above with the
    correlators of ``correlations``, and a complex weight vector (cos, sin) gives the sum of the two real measures."""
    L, nd = 10, 5
    bonds = ring_bonds(L)
    p = torch.cat([torch.ones(2 * L, dtype=F64), torch.zeros(L, dtype=F64)]).to(dev())
    op = SpinSectorOperator(L, bonds, p, nd)
    orig = CG.EPS_DEFAULT
    try:
        CG.EPS_DEFAULT = 1e-12
        symeig.setDominantSparseSymeig(op.H, op.Hadjoint_to_couplingsadjoint)
        torch.manual_seed(0)
        E0, psi0 = symeig.DominantSparseSymeig.apply(op.couplings, 200, op.dim, op.device)
    finally:
        CG.EPS_DEFAULT = orig
    E0, psi0 = float(E0), psi0.detach()
    dense_E = np.linalg.eigvalsh(sector_reference.dense(L, nd, bonds, p.cpu().numpy()))
    assert abs(E0 - dense_E[0]) <= TOL * abs(dense_E[0]) and dense_E[1] - dense_E[0] > 0.1      # non-degenerate
    xy, _, _ = op.correlations(psi0)
    xy = xy.cpu().numpy()
    target = SpinSectorOperator(L, bonds, p, nd + 1)
    z = torch.complex(torch.linspace(-1.0, 30.0, 64, dtype=F64), torch.full((64,), 0.5, dtype=F64))
    worst_g = worst_m = 0.0
    for m in range(1, L):
        re, im = ring_momentum_weights(L, m)
        lo = dynamical_structure_factor(op, psi0, E0, re, "-", k=200, target=target)
        zz = dynamical_structure_factor(op, psi0, E0, re, "zz", k=200)
        g_lo, g_zz = lo.greens(z), zz.greens(z)
        dev_g = float((g_lo - g_zz / 2).abs().max() / g_zz.abs().max())
        worst_g = max(worst_g, dev_g)
        assert dev_g <= TOL, (m, dev_g)
        assert float(lo.poles.min()) > -1e-8 and float(zz.poles.min()) > -1e-8     # excitation energies
        want = zz_first_moment_from_correlators(bonds, [1.0] * L, re.numpy(), xy)
        scale = float((zz.weights * zz.poles.abs()).sum())
        dev_m = abs(zz.moment(1) - want) / scale
        worst_m = max(worst_m, dev_m)
        assert dev_m <= TOL, (m, dev_m)
        if m in (1, 3):
            both = dynamical_structure_factor(op, psi0, E0, (re, im), "zz", k=200)
            zz_im = dynamical_structure_factor(op, psi0, E0, im, "zz", k=200)
            assert len(both) == len(zz) + len(zz_im)
            assert float((both.greens(z) - g_zz - zz_im.greens(z)).abs().max()) <= TOL * float(both.greens(z).abs().max())
            cplx = dynamical_structure_factor(op, psi0, E0, torch.complex(re, im), "zz", k=200)
            assert float((cplx.greens(z) - both.greens(z)).abs().max()) <= TOL * float(both.greens(z).abs().max())
            want2 = want + zz_first_moment_from_correlators(bonds, [1.0] * L, im.numpy(), xy)
            assert abs(both.moment(1) - want2) <= TOL * float((both.weights * both.poles.abs()).sum())
    print("worst |G_- - G_zz / 2| / max|G_zz| = %.2e   worst f-sum deviation = %.2e" % (worst_g, worst_m))
    # target=None builds the Hamiltonian of the destination sector itself; "+" lands in ndown - 1 and sees the triplet as well
    re, _ = ring_momentum_weights(L, 5)
    auto = dynamical_structure_factor(op, psi0, E0, re, "-", k=200)
    up = dynamical_structure_factor(op, psi0, E0, re, "+", k=200)
    zz = dynamical_structure_factor(op, psi0, E0, re, "zz", k=200)
    for other in (auto, up):
        assert float((other.greens(z) - zz.greens(z) / 2).abs().max()) <= TOL * float(zz.greens(z).abs().max())
    with pytest.raises(ValueError):
        dynamical_structure_factor(op, psi0, E0, re, "xx")
    with pytest.raises(ValueError):
        dynamical_structure_factor(op, psi0, E0, re, "+", target=target)        # a target in the wrong sector


def test_structure_factor_on_the_pair_operator():
    """the same Heisenberg ring as an all-pair operator: target=None goes through the pair operator's constructor"""
    L, nd = 8, 4
    J = torch.zeros((L, L), dtype=F64)
    for a, b in ring_bonds(L):
        J[min(a, b), max(a, b)] = 1.0
    probe = sector(L, nd)
    op = SpinSectorPairOperator(L, probe.pack(J, J, 0.0), nd, device=dev(), _tables=probe._tables)
    H = sector_reference.dense(L, nd, ring_bonds(L), np.concatenate([np.ones(2 * L), np.zeros(L)]))
    E, V = np.linalg.eigh(H)
    re, _ = ring_momentum_weights(L, 4)
    lo = dynamical_structure_factor(op, to_dev(V[:, 0]), E[0], re, "-", k=56)
    zz = dynamical_structure_factor(op, to_dev(V[:, 0]), E[0], re, "zz", k=70)
    z = torch.complex(torch.linspace(-1.0, 24.0, 32, dtype=F64), torch.full((32,), 0.5, dtype=F64))
    amp = V.T @ ref.apply(L, nd, 0, re.numpy(), V[:, 0])
    dense = torch.from_numpy(np.sum(amp ** 2 / (z.numpy()[:, None] - (E - E[0])[None, :]), axis=1))
    assert float((zz.greens(z) - dense).abs().max()) <= TOL * float(dense.abs().max())
    assert float((lo.greens(z) - dense / 2).abs().max()) <= TOL * float(dense.abs().max())


def test_example_dynamics():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "spin_lattice", "dynamics.py")
    spec = importlib.util.spec_from_file_location("spin_lattice_dynamics", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    orig = CG.EPS_DEFAULT
    try:
        out = ex.main(L=10)
    finally:
        CG.EPS_DEFAULT = orig
    assert out["L"] == 10 and out["n"] == 252 and len(out["q"]) == 9
    for key in ("gap_zz", "gap_pm", "dcp", "first_moment", "f_sum", "static_zz"):
        assert len(out[key]) == 9 and all(math.isfinite(v) for v in out[key]), key
    for got, want in zip(out["first_moment"], out["f_sum"]):
        assert abs(got - want) <= 1e-8 * abs(want)
    # finite-size triplet gaps lie above the des Cloizeaux-Pearson lower boundary of the thermodynamic limit at q = pi
    assert out["gap_zz"][4] > 0.0 and abs(out["gap_zz"][4] - out["gap_pm"][4]) < 1e-8
    assert np.isfinite(out["S_zz"]).all() and np.isfinite(out["S_pm"]).all() and (np.asarray(out["S_zz"]) >= 0.0).all()
