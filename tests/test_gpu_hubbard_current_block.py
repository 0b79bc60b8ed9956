"""The column dots of the Hubbard bond current map and the finite-temperature optical response on the GPU
(docs/design/40-finite-temperature-conductivity.md): k_hubbard_current_block_dots<R> against the longdouble twin of
tests/hubbard_current_block_reference.py at the shapes of tests/test_gpu_hubbard_current.py (the table is copied, not imported),
against the unfused product, bit for bit across calls and widths, the C entry's refusals, and
``thermal.hubbard_thermal_conductivity`` sampled against the twin on the same start vectors, dense against the 4^4 Fock space, and
at low temperature against ``spectral.optical_conductivity``.

    L, nup, ndn             n_up x n_dn = n          bonds                           what it reaches
    2,1,1                   2 x 2 = 4                (0,1) (0,1) (1,0)               less than a wave; repeated and reversed bond
    5,2,3                   10 x 10 = 100            random + one reversed, 7        n_dn < 64; chunks of 4 and of 2 end ragged
    5,2,3 five              100                      the first 5 of them             a ragged second chunk of 4, third chunk of 2
    6,3,3                   20 x 20 = 400            the ten bonds of the loop       two blocks, ragged last block: the thread past
                                                     lattice                         the last row adds nothing
    7,3,2                   35 x 21 = 735            (0,6) (5,6) (2,3) (1,4)         odd L; sign masks inside lo, inside hi, across
    7,3,2 one               735                      (6,0)                           one bond: a single ragged chunk at every R
    8,4,4                   70 x 70 = 4 900          complete graph, 28              n_dn = 70: waves straddle an ru boundary
    9,3,5                   84 x 126 = 10 584        complete graph cycled to 128    full bond table; two different table sets
    10,5,5, grid cap 2^6    252 x 252 = 63 504       24 random                       249 row ranges on 64 blocks: the accumulator
                                                                                     survives the ranges a block walks
    40,2,1                  780 x 40 = 31 200        ring + 10 random                words and sign masks wider than 32 bits
"""
import functools
import importlib.util
import math
import os
from ctypes import byref, c_int64, c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hubbard_current_block_reference as twin  # noqa: E402
import hubbard_reference as hub  # noqa: E402
import lattice_reference  # noqa: E402
from dominantsparseeigenad_amd import _lib, engine, thermal  # noqa: E402
from dominantsparseeigenad_amd.operators import HubbardOperator, hubbard_dim, ring_bonds  # noqa: E402
from dominantsparseeigenad_amd.spectral import optical_conductivity  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402

F64 = torch.float64
LD = np.longdouble
CAP = _lib.LATTICE_MAX_BONDS
LOOP_BONDS = ((0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (0, 3), (1, 4), (2, 5), (0, 2))
TOL = 1e-10


def small_bonds(L):
    """random pairs with one of them listed again reversed; at L = 2 that is (0, 1) more than once"""
    bonds = lattice_reference.random_bonds(L, L + 1, 7500 + L)
    a, b = bonds[0]
    return tuple(bonds + [(b, a)]) if L > 2 else ((0, 1), (0, 1), (1, 0))


def cyclic_complete(L, count):
    full = lattice_reference.complete_bonds(L)
    return tuple(full[i % len(full)] for i in range(count))


def ring_and_random(L):
    return tuple(ring_bonds(L) + lattice_reference.random_bonds(L, 10, 7600 + L))


# name -> (L, nup, ndn, log2 of the grid cap or None for the default, bonds)
GEOMETRY = {
    "L2-1-1": (2, 1, 1, None, small_bonds(2)),
    "L5-2-3": (5, 2, 3, None, small_bonds(5)),
    "L5-2-3-five": (5, 2, 3, None, small_bonds(5)[:5]),
    "L6-3-3-loops": (6, 3, 3, None, LOOP_BONDS),
    "L7-3-2-split": (7, 3, 2, None, ((0, 6), (5, 6), (2, 3), (1, 4))),
    "L7-3-2-one": (7, 3, 2, None, ((6, 0),)),
    "L8-4-4-complete": (8, 4, 4, None, tuple(lattice_reference.complete_bonds(8))),
    "L9-3-5-cap": (9, 3, 5, None, cyclic_complete(9, CAP)),
    "L10-5-5-walk": (10, 5, 5, 6, tuple(lattice_reference.random_bonds(10, 24, 7510))),
    "L40-2-1": (40, 2, 1, None, ring_and_random(40)),
}


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


def to_dev(a):
    return torch.from_numpy(np.array(a)).to(dev())      # (a copy: the cached case arrays are read-only)


def operator(name):
    """the operator of a case: the current map reads its sector, tables, bonds and grid cap, not its couplings"""
    L, nup, ndn, grid, bonds = GEOMETRY[name]
    op = HubbardOperator(L, bonds, torch.zeros(2 * len(bonds) + 2 * L, dtype=F64, device=dev()), nup, ndn)
    if grid is not None:
        op.set_grid_log2(grid)
    return op


@functools.lru_cache(maxsize=None)
def case(name):
    """(w, X [n, 8], Lft [n, 8], K X in float64, the longdouble dots, the twin's own fp64 - longdouble deviation), computed once
    per case and never written to; column 5 of X is zero"""
    L, nup, ndn, _, bonds = GEOMETRY[name]
    nb, n = len(bonds), hubbard_dim(L, nup, ndn)
    w = normal_vector(2 * nb, 4100 + L + nb).reshape(2, nb).copy()
    X = normal_vector(n * 8, 4200 + L + nup).reshape(n, 8).copy()
    Lft = normal_vector(n * 8, 4300 + L + nup).reshape(n, 8).copy()
    X[:, 5] = 0.0
    KX = twin.apply_block(L, nup, ndn, bonds, w, X)
    d_ld = twin.dots(L, nup, ndn, bonds, w, Lft, X, LD)
    own = np.abs(twin.dots(L, nup, ndn, bonds, w, Lft, X) - d_ld).astype(np.float64)
    d_want = d_ld.astype(np.float64)
    for a in (w, X, Lft, KX, d_want, own):
        a.setflags(write=False)
    return w, X, Lft, KX, d_want, own


def bars(name):
    """max(1e-13, 10 x the twin's fp64 - longdouble deviation) |l_j| |(K X)_j| per column, and the scale"""
    _, X, Lft, KX, _, own = case(name)
    scale = np.linalg.norm(Lft, axis=0) * np.linalg.norm(KX, axis=0)
    rel = np.where(scale > 0, own / np.where(scale > 0, scale, 1.0), 0.0)
    return np.maximum(1e-13, 10.0 * rel) * scale, scale


def entry(op, R, w, Lft, X, out, scratch):
    with torch.cuda.device(dev()):
        return _lib.load().dsea_op_hubbard_current_block_dots(op.handle, R, c_void_p(w.data_ptr()), c_void_p(Lft.data_ptr()),
                                                              c_void_p(X.data_ptr()), c_void_p(out.data_ptr()),
                                                              c_void_p(scratch.data_ptr()), engine._stream(dev()))


def scratch_for(op, R, fill=0.0):
    need = c_int64()
    assert _lib.load().dsea_op_hubbard_current_block_dots_scratch_doubles(int(op.N), int(op.nup), int(op.ndn), R, byref(need)) == 0
    return torch.full((need.value,), fill, dtype=F64, device=dev())


def test_the_cases_are_what_the_table_says():
    sizes = {name: hubbard_dim(*g[:3]) for name, g in GEOMETRY.items()}
    assert [sizes[k] for k in GEOMETRY] == [4, 100, 100, 400, 735, 735, 4900, 10584, 63504, 31200]
    counts = [len(g[4]) for g in GEOMETRY.values()]
    assert counts == [3, 7, 5, 10, 4, 1, 28, CAP, 24, 50]
    assert (sizes["L6-3-3-loops"] + 255) // 256 == 2 and sizes["L6-3-3-loops"] % 256 != 0
    assert (sizes["L10-5-5-walk"] + 255) // 256 == 249 > (1 << GEOMETRY["L10-5-5-walk"][3]) == 64
    assert (39, 0) in GEOMETRY["L40-2-1"][4] and max(hub.states(40, 2)) >= 1 << 32


@pytest.mark.parametrize("R", [1, 2, 4, 8])
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_the_c_entry_against_the_longdouble_twin(name, R):
    w, X, Lft, _, d_want, _ = case(name)
    bar, scale = bars(name)
    op = operator(name)
    cols = [0, 5, 7, 3, 1, 2, 4, 6][:R]                              # (the zero column is in every width above 1)
    wd = to_dev(w).reshape(-1)
    Xd, Ld = to_dev(X[:, cols]).contiguous(), to_dev(Lft[:, cols]).contiguous()
    out = torch.full((R,), -7.0, dtype=F64, device=dev())
    assert entry(op, R, wd, Ld, Xd, out, scratch_for(op, R, -7.0)) == 0
    err = np.abs(out.cpu().numpy() - d_want[cols])
    print("%s R = %d: max |dots - longdouble twin| / scale = %.2e"
          % (name, R, float((err / np.where(scale[cols] > 0, scale[cols], 1.0)).max())))
    assert (err <= bar[cols]).all(), (err, bar[cols])
    again = torch.full((R,), -7.0, dtype=F64, device=dev())
    assert entry(op, R, wd, Ld, Xd, again, scratch_for(op, R, 3.0)) == 0 and torch.equal(again, out)   # whatever the scratch held


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_block_dots(name):
    L, nup, ndn, grid, bonds = GEOMETRY[name]
    w, X, Lft, _, d_want, _ = case(name)
    bar, scale = bars(name)
    op = operator(name)
    cur = op.current()
    wd, Xd, Ld = to_dev(w), to_dev(X), to_dev(Lft)
    got = cur.block_dots(wd, Ld, Xd)
    assert got.shape == (8,) and got.dtype == F64 and got.device.type == "cuda" and not got.requires_grad
    assert (np.abs(got.cpu().numpy() - d_want) <= bar).all()
    unfused = (Ld * cur.apply_block(wd, Xd)).sum(0)
    assert (np.abs((got - unfused).cpu().numpy()) <= bar).all()
    assert float(got[5]) == 0.0                                     # the zero column
    assert torch.equal(cur.block_dots(wd, Ld, Xd), got)             # fixed-order sums, no atomics
    for j in (0, 5, 7):                                             # column j of the R = 8 call is the R = 1 call on that column
        assert torch.equal(cur.block_dots(wd, Ld[:, j:j + 1], Xd[:, j:j + 1])[0], got[j])
    # K is antisymmetric: x . K x = 0 and l . K x = -x . K l, up to the rounding of the two sums
    same = cur.block_dots(wd, Xd, Xd).cpu().numpy()
    self_bar = np.maximum(1e-13, bar / np.where(scale > 0, scale, 1.0)) * np.linalg.norm(X, axis=0) * np.linalg.norm(case(name)[3], axis=0)
    assert (np.abs(same) <= self_bar).all()
    back = cur.block_dots(wd, Xd, Ld).cpu().numpy()
    assert (np.abs(got.cpu().numpy() + back) <= bar).all()
    # one species' weights zero: the other species alone
    for s in (0, 1):
        ws = np.array(w)
        ws[s] = 0.0
        want = twin.dots(L, nup, ndn, bonds, ws, Lft, X, LD).astype(np.float64)
        assert (np.abs(cur.block_dots(to_dev(ws), Ld, Xd).cpu().numpy() - want) <= bar).all()
    if grid is not None:                                            # a walked grid against the default one
        op.set_grid_log2(12)                                        # (the cap at creation)
        try:
            flat = cur.block_dots(wd, Ld, Xd)
        finally:
            op.set_grid_log2(grid)
        assert (np.abs((flat - got).cpu().numpy()) <= bar).all()


@pytest.mark.parametrize("R", [3, 13])
@pytest.mark.parametrize("name", ["L5-2-3", "L6-3-3-loops", "L10-5-5-walk"])
def test_block_dots_takes_any_width(name, R):
    w, X, Lft, _, d_want, _ = case(name)
    bar, _ = bars(name)
    cur = operator(name).current()
    cols = [j % 8 for j in range(R)]
    got = cur.block_dots(to_dev(w), to_dev(Lft[:, cols]), to_dev(X[:, cols]))
    assert got.shape == (R,) and (np.abs(got.cpu().numpy() - d_want[cols]) <= bar[cols]).all()
    single = cur.block_dots(to_dev(w), to_dev(Lft[:, :1]), to_dev(X[:, :1]))
    assert torch.equal(got[0], single[0]) and (R < 9 or torch.equal(got[8], single[0]))


def test_c_abi_refusals_leave_the_outputs_alone():
    name = "L7-3-2-split"
    w, X, Lft, _, _, _ = case(name)
    op = operator(name)
    wd, Xd, Ld = to_dev(w).reshape(-1), to_dev(X), to_dev(Lft)
    out = torch.full((8,), -7.0, dtype=F64, device=dev())
    scratch = scratch_for(op, 8, -7.0)
    assert scratch.numel() == 8 * 3
    lib, st = _lib.load(), engine._stream(dev())
    P = lambda t, off=0: c_void_p(t.data_ptr() + off)  # noqa: E731
    assert Xd.data_ptr() % 16 == 0 and Ld.data_ptr() % 16 == 0

    def dots(h=op.handle, R=8, wt=P(wd), Lf=P(Ld), X=P(Xd), o=P(out), s=P(scratch)):
        return lib.dsea_op_hubbard_current_block_dots(h, R, wt, Lf, X, o, s, st)

    assert dots(X=P(Xd, 8)) == -2 and dots(Lf=P(Ld, 8)) == -2                               # DSEA_ERR_ALIGN
    for R in (3, 0, 16):
        assert dots(R=R) == _lib.ERR_ARG
    for null in ("h", "wt", "Lf", "X", "o", "s"):
        assert dots(**{null: None}) == _lib.ERR_ARG, null
    assert dots(X=P(Xd, 8), o=None) == _lib.ERR_ARG                                         # the argument checks come first
    from dominantsparseeigenad_amd.operators import SpinSectorOperator
    spin = SpinSectorOperator(7, ring_bonds(7), torch.zeros(2 * 7 + 7, dtype=F64, device=dev()), 3, dev())
    assert dots(h=spin.handle) == _lib.ERR_ARG                    # an operator of another kind
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((scratch == -7.0).all())                      # nothing refused has run
    assert dots(R=1, X=P(Xd, 8), Lf=P(Ld, 8)) == 0                                          # R = 1 needs 8-byte alignment only
    cur = op.current()
    with pytest.raises(ValueError):
        cur.block_dots(to_dev(w), Ld[:, :4], Xd)
    with pytest.raises(ValueError):
        cur.block_dots(to_dev(w), Ld.cpu(), Xd)


# ---- hubbard_thermal_conductivity
BETAS = [0.0, 0.5, 2.0]
MUS = [-0.4, 0.9]


@functools.lru_cache(maxsize=None)
def ring_model(L):
    """a ring plus one extra bond with random t, V, U and eps, and the displacements of its bonds"""
    bonds = tuple(ring_bonds(L)) + ((0, 2),)
    p = normal_vector(hub.nparam(L, bonds), 9980 + L).copy()
    p[:len(bonds)] = 1.0 + 0.3 * p[:len(bonds)]
    d = np.array([1.0] * L + [2.0])
    for a in (p, d):
        a.setflags(write=False)
    return bonds, p, d


SAMPLED = {4: [(2, 2), (3, 2), (1, 3)], 5: [(2, 2), (3, 2), (2, 4)]}


@pytest.mark.parametrize("kind", ["charge", "spin"])
@pytest.mark.parametrize("L", [4, 5])
def test_sampled_against_the_twin(L, kind):
    """dense_below = 0 on bulk sectors: every sector runs on the thermal pure quantum states, through the block current map,
    time_evolve and the fused dots, against the longdouble twin on the same start vectors.  |C - twin| <= 1e-13 orders C(0), the
    bar of docs/design/37-hubbard-finite-temperature-dynamics.md section 37.7; K_d within 1e-12 sum |t d^2|."""
    bonds, p, d = ring_model(L)
    R, seed, dt, steps = 4, 11, 0.3, 6
    got = thermal.hubbard_thermal_conductivity(L, bonds, to_dev(p), torch.from_numpy(d.copy()), BETAS, MUS, dt, steps, kind=kind, R=R,
                                               seed=seed, dense_below=0, sectors=SAMPLED[L])
    want = twin.sampled(L, bonds, p, d, kind, BETAS, MUS, dt, steps, SAMPLED[L], R=R, seed=seed, dtype=LD)
    assert got.correlation.shape == (3, 2, steps + 1) and got.correlation.dtype == torch.complex128 and got.correlation.device.type == "cpu"
    assert torch.equal(got.times, dt * torch.arange(steps + 1, dtype=F64)) and got.diamagnetic.shape == got.logXi.shape == (3, 2)
    C, ref_C = got.correlation.numpy(), want["C"]
    static = ref_C[:, :, 0].real
    assert (static > 0).all() and want["orders"][:, 1:].min() > 0
    bar = 1e-13 * np.maximum(want["orders"], 1.0)[:, None, :] * static[:, :, None]
    err = np.abs(C - ref_C)
    kd_err = np.abs(got.diamagnetic.numpy() - want["K_d"]).max()
    kd_bar = 1e-12 * float(np.abs(p[:len(bonds)] * d * d).sum())
    print("L = %d %s: worst |C - twin| / (1e-13 orders C(0)) = %.3f (orders up to %d), |K_d - twin| = %.2e (bar %.2e)"
          % (L, kind, float((err / bar).max()), int(want["orders"].max()), kd_err, kd_bar))
    assert (err <= bar).all()
    assert kd_err <= kd_bar
    assert (np.abs(got.logXi.numpy() - want["logXi"]) <= 1e-13 * np.maximum(want["orders"][:, :1], 10.0)).all()
    assert torch.equal(got.static(), got.correlation[:, :, 0].real)


@pytest.mark.parametrize("kind", ["charge", "spin"])
def test_dense_against_the_full_fock_space(kind):
    """L = 4, all 25 sectors at the default dense_below: every sector is dense (at most 36 rows); against the trace over all 4^4
    states, and ``stiffness`` against the twin's exactly broadened formula on the same grid (eta t_K = 10).  The grid is [-2, 10]:
    at omega < 0 g_beta = (e^{beta |omega|} - 1) / |omega| multiplies the rounding of S (about 1e-16 C(0)) and the window's cut
    (e^{-50} C(0)); at beta = 2 and omega = -2 that factor is 27, which leaves both far below 1e-10 K_d, while at omega = -20
    it would be 1e16."""
    L = 4
    bonds, p, d = ring_model(L)
    eta, dt = 0.5, 0.05
    steps = int(round(10.0 / (eta * dt)))
    got = thermal.hubbard_thermal_conductivity(L, bonds, to_dev(p), torch.from_numpy(d.copy()), BETAS, MUS, dt, steps, kind=kind)
    want = twin.full_space(L, bonds, p, d, kind, BETAS, MUS, dt * np.arange(steps + 1))
    scale = want["C"][:, :, :1].real
    err = np.abs(got.correlation.numpy() - want["C"]) / scale
    kd_err = np.abs(got.diamagnetic.numpy() - want["K_d"]).max()
    xi_err = np.abs(got.logXi.numpy() - want["logXi"]).max()
    print("%s: |C - full space| / C(0) = %.2e, |K_d - full space| = %.2e, |ln Xi - full space| = %.2e"
          % (kind, float(err.max()), kd_err, xi_err))
    assert (scale > 0).all() and (err <= TOL).all() and kd_err <= TOL and xi_err <= TOL
    assert eta * dt * steps >= 8.0
    omega = np.linspace(-2.0, 10.0, 1201)
    exact = twin.broadened(L, bonds, p, d, kind, BETAS, MUS, omega, eta)
    stiff_err = np.abs(got.stiffness(omega, eta).numpy() - exact["stiffness"])
    print("%s: |stiffness - exactly broadened| / K_d = %.2e (beta > 0)" % (kind, float((stiff_err[1:] / np.abs(exact["K_d"][1:])).max())))
    assert (stiff_err[1:] <= TOL * np.abs(exact["K_d"][1:])).all()
    # beta = 0: tr T_d = 0, so K_d is rounding (1e-16) and no scale; g_0 = 0 makes the weight exactly 0 and the stiffness K_d itself,
    # which is held to the full space above
    assert BETAS[0] == 0.0 and not got.weight(omega, eta)[0].any() and torch.equal(got.stiffness(omega, eta)[0], got.diamagnetic[0])
    assert np.abs(exact["K_d"][0]).max() <= 1e-14 and not exact["weight"][0].any()


def test_the_zero_temperature_limit():
    """L = 6 ring, U = 4, the sector (3, 3) alone and dense, beta large: ``diamagnetic`` and ``static()`` against K_d and the total
    weight of ``optical_conductivity`` on the dense ground state, within 10 e^{-beta gap} scale + 1e-8"""
    L, U, beta = 6, 4.0, 40.0
    bonds = tuple(ring_bonds(L))
    p = np.array([1.0] * L + [0.0] * L + [U] * L + [0.0] * L)
    d = np.ones(L)
    lam, vec = np.linalg.eigh(hub.dense(L, 3, 3, bonds, p))
    gap = float(lam[1] - lam[0])
    assert gap > 0.05
    op = HubbardOperator(L, bonds, to_dev(p), 3, 3)
    zero = optical_conductivity(op, to_dev(vec[:, 0].copy()), float(lam[0]), torch.from_numpy(d.copy()))
    got = thermal.hubbard_thermal_conductivity(L, bonds, to_dev(p), torch.from_numpy(d.copy()), [beta], [0.0], 0.1, 1,
                                               sectors=[(3, 3)], dense_below=400)
    total = float(zero.measure.weights.sum())
    slack = 10.0 * math.exp(-beta * gap)
    # the excited levels' K_d and <K^T K> are bounded by sum |t d^2| * 2 and |K|^2 <= (2 sum |t d|)^2
    kd_scale, w_scale = 2.0 * L, (2.0 * 2.0 * L) ** 2
    print("gap = %.4f  K_d: %.10f against %.10f   <K^T K>: %.10f against %.10f"
          % (gap, float(got.diamagnetic[0, 0]), zero.diamagnetic, float(got.static()[0, 0]), total))
    assert abs(float(got.diamagnetic[0, 0]) - zero.diamagnetic) <= slack * kd_scale + 1e-8
    assert abs(float(got.static()[0, 0]) - total) <= slack * w_scale + 1e-8


def test_example_thermal_optical():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "hubbard", "thermal_optical.py")
    spec = importlib.util.spec_from_file_location("hubbard_thermal_optical", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = ex.main(L=4)                                              # every sector is dense: at most 36 rows
    assert out["L"] == 4 and len(out["T"]) == 2
    sigma = np.asarray(out["sigma"])
    assert sigma.shape == (2, len(out["omega"])) and np.isfinite(sigma).all() and sigma.min() >= -1e-9
    K_d, weight, stiffness = (np.asarray(out[k]) for k in ("diamagnetic", "weight", "stiffness"))
    assert (K_d > 0).all() and (weight > 0).all()
    assert np.abs(math.pi * K_d - (weight + math.pi * stiffness)).max() <= 1e-12 * math.pi * K_d.max()
