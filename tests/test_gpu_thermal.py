"""The basis-free block Lanczos run and the finite-temperature layer on the GPU (docs/design/27-finite-temperature.md) against
the numpy twin of tests/sector_block_reference.py.

Short runs (k = 12) compare the coefficients alpha, beta themselves.  The bar is not a constant: per coefficient, in units of
B = sum_t (2 |Jxy_t| + |Jz_t|) + sum_i |hz_i| >= ||H||, it is max(1e-13, 10 x the largest deviation between the twin in float64
and the twin in longdouble on the same inputs) -- computed here; 10 x because the GPU's reduction order differs from both.
Long runs (k = 60) lose orthogonality, after which coefficients of two correct runs differ at order one BY CONSTRUCTION; what
they must agree on is the quadrature: ln Z, E and C of the measures, to the project's 1e-10 (absolute for ln Z, 1e-10 B for E,
1e-10 beta^2 B^2 for C).  The stochastic path is compared with the twin on the same seeds, never with exact numbers: the
difference to exact numbers is sampling error.
"""
import functools
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sector_block_reference as twin  # noqa: E402
import sector_reference as ref  # noqa: E402
import test_gpu_sector as base  # noqa: E402
from dominantsparseeigenad_amd import thermal  # noqa: E402
from dominantsparseeigenad_amd.operators import SpinSectorLadder, SpinSectorOperator, ring_bonds, ring_momentum_weights  # noqa: E402
from dominantsparseeigenad_amd.spectral import SpectralMeasure, dynamical_structure_factor  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402
from dominantsparseeigenad_amd.thermal import ThermalEnsemble  # noqa: E402

F64 = torch.float64
TOL = 1e-10
SHORT = {"L8-4": "L8-4-complete", "L11-5": "L11-5", "L16-8": "L16-8"}
BETAS3 = np.array([0.1, 1.0, 4.0])
BETAS5 = np.array([0.05, 0.2, 0.7, 1.5, 3.0])


def geometry(name):
    L, ndown, _, bonds = base.GEOMETRY[name]
    return L, ndown, bonds, base.couplings(L, bonds, "random")


@functools.lru_cache(maxsize=None)
def short_case(name):
    """(Phi (n, 8), the twin's (norm2, alphas, betas, steps) in float64, the largest float64-longdouble deviation of a
    coefficient in units of B) at k = 12, once per geometry"""
    L, ndown, bonds, p = geometry(SHORT[name])
    n = math.comb(L, ndown)
    Phi = twin.start_block(n, 8, 27100 + L)
    Phi.setflags(write=False)
    lo = twin.block_lanczos(L, ndown, bonds, p, Phi, 12, np.float64)
    hi = twin.block_lanczos(L, ndown, bonds, p, Phi, 12, np.longdouble)
    B = twin.coupling_bound(L, bonds, p)
    dev = max(float(np.abs(lo[i] - hi[i]).max()) for i in (1, 2)) / B
    return Phi, lo, dev, B


@pytest.mark.parametrize("R", [4, 8])
@pytest.mark.parametrize("name", list(SHORT))
def test_short_runs_have_the_coefficients_of_the_twin(name, R):
    L, ndown, bonds, p = geometry(SHORT[name])
    Phi, (norm2_t, alphas_t, betas_t, steps_t), twin_dev, B = short_case(name)
    op = SpinSectorOperator(L, bonds, base.to_dev(p), ndown)
    norm2, alphas, betas, steps = thermal.block_lanczos_coefficients(op, base.to_dev(Phi[:, :R]), 12)
    assert steps.tolist() == [12] * R and list(steps_t[:R]) == [12] * R
    bar = max(1e-13, 10.0 * twin_dev)
    got = max(float(np.abs(alphas.numpy() - np.asarray(alphas_t[:, :R], dtype=np.float64)).max()),
              float(np.abs(betas.numpy() - np.asarray(betas_t[:, :R], dtype=np.float64)).max())) / B
    print("%s R = %d: twin float64 vs longdouble %.2e B, GPU vs twin %.2e B, bar %.2e B" % (name, R, twin_dev, got, bar))
    assert got <= bar
    assert float(np.abs(norm2.numpy() / np.asarray(norm2_t[:R], dtype=np.float64) - 1.0).max()) <= 1e-13


@functools.lru_cache(maxsize=None)
def heisenberg_12():
    L, ndown = 12, 6
    bonds = tuple(ring_bonds(L))
    p = np.array([1.0] * L + [1.0] * L + [0.0] * L)
    Phi = twin.start_block(math.comb(L, ndown), 8, 27200)
    Phi.setflags(write=False)
    return L, ndown, bonds, p, Phi, twin.block_measures(L, ndown, bonds, p, Phi, 60)


def thermo_of(poles, weights, betas):
    entries = [(np.asarray(poles), np.asarray(weights), 0.0)]
    return twin.logZ(entries, betas), twin.energy(entries, betas), twin.specific_heat(entries, betas)


def test_long_runs_agree_in_the_quadrature_not_in_the_coefficients():
    L, ndown, bonds, p, Phi, parts = heisenberg_12()
    B = twin.coupling_bound(L, bonds, p)
    op = SpinSectorOperator(L, bonds, base.to_dev(p), ndown)
    measures = thermal.block_lanczos_measures(op, base.to_dev(Phi), 60)
    assert len(measures) == 8
    worst = [0.0, 0.0, 0.0]
    for j, (meas, (poles, weights)) in enumerate(zip(measures, parts)):
        assert meas.steps == 60 and len(meas) == 60
        ens = ThermalEnsemble([(meas, 0.0)])
        beta = torch.tensor(BETAS3)
        got = (ens.logZ(beta).numpy(), ens.energy(beta).numpy(), ens.specific_heat(beta).numpy())
        want = thermo_of(poles, weights, BETAS3)
        dev = [np.abs(got[0] - want[0]), np.abs(got[1] - want[1]) / B, np.abs(got[2] - want[2]) / (BETAS3 ** 2 * B ** 2)]
        for i in range(3):
            worst[i] = max(worst[i], float(dev[i].max()))
    print("k = 60, L12-6, R = 8: ln Z %.2e (bar 1e-10), E %.2e B (bar 1e-10 B), C %.2e beta^2 B^2 (bar 1e-10 beta^2 B^2)"
          % tuple(worst))
    assert worst[0] <= TOL and worst[1] <= TOL and worst[2] <= TOL


def test_breakdown_is_per_column_and_nothing_is_left_undefined():
    L, ndown, bonds, p = geometry("L8-4-complete")
    n = math.comb(L, ndown)
    E, V = np.linalg.eigh(ref.dense(L, ndown, bonds, p))
    pick, coef = [0, n // 2, n - 1], np.array([0.6, -0.5, 0.7])
    Phi = twin.start_block(n, 8, 27300)
    Phi[:, 0] = V[:, pick] @ coef
    op = SpinSectorOperator(L, bonds, base.to_dev(p), ndown)
    first = thermal.block_lanczos_coefficients(op, base.to_dev(Phi), 12)
    norm2, alphas, betas, steps = first
    assert steps.tolist() == [3] + [12] * 7
    assert all(bool(torch.isfinite(t).all()) for t in (norm2, alphas, betas))
    assert bool((alphas[3:, 0] == 0.0).all()) and bool((betas[2:, 0] == 0.0).all()) and bool((betas[:, 1:] > 0.0).all())
    meas = thermal.block_lanczos_measures(op, base.to_dev(Phi), 12)
    assert meas[0].steps == 3 and [m.steps for m in meas[1:]] == [12] * 7
    assert float((meas[0].poles - torch.from_numpy(E[pick])).abs().max()) <= TOL
    assert float((meas[0].weights - torch.from_numpy(coef ** 2)).abs().max()) <= TOL
    again = thermal.block_lanczos_coefficients(op, base.to_dev(Phi), 12)
    assert all(torch.equal(a, b) for a, b in zip(first, again))                 # two runs: identical bits
    # a zero column beside live ones, at another width
    Phi4 = Phi[:, 1:5].copy()
    Phi4[:, 2] = 0.0
    norm2, alphas, betas, steps = thermal.block_lanczos_coefficients(op, base.to_dev(Phi4), 12)
    assert steps.tolist() == [12, 12, 0, 12] and float(norm2[2]) == 0.0
    assert bool((alphas[:, 2] == 0.0).all()) and bool((betas[:, 2] == 0.0).all())
    assert all(bool(torch.isfinite(t).all()) for t in (norm2, alphas, betas))
    meas = thermal.block_lanczos_measures(op, base.to_dev(Phi4), 12)
    assert len(meas[2]) == 0 and meas[2].steps == 0 and len(meas[3]) == 12
    # k is cut to n, and a width that goes through the host split
    L2, nd2, bonds2, p2 = geometry("L5-2")
    op2 = SpinSectorOperator(L2, bonds2, base.to_dev(p2), nd2)
    out = thermal.block_lanczos_coefficients(op2, base.to_dev(twin.start_block(10, 3, 27310)), 50)
    assert out[1].shape == (10, 3) and all(bool(torch.isfinite(t).all()) for t in out[:3])


def thermo_bars(betas, B, L):
    """the bars of the five quantities: 1e-10 absolute for ln Z, 1e-10 B for E, 1e-10 beta^2 B^2 for C, their sum rule for
    S = ln Z + beta E, and 1e-10 beta (L / 2)^2 for chi (m^2 <= (L / 2)^2)"""
    return {"logZ": TOL * np.ones_like(betas), "energy": TOL * B * np.ones_like(betas), "specific_heat": TOL * betas ** 2 * B ** 2,
            "entropy": TOL * (1.0 + betas * B), "susceptibility": TOL * betas * (0.5 * L) ** 2}


def model(L, seed):
    bonds = tuple(ring_bonds(L)) + ((0, L // 2), (1, L - 2))
    return bonds, normal_vector(ref.nparam(L, bonds), seed)


def test_exact_sectors_give_the_thermodynamics_of_dense_diagonalisation():
    """L = 8 with the default dense_below: every sector is exact"""
    L = 8
    bonds, p = model(L, 27400)
    ens = thermal.spin_thermodynamics(L, bonds, torch.from_numpy(p), device=base.dev())
    entries = twin.exact_entries(L, bonds, p)
    assert ens.poles.numel() == 2 ** L and ens.moment(0) == 2 ** L
    beta = torch.tensor(BETAS5)
    for name in ("logZ", "energy", "specific_heat", "entropy", "susceptibility"):
        got, want = getattr(ens, name)(beta).numpy(), getattr(twin, name)(entries, BETAS5)
        assert np.all(np.abs(got - want) <= TOL * np.maximum(1.0, np.abs(want))), (name, got, want)


def test_stochastic_sectors_give_the_thermodynamics_of_the_twin_on_the_same_seeds():
    """L = 10, dense_below = 0, R = 4, k = 40: every sector but the two one-state sectors runs the block recurrence"""
    L = 10
    bonds, p = model(L, 27500)
    B = twin.coupling_bound(L, bonds, p)
    ens = thermal.spin_thermodynamics(L, bonds, torch.from_numpy(p), R=4, k=40, seed=3, dense_below=0, device=base.dev())
    entries = twin.spin_entries(L, bonds, p, R=4, k=40, seed=3, dense_below=0)
    assert [len(m) for m, _ in ens.entries] == [len(e[0]) for e in entries]
    assert ens.moment(0) == pytest.approx(2 ** L, rel=1e-12)
    beta = torch.tensor(BETAS5)
    bars = thermo_bars(BETAS5, B, L)
    for name in ("logZ", "energy", "specific_heat", "entropy", "susceptibility"):
        got, want = getattr(ens, name)(beta).numpy(), getattr(twin, name)(entries, BETAS5)
        print("%s: worst deviation / bar = %.3g" % (name, float((np.abs(got - want) / bars[name]).max())))
        assert np.all(np.abs(got - want) <= bars[name]), (name, got, want)


def test_the_basis_free_structure_factor_is_the_default_one():
    """L = 10, sigma^-_q at q = 2 pi 3 / L (complex weights: a block of two columns), k = n_dst.  The bar is measured: the twin's
    measure without re-orthogonalisation against the dense resolvent on the CPU, times ten, at least 1e-10."""
    L, ndown = 10, 5
    bonds, p = model(L, 27600)
    E, V = np.linalg.eigh(ref.dense(L, ndown, bonds, p))
    op0 = SpinSectorOperator(L, bonds, base.to_dev(p), ndown)
    target = SpinSectorOperator(L, bonds, base.to_dev(p), ndown + 1)
    psi0 = base.to_dev(V[:, 0])
    weights = ring_momentum_weights(L, 3)
    k = target.n
    default = dynamical_structure_factor(op0, psi0, E[0], weights, "-", k=k, target=target)
    free = dynamical_structure_factor(op0, psi0, E[0], weights, "-", k=k, target=target, basis_free=True)
    z = torch.complex(torch.linspace(-2.0, 2.5 * twin.coupling_bound(L, bonds, p), 64, dtype=F64), torch.full((64,), 0.5, dtype=F64))
    # the twin on the CPU: the same two vectors, no re-orthogonalisation, against the dense resolvent of the destination sector
    lad = SpinSectorLadder(op0, target)
    Phi = np.stack([lad(c.to(base.dev()), psi0).cpu().numpy() for c in weights], axis=1)
    Ed, Vd = np.linalg.eigh(ref.dense(L, ndown + 1, bonds, p))
    amp2 = ((Vd.T @ Phi) ** 2).sum(axis=1)
    dense = torch.from_numpy(np.sum(amp2 / (z.numpy()[:, None] - (Ed - E[0])[None, :]), axis=1))
    parts = twin.block_measures(L, ndown + 1, bonds, p, Phi, k)
    poles = np.concatenate([t for t, _ in parts]) - E[0]
    wts = np.concatenate([w for _, w in parts])
    twin_G = SpectralMeasure(poles, wts, float(wts.sum()), len(poles)).greens(z)
    scale = float(dense.abs().max())
    twin_dev = float((twin_G - dense).abs().max()) / scale
    bar = max(TOL, 10.0 * twin_dev)
    got = float((free.greens(z) - default.greens(z)).abs().max()) / scale
    print("basis-free vs default G(omega + 0.5i): %.2e of max|G|; twin vs dense %.2e; bar %.2e" % (got, twin_dev, bar))
    assert got <= bar
    assert free.norm2 == pytest.approx(default.norm2, rel=1e-12)
    with pytest.raises(ValueError):
        dynamical_structure_factor(op0.pair_operator(), psi0, E[0], weights, "zz", k=8, basis_free=True)


def test_example_thermodynamics():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "spin_lattice", "thermodynamics.py")
    spec = importlib.util.spec_from_file_location("spin_lattice_thermodynamics", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = ex.main(L=8)
    assert out["L"] == 8 and out["dimension"] == 256 and out["second_moment"] == pytest.approx(24.0, rel=1e-12)
    # the high-temperature limits at the hottest point (T = 64 J1): next order is relative O(beta J1)
    assert out["C"][-1] == pytest.approx(out["C_limit"][-1], rel=0.1)
    assert out["chi"][-1] == pytest.approx(out["chi_limit"][-1], rel=0.1)
    assert all(math.isfinite(v) and v >= 0.0 for key in ("C", "chi", "S") for v in out[key])
    assert out["S"][-1] == pytest.approx(math.log(2.0), abs=1e-3)
