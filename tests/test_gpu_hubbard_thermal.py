"""The basis-free block Lanczos run on the Hubbard block mat-vec and the grand-canonical layer on the GPU
(docs/design/28-hubbard-finite-temperature.md) against the numpy twin of tests/hubbard_block_reference.py.

Short runs (k = 12) compare the coefficients alpha, beta themselves.  The bar is not a constant: per coefficient, in units of
B = sum_t (2 |t_t| + 4 |V_t|) + sum_i (|U_i| + 2 |eps_i|) >= ||H||, it is max(1e-13, 10 x the largest deviation between the twin in
float64 and the twin in longdouble on the same inputs) -- computed here; 10 x because the GPU's reduction order differs from
both.  Long runs (k = 60) lose orthogonality, after which coefficients of two correct runs differ at order one BY CONSTRUCTION;
what they must agree on is the quadrature: ln Z, E and C of the measures, to the project's 1e-10 (absolute for ln Z, 1e-10 B for
E, 1e-10 beta^2 B^2 for C).  The stochastic path is compared with the twin on the same seeds, never with exact numbers: the
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

import hubbard_block_reference as twin  # noqa: E402
import hubbard_reference as ref  # noqa: E402
import test_gpu_hubbard as base  # noqa: E402
from dominantsparseeigenad_amd import thermal  # noqa: E402
from dominantsparseeigenad_amd.operators import HubbardLadder, HubbardOperator, hubbard_dim, ring_momentum_weights  # noqa: E402
from dominantsparseeigenad_amd.spectral import SpectralMeasure, hubbard_spectral_function  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402
from dominantsparseeigenad_amd.thermal import ThermalEnsemble  # noqa: E402

F64 = torch.float64
TOL = 1e-10
SHORT = {"L6-3-3": "L6-3-3-loops", "L8-4-4": "L8-4-4-complete", "L10-5-5": "L10-5-5-walk"}
BETAS3 = np.array([0.1, 1.0, 4.0])
BETAS5 = np.array([0.05, 0.2, 0.7, 1.5, 3.0])
MUS3 = np.array([-0.8, 0.6, 2.2])
FUNCTIONS = ("logZ", "energy", "density", "compressibility", "spin_susceptibility", "specific_heat", "entropy")


def geometry(name):
    L, nup, ndn, _, bonds = base.GEOMETRY[name]
    return L, nup, ndn, bonds, base.couplings(L, bonds, "random")


@functools.lru_cache(maxsize=None)
def short_case(name):
    """(Phi (n, 8), the twin's (norm2, alphas, betas, steps) in float64, the largest float64-longdouble deviation of a
    coefficient in units of B, B) at k = 12, once per geometry"""
    L, nup, ndn, bonds, p = geometry(SHORT[name])
    n = hubbard_dim(L, nup, ndn)
    Phi = twin.start_block(n, 8, 28100 + L)
    Phi.setflags(write=False)
    lo = twin.block_lanczos(L, nup, ndn, bonds, p, Phi, 12, np.float64)
    hi = twin.block_lanczos(L, nup, ndn, bonds, p, Phi, 12, np.longdouble)
    B = twin.coupling_bound(L, bonds, p)
    dev = max(float(np.abs(lo[i] - hi[i]).max()) for i in (1, 2)) / B
    return Phi, lo, dev, B


def test_the_walk_case_is_capped_at_64_blocks():
    assert base.GEOMETRY[SHORT["L10-5-5"]][3] == 6 and hubbard_dim(10, 5, 5) > 64 * 256


@pytest.mark.parametrize("R", [4, 8])
@pytest.mark.parametrize("name", list(SHORT))
def test_short_runs_have_the_coefficients_of_the_twin(name, R):
    Phi, (norm2_t, alphas_t, betas_t, steps_t), twin_dev, B = short_case(name)
    op = base.operator(SHORT[name], geometry(SHORT[name])[4])
    first = thermal.block_lanczos_coefficients(op, base.to_dev(Phi[:, :R]), 12)
    norm2, alphas, betas, steps = first
    assert steps.tolist() == [12] * R and list(steps_t[:R]) == [12] * R
    bar = max(1e-13, 10.0 * twin_dev)
    got = max(float(np.abs(alphas.numpy() - np.asarray(alphas_t[:, :R], dtype=np.float64)).max()),
              float(np.abs(betas.numpy() - np.asarray(betas_t[:, :R], dtype=np.float64)).max())) / B
    print("%s R = %d: twin float64 vs longdouble %.2e B, GPU vs twin %.2e B, bar %.2e B" % (name, R, twin_dev, got, bar))
    assert got <= bar
    assert float(np.abs(norm2.numpy() / np.asarray(norm2_t[:R], dtype=np.float64) - 1.0).max()) <= 1e-13
    again = thermal.block_lanczos_coefficients(op, base.to_dev(Phi[:, :R]), 12)
    assert all(torch.equal(a, b) for a, b in zip(first, again))                 # two runs: identical bits


def thermo_of(poles, weights, betas):
    """ln Z, E and C of one measure as plain sums"""
    poles, weights = np.asarray(poles), np.asarray(weights)
    out = np.zeros((3, len(betas)))
    for i, beta in enumerate(betas):
        low = poles.min()
        terms = weights * np.exp(-beta * (poles - low))
        prob = terms / terms.sum()
        E = float(prob @ poles)
        out[:, i] = math.log(terms.sum()) - beta * low, E, beta ** 2 * float(prob @ (poles - E) ** 2)
    return out


def test_long_runs_agree_in_the_quadrature_not_in_the_coefficients():
    """k = 60 on L8-4-4 with random site-dependent couplings, no re-orthogonalisation"""
    L, nup, ndn, bonds, p = geometry("L8-4-4-complete")
    B = twin.coupling_bound(L, bonds, p)
    Phi = twin.start_block(hubbard_dim(L, nup, ndn), 8, 28200)
    parts = twin.block_measures(L, nup, ndn, bonds, p, Phi, 60)
    op = base.operator("L8-4-4-complete", p)
    measures = thermal.block_lanczos_measures(op, base.to_dev(Phi), 60)
    assert len(measures) == 8
    worst = [0.0, 0.0, 0.0]
    for meas, (poles, weights) in zip(measures, parts):
        assert meas.steps == 60 and len(meas) == 60
        ens = ThermalEnsemble([(meas, 0.0)])
        beta = torch.tensor(BETAS3)
        got = (ens.logZ(beta).numpy(), ens.energy(beta).numpy(), ens.specific_heat(beta).numpy())
        want = thermo_of(poles, weights, BETAS3)
        dev = [np.abs(got[0] - want[0]), np.abs(got[1] - want[1]) / B, np.abs(got[2] - want[2]) / (BETAS3 ** 2 * B ** 2)]
        for i in range(3):
            worst[i] = max(worst[i], float(dev[i].max()))
    print("k = 60, L8-4-4, R = 8: ln Z %.2e (bar 1e-10), E %.2e B (bar 1e-10 B), C %.2e beta^2 B^2 (bar 1e-10 beta^2 B^2)"
          % tuple(worst))
    assert worst[0] <= TOL and worst[1] <= TOL and worst[2] <= TOL


def test_breakdown_is_per_column_and_nothing_is_left_undefined():
    name = "L6-3-3-loops"
    L, nup, ndn, bonds, p = geometry(name)
    n = hubbard_dim(L, nup, ndn)
    E, V = np.linalg.eigh(ref.dense(L, nup, ndn, bonds, p))
    pick, coef = [0, n // 2, n - 1], np.array([0.6, -0.5, 0.7])
    Phi = twin.start_block(n, 8, 28300)
    Phi[:, 0] = V[:, pick] @ coef
    op = base.operator(name, p)
    first = thermal.block_lanczos_coefficients(op, base.to_dev(Phi), 12)
    norm2, alphas, betas, steps = first
    assert steps.tolist() == [3] + [12] * 7
    assert all(bool(torch.isfinite(t).all()) for t in (norm2, alphas, betas))
    assert bool((alphas[3:, 0] == 0.0).all()) and bool((betas[2:, 0] == 0.0).all()) and bool((betas[:, 1:] > 0.0).all())
    meas = thermal.block_lanczos_measures(op, base.to_dev(Phi), 12)
    assert meas[0].steps == 3 and [m.steps for m in meas[1:]] == [12] * 7
    assert float((meas[0].poles - torch.from_numpy(E[pick])).abs().max()) <= TOL
    assert float((meas[0].weights - torch.from_numpy(coef ** 2)).abs().max()) <= TOL
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
    L2, nup2, ndn2, bonds2, p2 = geometry("L3-1-2")
    op2 = base.operator("L3-1-2", p2)
    out = thermal.block_lanczos_coefficients(op2, base.to_dev(twin.start_block(9, 3, 28310)), 50)
    assert out[1].shape == (9, 3) and all(bool(torch.isfinite(t).all()) for t in out[:3])


def model(L, seed):
    """the ring plus two chords (one written from the higher site), random site-dependent U and eps, random t and V"""
    bonds = tuple((i, (i + 1) % L) for i in range(L)) + ((L // 2, 0), (1, L - 2))
    return bonds, normal_vector(ref.nparam(L, bonds), seed)


def test_exact_sectors_give_the_thermodynamics_of_dense_diagonalisation():
    """L = 4 with the default dense_below: every sector is exact (the largest has 36 rows)"""
    L = 4
    bonds, p = model(L, 28400)
    ens = thermal.hubbard_thermodynamics(L, bonds, torch.from_numpy(p), device=base.dev())
    entries = twin.exact_entries(L, bonds, p)
    assert ens.poles.numel() == 4 ** L and ens.moment(0) == 4 ** L and len(ens.entries) == 25
    beta, mu = torch.tensor(BETAS5).reshape(5, 1), torch.tensor(MUS3).reshape(1, 3)
    both = thermal.hubbard_thermodynamics(L, bonds, torch.from_numpy(p), spin_symmetric=False, device=base.dev())
    for name in FUNCTIONS:
        got, want = getattr(ens, name)(beta, mu).numpy(), getattr(twin, name)(entries, BETAS5, MUS3)
        assert got.shape == (5, 3)
        assert np.all(np.abs(got - want) <= TOL * np.maximum(1.0, np.abs(want))), (name, got, want)
        other = getattr(both, name)(beta, mu).numpy()
        assert np.all(np.abs(other - want) <= TOL * np.maximum(1.0, np.abs(want))), (name, other, want)


def thermo_bars(betas, B, L):
    """the bars of the seven quantities on the grid [beta, mu]: 1e-10 x the natural scale of each"""
    b = betas[:, None] * np.ones((1, len(MUS3)))
    return {"logZ": TOL * np.ones_like(b), "energy": TOL * B * np.ones_like(b), "specific_heat": TOL * b ** 2 * B ** 2,
            "entropy": TOL * (1.0 + b * B), "density": TOL * L * np.ones_like(b), "compressibility": TOL * b * L ** 2,
            "spin_susceptibility": TOL * b * (0.5 * L) ** 2}


def test_stochastic_sectors_give_the_thermodynamics_of_the_twin_on_the_same_seeds():
    """L = 6, dense_below = 64, R = 4, k = 30: the sectors of 90 rows and more run the block recurrence"""
    L = 6
    bonds, p = model(L, 28500)
    B = twin.coupling_bound(L, bonds, p)
    ens = thermal.hubbard_thermodynamics(L, bonds, torch.from_numpy(p), R=4, k=30, seed=3, dense_below=64, device=base.dev())
    entries = twin.entries(L, bonds, p, R=4, k=30, seed=3, dense_below=64)
    assert [(e[1], e[2]) for e in ens.entries] == [(e[2], e[3]) for e in entries]
    assert [len(e[0]) for e in ens.entries] == [len(e[0]) for e in entries]
    stochastic = [len(e[0]) for e in entries if math.comb(L, e[2]) * math.comb(L, e[3]) >= 90 and 0 < e[2] < L and 0 < e[3] < L]
    assert stochastic and all(count == 4 * 30 for count in stochastic)          # no run broke down
    assert ens.moment(0) == pytest.approx(4 ** L, rel=1e-12)
    beta, mu = torch.tensor(BETAS5).reshape(5, 1), torch.tensor(MUS3).reshape(1, 3)
    bars = thermo_bars(BETAS5, B, L)
    for name in FUNCTIONS:
        got, want = getattr(ens, name)(beta, mu).numpy(), getattr(twin, name)(entries, BETAS5, MUS3)
        print("%s: worst deviation / bar = %.3g" % (name, float((np.abs(got - want) / bars[name]).max())))
        assert np.all(np.abs(got - want) <= bars[name]), (name, got, want)


def test_the_basis_free_spectral_function_is_the_default_one():
    """L = 6 at (3, 3), c_up at q = 2 pi 2 / L (complex weights: a block of two columns), k = n_dst = 300.  The bar is measured:
    the twin's measure without re-orthogonalisation against the dense resolvent on the CPU, times ten."""
    name = "L6-3-3-loops"
    L, nup, ndn, bonds, p = geometry(name)
    E, V = np.linalg.eigh(ref.dense(L, nup, ndn, bonds, p))
    op0 = base.operator(name, p)
    target = HubbardOperator(L, bonds, base.to_dev(p), nup - 1, ndn)
    psi0 = base.to_dev(V[:, 0])
    weights = ring_momentum_weights(L, 2)
    k = target.n
    assert k == 300
    default = hubbard_spectral_function(op0, psi0, E[0], weights, "c_up", k=k, target=target)
    free = hubbard_spectral_function(op0, psi0, E[0], weights, "c_up", k=k, target=target, basis_free=True)
    B = twin.coupling_bound(L, bonds, p)
    z = torch.complex(torch.linspace(-B, B, 64, dtype=F64), torch.full((64,), 0.5, dtype=F64))
    # the twin on the CPU: the same two vectors, no re-orthogonalisation, against the dense resolvent of the destination sector
    lad = HubbardLadder(op0, target, "up")
    Phi = np.stack([lad(c.to(base.dev()), psi0).cpu().numpy() for c in weights], axis=1)
    Ed, Vd = np.linalg.eigh(ref.dense(L, nup - 1, ndn, bonds, p))
    amp2 = ((Vd.T @ Phi) ** 2).sum(axis=1)
    dense = torch.from_numpy(np.sum(amp2 / (z.numpy()[:, None] - (Ed - E[0])[None, :]), axis=1))
    parts = twin.block_measures(L, nup - 1, ndn, bonds, p, Phi, k)
    poles = np.concatenate([t for t, _ in parts]) - E[0]
    wts = np.concatenate([w for _, w in parts])
    twin_G = SpectralMeasure(poles, wts, float(wts.sum()), len(poles)).greens(z)
    scale = float(dense.abs().max())
    twin_dev = float((twin_G - dense).abs().max()) / scale
    bar = 10.0 * twin_dev
    got = float((free.greens(z) - default.greens(z)).abs().max()) / scale
    print("basis-free vs default G(omega + 0.5i): %.2e of max|G|; twin vs dense %.2e; bar %.2e" % (got, twin_dev, bar))
    assert got <= bar
    assert free.norm2 == pytest.approx(default.norm2, rel=1e-12)
    real = hubbard_spectral_function(op0, psi0, E[0], weights[0], "n", k=20, basis_free=True)     # one column, in the sector
    assert real.norm2 == pytest.approx(hubbard_spectral_function(op0, psi0, E[0], weights[0], "n", k=20).norm2, rel=1e-12)


def test_example_thermodynamics(capsys):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "hubbard", "thermodynamics.py")
    spec = importlib.util.spec_from_file_location("hubbard_thermodynamics_example", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = ex.main(L=4)
    printed = capsys.readouterr().out
    assert out["L"] == 4 and out["dimension"] == 256
    assert max(abs(v - 4.0) for v in out["N_half"]) <= 1e-8             # particle-hole symmetry at mu = U / 2
    assert "largest |<N> - L| at mu = U / 2" in printed
    assert float(printed.rsplit(":", 1)[1]) <= 1e-8
    assert all(math.isfinite(v) and v >= 0.0 for key in ("S", "C", "chi_s") for v in out[key])
    assert out["S"][-1] == pytest.approx(math.log(4.0), abs=1e-3)        # T = 64 t
    middle = len(out["mu"]) // 2
    assert out["n"][0][middle] == pytest.approx(1.0, abs=1e-8)           # the plateau at T = 0.1 t
    assert all(a <= b + 1e-12 for f in out["n"] for a, b in zip(f, f[1:]))      # n(mu) does not decrease
