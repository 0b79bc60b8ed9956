"""examples/spin_lattice/thermal_correlations.py at L = 8 (every sector exact): the numbers it prints against identities of the
Heisenberg ring and against the dense full-space averages of the twin."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import sector_cheb_reference as twin  # noqa: E402
from dominantsparseeigenad_amd.operators import ring_bonds  # noqa: E402


def test_example_thermal_correlations(capsys):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "spin_lattice", "thermal_correlations.py")
    spec = importlib.util.spec_from_file_location("spin_lattice_thermal_correlations", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    L = 8
    out = mod.main(L=L)
    printed = capsys.readouterr().out
    assert "S(pi)" in printed and len(printed.splitlines()) == 2 + len(out["T"])
    T, nn, energy, Spi = (np.array(out[k]) for k in ("T", "nn", "energy", "S_pi"))
    assert np.abs(nn - energy / (4.0 * L)).max() <= 1e-12                  # H = 4 J1 sum_i S_i . S_{i+1}
    p = np.array([1.0] * L + [1.0] * L + [0.0] * L)
    want = twin.full_space_correlations(L, ring_bonds(L), p, 1.0 / T)
    SS = (want["xy"] + want["zz"]) / 4.0
    sign = (-1.0) ** (np.arange(L)[:, None] - np.arange(L)[None, :])
    assert np.abs(Spi - (sign[None] * SS).sum(axis=(1, 2)) / L).max() <= 1e-10
    assert np.abs(energy - want["energy"]).max() <= 1e-10 * 3.0 * L
    assert abs(Spi[0] - 0.75) < 0.05 and Spi[-1] > 2.0 * Spi[0]               # T = 64 J1 is near the limit; order grows on cooling
    assert nn[0] > -0.02 and np.all(np.diff(nn) < 0)                        # antiferromagnetic bonds strengthen on cooling
