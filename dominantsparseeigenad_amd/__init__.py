"""MI355X-native dominant-eigenpair autograd primitives (drop-in for DominantSparseEigenAD).

Sub-modules mirror the reference package layout (reference DominantSparseEigenAD/__init__.py is
empty; users import sub-modules by name):

    dominantsparseeigenad_amd.Lanczos   Lanczos, symeigLanczos
    dominantsparseeigenad_amd.CG        CG_torch, CGSubspace, setCGSubspaceSparse
    dominantsparseeigenad_amd.symeig    DominantSymeig, setDominantSparseSymeig
    dominantsparseeigenad_amd.eig       DominantEig, setDominantSparseEig
    dominantsparseeigenad_amd.operators TFIMOperator, CSROperator, Stencil3Operator (native mat-vecs)
                                        Bipartition (reduced density matrices and entanglement entropies of their vectors)
                                        SpinSectorLadder (sigma^-, sigma^+ and Z maps between magnetisation sectors)
                                        HubbardLadder (c+, c and n maps between Hubbard sectors), one_body_density_matrix
                                        HubbardCurrent (the bond current map of a Hubbard sector)
                                        HubbardPairLadder (pair and spin-flip maps between Hubbard sectors), pair_correlations,
                                        onsite_pairing, bond_pairing, total_spin
    dominantsparseeigenad_amd.spectral  lanczos_measure, SpectralMeasure, dynamical_structure_factor,
                                        hubbard_spectral_function, hubbard_pair_spectral_function, kpm_measure, kpm_structure_factor, optical_conductivity,
                                        OpticalResponse (re-exported here)
    dominantsparseeigenad_amd.thermal   block_lanczos_measures, sector_trace_measure, ThermalEnsemble, spin_thermodynamics,
                                        GrandCanonicalEnsemble, hubbard_thermodynamics, thermal_correlations,
                                        thermal_dynamics, ThermalDynamics, hubbard_thermal_dynamics, HubbardThermalDynamics, hubbard_thermal_conductivity, ThermalOpticalResponse, sector_density_of_states, spin_density_of_states, hubbard_density_of_states (finite
                                        temperature; re-exported here)
    dominantsparseeigenad_amd.chebyshev chebyshev_coefficients, exp_order, spectral_bounds, chebyshev_apply, expm_block,
                                        time_evolve (f(H) X without a basis), chebyshev_moments, jackson_kernel,
                                        lorentz_kernel, ChebyshevMeasure (moments and kernel polynomial densities; re-exported
                                        here)

The top-level ``DominantSparseEigenAD`` package in this repository re-exports the same modules
under the reference's import names.
"""
__version__ = "0.1.0"


def __getattr__(name):
    # the spectral functions under the package's own name, resolved on first use (the module imports torch and the engine)
    if name in ("spectral", "lanczos_measure", "SpectralMeasure", "dynamical_structure_factor",
                "hubbard_spectral_function", "hubbard_pair_spectral_function", "kpm_measure", "kpm_structure_factor", "optical_conductivity", "OpticalResponse"):
        import importlib
        mod = importlib.import_module(__name__ + ".spectral")
        return mod if name == "spectral" else getattr(mod, name)
    if name in ("thermal", "block_lanczos_measures", "sector_trace_measure", "ThermalEnsemble", "spin_thermodynamics",
                "GrandCanonicalEnsemble", "hubbard_thermodynamics", "thermal_correlations", "sector_density_of_states",
                "spin_density_of_states", "hubbard_density_of_states", "thermal_dynamics", "ThermalDynamics",
                "hubbard_thermal_dynamics", "HubbardThermalDynamics", "hubbard_thermal_conductivity",
                "ThermalOpticalResponse"):
        import importlib
        mod = importlib.import_module(__name__ + ".thermal")
        return mod if name == "thermal" else getattr(mod, name)
    if name in ("chebyshev", "chebyshev_coefficients", "exp_order", "spectral_bounds", "chebyshev_apply", "expm_block",
                "time_evolve", "chebyshev_moments", "jackson_kernel", "lorentz_kernel", "ChebyshevMeasure"):
        import importlib
        mod = importlib.import_module(__name__ + ".chebyshev")
        return mod if name == "chebyshev" else getattr(mod, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
