"""Structure of the six couplings-parameterised operators (docs/design/30-couplings-operator-base.md): the binding protocol, the
handle, the differentiable mat-vec and its adjoint hook are written once, in ``_CouplingsOperator``, and the module has one pair
of ``autograd.Function``s for them.  No device: the classes are looked at, not instantiated."""
import inspect

import torch

from dominantsparseeigenad_amd import operators

FAMILIES = {
    "SpinChainOperator": ("set_tile_log2", "rows Jx, Jy, Jz, hx, hz"),
    "SpinLatticeOperator": ("set_tile_log2", "Jx(nb), Jy(nb), Jz(nb), hx(L), hz(L)"),
    "SpinSectorOperator": ("set_grid_log2", "Jxy(nb), Jz(nb), hz(L)"),
    "SpinSectorPairOperator": ("set_grid_log2", "Jxy(P), Jz(P), hz(L)"),
    "SpinSymmetrySectorOperator": ("set_grid_log2", "Jxy(nb), Jz(nb), hz(L)"),
    "HubbardOperator": ("set_grid_log2", "t(nb), V(nb), U(L), eps(L)"),
}
SHARED = ("couplings", "handle", "H", "__call__", "Hadjoint_to_couplingsadjoint", "_native_methods", "_view", "_forms")
OLD_FUNCTIONS = [stem + kind for stem in ("_Chain", "_Lattice", "_Sector", "_PairSector", "_SymSector", "_Hubbard")
                 for kind in ("Apply", "Forms")]


def test_the_shared_members_come_from_the_base():
    base = operators._CouplingsOperator
    assert base._native_methods == ("H", "__call__") and base.__call__ is base.H
    assert isinstance(base.__dict__["couplings"], property) and base.__dict__["couplings"].fset is not None
    for name, (setter, families) in FAMILIES.items():
        cls = getattr(operators, name)
        assert issubclass(cls, base), name
        for member in SHARED:
            assert member not in cls.__dict__, (name, member)
            assert getattr(cls, member) is getattr(base, member), (name, member)
        # what a family supplies itself: its handle factory, its family list, its forms entry and its one tuning setter
        assert "_create" in cls.__dict__ and "__init__" in cls.__dict__, name
        assert cls._families == families, name
        assert cls._forms_stem.startswith("dsea_op_"), name
        other = "set_grid_log2" if setter == "set_tile_log2" else "set_tile_log2"
        assert setter in cls.__dict__ and cls.__dict__[setter].__doc__ and not hasattr(cls, other), name
    assert operators.SpinSymmetrySectorOperator.pack is operators.SpinSectorOperator.pack
    assert operators.SpinSymmetrySectorOperator.unpack is operators.SpinSectorOperator.unpack


def test_the_sector_row_helpers_are_shared_by_the_two_sector_operators():
    for member in ("states", "rank", "embed", "restrict", "bipartition", "ladder"):
        owners = [cls for cls in operators.SpinSectorPairOperator.__mro__ if member in cls.__dict__]
        assert owners and owners[0] is not operators.SpinSectorPairOperator, member
        assert getattr(operators.SpinSectorOperator, member) is getattr(operators.SpinSectorPairOperator, member), member


def test_one_pair_of_autograd_functions_serves_the_six_operators():
    functions = [obj for obj in vars(operators).values()
                 if inspect.isclass(obj) and issubclass(obj, torch.autograd.Function) and obj.__module__ == operators.__name__]
    by_forward = {}
    for fn in functions:
        by_forward.setdefault(tuple(inspect.signature(fn.forward).parameters), []).append(fn.__name__)
    assert by_forward[("ctx", "v", "c", "op", "view")] == ["_CouplingsApply"]
    assert by_forward[("ctx", "v1", "v2", "op", "view")] == ["_CouplingsForms"]
    for old in OLD_FUNCTIONS:
        assert not hasattr(operators, old), old
    # the TFIM operator keeps its own function: a scalar parameter with a separate dH/dg handle is not this protocol
    assert by_forward[("ctx", "v", "g", "op")] == ["_TFIMApply"]


def test_the_library_stays_reachable_for_the_host_check_tests():
    assert operators._lib.load is not None and inspect.ismodule(operators._lib)
