"""The contract of ``_CouplingsOperator`` (docs/design/30-couplings-operator-base.md), checked the same way on each of the six
operator families, and on the symmetry sector once more with a spin-flip generator (its second create call).  Sizes are the
smallest at which every code path of the host layer is still taken:

    case             geometry                                                     n     couplings
    chain            L = 3                                                        8     (5, 3)
    lattice          L = 3, ring_bonds(3)                                         8     15
    sector           L = 4, ndown = 2, ring_bonds(4)                              6     12
    pairsector       L = 4, ndown = 2                                             6     16
    symsector        L = 4, ndown = 2, ring_bonds(4), momentum 0                  2     12
    symsector_flip   the same with spin_flip = +1                                 2     12
    hubbard          L = 3, nup = 1, ndn = 2, ring_bonds(3): two table sets       9     12

Tolerances.  Everything is float64 and bilinear in (vector, couplings), so central differences are exact to rounding:
``gradcheck`` and ``gradgradcheck`` run with their defaults, as in test_gpu_pairsector.py.  The rebinding and in-place checks
compare runs of the same kernel on the same numbers and ask for equal bits.

The refused couplings: the shape and the contiguity message names the class's coupling families; a float32 tensor is refused
one check earlier, by the message "couplings must be a float64 tensor on <device>", which names none (and keeps its text)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from dominantsparseeigenad_amd import operators as ops  # noqa: E402
from dominantsparseeigenad_amd.synthetic import normal_vector  # noqa: E402

F64 = torch.float64

# name -> (couplings shape, constructor from a couplings tensor, tuning setter, family list of the error message)
CASES = {
    "chain": ((5, 3), lambda c: ops.SpinChainOperator(3, c), "set_tile_log2", "rows Jx, Jy, Jz, hx, hz"),
    "lattice": ((15,), lambda c: ops.SpinLatticeOperator(3, ops.ring_bonds(3), c), "set_tile_log2",
                "Jx(nb), Jy(nb), Jz(nb), hx(L), hz(L)"),
    "sector": ((12,), lambda c: ops.SpinSectorOperator(4, ops.ring_bonds(4), c, 2), "set_grid_log2", "Jxy(nb), Jz(nb), hz(L)"),
    "pairsector": ((16,), lambda c: ops.SpinSectorPairOperator(4, c, 2), "set_grid_log2", "Jxy(P), Jz(P), hz(L)"),
    "symsector": ((12,), lambda c: ops.SpinSymmetrySectorOperator(4, ops.ring_bonds(4), c, 2, ops.ring_symmetries(4, momentum=0)),
                  "set_grid_log2", "Jxy(nb), Jz(nb), hz(L)"),
    "symsector_flip": ((12,), lambda c: ops.SpinSymmetrySectorOperator(4, ops.ring_bonds(4), c, 2,
                                                                       ops.ring_symmetries(4, momentum=0, spin_flip=1)),
                       "set_grid_log2", "Jxy(nb), Jz(nb), hz(L)"),
    "hubbard": ((12,), lambda c: ops.HubbardOperator(3, ops.ring_bonds(3), c, 1, 2), "set_grid_log2", "t(nb), V(nb), U(L), eps(L)"),
}
ROWS = {"chain": 8, "lattice": 8, "sector": 6, "pairsector": 6, "symsector": 2, "symsector_flip": 2, "hubbard": 9}
SEED = {name: 31000 + 10 * k for k, name in enumerate(CASES)}

case = pytest.mark.parametrize("name", list(CASES))


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (no fallback)"
    return torch.device("cuda:0")


def draw(shape, seed):
    count = 1
    for s in shape:
        count *= s
    return torch.from_numpy(normal_vector(count, seed).copy()).reshape(shape).contiguous().to(dev())


def fresh(name, which=0):
    """(operator, its couplings tensor) with the ``which``-th couplings of the case"""
    shape, make, _, _ = CASES[name]
    c = draw(shape, SEED[name] + which)
    op = make(c)
    assert op.n == op.dim == ROWS[name] >= 2 and tuple(op.couplings.shape) == shape and op.couplings is c
    return op, c


def vector(name, which):
    return draw((ROWS[name],), SEED[name] + 5 + which)


def table_tensors(op):
    return [t for attr in ("_tables", "_up", "_dn") if hasattr(op, attr) for t in getattr(op, attr)]


def kept_alive(op):
    """(the couplings tensor whose pointer the kernels of the bound handle read, the tables that handle keeps alive)"""
    keep = op._H._h.keepalive
    return (keep, ()) if torch.is_tensor(keep) else keep


@case
def test_the_matvec_is_differentiable_twice_in_the_vector_and_the_couplings(name):
    op, c = fresh(name)

    def apply(v, c):
        op.couplings = c
        return op.H(v)

    args = (vector(name, 0).requires_grad_(True), c.requires_grad_(True))
    assert torch.autograd.gradcheck(apply, args)
    assert torch.autograd.gradgradcheck(apply, args)


@case
def test_the_forms_are_differentiable_twice_in_both_vectors(name):
    op, _ = fresh(name)
    args = (vector(name, 1).requires_grad_(True), vector(name, 2).requires_grad_(True))
    out = op.Hadjoint_to_couplingsadjoint(*args)
    assert tuple(out.shape) == CASES[name][0]
    assert torch.autograd.gradcheck(op.Hadjoint_to_couplingsadjoint, args)
    assert torch.autograd.gradgradcheck(op.Hadjoint_to_couplingsadjoint, args)


@case
def test_a_rebinding_makes_a_new_handle_on_the_same_tables_and_keeps_the_tuning(name):
    op, c1 = fresh(name)
    setter = CASES[name][2]
    getattr(op, setter)(6)
    assert op._H.tune_log2 == 6
    before, tables, groups = op.handle.value, table_tensors(op), [getattr(op, a, None) for a in ("_tables", "_up", "_dn")]
    c2 = draw(CASES[name][0], SEED[name] + 1)
    op.couplings = c2
    assert op.couplings is c2 and op.handle.value != before
    assert all(getattr(op, a, None) is g for a, g in zip(("_tables", "_up", "_dn"), groups))
    data, kept = kept_alive(op)
    assert data.data_ptr() == c2.data_ptr()                  # the handle keeps alive the tensor its kernels read
    assert len(kept) == len(tables) and all(any(t is u for u in tables) for t in kept)
    assert op._H.tune_log2 == 6                              # the new view carries the tuning
    twin, _ = fresh(name, 1)
    getattr(twin, setter)(6)
    v = vector(name, 0)
    assert torch.equal(op.H(v), twin.H(v))
    assert not torch.equal(op.H(v), CASES[name][1](c1).H(v))
    # ... and so does the adjoint handle of the forms' backward: same bits as on the twin
    v1, v2 = vector(name, 1).requires_grad_(True), vector(name, 2)
    w = draw(CASES[name][0], SEED[name] + 3)
    (g,) = torch.autograd.grad((op.Hadjoint_to_couplingsadjoint(v1, v2) * w).sum(), v1)
    (g_twin,) = torch.autograd.grad((twin.Hadjoint_to_couplingsadjoint(v1, v2) * w).sum(), v1)
    assert torch.equal(g, g_twin)


@case
def test_an_in_place_update_is_seen_through_the_same_handle(name):
    op, c = fresh(name)
    v = vector(name, 0)
    before, y0 = op.handle.value, op.H(v)
    delta = draw(CASES[name][0], SEED[name] + 4)
    with torch.no_grad():
        op.couplings.add_(delta)
    assert op.handle.value == before and op.couplings is c
    y1 = op.H(v)
    other, _ = fresh(name)
    other.couplings = draw(CASES[name][0], SEED[name]) + delta
    assert torch.equal(y1, other.H(v)) and not torch.equal(y1, y0)


@case
def test_refused_couplings_raise_value_errors_that_name_the_families(name):
    op, c = fresh(name)
    shape, _, _, families = CASES[name]
    handle = op.handle.value
    longer = shape[:-1] + (shape[-1] + 1,)
    with pytest.raises(ValueError) as err:
        op.couplings = torch.zeros(longer, dtype=F64, device=dev())
    assert families in str(err.value) and str(shape) in str(err.value)
    strided = torch.zeros(shape[:-1] + (2 * shape[-1],), dtype=F64, device=dev())[..., ::2]
    assert tuple(strided.shape) == shape and not strided.is_contiguous()
    with pytest.raises(ValueError) as err:
        op.couplings = strided
    assert families in str(err.value)
    with pytest.raises(ValueError) as err:
        op.couplings = torch.zeros(shape, dtype=torch.float32, device=dev())
    assert "float64" in str(err.value)
    assert op.couplings is c and op.handle.value == handle      # a refused tensor leaves the binding as it was
