"""tests/cg_reference.py proved on the CPU (no GPU) before it judges a kernel (tests/test_gpu_cg_stages.py): the stage
references composed in longdouble ARE conjugate gradients (np.linalg.solve, oracle.cg_solve iterate for iterate, a dense
restricted solve for the deflated form); the phase sequence and the fused step give the same iterates; the exact class is exact
at every size and m of the GPU test; an honest fp64 evaluation with its sums in a random order passes every verdict; and each
of the wrong kernels of cg_reference.MUTANTS fails one -- through the same Checks and judges the GPU test drives the library
with.

Left to the exact class alone here (the random-class judges in longdouble take minutes at these sizes on a CPU): n = 2^21 + 3,
2^19 + 2049 and 2^22 + 5."""
import numpy as np
import pytest
import torch

import cg_reference as ref
import oracle
from cg_reference import DONE, ITERS, RESNORM, RR, RRNEW, Checks, HostImpl, Reference
from dominantsparseeigenad_amd.synthetic import normal_vector

LD = np.longdouble
QUIET = {"log": lambda *a: None}


def spd(n, seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    w = np.linspace(1.0, 9.0, n)
    return (Q * w) @ Q.T, Q, w


def compose_cg(R, A, b, x, eps, steps, fused, shift=None):
    """CG.py:24-41 from the stage references; returns the iterates x_1 .. and the final state"""
    Ax = A @ x if shift is None else R.shift_dot(x, A @ x, shift)[0]
    r, d, state = R.cg_init(b, Ax)
    state = R.cg_init_check(state, eps)
    xs = []
    for it in range(steps):
        if state[DONE] != 0:
            break
        Ad = A @ d
        if fused:
            x, r, d, _, state = R.cg_step(x, r, d, Ad, shift, state, eps, it)
        else:
            Ad, state[ref.DAD] = R.shift_dot(d, Ad, shift)
            x, r, state = R.cg_update(x, r, d, Ad, state)
            state = R.cg_check(state, eps)
            d = R.cg_direction(r, d, state)
        xs.append(x)
    return xs, state


def test_the_composed_stages_are_cg():
    n = 60
    A, _, _ = spd(n, 1)
    b, x0 = normal_vector(n, 2), normal_vector(n, 3)
    R = Reference(LD)
    AL = A.astype(LD)
    for fused in (False, True):
        xs, state = compose_cg(R, AL, b.astype(LD), x0.astype(LD), 1e-15, 4 * n, fused)
        assert state[DONE] == 1 and state[RESNORM] < 1e-15
        want = np.linalg.solve(A, b)
        assert np.max(np.abs(xs[-1].astype(np.float64) - want)) <= 1e-13 * np.max(np.abs(want))
        for k in (1, 2, 3, 5, 8, 13):                  # iterate for iterate with the oracle (fp64 torch)
            xo = oracle.cg_solve(torch.from_numpy(A), torch.from_numpy(b), torch.from_numpy(x0), eps=1e-300, maxiter=k).numpy()
            assert np.max(np.abs(xs[k - 1].astype(np.float64) - xo)) <= 1e-12 * np.max(np.abs(xo)), (fused, k)


def test_the_phase_sequence_and_the_fused_step_give_the_same_iterates():
    n = 45
    A, _, _ = spd(n, 4)
    b, x0 = normal_vector(n, 5), normal_vector(n, 6)
    R = Reference(np.float64)
    for shift in (None, -0.25):
        xa, sa = compose_cg(R, A, b, x0, 1e-11, 9, False, shift)
        xb, sb = compose_cg(R, A, b, x0, 1e-11, 9, True, shift)
        assert len(xa) == len(xb) == 9
        for k in range(9):
            assert ref.same(xa[k], xb[k]), k
        assert sa[ITERS] == sb[ITERS] == 9 and sa[RESNORM] == sb[RESNORM]
        assert sa[RR] == sb[RRNEW]                      # nine steps: the ninth (parity 0) wrote its rr to RRNEW, cg_check to RR


def test_the_composed_deflated_stages_solve_the_restricted_system():
    n, m = 50, 3
    A, Q, w = spd(n, 7)
    Psi = np.ascontiguousarray(Q[:, :m].T)
    b, x0 = normal_vector(n, 8), normal_vector(n, 9)
    shift = float(w[0])
    R = Reference(LD)
    AL, PL = A.astype(LD), Psi.astype(LD)
    x = R.block_project(x0, PL)[0]
    r, d, state = R.deflated_init(b, x, AL @ x, shift, PL, 1e-15)
    for it in range(4 * n):
        if state[DONE] != 0:
            break
        x, r, d, _, state = R.deflated_step(x, r, d, AL @ d, shift, PL, state, 1e-15, it)
        # Psi is orthonormal to fp64 rounding only (Gram defect g): one projection leaves |Psi r| <= g |c| ~ 1e-16 |r|, and x
        # collects one such term per step
        assert np.max(np.abs(PL @ r)) <= 1e-14 * np.linalg.norm(r.astype(np.float64)) and np.max(np.abs(PL @ x)) <= 1e-14 * (it + 2)
    assert state[DONE] == 1
    P = np.eye(n) - Psi.T @ Psi
    want = Q[:, m:] @ ((Q[:, m:].T @ (P @ b)) / (w[m:] - shift))
    assert np.max(np.abs(x.astype(np.float64) - want)) <= 1e-13 * np.max(np.abs(want))


CPU_SIZES = ref.SIZES_SMALL + (140001, 300001)


@pytest.mark.parametrize("n", CPU_SIZES)
def test_an_honest_fp64_evaluation_passes_every_verdict(n):
    """sums in a random permutation; both classes; every m of the GPU test"""
    worst = 0.0
    for m in [m for m in ref.MS if m <= n]:
        big = n > 4097
        c = Checks(HostImpl(Reference(np.float64, order=1000 + n + m)), prove=not big, **QUIET)
        worst = max(worst, c.all(n, m, random=(not big or m == 3)))
    assert worst <= 1.0
    print("n = %d: worst error / bound of an honest fp64 evaluation %.3f" % (n, worst))


def test_an_honest_fp64_evaluation_passes_the_chains():
    c = Checks(HostImpl(Reference(np.float64, order=77)), **QUIET)
    assert c.cg_step_chain() <= 1.0 and c.deflated_chain() <= 1.0


@pytest.mark.parametrize("n", ref.SIZES_LARGE + ref.SIZES_PHASE_EXTRA)
def test_the_exact_class_has_headroom_at_the_large_sizes(n):
    """(the small sizes prove it inside test_an_honest_fp64_evaluation_passes_every_verdict: prove = True)  Every sum of every
    exact-class case is exact in any order, and fp64 = longdouble on every vector before beta"""
    c = Checks(HostImpl(Reference(np.float64)), prove=True, **QUIET)
    for run in (c.shift_dot, c.project_out, c.cg_init, c.cg_update, c.cg_direction):
        run(n, random=False)
    if n in ref.SIZES_PHASE_EXTRA:
        return
    c.cg_step(n, random=False)
    c.cg_step_converged_and_done(n)
    for m in ref.MS:
        c.prove = m == 8 or n < (1 << 21)         # (2^21 + 3 rows: longdouble beside fp64 for the largest m only; the sums for all)
        c.block_project(n, m, random=False)
        c.deflated_init(n, m, random=False)
        c.deflated_step(n, m, random=False)


def test_the_largest_exact_sum_stays_far_below_2_to_the_53():
    n = (1 << 21) + 3
    x, r, d, Ad, shift, state, eps, it = ref.exact_step_inputs(n, 5, ref.SHIFT_EXACT, 0)
    Psi, support = ref.exact_psi_for("deflated_step", n, 8, 6, lambda P: (x, r, d, Ad, shift, P, state, eps, it), prove=False)
    _, largest = ref.assert_headroom("deflated_step", x, r, d, Ad, shift, Psi, state, eps, it, prove=False)
    assert support == "edges" and largest < 2.0 ** 50, (support, np.log2(largest))


def test_the_edge_rows_and_the_launch_geometry():
    assert list(ref.edge_rows(1)) == [0] and list(ref.edge_rows(513)) == [0, 511, 512]
    n = (1 << 21) + 3
    assert ref.tile_blocks(1 << 21) == 4096 and ref.tile_blocks(n) == 1025 and ref.ew_blocks((1 << 22) + 5) == 2048
    rows = set(ref.edge_rows(n))
    assert {0, n - 1, 511, 512, 1025 * 512 - 1, 1025 * 512, 3 * 1025 * 512 - 1, 3 * 1025 * 512} <= rows       # four trips
    # sum_partials_block, thread 0: 274 partials = one trip through both accumulators (threads 18 .. 255 take the tail read
    # instead); 586 = one trip and the tail read; 1025 (n = 2^21 + 3, the grid-stride form) = two trips and the tail read
    assert ref.tile_blocks(140001) == 274 and ref.partial_trips(274) == (1, False)
    assert ref.tile_blocks(300001) == 586 and ref.partial_trips(586) == (1, True)
    assert ref.partial_trips(1025) == (2, True)
    # k_cg_finalize_rrnew strides 256 threads over ew_blocks(n) partials: more than 256 from 2^19 + 1 rows on
    assert ref.ew_blocks((1 << 19) + 2049) == 258 and ref.ew_blocks(1 << 19) == 256


# (smallest n, m at which the wrong kernel differs from the right one), then a large size
SMALL = {"Psi rows j and j + 1 are swapped in the apply": (2, 2)}


@pytest.mark.parametrize("name", sorted(ref.MUTANTS))
@pytest.mark.parametrize("size", ["smallest", "large"])
def test_a_wrong_kernel_fails_a_verdict(name, size):
    n, m = SMALL.get(name, (1, 1)) if size == "smallest" else (140001, 3)
    c = Checks(HostImpl(ref.MUTANTS[name](np.float64, order=5)), prove=False, **QUIET)
    with pytest.raises(AssertionError):
        c.all(n, m, random=True)


@pytest.mark.parametrize("name", ["the wrong parity slot is read", "the new rr is written to the current slot", "beta is inverted",
                                  "beta is formed from the new slot before its update (fused tail)",
                                  "the re-projection is skipped", "m - 1 rows are used in place of m",
                                  "Psi rows j and j + 1 are swapped in the apply", "one partial block is dropped",
                                  "the last row of an odd n is dropped from a sum"])
def test_a_wrong_kernel_fails_the_random_class_alone(name):
    """the chains see only random-class judges (no bit comparison with a reference run): they reject these by the bounds"""
    c = Checks(HostImpl(ref.MUTANTS[name](np.float64, order=6)), **QUIET)
    with pytest.raises(AssertionError), np.errstate(all="ignore"):
        c.cg_step_chain()
        c.deflated_chain()
