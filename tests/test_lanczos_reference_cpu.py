"""tests/lanczos_reference.py proved on the CPU (no GPU) before it judges a kernel (tests/test_gpu_lanczos_stages.py): the stage
references composed in longdouble ARE the Lanczos recurrence (oracle.lanczos_tridiag step for step); the phase sequence and the
fused step give the same fp64 iterates; the exact class is exact at every size of the GPU test; an honest fp64 evaluation with
its sums in a random order passes every verdict; and each of the wrong kernels of lanczos_reference.MUTANTS fails one -- through
the same Checks and judges the GPU test drives the library with.

Every size of the GPU test is judged here in both classes, except the set_split(16) sizes 102401 and 230401 and the grid-stride
size 2^20 + 129, which are left to the exact class (their random cases add nothing the neighbouring sizes do not show and cost
the most longdouble work)."""
import numpy as np
import pytest
import torch

import lanczos_reference as ref
import oracle
from lanczos_reference import SENTINEL, Checks, HostImpl, Reference

LD = np.longdouble
QUIET = {"log": lambda *a: None}


def honest(n, prove=True):
    return Checks(HostImpl(Reference(np.float64, order=1000 + n)), prove=prove, **QUIET)


# ---- composition ------------------------------------------------------------------------------------------------------------
def compose(R, A, q0, k, fused):
    """Lanczos.py:49-77 from the stage references: (Q rows, alphas, betas)"""
    n = q0.size
    Q = np.full((k, n), SENTINEL, dtype=R.dtype)
    Q[0], _ = R.scale_store(q0, R.dot(q0, q0))
    al, be = np.full(k, SENTINEL, dtype=R.dtype), np.full(k, SENTINEL, dtype=R.dtype)
    for i in range(1, k):
        u = A @ Q[i - 1]
        if fused:
            Q, al, be, _ = R.callable_step(Q, i, u, al, be)
        else:
            al[i - 1] = R.callable_alpha(Q[i - 1], u)
            r, c = R.rdots(Q, i, u, al[i - 1], be[i - 2] if i >= 2 else None)
            r, nrm2 = R.axpy_norm(Q, i, c, r)
            Q, be[i - 1] = R.store_row(r, nrm2, Q, i)
    al[k - 1] = R.callable_alpha(Q[k - 1], A @ Q[k - 1])
    return Q, al, be[:k - 1]


def symmetric(n, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    return (M + M.T) / 2.0


def test_the_composed_stages_are_the_lanczos_recurrence():
    n, k = 60, 20
    A = symmetric(n, 1)
    draws = [torch.from_numpy(np.random.default_rng(2 + t).standard_normal(n)) for t in range(2)]
    it = iter(draws)
    Qo, ao, bo = oracle.lanczos_tridiag(torch.from_numpy(A), k, draw=lambda n_, dtype: next(it), with_history=True)
    for fused in (False, True):
        Q, al, be = compose(Reference(LD), A.astype(LD), draws[0].numpy().astype(LD), k, fused)
        assert np.max(np.abs(al.astype(np.float64) - ao.numpy())) <= 1e-12
        assert np.max(np.abs(be.astype(np.float64) - bo.numpy())) <= 1e-12
        for i in range(k):                                   # step for step: every basis vector
            assert np.max(np.abs(Q[i].astype(np.float64) - Qo.numpy()[:, i])) <= 1e-11, (fused, i)


def test_the_phase_sequence_and_the_fused_step_give_the_same_iterates():
    n, k = 45, 12
    A = symmetric(n, 3)
    q0 = np.random.default_rng(4).standard_normal(n)
    a, b = compose(Reference(np.float64), A, q0, k, False), compose(Reference(np.float64), A, q0, k, True)
    for x, y in zip(a, b):
        assert ref.same(x, y)


# ---- an honest evaluation passes; the exact class has headroom --------------------------------------------------------------
@pytest.mark.parametrize("n", ref.SIZES_SPLIT16)
def test_an_honest_fp64_evaluation_passes_every_verdict_at_the_small_sizes(n):
    c = honest(n)
    worst = c.small(n)
    assert worst <= 1.0
    print("n = %d: %d cases, worst error / bound of an honest fp64 evaluation %.3f" % (n, c.cases, worst))


def test_an_honest_fp64_evaluation_passes_the_chain():
    assert honest(77).callable_chain() <= 1.0


BIG_RANDOM = (ref.SIZE_SPLIT8,) + ref.SIZES_NT2 + ref.SIZES_WAVE


@pytest.mark.parametrize("n", (ref.SIZE_SPLIT8,) + ref.SIZES_NT2 + ref.SIZES_WAVE + ref.SIZES_FINALIZE + (ref.SIZE_GRID_STRIDE,))
def test_an_honest_fp64_evaluation_passes_at_the_large_sizes(n):
    """the calls of the GPU test at this size (fp64 beside longdouble on every exact vector up to 131202 rows; the sums of every
    case at every size)"""
    random = n in BIG_RANDOM
    c = honest(n, prove=n <= ref.SIZES_WAVE[0])
    worst = 0.0
    if n in ref.SIZES_FINALIZE:
        worst = c.rdots(n, steps=(3,), random=False, split=16)
    elif n == ref.SIZE_GRID_STRIDE:
        worst = max(c.rdots(n, steps=(5,), random=False, rpl=2), c.axpy_norm(n, steps=(5,), random=False, rpl=2))
    else:
        worst = max(c.rdots(n, steps=(1, 2, 5), random=random), c.callable_step(n, steps=(1, 2, 5), random=random))
        if n not in ref.SIZES_NT2:
            worst = max(worst, c.axpy_norm(n, steps=(2, 5), random=random))
        if n in ref.SIZES_WAVE:
            worst = max(worst, c.ritz(n, steps=(5,), random=random))
    if n == ref.SIZES_WAVE[0]:
        c.partial_exact(n)
        worst = max(worst, c.partial_random(n), c.store(n), c.callable_alpha(n), c.callable_step(n + 1, steps=(2, 3)))
        c.twice(n)
    assert worst <= 1.0
    print("n = %d: %d cases, worst error / bound %.3f" % (n, c.cases, worst))


@pytest.mark.parametrize("n,rpl", [(129, 2), (300, 2)])
def test_an_honest_fp64_evaluation_passes_the_forced_geometries(n, rpl):
    c = honest(n)
    assert c.rdots(n, rpl=rpl) <= 1.0 and c.partial_random(n, rpl=rpl) <= 1.0
    c.partial_exact(n, rpl=rpl)


@pytest.mark.parametrize("n,i", [(300, i) for i in ref.STEPS_LDS] + [(129, i) for i in ref.STEPS_LDS_SPLIT])
def test_the_exact_class_has_headroom_at_the_long_recurrences(n, i):
    c = Checks(HostImpl(Reference(np.float64, order=i)), prove=(i == 2047), **QUIET)
    c.rdots(n, steps=(i,), random=False, kmax=ref.KMAX)
    c.axpy_norm(n, steps=(i,), random=False, kmax=ref.KMAX)


def test_the_largest_exact_sum_stays_far_below_2_to_the_53():
    """(runs after the cases above in file order; on its own it measures the two cases it runs itself)"""
    c = honest(5, prove=False)
    c.axpy_norm(300, steps=(7999,), random=False)
    c.callable_step((1 << 20) + 2, steps=(5,), random=False)
    print("largest sum of |terms| met in an exact-class case: 2^%.1f units" % np.log2(ref.assert_headroom.largest))
    assert ref.assert_headroom.largest < 2.0 ** 50


def test_the_launch_geometry_the_cases_rely_on():
    g = ref.geom
    assert [g(n)["split_w"] for n in ref.SIZES_SPLIT16] == [16] * 6 and g(ref.SIZE_SPLIT8)["split_w"] == 8
    assert g(32768)["split_w"] == 16 and g(32769)["split_w"] == 8
    for n, tiles in zip(ref.SIZES_NT2, (642, 643)):
        assert (g(n)["split_w"], g(n)["dots_nt"], g(n)["ntiles"]) == (8, 2, tiles) and ref.rdots_partials(n, 5) == 321 + (tiles == 643)
    assert 82049 - 641 * 128 == 1 and 82177 - 642 * 128 == 1             # one row in the second / in the first sub-tile of the last block
    assert [(g(n)["split_w"], g(n)["rpl"]) for n in ref.SIZES_WAVE] == [(0, 2), (0, 4), (0, 8), (0, 16)]
    assert g(131072)["split_w"] == 8 and g(131073)["split_w"] == 0
    for n, nw in zip(ref.SIZES_RPL2_SMALL, (2, 3)):
        assert (g(n, rpl=2)["split_w"], g(n, rpl=2)["nw"]) == (0, nw) and ref.rdots_partials(n, 5, rpl=2) == 1
    gs = g(ref.SIZE_GRID_STRIDE, rpl=2)
    assert (gs["ntiles"], gs["nw"]) == (8194, 8192) and ref.SIZE_GRID_STRIDE - 8193 * 128 == 1
    for n, count, trips in zip(ref.SIZES_FINALIZE, (801, 1801), ((1, 0), (2, 0))):
        assert g(n, split=16)["dots_nt"] == 1 and ref.rdots_partials(n, 3, split=16) == count and ref.finalize_trips(count) == trips
    assert ref.finalize_trips(768) == (0, 3) and ref.finalize_trips(769) == (1, 0)
    assert [ref.rdots_waves_per_block(i) for i in ref.STEPS_LDS] == [4, 2, 2, 1, 1]
    assert [ref.rdots_lds_bytes(300, i, rpl=2) for i in (2047, 4095, 7999)] == [65536, 65536, 64000]
    assert [ref.rdots_partials(300, i, rpl=2) for i in ref.STEPS_LDS] == [1, 2, 2, 3, 3]
    # alpha partials of dsea_lanczos_callable_alpha: one block per 2048 rows
    assert (129 + 2047) // 2048 == 1 and (131203 + 2047) // 2048 == 65
    rows = ref.support_rows(82177)
    assert {0, 82176, 82175, 127, 128, 82175 // 256 * 256} <= set(rows) and len(rows) <= 16


# ---- wrong kernels ----------------------------------------------------------------------------------------------------------
WAVE = ref.SIZES_WAVE[0]
RDOTS = lambda c, n: c.rdots(n, steps=(1, 2, 3, 5) if n > 4097 else ref.STEPS_REV)                      # noqa: E731
AXPY = lambda c, n: c.axpy_norm(n, steps=(2, 5))                                                        # noqa: E731
STORE = lambda c, n: c.store(n)                                                                         # noqa: E731
STEP = lambda c, n: c.callable_step(n, steps=(1, 2, 5))                                                 # noqa: E731
PARTIAL = lambda c, n: c.partial_exact(n)                                                               # noqa: E731
STRICT = lambda c, n: c.partial_strict(n)                                                               # noqa: E731
# name -> (the check that must fail, the smallest n at which the wrong kernel differs from the right one)
REJECTED_BY = {
    "the q(i-2) term is dropped at i >= 2": (RDOTS, 1),
    "the q(i-2) term is applied at i = 1": (RDOTS, 1),
    "a and b are exchanged": (RDOTS, 1),
    "the three-term update is contracted into FMAs": (RDOTS, 3),
    "the dots are taken against u": (RDOTS, 1),
    "the remainder vectors j >= 4 floor(i / 4) are dropped": (RDOTS, 1),
    "c_j is stored at i - 1 - j on odd i": (RDOTS, 1),
    "c_i is taken after the correction": (RDOTS, 1),
    "the last row of an odd n is dropped from a sum": (RDOTS, 1),
    "the last row of an odd n is dropped from a store": (RDOTS, 1),
    "one partial is dropped": (RDOTS, 1),
    "the second grid-stride trip overwrites": (lambda c, n: c.rdots(n, steps=(5,), random=False, rpl=2), ref.SIZE_GRID_STRIDE),
    "the correction runs over i - 1 vectors": (AXPY, 1),
    "the correction uses c_{j+1}": (AXPY, 1),
    "nrm2 is taken before the subtraction": (AXPY, 1),
    "beta without the square root": (STORE, 1),
    "Q[i] is written to row i - 1": (STORE, 1),
    "alphas[i-1] is not written": (STEP, 1),
    "a skipped step corrects anyway": (PARTIAL, 1),
    "a skipped step's nrm2_out is not rr": (PARTIAL, 1),
    "forced is ignored": (PARTIAL, 1),
    "the trigger is decided with <": (STRICT, 1),
    "the omega row is not reset after a selected step": (PARTIAL, 1),
    "anorm is not a running maximum": (PARTIAL, 1),
    "the counter is incremented on skipped steps": (PARTIAL, 1),
    "no restart at i = 1": (PARTIAL, 1),
}


def test_every_wrong_kernel_has_its_check():
    assert sorted(REJECTED_BY) == sorted(ref.MUTANTS) and len(ref.MUTANTS) == 26


@pytest.mark.parametrize("name", sorted(ref.MUTANTS))
@pytest.mark.parametrize("size", ["smallest", "wave-owned"])
def test_a_wrong_kernel_fails_a_verdict(name, size):
    run, smallest = REJECTED_BY[name]
    n = smallest if size == "smallest" else max(WAVE, smallest) + ("odd n" in name)
    c = Checks(HostImpl(ref.MUTANTS[name](np.float64, order=5)), prove=False, **QUIET)
    with pytest.raises(AssertionError), np.errstate(all="ignore"):
        run(c, n)
    if size == "smallest" and 1 < smallest < WAVE:          # ... and it IS the smallest of the split-16 sizes: the one below passes
        below = ref.SIZES_SPLIT16[ref.SIZES_SPLIT16.index(smallest) - 1]
        run(Checks(HostImpl(ref.MUTANTS[name](np.float64, order=5)), prove=False, **QUIET), below)


class RandomOnly(Checks):
    """the same checks with the exact class's verdict switched off"""

    def exact(self, tag, got, want):
        pass


# what the random-class bounds reject on their own (the others need the exact class: they change a decision, a counter, or a
# value that the random class can only bound -- docs/design/29-lanczos-stage-tests.md lists the reasons)
RANDOM_ALONE = {
    "the q(i-2) term is dropped at i >= 2": RDOTS, "the q(i-2) term is applied at i = 1": RDOTS, "a and b are exchanged": RDOTS, "the three-term update is contracted into FMAs": RDOTS,
    "the dots are taken against u": RDOTS, "the remainder vectors j >= 4 floor(i / 4) are dropped": RDOTS,
    "c_j is stored at i - 1 - j on odd i": RDOTS, "c_i is taken after the correction": RDOTS,
    "the last row of an odd n is dropped from a sum": RDOTS, "the last row of an odd n is dropped from a store": RDOTS,
    "one partial is dropped": RDOTS, "the correction runs over i - 1 vectors": AXPY, "the correction uses c_{j+1}": AXPY,
    "nrm2 is taken before the subtraction": AXPY, "beta without the square root": STORE, "Q[i] is written to row i - 1": STORE,
    "alphas[i-1] is not written": STEP, "a skipped step corrects anyway": lambda c, n: c.partial_random(n),
    "a skipped step's nrm2_out is not rr": lambda c, n: c.partial_random(n),
    "the counter is incremented on skipped steps": lambda c, n: c.partial_random(n),
}


@pytest.mark.parametrize("name", sorted(RANDOM_ALONE))
def test_a_wrong_kernel_fails_the_random_class_alone(name):
    c = RandomOnly(HostImpl(ref.MUTANTS[name](np.float64, order=6)), prove=False, **QUIET)
    with pytest.raises(AssertionError), np.errstate(all="ignore"):
        RANDOM_ALONE[name](c, 129)


def test_a_wrong_correction_in_the_fused_step_fails_the_random_class_alone():
    """the gap the random class closes: with a genuine Lanczos u the coefficients are rounding residue and these pass.  (What
    the fused step hides even so, because Q Q^T removes it again -- a dropped q(i-2) term, a dropped last vector whose coefficient
    alpha has already cancelled -- is left to the exact class, whose Q is not orthonormal.)"""
    for name in ("the correction uses c_{j+1}", "the dots are taken against u", "c_j is stored at i - 1 - j on odd i",
                 "nrm2 is taken before the subtraction"):
        c = RandomOnly(HostImpl(ref.MUTANTS[name](np.float64, order=7)), prove=False, **QUIET)
        with pytest.raises(AssertionError), np.errstate(all="ignore"):
            c.callable_step(129, steps=(), random=True)
