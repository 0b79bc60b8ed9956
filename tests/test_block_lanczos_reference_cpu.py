"""tests/block_lanczos_reference.py proved on the CPU (no GPU) before it judges a kernel (tests/test_gpu_block_lanczos_stages.py):
the stage reference composed in longdouble IS the recurrence of the numpy twins (sector_block_reference.block_lanczos,
hubbard_block_reference.block_lanczos) and its returned blocks satisfy the three-term relation against the dense matrix; the
exact class is exact at every size of the GPU test; an honest fp64 evaluation with its sums in a random order passes every
verdict; the teeth of the random class and the k = n + 2 agreement hold for the seeds used; and each of the wrong kernels of
block_lanczos_reference.MUTANTS fails a verdict -- through the same Checks and judges the GPU test drives the library with.

Sizes from 92378 rows on run the exact class only here (the GPU test runs their random cases).  L10-5-5-default and
L20-10-default differ from their -walk twins in the grid alone, which an evaluation on the host does not have: they appear here
where the grid matters (the launch geometry, the wrong kernels of the reduction), and 63504 rows run at R = 1 and R = 8."""
import numpy as np
import pytest

import block_lanczos_reference as ref
import hubbard_block_reference
import hubbard_reference
import sector_block_reference
import sector_reference
from block_lanczos_reference import Checks, HostImpl, Reference

LD = np.longdouble
QUIET = {"log": lambda *a: None}
CASES = ref.cases()
SMALL = [name for name in ref.ALL if name not in ref.THIN and name != "L10-5-5-default"]
HOST_WIDTHS = lambda name: (1, 8) if CASES[name].n > 1 << 15 else ref.widths(name, False)      # noqa: E731


def honest(seed=1000, prove=True):
    return Checks(HostImpl(Reference(np.float64, order=seed)), prove=prove, **QUIET)


# ---- composition ------------------------------------------------------------------------------------------------------------
def twin_of(case, p, Phi, k, dtype):
    if case.kind == "sector":
        return sector_block_reference.block_lanczos(case.L, case.fill, case.bonds, p, Phi, k, dtype), \
            sector_block_reference.coupling_bound(case.L, case.bonds, p), sector_reference.dense(case.L, case.fill, case.bonds, p)
    return hubbard_block_reference.block_lanczos(case.L, case.fill[0], case.fill[1], case.bonds, p, Phi, k, dtype), \
        hubbard_block_reference.coupling_bound(case.L, case.bonds, p), \
        hubbard_reference.dense(case.L, case.fill[0], case.fill[1], case.bonds, p)


@pytest.mark.parametrize("name", ["L9-4-cap", "L11-5", "L6-3-3-loops", "L3-1-2"])
def test_the_composed_stages_are_the_recurrence_of_the_twins(name):
    """coefficients to 1e-12 B against the twin's longdouble run; the returned blocks Q_k, Q_{k-1} (and Q_{k-2} from the run one
    step shorter) satisfy H Q_{k-1} = beta_{k-1} Q_{k-2} + alpha_{k-1} Q_{k-1} + beta_k Q_k against the dense matrix to 1e-11 B"""
    case = CASES[name]
    k = min(12, case.n - 1)
    p, Phi = ref.random_couplings(case), ref.random_block(case, 8)
    (norm2, alphas, betas, steps), B, H = twin_of(case, p, Phi, k, LD)
    run, shorter = Reference(LD).run(case, p, Phi, k), Reference(LD).run(case, p, Phi, k - 1)
    assert run.steps.tolist() == list(steps) == [k] * 8
    assert float(np.max(np.abs(run.norm2 / norm2 - 1.0))) <= 1e-15
    assert float(np.max(np.abs(run.alphas - alphas))) <= 1e-12 * B and float(np.max(np.abs(run.betas - betas))) <= 1e-12 * B
    latest, previous = ref.Run.latest(run), ref.Run.previous(run)
    assert ref.same(np.asarray(previous, dtype=np.float64), np.asarray(ref.Run.latest(shorter), dtype=np.float64))
    residual = H.astype(LD) @ previous - run.betas[k - 2][None, :] * ref.Run.previous(shorter) \
        - run.alphas[k - 1][None, :] * previous - run.betas[k - 1][None, :] * latest
    assert float(np.max(np.abs(residual))) <= 1e-11 * B
    assert float(np.max(np.abs(np.sum(latest * latest, axis=0) - 1.0))) <= 1e-12


# ---- an honest evaluation passes; the exact class has headroom --------------------------------------------------------------
@pytest.mark.parametrize("name,R", [(name, R) for name in SMALL for R in HOST_WIDTHS(name)])
def test_an_honest_fp64_evaluation_passes_every_verdict(name, R):
    case = CASES[name]
    c = honest(1000 + R)
    c.exact_class(case, R)
    if case.n > 1 + 1:
        worst = c.random(case, R)
        assert worst <= 1.0
    c.twice(case, R)
    print("%s R = %d: %d verdicts, worst ratios %s" % (name, R, c.cases, {k: round(v[0], 3) for k, v in c.worst.items()}))


@pytest.mark.parametrize("R", [1, 8])
@pytest.mark.parametrize("name", [name for name in ref.THIN if name != "L20-10-default"])
def test_the_exact_class_at_the_large_sizes(name, R):
    """92378 rows and more: the exact class (the k = 1 run and the break decisions at k = 4), an honest evaluation"""
    case = CASES[name]
    c = honest(2000 + R, prove=False)
    c.first_step(case, R)
    c.breaks(case, R, ks=(4,))
    c.all_break(case, R)
    c.strict(case, R)


def test_the_largest_exact_sum_stays_far_below_2_to_the_53():
    """(runs after the cases above in file order; on its own it measures the case it runs itself)"""
    honest().first_step(CASES["L16-8"], 8)
    print("largest sum of |terms| met in an exact-class case: 2^%.1f units of 2^-16" % np.log2(ref.Headroom.largest_met))
    assert ref.Headroom.largest_met < 2.0 ** 45


def test_the_break_kinds_every_geometry_offers():
    """which column kinds exist where: the two-row sector has no state without a partner; at L2-1-1 the one bond moves both
    species of every state (four coupled states: no exact break but the zero column); every other case has all kinds"""
    missing = {name: ref.break_data(name).missing for name in ref.ALL}
    assert missing.pop("L2-1") == ["U", "PP", "L"] and missing.pop("L2-1-1") == ["U", "P", "PP", "L"]
    assert missing.pop("L3-1") == ["PP", "L"] and missing.pop("L3-1-2") == ["L"]
    assert all(v == [] for v in missing.values()), missing
    assert not Checks(HostImpl(Reference()), **QUIET).strict(CASES["L2-1-1"], 1)
    assert all(Checks(HostImpl(Reference()), **QUIET).strict(CASES[name], 1) for name in ("L2-1", "L3-1", "L3-1-2"))


@pytest.mark.parametrize("name", ["L2-1", "L3-1"])
def test_k_beyond_n_breaks_at_the_same_step_in_float64_and_longdouble(name):
    for R in ref.WIDTHS:
        agree = honest().beyond_n(CASES[name], R)
        assert agree.all(), (name, R)


@pytest.mark.parametrize("name", [n for n in ref.ALL if n not in ("L2-1", "L10-5-5-default", "L20-10-default")])
def test_the_teeth_of_the_random_class_hold_on_the_twin(name):
    """both subtracted terms are at least 2^-10 of max |H Q_i| in every column of every judged step (twice that on the twin, so
    that the device's slightly different iterates keep the margin); L2-1 has one judged step and is covered by its own run, the
    -default cases share couplings and start block with their -walk twins"""
    assert all(ref.RANDOM_SEEDS.get(a, 0) == ref.RANDOM_SEEDS.get(b, 0) for a, b in (("L10-5-5-default", "L10-5-5-walk"), ("L20-10-default", "L20-10-walk")))
    case = CASES[name]
    p, Phi = ref.random_couplings(case), ref.random_block(case, 8)
    kmax = min(4, case.n - 1)
    mirror = Reference(np.float64)
    runs = {k: mirror.run(case, p, Phi, k) for k in range(1, kmax + 1)}
    Qs = [ref.Run.previous(runs[1])] + [ref.Run.latest(runs[k]) for k in range(1, kmax + 1)]
    last, worst = runs[kmax], np.inf
    for i in range(kmax):
        t = ref.teeth(i, case.apply(p, Qs[i]), Qs[i - 1] if i else None, Qs[i], last.alphas[i], last.betas[i - 1] if i else None)
        worst = min(worst, float(t.min()))
    print("%s: smallest subtracted term / max |A| = 2^%.1f" % (name, np.log2(worst)))
    assert worst >= 2.0 * ref.TEETH


def test_the_launch_geometry_the_cases_rely_on():
    rows = {name: (CASES[name].n, CASES[name].ranges, CASES[name].nblk) for name in ref.ALL}
    assert rows["L2-1"] == (2, 1, 1) and rows["L3-1"] == (3, 1, 1) and rows["L2-1-1"] == (4, 1, 1) and rows["L3-1-2"] == (9, 1, 1)
    assert rows["L9-4-cap"] == (126, 1, 1) and CASES["L9-4-cap"].nb == 128
    assert rows["L11-5"] == (462, 2, 2) and rows["L6-3-3-loops"] == (400, 2, 2)
    assert rows["L16-8"] == (12870, 51, 51) and rows["L8-4-4-complete"] == (4900, 20, 20)
    assert rows["L19-9"] == (92378, 361, 361) and rows["L20-10-default"] == (184756, 722, 722)
    assert rows["L20-10-walk"] == (184756, 722, 64) and CASES["L20-10-walk"].bonds == CASES["L20-10-default"].bonds
    assert rows["L10-5-5-walk"] == (63504, 249, 64) and rows["L10-5-5-default"] == (63504, 249, 249)
    assert rows["L21-8"] == (203490, 795, 795)
    assert rows["L40-2"] == (780, 4, 4) and rows["L40-2-1"] == (31200, 122, 122)
    assert ref.block_blocks(1 << 21) == 4096 and ref.block_blocks(1 << 21, 6) == 64 and ref.block_blocks(1, 6) == 1
    # sum_partials_block: (loop trips of thread 0, threads with as many, threads with a tail read)
    assert ref.partial_trips(1) == (0, 256, 1) and ref.partial_trips(51) == (0, 256, 51) and ref.partial_trips(249) == (0, 256, 249)
    assert ref.partial_trips(256) == (0, 256, 256) and ref.partial_trips(257) == (1, 1, 255)
    assert ref.partial_trips(361) == (1, 105, 151)          # the two-accumulator trip for threads 0 .. 104, nothing read past 360
    assert ref.partial_trips(512) == (1, 256, 0) and ref.partial_trips(513) == (1, 256, 1)
    assert ref.partial_trips(722) == (1, 256, 210)          # every thread one trip, then partials 512 .. 721 by the tail read
    assert ref.partial_trips(768) == (1, 256, 256) and ref.partial_trips(769) == (2, 1, 255)
    assert ref.partial_trips(795) == (2, 27, 229)           # a second loop trip for threads 0 .. 26
    assert ref.partial_reads(722, 0) == ([0], [256], 512) and ref.partial_reads(795, 26) == ([26, 538], [282, 794], None)
    # state words above bit 32
    assert CASES["L40-2"].L == 40 and CASES["L40-2-1"].L == 40
    for name in ("L19-9", "L20-10-default", "L20-10-walk", "L21-8", "L10-5-5-walk"):
        case = CASES[name]
        rows_ = set(ref.support_rows(case).tolist())
        assert {0, case.n - 1, 255, 256} <= rows_ and len(rows_) >= 16
    assert {64 * 256 - 1, 64 * 256} <= set(ref.support_rows(CASES["L20-10-walk"]).tolist())
    assert {256 * 256 - 1, 256 * 256, 512 * 256 - 1, 512 * 256} <= set(ref.support_rows(CASES["L20-10-default"]).tolist())
    assert [CASES[name].scratch_doubles(8) for name in ("L2-1", "L20-10-walk")] == [64 + 16, 64 + 16 * 722]


# ---- wrong kernels ----------------------------------------------------------------------------------------------------------
FIRST = lambda c, case, R: c.first_step(case, R)                                                        # noqa: E731
BREAKS = lambda c, case, R: c.breaks(case, R)                                                           # noqa: E731
STRICT = lambda c, case, R: c.strict(case, R)                                                           # noqa: E731
RANDOM = lambda c, case, R: c.random(case, R)                                                           # noqa: E731
# name -> (the check that must fail, the smallest case and width at which the wrong kernel differs, a multi-block case)
REJECTED_BY = {
    "the beta term is dropped": (BREAKS, "L2-1", 1, "L11-5"),
    "the beta term is applied on the first step": (FIRST, "L2-1", 1, "L11-5"),
    "beta_i is taken from the other state copy": (BREAKS, "L2-1", 1, "L11-5"),
    "the alpha correction is taken from Q_{i-1}": (FIRST, "L2-1", 1, "L11-5"),
    "product and difference are contracted into an FMA": (RANDOM, "L2-1", 1, "L11-5"),
    "norm2 reports the root": (FIRST, "L2-1", 1, "L11-5"),
    "column j uses the alpha and beta of column j ^ 1": (FIRST, "L2-1", 2, "L11-5"),
    "the last block's partial is dropped": (FIRST, "L2-1", 1, "L11-5"),
    "the second accumulator of the partial sum is dropped": (FIRST, "L19-9", 1, "L19-9"),
    "the partials from 512 on are dropped": (FIRST, "L20-10-default", 1, "L20-10-default"),
    "acc is reset on every row range of the walk": (FIRST, "L10-5-5-walk", 1, "L20-10-walk"),
    "a thread past the last row adds row n - 1 again": (FIRST, "L2-1", 1, "L11-5"),
    "the breaking beta is stored non-zero": (STRICT, "L2-1", 1, "L11-5"),
    "a breaking column is left alive in the other array": (BREAKS, "L2-1", 1, "L11-5"),
    "a dead column is divided by its zero beta": (BREAKS, "L2-1", 1, "L11-5"),
    "one break zeroes the whole block": (BREAKS, "L2-1", 2, "L11-5"),
    "the scale lacks the current alpha": (STRICT, "L2-1", 1, "L11-5"),
    "the scale lacks the betas": (STRICT, "L2-1", 1, "L11-5"),
    ">= in place of >": (STRICT, "L2-1", 1, "L11-5"),
    "steps is not set to k at the start": (FIRST, "L2-1", 1, "L11-5"),
    "steps of a dead column is overwritten later": (BREAKS, "L2-1", 1, "L11-5"),
}


def test_every_wrong_kernel_has_its_check():
    assert sorted(REJECTED_BY) == sorted(ref.MUTANTS) and len(ref.MUTANTS) == 21


@pytest.mark.parametrize("name", sorted(ref.MUTANTS))
@pytest.mark.parametrize("size", ["smallest", "multi-block"])
def test_a_wrong_kernel_fails_a_verdict(name, size):
    run, smallest, R, multi = REJECTED_BY[name]
    case = CASES[smallest if size == "smallest" else multi]
    c = Checks(HostImpl(ref.MUTANTS[name](np.float64, order=5)), prove=False, **QUIET)
    with pytest.raises(AssertionError), np.errstate(all="ignore"):
        run(c, case, max(R, 1) if size == "smallest" else max(R, 2))


def test_a_smaller_size_does_not_see_the_reduction_mutants():
    """... and the sizes named above ARE the smallest: 249 partials have no second accumulator, 361 none past 512, an uncapped
    grid no second row range, one column no neighbour"""
    for name, below, R in (("the second accumulator of the partial sum is dropped", "L10-5-5-default", 1),
                           ("the partials from 512 on are dropped", "L19-9", 1),
                           ("acc is reset on every row range of the walk", "L10-5-5-default", 1),
                           ("column j uses the alpha and beta of column j ^ 1", "L2-1", 1)):
        Checks(HostImpl(ref.MUTANTS[name](np.float64, order=5)), prove=False, **QUIET).first_step(CASES[below], R)
    Checks(HostImpl(ref.MUTANTS["one break zeroes the whole block"](np.float64, order=5)), prove=False, **QUIET).breaks(CASES["L2-1"], 1)


class RandomOnly(Checks):
    """the same checks with the exact class's verdict switched off"""

    def exact(self, tag, got, want, cols=None):
        pass


# what the random class rejects on its own; the others change a decision, `steps`, or a column that the random class never
# sees die (docs/design/36-block-lanczos-stage-tests.md gives the reasons)
RANDOM_ALONE = ["the beta term is dropped", "the beta term is applied on the first step", "beta_i is taken from the other state copy",
                "the alpha correction is taken from Q_{i-1}", "product and difference are contracted into an FMA",
                "norm2 reports the root", "column j uses the alpha and beta of column j ^ 1", "the last block's partial is dropped",
                "a thread past the last row adds row n - 1 again", "steps is not set to k at the start"]


@pytest.mark.parametrize("name", RANDOM_ALONE)
def test_a_wrong_kernel_fails_the_random_class_alone(name):
    c = RandomOnly(HostImpl(ref.MUTANTS[name](np.float64, order=6)), prove=False, **QUIET)
    with pytest.raises(AssertionError), np.errstate(all="ignore"):
        c.random(CASES["L11-5"], 2)


def test_the_walk_mutant_fails_the_random_class_alone():
    c = RandomOnly(HostImpl(ref.MUTANTS["acc is reset on every row range of the walk"](np.float64, order=6)), prove=False, **QUIET)
    with pytest.raises(AssertionError), np.errstate(all="ignore"):
        c.random(CASES["L10-5-5-walk"], 1, kmax=1)


def test_the_twins_count_beta_0_as_the_kernel_does():
    """the scale of the break rule holds beta_0 = |start column|: at the boundary where only beta_0 decides (phi = 2 e_r,
    alpha_0 = 1, beta_1 = 2e-13 or one ulp more) the whole-run twins break where the stage reference does"""
    for name in ("L3-1", "L3-1-2"):
        case = CASES[name]
        for above in (False, True):
            p, phi, c, _ = ref.strict_inputs(case, "beta", above)
            (_, _, betas, steps), _, _ = twin_of(case, p, phi[:, None], 2, np.float64)
            want = Reference(np.float64).run(case, p, phi[:, None], 2)
            assert steps.tolist() == want.steps.tolist() == [2 if above else 1] and betas[0, 0] == want.betas[0, 0] == (c if above else 0.0)
