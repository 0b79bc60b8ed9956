"""tests/krylov_reference.py judged on its own (no GPU): the longdouble step is an Arnoldi step, the cycle is GMRES, the exact
class is exact under any summation order, and an honest fp64 evaluation of the same algorithm in reversed and pairwise order
stays inside every operation-counted bound.  Every builder's margin assertion runs here for every case of
tests/test_gpu_krylov_stages.py."""
import numpy as np
import pytest

import krylov_reference as kr
import matvec_reference as mref
from dominantsparseeigenad_amd.synthetic import normal_vector

LD = np.longdouble
CPU_N = tuple(n for n in kr.STEP_N if n <= 131202)


dense_noise = kr.dense_noise


def test_longdouble_step_is_an_arnoldi_step():
    n, m = 300, 6
    A = dense_noise(n)
    apply = mref.dense_apply(A)
    V = np.zeros((m + 1, n), dtype=LD)
    v0 = np.asarray(normal_vector(n, 1), dtype=LD)
    V[0] = v0 / np.sqrt(np.sum(v0 * v0))
    H = np.zeros((m + 1, m), dtype=LD)
    shift = LD(kr.SHIFT_RANDOM)
    for j in range(m):
        st = kr.arnoldi_step(V[: j + 1], apply(V[j], LD)[0], shift, LD)
        assert not st.dead and st.margin_dead > 1e10
        H[: j + 2, j] = st.h
        V[j + 1] = st.v_next
    G = V @ V.T
    assert float(np.abs(G - np.eye(m + 1)).max()) < 1e-18 * n
    AV = np.stack([apply(V[j], LD)[0] - shift * V[j] for j in range(m)])
    res = AV - H.T @ V
    print("longdouble Arnoldi: |V V^T - I| = %.2e, relation residual %.2e" % (float(np.abs(G - np.eye(m + 1)).max()),
                                                                              float(np.abs(res).max())))
    assert float(np.abs(res).max()) < 1e-18 * n


@pytest.mark.parametrize("n,m", [(1, 1), (2, 1), (3, 1), (3, 3), (300, 4), (300, 8), (1001, 8)])
def test_gmres_cycle_is_the_least_squares_minimiser(n, m):
    A = dense_noise(n)
    apply = mref.dense_apply(A)
    b = normal_vector(n, 5)
    for shift, x0 in ((0.0, None), (kr.SHIFT_RANDOM, None), (kr.SHIFT_RANDOM, normal_vector(n, 6))):
        x, state, ex = kr.gmres_cycle(apply, shift, b, x0, m, 0.0)
        k = int(state[2])
        assert k == m or state[4] == 1.0
        true = np.asarray(b, dtype=LD) - (apply(x, LD)[0] - LD(shift) * x)
        tn = float(np.sqrt(np.sum(true * true)))
        assert abs(tn - float(state[0])) <= 1e-17 * n * float(state[3]), (tn, state[0])
        xl, rl, _, _ = kr.lstsq_over(apply, shift, b, x0, ex["V"][:k])
        assert float(np.abs(xl - x).max()) <= 1e-16 * float(np.abs(x).max() + 1), float(np.abs(xl - x).max())
        assert abs(float(rl) - tn) <= 1e-17 * n * float(state[3])


def test_gmres_cycle_states():
    n = 300
    apply = mref.dense_apply(dense_noise(n))
    b = normal_vector(n, 5)
    nb = float(np.sqrt(np.sum(b * b)))
    x, st, _ = kr.gmres_cycle(apply, 0.0, b, None, 8, 2 * nb)
    assert st[1] == st[4] == 1.0 and st[2] == 0 and not x.any()
    target, apply_mid = kr.midcycle_target(n, b)
    _, st, _ = kr.gmres_cycle(apply_mid, 0.0, b, None, 8, target)
    assert st[2] == 3 and st[1] == st[4] == 1.0
    # singular: diagonal A, b = e_k, shift = A_kk
    d = np.arange(1, n + 1) / 8.0
    e = np.zeros(n)
    e[7] = 1.0
    x, st, _ = kr.gmres_cycle(mref.dense_apply(np.diag(d)), d[7], e, None, 4, 1e-12)
    assert st[6] == 1.0 and st[4] == 1.0 and st[1] == 0.0 and st[2] == 0.0 and not x.any()
    # exhaustion: three eigenvalues
    A3 = kr.three_eigenvalue_matrix(300)
    x, st, _ = kr.gmres_cycle(mref.dense_apply(A3), 0.0, b, None, 8, 0.0)
    assert st[2] == 3 and st[4] == 1.0 and st[1] == 0.0
    r = b - A3 @ np.asarray(x, dtype=np.float64)
    assert float(np.abs(r).max()) < 1e-12 * nb


def all_exact_cases():
    for n in kr.STEP_N + (kr.N_CAPPED,):
        for j in kr.step_js(n):
            for kind in kr.exact_kinds(n, j):
                yield n, j, kind


def test_exact_class_is_exact_in_any_order():
    """fp64 under forward, reversed and pairwise summation = longdouble, bit for bit, for every exact case up to n = 131202
    (beyond, numpy's own order against longdouble)"""
    count = 0
    for n, j, kind in all_exact_cases():
        V, u, shift, p = kr.exact_step(n, j, kind)
        ref = kr.arnoldi_step(V, u, shift, LD)
        assert ref.second == (kind in ("second", "overlap", "dead")), (n, j, kind)      # (dead: w1 = 0 exactly fails the DGKS test)
        assert ref.dead == (kind in ("zero", "dead")), (n, j, kind)
        if not ref.dead:
            assert float(ref.beta) == 2.0 ** p, (n, j, kind, float(ref.beta))
        if kind == "overlap":
            assert ref.c2[0] != 0 and ref.h[0] == 0 and ref.h[1] == 0
        orders = kr.ORDERS.values() if n <= 32898 and j <= 17 else (None,)
        for summ in orders:
            s = kr.arnoldi_step(V, u, shift, np.float64, summ)
            assert s.second == ref.second and s.dead == ref.dead
            assert np.array_equal(np.asarray(ref.h, dtype=np.float64), s.h) and np.array_equal(s.h.astype(LD), ref.h)
            if not ref.dead:
                assert np.array_equal(s.v_next.astype(LD), ref.v_next)
        count += 1
    print("%d exact cases" % count)
    assert count > 100


def all_random_cases():
    for n in kr.STEP_N:
        for j in kr.step_js(n):
            for kind in kr.random_kinds(n, j):
                for with_shift in (False, True):
                    yield n, j, kind, with_shift
    for kind in kr.random_kinds(129, kr.J_LONG):
        yield 129, kr.J_LONG, kind, True


@pytest.mark.parametrize("n", kr.STEP_N)
def test_random_builders_keep_their_margins_and_fp64_stays_in_bounds(n):
    """every random case of the GPU test at this n builds (the builder asserts both margins); up to n = 131202 the fp64 twin
    under reversed and pairwise summation is judged by the bounds, worst ratio printed per family"""
    worst = {}
    cases = [c for c in all_random_cases() if c[0] == n]
    for _, j, kind, with_shift in cases:
        V, u, shift, ref = kr.random_step(n, j, kind, with_shift)
        if n > 131202:
            continue
        for name in ("reversed", "pairwise"):
            s = kr.arnoldi_step(V, u, shift, np.float64, kr.ORDERS[name])
            assert s.second == ref.second and s.dead == ref.dead, (n, j, kind, name)
            for fam, r in kr.judge_step(V, u, shift, ref, s.h, s.v_next).items():
                key = "%s/%s" % (kind, fam)
                worst[key] = max(worst.get(key, 0.0), r)
    for key in sorted(worst):
        print("n = %d  %-14s worst error / bound = %.4f" % (n, key, worst[key]))
        assert worst[key] <= 1.0, (n, key, worst[key])


def test_fp64_cycle_stays_in_the_gmres_bounds():
    for n, m in ((3, 1), (300, 4), (300, 8), (1001, 8)):
        A = dense_noise(n)
        apply = mref.dense_apply(A)
        b = normal_vector(n, 5)
        nb = float(np.sqrt(np.sum(b * b)))
        sv = np.linalg.svd(A - kr.SHIFT_RANDOM * np.eye(n), compute_uv=False)
        for name in ("reversed", "pairwise"):
            x, st, ex = kr.gmres_cycle(apply, kr.SHIFT_RANDOM, b, None, m, 0.0, np.float64, kr.ORDERS[name])
            k = int(st[2])
            xl, rl, _, Rm = kr.lstsq_over(apply, kr.SHIFT_RANDOM, b, None, ex["V"][:k])
            bx, br = kr.gmres_bounds(n, n, k, float(sv[0]), nb, kr.subspace_cond(sv[0], Rm))
            ex_ = float(np.sqrt(np.sum((np.asarray(x, dtype=LD) - xl) ** 2)))
            true = np.asarray(b, dtype=LD) - (apply(x, LD)[0] - LD(kr.SHIFT_RANDOM) * np.asarray(x, dtype=LD))
            er = abs(float(np.sqrt(np.sum(true * true))) - float(st[0]))
            print("gmres n = %d m = %d %s: |x - x_ls| / bound = %.4f   |estimate - true| / bound = %.4f"
                  % (n, m, name, ex_ / bx, er / br))
            assert ex_ <= bx and er <= br
