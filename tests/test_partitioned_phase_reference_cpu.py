"""The references of tests/test_gpu_partitioned_phases.py proved without a GPU (tests/partitioned_reference.py): the lockstep
composer -- P virtual ranks in one process, host-summed "all-reduce", torch-copy "exchange" -- runs on the torch-CPU test double
(tests/cpu_backend.CpuBackend) and must reproduce oracle.lanczos_tridiag / oracle.cg_solve on the FULL operator at the limits
the GPU file asserts; the plain phase expressions must agree with the double phase by phase.  No library call."""
import pytest
import torch

import partitioned_reference as pr
from cpu_backend import CpuBackend
from partitioned_reference import F64, SENTINEL, padded_basis, ulp_distance, vec


@pytest.mark.parametrize("kind,size,part", pr.lockstep_cases())
def test_lockstep_on_the_test_double_matches_the_oracle(kind, size, part):
    run = pr.make_lockstep(kind, size, part, CpuBackend)
    pr.check_lockstep_lanczos(run, kind, size)
    pr.check_lockstep_cg(run, kind, size)


@pytest.mark.parametrize("L,P", [(5, 4), (7, 8), (10, 4)])
def test_lockstep_exchange_forms_give_the_same_remote_part(L, P):
    """pairwise and transposed exchange of the composer deliver the same sum of partner slabs (to the order of the additions)"""
    x = vec(1 << L, 41)
    sums = {}
    for form in ("pairwise", "transposed"):
        run = pr.LockstepTFIM(L, P, CpuBackend, form=form)
        recv = run.exchange([run.slab(x, r) for r in range(P)])
        sums[form] = torch.cat([torch.stack(list(bufs)).sum(0) for bufs in recv])
    ref = sum(x[torch.arange(1 << L) ^ (1 << b)] for b in range(L - (P.bit_length() - 1), L))
    for form, got in sums.items():
        assert float((got - ref).abs().max()) <= 1e-14 * float(x.abs().max()) * P, form


def test_ulp_distance():
    a = torch.tensor([1.0, -1.0, 0.0, 1e-300], dtype=F64)
    assert ulp_distance(a, a.clone()) == 0
    assert ulp_distance(a, torch.nextafter(a, torch.full_like(a, 9.0))) == 1
    assert ulp_distance(torch.tensor([0.0], dtype=F64), torch.tensor([-0.0], dtype=F64)) == 0
    assert ulp_distance(torch.tensor([1.0], dtype=F64), torch.tensor([1.0 + 2.0 ** -50], dtype=F64)) == 4


@pytest.mark.parametrize("n", [3, 129, 1000])
def test_reference_expressions_agree_with_the_test_double(n):
    """every phase: the header's expression (partitioned_reference.ref_*) against CpuBackend on the same inputs -- bit for bit
    where both evaluate the same operations in the same order, 1e-13 x norms for the reductions"""
    be = CpuBackend(n)
    Q, ldq = padded_basis(6, n, 100 + n)
    u = vec(n, 200 + n)
    a, b = torch.tensor([0.7], dtype=F64), torch.tensor([-1.3], dtype=F64)
    for i, beta in ((1, None), (1, b), (2, b), (5, b), (5, None)):
        r, rc = torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
        be.form_r(Q, ldq, n, i, u, a, beta, r, rc)
        want = pr.ref_form_r(Q, n, i, u, 0.7, None if beta is None else -1.3)
        assert torch.equal(r, want) and torch.equal(rc, want)
        c = torch.zeros(i + 1, dtype=F64)
        be.plz_dots(Q, ldq, n, i, u, a, beta, r, c)
        assert torch.equal(r, want)
        assert float((c[:i] - Q[:i, :n] @ want).abs().max()) <= 1e-13 * float(want.norm() * Q[:i, :n].norm(dim=1).max())
        assert abs(float(c[i]) - float(want @ want)) <= 1e-13 * float(want @ want)
    # correction: row 0 leaves r alone
    r0 = vec(n, 300 + n)
    c = vec(6, 301) * 0.1
    for row in (0, 1, 5):
        r, pair = r0.clone(), torch.tensor([0.0, SENTINEL], dtype=F64)
        be.plz_correct(Q, ldq, n, row, c, r, pair)
        want = pr.ref_correct(Q, n, row, c, r0)
        assert torch.equal(r, r0) if row == 0 else float((r - want).abs().max()) <= 1e-13 * float(r0.norm() + 1.0)
        assert abs(float(pair[0]) - float(want @ want)) <= 1e-13 * float(want @ want) and float(pair[1]) == SENTINEL
    # flip sum: the double adds in the header's order
    for P in (1, 2, 8):
        xT, zT = vec(P * n, 400 + P), torch.zeros(P * n, dtype=F64)
        be.flipsum(xT, zT, P)
        assert torch.equal(zT, pr.ref_flipsum(xT, P, n))
    # remote part: one source is the same sequence of operations; several sources differ in the order of the additions
    x, y0 = vec(n, 500 + n), vec(n, 501 + n)
    xs = [vec(n, 510 + j) for j in range(3)]
    ad, sh = torch.tensor([0.37], dtype=F64), torch.tensor([-0.6], dtype=F64)
    for count, a_dev, shift in ((0, None, None), (0, ad, sh), (1, ad, sh), (1, None, None), (3, ad, sh)):
        y, out = y0.clone(), torch.zeros(1, dtype=F64)
        be.axpy_multi_dot(-2.0, a_dev, xs[:count], shift, None, x, y, out)
        want = pr.ref_axpy_multi(-2.0, None if a_dev is None else 0.37, xs[:count], None if shift is None else -0.6, x, y0)
        if count <= 1:
            assert torch.equal(y, want)
        else:
            assert float((y - want).abs().max()) <= 1e-14 * float(y0.abs().max() + 3 * 2.0 * max(t.abs().max() for t in xs))
        assert abs(float(out[0]) - float(x @ want)) <= 1e-13 * float(x.norm() * want.norm())
    y, out = y0.clone(), torch.tensor([SENTINEL], dtype=F64)
    be.axpy_multi_dot(-2.0, ad, xs, sh, torch.tensor([1.0], dtype=F64), x, y, out)
    assert torch.equal(y, y0) and float(out[0]) == SENTINEL
    # finish
    pair = torch.tensor([float(r0 @ r0), 0.3], dtype=F64)
    row = torch.full((ldq,), SENTINEL, dtype=F64)
    uo, al, bt = torch.zeros(n, dtype=F64), torch.zeros(1, dtype=F64), torch.zeros(1, dtype=F64)
    be.plz_finish(r0, y0, pair, row, 2, uo, al, bt)
    q, uw, alpha, beta = pr.ref_plz_finish(r0, y0, float(pair[0]), float(pair[1]))
    assert torch.equal(row[:n], q) and torch.equal(uo, uw) and float(al[0]) == alpha and float(bt[0]) == beta
    assert bool((row[n:] == SENTINEL).all())
