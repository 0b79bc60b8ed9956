"""Row-partitioned macro phases (include/dsea.h "row-partitioned macro phases"): their plain fp64 reference expressions and a
LOCKSTEP composer that runs the four-phase step for P virtual ranks held in ONE process.

Shared by tests/test_partitioned_phase_reference_cpu.py (backend: tests/cpu_backend.CpuBackend) and
tests/test_gpu_partitioned_phases.py (backend: partitioned.HipBackend).  No process group, no spawned process: the
"all-reduce" is a host sum of the P local results in rank order, the "exchange" a set of torch copies between the slabs.

The reference expressions take HOST tensors / python floats and evaluate the header's expression in the header's order with
every operation rounded on its own (torch CPU: one kernel per operation, no fma; the divisions of the finish phase go through
numpy because a device-side ``tensor / python_float`` may be evaluated as a multiplication by the reciprocal)."""
import functools
import math

import numpy as np
import torch

import oracle
from dominantsparseeigenad_amd.synthetic import normal_vector

F64 = torch.float64
RR, DAD, RRNEW, ALPHA, BETA, RESNORM, DONE, ITERS = range(8)      # the CG state of include/dsea.h (8 doubles)
SENTINEL = -7.25e300       # padding of a basis row / guard of a scalar slot: enormous (it would swamp any sum) and exact


def round_up(v, m):
    return (v + m - 1) // m * m


def vec(n, seed):
    return torch.from_numpy(normal_vector(int(n), int(seed)))


def padded_basis(rows, n, seed, ldq=None):
    """(rows x ldq) host basis of normal draws, ldq = round_up(n, 32) made > n, the padding columns hold SENTINEL"""
    ldq = ldq or round_up(n, 32)
    if ldq == n:
        ldq += 32
    Q = torch.full((rows, ldq), SENTINEL, dtype=F64)
    Q[:, :n] = torch.from_numpy(normal_vector(rows * n, seed).reshape(rows, n))
    return Q, ldq


def ulp_distance(a, b):
    """largest distance between two fp64 host tensors counted in representable numbers (0 = bit-identical up to the sign of
    zero)"""
    ia = a.contiguous().view(torch.int64)
    ib = b.contiguous().view(torch.int64)
    lo = torch.iinfo(torch.int64).min
    ia = torch.where(ia < 0, lo - ia, ia)           # sign-magnitude -> monotone integers
    ib = torch.where(ib < 0, lo - ib, ib)
    return int((ia - ib).abs().max()) if a.numel() else 0


# ------------------------------------------------------------------------------------------------ reference expressions
def ref_form_r(Q, n, i, u, alpha, beta):
    """r = (u - alpha Q[i-1]) - beta Q[i-2]; the beta term exists from i = 2 on and drops when beta is None"""
    r = u - alpha * Q[i - 1, :n]
    if beta is not None and i >= 2:
        r = r - beta * Q[i - 2, :n]
    return r


def ref_flipsum(xT, P, chunk):
    """zT[s] = sum over b = 0..p-1 of xT[s ^ (1<<b)], accumulated in that order from 0 (P = 1: zeros)"""
    X = xT.reshape(P, chunk)
    Z = torch.zeros_like(X)
    b = 1
    while b < P:
        Z = Z + X[[s ^ b for s in range(P)]]
        b <<= 1
    return Z.reshape(-1)


def ref_axpy_multi(a_host, a_dev, xs, shift, x, y):
    """y_new:  sum = ((xs0 + xs1) + ...) ; y = y + a sum ; y = y - s x,   a = a_host * a_dev (a_dev None: 1)"""
    a = a_host * (a_dev if a_dev is not None else 1.0)
    out = y
    if len(xs):
        s = xs[0]
        for t in xs[1:]:
            s = s + t
        out = out + a * s
    if shift is not None:
        out = out - shift * x
    return out.clone() if out is y else out


def ref_plz_finish(r, y, pair0, pair1):
    """(q, u, alpha, beta) = (r / sqrt(pair0), y / sqrt(pair0), pair1 / pair0, sqrt(pair0)): IEEE sqrt and divisions"""
    beta = math.sqrt(pair0)
    q = torch.from_numpy(r.numpy() / np.float64(beta))
    u = torch.from_numpy(y.numpy() / np.float64(beta))
    return q, u, pair1 / pair0, beta


def ref_correct(Q, n, row, c, r):
    """r - sum_{j<row} c_j Q[j]  (row = 0: r)"""
    if row == 0:
        return r.clone()
    return r - Q[:row, :n].T @ c[:row]


# ------------------------------------------------------------------------------------------------ full operators (oracle)
TFIM_G = 0.85


@functools.lru_cache(maxsize=None)
def tfim_full(L):
    return oracle.TFIMTables(L, g=torch.tensor([TFIM_G], dtype=F64))


STENCIL_N, STENCIL_CUTS = 1013, (337, 1, 675)         # three unequal slabs, one of a single row (both halos on one element)


def stencil_potential(n):
    return 0.5 * torch.linspace(-1, 1, n, dtype=F64) ** 2 + 0.1 * vec(n, 66).abs()


@functools.lru_cache(maxsize=None)
def stencil_full(n):
    return oracle.Stencil3(n, 2.0 / n, stencil_potential(n))


@functools.lru_cache(maxsize=None)
def oracle_lanczos(kind, size, k, seed):
    """oracle.lanczos_tridiag on the FULL operator from q0 = normal_vector(n, seed): computed once, shared, never modified"""
    A, n = (tfim_full(size).H, 1 << size) if kind == "tfim" else (stencil_full(size).H, size)
    draws = iter([vec(n, seed), torch.zeros(n, dtype=F64)])
    return oracle.lanczos_tridiag(A, k, sparse=True, dim=n, draw=lambda m, dtype: next(draws))


@functools.lru_cache(maxsize=None)
def oracle_cg_iterates(kind, size, shift, iters, seed):
    """[x_1 .. x_iters] of oracle.cg_solve on (A - shift) x = b: iterate j is the solve capped at j iterations"""
    A, n = (tfim_full(size).H, 1 << size) if kind == "tfim" else (stencil_full(size).H, size)
    b, x0 = vec(n, seed), vec(n, seed + 1)
    return [oracle.cg_solve(lambda v: A(v) - shift * v, b, x0, sparse=True, eps=0.0, maxiter=j) for j in range(1, iters + 1)]


# ------------------------------------------------------------------------------------------------ the lockstep composer
class _Rank:
    pass


class Lockstep:
    """P virtual ranks in one process.  ``make_backend(n_local)`` builds one backend per rank (CpuBackend or HipBackend);
    every phase is issued for rank 0..P-1 in turn before the next phase starts."""

    def __init__(self, rows, make_backend):
        self.rows = [int(m) for m in rows]
        self.offs = [sum(self.rows[:r]) for r in range(len(self.rows))]
        self.P, self.n = len(self.rows), sum(self.rows)
        self.bes = [make_backend(m) for m in self.rows]
        self.device = self.bes[0].device

    # -- the two collectives
    @staticmethod
    def allreduce(parts):
        """in-place sum of the P local results, added on the host in rank order; every rank receives the same bits"""
        tot = parts[0].detach().cpu().clone()
        for t in parts[1:]:
            tot = tot + t.detach().cpu()
        for t in parts:
            t.copy_(tot)

    def slab(self, full, r):
        return full[self.offs[r]:self.offs[r] + self.rows[r]].to(self.device).clone()

    def gather(self, parts):
        return torch.cat([t.detach().cpu() for t in parts])

    # -- operator specific
    def correct_and_matvec(self, i):
        """correction of S.r by S.c[:i] and y = A r over all ranks; leaves pair = (local r.r, local r.Ar)"""
        raise NotImplementedError

    def apply_shift_dot(self, xs, ys, shifts, outs, skips):
        """y = (A - shift) x over all ranks; outs[r] = local x.y"""
        raise NotImplementedError

    # -- Lanczos: dots -> all-reduce -> correct (+ mat-vec, exchange, remote part) -> all-reduce -> finish
    def lanczos_begin(self, k, q0_full):
        self.k, self.S = k, []
        for r, be in enumerate(self.bes):
            if hasattr(be, "reserve"):
                be.reserve(k)
            S, m = _Rank(), self.rows[r]
            S.n, S.ldq = m, round_up(m, 32)
            S.Q = be.zeros(k, S.ldq)
            S.alphas, S.betas = be.zeros(k), be.zeros(max(k - 1, 1))
            S.c, S.pair = be.zeros(k + 2), be.zeros(2)
            S.r, S.u, S.y = self.slab(q0_full, r), be.zeros(m), be.zeros(m)
            self.S.append(S)

    def lanczos_step(self, i):
        if i >= 1:
            for be, S in zip(self.bes, self.S):
                be.plz_dots(S.Q, S.ldq, S.n, i, S.u, S.alphas[i - 1:i], S.betas[i - 2:i - 1] if i >= 2 else None, S.r, S.c)
            self.allreduce([S.c[:i + 1] for S in self.S])
        self.correct_and_matvec(i)
        self.allreduce([S.pair for S in self.S])
        for be, S in zip(self.bes, self.S):
            be.plz_finish(S.r, S.y, S.pair, S.Q[i], i, S.u, S.alphas[i:i + 1], S.betas[i - 1:i] if i >= 1 else None)

    def basis_row(self, i):
        return self.gather([S.Q[i, :S.n] for S in self.S])

    def replicated(self, name, i):
        """scalar i of ``alphas`` / ``betas``: the ranks must hold the same bits"""
        vals = [float(getattr(S, name)[i]) for S in self.S]
        assert all(v == vals[0] for v in vals), (name, i, vals)
        return vals[0]

    # -- shifted CG (reference CG.py:24-41 on slabs): the loop of PartitionedOperator.solve_shifted, one iteration per call
    def cg_begin(self, shift, b_full, x0_full, eps=0.0):
        self.eps, self.C = float(eps), []
        for r, be in enumerate(self.bes):
            C, m = _Rank(), self.rows[r]
            C.state = be.zeros(8)
            C.r, C.d, C.Ad = be.zeros(m), be.zeros(m), be.zeros(m)
            C.x, C.b = self.slab(x0_full, r), self.slab(b_full, r)
            C.shift = torch.tensor([shift], dtype=F64).to(self.device)
            self.C.append(C)
        Cs = self.C
        self.apply_shift_dot([C.x for C in Cs], [C.Ad for C in Cs], [C.shift for C in Cs],
                             [C.state[DAD:DAD + 1] for C in Cs], [None] * self.P)
        for be, C in zip(self.bes, Cs):
            be.cg_init(C.b, C.Ad, C.r, C.d, C.state)
        self.allreduce([C.state[RR:RR + 1] for C in Cs])
        for be, C in zip(self.bes, Cs):
            be.cg_init_check(C.state, self.eps)

    def cg_iteration(self):
        Cs = self.C
        self.apply_shift_dot([C.d for C in Cs], [C.Ad for C in Cs], [C.shift for C in Cs],
                             [C.state[DAD:DAD + 1] for C in Cs], [C.state[DONE:DONE + 1] for C in Cs])
        self.allreduce([C.state[DAD:DAD + 1] for C in Cs])
        for be, C in zip(self.bes, Cs):
            be.cg_update(C.x, C.r, C.d, C.Ad, C.state)
        self.allreduce([C.state[RRNEW:RRNEW + 1] for C in Cs])
        for be, C in zip(self.bes, Cs):
            be.cg_check(C.state, self.eps)
            be.cg_direction(C.r, C.d, C.state)
        return self.gather([C.x for C in Cs])


class LockstepTFIM(Lockstep):
    """TFIM chain of L sites over P = 2^p slabs.  Top-bit flips: none (P = 1: axpy_multi_dot with count = 0 only closes the
    dot), pairwise (one whole slab per partner), or transposed (slab chunks to every rank, flipsum, chunks back) -- "auto" is
    the rule of PartitionedTFIMOperator: transposed from P = 4 on where a slab has at least P rows."""

    def __init__(self, L, P, make_backend, form="auto"):
        p = P.bit_length() - 1
        assert (1 << p) == P and p <= L
        nloc = 1 << (L - p)
        super().__init__([nloc] * P, make_backend)
        self.L, self.p, self.nloc = L, p, nloc
        self.transposed = (P >= 4 and nloc >= P) if form == "auto" else (form == "transposed")
        assert not self.transposed or (P >= 2 and nloc % P == 0)
        self.g = [torch.tensor([TFIM_G], dtype=F64).to(self.device) for _ in range(P)]
        for r, be in enumerate(self.bes):
            be.attach_tfim(L, L - p, r * nloc, self.g[r])
        if self.transposed:
            self.xT, self.zT, self.z = ([be.zeros(nloc) for be in self.bes] for _ in range(3))
        else:
            self.recv = [[be.zeros(nloc) for _ in range(p)] for be in self.bes]

    def exchange(self, vecs):
        """per rank the list of buffers whose sum is the remote part (the partner slabs, or their sum)"""
        P = self.P
        if not self.transposed:
            for r in range(P):
                for b in range(self.p):
                    self.recv[r][b].copy_(vecs[r ^ (1 << b)])
            return self.recv
        ch = self.nloc // P
        for me in range(P):                       # all-to-all: chunk `me` of every rank's slab goes to rank `me`
            for s in range(P):
                self.xT[me][s * ch:(s + 1) * ch].copy_(vecs[s][me * ch:(me + 1) * ch])
        for me, be in enumerate(self.bes):
            be.flipsum(self.xT[me], self.zT[me], P)
        for s in range(P):                        # all-to-all back: zT[s] of every rank to rank s
            for me in range(P):
                self.z[s][me * ch:(me + 1) * ch].copy_(self.zT[me][s * ch:(s + 1) * ch])
        return [[z] for z in self.z]

    def correct_and_matvec(self, i):
        for be, S in zip(self.bes, self.S):
            be.plz_correct_matvec(S.Q, S.ldq, i, S.c, S.r, S.y, S.pair)
        recv = self.exchange([S.r for S in self.S])
        for r, (be, S) in enumerate(zip(self.bes, self.S)):
            be.axpy_multi_dot(-1.0, self.g[r], recv[r], None, None, S.r, S.y, S.pair[1:2])

    def apply_shift_dot(self, xs, ys, shifts, outs, skips):
        for be, x, y in zip(self.bes, xs, ys):
            be.tfim_local(x, y, "H")
        recv = self.exchange(xs)
        for r, be in enumerate(self.bes):
            be.axpy_multi_dot(-1.0, self.g[r], recv[r], shifts[r], skips[r], xs[r], ys[r], outs[r])


class LockstepStencil(Lockstep):
    """3-point stencil on n grid points cut into contiguous slabs of ``rows`` points; one halo element per neighbour"""

    def __init__(self, n, rows, make_backend):
        assert sum(rows) == n
        super().__init__(rows, make_backend)
        V, coef = stencil_potential(n), -0.5 / (2.0 / n) ** 2
        self.halo, self.V = [], []
        for r, be in enumerate(self.bes):
            self.V.append(self.slab(V, r))
            self.halo.append(be.zeros(2))
            be.attach_stencil(self.rows[r], coef, self.V[r], self.halo[r], r > 0, r < self.P - 1)

    def halo_exchange(self, xs):
        for r in range(self.P):
            if r > 0:
                self.halo[r][0:1].copy_(xs[r - 1][self.rows[r - 1] - 1:self.rows[r - 1]])
            if r < self.P - 1:
                self.halo[r][1:2].copy_(xs[r + 1][0:1])

    def correct_and_matvec(self, i):
        for be, S in zip(self.bes, self.S):
            be.plz_correct(S.Q, S.ldq, S.n, i, S.c, S.r, S.pair)
        self.halo_exchange([S.r for S in self.S])
        for be, S in zip(self.bes, self.S):
            be.stencil_local(S.r, S.y, None, S.pair[1:2], None)

    def apply_shift_dot(self, xs, ys, shifts, outs, skips):
        self.halo_exchange(xs)
        for r, be in enumerate(self.bes):
            be.stencil_local(xs[r], ys[r], shifts[r], outs[r], skips[r])


# ------------------------------------------------------------------------------------------------ the shared assertions
LANCZOS_SEED, CG_SEED, CG_ITERS = 7300, 7400, 20
TOL = 1e-10


def lockstep_cases():
    """(kind, size, slab rows or P): TFIM L = 5, 7, 10 over P = 1, 2, 4, 8 (L = 5, P = 8: slabs of four rows, fewer rows than
    ranks, so the pairwise form carries three partners there) and the 3-point stencil in three unequal slabs"""
    return [("tfim", L, P) for L in (5, 7, 10) for P in (1, 2, 4, 8)] + [("stencil", STENCIL_N, STENCIL_CUTS)]


def make_lockstep(kind, size, part, make_backend):
    if kind == "tfim":
        return LockstepTFIM(size, part, make_backend)
    return LockstepStencil(size, part, make_backend)


def cg_shift(kind, size):
    """a shift below the spectrum: A - shift is positive definite (TFIM: |E| <= L (1 + g); the stencil is positive)"""
    return -(size * (1.0 + TFIM_G) + 1.0) if kind == "tfim" else -1.0


def oracle_valid_steps(ao, bo):
    """how many steps of the oracle run define a comparison.  The TFIM chain of L = 5 sites has 18 distinct eigenvalues, so the
    Krylov space of ANY start vector is exhausted at step 18: the oracle's own beta_17 is 5e-11 and everything it computes
    afterwards is its rounding error divided by that.  A vector q_i = r / beta_{i-1} carries the relative rounding error
    (1e-16) of r amplified by scale / beta_{i-1}; it supports a comparison at 1e-10 only while beta_{i-1} >= 1e-6 x scale.
    The rule reads the ORACLE's betas only; it cuts L = 5 at 18 steps and none of the other cases."""
    scale = float(ao.abs().max())
    small = (bo < 1e-6 * scale).nonzero()
    return int(small[0]) + 1 if small.numel() else int(ao.numel())


def check_lockstep_lanczos(run, kind, size):
    """k = min(n, 30) steps; after EVERY step alpha_i, beta_{i-1} within 1e-10 x scale and row i (i < 24) within 1e-10 of the
    oracle on the full operator, Q^T Q within 1e-13 of the identity (tests/test_gpu_parity.py::_lanczos_vs_oracle) -- over the
    steps the oracle itself defines (``oracle_valid_steps``: all of them except for L = 5); the steps after a breakdown are
    still run.  Returns the gathered (Q (valid, n), alphas, betas)."""
    n = run.n
    k = min(n, 30)
    Qo, ao, bo = oracle_lanczos(kind, size, k, LANCZOS_SEED)
    scale = float(ao.abs().max())
    valid = oracle_valid_steps(ao, bo)
    assert valid == (18 if (kind, size) == ("tfim", 5) else k)
    run.lanczos_begin(k, vec(n, LANCZOS_SEED))
    rows, alphas, betas = [], [], []
    for i in range(k):
        run.lanczos_step(i)
        alphas.append(run.replicated("alphas", i))
        if i >= 1:
            betas.append(run.replicated("betas", i - 1))
        rows.append(run.basis_row(i))
        if i >= 1 and i <= valid:     # (beta_{valid-1}, the breakdown itself, is a norm: still determined absolutely)
            assert abs(betas[i - 1] - float(bo[i - 1])) <= TOL * scale, ("beta", i - 1, betas[i - 1], float(bo[i - 1]))
        if i >= valid:
            continue
        assert abs(alphas[i] - float(ao[i])) <= TOL * scale, ("alpha", i, alphas[i], float(ao[i]))
        if i < min(k, 24):
            err = float((rows[i] - Qo[:, i]).abs().max())
            assert err <= TOL, ("basis row", i, err)
    Q = torch.stack(rows[:valid])
    G = Q @ Q.T
    assert float((G - torch.eye(valid, dtype=F64)).abs().max()) < 1e-13
    return Q, torch.tensor(alphas[:valid], dtype=F64), torch.tensor(betas[:valid - 1], dtype=F64)


def check_lockstep_cg(run, kind, size):
    """20 iterations of the shifted CG built from the phases, iterate for iterate against oracle.cg_solve on the full operator
    at 1e-10 x max|x| (tests/test_gpu_kernels.py::test_cg_phases_match_reference_sequence)"""
    n, shift = run.n, cg_shift(kind, size)
    ref = oracle_cg_iterates(kind, size, shift, CG_ITERS, CG_SEED)
    run.cg_begin(shift, vec(n, CG_SEED), vec(n, CG_SEED + 1))
    for j in range(CG_ITERS):
        x = run.cg_iteration()
        err = float((x - ref[j]).abs().max())
        assert err <= TOL * float(ref[j].abs().max()), ("CG iterate", j + 1, err)
    for C in run.C:
        assert float(C.state[ITERS]) == CG_ITERS and float(C.state[DONE]) == 0.0
