"""tests/matvec_reference.py proved on the CPU (no GPU): the numpy references against the oracle, scipy and dense products; the
exact input class really is exact (fp64 = longdouble bit for bit, in any summation order); the rounding bounds hold for an
honest fp64 evaluation in natural, reversed and random order; the case builders produce the geometry they claim."""
import numpy as np
import pytest
import torch

import matvec_reference as ref
import oracle
from dominantsparseeigenad_amd.synthetic import normal_vector

LD = np.longdouble
SHIFT_EXACT, SHIFT_RANDOM = 0.375, 0.6180339887498949
G_EXACT, G_RANDOM = 0.875, 1.0690449676496976


# ---- the operators as (rows, cols, vals) triplets: an evaluation that shares nothing with the references ----------------
def tfim_triplets(L, L_local, offset, g, ds):
    n = 1 << L_local
    i = np.arange(n, dtype=np.int64)
    d = np.empty(n, dtype=np.int64)
    for k in range(n):                                # -sum_j s_j s_j+1 on the bits of the global index, Python integers
        gi = offset + k
        s = [1 - 2 * ((gi >> j) & 1) for j in range(L)]
        d[k] = -sum(s[j] * s[(j + 1) % L] for j in range(L))
    rows = [i] + [i] * L_local
    cols = [i] + [i ^ (1 << j) for j in range(L_local)]
    vals = [ds * d.astype(np.float64)] + [np.full(n, -g)] * L_local
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), n


def csr_triplets(rowptr, cols, vals):
    n = rowptr.size - 1
    return np.repeat(np.arange(n), np.diff(rowptr)), cols.astype(np.int64), vals, n


def dense_triplets(S):
    n = S.shape[0]
    r, c = np.divmod(np.arange(n * n), n)
    return r, c, S.reshape(-1), n


def stencil_triplets(coef, V):
    n = V.size
    i = np.arange(n)
    rows = np.concatenate((i, i[:-1], i[1:]))
    cols = np.concatenate((i, i[1:], i[:-1]))
    vals = np.concatenate((-2 * coef + V, np.full(n - 1, coef), np.full(n - 1, coef)))
    return rows, cols, vals, n


def orders(count, seed):
    return {"natural": np.arange(count), "reversed": np.arange(count)[::-1], "random": np.random.default_rng(seed).permutation(count)}


def evaluate(trip, x, shift, order):
    """fp64, one term after the other in ``order`` (np.add.at is unbuffered and sequential); then the shift; x.y likewise"""
    rows, cols, vals, n = trip
    y = np.zeros(n)
    np.add.at(y, rows[order], (vals * x[cols])[order])
    y = y - shift * x
    p = x * y
    o = order[order < n] if order.size >= n else np.arange(n)
    return y, float(np.cumsum(p[o])[-1])


def small_cases(exact):
    """(name, apply, triplets, n, m) of every family at sizes that take seconds here"""
    g = G_EXACT if exact else G_RANDOM
    out = []
    for L, Ll, off in ((10, 10, 0), (10, 8, 3 << 8), (5, 5, 0), (33, 9, (1 << 32) | (0x15A5A5 << 9)), (62, 9, (1 << 61) | (1 << 60) | (1 << 9))):
        out.append(("tfim %d/%d" % (L, Ll), ref.tfim_apply(L, Ll, off, g, 1.0), tfim_triplets(L, Ll, off, g, 1.0), 1 << Ll, L + 1))
    for name in ("avg6-1", "avg6-1037", "avg2-1037", "avg60-129", "long-rows", "group-stride"):
        rowptr, cols, n, m = ref.csr_case(name)
        vals = ref.csr_values(int(rowptr[-1]), 31, exact)
        out.append(("csr " + name, ref.csr_apply(rowptr, cols, vals), csr_triplets(rowptr, cols, vals), n, m))
    for nsl in (1, 5, 37, 129):
        rowptr, cols, n, m = ref.sell_case(nsl)
        vals = ref.csr_values(int(rowptr[-1]), 41, exact)
        out.append(("sell %d" % nsl, ref.csr_apply(rowptr, cols, vals), csr_triplets(rowptr, cols, vals), n, m))
    for n in (1, 3, 513, 1025):
        coef = -1.625 if exact else -0.5 / 0.37 ** 2
        V = ref.eighths(n, 81) if exact else normal_vector(n, 82)
        out.append(("stencil %d" % n, ref.stencil_apply(coef, V), stencil_triplets(coef, V), n, 4))
    for n in (1, 65, 129):
        S = ref.symdense_storage(n, n + (n & 1) + 6, 91 if exact else 92, exact)[1]
        out.append(("symdense %d" % n, ref.dense_apply(S), dense_triplets(S), n, n))
    return out


# ---- the references say what the oracle, scipy and a dense product say -------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 3, 5, 8])
def test_tfim_reference_is_the_table_operator(L):
    n = 1 << L
    model = oracle.TFIMTables(L, g=torch.tensor([G_RANDOM], dtype=torch.float64))
    assert np.array_equal(ref.tfim_diag(L, 0, n), model.diag.numpy().astype(np.int64))
    x = normal_vector(n, 1)
    want = model.H(torch.from_numpy(x)).numpy()
    got, scale = ref.tfim_apply(L, L, 0, G_RANDOM, 1.0)(x, np.float64)
    assert np.max(np.abs(got - want)) <= 1e-14 * np.max(scale)
    assert np.allclose(ref.tfim_apply(L, L, 0, 1.0, 0.0)(x, np.float64)[0], model.dHdg(torch.from_numpy(x)).numpy(), rtol=0, atol=1e-13)
    for Ll in range(L):                               # slabs: the global diagonal, the local flips
        for rank in range(1 << (L - Ll)):
            off, nl = rank << Ll, 1 << Ll
            xs = x[:nl]
            want = model.diag.numpy()[off:off + nl] * xs - G_RANDOM * sum(xs[np.arange(nl) ^ (1 << j)] for j in range(Ll))
            assert np.allclose(ref.tfim_apply(L, Ll, off, G_RANDOM, 1.0)(xs, np.float64)[0], want, rtol=0, atol=1e-13)


def test_tfim_diag_both_paths_and_long_chains():
    assert np.array_equal(ref.tfim_diag(13, 0, 1 << 13), oracle.operators.tfim_diag_closed_form(13).astype(np.int64))
    assert np.array_equal(ref.tfim_diag(13, 0, 1 << 13)[:4096], ref.tfim_diag(13, 0, 4096))
    for L, off in ((33, (1 << 32) | (0x15A5A5 << 9)), (33, 0x1F0F0F << 9), (62, (1 << 61) | (0x5A5A5A5A5A5A5 << 9)),
                   (62, (1 << 60) | (0x2A5A5A5A5A5A5 << 9))):
        d = ref.tfim_diag(L, off, 512)
        for i in (0, 1, 2, 255, 510, 511):            # -sum_j s_j s_j+1 written out on the bits of the global index
            gi = off + i
            s = [1 - 2 * ((gi >> j) & 1) for j in range(L)]
            assert d[i] == -sum(s[j] * s[(j + 1) % L] for j in range(L))
        assert len(set(d.tolist())) > 1


def test_flip_sum_is_the_xor_gather():
    x = normal_vector(1 << 9, 3)
    i = np.arange(1 << 9)
    assert np.array_equal(ref.flip_sum(x, 9), sum((x[i ^ (1 << j)] for j in range(1, 9)), x[i ^ 1]))


@pytest.mark.parametrize("n", [1, 2, 3, 513])
def test_stencil_reference(n):
    V, x, h = normal_vector(n, 4), normal_vector(n, 5), 0.37
    model = oracle.Stencil3(n, h, torch.from_numpy(V))
    got, scale = ref.stencil_apply(-0.5 / h ** 2, V)(x, np.float64)
    assert np.max(np.abs(got - model.H(torch.from_numpy(x)).numpy())) <= 1e-14 * np.max(scale)
    # halos: rows 1..n of the (n + 2)-row operator applied to (lo, x, hi)
    big = oracle.Stencil3(n + 2, h, torch.from_numpy(np.concatenate(([0.0], V, [0.0]))))
    want = big.H(torch.from_numpy(np.concatenate(([0.7], x, [-1.3])))).numpy()[1:-1]
    assert np.max(np.abs(ref.stencil_apply(-0.5 / h ** 2, V, 0.7, -1.3)(x, np.float64)[0] - want)) <= 1e-14 * (np.max(scale) + 20)


def test_csr_reference_is_scipy_and_dense():
    import scipy.sparse as sp
    for name in ("avg6-1", "avg6-129", "avg2-129", "avg60-129"):
        rowptr, cols, n, m = ref.csr_case(name)
        vals = ref.csr_values(int(rowptr[-1]), 31, False)
        M = sp.csr_matrix((vals, cols, rowptr), shape=(n, n))
        x = normal_vector(n, 6)
        got, scale = ref.csr_apply(rowptr, cols, vals)(x, np.float64)
        assert np.max(np.abs(got - M @ x)) <= 1e-13 * max(np.max(scale), 1e-300)
        assert np.max(np.abs(got - M.toarray() @ x)) <= 1e-13 * max(np.max(scale), 1e-300)
        Mabs = sp.csr_matrix((np.abs(vals), cols, rowptr), shape=(n, n))      # (repeated columns: |v1| + |v2|, not |v1 + v2|)
        assert np.max(np.abs(scale - Mabs @ np.abs(x))) <= 1e-13 * max(np.max(scale), 1e-300)
        assert m == np.diff(rowptr).max()


def test_symdense_storage():
    for exact in (True, False):
        store, S = ref.symdense_storage(65, 72, 9, exact)
        assert np.array_equal(S, S.T) and np.array_equal(S.astype(np.float32).astype(np.float64), S)
        assert np.isnan(store[np.tril_indices(65, -1)]).all() and np.isnan(store[:, 65:]).all()
        assert np.array_equal(store[np.triu_indices(65)], S[np.triu_indices(65)])
        assert np.array_equal(ref.symmetric_from_upper(np.nan_to_num(store[:, :65])), S)
    x = normal_vector(65, 10)
    assert np.allclose(ref.dense_apply(S)(x, np.float64)[0], S @ x, rtol=0, atol=1e-12)


# ---- the exact class is exact --------------------------------------------------------------------------------------------
def test_exact_inputs_are_exact_in_any_order():
    for name, apply, trip, n, m in small_cases(True):
        x = ref.exact_vector(n, 21)
        y64, sc = ref.shifted(apply, x, SHIFT_EXACT, np.float64)
        yld, _ = ref.shifted(apply, x, SHIFT_EXACT, LD)
        ref.headroom(n, 4, float(sc.max()))
        assert np.array_equal(yld, y64.astype(LD)), name
        dot = float(np.sum(x * y64))
        assert LD(dot) == np.sum(x.astype(LD) * yld), name
        for label, order in orders(trip[0].size, 22).items():
            y, d = evaluate(trip, x, SHIFT_EXACT, order)
            assert np.array_equal(y, y64) and d == dot, (name, label)


def test_headroom_of_the_large_exact_cases():
    ref.headroom(1 << 24, 4, 24 * 4 + G_EXACT * 24 * 4 + 4)                 # TFIM L = 24
    ref.headroom((1 << 21) + 3, 4, 1.625 * 16 + 2 * 4 + 4)                  # stencil
    ref.headroom(64 * 16389, 4, 2 * 130 * 4 + 4)                            # SELL, second trip
    ref.headroom(128 * 4096 + 129, 4, 2 * 2100 * 4 + 4)                     # CSR
    with pytest.raises(AssertionError):
        ref.headroom(1 << 40, 4, 1 << 10)


# ---- the bounds hold for an honest fp64 evaluation -----------------------------------------------------------------------
def test_rounding_bounds_hold_in_every_order():
    worst = {}
    for name, apply, trip, n, m in small_cases(False):
        x = normal_vector(n, 23)
        want, scale = ref.shifted(apply, x, SHIFT_RANDOM, LD)
        dot = np.sum(x.astype(LD) * want)
        for label, order in orders(trip[0].size, 24).items():
            y, d = evaluate(trip, x, SHIFT_RANDOM, order)
            ry = ref.worst_ratio(np.abs(y.astype(LD) - want), ref.matvec_bound(m, scale))
            rd = ref.worst_ratio(abs(LD(d) - dot), ref.dot_bound(n, m, x, scale))
            assert ry <= 1.0 and rd <= 1.0, (name, label, ry, rd)
            worst[name] = max(worst.get(name, 0.0), ry, rd)
    print("  ".join("%s %.3f" % kv for kv in worst.items()))
    assert max(worst.values()) > 0.01          # (the bound is a bound, not a formality)


def test_a_wrong_precision_or_a_dropped_term_is_outside_the_bounds():
    name, apply, trip, n, m = small_cases(False)[0]
    x = normal_vector(n, 23)
    want, scale = ref.shifted(apply, x, SHIFT_RANDOM, LD)
    y32 = (apply(x.astype(np.float32), np.float32)[0] - np.float32(SHIFT_RANDOM) * x.astype(np.float32)).astype(np.float64)
    assert ref.worst_ratio(np.abs(y32.astype(LD) - want), ref.matvec_bound(m, scale)) > 1e3
    rows, cols, vals, _ = trip
    y, _ = evaluate((rows[1:], cols[1:], vals[1:], n), x, SHIFT_RANDOM, np.arange(rows.size - 1))
    assert ref.worst_ratio(np.abs(y.astype(LD) - want), ref.matvec_bound(m, scale)) > 1e3


def test_lanczos_relations_hold_for_fp64_and_catch_a_missing_division():
    for name, apply, trip, n, m in small_cases(False):
        if n < 64 or name.startswith(("symdense", "csr")):
            continue
        q0 = normal_vector(n, 25)
        for label, order in orders(n, 26).items():
            Q, a, b = ref.host_lanczos3(apply, q0, None if label == "natural" else order)
            ratios = ref.lanczos_relations(apply, m, q0, Q, a, b)
            assert max(ratios.values()) <= 1.0, (name, label, ratios)
        Q, a, b = ref.host_lanczos3(apply, q0)
        bad = Q.copy()
        bad[2] *= 1.0 + 1e-12                                   # q2 not quite r / beta
        assert max(ref.lanczos_relations(apply, m, q0, bad, a, b).values()) > 1.0
        assert max(ref.lanczos_relations(apply, m, q0, Q, [a[0], a[1] * (1 + 1e-11), a[2]], b).values()) > 1.0


# ---- the case builders produce the geometry they claim -------------------------------------------------------------------
def test_csr_case_geometry():
    for name in ("avg6-1", "avg6-129", "avg6-1037"):
        assert ref.csr_takes_stream(ref.csr_case(name)[0], 0) and not ref.csr_takes_stream(ref.csr_case(name)[0], 8)
    for name in ("avg2-129", "avg2-1037"):
        rowptr = ref.csr_case(name)[0]
        assert not ref.csr_takes_stream(rowptr, 0) and rowptr[-1] / (rowptr.size - 1) < 4
    rowptr = ref.csr_case("avg60-129")[0]
    assert rowptr[-1] / 129 > 48
    for name in ("avg6-129", "avg6-1037", "avg2-129", "avg2-1037", "avg60-129", "group-stride", "long-rows"):
        rowptr = ref.csr_case(name)[0]
        assert rowptr[1] == 0 and rowptr[-1] == rowptr[-2] and (np.diff(rowptr) == 0).sum() >= 3
    assert ref.csr_case("group-stride")[2] == 8192 + 5 > ref.MAX_EW_BLOCKS * 4
    rowptr, _, n, _ = ref.csr_case("stream-trips")
    assert ref.csr_takes_stream(rowptr, 0) and n == 128 * 4096 + 129 and ref.csr_chunk_sizes(rowptr).size == 4098
    rowptr, _, n, _ = ref.csr_case("long-rows")
    sizes = ref.csr_chunk_sizes(rowptr)
    assert n >= 2200 and ref.csr_takes_stream(rowptr, 0) and sizes[1] > ref.CSR_CAP and (np.delete(sizes, 1) <= ref.CSR_CAP).all()


@pytest.mark.parametrize("nslices", [1, 5, 37, 129, 4 * 4096 + 5])
def test_sell_case_geometry(nslices):
    rowptr, cols, n, m = ref.sell_case(nslices)
    assert (n + 63) // 64 == nslices and n % 64 != 0
    widths = ref.sell_slice_widths(rowptr, n)
    assert list(widths) == ref.sell_widths(nslices) and m == max(widths.max(), 1)
    if 30 < nslices < 1000:
        assert set(widths.tolist()) == set(ref.WIDTHS)
    if nslices == 1:
        assert widths[0] == 130
    assert list(ref.sell_slice_widths(rowptr, n, 2)) == [(w + 1) // 2 * 2 for w in widths]
    assert list(ref.sell_slice_widths(rowptr, n, 4)) == [(w + 3) // 4 * 4 for w in widths]
    assert cols.min() >= 0 and cols.max() < n
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    assert np.abs(cols - rows).max() <= 300                   # 16-bit column deltas apply
    if nslices > 1000:
        assert (nslices + 3) // 4 > ref.MAX_TFIM_BLOCKS       # second trip of the grid


@pytest.mark.parametrize("lo,hi", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("hb", [3, "n"])
def test_slab_pattern_geometry(hb, lo, hi):
    n = ref.sell_case(37)[2]
    hb = n if hb == "n" else hb
    rowptr, cols, n2, m = ref.slab_pattern(37, hb, lo, hi)
    assert n2 == n and rowptr[-1] == cols.size and m >= np.diff(rowptr).max()
    assert cols.min() >= (-hb if lo else 0) and cols.max() < (n + hb if hi else n)
    assert (cols.min() < 0) == lo and (cols.max() >= n) == hi


def test_tile_counts_and_block_rows():
    assert (1 << 18) >> 6 == ref.MAX_TFIM_BLOCKS and (1 << 19) >> 6 > ref.MAX_TFIM_BLOCKS
    assert (1000 + 63) // 64 >= 13
    assert ((1 << 21) + 3 + 511) // 512 > 4096
    table = ref.table_values(5000, 41)
    assert np.unique(table).size <= 200 and np.unique(ref.eighths(5000, 41)).size <= 33


def test_constant_row_sums():
    rowptr, cols = ref.csr_pattern(np.random.default_rng(5).integers(1, 10, size=4096), 6, band=300)
    vals = ref.constant_row_sum_values(rowptr, 5.0, 7)
    assert np.array_equal(ref.csr_apply(rowptr, cols, vals)(np.ones(4096), np.float64)[0], np.full(4096, 5.0))
    assert np.array_equal(vals, np.round(vals))
