"""numpy references, input classes, error bounds and case builders of the operator mat-vec tests (tests/test_gpu_matvec_kernels.py,
proved on the CPU by tests/test_matvec_reference_cpu.py); no GPU, no torch.

TWO INPUT CLASSES, TWO VERDICTS (docs/design/04-kernels.md, "which test reaches which kernel")

  exact     vector entries are integers in [-4, 4]; matrix values, g, shift, coef, V, diag_scale and dense entries are multiples
            of 1/8 of modest size (|.| <= 2, fp32-representable).  Every product is then a multiple of 1/8 and every partial
            sum of a row, and of x.y, is a multiple of 1/8 far below 2^53 / 8 -- exact in fp64 in ANY order, with or without
            FMA.  ``headroom`` asserts n * max|x| * max|y| * 64 < 2^50 for every case that claims it.  Verdict: bit equality.
  random    synthetic.normal_vector entries, reference in np.longdouble.  Verdict: the componentwise rounding bounds below,
            which count operations and need no knowledge of the reduction tree:
                |y - y_ref|   <= (m + 4) u (|A||x| + |shift x|)                       m = most terms of a row, u = 2^-53
                |dot - x.y|   <= (n + m + 4) u sum_i |x_i| (|A||x| + |shift x|)_i
            and for the fused Lanczos tails the three-term relations of ``lanczos_relations`` on the device's own outputs.

An operator reference is a function ``apply(x, dtype) -> (A x, |A| |x|)`` evaluated in ``dtype``."""
import functools

import numpy as np

LD = np.longdouble
U = 2.0 ** -53

CSR_ROWS, CSR_CAP = 128, 6144          # k_spmv_csr_stream: rows of a chunk, LDS products of a chunk
MAX_TFIM_BLOCKS, MAX_EW_BLOCKS = 4096, 2048
WIDTHS = (0, 1, 3, 8, 9, 63, 64, 65, 130)     # slice widths of the ragged SELL cases
SMALL_WIDTHS = (0, 1, 3, 8, 9)                # ... of the 16389-slice case (second trip of the grid)


# ---- inputs ------------------------------------------------------------------------------------------------------------
def exact_vector(n, seed):
    return np.random.default_rng(seed).integers(-4, 5, size=n).astype(np.float64)


def eighths(shape, seed, span=16):
    """multiples of 1/8 in [-span/8, span/8]"""
    return np.random.default_rng(seed).integers(-span, span + 1, size=shape).astype(np.float64) / 8.0


def headroom(n, xmax, ymax):
    """the exact class: every partial sum of x.y is a multiple of 1/8 (x integer, y a multiple of 1/8 ... of 1/64 with a
    shift) below n xmax ymax; with the factor 64 it stays far below 2^53"""
    assert float(n) * float(xmax) * float(ymax) * 64.0 < 2.0 ** 50, (n, xmax, ymax)


def table_values(count, seed):
    """``count`` random values from a table of 200 normals (at most 255 distinct: the value-coded SELL layout takes them)"""
    from dominantsparseeigenad_amd.synthetic import normal_vector
    table = normal_vector(200, seed)
    return table[np.random.default_rng(seed).integers(0, 200, size=count)]


# ---- bounds ------------------------------------------------------------------------------------------------------------
def matvec_bound(m, scale):
    return (m + 4) * U * np.asarray(scale, dtype=np.float64)


def dot_bound(n, m, x, scale):
    return (n + m + 4) * U * float(np.sum(np.abs(np.asarray(x, dtype=LD)) * np.asarray(scale, dtype=LD)))


def worst_ratio(err, bound):
    """max err / bound over the components (0 / 0 counts as 0; err > 0 over bound = 0 as inf)"""
    err, bound = np.atleast_1d(np.asarray(err, dtype=np.float64)), np.atleast_1d(np.asarray(bound, dtype=np.float64))
    out = np.zeros_like(err)
    nz = bound > 0
    out[nz] = err[nz] / bound[nz]
    out[(~nz) & (err > 0)] = np.inf
    return float(out.max()) if out.size else 0.0


def shifted(apply, x, shift, dtype):
    """(A x - shift x, |A||x| + |shift x|) in dtype"""
    ax, sc = apply(x, dtype)
    xd = np.asarray(x, dtype=dtype)
    return ax - dtype(shift) * xd, sc + abs(dtype(shift)) * np.abs(xd)


# ---- TFIM --------------------------------------------------------------------------------------------------------------
def tfim_diag(L, row_offset, n):
    """d(gi) = -(L - 2 popcount(gi ^ rotl_L(gi, 1))), gi = row_offset + i (include/dsea.h).  Python integers up to 4096 rows
    (any L up to 62: no fixed-width arithmetic to get wrong), the same in uint64 numpy beyond (L <= 32 there)."""
    mask = (1 << L) - 1
    if n <= 4096:
        out = np.empty(n, dtype=np.int64)
        for i in range(n):
            gi = row_offset + i
            rot = ((gi << 1) | (gi >> (L - 1))) & mask
            out[i] = -(L - 2 * bin(gi ^ rot).count("1"))
        return out
    assert L <= 32
    gi = np.arange(n, dtype=np.uint64) + np.uint64(row_offset)
    x = gi ^ (((gi << np.uint64(1)) | (gi >> np.uint64(L - 1))) & np.uint64(mask))
    pop = np.zeros(n, dtype=np.int64)
    for b in range(L):
        pop += ((x >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
    return -(L - 2 * pop)


def flip_sum(x, nbits):
    """sum_j x[i ^ (1 << j)], j < nbits: an XOR-gather per bit (as a reshape: bit j swaps neighbouring blocks of 2^j)"""
    s = np.zeros_like(x)
    for j in range(nbits):
        s += x.reshape(-1, 2, 1 << j)[:, ::-1, :].reshape(-1)
    return s


def tfim_apply(L, L_local, row_offset, g, diag_scale):
    """y[i] = diag_scale d(gi) x[i] - g sum_{j < L_local} x[i ^ (1 << j)]   (include/dsea.h dsea_op_create_tfim)"""
    d = tfim_diag(L, row_offset, 1 << L_local)

    def apply(x, dtype):
        xd = np.asarray(x, dtype=dtype)
        dd = dtype(diag_scale) * d.astype(dtype)
        ax = dd * xd - dtype(g) * flip_sum(xd, L_local)
        x64 = np.abs(np.asarray(x, dtype=np.float64))            # (the scale of a bound: fp64 is plenty)
        return ax, np.abs(dd.astype(np.float64)) * x64 + abs(g) * flip_sum(x64, L_local)

    return apply


# ---- XYZ spins: the chain and the bond list ------------------------------------------------------------------------------
def xor_gather(x, mask):
    """x[s ^ mask] for every row s: one block swap per set bit of the mask (as ``flip_sum``; no index array)"""
    j = 0
    while mask >> j:
        if (mask >> j) & 1:
            x = x.reshape(-1, 2, 1 << j)[:, ::-1, :].reshape(-1)
        j += 1
    return x


def site_bits(L):
    """bits[i][s] = bit i of the row index s, as int8"""
    s = np.arange(1 << L, dtype=np.int64)
    return [((s >> i) & 1).astype(np.int8) for i in range(L)]


def lattice_apply(L, bonds, p):
    """y[s] = (sum_t Jz_t zz_t + sum_i hz_i z_i) x[s] + sum_i hx_i x[s ^ (1 << i)] + sum_t (Jx_t - Jy_t zz_t) x[s ^ m_t]
    (include/dsea.h dsea_op_create_lattice; p = [Jx(nb), Jy(nb), Jz(nb), hx(L), hz(L)]).  The magnitude of an off-diagonal
    coefficient is |Jx_t| + |Jy_t|.  Vectorised over the rows: a term costs a few passes over the vector."""
    nb = len(bonds)
    p = np.asarray(p, dtype=np.float64).reshape(3 * nb + 2 * L)
    jx, jy, jz, hx, hz = p[:nb], p[nb:2 * nb], p[2 * nb:3 * nb], p[3 * nb:3 * nb + L], p[3 * nb + L:]
    bits = site_bits(L)

    def apply(x, dtype):
        xd = np.asarray(x, dtype=dtype)
        x64 = np.abs(np.asarray(x, dtype=np.float64))
        diag = np.zeros(1 << L, dtype=dtype)
        ax = np.zeros(1 << L, dtype=dtype)
        sc = (np.sum(np.abs(jz)) + np.sum(np.abs(hz))) * x64
        for i in range(L):
            diag += dtype(hz[i]) * (1 - 2 * bits[i]).astype(dtype)
            ax += dtype(hx[i]) * xor_gather(xd, 1 << i)
            sc += abs(hx[i]) * xor_gather(x64, 1 << i)
        for t, (a, b) in enumerate(bonds):
            zz = (1 - 2 * (bits[a] ^ bits[b])).astype(dtype)
            m = (1 << a) | (1 << b)
            diag += dtype(jz[t]) * zz
            ax += (dtype(jx[t]) - dtype(jy[t]) * zz) * xor_gather(xd, m)
            sc += (abs(jx[t]) + abs(jy[t])) * xor_gather(x64, m)
        return ax + diag * xd, sc

    return apply


def chain_bonds(L):
    """bond b joins sites b and (b + 1) mod L (at L = 2 both bonds join sites 0 and 1, and both count)"""
    return [(b, (b + 1) % L) for b in range(L)]


def chain_apply(L, c):
    """the periodic chain of include/dsea.h dsea_op_create_chain, couplings (5, L) in rows Jx, Jy, Jz, hx, hz: the bond list
    operator on ``chain_bonds``"""
    c = np.asarray(c, dtype=np.float64).reshape(5, L)
    return lattice_apply(L, chain_bonds(L), np.concatenate((c[0], c[1], c[2], c[3], c[4])))


# ---- CSR / SELL --------------------------------------------------------------------------------------------------------
def row_sums(rowptr, terms):
    """sum of each row's terms, in the order they are stored (empty rows: 0)"""
    out = np.zeros(rowptr.size - 1, dtype=terms.dtype)
    lens = np.diff(rowptr)
    nz = lens > 0
    if terms.size:
        out[nz] = np.add.reduceat(terms, rowptr[:-1][nz])
    return out


def csr_apply(rowptr, colidx, vals, gather=None):
    """A x with x[col] taken by ``gather(x, colidx)`` (default x[colidx]: the slab modes read it elsewhere)"""
    take = gather or (lambda x, c: x[c])

    def apply(x, dtype):
        xg = take(np.asarray(x, dtype=dtype), colidx)
        return row_sums(rowptr, vals.astype(dtype) * xg), row_sums(rowptr, np.abs(vals) * np.abs(xg.astype(np.float64)))

    return apply


def csr_pattern(lens, seed, band=None):
    """(rowptr, colidx) with the given row lengths; columns uniform over the rows, or within ``band`` of the own row
    (repeated columns are legal CSR: their products add up)"""
    lens = np.asarray(lens, dtype=np.int64)
    n = lens.size
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(lens)
    rng = np.random.default_rng(seed)
    nnz = int(rowptr[-1])
    if band is None:
        cols = rng.integers(0, n, size=nnz)
    else:
        rows = np.repeat(np.arange(n, dtype=np.int64), lens)
        cols = np.clip(rows + rng.integers(-band, band + 1, size=nnz), 0, n - 1)
    return rowptr, cols.astype(np.int32)


def csr_values(nnz, seed, exact):
    return eighths(nnz, seed) if exact else table_values(nnz, seed)


@functools.lru_cache(maxsize=None)
def csr_case(name):
    """named CSR patterns: (rowptr, colidx, n, most terms of a row).  Empty rows include the first and the last."""
    rng = np.random.default_rng(sum(map(ord, name)))

    def ragged(n, hi):
        lens = rng.integers(0, hi + 1, size=n)
        lens[[0, -1]] = 0
        lens[rng.integers(0, n, size=max(n // 8, 1))] = 0
        return lens

    if name.startswith("avg6-"):          # automatic G = 0: 4 <= average <= 48 -> the streaming kernel
        n = int(name[5:])
        lens = ragged(n, 14) if n > 1 else np.array([6])
        if n > 1:
            lens[1] += max(0, 5 * n - int(lens.sum()))       # (keep the average above 4 whatever the draw)
    elif name.startswith("avg2-"):        # average below 4 -> the group kernel at G = 4
        n = int(name[5:])
        lens = ragged(n, 4)
    elif name == "avg60-129":             # average above 48 -> the group kernel, automatic G = 64
        lens = ragged(129, 140)
        lens[1] += max(0, 60 * 129 - int(lens.sum()))
    elif name == "group-stride":          # G = 64: 4 rows per block, 2048 blocks -> 8192 rows per trip, 5 rows in the second
        lens = ragged(8192 + 5, 6)
    elif name == "stream-trips":          # 4098 chunks of 128 rows > 4096 blocks; exactly 4 per row (average 4.0: streaming)
        lens = np.full(CSR_ROWS * MAX_TFIM_BLOCKS + 129, 4)
    elif name == "long-rows":             # chunk 1 holds 3 x 2100 + ... > CSR_CAP products, the average stays below 48
        lens = np.full(2303, 4)
        lens[[130, 131, 200]] = 2100
        lens[[0, 1000, -1]] = 0
    else:
        raise KeyError(name)
    rowptr, cols = csr_pattern(lens, 17 + len(name))
    for a in (rowptr, cols):
        a.setflags(write=False)
    return rowptr, cols, int(lens.size), int(max(lens.max(), 1))


def csr_takes_stream(rowptr, group):
    """launch_spmv: the streaming kernel serves automatic tuning when 4 <= nnz / n and nnz / n * 128 <= 6144"""
    n = rowptr.size - 1
    avg = float(rowptr[-1]) / n
    return group == 0 and avg >= 4.0 and avg * CSR_ROWS <= CSR_CAP


def csr_chunk_sizes(rowptr):
    n = rowptr.size - 1
    edges = np.minimum(np.arange(0, n + CSR_ROWS, CSR_ROWS), n)
    return np.diff(rowptr[edges])


def sell_widths(nslices):
    if nslices > 1000:
        return [SMALL_WIDTHS[s % len(SMALL_WIDTHS)] for s in range(nslices)]
    start = {1: 8, 5: 4}.get(nslices, 0)
    return [WIDTHS[(s + start) % len(WIDTHS)] for s in range(nslices)]


@functools.lru_cache(maxsize=None)
def sell_case(nslices, row_sum=None):
    """ragged SELL pattern of ``nslices`` 64-row slices, n no multiple of 64: slice s has ONE heavy row of sell_widths(s)
    entries (at a lane that moves with s), the other rows up to 3.  Columns stay within 300 of the own row (16-bit deltas).
    Returns (rowptr, colidx, n, m)."""
    n = 37 if nslices == 1 else 64 * nslices - 27
    widths = sell_widths(nslices)
    rng = np.random.default_rng(1000 + nslices)
    lens = np.zeros(n, dtype=np.int64)
    for s, w in enumerate(widths):
        r0, r1 = 64 * s, min(64 * s + 64, n)
        lens[r0:r1] = rng.integers(0, min(w, 3) + 1, size=r1 - r0)
        lens[r0 + (7 * s + 3) % (r1 - r0)] = w
    rowptr, cols = csr_pattern(lens, 2000 + nslices, band=300)
    for a in (rowptr, cols):
        a.setflags(write=False)
    return rowptr, cols, n, int(max(lens.max(), 1))


def slab_pattern(nslices, hb, lo, hi):
    """the ragged pattern with LOCAL columns in [-hb, n + hb) (include/dsea.h dsea_op_set_slab); a missing neighbour's side
    holds no column"""
    rowptr, _, n, m = sell_case(nslices)
    lens = np.diff(rowptr)
    lens[:3] = lens[-3:] = 5                      # (the first and the last slice of the ragged pattern are empty)
    rowptr = np.concatenate(([0], np.cumsum(lens)))
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    cols = rows + np.random.default_rng(50 + hb).integers(-hb, hb + 1, size=rows.size)
    cols = np.clip(cols, -hb if lo else 0, n + hb - 1 if hi else n - 1)
    if lo:
        assert cols.min() < 0
    if hi:
        assert cols.max() >= n
    return rowptr, cols.astype(np.int32), n, m


def sell_slice_widths(rowptr, n, pad=1):
    """widths of the SELL-64 slices of a CSR pattern, padded to multiples of ``pad`` (2: sell16p2, 4: sell16v8)"""
    nsl = (n + 63) // 64
    lens = np.zeros(nsl * 64, dtype=np.int64)
    lens[:n] = np.diff(rowptr)
    w = lens.reshape(nsl, 64).max(axis=1)
    return (w + pad - 1) // pad * pad


def constant_row_sum_values(rowptr, c, seed):
    """integer values with every non-empty row summing to c (A 1 = c 1 needs no empty row): random integers in [-3, 3], the
    last entry of a row takes the remainder"""
    vals = np.random.default_rng(seed).integers(-3, 4, size=int(rowptr[-1])).astype(np.float64)
    lens = np.diff(rowptr)
    assert lens.min() >= 1
    last = rowptr[1:] - 1
    vals[last] = 0.0
    vals[last] = c - row_sums(rowptr, vals)
    return vals


# ---- stencil, symmetric dense ------------------------------------------------------------------------------------------
def stencil_apply(coef, V, lo=None, hi=None):
    """y[i] = coef ((-2 x[i] + x[i+1]) + x[i-1]) + V[i] x[i], x[-1] = lo, x[n] = hi (None: 0)"""
    def apply(x, dtype):
        xd = np.asarray(x, dtype=dtype)
        up = np.concatenate((xd[1:], [dtype(hi or 0.0)]))
        dn = np.concatenate(([dtype(lo or 0.0)], xd[:-1]))
        ax = dtype(coef) * ((dtype(-2) * xd + up) + dn) + V.astype(dtype) * xd
        a64 = np.abs(np.asarray(x, dtype=np.float64))
        up64 = np.concatenate((a64[1:], [abs(hi or 0.0)]))
        dn64 = np.concatenate(([abs(lo or 0.0)], a64[:-1]))
        return ax, abs(coef) * (2 * a64 + up64 + dn64) + np.abs(V) * a64

    return apply


def symmetric_from_upper(A):
    """the symmetric matrix whose upper triangle is that of A (whatever the lower triangle holds)"""
    up = np.triu(A)
    return up + np.triu(A, 1).T


def dense_apply(S):
    def apply(x, dtype):
        return S.astype(dtype) @ np.asarray(x, dtype=dtype), np.abs(S) @ np.abs(np.asarray(x, dtype=np.float64))

    return apply


def symdense_storage(n, lda, seed, exact):
    """(storage [n, lda] fp64 with NaN in the lower triangle and in the padding columns, the symmetric matrix it means).
    Every entry is representable in fp32."""
    vals = eighths((n, n), seed) if exact else table_values(n * n, seed).reshape(n, n).astype(np.float32).astype(np.float64)
    S = symmetric_from_upper(vals)
    store = np.full((n, lda), np.nan)
    iu = np.triu_indices(n)
    store[iu] = S[iu]
    return store, S


# ---- fused Lanczos tails: three steps judged by their own outputs ------------------------------------------------------
def lanczos_relations(apply, m, q0, Q, alphas, betas):
    """dsea_lanczos_run_basisfree with k = 3: Q = (q0n, q1, q2), alphas[3], betas[2], all from the device.  Returns the worst
    error / bound of each relation (every bound follows from the operation count; u = 2^-53):
        three-term 0   |A q0n - a0 q0n - b0 q1|            <= (m + 8) u (|A||q0n| + |a0 q0n| + |b0 q1|)
        three-term 1   |A q1 - a1 q1 - b0 q0n - b1 q2|     <= (m + 8) u (|A||q1| + |a1 q1| + |b0 q0n| + |b1 q2|)
        alpha j        |a_j - q_j.(A q_j)|                 <= (n + m + 4) u sum |q_j| |A||q_j|
        norm j         | ||q_j|| - 1 |                     <= (n + 6) u
        start          |q0n ||q0|| - q0|                   <= (n + 6) u |q0|"""
    n = Q.shape[1]
    q = [np.asarray(Q[j], dtype=LD) for j in range(3)]
    a = [LD(v) for v in alphas]
    b = [LD(v) for v in betas]
    Aq, sc = zip(*(apply(Q[j], LD) for j in range(3)))
    out = {}
    r0 = Aq[0] - a[0] * q[0] - b[0] * q[1]
    out["three-term 0"] = worst_ratio(np.abs(r0), (m + 8) * U * (sc[0] + np.abs(a[0] * q[0]) + np.abs(b[0] * q[1])))
    r1 = Aq[1] - a[1] * q[1] - b[0] * q[0] - b[1] * q[2]
    out["three-term 1"] = worst_ratio(np.abs(r1), (m + 8) * U * (sc[1] + np.abs(a[1] * q[1]) + np.abs(b[0] * q[0])
                                                                 + np.abs(b[1] * q[2])))
    for j in range(3):
        out["alpha %d" % j] = worst_ratio(abs(a[j] - np.sum(q[j] * Aq[j])), dot_bound(n, m, Q[j], sc[j]))
        out["norm %d" % j] = worst_ratio(abs(np.sqrt(np.sum(q[j] * q[j])) - 1), (n + 6) * U)
    q0 = np.asarray(q0, dtype=LD)
    out["start"] = worst_ratio(np.abs(q[0] * np.sqrt(np.sum(q0 * q0)) - q0), (n + 6) * U * np.abs(q0))
    return out


def host_lanczos3(apply, q0, order=None):
    """the same three steps in fp64 numpy (sums taken in ``order``, a permutation, or as stored): what the CPU test feeds
    ``lanczos_relations`` to show that the bounds hold for an honest fp64 evaluation"""
    def dot(x, y):
        p = x * y
        return float(np.sum(p if order is None else p[order]))

    q = [q0 / np.sqrt(dot(q0, q0))]
    alphas, betas = [], []
    prev, beta = None, 0.0
    for j in range(3):
        u = apply(q[j], np.float64)[0]
        alphas.append(dot(q[j], u))
        if j == 2:
            break
        r = u - alphas[j] * q[j] - (beta * prev if prev is not None else 0.0)
        beta = np.sqrt(dot(r, r))
        betas.append(beta)
        prev = q[j]
        q.append(r / beta)
    return np.stack(q), alphas, betas
