"""numpy reference of the XXZ spins in a lattice-symmetry sector (docs/design/20-symmetry-sector.md); no GPU, no torch.  Two
independent routes:

  (a) dense: the columns of B, |r> = (|G| sigma_r)^(-1/2) sum_g chi(g) |g s_r>, in the row order of sector_reference, and
      B^T H B on top of sector_reference.dense -- small cases only;
  (b) the vectorised representative-only row formula ``apply`` and the sums ``forms`` -- also the L = 22 cases.

``generators`` is a list of (perm, char): g(s) has bit perm[i] set iff s has bit i; ``p`` is the flat parameter
[Jxy(nb), Jz(nb), hz(L)] of sector_reference.

    close_group(L, generators)              the closed group, identity first, breadth-first
    orbit_ids(L, bonds, group)              orbit id per parameter
    symmetrise_matrix / symmetrise          S and S p (orbit means, ascending index order)
    basis(L, ndown, group)                  Basis: reps, sigma, bucket, and the counts the tests pin
    apply(case, p, x) / forms(case, v1, v2) route (b); ``case`` = Case(L, ndown, bonds, generators)
    dense_B(case) / dense_sym(case, p)      route (a)
"""
import functools

import numpy as np

import sector_reference as sec


def ring(L, d=1):
    return [(i, (i + d) % L) for i in range(L)]


def square(Lx, Ly):
    out = []
    for y in range(Ly):
        for x in range(Lx):
            out.append((y * Lx + x, y * Lx + (x + 1) % Lx))
            out.append((y * Lx + x, ((y + 1) % Ly) * Lx + x))
    return out


def translation(L):
    return tuple((i + 1) % L for i in range(L))


def reflection(L):
    return tuple(L - 1 - i for i in range(L))


def torus_tx(Lx, Ly):
    return tuple(y * Lx + (x + 1) % Lx for y in range(Ly) for x in range(Lx))


def torus_ty(Lx, Ly):
    return tuple(((y + 1) % Ly) * Lx + x for y in range(Ly) for x in range(Lx))


def square_rot(Lq):
    """the rotation (x, y) -> (Lq - 1 - y, x) of an Lq x Lq torus"""
    return tuple((i % Lq) * Lq + (Lq - 1 - i // Lq) for i in range(Lq * Lq))


def square_mirror(Lq):
    """(x, y) -> (Lq - 1 - x, y)"""
    return tuple((i // Lq) * Lq + (Lq - 1 - i % Lq) for i in range(Lq * Lq))


def close_group(L, generators):
    gens = [(tuple(int(v) for v in perm), int(char)) for perm, char in generators]
    ident = tuple(range(L))
    chars = {ident: 1}
    order, frontier = [ident], [ident]
    while frontier:
        new = []
        for p in frontier:
            for q, d in gens:
                r = tuple(q[p[i]] for i in range(L))
                e = chars[p] * d
                if r not in chars:
                    chars[r] = e
                    order.append(r)
                    new.append(r)
                else:
                    assert chars[r] == e, "inconsistent character"
        frontier = new
    return tuple((p, chars[p]) for p in order)


def orbit_ids(L, bonds, group):
    """orbit id per parameter, numbered by first appearance inside each family (Jxy, Jz, hz)"""
    index = {frozenset(b): t for t, b in enumerate(bonds)}
    assert len(index) == len(bonds), "repeated bond"
    low_b = [min(index[frozenset((perm[a], perm[b]))] for perm, _ in group) for a, b in bonds]
    low_s = [min(perm[i] for perm, _ in group) for i in range(L)]

    def number(low):
        ids = {}
        return [ids.setdefault(v, len(ids)) for v in low]

    ob, os_ = number(low_b), number(low_s)
    nob = max(ob) + 1
    return ob + [nob + v for v in ob] + [2 * nob + v for v in os_]


def symmetrise_matrix(orbits):
    orbits = np.asarray(orbits)
    same = (orbits[:, None] == orbits[None, :]).astype(np.float64)
    return same / same.sum(axis=1, keepdims=True)


def symmetrise(orbits, p):
    """S p, each mean summed in ascending index order"""
    p = np.asarray(p, dtype=np.float64)
    out = np.empty_like(p)
    for c, o in enumerate(orbits):
        members = [m for m, om in enumerate(orbits) if om == o]
        total = 0.0
        for m in members:
            total += p[m]
        out[c] = total / len(members)
    return out


def slice_tables(L, group):
    """tab[g, sl, byte] = the image under g of the state whose byte slice sl is ``byte``: the perm_tab of the library"""
    nsl = (L + 7) // 8
    tab = np.zeros((len(group), nsl, 256), dtype=np.int64)
    for g, (perm, _) in enumerate(group):
        for sl in range(nsl):
            for byte in range(256):
                v = 0
                for bit in range(8):
                    i = sl * 8 + bit
                    if i < L and (byte >> bit) & 1:
                        v |= 1 << perm[i]
                tab[g, sl, byte] = v
    return tab


def images(tab, s):
    """(|G|, len(s)) int64: g(s) for every g"""
    s = np.asarray(s, dtype=np.int64)
    out = np.zeros((tab.shape[0], s.size), dtype=np.int64)
    for sl in range(tab.shape[1]):
        out |= tab[:, sl, :][:, (s >> (8 * sl)) & 255]
    return out


class Basis:
    def __init__(self, L, ndown, group):
        self.L, self.ndown, self.group = L, ndown, group
        self.tab = slice_tables(L, group)
        self.chars = np.array([c for _, c in group], dtype=np.int64)
        words = np.array(sec.states(L, ndown), dtype=np.int64)
        smallest = np.ones(words.size, dtype=bool)
        sigma = np.zeros(words.size, dtype=np.int64)
        step = 1 << 16
        for lo in range(0, words.size, step):
            w = words[lo:lo + step]
            im = images(self.tab, w)
            smallest[lo:lo + step] = (im >= w[None, :]).all(axis=0)
            sigma[lo:lo + step] = ((im == w[None, :]) * self.chars[:, None]).sum(axis=0)
        assert ((sigma == 0) | (sigma > 0)).all()
        self.n_sector = words.size
        self.orbits = int(smallest.sum())
        keep = smallest & (sigma != 0)
        self.reps = words[keep]
        self.sigma = sigma[keep]
        self.n = int(keep.sum())
        self.zero_norm = self.orbits - self.n
        self.nontrivial = int((self.sigma > 1).sum())
        Llo = (L + 1) // 2
        self.bucket = np.searchsorted(self.reps >> Llo, np.arange((1 << (L - Llo)) + 1), side="left").astype(np.int64)
        for a in (self.reps, self.sigma, self.bucket):
            a.setflags(write=False)

    def row_of(self, s):
        s = np.asarray(s, dtype=np.int64)
        pos = np.minimum(np.searchsorted(self.reps, s), self.n - 1)
        return np.where(self.reps[pos] == s, pos, -1)


@functools.lru_cache(maxsize=None)
def basis(L, ndown, group):
    return Basis(L, ndown, group)


class Case:
    """one (L, ndown, bonds, generators): group, orbit ids, basis and the hop lists of route (b), computed once"""

    def __init__(self, L, ndown, bonds, generators):
        self.L, self.ndown = L, ndown
        self.bonds = tuple((int(a), int(b)) for a, b in bonds)
        self.nb = len(self.bonds)
        self.group = close_group(L, generators)
        self.orbit = tuple(orbit_ids(L, self.bonds, self.group))
        self.basis = basis(L, ndown, self.group)
        b = self.basis
        s = b.reps
        self.z = [1.0 - 2.0 * ((s >> i) & 1) for i in range(L)]
        self.hops = []
        self.n_hops = self.n_dead = 0
        sg = b.sigma.astype(np.float64)
        for a, c in self.bonds:
            differ = ((s >> a) ^ (s >> c)) & 1 == 1
            rows = np.nonzero(differ)[0]
            im = images(b.tab, s[rows] ^ ((1 << a) | (1 << c)))
            best = im.min(axis=0)
            which = im.argmin(axis=0)
            cols = b.row_of(best)
            keep = cols >= 0
            self.n_hops += rows.size
            self.n_dead += int((~keep).sum())
            rows, cols, which = rows[keep], cols[keep], which[keep]
            coef = 2.0 * b.chars[which] * np.sqrt(sg[cols] / sg[rows])
            self.hops.append((rows, cols, coef, np.where(differ, -1.0, 1.0)))

    def pbar(self, p):
        return symmetrise(self.orbit, p)


def apply(case, p, x):
    """route (b): the representative-only row formula on the orbit means of p"""
    jxy, jz, hz = sec.split(case.L, case.bonds, case.pbar(p))
    x = np.asarray(x, dtype=np.float64)
    diag = np.zeros(x.size)
    y = np.zeros(x.size)
    for i, z in enumerate(case.z):
        diag += hz[i] * z
    for t, (rows, cols, coef, zz) in enumerate(case.hops):
        diag += jz[t] * zz
        np.add.at(y, rows, jxy[t] * coef * x[cols])
    return y + diag * x


def raw_forms(case, v1, v2):
    v1, v2 = np.asarray(v1, dtype=np.float64), np.asarray(v2, dtype=np.float64)
    nb = case.nb
    out = np.zeros(2 * nb + case.L)
    for t, (rows, cols, coef, zz) in enumerate(case.hops):
        out[t] = np.sum(coef * v1[rows] * v2[cols])
        out[nb + t] = np.sum(zz * v1 * v2)
    for i, z in enumerate(case.z):
        out[2 * nb + i] = np.sum(z * v1 * v2)
    return out


def forms(case, v1, v2):
    """out = S raw"""
    return symmetrise(case.orbit, raw_forms(case, v1, v2))


def dense_B(case):
    """route (a): the n_sector x n_rep matrix of the basis vectors, built state by state from the permutations themselves"""
    L, b = case.L, case.basis
    rank = sec.rank(L, case.ndown)
    B = np.zeros((b.n_sector, b.n))
    for j, (s, sg) in enumerate(zip(b.reps.tolist(), b.sigma.tolist())):
        for perm, c in case.group:
            t = 0
            for i in range(L):
                if (s >> i) & 1:
                    t |= 1 << perm[i]
            B[rank[t], j] += c
        B[:, j] /= np.sqrt(len(case.group) * sg)
    return B


def dense_sym(case, p, symmetrised=True):
    """route (a): B^T H_sector(S p) B (or B^T H_sector(p) B)"""
    B = dense_B(case)
    H = sec.dense(case.L, case.ndown, case.bonds, case.pbar(p) if symmetrised else p)
    return B.T @ H @ B


def _ring_case(L, ndown, char_t, parity=None, second=False):
    gens = [(translation(L), char_t)] + ([(reflection(L), parity)] if parity is not None else [])
    return L, ndown, tuple(ring(L) + (ring(L, 2) if second else [])), tuple(gens)


# name -> ((L, ndown, bonds, generators), (|G|, n_sector, orbits, n_rep, orbits with sigma = 0, rows with sigma > 1))
TABLE = {
    "ring8-k0": (_ring_case(8, 4, 1), (8, 70, 10, 10, 0, 2)),
    "ring8-kpi-p+1-j1j2": (_ring_case(8, 4, -1, 1, second=True), (16, 70, 8, 5, 3, 3)),
    "ring8-k0-p-1": (_ring_case(8, 4, 1, -1), (16, 70, 8, 2, 6, 0)),
    "ring7-k0": (_ring_case(7, 3, 1), (7, 35, 5, 5, 0, 0)),
    "ring12-kpi-p-1": (_ring_case(12, 6, -1, -1), (24, 924, 50, 40, 10, 11)),
    "torus4x4-00": ((16, 8, tuple(square(4, 4)), ((torus_tx(4, 4), 1), (torus_ty(4, 4), 1))), (16, 12870, 822, 822, 0, 30)),
    "torus4x4-c4": ((16, 8, tuple(square(4, 4)), ((torus_tx(4, 4), 1), (torus_ty(4, 4), 1), (square_rot(4), -1))),
                    (64, 12870, 231, 225, 6, 45)),
    "torus4x4-pipi-nd7": ((16, 7, tuple(square(4, 4)), ((torus_tx(4, 4), -1), (torus_ty(4, 4), -1))),
                          (16, 11440, 715, 715, 0, 0)),
    "ring22-k0": (_ring_case(22, 11, 1), (22, 705432, 32066, 32066, 0, 1)),
    "ring22-k0-p-1": (_ring_case(22, 11, 1, -1), (44, 705432, 16159, 15907, 252, 0)),
}
# hops of all rows, and those that land on an orbit with sigma = 0 and are dropped
HOPS = {"ring12-kpi-p-1": (270, 30), "torus4x4-c4": (3844, 19)}


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(*TABLE[name][0])
