"""numpy reference of the XXZ spins in a symmetry sector whose group elements may carry the global spin flip
(docs/design/23-spin-inversion.md); no GPU, no torch.  Written from the definitions of that note on top of sector_reference and the
permutation builders of symsector_reference.

A generator is (perm, char) or (perm, char, flip); a group element acts as g(s) = perm(s) ^ (flip ? 2^L - 1 : 0), composition
multiplies the characters and XORs the flips.  ``p`` is the flat parameter [Jxy(nb), Jz(nb), hz(L)] of sector_reference.

    close_group(L, generators)              the closed group as (perm, char, flip) triples, identity first, breadth-first
    images(tab, flips, L, s)                g(s) for every g
    site_signs(L, group)                    eps_i in {+1, -1, 0}
    symmetrise_matrix(L, nb, orbits, group) S from its definition (a sum over the group), signed for hz
    symmetrise(orbits, eps, nb, p)          S p by orbit sums in ascending index order (the order of the kernels)
    basis(L, ndown, group)                  Basis: reps, sigma, bucket and the counts the tests pin
    Case(L, ndown, bonds, generators)       group, orbit ids, signs, basis and hop lists; apply / raw_forms / forms / dense_B
"""
import functools

import numpy as np

import sector_reference as sec
import symsector_reference as sym


def flip_generator(L, char):
    return (tuple(range(L)), int(char), True)


def close_group(L, generators):
    gens = []
    for gen in generators:
        perm, char = gen[0], gen[1]
        flip = bool(gen[2]) if len(gen) == 3 else False
        gens.append((tuple(int(v) for v in perm), int(char), flip))
    ident = (tuple(range(L)), False)
    chars = {ident: 1}
    order, frontier = [ident], [ident]
    while frontier:
        new = []
        for p, fp in frontier:
            for q, d, fq in gens:
                r = (tuple(q[p[i]] for i in range(L)), fp != fq)
                e = chars[(p, fp)] * d
                if r not in chars:
                    chars[r] = e
                    order.append(r)
                    new.append(r)
                else:
                    assert chars[r] == e, "inconsistent character"
        frontier = new
    return tuple((p, chars[(p, f)], f) for p, f in order)


def images(tab, flips, L, s):
    """(|G|, len(s)) int64: g(s) = perm_g(s) ^ (flip_g ? full : 0)"""
    full = (1 << L) - 1
    return sym.images(tab, s) ^ (np.asarray(flips, dtype=np.int64)[:, None] * full)


def site_signs(L, group):
    """eps_i: 0 on every orbit one of whose sites is fixed by a flipped element; otherwise +1 on the orbit's lowest site i0 and
    sgn(g) on perm_g[i0]"""
    low = [min(perm[i] for perm, _, _ in group) for i in range(L)]
    dead = set()
    for perm, _, flip in group:
        if flip:
            dead.update(low[i] for i in range(L) if perm[i] == i)
    eps = [0] * L
    for i0 in range(L):
        if low[i0] != i0 or i0 in dead:
            continue
        for perm, _, flip in group:
            sign = -1 if flip else 1
            assert eps[perm[i0]] in (0, sign), "the relative sign must not depend on the path"
            eps[perm[i0]] = sign
    return tuple(eps)


def symmetrise_matrix(L, nb, bonds, group):
    """S from its definition: (S p)_j = (1 / |G|) sum_g sgn(g) p_{g^-1(j)} with sgn(g) = -1 only for hz under a flipped g"""
    index = {frozenset(b): t for t, b in enumerate(bonds)}
    S = np.zeros((2 * nb + L, 2 * nb + L))
    for perm, _, flip in group:
        for t, (a, b) in enumerate(bonds):
            image = index[frozenset((perm[a], perm[b]))]
            S[image, t] += 1.0
            S[nb + image, nb + t] += 1.0
        for i in range(L):
            S[2 * nb + perm[i], 2 * nb + i] += -1.0 if flip else 1.0
    return S / len(group)


def symmetrise(orbits, eps, nb, p):
    """S p by orbits: the mean in ascending index order, for hz the mean of eps_j p_j times eps_i"""
    p = np.asarray(p, dtype=np.float64)
    out = np.empty_like(p)
    sign = [1.0] * (2 * nb) + [float(e) for e in eps]
    for c, o in enumerate(orbits):
        members = [m for m, om in enumerate(orbits) if om == o]
        total = 0.0
        for m in members:
            total += sign[m] * p[m]
        out[c] = sign[c] * (total / len(members))
    return out


class Basis:
    def __init__(self, L, ndown, group):
        self.L, self.ndown, self.group = L, ndown, group
        self.tab = sym.slice_tables(L, [(perm, char) for perm, char, _ in group])
        self.chars = np.array([c for _, c, _ in group], dtype=np.int64)
        self.flips = np.array([int(f) for _, _, f in group], dtype=np.int64)
        assert not self.flips.any() or 2 * ndown == L
        words = np.array(sec.states(L, ndown), dtype=np.int64)
        smallest = np.ones(words.size, dtype=bool)
        sigma = np.zeros(words.size, dtype=np.int64)
        step = 1 << 16
        for lo in range(0, words.size, step):
            w = words[lo:lo + step]
            im = images(self.tab, self.flips, L, w)
            smallest[lo:lo + step] = (im >= w[None, :]).all(axis=0)
            sigma[lo:lo + step] = ((im == w[None, :]) * self.chars[:, None]).sum(axis=0)
        assert (sigma >= 0).all()
        self.n_sector = words.size
        self.orbits = int(smallest.sum())
        keep = smallest & (sigma != 0)
        self.reps = words[keep]
        self.sigma = sigma[keep]
        self.n = int(keep.sum())
        self.zero_norm = self.orbits - self.n
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
    """one (L, ndown, bonds, generators): the group as (perm, char) pairs plus ``flips``, orbit ids, site signs, basis and the hop
    lists of the row formula, computed once.  It has the attributes symsector_reference.apply and raw_forms read."""

    def __init__(self, L, ndown, bonds, generators):
        self.L, self.ndown = L, ndown
        self.bonds = tuple((int(a), int(b)) for a, b in bonds)
        self.nb = len(self.bonds)
        self.elements = close_group(L, generators)
        self.group = tuple((perm, char) for perm, char, _ in self.elements)
        self.flips = tuple(flip for _, _, flip in self.elements)
        self.orbit = tuple(sym.orbit_ids(L, self.bonds, self.group))
        self.eps = site_signs(L, self.elements)
        self.basis = basis(L, ndown, self.elements)
        b = self.basis
        s = b.reps
        self.z = [1.0 - 2.0 * ((s >> i) & 1) for i in range(L)]
        self.hops = []
        sg = b.sigma.astype(np.float64)
        for a, c in self.bonds:
            differ = ((s >> a) ^ (s >> c)) & 1 == 1
            rows = np.nonzero(differ)[0]
            im = images(b.tab, b.flips, L, s[rows] ^ ((1 << a) | (1 << c)))
            best = im.min(axis=0)
            which = im.argmin(axis=0)
            cols = b.row_of(best)
            keep = cols >= 0
            rows, cols, which = rows[keep], cols[keep], which[keep]
            coef = 2.0 * b.chars[which] * np.sqrt(sg[cols] / sg[rows])
            self.hops.append((rows, cols, coef, np.where(differ, -1.0, 1.0)))

    def pbar(self, p):
        return symmetrise(self.orbit, self.eps, self.nb, p)

    def S(self):
        return symmetrise_matrix(self.L, self.nb, self.bonds, self.elements)


apply = sym.apply            # the row formula on case.pbar(p): the flip enters through the basis, the hops and the signed mean
raw_forms = sym.raw_forms


def forms(case, v1, v2):
    """out = S raw"""
    return case.pbar(raw_forms(case, v1, v2))


def dense_B(case):
    """the n_sector x n matrix of |r> = (|G| sigma_r)^(-1/2) sum_g chi(g) |g s_r>, state by state from the definition of g"""
    L, b = case.L, case.basis
    full = (1 << L) - 1
    rank = sec.rank(L, case.ndown)
    B = np.zeros((b.n_sector, b.n))
    for j, (s, sg) in enumerate(zip(b.reps.tolist(), b.sigma.tolist())):
        for perm, c, flip in case.elements:
            t = 0
            for i in range(L):
                if (s >> i) & 1:
                    t |= 1 << perm[i]
            B[rank[t ^ full if flip else t], j] += c
        B[:, j] /= np.sqrt(len(case.elements) * sg)
    return B


def dense_sym(case, p):
    """B^T H_sector(p) B, the couplings as they are"""
    B = dense_B(case)
    return B.T @ sec.dense(case.L, case.ndown, case.bonds, p) @ B


def _ring(L, ndown, gens, second=False):
    return L, ndown, tuple(sym.ring(L) + (sym.ring(L, 2) if second else [])), tuple(gens)


def _complete(L):
    return tuple((i, j) for i in range(L) for j in range(i + 1, L))


def geometry(name, z):
    """(L, ndown, bonds, generators) of a row of TABLE with the character z = +1 / -1 on the flipped generator"""
    T, R = sym.translation, sym.reflection
    if name == "flip-L8":
        return _ring(8, 4, [flip_generator(8, z)])
    if name == "ring8":
        return _ring(8, 4, [(T(8), 1), (R(8), 1), flip_generator(8, z)])
    if name == "ring12-j1j2":
        return _ring(12, 6, [(T(12), -1), (R(12), -1), flip_generator(12, z)], second=True)
    if name == "ring10-TF":
        return _ring(10, 5, [(T(10), z, True)])
    if name == "ring14-TF":
        return _ring(14, 7, [(T(14), z, True)])
    if name == "K16-D16":
        return 16, 8, _complete(16), ((T(16), 1), (R(16), -1), flip_generator(16, z))
    if name == "torus4x4-c4":
        return 16, 8, tuple(sym.square(4, 4)), ((sym.torus_tx(4, 4), 1), (sym.torus_ty(4, 4), 1), (sym.square_rot(4), 1),
                                                flip_generator(16, z))
    if name == "ring20":
        return _ring(20, 10, [(T(20), 1), (R(20), 1), flip_generator(20, z)])
    raise KeyError(name)


# name -> (|G|, n_sector, orbits, (sigma = 0 orbits at z = +1, at z = -1), (n at z = +1, at z = -1))
TABLE = {
    "flip-L8": (2, 70, 35, (0, 0), (35, 35)),
    "ring8": (32, 70, 7, (0, 6), (7, 1)),
    "ring12-j1j2": (48, 924, 35, (22, 8), (13, 27)),
    "ring10-TF": (10, 252, 30, (0, 8), (30, 22)),
    "ring14-TF": (14, 3432, 256, (0, 20), (256, 236)),
    "K16-D16": (64, 12870, 257, (99, 45), (158, 212)),
    "torus4x4-c4": (128, 12870, 149, (0, 67), (149, 82)),
    "ring20": (80, 184756, 2518, (0, 284), (2518, 2234)),
}
CASES = [(name, z) for name in TABLE for z in (1, -1)]


@functools.lru_cache(maxsize=None)
def case(name, z):
    return Case(*geometry(name, z))
