"""What the tests of the weighted-sum combine kernels (csrc/gram_sum.hip: pmt_quad_gram_sum_f64, pmt_quad_gram_sum_sub_f64) share: one
restatement of both entries by plain loops, the data family, the case tables, and the branch edges of the kernels that a case reaches.

The restatement is written from the contract in include/parametron_hip.h ("A WEIGHTED SUM of least-squares blocks ..") — not from the
kernels.  It takes the terms in expression order, block 1 anywhere among them, every diagonal / linear term with a list of positions or
without one, and returns whole images: the 3-word quadratic terms (coefficient bits, row, column: the last two as block 1 had them), the
2-word linear terms and the constant.  A term that is absent, or does not list a position, contributes NOTHING there: no `+ 0.0` is ever
written for it (that would turn a -0.0 into +0.0).  Elementwise numpy arithmetic is used where it keeps the order (one rounded multiply,
one rounded add per block, in expression order); whatever depends on j or on a list is a scalar loop.  tests/test_lsq_sum_host.py holds it
to the oracle bit for bit on exact data, shows that wrong restatements are told apart, and pins the edges below to the named cases.

THE NaN RULE.  Where a word is COMPUTED by the sum and the restated value is NaN, only "is NaN" is compared: the bits of inf - inf and of
a product of two NaNs are not fixed across the host and the GPU.  Every other word is compared as a word — also a NaN that the sum does
not touch (the off-diagonal coefficients and the unlisted diagonal ones of the diagonal-only form): that one is a copy and keeps its
payload and its signalling bit.  restate() returns the mask of the words under the rule; masked_counts() is held to the cap (2 % of the
quadratic coefficients, n/8 of the linear ones, the constant only in the case made for it) in the host test."""
import functools

import numpy as np

from sparse_assemble_util import DENORMAL, NAN_PAYLOAD, WORD, bits

TILE = 64                                                            # csrc/gram_sum.hip: SUM_TILE
MAX_TERMS, MAX_BLOCKS, MAX_RUNS = 32, 8, 64
INF = float("inf")
COLD = [0.0, -0.0, DENORMAL, -DENORMAL, -0.375, 0.625]               # specials that never make a NaN
SIGNALLING = np.array([0xFFF4BEEF0000DEAD], dtype=np.uint64).view(np.float64)[0]     # quiet bit clear: arithmetic would set it
OUTSIDE_BITS = np.array([0x7FF8BAD00BAD0BAD], dtype=np.uint64).view(np.int64)[0]     # what stands around every input on the device
NEG_ZERO_BITS = np.int64(-2 ** 63)
VAR_WORD = WORD + (1 << 40)                                          # lin[j].var = VAR_WORD + 2 j + 1: its own word position


def tree_sumsq(v):
    """S = sum_j v_j^2 in the kernel's order: 256 chains (chain t: j = t, t + 256, .. in order), then the halving tree"""
    red = np.zeros(256)
    for t in range(256):
        s = 0.0
        for x in v[t::256]:
            s = s + x * x
        red[t] = s
    h = 128
    while h:
        red[:h] = red[:h] + red[h:2 * h]
        h >>= 1
    return red[0]


def sequential_sumsq(v):
    s = 0.0
    for x in v:
        s = s + x * x
    return s


# ---- terms
class Term:
    """One pmt_lsq_term with its host data.  kind "block": values (CSC, nq) / lin (n coefficients) / constant of a LATER block (the first
    block's function is the image handed to restate; what its descriptor holds in these fields is a decoy the entry must ignore);
    "diag": v (or None) and sign; "linear": v = c; "constant": value (or None: 1.0).  cols: the listed positions of a diag / linear
    term (strictly increasing), or None for every column.  W = scale * weight (a device scalar), or scale."""

    def __init__(self, kind, scale=1.0, weight=None, values=None, lin=None, constant=None, v=None, sign=0, cols=None, value=None):
        self.kind, self.scale, self.weight, self.values, self.lin, self.constant = kind, float(scale), weight, values, lin, constant
        self.v = None if v is None else np.asarray(v, dtype=np.float64)
        self.sign, self.value = sign, value
        self.cols = None if cols is None else np.asarray(cols, dtype=np.int64)

    @property
    def W(self):
        return self.scale if self.weight is None else self.scale * float(self.weight)

    def index(self, j):
        """the term's vector index of position j, or -1 when it does not list j"""
        if self.cols is None:
            return j
        p = int(np.searchsorted(self.cols, j))
        return p if p < len(self.cols) and self.cols[p] == j else -1


def first_block(terms):
    return [t.kind for t in terms].index("block")


def is_fast(terms):
    """block 1 alone with the constant weight +1: the form that touches only the diagonal, lin and the constant"""
    b = [t for t in terms if t.kind == "block"]
    return len(b) == 1 and b[0].weight is None and b[0].scale == 1.0


def csc_of_rowmajor(n):
    j, k = np.triu_indices(n)
    return k * (k + 1) // 2 + j


def diag_positions(n):
    j = np.arange(n)
    return j * n - (j * (j - 1)) // 2


# ---- the restatement
def restate(n, terms, quad, lin, const, flaw=None):
    """quad: the 3 nq int64 words of block 1's terms (coefficient bits, row, col), lin: its 2 n words (coefficient bits, var), const: its
    constant.  -> (quad words, lin words, constant, masks) with masks = (bool per quadratic term, bool per linear term, bool): the
    coefficients under the NaN rule.  flaw: one of the deliberately wrong restatements of WRONG (the host test shows each is rejected)."""
    nq = n * (n + 1) // 2
    quad, lin = np.array(quad, dtype=np.int64).reshape(nq, 3), np.array(lin, dtype=np.int64).reshape(n, 2)
    q1, l1 = quad[:, 0].copy().view(np.float64), lin[:, 0].copy().view(np.float64)
    first = first_block(terms)
    later = [t for t in (terms[1:] if flaw == "blocks_from_term_1" else terms[first + 1:]) if t.kind == "block"]
    diags = [t for t in terms if t.kind == "diag"]
    W1, fast = terms[first].W, is_fast(terms)
    sumsq = sequential_sumsq if flaw == "sequential_sumsq" else tree_sumsq
    with np.errstate(all="ignore"):
        computed = np.zeros(nq, dtype=bool)
        coeff = q1.copy()
        if not fast:
            csc = csc_of_rowmajor(n)
            coeff = W1 * q1
            for t in later:
                coeff = coeff + t.W * (q1 if t is terms[first] else t.values[csc])
            computed[:] = True
        dpos = diag_positions(n)
        for j in range(n):
            d = None                                                 # no D term without a diagonal term listing j
            for t in diags:
                if t.index(j) < 0:
                    if flaw == "plus_zero":
                        d = 0.0 if d is None else d + 0.0
                    continue
                w2 = 2 * t.W
                d = w2 if d is None else d + w2
            if d is None:
                continue
            where = [dpos[j]] if flaw != "d_on_every_tile_diagonal" else \
                [dpos[i] + (j - i) for i in range(j % TILE, j + 1, TILE)]         # (i, j) with i = j mod 64: local row == local column
            for p in where:
                coeff[p] = (W1 * q1[p] if fast else coeff[p]) + d
                computed[p] = True
        out_lin = np.empty(n)
        for j in range(n):
            c = W1 * float(l1[j])
            for t in later:
                c = c + t.W * float(l1[j] if t is terms[first] else t.lin[j])
            for t in diags:
                i = t.index(j)
                if t.v is None:
                    continue
                if i >= 0:
                    c = c + t.W * (2 * ((0.0 + float(t.v[i])) if t.sign > 0 else (0.0 - float(t.v[i]))))
                elif flaw == "plus_zero":
                    c = c + 0.0
            for t in terms:
                if t.kind != "linear":
                    continue
                i = t.index(j)
                if i >= 0:
                    c = c + t.W * float(t.v[i])
                elif flaw == "plus_zero":
                    c = c + 0.0
            out_lin[j] = c
        s = W1 * float(const)
        for t in later:
            s = s + t.W * float(const if t is terms[first] else t.constant)
        for t in diags:
            if t.v is not None:
                s = s + t.W * float(sumsq(t.v))
        for t in terms:
            if t.kind == "constant":
                s = s + t.W * (1.0 if t.value is None else float(t.value))
    quad[:, 0] = bits(coeff)
    lin[:, 0] = bits(out_lin)
    masks = (computed & np.isnan(coeff), np.isnan(out_lin), bool(np.isnan(s)))
    return quad.reshape(-1), lin.reshape(-1), float(s), masks


WRONG = {
    "plus_zero": "an unlisted position gets + 0.0 from the term",
    "d_on_every_tile_diagonal": "D added wherever a tile's local row equals its local column, not on the matrix's j == k",
    "blocks_from_term_1": "the later blocks looped from term 1, not from behind block 1",
    "sequential_sumsq": "S_d summed left to right",
}


def masked_counts(masks):
    return int(masks[0].sum()), int(masks[1].sum()), bool(masks[2])


# ---- the data family (tests/sparse_assemble_util.py: both zeros, denormals, the infinities, one NaN with a payload)
def values(L, seed, hot=False, nan=False):
    """L doubles of both signs in [-0.5, 0.5) with +0.0, -0.0, denormals of both signs and two short dyadics planted; hot: both
    infinities too, nan: the NaN with a payload (only where L allows the cap on masked words: L >= 24).  The places depend on L and on
    what is planted alone, so that every vector of a case has its infinities at the same positions."""
    a = np.random.default_rng(seed).random(L) - 0.5
    a[a == 0.0] = 0.25
    sp = list(COLD) + ([INF, -INF] if hot and L >= 24 else []) + ([NAN_PAYLOAD] if nan and L >= 24 else [])
    if L >= 2 * len(sp):
        for k, s in enumerate(sp):
            a[(k * L) // 9 + 1] = s
    else:
        for k in range(min(L, len(COLD))):
            a[(seed + k) % L] = COLD[(seed + k) % len(COLD)]
    return a


WEIGHTS = [(0.7, None), (-1.0, None), (0.5, 1.3), (1.0, None), (0.0, None), (-3.0, 0.7), (1.0, 1.0), (0.7, -1.0)]     # (scale, device scalar)


class _Maker:
    """hands out seeds and weights in a fixed order"""

    def __init__(self, n, seed):
        self.n, self.nq, self.seed, self.k = n, n * (n + 1) // 2, 1000 * seed, 0

    def w(self, w=None):
        self.k += 1
        return WEIGHTS[(self.seed // 1000 + self.k) % len(WEIGHTS)] if w is None else w

    def next(self):
        self.seed += 1
        return self.seed

    def block(self, w=None, hot=True, first=False, decoy=True):
        scale, weight = self.w(w)
        if first and not decoy:
            return Term("block", scale, weight)
        # (a first block's arrays are decoys: ordinary numbers the entry must never read)
        live = hot and not first
        return Term("block", scale, weight, values=values(self.nq, self.next(), live, live), lin=values(self.n, self.next(), live, live),
                    constant=float(np.random.default_rng(self.next()).random() - 0.5))

    def diag(self, w=None, v=False, sign=0, cols=None, hot=False, nan=False):
        scale, weight = self.w(w)
        m = self.n if cols is None else len(cols)
        return Term("diag", scale, weight, v=values(m, self.next(), hot, nan) if v else None, sign=sign if v else 0, cols=cols)

    def linear(self, w=None, cols=None, hot=False):
        scale, weight = self.w(w)
        return Term("linear", scale, weight, v=values(self.n if cols is None else len(cols), self.next(), hot, hot), cols=cols)

    def constant(self, w=None, value=True):
        scale, weight = self.w(w)
        return Term("constant", scale, weight, value=float(np.random.default_rng(self.next()).random() - 0.5) if value else None)


class Case:
    """a named sum: n, the terms, block 1's image, which entry it goes through (sub: pmt_quad_gram_sum_sub_f64), and the edge it is for"""

    def __init__(self, name, why, n, terms, sub=False, seed=0, hot=True, negzero=None, signalling=()):
        self.name, self.why, self.n, self.terms, self.sub = name, why, n, terms, sub or any(t.cols is not None for t in terms)
        nq = n * (n + 1) // 2
        hot = hot and n >= 24
        coeff, lcoeff = values(nq, 7000 + seed, hot, hot), values(n, 8000 + seed, hot, hot)
        self.negzero = negzero or ((), (), ())
        dj, off, lj = self.negzero
        dpos = diag_positions(n)
        for j in dj:
            coeff[dpos[j]] = -0.0
        for j, k in off:
            coeff[dpos[j] + k - j] = -0.0
        for j in lj:
            lcoeff[j] = -0.0
        for j in signalling:                                         # on diagonal positions the diagonal-only form leaves alone
            coeff[dpos[j]] = SIGNALLING
        self.signalling = tuple(signalling)
        quad = WORD + np.arange(3 * nq, dtype=np.int64)              # row / col: their own word position
        quad[0::3] = bits(coeff)
        lin = VAR_WORD + np.arange(2 * n, dtype=np.int64)
        lin[0::2] = bits(lcoeff)
        self.quad, self.lin, self.const = quad, lin, float(np.random.default_rng(9000 + seed).random() - 0.5)

    def __repr__(self):
        return self.name

    @property
    def nq(self):
        return self.n * (self.n + 1) // 2

    @functools.lru_cache(maxsize=None)
    def restated(self):
        return restate(self.n, self.terms, self.quad, self.lin, self.const)

    def negzero_words(self):
        """(quad word positions, lin word positions) that hold -0.0 in block 1's image and must come back as -0.0"""
        dj, off, lj = self.negzero
        dpos = diag_positions(self.n)
        return [3 * int(dpos[j]) for j in dj] + [3 * int(dpos[j] + k - j) for j, k in off], [2 * j for j in lj]


def _mixed(n, K, lead, seed, first_w=None):
    """K blocks in expression order with the other kinds of term between them; `lead` terms (0, 1 or 3) stand in front of block 1"""
    m = _Maker(n, seed)
    terms = [m.diag(), m.linear(), m.constant()][:lead] if lead != 3 else [m.diag(v=True, sign=-1), m.linear(hot=True), m.constant()]
    for k in range(K):
        terms.append(m.block(first_w if k == 0 else None, first=(k == 0), decoy=(lead > 0 or k % 2 == 0)))
        if k % 2 == 0:
            terms.append(m.diag(v=(k % 4 == 0), sign=1 if k % 3 == 0 else -1))
        if k % 3 == 1 or K == 1:
            terms += [m.linear(), m.constant(value=bool(k % 2))]
    return terms


def _thirty_two(n, seed, lists=False):
    """8 blocks, 8 diagonal, 8 linear and 8 constant terms, interleaved; lists: every second diagonal / linear term lists part of x"""
    m = _Maker(n, seed)
    terms = []
    for k in range(8):
        part = np.arange(k, n, 5 + k)[:7] if lists and k % 2 else None           # single positions: 7 runs each, 56 in all
        terms += [m.diag(v=(k % 3 == 0), sign=-1 if k % 2 else 1, cols=part), m.block(first=(k == 0)), m.constant(value=bool(k % 2)),
                  m.linear(cols=None if part is None else part + 1)]
    return terms


ONE = (1.0, None)                                                    # the constant weight +1
ONE_ON_DEVICE = (1.0, 1.0)                                           # +1 as scale * device scalar: not the diagonal-only form


def _cases():
    out = []

    def add(name, why, n, terms, **kw):
        out.append(Case(name, why, n, terms, seed=len(out), **kw))

    # ---- the plain entry
    m = _Maker(0, 1)
    add("n0", "cols == 0: only the constant kernel runs", 0, [m.block(first=True, decoy=False), m.diag(), m.constant((0.7, None))])
    add("n1", "one term, one workgroup, a one-term row segment", 1, _mixed(1, 1, 0, 2, (0.7, None)))
    add("n2", "two rows, two blocks", 2, _mixed(2, 2, 0, 3))
    add("n63_block1_second", "one ragged tile; block 1 at term index 1, behind a diagonal term", 63, _mixed(63, 2, 1, 4))
    add("n64", "one full tile; three blocks", 64, _mixed(64, 3, 0, 5))
    add("n65_K8", "3 tiles, the last column tile one wide; 8 blocks", 65, _mixed(65, 8, 0, 6))
    add("n128_block1_fourth", "full tiles only; block 1 at term index 3", 128, _mixed(128, 2, 3, 7))
    add("n129_32_terms", "32 terms, 8 blocks", 129, _thirty_two(129, 8))
    add("n193", "4 tile rows: an off-diagonal tile that is not next to the diagonal", 193, _mixed(193, 2, 0, 9))
    add("n513", "S_d chains of length 3 (and 2); 9 tile rows", 513, _mixed(513, 2, 1, 10))
    add("n65_K1_weighted", "one block, weight 0.0 * device scalar: the tile kernel, not the diagonal-only form", 65, _mixed(65, 1, 0, 11, (0.0, 1.3)))
    # ---- the diagonal-only form (block 1 alone, no weight pointer, scale 1.0)
    m = _Maker(65, 12)
    add("fast_no_diag", "diagonal-only form without a diagonal term: quad untouched", 65, [m.block(ONE, first=True), m.linear(), m.constant()],
        signalling=(0, 64))
    m = _Maker(65, 13)
    add("fast_full_diag", "diagonal-only form, a diagonal term over all of x", 65, [m.block(ONE, first=True, decoy=False), m.diag((0.7, None), v=True, sign=-1, hot=True)])
    m = _Maker(129, 14)
    add("fast_listed_diag", "diagonal-only form, a listed diagonal term: unlisted diagonal words stay", 129,
        [m.diag((0.5, 1.3), cols=np.arange(3, 100)), m.block(ONE, first=True), m.linear(cols=[0, 128])], signalling=(0, 2, 100, 128))
    # ---- lists
    m = _Maker(70, 15)
    add("list_empty", "a list of length 0: the term adds nothing anywhere, S_d over no entries", 70,
        [m.block(first=True), m.diag(v=True, sign=1, cols=[]), m.linear(cols=[]), m.diag((0.7, None), cols=[5])])
    m = _Maker(70, 16)
    add("list_first", "{0}: a run at position 0", 70, [m.block(first=True), m.diag(v=True, sign=-1, cols=[0]), m.linear(cols=[0])])
    m = _Maker(70, 17)
    add("list_last", "{cols - 1}: a run ending at the last position", 70, [m.block(first=True), m.diag(v=True, sign=1, cols=[69]), m.linear(cols=[69])])
    m = _Maker(70, 18)
    add("list_all_but_0", "one run covering everything but position 0", 70,
        [m.block((-1.0, None), first=True), m.diag(v=True, sign=-1, cols=np.arange(1, 70)), m.linear(cols=np.arange(1, 70))])
    m = _Maker(129, 19)
    add("list_64_runs", "alternating positions: exactly 64 runs over all terms", 129,
        [m.block(first=True), m.diag(v=True, sign=1, cols=np.arange(0, 64, 2)), m.block(), m.linear(cols=np.arange(65, 129, 2))])
    m = _Maker(70, 20)
    add("two_diags_overlapping", "two diagonal terms (v and sign +1 | no v) whose lists overlap in part: D_j over those listing j", 70,
        [m.block(first=True), m.diag((0.7, None), v=True, sign=1, cols=np.arange(10, 40)), m.diag((0.5, 1.3), cols=np.r_[0:3, 30:50, 69])])
    m = _Maker(70, 21)
    add("listed_linear_full_diag", "a linear term with a list beside a diagonal term without one", 70,
        [m.linear(cols=np.r_[0, 7:12, 63:66]), m.block(first=True), m.diag((-3.0, 0.7), v=True, sign=-1, hot=True)])
    for length in (1, 255, 256, 257):
        m = _Maker(260, 22 + length)
        add("sd_%d" % length, "S_d over a listed vector of %d entries" % length, 260,
            [m.block(first=True), m.diag((0.7, None), v=True, sign=-1, cols=np.arange(2, 2 + length))], hot=False)
    add("list_32_terms", "32 terms, 8 blocks, 56 runs", 129, _thirty_two(129, 30, lists=True))
    # ---- -0.0 in block 1: what a term does not list gets nothing, not + 0.0
    nz = ((0, 5, 63, 64), ((0, 1), (3, 64), (63, 64)), (0, 5, 64))
    m = _Maker(65, 31)
    add("negzero_weight_one_unlisted", "-0.0 at weight +1 (scale * device scalar) on positions no term lists", 65,
        [m.block(ONE_ON_DEVICE, first=True), m.diag(v=True, sign=1, cols=np.arange(6, 60)), m.linear(cols=np.arange(10, 20))], negzero=nz, hot=False)
    m = _Maker(65, 32)
    add("negzero_no_diag", "-0.0 at weight +1 without a diagonal term: the tile kernel adds no D", 65,
        [m.block(ONE_ON_DEVICE, first=True), m.constant()], negzero=nz, hot=False)
    m = _Maker(65, 33)
    add("negzero_fast", "-0.0 in the diagonal-only form on unlisted positions", 65,
        [m.block(ONE, first=True), m.diag(v=True, sign=-1, cols=np.arange(6, 60)), m.linear(cols=np.arange(10, 20))], negzero=nz, hot=False)
    # ---- the one case whose constant is NaN
    m = _Maker(65, 34)
    add("constant_nan", "a NaN in v: S_d and the constant are NaN", 65, [m.block((0.5, 1.3), first=True), m.diag((0.7, None), v=True, sign=1, hot=True, nan=True)])
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return {c.name: c for c in _cases()}


def case(name):
    return cases()[name]


RECORDED = ("n65_K8", "two_diags_overlapping")                        # the cases replayed from a plan
SLICES = ("n65_K8", "n64")                                            # the two sums written into adjacent slices (65 and 64 columns)


# ---- the tables the sub entry hands its kernels, restated from the header (runs of consecutive positions)
def runs(cols):
    """[(start, length, first vector index)] of a strictly increasing list"""
    out = []
    for i, j in enumerate(int(v) for v in cols):
        if out and j == out[-1][0] + out[-1][1]:
            out[-1][1] += 1
        else:
            out.append([j, 1, i])
    return [tuple(r) for r in out]


def total_runs(terms):
    return sum(len(runs(t.cols)) for t in terms if t.cols is not None)


# ---- which branch edges of the kernels a case reaches
def edges(c, shift):
    """the edges of gram_sum_tile's row-segment stores (out_quad at 8 * shift mod 16) and of SubCols::find that case `c` reaches, from the
    numbers the kernel computes them from: n, the tile pair, the segment's first word, the runs"""
    out, n = set(), c.n
    fast = is_fast(c.terms)
    out.add("diagonal-only form" if fast else "tile kernel")
    if n == 0:
        return {"no columns"}
    if not fast:
        nt = -(-n // TILE)
        out.add("ragged last tile" if n % TILE else "full last tile")
        for bj in range(nt):
            for bk in range(bj, nt):
                out.add("diagonal tile" if bk == bj else ("off-diagonal tile next to the diagonal" if bk == bj + 1 else "off-diagonal tile not next to the diagonal"))
                j0, k0 = bj * TILE, bk * TILE
                for j in range(j0, min(j0 + TILE, n)):
                    ks, ke = max(k0, j), min(k0 + TILE, n)
                    nwords = 3 * (ke - ks)
                    lead = (shift + 3 * (j * n - (j * (j - 1)) // 2 + ks - j)) & 1
                    out.add("lead word" if lead else "no lead word")
                    out.add("single tail word" if (nwords - lead) & 1 else "tail pair")
                    if nwords == 3:
                        out.add("one-term segment")
                    if nwords > 128:
                        out.add("second round of a lane")
    for t in c.terms:
        if t.kind not in ("diag", "linear"):
            continue
        if t.cols is None:
            out.add("term without a list")
            continue
        rs = runs(t.cols)
        if not rs:
            out.add("empty list")
        for j in range(n):                                            # the kernels call find(t, j) for every position
            hit = [r for r in rs if r[0] <= j < r[0] + r[1]]
            if not hit:
                out.add("find: miss")
                if any(j == r[0] + r[1] for r in rs):
                    out.add("find: miss right behind a run")
                if any(j == r[0] - 1 for r in rs):
                    out.add("find: miss right before a run")
                continue
            s, ln, _ = hit[0]
            out.add("find: hit at run start" if j == s else ("find: hit at run end" if j == s + ln - 1 else "find: hit inside a run"))
            if j == s + ln - 1:
                out.add("find: hit at run end")
            if j == 0:
                out.add("find: hit at position 0")
            if j == n - 1:
                out.add("find: hit at position cols - 1")
            if hit[0] is not rs[0]:
                out.add("find: hit in a later run")
    if total_runs(c.terms) == MAX_RUNS:
        out.add("64 runs")
    return out


ALL_EDGES = {
    "tile kernel", "diagonal-only form", "no columns", "ragged last tile", "full last tile", "diagonal tile", "off-diagonal tile next to the diagonal",
    "off-diagonal tile not next to the diagonal", "lead word", "no lead word", "single tail word", "tail pair", "one-term segment", "second round of a lane",
    "term without a list", "empty list", "find: miss", "find: miss right behind a run", "find: miss right before a run", "find: hit at run start",
    "find: hit at run end", "find: hit inside a run", "find: hit at position 0", "find: hit at position cols - 1", "find: hit in a later run", "64 runs",
}
