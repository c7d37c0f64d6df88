"""Helpers of the tests of weighted sums over sparse least-squares blocks (include/parametron_hip.h, pmt_sparse_gram_sum_f64; record
mode "canonical-sparse-sum"): a brute-force Python restatement of the contract — structure, orders, first contributor — written from the
header text, not from the kernel, on sparse_gram_util.restate per block; an oracle builder that composes the literal function with
oracle.py alone (the per-block construction of sparse_gram_util.oracle_function, mul_quad_number / add_quad in expression order,
canonicalize, .moi(varmap)); and the derived bound between the two.  The restatement is proven against the oracle on the CPU
(test_sparse_sum_host.py) before any GPU output is compared with it bit for bit."""
import numpy as np

import sparse_gram_util as SG

EPS = SG.EPS
NONE = 0xFFFFFFFF


class Term:
    """One term of the sum, in plain data.  kind 'block': Cs (scipy CSC), d (or None), sign; 'diag': cols (positions in x, None = all of
    x), v (one entry per listed position, or None), sign; 'linear': cols, v = c; 'constant': value (None = 1.0).  The weight is
    W = scale * weight (one multiplication), or scale alone when weight is None."""

    def __init__(self, kind, scale=1.0, weight=None, Cs=None, d=None, sign=0, cols=None, v=None, value=None, pat=None):
        self.kind, self.scale, self.weight = kind, float(scale), weight
        self.Cs, self.d, self.sign, self.cols, self.value = Cs, d, sign, cols, value
        self.v = None if v is None else np.asarray(v, dtype=np.float64)
        # a block's pattern ([(j, k, products)], non-empty columns); `pat` given: synthetic lists without a matrix (the C ABI tests)
        self.pat = pat if pat is not None else (SG.pattern(Cs) if kind == "block" else None)

    @property
    def W(self):
        return self.scale if self.weight is None else self.scale * float(self.weight)

    def positions(self, n):
        return np.arange(n) if self.cols is None else np.asarray(self.cols, dtype=np.int64)

    def at(self, n, j):
        """the term's vector index of position j, or -1"""
        if self.cols is None:
            return j
        hit = np.flatnonzero(np.asarray(self.cols) == j)
        return int(hit[0]) if len(hit) else -1


def signed(v, sign):
    return 0.0 + float(v) if sign > 0 else 0.0 - float(v)


# ---- the structure, by brute force (sets and sorted(), not a merge)
def structure(n, terms):
    """(pairs, cols): the sorted quadratic pairs and linear columns of the contract"""
    pairs, cols = set(), set()
    for t in terms:
        if t.kind == "block":
            pairs |= {(j, k) for j, k, _ in t.pat[0]}
            cols |= set(t.pat[1])
        elif t.kind == "diag":
            pairs |= {(int(j), int(j)) for j in t.positions(n)}
            if t.v is not None:
                cols |= {int(j) for j in t.positions(n)}
        elif t.kind == "linear":
            cols |= {int(j) for j in t.positions(n)}
    return sorted(pairs), sorted(cols)


def gather_tables(n, terms):
    """per block (quad_at, lin_at) over the output terms, and per term with a column list its position table — what the merge must give"""
    pairs, cols = structure(n, terms)
    out = []
    for t in terms:
        if t.kind != "block":
            continue
        own = {(j, k): s for s, (j, k, _) in enumerate(t.pat[0])}
        lown = {j: l for l, j in enumerate(t.pat[1])}
        out.append((np.array([own.get(p, NONE) for p in pairs], dtype=np.uint32), np.array([lown.get(j, NONE) for j in cols], dtype=np.uint32)))
    pos = {}
    for i, t in enumerate(terms):
        if t.kind in ("diag", "linear") and t.cols is not None:
            p = np.full(n, -1, dtype=np.int32)
            p[np.asarray(t.cols, dtype=np.int64)] = np.arange(len(t.cols), dtype=np.int32)
            pos[i] = p
    return pairs, cols, out, pos


def block_outputs(xvar, varmap, terms):
    """per block its MOI-form outputs (Q_b, L_b, cc_b) of pmt_sparse_gram_f64, restated"""
    return [SG.restate(t.Cs, xvar, t.d, t.sign, 1, varmap, t.pat) for t in terms if t.kind == "block"]


def restate(n, xvar, varmap, terms, blocks=None):
    """The contract restated: (quad, lin, constant) as numpy QT / LT arrays and a float.  `blocks`: the blocks' (Q_b, L_b, cc_b) when the
    caller has them (synthetic lists at the C ABI); default: restated from the matrices."""
    from parametron_jl_amd._lib import LT, QT
    pairs, cols = structure(n, terms)
    blocks = blocks if blocks is not None else block_outputs(xvar, varmap, terms)
    x = np.asarray(xvar, dtype=np.int64)
    idx = np.asarray(varmap, dtype=np.int64)[x - 1]
    bt = [t for t in terms if t.kind == "block"]
    own = [{(j, k): s for s, (j, k, _) in enumerate(t.pat[0])} for t in bt]
    lown = [{j: l for l, j in enumerate(t.pat[1])} for t in bt]
    quad = np.zeros(len(pairs), dtype=QT)
    for s, (j, k) in enumerate(pairs):
        c, any_ = 0.0, False
        for t, o, (Q, _, _) in zip(bt, own, blocks):
            if (j, k) in o:
                v = t.W * float(Q["coeff"][o[(j, k)]])
                c = c + v if any_ else v
                any_ = True
        if j == k:
            d, anyd = 0.0, False
            for t in terms:
                if t.kind == "diag" and t.at(n, j) >= 0:
                    w2 = 2 * t.W
                    d = d + w2 if anyd else w2
                    anyd = True
            if anyd:
                c = c + d if any_ else d
        quad[s] = (c, idx[j], idx[k])
    lin = np.zeros(len(cols), dtype=LT)
    for l, j in enumerate(cols):
        c, any_ = 0.0, False
        for t, o, (_, L, _) in zip(bt, lown, blocks):
            if j in o:
                v = t.W * float(L["coeff"][o[j]])
                c = c + v if any_ else v
                any_ = True
        for t in terms:
            if t.kind == "diag" and t.v is not None and t.at(n, j) >= 0:
                v = t.W * (2 * signed(t.v[t.at(n, j)], t.sign))
                c = c + v if any_ else v
                any_ = True
        for t in terms:
            if t.kind == "linear" and t.at(n, j) >= 0:
                v = t.W * float(t.v[t.at(n, j)])
                c = c + v if any_ else v
                any_ = True
        lin[l] = (c, idx[j])
    const, any_ = 0.0, False
    for t, (_, _, cc) in zip(bt, blocks):
        v = t.W * float(cc)
        const = const + v if any_ else v
        any_ = True
    for t in terms:
        if t.kind == "diag" and t.v is not None:
            const = const + t.W * SG.chain_tree_sum(t.v * t.v)
    for t in terms:
        if t.kind == "constant":
            const = const + t.W * (1.0 if t.value is None else float(t.value))
    return quad, lin, float(const)


# ---- the oracle: the reference's literal sum restricted to the patterns
def _block_quad(O, t, xvar):
    """vecdot!(r, r) of rows holding the structural terms only — sparse_gram_util.oracle_function's construction, before canonicalize"""
    Cs = t.Cs
    m = Cs.shape[0]
    csr = Cs.tocsr()
    csr.sort_indices()
    c = SG.signed_consts(m, t.d, t.sign)
    r = O.AffVec(m)
    for i in range(m):
        row = r[i]
        row.zero()
        for u in range(csr.indptr[i], csr.indptr[i + 1]):
            row.push(float(csr.data[u]), int(xvar[csr.indices[u]]))
        row.set_constant(float(c[i]))
    return O.Quad().vecdot_affs_affs(r, r)


def oracle_function(n, xvar, varmap, terms):
    """(affine_terms, quadratic_terms, constant): every term's literal function scaled by its weight (mul_quad_number) and added in
    expression order (add_quad), canonicalize!, the MOI copy through varmap"""
    from oracle import oracle as O
    x = np.asarray(xvar, dtype=np.int64)
    total = O.Quad()
    for t in terms:
        if t.kind == "block":
            piece = _block_quad(O, t, x)
        elif t.kind == "diag":
            xs = x[t.positions(n)]
            if t.v is None:
                piece = O.Quad().vecdot_vars_vars(xs, xs)
            else:
                r = O.AffVec(len(xs))
                for i in range(len(xs)):
                    r[i].zero().push(1.0, int(xs[i])).set_constant(signed(t.v[i], t.sign))
                piece = O.Quad().vecdot_affs_affs(r, r)
        elif t.kind == "linear":
            piece = O.Quad().copy_from_aff(O.vecdot_aff_numbers_vars(t.v, x[t.positions(n)]))
        else:
            piece = O.Quad(constant=1.0 if t.value is None else float(t.value))
        total.add_quad(O.Quad().mul_quad_number(piece, t.W))
    return total.canonicalize().moi(varmap)


# ---- the derived bound
def bounds(n, terms):
    """Per coefficient, in the order of structure():  sum over the contributing blocks of |W_b| * (the block's own bound,
    sparse_gram_util.bounds: both sides add the block's products in their own orders)  +  nops * 2^-53 * T.
    T is the sum of the absolute contributions — |W_b| * S_b with S_b = 2 sum |C[i,j] C[i,k]| (linear: 2 sum |C[i,j] c_i|; constant:
    sum c_i^2), 2|W_t| per diagonal term on a diagonal pair, |W_t * 2 v_p| and |W_t * c_p| on a linear column, |W_t| S_t and |W_t * s| in
    the constant.  nops counts one rounding per multiplication and per addition of the combine, on both sides: the kernel multiplies each
    of the n_c contributions by its weight once and adds them in a chain (n_c - 1 additions; D_j's own chain and its addition are among
    them), the oracle multiplies every literal term by the same weight — each of those roundings is relative to its own term, so together
    they are one rounding over T — and joins the n_c groups with as many additions:  nops = 2 n_c + 1.  The weights themselves
    (scale * weight) and 2 * W are computed identically, or exactly, on both sides.  S_t of a diagonal term with v: the kernel's chains and
    tree against the oracle's left-to-right sum over nv squares, 2 nv 2^-53 S_t as for the blocks' constant.
    What the model assumes: the oracle's additions are counted block by block, each against the block's own S_b (the bare node's bound
    allows 4 L roundings where 3 L - 2 occur).  canonicalize!'s quicksort may interleave the terms of different blocks; the worst case of
    such an order is (N - 1) 2^-53 T over all N literal terms, which is LARGER than this bound.  The narrower, per-block bound is the one
    held here.  Not fitted to observed differences; no case is sampled or skipped."""
    pairs, cols = structure(n, terms)
    bt = [t for t in terms if t.kind == "block"]
    per = []
    for t in bt:
        bq, bl, bc = SG.bounds(t.Cs, t.d, t.sign, t.pat)
        v = t.Cs.data
        c = SG.signed_consts(t.Cs.shape[0], t.d, t.sign)
        Sq = {(j, k): 2 * sum(abs(v[ta] * v[tb]) for ta, tb in p) for j, k, p in t.pat[0]}
        Sl = {j: 2 * sum(abs(v[u] * c[t.Cs.indices[u]]) for u in range(t.Cs.indptr[j], t.Cs.indptr[j + 1])) for j in t.pat[1]}
        per.append(({(j, k): b for (j, k, _), b in zip(t.pat[0], bq)}, {j: b for j, b in zip(t.pat[1], bl)}, bc, Sq, Sl, float(np.sum(c * c))))
    outq = np.zeros(len(pairs))
    for s, (j, k) in enumerate(pairs):
        own, T, nc = 0.0, 0.0, 0
        for t, (bq, _, _, Sq, _, _) in zip(bt, per):
            if (j, k) in bq:
                own += abs(t.W) * bq[(j, k)]
                T += abs(t.W) * Sq[(j, k)]
                nc += 1
        if j == k:
            for t in terms:
                if t.kind == "diag" and t.at(n, j) >= 0:
                    T += 2 * abs(t.W)
                    nc += 1
        outq[s] = own + (2 * nc + 1) * EPS * T
    outl = np.zeros(len(cols))
    for l, j in enumerate(cols):
        own, T, nc = 0.0, 0.0, 0
        for t, (_, bl, _, _, Sl, _) in zip(bt, per):
            if j in bl:
                own += abs(t.W) * bl[j]
                T += abs(t.W) * Sl[j]
                nc += 1
        for t in terms:
            p = t.at(n, j) if t.kind in ("diag", "linear") and t.v is not None else -1
            if p >= 0:
                T += abs(t.W * t.v[p]) * (2 if t.kind == "diag" else 1)
                nc += 1
        outl[l] = own + (2 * nc + 1) * EPS * T
    own, T, nc = 0.0, 0.0, 0
    for t, (_, _, bc, _, _, cc) in zip(bt, per):
        own += abs(t.W) * bc
        T += abs(t.W) * cc
        nc += 1
    for t in terms:
        if t.kind == "diag" and t.v is not None:
            S = float(np.sum(t.v * t.v))
            own += abs(t.W) * 2 * len(t.v) * EPS * S
            T += abs(t.W) * S
            nc += 1
        elif t.kind == "constant":
            T += abs(t.W * (1.0 if t.value is None else float(t.value)))
            nc += 1
    return outq, outl, own + (2 * nc + 1) * EPS * T


assert_close_to_oracle = SG.assert_close_to_oracle


class ListTables:
    """the fields SparseSumTables reads of a block's SparseGramTables, from a pattern"""

    def __init__(self, pat):
        self.pair_j = np.array([j for j, _, _ in pat[0]], dtype=np.uint32)
        self.pair_k = np.array([k for _, k, _ in pat[0]], dtype=np.uint32)
        self.lin_col = np.array(pat[1], dtype=np.uint32)
        self.nq, self.nlin = len(self.pair_j), len(self.lin_col)


# ---- the library's symbolic phase for a term list (host tables only)
def merge_tables(n, terms, ctx=None):
    from parametron_jl_amd import _lib
    from parametron_jl_amd.device import SparseSumTables
    kind = {"block": _lib.PMT_LSQ_BLOCK, "diag": _lib.PMT_LSQ_DIAG, "linear": _lib.PMT_LSQ_LINEAR, "constant": _lib.PMT_LSQ_CONSTANT}
    Ts = [SG.tables(t.Cs) if t.Cs is not None else ListTables(t.pat) for t in terms if t.kind == "block"]
    return SparseSumTables(ctx, n, Ts, [(kind[t.kind], t.kind == "diag" and t.v is not None, t.cols) for t in terms])
