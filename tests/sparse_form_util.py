"""Helpers of the tests of the sparse quadratic form transpose(x)*Q*x (include/parametron_hip.h, pmt_sparse_form_f64; record mode
"canonical-sparse-form"): a brute-force numpy / Python restatement of the contract — pairs, source words, coefficients — written from the
header text, not from the kernel (dictionaries and sorted(), not a merge); the oracle sequence the contract cites; patterns of every
class the tests use.  The restatement is proven against the oracle on the CPU (test_sparse_form_host.py) before any GPU output is compared
with it bit for bit.  Self-contained: numpy and scipy only, besides the package's term dtypes."""
import numpy as np
import scipy.sparse as sp

NONE = 0xFFFFFFFF


def csc(Q):
    """canonical CSC (rows ascending within a column, no duplicates) keeping explicitly stored zeros"""
    Q = sp.csc_matrix(Q)
    Q.sort_indices()
    return Q


def from_entries(n, rows, cols, vals):
    """the n x n CSC matrix with exactly these stored entries (distinct positions; zeros stay stored)"""
    rows, cols, vals = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.float64)
    order = np.lexsort((rows, cols))
    rows, cols, vals = rows[order], cols[order], vals[order]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, cols + 1, 1)
    return sp.csc_matrix((vals, rows.astype(np.int64), np.cumsum(indptr)), shape=(n, n))


def tables(Q):
    """(pair_j, pair_k, src_a, src_b): per unordered pair {j, k}, j <= k, with Q[j,k] or Q[k,j] stored, sorted by (j, k), the position in
    nzval of Q[j,k] (row j, column k) and of Q[k,j], NONE where not stored; on the diagonal src_a is the entry and src_b NONE"""
    Q = csc(Q)
    n = Q.shape[0]
    at = {}
    for c in range(n):
        for p in range(Q.indptr[c], Q.indptr[c + 1]):
            at[(int(Q.indices[p]), c)] = p
    pairs = sorted({(min(r, c), max(r, c)) for r, c in at})
    pj = np.array([j for j, _ in pairs], dtype=np.uint32)
    pk = np.array([k for _, k in pairs], dtype=np.uint32)
    sa = np.array([at.get((j, k), NONE) for j, k in pairs], dtype=np.uint32)
    sb = np.array([at.get((k, j), NONE) if j != k else NONE for j, k in pairs], dtype=np.uint32)
    return pj, pk, sa, sb


def coefficients(nzval, tabs, moi):
    """the contract's coefficients: both stored: Q[j,k] + Q[k,j]; one stored: that value unchanged; diagonal: 2*Q[j,j] (moi) / Q[j,j]"""
    pj, pk, sa, sb = tabs
    v = np.asarray(nzval, dtype=np.float64)
    out = np.zeros(len(pj), dtype=np.float64)
    for s in range(len(pj)):
        if pj[s] == pk[s]:
            out[s] = 2 * v[sa[s]] if moi else v[sa[s]]
        elif sa[s] != NONE and sb[s] != NONE:
            out[s] = v[sa[s]] + v[sb[s]]
        else:
            out[s] = v[sa[s]] if sa[s] != NONE else v[sb[s]]
    return out


def restate(Q, xvar, moi, varmap=None, nzval=None, tabs=None):
    """the contract restated: the quadratic terms as a numpy QT array (no linear terms, constant 0.0)"""
    from parametron_jl_amd._lib import QT
    Q = csc(Q)
    tabs = tabs if tabs is not None else tables(Q)
    x = np.asarray(xvar, dtype=np.int64)
    idx = np.asarray(varmap, dtype=np.int64)[x - 1] if moi else x
    out = np.zeros(len(tabs[0]), dtype=QT)
    out["coeff"] = coefficients(Q.data if nzval is None else nzval, tabs, moi)
    out["row"], out["col"] = idx[tabs[0].astype(np.int64)], idx[tabs[1].astype(np.int64)]
    return out


def oracle_quad(Q, xvar):
    """the reference's literal function of transpose(x)*Q*x over the stored entries only, before canonicalize: bilinearmul!
    (src/functions.jl:840-858) emits (Q[r,c], x_r, x_c) per entry, here in CSC order"""
    from oracle import oracle as O
    Q = csc(Q)
    f = O.Quad().zero()
    for c in range(Q.shape[1]):
        for p in range(Q.indptr[c], Q.indptr[c + 1]):
            f.add_term(float(Q.data[p]), int(xvar[Q.indices[p]]), int(xvar[c]))
    return f


def oracle_function(Q, xvar, varmap):
    """(affine_terms, quadratic_terms, constant) of the oracle: add_term per stored entry, canonicalize!, the MOI copy through varmap
    (a lone term's two variables still in stored order: ordered_words)"""
    at, qt, const = oracle_quad(Q, xvar).canonicalize().moi(np.asarray(varmap, dtype=np.int64))
    return at, qt, const


def ordered_words(qt, xvar, varmap):
    """the oracle's quadratic terms with each term's two index words ordered by their positions in x; the terms keep the oracle's order
    (canonicalize! sorts by the ordered pair, so it is the contract's).  Returns a QT array."""
    x = np.asarray(xvar, dtype=np.int64)
    idx = np.asarray(varmap, dtype=np.int64)[x - 1]
    pos = {int(v): p for p, v in enumerate(idx)}
    out = qt.copy()
    a = np.array([pos[int(v)] for v in qt["row"]], dtype=np.int64)
    b = np.array([pos[int(v)] for v in qt["col"]], dtype=np.int64)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    out["row"], out["col"] = idx[lo], idx[hi]
    return out


def assert_same_words(got, want, what=""):
    """two QT arrays equal word for word (coefficients by bit pattern: -0.0 differs from 0.0)"""
    assert got.shape == want.shape, "%s: %d terms, expected %d" % (what, len(got), len(want))
    g, w = np.ascontiguousarray(got).view(np.int64), np.ascontiguousarray(want).view(np.int64)
    bad = np.flatnonzero(g != w)
    assert len(bad) == 0, "%s: word %d differs: %r vs %r" % (what, bad[0], got[bad[0] // 3], want[bad[0] // 3])


# ---- patterns
def values(rng, nnz, zeros=True):
    """normal values; with `zeros`, about one in eight is 0.0 and one in eight -0.0 (stored all the same)"""
    v = rng.standard_normal(nnz)
    if zeros and nnz:
        u = rng.random(nnz)
        v[u < 0.125] = 0.0
        v[(u >= 0.125) & (u < 0.25)] = -0.0
    return v


def pattern(kind, n, rng, density=0.3, zeros=True):
    """an n x n matrix of one of the classes: 'upper', 'lower', 'symmetric', 'mixed' (some pairs stored twice, some once, some diagonal),
    'diagonal', 'empty-columns' (mixed with about half of the columns empty), 'none' (nnz = 0)"""
    if kind == "none":
        return sp.csc_matrix((n, n), dtype=np.float64)
    if kind == "diagonal":
        keep = np.flatnonzero(rng.random(n) < max(density, 0.5))
        return from_entries(n, keep, keep, values(rng, len(keep), zeros))
    M = rng.random((n, n)) < density
    if kind == "upper":
        M = np.triu(M)
    elif kind == "lower":
        M = np.tril(M)
    elif kind == "symmetric":
        M = np.triu(M)
        M = M | M.T
    elif kind == "empty-columns":
        M[:, rng.random(n) < 0.5] = False
    elif kind != "mixed":
        raise ValueError(kind)
    r, c = np.nonzero(M)
    return from_entries(n, r, c, values(rng, len(r), zeros))


KINDS = ("upper", "lower", "symmetric", "mixed", "diagonal", "empty-columns", "none")


def with_nq(nq, n, rng, zeros=True):
    """a 'mixed' n x n matrix (both / upper-only / lower-only / diagonal pairs side by side) with exactly nq pairs, nq <= n(n+1)/2"""
    assert nq <= n * (n + 1) // 2
    iu = np.triu_indices(n)
    must = [0, n] if nq >= 4 else []                   # the pairs (0, 0) and (1, 1): a diagonal term among the first 64
    rest = np.setdiff1d(np.arange(len(iu[0])), must)
    pick = np.sort(np.concatenate([must, rng.choice(rest, size=nq - len(must), replace=False)]).astype(np.int64))
    rows, cols = [], []
    for t, (j, k) in enumerate(zip(iu[0][pick], iu[1][pick])):
        how = t % 3 if j != k else 0
        if how in (0, 2):
            rows.append(j); cols.append(k)
        if how in (1, 2) and j != k:
            rows.append(k); cols.append(j)
    return from_entries(n, rows, cols, values(rng, len(rows), zeros))


def form_tables(Q):
    """the library's symbolic phase for a pattern (host tables only): parametron_jl_amd.device.SparseFormTables"""
    from parametron_jl_amd.device import SparseFormTables
    Q = csc(Q)
    return SparseFormTables(None, Q.shape[0], Q.indptr, Q.indices)


# ---- sums with a form: sparse_sum_util's machinery with the form as a block of nlin = 0
class FormTerm:
    """transpose(x)*Q*x as a term of a weighted sum, in the shape sparse_sum_util.Term has for a block: `pat` = (its pairs, no linear
    columns), so that sparse_sum_util.structure / gather_tables / restate read it as a block without linear terms"""
    kind = "block"
    form = True
    Cs = d = cols = v = value = None
    sign = 0

    def __init__(self, Q, scale=1.0, weight=None):
        self.Q, self.scale, self.weight = csc(Q), float(scale), weight
        self.tabs = tables(self.Q)
        self.pat = ([(int(j), int(k), None) for j, k in zip(self.tabs[0], self.tabs[1])], [])

    @property
    def W(self):
        return self.scale if self.weight is None else self.scale * float(self.weight)

    def outputs(self, xvar, varmap):
        """(Q_b, L_b, cc_b): the form's MOI-form outputs as a block's — no linear terms, constant 0.0"""
        from parametron_jl_amd._lib import LT
        return restate(self.Q, xvar, 1, varmap, tabs=self.tabs), np.zeros(0, dtype=LT), 0.0


def sum_restate(n, xvar, varmap, terms):
    """sparse_sum_util.restate over a term list that holds FormTerms: the blocks' outputs are the bare nodes' restatements"""
    import sparse_gram_util as SG
    import sparse_sum_util as SU
    blocks = [t.outputs(xvar, varmap) if getattr(t, "form", False) else SG.restate(t.Cs, xvar, t.d, t.sign, 1, varmap, t.pat)
              for t in terms if t.kind == "block"]
    return SU.restate(n, xvar, varmap, terms, blocks=blocks)


def sum_oracle(n, xvar, varmap, terms):
    """sparse_sum_util.oracle_function with a form's literal function (oracle_quad) where a FormTerm stands: every term's literal
    function scaled by its weight (mul_quad_number), added in expression order (add_quad), canonicalize!, the MOI copy"""
    from oracle import oracle as O
    import sparse_sum_util as SU
    x = np.asarray(xvar, dtype=np.int64)
    total = O.Quad()
    for t in terms:
        if getattr(t, "form", False):
            piece = oracle_quad(t.Q, x)
        elif t.kind == "block":
            piece = SU._block_quad(O, t, x)
        elif t.kind == "diag":
            xs = x[t.positions(n)]
            if t.v is None:
                piece = O.Quad().vecdot_vars_vars(xs, xs)
            else:
                r = O.AffVec(len(xs))
                for i in range(len(xs)):
                    r[i].zero().push(1.0, int(xs[i])).set_constant(SU.signed(t.v[i], t.sign))
                piece = O.Quad().vecdot_affs_affs(r, r)
        elif t.kind == "linear":
            piece = O.Quad().copy_from_aff(O.vecdot_aff_numbers_vars(t.v, x[t.positions(n)]))
        else:
            piece = O.Quad(constant=1.0 if t.value is None else float(t.value))
        total.add_quad(O.Quad().mul_quad_number(piece, t.W))
    at, qt, const = total.canonicalize().moi(np.asarray(varmap, dtype=np.int64))
    return at, ordered_words(qt, xvar, varmap), const


def sum_bounds(n, terms):
    """sparse_sum_util.bounds for a term list that holds FormTerms.  That bound is, per coefficient,
        sum over the contributing blocks of |W_b| * (the block's own bound)  +  (2 n_c + 1) * 2^-53 * T
    with T the sum of the absolute contributions and n_c their number.  A form enters it as a block without linear terms and with
    constant 0.0 whose own bound is 2 * 2^-53 * (|Q[j,k]| + |Q[k,j]|) on a pair stored twice — one addition on either side: the kernel
    adds the two values, the oracle their weighted copies — and 0 elsewhere (a lone or diagonal value is copied, or doubled exactly), and
    whose absolute contribution is S = |Q[j,k]| + |Q[k,j]| (2 |Q[j,j]| on the diagonal).  sparse_sum_util.bounds reads a block's matrix,
    which a form does not have, so its formula is restated here whole, with a sparse block's figures computed exactly as there.
    Written from that derivation, not fitted."""
    import sparse_gram_util as SG
    import sparse_sum_util as SU
    EPS = SG.EPS
    pairs, cols = SU.structure(n, terms)
    bt = [t for t in terms if t.kind == "block"]
    per = []
    for t in bt:
        if getattr(t, "form", False):
            v = np.abs(t.Q.data)
            pj, pk, sa, sb = t.tabs
            S = {}
            own = {}
            for s in range(len(pj)):
                both = sa[s] != NONE and sb[s] != NONE
                a = v[sa[s]] if sa[s] != NONE else 0.0
                b = v[sb[s]] if sb[s] != NONE else 0.0
                S[(int(pj[s]), int(pk[s]))] = 2 * a if pj[s] == pk[s] else a + b
                own[(int(pj[s]), int(pk[s]))] = 2 * EPS * (a + b) if both else 0.0
            per.append((own, {}, 0.0, S, {}, 0.0))
        else:
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
