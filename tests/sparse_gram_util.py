"""Helpers of the sparse least-squares objective's tests (dot(r, r), r = C*x (+|-) d with a sparse C; include/parametron_hip.h,
pmt_sparse_gram_f64): a brute-force Python restatement of the contract — pattern, orders, doubling — written from the header, not from
the kernels, and an oracle builder that makes the literal function with oracle.py (rows holding the structural terms only,
vecdot_affs_affs, canonicalize, .moi(varmap)).  The restatement is proven against the oracle on the CPU (test_sparse_gram_host.py) before
any GPU output is compared with it bit for bit."""
import ctypes as C

import numpy as np

from gpu_util import run_sum_sequential, run_sum_wave

EPS = 2.0 ** -53
LONG = 64                      # segments of this many products or more are added in the one-wave order


def signed_values(rng, k):
    """signed test values, U[0, 1) - 0.5"""
    return rng.random(k) - 0.5


def random_csc(rng, m, n, density):
    import scipy.sparse as sp
    mask = rng.random((m, n)) < density
    Cs = sp.csc_matrix(np.where(mask, 1.0, 0.0))
    Cs.sort_indices()
    Cs.data = signed_values(rng, Cs.nnz)
    return Cs


def from_mask(mask, rng):
    import scipy.sparse as sp
    Cs = sp.csc_matrix(np.where(mask, 1.0, 0.0))
    Cs.sort_indices()
    Cs.data = signed_values(rng, Cs.nnz)
    return Cs


def banded(rng, m, n, per_row):
    """row i holds columns (i * n // m + 0 .. per_row - 1) mod n"""
    import scipy.sparse as sp
    rows = np.repeat(np.arange(m), per_row)
    cols = ((np.arange(m) * n // m)[:, None] + np.arange(per_row)[None, :]).reshape(-1) % n
    Cs = sp.csc_matrix((np.ones(len(rows)), (rows, cols)), shape=(m, n))
    Cs.sort_indices()
    assert Cs.nnz == m * per_row
    Cs.data = signed_values(rng, Cs.nnz)
    return Cs


# ---- the pattern, by brute force
def pattern(Cs):
    """(pairs, lin_col): pairs = sorted [(j, k, [(ta, tb), ..])] for j <= k sharing a row, the products in ascending row order, ta / tb the
    nzval positions in columns j / k; lin_col = the non-empty columns"""
    m, n = Cs.shape
    rows = [[] for _ in range(m)]                       # per row: (column, nzval position), columns ascending
    for j in range(n):
        for t in range(Cs.indptr[j], Cs.indptr[j + 1]):
            rows[Cs.indices[t]].append((j, t))
    pairs = {}
    for i in range(m):                                  # ascending rows
        e = rows[i]
        for a in range(len(e)):
            for b in range(a, len(e)):
                pairs.setdefault((e[a][0], e[b][0]), []).append((e[a][1], e[b][1]))
    lin_col = [j for j in range(n) if Cs.indptr[j + 1] > Cs.indptr[j]]
    return [(j, k, pairs[(j, k)]) for j, k in sorted(pairs)], lin_col


def segment_sum(products):
    """the contract's two orders: fewer than 64 products left to right from the first, otherwise 64 lanes from 0.0 and the shuffle tree"""
    return run_sum_sequential(products) if len(products) < LONG else run_sum_wave(products, skip_empty=False)


def chain_tree_sum(values):
    """256 chains (chain t adds elements t, t + 256, .. in order, from 0.0), then the halving tree"""
    red = np.zeros(256)
    for t in range(256):
        s = 0.0
        for v in values[t::256]:
            s = s + float(v)
        red[t] = s
    h = 128
    while h:
        red[:h] = red[:h] + red[h:2 * h]
        h >>= 1
    return float(red[0])


def signed_consts(m, d, sign):
    if d is None or sign == 0:
        return np.zeros(m)
    return (0.0 + np.asarray(d, dtype=np.float64)) if sign > 0 else (0.0 - np.asarray(d, dtype=np.float64))


def restate(Cs, xvar, d=None, sign=0, moi=1, varmap=None, pat=None):
    """The contract restated: (quad[(coeff, row, col)], lin[(coeff, var)], constant) as numpy QT / LT arrays and a float"""
    from parametron_jl_amd._lib import LT, QT
    pairs, lin_col = pat or pattern(Cs)
    m = Cs.shape[0]
    v = Cs.data
    x = np.asarray(xvar, dtype=np.int64)
    idx = x if not moi else np.asarray(varmap, dtype=np.int64)[x - 1]
    c = signed_consts(m, d, sign)
    quad = np.zeros(len(pairs), dtype=QT)
    for s, (j, k, prods) in enumerate(pairs):
        acc = segment_sum([v[ta] * v[tb] for ta, tb in prods])
        quad[s] = (2.0 * acc if (moi or j != k) else acc, idx[j], idx[k])
    lin = np.zeros(len(lin_col), dtype=LT)
    for l, j in enumerate(lin_col):
        ts = range(Cs.indptr[j], Cs.indptr[j + 1])
        lin[l] = (2.0 * segment_sum([v[t] * c[Cs.indices[t]] for t in ts]), idx[j])
    const = chain_tree_sum(c * c) if (d is not None and sign != 0) else 0.0
    return quad, lin, const


# ---- the oracle: the reference's literal function restricted to the pattern
def oracle_function(Cs, xvar, d=None, sign=0, varmap=None):
    """(affine_terms, quadratic_terms, constant): vecdot!(residual, residual) of rows holding the structural terms only, canonicalize!, the
    MOI copy through varmap (None: identity)"""
    from oracle import oracle as O
    m, n = Cs.shape
    csr = Cs.tocsr()
    csr.sort_indices()
    c = signed_consts(m, d, sign)
    r = O.AffVec(m)
    for i in range(m):
        row = r[i]
        row.zero()
        for u in range(csr.indptr[i], csr.indptr[i + 1]):
            row.push(float(csr.data[u]), int(xvar[csr.indices[u]]))
        row.set_constant(float(c[i]))
    q = O.Quad().vecdot_affs_affs(r, r).canonicalize()
    return q.moi(varmap)


def bounds(Cs, d=None, sign=0, pat=None):
    """The derived tolerances: a coefficient is a sum of L products rounded identically on both sides; the oracle adds 2L numbers in its
    sort's order, the kernel L and doubles exactly, so |got - want| <= 4 L 2^-53 S with S = 2 sum |C[i,j] C[i,k]| (linear: |C[i,j] c_i|);
    the constant: 2 m 2^-53 sum c_i^2."""
    pairs, lin_col = pat or pattern(Cs)
    m = Cs.shape[0]
    v = Cs.data
    c = signed_consts(m, d, sign)
    bq = np.array([4 * len(p) * EPS * 2 * sum(abs(v[ta] * v[tb]) for ta, tb in p) for _, _, p in pairs])
    bl = np.array([4 * (Cs.indptr[j + 1] - Cs.indptr[j]) * EPS * 2 * sum(abs(v[t] * c[Cs.indices[t]]) for t in range(Cs.indptr[j], Cs.indptr[j + 1]))
                   for j in lin_col])
    bc = 2 * m * EPS * float(np.sum(c * c))
    return bq, bl, bc


def assert_close_to_oracle(quad, lin, const, oracle, bq, bl, bc):
    """indices and term counts exact, every coefficient within its bound; no case skipped or sampled"""
    at, qt, oc = oracle
    assert len(quad) == len(qt) and len(lin) == len(at)
    assert np.array_equal(quad["row"], qt["row"]) and np.array_equal(quad["col"], qt["col"]) and np.array_equal(lin["var"], at["var"])
    dq, dl = np.abs(quad["coeff"] - qt["coeff"]), np.abs(lin["coeff"] - at["coeff"])
    assert np.all(dq <= bq), (float(dq.max()), float(bq.min()))
    assert np.all(dl <= bl), (float(dl.max()) if len(dl) else 0.0)
    assert abs(const - oc) <= bc, (const, oc, bc)


def tables(Cs, cap=2048):
    """the library's symbolic phase for this pattern (host tables only)"""
    from parametron_jl_amd.device import SparseGramTables
    return SparseGramTables(None, Cs.shape[0], Cs.shape[1], Cs.indptr, Cs.indices, cap)


def vp(a):
    return a.ctypes.data_as(C.c_void_p)
