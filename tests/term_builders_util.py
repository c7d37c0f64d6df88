"""Vectorised numpy restatements of the reference's literal term builders, for the shapes at which building the oracle's objects element by
element would take seconds (tests/test_gpu_term_builders.py), and the data family those tests share.

Every function is written from the reference's loop (src/functions.jl, src/moi_interop.jl: cited per function) and from the contract in
include/parametron_hip.h — not from the kernels.  tests/test_term_builders_host.py checks each of them against the oracle bit for bit at
small shapes that have every feature of the large ones, and checks that wrong restatements are told apart.

Layouts: a uniform Vector{AffineFunction} is (terms, consts) with terms a (rows, L) array of LT and consts a (rows,) float64 array; variable
vectors are int64 arrays of 1-based indices; varmap[v - 1] is the optimizer's index of variable v."""
import numpy as np

from oracle import oracle as O

LT, QT, VAT = O.LT, O.QT, O.VAT

DENORMAL = 5e-324 * 3


def family(n, seed, lo=-0.5):
    """n doubles in [lo, lo + 1) with +0.0, -0.0, a denormal and a value of each sign planted where n allows"""
    a = O.fill_uniform(n, seed) + lo
    special = [0.0, -0.0, DENORMAL, -0.375, 0.625, -DENORMAL]
    if n >= len(special):
        for k, s in enumerate(special):
            a[(k * n) // len(special) + (1 if n > 2 * len(special) else 0)] = s
    else:
        a[:n] = special[:n]
    return a


def variables(n, seed, nvars=5):
    """n variable indices in 1..nvars: duplicates inside the vector, overlaps between vectors drawn with different seeds"""
    return np.random.default_rng(seed).integers(1, nvars + 1, size=n).astype(np.int64)


def permuting_varmap(nvars, seed):
    return np.random.default_rng(seed).permutation(nvars).astype(np.int64) + 101


def uniform_affvec(rows, L, seed, nvars=5):
    """(terms (rows, L) LT, consts (rows,)): coefficients and constants from `family`, every row with its own variables"""
    t = np.empty((rows, L), dtype=LT)
    t["coeff"] = family(rows * L, seed).reshape(rows, L)
    t["var"] = variables(rows * L, seed + 1, nvars).reshape(rows, L)
    return t, family(rows, seed + 2)


def oracle_affvec(terms, consts):
    """the oracle's Vector{AffineFunction} holding the rows of (terms, consts); `terms` may be a list of per-row LT arrays (ragged)"""
    L_ = O.lib()
    X = O.AffVec(len(consts))
    for i in range(len(consts)):
        h = L_.pmo_affvec_at(X.h, i)
        row = terms[i]
        for c, v in zip(row["coeff"].tolist(), row["var"].tolist()):
            L_.pmo_aff_push(h, c, v)
        L_.pmo_aff_set_constant(h, float(consts[i]))
    return X


def seq_sum(p):
    """((0.0 + p[0]) + p[1]) + ..: the reference's accumulation into a zeroed constant (src/functions.jl:574, :521)"""
    p = np.asarray(p, dtype=np.float64)
    return float(np.add.accumulate(np.concatenate(([0.0], p)))[-1])


def _mapped(varmap, v, moi=True):
    return varmap[v - 1] if (moi and varmap is not None) else v


def _qt(coeff, row, col):
    out = np.empty(coeff.shape, dtype=QT)
    out["coeff"], out["row"], out["col"] = coeff, row, col
    return out.reshape(-1)


def _lt(coeff, var):
    out = np.empty(coeff.shape, dtype=LT)
    out["coeff"], out["var"] = coeff, var
    return out.reshape(-1)


def moi_quad(q, varmap):
    """update!(::MOI.ScalarQuadraticFunction) src/moi_interop.jl:53-60: 2 * coeff where rowvar == colvar, indices through varmap"""
    return _qt(np.where(q["row"] == q["col"], 2 * q["coeff"], q["coeff"]), _mapped(varmap, q["row"]), _mapped(varmap, q["col"]))


def moi_lin(t, varmap):
    """src/moi_interop.jl:39-42"""
    return _lt(t["coeff"].copy(), _mapped(varmap, t["var"]))


def bilinear(Q, xvar, yvar, moi=0, varmap=None):
    """bilinearmul! src/functions.jl:840-858: quadratic[k] = (Q[k], x[row], y[col]) with k counting up over (row, col) in ROW-major order
    while Q[k] is the matrix's column-major LINEAR index"""
    rows, cols = Q.shape
    lin = np.ascontiguousarray(Q.T).reshape(-1)
    k = np.arange(rows * cols)
    q = _qt(lin[k], xvar[k // cols], yvar[k % cols])
    return moi_quad(q, varmap) if moi else q


def quad_expand(xt, xc, yt, yc, moi=0, varmap=None):
    """_vecdot!(::QuadraticFunction, x, y) src/functions.jl:702-709 over muladd!(dest, ::AffineFunction, ::AffineFunction) :548-576, uniform
    rows: per row the products x.linear[a] * y.linear[b] (a outer), then x.linear * y.constant, then y.linear * x.constant; the constant
    accumulated over the rows in order"""
    rows, nx = xt.shape
    ny = yt.shape[1]
    shape = (rows, nx, ny)
    q = _qt(xt["coeff"][:, :, None] * yt["coeff"][:, None, :], np.broadcast_to(xt["var"][:, :, None], shape), np.broadcast_to(yt["var"][:, None, :], shape))
    lin = _lt(np.concatenate([xt["coeff"] * yc[:, None], yt["coeff"] * xc[:, None]], axis=1), np.concatenate([xt["var"], yt["var"]], axis=1))
    const = seq_sum(xc * yc)
    if moi:
        return moi_quad(q, varmap), moi_lin(lin, varmap), const
    return q, lin, const


def vecdot_affs_vars(xt, xc, yvar, moi=0, varmap=None):
    """_vecdot! :702-709 over muladd!(dest, ::AffineFunction, ::Variable) src/functions.jl:537-546: per row the terms x.linear[a] * y, then
    the linear term (x.constant, y)"""
    q = _qt(xt["coeff"].copy(), xt["var"], np.broadcast_to(yvar[:, None], xt.shape))
    lin = _lt(xc.copy(), yvar)
    if moi:
        return moi_quad(q, varmap), moi_lin(lin, varmap)
    return q, lin


def affvec_scale(yt, yc, s):
    """scale!(dest, x::Number, y::Vector{AffineFunction}) src/functions.jl:895-915 -> muladd! :515-523 into a zeroed dest"""
    return _lt(s * yt["coeff"], yt["var"]), 0.0 + yc * s


def matvecmul_affs(A, xt, xc):
    """matvecmul!(y, A, x::Vector{AffineFunction}) src/functions.jl:800-822: y[row] accumulates A[row, col] * x[col] over col in order"""
    rows, cols = A.shape
    L = xt.shape[1]
    terms = _lt(A[:, :, None] * xt["coeff"][None, :, :], np.broadcast_to(xt["var"][None, :, :], (rows, cols, L)))
    prods = xc[None, :] * A
    consts = np.add.accumulate(np.concatenate([np.zeros((rows, 1)), prods], axis=1), axis=1)[:, -1]
    return terms, consts


def vecdot_numbers_affs(v, xt, xc):
    """_vecdot!(::AffineFunction, numbers, affs) src/functions.jl:665-674 -> muladd! :524 -> :515-523"""
    return _lt(v[:, None] * xt["coeff"], xt["var"]), seq_sum(xc * v)


def quad_combine(qa, qb, sb):
    """copyto! src/functions.jl:434-439 then add! :459 / subtract! :492-500 on the quadratic lists: [qa ; sb * qb]"""
    b = qb.copy()
    if sb < 0:
        b["coeff"] = -b["coeff"]
    return np.concatenate([qa, b])


def quad_scale(q, s):
    """muladd!(dest::QuadraticFunction, x::QuadraticFunction, y::Number) src/functions.jl:526-534"""
    return _qt(s * q["coeff"], q["row"], q["col"])


def affvec_combine(xa, ca, xb, cb, sb):
    """vecadd!/vecsubtract! src/functions.jl:751-764 on uniform rows: copyto! :419-427 of part a (None: absent), then add! :452-455 /
    subtract! :474-485 of part b; a part without constants contributes none"""
    rows = len(ca if ca is not None else cb if cb is not None else (xa if xa is not None else xb))
    parts = []
    if xa is not None:
        parts.append(xa.copy())
    if xb is not None:
        b = xb.copy()
        if sb < 0:
            b["coeff"] = -b["coeff"]
        parts.append(b)
    terms = np.concatenate(parts, axis=1).reshape(-1) if parts else np.empty(0, dtype=LT)
    c = ca.copy() if ca is not None else np.zeros(rows)
    if cb is not None:
        c = c - cb if sb < 0 else c + cb
    return terms, c


# ---- deliberately wrong restatements (tests/test_term_builders_host.py shows that each is rejected)
def wrong_bilinear_row_col(Q, xvar, yvar, moi=0, varmap=None):
    """Q[row, col] in place of Q[k]"""
    rows, cols = Q.shape
    k = np.arange(rows * cols)
    q = _qt(Q[k // cols, k % cols], xvar[k // cols], yvar[k % cols])
    return moi_quad(q, varmap) if moi else q


def wrong_bilinear_matrix_diagonal(Q, xvar, yvar, moi=0, varmap=None):
    """the doubling on the matrix's diagonal instead of on equal variables"""
    rows, cols = Q.shape
    q = bilinear(Q, xvar, yvar)
    if not moi:
        return q
    k = np.arange(rows * cols)
    return _qt(np.where(k // cols == k % cols, 2 * q["coeff"], q["coeff"]), _mapped(varmap, q["row"]), _mapped(varmap, q["col"]))


def wrong_pairwise_sum(p):
    """a pairwise tree in place of the left-to-right sum"""
    p = np.concatenate(([0.0], np.asarray(p, dtype=np.float64)))
    while len(p) > 1:
        if len(p) % 2:
            p = np.concatenate((p, [0.0]))
        p = p[0::2] + p[1::2]
    return float(p[0])


def wrong_quad_combine_negates_a(qa, qb, sb):
    """the negation applied to part a"""
    a = qa.copy()
    if sb < 0:
        a["coeff"] = -a["coeff"]
    return np.concatenate([a, qb])
