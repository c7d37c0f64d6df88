"""CPU suite: the numpy restatements of the literal term builders (tests/term_builders_util.py), which the GPU tests use where the oracle's
objects would take seconds to build, against the oracle bit for bit — at small shapes that have every feature of the large ones: a
non-square Q, different x and y, duplicate and shared variables, a permuting varmap, signed zeros and a denormal.  And four wrong
restatements, each of which the same comparison tells apart."""
import ctypes as C

import numpy as np
import pytest

import term_builders_util as T
from oracle import oracle as O


def same_terms(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


NV = 5
VM = T.permuting_varmap(NV, 3)
BILINEAR_SHAPES = [(1, 1), (3, 5), (5, 3), (4, 4), (7, 33)]


def _bilinear_inputs(rows, cols):
    Q = T.family(rows * cols, 10 + rows).reshape(cols, rows).T.copy()
    x, y = T.variables(rows, 1, NV), T.variables(cols, 2, NV)
    y[0] = x[0]
    return Q, x, y


def test_the_data_family_has_signed_zeros_a_denormal_and_both_signs():
    a = T.family(40, 1)
    bits = a.view(np.int64)
    assert np.any(bits == 0) and np.any(bits == np.int64(-2 ** 63)) and np.any(a == T.DENORMAL) and np.any(a > 0.1) and np.any(a < -0.1)
    x, y = T.variables(40, 1), T.variables(40, 2)
    assert len(set(x)) < len(x) and set(x) & set(y) and not np.array_equal(x, y)
    assert not np.array_equal(VM, np.sort(VM))


@pytest.mark.parametrize("rows,cols", BILINEAR_SHAPES)
def test_bilinear_restatement(rows, cols):
    Q, x, y = _bilinear_inputs(rows, cols)
    ref = O.Quad().bilinearmul(Q, x, y)
    assert same_terms(T.bilinear(Q, x, y), ref.terms())
    assert same_terms(T.bilinear(Q, x, y, 1, VM), ref.moi(VM)[1])


@pytest.mark.parametrize("rows,nx,ny", [(1, 1, 1), (5, 2, 3), (9, 4, 1), (70, 3, 2), (3, 0, 2)])
def test_quad_expand_restatement(rows, nx, ny):
    xt, xc = T.uniform_affvec(rows, nx, 20, NV)
    yt, yc = T.uniform_affvec(rows, ny, 30, NV)
    ref = O.Quad().vecdot_affs_affs(T.oracle_affvec(xt, xc), T.oracle_affvec(yt, yc))
    q, lin, const = T.quad_expand(xt, xc, yt, yc)
    assert same_terms(q, ref.terms()) and same_terms(lin, ref.affine.terms()) and same_bits([const], [ref.affine.constant])
    at, qt, c = ref.moi(VM)
    q, lin, const = T.quad_expand(xt, xc, yt, yc, 1, VM)
    assert same_terms(q, qt) and same_terms(lin, at) and same_bits([const], [c])
    # x . x
    ref = O.Quad().vecdot_affs_affs(T.oracle_affvec(xt, xc), T.oracle_affvec(xt, xc))
    at, qt, c = ref.moi(VM)
    q, lin, const = T.quad_expand(xt, xc, xt, xc, 1, VM)
    assert same_terms(q, qt) and same_terms(lin, at) and same_bits([const], [c])


@pytest.mark.parametrize("rows,L", [(1, 1), (6, 4), (5, 0), (17, 3)])
def test_affine_vector_restatements(rows, L):
    xt, xc = T.uniform_affvec(rows, L, 40, NV)
    X = T.oracle_affvec(xt, xc)
    yv = T.variables(rows, 7, NV)
    # AffineFunction[] . Variable[]
    ref = O.Quad().vecdot_affs_vars(X, yv)
    q, lin = T.vecdot_affs_vars(xt, xc, yv)
    assert same_terms(q, ref.terms()) and same_terms(lin, ref.affine.terms())
    at, qt, _ = ref.moi(VM)
    q, lin = T.vecdot_affs_vars(xt, xc, yv, 1, VM)
    assert same_terms(q, qt) and same_terms(lin, at)
    # s * X for a scalar of each sign and both zeros
    for s in (-1.75, 0.0, -0.0, 3.0):
        terms, _, consts = O.AffVec(rows).scale_number_affs(s, X).flat()
        t, c = T.affvec_scale(xt, xc, s)
        assert same_terms(t, terms) and same_bits(c, consts)
    # A * X
    m = 4
    A = T.family(m * rows, 41).reshape(rows, m).T.copy()
    terms, _, consts = O.AffVec(m).matvecmul_affs(A, X).flat()
    t, c = T.matvecmul_affs(A, xt, xc)
    assert same_terms(t, terms) and same_bits(c, consts)
    # numbers . X
    v = T.family(rows, 42)
    r = O.vecdot_aff_numbers_affs(v, X)
    t, c = T.vecdot_numbers_affs(v, xt, xc)
    assert same_terms(t, r.terms()) and same_bits([c], [r.constant])
    # X (+|-) Y, numbers - X, X alone
    yt, yc = T.uniform_affvec(rows, L + 1, 50, NV)
    Y = T.oracle_affvec(yt, yc)
    for sb in (1, -1):
        terms, _, consts = O.AffVec(rows).vecaddsub(X, Y, subtract=sb < 0).flat()
        t, c = T.affvec_combine(xt, xc, yt, yc, sb)
        assert same_terms(t, terms) and same_bits(c, consts)
        terms, _, consts = O.AffVec(rows).vecaddsub(v, X, subtract=sb < 0).flat()
        t, c = T.affvec_combine(None, v, xt, xc, sb)
        assert same_terms(t, terms) and same_bits(c, consts)
    t, c = T.affvec_combine(xt, xc, None, None, 1)
    assert same_terms(t, X.flat()[0]) and same_bits(c, xc)


def _quad_of(q):
    return O.Quad(quad=[(float(c), int(r), int(cl)) for c, r, cl in zip(q["coeff"], q["row"], q["col"])])


@pytest.mark.parametrize("na,nb", [(0, 5), (5, 0), (7, 9), (1, 1)])
def test_quadratic_list_restatements(na, nb):
    Q, x, y = _bilinear_inputs(4, 4)
    pool = T.bilinear(Q, x, y)
    qa, qb = pool[:na].copy(), pool[16 - nb:].copy()
    A, B = _quad_of(qa), _quad_of(qb)
    assert same_terms(T.quad_combine(qa, qb, 1), O.Quad().copy_from(A).add_quad(B).terms())
    assert same_terms(T.quad_combine(qa, qb, -1), O.Quad().copy_from(A).sub_quad(B).terms())
    for s in (-1.75, -0.0, 2.0):
        assert same_terms(T.quad_scale(pool, s), O.Quad().mul_quad_number(_quad_of(pool), s).terms())
    assert same_terms(T.moi_quad(pool, VM), _quad_of(pool).moi(VM)[1])
    aff = O.Aff(terms=[(float(c), int(v)) for c, v in zip(qa["coeff"], qa["row"])])
    lt = np.empty(na, dtype=T.LT)
    lt["coeff"], lt["var"] = qa["coeff"], qa["row"]
    assert same_terms(T.moi_lin(lt, VM), O.aff_moi(aff, VM)[0])


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 129, 200])
def test_left_to_right_sum_restatement(n):
    """against a plain Python loop and against the oracle's constant of numbers . affs (src/functions.jl:521)"""
    p = T.family(n, 60) * 1e3
    acc = 0.0
    for v in p:
        acc = acc + v
    assert same_bits([T.seq_sum(p)], [acc])
    assert same_bits([T.seq_sum([-0.0])], [0.0])                    # 0.0 + -0.0
    xt, xc = T.uniform_affvec(n, 0, 61, NV)
    v = T.family(n, 62)
    assert same_bits([T.vecdot_numbers_affs(v, xt, xc)[1]], [O.vecdot_aff_numbers_affs(v, T.oracle_affvec(xt, xc)).constant])


def test_scale_numbers_and_scale_vars_are_single_products():
    y = T.family(40, 70)
    out = np.empty(40)
    for s in (-2.75, -0.0):
        assert O.lib().pmo_scale_number_numbers(out.ctypes.data_as(C.c_void_p), 40, s, y.ctypes.data_as(C.c_void_p), 40) == 0
        assert same_bits(s * y, out)


# ---- wrong restatements are rejected by the same comparisons
def test_wrong_bilinear_restatements_are_rejected():
    for rows, cols in [(3, 5), (5, 3), (4, 4), (7, 33)]:
        Q, x, y = _bilinear_inputs(rows, cols)
        ref = O.Quad().bilinearmul(Q, x, y)
        assert not same_terms(T.wrong_bilinear_row_col(Q, x, y), ref.terms()), (rows, cols)
        assert same_terms(T.wrong_bilinear_matrix_diagonal(Q, x, y), ref.terms())            # (identical without the MOI copy ...)
        assert not same_terms(T.wrong_bilinear_matrix_diagonal(Q, x, y, 1, VM), ref.moi(VM)[1]), (rows, cols)   # ... and told apart with it


def test_wrong_sum_order_is_rejected():
    for n in (65, 129, 200):
        xt, xc = T.uniform_affvec(n, 0, 61, NV)
        v = T.family(n, 62)
        want = O.vecdot_aff_numbers_affs(v, T.oracle_affvec(xt, xc)).constant
        assert same_bits([T.seq_sum(xc * v)], [want])
        assert not same_bits([T.wrong_pairwise_sum(xc * v)], [want]), n


def test_wrong_negated_part_is_rejected():
    Q, x, y = _bilinear_inputs(4, 4)
    pool = T.bilinear(Q, x, y)
    qa, qb = pool[:7].copy(), pool[7:].copy()
    want = O.Quad().copy_from(_quad_of(qa)).sub_quad(_quad_of(qb)).terms()
    assert same_terms(T.quad_combine(qa, qb, -1), want)
    assert not same_terms(T.wrong_quad_combine_negates_a(qa, qb, -1), want)
