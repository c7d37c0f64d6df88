"""CPU-only: the host side of the sparse quadratic form transpose(x)*Q*x (record modes "canonical-sparse-form" and, beside sparse blocks,
"canonical-sparse-sum") — the Python restatement of the contract against the oracle word for word, the symbolic phase
(pmt_sparse_form_count / _order) against the restatement's tables, every refusal before any device call, the quad_plan rows, the errors of
the bilinear rule, the record a "canonical-sparse-form" plan compiles (stub context), and a sum with a form against the oracle composition
within the derived bound."""
import ctypes as C

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")

import __graft_entry__ as entry  # noqa: E402
import sparse_form_util as U  # noqa: E402
import sparse_gram_util as SG  # noqa: E402
import sparse_sum_util as SU  # noqa: E402
from sparse_sum_util import Term  # noqa: E402
from test_record_tape_host import VARMAP_BUF, StubContext, _b, _block, _form, _model, _objective, _quad_out, _xvars  # noqa: E402
from test_sparse_gram_host import _sparse_block  # noqa: E402
from test_stacked_lsq_host import FAKE  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


def _unsymmetric():
    """6 x 6 by hand: (0,1) stored twice, (0,2) upper only, (1,3) lower only (entry (3,1)), the diagonal at 0 (a -0.0), 2 and 4, (2,4) twice
    with a 0.0 and a -0.0, (3,4) lower only holding -0.0, column 5 and row 5 empty"""
    rows = [0, 0, 1, 0, 3, 2, 4, 2, 4, 4]
    cols = [0, 1, 0, 2, 1, 2, 4, 4, 2, 3]
    vals = [-0.0, 1.5, -2.25, 0.75, 3.0, 0.0, -1.0, 0.0, -0.0, -0.0]
    return U.from_entries(6, rows, cols, vals)


def _patterns():
    rng = np.random.default_rng(16)
    out = {kind: U.pattern(kind, 12, rng) for kind in U.KINDS}
    out["unsymmetric by hand"] = _unsymmetric()
    out["n = 1"] = U.from_entries(1, [0], [0], [-0.0])
    out["n = 0"] = sp.csc_matrix((0, 0), dtype=np.float64)
    return out


PATTERNS = _patterns()


def _xvar_varmap(n, seed=3):
    rng = np.random.default_rng(seed)
    xvar = np.sort(rng.choice(np.arange(1, n + 6), n, replace=False)).astype(np.int64)
    vm = rng.permutation(n + 5).astype(np.int64) + 1 + int(rng.integers(0, 4))
    return xvar, vm


# ---- 1. the restatement against the oracle, before any GPU sees it
@pytest.mark.parametrize("name", list(PATTERNS))
def test_restatement_matches_the_oracle_word_for_word(lib, name):
    Q = PATTERNS[name]
    n = Q.shape[0]
    xvar, vm = _xvar_varmap(n)
    at, qt, const = U.oracle_function(Q, xvar, vm)
    assert len(at) == 0 and const == 0.0 and not np.signbit(const)
    U.assert_same_words(U.restate(Q, xvar, 1, vm), U.ordered_words(qt, xvar, vm), name)
    # moi = 0: canonicalize! alone — native indices, the diagonal undoubled
    ident = np.arange(1, n + 7, dtype=np.int64)
    native = U.oracle_quad(Q, xvar).canonicalize().terms()
    U.assert_same_words(U.restate(Q, xvar, 0), U.ordered_words(native, xvar, ident), name + " (moi = 0)")


def test_restatement_details_by_hand(lib):
    Q = _unsymmetric()
    pj, pk, sa, sb = U.tables(Q)
    assert list(zip(pj.tolist(), pk.tolist())) == [(0, 0), (0, 1), (0, 2), (1, 3), (2, 2), (2, 4), (3, 4), (4, 4)]
    N = U.NONE
    assert [(a == N, b == N) for a, b in zip(sa, sb)] == [(False, True), (False, False), (False, True), (True, False), (False, True), (False, False),
                                                          (True, False), (False, True)]
    c = U.coefficients(Q.data, (pj, pk, sa, sb), 1)
    assert c.tolist() == [-0.0, -0.75, 0.75, 3.0, 0.0, 0.0, -0.0, -2.0]
    assert np.signbit(c).tolist() == [True, True, False, False, False, False, True, True]     # lone -0.0 stays; 0.0 + -0.0 = 0.0; 2 * -0.0 = -0.0
    assert U.coefficients(Q.data, (pj, pk, sa, sb), 0)[-1] == -1.0
    # the oracle keeps the lone lower-triangle entries in stored order (row k, column j): the one departure
    xvar, ident = np.arange(1, 7), np.arange(1, 7)
    qt = U.oracle_function(Q, xvar, ident)[1]
    assert (int(qt["row"][3]), int(qt["col"][3])) == (4, 2) and (int(qt["row"][6]), int(qt["col"][6])) == (5, 4)
    r = U.restate(Q, xvar, 1, ident)
    assert (int(r["row"][3]), int(r["col"][3])) == (2, 4) and (int(r["row"][6]), int(r["col"][6])) == (4, 5)


# ---- 2. the symbolic phase
def _assert_tables(Q, what):
    T = U.form_tables(Q)
    pj, pk, sa, sb = U.tables(Q)
    assert T.nq == len(pj), what
    for got, want, name in ((T.pair_j, pj, "pair_j"), (T.pair_k, pk, "pair_k"), (T.src_a, sa, "src_a"), (T.src_b, sb, "src_b")):
        assert got.dtype == np.uint32 and np.array_equal(got, want), (what, name)
    assert not np.any((T.src_a == U.NONE) & (T.src_b == U.NONE))
    assert T.nlin == 0 and len(T.lin_col) == 0 and T.dev is None


@pytest.mark.parametrize("name", list(PATTERNS))
def test_symbolic_phase_equals_the_restatement(lib, name):
    _assert_tables(PATTERNS[name], name)


def test_symbolic_phase_on_random_patterns(lib):
    rng = np.random.default_rng(1600)
    for t in range(300):
        n = int(rng.integers(0, 41))
        kind = U.KINDS[t % len(U.KINDS)]
        _assert_tables(U.pattern(kind, n, rng, density=float(rng.choice([0.05, 0.2, 0.6, 1.0])), zeros=False), (t, kind, n))


# ---- 3. refusals, no GPU present
def _count(lib, n, colptr, rowval):
    nq = C.c_int64(-7)
    colptr = None if colptr is None else np.asarray(colptr, dtype=np.int64)
    rowval = None if rowval is None else np.asarray(rowval, dtype=np.int64)
    lib.call("pmt_sparse_form_count", n, None if colptr is None else SG.vp(colptr), None if rowval is None else SG.vp(rowval), C.byref(nq))
    return nq.value


POISON = 0xABABABAB


def _outputs(nq):
    return [np.full(max(nq, 1) + 2, POISON, dtype=np.uint32) for _ in range(4)]


def _order(lib, n, colptr, rowval, nq, null=None, out=None):
    colptr, rowval = np.asarray(colptr, dtype=np.int64), np.asarray(rowval, dtype=np.int64)
    out = _outputs(nq) if out is None else out
    args = [None if null == i else SG.vp(a) for i, a in enumerate(out)]
    lib.call("pmt_sparse_form_order", n, SG.vp(colptr), SG.vp(rowval), nq, *args)
    return out


GOOD = (3, [1, 3, 4, 6], [1, 3, 2, 1, 3])       # 3 x 3, 1-based: entries (1,1) (3,1) (2,2) (1,3) (3,3): pairs (0,0) (0,2) (1,1) (2,2)


def test_symbolic_phase_refusals(lib):
    n, cp, rv = GOOD
    assert _count(lib, n, cp, rv) == 4
    out = _order(lib, n, cp, rv, 4)
    assert out[0][:4].tolist() == [0, 0, 1, 2] and out[1][:4].tolist() == [0, 2, 1, 2] and out[2][:4].tolist() == [0, 3, 2, 4]
    assert out[3][:4].tolist() == [U.NONE, 1, U.NONE, U.NONE] and all(np.all(a[4:] == POISON) for a in out)       # nothing beyond nq
    bad = {"0-based colptr": (lib.ArgumentError, (n, [0, 2, 3, 5], rv)),
           "colptr not monotone": (lib.ArgumentError, (n, [1, 4, 3, 6], rv)),
           "rows not ascending": (lib.ArgumentError, (n, cp, [3, 1, 2, 1, 3])),
           "a repeated row": (lib.ArgumentError, (n, cp, [1, 1, 2, 1, 3])),
           "row 0": (lib.DimensionMismatch, (n, cp, [0, 3, 2, 1, 3])),
           "row n + 1": (lib.DimensionMismatch, (n, cp, [1, 4, 2, 1, 3])),
           "n < 0": (lib.DimensionMismatch, (-1, cp, rv)),
           "n = 2^31": (lib.DimensionMismatch, (1 << 31, cp, rv))}
    for name, (exc, a) in bad.items():
        with pytest.raises(exc):
            _count(lib, *a)
        out = _outputs(4)
        with pytest.raises(exc):
            _order(lib, *a, 4, out=out)
        assert all(np.all(o == POISON) for o in out), name                   # checked before anything is written
    # 2^32 - 1 non-zeros (colptr alone says so: refused before rowval is read)
    big = [1, 1 << 32]
    with pytest.raises(lib.DimensionMismatch, match="non-zeros"):
        _count(lib, 1, big, [1])
    with pytest.raises(lib.DimensionMismatch, match="non-zeros"):
        _order(lib, 1, big, [1], 1)
    # null pointers
    with pytest.raises(lib.ArgumentError, match="null"):
        _count(lib, n, None, rv)
    with pytest.raises(lib.ArgumentError, match="null"):
        _count(lib, n, cp, None)
    with pytest.raises(lib.ArgumentError, match="null"):
        lib.call("pmt_sparse_form_count", n, SG.vp(np.asarray(cp, dtype=np.int64)), SG.vp(np.asarray(rv, dtype=np.int64)), None)
    for i in range(4):
        with pytest.raises(lib.ArgumentError, match="null"):
            _order(lib, n, cp, rv, 4, null=i)
    # an nq that is not that of _count: nothing is written
    for nq in (3, 5, 0, -1):
        out = _outputs(8)
        with pytest.raises(lib.DimensionMismatch, match="nq"):
            _order(lib, n, cp, rv, nq, out=out)
        assert all(np.all(o == POISON) for o in out)
    # nnz = 0 and n = 0 are patterns like any other
    assert _count(lib, 3, [1, 1, 1, 1], None) == 0 and _count(lib, 0, [1], None) == 0
    lib.call("pmt_sparse_form_order", 3, SG.vp(np.ones(4, dtype=np.int64)), None, 0, None, None, None, None)


def _form_call(lib, **kw):
    a = dict(nzval=FAKE, src_a=FAKE, src_b=FAKE, pair_j=FAKE, pair_k=FAKE, nq=5, xvar=FAKE, moi=1, varmap=FAKE, out_quad=FAKE, out_const=FAKE)
    a.update(kw)
    lib.call("pmt_sparse_form_f64", *a.values(), None)


def test_entry_point_validates_before_any_device_call(lib):
    for name in ("nzval", "src_a", "src_b", "pair_j", "pair_k", "xvar", "out_quad"):
        with pytest.raises(lib.ArgumentError, match="null"):
            _form_call(lib, **{name: None})
        with pytest.raises(lib.ArgumentError, match="null"):
            _form_call(lib, **{name: None, "out_const": None})
    with pytest.raises(lib.ArgumentError, match="negative"):
        _form_call(lib, nq=-1)
    for moi in (2, -1):
        with pytest.raises(lib.ArgumentError, match="moi"):
            _form_call(lib, moi=moi)
    with pytest.raises(lib.ArgumentError, match="varmap"):
        _form_call(lib, varmap=None)
    # nq = 0 without a constant: a valid call that writes nothing and reaches no device
    _form_call(lib, nq=0, out_const=None, nzval=None, src_a=None, src_b=None, pair_j=None, pair_k=None, xvar=None, out_quad=None)
    _form_call(lib, nq=0, out_const=None, moi=0, varmap=None)


# ---- 4. quad_plan
def _sparse_form(Q, idx, ctx=None):
    """a SparseQuadForm without a device: the fields quad_plan and the compile steps read"""
    from parametron_jl_amd.device import DSpMat
    from parametron_jl_amd.lazyexpression import SparseQuadForm
    Q = U.csc(Q)
    spm = DSpMat.__new__(DSpMat)
    spm.rows, spm.cols, spm.nnz, spm.narrow, spm.buf, spm._gram, spm._form = Q.shape[0], Q.shape[1], Q.nnz, True, FAKE, None, None
    spm.indptr, spm.indices = Q.indptr.copy(), Q.indices.copy()
    return SparseQuadForm(ctx, spm, _xvars(idx))


def _q9(seed=7):
    return U.pattern("mixed", 9, np.random.default_rng(seed))


def test_quad_plan_rows_of_a_sparse_form(lib):
    from parametron_jl_amd.lazyexpression import LsqTerm
    from parametron_jl_amd.moi import quad_plan
    idx = np.arange(2, 11)
    form = _sparse_form(_q9(), idx)
    one = [LsqTerm("form", r=form)]
    vm = np.arange(1, 20, dtype=np.int64)[::-1].copy()                      # a map under which x does NOT keep its order
    for mode in ("auto", "canonical"):
        for small in (True, False):
            for handoff in ("moi", "device"):
                for is_objective in (True, False):
                    for sums in (True, False):
                        p = quad_plan(one, True, "quad", form.spmat.nnz, is_objective, mode, small, handoff, vm, sparse_sums=sums)
                        assert p.mode == "canonical-sparse-form" and p.form is form and not p.canonicalize and not p.gram_record
    for mode, handoff in (("literal", "moi"), ("literal", "device"), ("auto", "host_csc"), ("canonical", "host_csc")):
        with pytest.raises(lib.ArgumentError, match="sparse Q"):
            quad_plan(one, True, "quad", 9, True, mode, False, handoff, vm, sparse_sums=True)
    # a dense form keeps its rows
    dense = [LsqTerm("form", r=_form(9, idx))]
    assert quad_plan(dense, True, "quad", 81, True, "canonical", False, "moi", None, sparse_sums=True).mode == "canonical-form"
    assert quad_plan(dense, True, "quad", 81, True, "auto", False, "moi", None, sparse_sums=True).mode == "literal"


def test_quad_plan_rows_of_sums_with_a_sparse_form(lib):
    from parametron_jl_amd.lazyexpression import LsqTerm
    from parametron_jl_amd.moi import _lsq_groups, _lsq_sum_combines, _sparse_sum_combines, quad_plan
    idx = np.arange(2, 11)
    f1, f2 = _sparse_form(_q9(7), idx), _sparse_form(_q9(8), idx)
    rng = np.random.default_rng(5)
    r1 = _sparse_block(SG.from_mask(rng.random((40, 9)) < 0.3, rng), idx)
    vm = np.arange(1, 20, dtype=np.int64)
    sums = {"beside a sparse block": [LsqTerm("block", r=r1), LsqTerm("form", r=f1)],
            "qp": [LsqTerm("form", r=f1, scale=0.5), LsqTerm("linear", xvars=f1.xvars, vec=_b(9)), LsqTerm("constant", value=object())],
            "ridge": [LsqTerm("form", r=f1), LsqTerm("diag", xvars=f1.xvars, param=object())],
            "two forms": [LsqTerm("form", r=f1), LsqTerm("form", r=f2)],
            "a diagonal part": [LsqTerm("form", r=f1), LsqTerm("diag", xvars=_xvars([3, 5, 9]), scale=-0.5)],
            "weighted": [LsqTerm("form", r=f1, param=object())],
            "eight": [LsqTerm("form", r=f1)] * 4 + [LsqTerm("block", r=r1)] * 4}
    for name, terms in sums.items():
        assert _sparse_sum_combines(terms) and not _lsq_sum_combines(terms), name
        for mode in ("auto", "canonical"):
            for small in (True, False):
                for handoff in ("moi", "device"):
                    for is_objective in (True, False):
                        p = quad_plan(terms, False, "quad", 99, is_objective, mode, small, handoff, vm, sparse_sums=True)
                        assert p.mode == "canonical-sparse-sum" and p.terms is terms and not p.gram_record, name
    # a dense block or a dense form beside a sparse form; forms over different x; nine blocks and forms: no canonical sum of either kind
    dense_block, dense_form = _block(30, idx), _form(9, idx)
    others = {"dense block beside": [LsqTerm("form", r=f1), LsqTerm("block", r=dense_block)],
              "dense form beside": [LsqTerm("form", r=dense_form), LsqTerm("form", r=f1)],
              "different x": [LsqTerm("form", r=f1), LsqTerm("form", r=_sparse_form(_q9(8), np.arange(3, 12)))],
              "disjoint x": [LsqTerm("form", r=f1), LsqTerm("form", r=_sparse_form(_q9(8), np.arange(20, 29)))],
              "nine": [LsqTerm("form", r=f1)] * 5 + [LsqTerm("block", r=r1)] * 4}
    for name, terms in others.items():
        assert not _sparse_sum_combines(terms) and not _lsq_sum_combines(terms) and _lsq_groups(terms) is None, name
        for small in (True, False):
            for mode in ("auto", "canonical"):
                p = quad_plan(terms, False, "quad", 1 << 20, True, mode, small, "moi", vm, sparse_sums=True)
                assert p.mode == "literal" and p.mode not in ("canonical-sum", "canonical-sparse-sum", "canonical-groups"), name


# ---- 5. the bilinear rule
def _rule_case(n=6, idx=None):
    import parametron_jl_amd as P
    model = _model()
    x = [P.Variable(model) for _ in range(n + 2)]
    Q = U.pattern("mixed", n, np.random.default_rng(3))
    return P, model, x, Q


def test_rule_bilinear_takes_a_sparse_parameter_and_says_why_not(lib):
    from parametron_jl_amd.lazyexpression import SparseQuadForm, _NoLiteralQuad, _rule_bilinear
    P, model, x, Q = _rule_case()
    ctx = StubContext(lib)
    Qp = P.Parameter(lambda: Q, model)
    node = _rule_bilinear(model, ctx, x[:6], Qp, x[:6])
    assert node.lsq_bare and len(node.lsq_sum) == 1 and node.lsq_sum[0].kind == "form" and isinstance(node.lsq_sum[0].r, SparseQuadForm)
    assert isinstance(node.out, _NoLiteralQuad) and (node.out.nq, node.out.nl) == (Q.nnz, 0)
    assert node.lsq_sum[0].r.xvars.vars.tolist() == [1, 2, 3, 4, 5, 6] and node.lsq_sum[0].r.spmat.nnz == Q.nnz
    with pytest.raises(lib.ArgumentError, match="sparse Q has no literal form"):
        node.out.materialize()
    # non-square / wrong size: the reference's DimensionMismatch
    with pytest.raises(lib.DimensionMismatch, match=r"bilinearmul!: size\(Q\) != \(length\(x\), length\(y\)\)"):
        _rule_bilinear(model, ctx, x[:5], Qp, x[:5])
    rect = P.Parameter(lambda: sp.csc_matrix(np.ones((6, 5))), model)
    with pytest.raises(lib.DimensionMismatch, match="bilinearmul!"):
        _rule_bilinear(model, ctx, x[:6], rect, x[:6])
    with pytest.raises(lib.ArgumentError, match="same Variable vector"):
        _rule_bilinear(model, ctx, x[:6], Qp, x[1:7])
    with pytest.raises(lib.ArgumentError, match="strictly increasing"):
        _rule_bilinear(model, ctx, x[:6][::-1], Qp, x[:6][::-1])
    with pytest.raises(lib.ArgumentError, match="strictly increasing"):
        _rule_bilinear(model, ctx, x[:5] + x[4:5], Qp, x[:5] + x[4:5])
    # a pattern that is not canonical (rows descending in a column)
    raw = sp.csc_matrix((np.ones(3), np.array([2, 0, 1]), np.array([0, 2, 3, 3, 3, 3, 3])), shape=(6, 6))
    with pytest.raises(lib.ArgumentError, match="canonical CSC"):
        _rule_bilinear(model, ctx, x[:6], P.Parameter(lambda: raw, model), x[:6])


# ---- the record
@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("mapped", [False, True])
def test_canonical_sparse_form_record_tape(lib, small, mapped):
    from parametron_jl_amd.moi import QuadPlan
    Q = _q9()
    ctx = StubContext(lib)
    idx = np.arange(2, 11)
    form = _sparse_form(Q, idx, ctx=ctx)
    model = _model(small=small)
    rec = _objective(model, _quad_out(Q.nnz, 0), QuadPlan("canonical-sparse-form", form=form))
    vm = np.arange(1, 30, dtype=np.int64)[::-1].copy() if mapped else None
    emit = rec.compile(ctx, VARMAP_BUF, vm)
    pj, pk, sa, sb = U.tables(Q)
    f = rec.f
    assert len(f.quadratic_terms) == len(pj) and len(f.affine_terms) == 0
    assert set(rec.dev) == {"quad", "lin", "const"}
    x = idx if vm is None else vm[idx - 1]
    assert f.quadratic_terms["row"].tolist() == x[pj].tolist() and f.quadratic_terms["col"].tolist() == x[pk].tolist()
    # allocations: the four tables, beyond the small plan the twins (the empty linear list: 16 bytes)
    assert ctx.allocs == [4 * len(pj)] * 4 + ([16] if small else [24 * len(pj), 16, 16])
    if small:
        assert rec.dev["quad"] == f.quadratic_terms.ctypes.data and rec.dev["const"] == rec._cbuf.ctypes.data
    n_alloc = len(ctx.allocs)
    emit(ctx)
    emit(ctx)
    assert len(ctx.allocs) == n_alloc and [name for name, _ in ctx.raw] == ["pmt_sparse_form_f64"] * 2          # update! allocates nothing
    assert len(ctx.raw[0][1]) == len(lib.SIGNATURES["pmt_sparse_form_f64"][1]) - 1                                # (the context appends the stream)
    assert ctx.calls[0] == ("pmt_sparse_form_f64", (len(pj), 1))


def test_canonical_sparse_sum_record_tape_with_a_form(lib):
    from parametron_jl_amd.lazyexpression import LsqTerm
    from parametron_jl_amd.moi import QuadPlan
    Q = _q9()
    rng = np.random.default_rng(5)
    Cs = SG.from_mask(rng.random((40, 9)) < 0.3, rng)
    ctx = StubContext(lib)
    idx = np.arange(2, 11)
    form, r1 = _sparse_form(Q, idx, ctx=ctx), _sparse_block(Cs, idx, ctx=ctx)
    terms = [LsqTerm("block", r=r1), LsqTerm("form", r=form, scale=0.5), LsqTerm("constant", scale=2.0)]
    rec = _objective(_model(), _quad_out(7, 7), QuadPlan("canonical-sparse-sum", terms=terms))
    emit = rec.compile(ctx, VARMAP_BUF, None)
    spec = [Term("block", Cs=Cs), U.FormTerm(Q, scale=0.5), Term("constant", scale=2.0)]
    pairs, cols = SU.structure(9, spec)
    assert len(rec.f.quadratic_terms) == len(pairs) and len(rec.f.affine_terms) == len(cols)
    emit(ctx)
    assert [name for name, _ in ctx.raw] == ["pmt_sparse_gram_f64", "pmt_sparse_form_f64", "pmt_sparse_gram_sum_f64"]
    d = (lib.SparseLsqTerm * 3).from_address(ctx.raw[2][1][1])
    assert [t.kind for t in d] == [lib.PMT_LSQ_BLOCK, lib.PMT_LSQ_BLOCK, lib.PMT_LSQ_CONSTANT] and [t.scale for t in d] == [1.0, 0.5, 2.0]
    assert all(d[b].quad and d[b].lin and d[b].constant and d[b].quad_at and d[b].lin_at for b in (0, 1))
    # the form writes its own scratch quad list and constant word: the pointers of its descriptor
    fa = ctx.raw[1][1]
    assert fa[-2].value == d[1].quad and fa[-1].value == d[1].constant
    # its lin_at is the all-0xFFFFFFFF table the merge writes for a block without linear terms
    S = SU.merge_tables(9, [Term("block", Cs=Cs), Term("block", pat=U.FormTerm(Q).pat), Term("constant")])
    assert np.all(S.lin_at[1] == U.NONE) and np.count_nonzero(S.quad_at[1] != U.NONE) == len(U.tables(Q)[0])


# ---- 6. a sum with a form against the oracle composition
@pytest.mark.parametrize("seed", range(12))
def test_sum_with_a_form_matches_the_oracle_within_the_derived_bound(lib, seed):
    """exact indices and counts, every coefficient within sparse_sum_util's bound with the form as a block of nlin = 0
    (sparse_form_util.sum_bounds): forms alone and beside a sparse block, all other term kinds, negative weights, a permuting index map"""
    rng = np.random.default_rng(1660 + seed)
    n = 9
    Q, R = U.pattern("mixed", n, rng, zeros=seed % 2 == 0), U.pattern(U.KINDS[seed % 6], n, rng, zeros=False)
    terms = [U.FormTerm(Q, scale=0.5 if seed % 3 else -1.5, weight=float(rng.random() + 0.5) if seed % 2 else None)]
    if seed % 2:
        m = 25
        terms.insert(0, Term("block", Cs=SG.from_mask(rng.random((m, n)) < 0.3, rng), d=SG.signed_values(rng, m), sign=-1, weight=float(rng.random())))
    terms.append(Term("diag", weight=float(rng.random()), scale=-1.0 if seed % 3 == 0 else 1.0))
    terms.append(U.FormTerm(R, weight=float(rng.random() - 0.5)))
    terms.append(Term("diag", cols=np.sort(rng.choice(n, 4, replace=False)), v=SG.signed_values(rng, 4), sign=-1, scale=-0.5))
    terms.append(Term("linear", v=SG.signed_values(rng, n)))
    terms.append(Term("constant", value=float(rng.random() - 0.5), scale=3.0))
    xvar, vm = _xvar_varmap(n, seed)
    quad, lin, const = U.sum_restate(n, xvar, vm, terms)
    assert len(lin) == n
    SU.assert_close_to_oracle(quad, lin, const, U.sum_oracle(n, xvar, vm, terms), *U.sum_bounds(n, terms))


def test_a_form_alone_in_the_sum_machinery_is_the_bare_node(lib):
    """W = 1 is exact: 1.0 * x'Qx + s has the bare node's quadratic bits, no linear terms, the constant 0.0 + s"""
    Q = _q9()
    xvar, vm = _xvar_varmap(9)
    quad, lin, const = U.sum_restate(9, xvar, vm, [U.FormTerm(Q), Term("constant", value=0.375)])
    assert quad.tobytes() == U.restate(Q, xvar, 1, vm).tobytes() and len(lin) == 0 and const == 0.375
