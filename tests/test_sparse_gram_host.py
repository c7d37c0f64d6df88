"""CPU-only: the host side of the sparse least-squares objective dot(r, r), r = C*x (+|-) d with a sparse C — the symbolic phase
(pmt_sparse_gram_count / _order / _runs) against a brute-force pattern, the Python restatement of the contract against the oracle, the
quad_plan rows, the record a "canonical-sparse" plan compiles (stub context), and argument validation before any device call."""
import ctypes as C

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")

import __graft_entry__ as entry  # noqa: E402
import sparse_gram_util as U  # noqa: E402
from test_record_tape_host import VARMAP_BUF, StubContext, _model, _objective, _quad_out  # noqa: E402
from test_stacked_lsq_host import FAKE  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


# ---- the symbolic phase
def _mask_cases():
    rng = np.random.default_rng(7)
    cases = [("random %d" % t, rng.random((int(rng.integers(1, 40)), int(rng.integers(1, 30)))) < rng.uniform(0.05, 0.5)) for t in range(12)]
    cases.append(("no entry", np.zeros((5, 4), dtype=bool)))
    hole = rng.random((9, 8)) < 0.4
    hole[3, :], hole[:, 5] = False, False
    cases.append(("an empty row and an empty column", hole))
    full_row = rng.random((6, 70)) < 0.1
    full_row[2, :] = True
    cases.append(("one full row", full_row))
    full_col = rng.random((150, 6)) < 0.1
    full_col[:, 4] = True                                        # its diagonal segment has 150 products: a long one
    cases.append(("one full column", full_col))
    return cases


@pytest.mark.parametrize("name,mask", _mask_cases(), ids=[c[0] for c in _mask_cases()])
def test_symbolic_phase_matches_the_brute_force_pattern(lib, name, mask):
    rng = np.random.default_rng(3)
    Cs = U.from_mask(mask, rng)
    m, n = Cs.shape
    pairs, lin_col = U.pattern(Cs)
    T = U.tables(Cs, cap=64)
    lens = np.diff(Cs.tocsr().indptr)
    assert T.nprod == int(np.sum(lens * (lens + 1) // 2)) == sum(len(p) for _, _, p in pairs)
    A = abs(Cs)
    assert T.nq == len(pairs) == sp.triu(A.T @ A).nnz
    jk = list(zip(T.pair_j.tolist(), T.pair_k.tolist()))
    assert jk == sorted(jk) == [(j, k) for j, k, _ in pairs] and all(j <= k for j, k in jk)
    assert T.seg_ptr[0] == 0 and T.seg_ptr[-1] == T.nprod and np.all(np.diff(T.seg_ptr) >= 1)
    for s, (j, k, want) in enumerate(pairs):
        seg = T.prod[T.seg_ptr[s]:T.seg_ptr[s + 1]]
        assert [tuple(r) for r in seg.tolist()] == want
        ra, rb = Cs.indices[seg[:, 0]], Cs.indices[seg[:, 1]]
        assert np.array_equal(ra, rb) and np.all(np.diff(ra) > 0)                                      # ascending rows
        assert np.all((seg[:, 0] >= Cs.indptr[j]) & (seg[:, 0] < Cs.indptr[j + 1]) & (seg[:, 1] >= Cs.indptr[k]) & (seg[:, 1] < Cs.indptr[k + 1]))
    assert T.lin_col.tolist() == lin_col
    assert T.lin_long.tolist() == [l for l, j in enumerate(lin_col) if Cs.indptr[j + 1] - Cs.indptr[j] >= 64]
    assert T.lin_seg.tolist() == [int(Cs.indptr[j]) for j in lin_col] + [Cs.nnz] and np.array_equal(T.rowidx0, Cs.indices)
    lcov = np.zeros(T.nlin, dtype=int)
    for r in range(T.nlin_runs):
        l0, l1 = T.lin_runs[2 * r], T.lin_runs[2 * r + 1]
        assert l0 < l1 and np.all(np.diff(T.lin_seg)[l0:l1] < 64) and T.lin_seg[l1] - T.lin_seg[l0] <= 64
        lcov[l0:l1] += 1
    lcov[T.lin_long] += 1
    assert np.all(lcov == 1)
    # the cut: every short segment in exactly one run, runs within the cap, long segments listed apart
    seglen = np.diff(T.seg_ptr)
    covered = np.zeros(T.nq, dtype=int)
    for r in range(T.nruns):
        s0, s1 = T.runs[2 * r], T.runs[2 * r + 1]
        assert s0 < s1 and np.all(seglen[s0:s1] < 64) and seglen[s0:s1].sum() <= 64
        covered[s0:s1] += 1
    assert T.long_seg.tolist() == np.flatnonzero(seglen >= 64).tolist()
    covered[T.long_seg] += 1
    assert np.all(covered == 1)
    if name == "one full column":
        assert T.nlong >= 1 and T.nlin_long == 1


def test_an_empty_matrix_has_no_terms(lib):
    for shape in ((0, 0), (0, 3), (4, 0)):
        T = U.tables(sp.csc_matrix(shape), cap=2048)
        assert (T.nq, T.nprod, T.nlin, T.nruns, T.nlong, T.nlin_runs, T.nlin_long) == (0, 0, 0, 0, 0, 0, 0)


def _count(lib, m, n, colptr, rowval):
    nq, nprod = C.c_int64(), C.c_int64()
    colptr, rowval = np.asarray(colptr, dtype=np.int64), np.asarray(rowval, dtype=np.int64)
    lib.call("pmt_sparse_gram_count", m, n, U.vp(colptr), U.vp(rowval), C.byref(nq), C.byref(nprod))
    return nq.value, nprod.value


def _order(lib, m, n, colptr, rowval, nq=8, nprod=8):
    colptr, rowval = np.asarray(colptr, dtype=np.int64), np.asarray(rowval, dtype=np.int64)
    pj, pk, seg, prod, lc = (np.zeros(64, dtype=np.uint32), np.zeros(64, dtype=np.uint32), np.zeros(65, dtype=np.int64),
                             np.zeros(128, dtype=np.uint32), np.zeros(64, dtype=np.uint32))
    nlin = C.c_int64()
    lib.call("pmt_sparse_gram_order", m, n, U.vp(colptr), U.vp(rowval), nq, nprod, U.vp(pj), U.vp(pk), U.vp(seg), U.vp(prod), U.vp(lc), C.byref(nlin))


@pytest.mark.parametrize("helper", [_count, _order])
def test_symbolic_phase_rejects_bad_patterns_like_the_other_sparse_helpers(lib, helper):
    assert _count(lib, 3, 2, [1, 3, 4], [1, 3, 2]) == (2, 3)                 # (the good pattern the bad ones are made from)
    with pytest.raises(lib.ArgumentError, match="1-based"):
        helper(lib, 3, 2, [0, 2, 3], [1, 3, 2])
    with pytest.raises(lib.DimensionMismatch, match="out of range"):
        helper(lib, 3, 2, [1, 3, 4], [1, 4, 2])
    with pytest.raises(lib.DimensionMismatch, match="out of range"):
        helper(lib, 3, 2, [1, 3, 4], [0, 3, 2])
    with pytest.raises(lib.ArgumentError, match="ascend"):
        helper(lib, 3, 2, [1, 3, 4], [3, 1, 2])
    with pytest.raises(lib.ArgumentError, match="ascend"):
        helper(lib, 3, 2, [1, 3, 4], [2, 2, 2])                              # a duplicate entry
    with pytest.raises(lib.ArgumentError, match="monotone"):
        helper(lib, 3, 2, [1, 3, 2], [1, 3, 2])
    with pytest.raises(lib.DimensionMismatch):
        helper(lib, -1, 2, [1, 3, 4], [1, 3, 2])


def test_order_wants_the_counts_of_count(lib):
    with pytest.raises(lib.ArgumentError, match="nprod"):
        _order(lib, 3, 2, [1, 3, 4], [1, 3, 2], nq=2, nprod=4)
    for nq in (1, 3):
        with pytest.raises(lib.ArgumentError, match="nq"):
            _order(lib, 3, 2, [1, 3, 4], [1, 3, 2], nq=nq, nprod=3)
    _order(lib, 3, 2, [1, 3, 4], [1, 3, 2], nq=2, nprod=3)


def test_two_to_the_31_products_are_refused_with_advice(lib):
    n = 1 << 16                                                               # one full row: 65536 * 65537 / 2 products
    Cs = sp.csc_matrix((np.ones(n), np.zeros(n, dtype=np.int64), np.arange(n + 1)), shape=(1, n))
    assert _count(lib, 1, n, Cs.indptr + 1, Cs.indices + 1) == (-1, n * (n + 1) // 2)
    with pytest.raises(lib.ArgumentError, match=r"nprod = %d.*dense Parameter" % (n * (n + 1) // 2)):
        U.tables(Cs)
    with pytest.raises(lib.ArgumentError, match="nprod"):
        _order(lib, 3, 2, [1, 3, 4], [1, 3, 2], nq=2, nprod=1 << 31)


def test_runs_reject_bad_arguments(lib):
    seg = np.array([0, 3, 5], dtype=np.int64)
    nr, nl = C.c_int64(), C.c_int64()
    lib.call("pmt_sparse_gram_runs", U.vp(seg), 2, 64, None, C.byref(nr), None, C.byref(nl))
    assert (nr.value, nl.value) == (1, 0)
    for cap in (63, 2049):
        with pytest.raises(lib.ArgumentError):
            lib.call("pmt_sparse_gram_runs", U.vp(seg), 2, cap, None, C.byref(nr), None, C.byref(nl))
    with pytest.raises(lib.ArgumentError):
        lib.call("pmt_sparse_gram_runs", None, 2, 64, None, C.byref(nr), None, C.byref(nl))
    with pytest.raises(lib.ArgumentError):
        lib.call("pmt_sparse_gram_runs", U.vp(seg), -1, 64, None, C.byref(nr), None, C.byref(nl))


# ---- the restatement against the oracle, before any GPU sees it
@pytest.mark.parametrize("seed", range(20))
def test_restatement_matches_the_oracle(lib, seed):
    """indices exact, coefficients within the derived bound (sparse_gram_util.bounds), on 20 random small patterns: signed values, with
    and without d, both signs, through a permuting index map.  Every fourth pattern has a column of 70 rows (the one-wave order)."""
    rng = np.random.default_rng(100 + seed)
    m, n = (int(rng.integers(70, 90)), int(rng.integers(2, 7))) if seed % 4 == 3 else (int(rng.integers(1, 25)), int(rng.integers(1, 20)))
    mask = rng.random((m, n)) < rng.uniform(0.08, 0.5)
    if seed % 4 == 3:
        mask[:70, 0] = True
    Cs = U.from_mask(mask, rng)
    xvar = np.sort(rng.choice(np.arange(1, n + 6), n, replace=False))
    vm = rng.permutation(n + 5).astype(np.int64) + 1 + int(rng.integers(0, 4))
    pat = U.pattern(Cs)
    for d, sign in ((None, 0), (U.signed_values(rng, m), -1), (U.signed_values(rng, m), 1)):
        quad, lin, const = U.restate(Cs, xvar, d, sign, 1, vm, pat)
        U.assert_close_to_oracle(quad, lin, const, U.oracle_function(Cs, xvar, d, sign, vm), *U.bounds(Cs, d, sign, pat))
    # without d the linear terms still exist, one per non-empty column, with zero coefficients
    quad, lin, const = U.restate(Cs, xvar, None, 0, 1, vm, pat)
    assert len(lin) == int(np.count_nonzero(np.diff(Cs.indptr))) and np.all(lin["coeff"] == 0.0) and const == 0.0
    # the native form: same sums, native indices, the diagonal undoubled
    nat, nlin, _ = U.restate(Cs, xvar, None, 0, 0, None, pat)
    diag = nat["row"] == nat["col"]
    assert np.array_equal(nat["coeff"][diag] * 2, quad["coeff"][diag]) and np.array_equal(nat["coeff"][~diag], quad["coeff"][~diag])
    assert np.array_equal(nlin["var"], xvar[pat[1]])


# ---- quad_plan
def _sparse_block(Cs, idx, vec=None, sign=0, ctx=None):
    """a DSparseAff without a device: the fields quad_plan and _compile_sparse_gram read"""
    from parametron_jl_amd.device import DSparseAff, DSpMat, DVars
    spm = DSpMat.__new__(DSpMat)
    spm.rows, spm.cols, spm.nnz, spm.narrow, spm.buf, spm._gram = Cs.shape[0], Cs.shape[1], Cs.nnz, True, FAKE, None
    spm.indptr, spm.indices = Cs.indptr.copy(), Cs.indices.copy()
    x = DVars.__new__(DVars)
    x.vars, x.n, x.buf = np.asarray(idx, dtype=np.int64), len(idx), FAKE
    r = DSparseAff.__new__(DSparseAff)
    r.spmat, r.xvars, r.vec, r.sign, r.rows, r.ctx, r.need_terms = spm, x, vec, sign, Cs.shape[0], ctx, False
    return r


def _small_pattern():
    rng = np.random.default_rng(5)
    mask = rng.random((40, 9)) < 0.3
    mask[:, 7] = False                                                        # an empty column: no linear term
    return U.from_mask(mask, rng)


def test_quad_plan_rows_of_a_sparse_block(lib):
    from parametron_jl_amd.lazyexpression import LsqTerm
    from parametron_jl_amd.moi import quad_plan
    Cs = _small_pattern()
    r = _sparse_block(Cs, np.arange(2, 11))
    assert r.gram_operand()
    terms = [LsqTerm("block", r=r)]
    vm = np.arange(1, 20, dtype=np.int64)
    for mode in ("auto", "canonical"):
        for small in (True, False):
            for handoff in ("moi", "device"):
                for is_objective in (True, False):
                    p = quad_plan(terms, True, "quad", 99, is_objective, mode, small, handoff, vm)
                    assert p.mode == "canonical-sparse" and p.gram is r and not p.canonicalize and not p.gram_record
    with pytest.raises(lib.ArgumentError, match="quadratic_mode='literal'"):
        quad_plan(terms, True, "quad", 99, True, "literal", False, "moi", None)
    for mode in ("auto", "canonical"):
        with pytest.raises(lib.ArgumentError, match="handoff='host_csc'"):
            quad_plan(terms, True, "quad", 99, True, mode, False, "host_csc", vm)
    # in a sum the block is not combined: the literal path (which refuses a ragged residual when it materialises)
    both = terms + [LsqTerm("diag", xvars=r.xvars)]
    p = quad_plan(both, False, "quad", 99, True, "canonical", False, "moi", None)
    assert p.mode == "literal" and p.canonicalize
    # not an operand: x out of order, or a pattern with unsorted rows
    assert not _sparse_block(Cs, np.arange(10, 1, -1)).gram_operand()
    bad = Cs.copy()
    j = int(np.argmax(np.diff(bad.indptr) >= 2))
    bad.indices[bad.indptr[j]:bad.indptr[j] + 2] = bad.indices[bad.indptr[j]:bad.indptr[j] + 2][::-1].copy()
    assert not _sparse_block(bad, np.arange(2, 11)).gram_operand()


def test_quad_plan_dense_rows_are_unchanged(lib):
    from parametron_jl_amd.lazyexpression import LsqTerm
    from parametron_jl_amd.moi import quad_plan
    from test_record_tape_host import _block
    g = _block(30, [1, 2, 3])
    terms = [LsqTerm("block", r=g)]
    assert quad_plan(terms, True, "quad", 270, True, "canonical", False, "moi").mode == "canonical"
    assert quad_plan(terms, True, "quad", 270, True, "auto", False, "moi").mode == "literal"
    assert quad_plan(terms, True, "quad", (1 << 24) + 1, True, "auto", False, "moi").mode == "canonical"
    assert quad_plan(terms, True, "quad", 270, True, "literal", False, "moi").mode == "literal"
    assert quad_plan(terms, True, "quad", 270, True, "canonical", False, "device", np.arange(1, 5)).mode == "canonical-csc"
    assert quad_plan(terms, True, "quad", 270, True, "canonical", False, "host_csc", np.arange(1, 5)).mode == "canonical-csc"
    assert quad_plan(None, False, "aff", 0, True, "canonical", False, "moi").mode is None
    assert quad_plan(None, False, "quad", 10, True, "canonical", False, "moi").mode == "literal"


# ---- the record
@pytest.mark.parametrize("small", [False, True])
def test_canonical_sparse_record_tape(lib, small):
    from parametron_jl_amd.moi import QuadPlan
    from test_record_tape_host import _b
    Cs = _small_pattern()
    ctx = StubContext(lib)
    idx = np.arange(2, 11)
    r = _sparse_block(Cs, idx, vec=_b(40), sign=-1, ctx=ctx)
    model = _model(small=small)
    rec = _objective(model, _quad_out(7, 7), QuadPlan("canonical-sparse", gram=r))
    vm = np.arange(1, 30, dtype=np.int64)[::-1].copy()
    emit = rec.compile(ctx, VARMAP_BUF, vm)
    T = r.gram_tables()
    pairs, lin_col = U.pattern(Cs)
    assert (T.nq, T.nlin) == (len(pairs), 8) and T is r.gram_tables()                 # built once
    # allocations: the eleven tables, then (beyond the small plan) the three twins
    tables = [getattr(T, k) for k in T.TABLES]
    assert len(tables) == 11
    want_allocs = [max(t.nbytes, 8) for t in tables] + ([] if small else [24 * T.nq, 16 * T.nlin, 16])
    assert ctx.allocs == want_allocs
    f = rec.f
    assert len(f.quadratic_terms) == T.nq and len(f.affine_terms) == T.nlin
    assert set(rec.dev) == {"quad", "lin", "const"}
    assert [k for _, k in rec.buffers] == ["quad", "lin", "const"] and rec.buffers[0][0] is f.quadratic_terms and rec.buffers[1][0] is f.affine_terms
    if small:
        assert rec.dev == {"quad": f.quadratic_terms.ctypes.data, "lin": f.affine_terms.ctypes.data, "const": rec._cbuf.ctypes.data}
        assert rec.copies() == []
    else:
        assert len(rec.copies()) == 3
    # the static index fields are on the host before the first update, through the hand-off's map
    x = vm[idx - 1]
    assert f.quadratic_terms["row"].tolist() == [x[j] for j, _, _ in pairs] and f.quadratic_terms["col"].tolist() == [x[k] for _, k, _ in pairs]
    assert f.affine_terms["var"].tolist() == [x[j] for j in lin_col]
    assert rec.varmap_hooks == [] and rec.delivered == () and not rec.side_lane_ok
    n_alloc = len(ctx.allocs)
    emit(ctx)
    emit(ctx)
    assert len(ctx.allocs) == n_alloc                                               # update! allocates nothing
    name, args = ctx.raw[0]
    assert name == "pmt_sparse_gram_f64" and len(ctx.raw) == 2
    assert len(args) == len(lib.SIGNATURES["pmt_sparse_gram_f64"][1]) - 1          # (the context appends the stream)
    assert ctx.calls[0] == ("pmt_sparse_gram_f64", (T.nq, T.nruns, T.nlong, T.nlin, T.nlin_runs, T.nlin_long, 40, -1, 1))


def test_literal_consumers_of_the_sparse_node_get_the_literal_error(lib):
    from parametron_jl_amd.lazyexpression import _NoLiteralQuad
    q = _NoLiteralQuad(None, 10, 4)
    assert (q.nq, q.nl, q.quad) == (10, 4, None)
    with pytest.raises(lib.ArgumentError, match="dot of two Vector{AffineFunction} needs rows of equal length on the device"):
        q.materialize()


# ---- argument validation without a GPU
def _gram_call(lib, **kw):
    a = dict(nzval=FAKE, prod=FAKE, seg_ptr=FAKE, pair_j=FAKE, pair_k=FAKE, nq=3, runs=FAKE, nruns=1, long_seg=None, nlong=0, lin_seg=FAKE,
             rowidx0=FAKE, lin_col=FAKE, nlin=2, lin_runs=FAKE, nlin_runs=1, lin_long=None, nlin_long=0, rows=3, xvar=FAKE, d=FAKE, sign=-1, moi=1,
             varmap=FAKE, out_quad=FAKE, out_lin=FAKE, out_const=FAKE)
    a.update(kw)
    lib.call("pmt_sparse_gram_f64", *a.values(), None)


def test_entry_point_validates_before_any_device_call(lib):
    for name in ("nzval", "prod", "seg_ptr", "pair_j", "pair_k", "runs", "lin_seg", "rowidx0", "lin_col", "lin_runs", "xvar", "out_quad", "out_lin",
                 "out_const"):
        with pytest.raises(lib.ArgumentError, match="null pointer"):
            _gram_call(lib, **{name: None})
    for name in ("nq", "nruns", "nlong", "nlin", "nlin_runs", "nlin_long", "rows"):
        with pytest.raises(lib.ArgumentError, match="negative"):
            _gram_call(lib, **{name: -1})
    with pytest.raises(lib.ArgumentError, match="varmap"):
        _gram_call(lib, varmap=None)
    with pytest.raises(lib.ArgumentError, match="sign"):
        _gram_call(lib, sign=2)
    with pytest.raises(lib.ArgumentError, match="sign"):
        _gram_call(lib, d=None)                                                   # a sign without d
    with pytest.raises(lib.ArgumentError, match="null pointer"):
        _gram_call(lib, nlong=1)                                                  # long segments without their list
    with pytest.raises(lib.ArgumentError, match="null pointer"):
        _gram_call(lib, nlin_long=1)
    with pytest.raises(lib.ArgumentError):
        _gram_call(lib, nruns=3, nlong=1)                                         # more runs than segments
    with pytest.raises(lib.ArgumentError):
        _gram_call(lib, nruns=0)                                                  # segments that nothing computes
    with pytest.raises(lib.ArgumentError):
        _gram_call(lib, nlin_runs=0)                                              # columns that nothing computes
    with pytest.raises(lib.ArgumentError):
        _gram_call(lib, nlin_runs=2, nlin_long=1)                                 # more linear runs than columns
