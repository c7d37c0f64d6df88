"""CPU-only: the host side of weighted sums over sparse least-squares blocks (record mode "canonical-sparse-sum") — the symbolic merge
(pmt_sparse_gram_sum_merge) against brute force, the Python restatement of the contract against the oracle within the derived bound, the
quad_plan rows, the record a "canonical-sparse-sum" plan compiles (stub context), and argument validation before any device call."""
import ctypes as C

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")

import __graft_entry__ as entry  # noqa: E402
import sparse_gram_util as SG  # noqa: E402
import sparse_sum_util as U  # noqa: E402
from sparse_sum_util import Term  # noqa: E402
from test_record_tape_host import VARMAP_BUF, StubContext, _b, _model, _objective, _quad_out, _xvars  # noqa: E402
from test_sparse_gram_host import _sparse_block  # noqa: E402
from test_stacked_lsq_host import FAKE  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


def _masked(rng, m, n, density, empty=()):
    mask = rng.random((m, n)) < density
    for j in empty:
        mask[:, j] = False
    return SG.from_mask(mask, rng)


# ---- the symbolic merge
def _two_blocks():
    """9 columns.  Block 1 holds pair (0, 1), block 2 pair (2, 3), both hold (4, 5); column 6 is empty in both and listed by a diagonal
    term (its pair is D alone), column 7 is reached by a linear term only, column 8 by nothing"""
    a, b = np.zeros((5, 9), dtype=bool), np.zeros((7, 9), dtype=bool)
    a[0, [0, 1]] = True
    b[1, [2, 3]] = True
    a[2, [4, 5]], b[3, [4, 5]] = True, True
    rng = np.random.default_rng(1)
    return SG.from_mask(a, rng), SG.from_mask(b, rng)


def _merge_cases():
    rng = np.random.default_rng(2)
    A, B = _two_blocks()
    cases = {"pairs in one block, the other, both; a D-only pair; a linear-only column": (9, [
        Term("block", Cs=A), Term("block", Cs=B, scale=-2.0), Term("diag", cols=[4, 6]), Term("linear", cols=[0, 7], v=[0.5, -0.25]), Term("constant")])}
    cases["a diagonal term with v over part of x"] = (9, [Term("block", Cs=A), Term("diag", cols=[1, 2, 8], v=[0.1, 0.2, 0.3], sign=-1)])
    cases["all-empty blocks"] = (6, [Term("block", Cs=sp.csc_matrix((4, 6))), Term("block", Cs=sp.csc_matrix((0, 6))), Term("diag", cols=[2, 3])])
    cases["all-empty blocks alone"] = (6, [Term("block", Cs=sp.csc_matrix((4, 6)))])
    cases["K = 1, all of x"] = (12, [Term("block", Cs=_masked(rng, 20, 12, 0.3, empty=(5,))), Term("diag"), Term("linear", v=rng.random(12))])
    cases["K = 8"] = (15, [Term("block", Cs=_masked(rng, int(rng.integers(3, 30)), 15, 0.15)) for _ in range(8)] + [Term("diag", cols=[0, 14])])
    return cases


@pytest.mark.parametrize("name", list(_merge_cases()))
def test_merge_matches_brute_force(lib, name):
    n, terms = _merge_cases()[name]
    pairs, cols, tabs, pos = U.gather_tables(n, terms)
    S = U.merge_tables(n, terms)
    assert (S.nq, S.nlin) == (len(pairs), len(cols))
    assert list(zip(S.pair_j.tolist(), S.pair_k.tolist())) == pairs and S.lin_col.tolist() == cols
    assert len(S.quad_at) == len(S.lin_at) == len(tabs)
    for b, (qa, la) in enumerate(tabs):
        assert np.array_equal(S.quad_at[b], qa) and np.array_equal(S.lin_at[b], la)
        hit = S.quad_at[b][S.quad_at[b] != U.NONE]
        assert np.array_equal(hit, np.arange(len(hit)))                      # monotone: every block term is used once, in order
    assert set(S.term_pos) == set(pos) and all(np.array_equal(S.term_pos[t], pos[t]) for t in pos)
    if name.startswith("pairs in one"):
        at = {p: s for s, p in enumerate(pairs)}
        assert S.quad_at[0][at[(0, 1)]] != U.NONE and S.quad_at[1][at[(0, 1)]] == U.NONE
        assert S.quad_at[0][at[(2, 3)]] == U.NONE and S.quad_at[1][at[(2, 3)]] != U.NONE
        assert S.quad_at[0][at[(4, 5)]] != U.NONE and S.quad_at[1][at[(4, 5)]] != U.NONE
        assert S.quad_at[0][at[(6, 6)]] == U.NONE and S.quad_at[1][at[(6, 6)]] == U.NONE
        assert 7 in cols and 6 not in cols and 8 not in cols and S.lin_at[0][cols.index(7)] == U.NONE == S.lin_at[1][cols.index(7)]
    if name == "all-empty blocks":
        assert pairs == [(2, 2), (3, 3)] and cols == []
    if name == "all-empty blocks alone":
        assert (S.nq, S.nlin) == (0, 0)


def _merge_raw(lib, n, pj, pk, lc, kinds, cols=None, nblocks=None):
    """the counting call on raw lists"""
    vp = C.c_void_p
    arr = lambda xs, dt: [np.asarray(x, dtype=dt) for x in xs]                 # noqa: E731
    pj, pk, lc = arr(pj, np.uint32), arr(pk, np.uint32), arr(lc, np.uint32)
    ptrs = lambda v: (vp * max(len(v), 1))(*[a.ctypes.data if a is not None else None for a in v])       # noqa: E731
    nq, nl = np.array([len(a) for a in pj], dtype=np.int64), np.array([len(a) for a in lc], dtype=np.int64)
    kinds = np.asarray(kinds, dtype=np.int32)
    hv = np.zeros(len(kinds), dtype=np.int32)
    cols = [None if c is None else np.asarray(c, dtype=np.int64) for c in (cols or [None] * len(kinds))]
    nc = np.array([0 if c is None else len(c) for c in cols], dtype=np.int64)
    onq, onl = C.c_int64(), C.c_int64()
    lib.call("pmt_sparse_gram_sum_merge", n, len(pj) if nblocks is None else nblocks, ptrs(pj), ptrs(pk), SG.vp(nq), ptrs(lc), SG.vp(nl), len(kinds),
             SG.vp(kinds), SG.vp(hv), ptrs(cols), SG.vp(nc), C.byref(onq), C.byref(onl), None, None, None, None, None, None)
    return onq.value, onl.value


def test_merge_rejects_bad_inputs_with_typed_errors(lib):
    B, D, L = lib.PMT_LSQ_BLOCK, lib.PMT_LSQ_DIAG, lib.PMT_LSQ_LINEAR
    assert _merge_raw(lib, 4, [[0, 0, 1]], [[0, 2, 1]], [[0, 1, 2]], [B, D], [None, [1, 3]]) == (4, 3)      # (the good input the bad ones are made from)
    with pytest.raises(lib.ArgumentError, match="sorted"):
        _merge_raw(lib, 4, [[0, 0, 1]], [[2, 0, 1]], [[0, 1, 2]], [B])
    with pytest.raises(lib.ArgumentError, match="sorted"):
        _merge_raw(lib, 4, [[0, 0, 1]], [[0, 0, 1]], [[0, 1, 2]], [B])                                       # a duplicate pair
    with pytest.raises(lib.ArgumentError, match="increasing"):
        _merge_raw(lib, 4, [[0]], [[0]], [[1, 0]], [B])
    with pytest.raises(lib.ArgumentError, match="increasing"):
        _merge_raw(lib, 4, [[0]], [[0]], [[0]], [B, D], [None, [3, 1]])
    with pytest.raises(lib.DimensionMismatch, match="j <= k < n"):
        _merge_raw(lib, 4, [[0]], [[4]], [[0]], [B])
    with pytest.raises(lib.DimensionMismatch, match="j <= k < n"):
        _merge_raw(lib, 4, [[2]], [[1]], [[0]], [B])
    with pytest.raises(lib.DimensionMismatch, match="outside"):
        _merge_raw(lib, 4, [[0]], [[0]], [[4]], [B])
    with pytest.raises(lib.DimensionMismatch, match="outside"):
        _merge_raw(lib, 4, [[0]], [[0]], [[0]], [B, L], [None, [1, 4]])
    with pytest.raises(lib.ArgumentError, match="1 .. 8"):
        _merge_raw(lib, 4, [[0]] * 9, [[0]] * 9, [[0]] * 9, [B] * 9)
    with pytest.raises(lib.ArgumentError, match="1 .. 8"):
        _merge_raw(lib, 4, [], [], [], [D])
    with pytest.raises(lib.ArgumentError, match="1 .. 32"):
        _merge_raw(lib, 4, [[0]], [[0]], [[0]], [B] + [D] * 32)
    with pytest.raises(lib.ArgumentError, match="nblocks"):
        _merge_raw(lib, 4, [[0]], [[0]], [[0]], [B, B])
    with pytest.raises(lib.ArgumentError, match="column list"):
        _merge_raw(lib, 4, [[0]], [[0]], [[0]], [B], [[1]])
    with pytest.raises(lib.ArgumentError, match="kind"):
        _merge_raw(lib, 4, [[0]], [[0]], [[0]], [B, 7])
    with pytest.raises(lib.DimensionMismatch):
        _merge_raw(lib, -1, [[0]], [[0]], [[0]], [B])


# ---- the restatement against the oracle, before any GPU sees it
def _mixed_terms(rng, n, seed):
    """two or three blocks of different patterns and row counts (an empty column in the first), and every other kind of term, some weights
    negative, some as scale * weight"""
    m1, m2 = 40, int(rng.integers(5, 30))
    terms = [Term("block", Cs=_masked(rng, m1, n, 0.3, empty=(n - 2,)), d=SG.signed_values(rng, m1), sign=-1, weight=float(rng.random() + 0.5))]
    terms.append(Term("diag", weight=float(rng.random()), scale=-1.0 if seed % 3 == 0 else 1.0))
    terms.append(Term("block", Cs=_masked(rng, m2, n, 0.2), d=SG.signed_values(rng, m2), sign=1, scale=-0.75 if seed % 2 else 1.5))
    part = np.sort(rng.choice(n, 4, replace=False))
    terms.append(Term("diag", cols=part, v=SG.signed_values(rng, 4), sign=-1 if seed % 2 else 1, scale=0.5))
    terms.append(Term("linear", v=SG.signed_values(rng, n), scale=-1.0))
    if seed % 4 == 1:
        terms.append(Term("block", Cs=_masked(rng, 12, n, 0.4), scale=2.0, weight=float(-rng.random())))        # no d
    terms.append(Term("linear", cols=[0, n - 2], v=SG.signed_values(rng, 2), weight=float(rng.random())))
    terms.append(Term("constant", scale=3.25))
    terms.append(Term("constant", value=float(rng.random() - 0.5), scale=-1.0))
    if seed % 5 == 0:
        terms.append(Term("diag", cols=[1, 2, 3]))
    return terms


@pytest.mark.parametrize("seed", range(20))
def test_restatement_matches_the_oracle(lib, seed):
    """exact indices and counts, every coefficient within the derived bound (sparse_sum_util.bounds), on 20 random sums over 40 x 9
    blocks at 30 % with an empty column: all term kinds, negative weights, through a permuting index map"""
    rng = np.random.default_rng(500 + seed)
    n = 9
    terms = _mixed_terms(rng, n, seed)
    xvar = np.sort(rng.choice(np.arange(1, n + 6), n, replace=False))
    vm = rng.permutation(n + 5).astype(np.int64) + 1 + int(rng.integers(0, 4))
    quad, lin, const = U.restate(n, xvar, vm, terms)
    pairs, cols = U.structure(n, terms)
    assert len(quad) == len(pairs) and len(lin) == len(cols) == n            # the linear term over all of x fills every column
    U.assert_close_to_oracle(quad, lin, const, U.oracle_function(n, xvar, vm, terms), *U.bounds(n, terms))


def test_restatement_of_a_block_alone_is_the_bare_node(lib):
    """W = 1 is exact: 1.0 * dot(r, r) + s has the bare node's quadratic and linear bits and its constant + s; without a linear term the
    empty column has no term"""
    rng = np.random.default_rng(9)
    n = 9
    Cs = _masked(rng, 40, n, 0.3, empty=(7,))
    d = SG.signed_values(rng, 40)
    xvar, vm = np.arange(2, 11), np.arange(30, 0, -1, dtype=np.int64)
    bare = SG.restate(Cs, xvar, d, -1, 1, vm)
    quad, lin, const = U.restate(n, xvar, vm, [Term("block", Cs=Cs, d=d, sign=-1), Term("constant", value=0.375)])
    assert quad.tobytes() == bare[0].tobytes() and lin.tobytes() == bare[1].tobytes() and const == bare[2] + 0.375 and len(lin) == 8


# ---- quad_plan
def _pattern(seed=5, m=40, n=9):
    rng = np.random.default_rng(seed)
    return _masked(rng, m, n, 0.3, empty=(7,))


def test_quad_plan_rows_of_sparse_sums(lib):
    from parametron_jl_amd.lazyexpression import LsqTerm
    from parametron_jl_amd.moi import quad_plan
    from test_record_tape_host import _block
    idx = np.arange(2, 11)
    r1, r2 = _sparse_block(_pattern(5), idx), _sparse_block(_pattern(6, m=17), idx)
    ridge = [LsqTerm("block", r=r1), LsqTerm("diag", xvars=r1.xvars, param=object())]
    two = [LsqTerm("block", r=r1, scale=2.0), LsqTerm("block", r=r2, scale=-1.0), LsqTerm("diag", xvars=_xvars([3, 5, 9])), LsqTerm("constant", scale=2.0)]
    scaled = [LsqTerm("block", r=r1, scale=2.0)]
    vm = np.arange(1, 20, dtype=np.int64)
    for terms in (ridge, two, scaled):
        for mode in ("auto", "canonical"):
            for small in (True, False):
                for handoff in ("moi", "device"):
                    for is_objective in (True, False):
                        p = quad_plan(terms, False, "quad", 99, is_objective, mode, small, handoff, vm, sparse_sums=True)
                        assert p.mode == "canonical-sparse-sum" and p.terms is terms and not p.canonicalize and not p.gram_record
                        assert p.operands() == [t.r for t in terms if t.kind == "block"]
        # the default keyword: today's answer
        p = quad_plan(terms, False, "quad", 99, True, "canonical", False, "moi", None)
        assert p.mode == "literal" and p.canonicalize
        assert quad_plan(terms, False, "quad", 99, True, "auto", False, "moi", None).mode == "literal"
        # literal mode and host_csc keep today's path (which refuses the ragged residual when it materialises)
        p = quad_plan(terms, False, "quad", 99, True, "literal", False, "moi", None, sparse_sums=True)
        assert p.mode == "literal" and not p.canonicalize
        p = quad_plan(terms, False, "quad", 99, True, "canonical", False, "host_csc", vm, sparse_sums=True)
        assert p.mode == "literal" and p.canonicalize
    # the bare node is not a sum
    assert quad_plan(scaled[:1], True, "quad", 99, True, "auto", False, "moi", vm, sparse_sums=True).mode == "canonical-sparse"
    # a dense block beside a sparse one, blocks over different x, a term over variables outside x, nine blocks, 33 terms: today's answers
    dense = _block(30, idx)
    others = {"dense beside sparse": [LsqTerm("block", r=r1), LsqTerm("block", r=dense)],
              "different x": [LsqTerm("block", r=r1), LsqTerm("block", r=_sparse_block(_pattern(6), np.arange(3, 12)))],
              "outside x": [LsqTerm("block", r=r1), LsqTerm("diag", xvars=_xvars([1, 2]))],
              "unordered part": [LsqTerm("block", r=r1), LsqTerm("diag", xvars=_xvars([5, 3]))],
              "nine blocks": [LsqTerm("block", r=r1)] * 9,
              "33 terms": [LsqTerm("block", r=r1)] + [LsqTerm("constant")] * 32}
    for name, terms in others.items():
        for small in (True, False):
            p = quad_plan(terms, False, "quad", 99, True, "canonical", small, "moi", vm, sparse_sums=True)
            assert p.mode == "literal" and p.canonicalize, name
            assert quad_plan(terms, False, "quad", 99, True, "auto", small, "moi", vm, sparse_sums=True).mode == "literal", name
    # dense sums are untouched by the keyword
    dsum = [LsqTerm("block", r=dense), LsqTerm("diag", xvars=dense.xvars)]
    for flag in (False, True):
        assert quad_plan(dsum, False, "quad", 99, True, "canonical", False, "moi", None, sparse_sums=flag).mode == "canonical-sum"


def test_a_number_times_dot_of_variables_is_a_diagonal_term_for_the_sparse_combine_only(lib):
    """0.5 * dot(u, u) over plain Variables is multiplied on the host; the node description reads it as one diagonal term of weight 0.5,
    marked host_scaled: the sparse combine takes it, the dense combine keeps today's literal answer"""
    import parametron_jl_amd as P
    from parametron_jl_amd.lazyexpression import LsqTerm, _lsq_of
    from parametron_jl_amd.moi import quad_plan
    from test_record_tape_host import _block
    model = _model()
    x = [P.Variable(model) for _ in range(9)]
    u = [x[1], x[2], x[4]]
    one = _lsq_of(P.dot(u, u), None)
    assert len(one) == 1 and (one[0].kind, one[0].scale, one[0].host_scaled, one[0].xvars.vars.tolist()) == ("diag", 1.0, False, [2, 3, 5])
    half = _lsq_of(0.5 * P.dot(u, u), None)
    assert len(half) == 1 and (half[0].kind, half[0].scale, half[0].host_scaled, half[0].xvars.vars.tolist()) == ("diag", 0.5, True, [2, 3, 5])
    neg = half[0].scaled(-1.0)
    assert (neg.scale, neg.host_scaled) == (-0.5, True)
    assert _lsq_of(0.5 * P.dot(u, u) + 1.0 * x[0] * x[0], None) is None                      # not one weight
    idx = np.arange(1, 10)
    sparse = [LsqTerm("block", r=_sparse_block(_pattern(5), idx)), neg]
    assert quad_plan(sparse, False, "quad", 99, True, "auto", True, "moi", None, sparse_sums=True).mode == "canonical-sparse-sum"
    dense = _block(30, idx)
    for flag in (False, True):
        p = quad_plan([LsqTerm("block", r=dense), neg], False, "quad", 99, True, "canonical", False, "moi", None, sparse_sums=flag)
        assert p.mode == "literal" and p.canonicalize
        assert quad_plan([LsqTerm("block", r=dense), one[0]], False, "quad", 99, True, "canonical", False, "moi", None, sparse_sums=flag).mode == "canonical-sum"


def test_model_asks_for_sparse_sums(lib):
    import inspect

    from parametron_jl_amd.model import Model
    assert "sparse_sums=True" in inspect.getsource(Model._plan_quadratic_records)


# ---- the record
@pytest.mark.parametrize("small", [False, True])
def test_canonical_sparse_sum_record_tape(lib, small):
    from parametron_jl_amd.device import DNum
    from parametron_jl_amd.lazyexpression import LsqTerm
    from parametron_jl_amd.moi import QuadPlan
    C1, C2 = _pattern(5), _pattern(6, m=17)
    ctx = StubContext(lib)
    idx = np.arange(2, 11)
    r1, r2 = _sparse_block(C1, idx, vec=_b(40), sign=-1, ctx=ctx), _sparse_block(C2, idx, ctx=ctx)
    lam = DNum.__new__(DNum)
    lam.buf = FAKE
    part = _xvars([3, 4, 9])
    terms = [LsqTerm("block", r=r1), LsqTerm("block", r=r2, scale=0.5), LsqTerm("diag", xvars=part, param=lam), LsqTerm("linear", xvars=r1.xvars, vec=_b(9)),
             LsqTerm("constant", scale=2.0)]
    model = _model(small=small)
    rec = _objective(model, _quad_out(7, 7), QuadPlan("canonical-sparse-sum", terms=terms))
    vm = np.arange(1, 30, dtype=np.int64)[::-1].copy()
    emit = rec.compile(ctx, VARMAP_BUF, vm)
    spec = [Term("block", Cs=C1), Term("block", Cs=C2), Term("diag", cols=[1, 2, 7]), Term("linear", v=np.zeros(9)), Term("constant")]
    pairs, cols = U.structure(9, spec)
    assert (7, 7) in pairs and len(cols) == 9
    f = rec.f
    assert len(f.quadratic_terms) == len(pairs) and len(f.affine_terms) == len(cols)
    assert set(rec.dev) == {"quad", "lin", "const"}
    assert [k for _, k in rec.buffers] == ["quad", "lin", "const"] and rec.buffers[0][0] is f.quadratic_terms and rec.buffers[1][0] is f.affine_terms
    T1, T2 = r1.gram_tables(), r2.gram_tables()
    # allocations: the blocks' tables (eleven each), the merge's (three, two per block, one position table), beyond the small plan the three
    # twins, then three scratch buffers per block
    S = U.merge_tables(9, spec)
    merged = [S.pair_j, S.pair_k, S.lin_col] + S.quad_at + S.lin_at + [S.term_pos[2]]
    want = [max(getattr(T, k).nbytes, 8) for T in (T1, T2) for k in T.TABLES] + [max(a.nbytes, 8) for a in merged]
    want += ([] if small else [24 * S.nq, 16 * S.nlin, 16]) + [v for T in (T1, T2) for v in (24 * T.nq, 16 * T.nlin, 8)]
    assert ctx.allocs == want
    if small:
        assert rec.dev == {"quad": f.quadratic_terms.ctypes.data, "lin": f.affine_terms.ctypes.data, "const": rec._cbuf.ctypes.data}
        assert rec.copies() == []
    else:
        assert len(rec.copies()) == 3
    # the static index fields are on the host before the first update, through the hand-off's map
    x = vm[idx - 1]
    assert f.quadratic_terms["row"].tolist() == [x[j] for j, _ in pairs] and f.quadratic_terms["col"].tolist() == [x[k] for _, k in pairs]
    assert f.affine_terms["var"].tolist() == [x[j] for j in cols]
    assert rec.varmap_hooks == [] and rec.delivered == () and not rec.side_lane_ok
    n_alloc = len(ctx.allocs)
    emit(ctx)
    assert [name for name, _ in ctx.raw] == ["pmt_sparse_gram_f64", "pmt_sparse_gram_f64", "pmt_sparse_gram_sum_f64"]
    emit(ctx)
    assert len(ctx.allocs) == n_alloc and len(ctx.raw) == 6                          # update! allocates nothing
    for (name, args) in ctx.raw[:3]:
        assert len(args) == len(lib.SIGNATURES[name][1]) - 1                        # (the context appends the stream)
    assert ctx.calls[0] == ("pmt_sparse_gram_f64", (T1.nq, T1.nruns, T1.nlong, T1.nlin, T1.nlin_runs, T1.nlin_long, 40, -1, 1))
    assert ctx.calls[1] == ("pmt_sparse_gram_f64", (T2.nq, T2.nruns, T2.nlong, T2.nlin, T2.nlin_runs, T2.nlin_long, 17, 0, 1))
    assert ctx.calls[2] == ("pmt_sparse_gram_sum_f64", (9, 5, S.nq, S.nlin))
    # the descriptors the combine reads
    arr = lib.SparseLsqTerm * 5
    d = arr.from_address(ctx.raw[2][1][1])
    assert [t.kind for t in d] == [lib.PMT_LSQ_BLOCK, lib.PMT_LSQ_BLOCK, lib.PMT_LSQ_DIAG, lib.PMT_LSQ_LINEAR, lib.PMT_LSQ_CONSTANT]
    assert [t.scale for t in d] == [1.0, 0.5, 1.0, 1.0, 2.0] and [t.weight for t in d] == [None, None, FAKE, None, None]
    assert all(d[b].quad and d[b].lin and d[b].constant and d[b].quad_at and d[b].lin_at for b in (0, 1))
    assert d[2].pos and d[2].nvec == 3 and d[2].vec is None and d[2].sign == 0 and d[3].pos is None and d[3].nvec == 9 and d[3].vec


# ---- argument validation without a GPU
def _sum_call(lib, descs=None, nterms=None, **kw):
    B = lib.PMT_LSQ_BLOCK
    block = dict(kind=B, quad=FAKE, lin=FAKE, constant=FAKE, quad_at=FAKE, lin_at=FAKE)
    terms = [block, dict(kind=lib.PMT_LSQ_DIAG, nvec=4)] if descs is None else descs
    arr = lib.sparse_lsq_terms([dict(block, **t) if t.get("kind") == B else t for t in terms])
    a = dict(n=4, terms=C.addressof(arr), nterms=len(terms) if nterms is None else nterms, pair_j=FAKE, pair_k=FAKE, nq=3, lin_col=FAKE, nlin=2, xvar=FAKE,
             varmap=FAKE, out_quad=FAKE, out_lin=FAKE, out_const=FAKE)
    a.update(kw)
    lib.call("pmt_sparse_gram_sum_f64", *a.values(), None)


def test_entry_point_validates_before_any_device_call(lib):
    B, D, L = lib.PMT_LSQ_BLOCK, lib.PMT_LSQ_DIAG, lib.PMT_LSQ_LINEAR
    for name in ("terms", "pair_j", "pair_k", "lin_col", "xvar", "out_quad", "out_lin", "out_const"):
        with pytest.raises(lib.ArgumentError, match="null"):
            _sum_call(lib, **{name: None})
    with pytest.raises(lib.ArgumentError, match="varmap"):
        _sum_call(lib, varmap=None)
    for name in ("nq", "nlin"):
        with pytest.raises(lib.ArgumentError, match="negative"):
            _sum_call(lib, **{name: -1})
    with pytest.raises(lib.DimensionMismatch):
        _sum_call(lib, n=-1)
    with pytest.raises(lib.DimensionMismatch):
        _sum_call(lib, nlin=5)
    for field in ("quad", "lin", "constant", "quad_at", "lin_at"):
        with pytest.raises(lib.ArgumentError, match="block"):
            _sum_call(lib, descs=[{"kind": B, field: None}])
    for nterms in (0, 33):
        with pytest.raises(lib.ArgumentError, match="1 .. 32"):
            _sum_call(lib, nterms=nterms)
    with pytest.raises(lib.ArgumentError, match="1 .. 8"):
        _sum_call(lib, descs=[{"kind": B}] * 9)
    with pytest.raises(lib.ArgumentError, match="1 .. 8"):
        _sum_call(lib, descs=[{"kind": D, "nvec": 4}])
    for sign in (0, 2, -2):
        with pytest.raises(lib.ArgumentError, match="sign"):
            _sum_call(lib, descs=[{"kind": B}, {"kind": D, "nvec": 4, "vec": FAKE, "sign": sign}])
    with pytest.raises(lib.ArgumentError, match="sign"):
        _sum_call(lib, descs=[{"kind": B}, {"kind": D, "nvec": 4, "sign": 1}])          # a sign without v
    with pytest.raises(lib.ArgumentError, match="linear"):
        _sum_call(lib, descs=[{"kind": B}, {"kind": L, "nvec": 4}])
    with pytest.raises(lib.DimensionMismatch, match="vector length"):
        _sum_call(lib, descs=[{"kind": B}, {"kind": D, "nvec": 3}])                      # part of x without its position table
    with pytest.raises(lib.DimensionMismatch, match="vector length"):
        _sum_call(lib, descs=[{"kind": B}, {"kind": L, "vec": FAKE, "nvec": 5, "pos": FAKE}])
    with pytest.raises(lib.ArgumentError, match="kind"):
        _sum_call(lib, descs=[{"kind": B}, {"kind": 9}])
