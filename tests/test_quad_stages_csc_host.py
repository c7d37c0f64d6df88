"""CPU-only: horizon stage costs for the device hand-off (pmt_quad_stages_csc_f64; record mode "canonical-stages-csc").
pmt_quad_stages_csc_check and the entry point's refusals without a device; the quad_plan row with and without stage_csc; the
block -> (rows, cols) function of the hand-off against np.triu of a dense block-diagonal matrix; what one compiled record allocates and
calls."""
import ctypes as C
import inspect

import numpy as np
import pytest

import __graft_entry__ as entry
import test_quad_stages_diag_host as HD
import test_quad_stages_terms_host as HT
from test_quad_stages_host import _horizon
from test_record_tape_host import FAKE, VARMAP_BUF, StubContext, _b, _model, _objective, _quad_out


@pytest.fixture(scope="module")
def lib():
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


# ---- 1. pmt_quad_stages_csc_check and the entry point without a device
def _check(lib, arr, terms, diags, T, consts, nconsts, nvalues, nlin, name="pmt_quad_stages_csc_check"):
    adr = lambda a: C.addressof(a) if a is not None else None
    lib.call(name, adr(arr), adr(terms), adr(diags), T, adr(consts), nconsts, nvalues, nlin)


def test_the_symbols_are_exported_with_their_signatures(lib):
    dll = C.CDLL(lib.LIB_PATH)
    assert hasattr(dll, "pmt_quad_stages_csc_check") and hasattr(dll, "pmt_quad_stages_csc_f64")
    assert len(lib.SIGNATURES["pmt_quad_stages_csc_check"][1]) == 8 and len(lib.SIGNATURES["pmt_quad_stages_csc_f64"][1]) == 13
    assert lib.SIGNATURES["pmt_quad_stages_csc_f64"][1][7] is C.c_double          # alpha


def test_check_accepts_valid_tables(lib):
    """the value slices are counted in doubles: n(n+1)/2 per form stage, n per identity stage"""
    arr, terms, diags, consts, nv, nl = HD._tables(lib)
    assert nv == 6 + 4 + 15 + 6 + 28 and nl == 25
    _check(lib, arr, terms, diags, 5, consts, 2, nv, nl)
    _check(lib, arr, terms, None, 5, consts, 2, nv, nl)
    _check(lib, arr, terms, diags, 5, None, 0, nv + 3, nl + 1)
    _check(lib, None, None, None, 0, None, 0, 0, 0)
    # slices in another order than the table's, with a gap
    arr, terms, diags, consts, nv, nl = HD._tables(lib, {(0, "quad_at"): 6 + 4 + 15 + 6 + 28 + 1, (1, "quad_at"): 0})
    _check(lib, arr, terms, diags, 5, consts, 2, nv + 1 + 6, nl)


@pytest.mark.parametrize("edit,T,dv,dl", [({}, 5, -1, 0), ({}, 5, 0, -1), ({(1, "quad_at"): -1}, 5, 0, 0), ({(1, "quad_at"): 5}, 5, 0, 0),
                                          ({(2, "quad_at"): 6 + 3}, 5, 0, 0), ({(3, "lin_at"): 11}, 5, 0, 0), ({(4, "quad_at"): 32}, 5, 0, 0),
                                          ({(1, "n"): 0}, 5, 0, 0), ({(1, "n"): 257}, 5, 40000, 400), ({(2, "ldq"): 4}, 5, 0, 0), ({}, -1, 0, 0)],
                         ids=["values-past-the-end", "lin-past-the-end", "slice-below-zero", "identity-overlap-by-one", "form-overlaps-identity",
                              "lin-overlap-by-one", "last-slice-leaves-nvalues", "n-zero", "n-257", "ldq-below-n", "T-negative"])
def test_check_refuses_mismatches(lib, edit, T, dv, dl):
    arr, terms, diags, consts, nv, nl = HD._tables(lib, edit)
    with pytest.raises(lib.DimensionMismatch, match="quad_stages"):
        _check(lib, arr, terms, diags, T, consts, 2, nv + dv, nl + dl)


REFUSED = HD.test_check_refuses_invalid_arguments.pytestmark[0]


@pytest.mark.parametrize("edit,dedit", REFUSED.args[1], ids=REFUSED.kwargs["ids"])
def test_check_refuses_what_the_diag_check_refuses_as_invalid(lib, edit, dedit):
    arr, terms, diags, consts, nv, nl = HD._tables(lib, edit, dedit)
    with pytest.raises(lib.ArgumentError, match="quad_stages"):
        _check(lib, arr, terms, diags, 5, consts, 2, nv, nl)


def test_check_refuses_with_the_codes_of_the_diag_check(lib):
    arr, terms, diags, consts, nv, nl = HD._tables(lib)
    cases = [((None, terms, diags, 5, consts, 2, nv, nl), lib.ArgumentError), ((arr, None, diags, 5, consts, 2, nv, nl), lib.ArgumentError),
             ((arr, terms, diags, 5, None, 1, nv, nl), lib.ArgumentError), ((arr, terms, diags, 5, consts, -1, nv, nl), lib.DimensionMismatch),
             ((arr, terms, diags, 5, consts, 33, nv, nl), lib.DimensionMismatch), ((arr, terms, diags, 5, consts, 2, nv - 1, nl), lib.DimensionMismatch)]
    for args, exc in cases:
        for name in ("pmt_quad_stages_diag_check", "pmt_quad_stages_csc_check"):
            with pytest.raises(exc):
                _check(lib, *args, name=name)
    for edit in HT.test_check_refuses_what_the_unweighted_check_refuses_as_invalid.pytestmark[0].args[1][1:]:
        arr3, terms3, consts3, nq3, nl3 = HT._tables(lib, edit)
        with pytest.raises(lib.ArgumentError):
            _check(lib, arr3, terms3, None, 3, consts3, 2, nq3, nl3)


def _launch(lib, stages=FAKE, terms=FAKE, diags=FAKE, T=2, consts=FAKE, nconsts=1, varmap=FAKE, alpha=1.0, values=FAKE, lin=FAKE, sconsts=FAKE,
            const=FAKE):
    lib.call("pmt_quad_stages_csc_f64", stages, terms, diags, T, consts, nconsts, varmap, alpha, values, lin, sconsts, const, None)


@pytest.mark.parametrize("bad", [{"stages": None}, {"terms": None}, {"consts": None}, {"varmap": None}, {"values": None}, {"lin": None},
                                 {"sconsts": None}, {"const": None}, {"const": None, "T": 0}, {"consts": None, "T": 0},
                                 {"diags": None, "const": None}, {"values": None, "alpha": -1.0}],
                         ids=["null-table", "null-terms", "null-consts", "null-varmap", "null-values", "null-lin", "null-stage-consts", "null-const",
                              "null-const-T0", "null-consts-T0", "null-const-without-diags", "null-values-maximize"])
def test_entry_point_refuses_null_pointers_before_any_device_call(lib, bad):
    with pytest.raises(lib.ArgumentError, match="quad_stages_csc"):
        _launch(lib, **bad)


@pytest.mark.parametrize("bad", [{"T": -1}, {"nconsts": -1}, {"nconsts": 33}], ids=["T", "nconsts", "nconsts-33"])
def test_entry_point_refuses_bad_counts(lib, bad):
    with pytest.raises(lib.DimensionMismatch, match="quad_stages_csc"):
        _launch(lib, **bad)


# ---- 2. the quad_plan row
NVARS = 200
IDENT = np.arange(1, NVARS + 1, dtype=np.int64)


def _plan(terms, **args):
    """as Model calls quad_plan, under the device hand-off with an index map that keeps every order"""
    args.setdefault("stage_csc", True)
    args.setdefault("handoff", "device")
    args.setdefault("varmap", IDENT)
    return HD._plan(terms, **args)


def _rho_horizon(**kw):
    return HD._rho_horizon(rho=HD._Scalar(), **kw)


def test_plan_fires_under_the_device_handoff_with_an_ordered_map(lib):
    terms = _rho_horizon()
    p = _plan(terms)
    assert p.mode == "canonical-stages-csc" and not p.canonicalize and not p.gram_record
    assert len(p.stages) == 10 and [q.mat is None for q in p.stages] == [False, True] * 5 and p.stage_diags is None
    assert [id(q) for q in p.stages[::2]] == [id(t.r) for t in terms[::2]]
    assert [(s.scale, s.param is not None) for s in p.stage_terms] == [(1.0, False), (1.0, True)] * 5
    assert sorted(id(r) for r in p.operands() if r.mat is not None) == sorted(id(t.r) for t in terms[::2])
    # the optimizer numbers its variables from 3 on (MockOptimizer(variable_offset=2)): an offset map keeps every order
    assert _plan(terms, varmap=IDENT + 2).mode == "canonical-stages-csc"
    # stages that change places under the map keep their own order: still the row
    moved = IDENT.copy()
    moved[0:4] = [150, 151, 152, 153]                                     # the first stage behind all others
    assert _plan(terms, varmap=moved).mode == "canonical-stages-csc"
    # forms alone, weighted forms, a rider, a linear term and a constant
    assert _plan(_horizon()).mode == "canonical-stages-csc" and _plan(_horizon()).stage_terms is None
    assert _plan([t.scaled(0.5) for t in _horizon()]).stage_terms is not None
    hz = _horizon()
    rid = HD._diag(hz[2].r.xvars.vars, scale=2.0, host_scaled=True)
    p = _plan(hz + [rid])
    assert p.mode == "canonical-stages-csc" and p.stage_diags == [None, None, rid] + [None] * 6
    # exactly at the row's threshold
    assert _plan(terms, nq=1 << 14).mode == "canonical-stages-csc"


def test_plan_a_map_that_permutes_inside_one_stage_is_literal(lib):
    vm = IDENT.copy()
    vm[[1, 2]] = vm[[2, 1]]                                               # inside the first form's vector
    p = _plan(_rho_horizon(), varmap=vm)
    assert (p.mode, p.canonicalize) == ("literal", True) and p.stages is None
    vm = IDENT.copy()
    vm[[20, 21]] = vm[[21, 20]]                                           # inside the first identity stage's vector
    p = _plan(_rho_horizon(), varmap=vm)
    assert (p.mode, p.canonicalize) == ("literal", True) and p.stages is None
    # a reversed map permutes inside every stage
    assert _plan(_rho_horizon(), varmap=IDENT[::-1].copy()).mode == "literal"


@pytest.mark.parametrize("args,expected", [(dict(handoff="host_csc"), ("literal", True)), (dict(small=True), ("literal", True)),
                                           (dict(quadratic_mode="auto"), ("literal", False)), (dict(quadratic_mode="literal"), ("literal", False)),
                                           (dict(nq=(1 << 14) - 1), ("literal", True)), (dict(is_objective=False), ("literal", True))],
                         ids=["host_csc", "small", "auto", "literal", "nq-below-2^14", "constraint"])
def test_plan_other_conditions_are_untouched(lib, args, expected):
    p = _plan(_rho_horizon(), **args)
    assert (p.mode, p.canonicalize) == expected and p.stages is None


def test_plan_eight_vectors_stay_literal_under_the_device_handoff(lib):
    """2 .. 8 vectors are canonical-groups through the MOI boundary; the groups have no device route"""
    for terms in (HD._rho_horizon(stages=4, rho=HD._Scalar()), _horizon(stages=8), _horizon(stages=2)):
        p = _plan(terms)
        assert (p.mode, p.canonicalize) == ("literal", True) and p.stages is None and p.groups is None
    assert _plan(_horizon(stages=8), handoff="moi", varmap=None).mode == "canonical-groups"


def test_plan_lists_the_stage_row_refuses_stay_literal(lib):
    for what in ("part-of-a-form-stage", "across-two-stages", "two-riders-on-one-vector", "unsorted-identity-vector", "block-among-the-stages"):
        p = _plan(HD._literal_lists(what))
        assert (p.mode, p.canonicalize) == ("literal", True) and p.stages is None, what


def test_plan_without_the_keyword_is_as_it_was(lib):
    from parametron_jl_amd import model, moi
    assert inspect.signature(moi.quad_plan).parameters["stage_csc"].default is False
    assert list(inspect.signature(moi.quad_plan).parameters)[-1] == "stage_csc"
    assert "stage_csc=True" in inspect.getsource(model.Model._plan_quadratic_records)
    for terms in (_rho_horizon(), _horizon(), [t.scaled(0.5) for t in _horizon()]):
        for vm in (IDENT, IDENT + 2):
            p = _plan(terms, stage_csc=False, varmap=vm)
            assert (p.mode, p.canonicalize) == ("literal", True) and p.stages is None
    # through the MOI boundary the keyword changes nothing
    for terms in (_rho_horizon(), _horizon()):
        a, b = _plan(terms, handoff="moi", varmap=None), _plan(terms, handoff="moi", varmap=None, stage_csc=False)
        forms = lambda p: [id(q) for q in p.stages if q.mat is not None]
        assert a.mode == b.mode == "canonical-stages" and len(a.stages) == len(b.stages) and forms(a) == forms(b)
    # the bare forms keep their rows
    one = _horizon(stages=1, shifted=False)
    assert moi.quad_plan(one, True, "quad", 1 << 20, True, "canonical", False, "device", IDENT, stage_csc=True).mode == "canonical-form"


# ---- 3. the hand-off's pattern of the value buffer
def _dense_pattern(blocks, nvars):
    """(rows, cols), 1-based, of the upper triangle of the dense block-diagonal matrix, in CSC order, and per entry the stage it belongs to"""
    M = np.zeros((nvars, nvars), dtype=np.int64)
    for s, (idx, _, diagonal) in enumerate(blocks):
        idx = np.asarray(idx) - 1
        if diagonal:
            M[idx, idx] = s + 1
        else:
            M[np.ix_(idx, idx)] = s + 1
    U = np.triu(M)
    cols, rows = np.nonzero(U.T)                                          # column by column, rows ascending
    return rows + 1, cols + 1, U[rows, cols] - 1


def _blocks(sets, diagonal):
    """value slices one behind the other in the order of the sets' first index, as _compile_stages_csc lays them out"""
    order = np.argsort([s[0] for s in sets])
    at, pos = {}, 0
    for k in order:
        at[k] = pos
        pos += len(sets[k]) if diagonal[k] else len(sets[k]) * (len(sets[k]) + 1) // 2
    return [(np.asarray(s, dtype=np.int64), at[k], diagonal[k]) for k, s in enumerate(sets)], pos


@pytest.mark.parametrize("layout", ["in-order", "interleaved", "stages-out-of-order"])
def test_stage_blocks_pattern_is_the_upper_triangle_of_the_block_diagonal_matrix(lib, layout):
    from parametron_jl_amd.handoff import stage_blocks_pattern
    sizes, diagonal = [5, 3, 1, 4, 2, 6, 1], [False, True, True, False, True, False, False]
    if layout == "interleaved":
        pool = iter(range(3, 100))                                        # (optimizer indices from 3 on)
        sets = [[] for _ in sizes]
        for k in range(max(sizes)):
            for s, n in zip(sets, sizes):
                if k < n:
                    s.append(next(pool))
    else:
        start = np.concatenate([[3], 3 + np.cumsum(sizes)])
        sets = [list(range(start[g], start[g] + n)) for g, n in enumerate(sizes)]
        if layout == "stages-out-of-order":
            sets = [sets[g] for g in (3, 0, 6, 1, 5, 2, 4)]
            diagonal = [diagonal[g] for g in (3, 0, 6, 1, 5, 2, 4)]
    blocks, nvalues = _blocks(sets, diagonal)
    assert nvalues == 15 + 3 + 1 + 10 + 2 + 21 + 1
    rows, cols = stage_blocks_pattern(blocks, nvalues)
    assert rows.dtype == cols.dtype == np.int64 and len(rows) == len(cols) == nvalues and np.all(rows <= cols) and rows.min() >= 3
    nvars = 2 + sum(sizes)
    wr, wc, _ = _dense_pattern(blocks, nvars)
    # the same set of entries, each exactly once
    assert sorted(zip(cols.tolist(), rows.tolist())) == list(zip(wc.tolist(), wr.tolist()))
    # entry at + k(k+1)/2 + j is (idx[j], idx[k]); an identity stage's entry at + j is (idx[j], idx[j])
    for idx, at, diag in blocks:
        n = len(idx)
        if diag:
            assert np.array_equal(rows[at:at + n], idx) and np.array_equal(cols[at:at + n], idx)
        else:
            for k in range(n):
                for j in range(k + 1):
                    assert (rows[at + k * (k + 1) // 2 + j], cols[at + k * (k + 1) // 2 + j]) == (idx[j], idx[k])
    # consecutive indices per stage: the buffer is already in CSC order (the hand-off then takes it as P's value array)
    in_csc_order = np.array_equal(rows, wr) and np.array_equal(cols, wc)
    assert in_csc_order == (layout != "interleaved")


def test_stage_blocks_pattern_refuses_slices_that_do_not_tile_the_buffer(lib):
    from parametron_jl_amd.handoff import stage_blocks_pattern
    a, b = np.array([1, 2, 3]), np.array([4, 5])
    stage_blocks_pattern([(a, 0, False), (b, 6, True)], 8)
    with pytest.raises(lib.ArgumentError, match="overlap"):
        stage_blocks_pattern([(a, 0, False), (b, 5, True)], 8)
    with pytest.raises(lib.ArgumentError, match="leave"):
        stage_blocks_pattern([(a, 0, False), (b, 7, True)], 8)
    with pytest.raises(lib.ArgumentError, match="unnamed"):
        stage_blocks_pattern([(a, 0, False), (b, 7, True)], 9)


# ---- 4. one compiled record on the stub context
def _record(lib, plan, varmap, sense=None):
    model = _model(handoff="device")
    if sense is not None:
        model.sense = sense
    rec = _objective(model, _quad_out(7, 7), plan)
    ctx = StubContext(lib)
    return rec, ctx, rec.compile(ctx, VARMAP_BUF, varmap)


def test_record_is_one_call_and_allocates_nothing_after_compile(lib):
    T, nx, nu = 6, 5, 3
    vm = IDENT + 2
    rec, ctx, emit = _record(lib, _plan(_rho_horizon(stages=T, nx=nx, nu=nu), varmap=vm), vm)
    nv, nl = T * (nx * (nx + 1) // 2 + nu), T * (nx + nu)
    # P's values, the linear terms, the constant, the stage constants; an index buffer per identity stage; the stage table, the terms,
    # the constants: no quadratic term structs, no arena, no gather tables
    assert ctx.allocs == [8 * nv, 16 * nl, 8, 8 * 2 * T] + [8 * nu] * T + [56 * 2 * T, 40 * 2 * T, 24]
    assert rec.mode == "canonical-stages-csc" and set(rec.dev) == {"lin", "const", "P_stage_values", "P_stage_blocks"}
    assert len(rec.f.affine_terms) == nl and len(rec.f.quadratic_terms) == 0
    assert rec.groups_ordered is None
    mark = len(ctx.allocs)
    emit(ctx)
    emit(ctx)
    assert len(ctx.allocs) == mark                                        # update! allocates nothing
    assert ctx.calls == [("pmt_quad_stages_csc_f64", (2 * T, 0, 1.0))] * 2
    name, args = ctx.raw[-1]
    assert getattr(args[2], "value", None) is None                        # no rider: no third table
    assert args[8].value == rec.dev["P_stage_values"] and args[9].value == rec.dev["lin"] and args[11].value == rec.dev["const"]
    # the blocks: optimizer indices, slices one behind the other in the order of the first index
    blocks = rec.dev["P_stage_blocks"]
    # (the horizon's x_t lie in front of all u_t: the forms' slices come first, then the identity stages')
    for k, (idx, off, diag) in enumerate(blocks):
        t = k // 2
        if k % 2:
            assert np.array_equal(idx, np.arange(nu) + 1 + T * nx + t * nu + 2) and off == T * nx * (nx + 1) // 2 + t * nu and diag is True
        else:
            assert np.array_equal(idx, np.arange(nx) + 1 + t * nx + 2) and off == t * nx * (nx + 1) // 2 and diag is False
    # only the linear terms and the constant travel to the host function
    assert [key for _, key in rec.buffers] == ["quad", "lin", "const"] and [d for _, d in rec.copies()] == [rec.dev["lin"], rec.dev["const"]]


def test_record_for_maximize_passes_minus_one_and_riders_get_their_table(lib):
    T, n = 9, 4
    terms = _horizon(stages=T, n=n)
    rid = HD._diag(terms[4].r.xvars.vars, scale=0.5, param=HD._Scalar(), vec=_b(n), sign=-1)
    rec, ctx, emit = _record(lib, _plan(terms + [rid]), IDENT, sense="Maximize")
    nv, nl = T * n * (n + 1) // 2, T * n
    assert ctx.allocs == [8 * nv, 16 * nl, 8, 8 * T, 56 * T, 40 * T, 24, 32 * T]
    emit(ctx)
    assert ctx.calls == [("pmt_quad_stages_csc_f64", (T, 0, -1.0))]
    assert getattr(ctx.raw[-1][1][2], "value", None) is not None


def test_record_lays_the_slices_out_by_first_optimizer_index(lib):
    """Variables dealt out element by element: every stage keeps its order, the slices follow the stages' first optimizer index, and the
    hand-off's pattern of the buffer is not in CSC order (its gather places the values)"""
    from parametron_jl_amd.handoff import stage_blocks_pattern
    T, nx, nu = 5, 4, 3
    terms = _rho_horizon(stages=T, nx=nx, nu=nu)
    pool = iter(range(1, 100))
    vecs = [[] for _ in terms]
    for k in range(nx):
        for vec, n in zip(vecs[::-1], ([nx, nu] * T)[::-1]):            # the LAST stage gets the first index
            if k < n:
                vec.append(next(pool))
    for t, vec in zip(terms, vecs):
        (t.r.xvars if t.kind == "form" else t.xvars).vars = np.array(vec, dtype=np.int64)
    rec, ctx, emit = _record(lib, _plan(terms), IDENT)
    emit(ctx)
    assert ctx.calls == [("pmt_quad_stages_csc_f64", (2 * T, 0, 1.0))]      # one call: no gather of the record's own
    blocks = rec.dev["P_stage_blocks"]
    offs = [off for _, off, _ in blocks]
    assert offs == sorted(offs, reverse=True) and offs[-1] == 0
    nv = T * (nx * (nx + 1) // 2 + nu)
    rows, cols = stage_blocks_pattern(blocks, nv)
    key = cols * 1000 + rows
    assert len(set(key.tolist())) == nv and not np.all(np.diff(key) > 0)


def test_record_refuses_tables_the_check_refuses(lib):
    terms = _rho_horizon(stages=5)
    terms[2].r.mat.lda = 3                                                # ldq < n
    with pytest.raises(lib.DimensionMismatch, match="quad_stages"):
        _record(lib, _plan(terms), IDENT)


# ---- 5. the entry point of a plan, decided once (QuadPlan.stage_entry), and the check in front of every upload (_Record._stage_launch)
def _constant(**kw):
    from parametron_jl_amd.lazyexpression import LsqTerm
    return LsqTerm("constant", **kw)


def test_stage_entry_of_the_plans(lib):
    from parametron_jl_amd.moi import QuadPlan
    hz = _horizon()
    rid = HD._diag(hz[2].r.xvars.vars, scale=2.0, host_scaled=True)
    plans = {"a plain horizon": (HD._plan(_horizon()), "plain"),
             "unit weights": (HD._plan([t.scaled(1.0) for t in _horizon()]), "plain"),
             "built directly": (QuadPlan("canonical-stages", stages=[t.r for t in _horizon()]), "plain"),
             "weighted stages": (HD._plan([t.scaled(0.5) for t in _horizon()]), "terms"),
             "constants only": (HD._plan(_horizon() + [_constant(scale=2.0)]), "terms"),
             "a linear term": (HD._plan(HT._edited("linear")), "terms"),
             "an identity stage": (HD._plan(HD._rho_horizon()), "diag"),
             "weighted identity stages": (HD._plan(HD._rho_horizon(rho=HD._Scalar(), scale=0.5)), "diag"),
             "a rider": (HD._plan(hz + [rid]), "diag"),
             "the csc horizon": (_plan(_rho_horizon()), "csc"),
             "the csc horizon of plain forms": (_plan(_horizon()), "csc"),
             "eight groups": (HD._plan(_horizon(stages=8)), None),
             "literal": (HD._plan(_horizon(), quadratic_mode="literal"), None),
             "no mode": (QuadPlan(None), None)}
    modes = {"plain": "canonical-stages", "terms": "canonical-stages", "diag": "canonical-stages", "csc": "canonical-stages-csc"}
    assert plans["eight groups"][0].mode == "canonical-groups" and plans["literal"][0].mode == "literal"
    for name, (plan, entry) in plans.items():
        assert plan.stage_entry == entry, name
        assert entry is None or plan.mode == modes[entry], name
    # a computed property: no constructor argument, nothing to set
    assert "stage_entry" not in inspect.signature(QuadPlan.__init__).parameters and isinstance(QuadPlan.stage_entry, property)
    with pytest.raises(AttributeError):
        plans["a plain horizon"][0].stage_entry = "terms"
    # a caller of quad_plan that does not ask for the weighted entry keeps the literal row for exactly the plans that would take it
    for terms in ([t.scaled(0.5) for t in _horizon()], _horizon() + [_constant(scale=2.0)], HT._edited("linear")):
        assert HD._plan(terms, stage_terms=False).mode == "literal"
    for terms in (_horizon(), HD._rho_horizon(), hz + [rid]):
        assert HD._plan(terms, stage_terms=False).mode == "canonical-stages"


SYMBOLS = {"plain": ("pmt_quad_stages_check", "pmt_quad_stages_f64"), "terms": ("pmt_quad_stages_terms_check", "pmt_quad_stages_terms_f64"),
           "diag": ("pmt_quad_stages_diag_check", "pmt_quad_stages_diag_f64"), "csc": ("pmt_quad_stages_csc_check", "pmt_quad_stages_csc_f64")}


def _entry_terms(entry, T=9, n=4):
    """one list per entry point; none has an identity stage, so that compile uploads nothing but the tables"""
    hz = _horizon(stages=T, n=n)
    rid = HD._diag(hz[4].r.xvars.vars, scale=0.5, param=HD._Scalar(), vec=_b(n), sign=-1)
    return {"plain": hz, "terms": [t.scaled(0.5) for t in hz] + [_constant(scale=2.0)], "diag": hz + [rid], "csc": hz + [rid]}[entry]


class _Uploads(StubContext):
    """the stub context, noting every upload beside the allocations"""
    def __init__(self, lib):
        super().__init__(lib)
        self.uploads = []

    def upload_new(self, host):
        self.uploads.append(np.ascontiguousarray(host).nbytes)
        return super().upload_new(host)


def _compile_spied(lib, monkeypatch, entry, terms):
    """compile the plan of `terms` on the stub context with _lib.call spied on: (the record, the context, the emitter or the exception, the
    library calls made through _lib.call with the uploads made before each)"""
    plan = _plan(terms) if entry == "csc" else HD._plan(terms)
    assert plan.stage_entry == entry
    rec = _objective(_model(handoff="device") if entry == "csc" else _model(), _quad_out(7, 7), plan)
    ctx, seen, real = _Uploads(lib), [], lib.call

    def spy(name, *args):
        seen.append((name, len(ctx.uploads)))
        return real(name, *args)
    monkeypatch.setattr(lib, "call", spy)
    try:
        out = rec.compile(ctx, VARMAP_BUF, IDENT if entry == "csc" else None)
    except Exception as e:                                                # noqa: BLE001 (handed to the caller, which asserts its class)
        out = e
    monkeypatch.undo()
    return rec, ctx, out, seen


@pytest.mark.parametrize("entry", ["plain", "terms", "diag", "csc"])
def test_record_calls_its_entrys_check_and_no_other_before_its_launch(lib, monkeypatch, entry):
    T, n = 9, 4
    rec, ctx, emit, seen = _compile_spied(lib, monkeypatch, entry, _entry_terms(entry, T, n))
    check, launch = SYMBOLS[entry]
    assert seen == [(check, 0)]                                           # that check alone, and in front of the first upload
    tables = {"plain": [56 * T], "terms": [56 * T, 40 * T, 24], "diag": [56 * T, 40 * T, 24, 32 * T], "csc": [56 * T, 40 * T, 24, 32 * T]}[entry]
    assert ctx.uploads == tables and ctx.allocs[-len(tables):] == tables and ctx.calls == []
    emit(ctx)
    assert [name for name, _ in ctx.calls] == [launch] and len(ctx.uploads) == len(tables)


@pytest.mark.parametrize("entry", ["plain", "terms", "diag", "csc"])
def test_record_uploads_nothing_when_its_entrys_check_refuses(lib, monkeypatch, entry):
    T, n = 9, 4
    terms = _entry_terms(entry, T, n)
    terms[3].r.mat.lda = 3                                                # ldq < n
    rec, ctx, err, seen = _compile_spied(lib, monkeypatch, entry, terms)
    assert type(err) is lib.DimensionMismatch and str(err) == "quad_stages: ldq < n (stage 1)"      # (stages 1 and 3 read one matrix)
    assert seen == [(SYMBOLS[entry][0], 0)] and ctx.uploads == [] and ctx.calls == []
    # what is allocated by then are the record's own buffers: the outputs, the constant, the stages' constants
    nq, nl = T * n * (n + 1) // 2, T * n
    assert ctx.allocs == [(8 if entry == "csc" else 24) * nq, 16 * nl, 8, 8 * T]
