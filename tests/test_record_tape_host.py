"""CPU-only: what _Record.compile leaves on a record and what its emitter records, for one record of every function form, against a stub
context (no device: fake addresses, the real library only for the Gram workspace size); the lane / emit-order decision as a table; and
the declared state of Model, Parameter and records.

The expectations of part 1 are written out by hand from the entry points' argument lists (include/parametron_hip.h).  "Scalar arguments"
are the Python ints and floats of a call; pointers (ctypes objects, None, raw addresses >= 2^32) are left out — allocation order is free."""
import numpy as np
import pytest

import __graft_entry__ as entry
from test_stacked_lsq_host import FAKE, _dense, _dvars, _vec

VARMAP_BUF = 0x2000


@pytest.fixture(scope="module")
def lib():
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


class StubContext:
    """DeviceContext's surface as compile / the emitters / the fetches use it"""
    recording = False

    def __init__(self, lib):
        self.lib = lib.load()
        self.calls, self.allocs, self.fetched, self.recorded = [], [], [], []
        self.raw = []                                                       # (name, args) of every call, the arguments as they were passed
        self._next = 1 << 44

    def alloc(self, nbytes):
        self.allocs.append(int(nbytes))
        self._next += 1 << 24
        return self._next

    def pinned_array(self, n, dtype):
        return np.zeros(int(n), dtype=dtype)

    def upload(self, dptr, host):
        pass

    def upload_new(self, host):
        return self.alloc(max(np.ascontiguousarray(host).nbytes, 8))

    def zero(self, dptr, nbytes):
        pass

    def call(self, name, *args):
        self.raw.append((name, args))
        self.calls.append((name, tuple(a for a in args if isinstance(a, (int, float)) and not isinstance(a, bool) and abs(a) < 2 ** 32)))

    # a copy "lands" at once: every byte 0x40 (the double 32.5019...), so that the test sees where a constant was fetched to
    def fetch(self, host, dptr, nbytes):
        self.fetched.append((host.ctypes.data, dptr, int(nbytes)))
        host.view(np.uint8)[:] = 0x40

    def record_fetch(self, host, dptr, nbytes):
        self.recorded.append((host.ctypes.data, dptr, int(nbytes)))
        host.view(np.uint8)[:] = 0x40


LANDED = float(np.frombuffer(b"\x40" * 8, dtype=np.float64)[0])


# ---- device values without a device (as test_stacked_lsq_host builds them, plus the fields compile reads)
def _xvars(idx):
    x = _dvars(idx)
    x.buf = FAKE
    return x


def _block(rows, idx, vec=None, sign=0):
    d = _dense(rows, idx, vec, sign)
    d.xvars.buf = FAKE
    d.nterms, d.need_terms = rows * len(idx), False
    return d


def _b(n):
    v = _vec(n)
    v.padded = n
    return v


def _vars_aff(idx, vec, sign):
    from parametron_jl_amd.device import DVarsAff
    d = DVarsAff.__new__(DVarsAff)
    d.xvars, d.vec, d.sign, d.rows, d.nterms, d.need_terms = _xvars(idx), vec, sign, len(idx), len(idx), False
    return d


def _quad_out(nq=0, nl=0):
    from parametron_jl_amd.device import DQuad
    q = DQuad.__new__(DQuad)
    q.nq, q.nl, q.quad, q.lin, q.const, q.inputs = nq, nl, None, None, None, ()
    return q


def _form(n, idx):
    from parametron_jl_amd.device import DMat
    from parametron_jl_amd.lazyexpression import QuadForm
    m = DMat.__new__(DMat)
    m.rows, m.cols, m.lda, m.buf = n, n, n, FAKE
    return QuadForm(m, _xvars(idx))


def _model(**kw):
    from parametron_jl_amd.model import MockOptimizer, Model
    small = kw.pop("small", False)
    m = Model(MockOptimizer(), **kw)
    m._small = small
    return m


def _node(model, out):
    from parametron_jl_amd.lazyexpression import DeviceNode
    return DeviceNode(model, "test", [], out, None)


def _objective(model, out, plan=None):
    from parametron_jl_amd import moi
    r = moi.Objective(model, _node(model, out))
    if plan is not None:
        r.plan = plan
    return r


def _constraint(model, out):
    from parametron_jl_amd import moi
    return moi.Constraint(model, _node(model, out), moi.Zeros(out.rows))


def _run(lib, record, varmap=None):
    """compile + emit: (the stub context, the emitter)"""
    ctx = StubContext(lib)
    emit = record.compile(ctx, VARMAP_BUF, varmap)
    emit(ctx)
    return ctx, emit


def _ws(lib, rows, cols):
    return max(16, int(lib.load().pmt_quad_gram_workspace_bytes(rows, cols)))


def _table(record):
    """record.buffers as (address of the host array, dev key)"""
    return [(h.ctypes.data, k) for h, k in record.buffers]


def _scalar_table(r):
    return [(r.f.quadratic_terms.ctypes.data, "quad"), (r.f.affine_terms.ctypes.data, "lin"), (r._cbuf.ctypes.data, "const")]


def _vector_table(r):
    return [(r.f._terms.ctypes.data, "terms"), (r.f.constants.ctypes.data, "consts")]


def _copies(r):
    """what fetch() / record_fetch() must copy: the table's entries whose key is in dev and whose twin is not the host array itself"""
    return [(h.ctypes.data, r.dev[k], h.nbytes) for h, k in r.fetch_list() if k in r.dev and r.dev[k] != h.ctypes.data and h.nbytes]


def _dst(copies):
    return [(dptr, nbytes) for _, dptr, nbytes in copies]


# ---- part 1: one record of every form
def test_scalar_affine(lib):
    from parametron_jl_amd.device import DAff
    for small in (False, True):
        model = _model(small=small)
        out = DAff(StubContext(lib), 3)
        r = _objective(model, out)
        ctx, _ = _run(lib, r)
        assert ctx.calls == [("pmt_pack_scalar_affine_f64", (3,))] + ([("pmt_copy_bytes", (8,))] if small else [])
        assert set(r.dev) == {"terms", "const"} and not r.side_lane_ok
        assert ctx.allocs == ([] if small else [48])
        assert _table(r) == [(r.f.terms.ctypes.data, "terms"), (r._cbuf.ctypes.data, "const")]
        if small:                                              # zero-copy twins: nothing to fetch
            assert r.dev["terms"] == r.f.terms.ctypes.data and r.dev["const"] == r._cbuf.ctypes.data and _copies(r) == []
        else:
            assert r.dev["const"] == out.const
        r.fetch(ctx)
        assert ctx.fetched == _copies(r)
        r._cbuf[0] = 7.0 if small else r._cbuf[0]
        r.finish_fetch()
        assert r.f.constant == (7.0 if small else LANDED)


@pytest.mark.parametrize("overlap", [False, True])
def test_canonical_gram(lib, overlap):
    from parametron_jl_amd.moi import QuadPlan
    model = _model(quadratic_mode="canonical", overlap_fetch=overlap)
    g = _block(10, [1, 2, 3], _b(10), -1)
    r = _objective(model, _quad_out(), QuadPlan("canonical", gram=g))
    ctx, _ = _run(lib, r)
    if overlap:
        assert ctx.calls == [("pmt_quad_gram_deliver_f64", (10, 10, 3, -1, 1, 0))]
    else:
        assert ctx.calls == [("pmt_quad_gram_f64", (10, 10, 3, -1, 1))]
    assert set(r.dev) == {"quad", "lin", "const"} and not r.side_lane_ok
    assert sorted(ctx.allocs) == sorted([24 * 6, 16 * 3, 16, _ws(lib, 10, 3)])
    assert len(r.f.quadratic_terms) == 6 and len(r.f.affine_terms) == 3
    assert _table(r) == _scalar_table(r)
    # the overlapped boundary: recorded fetches, the quadratic terms delivered by the contraction itself; otherwise fetch() copies all three
    copies = _copies(r)
    if overlap:
        r.record_fetch(ctx)
        assert _dst(ctx.recorded) == _dst(c for c in copies if c[1] != r.dev["quad"])
        assert r._cbuf[0] == LANDED                                        # the constant always lands in _cbuf
        r.fetch(ctx)
        assert ctx.fetched == []
    else:
        r.fetch(ctx)
        assert ctx.fetched == copies and len(ctx.fetched) == 3
    r.finish_fetch()
    assert r.f.constant == LANDED


def test_canonical_csc(lib):
    from parametron_jl_amd.moi import QuadPlan
    model = _model(quadratic_mode="canonical", handoff="device")
    g = _block(10, [1, 2, 3], _b(10), -1)
    r = _objective(model, _quad_out(), QuadPlan("canonical-csc", gram=g))
    ctx, _ = _run(lib, r, np.array([2, 5, 7], dtype=np.int64))             # order-preserving early map
    assert ctx.calls == [("pmt_quad_gram_csc_f64", (10, 10, 3, -1, 1.0))]
    assert set(r.dev) == {"P_values", "P_vars", "lin", "const"} and list(r.dev["P_vars"]) == [2, 5, 7] and not r.side_lane_ok
    assert sorted(ctx.allocs) == sorted([8 * 6, 16 * 3, 8, _ws(lib, 10, 3)])
    assert len(r.f.quadratic_terms) == 0 and len(r.f.affine_terms) == 3
    assert _table(r) == _scalar_table(r)
    r.fetch(ctx)                                                           # "quad" is absent from dev: skipped
    assert ctx.fetched == _copies(r) and [c[1] for c in ctx.fetched] == [r.dev["lin"], r.dev["const"]]


def test_canonical_csc_delivered_to_the_host(lib):
    from parametron_jl_amd.moi import QuadPlan
    model = _model(quadratic_mode="canonical", handoff="host_csc")
    g = _block(10, [1, 2, 3])
    r = _objective(model, _quad_out(), QuadPlan("canonical-csc", gram=g))
    ctx, _ = _run(lib, r, np.array([1, 2, 3], dtype=np.int64))
    assert ctx.calls == [("pmt_quad_gram_csc_deliver_f64", (10, 10, 3, 0, 1.0, 0))]
    assert set(r.dev) == {"P_values", "P_vars", "P_host", "lin", "const"} and r.dev["P_host"].shape == (6,)
    assert sorted(ctx.allocs) == sorted([8 * 6, 16 * 3, 8, _ws(lib, 10, 3)])


def test_canonical_form_both_handoffs(lib):
    from parametron_jl_amd.moi import QuadPlan
    form = _form(3, [1, 2, 3])
    model = _model(quadratic_mode="canonical")
    r = _objective(model, _quad_out(9, 0), QuadPlan("canonical-form", form=form))
    ctx, _ = _run(lib, r)
    assert ctx.calls == [("pmt_quad_form_f64", (3, 3, 1, 1.0))]
    assert set(r.dev) == {"quad", "const"} and sorted(ctx.allocs) == [8, 24 * 6] and not r.side_lane_ok
    assert len(r.f.quadratic_terms) == 6 and len(r.f.affine_terms) == 0
    assert _table(r) == _scalar_table(r)
    copies = _copies(r)
    r.record_fetch(ctx)                                                    # "lin" is absent: no linear terms
    assert _dst(ctx.recorded) == _dst(copies) and [c[1] for c in ctx.recorded] == [r.dev["quad"], r.dev["const"]]
    assert r._cbuf[0] == LANDED                                            # the constant always lands in _cbuf
    r.finish_fetch()
    assert r.f.constant == LANDED

    model = _model(quadratic_mode="canonical", handoff="device")
    model.sense = "Maximize"
    r = _objective(model, _quad_out(9, 0), QuadPlan("canonical-form", form=form))
    ctx, _ = _run(lib, r, np.array([3, 4, 9], dtype=np.int64))
    assert ctx.calls == [("pmt_quad_form_f64", (3, 3, 1, -1.0))]
    assert set(r.dev) == {"P_values", "P_vars", "lin", "const"} and list(r.dev["P_vars"]) == [3, 4, 9]
    assert sorted(ctx.allocs) == [8, 8 * 6, 16 * 3]
    assert _table(r) == _scalar_table(r)


def test_canonical_sum_with_a_diagonal_over_part_of_x(lib):
    from parametron_jl_amd.lazyexpression import LsqTerm, _IndexVars
    from parametron_jl_amd.moi import QuadPlan
    b1, b2 = _block(10, [1, 2, 3], _b(10), -1), _block(7, [1, 2, 3])
    terms = [LsqTerm("block", r=b1), LsqTerm("block", scale=2.0, r=b2), LsqTerm("diag", scale=0.5, xvars=_IndexVars([2, 3]))]
    model = _model(quadratic_mode="canonical")
    r = _objective(model, _quad_out(), QuadPlan("canonical-sum", terms=terms))
    ctx, _ = _run(lib, r)
    assert ctx.calls == [("pmt_quad_gram_f64", (10, 10, 3, -1, 1)),
                         ("pmt_quad_gram_csc_f64", (7, 7, 3, 0, 1.0)),
                         ("pmt_quad_gram_sum_sub_f64", (3, 3))]
    assert set(r.dev) == {"quad", "lin", "const"} and not r.side_lane_ok
    assert sorted(ctx.allocs) == sorted([24 * 6, 16 * 3, 8, _ws(lib, 10, 3), _ws(lib, 7, 3), 8 * 6, 16 * 3, 8])
    assert _table(r) == _scalar_table(r)
    (lists, ptrs, counts), = r._sub_args                                   # kept alive for the recorded call
    assert [None if p is None else list(p) for p in lists] == [None, None, [1, 2]] and list(counts) == [0, 0, 2]
    # the terms are final only after the combine: never delivered by the contraction
    copies = _copies(r)
    r.record_fetch(ctx)
    assert _dst(ctx.recorded) == _dst(copies) and len(ctx.recorded) == 3
    assert r._cbuf[0] == LANDED                                            # the constant always lands in _cbuf


@pytest.mark.parametrize("sets, ordered", [(([1, 2, 3], [4, 5]), True), (([1, 3, 5], [2, 4]), False)])
def test_canonical_groups(lib, sets, ordered):
    from parametron_jl_amd.lazyexpression import LsqTerm
    from parametron_jl_amd.moi import QuadGroup, QuadPlan
    groups = [QuadGroup([LsqTerm("block", r=_block(10, s))], np.asarray(s, dtype=np.int64)) for s in sets]
    model = _model(quadratic_mode="canonical")
    r = _objective(model, _quad_out(), QuadPlan("canonical-groups", groups=groups))
    ctx, _ = _run(lib, r)
    per_group = [("pmt_quad_gram_f64", (10, 10, 3, 0, 1)), ("pmt_quad_gram_sum_f64", (3, 1)),
                 ("pmt_quad_gram_f64", (10, 10, 2, 0, 1)), ("pmt_quad_gram_sum_f64", (2, 1))]
    gather = [] if ordered else [("pmt_quad_groups_gather_f64", (5, 9, 5))]
    assert ctx.calls == per_group + gather + [("pmt_quad_groups_constant_f64", (2,))]
    assert r.groups_ordered is ordered and r.plan.gram_record
    assert set(r.dev) == {"quad", "lin", "const"} and not r.side_lane_ok
    arena = [] if ordered else [24 * 9, 16 * 5, 8 * 5, 8 * 6, 8 * 5]
    assert sorted(ctx.allocs) == sorted([24 * 9, 16 * 5, 8, 8 * 2, _ws(lib, 10, 3), _ws(lib, 10, 2)] + arena)
    assert len(r.f.quadratic_terms) == 9 and len(r.f.affine_terms) == 5
    assert _table(r) == _scalar_table(r)


def test_literal_quadratic(lib):
    from parametron_jl_amd.device import DQuad
    from parametron_jl_amd.moi import QuadPlan
    for small in (False, True):
        model = _model(small=small)
        out = DQuad(StubContext(lib), 4, 2)
        r = _objective(model, out, QuadPlan("literal"))
        ctx, _ = _run(lib, r)
        assert ctx.calls == [("pmt_pack_scalar_quadratic_f64", (4,)), ("pmt_pack_scalar_affine_f64", (2,))] + \
            ([("pmt_copy_bytes", (8,))] if small else [])
        assert set(r.dev) == {"quad", "lin", "const"} and not r.side_lane_ok
        assert sorted(ctx.allocs) == ([] if small else [16 * 2, 24 * 4])
        assert _table(r) == _scalar_table(r)
        assert r.dev["const"] == (r._cbuf.ctypes.data if small else out.const)
        r.fetch(ctx)
        assert ctx.fetched == _copies(r) and len(ctx.fetched) == (0 if small else 3)


@pytest.mark.parametrize("side", [False, True])
def test_dense_vector_block(lib, side):
    model = _model()
    r = _constraint(model, _block(4, [1, 2, 3], _b(4), 1))
    ctx = StubContext(lib)
    emit = r.compile(ctx, VARMAP_BUF, None)
    assert r.side_lane_ok and r.on_side_lane is False
    r.on_side_lane = side                                                  # Model.initialize decides between compile and the emit
    emit(ctx)
    assert ctx.calls == [("pmt_affine_pack_vector_background_f64" if side else "pmt_affine_pack_vector_f64", (4, 4, 3, 1, 0))]
    assert set(r.dev) == {"terms", "consts"} and sorted(ctx.allocs) == [8 * 4, 24 * 12]
    assert _table(r) == _vector_table(r)
    r.fetch(ctx)
    assert ctx.fetched == _copies(r) and len(ctx.fetched) == 2


def test_variables_plus_vector(lib):
    model = _model()
    r = _constraint(model, _vars_aff([1, 2, 3], _b(3), -1))
    ctx, _ = _run(lib, r)
    assert ctx.calls == [("pmt_vars_addsub_f64", (3, -1, 0))]
    assert set(r.dev) == {"terms", "consts"} and r.side_lane_ok and sorted(ctx.allocs) == [8 * 3, 24 * 3]
    assert _table(r) == _vector_table(r)


def test_host_csc_static_structure(lib):
    model = _model(handoff="host_csc")
    r = _constraint(model, _block(4, [1, 2, 3], _b(4), -1))
    ctx, _ = _run(lib, r, np.array([2, 5, 7], dtype=np.int64))
    assert ctx.calls == [("pmt_consts_f64", (4, -1))]
    assert set(r.dev) == {"consts"} and r.side_lane_ok and r.terms_static and ctx.allocs == [8 * 4]
    rows, variables = r.f.structure
    assert list(rows) == [1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4] and list(variables) == [2, 5, 7] * 4
    with pytest.raises(lib.ErrorException):
        r.f.terms
    assert _table(r) == _vector_table(r)
    r.fetch(ctx)                                                           # "terms" is absent from dev: only the constants travel
    assert ctx.fetched == [(r.f.constants.ctypes.data, r.dev["consts"], 32)]
    # a dense block without b records nothing at all
    r = _constraint(model, _block(4, [1, 2, 3]))
    ctx, _ = _run(lib, r, np.array([2, 5, 7], dtype=np.int64))
    assert ctx.calls == [] and set(r.dev) == {"consts"}


# ---- part 2: the lane / emit-order decision
G, C_OK, C_NO = (True, False), (False, True), (False, False)               # (plan.gram_record, side-lane eligible)


@pytest.mark.parametrize("records, small, side_lane, handoff, overlap_moi, order, lane", [
    ([C_NO, C_OK, C_OK], False, True, "moi", True, [0, 1, 2], set()),            # no Gram record: nothing moves
    ([G, C_OK], False, True, "moi", False, [0, 1], set()),                       # one small kernel on the lane does not pay ...
    ([G, C_OK], False, True, "moi", True, [1, 0], {1}),                          # ... unless its terms cross PCIe during the contraction
    ([G, C_OK, C_NO, C_OK], False, True, "moi", False, [1, 3, 0, 2], {1, 3}),    # two eligible: in front of the objective
    ([G, C_OK, C_OK], True, True, "moi", False, [1, 2, 0], set()),               # small: the Gram record last, no lane
    ([C_OK, G, C_OK], True, True, "moi", False, [0, 2, 1], set()),
    ([G, C_OK, C_OK], False, False, "moi", True, [0, 1, 2], set()),              # side_lane=False
    ([G, C_OK], False, True, "device", False, [1, 0], {1}),                      # a hand-off's launches join the one record on the lane
    ([G, C_OK], False, True, "host_csc", False, [1, 0], {1}),
    ([G, C_NO], False, True, "device", False, [0, 1], set()),
])
def test_lane_order(records, small, side_lane, handoff, overlap_moi, order, lane):
    from parametron_jl_amd.model import lane_order
    assert lane_order(records, small, side_lane, handoff, overlap_moi) == (order, lane)


# ---- part 3: the state is declared
def test_state_is_declared_with_its_defaults(lib):
    from parametron_jl_amd.parameter import DeviceUniformParameter, Parameter
    model = _model()
    assert model._small is False and model._lane_records == [] and model._tape_parameters is None and model._model_run is None
    assert model._run_slot == [] and model._fetches_read_parameters is False and model._varmap_buf is None and model._order == []
    assert model._records == [] and model._overlap_moi is True
    model.close()                                                          # never initialised: nothing to release
    p = Parameter(lambda: 1.0, model)
    d = DeviceUniformParameter((3,), 1, model)
    for x in (p, d):
        assert x._staged_pending is False and x._commit_on_side_lane is False and x._in_tape is False
        assert x._mailbox is None and x._mailbox_write is None and x._seed_word is None and x._run_val is None
        assert x._read_unordered_by_lane3 is False and x.pattern is None
    assert p.device_resident is False and d.device_resident is True
    assert Parameter.device_resident is False and Parameter.pattern is None
    r = _objective(model, _quad_out())
    assert r.varmap_hooks == [] and r.side_lane_ok is False and r.on_side_lane is False and r.terms_static is False
    assert r.groups_ordered is None and r._sub_args == [] and r._fetch_recorded is False and r._cbuf is None and r.buffers == []
    assert not hasattr(r, "_c")
    r.fetch(StubContext(lib))                                              # a record that was never compiled fetches nothing


def test_close_is_safe_on_a_model_whose_arguments_were_refused(lib):
    from parametron_jl_amd.model import MockOptimizer, Model
    for bad in ({"quadratic_mode": "other"}, {"handoff": "other"}, {"handoff": "host_csc", "use_graph": True}):
        model = Model.__new__(Model)
        with pytest.raises(lib.ArgumentError):
            model.__init__(MockOptimizer(), **bad)
        model.close()
        assert model._ctx is None and model._model_run is None and model._records == []


def test_device_values_declare_their_staging_state(lib):
    import scipy.sparse as sp
    from parametron_jl_amd.device import DMat, DNum, DSpMat, DVec
    ctx = StubContext(lib)
    pattern = sp.csc_matrix(np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]]))
    for dv in (DNum(ctx), DVec(ctx, 3), DSpMat(ctx, pattern)):
        assert dv._staging_slots == {} and dv._staged_bytes == 0 and dv._staged_slot == 0
    m = DMat(ctx, 3, 2)
    assert m._stage is None and m._stage_rm == {} and m._staging_cm == {} and m._staged_kind is None and m._staged_slot == 0


def test_a_second_compile_starts_from_the_declared_state(lib):
    from parametron_jl_amd.moi import QuadPlan
    model = _model(quadratic_mode="canonical")
    r = _objective(model, _quad_out(), QuadPlan("canonical", gram=_block(10, [1, 2, 3])))
    ctx, _ = _run(lib, r)
    r.record_fetch(ctx)
    r.on_side_lane = True
    assert r.delivered == ("quad",) and r._fetch_recorded
    model._overlap_moi = False
    ctx, _ = _run(lib, r)
    assert r.delivered == () and r._fetch_recorded is False and r.on_side_lane is False and r.varmap_hooks == []
    assert ctx.calls == [("pmt_quad_gram_f64", (10, 10, 3, 0, 1))] and _table(r) == _scalar_table(r)
