"""MathOptInterface hand-off (src/moi_interop.jl): function/set records, Objective / Constraint / Constraints and the
native -> MOI copies `update!(moi_f, f, varmap)` (:35-81).

MOI function buffers are numpy structured arrays with exactly the Julia isbits layouts, so a
Julia host can pass `pointer(moi_f.terms)` as the destination of pmt_plan_fetch.  For non-constant records the copy
itself runs on the device (the pack kernels write MOI terms, through `varmap`, into device twins of these buffers);
constant records are converted once on the host at setup, as in the reference (`isconstant`, :123,132,153,169).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import LT, QT, VAT, ArgumentError, DimensionMismatch, ErrorException
from .device import DAff, DAffVec, DDenseAff, DQuad, DSparseAff, DStackedAff, DVarsAff, P
from .functions import AffineFunction, LinearTerm, QuadraticFunction, QuadraticTerm, Variable, _isnum
from .lazyexpression import DeviceNode, QuadForm, SparseQuadForm, affine_stage_leaves, kind_of

MIN_SENSE, MAX_SENSE = "MIN_SENSE", "MAX_SENSE"


# ---- sets (MOI.AbstractSet)
class _Set:
    def __init__(self, value=None):
        self.value = value

    def __repr__(self):
        return "%s(%r)" % (type(self).__name__, self.value)

    def __eq__(self, o):
        return type(o) is type(self) and o.value == self.value

    def __hash__(self):
        return hash((type(self).__name__, self.value))


class GreaterThan(_Set): pass
class LessThan(_Set): pass
class EqualTo(_Set): pass
class Nonnegatives(_Set): pass
class Nonpositives(_Set): pass
class Zeros(_Set): pass
class Integer(_Set): pass
class ZeroOne(_Set): pass


# ---- functions (MOI.AbstractFunction)
def _zeros(n, dtype):
    return np.zeros(n, dtype=dtype)


# `alloc(n, dtype)` lets the device path place the term buffers in page-locked host memory (DeviceContext.pinned_array)
class ScalarAffineFunction:
    def __init__(self, nterms=0, alloc=_zeros):
        self.terms = alloc(nterms, LT)
        self.constant = 0.0


class ScalarQuadraticFunction:
    def __init__(self, naff=0, nquad=0, alloc=_zeros):
        self.affine_terms = alloc(naff, LT)
        self.quadratic_terms = alloc(nquad, QT)
        self.constant = 0.0


class VectorAffineFunction:
    def __init__(self, nterms=0, nrows=0, alloc=_zeros):
        self._terms = alloc(nterms, VAT)
        self.constants = alloc(nrows, np.float64)
        self.coefficients_unavailable = None      # a reason: the coefficients are NOT on the host (handoff="host_csc", dense block)

    @property
    def terms(self):
        """MOI.VectorAffineTerm[] (src/moi_interop.jl:64-81).  With handoff="host_csc" the terms of a dense block A*x (+|-) b are never packed —
        the solver's A is delivered as CSC values straight out of the Parameter's buffer — and only their STRUCTURE (`structure`) is host
        data: reading the coefficients is an error, not a NaN."""
        if self.coefficients_unavailable:
            raise ErrorException(self.coefficients_unavailable)
        return self._terms

    @terms.setter
    def terms(self, value):
        self._terms = value

    @property
    def structure(self):
        """(output rows, optimizer variables) of the terms — always host data"""
        return self._terms["out"], self._terms["var"]


class SingleVariable:
    def __init__(self, variable):
        self.variable = variable


# ---- host restatement of update!(moi_f, f, varmap) for CONSTANT records (setup time)
def _vm(varmap, idx):
    return idx if varmap is None else int(varmap[idx - 1])


def update_scalar_affine(moi_f, f, varmap=None):                      # src/moi_interop.jl:35-43
    moi_f.constant = float(f.constant)
    moi_f.terms = np.zeros(len(f.linear), dtype=LT)
    for i, t in enumerate(f.linear):
        moi_f.terms[i] = (t.coeff, _vm(varmap, t.var.index))
    return moi_f


def update_scalar_quadratic(moi_f, f, varmap=None):                   # src/moi_interop.jl:45-62
    update_scalar_affine_part = ScalarAffineFunction()
    update_scalar_affine(update_scalar_affine_part, f.affine, varmap)
    moi_f.constant = update_scalar_affine_part.constant
    moi_f.affine_terms = update_scalar_affine_part.terms
    moi_f.quadratic_terms = np.zeros(len(f.quadratic), dtype=QT)
    for i, t in enumerate(f.quadratic):
        coeff = 2 * t.coeff if t.rowvar == t.colvar else t.coeff        # :58
        moi_f.quadratic_terms[i] = (coeff, _vm(varmap, t.rowvar.index), _vm(varmap, t.colvar.index))
    return moi_f


def update_vector_affine(moi_f, fs, varmap=None):                     # src/moi_interop.jl:64-81
    n = sum(len(f.linear) for f in fs)
    moi_f.constants = np.zeros(len(fs), dtype=np.float64)
    moi_f.terms = np.zeros(n, dtype=VAT)
    i = 0
    for row, f in enumerate(fs):
        for t in f.linear:
            moi_f.terms[i] = (row + 1, t.coeff, _vm(varmap, t.var.index))
            i += 1
        moi_f.constants[row] = f.constant
    return moi_f


def canonical_function_kind(kind):                                     # src/moi_interop.jl:96-101
    if kind in ("var", "lt", "aff", "num"):
        return "aff"
    if kind in ("varvec", "affvec"):
        return "affvec"
    if kind in ("qt", "quad"):
        return "quad"
    raise ArgumentError("no canonical function type for %s" % kind)


def _to_native(kind, val):
    if kind == "aff":
        return AffineFunction.of(float(val) if _isnum(val) else val)
    if kind == "quad":
        return QuadraticFunction.of(val)
    return [AffineFunction.of(float(v) if _isnum(v) else v) for v in val]


def _gram_rows(gram):
    """Row count handed to the Gram kernel: the zero-padded count (device.row_padded) when both the matrix and the vector carry the
    zero padding rows — whole 16-row stages keep the contraction on its branch-free path; zero rows change nothing."""
    from .device import DMat, DVec, row_padded
    rows = gram.mat.rows
    padded = row_padded(rows)
    if padded == rows or not isinstance(gram.mat, DMat) or gram.mat.lda < padded:
        return rows
    if gram.vec is not None and not (isinstance(gram.vec, DVec) and getattr(gram.vec, "padded", 0) >= padded):
        return rows
    return padded


def _buf(x):                                                              # the address of a device value, None for none
    return x.buf if x is not None else None


def _vec_sign(vec, sign):                                                 # (address, sign) of the vector in (+|-) vec; none: (None, 0)
    b = _buf(vec)
    return b, sign if b else 0


def _table(ctx, arr):                                                     # a ctypes table in a device buffer of its own; the context keeps a
    # view of `arr` (no copy) for the upload: it is not to be written afterwards
    return ctx.upload_new(np.frombuffer(arr, dtype=np.uint8))


def _gram_args(g):
    """the leading arguments of the Gram family: r = mat*x (+|-) vec"""
    vec, sign = _vec_sign(g.vec, g.sign)
    return (P(g.mat.buf), g.mat.lda, _gram_rows(g), g.mat.cols, P(g.xvars.buf), P(vec), sign)


def _gram_workspace(ctx, g):
    return ctx.alloc(max(16, int(ctx.lib.pmt_quad_gram_workspace_bytes(_gram_rows(g), g.mat.cols))))


def _form_args(q, varmap_buf, alpha):                                    # the leading arguments of pmt_quad_form_f64 / _shift_f64
    if q.vec is not None:
        return (P(q.mat.buf), q.mat.lda, q.mat.cols, P(q.xvars.buf), P(q.vec.buf), q.sign, 1, P(varmap_buf), alpha)
    return (P(q.mat.buf), q.mat.lda, q.mat.cols, P(q.xvars.buf), 1, P(varmap_buf), alpha)


def _form_call(c, q, varmap_buf, alpha, outs, ws):
    """the form node's call: pmt_quad_form_f64, or pmt_quad_form_shift_f64 with its workspace `ws` for a shifted form (q.vec)"""
    if q.vec is not None:
        c.call("pmt_quad_form_shift_f64", *_form_args(q, varmap_buf, alpha), *outs, P(ws))
    else:
        c.call("pmt_quad_form_f64", *_form_args(q, varmap_buf, alpha), *outs)


def _form_workspace(ctx, q):
    """the partial sums of a shifted form's linear part (allocated at compile: update! allocates nothing); a plain form has none"""
    return ctx.alloc(max(16, int(ctx.lib.pmt_quad_form_shift_workspace_bytes(q.mat.cols)))) if q.vec is not None else None


def _sparse_gram_call(c, r, T, varmap_buf, dq, dl, dc):                    # the sparse Gram node's call (moi = 1); T: r.gram_tables()
    vec, sign = _vec_sign(r.vec, r.sign)
    c.call("pmt_sparse_gram_f64", P(r.spmat.buf), *T.call_args(r.rows), P(r.xvars.buf), P(vec), sign, 1, P(varmap_buf), P(dq), P(dl), P(dc))


def _sparse_form_call(c, q, T, varmap_buf, dq, dc):                        # the sparse form node's call (moi = 1); T: q.form_tables()
    c.call("pmt_sparse_form_f64", P(q.spmat.buf), *T.call_args(), P(q.xvars.buf), 1, P(varmap_buf), P(dq), P(dc))


def _static_indices(f, T, xvars, handoff_varmap):
    """The index fields of a sparse record's terms (T.pair_j, pair_k, lin_col: their columns of x) are static: written into f's host arrays
    at compile, through the hand-off's map, where its generic route finds them before the first update; the kernels rewrite them."""
    x = xvars.vars if handoff_varmap is None else np.asarray(handoff_varmap, dtype=np.int64)[xvars.vars - 1]
    f.quadratic_terms["row"], f.quadratic_terms["col"], f.quadratic_terms["coeff"] = x[T.pair_j], x[T.pair_k], 0.0
    f.affine_terms["var"], f.affine_terms["coeff"] = x[T.lin_col], 0.0


def _part_of(v, x):
    """The subset rule of the weighted sums, for the variables `v` of a diagonal / linear term and the record's strictly increasing `x`,
    read by the decision (_lsq_sum_combines, _sparse_sum_combines) and the execution (_term_positions) alike: None when v is x itself,
    the int64 positions of v in x when v is a non-empty strictly increasing part of x, False when it is neither (the sum is refused)."""
    if np.array_equal(v, x):
        return None
    pos = np.searchsorted(x, v).astype(np.int64)
    if len(v) and np.all(np.diff(v) > 0) and np.all(pos < len(x)) and np.array_equal(x[np.minimum(pos, len(x) - 1)], v):
        return pos
    return False


def _term_positions(terms, x):                                            # _part_of per term; None also for a term without variables
    lists = [_part_of(t.xvars.vars, x) if t.kind in ("diag", "linear") else None for t in terms]
    if any(p is False for p in lists):                                    # (the plan's predicate refuses such a list: quad_plan)
        raise ArgumentError("a term of the sum lies over variables that are no strictly increasing part of x")
    return lists


def _lsq_desc(t):
    """What the descriptors of the dense and the sparse combine (pmt_lsq_term, pmt_sparse_lsq_term) share for the LsqTerm t: kind (a form
    stands where a block stands), scale, weight, a diagonal term's vector and sign, a linear term's vector, a constant's value."""
    kind = {"block": _lib.PMT_LSQ_BLOCK, "form": _lib.PMT_LSQ_BLOCK, "diag": _lib.PMT_LSQ_DIAG, "linear": _lib.PMT_LSQ_LINEAR,
            "constant": _lib.PMT_LSQ_CONSTANT}
    d = {"kind": kind[t.kind], "scale": t.scale, "weight": _buf(t.param)}
    if t.kind in ("diag", "linear"):
        d["vec"], sign = _vec_sign(t.vec, t.sign)
        d["sign"] = sign if t.kind == "diag" else 0
    elif t.kind == "constant":
        d["vec"] = _buf(t.value)
    return d


class _Record:
    """Common part of Objective and Constraint (src/moi_interop.jl:113-129, 141-166)."""
    mode = property(lambda self: self.plan.mode)                          # "literal" / "canonical" / "canonical-csc" / "-form" / "-sum" / "-groups" / "-stages" / "-stages-csc" / "-sparse" / "-sparse-form" / "-sparse-sum"
    lsq_terms = property(lambda self: self.plan.terms)                    # the LsqTerm list a "canonical-sum" record combines, or None

    def _setup(self, model, expr):
        self.model = model
        self.expr = expr
        self.isconstant = not isinstance(expr, DeviceNode)                # "it's just a value; not a LazyExpression" (:123)
        self.plan = QuadPlan(None)                                        # a quadratic record's is decided in Model._plan_quadratic_records (quad_plan)
        self.stage_group = None                                           # Model.initialize: the AffineStageGroup whose one launch writes this record (affine_stage_group)
        self._reset_compiled()
        if self.isconstant:
            self.kind = canonical_function_kind(kind_of(expr))
            native = _to_native(self.kind, expr)
            if self.kind == "aff":
                self.f = update_scalar_affine(ScalarAffineFunction(), native)
            elif self.kind == "quad":
                self.f = update_scalar_quadratic(ScalarQuadraticFunction(), native)
            else:
                self.f = update_vector_affine(VectorAffineFunction(), native)
            self.nrows = len(native) if self.kind == "affvec" else 1
        else:
            self.kind = canonical_function_kind(expr.out.kind)
            self.f = None                                                 # sized by compile()
            self.nrows = expr.out.rows if self.kind == "affvec" else 1

    def _reset_compiled(self):
        """what compile() leaves for the model that runs the record: declared here, and fresh at every compile"""
        self.dev = None                                                   # compile: device twins of the MOI buffers, by key
        self.buffers = []                                                 # compile: (host array, key of dev) in fetch order, the constant's word included
        self.delivered = ()                                               # _compile_gram: keys of dev the producing kernel itself delivers to the host
        self._cbuf = None                                                 # compile: the page-locked word the scalar functions' constant lands in
        self.varmap_hooks = []                                            # _compile_sparse: called with the new host varmap whenever it changes
        self.side_lane_ok = False                                         # _implicit_twins, _compile_static: reads Parameter values only, writes its own buffers
        self.on_side_lane = False                                         # Model._record_tape, before the emitter runs
        self.terms_static = False                                         # _compile_static: the terms are host data, only the constants are rebuilt
        self.groups_ordered = None                                        # _compile_layout: every group / stage is one slice of the destination
        self._sub_args = []                                               # _lsq_sum_emitter: host arrays a recorded combine reads
        self._fetch_recorded = False                                      # record_fetch: the copies are entries of the tape

    # ---- device side of update!(moi_f, expr(), varmap)
    def compile(self, ctx, varmap_buf, handoff_varmap=None):
        """Allocate the MOI buffers (host + device twin) and return the emitter of the MOI copy: one method per function form, each
        sets self.f and self.dev.  `handoff_varmap` (host array, device hand-off only): the final model_var_to_optimizer; a Gram objective
        whose variables stay in increasing order under it writes the solver's CSC values of P directly from the contraction's epilogue and
        no quadratic term structs at all."""
        self._reset_compiled()
        self._cbuf = ctx.pinned_array(1, np.float64)
        if self.stage_group is not None:
            emit = self.stage_group.compile_member(self, ctx, varmap_buf)
            self.buffers = [(self.f._terms, "terms"), (self.f.constants, "consts")]
            return emit
        if self.kind == "aff":
            emit = self._compile_affine(ctx, varmap_buf, handoff_varmap)
            self.buffers = [(self.f.terms, "terms"), (self._cbuf, "const")]
        elif self.kind == "quad":
            emit = self._QUAD_FORMS[self.plan.mode](self, ctx, varmap_buf, handoff_varmap)
            self.buffers = [(self.f.quadratic_terms, "quad"), (self.f.affine_terms, "lin"), (self._cbuf, "const")]
        else:
            emit = self._compile_vector(ctx, varmap_buf, handoff_varmap)
            self.buffers = [(self.f._terms, "terms"), (self.f.constants, "consts")]
        return emit

    def _twin(self, ctx, host, nbytes):
        """The device twin of a host MOI buffer.  A SMALL model (Model._decide_small: launch-bound on the device) has none: the kernels store
        straight into the page-locked host arrays of the function object (a few KB over PCIe from inside the one launch), and update! ends with
        ONE stream synchronisation instead of a D2H copy per buffer (~10 us each: five of them were half of solve! at n = 100)"""
        if self.model._small and nbytes > 0 and host.nbytes >= nbytes:
            return host.ctypes.data
        return ctx.alloc(max(nbytes, 16))

    def _const_twin(self, out):
        """a small model: the constant (a word the expression's node left in HBM) is copied into its page-locked word by one more entry of
        the tape — a node of the one launch — instead of a D2H copy behind every replay (a hipMemcpyAsync of 8 bytes is ~5 us of host time)"""
        return self._cbuf.ctypes.data if self.model._small else out.const

    def _quad_buffers(self, ctx, nl, nq, twin, lin=True, floor=0):
        """self.f: the ScalarQuadraticFunction of nl linear and nq quadratic terms; self.dev: its device buffers {"quad", "lin", "const"},
        returned as (dq, dl, dc).  `twin`: they are _twin's — the record's kernels can write a small model's page-locked host arrays —,
        otherwise plain device buffers (the forms and combines of models beyond the small plan).  `lin` False: no linear terms, neither
        buffer nor key.  `floor` 1: room for one term at least, as canonical-sum has always asked (quad_plan does not keep its x from being
        empty); forms, groups and stages ask for exactly their terms, as before — pmt_plan_alloc hands out no empty buffer either way."""
        self.f = f = ScalarQuadraticFunction(nl, nq, alloc=ctx.pinned_array)
        if twin:
            dq, dl, dc = self._twin(ctx, f.quadratic_terms, 24 * nq), self._twin(ctx, f.affine_terms, 16 * nl), self._twin(ctx, self._cbuf, 8)
        else:
            dq = ctx.alloc(24 * max(nq, floor))
            dl = ctx.alloc(16 * max(nl, floor)) if lin else None
            dc = ctx.alloc(8)
        self.dev = {"quad": dq, "lin": dl, "const": dc} if lin else {"quad": dq, "const": dc}
        return dq, dl, dc

    def _csc_buffers(self, ctx, xvars, handoff_varmap, floor=0):
        """A record over x = `xvars` whose hand-off takes the CSC values of P (x keeps its order under its index map): self.f without
        quadratic terms, self.dev with "P_values" / "P_vars" / "lin" / "const"; returns (dp, dl, dc, alpha), alpha -1.0 for Maximize;
        `floor`: as in _quad_buffers (1: the Gram node's)."""
        n = len(xvars.vars)
        self.f = ScalarQuadraticFunction(n, 0, alloc=ctx.pinned_array)
        dp, dl, dc = ctx.alloc(8 * max(n * (n + 1) // 2, floor)), ctx.alloc(16 * max(n, floor)), ctx.alloc(8)
        self.dev = {"P_values": dp, "P_vars": handoff_varmap[xvars.vars - 1], "lin": dl, "const": dc}
        return dp, dl, dc, -1.0 if self.model.sense == "Maximize" else 1.0

    def _compile_affine(self, ctx, varmap_buf, handoff_varmap):
        out, zero_copy = self.expr.out, self.model._small
        n = out.nterms
        self.f = ScalarAffineFunction(n, alloc=ctx.pinned_array)
        dev_terms, dconst = self._twin(ctx, self.f.terms, 16 * n), self._const_twin(out)
        self.dev = {"terms": dev_terms, "const": dconst}

        def emit(c):
            c.call("pmt_pack_scalar_affine_f64", P(out.terms), n, P(varmap_buf), P(dev_terms))
            if zero_copy:
                c.call("pmt_copy_bytes", P(dconst), P(out.const), 8)
        return emit

    def _compile_literal(self, ctx, varmap_buf, handoff_varmap):
        out, zero_copy = self.expr.out, self.model._small
        out.materialize()
        self.f = ScalarQuadraticFunction(out.nl, out.nq, alloc=ctx.pinned_array)
        dq, dl = self._twin(ctx, self.f.quadratic_terms, 24 * out.nq), self._twin(ctx, self.f.affine_terms, 16 * out.nl)
        dconst = self._const_twin(out)                                    # (the word the expression's node writes: no buffer of the record's)
        self.dev = {"quad": dq, "lin": dl, "const": dconst}

        def emit(c):
            c.call("pmt_pack_scalar_quadratic_f64", P(out.quad), out.nq, P(varmap_buf), P(dq))
            c.call("pmt_pack_scalar_affine_f64", P(out.lin), out.nl, P(varmap_buf), P(dl))
            if zero_copy:
                c.call("pmt_copy_bytes", P(dconst), P(out.const), 8)
        return emit

    def _compile_gram(self, ctx, varmap_buf, handoff_varmap):
        """dot(r, r), r = A*x (+|-) b (plan.gram): MOI terms ("canonical"), or the CSC values of P for a hand-off under whose index map x
        keeps its order ("canonical-csc")"""
        gram = self.plan.gram
        n = gram.mat.cols
        nq = n * (n + 1) // 2
        ws = _gram_workspace(ctx, gram)
        if self.plan.mode == "canonical-csc":
            dp, dl, dc, alpha = self._csc_buffers(ctx, gram.xvars, handoff_varmap, floor=1)
            if not (self.model.handoff == "host_csc" and self.model._overlap_fetch):
                return lambda c: c.call("pmt_quad_gram_csc_f64", *_gram_args(gram), P(varmap_buf), alpha, P(dp), None, P(dl), P(dc), P(ws))
            # host solver hand-off: the contraction finishes P column band by column band and every finished group of bands leaves
            # for this page-locked array while the rest is still being computed (pmt_quad_gram_csc_deliver_f64)
            host_P = self.dev["P_host"] = ctx.pinned_array(max(nq, 1), np.float64)
            return lambda c: c.call("pmt_quad_gram_csc_deliver_f64", *_gram_args(gram), P(varmap_buf), alpha, P(dp),
                                    host_P.ctypes.data_as(C.c_void_p), 0, P(dl), P(dc), P(ws))
        (dq, dl, dc), f = self._quad_buffers(ctx, n, nq, twin=True), self.f
        if not (self.model._overlap_moi and nq > 0):
            return lambda c: c.call("pmt_quad_gram_f64", *_gram_args(gram), 1, P(varmap_buf), P(dq), P(dl), P(dc), P(ws))
        # the quadratic terms leave for f.quadratic_terms (page-locked) row band by row band while the contraction runs
        self.delivered = ("quad",)
        return lambda c: c.call("pmt_quad_gram_deliver_f64", *_gram_args(gram), 1, P(varmap_buf), P(dq),
                                f.quadratic_terms.ctypes.data_as(C.c_void_p), 0, P(dl), P(dc), P(ws))

    def _compile_form(self, ctx, varmap_buf, handoff_varmap):
        """transpose(x) * Q * x alone (plan.form): pmt_quad_form_f64 reads the Parameter matrix and writes the canonical
        MOI function — n(n+1)/2 quadratic terms, no linear terms, constant 0.0 — or, for the device hand-off, the CSC values of P.
        A shifted form transpose(x (+|-) v) * Q * (x (+|-) v) (MOI boundary only, quad_plan): pmt_quad_form_shift_f64 writes the same
        quadratic terms, n linear terms and the constant."""
        form = self.plan.form
        n = form.mat.cols
        nq = n * (n + 1) // 2
        if form.vec is not None:
            (dq, dl, dc), ws = self._quad_buffers(ctx, n, nq, twin=False), _form_workspace(ctx, form)
            return lambda c: _form_call(c, form, varmap_buf, 1.0, (P(dq), None, P(dl), P(dc)), ws)
        if handoff_varmap is not None:
            dp, dl, dc, alpha = self._csc_buffers(ctx, form.xvars, handoff_varmap)
            return lambda c: c.call("pmt_quad_form_f64", *_form_args(form, varmap_buf, alpha), None, P(dp), P(dl), P(dc))
        dq, _, dc = self._quad_buffers(ctx, 0, nq, twin=False, lin=False)     # (no "lin": a bare form has no linear terms)
        return lambda c: c.call("pmt_quad_form_f64", *_form_args(form, varmap_buf, 1.0), P(dq), None, None, P(dc))

    def _compile_lsq_sum(self, ctx, varmap_buf, handoff_varmap):
        """The objective as a weighted sum of least-squares blocks over one x (plan.terms): block 1 by pmt_quad_gram_f64 straight into the
        MOI buffers, blocks 2..K as CSC values (pmt_quad_gram_csc_f64, bit for bit the same coefficients), then pmt_quad_gram_sum_f64 weights
        and adds everything in place.  A form transpose(x) * Q * x stands where a block stands: pmt_quad_form_f64 writes the same outputs
        (its linear terms and constant are zero).  The terms are final only after the combine: no overlapped delivery of the quadratic terms."""
        terms = self.plan.terms
        n = [t for t in terms if t.kind in ("block", "form")][0].r.mat.cols
        return self._lsq_sum_emitter(ctx, varmap_buf, terms, *self._quad_buffers(ctx, n, n * (n + 1) // 2, twin=False, floor=1))

    def _lsq_sum_emitter(self, ctx, varmap_buf, terms, dq, dl, dc):
        """The steps of _compile_lsq_sum for the term list `terms`, writing the function into the device buffers dq / dl / dc (addresses;
        n(n+1)/2 quadratic terms, n linear terms, the constant) — the whole objective's, or one group's part of it (_compile_groups)."""
        blocks = [t for t in terms if t.kind in ("block", "form")]
        g1 = blocks[0].r
        n = g1.mat.cols
        nq = n * (n + 1) // 2
        ws = [_gram_workspace(ctx, t.r) if t.kind == "block" else _form_workspace(ctx, t.r) for t in blocks]
        # per block 2..K: its CSC values, linear terms and constant
        parts = [(ctx.alloc(8 * max(nq, 1)), ctx.alloc(16 * max(n, 1)), ctx.alloc(8)) for _ in blocks[1:]]
        desc = [_lsq_desc(t) for t in terms]
        for d, part in zip([d for t, d in zip(terms, desc) if t.kind in ("block", "form")][1:], parts):
            d["values"], d["lin"], d["constant"] = part
        arr = _lib.lsq_terms(desc)
        # diagonal / linear terms over part of x: their positions in x (pmt_quad_gram_sum_sub_f64); over all of x: the plain combine
        lists = _term_positions(terms, g1.xvars.vars)
        sub = any(p is not None for p in lists)
        if sub:
            ptrs = (C.c_void_p * len(lists))(*[p.ctypes.data if p is not None else None for p in lists])
            counts = np.array([len(p) if p is not None else 0 for p in lists], dtype=np.int64)
            self._sub_args.append((lists, ptrs, counts))                    # (the entry reads them when the call is recorded)

        def emit_block(c, t, w, first, part):
            if t.kind == "form":
                outs = (P(dq), None, P(dl), P(dc)) if first else (None, P(part[0]), P(part[1]), P(part[2]))
                _form_call(c, t.r, varmap_buf, 1.0, outs, w)
            elif first:
                c.call("pmt_quad_gram_f64", *_gram_args(t.r), 1, P(varmap_buf), P(dq), P(dl), P(dc), P(w))
            else:
                c.call("pmt_quad_gram_csc_f64", *_gram_args(t.r), P(varmap_buf), 1.0, P(part[0]), None, P(part[1]), P(part[2]), P(w))

        def emit(c):
            emit_block(c, blocks[0], ws[0], True, None)
            for t, w, part in zip(blocks[1:], ws[1:], parts):
                emit_block(c, t, w, False, part)
            if sub:
                c.call("pmt_quad_gram_sum_sub_f64", n, C.addressof(arr), len(desc), C.cast(ptrs, C.c_void_p), counts.ctypes.data_as(C.c_void_p),
                       P(dq), P(dl), P(dc))
            else:
                c.call("pmt_quad_gram_sum_f64", n, C.addressof(arr), len(desc), P(dq), P(dl), P(dc))
        return emit

    def _compile_layout(self, ctx, lay, nconsts):
        """What _compile_groups and _compile_stages share (`lay`: the GroupsLayout of their pairwise disjoint Variable vectors): the function
        over the sorted union z, `nconsts` words for the parts' constants, and where the parts are written — their slices of the MOI buffers
        when every part's variables are consecutive in z (pointer + offset: no copy, no extra pass), an arena otherwise, from where
        pmt_quad_groups_gather_f64 places the rows through the tables uploaded here.  Returns (bq, bl, oq, ol, consts, dc, gather): part k
        starts oq[k] quadratic / ol[k] linear terms behind bq / bl; gather(c) emits the gather, or nothing without an arena."""
        n, nq = lay.nlin, lay.nterms
        (dq, dl, dc), consts = self._quad_buffers(ctx, n, nq, twin=False), ctx.alloc(8 * nconsts)
        self.groups_ordered = lay.ordered
        if lay.ordered:
            return dq, dl, lay.dst_quad, lay.dst_lin, consts, dc, lambda c: None
        bq, bl = ctx.alloc(24 * nq), ctx.alloc(16 * n)
        row_src, row_dst, lin_src = [ctx.upload_new(t) for t in (lay.row_src, lay.row_dst, lay.lin_src)]
        return bq, bl, lay.src_quad, lay.src_lin, consts, dc, \
            lambda c: c.call("pmt_quad_groups_gather_f64", P(bq), P(row_src), P(row_dst), n, nq, P(bl), P(lin_src), n, P(dq), P(dl))

    def _compile_groups(self, ctx, varmap_buf, handoff_varmap):
        """The objective as a sum over groups of blocks / forms with pairwise disjoint Variable vectors (plan.groups): every group is written
        by the steps of its own canonical-sum list (_lsq_sum_emitter) into its part of the layout (_compile_layout: its slice of the MOI
        buffers, or the arena and the gather).  pmt_quad_groups_constant_f64 adds the groups' constants.
        As in canonical-sum the terms are final only after the last step: no overlapped delivery of the quadratic terms."""
        groups, G = self.plan.groups, len(self.plan.groups)
        bq, bl, oq, ol, consts, dc, gather = self._compile_layout(ctx, _lib.GroupsLayout([g.vars for g in groups]), G)
        emits = [self._lsq_sum_emitter(ctx, varmap_buf, g.terms, bq + 24 * int(oq[k]), bl + 16 * int(ol[k]), consts + 8 * k)
                 for k, g in enumerate(groups)]

        def emit(c):
            for e in emits:
                e(c)
            gather(c)
            c.call("pmt_quad_groups_constant_f64", P(consts), G, P(dc))
        return emit

    def _compile_stages(self, ctx, varmap_buf, handoff_varmap):
        """The objective as a sum of horizon stages — dense forms, plain or shifted, over pairwise disjoint Variable vectors, more
        of them than "canonical-groups" holds (plan.stages): ONE pmt_quad_stages_f64 writes every stage's canonical function from a device
        table of descriptors built, checked (pmt_quad_stages_check) and uploaded here once, into the stages' parts of the layout
        (_compile_layout: their slices of the MOI buffers, or the arena and the unchanged gather).  The stages' constants are added by
        the call's own second launch.  With weights, linear terms or constants beside the stages (plan.stage_terms, plan.stage_consts)
        the one call is pmt_quad_stages_terms_f64 over two more tables, checked by pmt_quad_stages_terms_check.  With identity stages
        W_t*dot(x_t (+|-) v_t, x_t (+|-) v_t) (an IdentityStage among plan.stages: n diagonal terms, rows of length 1 in the layout) or
        diagonal terms riding on form stages (plan.stage_diags) it is pmt_quad_stages_diag_f64 over a third table, checked by
        pmt_quad_stages_diag_check.  Which of the three it is says plan.stage_entry; _stage_launch checks and uploads the tables.  update!
        allocates nothing and makes one call, or two with the gather."""
        stages = self.plan.stages
        ident = [q.mat is None for q in stages]
        lay = _lib.GroupsLayout([q.xvars.vars for q in stages], diagonal=ident if any(ident) else None)
        bq, bl, oq, ol, consts, dc, gather = self._compile_layout(ctx, lay, len(stages))
        launch = self._stage_launch(ctx, varmap_buf, self._stage_table(ctx, stages, oq, ol), lay.nterms, lay.nlin, (bq, bl, consts, dc))

        def emit(c):
            launch(c)
            gather(c)
        return emit

    def _compile_stages_csc(self, ctx, varmap_buf, handoff_varmap):
        """The horizon of _compile_stages for the device hand-off (plan "canonical-stages-csc"): ONE pmt_quad_stages_csc_f64 writes the
        solver's CSC values of the block-diagonal upper-triangular P — times the sense — instead of quadratic term structs, and the linear
        terms and the constant as the MOI entry points do.  The three tables are built, checked (pmt_quad_stages_csc_check) and uploaded
        here once.  The value slices lie one behind the other in the order of the stages' first optimizer index: when every stage's
        optimizer indices are consecutive that IS P's CSC order and the hand-off takes the buffer as it is (handoff.stage_blocks_pattern),
        otherwise its gather places the values.  The linear slices are concatenated in table order — the hand-off orders q itself —, so
        there is no arena and no gather here.  update! allocates nothing and makes one call."""
        stages = self.plan.stages
        T = len(stages)
        sizes = [len(q.xvars.vars) for q in stages]
        ident = [q.mat is None for q in stages]
        idx = [np.asarray(handoff_varmap, dtype=np.int64)[q.xvars.vars - 1] for q in stages]
        nval = [n if d else n * (n + 1) // 2 for n, d in zip(sizes, ident)]
        at = np.zeros(T, dtype=np.int64)
        order = np.argsort([int(i[0]) for i in idx], kind="stable")
        at[order] = np.cumsum([0] + [nval[k] for k in order])[:-1]
        ol = np.cumsum([0] + sizes)
        n, nvalues = int(ol[-1]), int(sum(nval))
        self.f = ScalarQuadraticFunction(n, 0, alloc=ctx.pinned_array)
        dp, dl, dc, consts = ctx.alloc(8 * nvalues), ctx.alloc(16 * n), ctx.alloc(8), ctx.alloc(8 * T)
        self.dev = {"lin": dl, "const": dc, "P_stage_values": dp,
                    "P_stage_blocks": [(idx[k], int(at[k]), ident[k]) for k in range(T)]}
        return self._stage_launch(ctx, varmap_buf, self._stage_table(ctx, stages, at, ol), nvalues, n, (dp, dl, consts, dc),
                                  alpha=-1.0 if self.model.sense == "Maximize" else 1.0)

    def _stage_launch(self, ctx, varmap_buf, arr, nq, n, outs, alpha=None):
        """The one call of the plan's stage entry point (plan.stage_entry: its check and launch symbols in _STAGE_ENTRIES) over the host stage
        table `arr` (_stage_table), whose slices lie in nq quadratic terms — "csc": values — and n linear terms; `outs`: the device buffers of
        the quadratic terms or values, the linear terms, the stages' constants and the constant; `alpha` ("csc"): the sense.  The side tables
        the entry takes are built here (_stage_side_tables: none for "plain"), the entry's check runs on the host arrays, and exactly the
        arrays it checked are uploaded: the kernel does not re-check, and no stage table reaches the device another way.  Returns the
        closure that makes the call."""
        entry = self.plan.stage_entry
        check, launch = _STAGE_ENTRIES[entry]
        T, nc = len(self.plan.stages), len(self.plan.stage_consts)
        tables = [arr]                                                    # in upload order: the stages, their terms, the constants, the riders
        if entry != "plain":
            # the weights, the vectors and the constants are device mirrors of Parameters, read by the launch at run time
            tarr, darr, carr = self._stage_side_tables(T)
            tables += [tarr, carr] if entry == "terms" else [tarr, carr, darr]

        def lead(stages, terms=None, consts=None, *riders):               # what the check's and the launch's arguments begin with: the tables' addresses
            return [stages, T] if entry == "plain" else [stages, terms, *riders, T, consts, nc]
        _lib.call(check, *lead(*[C.addressof(t) if t is not None else None for t in tables]), nq, n)
        args = lead(*[P(_table(ctx, t)) if t is not None else None for t in tables]) + [P(varmap_buf)] + ([alpha] if entry == "csc" else [])
        return lambda c: c.call(launch, *args, *map(P, outs))

    @staticmethod
    def _stage_table(ctx, stages, oq, ol):
        """the host pmt_quad_stage table of plan.stages, stage k's slices starting at oq[k] / ol[k] (an identity stage's variables may be a
        host-built term's: their indices get a device buffer here)"""
        vs = [_vec_sign(q.vec, q.sign) for q in stages]
        return _lib.quad_stages([{"Q": None, "xvar": ctx.upload_new(np.ascontiguousarray(q.xvars.vars, dtype=np.int64)), "vec": vec,
                                  "n": len(q.xvars.vars), "sign": sign, "quad_at": int(oq[k]), "lin_at": int(ol[k])} if q.mat is None else
                                 {"Q": q.mat.buf, "ldq": q.mat.lda, "xvar": q.xvars.buf, "vec": vec, "n": q.mat.cols, "sign": sign,
                                  "quad_at": int(oq[k]), "lin_at": int(ol[k])} for k, (q, (vec, sign)) in enumerate(zip(stages, vs))])

    def _stage_side_tables(self, T):
        """the host tables beside the T stages of pmt_quad_stages_terms_f64 / _diag_f64 / _csc_f64: (terms — unit rows without
        plan.stage_terms —, riders — None without plan.stage_diags: no stage has one —, constants); nothing is allocated"""
        sterms, sconsts, sdiags = self.plan.stage_terms, self.plan.stage_consts, self.plan.stage_diags
        tarr = _lib.quad_stage_terms([self._stage_terms_row(s) for s in sterms or [StageTerms()] * T])
        rvs = [_vec_sign(r.vec, r.sign) if r is not None else None for r in sdiags or ()]
        darr = _lib.quad_stage_diags([{} if r is None else {"scale": r.scale, "weight": _buf(r.param), "vec": rv[0], "sign": rv[1]}
                                      for r, rv in zip(sdiags, rvs)]) if sdiags is not None else None
        carr = _lib.quad_stage_consts([{"scale": k.scale, "weight": _buf(k.param), "value": _buf(k.value)} for k in sconsts])
        return tarr, darr, carr

    @staticmethod
    def _stage_terms_row(s):                                              # the pmt_quad_stage_terms fields of a StageTerms
        if s.lin is None:
            return {"scale": s.scale, "weight": _buf(s.param)}
        return {"scale": s.scale, "weight": _buf(s.param), "lin_scale": s.lin.scale, "lin_weight": _buf(s.lin.param), "lin_vec": s.lin.vec.buf}

    def _compile_sparse_gram(self, ctx, varmap_buf, handoff_varmap):
        """dot(r, r), r = C*x (+|-) d with a sparse C (plan.gram, a DSparseAff): pmt_sparse_gram_f64 streams the pattern's product list
        (DSpMat.gram_tables, built here once) and writes the canonical MOI function — one quadratic term per pair of columns sharing a row,
        one linear term per non-empty column.  The index fields are static (_static_indices); the kernel rewrites them through varmap_buf
        at every call, so the record follows the optimizer's index map like the dense forms."""
        r = self.plan.gram
        T = r.gram_tables()
        dq, dl, dc = self._quad_buffers(ctx, T.nlin, T.nq, twin=True)
        _static_indices(self.f, T, r.xvars, handoff_varmap)
        return lambda c: _sparse_gram_call(c, r, T, varmap_buf, dq, dl, dc)

    def _compile_sparse_form(self, ctx, varmap_buf, handoff_varmap):
        """transpose(x) * Q * x with a sparse Q (plan.form, a SparseQuadForm), the counterpart of _compile_sparse_gram: pmt_sparse_form_f64
        streams the pattern's pair and source tables (DSpMat.form_tables, built here once) and writes the canonical MOI function — one
        quadratic term per unordered pair with a stored entry, no linear terms, constant 0.0.  The index fields are static (_static_indices)."""
        form = self.plan.form
        T = form.form_tables()
        dq, _, dc = self._quad_buffers(ctx, 0, T.nq, twin=True)            # ("lin": no terms; the hand-off's generic route asks for the key)
        _static_indices(self.f, T, form.xvars, handoff_varmap)
        return lambda c: _sparse_form_call(c, form, T, varmap_buf, dq, dc)

    def _compile_sparse_sum(self, ctx, varmap_buf, handoff_varmap):
        """A weighted sum over sparse least-squares blocks, diagonal, linear and constant terms over one x (plan.terms; quad_plan:
        _sparse_sum_combines): every block by the unchanged pmt_sparse_gram_f64 (moi = 1) into its own scratch term lists, then ONE
        pmt_sparse_gram_sum_f64 weights and adds them through the gather tables of the symbolic merge (device.SparseSumTables, built here
        once) and writes every term of the MOI buffers once — also straight into the page-locked host arrays of a small model.  The index
        fields are static (_static_indices).  A sparse form transpose(x)*Q*x among the blocks (LsqTerm 'form', a SparseQuadForm) is written
        by pmt_sparse_form_f64 (moi = 1) into a scratch quad list and constant word of its own and described to the unchanged combine as a
        block without linear terms: a 16-byte dummy `lin`, the all-0xFFFFFFFF `lin_at` the merge writes for nlin_b = 0."""
        from .device import SparseSumTables
        terms = self.plan.terms
        blocks = [t for t in terms if t.kind in ("block", "form")]
        xv = blocks[0].r.xvars
        n = len(xv.vars)
        desc = [_lsq_desc(t) for t in terms]
        lists = _term_positions(terms, xv.vars)
        # a sparse form stands where a block stands: its own scratch quad list and constant word (pmt_sparse_form_f64, moi = 1), no linear terms
        Ts = [t.r.form_tables() if t.kind == "form" else t.r.gram_tables() for t in blocks]
        S = SparseSumTables(ctx, n, Ts, [(d["kind"], t.kind == "diag" and t.vec is not None, p) for t, d, p in zip(terms, desc, lists)])
        dq, dl, dc = self._quad_buffers(ctx, S.nlin, S.nq, twin=True)
        _static_indices(self.f, S, xv, handoff_varmap)
        # per block: the scratch lists pmt_sparse_gram_f64 writes (its own nq / nlin terms, its constant)
        parts = [(ctx.alloc(24 * max(T.nq, 1)), ctx.alloc(16 * max(T.nlin, 1)), ctx.alloc(8)) for T in Ts]
        k = 0
        for i, (t, d) in enumerate(zip(terms, desc)):
            if t.kind in ("block", "form"):
                d["quad"], d["lin"], d["constant"] = parts[k]             # (a form's lin: a dummy allocation; its lin_at is all 0xFFFFFFFF)
                d["quad_at"], d["lin_at"] = S.dev["quad_at"][k], S.dev["lin_at"][k]
                k += 1
            elif t.kind in ("diag", "linear"):
                d["pos"], d["nvec"] = S.dev["term_pos"].get(i), len(t.xvars.vars)
        arr = _lib.sparse_lsq_terms(desc)
        self._sub_args.append((S, arr))                                     # (the entry reads the descriptors when the call is recorded)

        def emit(c):
            for t, T, part in zip(blocks, Ts, parts):
                if t.kind == "form":
                    _sparse_form_call(c, t.r, T, varmap_buf, part[0], part[2])
                else:
                    _sparse_gram_call(c, t.r, T, varmap_buf, *part)
            c.call("pmt_sparse_gram_sum_f64", n, C.addressof(arr), len(desc), P(S.dev["pair_j"]), P(S.dev["pair_k"]), S.nq, P(S.dev["lin_col"]),
                   S.nlin, P(xv.buf), P(varmap_buf), P(dq), P(dl), P(dc))
        return emit

    # the quadratic forms by plan.mode (quad_plan)
    _QUAD_FORMS = {"canonical-sparse": _compile_sparse_gram, "canonical-sparse-form": _compile_sparse_form, "canonical-sparse-sum": _compile_sparse_sum, "literal": _compile_literal, "canonical": _compile_gram, "canonical-csc": _compile_gram, "canonical-form": _compile_form,
                   "canonical-sum": _compile_lsq_sum, "canonical-groups": _compile_groups, "canonical-stages": _compile_stages,
                   "canonical-stages-csc": _compile_stages_csc}

    # ---- Vector{AffineFunction}
    def _compile_vector(self, ctx, varmap_buf, handoff_varmap):
        out = self.expr.out
        implicit = isinstance(out, (DDenseAff, DVarsAff, DSparseAff)) and not out.need_terms
        if implicit and handoff_varmap is not None and self.model.handoff == "host_csc" and not isinstance(out, DSparseAff):
            emit = self._compile_static(ctx, np.asarray(handoff_varmap, dtype=np.int64)[out.xvars.vars - 1])
            if emit is not None:
                return emit
        self.f = VectorAffineFunction(out.nterms, out.rows, alloc=ctx.pinned_array)
        if isinstance(out, DDenseAff) and implicit:
            return self._compile_dense(ctx, varmap_buf)
        if isinstance(out, DVarsAff) and implicit:
            return self._compile_vars(ctx, varmap_buf)
        if isinstance(out, DSparseAff) and implicit:
            return (self._compile_sparse_blocks if out.spmat.block_cw else self._compile_sparse_slabs)(ctx, handoff_varmap)
        dt = self._twin(ctx, self.f._terms, 24 * out.nterms)
        m = out.materialized()
        self.dev = {"terms": dt, "consts": m.consts}
        return lambda c: c.call("pmt_pack_vector_affine_f64", P(m.terms), P(m.row_ptr_buf), m.rows, m.row_len, P(varmap_buf), 0, P(dt))

    def _compile_static(self, ctx, xv):
        """handoff="host_csc": the deliverable is the solver's CSC arrays on the host and the index map is fixed (Model.initialize), so the MOI
        terms of a dense block A*x (+|-) b or of x (+|-) v would be an intermediate nobody reads: A's CSC values are the Parameter matrix
        column by column (they leave straight out of its buffer, handoff.py) and the coefficients of x (+|-) v are the constant 1.0.
        Only the constants 0 (+|-) b are rebuilt per re-evaluation; the term STRUCTURE (rows, optimizer variables `xv`) is static host data.
        None: a dense block whose columns are permuted or repeated keeps its terms."""
        out = self.expr.out
        dense = isinstance(out, DDenseAff)
        if dense and not (len(xv) and np.all(np.diff(xv) > 0)):
            return None
        self.f = VectorAffineFunction(out.nterms, out.rows)
        t = self.f._terms
        if dense:
            t["out"], t["var"], t["coeff"] = np.repeat(np.arange(1, out.rows + 1), out.mat.cols), np.tile(xv, out.rows), np.nan
            self.f.coefficients_unavailable = ("handoff=\"host_csc\": the MOI terms of a dense constraint block are not packed (its coefficients "
                                               "are the Parameter matrix, delivered as the CSC values of model.device_qp.host); use .structure for "
                                               "rows / variables, or handoff=\"moi\" for the reference's MOI functions")
        else:
            t["out"], t["var"], t["coeff"] = np.arange(1, out.rows + 1), xv, 1.0
        dc = ctx.alloc(8 * max(out.rows, 1))
        ctx.zero(dc, 8 * max(out.rows, 1))
        self.dev = {"consts": dc}                                         # (no "terms": they never leave the host)
        self.side_lane_ok = True
        self.terms_static = True

        def emit(c):
            if out.vec is not None and out.rows:
                c.call("pmt_consts_f64", P(out.vec.buf), out.rows, out.sign, P(dc))
        return emit

    def _implicit_twins(self, ctx):
        """terms + constants twins of an implicit block (A*x (+|-) b, x (+|-) v, C*x (+|-) d): its pack reads Parameter values only and writes
        its own MOI buffers, so it may go to the side lane (Model.lane_order)"""
        out = self.expr.out
        dt, dc = self._twin(ctx, self.f._terms, 24 * out.nterms), self._twin(ctx, self.f.constants, 8 * out.rows)
        self.dev = {"terms": dt, "consts": dc}
        self.side_lane_ok = True
        return dt, dc

    def _compile_dense(self, ctx, varmap_buf):
        out = self.expr.out
        dt, dc = self._implicit_twins(ctx)
        vec, sign = _vec_sign(out.vec, out.sign)

        def emit(c):
            # on the side lane (Model._record_tape sets on_side_lane before the emitter runs): the low-footprint kernel that is co-resident
            # with the contraction it runs beside
            c.call("pmt_affine_pack_vector_background_f64" if self.on_side_lane else "pmt_affine_pack_vector_f64", P(out.mat.buf), out.mat.lda,
                   out.mat.rows, out.mat.cols, P(out.xvars.buf), P(vec), sign, P(varmap_buf), 0, P(dt), P(dc))
        return emit

    def _compile_vars(self, ctx, varmap_buf):
        out = self.expr.out
        dt, dc = self._implicit_twins(ctx)
        return lambda c: c.call("pmt_vars_addsub_f64", P(out.xvars.buf), out.rows, P(out.vec.buf), out.sign, P(varmap_buf), 0, None, P(dt), P(dc))

    # The sparse forms fold varmap into static variable words: it changes with the optimizer's index map (mapindices!, src/model.jl:100-107),
    # not per re-evaluation, so the kernel reads varmap[x[col]] instead of gathering it for every term.  Block form: one word per COLUMN
    # (staged in LDS per column band); slab form: one per term
    def _compile_sparse_blocks(self, ctx, handoff_varmap):
        out, sp = self.expr.out, self.expr.out.spmat
        dt, dc = self._implicit_twins(ctx)
        colvar = ctx.alloc(8 * max(sp.cols, 1))

        def refresh(varmap_host):
            v = out.xvars.vars if varmap_host is None else np.asarray(varmap_host, dtype=np.int64)[out.xvars.vars - 1]
            ctx.upload(colvar, np.ascontiguousarray(v, dtype=np.int64))
        self.varmap_hooks.append(refresh)
        refresh(handoff_varmap)
        # terms and constants (0 (+|-) d) in one launch
        return lambda c: c.call("pmt_sparse_pack_vector_blocks_f64", P(sp.buf), P(sp.block_desc_buf), P(sp.block_idx_buf), P(sp.block_band_buf),
                                P(colvar), sp.rows, sp.cols, sp.nnz, sp.block_cw, None, 0, P(out.vec.buf) if out.vec is not None else None,
                                out.sign if out.vec is not None else 0, P(dt), P(dc))

    def _compile_sparse_slabs(self, ctx, handoff_varmap):
        out, sp = self.expr.out, self.expr.out.spmat
        dt, dc = self._implicit_twins(ctx)
        mapped = ctx.alloc((4 if sp.narrow else 8) * max(sp.nnz, 1))

        def refresh(varmap_host):
            if sp.nnz:
                v = out.term_var if varmap_host is None else np.asarray(varmap_host, dtype=np.int64)[out.term_var - 1]
                if sp.narrow and (v.max() >= 2 ** 32 or v.min() < 0):
                    raise DimensionMismatch("sparse constraint: optimizer variable indices of 2^32 or more with a 32-bit pattern")
                ctx.upload(mapped, v.astype(np.uint32) if sp.narrow else np.ascontiguousarray(v))
        self.varmap_hooks.append(refresh)
        refresh(handoff_varmap)

        def emit(c):
            c.call("pmt_sparse_pack_vector_slabs_u32_f64" if sp.narrow else "pmt_sparse_pack_vector_slabs_f64", P(sp.buf), P(sp.perm_buf), P(mapped),
                   P(sp.slab_ptr_buf), sp.rows, sp.nslab, None, 0, P(dt))
            if out.vec is not None:
                c.call("pmt_consts_f64", P(out.vec.buf), out.rows, out.sign, P(dc))
        return emit

    # ---- the MOI buffers' way to the host: every user of `buffers` goes through copies()
    def copies(self, skip=()):
        """(host array, device address) of the entries of `buffers` that need a D2H copy: a key absent from dev has none (P's CSC values are
        written instead of quadratic terms, a bare form has no linear terms, static terms never leave the host), and neither has a twin
        that IS the host array (a small model, _twin)"""
        if self.stage_group is not None:                                  # the group's two arenas travel with its first member
            return self.stage_group.copies(self)
        d = self.dev or {}
        return [(host, d[key]) for host, key in self.buffers if key in d and key not in skip and d[key] != host.ctypes.data]

    def record_fetch(self, ctx):
        """while recording (Model._overlap_moi): the same copies as fetch(), as tape entries behind this record's launches on their lane —
        they leave while the rest of the tape is still running (pmt_plan_record_fetch); what the contraction delivers itself (`delivered`:
        the quadratic terms of the canonical node) is not fetched"""
        for host, dptr in self.copies(skip=self.delivered):
            ctx.record_fetch(host, dptr, host.nbytes)
        self._fetch_recorded = True

    def fetch(self, ctx):
        """D2H of the MOI buffers into the host function object (asynchronous; caller synchronises)"""
        if not self._fetch_recorded:
            for host, dptr in self.copies():
                ctx.fetch(host, dptr, host.nbytes)

    def fetch_list(self):
        """(host array, key of self.dev) pairs fetch() copies — for a host that registers them once"""
        return list(self.buffers)

    def finish_fetch(self):
        if self.kind in ("aff", "quad"):
            self.f.constant = float(self._cbuf[0])


def _lsq_sum_combines(terms):
    """Whether pmt_quad_gram_sum_f64 / _sub_f64 can combine this LsqTerm list: 1 .. PMT_LSQ_MAX_BLOCKS least-squares blocks — forms
    transpose(x) * Q * x count among them —, at most PMT_LSQ_MAX_TERMS terms, every block over the same strictly increasing x (a stacked block
    over its sorted union z), every diagonal / linear term over x or a strictly increasing part of it (pmt_quad_gram_sum_sub_f64, whose launch
    holds at most PMT_LSQ_MAX_RUNS runs of positions)."""
    blocks = [t for t in terms or () if t.kind in ("block", "form")]
    if any(isinstance(t.r, (DSparseAff, SparseQuadForm)) for t in blocks):   # a sparse block or form: the dense combine cannot take it (_sparse_sum_combines)
        return False
    if any(t.host_scaled for t in terms or ()):                        # number * dot(u, u) multiplied on the host: the literal path, as before
        return False
    if len(terms or ()) > _lib.PMT_LSQ_MAX_TERMS or not 1 <= len(blocks) <= _lib.PMT_LSQ_MAX_BLOCKS or not blocks[0].r.xvars.strictly_increasing():
        return False
    x = blocks[0].r.xvars
    runs = 0
    for t in terms:
        if t.kind in ("block", "form"):
            if not np.array_equal(t.r.xvars.vars, x.vars):
                return False
        elif t.xvars is not None:
            pos = _part_of(t.xvars.vars, x.vars)
            if pos is False:
                return False
            runs += _lib.column_runs(pos) if pos is not None else 0
    return runs <= _lib.PMT_LSQ_MAX_RUNS


def _sparse_form_term(t):
    """the LsqTerm is transpose(x)*Q*x with a sparse Q (lazyexpression._rule_bilinear made it only for a strictly increasing x and a canonical pattern)"""
    return t is not None and t.kind == "form" and isinstance(t.r, SparseQuadForm)


def _sparse_sum_combines(terms):
    """Whether pmt_sparse_gram_sum_f64 can combine this LsqTerm list: 1 .. PMT_LSQ_MAX_BLOCKS blocks, every one a sparse Gram operand
    (DSparseAff.gram_operand) or a sparse form transpose(x)*Q*x (SparseQuadForm: it stands where a block stands and counts among them) — no
    dense block, no dense form beside them —, at most PMT_LSQ_MAX_TERMS terms, every block over the same strictly
    increasing x, every diagonal / linear term over x or a strictly increasing part of it (_lsq_sum_combines' subset rule; the positions
    are held in tables, so there is no limit on their runs)."""
    terms = terms or ()
    blocks = [t for t in terms if t.kind in ("block", "form")]
    if not 1 <= len(blocks) <= _lib.PMT_LSQ_MAX_BLOCKS or len(terms) > _lib.PMT_LSQ_MAX_TERMS:
        return False
    if not all(_sparse_form_term(t) or (t.kind == "block" and isinstance(t.r, DSparseAff) and t.r.gram_operand()) for t in blocks):
        return False
    x = blocks[0].r.xvars.vars
    return all(np.array_equal(t.r.xvars.vars, x) if t.kind in ("block", "form") else t.xvars is None or _part_of(t.xvars.vars, x) is not False
               for t in terms)


# A sum over disjoint Variable vectors whose literal function is smaller than this keeps the literal expansion + canonicalize: such models
# (a dozen variables per vector, beyond the small plan only because they replay a graph) take that path today, the canonical nodes round
# differently from it, and a function of a few hundred KB gains nothing from them.  The mode is for the sums the literal path is slow
# on or cannot build.
GROUPS_MIN_LITERAL_TERMS = 1 << 14


class QuadGroup:
    """One group of a "canonical-groups" plan: its LsqTerm list in expression order and its sorted variables"""
    def __init__(self, terms, vars_):
        self.terms, self.vars = terms, vars_


def _lsq_groups(terms):
    """The QuadGroups of an LsqTerm list whose blocks / forms lie over 2 .. PMT_QUAD_MAX_GROUPS pairwise disjoint, strictly increasing
    Variable vectors, or None: groups in the order of the first appearance of one of their blocks; a diagonal / linear term joins the group
    that holds its variables (a strictly increasing part of ONE group's set: _lsq_sum_combines' subset rule), constants join the first group;
    every group's list, expression order kept, is one the combine takes on its own (_lsq_sum_combines).  A term over variables of no group,
    or of two, leaves the whole sum to the literal path."""
    groups = []
    for t in terms or ():
        if t.kind in ("block", "form") and not any(np.array_equal(t.r.xvars.vars, g.vars) for g in groups):
            groups.append(QuadGroup([], t.r.xvars.vars))
    if not 2 <= len(groups) <= _lib.PMT_QUAD_MAX_GROUPS or any(len(g.vars) == 0 or np.any(np.diff(g.vars) <= 0) for g in groups):
        return None
    z = np.concatenate([g.vars for g in groups])
    if len(np.unique(z)) != len(z):                                      # overlapping sets
        return None
    for t in terms:
        if t.kind in ("block", "form"):
            home = [g for g in groups if np.array_equal(t.r.xvars.vars, g.vars)]
        elif t.xvars is not None:
            home = [g for g in groups if len(t.xvars.vars) and t.xvars.vars[0] in g.vars]
        else:
            home = groups[:1]
        if not home:
            return None
        home[0].terms.append(t)
    return groups if all(_lsq_sum_combines(g.terms) for g in groups) else None


class StageTerms:
    """What stands beside stage t of a "canonical-stages" plan (pmt_quad_stage_terms): the stage's weight scale * param (param: the DNum of
    a scalar Parameter, or None) and its linear term dot(c_t, x_t) (`lin`: the 'linear' LsqTerm with its own scale / param / vec, or None)"""
    __slots__ = ("scale", "param", "lin")

    def __init__(self, scale=1.0, param=None, lin=None):
        self.scale, self.param, self.lin = scale, param, lin

    def plain(self):
        return self.scale == 1.0 and self.param is None and self.lin is None


class IdentityStage:
    """An identity stage of a "canonical-stages" plan, W_t*dot(x_t (+|-) v_t, x_t (+|-) v_t): it stands among plan.stages where a QuadForm
    stands, without a matrix (mat None); xvars / vec / sign are those of its 'diag' LsqTerm, the weight lies in its StageTerms."""
    __slots__ = ("xvars", "vec", "sign")
    mat = None

    def __init__(self, xvars, vec=None, sign=0):
        self.xvars, self.vec, self.sign = xvars, vec, sign


def _lsq_stages(terms, diag=False):
    """(QuadForms, StageTerms per stage or None, 'constant' LsqTerms) of an LsqTerm list that is a horizon of stage costs, or None: more
    than PMT_QUAD_MAX_GROUPS 'form' terms, every one a dense form transpose(x_t)*Q*x_t or transpose(x_t (+|-) v_t)*Q*(x_t (+|-) v_t) over a
    strictly increasing vector of 1 .. PMT_QUAD_STAGES_MAX_N variables, the vectors pairwise disjoint, and at least two stages reading the
    same weight matrix (the device mirror of one matrix Parameter) — the horizon's shape; nine unrelated forms keep the literal path.
    Every form may carry a weight (a number times at most one scalar Parameter: 0.5*(..), a discount, rho*transpose(u)*R*u); beside the
    forms stand 'linear' terms dot(c_t, x_t), each over exactly the vector of one stage and at most one per stage, and at most
    PMT_QUAD_STAGES_MAX_CONSTS 'constant' terms.  Anything else in the list — a block, a diagonal term, a sparse form, a linear term over
    part of a stage or over other variables, a second one on a stage — leaves the sum to the literal path.  The StageTerms are None when
    no stage has a weight or a linear term: with no constant either, the record is the unweighted one (pmt_quad_stages_f64).
    `diag` (pmt_quad_stages_diag_f64): 'diag' terms are taken too, host-scaled ones among them (the literal coefficient s of s*u_i*u_i,
    doubled by the MOI copy, and (2*W_d) are the same word), and the result has a fourth entry.  A diagonal term over exactly the vector of
    a form is that stage's rider; one over a vector of its own — strictly increasing, 1 .. PMT_QUAD_STAGES_MAX_N variables, disjoint from
    every other — is a stage, an IdentityStage among the QuadForms at its place in expression order.  At most one diagonal term per
    vector; one over part of a stage or across two leaves the sum literal.  Stages are counted as vectors: more than PMT_QUAD_MAX_GROUPS
    of them, at least two FORMS reading one matrix.  The fourth entry holds the rider's 'diag' LsqTerm per stage, or None without a rider."""
    terms = terms or ()
    kinds = ("form", "linear", "constant", "diag") if diag else ("form", "linear", "constant")
    if any(t.kind not in kinds or (t.host_scaled and not diag) for t in terms):
        return None
    consts = [t for t in terms if t.kind == "constant"]
    forms = [t for t in terms if t.kind == "form"]
    # a stage is named by its first variable (disjoint vectors); a diagonal term over a form's own vector rides on it, any other is a stage
    fvars = {int(t.r.xvars.vars[0]): t.r.xvars.vars for t in forms if isinstance(t.r, QuadForm) and len(t.r.xvars.vars)}
    riding = lambda t: len(t.xvars.vars) and np.array_equal(fvars.get(int(t.xvars.vars[0]), ()), t.xvars.vars)
    stages = [t for t in terms if t.kind == "form" or (t.kind == "diag" and not riding(t))]
    if len(stages) <= _lib.PMT_QUAD_MAX_GROUPS or len(consts) > _lib.PMT_QUAD_STAGES_MAX_CONSTS:
        return None
    for t in stages:
        if t.kind == "form" and not isinstance(t.r, QuadForm):
            return None
        v = t.r.xvars.vars if t.kind == "form" else t.xvars.vars
        if not 1 <= len(v) <= _lib.PMT_QUAD_STAGES_MAX_N or (t.kind == "form" and t.r.mat.cols != len(v)) or np.any(np.diff(v) <= 0):
            return None
    svars = [np.asarray(t.r.xvars.vars if t.kind == "form" else t.xvars.vars, dtype=np.int64) for t in stages]
    z = np.concatenate(svars)
    if len(np.unique(z)) != len(z) or len({id(t.r.mat) for t in forms}) == len(forms):
        return None
    stage_terms = [StageTerms(t.scale, t.param) for t in stages]
    first = {int(v[0]): k for k, v in enumerate(svars)}
    riders = [None] * len(stages)
    for t in terms:
        if t.kind == "linear":
            v = t.xvars.vars if t.xvars is not None else ()
            k = first.get(int(v[0])) if len(v) else None
            if k is None or t.vec is None or stage_terms[k].lin is not None or not np.array_equal(v, svars[k]):
                return None
            stage_terms[k].lin = t
        elif t.kind == "diag" and riding(t):
            k = first[int(t.xvars.vars[0])]
            if riders[k] is not None:
                return None
            riders[k] = t
    out = [t.r if t.kind == "form" else IdentityStage(t.xvars, t.vec, t.sign) for t in stages], \
        None if all(s.plain() for s in stage_terms) else stage_terms, consts
    return out + (riders if any(r is not None for r in riders) else None,) if diag else out


# QuadPlan.stage_entry -> the (check, launch) symbols of the horizon's stage entry point (_Record._stage_launch)
_STAGE_ENTRIES = {"plain": ("pmt_quad_stages_check", "pmt_quad_stages_f64"), "terms": ("pmt_quad_stages_terms_check", "pmt_quad_stages_terms_f64"),
                  "diag": ("pmt_quad_stages_diag_check", "pmt_quad_stages_diag_f64"), "csc": ("pmt_quad_stages_csc_check", "pmt_quad_stages_csc_f64")}


class QuadPlan:
    """How a quadratic record reaches its MOI function (quad_plan decides; Model.initialize and _Record.compile execute): the mode and what it
    reads — the operand r of dot(r, r) (`gram`), the QuadForm (`form`), the LsqTerm list (`terms`), the QuadGroups of a sum over disjoint
    Variable vectors (`groups`) or the QuadForms of a horizon of stage costs (`stages`, with the StageTerms beside them in `stage_terms` —
    None: every stage has weight 1 and no linear term —, the 'constant' LsqTerms in `stage_consts` and, per stage, the 'diag' LsqTerm riding
    on it in `stage_diags` — None: no stage has a rider; an IdentityStage stands among `stages` itself); `canonicalize`: through
    canonicalize! first."""
    def __init__(self, mode, gram=None, form=None, terms=None, canonicalize=False, groups=None, stages=None, stage_terms=None, stage_consts=(),
                 stage_diags=None):
        self.mode, self.gram, self.form, self.terms, self.canonicalize, self.groups = mode, gram, form, terms, canonicalize, groups
        self.stages, self.stage_terms, self.stage_consts, self.stage_diags = stages, stage_terms, list(stage_consts), stage_diags
        # the MOI copy is the canonical least-squares node, bare or the weighted sum of such nodes (model.lane_order: side lane, small-plan order)
        self.gram_record = mode in ("canonical", "canonical-csc", "canonical-sum") or \
            (mode == "canonical-groups" and any(t.kind == "block" for g in groups for t in g.terms))

    @property
    def stage_entry(self):
        """which of the four stage entry points writes a horizon of stage costs (a key of _STAGE_ENTRIES), each a superset of the one in
        front of it: "plain" — the stages alone —, "terms" — weights, linear terms or constants beside them —, "diag" — an identity
        stage among them or a rider —, "csc" — any of these as P's CSC values; None: the plan is no such horizon"""
        if self.mode == "canonical-stages-csc":
            return "csc"
        if self.mode != "canonical-stages":
            return None
        if self.stage_diags is not None or any(q.mat is None for q in self.stages):
            return "diag"
        return "plain" if self.stage_terms is None and not self.stage_consts else "terms"

    def operands(self):
        """what the plan's kernels read: the Gram operand, the forms and blocks of its term lists (Model.initialize: their stacked matrices)"""
        lists = [self.terms or ()] + [g.terms for g in self.groups or ()]
        return [r for r in [self.gram] + [t.r for ts in lists for t in ts] + list(self.stages or ()) if r is not None]


def quad_plan(terms, bare, kind, nq, is_objective, quadratic_mode, small, handoff, varmap=None, sparse_sums=False, stage_terms=False,
              stage_diag=False, stage_csc=False):
    """The QuadPlan of a record over a node described by (terms, bare) = DeviceNode.(lsq_sum, lsq_bare); no mode unless kind == "quad".  `nq`:
    the terms of its literal expansion; `small`: Model._small; `varmap`: the optimizer's index map when it is fixed before the plan is recorded
    (handoff "device" / "host_csc"); `sparse_sums`: weighted sums over sparse blocks take the sparse combine (Model passes True);
    `stage_terms`: a horizon with weights, linear terms or constants beside its stages takes "canonical-stages" (Model passes True; a caller
    that does not ask gets the row as it was: such a horizon stays literal); `stage_diag`: likewise for a horizon with identity-weighted
    stage costs — rho*dot(u_t, u_t) as a stage, a ridge beside a form (Model passes True); `stage_csc`: a horizon under handoff "device" takes
    "canonical-stages-csc", P's CSC values from the stage launch (Model passes True; without it such a horizon stays literal).  Host data only: nothing is allocated, no stacked matrix is asked for.  First match wins."""
    one = terms[0] if bare and kind == "quad" else None
    block = one.r if one is not None and one.kind == "block" else None
    if isinstance(block, DSparseAff) and (quadratic_mode == "literal" or handoff == "host_csc"):
        raise ArgumentError("dot(r, r) of a sparse residual C*x (+|-) d has the canonical sparse form only: %s is not available for it "
                            "(use quadratic_mode 'auto' or 'canonical' with handoff 'moi' or 'device')"
                            % ("quadratic_mode='literal'" if quadratic_mode == "literal" else "handoff='host_csc'"))
    sform = one.r if _sparse_form_term(one) else None
    if sform is not None and (quadratic_mode == "literal" or handoff == "host_csc"):
        raise ArgumentError("transpose(x) * Q * x with a sparse Q has the canonical sparse form only: %s is not available for it "
                            "(use quadratic_mode 'auto' or 'canonical' with handoff 'moi' or 'device')"
                            % ("quadratic_mode='literal'" if quadratic_mode == "literal" else "handoff='host_csc'"))
    if kind != "quad" or quadratic_mode == "literal":
        return QuadPlan("literal" if kind == "quad" else None)

    def ordered(x):                       # x keeps its order under the index map fixed early
        return handoff in ("device", "host_csc") and bool(np.all(np.diff(varmap[x.vars - 1]) > 0))
    def gram_plan(g):                     # (ordered: P's CSC values straight from the contraction's epilogue, no quadratic term structs)
        return QuadPlan("canonical-csc" if ordered(g.xvars) else "canonical", gram=g)
    # dot(r, r), r = A*x (+|-) b over a strictly increasing x: the Gram node, in any record and any model — asked for, or ("auto") above 2^24 terms
    if isinstance(block, DDenseAff) and block.xvars.strictly_increasing() and (quadratic_mode == "canonical" or nq > (1 << 24)):
        return gram_plan(block)
    # dot(r, r), r = C*x (+|-) d with a sparse C: the sparse Gram node, in "auto" too (a ragged residual has no literal alternative), for the MOI
    # boundary and the device hand-off, in small models and beyond
    if isinstance(block, DSparseAff):
        return QuadPlan("canonical-sparse", gram=block)
    # transpose(x) * Q * x with a sparse Q: the sparse form node, under exactly the bare sparse block's conditions (the literal builder walks
    # a dense matrix: no literal alternative either)
    if sform is not None:
        return QuadPlan("canonical-sparse-form", form=sform)
    # a weighted sum over sparse blocks, diagonal, linear and constant terms over one x: the blocks' sparse Gram nodes combined through
    # the merged pattern — like the bare node in "auto" too, for both boundaries, in small models and beyond, objective or constraint
    if sparse_sums and not bare and handoff in ("moi", "device") and _sparse_sum_combines(terms):
        return QuadPlan("canonical-sparse-sum", terms=terms)
    if quadratic_mode == "auto":
        return QuadPlan("literal")
    if not small:
        # dot(r, r) of a stacked residual (lazyexpression._stacked_form): the Gram node of its stacked matrix over the union z — beyond the small plan only
        if isinstance(block, DStackedAff) and block.xvars.strictly_increasing():
            return gram_plan(block)
        # transpose(x) * Q * x alone (lazyexpression._rule_bilinear): the canonical node reads Q itself — MOI terms, or P's CSC values for
        # the device hand-off when x keeps its order under the optimizer's index map.  A shifted form transpose(x (+|-) v) * Q * (x (+|-) v): the
        # MOI boundary only (the CSC shortcut has no place for its linear part q yet: the literal function + canonicalize! as any other quadratic)
        if is_objective and bare and one.kind == "form" and isinstance(one.r, QuadForm) and \
                (handoff == "moi" or (handoff == "device" and one.r.vec is None and ordered(one.r.xvars))):
            return QuadPlan("canonical-form", form=one.r)
        # a weighted sum of least-squares blocks over one x: combined from the blocks' Gram nodes — the MOI boundary of a model beyond the small plan only
        if is_objective and handoff == "moi" and not bare and _lsq_sum_combines(terms):
            return QuadPlan("canonical-sum", terms=terms)
        # such sums over pairwise disjoint Variable vectors (transpose(x)*Q*x + transpose(u)*R*u): the groups' own canonical functions,
        # interleaved in (row, column) order — under the same conditions, from GROUPS_MIN_LITERAL_TERMS literal terms on
        if is_objective and handoff == "moi" and not bare and nq >= GROUPS_MIN_LITERAL_TERMS:
            groups = _lsq_groups(terms)
            if groups:
                return QuadPlan("canonical-groups", groups=groups)
            # a horizon of stage costs — more disjoint vectors than the groups hold, every form dense, plain or shifted, two or more of
            # them reading one weight matrix: all stages from one launch (pmt_quad_stages_f64; with weights, linear terms dot(c_t, x_t)
            # or constants beside the stages pmt_quad_stages_terms_f64; with diagonal terms as stages or beside them
            # pmt_quad_stages_diag_f64)
            stages = _lsq_stages(terms, diag=stage_diag)
            if stages:
                plan = QuadPlan("canonical-stages", stages=stages[0], stage_terms=stages[1], stage_consts=stages[2],
                                stage_diags=stages[3] if stage_diag else None)
                if stage_terms or plan.stage_entry != "terms":                # (the weighted entry only for a caller that asks for it)
                    return plan
        # the same horizon for the device hand-off: the stage launch writes the solver's CSC values of the block-diagonal P itself
        # (pmt_quad_stages_csc_f64) — every stage's vector has to keep its order under the optimizer's index map, as canonical-csc asks
        if stage_csc and is_objective and handoff == "device" and not bare and nq >= GROUPS_MIN_LITERAL_TERMS:
            stages = _lsq_stages(terms, diag=True)
            if stages and all(ordered(q.xvars) for q in stages[0]):
                return QuadPlan("canonical-stages-csc", stages=stages[0], stage_terms=stages[1], stage_consts=stages[2], stage_diags=stages[3])
    # anything else: the literal function through the generic device canonicalize! (sorted, duplicates combined) before the MOI copy
    return QuadPlan("literal", canonicalize=True)


# A horizon's dynamics records (x_{t+1} == A*x_t + B*u_t (+ w_t) for every stage) are grouped from this many on: more than "canonical-groups"
# holds, the objective's own threshold for "canonical-stages" (_lsq_stages), so a horizon model gets both launches or neither.  Measured
# (tools/affine_stages_probe.py, profiles/r21_affine_stages.txt): at nine records of 10 x (1 + 10 + 4) terms the group is already the faster
# plan — update! 308 against 361 us under a graph replay, 370 against 626 us as a tape with recorded fetches — and the ratio only grows
# with T (3.5 x at 100 x (64, 32)); no crossover above the threshold.
AFFINE_STAGE_MIN_RECORDS = 9


class AffineStageGroup:
    """The vector-affine constraint records one pmt_affine_stages_f64 launch writes (affine_stage_group decides; Model.initialize attaches
    the group to its members, _Record.compile executes).  `members` in update! order, `leaves` their affine_stage_leaves.  One page-locked
    arena for all terms and one for all constants, each with a device twin; every member's VectorAffineFunction lies over its slices, so
    set_constraint_function, .terms, .constants and mapindices! see what they see today.  The first member's emitter makes the call and
    its copies() are the group's two fetches; the other members emit and fetch nothing.  The tables are built, checked
    (pmt_affine_stages_check) and uploaded when the first member is compiled: update! allocates nothing."""

    def __init__(self, members, leaves):
        self.members, self.leaves = members, leaves
        self.terms_host = self.consts_host = None
        self.dev = None

    def _layout(self):
        """the part and stage tables as lists of dicts, the members' slices, (nterms, nconsts)"""
        parts, stages, slices = [], [], []
        ta = ca = 0
        for r, leaves in zip(self.members, self.leaves):
            rows, first, row_len, vec, vs = r.expr.out.rows, len(parts), 0, None, 0
            for kind, d, sign in leaves:
                if kind == "mat":
                    parts.append({"mat": d.mat.buf, "ld": d.mat.lda, "xvar": d.xvars.buf, "cols": d.mat.cols, "sign": sign})
                    row_len += d.mat.cols
                elif kind == "vars":
                    parts.append({"mat": None, "ld": 0, "xvar": d.buf, "cols": 1, "sign": sign})
                    row_len += 1
                else:
                    vec, vs = d.buf, sign
            stages.append({"vec": vec, "term_offset": ta, "const_offset": ca, "row_len": row_len, "rows": rows, "first_part": first,
                           "nparts": len(parts) - first, "vec_sign": vs})
            slices.append((ta, rows * row_len, ca, rows))
            ta, ca = ta + rows * row_len, ca + rows
        return parts, stages, slices, ta, ca

    def _build(self, ctx, varmap_buf):
        parts, stages, self.slices, nterms, nconsts = self._layout()
        parr, sarr = _lib.affine_parts(parts), _lib.affine_stages(stages)
        T = len(stages)
        _lib.call("pmt_affine_stages_check", C.addressof(sarr), T, C.addressof(parr), len(parts), nterms, nconsts)
        self.terms_host, self.consts_host = ctx.pinned_array(nterms, VAT), ctx.pinned_array(nconsts, np.float64)
        dterms, dconsts = ctx.alloc(24 * nterms), ctx.alloc(8 * nconsts)
        self.dev = {"terms": dterms, "consts": dconsts}
        stable, ptable = _table(ctx, sarr), _table(ctx, parr)
        return lambda c: c.call("pmt_affine_stages_f64", P(stable), T, P(ptable), P(varmap_buf), P(dterms), P(dconsts))

    def compile_member(self, r, ctx, varmap_buf):
        """sets r.f (over the member's arena slices) and r.dev; returns the member's emitter — the launch for the first, nothing for the rest"""
        k = [i for i, m in enumerate(self.members) if m is r][0]
        emit = self._build(ctx, varmap_buf) if k == 0 else (lambda c: None)
        ta, nt, ca, rows = self.slices[k]
        arena = {np.dtype(VAT): self.terms_host[ta:ta + nt], np.dtype(np.float64): self.consts_host[ca:ca + rows]}
        r.f = VectorAffineFunction(nt, rows, alloc=lambda n, dtype: arena[np.dtype(dtype)])
        r.dev = {"terms": self.dev["terms"] + 24 * ta, "consts": self.dev["consts"] + 8 * ca}
        return emit

    def copies(self, r):
        if r is not self.members[0] or self.dev is None:
            return []
        return [(host, dptr) for host, dptr in ((self.terms_host, self.dev["terms"]), (self.consts_host, self.dev["consts"])) if host.nbytes]


def affine_stage_group(records, small, handoff):
    """The AffineStageGroup of a model's records (`records`: the non-constant records in update! order), or None.  The one decision on
    the horizon dynamics' path: tests and tools/affine_stages_probe.py replace this function by one that returns None and get the plan
    every record had before for the same model.

    A record is eligible when it is a vector-affine constraint whose expression flattens (lazyexpression.affine_stage_leaves), whose
    node nobody else consumes — no other record over the same node, no consumer that asked for its terms — and that has a row.  The
    eligible records form the group when the model is beyond the small plan, the boundary is the host MOI functions (handoff "moi"),
    there are at least AFFINE_STAGE_MIN_RECORDS of them and two of them read the same matrix (a horizon's shape: nine unrelated records
    keep their own chains).  Every other record, interleaved among them or not, keeps its path and its place."""
    if small or handoff != "moi":
        return None
    nodes = [id(r.expr) for r in records]
    members, leaves = [], []
    for r in records:
        if not isinstance(r, Constraint) or r.kind != "affvec" or nodes.count(id(r.expr)) != 1:
            continue
        lv = affine_stage_leaves(r.expr)
        if lv is None or r.expr.out.need_terms or r.expr.out.rows < 1:
            continue
        members.append(r)
        leaves.append(lv)
    if len(members) < AFFINE_STAGE_MIN_RECORDS:
        return None
    readers = {}
    for k, lv in enumerate(leaves):
        for kind, d, _ in lv:
            if kind == "mat":
                readers.setdefault(id(d.mat), set()).add(k)
    if not any(len(v) >= 2 for v in readers.values()):
        return None
    return AffineStageGroup(members, leaves)


class Objective(_Record):                                                 # src/moi_interop.jl:113-137
    def __init__(self, model, expr):
        self._setup(model, expr)
        if self.kind not in ("aff", "quad"):
            raise ArgumentError("the objective must be a scalar affine or quadratic function")


class Constraint(_Record):                                                # src/moi_interop.jl:141-175
    def __init__(self, model, expr, set_, function=None):
        self.set = set_
        self.modelindex = None
        self.optimizerindex = None
        if function is not None:                                          # SingleVariable-in-Integer/ZeroOne (:161-165)
            self.model, self.expr, self.isconstant, self.kind, self.f, self.nrows, self.dev = model, None, True, "single", function, 1, None
            return
        self._setup(model, expr)

    @property
    def spec(self):
        fname = {"aff": "scalaraffinefunction", "quad": "scalarquadraticfunction", "affvec": "vectoraffinefunction", "single": "singlevariable"}[self.kind]
        return fname + "_in_" + type(self.set).__name__.lower()


# the 14 typed constraint vectors in the reference's fixed order (src/moi_interop.jl:180-193)
CONSTRAINT_ORDER = [
    "scalaraffinefunction_in_greaterthan", "scalaraffinefunction_in_lessthan", "scalaraffinefunction_in_equalto",
    "vectoraffinefunction_in_nonnegatives", "vectoraffinefunction_in_nonpositives", "vectoraffinefunction_in_zeros",
    "scalarquadraticfunction_in_greaterthan", "scalarquadraticfunction_in_lessthan", "scalarquadraticfunction_in_equalto",
    "vectorquadraticfunction_in_nonnegatives", "vectorquadraticfunction_in_nonpositives", "vectorquadraticfunction_in_zeros",
    "singlevariable_in_integer", "singlevariable_in_zeroone",
]


class Constraints:                                                        # src/moi_interop.jl:195-262
    def __init__(self):
        self.by_spec = {name: [] for name in CONSTRAINT_ORDER}

    def push(self, c):
        if c.spec not in self.by_spec:
            raise ArgumentError("unsupported constraint type %s" % c.spec)
        self.by_spec[c.spec].append(c)

    def __iter__(self):                                                    # update! order (:236-247)
        for name in CONSTRAINT_ORDER:
            yield from self.by_spec[name]

    def __len__(self):
        return sum(len(v) for v in self.by_spec.values())
