"""CPU-only: horizon dynamics constraints x+ == A*x + B*u (+ w) as one launch (pmt_affine_stages_f64, moi.affine_stage_group).  The numpy
restatement of the header's contract (affine_stages_util) against the oracle's vecadd! / vecsubtract! and MOI copy for four spellings of the
dynamics, on integer views with signed zeros; pmt_affine_stages_check; the two descriptors' layout in the header, ctypes and Julia; the
flattening of a record's expression (lazyexpression.affine_stage_leaves); the group decision and what a compiled group allocates, calls and
fetches on a stub context, beside the plan the same records had before."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import affine_stages_util as U
from test_record_tape_host import FAKE, VARMAP_BUF, StubContext, _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(U.SPELLINGS)


@pytest.fixture(scope="module")
def lib():
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


# ---- 1. the restatement against the oracle's builders
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("rows,nu", [(5, 3), (1, 1), (67, 9)])
def test_restatement_equals_the_oracle_chain(lib, name, rows, nu):
    """matvecmul! per product, vecadd! / vecsubtract! per + / -, update!(::MOI.VectorAffineFunction, fs, varmap): every word on integer
    views; A, B and w hold +0.0 and -0.0 entries"""
    from oracle import oracle as O
    rng = np.random.default_rng(rows * 31 + nu)
    A, B, w = U.special(rng, (rows, rows)), U.special(rng, (rows, nu)), U.special(rng, rows)
    w[0], w[-1] = -0.0, 0.0
    n = 2 * rows + nu
    perm = rng.permutation(n) + 1
    xp, x, u = perm[:rows].astype(np.int64), perm[rows:2 * rows].astype(np.int64), perm[2 * rows:].astype(np.int64)
    varmap = (rng.permutation(n) + 1 + 100).astype(np.int64)

    class Vec:
        """an operand of the oracle's vecadd! / vecsubtract!: an AffVec, Variable indices or numbers"""
        def __init__(self, v):
            self.v = v

        def _with(self, o, subtract):
            a, b = self.v, o.v
            if O._kind(a) == "vars" and O._kind(b) == "affs":
                # vecsubtract!(dest, x::Vector{Variable}, y): dest[i] = x[i] (copyto! :421: one (1.0, var) term, constant 0) first
                a = O.AffVec(len(a)).vecadd(a, np.zeros(len(a)))
            return Vec(O.AffVec(len(a) if not isinstance(a, O.AffVec) else a.n).vecaddsub(a, b, subtract))

        def __add__(self, o):
            return self._with(o, False)

        def __sub__(self, o):
            return self._with(o, True)

    Ax, Bu = O.AffVec(rows).matvecmul_vars(A, x), O.AffVec(rows).matvecmul_vars(B, u)
    got = U.spelled_expression(name, Vec(Ax), Vec(Bu), Vec(xp), Vec(w)).v
    terms, consts = got.moi(varmap)
    want_t, want_c = U.restate_stage(U.spelled_stage(name, A, B, xp, x, u, w), varmap)
    assert np.array_equal(terms.view(np.int64), want_t.view(np.int64))
    assert np.array_equal(consts.view(np.int64), want_c.view(np.int64))
    # not vacuous: flipped signs of zeros are in the image, and the constants hold no -0.0
    if "w" in [leaf for leaf, _ in U.SPELLINGS[name]]:
        assert not np.any(np.signbit(want_c[want_c == 0.0])) and np.any(want_c == 0.0)
    zero = want_t["coeff"] == 0.0
    assert rows == 1 or (np.any(np.signbit(want_t["coeff"][zero])) and np.any(~np.signbit(want_t["coeff"][zero])))


# ---- 2. pmt_affine_stages_check
def _tables(lib, edit_stage=None, edit_part=None, T=3):
    parts, stages = [], []
    ta = ca = 0
    for t in range(T):
        rows, nx, nu = 3 + t, 3 + t, 2
        first = len(parts)
        parts += [{"mat": None, "xvar": FAKE, "cols": 1, "sign": 1}, {"mat": FAKE, "ld": rows + 1, "xvar": FAKE, "cols": nx, "sign": -1},
                  {"mat": FAKE, "ld": rows, "xvar": FAKE, "cols": nu, "sign": -1}]
        L = 1 + nx + nu
        stages.append({"vec": FAKE if t % 2 == 0 else None, "vec_sign": -1 if t % 2 == 0 else 0, "rows": rows, "first_part": first, "nparts": 3,
                       "row_len": L, "term_offset": ta, "const_offset": ca})
        ta, ca = ta + rows * L, ca + rows
    for (t, field), value in (edit_stage or {}).items():
        stages[t][field] = value
    for (k, field), value in (edit_part or {}).items():
        parts[k][field] = value
    return lib.affine_stages(stages), lib.affine_parts(parts), len(parts), ta, ca


def _check(lib, tables, T=3, dt=0, dc=0):
    sarr, parr, nparts, nt, nc = tables
    lib.call("pmt_affine_stages_check", C.addressof(sarr), T, C.addressof(parr), nparts, nt + dt, nc + dc)


def test_check_accepts_a_built_table(lib):
    _check(lib, _tables(lib))
    _check(lib, _tables(lib, T=1), T=1)
    lib.call("pmt_affine_stages_check", None, 0, None, 0, 0, 0)
    # the stages in any order of their slices
    t = _tables(lib)
    sarr = t[0]
    a, b = (sarr[0].term_offset, sarr[0].const_offset), (sarr[2].term_offset, sarr[2].const_offset)
    s0, s2 = lib.AffineStage.from_buffer_copy(sarr[0]), lib.AffineStage.from_buffer_copy(sarr[2])
    sarr[0], sarr[2] = s2, s0
    assert (sarr[0].term_offset, sarr[0].const_offset) == b and (sarr[2].term_offset, sarr[2].const_offset) == a
    _check(lib, t)
    # nparts at both ends of its range
    parts = [{"mat": None, "xvar": FAKE, "cols": 1, "sign": -1}] * 8
    one = lib.affine_stages([{"rows": 2, "first_part": 0, "nparts": 8, "row_len": 8}, {"rows": 2, "first_part": 3, "nparts": 1, "row_len": 1,
                                                                                          "term_offset": 16, "const_offset": 2}])
    parr = lib.affine_parts(parts)
    lib.call("pmt_affine_stages_check", C.addressof(one), 2, C.addressof(parr), 8, 18, 4)


@pytest.mark.parametrize("stage,part", [
    ({(1, "vec_sign"): 2}, {}), ({(0, "vec_sign"): 0}, {}), ({(1, "vec_sign"): 1}, {}), ({(0, "vec"): None}, {}),
    ({}, {(4, "sign"): 0}), ({}, {(4, "sign"): 2}), ({}, {(0, "sign"): -2}), ({}, {(5, "xvar"): None}),
], ids=["vec-sign-two", "vector-without-sign", "sign-without-vector", "null-vec-with-sign", "part-sign-zero", "part-sign-two", "part-sign-minus-two",
        "null-xvar"])
def test_check_refuses_invalid_arguments(lib, stage, part):
    with pytest.raises(lib.ArgumentError, match="affine_stages"):
        _check(lib, _tables(lib, stage, part))


@pytest.mark.parametrize("stage,part,T,dt,dc", [
    ({(1, "term_offset"): 17}, {}, 3, 0, 0), ({(2, "const_offset"): 6}, {}, 3, 0, 0),            # overlap by one
    ({(2, "term_offset"): 47}, {}, 3, 1, 0), ({(2, "const_offset"): 8}, {}, 3, 0, 1),            # a gap of one
    ({}, {}, 3, 1, 0), ({}, {}, 3, 0, 1), ({}, {}, 3, -1, 0), ({}, {}, 3, 0, -1),                # the slices do not end at the totals
    ({(0, "term_offset"): -1}, {}, 3, 0, 0),
    ({(1, "nparts"): 0}, {}, 3, 0, 0), ({(0, "nparts"): 9}, {}, 3, 0, 0), ({(2, "first_part"): 7}, {}, 3, 0, 0), ({(2, "first_part"): -1}, {}, 3, 0, 0),
    ({(1, "row_len"): 6}, {}, 3, 0, 0), ({(1, "row_len"): 8}, {}, 3, 0, 0),
    ({(1, "rows"): 0}, {}, 3, 0, 0), ({}, {(2, "ld"): 2}, 3, 0, 0), ({}, {(1, "cols"): 0}, 3, 0, 0), ({}, {(0, "cols"): 2}, 3, 0, 0),
    ({}, {}, -1, 0, 0),
], ids=["term-overlap", "const-overlap", "term-gap", "const-gap", "terms-short-of-the-total", "consts-short-of-the-total", "terms-past-the-total",
        "consts-past-the-total", "slice-below-zero", "nparts-zero", "nparts-nine", "parts-past-the-table", "parts-below-zero", "row-len-below-the-sum",
        "row-len-above-the-sum", "rows-zero", "ld-below-rows", "cols-zero", "variable-part-of-two-cols", "T-negative"])
def test_check_refuses_dimension_mismatches(lib, stage, part, T, dt, dc):
    with pytest.raises(lib.DimensionMismatch, match="affine_stages"):
        _check(lib, _tables(lib, stage, part), T, dt, dc)


def test_check_and_entry_point_refuse_null_tables(lib):
    sarr, parr, nparts, nt, nc = _tables(lib)
    with pytest.raises(lib.ArgumentError, match="affine_stages"):
        lib.call("pmt_affine_stages_check", None, 3, C.addressof(parr), nparts, nt, nc)
    with pytest.raises(lib.ArgumentError, match="affine_stages"):
        lib.call("pmt_affine_stages_check", C.addressof(sarr), 3, None, nparts, nt, nc)
    for bad in range(4):                                                   # the launch: before any device call
        args = [FAKE, 3, FAKE, FAKE, FAKE, FAKE]
        args[(0, 2, 4, 5)[bad]] = None
        with pytest.raises(lib.ArgumentError, match="affine_stages"):
            lib.call("pmt_affine_stages_f64", *args, None)
    with pytest.raises(lib.DimensionMismatch, match="affine_stages"):
        lib.call("pmt_affine_stages_f64", FAKE, -1, FAKE, FAKE, FAKE, FAKE, None)
    lib.call("pmt_affine_stages_f64", None, 0, None, None, None, None, None)   # no stage: nothing to do


# ---- 3. the descriptors: header, ctypes, Julia
@pytest.mark.parametrize("cname,cls,jname,size,offsets", [
    ("pmt_affine_part", "AffinePart", "AffinePart", 32, {"mat": 0, "ld": 8, "xvar": 16, "cols": 24, "sign": 28}),
    ("pmt_affine_stage", "AffineStage", "AffineStage", 48, {"vec": 0, "term_offset": 8, "const_offset": 16, "row_len": 24, "rows": 32, "first_part": 36,
                                                            "nparts": 40, "vec_sign": 44}),
])
def test_descriptor_layouts_agree_in_header_ctypes_and_julia(lib, tmp_path, cname, cls, jname, size, offsets):
    import subprocess
    S = getattr(lib, cls)
    assert C.sizeof(S) == size and {name: getattr(S, name).offset for name, _ in S._fields_} == offsets
    hdr = open(os.path.join(ROOT, "include", "parametron_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % cname, hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [name for decl in body.split(";") for name in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert fields == [name for name, _ in S._fields_]
    assert "#define PMT_AFFINE_STAGES_MAX_PARTS %d" % lib.PMT_AFFINE_STAGES_MAX_PARTS in hdr and lib.PMT_AFFINE_STAGES_MAX_PARTS == 8
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "parametron_hip.h"\n_Static_assert(sizeof(%s) == %d, "size");\n' % (cname, size) +
                   "".join('_Static_assert(offsetof(%s, %s) == %d, "%s");\n' % (cname, k, v, k) for k, v in offsets.items()) +
                   "int main(void) { return 0; }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    jl = open(os.path.join(ROOT, "julia", "ParametronHIP.jl")).read()
    jfields = re.findall(r"^\s+(\w+)::(\w+)\s*$", re.search(r"struct %s\n(.*?)\nend" % jname, jl, flags=re.S).group(1), flags=re.M)
    width = {"DevPtr": 8, "Int64": 8, "Int32": 4}
    assert [f for f, _ in jfields] == [name for name, _ in S._fields_]
    assert [width[t] for _, t in jfields] == [C.sizeof(t) for _, t in S._fields_]
    for name in ("pmt_affine_stages_check", "pmt_affine_stages_f64"):
        assert "(:%s, lib)" % name in jl and name in lib.SIGNATURES and hasattr(C.CDLL(lib.LIB_PATH), name)


# ---- 4. the flattening, on device values without a device
class Horizon:
    """the nodes of a horizon's dynamics built by the real rules (lazyexpression._rule_vec_addsub) on a stub context: T stages over
    consecutive Variables [x_0, u_0, x_1, ..], A and B shared (or one pair per stage)"""

    def __init__(self, lib, T=9, nx=4, nu=2, shared=True, **model_kw):
        from parametron_jl_amd.device import DMat
        self.lib, self.ctx, self.model = lib, StubContext(lib), _model(**model_kw)
        self.T, self.nx, self.nu, self.shared = T, nx, nu, shared
        self.A, self.B = DMat(self.ctx, nx, nx), DMat(self.ctx, nx, nu)

    def node(self, out):
        from parametron_jl_amd.lazyexpression import DeviceNode
        return DeviceNode(self.model, "test", [], out, lambda c: None)

    def x(self, t):
        return np.arange(1, self.nx + 1, dtype=np.int64) + t * (self.nx + self.nu)

    def u(self, t):
        return self.x(t)[-1] + np.arange(1, self.nu + 1, dtype=np.int64)

    def operand(self, out):
        """an operand with + and - that go through the vector rule"""
        from parametron_jl_amd import lazyexpression as L
        h = self

        class Op:
            def __init__(self, node):
                self.node = node

            def __add__(self, o):
                return Op(L._rule_vec_addsub(h.model, h.ctx, self.node, o.node, +1))

            def __sub__(self, o):
                return Op(L._rule_vec_addsub(h.model, h.ctx, self.node, o.node, -1))
        return Op(self.node(out))

    def product(self, mat, idx):
        from parametron_jl_amd.device import DDenseAff, DVars

        def emit(c):
            if out.need_terms:
                c.call("pmt_affine_assemble_f64", out.rows, out.rows, mat.cols, 0)
        out = DDenseAff(self.ctx, mat, DVars.of_indices(self.ctx, idx), None, 0)
        op = self.operand(out)
        op.node._emit = emit
        return op

    def variables(self, idx):
        from parametron_jl_amd.device import DVars
        return self.operand(DVars.of_indices(self.ctx, idx))

    def numbers(self, n=None):
        from parametron_jl_amd.device import DVec
        return self.operand(DVec(self.ctx, n or self.nx))

    def dynamics(self, name, t):
        from parametron_jl_amd.device import DMat
        A, B = (self.A, self.B) if self.shared else (DMat(self.ctx, self.nx, self.nx), DMat(self.ctx, self.nx, self.nu))
        return U.spelled_expression(name, self.product(A, self.x(t)), self.product(B, self.u(t)), self.variables(self.x(t + 1)), self.numbers()).node

    def bound(self, t):
        """x_t - lo: an implicit block of its own"""
        return (self.variables(self.x(t)) - self.numbers()).node

    def records(self, names, bounds_every=0):
        from parametron_jl_amd import moi
        out = []
        for t in range(self.T):
            if bounds_every and t % bounds_every == 0:
                out.append(moi.Constraint(self.model, self.bound(t), moi.Nonnegatives(self.nx)))
            out.append(moi.Constraint(self.model, self.dynamics(names[t % len(names)], t), moi.Zeros(self.nx)))
        return out


@pytest.mark.parametrize("name", NAMES)
def test_leaves_of_every_spelling(lib, name):
    from parametron_jl_amd.lazyexpression import affine_stage_leaves
    h = Horizon(lib)
    node = h.dynamics(name, 2)
    leaves = affine_stage_leaves(node)
    kinds = {"x+": "vars", "A": "mat", "B": "mat", "w": "vec"}
    assert [(k, s) for k, _, s in leaves] == [(kinds[leaf], sign) for leaf, sign in U.SPELLINGS[name]]
    for (kind, d, _), (leaf, _) in zip(leaves, U.SPELLINGS[name]):
        if kind == "mat":
            assert d.mat is (h.A if leaf == "A" else h.B) and np.array_equal(d.xvars.vars, h.x(2) if leaf == "A" else h.u(2))
        elif kind == "vars":
            assert np.array_equal(d.vars, h.x(3))
    # nothing below the record was asked for its terms, and nothing was allocated for them
    assert not node.out.need_terms and node.out.terms is None
    assert max(h.ctx.allocs) <= 8 * max(h.nx * h.nx, 16)


def test_leaves_refuse_what_the_kernel_does_not_take(lib):
    import scipy.sparse as sp
    from parametron_jl_amd.device import DAffVec, DDenseAff, DMat, DSparseAff, DSpMat, DVars
    from parametron_jl_amd.lazyexpression import affine_stage_leaves
    h = Horizon(lib)
    Ax, Bu, xp, w = h.product(h.A, h.x(0)), h.product(h.B, h.u(0)), h.variables(h.x(1)), h.numbers()
    assert affine_stage_leaves(((w - Ax) - Bu - xp).node) is None                       # the number vector is the leftmost leaf
    assert affine_stage_leaves((w - (Ax + Bu)).node) is None
    scaled = h.operand(DAffVec(h.ctx, h.nx, row_len=h.nx))                               # dt*(A*x): a materialised vector
    assert affine_stage_leaves((xp - scaled - Bu).node) is None
    assert affine_stage_leaves((xp - Ax - w - h.numbers()).node) is None               # two number vectors
    pattern = sp.csc_matrix(np.eye(h.nx))
    sparse = h.operand(DSparseAff(h.ctx, DSpMat(h.ctx, pattern), DVars.of_indices(h.ctx, h.x(0)), None, 0))
    assert affine_stage_leaves((xp - sparse - Bu).node) is None
    nine = xp
    for k in range(8):
        nine = nine - h.product(DMat(h.ctx, h.nx, 1), np.array([100 + k]))
        assert (affine_stage_leaves(nine.node) is None) == (k == 7)                    # 2 .. 8 leaves pass, the ninth does not
    # implicit blocks on their own are no sums: they keep their packs
    assert affine_stage_leaves((Ax - w).node) is None and affine_stage_leaves(h.bound(0)) is None and affine_stage_leaves(Ax.node) is None
    assert isinstance((Ax - w).node.out, DDenseAff)
    # .. but as operands of a sum they are two leaves each
    fused = affine_stage_leaves((xp - (Ax - w)).node)
    assert [(k, s) for k, _, s in fused] == [("vars", 1), ("mat", -1), ("vec", 1)]
    assert affine_stage_leaves(np.zeros(3)) is None


# ---- 5. the group decision
def test_group_threshold_and_gates(lib):
    from parametron_jl_amd import moi
    assert moi.AFFINE_STAGE_MIN_RECORDS == lib.PMT_QUAD_MAX_GROUPS + 1
    assert moi.affine_stage_group(Horizon(lib, T=8).records(NAMES), False, "moi") is None
    recs = Horizon(lib, T=9).records(NAMES)
    g = moi.affine_stage_group(recs, False, "moi")
    assert g is not None and [id(m) for m in g.members] == [id(r) for r in recs] and len(g.leaves) == 9
    assert moi.affine_stage_group(recs, True, "moi") is None                             # the small plan
    assert moi.affine_stage_group(recs, False, "device") is None and moi.affine_stage_group(recs, False, "host_csc") is None
    assert moi.affine_stage_group(Horizon(lib, T=9, shared=False).records(NAMES), False, "moi") is None     # no two records share a matrix
    assert moi.affine_stage_group([], False, "moi") is None


def test_group_keeps_ineligible_records_out_and_the_order(lib):
    from parametron_jl_amd import moi
    h = Horizon(lib, T=10)
    recs = h.records(NAMES[:2], bounds_every=3)
    from parametron_jl_amd.device import DAff
    obj = moi.Objective(h.model, h.node(DAff(h.ctx, 3)))                            # a record of another kind
    recs = [obj] + recs
    g = moi.affine_stage_group(recs, False, "moi")
    dyn = [r for r in recs if isinstance(r, moi.Constraint) and isinstance(r.set, moi.Zeros)]
    assert len(recs) == 15 and len(dyn) == 10 and [id(m) for m in g.members] == [id(r) for r in dyn]
    # a record over a node that somebody asked for its terms, and two records over one node, stay out
    dyn[4].expr.out.materialized()
    shared = moi.Constraint(h.model, dyn[7].expr, moi.Nonnegatives(h.nx))
    g = moi.affine_stage_group(recs + [shared], False, "moi")
    assert g is None                                                                # eight are left
    h = Horizon(lib, T=12)
    recs = h.records(NAMES)
    recs[4].expr.out.materialized()
    g = moi.affine_stage_group(recs + [moi.Constraint(h.model, recs[7].expr, moi.Nonnegatives(h.nx))], False, "moi")
    assert [id(m) for m in g.members] == [id(r) for k, r in enumerate(recs) if k not in (4, 7)]


def _compile_all(lib, h, recs, group):
    from parametron_jl_amd.lazyexpression import schedule
    for r in recs:
        r.stage_group = None
    for r in (group.members if group else ()):
        r.stage_group = group
    ctx = h.ctx
    mark = len(ctx.allocs)
    emitters = [r.compile(ctx, VARMAP_BUF, None) for r in recs]
    allocs = ctx.allocs[mark:]
    ctx.calls = []
    for _ in range(2):
        for x in schedule([r.expr for r in recs]):
            x.emit(ctx)
        for e in emitters:
            e(ctx)
    return emitters, allocs


def test_compiled_group_is_one_call_two_arenas_two_fetches(lib):
    from parametron_jl_amd import moi
    T, nx, nu = 9, 4, 2
    h = Horizon(lib, T=T, nx=nx, nu=nu)
    recs = h.records(NAMES, bounds_every=4)                       # bounds before stages 0, 4, 8
    group = moi.affine_stage_group(recs, False, "moi")
    _, allocs = _compile_all(lib, h, recs, group)
    L = 1 + nx + nu
    nterms, nconsts, nparts = T * nx * L, T * nx, 3 * T
    bounds = [24 * nx, 8 * nx]
    assert allocs == bounds + [24 * nterms, 8 * nconsts, 48 * T, 32 * nparts] + bounds * 2
    per_update = [("pmt_vars_addsub_f64", (nx, -1, 0)), ("pmt_affine_stages_f64", (T,))] + [("pmt_vars_addsub_f64", (nx, -1, 0))] * 2
    assert h.ctx.calls == per_update * 2                          # nothing of the grouped records' nodes is emitted; update! allocates nothing
    assert len(h.ctx.allocs) - len(allocs) == len(h.ctx.allocs[:-len(allocs)])
    dyn = group.members
    base_t, base_c = group.terms_host.ctypes.data, group.consts_host.ctypes.data
    assert len(group.terms_host) == nterms and len(group.consts_host) == nconsts
    for k, r in enumerate(dyn):
        assert r.f.terms.ctypes.data == base_t + 24 * k * nx * L and len(r.f.terms) == nx * L
        assert r.f.constants.ctypes.data == base_c + 8 * k * nx and len(r.f.constants) == nx
        assert r.dev == {"terms": group.dev["terms"] + 24 * k * nx * L, "consts": group.dev["consts"] + 8 * k * nx}
        assert [key for _, key in r.buffers] == ["terms", "consts"] and not r.side_lane_ok
        assert not r.expr.out.need_terms
    # two fetches for the whole group, on both paths
    for r in recs:
        r.fetch(h.ctx)
    grouped = [(a, d, n) for a, d, n in h.ctx.fetched if d in (group.dev["terms"], group.dev["consts"])]
    assert grouped == [(base_t, group.dev["terms"], 24 * nterms), (base_c, group.dev["consts"], 8 * nconsts)]
    assert len(h.ctx.fetched) == 2 + 2 * 3
    for r in recs:
        r.record_fetch(h.ctx)
    assert len(h.ctx.recorded) == 2 + 2 * 3 and (base_t, group.dev["terms"], 24 * nterms) in h.ctx.recorded


def test_the_same_records_without_the_group_keep_their_chains(lib):
    """the plan every record had before: per record two assembles, two combines and the pack, its own buffers and two fetches"""
    T, nx, nu = 9, 4, 2
    h = Horizon(lib, T=T, nx=nx, nu=nu)
    recs = h.records(NAMES[:1])
    _compile_all(lib, h, recs, None)
    names = [c[0] for c in h.ctx.calls]
    assert names.count("pmt_affine_assemble_f64") == 2 * 2 * T and names.count("pmt_affvec_combine_f64") == 2 * 2 * T
    assert names.count("pmt_pack_vector_affine_f64") == 2 * T and "pmt_affine_stages_f64" not in names
    for r in recs:
        r.fetch(h.ctx)
    assert len(h.ctx.fetched) == 2 * T and all(r.expr.out.need_terms for r in recs)


def test_group_refuses_a_table_the_check_refuses(lib):
    from parametron_jl_amd import moi
    h = Horizon(lib)
    recs = h.records(NAMES)
    group = moi.affine_stage_group(recs, False, "moi")
    h.A.lda = h.nx - 1                                             # ld < rows
    for r in group.members:
        r.stage_group = group
    with pytest.raises(lib.DimensionMismatch, match="affine_stages"):
        recs[0].compile(h.ctx, VARMAP_BUF, None)
