"""CPU-only: horizon stage costs sum_t transpose(x_t (+|-) v_t) * Q * (x_t (+|-) v_t) as one canonical node (pmt_quad_stages_f64, record mode
"canonical-stages").  The numpy restatement of the header's order against the oracle's literal sequence and against Python integers;
pmt_quad_stages_check and the entry point's refusals; the descriptor's layout in the header, ctypes and Julia; the quad_plan row; what one
compiled record allocates and calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import quad_stages_util as U
from test_quad_form_shift_host import _shifted
from test_record_tape_host import FAKE, VARMAP_BUF, StubContext, _b, _block, _form, _model, _objective, _quad_out

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- 1. the restatement against the oracle's sequence and against integers
@pytest.mark.parametrize("name,ns,signs,interleave", [
    ("horizon", [5, 3] * 5, [-1, 0] * 5, False),
    ("both-signs", [1, 2, 63, 64, 65, 2, 1, 3, 4], [1, -1, 0, -1, 1, 0, 0, -1, 1], False),
    ("interleaved", [4, 6, 2, 5, 3, 4, 4, 2, 6], [-1, 1, 0, -1, -1, 0, 1, -1, 0], True),
], ids=lambda v: v if isinstance(v, str) else "")
def test_restatement_equals_the_oracle_sequence(lib, name, ns, signs, interleave):
    """indices exactly, quadratic coefficients bit for bit, linear coefficients and the constant within the derived bounds (quad_stages_util)"""
    stages, varmap, nterms, nlin = U.make_stages(ns, signs, 4000 + len(ns), special=(name == "both-signs"), interleave=interleave)
    at, qt, oconst = U.oracle(stages, varmap)
    quad, lin, const = U.merged(stages, varmap)
    parts, _ = U.restate(stages, varmap)
    assert len(qt) == nterms == len(quad) and len(lin) == nlin
    # the oracle's canonical order is by MODEL variable; the varmap only renames
    assert np.array_equal(qt["row"], quad["row"]) and np.array_equal(qt["col"], quad["col"])
    assert np.array_equal(bits(qt["coeff"]), bits(quad["coeff"]))
    got, want = U.lin_by_var(lin), U.lin_by_var(at)
    assert set(want) <= set(got)
    for st, (_, l, _) in zip(stages, parts):
        b = U.lin_bound(st)
        for var, coeff, bound in zip(l["var"].tolist(), l["coeff"].tolist(), b.tolist()):
            assert abs(coeff - want.get(var, 0.0)) <= bound, (name, var)
        if st["sign"] and len(l) >= 63:                                            # not vacuous
            assert np.max(b) < 1e-9 * np.max(np.abs(l["coeff"]))
    cb = U.const_bound(stages, [p[2] for p in parts])
    assert abs(const - oconst) <= cb
    assert cb < 1e-9 * sum(abs(p[2]) for p in parts)                               # not vacuous


def test_restatement_on_exact_integer_data(lib):
    """small integers: every product and sum is exact, so the restatement equals Python integer arithmetic"""
    rng = np.random.default_rng(9)
    stages, qa, la = [], 0, 0
    sizes = [3, 70, 1, 5, 130, 2, 3, 3, 4, 6]
    start = 1
    for t, n in enumerate(sizes):
        Q = rng.integers(-4, 5, size=(n, n)).astype(np.float64)
        sign = (-1, 0, 1)[t % 3]
        v = rng.integers(-3, 4, size=n).astype(np.float64) if sign else None
        stages.append({"Q": Q, "xvar": np.arange(start, start + n, dtype=np.int64), "v": v, "sign": sign, "quad_at": qa, "lin_at": la})
        start, qa, la = start + n, qa + n * (n + 1) // 2, la + n
    varmap = np.arange(1, start, dtype=np.int64)[::-1].copy()
    parts, const = U.restate(stages, varmap)
    total = 0
    for st, (quad, lin, c) in zip(stages, parts):
        Qi = [[int(a) for a in row] for row in st["Q"]]
        n = len(Qi)
        ci = [0] * n if not st["sign"] else [st["sign"] * int(a) for a in st["v"]]
        want_lin = [sum((Qi[j][k] + Qi[k][j]) * ci[k] for k in range(n)) for j in range(n)]
        want_c = sum(ci[j] * Qi[j][k] * ci[k] for j in range(n) for k in range(n))
        assert [int(a) for a in lin["coeff"]] == want_lin and int(c) == want_c and c == float(want_c)
        k = 0
        for j in range(n):
            for kk in range(j, n):
                assert int(quad["coeff"][k]) == Qi[j][kk] + Qi[kk][j] and quad["row"][k] == varmap[st["xvar"][j] - 1] and quad["col"][k] == varmap[st["xvar"][kk] - 1]
                k += 1
        total += want_c
    assert const == float(total)
    # a plain stage contributes +0.0; no stage at all gives +0.0
    assert parts[1][2] == 0.0 and not np.signbit(parts[1][2]) and not np.any(np.signbit(parts[1][1]["coeff"]))
    assert U.restate([], varmap)[1] == 0.0


def test_constant_order_is_256_chains_then_the_tree():
    """600 stage constants of mixed magnitude: the restated order, written out again by hand"""
    import quad_form_shift_util as S
    c = np.array([(1.0 + t * 2.0 ** -50) * 3.0 ** (t % 7) for t in range(600)])
    red = [0.0] * 256
    for t in range(600):
        red[t % 256] = red[t % 256] + c[t]
    h = 128
    while h:
        for i in range(h):
            red[i] = red[i] + red[i + h]
        h //= 2
    assert S.chain_tree_sum(c) == red[0]


# ---- 2. pmt_quad_stages_check and the entry point without a device
def _table(lib, edit=None, n_stages=3):
    rows, qa, la = [], 0, 0
    for t in range(n_stages):
        n = 3 + t
        rows.append({"Q": FAKE, "ldq": n, "xvar": FAKE, "vec": FAKE if t % 2 == 0 else None, "n": n, "sign": -1 if t % 2 == 0 else 0,
                     "quad_at": qa, "lin_at": la})
        qa, la = qa + n * (n + 1) // 2, la + n
    for (t, field), value in (edit or {}).items():
        rows[t][field] = value
    return lib.quad_stages(rows), qa, la


def _check(lib, arr, T, nterms, nlin):
    lib.call("pmt_quad_stages_check", C.addressof(arr) if arr is not None else None, T, nterms, nlin)


def test_check_accepts_a_valid_table(lib):
    arr, nq, nl = _table(lib)
    _check(lib, arr, 3, nq, nl)
    _check(lib, arr, 3, nq + 5, nl + 2)
    _check(lib, arr, 0, 0, 0)
    _check(lib, None, 0, 0, 0)
    # slices in any order, with gaps, at odd offsets
    arr, _, _ = _table(lib, {(0, "quad_at"): 101, (0, "lin_at"): 50, (1, "quad_at"): 1, (1, "lin_at"): 0, (2, "quad_at"): 11, (2, "lin_at"): 9})
    _check(lib, arr, 3, 107, 53)
    # n at both ends of its range
    arr = lib.quad_stages([{"Q": FAKE, "ldq": 256, "xvar": FAKE, "n": 256, "sign": 0}, {"Q": FAKE, "ldq": 1, "xvar": FAKE, "n": 1, "quad_at": 32896, "lin_at": 256}])
    _check(lib, arr, 2, 32897, 257)


@pytest.mark.parametrize("edit", [{(1, "Q"): None}, {(2, "xvar"): None}, {(0, "sign"): 2}, {(1, "sign"): -2}, {(1, "sign"): 1}, {(2, "vec"): None}],
                         ids=["null-Q", "null-xvar", "sign-two", "sign-minus-two", "null-vec-plus", "null-vec-minus"])
def test_check_refuses_invalid_arguments(lib, edit):
    arr, nq, nl = _table(lib, edit)
    with pytest.raises(lib.ArgumentError, match="quad_stages"):
        _check(lib, arr, 3, nq, nl)


@pytest.mark.parametrize("edit,T,dq,dl", [
    ({(1, "n"): 0}, 3, 0, 0), ({(1, "n"): -1}, 3, 0, 0), ({(1, "n"): 257, (1, "ldq"): 300}, 3, 40000, 400), ({(2, "ldq"): 4}, 3, 0, 0),
    ({}, -1, 0, 0), ({}, 3, -1, 0), ({}, 3, 0, -1), ({(0, "quad_at"): -1}, 3, 0, 0), ({(0, "lin_at"): -1}, 3, 0, 0),
    ({(1, "quad_at"): 5}, 3, 0, 0), ({(2, "lin_at"): 6}, 3, 0, 0), ({(2, "quad_at"): 0}, 3, 0, 0), ({(1, "lin_at"): 0}, 3, 0, 0),
], ids=["n-zero", "n-negative", "n-257", "ldq-below-n", "T-negative", "quad-slice-past-the-end", "lin-slice-past-the-end", "quad-slice-below-zero",
        "lin-slice-below-zero", "quad-overlap-by-one", "lin-overlap-by-one", "quad-same-start", "lin-same-start"])
def test_check_refuses_dimension_mismatches(lib, edit, T, dq, dl):
    arr, nq, nl = _table(lib, edit)
    with pytest.raises(lib.DimensionMismatch, match="quad_stages"):
        _check(lib, arr, T, nq + dq, nl + dl)


def test_check_refuses_a_null_table(lib):
    with pytest.raises(lib.ArgumentError, match="quad_stages"):
        _check(lib, None, 2, 10, 10)


def _launch(lib, stages=FAKE, T=2, varmap=FAKE, quad=FAKE, lin=FAKE, consts=FAKE, const=FAKE):
    lib.call("pmt_quad_stages_f64", stages, T, varmap, quad, lin, consts, const, None)


@pytest.mark.parametrize("bad", [{"stages": None}, {"varmap": None}, {"quad": None}, {"lin": None}, {"consts": None}, {"const": None}, {"const": None, "T": 0}],
                         ids=["null-table", "null-varmap", "null-quad", "null-lin", "null-stage-consts", "null-const", "null-const-T0"])
def test_entry_point_refuses_null_pointers_before_any_device_call(lib, bad):
    with pytest.raises(lib.ArgumentError, match="quad_stages"):
        _launch(lib, **bad)


def test_entry_point_refuses_a_negative_stage_count(lib):
    with pytest.raises(lib.DimensionMismatch, match="quad_stages"):
        _launch(lib, T=-1)


# ---- 3. the descriptor: header, ctypes, Julia
def test_descriptor_layout_agrees_in_header_ctypes_and_julia(lib, tmp_path):
    import subprocess
    assert C.sizeof(lib.QuadStage) == 56 and lib.PMT_QUAD_STAGES_MAX_N == 256
    offsets = {name: getattr(lib.QuadStage, name).offset for name, _ in lib.QuadStage._fields_}
    assert offsets == {"Q": 0, "ldq": 8, "xvar": 16, "vec": 24, "n": 32, "sign": 36, "quad_at": 40, "lin_at": 48}
    hdr = open(os.path.join(ROOT, "include", "parametron_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} pmt_quad_stage;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [name for decl in body.split(";") for name in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert fields == [name for name, _ in lib.QuadStage._fields_]
    assert "#define PMT_QUAD_STAGES_MAX_N 256" in hdr
    # a C compiler agrees on the size and the offsets
    src = tmp_path / "stage.c"
    src.write_text('#include <stddef.h>\n#include "parametron_hip.h"\n_Static_assert(sizeof(pmt_quad_stage) == 56, "size");\n' +
                   "".join('_Static_assert(offsetof(pmt_quad_stage, %s) == %d, "%s");\n' % (k, v, k) for k, v in offsets.items()) +
                   "int main(void) { return 0; }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # Julia: the same fields in the same order with types of the same size
    jl = open(os.path.join(ROOT, "julia", "ParametronHIP.jl")).read()
    jfields = re.findall(r"^\s+(\w+)::(\w+)\s*$", re.search(r"struct QuadStage\n(.*?)\nend", jl, flags=re.S).group(1), flags=re.M)
    size = {"DevPtr": 8, "Int64": 8, "Int32": 4}
    assert [f for f, _ in jfields] == [name for name, _ in lib.QuadStage._fields_]
    assert [size[t] for _, t in jfields] == [C.sizeof(t) for _, t in lib.QuadStage._fields_]
    for name in ("pmt_quad_stages_check", "pmt_quad_stages_f64"):
        assert "(:%s, lib)" % name in jl and name in lib.SIGNATURES and hasattr(C.CDLL(lib.LIB_PATH), name)
    assert len(lib.SIGNATURES["pmt_quad_stages_f64"][1]) == 8 and len(lib.SIGNATURES["pmt_quad_stages_check"][1]) == 4


# ---- 4. the quad_plan row
def _horizon(stages=9, n=4, shared=2, shifted=True):
    """LsqTerm('form') list over disjoint consecutive vectors; the forms share `shared` weight matrices (the same DMat object) in turn"""
    from parametron_jl_amd.lazyexpression import LsqTerm
    mats = {}
    terms = []
    for t in range(stages):
        idx = np.arange(1 + t * n, 1 + (t + 1) * n)
        f = _shifted(n, idx) if shifted and t % 2 == 0 else _form(n, idx)
        f.mat = mats.setdefault(t % shared, f.mat)
        terms.append(LsqTerm("form", r=f))
    return terms


def _plan(terms, **args):
    from parametron_jl_amd.moi import quad_plan
    kw = dict(kind="quad", nq=1 << 20, is_objective=True, quadratic_mode="canonical", small=False, handoff="moi", varmap=None, sparse_sums=True)
    kw.update(args)
    return quad_plan(terms, False, **kw)


def test_plan_nine_stages_with_two_shared_matrices(lib):
    terms = _horizon()
    p = _plan(terms)
    assert p.mode == "canonical-stages" and not p.canonicalize and not p.gram_record
    assert p.gram is None and p.form is None and p.terms is None and p.groups is None
    assert [id(q) for q in p.stages] == [id(t.r) for t in terms]
    assert sorted(id(r) for r in p.operands()) == sorted(id(t.r) for t in terms)      # Model.initialize: every stage's form is named
    # plain stages only; one matrix for all; n = 256; 300 stages
    assert _plan(_horizon(shifted=False)).mode == "canonical-stages"
    assert _plan(_horizon(shared=1)).mode == "canonical-stages"
    assert _plan(_horizon(n=256)).mode == "canonical-stages"
    assert len(_plan(_horizon(stages=300)).stages) == 300
    # exactly at the row's threshold
    from parametron_jl_amd.moi import GROUPS_MIN_LITERAL_TERMS
    assert GROUPS_MIN_LITERAL_TERMS == 1 << 14 and _plan(terms, nq=1 << 14).mode == "canonical-stages"


def _edited(what):
    from parametron_jl_amd.lazyexpression import LsqTerm
    terms = _horizon()
    if what == "weighted":
        terms[3] = terms[3].scaled(2.0)
    elif what == "negated":
        terms[8] = terms[8].scaled(-1.0)
    elif what == "parameter-weight":
        terms[3] = terms[3].scaled(1.0, object())
    elif what == "linear":
        terms.append(LsqTerm("linear", xvars=terms[0].r.xvars, vec=_b(4)))
    elif what == "constant":
        terms.append(LsqTerm("constant", scale=2.0))
    elif what == "block":
        terms[4] = LsqTerm("block", r=_block(10, terms[4].r.xvars.vars, _b(10), -1))
    elif what == "overlap":
        terms[5].r.xvars.vars = terms[5].r.xvars.vars - 1
    elif what == "unsorted":
        terms[5].r.xvars.vars = terms[5].r.xvars.vars[::-1].copy()
    elif what == "same-vector-twice":
        terms[5].r.xvars.vars = terms[4].r.xvars.vars.copy()
    return terms


LITERAL, ROW7 = ("literal", False), ("literal", True)
FALLS = [
    ("eight stages", lambda: _horizon(stages=8), {}, ("canonical-groups", False)),
    ("nine distinct matrices", lambda: _horizon(shared=9), {}, ROW7),
    ("nq below 2^14", _horizon, dict(nq=(1 << 14) - 1), ROW7),
    ("small", _horizon, dict(small=True), ROW7),
    ("auto", _horizon, dict(quadratic_mode="auto"), LITERAL),
    ("literal", _horizon, dict(quadratic_mode="literal"), LITERAL),
    ("handoff device", _horizon, dict(handoff="device", varmap=np.arange(1, 40, dtype=np.int64)), ROW7),
    ("handoff host_csc", _horizon, dict(handoff="host_csc", varmap=np.arange(1, 40, dtype=np.int64)), ROW7),
    ("constraint", _horizon, dict(is_objective=False), ROW7),
    ("weighted stage", lambda: _edited("weighted"), {}, ROW7),
    ("negated stage", lambda: _edited("negated"), {}, ROW7),
    ("parameter weight", lambda: _edited("parameter-weight"), {}, ROW7),
    ("extra linear term", lambda: _edited("linear"), {}, ROW7),
    ("extra constant", lambda: _edited("constant"), {}, ROW7),
    ("a block among the stages", lambda: _edited("block"), {}, ROW7),
    ("overlapping vectors", lambda: _edited("overlap"), {}, ROW7),
    ("unsorted vector", lambda: _edited("unsorted"), {}, ROW7),
    ("one vector twice", lambda: _edited("same-vector-twice"), {}, ("canonical-groups", False)),      # eight groups: that row takes it, as today
    ("n = 257", lambda: _horizon(n=257), {}, ROW7),
]


@pytest.mark.parametrize("name,make,args,expected", FALLS, ids=[f[0].replace(" ", "-") for f in FALLS])
def test_plan_falls_to_todays_row(lib, name, make, args, expected):
    p = _plan(make(), **args)
    assert (p.mode, p.canonicalize) == expected and p.stages is None


def test_groups_layout_first_is_one_pass_with_the_same_results(lib):
    """GroupsLayout over many groups, in order and interleaved: dst_lin / dst_quad are every group's first variable in z, as one flatnonzero per
    group gives them"""
    rng = np.random.default_rng(2)
    for interleave in (False, True):
        stages, _, _, _ = U.make_stages(list(rng.integers(1, 9, size=40)), [0] * 40, 77, interleave=interleave)
        lay = lib.GroupsLayout([st["xvar"] for st in stages])
        first = np.array([int(np.flatnonzero(lay.owner == g)[0]) for g in range(40)], dtype=np.int64)
        assert np.array_equal(lay.dst_lin, first) and np.array_equal(lay.dst_quad, lay.row_dst[first] // 3)
        assert lay.dst_lin.dtype == np.int64 and lay.ordered == (not interleave)


# ---- 5. one compiled record on the stub context
def _record(lib, forms):
    from parametron_jl_amd.moi import QuadPlan
    rec = _objective(_model(), _quad_out(7, 7), QuadPlan("canonical-stages", stages=forms))
    ctx = StubContext(lib)
    return rec, ctx, rec.compile(ctx, VARMAP_BUF, None)


def test_record_ordered_layout_is_one_call(lib):
    T, n = 10, 5
    forms = [t.r for t in _horizon(stages=T, n=n)]
    rec, ctx, emit = _record(lib, forms)
    nq, nl = T * n * (n + 1) // 2, T * n
    assert ctx.allocs == [24 * nq, 16 * nl, 8, 8 * T, 56 * T]
    assert rec.groups_ordered is True and set(rec.dev) == {"quad", "lin", "const"}
    assert len(rec.f.quadratic_terms) == nq and len(rec.f.affine_terms) == nl
    assert [k for _, k in rec.buffers] == ["quad", "lin", "const"]
    mark = len(ctx.allocs)
    emit(ctx)
    emit(ctx)
    assert len(ctx.allocs) == mark                                              # update! allocates nothing
    assert ctx.calls == [("pmt_quad_stages_f64", (T,))] * 2
    assert max(ctx.allocs) == 24 * nq                                           # no literal-sized buffer anywhere


def test_record_interleaved_layout_is_the_call_plus_the_gather(lib):
    T, n = 9, 4
    forms = [t.r for t in _horizon(stages=T, n=n)]
    z = np.arange(1, T * n + 1).reshape(n, T).T                                  # stage t: t + 1, t + 1 + T, ..
    for f, idx in zip(forms, z):
        f.xvars.vars = idx.astype(np.int64)
    rec, ctx, emit = _record(lib, forms)
    nq, nl = T * n * (n + 1) // 2, T * n
    assert ctx.allocs == [24 * nq, 16 * nl, 8, 8 * T, 24 * nq, 16 * nl, 8 * nl, 8 * (nl + 1), 8 * nl, 56 * T]
    assert rec.groups_ordered is False
    mark = len(ctx.allocs)
    emit(ctx)
    emit(ctx)
    assert len(ctx.allocs) == mark
    assert ctx.calls == [("pmt_quad_stages_f64", (T,)), ("pmt_quad_groups_gather_f64", (nl, nq, nl))] * 2


def test_record_refuses_a_table_the_check_refuses(lib):
    """the table goes through pmt_quad_stages_check at compile: a stage the kernel cannot take never reaches the device"""
    forms = [t.r for t in _horizon(stages=9, n=4)]
    forms[3].mat.lda = 3                                                         # ldq < n
    with pytest.raises(lib.DimensionMismatch, match="quad_stages"):
        _record(lib, forms)
