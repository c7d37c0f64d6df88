"""CPU-only: horizon stage costs with weights, linear terms and constants beside the stages (pmt_quad_stages_terms_f64, record mode
"canonical-stages").  The numpy restatement of the header's order against the oracle's literal sequence and against exact fractions;
pmt_quad_stages_terms_check and the entry point's refusals; the descriptors' layouts in the header, ctypes and Julia; the quad_plan row;
what one compiled record allocates and calls."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import __graft_entry__ as entry
import quad_stages_terms_util as W
import quad_stages_util as U
import test_quad_stages_host as H
from test_quad_stages_host import _edited, _horizon
from test_record_tape_host import FAKE, VARMAP_BUF, StubContext, _b, _block, _model, _objective, _quad_out

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- 1. the restatement against the oracle's sequence and against exact arithmetic
def check_against_the_oracle(stages, consts, varmap, nterms, nlin):
    at, qt, oconst = W.oracle(stages, consts, varmap)
    quad, lin, const = W.merged(stages, consts, varmap)
    assert len(qt) == nterms == len(quad) and len(lin) == nlin
    assert np.array_equal(qt["row"], quad["row"]) and np.array_equal(qt["col"], quad["col"])
    want_q = dict(zip(zip(qt["row"].tolist(), qt["col"].tolist()), qt["coeff"].tolist()))
    want_l = U.lin_by_var(at)
    for st in stages:
        q, l, _ = W.restate_stage(st, varmap)
        qb = W.quad_bound(st)
        got = np.array([want_q[(r, c)] for r, c in zip(q["row"].tolist(), q["col"].tolist())])
        exact = qb == 0.0
        same = exact & ((q["coeff"] != 0.0) | (W.weight(st["W"]) > 0))               # (a zero under a negative weight: equal, its sign may differ)
        assert np.array_equal(bits(q["coeff"][same]), bits(got[same])) and np.array_equal(q["coeff"][exact], got[exact])
        assert np.all(np.abs(q["coeff"] - got) <= qb)
        assert np.max(qb) <= 1e-14 * abs(W.weight(st["W"])) * np.max(np.abs(st["Q"]))   # not vacuous: 4 * gamma_2 < 1e-14
        lb = W.lin_bound(st, U.restate_stage(st, varmap)[1]["coeff"])
        for var, coeff, bound in zip(l["var"].tolist(), l["coeff"].tolist(), lb.tolist()):
            assert abs(coeff - want_l.get(var, 0.0)) <= bound, var
        if st["sign"] and len(l) >= 63:
            assert np.max(lb) < 1e-9 * np.max(np.abs(l["coeff"]))
    cb = W.const_bound(stages, consts, varmap)
    assert abs(const - oconst) <= cb
    return const, oconst, cb


@pytest.mark.parametrize("n", [1, 2, 64, 65, 130])
@pytest.mark.parametrize("T,nconsts", [(9, 0), (12, 3), (9, 1)])
def test_restatement_equals_the_oracle_sequence(lib, n, T, nconsts):
    """indices exactly; quadratic coefficients bit for bit on the diagonal and for weights that are powers of two, otherwise within quad_bound;
    linear coefficients and the constant within the derived bounds (quad_stages_terms_util).  The weights 1.0, 0.5, -1.0, 3.0, 1/3 and
    Parameter values come round in turn; stages with and without a shift, every other one with a linear term"""
    signs = [(-1, 0, 1)[t % 3] for t in range(T)]
    stages, varmap, nterms, nlin = W.make_stages([n] * T, signs, 6000 + 10 * n + T, special=(T == 12))
    assert {st["W"] for st in stages} >= set(W.WEIGHTS[:6]) and any(st["lin"] for st in stages) and not all(st["lin"] for st in stages)
    consts = W.make_consts(nconsts)
    const, _, cb = check_against_the_oracle(stages, consts, varmap, nterms, nlin)
    if n >= 64:
        assert cb < 1e-9 * sum(abs(W.restate_stage(st, varmap)[2]) for st in stages)     # not vacuous


def test_half_everywhere_is_bit_for_bit_the_oracle_in_the_quadratic_terms(lib):
    """0.5 * (sum of stages): scaling by a power of two commutes with every rounding"""
    stages, varmap, nterms, nlin = W.make_stages([5, 70, 3, 130, 2, 64, 1, 9, 65], [-1, 0, 1] * 3, 808, weights=[(0.5, None)], lin_every=0)
    at, qt, _ = W.oracle(stages, [], varmap)
    quad, lin, _ = W.merged(stages, [], varmap)
    assert np.array_equal(qt.view(np.int64), quad.view(np.int64))
    assert all(np.all(W.quad_bound(st) == 0.0) for st in stages)
    # and so are -1.0 and -4.0 (no coefficient of this data is a zero, whose sign could differ)
    for w in (-1.0, -4.0):
        for st in stages:
            st["W"] = (w, None)
        assert np.all(W.merged(stages, [], varmap)[0]["coeff"] != 0.0)
        assert np.array_equal(W.oracle(stages, [], varmap)[1].view(np.int64), W.merged(stages, [], varmap)[0].view(np.int64))


def test_restatement_on_exact_data(lib):
    """small integers and weights that are small dyadic numbers: every product and sum is exact, so the restatement equals fractions"""
    rng = np.random.default_rng(19)
    weights = [(1.0, None), (0.5, None), (-1.0, None), (3.0, None), (0.25, 6.0), (-2.0, 0.5)]
    stages, qa, la, start = [], 0, 0, 1
    for t, n in enumerate([3, 70, 1, 5, 130, 2, 3, 3, 4, 6]):
        Q = rng.integers(-4, 5, size=(n, n)).astype(np.float64)
        sign = (-1, 0, 1)[t % 3]
        v = rng.integers(-3, 4, size=n).astype(np.float64) if sign else None
        lin = (weights[(t + 1) % 6] + (rng.integers(-5, 6, size=n).astype(np.float64),)) if t % 2 else None
        stages.append({"Q": Q, "xvar": np.arange(start, start + n, dtype=np.int64), "v": v, "sign": sign, "quad_at": qa, "lin_at": la,
                       "W": weights[t % 6], "lin": lin})
        start, qa, la = start + n, qa + n * (n + 1) // 2, la + n
    varmap = np.arange(1, start, dtype=np.int64)[::-1].copy()
    consts = [(3.0, None, None), (1.0, None, -7.0), (-0.5, 4.0, 3.0)]
    parts, const = W.restate(stages, consts, varmap)
    total = Fraction(0)
    for st, (quad, lin, c) in zip(stages, parts):
        Wt = Fraction(W.weight(st["W"]))
        Qi = [[int(a) for a in row] for row in st["Q"]]
        n = len(Qi)
        ci = [0] * n if not st["sign"] else [st["sign"] * int(a) for a in st["v"]]
        want_lin = [Wt * sum((Qi[j][k] + Qi[k][j]) * ci[k] for k in range(n)) for j in range(n)]
        if st["lin"] is not None:
            want_lin = [a + Fraction(W.weight(st["lin"])) * int(b) for a, b in zip(want_lin, st["lin"][2])]
        want_c = Wt * sum(ci[j] * Qi[j][k] * ci[k] for j in range(n) for k in range(n))
        assert [Fraction(float(a)) for a in lin["coeff"]] == want_lin and Fraction(c) == want_c
        k = 0
        for j in range(n):
            for kk in range(j, n):
                assert Fraction(float(quad["coeff"][k])) == Wt * (Qi[j][kk] + Qi[kk][j])
                assert quad["row"][k] == varmap[st["xvar"][j] - 1] and quad["col"][k] == varmap[st["xvar"][kk] - 1]
                k += 1
        total += want_c
    assert Fraction(const) == total + 3 - 7 + Fraction(-0.5) * 4 * 3
    # a plain stage under a negative weight: -0.0 where no linear term follows (the sign pmt_quad_gram_sum_f64 leaves), +0.0 under a positive one
    neg = dict(stages[1], W=(-1.0, None), lin=None)
    q, l, c = W.restate_stage(neg, varmap)
    assert np.all(np.signbit(l["coeff"])) and np.all(l["coeff"] == 0.0) and c == 0.0 and np.signbit(c)
    pos = dict(stages[1], W=(3.0, None), lin=None)
    assert not np.any(np.signbit(W.restate_stage(pos, varmap)[1]["coeff"]))
    # no stage at all: the constants onto 0.0
    assert W.restate([], consts[:2], varmap)[1] == -4.0


def test_a_unit_table_restates_the_unweighted_stages(lib):
    stages, varmap, nterms, nlin = W.make_stages([4, 66, 1, 9, 3, 2, 5, 7, 8], [-1, 0, 1] * 3, 3, weights=[(1.0, None)], lin_every=0, special=True)
    a, b = W.images(stages, [], varmap, nterms, nlin), U.images(stages, varmap, nterms, nlin)
    assert all(np.array_equal(bits(x) if x.dtype == np.float64 else x, bits(y) if y.dtype == np.float64 else y) for x, y in zip(a[:3], b[:3]))
    assert bits([a[3]])[0] == bits([b[3]])[0]


# ---- 2. pmt_quad_stages_terms_check and the entry point without a device
def _tables(lib, edit=None, n_stages=3, nconsts=2):
    rows, qa, la = [], 0, 0
    for t in range(n_stages):
        n = 3 + t
        rows.append({"Q": FAKE, "ldq": n, "xvar": FAKE, "vec": FAKE if t % 2 == 0 else None, "n": n, "sign": -1 if t % 2 == 0 else 0,
                     "quad_at": qa, "lin_at": la})
        qa, la = qa + n * (n + 1) // 2, la + n
    for (t, field), value in (edit or {}).items():
        rows[t][field] = value
    terms = lib.quad_stage_terms([{"scale": 0.5}, {"weight": FAKE, "lin_vec": FAKE, "lin_scale": -1.0}, {"lin_vec": FAKE, "lin_weight": FAKE}][:n_stages])
    consts = lib.quad_stage_consts([{"scale": 2.0}, {"value": FAKE, "weight": FAKE}][:nconsts])
    return lib.quad_stages(rows), terms, consts, qa, la


def _check(lib, arr, terms, T, consts, nconsts, nterms, nlin):
    adr = lambda a: C.addressof(a) if a is not None else None
    lib.call("pmt_quad_stages_terms_check", adr(arr), adr(terms), T, adr(consts), nconsts, nterms, nlin)


def test_check_accepts_valid_tables(lib):
    arr, terms, consts, nq, nl = _tables(lib)
    _check(lib, arr, terms, 3, consts, 2, nq, nl)
    _check(lib, arr, terms, 3, None, 0, nq + 5, nl + 2)
    _check(lib, None, None, 0, consts, 2, 0, 0)
    _check(lib, None, None, 0, None, 0, 0, 0)
    big = lib.quad_stage_consts([{"scale": float(i)} for i in range(32)])
    _check(lib, arr, terms, 3, big, 32, nq, nl)
    assert lib.PMT_QUAD_STAGES_MAX_CONSTS == 32
    # the defaults of the builders: weight 1, no Parameter, no linear term
    assert (terms[0].scale, terms[0].lin_scale, terms[0].weight, terms[0].lin_vec) == (0.5, 1.0, None, None) and consts[1].scale == 1.0


@pytest.mark.parametrize("edit", [{(1, "Q"): None}, {(2, "xvar"): None}, {(0, "sign"): 2}, {(1, "sign"): 1}, {(2, "vec"): None}],
                         ids=["null-Q", "null-xvar", "sign-two", "null-vec-plus", "null-vec-minus"])
def test_check_refuses_what_the_unweighted_check_refuses_as_invalid(lib, edit):
    arr, terms, consts, nq, nl = _tables(lib, edit)
    with pytest.raises(lib.ArgumentError, match="quad_stages"):
        _check(lib, arr, terms, 3, consts, 2, nq, nl)


@pytest.mark.parametrize("edit,T,dq,dl", [({(1, "n"): 0}, 3, 0, 0), ({(1, "n"): 257, (1, "ldq"): 300}, 3, 40000, 400), ({(2, "ldq"): 4}, 3, 0, 0), ({}, -1, 0, 0),
                                          ({}, 3, -1, 0), ({}, 3, 0, -1), ({(0, "quad_at"): -1}, 3, 0, 0), ({(1, "quad_at"): 5}, 3, 0, 0), ({(2, "lin_at"): 6}, 3, 0, 0)],
                         ids=["n-zero", "n-257", "ldq-below-n", "T-negative", "quad-slice-past-the-end", "lin-slice-past-the-end", "quad-slice-below-zero",
                              "quad-overlap-by-one", "lin-overlap-by-one"])
def test_check_refuses_what_the_unweighted_check_refuses_as_a_mismatch(lib, edit, T, dq, dl):
    arr, terms, consts, nq, nl = _tables(lib, edit)
    with pytest.raises(lib.DimensionMismatch, match="quad_stages"):
        _check(lib, arr, terms, T, consts, 2, nq + dq, nl + dl)


def test_check_refuses_null_tables_and_constant_counts(lib):
    arr, terms, consts, nq, nl = _tables(lib)
    with pytest.raises(lib.ArgumentError, match="quad_stages"):
        _check(lib, None, terms, 3, consts, 2, nq, nl)
    with pytest.raises(lib.ArgumentError, match="quad_stages_terms"):
        _check(lib, arr, None, 3, consts, 2, nq, nl)
    with pytest.raises(lib.ArgumentError, match="quad_stages_terms"):
        _check(lib, arr, terms, 3, None, 1, nq, nl)
    with pytest.raises(lib.ArgumentError, match="quad_stages_terms"):
        _check(lib, None, None, 0, None, 1, 0, 0)
    for bad in (-1, 33):
        with pytest.raises(lib.DimensionMismatch, match="quad_stages_terms"):
            _check(lib, arr, terms, 3, consts, bad, nq, nl)


def _launch(lib, stages=FAKE, terms=FAKE, T=2, consts=FAKE, nconsts=1, varmap=FAKE, quad=FAKE, lin=FAKE, sconsts=FAKE, const=FAKE):
    lib.call("pmt_quad_stages_terms_f64", stages, terms, T, consts, nconsts, varmap, quad, lin, sconsts, const, None)


@pytest.mark.parametrize("bad", [{"stages": None}, {"terms": None}, {"consts": None}, {"varmap": None}, {"quad": None}, {"lin": None}, {"sconsts": None},
                                 {"const": None}, {"const": None, "T": 0}, {"consts": None, "T": 0}],
                         ids=["null-table", "null-terms", "null-consts", "null-varmap", "null-quad", "null-lin", "null-stage-consts", "null-const",
                              "null-const-T0", "null-consts-T0"])
def test_entry_point_refuses_null_pointers_before_any_device_call(lib, bad):
    with pytest.raises(lib.ArgumentError, match="quad_stages_terms"):
        _launch(lib, **bad)


@pytest.mark.parametrize("bad", [{"T": -1}, {"nconsts": -1}], ids=["T", "nconsts"])
def test_entry_point_refuses_negative_counts(lib, bad):
    with pytest.raises(lib.DimensionMismatch, match="quad_stages_terms"):
        _launch(lib, **bad)


# ---- 3. the descriptors: header, ctypes, Julia
def test_descriptor_layouts_agree_in_header_ctypes_and_julia(lib, tmp_path):
    import subprocess
    assert C.sizeof(lib.QuadStageTerms) == 40 and C.sizeof(lib.QuadStageConst) == 24 and C.sizeof(lib.QuadStage) == 56
    hdr = open(os.path.join(ROOT, "include", "parametron_hip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "ParametronHIP.jl")).read()
    checks = []
    for cname, cls, jname in (("pmt_quad_stage_terms", lib.QuadStageTerms, "QuadStageTerms"), ("pmt_quad_stage_const", lib.QuadStageConst, "QuadStageConst")):
        offsets = {name: getattr(cls, name).offset for name, _ in cls._fields_}
        assert list(offsets.values()) == list(range(0, C.sizeof(cls), 8))
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % cname, hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [m for decl in body.split(";") for m in re.findall(r"\*?\s*(\w+)\s*$", decl.strip())]
        assert fields == [name for name, _ in cls._fields_]
        checks.append('_Static_assert(sizeof(%s) == %d, "size");\n' % (cname, C.sizeof(cls)) +
                      "".join('_Static_assert(offsetof(%s, %s) == %d, "%s");\n' % (cname, k, v, k) for k, v in offsets.items()))
        jfields = re.findall(r"^\s+(\w+)::(\w+)\s*$", re.search(r"struct %s\n(.*?)\nend" % jname, jl, flags=re.S).group(1), flags=re.M)
        assert [f for f, _ in jfields] == [name for name, _ in cls._fields_]
        assert [{"DevPtr": 8, "Float64": 8}[t] for _, t in jfields] == [C.sizeof(t) for _, t in cls._fields_]
    assert "#define PMT_QUAD_STAGES_MAX_CONSTS 32" in hdr
    src = tmp_path / "terms.c"
    src.write_text('#include <stddef.h>\n#include "parametron_hip.h"\n' + "".join(checks) + "int main(void) { return 0; }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for name in ("pmt_quad_stages_terms_check", "pmt_quad_stages_terms_f64"):
        assert "(:%s, lib)" % name in jl and name in lib.SIGNATURES and hasattr(C.CDLL(lib.LIB_PATH), name)
    assert len(lib.SIGNATURES["pmt_quad_stages_terms_f64"][1]) == 11 and len(lib.SIGNATURES["pmt_quad_stages_terms_check"][1]) == 7


# ---- 4. the quad_plan row
def _plan(terms, **args):
    """test_quad_stages_host._plan as Model calls quad_plan: with stage_terms=True"""
    args.setdefault("stage_terms", True)
    return H._plan(terms, **args)


class _Scalar:
    """the device mirror of a scalar Parameter, as far as the plan and compile read it"""
    buf = FAKE


def _linear(form_term, scale=1.0, param=None):
    from parametron_jl_amd.lazyexpression import LsqTerm
    return LsqTerm("linear", scale=scale, param=param, xvars=form_term.r.xvars, vec=_b(len(form_term.r.xvars.vars)))


def test_plan_half_of_the_sum(lib):
    terms = [t.scaled(0.5) for t in _horizon()]
    p = _plan(terms)
    assert p.mode == "canonical-stages" and not p.canonicalize and not p.gram_record
    assert [id(q) for q in p.stages] == [id(t.r) for t in terms] and p.stage_consts == []
    assert [(s.scale, s.param, s.lin) for s in p.stage_terms] == [(0.5, None, None)] * 9
    assert sorted(id(r) for r in p.operands()) == sorted(id(t.r) for t in terms)


def test_plan_parameter_weights_negated_stages_linear_terms_and_constants(lib):
    from parametron_jl_amd.lazyexpression import LsqTerm
    terms = _horizon(stages=10)
    rho, gam, s = _Scalar(), _Scalar(), _Scalar()
    terms[1] = terms[1].scaled(1.0, rho)
    terms[3] = terms[3].scaled(-1.0)
    terms[5] = terms[5].scaled(0.25, gam)
    forms = list(terms)
    lin1, lin7 = _linear(forms[1], 2.0), _linear(forms[7], -1.0, gam)
    k0, k1 = LsqTerm("constant", scale=3.5), LsqTerm("constant", value=s).scaled(0.5, rho)
    full = forms[:4] + [lin7, k0] + forms[4:] + [lin1, k1]                        # linear terms and constants anywhere in the list
    p = _plan(full)
    assert p.mode == "canonical-stages" and [id(q) for q in p.stages] == [id(t.r) for t in forms]
    got = [(t.scale, t.param, t.lin) for t in p.stage_terms]
    want = [(1.0, None, None)] * 10
    want[1], want[3], want[5], want[7] = (1.0, rho, lin1), (-1.0, None, None), (0.25, gam, None), (1.0, None, lin7)
    assert got == want
    assert p.stage_consts == [k0, k1] and (k1.scale, k1.param, k1.value) == (0.5, rho, s)
    # 32 constants are the most
    assert _plan(forms + [k0] * 32).mode == "canonical-stages" and len(_plan(forms + [k0] * 32).stage_consts) == 32
    assert (_plan(forms + [k0] * 33).mode, _plan(forms + [k0] * 33).canonicalize) == ("literal", True)
    # the lists the row refused before this round
    for what in ("weighted", "negated", "linear", "constant"):
        q = _plan(_edited(what))
        assert q.mode == "canonical-stages" and len(q.stages) == 9, what
    q = _plan(_edited("parameter-weight"))
    assert q.mode == "canonical-stages" and q.stage_terms[3].param is not None and q.stage_terms[3].scale == 1.0


def test_plan_without_the_keyword_is_the_row_as_it_was(lib):
    """quad_plan's stage_terms defaults to False: a caller that does not ask gets the unweighted row only; Model asks"""
    import inspect
    from parametron_jl_amd import model, moi
    for what in ("weighted", "negated", "parameter-weight", "linear", "constant"):
        p = H._plan(_edited(what))
        assert (p.mode, p.canonicalize) == ("literal", True) and p.stages is None, what
    p = H._plan(_horizon())
    assert p.mode == "canonical-stages" and p.stage_terms is None and p.stage_consts == []
    assert inspect.signature(moi.quad_plan).parameters["stage_terms"].default is False
    assert "stage_terms=True" in inspect.getsource(model.Model._plan_quadratic_records)


def test_plan_unit_weights_is_the_unweighted_plan(lib):
    terms = [t.scaled(1.0) for t in _horizon()]
    p = _plan(terms)
    assert p.mode == "canonical-stages" and p.stage_terms is None and p.stage_consts == []
    p = _plan([t.scaled(-1.0).scaled(-1.0) for t in _horizon()])
    assert p.stage_terms is None


def _out_of_scope(what):
    from parametron_jl_amd.lazyexpression import LsqTerm
    terms = _horizon()
    f0 = terms[0]
    if what == "diag":
        terms.append(LsqTerm("diag", xvars=f0.r.xvars))
    elif what == "block":
        terms[4] = LsqTerm("block", r=_block(10, terms[4].r.xvars.vars, _b(10), -1)).scaled(0.5)
    elif what == "block-beside":
        terms.append(LsqTerm("block", r=_block(10, np.arange(100, 104), _b(10), -1)))
    elif what == "linear-over-part":
        t = _linear(f0)
        t.xvars = type(t.xvars).__new__(type(t.xvars))
        t.xvars.vars = f0.r.xvars.vars[:3].copy()
        terms.append(t)
    elif what == "linear-over-foreign":
        t = _linear(f0)
        t.xvars = type(t.xvars).__new__(type(t.xvars))
        t.xvars.vars = np.arange(200, 204, dtype=np.int64)
        terms.append(t)
    elif what == "linear-across-two-stages":
        t = _linear(f0)
        t.xvars = type(t.xvars).__new__(type(t.xvars))
        t.xvars.vars = np.concatenate([f0.r.xvars.vars[2:], terms[1].r.xvars.vars[:2]])
        terms.append(t)
    elif what == "two-linear-on-one-stage":
        terms += [_linear(f0), _linear(f0, 2.0)]
    elif what == "sparse-form":
        from parametron_jl_amd.lazyexpression import SparseQuadForm
        terms[2].r = SparseQuadForm.__new__(SparseQuadForm)
        terms[2].r.xvars = f0.r.xvars
    elif what == "host-scaled":
        terms.append(LsqTerm("diag", scale=2.0, xvars=f0.r.xvars, host_scaled=True))
    elif what == "weighted-n-257":
        terms = [t.scaled(0.5) for t in _horizon(n=257)]
    elif what == "weighted-distinct-matrices":
        terms = [t.scaled(0.5) for t in _horizon(shared=9)]
    elif what == "weighted-unsorted":
        terms = [t.scaled(0.5) for t in _edited("unsorted")]
    elif what == "weighted-overlap":
        terms = [t.scaled(0.5) for t in _edited("overlap")]
    return terms


@pytest.mark.parametrize("what", ["diag", "block", "block-beside", "linear-over-part", "linear-over-foreign", "linear-across-two-stages",
                                  "two-linear-on-one-stage", "sparse-form", "host-scaled", "weighted-n-257", "weighted-distinct-matrices",
                                  "weighted-unsorted", "weighted-overlap"])
def test_plan_out_of_scope_lists_keep_the_literal_path(lib, what):
    p = _plan(_out_of_scope(what))
    assert (p.mode, p.canonicalize) == ("literal", True) and p.stages is None and p.stage_terms is None


@pytest.mark.parametrize("args,expected", [(dict(nq=(1 << 14) - 1), ("literal", True)), (dict(small=True), ("literal", True)),
                                           (dict(quadratic_mode="auto"), ("literal", False)), (dict(quadratic_mode="literal"), ("literal", False)),
                                           (dict(handoff="device", varmap=np.arange(1, 40, dtype=np.int64)), ("literal", True)),
                                           (dict(is_objective=False), ("literal", True))],
                         ids=["nq-below-2^14", "small", "auto", "literal", "handoff-device", "constraint"])
def test_plan_other_conditions_are_untouched(lib, args, expected):
    from parametron_jl_amd.lazyexpression import LsqTerm
    terms = [t.scaled(0.5) for t in _horizon()] + [LsqTerm("constant", scale=1.0)]
    p = _plan(terms, **args)
    assert (p.mode, p.canonicalize) == expected and p.stages is None


def test_plan_eight_forms_are_still_canonical_groups(lib):
    from parametron_jl_amd.lazyexpression import LsqTerm
    terms = [t.scaled(0.5) for t in _horizon(stages=8)]
    terms += [_linear(terms[2], 2.0), LsqTerm("constant", scale=2.0)]
    p = _plan(terms)
    assert p.mode == "canonical-groups" and p.stages is None and len(p.groups) == 8


# ---- 5. one compiled record on the stub context
def _record(lib, plan):
    rec = _objective(_model(), _quad_out(7, 7), plan)
    ctx = StubContext(lib)
    return rec, ctx, rec.compile(ctx, VARMAP_BUF, None)


def test_record_with_terms_is_one_call_of_the_new_entry_point(lib):
    from parametron_jl_amd.lazyexpression import LsqTerm
    T, n = 10, 5
    terms = [t.scaled(0.5) for t in _horizon(stages=T, n=n)]
    terms[2] = terms[2].scaled(1.0, _Scalar())
    full = terms + [_linear(terms[4], 1.0, _Scalar()), LsqTerm("constant", value=_Scalar()), LsqTerm("constant", scale=2.0)]
    rec, ctx, emit = _record(lib, _plan(full))
    nq, nl = T * n * (n + 1) // 2, T * n
    assert ctx.allocs == [24 * nq, 16 * nl, 8, 8 * T, 56 * T, 40 * T, 24 * 2]
    assert rec.groups_ordered is True and set(rec.dev) == {"quad", "lin", "const"}
    mark = len(ctx.allocs)
    emit(ctx)
    emit(ctx)
    assert len(ctx.allocs) == mark                                              # update! allocates nothing
    assert ctx.calls == [("pmt_quad_stages_terms_f64", (T, 2))] * 2


def test_record_with_constants_only_takes_the_new_entry_point(lib):
    from parametron_jl_amd.lazyexpression import LsqTerm
    T, n = 9, 4
    rec, ctx, emit = _record(lib, _plan(_horizon(stages=T, n=n) + [LsqTerm("constant", scale=2.0)]))
    assert rec.plan.stage_terms is None and len(rec.plan.stage_consts) == 1
    emit(ctx)
    assert ctx.calls == [("pmt_quad_stages_terms_f64", (T, 1))] and ctx.allocs[-3:] == [56 * T, 40 * T, 24]


def test_record_interleaved_layout_keeps_the_gather(lib):
    T, n = 9, 4
    terms = [t.scaled(-1.0) for t in _horizon(stages=T, n=n)]
    z = np.arange(1, T * n + 1).reshape(n, T).T
    for t, idx in zip(terms, z):
        t.r.xvars.vars = idx.astype(np.int64)
    rec, ctx, emit = _record(lib, _plan(terms))
    nq, nl = T * n * (n + 1) // 2, T * n
    assert rec.groups_ordered is False
    emit(ctx)
    assert ctx.calls == [("pmt_quad_stages_terms_f64", (T, 0)), ("pmt_quad_groups_gather_f64", (nl, nq, nl))]


def test_record_of_unit_weights_makes_the_old_calls(lib):
    """a list of unit weights: the plan has no stage terms, and the compiled record allocates and calls exactly what it did before"""
    T, n = 10, 5
    rec, ctx, emit = _record(lib, _plan([t.scaled(1.0) for t in _horizon(stages=T, n=n)]))
    nq, nl = T * n * (n + 1) // 2, T * n
    assert ctx.allocs == [24 * nq, 16 * nl, 8, 8 * T, 56 * T]
    emit(ctx)
    assert ctx.calls == [("pmt_quad_stages_f64", (T,))]


def test_record_refuses_tables_the_check_refuses(lib):
    terms = [t.scaled(0.5) for t in _horizon(stages=9, n=4)]
    terms[3].r.mat.lda = 3                                                       # ldq < n
    with pytest.raises(lib.DimensionMismatch, match="quad_stages"):
        _record(lib, _plan(terms))
