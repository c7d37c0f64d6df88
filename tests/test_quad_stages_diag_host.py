"""CPU-only: horizon stage costs with identity-weighted terms (pmt_quad_stages_diag_f64; record mode "canonical-stages" with dot(u_t, u_t)
stages and ridge terms beside forms).  The numpy restatement of the header's order against the oracle's literal sequence;
pmt_quad_stages_diag_check and the entry point's refusals; the descriptor's layout in the header, ctypes and Julia; GroupsLayout with
diagonal sets; the quad_plan row with and without stage_diag; what one compiled record allocates and calls."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import quad_stages_diag_util as D
import quad_stages_terms_util as W
import quad_stages_util as U
import test_quad_stages_host as H
import test_quad_stages_terms_host as HT
from test_quad_stages_host import _horizon
from test_record_tape_host import FAKE, VARMAP_BUF, StubContext, _b, _model, _objective, _quad_out

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- 1. the restatement against the oracle's sequence
KINDS = ["f-", "i0", "f0r0", "i-", "f+r-", "i+", "f-r+", "f0", "i0", "f0r+", "i-", "f-r0"]


@pytest.mark.parametrize("n", [1, 2, 64, 65, 130])
@pytest.mark.parametrize("nconsts", [0, 2])
def test_restatement_equals_the_oracle_sequence(lib, n, nconsts):
    """twelve stages of every kind; indices exactly; identity stages: quadratic words bit for bit, linear words bit for bit unless the stage has
    both a vector and a linear term (then within ident_lin_bound); a rider's diagonal words bit for bit, its other words and every constant
    within the derived bounds (quad_stages_diag_util)"""
    stages, varmap, nterms, nlin = D.make_stages([n] * 12, KINDS, 9000 + n, special=(nconsts == 2))
    consts = W.make_consts(nconsts)
    at, qt, oconst = D.oracle(stages, consts, varmap)
    quad, lin, const = D.merged(stages, consts, varmap)
    assert len(qt) == nterms == len(quad) and len(lin) == nlin
    assert nterms == sum(n if k[0] == "i" else n * (n + 1) // 2 for k in KINDS)
    assert np.array_equal(qt["row"], quad["row"]) and np.array_equal(qt["col"], quad["col"])
    want_q = dict(zip(zip(qt["row"].tolist(), qt["col"].tolist()), qt["coeff"].tolist()))
    want_l = U.lin_by_var(at)
    exact_lin = bounded_lin = 0
    for st in stages:
        q, l, _ = D.restate_stage(st, varmap)
        got_q = np.array([want_q[(r, c)] for r, c in zip(q["row"].tolist(), q["col"].tolist())])
        got_l = np.array([want_l.get(v, 0.0) for v in l["var"].tolist()])
        if D.is_identity(st):
            assert np.array_equal(bits(q["coeff"]), bits(got_q))
            assert np.all(q["coeff"] == 2 * W.weight(st["W"]))
            lb = D.ident_lin_bound(st)
            assert np.all(np.abs(l["coeff"] - got_l) <= lb)
            free = lb == 0.0
            if st["sign"] or st["lin"] is not None:                       # (with neither the oracle holds no term at all; the node +0.0)
                assert np.array_equal(l["coeff"][free], got_l[free])
                nz = free & (l["coeff"] != 0.0)
                assert np.array_equal(bits(l["coeff"][nz]), bits(got_l[nz]))
                exact_lin += int(np.count_nonzero(free))
            else:
                assert np.all(bits(l["coeff"]) == 0)
            bounded_lin += int(np.count_nonzero(~free))
            continue
        dj = q["row"] == q["col"]
        qb = W.quad_bound(st)
        assert np.all(np.abs(q["coeff"] - got_q) <= qb)
        if D.rider(st) is not None:
            nzd = dj & (q["coeff"] != 0.0)
            assert np.array_equal(q["coeff"][dj], got_q[dj]) and np.array_equal(bits(q["coeff"][nzd]), bits(got_q[nzd]))
            lb = D.rider_lin_bound(st, U.restate_stage(st, varmap)[1]["coeff"])
        else:
            lb = W.lin_bound(st, U.restate_stage(st, varmap)[1]["coeff"])
        assert np.all(np.abs(l["coeff"] - got_l) <= lb)
        if n >= 64 and (st["sign"] or (D.rider(st) or (0, 0, 0, 0))[3]):
            assert np.max(lb) < 1e-9 * np.max(np.abs(l["coeff"]))         # not vacuous
    assert exact_lin > 0 and bounded_lin > 0
    cb = D.const_bound(stages, consts, varmap)
    assert abs(const - oconst) <= cb
    assert cb < 1e-9 * sum(abs(D.restate_stage(st, varmap)[2]) for st in stages)                 # not vacuous


def test_signs_of_zero_in_an_identity_stage(lib):
    """without v the linear word is W_c*c_t[j] alone: -0.0 survives; with neither it is +0.0; the constant without v is +0.0 under any weight"""
    x = np.arange(1, 5, dtype=np.int64)
    vm = np.arange(1, 5, dtype=np.int64)
    st = {"Q": None, "xvar": x, "v": None, "sign": 0, "W": (-3.0, None), "lin": (1.0, None, np.array([-0.0, 0.0, 1.0, -2.0])), "diag": None}
    q, l, c = D.restate_stage(st, vm)
    assert np.array_equal(np.signbit(l["coeff"]), [True, False, False, True]) and bits([c])[0] == 0 and np.all(q["coeff"] == -6.0)
    q, l, c = D.restate_stage(dict(st, lin=None), vm)
    assert np.all(bits(l["coeff"]) == 0) and bits([c])[0] == 0
    v = np.array([0.0, -0.0, 1.5, -2.0])
    q, l, c = D.restate_stage(dict(st, lin=None, v=v, sign=-1), vm)
    assert np.array_equal(l["coeff"], -3.0 * (2 * (0.0 - v))) and c == -3.0 * 6.25
    assert np.array_equal(np.signbit(l["coeff"]), [True, True, False, True])       # -3 * 2 * (0.0 - (+-0.0)) = -3 * (+0.0) = -0.0


def test_a_table_without_diagonal_terms_restates_the_weighted_stages(lib):
    stages, varmap, nterms, nlin = D.make_stages([4, 66, 1, 9, 3, 2, 5, 7, 8], ["f-", "f0", "f+"] * 3, 3, special=True)
    a, b = D.images(stages, [], varmap, nterms, nlin), W.images(stages, [], varmap, nterms, nlin)
    assert all(np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in zip(a[:3], b[:3])) and bits([a[3]])[0] == bits([b[3]])[0]


# ---- 2. pmt_quad_stages_diag_check and the entry point without a device
def _tables(lib, edit=None, dedit=None, diags=True):
    """five stages: form (shifted) with a rider, identity shifted, form plain, identity plain, form with a rider without vector"""
    rows, qa, la = [], 0, 0
    for t in range(5):
        n = 3 + t
        ident = t % 2 == 1
        rows.append({"Q": None if ident else FAKE, "ldq": 0 if ident else n, "xvar": FAKE, "vec": FAKE if t < 2 else None, "n": n,
                     "sign": (-1, 1, 0, 0, 0)[t], "quad_at": qa, "lin_at": la})
        qa, la = qa + (n if ident else n * (n + 1) // 2), la + n
    for (t, field), value in (edit or {}).items():
        rows[t][field] = value
    drows = [{"scale": 2.0, "vec": FAKE, "sign": 1}, {}, {}, {}, {"weight": FAKE}]
    for (t, field), value in (dedit or {}).items():
        drows[t] = dict(drows[t], **{field: value})
    terms = lib.quad_stage_terms([{"scale": 0.5}, {"weight": FAKE}, {"lin_vec": FAKE}, {"lin_vec": FAKE, "scale": -1.0}, {}])
    consts = lib.quad_stage_consts([{"scale": 2.0}, {"value": FAKE, "weight": FAKE}])
    return lib.quad_stages(rows), terms, lib.quad_stage_diags(drows) if diags else None, consts, qa, la


def _check(lib, arr, terms, diags, T, consts, nconsts, nterms, nlin):
    adr = lambda a: C.addressof(a) if a is not None else None
    lib.call("pmt_quad_stages_diag_check", adr(arr), adr(terms), adr(diags), T, adr(consts), nconsts, nterms, nlin)


def test_check_accepts_valid_tables(lib):
    arr, terms, diags, consts, nq, nl = _tables(lib)
    assert nq == 6 + 4 + 15 + 6 + 28 and nl == 25
    _check(lib, arr, terms, diags, 5, consts, 2, nq, nl)
    _check(lib, arr, terms, None, 5, consts, 2, nq, nl)                   # no table: no stage has a rider
    _check(lib, arr, terms, diags, 5, None, 0, nq + 3, nl + 1)
    _check(lib, None, None, None, 0, None, 0, 0, 0)
    assert (diags[0].scale, diags[0].sign, diags[0].present, diags[1].present, diags[1].scale, diags[4].present) == (2.0, 1, 1, 0, 1.0, 1)
    # an identity stage's ldq is not looked at; a rider's fields are not looked at without `present`
    arr, terms, diags, consts, nq, nl = _tables(lib, {(1, "ldq"): -7}, {(2, "sign"): 9, (2, "present"): 0})
    _check(lib, arr, terms, diags, 5, consts, 2, nq, nl)


def test_check_counts_an_identity_stage_as_n_terms(lib):
    arr, terms, diags, consts, nq, nl = _tables(lib)
    with pytest.raises(lib.DimensionMismatch, match="quad_stages"):
        _check(lib, arr, terms, diags, 5, consts, 2, nq - 1, nl)
    with pytest.raises(lib.DimensionMismatch, match="quad_stages"):
        _check(lib, arr, terms, diags, 5, consts, 2, nq, nl - 1)
    # the stage behind an identity stage may start n terms behind it, and not one earlier
    arr, terms, diags, consts, nq, nl = _tables(lib, {(2, "quad_at"): 6 + 3})
    with pytest.raises(lib.DimensionMismatch, match="overlap"):
        _check(lib, arr, terms, diags, 5, consts, 2, nq, nl)
    # the unweighted and the weighted check still refuse a stage without a matrix
    arr, terms, diags, consts, nq, nl = _tables(lib)
    with pytest.raises(lib.ArgumentError, match="null matrix"):
        lib.call("pmt_quad_stages_check", C.addressof(arr), 5, 1000, 1000)
    with pytest.raises(lib.ArgumentError, match="null matrix"):
        lib.call("pmt_quad_stages_terms_check", C.addressof(arr), C.addressof(terms), 5, C.addressof(consts), 2, 1000, 1000)


@pytest.mark.parametrize("edit,dedit", [({}, {(1, "present"): 1}), ({}, {(0, "present"): 2}), ({}, {(2, "present"): -1}), ({}, {(0, "sign"): 2}),
                                        ({}, {(0, "sign"): -2}), ({}, {(4, "sign"): -1}), ({}, {(0, "vec"): None}), ({(1, "sign"): 2}, {}),
                                        ({(1, "vec"): None}, {}), ({(3, "xvar"): None}, {})],
                         ids=["rider-on-identity", "present-two", "present-negative", "rider-sign-two", "rider-sign-minus-two", "rider-null-vec-minus",
                              "rider-null-vec-plus", "identity-sign-two", "identity-null-vec", "identity-null-xvar"])
def test_check_refuses_invalid_arguments(lib, edit, dedit):
    arr, terms, diags, consts, nq, nl = _tables(lib, edit, dedit)
    with pytest.raises(lib.ArgumentError, match="quad_stages"):
        _check(lib, arr, terms, diags, 5, consts, 2, nq, nl)


@pytest.mark.parametrize("edit,T,dq,dl", [({(1, "n"): 0}, 5, 0, 0), ({(1, "n"): 257}, 5, 40000, 400), ({(2, "ldq"): 4}, 5, 0, 0), ({}, -1, 0, 0),
                                          ({}, 5, -1, 0), ({}, 5, 0, -1), ({(1, "quad_at"): -1}, 5, 0, 0), ({(1, "quad_at"): 5}, 5, 0, 0),
                                          ({(3, "lin_at"): 11}, 5, 0, 0)],
                         ids=["identity-n-zero", "identity-n-257", "ldq-below-n", "T-negative", "quad-slice-past-the-end", "lin-slice-past-the-end",
                              "quad-slice-below-zero", "identity-quad-overlap-by-one", "identity-lin-overlap-by-one"])
def test_check_refuses_mismatches(lib, edit, T, dq, dl):
    arr, terms, diags, consts, nq, nl = _tables(lib, edit)
    with pytest.raises(lib.DimensionMismatch, match="quad_stages"):
        _check(lib, arr, terms, diags, T, consts, 2, nq + dq, nl + dl)


def test_check_refuses_what_the_weighted_check_refuses_with_its_codes(lib):
    arr, terms, diags, consts, nq, nl = _tables(lib)
    with pytest.raises(lib.ArgumentError, match="quad_stages"):
        _check(lib, None, terms, diags, 5, consts, 2, nq, nl)
    with pytest.raises(lib.ArgumentError, match="quad_stages_terms"):
        _check(lib, arr, None, diags, 5, consts, 2, nq, nl)
    with pytest.raises(lib.ArgumentError, match="quad_stages_terms"):
        _check(lib, arr, terms, diags, 5, None, 1, nq, nl)
    for bad in (-1, 33):
        with pytest.raises(lib.DimensionMismatch, match="quad_stages_terms"):
            _check(lib, arr, terms, diags, 5, consts, bad, nq, nl)
    # the refusals of the weighted check on the same edits, code for code
    for edit in HT.test_check_refuses_what_the_unweighted_check_refuses_as_invalid.pytestmark[0].args[1][1:]:
        arr3, terms3, consts3, nq3, nl3 = HT._tables(lib, edit)
        with pytest.raises(lib.ArgumentError):
            _check(lib, arr3, terms3, None, 3, consts3, 2, nq3, nl3)


def _launch(lib, stages=FAKE, terms=FAKE, diags=FAKE, T=2, consts=FAKE, nconsts=1, varmap=FAKE, quad=FAKE, lin=FAKE, sconsts=FAKE, const=FAKE):
    lib.call("pmt_quad_stages_diag_f64", stages, terms, diags, T, consts, nconsts, varmap, quad, lin, sconsts, const, None)


@pytest.mark.parametrize("bad", [{"stages": None}, {"terms": None}, {"consts": None}, {"varmap": None}, {"quad": None}, {"lin": None}, {"sconsts": None},
                                 {"const": None}, {"const": None, "T": 0}, {"consts": None, "T": 0}, {"diags": None, "const": None}],
                         ids=["null-table", "null-terms", "null-consts", "null-varmap", "null-quad", "null-lin", "null-stage-consts", "null-const",
                              "null-const-T0", "null-consts-T0", "null-const-without-diags"])
def test_entry_point_refuses_null_pointers_before_any_device_call(lib, bad):
    with pytest.raises(lib.ArgumentError, match="quad_stages_diag"):
        _launch(lib, **bad)


@pytest.mark.parametrize("bad", [{"T": -1}, {"nconsts": -1}, {"nconsts": 33}], ids=["T", "nconsts", "nconsts-33"])
def test_entry_point_refuses_bad_counts(lib, bad):
    with pytest.raises(lib.DimensionMismatch, match="quad_stages_diag"):
        _launch(lib, **bad)


# ---- 3. the descriptor: header, ctypes, Julia
def test_descriptor_layout_agrees_in_header_ctypes_and_julia(lib, tmp_path):
    import subprocess
    cls = lib.QuadStageDiag
    assert C.sizeof(cls) == 32
    offsets = {name: getattr(cls, name).offset for name, _ in cls._fields_}
    assert offsets == {"scale": 0, "weight": 8, "vec": 16, "sign": 24, "present": 28}
    hdr = open(os.path.join(ROOT, "include", "parametron_hip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "ParametronHIP.jl")).read()
    body = re.search(r"typedef struct \{([^}]*)\} pmt_quad_stage_diag;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [m.strip(" *") for decl in body.split(";") for m in re.sub(r"^\s*(const\s+)?\w+\s+", "", decl.strip()).split(",") if m.strip()]
    assert fields == [name for name, _ in cls._fields_]
    jfields = re.findall(r"^\s+(\w+)::(\w+)\s*$", re.search(r"struct QuadStageDiag\n(.*?)\nend", jl, flags=re.S).group(1), flags=re.M)
    assert [f for f, _ in jfields] == [name for name, _ in cls._fields_]
    assert [{"DevPtr": 8, "Float64": 8, "Int32": 4}[t] for _, t in jfields] == [C.sizeof(t) for _, t in cls._fields_]
    src = tmp_path / "diag.c"
    src.write_text('#include <stddef.h>\n#include "parametron_hip.h"\n_Static_assert(sizeof(pmt_quad_stage_diag) == 32, "size");\n' +
                   "".join('_Static_assert(offsetof(pmt_quad_stage_diag, %s) == %d, "%s");\n' % (k, v, k) for k, v in offsets.items()) +
                   "int main(void) { return 0; }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for name in ("pmt_quad_stages_diag_check", "pmt_quad_stages_diag_f64"):
        assert "(:%s, lib)" % name in jl and name in lib.SIGNATURES and hasattr(C.CDLL(lib.LIB_PATH), name)
    assert len(lib.SIGNATURES["pmt_quad_stages_diag_f64"][1]) == 12 and len(lib.SIGNATURES["pmt_quad_stages_diag_check"][1]) == 8
    assert "csrc/gram_sum.hip" in re.search(r"identity-weighted stage costs.*?pmt_quad_stage_diag;", hdr, flags=re.S).group(0)


# ---- 4. GroupsLayout with diagonal sets
def _brute_layout(sets, diagonal):
    """every term of every group placed by hand: arena terms in group order (a diagonal group: its n terms; otherwise its triangle by rows);
    the destination rows by increasing variable.  -> (row_src, row_dst, nterms) in words"""
    arena, at = {}, 0
    for g, s in enumerate(sets):
        for j, v in enumerate(s):
            cnt = 1 if diagonal[g] else len(s) - j
            arena[v] = (at, cnt)
            at += cnt
    src, dst, pos = [], [0], 0
    for v in sorted(arena):
        src.append(3 * arena[v][0])
        pos += arena[v][1]
        dst.append(3 * pos)
    return np.array(src), np.array(dst), at


@pytest.mark.parametrize("interleaved", [False, True], ids=["in-order", "interleaved"])
def test_groups_layout_with_diagonal_sets(lib, interleaved):
    sizes, diagonal = [5, 3, 1, 4, 2, 6], [False, True, True, False, True, False]
    if interleaved:
        pool = iter(range(1, 100))
        sets = [[] for _ in sizes]
        for k in range(max(sizes)):
            for s, n in zip(sets, sizes):
                if k < n:
                    s.append(next(pool))
    else:
        start = np.concatenate([[1], 1 + np.cumsum(sizes)])
        sets = [list(range(start[g], start[g] + n)) for g, n in enumerate(sizes)]
    lay = lib.GroupsLayout(sets, diagonal=diagonal)
    src, dst, nterms = _brute_layout(sets, diagonal)
    assert np.array_equal(lay.row_src, src) and np.array_equal(lay.row_dst, dst) and lay.nterms == nterms == 15 + 3 + 1 + 10 + 2 + 21
    assert lay.nlin == sum(sizes) and lay.ordered == (not interleaved)
    assert np.array_equal(lay.src_quad, np.concatenate([[0], np.cumsum([n if d else n * (n + 1) // 2 for n, d in zip(sizes, diagonal)])[:-1]]))
    if not interleaved:
        assert np.array_equal(lay.dst_quad, lay.src_quad) and np.array_equal(lay.dst_lin, lay.src_lin)
    with pytest.raises(lib.ArgumentError, match="diagonal"):
        lib.GroupsLayout(sets, diagonal=[True])


def test_groups_layout_without_the_argument_is_what_it_was(lib):
    """array for array: no flag, None and all-False flags against the layout computed by hand from the documented formulas"""
    rng = np.random.default_rng(4)
    sizes = [4, 1, 7, 3]
    z = rng.permutation(np.arange(1, 40))[:sum(sizes)]
    sets = [np.sort(s) for s in np.split(z, np.cumsum(sizes)[:-1])]
    a, b, c = lib.GroupsLayout(sets), lib.GroupsLayout(sets, None), lib.GroupsLayout(sets, diagonal=[False] * 4)
    src, dst, nterms = _brute_layout([list(s) for s in sets], [False] * 4)
    assert np.array_equal(a.row_src, src) and np.array_equal(a.row_dst, dst) and a.nterms == nterms
    for name in ("z", "owner", "src_quad", "src_lin", "row_src", "row_dst", "lin_src", "dst_quad", "dst_lin"):
        x, y, w = getattr(a, name), getattr(b, name), getattr(c, name)
        assert x.dtype == y.dtype == w.dtype == np.int64 and np.array_equal(x, y) and np.array_equal(x, w), name
    assert (a.nterms, a.nlin, a.ordered) == (b.nterms, b.nlin, b.ordered) == (c.nterms, c.nlin, c.ordered)
    assert list(inspect.signature(lib.GroupsLayout.__init__).parameters) == ["self", "sets", "diagonal"]


# ---- 5. the quad_plan row
def _plan(terms, **args):
    """as Model calls quad_plan: stage_terms=True, stage_diag=True"""
    args.setdefault("stage_terms", True)
    args.setdefault("stage_diag", True)
    return H._plan(terms, **args)


class _Scalar:
    buf = FAKE


def _vars(idx):
    from parametron_jl_amd.lazyexpression import _IndexVars
    return _IndexVars(idx)


def _diag(idx, scale=1.0, param=None, vec=None, sign=0, host_scaled=False):
    from parametron_jl_amd.lazyexpression import LsqTerm
    return LsqTerm("diag", scale=scale, param=param, xvars=_vars(idx), vec=vec, sign=sign, host_scaled=host_scaled)


def _rho_horizon(stages=5, nx=4, nu=3, rho=None, scale=1.0):
    """sum_t form over x_t + rho * dot(u_t, u_t): `stages` forms sharing two matrices and as many identity stages"""
    forms = _horizon(stages=stages, n=nx)
    base = 1 + stages * nx
    out = []
    for t, f in enumerate(forms):
        out += [f, _diag(np.arange(base + t * nu, base + (t + 1) * nu), scale=scale, param=rho, host_scaled=rho is None and scale != 1.0)]
    return out


def test_plan_identity_stages(lib):
    rho = _Scalar()
    terms = _rho_horizon(rho=rho, scale=0.5)
    p = _plan(terms)
    assert p.mode == "canonical-stages" and not p.canonicalize and p.stage_diags is None and len(p.stages) == 10
    assert [q.mat is None for q in p.stages] == [False, True] * 5
    assert [id(q) for q in p.stages[::2]] == [id(t.r) for t in terms[::2]]
    assert all(np.array_equal(q.xvars.vars, t.xvars.vars) and q.vec is None and q.sign == 0 for q, t in zip(p.stages[1::2], terms[1::2]))
    assert [(s.scale, s.param) for s in p.stage_terms] == [(1.0, None), (0.5, rho)] * 5
    # a Python number as the weight (multiplied on the host), a shifted identity stage, a linear term on an identity stage
    p = _plan(_rho_horizon(scale=2.5))
    assert p.mode == "canonical-stages" and [s.scale for s in p.stage_terms] == [1.0, 2.5] * 5
    terms = _rho_horizon()
    terms[3] = _diag(terms[3].xvars.vars, vec=_b(3), sign=-1)
    from parametron_jl_amd.lazyexpression import LsqTerm
    lin = LsqTerm("linear", xvars=_vars(terms[5].xvars.vars), vec=_b(3))
    p = _plan(terms + [lin])
    assert p.mode == "canonical-stages" and p.stages[3].sign == -1 and p.stages[3].vec is terms[3].vec and p.stage_terms[5].lin is lin
    # stages are counted as vectors: 4 + 4 are eight, 5 + 4 nine; two forms reading one matrix are needed
    assert _plan(_rho_horizon(stages=4)).mode == "literal"
    assert _plan(_rho_horizon(stages=5)[:-1]).mode == "canonical-stages"
    one = _rho_horizon(stages=9)
    for k, t in enumerate(one[::2]):
        t.r.mat = type(t.r.mat).__new__(type(t.r.mat)) if k else t.r.mat
        if k:
            t.r.mat.cols = 4
    assert _plan(one).mode == "literal"


def test_plan_riders(lib):
    lam = _Scalar()
    terms = _horizon()
    r2 = _diag(terms[2].r.xvars.vars, scale=1.0, param=lam)
    r7 = _diag(terms[7].r.xvars.vars, scale=3.0, vec=_b(4), sign=1, host_scaled=False)
    p = _plan([r7] + terms + [r2])                                        # a rider may stand anywhere in the list
    assert p.mode == "canonical-stages" and [id(q) for q in p.stages] == [id(t.r) for t in terms]
    assert p.stage_diags == [None, None, r2, None, None, None, None, r7, None] and p.stage_terms is None and p.stage_consts == []
    # riders and identity stages in one list
    mixed = _rho_horizon()
    r0 = _diag(mixed[0].r.xvars.vars, scale=2.0, host_scaled=True)
    p = _plan(mixed + [r0])
    assert p.mode == "canonical-stages" and p.stage_diags == [r0] + [None] * 9 and p.stages[1].mat is None


def _literal_lists(what):
    terms = _rho_horizon()
    x0, u0, u1 = terms[0].r.xvars.vars, terms[1].xvars.vars, terms[3].xvars.vars
    if what == "part-of-a-form-stage":
        terms.append(_diag(x0[:2]))
    elif what == "part-of-an-identity-stage":
        terms.append(_diag(u0[1:]))
    elif what == "across-two-stages":
        terms.append(_diag(np.concatenate([u0[1:], u1[:1]])))
    elif what == "two-riders-on-one-vector":
        terms += [_diag(x0), _diag(x0, scale=2.0)]
    elif what == "two-diagonal-terms-on-one-identity-vector":
        terms.append(_diag(u0, scale=2.0))
    elif what == "unsorted-identity-vector":
        terms[1] = _diag(u0[::-1].copy())
    elif what == "identity-n-257":
        terms[1] = _diag(np.arange(1000, 1257))
    elif what == "empty-identity-vector":
        terms.append(_diag(np.zeros(0, dtype=np.int64)))
    elif what == "block-among-the-stages":
        terms = HT._out_of_scope("block-beside") + terms[1::2]
    elif what == "sparse-form":
        terms = HT._out_of_scope("sparse-form") + terms[1::2]
    return terms


@pytest.mark.parametrize("what", ["part-of-a-form-stage", "part-of-an-identity-stage", "across-two-stages", "two-riders-on-one-vector",
                                  "two-diagonal-terms-on-one-identity-vector", "unsorted-identity-vector", "identity-n-257", "empty-identity-vector",
                                  "block-among-the-stages", "sparse-form"])
def test_plan_lists_that_stay_literal(lib, what):
    p = _plan(_literal_lists(what))
    assert (p.mode, p.canonicalize) == ("literal", True) and p.stages is None and p.stage_diags is None


def test_plan_without_the_keyword_is_the_row_as_it_was(lib):
    from parametron_jl_amd import model, moi
    assert inspect.signature(moi.quad_plan).parameters["stage_diag"].default is False
    assert inspect.signature(moi._lsq_stages).parameters["diag"].default is False
    assert "stage_diag=True" in inspect.getsource(model.Model._plan_quadratic_records)
    assert "sparse_sums=True, stage_terms=True" in inspect.getsource(model.Model._plan_quadratic_records)
    for what in ("diag", "host-scaled"):
        p = HT._plan(HT._out_of_scope(what))                              # stage_terms=True alone: literal, as today
        assert (p.mode, p.canonicalize) == ("literal", True) and p.stages is None, what
        q = _plan(HT._out_of_scope(what))                                 # with the keyword: a rider on stage 0
        assert q.mode == "canonical-stages" and q.stage_diags[0] is not None and q.stage_diags[1:] == [None] * 8, what
    for terms in (_rho_horizon(), _rho_horizon(scale=2.0)):
        p = HT._plan(terms)
        assert (p.mode, p.canonicalize) == ("literal", True)
    assert len(moi._lsq_stages(_horizon())) == 3 and len(moi._lsq_stages(_horizon(), diag=True)) == 4
    assert moi._lsq_stages(_rho_horizon()) is None and moi._lsq_stages(_horizon(), diag=True)[3] is None
    # a horizon without diagonal terms plans as before with the keyword
    for terms in (_horizon(), [t.scaled(0.5) for t in _horizon()]):
        a, b = HT._plan(terms), _plan(terms)
        assert a.mode == b.mode == "canonical-stages" and b.stage_diags is None and [id(q) for q in a.stages] == [id(q) for q in b.stages]
        assert (a.stage_terms is None) == (b.stage_terms is None)


@pytest.mark.parametrize("args,expected", [(dict(nq=(1 << 14) - 1), ("literal", True)), (dict(small=True), ("literal", True)),
                                           (dict(quadratic_mode="auto"), ("literal", False)), (dict(quadratic_mode="literal"), ("literal", False)),
                                           (dict(handoff="device", varmap=np.arange(1, 60, dtype=np.int64)), ("literal", True)),
                                           (dict(is_objective=False), ("literal", True))],
                         ids=["nq-below-2^14", "small", "auto", "literal", "handoff-device", "constraint"])
def test_plan_other_conditions_are_untouched(lib, args, expected):
    p = _plan(_rho_horizon(rho=_Scalar()), **args)
    assert (p.mode, p.canonicalize) == expected and p.stages is None


# ---- 6. one compiled record on the stub context
def _record(lib, plan):
    rec = _objective(_model(), _quad_out(7, 7), plan)
    ctx = StubContext(lib)
    return rec, ctx, rec.compile(ctx, VARMAP_BUF, None)


def test_record_with_identity_stages_is_one_call_of_the_new_entry_point(lib):
    T, nx, nu = 6, 5, 3
    rec, ctx, emit = _record(lib, _plan(_rho_horizon(stages=T, nx=nx, nu=nu, rho=_Scalar())))
    nq, nl = T * (nx * (nx + 1) // 2 + nu), T * (nx + nu)
    # MOI buffers, the constant, the stage constants; an index buffer per identity stage; the stage table, the terms, the constants
    assert ctx.allocs == [24 * nq, 16 * nl, 8, 8 * 2 * T] + [8 * nu] * T + [56 * 2 * T, 40 * 2 * T, 24]
    assert rec.groups_ordered is True                                     # every vector is consecutive in z: slices, no gather
    mark = len(ctx.allocs)
    emit(ctx)
    emit(ctx)
    assert len(ctx.allocs) == mark                                        # update! allocates nothing
    assert ctx.calls == [("pmt_quad_stages_diag_f64", (2 * T, 0))] * 2
    name, args = ctx.raw[-1]
    assert name == "pmt_quad_stages_diag_f64" and getattr(args[2], "value", None) is None     # no rider: no third table


def test_record_interleaved_layout_keeps_the_gather(lib):
    T, nx, nu = 5, 4, 3
    terms = _rho_horizon(stages=T, nx=nx, nu=nu, scale=2.0)
    pool = iter(range(1, 100))
    vecs = [[] for _ in terms]
    for k in range(nx):
        for vec, n in zip(vecs, [nx, nu] * T):
            if k < n:
                vec.append(next(pool))
    for t, vec in zip(terms, vecs):
        (t.r.xvars if t.kind == "form" else t.xvars).vars = np.array(vec, dtype=np.int64)
    rec, ctx, emit = _record(lib, _plan(terms))
    nq, nl = T * (nx * (nx + 1) // 2 + nu), T * (nx + nu)
    assert rec.groups_ordered is False
    emit(ctx)
    assert ctx.calls == [("pmt_quad_stages_diag_f64", (2 * T, 0)), ("pmt_quad_groups_gather_f64", (nl, nq, nl))]


def test_record_in_stage_order_needs_no_gather_and_riders_get_their_table(lib):
    T, n = 9, 4
    terms = _horizon(stages=T, n=n)
    rid = _diag(terms[4].r.xvars.vars, scale=0.5, param=_Scalar(), vec=_b(n), sign=-1)
    rec, ctx, emit = _record(lib, _plan(terms + [rid]))
    nq, nl = T * n * (n + 1) // 2, T * n
    assert ctx.allocs == [24 * nq, 16 * nl, 8, 8 * T, 56 * T, 40 * T, 24, 32 * T] and rec.groups_ordered is True
    emit(ctx)
    assert ctx.calls == [("pmt_quad_stages_diag_f64", (T, 0))]
    assert getattr(ctx.raw[-1][1][2], "value", None) is not None


def test_records_without_diagonal_terms_make_the_calls_they_made(lib):
    T, n = 10, 5
    rec, ctx, emit = _record(lib, _plan(_horizon(stages=T, n=n)))
    nq, nl = T * n * (n + 1) // 2, T * n
    assert ctx.allocs == [24 * nq, 16 * nl, 8, 8 * T, 56 * T]
    emit(ctx)
    assert ctx.calls == [("pmt_quad_stages_f64", (T,))]
    rec, ctx, emit = _record(lib, _plan([t.scaled(0.5) for t in _horizon(stages=T, n=n)]))
    assert ctx.allocs == [24 * nq, 16 * nl, 8, 8 * T, 56 * T, 40 * T, 24]
    emit(ctx)
    assert ctx.calls == [("pmt_quad_stages_terms_f64", (T, 0))]


def test_record_refuses_tables_the_check_refuses(lib):
    terms = _rho_horizon(stages=5)
    terms[2].r.mat.lda = 3                                                # ldq < n
    with pytest.raises(lib.DimensionMismatch, match="quad_stages"):
        _record(lib, _plan(terms))
