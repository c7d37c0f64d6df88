"""CPU-only: which sums over several Variable vectors become "canonical-groups" (moi.quad_plan, the row behind "canonical-sum"), how their
terms are dealt out to the groups, where the groups' functions stand in the function over the union (_lib.GroupsLayout), and the argument
checks of pmt_quad_groups_gather_f64 / pmt_quad_groups_constant_f64 — on device values built without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
from test_stacked_lsq_host import FAKE, _dense, _dvars, _vec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW7, LITERAL = ("literal", True), ("literal", False)


@pytest.fixture(scope="module")
def lib():
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


def _form(idx):
    from parametron_jl_amd.lazyexpression import LsqTerm, QuadForm
    return LsqTerm("form", r=QuadForm(_dense(len(idx), idx).mat, _dvars(idx)))


def _block(idx, rows=10):
    from parametron_jl_amd.lazyexpression import LsqTerm
    return LsqTerm("block", r=_dense(rows, idx, vec=_vec(rows), sign=-1))


def _terms(what):
    from parametron_jl_amd.lazyexpression import LsqTerm
    if what == "two-forms":
        return [_form([1, 2]), _form([3, 4, 5])]
    if what == "mixed":
        # dot(r, r) + 0.5*dot(x, x) + 2.0 + transpose(u)*R*u + dot(c, u) + s   over x = [1, 2, 3], u = [4, 5]
        return [_block([1, 2, 3]), LsqTerm("diag", xvars=_dvars([1, 2, 3])).scaled(0.5), LsqTerm("constant", scale=2.0), _form([4, 5]),
                LsqTerm("linear", xvars=_dvars([4, 5]), vec=_vec(2)), LsqTerm("constant", value=_vec(1))]
    if what == "interleaved":
        return [_form([1, 3, 5]), _form([2, 4])]
    if what == "u-first":
        return [_form([4, 5]), _block([1, 2, 3])]
    if what == "part":
        return [_block([1, 2, 3]), _form([4, 5, 6]), LsqTerm("diag", xvars=_dvars([4, 6]))]
    if what == "overlap":
        return [_form([1, 2, 3]), _form([3, 4])]
    if what == "linear-union":
        return [_form([1, 2]), _form([3, 4]), LsqTerm("linear", xvars=_dvars([1, 2, 3, 4]), vec=_vec(4))]
    if what == "foreign":
        return [_form([1, 2]), _form([3, 4]), LsqTerm("diag", xvars=_dvars([5, 6]))]
    if what == "unsorted":
        return [_form([1, 2]), _form([4, 3])]
    if what == "nine":
        return [_form([2 * g + 1, 2 * g + 2]) for g in range(9)]
    if what == "eight":
        return [_form([2 * g + 1, 2 * g + 2]) for g in range(8)]
    if what == "one":
        return [_form([1, 2, 3]), LsqTerm("linear", xvars=_dvars([1, 2, 3]), vec=_vec(3))]
    raise KeyError(what)


def _plan(what, **args):
    from parametron_jl_amd.moi import quad_plan
    # nq: the terms of the node's literal expansion, as the model hands them over — here of a sum large enough for the mode
    kw = dict(kind="quad", nq=1 << 20, is_objective=True, quadratic_mode="canonical", small=False, handoff="moi", varmap=None)
    kw.update(args)
    terms = _terms(what)
    return quad_plan(terms, False, **kw), terms


GROUPS = ("canonical-groups", False)
CASES = [
    ("two-forms", dict(), GROUPS),
    ("mixed", dict(), GROUPS),
    ("interleaved", dict(), GROUPS),
    ("u-first", dict(), GROUPS),
    ("part", dict(), GROUPS),
    ("eight", dict(), GROUPS),
    ("overlap", dict(), ROW7),
    ("linear-union", dict(), ROW7),
    ("foreign", dict(), ROW7),
    ("unsorted", dict(), ROW7),
    ("nine", dict(), ROW7),
    ("two-forms", dict(small=True), ROW7),
    ("two-forms", dict(handoff="device", varmap=np.arange(1, 6, dtype=np.int64)), ROW7),
    ("two-forms", dict(handoff="host_csc", varmap=np.arange(1, 6, dtype=np.int64)), ROW7),
    ("two-forms", dict(is_objective=False), ROW7),
    ("two-forms", dict(quadratic_mode="auto"), LITERAL),
    ("two-forms", dict(quadratic_mode="literal"), LITERAL),
    ("one", dict(), ("canonical-sum", False)),
    # a literal function below moi.GROUPS_MIN_LITERAL_TERMS (2^14 terms) keeps today's path; one group (row 6) has no such bound
    ("two-forms", dict(nq=(1 << 14) - 1), ROW7),
    ("mixed", dict(nq=5760), ROW7),
    ("two-forms", dict(nq=1 << 14), GROUPS),
    ("one", dict(nq=100), ("canonical-sum", False)),
]


@pytest.mark.parametrize("what,args,expected", CASES, ids=["%02d-%s-%s" % (i, c[0], c[2][0]) for i, c in enumerate(CASES)])
def test_table(lib, what, args, expected):
    plan, terms = _plan(what, **args)
    assert (plan.mode, plan.canonicalize) == expected
    assert plan.gram is None and plan.form is None
    assert (plan.groups is not None) == (plan.mode == "canonical-groups")
    assert plan.terms is (terms if plan.mode == "canonical-sum" else None)
    if plan.mode != "canonical-groups":
        return
    # every term is in exactly one group, expression order kept inside the group; the sets are the blocks' own, disjoint and sorted
    assert 2 <= len(plan.groups) <= lib.PMT_QUAD_MAX_GROUPS
    assert sorted(id(t) for g in plan.groups for t in g.terms) == sorted(id(t) for t in terms)
    for g in plan.groups:
        pos = [[id(t) for t in terms].index(id(t)) for t in g.terms]
        assert pos == sorted(pos)
        assert np.all(np.diff(g.vars) > 0)
    z = np.concatenate([g.vars for g in plan.groups])
    assert len(set(z.tolist())) == len(z)
    # a Gram record exactly when a group holds a least-squares block (Model.initialize: side lane)
    assert plan.gram_record == any(t.kind == "block" for t in terms)
    # Model.initialize asks every operand for its stacked matrix: all blocks and forms of all groups are named
    assert sorted(id(r) for r in plan.operands()) == sorted(id(t.r) for t in terms if t.kind in ("block", "form"))


def test_terms_join_the_right_group(lib):
    plan, terms = _plan("mixed")
    gx, gu = plan.groups
    assert list(gx.vars) == [1, 2, 3] and list(gu.vars) == [4, 5]
    assert [t.kind for t in gx.terms] == ["block", "diag", "constant", "constant"]          # both constants with the first group
    assert gx.terms[2].scale == 2.0 and gx.terms[3].value is terms[5].value
    assert [t.kind for t in gu.terms] == ["form", "linear"]
    # groups are ordered by the first appearance of one of their blocks, not by their variables
    plan, terms = _plan("u-first")
    assert [list(g.vars) for g in plan.groups] == [[4, 5], [1, 2, 3]]
    # a diagonal term over part of one group's set joins that group (the subset rule of pmt_quad_gram_sum_sub_f64)
    plan, terms = _plan("part")
    assert [t.kind for t in plan.groups[1].terms] == ["form", "diag"] and [t.kind for t in plan.groups[0].terms] == ["block"]


def test_row7_of_the_objective_table_stays(lib):
    """a block over [1, 2, 3] plus dot(u, u) over [4, 5]: one group only, a term over foreign variables — literal, as before"""
    from parametron_jl_amd.lazyexpression import LsqTerm
    from parametron_jl_amd.moi import quad_plan
    terms = [_block([1, 2, 3]), LsqTerm("diag", xvars=_dvars([4, 5]))]
    for nq in (100, 1 << 20):
        plan = quad_plan(terms, False, "quad", nq, True, "canonical", False, "moi")
        assert (plan.mode, plan.canonicalize) == ROW7 and plan.groups is None


def _restate_layout(sets):
    """destination (group, row, first column .. ) per row of z, and the words of every row, by plain loops"""
    owner = {int(v): (g, j) for g, s in enumerate(sets) for j, v in enumerate(s)}
    n = [len(s) for s in sets]
    base = np.concatenate([[0], np.cumsum([k * (k + 1) // 2 for k in n])])
    rows, w = [], 0
    for v in sorted(owner):
        g, j = owner[v]
        src = base[g] + sum(n[g] - i for i in range(j))
        rows.append((3 * src, w, g, j))
        w += 3 * (n[g] - j)
    return rows, w


@pytest.mark.parametrize("sets", [([1, 2], [3, 4, 5]), ([1, 3, 5], [2, 4]), ([7, 8, 9], [1, 2]), ([2], [1, 3]), ([5, 6], [1, 9], [2, 3, 4]),
                                  tuple([g + 1] for g in range(8))], ids=str)
def test_layout(lib, sets):
    lay = lib.GroupsLayout(sets)
    rows, words = _restate_layout(sets)
    assert list(lay.z) == sorted(v for s in sets for v in s)
    assert list(lay.row_src) == [r[0] for r in rows] and list(lay.row_dst) == [r[1] for r in rows] + [words]
    assert list(lay.owner) == [r[2] for r in rows]
    assert lay.nterms == sum(len(s) * (len(s) + 1) // 2 for s in sets) == words // 3 and lay.nlin == len(lay.z)
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])])
    assert list(lay.lin_src) == [off[g] + j for _, _, g, j in rows]
    # ordered: every group's variables are consecutive in z, whatever the order of the groups
    runs = 1 + sum(1 for a, b in zip(rows, rows[1:]) if a[2] != b[2])
    assert lay.ordered == (runs == len(sets))
    if lay.ordered:
        for g in range(len(sets)):
            first = [i for i, r in enumerate(rows) if r[2] == g][0]
            assert lay.dst_lin[g] == first and 3 * lay.dst_quad[g] == rows[first][1]


def test_layout_rejects_what_the_plan_rejects(lib):
    for sets in (([1, 2], [2, 3]), ([2, 1], [3]), ([1], []), ()):
        with pytest.raises(lib.ArgumentError):
            lib.GroupsLayout(sets)


# ---- the entry points: exported, bound, arguments checked before any device call
def test_entry_points_are_exported_and_bound(lib):
    raw = C.CDLL(lib.LIB_PATH)
    julia = open(os.path.join(ROOT, "julia", "ParametronHIP.jl")).read()
    for name in ("pmt_quad_groups_gather_f64", "pmt_quad_groups_constant_f64"):
        assert hasattr(raw, name) and name in lib.SIGNATURES
        assert re.search(r"ccall\(\(:%s, lib\)" % name, julia), name
    hdr = open(os.path.join(ROOT, "include", "parametron_hip.h")).read()
    assert re.search(r"#define PMT_QUAD_MAX_GROUPS %d\b" % lib.PMT_QUAD_MAX_GROUPS, hdr)


def _gather(lib, src=FAKE, row_src=FAKE, row_dst=FAKE, nrows=2, nterms=3, src_lin=FAKE, lin_src=FAKE, nlin=2, out_quad=FAKE, out_lin=FAKE):
    lib.call("pmt_quad_groups_gather_f64", src, row_src, row_dst, nrows, nterms, src_lin, lin_src, nlin, out_quad, out_lin, None)


def test_gather_rejects_bad_arguments(lib):
    for bad in (dict(nrows=-1), dict(nterms=-1), dict(nlin=-2), dict(nrows=4, nterms=3), dict(nrows=0, nterms=3)):
        with pytest.raises(lib.DimensionMismatch):
            _gather(lib, **bad)
    for bad in ("src", "row_src", "row_dst", "out_quad", "src_lin", "lin_src", "out_lin"):
        with pytest.raises(lib.ArgumentError):
            _gather(lib, **{bad: None})
    _gather(lib, nrows=0, nterms=0, nlin=0, src=None, row_src=None, row_dst=None, src_lin=None, lin_src=None, out_quad=None, out_lin=None)   # nothing to do


def test_constant_rejects_bad_arguments(lib):
    for g in (0, -1, lib.PMT_QUAD_MAX_GROUPS + 1):
        with pytest.raises(lib.ArgumentError):
            lib.call("pmt_quad_groups_constant_f64", FAKE, g, FAKE, None)
    with pytest.raises(lib.ArgumentError):
        lib.call("pmt_quad_groups_constant_f64", None, 2, FAKE, None)
    with pytest.raises(lib.ArgumentError):
        lib.call("pmt_quad_groups_constant_f64", FAKE, 2, None, None)
