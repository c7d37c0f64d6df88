"""CPU-only: which of literal / canonical / canonical-csc / canonical-form / canonical-sum a quadratic record takes (moi.quad_plan, the one
decision Model.initialize executes), row by row of its table, on device values built without a device."""
import numpy as np
import pytest

import __graft_entry__ as entry
from test_stacked_lsq_host import _dense, _dvars, _stacked, _vec

X = [1, 2, 3]
IDENT, PERMUTED = np.array([1, 2, 3, 4, 5], dtype=np.int64), np.array([2, 1, 3, 4, 5], dtype=np.int64)
BIG = 1 << 24


@pytest.fixture(scope="module")
def lib():
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


def _node(what):
    """(terms, bare, operand the plan must name) of a scalar node, as lazyexpression describes it"""
    from parametron_jl_amd.lazyexpression import LsqTerm, QuadForm
    A = _dense(10, X, vec=_vec(10), sign=-1)
    if what in ("dense", "dense-unsorted"):
        A = A if what == "dense" else _dense(10, [2, 1, 3])
        return [LsqTerm("block", r=A)], True, A                                   # dot(r, r)
    if what == "stacked":
        st = _stacked([(_dense(10, [1, 2]).mat, _dvars([1, 2]), 1), (_dense(10, [3]).mat, _dvars([3]), -1)], None, 0)
        st.xvars = _dvars(X)                                                      # (DStackedAff.__init__: the sorted union z)
        return [LsqTerm("block", r=st)], True, st
    if what == "form":
        Q = QuadForm(_dense(3, X).mat, _dvars(X))
        return [LsqTerm("form", r=Q)], True, Q                                    # transpose(x) * Q * x
    if what == "scaled":
        terms = [LsqTerm("block", r=A).scaled(1.0)]                               # 1.0 * dot(r, r): a sum of one term
    elif what == "sum":
        terms = [LsqTerm("block", r=A), LsqTerm("diag", xvars=_dvars(X)).scaled(0.5)]
    elif what == "sum-part":
        terms = [LsqTerm("block", r=A), LsqTerm("diag", xvars=_dvars([1, 3]))]    # dot(u, u) over part of x
    elif what == "sum-foreign":
        terms = [LsqTerm("block", r=A), LsqTerm("diag", xvars=_dvars([4, 5]))]    # over variables that are not in x
    elif what == "sum-9":
        terms = [LsqTerm("block", r=_dense(10, X)) for _ in range(9)]
    elif what == "sum-form":
        terms = [LsqTerm("form", r=QuadForm(_dense(3, X).mat, _dvars(X))), LsqTerm("linear", xvars=_dvars(X), vec=_vec(3))]
    return terms, False, terms


LITERAL, ROW7 = ("literal", False), ("literal", True)
# (node, arguments that differ from: the objective of a model beyond the small plan, quadratic_mode="canonical", handoff="moi", 100 literal
# terms) -> (mode, canonicalize)
CASES = [
    # row 1: quadratic_mode="literal"
    ("dense", dict(quadratic_mode="literal"), LITERAL),
    ("form", dict(quadratic_mode="literal"), LITERAL),
    ("sum", dict(quadratic_mode="literal"), LITERAL),
    # row 2: a bare dense block — any record, small or not; canonical-csc when the early varmap keeps x in order
    ("dense", dict(), ("canonical", False)),
    ("dense", dict(small=True), ("canonical", False)),
    ("dense", dict(is_objective=False), ("canonical", False)),
    ("dense", dict(handoff="device", varmap=IDENT), ("canonical-csc", False)),
    ("dense", dict(handoff="host_csc", varmap=IDENT + 7), ("canonical-csc", False)),
    ("dense", dict(handoff="device", varmap=PERMUTED), ("canonical", False)),
    ("dense", dict(is_objective=False, handoff="device", varmap=IDENT), ("canonical-csc", False)),
    ("dense", dict(quadratic_mode="auto", nq=BIG + 1), ("canonical", False)),
    ("dense", dict(quadratic_mode="auto", nq=BIG + 1, handoff="device", varmap=IDENT), ("canonical-csc", False)),
    # row 3: "auto" otherwise
    ("dense", dict(quadratic_mode="auto", nq=BIG), LITERAL),
    ("dense-unsorted", dict(quadratic_mode="auto", nq=BIG + 1), LITERAL),
    ("stacked", dict(quadratic_mode="auto", nq=BIG + 1), LITERAL),
    ("form", dict(quadratic_mode="auto", nq=BIG + 1), LITERAL),
    ("sum", dict(quadratic_mode="auto", nq=BIG + 1), LITERAL),
    # row 4: a bare stacked block beyond the small plan — any quad record
    ("stacked", dict(), ("canonical", False)),
    ("stacked", dict(is_objective=False), ("canonical", False)),
    ("stacked", dict(handoff="device", varmap=IDENT), ("canonical-csc", False)),
    ("stacked", dict(handoff="host_csc", varmap=PERMUTED), ("canonical", False)),
    ("stacked", dict(small=True), ROW7),
    # row 5: a bare form, the objective, beyond the small plan, "moi" or "device" with x in order
    ("form", dict(), ("canonical-form", False)),
    ("form", dict(handoff="device", varmap=IDENT), ("canonical-form", False)),
    ("form", dict(handoff="device", varmap=PERMUTED), ROW7),
    ("form", dict(handoff="host_csc", varmap=IDENT), ROW7),
    ("form", dict(is_objective=False), ROW7),
    ("form", dict(small=True), ROW7),
    # row 6: a sum the combine takes, the objective, beyond the small plan, "moi"
    ("sum", dict(), ("canonical-sum", False)),
    ("scaled", dict(), ("canonical-sum", False)),
    ("sum-part", dict(), ("canonical-sum", False)),
    ("sum-form", dict(), ("canonical-sum", False)),
    ("sum", dict(handoff="device", varmap=IDENT), ROW7),
    ("sum", dict(handoff="host_csc", varmap=IDENT), ROW7),
    ("sum", dict(is_objective=False), ROW7),
    ("sum", dict(small=True), ROW7),
    ("scaled", dict(small=True), ROW7),
    ("sum-9", dict(), ROW7),
    ("sum-foreign", dict(), ROW7),
    # row 7: "canonical" otherwise
    ("dense-unsorted", dict(), ROW7),
    ("dense-unsorted", dict(handoff="device", varmap=IDENT), ROW7),
]


@pytest.mark.parametrize("what,args,expected", CASES, ids=["%02d-%s-%s" % (i, c[0], c[2][0]) for i, c in enumerate(CASES)])
def test_table(lib, what, args, expected):
    from parametron_jl_amd.moi import quad_plan
    terms, bare, operand = _node(what)
    kw = dict(kind="quad", nq=100, is_objective=True, quadratic_mode="canonical", small=False, handoff="moi", varmap=None)
    kw.update(args)
    plan = quad_plan(terms, bare, **kw)
    mode, canonicalize = expected
    assert (plan.mode, plan.canonicalize) == (mode, canonicalize)
    # the plan names what its mode reads, and nothing else
    assert plan.gram is (operand if mode in ("canonical", "canonical-csc") else None)
    assert plan.form is (operand if mode == "canonical-form" else None)
    assert plan.terms is (operand if mode == "canonical-sum" else None)
    # the side lane and the small plan's order treat the Gram node and the sum of Gram nodes alike; a form is no Gram record
    assert plan.gram_record == (mode in ("canonical", "canonical-csc", "canonical-sum"))


def test_only_quadratic_records_have_a_mode(lib):
    from parametron_jl_amd.moi import quad_plan
    terms, bare, _ = _node("sum")
    for kind in ("aff", "affvec"):
        plan = quad_plan(terms, bare, kind, 0, True, "canonical", False, "moi")
        assert plan.mode is None and not plan.gram_record and not plan.canonicalize and plan.terms is None
    assert quad_plan(None, False, "quad", 9, True, "canonical", False, "moi").mode == "literal"          # a node with no description
