"""CPU-only: the tracking cost transpose(x (+|-) v) * Q * (x (+|-) v) as one canonical node (pmt_quad_form_shift_f64).  The numpy restatement
of the header's order against the oracle's literal composition; the bilinear rule's table against a stub context; the quad_plan rows of
the shifted form; what one compiled record allocates and calls; the entry point's argument validation and workspace arithmetic."""
import numpy as np
import pytest

import __graft_entry__ as entry
import quad_form_shift_util as U
from test_quad_form_host import restate_form
from test_record_tape_host import FAKE, VARMAP_BUF, StubContext, _b, _block, _form, _model


@pytest.fixture(scope="module")
def lib():
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- 1. the restatement against the oracle's composition
@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_restatement_equals_the_oracle_composition(n, sign):
    """indices exactly, quadratic coefficients bit for bit (each the sum of two numbers), lin and the constant within the sum of the
    node's and the oracle's own rounding bounds (quad_form_shift_util)"""
    Q, v, xvar, varmap = U.make_case(n, 1000 + 7 * n + sign, special=(n == 65))
    at, qt, const = U.oracle_tracking(Q, xvar, v, sign, varmap)
    coeff, row, col = restate_form(Q, xvar, varmap, 1)
    assert len(qt) == n * (n + 1) // 2 and len(at) == n
    assert np.array_equal(qt["row"], row) and np.array_equal(qt["col"], col)
    assert np.array_equal(bits(qt["coeff"]), bits(coeff))
    assert np.array_equal(at["var"], varmap[xvar - 1])
    lin, cst = U.restate_shift(Q, v, sign)
    bound = U.node_lin_bound(Q, v, sign) + U.oracle_lin_bound(Q, v, sign)
    assert np.all(np.abs(lin - at["coeff"]) <= bound), np.max(np.abs(lin - at["coeff"]) / np.maximum(bound, 1e-300))
    assert abs(cst - const) <= U.node_const_bound(Q, v, sign) + U.oracle_const_bound(Q, v, sign)
    # the bound is not vacuous: far below the values it guards
    if n >= 63:
        assert np.max(bound) < 1e-9 * np.max(np.abs(lin))
    # and against the exact values in extended precision
    c = U.shift_consts(v, sign).astype(np.longdouble)
    Ql = Q.astype(np.longdouble)
    assert np.all(np.abs(lin - ((Ql + Ql.T) @ c).astype(np.float64)) <= U.node_lin_bound(Q, v, sign) + 1e-18 * np.abs(lin) + 1e-300)


def test_restatement_by_hand():
    """n = 2, small integers: every step exact"""
    Q = np.array([[1.0, 2.0], [4.0, -3.0]])
    lin, cst = U.restate_shift(Q, np.array([1.0, 2.0]), -1)
    # c = (-1, -2); S = [[2, 6], [6, -6]]; lin = S c = (-14, 6); const = c'Qc = 1 + 4 + 8 - 12 = 1
    assert lin.tolist() == [-14.0, 6.0] and cst == 1.0
    lin, cst = U.restate_shift(Q, np.array([1.0, 2.0]), 1)
    assert lin.tolist() == [14.0, -6.0] and cst == 1.0
    # the first product starts the chain: a lone -0.0 product stays -0.0; the constant's chains start from +0.0
    lin, cst = U.restate_shift(np.array([[-1.0]]), np.array([0.0]), -1)       # S = -2, c = +0.0
    assert np.signbit(lin[0]) and cst == 0.0 and not np.signbit(cst)


# ---- 2. the rule table
@pytest.fixture
def rules(lib, monkeypatch):
    """a model whose device is a stub context (fake addresses; a dense matrix Parameter's upload is a no-op)"""
    import parametron_jl_amd as P
    from parametron_jl_amd.device import DMat
    monkeypatch.setattr(DMat, "upload", lambda self, ctx, m: None)
    model = _model()
    ctx = StubContext(lib)
    monkeypatch.setattr(model, "device", lambda: ctx)
    return P, model, ctx


def _operands(P, model, n, seed=3):
    rng = np.random.default_rng(seed)
    vals = {"Q": rng.standard_normal((n, n)), "p": rng.standard_normal(n), "p2": rng.standard_normal(n)}
    x = [P.Variable(model) for _ in range(n + 2)]
    Q = P.Parameter(lambda: vals["Q"], model)
    p = P.Parameter(lambda: vals["p"], model)
    p2 = P.Parameter(lambda: vals["p2"], model)
    return x, Q, p, p2, vals


def test_rule_gives_a_bare_shifted_form_for_both_spellings(rules):
    from parametron_jl_amd.device import DQuad
    from parametron_jl_amd.lazyexpression import QuadForm
    P, model, ctx = rules
    n = 6
    x, Q, p, p2, _ = _operands(P, model, n)
    xs = x[1:n + 1]
    for sign, e in ((-1, xs - p), (1, xs + p)):
        for node in (P.transpose(e) * Q * e, P.bilinear(e, Q, e)):
            assert node.lsq_bare and len(node.lsq_sum) == 1
            t = node.lsq_sum[0]
            assert t.kind == "form" and isinstance(t.r, QuadForm) and t.scale == 1.0 and t.param is None
            assert t.r.sign == sign and t.r.vec is e.out.vec and t.r.vec.buf == p._dev.buf and t.r.mat is Q._dev
            assert t.r.xvars.vars.tolist() == list(range(2, n + 2))
            # the literal function is dot(e, Q*e)'s: n^2 quadratic, n(n+1) linear terms, deferred
            assert isinstance(node.out, DQuad) and (node.out.nq, node.out.nl) == (n * n, n * (n + 1)) and node.out.quad is None
            assert node.builder == "vecdot!"
    # the plain form keeps its description: no vector, sign 0
    plain = (P.transpose(xs) * Q * xs).lsq_sum[0].r
    assert plain.vec is None and plain.sign == 0


def test_rule_leaves_every_other_mix_literal(rules):
    P, model, ctx = rules
    n = 6
    x, Q, p, p2, vals = _operands(P, model, n)
    xs = x[1:n + 1]
    e = xs - p
    mixes = {"plain left": P.transpose(xs) * Q * e,
             "plain right": P.transpose(e) * Q * xs,
             "another vector": P.transpose(e) * Q * (xs - p2),
             "another sign": P.transpose(e) * Q * (xs + p),
             "other variables": P.transpose(e) * Q * (x[2:n + 2] - p),
             "unsorted x": P.bilinear(xs[::-1] - p, Q, xs[::-1] - p),
             "repeated x": P.bilinear((xs[:-1] + xs[:1]) - p, Q, (xs[:-1] + xs[:1]) - p),
             "constant Q": P.bilinear(e, vals["Q"], e)}
    for name, node in mixes.items():
        assert node.lsq_sum is None and not node.lsq_bare, name
        assert node.out.kind == "quad" and node.out.nq == n * n, name
    # two nodes of the same x - p are the same shifted vector (the same buffer, the same sign): dot(x - v, x - v)'s test
    again = P.transpose(xs - p) * Q * (xs - p)
    assert again.lsq_bare and again.lsq_sum[0].r.sign == -1


def test_rule_errors(rules, lib):
    import scipy.sparse as sp
    P, model, ctx = rules
    n = 6
    x, Q, p, p2, _ = _operands(P, model, n)
    xs = x[1:n + 1]
    e = xs - p
    Qs = P.Parameter(lambda: sp.identity(n, format="csc"), model)
    with pytest.raises(lib.ArgumentError, match=r"shifted vector x \(\+\|-\) v beside a sparse Q is not supported"):
        P.transpose(e) * Qs * e
    with pytest.raises(lib.ArgumentError, match="sparse Q"):
        P.bilinear(xs, Qs, e)
    short = x[1:n] - P.Parameter(lambda: np.zeros(n - 1), model)
    for bad in (lambda: P.bilinear(short, Q, short), lambda: P.bilinear(e, Q, short), lambda: P.bilinear(short, Q, e),
                lambda: P.bilinear(short, Qs, short), lambda: P.bilinear(xs, Q, short)):
        with pytest.raises(lib.DimensionMismatch):
            bad()
    # a residual A*x - b on either side is no shifted Variable vector: the rule's refusal stays
    A = P.Parameter(lambda: np.ones((n, n)), model)
    r = A * xs - p
    with pytest.raises(lib.ArgumentError, match="taffvec \\* mat is not supported on the device"):
        P.transpose(r) * Q
    with pytest.raises(lib.ArgumentError, match="needs Variable vectors and a matrix"):
        P.bilinear(r, Q, r)


# ---- 3. quad_plan rows
def _shifted(n, idx, sign=-1):
    f = _form(n, idx)
    f.vec, f.sign = _b(n), sign
    return f


def test_quad_plan_rows_of_a_shifted_form(lib):
    from parametron_jl_amd.lazyexpression import LsqTerm
    from parametron_jl_amd.moi import GROUPS_MIN_LITERAL_TERMS, _lsq_groups, _lsq_sum_combines, quad_plan
    n = 9
    idx = np.arange(2, 2 + n)
    form = _shifted(n, idx)
    one = [LsqTerm("form", r=form)]
    vm = np.arange(1, 40, dtype=np.int64)                                   # x keeps its order: the plain form's CSC shortcut would apply
    p = quad_plan(one, True, "quad", n * n, True, "canonical", False, "moi", None)
    assert p.mode == "canonical-form" and p.form is form and not p.canonicalize and not p.gram_record
    # the device hand-off, constraints, small models: the literal function through canonicalize!
    for args in ((True, "canonical", False, "device"), (False, "canonical", False, "moi"), (False, "canonical", False, "device"),
                 (True, "canonical", True, "moi"), (True, "canonical", False, "host_csc")):
        p = quad_plan(one, True, "quad", n * n, args[0], args[1], args[2], args[3], vm)
        assert p.mode == "literal" and p.canonicalize and p.form is None, args
    # the plain form over the same x does take the shortcut: only the shift keeps it out
    assert quad_plan([LsqTerm("form", r=_form(n, idx))], True, "quad", n * n, True, "canonical", False, "device", vm).mode == "canonical-form"
    for small in (True, False):
        p = quad_plan(one, True, "quad", n * n, True, "auto", small, "moi", None)
        assert p.mode == "literal" and not p.canonicalize
    assert quad_plan(one, True, "quad", n * n, True, "literal", False, "moi", None).mode == "literal"
    # inside a sum: a block with a non-zero affine part, first or later
    block = _block(30, idx, _b(30), -1)
    sums = {"weighted": [LsqTerm("form", r=form, param=object())],
            "lqr over one x": [LsqTerm("form", r=form), LsqTerm("form", r=_form(n, idx))],
            "form + block": [LsqTerm("form", r=form), LsqTerm("block", r=block)],
            "block + form": [LsqTerm("block", r=block), LsqTerm("form", r=form, scale=0.5)],
            "ridge": [LsqTerm("form", r=form), LsqTerm("diag", xvars=form.xvars, param=object()), LsqTerm("linear", xvars=form.xvars, vec=_b(n)),
                      LsqTerm("constant", scale=2.0)]}
    for name, terms in sums.items():
        assert _lsq_sum_combines(terms), name
        p = quad_plan(terms, False, "quad", 99, True, "canonical", False, "moi", None, sparse_sums=True)
        assert p.mode == "canonical-sum" and p.terms is terms, name
        assert quad_plan(terms, False, "quad", 99, True, "canonical", False, "device", vm, sparse_sums=True).mode == "literal", name
    # over two disjoint vectors: the groups, from GROUPS_MIN_LITERAL_TERMS literal terms on
    u = np.arange(20, 25)
    pair = [LsqTerm("form", r=form), LsqTerm("form", r=_form(5, u))]
    assert not _lsq_sum_combines(pair) and len(_lsq_groups(pair)) == 2
    p = quad_plan(pair, False, "quad", GROUPS_MIN_LITERAL_TERMS, True, "canonical", False, "moi", None, sparse_sums=True)
    assert p.mode == "canonical-groups" and [g.vars.tolist() for g in p.groups] == [idx.tolist(), u.tolist()] and not p.gram_record
    assert p.groups[0].terms[0].r is form
    p = quad_plan(pair, False, "quad", GROUPS_MIN_LITERAL_TERMS - 1, True, "canonical", False, "moi", None, sparse_sums=True)
    assert p.mode == "literal" and p.canonicalize


# ---- 4. one compiled record, from the rule to the recorded calls
def _emit_all(ctx, node):
    from parametron_jl_amd.lazyexpression import DeviceNode, schedule
    order = [x for x in schedule([node]) if isinstance(x, DeviceNode)]
    for x in order:
        x.prepare()
    for x in order:
        x.emit(ctx)


def test_compiled_record_calls_the_node_and_allocates_nothing_literal(rules, lib):
    from parametron_jl_amd import moi
    P, model, ctx = rules
    n = 129
    x, Q, p, p2, _ = _operands(P, model, n)
    xs = x[1:n + 1]
    before = len(ctx.allocs)
    node = P.transpose(xs - p) * Q * (xs - p)
    assert max(ctx.allocs[before:]) <= 8 * Q._dev.lda * n                          # Q itself is the largest thing the rule allocates
    plan = moi.quad_plan(node.lsq_sum, node.lsq_bare, "quad", node.out.nq, True, "canonical", False, "moi", None, sparse_sums=True)
    assert plan.mode == "canonical-form"
    rec = moi.Objective(model, node)
    rec.plan = plan
    mark = len(ctx.allocs)
    emit = rec.compile(ctx, VARMAP_BUF, None)
    nq = n * (n + 1) // 2
    ws = int(lib.load().pmt_quad_form_shift_workspace_bytes(n))
    assert ws == 8 * (3 + 1) * n
    assert ctx.allocs[mark:] == [24 * nq, 16 * n, 8, ws]
    assert set(rec.dev) == {"quad", "lin", "const"} and len(rec.f.quadratic_terms) == nq and len(rec.f.affine_terms) == n
    _emit_all(ctx, node)                                                        # the nodes below the record: nothing to write
    assert ctx.calls == []
    mark = len(ctx.allocs)
    emit(ctx)
    emit(ctx)
    assert len(ctx.allocs) == mark                                              # update! allocates nothing
    assert ctx.calls == [("pmt_quad_form_shift_f64", (Q._dev.lda, n, -1, 1, 1.0))] * 2
    assert node.out.quad is None and node.inputs[1].out.terms is None and not node.inputs[0].out.need_terms
    assert max(ctx.allocs) < 16 * n * n                                         # no literal-sized buffer anywhere


def test_shifted_form_in_a_sum_calls_the_node_first_and_later(lib):
    """_lsq_sum_emitter: the shifted form as the first block (terms, lin, constant) and as a later block (CSC values, lin, constant), each
    with its own workspace; the plain form beside it keeps its call"""
    from parametron_jl_amd.lazyexpression import LsqTerm
    from parametron_jl_amd.moi import QuadPlan
    from test_record_tape_host import _objective, _quad_out
    n = 70
    idx = np.arange(3, 3 + n)
    f1, f2, plain = _shifted(n, idx, -1), _shifted(n, idx, 1), _form(n, idx)
    terms = [LsqTerm("form", r=f1, scale=2.0), LsqTerm("form", r=plain), LsqTerm("form", r=f2), LsqTerm("constant", scale=1.5)]
    rec = _objective(_model(), _quad_out(7, 7), QuadPlan("canonical-sum", terms=terms))
    ctx = StubContext(lib)
    emit = rec.compile(ctx, VARMAP_BUF, None)
    nq, ws = n * (n + 1) // 2, 8 * (2 + 1) * n
    assert ctx.allocs == [24 * nq, 16 * n, 8, ws, ws, 8 * nq, 16 * n, 8, 8 * nq, 16 * n, 8]
    mark = len(ctx.allocs)
    emit(ctx)
    assert len(ctx.allocs) == mark
    assert ctx.calls == [("pmt_quad_form_shift_f64", (n, n, -1, 1, 1.0)), ("pmt_quad_form_f64", (n, n, 1, 1.0)),
                         ("pmt_quad_form_shift_f64", (n, n, 1, 1, 1.0)), ("pmt_quad_gram_sum_f64", (n, 4))]


def test_literal_function_is_the_record_of_dot_e_Qe(rules):
    """a literal consumer: the new spelling schedules the calls of dot(e, Q*e) — the same builders, the same sizes, the same operands"""
    P, model, ctx = rules
    n = 8
    x, Q, p, p2, _ = _operands(P, model, n)
    xs = x[:n]
    e = xs - p
    new = P.transpose(e) * Q * e
    e2 = xs - p
    old = P.dot(e2, Q * e2)
    assert (new.out.nq, new.out.nl) == (old.out.nq, old.out.nl) == (n * n, n * n + n)
    for node in (new, old):
        node.out.materialize()
        ctx.calls.clear()
        _emit_all(ctx, node)
        node.calls = list(ctx.calls)
    assert new.calls == old.calls
    assert [c[0] for c in new.calls] == ["pmt_vars_addsub_f64", "pmt_matvecmul_affs_f64", "pmt_quad_expand_f64"]
    assert new.calls[1][1] == (Q._dev.lda, n, n, 1) and new.calls[2][1] == (n, 1, n, 0)


# ---- 5. the entry point without a device
def _call(lib, Q=FAKE, ldq=8, n=8, xvar=FAKE, v=FAKE, sign=-1, moi=1, varmap=FAKE, alpha=1.0, quad=FAKE, values=FAKE, lin=FAKE, const=FAKE, ws=FAKE):
    lib.call("pmt_quad_form_shift_f64", Q, ldq, n, xvar, v, sign, moi, varmap, alpha, quad, values, lin, const, ws, None)


@pytest.mark.parametrize("bad", [
    {"Q": None}, {"xvar": None}, {"v": None}, {"ws": None}, {"sign": 0}, {"sign": 2}, {"n": 0}, {"n": -3}, {"n": (1 << 21) + 1, "ldq": 1 << 22},
    {"ldq": 7}, {"moi": 1, "varmap": None}, {"quad": None, "values": None},
], ids=["null-Q", "null-xvar", "null-v", "null-workspace", "sign-zero", "sign-two", "n-zero", "n-negative", "n-beyond-2^21", "ldq-below-n",
        "moi-without-varmap", "no-output"])
def test_entry_point_rejects_bad_arguments_before_any_device_call(lib, bad):
    with pytest.raises(lib.ArgumentError) as err:
        _call(lib, **bad)
    assert "quad_form_shift" in str(err.value)


def test_entry_point_is_declared_bound_and_exported(lib):
    import ctypes as C
    raw = C.CDLL(lib.LIB_PATH)
    for name, nargs in (("pmt_quad_form_shift_f64", 15), ("pmt_quad_form_shift_workspace_bytes", 1)):
        assert hasattr(raw, name) and len(lib.SIGNATURES[name][1]) == nargs
    assert len(lib.SIGNATURES["pmt_quad_form_f64"][1]) == 12                     # the plain form keeps its signature


def test_workspace_bytes_is_host_arithmetic(lib):
    f = lib.load().pmt_quad_form_shift_workspace_bytes
    assert [int(f(n)) for n in (1, 64, 65, 4096)] == [8 * 2, 8 * 2 * 64, 8 * 3 * 65, 8 * 65 * 4096]
    assert int(f(129)) == 8 * 4 * 129 and int(f(0)) == 0
