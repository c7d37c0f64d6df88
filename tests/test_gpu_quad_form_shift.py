"""-m gpu: the tracking cost transpose(x (+|-) v) * Q * (x (+|-) v) as one canonical node (pmt_quad_form_shift_f64): the entry point, the bare
"canonical-form" objective, the node inside "canonical-sum" and "canonical-groups" objectives, the literal spelling, one solved model.

The quadratic part is compared word for word with pmt_quad_form_f64's for the same inputs; the linear part and the constant bit for bit with
the numpy restatement of the order include/parametron_hip.h fixes (tests/quad_form_shift_util.py), and with the oracle's literal composition
within the rounding bounds derived there."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import parametron_jl_amd as P  # noqa: E402
from parametron_jl_amd import _lib  # noqa: E402
from parametron_jl_amd.device import padded_lda  # noqa: E402
from parametron_jl_amd.moi import _gram_rows  # noqa: E402
import quad_form_shift_util as U  # noqa: E402
from test_gpu_lsq_sum import bits, restate  # noqa: E402
from test_quad_form_host import restate_form  # noqa: E402

DEV = "cuda:0"
GUARD = 8                                                   # poisoned words in front of and behind every output
POISON = -7


def dptr(t, offset_words=0):
    return C.c_void_p(t.data_ptr() + 8 * offset_words) if t is not None else None


def stream(s=None):
    return C.c_void_p((s or torch.cuda.current_stream()).cuda_stream)


# ------------------------------------------------------------------ 1. the entry point
@functools.lru_cache(maxsize=16)
def case(n, sign):
    """(Q, v, xvar, varmap, lin, const): zeros of both signs in Q and v, a permuting and offset varmap; the restatement computed once"""
    Q, v, xvar, varmap = U.make_case(n, 300 + 2 * n + sign, special=True)
    lin, const = U.restate_shift(Q, v, sign)
    return Q, v, xvar, varmap, lin, const


def device_Q(Q, ldq):
    n = Q.shape[0]
    buf = np.full((n, ldq), np.nan)                         # column j of Q at buf[j, :n]; the padding rows hold NaN and must never be read
    buf[:, :n] = Q.T
    return torch.from_numpy(buf.reshape(-1)).to(DEV)


def guarded(words):
    return torch.full((words + 2 * GUARD,), POISON, dtype=torch.int64, device=DEV)


def unguard(t, words, name):
    h = t.cpu().numpy()
    assert np.all(h[:GUARD] == POISON) and np.all(h[GUARD + words:] == POISON), "guard words around %s were written" % name
    return h[GUARD:GUARD + words]


class Entry:
    """device inputs and guarded outputs of one call; the workspace starts as NaN"""

    def __init__(self, n, sign, ldq, moi, want):
        Q, v, xvar, varmap, _, _ = case(n, sign)
        self.n, self.sign, self.ldq, self.moi, self.want = n, sign, ldq, moi, want
        nq = n * (n + 1) // 2
        self.words = {"quad": 3 * nq, "values": nq, "lin": 2 * n, "const": 1}
        self.dQ, self.dx, self.dv = device_Q(Q, ldq), torch.from_numpy(xvar).to(DEV), torch.from_numpy(v).to(DEV)
        self.dvm = torch.from_numpy(varmap).to(DEV)
        self.out = {k: guarded(self.words[k]) for k in want}
        self.ws_words = int(_lib.load().pmt_quad_form_shift_workspace_bytes(n)) // 8
        self.ws = torch.full((self.ws_words + 2 * GUARD,), np.nan, dtype=torch.float64, device=DEV)

    def args(self):
        o = {k: dptr(self.out[k], GUARD) if k in self.out else None for k in self.words}
        return o["quad"], o["values"], o["lin"], o["const"]

    def launch(self, s=None, alpha=1.0):
        _lib.call("pmt_quad_form_shift_f64", dptr(self.dQ), self.ldq, self.n, dptr(self.dx), dptr(self.dv), self.sign, self.moi,
                  dptr(self.dvm) if self.moi else None, alpha, *self.args(), dptr(self.ws, GUARD), stream(s))

    def plain(self, alpha=1.0):
        """pmt_quad_form_f64 on the same inputs: (quad words, value words) of the outputs asked for"""
        q = guarded(self.words["quad"]) if "quad" in self.out else None
        p = guarded(self.words["values"]) if "values" in self.out else None
        _lib.call("pmt_quad_form_f64", dptr(self.dQ), self.ldq, self.n, dptr(self.dx), self.moi, dptr(self.dvm) if self.moi else None, alpha,
                  dptr(q, GUARD), dptr(p, GUARD), None, None, stream())
        torch.cuda.synchronize()
        return (unguard(q, self.words["quad"], "plain quad") if q is not None else None,
                unguard(p, self.words["values"], "plain values") if p is not None else None)

    def results(self):
        torch.cuda.synchronize()
        ws = self.ws.cpu().numpy()
        assert np.all(np.isnan(ws[:GUARD])) and np.all(np.isnan(ws[GUARD + self.ws_words:])), "the workspace's surroundings were written"
        written = self.ws_words if "const" in self.out else self.ws_words - self.n       # the last row: the products behind the constant
        assert not np.any(np.isnan(ws[GUARD:GUARD + written])), "a partial sum of the workspace was never written"
        return {k: unguard(t, self.words[k], k) for k, t in self.out.items()}

    def check(self, got, alpha=1.0):
        Q, v, xvar, varmap, lin, const = case(self.n, self.sign)
        pq, pv = self.plain(alpha)
        if "quad" in got:
            assert np.array_equal(got["quad"], pq), "the quadratic terms differ from pmt_quad_form_f64's"
            coeff, row, col = restate_form(Q, xvar, varmap, self.moi)
            t = got["quad"].view(_lib.QT)
            assert np.array_equal(t["row"], row) and np.array_equal(t["col"], col) and np.array_equal(bits(t["coeff"]), bits(coeff))
        if "values" in got:
            assert np.array_equal(got["values"], pv), "the CSC values differ from pmt_quad_form_f64's"
        if "lin" in got:
            t = got["lin"].view(_lib.LT)
            assert np.array_equal(t["var"], varmap[xvar - 1] if self.moi else xvar)
            assert np.all(np.isfinite(t["coeff"]))
            assert np.array_equal(bits(t["coeff"]), bits(lin)), "lin differs from the restatement"
        if "const" in got:
            assert np.isfinite(got["const"].view(np.float64)[0])
            assert got["const"][0] == bits([const])[0], "the constant differs from the restatement"


def pitch(n):
    return {1: 1, 63: 64, 64: 64, 65: 67, 129: 132, 512: padded_lda(512)}[n]


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 512])
def test_entry_point_bit_for_bit(n, sign):
    """every output; the term output alone and the value output alone; native and MOI indices"""
    ldq = pitch(n)
    assert ldq >= n and (n != 512 or ldq == 576)
    for moi in (1, 0):
        for want in (("quad", "values", "lin", "const"), ("quad", "lin", "const"), ("values", "lin", "const")):
            e = Entry(n, sign, ldq, moi, want)
            e.launch()
            e.check(e.results())


@pytest.mark.parametrize("want", [("quad",), ("values",), ("quad", "lin"), ("values", "const")], ids="+".join)
def test_entry_point_optional_outputs_and_alpha(want):
    """out_lin and out_const are optional, each on its own; alpha scales the CSC values only"""
    for alpha in (1.0, -0.5):
        e = Entry(129, -1, 131, 1, want)
        e.launch(alpha=alpha)
        got = e.results()
        assert sorted(got) == sorted(want)
        e.check(got, alpha)


def test_two_launches_and_two_streams_give_the_same_bits():
    n, sign = 129, -1
    a, b, c = (Entry(n, sign, 130, 1, ("quad", "values", "lin", "const")) for _ in range(3))
    a.launch()
    a.launch()                                              # the second call over the first one's outputs and workspace
    ra = a.results()
    a.check(ra)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    b.launch(s1)
    c.launch(s2)
    rb, rc = b.results(), c.results()
    for k in ra:
        assert np.array_equal(ra[k], rb[k]) and np.array_equal(ra[k], rc[k]), k


# ------------------------------------------------------------------ 2. the bare objective in a model
class Perm(P.MockOptimizer):
    def copy_to(self, backend):
        out = super().copy_to(backend)
        out["variables"] = out["variables"][::-1].copy() + 10
        return out


def new_values(n, seed, special=False):
    Q, v, _, _ = U.make_case(n, seed, special)
    return Q, v


def solved(model):
    P.solve(model)
    f = model.objective.f
    return f.quadratic_terms.copy(), f.affine_terms.copy(), float(f.constant)


@pytest.mark.parametrize("spelling", ["transpose-minus", "bilinear-plus"])
@pytest.mark.parametrize("n", [65, 129])
def test_bare_shifted_form_model(n, spelling):
    """canonical mode beyond the small plan (a graph-replayed model): three solves with new Q and p"""
    sign = -1 if spelling == "transpose-minus" else 1
    extra = 3
    model = P.Model(Perm() if n == 129 else P.MockOptimizer(), quadratic_mode="canonical", use_graph=True)
    try:
        pre = [P.Variable(model) for _ in range(extra)]
        x = [P.Variable(model) for _ in range(n)]
        st = dict(zip(("Q", "p"), new_values(n, 11 * n)))
        Q, p = P.Parameter(lambda: st["Q"], model), P.Parameter(lambda: st["p"], model)
        expr = P.transpose(x - p) * Q * (x - p) if sign < 0 else P.bilinear(x + p, Q, x + p)
        P.objective(model, P.Minimize, expr)
        xvar = np.arange(extra + 1, extra + n + 1, dtype=np.int64)
        nbytes = []
        for it in range(3):
            if it:
                st["Q"], st["p"] = new_values(n, 11 * n + it, special=(it == 2))
            gq, gl, gc = solved(model)
            assert model.objective.mode == "canonical-form" and not model._small and model.objective.plan.form.sign == sign
            varmap = np.asarray(model.model_var_to_optimizer, dtype=np.int64)
            coeff, row, col = restate_form(st["Q"], xvar, varmap, 1)
            lin, const = U.restate_shift(st["Q"], st["p"], sign)
            assert np.array_equal(gq["row"], row) and np.array_equal(gq["col"], col) and np.array_equal(bits(gq["coeff"]), bits(coeff))
            assert np.array_equal(gl["var"], varmap[xvar - 1]) and np.array_equal(bits(gl["coeff"]), bits(lin))
            assert bits([gc])[0] == bits([const])[0]
            # the oracle's literal composition
            at, qt, oconst = U.oracle_tracking(st["Q"], xvar, st["p"], sign, varmap)
            assert np.array_equal(gq.view(np.int64), np.ascontiguousarray(qt).view(np.int64))
            assert np.array_equal(gl["var"], at["var"])
            assert np.all(np.abs(gl["coeff"] - at["coeff"]) <= U.node_lin_bound(st["Q"], st["p"], sign) + U.oracle_lin_bound(st["Q"], st["p"], sign))
            assert abs(gc - oconst) <= U.node_const_bound(st["Q"], st["p"], sign) + U.oracle_const_bound(st["Q"], st["p"], sign)
            nbytes.append(model.device().bytes_allocated())
        assert len(set(nbytes)) == 1, "plan memory grew across solves: %r" % (nbytes,)
    finally:
        model.close()


# ------------------------------------------------------------------ 3. in sums
def gram_outputs(model, n, first):
    """the least-squares block's own Gram outputs on the model's device buffers (row-major coefficients as block 1, CSC values later)"""
    g = [t.r for t in model.objective.lsq_terms if t.kind == "block"][0]
    nq = n * (n + 1) // 2
    ws = torch.zeros(max(2, int(_lib.load().pmt_quad_gram_workspace_bytes(_gram_rows(g), n)) // 8 + 1), dtype=torch.float64, device=DEV)
    lin = torch.empty(2 * n, dtype=torch.int64, device=DEV)
    cc = torch.empty(1, dtype=torch.float64, device=DEV)
    args = (C.c_void_p(g.mat.buf), g.mat.lda, _gram_rows(g), n, C.c_void_p(g.xvars.buf), C.c_void_p(g.vec.buf), g.sign)
    vm = C.c_void_p(model._varmap_buf)
    if first:
        q = torch.empty(3 * nq, dtype=torch.int64, device=DEV)
        _lib.call("pmt_quad_gram_f64", *args, 1, vm, dptr(q), dptr(lin), dptr(cc), dptr(ws), stream())
        torch.cuda.synchronize()
        coeff = q.cpu().numpy().view(_lib.QT)["coeff"].copy()
    else:
        v = torch.empty(nq, dtype=torch.float64, device=DEV)
        _lib.call("pmt_quad_gram_csc_f64", *args, vm, 1.0, dptr(v), None, dptr(lin), dptr(cc), dptr(ws), stream())
        torch.cuda.synchronize()
        coeff = v.cpu().numpy()
    return coeff, lin.cpu().numpy().view(_lib.LT)["coeff"].copy(), float(cc.cpu()[0])


@pytest.mark.parametrize("order", ["form-first", "form-later"])
def test_weighted_shifted_form_in_a_sum(order):
    """w * form_shift + dot(r, r) + dot(c, x) + s, the shifted form as the first block and as a later one: the header's combine order
    (pmt_quad_gram_sum_f64, restated in tests/test_gpu_lsq_sum.py) over the restated node and the Gram block's own outputs"""
    n, rows = 65, 40
    rng = np.random.default_rng(5)
    model = P.Model(P.MockOptimizer(), quadratic_mode="canonical", use_graph=True)
    try:
        x = [P.Variable(model) for _ in range(n)]
        st = {"A": rng.random((rows, n)) - 0.5, "b": rng.random(rows), "c": rng.standard_normal(n), "s": 0.75, "w": 1.5}
        st["Q"], st["p"] = new_values(n, 77)
        Q, p, A, b, c, s, w = (P.Parameter(lambda k=k: st[k], model) for k in ("Q", "p", "A", "b", "c", "s", "w"))
        form = P.transpose(x - p) * Q * (x - p)
        r = A * x - b
        expr = (w * form + P.dot(r, r) if order == "form-first" else P.dot(r, r) + w * form) + P.dot(c, x) + s
        P.objective(model, P.Minimize, expr)
        iu = np.triu_indices(n)
        csc = iu[1] * (iu[1] + 1) // 2 + iu[0]
        for it in range(2):
            if it:
                st["Q"], st["p"] = new_values(n, 78, special=True)
                st["A"], st["b"], st["c"] = rng.random((rows, n)) - 0.5, rng.random(rows), rng.standard_normal(n)
                st["w"], st["s"] = -0.625, float(rng.standard_normal())
            gq, gl, gc = solved(model)
            assert model.objective.mode == "canonical-sum" and not model._small
            c1 = restate_form(st["Q"], np.arange(1, n + 1))[0]
            lin, const = U.restate_shift(st["Q"], st["p"], -1)
            first = order == "form-first"
            if first:
                fcoeff = c1
            else:
                fcoeff = np.empty(len(c1))
                fcoeff[csc] = c1
            fterm = ("block", 1.0 * st["w"], (fcoeff, lin, const))
            gterm = ("block", 1.0, gram_outputs(model, n, not first))
            terms = ([fterm, gterm] if first else [gterm, fterm]) + [("linear", 1.0, st["c"]), ("constant", 1.0, st["s"])]
            coeff, wlin, wconst = restate(n, terms)
            assert np.array_equal(gq["row"], iu[0] + 1) and np.array_equal(gq["col"], iu[1] + 1) and np.array_equal(gl["var"], np.arange(1, n + 1))
            assert np.array_equal(bits(gq["coeff"]), bits(coeff)), "quadratic coefficients differ from the restated combine"
            assert np.array_equal(bits(gl["coeff"]), bits(wlin)), "linear coefficients differ from the restated combine"
            assert bits([gc])[0] == bits([wconst])[0], "the constant differs from the restated combine"
            # the node's affine part is in there: without it lin would be 2 W A'c + c alone
            assert np.max(np.abs(gl["coeff"] - (wlin - st["w"] * lin))) > 1e-3
    finally:
        model.close()


@pytest.mark.parametrize("layout", ["in-order", "interleaved"])
def test_lqr_pair_over_two_vectors(layout):
    """transpose(x - xr)*Q*(x - xr) + transpose(u)*R*u over 129 and 65 disjoint variables ("canonical-groups"): every group's slice is the
    group's own function word for word, the constant the groups' constants added in order"""
    nx, nu = 129, 65
    model = P.Model(P.MockOptimizer(), quadratic_mode="canonical", use_graph=True)
    try:
        x, u = [], []
        if layout == "in-order":
            x = [P.Variable(model) for _ in range(nx)]
            u = [P.Variable(model) for _ in range(nu)]
        else:
            for i in range(nx):
                x.append(P.Variable(model))
                if i < nu:
                    u.append(P.Variable(model))
        xv, uv = (np.array([v.index for v in vs], dtype=np.int64) for vs in (x, u))
        st = {}
        st["Q"], st["xr"] = new_values(nx, 91)
        st["R"], _ = new_values(nu, 92)
        Q, xr, R = (P.Parameter(lambda k=k: st[k], model) for k in ("Q", "xr", "R"))
        P.objective(model, P.Minimize, P.transpose(x - xr) * Q * (x - xr) + P.transpose(u) * R * u)
        nbytes = []
        for it in range(2):
            if it:
                st["Q"], st["xr"] = new_values(nx, 93, special=True)
                st["R"], _ = new_values(nu, 94)
            gq, gl, gc = solved(model)
            assert model.objective.mode == "canonical-groups" and model.objective.groups_ordered == (layout == "in-order")
            cx, rx, kx = restate_form(st["Q"], xv)
            cu, ru, ku = restate_form(st["R"], uv)
            lin, const = U.restate_shift(st["Q"], st["xr"], -1)
            coeff, row, col = np.concatenate([cx, cu]), np.concatenate([rx, ru]), np.concatenate([kx, ku])
            o = np.argsort(row, kind="stable")               # rows by increasing variable; a group's row keeps its own column order
            assert np.array_equal(gq["row"], row[o]) and np.array_equal(gq["col"], col[o]) and np.array_equal(bits(gq["coeff"]), bits(coeff[o]))
            lv, lc = np.concatenate([xv, uv]), np.concatenate([lin, np.zeros(nu)])
            o = np.argsort(lv)
            assert np.array_equal(gl["var"], lv[o]) and np.array_equal(bits(gl["coeff"]), bits(lc[o]))
            assert bits([gc])[0] == bits([const + 0.0])[0]
            nbytes.append(model.device().bytes_allocated())
        assert len(set(nbytes)) == 1
    finally:
        model.close()


# ------------------------------------------------------------------ 4. the literal spelling, the device hand-off
def tracking_model(n, spelling, st, **kw):
    model = P.Model(kw.pop("optimizer", None) or P.MockOptimizer(), **kw)
    x = [P.Variable(model) for _ in range(n)]
    Q, p = P.Parameter(lambda: st["Q"], model), P.Parameter(lambda: st["p"], model)
    e = x - p
    P.objective(model, P.Minimize, P.transpose(e) * Q * e if spelling == "new" else P.dot(e, Q * e))
    return model


def test_literal_spelling_equals_dot_e_Qe():
    """quadratic_mode "auto", a small model: the new spelling's record is dot(e, Q*e)'s, bit for bit"""
    n = 8
    st = dict(zip(("Q", "p"), new_values(n, 5)))
    a, b = tracking_model(n, "new", st, quadratic_mode="auto"), tracking_model(n, "dot", st, quadratic_mode="auto")
    try:
        for it in range(2):
            if it:
                st["Q"], st["p"] = new_values(n, 6, special=True)
            ra, rb = solved(a), solved(b)
            assert a._small and a.objective.mode == "literal" and a.objective.expr.builder == "vecdot!" and b.objective.expr.builder == "vecdot!"
            assert len(ra[0]) == n * n and len(ra[1]) == n * n + n
            assert np.array_equal(ra[0].view(np.int64), rb[0].view(np.int64)) and np.array_equal(ra[1].view(np.int64), rb[1].view(np.int64))
            assert bits([ra[2]])[0] == bits([rb[2]])[0]
    finally:
        a.close()
        b.close()


def test_device_handoff_takes_the_literal_function_through_canonicalize():
    """handoff="device": no CSC shortcut for the shifted form yet — the record dot(e, Q*e) gives, bit for bit"""
    n = 12
    st = dict(zip(("Q", "p"), new_values(n, 8)))
    kw = dict(quadratic_mode="canonical", handoff="device")
    a, b = tracking_model(n, "new", st, **kw), tracking_model(n, "dot", st, **kw)
    try:
        P.solve(a)
        P.solve(b)
        assert a.objective.mode == "literal" and a.objective.expr.builder == "canonicalize!" and a.objective.plan.form is None
        qa, qb = a.device_qp.fetch(), b.device_qp.fetch()
        assert np.array_equal(qa["P"][1], qb["P"][1]) and np.array_equal(qa["P"][2], qb["P"][2])
        assert np.array_equal(bits(qa["P"][0]), bits(qb["P"][0])) and np.array_equal(bits(qa["q"]), bits(qb["q"])) and qa["r"] == qb["r"]
        lin, const = U.restate_shift(st["Q"], st["p"], -1)
        assert np.all(np.abs(qa["q"] - lin) <= U.node_lin_bound(st["Q"], st["p"], -1) + U.oracle_lin_bound(st["Q"], st["p"], -1))
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 5. one solved model
def test_a_solved_tracking_problem_equals_its_expanded_statement():
    """minimize (x - p)'Q(x - p) subject to A x == b, n = 12, three equality rows, Q unsymmetric with a diagonal in [4, 5) and off-diagonal
    entries of at most 0.25 in magnitude (Q + Q' strictly diagonally dominant: strictly convex), through the KKT solve of tests/qp_solver.py;
    the same problem stated as x'Qx - g'x + s with g = (Q + Q')p and s = p'Qp computed on the host.
    Bound 1e-9.  Both objectives hold the same quadratic coefficients bit for bit (the form node's Q + Q'; the combine's weight is 1.0).
    The linear coefficients are two roundings of -(Q + Q')p: the node's, within gamma_{64+1} * |S||p| of it (quad_form_shift_util), and
    numpy's n-term dot products negated by the combine, within gamma_{n+1} * |S||p|.  So the two KKT systems K z = rhs share K and differ
    in rhs by at most d = (gamma_65 + gamma_13) * max_j (|S||p|)_j (computed and asserted below 1e-12), the exact solutions by at most
    |K^-1|_inf * d (asserted below 1e-11), and the solver's own rounding adds about cond(K) * 2^-52 * |z| to each: with cond(K) < 1e3
    (asserted) and |z| of order 1 below 1e-12.  All of it is two orders inside 1e-9."""
    from qp_solver import DenseQPOptimizer
    rng = np.random.default_rng(12)
    n = 12
    Q = 0.5 * (rng.random((n, n)) - 0.5)
    Q[np.diag_indices(n)] = 4.0 + rng.random(n)
    p, A, b = rng.standard_normal(n), rng.standard_normal((3, n)), rng.standard_normal(3)
    S = Q + Q.T
    assert np.all(2 * np.abs(np.diag(S)) > np.sum(np.abs(S), axis=1))
    g, s = S @ p, float(p @ Q @ p)
    sols = []
    for tracking in (True, False):
        model = P.Model(DenseQPOptimizer(), quadratic_mode="canonical", use_graph=True)
        try:
            x = [P.Variable(model) for _ in range(n)]
            Qp, pp, gp, sp_, Ap, bp = (P.Parameter(lambda v=v: v, model) for v in (Q, p, g, s, A, b))
            if tracking:
                P.objective(model, P.Minimize, P.transpose(x - pp) * Qp * (x - pp))
            else:
                P.objective(model, P.Minimize, P.transpose(x) * Qp * x - P.dot(gp, x) + sp_)
            P.constraint(model, Ap * x == bp)
            P.solve(model)
            assert model.objective.mode == ("canonical-form" if tracking else "canonical-sum")
            sols.append(np.array([P.value(model, v) for v in x]))
        finally:
            model.close()
    K = np.block([[S, A.T], [A, np.zeros((3, 3))]])
    d = (U.gamma(65) + U.gamma(n + 1)) * np.max(np.abs(S) @ np.abs(p))
    assert np.linalg.cond(K) < 1e3 and d < 1e-12 and np.linalg.norm(np.linalg.inv(K), np.inf) * d < 1e-11
    assert np.max(np.abs(sols[0] - sols[1])) <= 1e-9
    np.testing.assert_allclose(A @ sols[0], b, atol=1e-9)
    # the KKT solution computed here: the tracking problem's minimiser
    z = np.linalg.solve(K, np.concatenate([g, b]))
    assert np.max(np.abs(sols[0] - z[:n])) <= 1e-9
