"""-m gpu: transpose(x) * Q * x as its canonical function (pmt_quad_form_f64; the "canonical-form" model path and forms inside the
"canonical-sum" path).

The canonical function is defined bit for bit — every off-diagonal coefficient is the sum of exactly two numbers — so the entry point and the
bare model path are compared with `view(np.int64)` equality against the CPU oracle's bilinearmul -> canonicalize -> MOI copy.  Sums are
compared bit for bit with the numpy restatement of the order include/parametron_hip.h fixes for pmt_quad_gram_sum_f64 (tests/test_gpu_lsq_sum.py),
and against fp64 sums / the oracle's canonicalize of the literal sum at the canonical-mode tolerance with the form's magnitude added:
1e-12 * (sum_k |W_k| (2 |A_k|'|A_k|)[j,k] + sum_f |W_f| (|Q_f[j,k]| + |Q_f[k,j]|) + |D|)."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import parametron_jl_amd as P  # noqa: E402
from parametron_jl_amd import _lib  # noqa: E402
from parametron_jl_amd.device import fetch_f64, padded_lda  # noqa: E402
from parametron_jl_amd.moi import _gram_rows  # noqa: E402
from oracle import oracle as O  # noqa: E402
from test_gpu_lsq_sum import bits, restate  # noqa: E402
from test_quad_form_host import restate_form  # noqa: E402

DEV = "cuda:0"
GUARD = 8                                                   # poisoned words behind every output


def dptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------ 1. the entry point, bit for bit
def make_Q(n, special, seed):
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((n, n)) * rng.choice([1.0, -3.0, 1e-3, 40.0], size=(n, n))          # non-symmetric, mixed signs
    if special:
        # +-0.0, denormals and equal-and-opposite pairs (coefficient +0.0: canonicalize! does not prune)
        k = rng.integers(0, 6, size=(n, n))
        Q = np.where(k == 0, 0.0, Q)
        Q = np.where(k == 1, -0.0, Q)
        Q = np.where(k == 2, 5e-324 * rng.integers(1, 1000, size=(n, n)), Q)
        Q = np.where(k == 3, -2.5e-310, Q)
        lo = np.tril_indices(n, -1)
        opp = rng.random(len(lo[0])) < 0.3
        Q[lo[0][opp], lo[1][opp]] = -Q[lo[1][opp], lo[0][opp]]
    return np.ascontiguousarray(Q)


@functools.lru_cache(maxsize=16)
def oracle_form(n, special, seed):
    """(Q, xvar, varmap, the oracle's canonical MOI quadratic terms): a permuted, offset varmap over more variables than x uses"""
    Q = make_Q(n, special, seed)
    rng = np.random.default_rng(seed + 1)
    nvars = n + 9
    xvar = np.sort(rng.choice(np.arange(1, nvars + 1), n, replace=False)).astype(np.int64)
    varmap = (rng.permutation(nvars) + 1 + 100).astype(np.int64)
    at, qt, const = O.Quad().bilinearmul(Q, xvar, xvar).canonicalize().moi(varmap)
    assert len(at) == 0 and const == 0.0
    return Q, xvar, varmap, qt


def device_Q(Q, ldq):
    n = Q.shape[0]
    buf = np.full((n, ldq), 123.456)                        # column j of Q at buf[j, :n]; the padding rows hold junk that must be ignored
    buf[:, :n] = Q.T
    return torch.from_numpy(buf.reshape(-1)).to(DEV)


def run_entry(Q, ldq, xvar, varmap, moi, alpha, want_quad, want_values, want_lin, want_const):
    n = Q.shape[0]
    nq = n * (n + 1) // 2
    dQ = device_Q(Q, ldq)
    dx = torch.from_numpy(xvar).to(DEV)
    dvm = torch.from_numpy(varmap).to(DEV) if varmap is not None else None
    oq = torch.full((3 * nq + GUARD,), -7, dtype=torch.int64, device=DEV) if want_quad else None
    ov = torch.full((nq + GUARD,), -7, dtype=torch.int64, device=DEV) if want_values else None
    ol = torch.full((2 * n + GUARD,), -7, dtype=torch.int64, device=DEV) if want_lin else None
    oc = torch.full((1 + GUARD,), -7, dtype=torch.int64, device=DEV) if want_const else None
    _lib.call("pmt_quad_form_f64", dptr(dQ), ldq, n, dptr(dx), moi, dptr(dvm), alpha, dptr(oq), dptr(ov), dptr(ol), dptr(oc), stream())
    torch.cuda.synchronize()
    out = {}
    for name, t, words in (("quad", oq, 3 * nq), ("values", ov, nq), ("lin", ol, 2 * n), ("const", oc, 1)):
        if t is None:
            continue
        h = t.cpu().numpy()
        assert np.all(h[words:] == -7), "guard words behind %s were written" % name
        out[name] = h[:words]
    return out


def check_entry(out, Q, xvar, varmap, moi, alpha, qt=None):
    n = Q.shape[0]
    coeff, row, col = restate_form(Q, xvar, varmap, moi)
    c1 = restate_form(Q, xvar, varmap, 1)[0]
    if "quad" in out:
        got = out["quad"].view(_lib.QT)
        assert np.array_equal(got["row"], row) and np.array_equal(got["col"], col)
        assert np.array_equal(bits(got["coeff"]), bits(coeff))
        if qt is not None:                                  # the oracle's function itself, word for word
            assert np.array_equal(out["quad"], np.ascontiguousarray(qt).view(np.int64))
    if "values" in out:
        iu = np.triu_indices(n)
        csc = iu[1] * (iu[1] + 1) // 2 + iu[0]
        want = np.empty(len(c1))
        want[csc] = alpha * c1
        assert np.array_equal(out["values"], bits(want))
    if "lin" in out:
        got = out["lin"].view(_lib.LT)
        v = np.asarray(varmap)[xvar - 1] if (moi and varmap is not None) else xvar
        assert np.array_equal(got["var"], v)
        assert np.array_equal(bits(got["coeff"]), bits(np.zeros(n)))                # +0.0
    if "const" in out:
        assert out["const"][0] == 0                                                # +0.0


SIZES = [1, 2, 63, 64, 65, 127, 300, 1000, 2048]
PITCHES = {"tight": lambda n: n, "padded": padded_lda, "odd": lambda n: n + 1 + (n % 2)}


@pytest.mark.parametrize("pitch", sorted(PITCHES))
@pytest.mark.parametrize("n", SIZES)
def test_entry_point_matches_the_oracle(n, pitch):
    Q, xvar, varmap, qt = oracle_form(n, False, 100 + n)
    ldq = int(PITCHES[pitch](n))
    assert ldq >= n and (pitch != "odd" or ldq % 2 == 1)
    # every output, alpha = 1: the values equal the term coefficients bit for bit
    out = run_entry(Q, ldq, xvar, varmap, 1, 1.0, True, True, True, True)
    check_entry(out, Q, xvar, varmap, 1, 1.0, qt)
    assert np.array_equal(np.sort(out["values"]), np.sort(bits(out["quad"].view(_lib.QT)["coeff"])))
    # native form: indices not mapped, the diagonal undoubled (canonicalize! alone)
    out = run_entry(Q, ldq, xvar, varmap, 0, 1.0, True, False, True, False)
    native = O.Quad().bilinearmul(Q, xvar, xvar).canonicalize().terms() if n <= 300 else None
    check_entry(out, Q, xvar, varmap, 0, 1.0, native)


@pytest.mark.parametrize("n", [1, 65, 300, 1000])
def test_entry_point_special_values(n):
    """+-0.0, denormals, equal-and-opposite pairs: nothing pruned, every bit as the oracle's"""
    Q, xvar, varmap, qt = oracle_form(n, True, 500 + n)
    out = run_entry(Q, padded_lda(n), xvar, varmap, 1, 1.0, True, True, True, True)
    check_entry(out, Q, xvar, varmap, 1, 1.0, qt)
    assert len(qt) == n * (n + 1) // 2


@pytest.mark.parametrize("outputs", [(1, 0, 0, 0), (0, 1, 0, 0), (1, 1, 0, 0), (1, 0, 1, 0), (1, 0, 0, 1), (0, 1, 1, 1), (0, 1, 1, 0), (0, 1, 0, 1),
                                     (1, 1, 1, 0), (1, 1, 0, 1), (1, 0, 1, 1), (1, 1, 1, 1)], ids=lambda o: "".join(map(str, o)))
@pytest.mark.parametrize("n", [65, 300])
def test_entry_point_optional_outputs_and_alpha(n, outputs):
    Q, xvar, varmap, qt = oracle_form(n, False, 100 + n)
    for alpha in (1.0, 0.5, -1.0):
        out = run_entry(Q, n + 3, xvar, varmap, 1, alpha, *map(bool, outputs))
        assert sorted(out) == sorted(k for k, on in zip(("quad", "values", "lin", "const"), outputs) if on)
        check_entry(out, Q, xvar, varmap, 1, alpha, qt)


def test_entry_point_full_size():
    """n = 4096 at the padded pitch 4160: all 8 390 656 terms against numpy's Q + Q' (exact)"""
    n, ldq = 4096, 4160
    assert padded_lda(n) == ldq
    Q = make_Q(n, False, 9)
    xvar = np.arange(1, n + 1, dtype=np.int64)
    varmap = (np.arange(n, 0, -1) + 5).astype(np.int64)
    out = run_entry(Q, ldq, xvar, varmap, 1, 1.0, True, True, True, True)
    assert len(out["quad"]) == 3 * 8390656
    check_entry(out, Q, xvar, varmap, 1, 1.0)


# ------------------------------------------------------------------ 2. the bare objective in a model
class Perm(P.MockOptimizer):
    def copy_to(self, backend):
        out = super().copy_to(backend)
        out["variables"] = out["variables"][::-1].copy() + 10
        return out


def bare_model(n, generic=False, use_graph=False, permute=False, extra=3, **kw):
    """transpose(x) * Q * x with a host-updated Q; `generic`: the same objective through the generic canonicalize! node"""
    model = P.Model(Perm() if permute else P.MockOptimizer(), quadratic_mode="canonical", use_graph=use_graph, **kw)
    pre = [P.Variable(model) for _ in range(extra)]                     # x does not start at Variable 1
    x = [P.Variable(model) for _ in range(n)]
    st = {"Q": make_Q(n, False, 31)}
    Q = P.Parameter(lambda: st["Q"], model)
    expr = P.transpose(x) * Q * x
    P.objective(model, P.Minimize, expr.canonicalize() if generic else expr)
    return model, st, np.arange(extra + 1, extra + n + 1, dtype=np.int64), len(pre) + n


def solved(model):
    P.solve(model)
    f = model.objective.f
    return f.quadratic_terms.copy(), f.affine_terms.copy(), float(f.constant)


@pytest.mark.parametrize("use_graph", [False, True], ids=["stream", "graph"])
@pytest.mark.parametrize("permute", [False, True], ids=["identity", "permuted"])
def test_bare_form_model(use_graph, permute):
    n = 640                                                 # 409 600 host-updated elements: beyond the small plan (262 144)
    model, st, xvar, nvars = bare_model(n, use_graph=use_graph, permute=permute)
    ref, rst, _, _ = bare_model(n, generic=True, use_graph=use_graph, permute=permute)
    try:
        nbytes = []
        for it in range(3):
            if it:
                st["Q"] = make_Q(n, it == 2, 40 + it)       # the callback's value changes (the last one with +-0.0 and denormals)
                rst["Q"] = st["Q"]
            gq, gl, gc = solved(model)
            rq, rl, rc = solved(ref)
            assert model.objective.mode == "canonical-form" and not model._small
            assert ref.objective.mode == "literal" and ref.objective.expr.builder == "canonicalize!"
            assert len(gl) == 0 and gc == 0.0 and len(gq) == n * (n + 1) // 2
            varmap = np.asarray(model.model_var_to_optimizer, dtype=np.int64)
            assert np.array_equal(varmap, (np.arange(nvars, 0, -1) + 10) if permute else np.arange(1, nvars + 1))
            # (a) the oracle
            at, qt, const = O.Quad().bilinearmul(st["Q"], xvar, xvar).canonicalize().moi(varmap)
            assert len(at) == 0 and const == 0.0
            assert np.array_equal(gq.view(np.int64), np.ascontiguousarray(qt).view(np.int64))
            # (b) the generic path: bilinear + canonicalize! node + pack
            assert np.array_equal(gq.view(np.int64), rq.view(np.int64)) and len(rl) == 0 and rc == 0.0
            nbytes.append((model.device().bytes_allocated(), ref.device().bytes_allocated()))
        assert len(set(nbytes)) == 1, "plan memory grew across solves: %r" % (nbytes,)
        # the n^2-term literal buffer (and the canonicalize! node's permutation) is never allocated
        assert nbytes[0][1] - nbytes[0][0] >= 24 * n * n
    finally:
        model.close()
        ref.close()


@pytest.mark.parametrize("sense", ["Minimize", "Maximize"])
def test_bare_form_device_handoff(sense):
    """handoff="device": P's CSC values straight from the node, with the hand-off's alpha; equal to the generic path's P bit for bit"""
    n = 640

    def build(generic):
        model = P.Model(P.MockOptimizer(variable_offset=2), quadratic_mode="canonical", handoff="device")
        x = [P.Variable(model) for _ in range(n)]
        st = {"Q": make_Q(n, False, 61)}
        Q = P.Parameter(lambda: st["Q"], model)
        expr = P.transpose(x) * Q * x
        P.objective(model, P.Minimize if sense == "Minimize" else P.Maximize, expr.canonicalize() if generic else expr)
        return model, st
    a, sa = build(False)
    b, sb = build(True)
    try:
        for it in range(2):
            if it:
                sa["Q"] = sb["Q"] = make_Q(n, False, 62)
            P.solve(a)
            P.solve(b)
            assert a.objective.mode == "canonical-form" and "P_values" in a.objective.dev
            assert b.objective.mode == "literal"
            qa, qb = a.device_qp.fetch(), b.device_qp.fetch()
            assert np.array_equal(qa["P"][1], qb["P"][1]) and np.array_equal(qa["P"][2], qb["P"][2])
            assert np.array_equal(bits(qa["P"][0]), bits(qb["P"][0]))
            c1 = restate_form(sa["Q"], np.arange(1, n + 1))[0]
            iu = np.triu_indices(n)
            want = np.empty(len(c1))
            want[iu[1] * (iu[1] + 1) // 2 + iu[0]] = (-1.0 if sense == "Maximize" else 1.0) * c1
            assert np.array_equal(bits(qa["P"][0]), bits(want))
            assert np.all(qa["q"] == 0.0) and qa["r"] == 0.0
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 3. forms in weighted sums
SHAPES = [(80, 50), (40000, 40), (500, 100), (4096, 512), (2048, 2304), (600, 4200)]       # every form of the Gram node (tests/test_gpu_lsq_sum.py)


class SumProblem:
    """objective kinds:
      'qp'        transpose(x)*Q*x + dot(c, x) + s                      (the reference's own model test, forms only)
      'weighted'  lam * (transpose(x)*Q*x) + dot(x - p, x - p)
      'lsq+form'  dot(r, r) + transpose(x)*Q*x
      'form+lsq'  transpose(x)*Q*x + dot(r, r)
      'two'       0.5 * dot(r, r) - w * (transpose(x)*Q*x) + transpose(x)*Q2*x + lam * dot(x, x)"""

    def __init__(self, rows, n, kind, use_graph=False, seed=0):
        self.rng = rng = np.random.default_rng(seed)
        self.kind, self.n = kind, n
        self.model = m = P.Model(P.MockOptimizer(), quadratic_mode="canonical", use_graph=use_graph)
        self.x = x = [P.Variable(m) for _ in range(n)]
        self.st = st = {"A": rng.random((rows, n)) - 0.5, "b": rng.random(rows), "Q": rng.standard_normal((n, n)), "Q2": rng.standard_normal((n, n)),
                        "lam": 0.25, "w": 1.5, "p": rng.random(n), "c": rng.random(n), "s": 0.75}
        Q = P.Parameter(lambda: st["Q"], m)
        form = P.transpose(x) * Q * x
        if kind in ("lsq+form", "form+lsq", "two"):
            A = P.Parameter(lambda: st["A"], m)
            b = P.Parameter(lambda: st["b"], m)
            r = A * x - b
        if kind == "qp":
            c = P.Parameter(lambda: st["c"], m)
            s = P.Parameter(lambda: st["s"], m)
            expr = form + P.dot(c, x) + s
        elif kind == "weighted":
            lam = P.Parameter(lambda: st["lam"], m)
            p = P.Parameter(lambda: st["p"], m)
            expr = lam * form + P.dot(x - p, x - p)
        elif kind == "lsq+form":
            expr = P.dot(r, r) + form
        elif kind == "form+lsq":
            expr = form + P.dot(r, r)
        else:
            w = P.Parameter(lambda: st["w"], m)
            lam = P.Parameter(lambda: st["lam"], m)
            Q2 = P.Parameter(lambda: st["Q2"], m)
            expr = 0.5 * P.dot(r, r) - w * form + P.bilinear(x, Q2, x) + lam * P.dot(x, x)
        P.objective(m, P.Minimize, expr)

    def perturb(self):
        st, rng = self.st, self.rng
        st["A"] = rng.random(st["A"].shape) - 0.5
        for k in ("b", "p", "c"):
            st[k] = rng.random(st[k].shape)
        for k in ("Q", "Q2"):
            st[k] = rng.standard_normal(st[k].shape)
        st["lam"], st["w"], st["s"] = float(rng.uniform(0.1, 2)), float(rng.uniform(-2, 2)), float(rng.standard_normal())

    def terms(self):
        """(kind, W, source) in expression order"""
        st = self.st
        return {"qp": [("form", 1.0, "Q"), ("linear", 1.0, st["c"]), ("constant", 1.0, st["s"])],
                "weighted": [("form", 1.0 * st["lam"], "Q"), ("diag", 1.0, (st["p"], -1))],
                "lsq+form": [("block", 1.0, "A"), ("form", 1.0, "Q")],
                "form+lsq": [("form", 1.0, "Q"), ("block", 1.0, "A")],
                "two": [("block", 0.5, "A"), ("form", -1.0 * st["w"], "Q"), ("form", 1.0, "Q2"), ("diag", 1.0 * st["lam"], (None, 0))]}[self.kind]

    def solve(self):
        P.solve(self.model)
        f = self.model.objective.f
        return f.quadratic_terms.copy(), f.affine_terms.copy(), float(f.constant)

    def gram_outputs(self, first):
        """the least-squares block's own Gram outputs on the model's device buffers (row-major coefficients as block 1, CSC values later)"""
        g = [t.r for t in self.model.objective.lsq_terms if t.kind == "block"][0]
        n = self.n
        nq = n * (n + 1) // 2
        ws = torch.zeros(max(2, int(_lib.load().pmt_quad_gram_workspace_bytes(_gram_rows(g), n)) // 8 + 1), dtype=torch.float64, device=DEV)
        lin = torch.empty(2 * n, dtype=torch.int64, device=DEV)
        cc = torch.empty(1, dtype=torch.float64, device=DEV)
        args = (C.c_void_p(g.mat.buf), g.mat.lda, _gram_rows(g), n, C.c_void_p(g.xvars.buf), C.c_void_p(g.vec.buf), g.sign)
        vm = C.c_void_p(self.model._varmap_buf)
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

    def check(self, got):
        gq, gl, gc = got
        n, st = self.n, self.st
        iu = np.triu_indices(n)
        csc = iu[1] * (iu[1] + 1) // 2 + iu[0]
        assert self.model.objective.mode == "canonical-sum" and not self.model._small
        assert np.array_equal(gq["row"], iu[0] + 1) and np.array_equal(gq["col"], iu[1] + 1)
        assert np.array_equal(gl["var"], np.arange(1, n + 1))                  # the canonical-sum contract: n linear terms
        desc = self.terms()
        # fp64 sums at the canonical-mode tolerance, the form's magnitude added
        ref, tol, ref_lin, ref_c = np.zeros((n, n)), np.zeros((n, n)), np.zeros(n), 0.0
        for kind, W, src in desc:
            if kind == "block":
                A, cvec = st[src], 0.0 - st["b"]
                ref += W * 2 * (A.T @ A)
                tol += abs(W) * 2 * (abs(A).T @ abs(A))
                ref_lin += W * 2 * (A.T @ cvec)
                ref_c += W * float(cvec @ cvec)
            elif kind == "form":
                Qh = st[src]
                ref += W * (Qh + Qh.T)
                tol += abs(W) * (abs(Qh) + abs(Qh).T)
            elif kind == "diag":
                v, sign = src
                ref[np.diag_indices(n)] += 2 * W
                tol[np.diag_indices(n)] += 2 * abs(W)
                if v is not None:
                    ref_lin += W * 2 * (sign * v)
                    ref_c += W * float(v @ v)
            elif kind == "linear":
                ref_lin += W * src
            else:
                ref_c += W * src
        assert np.all(np.abs(gq["coeff"] - ref[iu]) <= 1e-12 * tol[iu] + 1e-300), "quadratic coefficients outside the tolerance"
        np.testing.assert_allclose(gl["coeff"], ref_lin, rtol=1e-9, atol=1e-9 * (1 + np.abs(ref_lin).max()))
        np.testing.assert_allclose(gc, ref_c, rtol=1e-9, atol=1e-9)
        # bits: the header's order applied to the blocks' own outputs; a form's outputs are exact (Q + Q', zero lin and constant)
        terms, first = [], True
        for kind, W, src in desc:
            if kind == "block":
                terms.append(("block", W, self.gram_outputs(first)))
                first = False
            elif kind == "form":
                c1 = restate_form(st[src], np.arange(1, n + 1))[0]
                if first:
                    coeff = c1
                else:
                    coeff = np.empty(len(c1))
                    coeff[csc] = c1
                terms.append(("block", W, (coeff, np.zeros(n), 0.0)))
                first = False
            else:
                terms.append((kind, W, src))
        coeff, lin, const = restate(n, terms)
        assert np.array_equal(bits(gq["coeff"]), bits(coeff)), "quadratic coefficients differ from the restatement"
        assert np.array_equal(bits(gl["coeff"]), bits(lin)), "linear coefficients differ from the restatement"
        assert bits([gc])[0] == bits([const])[0], "constant differs from the restatement"
        return tol


@pytest.mark.parametrize("use_graph", [False, True], ids=["stream", "graph"])
@pytest.mark.parametrize("kind", ["qp", "weighted"])
def test_sums_of_forms_only(kind, use_graph):
    n = 600
    prob = SumProblem(8, n, kind, use_graph=use_graph, seed=n + len(kind))
    try:
        for it in range(3):
            if it:
                prob.perturb()
            got = prob.solve()
            tol = prob.check(got)
            # the oracle's canonicalize of the literal sum
            st, xvar = prob.st, np.arange(1, n + 1, dtype=np.int64)
            form = O.Quad().bilinearmul(st["Q"], xvar, xvar)
            if kind == "qp":
                lin = O.Quad().copy_from_aff(O.vecdot_aff_numbers_vars(st["c"], xvar))
                total = O.Quad().copy_from(form).add_quad(lin)
                total.affine.add_number(st["s"])
            else:
                total = O.Quad().mul_quad_number(form, st["lam"])
                d = O.Quad()
                for j in range(n):                          # dot(x - p, x - p) = sum_j (x_j - p_j)^2
                    a = O.Aff([(1.0, int(xvar[j]))], 0.0).sub_number(st["p"][j])
                    d.add_quad(O.Quad().mul_aff_aff(a, a))
                total.add_quad(d)
            at, qt, const = total.canonicalize().moi()
            gq, gl, gc = got
            iu = np.triu_indices(n)
            assert np.array_equal(gq["row"], qt["row"]) and np.array_equal(gq["col"], qt["col"])
            assert np.all(np.abs(gq["coeff"] - qt["coeff"]) <= 1e-12 * tol[iu])
            full = np.zeros(n)
            full[at["var"] - 1] = at["coeff"]               # (the oracle's literal sum has no linear terms where the sum has none)
            np.testing.assert_allclose(gl["coeff"], full, rtol=1e-10, atol=1e-12)
            np.testing.assert_allclose(gc, const, rtol=1e-12, atol=1e-300)
    finally:
        prob.model.close()


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("kind", ["lsq+form", "form+lsq"])
def test_sum_of_a_block_and_a_form(shape, kind):
    rows, n = shape
    prob = SumProblem(rows, n, kind, use_graph=(rows * n + n * n <= 262144), seed=rows + n)
    try:
        for it in range(3):
            if it:
                prob.perturb()
            prob.check(prob.solve())
    finally:
        prob.model.close()


@pytest.mark.parametrize("shape", [(2000, 200), (4096, 512)], ids=["2000x200", "4096x512"])        # both beyond the small plan
@pytest.mark.parametrize("use_graph", [False, True], ids=["stream", "graph"])
def test_sum_of_a_block_and_two_weighted_forms(shape, use_graph):
    rows, n = shape
    prob = SumProblem(rows, n, "two", use_graph=use_graph, seed=3 * rows + n)
    try:
        nbytes = set()
        for it in range(3):
            if it:
                prob.perturb()
            prob.check(prob.solve())
            nbytes.add(prob.model.device().bytes_allocated())
        assert len(nbytes) == 1
    finally:
        prob.model.close()


@pytest.mark.parametrize("shape", [(80, 50), (500, 100)], ids=["80x50", "500x100"])
@pytest.mark.parametrize("kind", ["lsq+form", "form+lsq"])
def test_block_and_form_against_the_oracle(shape, kind):
    """the oracle's canonicalize of the literal sum: indices exactly, coefficients within the tolerance of the module docstring"""
    rows, n = shape
    prob = SumProblem(rows, n, kind, use_graph=True, seed=rows + 7 * n)
    try:
        for it in range(2):
            if it:
                prob.perturb()
            gq, gl, gc = got = prob.solve()
            tol = prob.check(got)
            st, xvar = prob.st, np.arange(1, n + 1, dtype=np.int64)
            w = O.LsqWorkspace(n, rows, 1)
            w.eval_objective(np.asfortranarray(st["A"]).reshape(-1, order="F"), st["b"], xvar)
            form = O.Quad().bilinearmul(st["Q"], xvar, xvar)
            total = O.Quad().copy_from(w.objective).add_quad(form) if kind == "lsq+form" else O.Quad().copy_from(form).add_quad(w.objective)
            at, qt, const = total.canonicalize().moi()
            iu = np.triu_indices(n)
            assert np.array_equal(gq["row"], qt["row"]) and np.array_equal(gq["col"], qt["col"]) and np.array_equal(gl["var"], at["var"])
            assert np.all(np.abs(gq["coeff"] - qt["coeff"]) <= 1e-12 * tol[iu])
            np.testing.assert_allclose(gl["coeff"], at["coeff"], rtol=1e-10, atol=1e-12)
            np.testing.assert_allclose(gc, const, rtol=1e-12)
    finally:
        prob.model.close()


def test_full_size_block_plus_form():
    """dot(r, r) + transpose(x)*Q*x at 4096 x 4096: the literal expansion (4096^3 + 4096^2 terms) cannot be built; sampled long-double sums"""
    n, rows = 4096, 4096
    model = P.Model(P.MockOptimizer(), quadratic_mode="canonical")
    try:
        x = [P.Variable(model) for _ in range(n)]
        A = P.DeviceUniformParameter((rows, n), 1, model, advance=False)
        b = P.DeviceUniformParameter((rows,), 2, model, advance=False)
        Q = P.DeviceUniformParameter((n, n), 3, model, scale=8.0, advance=False)
        r = A * x - b
        P.objective(model, P.Minimize, P.dot(r, r) + P.transpose(x) * Q * x)
        for _ in range(2):
            P.solve(model)
        assert model.objective.mode == "canonical-sum"
        assert Q._dev.lda == 4160
        gq = model.objective.f.quadratic_terms.copy()
        ctx = model.device()
        Ah = fetch_f64(ctx, A._dev.buf, A._dev.lda * n).reshape(n, A._dev.lda)[:, :rows]          # column j = row j here
        Qh = fetch_f64(ctx, Q._dev.buf, Q._dev.lda * n).reshape(n, Q._dev.lda)[:, :n].T           # Qh[j, k] = Q[j, k]
        ctx.synchronize()
        rng = np.random.default_rng(3)
        iu = np.triu_indices(n)
        pick = rng.choice(len(iu[0]), 1 << 16, replace=False)
        j, k = iu[0][pick], iu[1][pick]
        assert np.array_equal(gq["row"][pick], j + 1) and np.array_equal(gq["col"][pick], k + 1)
        want_ld = np.zeros(len(pick), dtype=np.longdouble)
        tol = np.zeros(len(pick))
        for s in range(0, len(pick), 4096):
            a, bb = Ah[j[s:s + 4096]], Ah[k[s:s + 4096]]
            want_ld[s:s + 4096] += 2 * np.einsum("ij,ij->i", a.astype(np.longdouble), bb.astype(np.longdouble))
            tol[s:s + 4096] += 2 * np.einsum("ij,ij->i", np.abs(a), np.abs(bb))
        on = j == k
        form = np.where(on, 2 * Qh[j, k], Qh[j, k] + Qh[k, j])
        want_ld += form.astype(np.longdouble)
        tol += np.abs(Qh[j, k]) + np.abs(Qh[k, j])
        assert np.all(np.abs(gq["coeff"][pick] - want_ld.astype(np.float64)) <= 1e-12 * tol)
        assert np.abs(form).max() > 1.0 and np.abs(gq["coeff"][pick] - (want_ld - form.astype(np.longdouble)).astype(np.float64)).max() > 1e-3
    finally:
        model.close()


# ------------------------------------------------------------------ 4. fallbacks stay what they are
def small_model(build, n=12, mode="canonical", nextra=0, **kw):
    model = P.Model(P.MockOptimizer(), quadratic_mode=mode, **kw)
    x = [P.Variable(model) for _ in range(n)]
    y = [P.Variable(model) for _ in range(n)]
    rng = np.random.default_rng(4)
    vals = {"Q": rng.standard_normal((n, n)), "A": rng.random((20, n)), "b": rng.random(20)}
    Q = P.Parameter(lambda: vals["Q"], model)
    P.objective(model, P.Minimize, build(model, x, y, Q, vals))
    return model, vals


def canonical_of(total):
    at, qt, const = total.canonicalize().moi()
    return qt


def test_fallback_two_different_vectors():
    n = 12
    model, vals = small_model(lambda m, x, y, Q, v: P.transpose(x) * Q * y, n=n, use_graph=True)
    try:
        gq, gl, gc = solved(model)
        assert model.objective.expr.builder == "canonicalize!" and model.objective.mode == "literal"
        assert getattr(model.objective, "form", None) is None
        x, y = np.arange(1, n + 1), np.arange(n + 1, 2 * n + 1)
        qt = canonical_of(O.Quad().bilinearmul(vals["Q"], x, y))
        assert np.array_equal(gq.view(np.int64), np.ascontiguousarray(qt).view(np.int64)) and len(gq) == n * n
    finally:
        model.close()


@pytest.mark.parametrize("case", ["small", "auto", "literal", "host_csc", "repeated-x"])
def test_fallback_modes(case):
    n = 16 if case != "host_csc" else 640
    kw = {"small": {}, "auto": {"mode": "auto", "use_graph": True}, "literal": {"mode": "literal", "use_graph": True},
          "host_csc": {"handoff": "host_csc"}, "repeated-x": {"use_graph": True}}[case]

    def build(m, x, y, Q, v):
        if case == "repeated-x":
            xs = x[:-1] + x[:1]                             # x_1 twice: not one strictly increasing vector
            return P.transpose(xs) * Q * xs
        return P.transpose(x) * Q * x
    model, vals = small_model(build, n=n, **kw)
    try:
        P.solve(model)
        obj = model.objective
        assert obj.plan.form is None and obj.mode == "literal"
        if case == "small":
            assert model._small
        if case in ("auto", "literal"):
            assert obj.expr.builder == "bilinearmul!" and len(obj.f.quadratic_terms) == n * n            # the literal n^2 terms
        else:
            assert obj.expr.builder == "canonicalize!"
        if case in ("small", "repeated-x"):
            xv = np.arange(1, n + 1)
            if case == "repeated-x":
                xv = np.concatenate([xv[:-1], xv[:1]])
            qt = canonical_of(O.Quad().bilinearmul(vals["Q"], xv, xv))
            got = obj.f.quadratic_terms
            assert np.array_equal(got["row"], qt["row"]) and np.array_equal(got["col"], qt["col"])
            if case == "small":
                assert np.array_equal(bits(got["coeff"]), bits(qt["coeff"]))
            else:
                # the repeated variable's pairs are sums of three or four terms: the order of the generic node's sums is not the oracle's;
                # their rounding errors stay below 3 eps * (the sum of the terms' magnitudes), far inside the canonical-mode bar of 1e-12
                mag = canonical_of(O.Quad().bilinearmul(np.abs(vals["Q"]), xv, xv))["coeff"]
                assert np.all(np.abs(got["coeff"] - qt["coeff"]) <= 1e-12 * mag)
    finally:
        model.close()


def test_fallback_form_over_other_variables_than_the_block():
    """dot(r, r) over x plus a form over y: not one canonical sum; the generic canonicalize! node takes the literal sum"""
    n = 12

    def build(m, x, y, Q, v):
        A = P.Parameter(lambda: v["A"], m)
        b = P.Parameter(lambda: v["b"], m)
        r = A * x - b
        return P.dot(r, r) + P.transpose(y) * Q * y
    model, vals = small_model(build, n=n, use_graph=True)
    try:
        gq, gl, gc = solved(model)
        assert model.objective.lsq_terms is None and model.objective.mode == "literal" and model.objective.expr.builder == "canonicalize!"
        x, y = np.arange(1, n + 1, dtype=np.int64), np.arange(n + 1, 2 * n + 1, dtype=np.int64)
        w = O.LsqWorkspace(n, 20, 1)
        w.eval_objective(np.asfortranarray(vals["A"]).reshape(-1, order="F"), vals["b"], x)
        total = O.Quad().copy_from(w.objective).add_quad(O.Quad().bilinearmul(vals["Q"], y, y))
        at, qt, const = total.canonicalize().moi()
        assert np.array_equal(gq["row"], qt["row"]) and np.array_equal(gq["col"], qt["col"])
        np.testing.assert_allclose(gq["coeff"], qt["coeff"], rtol=1e-12, atol=1e-13)
    finally:
        model.close()
