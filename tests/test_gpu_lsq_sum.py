"""-m gpu: weighted sums of least-squares terms as one canonical objective (pmt_quad_gram_sum_f64 and the "canonical-sum" model path).

The entry point is checked bit for bit against a numpy restatement of the order include/parametron_hip.h fixes; the model path against fp64
sums of A'A at the canonical-mode tolerance and, bit for bit, against the same restatement applied to the bare blocks' own Gram outputs."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import parametron_jl_amd as P  # noqa: E402
from parametron_jl_amd import _lib  # noqa: E402
from parametron_jl_amd.device import fetch_f64  # noqa: E402
from parametron_jl_amd.moi import _gram_rows  # noqa: E402
from oracle import oracle as O  # noqa: E402
from lsq_sum_util import tree_sumsq  # noqa: E402

DEV = "cuda:0"


def dptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def restate(n, terms):
    """terms: (kind, W, data) in expression order.  block: data = (coeff, lin, const) with coeff row-major for the first block and CSC for
    the others; diag: (v or None, sign); linear: c; constant: value or None.  Returns (quad coeff row-major, lin coeff, constant)."""
    iu = np.triu_indices(n)
    csc = iu[1] * (iu[1] + 1) // 2 + iu[0]
    blocks = [t for t in terms if t[0] == "block"]
    diags = [t for t in terms if t[0] == "diag"]
    coeff = blocks[0][1] * blocks[0][2][0]
    lin = blocks[0][1] * blocks[0][2][1]
    const = blocks[0][1] * blocks[0][2][2]
    for _, w, (v, q, cc) in blocks[1:]:
        coeff = coeff + w * v[csc]
        lin = lin + w * q
        const = const + w * cc
    if diags:
        d = 2 * diags[0][1]
        for _, w, _ in diags[1:]:
            d = d + 2 * w
        on = iu[0] == iu[1]
        coeff = coeff.copy()
        coeff[on] = coeff[on] + d
    for _, w, (v, sign) in diags:
        if v is not None:
            lin = lin + w * (2 * ((0.0 + v) if sign > 0 else (0.0 - v)))
    for kind, w, c in terms:
        if kind == "linear":
            lin = lin + w * c
    for _, w, (v, sign) in diags:
        if v is not None:
            const = const + w * tree_sumsq(v)
    for kind, w, val in terms:
        if kind == "constant":
            const = const + w * (1.0 if val is None else val)
    return coeff, lin, const


# ------------------------------------------------------------------ 1. the entry point, bit for bit
def _entry_case(n, K, rng, shape_diag=False):
    nq = n * (n + 1) // 2
    iu = np.triu_indices(n)
    q1 = np.zeros(nq, dtype=_lib.QT)
    q1["coeff"] = rng.standard_normal(nq)
    q1["row"], q1["col"] = iu[0] + 7, iu[1] + 7                     # any indices: they must come back unchanged
    l1 = np.zeros(n, dtype=_lib.LT)
    l1["coeff"], l1["var"] = rng.standard_normal(n), np.arange(n) + 3
    c1 = np.array([rng.standard_normal()])
    keep, terms, host = [], [], []

    def dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        keep.append(t)
        return t

    def weight(i):
        scale = float(rng.choice([1.0, -1.0, 0.5, -3.0]))
        if i % 2:
            w = float(rng.uniform(0.1, 2.0))
            return scale, dev(np.array([w])), scale * w
        return scale, None, scale
    dq, dl, dc = dev(q1.view(np.int64)), dev(l1.view(np.int64)), dev(c1)
    for k in range(K):
        scale, wt, W = (1.0, None, 1.0) if shape_diag else weight(k)
        if k == 0:
            terms.append({"kind": _lib.PMT_LSQ_BLOCK, "scale": scale, "weight": dptr(wt).value if wt is not None else None})
            host.append(("block", W, (q1["coeff"], l1["coeff"], c1[0])))
        else:
            v, q, cc = rng.standard_normal(nq), rng.standard_normal(n), rng.standard_normal()
            lq = np.zeros(n, dtype=_lib.LT)
            lq["coeff"] = q
            tv, tq, tc = dev(v), dev(lq.view(np.int64)), dev(np.array([cc]))
            terms.append({"kind": _lib.PMT_LSQ_BLOCK, "scale": scale, "weight": dptr(wt).value if wt is not None else None,
                          "values": tv.data_ptr(), "lin": tq.data_ptr(), "constant": tc.data_ptr()})
            host.append(("block", W, (v, q, cc)))
        # mixed extra terms between the blocks (expression order)
        if k % 2 == 0:
            scale, wt, W = weight(k + 1)
            v = rng.standard_normal(n) if k % 4 == 0 else None
            sign = 1 if k % 3 == 0 else -1
            terms.append({"kind": _lib.PMT_LSQ_DIAG, "scale": scale, "weight": dptr(wt).value if wt is not None else None,
                          "vec": dev(v).data_ptr() if v is not None else None, "sign": sign if v is not None else 0})
            host.append(("diag", W, (v, sign)))
        if k % 3 == 1 or K == 1:
            scale, wt, W = weight(k)
            c = rng.standard_normal(n)
            terms.append({"kind": _lib.PMT_LSQ_LINEAR, "scale": scale, "weight": dptr(wt).value if wt is not None else None, "vec": dev(c).data_ptr()})
            host.append(("linear", W, c))
            scale, wt, W = weight(k + 1)
            val = float(rng.standard_normal()) if k % 2 else None
            terms.append({"kind": _lib.PMT_LSQ_CONSTANT, "scale": scale, "weight": dptr(wt).value if wt is not None else None,
                          "vec": dev(np.array([val])).data_ptr() if val is not None else None})
            host.append(("constant", W, val))
    arr = _lib.lsq_terms(terms)
    _lib.call("pmt_quad_gram_sum_f64", n, C.addressof(arr), len(terms), dptr(dq), dptr(dl), dptr(dc), stream())
    torch.cuda.synchronize()
    gq = dq.cpu().numpy().view(_lib.QT)
    gl = dl.cpu().numpy().view(_lib.LT)
    coeff, lin, const = restate(n, host)
    assert np.array_equal(gq["row"], q1["row"]) and np.array_equal(gq["col"], q1["col"])
    assert np.array_equal(gl["var"], l1["var"])
    assert np.array_equal(bits(gq["coeff"]), bits(coeff)), "quadratic coefficients differ (n=%d, K=%d)" % (n, K)
    assert np.array_equal(bits(gl["coeff"]), bits(lin)), "linear coefficients differ (n=%d, K=%d)" % (n, K)
    assert bits([float(dc.cpu()[0])])[0] == bits([const])[0], "constant differs (n=%d, K=%d)" % (n, K)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300, 2049, 4160])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_entry_point_matches_the_restatement(n, K):
    _entry_case(n, K, np.random.default_rng(1000 * n + K))


@pytest.mark.parametrize("n", [1, 65, 2049])
def test_entry_point_diagonal_shape(n):
    """block 1 alone with the constant weight +1: only the diagonal, lin and the constant change"""
    _entry_case(n, 1, np.random.default_rng(7 + n), shape_diag=True)


# ------------------------------------------------------------------ 2. model parity
OBJECTIVES = ("ridge", "stacked", "tracking", "linear")
SHAPES = [(80, 50), (40000, 40), (500, 100), (4096, 512), (2048, 2304), (600, 4200)]       # every form of the Gram node


class _Problem:
    def __init__(self, rows, n, objective, use_graph=False, seed=0, **kw):
        self.rng = np.random.default_rng(seed)
        rng = self.rng
        self.model = P.Model(P.MockOptimizer(), quadratic_mode="canonical", use_graph=use_graph, **kw)
        m = self.model
        self.x = x = [P.Variable(m) for _ in range(n)]
        rows2 = max(rows // 2 + 3, 70)
        self.st = {"A1": rng.random((rows, n)) - 0.5, "b1": rng.random(rows), "A2": rng.random((rows2, n)) - 0.5, "b2": rng.random(rows2),
                   "lam": 0.25, "w1": 1.5, "p": rng.random(n), "c": rng.random(n), "s": 0.75}
        st = self.st
        A1 = P.Parameter(lambda: st["A1"], m)
        b1 = P.Parameter(lambda: st["b1"], m)
        r1 = A1 * x - b1
        self.kind = objective
        if objective == "ridge":                      # dot(r, r) + lam*dot(x, x)
            lam = P.Parameter(lambda: st["lam"], m)
            expr = P.dot(r1, r1) + lam * P.dot(x, x)
        elif objective == "stacked":                  # w1*dot(r1, r1) + w2*dot(r2, r2)
            A2 = P.Parameter(lambda: st["A2"], m)
            b2 = P.Parameter(lambda: st["b2"], m)
            r2 = A2 * x + b2
            w1 = P.Parameter(lambda: st["w1"], m)
            expr = w1 * P.dot(r1, r1) + 0.5 * P.dot(r2, r2)
        elif objective == "tracking":                 # dot(r, r) + dot(x - p, x - p)
            p = P.Parameter(lambda: st["p"], m)
            expr = P.dot(r1, r1) + P.dot(x - p, x - p)
        else:                                         # transpose(r)*r + dot(c, x) + s
            c = P.Parameter(lambda: st["c"], m)
            s = P.Parameter(lambda: st["s"], m)
            expr = P.transpose(r1) * r1 + P.dot(c, x) + s
        P.objective(m, P.Minimize, expr)

    def perturb(self):
        st, rng = self.st, self.rng
        for k in ("A1", "A2"):
            st[k] = rng.random(st[k].shape) - 0.5
        for k in ("b1", "b2", "p", "c"):
            st[k] = rng.random(st[k].shape)
        st["lam"], st["w1"], st["s"] = float(rng.uniform(0.1, 2)), float(rng.uniform(-2, 2)), float(rng.standard_normal())

    def weights_and_extras(self):
        """(kind, W, source) in expression order, host values of the current solve"""
        st, n = self.st, len(self.x)
        if self.kind == "ridge":
            return [("block", 1.0, "A1"), ("diag", 1.0 * st["lam"], (None, 0))]
        if self.kind == "stacked":
            return [("block", 1.0 * st["w1"], "A1"), ("block", 0.5, "A2")]
        if self.kind == "tracking":
            return [("block", 1.0, "A1"), ("diag", 1.0, (st["p"], -1))]
        return [("block", 1.0, "A1"), ("linear", 1.0, st["c"]), ("constant", 1.0, st["s"])]

    def solve(self):
        P.solve(self.model)
        f = self.model.objective.f
        return f.quadratic_terms.copy(), f.affine_terms.copy(), float(f.constant)

    def bare_outputs(self):
        """the blocks' own Gram outputs on the model's device buffers: pmt_quad_gram_f64 for block 1, pmt_quad_gram_csc_f64 for the rest"""
        ctx = self.model.device()
        blocks = [t.r for t in self.model.objective.lsq_terms if t.kind == "block"]
        n = len(self.x)
        nq = n * (n + 1) // 2
        out = []
        for i, g in enumerate(blocks):
            ws = torch.zeros(max(2, int(_lib.load().pmt_quad_gram_workspace_bytes(_gram_rows(g), n)) // 8 + 1), dtype=torch.float64, device=DEV)
            lin = torch.empty(2 * n, dtype=torch.int64, device=DEV)
            cc = torch.empty(1, dtype=torch.float64, device=DEV)
            vec = C.c_void_p(g.vec.buf) if g.vec is not None else None
            args = (C.c_void_p(g.mat.buf), g.mat.lda, _gram_rows(g), n, C.c_void_p(g.xvars.buf), vec, g.sign if vec else 0)
            if i == 0:
                q = torch.empty(3 * nq, dtype=torch.int64, device=DEV)
                _lib.call("pmt_quad_gram_f64", *args, 1, C.c_void_p(self.model._varmap_buf), dptr(q), dptr(lin), dptr(cc), dptr(ws), stream())
                torch.cuda.synchronize()
                out.append(q.cpu().numpy().view(_lib.QT)["coeff"].copy())
            else:
                v = torch.empty(nq, dtype=torch.float64, device=DEV)
                _lib.call("pmt_quad_gram_csc_f64", *args, C.c_void_p(self.model._varmap_buf), 1.0, dptr(v), None, dptr(lin), dptr(cc), dptr(ws), stream())
                torch.cuda.synchronize()
                out.append(v.cpu().numpy())
            out[-1] = (out[-1], lin.cpu().numpy().view(_lib.LT)["coeff"].copy(), float(cc.cpu()[0]))
        return out

    def check(self, got, sample=None):
        gq, gl, gc = got
        n = len(self.x)
        st = self.st
        iu = np.triu_indices(n)
        assert self.model.objective.mode == "canonical-sum"
        # indices: the canonical upper triangle, row-major, through the identity varmap; lin one term per variable
        assert np.array_equal(gq["row"], iu[0] + 1) and np.array_equal(gq["col"], iu[1] + 1)
        assert np.array_equal(gl["var"], np.arange(1, n + 1))
        # fp64 sums, tolerance 1e-12 * sum_k |W_k| (2 |A_k|'|A_k|)[j,k] (+ |D| on the diagonal)
        desc = self.weights_and_extras()
        ref = np.zeros((n, n))
        tol = np.zeros((n, n))
        ref_lin = np.zeros(n)
        ref_c = 0.0
        for kind, W, src in desc:
            if kind == "block":
                A = st[src]
                b = st["b1"] if src == "A1" else st["b2"]
                cvec = (0.0 - b) if src == "A1" else (0.0 + b)
                ref += W * 2 * (A.T @ A)
                tol += abs(W) * 2 * (abs(A).T @ abs(A))
                ref_lin += W * 2 * (A.T @ cvec)
                ref_c += W * float(cvec @ cvec)
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
        want = ref[iu]
        assert np.all(np.abs(gq["coeff"] - want) <= 1e-12 * tol[iu] + 1e-300), "quadratic coefficients outside the tolerance"
        np.testing.assert_allclose(gl["coeff"], ref_lin, rtol=1e-9, atol=1e-9 * (1 + np.abs(ref_lin).max()))
        np.testing.assert_allclose(gc, ref_c, rtol=1e-9, atol=1e-9)
        # bits: the restatement applied to the bare blocks' outputs
        bare = self.bare_outputs()
        terms, k = [], 0
        for kind, W, src in desc:
            if kind == "block":
                terms.append(("block", W, bare[k]))
                k += 1
            else:
                terms.append((kind, W, src))
        coeff, lin, const = restate(n, terms)
        assert np.array_equal(bits(gq["coeff"]), bits(coeff)), "quadratic coefficients differ from the restatement"
        assert np.array_equal(bits(gl["coeff"]), bits(lin)), "linear coefficients differ from the restatement"
        assert bits([gc])[0] == bits([const])[0], "constant differs from the restatement"


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_model_parity(shape, objective):
    rows, n = shape
    # (80, 50) is a small plan without a graph: the sum path belongs to the larger plans, so that shape replays as a graph
    prob = _Problem(rows, n, objective, use_graph=(rows * n < 262144), seed=rows + n)
    try:
        for it in range(3):
            if it:
                prob.perturb()
            prob.check(prob.solve())
    finally:
        prob.model.close()


@pytest.mark.parametrize("shape", [(80, 50), (500, 100)], ids=["80x50", "500x100"])
@pytest.mark.parametrize("objective", ("ridge", "stacked"))
def test_model_parity_against_the_oracle(shape, objective):
    """the CPU oracle's composition of the per-block LsqWorkspace objectives (mul_quad_number / add_quad / canonicalize, then the MOI copy):
    indices exactly, coefficients within 1e-12 * sum_k |W_k| (2 |A_k|'|A_k|)[j,k]"""
    rows, n = shape
    prob = _Problem(rows, n, objective, use_graph=True, seed=rows + 7 * n)
    try:
        for it in range(3):
            if it:
                prob.perturb()
            gq, gl, gc = prob.solve()
            st, xvar = prob.st, np.arange(1, n + 1, dtype=np.int64)
            w1 = O.LsqWorkspace(n, rows, 1)
            w1.eval_objective(np.asfortranarray(st["A1"]).reshape(-1, order="F"), st["b1"], xvar)
            total = O.Quad()
            tol = np.zeros((n, n))
            if objective == "ridge":
                total.copy_from(w1.objective).add_quad(O.Quad().mul_quad_number(O.Quad().vecdot_vars_vars(xvar, xvar), st["lam"]))
                tol += 2 * (abs(st["A1"]).T @ abs(st["A1"]))
                tol[np.diag_indices(n)] += 2 * st["lam"]
            else:
                r2 = st["A2"].shape[0]
                w2 = O.LsqWorkspace(n, r2, 1)
                w2.eval_objective(np.asfortranarray(st["A2"]).reshape(-1, order="F"), 0.0 - st["b2"], xvar)      # A2*x + b2 = A2*x - (-b2)
                total.mul_quad_number(w1.objective, st["w1"]).add_quad(O.Quad().mul_quad_number(w2.objective, 0.5))
                tol += abs(st["w1"]) * 2 * (abs(st["A1"]).T @ abs(st["A1"])) + 0.5 * 2 * (abs(st["A2"]).T @ abs(st["A2"]))
            at, qt, const = total.canonicalize().moi()
            assert np.array_equal(gq["row"], qt["row"]) and np.array_equal(gq["col"], qt["col"]) and np.array_equal(gl["var"], at["var"])
            iu = np.triu_indices(n)
            assert np.all(np.abs(gq["coeff"] - qt["coeff"]) <= 1e-12 * tol[iu])
            np.testing.assert_allclose(gl["coeff"], at["coeff"], rtol=1e-10, atol=1e-12)
            np.testing.assert_allclose(gc, const, rtol=1e-12)
    finally:
        prob.model.close()


# ------------------------------------------------------------------ 3. identities
def _device_lsq(n, rows, build, overlap_fetch=True):
    model = P.Model(P.MockOptimizer(), quadratic_mode="canonical", overlap_fetch=overlap_fetch)
    x = [P.Variable(model) for _ in range(n)]
    A = P.DeviceUniformParameter((rows, n), 11, model, advance=False)
    b = P.DeviceUniformParameter((rows,), 12, model, advance=False)
    r = A * x - b
    P.objective(model, P.Minimize, build(r, x))
    P.solve(model)
    f = model.objective.f
    out = f.quadratic_terms.copy(), f.affine_terms.copy(), float(f.constant), getattr(model.objective, "mode", None)
    model.close()
    return out


@pytest.mark.parametrize("shape", [(500, 200), (4096, 512)])
def test_identities(shape):
    rows, n = shape
    bq, bl, bc, bmode = _device_lsq(n, rows, lambda r, x: P.dot(r, r), overlap_fetch=False)
    assert bmode == "canonical"
    sq, sl, sc, smode = _device_lsq(n, rows, lambda r, x: P.dot(r, r) + P.dot(x, x))
    assert smode == "canonical-sum"
    iu = np.triu_indices(n)
    on = iu[0] == iu[1]
    assert np.array_equal(sq["row"], bq["row"]) and np.array_equal(sq["col"], bq["col"])
    assert np.array_equal(bits(sq["coeff"][~on]), bits(bq["coeff"][~on]))
    assert np.array_equal(bits(sq["coeff"][on]), bits(bq["coeff"][on] + 2.0))
    assert np.array_equal(sl.view(np.int64), bl.view(np.int64)) and sc == bc
    oq, ol, oc, omode = _device_lsq(n, rows, lambda r, x: 1.0 * P.dot(r, r))
    assert omode == "canonical-sum"
    assert np.array_equal(oq.view(np.int64), bq.view(np.int64)) and np.array_equal(ol.view(np.int64), bl.view(np.int64))
    assert bits([oc])[0] == bits([bc])[0]


# ------------------------------------------------------------------ 4. replay forms
def _ridge_stacked(use_graph, n=300, rows=700, seed=5, permute=False):
    class Perm(P.MockOptimizer):
        def copy_to(self, backend):
            out = super().copy_to(backend)
            out["variables"] = out["variables"][::-1].copy() + 10
            return out
    model = P.Model(Perm() if permute else P.MockOptimizer(), quadratic_mode="canonical", use_graph=use_graph)
    x = [P.Variable(model) for _ in range(n)]
    rng = np.random.default_rng(seed)
    st = {"A1": rng.random((rows, n)), "b1": rng.random(rows), "A2": rng.random((rows // 3, n)), "lam": 0.3, "w": 2.0}
    A1 = P.Parameter(lambda: st["A1"], model)
    b1 = P.Parameter(lambda: st["b1"], model)
    A2 = P.Parameter(lambda: st["A2"], model)
    lam = P.Parameter(lambda: st["lam"], model)
    w = P.Parameter(lambda: st["w"], model)
    r1, r2 = A1 * x - b1, A2 * x
    P.objective(model, P.Minimize, P.dot(r1, r1) + lam * P.dot(x, x) - w * (P.dot(r2, r2) * 0.25))
    return model, st, rng


def _run(model, st, rng, steps=3):
    outs = []
    for it in range(steps):
        if it:
            st["A1"] = rng.random(st["A1"].shape)
            st["lam"], st["w"] = float(rng.uniform(0.1, 1)), float(rng.uniform(0.5, 3))
        P.solve(model)
        f = model.objective.f
        outs.append((f.quadratic_terms.copy(), f.affine_terms.copy(), float(f.constant)))
    return outs


def _same(a, b):
    return all(np.array_equal(np.asarray(x).view(np.int64) if not np.isscalar(x) else bits([x]), np.asarray(y).view(np.int64) if not np.isscalar(y) else bits([y]))
               for x, y in zip(a, b))


def test_replay_forms_agree():
    runs = []
    for use_graph in (False, True):
        model, st, rng = _ridge_stacked(use_graph)
        runs.append(_run(model, st, rng))
        assert model.objective.mode == "canonical-sum"
        model.close()
    for a, b in zip(*runs):
        assert _same(a, b), "stream and graph replays differ"
    # repeated solves with the same values: the same bits
    model, st, rng = _ridge_stacked(False)
    first = _run(model, st, rng, steps=1)[0]
    P.solve(model)
    f = model.objective.f
    assert _same(first, (f.quadratic_terms, f.affine_terms, float(f.constant)))
    model.close()


def test_two_models_on_two_streams():
    """two models (each with its own plan and stream) updated alternately give the bits of one model solved alone"""
    ref, st, rng = _ridge_stacked(False, seed=9)
    want = _run(ref, st, rng, steps=1)[0]
    ref.close()
    ma, _, _ = _ridge_stacked(False, seed=9)
    mb, _, _ = _ridge_stacked(False, seed=9)
    try:
        ma.initialize(); mb.initialize()
        for _ in range(2):
            ma.update(); mb.update()
        for m in (ma, mb):
            f = m.objective.f
            assert _same((f.quadratic_terms, f.affine_terms, float(f.constant)), want)
    finally:
        ma.close(); mb.close()


def test_permuted_varmap_is_honoured():
    model, st, rng = _ridge_stacked(False, permute=True)
    plain, st2, rng2 = _ridge_stacked(False)
    try:
        q, l, c = _run(model, st, rng, steps=1)[0]
        pq, pl, pc = _run(plain, st2, rng2, steps=1)[0]
        vm = model.model_var_to_optimizer
        assert np.array_equal(q["row"], vm[pq["row"] - 1]) and np.array_equal(q["col"], vm[pq["col"] - 1])
        assert np.array_equal(l["var"], vm[pl["var"] - 1])
        assert np.array_equal(bits(q["coeff"]), bits(pq["coeff"])) and np.array_equal(bits(l["coeff"]), bits(pl["coeff"])) and c == pc
    finally:
        model.close(); plain.close()


# ------------------------------------------------------------------ 5. full size (config 2 + lam*dot(x, x) + a 512 x 4096 block)
def test_full_size_config2_sum():
    n, rows, rows2 = 4096, 4096, 512
    model = P.Model(P.MockOptimizer(), quadratic_mode="canonical")
    try:
        x = [P.Variable(model) for _ in range(n)]
        A = P.DeviceUniformParameter((rows, n), 1, model, advance=False)
        b = P.DeviceUniformParameter((rows,), 2, model, advance=False)
        A2 = P.DeviceUniformParameter((rows2, n), 3, model, advance=False)
        lam = P.Parameter(lambda: 0.125, model)
        r, r2 = A * x - b, A2 * x
        P.objective(model, P.Minimize, P.dot(r, r) + lam * P.dot(x, x) + P.dot(r2, r2))      # MemoryError at construction before
        for _ in range(2):
            P.solve(model)
        assert model.objective.mode == "canonical-sum"
        assert A._dev.lda > rows                                                               # the padded layout
        f = model.objective.f
        gq = f.quadratic_terms.copy()
        ctx = model.device()
        Ah = fetch_f64(ctx, A._dev.buf, A._dev.lda * n).reshape(n, A._dev.lda)[:, :rows]          # column j = row j here
        A2h = fetch_f64(ctx, A2._dev.buf, A2._dev.lda * n).reshape(n, A2._dev.lda)[:, :rows2]
        ctx.synchronize()
        rng = np.random.default_rng(3)
        iu = np.triu_indices(n)
        pick = rng.choice(len(iu[0]), 1 << 16, replace=False)
        j, k = iu[0][pick], iu[1][pick]
        assert np.array_equal(gq["row"][pick], j + 1) and np.array_equal(gq["col"][pick], k + 1)
        want = np.zeros(len(pick))
        want_ld = np.zeros(len(pick), dtype=np.longdouble)
        tol = np.zeros(len(pick))
        for M in (Ah, A2h):
            for s in range(0, len(pick), 4096):
                a, bb = M[j[s:s + 4096]], M[k[s:s + 4096]]
                want[s:s + 4096] += 2 * np.einsum("ij,ij->i", a, bb)
                want_ld[s:s + 4096] += 2 * np.einsum("ij,ij->i", a.astype(np.longdouble), bb.astype(np.longdouble))
                tol[s:s + 4096] += 2 * np.einsum("ij,ij->i", np.abs(a), np.abs(bb))
        on = j == k
        want[on] += 2 * 0.125
        want_ld[on] += 2 * 0.125
        tol[on] += 2 * 0.125
        assert np.all(np.abs(gq["coeff"][pick] - want) <= 1e-12 * tol)
        assert np.all(np.abs(gq["coeff"][pick] - want_ld.astype(np.float64)) <= 1e-12 * tol)
        # bits: the restatement from the bare blocks' outputs, on every sampled coefficient
        prob = _Problem.__new__(_Problem)
        prob.model, prob.x = model, x
        bare = prob.bare_outputs()
        csc = k * (k + 1) // 2 + j
        restated = (1.0 * bare[0][0][pick] + 1.0 * bare[1][0][csc])
        restated[on] = restated[on] + 2 * (1.0 * 0.125)
        assert np.array_equal(bits(gq["coeff"][pick]), bits(restated))
    finally:
        model.close()


# ------------------------------------------------------------------ 6. fallbacks unchanged
def _literal_reference(build, n=12, rows=20, seed=4, mode="literal", **kw):
    model = P.Model(P.MockOptimizer(), quadratic_mode=mode, **kw)
    x = [P.Variable(model) for _ in range(n)]
    y = [P.Variable(model) for _ in range(n)]
    rng = np.random.default_rng(seed)
    A = P.Parameter(model, val=rng.random((rows, n)))
    b = P.Parameter(model, val=rng.random(rows))
    lam = P.Parameter(lambda: 0.5, model)
    P.objective(model, P.Minimize, build(A, b, lam, x, y))
    P.solve(model)
    f = model.objective.f
    out = f.quadratic_terms.copy(), f.affine_terms.copy(), float(f.constant), getattr(model.objective, "mode", None)
    model.close()
    return out


def _oracle(n=12, rows=20, seed=4, y_block=False):
    """the same objective composed in the CPU oracle: dot(r, r) (LsqWorkspace) + 0.5 * (dot(x, x) or dot(A*y, A*y))"""
    rng = np.random.default_rng(seed)
    A, b = rng.random((rows, n)), rng.random(rows)
    xvar = np.arange(1, n + 1, dtype=np.int64)
    w1 = O.LsqWorkspace(n, rows, 1)
    w1.eval_objective(np.asfortranarray(A).reshape(-1, order="F"), b, xvar)
    if y_block:
        w2 = O.LsqWorkspace(n, rows, 1)
        w2.eval_objective(np.asfortranarray(A).reshape(-1, order="F"), np.zeros(rows), xvar + n)
        second = w2.objective
    else:
        second = O.Quad().vecdot_vars_vars(xvar, xvar)
    total = O.Quad().copy_from(w1.objective).add_quad(O.Quad().mul_quad_number(second, 0.5))
    return total


def _ridge_build(A, b, lam, x, y):
    r = A * x - b
    return P.dot(r, r) + lam * P.dot(x, x)


def test_fallback_blocks_over_different_variables():
    def build(A, b, lam, x, y):
        r, ry = A * x - b, A * y
        return P.dot(r, r) + lam * P.dot(ry, ry)
    q, l, c, mode = _literal_reference(build, mode="canonical", use_graph=True)
    assert mode == "literal"                                # the generic canonicalize! of the literal expansion
    at, qt, const = _oracle(y_block=True).canonicalize().moi()
    assert np.array_equal(q["row"], qt["row"]) and np.array_equal(q["col"], qt["col"]) and np.array_equal(l["var"], at["var"])
    np.testing.assert_allclose(q["coeff"], qt["coeff"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(l["coeff"], at["coeff"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(c, const, rtol=1e-12)


def test_fallback_auto_mode_stays_literal():
    build = _ridge_build
    q, l, c, mode = _literal_reference(build, mode="auto", use_graph=True)
    assert mode == "literal"
    assert len(q) == 20 * 12 * 12 + 12                     # r * n^2 terms of the residual product, n of dot(x, x)
    at, qt, const = _oracle().moi()
    assert np.array_equal(q.view(np.int64), qt.view(np.int64)) and np.array_equal(l.view(np.int64), at.view(np.int64)) and c == const


def test_fallback_small_plan():
    build = _ridge_build
    q, l, c, mode = _literal_reference(build, mode="canonical")
    assert mode == "literal"                                # a small plan: canonicalize! of the literal expansion, as before
    at, qt, const = _oracle().canonicalize().moi()
    assert np.array_equal(q["row"], qt["row"]) and np.array_equal(q["col"], qt["col"]) and np.array_equal(l["var"], at["var"])
    np.testing.assert_allclose(q["coeff"], qt["coeff"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(l["coeff"], at["coeff"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(c, const, rtol=1e-12)
    # the same tiny shape beyond the small plan (a graph replay): the sum path, whose block 1 is the interpreter's Gram node — the same
    # function to rounding
    gq, gl, gc, gmode = _literal_reference(build, mode="canonical", use_graph=True)
    assert gmode == "canonical-sum"
    qd = {(int(a), int(b_)): v for a, b_, v in zip(q["row"], q["col"], q["coeff"])}
    assert len(qd) == len(gq)
    for a, b_, v in zip(gq["row"], gq["col"], gq["coeff"]):
        np.testing.assert_allclose(v, qd[(int(a), int(b_))], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(gl["coeff"], l["coeff"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(gc, c, rtol=1e-12)
