"""-m gpu: least-squares objectives over several Variable vectors as one Gram (the stacking node pmt_affine_stack_columns_f64, stacked
residuals as Gram candidates, and weighted sums whose diagonal / linear terms cover part of the union, pmt_quad_gram_sum_sub_f64).

The stacking entry is checked bit for bit against numpy; the model path against the CPU oracle's canonicalize! of the literal dot(r, r)
and, bit for bit, against the same model written with one Parameter holding the host-stacked matrix [A B] over z = [x; u]."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import parametron_jl_amd as P  # noqa: E402
from parametron_jl_amd import _lib  # noqa: E402
from parametron_jl_amd.device import fetch_f64, fetch_terms  # noqa: E402
from oracle import oracle as O  # noqa: E402
from lsq_sum_util import tree_sumsq  # noqa: E402
from sparse_assemble_util import values as special_values  # noqa: E402
from test_gpu_lsq_sum import bits, dptr, stream  # noqa: E402

DEV = "cuda:0"


# ------------------------------------------------------------------ 1. the stacking entry, bit for bit
@pytest.mark.parametrize("rows", [0, 1, 37, 64, 65, 2047, 2048, 2049, 2050, 4097])
def test_stack_entry_matches_numpy(rows):
    """(2047, 2048, 2050: the 2048-row chunk edge in both phases.)  The last source column holds the special-value family — both zeros,
    denormals, the infinities, a NaN with a payload — and is stacked once with each sign: -v flips the sign bit, of a NaN and of a zero too"""
    rng = np.random.default_rng(rows)
    ldas = (rows + 3, rows + 1 if rows % 2 == 0 else rows, rows + 64, rows + 2)  # odd and even source pitches
    hosts = [rng.standard_normal(max(lda * 7, 1)) for lda in ldas[:3]] + [np.full(rows + 2, 7.5)]
    hosts[3][:rows] = special_values(rows, rows)
    srcs = [torch.from_numpy(h).to(DEV) for h in hosts]
    cols = [(k, j) for k in range(3) for j in range(7)] + [(3, 0), (3, 0)]
    perm = rng.permutation(len(cols))
    signs = rng.choice([1, -1], len(cols))
    signs[perm == 21], signs[perm == 22] = -1, 1
    ncols = len(cols)
    for ldo in (rows + 5, max(rows, 1) + 2):                                    # odd / even destination pitch
        out = torch.full((ldo * ncols + 3,), 7.25, dtype=torch.float64, device=DEV)
        addrs = [srcs[cols[p][0]].data_ptr() + 8 * cols[p][1] * ldas[cols[p][0]] for p in perm]
        table = torch.from_numpy(_lib.stack_table(addrs, signs).view(np.int64).copy()).to(DEV)
        _lib.call("pmt_affine_stack_columns_f64", dptr(table), ncols, rows, C.c_void_p(out.data_ptr() + 8), ldo, stream())
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got[0] == 7.25 and np.all(got[1 + ldo * ncols:] == 7.25)
        hs = [s.cpu().numpy() for s in srcs]
        for h, was in zip(hs, hosts):
            assert np.array_equal(bits(h), bits(was)), "a source changed"
        for c, p in enumerate(perm):
            k, j = cols[p]
            v = hs[k][j * ldas[k]:j * ldas[k] + rows]
            want = np.negative(v) if signs[c] < 0 else v
            col = got[1 + c * ldo:1 + (c + 1) * ldo]
            assert np.array_equal(bits(col[:rows]), bits(want)), "column %d" % c
            assert np.all(col[rows:] == 7.25), "padding rows written"


def test_stack_entry_zero_columns():
    out = torch.full((4,), 3.0, dtype=torch.float64, device=DEV)
    _lib.call("pmt_affine_stack_columns_f64", None, 0, 100, dptr(out), 100, stream())
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 3.0)


# ------------------------------------------------------------------ 2. models
def _values(rows, nx, nu, seed):
    rng = np.random.default_rng(seed)
    return {"A": rng.random((rows, nx)) - 0.5, "B": rng.random((rows, nu)) - 0.5, "C": rng.random((rows, 5)) - 0.5, "b": rng.random(rows),
            "lam": 0.375, "c": rng.random(nu), "v": rng.random(nu)}


def _stacked(st, form="Axu-b", use_graph=True, mode="canonical", handoff="moi", u_first=False, extra=None):
    """the model of a residual over x and u (and w); variables in the order x, u, w unless u_first"""
    model = P.Model(P.MockOptimizer(), quadratic_mode=mode, use_graph=use_graph, handoff=handoff)
    nx, nu = st["A"].shape[1], st["B"].shape[1]
    if u_first:
        u = [P.Variable(model) for _ in range(nu)]
        x = [P.Variable(model) for _ in range(nx)]
    else:
        x = [P.Variable(model) for _ in range(nx)]
        u = [P.Variable(model) for _ in range(nu)]
    A = P.Parameter(lambda: st["A"], model)
    B = P.Parameter(lambda: st["B"], model)
    b = P.Parameter(lambda: st["b"], model)
    if form == "Axu-b":
        r = A * x + B * u - b
    elif form == "Ax-b+Bu":
        r = A * x - b + B * u
    elif form == "Axu":
        r = A * x + B * u
    elif form == "Ax-Bu+Cw":
        w = [P.Variable(model) for _ in range(st["C"].shape[1])]
        Cp = P.Parameter(lambda: st["C"], model)
        r = A * x - B * u + Cp * w
    else:
        raise AssertionError(form)
    obj = P.dot(r, r)
    if extra is not None:
        obj = extra(obj, model, u, st)
    P.objective(model, P.Minimize, obj)
    return model, r, x, u


def _prestacked(st, use_graph=True, handoff="moi", sign_b=-1, extra=None):
    """the same objective with one Parameter holding [A B] over z = [x; u]"""
    model = P.Model(P.MockOptimizer(), quadratic_mode="canonical", use_graph=use_graph, handoff=handoff)
    nx, nu = st["A"].shape[1], st["B"].shape[1]
    z = [P.Variable(model) for _ in range(nx + nu)]
    AB = P.Parameter(lambda: np.hstack([st["A"], st["B"]]), model)
    b = P.Parameter(lambda: st["b"], model)
    r = AB * z - b if sign_b < 0 else AB * z
    obj = P.dot(r, r)
    if extra is not None:
        obj = extra(obj, model, z[nx:], st)
    P.objective(model, P.Minimize, obj)
    return model


def _out(model):
    P.solve(model)
    f = model.objective.f
    return f.quadratic_terms.copy(), f.affine_terms.copy(), float(f.constant)


def _same_bits(a, b):
    (qa, la, ca), (qb, lb, cb) = a, b
    assert np.array_equal(qa.view(np.int64), qb.view(np.int64)), "quadratic terms differ"
    assert np.array_equal(la.view(np.int64), lb.view(np.int64)), "affine terms differ"
    assert bits([ca])[0] == bits([cb])[0], "constants differ"


def _oracle_literal(st, form, u_first=False):
    """canonicalize! of the literal dot(r, r) in the CPU oracle, then the MOI copy"""
    A, B, Cm, b = st["A"], st["B"], st["C"], st["b"]
    nx, nu = A.shape[1], B.shape[1]
    xv = np.arange(1, nx + 1) + (nu if u_first else 0)
    uv = np.arange(1, nu + 1) + (0 if u_first else nx)
    wv = np.arange(1, Cm.shape[1] + 1) + nx + nu
    q = O.Quad()
    for i in range(A.shape[0]):
        if form == "Ax-Bu+Cw":
            terms = [(A[i, j], xv[j]) for j in range(nx)] + [(-B[i, j], uv[j]) for j in range(nu)] + [(Cm[i, j], wv[j]) for j in range(Cm.shape[1])]
            const = 0.0
        else:
            terms = [(A[i, j], xv[j]) for j in range(nx)] + [(B[i, j], uv[j]) for j in range(nu)]
            const = 0.0 if form == "Axu" else 0.0 - b[i]
        ri = O.Aff(terms, const)
        q.muladd_aff_aff(ri, ri)
    return q.canonicalize().moi()


@pytest.mark.parametrize("form,u_first", [("Axu-b", False), ("Ax-b+Bu", False), ("Axu", False), ("Ax-Bu+Cw", False), ("Axu-b", True)])
def test_parity_against_the_oracle(form, u_first):
    st = _values(40, 12, 9, seed=3)
    model, _, _, _ = _stacked(st, form, u_first=u_first)
    try:
        for it in range(2):
            if it:
                st.update(_values(40, 12, 9, seed=4))
            gq, gl, gc = _out(model)
            assert model.objective.mode == "canonical"
            at, qt, const = _oracle_literal(st, form, u_first)
            assert np.array_equal(gq["row"], qt["row"]) and np.array_equal(gq["col"], qt["col"])
            assert np.array_equal(gl["var"], at["var"])
            np.testing.assert_allclose(gq["coeff"], qt["coeff"], rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(gl["coeff"], at["coeff"], rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(gc, const, rtol=1e-12)
    finally:
        model.close()


SHAPES = [(40, 12, 9), (1 << 20, 16, 16), (4096, 300, 212), (1000, 1500, 1500), (4090, 200, 100)]


# (the tiny shape without a graph is a small plan: the literal path, test_fallback_auto_mode_and_small_plan)
CASES = [(s, g) for s in SHAPES for g in (True, False) if g or s[0] * (s[1] + s[2]) > 262144]


@pytest.mark.parametrize("shape,use_graph", CASES, ids=["%dx(%d+%d)-%s" % (s + ("graph" if g else "stream",)) for s, g in CASES])
def test_bits_equal_the_prestacked_model(shape, use_graph):
    rows, nx, nu = shape
    st = _values(rows, nx, nu, seed=rows + nx)
    a, _, _, _ = _stacked(st, use_graph=use_graph)
    b = _prestacked(st, use_graph=use_graph)
    try:
        ga, gb = _out(a), _out(b)
        assert a.objective.mode == b.objective.mode == "canonical"
        _same_bits(ga, gb)
    finally:
        a.close(); b.close()


def test_bits_equal_the_prestacked_model_device_handoff():
    st = _values(700, 130, 70, seed=8)
    a, _, _, _ = _stacked(st, handoff="device")
    b = _prestacked(st, handoff="device")
    try:
        for m in (a, b):
            m.initialize()
            m.update()
        assert a.objective.mode == b.objective.mode == "canonical-csc"
        n = 200
        outs = []
        for m in (a, b):
            ctx, dev = m.device(), m.objective.dev
            outs.append((fetch_f64(ctx, dev["P_values"], n * (n + 1) // 2), fetch_terms(ctx, dev["lin"], n, _lib.LT), fetch_f64(ctx, dev["const"], 1)))
            ctx.synchronize()
        for x, y in zip(*outs):
            assert np.array_equal(np.asarray(x).view(np.int64), np.asarray(y).view(np.int64))
    finally:
        a.close(); b.close()


def test_full_size_builds_and_equals_the_prestacked_model():
    """4096 x (2048 + 2048): the literal expansion (1.65 TB) cannot be built; canonical mode takes the stacked Gram"""
    st = _values(4096, 2048, 2048, seed=1)
    a, _, _, _ = _stacked(st, use_graph=False)
    try:
        ga = _out(a)
        assert a.objective.mode == "canonical"
    finally:
        a.close()
    b = _prestacked(st, use_graph=False)
    try:
        _same_bits(ga, _out(b))
    finally:
        b.close()


# ------------------------------------------------------------------ 3. replays
def test_device_regenerated_blocks_match_a_fresh_prestacked_model():
    rows, nx, nu = 600, 150, 90
    model = P.Model(P.MockOptimizer(), quadratic_mode="canonical", use_graph=True)
    x = [P.Variable(model) for _ in range(nx)]
    u = [P.Variable(model) for _ in range(nu)]
    A = P.DeviceUniformParameter((rows, nx), 21, model)
    B = P.DeviceUniformParameter((rows, nu), 22, model)
    b = P.DeviceUniformParameter((rows,), 23, model)
    r = A * x + B * u - b
    P.objective(model, P.Minimize, P.dot(r, r))
    try:
        seen = []
        for _ in range(3):
            got = _out(model)
            assert model.objective.mode == "canonical"
            ctx = model.device()
            st = {"A": A._dev.fetch(ctx), "B": B._dev.fetch(ctx), "b": fetch_f64(ctx, b._dev.buf, rows)}
            ctx.synchronize()
            seen.append(st["A"][0, 0])
            ref = _prestacked(st, use_graph=False)
            try:
                _same_bits(got, _out(ref))
            finally:
                ref.close()
        assert len(set(seen)) == 3, "the blocks were not regenerated"
    finally:
        model.close()


def _constraint_model(st, with_objective, mode="canonical", use_graph=True):
    model = P.Model(P.MockOptimizer(), quadratic_mode=mode, use_graph=use_graph)
    nx, nu = st["A"].shape[1], st["B"].shape[1]
    x = [P.Variable(model) for _ in range(nx)]
    u = [P.Variable(model) for _ in range(nu)]
    A = P.Parameter(lambda: st["A"], model)
    B = P.Parameter(lambda: st["B"], model)
    b = P.Parameter(lambda: st["b"], model)
    r = A * x + B * u - b
    P.constraint(model, r == 0.0 * st["b"])
    if with_objective:
        P.objective(model, P.Minimize, P.dot(r, r))
    return model


def _constraint_out(model):
    P.solve(model)
    c = model._records[-1].f
    return c._terms.copy(), np.asarray(c.constants).copy()


def test_residual_shared_with_a_constraint():
    st = _values(300, 40, 30, seed=6)
    shared = _constraint_model(st, True)
    alone = _constraint_model(st, False)
    literal = _constraint_model(st, True, mode="auto")              # today's combine path everywhere
    try:
        outs = [_constraint_out(m) for m in (shared, alone, literal)]
        assert shared.objective.mode == "canonical"
        for t, c in outs[1:]:
            assert np.array_equal(outs[0][0].view(np.int64), t.view(np.int64)) and np.array_equal(bits(outs[0][1]), bits(c))
        pre = _prestacked(st)
        try:
            _same_bits(_out(shared), _out(pre))
        finally:
            pre.close()
    finally:
        for m in (shared, alone, literal):
            m.close()


def test_constraint_only_model_runs_no_stacking_kernel():
    """stream replays beyond the small plan (every launch profiled): the objective's model runs the stacking node, the constraint-only one
    does not"""
    st = _values(600, 300, 200, seed=7)
    reports = []
    for with_objective in (False, True):
        model = _constraint_model(st, with_objective, use_graph=False)
        try:
            P.profile_enable(True)
            _constraint_out(model)
            _constraint_out(model)
            reports.append(P.profile_report())
        finally:
            P.profile_enable(False)
            model.close()
    assert not any("stack_columns" in k for k in reports[0]), sorted(reports[0])
    assert any("combine" in k for k in reports[0]), sorted(reports[0])
    assert any("stack_columns" in k for k in reports[1]), sorted(reports[1])


# ------------------------------------------------------------------ 4. sums whose simple terms cover part of z
def _effort(obj, model, u, st):
    lam = P.Parameter(lambda: st["lam"], model)
    return obj + lam * P.dot(u, u)


def _linear(obj, model, u, st):
    c = P.Parameter(lambda: st["c"], model)
    return obj + P.dot(c, u)


def _tracking(obj, model, u, st):
    v = P.Parameter(lambda: st["v"], model)
    return obj + P.dot(u - v, u - v)


EXTRAS = {"effort": _effort, "linear": _linear, "tracking": _tracking}


def _gram_of(st):
    """the bare stacked Gram node's outputs: the pre-stacked model's canonical function"""
    ref = _prestacked(st, use_graph=False)
    try:
        q, l, c = _out(ref)
        assert ref.objective.mode == "canonical"
        return q["coeff"].copy(), l["coeff"].copy(), c
    finally:
        ref.close()


@pytest.mark.parametrize("extra", sorted(EXTRAS))
def test_subset_sums(extra):
    rows, nx, nu = 400, 60, 35
    st = _values(rows, nx, nu, seed=11)
    n = nx + nu
    model, _, _, _ = _stacked(st, extra=EXTRAS[extra])
    try:
        for it in range(2):
            if it:
                st.update(_values(rows, nx, nu, seed=12))
                st["lam"] = 1.625
            gq, gl, gc = _out(model)
            assert model.objective.mode == "canonical-sum"
            # bits: the restatement of pmt_quad_gram_sum_sub_f64 over the bare Gram outputs, the subset terms widened to z with the
            # positions of u (nx .. n-1) and nothing elsewhere
            q1, l1, c1 = _gram_of(st)
            iu = np.triu_indices(n)
            coeff, lin, const = q1.copy(), l1.copy(), c1
            on_u = (iu[0] == iu[1]) & (iu[0] >= nx)
            if extra == "effort":
                coeff[on_u] = coeff[on_u] + 2 * (1.0 * st["lam"])
            elif extra == "linear":
                lin[nx:] = lin[nx:] + 1.0 * st["c"]
            else:
                coeff[on_u] = coeff[on_u] + 2 * 1.0
                lin[nx:] = lin[nx:] + 1.0 * (2 * (0.0 - st["v"]))
                const = const + 1.0 * tree_sumsq(st["v"])
            assert np.array_equal(bits(gq["coeff"]), bits(coeff)), "quadratic coefficients differ from the restatement"
            assert np.array_equal(bits(gl["coeff"]), bits(lin)), "linear coefficients differ from the restatement"
            assert bits([gc])[0] == bits([const])[0], "constant differs from the restatement"
            # the oracle: the literal dot(r, r) plus the extra term, canonicalized
            at, qt, oc = _oracle_literal(st, "Axu-b")
            want_q = dict(((int(a), int(b_)), v) for a, b_, v in zip(qt["row"], qt["col"], qt["coeff"]))
            want_l = dict((int(v), cf) for v, cf in zip(at["var"], at["coeff"]))
            for j in range(nx, n):
                if extra in ("effort", "tracking"):
                    want_q[(j + 1, j + 1)] += 2 * (st["lam"] if extra == "effort" else 1.0)
                if extra == "linear":
                    want_l[j + 1] += st["c"][j - nx]
                if extra == "tracking":
                    want_l[j + 1] += -2 * st["v"][j - nx]
            if extra == "tracking":
                oc += float(st["v"] @ st["v"])
            assert np.array_equal(gq["row"], iu[0] + 1) and np.array_equal(gq["col"], iu[1] + 1)
            np.testing.assert_allclose(gq["coeff"], [want_q[(int(a), int(b_))] for a, b_ in zip(gq["row"], gq["col"])], rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(gl["coeff"], [want_l[int(v)] for v in gl["var"]], rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(gc, oc, rtol=1e-12)
    finally:
        model.close()


def test_sub_entry_matches_the_restatement():
    """pmt_quad_gram_sum_sub_f64 directly: block 1 plus a diagonal term with v and a linear term over scattered positions"""
    rng = np.random.default_rng(5)
    n = 70
    nq = n * (n + 1) // 2
    iu = np.triu_indices(n)
    q1 = np.zeros(nq, dtype=_lib.QT)
    q1["coeff"], q1["row"], q1["col"] = rng.standard_normal(nq), iu[0] + 1, iu[1] + 1
    l1 = np.zeros(n, dtype=_lib.LT)
    l1["coeff"], l1["var"] = rng.standard_normal(n), np.arange(n) + 1
    c1 = np.array([rng.standard_normal()])
    pd = np.array([0, 1, 2, 9, 30, 31, 69], dtype=np.int64)
    pl = np.arange(10, 60, 3, dtype=np.int64)
    v, c = rng.standard_normal(len(pd)), rng.standard_normal(len(pl))
    keep = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (q1.view(np.int64), l1.view(np.int64), c1, v, c, np.array([0.7]))]
    dq, dl, dc, dv, dcv, dw = keep
    terms = _lib.lsq_terms([{"kind": _lib.PMT_LSQ_BLOCK, "scale": -2.0},
                            {"kind": _lib.PMT_LSQ_DIAG, "scale": 1.5, "weight": dw.data_ptr(), "vec": dv.data_ptr(), "sign": -1},
                            {"kind": _lib.PMT_LSQ_LINEAR, "scale": 0.5, "vec": dcv.data_ptr()}])
    lists = [None, pd, pl]
    ptrs = (C.c_void_p * 3)(*[p.ctypes.data if p is not None else None for p in lists])
    counts = np.array([0, len(pd), len(pl)], dtype=np.int64)
    _lib.call("pmt_quad_gram_sum_sub_f64", n, C.addressof(terms), 3, C.cast(ptrs, C.c_void_p), counts.ctypes.data_as(C.c_void_p),
              dptr(dq), dptr(dl), dptr(dc), stream())
    torch.cuda.synchronize()
    gq = dq.cpu().numpy().view(_lib.QT)
    gl = dl.cpu().numpy().view(_lib.LT)
    gc = float(dc.cpu()[0])
    W1, Wd, Wl = -2.0, 1.5 * 0.7, 0.5
    coeff = W1 * q1["coeff"]
    on = iu[0] == iu[1]
    listed = np.zeros(n, dtype=bool)
    listed[pd] = True
    sel = on & listed[iu[0]]
    coeff[sel] = coeff[sel] + 2 * Wd
    lin = W1 * l1["coeff"]
    lin[pd] = lin[pd] + Wd * (2 * (0.0 - v))
    lin[pl] = lin[pl] + Wl * c
    const = W1 * c1[0] + Wd * tree_sumsq(v)
    assert np.array_equal(bits(gq["coeff"]), bits(coeff))
    assert np.array_equal(gq["row"], q1["row"]) and np.array_equal(gq["col"], q1["col"])
    assert np.array_equal(bits(gl["coeff"]), bits(lin))
    assert bits([gc])[0] == bits([const])[0]
    del keep


# ------------------------------------------------------------------ 5. fallbacks unchanged
def _literal_bits(st, mode, use_graph, build):
    model = P.Model(P.MockOptimizer(), quadratic_mode=mode, use_graph=use_graph)
    nx, nu = st["A"].shape[1], st["B"].shape[1]
    x = [P.Variable(model) for _ in range(nx)]
    u = [P.Variable(model) for _ in range(nu)]
    A = P.Parameter(lambda: st["A"], model)
    B = P.Parameter(lambda: st["B"], model)
    b = P.Parameter(lambda: st["b"], model)
    P.objective(model, P.Minimize, build(A, B, b, x, u))
    try:
        out = _out(model)
        return out, model.objective.mode
    finally:
        model.close()


def _axu(A, B, b, x, u):
    r = A * x + B * u - b
    return P.dot(r, r)


def test_fallback_auto_mode_and_small_plan():
    st = _values(20, 6, 5, seed=2)
    at, qt, const = _oracle_literal(st, "Axu-b")
    # auto mode: the literal expansion, exactly the oracle's uncombined terms
    (q, l, c), mode = _literal_bits(st, "auto", True, _axu)
    assert mode == "literal" and len(q) == 20 * 11 * 11
    # the small plan: canonicalize! of the literal expansion
    (q, l, c), mode = _literal_bits(st, "canonical", False, _axu)
    assert mode == "literal"
    assert np.array_equal(q["row"], qt["row"]) and np.array_equal(q["col"], qt["col"])
    np.testing.assert_allclose(q["coeff"], qt["coeff"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(c, const, rtol=1e-12)


def test_fallback_overlapping_variables_and_different_sets():
    st = _values(30, 7, 7, seed=9)

    def overlap(A, B, b, x, u):
        r = A * x + B * x - b                                          # the same x twice: not a stacking
        return P.dot(r, r)

    (q, l, c), mode = _literal_bits(st, "canonical", True, overlap)
    assert mode == "literal"
    A, B, b = st["A"], st["B"], st["b"]
    qo = O.Quad()
    for i in range(30):
        ri = O.Aff([(A[i, j], j + 1) for j in range(7)] + [(B[i, j], j + 1) for j in range(7)], 0.0 - b[i])
        qo.muladd_aff_aff(ri, ri)
    at, qt, const = qo.canonicalize().moi()
    assert np.array_equal(q["row"], qt["row"]) and np.array_equal(q["col"], qt["col"])
    np.testing.assert_allclose(q["coeff"], qt["coeff"], rtol=1e-12, atol=1e-13)

    def different(A, B, b, x, u):
        r, s = A * x - b, B * u                                         # blocks over different sets in one sum
        return P.dot(r, r) + P.dot(s, s)

    (_, _, _), mode = _literal_bits(st, "canonical", True, different)
    assert mode == "literal"
