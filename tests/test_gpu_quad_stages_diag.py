"""-m gpu: horizon stage costs with identity-weighted terms (pmt_quad_stages_diag_f64) and the record mode "canonical-stages" over
objectives with rho*dot(u_t, u_t) stages and ridge terms.

C ABI: the WHOLE images of the outputs — the stages' slices with poisoned words in front of, between and behind them — compared bit for
bit with the numpy restatement of the header's order (tests/quad_stages_diag_util.py); every form stage's slice with what
pmt_quad_form_f64 / pmt_quad_form_shift_f64 followed by pmt_quad_gram_sum_f64 over [block, PMT_LSQ_DIAG, PMT_LSQ_LINEAR] leaves for that
stage alone.  Host API: the horizon sum_t (x_t - r_t)'Q(x_t - r_t) + rho*dot(u_t, u_t) at round 19's smallest shapes (with the row's size
threshold lowered: see SHAPES) and at the smallest shapes at which it fires as it is."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import parametron_jl_amd as P  # noqa: E402
from parametron_jl_amd import _lib  # noqa: E402
import quad_form_shift_util as S  # noqa: E402
import quad_stages_diag_util as D  # noqa: E402
import quad_stages_terms_util as W  # noqa: E402
import test_gpu_quad_stages as G  # noqa: E402
import test_gpu_quad_stages_terms as GT  # noqa: E402
from gpu_util import DEV, POISON_WORD, Guarded, ptr, stream  # noqa: E402

QT, LT = _lib.QT, _lib.LT
bits = G.bits


# ------------------------------------------------------------------ 1. the entry point
class Launch:
    """device inputs (every distinct Q uploaded once, pitch ldq = n + pad with NaN in the padding rows; every weight a device double of its
    own, every vector a device array), the four tables through pmt_quad_stages_diag_check, guarded outputs"""

    def __init__(self, stages, consts, varmap, nterms, nlin, pad=3, shift=0, diags=True):
        self.stages, self.cvals, self.varmap, self.nterms, self.nlin, self.T = stages, consts, varmap, nterms, nlin, len(stages)
        self.keep, mats = [], {}

        def vector(a, dtype=np.float64):
            t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)
            self.keep.append(t)
            return t.data_ptr()

        def scalar(x):
            return None if x is None else vector([x])
        self.rows, self.trows, self.drows = [], [], []
        for st in stages:
            n = len(st["xvar"])
            row = {"Q": None, "ldq": -5, "xvar": vector(st["xvar"], np.int64), "vec": vector(st["v"]) if st["sign"] else None, "n": n,
                   "sign": st["sign"], "quad_at": st["quad_at"], "lin_at": st["lin_at"]}
            if not D.is_identity(st):
                if id(st["Q"]) not in mats:
                    buf = np.full((n, n + pad), np.nan)
                    buf[:, :n] = np.asarray(st["Q"]).T
                    mats[id(st["Q"])] = vector(buf.reshape(-1))
                row.update(Q=mats[id(st["Q"])], ldq=n + pad)
            self.rows.append(row)
            trow = {"scale": st["W"][0], "weight": scalar(st["W"][1])}
            if st["lin"] is not None:
                trow.update(lin_scale=st["lin"][0], lin_weight=scalar(st["lin"][1]), lin_vec=vector(st["lin"][2]))
            self.trows.append(trow)
            d = D.rider(st)
            self.drows.append({} if d is None else {"scale": d[0], "weight": scalar(d[1]), "vec": vector(d[2]) if d[3] else None, "sign": d[3]})
        self.dvm = torch.from_numpy(np.ascontiguousarray(varmap, dtype=np.int64)).to(DEV)
        self.arr, self.tarr = _lib.quad_stages(self.rows), _lib.quad_stage_terms(self.trows)
        self.darr = _lib.quad_stage_diags(self.drows) if diags else None
        self.carr = _lib.quad_stage_consts([{"scale": k[0], "weight": scalar(k[1]), "value": scalar(k[2])} for k in consts])
        _lib.call("pmt_quad_stages_diag_check", C.addressof(self.arr), C.addressof(self.tarr), C.addressof(self.darr) if diags else None, self.T,
                  C.addressof(self.carr), len(consts), nterms, nlin)
        up = lambda a: torch.from_numpy(np.frombuffer(a, dtype=np.uint8).copy()).to(DEV)
        self.table, self.ttable, self.ctable = up(self.arr), up(self.tarr), up(self.carr)
        self.dtable = up(self.darr) if diags else None
        self.quad, self.lin = Guarded(3 * nterms, shift=shift), Guarded(2 * nlin, shift=shift)
        self.consts, self.const = Guarded(self.T, doubles=True), Guarded(1, doubles=True)

    def run(self, entry="diag"):
        outs = (ptr(self.dvm), self.quad.ptr(), self.lin.ptr(), self.consts.ptr(), self.const.ptr(), stream())
        if entry == "diag":
            _lib.call("pmt_quad_stages_diag_f64", ptr(self.table), ptr(self.ttable), ptr(self.dtable), self.T, ptr(self.ctable), len(self.cvals), *outs)
        else:
            _lib.call("pmt_quad_stages_terms_f64", ptr(self.table), ptr(self.ttable), self.T, ptr(self.ctable), len(self.cvals), *outs)
        return self

    def check(self):
        quad, lin, consts, const = D.images(self.stages, self.cvals, self.varmap, self.nterms, self.nlin, POISON_WORD)
        self.quad.check(quad, "quadratic terms")
        self.lin.check(lin, "linear terms")
        self.consts.check(consts, "stage constants")
        self.const.check(np.array([const]), "constant")
        return quad, lin, consts, const

    host = G.Launch.host

    def check_alone(self, which=None):
        """every form stage's slice against pmt_quad_form_f64 / pmt_quad_form_shift_f64 (moi = 1, alpha = 1.0) followed by
        pmt_quad_gram_sum_f64 over [the block with the stage's weight, PMT_LSQ_DIAG with the rider's, PMT_LSQ_LINEAR], for that stage alone"""
        quad, lin, consts, _ = self.host()
        for t in (range(self.T) if which is None else which):
            r, w, d, n = self.rows[t], self.trows[t], self.drows[t], self.rows[t]["n"]
            if r["Q"] is None:
                continue
            nq = n * (n + 1) // 2
            oq, ol, oc = Guarded(3 * nq, shift=t & 1), Guarded(2 * n), Guarded(1, doubles=True)
            if r["sign"]:
                ws = torch.full((int(_lib.load().pmt_quad_form_shift_workspace_bytes(n)) // 8 + 2,), np.nan, dtype=torch.float64, device=DEV)
                _lib.call("pmt_quad_form_shift_f64", C.c_void_p(r["Q"]), r["ldq"], n, C.c_void_p(r["xvar"]), C.c_void_p(r["vec"]), r["sign"], 1,
                          ptr(self.dvm), 1.0, oq.ptr(), None, ol.ptr(), oc.ptr(), ptr(ws), stream())
            else:
                _lib.call("pmt_quad_form_f64", C.c_void_p(r["Q"]), r["ldq"], n, C.c_void_p(r["xvar"]), 1, ptr(self.dvm), 1.0, oq.ptr(), None,
                          ol.ptr(), oc.ptr(), stream())
            desc = [{"kind": _lib.PMT_LSQ_BLOCK, "scale": w["scale"], "weight": w["weight"]}]
            if d:
                desc.append({"kind": _lib.PMT_LSQ_DIAG, "scale": d["scale"], "weight": d["weight"], "vec": d["vec"], "sign": d["sign"]})
            if "lin_vec" in w:
                desc.append({"kind": _lib.PMT_LSQ_LINEAR, "scale": w["lin_scale"], "weight": w["lin_weight"], "vec": w["lin_vec"]})
            arr = _lib.lsq_terms(desc)
            _lib.call("pmt_quad_gram_sum_f64", n, C.addressof(arr), len(desc), oq.ptr(), ol.ptr(), oc.ptr(), stream())
            oq.check(quad[3 * r["quad_at"]:3 * (r["quad_at"] + nq)], "stage %d: quadratic terms of the two nodes alone" % t)
            ol.check(lin[2 * r["lin_at"]:2 * (r["lin_at"] + n)], "stage %d: linear terms of the two nodes alone" % t)
            oc.check(consts[t:t + 1], "stage %d: constant of the two nodes alone" % t)


def signed_zeros(stages, seed):
    """-0.0 and +0.0 into the linear vectors (quad_form_shift_util.make_case puts them into v with special=True)"""
    rng = np.random.default_rng(seed)
    for st in stages:
        if st["lin"] is not None:
            c = st["lin"][2].copy()
            k = rng.integers(0, 4, size=len(c))
            c[k == 0], c[k == 1] = 0.0, -0.0
            st["lin"] = st["lin"][:2] + (c,)


# weight 1.0, negative, scale only, a Parameter weight, both, and one that is no power of two
MIXED = [(1.0, None), (-1.0, None), (3.0, None), (1.0, 0.7853981633974483), (-2.5, 1.375), (1.0 / 3.0, None)]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256])
def test_identity_stages_bit_for_bit(n):
    """eight identity stages — plain, -v, +v in turn, every other one with a linear term, the weights of MIXED — between two form stages;
    zeros of both signs in v and c_t; odd gaps, so that slices start 8 mod 16"""
    kinds = ["f-"] + ["i0", "i-", "i+", "i0", "i-", "i+", "i-", "i0"] + ["f0"]
    stages, varmap, _, _ = D.make_stages([n] * 10, kinds, 300 + n, weights=MIXED, special=True)
    signed_zeros(stages, n)
    plain = [st for st in stages if D.is_identity(st) and not st["sign"]]
    assert any(st["lin"] is None for st in plain) and any(st["lin"] is not None for st in plain)
    nterms, nlin = D.place(stages, [1, 2, 1, 0, 3, 1, 1, 2, 1, 0, 3])
    assert any(st["quad_at"] & 1 for st in stages if D.is_identity(st)) and any(st["lin_at"] & 1 for st in stages if D.is_identity(st))
    L = Launch(stages, W.make_consts(2), varmap, nterms, nlin).run()
    quad, lin, consts, _ = L.check()
    for st, c in zip(stages, consts):
        if D.is_identity(st):
            q = quad.view(QT)[st["quad_at"]:st["quad_at"] + n]
            assert np.all(q["coeff"] == 2 * W.weight(st["W"])) and np.array_equal(q["row"], q["col"])
            if not st["sign"]:
                assert bits([c])[0] == 0                                  # +0.0 without v, under any weight
    L.check_alone([0, 9])
    L.run().check()                                                       # a second call over the first one's outputs
    L2 = Launch(stages, W.make_consts(2), varmap, nterms, nlin, diags=False, shift=1).run()     # no rider anywhere: no third table
    L2.check()


def test_a_nan_weight_stays_in_its_stage():
    kinds = ["f-", "i-", "f0r-", "i0", "i+", "f+r0", "i-", "f-", "i0", "f0r+"]
    stages, varmap, nterms, nlin = D.make_stages([66, 8] * 5, kinds, 91)
    want_quad, want_lin, want_consts, _ = Launch(stages, [], varmap, nterms, nlin).run().check()
    for bad, what in ((1, "identity"), (3, "identity-parameter"), (2, "rider")):
        poisoned = [dict(st) for st in stages]
        if what == "rider":
            poisoned[bad]["diag"] = (1.0, np.nan) + poisoned[bad]["diag"][2:]
        else:
            poisoned[bad]["W"] = (np.nan, None) if what == "identity" else (2.0, np.nan)
        quad, lin, consts, const = Launch(poisoned, [], varmap, nterms, nlin).run().host()
        st = stages[bad]
        n = len(st["xvar"])
        mq, ml = np.zeros(nterms, dtype=bool), np.zeros(nlin, dtype=bool)
        mq[st["quad_at"]:st["quad_at"] + D.nquad(st)] = True
        ml[st["lin_at"]:st["lin_at"] + n] = True
        gq, wq, gl, wl = quad.view(QT), want_quad.view(QT), lin.view(LT), want_lin.view(LT)
        assert np.array_equal(gq["row"], wq["row"]) and np.array_equal(gq["col"], wq["col"]) and np.array_equal(gl["var"], wl["var"])
        assert np.array_equal(bits(gq["coeff"][~mq]), bits(wq["coeff"][~mq])) and np.array_equal(bits(gl["coeff"][~ml]), bits(wl["coeff"][~ml]))
        if what == "rider":                                               # the rider's weight reaches the diagonal, lin and the constant
            dj = (gq["row"] == gq["col"]) & mq
            assert np.all(np.isnan(gq["coeff"][dj])) and np.array_equal(bits(gq["coeff"][mq & ~dj]), bits(wq["coeff"][mq & ~dj]))
        else:
            assert np.all(np.isnan(gq["coeff"][mq]))
        if st["sign"] or what == "rider":
            assert np.all(np.isnan(gl["coeff"][ml])) and np.isnan(consts[bad]) and np.isnan(const)
        else:                                                             # W_t * dot(x, x): the weight reaches no linear word, no constant
            assert np.array_equal(bits(gl["coeff"][ml]), bits(wl["coeff"][ml])) and bits(consts)[bad] == 0 and not np.isnan(const)
        others = np.arange(len(stages)) != bad
        assert np.array_equal(bits(consts[others]), bits(want_consts[others]))


@pytest.mark.parametrize("n", [1, 64, 65, 129, 256])
def test_riders_match_the_two_nodes_alone(n):
    """plain and shifted forms; riders without v, with the form's sign and with another vector of the other sign; every other stage with a
    linear term; two stages without a rider in between"""
    kinds = ["f0r0", "f-r-", "f-r+", "f+r0", "f0r-", "f-", "f+r-", "f0r+", "f0", "f-r0"]
    stages, varmap, _, _ = D.make_stages([n] * 10, kinds, 400 + n, weights=MIXED, special=True)
    signed_zeros(stages, n + 1)
    with_lin = [st["lin"] is not None for st in stages]
    assert any(a and st["diag"] for a, st in zip(with_lin, stages)) and any(not a and st["diag"] for a, st in zip(with_lin, stages))
    nterms, nlin = D.place(stages, [1, 0, 1, 2, 1, 1, 0, 3, 1, 1, 2])
    L = Launch(stages, W.make_consts(1), varmap, nterms, nlin).run()
    L.check()
    L.check_alone()


def test_a_table_without_diagonal_terms_writes_the_words_of_the_weighted_launch():
    kinds = ["f-", "f0", "f+", "f0", "f-", "f+", "f0", "f-", "f+"]
    stages, varmap, _, _ = D.make_stages([70, 5, 130, 64, 3, 65, 2, 9, 256], kinds, 77, shared=2)
    nterms, nlin = D.place(stages, [1, 0, 1, 2, 1, 1, 0, 3, 1, 2])
    consts = W.make_consts(3)
    a = Launch(stages, consts, varmap, nterms, nlin).run()
    a.check()
    b = Launch(stages, consts, varmap, nterms, nlin).run("terms")
    c = Launch(stages, consts, varmap, nterms, nlin, diags=False).run()
    for x, y, z in zip(a.host(), b.host(), c.host()):
        assert np.array_equal(bits(x), bits(y)) and np.array_equal(bits(x), bits(z)) if np.asarray(x).dtype == np.float64 else \
            np.array_equal(x, y) and np.array_equal(x, z)
    GT.Launch(stages, consts, varmap, nterms, nlin).run().check()          # and they are the weighted launch's own restatement


@pytest.mark.parametrize("T", [1, 9, 257])
def test_stage_counts(T):
    """one identity stage; nine and 257 stages of all kinds — identity stages first, last and next to each other; with 257 the constant's
    chains hold more than one stage"""
    cycle = ["i-", "i0", "f-r+", "f0", "i+", "f+r0", "f-", "i-", "i0"]
    kinds = [cycle[t % 9] for t in range(T)]
    if T > 1:
        kinds[-1] = "i+"
    n = 70 if T == 9 else 5
    stages, varmap, _, _ = D.make_stages([n] * T, kinds, 500 + T, shared=3)
    nterms, nlin = D.place(stages, [t % 2 for t in range(T)] + [1])
    L = Launch(stages, W.make_consts(2), varmap, nterms, nlin).run()
    _, _, consts, const = L.check()
    L.check_alone(range(0, T, max(1, T // 8)))
    if T == 257:
        assert np.count_nonzero(consts) > T // 2 and const != float(np.sum(consts[:256]))


def test_results_do_not_depend_on_the_stage_count_or_position():
    kinds = ["i-", "f0r-", "f+", "i0", "f-r0", "i+", "f0", "i-", "f-r+"]
    stages, varmap, nterms, nlin = D.make_stages([70, 5, 130, 64, 3, 65, 2, 9, 70], kinds, 78, shared=2)
    consts = W.make_consts(2)
    quad, lin, sc, _ = Launch(stages, consts, varmap, nterms, nlin).run().check()
    perm = [4, 8, 0, 2, 7, 1, 6, 3, 5]
    q2, l2, c2, _ = Launch([stages[k] for k in perm], consts, varmap, nterms, nlin).run().check()
    assert np.array_equal(q2, quad) and np.array_equal(l2, lin) and np.array_equal(bits(c2), bits(sc[perm]))
    for t in (0, 8):
        one = dict(stages[t], quad_at=0, lin_at=0)
        q1, l1, c1, k1 = Launch([one], consts, varmap, D.nquad(one), len(one["xvar"])).run().host()
        assert np.array_equal(q1, quad[3 * stages[t]["quad_at"]:][:len(q1)]) and np.array_equal(l1, lin[2 * stages[t]["lin_at"]:][:len(l1)])
        assert bits(c1)[0] == bits(sc)[t] and bits([k1])[0] == bits([W.function_constant(sc[t:t + 1], consts)])[0]


# ------------------------------------------------------------------ 2. the host API
# The row fires from 2^14 literal terms (moi.GROUPS_MIN_LITERAL_TERMS, unchanged) and more than eight vectors.  5 x (57, 8) and 52 x (16, 8)
# are the smallest horizons that fire with a DENSE R (T*(nx^2 + nu^2) = 16565 and 16640 literal terms); with rho*dot(u_t, u_t) the same
# horizons have T*(nx^2 + nu) = 16285 and 13728 literal terms and keep the literal path, a choice of performance, not of correctness: the
# tests at these two shapes lower the threshold, as test_an_eight_form_prefix_is_canonical_groups_with_the_same_words does.  5 x (58, 8) and
# 63 x (16, 8) (16860 and 16632 literal terms) are the smallest such rho-horizons that fire as they are.
SHAPES = {"5x(57,8)": (5, 57, 8), "52x(16,8)": (52, 16, 8), "5x(58,8)": (5, 58, 8), "63x(16,8)": (63, 16, 8)}
LOWERED = ("5x(57,8)", "52x(16,8)")


def lower_threshold(monkeypatch, shape):
    from parametron_jl_amd import moi
    assert moi.GROUPS_MIN_LITERAL_TERMS == 1 << 14
    if shape in LOWERED:
        monkeypatch.setattr(moi, "GROUPS_MIN_LITERAL_TERMS", 1 << 13)


def new_values(shape, seed):
    T, nx, nu = shape
    st = {"Q": S.make_case(nx, seed)[0], "rho": float(np.random.default_rng(seed).uniform(0.3, 3.0)), "lam": 0.625}
    for t in range(T):
        st["r%d" % t] = S.make_case(nx, seed + 2 + t)[1]
    return st


def rho_model(shape, st, spelling="parameter", interleaved=False, optimizer=None, **kw):
    """sum_t (x_t - r_t)'Q(x_t - r_t) + rho*dot(u_t, u_t).  spelling "parameter": rho a scalar Parameter; "number": the Python number
    st["rho"] at build time; "rider": + lam*dot(x_t, x_t) on every x_t as well (lam a scalar Parameter); "dense": rho*I held in a matrix
    Parameter, the workaround; "none": no term over u_t at all"""
    T, nx, nu = shape
    model = P.Model(optimizer or P.MockOptimizer(), **kw)
    sizes = [nx, nu] * T
    if interleaved:
        vecs = [[] for _ in sizes]
        for k in range(max(sizes)):
            for vec, n in zip(vecs, sizes):
                if k < n:
                    vec.append(P.Variable(model))
    else:
        vecs = [[P.Variable(model) for _ in range(n)] for n in sizes]
    Q = P.Parameter(lambda: st["Q"], model)
    rho = P.Parameter(lambda: st["rho"], model) if spelling in ("parameter", "rider") else None
    lam = P.Parameter(lambda: st["lam"], model) if spelling == "rider" else None
    R = P.Parameter(lambda: st["rho"] * np.eye(nu), model) if spelling == "dense" else None
    expr = None
    for t in range(T):
        x, u = vecs[2 * t], vecs[2 * t + 1]
        r = P.Parameter(lambda t=t: st["r%d" % t], model)
        cost = P.transpose(x - r) * Q * (x - r)
        if spelling == "rider":
            cost = cost + lam * P.dot(x, x)
        if spelling == "dense":
            cost = cost + P.transpose(u) * R * u
        elif spelling != "none":
            cost = cost + (st["rho"] if spelling == "number" else rho) * P.dot(u, u)
        expr = cost if expr is None else expr + cost
    P.objective(model, P.Minimize, expr)
    return model, vecs


def described(shape, st, xvars, spelling, rho=None):
    """the model's stages in expression order, as quad_stages_diag_util takes them"""
    out = []
    rho = st["rho"] if rho is None else rho
    for k, xv in enumerate(xvars):
        if k % 2 == 0:
            out.append({"Q": st["Q"], "xvar": xv, "v": st["r%d" % (k // 2)], "sign": -1, "W": (1.0, None), "lin": None,
                        "diag": (1.0, st["lam"], None, 0) if spelling == "rider" else None})
        else:
            out.append({"Q": None, "xvar": xv, "v": None, "sign": 0, "W": (1.0, rho) if spelling != "number" else (rho, None), "lin": None, "diag": None})
    return out


CASES = [(shape, spelling, layout) for shape in LOWERED for spelling in ("parameter", "number", "rider") for layout in ("in-order", "interleaved")] + \
    [("5x(58,8)", "parameter", "in-order"), ("63x(16,8)", "parameter", "interleaved"), ("63x(16,8)", "number", "in-order")]


@pytest.mark.parametrize("shape,spelling,layout", CASES, ids=["-".join(c) for c in CASES])
def test_rho_horizon_model(shape, spelling, layout, monkeypatch):
    """mode "canonical-stages"; T*(nx(nx+1)/2 + nu) quadratic terms; bit for bit the restatement, solve after solve with new values; plan
    memory does not grow; Variables dealt out element by element take the arena and the gather"""
    shp = SHAPES[shape]
    T, nx, nu = shp
    st = new_values(shp, 40)
    rho0 = st["rho"]
    lower_threshold(monkeypatch, shape)
    model, vecs = rho_model(shp, st, spelling, interleaved=(layout == "interleaved"), quadratic_mode="canonical", use_graph=True)
    xvars = G.indices(vecs)
    try:
        nbytes = []
        for it in range(3):
            if it:
                st.update(new_values(shp, 40 + 100 * it))
            gq, gl, gc = G.solved(model)
            assert model.objective.mode == "canonical-stages" and not model._small
            assert [q.mat is None for q in model.objective.plan.stages] == [False, True] * T
            assert (model.objective.plan.stage_diags is not None) == (spelling == "rider")
            assert model.objective.groups_ordered == (layout == "in-order")
            assert len(gq) == T * (nx * (nx + 1) // 2 + nu) and len(gl) == T * (nx + nu)
            varmap = np.asarray(model.model_var_to_optimizer, dtype=np.int64)
            stages = described(shp, st, xvars, spelling, rho=rho0 if spelling == "number" else None)
            quad, lin, const = D.merged(stages, [], varmap)
            assert np.array_equal(gq.view(np.int64), quad.view(np.int64)), "quadratic terms differ from the restatement"
            assert np.array_equal(gl.view(np.int64), lin.view(np.int64)), "linear terms differ from the restatement"
            assert bits([gc])[0] == bits([const])[0], "the constant differs from the restatement"
            nbytes.append(model.device().bytes_allocated())
        assert len(set(nbytes)) == 1, "plan memory grew across solves: %r" % (nbytes,)
    finally:
        model.close()


def test_the_literal_model_is_the_literal_record_with_the_same_function():
    """quadratic_mode="literal" on the same expression is the literal record it was; its terms, added up per pair, are the canonical
    record's within the derived bounds (identity stages: bit for bit).  One variable fewer per x_t and the canonical model keeps the literal
    path too: the row's threshold is where it was"""
    shp = SHAPES["5x(58,8)"]
    T, nx, nu = shp
    st = new_values(shp, 7)
    model, vecs = rho_model(shp, st, quadratic_mode="canonical", use_graph=True)
    lit, _ = rho_model(shp, st, quadratic_mode="literal", use_graph=True)
    below, _ = rho_model(SHAPES["5x(57,8)"], new_values(SHAPES["5x(57,8)"], 7), quadratic_mode="canonical", use_graph=True)
    try:
        gq, gl, gc = G.solved(model)
        lq, ll, lc = G.solved(lit)
        G.solved(below)
        assert model.objective.mode == "canonical-stages" and (below.objective.mode, below.objective.plan.canonicalize) == ("literal", True)
        assert lit.objective.mode == "literal" and len(lq) == T * (nx * nx + nu)
        pairs, byvar = G.literal_function(lq, ll)
        assert len(pairs) == len(gq)
        varmap = np.asarray(model.model_var_to_optimizer, dtype=np.int64)
        stages = described(shp, st, G.indices(vecs), "parameter")
        for sd in stages:
            q, l, _ = D.restate_stage(sd, varmap)
            got = np.array([pairs[(min(r, c), max(r, c))] for r, c in zip(q["row"].tolist(), q["col"].tolist())])
            # (the MOI copy doubles a diagonal term; the literal function's rho*1.0 and the node's (2*W_t) are the same word)
            assert np.array_equal(bits(q["coeff"]), bits(got))
            if D.is_identity(sd):
                assert all(byvar.get(v, 0.0) == 0.0 for v in l["var"].tolist())
        assert abs(gc - lc) <= D.const_bound(stages, [], varmap)
    finally:
        model.close()
        lit.close()
        below.close()


@pytest.mark.parametrize("shape", list(LOWERED))
def test_models_without_diagonal_terms_record_the_calls_they_recorded(shape, monkeypatch):
    """the same horizon without the rho term, and with rho*I held dense: the entry points they called before, never the new one"""
    from parametron_jl_amd import device
    shp = SHAPES[shape]
    st = new_values(shp, 11)
    seen = []
    lower_threshold(monkeypatch, shape)
    real = device.DeviceContext.call
    monkeypatch.setattr(device.DeviceContext, "call", lambda self, name, *a: (seen.append(name), real(self, name, *a))[1])
    for spelling, want in (("dense", "pmt_quad_stages_f64"), ("parameter", "pmt_quad_stages_diag_f64")):
        del seen[:]
        model, _ = rho_model(shp, st, spelling, quadratic_mode="canonical", use_graph=True)
        try:
            G.solved(model)
            assert model.objective.mode == "canonical-stages"
            stage_calls = {n for n in seen if n.startswith("pmt_quad_stages")}
            assert stage_calls == {want}, stage_calls
        finally:
            model.close()


def test_a_solved_rho_horizon_equals_the_dense_workaround():
    """minimize sum_t (x_t - r_t)'Q(x_t - r_t) + rho*dot(u_t, u_t) subject to A z == b (five rows) through the KKT solve of tests/qp_solver.py,
    against the same problem with rho*I held in a dense matrix Parameter (the existing "canonical-stages" launch).  Both objectives hold the
    same function: the x stages are the same launch's words; a u stage's diagonal coefficient is 2*rho in one and 2*(rho*1.0) in the other, the
    same double; the dense statement's off-diagonal terms are 0.0 + 0.0.  So the two KKT systems are equal and each solve's own rounding is
    about cond(K) * 2^-52 * |z| (cond(K) < 1e4 asserted, |z| of order 1: below 1e-11): bound 1e-9, as test_a_solved_horizon_equals_its_dense_statement."""
    from qp_solver import DenseQPOptimizer
    shp = SHAPES["5x(58,8)"]
    T, nx, nu = shp
    rng = np.random.default_rng(3)
    Q = 0.1 * (rng.random((nx, nx)) - 0.5)
    Q[np.diag_indices(nx)] = 4.0 + rng.random(nx)
    st = {"Q": Q, "rho": 1.5, "lam": 0.0}
    for t in range(T):
        st["r%d" % t] = rng.standard_normal(nx)
    nz = T * (nx + nu)
    A, b = rng.standard_normal((5, nz)), rng.standard_normal(5)
    sols = []
    for spelling in ("parameter", "dense"):
        model, vecs = rho_model(shp, st, spelling, optimizer=DenseQPOptimizer(), quadratic_mode="canonical", use_graph=True)
        try:
            z = [v for vec in vecs for v in vec]
            Ap, bp = P.Parameter(lambda: A, model), P.Parameter(lambda: b, model)
            P.constraint(model, Ap * z == bp)
            P.solve(model)
            assert model.objective.mode == "canonical-stages"
            assert (model.objective.plan.stages[1].mat is None) == (spelling == "parameter")
            sols.append(np.array([P.value(model, v) for v in z]))
        finally:
            model.close()
    H = np.zeros((nz, nz))
    g = np.zeros(nz)
    for t in range(T):
        o = t * (nx + nu)
        H[o:o + nx, o:o + nx] = Q
        H[o + nx:o + nx + nu, o + nx:o + nx + nu] = st["rho"] * np.eye(nu)
        g[o:o + nx] = (Q + Q.T) @ st["r%d" % t]
    K = np.block([[H + H.T, A.T], [A, np.zeros((5, 5))]])
    assert np.linalg.cond(K) < 1e4
    assert np.max(np.abs(sols[0] - sols[1])) <= 1e-9
    np.testing.assert_allclose(A @ sols[0], b, atol=1e-9)
    zk = np.linalg.solve(K, np.concatenate([g, b]))
    assert np.max(np.abs(sols[0] - zk[:nz])) <= 1e-9
