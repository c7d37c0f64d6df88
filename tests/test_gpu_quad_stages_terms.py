"""-m gpu: horizon stage costs with weights, linear terms and constants beside the stages (pmt_quad_stages_terms_f64) and the record mode
"canonical-stages" over such objectives.

C ABI: the WHOLE images of the outputs — the stages' slices with poisoned words in front of, between and behind them — compared bit for
bit with the numpy restatement of the header's order (tests/quad_stages_terms_util.py), and every stage's slice with what
pmt_quad_form_f64 / pmt_quad_form_shift_f64 followed by pmt_quad_gram_sum_f64 leaves for that stage alone.  Host API: the 12-stage horizon
of test_gpu_quad_stages.py written as 0.5*(sum_t (x_t - r_t)'Q(x_t - r_t) + rho*u_t'R u_t) + sum_t dot(c_t, u_t) + s."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import parametron_jl_amd as P  # noqa: E402
from parametron_jl_amd import _lib  # noqa: E402
import quad_form_shift_util as S  # noqa: E402
import quad_stages_terms_util as W  # noqa: E402
import quad_stages_util as U  # noqa: E402
import test_gpu_quad_stages as G  # noqa: E402
from gpu_util import DEV, POISON_WORD, Guarded, ptr, stream  # noqa: E402

QT, LT = _lib.QT, _lib.LT
bits = G.bits


# ------------------------------------------------------------------ 1. the entry point
class Launch(G.Launch):
    """test_gpu_quad_stages.Launch plus the two further tables: every weight and constant value a device double of its own, every linear
    vector a device array, the tables through pmt_quad_stages_terms_check"""

    def __init__(self, stages, consts, varmap, nterms, nlin, pad=3, shift=0):
        super().__init__(stages, varmap, nterms, nlin, pad=pad, shift=shift)
        self.cvals = consts

        def scalar(x):
            if x is None:
                return None
            t = torch.tensor([x], dtype=torch.float64, device=DEV)
            self.keep.append(t)
            return t.data_ptr()
        self.trows = []
        for st in stages:
            row = {"scale": st["W"][0], "weight": scalar(st["W"][1])}
            if st["lin"] is not None:
                dc = torch.from_numpy(np.ascontiguousarray(st["lin"][2], dtype=np.float64)).to(DEV)
                self.keep.append(dc)
                row.update(lin_scale=st["lin"][0], lin_weight=scalar(st["lin"][1]), lin_vec=dc.data_ptr())
            self.trows.append(row)
        self.tarr = _lib.quad_stage_terms(self.trows)
        self.carr = _lib.quad_stage_consts([{"scale": k[0], "weight": scalar(k[1]), "value": scalar(k[2])} for k in consts])
        _lib.call("pmt_quad_stages_terms_check", C.addressof(self.arr), C.addressof(self.tarr), self.T, C.addressof(self.carr), len(consts), nterms, nlin)
        self.ttable = torch.from_numpy(np.frombuffer(self.tarr, dtype=np.uint8).copy()).to(DEV)
        self.ctable = torch.from_numpy(np.frombuffer(self.carr, dtype=np.uint8).copy()).to(DEV)

    def run(self, s=None):
        _lib.call("pmt_quad_stages_terms_f64", ptr(self.table), ptr(self.ttable), self.T, ptr(self.ctable), len(self.cvals), ptr(self.dvm),
                  self.quad.ptr(), self.lin.ptr(), self.consts.ptr(), self.const.ptr(), stream() if s is None else C.c_void_p(s.cuda_stream))
        return self

    def run_unweighted(self):
        G.Launch.run(self)
        return self

    def check(self):
        quad, lin, consts, const = W.images(self.stages, self.cvals, self.varmap, self.nterms, self.nlin, POISON_WORD)
        self.quad.check(quad, "quadratic terms")
        self.lin.check(lin, "linear terms")
        self.consts.check(consts, "stage constants")
        self.const.check(np.array([const]), "constant")
        return quad, lin, consts, const

    def check_alone(self, which=None):
        """every stage's slice against pmt_quad_form_f64 / pmt_quad_form_shift_f64 (moi = 1, alpha = 1.0) followed by pmt_quad_gram_sum_f64 over
        [the block with (scale, weight), PMT_LSQ_LINEAR with (lin_scale, lin_weight, lin_vec)], run for that stage alone"""
        quad, lin, consts, _ = self.host()
        for t in (range(self.T) if which is None else which):
            r, w, n = self.rows[t], self.trows[t], self.rows[t]["n"]
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
            if "lin_vec" in w:
                desc.append({"kind": _lib.PMT_LSQ_LINEAR, "scale": w["lin_scale"], "weight": w["lin_weight"], "vec": w["lin_vec"]})
            arr = _lib.lsq_terms(desc)
            _lib.call("pmt_quad_gram_sum_f64", n, C.addressof(arr), len(desc), oq.ptr(), ol.ptr(), oc.ptr(), stream())
            oq.check(quad[3 * r["quad_at"]:3 * (r["quad_at"] + nq)], "stage %d: quadratic terms of the two nodes alone" % t)
            ol.check(lin[2 * r["lin_at"]:2 * (r["lin_at"] + n)], "stage %d: linear terms of the two nodes alone" % t)
            oc.check(consts[t:t + 1], "stage %d: constant of the two nodes alone" % t)


# scale only, Parameter only, both, -1.0, 0.5, and a weight that is no power of two
MIXED = [(3.0, None), (1.0, 0.7853981633974483), (-2.5, 1.375), (-1.0, None), (0.5, None), (1.0 / 3.0, None)]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 128, 129, 256])
def test_every_tile_edge_bit_for_bit(n):
    """six stages of one size with the signs -1, 0, +1, 0, -1, +1 and the six weights of MIXED, every other one with a linear term (so one
    plain stage under -1.0 without one: -0.0 in its linear terms); zeros of both signs in Q and v; odd gaps around the slices"""
    stages, varmap, _, _ = W.make_stages([n] * 6, [-1, 0, 1, 0, -1, 1], 200 + n, weights=MIXED, special=True)
    assert stages[3]["W"] == (-1.0, None) and stages[3]["lin"] is None and not stages[3]["sign"]
    nterms, nlin = G.place(stages, [1, 2, 1, 0, 3, 1, 3])
    L = Launch(stages, W.make_consts(3), varmap, nterms, nlin).run()
    _, lin, _, _ = L.check()
    at = stages[3]["lin_at"]
    assert np.all(bits(lin.view(LT)["coeff"][at:at + n]) == np.iinfo(np.int64).min)          # -0.0
    L.check_alone()
    L.run().check()                                               # a second call over the first one's outputs


def test_mixed_sizes_in_one_launch_with_odd_offsets():
    ns = [3, 65, 1, 130, 2, 64, 7, 256, 5, 129, 63]
    signs = [-1, 0, 1, -1, 0, 1, 1, -1, 0, 1, -1]
    for shift in (0, 1):
        stages, varmap, _, _ = W.make_stages(ns, signs, 31 + shift, shared=1, interleave=bool(shift))
        nterms, nlin = G.place(stages, [1, 0, 1, 1, 2, 1, 0, 3, 1, 1, 0, 2])
        assert any(st["quad_at"] & 1 for st in stages) and any(not st["quad_at"] & 1 for st in stages)
        L = Launch(stages, W.make_consts(1), varmap, nterms, nlin, pad=0 if shift else 5, shift=shift).run()
        L.check()
        L.check_alone()


@pytest.mark.parametrize("T", [1, 9, "3CUs+5"])
def test_stage_counts(T):
    """one stage; nine; 3 CUs + 5 stages of n = 3, where the persistent loop wraps and the constant's chains hold more than one stage"""
    wrap = T == "3CUs+5"
    T = 3 * G.cu_count() + 5 if wrap else T
    n = 3 if wrap else 70
    stages, varmap, _, _ = W.make_stages([n] * T, [(-1, 0, 1)[t % 3] for t in range(T)], 500 + T, shared=3)
    nterms, nlin = G.place(stages, [t % 2 for t in range(T)] + [1])
    L = Launch(stages, W.make_consts(2), varmap, nterms, nlin).run()
    _, _, consts, const = L.check()
    L.check_alone(range(0, T, max(1, T // 8)))
    if wrap:
        assert T > 256 and np.count_nonzero(consts) > T // 2


def test_three_stages_match_the_two_nodes_alone_with_the_sign_of_zero():
    """n = 65: a shifted stage with a linear term, a plain stage under a negative weight (its linear terms and constant are -0.0, as
    pmt_quad_gram_sum_f64 leaves them), a plain stage with a linear term under a negative weight (-0.0 + W_c*c)"""
    stages, varmap, _, _ = W.make_stages([65] * 3, [-1, 0, 0], 65, weights=[(0.5, 3.0), (-1.0, None), (-3.0, None)], lin_every=2)
    assert stages[1]["lin"] is None and stages[2]["lin"] is not None
    nterms, nlin = G.place(stages, [1, 1, 0, 2])
    L = Launch(stages, [], varmap, nterms, nlin).run()
    _, lin, consts, _ = L.check()
    L.check_alone()
    assert np.all(np.signbit(lin.view(LT)["coeff"][stages[1]["lin_at"]:][:65])) and np.signbit(consts[1]) and consts[1] == 0.0


def test_a_unit_table_writes_the_words_of_the_unweighted_launch():
    stages, varmap, _, _ = W.make_stages([70, 5, 130, 64, 3, 65, 2, 9, 70], [-1, 0, 1, 0, -1, 1, 0, -1, 1], 77, weights=[(1.0, None)], lin_every=0, shared=2)
    nterms, nlin = G.place(stages, [1, 0, 1, 2, 1, 1, 0, 3, 1, 2])
    a = Launch(stages, [], varmap, nterms, nlin).run()
    a.check()
    b = Launch(stages, [], varmap, nterms, nlin).run_unweighted()
    for x, y in zip(a.host(), b.host()):
        assert np.array_equal(bits(x), bits(y)) if np.asarray(x).dtype == np.float64 else np.array_equal(x, y)
    G.Launch.check(b)


def test_results_do_not_depend_on_the_stage_count_or_position():
    stages, varmap, nterms, nlin = W.make_stages([70, 5, 130, 64, 3, 65, 2, 9, 70], [-1, 0, 1, 0, -1, 1, 0, -1, 1], 78, shared=2)
    consts = W.make_consts(2)
    quad, lin, sc, _ = Launch(stages, consts, varmap, nterms, nlin).run().check()
    perm = [4, 8, 0, 2, 7, 1, 6, 3, 5]
    q2, l2, c2, _ = Launch([stages[k] for k in perm], consts, varmap, nterms, nlin).run().check()
    assert np.array_equal(q2, quad) and np.array_equal(l2, lin) and np.array_equal(bits(c2), bits(sc[perm]))
    for t in (0, 8):
        one = dict(stages[t], quad_at=0, lin_at=0)
        n = len(one["xvar"])
        q1, l1, c1, k1 = Launch([one], consts, varmap, n * (n + 1) // 2, n).run().host()
        assert np.array_equal(q1, quad[3 * stages[t]["quad_at"]:][:len(q1)]) and np.array_equal(l1, lin[2 * stages[t]["lin_at"]:][:len(l1)])
        assert bits(c1)[0] == bits(sc)[t]
        assert bits([k1])[0] == bits([W.function_constant(sc[t:t + 1], consts)])[0]


def test_a_nan_weight_stays_in_its_stage():
    stages, varmap, nterms, nlin = W.make_stages([66, 8] * 5, [-1, 0] * 5, 91)
    clean = Launch(stages, [], varmap, nterms, nlin).run()
    want_quad, want_lin, want_consts, _ = clean.check()
    for bad in (4, 7):                                                          # a shifted stage; a plain one with a Parameter weight
        poisoned = [dict(st) for st in stages]
        poisoned[bad]["W"] = (np.nan, None) if bad == 4 else (2.0, np.nan)
        quad, lin, consts, const = Launch(poisoned, [], varmap, nterms, nlin).run().host()
        n = len(stages[bad]["xvar"])
        mq, ml = np.zeros(nterms, dtype=bool), np.zeros(nlin, dtype=bool)
        mq[stages[bad]["quad_at"]:stages[bad]["quad_at"] + n * (n + 1) // 2] = True
        ml[stages[bad]["lin_at"]:stages[bad]["lin_at"] + n] = True
        gq, wq, gl, wl = quad.view(QT), want_quad.view(QT), lin.view(LT), want_lin.view(LT)
        assert np.array_equal(gq["row"], wq["row"]) and np.array_equal(gq["col"], wq["col"]) and np.array_equal(gl["var"], wl["var"])
        assert np.all(np.isnan(gq["coeff"][mq])) and np.array_equal(bits(gq["coeff"][~mq]), bits(wq["coeff"][~mq]))
        assert np.all(np.isnan(gl["coeff"][ml])) and np.array_equal(bits(gl["coeff"][~ml]), bits(wl["coeff"][~ml]))
        others = np.arange(len(stages)) != bad
        assert np.array_equal(bits(consts[others]), bits(want_consts[others])) and np.isnan(consts[bad]) and np.isnan(const)


@pytest.mark.parametrize("count", [0, 1, 32])
def test_constants_beside_the_stages(count):
    """numbers, Parameter values and Parameter weights mixed, added in table order behind the tree"""
    stages, varmap, nterms, nlin = W.make_stages([9, 4] * 5, [-1, 0] * 5, 12)
    consts = W.make_consts(count, seed=count)
    _, _, sc, const = Launch(stages, consts, varmap, nterms, nlin).run().check()
    s = S.chain_tree_sum(sc)
    for k in consts:
        s = s + W.const_value(k)
    assert bits([const])[0] == bits([s])[0] and (count == 0 or const != S.chain_tree_sum(sc))


def test_no_stage_writes_the_constants_only():
    """T == 0: *out_const = the two constants added onto 0.0 and nothing else, whatever the other pointers"""
    consts = [(3.0, None, 0.7), (-0.5, 1.25, None)]
    keep = [torch.tensor([x], dtype=torch.float64, device=DEV) for x in (0.7, 1.25)]
    carr = _lib.quad_stage_consts([{"scale": 3.0, "value": keep[0].data_ptr()}, {"scale": -0.5, "weight": keep[1].data_ptr()}])
    ctable = torch.from_numpy(np.frombuffer(carr, dtype=np.uint8).copy()).to(DEV)
    quad, lin, const = Guarded(6), Guarded(4), Guarded(1, doubles=True)
    _lib.call("pmt_quad_stages_terms_f64", None, None, 0, ptr(ctable), 2, None, quad.ptr(), lin.ptr(), None, const.ptr(), stream())
    quad.check(quad.padding(6), "quadratic terms")
    lin.check(lin.padding(4), "linear terms")
    const.check(np.array([W.function_constant([], consts)]), "constant")
    assert W.function_constant([], consts) == (0.0 + 3.0 * 0.7) + (-0.5 * 1.25) * 1.0


# ------------------------------------------------------------------ 2. the host API
NX, NU, T_H = G.NX, G.NU, G.T_H


def new_values(seed):
    st = G.new_values(seed)
    rng = np.random.default_rng(seed + 999)
    st["rho"], st["s"] = float(rng.uniform(0.3, 3.0)), float(rng.standard_normal())
    for t in range(T_H):
        st["c%d" % t] = rng.standard_normal(NU) * rng.choice([1.0, 20.0], size=NU)
    return st


def weighted_model(st, stages=T_H, interleaved=False, optimizer=None, **kw):
    """0.5*(sum_t (x_t - r_t)'Q(x_t - r_t) + rho*u_t'R u_t) + sum_t dot(c_t, u_t) + s, rho and s scalar Parameters; the Variables of
    test_gpu_quad_stages.horizon_model"""
    model = P.Model(optimizer or P.MockOptimizer(), **kw)
    sizes = [NX, NU] * stages
    if interleaved:
        vecs = [[] for _ in sizes]
        for k in range(max(sizes)):
            for vec, n in zip(vecs, sizes):
                if k < n:
                    vec.append(P.Variable(model))
    else:
        vecs = [[P.Variable(model) for _ in range(n)] for n in sizes]
    Q, R = P.Parameter(lambda: st["Q"], model), P.Parameter(lambda: st["R"], model)
    rho, s = P.Parameter(lambda: st["rho"], model), P.Parameter(lambda: st["s"], model)
    quad = lin = None
    for t in range(stages):
        x, u = vecs[2 * t], vecs[2 * t + 1]
        r = P.Parameter(lambda t=t: st["r%d" % t], model)
        c = P.Parameter(lambda t=t: st["c%d" % t], model)
        cost = P.transpose(x - r) * Q * (x - r) + rho * (P.transpose(u) * R * u)
        quad = cost if quad is None else quad + cost
        lin = P.dot(c, u) if lin is None else lin + P.dot(c, u)
    P.objective(model, P.Minimize, 0.5 * quad + lin + s)
    return model, vecs


def described(st, xvars):
    """the weighted model's stages in expression order, as quad_stages_terms_util takes them, and its constants"""
    out = []
    for k, xv in enumerate(xvars):
        if k % 2 == 0:
            out.append({"Q": st["Q"], "xvar": xv, "v": st["r%d" % (k // 2)], "sign": -1, "W": (0.5, None), "lin": None})
        else:
            out.append({"Q": st["R"], "xvar": xv, "v": None, "sign": 0, "W": (0.5, st["rho"]), "lin": (1.0, None, st["c%d" % (k // 2)])})
    return out, [(1.0, None, st["s"])]


@pytest.mark.parametrize("layout", ["in-order", "interleaved"])
def test_weighted_horizon_model(layout):
    """mode "canonical-stages"; bit for bit the restatement, solve after solve with new values of rho, s, c_t, r_t, Q and R; within the derived
    bounds of the oracle's literal sequence; the same model with quadratic_mode="literal" is the literal record it was"""
    st = new_values(40)
    kw = dict(interleaved=(layout == "interleaved"), use_graph=True)
    model, vecs = weighted_model(st, quadratic_mode="canonical", **kw)
    lit, _ = weighted_model(st, quadratic_mode="literal", **kw)
    xvars = G.indices(vecs)
    try:
        nbytes = []
        for it in range(3):
            if it:
                st.update(new_values(40 + 100 * it))
            gq, gl, gc = G.solved(model)
            assert model.objective.mode == "canonical-stages" and not model._small
            assert model.objective.plan.stage_terms is not None and len(model.objective.plan.stage_consts) == 1
            assert model.objective.groups_ordered == (layout == "in-order")
            varmap = np.asarray(model.model_var_to_optimizer, dtype=np.int64)
            stages, consts = described(st, xvars)
            quad, lin, const = W.merged(stages, consts, varmap)
            assert np.array_equal(gq.view(np.int64), quad.view(np.int64)), "quadratic terms differ from the restatement"
            assert np.array_equal(gl.view(np.int64), lin.view(np.int64)), "linear terms differ from the restatement"
            assert bits([gc])[0] == bits([const])[0], "the constant differs from the restatement"
            nbytes.append(model.device().bytes_allocated())
            if it == 2:
                continue
            # the oracle's sequence: the same pairs; coefficients within quad_bound (0.5: bit for bit), lin_bound, const_bound
            at, qt, oconst = W.oracle(stages, consts, varmap)
            want_q = dict(zip(zip(qt["row"].tolist(), qt["col"].tolist()), qt["coeff"].tolist()))
            want_l = U.lin_by_var(at)
            assert len(qt) == len(gq)
            for sd in stages:
                q, l, _ = W.restate_stage(sd, varmap)
                got = np.array([want_q[(r, c)] for r, c in zip(q["row"].tolist(), q["col"].tolist())])
                qb = W.quad_bound(sd)
                assert np.all(np.abs(q["coeff"] - got) <= qb)
                if sd["W"] == (0.5, None):
                    assert np.array_equal(bits(q["coeff"]), bits(got))
                lb = W.lin_bound(sd, U.restate_stage(sd, varmap)[1]["coeff"])
                assert np.all(np.abs(l["coeff"] - np.array([want_l.get(v, 0.0) for v in l["var"].tolist()])) <= lb)
            assert abs(gc - oconst) <= W.const_bound(stages, consts, varmap)
            # the literal model is unchanged: the literal record, with the literal function's size
            lq, ll, lc = G.solved(lit)
            assert lit.objective.mode == "literal" and len(lq) == T_H * (NX * NX + NU * NU)
            pairs, byvar = G.literal_function(lq, ll)
            assert len(pairs) == len(gq)
            for sd in stages:
                q, l, _ = W.restate_stage(sd, varmap)
                got = np.array([pairs[(min(r, c), max(r, c))] for r, c in zip(q["row"].tolist(), q["col"].tolist())])
                assert np.all(np.abs(q["coeff"] - got) <= W.quad_bound(sd))
        assert len(set(nbytes)) == 1, "plan memory grew across solves: %r" % (nbytes,)
    finally:
        model.close()
        lit.close()


def test_an_eight_form_prefix_is_canonical_groups_with_the_same_words(monkeypatch):
    """the first four stages (eight forms) of the weighted horizon write, through the single-instance nodes of "canonical-groups", the
    quadratic and linear words the horizon's launch writes for them (the size threshold of that row is lowered for the small model)"""
    from parametron_jl_amd import moi
    st = new_values(7)
    model, vecs = weighted_model(st, quadratic_mode="canonical", use_graph=True)
    monkeypatch.setattr(moi, "GROUPS_MIN_LITERAL_TERMS", 1 << 12)
    prefix, pvars = weighted_model(st, stages=4, quadratic_mode="canonical", use_graph=True)
    try:
        gq, gl, gc = G.solved(model)
        pq, pl, pc = G.solved(prefix)
        assert model.objective.mode == "canonical-stages" and prefix.objective.mode == "canonical-groups" and prefix.objective.groups_ordered
        assert all(np.array_equal(a, b) for a, b in zip(G.indices(pvars), G.indices(vecs)[:8]))
        assert len(pq) == 4 * (NX * (NX + 1) // 2 + NU * (NU + 1) // 2) and len(pl) == 4 * (NX + NU)
        assert np.array_equal(pq.view(np.int64), gq[:len(pq)].view(np.int64))
        assert np.array_equal(pl.view(np.int64), gl[:len(pl)].view(np.int64))
    finally:
        model.close()
        prefix.close()


def test_a_solved_weighted_horizon_equals_its_dense_statement():
    """minimize 0.5*(sum_t (x_t - r_t)'Q(x_t - r_t) + rho*u_t'R u_t) + sum_t c_t'u_t + s subject to A z == b (five rows) through the KKT
    solve of tests/qp_solver.py, against the same problem stated densely as z'Hz - g'z + s2 ("canonical-sum") with
    H = 0.5*blockdiag(Q, rho*R, ..), g = (0.5*(Q + Q')r_t, -c_t, ..), and against numpy's solve of the KKT system.
    Bound 1e-9, as test_a_solved_horizon_equals_its_dense_statement derives it: the weights scale K and the right-hand side by factors
    between 0.5 and 1 (rho = 1.5: the u blocks by 0.75), which changes none of its terms by more than a factor of two; the quadratic
    coefficients of both statements differ by at most gamma_2-sized roundings of the weight (quad_stages_terms_util.quad_bound; 0.5 is
    exact), five orders inside 1e-9 after |K^-1|_inf (asserted below 1e2); the linear parts by (gamma_65 + gamma_41)*|S||r| + 3u|c|,
    asserted below 1e-12.  cond(K) < 1e4 is asserted."""
    from qp_solver import DenseQPOptimizer
    rng = np.random.default_rng(3)

    def weight(n):
        M = 0.1 * (rng.random((n, n)) - 0.5)
        M[np.diag_indices(n)] = 4.0 + rng.random(n)
        return M
    st = {"Q": weight(NX), "R": weight(NU), "rho": 1.5, "s": 0.25}
    for t in range(T_H):
        st["r%d" % t], st["c%d" % t] = rng.standard_normal(NX), rng.standard_normal(NU)
    nz = T_H * (NX + NU)
    A, b = rng.standard_normal((5, nz)), rng.standard_normal(5)
    H, g, s2 = np.zeros((nz, nz)), np.zeros(nz), st["s"]
    for t in range(T_H):
        o = t * (NX + NU)
        H[o:o + NX, o:o + NX], H[o + NX:o + NX + NU, o + NX:o + NX + NU] = 0.5 * st["Q"], 0.5 * st["rho"] * st["R"]
        g[o:o + NX], g[o + NX:o + NX + NU] = 0.5 * (st["Q"] + st["Q"].T) @ st["r%d" % t], -st["c%d" % t]
        s2 += 0.5 * float(st["r%d" % t] @ st["Q"] @ st["r%d" % t])
    Sm = H + H.T
    assert np.all(2 * np.abs(np.diag(Sm)) > np.sum(np.abs(Sm), axis=1))
    sols = []
    for horizon in (True, False):
        if horizon:
            model, vecs = weighted_model(st, optimizer=DenseQPOptimizer(), quadratic_mode="canonical", use_graph=True)
            z = [v for vec in vecs for v in vec]
        else:
            model = P.Model(DenseQPOptimizer(), quadratic_mode="canonical", use_graph=True)
        try:
            if not horizon:
                z = [P.Variable(model) for _ in range(nz)]
                Hp, gp, sp_ = (P.Parameter(lambda v=v: v, model) for v in (H, g, s2))
                P.objective(model, P.Minimize, P.transpose(z) * Hp * z - P.dot(gp, z) + sp_)
            Ap, bp = P.Parameter(lambda: A, model), P.Parameter(lambda: b, model)
            P.constraint(model, Ap * z == bp)
            P.solve(model)
            assert model.objective.mode == ("canonical-stages" if horizon else "canonical-sum")
            sols.append(np.array([P.value(model, v) for v in z]))
        finally:
            model.close()
    K = np.block([[Sm, A.T], [A, np.zeros((5, 5))]])
    absr = np.max([np.max(np.abs(st["Q"] + st["Q"].T) @ np.abs(st["r%d" % t])) for t in range(T_H)])
    absc = np.max([np.max(np.abs(st["c%d" % t])) for t in range(T_H)])
    d = (S.gamma(65) + S.gamma(NX + 1)) * absr + 3 * S.U * absc
    kinv = np.linalg.norm(np.linalg.inv(K), np.inf)
    assert np.linalg.cond(K) < 1e4 and d < 1e-12 and kinv < 1e2 and kinv * d < 1e-10
    assert np.max(np.abs(sols[0] - sols[1])) <= 1e-9
    np.testing.assert_allclose(A @ sols[0], b, atol=1e-9)
    zk = np.linalg.solve(K, np.concatenate([g, b]))
    assert np.max(np.abs(sols[0] - zk[:nz])) <= 1e-9
