"""-m gpu: horizon stage costs as one canonical node (pmt_quad_stages_f64) and the record mode "canonical-stages".

C ABI: the WHOLE images of the outputs — the stages' slices with poisoned words in front of, between and behind them — compared bit for
bit with the numpy restatement of the header's order (tests/quad_stages_util.py), and every stage's slice with what pmt_quad_form_f64 /
pmt_quad_form_shift_f64 writes for that stage alone.  Host API: a 12-stage horizon over x_t (n = 40, shifted by r_t) and u_t (n = 8) with
shared Q and R, bit for bit the restatement solve after solve, within the derived bounds of the literal model, in both layouts."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import parametron_jl_amd as P  # noqa: E402
from parametron_jl_amd import _lib  # noqa: E402
import quad_form_shift_util as S  # noqa: E402
import quad_stages_util as U  # noqa: E402
from gpu_util import DEV, POISON_WORD, Guarded, ptr, stream  # noqa: E402

QT, LT = _lib.QT, _lib.LT


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------ 1. the entry point
def place(stages, gaps):
    """the stages' slices one behind the other with gaps[t] terms in front of stage t (and the last gap behind the last stage)
    -> (nterms, nlin); an odd gap in front of a stage puts its quadratic slice at an address 8 mod 16"""
    qa = la = 0
    for st, g in zip(stages, gaps):
        st["quad_at"], st["lin_at"] = qa + g, la + g
        n = len(st["xvar"])
        qa, la = st["quad_at"] + n * (n + 1) // 2, st["lin_at"] + n
    return qa + gaps[-1], la + gaps[-1]


class Launch:
    """device inputs (every distinct Q uploaded once, pitch ldq = n + pad with NaN in the padding rows), the descriptor table through
    pmt_quad_stages_check, guarded outputs"""

    def __init__(self, stages, varmap, nterms, nlin, pad=3, shift=0):
        self.stages, self.varmap, self.nterms, self.nlin, self.T = stages, varmap, nterms, nlin, len(stages)
        self.keep, mats, rows = [], {}, []
        for st in stages:
            n = len(st["xvar"])
            if id(st["Q"]) not in mats:
                buf = np.full((n, n + pad), np.nan)
                buf[:, :n] = np.asarray(st["Q"]).T
                mats[id(st["Q"])] = torch.from_numpy(buf.reshape(-1)).to(DEV)
            dQ = mats[id(st["Q"])]
            dx = torch.from_numpy(np.ascontiguousarray(st["xvar"], dtype=np.int64)).to(DEV)
            dv = torch.from_numpy(np.ascontiguousarray(st["v"], dtype=np.float64)).to(DEV) if st["sign"] else None
            self.keep += [dQ, dx, dv]
            rows.append({"Q": dQ.data_ptr(), "ldq": n + pad, "xvar": dx.data_ptr(), "vec": dv.data_ptr() if dv is not None else None, "n": n,
                         "sign": st["sign"], "quad_at": st["quad_at"], "lin_at": st["lin_at"]})
        self.rows = rows
        self.arr = _lib.quad_stages(rows)
        _lib.call("pmt_quad_stages_check", C.addressof(self.arr), self.T, nterms, nlin)
        self.table = torch.from_numpy(np.frombuffer(self.arr, dtype=np.uint8).copy()).to(DEV)
        self.dvm = torch.from_numpy(np.ascontiguousarray(varmap, dtype=np.int64)).to(DEV)
        self.quad, self.lin = Guarded(3 * nterms, shift=shift), Guarded(2 * nlin, shift=shift)
        self.consts, self.const = Guarded(self.T, doubles=True), Guarded(1, doubles=True)

    def run(self, s=None):
        _lib.call("pmt_quad_stages_f64", ptr(self.table), self.T, ptr(self.dvm), self.quad.ptr(), self.lin.ptr(), self.consts.ptr(), self.const.ptr(),
                  stream() if s is None else C.c_void_p(s.cuda_stream))
        return self

    def check(self, skip=()):
        """whole images against the restatement; `skip`: stages whose linear coefficients and constant are not compared (a NaN's payload)"""
        quad, lin, consts, const = U.images(self.stages, self.varmap, self.nterms, self.nlin, POISON_WORD)
        self.quad.check(quad, "quadratic terms")
        if not skip:
            self.lin.check(lin, "linear terms")
            self.consts.check(consts, "stage constants")
            self.const.check(np.array([const]), "constant")
        return quad, lin, consts, const

    def host(self):
        torch.cuda.synchronize()
        g = lambda G: G.buf.cpu().numpy().view(np.int64)[G.off:G.off + G.n].copy()
        return g(self.quad), g(self.lin), g(self.consts).view(np.float64), g(self.const).view(np.float64)[0]

    def check_alone(self, which=None):
        """every stage's slice against the single node called alone with the same Q, xvar, varmap, moi = 1, alpha = 1.0"""
        quad, lin, consts, _ = self.host()
        for t in (range(self.T) if which is None else which):
            r, n = self.rows[t], self.rows[t]["n"]
            nq = n * (n + 1) // 2
            oq, ol, oc = Guarded(3 * nq, shift=t & 1), Guarded(2 * n), Guarded(1, doubles=True)
            if r["sign"]:
                ws = torch.full((int(_lib.load().pmt_quad_form_shift_workspace_bytes(n)) // 8 + 2,), np.nan, dtype=torch.float64, device=DEV)
                _lib.call("pmt_quad_form_shift_f64", C.c_void_p(r["Q"]), r["ldq"], n, C.c_void_p(r["xvar"]), C.c_void_p(r["vec"]), r["sign"], 1,
                          ptr(self.dvm), 1.0, oq.ptr(), None, ol.ptr(), oc.ptr(), ptr(ws), stream())
            else:
                _lib.call("pmt_quad_form_f64", C.c_void_p(r["Q"]), r["ldq"], n, C.c_void_p(r["xvar"]), 1, ptr(self.dvm), 1.0, oq.ptr(), None,
                          ol.ptr(), oc.ptr(), stream())
            oq.check(quad[3 * r["quad_at"]:3 * (r["quad_at"] + nq)], "stage %d: quadratic terms of the node alone" % t)
            ol.check(lin[2 * r["lin_at"]:2 * (r["lin_at"] + n)], "stage %d: linear terms of the node alone" % t)
            oc.check(consts[t:t + 1], "stage %d: constant of the node alone" % t)


@functools.lru_cache(maxsize=None)
def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 192, 255, 256])
def test_every_tile_edge_bit_for_bit(n):
    """three stages of one size — shifted by -v, plain, shifted by +v — over two shared matrices, zeros of both signs in Q and v; gaps of
    1, 2, 1 and 3 terms around the slices (the first and third quadratic slices start 8 mod 16)"""
    stages, varmap, _, _ = U.make_stages([n, n, n], [-1, 0, 1], 100 + n, special=True)
    nterms, nlin = place(stages, [1, 2, 1, 3])
    L = Launch(stages, varmap, nterms, nlin).run()
    L.check()
    L.check_alone()
    L.run().check()                                               # a second call over the first one's outputs


def test_mixed_sizes_in_one_launch_with_odd_offsets():
    ns = [3, 65, 1, 130, 2, 64, 7, 256, 5, 129, 63]
    signs = [-1, 0, 1, -1, 0, 1, 1, -1, 0, 1, -1]
    for shift in (0, 1):
        stages, varmap, _, _ = U.make_stages(ns, signs, 31 + shift, shared=1, interleave=bool(shift))
        nterms, nlin = place(stages, [1, 0, 1, 1, 2, 1, 0, 3, 1, 1, 0, 2])
        assert any(st["quad_at"] & 1 for st in stages) and any(not st["quad_at"] & 1 for st in stages)
        L = Launch(stages, varmap, nterms, nlin, pad=0 if shift else 5, shift=shift).run()
        L.check()
        L.check_alone()


@pytest.mark.parametrize("T", [1, 2, 9, "3CUs+5"])
def test_stage_counts(T):
    """one stage; fewer stages than workgroups; 3 CUs + 5 stages of n = 3, where the persistent loop wraps and the constant's chains hold
    more than one stage"""
    wrap = T == "3CUs+5"
    T = 3 * cu_count() + 5 if wrap else T
    n = 3 if wrap else 70
    stages, varmap, _, _ = U.make_stages([n] * T, [(-1, 0, 1)[t % 3] for t in range(T)], 500 + T, shared=3)
    nterms, nlin = place(stages, [t % 2 for t in range(T)] + [1])
    L = Launch(stages, varmap, nterms, nlin).run()
    _, _, consts, const = L.check()
    L.check_alone(range(0, T, max(1, T // 8)))
    if wrap:
        assert T > 256 and const == S.chain_tree_sum(consts) and np.count_nonzero(consts) > T // 2


def test_results_do_not_depend_on_the_stage_count_or_position():
    """a stage's words are the same alone (T = 1), first of nine and last of nine; a permuted table writes the same slices"""
    stages, varmap, nterms, nlin = U.make_stages([70, 5, 130, 64, 3, 65, 2, 9, 70], [-1, 0, 1, 0, -1, 1, 0, -1, 1], 77, shared=2)
    full = Launch(stages, varmap, nterms, nlin).run()
    quad, lin, consts, _ = full.check()
    perm = [4, 8, 0, 2, 7, 1, 6, 3, 5]
    again = Launch([stages[k] for k in perm], varmap, nterms, nlin).run()
    q2, l2, c2, _ = again.check()
    assert np.array_equal(q2, quad) and np.array_equal(l2, lin) and np.array_equal(bits(c2), bits(consts[perm]))
    for t in (0, 8):
        one = dict(stages[t], quad_at=0, lin_at=0)
        n = len(one["xvar"])
        q1, l1, c1, k1 = Launch([one], varmap, n * (n + 1) // 2, n).run().host()
        assert np.array_equal(q1, quad[3 * stages[t]["quad_at"]:][:len(q1)]) and np.array_equal(l1, lin[2 * stages[t]["lin_at"]:][:len(l1)])
        assert bits(c1)[0] == bits(consts)[t]
        assert bits([k1])[0] == bits([S.chain_tree_sum(consts[t:t + 1])])[0]


def test_a_nan_in_one_vector_stays_in_its_stage():
    stages, varmap, nterms, nlin = U.make_stages([66, 8] * 5, [-1, 1] * 5, 91)
    bad = 4
    stages[bad]["v"] = stages[bad]["v"].copy()
    stages[bad]["v"][17] = np.nan
    L = Launch(stages, varmap, nterms, nlin).run()
    want_quad, want_lin, want_consts, _ = L.check(skip=(bad,))
    quad, lin, consts, const = L.host()
    gl, wl = lin.view(LT), want_lin.view(LT)
    mine = np.zeros(nlin, dtype=bool)
    mine[stages[bad]["lin_at"]:stages[bad]["lin_at"] + 66] = True
    assert np.array_equal(gl["var"], wl["var"])
    assert np.array_equal(bits(gl["coeff"][~mine]), bits(wl["coeff"][~mine])) and np.all(np.isnan(gl["coeff"][mine]))
    others = np.arange(len(stages)) != bad
    assert np.array_equal(bits(consts[others]), bits(want_consts[others])) and np.isnan(consts[bad]) and np.isnan(const)
    assert not np.any(np.isnan(quad.view(QT)["coeff"]))


def test_no_stage_writes_the_constant_only():
    """T == 0: *out_const = +0.0 and nothing else, whatever the other pointers"""
    quad, lin, const = Guarded(6), Guarded(4), Guarded(1, doubles=True)
    _lib.call("pmt_quad_stages_f64", None, 0, None, quad.ptr(), lin.ptr(), None, const.ptr(), stream())
    quad.check(quad.padding(6), "quadratic terms")
    lin.check(lin.padding(4), "linear terms")
    const.check(np.array([0.0]), "constant")


# ------------------------------------------------------------------ 2. the host API
NX, NU, T_H = 40, 8, 12


def new_values(seed):
    st = {}
    st["Q"], _, _, _ = S.make_case(NX, seed)
    st["R"], _, _, _ = S.make_case(NU, seed + 1)
    for t in range(T_H):
        _, st["r%d" % t], _, _ = S.make_case(NX, seed + 2 + t)
    return st


def horizon_model(st, stages=T_H, interleaved=False, optimizer=None, **kw):
    """sum_t transpose(x_t - r_t)*Q*(x_t - r_t) + transpose(u_t)*R*u_t; Variables stage by stage, or dealt out element by element"""
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
    expr = None
    for t in range(stages):
        x, u = vecs[2 * t], vecs[2 * t + 1]
        r = P.Parameter(lambda t=t: st["r%d" % t], model)
        cost = P.transpose(x - r) * Q * (x - r) + P.transpose(u) * R * u
        expr = cost if expr is None else expr + cost
    P.objective(model, P.Minimize, expr)
    return model, vecs


def indices(vecs):
    return [np.array([v.index for v in vec], dtype=np.int64) for vec in vecs]


def described(st, xvars):
    """the model's stages in expression order, as quad_stages_util takes them"""
    out = []
    for k, xv in enumerate(xvars):
        out.append({"Q": st["Q"], "xvar": xv, "v": st["r%d" % (k // 2)], "sign": -1} if k % 2 == 0 else {"Q": st["R"], "xvar": xv, "v": None, "sign": 0})
    return out


def solved(model):
    P.solve(model)
    f = model.objective.f
    return f.quadratic_terms.copy(), f.affine_terms.copy(), float(f.constant)


def literal_function(gq, gl):
    """the literal model's MOI function with the terms of every pair / variable added up: {(row, col): coeff}, {var: coeff}"""
    quad, lin = {}, {}
    for c, r, k in zip(gq["coeff"].tolist(), gq["row"].tolist(), gq["col"].tolist()):
        key = (min(r, k), max(r, k))
        quad[key] = quad[key] + c if key in quad else c
    for c, v in zip(gl["coeff"].tolist(), gl["var"].tolist()):
        lin[v] = lin[v] + c if v in lin else c
    return quad, lin


@pytest.mark.parametrize("layout", ["in-order", "interleaved"])
def test_horizon_model(layout):
    """mode "canonical-stages"; bit for bit the restatement, solve after solve with new Parameter values; within the derived bounds of the
    same model built with quadratic_mode="literal"; Variables dealt out element by element take the gather"""
    st = new_values(40)
    kw = dict(interleaved=(layout == "interleaved"), use_graph=True)
    model, vecs = horizon_model(st, quadratic_mode="canonical", **kw)
    lit, _ = horizon_model(st, quadratic_mode="literal", **kw)
    xvars = indices(vecs)
    try:
        nbytes = []
        for it in range(3):
            if it:
                st.update(new_values(40 + 100 * it))
            gq, gl, gc = solved(model)
            assert model.objective.mode == "canonical-stages" and not model._small
            assert model.objective.groups_ordered == (layout == "in-order")
            varmap = np.asarray(model.model_var_to_optimizer, dtype=np.int64)
            stages = described(st, xvars)
            quad, lin, const = U.merged(stages, varmap)
            assert np.array_equal(gq.view(np.int64), quad.view(np.int64)), "quadratic terms differ from the restatement"
            assert np.array_equal(gl.view(np.int64), lin.view(np.int64)), "linear terms differ from the restatement"
            assert bits([gc])[0] == bits([const])[0], "the constant differs from the restatement"
            nbytes.append(model.device().bytes_allocated())
            if it == 2:
                continue
            # the literal model: the same pairs with the same sums of two numbers; lin and the constant within the bounds
            lq, ll, lc = solved(lit)
            assert lit.objective.mode == "literal" and len(lq) == T_H * (NX * NX + NU * NU)
            pairs, byvar = literal_function(lq, ll)
            assert len(pairs) == len(gq)
            want = np.array([pairs[(min(r, k), max(r, k))] for r, k in zip(gq["row"].tolist(), gq["col"].tolist())])
            # (the MOI copy doubles a diagonal term; off the diagonal the two literal terms are added here, in either order)
            assert np.array_equal(bits(gq["coeff"]), bits(want))
            parts, _ = U.restate(stages, varmap)
            for sd, (_, l, _) in zip(stages, parts):
                b = U.lin_bound(sd)
                got = np.array([byvar.get(v, 0.0) for v in l["var"].tolist()])
                assert np.all(np.abs(l["coeff"] - got) <= b)
            assert abs(gc - lc) <= U.const_bound(stages, [p[2] for p in parts])
        assert len(set(nbytes)) == 1, "plan memory grew across solves: %r" % (nbytes,)
    finally:
        model.close()
        lit.close()


def test_an_eight_form_prefix_is_canonical_groups_with_the_same_words(monkeypatch):
    """the first four stages (eight forms: as many as "canonical-groups" holds) write, through the single-instance nodes, the words the
    horizon's launch writes for them.  Their literal function (6656 terms) lies below that row's size threshold — a performance choice, not
    one of correctness — so the threshold is lowered for this model."""
    from parametron_jl_amd import moi
    st = new_values(7)
    model, vecs = horizon_model(st, quadratic_mode="canonical", use_graph=True)
    monkeypatch.setattr(moi, "GROUPS_MIN_LITERAL_TERMS", 1 << 12)
    prefix, pvars = horizon_model(st, stages=4, quadratic_mode="canonical", use_graph=True)
    try:
        gq, gl, gc = solved(model)
        pq, pl, pc = solved(prefix)
        assert model.objective.mode == "canonical-stages" and prefix.objective.mode == "canonical-groups" and prefix.objective.groups_ordered
        assert all(np.array_equal(a, b) for a, b in zip(indices(pvars), indices(vecs)[:8]))
        assert len(pq) == 4 * (NX * (NX + 1) // 2 + NU * (NU + 1) // 2) and len(pl) == 4 * (NX + NU)
        assert np.array_equal(pq.view(np.int64), gq[:len(pq)].view(np.int64))
        assert np.array_equal(pl.view(np.int64), gl[:len(pl)].view(np.int64))
    finally:
        model.close()
        prefix.close()


def test_a_solved_horizon_equals_its_dense_statement():
    """minimize sum_t (x_t - r_t)'Q(x_t - r_t) + u_t'R u_t subject to A z == b over all 576 variables z (five rows), through the KKT solve of
    tests/qp_solver.py; the same problem stated densely as z'Hz - g'z + s with H = blockdiag(Q, R, Q, R, ..), g = ((Q + Q')r_t, 0, ..) and
    s = sum_t r_t'Q r_t computed on the host ("canonical-sum").  Q and R are unsymmetric with diagonals in [4, 5) and off-diagonal entries of
    at most 0.05 in magnitude: Q + Q' is strictly diagonally dominant, the problem strictly convex.
    Bound 1e-9.  Both objectives hold the same quadratic coefficients bit for bit (sums of two numbers; the dense form's terms between two
    blocks are 0.0 + 0.0).  The linear coefficients are two roundings of -(Q + Q')r_t: the node's, within gamma_65 * |S||r| of it
    (quad_form_shift_util), and numpy's 40-term dot products negated by the combine, within gamma_41 * |S||r|.  So the two KKT systems share K
    and differ in the right-hand side by at most d = (gamma_65 + gamma_41) * max_j (|S||r_t|)_j (asserted below 1e-12), the exact solutions by
    at most |K^-1|_inf * d (asserted below 1e-10), and each solve's own rounding adds about cond(K) * 2^-52 * |z| (cond(K) < 1e4 asserted,
    |z| of order 1: below 1e-11).  All of it is an order inside 1e-9."""
    from qp_solver import DenseQPOptimizer
    rng = np.random.default_rng(3)

    def weight(n):
        W = 0.1 * (rng.random((n, n)) - 0.5)
        W[np.diag_indices(n)] = 4.0 + rng.random(n)
        return W
    st = {"Q": weight(NX), "R": weight(NU)}
    for t in range(T_H):
        st["r%d" % t] = rng.standard_normal(NX)
    nz = T_H * (NX + NU)
    A, b = rng.standard_normal((5, nz)), rng.standard_normal(5)
    H, g, s = np.zeros((nz, nz)), np.zeros(nz), 0.0
    for t in range(T_H):
        o = t * (NX + NU)
        H[o:o + NX, o:o + NX], H[o + NX:o + NX + NU, o + NX:o + NX + NU] = st["Q"], st["R"]
        g[o:o + NX] = (st["Q"] + st["Q"].T) @ st["r%d" % t]
        s += float(st["r%d" % t] @ st["Q"] @ st["r%d" % t])
    Sm = H + H.T
    assert np.all(2 * np.abs(np.diag(Sm)) > np.sum(np.abs(Sm), axis=1))
    sols = []
    for horizon in (True, False):
        if horizon:
            model, vecs = horizon_model(st, optimizer=DenseQPOptimizer(), quadratic_mode="canonical", use_graph=True)
            z = [v for vec in vecs for v in vec]
        else:
            model = P.Model(DenseQPOptimizer(), quadratic_mode="canonical", use_graph=True)
        try:
            if not horizon:
                z = [P.Variable(model) for _ in range(nz)]
                Hp, gp, sp_ = (P.Parameter(lambda v=v: v, model) for v in (H, g, s))
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
    d = (S.gamma(65) + S.gamma(NX + 1)) * absr
    assert np.linalg.cond(K) < 1e4 and d < 1e-12 and np.linalg.norm(np.linalg.inv(K), np.inf) * d < 1e-10
    assert np.max(np.abs(sols[0] - sols[1])) <= 1e-9
    np.testing.assert_allclose(A @ sols[0], b, atol=1e-9)
    zk = np.linalg.solve(K, np.concatenate([g, b]))
    assert np.max(np.abs(sols[0] - zk[:nz])) <= 1e-9

