"""-m gpu: horizon dynamics constraints as one launch (pmt_affine_stages_f64) and the record group moi.affine_stage_group.

C ABI: the WHOLE images of the two outputs, with poisoned guard words in front of and behind them, compared bit for bit with the numpy
restatement of the header's contract (tests/affine_stages_util.py), and every stage's words with what today's chain —
pmt_affine_assemble_f64 per product, pmt_affvec_combine_f64 per + / -, pmt_pack_vector_affine_f64 — writes on the same data.  Host API: a
12-stage horizon whose dynamics are written in four spellings between ineligible neighbours, bit for bit the same model built with the
group switched off, solve after solve; a solved QP with and without the group.  Every size used is valid; nothing here provokes a fault."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import parametron_jl_amd as P  # noqa: E402
from parametron_jl_amd import _lib  # noqa: E402
import affine_stages_util as U  # noqa: E402
from gpu_util import DEV, POISON_WORD, Guarded, empty_f64, empty_terms, ptr, stream, terms_to_host, f64_to_host  # noqa: E402

LT, VAT = _lib.LT, _lib.VAT
NAMES = list(U.SPELLINGS)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------ 1. the entry point
class Launch:
    """device inputs (every distinct matrix uploaded once, column-major with pitch ld = rows + pad and NaN in the padding rows), the two
    tables through pmt_affine_stages_check, guarded outputs"""

    def __init__(self, stages, varmap, pad=3, shift=0):
        self.stages, self.varmap, self.T = stages, varmap, len(stages)
        self.nterms, self.nconsts = U.place(stages)
        self.keep, mats, parts, rows = [], {}, [], []
        for st in stages:
            first = len(parts)
            for p in st["parts"]:
                dx = dev(np.asarray(p["xvar"], dtype=np.int64))
                self.keep.append(dx)
                if p["mat"] is None:
                    parts.append({"mat": None, "ld": 0, "xvar": dx.data_ptr(), "cols": 1, "sign": p["sign"]})
                    continue
                r, c = p["mat"].shape
                if id(p["mat"]) not in mats:
                    buf = np.full((c, r + pad), np.nan)
                    buf[:, :r] = np.asarray(p["mat"]).T
                    mats[id(p["mat"])] = dev(buf.reshape(-1))
                parts.append({"mat": mats[id(p["mat"])].data_ptr(), "ld": r + pad, "xvar": dx.data_ptr(), "cols": c, "sign": p["sign"]})
            dv = dev(np.asarray(st["vec"], dtype=np.float64)) if st["vec"] is not None else None
            self.keep.append(dv)
            rows.append({"vec": dv.data_ptr() if dv is not None else None, "term_offset": st["term_offset"], "const_offset": st["const_offset"],
                         "row_len": U.row_len(st), "rows": st["rows"], "first_part": first, "nparts": len(st["parts"]), "vec_sign": st["vec_sign"]})
        self.keep += list(mats.values())
        self.parts, self.rows = parts, rows
        self.parr, self.sarr = _lib.affine_parts(parts), _lib.affine_stages(rows)
        _lib.call("pmt_affine_stages_check", C.addressof(self.sarr), self.T, C.addressof(self.parr), len(parts), self.nterms, self.nconsts)
        self.stable = dev(np.frombuffer(self.sarr, dtype=np.uint8).copy())
        self.ptable = dev(np.frombuffer(self.parr, dtype=np.uint8).copy())
        self.dvm = dev(np.asarray(varmap, dtype=np.int64)) if varmap is not None else None
        self.terms, self.consts = Guarded(3 * self.nterms, shift=shift), Guarded(self.nconsts, doubles=True)

    def run(self):
        _lib.call("pmt_affine_stages_f64", ptr(self.stable), self.T, ptr(self.ptable), ptr(self.dvm), self.terms.ptr(), self.consts.ptr(), stream())
        return self

    def check(self, what=""):
        terms, consts = U.images(self.stages, self.varmap, self.nterms, self.nconsts, POISON_WORD)
        assert not np.any(terms == POISON_WORD) and not np.any(np.isnan(consts))          # the stages tile the outputs
        self.terms.check(terms, what + " terms")
        self.consts.check(consts, what + " constants")
        return terms, consts

    def host(self):
        torch.cuda.synchronize()
        g = lambda G: G.buf.cpu().numpy().view(np.int64)[G.off:G.off + G.n].copy()
        return g(self.terms), g(self.consts)


def make_stage(rng, rows, cols, with_var=True, vec_sign=-1, signs=None, start=1, shared=None):
    """[x+] (+|-) M_1*v_1 (+|-) M_2*v_2 .. over consecutive model variables from `start`; `cols`: the matrices' column counts;
    `shared`: {cols: matrix} to take the matrices from"""
    parts, v = [], start
    signs = list(signs) if signs is not None else [1] + [-1] * len(cols)
    if with_var:
        parts.append({"mat": None, "xvar": np.arange(v, v + rows, dtype=np.int64), "sign": signs[0]})
        v += rows
    for k, c in enumerate(cols):
        mat = shared[(rows, c)] if shared is not None and (rows, c) in shared else U.special(rng, (rows, c))
        if shared is not None:
            shared[(rows, c)] = mat
        parts.append({"mat": mat, "xvar": np.arange(v, v + c, dtype=np.int64), "sign": signs[1 + k]})
        v += c
    vec = U.special(rng, rows) if vec_sign else None
    return {"rows": rows, "parts": parts, "vec": vec, "vec_sign": vec_sign, "term_offset": 0, "const_offset": 0}, v


def permutation(rng, n):
    return (rng.permutation(n) + 1 + 1000).astype(np.int64)


@pytest.mark.parametrize("cols", [1, 64, 65, 129])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 130])
def test_every_tile_edge_bit_for_bit(rows, cols):
    """one stage, with and without a Variable-vector part and a number vector; the output base on a 16-byte boundary and 8 behind one"""
    rng = np.random.default_rng(1000 * rows + cols)
    for with_var, vec_sign in itertools.product((True, False), (-1, 0)):
        st, n = make_stage(rng, rows, [cols], with_var, vec_sign)
        L = Launch([st], permutation(rng, n), shift=int(with_var)).run()
        L.check("rows %d cols %d var %s vec %d" % (rows, cols, with_var, vec_sign))
        if with_var and vec_sign:
            L.run().check("a second call over the first one's outputs")


def test_mixed_sizes_in_one_launch_with_odd_offsets():
    rng = np.random.default_rng(5)
    shapes = [(3, [3, 2]), (65, [65, 7]), (1, [1]), (130, [129, 64, 3]), (7, [64]), (64, [64, 64]), (5, [2, 2, 2, 2, 2, 2, 2]), (63, [130]), (9, [1, 1])]
    stages, v = [], 1
    for k, (rows, cols) in enumerate(shapes):
        st, v = make_stage(rng, rows, cols, with_var=(k % 3 != 2), vec_sign=(-1, 0, 1)[k % 3], start=v)
        stages.append(st)
    for shift in (0, 1):
        L = Launch(stages, permutation(rng, v), pad=0 if shift else 5, shift=shift).run()
        odd = [st["term_offset"] & 1 for st in stages]
        assert any(odd) and not all(odd)                          # slices at 8 mod 16 and at 0 mod 16 in one launch
        L.check("mixed sizes, shift %d" % shift)


@pytest.mark.parametrize("T", [1, 9, 600, 2100])
def test_stage_counts(T):
    """small stages of 8 x (1 + 8 + 4): one; a few, whose items are shared among several workgroups; 600, more work items than workgroups
    resident at once; 2100, more stages than the persistent grid has workgroups (eight per CU), so that its loop over the stages wraps"""
    rng = np.random.default_rng(T)
    shared, stages, v = {}, [], 1
    for t in range(T):
        st, v = make_stage(rng, 8, [8, 4], True, (-1, 0, 1)[t % 3], start=v, shared=shared)
        stages.append(st)
    assert len(shared) == 2                                       # A and B, read by every stage
    Launch(stages, permutation(rng, v)).run().check("T = %d" % T)


def test_a_stage_writes_the_same_words_alone_and_as_the_last_of_fifty():
    rng = np.random.default_rng(50)
    shared, stages, v = {}, [], 1
    for t in range(50):
        rows, cols = ((70, [70, 5]) if t == 49 else (8, [8, 4]))
        st, v = make_stage(rng, rows, cols, True, -1, start=v, shared=shared)
        stages.append(st)
    varmap = permutation(rng, v)
    full = Launch(stages, varmap).run()
    terms, consts = full.check("fifty stages")
    last = dict(stages[49])
    ta, ca = last["term_offset"], last["const_offset"]
    t1, c1 = Launch([last], varmap).run().host()
    assert np.array_equal(t1, terms[3 * ta:]) and np.array_equal(c1.view(np.int64), consts[ca:].view(np.int64))
    # without a varmap the indices are the model's own
    st0, n0 = make_stage(rng, 66, [5], True, 1)
    Launch([st0], None).run().check("identity")


def test_every_sign_combination():
    """three parts and the number vector in all 2^3 x 3 sign combinations, zeros of both signs in the matrices and in w"""
    rng = np.random.default_rng(8)
    stages, v = [], 1
    for signs in itertools.product((1, -1), repeat=3):
        for vs in (-1, 0, 1):
            st, v = make_stage(rng, 5, [5, 3], True, vs, signs=signs, start=v)
            if vs:
                st["vec"][:2] = (0.0, -0.0)
            st["parts"][1]["mat"][0, :2] = (0.0, -0.0)
            stages.append(st)
    terms, consts = Launch(stages, permutation(rng, v)).run().check("signs")
    coeff = terms.view(VAT)["coeff"]
    assert np.any(np.signbit(coeff[coeff == 0.0])) and np.any(~np.signbit(coeff[coeff == 0.0]))
    assert not np.any(np.signbit(consts[consts == 0.0])) and np.count_nonzero(consts == 0.0) >= 16 * 2


# ---- today's chain on the device: assemble per product, combine per + / -, pack
class Chain:
    """operands of today's path as (LinearTerm buffer or None, terms per row, constants or None); + and - run pmt_affvec_combine_f64"""

    def __init__(self, rows, terms, row_len, consts):
        self.rows, self.terms, self.row_len, self.consts = rows, terms, row_len, consts

    @classmethod
    def product(cls, mat, xvar):
        rows, cols = mat.shape
        dA, dx = dev(np.ascontiguousarray(mat.T).reshape(-1)), dev(np.asarray(xvar, dtype=np.int64))
        t, c = empty_terms(rows * cols, LT), empty_f64(rows)
        _lib.call("pmt_affine_assemble_f64", ptr(dA), rows, rows, cols, ptr(dx), None, 0, ptr(t), ptr(c), stream())
        return cls(rows, t, cols, c)

    @classmethod
    def variables(cls, xvar):
        lt = np.empty(len(xvar), dtype=LT)
        lt["coeff"], lt["var"] = 1.0, xvar
        return cls(len(xvar), dev(lt.view(np.int64)), 1, None)

    @classmethod
    def numbers(cls, w):
        return cls(len(w), None, 0, dev(np.asarray(w, dtype=np.float64)))

    def _combine(self, o, sb):
        L = self.row_len + o.row_len
        t, c = empty_terms(self.rows * L, LT), empty_f64(self.rows)
        _lib.call("pmt_affvec_combine_f64", self.rows, ptr(self.terms), None, self.row_len, ptr(self.consts), ptr(o.terms), None, o.row_len,
                  ptr(o.consts), sb, ptr(t), None, L, ptr(c), stream())
        return Chain(self.rows, t, L, c)

    def __add__(self, o):
        return self._combine(o, 1)

    def __sub__(self, o):
        return self._combine(o, -1)

    def packed(self, varmap):
        out = empty_terms(self.rows * self.row_len, VAT)
        _lib.call("pmt_pack_vector_affine_f64", ptr(self.terms), None, self.rows, self.row_len, ptr(dev(varmap)), 0, ptr(out), stream())
        return terms_to_host(out, self.rows * self.row_len, VAT), f64_to_host(self.consts, self.rows)


@pytest.mark.parametrize("name", NAMES)
def test_kernel_equals_todays_chain(name):
    """per stage: the words of the assembles, the combines and the pack run on the same data, for every spelling"""
    rng = np.random.default_rng(len(name))
    stages, chains, v = [], [], 1
    for rows, nu in ((6, 3), (70, 9), (1, 1)):
        A, B, w = U.special(rng, (rows, rows)), U.special(rng, (rows, nu)), U.special(rng, rows)
        w[0] = -0.0
        x, u, xp = np.arange(v, v + rows), np.arange(v + rows, v + rows + nu), np.arange(v + rows + nu, v + 2 * rows + nu)
        v += 2 * rows + nu
        stages.append(U.spelled_stage(name, A, B, xp, x, u, w))
        chains.append(U.spelled_expression(name, Chain.product(A, x), Chain.product(B, u), Chain.variables(xp), Chain.numbers(w)))
    varmap = permutation(rng, v)
    terms, consts = Launch(stages, varmap).run().check(name)
    for st, ch in zip(stages, chains):
        t, c = ch.packed(varmap)
        ta, ca = st["term_offset"], st["const_offset"]
        assert np.array_equal(t.view(np.int64), terms[3 * ta:3 * (ta + len(t))]), "terms differ from today's chain"
        assert np.array_equal(c.view(np.int64), consts[ca:ca + len(c)].view(np.int64)), "constants differ from today's chain"


# ------------------------------------------------------------------ 2. the host API
def new_values(rng, T, nx, nu):
    st = {"A": U.special(rng, (nx, nx)), "B": U.special(rng, (nx, nu)), "lo": rng.standard_normal(nx), "x0": rng.standard_normal(nx)}
    W = rng.random((nx, nx)) * 0.1
    st["Q"] = W + np.diag(4.0 + rng.random(nx))
    W = rng.random((nu, nu)) * 0.1
    st["R"] = W + np.diag(4.0 + rng.random(nu))
    for t in range(T + 1):
        st["r%d" % t] = rng.standard_normal(nx)
        st["w%d" % t] = U.special(rng, nx)
        st["w%d" % t][t % nx] = -0.0
    return st


def horizon_model(st, T, nx, nu, names, optimizer=None, neighbours=True, beyond_small=False, **kw):
    """sum_t (x_t - r_t)'Q(x_t - r_t) + u_t'R u_t subject to x_{t+1} == A*x_t + B*u_t (+ w_t) in the spellings `names` in turn, with
    bounds x_t - lo >= 0 and the start x_0 == x0 (implicit blocks: ineligible) between them"""
    model = P.Model(optimizer or P.MockOptimizer(variable_offset=7), **kw)
    if beyond_small:
        # a work buffer of the user's beside the horizon's own data (Model.SMALL_MODEL_ELEMENTS counts every Parameter of the model): without a
        # graph replay the model is then beyond the small plan, and its MOI buffers leave as recorded fetches
        P.Parameter(model, val=np.zeros(300000))
    xs, us = [], []
    for t in range(T + 1):
        xs.append([P.Variable(model) for _ in range(nx)])
        if t < T:
            us.append([P.Variable(model) for _ in range(nu)])
    par = lambda key: P.Parameter(lambda: st[key], model)
    Q, R, A, B, lo, x0 = (par(k) for k in ("Q", "R", "A", "B", "lo", "x0"))
    expr = None
    for t in range(T):
        r = par("r%d" % t)
        cost = P.transpose(xs[t] - r) * Q * (xs[t] - r) + P.transpose(us[t]) * R * us[t]
        expr = cost if expr is None else expr + cost
    P.objective(model, P.Minimize, expr)
    spelled = []
    for t in range(T):
        if neighbours and t % 4 == 1:
            P.constraint(model, xs[t], ">=", lo)
        if t == 2:
            P.constraint(model, xs[0], "==", x0)
        name = names[t % len(names)]
        model.add_zero_constraint(U.spelled_expression(name, A * xs[t], B * us[t], xs[t + 1], par("w%d" % t)))
        spelled.append((name, t))
    idx = lambda vec: np.array([v.index for v in vec], dtype=np.int64)
    described = lambda: [U.spelled_stage(name, st["A"], st["B"], idx(xs[t + 1]), idx(xs[t]), idx(us[t]), st["w%d" % t]) for name, t in spelled]
    return model, xs, us, described


def functions(model):
    return [(c.f.terms.copy(), c.f.constants.copy()) for c in model.constraints]


def test_horizon_model_equals_the_plan_without_the_group(monkeypatch):
    """T = 12, (nx, nu) = (10, 4), a graph replay: every constraint's terms and constants bit for bit those of the same model built with
    affine_stage_group returning no group, and the restatement's, under a non-identity index map, three solves with new values; plan memory
    does not grow; the tape holds one pmt_affine_stages_f64 and none of the grouped records' combines and packs"""
    from parametron_jl_amd import moi
    from parametron_jl_amd.device import DeviceContext
    T, nx, nu = 12, 10, 4
    rng = np.random.default_rng(21)
    st = new_values(rng, T, nx, nu)
    taped = []
    call = DeviceContext.call

    def spy(self, name, *args):
        if self.recording:
            taped.append(name)
        return call(self, name, *args)
    monkeypatch.setattr(DeviceContext, "call", spy)
    kw = dict(use_graph=True, quadratic_mode="canonical")
    model, xs, us, described = horizon_model(st, T, nx, nu, NAMES, **kw)
    plain, _, _, _ = horizon_model(st, T, nx, nu, NAMES, **kw)
    try:
        P.solve(model)
        grouped_tape, taped[:] = list(taped), []
        monkeypatch.setattr(moi, "affine_stage_group", lambda records, small, handoff: None)
        P.solve(plain)
        plain_tape = list(taped)
        assert model._stage_group is not None and len(model._stage_group.members) == T and plain._stage_group is None and not model._small
        assert grouped_tape.count("pmt_affine_stages_f64") == 1 and "pmt_affine_stages_f64" not in plain_tape
        # per record today: two assembles, the combines of its spelling (2, 3, 3, 3) and the pack
        combines = sum({NAMES[0]: 2}.get(NAMES[t % 4], 3) for t in range(T))
        for name, gone in (("pmt_affine_assemble_f64", 2 * T), ("pmt_affvec_combine_f64", combines), ("pmt_pack_vector_affine_f64", T)):
            assert plain_tape.count(name) - grouped_tape.count(name) == gone, name
        assert grouped_tape.count("pmt_pack_vector_affine_f64") == 0
        nbytes = []
        for it in range(3):
            if it:
                st.update(new_values(np.random.default_rng(21 + it), T, nx, nu))
                P.solve(model)
                P.solve(plain)
            varmap = np.asarray(model.model_var_to_optimizer, dtype=np.int64)
            assert varmap[0] == 8 and np.array_equal(varmap, plain.model_var_to_optimizer)
            got, want = functions(model), functions(plain)
            assert len(got) == len(want) == T + 4
            for k, ((gt, gc), (wt, wc)) in enumerate(zip(got, want)):
                assert np.array_equal(gt.view(np.int64), wt.view(np.int64)), "constraint %d: terms differ from the plan without the group" % k
                assert np.array_equal(gc.view(np.int64), wc.view(np.int64)), "constraint %d: constants differ from the plan without the group" % k
            for r, sd in zip(model._stage_group.members, described()):
                t, c = U.restate_stage(sd, varmap)
                assert np.array_equal(r.f.terms.view(np.int64), t.view(np.int64)) and np.array_equal(r.f.constants.view(np.int64), c.view(np.int64))
                assert model.optimizer.constraints[r.optimizerindex] is r.f
            nbytes.append(model.device().bytes_allocated())
        assert len(set(nbytes)) == 1, "plan memory grew across solves: %r" % (nbytes,)
        assert model.device().tape_length() < plain.device().tape_length()
    finally:
        model.close()
        plain.close()


def test_horizon_model_with_recorded_fetches(monkeypatch):
    """the overlapped MOI boundary (no graph): the group's two arenas leave as recorded fetches; the same words as without the group"""
    from parametron_jl_amd import moi
    T, nx, nu = 10, 70, 5
    st = new_values(np.random.default_rng(4), T, nx, nu)
    kw = dict(quadratic_mode="canonical", beyond_small=True)
    model, _, _, described = horizon_model(st, T, nx, nu, NAMES[:2], **kw)
    plain, _, _, _ = horizon_model(st, T, nx, nu, NAMES[:2], **kw)
    try:
        P.solve(model)
        monkeypatch.setattr(moi, "affine_stage_group", lambda records, small, handoff: None)
        P.solve(plain)
        assert model._overlap_moi and not model._small and model._stage_group is not None and plain._stage_group is None
        for it in range(2):
            if it:
                st.update(new_values(np.random.default_rng(40), T, nx, nu))
                P.solve(model)
                P.solve(plain)
            for (gt, gc), (wt, wc) in zip(functions(model), functions(plain)):
                assert np.array_equal(gt.view(np.int64), wt.view(np.int64)) and np.array_equal(gc.view(np.int64), wc.view(np.int64))
    finally:
        model.close()
        plain.close()


def test_a_solved_horizon_is_the_same_with_and_without_the_group(monkeypatch):
    """a small horizon QP (equality constraints only) through the KKT solve of tests/qp_solver.py: the functions are the same bit for
    bit, so the solutions are"""
    from parametron_jl_amd import moi
    from qp_solver import DenseQPOptimizer
    T, nx, nu = 10, 6, 3
    st = new_values(np.random.default_rng(77), T, nx, nu)
    st["A"], st["B"] = 0.3 * st["A"], 0.5 * st["B"]
    sols = []
    for grouped in (True, False):
        if not grouped:
            monkeypatch.setattr(moi, "affine_stage_group", lambda records, small, handoff: None)
        model, xs, us, _ = horizon_model(st, T, nx, nu, NAMES, optimizer=DenseQPOptimizer(), neighbours=False, use_graph=True, quadratic_mode="canonical")
        try:
            P.solve(model)
            assert (model._stage_group is not None) == grouped
            z = [v for vec in xs + us for v in vec]
            sols.append(np.array([P.value(model, v) for v in z]))
            if grouped:                                           # the dynamics hold at the solution
                X = [np.array([P.value(model, v) for v in vec]) for vec in xs]
                Uv = [np.array([P.value(model, v) for v in vec]) for vec in us]
                for t in range(T):
                    # x+ == A*x + B*u in the first spelling, + w in the next two; the fourth reads x+ == A*x - (w - B*u)
                    w = (0.0, 1.0, 1.0, -1.0)[t % 4] * st["w%d" % t]
                    np.testing.assert_allclose(X[t + 1], st["A"] @ X[t] + st["B"] @ Uv[t] + w, atol=1e-9)
        finally:
            model.close()
    assert np.array_equal(sols[0].view(np.int64), sols[1].view(np.int64)) and np.all(np.isfinite(sols[0]))
