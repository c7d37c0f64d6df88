"""-m gpu: the record mode "canonical-stages-csc" — a horizon objective under handoff="device" whose one launch writes the solver's CSC
values of P (pmt_quad_stages_csc_f64).

The 12 x (40, 8) horizon of tests/test_gpu_quad_stages.py in two spellings, Variables stage by stage and dealt out element by element,
Minimize and Maximize.  The yardstick is a twin model through the MOI boundary (mode "canonical-stages") with the same optimizer: what the
hand-off holds in HBM — P (x, i, p), q, r — equals the twin's MOI function scattered by optimizer index, times the sense, bit for bit,
solve after solve."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import parametron_jl_amd as P  # noqa: E402
import test_gpu_quad_stages as G  # noqa: E402
import test_gpu_quad_stages_terms as GT  # noqa: E402

NX, NU, T_H = G.NX, G.NU, G.T_H
bits = G.bits


def horizon(st, spelling, sense, interleaved, constraints=False, optimizer=None, **kw):
    """spelling "plain":    sum_t (x_t - r_t)'Q(x_t - r_t) + u_t'R u_t
       spelling "weighted": 0.5*(sum_t (x_t - r_t)'Q(x_t - r_t) + rho*dot(u_t, u_t)) + sum_t dot(c_t, u_t) + s
    over the Variables of test_gpu_quad_stages.horizon_model; `constraints`: two dense equality blocks over all variables"""
    model = P.Model(optimizer or P.MockOptimizer(variable_offset=2), quadratic_mode="canonical", **kw)
    sizes = [NX, NU] * T_H
    if interleaved:
        vecs = [[] for _ in sizes]
        for k in range(max(sizes)):
            for vec, n in zip(vecs, sizes):
                if k < n:
                    vec.append(P.Variable(model))
    else:
        vecs = [[P.Variable(model) for _ in range(n)] for n in sizes]
    Q = P.Parameter(lambda: st["Q"], model)
    quad = lin = None
    if spelling == "plain":
        R = P.Parameter(lambda: st["R"], model)
    else:
        rho, s = P.Parameter(lambda: st["rho"], model), P.Parameter(lambda: st["s"], model)
    for t in range(T_H):
        x, u = vecs[2 * t], vecs[2 * t + 1]
        r = P.Parameter(lambda t=t: st["r%d" % t], model)
        if spelling == "plain":
            cost = P.transpose(x - r) * Q * (x - r) + P.transpose(u) * R * u
        else:
            cost = P.transpose(x - r) * Q * (x - r) + rho * P.dot(u, u)
            c = P.Parameter(lambda t=t: st["c%d" % t], model)
            lin = P.dot(c, u) if lin is None else lin + P.dot(c, u)
        quad = cost if quad is None else quad + cost
    P.objective(model, sense, quad if spelling == "plain" else 0.5 * quad + lin + s)
    if constraints:
        z = [v for vec in vecs for v in vec]
        for k in range(2):
            A = P.Parameter(lambda k=k: st["A%d" % k], model)
            b = P.Parameter(lambda k=k: st["b%d" % k], model)
            P.constraint(model, A * z == b)
    return model, vecs


def new_values(seed):
    st = GT.new_values(seed)
    rng = np.random.default_rng(seed + 5)
    for k in range(2):
        st["A%d" % k], st["b%d" % k] = rng.standard_normal((3, T_H * (NX + NU))), rng.standard_normal(3)
    return st


def upper_csc(quad, nvars, sense):
    """the twin's quadratic terms (optimizer indices, 1-based) scattered into an upper-triangular CSC, times the sense -> (x, i, p)"""
    r = np.minimum(quad["row"], quad["col"]) - 1
    c = np.maximum(quad["row"], quad["col"]) - 1
    order = np.lexsort((r, c))
    assert len(set(zip(c.tolist(), r.tolist()))) == len(r)                 # a canonical function: one term per pair
    p = np.zeros(nvars + 1, dtype=np.int64)
    np.add.at(p, c + 1, 1)
    return sense * quad["coeff"][order], r[order].astype(np.int64), np.cumsum(p)


CASES = [(sp, lay, se) for sp in ("plain", "weighted") for lay in ("in-order", "interleaved") for se in ("Minimize", "Maximize")]


@pytest.mark.parametrize("spelling,layout,sense", CASES, ids=["-".join(c) for c in CASES])
def test_device_handoff_of_a_horizon_equals_the_moi_twin(spelling, layout, sense):
    st = new_values(40)
    sense_, sign = getattr(P, sense), (-1.0 if sense == "Maximize" else 1.0)
    inter = layout == "interleaved"
    model, vecs = horizon(st, spelling, sense_, inter, handoff="device")
    twin, _ = horizon(st, spelling, sense_, inter, handoff="moi", use_graph=True)
    nvars = 2 + T_H * (NX + NU)
    try:
        nbytes = []
        for it in range(3):
            if it:
                st.update(new_values(40 + 100 * it))
            P.solve(model)
            tq, tl, tc = G.solved(twin)
            obj, qp = model.objective, model.device_qp
            assert obj.mode == "canonical-stages-csc" and twin.objective.mode == "canonical-stages" and not model._small
            assert [q.mat is None for q in obj.plan.stages] == ([False, False] if spelling == "plain" else [False, True]) * T_H
            assert qp._in_tape is False and qp.nvars == nvars
            assert "quad" not in obj.dev and "P_values" not in obj.dev
            # stage by stage the record's own buffer IS P's value array; dealt out element by element the hand-off's gather places it
            assert (qp.P.values_ptr == obj.dev["P_stage_values"]) == (not inter)
            assert np.array_equal(model.model_var_to_optimizer, twin.model_var_to_optimizer)
            got = qp.fetch()
            x, i, p = upper_csc(tq, nvars, sign)
            assert np.array_equal(got["P"][2], p) and np.array_equal(got["P"][1], i), "P's pattern differs from the twin's terms"
            assert np.array_equal(bits(got["P"][0]), bits(x)), "P's values differ from the twin's coefficients"
            q = np.zeros(nvars)
            q[tl["var"] - 1] = sign * tl["coeff"]
            assert len(set(tl["var"].tolist())) == len(tl) and np.array_equal(bits(got["q"]), bits(q)), "q differs from the twin's linear terms"
            assert bits([got["r"]])[0] == bits([sign * tc])[0], "r differs from the twin's constant"
            nbytes.append(model.device().bytes_allocated())
        assert len(set(nbytes)) == 1, "plan memory grew across solves: %r" % (nbytes,)
    finally:
        model.close()
        twin.close()


@pytest.mark.parametrize("spelling", ["plain", "weighted"])
def test_the_handoffs_launches_stay_behind_the_tape_beside_side_lane_constraints(spelling):
    """two non-constant dense constraints that are eligible for the side lane: a Gram objective would move the hand-off's launches onto
    it; a stage objective writes on the plan's stream, so they run behind the tape, as for a literal objective"""
    st = new_values(7)
    model, vecs = horizon(st, spelling, P.Minimize, False, constraints=True, handoff="device")
    twin, _ = horizon(st, spelling, P.Minimize, False, constraints=True, handoff="moi", use_graph=True)
    nvars = 2 + T_H * (NX + NU)
    try:
        for it in range(2):
            if it:
                st.update(new_values(107))
            P.solve(model)
            tq, tl, tc = G.solved(twin)
            qp = model.device_qp
            assert model.objective.mode == "canonical-stages-csc" and qp._in_tape is False and qp._in_tape_lane is None
            assert sum(1 for c in model.constraints if not c.isconstant) == 2 and all(model._side_lane_ok(c) for c in model.constraints)
            assert not model.objective.plan.gram_record and "P_values" not in model.objective.dev
            got = qp.fetch()
            x, i, p = upper_csc(tq, nvars, 1.0)
            assert np.array_equal(got["P"][2], p) and np.array_equal(got["P"][1], i) and np.array_equal(bits(got["P"][0]), bits(x))
            q = np.zeros(nvars)
            q[tl["var"] - 1] = tl["coeff"]
            assert np.array_equal(bits(got["q"]), bits(q)) and bits([got["r"]])[0] == bits([tc])[0]
            Ax, Ai, Ap = got["A"]
            dense = np.zeros((6, nvars))
            for c in range(nvars):
                dense[Ai[Ap[c]:Ap[c + 1]], c] = Ax[Ap[c]:Ap[c + 1]]
            assert np.array_equal(dense[:, 2:], np.vstack([st["A0"], st["A1"]]))
    finally:
        model.close()
        twin.close()


def test_a_permuting_optimizer_keeps_the_literal_plan():
    from qp_solver import DenseQPOptimizer
    st = new_values(3)
    model, _ = horizon(st, "plain", P.Minimize, False, optimizer=DenseQPOptimizer(permute_seed=4), handoff="device")
    try:
        model.initialize()
        assert (model.objective.mode, model.objective.plan.canonicalize) == ("literal", True)
        assert "P_stage_values" not in model.objective.dev
    finally:
        model.close()
