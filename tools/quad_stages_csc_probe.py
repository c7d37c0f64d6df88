"""Horizon stage costs under the device hand-off, J = sum_t transpose(x_t - r_t)*Q*(x_t - r_t) + transpose(u_t)*R*u_t (pmt_quad_stages_csc_f64,
record mode "canonical-stages-csc"), against its yardsticks, on one device, in one process, alternating.  For T x (n_x, n_u) = 12 x (40, 8),
50 x (32, 16), 100 x (64, 32), 200 x (128, 32) and the two smallest firing models, 5 x (57, 8) and 52 x (16, 8):
    update   Model.update() of the model under handoff="device" (MockOptimizer(variable_offset=2), quadratic_mode "canonical"): the tape and the
             hand-off's launches behind it, ending in a device synchronise; host clock around the call.  This commit's plan, and the plan the
             parent commit makes for the same model — quad_plan called without stage_csc, which is exactly the parent's decision: the literal
             function through canonicalize!, its 24-byte terms gathered back into P.  Variables stage by stage and dealt out element by
             element (the second only for this commit's plan: the hand-off's gather places the values, one more launch).
    launch   one call of pmt_quad_stages_csc_f64 (both launches) against pmt_quad_stages_diag_f64 on the same tables — unit terms, no riders,
             the MOI slices and the value slices one behind the other — in alternating windows (HIP events around `calls` calls back to back);
             `diag` is measured as two series whose difference is the pair's own spread in this run.  Stage by stage and interleaved
             (only the index words differ); interleaved also followed by the hand-off's pmt_csc_values_gather_f64 over the same values.
Every timed window comes after at least 30 ms of warm-up work of the same call; medians over `reps` windows.
    python tools/quad_stages_csc_probe.py [--reps 15] [--calls 20] [--cases 12x40x8,...] [--no-parent-above 200]      (GPU box)"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parametron_jl_amd as P  # noqa: E402
from parametron_jl_amd import _lib, handoff, moi  # noqa: E402
import quad_stages_probe as B  # noqa: E402

CASES = "12x40x8,50x32x16,100x64x32,200x128x32,5x57x8,52x16x8"


def csc_bytes(T, nx, nu):
    """algorithmic bytes of one call: values and linear terms written; Q and R once, r_t, the index vectors and the two tables read"""
    tri = lambda n: n * (n + 1) // 2
    written = T * (8 * (tri(nx) + tri(nu)) + 16 * (nx + nu)) + 8 * 2 * T + 8
    read = 8 * (nx * nx + nu * nu) + T * 8 * nx + T * 8 * (nx + nu) + 2 * T * (56 + 40)
    return float(written + read)


def variable_sets(T, nx, nu, interleaved):
    """the stages' model indices (1-based), x_0, u_0, x_1, ..: consecutive, or dealt out element by element"""
    sizes = [nx, nu] * T
    if not interleaved:
        start = np.concatenate([[1], 1 + np.cumsum(sizes)])
        return [np.arange(start[k], start[k] + n, dtype=np.int64) for k, n in enumerate(sizes)]
    sets, nxt = [[] for _ in sizes], 1
    for k in range(max(sizes)):
        for s, n in zip(sets, sizes):
            if k < n:
                s.append(nxt)
                nxt += 1
    return [np.array(s, dtype=np.int64) for s in sets]


class Kernels(B.Kernels):
    """the unweighted probe's device side over the given variable sets: the MOI table with unit terms for pmt_quad_stages_diag_f64, the same
    stages with value slices for pmt_quad_stages_csc_f64, and the hand-off's gather of those values into CSC order"""

    def __init__(self, T, nx, nu, stream, interleaved):
        super().__init__(T, nx, nu, stream)
        sets = variable_sets(T, nx, nu, interleaved)
        self.sets = torch.from_numpy(np.concatenate(sets)).to(B.DEV)
        rows, at = [], 0
        for r, s in zip(self.rows, sets):
            rows.append(dict(r, xvar=self.sets.data_ptr() + 8 * r["lin_at"]))
            assert len(s) == r["n"]
        order = np.argsort([int(s[0]) for s in sets], kind="stable")
        val_at = np.zeros(len(rows), dtype=np.int64)
        for k in order:
            val_at[k], at = at, at + rows[k]["n"] * (rows[k]["n"] + 1) // 2
        crows = [dict(r, quad_at=int(a)) for r, a in zip(rows, val_at)]
        self.nvalues = at
        arr, carr, uarr = _lib.quad_stages(rows), _lib.quad_stages(crows), _lib.quad_stage_terms([{}] * len(rows))
        _lib.call("pmt_quad_stages_diag_check", C.addressof(arr), C.addressof(uarr), None, len(rows), None, 0, self.nterms, self.nlin)
        _lib.call("pmt_quad_stages_csc_check", C.addressof(carr), C.addressof(uarr), None, len(rows), None, 0, at, self.nlin)
        up = lambda a: torch.from_numpy(np.frombuffer(a, dtype=np.uint8).copy()).to(B.DEV)
        self.dtable, self.ctable, self.utable = up(arr), up(carr), up(uarr)
        self.values = torch.empty(at, dtype=torch.float64, device=B.DEV)
        self.P = torch.empty(at, dtype=torch.float64, device=B.DEV)
        # the hand-off's gather (handoff.DeviceQP._build_matrix): one term address per entry of P in CSC order
        n = T * (nx + nu)
        rr, cc = handoff.stage_blocks_pattern([(s, int(a), False) for s, a in zip(sets, val_at)], at)
        perm, seg, _, _ = handoff._csc_order(rr, cc, n, n, True)
        self.in_csc_order = bool(np.array_equal(perm, np.arange(at)))
        self.addr = torch.from_numpy((np.uint64(self.values.data_ptr()) + perm.astype(np.uint64) * np.uint64(8)).view(np.int64)).to(B.DEV)
        self.seg = torch.from_numpy(np.ascontiguousarray(seg, dtype=np.int64)).to(B.DEV)

    def diag(self):
        _lib.call("pmt_quad_stages_diag_f64", B.ptr(self.dtable), B.ptr(self.utable), None, len(self.rows), None, 0, B.ptr(self.varmap),
                  B.ptr(self.quad), B.ptr(self.lin), B.ptr(self.consts), B.ptr(self.const), self.stream)

    def csc(self):
        _lib.call("pmt_quad_stages_csc_f64", B.ptr(self.ctable), B.ptr(self.utable), None, len(self.rows), None, 0, B.ptr(self.varmap), 1.0,
                  B.ptr(self.values), B.ptr(self.lin), B.ptr(self.consts), B.ptr(self.const), self.stream)

    def csc_gather(self):
        self.csc()
        _lib.call("pmt_csc_values_gather_f64", B.ptr(self.addr), self.nvalues, B.ptr(self.seg), self.nvalues, 1.0, None, B.ptr(self.P), self.stream)


def device_model(T, nx, nu, st, interleaved=False):
    model = P.Model(P.MockOptimizer(variable_offset=2), quadratic_mode="canonical", handoff="device")
    sizes = [nx, nu] * T
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
    for t in range(T):
        x, u = vecs[2 * t], vecs[2 * t + 1]
        r = P.Parameter(lambda t=t: st["r"][t], model)
        cost = P.transpose(x - r) * Q * (x - r) + P.transpose(u) * R * u
        expr = cost if expr is None else expr + cost
    P.objective(model, P.Minimize, expr)
    return model


def parent_model(*args):
    """the same model as the parent commit plans it: quad_plan without the keyword"""
    real = moi.quad_plan
    moi.quad_plan = lambda *a, **k: real(*a, **dict(k, stage_csc=False))
    try:
        model = device_model(*args)
        model.initialize()
    finally:
        moi.quad_plan = real
    assert model.objective.mode == "literal" and model.objective.plan.canonicalize
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--cases", default=CASES)
    ap.add_argument("--no-parent-above", type=int, default=200, help="skip the parent's plan for horizons of more stages than this")
    a = ap.parse_args()
    _lib.require_gpu()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    print("device %s, %d CUs; medians of %d windows, alternating; launches: %d calls a window, HIP events; update: host clock, 3 calls a window "
          "(the parent's plan: 1)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count, a.reps, a.calls), flush=True)
    for case in a.cases.split(","):
        T, nx, nu = (int(v) for v in case.split("x"))
        head = "T = %3d (n_x, n_u) = (%3d, %2d)" % (T, nx, nu)
        rng = np.random.default_rng(T)
        st = {"Q": rng.random((nx, nx)), "R": rng.random((nu, nu)), "r": rng.random((T, nx))}
        k, ki = Kernels(T, nx, nu, stream, False), Kernels(T, nx, nu, stream, True)
        assert k.in_csc_order and not ki.in_csc_order
        new, newi = device_model(T, nx, nu, st), device_model(T, nx, nu, st, interleaved=True)
        for m, own in ((new, True), (newi, False)):
            m.initialize()
            assert m.objective.mode == "canonical-stages-csc", m.objective.mode
            assert (m.device_qp.P.values_ptr == m.objective.dev["P_stage_values"]) == own
        runs = {"csc": (k.csc, a.calls, B.window), "diag": (k.diag, a.calls, B.window), "diag'": (k.diag, a.calls, B.window),
                "csc-i": (ki.csc, a.calls, B.window), "diag-i": (ki.diag, a.calls, B.window), "csc-i+gather": (ki.csc_gather, a.calls, B.window),
                "update": (new.update, 3, B.host_window), "update-i": (newi.update, 3, B.host_window)}
        old = None
        if T <= a.no_parent_above:
            old = parent_model(T, nx, nu, st)
            runs["parent"] = (old.update, 1, B.host_window)
        for run, calls, win in runs.values():
            B.warm(run, calls, win)
        t = {name: [] for name in runs}
        for _ in range(a.reps):
            for name, (run, calls, win) in runs.items():
                t[name].append(win(run, calls))
        torch.cuda.synchronize()
        med = {name: float(np.median(v)) for name, v in t.items()}
        nbytes, dbytes = csc_bytes(T, nx, nu), B.stage_bytes(T, nx, nu) + 2 * T * 40
        spread, best = abs(med["diag"] - med["diag'"]), min(med["diag"], med["diag'"])
        verdict = lambda x, ref: "not slower" if x <= ref + spread else "SLOWER beyond the spread"
        print("%s  launch  pmt_quad_stages_csc_f64          median %9.1f us (min %9.1f)  %7.2f MB  %5.1f %% of 8 TB/s" % (
            head, med["csc"], min(t["csc"]), nbytes / 1e6, 100 * nbytes / (med["csc"] * 1e-6) / B.PEAK))
        print("%s  launch  pmt_quad_stages_diag_f64         median %9.1f us (min %9.1f); again %9.1f us (min %9.1f): spread %.1f us  %7.2f MB;"
              " csc - diag = %+.1f us: %s" % (head, med["diag"], min(t["diag"]), med["diag'"], min(t["diag'"]), spread, dbytes / 1e6,
                                             med["csc"] - best, verdict(med["csc"], best)))
        print("%s  launch  interleaved: csc %9.1f us (min %9.1f), diag %9.1f us (min %9.1f): csc - diag = %+.1f us: %s; csc + the hand-off's gather"
              " %9.1f us (min %9.1f) = csc %+.1f us" % (head, med["csc-i"], min(t["csc-i"]), med["diag-i"], min(t["diag-i"]), med["csc-i"] - med["diag-i"],
                                                       verdict(med["csc-i"], med["diag-i"]), med["csc-i+gather"], min(t["csc-i+gather"]),
                                                       med["csc-i+gather"] - med["csc-i"]))
        print("%s  update  canonical-stages-csc, stage by stage  median %9.1f us (min %9.1f); interleaved (with the gather) %9.1f us (min %9.1f)" % (
            head, med["update"], min(t["update"]), med["update-i"], min(t["update-i"])))
        if old is not None:
            print("%s  update  parent's plan (literal + canon. + gather)  median %9.1f us (min %9.1f) = %6.1f x this commit's" % (
                head, med["parent"], min(t["parent"]), med["parent"] / med["update"]))
            ga, gb = new.device_qp.fetch(), old.device_qp.fetch()
            same = all(np.array_equal(x, y) for x, y in zip(ga["P"][1:], gb["P"][1:]))
            err = float(np.max(np.abs(ga["P"][0] - gb["P"][0]))) if same else float("nan")
            print("%s  the two plans' P: pattern %s, %d values, max |difference| %.3g; q max |difference| %.3g" % (
                head, "equal" if same else "DIFFERENT", len(ga["P"][0]), err, float(np.max(np.abs(ga["q"] - gb["q"])))), flush=True)
            old.close()
        else:
            print("%s  update  parent's plan: not measured (--no-parent-above %d)" % (head, a.no_parent_above), flush=True)
        new.close()
        newi.close()
        del k, ki


if __name__ == "__main__":
    main()
