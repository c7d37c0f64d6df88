"""Horizon stage costs J = sum_t transpose(x_t - r_t)*Q*(x_t - r_t) + transpose(u_t)*R*u_t (pmt_quad_stages_f64, record mode "canonical-stages")
against their yardsticks, on one device, in one process, alternating.  For T x (n_x, n_u) = 12 x (40, 8), 50 x (32, 16), 100 x (64, 32) and
200 x (128, 32):
    launch   one call of pmt_quad_stages_f64 over the 2 T stages (both launches: the stages and the constant): time per call (HIP events around
             `calls` calls back to back, median over `reps` windows) and the fraction of 8 TB/s on the algorithmic bytes — the 24- and
             16-byte terms written, every distinct Q once, the vectors, the index vectors and the descriptor table read
    loop     the single-instance nodes looped over the same stages into the same slices: pmt_quad_form_shift_f64 (three launches, a
             workspace) for every x_t, pmt_quad_form_f64 for every u_t
    update   Model.update() of the host model (quadratic_mode "canonical", graph replay; host clock around the call, which ends in a device
             synchronise): this commit's plan against the plan the parent commit makes for the same model — the row does not fire there
             and the record takes the literal function through canonicalize! (moi._lsq_stages answers None: exactly the parent's decision)
Every timed window comes after at least 30 ms of warm-up work of the same call.  The two models' quadratic terms are compared bit for bit.
    python tools/quad_stages_probe.py [--reps 15] [--calls 20] [--cases 12x40x8,50x32x16,...] [--no-parent-above 200]      (GPU box)"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import parametron_jl_amd as P  # noqa: E402
from parametron_jl_amd import _lib, moi  # noqa: E402

DEV = "cuda:0"
PEAK = 8e12                     # bytes/s of HBM (MI355X)
CASES = "12x40x8,50x32x16,100x64x32,200x128x32"


def ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + 8 * offset)


def window(run, calls):
    """microseconds per call of `calls` calls back to back"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def host_window(run, calls):
    """microseconds per call on the host clock; `run` ends in a device synchronise"""
    t0 = time.perf_counter()
    for _ in range(calls):
        run()
    return (time.perf_counter() - t0) * 1e6 / calls


def warm(run, calls, win=window):
    """at least 30 ms of the call's own work before anything is timed"""
    spent = 0.0
    while spent < 30e3:
        spent += win(run, calls) * calls


def stage_bytes(T, nx, nu):
    """algorithmic bytes of one call: terms written; Q and R once, r_t, the index vectors and the table read"""
    tri = lambda n: n * (n + 1) // 2
    written = T * (24 * (tri(nx) + tri(nu)) + 16 * (nx + nu)) + 8 * 2 * T + 8
    read = 8 * (nx * nx + nu * nu) + T * 8 * nx + T * 8 * (nx + nu) + 2 * T * 56
    return float(written + read)


class Kernels:
    """the device side alone: shared Q and R, T references, the stages' slices one behind the other"""

    def __init__(self, T, nx, nu, stream):
        self.T, self.nx, self.nu, self.stream = T, nx, nu, stream
        g = torch.Generator(device="cpu").manual_seed(T)
        self.Q = torch.rand(nx * nx, generator=g, dtype=torch.float64).to(DEV)
        self.R = torch.rand(nu * nu, generator=g, dtype=torch.float64).to(DEV)
        self.r = torch.rand(T * nx, generator=g, dtype=torch.float64).to(DEV)
        nvars = T * (nx + nu)
        self.xvar = torch.arange(1, nvars + 1, dtype=torch.int64, device=DEV)
        self.varmap = torch.arange(1, nvars + 1, dtype=torch.int64, device=DEV)
        rows, qa, la = [], 0, 0
        for t in range(T):
            for n, mat, vec in ((nx, self.Q, self.r.data_ptr() + 8 * t * nx), (nu, self.R, None)):
                rows.append({"Q": mat.data_ptr(), "ldq": n, "xvar": self.xvar.data_ptr() + 8 * la, "vec": vec, "n": n, "sign": -1 if vec else 0,
                             "quad_at": qa, "lin_at": la})
                qa, la = qa + n * (n + 1) // 2, la + n
        self.rows, self.nterms, self.nlin = rows, qa, la
        arr = _lib.quad_stages(rows)
        _lib.call("pmt_quad_stages_check", C.addressof(arr), len(rows), qa, la)
        self.table = torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()).to(DEV)
        self.quad = torch.empty(3 * qa, dtype=torch.int64, device=DEV)
        self.lin = torch.empty(2 * la, dtype=torch.int64, device=DEV)
        self.consts = torch.empty(len(rows), dtype=torch.float64, device=DEV)
        self.const = torch.empty(1, dtype=torch.float64, device=DEV)
        self.ws = torch.empty(int(_lib.load().pmt_quad_form_shift_workspace_bytes(nx)) // 8, dtype=torch.float64, device=DEV)

    def launch(self):
        _lib.call("pmt_quad_stages_f64", ptr(self.table), len(self.rows), ptr(self.varmap), ptr(self.quad), ptr(self.lin), ptr(self.consts),
                  ptr(self.const), self.stream)

    def loop(self):
        for k, r in enumerate(self.rows):
            out = (ptr(self.quad, 3 * r["quad_at"]), None, ptr(self.lin, 2 * r["lin_at"]), ptr(self.consts, k))
            if r["sign"]:
                _lib.call("pmt_quad_form_shift_f64", C.c_void_p(r["Q"]), r["ldq"], r["n"], C.c_void_p(r["xvar"]), C.c_void_p(r["vec"]), r["sign"], 1,
                          ptr(self.varmap), 1.0, *out, ptr(self.ws), self.stream)
            else:
                _lib.call("pmt_quad_form_f64", C.c_void_p(r["Q"]), r["ldq"], r["n"], C.c_void_p(r["xvar"]), 1, ptr(self.varmap), 1.0, *out, self.stream)


def horizon_model(T, nx, nu, st):
    model = P.Model(P.MockOptimizer(), quadratic_mode="canonical", use_graph=True)
    Q, R = P.Parameter(lambda: st["Q"], model), P.Parameter(lambda: st["R"], model)
    expr = None
    for t in range(T):
        x, u = [P.Variable(model) for _ in range(nx)], [P.Variable(model) for _ in range(nu)]
        r = P.Parameter(lambda t=t: st["r"][t], model)
        cost = P.transpose(x - r) * Q * (x - r) + P.transpose(u) * R * u
        expr = cost if expr is None else expr + cost
    P.objective(model, P.Minimize, expr)
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
    print("device %s, %d CUs; medians of %d windows, alternating; launch / loop: %d calls a window, HIP events; update: host clock, 3 calls a window" % (
        torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count, a.reps, a.calls), flush=True)
    for case in a.cases.split(","):
        T, nx, nu = (int(v) for v in case.split("x"))
        k = Kernels(T, nx, nu, stream)
        rng = np.random.default_rng(T)
        st = {"Q": rng.random((nx, nx)), "R": rng.random((nu, nu)), "r": rng.random((T, nx))}
        new = horizon_model(T, nx, nu, st)
        new.initialize()
        assert new.objective.mode == "canonical-stages", new.objective.mode
        runs = {"launch": (k.launch, a.calls, window), "loop": (k.loop, 1, window), "update": (new.update, 3, host_window)}
        old = None
        if T <= a.no_parent_above:
            keep = moi._lsq_stages
            moi._lsq_stages = lambda terms, diag=False: None         # the parent commit's decision for this model: the literal function + canonicalize!
            try:
                old = horizon_model(T, nx, nu, st)
                old.initialize()
            finally:
                moi._lsq_stages = keep
            assert old.objective.mode == "literal" and old.objective.plan.canonicalize
            runs["parent"] = (old.update, 3, host_window)
        for run, calls, win in runs.values():
            warm(run, calls, win)
        t = {name: [] for name in runs}
        for _ in range(a.reps):
            for name, (run, calls, win) in runs.items():
                t[name].append(win(run, calls))
        torch.cuda.synchronize()
        med = {name: float(np.median(v)) for name, v in t.items()}
        nbytes = stage_bytes(T, nx, nu)
        head = "T = %3d (n_x, n_u) = (%3d, %2d)" % (T, nx, nu)
        print("%s  launch  pmt_quad_stages_f64              median %9.1f us (min %9.1f)  %7.2f MB  %5.1f %% of 8 TB/s" % (
            head, med["launch"], min(t["launch"]), nbytes / 1e6, 100 * nbytes / (med["launch"] * 1e-6) / PEAK))
        print("%s  loop    %3d x form_shift + %3d x form     median %9.1f us (min %9.1f) = %5.1f x launch" % (
            head, T, T, med["loop"], min(t["loop"]), med["loop"] / med["launch"]))
        print("%s  update  canonical-stages                 median %9.1f us (min %9.1f)" % (head, med["update"], min(t["update"])))
        if old is not None:
            print("%s  update  parent's plan (literal + canon.)  median %9.1f us (min %9.1f) = %5.1f x this commit's" % (
                head, med["parent"], min(t["parent"]), med["parent"] / med["update"]))
            a_q, b_q = new.objective.f.quadratic_terms, old.objective.f.quadratic_terms
            same = a_q.shape == b_q.shape and np.array_equal(a_q.view(np.int64), b_q.view(np.int64))
            print("%s  the two plans' %d quadratic terms are %s; constants %.17g / %.17g" % (
                head, len(a_q), "bit for bit equal" if same else "DIFFERENT", new.objective.f.constant, old.objective.f.constant), flush=True)
            old.close()
        else:
            print("%s  update  parent's plan: not measured (--no-parent-above %d)" % (head, a.no_parent_above), flush=True)
        new.close()
        del k


if __name__ == "__main__":
    main()
