"""Weighted horizon stage costs J = 0.5*(sum_t transpose(x_t - r_t)*Q*(x_t - r_t) + rho*transpose(u_t)*R*u_t) + sum_t dot(c_t, u_t) + s
(pmt_quad_stages_terms_f64, record mode "canonical-stages" with weights, linear terms and a constant beside the stages) against their
yardsticks, on one device, in one process, alternating.  For T x (n_x, n_u) = 5 x (57, 8) and 52 x (16, 8) — the two smallest models the
row fires for — and 12 x (40, 8), 50 x (32, 16), 100 x (64, 32), 200 x (128, 32):
    terms    one call of pmt_quad_stages_terms_f64 over the 2 T stages (both launches): x_t under the weight 0.5, u_t under 0.5 * rho (a
             device scalar) with the linear term c_t, one constant; time per call (HIP events around `calls` calls back to back, median
             over `reps` windows) and the fraction of 8 TB/s on the algorithmic bytes — those of the unweighted call plus 40 bytes per
             stage, the vectors c_t and the constants' table
    plain    pmt_quad_stages_f64 on the same stage table with the weights stripped — measured as two series (plain, plain') that
             alternate with `terms`: their difference is the run-to-run spread of this session
    update   Model.update() of the host model (quadratic_mode "canonical", graph replay; host clock around the call, which ends in a device
             synchronise): this commit's plan against the plan the parent commit makes for the same model — the row does not fire there
             and the record takes the literal function through canonicalize! (moi._lsq_stages answers None: exactly the parent's decision)
Every timed window comes after at least 30 ms of warm-up work of the same call.  The two models' functions are compared.
    python tools/quad_stages_terms_probe.py [--reps 15] [--calls 20] [--cases 5x57x8,...] [--no-parent-above 200]      (GPU box)"""
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
from parametron_jl_amd import _lib, moi  # noqa: E402
import quad_stages_probe as B  # noqa: E402

CASES = "5x57x8,52x16x8,12x40x8,50x32x16,100x64x32,200x128x32"


def terms_bytes(T, nx, nu):
    """algorithmic bytes of one weighted call: the unweighted call's, the terms table, the vectors c_t, the weight and the constant"""
    return B.stage_bytes(T, nx, nu) + 2 * T * 40 + T * 8 * nu + 8 + 24 + 8


class Kernels(B.Kernels):
    """the unweighted probe's device side plus the two further tables"""

    def __init__(self, T, nx, nu, stream):
        super().__init__(T, nx, nu, stream)
        g = torch.Generator(device="cpu").manual_seed(T + 1)
        self.c = torch.rand(T * nu, generator=g, dtype=torch.float64).to(B.DEV)
        self.scalars = torch.tensor([1.7, 0.3], dtype=torch.float64, device=B.DEV)          # rho, s
        rho, s = self.scalars.data_ptr(), self.scalars.data_ptr() + 8
        rows = []
        for t in range(T):
            rows += [{"scale": 0.5}, {"scale": 0.5, "weight": rho, "lin_vec": self.c.data_ptr() + 8 * t * nu}]
        tarr, carr = _lib.quad_stage_terms(rows), _lib.quad_stage_consts([{"value": s}])
        arr = _lib.quad_stages(self.rows)
        _lib.call("pmt_quad_stages_terms_check", C.addressof(arr), C.addressof(tarr), len(rows), C.addressof(carr), 1, self.nterms, self.nlin)
        self.ttable = torch.from_numpy(np.frombuffer(tarr, dtype=np.uint8).copy()).to(B.DEV)
        self.ctable = torch.from_numpy(np.frombuffer(carr, dtype=np.uint8).copy()).to(B.DEV)

    def terms(self):
        _lib.call("pmt_quad_stages_terms_f64", B.ptr(self.table), B.ptr(self.ttable), len(self.rows), B.ptr(self.ctable), 1, B.ptr(self.varmap),
                  B.ptr(self.quad), B.ptr(self.lin), B.ptr(self.consts), B.ptr(self.const), self.stream)


def weighted_model(T, nx, nu, st):
    model = P.Model(P.MockOptimizer(), quadratic_mode="canonical", use_graph=True)
    Q, R = P.Parameter(lambda: st["Q"], model), P.Parameter(lambda: st["R"], model)
    rho, s = P.Parameter(lambda: st["rho"], model), P.Parameter(lambda: st["s"], model)
    quad = lin = None
    for t in range(T):
        x, u = [P.Variable(model) for _ in range(nx)], [P.Variable(model) for _ in range(nu)]
        r, c = P.Parameter(lambda t=t: st["r"][t], model), P.Parameter(lambda t=t: st["c"][t], model)
        cost = P.transpose(x - r) * Q * (x - r) + rho * (P.transpose(u) * R * u)
        quad = cost if quad is None else quad + cost
        lin = P.dot(c, u) if lin is None else lin + P.dot(c, u)
    P.objective(model, P.Minimize, 0.5 * quad + lin + s)
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
    print("device %s, %d CUs; medians of %d windows, alternating; terms / plain: %d calls a window, HIP events; update: host clock, 3 calls a window" % (
        torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count, a.reps, a.calls), flush=True)
    for case in a.cases.split(","):
        T, nx, nu = (int(v) for v in case.split("x"))
        k = Kernels(T, nx, nu, stream)
        rng = np.random.default_rng(T)
        st = {"Q": rng.random((nx, nx)), "R": rng.random((nu, nu)), "r": rng.random((T, nx)), "c": rng.random((T, nu)), "rho": 1.7, "s": 0.3}
        new = weighted_model(T, nx, nu, st)
        new.initialize()
        assert new.objective.mode == "canonical-stages" and new.objective.plan.stage_terms is not None, new.objective.mode
        runs = {"terms": (k.terms, a.calls, B.window), "plain": (k.launch, a.calls, B.window), "plain'": (k.launch, a.calls, B.window),
                "update": (new.update, 3, B.host_window)}
        old = None
        if T <= a.no_parent_above:
            keep = moi._lsq_stages
            moi._lsq_stages = lambda terms, diag=False: None         # the parent commit's decision for this model: the literal function + canonicalize!
            try:
                old = weighted_model(T, nx, nu, st)
                old.initialize()
            finally:
                moi._lsq_stages = keep
            assert old.objective.mode == "literal" and old.objective.plan.canonicalize
            runs["parent"] = (old.update, 3, B.host_window)
        for run, calls, win in runs.values():
            B.warm(run, calls, win)
        t = {name: [] for name in runs}
        for _ in range(a.reps):
            for name, (run, calls, win) in runs.items():
                t[name].append(win(run, calls))
        torch.cuda.synchronize()
        med = {name: float(np.median(v)) for name, v in t.items()}
        nbytes = terms_bytes(T, nx, nu)
        head = "T = %3d (n_x, n_u) = (%3d, %2d)" % (T, nx, nu)
        print("%s  terms   pmt_quad_stages_terms_f64        median %9.1f us (min %9.1f)  %7.2f MB  %5.1f %% of 8 TB/s" % (
            head, med["terms"], min(t["terms"]), nbytes / 1e6, 100 * nbytes / (med["terms"] * 1e-6) / B.PEAK))
        print("%s  plain   pmt_quad_stages_f64              median %9.1f us (min %9.1f); again %9.1f us (min %9.1f): spread %.1f us; terms - plain = %+.1f us" % (
            head, med["plain"], min(t["plain"]), med["plain'"], min(t["plain'"]), abs(med["plain"] - med["plain'"]),
            med["terms"] - min(med["plain"], med["plain'"])))
        print("%s  update  canonical-stages, weighted       median %9.1f us (min %9.1f)" % (head, med["update"], min(t["update"])))
        if old is not None:
            print("%s  update  parent's plan (literal + canon.)  median %9.1f us (min %9.1f) = %5.1f x this commit's" % (
                head, med["parent"], min(t["parent"]), med["parent"] / med["update"]))
            fa, fb = new.objective.f, old.objective.f
            same = len(fa.quadratic_terms) == len(fb.quadratic_terms) and \
                np.array_equal(fa.quadratic_terms["row"], fb.quadratic_terms["row"]) and np.array_equal(fa.quadratic_terms["col"], fb.quadratic_terms["col"])
            dq = float(np.max(np.abs(fa.quadratic_terms["coeff"] - fb.quadratic_terms["coeff"]))) if same else float("nan")
            print("%s  the two plans' %d quadratic terms: indices %s, largest coefficient difference %.3g (0.5 * rho is no power of two); constants %.17g / %.17g" % (
                head, len(fa.quadratic_terms), "equal" if same else "DIFFERENT", dq, fa.constant, fb.constant), flush=True)
            old.close()
        else:
            print("%s  update  parent's plan: not measured (--no-parent-above %d)" % (head, a.no_parent_above), flush=True)
        new.close()
        del k


if __name__ == "__main__":
    main()
