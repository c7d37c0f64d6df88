"""Horizon stage costs with an identity-weighted input penalty, J = sum_t transpose(x_t - r_t)*Q*(x_t - r_t) + rho*dot(u_t, u_t)
(pmt_quad_stages_diag_f64, record mode "canonical-stages" with identity stages), against its yardsticks, on one device, in one process,
alternating.  For T x (n_x, n_u) = 12 x (40, 8), 50 x (32, 16), 100 x (64, 32), 200 x (128, 32) and the two smallest models of round 19,
5 x (57, 8) and 52 x (16, 8):
    diag     one call of pmt_quad_stages_diag_f64 over the 2 T stages (both launches): x_t a shifted form, u_t an identity stage under rho
             (a device scalar), no rider table; time per call (HIP events around `calls` calls back to back, median over `reps` windows)
    dense    the workaround: pmt_quad_stages_f64 over the same x_t stages and u_t as a dense form with R = rho*I — measured as two series
             (dense, dense') that alternate with `diag`: their difference is the pair's own spread in this run, the margin of the claim
             "diag is not slower than dense"
    x-only   pmt_quad_stages_f64 over the T stages x_t alone: diag - x-only is what the T identity stages cost as whole workgroups — the most
             that packing several of them into one workgroup could save
    same     the dense table itself through the two other instantiations, unit terms and no rider table — pmt_quad_stages_terms_f64 and
             pmt_quad_stages_diag_f64 writing pmt_quad_stages_f64's words: what an instantiation costs on identical work
    riders   pmt_quad_stages_diag_f64 over the dense table with a rider lam*dot(x_t - p_t, x_t - p_t) on every x_t: what one more pass of
             the tree and n more words per stage cost
    update   Model.update() of the host model (quadratic_mode "canonical", graph replay; host clock around the call, which ends in a device
             synchronise): this commit's plan, the plan the parent commit makes for the same model (the row does not fire there: the literal
             function through canonicalize!; moi._lsq_stages answering None is exactly the parent's decision) and the dense workaround's
A rho-horizon has T*(n_x^2 + n_u) literal terms: 5 x (57, 8), 52 x (16, 8) lie below the row's 2^14 (moi.GROUPS_MIN_LITERAL_TERMS) and keep
the literal path as they are; for the `update` series of such a case the threshold is lowered and the line says so.
Every timed window comes after at least 30 ms of warm-up work of the same call.
    python tools/quad_stages_diag_probe.py [--reps 15] [--calls 20] [--cases 12x40x8,...] [--no-parent-above 200]      (GPU box)"""
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

CASES = "12x40x8,50x32x16,100x64x32,200x128x32,5x57x8,52x16x8"
RHO = 1.7


def diag_bytes(T, nx, nu):
    """algorithmic bytes of one call with identity stages: terms written; Q once, r_t, the index vectors, the two tables and rho read"""
    written = T * (24 * (nx * (nx + 1) // 2 + nu) + 16 * (nx + nu)) + 8 * 2 * T + 8
    read = 8 * nx * nx + T * 8 * nx + T * 8 * (nx + nu) + 2 * T * (56 + 40) + 8
    return float(written + read)


class Kernels(B.Kernels):
    """the unweighted probe's device side with R = rho*I, plus the table with identity stages and the one with riders"""

    def __init__(self, T, nx, nu, stream):
        super().__init__(T, nx, nu, stream)
        self.R.copy_((RHO * torch.eye(nu, dtype=torch.float64)).reshape(-1))
        self.scalars = torch.tensor([RHO, 0.625], dtype=torch.float64, device=B.DEV)        # rho, lam
        rho, lam = self.scalars.data_ptr(), self.scalars.data_ptr() + 8
        g = torch.Generator(device="cpu").manual_seed(T + 2)
        self.p = torch.rand(T * nx, generator=g, dtype=torch.float64).to(B.DEV)
        rows, trows, qa = [], [], 0
        for r in self.rows:
            ident = r["n"] == nu and not r["sign"]
            rows.append(dict(r, quad_at=qa, **({"Q": None, "ldq": 0} if ident else {})))
            trows.append({"weight": rho} if ident else {})
            qa += r["n"] if ident else r["n"] * (r["n"] + 1) // 2
        self.irows, self.inq = rows, qa
        drows = [{"weight": lam, "vec": self.p.data_ptr() + 8 * (k // 2) * nx, "sign": -1} if r["sign"] else {} for k, r in enumerate(self.rows)]
        arr, tarr = _lib.quad_stages(rows), _lib.quad_stage_terms(trows)
        _lib.call("pmt_quad_stages_diag_check", C.addressof(arr), C.addressof(tarr), None, len(rows), None, 0, qa, self.nlin)
        darr, uarr, dense = _lib.quad_stage_diags(drows), _lib.quad_stage_terms([{}] * len(rows)), _lib.quad_stages(self.rows)
        _lib.call("pmt_quad_stages_diag_check", C.addressof(dense), C.addressof(uarr), C.addressof(darr), len(rows), None, 0, self.nterms, self.nlin)
        up = lambda a: torch.from_numpy(np.frombuffer(a, dtype=np.uint8).copy()).to(B.DEV)
        self.itable, self.ttable, self.dtable, self.utable = up(arr), up(tarr), up(darr), up(uarr)
        xrows = [r for r in self.rows if r["sign"]]
        xarr = _lib.quad_stages(xrows)
        _lib.call("pmt_quad_stages_check", C.addressof(xarr), len(xrows), self.nterms, self.nlin)
        self.xtable, self.nx_stages = up(xarr), len(xrows)

    def x_only(self):
        _lib.call("pmt_quad_stages_f64", B.ptr(self.xtable), self.nx_stages, B.ptr(self.varmap), B.ptr(self.quad), B.ptr(self.lin), B.ptr(self.consts),
                  B.ptr(self.const), self.stream)

    def diag(self):
        _lib.call("pmt_quad_stages_diag_f64", B.ptr(self.itable), B.ptr(self.ttable), None, len(self.rows), None, 0, B.ptr(self.varmap),
                  B.ptr(self.quad), B.ptr(self.lin), B.ptr(self.consts), B.ptr(self.const), self.stream)

    def terms_dense(self):
        _lib.call("pmt_quad_stages_terms_f64", B.ptr(self.table), B.ptr(self.utable), len(self.rows), None, 0, B.ptr(self.varmap),
                  B.ptr(self.quad), B.ptr(self.lin), B.ptr(self.consts), B.ptr(self.const), self.stream)

    def diag_dense(self):
        _lib.call("pmt_quad_stages_diag_f64", B.ptr(self.table), B.ptr(self.utable), None, len(self.rows), None, 0, B.ptr(self.varmap),
                  B.ptr(self.quad), B.ptr(self.lin), B.ptr(self.consts), B.ptr(self.const), self.stream)

    def riders(self):
        _lib.call("pmt_quad_stages_diag_f64", B.ptr(self.table), B.ptr(self.utable), B.ptr(self.dtable), len(self.rows), None, 0, B.ptr(self.varmap),
                  B.ptr(self.quad), B.ptr(self.lin), B.ptr(self.consts), B.ptr(self.const), self.stream)


def rho_model(T, nx, nu, st, dense=False):
    model = P.Model(P.MockOptimizer(), quadratic_mode="canonical", use_graph=True)
    Q = P.Parameter(lambda: st["Q"], model)
    rho = P.Parameter((lambda: st["rho"] * np.eye(nu)) if dense else (lambda: st["rho"]), model)
    expr = None
    for t in range(T):
        x, u = [P.Variable(model) for _ in range(nx)], [P.Variable(model) for _ in range(nu)]
        r = P.Parameter(lambda t=t: st["r"][t], model)
        cost = P.transpose(x - r) * Q * (x - r) + (P.transpose(u) * rho * u if dense else rho * P.dot(u, u))
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
    print("device %s, %d CUs; medians of %d windows, alternating; diag / dense / riders: %d calls a window, HIP events; update: host clock, 3 calls a window" % (
        torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count, a.reps, a.calls), flush=True)
    for case in a.cases.split(","):
        T, nx, nu = (int(v) for v in case.split("x"))
        k = Kernels(T, nx, nu, stream)
        rng = np.random.default_rng(T)
        st = {"Q": rng.random((nx, nx)), "r": rng.random((T, nx)), "rho": RHO}
        literal_terms = T * (nx * nx + nu)
        keep_min = moi.GROUPS_MIN_LITERAL_TERMS
        lowered = literal_terms < keep_min
        if lowered:
            moi.GROUPS_MIN_LITERAL_TERMS = 1 << 13
        try:
            new = rho_model(T, nx, nu, st)
            new.initialize()
            assert new.objective.mode == "canonical-stages" and any(q.mat is None for q in new.objective.plan.stages), new.objective.mode
        finally:
            moi.GROUPS_MIN_LITERAL_TERMS = keep_min
        dense = rho_model(T, nx, nu, st, dense=True)
        dense.initialize()
        assert dense.objective.mode == "canonical-stages" and dense.objective.plan.stage_terms is None
        runs = {"diag": (k.diag, a.calls, B.window), "dense": (k.launch, a.calls, B.window), "dense'": (k.launch, a.calls, B.window),
                "x-only": (k.x_only, a.calls, B.window), "terms-dense": (k.terms_dense, a.calls, B.window),
                "diag-dense": (k.diag_dense, a.calls, B.window), "riders": (k.riders, a.calls, B.window), "update": (new.update, 3, B.host_window), "dense-update": (dense.update, 3, B.host_window)}
        old = None
        if T <= a.no_parent_above:
            keep = moi._lsq_stages
            moi._lsq_stages = lambda terms, diag=False: None     # the parent commit's decision for this model: the literal function + canonicalize!
            try:
                old = rho_model(T, nx, nu, st)
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
        nbytes, dbytes = diag_bytes(T, nx, nu), B.stage_bytes(T, nx, nu)
        head = "T = %3d (n_x, n_u) = (%3d, %2d)" % (T, nx, nu)
        spread = abs(med["dense"] - med["dense'"])
        best = min(med["dense"], med["dense'"])
        print("%s  diag    pmt_quad_stages_diag_f64         median %9.1f us (min %9.1f)  %7.2f MB  %5.1f %% of 8 TB/s" % (
            head, med["diag"], min(t["diag"]), nbytes / 1e6, 100 * nbytes / (med["diag"] * 1e-6) / B.PEAK))
        print("%s  dense   pmt_quad_stages_f64, R = rho*I   median %9.1f us (min %9.1f); again %9.1f us (min %9.1f): spread %.1f us  %7.2f MB;"
              " diag - dense = %+.1f us: %s" % (head, med["dense"], min(t["dense"]), med["dense'"], min(t["dense'"]), spread, dbytes / 1e6,
                                               med["diag"] - best, "not slower" if med["diag"] <= best + spread else "SLOWER beyond the spread"))
        print("%s  x-only  pmt_quad_stages_f64, the x_t alone  median %9.1f us (min %9.1f): the %d identity stages cost %+.1f us" % (
            head, med["x-only"], min(t["x-only"]), T, med["diag"] - med["x-only"]))
        print("%s  same    the dense table, unit terms: pmt_quad_stages_terms_f64 median %9.1f us = dense %+.1f us; pmt_quad_stages_diag_f64 %9.1f us = dense %+.1f us" % (
            head, med["terms-dense"], med["terms-dense"] - best, med["diag-dense"], med["diag-dense"] - best))
        print("%s  riders  the dense table + a rider per x_t median %9.1f us (min %9.1f) = dense %+.1f us" % (
            head, med["riders"], min(t["riders"]), med["riders"] - best))
        print("%s  update  canonical-stages, rho*dot(u, u)  median %9.1f us (min %9.1f)%s" % (
            head, med["update"], min(t["update"]), "  [%d literal terms < 2^14: fires only with the threshold lowered]" % literal_terms if lowered else ""))
        print("%s  update  canonical-stages, R = rho*I      median %9.1f us (min %9.1f) = %5.2f x this commit's" % (
            head, med["dense-update"], min(t["dense-update"]), med["dense-update"] / med["update"]))
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
        dense.close()
        del k


if __name__ == "__main__":
    main()
