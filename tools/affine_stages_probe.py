"""Horizon dynamics constraints x_{t+1} == A*x_t + B*u_t + w_t for every stage (pmt_affine_stages_f64, moi.affine_stage_group) against
their yardstick, on one device, in one process, alternating.  For T x (n_x, n_u) = 9 x (10, 4), 12 x (40, 8), 50 x (32, 16), 100 x (64, 32)
and 200 x (128, 32):
    launch   one call of pmt_affine_stages_f64 over the T records: time per call (HIP events around `calls` calls back to back, median over
             `reps` windows) and the fraction of 8 TB/s on the algorithmic bytes — the 24-byte terms and the constants written; A and B
             once, the w_t, the index vectors and the two tables read
    update   Model.update() of the host model — the stage costs as objective, the dynamics as constraints — (host clock around the call,
             which ends in a device synchronise): this commit's plan, with the group, against the plan the parent commit makes for the
             same model (moi.affine_stage_group replaced by one that returns no group: per record two assembles, the combines, the pack
             and two copies).  Both as a graph replay (use_graph) and as a replayed tape with recorded fetches (a model beyond the small
             plan by a work buffer of 300000 doubles).
Every timed window comes after at least 30 ms of warm-up work of the same call.  The two models' constraint functions are compared bit for bit.
    python tools/affine_stages_probe.py [--reps 15] [--calls 20] [--cases 9x10x4,12x40x8,...] [--modes graph,tape]      (GPU box)"""
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
CASES = "9x10x4,12x40x8,50x32x16,100x64x32,200x128x32"


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
    """algorithmic bytes of one call: terms and constants written; A and B once, w_t, the index vectors and the tables read"""
    L = 1 + nx + nu
    written = T * nx * (24 * L + 8)
    read = 8 * nx * (nx + nu) + T * 8 * nx + T * 8 * (2 * nx + nu) + T * (48 + 3 * 32)
    return float(written + read)


class Kernels:
    """the device side alone: shared A and B, T vectors w_t, the records' slices one behind the other"""

    def __init__(self, T, nx, nu, stream):
        self.T, self.stream = T, stream
        g = torch.Generator(device="cpu").manual_seed(T)
        self.A = torch.rand(nx * nx, generator=g, dtype=torch.float64).to(DEV)
        self.B = torch.rand(nx * nu, generator=g, dtype=torch.float64).to(DEV)
        self.w = torch.rand(T * nx, generator=g, dtype=torch.float64).to(DEV)
        nvars = (T + 1) * nx + T * nu
        self.xvar = torch.arange(1, nvars + 1, dtype=torch.int64, device=DEV)
        self.varmap = torch.arange(1, nvars + 1, dtype=torch.int64, device=DEV)
        L, step = 1 + nx + nu, nx + nu
        at = lambda k: self.xvar.data_ptr() + 8 * k
        parts, stages = [], []
        for t in range(T):
            parts += [{"mat": None, "xvar": at((t + 1) * step), "cols": 1, "sign": 1},
                      {"mat": self.A.data_ptr(), "ld": nx, "xvar": at(t * step), "cols": nx, "sign": -1},
                      {"mat": self.B.data_ptr(), "ld": nx, "xvar": at(t * step + nx), "cols": nu, "sign": -1}]
            stages.append({"vec": self.w.data_ptr() + 8 * t * nx, "vec_sign": -1, "rows": nx, "first_part": 3 * t, "nparts": 3, "row_len": L,
                           "term_offset": t * nx * L, "const_offset": t * nx})
        parr, sarr = _lib.affine_parts(parts), _lib.affine_stages(stages)
        _lib.call("pmt_affine_stages_check", C.addressof(sarr), T, C.addressof(parr), len(parts), T * nx * L, T * nx)
        self.stable = torch.from_numpy(np.frombuffer(sarr, dtype=np.uint8).copy()).to(DEV)
        self.ptable = torch.from_numpy(np.frombuffer(parr, dtype=np.uint8).copy()).to(DEV)
        self.terms = torch.empty(3 * T * nx * L, dtype=torch.int64, device=DEV)
        self.consts = torch.empty(T * nx, dtype=torch.float64, device=DEV)

    def launch(self):
        _lib.call("pmt_affine_stages_f64", ptr(self.stable), self.T, ptr(self.ptable), ptr(self.varmap), ptr(self.terms), ptr(self.consts), self.stream)


def horizon_model(T, nx, nu, st, graph):
    model = P.Model(P.MockOptimizer(), quadratic_mode="canonical", use_graph=graph)
    if not graph:
        P.Parameter(model, val=np.zeros(300000))        # a work buffer beside the horizon's data: beyond the small plan
    par = lambda key: P.Parameter(lambda: st[key], model)
    Q, R, A, B = par("Q"), par("R"), par("A"), par("B")
    xs = [[P.Variable(model) for _ in range(nx)]]
    expr = None
    for t in range(T):
        u = [P.Variable(model) for _ in range(nu)]
        xs.append([P.Variable(model) for _ in range(nx)])
        x, r, w = xs[t], P.Parameter(lambda t=t: st["r"][t], model), P.Parameter(lambda t=t: st["w"][t], model)
        cost = P.transpose(x - r) * Q * (x - r) + P.transpose(u) * R * u
        expr = cost if expr is None else expr + cost
        P.constraint(model, xs[t + 1], "==", A * x + B * u + w)
    P.objective(model, P.Minimize, expr)
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--cases", default=CASES)
    ap.add_argument("--modes", default="graph,tape")
    a = ap.parse_args()
    _lib.require_gpu()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    print("device %s, %d CUs; medians of %d windows, alternating; launch: %d calls a window, HIP events; update: host clock, 3 calls a window" % (
        torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count, a.reps, a.calls), flush=True)
    for case in a.cases.split(","):
        T, nx, nu = (int(v) for v in case.split("x"))
        k = Kernels(T, nx, nu, stream)
        rng = np.random.default_rng(T)
        st = {"Q": rng.random((nx, nx)), "R": rng.random((nu, nu)), "A": rng.random((nx, nx)), "B": rng.random((nx, nu)), "r": rng.random((T, nx)),
              "w": rng.random((T, nx))}
        runs = {"launch": (k.launch, a.calls, window)}
        models = {}
        for mode in a.modes.split(","):
            new = horizon_model(T, nx, nu, st, mode == "graph")
            new.initialize()
            assert new._stage_group is not None and len(new._stage_group.members) == T
            keep = moi.affine_stage_group
            moi.affine_stage_group = lambda records, small, handoff: None          # the parent commit's plan for this model
            try:
                old = horizon_model(T, nx, nu, st, mode == "graph")
                old.initialize()
            finally:
                moi.affine_stage_group = keep
            assert old._stage_group is None and not new._small and not old._small
            models[mode] = (new, old)
            runs[mode + " group"] = (new.update, 3, host_window)
            runs[mode + " parent"] = (old.update, 3, host_window)
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
        print("%s  launch  pmt_affine_stages_f64            median %9.1f us (min %9.1f)  %7.2f MB  %5.1f %% of 8 TB/s" % (
            head, med["launch"], min(t["launch"]), nbytes / 1e6, 100 * nbytes / (med["launch"] * 1e-6) / PEAK))
        for mode, (new, old) in models.items():
            g, p = mode + " group", mode + " parent"
            print("%s  update  %-5s one group of %3d records     median %9.1f us (min %9.1f)  tape %4d entries" % (
                head, mode, T, med[g], min(t[g]), new.device().tape_length()))
            print("%s  update  %-5s parent's plan (per record)   median %9.1f us (min %9.1f)  tape %4d entries = %5.2f x this commit's" % (
                head, mode, med[p], min(t[p]), old.device().tape_length(), med[p] / med[g]))
            same = all(np.array_equal(x.f.terms.view(np.int64), y.f.terms.view(np.int64)) and
                       np.array_equal(x.f.constants.view(np.int64), y.f.constants.view(np.int64)) for x, y in zip(new.constraints, old.constraints))
            print("%s  %-5s the two plans' %d constraint functions are %s" % (head, mode, len(new.constraints), "bit for bit equal" if same else "DIFFERENT"),
                  flush=True)
            new.close()
            old.close()
        del k


if __name__ == "__main__":
    main()
