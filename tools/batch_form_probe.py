"""Batched tracking-cost QPs (pmt_batch_form_coeffs_f64, batch.BatchTracking) against their two yardsticks, on one device, in one process,
alternating.  For B = 8192 instances of (n, m) = (128, 16) and (64, 16):
    form     one call of pmt_batch_form_coeffs_f64 over the batch: time per call (HIP events around `calls` calls back to back, median over `reps`
             windows) and the fraction of 8 TB/s on the algorithmic bytes 8 (n^2 + n + m n + m) + 8 L per instance
    lsq      pmt_batch_lsq_coeffs_f64 at BASELINE config 4 (n = r = 128, m = 16), the same way, on its own algorithmic bytes
             8 (r n + r + m n + m) + 8 L: the batch kernel this one stands beside
    loop     what the batch cost before the entry point existed: 64 instances looped through pmt_quad_form_shift_f64 (three launches each,
             terms + linear terms + constant; the constraint block not even included), timed as one window and scaled to B
Every timed window comes after at least 30 ms of warm-up work of the same call.
    python tools/batch_form_probe.py [--reps 15] [--calls 20] [--B 8192]                (GPU box)"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import parametron_jl_amd  # noqa: E402,F401
from parametron_jl_amd import _lib, batch  # noqa: E402

DEV = "cuda:0"
PEAK = 8e12                     # bytes/s of HBM (MI355X)
LOOPED = 64


def ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + 8 * offset)


def form_bytes(n, m):
    return 8.0 * (n * n + n + m * n + m) + 8.0 * batch.slab_layout(n, m)[1]


def lsq_bytes(n, r, m):
    return 8.0 * (r * n + r + m * n + m) + 8.0 * batch.slab_layout(n, m)[1]


def window(run, calls):
    """microseconds per call of `calls` calls back to back"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def warm(run, calls):
    """at least 30 ms of the call's own work before anything is timed"""
    spent = 0.0
    while spent < 30e3:
        spent += window(run, calls) * calls


def looped_run(wl):
    """pmt_quad_form_shift_f64 over the first LOOPED instances of the batch, one after the other"""
    n = wl.n
    nq = n * (n + 1) // 2
    x = torch.arange(1, n + 1, dtype=torch.int64, device=DEV)
    quad = torch.empty(LOOPED * 3 * nq, dtype=torch.int64, device=DEV)
    lin = torch.empty(LOOPED * 2 * n, dtype=torch.int64, device=DEV)
    cst = torch.empty(LOOPED, dtype=torch.float64, device=DEV)
    words = int(_lib.load().pmt_quad_form_shift_workspace_bytes(n)) // 8
    ws = torch.empty(words, dtype=torch.float64, device=DEV)

    def run():
        for i in range(LOOPED):
            _lib.call("pmt_quad_form_shift_f64", ptr(wl.Q, i * n * n), n, n, ptr(x), ptr(wl.p, i * n), -1, 1, ptr(x), 1.0, ptr(quad, i * 3 * nq), None,
                      ptr(lin, i * 2 * n), ptr(cst, i), ptr(ws), wl.stream)
    run.keep = (x, quad, lin, cst, ws)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--B", type=int, default=8192)
    a = ap.parse_args()
    _lib.require_gpu()
    B = a.B
    lsq = batch.BatchLSQ(torch, B, batch.N, batch.R, batch.M)
    lsq_b = lsq_bytes(batch.N, batch.R, batch.M) * B
    print("device %s, %d CUs; B = %d; medians of %d windows of %d calls, alternating; fractions of %.0f TB/s on algorithmic bytes" % (
        torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count, B, a.reps, a.calls, PEAK / 1e12), flush=True)
    for n, m in ((128, 16), (64, 16)):
        wl = batch.BatchTracking(torch, B, n, m)
        loop = looped_run(wl)
        runs = {"form": (wl.compute, a.calls), "lsq": (lsq.compute, a.calls), "loop": (loop, 1)}
        for run, calls in runs.values():
            warm(run, calls)
        t = {k: [] for k in runs}
        for _ in range(a.reps):
            for k, (run, calls) in runs.items():
                t[k].append(window(run, calls))
        torch.cuda.synchronize()
        med = {k: float(np.median(v)) for k, v in t.items()}
        fb = form_bytes(n, m) * B
        frac_form, frac_lsq = fb / (med["form"] * 1e-6) / PEAK, lsq_b / (med["lsq"] * 1e-6) / PEAK
        print("n = %3d m = %2d  form  pmt_batch_form_coeffs_f64        median %8.1f us (min %8.1f)  %7.1f MB  %5.1f %% of 8 TB/s" % (
            n, m, med["form"], min(t["form"]), fb / 1e6, 100 * frac_form))
        print("n = %3d m = %2d  lsq   pmt_batch_lsq_coeffs_f64 (C4)    median %8.1f us (min %8.1f)  %7.1f MB  %5.1f %% of 8 TB/s" % (
            batch.N, batch.M, med["lsq"], min(t["lsq"]), lsq_b / 1e6, 100 * frac_lsq))
        scaled = med["loop"] * B / LOOPED
        print("n = %3d m = %2d  loop  %d x pmt_quad_form_shift_f64      median %8.1f us (min %8.1f) = %6.1f us per instance; scaled to B: %10.1f us = %6.1f x form" % (
            n, m, LOOPED, med["loop"], min(t["loop"]), med["loop"] / LOOPED, scaled, scaled / med["form"]))
        verdict = "BELOW" if frac_form < 0.5 * frac_lsq else "not below"
        print("n = %3d m = %2d  HBM fraction of the form kernel / of the least-squares batch kernel = %.2f: %s half of it" % (n, m, frac_form / frac_lsq, verdict), flush=True)
        del wl, loop


if __name__ == "__main__":
    main()
