"""Batched MPC horizons (pmt_batch_horizon_coeffs_f64, batch.BatchHorizon) against the two routes the batch had before the entry point existed
and beside the sibling batch kernels, on one device, in one process, alternating.  For B = 8192 instances of every (T, nx, nu, m) below:
    horizon  one call of pmt_batch_horizon_coeffs_f64 over the batch: time per call back to back (HIP events around `calls` calls, median
             over `reps` windows) and cold (one call behind a 512 MiB write to another buffer, median over `reps`), and the fraction of
             8 TB/s on the algorithmic bytes 8 (nx^2 + nu^2 + T nx + T nu + m n + m) + 8 L per instance
    loop     64 instances looped through pmt_quad_stages_check + pmt_quad_stages_f64 (the tables built beforehand; two launches per
             instance; the constraint block not even included), timed as one window and scaled to B
    dense    where n = T (nx + nu) <= 256: batch.BatchTracking on n x n matrices — what the horizon's block-diagonal matrix held dense costs
    form     pmt_batch_form_coeffs_f64 at (n, m) = (128, 16) and
    lsq      pmt_batch_lsq_coeffs_f64 at BASELINE config 4, each on its own algorithmic bytes: the siblings' fractions in the same run
Every timed window comes after at least 30 ms of warm-up work of the same call.
    python tools/batch_horizon_probe.py [--reps 15] [--calls 20] [--B 8192]                (GPU box)"""
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
SHAPES = [(32, 32, 16, 0), (32, 32, 16, 32), (20, 12, 4, 12), (16, 128, 32, 0), (8, 16, 8, 0)]


def ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + 8 * offset)


def horizon_bytes(T, nx, nu, m):
    n = T * (nx + nu)
    return 8.0 * (nx * nx + nu * nu + T * nx + T * nu + m * n + m) + 8.0 * batch.horizon_slab_layout(T, nx, nu, m)[1]


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


def cold(run, flush, reps):
    """microseconds of one call behind a write of 512 MiB to another buffer"""
    out = []
    for k in range(reps):
        flush.fill_(float(k))
        out.append(window(run, 1))
    return out


def looped_run(wl):
    """pmt_quad_stages_check + pmt_quad_stages_f64 over the first LOOPED instances of the batch, one after the other: the instance's table
    [x_0, u_0, x_1, ..] over its own Q_i, R_i and references (u_t plain, as BatchHorizon.compute)"""
    T, nx, nu, n = wl.T, wl.nx, wl.nu, wl.n
    nterms = T * (nx * (nx + 1) // 2 + nu * (nu + 1) // 2)
    x = torch.arange(1, n + 1, dtype=torch.int64, device=DEV)
    quad = torch.empty(LOOPED * 3 * nterms, dtype=torch.int64, device=DEV)
    lin = torch.empty(LOOPED * 2 * n, dtype=torch.int64, device=DEV)
    nst = T * (2 if nu else 1)
    consts = torch.empty(LOOPED * nst, dtype=torch.float64, device=DEV)
    cst = torch.empty(LOOPED, dtype=torch.float64, device=DEV)
    hosts, tables = [], []
    for i in range(LOOPED):
        rows, qa, la = [], 0, 0
        for t in range(T):
            rows.append({"Q": wl.Q.data_ptr() + 8 * i * nx * nx, "ldq": nx, "xvar": x.data_ptr() + 8 * la, "vec": wl.r.data_ptr() + 8 * (i * T + t) * nx,
                         "n": nx, "sign": -1, "quad_at": qa, "lin_at": la})
            qa, la = qa + nx * (nx + 1) // 2, la + nx
            if nu:
                rows.append({"Q": wl.R.data_ptr() + 8 * i * nu * nu, "ldq": nu, "xvar": x.data_ptr() + 8 * la, "vec": None, "n": nu, "sign": 0,
                             "quad_at": qa, "lin_at": la})
                qa, la = qa + nu * (nu + 1) // 2, la + nu
        arr = _lib.quad_stages(rows)
        hosts.append(arr)
        tables.append(torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()).to(DEV))

    def run():
        for i in range(LOOPED):
            _lib.call("pmt_quad_stages_check", C.addressof(hosts[i]), nst, nterms, n)
            _lib.call("pmt_quad_stages_f64", ptr(tables[i]), nst, ptr(x), ptr(quad, i * 3 * nterms), ptr(lin, i * 2 * n), ptr(consts, i * nst),
                      ptr(cst, i), wl.stream)
    run.keep = (x, quad, lin, consts, cst, hosts, tables)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--B", type=int, default=8192)
    a = ap.parse_args()
    _lib.require_gpu()
    B = a.B
    flush = torch.empty(512 << 17, dtype=torch.float64, device=DEV)
    lsq = batch.BatchLSQ(torch, B, batch.N, batch.R, batch.M)
    form = batch.BatchTracking(torch, B, batch.N, batch.M)
    lsq_b, form_b = lsq_bytes(batch.N, batch.R, batch.M) * B, form_bytes(batch.N, batch.M) * B
    print("device %s, %d CUs; B = %d; medians of %d windows of %d calls, alternating; fractions of %.0f TB/s on algorithmic bytes" % (
        torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count, B, a.reps, a.calls, PEAK / 1e12), flush=True)
    for T, nx, nu, m in SHAPES:
        wl = batch.BatchHorizon(torch, B, T, nx, nu, m)
        n = wl.n
        tag = "T = %3d nx = %3d nu = %2d m = %2d " % (T, nx, nu, m)
        loop = looped_run(wl)
        runs = {"horizon": (wl.compute, a.calls), "form": (form.compute, a.calls), "lsq": (lsq.compute, a.calls), "loop": (loop, 1)}
        dense = batch.BatchTracking(torch, B, n, m) if n <= 256 else None
        if dense is not None:
            runs["dense"] = (dense.compute, a.calls)
        for run, calls in runs.values():
            warm(run, calls)
        t = {k: [] for k in runs}
        for _ in range(a.reps):
            for k, (run, calls) in runs.items():
                t[k].append(window(run, calls))
        tc = cold(wl.compute, flush, a.reps)
        torch.cuda.synchronize()
        med = {k: float(np.median(v)) for k, v in t.items()}
        hb = horizon_bytes(T, nx, nu, m) * B
        print(tag + "horizon pmt_batch_horizon_coeffs_f64      median %8.1f us (min %8.1f)  %7.1f MB  %5.1f %% of 8 TB/s; cold median %8.1f us (min %8.1f)  %5.1f %%" % (
            med["horizon"], min(t["horizon"]), hb / 1e6, 100 * hb / (med["horizon"] * 1e-6) / PEAK, float(np.median(tc)), min(tc),
            100 * hb / (float(np.median(tc)) * 1e-6) / PEAK))
        print(tag + "form    pmt_batch_form_coeffs_f64 (128,16) median %8.1f us (min %8.1f)  %7.1f MB  %5.1f %% of 8 TB/s" % (
            med["form"], min(t["form"]), form_b / 1e6, 100 * form_b / (med["form"] * 1e-6) / PEAK))
        print(tag + "lsq     pmt_batch_lsq_coeffs_f64 (C4)      median %8.1f us (min %8.1f)  %7.1f MB  %5.1f %% of 8 TB/s" % (
            med["lsq"], min(t["lsq"]), lsq_b / 1e6, 100 * lsq_b / (med["lsq"] * 1e-6) / PEAK))
        scaled = med["loop"] * B / LOOPED
        print(tag + "loop    %d x (check + pmt_quad_stages_f64)  median %8.1f us (min %8.1f) = %6.1f us per instance; scaled to B: %10.1f us = %7.1f x horizon" % (
            LOOPED, med["loop"], min(t["loop"]), med["loop"] / LOOPED, scaled, scaled / med["horizon"]))
        if dense is not None:
            db = form_bytes(n, m) * B
            print(tag + "dense   pmt_batch_form_coeffs_f64 (n = %d)  median %8.1f us (min %8.1f)  %7.1f MB moved = %5.1f x horizon's bytes; %5.1f x horizon's time" % (
                n, med["dense"], min(t["dense"]), db / 1e6, db / hb, med["dense"] / med["horizon"]))
        sys.stdout.flush()
        del wl, loop, dense, runs


if __name__ == "__main__":
    main()
