"""Batched horizons with a terminal cost, stage weights and linear stage terms (pmt_batch_horizon_terms_coeffs_f64,
batch.BatchWeightedHorizon) against the parent entry point and against the only route such a fleet had before, on one device, in one
process, alternating.  For B = 8192 instances of every (T, nx, nu, m) below:
    parent   one call of pmt_batch_horizon_coeffs_f64 (batch.BatchHorizon): the yardstick
    unit     one call of pmt_batch_horizon_terms_coeffs_f64 with every optional array absent, on inputs of the same sizes: what the
             generality costs (ratio unit / parent)
    full     the same entry point with a terminal stage, weights and linear vectors: time per call back to back (HIP events around `calls`
             calls, median over `reps` windows) and cold (one call behind a 512 MiB write to another buffer), and the fraction of 8 TB/s on
             its algorithmic bytes 8 (inputs read) + 8 L per instance
    loop     64 instances looped through pmt_quad_stages_terms_check + pmt_quad_stages_terms_f64 (the three tables built beforehand; two
             launches per instance; the constraint block not even included), timed as one window and scaled to B
    form     pmt_batch_form_coeffs_f64 at (n, m) = (128, 16) and
    lsq      pmt_batch_lsq_coeffs_f64 at BASELINE config 4, each on its own algorithmic bytes: the siblings' fractions in the same run
Every timed window comes after at least 30 ms of warm-up work of the same call.  The report goes to stdout and to --out.
    python tools/batch_horizon_terms_probe.py [--reps 15] [--calls 20] [--B 8192] [--out profiles/r24_batch_horizon_terms.txt]     (GPU box)"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import parametron_jl_amd  # noqa: E402,F401
from parametron_jl_amd import _lib, batch  # noqa: E402
from batch_horizon_probe import DEV, LOOPED, PEAK, SHAPES, cold, form_bytes, horizon_bytes, lsq_bytes, ptr, warm, window  # noqa: E402


def terms_bytes(wl):
    """algorithmic bytes of one instance: every input array read once, the slab written"""
    return 8.0 * sum(wl.per.values()) + 8.0 * wl.L


def looped_run(wl):
    """pmt_quad_stages_terms_check + pmt_quad_stages_terms_f64 over the first LOOPED instances of the full form, one after the other: the
    instance's table [x_0, u_0, .., x_T] over its own Q_i, R_i, P_i, references, weights (scale 1.0, weight = &W_s) and linear vectors
    (u_t plain, as BatchWeightedHorizon.compute)"""
    T, nx, nu, n = wl.T, wl.nx, wl.nu, wl.n
    nqx, nqu = nx * (nx + 1) // 2, nu * (nu + 1) // 2
    nterms = T * (nqx + nqu) + nqx
    nst = T * (2 if nu else 1) + 1
    x = torch.arange(1, n + 1, dtype=torch.int64, device=DEV)
    quad = torch.empty(LOOPED * 3 * nterms, dtype=torch.int64, device=DEV)
    lin = torch.empty(LOOPED * 2 * n, dtype=torch.int64, device=DEV)
    consts = torch.empty(LOOPED * nst, dtype=torch.float64, device=DEV)
    cst = torch.empty(LOOPED, dtype=torch.float64, device=DEV)
    none = _lib.quad_stage_consts([])
    dnone = torch.zeros(32, dtype=torch.uint8, device=DEV)
    p = {k: t.data_ptr() for k, t in wl.inputs.items()}
    hosts, tables = [], []
    for i in range(LOOPED):
        rows, terms, qa, la = [], [], 0, 0

        def stage(M, nd, vec, weight, lin_vec):
            nonlocal qa, la
            rows.append({"Q": M, "ldq": nd, "xvar": x.data_ptr() + 8 * la, "vec": vec, "n": nd, "sign": -1 if vec else 0, "quad_at": qa, "lin_at": la})
            terms.append({"weight": weight, "lin_vec": lin_vec})
            qa, la = qa + nd * (nd + 1) // 2, la + nd
        for t in range(T):
            stage(p["Q"] + 8 * i * nx * nx, nx, p["r"] + 8 * (i * T + t) * nx, p["wx"] + 8 * (i * T + t), p["gx"] + 8 * (i * T + t) * nx)
            if nu:
                stage(p["R"] + 8 * i * nu * nu, nu, None, p["wu"] + 8 * (i * T + t), p["gu"] + 8 * (i * T + t) * nu)
        stage(p["P"] + 8 * i * nx * nx, nx, p["rN"] + 8 * i * nx, p["wN"] + 8 * i, p["gN"] + 8 * i * nx)
        arr, tarr = _lib.quad_stages(rows), _lib.quad_stage_terms(terms)
        hosts.append((arr, tarr))
        tables.append(tuple(torch.from_numpy(np.frombuffer(a, dtype=np.uint8).copy()).to(DEV) for a in (arr, tarr)))

    def run():
        for i in range(LOOPED):
            _lib.call("pmt_quad_stages_terms_check", C.addressof(hosts[i][0]), C.addressof(hosts[i][1]), nst, C.addressof(none), 0, nterms, n)
            _lib.call("pmt_quad_stages_terms_f64", ptr(tables[i][0]), ptr(tables[i][1]), nst, ptr(dnone), 0, ptr(x), ptr(quad, i * 3 * nterms),
                      ptr(lin, i * 2 * n), ptr(consts, i * nst), ptr(cst, i), wl.stream)
    run.keep = (x, quad, lin, consts, cst, hosts, tables, none, dnone)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_batch_horizon_terms.txt"))
    a = ap.parse_args()
    _lib.require_gpu()
    B = a.B
    report = open(a.out, "w")

    def say(line):
        print(line, flush=True)
        report.write(line + "\n")
        report.flush()
    flush = torch.empty(512 << 17, dtype=torch.float64, device=DEV)
    lsq = batch.BatchLSQ(torch, B, batch.N, batch.R, batch.M)
    form = batch.BatchTracking(torch, B, batch.N, batch.M)
    lsq_b, form_b = lsq_bytes(batch.N, batch.R, batch.M) * B, form_bytes(batch.N, batch.M) * B
    say("device %s, %d CUs; B = %d; medians of %d windows of %d calls, alternating; fractions of %.0f TB/s on algorithmic bytes" % (
        torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count, B, a.reps, a.calls, PEAK / 1e12))
    for T, nx, nu, m in SHAPES:
        parent = batch.BatchHorizon(torch, B, T, nx, nu, m)
        unit = batch.BatchWeightedHorizon(torch, B, T, nx, nu, m, terminal=False, weights=False, linear=False)
        full = batch.BatchWeightedHorizon(torch, B, T, nx, nu, m)
        tag = "T = %3d nx = %3d nu = %2d m = %2d " % (T, nx, nu, m)
        loop = looped_run(full)
        runs = {"parent": (parent.compute, a.calls), "unit": (unit.compute, a.calls), "full": (full.compute, a.calls), "form": (form.compute, a.calls),
                "lsq": (lsq.compute, a.calls), "loop": (loop, 1)}
        for run, calls in runs.values():
            warm(run, calls)
        t = {k: [] for k in runs}
        for _ in range(a.reps):
            for k, (run, calls) in runs.items():
                t[k].append(window(run, calls))
        tc = cold(full.compute, flush, a.reps)
        torch.cuda.synchronize()
        med = {k: float(np.median(v)) for k, v in t.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in t.items()}
        pb, ub, fb = horizon_bytes(T, nx, nu, m) * B, terms_bytes(unit) * B, terms_bytes(full) * B
        say(tag + "parent  pmt_batch_horizon_coeffs_f64            median %8.1f us (min %8.1f, spread %4.1f %%)  %7.1f MB  %5.1f %% of 8 TB/s" % (
            med["parent"], min(t["parent"]), 100 * spread["parent"], pb / 1e6, 100 * pb / (med["parent"] * 1e-6) / PEAK))
        say(tag + "unit    pmt_batch_horizon_terms_coeffs_f64, none median %8.1f us (min %8.1f, spread %4.1f %%)  %7.1f MB  %5.1f %% of 8 TB/s; %5.3f x parent" % (
            med["unit"], min(t["unit"]), 100 * spread["unit"], ub / 1e6, 100 * ub / (med["unit"] * 1e-6) / PEAK, med["unit"] / med["parent"]))
        say(tag + "full    pmt_batch_horizon_terms_coeffs_f64, all  median %8.1f us (min %8.1f, spread %4.1f %%)  %7.1f MB  %5.1f %% of 8 TB/s; cold median %8.1f us (min %8.1f)  %5.1f %%" % (
            med["full"], min(t["full"]), 100 * spread["full"], fb / 1e6, 100 * fb / (med["full"] * 1e-6) / PEAK, float(np.median(tc)), min(tc),
            100 * fb / (float(np.median(tc)) * 1e-6) / PEAK))
        say(tag + "form    pmt_batch_form_coeffs_f64 (128,16)      median %8.1f us (min %8.1f)  %7.1f MB  %5.1f %% of 8 TB/s" % (
            med["form"], min(t["form"]), form_b / 1e6, 100 * form_b / (med["form"] * 1e-6) / PEAK))
        say(tag + "lsq     pmt_batch_lsq_coeffs_f64 (C4)           median %8.1f us (min %8.1f)  %7.1f MB  %5.1f %% of 8 TB/s" % (
            med["lsq"], min(t["lsq"]), lsq_b / 1e6, 100 * lsq_b / (med["lsq"] * 1e-6) / PEAK))
        scaled = med["loop"] * B / LOOPED
        say(tag + "loop    %d x (check + pmt_quad_stages_terms_f64) median %8.1f us (min %8.1f) = %6.1f us per instance; scaled to B: %10.1f us = %7.1f x full" % (
            LOOPED, med["loop"], min(t["loop"]), med["loop"] / LOOPED, scaled, scaled / med["full"]))
        del parent, unit, full, loop, runs
    report.close()


if __name__ == "__main__":
    main()
