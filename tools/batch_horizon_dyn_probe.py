"""The batch of horizons' compact dynamics sections (pmt_batch_horizon_dynamics_f64, pmt_batch_horizon_dynamics_expand_f64, batch.BatchMPC)
on one device, in one process, alternating with what they are compared with.
    (a) dyn      one call of pmt_batch_horizon_dynamics_f64 over B = 8192 instances at every (T, nx, nu) of SHAPES: time per call back to
                 back (HIP events around `calls` calls, median over `reps` windows) and cold (one call behind a 512 MiB write to another
                 buffer), and the fraction of 8 TB/s on the algorithmic bytes 16 Ld per instance; beside it, in the same windows,
        form     pmt_batch_form_coeffs_f64 at (n, m) = (128, 16) and
        lsq      pmt_batch_lsq_coeffs_f64 at BASELINE config 4, each on its own algorithmic bytes
    (b) mpc      batch.BatchMPC.compute() at (T, nx, nu) = (8, 16, 8) — the horizon's launch and the dynamics launch — against
        dense    the only route the batch had before: pmt_batch_horizon_coeffs_f64 with the same dynamics written out as a dense C_i of
                 m = T nx rows over all n = T (nx + nu) columns, and beside
        plain    the objective's launch alone (m = 0)
    (c) expand   one call of pmt_batch_horizon_dynamics_expand_f64 and the fraction of 8 TB/s on the bytes written (24 per term, 8 per
                 constant), beside pmt_batch_horizon_expand_f64 on a slab whose expansion is of similar size
Every timed window comes after at least 30 ms of warm-up work of the same call.
    python tools/batch_horizon_dyn_probe.py [--reps 15] [--calls 20] [--B 8192]                (GPU box)"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import parametron_jl_amd  # noqa: E402,F401
from parametron_jl_amd import _lib, batch  # noqa: E402
from batch_horizon_probe import DEV, PEAK, cold, form_bytes, lsq_bytes, ptr, warm, window  # noqa: E402

SHAPES = [(32, 32, 16), (16, 128, 32), (20, 12, 4), (8, 16, 8)]
DENSE = (8, 16, 8)
EXPAND = [((32, 32, 16), 32), ((16, 128, 32), 64)]          # (T, nx, nu), and the m that gives the sibling's expansion a similar size


def alternate(runs, reps):
    """medians and minima (us per call) of `reps` windows per run, the runs taking turns"""
    for run, calls in runs.values():
        warm(run, calls)
    t = {k: [] for k in runs}
    for _ in range(reps):
        for k, (run, calls) in runs.items():
            t[k].append(window(run, calls))
    torch.cuda.synchronize()
    return {k: (float(np.median(v)), min(v)) for k, v in t.items()}


def dense_rows(wl, mpc):
    """the dynamics of `mpc` (x_t - A x_{t-1} - B u_{t-1} - h_t, x_0 - h_0) as the dense block C_i z - d_i of the BatchHorizon `wl`"""
    B, T, nx, nu = mpc.B, mpc.T, mpc.nx, mpc.nu
    w, n, m = nx + nu, mpc.n, T * nx
    Ct = torch.zeros((B, n, m), dtype=torch.float64, device=DEV)           # C_i column-major: [column][row]
    At, Bt = mpc.A.view(B, nx, nx), mpc.Bm.view(B, nu, nx)
    k = torch.arange(nx, device=DEV)
    for t in range(T):
        Ct[:, t * w + k, t * nx + k] = 1.0
        if t:
            Ct[:, (t - 1) * w:(t - 1) * w + nx, t * nx:(t + 1) * nx] = -At
            Ct[:, (t - 1) * w + nx:t * w, t * nx:(t + 1) * nx] = -Bt
    wl.Cm.copy_(Ct.view(-1))
    wl.d.copy_(mpc.h)


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
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    print("(a) the coefficient launch alone")
    for T, nx, nu in SHAPES:
        Ld = batch.horizon_dynamics_layout(T, nx, nu)[1]
        A, Bm, h = (torch.rand(B * k, dtype=torch.float64, device=DEV) for k in (nx * nx, nx * nu, T * nx))
        out = torch.empty(B * Ld, dtype=torch.float64, device=DEV)

        def dyn():
            _lib.call("pmt_batch_horizon_dynamics_f64", ptr(A), ptr(Bm), ptr(h), B, T, nx, nu, -1, -1, -1, ptr(out), Ld, stream)
        med = alternate({"dyn": (dyn, a.calls), "form": (form.compute, a.calls), "lsq": (lsq.compute, a.calls)}, a.reps)
        tc = cold(dyn, flush, a.reps)
        db = 16.0 * Ld * B
        tag = "T = %3d nx = %3d nu = %2d " % (T, nx, nu)
        print(tag + "dyn     pmt_batch_horizon_dynamics_f64     median %8.1f us (min %8.1f)  %7.1f MB  %5.1f %% of 8 TB/s; cold median %8.1f us (min %8.1f)  %5.1f %%" % (
            med["dyn"][0], med["dyn"][1], db / 1e6, 100 * db / (med["dyn"][0] * 1e-6) / PEAK, float(np.median(tc)), min(tc),
            100 * db / (float(np.median(tc)) * 1e-6) / PEAK))
        print(tag + "form    pmt_batch_form_coeffs_f64 (128,16) median %8.1f us (min %8.1f)  %7.1f MB  %5.1f %% of 8 TB/s" % (
            med["form"][0], med["form"][1], form_b / 1e6, 100 * form_b / (med["form"][0] * 1e-6) / PEAK))
        print(tag + "lsq     pmt_batch_lsq_coeffs_f64 (C4)      median %8.1f us (min %8.1f)  %7.1f MB  %5.1f %% of 8 TB/s" % (
            med["lsq"][0], med["lsq"][1], lsq_b / 1e6, 100 * lsq_b / (med["lsq"][0] * 1e-6) / PEAK), flush=True)
        del A, Bm, h, out

    print("(b) BatchMPC.compute() against the dense constraint block")
    T, nx, nu = DENSE
    mpc = batch.BatchMPC(torch, B, T, nx, nu)
    wl = batch.BatchHorizon(torch, B, T, nx, nu, T * nx)
    dense_rows(wl, mpc)
    plain = batch.BatchHorizon(torch, B, T, nx, nu, 0)
    med = alternate({"mpc": (mpc.compute, a.calls), "dense": (wl.compute, a.calls), "plain": (plain.compute, a.calls)}, a.reps)
    tag = "T = %3d nx = %3d nu = %2d " % (T, nx, nu)
    cb_new, cb_old = 16.0 * mpc.Ld, 16.0 * (wl.m * wl.n + wl.m)
    print(tag + "plain   pmt_batch_horizon_coeffs_f64 m =   0 median %8.1f us (min %8.1f)  the objective's launch alone" % med["plain"])
    print(tag + "mpc     horizon (m = 0) + dynamics section  median %8.1f us (min %8.1f)  row of %d doubles, %.1f MB of rows" % (
        med["mpc"][0], med["mpc"][1], mpc.stride, 8.0 * mpc.stride * B / 1e6))
    print(tag + "dense   pmt_batch_horizon_coeffs_f64 m = %3d median %8.1f us (min %8.1f)  row of %d doubles, %.1f MB of rows = %5.1f x mpc's time; "
          "constraint bytes in and out per instance %.0f against %.0f = %.1f x" % (
              wl.m, med["dense"][0], med["dense"][1], wl.stride, 8.0 * wl.stride * B / 1e6, med["dense"][0] / med["mpc"][0], cb_old, cb_new, cb_old / cb_new))
    T, nx, nu = SHAPES[0]
    dense_gb = 8.0 * T * nx * T * (nx + nu) * B / 1e9
    print("        at (T, nx, nu) = (%d, %d, %d) the dense block is m n = %d doubles per instance: %.0f GB of C_i for %d instances and as much again in the "
          "slabs, %.0f of the device's %.0f GB for one batch (not attempted); the section is %d doubles, %.0f MB for the batch" % (
              T, nx, nu, T * nx * T * (nx + nu), dense_gb, B, 2 * dense_gb, torch.cuda.get_device_properties(0).total_memory / 1e9,
              batch.horizon_dynamics_layout(T, nx, nu)[1], 8.0 * batch.horizon_dynamics_layout(T, nx, nu)[1] * B / 1e6), flush=True)
    del mpc, wl, plain

    print("(c) the expansion of one instance")
    for (T, nx, nu), m in EXPAND:
        mpc = batch.BatchMPC(torch, 4, T, nx, nu)
        sib = batch.BatchHorizon(torch, 4, T, nx, nu, m)
        mpc.compute()
        sib.compute()
        n = mpc.n
        xvar = torch.arange(1, n + 1, dtype=torch.int64, device=DEV)
        varmap = torch.randperm(n, device=DEV) + 1
        nterms = nx + (T - 1) * nx * (1 + nx + nu)
        terms = torch.empty(3 * nterms, dtype=torch.int64, device=DEV)
        consts = torch.empty(T * nx, dtype=torch.float64, device=DEV)
        nq = T * (nx * (nx + 1) // 2 + nu * (nu + 1) // 2)
        quad, lin, cst = torch.empty(3 * nq, dtype=torch.int64, device=DEV), torch.empty(2 * n, dtype=torch.int64, device=DEV), torch.empty(1, dtype=torch.float64, device=DEV)
        vat, vc = torch.empty(3 * m * n, dtype=torch.int64, device=DEV), torch.empty(m, dtype=torch.float64, device=DEV)

        def expand():
            _lib.call("pmt_batch_horizon_dynamics_expand_f64", ptr(mpc.local, mpc.stride + mpc.L), T, nx, nu, 1, ptr(xvar), ptr(varmap), ptr(terms), ptr(consts), stream)

        def sibling():
            _lib.call("pmt_batch_horizon_expand_f64", ptr(sib.local, sib.stride), T, nx, nu, m, ptr(xvar), ptr(varmap), ptr(quad), ptr(lin), ptr(cst), ptr(vat),
                      ptr(vc), stream)
        med = alternate({"expand": (expand, a.calls), "sibling": (sibling, a.calls)}, a.reps)
        eb, sb = 24.0 * nterms + 8.0 * T * nx, 24.0 * nq + 16.0 * n + 8.0 + 24.0 * m * n + 8.0 * m
        tag = "T = %3d nx = %3d nu = %2d " % (T, nx, nu)
        print(tag + "expand  pmt_batch_horizon_dynamics_expand_f64   median %7.1f us (min %7.1f)  %7.2f MB written  %5.1f %% of 8 TB/s" % (
            med["expand"][0], med["expand"][1], eb / 1e6, 100 * eb / (med["expand"][0] * 1e-6) / PEAK))
        print(tag + "sibling pmt_batch_horizon_expand_f64 (m = %2d)   median %7.1f us (min %7.1f)  %7.2f MB written  %5.1f %% of 8 TB/s" % (
            m, med["sibling"][0], med["sibling"][1], sb / 1e6, 100 * sb / (med["sibling"][0] * 1e-6) / PEAK), flush=True)
        del mpc, sib


if __name__ == "__main__":
    main()
