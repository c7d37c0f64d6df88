"""The batch of horizons with time-varying stage weights (pmt_batch_horizon_tv_coeffs_f64, pmt_batch_horizon_tv_expand_f64,
batch.BatchTVHorizon) on one device, in one process, alternating with what it is compared with.
    (a) tv       one call of pmt_batch_horizon_tv_coeffs_f64 (x_t - r_t, u_t - v_t, m = 0, no terminal stage) at every (T, nx, nu) of SHAPES
                 over B instances: time per call back to back (HIP events around `calls` calls, median over `reps` windows) and cold (one
                 call behind a 512 MiB write to another buffer), and the fraction of 8 TB/s on the algorithmic bytes — the inputs read plus
                 8 L written.  Beside it, in the same windows,
        pair     the nearest route there was: two calls of pmt_batch_form_coeffs_f64 over the same stages as instances, B*T of n = nx and
                 B*T of n = nu, m = 0, on the same device data.  The same algorithmic bytes less the instance constants; no row per
                 instance, no instance constant, no expansion.  Its windows' spread is what the comparison is read against.
        hor      the time-invariant pmt_batch_horizon_coeffs_f64 at the same shape: other bytes (one Q_i, R_i per instance), a reference
        form     pmt_batch_form_coeffs_f64 at (n, m) = (128, 16) and
        lsq      pmt_batch_lsq_coeffs_f64 at BASELINE config 4, each on its own algorithmic bytes
    (b) thin     a thin fleet, B = 64 with T = 100 at (32, 16), beside the same number of stages as B = 800 with T = 8
    (c) looped   the host loop: pmt_quad_stages_check + pmt_quad_stages_f64 once per instance on a table that points at the instance's own
                 Q_t, R_t and references: LOOPED instances measured, scaled to B
    (d) expand   one call of pmt_batch_horizon_tv_expand_f64 and the fraction of 8 TB/s on the bytes written (24 per quadratic, 16 per linear
                 term), beside pmt_batch_horizon_expand_f64 at the same shape
Every timed window comes after at least 30 ms of warm-up work of the same call.
    python tools/batch_horizon_tv_probe.py [--reps 15] [--calls 20] [--B 8192]                (GPU box)"""
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
from batch_horizon_probe import DEV, PEAK, cold, form_bytes, horizon_bytes, lsq_bytes, ptr, warm, window  # noqa: E402
from batch_horizon_dyn_probe import alternate  # noqa: E402

SHAPES = [(32, 32, 16), (16, 128, 32), (20, 12, 4), (8, 16, 8)]
THIN = ((64, 100), (800, 8), (32, 16))
EXPAND = [(32, 32, 16), (16, 128, 32)]
LOOPED = 64
L3 = 256 << 20


def tv_bytes(T, nx, nu):
    """algorithmic bytes per instance (m = 0, no terminal stage): the matrices and references read, the slab written"""
    return 8.0 * T * (nx * nx + nx + nu * nu + nu) + 8.0 * batch.horizon_tv_slab_layout(T, nx, nu, 0, False)[1]


def pair_bytes(T, nx, nu):
    """... of the two calls over the stages as instances: the same inputs, [Q | q | const] per stage written"""
    return 8.0 * T * (nx * nx + nx + nu * nu + nu) + 8.0 * T * (batch.slab_layout(nx, 0)[1] + batch.slab_layout(nu, 0)[1])


def tv_call(wl, stream):
    def run():
        _lib.call("pmt_batch_horizon_tv_coeffs_f64", ptr(wl.Q), ptr(wl.R), ptr(wl.r), ptr(wl.v), None, None, wl.B, wl.T, wl.nx, wl.nu, 0, 0, -1, -1, 0,
                  ptr(wl.local), wl.stride, stream)
    return run


def pair_call(wl, stream):
    """pmt_batch_form_coeffs_f64 twice on the inputs of `wl`: B*T instances of n = nx, then B*T of n = nu"""
    items = wl.B * wl.T
    Lx, Lu = batch.slab_layout(wl.nx, 0)[1], batch.slab_layout(wl.nu, 0)[1]
    ox, ou = torch.empty(items * Lx, dtype=torch.float64, device=DEV), torch.empty(items * Lu, dtype=torch.float64, device=DEV)

    def run():
        _lib.call("pmt_batch_form_coeffs_f64", ptr(wl.Q), ptr(wl.r), None, None, items, wl.nx, 0, -1, 0, ptr(ox), Lx, stream)
        _lib.call("pmt_batch_form_coeffs_f64", ptr(wl.R), ptr(wl.v), None, None, items, wl.nu, 0, -1, 0, ptr(ou), Lu, stream)
    run.keep = (ox, ou)
    return run


def looped_run(wl, stream):
    """pmt_quad_stages_check + pmt_quad_stages_f64 over the first LOOPED instances of the batch, one after the other: the instance's table
    [x_0, u_0, x_1, ..] with stage s's Q at its own matrix"""
    T, nx, nu, n = wl.T, wl.nx, wl.nu, wl.n
    nterms = T * (nx * (nx + 1) // 2 + nu * (nu + 1) // 2)
    nst = T * (2 if nu else 1)
    x = torch.arange(1, n + 1, dtype=torch.int64, device=DEV)
    quad = torch.empty(LOOPED * 3 * nterms, dtype=torch.int64, device=DEV)
    lin = torch.empty(LOOPED * 2 * n, dtype=torch.int64, device=DEV)
    consts = torch.empty(LOOPED * nst, dtype=torch.float64, device=DEV)
    cst = torch.empty(LOOPED, dtype=torch.float64, device=DEV)
    hosts, tables = [], []
    for i in range(LOOPED):
        rows, qa, la = [], 0, 0
        for t in range(T):
            for M, ref, nd in ((wl.Q, wl.r, nx), (wl.R, wl.v, nu)):
                if nd:
                    rows.append({"Q": M.data_ptr() + 8 * (i * T + t) * nd * nd, "ldq": nd, "xvar": x.data_ptr() + 8 * la,
                                 "vec": ref.data_ptr() + 8 * (i * T + t) * nd, "n": nd, "sign": -1, "quad_at": qa, "lin_at": la})
                    qa, la = qa + nd * (nd + 1) // 2, la + nd
        arr = _lib.quad_stages(rows)
        hosts.append(arr)
        tables.append(torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()).to(DEV))

    def run():
        for i in range(LOOPED):
            _lib.call("pmt_quad_stages_check", C.addressof(hosts[i]), nst, nterms, n)
            _lib.call("pmt_quad_stages_f64", ptr(tables[i]), nst, ptr(x), ptr(quad, i * 3 * nterms), ptr(lin, i * 2 * n), ptr(consts, i * nst),
                      ptr(cst, i), stream)
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
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    frac = lambda nbytes, us: 100 * nbytes / (us * 1e-6) / PEAK

    print("(a) the coefficient call against the stages as instances of pmt_batch_form_coeffs_f64")
    for T, nx, nu in SHAPES:
        wl = batch.BatchTVHorizon(torch, B, T, nx, nu, 0)
        hor = batch.BatchHorizon(torch, B, T, nx, nu, 0)
        tb, pb, hb = tv_bytes(T, nx, nu) * B, pair_bytes(T, nx, nu) * B, horizon_bytes(T, nx, nu, 0) * B
        tv, pair = tv_call(wl, stream), pair_call(wl, stream)
        calls = max(2, min(a.calls, int(40e3 / (tb / 4e12 * 1e6)) + 1))            # windows of about 40 ms at the large shapes
        runs = {"tv": (tv, calls), "pair": (pair, calls), "hor": (hor.compute, a.calls), "form": (form.compute, a.calls), "lsq": (lsq.compute, a.calls)}
        win = {}
        for run, c in runs.values():
            warm(run, c)
        for _ in range(a.reps):
            for k, (run, c) in runs.items():
                win.setdefault(k, []).append(window(run, c))
        torch.cuda.synchronize()
        med = {k: (float(np.median(v)), min(v), max(v)) for k, v in win.items()}
        tc, pc = cold(tv, flush, a.reps), cold(pair, flush, a.reps)
        tag = "T = %3d nx = %3d nu = %2d " % (T, nx, nu)
        where = lambda nb: "beyond the Infinity Cache: an HBM figure" if nb > L3 else "within the Infinity Cache"
        print(tag + "tv      pmt_batch_horizon_tv_coeffs_f64     median %8.1f us (min %8.1f, max %8.1f)  %8.1f MB (%s)  %5.1f %% of 8 TB/s "
              "(windows %5.1f .. %5.1f %%); cold median %8.1f us (min %8.1f)  %5.1f %%" % (
                  med["tv"][0], med["tv"][1], med["tv"][2], tb / 1e6, where(tb), frac(tb, med["tv"][0]), frac(tb, med["tv"][2]), frac(tb, med["tv"][1]),
                  float(np.median(tc)), min(tc), frac(tb, float(np.median(tc)))))
        print(tag + "pair    2 x pmt_batch_form_coeffs_f64       median %8.1f us (min %8.1f, max %8.1f)  %8.1f MB  %5.1f %% of 8 TB/s "
              "(windows %5.1f .. %5.1f %%); cold median %8.1f us (min %8.1f)  %5.1f %%" % (
                  med["pair"][0], med["pair"][1], med["pair"][2], pb / 1e6, frac(pb, med["pair"][0]), frac(pb, med["pair"][2]), frac(pb, med["pair"][1]),
                  float(np.median(pc)), min(pc), frac(pb, float(np.median(pc)))))
        spread = med["pair"][2] - med["pair"][1]
        print(tag + "        tv / pair = %.3f (medians); tv - pair = %+.1f us against the pair's own spread of %.1f us over its %d windows: %s" % (
            med["tv"][0] / med["pair"][0], med["tv"][0] - med["pair"][0], spread, a.reps,
            "not slower" if med["tv"][0] <= med["pair"][0] + spread else "SLOWER beyond the spread"))
        print(tag + "hor     pmt_batch_horizon_coeffs_f64        median %8.1f us (min %8.1f)  %8.1f MB  %5.1f %% of 8 TB/s (one Q_i, R_i per instance: other bytes)" % (
            med["hor"][0], med["hor"][1], hb / 1e6, frac(hb, med["hor"][0])))
        print(tag + "form    pmt_batch_form_coeffs_f64 (128,16)  median %8.1f us (min %8.1f)  %8.1f MB  %5.1f %% of 8 TB/s" % (
            med["form"][0], med["form"][1], form_b / 1e6, frac(form_b, med["form"][0])))
        print(tag + "lsq     pmt_batch_lsq_coeffs_f64 (C4)       median %8.1f us (min %8.1f)  %8.1f MB  %5.1f %% of 8 TB/s" % (
            med["lsq"][0], med["lsq"][1], lsq_b / 1e6, frac(lsq_b, med["lsq"][0])), flush=True)
        # (c) at the same shape, on the same inputs
        loop = looped_run(wl, stream)
        lm = alternate({"looped": (loop, 2), "tv": (tv, calls)}, max(3, a.reps // 3))
        print(tag + "looped  pmt_quad_stages_check + _f64 x %d    median %8.1f us (min %8.1f) = %.1f us per instance, %.0f us scaled to %d: %.0f x the call" % (
            LOOPED, lm["looped"][0], lm["looped"][1], lm["looped"][0] / LOOPED, lm["looped"][0] / LOOPED * B, B, lm["looped"][0] / LOOPED * B / lm["tv"][0]),
            flush=True)
        del wl, hor, tv, pair, loop, runs

    print("(b) a thin fleet: the item is the stage")
    (Bthin, Tthin), (Bfat, Tfat), (nx, nu) = THIN
    assert Bthin * Tthin == Bfat * Tfat
    runs, nbytes, keep = {}, {}, []
    for name, Bq, Tq in (("thin", Bthin, Tthin), ("fat", Bfat, Tfat)):
        wl = batch.BatchTVHorizon(torch, Bq, Tq, nx, nu, 0)
        keep.append(wl)
        runs[name], nbytes[name] = (tv_call(wl, stream), a.calls), tv_bytes(Tq, nx, nu) * Bq
    med = alternate(runs, a.reps)
    for name, Bq, Tq in (("thin", Bthin, Tthin), ("fat", Bfat, Tfat)):
        print("nx = %3d nu = %2d  %-4s  B = %4d T = %3d (%d stage pairs)  median %7.1f us (min %7.1f)  %6.1f MB  %5.1f %% of 8 TB/s" % (
            nx, nu, name, Bq, Tq, Bq * Tq, med[name][0], med[name][1], nbytes[name] / 1e6, frac(nbytes[name], med[name][0])), flush=True)
    del keep, runs

    print("(d) the expansion of one instance")
    for T, nx, nu in EXPAND:
        wl, sib = batch.BatchTVHorizon(torch, 4, T, nx, nu, 0), batch.BatchHorizon(torch, 4, T, nx, nu, 0)
        wl.compute()
        sib.compute()
        n = wl.n
        xvar = torch.arange(1, n + 1, dtype=torch.int64, device=DEV)
        varmap = torch.randperm(n, device=DEV) + 1
        med = alternate({"expand": (lambda: wl.expand(1, xvar, varmap), a.calls), "sibling": (lambda: sib.expand(1, xvar, varmap), a.calls)}, a.reps)
        eb = 24.0 * T * (nx * (nx + 1) // 2 + nu * (nu + 1) // 2) + 16.0 * n
        tag = "T = %3d nx = %3d nu = %2d " % (T, nx, nu)
        print(tag + "expand  BatchTVHorizon.expand (pmt_batch_horizon_tv_expand_f64) median %7.1f us (min %7.1f)  %7.2f MB written  %5.1f %% of 8 TB/s" % (
            med["expand"][0], med["expand"][1], eb / 1e6, frac(eb, med["expand"][0])))
        print(tag + "sibling BatchHorizon.expand (pmt_batch_horizon_expand_f64)      median %7.1f us (min %7.1f)  %7.2f MB written  %5.1f %% of 8 TB/s" % (
            med["sibling"][0], med["sibling"][1], eb / 1e6, frac(eb, med["sibling"][0])), flush=True)
        del wl, sib


if __name__ == "__main__":
    main()
