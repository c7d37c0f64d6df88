"""The batch of horizons' time-varying dynamics sections (pmt_batch_horizon_dynamics_tv_f64, pmt_batch_horizon_dynamics_tv_expand_f64,
batch.BatchLTVMPC) on one device, in one process, alternating with what they are compared with.
    (a) ltv      one call of pmt_batch_horizon_dynamics_tv_f64 at every (T, nx, nu) of SHAPES over B = 8192 instances (LARGE_B at the shape
                 whose sections make 2.5 MB per instance): time per call back to back (HIP events around `calls` calls, median over `reps`
                 windows) and cold (one call behind a 512 MiB write to another buffer), and the fraction of 8 TB/s on the algorithmic
                 bytes 16 Ltv per instance; whether the launch's bytes exceed the 256 MiB Infinity Cache is printed with it.  Beside it, in
                 the same windows,
        dyn      pmt_batch_horizon_dynamics_f64 at the same (T, nx, nu) over 8192 instances — the yardstick: the same access pattern —,
        form     pmt_batch_form_coeffs_f64 at (n, m) = (128, 16) and
        lsq      pmt_batch_lsq_coeffs_f64 at BASELINE config 4, each on its own algorithmic bytes
    (b) thin     a thin fleet, B = 64 with T = 100 at (32, 16), beside the same number of matrix pairs as B = 792 with T = 9
    (c) mpc      batch.BatchLTVMPC.compute() at (T, nx, nu) = (8, 16, 8) — the horizon's launch and the dynamics launch — against
        dense    the only batched route there was: pmt_batch_horizon_coeffs_f64 with the same dynamics written out as a dense C_i of
                 m = T nx rows over all n = T (nx + nu) columns, beside
        plain    the objective's launch alone (m = 0), and
        looped   pmt_affine_stages_f64 once per instance on tables that point at the instance's own A_t, B_t, h: LOOPED instances
                 measured, scaled to B
    (d) expand   one call of pmt_batch_horizon_dynamics_tv_expand_f64 and the fraction of 8 TB/s on the bytes written (24 per term, 8 per
                 constant), beside pmt_batch_horizon_dynamics_expand_f64 at the same shape
Every timed window comes after at least 30 ms of warm-up work of the same call.
    python tools/batch_horizon_ltv_probe.py [--reps 15] [--calls 20] [--B 8192]                (GPU box)"""
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
from batch_horizon_dyn_probe import alternate  # noqa: E402

SHAPES = [(32, 32, 16), (16, 128, 32), (20, 12, 4), (8, 16, 8)]
LARGE_B = 4096                  # instances at (16, 128, 32): 2.47 MB of section each, 10 GB in and 10 GB out; 8192 would hold 40 GB
THIN = ((64, 100), (792, 9), (32, 16))
DENSE = (8, 16, 8)
EXPAND = [(32, 32, 16), (16, 128, 32)]
LOOPED = 64
L3 = 256 << 20


def ltv_doubles(T, nx, nu):
    return batch.horizon_dynamics_tv_layout(T, nx, nu)[1]


def ltv_inputs(B, T, nx, nu):
    return tuple(torch.rand(B * k, dtype=torch.float64, device=DEV) for k in ((T - 1) * nx * nx, (T - 1) * nx * nu, T * nx))


def ltv_call(A, Bm, h, B, T, nx, nu, out, stride, stream):
    def run():
        _lib.call("pmt_batch_horizon_dynamics_tv_f64", ptr(A), ptr(Bm), ptr(h), B, T, nx, nu, -1, -1, -1, ptr(out), stride, stream)
    return run


def dense_rows(wl, mpc):
    """the dynamics of `mpc` (x_t - A_t x_{t-1} - B_t u_{t-1} - h_t, x_0 - h_0) as the dense block C_i z - d_i of the BatchHorizon `wl`"""
    B, T, nx, nu = mpc.B, mpc.T, mpc.nx, mpc.nu
    w, n, m = nx + nu, mpc.n, T * nx
    Ct = torch.zeros((B, n, m), dtype=torch.float64, device=DEV)           # C_i column-major: [column][row]
    At, Bt = mpc.A.view(B, T - 1, nx, nx), mpc.Bm.view(B, T - 1, nu, nx)
    k = torch.arange(nx, device=DEV)
    for t in range(T):
        Ct[:, t * w + k, t * nx + k] = 1.0
        if t:
            Ct[:, (t - 1) * w:(t - 1) * w + nx, t * nx:(t + 1) * nx] = -At[:, t - 1]
            Ct[:, (t - 1) * w + nx:t * w, t * nx:(t + 1) * nx] = -Bt[:, t - 1]
    wl.Cm.copy_(Ct.view(-1))
    wl.d.copy_(mpc.h)


def looped_run(mpc, stream):
    """pmt_affine_stages_f64 over the first LOOPED instances of `mpc`, one call each, on device tables built once"""
    T, nx, nu, n = mpc.Td, mpc.nx, mpc.nu, mpc.n
    w, rl = nx + nu, 1 + nx + nu
    nterms = nx + (T - 1) * nx * rl
    x = torch.arange(1, n + 1, dtype=torch.int64, device=DEV)
    terms = torch.empty(LOOPED * 3 * nterms, dtype=torch.int64, device=DEV)
    consts = torch.empty(LOOPED * T * nx, dtype=torch.float64, device=DEV)
    tables = []
    for i in range(LOOPED):
        A_i, B_i, h_i = mpc.A.data_ptr() + 8 * i * (T - 1) * nx * nx, mpc.Bm.data_ptr() + 8 * i * (T - 1) * nx * nu, mpc.h.data_ptr() + 8 * i * T * nx
        parts, stages = [], []
        for t in range(T):
            first = len(parts)
            parts.append({"mat": None, "ld": 0, "xvar": x.data_ptr() + 8 * t * w, "cols": 1, "sign": 1})
            if t:
                parts.append({"mat": A_i + 8 * (t - 1) * nx * nx, "ld": nx, "xvar": x.data_ptr() + 8 * (t - 1) * w, "cols": nx, "sign": -1})
                parts.append({"mat": B_i + 8 * (t - 1) * nx * nu, "ld": nx, "xvar": x.data_ptr() + 8 * ((t - 1) * w + nx), "cols": nu, "sign": -1})
            stages.append({"vec": h_i + 8 * t * nx, "vec_sign": -1, "rows": nx, "first_part": first, "nparts": len(parts) - first,
                           "row_len": rl if t else 1, "term_offset": nx + (t - 1) * nx * rl if t else 0, "const_offset": t * nx})
        parr, sarr = _lib.affine_parts(parts), _lib.affine_stages(stages)
        _lib.call("pmt_affine_stages_check", C.addressof(sarr), T, C.addressof(parr), len(parts), nterms, T * nx)
        to = lambda arr: torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()).to(DEV)
        tables.append((to(sarr), to(parr)))

    def run():
        for i, (st, pt) in enumerate(tables):
            _lib.call("pmt_affine_stages_f64", ptr(st), T, ptr(pt), None, ptr(terms, i * 3 * nterms), ptr(consts, i * T * nx), stream)
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
    print("device %s, %d CUs; medians of %d windows of %d calls, alternating; fractions of %.0f TB/s on algorithmic bytes" % (
        torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count, a.reps, a.calls, PEAK / 1e12), flush=True)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    frac = lambda nbytes, us: 100 * nbytes / (us * 1e-6) / PEAK

    print("(a) the coefficient launch alone")
    for T, nx, nu in SHAPES:
        Ltv, Ld = ltv_doubles(T, nx, nu), batch.horizon_dynamics_layout(T, nx, nu)[1]
        Bt = min(B, LARGE_B) if 8 * Ltv > (2 << 20) else B
        A, Bm, h = ltv_inputs(Bt, T, nx, nu)
        out = torch.empty(Bt * Ltv, dtype=torch.float64, device=DEV)
        A1, B1, h1 = (torch.rand(B * k, dtype=torch.float64, device=DEV) for k in (nx * nx, nx * nu, T * nx))
        out1 = torch.empty(B * Ld, dtype=torch.float64, device=DEV)
        ltv = ltv_call(A, Bm, h, Bt, T, nx, nu, out, Ltv, stream)

        def dyn():
            _lib.call("pmt_batch_horizon_dynamics_f64", ptr(A1), ptr(B1), ptr(h1), B, T, nx, nu, -1, -1, -1, ptr(out1), Ld, stream)
        calls = max(2, min(a.calls, int(40e3 / (16.0 * Ltv * Bt / 4e12 * 1e6)) + 1))          # windows of about 40 ms at the large shapes
        med, win = {}, {}
        runs = {"ltv": (ltv, calls), "dyn": (dyn, a.calls), "form": (form.compute, a.calls), "lsq": (lsq.compute, a.calls)}
        for run, c in runs.values():
            warm(run, c)
        for _ in range(a.reps):
            for k, (run, c) in runs.items():
                win.setdefault(k, []).append(window(run, c))
        torch.cuda.synchronize()
        med = {k: (float(np.median(v)), min(v), max(v)) for k, v in win.items()}
        tc, tc1 = cold(ltv, flush, a.reps), cold(dyn, flush, a.reps)
        tb, db = 16.0 * Ltv * Bt, 16.0 * Ld * B
        tag = "T = %3d nx = %3d nu = %2d " % (T, nx, nu)
        print(tag + "ltv     pmt_batch_horizon_dynamics_tv_f64  B = %4d median %8.1f us (min %8.1f, max %8.1f)  %8.1f MB (%s)  %5.1f %% of 8 TB/s "
              "(windows %5.1f .. %5.1f %%); cold median %8.1f us (min %8.1f)  %5.1f %%" % (
                  Bt, med["ltv"][0], med["ltv"][1], med["ltv"][2], tb / 1e6, "beyond the Infinity Cache: an HBM figure" if tb > L3 else "within the Infinity Cache",
                  frac(tb, med["ltv"][0]), frac(tb, med["ltv"][2]), frac(tb, med["ltv"][1]), float(np.median(tc)), min(tc), frac(tb, float(np.median(tc)))))
        print(tag + "dyn     pmt_batch_horizon_dynamics_f64     B = %4d median %8.1f us (min %8.1f, max %8.1f)  %8.1f MB (%s)  %5.1f %% of 8 TB/s "
              "(windows %5.1f .. %5.1f %%); cold median %8.1f us (min %8.1f)  %5.1f %%" % (
                  B, med["dyn"][0], med["dyn"][1], med["dyn"][2], db / 1e6, "beyond the Infinity Cache" if db > L3 else "within the Infinity Cache",
                  frac(db, med["dyn"][0]), frac(db, med["dyn"][2]), frac(db, med["dyn"][1]), float(np.median(tc1)), min(tc1), frac(db, float(np.median(tc1)))))
        print(tag + "form    pmt_batch_form_coeffs_f64 (128,16) B = %4d median %8.1f us (min %8.1f)  %8.1f MB  %5.1f %% of 8 TB/s" % (
            B, med["form"][0], med["form"][1], form_b / 1e6, frac(form_b, med["form"][0])))
        print(tag + "lsq     pmt_batch_lsq_coeffs_f64 (C4)      B = %4d median %8.1f us (min %8.1f)  %8.1f MB  %5.1f %% of 8 TB/s" % (
            B, med["lsq"][0], med["lsq"][1], lsq_b / 1e6, frac(lsq_b, med["lsq"][0])), flush=True)
        del A, Bm, h, out, A1, B1, h1, out1

    print("(b) a thin fleet: the item is the matrix pair")
    (Bthin, Tthin), (Bfat, Tfat), (nx, nu) = THIN
    assert Bthin * (Tthin - 1) == Bfat * (Tfat - 1)
    runs, nbytes = {}, {}
    keep = []
    for name, Bq, Tq in (("thin", Bthin, Tthin), ("fat", Bfat, Tfat)):
        Ltv = ltv_doubles(Tq, nx, nu)
        A, Bm, h = ltv_inputs(Bq, Tq, nx, nu)
        out = torch.empty(Bq * Ltv, dtype=torch.float64, device=DEV)
        keep.append((A, Bm, h, out))
        runs[name], nbytes[name] = (ltv_call(A, Bm, h, Bq, Tq, nx, nu, out, Ltv, stream), a.calls), 16.0 * Ltv * Bq
    med = alternate(runs, a.reps)
    for name, Bq, Tq in (("thin", Bthin, Tthin), ("fat", Bfat, Tfat)):
        print("nx = %3d nu = %2d  %-4s  B = %4d T = %3d (%d matrix pairs)  median %7.1f us (min %7.1f)  %6.1f MB  %5.1f %% of 8 TB/s" % (
            nx, nu, name, Bq, Tq, Bq * (Tq - 1), med[name][0], med[name][1], nbytes[name] / 1e6, frac(nbytes[name], med[name][0])), flush=True)
    del keep, runs

    print("(c) BatchLTVMPC.compute() against the dense constraint block and the host loop")
    T, nx, nu = DENSE
    mpc = batch.BatchLTVMPC(torch, B, T, nx, nu)
    wl = batch.BatchHorizon(torch, B, T, nx, nu, T * nx)
    dense_rows(wl, mpc)
    plain = batch.BatchHorizon(torch, B, T, nx, nu, 0)
    med = alternate({"mpc": (mpc.compute, a.calls), "dense": (wl.compute, a.calls), "plain": (plain.compute, a.calls), "looped": (looped_run(mpc, stream), 2)}, a.reps)
    tag = "T = %3d nx = %3d nu = %2d " % (T, nx, nu)
    cb_new, cb_old = 16.0 * mpc.Ltv, 16.0 * (wl.m * wl.n + wl.m)
    print(tag + "plain   pmt_batch_horizon_coeffs_f64 m =   0 median %8.1f us (min %8.1f)  the objective's launch alone" % med["plain"])
    print(tag + "mpc     horizon (m = 0) + LTV section       median %8.1f us (min %8.1f)  row of %d doubles, %.1f MB of rows" % (
        med["mpc"][0], med["mpc"][1], mpc.stride, 8.0 * mpc.stride * B / 1e6))
    print(tag + "dense   pmt_batch_horizon_coeffs_f64 m = %3d median %8.1f us (min %8.1f)  row of %d doubles, %.1f MB of rows = %5.1f x mpc's time; "
          "constraint bytes in and out per instance %.0f against %.0f = %.1f x" % (
              wl.m, med["dense"][0], med["dense"][1], wl.stride, 8.0 * wl.stride * B / 1e6, med["dense"][0] / med["mpc"][0], cb_old, cb_new, cb_old / cb_new))
    print(tag + "looped  pmt_affine_stages_f64 x %d instances  median %8.1f us (min %8.1f) = %.1f us per instance, %.0f us scaled to %d: %.0f x the LTV launch "
          "alone (mpc - plain = %.1f us)" % (LOOPED, med["looped"][0], med["looped"][1], med["looped"][0] / LOOPED, med["looped"][0] / LOOPED * B, B,
                                           med["looped"][0] / LOOPED * B / max(med["mpc"][0] - med["plain"][0], 1e-3), med["mpc"][0] - med["plain"][0]), flush=True)
    del mpc, wl, plain

    print("(d) the expansion of one instance")
    for T, nx, nu in EXPAND:
        mpc = batch.BatchLTVMPC(torch, 4, T, nx, nu)
        sib = batch.BatchMPC(torch, 4, T, nx, nu)
        mpc.compute()
        sib.compute()
        n = mpc.n
        xvar = torch.arange(1, n + 1, dtype=torch.int64, device=DEV)
        varmap = torch.randperm(n, device=DEV) + 1
        nterms = nx + (T - 1) * nx * (1 + nx + nu)
        terms, terms1 = (torch.empty(3 * nterms, dtype=torch.int64, device=DEV) for _ in range(2))
        consts, consts1 = (torch.empty(T * nx, dtype=torch.float64, device=DEV) for _ in range(2))

        def expand():
            _lib.call("pmt_batch_horizon_dynamics_tv_expand_f64", ptr(mpc.local, mpc.stride + mpc.L), T, nx, nu, 1, ptr(xvar), ptr(varmap), ptr(terms), ptr(consts), stream)

        def sibling():
            _lib.call("pmt_batch_horizon_dynamics_expand_f64", ptr(sib.local, sib.stride + sib.L), T, nx, nu, 1, ptr(xvar), ptr(varmap), ptr(terms1), ptr(consts1), stream)
        med = alternate({"expand": (expand, a.calls), "sibling": (sibling, a.calls)}, a.reps)
        eb = 24.0 * nterms + 8.0 * T * nx
        tag = "T = %3d nx = %3d nu = %2d " % (T, nx, nu)
        print(tag + "expand  pmt_batch_horizon_dynamics_tv_expand_f64 median %7.1f us (min %7.1f)  %7.2f MB written  %5.1f %% of 8 TB/s" % (
            med["expand"][0], med["expand"][1], eb / 1e6, frac(eb, med["expand"][0])))
        print(tag + "sibling pmt_batch_horizon_dynamics_expand_f64    median %7.1f us (min %7.1f)  %7.2f MB written  %5.1f %% of 8 TB/s" % (
            med["sibling"][0], med["sibling"][1], eb / 1e6, frac(eb, med["sibling"][0])), flush=True)
        del mpc, sib


if __name__ == "__main__":
    main()
