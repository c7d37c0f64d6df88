"""A residual over two Variable vectors (r = A*x + B*u - b, stacked into one Gram by pmt_affine_stack_columns_f64) against the same model
written with one Parameter holding [A B] over z = [x; u] (config 2's work exactly), in one process, alternating:
    stacked     update! of the model with r = A*x + B*u - b at 4096 x (2048 + 2048) and a 512-row constraint C*z == d
    prestacked  update! of the model with r = AB*z - b and the same constraint
    stack       pmt_affine_stack_columns_f64 alone at 4096 x 4096 (padded layout), its 16*rows*cols bytes over time as a fraction of 8 TB/s
Every Parameter is regenerated on the device at every update (DeviceUniformParameter).  Update times are host wall clock of update!, which
ends with the replay (median of --reps); the node by HIP events.  Kernel times: run this under
`rocprofv3 --kernel-trace --stats -- python tools/stacked_lsq_probe.py`.
    python tools/stacked_lsq_probe.py [--reps 50]                (GPU box)"""
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
from parametron_jl_amd import _lib  # noqa: E402
from parametron_jl_amd.device import padded_lda  # noqa: E402

DEV = "cuda:0"
HBM = 8e12


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def model(stacked, rows=4096, nx=2048, nu=2048, crows=512):
    m = P.Model(P.MockOptimizer(), quadratic_mode="canonical")
    z = [P.Variable(m) for _ in range(nx + nu)]
    b = P.DeviceUniformParameter((rows,), 3, m)
    if stacked:
        A = P.DeviceUniformParameter((rows, nx), 1, m)
        B = P.DeviceUniformParameter((rows, nu), 2, m)
        r = A * z[:nx] + B * z[nx:] - b
    else:
        AB = P.DeviceUniformParameter((rows, nx + nu), 1, m)
        r = AB * z - b
    Cm = P.DeviceUniformParameter((crows, nx + nu), 4, m)
    d = P.DeviceUniformParameter((crows,), 5, m)
    P.objective(m, P.Minimize, P.dot(r, r))
    P.constraint(m, Cm * z == d)
    m.initialize()
    return m


def stack_node(reps, rows=4096, ncols=4096):
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lda = padded_lda(rows)
    src = torch.zeros(lda * ncols, dtype=torch.float64, device=DEV)
    _lib.call("pmt_fill_uniform_matrix_f64", ptr(src), rows, ncols, lda, 7, 1.0, s)
    out = torch.zeros(lda * ncols, dtype=torch.float64, device=DEV)
    half = ncols // 2
    addrs = [src.data_ptr() + 8 * lda * j for j in range(ncols)]
    signs = [1] * half + [-1] * (ncols - half)
    table = torch.from_numpy(_lib.stack_table(addrs, signs).view(np.int64).copy()).to(DEV)

    def run():
        _lib.call("pmt_affine_stack_columns_f64", ptr(table), ncols, rows, ptr(out), lda, s)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(); e1.record(); e1.synchronize()
        t.append(e0.elapsed_time(e1) * 1e3)
    med = float(np.median(t))
    nbytes = 16 * rows * ncols
    print("stack node %dx%d (lda %d)   median %7.1f us  min %7.1f us  %6.1f MB  %.2f of 8 TB/s" % (
        rows, ncols, lda, med, min(t), nbytes / 1e6, nbytes / (med * 1e-6) / HBM))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    _lib.require_gpu()
    ms = {"stacked": model(True), "prestacked": model(False)}
    assert ms["stacked"].objective.mode == ms["prestacked"].objective.mode == "canonical"
    for m in ms.values():
        for _ in range(3):
            m.update()
    t = {k: [] for k in ms}
    for _ in range(a.reps):                                # alternating
        for k, m in ms.items():
            t0 = time.perf_counter()
            m.update()
            t[k].append((time.perf_counter() - t0) * 1e6)
    med = {k: float(np.median(v)) for k, v in t.items()}
    for k in ms:
        print("%-10s update! %8.1f us  (min %8.1f, p90 %8.1f)" % (k, med[k], min(t[k]), float(np.percentile(t[k], 90))))
    print("stacked - prestacked: %+.1f us (medians)" % (med["stacked"] - med["prestacked"]))
    for m in ms.values():
        m.close()
    stack_node(a.reps)


if __name__ == "__main__":
    main()
