"""transpose(x) * Q * x as a canonical objective: the symmetrising node (pmt_quad_form_f64) against the generic path (bilinearmul! +
the canonicalize! node + the MOI pack), on one device, in one process, alternating.  For n = 512, 1024, 2048, 4096 (Q at the padded pitch):
    node     pmt_quad_form_f64 stand-alone by HIP events: back to back, and cold (behind a 1 GiB fill that empties L2 and the Infinity Cache);
             its bytes 8 n^2 + 24 n(n+1)/2 over time as a fraction of 8 TB/s
    update!  device time per update! of the objective's kernels, by the library's profiler (HIP events around every launch), two models
             alternating: `form` (mode "canonical-form": quad_form_kernel) and `generic` — the same objective wrapped in .canonicalize(), the
             path every such objective took before the node existed (bilinear_kernel + segment_sum_kernel + the pack kernels)
Q is regenerated on the device at every update (DeviceUniformParameter); its fill kernel is listed but not counted.  Kernel times and
counters: run this under `rocprofv3 --kernel-trace --stats -- python tools/quad_form_probe.py --sizes 4096 --reps 10`.
    python tools/quad_form_probe.py [--reps 30] [--sizes 512,1024,2048,4096]                (GPU box)"""
import argparse
import ctypes as C
import os
import sys

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


def node(n, reps, flush):
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ldq = padded_lda(n)
    Q = torch.zeros(ldq * n, dtype=torch.float64, device=DEV)
    _lib.call("pmt_fill_uniform_matrix_f64", ptr(Q), n, n, ldq, C.c_uint64(7), 1.0, s)
    x = torch.arange(1, n + 1, dtype=torch.int64, device=DEV)
    nq = n * (n + 1) // 2
    q = torch.empty(3 * nq, dtype=torch.int64, device=DEV)

    def run():
        _lib.call("pmt_quad_form_f64", ptr(Q), ldq, n, ptr(x), 1, ptr(x), 1.0, ptr(q), None, None, None, s)

    def timed():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) * 1e3
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    warm, cold = [], []
    for _ in range(reps):                                  # alternating
        warm.append(timed())
        flush.fill_(1.0)
        torch.cuda.synchronize()
        cold.append(timed())
    nbytes = 8 * n * n + 24 * nq
    for name, t in (("back to back", warm), ("cold", cold)):
        med = float(np.median(t))
        print("n = %4d  node %-12s median %7.1f us  min %7.1f  %6.1f MB  %.2f of 8 TB/s" % (n, name, med, min(t), nbytes / 1e6, nbytes / (med * 1e-6) / HBM),
              flush=True)


def model(n, generic):
    m = P.Model(P.MockOptimizer(), quadratic_mode="canonical")
    x = [P.Variable(m) for _ in range(n)]
    Q = P.DeviceUniformParameter((n, n), 1, m)
    expr = P.transpose(x) * Q * x
    P.objective(m, P.Minimize, expr.canonicalize() if generic else expr)
    m.initialize()
    return m


def kernel_totals():
    """{kernel: (launches, total ms)} of the profiler's report"""
    return {k: (v["launches"], v["avg_ms"] * v["launches"]) for k, v in P.profile_report().items()}


def updates(n, reps):
    ms = {"form": model(n, False), "generic": model(n, True)}
    assert ms["form"].objective.mode == "canonical-form" and ms["generic"].objective.mode == "literal"
    for m in ms.values():
        for _ in range(2):
            m.update()
    acc = {k: {} for k in ms}
    for _ in range(reps):                                  # alternating, one update! per profiler window
        for k, m in ms.items():
            P.profile_enable(True)
            before = kernel_totals()
            m.update()
            torch.cuda.synchronize()
            after = kernel_totals()
            P.profile_enable(False)
            for name, (cnt, tot) in after.items():
                c0, t0 = before.get(name, (0, 0.0))
                if cnt > c0:
                    acc[k].setdefault(name, []).append((tot - t0) * 1e3)
    total = {}
    for k in ms:
        total[k] = 0.0
        for name, t in sorted(acc[k].items()):
            counted = "fill" not in name
            med = float(np.median(t))
            total[k] += med if counted else 0.0
            print("n = %4d  update! %-8s %-36s median %8.1f us  min %8.1f  (%d updates)%s" % (
                n, k, name, med, min(t), len(t), "" if counted else "  [not counted]"))
    print("n = %4d  update! device time of the objective: form %8.1f us  generic %8.1f us  generic / form = %.2f" % (
        n, total["form"], total["generic"], total["generic"] / total["form"]), flush=True)
    for m in ms.values():
        m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sizes", default="512,1024,2048,4096")
    a = ap.parse_args()
    _lib.require_gpu()
    flush = torch.empty(1 << 27, dtype=torch.float64, device=DEV)        # 1 GiB
    for n in [int(v) for v in a.sizes.split(",")]:
        node(n, a.reps, flush)
        updates(n, a.reps)


if __name__ == "__main__":
    main()
