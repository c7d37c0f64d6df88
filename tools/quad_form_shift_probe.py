"""transpose(x - p) * Q * (x - p) as a canonical objective: the shifted form node (pmt_quad_form_shift_f64) against its yardsticks, on one
device, in one process, alternating.  For n = 1024, 2048, 4096 (Q at the padded pitch):
    node     pmt_quad_form_shift_f64 (terms, linear terms, constant) and pmt_quad_form_f64 (terms, zero linear terms, constant) on the same Q,
             stand-alone by HIP events, back to back and cold (behind a 1 GiB fill that empties L2 and the Infinity Cache); the ratio
    update!  device time per update! of the objective's kernels, by the library's profiler (HIP events around every launch):
             `bare`     transpose(x - p)*Q*(x - p)                      mode "canonical-form"
             `lqr`      ... + transpose(u)*R*u, u of n/2 Variables      mode "canonical-groups"
             `literal`  dot(e, Q*e), e = x - p, at n = 1024 only (the largest of the three whose literal buffers are modest): the path the
                        tracking cost took before the node existed — vars_addsub, matvecmul_affs, quad_expand, the segment sums, the packs
Q, R and p are regenerated on the device at every update (DeviceUniformParameter); their fill kernels are listed but not counted.
    python tools/quad_form_shift_probe.py [--reps 20] [--sizes 1024,2048,4096] [--literal 1024]                (GPU box)"""
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


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def node(n, reps, flush):
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ldq = padded_lda(n)
    Q = torch.zeros(ldq * n, dtype=torch.float64, device=DEV)
    _lib.call("pmt_fill_uniform_matrix_f64", ptr(Q), n, n, ldq, C.c_uint64(7), 1.0, s)
    v = torch.rand(n, dtype=torch.float64, device=DEV)
    x = torch.arange(1, n + 1, dtype=torch.int64, device=DEV)
    nq = n * (n + 1) // 2
    q = torch.empty(3 * nq, dtype=torch.int64, device=DEV)
    lin = torch.empty(2 * n, dtype=torch.int64, device=DEV)
    cst = torch.empty(1, dtype=torch.float64, device=DEV)
    ws = torch.empty(int(_lib.load().pmt_quad_form_shift_workspace_bytes(n)) // 8, dtype=torch.float64, device=DEV)
    runs = {"shift": lambda: _lib.call("pmt_quad_form_shift_f64", ptr(Q), ldq, n, ptr(x), ptr(v), -1, 1, ptr(x), 1.0, ptr(q), None, ptr(lin), ptr(cst),
                                       ptr(ws), s),
            "plain": lambda: _lib.call("pmt_quad_form_f64", ptr(Q), ldq, n, ptr(x), 1, ptr(x), 1.0, ptr(q), None, ptr(lin), ptr(cst), s)}

    def timed(run):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) * 1e3
    for run in runs.values():
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    t = {(k, c): [] for k in runs for c in ("back to back", "cold")}
    for _ in range(reps):                                  # alternating
        for k, run in runs.items():
            t[k, "back to back"].append(timed(run))
            flush.fill_(1.0)
            torch.cuda.synchronize()
            t[k, "cold"].append(timed(run))
    for c in ("back to back", "cold"):
        med = {k: float(np.median(t[k, c])) for k in runs}
        print("n = %4d  node %-12s shift median %7.1f us (min %7.1f)  plain median %7.1f us (min %7.1f)  shift / plain = %.3f  (workspace %.2f MB)" % (
            n, c, med["shift"], min(t["shift", c]), med["plain"], min(t["plain", c]), med["shift"] / med["plain"], 8 * ws.numel() / 1e6), flush=True)


def model(n, kind):
    m = P.Model(P.MockOptimizer(), quadratic_mode="canonical")
    x = [P.Variable(m) for _ in range(n)]
    Q = P.DeviceUniformParameter((n, n), 1, m)
    p = P.DeviceUniformParameter((n,), 2, m)
    e = x - p
    if kind == "literal":
        expr = P.dot(e, Q * e)
    else:
        expr = P.transpose(e) * Q * e
        if kind == "lqr":
            u = [P.Variable(m) for _ in range(n // 2)]
            R = P.DeviceUniformParameter((n // 2, n // 2), 3, m)
            expr = expr + P.transpose(u) * R * u
    P.objective(m, P.Minimize, expr)
    m.initialize()
    return m


def kernel_totals():
    """{kernel: (launches, total ms)} of the profiler's report"""
    return {k: (v["launches"], v["avg_ms"] * v["launches"]) for k, v in P.profile_report().items()}


def updates(n, reps, with_literal):
    kinds = ["bare", "lqr"] + (["literal"] if with_literal else [])
    ms = {k: model(n, k) for k in kinds}
    want = {"bare": "canonical-form", "lqr": "canonical-groups", "literal": "literal"}
    for k, m in ms.items():
        assert m.objective.mode == want[k], (k, m.objective.mode)
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
    line = "n = %4d  update! device time of the objective: bare %8.1f us  lqr %8.1f us" % (n, total["bare"], total["lqr"])
    if with_literal:
        line += "  literal %8.1f us  literal / bare = %.1f" % (total["literal"], total["literal"] / total["bare"])
    print(line, flush=True)
    print("n = %4d  plan memory: %s" % (n, "  ".join("%s %.1f MB" % (k, m.device().bytes_allocated() / 1e6) for k, m in ms.items())), flush=True)
    for m in ms.values():
        m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="1024,2048,4096")
    ap.add_argument("--literal", type=int, default=1024, help="the size at which dot(e, Q*e) is measured too")
    a = ap.parse_args()
    _lib.require_gpu()
    flush = torch.empty(1 << 27, dtype=torch.float64, device=DEV)        # 1 GiB
    for n in [int(v) for v in a.sizes.split(",")]:
        node(n, a.reps, flush)
        updates(n, a.reps, n == a.literal)


if __name__ == "__main__":
    main()
