"""Sums over disjoint Variable vectors as one canonical objective (mode "canonical-groups", csrc/groups.hip) on one device, in one process,
alternating.  Two forms transpose(x)*Q*x + transpose(u)*R*u of n = 2048 each, Variables created x then u (`ordered`: every group writes
straight into its slice) and x1, u1, x2, u2, .. (`interleaved`: arena + groups_gather_kernel):
    (a) groups    update! of the objective in mode "canonical-groups"
    (b) generic   the same objective wrapped in .canonicalize(): the literal expansion, the canonicalize! node and the pack — the path every
                  such objective took before the mode existed
    (c) alone     the two groups as objectives of models of their own ("canonical-form"), the sum of their update!s
update! here is its device part: Parameters marked dirty, the tape replayed, HIP events on the plan's stream round the replay (the copy of
the MOI buffers to the host is the same in (a) and (b) and is left out); Q and R are regenerated on the device at every update
(DeviceUniformParameter), their fill kernels are inside every figure.
    gather        pmt_quad_groups_gather_f64 stand-alone on the interleaved tables: back to back, and cold (behind a 1 GiB fill); 48 B per
                  quadratic term + 32 B per linear term over time as a fraction of 8 TB/s
    --big         dot(A*x - b, A*x - b) + dot(B*u - d, B*u - d) with two 4096 x 4096 blocks over different vectors: the model builds (its
                  literal function would be terabytes), update! time, 65536 sampled coefficients against long-double sums of 2 A'A at 1e-12
    python tools/separable_probe.py [--reps 50] [--n 2048] [--big]                (GPU box)"""
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
from parametron_jl_amd.device import fetch_f64  # noqa: E402

DEV = "cuda:0"
HBM = 8e12


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def variables(m, n, interleaved):
    x, u = [], []
    if interleaved:
        for _ in range(n):
            x.append(P.Variable(m))
            u.append(P.Variable(m))
    else:
        x = [P.Variable(m) for _ in range(n)]
        u = [P.Variable(m) for _ in range(n)]
    return x, u


def forms_model(n, interleaved, which):
    """which: 'groups' | 'generic' | 0 | 1 (group 0 / 1 alone)"""
    # generic: quadratic_mode="literal" + canonicalize(expr) is ONE canonicalize! node over the literal sum — what "canonical" mode did
    m = P.Model(P.MockOptimizer(), quadratic_mode="literal" if which == "generic" else "canonical")
    x, u = variables(m, n, interleaved)
    Q = P.DeviceUniformParameter((n, n), 1, m)
    R = P.DeviceUniformParameter((n, n), 2, m)
    fx, fu = P.transpose(x) * Q * x, P.transpose(u) * R * u
    expr = {"groups": lambda: fx + fu, "generic": lambda: (fx + fu).canonicalize(), 0: lambda: fx, 1: lambda: fu}[which]()
    P.objective(m, P.Minimize, expr)
    m.initialize()
    return m


def replay_us(m):
    """device time of one update!: the tape's replay between two events on the plan's stream"""
    ctx = m.device()
    s = torch.cuda.ExternalStream(ctx.stream.value)
    for p in m.params:
        p.setdirty()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    m._run_tape(fetch=False)
    e1.record(s)
    e1.synchronize()
    ctx.fetch_synchronize()
    ctx.synchronize()
    return e0.elapsed_time(e1) * 1e3


def updates(n, interleaved, reps):
    name = "interleaved" if interleaved else "ordered"
    ms = {"groups": forms_model(n, interleaved, "groups"), "generic": forms_model(n, interleaved, "generic"),
          "alone0": forms_model(n, interleaved, 0), "alone1": forms_model(n, interleaved, 1)}
    assert ms["groups"].objective.mode == "canonical-groups" and ms["groups"].objective.groups_ordered == (not interleaved)
    assert ms["generic"].objective.mode == "literal" and ms["alone0"].objective.mode == ms["alone1"].objective.mode == "canonical-form"
    for m in ms.values():
        for _ in range(3):
            m.update()
    # the function itself: equal to the generic path's word for word (sums of two numbers)
    a, b = ms["groups"].objective.f, ms["generic"].objective.f
    same = np.array_equal(a.quadratic_terms.view(np.int64), b.quadratic_terms.view(np.int64))
    print("n = %d x 2  %-11s %d quadratic terms, equal to the generic path's word for word: %s" % (n, name, len(a.quadratic_terms), same), flush=True)
    t = {k: [] for k in ms}
    for _ in range(reps):                                  # alternating
        for k, m in ms.items():
            t[k].append(replay_us(m))
    alone = np.array(t["alone0"]) + np.array(t["alone1"])
    rows = [("(a) groups", np.array(t["groups"])), ("(b) generic", np.array(t["generic"])), ("(c) alone, sum of two", alone)]
    for label, v in rows:
        print("n = %d x 2  %-11s update! %-22s median %8.1f us  min %8.1f  max %8.1f  quartiles %8.1f .. %8.1f  (%d updates)" % (
            n, name, label, np.median(v), v.min(), v.max(), np.percentile(v, 25), np.percentile(v, 75), len(v)), flush=True)
    ga, gb, gc = (float(np.median(v)) for _, v in rows)
    print("n = %d x 2  %-11s (b) / (a) = %.1f   (a) - (c) = %+.1f us" % (n, name, gb / ga, ga - gc), flush=True)
    for m in ms.values():
        m.close()


def gather(n, reps, flush):
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sets = [np.arange(1, 2 * n, 2), np.arange(2, 2 * n + 1, 2)]
    lay = _lib.GroupsLayout(sets)
    src = torch.randint(-2 ** 40, 2 ** 40, (3 * lay.nterms,), dtype=torch.int64, device=DEV)
    lin = torch.randint(-2 ** 40, 2 ** 40, (2 * lay.nlin,), dtype=torch.int64, device=DEV)
    tabs = [torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in (lay.row_src, lay.row_dst, lay.lin_src)]
    oq, ol = torch.empty_like(src), torch.empty_like(lin)

    def run():
        _lib.call("pmt_quad_groups_gather_f64", ptr(src), ptr(tabs[0]), ptr(tabs[1]), lay.nlin, lay.nterms, ptr(lin), ptr(tabs[2]), lay.nlin,
                  ptr(oq), ptr(ol), s)

    def timed():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) * 1e3
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    warm, cold = [], []
    for _ in range(reps):
        warm.append(timed())
        flush.fill_(1.0)
        torch.cuda.synchronize()
        cold.append(timed())
    nbytes = 48 * lay.nterms + 32 * lay.nlin
    for label, t in (("back to back", warm), ("cold", cold)):
        med = float(np.median(t))
        print("n = %d x 2  gather %-12s median %7.1f us  min %7.1f  %6.1f MB  %.2f of 8 TB/s" % (n, label, med, min(t), nbytes / 1e6,
                                                                                              nbytes / (med * 1e-6) / HBM), flush=True)


def big(reps):
    n = rows = 4096
    m = P.Model(P.MockOptimizer(), quadratic_mode="canonical")
    x, u = variables(m, n, False)
    A = P.DeviceUniformParameter((rows, n), 1, m, advance=False)
    b = P.DeviceUniformParameter((rows,), 2, m, advance=False)
    B = P.DeviceUniformParameter((rows, n), 3, m, advance=False)
    d = P.DeviceUniformParameter((rows,), 4, m, advance=False)
    r1, r2 = A * x - b, B * u - d
    P.objective(m, P.Minimize, P.dot(r1, r1) + P.dot(r2, r2))
    t0 = time.perf_counter()
    m.initialize()
    for _ in range(2):
        m.update()
    print("two 4096 x 4096 blocks over different vectors: mode %s, built and updated twice in %.1f s, %d quadratic terms" % (
        m.objective.mode, time.perf_counter() - t0, len(m.objective.f.quadratic_terms)), flush=True)
    t = np.array([replay_us(m) for _ in range(reps)])
    print("two 4096 x 4096 blocks: update! median %.1f us  min %.1f  max %.1f  (%d updates)" % (np.median(t), t.min(), t.max(), len(t)), flush=True)
    m.update()
    gq = m.objective.f.quadratic_terms
    ctx = m.device()
    nq = n * (n + 1) // 2
    rng = np.random.default_rng(3)
    iu = np.triu_indices(n)
    worst = 0.0
    for g, par in enumerate((A, B)):
        Ah = fetch_f64(ctx, par._dev.buf, par._dev.lda * n).reshape(n, par._dev.lda)[:, :rows]      # row j here = column j of the Parameter
        ctx.synchronize()
        pick = rng.choice(nq, 1 << 15, replace=False)
        j, k = iu[0][pick], iu[1][pick]
        got = gq[g * nq + pick]
        assert np.array_equal(got["row"], j + 1 + g * n) and np.array_equal(got["col"], k + 1 + g * n)
        for s in range(0, len(pick), 4096):
            a, bb = Ah[j[s:s + 4096]], Ah[k[s:s + 4096]]
            want = 2 * np.einsum("ij,ij->i", a.astype(np.longdouble), bb.astype(np.longdouble))
            mag = 2 * np.einsum("ij,ij->i", np.abs(a), np.abs(bb))
            err = np.abs(got["coeff"][s:s + 4096] - want.astype(np.float64)) / mag
            worst = max(worst, float(err.max()))
    print("two 4096 x 4096 blocks: 65536 sampled coefficients against long-double sums of 2 A'A: worst error %.2e of the terms' magnitude (bar 1e-12): %s" % (
        worst, "ok" if worst <= 1e-12 else "FAILED"), flush=True)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--big", action="store_true")
    a = ap.parse_args()
    _lib.require_gpu()
    for interleaved in (False, True):
        updates(a.n, interleaved, a.reps)
    flush = torch.empty(1 << 27, dtype=torch.float64, device=DEV)        # 1 GiB
    gather(a.n, a.reps, flush)
    del flush
    if a.big:
        big(a.reps)


if __name__ == "__main__":
    main()
