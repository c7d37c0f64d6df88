"""Times the sparse quadratic form node pmt_sparse_form_f64 (csrc/sparse_form.hip) by HIP events:
  (a) banded, n = 2^18, 8 entries per row (unsymmetric: a shape the dense node cannot hold) — back-to-back calls and cold calls (a 1 GB
      buffer is rewritten before each timed call), the fraction of 8 TB/s on the algorithmic bytes 16 nq (tables) + 24 nq (terms) +
      8 (values gathered);
  (b) n = 4096 at 1 % random fill, against the same matrix held dense through pmt_quad_form_f64, the two alternating in the same run,
      five rounds: the spread between rounds is the run-to-run scatter the comparison is read against;
  (c) the pattern of (a) through Model.update(): the bare form, the ridge x'Qx + lam*dot(x, x) and the QP 0.5*x'Qx + dot(c, x) + s, by the
      host clock around synchronising updates (Q's values regenerated on the device at every update).
GPU box:  timeout -k 10 900 python tools/sparse_form_probe.py [abc] > profiles/r16_sparse_form.txt"""
import ctypes as C
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import parametron_jl_amd as P  # noqa: E402
from parametron_jl_amd import _lib  # noqa: E402
from parametron_jl_amd.device import SparseFormTables  # noqa: E402
from sparse_gram_probe import DEV, HBM, dev_bytes, dptr, time_calls  # noqa: E402


def banded(n, per_row, rng):
    """row i holds columns (i - 2 .. i + per_row - 3) mod n: two below the diagonal, the diagonal, the rest above — pairs stored twice,
    once above and once below"""
    rows = np.repeat(np.arange(n), per_row)
    cols = (np.arange(n)[:, None] + np.arange(-2, per_row - 2)[None, :]).reshape(-1) % n
    Q = sp.csc_matrix((rng.random(len(rows)) - 0.5, (rows, cols)), shape=(n, n))
    Q.sort_indices()
    return Q


def random_fill(n, fill, rng):
    Q = sp.random(n, n, density=fill, format="csc", random_state=rng, data_rvs=lambda k: rng.random(k) - 0.5)
    Q.sort_indices()
    return Q


class Form:
    """one sparse form on the device: its tables, values and output"""

    def __init__(self, Q):
        n = Q.shape[0]
        t0 = time.time()
        self.T = T = SparseFormTables(None, n, Q.indptr, Q.indices)
        self.setup = time.time() - t0
        self.tabs = {k: dev_bytes(getattr(T, k)) for k in T.TABLES}
        self.nz = torch.from_numpy(Q.data.copy()).to(DEV)
        self.x = torch.arange(1, n + 1, dtype=torch.int64, device=DEV)
        self.oq = torch.empty(3 * max(T.nq, 1), dtype=torch.int64, device=DEV)
        self.oc = torch.empty(1, dtype=torch.float64, device=DEV)
        gathered = int(np.count_nonzero(T.src_a != 0xFFFFFFFF) + np.count_nonzero(T.src_b != 0xFFFFFFFF))
        self.nbytes = 16 * T.nq + 24 * T.nq + 8 * gathered
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(self):
        T = self.T
        _lib.call("pmt_sparse_form_f64", dptr(self.nz), *[dptr(self.tabs[k]) for k in ("src_a", "src_b", "pair_j", "pair_k")], T.nq, dptr(self.x), 1,
                  dptr(self.x), dptr(self.oq), dptr(self.oc), self.stream)


def us(t):
    return "best %8.1f us, mean %8.1f us" % (t[0] * 1e6, t[1] * 1e6)


def time_cold(fn, reps=10):
    """every timed call behind a rewrite of a 1 GB buffer: nothing of the tables, the values or the output is left in a cache"""
    junk = torch.empty(1 << 27, dtype=torch.float64, device=DEV)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best, total = float("inf"), 0.0
    fn()
    for r in range(reps):
        junk.fill_(float(r))
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        best, total = min(best, ms), total + ms
    return best * 1e-3, total / reps * 1e-3


def time_batch(fn, calls=50, reps=5):
    """back-to-back: `calls` calls between one pair of events, per call"""
    def batch():
        for _ in range(calls):
            fn()
    b, m = time_calls(batch, warmup=1, reps=reps)
    return b / calls, m / calls


def rate(f, t):
    return "algorithmic bytes %.1f MB -> %.0f GB/s at best = %.3f of 8 TB/s" % (f.nbytes / 1e6, f.nbytes / t[0] / 1e9, f.nbytes / t[0] / HBM)


def probe_a(Q):
    f = Form(Q)
    n = Q.shape[0]
    print("(a) banded: n = %d, nnz = %d, nq = %d; symbolic phase (host, once per pattern): %.2f s; tables on the device: %.1f MB"
          % (n, Q.nnz, f.T.nq, f.setup, 16 * f.T.nq / 1e6))
    one = time_calls(f.call)
    print("  one call per event pair (warm)   %s; %s" % (us(one), rate(f, one)))
    bb = time_batch(f.call)
    print("  back to back (50 calls per pair) %s; %s" % (us(bb), rate(f, bb)))
    cold = time_cold(f.call)
    print("  cold (1 GB rewritten before)     %s; %s" % (us(cold), rate(f, cold)))


def probe_b(Q):
    n = Q.shape[0]
    f = Form(Q)
    stream = f.stream
    dense = torch.from_numpy(np.ascontiguousarray(Q.toarray().T).reshape(-1)).to(DEV)
    nq = n * (n + 1) // 2
    oq, oc = torch.empty(3 * nq, dtype=torch.int64, device=DEV), torch.empty(1, dtype=torch.float64, device=DEV)

    def dense_call():
        _lib.call("pmt_quad_form_f64", dptr(dense), n, n, dptr(f.x), 1, dptr(f.x), 1.0, dptr(oq), None, None, dptr(oc), stream)
    print("(b) n = %d at %.1f %% random fill: nnz = %d, nq = %d (dense node: %d terms); bytes sparse %.2f MB, dense %.1f MB (8 n^2 read + 24 per term)"
          % (n, 100.0 * Q.nnz / n / n, Q.nnz, f.T.nq, nq, f.nbytes / 1e6, (8 * n * n + 24 * nq) / 1e6))
    rounds = []
    for r in range(5):
        s, d = time_calls(f.call), time_calls(dense_call)
        sb, db = time_batch(f.call), time_batch(dense_call)
        rounds.append((s[0], d[0], sb[0], db[0]))
        print("  round %d: sparse node %s | dense node %s | back to back: sparse %.1f us, dense %.1f us" % (r, us(s), us(d), sb[0] * 1e6, db[0] * 1e6))
    a = np.array(rounds) * 1e6
    print("  over the rounds (best times, us): sparse %.1f .. %.1f, dense %.1f .. %.1f; back to back: sparse %.1f .. %.1f, dense %.1f .. %.1f"
          % (a[:, 0].min(), a[:, 0].max(), a[:, 1].min(), a[:, 1].max(), a[:, 2].min(), a[:, 2].max(), a[:, 3].min(), a[:, 3].max()))
    print("  sparse / dense at the rounds' best: %.3f one call per pair, %.3f back to back; the sparse node is %s beyond the scatter shown"
          % (a[:, 0].min() / a[:, 1].min(), a[:, 2].min() / a[:, 3].min(), "NOT slower" if a[:, 2].min() <= a[:, 3].max() else "SLOWER"))


def probe_c(Q):
    n = Q.shape[0]
    out = {}
    for kind in ("bare", "ridge", "qp"):
        model = P.Model(P.MockOptimizer())
        try:
            x = [P.Variable(model) for _ in range(n)]
            Qp = P.DeviceUniformSparseParameter(Q, 7, model)
            form = P.transpose(x) * Qp * x
            if kind == "ridge":
                lam = P.Parameter(lambda: 0.25, model)
                expr = form + lam * P.dot(x, x)
            elif kind == "qp":
                c = P.DeviceUniformParameter((n,), 8, model)
                s = P.Parameter(lambda: 0.75, model)
                expr = 0.5 * form + P.dot(c, x) + s
            else:
                expr = form
            P.objective(model, P.Minimize, expr)
            t0 = time.time()
            P.solve(model)
            first = time.time() - t0
            times = []
            for _ in range(12):
                model.setdirty()
                t0 = time.perf_counter()
                model.update()
                times.append(time.perf_counter() - t0)
            times = np.array(times[2:])
            out[kind] = times.min()
            print("  %-5s mode %-22s nq = %d; first solve (symbolic phases, tables) %.2f s; update(): best %8.1f us, mean %8.1f us (host clock, synchronising)"
                  % (kind, model.objective.mode, len(model.objective.f.quadratic_terms), first, times.min() * 1e6, times.mean() * 1e6))
        finally:
            model.close()
    print("  ridge - bare = %.1f us, qp - bare = %.1f us (the block's scratch pass plus the combine; at best times)"
          % ((out["ridge"] - out["bare"]) * 1e6, (out["qp"] - out["bare"]) * 1e6))


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "abc"
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    print("device: %s" % torch.cuda.get_device_name(0))
    big = banded(1 << 18, 8, rng) if ("a" in which or "c" in which) else None
    if "a" in which:
        probe_a(big)
    if "b" in which:
        probe_b(random_fill(4096, 0.01, rng))
    if "c" in which:
        print("(c) the pattern of (a) through Model.update(), MOI hand-off (the terms are fetched to the host at every update)")
        probe_c(big)


if __name__ == "__main__":
    main()
