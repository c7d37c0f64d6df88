"""Times the sparse least-squares node pmt_sparse_gram_f64 (csrc/sparse_gram.hip) by HIP events at two patterns:
  (a) banded, m = 2^20, n = 2^18, 8 per row;
  (b) m = 65536, n = 2048, 8 random per row — there also the same matrix as a dense Parameter through pmt_quad_gram_f64.
Reports the time per call, GB/s on the algorithmic bytes 8 nprod + 8 (nq + 1) + 8 nq + 24 nq + 16 nlin + 8 nnz, and the fraction of 8 TB/s.
GPU box:  timeout -k 10 600 python tools/sparse_gram_probe.py [a|b] > profiles/r13_sparse_gram.txt"""
import ctypes as C
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import parametron_jl_amd  # noqa: E402
from parametron_jl_amd import _lib  # noqa: E402
from parametron_jl_amd.device import SparseGramTables, padded_lda  # noqa: E402

DEV = "cuda:0"
HBM = 8.0e12


def dptr(t):
    return C.c_void_p(t.data_ptr())


def dev_bytes(a):
    raw = np.frombuffer(np.ascontiguousarray(a).tobytes() + b"\0" * 8, dtype=np.uint8)
    return torch.from_numpy(raw.copy()).to(DEV)


def time_calls(fn, warmup=3, reps=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best, total = float("inf"), 0.0
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        best, total = min(best, ms), total + ms
    return best * 1e-3, total / reps * 1e-3


def banded(m, n, per_row, rng):
    rows = np.repeat(np.arange(m), per_row)
    cols = ((np.arange(m) * n // m)[:, None] + np.arange(per_row)[None, :]).reshape(-1) % n
    Cs = sp.csc_matrix((rng.random(len(rows)) - 0.5, (rows, cols)), shape=(m, n))
    Cs.sort_indices()
    return Cs


def random_rows(m, n, per_row, rng):
    """one column drawn at random from each of `per_row` equal column bands: distinct columns in every row"""
    band = n // per_row
    cols = (rng.integers(0, band, (m, per_row)) + np.arange(per_row)[None, :] * band).reshape(-1)
    rows = np.repeat(np.arange(m), per_row)
    Cs = sp.csc_matrix((rng.random(len(rows)) - 0.5, (rows, cols)), shape=(m, n))
    Cs.sort_indices()
    return Cs


def probe_sparse(name, Cs):
    m, n = Cs.shape
    t0 = time.time()
    T = SparseGramTables(None, m, n, Cs.indptr, Cs.indices, 2048)
    setup = time.time() - t0
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tabs = {k: dev_bytes(getattr(T, k)) for k in T.TABLES}
    nz = torch.from_numpy(Cs.data.copy()).to(DEV)
    x = torch.arange(1, n + 1, dtype=torch.int64, device=DEV)
    d = torch.rand(m, dtype=torch.float64, device=DEV) - 0.5
    oq = torch.empty(3 * max(T.nq, 1), dtype=torch.int64, device=DEV)
    ol = torch.empty(2 * max(T.nlin, 1), dtype=torch.int64, device=DEV)
    oc = torch.empty(1, dtype=torch.float64, device=DEV)
    args = T.call_args(m, lambda k: dptr(tabs[k]))

    def call(dvec, sign):
        _lib.call("pmt_sparse_gram_f64", dptr(nz), *args, dptr(x), dvec, sign, 1, dptr(x), dptr(oq), dptr(ol), dptr(oc), stream)
    nbytes = 8 * T.nprod + 8 * (T.nq + 1) + 8 * T.nq + 24 * T.nq + 16 * T.nlin + 8 * Cs.nnz
    print("%s: m = %d, n = %d, nnz = %d, nq = %d, nprod = %d, nlin = %d, runs = %d + %d linear, long segments = %d, long columns = %d" %
          (name, m, n, Cs.nnz, T.nq, T.nprod, T.nlin, T.nruns, T.nlin_runs, T.nlong, T.nlin_long))
    print("  symbolic phase (host, once per pattern): %.2f s; tables on the device: %.1f MB" % (setup, sum(v.numel() for v in tabs.values()) / 1e6))
    for label, dvec, sign in (("C*x - d", dptr(d), -1), ("C*x (no d: no constant chain)", None, 0)):
        best, mean = time_calls(lambda: call(dvec, sign))
        print("  %-32s best %8.1f us, mean %8.1f us; algorithmic bytes %.1f MB -> %.0f GB/s at best = %.3f of 8 TB/s"
              % (label, best * 1e6, mean * 1e6, nbytes / 1e6, nbytes / best / 1e9, nbytes / best / HBM))
    parametron_jl_amd.profile_enable(True)
    call(dptr(d), -1)
    torch.cuda.synchronize()
    rep = parametron_jl_amd.profile_report()
    parametron_jl_amd.profile_enable(False)
    print("  per kernel (one profiled call): " + ", ".join("%s %.1f us" % (k, v["avg_ms"] * 1e3) for k, v in sorted(rep.items()) if "sparse_gram" in k))
    return best


def probe_dense(Cs):
    m, n = Cs.shape
    lda = padded_lda(m)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    A = torch.zeros(lda * n, dtype=torch.float64, device=DEV)
    A.view(n, lda)[:, :m] = torch.from_numpy(np.ascontiguousarray(Cs.toarray().T)).to(DEV)
    x = torch.arange(1, n + 1, dtype=torch.int64, device=DEV)
    d = torch.rand(lda, dtype=torch.float64, device=DEV) - 0.5
    nq = n * (n + 1) // 2
    oq = torch.empty(3 * nq, dtype=torch.int64, device=DEV)
    ol = torch.empty(2 * n, dtype=torch.int64, device=DEV)
    oc = torch.empty(1, dtype=torch.float64, device=DEV)
    ws = torch.empty(max(16, int(_lib.load().pmt_quad_gram_workspace_bytes(m, n))) // 8 + 2, dtype=torch.float64, device=DEV)

    def call():
        _lib.call("pmt_quad_gram_f64", dptr(A), lda, m, n, dptr(x), dptr(d), -1, 1, dptr(x), dptr(oq), dptr(ol), dptr(oc), dptr(ws), stream)
    best, mean = time_calls(call)
    print("  the same matrix as a dense Parameter (pmt_quad_gram_f64, %d x %d, %d terms): best %8.1f us, mean %8.1f us" % (m, n, nq, best * 1e6, mean * 1e6))
    return best


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "ab"
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    if "a" in which:
        probe_sparse("(a) banded", banded(1 << 20, 1 << 18, 8, rng))
    if "b" in which:
        Cs = random_rows(65536, 2048, 8, rng)
        s = probe_sparse("(b) 8 random per row", Cs)
        dn = probe_dense(Cs)
        print("  sparse node / dense node: %.3f (%.1f x %s)" % (s / dn, max(s, dn) / min(s, dn), "faster" if s < dn else "SLOWER"))


if __name__ == "__main__":
    main()
