"""Times the combine of weighted sums over sparse least-squares blocks, pmt_sparse_gram_sum_f64 (csrc/sparse_gram_sum.hip), by HIP events
on the two matrices of tools/sparse_gram_probe.py:
  (A) banded, m = 2^20, n = 2^18, 8 per row;
  (B) m = 65536, n = 2048, 8 random per row — there also the dense "canonical-sum" time of the same ridge.
Timed, in one process, warm-up then best and mean over 20 calls:
  (a) the bare node pmt_sparse_gram_f64;
  (b) the ridge sum dot(r, r) + lam*dot(x, x), K = 1: the block into its scratch lists, then the combine;
  (c) a two-block sum w1*dot(r1, r1) + w2*dot(r2, r2) + lam*dot(x, x): r2 from the same generator (banded: the same pattern; random: another one);
  (d) the combine of (b) and of (c) alone.
Reports (b) - (a) and (c) - 2 (a) as the combine's cost, and the combine's GB/s and fraction of 8 TB/s on its algorithmic bytes: the
gather tables (4 bytes per block and output term), the coefficient word of each block term read (8 bytes) and the structs written (24 / 16).
GPU box:  timeout -k 10 900 python tools/sparse_sum_probe.py [A|B] > profiles/r14_sparse_sum.txt"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import parametron_jl_amd  # noqa: E402,F401
from parametron_jl_amd import _lib  # noqa: E402
from parametron_jl_amd.device import SparseGramTables, SparseSumTables, padded_lda  # noqa: E402
from sparse_gram_probe import DEV, HBM, banded, dev_bytes, dptr, random_rows, time_calls  # noqa: E402


class Block:
    """one sparse block on the device: its tables, values, d and the scratch lists pmt_sparse_gram_f64 writes"""

    def __init__(self, Cs):
        self.Cs = Cs
        m, n = Cs.shape
        self.T = T = SparseGramTables(None, m, n, Cs.indptr, Cs.indices, 2048)
        self.tabs = {k: dev_bytes(getattr(T, k)) for k in T.TABLES}
        self.nz = torch.from_numpy(Cs.data.copy()).to(DEV)
        self.d = torch.rand(m, dtype=torch.float64, device=DEV) - 0.5
        self.q = torch.empty(3 * max(T.nq, 1), dtype=torch.int64, device=DEV)
        self.l = torch.empty(2 * max(T.nlin, 1), dtype=torch.int64, device=DEV)
        self.c = torch.empty(1, dtype=torch.float64, device=DEV)
        self.args = T.call_args(m, lambda k: dptr(self.tabs[k]))

    def gram(self, x, stream, out=None):
        q, l, c = out or (self.q, self.l, self.c)
        _lib.call("pmt_sparse_gram_f64", dptr(self.nz), *self.args, dptr(x), dptr(self.d), -1, 1, dptr(x), dptr(q), dptr(l), dptr(c), stream)


class Sum:
    """the combine of `blocks` (weights: device scalars) + lam*dot(x, x)"""

    def __init__(self, n, blocks):
        t0 = time.time()
        kinds = [(_lib.PMT_LSQ_BLOCK, False, None)] * len(blocks) + [(_lib.PMT_LSQ_DIAG, False, None)]
        self.S = S = SparseSumTables(None, n, [b.T for b in blocks], kinds)
        self.setup = time.time() - t0
        self.n, self.blocks = n, blocks
        self.keep = [dev_bytes(a) for a in [S.pair_j, S.pair_k, S.lin_col] + S.quad_at + S.lin_at]
        K = len(blocks)
        self.w = torch.tensor([1.5, -0.625, 0.25][:K] + [0.25], dtype=torch.float64, device=DEV)
        desc = [dict(kind=_lib.PMT_LSQ_BLOCK, weight=self.w.data_ptr() + 8 * k, quad=b.q.data_ptr(), lin=b.l.data_ptr(), constant=b.c.data_ptr(),
                     quad_at=self.keep[3 + k].data_ptr(), lin_at=self.keep[3 + K + k].data_ptr()) for k, b in enumerate(blocks)]
        desc.append(dict(kind=_lib.PMT_LSQ_DIAG, weight=self.w.data_ptr() + 8 * K, nvec=n))
        self.arr = _lib.sparse_lsq_terms(desc)
        self.nterms = len(desc)
        self.oq = torch.empty(3 * max(S.nq, 1), dtype=torch.int64, device=DEV)
        self.ol = torch.empty(2 * max(S.nlin, 1), dtype=torch.int64, device=DEV)
        self.oc = torch.empty(1, dtype=torch.float64, device=DEV)
        self.nbytes = 4 * K * (S.nq + S.nlin) + 8 * sum(b.T.nq + b.T.nlin for b in blocks) + 24 * S.nq + 16 * S.nlin

    def combine(self, x, stream):
        S = self.S
        _lib.call("pmt_sparse_gram_sum_f64", self.n, C.addressof(self.arr), self.nterms, dptr(self.keep[0]), dptr(self.keep[1]), S.nq, dptr(self.keep[2]),
                  S.nlin, dptr(x), dptr(x), dptr(self.oq), dptr(self.ol), dptr(self.oc), stream)

    def whole(self, x, stream):
        for b in self.blocks:
            b.gram(x, stream)
        self.combine(x, stream)


def us(t):
    return "best %8.1f us, mean %8.1f us" % (t[0] * 1e6, t[1] * 1e6)


def probe(name, C1, C2, dense=False):
    m, n = C1.shape
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = torch.arange(1, n + 1, dtype=torch.int64, device=DEV)
    b1, b2 = Block(C1), Block(C2)
    out = (torch.empty_like(b1.q), torch.empty_like(b1.l), torch.empty_like(b1.c))
    ridge, two = Sum(n, [b1]), Sum(n, [b1, b2])
    print("%s: m = %d, n = %d, nnz = %d; block 1: nq = %d, nlin = %d; block 2: nq = %d, nlin = %d" % (name, m, n, C1.nnz, b1.T.nq, b1.T.nlin, b2.T.nq, b2.T.nlin))
    print("  merged: ridge nq = %d, nlin = %d (merge on the host, once: %.2f s); two blocks nq = %d, nlin = %d (%.2f s)"
          % (ridge.S.nq, ridge.S.nlin, ridge.setup, two.S.nq, two.S.nlin, two.setup))
    a = time_calls(lambda: b1.gram(x, stream, out))
    b = time_calls(lambda: ridge.whole(x, stream))
    c = time_calls(lambda: two.whole(x, stream))
    a2 = time_calls(lambda: b2.gram(x, stream, out))
    print("  (a) bare pmt_sparse_gram_f64                      %s   (block 2 alone: best %.1f us)" % (us(a), a2[0] * 1e6))
    print("  (b) ridge, K = 1: block + combine                 %s" % us(b))
    print("  (c) two blocks + lam*dot(x, x): 2 blocks + combine %s" % us(c))
    print("  combine's cost: (b) - (a) = %.1f us;  (c) - 2 (a) = %.1f us   (at best times)" % ((b[0] - a[0]) * 1e6, (c[0] - 2 * a[0]) * 1e6))
    for label, s in (("ridge", ridge), ("two blocks", two)):
        t = time_calls(lambda: s.combine(x, stream))
        print("  (d) the combine alone, %-10s %s; algorithmic bytes %.1f MB -> %.0f GB/s at best = %.3f of 8 TB/s; on its cost in the sum "
              "(%.1f us): %.3f" % (label, us(t), s.nbytes / 1e6, s.nbytes / t[0] / 1e9, s.nbytes / t[0] / HBM,
                                   ((b[0] - a[0]) if s is ridge else (c[0] - 2 * a[0])) * 1e6,
                                   s.nbytes / max((b[0] - a[0]) if s is ridge else (c[0] - 2 * a[0]), 1e-9) / HBM))
    if dense:
        lda = padded_lda(m)
        A = torch.zeros(lda * n, dtype=torch.float64, device=DEV)
        A.view(n, lda)[:, :m] = torch.from_numpy(np.ascontiguousarray(C1.toarray().T)).to(DEV)
        d = torch.rand(lda, dtype=torch.float64, device=DEV) - 0.5
        nq = n * (n + 1) // 2
        oq, ol = torch.empty(3 * nq, dtype=torch.int64, device=DEV), torch.empty(2 * n, dtype=torch.int64, device=DEV)
        oc = torch.empty(1, dtype=torch.float64, device=DEV)
        ws = torch.empty(max(16, int(_lib.load().pmt_quad_gram_workspace_bytes(m, n))) // 8 + 2, dtype=torch.float64, device=DEV)
        lam = torch.tensor([0.25], dtype=torch.float64, device=DEV)
        arr = _lib.lsq_terms([dict(kind=_lib.PMT_LSQ_BLOCK), dict(kind=_lib.PMT_LSQ_DIAG, weight=lam.data_ptr())])

        def call():
            _lib.call("pmt_quad_gram_f64", dptr(A), lda, m, n, dptr(x), dptr(d), -1, 1, dptr(x), dptr(oq), dptr(ol), dptr(oc), dptr(ws), stream)
            _lib.call("pmt_quad_gram_sum_f64", n, C.addressof(arr), 2, dptr(oq), dptr(ol), dptr(oc), stream)
        t = time_calls(call)
        print("  the same ridge with C a dense Parameter (canonical-sum: pmt_quad_gram_f64 + pmt_quad_gram_sum_f64, %d terms): %s -> sparse sum is %.1f x %s"
              % (nq, us(t), max(t[0], b[0]) / min(t[0], b[0]), "faster" if b[0] < t[0] else "SLOWER"))


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "AB"
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    if "A" in which:
        probe("(A) banded", banded(1 << 20, 1 << 18, 8, rng), banded(1 << 20, 1 << 18, 8, rng))
    if "B" in which:
        probe("(B) 8 random per row", random_rows(65536, 2048, 8, rng), random_rows(65536, 2048, 8, rng), dense=True)


if __name__ == "__main__":
    main()
