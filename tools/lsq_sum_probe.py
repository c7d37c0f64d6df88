"""Weighted least-squares sums (pmt_quad_gram_sum_f64) against the bare Gram node on the same device, in one process, alternating:
    bare       pmt_quad_gram_f64 of block 1 (moi = 1)
    composite  block 1 + pmt_quad_gram_csc_f64 of blocks 2..K + the combine
    combine    pmt_quad_gram_sum_f64 alone, its bytes over time as a fraction of 8 TB/s
Times are HIP events (median of --reps); kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/lsq_sum_probe.py`.
    python tools/lsq_sum_probe.py [--reps 50]                (GPU box)"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import parametron_jl_amd  # noqa: E402,F401
from parametron_jl_amd import _lib  # noqa: E402
from parametron_jl_amd.device import padded_lda  # noqa: E402

DEV = "cuda:0"
HBM = 8e12


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Block:
    def __init__(self, rows, n, seed):
        self.rows, self.n, self.lda = rows, n, padded_lda(rows)
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.A = torch.zeros(self.lda * n, dtype=torch.float64, device=DEV)
        _lib.call("pmt_fill_uniform_matrix_f64", ptr(self.A), rows, n, self.lda, seed, 1.0, s)
        self.b = torch.zeros(max(rows, 1), dtype=torch.float64, device=DEV)
        _lib.call("pmt_fill_uniform_f64", ptr(self.b), rows, seed + 1, 1.0, s)
        self.ws = torch.zeros(max(2, _lib.load().pmt_quad_gram_workspace_bytes(rows, n) // 8 + 1), dtype=torch.float64, device=DEV)
        nq = n * (n + 1) // 2
        self.v = torch.empty(max(nq, 1), dtype=torch.float64, device=DEV)
        self.lin = torch.empty(2 * n, dtype=torch.int64, device=DEV)
        self.c = torch.empty(1, dtype=torch.float64, device=DEV)

    def args(self, x):
        return (ptr(self.A), self.lda, self.rows, self.n, ptr(x), ptr(self.b), -1)


def case(name, n, extra_rows, lam, reps, rows1=4096):
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = torch.arange(1, n + 1, dtype=torch.int64, device=DEV)
    b1 = Block(rows1, n, 1)
    others = [Block(r, n, 10 + i) for i, r in enumerate(extra_rows)]
    nq = n * (n + 1) // 2
    q = torch.empty(3 * nq, dtype=torch.int64, device=DEV)
    lin, cc = torch.empty(2 * n, dtype=torch.int64, device=DEV), torch.empty(1, dtype=torch.float64, device=DEV)
    lam_d = torch.tensor([lam], dtype=torch.float64, device=DEV)
    terms = [{"kind": _lib.PMT_LSQ_BLOCK}]
    if lam:
        terms.append({"kind": _lib.PMT_LSQ_DIAG, "weight": lam_d.data_ptr()})
    for o in others:
        terms.append({"kind": _lib.PMT_LSQ_BLOCK, "values": o.v.data_ptr(), "lin": o.lin.data_ptr(), "constant": o.c.data_ptr()})
    arr = _lib.lsq_terms(terms)

    def bare():
        _lib.call("pmt_quad_gram_f64", *b1.args(x), 1, None, ptr(q), ptr(lin), ptr(cc), ptr(b1.ws), s)

    def combine():
        _lib.call("pmt_quad_gram_sum_f64", n, C.addressof(arr), len(terms), ptr(q), ptr(lin), ptr(cc), s)

    def composite():
        bare()
        for o in others:
            _lib.call("pmt_quad_gram_csc_f64", *o.args(x), None, 1.0, ptr(o.v), None, ptr(o.lin), ptr(o.c), ptr(o.ws), s)
        combine()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) * 1e3
    for fn in (bare, composite, combine):
        fn(); fn()
    torch.cuda.synchronize()
    t = {"bare": [], "composite": [], "combine": []}
    for _ in range(reps):                                  # alternating
        t["bare"].append(timed(bare))
        t["composite"].append(timed(composite))
        bare()                                             # (the combine works in place: give it block 1's terms again)
        torch.cuda.synchronize()
        t["combine"].append(timed(combine))
    med = {k: float(np.median(v)) for k, v in t.items()}
    diag = len(others) == 0
    nbytes = (48 * n + 32 * n + (8 * n if lam else 0)) if diag else (48 * nq + 8 * nq * len(others) + 32 * n * (1 + len(others)))
    print("%-44s bare %8.1f us  composite %8.1f us  (+%6.1f)  combine %7.1f us  %s  %6.1f MB  %.2f of 8 TB/s" % (
        name, med["bare"], med["composite"], med["composite"] - med["bare"], med["combine"], "diagonal" if diag else "full    ",
        nbytes / 1e6, nbytes / (med["combine"] * 1e-6) / HBM))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    _lib.require_gpu()
    case("4096x4096 (lda %d) + lam*dot(x,x)" % padded_lda(4096), 4096, [], 0.5, a.reps)
    case("4096x4096 + lam*dot(x,x) + 512x4096 block", 4096, [512], 0.5, a.reps)
    case("4096x512, two blocks", 512, [4096], 0.0, a.reps)


if __name__ == "__main__":
    main()
