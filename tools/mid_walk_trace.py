#!/usr/bin/env python
"""Where the persistent walk of the one-launch Gram node (gram_mid.hip built with -DPMT_MID_TRACE; PMT_LIB_PATH points at that build)
spends its time OUTSIDE the main loops, and how its launch ends: per workgroup the phases summed over its items, per XCD the time its
ticket ran dry (the first of its workgroups to leave) and the time its last workgroup finished, per workgroup the time it stood idle
before the launch ended.  With a third argument m the node is recorded in a plan with an m x n constraint pack behind it, which rides in
the node (plan.hip: riders): rider tiles per workgroup, and per XCD the last rider store against the end of the last Gram item.
usage: PMT_LIB_PATH=.../trace.so python tools/mid_walk_trace.py 4096 4096 [512]"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import parametron_jl_amd  # noqa: F401,E402
from parametron_jl_amd import _lib  # noqa: E402

r, n = int(sys.argv[1]), int(sys.argv[2])
m_pack = int(sys.argv[3]) if len(sys.argv) > 3 else 0
lib = _lib.load()
dev = "cuda:0"
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
A = torch.rand(r * n, dtype=torch.float64, device=dev)
b = torch.rand(r, dtype=torch.float64, device=dev)
x = torch.arange(1, n + 1, dtype=torch.int64, device=dev)
nq = n * (n + 1) // 2
oq = torch.empty(nq * 3, dtype=torch.int64, device=dev)
ol = torch.empty(n * 2, dtype=torch.int64, device=dev)
oc = torch.empty(1, dtype=torch.float64, device=dev)
ws = torch.empty(max(1, lib.pmt_quad_gram_workspace_bytes(r, n) // 8), dtype=torch.float64, device=dev)
p = lambda t: C.c_void_p(t.data_ptr())
fn = C.CDLL(os.environ["PMT_LIB_PATH"]).pmt_mid_walk_read
fn.argtypes = [C.c_void_p]
fn_riders = C.CDLL(os.environ["PMT_LIB_PATH"]).pmt_mid_riders_read
fn_riders.argtypes = [C.c_void_p]


def node(s):
    _lib.call("pmt_quad_gram_f64", p(A), r, r, n, p(x), p(b), -1, 1, None, p(oq), p(ol), p(oc), p(ws), s)


launch = lambda: node(stream)
if m_pack:
    Cm, d = torch.rand(m_pack * n, dtype=torch.float64, device=dev), torch.rand(m_pack, dtype=torch.float64, device=dev)
    vt, vc = torch.empty(m_pack * n * 3, dtype=torch.int64, device=dev), torch.empty(m_pack, dtype=torch.float64, device=dev)
    plan = C.c_void_p()
    _lib.call("pmt_plan_create", 0, stream, C.byref(plan))
    rec = C.c_void_p(lib.pmt_plan_recording_stream(plan))
    _lib.call("pmt_plan_begin_record", plan)
    node(rec)
    _lib.call("pmt_affine_pack_vector_f64", p(Cm), m_pack, m_pack, n, p(x), p(d), -1, None, 0, p(vt), p(vc), rec)
    _lib.call("pmt_plan_end_record", plan)
    nr, nt = C.c_int(), C.c_int64()
    _lib.call("pmt_plan_riders", plan, C.byref(nr), C.byref(nt))
    print("plan: %d rider(s), %d tiles" % (nr.value, nt.value))
    launch = lambda: _lib.call("pmt_plan_update", plan)
for _ in range(20):
    launch()
torch.cuda.synchronize()
rows = []
for rep in range(5):          # five more launches, each read on its own
    launch()
    torch.cuda.synchronize()
    buf = (C.c_ulonglong * (1024 * 8))()
    assert fn(buf) == 0
    t = np.frombuffer(buf, dtype=np.uint64).reshape(1024, 8).astype(np.int64)
    t = t[t[:, 0] > 0]
    if len(t) > 256:
        sys.exit("%d workgroups with items: not the persistent form" % len(t))
    items = t[:, 0].astype(float)
    start, end = t[:, 5].min(), t[:, 6].max()
    us = lambda v: v / 100.0
    total = us(end - start)
    per = lambda k: us(t[:, k].sum()) / items.sum()
    print("launch %d: %d workgroups, %d items, first start -> last store %.1f us" % (rep, len(t), int(items.sum()), total))
    # (a deferring item, gram_mid.hip: MidWalk: its hand-off counts as "sums", it has no epilogue, and the write-out of the tile before it is inside its main loop)
    print("  per item: main loop %.2f us, sums / count / fold / hand-off %.2f, epilogue %.2f, last store or hand-off -> next start %.2f" % (per(1), per(2), per(3), us(t[:, 4].sum()) / max(1.0, (items - 1).sum())))
    busy = us(t[:, 1] + t[:, 2] + t[:, 3] + t[:, 4])
    print("  per workgroup: in main loops %.1f us (median), elsewhere %.1f; items %d .. %d" % (np.median(us(t[:, 1])), np.median(busy - us(t[:, 1])), items.min(), items.max()))
    idle = us(end - t[:, 6])
    print("  last item's end -> end of the launch: median %.1f us, mean %.1f, max %.1f" % (np.median(idle), idle.mean(), idle.max()))
    wg = np.flatnonzero(np.frombuffer(buf, dtype=np.uint64).reshape(1024, 8)[:, 0] > 0)
    dry, last = [], []
    for xcd in range(8):
        m = (wg & 7) == xcd
        dry.append(us(t[m, 7].min() - start))
        last.append(us(t[m, 6].max() - start))
    print("  per XCD, ticket dry (first workgroup leaves): " + " ".join("%.0f" % v for v in dry) + "   spread %.1f us" % (max(dry) - min(dry)))
    print("  per XCD, last workgroup's end:               " + " ".join("%.0f" % v for v in last) + "   spread %.1f us" % (max(last) - min(last)))
    if m_pack:
        rbuf = (C.c_ulonglong * (1024 * 2))()
        assert fn_riders(rbuf) == 0
        rt = np.frombuffer(rbuf, dtype=np.uint64).reshape(1024, 2).astype(np.int64)[wg]
        print("  rider tiles per workgroup: min %d, median %d, max %d, sum %d; workgroups with none %d" % (rt[:, 0].min(), np.median(rt[:, 0]), rt[:, 0].max(), rt[:, 0].sum(), (rt[:, 0] == 0).sum()))
        over = [us(rt[(wg & 7) == xcd, 1].max() - t[(wg & 7) == xcd, 6].max()) for xcd in range(8)]
        print("  per XCD, last rider store - last Gram item's end: " + " ".join("%.1f" % v for v in over) + " us")
        print("  the launch: last rider store - last Gram item's end %.1f us (> 0: the riders outlast the Gram items by that much)" % us(rt[:, 1].max() - end))
    rows.append((total, per(1), per(2), per(3), us(t[:, 4].sum()) / max(1.0, (items - 1).sum()), np.median(idle), max(dry) - min(dry), max(last) - min(last)))
m = np.median(np.array(rows), axis=0)
print("median of the launches: %.1f us; per item loop %.2f, sums %.2f, epilogue %.2f, between %.2f; idle at the end %.1f (median workgroup); XCDs dry within %.1f us, done within %.1f" % tuple(m))
