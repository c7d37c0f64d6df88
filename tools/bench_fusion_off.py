#!/usr/bin/env python
"""bench.py with every plan replayed as recorded: pmt_plan_set_fusion(plan, 0) right behind each pmt_plan_end_record — no fused runs of
small nodes and no riders in the one-launch Gram node (include/parametron_hip.h).  Tells "the kernel's text changed" from "the riders
ride" in a same-box comparison of two builds (profiles/r15_gram_riders.txt).

    python tools/bench_fusion_off.py --gpus 1 --steps 200 --warmup 10
"""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parametron_jl_amd import _lib  # noqa: E402

_call = _lib.call


def call(name, *args):
    rc = _call(name, *args)
    if name == "pmt_plan_end_record":
        _call("pmt_plan_set_fusion", args[0], 0)
    return rc


_lib.call = call
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
runpy.run_path(sys.argv[0], run_name="__main__")
