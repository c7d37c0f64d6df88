"""CPU-only: who rides in a one-launch Gram node (csrc/plan.hip: pmt_plan_rider_check, the pure decision behind pmt_plan_end_record's
riders) — as a table of tapes described by kind, lane, shape and byte ranges, without a device.  A rider is a dense MOI vector pack
(update!(::MOI.VectorAffineFunction), src/moi_interop.jl:64-81) whose tiles the node's persistent workgroups draw once their Gram items
have run out (csrc/gram_mid.hip); it may only move into the node when both orders of the two give the same memory."""
import ctypes as C

import pytest

import __graft_entry__ as entry

OTHER, NODE, PACK = 0, 1, 2
RANGES = 5
CAP = 256 << 20                                     # PMT_MID_RIDER_BYTES: algorithmic bytes (32 per entry) of one node's riders


class Entry(C.Structure):
    _fields_ = [("kind", C.c_int32), ("lane", C.c_int32), ("rows", C.c_int64), ("cols", C.c_int64),
                ("reads", (C.c_uint64 * 2) * RANGES), ("writes", (C.c_uint64 * 2) * RANGES)]


@pytest.fixture(scope="module")
def lib():
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


def _entry(kind, lane, rows, cols, reads=(), writes=()):
    e = Entry(kind, lane, rows, cols)
    for k, (a, n) in enumerate(reads):
        e.reads[k][0], e.reads[k][1] = a, a + n
    for k, (a, n) in enumerate(writes):
        e.writes[k][0], e.writes[k][1] = a, a + n
    return e


SLOT = 1 << 32
# the node: 64 x 2112 (562 work items: persistent at any row count); every buffer in a 4 GiB slot of its own
N_ROWS, N_COLS = 64, 2112
A, B, XVAR, VARMAP, OUT_QUAD, OUT_LIN, OUT_CONST, WS = (k * SLOT for k in range(1, 9))
NQ = N_COLS * (N_COLS + 1) // 2


def node(rows=N_ROWS, cols=N_COLS, lane=0):
    return _entry(NODE, lane, rows, cols,
                  reads=[(A, 8 * rows * cols), (B, 8 * rows), (XVAR, 8 * cols), (VARMAP, 8 * cols)],
                  writes=[(OUT_QUAD, 24 * NQ), (OUT_LIN, 16 * cols), (OUT_CONST, 8), (WS, 32 << 20)])


def pack(k, rows=64, cols=128, lane=0, **over):
    """pack number k with buffers of its own (slot 16 + 4 k ..); `over` replaces the base address of one of C, d, out, consts"""
    base = {"C": (16 + 4 * k) * SLOT, "d": (17 + 4 * k) * SLOT, "out": (18 + 4 * k) * SLOT, "consts": (19 + 4 * k) * SLOT}
    base.update(over)
    return _entry(PACK, lane, rows, cols,
                  reads=[(base["C"], 8 * rows * cols), (XVAR, 8 * cols), (base["d"], 8 * rows), (VARMAP, 8 * cols)],
                  writes=[(base["out"], 24 * rows * cols), (base["consts"], 8 * rows)])


def other(lane=0):
    return _entry(OTHER, lane, 0, 0)


def check(lib, tape, at):
    arr = (Entry * len(tape))(*tape)
    rides = (C.c_int * len(tape))()
    count, tiles = C.c_int(-1), C.c_int64(-1)
    lib.call("pmt_plan_rider_check", C.cast(arr, C.c_void_p), len(tape), at, rides, C.byref(count), C.byref(tiles))
    assert count.value == sum(rides)
    return list(rides), tiles.value


TABLE = [
    # name, tape, index of the node, who rides
    ("an independent pack behind the node rides", [node(), pack(0)], 0, [0, 1]),
    ("two independent packs behind the node ride", [node(), pack(0), pack(1)], 0, [0, 1, 1]),
    ("b of the pack is the node's out_lin", [node(), pack(0, d=OUT_LIN)], 0, [0, 0]),
    ("A of the pack lies in the node's out_quad", [node(), pack(0, C=OUT_QUAD + 4096)], 0, [0, 0]),
    ("A of the pack lies in the node's workspace", [node(), pack(0, C=WS + 8)], 0, [0, 0]),
    ("the pack writes into the node's A", [node(), pack(0, out=A + 16)], 0, [0, 0]),
    ("the pack's constants land in the node's b", [node(), pack(0, consts=B)], 0, [0, 0]),
    ("two packs write the same output: the first rides", [node(), pack(0), pack(1, out=pack(0).writes[0][0] + 24)], 0, [0, 1, 0]),
    ("a pack reads what a pack that stays behind writes", [node(), pack(0, d=OUT_LIN), pack(1, C=pack(0).writes[0][0])], 0, [0, 0, 0]),
    ("an entry that is no pack between the node and the pack", [node(), other(), pack(0)], 0, [0, 0, 0]),
    ("the run of packs ends at the first other entry", [node(), pack(0), other(), pack(1)], 0, [0, 1, 0, 0]),
    ("a pack in front of the node on the plan's own lane", [pack(0), node()], 1, [0, 0]),
    ("a side-lane pack in front of the node rides", [pack(0, lane=1), node()], 1, [1, 0]),
    ("a side-lane pack behind another entry of the plan's lane rides", [node(), other(), pack(0, lane=1)], 0, [0, 0, 1]),
    ("a side-lane pack with an unknown side-lane neighbour (a recorded fetch of its output)", [pack(0, lane=1), other(lane=1), node()], 2, [0, 0, 0]),
    ("side-lane entries between the node and a pack of its own lane do not end the run", [node(), other(lane=1), pack(0)], 0, [0, 0, 1]),
    ("zero rows", [node(), pack(0, rows=0)], 0, [0, 0]),
    ("zero columns", [node(), pack(0, cols=0)], 0, [0, 0]),
    ("a node below two rounds (64 x 512) takes nobody", [node(64, 512), pack(0)], 0, [0, 0]),
    ("a pack over the byte cap", [node(), pack(0, rows=2048, cols=CAP // 32 // 2048 + 64)], 0, [0, 0]),
    ("a pack of exactly the byte cap rides", [node(), pack(0, rows=2048, cols=CAP // 32 // 2048)], 0, [0, 1]),
    ("two packs that exceed the cap together: the first rides", [node(), pack(0, rows=2048, cols=2048), pack(1, rows=2048, cols=2112)], 0, [0, 1, 0]),
    ("a ninth rider stays", [node()] + [pack(k) for k in range(9)], 0, [0] + [1] * 8 + [0]),
]


@pytest.mark.parametrize("name,tape,at,want", TABLE, ids=[t[0] for t in TABLE])
def test_who_rides(lib, name, tape, at, want):
    rides, tiles = check(lib, tape, at)
    assert rides == want, name
    # tiles: 64 columns wide; 32 rows high where 64-row tiles would be fewer than 1024 (and the block has more than 32 rows), else 64
    def ntiles(e):
        tr = 32 if (-(-e.cols // 64)) * (-(-e.rows // 64)) < 1024 and e.rows > 32 else 64
        return (-(-e.cols // 64)) * (-(-e.rows // tr))
    assert tiles == sum(ntiles(e) for e, r in zip(tape, rides) if r)


def test_the_node_index_must_name_a_node(lib):
    tape = [node(), pack(0)]
    arr = (Entry * 2)(*tape)
    rides = (C.c_int * 2)()
    with pytest.raises(lib.ArgumentError):
        lib.call("pmt_plan_rider_check", C.cast(arr, C.c_void_p), 2, 1, rides, None, None)
    with pytest.raises(lib.ArgumentError):
        lib.call("pmt_plan_rider_check", C.cast(arr, C.c_void_p), 2, 2, rides, None, None)
