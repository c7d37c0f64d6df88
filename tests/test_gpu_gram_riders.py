"""-m gpu: RIDERS of the one-launch canonical objective node (csrc/gram_mid.hip: mid_rider_tile; csrc/plan.hip: choose_riders) — dense MOI
constraint packs (pmt_affine_pack_vector_f64 = update!(::MOI.VectorAffineFunction), src/moi_interop.jl:64-81, of matvecmul! + vecsubtract!,
src/functions.jl:775-798,751-764) recorded beside a node that runs persistent, whose tiles the node's workgroups draw once their Gram items
have run out.  The node is the smallest that runs persistent: 64 x 2112 (562 work items), with exact-integer data as in
test_gpu_gram_mid_items.py: Q = 2 A'A, q = 2 A'c and c'c must equal the int64 results bit for bit with riders on.  Every output lives in
a poisoned buffer with guards (gpu_util.Guarded) whose whole image is compared: against the numpy restatement of the pack, with the
riders riding and again with the same tape replayed as recorded (pmt_plan_set_fusion 0)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROWS, N = 64, 2112
NQ = N * (N + 1) // 2
ROW_OFFSET = 7


def _riders(g, plan):
    n, tiles = C.c_int(-1), C.c_int64(-1)
    g.call("pmt_plan_riders", plan.plan, C.byref(n), C.byref(tiles))
    return n.value, tiles.value


def _tiles(rows, cols):
    tr = 32 if (-(-cols // 64)) * (-(-rows // 64)) < 1024 and rows > 32 else 64
    return (-(-cols // 64)) * (-(-rows // tr))


class Node:
    """the objective's operands (integers of [-3, 3]: every partial sum is exact in float64) and the image its three outputs must have"""

    def __init__(self, rows=ROWS, n=N, pad=0, seed=1):
        import gpu_util as g
        rng = np.random.default_rng(seed)
        self.rows, self.n, self.lda = rows, n, rows + pad
        A = rng.integers(-3, 4, size=(rows, n), dtype=np.int64)
        b = rng.integers(-3, 4, size=rows, dtype=np.int64)
        buf = np.full(self.lda * n, 1e300)
        buf.reshape(n, self.lda)[:, :rows] = A.T
        self.dA, self.db = g.to_dev(buf), g.to_dev(b.astype(np.float64))
        self.xvar = g.to_dev(np.arange(1, n + 1, dtype=np.int64))
        self.vm_h = rng.permutation(n).astype(np.int64) + 1 + 5
        self.vm = g.to_dev(self.vm_h)
        self.ws = g.empty_f64(g.lib().pmt_quad_gram_workspace_bytes(rows, n) // 8)
        assert 9 * rows < 2 ** 13
        At, c = torch.from_numpy(A), -b
        G = 2 * (At.T @ At).numpy()
        iu = np.triu_indices(n)
        self.quad = np.zeros(n * (n + 1) // 2, dtype=g.QT)
        self.quad["coeff"], self.quad["row"], self.quad["col"] = G[iu].astype(np.float64), self.vm_h[iu[0]], self.vm_h[iu[1]]
        self.lin = np.zeros(n, dtype=g.LT)
        self.lin["coeff"], self.lin["var"] = (2 * (A.T @ c)).astype(np.float64), self.vm_h
        self.const = np.array([float(c @ c)])
        self.out = (g.Guarded(3 * len(self.quad)), g.Guarded(2 * n), g.Guarded(1, doubles=True))

    def record(self, g, stream):
        oq, ol, oc = self.out
        g.call("pmt_quad_gram_f64", g.ptr(self.dA), self.lda, self.rows, self.n, g.ptr(self.xvar), g.ptr(self.db), -1, 1, g.ptr(self.vm),
               oq.ptr(), ol.ptr(), oc.ptr(), g.ptr(self.ws), stream)

    def guarded(self):
        return list(self.out)

    def check(self, what):
        for buf, want, name in zip(self.out, (self.quad, self.lin, self.const), ("Q", "q", "c'c")):
            buf.check(want.view(np.int64) if want.dtype.fields else want, "%s: %s" % (what, name))


class Pack:
    """one dense constraint block C x (+|-) d of rows x cols with a permuted variable vector, and the images of its two outputs"""

    def __init__(self, node, rows, cols, seed, pad=0, shift=0, sign=-1, has_b=True, has_consts=True):
        import gpu_util as g
        rng = np.random.default_rng(seed)
        self.rows, self.cols, self.lda, self.sign = rows, cols, rows + pad, sign if has_b else 0
        Cm = rng.standard_normal((rows, cols))
        buf = np.full(self.lda * cols, 1e300)
        buf.reshape(cols, self.lda)[:, :rows] = Cm.T
        self.dC = g.to_dev(buf)
        d = rng.standard_normal(rows)
        self.d_h = d if has_b else None
        self.dd = g.to_dev(d) if has_b else None
        xv = rng.permutation(node.n)[:cols].astype(np.int64) + 1
        if cols > node.n:                                            # more columns than the node has variables: some of them share one
            xv = np.concatenate([xv, rng.integers(1, node.n + 1, size=cols - node.n, dtype=np.int64)])
        self.xvar, self.vm = g.to_dev(xv), node.vm
        self.terms = np.zeros(rows * cols, dtype=g.VAT)
        self.terms["out"] = np.repeat(np.arange(rows, dtype=np.int64) + ROW_OFFSET + 1, cols)
        self.terms["coeff"] = Cm.reshape(-1)
        self.terms["var"] = np.tile(node.vm_h[xv - 1], rows)
        self.out = g.Guarded(3 * rows * cols, shift=shift)
        self.consts = g.Guarded(rows, doubles=True) if has_consts else None

    def want_consts(self, d=None):
        d = self.d_h if d is None else d
        if d is None or self.sign == 0:
            return np.zeros(self.rows)
        return (0.0 + d) if self.sign > 0 else (0.0 - d)

    def record(self, g, stream, b=None):
        """b: a device pointer to read the constants' vector from instead of the pack's own d"""
        g.call("pmt_affine_pack_vector_f64", g.ptr(self.dC), self.lda, self.rows, self.cols, g.ptr(self.xvar), b or g.ptr(self.dd), self.sign,
               g.ptr(self.vm), ROW_OFFSET, self.out.ptr(), self.consts.ptr() if self.consts else None, stream)

    def guarded(self):
        return [self.out] + ([self.consts] if self.consts else [])

    def check(self, what, d=None):
        self.out.check(self.terms.view(np.int64), what + ": the pack's terms")
        if self.consts:
            self.consts.check(self.want_consts(d), what + ": the pack's constants")


def _poison(g, parts):
    for p in parts:
        for buf in p.guarded():
            buf.buf.fill_(float("nan") if buf.doubles else g.POISON_WORD)
    torch.cuda.synchronize()


def _images(parts):
    torch.cuda.synchronize()
    return [buf.buf.cpu().numpy().tobytes() for p in parts for buf in p.guarded()]


@pytest.fixture(scope="module")
def node():
    import gpu_util as g
    g.lib()
    return Node()


# rows, cols, options of the pack
CASES = [
    ("64x128", 64, 128, {}),                                  # full tiles, both vector paths
    ("40x200-ragged", 40, 200, {}),                           # ragged rows and columns, even cols
    ("33x129-odd-cols", 33, 129, {}),                         # odd cols: the 8-byte store path
    ("64x128-odd-lda", 64, 128, {"pad": 1}),                  # the scalar load path
    ("64x128-shifted-out", 64, 128, {"shift": 1}),            # an output one word behind a 16-byte boundary
    ("64x128-plus", 64, 128, {"sign": 1}),
    ("64x128-minus", 64, 128, {"sign": -1}),
    ("64x128-sign0", 64, 128, {"sign": 0}),
    ("64x128-no-b", 64, 128, {"has_b": False}),
    ("64x128-no-consts", 64, 128, {"has_consts": False}),
    ("1x64-one-tile", 1, 64, {}),                             # fewer tiles than workgroups that run dry
    ("512x1024", 512, 1024, {}),                              # hundreds of tiles: every dry workgroup loops
    ("66x32726-64-row-tiles-cold", 66, 32726, {}),            # 1024 tiles: 64-row tiles, nontemporal loads, the three-store row pairs
    ("66x32726-64-row-tiles-cold-odd-lda", 66, 32726, {"pad": 1}),   # ... over the scalar load path
]


@pytest.mark.parametrize("name,rows,cols,opts", CASES, ids=[c[0] for c in CASES])
def test_a_pack_behind_the_node_rides_and_gives_the_stand_alone_bytes(node, name, rows, cols, opts):
    import gpu_util as g
    pack = Pack(node, rows, cols, seed=rows * 1000 + cols, **opts)
    plan = g.Plan()
    try:
        with plan:
            node.record(g, plan.rec)
            pack.record(g, plan.rec)
        assert _riders(g, plan) == (1, _tiles(rows, cols))
        assert plan.fused()[2] == 1, "the pack's entry has left the replay"
        _poison(g, [node, pack])
        plan.update()
        node.check("riders on")
        pack.check("riders on")
        plan.fusion(False)
        assert _riders(g, plan) == (0, 0) and plan.fused()[2] == 2
        _poison(g, [node, pack])
        plan.update()
        node.check("the tape as recorded")
        pack.check("the tape as recorded")
    finally:
        plan.close()


def test_a_node_on_the_masked_load_path_carries_riders_too():
    import gpu_util as g
    node = Node(pad=1, seed=3)
    pack = Pack(node, 40, 200, seed=5)
    plan = g.Plan()
    try:
        with plan:
            node.record(g, plan.rec)
            pack.record(g, plan.rec)
        assert _riders(g, plan) == (1, _tiles(40, 200))
        _poison(g, [node, pack])
        plan.update()
        node.check("odd pitch")
        pack.check("odd pitch")
    finally:
        plan.close()


def _three_riders_tape(g, node, plan):
    """a side-lane pack in front of the node, the node, a pack, a pack whose `b` is the node's out_lin buffer read as doubles, a pack"""
    front = Pack(node, 40, 200, seed=11)
    p1, p2 = Pack(node, 64, 128, seed=12), Pack(node, 33, 129, seed=13)
    dep = Pack(node, 48, 64, seed=14)
    with plan:
        g.call("pmt_plan_set_lane", plan.plan, 1)
        front.record(g, plan.rec)
        g.call("pmt_plan_set_lane", plan.plan, 0)
        node.record(g, plan.rec)
        p1.record(g, plan.rec)
        dep.record(g, plan.rec, b=node.out[1].ptr())
        p2.record(g, plan.rec)
    return front, p1, dep, p2


def test_three_riders_and_a_dependent_pack_that_stays(node):
    import gpu_util as g
    plan = g.Plan()
    try:
        front, p1, dep, p2 = _three_riders_tape(g, node, plan)
        parts = [node, front, p1, dep, p2]
        assert _riders(g, plan) == (3, _tiles(40, 200) + _tiles(64, 128) + _tiles(33, 129))
        assert plan.fused()[2] == 2, "the node with its riders, then the dependent pack"
        q_as_doubles = node.lin.view(np.float64)[:dep.rows]          # what the node writes this replay, read as the pack's d
        for mode in ("riders on", "the tape as recorded"):
            _poison(g, parts)
            plan.update()
            node.check(mode)
            for p in (front, p1, p2):
                p.check(mode)
            dep.check(mode, d=q_as_doubles)
            plan.fusion(False)
        assert _riders(g, plan) == (0, 0)
    finally:
        plan.close()


def test_twenty_replays_then_an_immediate_node_without_riders(node):
    import gpu_util as g
    pack = Pack(node, 512, 1024, seed=21)
    plan = g.Plan()
    try:
        with plan:
            node.record(g, plan.rec)
            pack.record(g, plan.rec)
        assert _riders(g, plan)[0] == 1
        first = None
        for k in range(20):
            _poison(g, [node, pack])
            plan.update()
            got = _images([node, pack])
            first = first or got
            assert got == first, "replay %d" % k
        node.check("the twentieth replay")
        pack.check("the twentieth replay")
        # the riders' ticket is re-armed with the others: an immediate call on the same stream — no plan, no riders — walks the same tickets
        _poison(g, [node, pack])
        node.record(g, C.c_void_p(g.lib().pmt_plan_stream(plan.plan)))
        node.check("an immediate call behind the replays")
        pack.out.check(pack.out.padding(pack.out.n), "an immediate node writes nothing of the pack")
    finally:
        plan.close()


def test_a_captured_graph_keeps_its_riders(node):
    import gpu_util as g
    pack = Pack(node, 40, 200, seed=31)
    plan = g.Plan()
    try:
        with plan:
            node.record(g, plan.rec)
            pack.record(g, plan.rec)
        _poison(g, [node, pack])
        plan.update()
        want = _images([node, pack])
        g.call("pmt_plan_instantiate_graph", plan.plan)
        assert _riders(g, plan) == (1, _tiles(40, 200))
        for k in range(2):
            _poison(g, [node, pack])
            plan.update()
            assert _images([node, pack]) == want, "graph replay %d" % k
        node.check("graph")
        pack.check("graph")
    finally:
        plan.close()


def test_two_plans_on_two_streams_each_get_what_they_get_alone():
    import gpu_util as g
    g.lib()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    nodes = [Node(seed=41), Node(seed=42)]
    packs = [Pack(nodes[0], 512, 1024, seed=43), Pack(nodes[1], 40, 200, seed=44)]
    torch.cuda.synchronize()
    plans = []
    try:
        for k in range(2):
            with torch.cuda.stream(streams[k]):
                plans.append(g.Plan())
                with plans[k]:
                    nodes[k].record(g, plans[k].rec)
                    packs[k].record(g, plans[k].rec)
            assert _riders(g, plans[k])[0] == 1
        alone = []
        for k in range(2):
            _poison(g, [nodes[k], packs[k]])
            plans[k].update()
            alone.append(_images([nodes[k], packs[k]]))
            nodes[k].check("alone")
            packs[k].check("alone")
        for i in range(6):
            _poison(g, nodes + packs)
            for k in range(2):
                plans[k].update()
            for k in range(2):
                assert _images([nodes[k], packs[k]]) == alone[k], "round %d, plan %d" % (i, k)
    finally:
        for p in plans:
            p.close()


def test_a_node_of_one_workgroup_per_item_takes_no_riders():
    import gpu_util as g
    node = Node(rows=64, n=512, seed=51)
    pack = Pack(node, 40, 200, seed=52)
    plan = g.Plan()
    try:
        with plan:
            node.record(g, plan.rec)
            pack.record(g, plan.rec)
        assert _riders(g, plan) == (0, 0)
        _poison(g, [node, pack])
        plan.update()
        node.check("64 x 512")
        pack.check("64 x 512")
    finally:
        plan.close()
