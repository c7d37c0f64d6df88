"""-m gpu: the persistent walk of the one-launch canonical objective node (csrc/gram_mid.hip: gram_mid_kernel with MidArgs::persist) at the
boundaries between two work items and between the node and the next tape entry (csrc/gram.hip: mid_node) — on the smallest shapes that
run persistent: 2112 columns are 33 panels, 528 + 33 + 1 = 562 work items at any row count (two full rounds of 256 plus the rest by ticket).

Exact data: A and b hold integers of [-3, 3], at most 320 rows, so every partial sum of a coefficient is an integer below 2^13 and the sums
are exact in float64 WHATEVER their order: Q = 2 A'A, q = 2 A'c and c'c must equal the int64 results bit for bit.  A group of rows that is
lost, read twice or read from another tile shows as a wrong integer.  Reference semantics: canonicalize(_vecdot!(residual, residual)) ->
update!(::MOI.ScalarQuadraticFunction), src/functions.jl:702-709,548-576,381-386 and src/moi_interop.jl:45-62."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

VARMAP_SHIFT = 5


def _order(rows, n):
    import gpu_util as g
    o = C.c_int()
    g.call("pmt_quad_gram_constant_order", rows, n, C.byref(o), None, None)
    return o.value


def _integer_data(rows, n, lda, seed):
    """device copies of an integer A (column-major with pitch lda, the padding poisoned with 1e300) and b, and their int64 originals"""
    import gpu_util as g
    rng = np.random.default_rng(seed)
    A = rng.integers(-3, 4, size=(rows, n), dtype=np.int64)
    b = rng.integers(-3, 4, size=rows, dtype=np.int64)
    buf = np.full(lda * n, 1e300)
    buf.reshape(n, lda)[:, :rows] = A.T
    return A, b, g.to_dev(buf), g.to_dev(b.astype(np.float64))


def _node(g, dA, lda, rows, n, xvar, db, vm, ws, stream, out=None):
    nq = n * (n + 1) // 2
    oq, ol, oc = out or (g.empty_terms(nq, g.QT), g.empty_terms(n, g.LT), g.empty_f64(1))
    g.call("pmt_quad_gram_f64", g.ptr(dA), lda, rows, n, g.ptr(xvar), g.ptr(db), -1, 1, g.ptr(vm), g.ptr(oq), g.ptr(ol), g.ptr(oc), g.ptr(ws), stream)
    return oq, ol, oc


def _bytes(g, out, n):
    oq, ol, oc = out
    return (g.terms_to_host(oq, n * (n + 1) // 2, g.QT).tobytes(), g.terms_to_host(ol, n, g.LT).tobytes(), g.f64_to_host(oc, 1).tobytes())


# (rows, columns, pad of the leading dimension)
EXACT = [
    (64, 2112, 0),          # two 8-row groups per wave: one round of the pipelined loop
    (96, 2112, 0),          # three: a leftover group behind the round
    (40, 2112, 0),          # waves with two groups and with one
    (60, 2112, 0),          # a ragged last group
    (64, 2100, 0),          # a ragged last column panel
    (256, 2112, 0),         # more than 4 MiB: the XCD-aware order and the super-tiles
    (320, 2112, 0),         # split tails and split diagonal tiles behind the unsplit body
    (128, 2304, 2),         # an even pad: the fast load path with a pitch that is not the row count
    (64, 2112, 1),          # an odd pitch: the masked load path
]


@pytest.mark.parametrize("rows,n,pad", EXACT)
def test_integer_data_gives_the_exact_integers(rows, n, pad):
    import gpu_util as g
    assert _order(rows, n) == 5, "the one-launch form did not take this shape"
    lda = rows + pad
    A, b, dA, db = _integer_data(rows, n, lda, rows * 7 + n + pad)
    xvar = g.to_dev(np.arange(1, n + 1, dtype=np.int64))
    vm_h = np.arange(1, n + 1, dtype=np.int64) + VARMAP_SHIFT
    ws = g.empty_f64(g.lib().pmt_quad_gram_workspace_bytes(rows, n) // 8)
    oq, ol, oc = _node(g, dA, lda, rows, n, xvar, db, g.to_dev(vm_h), ws, g.stream())
    nq = n * (n + 1) // 2
    q, l, const = g.terms_to_host(oq, nq, g.QT), g.terms_to_host(ol, n, g.LT), g.f64_to_host(oc, 1)
    c = -b
    assert 9 * rows < 2 ** 13                                          # |a| <= 3: no partial sum of a product of two entries leaves the integers
    At = torch.from_numpy(A)
    G = 2 * (At.T @ At).numpy()                                        # int64 on the CPU (torch's integer product: numpy's takes seconds here)
    iu = np.triu_indices(n)
    assert np.array_equal(q["row"], vm_h[iu[0]]) and np.array_equal(q["col"], vm_h[iu[1]])
    assert g.same_bits(q["coeff"], G[iu].astype(np.float64))
    assert np.array_equal(l["var"], vm_h)
    assert g.same_bits(l["coeff"], (2 * (A.T @ c)).astype(np.float64))
    assert const[0] == float(c @ c)


@pytest.mark.parametrize("rows,n", [(256, 2112), (320, 2112)])
def test_twenty_launches_in_a_row_give_the_same_bits(rows, n):
    """the tickets and the workgroups' leaving count re-arm themselves, whatever a workgroup still held when the items ran out"""
    import gpu_util as g
    assert _order(rows, n) == 5
    rng = np.random.default_rng(rows + n)
    dA, db = g.colmajor(rng.random((rows, n)) - 0.5), g.to_dev(rng.random(rows))
    xvar = g.to_dev(np.arange(1, n + 1, dtype=np.int64))
    ws = g.empty_f64(g.lib().pmt_quad_gram_workspace_bytes(rows, n) // 8)
    outs = [_node(g, dA, rows, rows, n, xvar, db, None, ws, g.stream()) for _ in range(20)]
    first = _bytes(g, outs[0], n)
    for out in outs[1:]:
        assert _bytes(g, out, n) == first


def test_two_streams_at_once_get_what_each_gets_alone():
    """two sets of 256 persistent workgroups share the CUs; tickets and arrival counts are the calling stream's"""
    import gpu_util as g
    rows, n = 256, 2112
    assert _order(rows, n) == 5
    rng = np.random.default_rng(11)
    nq = n * (n + 1) // 2
    data, alone = [], []
    for k in range(2):
        dA, db = g.colmajor(rng.random((rows, n)) - 0.5), g.to_dev(rng.random(rows))
        xvar = g.to_dev(np.arange(1, n + 1, dtype=np.int64))
        ws = g.empty_f64(g.lib().pmt_quad_gram_workspace_bytes(rows, n) // 8)
        data.append((dA, db, xvar, ws))
        alone.append(_bytes(g, _node(g, dA, rows, rows, n, xvar, db, None, ws, g.stream()), n))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    # (the poisoned output buffers are filled on torch's current stream: all of them exist, and the fills are done, before the two streams start)
    outs = [[(g.empty_terms(nq, g.QT), g.empty_terms(n, g.LT), g.empty_f64(1)) for _ in range(8)] for k in range(2)]
    torch.cuda.synchronize()
    for i in range(8):
        for k in range(2):
            dA, db, xvar, ws = data[k]
            _node(g, dA, rows, rows, n, xvar, db, None, ws, C.c_void_p(streams[k].cuda_stream), outs[k][i])
    torch.cuda.synchronize()
    for k in range(2):
        for out in outs[k]:
            assert _bytes(g, out, n) == alone[k]


def test_recorded_node_then_constraint_pack_replays_the_direct_calls():
    """config 2's tape in small — the node, then pmt_affine_pack_vector_f64 of a 32 x 2112 block, both on the plan's own lane: replayed
    three times with refreshed inputs, once more as a captured graph, and with the pack on the side lane (the node then forks the side
    stream behind itself, gram.hip: mid_node) the outputs are those of the direct calls, bit for bit"""
    import gpu_util as g
    rows, n, m = 256, 2112, 32
    assert _order(rows, n) == 5
    nq = n * (n + 1) // 2
    s = g.stream()
    dA, db, dC, dd = g.empty_f64(rows * n), g.empty_f64(rows), g.empty_f64(m * n), g.empty_f64(m)
    xvar = g.to_dev(np.arange(1, n + 1, dtype=np.int64))
    vm = g.to_dev(np.arange(1, n + 1, dtype=np.int64) + VARMAP_SHIFT)
    ws = g.empty_f64(g.lib().pmt_quad_gram_workspace_bytes(rows, n) // 8)

    def refresh(epoch):
        for buf, count, seed, scale in ((dA, rows * n, 1, 1.0), (db, rows, 2, 1.0), (dC, m * n, 3, 1.0), (dd, m, 4, 2.0)):
            g.call("pmt_fill_uniform_f64", g.ptr(buf), count, seed + 1000 * epoch, scale, s)

    def outputs():
        return (g.empty_terms(nq, g.QT), g.empty_terms(n, g.LT), g.empty_f64(1), g.empty_terms(m * n, g.VAT), g.empty_f64(m))

    def tape(out, stream, plan=None, side_lane=False):
        oq, ol, oc, vt, vc = out
        g.call("pmt_quad_gram_f64", g.ptr(dA), rows, rows, n, g.ptr(xvar), g.ptr(db), -1, 1, g.ptr(vm), g.ptr(oq), g.ptr(ol), g.ptr(oc), g.ptr(ws), stream)
        if side_lane:
            g.call("pmt_plan_set_lane", plan, 1)
        g.call("pmt_affine_pack_vector_f64", g.ptr(dC), m, m, n, g.ptr(xvar), g.ptr(dd), -1, g.ptr(vm), 0, g.ptr(vt), g.ptr(vc), stream)
        if side_lane:
            g.call("pmt_plan_set_lane", plan, 0)

    def host(out):
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy().tobytes() for t in out)

    def poison(out):
        for t in out[:2] + out[3:4]:
            t.fill_(g.POISON_WORD)
        for t in (out[2], out[4]):
            t.fill_(float("nan"))

    # the direct calls, epoch by epoch
    want = []
    direct = outputs()
    for epoch in range(5):
        refresh(epoch)
        poison(direct)
        tape(direct, s)
        want.append(host(direct))
    assert want[0] != want[1]

    plain, lane = g.Plan(), g.Plan()
    out_plain, out_lane = outputs(), outputs()
    try:
        with plain:
            tape(out_plain, plain.rec)
        with lane:
            tape(out_lane, lane.rec, lane.plan, side_lane=True)
        assert g.lib().pmt_plan_tape_length(plain.plan) == 2
        for epoch in range(3):
            refresh(epoch)
            poison(out_plain)
            plain.update()
            assert host(out_plain) == want[epoch], "replay %d of the node and the pack on one lane" % epoch
        g.call("pmt_plan_instantiate_graph", plain.plan)
        refresh(3)
        poison(out_plain)
        plain.update()
        assert host(out_plain) == want[3], "the same tape as a captured graph"
        for epoch in (4, 0):
            refresh(epoch)
            torch.cuda.synchronize()
            poison(out_lane)
            lane.update()
            assert host(out_lane) == want[epoch], "the pack on the side lane"
    finally:
        plain.close()
        lane.close()
