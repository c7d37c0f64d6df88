"""-m gpu: the STRIPS of the one-launch canonical objective node (csrc/gram_mid.hip: mid_strips, mid_so_op).  On a shape of many body tiles
a workgroup takes four consecutive strictly upper tiles of the walk at a time and each of its four waves owns one WHOLE tile: all 8-row
groups of the matrix, no sum across waves, the tile left in the wave's own region of LDS and written inside the first rounds of the
wave's next loop, behind that loop where it is too short, or at once behind a workgroup's last strip.  The body tiles that fill no strip,
the diagonal tiles with q, and c'c run the items they always ran, behind the strips.  The launch takes the strip build only where the
shape's plan has strips (pmt_quad_gram_mid_strips: whole 64-column panels, rows a multiple of 64, at least 1.5 strips per workgroup) and
the call is on the fast load path (16-byte aligned operands, an even pitch).  Every case asserts the query first, so none can pass on a
plan without strips.

Exact data as in test_gpu_gram_mid_deferred.py: A and b hold integers of [-3, 3] and at most 1024 rows, so every partial sum of a
coefficient is an integer below 2^14 and exact in float64 in ANY order: Q = 2 A'A, q = 2 A'c and c'c must equal the int64 results bit
for bit, and a row of a tile that is lost, written twice, taken from another wave's region or from the strip behind shows as a wrong
integer.  The outputs lie between poisoned guard words.  Reference semantics: canonicalize(_vecdot!(residual, residual)) ->
update!(::MOI.ScalarQuadraticFunction), src/functions.jl:702-709,548-576,381-386 and src/moi_interop.jl:45-62."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

VARMAP_SHIFT = 5


def _strips(rows, n):
    """(strips, tiles in strips) of the shape's plan; (0, 0): no strips"""
    import gpu_util as g
    order, strips, tiles = C.c_int(), C.c_int(), C.c_int()
    g.call("pmt_quad_gram_constant_order", rows, n, C.byref(order), None, None)
    assert order.value == 5, "not a shape of the one-launch form"
    g.call("pmt_quad_gram_mid_strips", rows, n, C.byref(strips), C.byref(tiles))
    return strips.value, tiles.value


def _integer_data(rows, n, lda, seed):
    import gpu_util as g
    rng = np.random.default_rng(seed)
    A = rng.integers(-3, 4, size=(rows, n), dtype=np.int64)
    b = rng.integers(-3, 4, size=rows, dtype=np.int64)
    buf = np.full(lda * n, 1e300)                                      # the padding of the leading dimension is poisoned
    buf.reshape(n, lda)[:, :rows] = A.T
    return A, b, g.to_dev(buf), g.to_dev(b.astype(np.float64))


def _expected(g, A, b, vm_h):
    n = A.shape[1]
    c = -b
    At = torch.from_numpy(A)
    G = 2 * (At.T @ At).numpy()                                        # int64 on the CPU
    iu = np.triu_indices(n)
    q = np.empty(len(iu[0]), dtype=g.QT)
    q["coeff"], q["row"], q["col"] = G[iu].astype(np.float64), vm_h[iu[0]], vm_h[iu[1]]
    l = np.empty(n, dtype=g.LT)
    l["coeff"], l["var"] = (2 * (A.T @ c)).astype(np.float64), vm_h
    return q, l, np.array([float(c @ c)])


def _node(g, dA, lda, rows, n, xvar, db, vm, ws, stream, oq, ol, oc):
    g.call("pmt_quad_gram_f64", g.ptr(dA), lda, rows, n, g.ptr(xvar), g.ptr(db), -1, 1, g.ptr(vm), oq, ol, oc, g.ptr(ws), stream)


# (rows, columns, pad of the leading dimension, (strips, tiles in strips) the query must report — it sees the shape, not the pitch)
EXACT = [
    (64, 4096, 0, (504, 2016)),         # four rounds per wave and strip: an eighth of a tile's write-out inside the loop, the rest behind it
    (256, 4096, 0, (504, 2016)),        # sixteen rounds: the write-out fills the whole loop
    (1024, 4096, 2, (504, 2016)),       # the write-out inside the first 16 of 64 rounds, then the steady loop; a pitch that is not the row count
    (128, 4032, 0, (488, 1952)),        # 1953 body tiles = 488 strips + one tile that stays an item of its own behind them
    (64, 3776, 0, (427, 1708)),         # 1711 body tiles = 427 strips + THREE tiles behind them, in a matrix that fits one L2 (the ids are not
    (128, 3776, 0, (427, 1708)),        # numbered XCD-major there): the tiles behind the strips are the last ranks of the SAME walk the strips took
    (64, 4090, 0, (0, 0)),              # a ragged last panel: no strips, the result is still exact
    (64, 4096, 1, (504, 2016)),         # an odd pitch: strips by the shape, but the call runs the masked build, which has none
    (96, 4096, 0, (0, 0)),              # rows that are no multiple of 64: no strips
]


@pytest.mark.parametrize("rows,n,pad,strips", EXACT)
def test_integer_data_gives_the_exact_integers_between_poisoned_guards(rows, n, pad, strips):
    import gpu_util as g
    assert _strips(rows, n) == strips, "the plan of this shape does not take strips as the case expects"
    assert 9 * rows < 2 ** 14                                          # |a| <= 3: no partial sum of products leaves the integers
    lda = rows + pad
    A, b, dA, db = _integer_data(rows, n, lda, rows * 7 + n + pad)
    xvar = g.to_dev(np.arange(1, n + 1, dtype=np.int64))
    vm_h = np.arange(1, n + 1, dtype=np.int64) + VARMAP_SHIFT
    ws = g.empty_f64(g.lib().pmt_quad_gram_workspace_bytes(rows, n) // 8)
    nq = n * (n + 1) // 2
    oq, ol, oc = g.Guarded(3 * nq), g.Guarded(2 * n), g.Guarded(1, doubles=True)
    _node(g, dA, lda, rows, n, xvar, db, g.to_dev(vm_h), ws, g.stream(), oq.ptr(), ol.ptr(), oc.ptr())
    q, l, const = _expected(g, A, b, vm_h)
    oq.check(q.view(np.int64), "quadratic terms")
    ol.check(l.view(np.int64), "linear terms")
    oc.check(const, "constant")


def _random_node(g, rows, n, seed):
    rng = np.random.default_rng(seed)
    dA, db = g.colmajor(rng.random((rows, n)) - 0.5), g.to_dev(rng.random(rows))
    xvar = g.to_dev(np.arange(1, n + 1, dtype=np.int64))
    ws = g.empty_f64(g.lib().pmt_quad_gram_workspace_bytes(rows, n) // 8)
    return dA, db, xvar, ws


def _launch(g, data, rows, n, stream, out=None):
    dA, db, xvar, ws = data
    oq, ol, oc = out or (g.empty_terms(n * (n + 1) // 2, g.QT), g.empty_terms(n, g.LT), g.empty_f64(1))
    _node(g, dA, rows, rows, n, xvar, db, None, ws, stream, g.ptr(oq), g.ptr(ol), g.ptr(oc))
    return oq, ol, oc


def _same(outs_a, outs_b):
    return all(torch.equal(a, b) for a, b in zip(outs_a, outs_b))


def test_twenty_launches_in_a_row_give_the_same_bits():
    """a launch starts while the one before it still writes its last tiles; nothing of a walk outlives it"""
    import gpu_util as g
    rows, n = 128, 4096
    assert _strips(rows, n) == (504, 2016)
    data = _random_node(g, rows, n, 5)
    outs = [_launch(g, data, rows, n, g.stream()) for _ in range(20)]
    torch.cuda.synchronize()
    assert not bool(torch.any(outs[0][0].view(torch.int64) == g.POISON_WORD))          # every word was written
    for out in outs[1:]:
        assert _same(out, outs[0])


def test_two_streams_at_once_get_what_each_gets_alone():
    import gpu_util as g
    rows, n = 128, 4096
    assert _strips(rows, n) == (504, 2016)
    nq = n * (n + 1) // 2
    data = [_random_node(g, rows, n, 21 + k) for k in range(2)]
    alone = [_launch(g, data[k], rows, n, g.stream()) for k in range(2)]
    torch.cuda.synchronize()
    assert not _same(alone[0], alone[1])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [[(g.empty_terms(nq, g.QT), g.empty_terms(n, g.LT), g.empty_f64(1)) for _ in range(3)] for k in range(2)]
    torch.cuda.synchronize()                                           # the poison fills are done before the two streams start
    for i in range(3):
        for k in range(2):
            _launch(g, data[k], rows, n, C.c_void_p(streams[k].cuda_stream), outs[k][i])
    torch.cuda.synchronize()
    for k in range(2):
        for out in outs[k]:
            assert _same(out, alone[k])


def test_a_constraint_pack_riding_in_the_node_changes_no_byte():
    """256 x 4096 with a 64-row constraint block recorded behind the node: its tiles ride in the strip build's launch, drawn by workgroups
    whose items have run out and written to the front of the LDS that held the waves' tiles a strip earlier (nothing is pending by then:
    a workgroup's last strip writes its tiles at once).  The bytes are those of the same tape with pmt_plan_set_fusion(plan, 0), where
    the pack is a launch of its own."""
    import gpu_util as g
    rows, n, m = 256, 4096, 64
    assert _strips(rows, n) == (504, 2016)
    nq = n * (n + 1) // 2
    rng = np.random.default_rng(77)
    dA, db = g.colmajor(rng.random((rows, n)) - 0.5), g.to_dev(rng.random(rows))
    dC, dd = g.colmajor(rng.random((m, n)) - 0.5), g.to_dev(rng.random(m))
    xvar = g.to_dev(np.arange(1, n + 1, dtype=np.int64))
    vm = g.to_dev(np.arange(1, n + 1, dtype=np.int64) + VARMAP_SHIFT)
    ws = g.empty_f64(g.lib().pmt_quad_gram_workspace_bytes(rows, n) // 8)
    out = (g.empty_terms(nq, g.QT), g.empty_terms(n, g.LT), g.empty_f64(1), g.empty_terms(m * n, g.VAT), g.empty_f64(m))

    def snapshot():
        torch.cuda.synchronize()
        return tuple(t.clone() for t in out)

    def poison():
        for t in out:
            t.fill_(g.POISON_WORD) if t.dtype == torch.int64 else t.fill_(float("nan"))

    plan = g.Plan()
    try:
        with plan:
            g.call("pmt_quad_gram_f64", g.ptr(dA), rows, rows, n, g.ptr(xvar), g.ptr(db), -1, 1, g.ptr(vm), g.ptr(out[0]), g.ptr(out[1]), g.ptr(out[2]), g.ptr(ws), plan.rec)
            g.call("pmt_affine_pack_vector_f64", g.ptr(dC), m, m, n, g.ptr(xvar), g.ptr(dd), -1, g.ptr(vm), 0, g.ptr(out[3]), g.ptr(out[4]), plan.rec)
        nr, nt = C.c_int(-1), C.c_int64(-1)
        g.call("pmt_plan_riders", plan.plan, C.byref(nr), C.byref(nt))
        assert nr.value == 1 and nt.value > 0, "the pack does not ride in the node"
        poison()
        plan.update()
        riding = snapshot()
        for t in riding[:1] + riding[3:4]:
            assert not bool(torch.any(t.view(torch.int64) == g.POISON_WORD))          # every term word was written
        plan.fusion(False)
        g.call("pmt_plan_riders", plan.plan, C.byref(nr), C.byref(nt))
        assert (nr.value, nt.value) == (0, 0)
        poison()
        plan.update()
        alone = snapshot()
        for a, b in zip(riding, alone):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    finally:
        plan.close()


def test_the_workspace_guard_stays_untouched():
    """pmt_quad_gram_workspace_bytes is what the node may write: a guard band behind it stays untouched (the items behind the strips keep
    the workspace slots they always had)"""
    import gpu_util as g
    rows, n = 128, 4096
    assert _strips(rows, n) == (504, 2016)
    rng = np.random.default_rng(9)
    nbytes = g.lib().pmt_quad_gram_workspace_bytes(rows, n)
    guard = 4096
    buf = torch.full((nbytes // 8 + guard,), 7.25, dtype=torch.float64, device="cuda")
    dA, db = g.colmajor(rng.random((rows, n))), g.to_dev(rng.random(rows))
    xvar = g.to_dev(np.arange(1, n + 1, dtype=np.int64))
    oq, ol, oc = g.empty_terms(n * (n + 1) // 2, g.QT), g.empty_terms(n, g.LT), g.empty_f64(1)
    _node(g, dA, rows, rows, n, xvar, db, None, buf, g.stream(), g.ptr(oq), g.ptr(ol), g.ptr(oc))
    torch.cuda.synchronize()
    assert bool(torch.all(buf[nbytes // 8:] == 7.25))
