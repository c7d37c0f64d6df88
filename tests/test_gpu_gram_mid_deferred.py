"""-m gpu: the DEFERRED tiles of the one-launch canonical objective node (csrc/gram_mid.hip: MidWalk, the hand-off in mid_body, mid_wo_op).
An unsplit strictly upper tile of the persistent walk leaves its four waves' raw sums in LDS; they are added and written inside the
first rounds of the next tile's main loop, behind that loop where it is too short, or at once in front of anything that does not defer
(a ragged last panel, a workgroup's last body tile).  The launch takes the deferring build of the kernel only where tiles will be
deferred — rows a multiple of 64, 16-byte aligned operands with an even pitch; every other launch runs the build without deferred tiles,
which is the kernel as it was.  Every shape asserts pmt_quad_gram_mid_defers, so no case can pass on a plan that never defers; its second
result says which build a fast-path call of the shape runs.

Exact data as in test_gpu_gram_mid_items.py: A and b hold integers of [-3, 3] and at most 1024 rows, so every partial sum of a
coefficient is an integer below 2^14 and exact in float64 in ANY order: Q = 2 A'A, q = 2 A'c and c'c must equal the int64 results bit
for bit, and a row of a tile that is lost, written twice, taken from another wave's region or from the tile behind shows as a wrong
integer.  The outputs lie between poisoned guard words.  Reference semantics: canonicalize(_vecdot!(residual, residual)) ->
update!(::MOI.ScalarQuadraticFunction), src/functions.jl:702-709,548-576,381-386 and src/moi_interop.jl:45-62."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

VARMAP_SHIFT = 5


def _defers(rows, n):
    """(the one-launch form's plan defers tiles, the row count gives every wave whole rounds so that whole-panel body tiles ARE deferred)"""
    import gpu_util as g
    order, plan, whole = C.c_int(), C.c_int(), C.c_int()
    g.call("pmt_quad_gram_constant_order", rows, n, C.byref(order), None, None)
    g.call("pmt_quad_gram_mid_defers", rows, n, C.byref(plan), C.byref(whole))
    return order.value == 5 and plan.value == 1, whole.value == 1


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


# (rows, columns, pad of the leading dimension, the query's second result: rows a multiple of 64 — with an even pitch the call runs the
# deferring build and body tiles of whole panels are deferred; the query cannot see the pitch)
EXACT = [
    (64, 2112, 0, True),            # one round per item: a quarter of a tile's write-out inside it, the rest behind the loop
    (128, 2112, 0, True),           # two rounds: half inside, half behind
    (192, 2112, 0, True),           # three rounds: three quarters inside
    (1024, 2112, 0, True),          # 16 rounds: the write-out inside the first four, then the loop as it was
    (96, 2112, 0, False),           # a leftover group behind the rounds: the build without deferred tiles
    (60, 2112, 0, False),           # a ragged group: the same build
    (64, 2100, 0, True),            # the deferring build with a ragged last panel: its tiles and the tiles in front of them take the immediate
                                    # path inside it, and a pending tile is written out in front of the first of them
    (128, 2304, 2, True),           # an even pad: deferred, with a pitch that is not the row count
    (64, 2112, 1, True),            # an odd pitch: the query says yes by the rows, the call runs the masked build, which never defers
]


@pytest.mark.parametrize("rows,n,pad,whole", EXACT)
def test_integer_data_gives_the_exact_integers_between_poisoned_guards(rows, n, pad, whole):
    import gpu_util as g
    assert _defers(rows, n) == (True, whole), "the plan of this shape does not defer as the case expects"
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


def _bytes(g, out, n):
    oq, ol, oc = out
    return (g.terms_to_host(oq, n * (n + 1) // 2, g.QT).tobytes(), g.terms_to_host(ol, n, g.LT).tobytes(), g.f64_to_host(oc, 1).tobytes())


def test_twenty_launches_in_a_row_give_the_same_bits():
    """a launch starts while the one before it still writes its last deferred tiles; nothing of a walk outlives it"""
    import gpu_util as g
    rows, n = 128, 2112
    assert _defers(rows, n) == (True, True)
    data = _random_node(g, rows, n, 5)
    outs = [_launch(g, data, rows, n, g.stream()) for _ in range(20)]
    first = _bytes(g, outs[0], n)
    for out in outs[1:]:
        assert _bytes(g, out, n) == first


def test_two_streams_at_once_get_what_each_gets_alone():
    import gpu_util as g
    rows, n = 128, 2112
    assert _defers(rows, n) == (True, True)
    nq = n * (n + 1) // 2
    data = [_random_node(g, rows, n, 21 + k) for k in range(2)]
    alone = [_bytes(g, _launch(g, data[k], rows, n, g.stream()), n) for k in range(2)]
    assert alone[0] != alone[1]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [[(g.empty_terms(nq, g.QT), g.empty_terms(n, g.LT), g.empty_f64(1)) for _ in range(6)] for k in range(2)]
    torch.cuda.synchronize()                                           # the poison fills are done before the two streams start
    for i in range(6):
        for k in range(2):
            _launch(g, data[k], rows, n, C.c_void_p(streams[k].cuda_stream), outs[k][i])
    torch.cuda.synchronize()
    for k in range(2):
        for out in outs[k]:
            assert _bytes(g, out, n) == alone[k]


def test_a_constraint_pack_riding_in_the_node_changes_no_byte():
    """256 x 2112 with a 64-row constraint block recorded behind the node: its tiles ride in the deferring build's launch, drawn by
    workgroups whose items have run out and written to the front of the LDS that held deferred partials a few items earlier (nothing is
    pending by then: a workgroup's last body tile does not defer).  The bytes are those of the same tape with
    pmt_plan_set_fusion(plan, 0), where the pack is a launch of its own."""
    import gpu_util as g
    rows, n, m = 256, 2112, 64
    assert _defers(rows, n) == (True, True)
    nq = n * (n + 1) // 2
    rng = np.random.default_rng(77)
    dA, db = g.colmajor(rng.random((rows, n)) - 0.5), g.to_dev(rng.random(rows))
    dC, dd = g.colmajor(rng.random((m, n)) - 0.5), g.to_dev(rng.random(m))
    xvar = g.to_dev(np.arange(1, n + 1, dtype=np.int64))
    vm = g.to_dev(np.arange(1, n + 1, dtype=np.int64) + VARMAP_SHIFT)
    ws = g.empty_f64(g.lib().pmt_quad_gram_workspace_bytes(rows, n) // 8)
    out = (g.empty_terms(nq, g.QT), g.empty_terms(n, g.LT), g.empty_f64(1), g.empty_terms(m * n, g.VAT), g.empty_f64(m))

    def host():
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy().tobytes() for t in out)

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
        riding = host()
        plan.fusion(False)
        g.call("pmt_plan_riders", plan.plan, C.byref(nr), C.byref(nt))
        assert (nr.value, nt.value) == (0, 0)
        poison()
        plan.update()
        assert host() == riding
    finally:
        plan.close()
