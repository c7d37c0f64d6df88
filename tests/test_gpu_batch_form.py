"""-m gpu: the batched tracking-cost entry point pmt_batch_form_coeffs_f64 (csrc/batch_form.hip) and its host class batch.BatchTracking.

Every output lies inside a guarded buffer whose WHOLE image is compared bit for bit with the numpy restatement of the header's order
(tests/batch_form_util.py; tests/test_batch_form_host.py checks that restatement against the oracle and against Python integers): guards in
front and behind and the out_stride - L words between two slabs must still hold the poison.  The data has full mantissas, mixed magnitudes,
zeros of both signs and pairs Q[j,k] = -Q[k,j], so a sum taken in another order, a neighbour's entry or a dropped sign of zero differs.
Beside the restatement: the slab of an instance expands (pmt_batch_expand_f64) to the words pmt_quad_form_shift_f64 / pmt_quad_form_f64 write
for that instance alone.  Every size used is valid; nothing here provokes a fault."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import batch_form_util as F  # noqa: E402
import batch_util as BU  # noqa: E402
from test_gpu_batch_slabs import cus, dev_f64, image, owned  # noqa: E402

NAME = "pmt_batch_form_coeffs_f64"
TILE_EDGES = [1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256]
MS = [0, 1, 16, 33, 70]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


class FormBatch:
    """a batch in the device layout, on the host and on the device; the restatement is computed once per sign pair"""

    def __init__(self, B, n, m, seed, gen=F.mixed, q_shift=0):
        self.B, self.n, self.m = B, n, m
        self.host = list(F.form_data(B, n, m, np.random.default_rng(seed), gen))
        self.upload(q_shift)

    def upload(self, q_shift=0):
        self.dev = [dev_f64(self.host[0], q_shift)] + [dev_f64(h) for h in self.host[1:]]
        self.refs = {}

    def reference(self, sign_p, sign_d):
        key = (sign_p, sign_d)
        if key not in self.refs:
            self.refs[key] = F.form_slab_reference(*self.host, sign_p, sign_d)
        return self.refs[key].copy()

    def run(self, sign_p=-1, sign_d=-1, gap=0, shift=0, null_p=False):
        """-> (Guarded output of B * out_stride doubles, out_stride)"""
        import gpu_util as g
        L = BU.slab_doubles(self.n, self.m)
        assert L == g.lib().pmt_batch_lsq_slab_doubles(self.n, self.m)
        stride = L + gap
        out = g.Guarded(self.B * stride, doubles=True, shift=shift)
        g.call(NAME, self.dev[0][1], None if null_p else self.dev[1][1], self.dev[2][1], self.dev[3][1], self.B, self.n, self.m, sign_p, sign_d,
               out.ptr(), stride, g.stream())
        return out, stride

    def check(self, sign_p=-1, sign_d=-1, gap=0, shift=0, null_p=False, what=""):
        out, stride = self.run(sign_p, sign_d, gap, shift, null_p)
        out.check(image(out, self.reference(sign_p, sign_d), stride),
                  "%s n=%d m=%d B=%d signs (%d, %d) gap %d shift %d" % (what, self.n, self.m, self.B, sign_p, sign_d, gap, shift))


@functools.lru_cache(maxsize=4)
def batch(B, n, m):
    return FormBatch(B, n, m, seed=11 + 1000 * n + m)


def b_many():
    return 3 * cus() + 37                       # three workgroups a CU are resident: every workgroup gets a second instance, 37 a third .. or none


# ---- a. bit for bit against the restatement, at the tile edges

@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", TILE_EDGES)
def test_slabs_are_the_restatement_bit_for_bit(n, m):
    """out_stride = L with both signs -1 on a 16-byte aligned base; out_stride = L + 3 with both signs +1, the base 8 bytes off (with an odd
    pitch every second slab then starts on a 16-byte boundary, the others 8 bytes behind one)"""
    bt = batch(5, n, m)
    bt.check(-1, -1, gap=0, shift=0, what="tile edges")
    bt.check(1, 1, gap=3, shift=1, what="tile edges")


def test_Q_eight_bytes_off_a_16_byte_boundary():
    bt = FormBatch(5, 129, 16, seed=3, q_shift=1)
    assert bt.dev[0][1].value % 16 == 8
    bt.check(-1, 1, gap=3, what="shifted Q")
    bt.check(0, -1, gap=0, shift=1, null_p=True, what="shifted Q, plain form")


# ---- b. more instances than resident workgroups

def test_more_instances_than_resident_workgroups():
    B = b_many()
    assert B > 3 * cus() and (cus() != 256 or B == 3 * 256 + 37)
    bt = FormBatch(B, 8, 1, seed=5)
    bt.check(-1, -1, gap=0, what="persistent loop")
    bt.check(1, 0, gap=3, shift=1, what="persistent loop")
    out, stride = bt.run()
    last = owned(out).reshape(B, stride)[B - 1]
    alone = FormBatch(1, 8, 1, seed=0)
    alone.host = [np.ascontiguousarray(h[B - 1:B]) for h in bt.host]
    alone.upload()
    o1, _ = alone.run()
    o1.check(last, "the last instance alone")


# ---- c. equality with the single-instance nodes

@pytest.mark.parametrize("n", [65, 128, 200])
def test_expanded_slab_equals_the_single_instance_nodes(n):
    """pmt_batch_expand_f64 on an instance's slab against pmt_quad_form_shift_f64 (moi = 1, the same xvar and varmap) for both signs and
    pmt_quad_form_f64 with out_lin / out_const for sign_p == 0 (p passed as NULL): quadratic terms, linear terms and the constant word for word"""
    import gpu_util as g
    B, m = 3, 0
    bt = batch(B, n, m)
    rng = np.random.default_rng(n)
    nvars = n + 9
    xvar = np.sort(rng.choice(np.arange(1, nvars + 1), n, replace=False)).astype(np.int64)
    varmap = (rng.permutation(nvars) + 1 + 100).astype(np.int64)
    d_x, d_map = g.to_dev(xvar), g.to_dev(varmap)
    nq = n * (n + 1) // 2
    ws = g.empty_f64(g.lib().pmt_quad_form_shift_workspace_bytes(n) // 8)
    for sign_p in (-1, 1, 0):
        out, stride = bt.run(sign_p, -1, gap=3, null_p=(sign_p == 0))
        torch.cuda.synchronize()
        for i in range(B):
            slab = C.c_void_p(out.ptr().value + 8 * i * stride)
            oq, ol, oc = g.Guarded(3 * nq), g.Guarded(2 * n), g.Guarded(1, doubles=True)
            g.call("pmt_batch_expand_f64", slab, n, m, g.ptr(d_x), g.ptr(d_map), oq.ptr(), ol.ptr(), oc.ptr(), None, None, g.stream())
            sq, sl, sc = g.empty_terms(nq, g.QT), g.empty_terms(n, g.LT), g.empty_f64(1)
            Qi = C.c_void_p(bt.dev[0][1].value + 8 * i * n * n)
            if sign_p:
                pi = C.c_void_p(bt.dev[1][1].value + 8 * i * n)
                g.call("pmt_quad_form_shift_f64", Qi, n, n, g.ptr(d_x), pi, sign_p, 1, g.ptr(d_map), 1.0, g.ptr(sq), None, g.ptr(sl), g.ptr(sc), g.ptr(ws), g.stream())
            else:
                g.call("pmt_quad_form_f64", Qi, n, n, g.ptr(d_x), 1, g.ptr(d_map), 1.0, g.ptr(sq), None, g.ptr(sl), g.ptr(sc), g.stream())
            tag = "n=%d instance %d sign %d" % (n, i, sign_p)
            oq.check(g.terms_to_host(sq, nq, g.QT).view(np.int64), "quadratic terms " + tag)
            ol.check(g.terms_to_host(sl, n, g.LT).view(np.int64), "linear terms " + tag)
            oc.check(g.f64_to_host(sc, 1), "constant " + tag)


# ---- d. the two signs are two arguments

@pytest.mark.parametrize("sign_d", [-1, 0, 1])
@pytest.mark.parametrize("sign_p", [-1, 0, 1])
@pytest.mark.parametrize("n,m", [(100, 5), (129, 33)])
def test_all_sign_pairs(n, m, sign_p, sign_d):
    bt = batch(5, n, m)
    want = bt.reference(sign_p, sign_d)
    sec = BU.sections(n, m)
    zero = bits(np.zeros(1))[0]
    if sign_p == 0:
        assert np.all(bits(want[:, sec["q"]]) == zero) and np.all(bits(want[:, sec["const"]]) == zero)
    else:
        assert np.any(want[:, sec["q"]] != 0) and np.all(want[:, sec["const"]] != 0)
    if sign_d == 0:
        assert np.all(bits(want[:, sec["d"]]) == zero)
    bt.check(sign_p, sign_d, gap=1, what="signs")
    if sign_p == 0:
        bt.check(sign_p, sign_d, gap=1, null_p=True, what="signs, p NULL")


# ---- e. edge cases, each a complete slab

def test_instances_without_variables_or_without_a_constraint_block():
    FormBatch(4, 0, 3, seed=9).check(-1, 1, gap=2, what="n == 0")                 # [+0.0 | d-consts]
    FormBatch(4, 0, 0, seed=9).check(-1, -1, gap=0, what="n == 0, m == 0")        # [+0.0]
    FormBatch(4, 0, 0, seed=9).check(1, 1, gap=1, shift=1, what="n == 0, m == 0")
    FormBatch(1, 1, 0, seed=9).check(-1, -1, what="L = 3, the smallest slab with a variable")
    # an empty batch: nothing is written
    import gpu_util as g
    out = g.Guarded(8, doubles=True)
    g.call(NAME, None, None, None, None, 0, 4, 2, -1, -1, out.ptr(), BU.slab_doubles(4, 2), g.stream())
    out.check(out.padding(8), "B == 0")


# ---- f. instances do not see each other

def _isolation(B, n, m, victims, seed):
    bt = FormBatch(B, n, m, seed=seed)
    clean, stride = bt.run(-1, 1, gap=1)
    want = bt.reference(-1, 1)
    clean.check(image(clean, want, stride), "clean run")
    sec = BU.sections(n, m)
    for which in (0, 1):                                                        # NaN in Q, then (separately) in p
        saved = bt.host[which].copy()
        for v in victims:
            bt.host[which][v].reshape(-1)[(7 * v + 3) % bt.host[which][v].size] = np.nan
        bt.upload()
        out, stride = bt.run(-1, 1, gap=1)
        got = owned(out).reshape(B, stride)
        expect = want.copy()
        for v in victims:
            head = got[v, :sec["C"].start]
            assert np.isnan(head).any(), "instance %d: the NaN did not reach its slab" % v
            if which == 1:                                                      # p does not enter the Q section
                assert np.array_equal(bits(head[sec["Q"]]), bits(want[v, sec["Q"]]))
                assert np.isnan(head[sec["const"]]).all()
            expect[v, :sec["C"].start] = head                                   # C and the d-consts of the victim stay as they were
        out.check(image(out, expect, stride), "NaN in %s of instances %r" % ("Qp"[which], victims))
        bt.host[which] = saved
    bt.upload()


def test_nan_in_one_instance_stays_in_its_slab():
    _isolation(7, 129, 5, [3], seed=21)


def test_nan_stays_in_its_slab_on_a_shared_workgroup():
    """instances v - G, v and v + G run on one persistent workgroup, one after the other, through the same LDS"""
    B, G = b_many(), 3 * cus()
    _isolation(B, 8, 1, [5 + G, B - 1], seed=22)


# ---- g. position independence

@pytest.mark.parametrize("n,m,many", [(130, 3, False), (8, 1, True)])
def test_a_slab_does_not_depend_on_the_instance_s_position(n, m, many):
    B = b_many() if many else 6
    bt = FormBatch(B, n, m, seed=33 + n)
    for h in bt.host:
        h[1] = h[0]
        h[B - 1] = h[0]
    bt.upload()
    out, stride = bt.run(gap=3)
    out.check(image(out, bt.reference(-1, -1), stride), "in place")
    got = owned(out).reshape(B, stride)
    L = BU.slab_doubles(n, m)
    assert np.array_equal(bits(got[0, :L]), bits(got[1, :L])) and np.array_equal(bits(got[0, :L]), bits(got[B - 1, :L]))
    alone = FormBatch(1, n, m, seed=0)
    alone.host = [np.ascontiguousarray(h[:1]) for h in bt.host]
    alone.upload()
    o1, _ = alone.run()
    o1.check(got[0, :L], "the instance alone against in place")


# ---- h. batch.BatchTracking

def _fetch(wl):
    B, n, m = wl.B, wl.n, wl.m
    return (wl.Q.cpu().numpy().reshape(B, n, n), wl.p.cpu().numpy().reshape(B, n), wl.Cm.cpu().numpy().reshape(B, n, m), wl.d.cpu().numpy().reshape(B, m))


def test_batch_tracking_compute_equals_the_restatement_on_its_inputs():
    from oracle import oracle as O
    from parametron_jl_amd import batch as PB
    total, n, m = 6, 70, 3
    wl = PB.BatchTracking(torch, total, n, m)
    off, L = PB.slab_layout(n, m)
    assert (wl.offsets, wl.L, wl.lo, wl.hi, wl.B) == (off, L, 0, total, total) and wl.local.shape == (total, L) and wl.gathered is wl.local
    assert set(PB.BatchTracking.SEEDS.values()).isdisjoint(PB.BatchLSQ.SEEDS.values())
    wl.local.fill_(float("nan"))
    wl.compute()
    torch.cuda.synchronize()
    Qt, p, Ct, d = _fetch(wl)
    assert np.array_equal(bits(Qt.reshape(-1)), bits(O.fill_uniform(total * n * n, PB.BatchTracking.SEEDS["Q"])))
    assert np.array_equal(bits(d.reshape(-1)), bits(O.fill_uniform(total * m, PB.BatchTracking.SEEDS["d"], 2.0)))
    assert np.array_equal(bits(wl.local.cpu().numpy()), bits(F.form_slab_reference(Qt, p, Ct, d, -1, -1)))
    # another epoch: other data, the same relation
    wl.regenerate(1)
    wl.step(None)
    torch.cuda.synchronize()
    Q1 = wl.Q.cpu().numpy()
    assert not np.array_equal(Q1, Qt.reshape(-1)) and np.array_equal(bits(Q1), bits(O.fill_uniform(total * n * n, PB.BatchTracking.SEEDS["Q"] + 1000)))
    assert np.array_equal(bits(wl.local.cpu().numpy()), bits(F.form_slab_reference(*_fetch(wl), -1, -1)))
    assert wl.gathered is wl.local


def test_batch_tracking_sharding_is_data_independent():
    from parametron_jl_amd import batch as PB
    total, n, m = 8, 128, 16
    whole = PB.BatchTracking(torch, total, n, m)
    whole.step(None)
    parts, inputs = [], []
    for rank in range(4):
        part = PB.BatchTracking(torch, total, n, m, rank=rank, world=4)
        assert (part.lo, part.hi, part.B) == (2 * rank, 2 * rank + 2, 2) and part.gathered.shape == (total, part.L) and part.local.shape == (2, part.L)
        part.compute()
        parts.append(part.local.clone())
        inputs.append(part.Q.clone())
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(inputs), whole.Q)
    assert torch.equal(torch.cat(parts), whole.local) and torch.equal(whole.gathered, whole.local)
