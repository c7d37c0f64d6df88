"""-m gpu: the batched horizons with time-varying stage weights pmt_batch_horizon_tv_coeffs_f64 / pmt_batch_horizon_tv_expand_f64
(csrc/batch_horizon_tv.hip) and their host classes batch.BatchTVHorizon / batch.BatchTVMPC.

Every output lies inside a guarded buffer whose WHOLE image is compared bit for bit with the restatement of the header's text
(tests/batch_horizon_tv_util.py; tests/test_batch_horizon_tv_host.py checks that restatement against the oracle and the siblings'):
out_stride = L + 3, and the guards in front and behind and the three words between two slabs must still hold the poison.  The matrices and
references name their place — (instance, stage, row, column), negative where the indices' sum is odd —, so the block of another stage, a
transposed index, a sum taken in another order or a lost sign differs.  Beside the restatement: with equal matrices per stage the words
are those pmt_batch_horizon_coeffs_f64 writes in the same test; every stage's words are those pmt_batch_form_coeffs_f64 writes for the stage
as an instance of its own, from the same device inputs; an instance's expansion equals, word for word, what pmt_quad_stages_f64 writes for
a table that points into the same device inputs, stage s's Q at its own matrix.  Every size used is valid; nothing here provokes a fault."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import batch_horizon_tv_util as V  # noqa: E402
import batch_horizon_util as H  # noqa: E402
from test_gpu_batch_slabs import cus, dev_f64, image, owned  # noqa: E402

COEFFS, EXPAND = "pmt_batch_horizon_tv_coeffs_f64", "pmt_batch_horizon_tv_expand_f64"
GAP = 3
# a shape (nx, nu) of each path pair: 32 and 16 stages a workgroup pass | 4 | 1 | the three-tile walk
P16, P32, P64, WIDE = (9, 3), (17, 20), (33, 40), (65, 70)
PACK = {3: (32, 6), 9: (16, 4), 17: (4, 4), 33: (1, 4), 65: (1, 4)}     # nd -> (stages per pass, resident workgroups per CU) of its path (csrc/batch_horizon_tv.hip)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


class TvBatch:
    """a batch in the device layout, on the host and on the device; the restatement is computed once per sign triple.  Q, R, r, v name
    their place (seed None) or are random; C and d are random"""

    def __init__(self, B, T, nx, nu, term=0, m=0, seed=None):
        self.B, self.T, self.nx, self.nu, self.term, self.m = B, T, nx, nu, term, m
        self.L = V.slab_doubles(T, nx, nu, term, m)
        rnd = V.tv_data(B, T, nx, nu, term, m, np.random.default_rng(7 if seed is None else seed))
        self.host = (list(V.encoded_data(B, T, nx, nu, term)) if seed is None else list(rnd[:4])) + list(rnd[4:])
        self.upload()

    def upload(self):
        self.dev = [dev_f64(h) for h in self.host]
        self.refs = {}

    def reference(self, signs):
        if signs not in self.refs:
            self.refs[signs] = V.slab_reference(*self.host, *signs)
        return self.refs[signs].copy()

    def pointers(self, signs):
        """NULL where the contract does not read: a reference whose sign is 0, R and v with nu == 0, C and d with m == 0"""
        p = [d[1] for d in self.dev]
        return (p[0], p[1] if self.nu else None, p[2] if signs[0] else None, p[3] if signs[1] and self.nu else None,
                p[4] if self.m else None, p[5] if self.m else None)

    def run(self, signs=(-1, -1, -1), shift=0):
        """-> Guarded output of B * (L + 3) doubles"""
        import gpu_util as g
        assert self.L == g.lib().pmt_batch_horizon_tv_slab_doubles(self.T, self.nx, self.nu, self.term, self.m)
        out = g.Guarded(self.B * (self.L + GAP), doubles=True, shift=shift)
        g.call(COEFFS, *self.pointers(signs), self.B, self.T, self.nx, self.nu, self.term, self.m, signs[0], signs[1], signs[2], out.ptr(),
               self.L + GAP, g.stream())
        return out

    def check(self, signs=(-1, -1, -1), shift=0, what=""):
        out = self.run(signs, shift)
        out.check(image(out, self.reference(signs), self.L + GAP), "%s T=%d nx=%d nu=%d term=%d m=%d B=%d signs %r shift %d" % (
            what, self.T, self.nx, self.nu, self.term, self.m, self.B, signs, shift))
        return out


@functools.lru_cache(maxsize=4)
def batch(B, T, nx, nu, term=0, m=0):
    return TvBatch(B, T, nx, nu, term, m)


# ---- 1. bit for bit against the restatement, at the path and tile edges

# (nx, nu) on both sides of 8 / 9, 16 / 17, 32 / 33, 64 / 65 for either matrix, and 128; one row; nu == 0
PATHS = [(8, 9), (9, 8), (16, 17), (17, 16), (32, 33), (33, 32), (64, 65), (65, 64), (128, 1), (1, 128), (1, 0), (5, 0), (128, 128), (15, 31), (63, 127), (2, 2)]


@pytest.mark.parametrize("nx,nu", PATHS)
def test_slabs_are_the_restatement_bit_for_bit(nx, nu):
    bt = batch(3, 3, nx, nu, 0, 2)
    bt.check((-1, -1, -1), what="path and tile edges")
    bt.check((1, 0, 1), what="path and tile edges")


@pytest.mark.parametrize("term", [0, 1])
@pytest.mark.parametrize("nx,nu", [(16, 17), (65, 64), (5, 0)])
def test_a_terminal_stage(nx, nu, term):
    batch(3, 3, nx, nu, term, 2).check((-1, 1, -1), what="terminal stage")


# ---- 2. stage counts

@pytest.mark.parametrize("nx,nu", [P16, P32, P64, WIDE, (4, 0)])
@pytest.mark.parametrize("T", [1, 2, 3])
def test_stage_counts(T, nx, nu):
    bt = batch(5, T, nx, nu, T & 1, 1)
    bt.check((-1, -1, -1), what="stage counts")
    bt.check((0, 1, 0), what="stage counts, r NULL")


def test_one_instance_of_130_stage_pairs():
    """260 stage constants: chain c of const adds the stages c, c + 256 in z order"""
    batch(1, 130, 5, 3).check((-1, 1, -1), what="B = 1, T = 130")


def test_the_largest_stage_count():
    bt = batch(2, 512, 2, 1, 1, 0)
    assert V.dims(512, 2, 1, 1)[1] == 1025
    bt.check((-1, -1, 0), what="T = 512, term = 1")


@pytest.mark.parametrize("nx,nu", [(2, 1), P32, (33, 0)])
def test_1500_instances_of_two_stages(nx, nu):
    batch(1500, 1 if nu else 2, nx, nu).check((-1, 1, -1), what="two stages, B = 1500")


# ---- 3. items against the resident grid: the item is the stage

def _split(items):
    """(B, T) with B * T == items where a stage count in 2 .. 64 divides it, else the next multiple of 33"""
    for per in range(64, 1, -1):
        if items % per == 0:
            return items // per, per
    return -(-items // 33), 33


@pytest.mark.parametrize("nd", [3, 9, 17, 33, 65])
def test_five_passes_more_than_resident_workgroups(nd):
    """five workgroups take a second pass, whose items lie in other instances or at other stages; the last pass is partial where a pass
    holds several items"""
    pack, per_cu = PACK[nd]
    items = pack * (per_cu * cus() + 5) - (3 if pack > 1 else 0)
    B, T = _split(items)
    assert B * T >= items and T > 1
    batch(B, T, nd, 0).check((-1, 0, 0), what="resident workgroups + 5")


@pytest.mark.parametrize("nd,as_u", [(9, False), (17, False), (17, True), (65, False)])
def test_many_rounds_with_a_stride_that_is_no_multiple_of_the_stage_count(nd, as_u):
    """(instance, stage) follows the item by adding (stride / per, stride % per) with a carry: three rounds, 7 stages an instance — of the x
    stages' launch, and of the u stages' (the x stages then have one row)"""
    B = -(-(PACK[nd][0] * (3 * PACK[nd][1] * cus() + 11)) // 7)
    batch(B, 7, 1 if as_u else nd, nd if as_u else 0).check((1, -1, 0), what="three rounds")


def test_position_independence():
    """the same instance data at positions 0, 1 and B - 1, and alone"""
    B, T = 9, 4
    for nx, nu in (P16, P32, P64, WIDE):
        bt = TvBatch(B, T, nx, nu, 1, 2, seed=5)
        for h in bt.host:
            h[1] = h[0]
            h[B - 1] = h[0]
        bt.upload()
        out = bt.check((-1, 1, -1), what="positions")
        got = owned(out).reshape(B, bt.L + GAP)
        assert np.array_equal(bits(got[0, :bt.L]), bits(got[1, :bt.L])) and np.array_equal(bits(got[0, :bt.L]), bits(got[B - 1, :bt.L]))
        alone = TvBatch(1, T, nx, nu, 1, 2, seed=0)
        alone.host = [np.ascontiguousarray(h[:1]) for h in bt.host]
        alone.upload()
        alone.run((-1, 1, -1)).check(np.concatenate([got[0, :bt.L], np.full(GAP, np.nan)]), "the instance alone against in place")


# ---- 4. the three signs are three arguments

@pytest.mark.parametrize("signs", list(itertools.product((-1, 0, 1), repeat=3)), ids=lambda s: "%+d%+d%+d" % s)
def test_all_27_sign_triples(signs):
    for nx, nu in (P16, P32, P64, WIDE):
        bt = batch(2, 2, nx, nu, 1, 2)
        want = bt.reference(signs)
        sec = V.sections(2, nx, nu, 1, 2)
        for (kind, _), qs in zip(V.stage_kinds(2, nu, 1), sec["qs"]):
            assert np.all(bits(want[:, qs]) == 0) == (signs[0 if kind == "x" else 1] == 0)
        assert np.all(bits(want[:, sec["d"]]) == 0) == (signs[2] == 0)
        bt.check(signs, what="signs")


def test_zeros_of_both_signs():
    """a -0.0 matrix word (S = -0.0 + 0.0 and 2 * -0.0), and a chain whose first product is -0.0: the first product starts the chain"""
    for nx, nu in (P16, P32, P64, WIDE):
        bt = TvBatch(3, 2, nx, nu, 0, 1, seed=9)
        Qt, Rt, r = bt.host[0], bt.host[1], bt.host[2]
        Qt[:, :, 1, 0], Qt[:, :, 0, 1] = -0.0, 0.0          # S[0,1] = Q[0,1] + Q[1,0]
        Qt[1, :, 2, 2] = -0.0                               # the diagonal: 2 * -0.0 = -0.0
        Qt[2, :, :, 0] = 0.0                                # row 0 of S is 0 but for its diagonal ...
        Qt[2, :, 0, :] = 0.0
        Qt[2, :, 0, 0] = -0.0                               # ... -0.0, so lin_0 = -0.0*c_0 + 0*c_1 + ..: its sign depends on where the chain starts
        Rt[0, :, 0, 0] = -0.0
        bt.upload()
        ref = bt.reference((1, -1, -1))
        sec = V.sections(2, nx, nu, 0, 1)
        blk = ref[:, sec["S"][0]]
        assert bits(blk[0, 1:2])[0] == 0 and bits(blk[1, 2 * nx - 1:2 * nx])[0] == bits([-0.0])[0]      # -0.0 + 0.0 = +0.0 at tri(0,1); 2 * -0.0 at tri(2,2)
        assert bits(blk[2, 0:1])[0] == bits([-0.0])[0]
        for signs in ((1, -1, -1), (-1, 1, 1)):
            bt.check(signs, what="zeros of both signs")


# ---- 5. alignment and placement

@pytest.mark.parametrize("nx,nu", [P16, P32, P64, WIDE, (2, 1)])
def test_slab_base_eight_bytes_off_a_16_byte_boundary(nx, nu):
    """with nx(nx+1)/2 odd (9: 45, 17: 153, 33: 561, 65: 2145, 2: 3) the blocks of one slab start on either parity"""
    assert (nx * (nx + 1) // 2) % 2 == 1
    bt = batch(3, 3, nx, nu, 1, 2)
    out = bt.check((-1, 1, 1), shift=1, what="base 8 mod 16")
    assert out.ptr().value % 16 == 8


@pytest.mark.parametrize("nx,nu,T,term", [(65, 10, 3, 0), (8, 3, 2, 1)])
def test_slab_and_dynamics_section_in_one_row_do_not_touch_each_other(nx, nu, T, term):
    """[L | Ltv | 3 words of gap] per instance: the new call and pmt_batch_horizon_dynamics_tv_f64 (T + term records) at the stride
    L + Ltv + 3, the section at out + L"""
    import gpu_util as g
    import batch_horizon_ltv_util as LV
    from test_gpu_batch_horizon_ltv import LtvBatch
    B, Td = 3, T + term
    bt, lt = batch(B, T, nx, nu, term, 0), LtvBatch(B, Td, nx, nu)
    L, Ltv = bt.L, lt.Ltv
    assert Ltv == LV.section_doubles(Td, nx, nu)
    stride = L + Ltv + GAP
    out = g.Guarded(B * stride, doubles=True)
    g.call("pmt_batch_horizon_dynamics_tv_f64", *lt.pointers((-1, -1, -1)), B, Td, nx, nu, -1, -1, -1, C.c_void_p(out.ptr().value + 8 * L), stride, g.stream())
    g.call(COEFFS, *bt.pointers((-1, 1, -1)), B, T, nx, nu, term, 0, -1, 1, -1, out.ptr(), stride, g.stream())
    rows = np.concatenate([bt.reference((-1, 1, -1)), lt.reference((-1, -1, -1))], axis=1)
    out.check(image(out, rows, stride), "slab and section in one row, nx=%d nu=%d T=%d" % (nx, nu, T))


# ---- 6. stages do not see each other

@pytest.mark.parametrize("nx,nu", [P16, P32, P64, WIDE])
def test_nan_in_one_matrix_stays_in_its_stage_and_its_instance_s_constant(nx, nu):
    signs, B, T = (-1, 1, 1), 3, 4
    bt = TvBatch(B, T, nx, nu, 0, 2)
    want = bt.reference(signs)
    bt.check(signs, what="clean run")
    bt.host[0][1, 2, nx // 2, 0] = np.nan       # Q_{1,2}[0, nx / 2]
    bt.upload()
    out = bt.run(signs)
    got = owned(out).reshape(B, bt.L + GAP)
    sec = V.sections(T, nx, nu, 0, 2)
    s = 4                                       # x_2 in z order: x_0, u_0, x_1, u_1, x_2
    may = np.zeros(bt.L, dtype=bool)
    may[sec["S"][s]] = may[sec["qs"][s]] = True
    may[sec["sconst"].start + s] = may[sec["const"]] = True
    nan = np.isnan(got[1, :bt.L])
    assert not np.any(nan & ~may) and nan[sec["S"][s].start + nx // 2] and nan[sec["const"]][0] and nan[sec["sconst"].start + s]
    assert np.all(nan[sec["qs"][s]][[0, nx // 2]]) and np.count_nonzero(nan[sec["S"][s]]) == 1
    expect = want.copy()
    expect[1, nan] = got[1, :bt.L][nan]
    out.check(image(out, expect, bt.L + GAP), "NaN in Q_{1,2}")


# ---- 7. the first anchor: equal matrices per stage

@pytest.mark.parametrize("nx,nu", [P16, (8, 9), (16, 17), P32, P64, WIDE, (5, 0), (128, 64)])
@pytest.mark.parametrize("term", [0, 1])
def test_equal_matrices_give_the_words_the_time_invariant_launch_writes(nx, nu, term):
    """term == 0: every S block, q and const; term == 1: the first T*(1 + (nu > 0)) stages' blocks and q words"""
    import gpu_util as g
    B, T, m = 3, 4, 2
    Qt1, Rt1, r, v, Ct, d = H.horizon_data(B, T, nx, nu, m, np.random.default_rng(nx + nu))
    rng = np.random.default_rng(1)
    bt = TvBatch(B, T, nx, nu, term, m, seed=0)
    n = V.dims(T, nx, nu, term)[0]
    bt.host = [np.concatenate([np.repeat(Qt1[:, None], T, axis=1)] + [rng.standard_normal((B, 1, nx, nx))] * term, axis=1), np.repeat(Rt1[:, None], T, axis=1),
               np.concatenate([r] + [rng.standard_normal((B, 1, nx))] * term, axis=1), v, rng.standard_normal((B, n, m)), d]
    bt.upload()
    signs = (-1, 1, -1)
    got = owned(bt.check(signs, what="equal matrices")).reshape(B, bt.L + GAP)
    Li = H.slab_doubles(T, nx, nu, m)
    sib = g.Guarded(B * (Li + GAP), doubles=True)
    dv = [dev_f64(a)[0] for a in (Qt1, Rt1, r, v, Ct, d)]
    g.call("pmt_batch_horizon_coeffs_f64", *[g.ptr(t) for t in dv], B, T, nx, nu, m, *signs, sib.ptr(), Li + GAP, g.stream())
    sib.check(image(sib, H.horizon_slab_reference(Qt1, Rt1, r, v, Ct, d, *signs, T=T), Li + GAP), "the sibling's slabs")
    one = owned(sib).reshape(B, Li + GAP)
    sv, si = V.sections(T, nx, nu, term, m), H.sections(T, nx, nu, m)
    for (kind, t), blk in zip(V.stage_kinds(T, nu, term), sv["S"]):
        if t < T:
            assert np.array_equal(bits(got[:, blk]), bits(one[:, si["SQ" if kind == "x" else "SR"]]))
    assert np.array_equal(bits(got[:, sv["q"]][:, :T * (nx + nu)]), bits(one[:, si["q"]]))
    if not term:
        assert np.array_equal(bits(got[:, sv["const"]]), bits(one[:, si["const"]]))


# ---- 8. the second anchor: every stage as an instance of pmt_batch_form_coeffs_f64, on the same device inputs

@pytest.mark.parametrize("nx,nu,term", [(5, 8, 0), P16 + (1,), P32 + (0,), P64 + (1,), WIDE + (0,), (128, 0, 1), (1, 1, 0)])
def test_every_stage_is_the_tracking_cost_s_slab_of_that_stage_alone(nx, nu, term):
    import gpu_util as g
    B, T = 3, 3
    bt = batch(B, T, nx, nu, term, 0)
    for signs in ((-1, 1, 0), (0, -1, 0)):
        got = owned(bt.check(signs, what="stage as instance")).reshape(B, bt.L + GAP)
        sec = V.sections(T, nx, nu, term, 0)
        kinds = V.stage_kinds(T, nu, term)
        for kind, nd, per, mat, ref, sign in (("x", nx, T + term, 0, 2, signs[0]), ("u", nu, T, 1, 3, signs[1])):
            if not nd:
                continue
            Lf = nd * (nd + 1) // 2 + nd + 1
            assert Lf == g.lib().pmt_batch_lsq_slab_doubles(nd, 0)
            form = g.Guarded(B * per * Lf, doubles=True)
            g.call("pmt_batch_form_coeffs_f64", bt.dev[mat][1], bt.dev[ref][1] if sign else None, None, None, B * per, nd, 0, sign, 0, form.ptr(), Lf, g.stream())
            slabs = owned(form).reshape(B, per, Lf)
            mine = [s for s, (k, _) in enumerate(kinds) if k == kind]
            assert len(mine) == per
            for t, s in enumerate(mine):
                want = np.concatenate([got[:, sec["S"][s]], got[:, sec["qs"][s]], got[:, sec["sconst"]][:, s:s + 1]], axis=1)
                assert np.array_equal(bits(slabs[:, t]), bits(want)), (kind, t)


# ---- 9. the third anchor: the expansion

def _device_table(bt, i, signs, d_x):
    """instance i's own table for pmt_quad_stages_f64, pointing into the batch's device inputs — stage s's Q at its own matrix; through
    pmt_quad_stages_check"""
    from parametron_jl_amd import _lib
    T, nx, nu, term = bt.T, bt.nx, bt.nu, bt.term
    Q, R, r, v = [d[1].value for d in bt.dev[:4]]
    rows, qa, la = [], 0, 0
    for kind, t in V.stage_kinds(T, nu, term):
        if kind == "x":
            nd, M, ref, sign = nx, Q + 8 * (i * (T + term) + t) * nx * nx, r + 8 * (i * (T + term) + t) * nx, signs[0]
        else:
            nd, M, ref, sign = nu, R + 8 * (i * T + t) * nu * nu, v + 8 * (i * T + t) * nu, signs[1]
        rows.append({"Q": M, "ldq": nd, "xvar": d_x.data_ptr() + 8 * la, "vec": ref if sign else None, "n": nd, "sign": sign, "quad_at": qa, "lin_at": la})
        qa, la = qa + nd * (nd + 1) // 2, la + nd
    arr = _lib.quad_stages(rows)
    _lib.call("pmt_quad_stages_check", C.addressof(arr), len(rows), qa, la)
    return torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()).to("cuda:0"), len(rows), qa, la


# both sides of each path threshold of the launches that wrote the slab, T = 1, nu = 0, more than 256 stages
@pytest.mark.parametrize("T,nx,nu,term,m", [(1, 5, 3, 0, 2), (2, 1, 0, 1, 0), (3, 8, 9, 0, 1), (3, 16, 17, 1, 2), (3, 32, 33, 0, 1), (2, 64, 65, 1, 2), (2, 128, 16, 0, 0),
                                            (130, 5, 2, 0, 1), (512, 2, 1, 1, 0)])
def test_expansion_equals_the_restatement_and_the_stage_node_on_the_same_device_inputs(T, nx, nu, term, m):
    import gpu_util as g
    B, i = 2, 1
    bt = batch(B, T, nx, nu, term, m)
    Qt, Rt, r, v, Ct, d = bt.host
    n, ns = V.dims(T, nx, nu, term)
    rng = np.random.default_rng(n)
    xvar = np.sort(rng.choice(np.arange(1, n + 10), n, replace=False)).astype(np.int64)
    varmap = (rng.permutation(n + 9) + 1 + 100).astype(np.int64)
    d_x, d_map = g.to_dev(xvar), g.to_dev(varmap)
    for signs in ((-1, 0, -1), (1, -1, 1)):
        out = bt.check(signs, what="the slabs")
        table, nst, nterms, nlin = _device_table(bt, i, signs, d_x)
        assert (nst, nlin) == (ns, n)
        # the expansion: whole buffers, the term buffers at an address 8 mod 16
        oq, ol, oc = g.Guarded(3 * nterms, shift=1), g.Guarded(2 * n, shift=1), g.Guarded(1, doubles=True)
        ov, ovc = g.Guarded(3 * m * n, shift=1), g.Guarded(m, doubles=True)
        g.call(EXPAND, C.c_void_p(out.ptr().value + 8 * i * (bt.L + GAP)), T, nx, nu, term, m, g.ptr(d_x), g.ptr(d_map), oq.ptr(), ol.ptr(), oc.ptr(),
               ov.ptr() if m else None, ovc.ptr() if m else None, g.stream())
        rq, rl, rc, rv, rvc = V.expanded_reference(V.matrices(Qt[i]), V.matrices(Rt[i]), r[i], v[i], Ct[i].T, d[i], *signs, xvar, varmap)
        oq.check(rq, "expanded quadratic terms %r" % (signs,))
        ol.check(rl, "expanded linear terms")
        oc.check(np.array([rc]), "expanded constant")
        ov.check(rv, "expanded constraint terms")
        ovc.check(rvc, "expanded constraint constants")
        # the single-model node on a table that points into the same device inputs
        nq, nl, ncs, nc = g.Guarded(3 * nterms, shift=1), g.Guarded(2 * n, shift=1), g.Guarded(ns, doubles=True), g.Guarded(1, doubles=True)
        g.call("pmt_quad_stages_f64", g.ptr(table), ns, g.ptr(d_map), nq.ptr(), nl.ptr(), ncs.ptr(), nc.ptr(), g.stream())
        nq.check(rq, "pmt_quad_stages_f64's quadratic terms %r" % (signs,))
        nl.check(rl, "pmt_quad_stages_f64's linear terms")
        nc.check(np.array([rc]), "pmt_quad_stages_f64's constant")
        torch.cuda.synchronize()
        assert torch.equal(oq.buf, nq.buf) and torch.equal(ol.buf, nl.buf) and torch.equal(oc.buf.view(torch.int64), nc.buf.view(torch.int64))
        # .. and its stage constants are the slab's sconst
        sec = V.sections(T, nx, nu, term, m)
        slab = owned(out).reshape(B, bt.L + GAP)[i, :bt.L]
        ncs.check(slab[sec["sconst"]], "pmt_quad_stages_f64's stage constants")


# ---- 10. batch.BatchTVHorizon, batch.BatchTVMPC

def _inputs(wl):
    f = lambda t, *shape: t.cpu().numpy().reshape(wl.B, *shape)
    Tx = wl.T + wl.term
    return (f(wl.Q, Tx, wl.nx, wl.nx), f(wl.R, wl.T, wl.nu, wl.nu), f(wl.r, Tx, wl.nx), f(wl.v, wl.T, wl.nu), f(wl.Cm, wl.n, wl.m), f(wl.d, wl.m))


def _check_class(wl, total, T, nx, nu, m, term, i):
    """the inputs are their seeds' oracle streams; compute / gather / expand equal the restatement; another epoch likewise"""
    import gpu_util as g
    from oracle import oracle as O
    from parametron_jl_amd import batch as PB
    off, L = PB.horizon_tv_slab_layout(T, nx, nu, m, bool(term))
    assert (wl.offsets, wl.L, wl.term, wl.n, wl.lo, wl.hi, wl.B) == (off, L, term, V.dims(T, nx, nu, term)[0], 0, total, total)
    assert wl.local.shape == (total, wl.stride) and wl.gathered is wl.local
    S = type(wl).SEEDS
    for epoch in (0, 1):
        if epoch:
            Q0 = wl.Q.clone()
            wl.regenerate(1)
            assert not torch.equal(Q0, wl.Q)
        wl.local.fill_(float("nan"))
        wl.step(None)                                                           # world = 1: the rows are the gathered rows
        torch.cuda.synchronize()
        hor = _inputs(wl)
        for name, a in zip(("Q", "R", "r", "v", "C", "d"), hor):
            assert np.array_equal(bits(a.reshape(-1)), bits(O.fill_uniform(a.size, S[name] + 1000 * epoch, PB._Batch.SCALES.get(name, 1.0)))), name
        rows = wl.gathered.cpu().numpy()
        assert np.array_equal(bits(rows[:, :L]), bits(V.slab_reference(*hor, -1, 0, -1)))
    n = wl.n
    xvar, varmap = np.arange(1, n + 1, dtype=np.int64), (np.random.default_rng(1).permutation(n) + 1).astype(np.int64)
    res = wl.expand(i, g.to_dev(xvar), g.to_dev(varmap))
    torch.cuda.synchronize()
    quad, lin, const, vat, vc = res[:5]
    Qt, Rt, r, v, Ct, d = hor
    rq, rl, rc, rv, rvc = V.expanded_reference(V.matrices(Qt[i]), V.matrices(Rt[i]), r[i], None, Ct[i].T, d[i], -1, 0, -1, xvar, varmap)
    assert np.array_equal(quad.cpu().numpy(), rq) and np.array_equal(lin.cpu().numpy(), rl) and np.array_equal(vat.cpu().numpy(), rv)
    assert bits(const.cpu().numpy())[0] == bits([rc])[0] and np.array_equal(bits(vc.cpu().numpy()), bits(rvc))
    return rows, res[5:], xvar, varmap


@pytest.mark.parametrize("terminal", [False, True])
def test_batch_tv_horizon_compute_gather_and_expand_equal_the_restatement_on_its_inputs(terminal):
    from parametron_jl_amd import batch as PB
    total, T, nx, nu, m = 37, 4, 6, 3, 2
    wl = PB.BatchTVHorizon(torch, total, T, nx, nu, m, terminal=terminal)
    assert wl.stride == wl.L
    _check_class(wl, total, T, nx, nu, m, int(terminal), 5)


@pytest.mark.parametrize("terminal", [False, True])
def test_batch_tv_mpc_holds_weights_and_dynamics_of_every_stage_in_one_row(terminal):
    import batch_horizon_ltv_util as LV
    from parametron_jl_amd import batch as PB
    total, T, nx, nu, m = 11, 4, 6, 3, 2
    term = int(terminal)
    wl = PB.BatchTVMPC(torch, total, T, nx, nu, m, terminal=terminal)
    Td = T + term
    doff, Ltv = PB.horizon_dynamics_tv_layout(Td, nx, nu)
    assert (wl.dyn_offsets, wl.Ltv, wl.stride, wl.Td) == (doff, Ltv, wl.L + Ltv, Td)
    assert PB.BatchTVMPC(torch, 2, 2, 3, 1).m == 0 and PB.BatchTVMPC(torch, 2, 2, 3, 1).term == 0          # m defaults to no dense rows
    i = 3
    rows, (terms, consts), xvar, varmap = _check_class(wl, total, T, nx, nu, m, term, i)
    f = lambda t, *shape: t.cpu().numpy().reshape(wl.B, *shape)
    dyn = (f(wl.A, Td - 1, nx, nx), f(wl.Bm, Td - 1, nu, nx), f(wl.h, Td, nx))
    section = LV.section_reference(*dyn, -1, -1, -1)
    assert np.array_equal(bits(rows[:, wl.L:]), bits(section))
    want_t, want_c = LV.expanded_reference(section[i], Td, nx, nu, 1, xvar, varmap)
    assert np.array_equal(terms.cpu().numpy(), want_t) and np.array_equal(bits(consts.cpu().numpy()), bits(want_c))


def test_sharding_is_data_independent():
    """the shards of rank 0 and rank 1 of world = 2, built on this one device, hold the rows world = 1 holds for the same instances"""
    from parametron_jl_amd import batch as PB
    total, T, nx, nu, m = 6, 4, 6, 3, 2
    for cls in (PB.BatchTVHorizon, PB.BatchTVMPC):
        whole = cls(torch, total, T, nx, nu, m, terminal=True)
        whole.step(None)
        parts = []
        for rank in range(2):
            part = cls(torch, total, T, nx, nu, m, terminal=True, rank=rank, world=2)
            assert (part.lo, part.hi, part.B) == (3 * rank, 3 * rank + 3, 3) and part.gathered.shape == (total, part.stride)
            part.compute()
            parts.append(part.local.clone())
        torch.cuda.synchronize()
        assert torch.equal(torch.cat(parts), whole.local) and whole.gathered is whole.local
