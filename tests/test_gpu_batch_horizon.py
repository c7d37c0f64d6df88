"""-m gpu: the batched MPC horizons pmt_batch_horizon_coeffs_f64 / pmt_batch_horizon_expand_f64 (csrc/batch_horizon.hip) and their host class
batch.BatchHorizon.

Every output lies inside a guarded buffer whose WHOLE image is compared bit for bit with the numpy restatement of the header's order
(tests/batch_horizon_util.py; tests/test_batch_horizon_host.py checks that restatement against the oracle, against Python integers and
against quad_stages_util's): out_stride = L + 3, and the guards in front and behind and the three words between two slabs must still hold
the poison.  The data has full mantissas, mixed magnitudes, zeros of both signs and pairs M[j,k] = -M[k,j], so a sum taken in another
order, a neighbour's entry or a dropped sign of zero differs.  Beside the restatement: an instance's slab and its expansion equal, word for
word, what pmt_quad_stages_f64 writes for that instance's own table.  Every size used is valid; nothing here provokes a fault."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import batch_horizon_util as H  # noqa: E402
from test_gpu_batch_slabs import cus, dev_f64, image, owned  # noqa: E402

COEFFS, EXPAND = "pmt_batch_horizon_coeffs_f64", "pmt_batch_horizon_expand_f64"
GAP = 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


class HorizonBatch:
    """a batch in the device layout, on the host and on the device; the restatement is computed once per sign triple"""

    def __init__(self, B, T, nx, nu, m, seed):
        self.B, self.T, self.nx, self.nu, self.m = B, T, nx, nu, m
        self.L = H.slab_doubles(T, nx, nu, m)
        self.host = list(H.horizon_data(B, T, nx, nu, m, np.random.default_rng(seed)))
        self.upload()

    def upload(self):
        self.dev = [dev_f64(h) for h in self.host]
        self.refs = {}

    def reference(self, signs):
        if signs not in self.refs:
            self.refs[signs] = H.horizon_slab_reference(*self.host, *signs, T=self.T)
        return self.refs[signs].copy()

    def run(self, signs=(-1, -1, -1), shift=0):
        """-> Guarded output of B * (L + 3) doubles; r / v are passed as NULL where their sign is 0"""
        import gpu_util as g
        assert self.L == g.lib().pmt_batch_horizon_slab_doubles(self.T, self.nx, self.nu, self.m)
        out = g.Guarded(self.B * (self.L + GAP), doubles=True, shift=shift)
        p = [d[1] for d in self.dev]
        g.call(COEFFS, p[0], p[1], p[2] if signs[0] else None, p[3] if signs[1] else None, p[4], p[5], self.B, self.T, self.nx, self.nu, self.m,
               signs[0], signs[1], signs[2], out.ptr(), self.L + GAP, g.stream())
        return out

    def check(self, signs=(-1, -1, -1), shift=0, what=""):
        out = self.run(signs, shift)
        out.check(image(out, self.reference(signs), self.L + GAP),
                  "%s T=%d nx=%d nu=%d m=%d B=%d signs %r shift %d" % (what, self.T, self.nx, self.nu, self.m, self.B, signs, shift))
        return out


@functools.lru_cache(maxsize=4)
def batch(B, T, nx, nu, m):
    return HorizonBatch(B, T, nx, nu, m, seed=13 + 1000 * nx + 10 * nu + T + m)


def b_many():
    return 3 * cus() + 37                       # dims <= 64: three workgroups a CU are resident — every workgroup gets a second instance, 37 a third


# ---- a. bit for bit against the restatement, at the tile and block edges

# every nx in {1, 63, 64, 65, 128} and every nu in {0, 1, 64, 65}; both kernels (dims <= 64 | <= 128) with either matrix the larger one
EDGES = [(1, 0, 1, 0), (1, 1, 2, 5), (1, 65, 3, 5), (63, 1, 3, 0), (63, 64, 2, 5), (64, 0, 1, 5), (64, 65, 2, 0), (65, 0, 3, 5), (65, 1, 1, 0),
         (65, 64, 2, 5), (128, 0, 2, 5), (128, 64, 1, 0), (128, 65, 3, 5)]


@pytest.mark.parametrize("nx,nu,T,m", EDGES)
def test_slabs_are_the_restatement_bit_for_bit(nx, nu, T, m):
    bt = batch(3, T, nx, nu, m)
    bt.check((-1, -1, -1), what="tile edges")
    bt.check((1, 1, 1), what="tile edges")


# ---- b. the constant's 256 chains wrap

@pytest.mark.parametrize("T,nx,nu", [(129, 3, 2), (300, 3, 2), (257, 3, 0)])
def test_more_than_256_stages(T, nx, nu):
    """258, 600 and 257 stage constants: chain c of the constant adds the stages c, c + 256, .. in z order"""
    bt = HorizonBatch(2, T, nx, nu, 1, seed=T)
    assert (2 * T if nu else T) > 256
    bt.check((-1, 1, -1), what="chains wrap")


# ---- c. more instances than resident workgroups; position independence

def test_more_instances_than_resident_workgroups_and_position_independence():
    B, T, nx, nu, m = 2000, 2, 3, 2, 1
    assert B > 3 * cus()
    bt = HorizonBatch(B, T, nx, nu, m, seed=5)
    for h in bt.host:                           # the same instance data at positions 0, 1 and B - 1
        h[1] = h[0]
        h[B - 1] = h[0]
    bt.upload()
    out = bt.check((-1, 1, -1), what="persistent loop")
    got = owned(out).reshape(B, bt.L + GAP)
    assert np.array_equal(bits(got[0, :bt.L]), bits(got[1, :bt.L])) and np.array_equal(bits(got[0, :bt.L]), bits(got[B - 1, :bt.L]))
    alone = HorizonBatch(1, T, nx, nu, m, seed=0)
    alone.host = [np.ascontiguousarray(h[:1]) for h in bt.host]
    alone.upload()
    o1 = alone.run((-1, 1, -1))
    o1.check(np.concatenate([got[0, :bt.L], np.full(GAP, np.nan)]), "the instance alone against in place")


# ---- d. the three signs are three arguments

@pytest.mark.parametrize("sign_d", [-1, 0, 1])
@pytest.mark.parametrize("sign_v", [-1, 0, 1])
@pytest.mark.parametrize("sign_r", [-1, 0, 1])
def test_all_sign_triples(sign_r, sign_v, sign_d):
    T, nx, nu, m = 3, 65, 10, 4
    bt = batch(2, T, nx, nu, m)
    signs = (sign_r, sign_v, sign_d)
    want = bt.reference(signs)
    sec = H.sections(T, nx, nu, m)
    q = want[:, sec["q"]].reshape(2, T, nx + nu)
    for part, s in ((q[:, :, :nx], sign_r), (q[:, :, nx:], sign_v)):
        assert np.all(bits(part) == 0) if s == 0 else np.any(part != 0)
    assert (np.all(bits(want[:, sec["const"]]) == 0)) == (sign_r == 0 and sign_v == 0)
    if sign_d == 0:
        assert np.all(bits(want[:, sec["d"]]) == 0)
    bt.check(signs, what="signs")               # (r / v NULL where their sign is 0)


# ---- e. a slab base 8 mod 16

@pytest.mark.parametrize("nx,nu,T,m", [(65, 10, 3, 4), (8, 3, 2, 1), (128, 33, 2, 0)])
def test_slab_base_eight_bytes_off_a_16_byte_boundary(nx, nu, T, m):
    """with the odd / even pitch L + 3 the later slabs start on either parity"""
    bt = batch(2, T, nx, nu, m)
    out = bt.check((-1, 1, 1), shift=1, what="base 8 mod 16")
    assert out.ptr().value % 16 == 8


# ---- f. instances do not see each other

def _isolation(B, T, nx, nu, m, victims, seed):
    signs = (-1, 1, 1)
    bt = HorizonBatch(B, T, nx, nu, m, seed=seed)
    want = bt.reference(signs)
    bt.check(signs, what="clean run")
    sec = H.sections(T, nx, nu, m)
    stride = bt.L + GAP
    for which in (0, 1, 2, 3):                                                  # NaN in Q, R, r, v — one at a time
        saved = bt.host[which].copy()
        for k in victims:
            bt.host[which][k].reshape(-1)[(7 * k + 3) % bt.host[which][k].size] = np.nan
        bt.upload()
        out = bt.run(signs)
        got = owned(out).reshape(B, stride)
        expect = want.copy()
        for k in victims:
            head = got[k, :sec["C"].start]
            assert np.isnan(head).any() and np.isnan(head[sec["const"]]).all(), "instance %d: the NaN did not reach its slab" % k
            if which >= 2:                                                      # the references do not enter SQ and SR
                assert np.array_equal(bits(head[sec["SQ"]]), bits(want[k, sec["SQ"]])) and np.array_equal(bits(head[sec["SR"]]), bits(want[k, sec["SR"]]))
            expect[k, :sec["C"].start] = head                                   # C and the d-consts of the victim stay as they were
        out.check(image(out, expect, stride), "NaN in %s of instances %r" % ("QRrv"[which], victims))
        bt.host[which] = saved
    bt.upload()


def test_nan_in_one_instance_stays_in_its_slab():
    _isolation(5, 3, 65, 10, 2, [2], seed=21)


def test_nan_stays_in_its_slab_on_a_shared_workgroup():
    """instances k - G, k and k + G run on one persistent workgroup, one after the other, through the same LDS"""
    B, G = b_many(), 3 * cus()
    assert B > G
    _isolation(B, 2, 3, 2, 1, [5 + G, B - 1], seed=22)


# ---- g. against the single-instance node

@pytest.mark.parametrize("T,nx,nu", [(3, 65, 10), (4, 128, 33), (130, 5, 2)])
def test_slab_and_expansion_equal_the_stage_node_for_the_instance_s_own_table(T, nx, nu):
    """pmt_quad_stages_check + pmt_quad_stages_f64 on the instance's own table [x_0, u_0, x_1, ..] (stages created one behind the other, a
    non-trivial varmap): SQ / SR / q / const of the slab are its coefficients word for word, pmt_batch_horizon_expand_f64 of the slab its
    buffers whole — the (0.0, var) linear terms of the plain stages among them —, and the constraint block what pmt_batch_expand_f64 writes"""
    import gpu_util as g
    from test_gpu_quad_stages import Launch
    B, m, i = 2, 4, 1
    bt = HorizonBatch(B, T, nx, nu, m, seed=T + nx)
    Qt, Rt, r, v, Ct, d = bt.host
    n, w = T * (nx + nu), nx + nu
    rng = np.random.default_rng(n)
    xvar = np.sort(rng.choice(np.arange(1, n + 10), n, replace=False)).astype(np.int64)
    varmap = (rng.permutation(n + 9) + 1 + 100).astype(np.int64)
    d_x, d_map = g.to_dev(xvar), g.to_dev(varmap)
    sec = H.sections(T, nx, nu, m)
    nqx, nqu = nx * (nx + 1) // 2, nu * (nu + 1) // 2
    for signs in ((-1, 0, -1), (1, -1, 1)):
        out = bt.check(signs, what="against the node")
        slab = owned(out).reshape(B, bt.L + GAP)[i, :bt.L]
        stages, nterms, nlin = H.instance_stages(Qt[i].T, Rt[i].T, r[i], v[i], signs[0], signs[1], xvar)
        node = Launch(stages, varmap, nterms, nlin).run()
        quad, lin, consts, const = node.host()
        qc = quad.reshape(-1, 3)[:, 0].view(np.float64)
        for t in range(T):
            at = t * (nqx + nqu)
            assert np.array_equal(bits(qc[at:at + nqx]), bits(slab[sec["SQ"]])) and np.array_equal(bits(qc[at + nqx:at + nqx + nqu]), bits(slab[sec["SR"]]))
        assert np.array_equal(lin.reshape(-1, 2)[:, 0], bits(slab[sec["q"]])) and bits([const])[0] == bits(slab[sec["const"]])[0]
        # the expansion: whole buffers, the quadratic terms at an address 8 mod 16
        oq, ol, oc = g.Guarded(3 * nterms, shift=1), g.Guarded(2 * n), g.Guarded(1, doubles=True)
        ov, ovc = g.Guarded(3 * m * n, shift=1), g.Guarded(m, doubles=True)
        slab_ptr = C.c_void_p(out.ptr().value + 8 * i * (bt.L + GAP))
        g.call(EXPAND, slab_ptr, T, nx, nu, m, g.ptr(d_x), g.ptr(d_map), oq.ptr(), ol.ptr(), oc.ptr(), ov.ptr(), ovc.ptr(), g.stream())
        oq.check(quad, "expanded quadratic terms against the node %r" % (signs,))
        ol.check(lin, "expanded linear terms against the node")
        oc.check(np.array([const]), "expanded constant against the node")
        if signs[1] == 0:                                                       # the plain stages' linear terms: (0.0, vm[xvar[j]])
            lu = lin.reshape(T, w, 2)[:, nx:, :]
            assert np.all(lu[:, :, 0] == 0) and np.array_equal(lu[:, :, 1].reshape(-1), varmap[xvar.reshape(T, w)[:, nx:].reshape(-1) - 1])
        # .. and the restatement of the expansion
        rq, rl, rc, rv, rvc = H.expanded_reference(Qt[i].T, Rt[i].T, r[i], v[i], Ct[i].T, d[i], *signs, xvar, varmap)
        oq.check(rq, "expanded quadratic terms")
        ol.check(rl, "expanded linear terms")
        ov.check(rv, "expanded constraint terms")
        ovc.check(rvc, "expanded constraint constants")
        # the constraint block of the least-squares batch's expansion: a slab in its layout [Q | q | const | C | d-consts] with the same tail
        nq = n * (n + 1) // 2
        fake = torch.cat([torch.zeros(nq + n + 1, dtype=torch.float64, device=g.DEV), torch.from_numpy(slab[sec["C"].start:].copy()).to(g.DEV)])
        sq, sl, sc = g.empty_terms(nq, g.QT), g.empty_terms(n, g.LT), g.empty_f64(1)
        sv, svc = g.Guarded(3 * m * n), g.Guarded(m, doubles=True)
        g.call("pmt_batch_expand_f64", g.ptr(fake), n, m, g.ptr(d_x), g.ptr(d_map), g.ptr(sq), g.ptr(sl), g.ptr(sc), sv.ptr(), svc.ptr(), g.stream())
        sv.check(rv, "pmt_batch_expand_f64's constraint terms")
        svc.check(rvc, "pmt_batch_expand_f64's constraint constants")


def test_expansion_without_inputs_or_constraints():
    """nu == 0 and m == 0: the table is [x_0, x_1, ..], out_vat / out_vconsts may be NULL"""
    import gpu_util as g
    T, nx = 5, 70
    bt = HorizonBatch(1, T, nx, 0, 0, seed=3)
    Qt, Rt, r, v, Ct, d = bt.host
    n = T * nx
    xvar, varmap = np.arange(2, n + 2, dtype=np.int64), (np.arange(n + 1, dtype=np.int64)[::-1] + 50).copy()
    out = bt.check((-1, 0, 0), what="nu == 0, m == 0")
    nterms = T * nx * (nx + 1) // 2
    oq, ol, oc = g.Guarded(3 * nterms), g.Guarded(2 * n, shift=1), g.Guarded(1, doubles=True)
    d_x, d_map = g.to_dev(xvar), g.to_dev(varmap)
    g.call(EXPAND, out.ptr(), T, nx, 0, 0, g.ptr(d_x), g.ptr(d_map), oq.ptr(), ol.ptr(), oc.ptr(), None, None, g.stream())
    rq, rl, rc, rv, rvc = H.expanded_reference(Qt[0].T, Rt[0].T, r[0], v[0], Ct[0].T, d[0], -1, 0, 0, xvar, varmap)
    oq.check(rq, "quadratic terms")
    ol.check(rl, "linear terms")
    oc.check(np.array([rc]), "constant")
    # an empty batch: nothing is written
    out = g.Guarded(8, doubles=True)
    g.call(COEFFS, None, None, None, None, None, None, 0, 3, 4, 2, 2, -1, -1, -1, out.ptr(), H.slab_doubles(3, 4, 2, 2), g.stream())
    out.check(out.padding(8), "B == 0")


# ---- h. batch.BatchHorizon

def _fetch(wl):
    B, T, nx, nu, n, m = wl.B, wl.T, wl.nx, wl.nu, wl.n, wl.m
    f = lambda t, *shape: t.cpu().numpy().reshape(B, *shape)
    return f(wl.Q, nx, nx), f(wl.R, nu, nu), f(wl.r, T, nx), f(wl.v, T, nu), f(wl.Cm, n, m), f(wl.d, m)


def test_batch_horizon_compute_and_expand_equal_the_restatement_on_its_inputs():
    import gpu_util as g
    from oracle import oracle as O
    from parametron_jl_amd import batch as PB
    total, T, nx, nu, m = 4, 3, 70, 6, 2
    wl = PB.BatchHorizon(torch, total, T, nx, nu, m)
    off, L = PB.horizon_slab_layout(T, nx, nu, m)
    assert (wl.offsets, wl.L, wl.lo, wl.hi, wl.B, wl.n) == (off, L, 0, total, total, T * (nx + nu)) and wl.local.shape == (total, L) and wl.gathered is wl.local
    assert set(PB.BatchHorizon.SEEDS.values()).isdisjoint(set(PB.BatchLSQ.SEEDS.values()) | set(PB.BatchTracking.SEEDS.values()))
    assert len(set(PB.BatchHorizon.SEEDS.values())) == 6
    wl.local.fill_(float("nan"))
    wl.compute()
    torch.cuda.synchronize()
    data = _fetch(wl)
    assert np.array_equal(bits(data[0].reshape(-1)), bits(O.fill_uniform(total * nx * nx, PB.BatchHorizon.SEEDS["Q"])))
    assert np.array_equal(bits(data[5].reshape(-1)), bits(O.fill_uniform(total * m, PB.BatchHorizon.SEEDS["d"], 2.0)))
    want = H.horizon_slab_reference(*data, -1, 0, -1)                           # x_t - r_t, u_t as it is, C*z - d
    assert np.array_equal(bits(wl.local.cpu().numpy()), bits(want))
    # one instance's MOI buffers
    n = wl.n
    xvar, varmap = np.arange(1, n + 1, dtype=np.int64), (np.random.default_rng(1).permutation(n) + 1).astype(np.int64)
    d_x, d_map = g.to_dev(xvar), g.to_dev(varmap)
    quad, lin, const, vat, vc = wl.expand(2, d_x, d_map)
    torch.cuda.synchronize()
    Qt, Rt, r, v, Ct, d = data
    rq, rl, rc, rv, rvc = H.expanded_reference(Qt[2].T, Rt[2].T, r[2], v[2], Ct[2].T, d[2], -1, 0, -1, xvar, varmap)
    assert np.array_equal(quad.cpu().numpy(), rq) and np.array_equal(lin.cpu().numpy(), rl) and np.array_equal(vat.cpu().numpy(), rv)
    assert bits(const.cpu().numpy())[0] == bits([rc])[0] and np.array_equal(bits(vc.cpu().numpy()), bits(rvc))
    # another epoch: other data, the same relation
    wl.regenerate(1)
    wl.step(None)
    torch.cuda.synchronize()
    Q1 = wl.Q.cpu().numpy()
    assert not np.array_equal(Q1, data[0].reshape(-1)) and np.array_equal(bits(Q1), bits(O.fill_uniform(total * nx * nx, PB.BatchHorizon.SEEDS["Q"] + 1000)))
    assert np.array_equal(bits(wl.local.cpu().numpy()), bits(H.horizon_slab_reference(*_fetch(wl), -1, 0, -1)))


def test_batch_horizon_sharding_is_data_independent():
    """the shards of rank 0 and rank 1 of world = 2, built on this one device, hold the slabs world = 1 holds for the same instances"""
    from parametron_jl_amd import batch as PB
    total, T, nx, nu, m = 6, 4, 65, 9, 3
    whole = PB.BatchHorizon(torch, total, T, nx, nu, m)
    whole.step(None)
    parts, inputs = [], {k: [] for k in "QRrvCd"}
    for rank in range(2):
        part = PB.BatchHorizon(torch, total, T, nx, nu, m, rank=rank, world=2)
        assert (part.lo, part.hi, part.B) == (3 * rank, 3 * rank + 3, 3) and part.gathered.shape == (total, part.L) and part.local.shape == (3, part.L)
        part.compute()
        parts.append(part.local.clone())
        for k, t in zip("QRrvCd", (part.Q, part.R, part.r, part.v, part.Cm, part.d)):
            inputs[k].append(t.clone())
    torch.cuda.synchronize()
    for k, t in zip("QRrvCd", (whole.Q, whole.R, whole.r, whole.v, whole.Cm, whole.d)):
        assert torch.equal(torch.cat(inputs[k]), t), k
    assert torch.equal(torch.cat(parts), whole.local) and whole.gathered is whole.local
