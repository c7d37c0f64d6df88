"""-m gpu: the batch of horizons' compact dynamics sections pmt_batch_horizon_dynamics_f64 / pmt_batch_horizon_dynamics_expand_f64
(csrc/batch_horizon_dyn.hip) and their host class batch.BatchMPC.

Every output lies inside a guarded buffer whose WHOLE image is compared bit for bit with the numpy restatement of the header's text
(tests/batch_horizon_dyn_util.py; tests/test_batch_horizon_dyn_host.py checks that restatement against affine_stages_util's and the
oracle): out_stride = Ld + 3, and the guards in front and behind and the three words between two sections must still hold the poison.
The data holds zeros of both signs among normals, so a dropped or doubled sign flip, a neighbour's entry or a transposed index differs.
Beside the restatement: an instance's expansion equals, word for word, what pmt_affine_stages_f64 writes for tables that point into the
same device inputs.  Every size used is valid; nothing here provokes a fault."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import affine_stages_util as U  # noqa: E402
import batch_horizon_dyn_util as D  # noqa: E402
from test_gpu_batch_slabs import cus, dev_f64, image, owned  # noqa: E402

COEFFS, EXPAND = "pmt_batch_horizon_dynamics_f64", "pmt_batch_horizon_dynamics_expand_f64"
GAP = 3
bits = D.bits


class DynBatch:
    """a batch in the device layout, on the host and on the device; the restatement is computed once per sign triple"""

    def __init__(self, B, T, nx, nu, seed):
        self.B, self.T, self.nx, self.nu = B, T, nx, nu
        self.Ld = D.section_doubles(T, nx, nu)
        self.host = list(D.dyn_data(B, T, nx, nu, np.random.default_rng(seed)))
        self.upload()

    def upload(self):
        self.dev = [dev_f64(h) for h in self.host]
        self.refs = {}

    def reference(self, signs):
        if signs not in self.refs:
            self.refs[signs] = D.section_reference(*self.host, *signs)
        return self.refs[signs].copy()

    def run(self, signs=(-1, -1, -1), shift=0):
        """-> Guarded output of B * (Ld + 3) doubles; Bm is passed as NULL with nu == 0, h where sign_h is 0"""
        import gpu_util as g
        assert self.Ld == g.lib().pmt_batch_horizon_dynamics_doubles(self.T, self.nx, self.nu)
        out = g.Guarded(self.B * (self.Ld + GAP), doubles=True, shift=shift)
        p = [d[1] for d in self.dev]
        g.call(COEFFS, p[0], p[1] if self.nu else None, p[2] if signs[2] else None, self.B, self.T, self.nx, self.nu, signs[0], signs[1], signs[2],
               out.ptr(), self.Ld + GAP, g.stream())
        return out

    def check(self, signs=(-1, -1, -1), shift=0, what=""):
        out = self.run(signs, shift)
        out.check(image(out, self.reference(signs), self.Ld + GAP),
                  "%s T=%d nx=%d nu=%d B=%d signs %r shift %d" % (what, self.T, self.nx, self.nu, self.B, signs, shift))
        return out


@functools.lru_cache(maxsize=4)
def batch(B, T, nx, nu):
    return DynBatch(B, T, nx, nu, seed=17 + 1000 * nx + 10 * nu + T)


# ---- 1. bit for bit against the restatement, at the tile and block edges

# every nx in {1, 63, 64, 65, 128}, every nu in {0, 1, 64, 65, 128}, every T in {1, 2, 3} ..
EDGES = [(1, 0, 1), (1, 1, 3), (1, 64, 3), (1, 128, 2), (63, 1, 3), (63, 64, 2), (64, 0, 1), (64, 65, 3), (64, 128, 2), (65, 0, 2), (65, 64, 1),
         (65, 128, 3), (128, 1, 2), (128, 65, 1), (128, 128, 2)]
# .. and every size at which the code takes another path: 512 AB words (a wave per instance up to there), 16 and 32 rows (the tile's shape)
PATHS = [(12, 4, 3), (16, 16, 2), (16, 17, 2), (22, 1, 2), (16, 128, 1), (17, 14, 2), (17, 128, 3), (32, 16, 3), (32, 97, 2), (33, 5, 2)]


@pytest.mark.parametrize("nx,nu,T", EDGES + PATHS)
def test_sections_are_the_restatement_bit_for_bit(nx, nu, T):
    bt = batch(3, T, nx, nu)
    bt.check((-1, -1, -1), what="tile edges")
    bt.check((1, 1, 1), what="tile edges")


# ---- 2. the three signs are three arguments

@pytest.mark.parametrize("sign_h", [-1, 0, 1])
@pytest.mark.parametrize("sign_b", [-1, 1])
@pytest.mark.parametrize("sign_a", [-1, 1])
def test_all_sign_triples(sign_a, sign_b, sign_h):
    T, nx, nu = 3, 5, 3
    bt = batch(2, T, nx, nu)
    signs = (sign_a, sign_b, sign_h)
    want = bt.reference(signs)
    sec = D.sections(T, nx, nu)
    ab = bits(want[:, sec["AB"]]).reshape(2, nx, nx + nu)
    At, Bt, h = bt.host
    assert np.array_equal(ab[:, :, :nx] < 0, (bits(At).transpose(0, 2, 1) < 0) ^ (sign_a < 0))
    assert np.array_equal(ab[:, :, nx:] < 0, (bits(Bt).transpose(0, 2, 1) < 0) ^ (sign_b < 0))
    assert np.all(bits(want[:, sec["hconst"]]) == 0) == (sign_h == 0)
    bt.check(signs, what="signs")               # (h NULL where sign_h is 0)


# ---- 3. more instances than resident workgroups; position independence

def _persistent(B, T, nx, nu):
    bt = DynBatch(B, T, nx, nu, seed=5)
    for h in bt.host:                           # the same instance data at positions 0, 1 and B - 1
        h[1] = h[0]
        h[B - 1] = h[0]
    bt.upload()
    out = bt.check((-1, 1, -1), what="persistent loop")
    got = owned(out).reshape(B, bt.Ld + GAP)
    assert np.array_equal(bits(got[0, :bt.Ld]), bits(got[1, :bt.Ld])) and np.array_equal(bits(got[0, :bt.Ld]), bits(got[B - 1, :bt.Ld]))
    alone = DynBatch(1, T, nx, nu, seed=0)
    alone.host = [np.ascontiguousarray(h[:1]) for h in bt.host]
    alone.upload()
    o1 = alone.run((-1, 1, -1))
    o1.check(np.concatenate([got[0, :bt.Ld], np.full(GAP, np.nan)]), "the instance alone against in place")


def test_more_instances_than_resident_workgroups_and_position_independence():
    assert 2000 > 4 * cus()
    _persistent(2000, 2, 3, 2)


def test_every_wave_of_the_small_kernel_takes_a_second_instance():
    """a wave per instance, eight workgroups of four waves resident per CU"""
    _persistent(32 * cus() + 37, 2, 3, 2)


def test_every_workgroup_of_the_tile_kernel_takes_a_second_instance():
    _persistent(4 * cus() + 37, 2, 17, 14)


# ---- 4. alignment and placement

@pytest.mark.parametrize("nx,nu,T", [(65, 10, 3), (8, 3, 2)])
def test_section_base_eight_bytes_off_a_16_byte_boundary(nx, nu, T):
    """with the odd / even pitch Ld + 3 the later sections start on either parity"""
    bt = batch(2, T, nx, nu)
    out = bt.check((-1, 1, 1), shift=1, what="base 8 mod 16")
    assert out.ptr().value % 16 == 8


@pytest.mark.parametrize("nx,nu,T", [(65, 10, 3), (8, 3, 2)])
def test_slab_and_section_in_one_row_do_not_touch_each_other(nx, nu, T):
    """[L | Ld | 3 words of gap] per instance: pmt_batch_horizon_coeffs_f64 (m = 0) and the new call at the stride L + Ld + 3"""
    import gpu_util as g
    import batch_horizon_util as H
    from test_gpu_batch_horizon import HorizonBatch
    B = 3
    hb, bt = HorizonBatch(B, T, nx, nu, 0, seed=nx), batch(B, T, nx, nu)
    L, Ld = hb.L, bt.Ld
    stride = L + Ld + GAP
    out = g.Guarded(B * stride, doubles=True)
    p = [d[1] for d in hb.dev]
    g.call("pmt_batch_horizon_coeffs_f64", p[0], p[1], p[2], p[3], p[4], p[5], B, T, nx, nu, 0, -1, 1, -1, out.ptr(), stride, g.stream())
    q = [d[1] for d in bt.dev]
    g.call(COEFFS, q[0], q[1], q[2], B, T, nx, nu, -1, -1, -1, C.c_void_p(out.ptr().value + 8 * L), stride, g.stream())
    assert L == H.slab_doubles(T, nx, nu, 0)
    rows = np.concatenate([hb.reference((-1, 1, -1)), bt.reference((-1, -1, -1))], axis=1)
    out.check(image(out, rows, stride), "slab and section in one row, nx=%d nu=%d T=%d" % (nx, nu, T))


# ---- 5. instances do not see each other

@pytest.mark.parametrize("nx,nu,T", [(65, 10, 3), (5, 3, 3)])
def test_nan_in_one_instance_stays_in_its_section(nx, nu, T):
    signs = (-1, 1, 1)
    bt = DynBatch(3, T, nx, nu, seed=21)
    want = bt.reference(signs)
    bt.check(signs, what="clean run")
    bt.host[0][1, nx // 2, 0] = np.nan          # A_1[0, nx / 2]
    bt.host[2][1, T - 1, nx - 1] = np.nan
    bt.upload()
    out = bt.run(signs)
    got = owned(out).reshape(3, bt.Ld + GAP)
    nan_at = np.zeros(bt.Ld, dtype=bool)
    nan_at[nx // 2] = nan_at[bt.Ld - 1] = True
    assert np.array_equal(np.isnan(got[1, :bt.Ld]), nan_at)
    expect = want.copy()
    expect[1, nan_at] = got[1, :bt.Ld][nan_at]
    out.check(image(out, expect, bt.Ld + GAP), "NaN in A and h of instance 1")


# ---- 6. the expansion

def _device_tables(d_A, d_B, d_h, i, T, nx, nu, signs, d_x):
    """the instance's own tables for pmt_affine_stages_f64, pointing into the batch's device inputs; through pmt_affine_stages_check"""
    from parametron_jl_amd import _lib
    sign_xp, sign_a, sign_b, sign_h = signs
    w, rl = nx + nu, 1 + nx + nu
    A_i, B_i, h_i, x = d_A.value + 8 * i * nx * nx, (d_B.value or 0) + 8 * i * nx * nu, d_h.value + 8 * i * T * nx, d_x.data_ptr()
    parts, stages = [], []
    for t in range(T):
        first = len(parts)
        parts.append({"mat": None, "ld": 0, "xvar": x + 8 * t * w, "cols": 1, "sign": sign_xp})
        if t:
            parts.append({"mat": A_i, "ld": nx, "xvar": x + 8 * (t - 1) * w, "cols": nx, "sign": sign_a})
            if nu:
                parts.append({"mat": B_i, "ld": nx, "xvar": x + 8 * ((t - 1) * w + nx), "cols": nu, "sign": sign_b})
        stages.append({"vec": h_i + 8 * t * nx if sign_h else None, "vec_sign": sign_h, "rows": nx, "first_part": first, "nparts": len(parts) - first,
                       "row_len": rl if t else 1, "term_offset": nx + (t - 1) * nx * rl if t else 0, "const_offset": t * nx})
    parr, sarr = _lib.affine_parts(parts), _lib.affine_stages(stages)
    _lib.call("pmt_affine_stages_check", C.addressof(sarr), T, C.addressof(parr), len(parts), D.term_count(T, nx, nu), T * nx)
    to = lambda arr: torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()).to("cuda:0")
    return to(sarr), to(parr)


@pytest.mark.parametrize("T,nx,nu", [(1, 5, 3), (2, 1, 0), (3, 65, 10), (4, 128, 33), (3, 64, 64), (130, 5, 2), (512, 2, 1)])
def test_expansion_equals_the_restatement_and_the_stage_node_on_the_same_device_inputs(T, nx, nu):
    import gpu_util as g
    B, i = 2, 1
    bt = DynBatch(B, T, nx, nu, seed=T + nx)
    n, nterms = T * (nx + nu), D.term_count(T, nx, nu)
    rng = np.random.default_rng(n)
    xvar = np.sort(rng.choice(np.arange(1, n + 10), n, replace=False)).astype(np.int64)
    perm = (rng.permutation(n + 9) + 1 + 100).astype(np.int64)
    d_x, d_map = g.to_dev(xvar), g.to_dev(perm)
    # (sign_xp, sign_a, sign_b, sign_h), the varmap, the term buffer's shift
    for signs, varmap, shift in (((1, -1, -1, -1), perm, 1), ((-1, 1, -1, 1), None, 0), ((1, -1, 1, 0), perm, 0)):
        out = bt.check(signs[1:], what="the sections")
        section = owned(out).reshape(B, bt.Ld + GAP)[i, :bt.Ld]
        ot, oc = g.Guarded(3 * nterms, shift=shift), g.Guarded(T * nx, doubles=True)
        assert ot.ptr().value % 16 == 8 * shift
        g.call(EXPAND, C.c_void_p(out.ptr().value + 8 * i * (bt.Ld + GAP)), T, nx, nu, signs[0], g.ptr(d_x), g.ptr(d_map) if varmap is not None else None,
               ot.ptr(), oc.ptr(), g.stream())
        want_t, want_c = D.expanded_reference(section, T, nx, nu, signs[0], xvar, varmap)
        ot.check(want_t, "expanded terms %r" % (signs,))
        oc.check(want_c, "expanded constants %r" % (signs,))
        # the single-model node on tables that point into the same device inputs
        stable, ptable = _device_tables(bt.dev[0][1], bt.dev[1][1], bt.dev[2][1], i, T, nx, nu, signs, d_x)
        nt, nc = g.Guarded(3 * nterms, shift=shift), g.Guarded(T * nx, doubles=True)
        g.call("pmt_affine_stages_f64", g.ptr(stable), T, g.ptr(ptable), g.ptr(d_map) if varmap is not None else None, nt.ptr(), nc.ptr(), g.stream())
        nt.check(want_t, "pmt_affine_stages_f64's terms %r" % (signs,))
        nc.check(want_c, "pmt_affine_stages_f64's constants %r" % (signs,))
        torch.cuda.synchronize()
        assert torch.equal(ot.buf, nt.buf) and torch.equal(oc.buf.view(torch.int64), nc.buf.view(torch.int64))


# ---- 7. batch.BatchMPC

def _fetch(wl):
    B, T, nx, nu, n, m = wl.B, wl.T, wl.nx, wl.nu, wl.n, wl.m
    f = lambda t, *shape: t.cpu().numpy().reshape(B, *shape)
    return (f(wl.Q, nx, nx), f(wl.R, nu, nu), f(wl.r, T, nx), f(wl.v, T, nu), f(wl.Cm, n, m), f(wl.d, m)), (f(wl.A, nx, nx), f(wl.Bm, nu, nx), f(wl.h, T, nx))


def _rows(wl):
    import batch_horizon_util as H
    hor, dyn = _fetch(wl)
    return np.concatenate([H.horizon_slab_reference(*hor, -1, 0, -1), D.section_reference(*dyn, -1, -1, -1)], axis=1)


def test_batch_mpc_compute_and_expand_equal_the_restatement_on_its_inputs():
    import gpu_util as g
    import batch_horizon_util as H
    from oracle import oracle as O
    from parametron_jl_amd import batch as PB
    total, T, nx, nu, m = 37, 4, 6, 3, 2
    wl = PB.BatchMPC(torch, total, T, nx, nu, m)
    (off, L), (doff, Ld) = PB.horizon_slab_layout(T, nx, nu, m), PB.horizon_dynamics_layout(T, nx, nu)
    assert (wl.offsets, wl.L, wl.dyn_offsets, wl.Ld, wl.stride, wl.lo, wl.hi, wl.B) == (off, L, doff, Ld, L + Ld, 0, total, total)
    assert wl.local.shape == (total, L + Ld) and wl.gathered is wl.local and Ld == D.section_doubles(T, nx, nu)
    S = PB.BatchMPC.SEEDS
    assert (S["A"], S["B"], S["h"]) == (307, 308, 309) and len(set(S.values())) == 9 and all(S[k] == v for k, v in PB.BatchHorizon.SEEDS.items())
    assert PB.BatchMPC(torch, 2, 2, 3, 1).m == 0                                # m defaults to no dense rows
    wl.local.fill_(float("nan"))
    wl.compute()
    torch.cuda.synchronize()
    hor, dyn = _fetch(wl)
    assert np.array_equal(bits(dyn[0].reshape(-1)), bits(O.fill_uniform(total * nx * nx, S["A"])))
    assert np.array_equal(bits(dyn[1].reshape(-1)), bits(O.fill_uniform(total * nx * nu, S["B"])))
    assert np.array_equal(bits(dyn[2].reshape(-1)), bits(O.fill_uniform(total * T * nx, S["h"])))
    assert np.array_equal(bits(wl.local.cpu().numpy()), bits(_rows(wl)))
    # one instance's MOI buffers
    n, i = wl.n, 5
    xvar, varmap = np.arange(1, n + 1, dtype=np.int64), (np.random.default_rng(1).permutation(n) + 1).astype(np.int64)
    d_x, d_map = g.to_dev(xvar), g.to_dev(varmap)
    quad, lin, const, vat, vc, terms, consts = wl.expand(i, d_x, d_map)
    torch.cuda.synchronize()
    Qt, Rt, r, v, Ct, d = hor
    rq, rl, rc, rv, rvc = H.expanded_reference(Qt[i].T, Rt[i].T, r[i], v[i], Ct[i].T, d[i], -1, 0, -1, xvar, varmap)
    assert np.array_equal(quad.cpu().numpy(), rq) and np.array_equal(lin.cpu().numpy(), rl) and np.array_equal(vat.cpu().numpy(), rv)
    assert bits(const.cpu().numpy())[0] == bits([rc])[0] and np.array_equal(bits(vc.cpu().numpy()), bits(rvc))
    want_t, want_c = D.expanded_reference(D.section_reference(*dyn, -1, -1, -1)[i], T, nx, nu, 1, xvar, varmap)
    assert np.array_equal(terms.cpu().numpy(), want_t) and np.array_equal(bits(consts.cpu().numpy()), bits(want_c))
    # .. which are the instance's own records x_t - A*x_{t-1} - B*u_{t-1} - h_t
    stages, nterms, nconsts = D.instance_stages(dyn[0][i].T, dyn[1][i].T, dyn[2][i], 1, -1, -1, -1, xvar)
    st, sc = U.images(stages, varmap, nterms, nconsts, -7)
    assert np.array_equal(want_t, st) and np.array_equal(bits(want_c), bits(sc))
    # another epoch: other data, the same relation
    wl.regenerate(1)
    wl.step(None)
    torch.cuda.synchronize()
    A1 = wl.A.cpu().numpy()
    assert not np.array_equal(A1, dyn[0].reshape(-1)) and np.array_equal(bits(A1), bits(O.fill_uniform(total * nx * nx, S["A"] + 1000)))
    assert np.array_equal(bits(wl.local.cpu().numpy()), bits(_rows(wl)))


def test_batch_mpc_sharding_is_data_independent():
    """the shards of rank 0 and rank 1 of world = 2, built on this one device, hold the rows world = 1 holds for the same instances"""
    from parametron_jl_amd import batch as PB
    total, T, nx, nu, m = 6, 4, 6, 3, 2
    names = ("Q", "R", "r", "v", "Cm", "d", "A", "Bm", "h")
    whole = PB.BatchMPC(torch, total, T, nx, nu, m)
    whole.step(None)
    parts, inputs = [], {k: [] for k in names}
    for rank in range(2):
        part = PB.BatchMPC(torch, total, T, nx, nu, m, rank=rank, world=2)
        assert (part.lo, part.hi, part.B) == (3 * rank, 3 * rank + 3, 3) and part.gathered.shape == (total, part.stride) and part.local.shape == (3, part.stride)
        part.compute()
        parts.append(part.local.clone())
        for k in names:
            inputs[k].append(getattr(part, k).clone())
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(torch.cat(inputs[k]), getattr(whole, k)), k
    assert torch.equal(torch.cat(parts), whole.local) and whole.gathered is whole.local
