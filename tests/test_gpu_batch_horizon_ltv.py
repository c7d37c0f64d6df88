"""-m gpu: the batch of horizons' time-varying dynamics sections pmt_batch_horizon_dynamics_tv_f64 / pmt_batch_horizon_dynamics_tv_expand_f64
(csrc/batch_horizon_ltv.hip) and their host classes batch.BatchLTVMPC / batch.BatchWeightedLTVMPC.

Every output lies inside a guarded buffer whose WHOLE image is compared bit for bit with the restatement of the header's text
(tests/batch_horizon_ltv_util.py; tests/test_batch_horizon_ltv_host.py checks that restatement against affine_stages_util's, the
time-invariant sibling's and the oracle): out_stride = Ltv + 3, and the guards in front and behind and the three words between two
sections must still hold the poison.  The values name their place — (instance, stage, row, column), negative where the indices' sum is
odd —, so a block of another item, a transposed index, a neighbour's entry or a dropped or doubled sign flip differs.  Beside the
restatement: with equal matrices per stage every block is what pmt_batch_horizon_dynamics_f64 writes in the same test, and an instance's
expansion equals, word for word, what pmt_affine_stages_f64 writes for tables that point into the same device inputs, stage t's matrix
parts at A_{i,t}, B_{i,t}.  Every size used is valid; nothing here provokes a fault."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import affine_stages_util as U  # noqa: E402
import batch_horizon_dyn_util as D  # noqa: E402
import batch_horizon_ltv_util as V  # noqa: E402
from test_gpu_batch_slabs import cus, dev_f64, image, owned  # noqa: E402

COEFFS, EXPAND = "pmt_batch_horizon_dynamics_tv_f64", "pmt_batch_horizon_dynamics_tv_expand_f64"
GAP = 3
bits = V.bits
# a shape of each path: 40 AB words a wave per pair; 17 x 32 the 32-row tile of 2048 words (w <= 64), 17 x 77 that of 4096
WAVE, TILE, FULL = (5, 3), (17, 15), (17, 60)


class LtvBatch:
    """a batch in the device layout, on the host and on the device; the restatement is computed once per sign triple"""

    def __init__(self, B, T, nx, nu, seed=None):
        self.B, self.T, self.nx, self.nu = B, T, nx, nu
        self.Ltv = V.section_doubles(T, nx, nu)
        self.host = list(V.encoded_data(B, T, nx, nu) if seed is None else V.ltv_data(B, T, nx, nu, np.random.default_rng(seed)))
        self.upload()

    def upload(self):
        self.dev = [dev_f64(h) for h in self.host]
        self.refs = {}

    def reference(self, signs):
        if signs not in self.refs:
            self.refs[signs] = V.section_reference(*self.host, *signs)
        return self.refs[signs].copy()

    def pointers(self, signs):
        """A and Bm are NULL where the contract does not read them: T == 1, Bm also with nu == 0; h where sign_h is 0"""
        p = [d[1] for d in self.dev]
        return p[0] if self.T > 1 else None, p[1] if self.T > 1 and self.nu else None, p[2] if signs[2] else None

    def run(self, signs=(-1, -1, -1), shift=0):
        """-> Guarded output of B * (Ltv + 3) doubles"""
        import gpu_util as g
        assert self.Ltv == g.lib().pmt_batch_horizon_dynamics_tv_doubles(self.T, self.nx, self.nu)
        out = g.Guarded(self.B * (self.Ltv + GAP), doubles=True, shift=shift)
        g.call(COEFFS, *self.pointers(signs), self.B, self.T, self.nx, self.nu, signs[0], signs[1], signs[2], out.ptr(), self.Ltv + GAP, g.stream())
        return out

    def check(self, signs=(-1, -1, -1), shift=0, what=""):
        out = self.run(signs, shift)
        out.check(image(out, self.reference(signs), self.Ltv + GAP),
                  "%s T=%d nx=%d nu=%d B=%d signs %r shift %d" % (what, self.T, self.nx, self.nu, self.B, signs, shift))
        return out


@functools.lru_cache(maxsize=4)
def batch(B, T, nx, nu):
    return LtvBatch(B, T, nx, nu)


def test_the_values_name_their_place():
    At, Bt, h = V.encoded_data(3, 4, 5, 3)
    words = np.concatenate([np.abs(At).reshape(-1), np.abs(Bt).reshape(-1), np.abs(h).reshape(-1)])
    assert len(np.unique(words)) == len(words) and np.any(At < 0) and np.any(At > 0) and np.any(h < 0) and np.any(Bt < 0)
    assert abs(At[2, 1, 3, 4]) == ((2 * 512 + 1) * 128 + 4) * 256 + 3 + 0.5 and abs(Bt[2, 1, 1, 4]) == ((2 * 512 + 1) * 128 + 4) * 256 + 5 + 1 + 0.5


# ---- 1. bit for bit against the restatement, at the path and tile edges

# (nx, nu): 512 words the wave path, 528 the 16-row tile; 17 rows the 32-row tile; 32 / 33 rows with w crossing 64; two row tiles with
# w = 128; w = 144 / 140 in the 16-row tile's 256 columns; 128 x 256; nu = 0; w = 128 / 129 at the 32-row tile's 128 columns; 529 words
# without a B and the wave path's largest nx; the tile of 2048 words against that of 4096: w = 64 / 65 at 32 rows, 128 / 129 at 16
PATHS = [(16, 16), (16, 17), (17, 15), (32, 33), (33, 31), (64, 64), (65, 63), (16, 128), (12, 128), (128, 128), (1, 0), (5, 0), (17, 111), (17, 112),
         (23, 0), (22, 1), (32, 32), (16, 112), (16, 113), (12, 116), (12, 117), (17, 60)]


@pytest.mark.parametrize("nx,nu", PATHS)
def test_sections_are_the_restatement_bit_for_bit(nx, nu):
    bt = batch(3, 3, nx, nu)
    bt.check((-1, -1, -1), what="path and tile edges")
    bt.check((1, -1, 1), what="path and tile edges")


# ---- 2. stage counts: no matrix at all, one, two, and more than 256

@pytest.mark.parametrize("nx,nu", [WAVE, TILE, FULL, (65, 10), (4, 0)])
@pytest.mark.parametrize("T", [1, 2, 3])
def test_stage_counts(T, nx, nu):
    """T == 1 is the constants alone, A and Bm NULL"""
    bt = batch(5, T, nx, nu)
    if T == 1:
        assert bt.pointers((-1, -1, -1))[:2] == (None, None) and bt.Ltv == nx
    bt.check((-1, -1, -1), what="stage counts")
    bt.check((1, 1, 0), what="stage counts, h NULL")


@pytest.mark.parametrize("nx,nu", [WAVE, TILE, FULL, (65, 10)])
def test_one_instance_of_300_stages(nx, nu):
    batch(1, 300, nx, nu).check((-1, 1, -1), what="B = 1, T = 300")


@pytest.mark.parametrize("nx,nu", [(2, 1), TILE, FULL])
def test_1500_instances_of_two_stages(nx, nu):
    batch(1500, 2, nx, nu).check((-1, 1, -1), what="T = 2, B = 1500")


# ---- 3. items against the resident grid: the item is the matrix pair

def _split(items):
    """(B, T - 1) with B * (T - 1) == items where a stage count in 2 .. 64 divides it, else the next multiple of 33"""
    for per in range(64, 1, -1):
        if items % per == 0:
            return items // per, per
    return -(-items // 33), 33


@pytest.mark.parametrize("nx,nu,per_cu", [TILE + (8,), FULL + (4,)])
def test_five_items_more_than_resident_workgroups_of_the_tile_kernel(nx, nu, per_cu):
    """eight workgroups per CU with the tile of 2048 words, four with that of 4096: five workgroups take a second item, which lies in
    another instance or at another stage"""
    B, per = _split(per_cu * cus() + 5)
    assert B * per >= per_cu * cus() + 5 and per > 1
    batch(B, per + 1, nx, nu).check((-1, -1, -1), what="resident workgroups + 5")


def test_seven_items_more_than_resident_waves_of_the_wave_path():
    """eight workgroups of four waves per CU"""
    B, per = _split(32 * cus() + 7)
    assert B * per >= 32 * cus() + 7
    batch(B, per + 1, 2, 1).check((-1, -1, -1), what="resident waves + 7")


def test_many_rounds_with_a_stride_that_is_no_multiple_of_the_stage_count():
    """(instance, stage) follows the item by adding (G / (T-1), G % (T-1)) with a carry: several rounds, T - 1 = 7 against G = 4 CUs"""
    B = -(-(3 * 4 * cus() + 11) // 7)
    batch(B, 8, *FULL).check((1, -1, -1), what="three rounds")


def test_position_independence():
    """the same instance data at positions 0, 1 and B - 1, and alone"""
    B, T = 9, 4
    for nx, nu in (WAVE, TILE, FULL):
        bt = LtvBatch(B, T, nx, nu, seed=5)
        for h in bt.host:
            h[1] = h[0]
            h[B - 1] = h[0]
        bt.upload()
        out = bt.check((-1, 1, -1), what="positions")
        got = owned(out).reshape(B, bt.Ltv + GAP)
        assert np.array_equal(bits(got[0, :bt.Ltv]), bits(got[1, :bt.Ltv])) and np.array_equal(bits(got[0, :bt.Ltv]), bits(got[B - 1, :bt.Ltv]))
        alone = LtvBatch(1, T, nx, nu, seed=0)
        alone.host = [np.ascontiguousarray(h[:1]) for h in bt.host]
        alone.upload()
        alone.run((-1, 1, -1)).check(np.concatenate([got[0, :bt.Ltv], np.full(GAP, np.nan)]), "the instance alone against in place")


# ---- 4. the three signs are three arguments

@pytest.mark.parametrize("sign_h", [-1, 0, 1])
@pytest.mark.parametrize("sign_b", [-1, 1])
@pytest.mark.parametrize("sign_a", [-1, 1])
@pytest.mark.parametrize("nx,nu", [WAVE, TILE, FULL])
def test_all_sign_triples(nx, nu, sign_a, sign_b, sign_h):
    B, T = 2, 3
    bt = batch(B, T, nx, nu)
    signs = (sign_a, sign_b, sign_h)
    want = bt.reference(signs)
    sec = V.sections(T, nx, nu)
    At, Bt, h = bt.host
    for s, blk in enumerate(sec["AB"]):
        ab = bits(want[:, blk]).reshape(B, nx, nx + nu)
        assert np.array_equal(ab[:, :, :nx] < 0, (bits(At[:, s]).transpose(0, 2, 1) < 0) ^ (sign_a < 0))
        assert np.array_equal(ab[:, :, nx:] < 0, (bits(Bt[:, s]).transpose(0, 2, 1) < 0) ^ (sign_b < 0))
    assert np.all(bits(want[:, sec["hconst"]]) == 0) == (sign_h == 0)
    bt.check(signs, what="signs")               # (h NULL where sign_h is 0)


def test_negative_zero_entries_keep_their_sign_bit_and_negative_zero_constants_do_not():
    for nx, nu in (WAVE, TILE):
        bt = LtvBatch(3, 3, nx, nu, seed=9)     # zeros of both signs among normals
        assert np.any(np.signbit(bt.host[0][bt.host[0] == 0.0])) and np.any(np.signbit(bt.host[2][bt.host[2] == 0.0]))
        for signs in ((-1, 1, -1), (1, -1, 1)):
            bt.check(signs, what="zeros of both signs")


# ---- 5. alignment and placement

@pytest.mark.parametrize("nx,nu", [WAVE, TILE, FULL, (65, 10)])
def test_section_base_eight_bytes_off_a_16_byte_boundary(nx, nu):
    """every section then starts 8 bytes off (the pitch Ltv + 3 is even at these shapes), and with nx*(nx + nu) odd (65 x 75) the blocks of
    one section start on either parity"""
    bt = batch(3, 3, nx, nu)
    out = bt.check((-1, 1, 1), shift=1, what="base 8 mod 16")
    assert out.ptr().value % 16 == 8


@pytest.mark.parametrize("nx,nu,T", [(65, 10, 3), (8, 3, 2)])
def test_slab_and_section_in_one_row_do_not_touch_each_other(nx, nu, T):
    """[L | Ltv | 3 words of gap] per instance: pmt_batch_horizon_coeffs_f64 (m = 0) and the new call at the stride L + Ltv + 3, out = slabs + L"""
    import gpu_util as g
    import batch_horizon_util as H
    from test_gpu_batch_horizon import HorizonBatch
    B = 3
    hb, bt = HorizonBatch(B, T, nx, nu, 0, seed=nx), batch(B, T, nx, nu)
    L, Ltv = hb.L, bt.Ltv
    stride = L + Ltv + GAP
    out = g.Guarded(B * stride, doubles=True)
    p = [d[1] for d in hb.dev]
    g.call("pmt_batch_horizon_coeffs_f64", p[0], p[1], p[2], p[3], p[4], p[5], B, T, nx, nu, 0, -1, 1, -1, out.ptr(), stride, g.stream())
    g.call(COEFFS, *bt.pointers((-1, -1, -1)), B, T, nx, nu, -1, -1, -1, C.c_void_p(out.ptr().value + 8 * L), stride, g.stream())
    assert L == H.slab_doubles(T, nx, nu, 0)
    rows = np.concatenate([hb.reference((-1, 1, -1)), bt.reference((-1, -1, -1))], axis=1)
    out.check(image(out, rows, stride), "slab and section in one row, nx=%d nu=%d T=%d" % (nx, nu, T))


# ---- 6. items do not see each other

@pytest.mark.parametrize("nx,nu", [WAVE, TILE, FULL, (65, 10)])
def test_nan_in_one_matrix_stays_in_its_block(nx, nu):
    signs, B, T = (-1, 1, 1), 3, 4
    bt = LtvBatch(B, T, nx, nu)
    want = bt.reference(signs)
    bt.check(signs, what="clean run")
    bt.host[0][1, 2, nx // 2, 0] = np.nan       # A_{1,3}[0, nx / 2]: block AB_3 of instance 1
    bt.host[2][1, T - 1, nx - 1] = np.nan       # the last constant of instance 1
    bt.upload()
    out = bt.run(signs)
    got = owned(out).reshape(B, bt.Ltv + GAP)
    nan_at = np.zeros(bt.Ltv, dtype=bool)
    nan_at[V.sections(T, nx, nu)["AB"][2].start + nx // 2] = nan_at[bt.Ltv - 1] = True
    assert np.array_equal(np.isnan(got[1, :bt.Ltv]), nan_at)
    expect = want.copy()
    expect[1, nan_at] = got[1, :bt.Ltv][nan_at]
    out.check(image(out, expect, bt.Ltv + GAP), "NaN in A_{1,3} and h of instance 1")


# ---- 7. the first anchor: equal matrices per stage

@pytest.mark.parametrize("nx,nu", [WAVE, (16, 16), (16, 17), TILE, FULL, (65, 10), (5, 0)])
def test_equal_matrices_give_the_blocks_the_time_invariant_launch_writes(nx, nu):
    import gpu_util as g
    B, T = 3, 4
    At1, Bt1, h = D.dyn_data(B, T, nx, nu, np.random.default_rng(nx + nu))
    bt = LtvBatch(B, T, nx, nu, seed=0)
    bt.host = [np.repeat(At1[:, None], T - 1, axis=1), np.repeat(Bt1[:, None], T - 1, axis=1), h]
    bt.upload()
    signs = (-1, 1, -1)
    got = owned(bt.check(signs, what="equal matrices")).reshape(B, bt.Ltv + GAP)
    Ld = D.section_doubles(T, nx, nu)
    sib = g.Guarded(B * (Ld + GAP), doubles=True)
    d = [dev_f64(a)[0] for a in (At1, Bt1, h)]
    g.call("pmt_batch_horizon_dynamics_f64", g.ptr(d[0]), g.ptr(d[1]) if nu else None, g.ptr(d[2]), B, T, nx, nu, *signs, sib.ptr(), Ld + GAP, g.stream())
    sib.check(image(sib, D.section_reference(At1, Bt1, h, *signs), Ld + GAP), "the sibling's sections")
    one = owned(sib).reshape(B, Ld + GAP)
    sv, si = V.sections(T, nx, nu), D.sections(T, nx, nu)
    for blk in sv["AB"]:
        assert np.array_equal(bits(got[:, blk]), bits(one[:, si["AB"]]))
    assert np.array_equal(bits(got[:, sv["hconst"]]), bits(one[:, si["hconst"]]))


# ---- 8. the second anchor: the expansion

def _device_tables(d_A, d_B, d_h, i, T, nx, nu, signs, d_x):
    """the instance's own tables for pmt_affine_stages_f64, pointing into the batch's device inputs — stage t's matrix parts at A_{i,t},
    B_{i,t}; through pmt_affine_stages_check"""
    from parametron_jl_amd import _lib
    sign_xp, sign_a, sign_b, sign_h = signs
    w, rl = nx + nu, 1 + nx + nu
    A_i, B_i = (d_A.value or 0) + 8 * i * (T - 1) * nx * nx, (d_B.value or 0) + 8 * i * (T - 1) * nx * nu
    h_i, x = d_h.value + 8 * i * T * nx, d_x.data_ptr()
    parts, stages = [], []
    for t in range(T):
        first = len(parts)
        parts.append({"mat": None, "ld": 0, "xvar": x + 8 * t * w, "cols": 1, "sign": sign_xp})
        if t:
            parts.append({"mat": A_i + 8 * (t - 1) * nx * nx, "ld": nx, "xvar": x + 8 * (t - 1) * w, "cols": nx, "sign": sign_a})
            if nu:
                parts.append({"mat": B_i + 8 * (t - 1) * nx * nu, "ld": nx, "xvar": x + 8 * ((t - 1) * w + nx), "cols": nu, "sign": sign_b})
        stages.append({"vec": h_i + 8 * t * nx if sign_h else None, "vec_sign": sign_h, "rows": nx, "first_part": first, "nparts": len(parts) - first,
                       "row_len": rl if t else 1, "term_offset": nx + (t - 1) * nx * rl if t else 0, "const_offset": t * nx})
    parr, sarr = _lib.affine_parts(parts), _lib.affine_stages(stages)
    _lib.call("pmt_affine_stages_check", C.addressof(sarr), T, C.addressof(parr), len(parts), V.term_count(T, nx, nu), T * nx)
    to = lambda arr: torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()).to("cuda:0")
    return to(sarr), to(parr)


# both sides of each path threshold of the launch that wrote the section (512 words; 16 and 32 rows), T = 1 and 2, nu = 0, many stages
@pytest.mark.parametrize("T,nx,nu", [(1, 5, 3), (2, 1, 0), (3, 16, 16), (3, 16, 17), (3, 17, 15), (3, 32, 32), (3, 32, 33), (3, 33, 31), (4, 128, 33), (3, 64, 64),
                                     (130, 5, 2), (512, 2, 1)])
def test_expansion_equals_the_restatement_and_the_stage_node_on_the_same_device_inputs(T, nx, nu):
    import gpu_util as g
    B, i = 2, 1
    bt = batch(B, T, nx, nu)
    n, nterms = T * (nx + nu), V.term_count(T, nx, nu)
    rng = np.random.default_rng(n)
    xvar = np.sort(rng.choice(np.arange(1, n + 10), n, replace=False)).astype(np.int64)
    perm = (rng.permutation(n + 9) + 1 + 100).astype(np.int64)
    d_x, d_map = g.to_dev(xvar), g.to_dev(perm)
    # (sign_xp, sign_a, sign_b, sign_h), the varmap, the term buffer's shift
    for signs, varmap, shift in (((1, -1, -1, -1), perm, 1), ((-1, 1, -1, 1), None, 0), ((1, -1, 1, 0), perm, 0)):
        out = bt.check(signs[1:], what="the sections")
        section = owned(out).reshape(B, bt.Ltv + GAP)[i, :bt.Ltv]
        ot, oc = g.Guarded(3 * nterms, shift=shift), g.Guarded(T * nx, doubles=True, shift=shift)
        assert ot.ptr().value % 16 == 8 * shift and oc.ptr().value % 16 == 8 * shift
        g.call(EXPAND, C.c_void_p(out.ptr().value + 8 * i * (bt.Ltv + GAP)), T, nx, nu, signs[0], g.ptr(d_x), g.ptr(d_map) if varmap is not None else None,
               ot.ptr(), oc.ptr(), g.stream())
        want_t, want_c = V.expanded_reference(section, T, nx, nu, signs[0], xvar, varmap)
        ot.check(want_t, "expanded terms %r" % (signs,))
        oc.check(want_c, "expanded constants %r" % (signs,))
        # the single-model node on tables that point into the same device inputs
        stable, ptable = _device_tables(bt.dev[0][1], bt.dev[1][1], bt.dev[2][1], i, T, nx, nu, signs, d_x)
        nt, nc = g.Guarded(3 * nterms, shift=shift), g.Guarded(T * nx, doubles=True, shift=shift)
        g.call("pmt_affine_stages_f64", g.ptr(stable), T, g.ptr(ptable), g.ptr(d_map) if varmap is not None else None, nt.ptr(), nc.ptr(), g.stream())
        nt.check(want_t, "pmt_affine_stages_f64's terms %r" % (signs,))
        nc.check(want_c, "pmt_affine_stages_f64's constants %r" % (signs,))
        torch.cuda.synchronize()
        assert torch.equal(ot.buf, nt.buf) and torch.equal(oc.buf.view(torch.int64), nc.buf.view(torch.int64))


# ---- 9. batch.BatchLTVMPC, batch.BatchWeightedLTVMPC

def _dynamics(wl):
    f = lambda t, *shape: t.cpu().numpy().reshape(wl.B, *shape)
    return f(wl.A, wl.Td - 1, wl.nx, wl.nx), f(wl.Bm, wl.Td - 1, wl.nu, wl.nx), f(wl.h, wl.Td, wl.nx)


def _check_dynamics_of(wl, S, section, i, xvar, varmap, terms, consts):
    """the dynamics inputs are their seeds' streams, instance i's records are its own tables'"""
    from oracle import oracle as O
    At, Bt, h = _dynamics(wl)
    Td, nx, nu = wl.Td, wl.nx, wl.nu
    assert np.array_equal(bits(At.reshape(-1)), bits(O.fill_uniform(wl.total * (Td - 1) * nx * nx, S["A"])))
    assert np.array_equal(bits(Bt.reshape(-1)), bits(O.fill_uniform(wl.total * (Td - 1) * nx * nu, S["B"])))
    assert np.array_equal(bits(h.reshape(-1)), bits(O.fill_uniform(wl.total * Td * nx, S["h"])))
    want_t, want_c = V.expanded_reference(section[i], Td, nx, nu, 1, xvar, varmap)
    assert len(want_t) == 3 * V.term_count(Td, nx, nu) and len(want_c) == Td * nx
    assert np.array_equal(terms.cpu().numpy(), want_t) and np.array_equal(bits(consts.cpu().numpy()), bits(want_c))
    A, Bm = V.matrices(At[i], Bt[i])
    stages, nterms, nconsts = V.instance_stages(A, Bm, h[i], 1, -1, -1, -1, xvar)
    st, sc = U.images(stages, varmap, nterms, nconsts, -7)
    assert np.array_equal(want_t, st) and np.array_equal(bits(want_c), bits(sc))
    return want_t


def test_batch_ltv_mpc_compute_gather_and_expand_equal_the_restatement_on_its_inputs():
    import gpu_util as g
    import batch_horizon_util as H
    from parametron_jl_amd import batch as PB
    total, T, nx, nu, m = 37, 4, 6, 3, 2
    wl = PB.BatchLTVMPC(torch, total, T, nx, nu, m)
    (off, L), (doff, Ltv) = PB.horizon_slab_layout(T, nx, nu, m), PB.horizon_dynamics_tv_layout(T, nx, nu)
    assert (wl.offsets, wl.L, wl.dyn_offsets, wl.Ltv, wl.stride, wl.Td, wl.lo, wl.hi, wl.B) == (off, L, doff, Ltv, L + Ltv, T, 0, total, total)
    assert wl.local.shape == (total, L + Ltv) and wl.gathered is wl.local and Ltv == V.section_doubles(T, nx, nu)
    S = PB.BatchLTVMPC.SEEDS
    taken = set(PB.BatchLSQ.SEEDS.values()) | set(PB.BatchTracking.SEEDS.values()) | set(PB.BatchMPC.SEEDS.values()) | set(PB.BatchWeightedMPC.SEEDS.values())
    assert len(set(S.values())) == 9 and all(S[k] == v for k, v in PB.BatchHorizon.SEEDS.items()) and {S["A"], S["B"], S["h"]}.isdisjoint(taken)
    assert PB.BatchLTVMPC(torch, 2, 2, 3, 1).m == 0                             # m defaults to no dense rows
    wl.local.fill_(float("nan"))
    wl.compute()
    wl.gather(None)                                                             # world = 1: the rows are the gathered rows
    torch.cuda.synchronize()
    f = lambda t, *shape: t.cpu().numpy().reshape(total, *shape)
    hor = (f(wl.Q, nx, nx), f(wl.R, nu, nu), f(wl.r, T, nx), f(wl.v, T, nu), f(wl.Cm, wl.n, m), f(wl.d, m))
    section = V.section_reference(*_dynamics(wl), -1, -1, -1)
    rows = np.concatenate([H.horizon_slab_reference(*hor, -1, 0, -1), section], axis=1)
    assert np.array_equal(bits(wl.gathered.cpu().numpy()), bits(rows))
    n, i = wl.n, 5
    xvar, varmap = np.arange(1, n + 1, dtype=np.int64), (np.random.default_rng(1).permutation(n) + 1).astype(np.int64)
    quad, lin, const, vat, vc, terms, consts = wl.expand(i, g.to_dev(xvar), g.to_dev(varmap))
    torch.cuda.synchronize()
    Qt, Rt, r, v, Ct, d = hor
    rq, rl, rc, rv, rvc = H.expanded_reference(Qt[i].T, Rt[i].T, r[i], v[i], Ct[i].T, d[i], -1, 0, -1, xvar, varmap)
    assert np.array_equal(quad.cpu().numpy(), rq) and np.array_equal(lin.cpu().numpy(), rl) and np.array_equal(vat.cpu().numpy(), rv)
    assert bits(const.cpu().numpy())[0] == bits([rc])[0] and np.array_equal(bits(vc.cpu().numpy()), bits(rvc))
    _check_dynamics_of(wl, S, section, i, xvar, varmap, terms, consts)
    # another epoch: other data, the same relation
    A0 = wl.A.clone()
    wl.regenerate(1)
    wl.step(None)
    torch.cuda.synchronize()
    assert not torch.equal(A0, wl.A)
    hor = (f(wl.Q, nx, nx), f(wl.R, nu, nu), f(wl.r, T, nx), f(wl.v, T, nu), f(wl.Cm, wl.n, m), f(wl.d, m))
    rows = np.concatenate([H.horizon_slab_reference(*hor, -1, 0, -1), V.section_reference(*_dynamics(wl), -1, -1, -1)], axis=1)
    assert np.array_equal(bits(wl.local.cpu().numpy()), bits(rows))


def test_batch_weighted_ltv_mpc_with_a_terminal_stage():
    """Td = T + 1 records, up to x_T == A_T*x_{T-1} + B_T*u_{T-1} + h_T; the n = T*(nx + nu) + nx variables suffice"""
    import gpu_util as g
    import batch_horizon_terms_util as HT
    from test_gpu_batch_horizon_terms import _fetch
    from parametron_jl_amd import batch as PB
    total, T, nx, nu, m = 5, 4, 6, 3, 2
    wl = PB.BatchWeightedLTVMPC(torch, total, T, nx, nu, m, terminal=True)
    Td = T + 1
    (off, L), (doff, Ltv) = PB.horizon_terms_slab_layout(T, nx, nu, m, True), PB.horizon_dynamics_tv_layout(Td, nx, nu)
    assert (wl.offsets, wl.L, wl.dyn_offsets, wl.Ltv, wl.stride, wl.Td) == (off, L, doff, Ltv, L + Ltv, Td) and wl.local.shape == (total, L + Ltv)
    assert Ltv == V.section_doubles(Td, nx, nu) and PB.BatchWeightedLTVMPC(torch, 2, 2, 3, 1).m == 0
    assert PB.BatchWeightedLTVMPC(torch, 2, 2, 3, 1, terminal=False).Td == 2
    S = PB.BatchWeightedLTVMPC.SEEDS
    taken = set(PB.BatchLSQ.SEEDS.values()) | set(PB.BatchTracking.SEEDS.values()) | set(PB.BatchMPC.SEEDS.values()) | set(PB.BatchWeightedMPC.SEEDS.values()) \
        | set(PB.BatchLTVMPC.SEEDS.values())
    assert len(set(S.values())) == 17 and all(S[k] == v for k, v in PB.BatchWeightedHorizon.SEEDS.items()) and {S["A"], S["B"], S["h"]}.isdisjoint(taken)
    wl.local.fill_(float("nan"))
    wl.compute()
    wl.gather(None)
    torch.cuda.synchronize()
    b = _fetch(wl)
    signs = (-1, 0, -1, -1)
    section = V.section_reference(*_dynamics(wl), -1, -1, -1)
    assert np.array_equal(bits(wl.gathered.cpu().numpy()), bits(np.concatenate([HT.slab_reference(b, signs), section], axis=1)))
    n, i = wl.n, 3
    assert n == T * (nx + nu) + nx
    xvar, varmap = np.arange(1, n + 1, dtype=np.int64), (np.random.default_rng(2).permutation(n) + 1).astype(np.int64)
    d_x = g.to_dev(xvar)
    assert d_x.numel() == n
    quad, lin, const, vat, vc, terms, consts = wl.expand(i, d_x, g.to_dev(varmap))
    torch.cuda.synchronize()
    rq, rl, rc, rv, rvc = HT.expanded_reference(HT.instance(b, i, signs), xvar, varmap)
    assert np.array_equal(quad.cpu().numpy(), rq) and np.array_equal(lin.cpu().numpy(), rl) and np.array_equal(vat.cpu().numpy(), rv)
    assert bits(const.cpu().numpy())[0] == bits([rc])[0] and np.array_equal(bits(vc.cpu().numpy()), bits(rvc))
    want_t = _check_dynamics_of(wl, S, section, i, xvar, varmap, terms, consts)
    last = want_t.reshape(-1, 3)[V.term_count(T, nx, nu):].reshape(nx, 1 + nx + nu, 3)
    assert np.array_equal(last[:, 0, 2], varmap[xvar[T * (nx + nu):] - 1])     # the last record's x_+ part is x_T, the last nx variables of z


def test_sharding_is_data_independent():
    """the shards of rank 0 and rank 1 of world = 2, built on this one device, hold the rows world = 1 holds for the same instances"""
    from parametron_jl_amd import batch as PB
    total, T, nx, nu, m = 6, 4, 6, 3, 2
    whole = PB.BatchLTVMPC(torch, total, T, nx, nu, m)
    whole.step(None)
    parts, dyn = [], {k: [] for k in ("A", "Bm", "h")}
    for rank in range(2):
        part = PB.BatchLTVMPC(torch, total, T, nx, nu, m, rank=rank, world=2)
        assert (part.lo, part.hi, part.B) == (3 * rank, 3 * rank + 3, 3) and part.gathered.shape == (total, part.stride) and part.local.shape == (3, part.stride)
        part.compute()
        parts.append(part.local.clone())
        for k in dyn:
            dyn[k].append(getattr(part, k).clone())
    torch.cuda.synchronize()
    for k in dyn:
        assert torch.equal(torch.cat(dyn[k]), getattr(whole, k)), k
    assert torch.equal(torch.cat(parts), whole.local) and whole.gathered is whole.local
