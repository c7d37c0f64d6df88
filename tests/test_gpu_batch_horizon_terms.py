"""-m gpu: the batched horizons with a terminal cost, stage weights and linear stage terms — pmt_batch_horizon_terms_coeffs_f64 /
pmt_batch_horizon_terms_expand_f64 (csrc/batch_horizon_terms.hip) and their host classes batch.BatchWeightedHorizon / BatchWeightedMPC.

Every output lies inside a guarded buffer whose WHOLE image is compared bit for bit with the numpy restatement of the header's order
(tests/batch_horizon_terms_util.py; tests/test_batch_horizon_terms_host.py checks that restatement against quad_stages_terms_util's, the
sibling's and the oracle): out_stride = L + 3, and the guards in front and behind and the three words between two slabs must still hold the
poison.  The data is the sibling's (full mantissas, mixed magnitudes, zeros of both signs, pairs M[j,k] = -M[k,j]); the weights come from a
pool with negative ones, zeros of both signs and numbers that are no power of two, so a weight applied at another place, a neighbour's
weight or a dropped sign of zero differs.  Beside the restatement: an instance's slab and its expansion equal, word for word, what
pmt_quad_stages_terms_f64 writes for that instance's own table, and without the optional arrays the slab is the parent entry point's.
Every size used is valid; nothing here provokes a fault."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import batch_horizon_dyn_util as D  # noqa: E402
import batch_horizon_terms_util as HT  # noqa: E402
import batch_horizon_util as H  # noqa: E402
from test_gpu_batch_slabs import cus, dev_f64, image, owned  # noqa: E402

COEFFS, EXPAND = "pmt_batch_horizon_terms_coeffs_f64", "pmt_batch_horizon_terms_expand_f64"
GAP = 3
OPTIONAL = ("wx", "wu", "wN", "gx", "gu", "gN")
FULL = (-1, 1, -1, -1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


class TermsBatch:
    """a batch in the device layout, on the host and on the device; the restatement is computed once per (signs, dropped arrays)"""

    def __init__(self, B, T, nx, nu, m, seed, terminal=True, weights=True, linear=True):
        self.B, self.T, self.nx, self.nu, self.m, self.term = B, T, nx, nu, m, 1 if terminal else 0
        self.L = HT.slab_doubles(T, nx, nu, self.term, m)
        self.host = HT.terms_data(B, T, nx, nu, m, np.random.default_rng(seed), terminal, weights, linear)
        self.upload()

    def upload(self):
        self.dev = {k: dev_f64(self.host[k]) for k in HT.KEYS if self.host.get(k) is not None}
        self.refs = {}

    def given(self, signs, drop):
        """the arrays the call gets: a reference only where its sign is not 0, an optional array unless dropped"""
        ref_sign = {"r": signs[0], "v": signs[1], "rN": signs[2]}
        return [k for k in self.dev if k not in drop and ref_sign.get(k, 1)]

    def reference(self, signs=FULL, drop=()):
        key = (tuple(signs), tuple(sorted(drop)))
        if key not in self.refs:
            b = dict(self.host)
            b.update({k: None for k in drop})
            self.refs[key] = HT.slab_reference(b, signs)
        return self.refs[key].copy()

    def descriptor(self, signs=FULL, drop=()):
        from parametron_jl_amd import _lib
        fields = {HT.FIELDS[k]: self.dev[k][1].value for k in self.given(signs, drop)}
        return _lib.batch_horizon_terms(sign_r=signs[0], sign_v=signs[1], sign_rN=signs[2], sign_d=signs[3], **fields)

    def run(self, signs=FULL, shift=0, drop=()):
        """-> Guarded output of B * (L + 3) doubles"""
        import gpu_util as g
        assert self.L == g.lib().pmt_batch_horizon_terms_slab_doubles(self.T, self.nx, self.nu, self.term, self.m)
        out = g.Guarded(self.B * (self.L + GAP), doubles=True, shift=shift)
        desc = self.descriptor(signs, drop)
        g.call(COEFFS, C.byref(desc), self.B, self.T, self.nx, self.nu, self.m, out.ptr(), self.L + GAP, g.stream())
        return out

    def check(self, signs=FULL, shift=0, drop=(), what=""):
        out = self.run(signs, shift, drop)
        out.check(image(out, self.reference(signs, drop), self.L + GAP), "%s T=%d nx=%d nu=%d m=%d term=%d B=%d signs %r drop %r shift %d" % (
            what, self.T, self.nx, self.nu, self.m, self.term, self.B, signs, drop, shift))
        return out


@functools.lru_cache(maxsize=4)
def batch(B, T, nx, nu, m, terminal=True):
    return TermsBatch(B, T, nx, nu, m, seed=17 + 1000 * nx + 10 * nu + T + m, terminal=terminal)


def b_many():
    return 3 * cus() + 37                       # dims <= 64: three workgroups a CU are resident — every workgroup gets a second instance, 37 a third


# ---- a. bit for bit against the restatement: lane packing (16, 32, 64 lanes a stage), one and three tiles, more than one round

# nx over {1, 16, 17, 32, 33, 64, 65, 128}; nu in {0, 3, 65} where it changes the path (no u stages | packed | two waves, and the kernel of
# three tiles for a small nx); T in {1, 2, 17}: 17 stages are more than one round at 16, 8, 4 stages (or 2) a round
EDGES = [(1, 0, 1, True), (1, 3, 17, False), (16, 0, 17, True), (16, 65, 17, False), (17, 3, 2, True), (32, 0, 17, False), (33, 3, 17, True),
         (64, 65, 2, True), (64, 0, 1, False), (65, 0, 17, True), (65, 3, 1, False), (128, 65, 2, True), (128, 0, 1, True), (128, 3, 17, False)]


@pytest.mark.parametrize("nx,nu,T,terminal", EDGES)
def test_slabs_are_the_restatement_bit_for_bit(nx, nu, T, terminal):
    bt = TermsBatch(3, T, nx, nu, 5 if nx % 2 else 0, seed=nx + 7 * nu + T, terminal=terminal)
    bt.check((-1, -1, -1, -1), what="tile edges")
    bt.check((1, 1, 1, 1), what="tile edges")


# ---- b. the stage constants' capacity

@pytest.mark.parametrize("T,nx,nu", [(129, 3, 2), (512, 2, 1), (512, 2, 0)])
def test_stage_constant_capacity(T, nx, nu):
    """259 stage constants: chain c of the constant adds the stages c, c + 256; 1025 = 2 * 512 + 1: the last word of the kernel's table; 513"""
    bt = TermsBatch(2, T, nx, nu, 1, seed=T)
    assert T * (2 if nu else 1) + 1 in (259, 1025, 513)
    bt.check((-1, 1, -1, -1), what="stage constants")


# ---- c. signs, weights, linear vectors

@pytest.mark.parametrize("sign_rN", [-1, 0, 1])
@pytest.mark.parametrize("sign_v", [-1, 0, 1])
@pytest.mark.parametrize("sign_r", [-1, 0, 1])
def test_all_sign_triples(sign_r, sign_v, sign_rN):
    T, nx, nu, m = 3, 65, 10, 4
    bt = batch(2, T, nx, nu, m)
    signs = (sign_r, sign_v, sign_rN, (sign_r + sign_v + sign_rN) % 3 - 1)      # (sign_d comes round as well)
    bt.check(signs, what="signs")                                               # (references NULL where their sign is 0)
    # the plain stages without linear vectors: W_s * +0.0, -0.0 under a negative weight
    want = bt.reference(signs, ("gx", "gu", "gN"))
    sec = HT.sections(T, nx, nu, 1, m)
    q = want[:, sec["q"]][:, :T * (nx + nu)].reshape(2, T, nx + nu)
    for part, s, wts in ((q[:, :, :nx], sign_r, bt.host["wx"]), (q[:, :, nx:], sign_v, bt.host["wu"])):
        if s == 0:
            assert np.array_equal(bits(part), bits(wts[:, :, None] * np.zeros(part.shape)))
    bt.check(signs, drop=("gx", "gu", "gN"), what="signs, no linear vectors")


@pytest.mark.parametrize("drop", [OPTIONAL, ("wx", "wu", "wN"), ("gx", "gu", "gN"), ("gu", "gN"), ("gx", "gN"), ("gx", "gu"), ("wx",), ("wu", "gN"), ("wN", "gx")],
                         ids=lambda d: "without-" + "-".join(d))
def test_optional_arrays_are_optional_one_by_one(drop):
    """weights absent or present per kind of stage; linear vectors on x only, on u only, on the terminal stage only"""
    bt = batch(2, 3, 65, 10, 4)
    bt.check((-1, 1, -1, -1), drop=drop, what="optional arrays")
    bt.check((0, 0, 0, 1), drop=drop, what="optional arrays, plain stages")


def test_zero_and_negative_weights():
    """a weight of 0 switches a stage off: its q words are its linear vector (or a zero of the weight's sign), its constant a zero"""
    T, nx, nu, m = 17, 20, 3, 0
    bt = TermsBatch(2, T, nx, nu, m, seed=3)
    bt.host["wx"][:] = 0.0
    bt.host["wu"][0], bt.host["wu"][1] = -0.0, -1.0
    bt.host["wN"][:] = [0.0, -3.0]
    bt.upload()
    sec = HT.sections(T, nx, nu, 1, m)
    want = bt.reference((-1, 1, -1, 0), ("gx", "gu", "gN"))
    q = want[:, sec["q"]][:, :T * (nx + nu)].reshape(2, T, nx + nu)
    assert np.all(q[:, :, :nx] == 0) and np.all(q[0] == 0) and np.any(q[1, :, nx:] != 0) and np.any(bits(q[:, :, :nx]) != 0)
    assert bits(want[0, sec["const"]])[0] in (0, np.int64(-2 ** 63)) and want[1, sec["const"]][0] != 0
    bt.check((-1, 1, -1, 0), drop=("gx", "gu", "gN"), what="zero weights")
    bt.check((-1, 1, -1, 0), what="zero weights, linear vectors")
    bt.check((0, 0, 0, 0), what="zero weights, plain stages")


# ---- d. a NaN weight stays in its stage and its instance

def _nan_weight(B, T, nx, nu, victims, seed):
    signs = (-1, 1, -1, 1)
    bt = TermsBatch(B, T, nx, nu, 1, seed=seed)
    want = bt.reference(signs)
    bt.check(signs, what="clean run")
    sec = HT.sections(T, nx, nu, 1, 1)
    stride, w = bt.L + GAP, nx + nu
    for name, t in (("wx", T - 1), ("wu", 0), ("wN", None)):
        saved = bt.host[name].copy()
        for k in victims:
            if t is None:
                bt.host[name][k] = np.nan
            else:
                bt.host[name][k, t] = np.nan
        bt.upload()
        out = bt.run(signs)
        got = owned(out).reshape(B, stride)
        expect = want.copy()
        s, at, nd = {"wx": (2 * t if t is not None else 0, (t or 0) * w, nx), "wu": (1, nx, nu), "wN": (2 * T, T * w, nx)}[name]
        for k in victims:
            words = np.concatenate([np.arange(sec["q"].start + at, sec["q"].start + at + nd), [sec["const"].start, sec["W"].start + s]])
            assert np.isnan(got[k, words]).all(), "instance %d: the NaN weight did not reach its stage" % k
            expect[k, words] = got[k, words]                                    # (a NaN's payload is not part of the contract)
        out.check(image(out, expect, stride), "NaN in %s of instances %r" % (name, victims))
        bt.host[name] = saved
    bt.upload()


def test_a_nan_weight_stays_in_its_stage_and_its_instance():
    _nan_weight(5, 3, 65, 10, [2], seed=21)


def test_a_nan_weight_stays_in_its_slab_on_a_shared_workgroup():
    """instances k - G, k and k + G run on one persistent workgroup, one after the other, through the same LDS"""
    B, G = b_many(), 3 * cus()
    assert B > G
    _nan_weight(B, 2, 3, 2, [5 + G, B - 1], seed=22)


# ---- e. more instances than resident workgroups; position independence

def test_more_instances_than_resident_workgroups_and_position_independence():
    B, T, nx, nu, m = 2000, 2, 3, 2, 1
    assert B > 3 * cus()
    bt = TermsBatch(B, T, nx, nu, m, seed=5)
    for k in HT.KEYS:                            # the same instance data at positions 0, 1 and B - 1
        bt.host[k][1] = bt.host[k][0]
        bt.host[k][B - 1] = bt.host[k][0]
    bt.upload()
    out = bt.check(FULL, what="persistent loop")
    got = owned(out).reshape(B, bt.L + GAP)
    assert np.array_equal(bits(got[0, :bt.L]), bits(got[1, :bt.L])) and np.array_equal(bits(got[0, :bt.L]), bits(got[B - 1, :bt.L]))
    alone = TermsBatch(1, T, nx, nu, m, seed=0)
    alone.host = dict(bt.host, **{k: np.ascontiguousarray(bt.host[k][:1]) for k in HT.KEYS})
    alone.upload()
    o1 = alone.run(FULL)
    o1.check(np.concatenate([got[0, :bt.L], np.full(GAP, np.nan)]), "the instance alone against in place")


# ---- f. a slab base 8 mod 16

@pytest.mark.parametrize("nx,nu,T,m", [(65, 10, 3, 4), (8, 3, 2, 1), (128, 33, 2, 0)])
def test_slab_base_eight_bytes_off_a_16_byte_boundary(nx, nu, T, m):
    """with the odd / even pitch L + 3 the later slabs start on either parity"""
    bt = batch(2, T, nx, nu, m)
    out = bt.check(FULL, shift=1, what="base 8 mod 16")
    assert out.ptr().value % 16 == 8


# ---- g. against the single-instance node

@pytest.mark.parametrize("T,nx,nu", [(3, 65, 10), (4, 128, 33), (130, 5, 2)])
def test_slab_and_expansion_equal_the_stage_node_for_the_instance_s_own_table(T, nx, nu):
    """pmt_quad_stages_terms_check + pmt_quad_stages_terms_f64 on the instance's own table [x_0, u_0, .., x_T] (scale = 1.0, weight = &W_s,
    lin_vec = g_s; stages one behind the other, a non-trivial varmap): W * section, q and const of the slab are its coefficients word for
    word, pmt_batch_horizon_terms_expand_f64 of the slab its buffers whole, and the constraint block the restatement's"""
    import gpu_util as g
    from test_gpu_quad_stages_terms import Launch
    B, m, i = 2, 4, 1
    bt = TermsBatch(B, T, nx, nu, m, seed=T + nx)
    n = T * (nx + nu) + nx
    rng = np.random.default_rng(n)
    xvar = np.sort(rng.choice(np.arange(1, n + 10), n, replace=False)).astype(np.int64)
    varmap = (rng.permutation(n + 9) + 1 + 100).astype(np.int64)
    d_x, d_map = g.to_dev(xvar), g.to_dev(varmap)
    sec = HT.sections(T, nx, nu, 1, m)
    for signs, drop in (((-1, 0, -1, -1), ()), ((1, -1, 0, 1), ("gu",)), ((0, 1, 1, -1), ("wx", "wu", "wN"))):
        out = bt.check(signs, drop=drop, what="against the node")
        slab = owned(out).reshape(B, bt.L + GAP)[i, :bt.L]
        b = dict(bt.host)
        b.update({k: None for k in drop})
        inst = HT.instance(b, i, signs)
        stages, nterms, nlin = HT.instance_table(inst, xvar)
        node = Launch(stages, [], varmap, nterms, nlin).run()
        quad, lin, consts, const = node.host()
        assert np.array_equal(lin.reshape(-1, 2)[:, 0], bits(slab[sec["q"]])) and bits([const])[0] == bits(slab[sec["const"]])[0]
        qc = quad.reshape(-1, 3)[:, 0].view(np.float64)
        for s, st in enumerate(stages):
            nd = len(st["xvar"])
            S = slab[sec["SP" if s == len(stages) - 1 else ("SQ", "SR")[s % 2]]]
            assert np.array_equal(bits(qc[st["quad_at"]:st["quad_at"] + nd * (nd + 1) // 2]), bits(slab[sec["W"]][s] * S)), s
        # the expansion: whole buffers, the quadratic terms at an address 8 mod 16
        oq, ol, oc = g.Guarded(3 * nterms, shift=1), g.Guarded(2 * n), g.Guarded(1, doubles=True)
        ov, ovc = g.Guarded(3 * m * n, shift=1), g.Guarded(m, doubles=True)
        slab_ptr = C.c_void_p(out.ptr().value + 8 * i * (bt.L + GAP))
        g.call(EXPAND, slab_ptr, T, nx, nu, 1, m, g.ptr(d_x), g.ptr(d_map), oq.ptr(), ol.ptr(), oc.ptr(), ov.ptr(), ovc.ptr(), g.stream())
        oq.check(quad, "expanded quadratic terms against the node %r" % (signs,))
        ol.check(lin, "expanded linear terms against the node")
        oc.check(np.array([const]), "expanded constant against the node")
        rq, rl, rc, rv, rvc = HT.expanded_reference(inst, xvar, varmap)
        oq.check(rq, "expanded quadratic terms")
        ol.check(rl, "expanded linear terms")
        ov.check(rv, "expanded constraint terms")
        ovc.check(rvc, "expanded constraint constants")


def test_expansion_without_inputs_terminal_stage_or_constraints():
    """nu == 0, term == 0 and m == 0: the table is [x_0, x_1, ..], out_vat / out_vconsts may be NULL; an empty batch writes nothing"""
    import gpu_util as g
    T, nx = 5, 70
    bt = TermsBatch(1, T, nx, 0, 0, seed=3, terminal=False)
    n = T * nx
    xvar, varmap = np.arange(2, n + 2, dtype=np.int64), (np.arange(n + 1, dtype=np.int64)[::-1] + 50).copy()
    signs = (-1, 0, 0, 0)
    out = bt.check(signs, what="nu == 0, term == 0, m == 0")
    oq, ol, oc = g.Guarded(3 * T * nx * (nx + 1) // 2), g.Guarded(2 * n, shift=1), g.Guarded(1, doubles=True)
    d_x, d_map = g.to_dev(xvar), g.to_dev(varmap)
    g.call(EXPAND, out.ptr(), T, nx, 0, 0, 0, g.ptr(d_x), g.ptr(d_map), oq.ptr(), ol.ptr(), oc.ptr(), None, None, g.stream())
    rq, rl, rc, rv, rvc = HT.expanded_reference(HT.instance(bt.host, 0, signs), xvar, varmap)
    oq.check(rq, "quadratic terms")
    ol.check(rl, "linear terms")
    oc.check(np.array([rc]), "constant")
    empty = g.Guarded(8, doubles=True)
    desc = bt.descriptor(signs)
    g.call(COEFFS, C.byref(desc), 0, T, nx, 0, 0, empty.ptr(), bt.L, g.stream())
    empty.check(empty.padding(8), "B == 0")


# ---- h. without the optional arrays: the parent entry point's slab

@pytest.mark.parametrize("T,nx,nu,m", [(3, 65, 10, 4), (17, 20, 3, 0), (2, 128, 0, 1)])
def test_without_the_optionals_the_slab_minus_w_is_the_parent_entry_point_s(T, nx, nu, m):
    import gpu_util as g
    B = 3
    bt = TermsBatch(B, T, nx, nu, m, seed=T + nu, terminal=False, weights=False, linear=False)
    Lp = H.slab_doubles(T, nx, nu, m)
    sec = HT.sections(T, nx, nu, 0, m)
    p = {k: v[1] for k, v in bt.dev.items()}
    for sr, sv, sd in ((-1, 0, -1), (1, -1, 1), (0, 0, 0)):
        out = bt.check((sr, sv, 0, sd), what="no optionals")
        parent = g.Guarded(B * (Lp + GAP), doubles=True)
        g.call("pmt_batch_horizon_coeffs_f64", p["Qt"], p["Rt"], p["r"] if sr else None, p["v"] if sv else None, p["Ct"], p["d"], B, T, nx, nu, m,
               sr, sv, sd, parent.ptr(), Lp + GAP, g.stream())
        got = owned(out).reshape(B, bt.L + GAP)[:, :bt.L]
        assert np.all(got[:, sec["W"]] == 1.0)
        want = owned(parent).reshape(B, Lp + GAP)[:, :Lp]
        assert np.array_equal(bits(np.delete(got, np.arange(sec["W"].start, sec["W"].stop), axis=1)), bits(want))


# ---- i. batch.BatchWeightedHorizon, batch.BatchWeightedMPC

def _fetch(wl):
    """the workload's inputs as a batch_horizon_terms_util batch"""
    B, T, nx, nu, n, m = wl.B, wl.T, wl.nx, wl.nu, wl.n, wl.m
    shapes = {"Q": (nx, nx), "R": (nu, nu), "P": (nx, nx), "r": (T, nx), "v": (T, nu), "rN": (nx,), "wx": (T,), "wu": (T,), "wN": (), "gx": (T, nx),
              "gu": (T, nu), "gN": (nx,), "C": (n, m), "d": (m,)}
    names = {v: k for k, v in HT.FIELDS.items()}
    b = {"T": T}
    b.update({k: None for k in HT.KEYS})
    for name, t in wl.inputs.items():
        b[names[name]] = t.cpu().numpy().reshape(B, *shapes[name])
    return b


@pytest.mark.parametrize("terminal,weights,linear", [(True, True, True), (False, True, False), (True, False, True), (False, False, False)])
def test_batch_weighted_horizon_compute_and_expand_equal_the_restatement_on_its_inputs(terminal, weights, linear):
    import gpu_util as g
    from oracle import oracle as O
    from parametron_jl_amd import batch as PB
    total, T, nx, nu, m = 4, 3, 70, 6, 2
    wl = PB.BatchWeightedHorizon(torch, total, T, nx, nu, m, terminal, weights, linear)
    off, L = PB.horizon_terms_slab_layout(T, nx, nu, m, terminal)
    assert (wl.offsets, wl.L, wl.lo, wl.hi, wl.B, wl.n) == (off, L, 0, total, total, T * (nx + nu) + (nx if terminal else 0))
    assert wl.local.shape == (total, L) and wl.gathered is wl.local
    S = PB.BatchWeightedHorizon.SEEDS
    others = set(PB.BatchLSQ.SEEDS.values()) | set(PB.BatchTracking.SEEDS.values()) | set(PB.BatchMPC.SEEDS.values())
    assert len(set(S.values())) == 14 and set(S.values()).isdisjoint(others)
    assert set(wl.inputs) == {"Q", "R", "r", "C", "d"} | ({"P", "rN"} if terminal else set()) | ({"wx", "wu"} | ({"wN"} if terminal else set()) if weights else set()) \
        | ({"gx", "gu"} | ({"gN"} if terminal else set()) if linear else set())
    wl.local.fill_(float("nan"))
    wl.compute()
    torch.cuda.synchronize()
    b = _fetch(wl)
    assert np.array_equal(bits(b["Qt"].reshape(-1)), bits(O.fill_uniform(total * nx * nx, S["Q"])))
    assert np.array_equal(bits(b["d"].reshape(-1)), bits(O.fill_uniform(total * m, S["d"], 2.0)))
    if weights:
        assert np.array_equal(bits(b["wx"].reshape(-1)), bits(O.fill_uniform(total * T, S["wx"])))
    signs = (-1, 0, -1, -1)                                                     # x_t - r_t, u_t as it is, x_T - rN, C*z - d
    assert np.array_equal(bits(wl.local.cpu().numpy()), bits(HT.slab_reference(b, signs)))
    # one instance's MOI buffers
    n = wl.n
    xvar, varmap = np.arange(1, n + 1, dtype=np.int64), (np.random.default_rng(1).permutation(n) + 1).astype(np.int64)
    quad, lin, const, vat, vc = wl.expand(2, g.to_dev(xvar), g.to_dev(varmap))
    torch.cuda.synchronize()
    rq, rl, rc, rv, rvc = HT.expanded_reference(HT.instance(b, 2, signs), xvar, varmap)
    assert np.array_equal(quad.cpu().numpy(), rq) and np.array_equal(lin.cpu().numpy(), rl) and np.array_equal(vat.cpu().numpy(), rv)
    assert bits(const.cpu().numpy())[0] == bits([rc])[0] and np.array_equal(bits(vc.cpu().numpy()), bits(rvc))
    # another epoch: other data, the same relation
    wl.regenerate(1)
    wl.step(None)
    torch.cuda.synchronize()
    b1 = _fetch(wl)
    assert not np.array_equal(b1["Qt"], b["Qt"]) and np.array_equal(bits(b1["Qt"].reshape(-1)), bits(O.fill_uniform(total * nx * nx, S["Q"] + 1000)))
    assert np.array_equal(bits(wl.local.cpu().numpy()), bits(HT.slab_reference(b1, signs)))


@pytest.mark.parametrize("terminal", [True, False])
def test_batch_weighted_mpc_rows_and_the_dynamics_records_of_a_terminal_stage(terminal):
    """one row per instance [slab | dynamics section]; with a terminal stage the unchanged dynamics entry points run with T + 1 records, up
    to x_T == A*x_{T-1} + B*u_{T-1} + h_T, and their expansion reads no variable past x_T: the n = T*(nx + nu) + nx variables suffice (the
    index tensor holds exactly n words)"""
    import gpu_util as g
    from parametron_jl_amd import batch as PB
    total, T, nx, nu, m = 5, 4, 6, 3, 2
    wl = PB.BatchWeightedMPC(torch, total, T, nx, nu, m, terminal=terminal)
    Td = T + (1 if terminal else 0)
    (off, L), (doff, Ld) = PB.horizon_terms_slab_layout(T, nx, nu, m, terminal), PB.horizon_dynamics_layout(Td, nx, nu)
    assert (wl.offsets, wl.L, wl.dyn_offsets, wl.Ld, wl.stride, wl.Td) == (off, L, doff, Ld, L + Ld, Td) and wl.local.shape == (total, L + Ld)
    assert Ld == D.section_doubles(Td, nx, nu) and PB.BatchWeightedMPC(torch, 2, 2, 3, 1).m == 0
    S = PB.BatchWeightedMPC.SEEDS
    assert len(set(S.values())) == 17 and all(S[k] == v for k, v in PB.BatchWeightedHorizon.SEEDS.items())
    wl.local.fill_(float("nan"))
    wl.compute()
    torch.cuda.synchronize()
    b = _fetch(wl)
    f = lambda t, *shape: t.cpu().numpy().reshape(total, *shape)
    dyn = (f(wl.A, nx, nx), f(wl.Bm, nu, nx), f(wl.h, Td, nx))
    signs = (-1, 0, -1, -1)
    section = D.section_reference(*dyn, -1, -1, -1)
    assert np.array_equal(bits(wl.local.cpu().numpy()), bits(np.concatenate([HT.slab_reference(b, signs), section], axis=1)))
    n, i = wl.n, 3
    assert n == T * (nx + nu) + (nx if terminal else 0)
    xvar, varmap = np.arange(1, n + 1, dtype=np.int64), (np.random.default_rng(2).permutation(n) + 1).astype(np.int64)
    d_x = g.to_dev(xvar)
    assert d_x.numel() == n
    quad, lin, const, vat, vc, terms, consts = wl.expand(i, d_x, g.to_dev(varmap))
    torch.cuda.synchronize()
    rq, rl, rc, rv, rvc = HT.expanded_reference(HT.instance(b, i, signs), xvar, varmap)
    assert np.array_equal(quad.cpu().numpy(), rq) and np.array_equal(lin.cpu().numpy(), rl) and np.array_equal(vat.cpu().numpy(), rv)
    assert bits(const.cpu().numpy())[0] == bits([rc])[0] and np.array_equal(bits(vc.cpu().numpy()), bits(rvc))
    want_t, want_c = D.expanded_reference(section[i], Td, nx, nu, 1, xvar, varmap)
    assert len(want_t) == 3 * D.term_count(Td, nx, nu) and len(want_c) == Td * nx
    assert np.array_equal(terms.cpu().numpy(), want_t) and np.array_equal(bits(consts.cpu().numpy()), bits(want_c))
    if terminal:                                                                # the last record's x_+ part is x_T, the last nx variables of z
        last = want_t.reshape(-1, 3)[D.term_count(T, nx, nu):].reshape(nx, 1 + nx + nu, 3)
        assert np.array_equal(last[:, 0, 2], varmap[xvar[T * (nx + nu):] - 1])


@pytest.mark.parametrize("cls", ["BatchWeightedHorizon", "BatchWeightedMPC"])
def test_sharding_is_data_independent(cls):
    """the shards of rank 0 and rank 1 of world = 2, built on this one device, hold the rows world = 1 holds for the same instances"""
    from parametron_jl_amd import batch as PB
    total, T, nx, nu, m = 6, 4, 65, 9, 3
    make = lambda **kw: getattr(PB, cls)(torch, total, T, nx, nu, m, **kw)
    whole = make()
    whole.step(None)
    parts, inputs = [], {k: [] for k in whole.inputs}
    for rank in range(2):
        part = make(rank=rank, world=2)
        assert (part.lo, part.hi, part.B) == (3 * rank, 3 * rank + 3, 3) and part.gathered.shape == (total, part.stride) and part.local.shape == (3, part.stride)
        part.compute()
        parts.append(part.local.clone())
        for k, t in part.inputs.items():
            inputs[k].append(t.clone())
    torch.cuda.synchronize()
    for k, t in whole.inputs.items():
        assert torch.equal(torch.cat(inputs[k]), t), k
    assert torch.equal(torch.cat(parts), whole.local) and whole.gathered is whole.local
