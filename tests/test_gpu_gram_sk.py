"""-m gpu: the stream-K form of the canonical objective node (csrc/gram_sk.hip: gram_sk_kernel in both instantiations, its two fix-up
kernels, the balanced pair fold) in its three jobs — plain calls beyond 4096 columns, staged host deliveries, the strict launch inside the
fused form — on every load path, split regime and fix-up, against numpy, bit for bit.

There is no tolerance and no sampling in the exact cases: the data are dyadic (gram_sk_util.dyadic: integers scaled by 2^-bits, with
2 bits + ceil(log2 rows) + 1 <= 52), so every product and every partial sum of A'A, A'c and c'c is exact in any order, the float64 results
are unique, and plain numpy (A.T @ A, A.T @ c, c @ c) is the reference.  Every case asserts on every element:
  1. coefficients, q and the constant equal the reference bit for bit; row, column and variable indices exactly;
  2. the surroundings are untouched: outputs live in gpu_util.Guarded buffers (the whole image is compared), A's padding rows and shift
     word hold NaN (the header lets padding be read and ignored: a NaN anywhere in an output fails), the workspace is NaN-filled and
     followed by a guard band of 4096 doubles of 7.25, a delivered host array is followed by poisoned guard words;
  3. a second call with the same, now dirty, workspace and re-poisoned outputs gives the same bits; a delivered host array equals the
     device array bit for bit and pmt_fetch_synchronize returns PMT_OK;
  4. the profile report names what ran: gram_sk_kernel once per launch of the restatement (gram_sk_util.case_launches), and
     gram_sk_fixup_sliced_kernel / gram_sk_fixup_kernel as often as the restatement says.  The two variants of gram_sk_fixup_kernel
     (<2, 4> and <2, 1>) share ONE name in the report: which of them a case runs rests on the restatement alone
     (test_gram_sk_plan_host.py), not on anything observed here.
Two cases also run with rng.random() - 0.4 data against the project's own bar, 1e-12 * (2 |A|'|A|), bit-equal over three calls.

Boundary -> case (rows, cols, lda pad, base shift[, ngroups]); what each reaches is proved on the CPU by test_gram_sk_plan_host.py:

  sk_load_panel        one row, one column in the last tile, odd pitch      plain (1,4097,0,0); deliver (5,2049,0,0,0)
    (masked path,      odd row count: the scalar tail of a 16-byte piece    (257,4100,0,0) (1,4097,0,0) (5,2049,0,0,0) (260113,129,0,0)
    vec_in == 0)       8-byte-shifted base on an even pitch                 (600,4200,2,1)
                       odd pitch from the padding                           (500,2100,1,0,0)
  sk_load_panel        16-byte loads, ragged last stage / last tile         (1030,4224,2,0) (600,2100,0,0,*) (300,4100,0,0,0) (261128,257,0,0)
    (vec_in == 1)      whole panels and stages: the FAST body alone         (16,4224,0,0) (512,2176,0,0,*)
                       half-filled last column tile                         (1552,4160,0,0)
                       odd row count: the last row through the scalar tail  csc (257,4100,1,0); deliver (601,2100,1,0,0)
  phase A + phase B    tfull = 2 with a remainder of 49 tiles               every plain case; ranged: deliver (300,4100,0,0,1)
                       nchunk = 1: whole tiles only                         (1,4097,0,0) (16,4224,0,0) (5,2049,0,0,0)
                       U < G: workgroups without a unit BETWEEN the owners  (257,4100,0,0) (257,4100,1,0) (600,4200,2,1) (1030,4224,2,0);
                       of a split tile — the fix-up adds their slots too,   ranged: deliver (300,4100,0,0,1)
                       launch_gram_sk clears them (with the NaN-filled
                       workspace of this file every such tile came out NaN
                       before it did)
                       U > G: two partial slots in one workgroup            (1552,4160,0,0)
  RANGED walk          order_w < 0, seq_step = -1 (column bands, from the   every csc_deliver case
                       end); one stage / 2 / 5 / 16 stages
                       order_w = 0 (row bands, forward)                     terms_deliver (600,2100,0,0,0) and (..,16)
  pair fold            grids of 256 and 50; of 20 and 6; of 256 and 98      (512,2176,0,0,0) (512,2176,0,0,16) (300,4100,0,0,0)
                       on the masked path                                   (500,2100,1,0,0)
  gram_sk_fixup_kernel <2,4> tail loop alone (2 or 3 partials)              (257,4100,0,0) (600,4200,2,1) (600,2100,0,0,0)
                       <2,4> unrolled loop and tail (about 26 partials)     (8200,2100,0,0,16), stages of 10
                       <2,1> (3 tiles, 3 partials each)                     (600,2100,0,0,16), last stage
  gram_sk_fixup_sliced 3 tiles on 99 workgroups (ranged, not strict)        (8200,2100,0,0,16), last stage
                       1 strict tile, 256 partials                          (260113,129,0,0)
  strict launch        grid a multiple of the tile count: 255 = 3 x 85      (261128,257,0,0)
  sk_epilogue          CSC store with alpha = -0.5 / 2.0, with and without  csc and csc_deliver cases
                       out_quad; term store through a permuting varmap,
                       gaps in xvar; moi = 0 (diagonal not doubled)
  q and c'c            gram_linear_kernel, b = NULL (q = +0.0, constant 0)  sign = 0 cases; gram_linear_split_kernel: (8200,2100,0,0,16)
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_util as g  # noqa: E402
import gram_sk_util as U  # noqa: E402
import parametron_jl_amd as P  # noqa: E402
from parametron_jl_amd import _lib  # noqa: E402

WS_GUARD = 4096
HOST_GUARD = 8
NAN = float("nan")


class Inputs:
    """A (column-major, pitch rows + pad, base shifted by `shift` words; padding rows and the shift word hold NaN), b, xvar, varmap on the
    device, and their host copies for the reference"""

    def __init__(self, c, random=False):
        rows, n = c.rows, c.cols
        self.lda = rows + c.pad
        self.buf = torch.full((c.shift + self.lda * n,), NAN, dtype=torch.float64, device=g.DEV)
        M = self.buf[c.shift:].view(n, self.lda)
        rng = np.random.default_rng(rows * 131 + n)
        if random:
            M[:, :rows] = torch.from_numpy(np.ascontiguousarray((rng.random((rows, n)) - 0.4).T)).to(g.DEV)
            self.b = rng.random(rows) - 0.5
        else:
            gen = torch.Generator(device=g.DEV)
            gen.manual_seed(rows * 131 + n)
            lim = 1 << c.bits
            M[:, :rows] = torch.randint(-lim + 1, lim, (n, rows), generator=gen, device=g.DEV, dtype=torch.int64).double() / float(lim)
            self.b = U.dyadic(rows, c.bits, rng)
        self.A = M[:, :rows].cpu().numpy().T                       # (rows, n), copied back for the reference
        self.dA = C.c_void_p(self.buf.data_ptr() + 8 * c.shift)
        assert (self.buf.data_ptr() % 16 == 0) and (self.lda * n == M.numel())
        self.db = g.to_dev(self.b) if c.sign else None
        self.xv, self.vm = U.variables(n, n, gaps=c.vm)
        if not (c.vm and c.moi):
            self.vm = None
        self.dxv = g.to_dev(self.xv)
        self.dvm = g.to_dev(self.vm) if self.vm is not None else None
        nbytes = g.lib().pmt_quad_gram_workspace_bytes(rows, n)
        self.ws_words = nbytes // 8
        self.ws = torch.full((self.ws_words + WS_GUARD,), NAN, dtype=torch.float64, device=g.DEV)
        self.ws[self.ws_words:] = 7.25


class Outputs:
    def __init__(self, c):
        n = c.cols
        self.nq = nq = n * (n + 1) // 2
        self.quad = g.Guarded(3 * nq, shift=c.shift) if c.quad else None
        self.csc = g.Guarded(nq, doubles=True) if c.entry in ("csc", "csc_deliver") else None
        self.lin = g.Guarded(2 * n)
        self.const = g.Guarded(1, doubles=True)
        self.hp, self.host = None, None
        if c.entry.endswith("deliver"):
            self.hwords = nq if c.entry == "csc_deliver" else 3 * nq
            self.hp = C.c_void_p()
            g.call("pmt_host_alloc", 8 * (self.hwords + HOST_GUARD), C.byref(self.hp))
            self.host = np.frombuffer((C.c_char * (8 * (self.hwords + HOST_GUARD))).from_address(self.hp.value), dtype=np.int64)
            self.host[:] = g.POISON_WORD

    def poison(self):
        for o in (self.quad, self.csc, self.lin, self.const):
            if o is not None:
                o.buf.fill_(NAN if o.doubles else g.POISON_WORD)
        if self.host is not None:
            self.host[:] = g.POISON_WORD
        torch.cuda.synchronize()

    def free(self):
        if self.hp is not None:
            self.host = None
            g.call("pmt_host_free", self.hp)
            self.hp = None


def _call(c, x, o):
    s = g.stream()
    q = o.quad.ptr() if o.quad is not None else None
    if c.entry == "plain":
        g.call("pmt_quad_gram_f64", x.dA, x.lda, c.rows, c.cols, g.ptr(x.dxv), g.ptr(x.db), c.sign, c.moi, g.ptr(x.dvm), q, o.lin.ptr(), o.const.ptr(),
               g.ptr(x.ws), s)
    elif c.entry == "csc":
        g.call("pmt_quad_gram_csc_f64", x.dA, x.lda, c.rows, c.cols, g.ptr(x.dxv), g.ptr(x.db), c.sign, g.ptr(x.dvm), c.alpha, o.csc.ptr(), q, o.lin.ptr(),
               o.const.ptr(), g.ptr(x.ws), s)
    elif c.entry == "csc_deliver":
        g.call("pmt_quad_gram_csc_deliver_f64", x.dA, x.lda, c.rows, c.cols, g.ptr(x.dxv), g.ptr(x.db), c.sign, g.ptr(x.dvm), c.alpha, o.csc.ptr(), o.hp,
               c.ngroups, o.lin.ptr(), o.const.ptr(), g.ptr(x.ws), s)
    else:
        g.call("pmt_quad_gram_deliver_f64", x.dA, x.lda, c.rows, c.cols, g.ptr(x.dxv), g.ptr(x.db), c.sign, c.moi, g.ptr(x.dvm), q, o.hp, c.ngroups,
               o.lin.ptr(), o.const.ptr(), g.ptr(x.ws), s)
    if o.hp is not None:
        assert g.lib().pmt_fetch_synchronize(s) == _lib.PMT_OK, "pmt_fetch_synchronize"
    torch.cuda.synchronize()


def _owned(gd):
    return gd.buf[gd.off:gd.off + gd.n].cpu().numpy().view(np.int64).copy()


def _check_surroundings(c, x, o, what):
    assert bool(torch.all(x.ws[x.ws_words:] == 7.25)), what + ": the guard band behind the workspace was written"
    if o.host is not None:
        assert np.all(o.host[o.hwords:] == g.POISON_WORD), what + ": the words behind the delivered host array were written"
        dev = _owned(o.csc if c.entry == "csc_deliver" else o.quad)
        assert np.array_equal(o.host[:o.hwords], dev), what + ": the delivered host array differs from the device array"


def _check_exact(c, x, o, ref, what):
    if o.quad is not None:
        o.quad.check(ref["quad"], what + " out_quad")
    if o.csc is not None:
        o.csc.check(ref["csc"], what + " out_csc")
    o.lin.check(ref["lin"], what + " out_lin")
    o.const.check(np.array([ref["const"]]), what + " out_const")
    _check_surroundings(c, x, o, what)


def _check_profile(c, rep):
    launches = U.case_launches(c)
    kinds = [p.fixup for p, _, _ in launches]
    want = {"gram_sk_kernel": len(launches), "gram_sk_fixup_sliced_kernel": kinds.count("sliced"),
            "gram_sk_fixup_kernel": kinds.count("apb4") + kinds.count("apb1")}
    got = {k: rep.get(k, {"launches": 0})["launches"] for k in want}
    assert got == want, sorted(rep)
    splits = U.linear_splits(c.rows, c.cols) > 1 and c.sign != 0 and c.use != "strict"
    assert ("gram_linear_split_kernel" in rep) == splits and ("gram_linear_kernel" in rep) == (not splits and c.use != "strict"), sorted(rep)


@pytest.mark.parametrize("c", U.CASES, ids=[U.case_id(c) for c in U.CASES])
def test_stream_k_form_equals_numpy_bit_for_bit(c):
    assert U.dyadic_bound_holds(c.rows, c.bits)
    x, o = Inputs(c), Outputs(c)
    try:
        ref = U.reference(c, x.A, x.b if c.sign else None, x.xv, x.vm)
        P.profile_enable(True)
        try:
            _call(c, x, o)
            rep = P.profile_report()
        finally:
            P.profile_enable(False)
        _check_exact(c, x, o, ref, "first call")
        _check_profile(c, rep)
        o.poison()                                  # the workspace stays as the first call left it
        _call(c, x, o)
        _check_exact(c, x, o, ref, "second call")
    finally:
        o.free()


@pytest.mark.parametrize("c", U.RANDOM, ids=[U.case_id(c) for c in U.RANDOM])
def test_stream_k_form_on_random_data_within_the_projects_bar_and_repeatable(c):
    """a non-dyadic case per instantiation: 1e-12 * (2 |A|'|A|) as test_gpu_fuzz._check_gram_node, and the same bits over three calls"""
    x, o = Inputs(c, random=True), Outputs(c)
    try:
        n = c.cols
        iu = np.triu_indices(n)
        G = 2 * x.A.T @ x.A
        scale = 2 * np.abs(x.A).T @ np.abs(x.A)
        cvec = 0.0 - x.b if c.sign < 0 else 0.0 + x.b
        first = None
        for rep in range(3):
            o.poison()
            _call(c, x, o)
            vals = _owned(o.csc)
            lin, const = _owned(o.lin).reshape(n, 2), _owned(o.const)
            for gd, own in ((o.csc, vals), (o.lin, lin), (o.const, const)):
                gd.check(own, "guards, call %d" % rep)
            _check_surroundings(c, x, o, "call %d" % rep)
            if first is None:
                first = (vals, lin, const)
                got = vals.view(np.float64)[iu[1] * (iu[1] + 1) // 2 + iu[0]]
                assert np.all(np.abs(got - c.alpha * G[iu]) <= 1e-12 * abs(c.alpha) * scale[iu] + 1e-300)
                assert np.array_equal(lin[:, 1], x.xv)
                assert np.all(np.abs(lin[:, 0].copy().view(np.float64) - 2 * x.A.T @ cvec) <= 1e-12 * (2 * np.abs(x.A).T @ np.abs(cvec)) + 1e-300)
                assert const.view(np.float64)[0] == pytest.approx(float(cvec @ cvec), rel=1e-13)
            else:
                assert all(np.array_equal(a, b) for a, b in zip(first, (vals, lin, const))), "call %d gave other bits" % rep
    finally:
        o.free()
