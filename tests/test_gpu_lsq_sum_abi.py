"""-m gpu: the weighted-sum combine kernels (csrc/gram_sum.hip) at the C ABI — pmt_quad_gram_sum_f64 and pmt_quad_gram_sum_sub_f64 — against
the numpy restatement of tests/lsq_sum_util.py (held to the oracle in tests/test_lsq_sum_host.py), word for word.

Every case of lsq_sum_util.cases() goes through the entry it names, at both alignments of the outputs:
  outputs      out_quad and out_lin in gpu_util.Guarded buffers (first word on a 16-byte boundary | 8 bytes behind one), out_const one word in
               a guarded buffer of doubles; block 1's image is uploaded into the owned words first and the WHOLE buffer image is compared.
               Row / col / var words name their own position and come back in place.
  the NaN rule where the restated coefficient is a computed NaN only "is NaN" is compared (lsq_sum_util: at most 2 % of a case's quadratic
               and n/8 of its linear coefficients); every other word is compared as a word, -0.0 and untouched signalling NaNs included.
  inputs       every later block's values / lin / constant, every vec and weight scalar (and block 1's decoy arrays, which the entry must
               ignore) stand between words holding a NaN payload of their own; they are fetched back unchanged and no output holds the payload.
Then: cols == 0 with null outputs, the recorded form (a plan replayed twice) against the immediate call, and two sums written into adjacent
slices of one quadratic / linear / constants buffer as moi.py lays a group record out, in both orders."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_util as g  # noqa: E402
import lsq_sum_util as U  # noqa: E402
from parametron_jl_amd import _lib  # noqa: E402

MARGIN = 2
KIND = {"block": _lib.PMT_LSQ_BLOCK, "diag": _lib.PMT_LSQ_DIAG, "linear": _lib.PMT_LSQ_LINEAR, "constant": _lib.PMT_LSQ_CONSTANT}


class Inputs:
    """device copies of the inputs, each between MARGIN words of U.OUTSIDE_BITS; check(): all of it is still what was uploaded"""

    def __init__(self):
        self.held = []

    def put(self, words, what):
        a = np.ascontiguousarray(words).reshape(-1).view(np.int64)
        image = np.full(len(a) + 2 * MARGIN, U.OUTSIDE_BITS, dtype=np.int64)
        image[MARGIN:MARGIN + len(a)] = a
        t = g.to_dev(image)
        self.held.append((t, image, what))
        return t.data_ptr() + 8 * MARGIN

    def check(self, name):
        torch.cuda.synchronize()
        for t, image, what in self.held:
            assert np.array_equal(t.cpu().numpy(), image), "%s: input changed: %s" % (name, what)


def lt_words(coeff):
    """a later block's linear terms: (coefficient bits, any variable word)"""
    w = 0x7700000000 + np.arange(2 * len(coeff), dtype=np.int64)
    w[0::2] = U.bits(coeff)
    return w


def check_image(buf, want, mask, what):
    """the WHOLE Guarded buffer against the poison overwritten by `want`; `mask`: the owned words under the NaN rule"""
    torch.cuda.synchronize()
    got = buf.buf.cpu().numpy().view(np.int64)
    image = buf.padding(len(got)).view(np.int64).copy()
    image[buf.off:buf.off + buf.n] = np.ascontiguousarray(want).reshape(-1).view(np.int64)
    m = np.zeros(len(got), dtype=bool)
    m[buf.off:buf.off + buf.n] = mask
    bad = np.flatnonzero((got != image) & ~m)
    if len(bad):
        k = int(bad[0])
        where = "front guard" if k < buf.off else ("back guard" if k >= buf.off + buf.n else "owned word %d of %d" % (k - buf.off, buf.n))
        raise AssertionError("%s: %d words differ, the first at %s: got %#018x, want %#018x" % (what, len(bad), where, int(got[k]) % 2 ** 64, int(image[k]) % 2 ** 64))
    assert np.all(np.isnan(got.view(np.float64)[m])), "%s: a coefficient restated as NaN is a number" % what
    assert not np.any(got == U.OUTSIDE_BITS), "%s: a word from outside an input" % what
    return got


def word_mask(mask, width):
    m = np.zeros(width * len(mask), dtype=bool)
    m[0::width] = mask
    return m


class Run:
    """one case on the device: inputs, descriptors, lists, and where its three outputs stand (Guarded buffers of its own unless `place`
    names words of shared ones: (quad buffer, word offset, lin buffer, word offset, constants buffer, word offset))"""

    def __init__(self, c, shift=0, place=None, force_sub=None):
        self.c, self.inp = c, Inputs()
        n, nt = c.n, len(c.terms)
        desc = []
        for i, t in enumerate(c.terms):
            d = {"kind": KIND[t.kind], "scale": t.scale, "sign": t.sign}
            if t.weight is not None:
                d["weight"] = self.inp.put(np.array([t.weight], dtype=np.float64), "term %d: weight" % i)
            if t.kind == "block" and t.values is not None:
                d["values"] = self.inp.put(t.values, "term %d: values" % i)
                d["lin"] = self.inp.put(lt_words(t.lin), "term %d: lin" % i)
                d["constant"] = self.inp.put(np.array([t.constant]), "term %d: constant" % i)
            elif t.kind in ("diag", "linear") and t.v is not None:
                d["vec"] = self.inp.put(t.v, "term %d: vec" % i)
            elif t.kind == "constant" and t.value is not None:
                d["vec"] = self.inp.put(np.array([t.value]), "term %d: scalar" % i)
            desc.append(d)
        self.terms = _lib.lsq_terms(desc)
        self.sub = c.sub if force_sub is None else True
        self.lists = [None if t.cols is None else np.ascontiguousarray(t.cols, dtype=np.int64) for t in c.terms]
        self.counts = np.array([0 if a is None else len(a) for a in self.lists], dtype=np.int64)
        # (a list of length 0 is still a list: its pointer is not NULL)
        self.ptrs = (C.c_void_p * nt)(*[None if a is None else (a.ctypes.data if len(a) else self.counts.ctypes.data) for a in self.lists])
        self.null_lists = force_sub == "null"
        if place is None:
            place = (g.Guarded(3 * c.nq, shift=shift), 0, g.Guarded(2 * n, shift=shift), 0, g.Guarded(1, doubles=True), 0)
        self.oq, self.q_at, self.ol, self.l_at, self.oc, self.c_at = place
        self.own = place

    def upload(self):
        c = self.c
        if c.nq:
            a = self.oq.off + self.q_at
            self.oq.buf[a:a + 3 * c.nq] = g.to_dev(c.quad)
            a = self.ol.off + self.l_at
            self.ol.buf[a:a + 2 * c.n] = g.to_dev(c.lin)
        a = self.oc.off + self.c_at
        self.oc.buf[a:a + 1] = g.to_dev(np.array([c.const]))

    def issue(self, stream, null_outputs=False):
        c = self.c
        q = None if null_outputs else C.c_void_p(self.oq.ptr().value + 8 * self.q_at)
        l = None if null_outputs else C.c_void_p(self.ol.ptr().value + 8 * self.l_at)
        k = C.c_void_p(self.oc.ptr().value + 8 * self.c_at)
        if self.sub:
            lists = None if self.null_lists else C.cast(self.ptrs, C.c_void_p)
            g.call("pmt_quad_gram_sum_sub_f64", c.n, C.addressof(self.terms), len(c.terms), lists, self.counts.ctypes.data_as(C.c_void_p), q, l, k, stream)
        else:
            g.call("pmt_quad_gram_sum_f64", c.n, C.addressof(self.terms), len(c.terms), q, l, k, stream)

    def check(self, what=""):
        """for a run with Guarded buffers of its own; -> the three whole images as fetched"""
        c = self.c
        quad, lin, const, masks = c.restated()
        name = "%s %s" % (c.name, what)
        got = (check_image(self.oq, quad, word_mask(masks[0], 3), name + ": quad"), check_image(self.ol, lin, word_mask(masks[1], 2), name + ": lin"),
               check_image(self.oc, np.array([const]), np.array([masks[2]]), name + ": constant"))
        self.inp.check(name)
        qw, lw = c.negzero_words()
        assert np.all(got[0][self.oq.off + np.array(qw, dtype=np.int64)] == U.NEG_ZERO_BITS) and np.all(got[1][self.ol.off + np.array(lw, dtype=np.int64)] == U.NEG_ZERO_BITS)
        return got


# ------------------------------------------------------------------ every case through the entry it names
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("name", list(U.cases()))
def test_case_matches_the_restatement(name, shift):
    r = Run(U.case(name), shift)
    r.upload()
    r.issue(g.stream())
    r.check("shift %d" % shift)


@pytest.mark.parametrize("lists", ["null", "entries"])
@pytest.mark.parametrize("name", ["n1", "n65_K8", "fast_full_diag"])
def test_plain_case_through_the_sub_entry(name, lists):
    """no list anywhere — term_cols NULL, or an array of NULL entries — is the plain sum"""
    r = Run(U.case(name), 1, force_sub=lists)
    r.upload()
    r.issue(g.stream())
    r.check("through the sub entry, lists %s" % lists)


# ------------------------------------------------------------------ cols == 0
@pytest.mark.parametrize("sub", [False, True])
def test_no_columns_changes_only_the_constant(sub):
    """null out_quad / out_lin, a diagonal term with a null vec and a constant term: only the constant kernel runs"""
    c = U.case("n0")
    assert c.n == 0 and [t.kind for t in c.terms] == ["block", "diag", "constant"] and c.terms[1].v is None
    r = Run(c, 0, force_sub="null" if sub else None)
    r.upload()
    r.issue(g.stream(), null_outputs=True)
    r.check("null outputs")                                          # (the empty quad / lin buffers standing by keep their poison)


# ------------------------------------------------------------------ the recorded form
@pytest.mark.parametrize("name", U.RECORDED)
def test_recorded_form_equals_the_immediate_call(name):
    """dispatch with a recording handle, the constant step queued by gram_after_deferred: each replay equals the immediate call word for word"""
    c = U.case(name)
    now = Run(c, 1)
    now.upload()
    now.issue(g.stream())
    want = now.check("immediate")
    rec = Run(c, 1)
    rec.upload()
    p = g.Plan()
    with p:
        rec.issue(p.rec)
    for replay in (1, 2):
        rec.upload()                                                 # the sum is in place: block 1's image is restored before each replay
        p.update()
        got = rec.check("replay %d" % replay)
        for a, b, what in zip(got, want, ("quad", "lin", "constant")):
            assert np.array_equal(a, b), "%s: replay %d differs from the immediate call in %s" % (name, replay, what)
    p.close()


# ------------------------------------------------------------------ adjacent slices with live neighbours
@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
@pytest.mark.parametrize("shift", [0, 1])
def test_two_sums_in_adjacent_slices(order, shift):
    """sums over 65 and 64 columns write bq + 24 * oq[k], bl + 16 * ol[k] and consts + 8 * k of one buffer each, as a group record lays
    them out: the second quadratic slice starts at an odd term offset (8 mod 16 from the first), the words in front of it are the first
    sum's last column index, the words behind the first are the second's first coefficient.  Both orders of the two calls."""
    cs = [U.case(s) for s in U.SLICES]
    assert cs[0].nq % 2 == 1
    oq, ol, oc = g.Guarded(3 * (cs[0].nq + cs[1].nq), shift=shift), g.Guarded(2 * (cs[0].n + cs[1].n), shift=shift), g.Guarded(2, doubles=True)
    runs = [Run(cs[0], place=(oq, 0, ol, 0, oc, 0)), Run(cs[1], place=(oq, 3 * cs[0].nq, ol, 2 * cs[0].n, oc, 1))]
    for r in runs:
        r.upload()
    for k in order:
        runs[k].issue(g.stream())
    res = [c.restated() for c in cs]
    name = "slices, order %s, shift %d" % (order, shift)
    check_image(oq, np.concatenate([res[0][0], res[1][0]]), np.concatenate([word_mask(res[0][3][0], 3), word_mask(res[1][3][0], 3)]), name + ": quad")
    check_image(ol, np.concatenate([res[0][1], res[1][1]]), np.concatenate([word_mask(res[0][3][1], 2), word_mask(res[1][3][1], 2)]), name + ": lin")
    check_image(oc, np.array([res[0][2], res[1][2]]), np.array([res[0][3][2], res[1][3][2]]), name + ": constants")
    for r in runs:
        r.inp.check(name)
