"""-m gpu: the sparse assemble / pack kernels (csrc/sparse.hip) at the C ABI — the flat gather, the XCD-aware slab kernel with int64 and
uint32 index streams, and the LDS block kernel, each as pmt_linear_term (2 words) and pmt_vector_affine_term (3 words) — against the
plain-loop restatement of sparse_assemble_util (checked against the oracle in test_sparse_assemble_host.py), bit for bit.

Every operation here is a copy, or 0.0 (+|-) d: there is no tolerance in this file.  Every output lives in a poisoned buffer (a distinct
word per position, 16 guard words on both sides) and the WHOLE buffer is compared, at a 16-byte-aligned base and at one shifted by a word:
with an aligned base a run of 2-word terms never starts on an odd word, so the leading single word of the 16-byte repacking
(wave_write_words, the block kernel's image copy) is only ever taken by the shifted runs.  The coefficients carry both zeros, denormals,
both infinities and a NaN with a payload; d carries both zeros, so the sign of a zero constant is pinned.

Which pattern reaches which branch edge is computed, not claimed: test_sparse_assemble_host.py (block_edges / slab_edges).  In short:

  sparse_block_kernel   column runs 0 1 2 3 5 15..19 24 25 127 128 (pair load, len > 16 tail, a full column)   column_runs
                        the pair load whose first coefficient is nzval's last                                   column_runs, single
                        row runs 0 1 2 3 63 64 65 127 128 129 192 193 300 (write rounds 1..5), two bands         staircase
                        a block of exactly SB_CAP coefficients | one more: 32-wide bands, a ragged last one      capacity | over_capacity
                        nine bands (second octet of the workgroup map, idle workgroups), a 2-row row block       nine_bands
                        an empty row block, empty columns, empty first and last row                              holes
                        band widths 32, 64, 128, 1024                                                            random_*
                        out_consts null; d null with sign 0; d given with sign 0; sign +-1 with neither         every pattern
  sparse_slab_kernel    rows 1 15 16 17 33; four rows of a wave of lengths 129 0 1 65                            ragged*
                        segments 0 1 63 64 65 129, up to five rounds; nslab 1 3 8 64                             staircase, ragged*
                        more slabs than columns, empty slabs                                                     five_columns, single
  flat kernels          the second trip of the stride loop: 2048 * 256 + 3 terms                                 flat_long
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_util as g  # noqa: E402
import sparse_assemble_util as U  # noqa: E402
from parametron_jl_amd import _lib  # noqa: E402

SHIFTS = (0, 1)
ROW_OFFSETS = (0, 7)
SEED, FRESH = 21, 22


class Out:
    """a poisoned device buffer around an output of `nwords` words (sparse_assemble_util.Poisoned)"""

    def __init__(self, nwords, shift, fields):
        self.img, self.fields = U.Poisoned(nwords, shift), fields
        self.buf = torch.from_numpy(self.img.image.copy()).to(g.DEV)
        assert self.buf.data_ptr() % 16 == 0 and (self.buf.data_ptr() + 8 * self.img.off) % 16 == 8 * shift

    def ptr(self):
        return g.C.c_void_p(self.buf.data_ptr() + 8 * self.img.off)

    def check(self, words, what):
        torch.cuda.synchronize()
        self.img.check(self.buf.cpu().numpy(), words, self.fields, what)
        self.buf.copy_(torch.from_numpy(self.img.image))               # poisoned again for the next call


NOTHING = np.empty(0, dtype=np.int64)


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to(g.DEV)


class Case:
    """a pattern's inputs and static tables on the device, and what the node must write"""

    def __init__(self, name):
        self.name, self.pat, self.t = name, U.pattern(name), U.tables(name)
        p, t = self.pat, self.t
        self.xvar, self.varmap = U.column_variables(p.n, 31), U.permuting_varmap(p.n, 32)
        self.d = U.values(p.m, 33, nan=False)
        tvar = t.term_var(self.xvar)
        self.keep = {"perm": dev(t.perm), "trow": dev(t.trow), "tvar": dev(tvar), "mapped": dev(self.varmap[tvar - 1]), "xvar": dev(self.xvar),
                     "varmap": dev(self.varmap), "d": dev(self.d), "perm32": dev(t.perm.astype(np.uint32)), "tvar32": dev(tvar.astype(np.uint32)),
                     "mapped32": dev(self.varmap[tvar - 1].astype(np.uint32))}
        if t.cw > 0:
            self.keep.update(desc=dev(t.desc), idx=dev(t.idx), band=dev(t.band))
        self.nz = {}

    def p(self, key):
        return g.ptr(self.keep[key])

    def nzval(self, seed):
        if seed not in self.nz:
            host = U.values(self.pat.nnz, seed)
            self.nz[seed] = (host, dev(host if self.pat.nnz else np.zeros(1)))
        return self.nz[seed]

    def slab(self, nslab):
        key = "slab%d" % nslab
        if key not in self.keep:
            self.keep[key] = dev(self.t.slab_ptr(nslab))
        return self.p(key)

    @functools.lru_cache(maxsize=None)
    def want(self, seed, mapped, row_offset):
        p = self.pat
        vat, lt, _ = U.restate(p.m, p.n, p.colptr, p.rowval, self.nzval(seed)[0], self.xvar, self.varmap if mapped else None, row_offset, None, 0)
        assert len(vat) == 3 * p.nnz and len(lt) == 2 * p.nnz
        return vat, lt

    def consts(self, with_d, sign):
        return U.constants(self.pat.m, self.d if with_d else None, sign)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def outs(c, shift):
    return Out(3 * c.pat.nnz, shift, U.VAT_FIELDS), Out(2 * c.pat.nnz, shift, U.LT_FIELDS)


# ------------------------------------------------------------------ the flat gather
def flat_calls(c, seed, shift, crossed, vat, lt):
    nz, nnz = g.ptr(c.nzval(seed)[1]), c.pat.nnz
    for mapped in ((True, False) if crossed else (True,)):
        for off in (ROW_OFFSETS if crossed else (7,)):
            g.call("pmt_sparse_pack_vector_f64", nz, c.p("perm"), c.p("trow"), c.p("tvar"), nnz, c.p("varmap") if mapped else None, off, vat.ptr(), g.stream())
            vat.check(c.want(seed, mapped, off)[0], "%s flat VAT shift %d varmap %d row_offset %d" % (c.name, shift, mapped, off))
    g.call("pmt_sparse_assemble_f64", nz, c.p("perm"), c.p("tvar"), nnz, lt.ptr(), g.stream())
    lt.check(c.want(seed, True, 7)[1], "%s flat LT shift %d" % (c.name, shift))


@pytest.mark.parametrize("name", U.NAMED + U.SLAB_MADE)
def test_flat_kernels(name):
    c = case(name)
    for shift in SHIFTS:
        vat, lt = outs(c, shift)
        flat_calls(c, SEED, shift, True, vat, lt)
        flat_calls(c, FRESH, shift, False, vat, lt)                  # the same tables, new coefficients


def test_flat_kernels_beyond_one_pass_of_the_grid():
    c = Case("flat_long")
    assert c.pat.nnz == 2048 * 256 + 3
    for shift in SHIFTS:
        vat, lt = outs(c, shift)
        flat_calls(c, SEED, shift, False, vat, lt)


# ------------------------------------------------------------------ the slab kernel, int64 and uint32 index streams
def slab_calls(c, nslab, seed, shift, crossed, vat, lt):
    nz, m, sp = g.ptr(c.nzval(seed)[1]), c.pat.m, c.slab(nslab)
    for mapped in ((True, False) if crossed else (True,)):
        for off in (ROW_OFFSETS if crossed else (7,)):
            want = c.want(seed, mapped, off)[0]
            what = "%s nslab %d shift %d varmap %d row_offset %d: slab VAT " % (c.name, nslab, shift, mapped, off)
            vm = c.p("varmap") if mapped else None
            g.call("pmt_sparse_pack_vector_slabs_f64", nz, c.p("perm"), c.p("tvar"), sp, m, nslab, vm, off, vat.ptr(), g.stream())
            vat.check(want, what + "int64")
            g.call("pmt_sparse_pack_vector_slabs_u32_f64", nz, c.p("perm32"), c.p("tvar32"), sp, m, nslab, vm, off, vat.ptr(), g.stream())
            vat.check(want, what + "uint32")
            if mapped:                                               # varmap folded into the variable stream, no gather in the kernel
                g.call("pmt_sparse_pack_vector_slabs_f64", nz, c.p("perm"), c.p("mapped"), sp, m, nslab, None, off, vat.ptr(), g.stream())
                vat.check(want, what + "int64, folded varmap")
                g.call("pmt_sparse_pack_vector_slabs_u32_f64", nz, c.p("perm32"), c.p("mapped32"), sp, m, nslab, None, off, vat.ptr(), g.stream())
                vat.check(want, what + "uint32, folded varmap")
    want = c.want(seed, True, 7)[1]
    g.call("pmt_sparse_assemble_slabs_f64", nz, c.p("perm"), c.p("tvar"), sp, m, nslab, lt.ptr(), g.stream())
    lt.check(want, "%s nslab %d shift %d: slab LT int64" % (c.name, nslab, shift))
    g.call("pmt_sparse_assemble_slabs_u32_f64", nz, c.p("perm32"), c.p("tvar32"), sp, m, nslab, lt.ptr(), g.stream())
    lt.check(want, "%s nslab %d shift %d: slab LT uint32" % (c.name, nslab, shift))


@pytest.mark.parametrize("name,nslab", U.SLAB_CASES)
def test_slab_kernels(name, nslab):
    c = case(name)
    for shift in SHIFTS:
        vat, lt = outs(c, shift)
        slab_calls(c, nslab, SEED, shift, True, vat, lt)
        slab_calls(c, nslab, FRESH, shift, False, vat, lt)


# ------------------------------------------------------------------ the block kernel
# (d given, sign): 0.0 - d, 0.0 + d, no vector, a vector that sign 0 leaves out
CONSTANTS = ((True, -1), (True, 1), (False, 0), (True, 0))


def block_calls(c, seed, shift, crossed, vat, lt, kc):
    p, t = c.pat, c.t
    nz = g.ptr(c.nzval(seed)[1])
    tab = (c.p("desc"), c.p("idx"), c.p("band"), c.p("xvar"), p.m, p.n, p.nnz, t.cw)
    for with_d, sign in (CONSTANTS if crossed else CONSTANTS[:1]):
        dd = c.p("d") if with_d else None
        for with_consts in ((True, False) if crossed else (True,)):
            oc = kc.ptr() if with_consts else None
            wc = c.consts(with_d, sign) if with_consts else NOTHING
            for mapped in ((True, False) if crossed else (True,)):
                for off in (ROW_OFFSETS if crossed else (7,)):
                    what = "%s block VAT shift %d d %d sign %d out_consts %d varmap %d row_offset %d" % (c.name, shift, with_d, sign, with_consts, mapped, off)
                    g.call("pmt_sparse_pack_vector_blocks_f64", nz, *tab, c.p("varmap") if mapped else None, off, dd, sign, vat.ptr(), oc, g.stream())
                    vat.check(c.want(seed, mapped, off)[0], what)
                    kc.check(wc, what + ": constants")
            what = "%s block LT shift %d d %d sign %d out_consts %d" % (c.name, shift, with_d, sign, with_consts)
            g.call("pmt_sparse_assemble_blocks_f64", nz, *tab, dd, sign, lt.ptr(), oc, g.stream())
            lt.check(c.want(seed, True, 7)[1], what)
            kc.check(wc, what + ": constants")
    if crossed:                                                      # a sign without a vector is admitted where no constants are asked for
        g.call("pmt_sparse_pack_vector_blocks_f64", nz, *tab, c.p("varmap"), 7, None, -1, vat.ptr(), None, g.stream())
        vat.check(c.want(seed, True, 7)[0], "%s block VAT shift %d sign -1 without d or out_consts" % (c.name, shift))
        g.call("pmt_sparse_assemble_blocks_f64", nz, *tab, None, 1, lt.ptr(), None, g.stream())
        lt.check(c.want(seed, True, 7)[1], "%s block LT shift %d sign +1 without d or out_consts" % (c.name, shift))
        kc.check(NOTHING, "%s: constants nobody asked for" % c.name)


@pytest.mark.parametrize("name", U.NAMED + U.SLAB_MADE)
def test_block_kernels(name):
    c = case(name)
    assert c.t.cw > 0
    for shift in SHIFTS:
        vat, lt = outs(c, shift)
        kc = Out(c.pat.m, shift, ("constant",))
        block_calls(c, SEED, shift, True, vat, lt, kc)
        block_calls(c, FRESH, shift, False, vat, lt, kc)


# ------------------------------------------------------------------ calls that write nothing, or the constants only
class Scratch:
    """poisoned stand-ins for every argument: valid device addresses that an empty or refused call must leave alone"""

    def __init__(self):
        self.o = {k: Out(64, 0, ("word",)) for k in ("nzval", "perm", "trow", "tvar", "slab", "varmap", "desc", "idx", "band", "colvar", "d", "vat", "lt", "consts")}

    def __getattr__(self, k):
        return self.o[k].ptr()

    def untouched(self, what, but=()):
        for k, o in self.o.items():
            if k not in but:
                o.check(NOTHING, "%s: %s" % (what, k))


def test_empty_calls_write_nothing():
    s, st = Scratch(), g.stream()
    g.call("pmt_sparse_pack_vector_f64", s.nzval, s.perm, s.trow, s.tvar, 0, s.varmap, 7, s.vat, st)
    g.call("pmt_sparse_assemble_f64", s.nzval, s.perm, s.tvar, 0, s.lt, st)
    for suffix, rows in (("", 0), ("u32_", 0)):
        g.call("pmt_sparse_pack_vector_slabs_%sf64" % suffix, s.nzval, s.perm, s.tvar, s.slab, rows, 8, s.varmap, 7, s.vat, st)
        g.call("pmt_sparse_assemble_slabs_%sf64" % suffix, s.nzval, s.perm, s.tvar, s.slab, rows, 8, s.lt, st)
    for rows, cols, nnz, consts in ((0, 4, 5, True), (0, 0, 0, True), (3, 4, 0, False), (3, 0, 0, False), (3, 0, 5, False)):
        oc = s.consts if consts else None
        g.call("pmt_sparse_pack_vector_blocks_f64", s.nzval, s.desc, s.idx, s.band, s.colvar, rows, cols, nnz, 32, s.varmap, 7, s.d, -1, s.vat, oc, st)
        g.call("pmt_sparse_assemble_blocks_f64", s.nzval, s.desc, s.idx, s.band, s.colvar, rows, cols, nnz, 32, s.d, -1, s.lt, oc, st)
    s.untouched("empty calls")


@pytest.mark.parametrize("rows,cols,nnz", [(5, 4, 0), (5, 0, 0), (37, 0, 9)])
def test_a_node_without_terms_writes_exactly_its_constants(rows, cols, nnz):
    s, st = Scratch(), g.stream()
    d = U.values(rows, 41, nan=False)
    dd = dev(d)
    for shift in SHIFTS:
        kc = Out(rows, shift, ("constant",))
        for with_d, sign in CONSTANTS:
            dp = g.ptr(dd) if with_d else None
            what = "rows %d cols %d nnz %d shift %d d %d sign %d" % (rows, cols, nnz, shift, with_d, sign)
            g.call("pmt_sparse_pack_vector_blocks_f64", s.nzval, s.desc, s.idx, s.band, s.colvar, rows, cols, nnz, 32, s.varmap, 7, dp, sign, s.vat, kc.ptr(), st)
            kc.check(U.constants(rows, d if with_d else None, sign), what + " VAT")
            g.call("pmt_sparse_assemble_blocks_f64", s.nzval, s.desc, s.idx, s.band, s.colvar, rows, cols, nnz, 32, dp, sign, s.lt, kc.ptr(), st)
            kc.check(U.constants(rows, d if with_d else None, sign), what + " LT")
    s.untouched("constants only")
    assert np.array_equal(dd.cpu().numpy().view(np.int64), U.bits(d))


def test_refused_calls_write_nothing():
    """one refusal per kernel family, with every argument a live device buffer"""
    s, st = Scratch(), g.stream()
    with pytest.raises(_lib.DimensionMismatch):
        g.call("pmt_sparse_pack_vector_f64", s.nzval, s.perm, s.trow, s.tvar, -1, s.varmap, 7, s.vat, st)
    with pytest.raises(_lib.DimensionMismatch):
        g.call("pmt_sparse_assemble_f64", s.nzval, s.perm, s.tvar, -1, s.lt, st)
    with pytest.raises(_lib.DimensionMismatch):
        g.call("pmt_sparse_pack_vector_slabs_f64", s.nzval, s.perm, s.tvar, s.slab, 3, 65, s.varmap, 7, s.vat, st)
    with pytest.raises(_lib.DimensionMismatch):
        g.call("pmt_sparse_assemble_slabs_u32_f64", s.nzval, s.perm, s.tvar, s.slab, 3, 0, s.lt, st)
    with pytest.raises(_lib.ArgumentError):
        g.call("pmt_sparse_pack_vector_blocks_f64", s.nzval, s.desc, s.idx, s.band, s.colvar, 3, 4, 5, 48, s.varmap, 7, s.d, -1, s.vat, s.consts, st)
    with pytest.raises(_lib.ArgumentError):
        g.call("pmt_sparse_assemble_blocks_f64", s.nzval, s.desc, s.idx, s.band, s.colvar, 3, 4, 5, 32, None, 1, s.lt, s.consts, st)
    with pytest.raises(_lib.ArgumentError):
        g.call("pmt_sparse_assemble_blocks_f64", s.nzval, s.desc, s.idx, s.band, s.colvar, 3, 4, 0, 32, s.d, 2, s.lt, s.consts, st)
    s.untouched("refused calls")
