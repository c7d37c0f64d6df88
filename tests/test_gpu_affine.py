"""-m gpu: the dense affine assemble / pack kernels (csrc/affine.hip, csrc/affine_tile.h) at the C ABI — pmt_affine_assemble_f64,
pmt_affine_pack_vector_f64, pmt_affine_pack_vector_background_f64, pmt_vars_addsub_f64, pmt_consts_f64 — and the interpreter's second
implementation of the same nodes (csrc/small.hip), against the numpy restatement of tests/affine_util.py (held to the oracle in
tests/test_affine_host.py), bit for bit.

Everything here is a copy, an index map or 0.0 (+|-) b: there is no tolerance in this file.  Every output lives in a gpu_util.Guarded
buffer whose WHOLE image is compared (guard words on both sides keep their poison).  Every matrix entry names its (row, column); a fixed
set holds -0.0, denormals, infinities, a quiet and a signalling NaN with payloads; padding rows of A and the words behind it hold 1e300;
xvar has gaps, varmap permutes, the words behind xvar and b are valid sentinels.  No case is built so that a wrong kernel would leave
memory the test owns: indices stay in range and buffers have their full size.

Boundary -> case (constants as in the sources: 64-column tiles, TR = 32 when cdiv(cols,64)*cdiv(rows,64) < 1024 and rows > 32, else 64;
nontemporal loads in MODE 1 from rows*cols*8 >= 8 MiB; vec_in = A on 16 bytes and lda even; vec_out = output on 16 bytes and cols even;
MODE 0 = LinearTerm, MODE 1 = VectorAffineTerm; the tables and why each case is there: affine_util.py):

  affine_tile_kernel
   <0,true,64,false>   rows <= 32: never a full tile (scalar loads)   LOW (1,1) (1,64) (32,64) (32,65) (7,300); (32,128) | (33,128)
   <1,true,64,false>   the same, 8-byte stores                        the same cases, MODE 1.  ITS FULL-TILE PATH IS UNREACHABLE: more
                                                                      than 32 rows and 1024 tiles or more is 33*64*1024*8 bytes at least,
                                                                      which makes the block cold (<1,true,64,true>)
   <0,true,32,false>   tile edges: full | short rows | short cols |   EDGES (33,64) (63,65) (64,64) (65,63) (96,128) (97,129) (40,200),
   <1,true,32,false>   corner, one and several tiles                  both modes
                       vec_in x vec_out, each 0 by either cause       VARIANTS: at every EDGES shape with a full tile the full factorial
                       (lda odd | A shifted; cols odd | out shifted), of lda even | odd, A shifted 0 | 1, output shifted 0 | 1 (cols even
                       MODE 0's 16-byte stores on an 8-byte boundary  and odd come with the shapes); both modes
   <0,true,64,false>   1024 tiles: 16-byte loads at TR = 64           TILE_COUNT 66 x 32726 (full, short-row, short-col and corner tile),
   <1,true,64,true>    ... and the three-store row pairs at TR = 64,  aligned | odd lda | cols 32725 | output shifted, both modes;
                       nontemporal loads                              MODE 0 boundary 66 x 32704 (1022 tiles, TR 32) | 66 x 32705
   <1,true,32,true>    8 MiB exactly | below; cold and ragged         COLD 1024 x 1024 | 1024 x 1022; 1000 x 1050
   signs, nulls        sign -1 0 +1; b null; b with sign 0 (+0.0      SIGNS at 64 x 128 (full), 40 x 200 (ragged, odd lda), 7 x 70
                       where b is NaN, -0.0); out_consts null;        (TR 64); EMPTY (5,0) (0,5)
                       varmap null; row_offset 0 7 11; no cols / rows
   grid y              65535 block rows run, 65536 are refused        rows 4194240 | 4194241, cols 1: full-size buffers, both modes
  affine_pack_         one wave per (row, 256 columns), lanes 64      BACKGROUND (1,1) (1,256) (1,257) (3,255) (5,512) (5,513) (130,257):
  background_kernel    columns apart; 4 waves per workgroup           lda odd, A shifted, output shifted; the sign / null set; against
                                                                      the RESTATEMENT; constants through pmt_consts_f64 / a memset
  vars_addsub_kernel,  last thread of a block, first of the next      n 1 255 256 257 513: each subset of the three outputs, v null,
  consts_kernel                                                       varmap null | permuting, VAT shifted; consts sign -1 0 +1
  sp_node              SOP_AFFINE_LT / VAT, SOP_VARS_ADDSUB,          every case above of at most 32768 elements, recorded on plans and
                       SOP_CONSTS                                     replayed FUSED (pmt_plan_fused), against the same images
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import affine_util as U  # noqa: E402
import gpu_util as g  # noqa: E402
from parametron_jl_amd import _lib  # noqa: E402

ENTRY = {0: "pmt_affine_assemble_f64", 1: "pmt_affine_pack_vector_f64", "bg": "pmt_affine_pack_vector_background_f64"}


class Case:
    """inputs on the device, guarded outputs with what they must hold, and the one call in between (issued on a stream or recorded on a plan)"""

    def __init__(self, name):
        self.name, self.keep, self.calls, self.outs, self.small, self.work = name, [], [], [], True, 0

    def dev(self, words, shift=0):
        """device copy of int64 / float64 words (None stays NULL); shift = 1: based one word off a 16-byte boundary"""
        if words is None:
            return None
        a = np.ascontiguousarray(words).reshape(-1).view(np.int64)
        t = torch.zeros(len(a) + 2, dtype=torch.int64, device=g.DEV)
        if len(a):
            t[shift:shift + len(a)] = torch.from_numpy(a.copy()).to(g.DEV)
        self.keep.append(t)
        assert t.data_ptr() % 16 == 0
        return g.C.c_void_p(t.data_ptr() + 8 * shift)

    def out(self, want, shift=0, what="", doubles=False):
        want = np.ascontiguousarray(want)
        buf = g.Guarded(want.nbytes // 8, doubles=doubles, shift=shift)
        self.outs.append((buf, want, what))
        return buf

    def call(self, name, work, *args, fusable=True):
        self.calls.append((name, args))
        self.work += work
        if work > U.NODE_MAX or not fusable:
            self.small = False

    def issue(self, stream):
        for name, args in self.calls:
            g.call(name, *args, stream)

    def check(self):
        for buf, want, what in self.outs:
            buf.check(want, "%s: %s" % (self.name, what))

    def run(self):
        self.issue(g.stream())
        self.check()


def affine_case(s, mode, background=False):
    """one Spec through one entry point: `mode` 0 LinearTerm, 1 VectorAffineTerm (background: the background pack's entry)"""
    rows, cols, lda = s.rows, s.cols, U.lda_of(s)
    M = U.cached_matrix(rows, cols)
    x = U.variables(cols)
    vm = U.permuting_varmap(cols) if (s.mapped and mode == 1) else None
    b = U.vector(rows, nan=s.b_nan) if s.has_b else None
    c = Case("%s mode=%s %s (%s)" % ("background" if background else "tile", mode, U.spec_id(s), s.why))
    terms = U.lt_words(M, x) if mode == 0 else U.vat_words(M, x, vm, s.row_offset)
    ot = c.out(terms, s.out_shift, "terms")
    oc = c.out(U.constants(rows, b, s.sign), 0, "constants", doubles=True) if s.has_consts else None
    args = [c.dev(U.colmajor_words(M, lda), s.a_shift), lda, rows, cols, c.dev(x), c.dev(b), s.sign]
    if mode == 1:
        args += [c.dev(vm), s.row_offset]
    args += [ot.ptr(), oc.ptr() if oc else None]
    # what the interpreter can take: the tile entries' own node, or the constants' node of a block without columns
    node = (rows > 0 and cols > 0) or (rows > 0 and oc is not None and b is not None and s.sign != 0)
    c.call(ENTRY["bg" if background else mode], U.work_of(s) if cols else rows, *args, fusable=node and not background)
    return c


def run_specs(specs):
    for s in specs:
        for mode in s.modes:
            affine_case(s, mode).run()


# ------------------------------------------------------------------ the tile kernel
@pytest.mark.parametrize("s", U.LOW, ids=U.spec_id)
def test_blocks_of_at_most_32_rows_and_the_first_beyond(s):
    run_specs([s])


@pytest.mark.parametrize("s", U.EDGES, ids=U.spec_id)
def test_tile_edges_at_32_rows_per_tile(s):
    run_specs([s])


@pytest.mark.parametrize("shape", U.VARIANT_SHAPES, ids=str)
def test_every_load_and_store_path_at_32_rows_per_tile(shape):
    run_specs(U.variants(*shape))


@pytest.mark.parametrize("s", U.TILE_COUNT, ids=U.spec_id)
def test_1024_tiles_and_more_take_64_rows_per_tile(s):
    run_specs([s])


@pytest.mark.parametrize("s", U.COLD, ids=U.spec_id)
def test_the_pack_of_8_MiB_and_more_at_32_rows_per_tile(s):
    run_specs([s])


def test_signs_and_null_arguments():
    run_specs(U.SIGNS + U.EMPTY)


# ------------------------------------------------------------------ the grid's y extent
def _rows_case(rows, mode):
    s = U.spec(rows, 1, why="block rows of 64: %d" % U.cdiv(rows, 64))
    return affine_case(s, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_65535_block_rows_run(mode):
    _rows_case(U.TOO_MANY_ROWS - 1, mode).run()


@pytest.mark.parametrize("mode", [0, 1])
def test_65536_block_rows_are_refused_before_anything_is_written(mode):
    """launch_affine puts cdiv(rows, 64) into the grid's y extent and does not wrap; validate_affine_tiles refuses the shape.  Inputs and
    outputs have their full size (34 MB in, 67 / 101 MB out): whatever a launch did, it could touch only memory this test owns."""
    c = _rows_case(U.TOO_MANY_ROWS, mode)
    with pytest.raises(_lib.DimensionMismatch):
        c.issue(g.stream())
    for buf, want, what in c.outs:
        buf.check(buf.padding(buf.n), "%s: %s untouched" % (c.name, what))


# ------------------------------------------------------------------ the background pack, against the restatement
def test_background_pack():
    for s in U.background_cases():
        affine_case(s, 1, background=True).run()


# ------------------------------------------------------------------ x (+|-) v and the constants alone
def vars_addsub_cases(n):
    x, vm = U.variables(n), U.permuting_varmap(n)
    cases = []
    subsets = [(lt, vat, cs) for lt in (1, 0) for vat in (1, 0) for cs in (1, 0)]
    # every subset of the outputs at sign -1 through the map; then the other arguments with all three present
    variants = [(sub, -1, True, True, 0, 3) for sub in subsets]
    variants += [((1, 1, 1), 1, True, True, 1, 11), ((1, 1, 1), 0, True, True, 0, 0), ((1, 1, 1), 0, False, True, 1, 3), ((1, 1, 1), 1, True, False, 1, 0)]
    for (has_lt, has_vat, has_cs), sign, has_v, mapped, shift, row_offset in variants:
        v = U.vector(n, nan=(sign == 0)) if has_v else None
        lt, vat, cs = U.vars_addsub_words(x, n, v, sign, vm if mapped else None, row_offset)
        c = Case("vars_addsub n=%d outputs=%d%d%d sign=%d v=%s mapped=%s shift=%d row_offset=%d" % (n, has_lt, has_vat, has_cs, sign, has_v, mapped, shift, row_offset))
        # an absent output is NULL; a guarded buffer of its size stands by all the same and must keep its poison
        olt, ovat, ocs = c.out(lt if has_lt else np.full(2 * n, g.POISON_WORD), 0, "lt"), c.out(vat if has_vat else np.full(3 * n, g.POISON_WORD), shift, "vat"), \
            c.out(cs if has_cs else np.full(n, np.nan), 0, "constants", doubles=True)
        c.call("pmt_vars_addsub_f64", n, c.dev(x), n, c.dev(v), sign, c.dev(vm) if mapped else None, row_offset,
               olt.ptr() if has_lt else None, ovat.ptr() if has_vat else None, ocs.ptr() if has_cs else None)
        cases.append(c)
    for sign in (-1, 0, 1):
        d = U.vector(n, nan=(sign == 0))
        c = Case("consts n=%d sign=%d" % (n, sign))
        o = c.out(U.constants(n, d, sign), 0, "constants", doubles=True)
        c.call("pmt_consts_f64", n, c.dev(d), n, sign, o.ptr())
        cases.append(c)
    return cases


@pytest.mark.parametrize("n", U.ELEMENTWISE)
def test_variables_plus_numbers_and_the_constants_alone(n):
    for c in vars_addsub_cases(n):
        c.run()


# ------------------------------------------------------------------ the interpreter: the same cases as nodes of fused runs
def small_cases():
    cases = [affine_case(s, mode) for s in U.tile_cases() + U.EMPTY for mode in s.modes]
    cases += [affine_case(s, mode) for r, c in U.BACKGROUND_SHAPES for s in [U.spec(r, c, pad=1, out_shift=1, why="a background shape as a tile node")] for mode in (0, 1)]
    cases += [c for n in U.ELEMENTWISE for c in vars_addsub_cases(n)]
    return [c for c in cases if c.small]


def test_interpreter_replays_the_same_cases_fused():
    """every case of at most 32768 elements, recorded on plans next to other small nodes and replayed as fused runs (one interpreter launch
    per plan: asserted through pmt_plan_fused), checked against the same images with the same guards"""
    cases = small_cases()
    names = " | ".join(c.name for c in cases)
    for needle in ("tile mode=0 1x1", "tile mode=1 32x65", "tile mode=1 97x129 pad=3 a_shift=1 out_shift=1", "tile mode=0 40x200 pad=3", "tile mode=1 5x0",
                   "sign=0 b_nan=True", "has_b=False", "has_consts=False", "mapped=False", "vars_addsub n=513 outputs=010", "consts n=257 sign=0", "tile mode=1 5x513 pad=1 out_shift=1"):
        assert needle in names, needle
    assert len(cases) >= 200
    # plans of at most 40 nodes and 60000 elements: inside one run's bounds (48 nodes, 65536 elements: csrc/small.hip, csrc/common.h)
    plans, cur, work = [], [], 0
    for c in cases:
        if cur and (work + c.work > 60000 or len(cur) + 1 > 40):
            plans.append(cur)
            cur, work = [], 0
        cur.append(c)
        work += c.work
    if len(cur) == 1 and plans:                                           # (a run is two nodes at least)
        cur.insert(0, plans[-1].pop())
    plans.append(cur)
    for group in plans:
        assert len(group) >= 2 and all(len(c.calls) == 1 for c in group)
        p = g.Plan()
        with p:
            for c in group:
                c.issue(p.rec)
        assert p.fused() == (1, len(group), 1), (p.fused(), [c.name for c in group])
        p.update()
        for c in group:
            c.check()
        p.close()
