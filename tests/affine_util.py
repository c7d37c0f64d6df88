"""What the tests of the dense affine assemble / pack kernels (csrc/affine.hip, csrc/affine_tile.h) share: a numpy restatement of the node
A*x (+|-) b in its two output forms, of x (+|-) v and of the constants alone; the data family; a restatement of the choices launch_affine
makes for a shape (tile height, nontemporal loads, the vector load / store paths, the kinds of tile that occur); and the case tables, each
case naming the instance and the paths it is there for.

The restatement of the NODE is written from the contract in include/parametron_hip.h and the reference's loops (matvecmul!,
src/functions.jl:775-798; vecadd!/vecsubtract!, :751-764; copyto!(f, ::Variable), :421; update!(::MOI.VectorAffineFunction),
src/moi_interop.jl:64-81) — not from the kernels.  tests/test_affine_host.py checks it against the oracle bit for bit.  The restatement of
the CHOICE (choice()) is written from launch_affine's constants; test_affine_host.py holds every case of the tables to what it names, and
ties the tile count to the library through pmt_plan_rider_check, so that a changed threshold cannot silently empty a case.

Everything is compared as int64 words: a pmt_vector_affine_term is (row, coefficient bits, variable), a pmt_linear_term (coefficient bits,
variable).  One limit of the data: a NaN stands in `b` only where the sign is 0 (the constant is +0.0 whatever b holds).  The sign and
payload of 0.0 - NaN are not fixed by IEEE 754 (a negated operand may or may not carry its sign into the result), so no bit image of it
could be held against two machines; every other special value only ever moves, and moves as bits."""
import collections
import functools

import numpy as np

TILE = 64                                      # affine_tile.h: columns per tile, and rows unless the block is small
SMALL_TILES = 1024                             # affine.hip: affine_small_tiles — fewer 64 x 64 tiles than this (and rows > 32): 32-row tiles
NTL_MIN_BYTES = 8 << 20                        # affine.hip: the MOI pack of a block this large loads its matrix nontemporally
MAX_TILE_ROWS = 65535                          # affine.hip: AFFINE_MAX_TILE_ROWS — block rows of 64 beyond this are refused
NODE_MAX = 32768                               # common.h: SMALL_NODE_WORK_MAX
BG_CHUNK = 256                                 # affine_pack_background_kernel: columns per wave

PAD_VALUE = 1e300                              # leading-dimension padding rows of A: must never reach an output
DENORMAL = 5e-324 * 3
_U = lambda *w: np.array(w, dtype=np.uint64).view(np.float64)
QNAN, SNAN = _U(0x7FF8DEAD0000BEEF)[0:1], _U(0xFFF4BEEF0000DEAD)[0:1]      # quiet / signalling (quiet bit clear), payloads, both signs
SPECIAL_BITS = np.concatenate([_U(0x8000000000000000), np.array([DENORMAL, np.inf, -np.inf]), QNAN, SNAN, np.array([-DENORMAL, 0.0])]).view(np.int64)
TAIL = 64                                      # sentinel words behind the end of xvar and b
B_SENTINEL = 777.25


def cdiv(a, b):
    return -(-a // b)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------------------------- data
def matrix(rows, cols):
    """every entry distinct and naming its place: +-((row + 1) * 65536 + col + 1), exact in float64 below 2^37 rows; then a fixed set of
    entries overwritten, as bits, with -0.0, denormals, both infinities, a quiet and a signalling NaN with payloads, and +0.0"""
    assert cols < 65535 and rows < 2 ** 36
    r, c = np.arange(rows, dtype=np.int64)[:, None], np.arange(cols, dtype=np.int64)[None, :]
    M = ((r + 1) * 65536 + (c + 1)).astype(np.float64)
    M[(r + c) % 2 == 1] *= -1.0
    flat = M.reshape(-1).view(np.int64)
    n, k = rows * cols, len(SPECIAL_BITS)
    if n >= 2 * k:
        flat[(np.arange(k) * n) // k + 1] = SPECIAL_BITS              # spread over the block: first and last tile rows both get some
    else:
        flat[:n] = SPECIAL_BITS[(np.arange(n) + rows + cols) % k]    # a block of a few entries takes the specials in turn
    return M


def colmajor_words(M, lda, tail=TAIL):
    """the column-major image with leading dimension lda as int64 words: padding rows and `tail` words behind the end hold PAD_VALUE"""
    rows, cols = M.shape
    P = np.full((cols, lda), PAD_VALUE)
    P[:, :rows] = M.T
    return np.concatenate([P.reshape(-1), np.full(tail, PAD_VALUE)]).view(np.int64)


def nvars(cols):
    return 2 * cols + 3


def variables(cols, seed=1):
    """x[col]: distinct model variables out of 1 .. 2 cols + 3 in no particular order (gaps: half of the indices are not used), with TAIL
    sentinel words behind the end that are valid indices too"""
    rng = np.random.default_rng(1000 + seed)
    x = rng.permutation(nvars(cols))[:cols].astype(np.int64) + 1
    return np.concatenate([x, np.full(TAIL, nvars(cols), dtype=np.int64)])


def permuting_varmap(cols, seed=1):
    """the optimizer's index of model variable v at varmap[v - 1]: a permutation of 101 .. 100 + nvars, a slot for every index incl. the spare ones"""
    return np.random.default_rng(2000 + seed).permutation(nvars(cols)).astype(np.int64) + 101


def vector(n, seed=1, nan=False):
    """b / v: n doubles of both signs with -0.0, +0.0, a denormal and an infinity planted where n allows (nan=True: and both NaNs — for the
    sign-0 cases only, see the module's docstring), with TAIL sentinel words behind the end"""
    a = np.random.default_rng(3000 + seed).random(n) - 0.5
    a[a == 0.0] = 0.25
    sp = [-0.0, 0.0, DENORMAL, -np.inf] + ([QNAN[0], SNAN[0]] if nan else [])
    w = a.view(np.int64)
    for k, s in enumerate(sp[:n]):
        w[(k * n) // len(sp) + 1 if n >= 2 * len(sp) else k] = bits(np.array([s]))[0]
    return np.concatenate([a, np.full(TAIL, B_SENTINEL)])


# ---------------------------------------------------------------------------------------------------------------- the restatement
def constants(n, b, sign):
    """0.0 + b, 0.0 - b (vecadd!/vecsubtract! into a zeroed constant), or +0.0 for sign 0 or without a vector -> float64 (n,)"""
    if b is None or sign == 0:
        return np.zeros(n)
    b = np.asarray(b, dtype=np.float64)[:n]
    return (np.float64(0.0) + b) if sign > 0 else (np.float64(0.0) - b)


def lt_words(M, xvar):
    """pmt_affine_assemble_f64: out[row * cols + col] = (A[row, col], xvar[col]) -> int64 (2 rows cols,)"""
    rows, cols = M.shape
    w = np.empty((rows, cols, 2), dtype=np.int64)
    w[:, :, 0] = bits(M).reshape(rows, cols)
    w[:, :, 1] = np.asarray(xvar, dtype=np.int64)[None, :cols]
    return w.reshape(-1)


def vat_words(M, xvar, varmap, row_offset):
    """pmt_affine_pack_vector_f64: out[row * cols + col] = (row_offset + row + 1, A[row, col], varmap[xvar[col] - 1]) -> int64 (3 rows cols,)"""
    rows, cols = M.shape
    x = np.asarray(xvar, dtype=np.int64)[:cols]
    w = np.empty((rows, cols, 3), dtype=np.int64)
    w[:, :, 0] = (row_offset + 1 + np.arange(rows, dtype=np.int64))[:, None]
    w[:, :, 1] = bits(M).reshape(rows, cols)
    w[:, :, 2] = (x if varmap is None else np.asarray(varmap, dtype=np.int64)[x - 1])[None, :]
    return w.reshape(-1)


def vars_addsub_words(xvar, n, v, sign, varmap, row_offset):
    """pmt_vars_addsub_f64: one term (1.0, xvar[i]) per row, its MOI copy (row_offset + i + 1, 1.0, varmap[xvar[i] - 1]), constants
    0.0 (+|-) v[i] -> (LT words, VAT words, constants float64)"""
    one = bits(np.array([1.0]))[0]
    x = np.asarray(xvar, dtype=np.int64)[:n]
    lt = np.empty((n, 2), dtype=np.int64)
    lt[:, 0], lt[:, 1] = one, x
    vat = np.empty((n, 3), dtype=np.int64)
    vat[:, 0], vat[:, 1] = row_offset + 1 + np.arange(n, dtype=np.int64), one
    vat[:, 2] = x if varmap is None else np.asarray(varmap, dtype=np.int64)[x - 1]
    return lt.reshape(-1), vat.reshape(-1), constants(n, v, sign)


# ---------------------------------------------------------------------------------------------------------------- launch_affine's choice
Choice = collections.namedtuple("Choice", "tr ntl vec_in vec_out kinds tiles instance")


def tile_rows(rows, cols):
    return 32 if cdiv(cols, TILE) * cdiv(rows, TILE) < SMALL_TILES and rows > 32 else 64


def choice(mode, rows, cols, lda, a_shift=0, out_shift=0):
    """what launch_affine<mode> chooses for a block whose A starts a_shift words and whose output out_shift words behind a 16-byte boundary:
    rows per tile; nontemporal loads (MODE 1 of 8 MiB and more); the 16-byte load path (full tiles only) and the 16-byte VAT store path
    (full tiles, MODE 1 only); which kinds of tile occur: "full", "rows" (short in rows only), "cols" (short in columns only), "corner";
    the tile count; the template instance (stores are nontemporal in every production build)"""
    tr = tile_rows(rows, cols)
    ntl = bool(mode == 1 and rows * cols * 8 >= NTL_MIN_BYTES)
    vec_in = int(a_shift % 2 == 0 and lda % 2 == 0)
    vec_out = int(out_shift % 2 == 0 and cols % 2 == 0)
    kinds = set()
    if rows >= tr and cols >= TILE:
        kinds.add("full")
    if rows % tr and cols >= TILE:
        kinds.add("rows")
    if cols % TILE and rows >= tr:
        kinds.add("cols")
    if rows % tr and cols % TILE:
        kinds.add("corner")
    return Choice(tr, ntl, vec_in, vec_out, frozenset(kinds), cdiv(cols, TILE) * cdiv(rows, tr),
                  "<%d,true,%d,%s>" % (mode, tr, "true" if ntl else "false"))


# ---------------------------------------------------------------------------------------------------------------- the case tables
# A Spec is one call.  modes: which entry points run it (0: pmt_affine_assemble_f64, 1: pmt_affine_pack_vector_f64).  pad: lda = rows + pad.
# `instance` maps a mode to the template instance the case is there for, `kinds` are tile kinds it must have, `vec` = (vec_in, vec_out)
# where the case is there for a load / store path (None: not pinned).  test_affine_host.py checks all three against choice().
_SPEC = dict(pad=0, a_shift=0, out_shift=0, sign=-1, has_b=True, b_nan=False, has_consts=True, mapped=True, row_offset=7,
             modes=(0, 1), instance=None, kinds=(), vec=None, why="")
Spec = collections.namedtuple("Spec", ["rows", "cols"] + list(_SPEC))


def spec(rows, cols, **kw):
    d = dict(_SPEC)
    d.update(kw)
    return Spec(rows, cols, **d)


def spec_id(s):
    parts = ["%dx%d" % (s.rows, s.cols)]
    for f, v in _SPEC.items():
        if f in ("instance", "kinds", "vec", "why", "modes"):
            continue
        if getattr(s, f) != v:
            parts.append("%s=%s" % (f, getattr(s, f)))
    return " ".join(parts)


def lda_of(s):
    return s.rows + s.pad


def work_of(s):
    return s.rows * s.cols + s.rows            # the SmallNode's work (affine.hip)


def _inst(tr, ntl1=False):
    return {0: "<0,true,%d,false>" % tr, 1: "<1,true,%d,%s>" % (tr, "true" if ntl1 else "false")}


# TR = 64 through rows <= 32: never a full tile, so the scalar load and the 8-byte (VAT) stores whatever vec_in / vec_out say
LOW = [spec(1, 1, instance=_inst(64), kinds=("corner",), why="one entry"),
       spec(1, 64, instance=_inst(64), kinds=("rows",), why="one row of a whole tile's columns"),
       spec(32, 64, instance=_inst(64), kinds=("rows",), why="the most rows that keep TR = 64: half a tile, aligned, still no vector path"),
       spec(32, 65, pad=2, instance=_inst(64), kinds=("rows", "corner"), why="... with a second tile of one column"),
       spec(7, 300, pad=1, instance=_inst(64), kinds=("rows", "corner"), why="five tiles in a row, odd lda"),
       spec(32, 128, instance=_inst(64), kinds=("rows",), why="boundary rows > 32: below"),
       spec(33, 128, pad=1, instance=_inst(32), kinds=("full", "rows"), vec=(1, 1), why="boundary rows > 32: above (a full 32-row tile over a tile of one row)")]

# TR = 32 tile edges, both modes, aligned
EDGES = [spec(33, 64, pad=1, instance=_inst(32), kinds=("full", "rows"), vec=(1, 1), why="one row beyond a tile"),
         spec(63, 65, pad=1, instance=_inst(32), kinds=("full", "rows", "cols", "corner"), vec=(1, 0), why="all four kinds; odd cols (cause of vec_out = 0)"),
         spec(64, 64, instance=_inst(32), kinds=("full",), vec=(1, 1), why="two full tiles, nothing else"),
         spec(65, 63, pad=1, instance=_inst(32), kinds=("cols", "corner"), why="no full tile: 63 columns"),
         spec(96, 128, instance=_inst(32), kinds=("full",), vec=(1, 1), why="3 x 2 full tiles"),
         spec(97, 129, pad=1, instance=_inst(32), kinds=("full", "rows", "cols", "corner"), vec=(1, 0), why="all four kinds beside several full tiles; odd cols"),
         spec(40, 200, instance=_inst(32), kinds=("full", "rows", "cols", "corner"), vec=(1, 1), why="all four kinds with vec_in = vec_out = 1")]

# TR = 32 path variants: the FULL factorial (not a pairwise selection) of lda even | odd, A base shifted 0 | 1 word, output shifted 0 | 1 word
# at every shape above that has a full tile — cols even and odd come with the shapes.  Every (vec_in, vec_out) thus meets a full tile and a
# ragged one (63x65, 97x129: odd cols; 33x64, 40x200: even), and each predicate is 0 through either cause and through both.
VARIANT_SHAPES = [(s.rows, s.cols) for s in EDGES if "full" in s.kinds]


def variants(rows, cols):
    out = []
    for lda_odd in (0, 1):
        for a_shift in (0, 1):
            for out_shift in (0, 1):
                pad = 2 + ((rows + lda_odd) % 2)                     # 2 or 3 padding rows: lda of the parity asked for
                vec = (int(not lda_odd and not a_shift), int(not out_shift and cols % 2 == 0))
                out.append(spec(rows, cols, pad=pad, a_shift=a_shift, out_shift=out_shift, instance=_inst(32), kinds=("full",), vec=vec,
                                why="vec_in = %d, vec_out = %d" % vec))
    return out


# TR = 64 through the tile count.  66 x 32726: 2 x 512 = 1024 tiles, one of each kind and 510 more full ones; 17.3 MB of matrix: cold
BIG = (66, 32726)
_BIGI = _inst(64, True)
TILE_COUNT = [spec(*BIG, instance=_BIGI, kinds=("full", "rows", "cols", "corner"), vec=(1, 1), why="the 16-byte loads and the three-store row pairs at TR = 64"),
              spec(*BIG, pad=1, instance=_BIGI, kinds=("full", "rows", "cols", "corner"), vec=(0, 1), why="odd lda: scalar loads under the three-store row pairs"),
              spec(66, 32725, instance=_BIGI, kinds=("full", "rows", "cols", "corner"), vec=(1, 0), why="odd cols: 16-byte loads under 8-byte stores"),
              spec(*BIG, out_shift=1, instance=_BIGI, kinds=("full", "rows", "cols", "corner"), vec=(1, 0), why="output on an 8-byte-only boundary"),
              spec(66, 32704, modes=(0,), instance=_inst(32), kinds=("full", "rows"), vec=(1, 1), why="boundary of the tile count: 1022 tiles, TR = 32"),
              spec(66, 32705, modes=(0,), instance=_inst(64), kinds=("full", "rows", "cols", "corner"), vec=(1, 0), why="boundary of the tile count: 1024 tiles, TR = 64")]

# the NTL boundary at TR = 32 (MODE 1)
COLD = [spec(1024, 1024, modes=(1,), instance=_inst(32, True), kinds=("full",), vec=(1, 1), why="exactly 8 MiB: cold"),
        spec(1024, 1022, modes=(1,), instance=_inst(32, False), kinds=("full", "cols"), vec=(1, 1), why="16 KiB below 8 MiB: plain loads"),
        spec(1000, 1050, modes=(1,), instance=_inst(32, True), kinds=("full", "rows", "cols", "corner"), vec=(1, 1), why="cold and ragged both ways")]


def sign_set(rows, cols, **kw):
    """signs and null arguments at one shape"""
    return [spec(rows, cols, sign=1, why="vecadd!", **kw), spec(rows, cols, sign=-1, row_offset=0, why="vecsubtract!, row_offset 0", **kw),
            spec(rows, cols, sign=0, b_nan=True, row_offset=11, why="b given, sign 0: +0.0 even where b is NaN or -0.0; row_offset 11", **kw),
            spec(rows, cols, sign=0, has_b=False, why="b null", **kw), spec(rows, cols, has_consts=False, why="out_consts null", **kw),
            spec(rows, cols, mapped=False, why="varmap null", **kw)]


SIGNS = (sign_set(64, 128, instance=_inst(32), kinds=("full",), vec=(1, 1)) + sign_set(40, 200, pad=3, instance=_inst(32), kinds=("full", "rows", "cols", "corner"), vec=(0, 1))
         + sign_set(7, 70, instance=_inst(64), kinds=("rows", "corner")))
EMPTY = [spec(5, 0, sign=-1, why="no columns: the constants alone (pmt_consts_f64)"), spec(5, 0, sign=0, has_b=False, why="no columns, no vector: +0.0"),
         spec(5, 0, sign=0, b_nan=True, why="no columns, b given with sign 0: +0.0"), spec(5, 0, has_consts=False, why="no columns, no constants: nothing"),
         spec(0, 5, why="no rows: nothing")]

# the background pack: one wave per (row, 256-column chunk), lanes 64 columns apart
BACKGROUND_SHAPES = [(1, 1), (1, 256), (1, 257), (3, 255), (5, 512), (5, 513), (130, 257)]


def background_cases():
    out = [spec(r, c, pad=p, a_shift=a, out_shift=o, why="background %dx%d" % (r, c))
           for r, c in BACKGROUND_SHAPES for p, a, o in ((0, 0, 0), (1, 0, 0), (2, 1, 0), (0, 0, 1), (3, 1, 1))]
    return out + sign_set(5, 513) + sign_set(130, 257, pad=1) + EMPTY


ELEMENTWISE = [1, 255, 256, 257, 513]          # one thread per element, 256 per block: vars_addsub_kernel, consts_kernel

# the grid's y extent: the first row count that needs 65536 block rows of 64 (refused), and the last that does not
TOO_MANY_ROWS = MAX_TILE_ROWS * TILE + 1


def tile_cases():
    """every Spec that goes through launch_affine"""
    return LOW + EDGES + [v for sh in VARIANT_SHAPES for v in variants(*sh)] + TILE_COUNT + COLD + SIGNS


@functools.lru_cache(maxsize=4)
def cached_matrix(rows, cols):
    M = matrix(rows, cols)
    M.setflags(write=False)
    return M
