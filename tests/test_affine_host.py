"""CPU suite for tests/affine_util.py, which tests/test_gpu_affine.py relies on: the numpy restatement of the dense node A*x (+|-) b, of
x (+|-) v and of the constants against the oracle bit for bit (special values included), the data family, every case of the tables held
to the instance, tile kinds and load / store paths it names, and the restated tile count held to the library's own
(pmt_plan_rider_check: a pure host function) for every shape of the tables."""
import ctypes as C

import numpy as np
import pytest

import affine_util as U
from oracle import oracle as O


# ---------------------------------------------------------------------------------------------------------------- data
def test_the_matrix_names_every_place_and_carries_every_special():
    M = U.matrix(40, 30)
    w = U.bits(M).reshape(-1)
    assert len(set(w.tolist())) == w.size and set(U.SPECIAL_BITS.tolist()) <= set(w.tolist())
    plain = ~np.isin(w, U.SPECIAL_BITS)
    r, c = np.divmod(np.flatnonzero(plain), 30)
    assert np.array_equal(np.abs(M.reshape(-1)[plain]), (r + 1) * 65536.0 + c + 1)       # the value names (row, column)
    assert np.any(M.reshape(-1)[plain] < 0) and np.any(M.reshape(-1)[plain] > 0)
    sp = U.SPECIAL_BITS.view(np.uint64).tolist()
    assert 0x8000000000000000 in sp and 0 in sp and 0x7FF8DEAD0000BEEF in sp and 0xFFF4BEEF0000DEAD in sp
    f = U.SPECIAL_BITS.view(np.float64)
    assert np.sum(np.isnan(f)) == 2 and np.sum(np.isinf(f)) == 2 and np.sum((f != 0) & (np.abs(f) < 1e-300)) == 2
    assert (0xFFF4BEEF0000DEAD >> 51) & 1 == 0 and (0x7FF8DEAD0000BEEF >> 51) & 1 == 1       # signalling: quiet bit clear
    # a block of a few entries still has specials; one of several million entries keeps every value exact
    assert np.any(np.isin(U.bits(U.matrix(1, 1)), U.SPECIAL_BITS))
    top = U.matrix(U.TOO_MANY_ROWS, 1)[-1, 0]
    assert abs(top) == U.TOO_MANY_ROWS * 65536.0 + 1


def test_vectors_variables_and_maps():
    x, vm = U.variables(50), U.permuting_varmap(50)
    assert len(x) == 50 + U.TAIL and len(set(x[:50].tolist())) == 50 and x[:50].min() >= 1 and x.max() <= U.nvars(50) == len(vm)
    assert not np.array_equal(x[:50], np.sort(x[:50])) and len(set(range(1, U.nvars(50) + 1)) - set(x[:50].tolist())) >= 50     # unordered, with gaps
    assert sorted(vm.tolist()) == list(range(101, 101 + U.nvars(50))) and not np.array_equal(vm, np.sort(vm))
    b = U.vector(40)
    wb = U.bits(b[:40])
    assert len(b) == 40 + U.TAIL and np.all(b[40:] == U.B_SENTINEL) and not np.any(np.isnan(b))
    assert np.any(wb == np.int64(-2 ** 63)) and np.any(wb == 0) and np.any(np.isinf(b)) and np.any(b == U.DENORMAL)
    bn = U.bits(U.vector(40, nan=True)[:40]).view(np.uint64).tolist()
    assert 0x7FF8DEAD0000BEEF in bn and 0xFFF4BEEF0000DEAD in bn and 0x8000000000000000 in bn
    assert np.any(U.bits(U.vector(1)) == np.int64(-2 ** 63))                             # a single constant is -0.0


# ---------------------------------------------------------------------------------------------------------------- against the oracle
def _oracle(M, x, varmap, row_offset, b, sign):
    rows = M.shape[0]
    f = O.AffVec(rows).matvecmul_vars(M, x)
    if b is not None and sign:
        f = O.AffVec(rows).vecaddsub(f, b, sign < 0)
    lt, ptr, lc = f.flat()
    assert np.array_equal(ptr, np.arange(rows + 1) * M.shape[1])
    if row_offset:                                                   # stacked under `row_offset` rows of anything (vcat!, src/functions.jl:870-885)
        top = O.AffVec(row_offset).matvecmul_vars(np.full((row_offset, 1), 1.5), [1])
        vt, vc = O.AffVec(row_offset + rows).vcat(top, f).moi(varmap)
        vt, vc = vt[vt["out"] > row_offset], vc[row_offset:]
    else:
        vt, vc = f.moi(varmap)
    assert U.bits(vc).tolist() == U.bits(lc).tolist()
    return lt.view(np.int64).reshape(-1), vt.view(np.int64).reshape(-1), U.bits(lc)


ORACLE_SHAPES = [(1, 1), (3, 5), (5, 3), (7, 13), (33, 4), (2, 70)]
ORACLE_CROSS = [(True, 7, -1), (False, 0, 1), (True, 0, 0), (False, 11, 1), (True, 11, None)]


@pytest.mark.parametrize("shape", ORACLE_SHAPES, ids=str)
def test_the_restatement_against_the_oracle(shape):
    rows, cols = shape
    M, x, vm = U.matrix(rows, cols), U.variables(cols)[:cols], U.permuting_varmap(cols)
    if rows * cols >= 2 * len(U.SPECIAL_BITS):
        assert set(U.SPECIAL_BITS.tolist()) <= set(U.bits(M).reshape(-1).tolist())
    for mapped, row_offset, sign in ORACLE_CROSS:
        b = None if sign is None else U.vector(rows)[:rows]
        lt, vt, consts = _oracle(M, x, vm if mapped else None, row_offset, b, sign or 0)
        assert np.array_equal(U.lt_words(M, x), lt), (shape, "LinearTerm")
        assert np.array_equal(U.vat_words(M, x, vm if mapped else None, row_offset), vt), (shape, mapped, row_offset)
        assert np.array_equal(U.bits(U.constants(rows, b, sign or 0)), consts), (shape, sign)


def test_wrong_restatements_are_told_apart():
    M, x, vm = U.matrix(5, 7), U.variables(7)[:7], U.permuting_varmap(7)
    lt, vt, consts = _oracle(M, x, vm, 7, U.vector(5)[:5], -1)
    assert not np.array_equal(U.lt_words(np.ascontiguousarray(M.T).reshape(5, 7), x), lt)          # the column-major walk
    assert not np.array_equal(U.vat_words(M, x, None, 7), vt) and not np.array_equal(U.vat_words(M, x, vm, 6), vt)
    assert not np.array_equal(U.vat_words(M, x, np.roll(vm, 1), 7), vt)                            # varmap[v] for varmap[v - 1]
    assert not np.array_equal(U.bits(-U.vector(5)[:5]), consts)                                    # -b for 0.0 - b: differs at b = +0.0
    assert not np.array_equal(U.bits(U.constants(5, U.vector(5), 1)), consts)


@pytest.mark.parametrize("n", [1, 5, 40])
def test_variables_plus_numbers_against_the_oracle(n):
    x, vm, v = U.variables(n)[:n], U.permuting_varmap(n), U.vector(n)[:n]
    for sign in (-1, 1):
        ref = O.AffVec(n).vecaddsub(x, v, subtract=sign < 0)
        terms, _, consts = ref.flat()
        for mapped in (True, False):
            mt, mc = ref.moi(vm if mapped else None)
            lt, vat, c = U.vars_addsub_words(x, n, v, sign, vm if mapped else None, 0)
            assert np.array_equal(lt, terms.view(np.int64).reshape(-1)) and np.array_equal(vat, mt.view(np.int64).reshape(-1))
            assert np.array_equal(U.bits(c), U.bits(consts)) and np.array_equal(U.bits(c), U.bits(mc))
        assert np.array_equal(U.vars_addsub_words(x, n, v, sign, vm, 11)[1].reshape(n, 3)[:, 0], np.arange(n) + 12)
    assert np.array_equal(U.bits(U.vars_addsub_words(x, n, None, 0, vm, 0)[2]), np.zeros(n, dtype=np.int64))
    assert np.array_equal(U.bits(U.constants(n, U.vector(n, nan=True), 0)), np.zeros(n, dtype=np.int64))      # sign 0: +0.0 whatever b holds


# ---------------------------------------------------------------------------------------------------------------- the tables
def _all_specs():
    return U.tile_cases()


def test_every_case_reaches_what_it_names():
    seen = set()
    for s in _all_specs():
        assert s.instance is not None, s
        for mode in s.modes:
            ch = U.choice(mode, s.rows, s.cols, U.lda_of(s), s.a_shift, s.out_shift)
            assert ch.instance == s.instance[mode], (U.spec_id(s), mode, ch)
            assert set(s.kinds) <= ch.kinds, (U.spec_id(s), ch)
            if s.vec is not None:
                assert (ch.vec_in, ch.vec_out) == s.vec, (U.spec_id(s), ch)
            seen.add((ch.instance, ch.vec_in if "full" in ch.kinds else None, ch.vec_out if "full" in ch.kinds and mode == 1 else None, "full" in ch.kinds))
        assert U.lda_of(s) >= s.rows and (s.has_b or s.sign == 0)
    insts = {i for i, _, _, _ in seen}
    assert insts == {"<0,true,32,false>", "<0,true,64,false>", "<1,true,32,false>", "<1,true,32,true>", "<1,true,64,false>", "<1,true,64,true>"}
    # each instance with a full tile meets both load paths, each MODE 1 instance with one both store paths ...
    for inst in ("<0,true,32,false>", "<0,true,64,false>", "<1,true,32,false>", "<1,true,64,true>"):
        assert {vi for i, vi, _, full in seen if i == inst and full} == {0, 1}, inst
    for inst in ("<1,true,32,false>", "<1,true,64,true>"):
        assert {vo for i, _, vo, full in seen if i == inst and full} == {0, 1}, inst
    assert {(vi, vo) for i, vi, vo, full in seen if i == "<1,true,32,false>" and full} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # ... and <1,true,64,false> never a full tile: rows > 32 with 1024 tiles or more is 33 x 1024 x 64 x 8 bytes at least — cold
    assert not any(full for i, _, _, full in seen if i == "<1,true,64,false>")
    assert 33 * 64 * U.SMALL_TILES * 8 >= U.NTL_MIN_BYTES


def test_the_groups_hold_what_their_comments_say():
    for s in U.LOW[:6]:                                                  # TR = 64 through rows <= 32: no full tile in either mode
        for mode in s.modes:
            ch = U.choice(mode, s.rows, s.cols, U.lda_of(s))
            assert ch.tr == 64 and "full" not in ch.kinds and not ch.ntl
    assert U.tile_rows(32, 128) == 64 and U.tile_rows(33, 128) == 32
    # the factorial of the path variants: per shape 8 cases, all four (vec_in, vec_out) at even cols, each predicate 0 by either cause
    for rows, cols in U.VARIANT_SHAPES:
        vs = U.variants(rows, cols)
        assert len(vs) == 8 and {(U.lda_of(v) % 2, v.a_shift, v.out_shift) for v in vs} == {(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}
        assert all(U.lda_of(v) > rows + 1 for v in vs)                       # padding rows in every one
        assert {v.vec for v in vs} == ({(0, 0), (0, 1), (1, 0), (1, 1)} if cols % 2 == 0 else {(0, 0), (1, 0)})
    kinds = lambda r, c: U.choice(1, r, c, r).kinds
    assert any(cols % 2 == 0 and kinds(rows, cols) > {"full"} for rows, cols in U.VARIANT_SHAPES)       # even cols with ragged tiles
    assert any(cols % 2 == 1 and kinds(rows, cols) > {"full"} for rows, cols in U.VARIANT_SHAPES)
    # the tile count's boundary, the NTL boundary
    assert U.cdiv(32704, 64) * U.cdiv(66, 64) == 1022 and U.choice(0, 66, 32704, 66).tr == 32 and U.choice(0, 66, 32704, 66).tiles == 511 * 3
    assert U.choice(0, 66, 32705, 66).tiles == 1024 and U.choice(1, *U.BIG, 66).tiles == 1024
    assert 1024 * 1024 * 8 == U.NTL_MIN_BYTES and 1024 * 1022 * 8 < U.NTL_MIN_BYTES
    assert 32 * U.BIG[0] * U.BIG[1] < 256 << 20                               # under PMT_MID_RIDER_BYTES: the pack rides (test_gpu_gram_riders.py)
    # the background pack's shapes stand on both sides of a 256-column chunk and of a workgroup of four waves
    assert {c % U.BG_CHUNK for _, c in U.BACKGROUND_SHAPES} >= {0, 1, 255} and {(r * U.cdiv(c, U.BG_CHUNK)) % 4 for r, c in U.BACKGROUND_SHAPES} >= {0, 1, 2, 3}
    # the interpreter gets every kind of small case
    small = [s for s in _all_specs() if U.work_of(s) <= U.NODE_MAX]
    assert len(small) >= 60 and any(s.a_shift and s.out_shift for s in small) and any("corner" in s.kinds for s in small)
    assert U.TOO_MANY_ROWS == 4194241 and U.cdiv(U.TOO_MANY_ROWS, 64) == 65536 and U.tile_rows(U.TOO_MANY_ROWS, 1) == 64


# ---------------------------------------------------------------------------------------------------------------- the library's tile count
RANGES = 5


class Entry(C.Structure):                                                # pmt_rider_entry (include/parametron_hip.h)
    _fields_ = [("kind", C.c_int32), ("lane", C.c_int32), ("rows", C.c_int64), ("cols", C.c_int64),
                ("reads", (C.c_uint64 * 2) * RANGES), ("writes", (C.c_uint64 * 2) * RANGES)]


def _library_tiles(lib, rows, cols):
    """a persistent node (64 x 2112) with one independent pack of rows x cols behind it: (rides, tiles)"""
    slot = 1 << 40
    node, pack = Entry(1, 0, 64, 2112), Entry(2, 0, rows, cols)
    for e, n_r, n_w in ((node, 4, 4), (pack, 4, 2)):
        base = slot if e is node else 16 * slot
        for k in range(n_r):
            e.reads[k][0], e.reads[k][1] = base + k * slot, base + k * slot + 8
        for k in range(n_w):
            e.writes[k][0], e.writes[k][1] = base + (8 + k) * slot, base + (8 + k) * slot + 8
    arr = (Entry * 2)(node, pack)
    rides = (C.c_int * 2)()
    count, tiles = C.c_int(-1), C.c_int64(-1)
    lib.call("pmt_plan_rider_check", C.cast(arr, C.c_void_p), 2, 0, rides, C.byref(count), C.byref(tiles))
    return list(rides), tiles.value


def test_the_restated_tile_count_is_the_librarys():
    import __graft_entry__ as entry
    entry.build()
    from parametron_jl_amd import _lib
    shapes = sorted({(s.rows, s.cols) for s in _all_specs()} | {(32, 64 * 1024), (33, 64 * 1023), (33, 64 * 1024), (64, 64 * 1023), (65, 64 * 512), (65, 64 * 511)})
    assert (66, 32726) in shapes
    for rows, cols in shapes:
        if 32 * rows * cols > 256 << 20:
            continue
        rides, tiles = _library_tiles(_lib, rows, cols)
        assert rides == [0, 1], (rows, cols)
        assert tiles == U.choice(1, rows, cols, rows).tiles, (rows, cols, tiles)


# ---------------------------------------------------------------------------------------------------------------- the grid's y extent
@pytest.mark.parametrize("name", ["pmt_affine_assemble_f64", "pmt_affine_pack_vector_f64"])
def test_a_block_of_65536_block_rows_is_refused_on_the_host(name):
    """decided by validate_affine_tiles before anything reaches a device (the pointers are never read)"""
    import __graft_entry__ as entry
    entry.build()
    from parametron_jl_amd import _lib
    buf = np.zeros(4)
    p = buf.ctypes.data_as(C.c_void_p)
    tail = (p, p, None) if name == "pmt_affine_assemble_f64" else (None, 0, p, p, None)
    with pytest.raises(_lib.DimensionMismatch, match="65535"):
        _lib.call(name, p, U.TOO_MANY_ROWS, U.TOO_MANY_ROWS, 1, p, p, -1, *tail)
    with pytest.raises(_lib.DimensionMismatch, match="65535"):
        _lib.call(name, p, 2 * U.TOO_MANY_ROWS, 2 * U.TOO_MANY_ROWS, 3, p, None, 0, *tail)
