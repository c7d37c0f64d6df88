"""CPU-only: the stacking entry point (pmt_affine_stack_columns_f64) and the subset sum (pmt_quad_gram_sum_sub_f64) are exported, bound in
Python and Julia, and validate their arguments before any launch; which residuals become stacked ones (lazyexpression._stacked_form)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000            # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def lib():
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


def test_entry_points_are_exported_and_bound(lib):
    raw = C.CDLL(lib.LIB_PATH)
    julia = open(os.path.join(ROOT, "julia", "ParametronHIP.jl")).read()
    for name in ("pmt_affine_stack_columns_f64", "pmt_quad_gram_sum_sub_f64"):
        assert hasattr(raw, name)
        assert name in lib.SIGNATURES
        assert re.search(r"ccall\(\(:%s, lib\)" % name, julia), name
    hdr = open(os.path.join(ROOT, "include", "parametron_hip.h")).read()
    assert re.search(r"#define PMT_LSQ_MAX_RUNS %d\b" % lib.PMT_LSQ_MAX_RUNS, hdr)
    assert lib.STACK_COLUMN.itemsize == 16 and lib.STACK_COLUMN.fields["sign"][1] == 8


# ---- pmt_affine_stack_columns_f64
def _stack(lib, table=FAKE, ncols=4, rows=10, out=FAKE, ldo=10):
    lib.call("pmt_affine_stack_columns_f64", table, ncols, rows, out, ldo, None)


def test_stack_rejects_bad_arguments(lib):
    with pytest.raises(lib.DimensionMismatch):
        _stack(lib, ncols=-1)
    with pytest.raises(lib.DimensionMismatch):
        _stack(lib, rows=-3)
    with pytest.raises(lib.DimensionMismatch):
        _stack(lib, ldo=9)                                   # ldo < rows
    with pytest.raises(lib.ArgumentError):
        _stack(lib, table=None)
    with pytest.raises(lib.ArgumentError):
        _stack(lib, out=None)


def test_stack_table_checks_signs_and_sources(lib):
    t = lib.stack_table([FAKE, FAKE + 8], [1, -1])
    assert t.dtype == lib.STACK_COLUMN and list(t["sign"]) == [1, -1] and list(t["src"]) == [FAKE, FAKE + 8]
    for bad in ([0, 1], [1, 2], [1, -2]):
        with pytest.raises(lib.ArgumentError):
            lib.stack_table([FAKE, FAKE + 8], bad)
    with pytest.raises(lib.ArgumentError):
        lib.stack_table([FAKE, 0], [1, 1])                   # null column source
    with pytest.raises(lib.DimensionMismatch):
        lib.stack_table([FAKE], [1, 1])


# ---- pmt_quad_gram_sum_sub_f64
def _sub(lib, lists, cols=8, kinds=None, counts=None, nterms=None):
    kinds = kinds or [lib.PMT_LSQ_BLOCK] + [lib.PMT_LSQ_DIAG] * (len(lists) - 1)
    terms = lib.lsq_terms([{"kind": k, "vec": FAKE if k != lib.PMT_LSQ_BLOCK else None, "sign": 1} for k in kinds])
    arrs = [np.asarray(p, dtype=np.int64) if p is not None else None for p in lists]
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data if a is not None else None for a in arrs])
    cnt = np.array(counts if counts is not None else [len(a) if a is not None else 0 for a in arrs], dtype=np.int64)
    lib.call("pmt_quad_gram_sum_sub_f64", cols, C.addressof(terms), nterms or len(kinds), C.cast(ptrs, C.c_void_p), cnt.ctypes.data_as(C.c_void_p),
             FAKE, FAKE, FAKE, None)


def test_sub_rejects_bad_lists(lib):
    with pytest.raises(lib.ArgumentError):
        _sub(lib, [None, [3, 2]])                            # not increasing
    with pytest.raises(lib.ArgumentError):
        _sub(lib, [None, [2, 2]])                            # repeated
    with pytest.raises(lib.DimensionMismatch):
        _sub(lib, [None, [5, 8]])                            # beyond cols - 1
    with pytest.raises(lib.DimensionMismatch):
        _sub(lib, [None, [-1, 2]])
    with pytest.raises(lib.DimensionMismatch):
        _sub(lib, [None, [1, 2]], counts=[0, 9])             # more positions than columns
    with pytest.raises(lib.DimensionMismatch):
        _sub(lib, [None, [1, 2]], counts=[0, -1])
    with pytest.raises(lib.ArgumentError):
        _sub(lib, [[0, 1], None])                            # a list for a block
    with pytest.raises(lib.ArgumentError):
        _sub(lib, [None, list(range(0, 260, 2))], cols=300)  # 130 runs of one position
    with pytest.raises(lib.DimensionMismatch):
        _sub(lib, [None, [1]], cols=-1)
    with pytest.raises(lib.ArgumentError):
        lib.call("pmt_quad_gram_sum_sub_f64", 8, None, 1, None, None, FAKE, FAKE, FAKE, None)   # null term list


def test_sub_counts_runs_like_the_host(lib):
    assert lib.column_runs([]) == 0
    assert lib.column_runs([4, 5, 6, 7]) == 1
    assert lib.column_runs([0, 2, 3, 9]) == 3


# ---- which residuals are stacked (host classification; device values built without a device)
def _dvars(idx):
    from parametron_jl_amd.device import DVars
    d = DVars.__new__(DVars)
    d.vars = np.asarray(idx, dtype=np.int64)
    d.n = len(d.vars)
    return d


def _dense(rows, idx, vec=None, sign=0):
    from parametron_jl_amd.device import DDenseAff, DMat
    m = DMat.__new__(DMat)
    m.rows, m.cols, m.lda, m.buf = rows, len(idx), rows, FAKE
    d = DDenseAff.__new__(DDenseAff)
    d.mat, d.xvars, d.vec, d.sign, d.rows = m, _dvars(idx), vec, sign, rows
    return d


def _vec(n):
    from parametron_jl_amd.device import DVec
    v = DVec.__new__(DVec)
    v.n, v.buf = n, FAKE
    return v


def _stacked(blocks, vec, sign):
    from parametron_jl_amd.device import DStackedAff
    s = DStackedAff.__new__(DStackedAff)
    s.blocks, s.vec, s.sign = blocks, vec, sign
    return s


def test_classification(lib):
    from parametron_jl_amd.device import DSparseAff, DVarsAff
    from parametron_jl_amd.lazyexpression import _stacked_form
    Ax, Bu, Cw = _dense(10, [1, 2, 3]), _dense(10, [4, 5]), _dense(10, [6])
    b = _vec(10)
    # A*x + B*u: two blocks, no b
    blocks, vec, sign = _stacked_form(Ax, Bu, +1)
    assert [k for _, _, k in blocks] == [1, 1] and vec is None and sign == 0
    # A*x - B*u: the second block negated
    blocks, _, _ = _stacked_form(Ax, Bu, -1)
    assert [k for _, _, k in blocks] == [1, -1]
    # (A*x + B*u) - b, and (A*x - b) + B*u: b with sign -1
    ab = _stacked(*_stacked_form(Ax, Bu, +1))
    blocks, vec, sign = _stacked_form(ab, b, -1)
    assert vec is b and sign == -1 and len(blocks) == 2
    Axb = _dense(10, [1, 2, 3], vec=b, sign=-1)
    blocks, vec, sign = _stacked_form(Axb, Bu, +1)
    assert vec is b and sign == -1
    # A*x - (B*u - b): b's sign flips with the block's
    Bub = _dense(10, [4, 5], vec=b, sign=-1)
    blocks, vec, sign = _stacked_form(Ax, Bub, -1)
    assert vec is b and sign == 1 and [k for _, _, k in blocks] == [1, -1]
    # (A*x - B*u) + C*w: three blocks
    blocks, _, _ = _stacked_form(_stacked(*_stacked_form(Ax, Bu, -1)), Cw, +1)
    assert [k for _, _, k in blocks] == [1, -1, 1]
    # not stacked: one block (A*x - b), a shared variable, a repeated one, two b, unequal rows, other operand kinds
    assert _stacked_form(Ax, b, -1) is None
    assert _stacked_form(Ax, _dense(10, [3, 4]), +1) is None
    assert _stacked_form(_dense(10, [1, 1]), Bu, +1) is None
    assert _stacked_form(Axb, Bub, +1) is None
    assert _stacked_form(Ax, _dense(11, [4, 5]), +1) is None
    assert _stacked_form(Ax, DVarsAff.__new__(DVarsAff), +1) is None
    assert _stacked_form(Ax, DSparseAff.__new__(DSparseAff), +1) is None
    assert _stacked_form(b, b, +1) is None
