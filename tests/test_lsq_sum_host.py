"""CPU-only: the weighted least-squares sum entry point (pmt_quad_gram_sum_f64) is exported, bound in Python and Julia, and validates its
arguments before any launch."""
import ctypes as C
import os
import re

import pytest

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000            # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def lib():
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


def _block(lib, first=False, values=FAKE):
    return {"kind": lib.PMT_LSQ_BLOCK} if first else {"kind": lib.PMT_LSQ_BLOCK, "values": values, "lin": FAKE, "constant": FAKE}


def _call(lib, terms, cols=8):
    arr = lib.lsq_terms(terms)
    lib.call("pmt_quad_gram_sum_f64", cols, C.addressof(arr), len(terms), FAKE, FAKE, FAKE, None)


def test_sum_entry_point_is_exported_and_bound(lib):
    raw = C.CDLL(lib.LIB_PATH)
    assert hasattr(raw, "pmt_quad_gram_sum_f64")
    assert "pmt_quad_gram_sum_f64" in lib.SIGNATURES
    assert C.sizeof(lib.LsqTerm) == 56
    src = open(os.path.join(ROOT, "julia", "ParametronHIP.jl")).read()
    assert re.search(r"ccall\(\(:pmt_quad_gram_sum_f64, lib\)", src)
    hdr = open(os.path.join(ROOT, "include", "parametron_hip.h")).read()
    for name, value in (("PMT_LSQ_BLOCK", lib.PMT_LSQ_BLOCK), ("PMT_LSQ_DIAG", lib.PMT_LSQ_DIAG), ("PMT_LSQ_LINEAR", lib.PMT_LSQ_LINEAR),
                        ("PMT_LSQ_CONSTANT", lib.PMT_LSQ_CONSTANT), ("PMT_LSQ_MAX_TERMS", lib.PMT_LSQ_MAX_TERMS),
                        ("PMT_LSQ_MAX_BLOCKS", lib.PMT_LSQ_MAX_BLOCKS)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name


def test_sum_rejects_no_block(lib):
    with pytest.raises(lib.ArgumentError):
        _call(lib, [{"kind": lib.PMT_LSQ_DIAG}, {"kind": lib.PMT_LSQ_CONSTANT, "scale": 2.0}])


def test_sum_rejects_nine_blocks(lib):
    with pytest.raises(lib.ArgumentError):
        _call(lib, [_block(lib, first=True)] + [_block(lib) for _ in range(8)])


def test_sum_rejects_null_value_array(lib):
    with pytest.raises(lib.ArgumentError):
        _call(lib, [_block(lib, first=True), _block(lib, values=None)])
    with pytest.raises(lib.ArgumentError):
        _call(lib, [_block(lib, first=True), {"kind": lib.PMT_LSQ_BLOCK, "values": FAKE, "lin": None, "constant": FAKE}])
    with pytest.raises(lib.ArgumentError):
        _call(lib, [_block(lib, first=True), {"kind": lib.PMT_LSQ_LINEAR}])                    # dot(c, x) without c


def test_sum_rejects_bad_shapes_and_lists(lib):
    with pytest.raises(lib.DimensionMismatch):
        _call(lib, [_block(lib, first=True)], cols=-1)
    with pytest.raises(lib.ArgumentError):
        lib.call("pmt_quad_gram_sum_f64", 8, None, 1, FAKE, FAKE, FAKE, None)
    with pytest.raises(lib.ArgumentError):
        _call(lib, [_block(lib, first=True)] + [{"kind": lib.PMT_LSQ_CONSTANT}] * lib.PMT_LSQ_MAX_TERMS)   # 33 terms
    with pytest.raises(lib.ArgumentError):
        _call(lib, [_block(lib, first=True), {"kind": 7}])
    with pytest.raises(lib.ArgumentError):
        _call(lib, [_block(lib, first=True), {"kind": lib.PMT_LSQ_DIAG, "vec": FAKE, "sign": 0}])
    arr = lib.lsq_terms([_block(lib, first=True)])
    with pytest.raises(lib.ArgumentError):
        lib.call("pmt_quad_gram_sum_f64", 8, C.addressof(arr), 1, None, FAKE, FAKE, None)       # null output
