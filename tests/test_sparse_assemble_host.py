"""CPU suite for tests/sparse_assemble_util.py, which tests/test_gpu_sparse_assemble.py relies on: the plain-loop restatement of the sparse
node C*x (+|-) d against the oracle bit for bit, four wrong restatements that the same comparison tells apart, the branch edges of the
kernels of csrc/sparse.hip that the named patterns reach (computed from the tables the kernels read, so that a later edit of a pattern
cannot silently lose one), and the refusals of the entry points that are decided before anything reaches the device."""
import ctypes as C

import numpy as np
import pytest

import sparse_assemble_util as U
from oracle import oracle as O
from parametron_jl_amd import _lib

vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


def test_the_data_family_has_every_special():
    a = U.values(40, 1)
    b = U.bits(a)
    assert np.any(b == 0) and np.any(b == np.int64(-2 ** 63)) and np.any(a == U.DENORMAL) and np.any(a == -U.DENORMAL)
    assert np.any(a == np.inf) and np.any(a == -np.inf) and np.any(a > 0.1) and np.any(a < -0.1)
    nan = b[np.isnan(a)]
    assert len(nan) == 1 and nan[0] == 0x7FF8DEAD0000BEEF and nan[0] != U.bits(np.array([np.nan]))[0]
    d = U.values(40, 2, nan=False)
    assert not np.any(np.isnan(d)) and np.any(U.bits(d) == 0) and np.any(U.bits(d) == np.int64(-2 ** 63)) and np.any(np.isinf(d))
    f = U.values(40, 3, zeros=False)
    assert np.all(np.isfinite(f)) and np.all(f != 0.0) and np.any(f == U.DENORMAL)
    assert len(set(U.bits(U.values(1, s))[0] for s in range(9))) == 9                 # a single coefficient takes every special in turn
    vm = U.permuting_varmap(30, 1)
    assert not np.array_equal(vm, np.sort(vm)) and not np.array_equal(U.column_variables(30, 1), np.sort(U.column_variables(30, 1)))


def _inputs(name, seed, **kw):
    pat = U.pattern(name)
    return pat, U.values(pat.nnz, seed, **kw), U.column_variables(pat.n, seed + 1), U.permuting_varmap(pat.n, seed + 2), U.values(pat.m, seed + 3, nan=False)


def _oracle(pat, nzval, xvar, varmap, row_offset, d, sign):
    """the reference's dense builders on the densified matrix, the zero coefficients removed (as tests/test_gpu_sparse.py::_oracle_sparse_rows)"""
    m = pat.m
    f = O.AffVec(m).matvecmul_vars(pat.dense(nzval), xvar)
    if d is not None and sign:
        f = O.AffVec(m).vecaddsub(f, d, sign < 0)
    lt, _, lc = f.flat()
    if row_offset:                                                   # stacked under `row_offset` rows of anything (vcat!, src/functions.jl:870-885)
        top = O.AffVec(row_offset).matvecmul_vars(np.full((row_offset, 1), 1.5), [1])
        vt, vc = O.AffVec(row_offset + m).vcat(top, f).moi(varmap)
        vt, vc = vt[vt["out"] > row_offset], vc[row_offset:]
    else:
        vt, vc = f.moi(varmap)
    assert U.bits(vc).tolist() == U.bits(lc).tolist()
    vt, lt = vt[vt["coeff"] != 0.0], lt[lt["coeff"] != 0.0]
    return vt.view(np.int64).reshape(-1), lt.view(np.int64).reshape(-1), U.bits(lc)


def _same(a, b):
    return all(x.dtype == np.int64 and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


ORACLE_CROSS = [(True, 7, -1), (False, 0, 1), (True, 0, 0), (False, 7, 1)]


@pytest.mark.parametrize("name", U.SMALL_FOR_THE_ORACLE)
def test_the_restatement_against_the_oracle(name):
    pat, nzval, xvar, varmap, d = _inputs(name, 11, zeros=False, nan=False)
    for mapped, row_offset, sign in ORACLE_CROSS:
        args = (varmap if mapped else None, row_offset, d if sign else None, sign)
        want = _oracle(pat, nzval, xvar, *args)
        assert len(want[0]) == 3 * pat.nnz and len(want[1]) == 2 * pat.nnz
        assert _same(U.restate(pat.m, pat.n, pat.colptr, pat.rowval, nzval, xvar, *args), want), (name, mapped, row_offset, sign)


@pytest.mark.parametrize("name", ["five_columns", "column_runs", "holes"])
def test_wrong_restatements_are_rejected(name):
    pat, nzval, xvar, varmap, d = _inputs(name, 11, zeros=False, nan=False)
    for sign in (-1, 1):
        args = (pat.m, pat.n, pat.colptr, pat.rowval, nzval, xvar, varmap, 7, d, sign)
        want = _oracle(pat, nzval, xvar, varmap, 7, d, sign)
        assert _same(U.restate(*args), want)
        for wrong, part in ((U.wrong_column_major, (0, 1)), (U.wrong_lt_mapped, (1,)), (U.wrong_d_minus_zero, (2,)), (U.wrong_row_offset, (0,))):
            got = wrong(*args)
            assert not _same(got, want), (name, wrong.__name__)
            for k in range(3):                                       # ... and it is wrong in the part it names only
                assert np.array_equal(got[k], want[k]) == (k not in part), (name, wrong.__name__, k)


# ---- the coverage claims
def _block_edges():
    return {name: U.block_edges(U.tables(name)) for name in U.NAMED}


def _slab_edges():
    return {(name, nslab): U.slab_edges(U.tables(name), nslab) for name, nslab in U.SLAB_CASES}


def test_the_named_patterns_have_the_shapes_they_are_named_for():
    e = _block_edges()
    want = {"staircase": (12, 1027, 1024, 1, 2), "column_runs": (131, 15, 1024, 2, 1), "capacity": (128, 56, 1024, 1, 1),
            "over_capacity": (128, 57, 32, 1, 2), "nine_bands": (130, 257, 32, 2, 9), "single": (1, 1, 1024, 1, 1)}
    for name, shape in want.items():
        p = U.pattern(name)
        assert (p.m, p.n, e[name]["cw"], e[name]["nrb"], e[name]["ncb"]) == shape, name
    assert U.pattern("capacity").nnz == U.SB_CAP == e["capacity"]["block_fill_max"]
    assert e["over_capacity"]["ragged_last_band"] == 25 and e["nine_bands"]["ragged_last_row_block"] == 2
    assert set(e["staircase"]["row_runs"]) == {0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 192, 193, 300}
    assert set(e["column_runs"]["column_runs"]) == {0, 1, 2, 3, 5, 15, 16, 17, 18, 19, 24, 25, 127, 128}
    assert e["column_runs"]["pair_load_at_the_last_coefficient"]
    h = U.pattern("holes")
    assert 250 <= h.m <= 270 and 60 <= h.n <= 80 and not h.mask[128:256].any() and not h.mask[0].any() and not h.mask[-1].any()
    assert e["holes"]["empty_row_block"] and np.any(h.mask.sum(axis=0) == 0) and h.mask[256:].any()
    for name in U.NAMED:
        assert U.pattern(name).m <= 300 and U.pattern(name).n <= 1027
    assert U.pattern("flat_long").nnz == U.FLAT_GRID + 3


def test_the_patterns_reach_the_block_kernels_edges():
    e = _block_edges()
    widths = set(v["cw"] for v in e.values())
    assert {32, 1024} <= widths and any(32 < w < 1024 for w in (e[n]["cw"] for n in U.NAMED if n.startswith("random")))
    col = set().union(*(v["column_runs"] for v in e.values()))
    assert {0, 1, 2, 15, 16, 17, 18, 128} <= col                     # the pair load, the len > 16 tail loop, a full column
    row = set().union(*(v["row_runs"] for v in e.values()))
    assert {0, 1, 63, 64, 65, 128, 129} <= row and max(row) > 192
    assert {1, 2, 3, 4, 5} <= set().union(*(v["write_rounds"] for v in e.values()))
    assert any(v["block_fill_max"] == U.SB_CAP for v in e.values())
    assert any(v["empty_row_block"] for v in e.values()) and any(v["empty_block"] for v in e.values())
    assert any(v["ncb"] >= 9 and v["idle_workgroups"] > 0 for v in e.values())
    assert any(v["pair_load_at_the_last_coefficient"] for v in e.values())
    assert any(v["ragged_last_band"] for v in e.values()) and any(v["ragged_last_row_block"] for v in e.values())
    # the 16-byte repacking: both leads and both kinds of tail for 2-word and 3-word terms — only because the destination also runs at
    # 8 mod 16: at an aligned base a run of 2-word terms never starts on an odd word
    par = set().union(*(v["parities"] for v in e.values()))
    assert par == {(W, lead, tail) for W in (2, 3) for lead in (0, 1) for tail in (0, 1) if W == 3 or lead == tail}
    for name in U.NAMED:
        t = U.tables(name)
        band = t.band.reshape(t.pat.m, t.ncb + 1)
        starts = band[:, :-1][np.diff(band, axis=1) > 0]
        assert set((2 * starts) & 1) <= {0}, name                    # the lead of an LT run at an aligned base
    assert {(W, lead) for W, lead, _ in par} == {(2, 0), (2, 1), (3, 0), (3, 1)}


def test_the_patterns_reach_the_slab_kernels_edges():
    e = _slab_edges()
    assert {1, 3, 8, 64} == set(v["nslab"] for v in e.values())
    assert {0, 1, 15} <= set(v["rows_mod_16"] for v in e.values()) and {1, 15, 16, 17, 33} <= set(U.pattern(n).m for n, _ in e)
    seg = set().union(*(v["segments"] for v in e.values()))
    assert {0, 1, 63, 64, 65, 129} <= seg
    assert {1, 2, 3} <= set().union(*(v["rounds"] for v in e.values()))
    assert any(v["four_different_rows"] for v in e.values())
    assert any(v["empty_slab"] for v in e.values()) and e[("five_columns", 8)]["more_slabs_than_columns"] and U.pattern("five_columns").n == 5
    par = set().union(*(v["parities"] for v in e.values()))
    assert par == {(W, lead, tail) for W in (2, 3) for lead in (0, 1) for tail in (0, 1) if W == 3 or lead == tail}
    assert sorted(U.RAGGED_LENGTHS[:4]) == [0, 1, 65, 129] and e[("ragged16", 1)]["four_different_rows"]


def test_the_edges_table_lists_every_case():
    """the table of pattern -> edges (python -m pytest -s prints it) has a line for every block-form and slab-form case of the GPU tests"""
    lines = ["block  %-15s %s" % (name, {k: (sorted(x) if isinstance(x, set) else x) for k, x in v.items()}) for name, v in _block_edges().items()]
    lines += ["slab   %-15s %s" % (name, {k: (sorted(x) if isinstance(x, set) else x) for k, x in v.items()}) for (name, _), v in _slab_edges().items()]
    print("\n" + "\n".join(lines))
    assert len(lines) == len(U.NAMED) + len(U.SLAB_CASES) and all(U.tables(name).cw > 0 for name in U.NAMED + U.SLAB_MADE)


# ---- refusals that are decided on the host: PMT_REQUIRE runs before anything is handed to the device
class _Args:
    """host arrays standing in for every pointer of an entry point: a refused call may not touch them (nor follow them)"""

    def __init__(self):
        self.a = {k: U.WORD + np.arange(64, dtype=np.int64) + 1000 * i for i, k in enumerate(
            ("nzval", "perm", "trow", "tvar", "slab", "varmap", "out", "desc", "idx", "band", "colvar", "d", "consts"))}
        self.before = {k: v.copy() for k, v in self.a.items()}

    def __getattr__(self, k):
        return vp(self.a[k])

    def untouched(self):
        return all(np.array_equal(self.a[k], self.before[k]) for k in self.a)


def _flat(h, vat, nnz=5, null=None):
    p = {k: (None if k == null else getattr(h, k)) for k in ("nzval", "perm", "trow", "tvar", "out")}
    if vat:
        return "pmt_sparse_pack_vector_f64", (p["nzval"], p["perm"], p["trow"], p["tvar"], nnz, h.varmap, 7, p["out"], None)
    return "pmt_sparse_assemble_f64", (p["nzval"], p["perm"], p["tvar"], nnz, p["out"], None)


def _slab(h, vat, u32, rows=3, nslab=2, null=None):
    p = {k: (None if k == null else getattr(h, k)) for k in ("nzval", "perm", "tvar", "slab", "out")}
    name = "pmt_sparse_%s_slabs_%sf64" % ("pack_vector" if vat else "assemble", "u32_" if u32 else "")
    if vat:
        return name, (p["nzval"], p["perm"], p["tvar"], p["slab"], rows, nslab, h.varmap, 7, p["out"], None)
    return name, (p["nzval"], p["perm"], p["tvar"], p["slab"], rows, nslab, p["out"], None)


def _blocks(h, vat, rows=3, cols=4, nnz=5, cw=32, sign=-1, d=True, consts=True, null=None):
    p = {k: (None if k == null else getattr(h, k)) for k in ("nzval", "desc", "idx", "band", "colvar", "out")}
    dd, cc = (h.d if d else None), (h.consts if consts else None)
    if vat:
        return "pmt_sparse_pack_vector_blocks_f64", (p["nzval"], p["desc"], p["idx"], p["band"], p["colvar"], rows, cols, nnz, cw, h.varmap, 7, dd, sign,
                                                     p["out"], cc, None)
    return "pmt_sparse_assemble_blocks_f64", (p["nzval"], p["desc"], p["idx"], p["band"], p["colvar"], rows, cols, nnz, cw, dd, sign, p["out"], cc, None)


def _refusals():
    h = _Args()
    DM, AE = _lib.DimensionMismatch, _lib.ArgumentError
    cases = []
    for vat in (True, False):
        cases.append(("negative nnz", DM, _flat(h, vat, nnz=-1)))
        cases += [("null %s" % k, AE, _flat(h, vat, null=k)) for k in ("nzval", "perm", "tvar", "out") + (("trow",) if vat else ())]
        for u32 in (False, True):
            cases += [("nslab %d" % s, DM, _slab(h, vat, u32, nslab=s)) for s in (0, 65)]
            cases.append(("negative rows", DM, _slab(h, vat, u32, rows=-1)))
            cases += [("null %s" % k, AE, _slab(h, vat, u32, null=k)) for k in ("nzval", "perm", "tvar", "slab", "out")]
        cases += [("cw %d" % cw, AE, _blocks(h, vat, cw=cw)) for cw in (16, 48, 2048, 0, -32)]
        cases += [("nnz %d" % k, DM, _blocks(h, vat, nnz=k)) for k in (-1, 2 ** 32)]
        cases += [("negative %s" % k, DM, _blocks(h, vat, **{k: -1})) for k in ("rows", "cols")]
        cases += [("sign %d" % s, AE, _blocks(h, vat, sign=s)) for s in (2, -2)]
        cases += [("sign %d without d" % s, AE, _blocks(h, vat, sign=s, d=False)) for s in (1, -1)]
        cases += [("sign %d without d, nnz 0" % s, AE, _blocks(h, vat, sign=s, d=False, nnz=0)) for s in (1, -1)]
        cases += [("null %s" % k, AE, _blocks(h, vat, null=k)) for k in ("nzval", "desc", "idx", "band", "colvar", "out")]
    return h, cases


def test_refused_calls_raise_and_touch_nothing():
    h, cases = _refusals()
    assert len(set(name for _, _, (name, _) in cases)) == 8         # flat, slab, slab u32 and block form, each as terms and as triplets
    for what, exc, (name, args) in cases:
        with pytest.raises(exc):
            _lib.call(name, *args)
            pytest.fail("%s accepted %s" % (name, what))
        assert h.untouched(), (name, what)


def test_empty_calls_are_accepted_on_the_host_and_touch_nothing():
    """nnz == 0 / rows == 0 return before the pointers are looked at: null pointers pass, and nothing is written"""
    h = _Args()
    for vat in (True, False):
        for call in (_flat(h, vat, nnz=0), _flat(h, vat, nnz=0, null="out"), _slab(h, vat, False, rows=0), _slab(h, vat, True, rows=0, null="nzval"),
                     _blocks(h, vat, rows=0), _blocks(h, vat, nnz=0, consts=False), _blocks(h, vat, cols=0, consts=False, null="desc"),
                     _blocks(h, vat, rows=0, cw=48)):
            _lib.call(*((call[0],) + call[1]))
            assert h.untouched(), call[0]
