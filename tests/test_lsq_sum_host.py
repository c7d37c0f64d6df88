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


# ================================================================== tests/lsq_sum_util.py, which tests/test_gpu_lsq_sum_abi.py relies on
import numpy as np  # noqa: E402

import lsq_sum_util as U  # noqa: E402
from lsq_sum_util import Term  # noqa: E402
from oracle import oracle as O  # noqa: E402


# ---- the restatement against the oracle, bit for bit, on exact data: small integers and dyadic weights make every product and sum exact,
# so the order of summation cannot matter and the oracle's canonicalize! of the literal expression is THE answer
class _Block(Term):
    """dot(r, r), r = A*x (+|-) b, with its exact MOI blocks: 2 A'A, 2 A'c and c'c for c = 0.0 (+|-) b"""

    def __init__(self, rng, rows, n, bsign, scale=1.0, weight=None):
        self.A, self.b, self.bsign = rng.integers(-3, 4, (rows, n)).astype(np.float64), rng.integers(-4, 5, rows).astype(np.float64), bsign
        c = (0.0 + self.b) if bsign > 0 else (0.0 - self.b)
        self.P, q = 2 * (self.A.T @ self.A), 2 * (self.A.T @ c)
        j, k = np.triu_indices(n)
        values = np.empty(len(j))
        values[k * (k + 1) // 2 + j] = self.P[j, k]
        super().__init__("block", scale, weight, values=values, lin=q, constant=float(c @ c))


def _oracle_term(t, x):
    n = len(x)
    if t.kind == "block":
        r = O.AffVec(t.A.shape[0]).vecaddsub(O.AffVec(t.A.shape[0]).matvecmul_vars(t.A, x), t.b, t.bsign < 0)
        return O.Quad().vecdot_affs_affs(r, r)
    xs = x if t.cols is None else x[t.cols]
    if t.kind == "diag":
        if t.v is None:
            return O.Quad().vecdot_vars_vars(xs, xs)
        s = O.AffVec(len(xs)).vecaddsub(xs, t.v, t.sign < 0)
        return O.Quad().vecdot_affs_affs(s, s)
    if t.kind == "linear":
        return O.Quad().copy_from_aff(O.vecdot_aff_numbers_vars(t.v, xs))
    return O.Quad(constant=1.0 if t.value is None else t.value)


def _exact_shapes():
    def ints(rng, m):
        return rng.integers(-5, 6, m).astype(np.float64)

    def make(n, build):
        rng = np.random.default_rng(n)
        return n, build(rng, n)
    B = _Block
    return {
        "ridge": make(6, lambda r, n: [B(r, 9, n, -1), Term("diag", 0.5, 0.25)]),
        "tracking x + v": make(5, lambda r, n: [B(r, 7, n, -1), Term("diag", -2.0, v=ints(r, n), sign=1)]),
        "tracking x - v": make(5, lambda r, n: [B(r, 7, n, 1, 0.5), Term("diag", 1.0, 4.0, v=ints(r, n), sign=-1)]),
        "linear": make(4, lambda r, n: [B(r, 3, n, -1, -1.0), Term("linear", 0.25, v=ints(r, n))]),
        "constant": make(4, lambda r, n: [B(r, 5, n, -1), Term("constant", 3.0), Term("constant", -0.5, 2.0, value=7.0)]),
        "two blocks": make(7, lambda r, n: [B(r, 4, n, -1, 2.0), B(r, 9, n, 1, -0.5, 0.5)]),
        "three blocks": make(5, lambda r, n: [B(r, 4, n, -1, 1.0, 0.25), Term("diag", 1.0), B(r, 2, n, 1, 4.0), Term("linear", -1.0, v=ints(r, n)), B(r, 6, n, -1, -1.0)]),
        "subset diagonal": make(8, lambda r, n: [B(r, 5, n, -1), Term("diag", 0.5, v=ints(r, 4), sign=-1, cols=[0, 3, 4, 7]), Term("diag", 2.0, cols=[3, 5]),
                                                  Term("linear", 1.0, 0.5, v=ints(r, 2), cols=[1, 7])]),
        "block 1 second": make(6, lambda r, n: [Term("diag", 0.5, 0.5), B(r, 8, n, -1, 2.0)]),
        "block 1 fourth": make(6, lambda r, n: [Term("diag", 1.0, v=ints(r, n), sign=1), Term("linear", 2.0, v=ints(r, n)), Term("constant", 0.5), B(r, 8, n, 1),
                                                 B(r, 3, n, -1, 0.25)]),
        "one block at weight +1, 66 columns": make(66, lambda r, n: [B(r, 2, n, -1), Term("diag", 0.5, cols=np.arange(1, 66))]),
        "two tiles of columns": make(66, lambda r, n: [Term("diag", 0.5), B(r, 2, n, -1, 2.0), B(r, 1, n, 1)]),
    }


def _block1_image(t, n):
    j, k = np.triu_indices(n)
    q = np.zeros(len(j), dtype=[("coeff", "<f8"), ("row", "<i8"), ("col", "<i8")])
    q["coeff"], q["row"], q["col"] = t.P[j, k], j + 1, k + 1
    l = np.zeros(n, dtype=[("coeff", "<f8"), ("var", "<i8")])
    l["coeff"], l["var"] = t.lin, np.arange(1, n + 1)
    return q.view(np.int64), l.view(np.int64), t.constant


def _against_the_oracle(n, terms, flaw=None):
    """the first difference between the restatement and the oracle's canonical function, or None"""
    x = np.arange(1, n + 1, dtype=np.int64)
    total = O.Quad()
    for t in terms:
        total.add_quad(O.Quad().mul_quad_number(_oracle_term(t, x), t.W))
    at, qt, oconst = total.canonicalize().moi()
    quad, lin, const, masks = U.restate(n, terms, *_block1_image(terms[U.first_block(terms)], n), flaw=flaw)
    assert not masks[0].any() and not masks[1].any() and not masks[2]
    want = {(int(r), int(c)): float(v) for v, r, c in zip(qt["coeff"], qt["row"], qt["col"])}
    assert len(want) == len(qt) and all(r <= c for r, c in want)                          # canonical: every pair once, upper triangle
    quad, lin = quad.reshape(-1, 3), lin.reshape(-1, 2)
    got = {(int(r), int(c)): float(v) for v, r, c in zip(quad[:, 0].copy().view(np.float64), quad[:, 1], quad[:, 2])}
    if set(want) - set(got):
        return "the oracle has pairs the restatement has not"
    for key, v in got.items():                                                            # (an exact 0 may be absent from the oracle's list)
        if U.bits([v])[0] != U.bits([want.get(key, v if v == 0.0 else np.nan)])[0] and not (v == 0.0 == want.get(key)):
            return "quad %s: %r, oracle %r" % (key, v, want.get(key))
    wl = {int(v): float(c) for c, v in zip(at["coeff"], at["var"])}
    for c, v in zip(lin[:, 0].copy().view(np.float64), lin[:, 1]):
        if float(c) != wl.get(int(v), 0.0):
            return "lin %d: %r, oracle %r" % (v, c, wl.get(int(v)))
    if const != oconst:
        return "constant %r, oracle %r" % (const, oconst)
    return None


@pytest.mark.parametrize("shape", list(_exact_shapes()))
def test_the_restatement_against_the_oracle_on_exact_data(lib, shape):
    n, terms = _exact_shapes()[shape]
    assert _against_the_oracle(n, terms) is None


def test_wrong_restatements_are_rejected_by_the_oracle(lib):
    """the flaws that exact data can show: the later blocks looped from term 1 (block 1 counted twice), D on every tile's local diagonal"""
    shapes = _exact_shapes()
    assert _against_the_oracle(*shapes["block 1 second"], flaw="blocks_from_term_1") is not None
    assert _against_the_oracle(*shapes["block 1 fourth"], flaw="blocks_from_term_1") is not None
    assert _against_the_oracle(*shapes["two tiles of columns"], flaw="d_on_every_tile_diagonal") is not None
    for flaw in ("plus_zero", "sequential_sumsq"):                   # (neither shows on exact data without a -0.0: that is what the named cases are for)
        assert _against_the_oracle(*shapes["subset diagonal"], flaw=flaw) is None


REJECTED_BY = {"plus_zero": ("negzero_weight_one_unlisted", "negzero_fast", "fast_listed_diag"), "d_on_every_tile_diagonal": ("n65_K8", "n193"),
               "blocks_from_term_1": ("n63_block1_second", "n128_block1_fourth", "fast_listed_diag"), "sequential_sumsq": ("n513", "sd_257")}


@pytest.mark.parametrize("flaw", list(U.WRONG))
def test_wrong_restatements_are_rejected_by_named_cases(flaw):
    assert set(REJECTED_BY) == set(U.WRONG)
    for name in REJECTED_BY[flaw]:
        c = U.case(name)
        right, wrong = c.restated(), U.restate(c.n, c.terms, c.quad, c.lin, c.const, flaw=flaw)
        same = np.array_equal(right[0], wrong[0]) and np.array_equal(right[1], wrong[1]) and U.bits([right[2]])[0] == U.bits([wrong[2]])[0]
        assert not same, (flaw, name)
        # the difference is outside the words the NaN rule masks: a GPU result equal to the wrong restatement fails the comparison
        dq, dl = (right[0] != wrong[0]).reshape(-1, 3)[:, 0] & ~right[3][0], (right[1] != wrong[1]).reshape(-1, 2)[:, 0] & ~right[3][1]
        assert dq.any() or dl.any() or (U.bits([right[2]])[0] != U.bits([wrong[2]])[0] and not right[3][2]), (flaw, name)


# ---- the tables
def test_the_tables_hold_what_they_name():
    cs = U.cases()
    plain = [c for c in cs.values() if not c.sub]
    assert {0, 1, 2, 63, 64, 65, 128, 129, 193, 513} <= {c.n for c in plain}
    blocks = lambda c: sum(t.kind == "block" for t in c.terms)                    # noqa: E731
    assert {1, 2, 8} <= {blocks(c) for c in plain} and {0, 1, 3} <= {U.first_block(c.terms) for c in plain}
    assert len(cs["n129_32_terms"].terms) == 32 == len(cs["list_32_terms"].terms) and blocks(cs["list_32_terms"]) == 8 == blocks(cs["n129_32_terms"])
    assert U.first_block(cs["n63_block1_second"].terms) == 1 and cs["n63_block1_second"].terms[0].kind == "diag"
    assert U.first_block(cs["n128_block1_fourth"].terms) == 3
    assert all(max(blocks(c), 1) <= U.MAX_BLOCKS and len(c.terms) <= U.MAX_TERMS and U.total_runs(c.terms) <= U.MAX_RUNS and c.n <= 513 for c in cs.values())
    assert U.total_runs(cs["list_64_runs"].terms) == 64 and U.total_runs(cs["list_32_terms"].terms) == 56
    lists = lambda name: [t.cols.tolist() for t in cs[name].terms if t.cols is not None]          # noqa: E731
    assert [] in lists("list_empty") and lists("list_first") == [[0], [0]] and lists("list_last") == [[69], [69]]
    assert lists("list_all_but_0")[0] == list(range(1, 70))
    a, b = [t for t in cs["two_diags_overlapping"].terms if t.kind == "diag"]
    assert a.v is not None and a.sign == 1 and b.v is None and set(a.cols) & set(b.cols) and set(a.cols) - set(b.cols) and set(b.cols) - set(a.cols)
    ld = cs["listed_linear_full_diag"].terms
    assert ld[0].kind == "linear" and ld[0].cols is not None and ld[2].kind == "diag" and ld[2].cols is None
    assert [len(cs["sd_%d" % m].terms[1].v) for m in (1, 255, 256, 257)] == [1, 255, 256, 257]
    for name, ndiag, listed in (("fast_no_diag", 0, False), ("fast_full_diag", 1, False), ("fast_listed_diag", 1, True), ("negzero_fast", 1, True)):
        d = [t for t in cs[name].terms if t.kind == "diag"]
        assert U.is_fast(cs[name].terms) and len(d) == ndiag and all((t.cols is not None) == listed for t in d), name
    assert not any(U.is_fast(c.terms) for n_, c in cs.items() if not n_.startswith(("fast_", "negzero_fast", "n0")))
    # the weights: a pure scale and scale * device scalar; +1, -1, 0 and a value that is no power of two
    ws = [(t.scale, t.weight) for c in cs.values() for t in c.terms]
    assert any(w is None for _, w in ws) and any(w is not None for _, w in ws)
    assert {1.0, -1.0, 0.0, 0.7} <= {t.W for c in cs.values() for t in c.terms}
    # every sub case has a list, every plain one has none; the plan and slice cases exist
    assert all(c.sub == any(t.cols is not None for t in c.terms) for c in cs.values())
    assert not cs[U.RECORDED[0]].sub and cs[U.RECORDED[1]].sub and [cs[s].n for s in U.SLICES] == [65, 64] and cs[U.SLICES[0]].nq % 2 == 1


def test_the_data_family():
    v = U.values(65, 3, hot=True, nan=True)
    w = U.bits(v).view(np.uint64).tolist()
    assert 0 in w and 0x8000000000000000 in w and 0x7FF8DEAD0000BEEF in w and np.sum(np.isinf(v)) == 2 and np.sum((v != 0) & (np.abs(v) < 1e-300)) == 2
    assert not np.any(np.isnan(U.values(65, 3, hot=True))) and not np.any(np.isinf(U.values(65, 3)))
    assert np.array_equal(np.flatnonzero(np.isinf(v)), np.flatnonzero(np.isinf(U.values(65, 9, hot=True))))        # the same places in every vector
    assert np.all(np.isfinite(U.values(5, 1, hot=True, nan=True))) and len(U.values(0, 1)) == 0
    assert (int(U.bits([U.SIGNALLING])[0]) >> 51) & 1 == 0 and np.isnan(U.SIGNALLING)


@pytest.mark.parametrize("name", list(U.cases()))
def test_the_cap_on_masked_words(name):
    c = U.case(name)
    nquad, nlin, cnan = U.masked_counts(c.restated()[3])
    assert nquad <= 0.02 * c.nq and nlin <= c.n / 8 and cnan == (name == "constant_nan"), (name, nquad, c.nq, nlin, c.n, cnan)
    if name == "constant_nan":
        assert np.isnan(c.restated()[2])


@pytest.mark.parametrize("name", ["negzero_weight_one_unlisted", "negzero_no_diag", "negzero_fast"])
def test_minus_zero_comes_back_as_minus_zero(name):
    c = U.case(name)
    qw, lw = c.negzero_words()
    assert len(qw) >= 6 and len(lw) >= 3
    quad, lin = c.restated()[:2]
    assert np.all(c.quad[qw] == U.NEG_ZERO_BITS) and np.all(c.lin[lw] == U.NEG_ZERO_BITS)
    assert np.all(quad[qw] == U.NEG_ZERO_BITS) and np.all(lin[lw] == U.NEG_ZERO_BITS)
    if name != "negzero_no_diag":                                    # with a diagonal term about: + 0.0 at the unlisted positions would show
        wrong = U.restate(c.n, c.terms, c.quad, c.lin, c.const, flaw="plus_zero")
        dj = [3 * int(p) for p in U.diag_positions(c.n)[list(c.negzero[0])]]
        assert np.all(wrong[0][dj] == 0) and np.all(wrong[1][lw] == 0)


def test_untouched_words_keep_a_signalling_nan():
    for name in ("fast_no_diag", "fast_listed_diag"):
        c = U.case(name)
        at = [3 * int(p) for p in U.diag_positions(c.n)[list(c.signalling)]]
        assert len(at) >= 2 and np.all(c.restated()[0][at] == U.bits([U.SIGNALLING])[0]) and not c.restated()[3][0][[a // 3 for a in at]].any()


# ---- the edges
NAMED_EDGES = {
    "n0": {"no columns"}, "n1": {"one-term segment", "ragged last tile"}, "n64": {"full last tile", "second round of a lane"},
    "n65_K8": {"off-diagonal tile next to the diagonal", "one-term segment", "lead word", "no lead word", "single tail word", "tail pair", "term without a list"},
    "n128_block1_fourth": {"full last tile"}, "n193": {"off-diagonal tile not next to the diagonal"}, "fast_no_diag": {"diagonal-only form"},
    "list_empty": {"empty list", "find: miss"}, "list_first": {"find: hit at position 0", "find: miss right behind a run"},
    "list_last": {"find: hit at position cols - 1", "find: miss right before a run"}, "list_all_but_0": {"find: miss right before a run", "find: hit at run end"},
    "list_64_runs": {"64 runs", "find: hit in a later run", "find: miss right behind a run"},
    "two_diags_overlapping": {"find: hit at run start", "find: hit at run end", "find: hit inside a run", "find: miss right behind a run"},
}


def test_every_edge_is_reached_and_named_cases_reach_theirs():
    reached = {}
    for name, c in U.cases().items():
        for shift in (0, 1):
            reached[name, shift] = U.edges(c, shift)
    assert set().union(*reached.values()) == U.ALL_EDGES
    for name, want in NAMED_EDGES.items():
        for shift in (0, 1):
            assert want <= reached[name, shift], (name, shift, want - reached[name, shift])
    # both parities of a segment's first word and of its last at BOTH alignments of out_quad, in the slice cases too
    for name in ("n65_K8", "n64", "n193"):
        for shift in (0, 1):
            assert {"lead word", "no lead word", "single tail word", "tail pair"} <= reached[name, shift], (name, shift)
    assert U.runs([0, 1, 2, 9, 30, 31, 69]) == [(0, 3, 0), (9, 1, 3), (30, 2, 4), (69, 1, 6)] and U.runs([]) == []


# ---- host-side refusals touch nothing: the argument arrays stand in host memory between guard words
GUARD_WORD, NGUARD = 0x5EED5EED5EED5EED, 4


def _refused(lib, exc, cols, terms, lists=None, counts=None, out=(FAKE, FAKE, FAKE), nterms=None, sub=True, no_counts=False, no_terms=False):
    nt = len(terms)
    parts = [np.frombuffer(bytes(lib.lsq_terms(terms)), dtype=np.int64)[:7 * nt]]
    if lists is not None:
        lists = [None if a is None else np.asarray(a, dtype=np.int64) for a in lists]
        counts = np.asarray([0 if a is None else len(a) for a in lists] if counts is None else counts, dtype=np.int64)
        parts += [np.zeros(nt, dtype=np.int64), counts] + [a for a in lists if a is not None]
    at, total = [], NGUARD
    for p in parts:
        at.append(total)
        total += len(p) + NGUARD
    buf = np.full(total, GUARD_WORD, dtype=np.int64)
    for o, p in zip(at, parts):
        buf[o:o + len(p)] = p
    addr = lambda o: buf.ctypes.data + 8 * o                                         # noqa: E731
    if lists is not None:
        rest = iter(at[3:])
        buf[at[1]:at[1] + nt] = [0 if a is None else addr(next(rest)) for a in lists]
    before = buf.copy()
    tp = None if no_terms else addr(at[0])
    with pytest.raises(exc):
        if sub:
            lib.call("pmt_quad_gram_sum_sub_f64", cols, tp, nt if nterms is None else nterms, addr(at[1]) if lists is not None else None,
                     None if (lists is None or no_counts) else addr(at[2]), *out, None)
        else:
            lib.call("pmt_quad_gram_sum_f64", cols, tp, nt if nterms is None else nterms, *out, None)
    assert np.array_equal(buf, before), "a refused call wrote to its arguments"


def test_refusals_leave_the_argument_arrays_alone(lib):
    A, D = lib.ArgumentError, lib.DimensionMismatch
    b1, blk = _block(lib, first=True), _block(lib)
    diag, lin, cst = {"kind": lib.PMT_LSQ_DIAG}, {"kind": lib.PMT_LSQ_LINEAR, "vec": FAKE}, {"kind": lib.PMT_LSQ_CONSTANT}
    for sub in (False, True):                                        # sum_args, through both entries
        _refused(lib, D, -1, [b1], sub=sub)
        _refused(lib, A, 8, [b1], sub=sub, no_terms=True)
        _refused(lib, A, 8, [b1], sub=sub, nterms=0)
        _refused(lib, A, 8, [b1] + [cst] * 32, sub=sub)
        _refused(lib, A, 8, [b1, _block(lib, values=None)], sub=sub)
        _refused(lib, A, 8, [b1, {"kind": lib.PMT_LSQ_BLOCK, "values": FAKE, "lin": FAKE, "constant": None}], sub=sub)
        _refused(lib, A, 8, [b1, {"kind": lib.PMT_LSQ_DIAG, "vec": FAKE, "sign": 2}], sub=sub)
        _refused(lib, A, 8, [b1, {"kind": lib.PMT_LSQ_LINEAR}], sub=sub)
        _refused(lib, A, 8, [b1, {"kind": 0}], sub=sub)
        _refused(lib, A, 8, [diag, cst], sub=sub)
        _refused(lib, A, 8, [b1] + [blk] * 8, sub=sub)
        _refused(lib, A, 8, [b1], sub=sub, out=(FAKE, FAKE, None))
        _refused(lib, A, 8, [b1], sub=sub, out=(None, FAKE, FAKE))
        _refused(lib, A, 8, [b1], sub=sub, out=(FAKE, None, FAKE))
    # the list walk of the sub entry
    _refused(lib, A, 8, [b1, diag], lists=[[1, 2], None])                                   # a list for a block
    _refused(lib, A, 8, [b1, cst], lists=[None, [1]])                                       # ... for a constant
    _refused(lib, A, 8, [b1, diag], lists=[None, [1]], no_counts=True)
    _refused(lib, D, 8, [b1, diag], lists=[None, [1]], counts=[0, -1])
    _refused(lib, D, 8, [b1, diag], lists=[None, list(range(8)) + [8]])                     # 9 positions of 8 columns
    _refused(lib, D, 8, [b1, diag], lists=[None, [-1, 2]])
    _refused(lib, D, 8, [b1, lin], lists=[None, [2, 8]])
    _refused(lib, A, 8, [b1, lin], lists=[None, [2, 1]])
    _refused(lib, A, 8, [b1, lin], lists=[None, [2, 2]])
    _refused(lib, A, 200, [b1, diag, lin], lists=[None, list(range(0, 80, 2)), list(range(100, 150, 2))])      # 40 + 25 runs: the 65th is refused mid-walk
    _refused(lib, D, 2 ** 31, [b1, diag], lists=[None, [1]])
    _refused(lib, D, 2 ** 31, [b1])


# ---- the subset rule of the weighted sums: the decisions and the compile sites read one function (moi._part_of)
X = [2, 4, 5, 9]


@pytest.mark.parametrize("v, want", [(X, None), ([4, 9], [1, 3]), ([9], [3]), ([], False), ([4, 4], False), ([9, 4], False), ([3], False),
                                     ([4, 10], False)])
def test_the_subset_rule_as_a_table(lib, v, want):
    """None: the whole vector; a list: the positions of a non-empty strictly increasing part of x; False: refused — and both
    predicates refuse a term list exactly where the function refuses the variables of its diagonal or linear term, and the compile
    sites' lists are the function's answers and raise where it refuses"""
    import sparse_gram_util as SG
    from parametron_jl_amd.lazyexpression import LsqTerm
    from parametron_jl_amd.moi import _lsq_sum_combines, _part_of, _sparse_sum_combines, _term_positions
    from test_record_tape_host import _b, _block, _xvars
    from test_sparse_gram_host import _sparse_block
    pos = _part_of(np.array(v, dtype=np.int64), np.array(X, dtype=np.int64))
    if want is None or want is False:
        assert pos is want
    else:
        assert pos.dtype == np.int64 and pos.tolist() == want
    pattern = SG.from_mask(np.ones((6, len(X)), dtype=bool), np.random.default_rng(1))
    dense, sparse = LsqTerm("block", r=_block(6, X)), LsqTerm("block", r=_sparse_block(pattern, X))
    for term in (LsqTerm("diag", xvars=_xvars(v)), LsqTerm("linear", xvars=_xvars(v), vec=_b(len(v)))):
        assert _lsq_sum_combines([dense, term]) == (pos is not False), term.kind
        assert _sparse_sum_combines([sparse, term]) == (pos is not False), term.kind
        if pos is False:
            with pytest.raises(lib.ArgumentError):
                _term_positions([dense, term], np.array(X, dtype=np.int64))
        else:
            first, got = _term_positions([dense, term], np.array(X, dtype=np.int64))
            assert first is None and (got is None if pos is None else got.tolist() == want)
