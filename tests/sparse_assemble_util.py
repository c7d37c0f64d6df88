"""What the tests of the sparse assemble / pack kernels (csrc/sparse.hip) share: a restatement of the node C*x (+|-) d by plain loops, the data
family, the named sparsity patterns, poisoned buffer images, and the branch edges of the kernels that a pattern reaches.

The restatement is written from the contract in include/parametron_hip.h and the reference's loops (matvecmul!, src/functions.jl:775-798;
vecadd!/vecsubtract!, :751-764; update!(::MOI.VectorAffineFunction), src/moi_interop.jl:64-81) with the structural zeros left out — not from
the kernels, and it reads nothing the library made: no `perm` of pmt_sparse_rowmajor_order.  tests/test_sparse_assemble_host.py checks it
against the oracle bit for bit, shows that wrong restatements are told apart, and pins the edges below to the named patterns.

Patterns are 1-based colptr / rowval as in a Julia SparseMatrixCSC, built with numpy alone.  Everything is compared as int64 words: a
pmt_vector_affine_term is (row, coefficient bits, variable), a pmt_linear_term is (coefficient bits, variable)."""
import ctypes as C
import functools

import numpy as np

DENORMAL = 5e-324 * 3
NAN_PAYLOAD = np.array([0x7FF8DEAD0000BEEF], dtype=np.uint64).view(np.float64)[0]     # quiet, with a payload that is not the default's
SPECIALS = [0.0, -0.0, DENORMAL, float("inf"), -float("inf"), -DENORMAL, -0.375, 0.625]

SB_RB, SB_CAP, SB_MAXCW = 128, 7168, 1024            # csrc/sparse.hip: rows per block, coefficients of a block, widest band
FLAT_GRID = 2048 * 256                               # threads of the flat kernels' capped grid
VAT_FIELDS, LT_FIELDS = ("row", "coeff", "var"), ("coeff", "var")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def values(n, seed, nan=True, zeros=True):
    """n doubles of both signs in [-0.5, 0.5) with the specials planted where n allows: +0.0, -0.0, denormals of both signs, both infinities
    and (nan=True) a NaN with a payload.  zeros=False leaves both zeros, the infinities and the NaN out (what the oracle comparison can
    carry: it drops coeff == 0.0).  A vector shorter than the list takes the specials from position `seed` on."""
    a = np.random.default_rng(seed).random(n) - 0.5
    a[a == 0.0] = 0.25
    sp = list(SPECIALS) + ([NAN_PAYLOAD] if nan else [])
    if not zeros:
        sp = [DENORMAL, -DENORMAL, -0.375, 0.625]
    if n >= 2 * len(sp):
        for k, s in enumerate(sp):
            a[(k * n) // len(sp) + 1] = s
    else:
        for k in range(n):
            a[k] = sp[(seed + k) % len(sp)]
    return a


def column_variables(n, seed):
    """x[col]: the columns' variables in no particular order, 4 .. n + 3"""
    return np.random.default_rng(seed).permutation(np.arange(1, n + 1)).astype(np.int64) + 3


def permuting_varmap(n, seed):
    """the optimizer's index of model variable v at varmap[v - 1], v in 1 .. n + 3"""
    return np.random.default_rng(seed).permutation(np.arange(1, n + 4)).astype(np.int64) + 100


# ---- the restatement
def restate(m, n, colptr, rowval, nzval, xvar, varmap, row_offset, d, sign):
    """-> (VAT words (3 nnz), LT words (2 nnz), constants' words (m)), all int64.  Row by row, ascending column within a row."""
    colptr, rowval = [int(v) for v in colptr], [int(v) for v in rowval]
    coeff = [int(v) for v in bits(nzval)] if len(rowval) else []
    xvar = [int(v) for v in xvar]
    vmap = None if varmap is None else [int(v) for v in varmap]
    per_row = [[] for _ in range(m)]
    for col in range(n):                                             # ascending column => ascending column within every row
        for p in range(colptr[col] - 1, colptr[col + 1] - 1):
            per_row[rowval[p] - 1].append((coeff[p], xvar[col]))
    vat, lt = [], []
    for row in range(m):
        for c, v in per_row[row]:
            vat += [row_offset + row + 1, c, v if vmap is None else vmap[v - 1]]
            lt += [c, v]                                             # the native term keeps the model's variable: never mapped
    return np.array(vat, dtype=np.int64), np.array(lt, dtype=np.int64), constants(m, d, sign)


def constants(m, d, sign):
    """0.0 - d, 0.0 + d (src/functions.jl:751-764 into a zeroed constant), or +0.0 without a vector"""
    if d is None or sign == 0:
        return np.zeros(m, dtype=np.int64)
    zero = np.float64(0.0)
    out = np.empty(m, dtype=np.float64)
    for i in range(m):
        out[i] = zero - np.float64(d[i]) if sign < 0 else zero + np.float64(d[i])
    return bits(out).copy()


# ---- deliberately wrong restatements (tests/test_sparse_assemble_host.py shows that each is rejected)
def wrong_column_major(m, n, colptr, rowval, nzval, xvar, varmap, row_offset, d, sign):
    """the terms in the order of the CSC storage"""
    cb = bits(nzval)
    vat, lt = [], []
    for col in range(n):
        for p in range(int(colptr[col]) - 1, int(colptr[col + 1]) - 1):
            v = int(xvar[col])
            vat += [row_offset + int(rowval[p]), int(cb[p]), v if varmap is None else int(varmap[v - 1])]
            lt += [int(cb[p]), v]
    return np.array(vat, dtype=np.int64), np.array(lt, dtype=np.int64), constants(m, d, sign)


def wrong_lt_mapped(*args):
    """the optimizer's index map applied to the native terms too"""
    vat, lt, c = restate(*args)
    lt = lt.copy()
    lt[1::2] = vat[2::3]
    return vat, lt, c


def wrong_d_minus_zero(*args):
    """(+|-d) - 0.0 in place of 0.0 (+|-) d: the sign of a zero constant"""
    vat, lt, _ = restate(*args)
    m, d, sign = args[0], args[8], args[9]
    if d is None or sign == 0:
        return vat, lt, np.zeros(m, dtype=np.int64)
    d = np.asarray(d, dtype=np.float64)
    return vat, lt, bits((-d if sign < 0 else d) - np.float64(0.0)).copy()


def wrong_row_offset(*args):
    """0-based rows under the offset"""
    vat, lt, c = restate(*args)
    vat = vat.copy()
    vat[0::3] -= 1
    return vat, lt, c


# ---- patterns
class Pattern:
    def __init__(self, name, mask):
        mask = np.asarray(mask, dtype=bool)
        self.name, (self.m, self.n) = name, mask.shape
        cols, rows = np.nonzero(mask.T)                              # column after column, rows ascending within a column
        self.colptr = np.concatenate(([1], 1 + np.cumsum(mask.sum(axis=0)))).astype(np.int64)
        self.rowval = (rows + 1).astype(np.int64)
        self.nnz = int(len(rows))
        self.mask = mask

    def __repr__(self):
        return self.name

    def dense(self, nzval):
        """the matrix with nzval at the structural non-zeros (for the oracle's dense builders)"""
        A = np.zeros((self.m, self.n))
        cols = np.repeat(np.arange(self.n), np.diff(self.colptr))
        A[self.rowval - 1, cols] = nzval
        return A


def _first_columns(m, n, lengths):
    mask = np.zeros((m, n), dtype=bool)
    for r, L in enumerate(lengths):
        mask[r, :L] = True
    return mask


STAIRCASE_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 300)
COLUMN_RUN_LENGTHS = (0, 1, 2, 3, 15, 16, 17, 18, 19, 24, 25, 127, 128, 5, 1)
RAGGED_LENGTHS = (129, 0, 1, 65, 63, 64, 2, 130)


def _staircase():
    mask = _first_columns(12, 1027, STAIRCASE_LENGTHS)
    mask[3, 1024:] = mask[5, 1024:] = True
    return Pattern("staircase", mask)


def _column_runs():
    mask = _first_columns(15, 131, COLUMN_RUN_LENGTHS).T.copy()
    mask[128, 3] = mask[129, 7] = mask[130, 14] = True               # the last one is the pattern's last entry: a run starting at nnz - 1
    return Pattern("column_runs", mask)


def _holes():
    rng = np.random.default_rng(17)
    mask = rng.random((260, 70)) < 0.12
    mask[128:256] = False                                            # a whole row block
    mask[0] = mask[259] = False
    mask[:, [0, 5, 33, 69]] = False
    return Pattern("holes", mask)


def _random(name, m, n, density, seed):
    return Pattern(name, np.random.default_rng(seed).random((m, n)) < density)


def _ragged(rows):
    """rows of RAGGED_LENGTHS leading columns: the first group of four rows is (129, 0, 1, 65)"""
    return Pattern("ragged%d" % rows, _first_columns(rows, 140, [RAGGED_LENGTHS[r % len(RAGGED_LENGTHS)] for r in range(rows)]))


def _five_columns():
    mask = np.ones((6, 5), dtype=bool)
    mask[1, 1:4] = mask[4] = False
    return Pattern("five_columns", mask)


def _flat_long():
    """FLAT_GRID + 3 terms: 1024 rows of 512 consecutive columns each, three rows with one more"""
    mask = np.zeros((1024, 600), dtype=bool)
    for r in range(1024):
        mask[r, r % 64:r % 64 + 512 + (1 if r in (0, 500, 1023) else 0)] = True
    return Pattern("flat_long", mask)


_MAKERS = {
    "staircase": _staircase,
    "column_runs": _column_runs,
    "capacity": lambda: Pattern("capacity", np.ones((128, 56), dtype=bool)),
    "over_capacity": lambda: Pattern("over_capacity", np.ones((128, 57), dtype=bool)),
    "nine_bands": lambda: Pattern("nine_bands", np.ones((130, 257), dtype=bool)),
    "holes": _holes,
    "single": lambda: Pattern("single", np.ones((1, 1), dtype=bool)),
    "random_half": lambda: _random("random_half", 300, 300, 0.5, 1),
    "random_tenth": lambda: _random("random_tenth", 200, 500, 0.1, 2),
    "random_quarter": lambda: _random("random_quarter", 257, 300, 0.25, 3),
    "ragged1": lambda: _ragged(1), "ragged15": lambda: _ragged(15), "ragged16": lambda: _ragged(16), "ragged17": lambda: _ragged(17),
    "ragged33": lambda: _ragged(33),
    "five_columns": _five_columns,
    "flat_long": _flat_long,
}
NAMED = ("staircase", "column_runs", "capacity", "over_capacity", "nine_bands", "holes", "single", "random_half", "random_tenth", "random_quarter")
SLAB_MADE = ("ragged1", "ragged15", "ragged16", "ragged17", "ragged33", "five_columns")
SLAB_CASES = ([("staircase", s) for s in (1, 3, 8, 64)] + [("column_runs", 8), ("capacity", 3), ("over_capacity", 64), ("nine_bands", 3), ("holes", 8),
              ("single", 1), ("single", 64), ("random_half", 8), ("random_tenth", 3), ("random_quarter", 64)]
              + [("ragged1", 1), ("ragged15", 3), ("ragged16", 1), ("ragged17", 8), ("ragged33", 1), ("ragged33", 3), ("five_columns", 8)])
SMALL_FOR_THE_ORACLE = ("single", "five_columns", "column_runs", "holes", "ragged17")


@functools.lru_cache(maxsize=None)
def pattern(name):
    return _MAKERS[name]()


# ---- the library's static tables of a pattern (host functions of csrc/sparse.hip; no GPU)
_vp = lambda a: a.ctypes.data_as(C.c_void_p)


class Tables:
    """perm / trow / tcol / rptr of pmt_sparse_rowmajor_order and, where the block form applies (cw > 0), desc / idx / band of
    pmt_sparse_blocks_build"""

    def __init__(self, pat):
        from parametron_jl_amd import _lib
        m, n, nnz = pat.m, pat.n, pat.nnz
        self.pat = pat
        self.perm, self.trow, self.tcol = (np.zeros(max(nnz, 1), dtype=np.int64) for _ in range(3))
        self.rptr = np.zeros(m + 1, dtype=np.int64)
        _lib.call("pmt_sparse_rowmajor_order", m, n, _vp(pat.colptr), _vp(pat.rowval), _vp(self.perm), _vp(self.trow), _vp(self.tcol), _vp(self.rptr))
        cw = C.c_int(-1)
        _lib.call("pmt_sparse_blocks_width", m, n, _vp(pat.colptr), _vp(pat.rowval), C.byref(cw))
        self.cw = cw.value
        if self.cw > 0:
            self.nrb, self.ncb = -(-m // SB_RB), -(-n // self.cw)
            self.desc, self.idx = np.zeros(self.nrb * n, dtype=np.uint64), np.zeros(max(nnz, 1), dtype=np.uint32)
            self.band = np.zeros(m * (self.ncb + 1), dtype=np.int64)
            _lib.call("pmt_sparse_blocks_build", m, n, _vp(pat.colptr), _vp(pat.rowval), _vp(self.perm), _vp(self.tcol), _vp(self.rptr), self.cw,
                      _vp(self.desc), _vp(self.idx), _vp(self.band))

    def slab_ptr(self, nslab):
        from parametron_jl_amd import _lib
        out = np.zeros(max(self.pat.m * (nslab + 1), 1), dtype=np.int64)
        _lib.call("pmt_sparse_slab_ptr", self.pat.m, self.pat.n, nslab, _vp(self.rptr), _vp(self.tcol), _vp(out))
        return out

    def term_var(self, xvar):
        return xvar[self.tcol[:self.pat.nnz] - 1] if self.pat.nnz else np.ones(1, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def tables(name):
    return Tables(pattern(name))


# ---- which branch edges of the kernels a pattern reaches, computed from the tables the kernels read
def _run_parities(starts, lengths, W):
    """{(W, lead, trailing single word)} over the non-empty runs of 64 terms at most that a wave writes, for both destination bases"""
    out = set()
    for ts, L in zip(starts, lengths):
        for base in range(0, int(L), 64):
            cnt = min(64, int(L) - base)
            for shift in (0, 1):
                lead = (shift + (int(ts) + base) * W) & 1
                out.add((W, lead, (lead + cnt * W) & 1))
    return out


def block_edges(t):
    """the edges of sparse_block_kernel that the pattern of Tables `t` reaches"""
    pat, n, nnz = t.pat, t.pat.n, t.pat.nnz
    p0 = (t.desc & np.uint64(0xffffffff)).astype(np.int64).reshape(t.nrb, n)
    ln = ((t.desc >> np.uint64(32)) & np.uint64(0xffff)).astype(np.int64).reshape(t.nrb, n)
    band = t.band.reshape(pat.m, t.ncb + 1)
    runs = np.diff(band, axis=1)                                     # (row, band): terms of the row inside the band
    fill = np.zeros((t.nrb, t.ncb), dtype=np.int64)                  # coefficients of a block
    for cb in range(t.ncb):
        fill[:, cb] = ln[:, cb * t.cw:(cb + 1) * t.cw].sum(axis=1)
    pair_at_end = False                                              # a two-coefficient load whose first one is the last of nzval
    for rb, c in zip(*np.nonzero(ln)):
        first = p0[rb, c] + 2 * np.arange(8)
        pair_at_end |= bool(np.any((2 * np.arange(8) < ln[rb, c]) & (first == nnz - 1)))
    parities = set()
    for W in (2, 3):
        parities |= _run_parities(band[:, :-1].reshape(-1), runs.reshape(-1), W)
    return {
        "cw": t.cw, "nrb": t.nrb, "ncb": t.ncb,
        "column_runs": set(int(v) for v in np.unique(ln)),
        "row_runs": set(int(v) for v in np.unique(runs)),
        "write_rounds": set(int(-(-v // 64)) for v in np.unique(runs)),
        "block_fill_max": int(fill.max()),
        "empty_block": bool(np.any(fill == 0)),
        "empty_row_block": bool(np.any(fill.sum(axis=1) == 0)),
        "empty_band": bool(np.any(fill.sum(axis=0) == 0)),
        "ragged_last_band": n % t.cw,
        "ragged_last_row_block": pat.m % SB_RB,
        "idle_workgroups": (-(-t.ncb // 8) * 8 - t.ncb) * t.nrb,
        "pair_load_at_the_last_coefficient": pair_at_end,
        "parities": parities,
    }


def slab_edges(t, nslab):
    """the edges of sparse_slab_kernel that the pattern of Tables `t` reaches with `nslab` column slabs"""
    m = t.pat.m
    sl = t.slab_ptr(nslab)[:m * (nslab + 1)].reshape(m, nslab + 1)
    seg = np.diff(sl, axis=1)
    padded = np.zeros((-(-m // 4) * 4, nslab), dtype=np.int64)
    padded[:m] = seg
    groups = padded.reshape(-1, 4, nslab)                            # the four rows of one wave
    distinct = np.array([[len(set(groups[g, :, s])) for s in range(nslab)] for g in range(groups.shape[0])])
    parities = set()
    for W in (2, 3):
        parities |= _run_parities(sl[:, :-1].reshape(-1), seg.reshape(-1), W)
    return {
        "nslab": nslab, "rows_mod_16": m % 16, "workgroups": -(-m // 16) * nslab,
        "segments": set(int(v) for v in np.unique(seg)),
        "rounds": set(int(-(-v // 64)) for v in np.unique(groups.max(axis=1))),
        "four_different_rows": bool(np.any(distinct == 4)),
        "empty_slab": bool(np.any(seg.sum(axis=0) == 0)),
        "more_slabs_than_columns": nslab > t.pat.n,
        "parities": parities,
    }


# ---- poisoned buffers
WORD = 0x5A5A000000000000                                            # a distinct word per position: WORD + position
GUARD = 16


class Poisoned:
    """The image of an output of `nwords` 8-byte words inside a larger buffer that holds WORD + position everywhere: GUARD words in front
    of it and behind it.  The buffer itself is 16-byte aligned; shift = 1 puts the output's first word at 8 mod 16."""

    def __init__(self, nwords, shift=0):
        self.n, self.off = int(nwords), GUARD + shift
        self.image = WORD + np.arange(self.off + self.n + GUARD + (1 - shift), dtype=np.int64)

    def expected(self, words):
        words = np.ascontiguousarray(words).reshape(-1).view(np.int64)
        assert len(words) <= self.n
        want = self.image.copy()
        want[self.off:self.off + len(words)] = words
        return want

    def check(self, got, words, fields, what=""):
        """the WHOLE buffer `got` against the poison overwritten by `words` (terms of `fields`); an AssertionError names the first difference"""
        want = self.expected(words)
        got = np.ascontiguousarray(got).view(np.int64)
        if got.shape == want.shape and np.array_equal(got, want):
            return
        assert got.shape == want.shape, (what, got.shape, want.shape)
        bad = np.flatnonzero(got != want)
        k = int(bad[0])
        q = k - self.off
        if q < 0:
            where = "front guard, %d words before the output" % -q
        elif q >= len(np.ascontiguousarray(words).reshape(-1)):
            where = "behind the output, word %d past its end" % (q - len(np.ascontiguousarray(words).reshape(-1)))
        else:
            where = "term %d, field %s (word %d)" % (q // len(fields), fields[q % len(fields)], q)
        raise AssertionError("%s: %d words differ, the first at %s: got %#018x, want %#018x"
                             % (what, len(bad), where, int(got[k]) % 2 ** 64, int(want[k]) % 2 ** 64))
