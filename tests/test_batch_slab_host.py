"""CPU suite: the numpy restatement of the batched-instance slab (tests/batch_util.py), which tests/test_gpu_batch_slabs.py compares the kernels
with bit for bit, against the oracle; five wrong restatements the same comparison tells apart; the exactness of the dyadic data at every shape
the GPU file uses; the case table against csrc/batch_small.hip; and the argument validation of the two entry points, which needs no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import batch_util as U
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def instance(n, r, m, seed):
    rng = np.random.default_rng(seed)
    At, b, Ct, d = U.batch_data(1, n, r, m, rng)
    return At[0].T.copy(), b[0], Ct[0].T.copy(), d[0]


def oracle_slab(A, b, Cm, d, sign_b, sign_d):
    """the slab from the reference's own steps: A*x (+|-) b, residual . residual, canonicalize!, the MOI copies; C*x (+|-) d"""
    r, n = A.shape
    m = Cm.shape[0]
    x = np.arange(1, n + 1, dtype=np.int64)
    res = O.AffVec(r).matvecmul_vars(A, x)
    if sign_b:
        res = O.AffVec(r).vecaddsub(res, b, sign_b < 0)
    obj = O.Quad().vecdot_affs_affs(res, res).canonicalize()
    at, qt, const = obj.moi()
    iu = np.triu_indices(n)
    assert np.array_equal(qt["row"], iu[0] + 1) and np.array_equal(qt["col"], iu[1] + 1)
    assert np.array_equal(at["var"], x)
    # without constants the reference's affine terms are the products 0.0 * a_ij, -0.0 where a lone a_ij is negative; the slab's contract
    # (include/parametron_hip.h) is +0.0 for sign 0, so the sign of that zero is all that is dropped — and nothing else: the values must be zeros
    q = at["coeff"] if sign_b else at["coeff"] + 0.0
    assert sign_b or not np.any(q)
    parts = [qt["coeff"], q, [const]]
    if m:
        con = O.AffVec(m).vecaddsub(O.AffVec(m).matvecmul_vars(Cm, x), d, sign_d < 0)
        ct, cc = con.moi()
        assert np.array_equal(ct["out"], np.repeat(np.arange(1, m + 1), n)) and np.array_equal(ct["var"], np.tile(x, m))
        parts += [ct["coeff"], cc]
    return np.concatenate([np.asarray(p, dtype=np.float64) for p in parts])


SHAPES = [(5, 3, 0), (5, 3, 1), (5, 3, 4), (17, 9, 0), (17, 9, 1), (17, 9, 4), (1, 1, 1), (3, 40, 2)]


@pytest.mark.parametrize("n,r,m", SHAPES)
def test_slab_reference_is_the_oracle_s_slab_bit_for_bit(n, r, m):
    A, b, Cm, d = instance(n, r, m, 100 * n + r + m)
    for sign_b in (-1, 0, 1):
        for sign_d in (-1, 1):
            got = U.slab_reference(A, b, Cm, d, sign_b, sign_d)
            assert len(got) == U.slab_doubles(n, m)
            assert same_bits(got, oracle_slab(A, b, Cm, d, sign_b, sign_d)), (sign_b, sign_d)
        # sign_d = 0: the constraint block without constants
        got = U.slab_reference(A, b, Cm, d, sign_b, 0)
        assert same_bits(got[U.sections(n, m)["d"]], np.zeros(m)) and same_bits(got[:U.sections(n, m)["d"].start], U.slab_reference(A, b, Cm, d, sign_b, 1)[:U.sections(n, m)["d"].start])


@pytest.mark.parametrize("n,r,m", [(5, 3, 4), (17, 9, 4)])
def test_slab_reference_is_lsq_workspace_s_slab_for_sign_minus(n, r, m):
    A, b, Cm, d = instance(n, r, m, 7 * n + m)
    x = np.arange(1, n + 1, dtype=np.int64)
    w = O.LsqWorkspace(n, r, m)
    w.eval_objective(np.ascontiguousarray(A.T).reshape(-1), b, x)
    w.eval_constraint(np.ascontiguousarray(Cm.T).reshape(-1), d, x)
    w.objective.canonicalize()
    at, qt, const = w.objective.moi()
    ct, cc = w.constraint.moi()
    want = np.concatenate([qt["coeff"], at["coeff"], [const], ct["coeff"], cc])
    assert same_bits(U.slab_reference(A, b, Cm, d, -1, -1), want)


def test_batch_restatement_is_the_per_instance_one():
    rng = np.random.default_rng(5)
    At, b, Ct, d = U.batch_data(4, 9, 6, 3, rng)
    got = U.slab_reference_batch(At, b, Ct, d, 1, -1)
    for i in range(4):
        assert same_bits(got[i], U.slab_reference(At[i].T, b[i], Ct[i].T, d[i], 1, -1))


def test_wrong_builders_are_told_apart():
    n, r, m = 5, 3, 4
    A, b, Cm, d = instance(n, r, m, 11)
    want = oracle_slab(A, b, Cm, d, -1, 1)
    sec = U.sections(n, m)
    right = U.slab_reference(A, b, Cm, d, -1, 1)
    assert same_bits(right, want)
    iu = np.triu_indices(n)

    undoubled = right.copy()                                                   # the diagonal of A'A taken once
    undoubled[sec["Q"]][iu[0] == iu[1]] *= 0.5
    colmajor = right.copy()                                                    # C left as it came in
    colmajor[sec["C"]] = np.ascontiguousarray(Cm.T).reshape(-1)
    sign_confused = U.slab_reference(A, b, Cm, d, -1, -1)                      # sign_b used for the d-consts
    q_flipped = right.copy()                                                   # q of A x + b
    q_flipped[sec["q"]] = U.slab_reference(A, b, Cm, d, 1, 1)[sec["q"]]
    lower = right.copy()                                                       # the triangle walked column by column
    G = 2.0 * (A.T @ A)
    lower[sec["Q"]] = G[np.tril_indices(n)]
    for name, wrong in (("undoubled diagonal", undoubled), ("column-major C", colmajor), ("sign_b for d", sign_confused), ("q sign", q_flipped),
                        ("column-wise triangle", lower)):
        assert not same_bits(wrong, want), name


def test_dyadic_data_is_what_it_says():
    a = U.dyadic((4000,), np.random.default_rng(1))
    bits = a.view(np.int64)
    assert np.any(bits == 0) and np.any(bits == np.int64(-2 ** 63)) and 0.03 < np.mean(a == 0) < 0.07
    assert np.any(a < 0) and np.any(a > 0) and np.max(np.abs(a)) <= 1023 * 16
    scaled = a * 16
    assert np.array_equal(scaled, np.round(scaled))
    m, e = np.frexp(a[a != 0])
    assert np.all(np.abs(a[a != 0]) >= 2.0 ** -4)
    assert len(np.unique(e)) >= 9


@pytest.mark.parametrize("n,r", U.gpu_shapes() + [(128, 1024)])
def test_dyadic_sums_are_exact_at_every_shape_the_gpu_file_uses(n, r):
    """Integer arithmetic on the values times 2^4 (products times 2^8) against float64 numpy: equal, and every partial sum — bounded by the sum
    of the absolute values — stays below 2^44, nine bits inside the mantissa"""
    rng = np.random.default_rng(1000 * n + r)
    At, b, _, _ = U.batch_data(1, n, r, 0, rng)
    At, b = At[0], b[0]
    Ai, bi = (At * 16).astype(np.int64), (b * 16).astype(np.int64)
    assert np.array_equal(Ai / 16.0, At) and np.array_equal(bi / 16.0, b)
    S, Sabs = Ai @ Ai.T, np.abs(Ai) @ np.abs(Ai).T                               # int64: exact, and below 2^47 by the bound in batch_util's docstring
    s, sabs = Ai.astype(object).dot((-bi).astype(object)), np.abs(Ai) @ np.abs(bi)      # q with Python integers throughout
    cc = [int(v) * int(v) for v in bi.tolist()]
    assert all(int(v) < 2 ** 44 for v in (2 * Sabs).reshape(-1).tolist() + (2 * sabs).tolist() + [sum(cc)])
    # Q: int64 is integer arithmetic too and holds 2^47; a sample of entries with Python integers checks the int64 products themselves
    for j, k in [(0, 0), (n - 1, n - 1), (0, n - 1), (n // 2, n // 3)] if n else []:
        assert int(S[j, k]) == sum(int(x) * int(y) for x, y in zip(Ai[j].tolist(), Ai[k].tolist()))
    slab = U.slab_reference(At.T, b, np.zeros((0, n)), np.zeros(0), -1, 0)
    sec = U.sections(n, 0)
    iu = np.triu_indices(n)
    assert np.array_equal(slab[sec["Q"]] * 256.0, (2 * S[iu]).astype(np.float64))
    assert np.array_equal(slab[sec["q"]] * 256.0, np.array([float(2 * v) for v in s], dtype=np.float64))
    assert slab[sec["const"]][0] * 256.0 == float(sum(cc))
    # summation order does not matter: the rows reversed
    rev = U.slab_reference(At.T[::-1], b[::-1], np.zeros((0, n)), np.zeros(0), -1, 0)
    assert same_bits(rev, slab)


def test_exact_integer_reference_on_full_mantissa_data():
    """as_scaled_ints / exact_gram / within_inner_product_bound (the position-independence test's reference): the integers restate the doubles
    exactly, numpy's own sums are inside the bound, and an entry off by a relative 1e-12 is outside"""
    rng = np.random.default_rng(3)
    n, r = 7, 31
    At, c = rng.random((n, r)) - 0.5, rng.random(r) - 0.5
    I, k = U.as_scaled_ints(At)
    assert all(float(i) * 2.0 ** k == v for i, v in zip(I.reshape(-1).tolist(), At.reshape(-1).tolist()))
    S, Sabs, s, sabs, k2 = U.exact_gram(At, c)
    G, g = 2.0 * (At @ At.T), 2.0 * (At @ c)
    assert U.within_inner_product_bound(G, S, Sabs, k2, r).all() and U.within_inner_product_bound(g, s, sabs, k2, r).all()
    assert not U.within_inner_product_bound(G * (1 + 1e-12), S, Sabs, k2, r).any()
    swapped = G.copy()
    swapped[0, 1], swapped[0, 2] = G[0, 2], G[0, 1]
    assert not U.within_inner_product_bound(swapped, S, Sabs, k2, r).all()


def test_case_table_matches_the_kernel_source():
    src = open(os.path.join(ROOT, "parametron.jl_amd", "csrc", "batch_small.hip")).read()
    for text in ("constexpr int STAGE_CAP = %d;" % U.STAGE_CAP, "constexpr int CREG = %d;" % U.CREG, "NS = %d;" % U.NS, "constexpr int CK = %d;" % U.CK,
                 "constexpr int SN = %d;" % U.SMALL_MAX_N,
                 "p.stage_all = (nq + cols + 1 + p.m * cols + p.m + 1 <= STAGE_CAP) ? 1 : 0;",
                 "p.Cm && p.stage_all && mn <= (int64_t)CREG * NS && m <= NS;"):
        assert text in src, "batch_small.hip no longer holds `%s`" % text
    host = open(os.path.join(ROOT, "parametron.jl_amd", "csrc", "batch.hip")).read()
    assert "n <= %d" % U.SMALL_MAX_N in host
    # wherever the register prefetch applies the whole slab is staged (the kernel asks for both)
    for n in range(1, U.SMALL_MAX_N + 1):
        for m in range(1, U.CREG * U.NS // n + 1):
            assert not U.takes_register_prefetch(n, m) or U.stages_whole_slab(n, m)
    # the chosen pairs lie on the intended side of each threshold
    st, pf = U.stages_whole_slab, U.takes_register_prefetch
    assert st(128, 16) and pf(128, 16) and not st(128, 17) and not pf(128, 17)
    assert st(64, 127) and not st(64, 128) and not pf(64, 127)
    assert pf(16, 128) and st(16, 128) and not pf(16, 129) and not pf(17, 128)
    assert st(8, 200) and not pf(8, 200) and 8 * 200 <= U.CREG * U.NS
    assert st(127, 17) and not pf(127, 17) and 127 * 17 > U.CREG * U.NS
    assert st(100, 5) and pf(100, 5) and pf(65, 2) and pf(2, 1) and not pf(128, 0) and st(1, 0) and U.slab_doubles(1, 0) == 3
    assert [U.chunks(r) for r in (0, 1, 32, 33, 70, 96, 224)] == [1, 1, 1, 2, 3, 3, 7]
    assert U.slab_doubles(128, 16) % 2 == 1 and U.slab_doubles(127, 17) % 2 == 0           # both parities for the placement test
    assert {n for n, _, _, _ in U.SMALL_CASES} <= set(range(1, U.SMALL_MAX_N + 1)) and all(c[0] > U.SMALL_MAX_N for c in U.GENERAL_CASES)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


def test_batch_argument_validation_needs_no_gpu(lib):
    p = C.c_void_p(64)                      # never dereferenced: each call is rejected, or returns, before any device call
    L = U.slab_doubles(4, 2)
    assert lib.load().pmt_batch_lsq_slab_doubles(4, 2) == L == 10 + 4 + 1 + 8 + 2
    for B, n, r, m in ((-1, 4, 3, 2), (1, -4, 3, 2), (1, 4, -3, 2), (1, 4, 3, -2)):
        with pytest.raises(lib.DimensionMismatch):
            lib.call("pmt_batch_lsq_coeffs_f64", p, p, p, p, B, n, r, m, -1, -1, p, 1 << 20, None)
    with pytest.raises(lib.DimensionMismatch, match="out_stride"):
        lib.call("pmt_batch_lsq_coeffs_f64", p, p, p, p, 1, 4, 3, 2, -1, -1, p, L - 1, None)
    for sb, sd in ((2, 0), (-2, 0), (0, 2), (0, -2)):
        with pytest.raises(lib.ArgumentError, match="sign"):
            lib.call("pmt_batch_lsq_coeffs_f64", p, p, p, p, 1, 4, 3, 2, sb, sd, p, L, None)
    for k in range(5):                                                  # A, b, C, d, out in turn
        a = [None if i == k else p for i in range(5)]
        with pytest.raises(lib.ArgumentError, match="null"):
            lib.call("pmt_batch_lsq_coeffs_f64", a[0], a[1], a[2], a[3], 1, 4, 3, 2, -1, -1, a[4], L, None)
    # an empty batch is complete as it stands, whatever the pointers
    lib.call("pmt_batch_lsq_coeffs_f64", None, None, None, None, 0, 4, 3, 2, -1, -1, None, L, None)
    # pmt_batch_expand_f64
    for n, m in ((-1, 2), (4, -2)):
        with pytest.raises(lib.DimensionMismatch):
            lib.call("pmt_batch_expand_f64", p, n, m, p, None, p, p, p, p, p, None)
    for k in range(7):                                                  # slab, xvar, out_quad, out_lin, out_const, out_vat, out_vconsts
        a = [None if i == k else p for i in range(7)]
        with pytest.raises(lib.ArgumentError, match="null"):
            lib.call("pmt_batch_expand_f64", a[0], 4, 2, a[1], None, a[2], a[3], a[4], a[5], a[6], None)
