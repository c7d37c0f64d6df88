"""CPU suite of the batched tracking-cost entry point (pmt_batch_form_coeffs_f64): the numpy restatement of its slab (tests/batch_form_util.py),
which tests/test_gpu_batch_form.py compares the kernel with bit for bit, against the oracle's literal composition per instance; the same
restatement against Python integers on data whose every sum is exact; wrong restatements the comparison tells apart; and the entry point's
argument validation and edge cases, which need no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import batch_form_util as F
import batch_util as BU
import quad_form_shift_util as SU
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pmt_batch_form_coeffs_f64"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- 1. the restatement against the oracle, instance by instance

@pytest.mark.parametrize("n", [1, 5, 64, 65, 130, 256])
def test_restatement_equals_the_oracle_composition_per_instance(n):
    """Q section bit for bit (each entry the sum of two numbers); q and const within the sum of the node's and the oracle's own rounding bounds
    (quad_form_shift_util: nothing tuned); the constraint block and its constants bit for bit (C*x (+|-) d through the oracle's builders)"""
    B, m = 2, 3
    rng = np.random.default_rng(50 + n)
    Qt, p, Ct, d = F.form_data(B, n, m, rng)
    x = np.arange(1, n + 1, dtype=np.int64)
    sec = BU.sections(n, m)
    iu = np.triu_indices(n)
    for sign_p, sign_d in ((-1, 1), (1, -1)):
        got = F.form_slab_reference(Qt, p, Ct, d, sign_p, sign_d)
        assert got.shape == (B, BU.slab_doubles(n, m))
        for i in range(B):
            Q = Qt[i].T
            at, qt, const = SU.oracle_tracking(Q, x, p[i], sign_p)
            assert np.array_equal(qt["row"], iu[0] + 1) and np.array_equal(qt["col"], iu[1] + 1) and np.array_equal(at["var"], x)
            assert np.array_equal(bits(got[i, sec["Q"]]), bits(qt["coeff"]))
            bound = SU.node_lin_bound(Q, p[i], sign_p) + SU.oracle_lin_bound(Q, p[i], sign_p)
            err = np.abs(got[i, sec["q"]] - at["coeff"])
            assert np.all(err <= bound), np.max(err / np.maximum(bound, 1e-300))
            assert abs(got[i, sec["const"]][0] - const) <= SU.node_const_bound(Q, p[i], sign_p) + SU.oracle_const_bound(Q, p[i], sign_p)
            if n >= 64:                                                 # the bound is not vacuous
                assert np.max(bound) < 1e-9 * np.max(np.abs(got[i, sec["q"]]))
            con = O.AffVec(m).vecaddsub(O.AffVec(m).matvecmul_vars(np.ascontiguousarray(Ct[i].T), x), d[i], sign_d < 0)
            ct, cc = con.moi()
            assert np.array_equal(bits(got[i, sec["C"]]), bits(ct["coeff"])) and np.array_equal(bits(got[i, sec["d"]]), bits(cc))


def test_plain_form_and_signs_of_the_restatement():
    """sign_p == 0: q and const are +0.0 and p is not read; the Q section, C and the d-consts do not depend on sign_p; sign_d == 0: +0.0"""
    B, n, m = 3, 70, 4
    Qt, p, Ct, d = F.form_data(B, n, m, np.random.default_rng(4))
    sec = BU.sections(n, m)
    plain = F.form_slab_reference(Qt, None, Ct, d, 0, 1)
    minus = F.form_slab_reference(Qt, p, Ct, d, -1, 1)
    plus = F.form_slab_reference(Qt, p, Ct, d, 1, 0)
    zero = bits(np.zeros(1))[0]
    assert np.all(bits(plain[:, sec["q"]]) == zero) and np.all(bits(plain[:, sec["const"]]) == zero)
    for other in (minus, plus):
        assert np.array_equal(bits(plain[:, sec["Q"]]), bits(other[:, sec["Q"]])) and np.array_equal(bits(plain[:, sec["C"]]), bits(other[:, sec["C"]]))
    assert np.array_equal(bits(minus[:, sec["d"]]), bits(0.0 + d)) and np.all(bits(plus[:, sec["d"]]) == zero)
    # c -> -c: lin changes its sign exactly (every product does), the constant does not change
    assert np.array_equal(bits(plus[:, sec["q"]]), bits(-minus[:, sec["q"]])) and np.array_equal(bits(plus[:, sec["const"]]), bits(minus[:, sec["const"]]))
    # no variables: [+0.0 | d-consts]
    none = F.form_slab_reference(np.zeros((2, 0, 0)), np.zeros((2, 0)), np.zeros((2, 0, 3)), d[:2, :3], -1, -1)
    assert none.shape == (2, 4) and np.all(bits(none[:, 0]) == zero) and np.array_equal(bits(none[:, 1:]), bits(0.0 - d[:2, :3]))


def test_wrong_restatements_are_told_apart():
    B, n, m = 1, 70, 2
    Qt, p, Ct, d = F.form_data(B, n, m, np.random.default_rng(8))
    right = F.form_slab_reference(Qt, p, Ct, d, -1, -1)[0]
    sec = BU.sections(n, m)
    iu = np.triu_indices(n)
    Q = Qt[0].T
    undoubled = right.copy()
    undoubled[sec["Q"]][iu[0] == iu[1]] *= 0.5
    lower = right.copy()
    lower[sec["Q"]] = SU.symmetrised(Q)[np.tril_indices(n)]
    one_chain = right.copy()                                                   # lin as one chain over all n columns, not block by block
    S, c = SU.symmetrised(Q), SU.shift_consts(p[0], -1)
    acc = S[:, 0] * c[0]
    for k in range(1, n):
        acc = acc + S[:, k] * c[k]
    one_chain[sec["q"]] = acc
    unsym = right.copy()                                                       # Q*c, the matrix taken as symmetric
    unsym[sec["q"]] = 2.0 * (Q @ c)
    left_to_right = right.copy()                                               # the constant as a plain chain
    t = 0.0
    for j in range(n):
        t = t + c[j] * right[sec["q"]][j]
    left_to_right[sec["const"]] = 0.5 * t
    other_sign = F.form_slab_reference(Qt, p, Ct, d, 1, -1)[0]
    colmajor = right.copy()
    colmajor[sec["C"]] = Ct[0].reshape(-1)
    for name, wrong in (("undoubled diagonal", undoubled), ("column-wise triangle", lower), ("one chain", one_chain), ("Q taken as symmetric", unsym),
                        ("sequential constant", left_to_right), ("sign of p", other_sign), ("column-major C", colmajor)):
        assert not np.array_equal(bits(wrong), bits(right)), name


# ---- 2. exact data

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 200, 256])
def test_restatement_is_exact_on_coarse_dyadic_data(n):
    """Coarse dyadic data (batch_form_util): multiples of 8 below 2^14.  In units of 8, 64 and 512 every S is an integer below 2^12, every
    product S*c below 2^23, every partial sum of a lin_j (at most 256 products) below 2^31, every product c_j*lin_j below 2^42 and every
    partial sum of T below 2^50 — all inside the 53-bit mantissa, so the restatement's Q, q and const equal the Python-integer values bit for
    bit, in every order.  The sums of absolute values, which bound every partial sum, are asserted to stay below 2^50 units.  Zeros are compared
    after + 0.0 (a chain of lin_j starts from its first product and may keep a -0.0; integers know no signed zero)."""
    B, m = 3, 2
    rng = np.random.default_rng(900 + n)
    Qt, p, Ct, d = F.form_data(B, n, m, rng, gen=F.coarse_dyadic)
    assert all(np.array_equal(a, 8 * np.round(a / 8)) and np.max(np.abs(a)) <= 16368 for a in (Qt, p)) and (n < 63 or np.any(bits(Qt) == bits(-0.0)[0]))
    sec = BU.sections(n, m)
    for sign_p in (-1, 1):
        got = F.form_slab_reference(Qt, p, Ct, d, sign_p, -1)
        for i in range(B):
            S, lin, T, mag_lin, mag_T, k = F.exact_form(Qt[i].T, p[i], sign_p)
            # as_scaled_ints keeps full 53-bit mantissas: k < 0, the units of 8, 64 and 512 are 2^(3-k), 2^(6-2k) and 2^(9-3k) of its integers
            assert k <= 0 and all(int(v) < 2 ** (31 + 6 - 2 * k) for v in mag_lin.tolist()) and mag_T < 2 ** (50 + 9 - 3 * k)
            want_Q = np.array([float(int(v)) for v in S.tolist()]) * 2.0 ** k
            want_q = np.array([float(int(v)) for v in lin.tolist()]) * 2.0 ** (2 * k)
            want_c = 0.5 * (float(T) * 2.0 ** (3 * k))
            assert np.array_equal(bits(got[i, sec["Q"]] + 0.0), bits(want_Q + 0.0))
            assert np.array_equal(bits(got[i, sec["q"]] + 0.0), bits(want_q + 0.0))
            assert bits(got[i, sec["const"]])[0] == bits([want_c + 0.0])[0]
    # the order does not matter on such data: the variables reversed give the same constant and the reversed q
    rev = F.form_slab_reference(np.ascontiguousarray(Qt[:, ::-1, ::-1]), np.ascontiguousarray(p[:, ::-1]), Ct, d, -1, -1)
    fwd = F.form_slab_reference(Qt, p, Ct, d, -1, -1)
    assert np.array_equal(bits(rev[:, sec["q"]] + 0.0), bits(fwd[:, sec["q"]][:, ::-1] + 0.0)) and np.array_equal(bits(rev[:, sec["const"]]), bits(fwd[:, sec["const"]]))


def test_coarse_truncates_towards_zero_and_keeps_the_sign_of_zero():
    v = F.coarse(np.array([16368.0, -16368.0, 9.5, -9.5, 7.9375, -7.9375, 0.0, -0.0, 8.0, -8.0]))
    assert v.tolist() == [16368.0, -16368.0, 8.0, -8.0, 0.0, -0.0, 0.0, -0.0, 8.0, -8.0]
    assert np.signbit(v).tolist() == [False, True, False, True, False, True, False, True, False, True]


# ---- 3. the entry point without a device

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


P = C.c_void_p(64)                          # never dereferenced: each call is rejected, or returns, before any device call


def _call(lib, Q=P, p=P, Cm=P, d=P, B=1, n=4, m=2, sign_p=-1, sign_d=-1, out=P, stride=None):
    lib.call(NAME, Q, p, Cm, d, B, n, m, sign_p, sign_d, out, BU.slab_doubles(max(n, 0), max(m, 0)) if stride is None else stride, None)


def test_entry_point_is_declared_bound_and_exported(lib):
    raw = C.CDLL(lib.LIB_PATH)
    assert hasattr(raw, NAME) and len(lib.SIGNATURES[NAME][1]) == 12
    assert len(lib.SIGNATURES["pmt_batch_lsq_coeffs_f64"][1]) == 13                # the least-squares batch keeps its signature


@pytest.mark.parametrize("bad", [{"B": -1}, {"n": -4, "stride": 1 << 20}, {"m": -2, "stride": 1 << 20}, {"n": F.MAX_N + 1, "m": 0}, {"n": 1 << 40, "m": 0, "stride": 1 << 62},
                                 {"stride": BU.slab_doubles(4, 2) - 1}, {"stride": 0}, {"stride": -5}],
                         ids=["B-negative", "n-negative", "m-negative", "n-257", "n-huge", "stride-L-1", "stride-zero", "stride-negative"])
def test_dimension_errors_come_before_any_device_call(lib, bad):
    with pytest.raises(lib.DimensionMismatch, match="batch_form"):
        _call(lib, **bad)
    # .. and before the empty batch's return: B == 0 does not excuse them
    if "B" not in bad:
        with pytest.raises(lib.DimensionMismatch, match="batch_form"):
            _call(lib, B=0, **bad)


@pytest.mark.parametrize("sign_p,sign_d", [(2, 0), (-2, 0), (0, 2), (0, -2), (7, 7)])
def test_signs_outside_minus_one_zero_one_are_argument_errors(lib, sign_p, sign_d):
    with pytest.raises(lib.ArgumentError, match="sign"):
        _call(lib, sign_p=sign_p, sign_d=sign_d)
    # the dimension checks come first
    with pytest.raises(lib.DimensionMismatch):
        _call(lib, sign_p=sign_p, sign_d=sign_d, stride=3)


@pytest.mark.parametrize("null", ["Q", "p", "Cm", "d", "out"])
def test_null_pointers_where_data_is_needed(lib, null):
    with pytest.raises(lib.ArgumentError, match="null"):
        _call(lib, **{null: None})


def test_null_pointers_where_no_data_is_read_and_empty_batches(lib):
    """What these calls would launch needs a GPU: on a machine without one a launch is a HIP error, with one the dummy pointers would be read —
    each must be rejected for the pointer that IS needed, or return PMT_OK without a launch"""
    # sign_p == 0: p may be NULL; the call then gets as far as the next missing pointer
    with pytest.raises(lib.ArgumentError, match="null"):
        _call(lib, p=None, sign_p=0, out=None)
    # m == 0: C and d are not needed; n == 0: Q, p and C are not needed
    with pytest.raises(lib.ArgumentError, match="null"):
        _call(lib, Cm=None, d=None, m=0, out=None)
    with pytest.raises(lib.ArgumentError, match="null"):
        _call(lib, Q=None, p=None, Cm=None, n=0, d=None)
    with pytest.raises(lib.ArgumentError, match="null"):
        _call(lib, Q=None, p=None, Cm=None, n=0, out=None)
    # sign_d == 0 still needs d, as the least-squares batch does
    with pytest.raises(lib.ArgumentError, match="null"):
        _call(lib, d=None, sign_d=0)
    # an empty batch is complete as it stands, whatever the pointers: PMT_OK, nothing launched
    for n, m in ((4, 2), (0, 0), (0, 3), (5, 0), (F.MAX_N, 1)):
        lib.call(NAME, None, None, None, None, 0, n, m, -1, 1, None, BU.slab_doubles(n, m), None)
        lib.call(NAME, None, None, None, None, 0, n, m, 0, 0, None, BU.slab_doubles(n, m) + 3, None)


def test_slab_length_is_the_least_squares_batch_s(lib):
    for n, m in ((0, 0), (0, 3), (1, 0), (128, 16), (256, 70)):
        assert lib.load().pmt_batch_lsq_slab_doubles(n, m) == BU.slab_doubles(n, m)
    assert BU.slab_doubles(0, 0) == 1 and BU.slab_doubles(0, 3) == 4


def test_header_bound_is_the_source_s():
    hdr = open(os.path.join(ROOT, "include", "parametron_hip.h")).read()
    src = open(os.path.join(ROOT, "parametron.jl_amd", "csrc", "batch_form.hip")).read()
    m = re.search(r"^#define PMT_BATCH_FORM_MAX_N (\d+)$", hdr, re.M)
    k = re.search(r"^constexpr int BF_MAX_N = (\d+);$", src, re.M)
    assert m and k and int(m.group(1)) == int(k.group(1)) == F.MAX_N == 256
    assert "static_assert(BF_MAX_N == PMT_BATCH_FORM_MAX_N" in src
    # the chains of a tile are 64 long, the tree 256 wide: the header's order for the shifted form
    assert re.search(r"^constexpr int BF_TILE = 64;$", src, re.M) and re.search(r"^constexpr int BF_THREADS = 256;$", src, re.M) and SU.TILE == 64
