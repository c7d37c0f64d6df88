"""CPU suite of the batched MPC horizons (pmt_batch_horizon_coeffs_f64, pmt_batch_horizon_expand_f64, batch.horizon_slab_layout): the numpy
restatement of the slab (tests/batch_horizon_util.py), which tests/test_gpu_batch_horizon.py compares the kernel with bit for bit, against
the oracle's literal composition per instance — every stage's dot(e, Q*e) sequence, added in z order, canonicalize!, the MOI copy
(quad_stages_util.oracle) —, against Python integers on data whose every sum is exact, and against quad_stages_util's restatement of
pmt_quad_stages_f64 for the instance's table; the slab length against the layout; and the argument validation of both device entry points,
which needs no GPU."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import batch_form_util as F
import batch_horizon_util as H
import quad_stages_util as QU
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COEFFS, EXPAND, DOUBLES = "pmt_batch_horizon_coeffs_f64", "pmt_batch_horizon_expand_f64", "pmt_batch_horizon_slab_doubles"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


def z_vars(n, rng, extra=7):
    """n strictly increasing model variables among n + extra, and a permuting, offset varmap"""
    xvar = np.sort(rng.choice(np.arange(1, n + extra + 1), n, replace=False)).astype(np.int64)
    return xvar, (rng.permutation(n + extra) + 1 + 100).astype(np.int64)


# ---- 1. the slab length and the layout

GRID = [(T, nx, nu, m) for T in (1, 2, 7, 512) for nx in (1, 3, 64, 65, 128) for nu in (0, 1, 64, 128) for m in (0, 1, 5, 33)]


def test_slab_length_equals_the_layout_over_a_grid(lib):
    from parametron_jl_amd import batch as PB
    fn = lib.load().pmt_batch_horizon_slab_doubles
    for T, nx, nu, m in GRID:
        off, L = PB.horizon_slab_layout(T, nx, nu, m)
        n = T * (nx + nu)
        assert fn(T, nx, nu, m) == L == H.slab_doubles(T, nx, nu, m)
        sec = H.sections(T, nx, nu, m)
        assert [off[k] for k in ("SQ", "SR", "q", "const", "C", "dconst")] == [sec[k].start for k in ("SQ", "SR", "q", "const", "C", "d")]
        assert sec["d"].stop == L and sec["q"].stop - sec["q"].start == n and sec["C"].stop - sec["C"].start == m * n
        assert (off["SR"] == off["q"]) == (nu == 0) and (off["C"] == off["dconst"] == L) == (m == 0)
    assert PB.horizon_slab_layout(1, 1, 0, 0)[1] == 3                    # [SQ: 1 | q: 1 | const]
    # a horizon of one stage without inputs is the tracking cost's slab
    assert PB.horizon_slab_layout(1, 40, 0, 6) == ({k2: PB.slab_layout(40, 6)[0][k1] for k1, k2 in
                                                     (("Q", "SQ"), ("q", "SR"), ("q", "q"), ("const", "const"), ("C", "C"), ("dconst", "dconst"))},
                                                    PB.slab_layout(40, 6)[1])


def test_entry_points_are_declared_bound_and_exported(lib):
    raw = C.CDLL(lib.LIB_PATH)
    for name, nargs in ((DOUBLES, 4), (COEFFS, 17), (EXPAND, 13)):
        assert hasattr(raw, name) and len(lib.SIGNATURES[name][1]) == nargs
    assert len(lib.SIGNATURES["pmt_batch_form_coeffs_f64"][1]) == 12 and len(lib.SIGNATURES["pmt_batch_expand_f64"][1]) == 11        # the siblings keep theirs


def test_header_bounds_are_the_source_s():
    hdr = open(os.path.join(ROOT, "include", "parametron_hip.h")).read()
    src = open(os.path.join(ROOT, "parametron.jl_amd", "csrc", "batch_horizon.hip")).read()
    d = re.search(r"^#define PMT_BATCH_HORIZON_MAX_DIM (\d+)", hdr, re.M)
    t = re.search(r"^#define PMT_BATCH_HORIZON_MAX_T +(\d+)", hdr, re.M)
    kd = re.search(r"^constexpr int BH_MAX_DIM = (\d+);$", src, re.M)
    kt = re.search(r"^constexpr int BH_MAX_T = (\d+);$", src, re.M)
    assert int(d.group(1)) == int(kd.group(1)) == H.MAX_DIM == 128 and int(t.group(1)) == int(kt.group(1)) == H.MAX_T == 512
    assert "static_assert(BH_MAX_DIM == PMT_BATCH_HORIZON_MAX_DIM && BH_MAX_T == PMT_BATCH_HORIZON_MAX_T" in src
    assert re.search(r"^constexpr int BH_TILE = 64;$", src, re.M) and re.search(r"^constexpr int BH_THREADS = 256;$", src, re.M)


# ---- 2. the restatement against the oracle's literal composition, instance by instance

@pytest.mark.parametrize("T,nx,nu", [(1, 1, 0), (3, 5, 2), (2, 64, 1), (2, 65, 10), (3, 10, 65), (2, 128, 33), (4, 7, 0)])
def test_restatement_equals_the_oracle_composition_per_instance(T, nx, nu):
    """quadratic coefficients bit for bit (each the sum of two numbers) at the oracle's indices; every linear coefficient and the constant
    within the bounds quad_stages_util derives for a stage and for the sum of the stage constants (nothing tuned; a plain stage has no linear
    term in the oracle and +0.0 in the slab); the constraint block and its constants bit for bit"""
    B, m = 2, 3
    rng = np.random.default_rng(70 + 100 * nx + nu)
    Qt, Rt, r, v, Ct, d = H.horizon_data(B, T, nx, nu, m, rng)
    n = T * (nx + nu)
    xvar, varmap = z_vars(n, rng)
    sec = H.sections(T, nx, nu, m)
    for sign_r, sign_v, sign_d in ((-1, 0, -1), (1, -1, 1), (-1, 1, 0)):
        got = H.horizon_slab_reference(Qt, Rt, r, v, Ct, d, sign_r, sign_v, sign_d)
        assert got.shape == (B, H.slab_doubles(T, nx, nu, m))
        for i in range(B):
            stages, nterms, nlin = H.instance_stages(Qt[i].T, Rt[i].T, r[i], v[i], sign_r, sign_v, xvar)
            assert nlin == n and nterms == T * (nx * (nx + 1) // 2 + nu * (nu + 1) // 2) and len(stages) == (2 * T if nu else T)
            at, qt, oconst = QU.oracle(stages, varmap)
            # the slab's coefficients at the indices of the instance's canonical function: rows in z order, a stage's row its own columns
            coeff = np.concatenate([got[i, sec["SQ"]], got[i, sec["SR"]]] * T)
            rows = np.concatenate([np.repeat(st["xvar"], np.arange(len(st["xvar"]), 0, -1)) for st in stages])
            cols = np.concatenate([st["xvar"][j:] for st in stages for j in range(len(st["xvar"]))])
            assert np.array_equal(qt["row"], varmap[rows - 1]) and np.array_equal(qt["col"], varmap[cols - 1])
            assert np.array_equal(bits(qt["coeff"]), bits(coeff))
            want = QU.lin_by_var(at)
            q = got[i, sec["q"]]
            assert set(want) <= set(varmap[xvar - 1].tolist())
            consts = []
            for st in stages:
                la, nd = st["lin_at"], len(st["xvar"])
                bound = QU.lin_bound(st)
                err = np.abs(q[la:la + nd] - np.array([want.get(k, 0.0) for k in varmap[st["xvar"] - 1].tolist()]))
                assert np.all(err <= bound), (st["lin_at"], np.max(err / np.maximum(bound, 1e-300)))
                if st["sign"] and nd >= 63:                                     # the bound is not vacuous
                    assert np.max(bound) < 1e-9 * np.max(np.abs(q[la:la + nd]))
                if not st["sign"]:
                    assert np.all(bits(q[la:la + nd]) == 0)
                consts.append(H.stage_words(st["Q"], st["v"], st["sign"])[1])
            cb = QU.const_bound(stages, consts)
            assert abs(got[i, sec["const"]][0] - oconst) <= cb
            assert cb < 1e-9 * sum(abs(c) for c in consts)
            con = O.AffVec(m).vecaddsub(O.AffVec(m).matvecmul_vars(np.ascontiguousarray(Ct[i].T), xvar), d[i], sign_d < 0) if sign_d else \
                O.AffVec(m).matvecmul_vars(np.ascontiguousarray(Ct[i].T), xvar)
            ct, cc = con.moi(varmap)
            assert np.array_equal(bits(got[i, sec["C"]]), bits(ct["coeff"])) and np.array_equal(bits(got[i, sec["d"]]), bits(cc))
            assert np.array_equal(ct["var"], np.tile(varmap[xvar - 1], m)) and np.array_equal(ct["out"], np.repeat(np.arange(1, m + 1), n))


@pytest.mark.parametrize("T,nx,nu", [(1, 1, 0), (2, 2, 1), (3, 63, 5), (2, 64, 65), (2, 128, 3), (8, 20, 9), (5, 128, 0)])
def test_restatement_is_exact_on_coarse_dyadic_data(T, nx, nu):
    """Coarse dyadic data (batch_horizon_util): every intermediate value is an integer below 2^53 in its unit — asserted on the sums of
    magnitudes —, so SQ, SR, q and const equal the Python-integer values bit for bit and the oracle's literal composition word for word, in
    every order.  Zeros are compared after + 0.0."""
    B, m = 2, 2
    rng = np.random.default_rng(300 + 10 * nx + nu)
    Qt, Rt, r, v, Ct, d = H.horizon_data(B, T, nx, nu, m, rng, gen=F.coarse_dyadic)
    assert all(np.array_equal(a, 8 * np.round(a / 8)) and (a.size == 0 or np.max(np.abs(a)) <= 16368) for a in (Qt, Rt, r, v))
    n = T * (nx + nu)
    xvar, varmap = z_vars(n, rng)
    sec = H.sections(T, nx, nu, m)
    for sign_r, sign_v in ((-1, 1), (1, 0), (-1, -1)):
        got = H.horizon_slab_reference(Qt, Rt, r, v, Ct, d, sign_r, sign_v, -1)
        for i in range(B):
            SQ, SR, q, total, mags = H.exact_instance(Qt[i].T, Rt[i].T, r[i], v[i], sign_r, sign_v)
            assert mags[0] < 2 ** 31 and mags[1] < 2 ** 48 and mags[2] < 2 ** 53
            fl = lambda xs: np.array([float(x) for x in xs], dtype=np.float64)
            assert all(Fraction(float(x)) == x for x in SQ + SR + q + [total])                  # representable: the conversion rounds nothing
            assert np.array_equal(bits(got[i, sec["SQ"]] + 0.0), bits(fl(SQ) + 0.0)) and np.array_equal(bits(got[i, sec["SR"]] + 0.0), bits(fl(SR) + 0.0))
            assert np.array_equal(bits(got[i, sec["q"]] + 0.0), bits(fl(q) + 0.0))
            assert bits(got[i, sec["const"]])[0] == bits([float(total) + 0.0])[0]
            # .. and the oracle: the same numbers, whatever its order
            stages, _, _ = H.instance_stages(Qt[i].T, Rt[i].T, r[i], v[i], sign_r, sign_v, xvar)
            at, qt, oconst = QU.oracle(stages, varmap)
            assert np.array_equal(bits(qt["coeff"] + 0.0), bits(np.concatenate([got[i, sec["SQ"]], got[i, sec["SR"]]] * T) + 0.0))
            want = QU.lin_by_var(at)
            assert np.array_equal(bits(np.array([want.get(k, 0.0) for k in varmap[xvar - 1].tolist()]) + 0.0), bits(got[i, sec["q"]] + 0.0))
            assert bits([oconst + 0.0])[0] == bits(got[i, sec["const"]] + 0.0)[0]


# ---- 3. the restatement against quad_stages_util's restatement of pmt_quad_stages_f64 for the instance's table

@pytest.mark.parametrize("T,nx,nu", [(3, 65, 10), (4, 128, 33), (130, 5, 2), (257, 3, 0), (1, 1, 1)])
def test_restatement_equals_the_stage_node_s_for_the_instance_table(T, nx, nu):
    rng = np.random.default_rng(T + nx)
    Qt, Rt, r, v, Ct, d = H.horizon_data(1, T, nx, nu, 0, rng)
    n = T * (nx + nu)
    xvar, varmap = z_vars(n, rng)
    sec = H.sections(T, nx, nu, 0)
    for sign_r, sign_v in ((-1, 0), (1, -1), (0, 0), (0, 1)):
        got = H.horizon_slab_reference(Qt, Rt, r, v, Ct, d, sign_r, sign_v, -1)[0]
        stages, nterms, nlin = H.instance_stages(Qt[0].T, Rt[0].T, r[0], v[0], sign_r, sign_v, xvar)
        parts, const = QU.restate(stages, varmap)
        per = 2 if nu else 1
        for t in range(T):
            assert np.array_equal(bits(parts[per * t][0]["coeff"]), bits(got[sec["SQ"]]))
            if nu:
                assert np.array_equal(bits(parts[2 * t + 1][0]["coeff"]), bits(got[sec["SR"]]))
        assert np.array_equal(bits(np.concatenate([p[1]["coeff"] for p in parts])), bits(got[sec["q"]]))
        assert bits([const])[0] == bits(got[sec["const"]])[0]
        if not sign_r and not sign_v:
            assert np.all(bits(got[sec["q"]]) == 0) and bits(got[sec["const"]])[0] == 0
        # the expanded buffers are those slices with their indices, whole
        quad, lin, c2, vat, vc = H.expanded_reference(Qt[0].T, Rt[0].T, r[0], v[0], Ct[0].T, d[0], sign_r, sign_v, -1, xvar, varmap)
        assert len(quad) == 3 * nterms and len(lin) == 2 * n and len(vat) == 0 and len(vc) == 0 and bits([c2])[0] == bits([const])[0]
        assert np.array_equal(lin[1::2], varmap[xvar - 1]) and np.array_equal(lin[0::2], bits(got[sec["q"]]))


def test_wrong_restatements_are_told_apart():
    T, nx, nu, m = 3, 70, 5, 2
    Qt, Rt, r, v, Ct, d = H.horizon_data(1, T, nx, nu, m, np.random.default_rng(8))
    right = H.horizon_slab_reference(Qt, Rt, r, v, Ct, d, -1, 1, -1)[0]
    sec = H.sections(T, nx, nu, m)
    q = right[sec["q"]].reshape(T, nx + nu)
    stage_major = right.copy()                                                  # all x stages, then all u stages
    stage_major[sec["q"]] = np.concatenate([q[:, :nx].reshape(-1), q[:, nx:].reshape(-1)])
    swapped = H.horizon_slab_reference(Qt, Rt, r, v, Ct, d, 1, -1, -1)[0]       # the two signs exchanged
    consts = [H.stage_words(M, ref[t], s)[1] for t in range(T) for M, ref, s in ((Qt[0].T, r[0], -1), (Rt[0].T, v[0], 1))]
    assert right[sec["const"]][0] == H.SU.chain_tree_sum(np.array(consts))      # z order: x_0, u_0, x_1, ..
    x_only = right.copy()                                                       # the inputs' constants left out
    x_only[sec["const"]] = H.SU.chain_tree_sum(np.array(consts[0::2]))
    other_R = right.copy()
    other_R[sec["SR"]] = H.SU.symmetrised(Rt[0].T)[np.tril_indices(nu)]
    colmajor = right.copy()
    colmajor[sec["C"]] = Ct[0].reshape(-1)
    for name, wrong in (("q stage-major per matrix", stage_major), ("signs exchanged", swapped), ("column-wise triangle of R", other_R),
                        ("column-major C", colmajor), ("constant of the x stages alone", x_only)):
        assert not np.array_equal(bits(wrong), bits(right)), name


# ---- 4. the entry points without a device

P = C.c_void_p(64)                          # never dereferenced: each call is rejected, or returns, before any device call


def _coeffs(lib, Q=P, R=P, r=P, v=P, Cm=P, d=P, B=1, T=3, nx=4, nu=2, m=2, sign_r=-1, sign_v=-1, sign_d=-1, out=P, stride=None):
    L = H.slab_doubles(max(T, 0), max(nx, 0), max(nu, 0), max(m, 0))
    lib.call(COEFFS, Q, R, r, v, Cm, d, B, T, nx, nu, m, sign_r, sign_v, sign_d, out, L if stride is None else stride, None)


def _expand(lib, slab=P, T=3, nx=4, nu=2, m=2, xvar=P, varmap=P, quad=P, lin=P, const=P, vat=P, vconsts=P):
    lib.call(EXPAND, slab, T, nx, nu, m, xvar, varmap, quad, lin, const, vat, vconsts, None)


BAD_DIMS = [{"T": -1}, {"nx": -4}, {"nu": -1}, {"m": -2}, {"nx": 0}, {"nx": H.MAX_DIM + 1}, {"nu": H.MAX_DIM + 1}, {"nx": 1 << 40}, {"T": 0}, {"T": H.MAX_T + 1},
            {"T": 1 << 40}]
BAD_IDS = ["T-negative", "nx-negative", "nu-negative", "m-negative", "nx-zero", "nx-129", "nu-129", "nx-huge", "T-zero", "T-513", "T-huge"]


@pytest.mark.parametrize("bad", BAD_DIMS + [{"B": -1}, {"stride": H.slab_doubles(3, 4, 2, 2) - 1}, {"stride": 0}, {"stride": -5}],
                         ids=BAD_IDS + ["B-negative", "stride-L-1", "stride-zero", "stride-negative"])
def test_dimension_errors_of_the_coefficients_come_before_any_device_call(lib, bad):
    kw = dict(bad)
    if "stride" not in kw:
        kw["stride"] = 1 << 62
    with pytest.raises(lib.DimensionMismatch, match="batch_horizon"):
        _coeffs(lib, **kw)
    # .. and before the empty batch's return: B == 0 does not excuse them
    if "B" not in bad:
        with pytest.raises(lib.DimensionMismatch, match="batch_horizon"):
            _coeffs(lib, B=0, **kw)


@pytest.mark.parametrize("bad", BAD_DIMS, ids=BAD_IDS)
def test_dimension_errors_of_the_expansion_come_before_any_device_call(lib, bad):
    with pytest.raises(lib.DimensionMismatch, match="batch_horizon_expand"):
        _expand(lib, **bad)


@pytest.mark.parametrize("signs", [(2, 0, 0), (-2, 0, 0), (0, 2, 0), (0, -2, 0), (0, 0, 2), (0, 0, -2), (7, 7, 7)])
def test_signs_outside_minus_one_zero_one_are_argument_errors(lib, signs):
    with pytest.raises(lib.ArgumentError, match="sign"):
        _coeffs(lib, sign_r=signs[0], sign_v=signs[1], sign_d=signs[2])
    with pytest.raises(lib.DimensionMismatch):                                  # the dimension checks come first
        _coeffs(lib, sign_r=signs[0], sign_v=signs[1], sign_d=signs[2], stride=3)


@pytest.mark.parametrize("null", ["Q", "R", "r", "v", "Cm", "d", "out"])
def test_null_pointers_where_the_coefficients_need_data(lib, null):
    with pytest.raises(lib.ArgumentError, match="null"):
        _coeffs(lib, **{null: None})


@pytest.mark.parametrize("null", ["slab", "xvar", "varmap", "quad", "lin", "const", "vat", "vconsts"])
def test_null_pointers_where_the_expansion_needs_them(lib, null):
    with pytest.raises(lib.ArgumentError, match="null"):
        _expand(lib, **{null: None})


def test_null_pointers_where_no_data_is_read_and_empty_batches(lib):
    """What these calls would launch needs a GPU: on a machine without one a launch is a HIP error, with one the dummy pointers would be read —
    each must be rejected for the pointer that IS needed, or return PMT_OK without a launch"""
    # a sign of 0: the reference may be NULL; the call then gets as far as the next missing pointer
    with pytest.raises(lib.ArgumentError, match="null"):
        _coeffs(lib, r=None, sign_r=0, out=None)
    with pytest.raises(lib.ArgumentError, match="null"):
        _coeffs(lib, v=None, sign_v=0, out=None)
    with pytest.raises(lib.ArgumentError, match="null"):
        _coeffs(lib, r=None, v=None, sign_r=0, sign_v=0, out=None)
    # nu == 0: R and v are not needed; m == 0: C and d are not needed
    with pytest.raises(lib.ArgumentError, match="null"):
        _coeffs(lib, R=None, v=None, nu=0, out=None)
    with pytest.raises(lib.ArgumentError, match="null"):
        _coeffs(lib, Cm=None, d=None, m=0, out=None)
    with pytest.raises(lib.ArgumentError, match="null"):
        _expand(lib, vat=None, vconsts=None, m=0, const=None)
    # sign_d == 0 still needs d, as the siblings do
    with pytest.raises(lib.ArgumentError, match="null"):
        _coeffs(lib, d=None, sign_d=0)
    # an empty batch is complete as it stands, whatever the pointers: PMT_OK, nothing launched
    for T, nx, nu, m in ((3, 4, 2, 2), (1, 1, 0, 0), (H.MAX_T, H.MAX_DIM, H.MAX_DIM, 1), (5, 2, 0, 3)):
        L = H.slab_doubles(T, nx, nu, m)
        lib.call(COEFFS, None, None, None, None, None, None, 0, T, nx, nu, m, -1, 1, -1, None, L, None)
        lib.call(COEFFS, None, None, None, None, None, None, 0, T, nx, nu, m, 0, 0, 0, None, L + 3, None)


# ---- 5. the dimension checks the three objective files share: every out-of-range argument, its code and the whole message

# (argument, value) -> the message behind "<who>: ", as the sources worded it when each file had its own copy of the checks; the first
# failing check speaks, in the order negative, nx < 1, above 128, T, term, m
DIM_MESSAGES = [("T", -1, "negative dimension"), ("nx", -4, "negative dimension"), ("nu", -1, "negative dimension"), ("m", -2, "negative dimension"),
                ("nx", 0, "nx < 1"), ("nx", 129, "nx or nu above 128"), ("nu", 129, "nx or nu above 128"), ("nx", 1 << 40, "nx or nu above 128"),
                ("T", 0, "T outside 1 .. 512"), ("T", 513, "T outside 1 .. 512"), ("T", 1 << 40, "T outside 1 .. 512"),
                ("term", 2, "term must be 0 or 1"), ("term", -1, "term must be 0 or 1"), ("m", (1 << 40) + 1, "m beyond 2^40")]


def _objective_calls(lib):
    """who -> (call(T, nx, nu, term, m), takes a term): the six entry points with every pointer made up and a stride that is never short"""
    big = 1 << 62
    desc = lib.batch_horizon_terms(Q=64, R=64, r=64, v=64, C=64, d=64, sign_r=-1, sign_v=-1, sign_d=-1)      # (no P: term == 0 there)
    return {
        "batch_horizon": (lambda T, nx, nu, term, m: lib.call(COEFFS, P, P, P, P, P, P, 1, T, nx, nu, m, -1, -1, -1, P, big, None), False),
        "batch_horizon_expand": (lambda T, nx, nu, term, m: lib.call(EXPAND, P, T, nx, nu, m, P, P, P, P, P, P, P, None), False),
        "batch_horizon_terms": (lambda T, nx, nu, term, m: lib.call("pmt_batch_horizon_terms_coeffs_f64", C.byref(desc), 1, T, nx, nu, m, P, big, None), False),
        "batch_horizon_terms_expand": (lambda T, nx, nu, term, m: lib.call("pmt_batch_horizon_terms_expand_f64", P, T, nx, nu, term, m, P, P, P, P, P, P, P, None), True),
        "batch_horizon_tv": (lambda T, nx, nu, term, m: lib.call("pmt_batch_horizon_tv_coeffs_f64", P, P, P, P, P, P, 1, T, nx, nu, term, m, -1, -1, -1, P, big, None), True),
        "batch_horizon_tv_expand": (lambda T, nx, nu, term, m: lib.call("pmt_batch_horizon_tv_expand_f64", P, T, nx, nu, term, m, P, P, P, P, P, P, P, None), True),
    }


@pytest.mark.parametrize("who", ["batch_horizon", "batch_horizon_expand", "batch_horizon_terms", "batch_horizon_terms_expand", "batch_horizon_tv",
                                 "batch_horizon_tv_expand"])
def test_every_out_of_range_dimension_keeps_its_code_and_message(lib, who):
    fn, takes_term = _objective_calls(lib)[who]
    for arg, value, text in DIM_MESSAGES:
        if arg == "term" and not takes_term:
            continue
        kw = dict(T=3, nx=4, nu=2, term=0, m=2)
        kw[arg] = value
        with pytest.raises(lib.DimensionMismatch) as e:
            fn(**kw)
        assert str(e.value) == "%s: %s" % (who, text), (arg, value)
    # the bounds themselves are in range: T, nx and nu at theirs get as far as the null output
    with pytest.raises(lib.ArgumentError, match="null pointer"):
        lib.call(COEFFS, P, P, P, P, P, P, 1, H.MAX_T, H.MAX_DIM, H.MAX_DIM, 1, -1, -1, -1, None, 1 << 62, None)
