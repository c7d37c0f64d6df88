"""CPU-only: the batched horizons with time-varying stage weights (pmt_batch_horizon_tv_coeffs_f64, pmt_batch_horizon_tv_expand_f64,
batch.horizon_tv_slab_layout).  The restatement of the header's contract (batch_horizon_tv_util), which tests/test_gpu_batch_horizon_tv.py
compares the kernels with bit for bit, against the oracle's literal composition per instance — every stage's dot(e, M*e) sequence with the
stage's own matrix, added in z order, canonicalize!, the MOI copy (quad_stages_util.oracle) — on coarse dyadic data whose every sum is exact
(batch_horizon_util's docstring: at most 16 stage constants); against the time-invariant sibling's restatement with equal matrices per
stage, and the terminal sibling's with unit weights; the slab's layout; both entry points' argument errors through the C ABI, which need no
GPU because validation precedes any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import batch_form_util as F
import batch_horizon_terms_util as HT
import batch_horizon_tv_util as V
import batch_horizon_util as H
import quad_stages_util as QU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COEFFS, EXPAND, DOUBLES = "pmt_batch_horizon_tv_coeffs_f64", "pmt_batch_horizon_tv_expand_f64", "pmt_batch_horizon_tv_slab_doubles"
P = C.c_void_p(64)                          # never dereferenced: each call is rejected, or returns, before any device call


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def lib():
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


def z_vars(n, rng, extra=7):
    xvar = np.sort(rng.choice(np.arange(1, n + extra + 1), n, replace=False)).astype(np.int64)
    return xvar, (rng.permutation(n + extra) + 1 + 100).astype(np.int64)


# ---- 1. the restatement against the oracle's literal composition, on data whose every sum is exact

@pytest.mark.parametrize("T,nx,nu,term", [(1, 1, 0, 0), (2, 2, 1, 1), (3, 63, 5, 0), (2, 64, 65, 1), (2, 128, 3, 0), (7, 20, 9, 1), (5, 128, 0, 1), (8, 17, 33, 0)])
def test_restatement_equals_the_oracle_composition_on_coarse_dyadic_data(T, nx, nu, term):
    """at most 16 stage constants of at most 128 rows: every product and sum is exact in every order (batch_horizon_util), so S, q and const
    equal the oracle's canonical function word for word.  Zeros are compared after + 0.0: integers know no signed zero."""
    B, m = 2, 2
    n, ns = V.dims(T, nx, nu, term)
    assert ns <= 16
    rng = np.random.default_rng(500 + 10 * nx + nu + term)
    Qt, Rt, r, v, Ct, d = V.tv_data(B, T, nx, nu, term, m, rng, gen=F.coarse_dyadic)
    assert all(np.array_equal(a, 8 * np.round(a / 8)) and (a.size == 0 or np.max(np.abs(a)) <= 16368) for a in (Qt, Rt, r, v))
    xvar, varmap = z_vars(n, rng)
    sec = V.sections(T, nx, nu, term, m)
    for sign_r, sign_v in ((-1, 1), (1, 0), (-1, -1)):
        got = V.slab_reference(Qt, Rt, r, v, Ct, d, sign_r, sign_v, -1)
        assert got.shape == (B, V.slab_doubles(T, nx, nu, term, m))
        for i in range(B):
            stages, nterms, nlin = V.instance_stages(V.matrices(Qt[i]), V.matrices(Rt[i]), r[i], v[i], sign_r, sign_v, xvar)
            assert (nterms, nlin, len(stages)) == (sec["q"].start, n, ns)
            at, qt, oconst = QU.oracle(stages, varmap)
            assert np.array_equal(bits(qt["coeff"] + 0.0), bits(got[i, :sec["q"].start] + 0.0))
            want = QU.lin_by_var(at)
            assert np.array_equal(bits(np.array([want.get(k, 0.0) for k in varmap[xvar - 1].tolist()]) + 0.0), bits(got[i, sec["q"]] + 0.0))
            assert bits([oconst + 0.0])[0] == bits(got[i, sec["const"]] + 0.0)[0]
            # the stage constants: each the oracle's constant of the stage alone; const their exact sum
            for s, st in enumerate(stages):
                one = dict(st, quad_at=0, lin_at=0)
                assert bits([QU.oracle([one], varmap)[2] + 0.0])[0] == bits(got[i, sec["sconst"]][s:s + 1] + 0.0)[0]
            assert float(np.sum(got[i, sec["sconst"]])) == got[i, sec["const"]][0]
            assert np.array_equal(bits(got[i, sec["C"]]), bits(Ct[i].T.reshape(-1))) and np.array_equal(bits(got[i, sec["d"]]), bits(0.0 - d[i]))


# ---- 2. against the siblings' restatements

@pytest.mark.parametrize("T,nx,nu", [(1, 3, 2), (3, 5, 0), (4, 17, 15), (2, 65, 10), (130, 3, 2)])
def test_equal_matrices_per_stage_give_the_time_invariant_slab_section_by_section(T, nx, nu):
    B, m = 2, 3
    Qt1, Rt1, r, v, Ct, d = H.horizon_data(B, T, nx, nu, m, np.random.default_rng(T + nx + nu))
    Qt, Rt = np.repeat(Qt1[:, None], T, axis=1), np.repeat(Rt1[:, None], T, axis=1)
    sv, si = V.sections(T, nx, nu, 0, m), H.sections(T, nx, nu, m)
    for signs in ((-1, 1, -1), (1, 0, 0), (0, -1, 1)):
        tv, ti = V.slab_reference(Qt, Rt, r, v, Ct, d, *signs), H.horizon_slab_reference(Qt1, Rt1, r, v, Ct, d, *signs, T=T)
        for (kind, _), blk in zip(V.stage_kinds(T, nu, 0), sv["S"]):
            assert np.array_equal(bits(tv[:, blk]), bits(ti[:, si["SQ" if kind == "x" else "SR"]]))
        for k in ("q", "const", "C", "d"):
            assert np.array_equal(bits(tv[:, sv[k]]), bits(ti[:, si[k]])), k


@pytest.mark.parametrize("T,nx,nu", [(1, 3, 2), (3, 5, 0), (3, 17, 15), (2, 65, 10)])
def test_a_terminal_stage_with_equal_matrices_gives_the_terminal_sibling_s_words_with_unit_weights(T, nx, nu):
    """term == 1, Q_{i,t} = Q_i for t < T and Q_{i,T} = P_i: as far as the layouts share words — the blocks, q, const, C, d-consts"""
    B, m = 2, 2
    rng = np.random.default_rng(T * nx + nu)
    Qt1, Rt1, r, v, _, _ = H.horizon_data(B, T, nx, nu, 0, rng)
    Pt, rN = rng.standard_normal((B, nx, nx)), rng.standard_normal((B, nx))
    n, ns = V.dims(T, nx, nu, 1)
    Ct, d = rng.standard_normal((B, n, m)), rng.standard_normal((B, m))
    Qt = np.concatenate([np.repeat(Qt1[:, None], T, axis=1), Pt[:, None]], axis=1)
    Rt = np.repeat(Rt1[:, None], T, axis=1)
    rr = np.concatenate([r, rN[:, None]], axis=1)
    batch = {"T": T, "Qt": Qt1, "Rt": Rt1, "Pt": Pt, "r": r, "v": v, "rN": rN, "Ct": Ct, "d": d}
    sv, st = V.sections(T, nx, nu, 1, m), HT.sections(T, nx, nu, 1, m)
    for sign_r, sign_v, sign_d in ((-1, 1, -1), (1, 0, 1), (0, -1, 0)):
        tv = V.slab_reference(Qt, Rt, rr, v, Ct, d, sign_r, sign_v, sign_d)
        ti = HT.slab_reference(batch, (sign_r, sign_v, sign_r, sign_d))
        for (kind, t), blk in zip(V.stage_kinds(T, nu, 1), sv["S"]):
            assert np.array_equal(bits(tv[:, blk]), bits(ti[:, st["SP" if t == T else ("SQ" if kind == "x" else "SR")]]))
        for k in ("q", "const", "C", "d"):
            assert np.array_equal(bits(tv[:, sv[k]]), bits(ti[:, st[k]])), k
        assert np.all(ti[:, st["W"]] == 1.0) and st["W"].stop - st["W"].start == ns


def test_stages_differ_so_a_stage_mix_up_shows():
    T, nx, nu, m = 3, 4, 2, 1
    Qt, Rt, r, v, Ct, d = V.tv_data(2, T, nx, nu, 1, m, np.random.default_rng(3))
    right = V.slab_reference(Qt, Rt, r, v, Ct, d, -1, 1, -1)
    sec = V.sections(T, nx, nu, 1, m)
    assert not np.array_equal(bits(right[:, sec["S"][0]]), bits(right[:, sec["S"][2]]))
    swapped = V.slab_reference(Qt[:, ::-1], Rt, r[:, ::-1], v, Ct, d, -1, 1, -1)               # the x stages in reverse
    assert np.array_equal(bits(swapped[:, sec["S"][0]]), bits(right[:, sec["S"][-1]]))
    assert np.array_equal(bits(swapped[:, sec["qs"][0]]), bits(right[:, sec["qs"][-1]]))
    assert np.array_equal(bits(swapped[:, sec["sconst"]][:, 0]), bits(right[:, sec["sconst"]][:, -1]))
    assert np.array_equal(bits(swapped[:, sec["S"][1]]), bits(right[:, sec["S"][1]]))          # u_0 stays
    other = V.slab_reference(Qt, Rt, r, v, Ct, d, 1, -1, -1)                                    # the two signs exchanged
    assert not np.array_equal(bits(other[:, sec["q"]]), bits(right[:, sec["q"]]))
    # the encoded data name their place
    Qe, Re, re_, ve = V.encoded_data(3, 4, 5, 3, 1)
    words = np.concatenate([np.abs(a).reshape(-1) for a in (Qe, Re)])
    assert len(np.unique(words)) == len(words) and np.any(Qe < 0) and np.any(Qe > 0) and np.any(re_ < 0) and np.any(ve > 0)
    assert abs(Qe[2, 4, 3, 1]) == (((2 * 1024 + 8) * 128 + 1) * 128 + 3) + 0.5 and abs(Re[2, 1, 0, 2]) == (((2 * 1024 + 3) * 128 + 2) * 128 + 0) + 0.5
    assert abs(re_[1, 2, 4]) == ((1024 + 4) * 128 + 4) + 0.25


def test_expanded_reference_is_the_slab_with_its_indices():
    T, nx, nu, term, m = 3, 5, 2, 1, 2
    n, ns = V.dims(T, nx, nu, term)
    rng = np.random.default_rng(12)
    Qt, Rt, r, v, Ct, d = V.tv_data(1, T, nx, nu, term, m, rng)
    xvar, varmap = z_vars(n, rng)
    sec = V.sections(T, nx, nu, term, m)
    slab = V.slab_reference(Qt, Rt, r, v, Ct, d, -1, 0, 1)[0]
    quad, lin, const, vat, vc = V.expanded_reference(V.matrices(Qt[0]), V.matrices(Rt[0]), r[0], None, Ct[0].T, d[0], -1, 0, 1, xvar, varmap)
    assert np.array_equal(quad.reshape(-1, 3)[:, 0], bits(slab[:sec["q"].start])) and np.array_equal(lin[0::2], bits(slab[sec["q"]]))
    assert np.array_equal(lin[1::2], varmap[xvar - 1]) and bits([const])[0] == bits(slab[sec["const"]])[0]
    assert np.array_equal(vat.reshape(-1, 3)[:, 1], bits(slab[sec["C"]])) and np.array_equal(bits(vc), bits(slab[sec["d"]]))
    # a row of stage s names the stage's own variables
    rows = quad.reshape(-1, 3)[sec["S"][2]]
    assert set(rows[:, 1].tolist()) | set(rows[:, 2].tolist()) == set(varmap[xvar[nx + nu:2 * nx + nu] - 1].tolist())


# ---- 3. the layout

def test_slab_length_equals_the_layout_over_a_grid(lib):
    from parametron_jl_amd import batch as PB
    fn = lib.load().pmt_batch_horizon_tv_slab_doubles
    for T in (1, 2, 7, 512):
        for nx in (1, 3, 64, 65, 128):
            for nu in (0, 1, 64, 128):
                for m in (0, 1, 33):
                    for term in (0, 1):
                        off, L = PB.horizon_tv_slab_layout(T, nx, nu, m, bool(term))
                        sec = V.sections(T, nx, nu, term, m)
                        n, ns = V.dims(T, nx, nu, term)
                        assert fn(T, nx, nu, term, m) == L == V.slab_doubles(T, nx, nu, term, m) == sec["d"].stop
                        assert off["S"] == [s.start for s in sec["S"]] and len(off["S"]) == ns
                        assert [off[k] for k in ("q", "sconst", "const", "C", "dconst")] == [sec[k].start for k in ("q", "sconst", "const", "C", "d")]
                        assert [0] + [s.stop for s in sec["S"]] == [s.start for s in sec["S"]] + [sec["q"].start]        # the blocks tile S
    assert PB.horizon_tv_slab_layout(1, 1, 0, 0, False)[1] == 4                  # [S: 1 | q: 1 | sconst: 1 | const]
    # one stage without inputs: the tracking cost's slab with the stage constant between q and const
    off, L = PB.horizon_tv_slab_layout(1, 40, 0, 6, False)
    assert L == PB.slab_layout(40, 6)[1] + 1 and off["q"] == PB.slab_layout(40, 6)[0]["q"]
    # with T stages the blocks of the time-invariant sibling T times, and one constant per stage
    assert PB.horizon_tv_slab_layout(5, 7, 3, 2, False)[1] == PB.horizon_slab_layout(5, 7, 3, 2)[1] + 4 * (28 + 6) + 10


# ---- 4. the entry points without a device

def _coeffs(lib, Q=P, R=P, r=P, v=P, Cm=P, d=P, B=1, T=3, nx=4, nu=2, term=0, m=2, sign_r=-1, sign_v=-1, sign_d=-1, out=P, stride=None):
    L = V.slab_doubles(max(T, 0), max(nx, 0), max(nu, 0), 1 if term else 0, max(m, 0))
    lib.call(COEFFS, Q, R, r, v, Cm, d, B, T, nx, nu, term, m, sign_r, sign_v, sign_d, out, L if stride is None else stride, None)


def _expand(lib, slab=P, T=3, nx=4, nu=2, term=0, m=2, xvar=P, varmap=P, quad=P, lin=P, const=P, vat=P, vconsts=P):
    lib.call(EXPAND, slab, T, nx, nu, term, m, xvar, varmap, quad, lin, const, vat, vconsts, None)


BAD_DIMS = [{"T": -1}, {"nx": -4}, {"nu": -1}, {"m": -2}, {"nx": 0}, {"nx": 129}, {"nu": 129}, {"nx": 1 << 40}, {"T": 0}, {"T": 513}, {"T": 1 << 40},
            {"term": 2}, {"term": -1}]


@pytest.mark.parametrize("bad", BAD_DIMS + [{"B": -1}, {"stride": V.slab_doubles(3, 4, 2, 0, 2) - 1}, {"stride": 0}, {"stride": -5}], ids=str)
def test_dimension_errors_of_the_coefficients_come_before_any_device_call(lib, bad):
    hdr = open(os.path.join(ROOT, "include", "parametron_hip.h")).read()
    assert re.search(r"#define PMT_BATCH_HORIZON_MAX_DIM\s+128", hdr) and re.search(r"#define PMT_BATCH_HORIZON_MAX_T\s+512", hdr)
    kw = dict(bad)
    if "stride" not in kw:
        kw["stride"] = 1 << 62
    with pytest.raises(lib.DimensionMismatch, match="batch_horizon_tv"):
        _coeffs(lib, **kw)
    if "B" not in bad:                                                          # B == 0 does not excuse them
        with pytest.raises(lib.DimensionMismatch, match="batch_horizon_tv"):
            _coeffs(lib, B=0, **kw)


def test_the_stride_of_the_time_invariant_slab_is_too_short(lib):
    with pytest.raises(lib.DimensionMismatch, match="out_stride"):
        _coeffs(lib, stride=H.slab_doubles(3, 4, 2, 2))
    with pytest.raises(lib.DimensionMismatch, match="out_stride"):              # the terminal stage's words count
        _coeffs(lib, term=1, stride=V.slab_doubles(3, 4, 2, 0, 2))


@pytest.mark.parametrize("bad", BAD_DIMS, ids=str)
def test_dimension_errors_of_the_expansion_come_before_any_device_call(lib, bad):
    with pytest.raises(lib.DimensionMismatch, match="batch_horizon_tv_expand"):
        _expand(lib, **bad)


@pytest.mark.parametrize("signs", [(2, 0, 0), (-2, 0, 0), (0, 2, 0), (0, -2, 0), (0, 0, 2), (0, 0, -2), (7, 7, 7)])
def test_signs_outside_minus_one_zero_one_are_argument_errors(lib, signs):
    with pytest.raises(lib.ArgumentError, match="sign"):
        _coeffs(lib, sign_r=signs[0], sign_v=signs[1], sign_d=signs[2])
    with pytest.raises(lib.DimensionMismatch):                                  # the dimension checks come first
        _coeffs(lib, sign_r=signs[0], sign_v=signs[1], sign_d=signs[2], stride=3)


@pytest.mark.parametrize("null", ["Q", "R", "r", "v", "Cm", "d", "out"])
def test_null_pointers_where_the_coefficients_need_data(lib, null):
    with pytest.raises(lib.ArgumentError, match="null pointer"):
        _coeffs(lib, **{null: None})


@pytest.mark.parametrize("null", ["slab", "xvar", "varmap", "quad", "lin", "const", "vat", "vconsts"])
def test_null_pointers_where_the_expansion_needs_data(lib, null):
    with pytest.raises(lib.ArgumentError, match="null pointer"):
        _expand(lib, **{null: None})


def test_an_empty_batch_is_ok_whatever_the_pointers(lib):
    _coeffs(lib, Q=None, R=None, r=None, v=None, Cm=None, d=None, out=None, B=0)
    _coeffs(lib, Q=None, R=None, r=None, v=None, Cm=None, d=None, out=None, B=0, T=1, nx=1, nu=0, term=1, m=0)


def test_null_is_allowed_where_the_contract_does_not_read(lib):
    """a reference whose sign is 0, R and v with nu == 0, C and d with m == 0, out_vat / out_vconsts with m == 0: the source's null-pointer
    tests say so, and an empty batch passes validation with them; the calls that write such slabs run in the GPU suite (a call with made-up
    addresses must never reach a launch here)"""
    _coeffs(lib, B=0, r=None, v=None, sign_r=0, sign_v=0)
    _coeffs(lib, B=0, R=None, v=None, nu=0)
    _coeffs(lib, B=0, Cm=None, d=None, m=0)
    src = open(os.path.join(ROOT, "parametron.jl_amd", "csrc", "batch_horizon_tv.hip")).read()
    assert "PMT_REQUIRE(out && Q && (nu == 0 || R) && (sign_r == 0 || r) && (nu == 0 || sign_v == 0 || v) && (m == 0 || (Cm && d)), PMT_INVALID_ARGUMENT" in src
    assert "&& out_const && (m == 0 || (out_vat && out_vconsts)), PMT_INVALID_ARGUMENT" in src
    assert src.index("if (B == 0) return PMT_OK;") < src.index("PMT_REQUIRE(out && Q &&") < src.index("return dispatch(stream")


def test_bindings_and_julia_wrappers_name_the_entry_points(lib):
    jl = open(os.path.join(ROOT, "julia", "ParametronHIP.jl")).read()
    hdr = open(os.path.join(ROOT, "include", "parametron_hip.h")).read()
    raw = C.CDLL(lib.LIB_PATH)
    for name, nargs in ((DOUBLES, 5), (COEFFS, 18), (EXPAND, 14)):
        assert "(:%s, lib)" % name in jl and hasattr(raw, name) and len(lib.SIGNATURES[name][1]) == nargs and name + "(" in hdr
    from parametron_jl_amd import batch as PB
    taken = set()
    for cls in (PB.BatchLSQ, PB.BatchTracking, PB.BatchMPC, PB.BatchLTVMPC, PB.BatchWeightedMPC, PB.BatchWeightedLTVMPC):
        taken |= set(cls.SEEDS.values())
    S = PB.BatchTVMPC.SEEDS
    assert len(set(S.values())) == 9 and set(S.values()).isdisjoint(taken) and all(S[k] == s for k, s in PB.BatchTVHorizon.SEEDS.items())
    assert PB.BatchTVHorizon.EXPAND == EXPAND and issubclass(PB.BatchTVMPC, PB._TimeVaryingDynamics) and issubclass(PB.BatchTVHorizon, PB._HorizonBatch)
