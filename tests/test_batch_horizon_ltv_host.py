"""CPU-only: the batch of horizons' time-varying dynamics sections (pmt_batch_horizon_dynamics_tv_f64, pmt_batch_horizon_dynamics_tv_expand_f64).
The restatement of the header's contract (batch_horizon_ltv_util) against its two anchors — affine_stages_util's restatement of
pmt_affine_stages_f64 on the instance's own tables with a matrix pair per stage, word for word on integer views, and, with equal matrices
per stage, batch_horizon_dyn_util's section block by block — and against the oracle's vecadd! / vecsubtract! chain and MOI copy for the
spelling x+ - A*x - B*u - w; the section's layout; both entry points' argument errors through the C ABI, which need no GPU because
validation precedes any device call.  Nothing here takes a tolerance: nothing is computed."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import affine_stages_util as U
import batch_horizon_dyn_util as D
import batch_horizon_ltv_util as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COEFFS, EXPAND, DOUBLES = "pmt_batch_horizon_dynamics_tv_f64", "pmt_batch_horizon_dynamics_tv_expand_f64", "pmt_batch_horizon_dynamics_tv_doubles"
FAKE = C.c_void_p(64)                       # never dereferenced: the calls below are rejected first, or have nothing to do
POISON = -7
SHAPES = [(1, 3, 2), (2, 1, 0), (3, 3, 2), (4, 5, 0)]          # (T, nx, nu): T = 1, T = 2, nu = 0 among them


@pytest.fixture(scope="module")
def lib():
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


def _limits():
    hdr = open(os.path.join(ROOT, "include", "parametron_hip.h")).read()
    return tuple(int(re.search(r"#define %s\s+(\d+)" % name, hdr).group(1)) for name in ("PMT_BATCH_HORIZON_MAX_DIM", "PMT_BATCH_HORIZON_MAX_T"))


def _instance(T, nx, nu, seed):
    """one instance (index 1 of three) with its variables and a permuted varmap; zeros of both signs among the data"""
    rng = np.random.default_rng(seed)
    At, Bt, h = V.ltv_data(3, T, nx, nu, rng)
    h[1, 0, 0], h[1, -1, -1] = -0.0, 0.0
    if T > 1:
        At[1, 0, 0, 0], At[1, -1, -1, -1] = -0.0, 0.0
    n = T * (nx + nu)
    xvar = np.sort(rng.choice(np.arange(1, n + 10), n, replace=False)).astype(np.int64)
    varmap = (rng.permutation(n + 9) + 1 + 100).astype(np.int64)
    return At, Bt, h, xvar, varmap


def _check_against_the_tables(T, nx, nu, signs, seed=0):
    sign_xp, sign_a, sign_b, sign_h = signs
    At, Bt, h, xvar, varmap = _instance(T, nx, nu, seed + 100 * T + 10 * nx + nu)
    section = V.section_reference(At, Bt, h, sign_a, sign_b, sign_h)[1]
    assert section.shape == (V.section_doubles(T, nx, nu),)
    A, Bm = V.matrices(At[1], Bt[1])
    stages, nterms, nconsts = V.instance_stages(A, Bm, h[1], sign_xp, sign_a, sign_b, sign_h, xvar)
    assert (nterms, nconsts) == (V.term_count(T, nx, nu), T * nx)
    for vmap in (varmap, None):
        terms, consts = V.expanded_reference(section, T, nx, nu, sign_xp, xvar, vmap)
        want_t, want_c = U.images(stages, vmap, nterms, nconsts, POISON)
        assert np.array_equal(terms, want_t), (T, nx, nu, signs)
        assert np.array_equal(V.bits(consts), V.bits(want_c)), (T, nx, nu, signs)
    return section


@pytest.mark.parametrize("signs", list(itertools.product((1, -1), (1, -1), (1, -1), (-1, 0, 1))), ids=lambda s: "%+d%+d%+d%+d" % s)
def test_restated_expansion_equals_the_stage_tables_for_all_24_sign_combinations(signs):
    for T, nx, nu in SHAPES:
        section = _check_against_the_tables(T, nx, nu, signs, seed=7)
        hc = section[V.sections(T, nx, nu)["hconst"]]
        assert not np.any(np.signbit(hc[hc == 0.0])) and np.any(hc == 0.0)            # a -0.0 does not survive 0.0 (+|-) h
        if T * nx > 2:                      # (_instance zeroes two of the constants)
            assert np.all(V.bits(hc) == 0) == (signs[3] == 0)
        if T > 1 and nx > 1:              # not vacuous: zeros of both signs among the AB words
            ab = section[:V.sections(T, nx, nu)["hconst"].start]
            assert np.any(np.signbit(ab[ab == 0.0])) and np.any(~np.signbit(ab[ab == 0.0]))


def test_stages_differ_so_a_stage_mix_up_shows():
    """the stage tables of the check above really carry a matrix pair per stage"""
    At, Bt, h, xvar, varmap = _instance(3, 3, 2, 5)
    assert not np.array_equal(At[1, 0], At[1, 1]) and not np.array_equal(Bt[1, 0], Bt[1, 1])
    sec = V.sections(3, 3, 2)
    section = V.section_reference(At, Bt, h, -1, -1, -1)[1]
    assert not np.array_equal(V.bits(section[sec["AB"][0]]), V.bits(section[sec["AB"][1]]))
    swapped = V.section_reference(At[:, ::-1], Bt[:, ::-1], h, -1, -1, -1)[1]
    assert np.array_equal(V.bits(swapped[sec["AB"][0]]), V.bits(section[sec["AB"][1]]))
    assert np.array_equal(V.bits(swapped[sec["hconst"]]), V.bits(section[sec["hconst"]]))


def test_restatement_equals_the_oracle_chain():
    """x_0 - h_0 and x_t - A_t*x_{t-1} - B_t*u_{t-1} - h_t through the oracle: matvecmul! per product, vecsubtract! per -, and
    update!(::MOI.VectorAffineFunction, fs, varmap); every word on integer views, the data with zeros of both signs"""
    entry.build()
    from oracle import oracle as O
    T, nx, nu = 4, 3, 2
    w = nx + nu
    At, Bt, h, xvar, varmap = _instance(T, nx, nu, 11)
    A, Bm = V.matrices(At[1], Bt[1])

    def sub(a, b):
        if O._kind(a) == "vars" and O._kind(b) == "affs":
            # vecsubtract!(dest, x::Vector{Variable}, y): dest[i] = x[i] (copyto!: one (1.0, var) term, constant 0) first
            a = O.AffVec(len(a)).vecadd(a, np.zeros(len(a)))
        return O.AffVec(len(a) if not isinstance(a, O.AffVec) else a.n).vecaddsub(a, b, True)

    terms, consts = [], []
    for t in range(T):
        xt = xvar[t * w:t * w + nx]
        if t == 0:
            rec = sub(xt, h[1, 0])
        else:
            xm, um = xvar[(t - 1) * w:(t - 1) * w + nx], xvar[(t - 1) * w + nx:t * w]
            rec = sub(sub(sub(xt, O.AffVec(nx).matvecmul_vars(A[t - 1], xm)), O.AffVec(nx).matvecmul_vars(Bm[t - 1], um)), h[1, t])
        tt, cc = rec.moi(varmap)
        terms.append(tt.view(np.int64))
        consts.append(cc)
    section = V.section_reference(At, Bt, h, -1, -1, -1)[1]
    got_t, got_c = V.expanded_reference(section, T, nx, nu, 1, xvar, varmap)
    assert np.array_equal(got_t, np.concatenate(terms))
    assert np.array_equal(V.bits(got_c), V.bits(np.concatenate(consts)))


@pytest.mark.parametrize("T,nx,nu", SHAPES + [(3, 17, 15)])
def test_equal_matrices_per_stage_give_the_time_invariant_section_block_by_block(T, nx, nu):
    rng = np.random.default_rng(T + nx + nu)
    At1, Bt1, h = D.dyn_data(3, T, nx, nu, rng)
    At = np.repeat(At1[:, None], T - 1, axis=1)
    Bt = np.repeat(Bt1[:, None], T - 1, axis=1)
    for signs in ((-1, -1, -1), (1, -1, 0), (-1, 1, 1)):
        tv, ti = V.section_reference(At, Bt, h, *signs), D.section_reference(At1, Bt1, h, *signs)
        sv, si = V.sections(T, nx, nu), D.sections(T, nx, nu)
        assert len(sv["AB"]) == T - 1
        for blk in sv["AB"]:
            assert np.array_equal(V.bits(tv[:, blk]), V.bits(ti[:, si["AB"]]))
        assert np.array_equal(V.bits(tv[:, sv["hconst"]]), V.bits(ti[:, si["hconst"]]))
        assert tv.shape[1] == sv["hconst"].stop


def test_section_layout_is_host_arithmetic(lib):
    L = lib.load()
    dim, tmax = _limits()
    from parametron_jl_amd import batch as PB
    for T, nx, nu in ((1, 1, 0), (1, 3, 2), (2, 3, 2), (3, 3, 2), (32, 32, 16), (20, 12, 4), (tmax, dim, dim)):
        sec = V.sections(T, nx, nu)
        Ltv = (T - 1) * nx * (nx + nu) + T * nx
        assert L.pmt_batch_horizon_dynamics_tv_doubles(T, nx, nu) == V.section_doubles(T, nx, nu) == sec["hconst"].stop == Ltv
        off, length = PB.horizon_dynamics_tv_layout(T, nx, nu)
        assert length == Ltv and off == {"AB": [s.start for s in sec["AB"]], "hconst": sec["hconst"].start}
        # one block: the sibling's AB; the blocks and the constants tile the section
        assert Ltv == (T - 1) * D.sections(T, nx, nu)["AB"].stop + T * nx
        assert [0] + [s.stop for s in sec["AB"]] == [s.start for s in sec["AB"]] + [sec["hconst"].start]


def _coeffs(lib, T=3, nx=4, nu=2, B=2, signs=(-1, -1, -1), stride=None, A=FAKE, Bm=FAKE, h=FAKE, out=FAKE):
    stride = V.section_doubles(T, nx, nu) if stride is None else stride
    lib.call(COEFFS, A, Bm, h, B, T, nx, nu, signs[0], signs[1], signs[2], out, stride, None)


def _expand(lib, T=3, nx=4, nu=2, sign_xp=1, section=FAKE, xvar=FAKE, terms=FAKE, consts=FAKE):
    lib.call(EXPAND, section, T, nx, nu, sign_xp, xvar, None, terms, consts, None)


def test_dimension_errors_come_before_any_device_call(lib):
    dim, tmax = _limits()
    assert (dim, tmax) == (128, 512)
    for kw in ({"nx": 0}, {"nx": dim + 1}, {"nu": -1}, {"nu": dim + 1}, {"T": 0}, {"T": tmax + 1}):
        with pytest.raises(lib.DimensionMismatch, match="batch_horizon_dynamics_tv"):
            _coeffs(lib, **kw)
        with pytest.raises(lib.DimensionMismatch, match="batch_horizon_dynamics_tv_expand"):
            _expand(lib, **kw)
    with pytest.raises(lib.DimensionMismatch, match="out_stride"):
        _coeffs(lib, stride=V.section_doubles(3, 4, 2) - 1)
    with pytest.raises(lib.DimensionMismatch, match="out_stride"):       # the time-invariant length is too short from T = 3 on
        _coeffs(lib, stride=D.section_doubles(3, 4, 2))
    with pytest.raises(lib.DimensionMismatch, match="batch_horizon_dynamics_tv"):
        _coeffs(lib, B=-1)


def test_argument_errors_come_before_any_device_call(lib):
    for signs in ((0, -1, -1), (-1, 0, -1), (2, 1, 1), (-1, -1, 2), (1, 1, -2)):
        with pytest.raises(lib.ArgumentError, match="batch_horizon_dynamics_tv"):
            _coeffs(lib, signs=signs)
    for kw in ({"A": None}, {"h": None}, {"Bm": None}, {"out": None}):       # a null A; a null h with sign_h != 0; a null Bm with nu > 0
        with pytest.raises(lib.ArgumentError, match="null pointer"):
            _coeffs(lib, **kw)
    with pytest.raises(lib.ArgumentError, match="null pointer"):             # T == 1 still needs its h and its output
        _coeffs(lib, T=1, A=None, Bm=None, h=None)
    with pytest.raises(lib.ArgumentError, match="null pointer"):
        _coeffs(lib, T=1, A=None, Bm=None, out=None)
    for sign_xp in (0, 2, -2):
        with pytest.raises(lib.ArgumentError, match="sign_xp"):
            _expand(lib, sign_xp=sign_xp)
    for kw in ({"section": None}, {"xvar": None}, {"terms": None}, {"consts": None}):
        with pytest.raises(lib.ArgumentError, match="null pointer"):
            _expand(lib, **kw)


def test_an_empty_batch_is_ok_whatever_the_pointers(lib):
    _coeffs(lib, B=0, A=None, Bm=None, h=None, out=None)
    _coeffs(lib, B=0, A=None, Bm=None, h=None, out=None, T=1, nx=1, nu=0, signs=(1, 1, 0), stride=1)


def test_a_single_stage_needs_no_matrices(lib):
    """T == 1: the constants only, A and Bm may be NULL.  The source's null-pointer test says so, and an empty batch passes validation with
    them; the call that writes such sections runs in the GPU suite (a call with made-up addresses must never reach a launch here)."""
    _coeffs(lib, B=0, T=1, A=None, Bm=None)
    src = open(os.path.join(ROOT, "parametron.jl_amd", "csrc", "batch_horizon_ltv.hip")).read()
    assert 'PMT_REQUIRE(out && (T == 1 || (A && (nu == 0 || Bm))) && (sign_h == 0 || h), PMT_INVALID_ARGUMENT' in src


def test_bindings_and_julia_wrappers_name_the_entry_points(lib):
    jl = open(os.path.join(ROOT, "julia", "ParametronHIP.jl")).read()
    raw = C.CDLL(lib.LIB_PATH)
    for name in (COEFFS, EXPAND, DOUBLES):
        assert "(:%s, lib)" % name in jl and name in lib.SIGNATURES and hasattr(raw, name)
