"""CPU-only: the batch of horizons' compact dynamics sections (pmt_batch_horizon_dynamics_f64, pmt_batch_horizon_dynamics_expand_f64).  The
numpy restatement of the header's contract (batch_horizon_dyn_util) against its anchor — affine_stages_util's restatement of
pmt_affine_stages_f64 on the instance's own tables, word for word on integer views — and against the oracle's vecadd! / vecsubtract!
chain and MOI copy for the spelling x+ - A*x - B*u - w; the section's length; both entry points' argument errors through the C ABI, which
need no GPU because validation precedes any device call."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import affine_stages_util as U
import batch_horizon_dyn_util as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COEFFS, EXPAND, DOUBLES = "pmt_batch_horizon_dynamics_f64", "pmt_batch_horizon_dynamics_expand_f64", "pmt_batch_horizon_dynamics_doubles"
FAKE = C.c_void_p(64)                       # never dereferenced: the calls below are rejected first, or have nothing to do
POISON = -7


@pytest.fixture(scope="module")
def lib():
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


def _limits():
    hdr = open(os.path.join(ROOT, "include", "parametron_hip.h")).read()
    return tuple(int(re.search(r"#define %s\s+(\d+)" % name, hdr).group(1)) for name in ("PMT_BATCH_HORIZON_MAX_DIM", "PMT_BATCH_HORIZON_MAX_T"))


def _instance(T, nx, nu, seed):
    """one instance (index 1 of three) with its variables and a permuted varmap"""
    rng = np.random.default_rng(seed)
    At, Bt, h = D.dyn_data(3, T, nx, nu, rng)
    h[1, 0, 0], h[1, -1, -1] = -0.0, 0.0
    n = T * (nx + nu)
    xvar = np.sort(rng.choice(np.arange(1, n + 10), n, replace=False)).astype(np.int64)
    varmap = (rng.permutation(n + 9) + 1 + 100).astype(np.int64)
    return At, Bt, h, xvar, varmap


def _check_against_the_tables(T, nx, nu, signs, seed=0):
    sign_xp, sign_a, sign_b, sign_h = signs
    At, Bt, h, xvar, varmap = _instance(T, nx, nu, seed + 100 * T + 10 * nx + nu)
    section = D.section_reference(At, Bt, h, sign_a, sign_b, sign_h)[1]
    assert section.shape == (D.section_doubles(T, nx, nu),)
    stages, nterms, nconsts = D.instance_stages(At[1].T, Bt[1].T, h[1], sign_xp, sign_a, sign_b, sign_h, xvar)
    assert (nterms, nconsts) == (D.term_count(T, nx, nu), T * nx)
    for vmap in (varmap, None):
        terms, consts = D.expanded_reference(section, T, nx, nu, sign_xp, xvar, vmap)
        want_t, want_c = U.images(stages, vmap, nterms, nconsts, POISON)
        assert np.array_equal(terms, want_t), (T, nx, nu, signs)
        assert np.array_equal(D.bits(consts), D.bits(want_c)), (T, nx, nu, signs)
    return section


@pytest.mark.parametrize("T,nx,nu", [(1, 3, 2), (2, 1, 0), (3, 3, 2), (3, 65, 10)])
def test_restated_expansion_equals_the_stage_tables_word_for_word(T, nx, nu):
    for signs in ((1, -1, -1, -1), (-1, 1, 1, 1)):
        _check_against_the_tables(T, nx, nu, signs)


@pytest.mark.parametrize("signs", list(itertools.product((1, -1), (1, -1), (1, -1), (-1, 0, 1))), ids=lambda s: "%+d%+d%+d%+d" % s)
def test_all_24_sign_combinations(signs):
    T, nx, nu = 3, 3, 2
    section = _check_against_the_tables(T, nx, nu, signs, seed=7)
    # not vacuous: zeros of both signs among the AB words, none negative among the constants
    sec = D.sections(T, nx, nu)
    ab, hc = section[sec["AB"]], section[sec["hconst"]]
    assert np.any(np.signbit(ab[ab == 0.0])) and np.any(~np.signbit(ab[ab == 0.0]))
    assert not np.any(np.signbit(hc[hc == 0.0])) and np.any(hc == 0.0)
    assert np.all(D.bits(hc) == 0) == (signs[3] == 0)


def test_restatement_equals_the_oracle_chain():
    """x_0 - h_0 and x_t - A*x_{t-1} - B*u_{t-1} - h_t through the oracle: matvecmul! per product, vecsubtract! per -, and
    update!(::MOI.VectorAffineFunction, fs, varmap); every word on integer views"""
    entry.build()
    from oracle import oracle as O
    T, nx, nu = 3, 3, 2
    w = nx + nu
    At, Bt, h, xvar, varmap = _instance(T, nx, nu, 11)
    A, Bm = At[1].T, Bt[1].T

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
            rec = sub(sub(sub(xt, O.AffVec(nx).matvecmul_vars(A, xm)), O.AffVec(nx).matvecmul_vars(Bm, um)), h[1, t])
        tt, cc = rec.moi(varmap)
        terms.append(tt.view(np.int64))
        consts.append(cc)
    section = D.section_reference(At, Bt, h, -1, -1, -1)[1]
    got_t, got_c = D.expanded_reference(section, T, nx, nu, 1, xvar, varmap)
    assert np.array_equal(got_t, np.concatenate(terms))
    assert np.array_equal(D.bits(got_c), D.bits(np.concatenate(consts)))


def test_section_length_is_host_arithmetic(lib):
    L = lib.load()
    dim, tmax = _limits()
    for T, nx, nu in ((1, 1, 0), (3, 3, 2), (32, 32, 16), (20, 12, 4), (tmax, dim, dim)):
        off = D.sections(T, nx, nu)
        assert L.pmt_batch_horizon_dynamics_doubles(T, nx, nu) == D.section_doubles(T, nx, nu) == off["hconst"].stop == nx * (nx + nu) + T * nx
        from parametron_jl_amd import batch as PB
        assert PB.horizon_dynamics_layout(T, nx, nu) == ({"AB": 0, "hconst": off["hconst"].start}, D.section_doubles(T, nx, nu))


def _coeffs(lib, T=3, nx=4, nu=2, B=2, signs=(-1, -1, -1), stride=None, A=FAKE, Bm=FAKE, h=FAKE, out=FAKE):
    stride = D.section_doubles(T, nx, nu) if stride is None else stride
    lib.call(COEFFS, A, Bm, h, B, T, nx, nu, signs[0], signs[1], signs[2], out, stride, None)


def _expand(lib, T=3, nx=4, nu=2, sign_xp=1, section=FAKE, xvar=FAKE, terms=FAKE, consts=FAKE):
    lib.call(EXPAND, section, T, nx, nu, sign_xp, xvar, None, terms, consts, None)


def test_dimension_errors_come_before_any_device_call(lib):
    dim, tmax = _limits()
    assert (dim, tmax) == (128, 512)
    for kw in ({"nx": 0}, {"nx": dim + 1}, {"nu": -1}, {"nu": dim + 1}, {"T": 0}, {"T": tmax + 1}):
        with pytest.raises(lib.DimensionMismatch, match="batch_horizon_dynamics"):
            _coeffs(lib, **kw)
        with pytest.raises(lib.DimensionMismatch, match="batch_horizon_dynamics_expand"):
            _expand(lib, **kw)
    with pytest.raises(lib.DimensionMismatch, match="out_stride"):
        _coeffs(lib, stride=D.section_doubles(3, 4, 2) - 1)
    with pytest.raises(lib.DimensionMismatch, match="batch_horizon_dynamics"):
        _coeffs(lib, B=-1)


def test_argument_errors_come_before_any_device_call(lib):
    for signs in ((0, -1, -1), (-1, 0, -1), (2, 1, 1), (-1, -1, 2), (1, 1, -2)):
        with pytest.raises(lib.ArgumentError, match="batch_horizon_dynamics"):
            _coeffs(lib, signs=signs)
    for kw in ({"A": None}, {"h": None}, {"Bm": None}, {"out": None}):       # a null A; a null h with sign_h != 0; a null Bm with nu > 0
        with pytest.raises(lib.ArgumentError, match="null pointer"):
            _coeffs(lib, **kw)
    for sign_xp in (0, 2, -2):
        with pytest.raises(lib.ArgumentError, match="sign_xp"):
            _expand(lib, sign_xp=sign_xp)
    for kw in ({"section": None}, {"xvar": None}, {"terms": None}, {"consts": None}):
        with pytest.raises(lib.ArgumentError, match="null pointer"):
            _expand(lib, **kw)


def test_an_empty_batch_is_ok_whatever_the_pointers(lib):
    _coeffs(lib, B=0, A=None, Bm=None, h=None, out=None)
    _coeffs(lib, B=0, A=None, Bm=None, h=None, out=None, T=1, nx=1, nu=0, signs=(1, 1, 0), stride=2)


def test_bindings_and_julia_wrappers_name_the_entry_points(lib):
    jl = open(os.path.join(ROOT, "julia", "ParametronHIP.jl")).read()
    raw = C.CDLL(lib.LIB_PATH)
    for name in (COEFFS, EXPAND, DOUBLES):
        assert "(:%s, lib)" % name in jl and name in lib.SIGNATURES and hasattr(raw, name)
