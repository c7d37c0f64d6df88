"""CPU-only: the canonical quadratic-form entry point (pmt_quad_form_f64) is exported, bound in Python and Julia, validates its arguments
before any device call, and the numpy restatement the GPU tests use equals the oracle's bilinearmul -> canonicalize -> MOI copy bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000            # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def lib():
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


def restate_form(Q, xvar, varmap=None, moi=1):
    """transpose(x) * Q * x as its canonical function: (coeff, row, col) on the row-major upper triangle.  Q[j,k] + Q[k,j] off the
    diagonal, Q[j,j] on it (doubled by the MOI copy); indices through varmap (1-based optimizer index of Variable k at varmap[k-1])."""
    Q = np.asarray(Q, dtype=np.float64)
    xvar = np.asarray(xvar, dtype=np.int64)
    n = Q.shape[0]
    iu = np.triu_indices(n)
    coeff = Q[iu] + Q.T[iu]
    on = iu[0] == iu[1]
    coeff[on] = 2 * Q[iu][on] if moi else Q[iu][on]
    v = xvar if (varmap is None or not moi) else np.asarray(varmap, dtype=np.int64)[xvar - 1]
    return coeff, v[iu[0]], v[iu[1]]


def _call(lib, Q=FAKE, ldq=8, n=8, xvar=FAKE, moi=1, varmap=FAKE, alpha=1.0, quad=FAKE, values=FAKE, lin=FAKE, const=FAKE):
    lib.call("pmt_quad_form_f64", Q, ldq, n, xvar, moi, varmap, alpha, quad, values, lin, const, None)


def test_form_entry_point_is_exported_and_bound(lib):
    raw = C.CDLL(lib.LIB_PATH)
    assert hasattr(raw, "pmt_quad_form_f64")
    assert "pmt_quad_form_f64" in lib.SIGNATURES
    assert len(lib.SIGNATURES["pmt_quad_form_f64"][1]) == 12
    src = open(os.path.join(ROOT, "julia", "ParametronHIP.jl")).read()
    assert re.search(r"ccall\(\(:pmt_quad_form_f64, lib\)", src)
    hdr = open(os.path.join(ROOT, "include", "parametron_hip.h")).read()
    assert re.search(r"int pmt_quad_form_f64\(const double \*Q, int64_t ldq, int64_t n, const int64_t \*xvar", hdr)


@pytest.mark.parametrize("bad", [
    {"Q": None}, {"xvar": None}, {"n": 0}, {"n": -3}, {"ldq": 7}, {"moi": 1, "varmap": None}, {"quad": None, "values": None},
], ids=["null-Q", "null-xvar", "n-zero", "n-negative", "ldq-below-n", "moi-without-varmap", "no-output"])
def test_form_rejects_bad_arguments(lib, bad):
    with pytest.raises(lib.ArgumentError) as e:
        _call(lib, **bad)
    assert "quad_form" in str(e.value)                    # the message comes through pmt_last_error


@pytest.mark.parametrize("n", [1, 2, 37, 130])
@pytest.mark.parametrize("moi", [0, 1])
def test_restatement_equals_the_oracle(n, moi):
    from oracle import oracle as O
    rng = np.random.default_rng(17 * n + moi)
    Q = rng.standard_normal((n, n))
    if n > 2:
        Q[1, 2], Q[2, 1] = 0.75, -0.75                    # an equal-and-opposite pair stays as a +0.0 coefficient: canonicalize! does not prune
        Q[0, 0] = -0.0
    nvars = n + 5
    xvar = np.sort(rng.choice(np.arange(1, nvars + 1), n, replace=False)).astype(np.int64)
    varmap = (rng.permutation(nvars) + 11).astype(np.int64)
    f = O.Quad().bilinearmul(Q, xvar, xvar).canonicalize()
    if moi:
        at, qt, const = f.moi(varmap)
        assert len(at) == 0 and const == 0.0
    else:
        qt = f.terms()
    coeff, row, col = restate_form(Q, xvar, varmap, moi)
    assert len(qt) == n * (n + 1) // 2
    assert np.array_equal(qt["row"], row) and np.array_equal(qt["col"], col)
    assert np.array_equal(qt["coeff"].view(np.int64), coeff.view(np.int64))
