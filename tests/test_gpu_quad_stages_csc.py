"""-m gpu: horizon stage costs as the CSC values of P (pmt_quad_stages_csc_f64), at the C ABI.

Every comparison is bit for bit against an existing entry point on the same device data: a single stage against the out_P_values, linear
terms and constant of pmt_quad_form_f64 / pmt_quad_form_shift_f64 with the same alpha; a mixed table against pmt_quad_stages_diag_f64 on
the same tables with MOI slices, coefficient tri(j,k) <-> value k(k+1)/2 + j.  The outputs are pre-filled with poison: the WHOLE images are
compared, so gaps and margins must be untouched and every slice word overwritten."""
import ctypes as C
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from parametron_jl_amd import _lib  # noqa: E402
import quad_stages_diag_util as D  # noqa: E402
import quad_stages_terms_util as W  # noqa: E402
import quad_stages_util as U  # noqa: E402
import test_gpu_quad_stages as G  # noqa: E402
import test_gpu_quad_stages_diag as GD  # noqa: E402
from gpu_util import DEV, Guarded, ptr, stream  # noqa: E402

QT = _lib.QT
bits = G.bits
SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 200, 256]
SIGN_BIT = np.int64(-2 ** 63)


def upload(arr):
    return torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()).to(DEV)


def nvalues_of(st):
    return D.nquad(st)


def place_values(stages, order, gaps):
    """value slices one behind the other in `order`, gaps[i] doubles in front of the i-th slice (and the last gap behind the last one)
    -> (val_at per stage, nvalues)"""
    at, pos = [0] * len(stages), 0
    for i, t in enumerate(order):
        at[t] = pos + gaps[i % len(gaps)]
        pos = at[t] + nvalues_of(stages[t])
    return at, pos + gaps[len(order) % len(gaps)]


def csc_launch(L, val_at, nvalues, alpha=1.0, shift=0):
    """pmt_quad_stages_csc_f64 over the device tables of a test_gpu_quad_stages_diag.Launch, the stage table with quad_at = val_at,
    through pmt_quad_stages_csc_check, into guarded (poisoned) outputs"""
    adr = lambda a: C.addressof(a) if a is not None else None
    rows = [dict(r, quad_at=int(a)) for r, a in zip(L.rows, val_at)]
    arr = _lib.quad_stages(rows)
    _lib.call("pmt_quad_stages_csc_check", adr(arr), adr(L.tarr), adr(L.darr), L.T, adr(L.carr), len(L.cvals), nvalues, L.nlin)
    out = types.SimpleNamespace(table=upload(arr), rows=rows, nvalues=nvalues, values=Guarded(nvalues, doubles=True, shift=shift),
                                lin=Guarded(2 * L.nlin, shift=shift), consts=Guarded(L.T, doubles=True), const=Guarded(1, doubles=True))
    out.run = lambda: _lib.call("pmt_quad_stages_csc_f64", ptr(out.table), ptr(L.ttable), ptr(L.dtable), L.T, ptr(L.ctable), len(L.cvals),
                                ptr(L.dvm), alpha, out.values.ptr(), out.lin.ptr(), out.consts.ptr(), out.const.ptr(), stream())
    out.run()
    return out


def unit(stages):
    """unit rows beside the stages: weight 1, no linear term, no rider"""
    for st in stages:
        st.update(W=(1.0, None), lin=None, diag=None)
    return stages


def check_against_the_nodes_alone(L, out, alpha):
    """every stage's value slice, linear terms and constant against pmt_quad_form_f64 / pmt_quad_form_shift_f64 for that stage alone with
    the same alpha (moi = 1: the same index words); the references are written into one buffer each and fetched once.  Whole images:
    the words around the slices hold the poison."""
    T = L.T
    ref_at, pos = [], 0
    for r in out.rows:                                                    # (the references' slices start on 16-byte boundaries)
        ref_at.append(pos)
        pos += (r["n"] * (r["n"] + 1) // 2 + 1) & ~1
    rv = torch.full((max(pos, 1),), np.nan, dtype=torch.float64, device=DEV)
    rl = torch.full((2 * L.nlin,), -7, dtype=torch.int64, device=DEV)
    rc = torch.full((T,), np.nan, dtype=torch.float64, device=DEV)
    nmax = max(r["n"] for r in out.rows)
    ws = torch.full((int(_lib.load().pmt_quad_form_shift_workspace_bytes(nmax)) // 8 + 2,), np.nan, dtype=torch.float64, device=DEV)
    for t, r in enumerate(out.rows):
        n = r["n"]
        pv, pl, pc = C.c_void_p(rv.data_ptr() + 8 * ref_at[t]), C.c_void_p(rl.data_ptr() + 16 * r["lin_at"]), C.c_void_p(rc.data_ptr() + 8 * t)
        if r["sign"]:
            _lib.call("pmt_quad_form_shift_f64", C.c_void_p(r["Q"]), r["ldq"], n, C.c_void_p(r["xvar"]), C.c_void_p(r["vec"]), r["sign"], 1,
                      ptr(L.dvm), alpha, None, pv, pl, pc, ptr(ws), stream())
        else:
            _lib.call("pmt_quad_form_f64", C.c_void_p(r["Q"]), r["ldq"], n, C.c_void_p(r["xvar"]), 1, ptr(L.dvm), alpha, None, pv, pl, pc, stream())
    torch.cuda.synchronize()
    rv, rl, rc = rv.cpu().numpy(), rl.cpu().numpy(), rc.cpu().numpy()
    image = out.values.padding(out.nvalues)
    for t, r in enumerate(out.rows):
        nv = r["n"] * (r["n"] + 1) // 2
        assert not np.any(np.isnan(rv[ref_at[t]:ref_at[t] + nv]))           # (the data holds no NaN: the poison cannot pass for a value)
        image[r["quad_at"]:r["quad_at"] + nv] = rv[ref_at[t]:ref_at[t] + nv]
    assert not np.any(np.isnan(rc)) and not np.any(rl == -7)
    out.values.check(image, "P's values against the nodes alone")
    out.lin.check(rl, "linear terms against the nodes alone")
    out.consts.check(rc, "stage constants against the nodes alone")
    out.const.check(np.array([W.function_constant(rc, L.cvals)]), "constant")


# ------------------------------------------------------------------ 1. single stages
@pytest.mark.parametrize("n", SIZES)
def test_a_single_stage_equals_the_form_nodes_values(n):
    """plain, +v and -v; ldq = n and n + 3; alpha 1.0 and -1.0; unit terms; the slice starts one double into the buffer, on both parities
    of the 16-byte boundary, with two doubles of margin behind it"""
    case = 0
    for sign in (0, 1, -1):
        stages, varmap, nterms, nlin = U.make_stages([n], [sign], 700 + n + sign, special=True)
        unit(stages)
        for pad in (0, 3):
            L = GD.Launch(stages, [], varmap, nterms, nlin, pad=pad, diags=False)
            assert L.rows[0]["ldq"] == n + pad
            for alpha in (1.0, -1.0):
                out = csc_launch(L, [1], n * (n + 1) // 2 + 3, alpha=alpha, shift=case & 1)
                check_against_the_nodes_alone(L, out, alpha)
                case += 1


# ------------------------------------------------------------------ 2. a mixed table against the MOI launch
KINDS = ["f-", "i0", "f0r0", "i-", "f+r-", "f0", "i+", "f-r+", "f0r+", "i0", "f+", "f-r0", "i-"]
WEIGHTS = GD.MIXED + [(0.0, None), (2.0, 0.0)]


def mixed_table():
    T = 23
    ns = [SIZES[t % len(SIZES)] for t in range(T)]
    kinds = [KINDS[t % len(KINDS)] for t in range(T)]
    stages, varmap, nterms, nlin = D.make_stages(ns, kinds, 2300, weights=WEIGHTS, shared=1)
    nterms, nlin = D.place(stages, [t % 3 for t in range(T)] + [1])
    return stages, varmap, nterms, nlin, W.make_consts(3)


def test_the_mixed_table_covers_what_it_should():
    stages, _, _, _, consts = mixed_table()
    forms = [st for st in stages if not D.is_identity(st)]
    uses = {}
    for st in forms:
        uses[id(st["Q"])] = uses.get(id(st["Q"]), 0) + 1
    assert sum(1 for c in uses.values() if c >= 2) >= 3                    # matrices shared among the form stages
    ws = [st["W"] for st in stages]
    assert any(w[1] is None for w in ws) and any(w[1] is not None for w in ws) and any(W.weight(w) < 0 for w in ws)
    assert any(W.weight(w) == 0.0 and w[1] is None for w in ws) and any(W.weight(w) == 0.0 and w[1] is not None for w in ws)
    assert any(st["lin"] is not None for st in stages) and any(st["lin"] is None for st in stages)
    riders = [D.rider(st) for st in forms if D.rider(st) is not None]
    assert any(d[3] for d in riders) and any(not d[3] for d in riders) and any(D.rider(st) is None for st in forms)
    ident = [st for st in stages if D.is_identity(st)]
    assert any(st["sign"] for st in ident) and any(not st["sign"] for st in ident)
    assert sorted({len(st["xvar"]) for st in stages}) == SIZES and len(consts) == 3
    assert not any(np.any(np.isnan(np.asarray(st["Q"]))) for st in forms)


@pytest.mark.parametrize("alpha", [1.0, -1.0])
def test_a_mixed_table_equals_the_moi_launch_coefficient_for_value(alpha):
    stages, varmap, nterms, nlin, consts = mixed_table()
    T = len(stages)
    L = GD.Launch(stages, consts, varmap, nterms, nlin).run()
    quad, lin, sconsts, const = L.host()
    coeff = quad.view(QT)["coeff"]
    assert not np.any(np.isnan(coeff[np.concatenate([np.arange(st["quad_at"], st["quad_at"] + D.nquad(st)) for st in stages])]))
    order = np.random.default_rng(23).permutation(T).tolist()
    val_at, nvalues = place_values(stages, order, [1, 0, 2, 1, 3, 0, 1])
    assert any(a & 1 for a in val_at) and any(not a & 1 for a in val_at) and order != sorted(order)
    for shift in (0, 1):
        out = csc_launch(L, val_at, nvalues, alpha=alpha, shift=shift)
        image = out.values.padding(nvalues)
        for st, at in zip(stages, val_at):
            n = len(st["xvar"])
            c = coeff[st["quad_at"]:st["quad_at"] + D.nquad(st)]
            if D.is_identity(st):
                vals = c
            else:
                j, k = np.triu_indices(n)                                   # row-major upper triangle: tri(j,k) in ascending order
                vals = np.empty(len(c))
                vals[k * (k + 1) // 2 + j] = c
            if alpha == -1.0:                                             # one more IEEE multiply by -1.0: the sign bit flips
                vals = (bits(vals) ^ SIGN_BIT).view(np.float64)
            image[at:at + len(vals)] = vals
        out.values.check(image, "P's values against the MOI launch's coefficients")
        out.lin.check(lin, "linear terms")
        out.consts.check(sconsts, "stage constants")
        out.const.check(np.array([const]), "constant")


# ------------------------------------------------------------------ 3. more stages than workgroups
def test_more_stages_than_the_grid_holds():
    """3 CUs + 5 stages of n = 5 and a last one of n = 256: the persistent loop wraps, and the constant's chains hold more than one stage"""
    T = 3 * G.cu_count() + 5
    ns = [5] * T + [256]
    stages, varmap, nterms, nlin = U.make_stages(ns, [(-1, 0, 1)[t % 3] for t in range(T + 1)], 3000, shared=3)
    unit(stages)
    L = GD.Launch(stages, [], varmap, nterms, nlin, diags=False)
    val_at, nvalues = place_values(stages, list(range(T + 1)), [1, 0, 2])
    for alpha in (1.0, -1.0):
        out = csc_launch(L, val_at, nvalues, alpha=alpha)
        check_against_the_nodes_alone(L, out, alpha)
    assert T + 1 > 256


# ------------------------------------------------------------------ 4. no stage; determinism
def test_no_stage_writes_the_constants_only():
    """T == 0: *out_const = the constants added onto 0.0 in table order and nothing else, whatever the other pointers"""
    consts = [(3.0, None, 0.7), (-0.5, 1.25, None), (1.0, None, None)]
    keep = [torch.tensor([x], dtype=torch.float64, device=DEV) for x in (0.7, 1.25)]
    carr = _lib.quad_stage_consts([{"scale": 3.0, "value": keep[0].data_ptr()}, {"scale": -0.5, "weight": keep[1].data_ptr()}, {"scale": 1.0}])
    ctable = upload(carr)
    values, lin, const = Guarded(6, doubles=True), Guarded(4), Guarded(1, doubles=True)
    for nc in (3, 0):
        _lib.call("pmt_quad_stages_csc_f64", None, None, None, 0, ptr(ctable), nc, None, -1.0, values.ptr(), lin.ptr(), None, const.ptr(), stream())
        values.check(values.padding(6), "P's values")
        lin.check(lin.padding(4), "linear terms")
        const.check(np.array([W.function_constant([], consts[:nc])]), "constant")
    assert W.function_constant([], consts) == ((0.0 + 3.0 * 0.7) + (-0.5 * 1.25) * 1.0) + 1.0


def test_two_calls_give_equal_bits():
    stages, varmap, nterms, nlin, consts = mixed_table()
    L = GD.Launch(stages, consts, varmap, nterms, nlin)
    val_at, nvalues = place_values(stages, list(range(len(stages)))[::-1], [1, 2, 0])
    out = csc_launch(L, val_at, nvalues, alpha=-1.0)
    host = lambda: [g.buf.cpu().numpy().view(np.int64).copy() for g in (out.values, out.lin, out.consts, out.const)]
    torch.cuda.synchronize()
    first = host()
    out.run()                                                             # a second call over the first one's outputs
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(first, host()))
