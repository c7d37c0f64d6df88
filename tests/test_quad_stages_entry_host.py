"""CPU-only: every refusal of the four stage-cost checks (pmt_quad_stages_check, _terms_check, _diag_check, _csc_check) and of the four entry
points (pmt_quad_stages_f64, _terms_f64, _diag_f64, _csc_f64), with the exact exception class and the full message text as literals — the
stage-table messages say `quad_stages:`, the side-table messages `quad_stages_terms:`, the rider messages `quad_stages_diag:` whichever check
is called, an entry point's messages carry its own name —, the cases a check accepts, and cases with two things wrong at once: the order
is counts, stage table, slices, side tables, riders.  Every entry-point call here is refused before any device call."""
import ctypes as C

import pytest

import __graft_entry__ as entry
from test_record_tape_host import FAKE

KINDS = ("plain", "terms", "diag", "csc")
CHECK = {"plain": "pmt_quad_stages_check", "terms": "pmt_quad_stages_terms_check", "diag": "pmt_quad_stages_diag_check",
         "csc": "pmt_quad_stages_csc_check"}
SIDE, RIDERS = KINDS[1:], KINDS[2:]                                       # the checks that take side tables / a rider table
A, D = "ArgumentError", "DimensionMismatch"


@pytest.fixture(scope="module")
def lib():
    entry.build()
    from parametron_jl_amd import _lib
    return _lib


# ---- 1. the four checks
def _tables(lib, edit=None, dedit=None):
    """three form stages of n = 3, 4, 5, the first and the last shifted, their slices one behind the other; a term row and a rider row per
    stage (riders on stages 0 and 2, the first with a vector); two constants"""
    rows, qa, la = [], 0, 0
    for t in range(3):
        n = 3 + t
        rows.append({"Q": FAKE, "ldq": n, "xvar": FAKE, "vec": FAKE if t % 2 == 0 else None, "n": n, "sign": -1 if t % 2 == 0 else 0,
                     "quad_at": qa, "lin_at": la})
        qa, la = qa + n * (n + 1) // 2, la + n
    for (t, field), value in (edit or {}).items():
        rows[t][field] = value
    drows = [{"scale": 2.0, "vec": FAKE, "sign": 1}, {}, {"weight": FAKE}]
    for (t, field), value in (dedit or {}).items():
        drows[t] = dict(drows[t], **{field: value})
    terms = lib.quad_stage_terms([{"scale": 0.5}, {"weight": FAKE, "lin_vec": FAKE, "lin_scale": -1.0}, {"lin_vec": FAKE, "lin_weight": FAKE}])
    consts = lib.quad_stage_consts([{"scale": 2.0}, {"value": FAKE, "weight": FAKE}])
    return {"stages": lib.quad_stages(rows), "terms": terms, "diags": lib.quad_stage_diags(drows), "consts": consts}, qa, la


def _check(lib, kind, edit=None, dedit=None, null=(), T=3, nconsts=2, dq=0, dl=0):
    """the check of `kind` over _tables with the stage fields `edit` and the rider fields `dedit` replaced, the tables named in `null` passed as
    NULL, and nterms / nlin `dq` / `dl` beside what the unedited slices need (6 + 10 + 15 quadratic, 3 + 4 + 5 linear terms)"""
    tab, nq, nl = _tables(lib, edit, dedit)
    assert (nq, nl) == (31, 12)
    s, t, d, c = (None if k in null else C.addressof(tab[k]) for k in ("stages", "terms", "diags", "consts"))
    args = {"plain": (s, T), "terms": (s, t, T, c, nconsts), "diag": (s, t, d, T, c, nconsts), "csc": (s, t, d, T, c, nconsts)}[kind]
    lib.call(CHECK[kind], *args, nq + dq, nl + dl)


STAGE = lambda t: " (stage %d)" % t
QUAD_SLICES = "quad_stages: quadratic slices overlap or leave [0, nterms)"
LIN_SLICES = "quad_stages: linear slices overlap or leave [0, nlin)"
NCONSTS = "quad_stages_terms: nconsts outside 0 .. 32"
NULL_CONSTS = "quad_stages_terms: null table of constants"
NULL_TERMS = "quad_stages_terms: null table of stage terms"

# (id, the checks it goes through, _check's arguments, the exception class, the message); None, None: accepted
CHECKS = [
    # counts
    ("T-negative", KINDS, dict(T=-1), D, "quad_stages: negative stage count"),
    ("nterms-negative", KINDS, dict(dq=-32), D, "quad_stages: negative term count"),
    ("nlin-negative", KINDS, dict(dl=-13), D, "quad_stages: negative term count"),
    ("nterms-negative-T0", KINDS, dict(T=0, dq=-32), D, "quad_stages: negative term count"),
    # the stage table
    ("null-table", KINDS, dict(null=("stages",)), A, "quad_stages: null stage table"),
    ("null-matrix", KINDS[:2], dict(edit={(1, "Q"): None}), A, "quad_stages: null matrix" + STAGE(1)),
    ("null-matrix-is-an-identity-stage", RIDERS, dict(edit={(1, "Q"): None}), None, None),
    ("null-matrix-ldq-not-looked-at", RIDERS, dict(edit={(1, "Q"): None, (1, "ldq"): -7}), None, None),
    ("null-xvar", KINDS, dict(edit={(2, "xvar"): None}), A, "quad_stages: null variable indices" + STAGE(2)),
    ("sign-two", KINDS, dict(edit={(0, "sign"): 2}), A, "quad_stages: sign must be -1, 0 or +1" + STAGE(0)),
    ("sign-minus-two", KINDS, dict(edit={(1, "sign"): -2}), A, "quad_stages: sign must be -1, 0 or +1" + STAGE(1)),
    ("shifted-without-vector", KINDS, dict(edit={(1, "sign"): 1}), A, "quad_stages: a shifted stage without its vector" + STAGE(1)),
    ("shifted-vector-removed", KINDS, dict(edit={(2, "vec"): None}), A, "quad_stages: a shifted stage without its vector" + STAGE(2)),
    ("n-zero", KINDS, dict(edit={(1, "n"): 0}), D, "quad_stages: n outside 1 .. 256" + STAGE(1)),
    ("n-257", KINDS, dict(edit={(1, "n"): 257, (1, "ldq"): 300}, dq=40000, dl=400), D, "quad_stages: n outside 1 .. 256" + STAGE(1)),
    ("identity-n-257", RIDERS, dict(edit={(1, "Q"): None, (1, "n"): 257}, dq=400, dl=400), D, "quad_stages: n outside 1 .. 256" + STAGE(1)),
    ("ldq-below-n", KINDS, dict(edit={(2, "ldq"): 4}), D, "quad_stages: ldq < n" + STAGE(2)),
    ("quad-slice-below-zero", KINDS, dict(edit={(0, "quad_at"): -1}), D, "quad_stages: a slice starts below 0" + STAGE(0)),
    ("lin-slice-below-zero", KINDS, dict(edit={(1, "lin_at"): -1}), D, "quad_stages: a slice starts below 0" + STAGE(1)),
    # the slices
    ("quad-overlap-by-one", KINDS, dict(edit={(1, "quad_at"): 5}), D, QUAD_SLICES),
    ("quad-leaves-the-total", KINDS, dict(dq=-1), D, QUAD_SLICES),
    ("lin-overlap-by-one", KINDS, dict(edit={(2, "lin_at"): 6}), D, LIN_SLICES),
    ("lin-leaves-the-total", KINDS, dict(dl=-1), D, LIN_SLICES),
    ("identity-counts-n-terms", RIDERS, dict(edit={(1, "Q"): None, (2, "quad_at"): 10}, dq=-6), None, None),
    ("identity-counts-n-terms-overlap-by-one", RIDERS, dict(edit={(1, "Q"): None, (2, "quad_at"): 9}), D, QUAD_SLICES),
    ("identity-counts-n-terms-leaves-the-total", RIDERS, dict(edit={(1, "Q"): None, (2, "quad_at"): 10}, dq=-7), D, QUAD_SLICES),
    ("room-to-spare", KINDS, dict(dq=5, dl=2), None, None),
    # the side tables
    ("null-terms", SIDE, dict(null=("terms",)), A, NULL_TERMS),
    ("nconsts-minus-one", SIDE, dict(nconsts=-1), D, NCONSTS),
    ("nconsts-33", SIDE, dict(nconsts=33), D, NCONSTS),
    ("null-consts-nconsts-1", SIDE, dict(null=("consts",), nconsts=1), A, NULL_CONSTS),
    ("null-consts-nconsts-0", SIDE, dict(null=("consts",), nconsts=0), None, None),
    # the riders
    ("present-two", RIDERS, dict(dedit={(0, "present"): 2}), A, "quad_stages_diag: present must be 0 or 1" + STAGE(0)),
    ("present-negative", RIDERS, dict(dedit={(1, "present"): -1}), A, "quad_stages_diag: present must be 0 or 1" + STAGE(1)),
    ("rider-on-identity", RIDERS, dict(edit={(1, "Q"): None}, dedit={(1, "present"): 1}), A, "quad_stages_diag: a rider on an identity stage" + STAGE(1)),
    ("rider-sign-two", RIDERS, dict(dedit={(0, "sign"): 2}), A, "quad_stages_diag: sign must be -1, 0 or +1" + STAGE(0)),
    ("rider-sign-minus-two", RIDERS, dict(dedit={(2, "sign"): -2}), A, "quad_stages_diag: sign must be -1, 0 or +1" + STAGE(2)),
    ("shifted-rider-without-vector", RIDERS, dict(dedit={(0, "vec"): None}), A, "quad_stages_diag: a shifted rider without its vector" + STAGE(0)),
    ("shifted-rider-without-vector-minus", RIDERS, dict(dedit={(2, "sign"): -1}), A, "quad_stages_diag: a shifted rider without its vector" + STAGE(2)),
    ("absent-rider-not-looked-at", RIDERS, dict(dedit={(1, "sign"): 9, (1, "present"): 0}), None, None),
    ("null-riders", RIDERS, dict(null=("diags",)), None, None),
    # T == 0: the plain check looks at nothing more; the others still test nconsts and the constants; no rider is looked at
    ("T0", KINDS, dict(T=0), None, None),
    ("T0-null-tables", KINDS, dict(T=0, null=("stages", "terms", "diags", "consts"), nconsts=0, dq=-31, dl=-12), None, None),
    ("T0-null-stages-and-terms", SIDE, dict(T=0, null=("stages", "terms")), None, None),
    ("T0-nconsts-33", SIDE, dict(T=0, nconsts=33), D, NCONSTS),
    ("T0-nconsts-minus-one", SIDE, dict(T=0, nconsts=-1), D, NCONSTS),
    ("T0-null-consts-nconsts-1", SIDE, dict(T=0, null=("stages", "terms", "consts"), nconsts=1), A, NULL_CONSTS),
    ("T0-bad-rider", RIDERS, dict(T=0, dedit={(0, "present"): 2}), None, None),
    # two things wrong at once: counts, stage table, slices, side tables, riders
    ("T-negative-before-nconsts-33", SIDE, dict(T=-1, nconsts=33), D, "quad_stages: negative stage count"),
    ("T-negative-before-negative-nterms", KINDS, dict(T=-1, dq=-32), D, "quad_stages: negative stage count"),
    ("negative-nlin-before-null-table", KINDS, dict(dl=-13, null=("stages",)), D, "quad_stages: negative term count"),
    ("bad-stage-before-null-terms", SIDE, dict(edit={(0, "sign"): 2}, null=("terms",)), A, "quad_stages: sign must be -1, 0 or +1" + STAGE(0)),
    ("earlier-stage-before-later-stage", KINDS, dict(edit={(0, "n"): 0, (1, "xvar"): None}), D, "quad_stages: n outside 1 .. 256" + STAGE(0)),
    ("xvar-before-sign-in-one-stage", KINDS, dict(edit={(1, "xvar"): None, (1, "sign"): 2}), A, "quad_stages: null variable indices" + STAGE(1)),
    ("n-before-ldq-in-one-stage", KINDS, dict(edit={(2, "n"): 0, (2, "ldq"): -1}), D, "quad_stages: n outside 1 .. 256" + STAGE(2)),
    ("stage-before-slices", KINDS, dict(edit={(2, "ldq"): 4}, dq=-1), D, "quad_stages: ldq < n" + STAGE(2)),
    ("quad-slices-before-lin-slices", KINDS, dict(dq=-1, dl=-1), D, QUAD_SLICES),
    ("slices-before-null-terms", SIDE, dict(dl=-1, null=("terms",)), D, LIN_SLICES),
    ("null-terms-before-nconsts", SIDE, dict(null=("terms",), nconsts=33), A, NULL_TERMS),
    ("nconsts-before-null-consts", SIDE, dict(null=("consts",), nconsts=33), D, NCONSTS),
    ("null-consts-before-riders", RIDERS, dict(null=("consts",), nconsts=1, dedit={(0, "present"): 2}), A, NULL_CONSTS),
    ("present-before-identity", RIDERS, dict(edit={(1, "Q"): None}, dedit={(1, "present"): 2}), A, "quad_stages_diag: present must be 0 or 1" + STAGE(1)),
    ("rider-sign-before-vector", RIDERS, dict(dedit={(0, "sign"): 2, (0, "vec"): None}), A, "quad_stages_diag: sign must be -1, 0 or +1" + STAGE(0)),
    ("earlier-rider-before-later-rider", RIDERS, dict(dedit={(0, "vec"): None, (2, "sign"): 2}), A,
     "quad_stages_diag: a shifted rider without its vector" + STAGE(0)),
]


def _raises(lib, exc, message, fn, *args, **kw):
    """fn(..) raises exactly lib.<exc> — no subclass of it — with exactly `message`; exc None: it returns"""
    if exc is None:
        return fn(*args, **kw)
    with pytest.raises(getattr(lib, exc)) as info:
        fn(*args, **kw)
    assert type(info.value) is getattr(lib, exc) and str(info.value) == message


@pytest.mark.parametrize("kind,args,exc,message", [(k, a, e, m) for _, ks, a, e, m in CHECKS for k in ks],
                         ids=["%s-%s" % (i, k) for i, ks, _, _, _ in CHECKS for k in ks])
def test_check(lib, kind, args, exc, message):
    _raises(lib, exc, message, _check, lib, kind, **args)


def test_the_table_of_checks_is_complete():
    """every case has its own id; every refusal message of the checks is in the table, through every check that can give it"""
    ids = [c[0] for c in CHECKS]
    assert len(set(ids)) == len(ids)
    through = {}
    for _, kinds, _, exc, message in CHECKS:
        if exc is not None:
            through.setdefault(message.split(" (stage")[0], set()).update(kinds)
    stage = {"quad_stages: " + m for m in ("negative stage count", "negative term count", "null stage table", "null variable indices",
                                           "sign must be -1, 0 or +1", "a shifted stage without its vector", "n outside 1 .. 256", "ldq < n",
                                           "a slice starts below 0", "quadratic slices overlap or leave [0, nterms)",
                                           "linear slices overlap or leave [0, nlin)")}
    riders = {"quad_stages_diag: " + m for m in ("present must be 0 or 1", "a rider on an identity stage", "sign must be -1, 0 or +1",
                                                 "a shifted rider without its vector")}
    want = {**{m: set(KINDS) for m in stage}, **{m: set(SIDE) for m in (NULL_TERMS, NCONSTS, NULL_CONSTS)}, **{m: set(RIDERS) for m in riders}}
    want["quad_stages: null matrix"] = {"plain", "terms"}
    assert through == want


# ---- 2. the four entry points, refused before any device call
ENTRY = {"plain": "pmt_quad_stages_f64", "terms": "pmt_quad_stages_terms_f64", "diag": "pmt_quad_stages_diag_f64", "csc": "pmt_quad_stages_csc_f64"}
PREFIX = {"plain": "quad_stages", "terms": "quad_stages_terms", "diag": "quad_stages_diag", "csc": "quad_stages_csc"}


def _launch(lib, kind, T=2, nconsts=1, alpha=1.0, **ptr):
    """the entry point of `kind` with fake non-NULL addresses, those named in `ptr` replaced; `quad`: the quadratic output, out_P_values for csc"""
    p = dict({k: FAKE for k in ("stages", "terms", "diags", "consts", "varmap", "quad", "lin", "sconsts", "const")}, **ptr)
    tail = (p["quad"], p["lin"], p["sconsts"], p["const"], None)
    args = {"plain": (p["stages"], T, p["varmap"]) + tail,
            "terms": (p["stages"], p["terms"], T, p["consts"], nconsts, p["varmap"]) + tail,
            "diag": (p["stages"], p["terms"], p["diags"], T, p["consts"], nconsts, p["varmap"]) + tail,
            "csc": (p["stages"], p["terms"], p["diags"], T, p["consts"], nconsts, p["varmap"], alpha) + tail}[kind]
    lib.call(ENTRY[kind], *args)


# (id, the entry points it goes through, _launch's arguments, the exception class, the message behind the entry's own prefix)
ENTRIES = [
    ("T-negative", KINDS, dict(T=-1), D, "negative stage count"),
    ("nconsts-minus-one", SIDE, dict(nconsts=-1), D, "nconsts outside 0 .. 32"),
    ("nconsts-33", SIDE, dict(nconsts=33), D, "nconsts outside 0 .. 32"),
    ("null-const", KINDS, dict(const=None), A, "null constant"),
    ("null-const-T0", KINDS, dict(const=None, T=0), A, "null constant"),
    ("null-const-T0-no-tables", KINDS, dict(const=None, T=0, nconsts=0, stages=None, terms=None, diags=None, consts=None, varmap=None, quad=None,
                                            lin=None, sconsts=None), A, "null constant"),
    ("null-const-without-riders", RIDERS, dict(const=None, diags=None), A, "null constant"),
    ("null-consts", SIDE, dict(consts=None), A, "null table of constants"),
    ("null-consts-T0", SIDE, dict(consts=None, T=0), A, "null table of constants"),
    ("null-consts-nconsts-32", SIDE, dict(consts=None, nconsts=32), A, "null table of constants"),
    ("null-stages", KINDS, dict(stages=None), A, "null pointer"),
    ("null-terms", SIDE, dict(terms=None), A, "null pointer"),
    ("null-varmap", KINDS, dict(varmap=None), A, "null pointer"),
    ("null-quad", KINDS, dict(quad=None), A, "null pointer"),
    ("null-values-maximize", KINDS[3:], dict(quad=None, alpha=-1.0), A, "null pointer"),
    ("null-lin", KINDS, dict(lin=None), A, "null pointer"),
    ("null-stage-consts", KINDS, dict(sconsts=None), A, "null pointer"),
    ("null-stages-without-consts", SIDE, dict(stages=None, consts=None, nconsts=0), A, "null pointer"),
    # two things wrong at once: T, nconsts, out_const, the constants table, the other pointers
    ("T-negative-before-nconsts-33", SIDE, dict(T=-1, nconsts=33), D, "negative stage count"),
    ("T-negative-before-null-const", KINDS, dict(T=-1, const=None), D, "negative stage count"),
    ("nconsts-before-null-const", SIDE, dict(nconsts=33, const=None), D, "nconsts outside 0 .. 32"),
    ("null-const-before-null-consts", SIDE, dict(const=None, consts=None), A, "null constant"),
    ("null-const-before-null-stages", KINDS, dict(const=None, stages=None), A, "null constant"),
    ("null-consts-before-null-stages", SIDE, dict(consts=None, stages=None), A, "null table of constants"),
]


@pytest.mark.parametrize("kind,args,exc,message", [(k, a, e, m) for _, ks, a, e, m in ENTRIES for k in ks],
                         ids=["%s-%s" % (i, k) for i, ks, _, _, _ in ENTRIES for k in ks])
def test_entry_point(lib, kind, args, exc, message):
    _raises(lib, exc, "%s: %s" % (PREFIX[kind], message), _launch, lib, kind, **args)


def test_the_table_of_entry_points_is_complete():
    """every case has its own id and is a refusal (an accepted call would reach the device); every pointer an entry point takes is NULL in
    turn — but for the rider table, which may be NULL — and every count out of its range"""
    ids = [c[0] for c in ENTRIES]
    assert len(set(ids)) == len(ids) and all(exc is not None for _, _, _, exc, _ in ENTRIES)
    alone = {}
    for _, kinds, args, _, _ in ENTRIES:
        if len(args) == 1:
            for k in kinds:
                alone.setdefault(k, set()).update(args.items())
    common = {("T", -1), ("const", None), ("stages", None), ("varmap", None), ("quad", None), ("lin", None), ("sconsts", None)}
    side = common | {("nconsts", -1), ("nconsts", 33), ("consts", None), ("terms", None)}
    assert alone == {"plain": common, "terms": side, "diag": side, "csc": side}
