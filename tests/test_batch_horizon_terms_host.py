"""CPU suite of the batched horizons with a terminal cost, stage weights and linear stage terms (pmt_batch_horizon_terms_coeffs_f64,
pmt_batch_horizon_terms_expand_f64, batch.horizon_terms_slab_layout): the numpy restatement (tests/batch_horizon_terms_util.py), which
tests/test_gpu_batch_horizon_terms.py compares the kernels with bit for bit, against quad_stages_terms_util's restatement of
pmt_quad_stages_terms_f64 for the instance's own table, against the sibling's restatement where everything optional is absent, and against
the oracle's literal sequence within the rounding bounds quad_stages_terms_util derives; wrong restatements are told apart; the slab length
against the layout; and the argument validation of both device entry points, which needs no GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import batch_horizon_terms_util as HT
import batch_horizon_util as H
import batch_util as BU
import quad_form_shift_util as SU
import quad_stages_terms_util as W
import quad_stages_util as QU

COEFFS, EXPAND, DOUBLES = "pmt_batch_horizon_terms_coeffs_f64", "pmt_batch_horizon_terms_expand_f64", "pmt_batch_horizon_terms_slab_doubles"


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

def test_slab_length_equals_the_layout_over_a_grid(lib):
    from parametron_jl_amd import batch as PB
    fn = getattr(lib.load(), DOUBLES)
    for T, nx, nu, m, term in itertools.product((1, 2, 7, 512), (1, 3, 64, 65, 128), (0, 1, 64, 128), (0, 1, 5, 33), (0, 1)):
        off, L = PB.horizon_terms_slab_layout(T, nx, nu, m, bool(term))
        n, ns = T * (nx + nu) + term * nx, T * (2 if nu else 1) + term
        assert fn(T, nx, nu, term, m) == L == HT.slab_doubles(T, nx, nu, term, m)
        sec = HT.sections(T, nx, nu, term, m)
        assert [off[k] for k in ("SQ", "SR", "SP", "W", "q", "const", "C", "dconst")] == [sec[k].start for k in ("SQ", "SR", "SP", "W", "q", "const", "C", "d")]
        assert sec["d"].stop == L and sec["q"].stop - sec["q"].start == n and sec["W"].stop - sec["W"].start == ns
        assert sec["SP"].stop - sec["SP"].start == term * nx * (nx + 1) // 2 and sec["C"].stop - sec["C"].start == m * n
        # the sibling's slab and the stage weights, nothing else, without a terminal stage
        if not term:
            assert L == H.slab_doubles(T, nx, nu, m) + ns
    assert PB.horizon_terms_slab_layout(1, 1, 0, 0, False)[1] == 4              # [SQ: 1 | W: 1 | q: 1 | const]
    assert PB.horizon_terms_slab_layout(1, 1, 0, 0, True)[1] == 7               # [SQ: 1 | SP: 1 | W: 2 | q: 2 | const]


def test_entry_points_are_declared_bound_and_exported(lib):
    raw = C.CDLL(lib.LIB_PATH)
    for name, nargs in ((DOUBLES, 5), (COEFFS, 9), (EXPAND, 14)):
        assert hasattr(raw, name) and len(lib.SIGNATURES[name][1]) == nargs
    assert C.sizeof(lib.BatchHorizonTerms) == 128
    assert [f[0] for f in lib.BatchHorizonTerms._fields_] == ["Q", "R", "P", "r", "v", "rN", "wx", "wu", "wN", "gx", "gu", "gN", "C", "d", "sign_r", "sign_v",
                                                               "sign_rN", "sign_d"]
    assert len(lib.SIGNATURES["pmt_batch_horizon_coeffs_f64"][1]) == 17 and len(lib.SIGNATURES["pmt_batch_horizon_expand_f64"][1]) == 13   # the siblings keep theirs


# ---- 2. the restated expansion against quad_stages_terms_util's restatement for the instance's own table

COMBOS = [(terminal, weights, linear) for terminal in (False, True) for weights in (False, True) for linear in (False, True)]


@pytest.mark.parametrize("terminal,weights,linear", COMBOS)
@pytest.mark.parametrize("T,nx,nu", [(3, 65, 10), (2, 5, 0), (130, 3, 2), (1, 1, 1)])
def test_restated_expansion_equals_the_stage_node_s_for_the_instance_table(T, nx, nu, terminal, weights, linear):
    """every combination of terminal, weights, linear, with and without inputs, over sign quadruples that make every kind of stage plain
    once: the slab's W / q / const and the expansion's buffers equal, word for word, W.restate on the table [x_0, u_0, .., x_T]"""
    rng = np.random.default_rng(T + 10 * nx + nu)
    m = 2
    b = HT.terms_data(2, T, nx, nu, m, rng, terminal, weights, linear)
    term = 1 if terminal else 0
    n = T * (nx + nu) + term * nx
    xvar, varmap = z_vars(n, rng)
    sec = HT.sections(T, nx, nu, term, m)
    for signs in ((-1, 0, -1, -1), (1, -1, 0, 1), (0, 1, 1, 0), (0, 0, 0, -1)):
        inst = HT.instance(b, 1, signs)
        slab = HT.instance_slab(inst)
        stages, nterms, nlin = HT.instance_table(inst, xvar)
        assert nlin == n and len(stages) == T * (2 if nu else 1) + term
        assert nterms == T * (nx * (nx + 1) // 2 + nu * (nu + 1) // 2) + term * nx * (nx + 1) // 2
        quad, lin, _, const = W.images(stages, [], varmap, nterms, nlin)
        rq, rl, rc, rv, rvc = HT.expanded_reference(inst, xvar, varmap)
        assert np.array_equal(rq, quad) and np.array_equal(rl, lin) and bits([rc])[0] == bits([const])[0]
        assert np.array_equal(bits(slab[sec["q"]]), lin[0::2]) and bits(slab[sec["const"]])[0] == bits([const])[0]
        assert np.array_equal(bits(slab[sec["W"]]), bits([W.weight(st["W"]) for st in stages]))
        if not weights:
            assert np.all(slab[sec["W"]] == 1.0)
        # the constraint block over the n columns of this z
        assert len(rv) == 3 * m * n and np.array_equal(rv[2::3], np.tile(varmap[xvar - 1], m))
        assert np.array_equal(bits(rvc), bits(BU.signed(inst["d"], signs[3])))


def test_negative_and_nan_weights_on_plain_stages():
    """a plain stage multiplies its +0.0: -0.0 under a negative weight or a -0.0 weight where no linear term follows, NaN under a NaN weight —
    in its own q words and in the constant, nowhere else"""
    T, nx, nu = 3, 4, 2
    b = HT.terms_data(1, T, nx, nu, 0, np.random.default_rng(4), True, True, False)
    b["wx"][0] = [-2.0, 3.0, -0.0]
    b["wu"][0] = [1.0, -1.0, 0.0]
    sec = HT.sections(T, nx, nu, 1, 0)
    slab = HT.instance_slab(HT.instance(b, 0, (0, 0, -1, 0)))
    q = slab[sec["q"]][:T * (nx + nu)].reshape(T, nx + nu)
    neg = np.int64(-2 ** 63)
    assert np.all(bits(q[0, :nx]) == neg) and np.all(bits(q[1, :nx]) == 0) and np.all(bits(q[2, :nx]) == neg)
    assert np.all(bits(q[0, nx:]) == 0) and np.all(bits(q[1, nx:]) == neg) and np.all(bits(q[2, nx:]) == 0)
    clean = slab.copy()
    b["wu"][0, 1] = np.nan
    slab = HT.instance_slab(HT.instance(b, 0, (0, 0, -1, 0)))
    changed = np.flatnonzero(bits(slab) != bits(clean))
    at = sec["q"].start + (nx + nu) + nx
    assert set(changed.tolist()) == set(range(at, at + nu)) | {sec["const"].start, sec["W"].start + 3}
    assert np.isnan(slab[changed]).all()


# ---- 3. everything optional absent: the sibling's slab

@pytest.mark.parametrize("T,nx,nu,m", [(3, 65, 10, 2), (2, 7, 0, 0), (130, 3, 2, 1), (1, 128, 33, 0)])
def test_without_the_optionals_the_slab_minus_w_is_the_sibling_s(T, nx, nu, m):
    b = HT.terms_data(2, T, nx, nu, m, np.random.default_rng(T + nx), False, False, False)
    sec = HT.sections(T, nx, nu, 0, m)
    for sr, sv, sd in ((-1, 0, -1), (1, -1, 1), (0, 0, 0), (0, 1, -1)):
        for i in range(2):
            got = HT.instance_slab(HT.instance(b, i, (sr, sv, 0, sd)))
            want = H.instance_slab(b["Qt"][i].T, b["Rt"][i].T, b["r"][i] if sr else [None] * T, b["v"][i] if sv else [None] * T, b["Ct"][i].T,
                                   b["d"][i], sr, sv, sd)
            assert np.all(got[sec["W"]] == 1.0)
            assert np.array_equal(bits(np.delete(got, np.arange(sec["W"].start, sec["W"].stop))), bits(want))


# ---- 4. against the oracle's literal sequence, within the derived bounds

@pytest.mark.parametrize("T,nx,nu", [(3, 5, 2), (2, 65, 10), (2, 10, 65), (4, 7, 0), (1, 128, 3)])
def test_restatement_equals_the_oracle_sequence_within_the_derived_bounds(lib, T, nx, nu):
    """indices exactly; quadratic coefficients bit for bit on the diagonal and for weights that are zero or powers of two (a zero's sign
    apart), otherwise within quad_bound; linear coefficients within lin_bound, the constant within const_bound — nothing tuned.  The weights
    include negative ones, 0.0 and -0.0."""
    rng = np.random.default_rng(500 + 10 * nx + nu)
    b = HT.terms_data(1, T, nx, nu, 0, rng, True, True, True)
    b["wx"][0, 0], b["wN"][0] = -0.0, -2.5
    if T > 1:
        b["wx"][0, 1] = 0.0
    n = T * (nx + nu) + nx
    xvar, varmap = z_vars(n, rng)
    for signs in ((-1, 0, -1, 0), (1, -1, 1, 0)):
        inst = HT.instance(b, 0, signs)
        stages, nterms, nlin = HT.instance_table(inst, xvar)
        at, qt, oconst = W.oracle(stages, [], varmap)
        rq, rl, rc, _, _ = HT.expanded_reference(inst, xvar, varmap)
        quad, lin = rq.view(lib.QT), rl.view(lib.LT)
        want_q = dict(zip(zip(qt["row"].tolist(), qt["col"].tolist()), qt["coeff"].tolist()))
        want_l = QU.lin_by_var(at)
        assert set(want_q) <= set(zip(quad["row"].tolist(), quad["col"].tolist())) and set(want_l) <= set(lin["var"].tolist())
        for st in stages:
            nd = len(st["xvar"])
            q = quad[st["quad_at"]:st["quad_at"] + nd * (nd + 1) // 2]
            l = lin[st["lin_at"]:st["lin_at"] + nd]
            qb = W.quad_bound(st)
            got = np.array([want_q.get((r, c), 0.0) for r, c in zip(q["row"].tolist(), q["col"].tolist())])
            exact = qb == 0.0
            assert np.array_equal(q["coeff"][exact], got[exact]) and np.all(np.abs(q["coeff"] - got) <= qb)
            lb = W.lin_bound(st, QU.restate_stage(st, varmap)[1]["coeff"])
            err = np.abs(l["coeff"] - np.array([want_l.get(k, 0.0) for k in l["var"].tolist()]))
            assert np.all(err <= lb), (st["lin_at"], np.max(err / np.maximum(lb, 1e-300)))
            if st["sign"] and nd >= 63 and W.weight(st["W"]) != 0.0:                  # the bound is not vacuous
                assert np.max(lb) < 1e-9 * np.max(np.abs(l["coeff"]))
        cb = W.const_bound(stages, [], varmap)
        assert abs(rc - oconst) <= cb
        assert cb < 1e-9 * sum(abs(HT.weighted_words(s)[2]) for s in HT.stage_list(inst))


# ---- 5. wrong restatements are told apart

def test_wrong_restatements_are_told_apart():
    T, nx, nu = 3, 70, 5
    b = HT.terms_data(1, T, nx, nu, 0, np.random.default_rng(8), True, True, True)
    b["wx"][0], b["wu"][0], b["wN"][0] = [1.0 / 3.0, 0.9, -2.5], [0.81, 3.0, 1.0 / 3.0], 0.7853981633974483
    inst = HT.instance(b, 0, (-1, 1, -1, 0))
    right = HT.instance_slab(inst)
    sec = HT.sections(T, nx, nu, 1, 0)
    stages = HT.stage_list(inst)
    q_in, q_first, consts = [], [], []
    for st in stages:
        Wt, _, c = HT.weighted_words(st)
        # (a) the weight inside the chain: lin of (W * S) instead of W * lin
        q_in.append(H.stage_words(Wt * np.asarray(st["M"]), st["ref"], st["sign"])[0] + st["g"])
        # (b) the linear term added before the weight: W * (lin + g)
        q_first.append(Wt * (H.stage_words(st["M"], st["ref"], st["sign"])[0] + st["g"]))
        consts.append(c)
    inside, first = right.copy(), right.copy()
    inside[sec["q"]], first[sec["q"]] = np.concatenate(q_in), np.concatenate(q_first)
    # (c) the terminal constant out of z order: in front of the others.  With fewer than 256 stages every chain of S_d holds one stage
    # constant and the order is the tree's: the terminal constant at leaf 0 and the others moved up one leaf
    assert right[sec["const"]][0] == SU.chain_tree_sum(np.array(consts))
    moved = right.copy()
    moved[sec["const"]] = SU.chain_tree_sum(np.array(consts[-1:] + consts[:-1]))
    # (d) the weights applied to the sections; (e) the unweighted constant
    folded = right.copy()
    folded[sec["SQ"]] = right[sec["W"]][0] * right[sec["SQ"]]
    unweighted = right.copy()
    unweighted[sec["const"]] = SU.chain_tree_sum(np.array([H.stage_words(st["M"], st["ref"], st["sign"])[1] for st in stages]))
    for name, wrong in (("weight inside the chain", inside), ("linear term before the weight", first), ("terminal constant out of z order", moved),
                        ("weights folded into SQ", folded), ("unweighted constant", unweighted)):
        assert not np.array_equal(bits(wrong), bits(right)), name


# ---- 6. the entry points without a device

P = C.c_void_p(64)                          # never dereferenced: each call is rejected, or returns, before any device call
ALL = ("Q", "R", "P", "r", "v", "rN", "wx", "wu", "wN", "gx", "gu", "gN", "C", "d")


def _coeffs(lib, B=1, T=3, nx=4, nu=2, m=2, out=P, stride=None, desc=True, sign_r=-1, sign_v=-1, sign_rN=-1, sign_d=-1, **ptrs):
    fields = {k: ptrs.get(k, P.value) for k in ALL}
    term = 0 if fields["P"] is None else 1
    L = HT.slab_doubles(max(T, 0), max(nx, 0), max(nu, 0), term, max(m, 0))
    d = lib.batch_horizon_terms(sign_r=sign_r, sign_v=sign_v, sign_rN=sign_rN, sign_d=sign_d, **fields)
    lib.call(COEFFS, C.byref(d) if desc else None, B, T, nx, nu, m, out, L if stride is None else stride, None)


def _expand(lib, slab=P, T=3, nx=4, nu=2, term=1, m=2, xvar=P, varmap=P, quad=P, lin=P, const=P, vat=P, vconsts=P):
    lib.call(EXPAND, slab, T, nx, nu, term, m, xvar, varmap, quad, lin, const, vat, vconsts, None)


BAD_DIMS = [{"T": -1}, {"nx": -4}, {"nu": -1}, {"m": -2}, {"nx": 0}, {"nx": H.MAX_DIM + 1}, {"nu": H.MAX_DIM + 1}, {"nx": 1 << 40}, {"T": 0}, {"T": H.MAX_T + 1},
            {"T": 1 << 40}]
BAD_IDS = ["T-negative", "nx-negative", "nu-negative", "m-negative", "nx-zero", "nx-129", "nu-129", "nx-huge", "T-zero", "T-513", "T-huge"]


@pytest.mark.parametrize("bad", BAD_DIMS + [{"B": -1}, {"stride": HT.slab_doubles(3, 4, 2, 1, 2) - 1}, {"stride": HT.slab_doubles(3, 4, 2, 0, 2)}, {"stride": 0},
                                            {"stride": -5}],
                         ids=BAD_IDS + ["B-negative", "stride-L-1", "stride-of-no-terminal-stage", "stride-zero", "stride-negative"])
def test_dimension_errors_of_the_coefficients_come_before_any_device_call(lib, bad):
    kw = dict(bad)
    if "stride" not in kw:
        kw["stride"] = 1 << 62
    with pytest.raises(lib.DimensionMismatch, match="batch_horizon_terms"):
        _coeffs(lib, **kw)
    if "B" not in bad:                                                          # B == 0 does not excuse them
        with pytest.raises(lib.DimensionMismatch, match="batch_horizon_terms"):
            _coeffs(lib, B=0, **kw)


@pytest.mark.parametrize("bad", BAD_DIMS + [{"term": 2}, {"term": -1}], ids=BAD_IDS + ["term-2", "term-negative"])
def test_dimension_errors_of_the_expansion_come_before_any_device_call(lib, bad):
    with pytest.raises(lib.DimensionMismatch, match="batch_horizon_terms_expand"):
        _expand(lib, **bad)


@pytest.mark.parametrize("which", ["sign_r", "sign_v", "sign_rN", "sign_d"])
@pytest.mark.parametrize("value", [2, -2, 7])
def test_signs_outside_minus_one_zero_one_are_argument_errors(lib, which, value):
    with pytest.raises(lib.ArgumentError, match="sign"):
        _coeffs(lib, **{which: value})
    with pytest.raises(lib.DimensionMismatch):                                  # the dimension checks come first
        _coeffs(lib, stride=3, **{which: value})
    if which == "sign_rN":                                                      # checked without a terminal stage too
        with pytest.raises(lib.ArgumentError, match="sign"):
            _coeffs(lib, P=None, sign_rN=value)


@pytest.mark.parametrize("null", ["Q", "R", "r", "v", "rN", "C", "d", "out"])
def test_null_pointers_where_the_coefficients_need_data(lib, null):
    with pytest.raises(lib.ArgumentError, match="null"):
        _coeffs(lib, **{null: None})


def test_a_null_descriptor_is_an_argument_error(lib):
    with pytest.raises(lib.ArgumentError, match="null"):
        _coeffs(lib, desc=False)
    with pytest.raises(lib.ArgumentError, match="null"):
        _coeffs(lib, desc=False, B=0)


@pytest.mark.parametrize("null", ["slab", "xvar", "varmap", "quad", "lin", "const", "vat", "vconsts"])
def test_null_pointers_where_the_expansion_needs_them(lib, null):
    with pytest.raises(lib.ArgumentError, match="null"):
        _expand(lib, **{null: None})


def test_null_pointers_where_no_data_is_read_and_empty_batches(lib):
    """What these calls would launch needs a GPU: each must be rejected for the pointer that IS needed (out), or return PMT_OK without a launch"""
    none = {k: None for k in ("wx", "wu", "wN", "gx", "gu", "gN")}
    with pytest.raises(lib.ArgumentError, match="null"):                        # every optional array absent
        _coeffs(lib, out=None, **none)
    with pytest.raises(lib.ArgumentError, match="null"):                        # no terminal stage: rN is not needed
        _coeffs(lib, out=None, P=None, rN=None, **none)
    with pytest.raises(lib.ArgumentError, match="null"):                        # signs of 0: the references may be NULL
        _coeffs(lib, out=None, r=None, v=None, rN=None, sign_r=0, sign_v=0, sign_rN=0)
    with pytest.raises(lib.ArgumentError, match="null"):                        # nu == 0: R, v, wu, gu are not needed
        _coeffs(lib, out=None, R=None, v=None, wu=None, gu=None, nu=0)
    with pytest.raises(lib.ArgumentError, match="null"):                        # m == 0: C and d are not needed
        _coeffs(lib, out=None, C=None, d=None, m=0)
    with pytest.raises(lib.ArgumentError, match="null"):
        _expand(lib, vat=None, vconsts=None, m=0, const=None)
    with pytest.raises(lib.ArgumentError, match="null"):                        # sign_d == 0 still needs d, as the siblings do
        _coeffs(lib, d=None, sign_d=0)
    # an empty batch is complete as it stands, whatever the device pointers: PMT_OK, nothing launched
    for T, nx, nu, m in ((3, 4, 2, 2), (1, 1, 0, 0), (H.MAX_T, H.MAX_DIM, H.MAX_DIM, 1), (5, 2, 0, 3)):
        for term in (0, 1):
            d = lib.batch_horizon_terms(P=P.value if term else None, sign_r=-1, sign_v=1, sign_rN=-1, sign_d=-1)
            lib.call(COEFFS, C.byref(d), 0, T, nx, nu, m, None, HT.slab_doubles(T, nx, nu, term, m) + 3 * term, None)
