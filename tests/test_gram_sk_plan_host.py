"""CPU: the case tables of test_gpu_gram_sk.py pushed through the host restatement of the stream-K form's launch arithmetic
(gram_sk_util: launch_gram_sk, deliver_plan, gram_form).  Proves, without a GPU, that the tables reach every load path, split regime and
fix-up of csrc/gram_sk.hip, that the exact-data bound holds for every case, and that each case's expected use of the kernel agrees with the
library's own dispatch (pmt_quad_gram_constant_order)."""
import ctypes as C

import numpy as np
import pytest

import gram_sk_util as U

IDS = [U.case_id(c) for c in U.CASES]


def _launches(cases=U.CASES):
    return [(c, p, ow, st) for c in cases for p, ow, st in U.case_launches(c)]


def test_restated_form_is_the_use_each_case_expects():
    for c in U.CASES:
        csc, deliver = c.entry in ("csc", "csc_deliver"), c.entry.endswith("deliver")
        assert U.sk_use(c.rows, c.cols, csc, deliver) == c.use, U.case_id(c)
        assert c.quad or csc, "a case without an output"
    # the three jobs and both instantiations are all present
    assert {c.use for c in U.CASES} == {"plain", "staged", "strict"}


@pytest.mark.parametrize("c", U.CASES, ids=IDS)
def test_expected_form_agrees_with_the_librarys_dispatch(c):
    """pmt_quad_gram_constant_order needs no GPU: orders 0 / 1 are the stream-K node, 5 a staged delivery of a shape whose plain call is
    the one-launch form, 2 .. 4 the fused form (whose strictly upper tiles are the strict launch)"""
    from parametron_jl_amd import _lib
    order = C.c_int()
    _lib.call("pmt_quad_gram_constant_order", c.rows, c.cols, C.byref(order), None, None)
    assert order.value in U.expected_constant_order(c.use, c.rows, c.cols), (U.case_id(c), order.value)
    if c.use == "plain":
        assert c.cols > 4096 and order.value in (0, 1)
    if c.use == "staged":
        assert order.value == (5 if c.cols <= 4096 else 0)


def test_plain_cases_are_the_33_tile_column_launch():
    for c in U.PLAIN:
        (p, ow, st), = U.case_launches(c)
        assert U.ntiles(c.cols) == 33 and (p.G, p.tfull, p.R, p.skc) == (256, 2, 49, 256) and st is None
        assert p.nchunk == U.cdiv(c.rows, 256) and p.U == 49 * p.nchunk and not p.fold
    plans = [U.case_launches(c)[0][0] for c in U.PLAIN]
    assert [p.nchunk for p in plans] == [1, 1, 2, 3, 5, 7]
    assert [p.fixup for p in plans] == ["none", "none", "apb4", "apb4", "apb4", "apb4"]
    assert plans[2].U < plans[2].G and plans[2].units_min == 0                      # (257, 4100): workgroups without a unit
    assert plans[4].U < plans[4].G
    assert plans[5].U > plans[5].G and U.slots_per_workgroup(plans[5]) == 2         # (1552, 4160): two partial slots in one workgroup
    assert all(U.slots_per_workgroup(p) <= 2 for p in plans)


def test_delivery_stages_are_the_ones_the_table_names():
    def sizes(c):
        return [st.seq_count for _, _, st in U.case_launches(c)]
    d = U.CSC_DELIVER
    assert sizes(d[0]) == [153]
    assert sizes(d[1]) == [128, 25] and sizes(d[2]) == [128, 25] and sizes(d[3]) == [128, 25]
    assert sizes(d[4]) == [10] * 15 + [3] and sizes(d[5]) == [10] * 15 + [3] and sizes(d[6]) == [10] * 15 + [3]
    assert sizes(d[7]) == [128] * 4 + [49]
    assert sizes(U.TERMS_DELIVER[0]) == [128, 25] and sizes(U.TERMS_DELIVER[1]) == [10] * 15 + [3]
    for c in U.CSC_DELIVER + U.TERMS_DELIVER:
        ow, stages = U.deliver_stages(c.rows, c.cols, c.ngroups, c.entry == "terms_deliver")
        assert len(stages) <= U.MAXGROUPS and sum(st.seq_count for st in stages) == U.tri(U.ntiles(c.cols))
        assert [st.seq_begin for st in stages] == list(np.cumsum([0] + [st.seq_count for st in stages[:-1]]))

    def kinds(c):
        return [(p.G, p.fold, p.fixup) for p, _, _ in U.case_launches(c)]
    assert kinds(d[0]) == [(153, False, "none")]                                        # whole tiles: nchunk = 1, tfull = 1, R = 0
    assert kinds(d[1]) == [(256, True, "none"), (50, True, "none")] == kinds(d[2])      # the pair fold, aligned and masked
    assert kinds(d[3]) == [(256, False, "apb4"), (75, False, "apb4")]
    assert kinds(d[4]) == [(30, False, "apb4")] * 15 + [(9, False, "apb1")]
    assert kinds(d[5]) == [(20, True, "none")] * 15 + [(6, True, "none")]
    assert kinds(d[6]) == [(256, False, "apb4")] * 15 + [(99, False, "sliced")]
    assert kinds(d[7]) == [(256, True, "none")] * 4 + [(98, True, "none")]
    assert U.linear_splits(8200, 2100) == 2                                             # gram_linear_split_kernel (b given: CSC_DELIVER[6])
    assert d[6].sign != 0
    assert all(U.linear_splits(c.rows, c.cols) == 1 for c in U.CASES if c is not d[6] and c.use != "strict")


def test_strict_cases_take_the_sliced_fixup_and_the_multiple_of_tile_count_grid():
    (p1, _, _), = U.case_launches(U.STRICT[0])
    (p3, _, _), = U.case_launches(U.STRICT[1])
    assert (p1.R, p1.G, p1.nchunk, p1.tfull, p1.fixup, p1.max_partials) == (1, 256, 1017, 0, "sliced", 256)
    assert (p3.R, p3.G, p3.nchunk, p3.tfull, p3.fixup) == (3, 255, 1021, 0, "sliced")      # 255 = 3 * (256 // 3), not 256
    assert p3.G % p3.R == 0 and p3.max_partials == 85
    assert U.load_path(U.STRICT[0]) == "masked" and U.load_path(U.STRICT[1]) == "vec"
    # the skc shrink is reachable only where T * chunks < 256: a strict launch of few rows (stated once; such shapes are the one-launch
    # form's today, so no case runs it)
    assert U.sk_launch_plan(300, 3, True, True, False).skc == 64 and U.sk_launch_plan(300, 3, True, False, False).skc == 256
    assert U.sk_launch_plan(5000, 1, False, False, False).skc == 64


def test_every_regime_is_reached_at_least_once():
    L = _launches()
    assert any(p.nchunk == 1 and p.fixup == "none" and not p.fold for _, p, _, _ in L)              # whole tiles, nothing split
    assert any(p.fold for _, p, _, _ in L)
    assert {p.fixup for _, p, _, _ in L} == {"none", "apb4", "apb1", "sliced"}
    assert any(p.U > p.G and U.slots_per_workgroup(p) == 2 for _, p, _, _ in L)
    assert any(p.R > 0 and p.U < p.G and p.units_min == 0 for _, p, _, _ in L)
    assert any(p.tfull > 0 and p.R > 0 for _, p, _, _ in L)
    assert any(c.use == "strict" and p.G != 256 and p.G % p.R == 0 for c, p, _, _ in L)
    assert {ow for c, _, ow, _ in L if c.use == "staged"} == {0, -U.DELIVER_ORDER_W}
    # the fix-up kernels' two loops: gram_sk_fixup_kernel loads LB = 4 (APB 4) or 16 (APB 1) partials at a time and has a tail loop
    assert any(p.fixup == "apb4" and p.max_partials >= 4 and p.max_partials % 4 for _, p, _, _ in L), "apb4: unrolled loop and tail"
    assert any(p.fixup == "apb4" and p.max_partials < 4 for _, p, _, _ in L), "apb4: tail only"
    assert any(p.fixup == "apb1" and 1 < p.max_partials < 16 for _, p, _, _ in L), "apb1: tail only"
    assert any(p.fixup == "sliced" and p.max_partials > 32 for _, p, _, _ in L), "sliced: the four-deep loop and its tail"
    # workgroups WITHOUT a unit between the first and the last owner of a split tile (their slots are added by the fix-up all the same:
    # launch_gram_sk clears them), on both instantiations; on the ranged one this is also the only launch with phase A (tfull = 2)
    for ranged in (False, True):
        assert any((c.use != "plain") == ranged and p.fixup != "none" and p.U < p.G and p.tfull == 2 and p.max_partials > p.nchunk for c, p, _, _ in L)
    # both instantiations see each fix-up they can launch, the fold only exists on the ranged one
    assert {p.fixup for c, p, _, _ in L if c.use == "plain"} == {"none", "apb4"}


def test_every_load_path_is_reached_on_both_instantiations():
    for ranged in (False, True):
        cases = [c for c in U.CASES if (c.use != "plain") == ranged]
        masked = [c for c in cases if U.load_path(c) == "masked"]
        assert any(c.rows < 16 for c in masked), "fewer than 16 rows"
        assert any(c.rows % 2 for c in masked), "an odd row count: the scalar tail of the 16-byte pieces"
        assert any((c.rows + c.pad) % 2 for c in masked), "an odd pitch"
        assert any(c.cols % U.ST == 1 for c in masked), "one column in the last column tile"
        # a chunk whose last stage is ragged: some unit range ends at the matrix's last row and its length is no multiple of SK_BK
        assert any(c.rows % U.SK_BK for c in masked)
        vec = [c for c in cases if U.load_path(c) == "vec"]
        assert any(c.rows % U.SK_BK == 0 and c.cols % U.ST == 0 for c in vec), "whole panels, whole stages: the FAST body alone"
        assert any(c.rows % U.SK_BK for c in vec), "16-byte loads with a ragged last stage"
        assert any(c.rows % 2 for c in vec), "16-byte loads and an odd row count: the last row comes through the scalar tail"
    assert any(c.shift == 1 for c in U.PLAIN), "an 8-byte-shifted base"


def test_options_are_spread_over_both_instantiations():
    for ranged in (False, True):
        cases = [c for c in U.CASES if (c.use != "plain") == ranged]
        assert {c.sign for c in cases} == {-1, 0, 1}
        assert any(c.moi == 1 and c.vm and c.quad for c in cases) and any(c.moi == 0 and c.quad for c in cases)
        for alpha in (-0.5, 2.0):
            assert any(c.alpha == alpha for c in cases)
        assert any(c.alpha != 1.0 and c.quad for c in cases) and any(c.alpha != 1.0 and not c.quad for c in cases)
    assert all(c.alpha in (-0.5, 2.0) for c in U.CASES if c.entry in ("csc", "csc_deliver"))
    assert {c.moi for c in U.TERMS_DELIVER} == {0, 1}
    assert [U.CASES.index(c) for c in U.RANDOM] == [3, 10] and U.RANDOM[1].ngroups == 16


def test_reversed_walk_covers_every_tile_once_and_completes_bands_in_descending_order():
    for c in (U.CSC_DELIVER[1], U.CSC_DELIVER[4], U.TERMS_DELIVER[1]):
        quad = c.entry == "terms_deliver"
        ow, stages = U.deliver_stages(c.rows, c.cols, c.ngroups, quad)
        nt = U.ntiles(c.cols)
        tiles = [t for st in stages for t in U.stage_tiles(c.cols, ow, st)]
        assert sorted(tiles) == sorted((j, k) for j in range(nt) for k in range(j, nt))
        if not quad:
            assert tiles[0] == (nt - 1, nt - 1) and tiles[-1] == (0, 0)
            assert [k for _, k in tiles] == sorted((k for _, k in tiles), reverse=True)
        else:
            assert tiles[0] == (0, 0) and tiles[-1] == (nt - 1, nt - 1)


@pytest.mark.parametrize("c", U.CASES, ids=IDS)
def test_dyadic_bound_holds_and_sampled_sums_are_exact(c):
    """the bound 2 bits + ceil(log2 rows) + 1 <= 52, and what it buys: numpy's float64 sums of a few columns equal the Python-integer sums,
    in the given and in the reversed row order"""
    assert U.dyadic_bound_holds(c.rows, c.bits) and c.bits >= 16
    rng = np.random.default_rng(c.rows + c.cols)
    A, b = U.dyadic((c.rows, 3), c.bits, rng), U.dyadic(c.rows, c.bits, rng)
    assert np.all(np.abs(A) < 1) and np.all(A * 2.0 ** c.bits == np.rint(A * 2.0 ** c.bits))
    G, q, cc = A.T @ A, A.T @ (0.0 - b), b @ b
    Gr, qr = A[::-1].T @ A[::-1], A[::-1].T @ (0.0 - b[::-1])
    assert U.exact_dot(b, b, c.bits) == cc
    for j in range(3):
        assert U.exact_dot(A[:, j], 0.0 - b, c.bits) == q[j] == qr[j]
        for k in range(3):
            assert U.exact_dot(A[:, j], A[:, k], c.bits) == G[j, k] == Gr[j, k]
    if c.rows > 64:
        lo = np.abs(G.view(np.int64)) & 0xFFFFFFFF
        assert np.any(lo != 0), "the low words of the sums are filled"


def test_reference_layout_on_a_small_case():
    """the numpy reference's term / CSC layout against a dense restatement (3 columns)"""
    c = U._case("csc", "plain", 4, 3, 0, 0, sign=-1, vm=True, alpha=-0.5, quad=True)
    rng = np.random.default_rng(1)
    A, b = U.dyadic((4, 3), c.bits, rng), U.dyadic(4, c.bits, rng)
    xv, vm = U.variables(3, 7)
    ref = U.reference(c, A, b, xv, vm)
    G = 2 * A.T @ A
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    assert np.array_equal(ref["quad"][:, 0].view(np.float64), [G[j, k] for j, k in pairs])
    assert np.array_equal(ref["quad"][:, 1], [vm[xv[j] - 1] for j, _ in pairs]) and np.array_equal(ref["quad"][:, 2], [vm[xv[k] - 1] for _, k in pairs])
    assert np.array_equal(ref["csc"], [-0.5 * G[j, k] for k in range(3) for j in range(k + 1)])
    assert np.array_equal(ref["lin"][:, 0].view(np.float64), -2 * A.T @ b) and ref["const"] == float(b @ b)
    native = U.reference(c._replace(entry="plain", moi=0), A, b, xv, vm)
    assert np.array_equal(native["quad"][:, 0].view(np.float64), [G[j, k] / (2 if j == k else 1) for j, k in pairs])
    assert np.array_equal(native["quad"][:, 1], [xv[j] for j, _ in pairs]) and native["csc"] is None
