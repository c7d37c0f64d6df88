"""-m gpu: the reduction and hand-off kernels of the generic route at the C ABI, in their exact order.

literal terms -> pmt_canonical_order_* -> pmt_segment_sum_f64 -> the solver hand-off (pmt_csc_values_f64, pmt_csc_values_gather_f64,
pmt_copy_2d_f64, pmt_qp_bounds_rows_f64), and the generic builders of csrc/terms.hip launched directly.  Every sum is compared BIT FOR BIT
with a CPU restatement of the order its kernel documents (gpu_util.run_sum_sequential / run_sum_wave, written from the kernels' comments and
include/parametron_hip.h) and, independently of any order, with math.fsum: a sum of L terms in ANY order differs from the exact sum by at
most (L - 1) u sum|c| (1 + O(L u)), u = 2^-53, and fsum is within u |sum| of the exact one — together at most L * 2^-53 * sum|c|.
The coefficients are signed and spread over 40 binades, so that a different order gives different bits; every test asserts on the CPU,
before its first launch, that its data does tell the tree order from the left-to-right order.  Buffers are bit images (int64 words) with
recognisable words around everything a kernel owns: what a kernel does not own must come back unchanged."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import gpu_util as g  # noqa: E402
from parametron_jl_amd import _lib  # noqa: E402
from parametron_jl_amd.handoff import _csc_order  # noqa: E402
from parametron_jl_amd.lazyexpression import _canonical_order  # noqa: E402

U = 2.0 ** -53
ALPHA = -0.3                                       # not a power of two: alpha * (sum) and sum(alpha * c) differ in bits
NAN_DST = 0x7FF80000DEADBEEF                       # quiet NaNs with fixed payloads: untouched destination / source padding
NAN_SRC = 0x7FF800000BADF00D
NAN_DATA = 0x7FF8000000C0FFEE                      # ... and one that is DATA and must be copied as it is
WORD = 0x5A5A000000000000                          # recognisable index words: WORD + position
GUARD = 64


def coeffs(rng, n):
    """signed, spread over 40 binades"""
    return (rng.random(n) - 0.5) * 2.0 ** rng.integers(-20, 21, n)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def words(n, base=WORD):
    return base + np.arange(n, dtype=np.int64)


def host_words(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def at(t, word):
    """device address of word `word` of an int64 / float64 tensor"""
    return C.c_void_p(t.data_ptr() + 8 * int(word))


def runs_of(c, perm, seg):
    return [c[perm[seg[s]:seg[s + 1]]] for s in range(len(seg) - 1)]


def assert_not_identity(perm):
    assert not np.array_equal(perm, np.arange(len(perm))), "the permutation is the identity: the runs are not interleaved"


def assert_orders_distinguishable(runs, skip_empty):
    """a data set that cannot tell the tree order from the left-to-right order must not pass"""
    assert any(len(r) >= 3 and not g.same_bits(g.run_sum_wave(r, skip_empty), g.run_sum_sequential(r)) for r in runs), \
        "no run of this data has different tree and sequential sums"


def assert_alpha_distinguishable(runs, alpha, run_sum):
    assert any(not g.same_bits(alpha * run_sum(r), run_sum([alpha * v for v in r])) for r in runs), \
        "alpha per run and alpha per term give the same bits on this data"


def assert_within_fsum_bound(got, runs, alpha=1.0):
    """|got - alpha * fsum(run)| <= |alpha| L 2^-53 sum|c| (any order; see the module docstring); with alpha != 1 the one product
    got = fl(alpha * acc) adds at most 2^-53 |got|, and the reference product fl(alpha * fsum) as much again"""
    for s, r in enumerate(runs):
        ref = alpha * math.fsum(r)
        bound = abs(alpha) * len(r) * U * math.fsum(np.abs(r))
        if alpha != 1.0:
            bound += U * (abs(float(got[s])) + abs(ref))
        assert abs(float(got[s]) - ref) <= bound, (s, len(r), float(got[s]), ref, bound)


def interleaved_keys(rng, lens):
    """key k (from 1) occurs lens[k - 1] times, in random positions"""
    keys = np.repeat(np.arange(1, len(lens) + 1, dtype=np.int64), lens)
    rng.shuffle(keys)
    return keys


# ---- 1. pmt_segment_sum_f64 -----------------------------------------------------------------------------------------------------------
SEG_NSEG = 1027


@functools.lru_cache(maxsize=None)
def segment_data():
    """1027 runs of lengths 1, 2, 3, 63, 64, 65, 127, 128, 129, 200 (cycled) and one of 4097 at position 10, interleaved; ordered by the host
    ordering; the sums restated once.  The launches below take ranges of these runs (seg_ptr + first), so `perm` is never the identity,
    not even for a single run."""
    rng = np.random.default_rng(20261)
    lens = [(1, 2, 3, 63, 64, 65, 127, 128, 129, 200)[s % 10] for s in range(SEG_NSEG - 1)]
    lens.insert(10, 4097)
    keys = interleaved_keys(rng, lens)
    c = coeffs(rng, len(keys))
    perm, seg, (ov,) = _canonical_order("aff", keys)
    assert np.array_equal(np.diff(seg), lens) and len(ov) == SEG_NSEG
    assert_not_identity(perm)
    runs = runs_of(c, perm, seg)
    want = np.array([g.run_sum_wave(r, True) for r in runs])
    assert_within_fsum_bound(want, runs)
    return c, perm, seg, runs, want


def segment_sum_image(before, sums, out_words):
    """the output term buffer after the call: word 0 of each term is the run's sum, every other word as it was"""
    img = before.copy()
    img[np.arange(len(sums)) * out_words] = bits(sums)
    return img


# (nseg, first run): 1 -> the run of 4097; 3 -> 200, 4097, 1; 4 -> 64, 65, 127, 128 (one FULL workgroup of four waves); 5 -> 1, 2, 3, 63, 64
# (the second workgroup has one wave of four at work); 1027 -> every length in one call, the last workgroup three waves
@pytest.mark.parametrize("strides", [(16, 16), (24, 24), (8, 8), (24, 8)])
@pytest.mark.parametrize("nseg,first", [(1, 10), (3, 9), (4, 4), (5, 0), (SEG_NSEG, 0)])
def test_segment_sum_in_the_wave_order_writes_only_coefficients(nseg, first, strides):
    c, perm, seg, runs, want = segment_data()
    runs, want = runs[first:first + nseg], want[first:first + nseg]
    if nseg == SEG_NSEG:
        assert sorted(set(len(r) for r in runs)) == [1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 4097]
    assert_orders_distinguishable(runs, True)
    iw, ow = strides[0] // 8, strides[1] // 8
    src = words(len(c) * iw, 0x1111000000000000)
    src[::iw] = bits(c)
    before = words(nseg * ow + GUARD)
    want_img = segment_sum_image(before, want, ow)
    g.lib()
    dsrc, dperm, dseg, out = g.to_dev(src), g.to_dev(perm), g.to_dev(seg), g.to_dev(before)
    g.call("pmt_segment_sum_f64", g.ptr(dsrc), strides[0], g.ptr(dperm), at(dseg, first), nseg, g.ptr(out), strides[1], g.stream())
    got = host_words(out)
    assert np.array_equal(got[nseg * ow:], before[nseg * ow:]), "the guard band behind the last term changed"
    for k in range(1, ow):
        assert np.array_equal(got[k:nseg * ow:ow], before[k:nseg * ow:ow]), "index word %d of an output term changed" % k
    sums = got[:nseg * ow:ow].view(np.float64)
    assert_within_fsum_bound(sums, runs)
    bad = np.flatnonzero(got[:nseg * ow:ow] != bits(want))
    assert bad.size == 0, "runs %s (lengths %s) differ from the restated order" % (bad[:5], [len(runs[i]) for i in bad[:5]])
    assert np.array_equal(got, want_img)


def test_segment_sum_signed_zeros_empty_call_and_argument_errors():
    """empty lanes add nothing, not even +0.0: [-0.0] -> -0.0, [-0.0, -0.0] -> -0.0, [-0.0, 0.0] -> 0.0 (a lane or a tree that started from
    +0.0 would give +0.0 for the first two)"""
    rng = np.random.default_rng(20262)
    n = 5 + 65
    # the five zero terms keep their order among themselves (keys 2, 3, 1, 2, 3), at random places among the 65 terms of a fourth run
    slots = np.sort(rng.choice(n, 5, replace=False))
    rest = np.setdiff1d(np.arange(n), slots)
    mixed_keys, mixed_c = np.full(n, 4, dtype=np.int64), np.zeros(n)
    mixed_keys[slots], mixed_c[slots] = [2, 3, 1, 2, 3], [-0.0, -0.0, -0.0, -0.0, 0.0]
    mixed_c[rest] = coeffs(rng, 65)
    perm, seg, (ov,) = _canonical_order("aff", mixed_keys)
    assert ov.tolist() == [1, 2, 3, 4] and np.diff(seg).tolist() == [1, 2, 2, 65]
    assert_not_identity(perm)
    runs = runs_of(mixed_c, perm, seg)
    assert g.same_bits(np.concatenate(runs[:3]), [-0.0, -0.0, -0.0, -0.0, 0.0])          # [-0.0], [-0.0, -0.0], [-0.0, 0.0]
    want = np.array([g.run_sum_wave(r, True) for r in runs])
    assert g.same_bits(want[:3], [-0.0, -0.0, 0.0])
    assert_orders_distinguishable(runs, True)
    t = np.zeros(len(mixed_c), dtype=g.LT)
    t["coeff"], t["var"] = mixed_c, mixed_keys
    before = words(4 * 2 + GUARD)
    g.lib()
    dt, dperm, dseg, out = g.to_dev(t), g.to_dev(perm), g.to_dev(seg), g.to_dev(before)
    g.call("pmt_segment_sum_f64", g.ptr(dt), 16, g.ptr(dperm), g.ptr(dseg), 4, g.ptr(out), 16, g.stream())
    got = host_words(out)
    assert g.same_bits(got[0:6:2].view(np.float64), [-0.0, -0.0, 0.0])
    assert np.array_equal(got, segment_sum_image(before, want, 2))
    # nseg = 0: OK, and nothing is written
    out = g.to_dev(before)
    g.call("pmt_segment_sum_f64", g.ptr(dt), 16, g.ptr(dperm), g.ptr(dseg), 0, g.ptr(out), 16, g.stream())
    assert np.array_equal(host_words(out), before)
    for bad in (4, 12):
        with pytest.raises(_lib.ArgumentError):
            g.call("pmt_segment_sum_f64", g.ptr(dt), bad, g.ptr(dperm), g.ptr(dseg), 4, g.ptr(out), 16, g.stream())
        with pytest.raises(_lib.ArgumentError):
            g.call("pmt_segment_sum_f64", g.ptr(dt), 16, g.ptr(dperm), g.ptr(dseg), 4, g.ptr(out), bad, g.stream())
    with pytest.raises(_lib.DimensionMismatch):
        g.call("pmt_segment_sum_f64", g.ptr(dt), 16, g.ptr(dperm), g.ptr(dseg), -1, g.ptr(out), 16, g.stream())
    assert np.array_equal(host_words(out), before)


# ---- 2. the device ordering composed with the sum ---------------------------------------------------------------------------------------
def order_init_sum_on_the_device(t):
    """pmt_canonical_order_device -> pmt_canonical_init_terms -> pmt_segment_sum_f64 (into the buffer init_terms wrote);
    returns perm, seg_ptr, the output terms and the guard band behind them"""
    dtype, n = t.dtype, len(t)
    wpt = dtype.itemsize // 8
    g.lib()
    dt = g.to_dev(t)
    dperm = torch.full((n,), -1, dtype=torch.int64, device=g.DEV)
    dseg = torch.full((n + 1,), -1, dtype=torch.int64, device=g.DEV)
    nseg = C.c_int64(-1)
    torch.cuda.synchronize()
    g.call("pmt_canonical_order_device", g.ptr(dt), n, dtype.itemsize, g.ptr(dperm), g.ptr(dseg), C.byref(nseg), g.stream())
    k = nseg.value
    assert 1 <= k <= n
    out = g.to_dev(words(k * wpt + GUARD))
    g.call("pmt_canonical_init_terms", g.ptr(dt), dtype.itemsize, g.ptr(dperm), g.ptr(dseg), k, g.ptr(out), g.stream())
    g.call("pmt_segment_sum_f64", g.ptr(dt), dtype.itemsize, g.ptr(dperm), g.ptr(dseg), k, g.ptr(out), dtype.itemsize, g.stream())
    img = host_words(out)
    return host_words(dperm), host_words(dseg)[:k + 1], img[:k * wpt].view(dtype), img[k * wpt:]


def check_chain_against_the_host_ordering(t):
    if t.dtype == g.QT:
        perm, seg, outs = _canonical_order("quad", t["row"], t["col"])
        names = ("row", "col")
    else:
        perm, seg, outs = _canonical_order("aff", t["var"])
        names = ("var",)
    assert_not_identity(perm)
    runs = runs_of(t["coeff"], perm, seg)
    assert_orders_distinguishable(runs, True)
    want = np.array([g.run_sum_wave(r, True) for r in runs])
    assert_within_fsum_bound(want, runs)
    dperm, dseg, got, guard = order_init_sum_on_the_device(t)
    assert np.array_equal(dperm, perm) and np.array_equal(dseg, seg)
    for name, o in zip(names, outs):
        assert np.array_equal(got[name], o), name
    assert np.array_equal(guard, WORD + (len(seg) - 1) * (t.dtype.itemsize // 8) + np.arange(GUARD)), "the guard band changed"
    assert_within_fsum_bound(got["coeff"], runs)
    bad = np.flatnonzero(bits(got["coeff"]) != bits(want))
    assert bad.size == 0, "runs %s (lengths %s) differ from the restated order" % (bad[:5], [len(runs[i]) for i in bad[:5]])


@pytest.mark.parametrize("kind", ["quad", "aff"])
def test_device_ordering_then_init_then_sum_gives_the_restated_coefficients(kind):
    """20000 quadratic terms over 5 variables (15 keys, runs of about 1300) / 5000 linear terms over 3 variables"""
    rng = np.random.default_rng(20263 if kind == "quad" else 20264)
    if kind == "quad":
        t = np.zeros(20000, dtype=g.QT)
        t["row"], t["col"] = rng.integers(1, 6, 20000), rng.integers(1, 6, 20000)
    else:
        t = np.zeros(5000, dtype=g.LT)
        t["var"] = rng.integers(1, 4, 5000)
    t["coeff"] = coeffs(rng, len(t))
    check_chain_against_the_host_ordering(t)


def packed_key_edge_terms():
    rng = np.random.default_rng(20265)
    big = 2 ** 32 - 1
    pool = np.array([1, 2, big - 1, big], dtype=np.int64)
    t = np.zeros(240, dtype=g.QT)
    t["row"], t["col"] = pool[rng.integers(0, 4, 240)], pool[rng.integers(0, 4, 240)]
    t["row"][:3], t["col"][:3] = [big, big, 1], [big, 1, big]
    t["coeff"] = coeffs(rng, 240)
    assert max(t["row"].max(), t["col"].max()) == big
    return t


def test_packed_key_accepts_indices_up_to_its_edge():
    """the packed 64-bit key holds both indices below 2^32: 2^32 - 1 is the largest accepted one, in either half of the key"""
    check_chain_against_the_host_ordering(packed_key_edge_terms())


def test_packed_key_refuses_the_first_index_beyond_its_edge():
    t = packed_key_edge_terms()
    for f in ("row", "col"):
        t[f][t[f] == 2 ** 32 - 1] = 2 ** 32
    g.lib()
    dt = g.to_dev(t)
    dperm, dseg = torch.zeros(len(t), dtype=torch.int64, device=g.DEV), torch.zeros(len(t) + 1, dtype=torch.int64, device=g.DEV)
    nseg = C.c_int64()
    torch.cuda.synchronize()
    with pytest.raises(_lib.ArgumentError, match="host ordering"):
        g.call("pmt_canonical_order_device", g.ptr(dt), len(t), 24, g.ptr(dperm), g.ptr(dseg), C.byref(nseg), g.stream())
    torch.cuda.synchronize()


def test_linear_keys_are_not_packed():
    """a LinearTerm's key is its variable index alone: 2^40 is accepted and ordered like the host's"""
    rng = np.random.default_rng(20266)
    t = np.zeros(200, dtype=g.LT)
    t["var"] = np.array([3, 2 ** 40, 7], dtype=np.int64)[rng.integers(0, 3, 200)]
    t["var"][0] = 2 ** 40
    t["coeff"] = coeffs(rng, 200)
    check_chain_against_the_host_ordering(t)


# ---- 3. pmt_csc_values_f64 --------------------------------------------------------------------------------------------------------------
LAYOUTS = {"linear": (g.LT, 0), "quadratic": (g.QT, 0), "vector_affine": (g.VAT, 8)}      # (term, offset of its coefficient)


def term_source(c, layout, rng):
    """a term buffer of this layout that holds the coefficients c (recognisable words in the index fields);
    returns the tensor, the address of the coefficient of term 0 and the stride"""
    dtype, off = LAYOUTS[layout]
    t = np.zeros(len(c), dtype=dtype)
    for f in dtype.names:
        t[f] = c if f == "coeff" else rng.integers(1, 1 << 40, len(c))
    dt = g.to_dev(t)
    return dt, C.c_void_p(dt.data_ptr() + off), dtype.itemsize


def csc_structure(rng, lens, ncols=5):
    """entry k of a matrix with `ncols` columns occurs lens[k] times, in random positions; the project's CSC ordering of that list"""
    ids = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    rng.shuffle(ids)
    perm, seg, col_ptr, row_idx = _csc_order(ids // ncols + 1, ids % ncols + 1, (len(lens) - 1) // ncols + 1, ncols, upper=False)
    assert len(seg) - 1 == len(lens) and sorted(np.diff(seg).tolist()) == sorted(lens)
    assert_not_identity(perm)
    return perm, seg


def injection(rng, nseg):
    """dst_index: a random injection into a destination twice as large, filled with a NaN of a fixed payload"""
    return rng.permutation(2 * nseg)[:nseg].astype(np.int64), np.full(2 * nseg, NAN_DST, dtype=np.int64)


def csc_values_image(before, runs, alpha, dst_index, run_sum):
    """dst[dst_index[s]] = alpha * (the sum of run s) (include/parametron_hip.h): alpha once per run, everything else as it was"""
    img = before.copy()
    img[dst_index] = bits([alpha * run_sum(r) for r in runs])
    return img


def check_csc_values(c, perm, seg, first, nseg, layout, rng, run_sum):
    runs = runs_of(c, perm, seg)[first:first + nseg]
    nnz_in = int(seg[first + nseg] - seg[first])
    dst_index, before = injection(rng, nseg)
    want_img = csc_values_image(before, runs, ALPHA, dst_index, run_sum)
    g.lib()
    dt, src, stride = term_source(c, layout, rng)
    dperm, dseg, didx, dst = g.to_dev(perm), g.to_dev(seg), g.to_dev(dst_index), g.to_dev(before)
    g.call("pmt_csc_values_f64", src, stride, nnz_in, g.ptr(dperm), at(dseg, first), nseg, ALPHA, g.ptr(didx), g.ptr(dst), g.stream())
    got = host_words(dst)
    del dt
    untouched = np.setdiff1d(np.arange(2 * nseg), dst_index)
    assert np.all(got[untouched] == NAN_DST), "a slot outside dst_index changed"
    assert_within_fsum_bound(got[dst_index].view(np.float64), runs, ALPHA)
    bad = np.flatnonzero(got[dst_index] != want_img[dst_index])
    assert bad.size == 0, "runs %s (lengths %s) differ from the restated order" % (bad[:5], [len(runs[i]) for i in bad[:5]])


WAVE_LENS = [1, 31, 32, 63, 64, 65, 129, 300, 6] + [1] * 13        # 22 runs, 704 = 32 * 22 terms


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("form", ["wave", "thread"])
def test_csc_values_on_both_sides_of_the_form_switch(form, layout):
    """The rule (csrc/handoff.hip, not observable through the ABI): nnz_in >= 32 * nseg takes csc_values_wave_kernel (every lane starts at
    0.0, all 64 enter the tree), anything below takes csc_values_thread_kernel (left to right from the first term).  The same run
    structure exactly on the switch, and with ONE duplicate of the longest run removed just below it; each restated in its kernel's
    order.  (A run of -0.0 alone would give +0.0 in the wave form and -0.0 in the thread form: the two documented orders.)"""
    rng = np.random.default_rng(20267)
    lens = list(WAVE_LENS)
    assert sum(lens) == 32 * len(lens)
    if form == "thread":
        lens[7] -= 1
        assert sum(lens) == 32 * len(lens) - 1
    perm, seg = csc_structure(rng, lens)
    c = coeffs(rng, sum(lens))
    run_sum = (lambda r: g.run_sum_wave(r, False)) if form == "wave" else g.run_sum_sequential
    runs = runs_of(c, perm, seg)
    assert_orders_distinguishable(runs, False)
    assert_alpha_distinguishable(runs, ALPHA, run_sum)
    assert_within_fsum_bound([run_sum(r) for r in runs], runs)
    check_csc_values(c, perm, seg, 0, len(lens), layout, rng, run_sum)


@functools.lru_cache(maxsize=None)
def thread_form_data():
    rng = np.random.default_rng(20268)
    lens = [(1, 2, 40)[k % 3] for k in range(1025)]
    perm, seg = csc_structure(rng, lens)
    c = coeffs(rng, sum(lens))
    runs = runs_of(c, perm, seg)
    assert_orders_distinguishable(runs, False)
    assert_alpha_distinguishable(runs, ALPHA, g.run_sum_sequential)
    return c, perm, seg


@pytest.mark.parametrize("nseg,layout", [(1, "linear"), (255, "quadratic"), (256, "vector_affine"), (257, "linear"), (1025, "vector_affine")])
def test_csc_values_one_thread_per_run_over_256_thread_workgroups(nseg, layout):
    """runs of 1, 2 and 40 (fewer than 32 terms per run on average: the thread form); nseg around the workgroup size.  A single run in the
    thread form has fewer than 32 terms: the range of one run starts at a run of 2"""
    c, perm, seg = thread_form_data()
    lens = np.diff(seg)
    runs = runs_of(c, perm, seg)
    if nseg == 1:                                                                 # ... the first one that tells alpha per run from alpha per term
        first = next(s for s in np.flatnonzero(lens == 2) if not g.same_bits(ALPHA * (runs[s][0] + runs[s][1]), ALPHA * runs[s][0] + ALPHA * runs[s][1]))
    else:
        first = 0 if nseg == 1025 else 3
    assert int(seg[first + nseg] - seg[first]) < 32 * nseg                       # the thread form
    runs = runs[first:first + nseg]
    assert_alpha_distinguishable(runs, ALPHA, g.run_sum_sequential)
    if nseg > 1:
        assert sorted(set(len(r) for r in runs)) == [1, 2, 40]
        assert_orders_distinguishable(runs, False)
    check_csc_values(c, perm, seg, first, nseg, layout, np.random.default_rng(nseg), g.run_sum_sequential)


def test_csc_values_refuses_more_runs_than_terms():
    g.lib()
    z = torch.zeros(8, dtype=torch.int64, device=g.DEV)
    with pytest.raises(_lib.DimensionMismatch):
        g.call("pmt_csc_values_f64", g.ptr(z), 16, 3, g.ptr(z), g.ptr(z), 4, ALPHA, None, g.ptr(z), g.stream())
    with pytest.raises(_lib.DimensionMismatch):
        g.call("pmt_csc_values_gather_f64", g.ptr(z), 3, g.ptr(z), 4, ALPHA, None, g.ptr(z), g.stream())


# ---- 4. pmt_csc_values_gather_f64 ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gather_data():
    """1000 runs of 1, 2, 7 and 70 terms; every term lies in one of THREE term buffers (linear, quadratic, vector-affine with its coefficient
    at offset 8), at a random place of it: (buffer, slot) per term, in the input order of the terms"""
    rng = np.random.default_rng(20269)
    lens = [(1, 2, 7, 70)[k % 4] for k in range(1000)]
    perm, seg = csc_structure(rng, lens)
    n = sum(lens)
    c = coeffs(rng, n)
    buf = rng.integers(0, 3, n)
    slot = np.zeros(n, dtype=np.int64)
    for b in range(3):
        mine = np.flatnonzero(buf == b)
        slot[mine] = rng.permutation(len(mine))
    runs = runs_of(c, perm, seg)
    assert_orders_distinguishable(runs, True)
    assert_alpha_distinguishable(runs, ALPHA, g.run_sum_sequential)
    return c, perm, seg, buf, slot


@pytest.mark.parametrize("nseg", [1, 256, 257, 1000])
def test_csc_values_gather_reads_three_term_buffers_through_its_pointer_table(nseg):
    c, perm, seg, buf, slot = gather_data()
    lens = np.diff(seg)
    runs = runs_of(c, perm, seg)
    if nseg == 1:                                                                 # a single run: the first of 70 terms that tells the orders apart
        first = next(s for s in np.flatnonzero(lens == 70) if not g.same_bits(g.run_sum_wave(runs[s], True), g.run_sum_sequential(runs[s])))
    else:
        first = 0 if nseg == 1000 else 5
    runs = runs[first:first + nseg]
    if nseg > 1:
        assert sorted(set(len(r) for r in runs)) == [1, 2, 7, 70]
    assert_orders_distinguishable(runs, True)
    assert_alpha_distinguishable(runs, ALPHA, g.run_sum_sequential)
    for L in sorted(set(lens[first:first + nseg]) - {1}):                        # runs take their terms from more than one buffer
        assert any(len(set(buf[perm[seg[s]:seg[s + 1]]])) > 1 for s in range(first, first + nseg) if lens[s] == L), L
    rng = np.random.default_rng(nseg)
    dst_index, before = injection(rng, nseg)
    want_img = csc_values_image(before, runs, ALPHA, dst_index, g.run_sum_sequential)
    g.lib()
    sources, base, stride = [], np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.uint64)
    for b, layout in enumerate(("linear", "quadratic", "vector_affine")):
        mine = np.flatnonzero(buf == b)
        cb = np.zeros(len(mine))
        cb[slot[mine]] = c[mine]
        dt, p, st = term_source(cb, layout, rng)
        sources.append(dt)                                                    # alive until after the synchronise
        base[b], stride[b] = p.value, st
    addr = base[buf] + stride[buf] * slot.astype(np.uint64)                   # the coefficient's address, per term in input order
    table = addr[perm]                                                        # ... in CSC order: what the host folds once
    dtable, dseg, didx, dst = g.to_dev(table.view(np.int64)), g.to_dev(seg), g.to_dev(dst_index), g.to_dev(before)
    nnz_in = int(seg[first + nseg] - seg[first])
    g.call("pmt_csc_values_gather_f64", g.ptr(dtable), nnz_in, at(dseg, first), nseg, ALPHA, g.ptr(didx), g.ptr(dst), g.stream())
    got = host_words(dst)
    del sources
    untouched = np.setdiff1d(np.arange(2 * nseg), dst_index)
    assert np.all(got[untouched] == NAN_DST), "a slot outside dst_index changed"
    assert_within_fsum_bound(got[dst_index].view(np.float64), runs, ALPHA)
    bad = np.flatnonzero(got[dst_index] != want_img[dst_index])
    assert bad.size == 0, "runs %s (lengths %s) differ from the left-to-right order" % (bad[:5], [len(runs[i]) for i in bad[:5]])


# ---- 5. pmt_copy_2d_f64 -------------------------------------------------------------------------------------------------------------------
def copy_2d_image(before, base, data, column_start):
    """column j of `data` (rows x cols) lands at word base + column_start[j]; everything else as it was"""
    rows = data.shape[0]
    img = before.copy()
    idx = base + np.asarray(column_start, dtype=np.int64)[:, None] + np.arange(rows, dtype=np.int64)[None, :]
    img[idx.reshape(-1)] = bits(np.ascontiguousarray(data.T)).reshape(-1)
    return img


COPY_SHAPES = [(r, c) for r in (1, 63, 64, 65, 130) for c in (1, 3, 4, 5)] + [(3, 16389)]     # 16389 columns: more than the 16384 waves of the capped grid


@pytest.mark.parametrize("rows,cols", COPY_SHAPES)
def test_copy_2d_plain_and_offset_forms_touch_only_their_columns(rows, cols):
    rng = np.random.default_rng(1000 * rows + cols)
    data = coeffs(rng, rows * cols)
    data[0] = -0.0
    data = data.view(np.int64)
    data[-1] = NAN_DATA
    data = data.view(np.float64).reshape(cols, rows).T                           # column-major rows x cols
    spitch, dpitch = rows + 3, rows + 5
    src = copy_2d_image(np.full(1 + cols * spitch, NAN_SRC, dtype=np.int64), 1, data, np.arange(cols) * spitch)
    g.lib()
    dsrc = g.to_dev(src)
    # plain form, both bases shifted by 8 bytes
    before = np.full(1 + cols * dpitch + GUARD, NAN_DST, dtype=np.int64)
    want = copy_2d_image(before, 1, data, np.arange(cols) * dpitch)
    dst = g.to_dev(before)
    g.call("pmt_copy_2d_f64", at(dsrc, 1), spitch, at(dst, 1), dpitch, None, rows, cols, g.stream())
    got = host_words(dst)
    assert np.array_equal(got, want)
    # dst_offset form: irregular, strictly increasing offsets with gaps of different size; dst_pitch = 0
    gaps = 1 + rng.permutation(cols + 1) % 7
    offsets = (gaps[0] + np.concatenate([[0], np.cumsum(rows + gaps[1:cols])])).astype(np.int64)
    assert len(offsets) == cols and np.all(np.diff(offsets) >= rows + 1) and (cols < 3 or len(set(np.diff(offsets))) > 1)
    before = np.full(1 + int(offsets[-1]) + rows + GUARD, NAN_DST, dtype=np.int64)
    want = copy_2d_image(before, 1, data, offsets)
    dst, doff = g.to_dev(before), g.to_dev(offsets)
    g.call("pmt_copy_2d_f64", at(dsrc, 1), spitch, at(dst, 1), 0, g.ptr(doff), rows, cols, g.stream())
    got = host_words(dst)
    assert np.all(got[1 + int(offsets[-1]) + rows:] == NAN_DST), "the words behind the last column changed"
    assert np.array_equal(got, want)
    with pytest.raises(_lib.DimensionMismatch):
        g.call("pmt_copy_2d_f64", at(dsrc, 1), rows - 1, at(dst, 1), dpitch, None, rows, cols, g.stream())
    with pytest.raises(_lib.DimensionMismatch):
        g.call("pmt_copy_2d_f64", at(dsrc, 1), rows - 1, at(dst, 1), 0, g.ptr(doff), rows, cols, g.stream())


# ---- 6. pmt_qp_bounds_rows_f64 ------------------------------------------------------------------------------------------------------------
def qp_bounds_rows(value, const, kind, infty):
    """row i of f(x) in set, f = a'x + c: l = u = v - c (EQUAL 0) | l = v - c, u = +infty (GREATER 1) | l = -infty, u = v - c (LESS 2)"""
    b = value - const
    return np.where(kind == 2, -infty, b), np.where(kind == 1, infty, b)


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 1000])
def test_qp_bounds_rows_reads_each_constant_through_its_own_pointer(rows):
    rng = np.random.default_rng(rows)
    infty = 1e20
    sizes = (rows // 3 + 1, rows // 2 + 1, rows)                                   # three separate constant buffers
    consts = [coeffs(rng, k) for k in sizes]
    for cb in consts:
        cb[::3] = -0.0
    which = rng.integers(0, 3, rows)
    where = np.array([rng.integers(0, sizes[b]) for b in which], dtype=np.int64)    # shuffled: row i reads buffer which[i] at where[i]
    const = np.array([consts[b][k] for b, k in zip(which, where)])
    kind = rng.integers(0, 3, rows).astype(np.int32)
    value = coeffs(rng, rows)
    value[::4] = -0.0
    value[1::4] = 0.0
    want_l, want_u = qp_bounds_rows(value, const, kind, infty)
    g.lib()
    dconsts = [g.to_dev(cb) for cb in consts]
    table = np.array([dconsts[b].data_ptr() for b in which], dtype=np.uint64) + 8 * where.astype(np.uint64)
    dtable, dkind, dvalue = g.to_dev(table.view(np.int64)), g.to_dev(kind), g.to_dev(value)
    before = np.full(rows + GUARD, NAN_DST, dtype=np.int64)
    dl, du = g.to_dev(before), g.to_dev(before)
    g.call("pmt_qp_bounds_rows_f64", g.ptr(dtable), g.ptr(dkind), g.ptr(dvalue), rows, infty, g.ptr(dl), g.ptr(du), g.stream())
    got_l, got_u = host_words(dl), host_words(du)
    del dconsts
    assert np.all(got_l[rows:] == NAN_DST) and np.all(got_u[rows:] == NAN_DST)
    assert np.array_equal(got_l[:rows], bits(want_l)) and np.array_equal(got_u[:rows], bits(want_u))
    g.call("pmt_qp_bounds_rows_f64", g.ptr(dtable), g.ptr(dkind), g.ptr(dvalue), 0, infty, g.ptr(dl), g.ptr(du), g.stream())
    assert np.array_equal(host_words(dl), got_l)


# ---- 7. csrc/terms.hip launched directly ------------------------------------------------------------------------------------------------------
TRANSPOSE_SHAPES = [(1, 1), (1, 70), (70, 1), (31, 33), (32, 32), (33, 31), (64, 96), (65, 97), (100, 257)]


def transpose_case(rows, cols, pad):
    """A[i, j] = i + 1000 j, column-major with leading dimension rows + pad; dest = A' with leading dimension cols + pad; NaN padding"""
    lds, ldd = rows + pad, cols + pad
    A = np.arange(rows, dtype=np.float64)[:, None] + 1000.0 * np.arange(cols, dtype=np.float64)[None, :]
    src = copy_2d_image(np.full(cols * lds + GUARD, NAN_SRC, dtype=np.int64), 0, A, np.arange(cols) * lds)
    before = np.full(rows * ldd + GUARD, NAN_DST, dtype=np.int64)
    want = copy_2d_image(before, 0, np.ascontiguousarray(A.T), np.arange(rows) * ldd)
    return lds, ldd, src, before, want


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("rows,cols", TRANSPOSE_SHAPES)
def test_transpose_ragged_tiles_and_padded_leading_dimensions(rows, cols, pad):
    lds, ldd, src, before, want = transpose_case(rows, cols, pad)
    g.lib()
    dsrc, dst = g.to_dev(src), g.to_dev(before)
    g.call("pmt_transpose_f64", g.ptr(dsrc), lds, rows, cols, g.ptr(dst), ldd, g.stream())
    assert np.array_equal(host_words(dst), want)
    assert np.array_equal(host_words(dsrc), src)


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("rows,cols", TRANSPOSE_SHAPES)
def test_transpose_as_a_fused_plan_node(rows, cols, pad):
    """the interpreter's SOP_TRANSPOSE (csrc/small.hip) against numpy — not against the unfused run.  A run of the interpreter has at
    least two nodes: a one-element scale!(dest, s, y) rides along"""
    lds, ldd, src, before, want = transpose_case(rows, cols, pad)
    g.lib()
    dsrc, dst = g.to_dev(src), g.to_dev(before)
    y, out = g.to_dev(np.array([3.0])), g.empty_f64(1)
    plan = C.c_void_p()
    g.call("pmt_plan_create", 0, g.stream(), C.byref(plan))
    try:
        rec = C.c_void_p(g.lib().pmt_plan_recording_stream(plan))
        g.call("pmt_plan_begin_record", plan)
        g.call("pmt_transpose_f64", g.ptr(dsrc), lds, rows, cols, g.ptr(dst), ldd, rec)
        g.call("pmt_scale_numbers_f64", g.ptr(y), 1, None, 0.5, g.ptr(out), rec)
        g.call("pmt_plan_end_record", plan)
        groups, nodes, launches = C.c_int(), C.c_int(), C.c_int64()
        g.call("pmt_plan_fused", plan, C.byref(groups), C.byref(nodes), C.byref(launches))
        assert (groups.value, nodes.value, launches.value) == (1, 2, 1), "the transpose was not fused"
        g.call("pmt_plan_update", plan)
        assert np.array_equal(host_words(dst), want)
        assert g.f64_to_host(out, 1)[0] == 1.5
    finally:
        torch.cuda.synchronize()
        g.call("pmt_plan_destroy", plan)


def quad_terms(rng, n, first_index=1):
    t = np.zeros(n, dtype=g.QT)
    t["coeff"] = coeffs(rng, n)
    t["coeff"][::5] = 0.0
    t["coeff"][1::5] = -0.0
    t["row"], t["col"] = first_index + np.arange(n), rng.integers(1, 1 << 40, n)
    return t


@pytest.mark.parametrize("sb", [1, -1])
@pytest.mark.parametrize("na,nb", [(0, 5), (5, 0), (255, 2), (256, 257), (70000, 3)])
def test_quad_combine_copies_the_first_part_and_signs_the_second(na, nb, sb):
    """out = [qa ; sb * qb]: the sign flips the coefficients of the second part only (0.0 -> -0.0 too); indices are copied"""
    rng = np.random.default_rng(na + 7 * nb)
    qa, qb = quad_terms(rng, na), quad_terms(rng, nb, 10 ** 6)
    want = np.concatenate([qa, qb])
    if sb < 0:
        want["coeff"][na:] = -qb["coeff"]
    before = words(3 * (na + nb) + GUARD)
    want_img = np.concatenate([want.view(np.int64), before[3 * (na + nb):]])
    g.lib()
    da, db, out = (g.to_dev(qa) if na else None), (g.to_dev(qb) if nb else None), g.to_dev(before)
    g.call("pmt_quad_combine_f64", g.ptr(da), na, g.ptr(db), nb, sb, g.ptr(out), g.stream())
    assert np.array_equal(host_words(out), want_img)


@pytest.mark.parametrize("n", [1, 257, 70000])
def test_quad_scale_device_scalar_and_immediate(n):
    """out = (s * coeff, row, col), one product per term; the device scalar wins over the immediate when both are given"""
    rng = np.random.default_rng(n)
    q = quad_terms(rng, n)
    before = words(3 * n + GUARD)
    g.lib()
    dq, ds = g.to_dev(q), g.to_dev(np.array([ALPHA]))
    for s_dev, s_host, s in ((ds, 9.0, ALPHA), (None, 3.7, 3.7)):
        want = q.copy()
        want["coeff"] = s * q["coeff"]
        out = g.to_dev(before)
        g.call("pmt_quad_scale_f64", g.ptr(dq), n, g.ptr(s_dev), s_host, g.ptr(out), g.stream())
        assert np.array_equal(host_words(out), np.concatenate([want.view(np.int64), before[3 * n:]]))


@pytest.mark.parametrize("n", [1, 256, 257])
def test_scale_vars_writes_the_scalar_beside_every_variable(n):
    """scale!(dest, s, y::Vector{Variable}): dest[i] = (s, yvar[i])"""
    rng = np.random.default_rng(n)
    yvar = rng.integers(1, 1 << 40, n).astype(np.int64)
    before = words(2 * n + GUARD)
    g.lib()
    dy, ds = g.to_dev(yvar), g.to_dev(np.array([ALPHA]))
    for s_dev, s_host, s in ((ds, 9.0, ALPHA), (None, -0.0, -0.0)):
        want = np.zeros(n, dtype=g.LT)
        want["coeff"], want["var"] = s, yvar
        out = g.to_dev(before)
        g.call("pmt_scale_vars_f64", g.ptr(dy), n, g.ptr(s_dev), s_host, g.ptr(out), g.stream())
        assert np.array_equal(host_words(out), np.concatenate([want.view(np.int64), before[2 * n:]]))
