"""-m gpu: the batched-instance entry points at the C ABI — pmt_batch_lsq_coeffs_f64 (csrc/batch_small.hip up to 128 columns, the tiled general path
beyond) and pmt_batch_expand_f64 — with chosen data, both signs passed separately, slabs placed at every alignment and pitch, and every
output inside a guarded buffer whose WHOLE image is compared bit for bit: guards in front and behind and the out_stride - L words between
two slabs must still hold the poison.

The data is dyadic (tests/batch_util.py): Q, q and c'c are exact in every summation order, so the expected slab is plain numpy and the
comparison needs no restated MFMA order — an entry swapped with its neighbour, or taken from the neighbouring instance, differs.  Batches of
B_many = 2 CUs + 37 instances give every persistent workgroup two or three instances, which is where the pipeline that runs on across
instance boundaries, the reuse of the LDS staging buffer and the copy-out that overlaps the next instance operate.
tests/test_batch_slab_host.py checks the numpy restatement against the oracle.

Not covered: B > 65535 on the general path (the gridDim.y split needs a 4 GB output); non-finite data under sign_b = 0 is not specified."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import batch_util as U  # noqa: E402

B_FEW = 3


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def b_many():
    return 2 * cus() + 37


def dev_f64(a, shift=0):
    """device copy of a float64 array (at least one element, so that the pointer is valid); shift = 1: first element 8 bytes behind a 16-byte boundary"""
    import gpu_util as g
    flat = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    t = torch.zeros(max(len(flat), 1) + shift, dtype=torch.float64, device=g.DEV)
    if len(flat):
        t[shift:shift + len(flat)] = torch.from_numpy(flat)
    assert t.data_ptr() % 16 == 0
    return t, C.c_void_p(t.data_ptr() + 8 * shift)


class Batch:
    """a batch in the device layout, on the host and on the device"""

    def __init__(self, B, n, r, m, seed, gen=U.dyadic, a_shift=0):
        self.B, self.n, self.r, self.m = B, n, r, m
        self.host = U.batch_data(B, n, r, m, np.random.default_rng(seed), gen)
        self.upload(a_shift)

    def upload(self, a_shift=0):
        self.dev = [dev_f64(self.host[0], a_shift)] + [dev_f64(h) for h in self.host[1:]]

    def reference(self, sign_b, sign_d):
        return U.slab_reference_batch(*self.host, sign_b, sign_d)

    def run(self, sign_b=-1, sign_d=-1, gap=0, shift=0):
        """-> (Guarded output of B * out_stride doubles, out_stride)"""
        import gpu_util as g
        L = U.slab_doubles(self.n, self.m)
        assert L == g.lib().pmt_batch_lsq_slab_doubles(self.n, self.m)
        stride = L + gap
        out = g.Guarded(self.B * stride, doubles=True, shift=shift)
        g.call("pmt_batch_lsq_coeffs_f64", self.dev[0][1], self.dev[1][1], self.dev[2][1], self.dev[3][1], self.B, self.n, self.r, self.m, sign_b, sign_d,
               out.ptr(), stride, g.stream())
        return out, stride


def image(out, slabs, stride):
    """the expected content of a Guarded output: the slabs at their pitch, poison between them"""
    B, L = slabs.shape
    img = out.padding((B, stride))
    img[:, :L] = slabs
    return img


def owned(out):
    torch.cuda.synchronize()
    return out.buf.cpu().numpy()[out.off:out.off + out.n].copy()


@functools.lru_cache(maxsize=2)
def dyadic_batch(B, n, r, m):
    return Batch(B, n, r, m, seed=7 + 1000 * n + 10 * r + m)


def check_batch(bt, sign_b=-1, sign_d=-1, gap=0, shift=0, what=""):
    out, stride = bt.run(sign_b, sign_d, gap, shift)
    out.check(image(out, bt.reference(sign_b, sign_d), stride), "%s n=%d r=%d m=%d B=%d signs (%d, %d) gap %d shift %d" % (what, bt.n, bt.r, bt.m, bt.B, sign_b, sign_d, gap, shift))


# ---- a. the small path

@pytest.mark.parametrize("many", [True, False], ids=["B_many", "B_few"])
@pytest.mark.parametrize("n,r,m", [c[:3] for c in U.SMALL_CASES], ids=["%dx%dx%d" % c[:3] for c in U.SMALL_CASES])
def test_small_path_slabs_are_the_reference_bit_for_bit(n, r, m, many):
    check_batch(dyadic_batch(b_many() if many else B_FEW, n, r, m), what="small path")


def test_small_path_with_A_eight_bytes_off_a_16_byte_boundary():
    """128 x 64 x 16 would take the aligned 16-byte loads; the base alone sends it down the bounds-checked path"""
    check_batch(Batch(b_many(), 128, 64, 16, seed=3, a_shift=1), what="shifted A")


# ---- b. output placement: all slabs aligned, all shifted, alternating — for both parities of L

@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("gap", [0, 1, 6])
@pytest.mark.parametrize("n,r,m", U.POSITION_SHAPES)
def test_output_placement(n, r, m, gap, shift):
    check_batch(dyadic_batch(b_many(), n, r, m), gap=gap, shift=shift, what="placement")


# ---- c. the two signs are two arguments

@pytest.mark.parametrize("sign_d", [-1, 0, 1])
@pytest.mark.parametrize("sign_b", [-1, 0, 1])
@pytest.mark.parametrize("n,r,m", U.SIGN_SHAPES)
def test_all_sign_pairs(n, r, m, sign_b, sign_d):
    bt = dyadic_batch(b_many() if n <= U.SMALL_MAX_N else 5, n, r, m)
    want = bt.reference(sign_b, sign_d)
    sec = U.sections(n, m)
    zero = np.zeros(1).view(np.int64)[0]
    assert np.any(bt.host[0] < 0) and np.any(bt.host[1] < 0)                   # products with c = +0.0 are -0.0: the sums must still be +0.0
    if sign_b == 0:
        assert np.all(want[:, sec["q"]].view(np.int64) == zero) and np.all(want[:, sec["const"]].view(np.int64) == zero)
    if sign_d == 0:
        assert np.all(want[:, sec["d"]].view(np.int64) == zero)
    out, stride = bt.run(sign_b, sign_d, gap=1)
    out.check(image(out, want, stride), "signs (%d, %d) at %d x %d x %d" % (sign_b, sign_d, n, r, m))


# ---- d. the general path (more than 128 columns)

@pytest.mark.parametrize("B", [5, 70])
@pytest.mark.parametrize("n,r,m,gap3,a_shift", U.GENERAL_CASES)
def test_general_path_slabs_are_the_reference_bit_for_bit(n, r, m, gap3, a_shift, B):
    bt = Batch(B, n, r, m, seed=n + r + m + B, a_shift=1 if a_shift else 0)
    check_batch(bt, sign_b=1 if gap3 else -1, sign_d=-1 if gap3 else 1, gap=3 if gap3 else 0, what="general path")


# ---- e. no variables: the slab is [c'c | d-consts]

def test_instances_without_variables_still_get_their_constant():
    check_batch(Batch(4, 0, 5, 3, seed=9), sign_b=-1, sign_d=1, gap=2, what="n == 0")
    check_batch(Batch(4, 0, 5, 0, seed=9), what="n == 0, m == 0")


# ---- f. instances do not see each other

@pytest.mark.parametrize("n,r,m", U.ISOLATION_SHAPES)
def test_nan_in_one_instance_stays_in_its_slab(n, r, m):
    """NaN sits in input DATA only (no address depends on it): A, b, C and d of three instances — the first on its workgroup, a second one,
    and the last of the batch.  Every other slab keeps the bits of the clean run; a poisoned slab is NaN throughout Q, q and const and
    carries its constraint block (C as it is, 0.0 + d) bit for bit."""
    B, G = b_many(), cus()
    bt = Batch(B, n, r, m, seed=21 + n)
    clean, stride = bt.run(-1, 1, gap=1)
    want = bt.reference(-1, 1)
    clean.check(image(clean, want, stride), "clean run")
    victims = [3, G + 5, B - 1]
    assert all(v // G == k for v, k in zip(victims[:2], (0, 1))) and B - 1 >= 2 * G
    for h in bt.host:
        h[victims] = np.nan
    bt.upload()
    out, stride = bt.run(-1, 1, gap=1)
    got = owned(out).reshape(B, stride)
    sec = U.sections(n, m)
    At, b, Ct, d = bt.host
    for v in victims:
        assert np.isnan(got[v, :sec["C"].start]).all(), "instance %d: Q, q or const holds a number" % v
        want[v, :sec["C"].start] = got[v, :sec["C"].start]
        want[v, sec["C"]] = Ct[v].T.reshape(-1)
        want[v, sec["d"]] = 0.0 + d[v]
    out.check(image(out, want, stride), "three poisoned instances")


# ---- g. position independence on full-mantissa data

def centred(shape, rng):
    return rng.random(shape) - 0.5


@pytest.mark.parametrize("n,r,m", U.POSITION_SHAPES)
def test_a_slab_does_not_depend_on_the_instance_s_position(n, r, m):
    """Six instances of a B_many batch — first, second and third on a workgroup, and the last: the same bits in place as computed alone, and
    inside the bound of an r-term inner product around the exact value (Python integers from the doubles' own mantissas), which needs no
    measured tolerance: |Q_jk - 2 sum a_ij a_ik| <= (r + 2) 2^-53 * 2 sum |a_ij| |a_ik|, for q with c_i in place of a_ik."""
    B, G = b_many(), cus()
    bt = Batch(B, n, r, m, seed=33 + n, gen=centred)
    out, stride = bt.run()
    got = owned(out).reshape(B, stride)
    sec = U.sections(n, m)
    L = U.slab_doubles(n, m)
    # const (left to right), C and the d-consts do not depend on a summation order of the kernel's: bit for bit, as are the guards and gaps
    want = bt.reference(-1, -1)
    want[:, :sec["const"].start] = got[:, :sec["const"].start]
    out.check(image(out, want, stride), "in place")
    picks = [0, 5, G, G + 7, 2 * G + 3, B - 1]
    assert [p // G for p in picks] == [0, 0, 1, 1, 2, 2]
    iu = np.triu_indices(n)
    At, b, Ct, d = bt.host
    for i in picks:
        alone = Batch(1, n, r, m, seed=0)
        alone.host = tuple(np.ascontiguousarray(h[i:i + 1]) for h in bt.host)
        alone.upload()
        o1, _ = alone.run()
        o1.check(got[i:i + 1, :L], "instance %d alone against in place" % i)
        S, Sabs, s, sabs, k2 = U.exact_gram(At[i], 0.0 - b[i])
        okQ = U.within_inner_product_bound(got[i, sec["Q"]], S[iu], Sabs[iu], k2, r)
        okq = U.within_inner_product_bound(got[i, sec["q"]], s, sabs, k2, r)
        assert okQ.all() and okq.all(), "instance %d: %d Q and %d q entries outside the inner-product bound" % (i, (~okQ).sum(), (~okq).sum())


# ---- h. pmt_batch_expand_f64

@pytest.mark.parametrize("m", [0, 1, 5])
@pytest.mark.parametrize("n", [1, 2, 3, 127, 128, 129, 200, 1024])
def test_expand_carries_every_word_to_its_term(n, m):
    """The slab holds float(i) at word i, so every term must carry its own word; xvar increases with gaps; varmap a permutation, and NULL
    (native indices).  n = 1024: more than 2048 x 256 words, the grid-stride loop wraps."""
    import gpu_util as g
    L = U.slab_doubles(n, m)
    assert (L > 2048 * 256) == (n == 1024)
    nq = n * (n + 1) // 2
    rng = np.random.default_rng(n + m)
    xvar = np.cumsum(rng.integers(1, 4, size=n)).astype(np.int64)
    perm = (rng.permutation(int(xvar[-1])) + 1).astype(np.int64)
    slab = np.arange(L, dtype=np.float64)
    iu = np.triu_indices(n)
    d_slab, d_x, d_perm = g.to_dev(slab), g.to_dev(xvar), g.to_dev(perm)
    for varmap, d_map in ((perm, d_perm), (None, None)):
        mapped = xvar if varmap is None else varmap[xvar - 1]
        q = np.empty(nq, dtype=g.QT)
        q["coeff"], q["row"], q["col"] = slab[:nq], mapped[iu[0]], mapped[iu[1]]
        lin = np.empty(n, dtype=g.LT)
        lin["coeff"], lin["var"] = slab[nq:nq + n], mapped
        vat = np.empty(m * n, dtype=g.VAT)
        vat["out"], vat["coeff"], vat["var"] = np.repeat(np.arange(1, m + 1), n), slab[nq + n + 1:nq + n + 1 + m * n], np.tile(mapped, m)
        oq, ol, ov = g.Guarded(3 * nq, doubles=False), g.Guarded(2 * n, doubles=False), g.Guarded(3 * m * n, doubles=False)
        oc, ovc = g.Guarded(1, doubles=True), g.Guarded(m, doubles=True)
        g.call("pmt_batch_expand_f64", g.ptr(d_slab), n, m, g.ptr(d_x), g.ptr(d_map), oq.ptr(), ol.ptr(), oc.ptr(), ov.ptr(), ovc.ptr(), g.stream())
        tag = "n=%d m=%d %s" % (n, m, "varmap" if varmap is not None else "native")
        oq.check(q.view(np.int64), "quadratic terms " + tag)
        ol.check(lin.view(np.int64), "affine terms " + tag)
        oc.check(slab[nq + n:nq + n + 1], "constant " + tag)
        ov.check(vat.view(np.int64), "constraint terms " + tag)
        ovc.check(slab[nq + n + 1 + m * n:], "constraint constants " + tag)
