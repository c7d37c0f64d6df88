"""-m gpu: the literal term builders (csrc/quad.hip, csrc/terms.hip, the MOI packs of csrc/affine.hip) and their second implementation, the
small-plan interpreter (csrc/small.hip: sp_node), at their tile, wave and grid edges — against the oracle, bit for bit.

Every operation here is a copy, a sign flip, one product or a fixed-order sum: there is no tolerance in this file.  Every output lives in a
gpu_util.Guarded buffer (poisoned guard words on both sides and in any leading-dimension padding; the whole image is compared); every
24-byte-term output runs at a 16-byte-aligned base and at one shifted by a word; the data family (term_builders_util.family / variables)
has both zeros, denormals, both signs, duplicate and shared variables, and every MOI copy goes through a permuting varmap.  The cases of
5e5 elements and more compare with term_builders_util's numpy restatements (checked against the oracle in test_term_builders_host.py).

Boundary -> case (constants as in the sources: QE_BT = 1024, QE_AB = 8, 256 threads, 64 lanes, 32 x 32 tiles, grids of 256*8 / 256*16):

  bilinear_kernel      one term / non-square either way            BILINEAR (1,1) (3,5) (5,3)
                       second column block of ONE term, div/mod    (7,1025)   [nxr < 1024: many columns per block row]
                       three column blocks                         (2,2049)
                       nxr == QE_BT (first shape of the wrap path) (1024,3)
                       wrap branch, 1 and 2 column blocks, double
                       buffering over many rows                    (1030,5) (1030,1100)
                       block rows beyond gridDim.y = 65535         (65537,1) (65600,2)
                       ldq > rows (NaN padding rows), moi 0 / 1    every shape: pad 0 and 3
  write_qt_segment     segment's first word on either parity       every bilinear / quad_expand case: shift 0 and 1; odd ny
  quad_expand_kernel   nx across QE_AB, ny across QE_BT, x != y    QUAD_EXPAND (2,9,1025)
                       rows beyond gridDim.z = 65535               (65539,1,1) (65539,4,5)
  quad_expand_linear   idx / w non-trivial                         (600,30,30)
                       beyond one pass of 524288                   (65539,4,5): 589851 elements
  seq_dot_kernel<0/1>  both sides of each 64-product round         QUAD_EXPAND rows 63 64 65 100 128 129 200 (x != y; x . x);
                                                                   SEQ_DOT n 63 64 65 100 129 (numbers . affs)
                       rows = 0: constant 0.0, nothing else        (0,2,3)
  one thread / element last thread of a block, first of the next   ELEMENTWISE n 1 255 256 257 513
  grid-strided kernels one below / above one pass, above two;      STRIDED: 524287 524289 1048577 elements (matvecmul_affs:
                       quadratic | linear boundary inside a pass   1048575 1048577 2097153)
                       L = 0, rows = 1, na = 0, nb = 0, sb = -1,
                       scalar from the device / the host           SMALL_EDGES
  matvecmul consts     64-thread blocks, column-order sum          MATVEC rows 1 63 64 65 130, cols 3, L 2, lda = rows + 1
  pack_scalar_quadratic LDS path | per-thread path, full and       PACK_SQ n 1 255 256 257 511 512 513, input and output base each
                       partial blocks                              aligned / shifted
  pack_vector_affine,  one wave per row, 64 terms per round, four  PACK_VA row_len 0 1 63 64 65 129 x rows 1 4 5 9, ragged
  wave_write_words     rows per workgroup; segment parity          0 1 64 65 200 0 3, row_offset 11, shift 0 and 1
  affvec_combine       the same walk; a | b | both, sb, null parts COMBINE row lengths 0 1 64 65 130, rows 5 and 9, ragged
  transpose_kernel     partial tiles both ways, several tiles,     TRANSPOSE (1,1) (31,33) (32,32) (33,31) (1,65) (65,1) (64,96)
                       padded leading dimensions                   (100,37), leading dimensions tight and + 3
  sp_node              all of the above that write <= 32768        test_interpreter_*: the same cases recorded on plans and replayed
                       elements; narrow-node switch (256 | 257),   FUSED (pmt_plan_fused), compared with the oracle directly;
                       the 1024-thread stride (1023 1024 1025)     COUNTS n 256 257 1023 1024 1025
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_util as g  # noqa: E402
import term_builders_util as T  # noqa: E402
from oracle import oracle as O  # noqa: E402

NV = 5
VM = T.permuting_varmap(NV, 3)
NODE_MAX = 32768                       # SMALL_NODE_WORK_MAX (csrc/common.h; test_large_nodes_keep_their_own_kernels)
SHIFTS = (0, 1)


class Case:
    """inputs on the device, guarded outputs with what they must hold, and the calls in between (issued on a stream or recorded on a plan)"""

    def __init__(self, name):
        self.name, self.keep, self.calls, self.outs, self.small = name, [], [], [], True
        self.work = 0

    def dev(self, a, shift=0):
        """device copy of `a` (None stays NULL; an empty array gets a valid address nobody reads); shift = 1: based one word off 16 bytes"""
        if a is None:
            return None
        a = np.ascontiguousarray(a).reshape(-1)
        if a.dtype.fields is not None:
            a = a.view(np.int64)
        t = torch.zeros(len(a) + 2, dtype=torch.int64, device=g.DEV)
        if len(a):
            t[shift:shift + len(a)] = torch.from_numpy(a.view(np.int64).copy()).to(g.DEV)
        self.keep.append(t)
        assert t.data_ptr() % 16 == 0
        return g.C.c_void_p(t.data_ptr() + 8 * shift)

    def out(self, want, shift=0, what=""):
        want = np.ascontiguousarray(want)
        buf = g.Guarded(want.nbytes // 8, doubles=(want.dtype == np.float64), shift=shift)
        self.outs.append((buf, want, what))
        return buf

    def call(self, name, work, *args, fusable=True):
        """`work`: the elements the entry writes as the library counts them (the SmallNode's work in the entry point's source)"""
        self.calls.append((name, args))
        self.work += work
        if work > NODE_MAX or not fusable:
            self.small = False

    def issue(self, stream):
        for name, args in self.calls:
            g.call(name, *args, stream)

    def check(self):
        for buf, want, what in self.outs:
            buf.check(want, "%s %s" % (self.name, what))

    def run(self):
        self.issue(g.stream())
        self.check()


def run_all(cases):
    for c in cases:
        c.run()


def colmajor_padded(A, ld):
    """rows x cols -> the column-major image with leading dimension ld, the padding rows NaN"""
    P = np.full((ld, A.shape[1]), np.nan)
    P[:A.shape[0]] = A
    return np.ascontiguousarray(P.T).reshape(-1)


def matrix(rows, cols, seed):
    return T.family(rows * cols, seed).reshape(cols, rows).T.copy()


def quad_of(q):
    return O.Quad(quad=[(float(c), int(r), int(cl)) for c, r, cl in zip(q["coeff"], q["row"], q["col"])])


def lt_of(coeff, var):
    t = np.empty(len(coeff), dtype=g.LT)
    t["coeff"], t["var"] = coeff, var
    return t


# ------------------------------------------------------------------ bilinearmul!
BILINEAR = [(1, 1), (3, 5), (5, 3), (7, 1025), (2, 2049), (1024, 3), (1030, 5), (1030, 1100), (65537, 1), (65600, 2)]


@functools.lru_cache(maxsize=None)
def bilinear_ref(rows, cols):
    Q = matrix(rows, cols, 100 + (rows + 3 * cols) % 89)
    x, y = T.variables(rows, 11, NV), T.variables(cols, 12, NV)
    y[0] = x[0]                                                          # (a doubled term also in the one-term shapes)
    ref = O.Quad().bilinearmul(Q, x, y)
    return Q, x, y, ref.terms(), ref.moi(VM)[1]


def bilinear_cases(shape):
    rows, cols = shape
    Q, x, y, native, moi_terms = bilinear_ref(rows, cols)
    assert min(rows, cols) <= 2 or not np.array_equal(x[:min(rows, cols)], y[:min(rows, cols)])       # different vectors that share variables
    cases = []
    for moi in (0, 1):
        for pad in (0, 3):
            for shift in SHIFTS:
                c = Case("bilinear %dx%d moi=%d ldq=rows+%d shift=%d" % (rows, cols, moi, pad, shift))
                oq = c.out(moi_terms if moi else native, shift, "quad")
                c.call("pmt_bilinear_f64", rows * cols, c.dev(colmajor_padded(Q, rows + pad)), rows + pad, rows, cols, c.dev(x), c.dev(y), moi,
                       c.dev(VM) if moi else None, oq.ptr())
                cases.append(c)
    return cases


@pytest.mark.parametrize("shape", BILINEAR, ids=str)
def test_bilinear(shape):
    run_all(bilinear_cases(shape))


# ------------------------------------------------------------------ literal x . y of affine vectors
QUAD_EXPAND = [(63, 2, 3), (64, 2, 3), (65, 2, 3), (100, 2, 3), (128, 2, 3), (129, 2, 3), (200, 2, 3), (2, 9, 1025), (65539, 1, 1), (600, 30, 30), (65539, 4, 5),
               (0, 2, 3)]
QUAD_EXPAND_SAME = [(63, 2, 2), (64, 2, 2), (65, 2, 2), (100, 2, 2), (129, 2, 2)]


@functools.lru_cache(maxsize=None)
def quad_expand_ref(rows, nx, ny, same):
    xt, xc = T.uniform_affvec(rows, nx, 200, NV)
    yt, yc = (xt, xc) if same else T.uniform_affvec(rows, ny, 300, NV)
    if rows == 0:                                                        # zero!(dest) and no row to add: the constant is 0.0
        return xt, xc, yt, yc, (None, None, 0.0), (None, None, 0.0)
    if rows * (nx + ny) >= 500000:                                       # the oracle's objects would take seconds: the numpy restatement
        return xt, xc, yt, yc, T.quad_expand(xt, xc, yt, yc), T.quad_expand(xt, xc, yt, yc, 1, VM)
    ref = O.Quad().vecdot_affs_affs(T.oracle_affvec(xt, xc), T.oracle_affvec(yt, yc))
    at, qt, const = ref.moi(VM)
    return xt, xc, yt, yc, (ref.terms(), ref.affine.terms(), ref.affine.constant), (qt, at, const)


def quad_expand_cases(shape, same=False):
    rows, nx, ny = shape
    xt, xc, yt, yc, native, moi_ref = quad_expand_ref(rows, nx, ny, same)
    cases = []
    for moi in (0, 1):
        for shift in SHIFTS:
            c = Case("quad_expand %s%s moi=%d shift=%d" % (shape, " x.x" if same else "", moi, shift))
            q, lin, const = moi_ref if moi else native
            if rows == 0:                                                # nothing but the constant is written
                q, lin = np.full(6, g.POISON_WORD, dtype=np.int64), np.full(6, g.POISON_WORD, dtype=np.int64)
            oq, ol, oc = c.out(q, shift, "quad"), c.out(lin, 0, "lin"), c.out(np.array([const]), 0, "const")
            dxt, dxc = c.dev(xt), c.dev(xc)
            dyt, dyc = (dxt, dxc) if same else (c.dev(yt), c.dev(yc))
            work = rows * nx * ny + rows * (nx + ny) + 16 * rows
            c.call("pmt_quad_expand_f64", work, rows, dxt, nx, dxc, dyt, ny, dyc, moi, c.dev(VM) if moi else None, oq.ptr(), ol.ptr(), oc.ptr(),
                   fusable=rows <= 2048)
            cases.append(c)
    return cases


@pytest.mark.parametrize("shape", QUAD_EXPAND, ids=str)
def test_quad_expand(shape):
    run_all(quad_expand_cases(shape))


@pytest.mark.parametrize("shape", QUAD_EXPAND_SAME, ids=str)
def test_quad_expand_of_a_vector_with_itself(shape):
    run_all(quad_expand_cases(shape, same=True))


# ------------------------------------------------------------------ one thread per element
ELEMENTWISE = [1, 255, 256, 257, 513]
COUNTS = [256, 257, 1023, 1024, 1025]


def vecdot_terms_cases(n):
    a, b = T.family(n, 21), T.family(n, 22)
    x, y = T.variables(n, 23, NV), T.variables(n, 24, NV)
    cases = []
    for xc, yc in ((a, b), (a, None), (None, b), (None, None)):
        ref = O.Quad().vecdot_terms_terms(list(zip((xc if xc is not None else np.ones(n)).tolist(), x.tolist())),
                                          list(zip((yc if yc is not None else np.ones(n)).tolist(), y.tolist())))
        for moi in (0, 1):
            for shift in SHIFTS:
                c = Case("vecdot_terms n=%d xc=%s yc=%s moi=%d shift=%d" % (n, xc is not None, yc is not None, moi, shift))
                oq = c.out(ref.moi(VM)[1] if moi else ref.terms(), shift, "quad")
                c.call("pmt_vecdot_terms_f64", n, n, c.dev(xc), c.dev(x), c.dev(yc), c.dev(y), moi, c.dev(VM) if moi else None, oq.ptr())
                cases.append(c)
    return cases


def elementwise_cases(n):
    cases = vecdot_terms_cases(n)
    v, x = T.family(n, 25), T.variables(n, 26, NV)
    # numbers . variables
    c = Case("vecdot_numbers_vars n=%d" % n)
    r = O.vecdot_aff_numbers_vars(v, x)
    ot, oc = c.out(r.terms(), 0, "terms"), c.out(np.array([r.constant]), 0, "const")
    c.call("pmt_vecdot_numbers_vars_f64", n + 1, c.dev(v), c.dev(x), n, ot.ptr(), oc.ptr())
    cases.append(c)
    # s * variables: the scalar from the device (wins over the immediate) and from the host
    for s_dev, s_host in ((np.array([-1.75]), 9.0), (None, -0.0)):
        c = Case("scale_vars n=%d dev=%s" % (n, s_dev is not None))
        ot = c.out(O.scale_number_vars(float(s_dev[0]) if s_dev is not None else s_host, x), 0, "terms")
        c.call("pmt_scale_vars_f64", n, c.dev(x), n, c.dev(s_dev), s_host, ot.ptr())
        cases.append(c)
    # MOI copy of an affine function
    c = Case("pack_scalar_affine n=%d" % n)
    ot = c.out(O.aff_moi(O.Aff(terms=list(zip(v.tolist(), x.tolist()))), VM)[0], 0, "terms")
    c.call("pmt_pack_scalar_affine_f64", n, c.dev(lt_of(v, x)), n, c.dev(VM), ot.ptr())
    cases.append(c)
    # variables (+|-) numbers with the MOI copy beside it; the constants alone
    for sign in (-1, 1):
        ref = O.AffVec(n).vecaddsub(x, v, subtract=sign < 0)
        terms, _, consts = ref.flat()
        mt, _ = ref.moi(VM)
        mt["out"] += 3
        for shift in SHIFTS:
            c = Case("vars_addsub n=%d sign=%d shift=%d" % (n, sign, shift))
            olt, ovat, oc = c.out(terms, 0, "lt"), c.out(mt, shift, "vat"), c.out(consts, 0, "consts")
            c.call("pmt_vars_addsub_f64", n, c.dev(x), n, c.dev(v), sign, c.dev(VM), 3, olt.ptr(), ovat.ptr(), oc.ptr())
            cases.append(c)
        c = Case("consts n=%d sign=%d" % (n, sign))
        oc = c.out(consts, 0, "consts")
        c.call("pmt_consts_f64", n, c.dev(v), n, sign, oc.ptr())
        cases.append(c)
    return cases


@pytest.mark.parametrize("n", ELEMENTWISE)
def test_one_thread_per_element_kernels(n):
    run_all(elementwise_cases(n))


# ------------------------------------------------------------------ grid-strided kernels: beyond one pass, and their small edges
def vecdot_affs_vars_case(rows, L, moi, shift, oracle=False):
    xt, xc = T.uniform_affvec(rows, L, 31, NV)
    y = T.variables(rows, 32, NV)
    if oracle:
        ref = O.Quad().vecdot_affs_vars(T.oracle_affvec(xt, xc), y)
        at, qt, _ = ref.moi(VM)
        q, lin = (qt, at) if moi else (ref.terms(), ref.affine.terms())
    else:
        q, lin = T.vecdot_affs_vars(xt, xc, y, moi, VM)
    c = Case("vecdot_affs_vars rows=%d L=%d moi=%d shift=%d" % (rows, L, moi, shift))
    oq, ol = c.out(q, shift, "quad"), c.out(lin, 0, "lin")
    c.call("pmt_vecdot_affs_vars_f64", rows * L + rows, rows, c.dev(xt), L, c.dev(xc), c.dev(y), moi, c.dev(VM) if moi else None, oq.ptr(), ol.ptr())
    return c


def affvec_scale_case(rows, nterms, s_dev, s_host, oracle=False):
    s = float(s_dev[0]) if s_dev is not None else s_host
    if oracle:                                                           # uniform rows: nterms = rows * L
        yt, yc = T.uniform_affvec(rows, nterms // max(rows, 1), 33, NV)
        terms, _, consts = O.AffVec(rows).scale_number_affs(s, T.oracle_affvec(yt, yc)).flat()
    else:
        yt, yc = T.uniform_affvec(1, nterms, 33, NV)[0], T.family(rows, 34)
        terms, consts = T.affvec_scale(yt, yc, s)
    c = Case("affvec_scale rows=%d nterms=%d dev=%s" % (rows, nterms, s_dev is not None))
    ot, oc = c.out(terms, 0, "terms"), c.out(consts, 0, "consts")
    c.call("pmt_affvec_scale_f64", nterms + rows, rows, nterms, c.dev(yt), c.dev(yc), c.dev(s_dev), s_host, ot.ptr(), oc.ptr())
    return c


def matvecmul_affs_case(rows, cols, L, pad, oracle=False):
    A = matrix(rows, cols, 35)
    xt, xc = T.uniform_affvec(cols, L, 36, NV)
    if oracle:
        terms, _, consts = O.AffVec(rows).matvecmul_affs(A, T.oracle_affvec(xt, xc)).flat()
    else:
        terms, consts = T.matvecmul_affs(A, xt, xc)
    c = Case("matvecmul_affs %dx%d L=%d lda=rows+%d" % (rows, cols, L, pad))
    ot, oc = c.out(terms, 0, "terms"), c.out(consts, 0, "consts")
    c.call("pmt_matvecmul_affs_f64", rows * cols * L + rows * cols, c.dev(colmajor_padded(A, rows + pad)), rows + pad, rows, cols, c.dev(xt), L, c.dev(xc),
           ot.ptr(), oc.ptr())
    return c


def vecdot_numbers_affs_case(n, L, oracle=False):
    v = T.family(n, 37)
    xt, xc = T.uniform_affvec(n, L, 38, NV)
    if oracle:
        r = O.vecdot_aff_numbers_affs(v, T.oracle_affvec(xt, xc))
        terms, const = r.terms(), r.constant
    else:
        terms, const = T.vecdot_numbers_affs(v, xt, xc)
    c = Case("vecdot_numbers_affs n=%d L=%d" % (n, L))
    ot, oc = c.out(terms, 0, "terms"), c.out(np.array([const]), 0, "const")
    c.call("pmt_vecdot_numbers_affs_f64", n * L + 16 * n, c.dev(v), n, c.dev(xt), L, c.dev(xc), ot.ptr(), oc.ptr(), fusable=n <= 2048)
    return c


def quad_pool(n, seed):
    q = np.empty(n, dtype=g.QT)
    q["coeff"], q["row"], q["col"] = T.family(n, seed), T.variables(n, seed + 1, NV), T.variables(n, seed + 2, NV)
    return q


def quad_combine_case(na, nb, sb, shift, oracle=False):
    qa, qb = quad_pool(na, 41), quad_pool(nb, 44)
    if oracle:
        A, B = quad_of(qa), quad_of(qb)
        want = (O.Quad().copy_from(A).sub_quad(B) if sb < 0 else O.Quad().copy_from(A).add_quad(B)).terms()
    else:
        want = T.quad_combine(qa, qb, sb)
    c = Case("quad_combine na=%d nb=%d sb=%d shift=%d" % (na, nb, sb, shift))
    oq = c.out(want, shift, "quad")
    c.call("pmt_quad_combine_f64", na + nb, c.dev(qa), na, c.dev(qb), nb, sb, oq.ptr())
    return c


def quad_scale_case(n, s_dev, s_host, shift, oracle=False):
    q = quad_pool(n, 47)
    s = float(s_dev[0]) if s_dev is not None else s_host
    want = O.Quad().mul_quad_number(quad_of(q), s).terms() if oracle else T.quad_scale(q, s)
    c = Case("quad_scale n=%d dev=%s shift=%d" % (n, s_dev is not None, shift))
    oq = c.out(want, shift, "quad")
    c.call("pmt_quad_scale_f64", n, c.dev(q), n, c.dev(s_dev), s_host, oq.ptr())
    return c


def scale_numbers_case(n, s_dev, s_host):
    y = T.family(n, 50)
    s = float(s_dev[0]) if s_dev is not None else s_host
    c = Case("scale_numbers n=%d dev=%s" % (n, s_dev is not None))
    o = c.out(s * y, 0, "out")                                           # dest .= x .* y, one product each (src/functions.jl:917-925)
    c.call("pmt_scale_numbers_f64", n, c.dev(y), n, c.dev(s_dev), s_host, o.ptr())
    return c


SDEV = np.array([-1.75])
# one pass of the capped grids: 256 * 8 workgroups of 256 threads (256 * 16 for matvecmul_affs)
PASS = 256 * 8 * 256
assert (PASS - 1, PASS + 1, 2 * PASS + 1) == (1 * 524287, 3 * 174763, 17 * 61681)


def strided_cases(kind):
    if kind == "vecdot_affs_vars":                                       # rows * (L + 1) elements; the quad | lin boundary rows * L inside a pass
        return [vecdot_affs_vars_case(rows, L, moi, shift) for rows, L, moi in ((1, PASS - 2, 1), (3, 174762, 0), (17, 61680, 1)) for shift in SHIFTS]
    if kind == "affvec_scale":                                           # nterms + rows elements; the boundary i == nterms inside a pass
        return [affvec_scale_case(1000, PASS - 1 - 1000, SDEV, 9.0), affvec_scale_case(1000, PASS + 1 - 1000, None, -1.75),
                affvec_scale_case(1000, 2 * PASS + 1 - 1000, SDEV, 9.0)]
    if kind == "matvecmul_affs":                                         # rows * cols * L elements, one pass = 2 * PASS
        assert (41 * 93 * 275, 17 * 1 * 61681, 9 * 43 * 5419) == (2 * PASS - 1, 2 * PASS + 1, 4 * PASS + 1)
        return [matvecmul_affs_case(41, 93, 275, 1), matvecmul_affs_case(17, 1, 61681, 0), matvecmul_affs_case(9, 43, 5419, 1)]
    if kind == "vecdot_numbers_affs":                                    # n * L elements (524287 is prime)
        return [vecdot_numbers_affs_case(PASS - 1, 1), vecdot_numbers_affs_case(174763, 3), vecdot_numbers_affs_case(61681, 17)]
    if kind == "quad_combine":                                           # na + nb elements; the boundary i == na inside a pass
        return [quad_combine_case(na, total - na, -1, shift) for na, total in ((300000, PASS - 1), (300001, PASS + 1), (700000, 2 * PASS + 1))
                for shift in SHIFTS]
    if kind == "quad_scale":
        return [quad_scale_case(n, SDEV, 9.0, shift) for n in (PASS - 1, PASS + 1, 2 * PASS + 1) for shift in SHIFTS]
    assert kind == "scale_numbers"
    return [scale_numbers_case(n, SDEV, 9.0) for n in (PASS - 1, PASS + 1, 2 * PASS + 1)]


STRIDED = ["vecdot_affs_vars", "affvec_scale", "matvecmul_affs", "vecdot_numbers_affs", "quad_combine", "quad_scale", "scale_numbers"]


@pytest.mark.parametrize("kind", STRIDED)
def test_grid_strided_kernels_beyond_one_pass(kind):
    run_all(strided_cases(kind))


def small_edge_cases():
    """L = 0, rows = 1, na = 0, nb = 0, sb = -1, the scalar from the device pointer and from the host argument — against the oracle"""
    cases = []
    for moi in (0, 1):
        for shift in SHIFTS:
            cases += [vecdot_affs_vars_case(5, 0, moi, shift, oracle=True), vecdot_affs_vars_case(1, 7, moi, shift, oracle=True),
                      vecdot_affs_vars_case(9, 13, moi, shift, oracle=True)]
    for s_dev, s_host in ((SDEV, 9.0), (None, -1.75), (None, -0.0)):
        cases += [affvec_scale_case(5, 0, s_dev, s_host, oracle=True), affvec_scale_case(1, 7, s_dev, s_host, oracle=True),
                  affvec_scale_case(6, 30, s_dev, s_host, oracle=True), scale_numbers_case(1, s_dev, s_host), scale_numbers_case(300, s_dev, s_host)]
        cases += [quad_scale_case(n, s_dev, s_host, shift, oracle=True) for n in (1, 300) for shift in SHIFTS]
    cases += [matvecmul_affs_case(4, 6, 0, 1, oracle=True), matvecmul_affs_case(1, 6, 5, 0, oracle=True), matvecmul_affs_case(4, 1, 5, 2, oracle=True)]
    cases += [vecdot_numbers_affs_case(6, 0, oracle=True), vecdot_numbers_affs_case(1, 5, oracle=True)]
    for sb in (1, -1):
        for shift in SHIFTS:
            cases += [quad_combine_case(0, 9, sb, shift, oracle=True), quad_combine_case(9, 0, sb, shift, oracle=True),
                      quad_combine_case(7, 300, sb, shift, oracle=True), quad_combine_case(1, 1, sb, shift, oracle=True)]
    return cases


def test_small_edges_of_the_grid_strided_kernels():
    run_all(small_edge_cases())


# ------------------------------------------------------------------ the left-to-right constant; the 64-thread constants of A * X
SEQ_DOT = [63, 64, 65, 100, 129]                     # (100: a looped tail of 36 behind a full round)
MATVEC = [1, 63, 64, 65, 130]


@pytest.mark.parametrize("n", SEQ_DOT)
def test_numbers_dot_affs_constant_on_both_sides_of_a_round(n):
    vecdot_numbers_affs_case(n, 2, oracle=True).run()


@pytest.mark.parametrize("rows", MATVEC)
def test_matvecmul_affs_rows_around_the_constant_kernel_block(rows):
    matvecmul_affs_case(rows, 3, 2, 1, oracle=True).run()


# ------------------------------------------------------------------ MOI copies
PACK_SQ = [1, 255, 256, 257, 511, 512, 513]


def pack_sq_cases(n):
    q = quad_pool(n, 61)
    zero = np.flatnonzero((q["coeff"] == 0.0) & np.signbit(q["coeff"]))
    q["col"][zero] = q["row"][zero]                                      # a -0.0 coefficient on the diagonal: 2 * -0.0
    assert n < 6 or (len(zero) and np.any(q["row"] == q["col"]) and np.any(q["row"] != q["col"]))
    want = quad_of(q).moi(VM)[1]
    cases = []
    for in_shift in SHIFTS:
        for shift in SHIFTS:
            c = Case("pack_scalar_quadratic n=%d in_shift=%d shift=%d" % (n, in_shift, shift))
            oq = c.out(want, shift, "quad")
            c.call("pmt_pack_scalar_quadratic_f64", n, c.dev(q, in_shift), n, c.dev(VM), oq.ptr())
            cases.append(c)
    return cases


@pytest.mark.parametrize("n", PACK_SQ)
def test_pack_scalar_quadratic(n):
    run_all(pack_sq_cases(n))


def ragged_affvec(lens, seed):
    n = int(sum(lens))
    coeff, var = T.family(n, seed), T.variables(n, seed + 1, NV)
    ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    rows = [lt_of(coeff[ptr[i]:ptr[i + 1]], var[ptr[i]:ptr[i + 1]]) for i in range(len(lens))]
    return rows, T.family(len(lens), seed + 2), ptr


RAGGED = [0, 1, 64, 65, 200, 0, 3]


def pack_va_cases():
    cases = []
    for row_len in (0, 1, 63, 64, 65, 129):
        for rows in (1, 4, 5, 9):
            xt, xc = T.uniform_affvec(rows, row_len, 71, NV)
            want = T.oracle_affvec(xt, xc).moi(VM)[0]
            want["out"] += 11
            for shift in SHIFTS:
                c = Case("pack_vector_affine rows=%d row_len=%d shift=%d" % (rows, row_len, shift))
                ov = c.out(want, shift, "vat")
                c.call("pmt_pack_vector_affine_f64", rows * row_len, c.dev(xt), None, rows, row_len, c.dev(VM), 11, ov.ptr())
                cases.append(c)
    rws, consts, ptr = ragged_affvec(RAGGED, 74)
    want = T.oracle_affvec(rws, consts).moi(VM)[0]
    want["out"] += 11
    assert {int(3 * p) % 2 for p in ptr[:-1]} == {0, 1}                  # segments start on both word parities
    for shift in SHIFTS:
        c = Case("pack_vector_affine ragged shift=%d" % shift)
        ov = c.out(want, shift, "vat")
        c.call("pmt_pack_vector_affine_f64", 0, c.dev(np.concatenate(rws)), c.dev(ptr), len(RAGGED), 0, c.dev(VM), 11, ov.ptr(), fusable=False)
        cases.append(c)
    return cases


def test_pack_vector_affine():
    run_all(pack_va_cases())


# ------------------------------------------------------------------ vecadd! / vecsubtract! / copyto! on affine vectors
def combine_cases():
    cases = []
    lens = (0, 1, 64, 65, 130)
    for rows in (5, 9):
        v = T.family(rows, 80)
        for k, la in enumerate(lens):
            lb = lens[(k + 1) % len(lens)]
            xt, xc = T.uniform_affvec(rows, la, 81, NV)
            yt, yc = T.uniform_affvec(rows, lb, 84, NV)
            X, Y = T.oracle_affvec(xt, xc), T.oracle_affvec(yt, yc)

            def case(name, want, xa, ca, la_, xb, cb, lb_, sb):
                terms, _, consts = want.flat()
                c = Case("affvec_combine %s rows=%d la=%d lb=%d sb=%d" % (name, rows, la_, lb_, sb))
                ot, oc = c.out(terms, 0, "terms"), c.out(consts, 0, "consts")
                lo = (la_ if xa is not None else 0) + (lb_ if xb is not None else 0)
                c.call("pmt_affvec_combine_f64", rows * lo + rows, rows, c.dev(xa), None, la_, c.dev(ca), c.dev(xb), None, lb_, c.dev(cb), sb, ot.ptr(), None, lo,
                       oc.ptr())
                cases.append(c)
            case("a", O.AffVec(rows).vcat(X), xt, xc, la, None, None, 0, 1)                               # copyto! alone
            for sb in (1, -1):
                case("a,b", O.AffVec(rows).vecaddsub(X, Y, subtract=sb < 0), xt, xc, la, yt, yc, lb, sb)
                case("b", O.AffVec(rows).vecaddsub(np.zeros(rows), Y, subtract=sb < 0), None, None, 0, yt, yc, lb, sb)
                case("numbers,b", O.AffVec(rows).vecaddsub(v, Y, subtract=sb < 0), None, v, 0, yt, yc, lb, sb)  # numbers (+|-) affs
        # variables (+|-) numbers: part a is one (1.0, var) term per row WITHOUT constants, part b constants only
        x = T.variables(rows, 87, NV)
        for sb in (1, -1):
            terms, _, consts = O.AffVec(rows).vecaddsub(x, v, subtract=sb < 0).flat()
            c = Case("affvec_combine vars,numbers rows=%d sb=%d" % (rows, sb))
            ot, oc = c.out(terms, 0, "terms"), c.out(consts, 0, "consts")
            c.call("pmt_affvec_combine_f64", 2 * rows, rows, c.dev(lt_of(np.ones(rows), x)), None, 1, None, None, None, 0, c.dev(v), sb, ot.ptr(), None, 1, oc.ptr())
            cases.append(c)
        # ragged rows through row_ptr on every part
        la_r = [lens[i % 5] for i in range(rows)]
        lb_r = [lens[(i + 2) % 5] for i in range(rows)]
        ra, ca, pa = ragged_affvec(la_r, 90)
        rb, cb, pb = ragged_affvec(lb_r, 93)
        X, Y = T.oracle_affvec(ra, ca), T.oracle_affvec(rb, cb)
        for sb in (1, -1):
            terms, po, consts = O.AffVec(rows).vecaddsub(X, Y, subtract=sb < 0).flat()
            c = Case("affvec_combine ragged rows=%d sb=%d" % (rows, sb))
            ot, oc = c.out(terms, 0, "terms"), c.out(consts, 0, "consts")
            c.call("pmt_affvec_combine_f64", 0, rows, c.dev(np.concatenate(ra)), c.dev(pa), 0, c.dev(ca), c.dev(np.concatenate(rb)), c.dev(pb), 0, c.dev(cb), sb,
                   ot.ptr(), c.dev(po), 0, oc.ptr(), fusable=False)
            cases.append(c)
    return cases


def test_affvec_combine():
    run_all(combine_cases())


# ------------------------------------------------------------------ adjoint
TRANSPOSE = [(1, 1), (31, 33), (32, 32), (33, 31), (1, 65), (65, 1), (64, 96), (100, 37)]


def transpose_cases(shape):
    rows, cols = shape
    A = matrix(rows, cols, 95)
    cases = []
    for pad_s in (0, 3):
        for pad_d in (0, 3):
            c = Case("transpose %dx%d lds=rows+%d ldd=cols+%d" % (rows, cols, pad_s, pad_d))
            ldd = cols + pad_d
            want = np.full((rows, ldd), np.nan)                          # dst is cols x rows column-major: column r holds A[r, :], then its padding
            want[:, :cols] = A
            o = c.out(want, 0, "dst")
            c.call("pmt_transpose_f64", rows * cols, c.dev(colmajor_padded(A, rows + pad_s)), rows + pad_s, rows, cols, o.ptr(), ldd)
            cases.append(c)
    return cases


@pytest.mark.parametrize("shape", TRANSPOSE, ids=str)
def test_transpose(shape):
    run_all(transpose_cases(shape))


# ------------------------------------------------------------------ the interpreter: the same cases as nodes of fused runs
def count_cases(n):
    """element counts around the narrow-node switch (256 | 257) and the interpreter's 1024-thread stride"""
    cases = [scale_numbers_case(n, SDEV, 9.0), quad_scale_case(n, None, -1.75, 1), quad_combine_case(n // 3, n - n // 3, -1, 0)]
    cases += pack_sq_cases(n)[1:3] + vecdot_terms_cases(n)[3:5] + bilinear_cases((1, n))[-1:] + bilinear_cases((n, 1))[-2:-1]
    cases += [vecdot_affs_vars_case(1, n - 1, 1, 1), affvec_scale_case(3, n - 3, SDEV, 9.0), vecdot_numbers_affs_case(n // 17, 1)]
    return cases


FAMILIES = {
    "bilinear": lambda: [c for s in BILINEAR if s[0] * s[1] <= NODE_MAX for c in bilinear_cases(s)],
    "quad_expand": lambda: ([c for s in QUAD_EXPAND if s[0] <= 2048 and s[0] * s[1] * s[2] <= NODE_MAX for c in quad_expand_cases(s)]
                            + [c for s in QUAD_EXPAND_SAME for c in quad_expand_cases(s, True)]),
    "elementwise": lambda: [c for n in ELEMENTWISE for c in elementwise_cases(n)],
    "small_edges": small_edge_cases,
    "seq_dot_and_matvec": lambda: [vecdot_numbers_affs_case(n, 2, oracle=True) for n in SEQ_DOT] + [matvecmul_affs_case(r, 3, 2, 1, oracle=True) for r in MATVEC],
    "pack_scalar_quadratic": lambda: [c for n in PACK_SQ for c in pack_sq_cases(n)],
    "pack_vector_affine": pack_va_cases,
    "affvec_combine": combine_cases,
    "transpose": lambda: [c for s in TRANSPOSE for c in transpose_cases(s)],
    "counts": lambda: [c for n in COUNTS for c in count_cases(n)],
}
# what each family must at least bring to the interpreter (the rest of its cases are too large for a node, or ragged)
MUST_FUSE = {"bilinear": ["bilinear 3x5 moi=1 ldq=rows+3", "bilinear 1030x5 moi=1 ldq=rows+3", "bilinear 7x1025"], "transpose": ["transpose 100x37 lds=rows+3 ldd=cols+3"],
             "quad_expand": ["quad_expand (2, 9, 1025)", "quad_expand (200, 2, 3)", "quad_expand (0, 2, 3)", "x.x"]}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_interpreter_replays_the_same_cases_fused(family):
    """the cases of at most 32768 elements per node, recorded on plans and replayed as fused runs (one interpreter launch per plan: asserted
    through pmt_plan_fused), checked against the ORACLE with the same guards — not against the unfused replay"""
    cases = [c for c in FAMILIES[family]() if c.small and c.calls]
    assert len(cases) >= 2
    for needle in MUST_FUSE.get(family, []):
        assert any(needle in c.name for c in cases), needle
    # plans of at most 40 nodes and 60000 elements: inside one run's bounds (48 nodes, 65536 elements: csrc/small.hip, csrc/common.h)
    plans, cur, work = [], [], 0
    for c in cases:
        if cur and (work + c.work > 60000 or len(cur) + 1 > 40):
            plans.append(cur)
            cur, work = [], 0
        cur.append(c)
        work += c.work
    if len(cur) == 1 and plans:                                           # (a run is two nodes at least)
        cur.insert(0, plans[-1].pop())
    plans.append(cur)
    for group in plans:
        assert len(group) >= 2 and all(len(c.calls) == 1 for c in group)
        p = g.Plan()
        with p:
            for c in group:
                c.issue(p.rec)
        assert p.fused() == (1, len(group), 1), (p.fused(), [c.name for c in group])
        p.update()
        for c in group:
            c.check()
        p.close()
