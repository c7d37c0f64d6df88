"""The batched-instance entry points (pmt_batch_lsq_coeffs_f64, pmt_batch_expand_f64) restated in numpy, the data the tests drive them with,
and the table of shapes at which csrc/batch_small.hip takes another path (tests/test_gpu_batch_slabs.py, tests/test_batch_slab_host.py).

Written from the contract in include/parametron_hip.h (slab layout, signs) and from the reference's loops (src/functions.jl:548-576,702-709:
residual . residual; :381-386: canonicalize!; src/moi_interop.jl:45-81: the MOI copies) — not from the kernels.

Device layout of a batch: instance-major, every matrix column-major — so a batch of A is a (B, n, r) C-ordered array `At` with
At[i, col, row], the constraint matrices a (B, n, m) array `Ct`, b is (B, r) and d is (B, m).

DYADIC DATA.  dyadic() draws integers in [-1023, 1023] times 2^e, e in [-4, 4]: every value is a multiple of 2^-4 below 2^14, every product
a multiple of 2^-8 below 2^28, so a sum of up to 1024 doubled products is an integer times 2^-8 below 2^47 — far inside the 53-bit
mantissa.  Q = 2 A'A, q = 2 A'c and c'c are therefore EXACT in every summation order, with or without fma, and a kernel's result can be
compared with numpy's bit for bit without restating the kernel's order.  (A sum that cancels to zero is +0.0 in every order that starts
from +0.0, which all kernels here do; numpy's matmul is normalised with + 0.0.)"""
import numpy as np

# csrc/batch_small.hip's constants, restated (test_batch_slab_host.py checks that the source still holds them verbatim)
STAGE_CAP = 10464       # doubles of LDS staging: the whole slab + 1 alignment shift must fit for C and d to be staged
CREG = 16               # constraint entries a storer thread prefetches into registers
NS = 128                # storer threads
CK = 32                 # rows per chunk
SMALL_MAX_N = 128       # up to here the one persistent-workgroup kernel; beyond, the general tiled path


def slab_doubles(n, m):
    return n * (n + 1) // 2 + n + 1 + m * n + m


def stages_whole_slab(n, m):
    """batch_small.hip assembles [Q | q | const | C | d] in LDS; otherwise only [Q | q | const], and C and d go straight to HBM"""
    return slab_doubles(n, m) + 1 <= STAGE_CAP


def takes_register_prefetch(n, m):
    """the constraint block is loaded into registers in the instance's first phase (else read when it is staged)"""
    return m > 0 and m * n <= CREG * NS and m <= NS


def chunks(r):
    return max(1, -(-r // CK))


# (n, r, m, what it exercises): the small path's shapes
SMALL_CASES = [
    (128, 96, 16, "FAST loads, register prefetch, staged slab"),
    (128, 32, 16, "one chunk per instance: the loader's chunk g + 2 is two instances ahead"),
    (128, 224, 16, "seven chunks"),
    (128, 64, 17, "first m whose slab is not staged at n = 128"),
    (64, 40, 127, "last m that stages the whole slab at n = 64"),
    (64, 40, 128, "first m that does not stage at n = 64"),
    (16, 33, 128, "m n = 2048 and m = 128: last prefetch case"),
    (8, 20, 200, "m n <= 2048 but m > 128: no prefetch"),
    (127, 31, 17, "ragged rows and columns, m n > 2048"),
    (100, 33, 5, "ragged rows and columns"),
    (65, 70, 2, "three chunks with a ragged last one"),
    (2, 7, 1, "tiny instance"),
    (1, 1, 0, "L = 3, the smallest slab"),
    (128, 33, 0, "no constraint block"),
    (128, 0, 3, "no rows: Q, q and const are +0.0"),
]
# (n, r, m, out_stride = L + 3, A shifted by 8 bytes): the general path's shapes (r = 33: an odd pitch, so no 16-byte loads)
GENERAL_CASES = [
    (129, 50, 33, False, False),
    (200, 64, 4, True, False),
    (256, 16, 0, False, False),
    (257, 17, 40, True, False),
    (130, 0, 2, False, False),
    (200, 33, 3, True, False),
    (200, 33, 3, False, True),
]
SIGN_SHAPES = [(100, 33, 5), (129, 50, 33)]
POSITION_SHAPES = [(128, 96, 16), (127, 31, 17)]
ISOLATION_SHAPES = [(128, 96, 16), (100, 70, 5)]


def gpu_shapes():
    """every (n, r) the GPU file computes on dyadic data"""
    s = {(n, r) for n, r, _, _ in SMALL_CASES} | {(n, r) for n, r, _, _, _ in GENERAL_CASES} | {(n, r) for n, r, _ in SIGN_SHAPES + ISOLATION_SHAPES}
    return sorted(s | {(128, 64), (0, 5)})


def dyadic(shape, rng):
    """doubles m * 2^e, m an integer in [-1023, 1023], e in [-4, 4]; about 5 % exact zeros, two fifths of them -0.0"""
    m = rng.integers(-1023, 1024, size=shape)
    e = rng.integers(-4, 5, size=shape)
    v = np.ldexp(m.astype(np.float64), e)
    u = rng.random(shape)
    v = np.where(u < 0.05, 0.0, v)
    v = np.where(u < 0.02, -0.0, v)
    return np.ascontiguousarray(v)


def batch_data(B, n, r, m, rng, gen=dyadic):
    """(At (B, n, r), b (B, r), Ct (B, n, m), d (B, m)) in the device layout"""
    return gen((B, n, r), rng), gen((B, r), rng), gen((B, n, m), rng), gen((B, m), rng)


def signed(v, sign):
    """0.0 (+|-) v, the constant a zeroed AffineFunction holds after add! / subtract! of a Number; sign 0: +0.0"""
    v = np.asarray(v, dtype=np.float64)
    return 0.0 + v if sign > 0 else (0.0 - v if sign < 0 else np.zeros_like(v))


def slab_reference_batch(At, b, Ct, d, sign_b, sign_d):
    """(B, L) slabs [Q | q | const | C row-major | d-consts] of a batch in the device layout; Q and q through numpy's matmul (exact on dyadic
    data, whatever its order), the constant as the reference's left-to-right sum"""
    B, n, r = At.shape
    m = Ct.shape[2]
    c = signed(b, sign_b)
    iu = np.triu_indices(n)
    Q = 2.0 * np.matmul(At, At.transpose(0, 2, 1)) + 0.0
    q = 2.0 * np.matmul(At, c[:, :, None])[:, :, 0] + 0.0
    const = np.zeros(B)
    for i in range(r):
        const = const + c[:, i] * c[:, i]
    out = np.empty((B, slab_doubles(n, m)))
    nq = len(iu[0])
    out[:, :nq] = Q[:, iu[0], iu[1]]
    out[:, nq:nq + n] = q
    out[:, nq + n] = const
    out[:, nq + n + 1:nq + n + 1 + m * n] = Ct.transpose(0, 2, 1).reshape(B, m * n)
    out[:, nq + n + 1 + m * n:] = signed(d, sign_d)
    return out


def slab_reference(A, b, C, d, sign_b, sign_d):
    """one instance: A (r, n), b (r,), C (m, n), d (m,) as mathematical matrices -> its slab of slab_doubles(n, m) doubles"""
    A, C = np.asarray(A, dtype=np.float64), np.asarray(C, dtype=np.float64)
    return slab_reference_batch(np.ascontiguousarray(A.T)[None], np.asarray(b, dtype=np.float64)[None], np.ascontiguousarray(C.T)[None],
                                np.asarray(d, dtype=np.float64)[None], sign_b, sign_d)[0]


def sections(n, m):
    """name -> slice of a slab"""
    nq = n * (n + 1) // 2
    return {"Q": slice(0, nq), "q": slice(nq, nq + n), "const": slice(nq + n, nq + n + 1), "C": slice(nq + n + 1, nq + n + 1 + m * n),
            "d": slice(nq + n + 1 + m * n, nq + n + 1 + m * n + m)}


# ---- exact integer arithmetic on doubles: every finite double is an integer times a power of two

def as_scaled_ints(a):
    """(object array of Python ints I, k) with a == I * 2^k exactly, one k for the whole array"""
    a = np.asarray(a, dtype=np.float64)
    mant, ex = np.frexp(a)                                              # a = mant * 2^ex, |mant| in [0.5, 1) or 0
    M = np.ldexp(mant, 53).astype(np.int64)                             # exact: 53 bits
    e = ex.astype(np.int64) - 53
    live = M != 0
    k = int(e[live].min()) if live.any() else 0
    sh = np.where(live, e - k, 0)
    I = np.array([int(x) << int(s) for x, s in zip(M.reshape(-1).tolist(), sh.reshape(-1).tolist())], dtype=object).reshape(a.shape)
    return I, k


def exact_gram(At, c):
    """one instance, exact: (S, Sabs, s, sabs, 2 k) with A'A = S * 2^(2k), sum |a||a| = Sabs * 2^(2k), A'c = s * 2^(2k), sum |c||a| = sabs *
    2^(2k); At is (n, r), c is (r,); Python integers throughout"""
    I, k = as_scaled_ints(np.concatenate([At.reshape(-1), c.reshape(-1)]))
    n, r = At.shape
    Ai, ci = I[:n * r].reshape(n, r), I[n * r:]
    Aa, ca = np.abs(Ai), np.abs(ci)
    return Ai.dot(Ai.T), Aa.dot(Aa.T), Ai.dot(ci), Aa.dot(ca), 2 * k


def within_inner_product_bound(got, S, Sabs, k2, r):
    """|got - 2 S 2^k2| <= (r + 2) 2^-53 * 2 Sabs 2^k2, in integers — the standard bound of an r-term inner product summed in any order, with or
    without fma (the doubling is exact).  got, S, Sabs: arrays of equal shape."""
    ok = np.empty(np.shape(got), dtype=bool)
    for idx in np.ndindex(*np.shape(got)):
        g = float(got[idx])
        if not np.isfinite(g):
            ok[idx] = False
            continue
        num, den = g.as_integer_ratio()                                   # exact
        # |num / den - 2 S 2^k2| * 2^53 <= (r + 2) * 2 Sabs 2^k2, both sides times den * 2^-k2 (k2 < 0 here; kept general)
        s2, b2 = 2 * int(S[idx]), 2 * int(Sabs[idx])
        if k2 >= 0:
            err, bound = abs(num - s2 * den * (1 << k2)), (r + 2) * b2 * den * (1 << k2)
        else:
            err, bound = abs(num * (1 << -k2) - s2 * den), (r + 2) * b2 * den
        ok[idx] = (err << 53) <= bound
    return ok
