"""The batched tracking-cost entry point (pmt_batch_form_coeffs_f64) restated in numpy, and the data its tests drive it with
(tests/test_batch_form_host.py, tests/test_gpu_batch_form.py).

Written from the contract in include/parametron_hip.h — the slab layout and signs of the least-squares batch (batch_util), the Q section of
pmt_quad_form_f64 and the order fixed for pmt_quad_form_shift_f64's linear part and constant (quad_form_shift_util) — not from the kernel.

Device layout of a batch: instance-major, every matrix column-major — a batch of Q is a (B, n, n) C-ordered array `Qt` with Qt[i, col, row],
the constraint matrices a (B, n, m) array `Ct`, p is (B, n) and d is (B, m).

COARSE DYADIC DATA.  batch_util.dyadic draws integers in [-1023, 1023] times 2^e, e in [-4, 4]: |v| <= 16368.  coarse() truncates such a
value towards zero to a multiple of 8 (the sign of a zero is kept), so v = 8 a with an integer |a| <= 2046 < 2^11.  Then, in units of 8,
64, 64 and 512:
    S[j,k] = Q[j,k] + Q[k,j]            an integer below 2^12
    S[j,k] * c_k                        an integer below 2^23
    any partial sum of lin_j            (at most n <= 256 products) an integer below 2^31
    c_j * lin_j                         an integer below 2^42
    any partial sum of T                (at most 256 products) an integer below 2^50
— every intermediate value of the restatement is an integer below 2^53 in its unit, so every product and every sum is EXACT in every order,
with or without fma, and Q, q and const can be compared bit for bit with a computation in Python integers.  (A sum that cancels to zero is
+0.0 where a chain starts from +0.0; a chain of lin_j starts from its first product, so a lone zero keeps that product's sign — the integer
computation knows no signed zero, and the comparison adds + 0.0 on both sides.)"""
import numpy as np

import batch_util as BU
import quad_form_shift_util as SU

MAX_N = 256             # PMT_BATCH_FORM_MAX_N (test_batch_form_host.py checks the header and the source)


def form_slab_reference(Qt, p, Ct, d, sign_p, sign_d):
    """(B, L) slabs [Q | q | const | C row-major | d-consts] of a batch in the device layout.  Q section: S = Q + Q' on the row-major upper
    triangle, 2*Q[j,j] on the diagonal; q, const: the header's order for the shifted form with c = 0.0 (+|-) p (sign_p == 0: +0.0, p is not
    read); C and the d-consts as the least-squares batch"""
    Qt, Ct, d = (np.asarray(a, dtype=np.float64) for a in (Qt, Ct, d))
    B, n, _ = Qt.shape
    m = Ct.shape[2]
    sec = BU.sections(n, m)
    iu = np.triu_indices(n)
    out = np.empty((B, BU.slab_doubles(n, m)))
    for i in range(B):
        Q = Qt[i].T
        out[i, sec["Q"]] = SU.symmetrised(Q)[iu]
        if sign_p and n:
            out[i, sec["q"]], out[i, sec["const"]] = SU.restate_shift(Q, p[i], sign_p)
        else:
            out[i, sec["q"]], out[i, sec["const"]] = 0.0, 0.0
    out[:, sec["C"]] = Ct.transpose(0, 2, 1).reshape(B, m * n)
    out[:, sec["d"]] = BU.signed(d, sign_d)
    return out


def coarse(v):
    """a dyadic value truncated towards zero to a multiple of 8; -0.0 stays -0.0, a negative value below 8 becomes -0.0"""
    return np.ascontiguousarray(8.0 * np.trunc(np.asarray(v, dtype=np.float64) / 8.0))


def coarse_dyadic(shape, rng):
    return coarse(BU.dyadic(shape, rng))


def mixed(shape, rng):
    """full-mantissa data of mixed magnitudes; about a tenth exact zeros of both signs"""
    v = rng.standard_normal(shape) * rng.choice([1.0, -3.0, 1e-3, 40.0], size=shape)
    u = rng.random(shape)
    v = np.where(u < 0.10, 0.0, v)
    v = np.where(u < 0.05, -0.0, v)
    return np.ascontiguousarray(v)


def form_data(B, n, m, rng, gen=mixed):
    """(Qt (B, n, n), p (B, n), Ct (B, n, m), d (B, m)) in the device layout; with gen = mixed, three in ten pairs Q[j,k] = -Q[k,j]: sums that
    cancel to +0.0"""
    Qt, p, Ct, d = gen((B, n, n), rng), gen((B, n), rng), gen((B, n, m), rng), gen((B, m), rng)
    if gen is mixed and n > 1:
        lo = np.tril_indices(n, -1)
        opp = rng.random((B, len(lo[0]))) < 0.3
        for i in range(B):
            Qt[i][lo[0][opp[i]], lo[1][opp[i]]] = -Qt[i][lo[1][opp[i]], lo[0][opp[i]]]
    return Qt, p, Ct, d


def exact_form(Q, p, sign_p):
    """one instance in Python integers: (S on the upper triangle, lin, T, sum |S c| per row, sum |c lin|, k) with Q = Qi * 2^k, p = pi * 2^k:
    S * 2^k, lin * 2^(2k), T * 2^(3k) are the exact values of Q + Q', (Q + Q')c and c'(Q + Q')c"""
    n = len(p)
    I, k = BU.as_scaled_ints(np.concatenate([np.asarray(Q).reshape(-1), np.asarray(p).reshape(-1)]))
    Qi, ci = I[:n * n].reshape(n, n), I[n * n:] * (1 if sign_p > 0 else -1)
    S = Qi + Qi.T                                                       # (the diagonal: 2 * Q[j,j])
    lin = S.dot(ci) if n else np.zeros(0, dtype=object)
    T = sum(int(c) * int(l) for c, l in zip(ci.tolist(), lin.tolist()))
    mag_lin = np.abs(S).dot(np.abs(ci)) if n else np.zeros(0, dtype=object)
    mag_T = sum(abs(int(c)) * int(l) for c, l in zip(ci.tolist(), mag_lin.tolist()))
    return S[np.triu_indices(n)], lin, T, mag_lin, mag_T, k
