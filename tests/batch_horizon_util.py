"""The batched MPC horizons (pmt_batch_horizon_coeffs_f64, pmt_batch_horizon_expand_f64) restated in numpy, and the data their tests drive
them with (tests/test_batch_horizon_host.py, tests/test_gpu_batch_horizon.py).

Written from the contract in include/parametron_hip.h, not from the kernel: the slab
    [ SQ: nx(nx+1)/2 | SR: nu(nu+1)/2 | q: n | const: 1 | C: m*n row-major | d-consts: m ],   n = T*(nx + nu), z = [x_0; u_0; x_1; u_1; ..]
with SQ / SR the Q section of pmt_quad_form_f64 (quad_form_shift_util.symmetrised), every stage's words of q and its constant those of
pmt_quad_form_shift_f64 (quad_form_shift_util.restate_shift: 64-column chains, the first product starting the chain, the blocks in order;
256 chains onto 0.0 and the halving tree; a plain stage: +0.0), the constant the stage constants in z order added in S_d's order
(quad_form_shift_util.chain_tree_sum), C and the d-consts as the least-squares batch (batch_util).

Device layout of a batch: instance-major, every matrix column-major — Qt (B, nx, nx) and Rt (B, nu, nu) C-ordered with Qt[i, col, row],
r (B, T, nx) and v (B, T, nu) stage-major, the constraint matrices Ct (B, n, m), d (B, m).

COARSE DYADIC DATA (batch_form_util.coarse_dyadic): multiples of 8 below 2^14.  In units of 8, 64, 64 and 512 every S is an integer below
2^12, every product S*c below 2^23, every partial sum of a lin_j (at most 128 products here) below 2^30, every product c_j*lin_j below 2^41
and every partial sum of a stage's T_s (at most 128 products) below 2^48; the halved T_s is an integer below 2^48 in units of 256, and a sum
of up to 16 stage constants (T <= 8) stays below 2^52: every intermediate value is an integer below 2^53 in its unit, so every product and
sum is EXACT in every order, with or without fma, and the slab can be compared bit for bit with Python integers and with the oracle.  (Zeros
are compared after + 0.0: a chain of lin_j starts from its first product and may keep a -0.0; integers know no signed zero.)"""
from fractions import Fraction

import numpy as np

import batch_form_util as F
import batch_util as BU
import quad_form_shift_util as SU
import quad_stages_util as QU

MAX_DIM = 128           # PMT_BATCH_HORIZON_MAX_DIM (test_batch_horizon_host.py checks the header and the source)
MAX_T = 512             # PMT_BATCH_HORIZON_MAX_T


def slab_doubles(T, nx, nu, m):
    n = T * (nx + nu)
    return nx * (nx + 1) // 2 + nu * (nu + 1) // 2 + n + 1 + m * n + m


def sections(T, nx, nu, m):
    """name -> slice of a slab"""
    n = T * (nx + nu)
    nqx, nqu = nx * (nx + 1) // 2, nu * (nu + 1) // 2
    q = nqx + nqu
    return {"SQ": slice(0, nqx), "SR": slice(nqx, q), "q": slice(q, q + n), "const": slice(q + n, q + n + 1),
            "C": slice(q + n + 1, q + n + 1 + m * n), "d": slice(q + n + 1 + m * n, q + n + 1 + m * n + m)}


def stage_words(M, ref, sign):
    """(lin, constant) of one stage transpose(y (+|-) ref) * M * (y (+|-) ref) in the single node's order; sign == 0: the plain stage, +0.0
    (ref is not read)"""
    if not sign:
        return np.zeros(len(M)), 0.0
    lin, const = SU.restate_shift(M, ref, sign)
    return lin, float(const)


def instance_slab(Q, R, r, v, Cm, d, sign_r, sign_v, sign_d):
    """one instance: Q (nx, nx), R (nu, nu), Cm (m, n) as mathematical matrices, r (T, nx), v (T, nu) (None with sign 0), d (m,) -> its slab"""
    Q, R = np.asarray(Q, dtype=np.float64), np.asarray(R, dtype=np.float64)
    nx, nu, T, m = len(Q), len(R), (len(r) if r is not None else len(v)), len(d)
    w = nx + nu
    sec = sections(T, nx, nu, m)
    out = np.empty(slab_doubles(T, nx, nu, m))
    out[sec["SQ"]] = SU.symmetrised(Q)[np.triu_indices(nx)]
    out[sec["SR"]] = SU.symmetrised(R)[np.triu_indices(nu)] if nu else []
    q, consts = np.empty((T, w)), []
    for t in range(T):
        q[t, :nx], c = stage_words(Q, r[t] if sign_r else None, sign_r)
        consts.append(c)
        if nu:
            q[t, nx:], c = stage_words(R, v[t] if sign_v else None, sign_v)
            consts.append(c)
    out[sec["q"]] = q.reshape(-1)
    out[sec["const"]] = SU.chain_tree_sum(np.array(consts, dtype=np.float64))          # the table [x_0, u_0, x_1, ..] ([x_0, x_1, ..] with nu == 0)
    out[sec["C"]] = np.asarray(Cm, dtype=np.float64).reshape(-1)                        # row-major
    out[sec["d"]] = BU.signed(d, sign_d)
    return out


def horizon_slab_reference(Qt, Rt, r, v, Ct, d, sign_r, sign_v, sign_d, T=None):
    """(B, L) slabs of a batch in the device layout; r / v may be None where the sign is 0 (then T must be given)"""
    B = len(Qt)
    if T is None:
        T = (r if r is not None else v).shape[1]
    return np.stack([instance_slab(Qt[i].T, Rt[i].T, r[i] if sign_r else [None] * T, v[i] if sign_v else [None] * T, Ct[i].T, d[i], sign_r, sign_v,
                                   sign_d) for i in range(B)])


def instance_stages(Q, R, r, v, sign_r, sign_v, xvar):
    """the instance's table for pmt_quad_stages_f64 as quad_stages_util takes it: the stages [x_0, u_0, x_1, u_1, ..] over the n variables
    `xvar` of z, created stage by stage (quad_at / lin_at cumulative in z order) -> (stages, nterms, nlin)"""
    nx, nu, T = len(Q), len(R), len(xvar) // (len(Q) + len(R))
    xvar = np.asarray(xvar, dtype=np.int64)
    stages, qa, la = [], 0, 0
    for t in range(T):
        for M, ref, sign, nd in ((Q, r, sign_r, nx), (R, v, sign_v, nu)):
            if nd:
                stages.append({"Q": np.asarray(M, dtype=np.float64), "xvar": xvar[la:la + nd], "v": np.asarray(ref[t], dtype=np.float64) if sign else None,
                               "sign": sign, "quad_at": qa, "lin_at": la})
                qa, la = qa + nd * (nd + 1) // 2, la + nd
    return stages, qa, la


def expanded_reference(Q, R, r, v, Cm, d, sign_r, sign_v, sign_d, xvar, varmap):
    """what pmt_batch_horizon_expand_f64 leaves for the instance: (quadratic term words, linear term words, constant, vector-affine term words,
    their constants) — the first three what pmt_quad_stages_f64 writes for the instance's table (quad_stages_util's restatement), the
    constraint block that of pmt_batch_expand_f64: term e = row*n + col is (row + 1, C[row, col], vm[xvar[col]])"""
    from parametron_jl_amd import _lib
    stages, nterms, nlin = instance_stages(Q, R, r, v, sign_r, sign_v, xvar)
    quad, lin, _, const = QU.images(stages, varmap, nterms, nlin)
    Cm = np.asarray(Cm, dtype=np.float64)
    m, n = Cm.shape
    vat = np.empty(m * n, dtype=_lib.VAT)
    vat["out"] = np.repeat(np.arange(1, m + 1, dtype=np.int64), n)
    vat["coeff"] = Cm.reshape(-1)
    vat["var"] = np.tile(np.asarray(varmap, dtype=np.int64)[np.asarray(xvar, dtype=np.int64) - 1], m)
    return quad, lin, const, vat.view(np.int64), BU.signed(d, sign_d)


# ---- data

def horizon_data(B, T, nx, nu, m, rng, gen=F.mixed):
    """(Qt (B, nx, nx), Rt (B, nu, nu), r (B, T, nx), v (B, T, nu), Ct (B, n, m), d (B, m)) in the device layout; with gen = mixed, three in
    ten pairs M[j,k] = -M[k,j]: sums that cancel to +0.0"""
    n = T * (nx + nu)
    Qt, Rt, r, v = gen((B, nx, nx), rng), gen((B, nu, nu), rng), gen((B, T, nx), rng), gen((B, T, nu), rng)
    Ct, d = gen((B, n, m), rng), gen((B, m), rng)
    if gen is F.mixed:
        for Mt in (Qt, Rt):
            nd = Mt.shape[1]
            if nd > 1:
                lo = np.tril_indices(nd, -1)
                opp = rng.random((B, len(lo[0]))) < 0.3
                for i in range(B):
                    Mt[i][lo[0][opp[i]], lo[1][opp[i]]] = -Mt[i][lo[1][opp[i]], lo[0][opp[i]]]
    return Qt, Rt, r, v, Ct, d


def exact_instance(Q, R, r, v, sign_r, sign_v):
    """one instance in Python integers / fractions: (SQ, SR, q, const) as exact rationals — S on the upper triangles, q in z order, the
    constant sum_t c'Qc + c'Rc — and the largest sum of magnitudes met on the way, in the units of the module docstring: (lin, T_s, total)"""
    T, nx, nu = len(r), len(Q), len(R)
    q, total, mags = [], Fraction(0), [0, 0, Fraction(0)]
    secs = []
    for M, nd in ((Q, nx), (R, nu)):
        if nd:
            S, _, _, _, _, k = F.exact_form(M, np.zeros(nd), 1)
            secs.append([Fraction(int(s)) * Fraction(2) ** k for s in S.tolist()])
        else:
            secs.append([])
    for t in range(T):
        for M, ref, sign, nd in ((Q, r, sign_r, nx), (R, v, sign_v, nu)):
            if not nd:
                continue
            if not sign:
                q += [Fraction(0)] * nd
                continue
            _, lin, Ts, mag_lin, mag_T, k = F.exact_form(M, ref[t], sign)
            q += [Fraction(int(l)) * Fraction(2) ** (2 * k) for l in lin.tolist()]
            c = Fraction(int(Ts)) * Fraction(2) ** (3 * k) / 2
            total += c
            mags[0] = max([mags[0]] + [Fraction(int(a)) * Fraction(2) ** (2 * k) / 64 for a in mag_lin.tolist()])
            mags[1] = max(mags[1], Fraction(int(mag_T)) * Fraction(2) ** (3 * k) / 512)
            mags[2] += Fraction(int(mag_T)) * Fraction(2) ** (3 * k) / 512                # (in units of 256: twice this; the halved constants)
    return secs[0], secs[1], q, total, mags
