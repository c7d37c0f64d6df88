"""The batched horizons with time-varying stage weights (pmt_batch_horizon_tv_coeffs_f64, pmt_batch_horizon_tv_expand_f64) restated in numpy,
and the data their tests drive them with (tests/test_batch_horizon_tv_host.py, tests/test_gpu_batch_horizon_tv.py).

Written from the contract in include/parametron_hip.h, not from the kernel: over z = [x_0; u_0; ..; u_{T-1}; (x_T)] (x_T with term == 1),
n = T*(nx + nu) + term*nx variables and ns = T*(1 + (nu > 0)) + term stages in z order, the slab
    [ S: ns blocks in z order, nd(nd+1)/2 words each | q: n | sconst: ns | const: 1 | C: m*n row-major | d-consts: m ]
with block s the sibling's section of the stage's own matrix (quad_form_shift_util.symmetrised), the stage's q words and sconst[s] those of
pmt_quad_form_shift_f64 (batch_horizon_util.stage_words: 64-column chains, the first product starting the chain, the blocks in order; 256
chains onto 0.0 and the halving tree; a plain stage: +0.0), const the sconst words added in S_d's order (quad_form_shift_util.chain_tree_sum),
C and the d-consts as the least-squares batch (batch_util.signed).

Device layout of a batch: instance-major, then stage-major, every matrix column-major — Qt (B, T + term, nx, nx) and Rt (B, T, nu, nu)
C-ordered with Qt[i, t, col, row], r (B, T + term, nx), v (B, T, nu), the constraint matrices Ct (B, n, m), d (B, m)."""
import numpy as np

import batch_horizon_util as H
import batch_util as BU
import quad_form_shift_util as SU
import quad_stages_util as QU


def dims(T, nx, nu, term):
    """(n, ns)"""
    return T * (nx + nu) + term * nx, T * (2 if nu else 1) + term


def slab_doubles(T, nx, nu, term, m):
    n, ns = dims(T, nx, nu, term)
    return T * (nx * (nx + 1) // 2 + nu * (nu + 1) // 2) + term * (nx * (nx + 1) // 2) + n + ns + 1 + m * n + m


def stage_kinds(T, nu, term):
    """the stages in z order: [(kind, t)], kind "x" | "u\""""
    out = []
    for t in range(T + term):
        out.append(("x", t))
        if nu and t < T:
            out.append(("u", t))
    return out


def sections(T, nx, nu, term, m):
    """name -> slice of a slab; "S" the list of the ns blocks' slices in z order, "qs" the list of the stages' slices of q"""
    n, ns = dims(T, nx, nu, term)
    S, qs, at, qa = [], [], 0, 0
    for kind, _ in stage_kinds(T, nu, term):
        nd = nx if kind == "x" else nu
        S.append(slice(at, at + nd * (nd + 1) // 2))
        at += nd * (nd + 1) // 2
    q = at
    for kind, _ in stage_kinds(T, nu, term):
        nd = nx if kind == "x" else nu
        qs.append(slice(q + qa, q + qa + nd))
        qa += nd
    assert qa == n and len(S) == ns
    return {"S": S, "qs": qs, "q": slice(q, q + n), "sconst": slice(q + n, q + n + ns), "const": slice(q + n + ns, q + n + ns + 1),
            "C": slice(q + n + ns + 1, q + n + ns + 1 + m * n), "d": slice(q + n + ns + 1 + m * n, q + n + ns + 1 + m * n + m)}


def stage_list(Q, R, r, v, sign_r, sign_v):
    """one instance's stages in z order from its matrices Q (T + term, nx, nx), R (T, nu, nu) (mathematical: M[t][row, col]) and references
    r (T + term, nx), v (T, nu) (None with sign 0): [(M, ref or None, sign)]"""
    T, nu = len(R), (R.shape[1] if len(R) else 0)
    out = []
    for kind, t in stage_kinds(T, nu, len(Q) - T):
        if kind == "x":
            out.append((np.asarray(Q[t], dtype=np.float64), r[t] if sign_r else None, sign_r))
        else:
            out.append((np.asarray(R[t], dtype=np.float64), v[t] if sign_v else None, sign_v))
    return out


def instance_slab(Q, R, r, v, Cm, d, sign_r, sign_v, sign_d):
    """one instance: Q (T + term, nx, nx), R (T, nu, nu), Cm (m, n) as mathematical matrices -> its slab"""
    T, nx, nu, m = len(R), Q.shape[1], R.shape[1], len(d)
    term = len(Q) - T
    sec = sections(T, nx, nu, term, m)
    out = np.empty(slab_doubles(T, nx, nu, term, m))
    consts = []
    for s, (M, ref, sign) in enumerate(stage_list(Q, R, r, v, sign_r, sign_v)):
        out[sec["S"][s]] = SU.symmetrised(M)[np.triu_indices(len(M))]
        out[sec["qs"][s]], c = H.stage_words(M, ref, sign)
        consts.append(c)
    out[sec["sconst"]] = consts
    out[sec["const"]] = SU.chain_tree_sum(np.array(consts, dtype=np.float64))
    out[sec["C"]] = np.asarray(Cm, dtype=np.float64).reshape(-1)                        # row-major
    out[sec["d"]] = BU.signed(d, sign_d)
    return out


def matrices(Mt_i):
    """one instance's memory images [stages, col, row] as matrices [stages, row, col]"""
    return np.ascontiguousarray(np.asarray(Mt_i).transpose(0, 2, 1))


def slab_reference(Qt, Rt, r, v, Ct, d, sign_r, sign_v, sign_d):
    """(B, L) slabs of a batch in the device layout; Rt is (B, T, nu, nu) also with nu == 0 (it carries T)"""
    return np.stack([instance_slab(matrices(Qt[i]), matrices(Rt[i]), r[i] if sign_r else None, v[i] if sign_v else None, Ct[i].T, d[i],
                                   sign_r, sign_v, sign_d) for i in range(len(Qt))])


def instance_stages(Q, R, r, v, sign_r, sign_v, xvar):
    """the instance's table for pmt_quad_stages_f64 as quad_stages_util takes it — a Q of its own per stage —, the stages laid out one
    behind the other over the n variables `xvar` of z (quad_at / lin_at cumulative in z order) -> (stages, nterms, nlin)"""
    xvar = np.asarray(xvar, dtype=np.int64)
    stages, qa, la = [], 0, 0
    for M, ref, sign in stage_list(Q, R, r, v, sign_r, sign_v):
        nd = len(M)
        stages.append({"Q": M, "xvar": xvar[la:la + nd], "v": np.asarray(ref, dtype=np.float64) if sign else None, "sign": sign,
                       "quad_at": qa, "lin_at": la})
        qa, la = qa + nd * (nd + 1) // 2, la + nd
    return stages, qa, la


def expanded_reference(Q, R, r, v, Cm, d, sign_r, sign_v, sign_d, xvar, varmap):
    """what pmt_batch_horizon_tv_expand_f64 leaves for the instance: (quadratic term words, linear term words, constant, vector-affine term
    words, their constants) — the first three what pmt_quad_stages_f64 writes for the instance's table (quad_stages_util's restatement), the
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

def tv_data(B, T, nx, nu, term, m, rng, gen=None):
    """(Qt (B, T + term, nx, nx), Rt (B, T, nu, nu), r (B, T + term, nx), v (B, T, nu), Ct (B, n, m), d (B, m)) in the device layout: standard
    normal numbers by default, `gen(shape, rng)` otherwise (batch_form_util.mixed, coarse_dyadic)"""
    gen = gen or (lambda shape, g: g.standard_normal(shape))
    n, _ = dims(T, nx, nu, term)
    return (gen((B, T + term, nx, nx), rng), gen((B, T, nu, nu), rng), gen((B, T + term, nx), rng), gen((B, T, nu), rng), gen((B, n, m), rng),
            gen((B, m), rng))


def encoded_data(B, T, nx, nu, term):
    """(Qt, Rt, r, v) whose values name their place: |Q_{i,t}[row, col]| = (((i*1024 + s)*128 + row)*128 + col) + 0.5 with s the stage's index
    in z order, |r_{i,t}[row]| = ((i*1024 + s)*128 + row) + 0.25 — exact doubles, all different, negative where the indices' sum is odd: the
    block of another stage or instance, a transposed index or a lost sign differs"""
    step = 2 if nu else 1

    def mats(cnt, nd, first):
        i = np.arange(B, dtype=np.int64)[:, None, None, None]
        s = first + step * np.arange(cnt, dtype=np.int64)[None, :, None, None]
        col = np.arange(nd, dtype=np.int64)[None, None, :, None]
        row = np.arange(nd, dtype=np.int64)[None, None, None, :]
        code = (((i * 1024 + s) * 128 + row) * 128 + col).astype(np.float64) + 0.5
        return np.where((i + s + row + col) % 2 == 1, -code, code)

    def vecs(cnt, nd, first):
        i = np.arange(B, dtype=np.int64)[:, None, None]
        s = first + step * np.arange(cnt, dtype=np.int64)[None, :, None]
        row = np.arange(nd, dtype=np.int64)[None, None, :]
        code = ((i * 1024 + s) * 128 + row).astype(np.float64) + 0.25
        return np.where((i + s + row) % 2 == 1, -code, code)

    return mats(T + term, nx, 0), mats(T, nu, 1), vecs(T + term, nx, 0), vecs(T, nu, 1)
