"""The batched horizons with a terminal cost, stage weights and linear stage terms (pmt_batch_horizon_terms_coeffs_f64,
pmt_batch_horizon_terms_expand_f64) restated in numpy, and the data their tests drive them with (tests/test_batch_horizon_terms_host.py,
tests/test_gpu_batch_horizon_terms.py).

Written from the contract in include/parametron_hip.h, not from the kernel: over z = [x_0; u_0; ..; x_{T-1}; u_{T-1}; x_T] (x_T only with a
P; term in {0, 1}), n = T*(nx + nu) + term*nx variables and ns = T*(1 + (nu > 0)) + term stages in z order, the slab
    [ SQ | SR | SP: term*nx(nx+1)/2 | W: ns | q: n | const: 1 | C: m*n row-major | d-consts: m ]
with SQ / SR / SP the unweighted sections of the sibling (quad_form_shift_util.symmetrised), W[s] the stage's weight as read (1.0 without a
weight array), q of stage s the words W_s * lin_j, then + g_s[j] with a linear vector — lin_j the sibling's (batch_horizon_util.stage_words;
a plain stage: +0.0, so a negative weight leaves -0.0) —, every stage constant W_s * (0.5 * T_s), the ns of them added in S_d's order
(quad_form_shift_util.chain_tree_sum), C and the d-consts as the sibling.  The expansion: coeff = W_s * S[j,k] per quadratic term, the
linear terms and the constant copied, the index words through the varmap.

A batch is a dict in the device layout, instance-major, every matrix column-major: Qt (B, nx, nx), Rt (B, nu, nu), Pt (B, nx, nx) C-ordered
with Mt[i, col, row]; r (B, T, nx), v (B, T, nu), rN (B, nx); wx (B, T), wu (B, T), wN (B,); gx (B, T, nx), gu (B, T, nu), gN (B, nx);
Ct (B, n, m), d (B, m).  Pt None: no terminal stage; a weight / linear array None: absent.  `signs` = (sign_r, sign_v, sign_rN, sign_d)."""
import numpy as np

import batch_horizon_util as H
import batch_util as BU
import quad_form_shift_util as SU

KEYS = ("Qt", "Rt", "Pt", "r", "v", "rN", "wx", "wu", "wN", "gx", "gu", "gN", "Ct", "d")
FIELDS = dict(zip(KEYS, ("Q", "R", "P", "r", "v", "rN", "wx", "wu", "wN", "gx", "gu", "gN", "C", "d")))        # the struct's names
# weights that tell orders apart: no power of two, negative, zeros of both signs, a tiny and a large one
WEIGHT_POOL = np.array([1.0 / 3.0, -2.5, 0.9, 0.0, -0.0, 0.81, 1.0, -1.0, 0.7853981633974483, 3.0, 1e-3, 0.5])


def slab_doubles(T, nx, nu, term, m):
    n, ns = T * (nx + nu) + term * nx, T * (2 if nu else 1) + term
    return nx * (nx + 1) // 2 + nu * (nu + 1) // 2 + term * (nx * (nx + 1) // 2) + ns + n + 1 + m * n + m


def sections(T, nx, nu, term, m):
    """name -> slice of a slab"""
    n, ns = T * (nx + nu) + term * nx, T * (2 if nu else 1) + term
    nqx, nqu = nx * (nx + 1) // 2, nu * (nu + 1) // 2
    w0 = nqx + nqu + term * nqx
    q = w0 + ns
    return {"SQ": slice(0, nqx), "SR": slice(nqx, nqx + nqu), "SP": slice(nqx + nqu, w0), "W": slice(w0, q), "q": slice(q, q + n),
            "const": slice(q + n, q + n + 1), "C": slice(q + n + 1, q + n + 1 + m * n), "d": slice(q + n + 1 + m * n, q + n + 1 + m * n + m)}


def instance(batch, i, signs):
    """instance i as mathematical matrices: dict with Q, R, P (None), r, v, rN (None where the sign is 0), the weights and linear vectors
    (None where absent), Cm (m, n), d and the signs"""
    g = lambda k: None if batch.get(k) is None else batch[k][i]
    T = batch["T"]
    inst = {"Q": batch["Qt"][i].T, "R": batch["Rt"][i].T, "P": None if batch.get("Pt") is None else batch["Pt"][i].T, "T": T,
            "r": g("r") if signs[0] else None, "v": g("v") if signs[1] else None, "rN": g("rN") if signs[2] else None,
            "Cm": batch["Ct"][i].T, "d": batch["d"][i], "signs": tuple(signs)}
    for k in ("wx", "wu", "wN", "gx", "gu", "gN"):
        inst[k] = g(k)
    return inst


def stage_list(inst):
    """the instance's stages in z order: dicts {M, ref, sign, W (None: no weight array), g (None: no linear vector), kind}"""
    T, nu = inst["T"], len(inst["R"])
    sr, sv, sn, _ = inst["signs"]
    out = []
    for t in range(T):
        out.append({"M": inst["Q"], "ref": inst["r"][t] if sr else None, "sign": sr, "W": None if inst["wx"] is None else inst["wx"][t],
                    "g": None if inst["gx"] is None else inst["gx"][t], "kind": "x"})
        if nu:
            out.append({"M": inst["R"], "ref": inst["v"][t] if sv else None, "sign": sv, "W": None if inst["wu"] is None else inst["wu"][t],
                        "g": None if inst["gu"] is None else inst["gu"][t], "kind": "u"})
    if inst["P"] is not None:
        out.append({"M": inst["P"], "ref": inst["rN"] if sn else None, "sign": sn, "W": None if inst["wN"] is None else inst["wN"],
                    "g": inst["gN"], "kind": "N"})
    return out


def weighted_words(st):
    """(W_s, q words, stage constant) of one stage: W_s * lin_j (+ g_s[j]), W_s * (0.5 * T_s)"""
    lin, const = H.stage_words(st["M"], st["ref"], st["sign"])
    W = np.float64(1.0 if st["W"] is None else st["W"])
    q = W * np.asarray(lin, dtype=np.float64)
    if st["g"] is not None:
        q = q + np.asarray(st["g"], dtype=np.float64)
    return W, q, W * np.float64(const)


def instance_slab(inst):
    nx, nu, T, m = len(inst["Q"]), len(inst["R"]), inst["T"], len(inst["d"])
    term = 0 if inst["P"] is None else 1
    sec = sections(T, nx, nu, term, m)
    out = np.empty(slab_doubles(T, nx, nu, term, m))
    out[sec["SQ"]] = SU.symmetrised(np.asarray(inst["Q"], dtype=np.float64))[np.triu_indices(nx)]
    out[sec["SR"]] = SU.symmetrised(np.asarray(inst["R"], dtype=np.float64))[np.triu_indices(nu)] if nu else []
    out[sec["SP"]] = SU.symmetrised(np.asarray(inst["P"], dtype=np.float64))[np.triu_indices(nx)] if term else []
    words = [weighted_words(st) for st in stage_list(inst)]
    out[sec["W"]] = [w[0] for w in words]
    out[sec["q"]] = np.concatenate([w[1] for w in words])
    out[sec["const"]] = SU.chain_tree_sum(np.array([w[2] for w in words], dtype=np.float64))
    out[sec["C"]] = np.asarray(inst["Cm"], dtype=np.float64).reshape(-1)                # row-major
    out[sec["d"]] = BU.signed(inst["d"], inst["signs"][3])
    return out


def slab_reference(batch, signs):
    """(B, L) slabs of a batch"""
    return np.stack([instance_slab(instance(batch, i, signs)) for i in range(len(batch["Qt"]))])


def expanded_reference(inst, xvar, varmap):
    """what pmt_batch_horizon_terms_expand_f64 leaves for the instance, restated from its slab: (quadratic term words, linear term words,
    constant, vector-affine term words, their constants)"""
    from parametron_jl_amd import _lib
    nx, nu, T, m = len(inst["Q"]), len(inst["R"]), inst["T"], len(inst["d"])
    term = 0 if inst["P"] is None else 1
    sec = sections(T, nx, nu, term, m)
    slab = instance_slab(inst)
    xvar, vm = np.asarray(xvar, dtype=np.int64), np.asarray(varmap, dtype=np.int64)
    n = len(xvar)
    assert n == T * (nx + nu) + term * nx
    quads, zb = [], 0
    for s, st in enumerate(stage_list(inst)):
        nd = len(st["M"])
        S = slab[sec[{"x": "SQ", "u": "SR", "N": "SP"}[st["kind"]]]]
        j, k = np.triu_indices(nd)
        qt = np.empty(len(S), dtype=_lib.QT)
        qt["coeff"] = slab[sec["W"]][s] * S
        qt["row"], qt["col"] = vm[xvar[zb + j] - 1], vm[xvar[zb + k] - 1]
        quads.append(qt)
        zb += nd
    lin = np.empty(n, dtype=_lib.LT)
    lin["coeff"], lin["var"] = slab[sec["q"]], vm[xvar - 1]
    vat = np.empty(m * n, dtype=_lib.VAT)
    vat["out"] = np.repeat(np.arange(1, m + 1, dtype=np.int64), n)
    vat["coeff"] = slab[sec["C"]]
    vat["var"] = np.tile(vm[xvar - 1], m)
    return np.concatenate(quads).view(np.int64), lin.view(np.int64), float(slab[sec["const"]][0]), vat.view(np.int64), slab[sec["d"]].copy()


def instance_table(inst, xvar):
    """the instance's table for pmt_quad_stages_terms_f64 as quad_stages_terms_util takes it: the stages [x_0, u_0, .., x_T] over the n
    variables `xvar` of z, one behind the other, scale = 1.0, weight = W_s (None without a weight array), lin = (1.0, None, g_s)
    -> (stages, nterms, nlin)"""
    xvar = np.asarray(xvar, dtype=np.int64)
    stages, qa, la = [], 0, 0
    for st in stage_list(inst):
        nd = len(st["M"])
        stages.append({"Q": np.asarray(st["M"], dtype=np.float64), "xvar": xvar[la:la + nd],
                       "v": np.asarray(st["ref"], dtype=np.float64) if st["sign"] else None, "sign": st["sign"], "quad_at": qa, "lin_at": la,
                       "W": (1.0, None if st["W"] is None else float(st["W"])),
                       "lin": None if st["g"] is None else (1.0, None, np.asarray(st["g"], dtype=np.float64))})
        qa, la = qa + nd * (nd + 1) // 2, la + nd
    return stages, qa, la


# ---- data

def terms_data(B, T, nx, nu, m, rng, terminal=True, weights=True, linear=True):
    """a batch (module docstring) with batch_horizon_util's mixed data; the weights dealt from WEIGHT_POOL at random, the linear vectors of
    mixed magnitude with zeros"""
    term = 1 if terminal else 0
    n = T * (nx + nu) + term * nx
    Qt, Rt, r, v, _, d = H.horizon_data(B, T, nx, nu, m, rng)
    b = {"T": T, "Qt": Qt, "Rt": Rt, "r": r, "v": v, "d": d, "Ct": H.F.mixed((B, n, m), rng)}
    b["Pt"], b["rN"] = (H.horizon_data(B, 1, nx, 0, 0, rng)[0], H.F.mixed((B, nx), rng)) if terminal else (None, None)
    pick = lambda shape: rng.choice(WEIGHT_POOL, size=shape)
    b["wx"], b["wu"], b["wN"] = (pick((B, T)), pick((B, T)), pick((B,)) if terminal else None) if weights else (None, None, None)

    def vec(shape):
        g = rng.standard_normal(shape) * rng.choice([1.0, 30.0, 1e-2], size=shape)
        g[rng.random(shape) < 0.15] = 0.0
        return g
    b["gx"], b["gu"], b["gN"] = (vec((B, T, nx)), vec((B, T, nu)), vec((B, nx)) if terminal else None) if linear else (None, None, None)
    return b
