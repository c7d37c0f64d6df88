"""Shared by the tests of the weighted horizon stage costs (pmt_quad_stages_terms_f64; record mode "canonical-stages" with weights, linear
terms and constants beside the stages): the numpy restatement written from the text of include/parametron_hip.h, the oracle's literal
sequence, and the rounding bounds between the two.

A stage is a dict of quad_stages_util ({Q, xvar, v, sign, quad_at, lin_at}) with two more keys:
  "W":   (scale, weight) — weight a number (the value of a scalar Parameter) or None; W_t = scale * weight as ONE rounded double, or scale
  "lin": None, or (lin_scale, lin_weight, c) — c the n numbers of dot(c, x_t); W_c likewise
A constant is (scale, weight, value), weight / value numbers or None: k_i = W_i * (value or 1.0).

The restatement.  With quad c(j,k), lin_j and cc_t of the unweighted stage (quad_stages_util.restate_stage), plain multiplies and adds:
    coeff(j,k) = W_t * c(j,k);   lin[j] = W_t * lin_j, then + W_c * c[j] when the stage has a linear term;   stage constant = W_t * cc_t;
the function's constant is the chain-then-tree sum of the stage constants (quad_form_shift_util.chain_tree_sum), then s = s + k_i in order.

The oracle sequence: every stage's literal function as in quad_stages_util.oracle, multiplied by W_t (mul!: every coefficient and the
constant times the one double W_t) and added in stage order (add!); then the linear terms dot(c, x_t) (vecdot!) scaled by W_c and the
constants k_i, added in that order; canonicalize!; the MOI copy.

The bounds (u = 2^-53, gamma_m as in quad_form_shift_util; nothing is tuned; first factors of (1 + d) are collected into gamma_m the standard way).
No pair (j, k) and no variable is shared between stages.
  * A quadratic coefficient off the diagonal is fl(W * fl(a + b)) in the node and fl(fl(W*a) + fl(W*b)) in the oracle (the literal function holds the
    two terms a = Q[j,k] and b = Q[k,j], each scaled, canonicalize! adds them).  Scaling by a power of two, of either sign, is exact: for such a W
    the two are equal bit for bit — except in the sign of a zero under a negative W: where a + b is +0.0 (a = -b, or zeros of opposite sign) the
    node holds W * (+0.0) = -0.0 and the oracle (W*a) + (W*b) = +0.0; they are equal as numbers.  Otherwise the node is within gamma_2 * |W| * |a + b| of W * (a + b) (two roundings) and the oracle within
    gamma_2 * |W| * (|a| + |b|) (each product meets two roundings):
        |node - oracle| <= gamma_2 * |W| * (|a + b| + |a| + |b|)                                                       (quad_bound).
    On the diagonal both hold 2 * fl(W * Q[j,j]) = fl(W * (2 * Q[j,j])): equal bit for bit (the bound above, with b = a, is not needed).
  * A linear coefficient.  Exact value X = W * L_j + W_c * c_j.  The node: fl(fl(W * lin_j) + fl(W_c * c_j)) with |lin_j - L_j| <= e_j
    (quad_form_shift_util.node_lin_bound), so |node - X| <= |W| * e_j + gamma_2 * (|W * lin_j| + |W_c * c_j|).  The oracle: the n + 1 numbers of
    the unweighted literal function (at most 2n roundings on the way of any product, quad_form_shift_util) each meet one more rounding (times W),
    W_c * c_j meets one, and canonicalize! adds n + 2 numbers instead of n + 1 (one more addition): at most 2n + 2 roundings,
    |oracle - X| <= gamma_{2n+2} * (|W| * A_j + |W_c * c_j|), A_j = sum_k (|Q[j,k]| + |Q[k,j]|) * |c_k|.  A plain stage has e_j = lin_j = A_j = 0.
        |node - oracle| <= the sum of the two                                                                          (lin_bound).
  * The constant.  Stage t: exact W * C_t.  The node holds a_t = fl(W * cc_t), |cc_t - C_t| <= e_t (node_const_bound):
    |a_t - W * C_t| <= e'_t = |W| * e_t + u * |W * cc_t|.  The oracle holds b_t = fl(W * cc'_t), |cc'_t - C_t| <= f_t (oracle_const_bound),
    |cc'_t| <= |cc_t| + e_t + f_t: |b_t - W * C_t| <= f'_t = |W| * f_t + u * |W| * (|cc_t| + e_t + f_t).  The constants k_i are the same doubles
    in both.  The node adds the a_t along ceil(T / 256) chain additions and 8 tree levels, then the nc constants: every a_t meets at most
    m = ceil(T / 256) + 8 + nc roundings, every k_i at most nc.  The oracle adds left to right: at most T - 1 + nc roundings (the linear terms
    add 0.0 to the constant: exact).  With |b_t| <= |a_t| + e'_t + f'_t:
        |node - oracle| <= sum_t (e'_t + f'_t) + gamma_m * (sum_t |a_t| + sum_i |k_i|)
                           + gamma_{T-1+nc} * (sum_t (|a_t| + e'_t + f'_t) + sum_i |k_i|)                              (const_bound)."""
import numpy as np

import quad_form_shift_util as S
import quad_stages_util as U


def weight(pair):
    """W = scale * weight as one double, or scale"""
    scale, w = pair[0], pair[1]
    return float(np.float64(scale) * np.float64(w)) if w is not None else float(scale)


def const_value(k):
    """k_i = W_i * (value or 1.0)"""
    return float(np.float64(weight(k)) * np.float64(k[2] if k[2] is not None else 1.0))


def restate_stage(st, varmap):
    """(quadratic terms, linear terms, constant) of one weighted stage"""
    quad, lin, const = U.restate_stage(st, varmap)
    W = np.float64(weight(st["W"]))
    quad, lin = quad.copy(), lin.copy()
    quad["coeff"] = W * quad["coeff"]
    lin["coeff"] = W * lin["coeff"]
    if st["lin"] is not None:
        lin["coeff"] = lin["coeff"] + np.float64(weight(st["lin"])) * np.asarray(st["lin"][2], dtype=np.float64)
    return quad, lin, float(W * np.float64(const))


def function_constant(stage_consts, consts):
    s = np.float64(S.chain_tree_sum(np.asarray(stage_consts, dtype=np.float64)))
    for k in consts:
        s = s + np.float64(const_value(k))
    return float(s)


def restate(stages, consts, varmap):
    """per stage (quad, lin, const), and the function's constant"""
    parts = [restate_stage(st, varmap) for st in stages]
    return parts, function_constant([p[2] for p in parts], consts)


def images(stages, consts, varmap, nterms, nlin, poison=-7):
    """quad_stages_util.images for weighted stages: whole images of out_quad / out_lin, the stage constants, the function's constant"""
    parts, const = restate(stages, consts, varmap)
    quad = np.full(3 * nterms, poison, dtype=np.int64)
    lin = np.full(2 * nlin, poison, dtype=np.int64)
    for st, (q, l, _) in zip(stages, parts):
        quad[3 * st["quad_at"]:3 * (st["quad_at"] + len(q))] = q.view(np.int64)
        lin[2 * st["lin_at"]:2 * (st["lin_at"] + len(l))] = l.view(np.int64)
    return quad, lin, np.array([p[2] for p in parts], dtype=np.float64), const


def merged(stages, consts, varmap):
    """the canonical function over the sorted union of the stages' variables (quad_stages_util.merged) -> (quad, lin, const)"""
    parts, const = restate(stages, consts, varmap)
    x = np.concatenate([np.asarray(st["xvar"], dtype=np.int64) for st in stages])
    rows = np.concatenate([np.repeat(np.asarray(st["xvar"], dtype=np.int64), np.arange(len(st["xvar"]), 0, -1)) for st in stages])
    quad, lin = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    return quad[np.argsort(rows, kind="stable")], lin[np.argsort(x, kind="stable")], const


def oracle(stages, consts, varmap=None):
    """module docstring: the oracle sequence -> (affine terms, quadratic terms, constant)"""
    from oracle import oracle as O
    total = None
    for st in stages:
        xvar = np.ascontiguousarray(st["xvar"], dtype=np.int64)
        Q = np.asarray(st["Q"], dtype=np.float64)
        if st["sign"]:
            e = O.AffVec(len(xvar)).vecaddsub(xvar, np.ascontiguousarray(st["v"], dtype=np.float64), st["sign"] < 0)
            f = O.Quad().vecdot_affs_affs(e, O.AffVec(len(xvar)).matvecmul_affs(Q, e))
        else:
            f = O.Quad().bilinearmul(Q, xvar, xvar)
        f = O.Quad().mul_quad_number(f, weight(st["W"]))
        total = f if total is None else O.Quad().copy_from(total).add_quad(f)
    for st in stages:
        if st["lin"] is not None:
            a = O.vecdot_aff_numbers_vars(np.ascontiguousarray(st["lin"][2], dtype=np.float64), np.ascontiguousarray(st["xvar"], dtype=np.int64))
            total = O.Quad().copy_from(total).add_quad(O.Quad().copy_from_aff(O.Aff().mul_aff_number(a, weight(st["lin"]))))
    for k in consts:
        total = O.Quad().copy_from(total).add_quad(O.Quad(constant=const_value(k)))
    return total.canonicalize().moi(varmap)


def quad_bound(st):
    """per quadratic term of the stage, in the slice's order (row j: its columns k >= j): 0 for W a power of two and on the diagonal"""
    Q = np.asarray(st["Q"], dtype=np.float64)
    W = abs(weight(st["W"]))
    n = len(Q)
    j, k = np.triu_indices(n)
    a, b = Q[j, k], Q[k, j]
    bound = S.gamma(2) * W * (np.abs(a + b) + np.abs(a) + np.abs(b))
    exact = W == 0.0 or np.frexp(W)[0] == 0.5
    return np.where((j == k) | exact, 0.0, bound)


def lin_bound(st, lin_unweighted):
    """per linear term of the stage; `lin_unweighted`: the node's lin_j of the unweighted stage (zeros for a plain one)"""
    n = len(st["xvar"])
    W = abs(weight(st["W"]))
    wc = np.abs(weight(st["lin"]) * np.asarray(st["lin"][2], dtype=np.float64)) if st["lin"] is not None else np.zeros(n)
    if st["sign"]:
        e = S.node_lin_bound(st["Q"], st["v"], st["sign"])
        Qa, c = np.abs(np.asarray(st["Q"], dtype=np.float64)), np.abs(S.shift_consts(st["v"], st["sign"]))
        A = (Qa + Qa.T) @ c
    else:
        e, A = np.zeros(n), np.zeros(n)
    node = W * e + S.gamma(2) * (W * np.abs(lin_unweighted) + wc)
    return node + S.gamma(2 * n + 2) * (W * A + wc)


def const_bound(stages, consts, varmap):
    """|node constant - oracle constant| (module docstring)"""
    u = S.U
    W = np.array([abs(weight(st["W"])) for st in stages])
    cc = np.array([abs(U.restate_stage(st, varmap)[2]) for st in stages])
    e = np.array([S.node_const_bound(st["Q"], st["v"], st["sign"]) if st["sign"] else 0.0 for st in stages])
    f = np.array([S.oracle_const_bound(st["Q"], st["v"], st["sign"]) if st["sign"] else 0.0 for st in stages])
    a = W * cc * (1 + u)                                                 # |a_t| <= |W * cc_t| * (1 + u)
    e1 = W * e + u * W * cc
    f1 = W * f + u * W * (cc + e + f)
    k = float(np.sum([abs(const_value(c)) for c in consts])) if consts else 0.0
    T, nc = len(stages), len(consts)
    m = -(-T // 256) + 8 + nc
    return float(np.sum(e1 + f1) + S.gamma(m) * (np.sum(a) + k) + S.gamma(max(T - 1 + nc, 1)) * (np.sum(a + e1 + f1) + k))


WEIGHTS = [(1.0, None), (0.5, None), (-1.0, None), (3.0, None), (1.0 / 3.0, None), (1.0, 0.7853981633974483), (-2.5, 1.375)]


def make_stages(ns, signs, seed, weights=None, lin_every=2, **kw):
    """quad_stages_util.make_stages with a weight per stage dealt out in turn from `weights` (default WEIGHTS) and a linear term on every
    `lin_every`-th stage (0: none), its own weight dealt out likewise -> (stages, varmap, nterms, nlin)"""
    stages, varmap, nterms, nlin = U.make_stages(ns, signs, seed, **kw)
    rng = np.random.default_rng(seed + 12345)
    weights = WEIGHTS if weights is None else weights
    for t, st in enumerate(stages):
        st["W"] = weights[t % len(weights)]
        st["lin"] = None
        if lin_every and t % lin_every == 0:
            c = rng.standard_normal(len(st["xvar"])) * rng.choice([1.0, 30.0, 1e-2], size=len(st["xvar"]))
            c[rng.random(len(c)) < 0.15] = 0.0
            st["lin"] = weights[(t + 3) % len(weights)] + (c,)
    return stages, varmap, nterms, nlin


def make_consts(count, seed=5):
    """`count` constants: numbers folded into the scale, Parameter values and Parameter weights in turn"""
    rng = np.random.default_rng(seed)
    kinds = [lambda: (float(rng.standard_normal()), None, None), lambda: (1.0, None, float(rng.standard_normal())),
             lambda: (-0.5, float(rng.standard_normal()), float(rng.standard_normal())), lambda: (3.0, float(rng.standard_normal()), None)]
    return [kinds[i % 4]() for i in range(count)]
