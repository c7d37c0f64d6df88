"""Shared by the tests of the horizon stage costs (pmt_quad_stages_f64, record mode "canonical-stages"): the numpy restatement written from
the text of include/parametron_hip.h, the oracle's literal sequence, and the rounding bounds between the two.

A stage is a dict {Q, xvar, v, sign, quad_at, lin_at}: Q an n x n array, xvar n strictly increasing model-variable indices, v the vector
(None with sign 0), and the stage's first quadratic / linear term in the outputs.

The restatement.  A stage's words are those of the single node: the quadratic terms of pmt_quad_form_f64 (test_quad_form_host.restate_form),
lin and 0.5*T of pmt_quad_form_shift_f64 (quad_form_shift_util.restate_shift: 64-column chains, the first product starting the chain, the
blocks in order; 256 chains onto 0.0 and the halving tree); a plain stage has lin = +0.0 and the constant +0.0.  The function's constant is
the sum of the stages' constants in S_d's order (quad_form_shift_util.chain_tree_sum: chain c adds the stages c, c + 256, .. in order onto
0.0, then the halving tree).

The oracle sequence: every stage's literal function (bilinearmul! for a plain stage; vecaddsub, matvecmul! and vecdot! for a shifted one),
the stages added in expression order (add!: the sum so far, then the stage), canonicalize!, the MOI copy.

The bounds (u = 2^-53, gamma_m as in quad_form_shift_util; nothing is tuned).  No pair (j, k) and no variable is shared between stages, so:
  * a quadratic coefficient is the sum of two numbers in both: equal bit for bit;
  * a linear coefficient of stage t is that stage's alone in both: |node - oracle| <= node_lin_bound + oracle_lin_bound of the stage;
  * the constant.  Let c_t be the exact constant of stage t, a_t / b_t the node's / the oracle's computed ones, with
    |a_t - c_t| <= e_t = node_const_bound(t) and |b_t - c_t| <= f_t = oracle_const_bound(t).  The node adds T numbers along a chain of
    ceil(T / 256) additions and 8 tree levels; to first order each a_t meets at most m = ceil(T / 256) + 8 roundings:
        |node - sum_t c_t| <= sum_t e_t + gamma_m * sum_t |a_t|.
    The oracle adds them left to right, at most T - 1 roundings: |oracle - sum_t c_t| <= sum_t f_t + gamma_{T-1} * sum_t |b_t|.
    With |b_t| <= |a_t| + e_t + f_t the two differ by at most
        sum_t (e_t + f_t) + gamma_m * sum_t |a_t| + gamma_{T-1} * sum_t (|a_t| + e_t + f_t)                    (const_bound)."""
import numpy as np

import quad_form_shift_util as S
from test_quad_form_host import restate_form


def restate_stage(st, varmap):
    """(quadratic terms, linear terms, constant) of one stage, as the single node writes them with moi = 1 and alpha = 1.0"""
    from parametron_jl_amd import _lib
    Q, xvar = np.asarray(st["Q"], dtype=np.float64), np.asarray(st["xvar"], dtype=np.int64)
    n = len(xvar)
    coeff, row, col = restate_form(Q, xvar, varmap, 1)
    quad = np.empty(n * (n + 1) // 2, dtype=_lib.QT)
    quad["coeff"], quad["row"], quad["col"] = coeff, row, col
    lin = np.empty(n, dtype=_lib.LT)
    lin["var"] = np.asarray(varmap, dtype=np.int64)[xvar - 1]
    if st["sign"]:
        lin["coeff"], const = S.restate_shift(Q, st["v"], st["sign"])
    else:
        lin["coeff"], const = 0.0, 0.0
    return quad, lin, float(const)


def restate(stages, varmap):
    """per stage (quad, lin, const), and the function's constant in S_d's order over the stages"""
    parts = [restate_stage(st, varmap) for st in stages]
    return parts, float(S.chain_tree_sum(np.array([p[2] for p in parts], dtype=np.float64)))


def images(stages, varmap, nterms, nlin, poison=-7):
    """the whole images of out_quad (3 * nterms words) and out_lin (2 * nlin words) — `poison` wherever no stage's slice lies —, the
    stages' constants and the function's constant"""
    parts, const = restate(stages, varmap)
    quad = np.full(3 * nterms, poison, dtype=np.int64)
    lin = np.full(2 * nlin, poison, dtype=np.int64)
    for st, (q, l, _) in zip(stages, parts):
        quad[3 * st["quad_at"]:3 * (st["quad_at"] + len(q))] = q.view(np.int64)
        lin[2 * st["lin_at"]:2 * (st["lin_at"] + len(l))] = l.view(np.int64)
    return quad, lin, np.array([p[2] for p in parts], dtype=np.float64), const


def merged(stages, varmap):
    """the canonical function over the sorted union of the stages' variables: rows by increasing model variable, a stage's row keeping its own
    columns; linear terms by increasing variable; the constant -> (quad, lin, const), the layout of "canonical-groups" / "canonical-stages" """
    parts, const = restate(stages, varmap)
    x = np.concatenate([np.asarray(st["xvar"], dtype=np.int64) for st in stages])
    rows = np.concatenate([np.repeat(np.asarray(st["xvar"], dtype=np.int64), np.arange(len(st["xvar"]), 0, -1)) for st in stages])
    quad, lin = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    return quad[np.argsort(rows, kind="stable")], lin[np.argsort(x, kind="stable")], const


def oracle(stages, varmap=None):
    """the literal functions per stage, added in expression order, canonicalize!, the MOI copy -> (affine terms, quadratic terms, constant)"""
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
        total = f if total is None else O.Quad().copy_from(total).add_quad(f)
    return total.canonicalize().moi(varmap)


def lin_bound(st):
    """per linear term of the stage: the node's bound plus the oracle's (a plain stage: both hold +0.0 or no term at all)"""
    if not st["sign"]:
        return np.zeros(len(st["xvar"]))
    return S.node_lin_bound(st["Q"], st["v"], st["sign"]) + S.oracle_lin_bound(st["Q"], st["v"], st["sign"])


def const_bound(stages, consts):
    """|node constant - oracle constant| (module docstring); `consts`: the node's stage constants a_t"""
    e = np.array([S.node_const_bound(st["Q"], st["v"], st["sign"]) if st["sign"] else 0.0 for st in stages])
    f = np.array([S.oracle_const_bound(st["Q"], st["v"], st["sign"]) if st["sign"] else 0.0 for st in stages])
    a = np.abs(np.asarray(consts, dtype=np.float64))
    T = len(stages)
    m = -(-T // 256) + 8
    return float(np.sum(e + f) + S.gamma(m) * np.sum(a) + S.gamma(max(T - 1, 1)) * np.sum(a + e + f))


def lin_by_var(terms):
    """{variable: coefficient} of linear terms (the oracle holds no term for a plain stage's variables; the node holds 0.0)"""
    return dict(zip(terms["var"].tolist(), terms["coeff"].tolist()))


def make_stages(ns, signs, seed, shared=2, special=False, interleave=False, nvars_extra=5):
    """stages of sizes `ns` and signs `signs` over pairwise disjoint, strictly increasing variable sets, `shared` weight matrices per size
    dealt out in turn, slices one behind the other; a permuting, offset varmap -> (stages, varmap, nterms, nlin).  `interleave`: the
    variables of the stages are dealt out element by element (no stage's variables are consecutive)."""
    rng = np.random.default_rng(seed)
    total = int(np.sum(ns))
    nvars = total + nvars_extra
    pool = np.sort(rng.choice(np.arange(1, nvars + 1), total, replace=False)).astype(np.int64)
    if interleave:
        owner = np.concatenate([np.arange(len(ns))[np.array(ns) > k] for k in range(max(ns))])
    else:
        owner = np.repeat(np.arange(len(ns)), ns)
    mats, stages, qa, la = {}, [], 0, 0
    for t, (n, sign) in enumerate(zip(ns, signs)):
        key = (n, t % shared)
        Q, v, _, _ = S.make_case(n, seed + 31 * t + 7, special=special)
        Q = mats.setdefault(key, Q)
        stages.append({"Q": Q, "xvar": pool[owner == t], "v": v if sign else None, "sign": sign, "quad_at": qa, "lin_at": la})
        qa, la = qa + n * (n + 1) // 2, la + n
    varmap = (rng.permutation(nvars) + 1 + 100).astype(np.int64)
    return stages, varmap, qa, la
