"""Shared by the tests of the horizon stage costs with identity-weighted terms (pmt_quad_stages_diag_f64; record mode "canonical-stages"
with dot(u_t, u_t) stages and ridge terms): the numpy restatement written from the text of include/parametron_hip.h, the oracle's literal
sequence, and the rounding bounds between the two.

A stage is a dict of quad_stages_terms_util ({Q, xvar, v, sign, quad_at, lin_at, W, lin}) with
  "Q": None      an IDENTITY stage W_t * dot(x (+|-) v, x (+|-) v) (v None with sign 0: W_t * dot(x, x)); it owns n quadratic terms
  "diag":        None, or the RIDER (scale, weight, v_d, sign_d) beside the form of a stage with a Q: W_d * dot(x (+|-) v_d, x (+|-) v_d),
                 v_d None with sign_d 0; W_d = scale * weight as ONE rounded double, or scale.  A missing key is None.

The restatement (c_j = 0.0 (+|-) v_j; S = sum_j c_j*c_j by quad_form_shift_util.chain_tree_sum; plain multiplies and adds):
  identity stage   coeff_j = 2*W_t on (vm[x_j], vm[x_j]);  lin[j] = W_t*(2*c_j) with a v, then + W_c*c_t[j] with a linear term; W_c*c_t[j] alone
                   without v; +0.0 with neither;  constant = W_t*S with a v, +0.0 without.
  rider            the weighted stage of quad_stages_terms_util, except: diagonal coefficient W_t*(2*Q[j,j]) + (2*W_d);  lin[j] = W_t*lin_j, then
                   + W_d*(2*c^d_j) with a v_d, then + W_c*c_t[j];  constant = W_t*cc_t, then + W_d*S with a v_d.
  other stages     quad_stages_terms_util.restate_stage.
The function's constant: quad_stages_terms_util.function_constant over the stages' constants.

The oracle sequence: quad_stages_terms_util.oracle's, with an identity stage's literal function dot(e, e), e = x (+|-) v (vecaddsub and
vecdot_affs_affs; vecdot_vars_vars without v) times W_t (mul_quad_number) at its place among the stages, and every rider's literal function
times W_d added (add_quad) behind the stages and in front of the linear terms; canonicalize!; the MOI copy.

The bounds (u = 2^-53, gamma_m as in quad_form_shift_util; nothing is tuned).  Data away from over- and underflow, so that doubling is exact.
  * Identity stage, quadratic word: the literal function holds W_t * 1.0 on (x_j, x_j), the MOI copy doubles it: 2*W_t in both, bit for bit.
  * Identity stage, linear word: the literal function holds the two terms fl(W_t*c_j) (from c_j*1.0 twice); their sum is 2*fl(W_t*c_j) =
    fl(W_t*(2*c_j)) exactly: bit for bit with the node where the stage has no linear term, and W_c*c_t[j] alone without v is one product in
    both: bit for bit.  With both, canonicalize! adds the three numbers a, a, b in an order its (unstable) sort decides: (a + a) + b as
    the node — one rounding, 2a is exact — or (a + b) + a, two: |node - oracle| <= (u + gamma_2) * (2|a| + |b|)          (ident_lin_bound).
  * Identity stage, constant: the node's W_t*S meets n products, a chain of ceil(n/256) additions and 8 tree levels, then the weight:
    |node - W_t*sum c_j^2| <= gamma_{ceil(n/256)+10} * |W_t| * sum c_j^2; the oracle adds c_j*c_j left to right and scales:
    gamma_{n+1} * |W_t| * sum c_j^2                                                                                   (stage_const_bounds).
  * Rider, diagonal word: node fl(fl(W_t*2Q_jj) + 2W_d); the oracle holds fl(W_t*Q_jj) and W_d, adds them in canonicalize!, and the MOI copy
    doubles: 2*fl(fl(W_t*Q_jj) + W_d), the same double: bit for bit.  Off the diagonal: quad_stages_terms_util.quad_bound.
  * Rider, linear word: exact X = W_t*L_j + 2*W_d*c^d_j + W_c*c_j.  The node is fl(fl(fl(W_t*lin_j) + fl(W_d*(2c^d_j))) + fl(W_c*c_j)) with
    |lin_j - L_j| <= e_j (quad_form_shift_util.node_lin_bound): every addend meets at most 3 roundings (its product, two additions),
    |node - X| <= |W_t|*e_j + gamma_3 * (|W_t*lin_j| + |2 W_d c^d_j| + |W_c c_j|).  The oracle: quad_stages_terms_util.lin_bound's count with two more
    numbers (fl(W_d*c^d_j) twice) in canonicalize!'s sum: gamma_{2n+4} * (|W_t|*A_j + 2|W_d c^d_j| + |W_c c_j|).  Their sum   (rider_lin_bound).
    A rider without a vector leaves the linear word to quad_stages_terms_util.lin_bound.
  * Rider, constant: the node adds a_f = fl(W_t*cc_t) and a_d = fl(W_d*S), one more rounding: e'_t + e_d + u * (|a_f| + |a_d|); the oracle adds
    the rider's constant as an addend of its own behind the stages: f'_t + f_d, and one more addition in its chain   (stage_const_bounds).
  * The function's constant: quad_stages_terms_util.const_bound's formula over these per-stage terms                     (const_bound)."""
import numpy as np

import quad_form_shift_util as S
import quad_stages_terms_util as W
import quad_stages_util as U


def rider(st):
    return st.get("diag")


def is_identity(st):
    return st["Q"] is None


def nquad(st):
    n = len(st["xvar"])
    return n if is_identity(st) else n * (n + 1) // 2


def _sumsq(c):
    return np.float64(S.chain_tree_sum(c * c))


def restate_stage(st, varmap):
    """(quadratic terms, linear terms, constant) of one stage (module docstring)"""
    from parametron_jl_amd import _lib
    d = rider(st)
    if not is_identity(st) and d is None:
        return W.restate_stage(st, varmap)
    xvar = np.asarray(st["xvar"], dtype=np.int64)
    n = len(xvar)
    Wt = np.float64(W.weight(st["W"]))
    ct = np.asarray(st["lin"][2], dtype=np.float64) if st["lin"] is not None else None
    Wc = np.float64(W.weight(st["lin"])) if st["lin"] is not None else None
    if is_identity(st):
        vm = np.asarray(varmap, dtype=np.int64)[xvar - 1]
        quad = np.empty(n, dtype=_lib.QT)
        quad["coeff"], quad["row"], quad["col"] = 2 * Wt, vm, vm
        lin = np.empty(n, dtype=_lib.LT)
        lin["var"] = vm
        if st["sign"]:
            c = S.shift_consts(st["v"], st["sign"])
            lin["coeff"] = Wt * (2 * c)
            if ct is not None:
                lin["coeff"] = lin["coeff"] + Wc * ct
            return quad, lin, float(Wt * _sumsq(c))
        lin["coeff"] = Wc * ct if ct is not None else 0.0
        return quad, lin, 0.0
    quad, lin, const = U.restate_stage(st, varmap)
    quad, lin = quad.copy(), lin.copy()
    Wd = np.float64(W.weight(d))
    quad["coeff"] = Wt * quad["coeff"]
    dj = quad["row"] == quad["col"]
    quad["coeff"][dj] = quad["coeff"][dj] + 2 * Wd
    lin["coeff"] = Wt * lin["coeff"]
    const = Wt * np.float64(const)
    if d[3]:
        cd = S.shift_consts(d[2], d[3])
        lin["coeff"] = lin["coeff"] + Wd * (2 * cd)
        const = const + Wd * _sumsq(cd)
    if ct is not None:
        lin["coeff"] = lin["coeff"] + Wc * ct
    return quad, lin, float(const)


def restate(stages, consts, varmap):
    parts = [restate_stage(st, varmap) for st in stages]
    return parts, W.function_constant([p[2] for p in parts], consts)


def images(stages, consts, varmap, nterms, nlin, poison=-7):
    """whole images of out_quad / out_lin (`poison` outside the slices), the stage constants, the function's constant"""
    parts, const = restate(stages, consts, varmap)
    quad = np.full(3 * nterms, poison, dtype=np.int64)
    lin = np.full(2 * nlin, poison, dtype=np.int64)
    for st, (q, l, _) in zip(stages, parts):
        quad[3 * st["quad_at"]:3 * (st["quad_at"] + len(q))] = q.view(np.int64)
        lin[2 * st["lin_at"]:2 * (st["lin_at"] + len(l))] = l.view(np.int64)
    return quad, lin, np.array([p[2] for p in parts], dtype=np.float64), const


def merged(stages, consts, varmap):
    """the canonical function over the sorted union of the stages' variables: an identity stage's rows hold one term -> (quad, lin, const)"""
    parts, const = restate(stages, consts, varmap)
    x = np.concatenate([np.asarray(st["xvar"], dtype=np.int64) for st in stages])
    rows = np.concatenate([np.asarray(st["xvar"], dtype=np.int64) if is_identity(st) else
                           np.repeat(np.asarray(st["xvar"], dtype=np.int64), np.arange(len(st["xvar"]), 0, -1)) for st in stages])
    quad, lin = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    return quad[np.argsort(rows, kind="stable")], lin[np.argsort(x, kind="stable")], const


def place(stages, gaps):
    """test_gpu_quad_stages.place with an identity stage's n quadratic terms -> (nterms, nlin)"""
    qa = la = 0
    for st, g in zip(stages, gaps):
        st["quad_at"], st["lin_at"] = qa + g, la + g
        qa, la = st["quad_at"] + nquad(st), st["lin_at"] + len(st["xvar"])
    return qa + gaps[-1], la + gaps[-1]


def _literal_diag(xvar, v, sign):
    from oracle import oracle as O
    xvar = np.ascontiguousarray(xvar, dtype=np.int64)
    if not sign:
        return O.Quad().vecdot_vars_vars(xvar, xvar)
    e = O.AffVec(len(xvar)).vecaddsub(xvar, np.ascontiguousarray(v, dtype=np.float64), sign < 0)
    return O.Quad().vecdot_affs_affs(e, e)


def oracle(stages, consts, varmap=None):
    """module docstring: the oracle sequence -> (affine terms, quadratic terms, constant)"""
    from oracle import oracle as O
    total = None
    for st in stages:
        xvar = np.ascontiguousarray(st["xvar"], dtype=np.int64)
        if is_identity(st):
            f = _literal_diag(xvar, st["v"], st["sign"])
        elif st["sign"]:
            Q = np.asarray(st["Q"], dtype=np.float64)
            e = O.AffVec(len(xvar)).vecaddsub(xvar, np.ascontiguousarray(st["v"], dtype=np.float64), st["sign"] < 0)
            f = O.Quad().vecdot_affs_affs(e, O.AffVec(len(xvar)).matvecmul_affs(Q, e))
        else:
            f = O.Quad().bilinearmul(np.asarray(st["Q"], dtype=np.float64), xvar, xvar)
        f = O.Quad().mul_quad_number(f, W.weight(st["W"]))
        total = f if total is None else O.Quad().copy_from(total).add_quad(f)
    for st in stages:
        d = rider(st)
        if d is not None:
            f = O.Quad().mul_quad_number(_literal_diag(st["xvar"], d[2], d[3]), W.weight(d))
            total = O.Quad().copy_from(total).add_quad(f)
    for st in stages:
        if st["lin"] is not None:
            a = O.vecdot_aff_numbers_vars(np.ascontiguousarray(st["lin"][2], dtype=np.float64), np.ascontiguousarray(st["xvar"], dtype=np.int64))
            total = O.Quad().copy_from(total).add_quad(O.Quad().copy_from_aff(O.Aff().mul_aff_number(a, W.weight(st["lin"]))))
    for k in consts:
        total = O.Quad().copy_from(total).add_quad(O.Quad(constant=W.const_value(k)))
    return total.canonicalize().moi(varmap)


def _wc(st):
    n = len(st["xvar"])
    return np.abs(W.weight(st["lin"]) * np.asarray(st["lin"][2], dtype=np.float64)) if st["lin"] is not None else np.zeros(n)


def ident_lin_bound(st):
    """per linear word of an identity stage: 0 (bit for bit) unless it has both a v and a linear term"""
    n = len(st["xvar"])
    if not st["sign"] or st["lin"] is None:
        return np.zeros(n)
    a = np.abs(W.weight(st["W"]) * S.shift_consts(st["v"], st["sign"]))
    return (S.U + S.gamma(2)) * (2 * a + _wc(st))


def _sq_bounds(v, sign, w):
    """(node bound, oracle bound, |w| * sum_j c_j^2) of w * sum_j c_j^2: n products, ceil(n/256) chain additions, 8 tree levels and the
    weight in the node; n products, n - 1 additions and the weight in the oracle"""
    c = S.shift_consts(v, sign)
    n, s = len(c), abs(w) * float(np.sum(c * c))
    return S.gamma(-(-n // 256) + 10) * s, S.gamma(n + 1) * s, s


def rider_lin_bound(st, lin_unweighted):
    """per linear word of a stage with a rider; `lin_unweighted`: the node's lin_j of the unweighted stage (zeros for a plain one)"""
    d = rider(st)
    if not d[3]:
        return W.lin_bound(st, lin_unweighted)
    n = len(st["xvar"])
    Wt = abs(W.weight(st["W"]))
    a = np.abs(W.weight(d) * S.shift_consts(d[2], d[3]))
    if st["sign"]:
        e = S.node_lin_bound(st["Q"], st["v"], st["sign"])
        Qa, c = np.abs(np.asarray(st["Q"], dtype=np.float64)), np.abs(S.shift_consts(st["v"], st["sign"]))
        A = (Qa + Qa.T) @ c
    else:
        e, A = np.zeros(n), np.zeros(n)
    node = Wt * e + S.gamma(3) * (Wt * np.abs(lin_unweighted) + 2 * a + _wc(st))
    return node + S.gamma(2 * n + 4) * (Wt * A + 2 * a + _wc(st))


def stage_const_bounds(st, varmap):
    """(a, e', f') of one stage: a bound on the node's constant in magnitude, the node's and the oracle's distance from the exact one"""
    u = S.U
    if is_identity(st):
        if not st["sign"]:
            return 0.0, 0.0, 0.0
        e, f, s = _sq_bounds(st["v"], st["sign"], W.weight(st["W"]))
        return s + e, e, f
    Wt = abs(W.weight(st["W"]))
    cc = abs(U.restate_stage(st, varmap)[2])
    e = S.node_const_bound(st["Q"], st["v"], st["sign"]) if st["sign"] else 0.0
    f = S.oracle_const_bound(st["Q"], st["v"], st["sign"]) if st["sign"] else 0.0
    a, e1, f1 = Wt * cc * (1 + u), Wt * e + u * Wt * cc, Wt * f + u * Wt * (cc + e + f)       # quad_stages_terms_util.const_bound's terms
    d = rider(st)
    if d is not None and d[3]:
        ed, fd, s = _sq_bounds(d[2], d[3], W.weight(d))
        ad = s + ed
        return (a + ad) * (1 + u), e1 + ed + u * (a + ad), f1 + fd
    return a, e1, f1


def const_bound(stages, consts, varmap):
    """|node constant - oracle constant|: quad_stages_terms_util.const_bound's formula over stage_const_bounds.  The oracle adds the
    riders' constants behind the stages: T - 1 + R + nc additions at the most (R riders with a vector)."""
    b = np.array([stage_const_bounds(st, varmap) for st in stages], dtype=np.float64).reshape(-1, 3)
    a, e1, f1 = b[:, 0], b[:, 1], b[:, 2]
    k = float(np.sum([abs(W.const_value(c)) for c in consts])) if consts else 0.0
    T, nc = len(stages), len(consts)
    R = sum(1 for st in stages if rider(st) is not None and rider(st)[3])
    m = -(-T // 256) + 8 + nc
    return float(np.sum(e1 + f1) + S.gamma(m) * (np.sum(a) + k) + S.gamma(max(T - 1 + R + nc, 1)) * (np.sum(a + e1 + f1) + k))


def make_stages(ns, kinds, seed, weights=None, lin_every=2, special=False, **kw):
    """quad_stages_terms_util.make_stages over sizes `ns`, with a kind per stage:
         "f-" "f0" "f+"            a form stage, shifted by -v, plain, by +v
         "i-" "i0" "i+"            an identity stage dot(x - v, x - v), dot(x, x), dot(x + v, x + v)
       a form kind followed by "r-" "r0" "r+" ("f-r+": the rider's vector is another one than the form's shift, with the other sign)
       -> (stages, varmap, nterms, nlin), the slices one behind the other"""
    signs = {"-": -1, "0": 0, "+": 1}
    stages, varmap, _, _ = W.make_stages(ns, [signs[k[1]] for k in kinds], seed, weights=weights, lin_every=lin_every, special=special, **kw)
    rng = np.random.default_rng(seed + 777)
    wts = W.WEIGHTS if weights is None else weights
    qa = la = 0
    for t, (st, k) in enumerate(zip(stages, kinds)):
        n = len(st["xvar"])
        st["diag"] = None
        if k[0] == "i":
            st["Q"] = None
        elif len(k) == 4:
            sd = signs[k[3]]
            vd = None
            if sd:
                vd = rng.standard_normal(n) * rng.choice([1.0, 25.0, 1e-2], size=n)
                if special:
                    vd[rng.random(n) < 0.2] = 0.0
                    vd[rng.random(n) < 0.2] = -0.0
            st["diag"] = wts[(t + 5) % len(wts)] + (vd, sd)
        st["quad_at"], st["lin_at"] = qa, la
        qa, la = qa + nquad(st), la + n
    return stages, varmap, qa, la
