"""Shared by the tests of the shifted quadratic form transpose(x (+|-) v) * Q * (x (+|-) v) (pmt_quad_form_shift_f64): the numpy restatement of
the order include/parametron_hip.h fixes for its linear part and constant, the oracle's literal composition, and the rounding bounds.

The bounds.  u = 2^-53, gamma_m = m*u / (1 - m*u) (the standard bound on m successive roundings).  With the exact values
    L_j = sum_k (Q[j,k] + Q[k,j]) * c_k        and        C = c'Qc = 0.5 * sum_j c_j * L_j
  * the node rounds S[j,k] once (the sum of two numbers; 2*Q[j,j] is exact), each product S[j,k]*c_k once, and adds along a chain of at most
    63 additions inside a column block and nb - 1 additions over the nb = ceil(n/64) blocks: at most m = 64 + nb roundings on the way of any
    product into lin_j, so  |lin_j - L_j| <= gamma_m * sum_k |S[j,k]*c_k|                                               (node_lin_bound);
  * its constant adds the products c_j*lin_j (one more rounding) along a chain of ceil(n/256) additions and 8 tree levels; the halving is
    exact:  |const - C| <= 0.5 * gamma_{m + 9 + ceil(n/256)} * sum_j |c_j| * sum_k |S[j,k]*c_k|                        (node_const_bound);
  * the oracle's literal function holds, for x_j, the row constant sum_k Q[j,k]*c_k (n products, n - 1 additions) and the n terms
    c_k*Q[k,j]; canonicalize! adds these n + 1 numbers in an order the sort decides — at most 2n roundings on the way of any product:
    |oracle_lin_j - L_j| <= gamma_{2n} * sum_k (|Q[j,k]| + |Q[k,j]|)*|c_k|                                              (oracle_lin_bound);
  * its constant is sum_j c_j * (row constant j), a chain over j of products of chains over k: at most 2n + 1 roundings:
    |oracle_const - C| <= gamma_{2n+1} * sum_jk |c_j*Q[j,k]*c_k|                                                       (oracle_const_bound).
Two computed values of the same exact number differ by at most the sum of their bounds.  Nothing here is tuned."""
import numpy as np

U = 2.0 ** -53
TILE = 64


def gamma(m):
    return m * U / (1 - m * U)


def shift_consts(v, sign):
    """c_j = 0.0 + v_j (sign +1) or 0.0 - v_j (sign -1): the constants of x (+|-) v (pmt_vars_addsub_f64, a PMT_LSQ_DIAG term)"""
    v = np.asarray(v, dtype=np.float64)
    return (0.0 + v) if sign > 0 else (0.0 - v)


def symmetrised(Q):
    """S[j,k] = Q[j,k] + Q[k,j] (rounded, bitwise symmetric), S[j,j] = 2*Q[j,j]"""
    Q = np.asarray(Q, dtype=np.float64)
    S = Q + Q.T
    S[np.diag_indices(len(Q))] = 2 * np.diag(Q)
    return S


def chain_tree_sum(t):
    """sum_j t_j in S_d's order: 256 chains (chain r adds j = r, r + 256, .. in order onto 0.0), then the halving tree"""
    red = np.zeros(256)
    for s in range(0, len(t), 256):
        seg = t[s:s + 256]
        red[:len(seg)] = red[:len(seg)] + seg
    h = 128
    while h:
        red[:h] = red[:h] + red[h:2 * h]
        h >>= 1
    return red[0]


def restate_shift(Q, v, sign):
    """(lin, const) of the shifted form in the header's order; plain float64 multiplies and adds in the stated sequence"""
    S, c = symmetrised(Q), shift_consts(v, sign)
    n = len(c)
    lin = None
    for k0 in range(0, n, TILE):
        prod = S[:, k0:k0 + TILE] * c[k0:k0 + TILE]
        part = prod[:, 0].copy()                           # the first product starts the chain
        for kk in range(1, prod.shape[1]):
            part = part + prod[:, kk]
        lin = part if lin is None else lin + part          # the blocks in order
    return lin, 0.5 * chain_tree_sum(c * lin)


def node_lin_bound(Q, v, sign):
    S, c = symmetrised(Q), shift_consts(v, sign)
    nb = -(-len(c) // TILE)
    return gamma(64 + nb) * (np.abs(S) @ np.abs(c))


def node_const_bound(Q, v, sign):
    S, c = symmetrised(Q), shift_consts(v, sign)
    n = len(c)
    nb = -(-n // TILE)
    return 0.5 * gamma(64 + nb + 9 + -(-n // 256)) * float(np.abs(c) @ (np.abs(S) @ np.abs(c)))


def oracle_lin_bound(Q, v, sign):
    Q, c = np.abs(np.asarray(Q, dtype=np.float64)), np.abs(shift_consts(v, sign))
    return gamma(2 * len(c)) * ((Q + Q.T) @ c)


def oracle_const_bound(Q, v, sign):
    Q, c = np.abs(np.asarray(Q, dtype=np.float64)), np.abs(shift_consts(v, sign))
    return gamma(2 * len(c) + 1) * float(c @ (Q @ c))


def oracle_tracking(Q, xvar, v, sign, varmap=None):
    """the oracle's literal composition: e = x (+|-) v, dot(e, Q*e) by matvecmul! over the affine vector and vecdot!, canonicalize!, the MOI
    copy -> (affine terms, quadratic terms, constant)"""
    from oracle import oracle as O
    xvar = np.ascontiguousarray(xvar, dtype=np.int64)
    n = len(xvar)
    e = O.AffVec(n).vecaddsub(xvar, np.ascontiguousarray(v, dtype=np.float64), sign < 0)
    Qe = O.AffVec(n).matvecmul_affs(np.asarray(Q, dtype=np.float64), e)
    return O.Quad().vecdot_affs_affs(e, Qe).canonicalize().moi(varmap)


def make_case(n, seed, special=False):
    """(Q, v, xvar, varmap): a non-symmetric Q with mixed magnitudes, x strictly increasing among n + 9 variables, a permuting, offset varmap;
    `special`: +0.0 and -0.0 in Q and v, equal-and-opposite pairs in Q"""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((n, n)) * rng.choice([1.0, -3.0, 1e-3, 40.0], size=(n, n))
    v = rng.standard_normal(n) * rng.choice([1.0, 25.0, 1e-2], size=n)
    if special:
        k = rng.integers(0, 5, size=(n, n))
        Q = np.where(k == 0, 0.0, Q)
        Q = np.where(k == 1, -0.0, Q)
        lo = np.tril_indices(n, -1)
        opp = rng.random(len(lo[0])) < 0.3
        Q[lo[0][opp], lo[1][opp]] = -Q[lo[1][opp], lo[0][opp]]
        kv = rng.integers(0, 4, size=n)
        v = np.where(kv == 0, 0.0, v)
        v = np.where(kv == 1, -0.0, v)
    nvars = n + 9
    xvar = np.sort(rng.choice(np.arange(1, nvars + 1), n, replace=False)).astype(np.int64)
    varmap = (rng.permutation(nvars) + 1 + 100).astype(np.int64)
    return np.ascontiguousarray(Q), np.ascontiguousarray(v), xvar, varmap
