"""Shared by the tests of the horizon dynamics constraints (pmt_affine_stages_f64, moi.affine_stage_group): the numpy restatement of the
contract, written from include/parametron_hip.h alone, and the dynamics' spellings.

A stage is a dict {"rows", "parts": [{"mat": (rows, cols) array or None, "xvar": int64 model variables, "sign": +1 | -1}], "vec": array or
None, "vec_sign": +1 | -1 | 0, "term_offset", "const_offset"}; a part without a matrix is a Variable vector (xvar has `rows` entries)."""
import numpy as np

VAT = np.dtype([("out", "<i8"), ("coeff", "<f8"), ("var", "<i8")])
SIGN_BIT = np.int64(-2 ** 63)


def row_len(st):
    return sum(1 if p["mat"] is None else p["mat"].shape[1] for p in st["parts"])


def restate_stage(st, varmap):
    """(terms[VAT] row-major, constants) of one stage: term (i + 1, mat[i, j] with its sign bit flipped for sign -1, vm[xvar[j]]) at
    i*row_len + o_p + j; a Variable-vector part (i + 1, +-1.0, vm[xvar[i]]); the constant 0.0 (+|-) vec[i], 0.0 without a vector"""
    rows, L = st["rows"], row_len(st)
    vm = (lambda v: v) if varmap is None else (lambda v: np.asarray(varmap, dtype=np.int64)[v - 1])
    out = np.zeros((rows, L), dtype=np.int64)
    coeff = np.zeros((rows, L), dtype=np.int64)            # the doubles' bit patterns
    var = np.zeros((rows, L), dtype=np.int64)
    out[:] = np.arange(1, rows + 1)[:, None]
    o = 0
    for p in st["parts"]:
        flip = SIGN_BIT if p["sign"] < 0 else np.int64(0)
        x = np.asarray(p["xvar"], dtype=np.int64)
        if p["mat"] is None:
            assert len(x) == rows
            coeff[:, o] = np.float64(1.0).view(np.int64) ^ flip
            var[:, o] = vm(x)
            o += 1
        else:
            m = np.ascontiguousarray(p["mat"], dtype=np.float64)
            assert m.shape == (rows, len(x))
            coeff[:, o:o + len(x)] = m.view(np.int64) ^ flip
            var[:, o:o + len(x)] = vm(x)[None, :]
            o += len(x)
    t = np.zeros(rows * L, dtype=VAT)
    t["out"], t["coeff"], t["var"] = out.reshape(-1), coeff.reshape(-1).view(np.float64), var.reshape(-1)
    if st["vec"] is None:
        c = np.zeros(rows)
    else:
        v = np.asarray(st["vec"], dtype=np.float64)
        c = (0.0 + v) if st["vec_sign"] > 0 else (0.0 - v)
    return t, c


def images(stages, varmap, nterms, nconsts, poison):
    """the whole outputs as 8-byte words: the stages' slices over a background of `poison` words (terms) / NaN (constants)"""
    terms = np.full(3 * nterms, poison, dtype=np.int64)
    consts = np.full(nconsts, np.nan)
    for st in stages:
        t, c = restate_stage(st, varmap)
        terms[3 * st["term_offset"]:3 * (st["term_offset"] + len(t))] = t.view(np.int64)
        consts[st["const_offset"]:st["const_offset"] + len(c)] = c
    return terms, consts


def place(stages):
    """offsets that tile the outputs in table order -> (nterms, nconsts)"""
    ta = ca = 0
    for st in stages:
        st["term_offset"], st["const_offset"] = ta, ca
        ta, ca = ta + st["rows"] * row_len(st), ca + st["rows"]
    return ta, ca


def special(rng, shape):
    """standard normal numbers with +0.0 and -0.0 entries among them (no NaN: its sign under -1 is not part of the contract)"""
    a = rng.standard_normal(shape)
    flat = a.reshape(-1)
    if flat.size:
        k = rng.integers(0, flat.size, size=max(2, flat.size // 7))
        flat[k[0::2]] = 0.0
        flat[k[1::2]] = -0.0
    return a


# ---- the dynamics x+ == A*x + B*u (+ w) as constraint() sees it (lhs - rhs), in four spellings.  Per spelling: the leaves in expression
# order with their effective signs ("x+" | "A" | "B" | "w", sign)
SPELLINGS = {
    "x+ - (A*x + B*u)": [("x+", 1), ("A", -1), ("B", -1)],
    "(A*x + B*u + w) - x+": [("A", 1), ("B", 1), ("w", 1), ("x+", -1)],
    "x+ - A*x - B*u - w": [("x+", 1), ("A", -1), ("B", -1), ("w", -1)],
    "x+ - (A*x - (w - B*u))": [("x+", 1), ("A", -1), ("w", 1), ("B", -1)],
}


def spelled_stage(name, A, B, xp, x, u, w):
    """the stage of one dynamics record: matrices (rows, cols) arrays, xp / x / u model variable indices, w the number vector"""
    parts, vec, vs = [], None, 0
    for leaf, sign in SPELLINGS[name]:
        if leaf == "w":
            vec, vs = w, sign
        elif leaf == "x+":
            parts.append({"mat": None, "xvar": np.asarray(xp, dtype=np.int64), "sign": sign})
        else:
            parts.append({"mat": A if leaf == "A" else B, "xvar": np.asarray(x if leaf == "A" else u, dtype=np.int64), "sign": sign})
    return {"rows": len(xp), "parts": parts, "vec": vec, "vec_sign": vs, "term_offset": 0, "const_offset": 0}


def spelled_expression(name, Ax, Bu, xp, w):
    """the same record's left-hand side minus right-hand side from operands that support + and -: Ax, Bu the products, xp the Variable
    vector, w the number vector"""
    if name == "x+ - (A*x + B*u)":
        return xp - (Ax + Bu)
    if name == "(A*x + B*u + w) - x+":
        return (Ax + Bu + w) - xp
    if name == "x+ - A*x - B*u - w":
        return xp - Ax - Bu - w
    if name == "x+ - (A*x - (w - B*u))":
        return xp - (Ax - (w - Bu))
    raise KeyError(name)
