"""Shared by the tests of the batch of horizons' compact dynamics sections (pmt_batch_horizon_dynamics_f64,
pmt_batch_horizon_dynamics_expand_f64, batch.BatchMPC): the numpy restatement of both entry points, written from include/parametron_hip.h
alone — nothing is computed there but copies, sign-bit flips (on integer views) and 0.0 (+|-) h —, and the builder of one instance's own
stage tables in affine_stages_util's format, the anchor the header names.

Host arrays are the device's memory images: At[B, nx, nx] with At[i, j, r] = A_i[r, j] (column-major, leading dimension nx), Bt[B, nu, nx]
likewise, h[B, T, nx] stage-major."""
import numpy as np

import affine_stages_util as U

SIGN_BIT = U.SIGN_BIT
ONE = np.float64(1.0).view(np.int64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def section_doubles(T, nx, nu):
    return nx * (nx + nu) + T * nx


def sections(T, nx, nu):
    nab = nx * (nx + nu)
    return {"AB": slice(0, nab), "hconst": slice(nab, nab + T * nx)}


def term_count(T, nx, nu):
    return nx + (T - 1) * nx * (1 + nx + nu)


def dyn_data(B, T, nx, nu, rng):
    """(At, Bt, h): standard normal numbers with zeros of both signs among them, no NaN"""
    return U.special(rng, (B, nx, nx)), U.special(rng, (B, nu, nx)), U.special(rng, (B, T, nx))


def section_reference(At, Bt, h, sign_a, sign_b, sign_h):
    """[B, Ld]: AB[r*(nx+nu) + j] = A_i[r + j*nx] (j < nx) | B_i[r + (j-nx)*nx], the sign bit flipped under sign -1; then 0.0 (+|-) h"""
    B, nx = At.shape[0], At.shape[1]
    nu, T = Bt.shape[1], h.shape[1]
    w = nx + nu
    ab = np.empty((B, nx, w), dtype=np.int64)
    ab[:, :, :nx] = bits(At).transpose(0, 2, 1) ^ (SIGN_BIT if sign_a < 0 else np.int64(0))
    ab[:, :, nx:] = bits(Bt).reshape(B, nu, nx).transpose(0, 2, 1) ^ (SIGN_BIT if sign_b < 0 else np.int64(0))
    hv = np.asarray(h, dtype=np.float64).reshape(B, T * nx)
    hc = (0.0 + hv) if sign_h > 0 else ((0.0 - hv) if sign_h < 0 else np.zeros((B, T * nx)))
    return np.concatenate([ab.reshape(B, nx * w).view(np.float64), hc], axis=1)


def expanded_reference(section, T, nx, nu, sign_xp, xvar, varmap):
    """(terms as 3 words each, constants) of one instance from its section: stage 0 the rows (i + 1, +-1.0, vm[xvar[i]]); stage t >= 1 at
    term nx + (t-1)*nx*(1+nx+nu), row r: (r + 1, +-1.0, vm[xvar[t*(nx+nu) + r]]) and then (r + 1, AB[r*(nx+nu) + j], vm[xvar[(t-1)*(nx+nu) + j]])"""
    w = nx + nu
    sec = sections(T, nx, nu)
    xvar = np.asarray(xvar, dtype=np.int64)
    vm = xvar if varmap is None else np.asarray(varmap, dtype=np.int64)[xvar - 1]
    one = ONE ^ (SIGN_BIT if sign_xp < 0 else np.int64(0))
    ab = bits(section[sec["AB"]]).reshape(nx, w)
    rows = np.arange(1, nx + 1, dtype=np.int64)
    out = [np.stack([rows, np.full(nx, one), vm[:nx]], axis=1).reshape(-1)]
    for t in range(1, T):
        rec = np.empty((nx, 1 + w, 3), dtype=np.int64)
        rec[:, :, 0] = rows[:, None]
        rec[:, 0, 1], rec[:, 0, 2] = one, vm[t * w:t * w + nx]
        rec[:, 1:, 1], rec[:, 1:, 2] = ab, vm[None, (t - 1) * w:t * w]
        out.append(rec.reshape(-1))
    return np.concatenate(out), np.array(section[sec["hconst"]], dtype=np.float64)


def instance_stages(A, Bmat, h, sign_xp, sign_a, sign_b, sign_h, xvar):
    """the instance's own records as affine_stages_util stages, placed one behind the other: A (nx, nx) and Bmat (nx, nu) as matrices,
    h (T, nx) -> (stages, nterms, nconsts)"""
    nx, nu, T = A.shape[0], Bmat.shape[1], h.shape[0]
    w = nx + nu
    xvar = np.asarray(xvar, dtype=np.int64)
    stages = []
    for t in range(T):
        parts = [{"mat": None, "xvar": xvar[t * w:t * w + nx], "sign": sign_xp}]
        if t:
            parts.append({"mat": A, "xvar": xvar[(t - 1) * w:(t - 1) * w + nx], "sign": sign_a})
            if nu:
                parts.append({"mat": Bmat, "xvar": xvar[(t - 1) * w + nx:t * w], "sign": sign_b})
        stages.append({"rows": nx, "parts": parts, "vec": h[t] if sign_h else None, "vec_sign": sign_h, "term_offset": 0, "const_offset": 0})
    nterms, nconsts = U.place(stages)
    return stages, nterms, nconsts
