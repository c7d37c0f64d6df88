"""Shared by the tests of the batch of horizons' time-varying dynamics sections (pmt_batch_horizon_dynamics_tv_f64,
pmt_batch_horizon_dynamics_tv_expand_f64, batch.BatchLTVMPC, batch.BatchWeightedLTVMPC): the restatement of both entry points, written from
include/parametron_hip.h alone — nothing is computed there but copies, sign-bit flips (on integer views) and 0.0 (+|-) h, so these are plain
loops over instance, stage and row —, and the builder of one instance's own stage tables in affine_stages_util's format with a matrix pair
per stage, the anchor the header names.

Host arrays are the device's memory images: At[B, T-1, nx, nx] with At[i, s, j, r] = A_{i,s+1}[r, j] (column-major, leading dimension nx;
matrix index s belongs to record s + 1), Bt[B, T-1, nu, nx] likewise, h[B, T, nx] stage-major."""
import numpy as np

import affine_stages_util as U

SIGN_BIT = U.SIGN_BIT
ONE = np.float64(1.0).view(np.int64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def section_doubles(T, nx, nu):
    return (T - 1) * nx * (nx + nu) + T * nx


def sections(T, nx, nu):
    """"AB": the slice of AB_t at index t - 1; "hconst": the constants"""
    nab = nx * (nx + nu)
    return {"AB": [slice(s * nab, (s + 1) * nab) for s in range(T - 1)], "hconst": slice((T - 1) * nab, (T - 1) * nab + T * nx)}


def term_count(T, nx, nu):
    return nx + (T - 1) * nx * (1 + nx + nu)


def ltv_data(B, T, nx, nu, rng):
    """(At, Bt, h): standard normal numbers with zeros of both signs among them, no NaN"""
    return U.special(rng, (B, T - 1, nx, nx)), U.special(rng, (B, T - 1, nu, nx)), U.special(rng, (B, T, nx))


def encoded_data(B, T, nx, nu):
    """(At, Bt, h) whose values name their place: |A_{i,s}[r, j]| = (((i*512 + s)*128 + r)*256 + j) + 0.5 with column j of [A | B] (B's columns
    from nx on), |h_{i,t}[r]| = ((i*512 + t)*128 + r) + 0.25 — exact doubles, all different, negative where the indices' sum is odd: a block
    of another item, a transposed index or a dropped sign flip differs"""
    i = np.arange(B, dtype=np.int64)[:, None, None, None]
    s = np.arange(T - 1, dtype=np.int64)[None, :, None, None]
    r = np.arange(nx, dtype=np.int64)[None, None, None, :]

    def mat(cols, first):
        j = first + np.arange(cols, dtype=np.int64)[None, None, :, None]
        code = (((i * 512 + s) * 128 + r) * 256 + j).astype(np.float64) + 0.5
        return np.where((i + s + r + j) % 2 == 1, -code, code)

    ih, th, rh = np.arange(B, dtype=np.int64)[:, None, None], np.arange(T, dtype=np.int64)[None, :, None], np.arange(nx, dtype=np.int64)[None, None, :]
    hcode = ((ih * 512 + th) * 128 + rh).astype(np.float64) + 0.25
    return mat(nx, 0), mat(nu, nx), np.where((ih + th + rh) % 2 == 1, -hcode, hcode)


def section_reference(At, Bt, h, sign_a, sign_b, sign_h):
    """[B, Ltv]: AB_t[r*(nx+nu) + j] = A_{i,t}[r + j*nx] (j < nx) | B_{i,t}[r + (j-nx)*nx] at (t-1)*nx*(nx+nu), the sign bit flipped under
    sign -1; then h-consts[t*nx + r] = 0.0 (+|-) h"""
    B, nx = At.shape[0], At.shape[2]
    nu, T = Bt.shape[2], h.shape[1]
    w = nx + nu
    nab = nx * w
    a, b = bits(At), bits(Bt)
    fa, fb = (SIGN_BIT if sign_a < 0 else np.int64(0)), (SIGN_BIT if sign_b < 0 else np.int64(0))
    out = np.empty((B, section_doubles(T, nx, nu)), dtype=np.int64)
    hv = np.asarray(h, dtype=np.float64).reshape(B, T * nx)
    for i in range(B):
        for s in range(T - 1):
            for r in range(nx):
                at = s * nab + r * w
                out[i, at:at + nx] = a[i, s, :, r] ^ fa                   # A_{i,s+1}[r + j*nx], j = 0 .. nx-1
                out[i, at + nx:at + w] = b[i, s, :, r] ^ fb
        hc = (0.0 + hv[i]) if sign_h > 0 else ((0.0 - hv[i]) if sign_h < 0 else np.zeros(T * nx))
        out[i, (T - 1) * nab:] = bits(hc)
    return out.view(np.float64)


def expanded_reference(section, T, nx, nu, sign_xp, xvar, varmap):
    """(terms as 3 words each, constants) of one instance from its section: stage 0 the rows (i + 1, +-1.0, vm[xvar[i]]); stage t >= 1 at
    term nx + (t-1)*nx*(1+nx+nu), row r: (r + 1, +-1.0, vm[xvar[t*(nx+nu) + r]]) and then (r + 1, AB_t[r*(nx+nu) + j], vm[xvar[(t-1)*(nx+nu) + j]])"""
    w = nx + nu
    nab = nx * w
    xvar = np.asarray(xvar, dtype=np.int64)
    vm = xvar if varmap is None else np.asarray(varmap, dtype=np.int64)[xvar - 1]
    one = ONE ^ (SIGN_BIT if sign_xp < 0 else np.int64(0))
    sec = bits(section)
    terms = np.empty((term_count(T, nx, nu), 3), dtype=np.int64)
    for r in range(nx):
        terms[r] = (r + 1, one, vm[r])
    k = nx
    for t in range(1, T):
        for r in range(nx):
            terms[k] = (r + 1, one, vm[t * w + r])
            terms[k + 1:k + 1 + w, 0] = r + 1
            terms[k + 1:k + 1 + w, 1] = sec[(t - 1) * nab + r * w:(t - 1) * nab + (r + 1) * w]
            terms[k + 1:k + 1 + w, 2] = vm[(t - 1) * w:t * w]
            k += 1 + w
    assert k == len(terms)
    return terms.reshape(-1), np.array(section[(T - 1) * nab:(T - 1) * nab + T * nx], dtype=np.float64)


def instance_stages(A, Bmat, h, sign_xp, sign_a, sign_b, sign_h, xvar):
    """the instance's own records as affine_stages_util stages, placed one behind the other: A (T-1, nx, nx) and Bmat (T-1, nx, nu) as
    matrices — stage t's parts point at A[t-1], Bmat[t-1] —, h (T, nx) -> (stages, nterms, nconsts)"""
    nx, nu, T = h.shape[1], Bmat.shape[2], h.shape[0]
    w = nx + nu
    xvar = np.asarray(xvar, dtype=np.int64)
    stages = []
    for t in range(T):
        parts = [{"mat": None, "xvar": xvar[t * w:t * w + nx], "sign": sign_xp}]
        if t:
            parts.append({"mat": A[t - 1], "xvar": xvar[(t - 1) * w:(t - 1) * w + nx], "sign": sign_a})
            if nu:
                parts.append({"mat": Bmat[t - 1], "xvar": xvar[(t - 1) * w + nx:t * w], "sign": sign_b})
        stages.append({"rows": nx, "parts": parts, "vec": h[t] if sign_h else None, "vec_sign": sign_h, "term_offset": 0, "const_offset": 0})
    nterms, nconsts = U.place(stages)
    return stages, nterms, nconsts


def matrices(At_i, Bt_i):
    """one instance's memory images [T-1, cols, nx] as matrices [T-1, nx, cols]"""
    return np.ascontiguousarray(At_i.transpose(0, 2, 1)), np.ascontiguousarray(Bt_i.transpose(0, 2, 1))
