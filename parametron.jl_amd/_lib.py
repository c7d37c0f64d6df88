"""ctypes binding of libparametron_hip.so (the C ABI declared in include/parametron_hip.h).

This is the product path: there is NO CPU fallback.  If the shared library is missing or no
MI355X is visible, the calls raise — loudly.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PMT_LIB_PATH") or os.path.join(HERE, "lib", "libparametron_hip.so")   # override: A/B builds of the library

# Julia isbits layouts as numpy structured dtypes
LT = np.dtype([("coeff", "<f8"), ("var", "<i8")])
QT = np.dtype([("coeff", "<f8"), ("row", "<i8"), ("col", "<i8")])
VAT = np.dtype([("out", "<i8"), ("coeff", "<f8"), ("var", "<i8")])

PMT_OK, PMT_DIMENSION_MISMATCH, PMT_INVALID_ARGUMENT, PMT_HIP_ERROR, PMT_STATE_ERROR, PMT_OUT_OF_MEMORY = range(6)
PMT_LSQ_BLOCK, PMT_LSQ_DIAG, PMT_LSQ_LINEAR, PMT_LSQ_CONSTANT = 1, 2, 3, 4
PMT_LSQ_MAX_TERMS, PMT_LSQ_MAX_BLOCKS, PMT_LSQ_MAX_RUNS = 32, 8, 64
PMT_QUAD_MAX_GROUPS = 8
PMT_SPARSE_SUM_WG_TERMS = 256                                    # output terms per workgroup of pmt_sparse_gram_sum_f64
STACK_COLUMN = np.dtype([("src", "<u8"), ("sign", "<i8")])       # pmt_stack_column


class LsqTerm(C.Structure):
    """pmt_lsq_term: one term of the weighted sum pmt_quad_gram_sum_f64 combines (pointers are device addresses, or None)."""
    _fields_ = [("kind", C.c_int32), ("sign", C.c_int32), ("scale", C.c_double), ("weight", C.c_void_p), ("values", C.c_void_p),
                ("lin", C.c_void_p), ("constant", C.c_void_p), ("vec", C.c_void_p)]


def lsq_terms(terms):
    """host array of pmt_lsq_term from dicts {kind, sign, scale, weight, values, lin, constant, vec} (missing fields: 0 / None)"""
    arr = (LsqTerm * max(len(terms), 1))()
    for i, t in enumerate(terms):
        for k, v in t.items():
            setattr(arr[i], k, v)
        if "scale" not in t:
            arr[i].scale = 1.0
    return arr


class SparseLsqTerm(C.Structure):
    """pmt_sparse_lsq_term: one term of the weighted sum pmt_sparse_gram_sum_f64 combines (pointers are device addresses, or None)."""
    _fields_ = [("kind", C.c_int32), ("sign", C.c_int32), ("scale", C.c_double), ("weight", C.c_void_p), ("quad", C.c_void_p),
                ("lin", C.c_void_p), ("constant", C.c_void_p), ("quad_at", C.c_void_p), ("lin_at", C.c_void_p), ("vec", C.c_void_p),
                ("pos", C.c_void_p), ("nvec", C.c_int64)]


def sparse_lsq_terms(terms):
    """host array of pmt_sparse_lsq_term from dicts of its fields (missing fields: 0 / None, scale 1.0)"""
    arr = (SparseLsqTerm * max(len(terms), 1))()
    for i, t in enumerate(terms):
        for k, v in t.items():
            setattr(arr[i], k, v)
        if "scale" not in t:
            arr[i].scale = 1.0
    return arr


PMT_QUAD_STAGES_MAX_N = 256


class QuadStage(C.Structure):
    """pmt_quad_stage: one stage of pmt_quad_stages_f64 (pointers are device addresses; vec None with sign 0)."""
    _fields_ = [("Q", C.c_void_p), ("ldq", C.c_int64), ("xvar", C.c_void_p), ("vec", C.c_void_p), ("n", C.c_int32), ("sign", C.c_int32),
                ("quad_at", C.c_int64), ("lin_at", C.c_int64)]


def quad_stages(stages):
    """host array of pmt_quad_stage from dicts of its fields (missing fields: 0 / None)"""
    arr = (QuadStage * max(len(stages), 1))()
    for i, t in enumerate(stages):
        for k, v in t.items():
            setattr(arr[i], k, v)
    return arr


PMT_QUAD_STAGES_MAX_CONSTS = 32


class QuadStageTerms(C.Structure):
    """pmt_quad_stage_terms: the weight and the linear term of one stage of pmt_quad_stages_terms_f64 (device addresses, or None)."""
    _fields_ = [("scale", C.c_double), ("weight", C.c_void_p), ("lin_scale", C.c_double), ("lin_weight", C.c_void_p), ("lin_vec", C.c_void_p)]


class QuadStageConst(C.Structure):
    """pmt_quad_stage_const: one scalar constant beside the stages of pmt_quad_stages_terms_f64 (device addresses, or None)."""
    _fields_ = [("scale", C.c_double), ("weight", C.c_void_p), ("value", C.c_void_p)]


class QuadStageDiag(C.Structure):
    """pmt_quad_stage_diag: the diagonal term riding on stage t of pmt_quad_stages_diag_f64 (device addresses, or None; present 0: none)."""
    _fields_ = [("scale", C.c_double), ("weight", C.c_void_p), ("vec", C.c_void_p), ("sign", C.c_int32), ("present", C.c_int32)]


assert C.sizeof(QuadStageTerms) == 40 and C.sizeof(QuadStageConst) == 24 and C.sizeof(QuadStageDiag) == 32


def _scaled_struct_array(cls, rows, scales):
    arr = (cls * max(len(rows), 1))()
    for i, t in enumerate(rows):
        for k in scales:
            setattr(arr[i], k, 1.0)
        for k, v in t.items():
            setattr(arr[i], k, v)
    return arr


def quad_stage_terms(terms):
    """host array of pmt_quad_stage_terms from dicts of its fields (missing fields: scale / lin_scale 1.0, pointers None)"""
    return _scaled_struct_array(QuadStageTerms, terms, ("scale", "lin_scale"))


def quad_stage_consts(consts):
    """host array of pmt_quad_stage_const from dicts of its fields (missing fields: scale 1.0, pointers None)"""
    return _scaled_struct_array(QuadStageConst, consts, ("scale",))


def quad_stage_diags(diags):
    """host array of pmt_quad_stage_diag from dicts of its fields, an empty dict for a stage without a rider (missing fields: scale 1.0,
    pointers None, sign 0; present 1 unless the dict is empty or says otherwise)"""
    return _scaled_struct_array(QuadStageDiag, [dict({"present": 1}, **t) if t else {} for t in diags], ("scale",))


PMT_AFFINE_STAGES_MAX_PARTS = 8


class AffinePart(C.Structure):
    """pmt_affine_part: one leaf with terms of a record of pmt_affine_stages_f64 (device addresses; mat None: a Variable vector, cols 1)."""
    _fields_ = [("mat", C.c_void_p), ("ld", C.c_int64), ("xvar", C.c_void_p), ("cols", C.c_int32), ("sign", C.c_int32)]


class AffineStage(C.Structure):
    """pmt_affine_stage: one record of pmt_affine_stages_f64 (vec a device address, or None with vec_sign 0)."""
    _fields_ = [("vec", C.c_void_p), ("term_offset", C.c_int64), ("const_offset", C.c_int64), ("row_len", C.c_int64), ("rows", C.c_int32),
                ("first_part", C.c_int32), ("nparts", C.c_int32), ("vec_sign", C.c_int32)]


def _struct_array(cls, rows):
    arr = (cls * max(len(rows), 1))()
    for i, t in enumerate(rows):
        for k, v in t.items():
            setattr(arr[i], k, v)
    return arr


def affine_parts(parts):
    """host array of pmt_affine_part from dicts of its fields (missing fields: 0 / None)"""
    return _struct_array(AffinePart, parts)


def affine_stages(stages):
    """host array of pmt_affine_stage from dicts of its fields (missing fields: 0 / None)"""
    return _struct_array(AffineStage, stages)


class BatchHorizonTerms(C.Structure):
    """pmt_batch_horizon_terms: the inputs of pmt_batch_horizon_terms_coeffs_f64 (device addresses, instance-major; None: P no terminal stage,
    a weight array every weight 1.0, a linear array no linear term, a reference only where its sign is 0)."""
    _fields_ = [(k, C.c_void_p) for k in ("Q", "R", "P", "r", "v", "rN", "wx", "wu", "wN", "gx", "gu", "gN", "C", "d")] + \
               [(k, C.c_int32) for k in ("sign_r", "sign_v", "sign_rN", "sign_d")]


assert C.sizeof(BatchHorizonTerms) == 128


def batch_horizon_terms(**fields):
    """one pmt_batch_horizon_terms from its fields (missing fields: None / 0)"""
    return _struct_array(BatchHorizonTerms, [fields])[0]


def stack_table(srcs, signs):
    """host image of the pmt_stack_column table of pmt_affine_stack_columns_f64: column c is signs[c] * (the column at device address
    srcs[c]).  The entry point reads the table on the device only, so the signs are checked here."""
    srcs = np.asarray(srcs, dtype=np.uint64).reshape(-1)
    signs = np.asarray(signs, dtype=np.int64).reshape(-1)
    if srcs.shape != signs.shape:
        raise DimensionMismatch("stack_table: %d sources, %d signs" % (len(srcs), len(signs)))
    if not np.all((signs == 1) | (signs == -1)):
        raise ArgumentError("stack_table: every sign must be +1 or -1")
    if np.any(srcs == 0):
        raise ArgumentError("stack_table: null column source")
    t = np.empty(len(srcs), dtype=STACK_COLUMN)
    t["src"], t["sign"] = srcs, signs
    return t


def column_runs(positions):
    """the number of runs of consecutive positions in a strictly increasing list (pmt_quad_gram_sum_sub_f64 holds PMT_LSQ_MAX_RUNS)"""
    p = np.asarray(positions, dtype=np.int64)
    return int(len(p) and 1 + np.count_nonzero(np.diff(p) != 1))


class GroupsLayout:
    """Where the canonical functions of groups over pairwise disjoint, strictly increasing variable sets (`sets`, in group order) stand in
    the function over their sorted union z (include/parametron_hip.h, pmt_quad_groups_gather_f64).  Offsets in terms; the arena holds the
    groups' functions one behind the other in group order.
      z, owner              the union and the group of each of its variables
      ordered               every group's variables are consecutive in z: its function is one slice of the destination
      dst_quad, dst_lin     per group, the slice's first term (meaningful when ordered)
      src_quad, src_lin     per group, its first term in the arena
      row_src, row_dst      the gather's tables in 8-byte words (row_dst: len(z) + 1 entries);  lin_src: per variable of z, its arena term
    `diagonal` (one flag per set, or None: no set): a flagged set's function holds its n diagonal terms only (an identity stage of
    pmt_quad_stages_diag_f64) — n rows of length 1 instead of the triangle's rows of length n .. 1."""

    def __init__(self, sets, diagonal=None):
        sets = [np.asarray(s, dtype=np.int64).reshape(-1) for s in sets]
        n = np.array([len(s) for s in sets], dtype=np.int64)
        diag = np.zeros(len(sets), dtype=bool) if diagonal is None else np.asarray(diagonal, dtype=bool).reshape(-1)
        if len(diag) != len(sets):
            raise ArgumentError("groups_layout: one diagonal flag per group")
        if len(sets) < 1 or np.any(n < 1) or any(np.any(np.diff(s) <= 0) for s in sets):
            raise ArgumentError("groups_layout: every group needs a non-empty, strictly increasing variable set")
        z = np.concatenate(sets)
        order = np.argsort(z, kind="stable")
        self.z = z[order]
        if np.any(np.diff(self.z) == 0):
            raise ArgumentError("groups_layout: the groups' variable sets overlap")
        self.owner = owner = np.repeat(np.arange(len(sets), dtype=np.int64), n)[order]
        local = np.concatenate([np.arange(k, dtype=np.int64) for k in n])[order]          # the variable's position in its group
        self.src_quad = np.concatenate([[0], np.cumsum(np.where(diag, n, n * (n + 1) // 2))[:-1]]).astype(np.int64)
        self.src_lin = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
        ng, dg = n[owner], diag[owner]
        self.row_dst = 3 * np.concatenate([[0], np.cumsum(np.where(dg, 1, ng - local))]).astype(np.int64)
        self.row_src = 3 * (self.src_quad[owner] + np.where(dg, local, local * ng - local * (local - 1) // 2))
        self.lin_src = self.src_lin[owner] + local
        self.nterms, self.nlin = int(self.row_dst[-1]) // 3, len(self.z)
        self.ordered = int(np.count_nonzero(np.diff(owner))) == len(sets) - 1
        first = np.full(len(sets), len(owner), dtype=np.int64)                             # every group's first variable in z: one pass
        np.minimum.at(first, owner, np.arange(len(owner), dtype=np.int64))
        self.dst_quad, self.dst_lin = self.row_dst[first] // 3, first


class DimensionMismatch(Exception):
    """Julia's DimensionMismatch (src/functions.jl:780-781 and the other @boundscheck sites)."""


class ArgumentError(ValueError):
    """Julia's ArgumentError (src/lazyexpression.jl:175,185; src/model.jl:226,243,246)."""


class ErrorException(RuntimeError):
    """Julia's ErrorException — error(...) (src/model.jl:50,61,69,139)."""


class HipError(RuntimeError):
    pass


_vp, _i64, _f64, _ci, _u64, _sz = C.c_void_p, C.c_int64, C.c_double, C.c_int, C.c_uint64, C.c_size_t

# name -> (restype, argtypes); every symbol include/parametron_hip.h declares
SIGNATURES = {
    "pmt_last_error": (C.c_char_p, []),
    "pmt_version": (_ci, []),
    "pmt_device_count": (_ci, []),
    "pmt_affine_assemble_f64": (_ci, [_vp, _i64, _i64, _i64, _vp, _vp, _ci, _vp, _vp, _vp]),
    "pmt_affine_pack_vector_f64": (_ci, [_vp, _i64, _i64, _i64, _vp, _vp, _ci, _vp, _i64, _vp, _vp, _vp]),
    "pmt_affine_pack_vector_background_f64": (_ci, [_vp, _i64, _i64, _i64, _vp, _vp, _ci, _vp, _i64, _vp, _vp, _vp]),
    "pmt_vars_addsub_f64": (_ci, [_vp, _i64, _vp, _ci, _vp, _i64, _vp, _vp, _vp, _vp]),
    "pmt_affvec_combine_f64": (_ci, [_i64, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _ci, _vp, _vp, _i64, _vp, _vp]),
    "pmt_affvec_scale_f64": (_ci, [_i64, _i64, _vp, _vp, _vp, _f64, _vp, _vp, _vp]),
    "pmt_scale_vars_f64": (_ci, [_vp, _i64, _vp, _f64, _vp, _vp]),
    "pmt_scale_numbers_f64": (_ci, [_vp, _i64, _vp, _f64, _vp, _vp]),
    "pmt_transpose_f64": (_ci, [_vp, _i64, _i64, _i64, _vp, _i64, _vp]),
    "pmt_quad_combine_f64": (_ci, [_vp, _i64, _vp, _i64, _ci, _vp, _vp]),
    "pmt_quad_scale_f64": (_ci, [_vp, _i64, _vp, _f64, _vp, _vp]),
    "pmt_copy_bytes": (_ci, [_vp, _vp, _sz, _vp]),
    "pmt_matvecmul_affs_f64": (_ci, [_vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    "pmt_vecdot_numbers_vars_f64": (_ci, [_vp, _vp, _i64, _vp, _vp, _vp]),
    "pmt_vecdot_numbers_affs_f64": (_ci, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    "pmt_quad_expand_f64": (_ci, [_i64, _vp, _i64, _vp, _vp, _i64, _vp, _ci, _vp, _vp, _vp, _vp, _vp]),
    "pmt_quad_gram_workspace_bytes": (_sz, [_i64, _i64]),
    "pmt_quad_gram_constant_order": (_ci, [_i64, _i64, C.POINTER(_ci), C.POINTER(_ci), C.POINTER(_ci)]),
    "pmt_quad_gram_mid_defers": (_ci, [_i64, _i64, C.POINTER(_ci), C.POINTER(_ci)]),
    "pmt_quad_gram_mid_strips": (_ci, [_i64, _i64, C.POINTER(_ci), C.POINTER(_ci)]),
    "pmt_quad_gram_f64": (_ci, [_vp, _i64, _i64, _i64, _vp, _vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pmt_quad_gram_csc_f64": (_ci, [_vp, _i64, _i64, _i64, _vp, _vp, _ci, _vp, _f64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pmt_quad_gram_csc_deliver_f64": (_ci, [_vp, _i64, _i64, _i64, _vp, _vp, _ci, _vp, _f64, _vp, _vp, _ci, _vp, _vp, _vp, _vp]),
    "pmt_quad_gram_deliver_f64": (_ci, [_vp, _i64, _i64, _i64, _vp, _vp, _ci, _ci, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _vp]),
    "pmt_quad_gram_sum_f64": (_ci, [_i64, _vp, _ci, _vp, _vp, _vp, _vp]),
    "pmt_quad_gram_sum_sub_f64": (_ci, [_i64, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pmt_affine_stack_columns_f64": (_ci, [_vp, _i64, _i64, _vp, _i64, _vp]),
    "pmt_quad_form_f64": (_ci, [_vp, _i64, _i64, _vp, _ci, _vp, _f64, _vp, _vp, _vp, _vp, _vp]),
    "pmt_quad_form_shift_workspace_bytes": (_i64, [_i64]),
    "pmt_quad_form_shift_f64": (_ci, [_vp, _i64, _i64, _vp, _vp, _ci, _ci, _vp, _f64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pmt_quad_groups_gather_f64": (_ci, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp]),
    "pmt_quad_groups_constant_f64": (_ci, [_vp, _ci, _vp, _vp]),
    "pmt_fetch_synchronize": (_ci, [_vp]),
    "pmt_set_host_delivery": (_ci, [_ci]),
    "pmt_get_host_delivery": (_ci, [_ci, C.POINTER(_ci), C.POINTER(_ci)]),
    "pmt_set_fault_injection": (_ci, [_ci]),
    "pmt_bilinear_f64": (_ci, [_vp, _i64, _i64, _i64, _vp, _vp, _ci, _vp, _vp, _vp]),
    "pmt_fill_uniform_matrix_f64": (_ci, [_vp, _i64, _i64, _i64, _u64, _f64, _vp]),
    "pmt_plan_upload_2d": (_ci, [_vp, _vp, _sz, _vp, _sz, _sz, _sz]),
    "pmt_plan_fetch_2d": (_ci, [_vp, _vp, _sz, _vp, _sz, _sz, _sz]),
    "pmt_vecdot_terms_f64": (_ci, [_i64, _vp, _vp, _vp, _vp, _ci, _vp, _vp, _vp]),
    "pmt_vecdot_affs_vars_f64": (_ci, [_i64, _vp, _i64, _vp, _vp, _ci, _vp, _vp, _vp, _vp]),
    "pmt_pack_scalar_affine_f64": (_ci, [_vp, _i64, _vp, _vp, _vp]),
    "pmt_pack_scalar_quadratic_f64": (_ci, [_vp, _i64, _vp, _vp, _vp]),
    "pmt_pack_vector_affine_f64": (_ci, [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _vp]),
    "pmt_canonical_order_affine": (_ci, [_i64, _vp, _vp, _vp, _vp, C.POINTER(_i64)]),
    "pmt_canonical_order_quadratic": (_ci, [_i64, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i64)]),
    "pmt_canonical_order_device": (_ci, [_vp, _i64, _ci, _vp, _vp, C.POINTER(_i64), _vp]),
    "pmt_canonical_init_terms": (_ci, [_vp, _ci, _vp, _vp, _i64, _vp, _vp]),
    "pmt_segment_sum_f64": (_ci, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp]),
    "pmt_prune_zero_workspace_bytes": (_sz, [_i64, _ci]),
    "pmt_prune_zero_f64": (_ci, [_vp, _i64, _ci, _f64, _vp, _vp, _vp, _sz, _vp]),
    "pmt_csc_order": (_ci, [_i64, _vp, _vp, _i64, _i64, _ci, _vp, _vp, _vp, _vp, C.POINTER(_i64)]),
    "pmt_csc_values_f64": (_ci, [_vp, _i64, _i64, _vp, _vp, _i64, _f64, _vp, _vp, _vp]),
    "pmt_qp_bounds_f64": (_ci, [_vp, _i64, _ci, _f64, _f64, _vp, _vp, _vp]),
    "pmt_csc_values_gather_f64": (_ci, [_vp, _i64, _vp, _i64, _f64, _vp, _vp, _vp]),
    "pmt_copy_2d_f64": (_ci, [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _vp]),
    "pmt_qp_bounds_rows_f64": (_ci, [_vp, _vp, _vp, _i64, _f64, _vp, _vp, _vp]),
    "pmt_sparse_rowmajor_order": (_ci, [_i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pmt_sparse_assemble_f64": (_ci, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "pmt_sparse_pack_vector_f64": (_ci, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp]),
    "pmt_sparse_slab_ptr": (_ci, [_i64, _i64, _ci, _vp, _vp, _vp]),
    "pmt_sparse_pack_vector_slabs_f64": (_ci, [_vp, _vp, _vp, _vp, _i64, _ci, _vp, _i64, _vp, _vp]),
    "pmt_sparse_assemble_slabs_f64": (_ci, [_vp, _vp, _vp, _vp, _i64, _ci, _vp, _vp]),
    "pmt_sparse_pack_vector_slabs_u32_f64": (_ci, [_vp, _vp, _vp, _vp, _i64, _ci, _vp, _i64, _vp, _vp]),
    "pmt_sparse_assemble_slabs_u32_f64": (_ci, [_vp, _vp, _vp, _vp, _i64, _ci, _vp, _vp]),
    "pmt_sparse_blocks_width": (_ci, [_i64, _i64, _vp, _vp, _vp]),
    "pmt_sparse_blocks_build": (_ci, [_i64, _i64, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp, _vp]),
    "pmt_sparse_pack_vector_blocks_f64": (_ci, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _ci, _vp, _i64, _vp, _ci, _vp, _vp, _vp]),
    "pmt_sparse_assemble_blocks_f64": (_ci, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _ci, _vp, _ci, _vp, _vp, _vp]),
    "pmt_sparse_gram_count": (_ci, [_i64, _i64, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "pmt_sparse_gram_order": (_ci, [_i64, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i64)]),
    "pmt_sparse_gram_runs": (_ci, [_vp, _i64, _i64, _vp, C.POINTER(_i64), _vp, C.POINTER(_i64)]),
    "pmt_sparse_gram_f64": (_ci, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _ci,
                                  _ci, _vp, _vp, _vp, _vp, _vp]),
    "pmt_sparse_gram_sum_merge": (_ci, [_i64, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64), _vp, _vp, _vp, _vp,
                                        _vp, _vp]),
    "pmt_sparse_gram_sum_f64": (_ci, [_i64, _vp, _ci, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pmt_sparse_form_count": (_ci, [_i64, _vp, _vp, C.POINTER(_i64)]),
    "pmt_sparse_form_order": (_ci, [_i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "pmt_sparse_form_f64": (_ci, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _ci, _vp, _vp, _vp, _vp]),
    "pmt_batch_lsq_slab_doubles":(_i64, [_i64, _i64]),
    "pmt_batch_lsq_coeffs_f64": (_ci, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _ci, _ci, _vp, _i64, _vp]),
    "pmt_batch_expand_f64": (_ci, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pmt_batch_form_coeffs_f64": (_ci, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _ci, _ci, _vp, _i64, _vp]),
    "pmt_batch_horizon_slab_doubles": (_i64, [_i64, _i64, _i64, _i64]),
    "pmt_batch_horizon_coeffs_f64": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _ci, _ci, _ci, _vp, _i64, _vp]),
    "pmt_batch_horizon_expand_f64": (_ci, [_vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pmt_batch_horizon_terms_slab_doubles": (_i64, [_i64, _i64, _i64, _i64, _i64]),
    "pmt_batch_horizon_terms_coeffs_f64": (_ci, [_vp, _i64, _i64, _i64, _i64, _i64, _vp, _i64, _vp]),
    "pmt_batch_horizon_terms_expand_f64": (_ci, [_vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pmt_batch_horizon_dynamics_doubles": (_i64, [_i64, _i64, _i64]),
    "pmt_batch_horizon_dynamics_f64": (_ci, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _ci, _ci, _ci, _vp, _i64, _vp]),
    "pmt_batch_horizon_dynamics_expand_f64": (_ci, [_vp, _i64, _i64, _i64, _ci, _vp, _vp, _vp, _vp, _vp]),
    "pmt_batch_horizon_dynamics_tv_doubles": (_i64, [_i64, _i64, _i64]),
    "pmt_batch_horizon_dynamics_tv_f64": (_ci, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _ci, _ci, _ci, _vp, _i64, _vp]),
    "pmt_batch_horizon_dynamics_tv_expand_f64": (_ci, [_vp, _i64, _i64, _i64, _ci, _vp, _vp, _vp, _vp, _vp]),
    "pmt_batch_horizon_tv_slab_doubles": (_i64, [_i64, _i64, _i64, _i64, _i64]),
    "pmt_batch_horizon_tv_coeffs_f64": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _ci, _ci, _ci, _vp, _i64, _vp]),
    "pmt_batch_horizon_tv_expand_f64": (_ci, [_vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pmt_quad_stages_check": (_ci, [_vp, _i64, _i64, _i64]),
    "pmt_quad_stages_f64": (_ci, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pmt_quad_stages_terms_check": (_ci, [_vp, _vp, _i64, _vp, _i64, _i64, _i64]),
    "pmt_quad_stages_terms_f64": (_ci, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pmt_quad_stages_diag_check": (_ci, [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64]),
    "pmt_quad_stages_diag_f64": (_ci, [_vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pmt_quad_stages_csc_check": (_ci, [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64]),
    "pmt_quad_stages_csc_f64": (_ci, [_vp, _vp, _vp, _i64, _vp, _i64, _vp, _f64, _vp, _vp, _vp, _vp, _vp]),
    "pmt_affine_stages_check": (_ci, [_vp, _i64, _vp, _i64, _i64, _i64]),
    "pmt_affine_stages_f64": (_ci, [_vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "pmt_comm_unique_id": (_ci, [_vp]),
    "pmt_comm_init_rank": (_ci, [_ci, _ci, _vp, _ci, C.POINTER(_vp)]),
    "pmt_comm_destroy": (_ci, [_vp]),
    "pmt_comm_rccl_calls": (_i64, [_vp]),
    "pmt_batch_num_chunks": (_i64, [_i64, _i64]),
    "pmt_batch_chunk_range": (_ci, [_i64, _i64, _i64, C.POINTER(_i64), C.POINTER(_i64)]),
    "pmt_batch_gathered_offset": (_i64, [_ci, _i64, _i64, _i64]),
    "pmt_batch_shard": (_ci, [_i64, _ci, _ci, C.POINTER(_i64), C.POINTER(_i64)]),
    "pmt_batch_allgather_f64": (_ci, [_vp, _vp, _vp, _i64, _i64, _i64, _vp]),
    "pmt_batch_step_f64": (_ci, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _ci, _ci, _vp, _vp, _i64, _i64, _vp]),
    "pmt_consts_f64": (_ci, [_vp, _i64, _ci, _vp, _vp]),
    "pmt_fill_uniform_f64": (_ci, [_vp, _i64, _u64, _f64, _vp]),
    "pmt_fill_uniform_offset_f64": (_ci, [_vp, _i64, _u64, _u64, _f64, _vp]),
    "pmt_profile_enable": (_ci, [_ci]),
    "pmt_profile_filter": (_ci, [C.c_char_p]),
    "pmt_profile_kernel_stamps": (_ci, [_vp, _i64]),
    "pmt_device_clock_khz": (_ci, [_ci, C.POINTER(_ci)]),
    "pmt_profile_report": (_i64, [C.c_char_p, _sz]),
    "pmt_plan_create": (_ci, [_ci, _vp, C.POINTER(_vp)]),
    "pmt_plan_destroy": (_ci, [_vp]),
    "pmt_plan_stream": (_vp, [_vp]),
    "pmt_plan_alloc": (_ci, [_vp, _sz, C.POINTER(_vp)]),
    "pmt_plan_bytes_allocated": (_sz, [_vp]),
    "pmt_host_alloc": (_ci, [_sz, C.POINTER(_vp)]),
    "pmt_host_free": (_ci, [_vp]),
    "pmt_plan_upload": (_ci, [_vp, _vp, _vp, _sz]),
    "pmt_plan_fetch": (_ci, [_vp, _vp, _vp, _sz]),
    "pmt_plan_zero": (_ci, [_vp, _vp, _sz]),
    "pmt_plan_synchronize": (_ci, [_vp]),
    "pmt_plan_check": (_ci, [_vp]),
    "pmt_model_create": (_ci, [_vp, C.POINTER(_vp)]),
    "pmt_model_destroy": (_ci, [_vp]),
    "pmt_model_add_mailbox": (_ci, [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _i64, C.POINTER(_ci)]),
    "pmt_model_add_seed": (_ci, [_vp, C.POINTER(C.c_uint64), C.c_uint64, C.c_uint64, C.POINTER(_ci)]),
    "pmt_model_set_host": (_ci, [_vp, _ci, _vp]),
    "pmt_model_add_constant": (_ci, [_vp, _vp, _vp]),
    "pmt_model_add_fetch": (_ci, [_vp, _vp, _vp, C.c_size_t]),
    "pmt_model_num_slots": (_ci, [_vp]),
    "pmt_model_update": (_ci, [_vp, _vp, _ci, _ci]),
    "pmt_model_wait": (_ci, [_vp]),
    "pmt_plan_record_fetch": (_ci, [_vp, _vp, _vp, _sz]),
    "pmt_plan_record_fetch_2d": (_ci, [_vp, _vp, _sz, _vp, _sz, _sz, _sz]),
    "pmt_host_copy_2d": (_ci, [_vp, _sz, _vp, _sz, _sz, _sz, _ci]),
    "pmt_plan_fetch_synchronize": (_ci, [_vp]),
    "pmt_plan_stage_upload": (_ci, [_vp, _vp, _vp, _sz]),
    "pmt_plan_stage_upload_2d": (_ci, [_vp, _vp, _sz, _vp, _sz, _sz, _sz]),
    "pmt_plan_wait_staged": (_ci, [_vp]),
    "pmt_plan_commit_staged": (_ci, [_vp, _vp, _vp, _sz]),
    "pmt_plan_staging_consumed": (_ci, [_vp]),
    "pmt_plan_staged_synchronize": (_ci, [_vp]),
    "pmt_plan_stage_slot": (_ci, [_vp, _ci]),
    "pmt_plan_begin_record": (_ci, [_vp]),
    "pmt_plan_end_record": (_ci, [_vp]),
    "pmt_plan_commit_lane": (_ci, [_vp, _ci]),
    "pmt_plan_set_lane": (_ci, [_vp, _ci]),
    "pmt_plan_lane_stream": (_ci, [_vp, _ci, C.POINTER(_vp)]),
    "pmt_plan_recording_stream": (_vp, [_vp]),
    "pmt_plan_tape_length": (_i64, [_vp]),
    "pmt_plan_set_fusion": (_ci, [_vp, _ci]),
    "pmt_plan_fused": (_ci, [_vp, C.POINTER(_ci), C.POINTER(_ci), C.POINTER(_i64)]),
    "pmt_plan_riders": (_ci, [_vp, C.POINTER(_ci), C.POINTER(_i64)]),
    "pmt_plan_rider_check": (_ci, [_vp, _i64, _i64, C.POINTER(_ci), C.POINTER(_ci), C.POINTER(_i64)]),
    "pmt_plan_fused_phases": (_ci, [_vp]),
    "pmt_plan_fused_workgroups": (_ci, [_vp]),
    "pmt_fill_uniform_dyn_f64": (_ci, [_vp, _i64, _i64, _i64, C.POINTER(_u64), _f64, _vp]),
    "pmt_plan_update": (_ci, [_vp]),
    "pmt_plan_instantiate_graph": (_ci, [_vp]),
}

_lib = None


def load():
    """Load the HIP library; raises if it has not been built (python __graft_entry__.py / make -C csrc)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ErrorException(
                "libparametron_hip.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
        # PyTorch-ROCm bundles its own libamdhip64.so.7 (same SONAME as /opt/rocm's).  Whichever copy is loaded
        # first serves the whole process, and torch cannot initialise on top of the system copy ("No HIP GPUs are
        # available").  Hosts that use torch for device memory / streams / torch.distributed must therefore have
        # torch loaded BEFORE this library; a torch-free host (the Julia binding) uses /opt/rocm's runtime.
        if os.environ.get("PMT_NO_TORCH_PRELOAD") != "1":
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def require_gpu():
    n = load().pmt_device_count()
    if n <= 0:
        raise ErrorException("no MI355X / HIP device visible: the Parametron hot path has no CPU fallback")
    return n


def check(rc):
    if rc == PMT_OK:
        return
    msg = load().pmt_last_error().decode("utf-8", "replace")
    if rc == PMT_DIMENSION_MISMATCH:
        raise DimensionMismatch(msg)
    if rc == PMT_INVALID_ARGUMENT:
        raise ArgumentError(msg)
    if rc == PMT_STATE_ERROR:
        raise ErrorException(msg)
    if rc == PMT_OUT_OF_MEMORY:
        raise MemoryError(msg)
    raise HipError(msg)


def call(name, *args):
    """Call a status-returning entry point and raise the reference's exception type on failure."""
    check(getattr(load(), name)(*args))
