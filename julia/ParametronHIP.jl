# ParametronHIP.jl — the reference-side binding a Parametron.jl maintainer would add to route the update! hot path
# through libparametron_hip.so (include/parametron_hip.h): the thin ccall layer.  ParametronHIPBackend.jl (next to this file) builds the
# plan from a Parametron.Model and overrides update! / solve!.  The build image has no Julia (SURVEY.md §0.4): tests/test_cabi_exports.py
# checks every ccall against the header statically (symbol, argument count, argument type classes), tests/test_gpu_julia.py runs
# julia/example1_parity.jl when a julia binary exists on the GPU box; the same C ABI is exercised from Python by tests/.
#
# Usage sketch (README Example 1, README.md:23-57 of the reference):
#
#     using Parametron, ParametronHIP
#     model = Model(optimizer); x = [Variable(model) for _ = 1:n]
#     A = DeviceParameter(rand!, zeros(n, n), plan) ...          # host callback + H2D, or device_uniform!(…)
#     hip = HIPObjective(plan, A, x, b)                            # canonical residual ⋅ residual
#     ...
#     ParametronHIP.update!(plan); fetch!(moi_f.quadratic_terms, hip.quad)   # then MOI.set as in src/moi_interop.jl:134
module ParametronHIP

using SparseArrays

const lib = get(ENV, "PARAMETRON_HIP_LIB", "libparametron_hip.so")

# isbits layouts shared with the C structs (SURVEY.md Appendix C): LinearTerm{Float64} / MOI.ScalarAffineTerm{Float64} = 16 B,
# QuadraticTerm{Float64} / MOI.ScalarQuadraticTerm{Float64} = 24 B, MOI.VectorAffineTerm{Float64} = 24 B.
const DevPtr = Ptr{Cvoid}

struct HIPError <: Exception
    code::Cint
    msg::String
end

function check(code::Cint)
    code == 0 && return nothing
    msg = unsafe_string(ccall((:pmt_last_error, lib), Cstring, ()))
    code == 1 && throw(DimensionMismatch(msg))      # src/functions.jl:780-781 and the other @boundscheck sites
    code == 2 && throw(ArgumentError(msg))          # src/lazyexpression.jl:175,185
    code == 4 && error(msg)                         # src/model.jl:50,61,69
    throw(HIPError(code, msg))
end

# ---- plan: device buffers + tape (↔ dest = deepcopy(expr()) and the FunctionWrapper loop)
mutable struct Plan
    handle::Ptr{Cvoid}
    function Plan(device::Integer = 0)
        ref = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:pmt_plan_create, lib), Cint, (Cint, Ptr{Cvoid}, Ref{Ptr{Cvoid}}), device, C_NULL, ref))
        p = new(ref[])
        finalizer(p -> ccall((:pmt_plan_destroy, lib), Cint, (Ptr{Cvoid},), p.handle), p)
        p
    end
end

function alloc(plan::Plan, bytes::Integer)
    ref = Ref{DevPtr}(C_NULL)
    check(ccall((:pmt_plan_alloc, lib), Cint, (Ptr{Cvoid}, Csize_t, Ref{DevPtr}), plan.handle, bytes, ref))
    ref[]
end
upload!(plan::Plan, dst::DevPtr, src::Array) =
    check(ccall((:pmt_plan_upload, lib), Cint, (Ptr{Cvoid}, DevPtr, Ptr{Cvoid}, Csize_t), plan.handle, dst, src, sizeof(src)))
# `dst` may be moi_f.terms / moi_f.quadratic_terms after resize! — isbits element layouts match the device structs
fetch!(plan::Plan, dst::Array, src::DevPtr) =
    check(ccall((:pmt_plan_fetch, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, DevPtr, Csize_t), plan.handle, dst, src, sizeof(dst)))
synchronize(plan::Plan) = check(ccall((:pmt_plan_synchronize, lib), Cint, (Ptr{Cvoid},), plan.handle))
"the plan's device-side error state behind a wait the caller made by other means (a timed-out grid barrier of a fused run throws here)"
check_plan(plan::Plan) = check(ccall((:pmt_plan_check, lib), Cint, (Ptr{Cvoid},), plan.handle))
recording_stream(plan::Plan) = ccall((:pmt_plan_recording_stream, lib), Ptr{Cvoid}, (Ptr{Cvoid},), plan.handle)
begin_record!(plan::Plan) = check(ccall((:pmt_plan_begin_record, lib), Cint, (Ptr{Cvoid},), plan.handle))
end_record!(plan::Plan) = check(ccall((:pmt_plan_end_record, lib), Cint, (Ptr{Cvoid},), plan.handle))
"small plans: runs of small tape entries replay as ONE launch (automatic); `fusion!(plan, false)` replays the tape as recorded"
fusion!(plan::Plan, on::Bool) = check(ccall((:pmt_plan_set_fusion, lib), Cint, (Ptr{Cvoid}, Cint), plan.handle, on ? 1 : 0))
"barrier-separated phases over all fused runs (independent nodes share a phase)"
fused_phases(plan::Plan) = Int(ccall((:pmt_plan_fused_phases, lib), Cint, (Ptr{Cvoid},), plan.handle))
fused_workgroups(plan::Plan) = Int(ccall((:pmt_plan_fused_workgroups, lib), Cint, (Ptr{Cvoid},), plan.handle))
"(fused runs, tape entries they replace, launches-or-entries per replay)"
function fused(plan::Plan)
    g = Ref{Cint}(0); n = Ref{Cint}(0); len = Ref{Int64}(0)
    check(ccall((:pmt_plan_fused, lib), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}, Ref{Int64}), plan.handle, g, n, len))
    Int(g[]), Int(n[]), len[]
end
"(constraint packs that ride in the plan's one-launch Gram nodes, their tiles)"
function riders(plan::Plan)
    n = Ref{Cint}(0); tiles = Ref{Int64}(0)
    check(ccall((:pmt_plan_riders, lib), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Int64}), plan.handle, n, tiles))
    Int(n[]), tiles[]
end
"while recording: lane 1 = the following calls only read Parameter values and are independent of the rest of the tape (side lane), 0 = back"
set_lane!(plan::Plan, lane::Integer) = check(ccall((:pmt_plan_set_lane, lib), Cint, (Ptr{Cvoid}, Cint), plan.handle, lane))
"One update!(model) worth of kernels (src/model.jl:132-143): replays the tape, no allocation."
update!(plan::Plan) = check(ccall((:pmt_plan_update, lib), Cint, (Ptr{Cvoid},), plan.handle))

# ---- builders (each replaces the Parametron.Functions method named in include/parametron_hip.h)

"matvecmul!(y, A, x) fused with vecadd!/vecsubtract!(dest, y, b)  — src/functions.jl:775-798, :751-764"
affine_assemble!(out_terms::DevPtr, out_consts::DevPtr, A::DevPtr, lda, rows, cols, xvar::DevPtr, b::DevPtr, sign, stream) =
    check(ccall((:pmt_affine_assemble_f64, lib), Cint,
                (DevPtr, Int64, Int64, Int64, DevPtr, DevPtr, Cint, DevPtr, DevPtr, Ptr{Cvoid}),
                A, lda, rows, cols, xvar, b, sign, out_terms, out_consts, stream))

"the same chain + update!(::MOI.VectorAffineFunction, fs, varmap) — src/moi_interop.jl:64-81"
affine_pack_vector!(out_terms::DevPtr, out_consts::DevPtr, A::DevPtr, lda, rows, cols, xvar::DevPtr, b::DevPtr, sign,
                    varmap::DevPtr, row_offset, stream) =
    check(ccall((:pmt_affine_pack_vector_f64, lib), Cint,
                (DevPtr, Int64, Int64, Int64, DevPtr, DevPtr, Cint, DevPtr, Int64, DevPtr, DevPtr, Ptr{Cvoid}),
                A, lda, rows, cols, xvar, b, sign, varmap, row_offset, out_terms, out_consts, stream))

"_vecdot!(dest::QuadraticFunction, x, y) literal expansion (+ MOI copy when moi != 0) — src/functions.jl:702-709, :548-576"
quad_expand!(out_quad, out_lin, out_const, rows, xt, nx, xc, yt, ny, yc, moi, varmap, stream) =
    check(ccall((:pmt_quad_expand_f64, lib), Cint,
                (Int64, DevPtr, Int64, DevPtr, DevPtr, Int64, DevPtr, Cint, DevPtr, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                rows, xt, nx, xc, yt, ny, yc, moi, varmap, out_quad, out_lin, out_const, stream))

"canonicalize!(residual ⋅ residual) + MOI copy on the f64 matrix cores — src/functions.jl:381-386, src/moi_interop.jl:45-62"
quad_gram!(out_quad, out_lin, out_const, A, lda, rows, cols, xvar, b, sign, moi, varmap, workspace, stream) =
    check(ccall((:pmt_quad_gram_f64, lib), Cint,
                (DevPtr, Int64, Int64, Int64, DevPtr, DevPtr, Cint, Cint, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                A, lda, rows, cols, xvar, b, sign, moi, varmap, out_quad, out_lin, out_const, workspace, stream))

"bilinearmul!(dest, Q, x', y) — src/functions.jl:840-858"
bilinear!(out_quad, Q, ldq, rows, cols, xvar, yvar, moi, varmap, stream) =
    check(ccall((:pmt_bilinear_f64, lib), Cint, (DevPtr, Int64, Int64, Int64, DevPtr, DevPtr, Cint, DevPtr, DevPtr, Ptr{Cvoid}),
                Q, ldq, rows, cols, xvar, yvar, moi, varmap, out_quad, stream))

"Matrix{Float64} -> padded device copy (leading dimension ldd >= rows; DESIGN.md §2): a pitched host-to-device copy"
upload_matrix!(plan::Plan, dst::DevPtr, ldd, A::Matrix{Float64}) =
    check(ccall((:pmt_plan_upload_2d, lib), Cint, (Ptr{Cvoid}, DevPtr, Csize_t, Ptr{Cvoid}, Csize_t, Csize_t, Csize_t),
                plan.handle, dst, 8 * ldd, A, 8 * size(A, 1), 8 * size(A, 1), size(A, 2)))

# ---- solver hand-off (DESIGN.md §8): OSQP-style CSC data built on the device, behind MOI.set

"the Gram node with P's CSC values written from the contraction's epilogue (out_quad may be C_NULL)"
quad_gram_csc!(out_P_values, out_quad, out_lin, out_const, A, lda, rows, cols, xvar, b, sign, varmap, alpha, workspace, stream) =
    check(ccall((:pmt_quad_gram_csc_f64, lib), Cint,
                (DevPtr, Int64, Int64, Int64, DevPtr, DevPtr, Cint, DevPtr, Cdouble, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                A, lda, rows, cols, xvar, b, sign, varmap, alpha, out_P_values, out_quad, out_lin, out_const, workspace, stream))

"pmt_lsq_term (include/parametron_hip.h): one term of a weighted least-squares sum; kind PMT_LSQ_BLOCK = 1, DIAG = 2, LINEAR = 3, CONSTANT = 4"
struct LsqTerm
    kind::Int32
    sign::Int32
    scale::Float64
    weight::DevPtr
    values::DevPtr
    lin::DevPtr
    constant::DevPtr
    vec::DevPtr
end

"weighted sum of least-squares blocks (the first one already in out_quad / out_lin / out_const) and simple terms, combined in place —
 add! / mul! of quadratic functions and canonicalize!, src/functions.jl:452-461, 578, 381-386; src/moi_interop.jl:45-62"
quad_gram_sum!(out_quad, out_lin, out_const, cols, terms::Vector{LsqTerm}, stream) =
    check(ccall((:pmt_quad_gram_sum_f64, lib), Cint, (Int64, Ptr{LsqTerm}, Cint, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                cols, terms, length(terms), out_quad, out_lin, out_const, stream))

"weighted least-squares sum whose diagonal / linear terms cover only the positions listed in term_cols[t] (host vectors, strictly
 increasing 0-based positions; `nothing` = every column) — the same combine as quad_gram_sum!, restricted to the listed columns"
function quad_gram_sum_sub!(out_quad, out_lin, out_const, cols, terms::Vector{LsqTerm}, term_cols::Vector{Union{Nothing,Vector{Int64}}}, stream)
    length(term_cols) == length(terms) || throw(DimensionMismatch("one column list (or nothing) per term"))
    ptrs = Ptr{Int64}[c === nothing ? Ptr{Int64}(C_NULL) : pointer(c) for c in term_cols]
    counts = Int64[c === nothing ? 0 : length(c) for c in term_cols]
    GC.@preserve term_cols check(ccall((:pmt_quad_gram_sum_sub_f64, lib), Cint,
                                       (Int64, Ptr{LsqTerm}, Cint, Ptr{Ptr{Int64}}, Ptr{Int64}, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                                       cols, terms, length(terms), ptrs, counts, out_quad, out_lin, out_const, stream))
end

"pmt_stack_column (include/parametron_hip.h): the device address of a column and its sign (+1 or -1)"
struct StackColumn
    src::DevPtr
    sign::Int64
end

"out[:, c] = table[c].sign * column table[c].src (rows of each; out's rows rows+1 .. ldo untouched) — the blocks of a residual over several
 Variable vectors as one matrix (vecadd!/vecsubtract! src/functions.jl:751-764, rules src/lazyexpression.jl:238-258); `table` on the device"
affine_stack_columns!(out, ldo, table, ncols, rows, stream) =
    check(ccall((:pmt_affine_stack_columns_f64, lib), Cint, (DevPtr, Int64, Int64, DevPtr, Int64, Ptr{Cvoid}),
                table, ncols, rows, out, ldo, stream))

"transpose(x) * Q * x as its canonical function (bilinearmul! src/functions.jl:840-858, canonicalize! :381-386, MOI copy src/moi_interop.jl:45-62):
 Q[j,k] + Q[k,j] on the row-major upper triangle, 2 Q[j,j] on the diagonal; out_quad or out_P_values may be C_NULL (not both), out_lin
 (zero coefficients) and out_const (0.0) are optional"
quad_form!(out_quad, out_P_values, out_lin, out_const, Q, ldq, n, xvar, moi, varmap, alpha, stream) =
    check(ccall((:pmt_quad_form_f64, lib), Cint,
                (DevPtr, Int64, Int64, DevPtr, Cint, DevPtr, Cdouble, DevPtr, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                Q, ldq, n, xvar, moi, varmap, alpha, out_quad, out_P_values, out_lin, out_const, stream))

"transpose(x ± v) * Q * (x ± v) as its canonical function (matvecmul! src/functions.jl:800-822, vecdot! :702-709 over :548-576, canonicalize!
 :381-386, MOI copy src/moi_interop.jl:45-62): quad_form!'s quadratic part, lin = (Q + Q')c and the constant c'Qc with c = 0.0 ± v, in the
 order include/parametron_hip.h fixes; `workspace`: quad_form_shift_workspace_bytes(n) device bytes, no zeroing"
quad_form_shift!(out_quad, out_P_values, out_lin, out_const, Q, ldq, n, xvar, v, sign, moi, varmap, alpha, workspace, stream) =
    check(ccall((:pmt_quad_form_shift_f64, lib), Cint,
                (DevPtr, Int64, Int64, DevPtr, DevPtr, Cint, Cint, DevPtr, Cdouble, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                Q, ldq, n, xvar, v, sign, moi, varmap, alpha, out_quad, out_P_values, out_lin, out_const, workspace, stream))
quad_form_shift_workspace_bytes(n) = ccall((:pmt_quad_form_shift_workspace_bytes, lib), Int64, (Int64,), n)

"rows of the groups' canonical functions (an arena, src_quad / src_lin) placed in the function over the sorted union of their disjoint
 variable sets: device tables row_src (nrows), row_dst (nrows + 1) in 8-byte words, lin_src (nlin) — include/parametron_hip.h"
quad_groups_gather!(out_quad, out_lin, src_quad, row_src, row_dst, nrows, nterms, src_lin, lin_src, nlin, stream) =
    check(ccall((:pmt_quad_groups_gather_f64, lib), Cint,
                (DevPtr, DevPtr, DevPtr, Int64, Int64, DevPtr, DevPtr, Int64, DevPtr, DevPtr, Ptr{Cvoid}),
                src_quad, row_src, row_dst, nrows, nterms, src_lin, lin_src, nlin, out_quad, out_lin, stream))

"out_const = ((c_1 + c_2) + ..) + c_G over the groups' constants (device doubles), queued behind their own constant steps"
quad_groups_constant!(out_const, group_consts, ngroups, stream) =
    check(ccall((:pmt_quad_groups_constant_f64, lib), Cint, (DevPtr, Cint, DevPtr, Ptr{Cvoid}), group_consts, ngroups, out_const, stream))

"pmt_quad_stage (include/parametron_hip.h): one stage transpose(x_t (+|-) v_t) * Q * (x_t (+|-) v_t) of pmt_quad_stages_f64 — device
 addresses (vec C_NULL with sign 0), n in 1 .. 256, and the stage's first quadratic / linear term in the outputs; 56 bytes, no padding"
struct QuadStage
    Q::DevPtr
    ldq::Int64
    xvar::DevPtr
    vec::DevPtr
    n::Int32
    sign::Int32
    quad_at::Int64
    lin_at::Int64
end
const QUAD_STAGES_MAX_N = 256

"host arithmetic over a host Vector{QuadStage}: pointers, signs, sizes, and slices inside [0, nterms) / [0, nlin) that do not overlap"
quad_stages_check(stages::Vector{QuadStage}, nterms, nlin) =
    check(ccall((:pmt_quad_stages_check, lib), Cint, (Ptr{QuadStage}, Int64, Int64, Int64), stages, length(stages), nterms, nlin))

"a horizon of T stage costs over pairwise disjoint Variable vectors as one canonical MOI function from one launch: `stages` is the DEVICE copy
 of a table quad_stages_check accepted (the kernel does not check it again); stage_consts: T device doubles"
quad_stages!(out_quad, out_lin, stage_consts, out_const, stages::DevPtr, T, varmap, stream) =
    check(ccall((:pmt_quad_stages_f64, lib), Cint, (DevPtr, Int64, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                stages, T, varmap, out_quad, out_lin, stage_consts, out_const, stream))

"pmt_quad_stage_terms (include/parametron_hip.h): what stands beside stage t of pmt_quad_stages_terms_f64 — the weight scale * (*weight)
 (weight C_NULL: scale alone) and the linear term dot(c_t, x_t) with its own weight (lin_vec C_NULL: none); 40 bytes, no padding"
struct QuadStageTerms
    scale::Float64
    weight::DevPtr
    lin_scale::Float64
    lin_weight::DevPtr
    lin_vec::DevPtr
end

"pmt_quad_stage_const (include/parametron_hip.h): one scalar constant scale * (*weight) * (*value) beside the stages (value C_NULL: 1.0);
 24 bytes"
struct QuadStageConst
    scale::Float64
    weight::DevPtr
    value::DevPtr
end

"quad_stages_check over the stages, and the two further host tables: one QuadStageTerms per stage, at most 32 constants"
quad_stages_terms_check(stages::Vector{QuadStage}, terms::Vector{QuadStageTerms}, consts::Vector{QuadStageConst}, nterms, nlin) =
    check(ccall((:pmt_quad_stages_terms_check, lib), Cint, (Ptr{QuadStage}, Ptr{QuadStageTerms}, Int64, Ptr{QuadStageConst}, Int64, Int64, Int64),
                stages, terms, length(stages), consts, length(consts), nterms, nlin))

"quad_stages! with a weight and a linear term per stage and scalar constants beside the stages: `stages`, `terms` (T entries) and `consts`
 (nconsts entries) are the DEVICE copies of tables quad_stages_terms_check accepted; the weights are read on the device at run time"
quad_stages_terms!(out_quad, out_lin, stage_consts, out_const, stages::DevPtr, terms::DevPtr, T, consts::DevPtr, nconsts, varmap, stream) =
    check(ccall((:pmt_quad_stages_terms_f64, lib), Cint,
                (DevPtr, DevPtr, Int64, DevPtr, Int64, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                stages, terms, T, consts, nconsts, varmap, out_quad, out_lin, stage_consts, out_const, stream))

"pmt_quad_stage_diag (include/parametron_hip.h): the diagonal term W_d*dot(x (+|-) v, x (+|-) v) riding on stage t of
 pmt_quad_stages_diag_f64 beside its form — W_d = scale * (*weight) (weight C_NULL: scale alone), vec C_NULL with sign 0: W_d*dot(x, x);
 present 1 | 0 (no rider: the other fields are not read); 32 bytes, no padding"
struct QuadStageDiag
    scale::Float64
    weight::DevPtr
    vec::DevPtr
    sign::Int32
    present::Int32
end

"quad_stages_terms_check with identity stages (a QuadStage with Q C_NULL: W_t*dot(x (+|-) v, x (+|-) v), n quadratic terms) and riders:
 `diags` one QuadStageDiag per stage, or nothing when no stage has a rider"
quad_stages_diag_check(stages::Vector{QuadStage}, terms::Vector{QuadStageTerms}, diags::Union{Vector{QuadStageDiag},Nothing},
                       consts::Vector{QuadStageConst}, nterms, nlin) =
    check(ccall((:pmt_quad_stages_diag_check, lib), Cint,
                (Ptr{QuadStage}, Ptr{QuadStageTerms}, Ptr{QuadStageDiag}, Int64, Ptr{QuadStageConst}, Int64, Int64, Int64),
                stages, terms, diags === nothing ? C_NULL : diags, length(stages), consts, length(consts), nterms, nlin))

"quad_stages_terms! with identity stages and riders: `stages`, `terms`, `diags` (T entries, or C_NULL: no rider) and `consts` are the DEVICE
 copies of tables quad_stages_diag_check accepted"
quad_stages_diag!(out_quad, out_lin, stage_consts, out_const, stages::DevPtr, terms::DevPtr, diags::DevPtr, T, consts::DevPtr, nconsts, varmap,
                  stream) =
    check(ccall((:pmt_quad_stages_diag_f64, lib), Cint,
                (DevPtr, DevPtr, DevPtr, Int64, DevPtr, Int64, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                stages, terms, diags, T, consts, nconsts, varmap, out_quad, out_lin, stage_consts, out_const, stream))

"quad_stages_diag_check for the tables of quad_stages_csc!: a stage's quad_at is its first double among the `nvalues` CSC values of P
 (n(n+1)/2 per form stage, n per identity stage)"
quad_stages_csc_check(stages::Vector{QuadStage}, terms::Vector{QuadStageTerms}, diags::Union{Vector{QuadStageDiag},Nothing},
                      consts::Vector{QuadStageConst}, nvalues, nlin) =
    check(ccall((:pmt_quad_stages_csc_check, lib), Cint,
                (Ptr{QuadStage}, Ptr{QuadStageTerms}, Ptr{QuadStageDiag}, Int64, Ptr{QuadStageConst}, Int64, Int64, Int64),
                stages, terms, diags === nothing ? C_NULL : diags, length(stages), consts, length(consts), nvalues, nlin))

"quad_stages_diag! for a device-resident solver: out_P_values[quad_at + k(k+1)/2 + j] = alpha * c(j,k), the CSC values of the block-diagonal
 upper-triangular P, instead of quadratic term structs; out_lin, stage_consts and out_const as quad_stages_diag! writes them (not scaled)"
quad_stages_csc!(out_P_values, out_lin, stage_consts, out_const, stages::DevPtr, terms::DevPtr, diags::DevPtr, T, consts::DevPtr, nconsts, varmap,
                 alpha, stream) =
    check(ccall((:pmt_quad_stages_csc_f64, lib), Cint,
                (DevPtr, DevPtr, DevPtr, Int64, DevPtr, Int64, DevPtr, Float64, DevPtr, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                stages, terms, diags, T, consts, nconsts, varmap, alpha, out_P_values, out_lin, stage_consts, out_const, stream))

"pmt_affine_part (include/parametron_hip.h): one leaf with terms of a record of pmt_affine_stages_f64 — a matrix (column-major, leading
 dimension ld) over `cols` model variables, or mat C_NULL for a Variable vector (cols 1); sign +1 | -1; 32 bytes, no padding"
struct AffinePart
    mat::DevPtr
    ld::Int64
    xvar::DevPtr
    cols::Int32
    sign::Int32
end

"pmt_affine_stage: one record — its number vector (C_NULL with vec_sign 0), its first term / constant in the outputs, the terms per row, its
 rows and its run of parts; 48 bytes, no padding"
struct AffineStage
    vec::DevPtr
    term_offset::Int64
    const_offset::Int64
    row_len::Int64
    rows::Int32
    first_part::Int32
    nparts::Int32
    vec_sign::Int32
end
const AFFINE_STAGES_MAX_PARTS = 8

"host arithmetic over host tables: pointers, signs, sizes, row_len = the sum of the parts' cols, slices that tile [0, nterms) / [0, nconsts)"
affine_stages_check(stages::Vector{AffineStage}, parts::Vector{AffinePart}, nterms, nconsts) =
    check(ccall((:pmt_affine_stages_check, lib), Cint, (Ptr{AffineStage}, Int64, Ptr{AffinePart}, Int64, Int64, Int64),
                stages, length(stages), parts, length(parts), nterms, nconsts))

"the MOI.VectorAffineFunction buffers of T affine records (a horizon's dynamics constraints) from one launch: `stages` and `parts` are the
 DEVICE copies of tables affine_stages_check accepted (the kernel does not check them again)"
affine_stages!(out_terms, out_consts, stages::DevPtr, T, parts::DevPtr, varmap, stream) =
    check(ccall((:pmt_affine_stages_f64, lib), Cint, (DevPtr, Int64, DevPtr, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                stages, T, parts, varmap, out_terms, out_consts, stream))

"structure of a solver matrix from 1-based (row, col) indices (host, once): perm, seg_ptr, colptr, rowval (0-based), nnz"
function csc_order(rows::Vector{Int64}, cols::Vector{Int64}, nrows, ncols; upper::Bool=false)
    n = length(rows)
    perm, seg = zeros(Int64, max(n, 1)), zeros(Int64, n + 1)
    colptr, rowval, nnz = zeros(Int64, ncols + 1), zeros(Int64, max(n, 1)), Ref{Int64}(0)
    check(ccall((:pmt_csc_order, lib), Cint,
                (Int64, Ptr{Int64}, Ptr{Int64}, Int64, Int64, Cint, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ref{Int64}),
                n, rows, cols, nrows, ncols, upper, perm, seg, colptr, rowval, nnz))
    perm[1:n], seg[1:nnz[] + 1], colptr, rowval[1:nnz[]]
end

"values of a solver matrix: dst[dst_index[s]] = alpha * sum of the MOI coefficients of run s (per re-evaluation)"
csc_values!(dst::DevPtr, src_coeff::DevPtr, stride, nnz_in, perm::DevPtr, seg::DevPtr, nnz_out, alpha, dst_index::DevPtr, stream) =
    check(ccall((:pmt_csc_values_f64, lib), Cint, (DevPtr, Int64, Int64, DevPtr, DevPtr, Int64, Cdouble, DevPtr, DevPtr, Ptr{Cvoid}),
                src_coeff, stride, nnz_in, perm, seg, nnz_out, alpha, dst_index, dst, stream))

"l, u of `f(x) in set` rows from the constants: kind 0 = Zeros/EqualTo, 1 = Nonnegatives/GreaterThan, 2 = Nonpositives/LessThan"
qp_bounds!(l::DevPtr, u::DevPtr, consts::DevPtr, rows, kind, value, infty, stream) =
    check(ccall((:pmt_qp_bounds_f64, lib), Cint, (DevPtr, Int64, Cint, Cdouble, Cdouble, DevPtr, DevPtr, Ptr{Cvoid}),
                consts, rows, kind, value, infty, l, u, stream))

# ---- sparse constraint matrix (SparseMatrixCSC with a fixed pattern; BASELINE config 5)

"row-major order of the structural non-zeros + per-row boundaries of `nslab` column slabs (host, once per pattern)"
function sparse_plan(C::SparseMatrixCSC{Float64,Int64}; nslab::Integer=8)
    m, n = size(C)
    nz = length(C.nzval)
    perm, trow, tcol, rowptr = zeros(Int64, max(nz, 1)), zeros(Int64, max(nz, 1)), zeros(Int64, max(nz, 1)), zeros(Int64, m + 1)
    check(ccall((:pmt_sparse_rowmajor_order, lib), Cint,
                (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
                m, n, C.colptr, C.rowval, perm, trow, tcol, rowptr))
    slab = zeros(Int64, max(m, 1) * (nslab + 1))
    check(ccall((:pmt_sparse_slab_ptr, lib), Cint, (Int64, Int64, Cint, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}), m, n, nslab, rowptr, tcol, slab))
    (perm = perm, term_col = tcol, row_ptr = rowptr, slab_ptr = slab)
end

"C*x (+|-) d for a sparse C written straight into MOI.VectorAffineTerms (XCD-aware scatter)"
sparse_pack_vector!(out_terms::DevPtr, nzval::DevPtr, perm::DevPtr, term_var::DevPtr, slab_ptr::DevPtr, rows, nslab, varmap::DevPtr,
                    row_offset, stream) =
    check(ccall((:pmt_sparse_pack_vector_slabs_f64, lib), Cint,
                (DevPtr, DevPtr, DevPtr, DevPtr, Int64, Cint, DevPtr, Int64, DevPtr, Ptr{Cvoid}),
                nzval, perm, term_var, slab_ptr, rows, nslab, varmap, row_offset, out_terms, stream))

"the same with UInt32 perm / variable streams (nnz and indices below 2^32: half the index bytes).  Fold the optimizer's index map into
`term_var` (term_var[t] = varmap[x[col]]) and pass `varmap = C_NULL` to drop the per-term map gather; refresh it after mapindices!."
sparse_pack_vector_u32!(out_terms::DevPtr, nzval::DevPtr, perm32::DevPtr, term_var32::DevPtr, slab_ptr::DevPtr, rows, nslab, varmap::DevPtr,
                        row_offset, stream) =
    check(ccall((:pmt_sparse_pack_vector_slabs_u32_f64, lib), Cint,
                (DevPtr, DevPtr, DevPtr, DevPtr, Int64, Cint, DevPtr, Int64, DevPtr, Ptr{Cvoid}),
                nzval, perm32, term_var32, slab_ptr, rows, nslab, varmap, row_offset, out_terms, stream))

"block form of the sparse node (CSC -> row-major through LDS, sparse.hip): band width `cw` (0: use the slab form), column descriptors, the
4-byte index word per term and the per-row band boundaries (host, once per pattern; `plan` from sparse_plan)"
function sparse_block_plan(C::SparseMatrixCSC{Float64,Int64}, plan)
    m, n = size(C)
    nz = length(C.nzval)
    cw = Ref{Cint}(0)
    check(ccall((:pmt_sparse_blocks_width, lib), Cint, (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ref{Cint}), m, n, C.colptr, C.rowval, cw))
    cw[] == 0 && return (cw = 0, desc = UInt64[], idx = UInt32[], band_ptr = Int64[])
    nrb, ncb = cld(m, 128), cld(n, Int(cw[]))
    desc, idx, band = zeros(UInt64, nrb * n), zeros(UInt32, nz), zeros(Int64, m * (ncb + 1))
    check(ccall((:pmt_sparse_blocks_build, lib), Cint,
                (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Cint, Ptr{UInt64}, Ptr{UInt32}, Ptr{Int64}),
                m, n, C.colptr, C.rowval, plan.perm, plan.term_col, plan.row_ptr, cw[], desc, idx, band))
    (cw = Int(cw[]), desc = desc, idx = idx, band_ptr = band)
end

"C*x (+|-) d for a sparse C written straight into MOI.VectorAffineTerms, block form: `col_var[c]` = x[c] (or varmap[x[c]] with `varmap = C_NULL`);
the constants 0 (+|-) d come out of the same launch (`d = C_NULL`, `sign = 0`: zeros; `out_consts = C_NULL`: not written)"
sparse_pack_vector_blocks!(out_terms::DevPtr, out_consts::DevPtr, nzval::DevPtr, desc::DevPtr, idx::DevPtr, band_ptr::DevPtr, col_var::DevPtr, rows, cols,
                           nnz, cw, varmap::DevPtr, row_offset, d::DevPtr, sign, stream) =
    check(ccall((:pmt_sparse_pack_vector_blocks_f64, lib), Cint,
                (DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, Int64, Int64, Int64, Cint, DevPtr, Int64, DevPtr, Cint, DevPtr, DevPtr, Ptr{Cvoid}),
                nzval, desc, idx, band_ptr, col_var, rows, cols, nnz, cw, varmap, row_offset, d, sign, out_terms, out_consts, stream))

"native LinearTerms of the same node, block form"
sparse_assemble_blocks!(out_terms::DevPtr, out_consts::DevPtr, nzval::DevPtr, desc::DevPtr, idx::DevPtr, band_ptr::DevPtr, col_var::DevPtr, rows, cols, nnz,
                        cw, d::DevPtr, sign, stream) =
    check(ccall((:pmt_sparse_assemble_blocks_f64, lib), Cint,
                (DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, Int64, Int64, Int64, Cint, DevPtr, Cint, DevPtr, DevPtr, Ptr{Cvoid}),
                nzval, desc, idx, band_ptr, col_var, rows, cols, nnz, cw, d, sign, out_terms, out_consts, stream))

"out[i] = 0.0 (+|-) d[i] (sign -1 / +1): the constants of C*x (+|-) d (src/functions.jl:751-764)"
consts!(out::DevPtr, d::DevPtr, n, sign, stream) =
    check(ccall((:pmt_consts_f64, lib), Cint, (DevPtr, Int64, Cint, DevPtr, Ptr{Cvoid}), d, n, sign, out, stream))

"symbolic phase of the sparse least-squares objective dot(C*x (+|-) d, C*x (+|-) d) (host, once per pattern): the pairs of columns sharing a
row sorted by (j, k), their product list (positions in nzval, rows ascending within a segment), the non-empty columns, and the cut of one
launch into workgroup runs of at most `cap` products (segments of 64 products or more apart, one wave each)"
function sparse_gram_plan(C::SparseMatrixCSC{Float64,Int64}; cap::Integer=2048)
    m, n = size(C)
    nq, nprod = Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:pmt_sparse_gram_count, lib), Cint, (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ref{Int64}, Ref{Int64}), m, n, C.colptr, C.rowval, nq, nprod))
    nprod[] < 2^31 || throw(ArgumentError("sparse dot(r, r): nprod = $(nprod[]) products, 2^31 or more: hold the matrix in a dense Parameter"))
    pj, pk, seg = zeros(UInt32, max(nq[], 1)), zeros(UInt32, max(nq[], 1)), zeros(Int64, nq[] + 1)
    prod, lin_col, nlin = zeros(UInt64, max(nprod[], 1)), zeros(UInt32, max(n, 1)), Ref{Int64}(0)
    check(ccall((:pmt_sparse_gram_order, lib), Cint,
                (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Int64, Int64, Ptr{UInt32}, Ptr{UInt32}, Ptr{Int64}, Ptr{Cvoid}, Ptr{UInt32}, Ref{Int64}),
                m, n, C.colptr, C.rowval, nq[], nprod[], pj, pk, seg, prod, lin_col, nlin))
    runs, nruns, long_seg, nlong = sparse_gram_runs(seg, nq[], cap)
    resize!(lin_col, nlin[])
    lin_seg = Int64[C.colptr[j + 1] - 1 for j in lin_col]        # the first entry of every non-empty column, 0-based; then nnz
    push!(lin_seg, length(C.nzval))
    lin_runs, nlin_runs, lin_long, nlin_long = sparse_gram_runs(lin_seg, nlin[], cap)
    (nq = nq[], nprod = nprod[], pair_j = pj, pair_k = pk, seg_ptr = seg, prod = prod, runs = runs, nruns = nruns, long_seg = long_seg,
     nlong = nlong, lin_seg = lin_seg, rowidx0 = UInt32.(C.rowval .- 1), lin_col = lin_col, nlin = nlin[], lin_runs = lin_runs,
     nlin_runs = nlin_runs, lin_long = lin_long, nlin_long = nlin_long)
end

"the cut of a segment table into workgroup runs of at most `cap` products and the long segments (64 products or more): count, then fill"
function sparse_gram_runs(seg::Vector{Int64}, nseg, cap)
    nruns, nlong = Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:pmt_sparse_gram_runs, lib), Cint, (Ptr{Int64}, Int64, Int64, Ptr{Int64}, Ref{Int64}, Ptr{Int64}, Ref{Int64}),
                seg, nseg, cap, C_NULL, nruns, C_NULL, nlong))
    runs, long_seg = zeros(Int64, 2 * max(nruns[], 1)), zeros(Int64, max(nlong[], 1))
    check(ccall((:pmt_sparse_gram_runs, lib), Cint, (Ptr{Int64}, Int64, Int64, Ptr{Int64}, Ref{Int64}, Ptr{Int64}, Ref{Int64}),
                seg, nseg, cap, runs, nruns, long_seg, nlong))
    runs, nruns[], long_seg, nlong[]
end

"the canonical MOI function of dot(r, r), r = C*x (+|-) d with a sparse C (csrc/sparse_gram.hip): the tables of sparse_gram_plan as device
copies; `d = C_NULL`, `sign = 0`: no d"
sparse_gram!(out_quad::DevPtr, out_lin::DevPtr, out_const::DevPtr, nzval::DevPtr, prod::DevPtr, seg_ptr::DevPtr, pair_j::DevPtr, pair_k::DevPtr, nq,
             runs::DevPtr, nruns, long_seg::DevPtr, nlong, lin_seg::DevPtr, rowidx0::DevPtr, lin_col::DevPtr, nlin, lin_runs::DevPtr, nlin_runs,
             lin_long::DevPtr, nlin_long, rows, xvar::DevPtr, d::DevPtr, sign, moi, varmap::DevPtr, stream) =
    check(ccall((:pmt_sparse_gram_f64, lib), Cint,
                (DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, Int64, DevPtr, Int64, DevPtr, Int64, DevPtr, DevPtr, DevPtr, Int64, DevPtr, Int64, DevPtr, Int64,
                 Int64, DevPtr, DevPtr, Cint, Cint, DevPtr, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                nzval, prod, seg_ptr, pair_j, pair_k, nq, runs, nruns, long_seg, nlong, lin_seg, rowidx0, lin_col, nlin, lin_runs, nlin_runs, lin_long,
                nlin_long, rows, xvar, d, sign, moi, varmap, out_quad, out_lin, out_const, stream))

"""
the symbolic merge of a weighted sum over sparse blocks (csrc/sparse_gram_sum.hip): `plans` are the blocks' sparse_gram_plan results in
block order, `kinds` / `has_vec` / `cols` describe the nterms terms in expression order (cols[t]: 0-based positions in x, or `nothing`
for all of x).  Returns the merged pairs and columns, the blocks' gather tables and the position tables of the terms with a list.
"""
function sparse_gram_sum_plan(n::Integer, plans, kinds::Vector{Int32}, has_vec::Vector{Int32}, cols)
    K, nt = length(plans), length(kinds)
    pj, pk, lc = [p.pair_j for p in plans], [p.pair_k for p in plans], [p.lin_col for p in plans]
    nqs, nls = Int64[p.nq for p in plans], Int64[p.nlin for p in plans]
    lists = [c === nothing ? nothing : Vector{Int64}(c) for c in cols]
    keep = [c === nothing ? nothing : (isempty(c) ? Int64[0] : c) for c in lists]
    ncols = Int64[c === nothing ? 0 : length(c) for c in lists]
    ptrs(v) = Ptr{Cvoid}[a === nothing ? C_NULL : Ptr{Cvoid}(pointer(a)) for a in v]
    nq, nlin = Ref{Int64}(0), Ref{Int64}(0)
    arg(a) = a === nothing ? C_NULL : a
    tabs(v) = v === nothing ? C_NULL : ptrs(v)
    merge(opj, opk, olc, qat, lat, pos) = GC.@preserve pj pk lc keep qat lat pos check(ccall((:pmt_sparse_gram_sum_merge, lib), Cint,
        (Int64, Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{Ptr{Cvoid}}, Ptr{Int64},
         Ref{Int64}, Ref{Int64}, Ptr{UInt32}, Ptr{UInt32}, Ptr{UInt32}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}),
        n, K, ptrs(pj), ptrs(pk), nqs, ptrs(lc), nls, nt, kinds, has_vec, ptrs(keep), ncols, nq, nlin,
        arg(opj), arg(opk), arg(olc), tabs(qat), tabs(lat), tabs(pos)))
    merge(nothing, nothing, nothing, nothing, nothing, nothing)
    opj, opk, olc = zeros(UInt32, max(nq[], 1)), zeros(UInt32, max(nq[], 1)), zeros(UInt32, max(nlin[], 1))
    qat, lat = [zeros(UInt32, max(nq[], 1)) for _ in 1:K], [zeros(UInt32, max(nlin[], 1)) for _ in 1:K]
    pos = [c === nothing ? nothing : fill(Int32(-1), max(n, 1)) for c in lists]
    merge(opj, opk, olc, qat, lat, pos)
    (nq = nq[], nlin = nlin[], pair_j = opj, pair_k = opk, lin_col = olc, quad_at = qat, lin_at = lat, term_pos = pos)
end

"pmt_sparse_lsq_term: one term of the weighted sum sparse_gram_sum! combines (pointers are device addresses or C_NULL)"
struct SparseLsqTerm
    kind::Int32
    sign::Int32
    scale::Float64
    weight::DevPtr
    quad::DevPtr
    lin::DevPtr
    constant::DevPtr
    quad_at::DevPtr
    lin_at::DevPtr
    vec::DevPtr
    pos::DevPtr
    nvec::Int64
end

"the canonical MOI function of a weighted sum over sparse blocks (csrc/sparse_gram_sum.hip): every block's sparse_gram! (moi = 1) has
written its scratch lists; `terms` is a host Vector{SparseLsqTerm} in expression order, the tables those of sparse_gram_sum_plan as device copies"
sparse_gram_sum!(out_quad::DevPtr, out_lin::DevPtr, out_const::DevPtr, n, terms::Vector{SparseLsqTerm}, pair_j::DevPtr, pair_k::DevPtr, nq,
                 lin_col::DevPtr, nlin, xvar::DevPtr, varmap::DevPtr, stream) =
    check(ccall((:pmt_sparse_gram_sum_f64, lib), Cint,
                (Int64, Ptr{SparseLsqTerm}, Cint, DevPtr, DevPtr, Int64, DevPtr, Int64, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                n, terms, length(terms), pair_j, pair_k, nq, lin_col, nlin, xvar, varmap, out_quad, out_lin, out_const, stream))

"symbolic phase of the sparse quadratic form transpose(x)*Q*x (host, once per pattern): the unordered pairs {j, k}, j <= k, with Q[j,k] or
Q[k,j] stored, sorted by (j, k), and per pair the positions in nzval of Q[j,k] (src_a) and Q[k,j] (src_b), 0xFFFFFFFF where not stored"
function sparse_form_plan(Q::SparseMatrixCSC{Float64,Int64})
    n = size(Q, 1)
    size(Q, 2) == n || throw(DimensionMismatch("sparse_form_plan: Q must be square"))
    nq = Ref{Int64}(0)
    check(ccall((:pmt_sparse_form_count, lib), Cint, (Int64, Ptr{Int64}, Ptr{Int64}, Ref{Int64}), n, Q.colptr, Q.rowval, nq))
    pj, pk, sa, sb = (zeros(UInt32, max(nq[], 1)) for _ in 1:4)
    check(ccall((:pmt_sparse_form_order, lib), Cint, (Int64, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{UInt32}, Ptr{UInt32}, Ptr{UInt32}, Ptr{UInt32}),
                n, Q.colptr, Q.rowval, nq[], pj, pk, sa, sb))
    (nq = nq[], pair_j = pj, pair_k = pk, src_a = sa, src_b = sb)
end

"the canonical MOI function of transpose(x)*Q*x with a sparse Q (csrc/sparse_form.hip): the tables of sparse_form_plan as device copies;
nq quadratic terms, no linear terms, `out_const` (or C_NULL) receives 0.0"
sparse_form!(out_quad::DevPtr, out_const::DevPtr, nzval::DevPtr, src_a::DevPtr, src_b::DevPtr, pair_j::DevPtr, pair_k::DevPtr, nq, xvar::DevPtr, moi,
             varmap::DevPtr, stream) =
    check(ccall((:pmt_sparse_form_f64, lib), Cint,
                (DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, Int64, DevPtr, Cint, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                nzval, src_a, src_b, pair_j, pair_k, nq, xvar, moi, varmap, out_quad, out_const, stream))

"dst (cols x rows, leading dimension ldd) = transpose of src (rows x cols, leading dimension lds) — the adjoint rule, src/lazyexpression.jl:206-217"
transpose!(dst::DevPtr, ldd, src::DevPtr, lds, rows, cols, stream) =
    check(ccall((:pmt_transpose_f64, lib), Cint, (DevPtr, Int64, Int64, Int64, DevPtr, Int64, Ptr{Cvoid}), src, lds, rows, cols, dst, ldd, stream))

"(order, groups, stage_rows): the fixed summation order of the node's constant for an r x n problem (include/parametron_hip.h)"
function quad_gram_constant_order(rows, cols)
    o = Ref{Cint}(0); g = Ref{Cint}(0); s = Ref{Cint}(0)
    check(ccall((:pmt_quad_gram_constant_order, lib), Cint, (Int64, Int64, Ref{Cint}, Ref{Cint}, Ref{Cint}), rows, cols, o, g, s))
    Int(o[]), Int(g[]), Int(s[])
end
"bytes of workspace pmt_quad_gram_f64 needs for an r x n problem"
quad_gram_workspace_bytes(rows, cols) = ccall((:pmt_quad_gram_workspace_bytes, lib), Csize_t, (Int64, Int64), rows, cols)

# ---- staged (overlapped) uploads of host-updated Parameters (`Parameter(model, val=buf)`, src/parameter.jl:88): copy stream + commit
stage_upload!(plan::Plan, staging::DevPtr, src::Array) =
    check(ccall((:pmt_plan_stage_upload, lib), Cint, (Ptr{Cvoid}, DevPtr, Ptr{Cvoid}, Csize_t), plan.handle, staging, src, sizeof(src)))
stage_upload_matrix!(plan::Plan, staging::DevPtr, ldd, A::Matrix{Float64}) =
    check(ccall((:pmt_plan_stage_upload_2d, lib), Cint, (Ptr{Cvoid}, DevPtr, Csize_t, Ptr{Cvoid}, Csize_t, Csize_t, Csize_t),
                plan.handle, staging, 8 * ldd, A, 8 * size(A, 1), 8 * size(A, 1), size(A, 2)))
"the same from a FLAT page-locked vector holding the rows x cols value column-major (the staging copy of a Parameter value)"
stage_upload_pitched!(plan::Plan, staging::DevPtr, ldd, src::Vector{Float64}, rows, cols) =
    check(ccall((:pmt_plan_stage_upload_2d, lib), Cint, (Ptr{Cvoid}, DevPtr, Csize_t, Ptr{Cvoid}, Csize_t, Csize_t, Csize_t),
                plan.handle, staging, 8 * ldd, src, 8 * rows, 8 * rows, cols))
commit_staged!(plan::Plan, dst::DevPtr, staging::DevPtr, bytes) =
    check(ccall((:pmt_plan_commit_staged, lib), Cint, (Ptr{Cvoid}, DevPtr, DevPtr, Csize_t), plan.handle, dst, staging, bytes))
staging_consumed!(plan::Plan) = check(ccall((:pmt_plan_staging_consumed, lib), Cint, (Ptr{Cvoid},), plan.handle))
staged_synchronize(plan::Plan) = check(ccall((:pmt_plan_staged_synchronize, lib), Cint, (Ptr{Cvoid},), plan.handle))
"staging slot (0 / 1) of the calls above; alternate it (and the staging buffers) per update so the next copy does not wait for this update's commits"
stage_slot!(plan::Plan, slot::Integer) = check(ccall((:pmt_plan_stage_slot, lib), Cint, (Ptr{Cvoid}, Cint), plan.handle, slot))

"lane of the commits that follow: 0 = the plan's stream, 1 = its side stream (Parameters that only side-lane entries of the tape read)"
commit_lane!(plan::Plan, lane::Integer) = check(ccall((:pmt_plan_commit_lane, lib), Cint, (Ptr{Cvoid}, Cint), plan.handle, lane))

"plan stream: wait for the staged uploads of the current slot (then commit / consume them)"
wait_staged!(plan::Plan) = check(ccall((:pmt_plan_wait_staged, lib), Cint, (Ptr{Cvoid},), plan.handle))

# ---- page-locked host memory: the staging buffers of host-updated Parameters and the arrays a HOST solver is handed
"a Vector{Float64} over page-locked memory (pmt_host_alloc); free with host_free — NOT garbage collected, the device copies into it asynchronously"
function host_alloc(n::Integer)
    ref = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pmt_host_alloc, lib), Cint, (Csize_t, Ref{Ptr{Cvoid}}), 8 * max(n, 1), ref))
    unsafe_wrap(Array, Ptr{Float64}(ref[]), n; own = false)
end
host_free(v::Vector{Float64}) = check(ccall((:pmt_host_free, lib), Cint, (Ptr{Cvoid},), pointer(v)))

"""host_alloc_as(T, n) -> Vector{T} over page-locked memory (pmt_host_alloc) for an isbits T — e.g. the `terms` vector of an MOI function
(`MOI.VectorAffineTerm{Float64}` = 24 bytes = pmt_vector_affine_term): a recorded entry point is given `pointer(v)` as its output and the kernel
stores straight into the vector the function object holds — no device twin, no fetch.  NOT garbage collected (`host_free_ptr(pointer(v))`).
(Registering the host language's own arrays in place — hipHostRegister — was tried in round 6 and removed: small heap arrays share pages
with their neighbours, and unregistering one pulls the mapping from under the others.)"""
function host_alloc_as(::Type{T}, n::Integer) where {T}
    isbitstype(T) || throw(ArgumentError("host_alloc_as: $T is not an isbits type"))
    ref = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pmt_host_alloc, lib), Cint, (Csize_t, Ref{Ptr{Cvoid}}), sizeof(T) * max(n, 1), ref))
    unsafe_wrap(Array, Ptr{T}(ref[]), n; own = false)
end
host_free_ptr(p::Ptr) = check(ccall((:pmt_host_free, lib), Cint, (Ptr{Cvoid},), p))

# ---- update!(m::Model) of a SMALL model behind one call (include/parametron_hip.h: pmt_model_*; csrc/modelrun.hip)
"the per-solve walk of a small model: mailboxes of host-updated Parameters, seed words of device-regenerated ones, fetches, constants"
mutable struct ModelRun
    handle::Ptr{Cvoid}
    plan::Plan                        # (kept alive: the run refers to it)
    function ModelRun(plan::Plan)
        ref = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:pmt_model_create, lib), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), plan.handle, ref))
        r = new(ref[], plan)
        finalizer(r -> ccall((:pmt_model_destroy, lib), Cint, (Ptr{Cvoid},), r.handle), r)
        r
    end
end
"`host`: the Parameter's value (Matrix: strides (1, size(host, 1)); Vector: cols = 0); `mailbox`: page-locked, `ld` doubles per column.  Returns the slot."
function add_mailbox!(run::ModelRun, host::Ptr{Float64}, rows::Integer, cols::Integer, row_stride::Integer, col_stride::Integer, mailbox::Vector{Float64}, ld::Integer)
    slot = Ref{Cint}(-1)
    check(ccall((:pmt_model_add_mailbox, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Int64, Ptr{Float64}, Int64, Ref{Cint}),
                run.handle, host, rows, cols, row_stride, col_stride, pointer(mailbox), ld, slot))
    Int(slot[])
end
"a device-regenerated Parameter: `word[]` = base + stride * (number of updates so far), stored before every replay"
function add_seed!(run::ModelRun, word::Ref{UInt64}, base::Integer, stride::Integer)
    slot = Ref{Cint}(-1)
    check(ccall((:pmt_model_add_seed, lib), Cint, (Ptr{Cvoid}, Ref{UInt64}, UInt64, UInt64, Ref{Cint}), run.handle, word, base, stride, slot))
    Int(slot[])
end
set_host!(run::ModelRun, slot::Integer, host::Ptr{Float64}) =
    check(ccall((:pmt_model_set_host, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}), run.handle, slot, host))
"behind the wait of every update: `dst[] = src[]` (e.g. a scalar function's constant out of its page-locked word)"
add_constant!(run::ModelRun, src::Ptr{Float64}, dst::Ptr{Float64}) =
    check(ccall((:pmt_model_add_constant, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), run.handle, src, dst))
"a result that lives in HBM: copied into `dst` (page-locked) behind every replay, in front of the wait"
add_fetch!(run::ModelRun, dst::Array, src::DevPtr, bytes::Integer = sizeof(dst)) =
    check(ccall((:pmt_model_add_fetch, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, DevPtr, Csize_t), run.handle, dst, src, bytes))
num_slots(run::ModelRun) = Int(ccall((:pmt_model_num_slots, lib), Cint, (Ptr{Cvoid},), run.handle))
"""one update!(model): dirty mailboxes / seeds refreshed, the tape replayed, (synchronize) the MOI buffers complete on the host.
`dirty === nothing`: every slot (setdirty!(model) semantics, src/model.jl:132-133); else one byte per slot."""
model_update!(run::ModelRun, dirty::Nothing, synchronize::Bool = true) =
    check(ccall((:pmt_model_update, lib), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Cint, Cint), run.handle, C_NULL, 0, synchronize ? 1 : 0))
model_update!(run::ModelRun, dirty::Vector{UInt8}, synchronize::Bool = true) =
    check(ccall((:pmt_model_update, lib), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Cint, Cint), run.handle, dirty, length(dirty), synchronize ? 1 : 0))
model_wait!(run::ModelRun) = check(ccall((:pmt_model_wait, lib), Cint, (Ptr{Cvoid},), run.handle))

# ---- delivery to a HOST solver while the re-evaluation runs (include/parametron_hip.h: pmt_plan_record_fetch, pmt_quad_gram_csc_deliver_f64)
"while recording: `dst` (page-locked) receives `bytes` from `src` on the plan's fetch path as soon as what was recorded before it on its lane is done"
record_fetch!(plan::Plan, dst::Array, src::DevPtr, bytes::Integer = sizeof(dst)) =
    check(ccall((:pmt_plan_record_fetch, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, DevPtr, Csize_t), plan.handle, dst, src, bytes))
"while recording, pitched: `cols` columns of `rows` doubles out of a padded device matrix (leading dimension `lds`) into host columns `dst_pitch_bytes` apart —
the CSC values of a dense constraint block leave straight out of its Parameter buffer"
record_fetch_matrix!(plan::Plan, dst::Ptr{Float64}, dst_pitch_bytes, src::DevPtr, lds, rows, cols) =
    check(ccall((:pmt_plan_record_fetch_2d, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, DevPtr, Csize_t, Csize_t, Csize_t),
                plan.handle, dst, dst_pitch_bytes, src, 8 * lds, 8 * rows, cols))
"host -> host: `cols` columns of `rows` doubles, `src_pitch_bytes` apart in the source, `dst_pitch_bytes` apart in the destination, on the library's
worker threads (pmt_host_copy_2d) — the dense blocks of a host solver's A whose Parameter values are already on the host"
host_copy_matrix!(dst::Ptr{Float64}, dst_pitch_bytes, src::Ptr{Float64}, src_pitch_bytes, rows, cols; threads::Integer = 0) =
    check(ccall((:pmt_host_copy_2d, lib), Cint, (Ptr{Cvoid}, Csize_t, Ptr{Cvoid}, Csize_t, Csize_t, Csize_t, Cint),
                dst, dst_pitch_bytes, src, src_pitch_bytes, 8 * rows, cols, threads))
"how results leave for the host: 0 automatic, 1 copy engine or an error, 2 kernel copies (include/parametron_hip.h)"
set_host_delivery(mode::Integer) = check(ccall((:pmt_set_host_delivery, lib), Cint, (Cint,), mode))
"(mode, copy engine usable on `device`)"
function host_delivery(device::Integer = 0)
    mode, engine = Ref{Cint}(0), Ref{Cint}(0)
    check(ccall((:pmt_get_host_delivery, lib), Cint, (Cint, Ref{Cint}, Ref{Cint}), device, mode, engine))
    (Int(mode[]), engine[] != 0)
end
"host: every recorded fetch / delivered band group of the last update has landed"
fetch_synchronize(plan::Plan) = check(ccall((:pmt_plan_fetch_synchronize, lib), Cint, (Ptr{Cvoid},), plan.handle))
"pitched device -> host copy on the plan's stream: the columns of a padded device matrix into a dense host column range (setup / serial path)"
fetch_matrix!(plan::Plan, dst::Ptr{Float64}, dst_pitch_bytes, src::DevPtr, lds, rows, cols) =
    check(ccall((:pmt_plan_fetch_2d, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, DevPtr, Csize_t, Csize_t, Csize_t),
                plan.handle, dst, dst_pitch_bytes, src, 8 * lds, 8 * rows, cols))
"the Gram node with P's CSC values DELIVERED band group by band group into the page-locked `host_P` while the contraction runs"
quad_gram_csc_deliver!(out_P_values, host_P::Vector{Float64}, out_lin, out_const, A, lda, rows, cols, xvar, b, sign, varmap, alpha, workspace, stream; ngroups::Integer = 0) =
    check(ccall((:pmt_quad_gram_csc_deliver_f64, lib), Cint,
                (DevPtr, Int64, Int64, Int64, DevPtr, DevPtr, Cint, DevPtr, Cdouble, DevPtr, Ptr{Cvoid}, Cint, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                A, lda, rows, cols, xvar, b, sign, varmap, alpha, out_P_values, host_P, ngroups, out_lin, out_const, workspace, stream))

"the Gram node with the MOI quadratic terms DELIVERED row band by row band into page-locked `host_quad` (pmt_host_alloc'ed memory viewed as
24-byte terms) while the contraction runs — the reference's own boundary, src/moi_interop.jl:131-137"
quad_gram_deliver!(out_quad::DevPtr, host_quad::Ptr{Cvoid}, out_lin, out_const, A, lda, rows, cols, xvar, b, sign, moi, varmap, workspace, stream; nstages::Integer = 0) =
    check(ccall((:pmt_quad_gram_deliver_f64, lib), Cint,
                (DevPtr, Int64, Int64, Int64, DevPtr, DevPtr, Cint, Cint, DevPtr, DevPtr, Ptr{Cvoid}, Cint, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                A, lda, rows, cols, xvar, b, sign, moi, varmap, out_quad, host_quad, nstages, out_lin, out_const, workspace, stream))

# ---- further builders used by ParametronHIPBackend.jl
"x (+|-) v for x::Vector{Variable} (bounds): one term per row; native and/or MOI output may be C_NULL — src/functions.jl:421,751-764"
vars_addsub!(out_lt::DevPtr, out_vat::DevPtr, out_consts::DevPtr, xvar::DevPtr, n, v::DevPtr, sign, varmap::DevPtr, row_offset, stream) =
    check(ccall((:pmt_vars_addsub_f64, lib), Cint, (DevPtr, Int64, DevPtr, Cint, DevPtr, Int64, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                xvar, n, v, sign, varmap, row_offset, out_lt, out_vat, out_consts, stream))
"dest[i] = s * y[i] for a device scalar s: scale!(dest, x::Number, y::Vector{AffineFunction}) — src/functions.jl:895-915"
affvec_scale!(out_terms::DevPtr, out_consts::DevPtr, rows, nterms, y_terms::DevPtr, y_consts::DevPtr, s_dev::DevPtr, stream) =
    check(ccall((:pmt_affvec_scale_f64, lib), Cint, (Int64, Int64, DevPtr, DevPtr, DevPtr, Cdouble, DevPtr, DevPtr, Ptr{Cvoid}),
                rows, nterms, y_terms, y_consts, s_dev, 0.0, out_terms, out_consts, stream))
"update!(::MOI.VectorAffineFunction, fs, varmap) of a materialised Vector{AffineFunction} with uniform rows — src/moi_interop.jl:64-81"
pack_vector_affine!(out_terms::DevPtr, terms::DevPtr, rows, row_len, varmap::DevPtr, row_offset, stream) =
    check(ccall((:pmt_pack_vector_affine_f64, lib), Cint, (DevPtr, DevPtr, Int64, Int64, DevPtr, Int64, DevPtr, Ptr{Cvoid}),
                terms, C_NULL, rows, row_len, varmap, row_offset, out_terms, stream))
"device-to-device copy on the stream (vcat! pieces of constants)"
copy_bytes!(dst::DevPtr, src::DevPtr, bytes, stream) =
    check(ccall((:pmt_copy_bytes, lib), Cint, (DevPtr, DevPtr, Csize_t, Ptr{Cvoid}), dst, src, bytes, stream))

# ---- batched independent models across GPUs (BASELINE config 4): the library's own RCCL communicator
"rank 0: a fresh 128-byte id; carry it to the other ranks with whatever launcher is at hand (MPI.jl, Distributed, a file)"
function comm_unique_id()
    id = zeros(UInt8, 128)
    check(ccall((:pmt_comm_unique_id, lib), Cint, (Ptr{Cvoid},), id))
    id
end
function comm_init_rank(nranks::Integer, rank::Integer, id::Vector{UInt8}, device::Integer)
    ref = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pmt_comm_init_rank, lib), Cint, (Cint, Cint, Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}), nranks, rank, id, device, ref))
    ref[]
end
comm_destroy(comm::Ptr{Cvoid}) = check(ccall((:pmt_comm_destroy, lib), Cint, (Ptr{Cvoid},), comm))
"(per_rank, first) of `rank`'s shard of `total` instances; DimensionMismatch when the batch does not divide over the ranks"
function batch_shard(total::Integer, nranks::Integer, rank::Integer)
    per = Ref{Int64}(0); first = Ref{Int64}(0)
    check(ccall((:pmt_batch_shard, lib), Cint, (Int64, Cint, Cint, Ref{Int64}, Ref{Int64}), total, nranks, rank, per, first))
    per[], first[]
end
"one re-evaluation of this rank's instances, chunk c on the wire while chunk c + 1 is computed; `gathered` ends up with every rank's slabs"
batch_step!(comm::Ptr{Cvoid}, A::DevPtr, b::DevPtr, C::DevPtr, d::DevPtr, per_rank, n, r, m, local_slabs::DevPtr, gathered::DevPtr, stride, chunk, stream) =
    check(ccall((:pmt_batch_step_f64, lib), Cint,
                (Ptr{Cvoid}, DevPtr, DevPtr, DevPtr, DevPtr, Int64, Int64, Int64, Int64, Cint, Cint, DevPtr, DevPtr, Int64, Int64, Ptr{Cvoid}),
                comm, A, b, C, d, per_rank, n, r, m, -1, -1, local_slabs, gathered, stride, chunk, stream))

"one slab [Q | q | const | C | d-consts] per instance for the batch of tracking costs transpose(x ± p_i) * Q_i * (x ± p_i) over C_i*x ± d_i
 (n <= 256): instance-major Q (column-major, need not be symmetric), p, C, d; the layout of the least-squares batch, the Q / q / const of
 quad_form_shift! for the instance alone bit for bit; sign_p == 0: the plain form"
batch_form_coeffs!(out::DevPtr, out_stride, Q::DevPtr, p::DevPtr, C::DevPtr, d::DevPtr, B, n, m, sign_p, sign_d, stream) =
    check(ccall((:pmt_batch_form_coeffs_f64, lib), Cint,
                (DevPtr, DevPtr, DevPtr, DevPtr, Int64, Int64, Int64, Cint, Cint, DevPtr, Int64, Ptr{Cvoid}),
                Q, p, C, d, B, n, m, sign_p, sign_d, out, out_stride, stream))

"doubles of one instance's slab [SQ | SR | q | const | C | d-consts] of the batch of horizons, n = T*(nx + nu)"
batch_horizon_slab_doubles(T, nx, nu, m) = ccall((:pmt_batch_horizon_slab_doubles, lib), Int64, (Int64, Int64, Int64, Int64), T, nx, nu, m)

"one slab per instance for the batch of horizons sum_t transpose(x_t ± r_t) * Q_i * (x_t ± r_t) + transpose(u_t ± v_t) * R_i * (u_t ± v_t) over
 C_i*z ± d_i, z = [x_0; u_0; x_1; ..] (nx, nu <= 128, T <= 512): instance-major Q, R (column-major, need not be symmetric), stage-major r, v;
 SQ / SR / q / const bit for bit what quad_stages! writes for the instance's own table; a sign of 0: plain stages, the reference may be C_NULL"
batch_horizon_coeffs!(out::DevPtr, out_stride, Q::DevPtr, R::DevPtr, r::DevPtr, v::DevPtr, C::DevPtr, d::DevPtr, B, T, nx, nu, m, sign_r, sign_v,
                      sign_d, stream) =
    check(ccall((:pmt_batch_horizon_coeffs_f64, lib), Cint,
                (DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, Int64, Int64, Int64, Int64, Int64, Cint, Cint, Cint, DevPtr, Int64, Ptr{Cvoid}),
                Q, R, r, v, C, d, B, T, nx, nu, m, sign_r, sign_v, sign_d, out, out_stride, stream))

"one instance's MOI buffers from its horizon slab: the quadratic / linear terms and the constant of quad_stages! for its table, the
 constraint block of the least-squares batch's expansion; xvar: the n model variables of z"
batch_horizon_expand!(slab::DevPtr, T, nx, nu, m, xvar::DevPtr, varmap::DevPtr, out_quad::DevPtr, out_lin::DevPtr, out_const::DevPtr,
                      out_vat::DevPtr, out_vconsts::DevPtr, stream) =
    check(ccall((:pmt_batch_horizon_expand_f64, lib), Cint,
                (DevPtr, Int64, Int64, Int64, Int64, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                slab, T, nx, nu, m, xvar, varmap, out_quad, out_lin, out_const, out_vat, out_vconsts, stream))

"doubles of one instance's dynamics section [AB: nx*(nx + nu) | h-consts: T*nx] of the batch of horizons"
batch_horizon_dynamics_doubles(T, nx, nu) = ccall((:pmt_batch_horizon_dynamics_doubles, lib), Int64, (Int64, Int64, Int64), T, nx, nu)

"one compact dynamics section per instance for the batch of horizons: x_0 ± h_0 and ±x_t ± A_i*x_{t-1} ± B_i*u_{t-1} ± h_t, t = 1 .. T-1
 (nx, nu <= 128, T <= 512): instance-major A, B (column-major, leading dimension nx), stage-major h; AB row-major with the parts' signs on
 its words, the constants 0.0 ± h; sign_h = 0: h may be C_NULL; nu = 0: B may be C_NULL.  out = slabs + L, out_stride = L + Ld puts the
 section behind the instance's objective slab"
batch_horizon_dynamics!(out::DevPtr, out_stride, A::DevPtr, B::DevPtr, h::DevPtr, nbatch, T, nx, nu, sign_a, sign_b, sign_h, stream) =
    check(ccall((:pmt_batch_horizon_dynamics_f64, lib), Cint,
                (DevPtr, DevPtr, DevPtr, Int64, Int64, Int64, Int64, Cint, Cint, Cint, DevPtr, Int64, Ptr{Cvoid}),
                A, B, h, nbatch, T, nx, nu, sign_a, sign_b, sign_h, out, out_stride, stream))

"one instance's T MOI.VectorAffineFunction buffers from its dynamics section, word for word what affine_stages! writes for the instance's
 own tables; xvar: the n model variables of z, varmap may be C_NULL (the identity)"
batch_horizon_dynamics_expand!(section::DevPtr, T, nx, nu, sign_xp, xvar::DevPtr, varmap::DevPtr, out_terms::DevPtr, out_consts::DevPtr, stream) =
    check(ccall((:pmt_batch_horizon_dynamics_expand_f64, lib), Cint,
                (DevPtr, Int64, Int64, Int64, Cint, DevPtr, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                section, T, nx, nu, sign_xp, xvar, varmap, out_terms, out_consts, stream))

"doubles of one instance's time-varying dynamics section [AB_1 | .. | AB_{T-1} | h-consts: T*nx], each AB_t nx*(nx + nu) words"
batch_horizon_dynamics_tv_doubles(T, nx, nu) = ccall((:pmt_batch_horizon_dynamics_tv_doubles, lib), Int64, (Int64, Int64, Int64), T, nx, nu)

"one compact section per instance for horizons whose dynamics change with the stage: x_0 ± h_0 and ±x_t ± A_{i,t}*x_{t-1} ± B_{i,t}*u_{t-1} ± h_t,
 t = 1 .. T-1 (nx, nu <= 128, T <= 512): A[nbatch][T-1][nx*nx], B[nbatch][T-1][nx*nu] instance- then stage-major (column-major, leading
 dimension nx; matrix index t-1 belongs to record t), stage-major h; every AB_t is the block batch_horizon_dynamics! writes for that pair, the
 constants 0.0 ± h; sign_h = 0: h may be C_NULL; nu = 0: B may be C_NULL; T = 1: A and B may be C_NULL"
batch_horizon_dynamics_tv!(out::DevPtr, out_stride, A::DevPtr, B::DevPtr, h::DevPtr, nbatch, T, nx, nu, sign_a, sign_b, sign_h, stream) =
    check(ccall((:pmt_batch_horizon_dynamics_tv_f64, lib), Cint,
                (DevPtr, DevPtr, DevPtr, Int64, Int64, Int64, Int64, Cint, Cint, Cint, DevPtr, Int64, Ptr{Cvoid}),
                A, B, h, nbatch, T, nx, nu, sign_a, sign_b, sign_h, out, out_stride, stream))

"one instance's T MOI.VectorAffineFunction buffers from its time-varying dynamics section, word for word what affine_stages! writes for the
 instance's own tables with stage t's matrix parts at A_{i,t}, B_{i,t}; xvar: the n model variables of z, varmap may be C_NULL (the identity)"
batch_horizon_dynamics_tv_expand!(section::DevPtr, T, nx, nu, sign_xp, xvar::DevPtr, varmap::DevPtr, out_terms::DevPtr, out_consts::DevPtr, stream) =
    check(ccall((:pmt_batch_horizon_dynamics_tv_expand_f64, lib), Cint,
                (DevPtr, Int64, Int64, Int64, Cint, DevPtr, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                section, T, nx, nu, sign_xp, xvar, varmap, out_terms, out_consts, stream))

"doubles of one instance's slab [S: ns blocks in z order | q: n | sconst: ns | const | C: m*n | d-consts: m] of a horizon with a weight matrix
 per stage, n = T*(nx + nu) + term*nx, ns = T*(1 + (nu > 0)) + term"
batch_horizon_tv_slab_doubles(T, nx, nu, term, m) =
    ccall((:pmt_batch_horizon_tv_slab_doubles, lib), Int64, (Int64, Int64, Int64, Int64, Int64), T, nx, nu, term, m)

"one slab per instance for horizons whose stage weights change with the stage: sum_t (x_t ± r_t)'Q_{i,t}(x_t ± r_t) + (u_t ± v_t)'R_{i,t}(u_t ± v_t),
 with term = 1 a last stage x_T under Q_{i,T}, subject to C_i*z ± d_i (nx, nu <= 128, T <= 512): Q[nbatch][T+term][nx*nx], R[nbatch][T][nu*nu]
 instance- then stage-major (column-major), r[nbatch][T+term][nx], v[nbatch][T][nu]; every block, q word and constant is what quad_stages!
 writes for the instance's own table; a sign of 0: the reference may be C_NULL; nu = 0: R and v may be C_NULL"
batch_horizon_tv_coeffs!(out::DevPtr, out_stride, Q::DevPtr, R::DevPtr, r::DevPtr, v::DevPtr, C::DevPtr, d::DevPtr, nbatch, T, nx, nu, term, m,
                         sign_r, sign_v, sign_d, stream) =
    check(ccall((:pmt_batch_horizon_tv_coeffs_f64, lib), Cint,
                (DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, Int64, Int64, Int64, Int64, Int64, Int64, Cint, Cint, Cint, DevPtr, Int64, Ptr{Cvoid}),
                Q, R, r, v, C, d, nbatch, T, nx, nu, term, m, sign_r, sign_v, sign_d, out, out_stride, stream))

"one instance's MOI buffers from its slab of batch_horizon_tv_coeffs!, word for word what quad_stages! writes for the instance's own table with
 stage s's Q at its own matrix; xvar: the n model variables of z, varmap required"
batch_horizon_tv_expand!(slab::DevPtr, T, nx, nu, term, m, xvar::DevPtr, varmap::DevPtr, out_quad::DevPtr, out_lin::DevPtr, out_const::DevPtr,
                         out_vat::DevPtr, out_vconsts::DevPtr, stream) =
    check(ccall((:pmt_batch_horizon_tv_expand_f64, lib), Cint,
                (DevPtr, Int64, Int64, Int64, Int64, Int64, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                slab, T, nx, nu, term, m, xvar, varmap, out_quad, out_lin, out_const, out_vat, out_vconsts, stream))

"pmt_batch_horizon_terms (include/parametron_hip.h): the inputs of batch_horizon_terms_coeffs!, device pointers, instance-major.  C_NULL: P no
 terminal stage, a weight array every weight 1.0, a linear array no linear term, a reference only where its sign is 0; 128 bytes, no padding"
struct BatchHorizonTerms
    Q::DevPtr
    R::DevPtr
    P::DevPtr
    r::DevPtr
    v::DevPtr
    rN::DevPtr
    wx::DevPtr
    wu::DevPtr
    wN::DevPtr
    gx::DevPtr
    gu::DevPtr
    gN::DevPtr
    C::DevPtr
    d::DevPtr
    sign_r::Int32
    sign_v::Int32
    sign_rN::Int32
    sign_d::Int32
end

"doubles of one instance's slab [SQ | SR | SP | W | q | const | C | d-consts] of the batch of horizons with terms; term = 1 with a terminal stage"
batch_horizon_terms_slab_doubles(T, nx, nu, term, m) =
    ccall((:pmt_batch_horizon_terms_slab_doubles, lib), Int64, (Int64, Int64, Int64, Int64, Int64), T, nx, nu, term, m)

"one slab per instance for the batch of horizons with a terminal cost wN * transpose(x_T ± rN) * P_i * (x_T ± rN), a weight per stage and linear
 stage terms dot(g, ·): W / q / const bit for bit what quad_stages_terms! writes for the instance's own table with scale = 1.0 and
 weight = &W_s; with every optional pointer C_NULL the slab without its W section is batch_horizon_coeffs!'s"
batch_horizon_terms_coeffs!(out::DevPtr, out_stride, desc::BatchHorizonTerms, B, T, nx, nu, m, stream) =
    check(ccall((:pmt_batch_horizon_terms_coeffs_f64, lib), Cint,
                (Ref{BatchHorizonTerms}, Int64, Int64, Int64, Int64, Int64, DevPtr, Int64, Ptr{Cvoid}),
                desc, B, T, nx, nu, m, out, out_stride, stream))

"one instance's MOI buffers from its slab with terms: the quadratic terms W_s * S[j,k], the linear terms and the constant copied — what
 quad_stages_terms! writes for its table [x_0, u_0, .., x_T]; xvar: the n = T*(nx + nu) + term*nx model variables of z"
batch_horizon_terms_expand!(slab::DevPtr, T, nx, nu, term, m, xvar::DevPtr, varmap::DevPtr, out_quad::DevPtr, out_lin::DevPtr, out_const::DevPtr,
                            out_vat::DevPtr, out_vconsts::DevPtr, stream) =
    check(ccall((:pmt_batch_horizon_terms_expand_f64, lib), Cint,
                (DevPtr, Int64, Int64, Int64, Int64, Int64, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                slab, T, nx, nu, term, m, xvar, varmap, out_quad, out_lin, out_const, out_vat, out_vconsts, stream))

"the same callback RECORDED with its seed in a host word (`Ref{UInt64}`, kept alive by the caller): every replay draws the stream of the
seed the word holds then — `seed[] += 1000` before `update!(plan)` is the whole callback"
device_uniform_dyn!(dst::DevPtr, rows, cols, lda, seed::Ref{UInt64}, scale, stream) =
    check(ccall((:pmt_fill_uniform_dyn_f64, lib), Cint, (DevPtr, Int64, Int64, Int64, Ref{UInt64}, Cdouble, Ptr{Cvoid}), dst, rows, cols, lda, seed, scale, stream))

"device-side `rand!` Parameter callback (README.md:36-43): U[0,1)*scale, counter based"
device_uniform!(dst::DevPtr, n, seed, scale, stream) =
    check(ccall((:pmt_fill_uniform_f64, lib), Cint, (DevPtr, Int64, UInt64, Cdouble, Ptr{Cvoid}), dst, n, seed, scale, stream))

end # module
