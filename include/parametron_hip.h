/*
 * parametron_hip.h — C ABI of libparametron_hip.so: the MI355X (gfx950) implementation of
 * Parametron.jl's parameter-update / coefficient re-evaluation hot path.
 *
 * The reference (tkoolen/Parametron.jl v0.9.1, pure Julia) has no FFI of its own; the de-facto
 * operator interface of the path is
 *   (1) the in-place builders of Parametron.Functions that the `optimize` rewrite rules splice
 *       into the lazy-expression DAG           (src/lazyexpression.jl:200-302, src/functions.jl)
 *   (2) update!(moi_f, f, varmap) x3            (src/moi_interop.jl:35-81)
 *   (3) the per-node call ABI FunctionWrapper{T,Tuple{}} (src/FunctionWrappersQuickFix.jl:108-126)
 *       driven by update!(m::Model)             (src/model.jl:132-143).
 * Each entry point below names the reference function(s) it replaces.  A Julia host binds them
 * with `ccall((:pmt_xxx, libparametron_hip), Cint, (...), ...)` — see INTEGRATION.md.
 *
 * Conventions
 *   - plain C, no HIP/torch types: `void *stream` is a hipStream_t (NULL = default stream);
 *     every `const double *`, term pointer etc. is a DEVICE pointer unless named host_*.
 *   - all calls are asynchronous on `stream`; nothing allocates or synchronises unless stated
 *     (the reference's `@allocated solve!(model) == 0` contract, test/model.jl:116-124).
 *   - matrices are column-major with leading dimension `lda` (Julia Matrix{Float64},
 *     src/functions.jl:790-796); variable indices are 1-based Int64 (Variable.index).
 *   - `varmap` is model_var_to_optimizer (src/model.jl:8,100-107): varmap[k-1] is the optimizer
 *     index of Variable k; NULL = IdentityVarMap (src/moi_interop.jl:32-33).
 *   - return value: PMT_OK or an error code; pmt_last_error() gives the message.  The Julia/Python
 *     host maps PMT_DIMENSION_MISMATCH -> DimensionMismatch, PMT_INVALID_ARGUMENT -> ArgumentError,
 *     PMT_STATE_ERROR -> ErrorException (src/functions.jl:780-781, src/model.jl:50,61,69).
 *   - threading: calls on one stream/plan must be externally serialised (the reference is
 *     single-threaded and shares `dest` buffers, src/lazyexpression.jl:202-203).
 */
#ifndef PARAMETRON_HIP_H
#define PARAMETRON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMT_OK 0
#define PMT_DIMENSION_MISMATCH 1
#define PMT_INVALID_ARGUMENT 2
#define PMT_HIP_ERROR 3
#define PMT_STATE_ERROR 4
#define PMT_OUT_OF_MEMORY 5

/* Term layouts = the Julia isbits structs. */
typedef struct { double coeff; int64_t var; } pmt_linear_term;                 /* LinearTerm{Float64} src/functions.jl:110-113 == MOI.ScalarAffineTerm (moi_interop.jl:40) */
typedef struct { double coeff; int64_t row; int64_t col; } pmt_quadratic_term; /* QuadraticTerm{Float64} src/functions.jl:136-140 == MOI.ScalarQuadraticTerm (moi_interop.jl:59) */
typedef struct { int64_t output_index; double coeff; int64_t var; } pmt_vector_affine_term; /* MOI.VectorAffineTerm (moi_interop.jl:75) */

const char *pmt_last_error(void);
int pmt_version(void);
/* number of visible HIP devices (<= 0: none); used by hosts to fail loudly without a GPU */
int pmt_device_count(void);

/* ---------------------------------------------------------------------------------------
 * Dense affine nodes
 * ------------------------------------------------------------------------------------- */

/* y = A*x (+|-) b as Vector{AffineFunction}: out_terms[row*cols + col] = (A[row,col], xvar[col]),
 * out_consts[row] = 0.0 (+|-) b[row].   sign: +1 vecadd!, -1 vecsubtract!, 0 no vector (b ignored).
 * Replaces matvecmul!(y, A, x::Vector{Variable}) src/functions.jl:775-798 fused with
 * vecadd!/vecsubtract!(dest, y, b) :751-764 (copyto! :422-427, add!/subtract! Number :452,:474).
 * A block of more than 65535 * 64 = 4194240 rows (with columns) is refused with PMT_DIMENSION_MISMATCH, here and in
 * pmt_affine_pack_vector_f64: the kernel's grid has one block row per 64 rows and does not wrap. */
int pmt_affine_assemble_f64(const double *A, int64_t lda, int64_t rows, int64_t cols,
                            const int64_t *xvar, const double *b, int sign,
                            pmt_linear_term *out_terms, double *out_consts, void *stream);

/* A residual over SEVERAL Variable vectors, r = (+|-)A_1*x_1 (+|-) A_2*x_2 .. (vecadd! / vecsubtract! src/functions.jl:751-764, rules
 * src/lazyexpression.jl:238-258), as one dense block over the union z of the variables:
 *   out[i + c*ldo] = cols[c].sign * cols[c].src[i]   for i < rows, c < ncols  (the product exact: sign is +1 or -1, -1 flips the sign bit)
 * `cols` is a DEVICE table of ncols entries built once by the host: entry c is the c-th variable of z, `src` the start of its column in
 * the block's matrix (A_k + j*lda_k), `sign` that of the block.  Rows rows .. ldo-1 of `out` are never written (a zero-padded workspace
 * stays zero-padded), so the Gram family reads `out` exactly as it reads a Parameter holding the stacked matrix (csrc/stack.hip).  The
 * table's signs are not read on the host: _lib.stack_table (parametron.jl_amd/_lib.py) builds it and checks them. */
typedef struct {
    const double *src;                /* column start */
    int64_t sign;                     /* +1 or -1 */
} pmt_stack_column;                   /* 16 bytes, no padding (static_assert in csrc/stack.hip) */
int pmt_affine_stack_columns_f64(const pmt_stack_column *cols, int64_t ncols, int64_t rows, double *out, int64_t ldo, void *stream);

/* Same node written straight into MOI.VectorAffineFunction buffers:
 * out_terms[row*cols + col] = (row_offset + row + 1, A[row,col], varmap[xvar[col]]), out_consts as above.
 * Replaces the chain above + update!(::MOI.VectorAffineFunction, fs, varmap) src/moi_interop.jl:64-81. */
int pmt_affine_pack_vector_f64(const double *A, int64_t lda, int64_t rows, int64_t cols,
                               const int64_t *xvar, const double *b, int sign,
                               const int64_t *varmap, int64_t row_offset,
                               pmt_vector_affine_term *out_terms, double *out_consts, void *stream);
/* The same node in its BACKGROUND form (identical output): a kernel of at most 16 VGPRs and no LDS, slow on an idle chip but co-resident
 * with the persistent contraction of pmt_quad_gram_f64 (which leaves 16 of a SIMD's 512 VGPRs free).  Recorded on a plan's side lane
 * (pmt_plan_set_lane) it runs inside the contraction instead of behind it. */
int pmt_affine_pack_vector_background_f64(const double *A, int64_t lda, int64_t rows, int64_t cols, const int64_t *xvar, const double *b,
                                          int sign, const int64_t *varmap, int64_t row_offset, pmt_vector_affine_term *out_terms,
                                          double *out_consts, void *stream);

/* dest[i] = x[i] (+|-) v[i] for x::Vector{Variable}: one term (1.0, xvar[i]) per row, constant 0.0 (+|-) v[i]
 * (`x - l` bounds, test/model.jl:162-163).  vecadd!/vecsubtract! with copyto!(f, ::Variable)
 * src/functions.jl:421.  Native output (out_terms_lt) and/or MOI output (out_terms_vat) may be NULL. */
int pmt_vars_addsub_f64(const int64_t *xvar, int64_t n, const double *v, int sign,
                        const int64_t *varmap, int64_t row_offset,
                        pmt_linear_term *out_terms_lt, pmt_vector_affine_term *out_terms_vat,
                        double *out_consts, void *stream);

/* ---------------------------------------------------------------------------------------
 * Generic term-list nodes (materialised Vector{AffineFunction} = flat LT buffer + row_ptr + consts).
 * row_ptr has rows+1 entries (device); NULL means uniform rows of `row_len` terms.
 * ------------------------------------------------------------------------------------- */

/* dst row i = [ xa[i].linear ; sb * xb[i].linear ],  constant  ca[i] (+ sb*cb[i])  with sb = +1 or -1 (exact):
 *   copyto! (:422-427)  then  add!(f, ::AffineFunction) :455  /  subtract!(f, ::AffineFunction) :477-485,
 * i.e. vecadd!/vecsubtract! :751-764 on any mix of Vector{AffineFunction}, Vector{Variable} (pre-materialised
 * by the host as one (1.0, var) term per row, consts NULL: copyto!(f, ::Variable) :421 leaves the constant 0)
 * and number vectors (terms NULL, consts = the numbers: copyto!(f, ::Number) :419, add!/subtract! :452,:474).
 * A part with consts == NULL contributes no constant; part b may be absent altogether (plain copyto!, vcat!
 * pieces :969-994).  If part a has no constants the row constant is 0.0 (+ sb*cb[i]). */
int pmt_affvec_combine_f64(int64_t rows,
                           const pmt_linear_term *xa_terms, const int64_t *xa_row_ptr, int64_t xa_row_len, const double *xa_consts,
                           const pmt_linear_term *xb_terms, const int64_t *xb_row_ptr, int64_t xb_row_len, const double *xb_consts, int sb,
                           pmt_linear_term *out_terms, const int64_t *out_row_ptr, int64_t out_row_len, double *out_consts,
                           void *stream);

/* dest[i] = s * y[i] where s is a device scalar (Parameter{Float64}) or host constant:
 * scale!(dest, x::Number, y::Vector{AffineFunction}) src/functions.jl:895-915 -> mul! :578 -> muladd! :515-523.
 * coeff = s*coeff, const = 0 + y.c*s.  s_dev == NULL uses s_host. */
int pmt_affvec_scale_f64(int64_t rows, int64_t nterms, const pmt_linear_term *y_terms, const double *y_consts,
                         const double *s_dev, double s_host,
                         pmt_linear_term *out_terms, double *out_consts, void *stream);

/* dest[i] = (s, yvar[i]): scale!(dest::Vector{LinearTerm}, x::Number, y::Vector{Variable}) src/functions.jl:873-893 */
int pmt_scale_vars_f64(const int64_t *yvar, int64_t n, const double *s_dev, double s_host, pmt_linear_term *out_terms, void *stream);
/* dest .= s .* y for number arrays: scale! src/functions.jl:917-925 */
int pmt_scale_numbers_f64(const double *y, int64_t n, const double *s_dev, double s_host, double *out, void *stream);
/* dest[j, i] = A[i, j] — the closure of the `adjoint` rewrite rule src/lazyexpression.jl:206-217.
 * src is rows x cols (leading dimension lds), dst is cols x rows (leading dimension ldd), both column-major. */
int pmt_transpose_f64(const double *src, int64_t lds, int64_t rows, int64_t cols, double *dst, int64_t ldd, void *stream);
/* quadratic term lists: out = [ qa ; sb*qb ], sb = +1/-1: copyto! src/functions.jl:434-439, add! :459, subtract! :492-500 */
int pmt_quad_combine_f64(const pmt_quadratic_term *qa, int64_t na, const pmt_quadratic_term *qb, int64_t nb, int sb,
                         pmt_quadratic_term *out, void *stream);
/* out[i] = (s * q[i].coeff, row, col): muladd!(dest::QuadraticFunction, x::QuadraticFunction, y::Number) :526-534 */
int pmt_quad_scale_f64(const pmt_quadratic_term *q, int64_t n, const double *s_dev, double s_host, pmt_quadratic_term *out, void *stream);
/* device-to-device copy on the stream (array-of-references copyto! nodes, src/lazyexpression.jl:280-282) */
int pmt_copy_bytes(void *dst, const void *src, size_t bytes, void *stream);

/* y = A * X with X::Vector{AffineFunction} of uniform length L:
 * row `row` = concat over col of A[row,col]*X[col].linear ; const = sum_col X.c[col]*A[row,col] (in col order).
 * matvecmul!(y, A, x::Vector{AffineFunction}) src/functions.jl:800-822 (muladd! :524 -> :515-523). */
int pmt_matvecmul_affs_f64(const double *A, int64_t lda, int64_t rows, int64_t cols,
                           const pmt_linear_term *x_terms, int64_t x_row_len, const double *x_consts,
                           pmt_linear_term *out_terms, double *out_consts, void *stream);

/* dot(v, x) family producing an AffineFunction (src/functions.jl:665-687):
 *   Number[] . Variable[]        -> out_terms[i] = (v[i], xvar[i]), const 0            (:676-687)
 *   Number[] . AffineFunction[]  -> concat_i v[i]*X[i].linear, const = sum_i X.c[i]*v[i] (:665-674, uniform L) */
int pmt_vecdot_numbers_vars_f64(const double *v, const int64_t *xvar, int64_t n,
                                pmt_linear_term *out_terms, double *out_const, void *stream);
int pmt_vecdot_numbers_affs_f64(const double *v, int64_t n,
                                const pmt_linear_term *x_terms, int64_t x_row_len, const double *x_consts,
                                pmt_linear_term *out_terms, double *out_const, void *stream);

/* ---------------------------------------------------------------------------------------
 * Quadratic nodes
 * ------------------------------------------------------------------------------------- */

/* dest = x . y for x, y ::Vector{AffineFunction} with uniform row lengths nx, ny (LITERAL expansion):
 *   quad[(i*nx + a)*ny + b] = (x[i].lin[a].coeff * y[i].lin[b].coeff, x[i].lin[a].var, y[i].lin[b].var)
 *   lin[i*(nx+ny) + a]      = (y.c[i] * x[i].lin[a].coeff, var)        a < nx
 *   lin[i*(nx+ny) + nx + b] = (x.c[i] * y[i].lin[b].coeff, var)        b < ny
 *   const = sum_i x.c[i]*y.c[i]  accumulated left to right
 * = _vecdot!(dest::QuadraticFunction, x, y) src/functions.jl:702-709 over muladd! :548-576.
 * moi != 0 fuses update!(::MOI.ScalarQuadraticFunction, f, varmap) src/moi_interop.jl:45-62:
 * indices go through varmap and coefficients with rowvar == colvar are doubled (:58). */
int pmt_quad_expand_f64(int64_t rows,
                        const pmt_linear_term *x_terms, int64_t nx, const double *x_consts,
                        const pmt_linear_term *y_terms, int64_t ny, const double *y_consts,
                        int moi, const int64_t *varmap,
                        pmt_quadratic_term *out_quad, pmt_linear_term *out_lin, double *out_const,
                        void *stream);

/* Canonical least-squares objective for residual = A*x (+|-) b:  canonicalize!(residual . residual)
 * (src/functions.jl:381-386 applied to the literal result above), then the MOI copy:
 *   out_quad[tri(j,k)] = (2 * sum_i A[i,j]*A[i,k], vm[xvar[j]], vm[xvar[k]])  for j <= k, row-major upper triangle
 *   out_lin[j]         = (2 * sum_i c_i*A[i,j], vm[xvar[j]])   with c_i = 0.0 (+|-) b[i]
 *   out_const          = sum_i c_i^2 in a FIXED order that (rows, cols) alone determine (pmt_quad_gram_constant_order below): the
 *                        reference's left-to-right sum (src/functions.jl:574, bit for bit), 2048 interleaved chains, or the fused
 *                        forms' per-workgroup order — every one within (rows / 2048 + 2048) * eps / 2 of the exact sum.
 * The node takes one of five forms, which (rows, cols) and the kind of call fix (csrc/gram.hip: gram_form): tiny shapes of a plain call
 * are nodes of the small-plan interpreter (csrc/small.hip); wide shapes of 129 .. 2048 columns by measured element counts, and 2049 .. 4096
 * columns below 2^29 elements (config 2) unless delivered, the one-launch form of csrc/gram_mid.hip; the rest of up to 2048 columns the
 * fused form of csrc/gram_tall.hip (the triangle of every diagonal 128-column tile, out_lin and out_const from ONE pass over A; the
 * strictly upper tiles from one stream-K launch); every other shape the stream-K node with the two reductions on a side stream, staged
 * for the `_deliver_` entry points (there, at 2049 .. 4096 columns, out_lin within 1e-13 of the plain call's and out_const in its order).
 * A is read as lda x cols doubles: a kernel may read (and ignore) the padding rows rows .. lda - 1 of a column, the last one included.
 * Requires xvar strictly increasing (distinct variables in sorted order — what Variable(model) yields);
 * moi == 0 keeps native indices (no varmap) but the same coefficients as the MOI form are NOT produced:
 *   native canonical form has diagonal coefficient (A'A)[j,j] and off-diagonal 2*(A'A)[j,k].
 * f64 MFMA contraction; `workspace` (device, pmt_quad_gram_workspace_bytes) holds split-K partial tiles and the chunk / chain sums.  It is
 * required: NULL is an ArgumentError (PMT_INVALID_ARGUMENT) wherever the fused or the one-launch form is taken, before anything runs. */
size_t pmt_quad_gram_workspace_bytes(int64_t rows, int64_t cols);
/* The summation order of the node's constant c'c for an r x n problem — fixed by (rows, cols) alone, reported so that a caller (and the
 * parity tests) can restate it:
 *   order 0  sequential, the reference's left-to-right sum (src/functions.jl:574), bit for bit: tiny shapes, and the stream-K node (beyond
 *            4096 columns or from 2^29 elements) where the contraction hides the one-wave chain
 *   order 1  `groups` = 2048 interleaved chains (chain t adds rows t, t + 2048, .. in order), chain totals added left to right: the stream-K
 *            node with rows > 8192, or a sequential chain that would take half as long as the contraction beside it or longer
 *   order 2  the fused forms (cols <= 2048; csrc/gram_tall.hip): `groups` workgroups, workgroup g takes the stages g, g + groups, .. of
 *            `stage_rows` rows; per stage eight row-pair lanes (rows 16 j + 2 p, + 1) add their squares in row order, an 8-lane tree
 *            ((0+4)+(2+6))+((1+5)+(3+7)) closes a workgroup, the workgroups are added in 16 interleaved slices, then the slices
 *   order 3  the same with SIXTEEN row-pair lanes (rows 32 j + 2 p, + 1; a 16-lane tree): the 16-column panel, cols <= 16
 *            (cols <= 64: below 32768 rows)
 *   order 4  narrow panels, cols <= 64, from 32768 rows (gram_stream_kernel): iterations of `stage_rows` rows dealt out to the 4 * `groups` WAVES (wave
 *            4 g + w: iterations 4 g + w, + 4 * groups, ..); contraction slot k of a wave adds rows 8 i + 2 k, + 1 of its iterations in order;
 *            slots (0 + 2) + (1 + 3); the four waves of a workgroup in order; workgroups in 16 interleaved slices, then the slices
 *   order 5  wide shapes in one launch (gram_mid.hip: 129 .. 4096 columns — from 384 columns everything below 2^29 elements, below 384 / 320 / 193
 *            columns up to 2^27 / 2^26 / 2^25; gram.hip: gram_mid_applies — config 2 since round 6c): `stage_rows` = 512 strided chains (thread
 *            t adds rows t, t + 512, ..), a shuffle tree (32, 16, .., 1) per 64 threads, the eight results in order
 * (tests/gpu_util.py restates every order bit for bit.)
 * Every order is within (rows / 2048 + 2048) * eps / 2 relative of the exact sum for same-signed terms: far inside the 1e-12 parity bar. */
int pmt_quad_gram_constant_order(int64_t rows, int64_t cols, int *order, int *groups, int *stage_rows);
/* Pure host query beside it: does the one-launch form of an undelivered plain call defer its tiles (gram_mid.hip: MidWalk — a finished
 * tile's sums and stores run inside the next tile's main loop)?  *plan: the shape runs the persistent walk over an unsplit body of at
 * least two tiles per workgroup, so tiles can be deferred; *whole_rounds (may be null): the row count (a multiple of 64) also gives every
 * wave whole rounds, so with 16-byte aligned operands and an even pitch the call runs the deferring build of the kernel and every body
 * tile of two whole 64-column panels but a workgroup's last IS deferred.  Both 0 for shapes of the other forms.
 * The results do not depend on it (the sums add the same operands level by level); tests use it to know which path they exercise. */
int pmt_quad_gram_mid_defers(int64_t rows, int64_t cols, int *plan, int *whole_rounds);
/* Pure host query beside it: does the one-launch form of an undelivered plain call run its first body tiles as STRIPS (gram_mid.hip:
 * mid_strips)?  *strips: how many — a strip is four consecutive strictly upper tiles of the walk, one WHOLE tile per wave of a workgroup,
 * so a coefficient of such a tile is ONE chain: the 8-row groups 0, 1, 2, .. of the matrix in MFMA k order (rows 2 k, 2 k + 1 of a group
 * in contraction slot k), with no wave level and no chunk level; *tiles_in_strips (may be null): 4 * *strips, the first ranks of the walk.
 * Every other tile, q and c'c are summed as they always were.  Non-zero only where the shape defers with whole rounds
 * (pmt_quad_gram_mid_defers), cols is a multiple of 64, there are at least 1.5 strips per workgroup AND the plan's cost estimate says
 * that strips in rounds of one per CU end sooner than single tiles (it says no where the strips would fill the last round badly: 4096 x
 * 3584 has 384 whole strips and takes none) — a shape that meets the first three conditions may still report 0; the call then runs the strip
 * build with 16-byte aligned operands and an even pitch (terms only), otherwise the kernels it ran before.  A function of (rows, cols)
 * alone, as the order is: repeated launches and concurrent streams give the same bits.  Both 0 for shapes of the other forms. */
int pmt_quad_gram_mid_strips(int64_t rows, int64_t cols, int *strips, int *tiles_in_strips);
int pmt_quad_gram_f64(const double *A, int64_t lda, int64_t rows, int64_t cols,
                      const int64_t *xvar, const double *b, int sign,
                      int moi, const int64_t *varmap,
                      pmt_quadratic_term *out_quad, pmt_linear_term *out_lin, double *out_const,
                      void *workspace, void *stream);
/* The same node with the solver hand-off fused into the epilogue (see "Solver hand-off" below): the values of P's upper
 * triangle in CSC order, out_P_values[k(k+1)/2 + j] = alpha * 2 * sum_i A[i,j]*A[i,k] (j <= k) — valid as the CSC value array
 * whenever j -> vm[xvar[j]] is strictly increasing (col_ptr[c] counts the variables below, row indices follow).  out_quad
 * (MOI terms, as above with moi = 1) is optional here: NULL skips the 24-byte term structs entirely.  out_lin / out_const as above.
 * The values equal the coefficients pmt_quad_gram_f64 writes for the same inputs bit for bit, except for TINY shapes (those the small-plan
 * interpreter takes: row-order sums there, the contraction's MFMA order here — equal to rounding; the constant is sequential in both). */
int pmt_quad_gram_csc_f64(const double *A, int64_t lda, int64_t rows, int64_t cols,
                          const int64_t *xvar, const double *b, int sign, const int64_t *varmap,
                          double alpha, double *out_P_values, pmt_quadratic_term *out_quad,
                          pmt_linear_term *out_lin, double *out_const, void *workspace, void *stream);

/* The same node (values only, no term structs) with the values additionally DELIVERED TO THE HOST while the contraction runs — the
 * reference's boundary is a host solver (MOI.set, src/moi_interop.jl:131-137; OSQP's update_P takes exactly this array).  host_P_values
 * is page-locked host memory (pmt_host_alloc) of cols*(cols+1)/2 doubles.  The contraction runs in STAGES over the column bands of P
 * (`ngroups` stages, 0 = default: half a grid's worth of 128 x 128 tiles per stage, at most 16), walked from the LAST band to the first (the
 * long bands leave while the contraction is still busy, the short ones are what is left at its end): each stage is a launch over all CUs
 * with its tiles split in two along the contraction — the two workgroups of a tile exchange halves through the workspace and each finishes
 * one row half (other stage sizes: a second launch adds the partial sums) — and the copy engine (HSA SDMA; a courier kernel where that is
 * not available) ships the bands a stage has completed while the next stage is computed, so P leaves at PCIe speed from the first stage on.
 * Splitting a tile changes its summation order (two half sums added): out_P_values here and from pmt_quad_gram_csc_f64 agree to rounding
 * (a few ulp), not bit for bit; both are deterministic, and host_P_values is out_P_values of the same call bit for bit.  `stream` does not
 * wait for the delivery: pmt_plan_fetch_synchronize (or pmt_fetch_synchronize for a plain stream) does — PMT_HIP_ERROR there if a transfer
 * never started (10 s; courier: no progress for 2 s); the next call on the same stream waits by itself until the previous delivery has
 * read out_P_values. */
int pmt_quad_gram_csc_deliver_f64(const double *A, int64_t lda, int64_t rows, int64_t cols,
                                  const int64_t *xvar, const double *b, int sign, const int64_t *varmap,
                                  double alpha, double *out_P_values, double *host_P_values, int ngroups,
                                  pmt_linear_term *out_lin, double *out_const, void *workspace, void *stream);
/* pmt_quad_gram_f64 with the QUADRATIC TERMS delivered to the host the same way — the reference's own boundary (MOI.set of the objective's
 * ScalarQuadraticFunction, src/moi_interop.jl:131-137): host_quad is page-locked memory for cols*(cols+1)/2 pmt_quadratic_term; the stages run
 * over tile ROW bands (the term array is row-major), each completed band range leaves while the next stage is computed.  Same remarks as above
 * (stages, summation order of split tiles, pmt_plan_fetch_synchronize / pmt_fetch_synchronize). */
int pmt_quad_gram_deliver_f64(const double *A, int64_t lda, int64_t rows, int64_t cols, const int64_t *xvar, const double *b, int sign,
                              int moi, const int64_t *varmap, pmt_quadratic_term *out_quad, pmt_quadratic_term *host_quad, int nstages,
                              pmt_linear_term *out_lin, double *out_const, void *workspace, void *stream);
/* A WEIGHTED SUM of least-squares blocks and simple terms over one Variable vector x (n = cols variables) as one canonical MOI function:
 * add! / mul! of quadratic functions (src/functions.jl:452-461 append the term lists, :578 scales them), canonicalize! (:381-386), then the
 * MOI copy (src/moi_interop.jl:45-62).  `terms` is a HOST array of `nterms` (1 .. PMT_LSQ_MAX_TERMS) descriptors in expression order:
 *   PMT_LSQ_BLOCK     dot(r_k, r_k), r_k = A_k*x (+|-) b_k.  The FIRST block is the function already in out_quad / out_lin / out_const
 *                     (pmt_quad_gram_f64, moi = 1, with the model's varmap); every later one gives `values` (its CSC values,
 *                     pmt_quad_gram_csc_f64 with alpha = 1), `lin` (its out_lin) and `constant` (its out_const).  1 .. 8 blocks.
 *   PMT_LSQ_DIAG      dot(x, x) (vec NULL) or dot(x (+|-) v, x (+|-) v) (vec = v, sign = +1 | -1)
 *   PMT_LSQ_LINEAR    dot(c, x) (vec = c)
 *   PMT_LSQ_CONSTANT  a scalar: *vec (a scalar Parameter), or 1.0 when vec is NULL (a number folded into `scale`)
 * Every term is weighted by W = scale * (*weight), or scale when weight is NULL (a scalar Parameter read on the device at run time).
 * In place, with every operation in the order written (no contraction into fma):
 *   quad[(j,k)].coeff = (((W_1*Q_1[j,k] + W_2*V_2[k(k+1)/2 + j]) + ..) + W_K*V_K[..]) + D*[j == k],   D = ((2*W_d1) + (2*W_d2)) + ..
 *                       over the diagonal terms (no D term without one); row / col stay as block 1 wrote them
 *   lin[j].coeff      = W_k*q_k[j] for each block, then W_d*(2*(0.0 (+|-) v_j)) for each diagonal term with v, then W_c*c_j for each
 *                       linear term
 *   const             = W_k*cc_k for each block, then W_d*S_d for each diagonal term with v, then W_s*(*vec or 1.0) for each constant;
 *                       S_d = sum_j v_j^2: 256 chains (chain t adds j = t, t + 256, .. in order), then a halving tree (t += t + 128, t + 64, ..)
 * Block 1 alone with the constant weight +1 (no weight pointer, scale 1.0) touches only the n diagonal terms, lin and the constant;
 * otherwise one 64 x 64 tile of the upper triangle per workgroup rewrites every term (csrc/gram_sum.hip).  Recorded into a plan behind
 * stream-K Gram nodes (whose constant is written at the end of the replay), the constant step is queued behind those constants.
 * For a binding author, said plainly:
 *   - Block 1 is the first PMT_LSQ_BLOCK of the list, at ANY index (lam*dot(x, x) + dot(r, r) puts it second): W_1 is that term's weight, the
 *     later blocks are the PMT_LSQ_BLOCK terms behind it, and the diagonal / linear / constant terms count wherever they stand, in front of
 *     it too.  Its `values`, `lin` and `constant` fields are never read.
 *   - A term that is absent contributes NOTHING: there is no `+ 0.0` for it.  Without a diagonal term no D is added, so a coefficient
 *     W_1*Q_1[j,j] = -0.0 stays -0.0; lin[j] and the constant likewise take only the terms that exist.
 *   - Block 1 alone at the constant weight +1 leaves every word it does not name as it is, bit for bit: the off-diagonal coefficients are not
 *     rewritten (not even multiplied by 1.0) and, without a diagonal term, neither are the diagonal ones. */
#define PMT_LSQ_BLOCK 1
#define PMT_LSQ_DIAG 2
#define PMT_LSQ_LINEAR 3
#define PMT_LSQ_CONSTANT 4
#define PMT_LSQ_MAX_TERMS 32
#define PMT_LSQ_MAX_BLOCKS 8
typedef struct {
    int32_t kind;                     /* PMT_LSQ_* */
    int32_t sign;                     /* PMT_LSQ_DIAG with vec: +1 for x + v, -1 for x - v */
    double scale;                     /* host factor of the weight */
    const double *weight;             /* device scalar factor of the weight, or NULL */
    const double *values;             /* PMT_LSQ_BLOCK after the first: CSC values of the block (cols*(cols+1)/2) */
    const pmt_linear_term *lin;       /* PMT_LSQ_BLOCK after the first: the block's linear terms (cols) */
    const double *constant;           /* PMT_LSQ_BLOCK after the first: the block's constant */
    const double *vec;                /* PMT_LSQ_DIAG: v or NULL; PMT_LSQ_LINEAR: c (cols); PMT_LSQ_CONSTANT: the scalar or NULL */
} pmt_lsq_term;
int pmt_quad_gram_sum_f64(int64_t cols, const pmt_lsq_term *terms, int nterms, pmt_quadratic_term *out_quad,
                          pmt_linear_term *out_lin, double *out_const, void *stream);
/* The same sum when PMT_LSQ_DIAG / PMT_LSQ_LINEAR terms cover only PART of the columns (dot(r, r) + lam*dot(u, u) with r stacked over
 * z = [x; u], pmt_affine_stack_columns_f64).  term_cols[t] (a HOST array of nterms pointers, or NULL for all terms) lists the device
 * positions term t covers: term_ncols[t] strictly increasing positions in 0 .. cols-1, read on the host at call time; NULL (the pointer
 * array or its entry t) means every column.  Blocks and constants cover every column (a list for them is an error).  The vec of a subset
 * term has one entry per listed position (term_ncols[t] entries; a list of 0 positions is allowed: such a term adds nothing to any coefficient,
 * a diagonal one with v still adds W_d*S_d = W_d*0.0 to the constant).  A position a term does not list gets nothing from it (no + 0.0: a -0.0 there stays -0.0, and in the diagonal-only form of
 * block 1 alone at weight +1 the diagonal coefficient of a position no diagonal term lists is not rewritten at all);
 * otherwise the order is the one fixed above for pmt_quad_gram_sum_f64, restricted to the listed positions:
 *   D_j = ((2*W_d1) + (2*W_d2)) + .. over the diagonal terms listing j (added only when one does); lin[j] takes the terms listing j in
 *   the order above; S_d is the chain-then-tree sum over the term's own vector.
 * The lists are held in the launch's arguments as runs of consecutive positions: at most PMT_LSQ_MAX_RUNS runs over all terms. */
#define PMT_LSQ_MAX_RUNS 64
int pmt_quad_gram_sum_sub_f64(int64_t cols, const pmt_lsq_term *terms, int nterms, const int64_t *const *term_cols, const int64_t *term_ncols,
                              pmt_quadratic_term *out_quad, pmt_linear_term *out_lin, double *out_const, void *stream);

/* transpose(x) * Q * x as its canonical function, for Q an n x n matrix (column-major, leading dimension ldq: the device layout of a
 * matrix Parameter) that need not be symmetric and x = n DISTINCT variables in strictly increasing order: bilinearmul! (src/functions.jl:840-858:
 * all n^2 terms (Q[j,k], x_j, x_k)), canonicalize! (:381-386: the two terms of every pair {j, k} added) and the MOI copy
 * (src/moi_interop.jl:45-62) in one pass.  An off-diagonal coefficient is the sum of exactly two numbers and IEEE addition commutes, so
 * the result is defined bit for bit, whatever order the reference's sort combines in (the builder's Q' pairing, :840-858, drops out
 * because Q + Q' is its own transpose):
 *   out_quad[tri(j,k)] = (Q[j,k] + Q[k,j], vm[xvar[j]], vm[xvar[k]]) for j < k, (2*Q[j,j], vm[xvar[j]], vm[xvar[j]]) on the diagonal, on the
 *                        row-major upper triangle (tri(j,k) = j*n - j*(j-1)/2 + k - j, 0-based: the positions pmt_quad_gram_f64 uses).
 *                        moi == 0: native indices (varmap not read) and Q[j,j] undoubled on the diagonal — what canonicalize! alone yields.
 *   out_P_values[k(k+1)/2 + j] = alpha * c(j,k), c the moi = 1 coefficient: the CSC layout and meaning of pmt_quad_gram_csc_f64.
 *                        With alpha == 1.0 the values equal the term coefficients bit for bit.
 *   out_lin[j] = (0.0, vm[xvar[j]]) and *out_const = 0.0 when given: with them the node's outputs stand wherever a least-squares block's
 *                        stand in pmt_quad_gram_sum_f64 / _sum_sub_f64 (first block: out_quad / out_lin / out_const; later: values / lin / constant).
 * At least one of out_quad / out_P_values; out_lin and out_const are optional.  A null Q or xvar, n < 1 (or beyond 2^21), ldq < n, moi != 0
 * without a varmap: PMT_INVALID_ARGUMENT before any device call.  No workspace.  Q is read as n columns of ldq doubles; padding rows are
 * never used.  One 64 x 64 tile of the upper triangle per workgroup: 8 n^2 bytes read, 24 / 8 / 32 bytes per entry written (csrc/form.hip). */
int pmt_quad_form_f64(const double *Q, int64_t ldq, int64_t n, const int64_t *xvar, int moi, const int64_t *varmap, double alpha,
                      pmt_quadratic_term *out_quad, double *out_P_values, pmt_linear_term *out_lin, double *out_const, void *stream);

/* The tracking cost transpose(x (+|-) v) * Q * (x (+|-) v) as its canonical function, for the Q and x of pmt_quad_form_f64 and v a vector of
 * n numbers: matvecmul! over the affine vector (src/functions.jl:800-822), vecdot! (:702-709 over :548-576: n^2 quadratic and n(n+1) linear
 * terms), canonicalize! (:381-386) and the MOI copy (src/moi_interop.jl:45-62) in one pass over Q and two short launches.  With
 * c_j = 0.0 + v_j (sign +1) or 0.0 - v_j (sign -1) — the constants of pmt_vars_addsub_f64 and of a PMT_LSQ_DIAG term — the function is
 * the plain form's quadratic part plus lin = (Q + Q')c and the constant c'Qc = 0.5 * c'lin:
 *   out_quad, out_P_values   word for word what pmt_quad_form_f64 writes for the same Q, xvar, moi, varmap and alpha.
 *   out_lin[j] = (lin_j, vm[xvar[j]]) (moi == 0: native indices), *out_const = the constant; the same in both index modes.
 * The arithmetic is fixed — plain multiplies and adds, no fma, independent of launch geometry, timing and streams:
 *   S[j,k]   = Q[j,k] + Q[k,j] for j != k (the rounded sum the quadratic term holds, bitwise symmetric), S[j,j] = 2*Q[j,j];
 *   P[B][j]  = ((S[j,k0]*c_k0 + S[j,k0+1]*c_{k0+1}) + ..) + S[j,k1]*c_k1 over column block B = columns k0 = 64 B .. k1 = min(64 B + 63, n-1),
 *              ascending, the first product starting the chain (no 0.0 +);
 *   lin_j    = ((P[0][j] + P[1][j]) + ..) + P[nb-1][j], nb = ceil(n / 64) blocks in order;
 *   constant = 0.5 * T, T = sum_j c_j*lin_j in S_d's order of pmt_quad_gram_sum_f64: 256 chains (chain t adds j = t, t + 256, .. in order
 *              onto 0.0), then the halving tree (t += t + 128, t + 64, ..).
 * The outputs stand wherever a least-squares block's stand in pmt_quad_gram_sum_f64 / _sum_sub_f64, like the plain form's.  `workspace`
 * (device, pmt_quad_form_shift_workspace_bytes(n) = 8 * (ceil(n/64) + 1) * n bytes, host arithmetic) holds P and, in its last row, the
 * products c_j*lin_j (written only when out_const is given); every entry is written once per call
 * before it is read, so it needs no zeroing.  At least one of out_quad / out_P_values; out_lin and out_const are optional.  A null Q, xvar,
 * v or workspace, a sign other than +-1, n < 1 (or beyond 2^21), ldq < n, moi != 0 without a varmap: PMT_INVALID_ARGUMENT before any device
 * call.  Three launches behind each other on the stream (csrc/form.hip): the tile kernel of the plain form, whose workgroup (J, K) also adds
 * the chains of its rows and, off the diagonal, of its columns from the S it holds in LDS; one thread per j adds the blocks, stores the
 * linear term and leaves c_j*lin_j; one workgroup adds those n products into the constant (only when out_const is given).  Stream order
 * alone orders them: no workgroup waits for another, no floating-point atomics. */
int64_t pmt_quad_form_shift_workspace_bytes(int64_t n);
int pmt_quad_form_shift_f64(const double *Q, int64_t ldq, int64_t n, const int64_t *xvar, const double *v, int sign, int moi,
                            const int64_t *varmap, double alpha, pmt_quadratic_term *out_quad, double *out_P_values,
                            pmt_linear_term *out_lin, double *out_const, void *workspace, void *stream);

/* A sum whose least-squares blocks and forms lie over 2 .. PMT_QUAD_MAX_GROUPS pairwise DISJOINT, strictly increasing Variable vectors
 * (transpose(x)*Q*x + transpose(u)*R*u; dot(r1, r1) + w*dot(r2, r2) with r1 over x and r2 over u) as one canonical MOI function.  No pair
 * (j, k) is shared between two groups, so canonicalize! (src/functions.jl:381-386) combines nothing across them.  With z the sorted union
 * of the groups' variables and n_g the size of group g, the function has sum_g n_g(n_g+1)/2 quadratic terms, sum_g n_g linear terms and
 * one constant:
 *   quadratic terms  rows in increasing model-variable index over z; row j of group g holds g's columns k >= j in increasing order — the
 *                    (row, col) order of canonicalize! on the literal function; indices through the varmap.  Every term equals, word for
 *                    word, the term pmt_quad_gram_sum_f64 / _sum_sub_f64 leaves for that group's term list alone (block 1 of the group by
 *                    pmt_quad_gram_f64 or pmt_quad_form_f64; a group of one block with weight 1: only its diagonal, linear terms and
 *                    constant are touched).
 *   linear terms     the groups' linear terms merged by increasing variable, word for word.
 *   constant         ((c_1 + c_2) + ..) + c_G over the groups' constants, groups in the order of the first appearance of one of their
 *                    blocks in the expression (scalar constants of the expression belong to group 1); no fma.
 * A group whose variables are consecutive in z owns one slice of out_quad / out_lin, and the entry points above write straight into it
 * (term offset: the terms of the rows before it; an odd offset is an address 8 mod 16, which every one of them takes).  Otherwise the
 * groups write into an arena of their own and pmt_quad_groups_gather_f64 places the rows:
 *   out_quad words row_dst[r] .. row_dst[r+1]-1 = src_quad words row_src[r] ..   for r = 0 .. nrows-1   (a term is three 8-byte words)
 *   out_lin[j] = src_lin[lin_src[j]]                                              for j = 0 .. nlin-1
 * row_src (nrows), row_dst (nrows + 1, increasing, row_dst[0] = 0, row_dst[nrows] = 3*nterms: every row holds at least one term) and
 * lin_src (nlin) are DEVICE tables built once; the call does no host work beyond the launch.  Source and destination segments may differ
 * in parity; out_quad needs 8-byte alignment only; nothing outside the nterms / nlin terms is written.  HBM-bound: 48 bytes per
 * quadratic term.  A negative size or nterms < nrows: PMT_DIMENSION_MISMATCH; a null table or array that a non-zero size needs:
 * PMT_INVALID_ARGUMENT — before any device call (csrc/groups.hip). */
#define PMT_QUAD_MAX_GROUPS 8
int pmt_quad_groups_gather_f64(const pmt_quadratic_term *src_quad, const int64_t *row_src, const int64_t *row_dst, int64_t nrows,
                               int64_t nterms, const pmt_linear_term *src_lin, const int64_t *lin_src, int64_t nlin,
                               pmt_quadratic_term *out_quad, pmt_linear_term *out_lin, void *stream);
/* *out_const = ((group_consts[0] + group_consts[1]) + ..) + group_consts[ngroups-1] (device doubles; out_const may be group_consts[0]).
 * Queued behind the groups' own constant steps; in a plan's replay behind deferred stream-K constants, exactly as the constant step of
 * pmt_quad_gram_sum_f64.  ngroups outside 1 .. PMT_QUAD_MAX_GROUPS or a null pointer: PMT_INVALID_ARGUMENT before any device call. */
int pmt_quad_groups_constant_f64(const double *group_consts, int ngroups, double *out_const, void *stream);

/* host: block until every copy on the fetch stream of `stream` (a HIP stream, not a recording handle) has landed.  PMT_HIP_ERROR when a
 * delivery failed on the device: a transfer that never started, a courier without progress, or a split tile of a staged contraction whose
 * first half never arrived (the tile is then NaN in out_P_values / out_quad — never a plausible half sum — and this call says so). */
int pmt_fetch_synchronize(void *stream);

/* How results leave for the host (recorded fetches, the deliveries above), process-wide, from the next replay / call on:
 *   0  automatic (default): the copy engine (HSA SDMA transfers started by signals the kernels set) when the process's HSA runtime and the
 *      device's agent are found — matched by PCI domain:bus:device, an ambiguous match counts as none — kernel copies otherwise;
 *   1  the copy engine or PMT_STATE_ERROR (a deployment that must not fall back silently);
 *   2  kernel copies (a courier kernel for deliveries, copy kernels for recorded fetches) on the stream's fetch stream.
 * Same bytes in the host arrays either way.  pmt_get_host_delivery reports the mode and whether `device` has a usable copy engine. */
int pmt_set_host_delivery(int mode);
int pmt_get_host_delivery(int device, int *out_mode, int *out_copy_engine);
/* TEST HOOK (fault injection; 0 = off, the default).  1: in a staged contraction the first halves of split tiles never announce
 * themselves, and the second halves' bounded wait is cut from 2 s to 20 ms — exercises the error path of pmt_fetch_synchronize above.
 * 2: the grid barriers of a small plan's run on several workgroups wait (20 ms) for an arrival that never comes: pmt_plan_synchronize
 * returns PMT_HIP_ERROR for that re-evaluation.  4: every run on several workgroups is launched on ONE (the path a plan takes while another
 * plan's multi-workgroup run is in flight on the device).  Bits combine. */
int pmt_set_fault_injection(int what);

/* dest = transpose(x) * Q * y:  quad[k] = (Q[k] (column-major linear index), x[k / ny], y[k % ny])
 * bilinearmul! src/functions.jl:840-858 (the Q' pairing quirk is reproduced).
 * The linear index k is that of the rows x cols matrix; ldq is the leading dimension of its device copy.  moi as above. */
int pmt_bilinear_f64(const double *Q, int64_t ldq, int64_t rows, int64_t cols, const int64_t *xvar, const int64_t *yvar,
                     int moi, const int64_t *varmap, pmt_quadratic_term *out_quad, void *stream);

/* x . y for Variable/LinearTerm vectors: quad[i] = (xc[i]*yc[i], xvar[i], yvar[i]); xc/yc NULL = Variables (coeff 1)
 * _vecdot! src/functions.jl:689-700. */
int pmt_vecdot_terms_f64(int64_t n, const double *xc, const int64_t *xvar, const double *yc, const int64_t *yvar,
                         int moi, const int64_t *varmap, pmt_quadratic_term *out_quad, void *stream);

/* AffineFunction[] . Variable[] (uniform row length L):
 *   quad[i*L + a] = (x[i].lin[a].coeff, x[i].lin[a].var, yvar[i]) ; lin[i] = (x.c[i], yvar[i])
 * _vecdot! :702-709 over muladd!(dest, ::AffineFunction, ::Variable) src/functions.jl:537-546. */
int pmt_vecdot_affs_vars_f64(int64_t rows, const pmt_linear_term *x_terms, int64_t L, const double *x_consts,
                             const int64_t *yvar, int moi, const int64_t *varmap,
                             pmt_quadratic_term *out_quad, pmt_linear_term *out_lin, void *stream);

/* ---------------------------------------------------------------------------------------
 * MOI copies of materialised native functions — update!(moi_f, f, varmap) src/moi_interop.jl:35-81
 * ------------------------------------------------------------------------------------- */
int pmt_pack_scalar_affine_f64(const pmt_linear_term *terms, int64_t n, const int64_t *varmap,
                               pmt_linear_term *out_terms, void *stream);                       /* :35-43 */
int pmt_pack_scalar_quadratic_f64(const pmt_quadratic_term *quad, int64_t nq, const int64_t *varmap,
                                  pmt_quadratic_term *out_quad, void *stream);                  /* :53-60 (diag x2) */
int pmt_pack_vector_affine_f64(const pmt_linear_term *terms, const int64_t *row_ptr, int64_t rows, int64_t row_len,
                               const int64_t *varmap, int64_t row_offset,
                               pmt_vector_affine_term *out_terms, void *stream);                /* :64-81 */

/* ---------------------------------------------------------------------------------------
 * Generic canonicalize! (src/functions.jl:269-272, 381-386; sort_and_combine! src/util.jl:9-26) for arbitrary term lists.
 * Indices are static on this path, so the sort happens once on the host (pmt_canonical_order_*: permutation by canonical key,
 * run boundaries seg_ptr[nseg+1], and the indices of the combined terms — a run of one keeps its original (row, col), util.jl:18-19);
 * per re-evaluation pmt_segment_sum_f64 adds the coefficients of each run (duplicates in original order; the reference's order is
 * that of its unstable QuickSort, so coefficients agree to rounding) and writes ONLY the coefficient field (offset 0) of each
 * output term, whose index fields the host wrote when the node was created.
 * ------------------------------------------------------------------------------------- */
int pmt_canonical_order_affine(int64_t n, const int64_t *host_vars, int64_t *host_perm, int64_t *host_seg_ptr, int64_t *host_out_vars,
                               int64_t *nseg);
int pmt_canonical_order_quadratic(int64_t n, const int64_t *host_rows, const int64_t *host_cols, int64_t *host_perm, int64_t *host_seg_ptr,
                                  int64_t *host_out_rows, int64_t *host_out_cols, int64_t *nseg);
int pmt_segment_sum_f64(const void *in_terms, int64_t in_stride_bytes, const int64_t *perm, const int64_t *seg_ptr, int64_t nseg,
                        void *out_terms, int64_t out_stride_bytes, void *stream);
/* The same ordering computed ON THE DEVICE from the term buffer where it lies (no copy of the indices to the host, no single-threaded
 * sort): a stable radix sort by the packed canonical key, the run boundaries by stream compaction.  perm: int64[n], seg_ptr: int64[n + 1],
 * both device; *nseg_host receives the number of distinct terms (the only bytes that cross PCIe — the host sizes the output from them).
 * Setup-time call on a HIP stream (synchronises).  PMT_INVALID_ARGUMENT when an index does not fit the packed key (>= 2^32): use the
 * host functions above.  pmt_canonical_init_terms then writes the static part of the canonical function, out_terms[s] = (0.0, indices of
 * run s), with the reference's conventions (a run of one keeps its original (row, col), util.jl:18-19). */
int pmt_canonical_order_device(const void *terms, int64_t n, int term_bytes, int64_t *perm, int64_t *seg_ptr, int64_t *nseg_host, void *stream);
int pmt_canonical_init_terms(const void *terms, int term_bytes, const int64_t *perm, const int64_t *seg_ptr, int64_t nseg, void *out_terms, void *stream);

/* prune_zero!(f; atol) (src/functions.jl:294-297, 409-413): out_terms = the terms with abs(coeff) > atol, in order; *out_count (DEVICE
 * memory) = how many.  term_bytes: 16 (pmt_linear_term) or 24 (pmt_quadratic_term).  Not on the solve path: the count is data
 * dependent, the caller synchronises before using it.  NOTE the reference's quirk: prune_zero!(::QuadraticFunction; atol) prunes the
 * affine part with the DEFAULT atol (0), :410 — callers that mirror it pass atol only for the quadratic terms. */
size_t pmt_prune_zero_workspace_bytes(int64_t n, int term_bytes);
int pmt_prune_zero_f64(const void *terms, int64_t n, int term_bytes, double atol, void *out_terms, int64_t *out_count,
                       void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Solver hand-off: what happens AFTER MOI.set(optimizer, ...) (src/moi_interop.jl:134,171) — in the
 * reference third-party code (MathOptInterface 0.8 + the OSQP wrapper) on the host.  Here the MOI buffers stay in HBM and
 *     minimize 1/2 x'Px + q'x   subject to   l <= Ax <= u      (P upper triangular; P, A in CSC with 0-based Int64 indices)
 * is rebuilt on the device: the CSC structure depends only on the static indices (pmt_csc_order, host, once), the values are
 * per-run sums of MOI coefficients (pmt_csc_values_f64, per re-evaluation), the bounds come from the constants and the set.
 *   pmt_csc_order: rows/cols are the 1-BASED optimizer indices as they stand in the MOI terms; `upper` folds (i,j) onto
 *     (min,max) (ScalarQuadraticTerm: Q_ij = Q_ji).  Outputs: perm[nnz_in] (terms sorted by column, then row, stable), seg_ptr[nnz_out+1]
 *     (runs of equal (row, col)), col_ptr[ncols+1], row_idx[nnz_out] (0-based), *nnz_out.  Arrays sized for nnz_in suffice.
 *   pmt_csc_values_f64: dst[dst_index ? dst_index[s] : s] = alpha * sum_{p in run s} coeff(perm[p]); src_coeff points at the
 *     coefficient field of term 0 (offset 0 for linear/quadratic terms, 8 for pmt_vector_affine_term), stride = sizeof(term).
 *     dst_index places a block's entries inside a larger matrix (several constraint blocks stacked) or scatters q.
 *   pmt_qp_bounds_f64: row i of `f(x) in set`, f = a'x + c:  l = u = v - c (EQUAL) | l = v - c, u = +infty (GREATER) | l = -infty, u = v - c (LESS).
 * ------------------------------------------------------------------------------------- */
enum { PMT_SET_EQUAL = 0, PMT_SET_GREATER = 1, PMT_SET_LESS = 2 };
int pmt_csc_order(int64_t nnz_in, const int64_t *host_rows, const int64_t *host_cols, int64_t nrows, int64_t ncols, int upper,
                  int64_t *host_perm, int64_t *host_seg_ptr, int64_t *host_col_ptr, int64_t *host_row_idx, int64_t *nnz_out);
int pmt_csc_values_f64(const void *src_coeff, int64_t src_stride_bytes, int64_t nnz_in, const int64_t *perm, const int64_t *seg_ptr,
                       int64_t nnz_out, double alpha, const int64_t *dst_index, double *dst_values, void *stream);
int pmt_qp_bounds_f64(const double *consts, int64_t rows, int set_kind, double set_value, double infty, double *l, double *u,
                      void *stream);
/* Several term buffers feeding one matrix / several constraint blocks in ONE launch each (a model with k constraint blocks otherwise
 * pays 2k small kernels and their in-stream gaps per re-evaluation):
 *   pmt_csc_values_gather_f64: as pmt_csc_values_f64 with term_ptr[p] = device address of the coefficient of the p-th term in CSC order
 *     (the caller folds base pointer, stride and permutation of every block into it, once);
 *   pmt_qp_bounds_rows_f64: row i reads its constant through const_ptr[i] and has its own set kind / value. */
int pmt_csc_values_gather_f64(const double *const *term_ptr, int64_t nnz_in, const int64_t *seg_ptr, int64_t nnz_out, double alpha,
                              const int64_t *dst_index, double *dst_values, void *stream);
/* A DENSE block of a solver matrix: column j of dst (dst + j*dst_pitch doubles) takes the `rows` doubles of column j of src
 * (src + j*src_pitch) — the CSC values of a dense constraint block C*x (+|-) d are the Parameter matrix C itself, column by column,
 * placed at the block's row range of every column of the stacked matrix.  dst_offset != NULL: column j goes to dst + dst_offset[j]
 * instead (the other blocks do not have the same height in every column).  No term structs are read. */
int pmt_copy_2d_f64(const double *src, int64_t src_pitch, double *dst, int64_t dst_pitch, const int64_t *dst_offset, int64_t rows,
                    int64_t cols, void *stream);
int pmt_qp_bounds_rows_f64(const double *const *const_ptr, const int *set_kind, const double *set_value, int64_t rows, double infty,
                           double *l, double *u, void *stream);

/* ---------------------------------------------------------------------------------------
 * Sparse constraint matrix (BASELINE config 5): C given in CSC (Julia SparseMatrixCSC: colptr/rowval
 * 1-based Int64, nzval).  The reference has no sparse path — matvecmul!(y, A::AbstractMatrix, x) src/functions.jl:775-798 walks every
 * (row, col) — so the output here is the reference's output minus the structural zeros.  pmt_sparse_rowmajor_order computes ONCE the
 * row-major order of the structural non-zeros; per re-evaluation pmt_sparse_pack_vector_f64 gathers nzval through it into
 * MOI.VectorAffineTerms (update! src/moi_interop.jl:64-81; row-major, columns ascending within a row = matvecmul!'s order).
 * ------------------------------------------------------------------------------------- */
/* host-side helper: perm[t] = index into nzval of the t-th term in row-major order, rows_out[t], cols_out[t] (1-based) */
int pmt_sparse_rowmajor_order(int64_t m, int64_t n, const int64_t *host_colptr, const int64_t *host_rowval,
                              int64_t *host_perm, int64_t *host_rows, int64_t *host_cols, int64_t *host_row_ptr);
int pmt_sparse_pack_vector_f64(const double *nzval, const int64_t *perm, const int64_t *term_row, const int64_t *term_var,
                               int64_t nnz, const int64_t *varmap, int64_t row_offset,
                               pmt_vector_affine_term *out_terms, void *stream);
/* native form of the same node (Vector{AffineFunction} with ragged rows): out[t] = (nzval[perm[t]], term_var[t]) */
int pmt_sparse_assemble_f64(const double *nzval, const int64_t *perm, const int64_t *term_var, int64_t nnz,
                            pmt_linear_term *out_terms, void *stream);
/* XCD-aware form of the two entry points above (same outputs, bit for bit): columns are cut into `nslab` slabs, workgroup b works on
 * slab b % nslab, so with nslab = 8 (the XCD count) each XCD's L2 only sees one eighth of nzval.  slab_ptr[row*(nslab+1) + s] = index of
 * the first term of `row` whose column is in slab s (host helper, once per pattern; term_col from pmt_sparse_rowmajor_order). */
int pmt_sparse_slab_ptr(int64_t rows, int64_t cols, int nslab, const int64_t *host_row_ptr, const int64_t *host_term_col,
                        int64_t *host_slab_ptr);
int pmt_sparse_pack_vector_slabs_f64(const double *nzval, const int64_t *perm, const int64_t *term_var, const int64_t *slab_ptr,
                                     int64_t rows, int nslab, const int64_t *varmap, int64_t row_offset,
                                     pmt_vector_affine_term *out_terms, void *stream);
int pmt_sparse_assemble_slabs_f64(const double *nzval, const int64_t *perm, const int64_t *term_var, const int64_t *slab_ptr,
                                  int64_t rows, int nslab, pmt_linear_term *out_terms, void *stream);
/* the same two entry points with 32-bit perm / term_var (same values; half the index stream).  Usable when nnz and every variable index
 * (after varmap, if the caller folds it in — see below) are below 2^32.
 * Folding varmap in: pass term_var[t] = varmap[x-variable of term t] and varmap = NULL; the per-term varmap gather disappears (the map
 * only changes when the optimizer's index map does, src/model.jl:100-107, not per re-evaluation). */
int pmt_sparse_pack_vector_slabs_u32_f64(const double *nzval, const uint32_t *perm, const uint32_t *term_var, const int64_t *slab_ptr,
                                         int64_t rows, int nslab, const int64_t *varmap, int64_t row_offset,
                                         pmt_vector_affine_term *out_terms, void *stream);
int pmt_sparse_assemble_slabs_u32_f64(const double *nzval, const uint32_t *perm, const uint32_t *term_var, const int64_t *slab_ptr,
                                      int64_t rows, int nslab, pmt_linear_term *out_terms, void *stream);

/* Block form of the same two nodes (same outputs, bit for bit): the matrix is cut into blocks of 128 rows x `cw` columns; a workgroup reads
 * the coefficients of its block with coalesced loads (the rows of a CSC column ascend, so a column's part of a block is one contiguous run
 * of nzval) into LDS and writes each row's terms of the column band from there.  No per-term gather from HBM / L2 and a 4-byte instead of
 * an 8-byte static index per term: 36 bytes per non-zero.  The variable word of a term comes from the per-COLUMN array col_var[cols]
 * (x[col]; with `varmap` non-null varmap[col_var[col] - 1] as in moi_interop.jl:64-81).  out_consts (optional) = 0.0 (+|-) d[row], the
 * constants of C*x (+|-) d, written by the same launch (d may be NULL with sign 0: zeros).
 * Host helpers, once per pattern:
 *   pmt_sparse_blocks_width  -> *out_cw = the widest band width (power of two, 32..1024) whose blocks all fit the kernel's LDS buffer,
 *                               or 0 when the form does not apply (rows not ascending within a column, 2^32 or more non-zeros, empty matrix):
 *                               use the slab form then;
 *   pmt_sparse_blocks_build  -> desc[ceil(m/128) * n] (8 bytes per (row block, column)), idx[nnz] (4 bytes per term, row-major order),
 *                               band_ptr[m * (ceil(n/cw) + 1)]; perm / term_col / row_ptr from pmt_sparse_rowmajor_order. */
int pmt_sparse_blocks_width(int64_t m, int64_t n, const int64_t *host_colptr, const int64_t *host_rowval, int *out_cw);
int pmt_sparse_blocks_build(int64_t m, int64_t n, const int64_t *host_colptr, const int64_t *host_rowval, const int64_t *host_perm,
                            const int64_t *host_term_col, const int64_t *host_row_ptr, int cw, uint64_t *host_desc, uint32_t *host_idx,
                            int64_t *host_band_ptr);
int pmt_sparse_pack_vector_blocks_f64(const double *nzval, const uint64_t *desc, const uint32_t *idx, const int64_t *band_ptr,
                                      const int64_t *col_var, int64_t rows, int64_t cols, int64_t nnz, int cw, const int64_t *varmap,
                                      int64_t row_offset, const double *d, int sign, pmt_vector_affine_term *out_terms,
                                      double *out_consts, void *stream);
int pmt_sparse_assemble_blocks_f64(const double *nzval, const uint64_t *desc, const uint32_t *idx, const int64_t *band_ptr,
                                   const int64_t *col_var, int64_t rows, int64_t cols, int64_t nnz, int cw, const double *d, int sign,
                                   pmt_linear_term *out_terms, double *out_consts, void *stream);
/* constants of the same node: out[i] = 0.0 (+|-) d[i]  (vecadd!/vecsubtract! on zero!'d functions, src/functions.jl:244,452,474) */
int pmt_consts_f64(const double *d, int64_t n, int sign, double *out, void *stream);

/* Sparse least-squares objective: dot(r, r), r = C*x (+|-) d with C the fixed-pattern CSC matrix above, as the canonical MOI function —
 * vecdot! (src/functions.jl:702-709 over :548-576) of rows holding the STRUCTURAL terms only (the reference's output minus the structural
 * zeros, as for the constraint node), canonicalize! (:381-386), the MOI copy (src/moi_interop.jl:45-62).  With c_i = 0.0 (+|-) d[i]:
 *   out_quad[s] = (2 * sum_i C[i,j]*C[i,k], vm[xvar[j]], vm[xvar[k]])  one term per pair of columns j <= k that share at least one row,
 *                 sorted by (j, k), the sum over the shared rows (diagonal included, as for pmt_quad_gram_f64); nq terms
 *   out_lin[l]  = (2 * sum_i C[i,j]*c_i, vm[xvar[j]])                  one term per NON-EMPTY column j = lin_col[l]; without d the
 *                 coefficients are sums of C[i,j]*0.0 — zeros — and the terms still exist
 *   out_const   = sum_i c_i^2 over all `rows` rows (0.0 without d)
 * moi == 0: native indices (no varmap) and the diagonal coefficients undoubled, as in pmt_quad_gram_f64.  The whole 24- and 16-byte structs
 * are written at every call.  Requires a canonical pattern (rows strictly ascending within a column), xvar strictly increasing, fewer than
 * 2^32 non-zeros and fewer than 2^31 products.
 * Symbolic phase, host, once per pattern (colptr / rowval 1-based as above; linear in nprod + nnz + m + n, no comparison sort):
 *   pmt_sparse_gram_count -> nq and nprod = sum over the rows of L(L+1)/2, L the row's length (nprod >= 2^31: nq = -1, not counted)
 *   pmt_sparse_gram_order -> pair_j[nq], pair_k[nq] (0-based column positions, sorted by (j, k)); seg_ptr[nq+1]; prod[nprod] of
 *                            { uint32 ta, uint32 tb }: positions in nzval, ta in column j, tb in column k, within a segment in ascending
 *                            row order; lin_col[*nlin] (capacity n): the non-empty columns.  nq / nprod are those of _count.
 *   pmt_sparse_gram_runs  -> how one launch is cut: runs[2r], runs[2r+1] = the first and one past the last segment of workgroup run r —
 *                            whole segments of fewer than 64 products, at most `cap` (64 .. 2048) products together — and long_seg[]: the
 *                            segments of 64 products or more.  runs / long_seg NULL: the counts only.
 *   a 0-based colptr is PMT_INVALID_ARGUMENT, an out-of-range row PMT_DIMENSION_MISMATCH, rows that do not ascend PMT_INVALID_ARGUMENT.
 * The arithmetic is part of this contract and does not depend on the runs (no fused multiply-add anywhere):
 *   product        p = nzval[ta]*nzval[tb]                        (linear terms: nzval[t]*c_i over column j's entries in CSC order)
 *   short segment  (fewer than 64 products)  acc = p_0; acc += p_1; ..  left to right; the coefficient is 2.0*acc
 *   long segment   every lane of 64 starts at 0.0, lane l adds products l, l + 64, .. in order, then the __shfl_down tree over
 *                  32, 16, .., 1 (the one-wave order of pmt_csc_values_f64's long runs); the coefficient is 2.0*total
 *   constant       256 chains (chain t adds rows t, t + 256, .. in order), then the halving tree — S_d's order in pmt_quad_gram_sum_f64
 * Per call: the kernels stream the product list (8 bytes per product), gather the two values from nzval and add every segment's products
 * from LDS; no floating-point atomics.  The linear terms are cut the same way: lin_seg[l] (nlin + 1 entries, 0-based) is the position in nzval
 * of the first entry of column lin_col[l] (the last entry: nnz) — the non-empty columns lie back to back in CSC storage —, rowidx0 (nnz,
 * 0-based) the entries' rows, lin_runs / lin_long the runs and long segments pmt_sparse_gram_runs makes of lin_seg.  Null pointers,
 * negative counts and moi without varmap are PMT_INVALID_ARGUMENT before any device call. */
int pmt_sparse_gram_count(int64_t m, int64_t n, const int64_t *host_colptr, const int64_t *host_rowval, int64_t *nq, int64_t *nprod);
int pmt_sparse_gram_order(int64_t m, int64_t n, const int64_t *host_colptr, const int64_t *host_rowval, int64_t nq, int64_t nprod,
                          uint32_t *host_pair_j, uint32_t *host_pair_k, int64_t *host_seg_ptr, void *host_prod, uint32_t *host_lin_col,
                          int64_t *nlin);
int pmt_sparse_gram_runs(const int64_t *host_seg_ptr, int64_t nq, int64_t cap, int64_t *host_runs, int64_t *nruns, int64_t *host_long_seg,
                         int64_t *nlong);
int pmt_sparse_gram_f64(const double *nzval, const void *prod, const int64_t *seg_ptr, const uint32_t *pair_j, const uint32_t *pair_k,
                        int64_t nq, const int64_t *runs, int64_t nruns, const int64_t *long_seg, int64_t nlong,
                        const int64_t *lin_seg, const uint32_t *rowidx0, const uint32_t *lin_col, int64_t nlin, const int64_t *lin_runs,
                        int64_t nlin_runs, const int64_t *lin_long, int64_t nlin_long, int64_t rows, const int64_t *xvar, const double *d,
                        int sign, int moi, const int64_t *varmap, pmt_quadratic_term *out_quad, pmt_linear_term *out_lin, double *out_const,
                        void *stream);

/* A WEIGHTED SUM over sparse least-squares blocks and simple terms over one strictly increasing Variable vector x (n columns) as one
 * canonical MOI function: dot(r, r) + lam*dot(x, x), w1*dot(r1, r1) + w2*dot(r2, r2), dot(r, r) + dot(c, x) + s, 2.0*dot(r, r) ..  The
 * function is the reference's literal function (add! / mul! of the terms' functions, src/functions.jl:452-461, :578) minus the structural
 * zeros, canonicalize!d (:381-386), then the MOI copy (src/moi_interop.jl:45-62).  `terms` is a HOST array of `nterms`
 * (1 .. PMT_LSQ_MAX_TERMS) pmt_sparse_lsq_term descriptors in expression order, of the kinds of pmt_lsq_term:
 *   PMT_LSQ_BLOCK     dot(r_b, r_b), r_b = C_b*x (+|-) d_b, C_b sparse: `quad`, `lin`, `constant` are the block's MOI-form outputs of
 *                     pmt_sparse_gram_f64 (moi = 1, the same varmap: coefficients already doubled), left in scratch lists of the block's
 *                     own nq_b / nlin_b terms; `quad_at` / `lin_at` its gather tables (below).  1 .. PMT_LSQ_MAX_BLOCKS blocks; patterns and
 *                     row counts may differ between blocks.
 *   PMT_LSQ_DIAG      dot(x, x) (vec NULL, sign 0) or dot(x (+|-) v, x (+|-) v) (vec = v, sign = +1 | -1)
 *   PMT_LSQ_LINEAR    dot(c, x) (vec = c)
 *   PMT_LSQ_CONSTANT  a scalar: *vec (a scalar Parameter), or 1.0 when vec is NULL (a number folded into `scale`)
 * A diagonal or linear term lies over all of x (`pos` NULL, nvec = n) or over a strictly increasing part of it: `pos` is then a device
 * table over the positions 0 .. n-1 giving the index into the term's vector (nvec entries), or -1 for a position the term does not list.
 * Every term is weighted by W = scale * (*weight), or scale when weight is NULL.
 * STRUCTURE (from the patterns alone; terms exist even when a coefficient is 0.0, as in the bare node):
 *   quadratic pairs   the sorted union, by (j, k) with j <= k, of the blocks' pair sets and of (j, j) for every position j that some
 *                     diagonal term lists
 *   linear columns    the sorted union of the blocks' non-empty columns, the positions listed by diagonal terms with a v, and the positions
 *                     listed by linear terms
 * COEFFICIENTS, every operation in the order written, no contraction into fma; a position or pair a term does not hold gets nothing from
 * it (no + 0.0), the first contributor starts the chain (no 0.0 +):
 *   quad[(j,k)]  W_b*Q_b[(j,k)] over the blocks holding the pair, in block order (c = c + W_b*Q_b); on the diagonal, when a diagonal term
 *                lists j, then + D_j,  D_j = ((2*W_d1) + (2*W_d2)) + .. over the diagonal terms that list j, in order; D_j alone when no
 *                block holds the pair
 *   lin[j]       W_b*L_b[j] over the blocks that have column j, in block order; then + W_t*(2*(0.0 (+|-) v[p])) over the diagonal terms
 *                with v that list j, in order; then + W_t*c[p] over the linear terms that list j, in order
 *   constant     W_b*cc_b in block order; then W_t*S_t for every diagonal term with v, S_t the sum of v^2 over the term's own vector: 256
 *                chains (chain t adds entries t, t + 256, .. in order), then the halving tree — S_d's order in pmt_quad_gram_sum_f64; then
 *                W_t*(*vec or 1.0) for the scalar constants, in expression order
 * The row, column and variable words go through varmap at every call, and the whole 24- or 16-byte struct is written every time, every
 * output term exactly once: the output may be host-visible memory.  One launch (csrc/sparse_gram_sum.hip): workgroup 0 the constant, then
 * one workgroup per PMT_SPARSE_SUM_WG_TERMS output quadratic terms (the structs go through LDS and leave as 16-byte stores per wave; an
 * output base that is 8 mod 16 is fine), then one per PMT_SPARSE_SUM_WG_TERMS output linear terms.
 * SYMBOLIC PHASE, host, once per term list: pmt_sparse_gram_sum_merge merges the blocks' sorted lists (pair_j[b], pair_k[b], nq[b] and
 * lin_col[b], nlin[b] of pmt_sparse_gram_order, HOST arrays of `nblocks` pointers / counts in block order) with the column lists of the
 * diagonal and linear terms — term_kind[t] (PMT_LSQ_*), term_has_vec[t] (a diagonal term's v), term_cols[t] / term_ncols[t] as in
 * pmt_quad_gram_sum_sub_f64 (NULL: all of x) for each of the nterms terms in expression order; the blocks among them number nblocks.
 * Linear in the input (the lists are sorted: each output pair looks at the at most nine list heads, no comparison sort).  With every output array
 * NULL it returns the counts *out_nq / *out_nlin only; otherwise it also writes out_pair_j / out_pair_k (out_nq entries), out_lin_col
 * (out_nlin), per block quad_at[b] (out_nq entries: the index of the output pair in the block's own list, or 0xFFFFFFFF when the block
 * has no such pair) and lin_at[b] (out_nlin entries, likewise), and per term with a column list term_pos[t] (n entries of int32: the `pos`
 * table above).  Unsorted lists are PMT_INVALID_ARGUMENT, positions outside 0 .. n-1 PMT_DIMENSION_MISMATCH, nblocks outside
 * 1 .. PMT_LSQ_MAX_BLOCKS or nterms outside 1 .. PMT_LSQ_MAX_TERMS PMT_INVALID_ARGUMENT — all checked before anything is written.
 * pmt_sparse_gram_sum_f64 rejects null pointers, negative counts, bad signs and term / block counts out of range before any device call. */
#define PMT_SPARSE_SUM_WG_TERMS 256
typedef struct {
    int32_t kind;                     /* PMT_LSQ_* */
    int32_t sign;                     /* PMT_LSQ_DIAG with vec: +1 for x + v, -1 for x - v; otherwise 0 */
    double scale;                     /* host factor of the weight */
    const double *weight;             /* device scalar factor of the weight, or NULL */
    const pmt_quadratic_term *quad;   /* PMT_LSQ_BLOCK: the block's quadratic terms (nq_b) */
    const pmt_linear_term *lin;       /* PMT_LSQ_BLOCK: the block's linear terms (nlin_b) */
    const double *constant;           /* PMT_LSQ_BLOCK: the block's constant */
    const uint32_t *quad_at;          /* PMT_LSQ_BLOCK: per output quadratic term, its index in `quad` or 0xFFFFFFFF */
    const uint32_t *lin_at;           /* PMT_LSQ_BLOCK: per output linear term, its index in `lin` or 0xFFFFFFFF */
    const double *vec;                /* PMT_LSQ_DIAG: v or NULL; PMT_LSQ_LINEAR: c; PMT_LSQ_CONSTANT: the scalar or NULL */
    const int32_t *pos;               /* PMT_LSQ_DIAG / PMT_LSQ_LINEAR over part of x: per position its index in vec or -1; NULL: all of x */
    int64_t nvec;                     /* PMT_LSQ_DIAG / PMT_LSQ_LINEAR: the number of positions the term lists (the length of vec) */
} pmt_sparse_lsq_term;
int pmt_sparse_gram_sum_merge(int64_t n, int nblocks, const uint32_t *const *host_pair_j, const uint32_t *const *host_pair_k,
                              const int64_t *host_nq, const uint32_t *const *host_lin_col, const int64_t *host_nlin, int nterms,
                              const int32_t *term_kind, const int32_t *term_has_vec, const int64_t *const *term_cols,
                              const int64_t *term_ncols, int64_t *out_nq, int64_t *out_nlin, uint32_t *out_pair_j, uint32_t *out_pair_k,
                              uint32_t *out_lin_col, uint32_t *const *quad_at, uint32_t *const *lin_at, int32_t *const *term_pos);
int pmt_sparse_gram_sum_f64(int64_t n, const pmt_sparse_lsq_term *terms, int nterms, const uint32_t *pair_j, const uint32_t *pair_k,
                            int64_t nq, const uint32_t *lin_col, int64_t nlin, const int64_t *xvar, const int64_t *varmap,
                            pmt_quadratic_term *out_quad, pmt_linear_term *out_lin, double *out_const, void *stream);

/* Sparse quadratic form: transpose(x) * Q * x with Q an n x n fixed-pattern CSC matrix (only nzval changes between calls) and x = n
 * DISTINCT variables in strictly increasing order, as the canonical MOI function.  The function is the reference's literal one minus the
 * structural zeros: bilinearmul! (src/functions.jl:840-858) emitting a term (Q[r,c], x_r, x_c) for the STORED entries only,
 * canonicalize! (:381-386), then the MOI copy (src/moi_interop.jl:45-62):
 *   quadratic terms  one per unordered pair {j, k}, j <= k, for which Q[j,k] or Q[k,j] is stored, sorted by (j, k); nq terms.  A term
 *                    exists even when its coefficient is 0.0.  The coefficient is
 *                      Q[j,k] + Q[k,j]   when both are stored: the sum of two numbers, defined bit for bit as in pmt_quad_form_f64;
 *                      the stored value  UNCHANGED when only one of them is stored (no + 0.0: -0.0 stays -0.0);
 *                      2*Q[j,j]          on the diagonal with moi = 1 (moi_interop.jl:58), Q[j,j] with moi = 0.
 *                    The index words are always (vm[xvar[j]], vm[xvar[k]]) with j <= k (moi = 0: xvar[j], xvar[k], varmap not read).  This
 *                    is one deliberate departure from the reference, whose canonicalize! leaves a lone term's two variables in stored
 *                    order (src/util.jl:18-19 compares the ordered pair, the term itself is kept): a lone lower-triangle entry Q[k,j]
 *                    keeps (x_k, x_j) there — the same monomial.
 *   linear terms     none
 *   constant         0.0
 * Symbolic phase, host, once per pattern (colptr / rowval 1-based as for pmt_sparse_gram_*; linear in nnz + n, no comparison sort: the
 * transpose pattern of the upper part by a counting pass, then row j of the upper part and column j of the lower part walked together):
 *   pmt_sparse_form_count -> nq
 *   pmt_sparse_form_order -> pair_j[nq], pair_k[nq] (0-based positions, sorted by (j, k)); src_a[nq]: the position in nzval of Q[j,k] (row j,
 *                            column k) or 0xFFFFFFFF; src_b[nq]: the position of Q[k,j] or 0xFFFFFFFF.  On the diagonal src_a is the entry
 *                            and src_b is 0xFFFFFFFF.  Never are both 0xFFFFFFFF.  nq is that of _count.
 *   a 0-based or non-monotone colptr, rows that do not ascend strictly within a column and null pointers are PMT_INVALID_ARGUMENT; a row
 *   outside 1 .. n, n < 0 or n >= 2^31, 2^32 - 1 or more non-zeros and an nq that is not that of _count are PMT_DIMENSION_MISMATCH — all
 *   checked before anything is written.
 * Per call, pmt_sparse_form_f64: ONE launch (csrc/sparse_form.hip), one workgroup per PMT_SPARSE_SUM_WG_TERMS output terms, one term per
 * thread.  The four table words are read coalesced; one or two values are gathered from nzval, each only where its source word is not
 * 0xFFFFFFFF; the add or the doubling above, no fma.  The 24-byte structs go through LDS and leave as 16-byte stores per wave; an output
 * base that is 8 mod 16 is fine.  The whole struct is rewritten at every call — the index words through varmap — every output term
 * exactly once, nothing beyond nq terms: the output may be host-visible memory.  *out_const = 0.0 when out_const is given.  nq = 0 is a
 * valid call (the constant only, or nothing).  No atomics, no wait between workgroups, no workspace.  The gathers are in range only because
 * pmt_sparse_form_order produced the tables: the kernel does not check them.  Null pointers (with nq > 0), a negative nq, moi outside
 * {0, 1} and moi without varmap are PMT_INVALID_ARGUMENT before any device call.  Algorithmic bytes: 16 nq (tables) + 24 nq (terms) + 8 per
 * value gathered. */
int pmt_sparse_form_count(int64_t n, const int64_t *host_colptr, const int64_t *host_rowval, int64_t *nq);
int pmt_sparse_form_order(int64_t n, const int64_t *host_colptr, const int64_t *host_rowval, int64_t nq, uint32_t *host_pair_j,
                          uint32_t *host_pair_k, uint32_t *host_src_a, uint32_t *host_src_b);
int pmt_sparse_form_f64(const double *nzval, const uint32_t *src_a, const uint32_t *src_b, const uint32_t *pair_j, const uint32_t *pair_k,
                        int64_t nq, const int64_t *xvar, int moi, const int64_t *varmap, pmt_quadratic_term *out_quad, double *out_const,
                        void *stream);

/* ---------------------------------------------------------------------------------------
 * Batched independent QPs (BASELINE config 4).  In the reference a batch is many independent Models (src/model.jl:1-22); all
 * instances share one structure, so per re-evaluation only coefficients are produced: one slab of
 * pmt_batch_lsq_slab_doubles(n, m) doubles per instance,
 *     [ Q: n(n+1)/2 | q: n | const: 1 | C: m*n row-major | d-consts: m ],
 * = the coefficients of the canonical MOI objective of residual . residual (Appendix A.3) and of the constraint block
 * C*x (+|-) d (Appendix A.4).  Inputs are instance-major: A[B][r*n] column-major, b[B][r], C[B][m*n] column-major, d[B][m].
 * Instance i's slab starts at out + i * out_stride (out_stride >= the slab length; the words between two slabs are not written).
 * Q is 2 A'A on the row-major upper triangle, q is 2 A'c with c = 0.0 (+|-) b, const is c'c summed left to right, the d-consts are
 * 0.0 (+|-) d.  Edge cases, each a complete slab:
 *   sign_b == 0   no constants in the residual: q and const are +0.0; sign_d == 0: the d-consts are +0.0 (b / d must still be valid)
 *   r == 0        no rows: Q, q and const are +0.0
 *   m == 0        no constraint block: the slab is [Q | q | const]
 *   n == 0        no variables: the slab is [const | d-consts]
 * pmt_batch_expand_f64 rebuilds the full MOI term buffers (with indices through xvar / varmap) of ONE instance from its slab: indices
 * and layout as pmt_quad_gram_f64 / pmt_affine_pack_vector_f64 produce them for that instance alone, Q and q equal to rounding (the
 * single-instance node sums in an order of its own), the constant and the constraint block bit for bit.
 * ------------------------------------------------------------------------------------- */
int64_t pmt_batch_lsq_slab_doubles(int64_t n, int64_t m);
int pmt_batch_lsq_coeffs_f64(const double *A, const double *b, const double *C, const double *d, int64_t B, int64_t n, int64_t r,
                             int64_t m, int sign_b, int sign_d, double *out, int64_t out_stride, void *stream);
int pmt_batch_expand_f64(const double *slab, int64_t n, int64_t m, const int64_t *xvar, const int64_t *varmap,
                         pmt_quadratic_term *out_quad, pmt_linear_term *out_lin, double *out_const,
                         pmt_vector_affine_term *out_vat, double *out_vconsts, void *stream);

/* The batch whose objective is the tracking cost transpose(x (+|-) p_i) * Q_i * (x (+|-) p_i) — every instance with a weight matrix and a
 * reference of its own — over the constraint block C_i*x (+|-) d_i: one slab per instance at out + i * out_stride, in the layout above
 * (pmt_batch_lsq_slab_doubles(n, m) doubles; out_stride >= that; the words between two slabs are never written), so pmt_batch_expand_f64,
 * pmt_batch_allgather_f64 and the chunk arithmetic take it as it is.  Inputs are instance-major: Q[B][n*n] column-major with leading
 * dimension n (it need not be symmetric), p[B][n], C[B][m*n] column-major, d[B][m].  The contents are fixed bit for bit — plain multiplies
 * and adds, no fma, independent of B, of the instance's position, of launch geometry and timing:
 *   Q section   at tri(j,k) = j*n - j*(j-1)/2 + k - j: S[j,k] = Q[j,k] + Q[k,j] for j < k, 2*Q[j,j] on the diagonal — the moi = 1 coefficients
 *               of pmt_quad_form_f64.
 *   q, const    sign_p = +-1, c = 0.0 (+|-) p: q[j] = lin_j and const = 0.5 * T in the order fixed above for pmt_quad_form_shift_f64, word
 *               for word: P[Bk][j] = ((S[j,k0]*c_k0 + S[j,k0+1]*c_{k0+1}) + ..) + S[j,k1]*c_k1 over column block Bk = columns k0 = 64 Bk ..
 *               k1 = min(64 Bk + 63, n-1), the first product starting the chain; lin_j = ((P[0][j] + P[1][j]) + ..) + P[nb-1][j], the
 *               nb = ceil(n / 64) blocks in order; T = sum_j c_j*lin_j by 256 chains onto 0.0 (n <= 256: chain t holds 0.0 + c_t*lin_t),
 *               then the halving tree (t += t + 128, t + 64, ..).  The slab equals what that node writes for the instance alone.
 *               sign_p == 0: q and const are +0.0 and p may be NULL — the plain form, pmt_quad_form_f64 with out_lin / out_const.
 *   C, d-consts as pmt_batch_lsq_coeffs_f64: C row-major, 0.0 (+|-) d, +0.0 with sign_d == 0 (d must still be valid).
 * Edge cases, each a complete slab: m == 0: [Q | q | const]; n == 0: [+0.0 | d-consts]; B == 0: PMT_OK without a launch, whatever the
 * pointers.  A negative dimension, n > PMT_BATCH_FORM_MAX_N or out_stride below the slab length: PMT_DIMENSION_MISMATCH; a sign outside
 * {-1, 0, 1} or a null pointer where data is needed: PMT_INVALID_ARGUMENT — all before any device call.  One launch (csrc/batch_form.hip):
 * one workgroup per instance walks its 64 x 64 tile pairs as pmt_quad_form_shift_f64's tile kernel does and keeps the chains P in LDS
 * where that node has its workspace; no workspace, no atomics, no workgroup waits for another.  Algorithmic bytes per instance:
 * 8 (n^2 + n + m n + m) read, 8 L written. */
#define PMT_BATCH_FORM_MAX_N 256
int pmt_batch_form_coeffs_f64(const double *Q, const double *p, const double *C, const double *d, int64_t B, int64_t n, int64_t m, int sign_p,
                              int sign_d, double *out, int64_t out_stride, void *stream);

/* Horizon stage costs: a sum of T >= 1 stages over pairwise DISJOINT, strictly increasing Variable vectors x_t as one canonical MOI function
 * from one launch — J = sum_t transpose(x_t - r_t)*Q*(x_t - r_t) + transpose(u_t)*R*u_t, what a model-predictive controller writes.  Stage t
 * is transpose(x_t (+|-) v_t) * Q_t * (x_t (+|-) v_t) (sign = +-1), or the plain form transpose(x_t) * Q_t * x_t (sign == 0, vec may be NULL);
 * many stages may name the same Q.  No pair (j, k) is shared between two stages, so canonicalize! (src/functions.jl:381-386) combines
 * nothing across them.  The caller builds a DEVICE array of descriptors once; indices go through the varmap (moi = 1, alpha = 1.0):
 *   quadratic terms  stage t writes its n(n+1)/2 terms at out_quad + quad_at, row j holding its columns k >= j at tri(j,k) = j*n - j*(j-1)/2 + k - j;
 *                    every word equals what pmt_quad_form_f64 / pmt_quad_form_shift_f64 writes for that stage alone with the same Q, xvar,
 *                    varmap, moi = 1 and alpha = 1.0.  quad_at may be odd: an address 8 mod 16.
 *   linear terms     stage t writes n terms at out_lin + lin_at: (lin_j, vm[xvar[j]]), lin_j in the order fixed above for
 *                    pmt_quad_form_shift_f64 (64-column chains, the first product starting the chain, then the blocks in order), word for
 *                    word; a plain stage writes (0.0, vm[xvar[j]]).
 *   constant         stage_consts[t] = 0.5 * T_t, T_t = sum_j c_j*lin_j in that node's chain-then-tree order (n <= 256: chain j holds
 *                    0.0 + c_j*lin_j); a plain stage contributes +0.0.  *out_const = the sum of stage_consts in S_d's order of
 *                    pmt_quad_gram_sum_f64: 256 chains (chain c adds the stages c, c + 256, .. in order onto 0.0), then the halving tree
 *                    (c += c + 128, c + 64, ..) — a short second launch of one workgroup, ordered by the stream alone.
 * Plain multiplies and adds, no fma, no floating-point atomics, no workgroup waits for another; the results do not depend on T, on the
 * stage's position in the table, on launch geometry or on timing.  Every output word is written exactly once per call, nothing outside the
 * stages' slices is written, and stage_consts (device, T doubles) is written before it is read: it needs no zeroing.
 * pmt_quad_stages_check is host arithmetic over a HOST copy of the table (no device call): a null Q or xvar, a sign outside {-1, 0, 1}, a
 * NULL vec with sign != 0 (or a null table with T > 0): PMT_INVALID_ARGUMENT; n outside 1 .. PMT_QUAD_STAGES_MAX_N, ldq < n, T < 0, a slice
 * leaving [0, nterms) / [0, nlin), slices that overlap: PMT_DIMENSION_MISMATCH.  pmt_quad_stages_f64 itself rejects null pointers
 * (PMT_INVALID_ARGUMENT) and T < 0 (PMT_DIMENSION_MISMATCH) before any device call; T == 0 writes *out_const = 0.0 only.  The kernel reads
 * the table on the device and does NOT check it again: pass a table only after pmt_quad_stages_check accepted its host copy.
 * Persistent workgroups of 256 threads, three per CU, grid = min(T, 3 CUs), workgroup g taking the stages g, g + G, ..; a stage is walked as
 * pmt_batch_form_coeffs_f64 walks an instance, with the chains in LDS (csrc/quad_stages.hip).  Algorithmic bytes: 24 per quadratic and 16 per
 * linear term written; every distinct Q once, the vectors and the table read. */
#define PMT_QUAD_STAGES_MAX_N 256
typedef struct {
    const double *Q; int64_t ldq;      /* n columns of ldq doubles; many stages may name the same Q */
    const int64_t *xvar;               /* n model-variable indices, strictly increasing */
    const double *vec;                 /* v_t, or NULL with sign == 0 */
    int32_t n, sign;                   /* 1 .. PMT_QUAD_STAGES_MAX_N; -1 | 0 | +1 */
    int64_t quad_at, lin_at;           /* first quadratic / linear term of the stage in out_quad / out_lin */
} pmt_quad_stage;                      /* 56 bytes, no padding (static_assert in csrc/quad_stages.hip) */
int pmt_quad_stages_check(const pmt_quad_stage *host_stages, int64_t T, int64_t nterms, int64_t nlin);
int pmt_quad_stages_f64(const pmt_quad_stage *stages, int64_t T, const int64_t *varmap, pmt_quadratic_term *out_quad,
                        pmt_linear_term *out_lin, double *stage_consts, double *out_const, void *stream);
/* The same horizon with a weight, a linear term and scalar constants beside the stages — 0.5*(sum_t ..), a discount g_t*(..), a tunable
 * rho*transpose(u_t)*R*u_t, an economic term dot(c_t, u_t), an offset — still one launch plus the short constant launch.  `terms` is a
 * DEVICE array of T entries, entry t belonging to stage t of `stages`; `consts` a DEVICE array of nconsts (0 .. PMT_QUAD_STAGES_MAX_CONSTS)
 * entries.  Weights are read on the device at run time: W_t = scale * (*weight), or scale when weight is NULL; W_c likewise from
 * lin_scale / lin_weight (ignored when lin_vec is NULL); W_i likewise for constant i.  Each product scale * (*weight) is one rounded double.
 * Stage t's slice equals, word for word, what two calls leave for that stage alone: pmt_quad_form_f64 / pmt_quad_form_shift_f64 (moi = 1,
 * alpha = 1.0), then pmt_quad_gram_sum_f64 over [first block with (scale, weight), PMT_LSQ_LINEAR with (lin_scale, lin_weight, lin_vec)].
 * With c(j,k), lin_j and cc_t = 0.5*T_t as pmt_quad_stages_f64 defines them, plain multiplies and adds, no fma:
 *   quadratic terms  coeff(j,k) = W_t * c(j,k) (c = S[j,k], and 2*Q[j,j] on the diagonal: W_t * (2*Q[j,j])); the index words are unchanged.
 *   linear terms     lin[j] = W_t * lin_j, then + W_c * c_t[j] when lin_vec is given.  A plain stage multiplies its +0.0: a negative W_t
 *                    leaves -0.0 where no linear term follows, as pmt_quad_gram_sum_f64 does; the sign of that zero is part of the contract.
 *   constant         stage_consts[t] = W_t * cc_t (a plain stage: W_t * +0.0).  *out_const = the chain-then-tree sum of stage_consts exactly
 *                    as pmt_quad_stages_f64 adds it; then, in table order, s = s + W_i * (value_i ? *value_i : 1.0) for the nconsts
 *                    constants, by one thread of the same second launch.  T == 0 writes only *out_const: the constants added onto 0.0.
 * A stage with scale == 1.0, weight == NULL and lin_vec == NULL writes the words of pmt_quad_stages_f64: multiplying by 1.0 is exact.  A
 * NaN weight puts NaN into its own stage's coefficients and into *out_const, and into no other stage's words.
 * Everything else of pmt_quad_stages_f64's contract holds unchanged: every output word is written exactly once per call, nothing outside
 * the slices, results independent of T, of a stage's position, of launch geometry and of timing; no workgroup waits for another, no
 * atomics, no workspace; stage_consts needs no zeroing.  The chains behind lin_j and cc_t stay unweighted, so they keep their order.
 * pmt_quad_stages_terms_check is host arithmetic over HOST copies of the three tables (no device call): everything
 * pmt_quad_stages_check refuses, with its code; a null host_terms with T > 0 or a null host_consts with nconsts > 0: PMT_INVALID_ARGUMENT;
 * nconsts outside 0 .. PMT_QUAD_STAGES_MAX_CONSTS: PMT_DIMENSION_MISMATCH.  pmt_quad_stages_terms_f64 itself rejects null pointers
 * (PMT_INVALID_ARGUMENT) and negative counts (PMT_DIMENSION_MISMATCH) before any device call and does not check the tables again.
 * Algorithmic bytes: those of pmt_quad_stages_f64, plus 40 per stage, n per linear vector and 24 per constant read. */
typedef struct {
    double scale; const double *weight;          /* W_t = weight ? scale * *weight : scale  (device scalar, read at run time) */
    double lin_scale; const double *lin_weight;  /* W_c likewise; ignored when lin_vec is NULL */
    const double *lin_vec;                       /* c_t (n doubles) of dot(c_t, x_t), or NULL */
} pmt_quad_stage_terms;                          /* 40 bytes, no padding; entry t belongs to stage t */
typedef struct {
    double scale; const double *weight; const double *value;   /* W_s * (value ? *value : 1.0) */
} pmt_quad_stage_const;                          /* 24 bytes */
#define PMT_QUAD_STAGES_MAX_CONSTS 32
int pmt_quad_stages_terms_check(const pmt_quad_stage *host_stages, const pmt_quad_stage_terms *host_terms, int64_t T,
                                const pmt_quad_stage_const *host_consts, int64_t nconsts, int64_t nterms, int64_t nlin);
int pmt_quad_stages_terms_f64(const pmt_quad_stage *stages, const pmt_quad_stage_terms *terms, int64_t T,
                              const pmt_quad_stage_const *consts, int64_t nconsts, const int64_t *varmap,
                              pmt_quadratic_term *out_quad, pmt_linear_term *out_lin, double *stage_consts, double *out_const, void *stream);
/* The same horizon with identity-weighted stage costs — rho*dot(u_t, u_t), dot(x_t - r_t, x_t - r_t), a ridge lam*dot(x_t, x_t) on a vector
 * that already carries a form — still one launch plus the short constant launch.  A stage is at most one of each over ONE strictly
 * increasing vector: a dense form with its weight, a diagonal term W_d*dot(x_t (+|-) v_t, x_t (+|-) v_t) (W_d*dot(x_t, x_t) without v), a
 * linear term W_c*dot(c_t, x_t); at least one of the form and the diagonal term.  `stages` and `terms` are the tables of
 * pmt_quad_stages_terms_f64, `diags` a DEVICE array of T entries or NULL (no stage has a rider):
 *   identity stage   Q == NULL: the stage is W_t*dot(x (+|-) v, x (+|-) v) with v = vec, sign = sign (sign == 0: dot(x, x)) and
 *                    W_t from terms[t].scale / .weight.  It owns n quadratic terms at quad_at — NOT n(n+1)/2 — and n linear terms at
 *                    lin_at; ldq is ignored; diags[t].present must be 0.
 *   rider            diags[t].present == 1 on a stage with a Q: the diagonal term W_d*dot(x (+|-) v^d, x (+|-) v^d) beside the form on the
 *                    same vector, W_d = weight ? scale * *weight : scale (one rounded product); v^d may differ from the form's shift.
 * The arithmetic is that of pmt_quad_gram_sum_f64 for a PMT_LSQ_DIAG term (D = (2*W_d) on the diagonal; W_d*(2*(0.0 (+|-) v_j)) in lin[j]
 * behind the blocks and in front of the linear terms; W_d*S_d in the constant; csrc/gram_sum.hip: sum_diag_shift_at, gram_sum_aux,
 * gram_sum_const).  With c_j = 0.0 (+|-) v_j and S = sum_j c_j*c_j in S_d's order (n <= 256: chain j holds 0.0 + c_j*c_j, then the halving
 * tree; c_j*c_j and v_j*v_j are the same double), plain multiplies and adds, no fma:
 *   identity stage   quadratic term j = ((2*W_t), vm[xvar[j]], vm[xvar[j]]).  lin[j] = W_t*(2*c_j) with a v, then + W_c*c_t[j] when lin_vec
 *                    is given; without v W_c*c_t[j] alone (the first contributor starts the chain: a -0.0 survives); with neither +0.0.
 *                    stage_consts[t] = W_t*S with a v, +0.0 without.
 *   rider            every word as pmt_quad_stages_terms_f64 writes it, except: the diagonal coefficient is W_t*(2*Q[j,j]) + (2*W_d);
 *                    lin[j] = W_t*lin_j, then + W_d*(2*c^d_j) when the rider has a v, then + W_c*c_t[j]; stage_consts[t] = W_t*cc_t,
 *                    then + W_d*S when the rider has a v.  Word for word what pmt_quad_form_f64 / pmt_quad_form_shift_f64 (moi = 1,
 *                    alpha = 1.0) leave for the stage alone, followed by pmt_quad_gram_sum_f64 over [block, PMT_LSQ_DIAG, PMT_LSQ_LINEAR].
 *   other stages     the words of pmt_quad_stages_terms_f64 (with unit terms: of pmt_quad_stages_f64).
 *   *out_const       unchanged: the chain-then-tree sum of stage_consts, then the scalar constants in table order.
 * Everything else of pmt_quad_stages_terms_f64's contract holds: every output word written exactly once, nothing outside the slices,
 * results independent of T, of a stage's position, of launch geometry and of timing; no workgroup waits for another, no atomics, no
 * workspace.  A NaN weight reaches its own stage's words and *out_const only.
 * pmt_quad_stages_diag_check is host arithmetic over HOST copies of the tables: everything pmt_quad_stages_terms_check refuses, with its
 * code, except that a NULL Q is an identity stage (its slice counted as n quadratic terms, its ldq not looked at); an identity stage with
 * present != 0, a present outside {0, 1}, a rider's sign outside {-1, 0, 1} (an identity stage's: the stage's own check), a rider's NULL
 * vec with sign != 0: PMT_INVALID_ARGUMENT; overlap or overrun of the slices: PMT_DIMENSION_MISMATCH.  host_diags may be NULL.
 * pmt_quad_stages_diag_f64 itself rejects null pointers (PMT_INVALID_ARGUMENT; diags may be NULL) and negative counts
 * (PMT_DIMENSION_MISMATCH) before any device call and does not check the tables again.  Algorithmic bytes: an identity stage reads its
 * vectors and writes 24 n + 16 n bytes; a rider reads n more doubles. */
typedef struct {
    double scale; const double *weight;          /* W_d = weight ? scale * *weight : scale, one rounded product */
    const double *vec;                           /* v_t (n doubles), or NULL with sign == 0 */
    int32_t sign, present;                       /* +1 | -1 with vec; present: 1 if stage t has a rider, else 0 */
} pmt_quad_stage_diag;                           /* 32 bytes, no padding */
int pmt_quad_stages_diag_check(const pmt_quad_stage *host_stages, const pmt_quad_stage_terms *host_terms,
                               const pmt_quad_stage_diag *host_diags, int64_t T, const pmt_quad_stage_const *host_consts,
                               int64_t nconsts, int64_t nterms, int64_t nlin);
int pmt_quad_stages_diag_f64(const pmt_quad_stage *stages, const pmt_quad_stage_terms *terms, const pmt_quad_stage_diag *diags,
                             int64_t T, const pmt_quad_stage_const *consts, int64_t nconsts, const int64_t *varmap,
                             pmt_quadratic_term *out_quad, pmt_linear_term *out_lin, double *stage_consts, double *out_const,
                             void *stream);
/* The same horizon for a device-resident solver: the CSC values of the block-diagonal upper-triangular P instead of quadratic term
 * structs — 8 bytes per entry, no index words —, from the same launch over the unchanged tables of pmt_quad_stages_diag_f64 (`terms` is
 * required: unit rows give the unweighted words; `diags` may be NULL; Q == NULL is an identity stage).  quad_at means something else here:
 * the stage's first double in out_P_values; the slice is n(n+1)/2 doubles, n for an identity stage.
 *   values           out_P_values[quad_at + k(k+1)/2 + j] = alpha * c(j,k) for j <= k: the layout and meaning of pmt_quad_form_f64's
 *                    out_P_values.  c(j,k) is the coefficient word pmt_quad_stages_diag_f64 writes at tri(j,k) for the same tables:
 *                    W_t*(Q[j,k] + Q[k,j]), W_t*(2*Q[j,j]), and + (2*W_d) under a rider.
 *   identity stage   out_P_values[quad_at + j] = alpha * (2*W_t).
 *   alpha            with alpha == 1.0 the values equal those coefficient words bit for bit; alpha is one more IEEE multiply (-1.0 flips
 *                    the sign bit).  Plain multiplies and adds, no fma.
 *   other outputs    out_lin, stage_consts and *out_const are word for word what pmt_quad_stages_diag_f64 writes; they are NOT scaled by
 *                    alpha (the hand-off applies the sense to q and r itself, as for pmt_quad_gram_csc_f64 / pmt_quad_form_f64).
 * Every output word is written exactly once per call and nothing outside the slices is written; a slice may start at any 8-byte address.
 * Results do not depend on T, on a stage's position in the table, on launch geometry or on timing; no workgroup waits for another, no
 * atomics, no workspace; persistent workgroups of 256 threads, three per CU, as pmt_quad_stages_diag_f64 (csrc/quad_stages.hip).
 * pmt_quad_stages_csc_check is host arithmetic over HOST copies of the tables: everything pmt_quad_stages_diag_check refuses for the stage,
 * terms, diag and const tables, with its codes; value slices that leave [0, nvalues) or overlap (linear slices: [0, nlin)):
 * PMT_DIMENSION_MISMATCH.  pmt_quad_stages_csc_f64 itself rejects a null stages, terms, varmap, out_P_values, out_lin or stage_consts (with
 * T > 0), a null out_const and a null consts with nconsts > 0 (PMT_INVALID_ARGUMENT), T < 0 and nconsts outside
 * 0 .. PMT_QUAD_STAGES_MAX_CONSTS (PMT_DIMENSION_MISMATCH) before any device call and does not check the tables again; T == 0 writes
 * *out_const only.  Algorithmic bytes: 8 per value and 16 per linear term written; every distinct Q once, the vectors and the tables read. */
int pmt_quad_stages_csc_check(const pmt_quad_stage *host_stages, const pmt_quad_stage_terms *host_terms,
                              const pmt_quad_stage_diag *host_diags, int64_t T, const pmt_quad_stage_const *host_consts,
                              int64_t nconsts, int64_t nvalues, int64_t nlin);
int pmt_quad_stages_csc_f64(const pmt_quad_stage *stages, const pmt_quad_stage_terms *terms, const pmt_quad_stage_diag *diags,
                            int64_t T, const pmt_quad_stage_const *consts, int64_t nconsts, const int64_t *varmap, double alpha,
                            double *out_P_values, pmt_linear_term *out_lin, double *stage_consts, double *out_const, void *stream);

/* Horizon dynamics constraints: the MOI.VectorAffineFunction buffers of T affine records from one launch — x_{t+1} == A*x_t + B*u_t (+ w_t)
 * for every stage of a horizon, the other half of the model whose objective pmt_quad_stages_f64 writes.  A record is a sum
 * (+|-)L_1 (+|-) L_2 .. of 1 .. PMT_AFFINE_STAGES_MAX_PARTS leaves of equal row count with terms — a dense product M*v of a column-major
 * matrix and a Variable vector, or a Variable vector alone — and at most one number vector.  In the reference every product is matvecmul!
 * (src/functions.jl:775-798), every + / - vecadd! / vecsubtract! (:751-764: copyto! :419-427, add! / subtract! :452-485) and the copy
 * update!(::MOI.VectorAffineFunction, fs, varmap) (src/moi_interop.jl:64-81).  Two DEVICE tables describe the records; the host builds them once:
 *   pmt_affine_part   one leaf with terms, in expression order: `mat` (rows x cols, leading dimension ld) over the cols model variables
 *                     `xvar`, or mat == NULL for a Variable vector (cols == 1, `xvar` has the record's `rows` entries); sign = +1 | -1, the
 *                     product of the signs on the leaf's way to the root.
 *   pmt_affine_stage  one record: rows, its parts first_part .. first_part + nparts - 1, row_len = the sum of their cols, its first term
 *                     (term_offset) and first constant (const_offset) in the outputs, its number vector `vec` with vec_sign = +1 | -1, or
 *                     NULL with vec_sign == 0.
 * For stage s, row i, part p starting at term o_p of the row (the cols of the parts before it), column j:
 *   out_terms[term_offset + i*row_len + o_p + j] = (i + 1,  mat[i + j*ld], with its sign bit flipped when sign == -1,  vm[xvar[j]])
 *       a Variable-vector part:                    (i + 1,  +1.0 | -1.0,  vm[xvar[i]])                (vm[v] = varmap[v - 1], v itself without a varmap)
 *   out_consts[const_offset + i] = 0.0 (+|-) vec[i] by vec_sign,  0.0 without a vector
 * These are the words of pmt_affine_assemble_f64 per product, pmt_affvec_combine_f64 per + / - and pmt_pack_vector_affine_f64 on the same
 * data: the combine copies part a and multiplies part b by an exact +1 / -1 (-1 flips the sign bit, of a zero too), the pack copies the
 * coefficients.  The constant: a product's constants are +0.0, a Variable vector has none, and every combine gives ca (+ sb*cb), or 0.0 + sb*cb
 * without ca; so a number vector that is NOT the leftmost leaf of the whole sum has passed through at least one `0.0 (+|-)` or `+0.0 +` by
 * the root, which leaves 0.0 (+|-) vec[i] for every input, signed zeros included (NaN payloads are not part of the contract).  A leftmost
 * number vector enters as itself (a -0.0 entry survives): such a record is not described by these tables.
 * Every output word is written exactly once per call, nothing outside the stages' slices; no atomics, no workgroup waits for another; the
 * words do not depend on T, on a stage's position in the table, on launch geometry or on timing.  Persistent workgroups of 256 threads walk
 * the stages; a matrix part is cut into tiles of 16 rows x 64 columns, read along its columns, transposed through LDS and written row segment by row
 * segment as 16-byte stores — a segment may start at an address 8 mod 16 (csrc/affine_stages.hip).  Algorithmic bytes: 24 per term and 8
 * per constant written; every matrix once per stage (from L2 when stages share it), the vectors, index words and tables read.
 * pmt_affine_stages_check is host arithmetic over HOST copies of the tables (no device call): a null table with T > 0, a null xvar, a part
 * sign other than +-1, a vec_sign outside {-1, 0, 1}, a vector without a sign or a sign without a vector: PMT_INVALID_ARGUMENT; negative
 * counts, rows < 1, nparts outside 1 .. PMT_AFFINE_STAGES_MAX_PARTS, parts outside [0, nparts), cols < 1, ld < rows, a Variable-vector part
 * with cols != 1, row_len not the sum of the parts' cols, or term / constant slices that do not tile [0, nterms) / [0, nconsts) exactly — an
 * overlap, a gap, a slice past the end: PMT_DIMENSION_MISMATCH.  pmt_affine_stages_f64 itself rejects T < 0 (PMT_DIMENSION_MISMATCH) and,
 * with T > 0, a null table or output (PMT_INVALID_ARGUMENT) before any device call; varmap may be NULL (the identity); T == 0 writes
 * nothing.  The kernel reads the tables on the device and does NOT check them again: pass tables only after the check accepted their host copies. */
#define PMT_AFFINE_STAGES_MAX_PARTS 8
typedef struct {
    const double *mat; int64_t ld;     /* rows x cols, column-major; NULL: a Variable vector */
    const int64_t *xvar;               /* cols model-variable indices (a Variable vector: rows of them) */
    int32_t cols, sign;                /* terms per row; +1 | -1 */
} pmt_affine_part;                     /* 32 bytes, no padding (static_assert in csrc/affine_stages.hip) */
typedef struct {
    const double *vec;                 /* the number vector, or NULL with vec_sign == 0 */
    int64_t term_offset, const_offset; /* first term / constant of the stage in out_terms / out_consts */
    int64_t row_len;                   /* terms per row: the sum of the parts' cols */
    int32_t rows, first_part, nparts, vec_sign;
} pmt_affine_stage;                    /* 48 bytes, no padding (static_assert in csrc/affine_stages.hip) */
int pmt_affine_stages_check(const pmt_affine_stage *host_stages, int64_t T, const pmt_affine_part *host_parts, int64_t nparts,
                            int64_t nterms, int64_t nconsts);
int pmt_affine_stages_f64(const pmt_affine_stage *stages, int64_t T, const pmt_affine_part *parts, const int64_t *varmap,
                          pmt_vector_affine_term *out_terms, double *out_consts, void *stream);

/* The batch of horizons: B independent instances (src/model.jl:1-22), each the whole horizon above with weights and references of its own,
 *   J_i = sum_{t<T} transpose(x_t (+|-) r_{i,t})*Q_i*(x_t (+|-) r_{i,t}) + transpose(u_t (+|-) v_{i,t})*R_i*(u_t (+|-) v_{i,t})
 * over the instance's variables z = [x_0; u_0; x_1; u_1; ..], n = T*(nx + nu), subject to the constraint block C_i*z (+|-) d_i.  Per instance
 * this replaces, stage by stage, matvecmul! over the affine vector (src/functions.jl:800-822) and vecdot! (:702-709 over :548-576), the add!
 * of the stages (:244), canonicalize! (:381-386) and the MOI copies (src/moi_interop.jl:45-81), coefficients only.  Q_i and R_i are shared by
 * the instance's T stages, so its slab of pmt_batch_horizon_slab_doubles(T, nx, nu, m) doubles at out + i * out_stride holds each once:
 *     [ SQ: nx(nx+1)/2 | SR: nu(nu+1)/2 | q: n | const: 1 | C: m*n row-major | d-consts: m ]
 * (out_stride >= that length; the words between two slabs are never written).  Inputs are instance-major: Q[B][nx*nx] and R[B][nu*nu]
 * column-major with leading dimension nx / nu (they need not be symmetric), r[B][T*nx] and v[B][T*nu] stage-major, C[B][m*n] column-major,
 * d[B][m].  The contents are fixed bit for bit — plain multiplies and adds, no fma, no floating-point atomics, no workgroup waits for
 * another; independent of B, of the instance's position, of launch geometry and timing:
 *   SQ, SR      the moi = 1 coefficients of pmt_quad_form_f64 for Q_i / R_i at tri(j,k) = j*nd - j*(j-1)/2 + k - j (nd = nx / nu): S[j,k] =
 *               M[j,k] + M[k,j] for j < k, 2*M[j,j] on the diagonal — the Q section of pmt_batch_form_coeffs_f64.
 *   q           in z order: the nx words of stage x_t are the lin_j of pmt_quad_form_shift_f64 for (Q_i, r_{i,t}, sign_r), the nu words of
 *               stage u_t those for (R_i, v_{i,t}, sign_v), in that node's order (64-column chains, the first product starting the chain, then
 *               the nb <= 2 blocks in order).  A sign of 0 is the plain stage: +0.0, and the reference pointer may be NULL.
 *   const       what pmt_quad_stages_f64 leaves in *out_const for the table [x_0, u_0, x_1, u_1, ..] ([x_0, x_1, ..] with nu == 0): each stage's
 *               constant 0.5 * T_s in that node's chain-then-tree order (a plain stage: +0.0), the stage constants added in S_d's order — 256
 *               chains over the stages in z order onto 0.0, then the halving tree.
 *   C, d-consts as pmt_batch_lsq_coeffs_f64: C row-major, 0.0 (+|-) d, +0.0 with sign_d == 0 (d must still be valid).
 * Edge cases, each a complete slab: m == 0: [SQ | SR | q | const]; nu == 0: no SR, the stages are x_0, x_1, ..; both signs 0: the plain
 * horizon, q and const +0.0; B == 0: PMT_OK without a launch, whatever the pointers.  A negative dimension, nx < 1, nx or nu above
 * PMT_BATCH_HORIZON_MAX_DIM, T outside 1 .. PMT_BATCH_HORIZON_MAX_T or out_stride below the slab length: PMT_DIMENSION_MISMATCH; a sign
 * outside {-1, 0, 1} or a null pointer where data is needed: PMT_INVALID_ARGUMENT — all before any device call.  One launch, no workspace
 * (csrc/batch_horizon.hip): persistent workgroups of 256 threads, workgroup g taking the instances g, g + G, ..; a workgroup forms S_Q's
 * upper 64 x 64 tiles once as pmt_batch_form_coeffs_f64's does and keeps them in LDS (one tile for dims <= 64: three workgroups per CU; three
 * for dims <= 128: one per CU), writes SQ, runs the T matvecs from LDS with one thread per row (a stage in 16, 32 or 64 lanes of a wave, or
 * in two waves above 64 rows), then the same for R_i, the constants' tree, C_i and the d-consts.  Algorithmic bytes per instance: 8 (nx^2 + nu^2 + T nx + T nu + m n + m) read, 8 L written.
 * pmt_batch_horizon_expand_f64 rebuilds ONE instance's MOI buffers from its slab, with xvar the n model variables of z and indices through
 * the varmap: out_quad (T (nx(nx+1)/2 + nu(nu+1)/2) terms), out_lin (n terms) and *out_const are, word for word, what pmt_quad_stages_f64
 * writes for the instance's table with the stages laid out one behind the other (quad_at / lin_at cumulative in z order; a plain stage's
 * linear terms are (0.0, vm[xvar[j]])); out_vat (m*n terms) and out_vconsts (m) are what pmt_batch_expand_f64 writes.  Every output needs
 * 8-byte alignment only.  The dimension errors above (PMT_DIMENSION_MISMATCH) and a null slab, xvar, varmap or output that a non-zero size
 * needs (PMT_INVALID_ARGUMENT) come before any device call.  A streaming launch: 8 L bytes read, 24 / 16 / 24 bytes per term written. */
#define PMT_BATCH_HORIZON_MAX_DIM 128      /* nx, nu */
#define PMT_BATCH_HORIZON_MAX_T   512
int64_t pmt_batch_horizon_slab_doubles(int64_t T, int64_t nx, int64_t nu, int64_t m);
int pmt_batch_horizon_coeffs_f64(const double *Q, const double *R, const double *r, const double *v, const double *C, const double *d,
                                 int64_t B, int64_t T, int64_t nx, int64_t nu, int64_t m, int sign_r, int sign_v, int sign_d,
                                 double *out, int64_t out_stride, void *stream);
int pmt_batch_horizon_expand_f64(const double *slab, int64_t T, int64_t nx, int64_t nu, int64_t m, const int64_t *xvar, const int64_t *varmap,
                                 pmt_quadratic_term *out_quad, pmt_linear_term *out_lin, double *out_const,
                                 pmt_vector_affine_term *out_vat, double *out_vconsts, void *stream);

/* The batch of horizons' own dynamics: instance i's constraints x_{t+1} == A_i*x_t + B_i*u_t + w_{i,t} as a COMPACT section instead of rows of
 * the dense C_i above — of those rows every word outside T-1 copies of [A_i | B_i] and one +-1.0 per row is a structural zero.  An instance's
 * constraints are T vector-affine records over z = [x_0; u_0; x_1; u_1; ..], the records of pmt_affine_stages_f64 on the instance's own
 * tables — in the reference matvecmul! (src/functions.jl:775-798) per product, vecadd! / vecsubtract! (:751-764: copyto! :419-427, add! /
 * subtract! :452-485) per + / - and update!(::MOI.VectorAffineFunction, fs, varmap) (src/moi_interop.jl:64-81):
 *   record 0              x_0 (+|-) h_{i,0}: the initial condition, one Variable-vector part
 *   record t = 1 .. T-1   (+|-)x_t (+|-) A_i*x_{t-1} (+|-) B_i*u_{t-1} (+|-) h_{i,t}, the parts in this order (the spelling x+ - A*x - B*u - w);
 *                         with nu == 0 there is no B part
 * nx in 1 .. PMT_BATCH_HORIZON_MAX_DIM, nu in 0 .. PMT_BATCH_HORIZON_MAX_DIM, T in 1 .. PMT_BATCH_HORIZON_MAX_T.
 * pmt_batch_horizon_dynamics_doubles (host arithmetic) is the section's length Ld = nx*(nx + nu) + T*nx.  pmt_batch_horizon_dynamics_f64
 * writes, at out + i * out_stride (out_stride >= Ld; the words between two sections are never written), the section
 *     [ AB: nx*(nx + nu) | h-consts: T*nx ]
 * from the instance-major inputs A[B][nx*nx] and Bm[B][nx*nu], column-major with leading dimension nx, and h[B][T*nx], stage-major:
 *   AB        row-major with row length nx + nu: AB[r*(nx + nu) + j] = A_i[r + j*nx] for j < nx, its sign bit flipped when sign_a == -1, and
 *             B_i[r + (j - nx)*nx] for j >= nx, flipped when sign_b == -1 — a row is the coefficient words of one row of a record, part A
 *             then part B.
 *   h-consts  h-consts[t*nx + r] = 0.0 (+|-) h_i[t*nx + r] by sign_h, so a -0.0 does not survive; +0.0 with sign_h == 0 (h may be NULL).
 * No arithmetic beyond that: copies, sign-bit flips and 0.0 (+|-) h.  Every word is written exactly once per call; no atomics, no workgroup
 * waits for another; the words do not depend on B, on the instance's position, on launch geometry or on timing.  Each of T == 1, nu == 0 (Bm
 * may be NULL) and sign_h == 0 is a complete section; B == 0 is PMT_OK without a launch, whatever the pointers.  Dimensions outside the
 * limits, a negative B or out_stride < Ld: PMT_DIMENSION_MISMATCH; sign_a or sign_b not +-1, sign_h outside {-1, 0, 1} or a null pointer
 * where data is needed: PMT_INVALID_ARGUMENT — all before any device call.  `out` and `out_stride` are free, so a caller places the section
 * behind the instance's objective slab in one row: out = slabs + L, out_stride = L + Ld with pmt_batch_horizon_coeffs_f64 at the same stride.
 * One launch, no workspace (csrc/batch_horizon_dyn.hip): persistent workgroups of 256 threads take the instances g, g + G, ..; [A_i | B_i]
 * is read along its columns in tiles of 4096 words (64 rows x 64 columns; 32 x 128 up to 32 rows, 16 x 256 up to 16), every load of a tile
 * unconditional on a clamped index and issued before the first value is looked at, transposed through LDS (pitch: the tile's columns + 1)
 * and stored as 8-byte words with the column on the lanes — a section starts at any 8-byte address; h streams through registers.
 * Instances of at most 512 AB words take a wave each, four to a workgroup, without LDS.  Algorithmic bytes per instance: 8 Ld read, 8 Ld
 * written.
 * pmt_batch_horizon_dynamics_expand_f64 rebuilds ONE instance's T MOI.VectorAffineFunction buffers from its section, with xvar the
 * n = T*(nx + nu) model variables of z and indices through the varmap (NULL: the identity): nx + (T-1)*nx*(1 + nx + nu) terms and T*nx
 * constants that are, word for word, what pmt_affine_stages_f64 writes for the instance's own tables —
 *   stage 0       rows = nx, one Variable-vector part over xvar[0 .. nx) with sign sign_xp, term_offset = 0, row_len = 1
 *   stage t >= 1  row_len = 1 + nx + nu, term_offset = nx + (t-1)*nx*(1 + nx + nu), the parts: the Variable vector over
 *                 xvar[t*(nx + nu) .. + nx) with sign sign_xp; A_i over xvar[(t-1)*(nx + nu) .. + nx) with sign sign_a; B_i over the next nu
 *                 entries with sign sign_b
 *   all stages    const_offset = t*nx, vec = h_{i,t}, vec_sign = sign_h
 * that is: row index r + 1 within each record, a Variable-part coefficient of +1.0 | -1.0, the AB words copied (they carry their signs),
 * the constants copied; the columns of a row are the contiguous slice xvar[(t-1)*(nx + nu) .. t*(nx + nu)).  Every output needs 8-byte
 * alignment only.  The dimension errors above (PMT_DIMENSION_MISMATCH), a sign_xp other than +-1 and a null section, xvar or output
 * (PMT_INVALID_ARGUMENT) come before any device call.  A streaming launch: a workgroup per four rows of a stage, the stage's nx + nu index
 * words vm[xvar[..]] fetched once into LDS, a wave per row through 16-byte stores; the section is read T-1 times, from cache; 24 bytes per
 * term and 8 per constant written. */
int64_t pmt_batch_horizon_dynamics_doubles(int64_t T, int64_t nx, int64_t nu);
int pmt_batch_horizon_dynamics_f64(const double *A, const double *Bm, const double *h, int64_t B, int64_t T, int64_t nx, int64_t nu,
                                   int sign_a, int sign_b, int sign_h, double *out, int64_t out_stride, void *stream);
int pmt_batch_horizon_dynamics_expand_f64(const double *section, int64_t T, int64_t nx, int64_t nu, int sign_xp, const int64_t *xvar,
                                          const int64_t *varmap, pmt_vector_affine_term *out_terms, double *out_consts, void *stream);

/* The batch of horizons' TIME-VARYING dynamics: instance i's constraints x_t == A_{i,t}*x_{t-1} + B_{i,t}*u_{t-1} + h_{i,t} with a matrix pair
 * per stage — the fleet that re-linearises every stage at every solve (real-time iteration, gain scheduling, trajectory tracking, scenario
 * trees over a nonlinear plant).  The siblings of pmt_batch_horizon_dynamics_*: the same argument order, limits and error codes, the same
 * records over z = [x_0; u_0; x_1; u_1; ..] — those of pmt_affine_stages_f64 on the instance's own tables; in the reference matvecmul!
 * (src/functions.jl:775-798) per product, vecadd! / vecsubtract! (:751-764: copyto! :419-427, add! / subtract! :452-485) per + / - and
 * update!(::MOI.VectorAffineFunction, fs, varmap) (src/moi_interop.jl:64-81):
 *   record 0              x_0 (+|-) h_{i,0}
 *   record t = 1 .. T-1   (+|-)x_t (+|-) A_{i,t}*x_{t-1} (+|-) B_{i,t}*u_{t-1} (+|-) h_{i,t}, the parts in this order; with nu == 0 there is no B part
 * nx in 1 .. PMT_BATCH_HORIZON_MAX_DIM, nu in 0 .. PMT_BATCH_HORIZON_MAX_DIM, T in 1 .. PMT_BATCH_HORIZON_MAX_T.
 * pmt_batch_horizon_dynamics_tv_doubles (host arithmetic) is the section's length Ltv = (T-1)*nx*(nx + nu) + T*nx.
 * pmt_batch_horizon_dynamics_tv_f64 writes, at out + i * out_stride (out_stride >= Ltv; the words between two sections are never written), the
 * section
 *     [ AB_1 | AB_2 | .. | AB_{T-1} | h-consts: T*nx ]
 * from inputs that are instance-major, then stage-major: A[B][T-1][nx*nx] and Bm[B][T-1][nx*nu], each matrix column-major with leading
 * dimension nx, matrix index s = t-1 belonging to record t; h[B][T*nx] as in the sibling:
 *   AB_t      nx*(nx + nu) words at (t-1)*nx*(nx + nu), row-major with row length nx + nu: AB_t[r*(nx + nu) + j] = A_{i,t}[r + j*nx] for j < nx,
 *             its sign bit flipped when sign_a == -1, and B_{i,t}[r + (j - nx)*nx] for j >= nx, flipped when sign_b == -1 — exactly the
 *             words the sibling's AB holds for that matrix pair.
 *   h-consts  h-consts[t*nx + r] = 0.0 (+|-) h_i[t*nx + r] by sign_h, so a -0.0 does not survive; +0.0 with sign_h == 0 (h may be NULL).
 * No arithmetic beyond that, so there is no order question.  Every word is written exactly once per call; no atomics, no workgroup waits
 * for another, no workspace; the words do not depend on B, on the instance's position, on launch geometry or on timing.  Each of T == 1
 * (the constants only; A and Bm may be NULL), nu == 0 (Bm may be NULL) and sign_h == 0 is a complete section; B == 0 is PMT_OK without a
 * launch, whatever the pointers.  Dimensions outside the limits, a negative B or out_stride < Ltv: PMT_DIMENSION_MISMATCH; sign_a or
 * sign_b not +-1, sign_h outside {-1, 0, 1} or a null pointer where data is needed: PMT_INVALID_ARGUMENT — all before any device call.
 * `out` and `out_stride` are free as in the sibling: out = slabs + L, out_stride = L + Ltv puts the section behind the objective slab.
 * Two anchors, both exact:
 *   - with A_{i,t} = A_i and B_{i,t} = B_i for every t, every block AB_t and the h-consts equal, word for word, the AB and the h-consts
 *     of pmt_batch_horizon_dynamics_f64's section for (A_i, B_i, h_i);
 *   - pmt_batch_horizon_dynamics_tv_expand_f64 rebuilds ONE instance's nx + (T-1)*nx*(1 + nx + nu) vector-affine terms and T*nx constants,
 *     word for word what pmt_affine_stages_f64 writes for the instance's own tables: the table layout given above for
 *     pmt_batch_horizon_dynamics_expand_f64 (stage 0: one Variable-vector part, row_len 1, term_offset 0; stage t >= 1: row_len 1 + nx + nu,
 *     term_offset nx + (t-1)*nx*(1 + nx + nu), the Variable vector over xvar[t*(nx + nu) .. + nx) with sign_xp, then the matrix parts over
 *     xvar[(t-1)*(nx + nu) ..); const_offset t*nx, vec = h_{i,t}, vec_sign = sign_h), except that stage t's matrix parts point at A_{i,t}
 *     and B_{i,t}.  Row index r + 1 within each record, a Variable-part coefficient of +1.0 | -1.0, the AB_t words copied (they carry their
 *     signs), the constants copied.  xvar: the n = T*(nx + nu) model variables of z (a horizon with a terminal stage: T + 1 records over
 *     T*(nx + nu) + nx variables, as for the sibling); varmap NULL: the identity.  Errors as the sibling's expansion.
 * Every output needs 8-byte alignment only.  One launch (csrc/batch_horizon_ltv.hip).  The work item is one matrix pair (i, t), item =
 * i*(T-1) + t-1 — consecutive items are contiguous in A and Bm — dealt over persistent workgroups of 256 threads, so that few instances
 * with many stages fill the device as many instances with few do; (i, t) follows the item without a division per item, all offsets are
 * 64-bit.  Tiles as in the sibling (4096 words read along the columns, loads unconditional on clamped indices and issued together,
 * transposed through LDS, 8-byte stores with the column on the lanes), the next tile's loads in flight under the current tile's stores,
 * and a tile of 2048 words, eight workgroups per CU, where that holds a whole row (nx + nu <= 64 at 17 .. 32 rows, <= 128 up to 16);
 * pairs of at most 512 AB words take a wave each without LDS.  Item (i, t) also writes the nx constants of stage t, the item of t = 1
 * those of stage 0 with them; T == 1 is a launch of the constants alone.  The expansion is the sibling's streaming writer reading row r of
 * AB_t: each section word is read once.  Algorithmic bytes per instance: 8 Ltv read, 8 Ltv written. */
int64_t pmt_batch_horizon_dynamics_tv_doubles(int64_t T, int64_t nx, int64_t nu);
int pmt_batch_horizon_dynamics_tv_f64(const double *A, const double *Bm, const double *h, int64_t B, int64_t T, int64_t nx, int64_t nu,
                                      int sign_a, int sign_b, int sign_h, double *out, int64_t out_stride, void *stream);
int pmt_batch_horizon_dynamics_tv_expand_f64(const double *section, int64_t T, int64_t nx, int64_t nu, int sign_xp, const int64_t *xvar,
                                             const int64_t *varmap, pmt_vector_affine_term *out_terms, double *out_consts, void *stream);

/* The batch of horizons with TIME-VARYING stage weights: the fleet that re-linearises every stage at every solve re-linearises its cost as
 * well — the Gauss-Newton or exact Hessian block of stage t changes with the stage — so instance i has a matrix per stage,
 *   J_i = sum_{t<T} transpose(x_t (+|-) r_{i,t})*Q_{i,t}*(x_t (+|-) r_{i,t}) + transpose(u_t (+|-) v_{i,t})*R_{i,t}*(u_t (+|-) v_{i,t})
 *         [+ transpose(x_T (+|-) r_{i,T})*Q_{i,T}*(x_T (+|-) r_{i,T})  when term == 1]
 * over z = [x_0; u_0; ..; u_{T-1}; (x_T)] subject to the siblings' dense constraint block C_i*z (+|-) d_i: the objective sibling of
 * pmt_batch_horizon_dynamics_tv_f64, with the limits and error codes of pmt_batch_horizon_coeffs_f64.  With term in {0, 1}
 *     n = T*(nx + nu) + term*nx variables,   ns = T*(1 + (nu > 0)) + term stages in z order: x_0, u_0, x_1, .., (x_T)  (x_0, x_1, .. with nu == 0).
 * Inputs are instance-major, then stage-major: Q[B][T+term][nx*nx] and R[B][T][nu*nu], each matrix column-major with leading dimension nx / nu
 * (they need not be symmetric), r[B][T+term][nx], v[B][T][nu], C[B][m*n] column-major, d[B][m].  The slab of
 * pmt_batch_horizon_tv_slab_doubles(T, nx, nu, term, m) doubles (host arithmetic) at out + i * out_stride (out_stride >= that length L; the
 * words between two slabs are never written; every slab word is written exactly once per call) is
 *     [ S: ns blocks in z order, block s = nd(nd+1)/2 words (nd = nx or nu) | q: n | sconst: ns | const: 1 | C: m*n row-major | d-consts: m ]
 * fixed bit for bit — plain multiplies and adds, no fma, no floating-point atomics, no workgroup waits for another; independent of B, of the
 * instance's position, of launch geometry and of timing:
 *   S           block s is the SQ / SR section of pmt_batch_horizon_coeffs_f64 for that stage's matrix M: M[j,k] + M[k,j] at
 *               tri(j,k) = j*nd - j*(j-1)/2 + k - j for j < k, 2*M[j,j] on the diagonal.
 *   q           in z order: stage s's nd words are the lin_j of pmt_quad_form_shift_f64 for (the stage's matrix, its reference, its sign) in
 *               that node's order (64-column chains, the first product starting the chain, the nb <= 2 blocks in order).  A sign of 0 is the
 *               plain stage: +0.0, and the reference pointer may be NULL.
 *   sconst      sconst[s] = the stage's constant 0.5 * T_s in that node's chain-then-tree order; a plain stage: +0.0.
 *   const       the ns sconst words added in S_d's order — 256 chains onto 0.0, chain c taking the stages c, c + 256, .. in order, then the
 *               halving tree: what pmt_quad_stages_f64 leaves in *out_const for the instance's own table.
 *   C, d-consts as in pmt_batch_horizon_coeffs_f64, over the n columns of this z.
 * Anchors, all exact: with Q_{i,t} = Q_i and R_{i,t} = R_i every S block, q and const equal the words of pmt_batch_horizon_coeffs_f64
 * (term == 0); block s, the stage's q words and sconst[s] equal the [Q | q | const] slab pmt_batch_form_coeffs_f64 writes for that stage as an
 * instance of its own (n = nd, m = 0).  Each of nu == 0 (R and v may be NULL), m == 0, term == 0 and T == 1 is a complete slab; B == 0 is
 * PMT_OK without a launch, whatever the pointers.  A negative dimension, nx outside 1 .. PMT_BATCH_HORIZON_MAX_DIM, nu above it, T outside
 * 1 .. PMT_BATCH_HORIZON_MAX_T, a term other than 0 or 1 or out_stride < L: PMT_DIMENSION_MISMATCH; a sign outside {-1, 0, 1} or a null pointer
 * where data is needed (out, Q, R with nu > 0, a reference whose sign is not 0, C and d with m > 0): PMT_INVALID_ARGUMENT — all before any
 * device call.  No workspace.
 * A streaming problem — every matrix is read once, about half its bytes are written, nothing is shared between stages — so the work item is
 * one STAGE, dealt over persistent workgroups of 256 threads; (i, t) follows the item without a division per item, all offsets are 64-bit:
 * 64 instances of 100 stages fill the device as 800 of 8 do.  The x stages of the batch are contiguous in Q and the u stages in R, so the call
 * is up to three launches ordered by the stream alone (csrc/batch_horizon_tv.hip): the x stages, the u stages (nu > 0), and a short launch
 * with a workgroup per instance that adds the instance's sconst words into const and writes C and the d-consts (these ride in that third
 * launch; with m == 0 it is a wave per instance and const alone).  Stages of nd <= 8 / 16 / 32 / 64 are packed 32 / 16 / 4 / 1 to a
 * workgroup pass (8, 16, 64 or 256 threads a stage, 8 or 16 loads a thread): the matrix is one tile, symmetrised through LDS from one
 * load, the next pass's loads issued before this pass's stores, the chain by one thread per row and the tree inside the stage's 8, 16, 32
 * or 64 lanes.  Stages of 65 .. 128 rows take pmt_batch_form_coeffs_f64's walk of the three upper 64 x 64 tiles.  Four workgroups per CU,
 * six at nd <= 8.  Algorithmic bytes per instance: 8 ((T+term)(nx^2 + nx) + T(nu^2 + nu) + m n + m) read, 8 L written.
 * pmt_batch_horizon_tv_expand_f64 rebuilds ONE instance's MOI buffers from its slab, xvar the n model variables of this z and indices through
 * the varmap (required): out_quad (T (nx(nx+1)/2 + nu(nu+1)/2) + term nx(nx+1)/2 terms), out_lin (n terms) and *out_const are, word for
 * word, what pmt_quad_stages_check + pmt_quad_stages_f64 write for the instance's own table — the stages laid out one behind the other,
 * quad_at / lin_at cumulative in z order, stage s's Q pointer at its own matrix; out_vat (m*n terms) and out_vconsts (m) as
 * pmt_batch_horizon_expand_f64 writes them.  Every output needs 8-byte alignment only.  Errors as the sibling's expansion, and a term other than
 * 0 or 1: PMT_DIMENSION_MISMATCH.  A streaming launch: 8 L bytes read, 24 / 16 / 24 bytes per term written.
 * The dynamics beside it: pmt_batch_horizon_dynamics_tv_f64 with T + term records at out + L, both calls at out_stride >= L + Ltv. */
int64_t pmt_batch_horizon_tv_slab_doubles(int64_t T, int64_t nx, int64_t nu, int64_t term, int64_t m);
int pmt_batch_horizon_tv_coeffs_f64(const double *Q, const double *R, const double *r, const double *v, const double *C, const double *d,
                                    int64_t B, int64_t T, int64_t nx, int64_t nu, int64_t term, int64_t m,
                                    int sign_r, int sign_v, int sign_d, double *out, int64_t out_stride, void *stream);
int pmt_batch_horizon_tv_expand_f64(const double *slab, int64_t T, int64_t nx, int64_t nu, int64_t term, int64_t m,
                                    const int64_t *xvar, const int64_t *varmap, pmt_quadratic_term *out_quad, pmt_linear_term *out_lin,
                                    double *out_const, pmt_vector_affine_term *out_vat, double *out_vconsts, void *stream);

/* The batch of horizons with a terminal cost, a weight per stage and linear stage terms — what pmt_quad_stages_terms_f64 added to the single
 * horizon, for the fleet, still one launch without a workspace:
 *   J_i = sum_{t<T} wx_{i,t} * transpose(x_t (+|-) r_{i,t})*Q_i*(x_t (+|-) r_{i,t}) + dot(gx_{i,t}, x_t)
 *                 + wu_{i,t} * transpose(u_t (+|-) v_{i,t})*R_i*(u_t (+|-) v_{i,t}) + dot(gu_{i,t}, u_t)
 *         + wN_i * transpose(x_T (+|-) rN_i)*P_i*(x_T (+|-) rN_i) + dot(gN_i, x_T)
 * over z = [x_0; u_0; ..; x_{T-1}; u_{T-1}; x_T] subject to C_i*z (+|-) d_i: a discount or a scenario probability per stage (a weight of 0
 * switches a stage off), the economic term or the gradient of a sequential linearisation, a terminal matrix of its own.  The terminal stage
 * x_T exists only when P is given; with term = (P != NULL) in {0, 1}
 *     n = T*(nx + nu) + term*nx variables,   ns = T*(1 + (nu > 0)) + term stages in z order: x_0, u_0, x_1, .., x_T (x_0, x_1, .. with nu == 0).
 * pmt_batch_horizon_terms describes the inputs: a HOST struct of DEVICE pointers, all instance-major as in pmt_batch_horizon_coeffs_f64, read
 * by the call and not kept.  A NULL weight array means every weight 1.0, a NULL linear array no linear term on those stages; each optional
 * array is all or nothing for its kind of stage.  The slab of pmt_batch_horizon_terms_slab_doubles(T, nx, nu, term, m) doubles (host arithmetic)
 * at out + i * out_stride (out_stride >= that length L; the words between two slabs are never written) is
 *     [ SQ: nx(nx+1)/2 | SR: nu(nu+1)/2 | SP: term*nx(nx+1)/2 | W: ns | q: n | const: 1 | C: m*n row-major | d-consts: m ]
 * fixed bit for bit — plain multiplies and adds, no fma, no floating-point atomics, no workgroup waits for another; independent of B, of the
 * instance's position, of launch geometry and timing:
 *   SQ, SR, SP  the moi = 1 coefficients of pmt_quad_form_f64 for Q_i / R_i / P_i, exactly as in pmt_batch_horizon_coeffs_f64: unweighted, once.
 *   W           W[s] the weight of stage s in z order as read; 1.0 where the weight array is NULL.
 *   q           in z order, stage s, row j: W_s * lin_j, then + g_s[j] when the stage has a linear vector; lin_j the chain of
 *               pmt_quad_form_shift_f64 (64-column blocks, the first product starting the chain, the blocks in order).  A plain stage (sign 0)
 *               multiplies its +0.0: a negative weight leaves -0.0 where no linear term follows, a NaN weight NaN.  These are the words
 *               pmt_quad_stages_terms_f64 leaves with scale = 1.0, weight = &W_s, lin_scale = 1.0, lin_weight = NULL, lin_vec = g_s.
 *   const       each stage constant W_s * (0.5 * T_s), the ns of them added in S_d's order — 256 chains over the stages in z order onto 0.0,
 *               then the halving tree: what pmt_quad_stages_terms_f64 leaves in *out_const for the instance's own table with nconsts = 0.
 *   C, d-consts as in pmt_batch_horizon_coeffs_f64, over the n columns of this z.
 * With every optional pointer NULL the slab without its W section equals the slab of pmt_batch_horizon_coeffs_f64 word for word (multiplying
 * by 1.0 is exact; a plain stage still yields +0.0).  A NaN weight reaches its own stage's q words and its own instance's const, no other word.
 * Each of nu == 0 (R, v, wu, gu are not read), m == 0, term == 0 (rN, wN, gN are not read) and T == 1 is a complete slab; B == 0 is PMT_OK
 * without a launch, whatever the device pointers.  A null `in`: PMT_INVALID_ARGUMENT.  A negative dimension, nx outside 1 ..
 * PMT_BATCH_HORIZON_MAX_DIM, nu above it, T outside 1 .. PMT_BATCH_HORIZON_MAX_T, a term other than 0 or 1 (the expansion) or out_stride < L:
 * PMT_DIMENSION_MISMATCH; a sign outside {-1, 0, 1} (sign_rN is checked without a P too) or a null pointer where data is needed (out, Q, R
 * with nu > 0, a reference whose sign is not 0, C and d with m > 0): PMT_INVALID_ARGUMENT — all before any device call.  The walk is
 * pmt_batch_horizon_coeffs_f64's (csrc/batch_horizon_terms.hip) with a third phase for P_i through the same resident tiles: three workgroups per CU
 * with one tile (dims <= 64), one with three; a stage's weight and linear words are fetched with its reference, a round ahead.  Algorithmic
 * bytes per instance: the sibling's, plus 8 (term*(nx^2 + nx) + ns + n) read where the optional arrays are given, 8 L written.
 * pmt_batch_horizon_terms_expand_f64 rebuilds ONE instance's MOI buffers from its slab, xvar the n model variables of this z: out_quad (T (nx(nx+1)/2
 * + nu(nu+1)/2) + term nx(nx+1)/2 terms) holds W_s * S[j,k] for stage s (the diagonal W_s * (2*M[j,j]); the section already holds 2*M[j,j]),
 * out_lin (n terms) and *out_const are copied from the slab, the index words go through varmap: word for word what
 * pmt_quad_stages_terms_check + pmt_quad_stages_terms_f64 write for the instance's own table [x_0, u_0, .., x_T] with the stages laid out one
 * behind the other; out_vat (m*n terms) and out_vconsts (m) as pmt_batch_expand_f64 writes them.  Errors as the sibling's expansion.
 * The dynamics of a horizon with a terminal stage have T + 1 records, up to x_T == A*x_{T-1} + B*u_{T-1} + h_T: call the unchanged
 * pmt_batch_horizon_dynamics_f64 and pmt_batch_horizon_dynamics_expand_f64 with T + 1.  Their expansion reads only xvar[t*w .. t*w + nx) and
 * xvar[(t-1)*w .. t*w), w = nx + nu, for the records t <= T: it never touches a u_T, so the n = T*w + nx variables of this z suffice. */
typedef struct {
    const double *Q, *R, *P;      /* [B][nx*nx], [B][nu*nu], [B][nx*nx] column-major; P NULL: no terminal stage */
    const double *r, *v, *rN;     /* [B][T*nx], [B][T*nu], [B][nx]; may be NULL where the sign is 0 */
    const double *wx, *wu, *wN;   /* [B][T], [B][T], [B]; NULL: every weight 1.0 */
    const double *gx, *gu, *gN;   /* [B][T*nx], [B][T*nu], [B][nx]; NULL: no linear term on those stages */
    const double *C, *d;          /* [B][m*n] column-major, [B][m] */
    int32_t sign_r, sign_v, sign_rN, sign_d;
} pmt_batch_horizon_terms;        /* 128 bytes, no padding */
int64_t pmt_batch_horizon_terms_slab_doubles(int64_t T, int64_t nx, int64_t nu, int64_t term, int64_t m);
int pmt_batch_horizon_terms_coeffs_f64(const pmt_batch_horizon_terms *in, int64_t B, int64_t T, int64_t nx, int64_t nu, int64_t m, double *out,
                                       int64_t out_stride, void *stream);
int pmt_batch_horizon_terms_expand_f64(const double *slab, int64_t T, int64_t nx, int64_t nu, int64_t term, int64_t m, const int64_t *xvar,
                                       const int64_t *varmap, pmt_quadratic_term *out_quad, pmt_linear_term *out_lin, double *out_const,
                                       pmt_vector_affine_term *out_vat, double *out_vconsts, void *stream);

/* ---------------------------------------------------------------------------------------
 * Device-side Parameter update callbacks for synthetic inputs (counter-based):
 * dst[i] = scale * U[0,1)(seed, i)   — the analogue of `Parameter(rand!, zeros(n, n), model)` README.md:36-43
 * ------------------------------------------------------------------------------------- */
int pmt_fill_uniform_f64(double *dst, int64_t n, uint64_t seed, double scale, void *stream);
/* column-major rows x cols matrix with leading dimension lda: dst[c*lda + i] = scale * U(seed, c*rows + i) — same values as the
 * contiguous stream.  Device copies of Parameter matrices whose column stride would be a multiple of 4 KiB are kept with a padded
 * lda: a power-of-two stride puts every column segment of a tile on the same memory channel. */
int pmt_fill_uniform_matrix_f64(double *dst, int64_t rows, int64_t cols, int64_t lda, uint64_t seed, double scale, void *stream);
/* The matrix fill with the seed read from the HOST word *seed_word at every launch — recorded into a plan, at every replay: a recorded
 * Parameter callback (README.md:36-43 rand!, new values at every update!) advances by the host storing the next seed into the word before
 * pmt_plan_update, with no call of its own and, in a small plan, no launch of its own.  cols == 1, lda == rows: a vector.  The word must
 * outlive the plan's tape.  A tape holding such an entry is not captured into a hipGraph. */
int pmt_fill_uniform_dyn_f64(double *dst, int64_t rows, int64_t cols, int64_t lda, const uint64_t *seed_word, double scale, void *stream);
/* the same stream from element index_offset on: dst[i] = scale * U(seed, index_offset + i) (shard of a larger array) */
int pmt_fill_uniform_offset_f64(double *dst, int64_t n, uint64_t seed, uint64_t index_offset, double scale, void *stream);

/* ---------------------------------------------------------------------------------------
 * Per-kernel timing report — the device analogue of `findallocs` (src/debug.jl:4-23), which walks the DAG and
 * reports a cost per node.  While enabled, every launch is bracketed by HIP events on its own stream (never inside
 * a hipGraph capture).  pmt_profile_report synchronises on the recorded events and writes one line per kernel:
 * "<kernel>\t<launches>\t<total_ms>\t<min_ms>\t<max_ms>\n"; returns the untruncated length.
 * ------------------------------------------------------------------------------------- */
int pmt_profile_enable(int on);
/* restrict the bracketing to kernels whose name contains `substring` (NULL or "": all) — two event records per launch are not
 * free (a few microseconds of queue time each), so a benchmark times only the kernel it reports on */
int pmt_profile_filter(const char *substring);
int64_t pmt_profile_report(char *host_buf, size_t cap);
/* Measurement hook for ONE kernel inside a step, without the in-stream gap a HIP-event pair around an in-step launch includes: while
 * `device_words` (2 * workgroups uint64 words in device memory, zeroed by the caller) is set, workgroup w < `workgroups` of the MOI pack
 * kernel (affine_tile_kernel<VAT>, pmt_affine_pack_vector_f64) stores its start / end on the constant-rate device clock (wall_clock64)
 * into words 2w, 2w + 1; the launch ran from the smallest start to the largest end.  NULL or 0 (the default) switches it off: one
 * uniform branch. */
int pmt_profile_kernel_stamps(void *device_words, int64_t workgroups);
/* rate of that clock in kHz (hipDeviceAttributeWallClockRate) */
int pmt_device_clock_khz(int device, int *khz);

/* ---------------------------------------------------------------------------------------
 * Multi-GPU exchange of the batched configuration (BASELINE config 4): one process per GPU, rank g owns the instances
 * [g * per_rank, (g + 1) * per_rank); after the exchange every rank holds every slab (`gathered`: nranks * per_rank slabs of `stride`
 * doubles, global instance order).  The reference has no counterpart (a batch is many independent Models, src/model.jl:1-22).
 * RCCL (librccl.so, dlopen'ed on first use) is driven from inside the library: the host only carries the 128-byte unique id from
 * rank 0 to the others (any launcher: torch.distributed, MPI, a file).  xGMI is point-to-point, so the exchange is the DIRECT schedule
 * — one grouped ncclSend / ncclRecv pair per peer, each over that peer's own link — not a ring.
 *   pmt_comm_unique_id        rank 0: a fresh id (128 bytes)
 *   pmt_comm_init_rank        every rank; nranks == 1 with a NULL id needs no RCCL (nothing to exchange); nranks == 1 WITH an id builds a
 *                             real one-rank RCCL communicator whose exchange is a grouped ncclSend/ncclRecv to itself — the N-rank
 *                             code path on a single GPU
 *   pmt_comm_rccl_calls       ncclSend + ncclRecv calls this communicator has issued so far
 *   pmt_batch_num_chunks / pmt_batch_chunk_range / pmt_batch_gathered_offset
 *                             the chunk schedule, pure host arithmetic: chunk c of a rank = local instances [c * chunk, min(., per_rank))
 *                             (chunk <= 0: one chunk); the slab of global instance i sits at i * stride doubles of `gathered`
 *   pmt_batch_allgather_f64   exchange of slabs that are already computed, chunk by chunk, enqueued on `stream`
 *   pmt_batch_step_f64        pmt_batch_lsq_coeffs_f64 over this rank's instances chunk by chunk on `stream`, chunk c on the wire (the
 *                             communicator's own stream) while chunk c + 1 is computed; `stream` is joined with the last exchange.
 *                             `stream` must be a HIP stream (not a plan's recording handle).
 * ------------------------------------------------------------------------------------- */
int pmt_comm_unique_id(void *out_id_128_bytes);
int pmt_comm_init_rank(int nranks, int rank, const void *unique_id_128_bytes, int device, void **out_comm);
int64_t pmt_comm_rccl_calls(void *comm);
int pmt_comm_destroy(void *comm);
/* the shard of rank `rank`: per_rank = total / nranks instances starting at `first`.  The exchange assumes the SAME per_rank on every
 * rank (the gathered buffer is nranks * per_rank slabs): a batch that does not divide is PMT_DIMENSION_MISMATCH, never an uneven split. */
int pmt_batch_shard(int64_t total, int nranks, int rank, int64_t *per_rank, int64_t *first);
int64_t pmt_batch_num_chunks(int64_t per_rank, int64_t chunk);
int pmt_batch_chunk_range(int64_t per_rank, int64_t chunk, int64_t c, int64_t *lo, int64_t *hi);
int64_t pmt_batch_gathered_offset(int rank, int64_t per_rank, int64_t local_instance, int64_t stride);
int pmt_batch_allgather_f64(void *comm, const double *local, double *gathered, int64_t per_rank, int64_t stride, int64_t chunk, void *stream);
int pmt_batch_step_f64(void *comm, const double *A, const double *b, const double *C, const double *d, int64_t per_rank, int64_t n, int64_t r,
                       int64_t m, int sign_b, int sign_d, double *local, double *gathered, int64_t stride, int64_t chunk, void *stream);

/* ---------------------------------------------------------------------------------------
 * Plan = a recorded re-evaluation: device buffers + a tape of the launches above.
 * Built once by the host from the lazy-expression DAG (↔ `dest = deepcopy(expr())` pre-allocation,
 * src/lazyexpression.jl:202,230,243), replayed by every update!(model) (src/model.jl:132-143) with no
 * allocation and no host logic (↔ FunctionWrapper hop per node, FunctionWrappersQuickFix.jl:108-126).
 * ------------------------------------------------------------------------------------- */
typedef struct pmt_plan pmt_plan;

int pmt_plan_create(int device, void *stream /* NULL: plan creates its own stream */, pmt_plan **out);
int pmt_plan_destroy(pmt_plan *plan);
void *pmt_plan_stream(pmt_plan *plan);
/* device allocation owned by the plan (zero-filled); freed by pmt_plan_destroy */
int pmt_plan_alloc(pmt_plan *plan, size_t bytes, void **out_device_ptr);
size_t pmt_plan_bytes_allocated(const pmt_plan *plan);
/* page-locked host memory (e.g. for the MOI function buffers pmt_plan_fetch writes into); not tied to a plan */
int pmt_host_alloc(size_t bytes, void **out_host_ptr);
int pmt_host_free(void *host_ptr);
/* asynchronous copies on the plan's stream */
int pmt_plan_upload(pmt_plan *plan, void *device_dst, const void *host_src, size_t bytes);
int pmt_plan_fetch(pmt_plan *plan, void *host_dst, const void *device_src, size_t bytes);
/* zero a device buffer (setup time): the padding rows of a Parameter matrix / vector must be zero when a kernel is given the padded row count */
int pmt_plan_zero(pmt_plan *plan, void *device_dst, size_t bytes);
/* pitched variants (hipMemcpy2DAsync): `height` rows of `width_bytes`, e.g. the columns of a matrix whose device copy is padded */
int pmt_plan_upload_2d(pmt_plan *plan, void *device_dst, size_t dst_pitch, const void *host_src, size_t src_pitch, size_t width_bytes,
                       size_t height);
int pmt_plan_fetch_2d(pmt_plan *plan, void *host_dst, size_t dst_pitch, const void *device_src, size_t src_pitch, size_t width_bytes,
                      size_t height);
int pmt_plan_synchronize(pmt_plan *plan);
/* The plan's device-side error state for callers that wait for its stream by other means (hipStreamSynchronize, an event, a wait of
 * their own): PMT_OK, or PMT_HIP_ERROR (cleared by the call) when a grid barrier of a fused run timed out during a replay since the last
 * check — the outputs of that re-evaluation are invalid.  pmt_plan_synchronize and pmt_plan_fetch_synchronize check it themselves. */
int pmt_plan_check(pmt_plan *plan);
/* Recorded fetch (while recording; lane-aware like every recorded call): at replay the D2H copy goes to the plan's FETCH stream, ordered
 * behind everything recorded before it on its lane, and runs while the rest of the tape is still busy — results reach a HOST solver
 * (MOI.set, src/moi_interop.jl:134,171) without waiting for the end of the re-evaluation.  host_dst should be page-locked.  The plan's
 * stream does not wait for these copies; pmt_plan_fetch_synchronize blocks the host until all of them (and a delivery of
 * pmt_quad_gram_csc_deliver_f64) have landed; the next pmt_plan_update waits on the device until they have read their buffers.
 * A plan with recorded fetches cannot be instantiated as a hipGraph. */
int pmt_plan_record_fetch(pmt_plan *plan, void *host_dst, const void *device_src, size_t bytes);
/* pitched recorded fetch: `height` rows of `width_bytes`, row r at device_src + r*src_pitch -> host_dst + r*dst_pitch.  The CSC values of a
 * DENSE constraint block are its Parameter matrix column by column (update!(::MOI.VectorAffineFunction) writes one term per entry,
 * src/moi_interop.jl:64-81): they leave straight out of the Parameter's (padded) device buffer for the block's row range in every column
 * of the solver's stacked matrix — no kernel, the copy engine's rectangle copy where it exists. */
int pmt_plan_record_fetch_2d(pmt_plan *plan, void *host_dst, size_t dst_pitch, const void *device_src, size_t src_pitch, size_t width_bytes,
                             size_t height);
/* HOST -> HOST pitched copy on `threads` worker threads (0: eight; small copies use fewer): `height` rows of `width_bytes`.  For the dense
 * blocks of a host solver's A whose Parameter the HOST updates (`Parameter(model, val=buf)`, src/parameter.jl:88): their values are already
 * on the host and are copied there — from the Parameter's buffer into the block's row range of every column of the solver's array — while
 * the device re-evaluates the rest, instead of coming back over PCIe.  Synchronous; no device work; the worker threads are created and joined
 * inside the call (the library keeps no threads of its own). */
int pmt_host_copy_2d(void *host_dst, size_t dst_pitch, const void *host_src, size_t src_pitch, size_t width_bytes, size_t height, int threads);
/* host: block until the plan's recorded fetches / deliveries have landed; errors as pmt_fetch_synchronize */
int pmt_plan_fetch_synchronize(pmt_plan *plan);

/* Staged (overlapped) uploads of host-updated Parameter values — `Parameter(model, val=buf)` / `Parameter(f, val, model)`,
 * src/parameter.jl:57,88,101-102: the user (or f) rewrites a host buffer between solves and update!() reads it when the Parameter is
 * evaluated.  pmt_plan_upload puts that PCIe copy on the plan's stream, serially in front of the kernels.  A staged upload goes through
 * the plan's COPY stream into a second device buffer (`device_staging`, same size / pitch as the Parameter's buffer) and therefore runs
 * while the kernels of the previous re-evaluation are still busy; the next update consumes it on the plan's stream:
 *     pmt_plan_stage_upload[_2d]   copy stream: waits until the previous commit has read the staging buffer, H2D, records "staged"
 *     pmt_plan_wait_staged         plan stream: waits for every staged upload issued so far
 *     pmt_plan_commit_staged       pmt_plan_wait_staged + device-to-device copy staging -> Parameter buffer (a Parameter that needs a
 *                                  transposition / permutation anyway runs that kernel from the staging buffer instead)
 *     pmt_plan_staging_consumed    plan stream: records "consumed" behind the commits (call once after the last commit of an update)
 *     pmt_plan_staged_synchronize  host: blocks until the staged uploads have left the HOST buffers (which may then be overwritten)
 * The host buffers must be page-locked (pmt_host_alloc) for the copy to be asynchronous. */
int pmt_plan_stage_upload(pmt_plan *plan, void *device_staging, const void *host_src, size_t bytes);
int pmt_plan_stage_upload_2d(pmt_plan *plan, void *device_staging, size_t dst_pitch, const void *host_src, size_t src_pitch, size_t width_bytes,
                             size_t height);
int pmt_plan_wait_staged(pmt_plan *plan);
int pmt_plan_commit_staged(pmt_plan *plan, void *device_dst, const void *device_staging, size_t bytes);
int pmt_plan_staging_consumed(pmt_plan *plan);
/* Lane of the commits that follow (pmt_plan_wait_staged / pmt_plan_commit_staged): 0 = the plan's stream (default), 1 = its side stream, the
 * one the side-lane entries of the tape run on (pmt_plan_set_lane).  A Parameter that ONLY side-lane entries read — the data of a constraint
 * whose MOI copy sits on the side lane — may be committed there: the plan's stream, i.e. the contraction of a least-squares objective, then
 * starts at once instead of waiting for this solve's upload (config 3 through the host hand-off: -0.3 ms per solve).  The caller
 * guarantees that nothing on the plan's stream reads those Parameters; pmt_plan_staging_consumed covers both lanes. */
int pmt_plan_commit_lane(pmt_plan *plan, int lane);
int pmt_plan_staged_synchronize(pmt_plan *plan);
/* Two staging SLOTS (0 / 1): the four calls above act on the current slot, each slot with its own staged / consumed events.  Alternating
 * the slot — and the staging buffers — from one update to the next lets the copy of update k+1 start while the commits of update k are
 * still reading theirs (with one slot it has to wait for them).  Optional: without this call everything uses slot 0. */
int pmt_plan_stage_slot(pmt_plan *plan, int slot);

/* recording: between begin_record and end_record every pmt_*_f64 call issued with stream ==
 * pmt_plan_recording_stream(plan) is appended to the plan's tape instead of being launched */
int pmt_plan_begin_record(pmt_plan *plan);
int pmt_plan_end_record(pmt_plan *plan);
/* While recording: lane 1 marks the following calls as SIDE-LANE entries, lane 0 (the default) returns to the plan's stream.  A side-lane
 * entry must read only buffers that are complete before pmt_plan_update starts (Parameter values) and write outputs that no other
 * entry of the tape reads — the MOI copy of a constraint built straight from its Parameters (update! of one Constraint,
 * src/moi_interop.jl:168-175, is independent of every other record).  At replay these entries fork from the plan's stream at the
 * top of the tape and join at its end; they are queued on the stream's side stream BEHIND the two small reductions of a canonical
 * least-squares objective, so they are dispatched when the contraction's workgroups are already placed and run while those drain and
 * while the fix-up pass runs, instead of adding their own kernels and in-stream gaps behind it.
 * Lane 2 is the FRONT of the side lane: the same stream, but replayed before every other entry of the tape whatever its position in the
 * recording — for an entry that needs nothing of this re-evaluation, e.g. the recorded fetch of a dense constraint block's CSC values
 * straight out of its Parameter buffer (pmt_plan_record_fetch_2d): PCIe is busy from the first microseconds of the solve.
 * Lane 3 is lane 2 WITHOUT the fork from the plan's stream: for an entry whose inputs are produced on the side stream itself (a Parameter
 * committed there, pmt_plan_commit_lane, or regenerated there, pmt_plan_lane_stream) — it does not wait for what the plan's stream still has
 * to do in front of the tape (the callbacks of the objective's Parameters).  The caller vouches for that; everything joins at the end. */
int pmt_plan_set_lane(pmt_plan *plan, int lane);
/* The HIP stream the entries of a lane are replayed on (0: pmt_plan_stream; 1, 2: the side stream).  A device-side Parameter callback whose
 * value only side-lane entries read may run THERE (in front of pmt_plan_update): a transfer at the front of the side lane then does not
 * wait for the callbacks of the objective's Parameters on the plan's stream.  Work issued on it is ordered before the side-lane entries
 * of the next update and joined into the plan's stream at that update's end. */
int pmt_plan_lane_stream(pmt_plan *plan, int lane, void **out_stream);
void *pmt_plan_recording_stream(pmt_plan *plan);
int64_t pmt_plan_tape_length(const pmt_plan *plan);
/* SMALL PLANS.  The reference walks a model's lazy-expression DAG at nanoseconds per hop (src/lazyexpression.jl:50-61; README Example 1
 * re-evaluates in ~15 us on a CPU core, README.md:132-136); a tape replay pays one kernel launch (~5 us) per hop whatever its size.
 * pmt_plan_end_record therefore replaces every run of two or more consecutive SMALL entries of the tape (lane 0; pmt_fill_uniform_*,
 * pmt_affine_assemble_f64, pmt_affine_pack_vector_f64, pmt_quad_expand_f64, pmt_vars_addsub_f64, pmt_consts_f64, pmt_pack_*_f64,
 * pmt_copy_bytes, pmt_transpose_f64, pmt_affvec_combine_f64 (uniform rows), pmt_affvec_scale_f64, pmt_matvecmul_affs_f64, the pmt_vecdot_*
 * forms, pmt_bilinear_f64, pmt_quad_combine_f64, pmt_quad_scale_f64, pmt_scale_*_f64, and pmt_quad_gram_f64 for tiny shapes — each writing
 * at most 32768 elements, a run at most 65536) by ONE launch of an interpreter kernel that executes the
 * run's nodes in tape order with a barrier between dependent ones (csrc/small.hip; one workgroup, or up to 32 with a grid barrier for
 * runs of tens of thousands of elements: pmt_plan_fused_workgroups).  Every element is computed by the same expression
 * as in the entry's own kernel: outputs are bit-identical.  Automatic; larger entries and everything else replay as recorded.
 *   pmt_plan_set_fusion  0: replay the tape as recorded (A/B and tests); 1 (default): fuse.  Not while recording / after graph capture.
 *   pmt_plan_fused       number of fused runs, tape entries they replace, and launches-or-entries one replay executes */
int pmt_plan_set_fusion(pmt_plan *plan, int on);
int pmt_plan_fused(const pmt_plan *plan, int *groups, int *nodes, int64_t *exec_length);
/* RIDERS.  The one-launch form of pmt_quad_gram_f64 / _csc (2049 .. 4096 columns and the wide shapes below; csrc/gram_mid.hip) runs, from
 * 512 work items on, as 256 persistent workgroups that hold every CU until they leave, and a workgroup's last item ends tens of
 * microseconds before the launch does.  pmt_plan_end_record lets dense constraint packs of the tape (pmt_affine_pack_vector_f64 with rows,
 * cols > 0) RIDE in such a node that delivers nothing to the host: a workgroup whose Gram items have run out draws the packs' tiles — the
 * stand-alone kernel's own tile body, so the pack's output is bit-identical — and the pack's entry leaves the replay.  Who rides:
 *   (a) the packs of the unbroken run of packs directly behind the node on the plan's own lane, and
 *   (b) side-lane packs (pmt_plan_set_lane 1) anywhere in the tape, as long as the caller has put nothing of its own on the side stream
 *       (pmt_plan_commit_lane(1), pmt_plan_lane_stream): from the first such call on they stay on the side stream, which alone orders them,
 * whose reads and writes are independent, by byte range, of the node's writes (and the node's reads of their writes), of the other riders
 * and, for (a), of what stays between them and the node; for (b) of every other entry that is not on the plan's own lane (an entry
 * whose ranges the plan does not know, such as a recorded fetch, counts as dependent).  At most 8 riders per node and 256 MB of
 * algorithmic bytes (32 per matrix entry) in all — measured beside a 4096 x 4096 node: 64 and 256 MB ride 12 us per step faster than
 * alone, 512 MB only 3-4 us, within the noise; a persistent workgroup is one per CU where the stand-alone pack runs eight, so larger
 * packs stay alone.  Immediate calls never have riders;
 * pmt_plan_set_fusion(plan, 0) turns riders off with the fused runs; a captured graph keeps them.
 *   pmt_plan_riders       packs that ride in this plan's nodes, and their tiles
 *   pmt_plan_rider_check  the decision alone, a pure host function: tape[0 .. n) describes the entries (kind 1: a one-launch node, 2: a dense
 *                         vector pack, 0: anything else / unknown ranges; the lane; the shape; up to PMT_RIDER_RANGES byte ranges
 *                         [begin, end) read and written, begin == end: none), `node` is the index of the node; rides[i] = 1 where entry i rides */
#define PMT_RIDER_RANGES 5
typedef struct pmt_rider_entry {
    int32_t kind, lane;
    int64_t rows, cols;
    uint64_t reads[PMT_RIDER_RANGES][2], writes[PMT_RIDER_RANGES][2];
} pmt_rider_entry;
int pmt_plan_riders(const pmt_plan *plan, int *riders, int64_t *tiles);
int pmt_plan_rider_check(const pmt_rider_entry *tape, int64_t n, int64_t node, int *rides, int *riders, int64_t *tiles);
/* Inside a fused run a workgroup barrier stands only in front of a node that touches what an earlier node since the last barrier wrote
 * (or writes what one read): independent nodes — the Parameter callbacks; the objective's chain and a constraint's — share a PHASE.
 * Number of phases over all fused runs (README Example 1: 7 entries, 3 phases). */
int pmt_plan_fused_phases(const pmt_plan *plan);
/* workgroups of the plan's largest fused run (1 .. 32: one per 4096 elements of work beyond 8192, never more than HALF of what the CUs
 * of the plan's stream hold at once — occupancy calculator x the stream's CU mask / the partition's CU count; the barrier in front of a
 * dependent node is then a grid barrier on a counter the plan owns; a hipGraph replays every run with ONE workgroup).  At most one such
 * run is in flight per device: while another plan's is, a launch goes out on one workgroup (same results).  A grid barrier that still
 * times out (kernels of other processes holding the CUs) is reported by pmt_plan_synchronize / pmt_plan_fetch_synchronize / pmt_plan_check. */
int pmt_plan_fused_workgroups(const pmt_plan *plan);
/* update!(m::Model) of a SMALL model behind ONE call (csrc/modelrun.hip) — what src/model.jl:132-143 does per solve, for a host that
 * has recorded its model's tape in the small-model form:
 *   - setdirty! + the Parameter refresh (src/parameter.jl:93-104): a HOST-updated Parameter's value array is copied into its page-locked
 *     mailbox in the device layout (the tape's first entries copy mailbox -> Parameter buffer inside the one launch); a DEVICE-regenerated
 *     Parameter's seed word is advanced (word = base + stride * number of updates so far);
 *   - the re-evaluation + MOI copies (src/model.jl:134-143, src/moi_interop.jl:131-137,168-175): pmt_plan_update;
 *   - results: registered fetches (pmt_model_add_fetch) are enqueued behind the replay; with synchronize != 0 the call returns when the
 *     plan's stream is idle (pmt_plan_synchronize, incl. the fused runs' barrier error) and stores the registered constants
 *     (*dst = *src, e.g. MOI function .constant fields); with 0, pmt_model_wait does that later.
 * A pmt_model owns nothing: plan, mailboxes, seed words, host arrays stay the caller's and must outlive it.
 *   pmt_model_add_mailbox   `host`: rows x cols doubles with strides (row_stride, col_stride) in doubles — Julia Matrix: (1, size(A, 1)),
 *                           numpy C order: (shape[1], 1); cols == 0: a vector / scalar.  `mailbox`: `ld` doubles per column.  *out_slot = the
 *                           slot's index (registration order) = its byte in pmt_model_update's dirty mask
 *   pmt_model_set_host      the value array moved (an out-of-place callback returned a new array)
 *   pmt_model_update        dirty: one byte per slot, or NULL = every slot changed (setdirty!(model) + callbacks that always write).
 *                           A mailbox is only rewritten after the previous replay has been waited for (the launch reads it). */
typedef struct pmt_model pmt_model;
int pmt_model_create(pmt_plan *plan, pmt_model **out);
int pmt_model_destroy(pmt_model *model);
int pmt_model_add_mailbox(pmt_model *model, const double *host, int64_t rows, int64_t cols, int64_t row_stride, int64_t col_stride,
                          double *mailbox, int64_t ld, int *out_slot);
int pmt_model_add_seed(pmt_model *model, uint64_t *seed_word, uint64_t base, uint64_t stride, int *out_slot);
int pmt_model_set_host(pmt_model *model, int slot, const double *host);
int pmt_model_add_constant(pmt_model *model, const double *src, double *dst);
int pmt_model_add_fetch(pmt_model *model, void *host_dst, const void *device_src, size_t bytes);
int pmt_model_num_slots(const pmt_model *model);
int pmt_model_update(pmt_model *model, const unsigned char *dirty, int nslots, int synchronize);
int pmt_model_wait(pmt_model *model);
/* replay the tape on the plan's stream: one update!(m::Model) (src/model.jl:132-143) — the loop over FunctionWrapper calls
 * (src/FunctionWrappersQuickFix.jl:108-126) becomes a loop over recorded launches; after pmt_plan_instantiate_graph, one hipGraph launch */
int pmt_plan_update(pmt_plan *plan);
int pmt_plan_instantiate_graph(pmt_plan *plan);

#ifdef __cplusplus
}
#endif
#endif
