// Dense affine nodes: A*x (+|-) b  ->  Vector{AffineFunction} term block (LinearTerm AoS) or, fused with
// the MOI copy, MOI.VectorAffineTerm AoS.  HBM-bound streaming transpose (column-major in, row-major out).
//
// Reference loops replaced (see include/parametron_hip.h):
//   matvecmul!    src/functions.jl:775-798      vecadd!/vecsubtract!  src/functions.jl:751-764
//   update!(::MOI.VectorAffineFunction, ...)    src/moi_interop.jl:64-81
//
// Kernel shape (gfx950): 64x64 tile per 256-thread workgroup.  Loads: each half-wave reads one column
// segment of 64 rows as 32 x 16 B (512 B contiguous).  The tile is transposed through LDS (pitch 65
// doubles) and written row-major; every wave store instruction covers one contiguous 1 KiB (LinearTerm)
// or 1 KiB-chunks of the 1.5 KiB row segment (24-byte VectorAffineTerm, assembled as 16-byte chunks so
// that all stores are global_store_dwordx4).  Algorithmic bytes: 8 read + 16 (LT) / 24 (VAT) written
// per matrix entry.
#include "affine_tile.h"

namespace pmt {

// NTL (nontemporal loads of the matrix): measured (profiles/r04_batch_small.txt section 3, r04_affine_pack_nt.txt) — a matrix that is still in
// the Infinity Cache is read 16 % slower with the policy, a cold one faster.  The MOI pack of a LARGE constraint block runs behind the
// objective's contraction, which has streamed ~1 GB through the cache since the block was last touched: it is always cold there, and the
// policy takes the in-step launch of config 2's 512 x 4096 block from 15.4 to ~13.8 us.  Small blocks and the LinearTerm form keep plain loads.
constexpr int64_t NTL_MIN_BYTES = 8 << 20;

// MODE 0: LinearTerm output   MODE 1: VectorAffineTerm output
// TR: rows per tile (64, or 32 for blocks that would otherwise give fewer than ~4 workgroups per CU: the 512 x 4096 constraint block
// of config 2 is 512 tiles of 64 x 64 — two per CU, 8 waves, tail-dominated: 19 us inside the step against 13 us when it had the
// chip to itself; with 32-row tiles 1024 workgroups of half the LDS)
template <int MODE, bool NT, int TR, bool NTL = false>
__global__ __launch_bounds__(256) void affine_tile_kernel(
    const double *__restrict__ A, int64_t lda, int64_t rows, int64_t cols,
    const int64_t *__restrict__ xvar, const double *__restrict__ b, int sign,
    const int64_t *__restrict__ varmap, int64_t row_offset,
    u64 *__restrict__ out, double *__restrict__ out_consts, int vec_in, int vec_out, u64 *stamps, unsigned stamp_cap) {
    __shared__ double tile[TR * PITCH];
    __shared__ u64 vmx[TILE];

    const int t = threadIdx.x;
    // measurement hook (pmt_profile_kernel_stamps; null in production): this workgroup's start on the device's constant-rate clock, into
    // its own slot (plain stores — atomics of a thousand workgroups on one word serialise and triple the launch)
    const unsigned wg = blockIdx.y * gridDim.x + blockIdx.x;
    if (stamps && t == 0 && wg < stamp_cap) stamps[2 * wg] = (u64)wall_clock64();
    // (the tile itself: affine_tile.h, shared with the riders of the one-launch Gram node)
    affine_tile_body<MODE, NT, TR, NTL>(A, lda, rows, cols, xvar, b, sign, varmap, row_offset, out, out_consts, vec_in, vec_out,
                                        (int)blockIdx.x, (int)blockIdx.y, t, tile, vmx);
    if (stamps) {                    // ... and the latest workgroup end, behind this workgroup's stores
        __syncthreads();
        if (t == 0 && wg < stamp_cap) {
            __builtin_amdgcn_s_waitcnt(0);
            stamps[2 * wg + 1] = (u64)wall_clock64();
        }
    }
}

// x (+|-) v for x::Vector{Variable}
__global__ void vars_addsub_kernel(const int64_t *__restrict__ xvar, int64_t n, const double *__restrict__ v, int sign,
                                   const int64_t *__restrict__ varmap, int64_t row_offset,
                                   LT *__restrict__ out_lt, VAT *__restrict__ out_vat, double *__restrict__ out_consts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t var = xvar[i];
    if (out_lt) { LT t; t.coeff = 1.0; t.var = var; out_lt[i] = t; }
    if (out_vat) { VAT t; t.output_index = row_offset + i + 1; t.coeff = 1.0; t.var = map_var(varmap, var); out_vat[i] = t; }
    if (out_consts) out_consts[i] = signed_const(v ? v[i] : 0.0, v ? sign : 0);
}

__global__ void consts_kernel(const double *__restrict__ d, int64_t n, int sign, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = signed_const(d[i], sign);
}

// "Background" form of the MOI constraint pack (same output as affine_tile_kernel<VAT>): at most 16 VGPRs and no LDS, so that its
// waves are CO-RESIDENT with the persistent Gram kernel, which leaves 16 of a SIMD's 512 VGPRs free (gram.hip) — on the plan's side
// lane it then runs inside the contraction instead of behind it.  One wave per (row, 256-column chunk); lanes read one element of
// 64 different columns (8-byte reads, one cache line each — the 8 rows that share those lines are handled by the next 7 waves, so
// they come from L2) and write their 24-byte term.  Slow on its own (it is not the kernel to use on an idle chip), free where it runs.
__global__ __launch_bounds__(256) void affine_pack_background_kernel(const double *__restrict__ A, int64_t lda, int rows, int cols,
                                                                     const int64_t *__restrict__ xvar, const int64_t *__restrict__ varmap,
                                                                     int64_t row_offset, unsigned long long *__restrict__ out) {
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int chunk = wave / rows, row = wave - chunk * rows;
    const int c0 = chunk * 256 + lane;
    const double *a = A + row;
    unsigned long long *o = out + (int64_t)row * cols * 3;
    const unsigned long long rowword = (unsigned long long)(row_offset + row + 1);
#pragma unroll 1
    for (int c = c0; c < min(cols, chunk * 256 + 256); c += 64) {
        const double v = a[(int64_t)c * lda];
        const int64_t var = map_var(varmap, xvar[c]);
        unsigned long long *p = o + (int64_t)c * 3;
        p[0] = rowword;
        p[1] = (unsigned long long)__double_as_longlong(v);
        p[2] = (unsigned long long)var;
    }
}

// ---- MOI copies of materialised native functions (src/moi_interop.jl:35-81)
__global__ void pack_scalar_affine_kernel(const LT *__restrict__ in, int64_t n, const int64_t *__restrict__ varmap, LT *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    LT t = in[i];
    t.var = map_var(varmap, t.var);
    out[i] = t;
}
// 256 consecutive terms per workgroup: the 24-byte structs come in and go out as 16-byte chunks through LDS (a per-thread struct
// copy is three strided 8-byte accesses each way); falls back to the per-thread form for unaligned buffers
__global__ __launch_bounds__(256) void pack_scalar_quadratic_kernel(const QT *__restrict__ in, int64_t n, const int64_t *__restrict__ varmap,
                                                                    QT *__restrict__ out, int aligned) {
    typedef unsigned long long u64;
    typedef u64 u64x2 __attribute__((ext_vector_type(2)));
    __shared__ u64 words[256 * 3];
    const int64_t base = (int64_t)blockIdx.x * 256;
    const int cnt = (int)min((int64_t)256, n - base);
    const int tid = threadIdx.x;
    if (aligned && cnt == 256) {
        const u64x2 *src = reinterpret_cast<const u64x2 *>(in + base);
        u64x2 *sw = reinterpret_cast<u64x2 *>(words);
        sw[tid] = src[tid];
        if (tid < 128) sw[256 + tid] = src[256 + tid];
        __syncthreads();
        const double c = __longlong_as_double((long long)words[3 * tid]);
        const int64_t r = (int64_t)words[3 * tid + 1], cl = (int64_t)words[3 * tid + 2];
        const double cm = (r == cl) ? 2 * c : c;                 // moi_interop.jl:58 (each thread rewrites its own three words)
        words[3 * tid] = (u64)__double_as_longlong(cm);
        words[3 * tid + 1] = (u64)map_var(varmap, r);
        words[3 * tid + 2] = (u64)map_var(varmap, cl);
        __syncthreads();
        u64x2 *dst = reinterpret_cast<u64x2 *>(out + base);
        dst[tid] = sw[tid];
        if (tid < 128) dst[256 + tid] = sw[256 + tid];
        return;
    }
    if (tid < cnt) {
        QT t = in[base + tid];
        QT o;
        o.coeff = (t.row == t.col) ? 2 * t.coeff : t.coeff;     // moi_interop.jl:58
        o.row = map_var(varmap, t.row);
        o.col = map_var(varmap, t.col);
        out[base + tid] = o;
    }
}
// one wave per row (handles ragged rows through row_ptr): 64 terms at a time through LDS, written as 16-byte chunks
__global__ __launch_bounds__(256) void pack_vector_affine_kernel(const LT *__restrict__ in, const int64_t *__restrict__ row_ptr, int64_t rows,
                                                                 int64_t row_len, const int64_t *__restrict__ varmap, int64_t row_offset,
                                                                 VAT *__restrict__ out) {
    typedef unsigned long long u64;
    __shared__ u64 s_c[4][64], s_v[4][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= rows) return;                                     // (no workgroup barrier below: waves are independent)
    const int64_t beg = row_ptr ? row_ptr[row] : row * row_len;
    const int64_t end = row_ptr ? row_ptr[row + 1] : beg + row_len;
    const u64 rowword = (u64)(row_offset + row + 1);
    for (int64_t ts = beg; ts < end; ts += 64) {
        const int cnt = (int)min((int64_t)64, end - ts);
        if (lane < cnt) {
            const LT t = in[ts + lane];
            s_c[wave][lane] = (u64)__double_as_longlong(t.coeff);
            s_v[wave][lane] = (u64)map_var(varmap, t.var);
        }
        __builtin_amdgcn_wave_barrier();
        wave_write_words<3>(reinterpret_cast<u64 *>(out) + ts * 3, cnt, lane, [&](int q) -> u64 {
            const int t = q / 3, f = q - 3 * t;
            return f == 0 ? rowword : (f == 1 ? s_c[wave][t] : s_v[wave][t]);
        });
        __builtin_amdgcn_wave_barrier();
    }
}

static int validate_affine(const double *A, int64_t lda, int64_t rows, int64_t cols, const int64_t *xvar, const double *b,
                           int sign, const void *out_terms) {
    PMT_REQUIRE(rows >= 0 && cols >= 0, PMT_DIMENSION_MISMATCH, "affine: negative dimension");
    PMT_REQUIRE(lda >= rows, PMT_DIMENSION_MISMATCH, "affine: lda < rows");
    PMT_REQUIRE(sign >= -1 && sign <= 1, PMT_INVALID_ARGUMENT, "affine: sign must be -1, 0 or +1");
    if (rows > 0 && cols > 0) {
        PMT_REQUIRE(A && xvar && out_terms, PMT_INVALID_ARGUMENT, "affine: null pointer");
    }
    PMT_REQUIRE(sign == 0 || b || rows == 0, PMT_INVALID_ARGUMENT, "affine: sign != 0 needs b");
    return PMT_OK;
}
// The tile kernel's grid has one block row per tile row and does not wrap: 65535 block rows is what the literal term builders launch at
// most (quad.hip), and nothing larger has been run.  Beyond it (64-row tiles: such a block has 1024 tiles or more) the shape is refused
// before anything is launched or recorded, instead of leaving it to the launch.
constexpr int64_t AFFINE_MAX_TILE_ROWS = 65535;
static int validate_affine_tiles(int64_t rows, int64_t cols) {
    PMT_REQUIRE(cols == 0 || cdiv(rows, TILE) <= AFFINE_MAX_TILE_ROWS, PMT_DIMENSION_MISMATCH,
                "affine: more than 65535 * 64 rows in one dense block");
    return PMT_OK;
}

// term buffers are write-once streams: non-temporal stores (tuning builds can switch them off with PMT_NONTEMPORAL=0)
static bool env_nt() {
#ifdef PMT_TUNING
    static int v = -1;
    if (v < 0) { const char *e = getenv("PMT_NONTEMPORAL"); v = (e && e[0] == '0') ? 0 : 1; }
    return v != 0;
#else
    return true;
#endif
}

// pmt_profile_kernel_stamps: device words {start, end} per workgroup the affine tile kernel of the NEXT launches reports into
static u64 *g_stamps = nullptr;
static unsigned g_stamp_cap = 0;

// small blocks: 32-row tiles, twice the workgroups (see the kernel's comment); ~1024 = 4 per CU is where 64-row tiles start to fill the chip
static bool affine_small_tiles(int64_t rows, int64_t cols) { return cdiv(cols, TILE) * cdiv(rows, TILE) < 1024 && rows > 32; }
// the MOI pack of a block this large reads its matrix with the nontemporal policy (NTL_MIN_BYTES)
static bool affine_cold(int64_t rows, int64_t cols) { return rows * cols * (int64_t)sizeof(double) >= NTL_MIN_BYTES; }

template <int MODE>
static int launch_affine(const double *A, int64_t lda, int64_t rows, int64_t cols, const int64_t *xvar, const double *b, int sign,
                         const int64_t *varmap, int64_t row_offset, void *out_terms, double *out_consts, hipStream_t s) {
    if (rows == 0 || cols == 0) return PMT_OK;   // cols == 0 (constants only) is handled by the callers
    const int vec_in = ((reinterpret_cast<uintptr_t>(A) & 15) == 0 && (lda & 1) == 0) ? 1 : 0;
    const int vec_out = ((reinterpret_cast<uintptr_t>(out_terms) & 15) == 0 && (cols & 1) == 0) ? 1 : 0;
    const char *name = MODE == 0 ? "affine_tile_kernel<LT>" : "affine_tile_kernel<VAT>";
    u64 *out = reinterpret_cast<u64 *>(out_terms);
    const bool small = affine_small_tiles(rows, cols);
    const bool ntl = MODE == 1 && affine_cold(rows, cols);
    u64 *stamps = MODE == 1 ? g_stamps : nullptr;
#define AFFINE_LAUNCH(NTV, TRV, NTLV)                                                                                                    \
    PMT_LAUNCH_NAMED(name, (affine_tile_kernel<MODE, NTV, TRV, NTLV>), dim3((unsigned)cdiv(cols, TILE), (unsigned)cdiv(rows, TRV)), dim3(256), 0, s, A, \
                     lda, rows, cols, xvar, b, sign, varmap, row_offset, out, out_consts, vec_in, vec_out, stamps, g_stamp_cap)
    if constexpr (MODE == 1) {
        if (ntl) {
            if (small) AFFINE_LAUNCH(true, 32, true); else AFFINE_LAUNCH(true, 64, true);
            return check_launch("affine_tile_kernel");
        }
    }
    if (env_nt()) { if (small) AFFINE_LAUNCH(true, 32, false); else AFFINE_LAUNCH(true, 64, false); }
    else { if (small) AFFINE_LAUNCH(false, 32, false); else AFFINE_LAUNCH(false, 64, false); }
#undef AFFINE_LAUNCH
    return check_launch("affine_tile_kernel");
}

// the pack as a rider of the one-launch Gram node (affine_tile.h): what launch_affine<1> would choose for it
int64_t affine_rider_tiles(int64_t rows, int64_t cols) {
    if (rows <= 0 || cols <= 0) return 0;
    return cdiv(cols, TILE) * cdiv(rows, affine_small_tiles(rows, cols) ? 32 : 64);
}
bool affine_rider(const SmallNode &nd, AffineRider *r) {
    const int64_t lda = nd.d[0], rows = nd.d[1], cols = nd.d[2];
    if (nd.op != SOP_AFFINE_VAT || rows <= 0 || cols <= 0) return false;
    r->A = static_cast<const double *>(nd.in[0]); r->lda = lda; r->rows = rows; r->cols = cols;
    r->xvar = static_cast<const int64_t *>(nd.in[1]); r->b = static_cast<const double *>(nd.in[2]);
    r->varmap = static_cast<const int64_t *>(nd.in[3]); r->row_offset = nd.d[3];
    r->out = static_cast<u64 *>(nd.out[0]); r->out_consts = static_cast<double *>(nd.out[1]);
    r->sign = nd.sign;
    r->vec_in = ((reinterpret_cast<uintptr_t>(r->A) & 15) == 0 && (lda & 1) == 0) ? 1 : 0;
    r->vec_out = ((reinterpret_cast<uintptr_t>(r->out) & 15) == 0 && (cols & 1) == 0) ? 1 : 0;
    r->tr = affine_small_tiles(rows, cols) ? 32 : 64;
    r->ntl = affine_cold(rows, cols) ? 1 : 0;
    r->nt = (r->ntl || env_nt()) ? 1 : 0;
    r->tiles_x = (int)cdiv(cols, TILE);
    r->first_tile = 0;
    return true;
}

}  // namespace pmt

using namespace pmt;

extern "C" int pmt_profile_kernel_stamps(void *device_words, int64_t workgroups) {
    PMT_REQUIRE(workgroups >= 0 && workgroups < ((int64_t)1 << 31), PMT_INVALID_ARGUMENT, "profile_kernel_stamps: bad capacity");
    g_stamps = workgroups > 0 ? reinterpret_cast<u64 *>(device_words) : nullptr;
    g_stamp_cap = g_stamps ? (unsigned)workgroups : 0;
    return PMT_OK;
}

extern "C" int pmt_device_clock_khz(int device, int *khz) {
    PMT_REQUIRE(khz, PMT_INVALID_ARGUMENT, "device_clock_khz: null pointer");
    PMT_HIP_CHECK(hipDeviceGetAttribute(khz, hipDeviceAttributeWallClockRate, device));
    return PMT_OK;
}

extern "C" int pmt_affine_assemble_f64(const double *A, int64_t lda, int64_t rows, int64_t cols, const int64_t *xvar, const double *b,
                                       int sign, pmt_linear_term *out_terms, double *out_consts, void *stream) {
    int rc = validate_affine(A, lda, rows, cols, xvar, b, sign, out_terms);
    if (rc) return rc;
    if ((rc = validate_affine_tiles(rows, cols))) return rc;
    if (cols == 0 && rows > 0 && out_consts)
        return b && sign ? pmt_consts_f64(b, rows, sign, out_consts, stream)
                         : dispatch(stream, [=](hipStream_t s) { PMT_HIP_CHECK(hipMemsetAsync(out_consts, 0, rows * sizeof(double), s)); return PMT_OK; });
    SmallNode nd;
    nd.op = SOP_AFFINE_LT; nd.sign = sign; nd.d[0] = lda; nd.d[1] = rows; nd.d[2] = cols; nd.d[3] = 0;
    nd.in[0] = A; nd.in[1] = xvar; nd.in[2] = b; nd.out[0] = out_terms; nd.out[1] = out_consts; nd.work = rows * cols + rows;
    return dispatch(stream, [=](hipStream_t s) {
        return launch_affine<0>(A, lda, rows, cols, xvar, b, sign, nullptr, 0, out_terms, out_consts, s);
    }, nd);
}

extern "C" int pmt_affine_pack_vector_f64(const double *A, int64_t lda, int64_t rows, int64_t cols, const int64_t *xvar, const double *b,
                                          int sign, const int64_t *varmap, int64_t row_offset, pmt_vector_affine_term *out_terms,
                                          double *out_consts, void *stream) {
    int rc = validate_affine(A, lda, rows, cols, xvar, b, sign, out_terms);
    if (rc) return rc;
    if ((rc = validate_affine_tiles(rows, cols))) return rc;
    if (cols == 0 && rows > 0 && out_consts)
        return b && sign ? pmt_consts_f64(b, rows, sign, out_consts, stream)
                         : dispatch(stream, [=](hipStream_t s) { PMT_HIP_CHECK(hipMemsetAsync(out_consts, 0, rows * sizeof(double), s)); return PMT_OK; });
    SmallNode nd;
    nd.op = SOP_AFFINE_VAT; nd.sign = sign; nd.d[0] = lda; nd.d[1] = rows; nd.d[2] = cols; nd.d[3] = row_offset;
    nd.in[0] = A; nd.in[1] = xvar; nd.in[2] = b; nd.in[3] = varmap; nd.out[0] = out_terms; nd.out[1] = out_consts; nd.work = rows * cols + rows;
    return dispatch(stream, [=](hipStream_t s) {
        return launch_affine<1>(A, lda, rows, cols, xvar, b, sign, varmap, row_offset, out_terms, out_consts, s);
    }, nd);
}

extern "C" int pmt_affine_pack_vector_background_f64(const double *A, int64_t lda, int64_t rows, int64_t cols, const int64_t *xvar, const double *b,
                                                     int sign, const int64_t *varmap, int64_t row_offset, pmt_vector_affine_term *out_terms,
                                                     double *out_consts, void *stream) {
    int rc = validate_affine(A, lda, rows, cols, xvar, b, sign, out_terms);
    if (rc) return rc;
    PMT_REQUIRE(rows < (1 << 30) && cols < (1 << 30) && cdiv(cols, 256) * rows < ((int64_t)1 << 31), PMT_DIMENSION_MISMATCH,
                "affine_pack_vector_background: block too large");
    if (rows > 0 && out_consts) {
        rc = b && sign ? pmt_consts_f64(b, rows, sign, out_consts, stream)
                       : dispatch(stream, [=](hipStream_t s) { PMT_HIP_CHECK(hipMemsetAsync(out_consts, 0, rows * sizeof(double), s)); return PMT_OK; });
        if (rc) return rc;
    }
    if (rows == 0 || cols == 0) return PMT_OK;
    return dispatch(stream, [=](hipStream_t s) {
        const int64_t waves = cdiv(cols, 256) * rows;
        PMT_LAUNCH(affine_pack_background_kernel, dim3((unsigned)cdiv(waves, 4)), dim3(256), 0, s, A, lda, (int)rows, (int)cols, xvar, varmap, row_offset,
                   reinterpret_cast<unsigned long long *>(out_terms));
        return check_launch("affine_pack_background_kernel");
    });
}

extern "C" int pmt_vars_addsub_f64(const int64_t *xvar, int64_t n, const double *v, int sign, const int64_t *varmap, int64_t row_offset,
                                   pmt_linear_term *out_terms_lt, pmt_vector_affine_term *out_terms_vat, double *out_consts, void *stream) {
    PMT_REQUIRE(n >= 0, PMT_DIMENSION_MISMATCH, "vars_addsub: negative length");
    PMT_REQUIRE(sign >= -1 && sign <= 1, PMT_INVALID_ARGUMENT, "vars_addsub: sign must be -1, 0 or +1");
    if (n == 0) return PMT_OK;
    PMT_REQUIRE(xvar, PMT_INVALID_ARGUMENT, "vars_addsub: null xvar");
    PMT_REQUIRE(sign == 0 || v, PMT_INVALID_ARGUMENT, "vars_addsub: sign != 0 needs v");
    SmallNode nd;
    nd.op = SOP_VARS_ADDSUB; nd.sign = sign; nd.d[0] = n; nd.d[1] = row_offset; nd.in[0] = xvar; nd.in[1] = v; nd.in[2] = varmap;
    nd.out[0] = out_terms_lt; nd.out[1] = out_terms_vat; nd.out[2] = out_consts; nd.work = n;
    return dispatch(stream, [=](hipStream_t s) {
        PMT_LAUNCH(vars_addsub_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, xvar, n, v, sign, varmap, row_offset,
                           out_terms_lt, out_terms_vat, out_consts);
        return check_launch("vars_addsub_kernel");
    }, nd);
}

extern "C" int pmt_consts_f64(const double *d, int64_t n, int sign, double *out, void *stream) {
    PMT_REQUIRE(n >= 0, PMT_DIMENSION_MISMATCH, "consts: negative length");
    if (n == 0) return PMT_OK;
    PMT_REQUIRE(d && out, PMT_INVALID_ARGUMENT, "consts: null pointer");
    SmallNode nd;
    nd.op = SOP_CONSTS; nd.sign = sign; nd.d[0] = n; nd.in[0] = d; nd.out[0] = out; nd.work = n;
    return dispatch(stream, [=](hipStream_t s) {
        PMT_LAUNCH(consts_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, d, n, sign, out);
        return check_launch("consts_kernel");
    }, nd);
}

extern "C" int pmt_pack_scalar_affine_f64(const pmt_linear_term *terms, int64_t n, const int64_t *varmap, pmt_linear_term *out_terms,
                                          void *stream) {
    PMT_REQUIRE(n >= 0, PMT_DIMENSION_MISMATCH, "pack_scalar_affine: negative length");
    if (n == 0) return PMT_OK;
    PMT_REQUIRE(terms && out_terms, PMT_INVALID_ARGUMENT, "pack_scalar_affine: null pointer");
    SmallNode nd;
    nd.op = SOP_PACK_SA; nd.d[0] = n; nd.in[0] = terms; nd.in[1] = varmap; nd.out[0] = out_terms; nd.work = n;
    return dispatch(stream, [=](hipStream_t s) {
        PMT_LAUNCH(pack_scalar_affine_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, terms, n, varmap, out_terms);
        return check_launch("pack_scalar_affine_kernel");
    }, nd);
}

extern "C" int pmt_pack_scalar_quadratic_f64(const pmt_quadratic_term *quad, int64_t nq, const int64_t *varmap,
                                             pmt_quadratic_term *out_quad, void *stream) {
    PMT_REQUIRE(nq >= 0, PMT_DIMENSION_MISMATCH, "pack_scalar_quadratic: negative length");
    if (nq == 0) return PMT_OK;
    PMT_REQUIRE(quad && out_quad, PMT_INVALID_ARGUMENT, "pack_scalar_quadratic: null pointer");
    SmallNode nd;
    nd.op = SOP_PACK_SQ; nd.d[0] = nq; nd.in[0] = quad; nd.in[1] = varmap; nd.out[0] = out_quad; nd.work = nq;
    return dispatch(stream, [=](hipStream_t s) {
        const int aligned = (((reinterpret_cast<uintptr_t>(quad) | reinterpret_cast<uintptr_t>(out_quad)) & 15) == 0) ? 1 : 0;
        PMT_LAUNCH(pack_scalar_quadratic_kernel, dim3((unsigned)cdiv(nq, 256)), dim3(256), 0, s, quad, nq, varmap, out_quad, aligned);
        return check_launch("pack_scalar_quadratic_kernel");
    }, nd);
}

extern "C" int pmt_pack_vector_affine_f64(const pmt_linear_term *terms, const int64_t *row_ptr, int64_t rows, int64_t row_len,
                                          const int64_t *varmap, int64_t row_offset, pmt_vector_affine_term *out_terms, void *stream) {
    PMT_REQUIRE(rows >= 0 && row_len >= 0, PMT_DIMENSION_MISMATCH, "pack_vector_affine: negative dimension");
    if (rows == 0) return PMT_OK;
    PMT_REQUIRE((terms && out_terms) || (!row_ptr && row_len == 0), PMT_INVALID_ARGUMENT, "pack_vector_affine: null pointer");
    SmallNode nd;
    nd.op = SOP_PACK_VA; nd.d[0] = rows; nd.d[1] = row_len; nd.d[2] = row_offset; nd.in[0] = terms; nd.in[1] = row_ptr; nd.in[2] = varmap;
    nd.out[0] = out_terms;
    // (ragged rows: the term count is on the device; such a node joins a group only when its row count alone bounds it)
    nd.work = row_ptr ? SMALL_NODE_WORK_MAX + 1 : rows * row_len;
    return dispatch(stream, [=](hipStream_t s) {
        PMT_LAUNCH(pack_vector_affine_kernel, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, s, terms, row_ptr, rows, row_len, varmap,
                           row_offset, out_terms);
        return check_launch("pack_vector_affine_kernel");
    }, nd);
}
