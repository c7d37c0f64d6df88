// A residual over several Variable vectors as one dense block: the stacking node behind pmt_affine_stack_columns_f64.
//
// The reference builds r = A*x + B*u - b with vecadd! / vecsubtract! (src/functions.jl:751-764, rules src/lazyexpression.jl:238-258): the
// LinearTerms of every block row by row, which dot(r, r) then multiplies out.  Here the blocks stay the Parameter matrices they are, and this
// node copies their columns, signed, into one column-major matrix over the union z of the variables: [A B] (or [A -B], or any permutation of
// columns), which the Gram contraction (pmt_quad_gram_f64 and its family) then reads as it would read a Parameter holding that matrix.
//
// Bandwidth-bound: 8 bytes read and 8 written per element.  One workgroup per (column, 2048-row chunk); a lane moves 16-byte pairs along
// the column when source and destination columns share their 16-byte phase (every padded Parameter layout), 8-byte elements otherwise.
#include "common.h"

namespace pmt {

static_assert(sizeof(pmt_stack_column) == 16, "pmt_stack_column: 16 bytes (src, sign)");

constexpr int STACK_THREADS = 256;
constexpr int STACK_PAIRS = 4;                                          // 16-byte pairs per lane per chunk
constexpr int64_t STACK_ROWS = 2 * STACK_PAIRS * STACK_THREADS;         // 2048 rows per workgroup
constexpr int64_t STACK_MAX_GRID_Y = 65535;

__device__ __forceinline__ double stack_sign(double v, bool neg) { return neg ? -v : v; }

__global__ __launch_bounds__(STACK_THREADS) void stack_columns_kernel(const pmt_stack_column *__restrict__ table, int64_t rows,
                                                                       double *__restrict__ out, int64_t ldo) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    const int64_t c = blockIdx.x;
    const pmt_stack_column e = table[c];
    const double *__restrict__ src = e.src;
    const bool neg = e.sign < 0;
    double *__restrict__ dst = out + c * ldo;
    const int tid = threadIdx.x;
    const int sp = (int)((reinterpret_cast<uintptr_t>(src) >> 3) & 1), dp = (int)((reinterpret_cast<uintptr_t>(dst) >> 3) & 1);
    for (int64_t r0 = (int64_t)blockIdx.y * STACK_ROWS; r0 < rows; r0 += (int64_t)gridDim.y * STACK_ROWS) {
        const int64_t r1 = r0 + STACK_ROWS < rows ? r0 + STACK_ROWS : rows;
        if (sp != dp) {
            for (int64_t i = r0 + tid; i < r1; i += STACK_THREADS) dst[i] = stack_sign(src[i], neg);
            continue;
        }
        // r0 is even: src + r0 and dst + r0 have the phase sp; the pairs start at the first 16-byte boundary
        const int64_t i0 = r0 + sp < r1 ? r0 + sp : r1;
        const int64_t npairs = (r1 - i0) / 2;
        if (tid == 0 && i0 > r0) dst[r0] = stack_sign(src[r0], neg);
        if (tid == STACK_THREADS - 1 && i0 + 2 * npairs < r1) dst[r1 - 1] = stack_sign(src[r1 - 1], neg);
        const d2 *__restrict__ s2 = reinterpret_cast<const d2 *>(src + i0);
        d2 *__restrict__ d2p = reinterpret_cast<d2 *>(dst + i0);
        d2 v[STACK_PAIRS];
#pragma unroll
        for (int k = 0; k < STACK_PAIRS; ++k) {
            const int64_t p = tid + (int64_t)k * STACK_THREADS;
            if (p < npairs) v[k] = s2[p];
        }
#pragma unroll
        for (int k = 0; k < STACK_PAIRS; ++k) {
            const int64_t p = tid + (int64_t)k * STACK_THREADS;
            if (p < npairs) {
                d2 w;
                w.x = stack_sign(v[k].x, neg);
                w.y = stack_sign(v[k].y, neg);
                d2p[p] = w;
            }
        }
    }
}

}  // namespace pmt

using namespace pmt;

extern "C" int pmt_affine_stack_columns_f64(const pmt_stack_column *cols, int64_t ncols, int64_t rows, double *out, int64_t ldo, void *stream) {
    PMT_REQUIRE(ncols >= 0 && rows >= 0, PMT_DIMENSION_MISMATCH, "affine_stack_columns: negative size");
    PMT_REQUIRE(ldo >= rows, PMT_DIMENSION_MISMATCH, "affine_stack_columns: ldo < rows");
    PMT_REQUIRE(ncols <= INT32_MAX, PMT_DIMENSION_MISMATCH, "affine_stack_columns: more than 2^31 - 1 columns");
    PMT_REQUIRE(cols || ncols == 0, PMT_INVALID_ARGUMENT, "affine_stack_columns: null column table");
    PMT_REQUIRE(out || ncols == 0 || rows == 0, PMT_INVALID_ARGUMENT, "affine_stack_columns: null output");
    return dispatch(stream, [=](hipStream_t s) {
        if (ncols == 0 || rows == 0) return (int)PMT_OK;
        const int64_t gy = cdiv(rows, STACK_ROWS) < STACK_MAX_GRID_Y ? cdiv(rows, STACK_ROWS) : STACK_MAX_GRID_Y;
        PMT_LAUNCH(stack_columns_kernel, dim3((unsigned)ncols, (unsigned)gy), dim3(STACK_THREADS), 0, s, cols, rows, out, ldo);
        return check_launch("stack_columns_kernel");
    });
}
