// Separable sums: an objective whose least-squares blocks and forms fall into groups over pairwise disjoint Variable vectors
// (transpose(x)*Q*x + transpose(u)*R*u).  No pair (j, k) is shared between two groups, so the reference's canonicalize!
// (src/functions.jl:381-386) combines nothing across them: the canonical function is the groups' own canonical functions interleaved in
// (row, col) order.  Every group is written by the entry points it would be written by alone (gram.hip, form.hip, gram_sum.hip) — straight
// into its slice of the MOI buffers when its variables are consecutive in the sorted union z, into an arena otherwise.  This file holds
// what is left: the placement of arena rows (pmt_quad_groups_gather_f64) and the sum of the groups' constants (pmt_quad_groups_constant_f64).
#include "streams.h"

namespace pmt {

typedef unsigned long long u64w;
typedef u64w u64w2 __attribute__((ext_vector_type(2)));

constexpr int GATHER_CHUNKS = 8;                       // 16-byte chunks per thread
constexpr int GATHER_BLOCK_CHUNKS = 256 * GATHER_CHUNKS;

// the row that holds destination word q: the largest r in lo .. hi with row_dst[r] <= q
__device__ __forceinline__ int64_t gather_row(const int64_t *__restrict__ row_dst, int64_t lo, int64_t hi, int64_t q) {
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (row_dst[mid] <= q) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Destination row r is the words row_dst[r] .. row_dst[r + 1] - 1 of `dst`, copied from src[row_src[r] ..].  The work is dealt out by
// destination WORDS (the short rows at the end of a triangle would leave a wave per row idle): a workgroup takes 4096 consecutive words,
// finds the rows they lie in by bisection of the prefix table — restricted to the few rows its own words touch — and writes 16-byte chunks
// at 16-byte-aligned addresses (a leading / trailing single word as in wave_write_words, common.h).  The two words of a chunk are loaded
// one by one: a source segment may start at the other parity than its destination, and a chunk may straddle two rows.
// Blocks quad_blocks .. : the linear terms, one 16-byte term per thread.
__global__ __launch_bounds__(256) void groups_gather_kernel(const u64w *__restrict__ src, const int64_t *__restrict__ row_src,
                                                            const int64_t *__restrict__ row_dst, int64_t nrows, int64_t nwords,
                                                            u64w *__restrict__ dst, int64_t quad_blocks, const LT *__restrict__ src_lin,
                                                            const int64_t *__restrict__ lin_src, int64_t nlin, LT *__restrict__ out_lin) {
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    if (b >= quad_blocks) {
        const int64_t j = (b - quad_blocks) * 256 + tid;
        if (j < nlin) out_lin[j] = src_lin[lin_src[j]];
        return;
    }
    const int64_t lead = (int64_t)((reinterpret_cast<uintptr_t>(dst) >> 3) & 1);
    const int64_t w_lo = b == 0 ? 0 : lead + 2 * b * GATHER_BLOCK_CHUNKS;
    if (w_lo >= nwords) return;
    int64_t w_hi = lead + 2 * (b + 1) * GATHER_BLOCK_CHUNKS;
    w_hi = (w_hi < nwords ? w_hi : nwords) - 1;
    const int64_t r_lo = gather_row(row_dst, 0, nrows - 1, w_lo);
    const int64_t r_hi = gather_row(row_dst, r_lo, nrows - 1, w_hi);
    if (lead && b == 0 && tid == 0) dst[0] = src[row_src[r_lo]];
#pragma unroll 2
    for (int i = 0; i < GATHER_CHUNKS; ++i) {
        const int64_t q0 = lead + 2 * (b * GATHER_BLOCK_CHUNKS + (int64_t)i * 256 + tid);
        if (q0 >= nwords) break;
        const int64_t r = gather_row(row_dst, r_lo, r_hi, q0);
        const int64_t s0 = row_src[r] + (q0 - row_dst[r]);
        const u64w x = src[s0];
        if (q0 + 1 < nwords) {
            int64_t s1 = s0 + 1;
            if (q0 + 1 >= row_dst[r + 1]) {             // the chunk's second word opens the next row that has words
                int64_t r1 = r + 1;
                while (r1 + 1 < nrows && row_dst[r1 + 1] <= q0 + 1) ++r1;
                s1 = row_src[r1];
            }
            u64w2 v;
            v.x = x;
            v.y = src[s1];
            *reinterpret_cast<u64w2 *>(dst + q0) = v;
        } else {
            dst[q0] = x;
        }
    }
}

// ((c_1 + c_2) + ..) + c_G, one thread
__global__ void groups_constant_kernel(const double *__restrict__ consts, int ngroups, double *out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = consts[0];
    for (int g = 1; g < ngroups; ++g) s = s + consts[g];
    *out = s;
}

}  // namespace pmt

using namespace pmt;

extern "C" int pmt_quad_groups_gather_f64(const pmt_quadratic_term *src_quad, const int64_t *row_src, const int64_t *row_dst, int64_t nrows,
                                          int64_t nterms, const pmt_linear_term *src_lin, const int64_t *lin_src, int64_t nlin,
                                          pmt_quadratic_term *out_quad, pmt_linear_term *out_lin, void *stream) {
    PMT_REQUIRE(nrows >= 0 && nterms >= 0 && nlin >= 0, PMT_DIMENSION_MISMATCH, "quad_groups_gather: negative size");
    PMT_REQUIRE(nterms >= nrows && (nrows > 0 || nterms == 0), PMT_DIMENSION_MISMATCH, "quad_groups_gather: fewer terms than rows (a row holds at least one)");
    PMT_REQUIRE(nterms < ((int64_t)1 << 40) && nlin < ((int64_t)1 << 38), PMT_DIMENSION_MISMATCH, "quad_groups_gather: sizes beyond one launch");
    PMT_REQUIRE(nterms == 0 || (src_quad && row_src && row_dst && out_quad), PMT_INVALID_ARGUMENT, "quad_groups_gather: null quadratic table or array");
    PMT_REQUIRE(nlin == 0 || (src_lin && lin_src && out_lin), PMT_INVALID_ARGUMENT, "quad_groups_gather: null linear table or array");
    const int64_t nwords = 3 * nterms;
    // (one chunk more than nwords / 2: the chunks start behind a leading word when out_quad is 8 mod 16)
    const int64_t quad_blocks = nterms ? cdiv(nwords / 2 + 1, GATHER_BLOCK_CHUNKS) : 0;
    const int64_t blocks = quad_blocks + cdiv(nlin, 256);
    if (blocks == 0) return PMT_OK;
    return dispatch(stream, [=](hipStream_t s) {
        PMT_LAUNCH(groups_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<const u64w *>(src_quad), row_src, row_dst, nrows,
                   nwords, reinterpret_cast<u64w *>(out_quad), quad_blocks, src_lin, lin_src, nlin, out_lin);
        return check_launch("groups_gather_kernel");
    });
}

extern "C" int pmt_quad_groups_constant_f64(const double *group_consts, int ngroups, double *out_const, void *stream) {
    PMT_REQUIRE(ngroups >= 1 && ngroups <= PMT_QUAD_MAX_GROUPS, PMT_INVALID_ARGUMENT, "quad_groups_constant: 1 .. 8 groups");
    PMT_REQUIRE(group_consts && out_const, PMT_INVALID_ARGUMENT, "quad_groups_constant: null pointer");
    return dispatch(stream, [=](hipStream_t s) {
        // the groups' constants are written by their own constant steps, which a plan's replay may have queued behind deferred stream-K
        // constants (gram_sum.hip): this launch queues behind them the same way
        return gram_after_deferred(s, [=]() -> int {
            PMT_LAUNCH(groups_constant_kernel, dim3(1), dim3(64), 0, s, group_consts, ngroups, out_const);
            return check_launch("groups_constant_kernel");
        });
    });
}
