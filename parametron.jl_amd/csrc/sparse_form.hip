// Sparse quadratic form: transpose(x) * Q * x with Q a fixed-pattern n x n CSC matrix, as the canonical MOI function.
// The function is the reference's literal one minus the structural zeros: bilinearmul! (src/functions.jl:840-858) emitting a term
// (Q[r,c], x_r, x_c) for the stored entries only, canonicalize! (:381-386) and the MOI copy (src/moi_interop.jl:45-62):
//   one quadratic term per unordered pair {j, k}, j <= k, for which Q[j,k] or Q[k,j] is stored, sorted by (j, k):
//     Q[j,k] + Q[k,j] when both are stored, the one stored value unchanged otherwise, 2*Q[j,j] (moi) / Q[j,j] on the diagonal
//   no linear terms, constant 0.0
// Which pairs exist and which one or two entries of nzval each one reads depend on the pattern alone: the SYMBOLIC phase runs once per
// pattern on the host (pmt_sparse_form_count / _order) and leaves per output term its pair and two source words.  Per re-evaluation ONE
// launch streams those tables (16 bytes per term), gathers the one or two values and writes every 24-byte term once.
#include <new>
#include <vector>

#include "common.h"

namespace pmt {

constexpr int SF_NT = 256;
static_assert(PMT_SPARSE_SUM_WG_TERMS == SF_NT, "one output term per thread, the workgroup of the sparse combine");
constexpr uint32_t SF_NONE = 0xFFFFFFFFu;

// One term per thread: the four table words are read coalesced, the values gathered from nzval (small next to the tables and
// cache-resident), the 24-byte structs parked in LDS and written by each wave as 16-byte stores (sparse_gram_sum_kernel's way out).
__global__ __launch_bounds__(SF_NT) void sparse_form_kernel(const double *__restrict__ nzval, const uint32_t *__restrict__ src_a,
                                                            const uint32_t *__restrict__ src_b, const uint32_t *__restrict__ pair_j,
                                                            const uint32_t *__restrict__ pair_k, int64_t nq, const int64_t *__restrict__ xvar, int moi,
                                                            const int64_t *__restrict__ varmap, QT *__restrict__ out_quad,
                                                            double *__restrict__ out_const) {
    typedef unsigned long long u64w;
    __shared__ u64w s_w[3 * SF_NT];
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && tid == 0 && out_const) *out_const = 0.0;
    const int64_t s0 = (int64_t)blockIdx.x * SF_NT, s = s0 + tid;
    if (s < nq) {
        const uint32_t a = src_a[s], b = src_b[s], j = pair_j[s], k = pair_k[s];
        double c;
        if (a != SF_NONE && b != SF_NONE) {
            c = nzval[a] + nzval[b];
        } else {
            c = nzval[a != SF_NONE ? a : b];                     // the one stored value unchanged (no + 0.0: -0.0 stays -0.0)
            if (j == k && moi) c = 2.0 * c;                      // moi_interop.jl:58 doubles the diagonal
        }
        s_w[3 * tid] = (u64w)__double_as_longlong(c);
        s_w[3 * tid + 1] = (u64w)(moi ? map_var(varmap, xvar[j]) : xvar[j]);
        s_w[3 * tid + 2] = (u64w)(moi ? map_var(varmap, xvar[k]) : xvar[k]);
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    const int64_t w0 = s0 + 64 * wave;
    const int cnt = (int)(nq - w0 < 64 ? nq - w0 : 64);
    if (cnt > 0) {                                               // (an empty segment must not reach the leading-word store)
        const u64w *src = s_w + 3 * 64 * wave;
        wave_write_words<3>(reinterpret_cast<u64w *>(out_quad + w0), cnt, lane, [&](int q) -> u64w { return src[q]; });
    }
}

// ---- symbolic phase (host, once per pattern)
// checks the pattern: canonical CSC, 1-based, rows strictly ascending within a column and inside 1 .. n — nothing is written before this
static int sf_check(const char *who, int64_t n, const int64_t *colptr, const int64_t *rowval) {
    const std::string w(who);
    PMT_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), PMT_DIMENSION_MISMATCH, w + ": need 0 <= n < 2^31");
    PMT_REQUIRE(colptr, PMT_INVALID_ARGUMENT, w + ": null pointer");
    PMT_REQUIRE(colptr[0] == 1, PMT_INVALID_ARGUMENT, w + ": colptr must be 1-based");
    for (int64_t c = 0; c < n; ++c) PMT_REQUIRE(colptr[c + 1] >= colptr[c], PMT_INVALID_ARGUMENT, w + ": colptr not monotone");
    const int64_t nnz = colptr[n] - 1;
    PMT_REQUIRE(nnz < (int64_t)SF_NONE, PMT_DIMENSION_MISMATCH, w + ": 2^32 - 1 or more non-zeros");
    PMT_REQUIRE(nnz == 0 || rowval, PMT_INVALID_ARGUMENT, w + ": null pointer");
    for (int64_t c = 0; c < n; ++c) {
        int64_t prev = 0;
        for (int64_t p = colptr[c] - 1; p < colptr[c + 1] - 1; ++p) {
            const int64_t r = rowval[p];
            PMT_REQUIRE(r >= 1 && r <= n, PMT_DIMENSION_MISMATCH, w + ": row index outside 1 .. n");
            PMT_REQUIRE(r > prev, PMT_INVALID_ARGUMENT, w + ": rows must ascend strictly within a column");
            prev = r;
        }
    }
    return PMT_OK;
}

// The pairs of a checked pattern in (j, k) order.  The upper part (entries (j, k), k >= j) is needed by ROW: the transpose pattern of
// the upper part is built by a counting pass (ascending column => ascending column within each row).  The lower part (entries (k, j),
// k > j) is column j itself, rows ascending.  Row j of the upper part and column j of the lower part are walked together.  With
// pair_j == NULL the pairs are counted only; otherwise at most `cap` of them are written.  Returns the number of pairs.
static int64_t sf_walk(int64_t n, const int64_t *colptr, const int64_t *rowval, int64_t cap, uint32_t *pair_j, uint32_t *pair_k, uint32_t *src_a,
                       uint32_t *src_b) {
    std::vector<int64_t> row_ptr((size_t)n + 1, 0);
    for (int64_t c = 0; c < n; ++c)
        for (int64_t p = colptr[c] - 1; p < colptr[c + 1] - 1 && rowval[p] - 1 <= c; ++p) ++row_ptr[(size_t)rowval[p]];
    for (int64_t i = 0; i < n; ++i) row_ptr[(size_t)i + 1] += row_ptr[(size_t)i];
    const int64_t nup = row_ptr[(size_t)n];
    std::vector<uint32_t> ucol((size_t)nup), upos((size_t)nup);
    {
        std::vector<int64_t> cursor(row_ptr.begin(), row_ptr.end() - 1);
        for (int64_t c = 0; c < n; ++c)
            for (int64_t p = colptr[c] - 1; p < colptr[c + 1] - 1 && rowval[p] - 1 <= c; ++p) {
                const int64_t u = cursor[(size_t)(rowval[p] - 1)]++;
                ucol[(size_t)u] = (uint32_t)c;
                upos[(size_t)u] = (uint32_t)p;
            }
    }
    int64_t total = 0;
    for (int64_t j = 0; j < n; ++j) {
        int64_t u = row_ptr[(size_t)j];
        const int64_t ue = row_ptr[(size_t)j + 1];
        int64_t p = colptr[j] - 1;
        const int64_t pe = colptr[j + 1] - 1;
        while (p < pe && rowval[p] - 1 <= j) ++p;                // the lower part of column j: rows k > j
        while (u < ue || p < pe) {
            const int64_t ka = u < ue ? (int64_t)ucol[(size_t)u] : n, kb = p < pe ? rowval[p] - 1 : n;
            const int64_t k = ka < kb ? ka : kb;
            if (pair_j && total < cap) {
                pair_j[total] = (uint32_t)j;
                pair_k[total] = (uint32_t)k;
                src_a[total] = ka == k ? upos[(size_t)u] : SF_NONE;
                src_b[total] = kb == k ? (uint32_t)p : SF_NONE;
            }
            if (ka == k) ++u;
            if (kb == k) ++p;
            ++total;
        }
    }
    return total;
}

}  // namespace pmt

using namespace pmt;

extern "C" int pmt_sparse_form_count(int64_t n, const int64_t *colptr, const int64_t *rowval, int64_t *nq) try {
    PMT_REQUIRE(nq, PMT_INVALID_ARGUMENT, "sparse_form_count: null pointer");
    if (int rc = sf_check("sparse_form_count", n, colptr, rowval)) return rc;
    *nq = sf_walk(n, colptr, rowval, 0, nullptr, nullptr, nullptr, nullptr);
    return PMT_OK;
} catch (const std::bad_alloc &) {
    return pmt::fail(PMT_OUT_OF_MEMORY, "sparse_form_count: out of host memory");
}

extern "C" int pmt_sparse_form_order(int64_t n, const int64_t *colptr, const int64_t *rowval, int64_t nq, uint32_t *pair_j, uint32_t *pair_k,
                                     uint32_t *src_a, uint32_t *src_b) try {
    if (int rc = sf_check("sparse_form_order", n, colptr, rowval)) return rc;
    const int64_t want = sf_walk(n, colptr, rowval, 0, nullptr, nullptr, nullptr, nullptr);
    PMT_REQUIRE(nq == want, PMT_DIMENSION_MISMATCH, "sparse_form_order: nq is not this pattern's (pmt_sparse_form_count)");
    PMT_REQUIRE(nq == 0 || (pair_j && pair_k && src_a && src_b), PMT_INVALID_ARGUMENT, "sparse_form_order: null pointer");
    if (nq > 0) sf_walk(n, colptr, rowval, nq, pair_j, pair_k, src_a, src_b);
    return PMT_OK;
} catch (const std::bad_alloc &) {
    return pmt::fail(PMT_OUT_OF_MEMORY, "sparse_form_order: out of host memory");
}

extern "C" int pmt_sparse_form_f64(const double *nzval, const uint32_t *src_a, const uint32_t *src_b, const uint32_t *pair_j, const uint32_t *pair_k,
                                   int64_t nq, const int64_t *xvar, int moi, const int64_t *varmap, pmt_quadratic_term *out_quad, double *out_const,
                                   void *stream) {
    PMT_REQUIRE(nq >= 0, PMT_INVALID_ARGUMENT, "sparse_form: negative count");
    PMT_REQUIRE(moi == 0 || moi == 1, PMT_INVALID_ARGUMENT, "sparse_form: moi must be 0 or 1");
    PMT_REQUIRE(!moi || varmap, PMT_INVALID_ARGUMENT, "sparse_form: the MOI form needs varmap");
    PMT_REQUIRE(nq == 0 || (nzval && src_a && src_b && pair_j && pair_k && xvar && out_quad), PMT_INVALID_ARGUMENT, "sparse_form: null pointer");
    PMT_REQUIRE(cdiv(nq, SF_NT) < ((int64_t)1 << 31) - 1, PMT_DIMENSION_MISMATCH, "sparse_form: too many terms for one launch");
    if (nq == 0 && !out_const) return PMT_OK;                    // nothing to write
    return dispatch(stream, [=](hipStream_t s) {
        PMT_LAUNCH(sparse_form_kernel, dim3((unsigned)(nq > 0 ? cdiv(nq, SF_NT) : 1)), dim3(SF_NT), 0, s, nzval, src_a, src_b, pair_j, pair_k, nq, xvar,
                   moi, varmap, out_quad, out_const);
        return check_launch("sparse_form_kernel");
    });
}
