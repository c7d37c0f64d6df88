// Sparse least-squares objective: dot(r, r) with r = C*x (+|-) d and C a fixed-pattern CSC matrix, as the canonical MOI function.
// The reference has no sparse path (matvecmul!, src/functions.jl:775-798, walks every (row, col)), so — as for the sparse constraint node
// (sparse.hip) — the function is the reference's output minus the structural zeros: vecdot! (src/functions.jl:702-709 over :548-576) of
// rows that hold the structural terms only, canonicalize! (:381-386), then the MOI copy (src/moi_interop.jl:45-62).
//   quadratic term (j, k), j <= k, for every pair of columns that share a row:  2 * sum over the shared rows of C[i,j]*C[i,k]
//   linear term j for every non-empty column:                                   2 * sum_i C[i,j]*c_i,  c_i = 0.0 (+|-) d[i]
//   constant:                                                                   sum_i c_i^2
// Which pairs exist, their order and which products each one adds depend on the pattern alone: the SYMBOLIC phase runs once per pattern
// on the host (pmt_sparse_gram_count / _order / _runs below) and leaves a product list — per pair the (ta, tb) positions in nzval of its
// products, rows ascending.  Per re-evaluation the kernels stream that list (8 bytes per product), gather the two values from nzval (small
// and cache-resident next to the list), and add each pair's products in a FIXED order that is part of the ABI (include/parametron_hip.h):
// short segments left to right, segments of 64 products or more in the one-wave order of csc_values_wave_kernel (handoff.hip).  How the
// launch is cut into workgroup runs does not change a bit of the output.
#include <new>
#include <vector>

#include "common.h"

namespace pmt {

constexpr int SG_NT = 256;
constexpr int SG_CAP = 2048;       // products of one workgroup run held in LDS (16 KB: several workgroups per CU)
constexpr int SG_LONG = 64;        // segments of this many products or more: one wave each
constexpr int SG_CU = 32;          // the constant's chains: loads in flight per thread

__device__ __forceinline__ void sg_store_quad(QT *__restrict__ out, int64_t s, double acc, uint32_t j, uint32_t k,
                                              const int64_t *__restrict__ xvar, const int64_t *__restrict__ varmap, int moi) {
    QT o;                                                        // the whole 24-byte struct, every call
    o.coeff = (moi || j != k) ? 2.0 * acc : acc;                 // native form: the diagonal is not doubled (moi_interop.jl:58 does that)
    o.row = moi ? map_var(varmap, xvar[j]) : xvar[j];
    o.col = moi ? map_var(varmap, xvar[k]) : xvar[k];
    out[s] = o;
}

__device__ __forceinline__ void sg_store_lin(LT *__restrict__ out, int64_t l, double acc, uint32_t j, const int64_t *__restrict__ xvar,
                                             const int64_t *__restrict__ varmap, int moi) {
    LT o;
    o.coeff = 2.0 * acc;
    o.var = moi ? map_var(varmap, xvar[j]) : xvar[j];
    out[l] = o;
}

// The constant, one workgroup: 256 chains (chain t adds rows t, t + 256, .. in order), then the halving tree — the order of S_d in
// pmt_quad_gram_sum_f64 (gram_sum.hip).  A chain is serial, so its time is load latency: SG_CU loads per thread are in flight before their
// squares join the chain, and the workgroup is the FIRST of its launch, so that the chain runs beside the segment work, not behind it.
__device__ __forceinline__ void sg_constant(double *red, const double *__restrict__ d, int sign, int64_t rows, double *__restrict__ out_const) {
    const int tid = threadIdx.x;
    double part = 0.0;
    if (d && sign) {
        int64_t i = tid;
        for (; i + (SG_CU - 1) * SG_NT < rows; i += SG_CU * SG_NT) {
            double c[SG_CU];
#pragma unroll
            for (int u = 0; u < SG_CU; ++u) c[u] = signed_const(d[i + u * SG_NT], sign);
#pragma unroll
            for (int u = 0; u < SG_CU; ++u) part = part + c[u] * c[u];
        }
        for (; i < rows; i += SG_NT) {
            const double c = signed_const(d[i], sign);
            part = part + c * c;
        }
    }
    red[tid] = part;
    __syncthreads();
    for (int h = SG_NT / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] = red[tid] + red[tid + h];
        __syncthreads();
    }
    if (tid == 0) *out_const = red[0];
}

// Short segments, one launch.  Workgroup 0 writes the constant.  Workgroup 1 + r takes quadratic run r = the whole segments runs[2r] ..
// runs[2r+1]-1 (host table, pmt_sparse_gram_runs: every one short, at most SG_CAP products together): it reads their 8-byte (ta, tb) pairs
// coalesced, gathers the two values, parks the products in LDS, and one lane per segment adds its products from there left to right.
// Workgroup 1 + nruns + r does the same for linear run r: its segments are whole columns, consecutive in CSC storage, so nzval and the
// row indices are read coalesced (lin_seg[l] = the first entry of column lin_col[l]) and only c_i = 0.0 (+|-) d[row] is gathered.
__global__ __launch_bounds__(SG_NT) void sparse_gram_runs_kernel(const double *__restrict__ nzval, const uint2 *__restrict__ prod,
                                                                 const int64_t *__restrict__ seg_ptr, const uint32_t *__restrict__ pair_j,
                                                                 const uint32_t *__restrict__ pair_k, const int64_t *__restrict__ runs, int64_t nruns,
                                                                 const int64_t *__restrict__ lin_seg, const uint32_t *__restrict__ rowidx0,
                                                                 const uint32_t *__restrict__ lin_col, const int64_t *__restrict__ lin_runs,
                                                                 const int64_t *__restrict__ xvar, const int64_t *__restrict__ varmap, int moi,
                                                                 QT *__restrict__ out_quad, LT *__restrict__ out_lin, const double *__restrict__ d, int sign,
                                                                 int64_t rows, double *__restrict__ out_const) {
    __shared__ double s_p[SG_CAP];
    static_assert(SG_CAP >= SG_NT, "the constant's tree uses the product buffer");
    const int tid = threadIdx.x;
    if (blockIdx.x == 0) {
        sg_constant(s_p, d, sign, rows, out_const);
        return;
    }
    const int64_t b = (int64_t)blockIdx.x - 1;
    if (b < nruns) {
        const int64_t s0 = runs[2 * b], s1 = runs[2 * b + 1];
        const int64_t p0 = seg_ptr[s0];
        const int64_t np = seg_ptr[s1] - p0;
        if (np < 0 || np > SG_CAP) return;                       // not a run of pmt_sparse_gram_runs: nothing is written
        for (int q = tid; q < (int)np; q += SG_NT) {
            const uint2 pr = prod[p0 + q];
            s_p[q] = nzval[pr.x] * nzval[pr.y];
        }
        __syncthreads();
        for (int64_t s = s0 + tid; s < s1; s += SG_NT) {
            const int a = (int)(seg_ptr[s] - p0), e = (int)(seg_ptr[s + 1] - p0);
            double acc = s_p[a];
            for (int q = a + 1; q < e; ++q) acc = acc + s_p[q];
            sg_store_quad(out_quad, s, acc, pair_j[s], pair_k[s], xvar, varmap, moi);
        }
        return;
    }
    const int64_t r = b - nruns;
    const int64_t l0 = lin_runs[2 * r], l1 = lin_runs[2 * r + 1];
    const int64_t t0 = lin_seg[l0];
    const int64_t np = lin_seg[l1] - t0;
    if (np < 0 || np > SG_CAP) return;
    for (int q = tid; q < (int)np; q += SG_NT) s_p[q] = nzval[t0 + q] * signed_const(d ? d[rowidx0[t0 + q]] : 0.0, d ? sign : 0);
    __syncthreads();
    for (int64_t l = l0 + tid; l < l1; l += SG_NT) {
        const int a = (int)(lin_seg[l] - t0), e = (int)(lin_seg[l + 1] - t0);
        double acc = s_p[a];
        for (int q = a + 1; q < e; ++q) acc = acc + s_p[q];
        sg_store_lin(out_lin, l, acc, lin_col[l], xvar, varmap, moi);
    }
}

// Long segments (two columns sharing 64 rows or more), one wave each: every lane starts at 0.0, lane l adds products l, l + 64, .. in
// order, then the __shfl_down tree 32, 16, .., 1
__global__ __launch_bounds__(256) void sparse_gram_long_kernel(const double *__restrict__ nzval, const uint2 *__restrict__ prod,
                                                               const int64_t *__restrict__ seg_ptr, const uint32_t *__restrict__ pair_j,
                                                               const uint32_t *__restrict__ pair_k, const int64_t *__restrict__ long_seg, int64_t nlong,
                                                               const int64_t *__restrict__ xvar, const int64_t *__restrict__ varmap, int moi,
                                                               QT *__restrict__ out_quad) {
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nlong) return;
    const int lane = threadIdx.x & 63;
    const int64_t s = long_seg[w];
    const int64_t p0 = seg_ptr[s], p1 = seg_ptr[s + 1];
    double acc = 0.0;
    for (int64_t p = p0 + lane; p < p1; p += 64) {
        const uint2 pr = prod[p];
        acc = acc + nzval[pr.x] * nzval[pr.y];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc = acc + __shfl_down(acc, off, 64);
    if (lane == 0) sg_store_quad(out_quad, s, acc, pair_j[s], pair_k[s], xvar, varmap, moi);
}

// Linear terms of columns with 64 entries or more (lin_long: their positions in lin_col), one wave each, in the long segments' order
__global__ __launch_bounds__(256) void sparse_gram_lin_long_kernel(const double *__restrict__ nzval, const int64_t *__restrict__ lin_seg,
                                                                   const uint32_t *__restrict__ rowidx0, const uint32_t *__restrict__ lin_col,
                                                                   const int64_t *__restrict__ lin_long, int64_t nlin_long, const double *__restrict__ d,
                                                                   int sign, const int64_t *__restrict__ xvar, const int64_t *__restrict__ varmap,
                                                                   int moi, LT *__restrict__ out_lin) {
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nlin_long) return;
    const int lane = threadIdx.x & 63;
    const int64_t l = lin_long[w];
    const int64_t t0 = lin_seg[l], t1 = lin_seg[l + 1];
    double acc = 0.0;
    for (int64_t t = t0 + lane; t < t1; t += 64) acc = acc + nzval[t] * signed_const(d ? d[rowidx0[t]] : 0.0, d ? sign : 0);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc = acc + __shfl_down(acc, off, 64);
    if (lane == 0) sg_store_lin(out_lin, l, acc, lin_col[l], xvar, varmap, moi);
}

// ---- symbolic phase (host, once per pattern)
struct RowMajor {
    std::vector<int64_t> row_ptr;      // m + 1
    std::vector<uint32_t> col, pos;    // per entry in row-major order: its column and its position in nzval
};

// checks the pattern (canonical CSC: 1-based, rows strictly ascending within a column) and builds its row-major view by counting
static int sg_rowmajor(const char *who, int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval, RowMajor &R) {
    const std::string w(who);
    PMT_REQUIRE(m >= 0 && n >= 0, PMT_DIMENSION_MISMATCH, w + ": negative dimension");
    PMT_REQUIRE(colptr, PMT_INVALID_ARGUMENT, w + ": null pointer");
    PMT_REQUIRE(colptr[0] == 1, PMT_INVALID_ARGUMENT, w + ": colptr must be 1-based");
    for (int64_t c = 0; c < n; ++c) PMT_REQUIRE(colptr[c + 1] >= colptr[c], PMT_INVALID_ARGUMENT, w + ": colptr not monotone");
    const int64_t nnz = colptr[n] - 1;
    PMT_REQUIRE(nnz < ((int64_t)1 << 32) && n < ((int64_t)1 << 32), PMT_DIMENSION_MISMATCH, w + ": 2^32 or more non-zeros or columns");
    PMT_REQUIRE(nnz == 0 || rowval, PMT_INVALID_ARGUMENT, w + ": null pointer");
    R.row_ptr.assign((size_t)m + 1, 0);
    for (int64_t c = 0; c < n; ++c) {
        int64_t prev = 0;
        for (int64_t p = colptr[c] - 1; p < colptr[c + 1] - 1; ++p) {
            const int64_t r = rowval[p];
            PMT_REQUIRE(r >= 1 && r <= m, PMT_DIMENSION_MISMATCH, w + ": row index out of range");
            PMT_REQUIRE(r > prev, PMT_INVALID_ARGUMENT, w + ": rows must ascend strictly within a column");
            prev = r;
            R.row_ptr[(size_t)r]++;
        }
    }
    for (int64_t i = 0; i < m; ++i) R.row_ptr[(size_t)i + 1] += R.row_ptr[(size_t)i];
    R.col.resize((size_t)nnz);
    R.pos.resize((size_t)nnz);
    std::vector<int64_t> cursor(R.row_ptr.begin(), R.row_ptr.end() - 1);
    for (int64_t c = 0; c < n; ++c)                              // ascending column => ascending column within each row
        for (int64_t p = colptr[c] - 1; p < colptr[c + 1] - 1; ++p) {
            const int64_t u = cursor[(size_t)(rowval[p] - 1)]++;
            R.col[(size_t)u] = (uint32_t)c;
            R.pos[(size_t)u] = (uint32_t)p;
        }
    return PMT_OK;
}

}  // namespace pmt

using namespace pmt;

extern "C" int pmt_sparse_gram_count(int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval, int64_t *nq, int64_t *nprod) try {
    PMT_REQUIRE(nq && nprod, PMT_INVALID_ARGUMENT, "sparse_gram_count: null pointer");
    RowMajor R;
    if (int rc = sg_rowmajor("sparse_gram_count", m, n, colptr, rowval, R)) return rc;
    int64_t np = 0;
    for (int64_t i = 0; i < m; ++i) {
        const int64_t L = R.row_ptr[(size_t)i + 1] - R.row_ptr[(size_t)i];
        np += L * (L + 1) / 2;
    }
    *nprod = np;
    *nq = -1;
    if (np >= ((int64_t)1 << 31)) return PMT_OK;                 // too many products for this node (the caller refuses): the pairs are not counted
    // pairs (j, k), j <= k: per column j the distinct columns k >= j of the rows it touches (a mark per column; the row's entry of column
    // j is where the row's cursor stands, since the columns are walked in ascending order)
    std::vector<int64_t> mark((size_t)n, -1), cursor(R.row_ptr.begin(), R.row_ptr.end() - 1);
    int64_t pairs = 0;
    for (int64_t j = 0; j < n; ++j)
        for (int64_t p = colptr[j] - 1; p < colptr[j + 1] - 1; ++p) {
            const int64_t i = rowval[p] - 1;
            for (int64_t u = cursor[(size_t)i]++; u < R.row_ptr[(size_t)i + 1]; ++u) {
                const uint32_t k = R.col[(size_t)u];
                if (mark[k] != j) { mark[k] = j; ++pairs; }
            }
        }
    *nq = pairs;
    *nprod = np;
    return PMT_OK;
} catch (const std::bad_alloc &) {
    return pmt::fail(PMT_OUT_OF_MEMORY, "sparse_gram_count: out of host memory");
}

extern "C" int pmt_sparse_gram_order(int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval, int64_t nq, int64_t nprod,
                                     uint32_t *pair_j, uint32_t *pair_k, int64_t *seg_ptr, void *prod_out, uint32_t *lin_col, int64_t *nlin) try {
    PMT_REQUIRE(nq >= 0 && nprod >= 0, PMT_INVALID_ARGUMENT, "sparse_gram_order: negative count");
    PMT_REQUIRE(nprod < ((int64_t)1 << 31), PMT_INVALID_ARGUMENT,
                "sparse_gram_order: nprod = " + std::to_string(nprod) + " products, 2^31 or more: at that fill-in hold the matrix in a dense Parameter");
    PMT_REQUIRE(seg_ptr && nlin && (nq == 0 || (pair_j && pair_k)) && (nprod == 0 || prod_out) && (n == 0 || lin_col), PMT_INVALID_ARGUMENT,
                "sparse_gram_order: null pointer");
    RowMajor R;
    if (int rc = sg_rowmajor("sparse_gram_order", m, n, colptr, rowval, R)) return rc;
    uint2 *prod = reinterpret_cast<uint2 *>(prod_out);
    // The products in (k, row, j) order — column k, its entries by ascending row, the row's entries up to column k — dealt into one bucket
    // per j (counting pass, then placement): every bucket then holds its products by (k, row), i.e. the segments of j in order of k with
    // ascending rows inside.  Linear in nprod + n, no comparison sort.
    std::vector<int64_t> start((size_t)n + 1, 0);
    {
        std::vector<int64_t> upto(R.row_ptr.begin(), R.row_ptr.end() - 1);       // per row: one past its entry of the current column k
        int64_t total = 0;
        for (int64_t k = 0; k < n; ++k)
            for (int64_t p = colptr[k] - 1; p < colptr[k + 1] - 1; ++p) {
                const int64_t i = rowval[p] - 1;
                const int64_t end = ++upto[(size_t)i];
                for (int64_t u = R.row_ptr[(size_t)i]; u < end; ++u) ++start[(size_t)R.col[(size_t)u] + 1];
                total += end - R.row_ptr[(size_t)i];
            }
        PMT_REQUIRE(total == nprod, PMT_INVALID_ARGUMENT, "sparse_gram_order: nprod is not this pattern's (pmt_sparse_gram_count)");
    }
    for (int64_t j = 0; j < n; ++j) start[(size_t)j + 1] += start[(size_t)j];
    std::vector<uint32_t> kk((size_t)nprod);
    {
        std::vector<int64_t> fill(start.begin(), start.end() - 1), upto(R.row_ptr.begin(), R.row_ptr.end() - 1);
        for (int64_t k = 0; k < n; ++k)
            for (int64_t p = colptr[k] - 1; p < colptr[k + 1] - 1; ++p) {
                const int64_t i = rowval[p] - 1;
                const int64_t end = ++upto[(size_t)i];
                for (int64_t u = R.row_ptr[(size_t)i]; u < end; ++u) {
                    const int64_t at = fill[(size_t)R.col[(size_t)u]]++;
                    prod[at] = make_uint2(R.pos[(size_t)u], (uint32_t)p);
                    kk[(size_t)at] = (uint32_t)k;
                }
            }
    }
    int64_t nseg = 0;
    for (int64_t j = 0; j < n; ++j)
        for (int64_t at = start[(size_t)j]; at < start[(size_t)j + 1]; ++at)
            if (at == start[(size_t)j] || kk[(size_t)at] != kk[(size_t)at - 1]) {
                PMT_REQUIRE(nseg < nq, PMT_INVALID_ARGUMENT, "sparse_gram_order: nq is not this pattern's (pmt_sparse_gram_count)");
                pair_j[nseg] = (uint32_t)j;
                pair_k[nseg] = kk[(size_t)at];
                seg_ptr[nseg++] = at;
            }
    PMT_REQUIRE(nseg == nq, PMT_INVALID_ARGUMENT, "sparse_gram_order: nq is not this pattern's (pmt_sparse_gram_count)");
    seg_ptr[nq] = nprod;
    int64_t nl = 0;
    for (int64_t j = 0; j < n; ++j)
        if (colptr[j + 1] > colptr[j]) lin_col[nl++] = (uint32_t)j;
    *nlin = nl;
    return PMT_OK;
} catch (const std::bad_alloc &) {
    return pmt::fail(PMT_OUT_OF_MEMORY, "sparse_gram_order: out of host memory");
}

extern "C" int pmt_sparse_gram_runs(const int64_t *seg_ptr, int64_t nq, int64_t cap, int64_t *runs, int64_t *nruns, int64_t *long_seg,
                                    int64_t *nlong) {
    PMT_REQUIRE(nq >= 0 && cap >= SG_LONG && cap <= SG_CAP, PMT_INVALID_ARGUMENT, "sparse_gram_runs: need nq >= 0 and 64 <= cap <= 2048");
    PMT_REQUIRE(seg_ptr && nruns && nlong, PMT_INVALID_ARGUMENT, "sparse_gram_runs: null pointer");
    int64_t nr = 0, nl = 0, s = 0;
    while (s < nq) {
        const int64_t len = seg_ptr[s + 1] - seg_ptr[s];
        PMT_REQUIRE(len >= 1, PMT_INVALID_ARGUMENT, "sparse_gram_runs: empty segment");
        if (len >= SG_LONG) {
            if (long_seg) long_seg[nl] = s;
            ++nl; ++s;
            continue;
        }
        int64_t e = s, total = 0;
        while (e < nq && seg_ptr[e + 1] - seg_ptr[e] < SG_LONG && total + (seg_ptr[e + 1] - seg_ptr[e]) <= cap) {
            PMT_REQUIRE(seg_ptr[e + 1] > seg_ptr[e], PMT_INVALID_ARGUMENT, "sparse_gram_runs: empty segment");
            total += seg_ptr[e + 1] - seg_ptr[e];
            ++e;
        }
        if (runs) { runs[2 * nr] = s; runs[2 * nr + 1] = e; }
        ++nr;
        s = e;
    }
    *nruns = nr;
    *nlong = nl;
    return PMT_OK;
}

extern "C" int pmt_sparse_gram_f64(const double *nzval, const void *prod, const int64_t *seg_ptr, const uint32_t *pair_j, const uint32_t *pair_k,
                                   int64_t nq, const int64_t *runs, int64_t nruns, const int64_t *long_seg, int64_t nlong,
                                   const int64_t *lin_seg, const uint32_t *rowidx0, const uint32_t *lin_col, int64_t nlin, const int64_t *lin_runs,
                                   int64_t nlin_runs, const int64_t *lin_long, int64_t nlin_long, int64_t rows, const int64_t *xvar, const double *d,
                                   int sign, int moi, const int64_t *varmap, pmt_quadratic_term *out_quad, pmt_linear_term *out_lin,
                                   double *out_const, void *stream) {
    PMT_REQUIRE(nq >= 0 && nruns >= 0 && nlong >= 0 && nlin >= 0 && nlin_runs >= 0 && nlin_long >= 0 && rows >= 0, PMT_INVALID_ARGUMENT,
                "sparse_gram: negative count");
    PMT_REQUIRE(nruns + nlong <= nq && nlin_runs + nlin_long <= nlin && nruns + nlin_runs < ((int64_t)1 << 31) - 1 && nlin < ((int64_t)1 << 32),
                PMT_INVALID_ARGUMENT, "sparse_gram: more runs than segments");
    PMT_REQUIRE(sign >= -1 && sign <= 1 && (sign == 0 || d), PMT_INVALID_ARGUMENT, "sparse_gram: sign must be -1, 0 or +1 and needs d");
    PMT_REQUIRE(!moi || varmap, PMT_INVALID_ARGUMENT, "sparse_gram: the MOI form needs varmap");
    PMT_REQUIRE(out_const, PMT_INVALID_ARGUMENT, "sparse_gram: null pointer");
    PMT_REQUIRE(nq == 0 || (nzval && prod && seg_ptr && pair_j && pair_k && xvar && out_quad && (nruns == 0 || runs) && (nlong == 0 || long_seg)),
                PMT_INVALID_ARGUMENT, "sparse_gram: null pointer");
    PMT_REQUIRE(nq == 0 || nruns + nlong > 0, PMT_INVALID_ARGUMENT, "sparse_gram: segments without runs");
    PMT_REQUIRE(nlin == 0 || (nzval && lin_seg && rowidx0 && lin_col && xvar && out_lin && (nlin_runs == 0 || lin_runs) && (nlin_long == 0 || lin_long)),
                PMT_INVALID_ARGUMENT, "sparse_gram: null pointer");
    PMT_REQUIRE(nlin == 0 || nlin_runs + nlin_long > 0, PMT_INVALID_ARGUMENT, "sparse_gram: columns without runs");
    if (!d) sign = 0;
    return dispatch(stream, [=](hipStream_t s) {
        const uint2 *pp = reinterpret_cast<const uint2 *>(prod);
        PMT_LAUNCH(sparse_gram_runs_kernel, dim3((unsigned)(1 + nruns + nlin_runs)), dim3(SG_NT), 0, s, nzval, pp, seg_ptr, pair_j, pair_k, runs, nruns,
                   lin_seg, rowidx0, lin_col, lin_runs, xvar, varmap, moi, out_quad, out_lin, d, sign, rows, out_const);
        if (nlong > 0)
            PMT_LAUNCH(sparse_gram_long_kernel, dim3((unsigned)cdiv(nlong, 4)), dim3(256), 0, s, nzval, pp, seg_ptr, pair_j, pair_k, long_seg, nlong, xvar,
                       varmap, moi, out_quad);
        if (nlin_long > 0)
            PMT_LAUNCH(sparse_gram_lin_long_kernel, dim3((unsigned)cdiv(nlin_long, 4)), dim3(256), 0, s, nzval, lin_seg, rowidx0, lin_col, lin_long,
                       nlin_long, d, sign, xvar, varmap, moi, out_lin);
        return check_launch("sparse_gram_kernel");
    });
}
