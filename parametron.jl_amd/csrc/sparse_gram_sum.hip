// Weighted sums over sparse least-squares blocks as one canonical objective: dot(r, r) + lam*dot(x, x), w1*dot(r1, r1) + w2*dot(r2, r2), ..
// with r_b = C_b*x (+|-) d_b and every C_b a fixed-pattern CSC matrix (sparse_gram.hip).
//
// The reference builds such an objective with add! / mul! of quadratic functions (src/functions.jl:452-461 append the term lists, :578
// scales them) and canonicalize! (:381-386) merges the duplicates before the MOI copy (src/moi_interop.jl:45-62).  Here every block is
// first written by the unchanged pmt_sparse_gram_f64 (moi = 1) as its own canonical term lists; which output term takes which block term
// depends on the patterns alone, so the SYMBOLIC phase (pmt_sparse_gram_sum_merge, host, once per record) merges the blocks' sorted pair
// and column lists with the positions of the diagonal / linear terms and leaves one gather table per block.  Per re-evaluation ONE launch
// weights and adds the blocks' coefficients through those tables, in the order the header fixes, and writes every output term once.
#include <new>
#include <vector>

#include "common.h"

namespace pmt {

constexpr int SS_NT = 256;
static_assert(PMT_SPARSE_SUM_WG_TERMS == SS_NT, "one output term per thread");
constexpr uint32_t SS_NONE = 0xFFFFFFFFu;

struct SparseSumArgs {
    int nterms;
    pmt_sparse_lsq_term t[PMT_LSQ_MAX_TERMS];
};

// W_t = scale_t * (*weight_t), or scale_t
__device__ __forceinline__ double ss_weight(const pmt_sparse_lsq_term &t) { return t.weight ? t.scale * *t.weight : t.scale; }

// the term's vector index of position j, or -1 when the term does not list j (no table: the term lies over all of x)
__device__ __forceinline__ int64_t ss_find(const pmt_sparse_lsq_term &t, int64_t j) { return t.pos ? (int64_t)t.pos[j] : j; }

// The constant, one workgroup: sum_b W_b*cc_b, then W_d * (sum v^2) per diagonal term with v, then the scalar constants — each in
// expression order, the order of gram_sum_const (gram_sum.hip): 256 chains over the term's own vector, then the halving tree.
__device__ __forceinline__ void ss_constant(const SparseSumArgs &g, double *red, double *__restrict__ out_const) {
    const int tid = threadIdx.x;
    double s = 0.0;
    bool any = false;
    for (int i = 0; i < g.nterms; ++i) {
        if (g.t[i].kind != PMT_LSQ_BLOCK) continue;
        const double v = ss_weight(g.t[i]) * *g.t[i].constant;
        s = any ? s + v : v;
        any = true;
    }
    for (int i = 0; i < g.nterms; ++i) {
        if (g.t[i].kind != PMT_LSQ_DIAG || !g.t[i].vec) continue;
        const double *__restrict__ v = g.t[i].vec;
        const int64_t nv = g.t[i].nvec;
        double part = 0.0;
        for (int64_t jj = tid; jj < nv; jj += SS_NT) part = part + v[jj] * v[jj];
        __syncthreads();
        red[tid] = part;
        __syncthreads();
        for (int h = SS_NT / 2; h > 0; h >>= 1) {
            if (tid < h) red[tid] = red[tid] + red[tid + h];
            __syncthreads();
        }
        s = s + ss_weight(g.t[i]) * red[0];
    }
    for (int i = 0; i < g.nterms; ++i)
        if (g.t[i].kind == PMT_LSQ_CONSTANT) s = s + ss_weight(g.t[i]) * (g.t[i].vec ? *g.t[i].vec : 1.0);
    if (tid == 0) *out_const = s;
}

// One launch.  Workgroup 0 writes the constant (its serial chains run beside the rest).  Workgroup 1 + w takes the output quadratic terms
// 256 w .. 256 w + 255, one per thread: the blocks' coefficients through their gather tables (monotone: neighbouring threads read
// neighbouring block terms), the whole 24-byte structs parked in LDS and written by each wave as 16-byte stores.  The workgroups behind
// them take 256 output linear terms each.
__global__ __launch_bounds__(SS_NT) void sparse_gram_sum_kernel(SparseSumArgs g, const uint32_t *__restrict__ pair_j, const uint32_t *__restrict__ pair_k,
                                                                int64_t nq, const uint32_t *__restrict__ lin_col, int64_t nlin,
                                                                const int64_t *__restrict__ xvar, const int64_t *__restrict__ varmap,
                                                                QT *__restrict__ out_quad, LT *__restrict__ out_lin, double *__restrict__ out_const) {
    typedef unsigned long long u64w;
    __shared__ u64w s_w[3 * SS_NT];
    const int tid = threadIdx.x;
    if (blockIdx.x == 0) {
        ss_constant(g, reinterpret_cast<double *>(s_w), out_const);
        return;
    }
    const int64_t nqwg = (nq + SS_NT - 1) / SS_NT;
    const int64_t b = (int64_t)blockIdx.x - 1;
    if (b < nqwg) {
        const int64_t s0 = b * SS_NT, s = s0 + tid;
        if (s < nq) {
            const uint32_t j = pair_j[s], k = pair_k[s];
            double c = 0.0;
            bool any = false;
            for (int i = 0; i < g.nterms; ++i) {
                if (g.t[i].kind != PMT_LSQ_BLOCK) continue;
                const uint32_t u = g.t[i].quad_at[s];
                if (u == SS_NONE) continue;
                const double v = ss_weight(g.t[i]) * g.t[i].quad[u].coeff;
                c = any ? c + v : v;
                any = true;
            }
            if (j == k) {
                // D_j = ((2*W_d1) + (2*W_d2)) + ..  over the diagonal terms that list position j, in order
                double d = 0.0;
                bool anyd = false;
                for (int i = 0; i < g.nterms; ++i) {
                    if (g.t[i].kind != PMT_LSQ_DIAG || ss_find(g.t[i], j) < 0) continue;
                    const double w2 = 2 * ss_weight(g.t[i]);
                    d = anyd ? d + w2 : w2;
                    anyd = true;
                }
                if (anyd) c = any ? c + d : d;
            }
            s_w[3 * tid] = (u64w)__double_as_longlong(c);
            s_w[3 * tid + 1] = (u64w)map_var(varmap, xvar[j]);
            s_w[3 * tid + 2] = (u64w)map_var(varmap, xvar[k]);
        }
        __syncthreads();
        const int wave = tid >> 6, lane = tid & 63;
        const int64_t w0 = s0 + 64 * wave;
        const int cnt = (int)(nq - w0 < 64 ? nq - w0 : 64);
        if (cnt > 0) {                                           // (an empty segment must not reach the leading-word store)
            const u64w *src = s_w + 3 * 64 * wave;
            wave_write_words<3>(reinterpret_cast<u64w *>(out_quad + w0), cnt, lane, [&](int q) -> u64w { return src[q]; });
        }
        return;
    }
    const int64_t l = (b - nqwg) * SS_NT + tid;
    if (l >= nlin) return;
    const uint32_t j = lin_col[l];
    double c = 0.0;
    bool any = false;
    for (int i = 0; i < g.nterms; ++i) {
        if (g.t[i].kind != PMT_LSQ_BLOCK) continue;
        const uint32_t u = g.t[i].lin_at[l];
        if (u == SS_NONE) continue;
        const double v = ss_weight(g.t[i]) * g.t[i].lin[u].coeff;
        c = any ? c + v : v;
        any = true;
    }
    for (int i = 0; i < g.nterms; ++i) {
        if (g.t[i].kind != PMT_LSQ_DIAG || !g.t[i].vec) continue;
        const int64_t p = ss_find(g.t[i], j);
        if (p < 0) continue;
        const double v = ss_weight(g.t[i]) * (2 * signed_const(g.t[i].vec[p], g.t[i].sign));
        c = any ? c + v : v;
        any = true;
    }
    for (int i = 0; i < g.nterms; ++i) {
        if (g.t[i].kind != PMT_LSQ_LINEAR) continue;
        const int64_t p = ss_find(g.t[i], j);
        if (p < 0) continue;
        const double v = ss_weight(g.t[i]) * g.t[i].vec[p];
        c = any ? c + v : v;
        any = true;
    }
    LT o;                                                        // the whole 16-byte struct, every call
    o.coeff = c;
    o.var = map_var(varmap, xvar[j]);
    out_lin[l] = o;
}

}  // namespace pmt

using namespace pmt;

// ---- symbolic phase (host, once per record)
extern "C" int pmt_sparse_gram_sum_merge(int64_t n, int nblocks, const uint32_t *const *pair_j, const uint32_t *const *pair_k, const int64_t *nq,
                                         const uint32_t *const *lin_col, const int64_t *nlin, int nterms, const int32_t *term_kind,
                                         const int32_t *term_has_vec, const int64_t *const *term_cols, const int64_t *term_ncols,
                                         int64_t *out_nq, int64_t *out_nlin, uint32_t *out_pair_j, uint32_t *out_pair_k, uint32_t *out_lin_col,
                                         uint32_t *const *quad_at, uint32_t *const *lin_at, int32_t *const *term_pos) try {
    const std::string w("sparse_gram_sum_merge");
    PMT_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), PMT_DIMENSION_MISMATCH, w + ": need 0 <= n < 2^31 columns");
    PMT_REQUIRE(nblocks >= 1 && nblocks <= PMT_LSQ_MAX_BLOCKS, PMT_INVALID_ARGUMENT, w + ": 1 .. 8 least-squares blocks");
    PMT_REQUIRE(nterms >= 1 && nterms <= PMT_LSQ_MAX_TERMS, PMT_INVALID_ARGUMENT, w + ": 1 .. 32 terms");
    PMT_REQUIRE(pair_j && pair_k && nq && lin_col && nlin && term_kind && term_has_vec && out_nq && out_nlin, PMT_INVALID_ARGUMENT,
                w + ": null pointer");
    const bool fill = out_pair_j || out_pair_k || out_lin_col || quad_at || lin_at || term_pos;
    PMT_REQUIRE(!fill || (out_pair_j && out_pair_k && out_lin_col && quad_at && lin_at), PMT_INVALID_ARGUMENT,
                w + ": null pointer (the outputs come together)");
    int kb = 0;
    for (int t = 0; t < nterms; ++t) {
        const int kind = term_kind[t];
        PMT_REQUIRE(kind == PMT_LSQ_BLOCK || kind == PMT_LSQ_DIAG || kind == PMT_LSQ_LINEAR || kind == PMT_LSQ_CONSTANT, PMT_INVALID_ARGUMENT,
                    w + ": unknown term kind");
        if (kind == PMT_LSQ_BLOCK) ++kb;
        const int64_t *list = term_cols ? term_cols[t] : nullptr;
        if (!list) continue;
        PMT_REQUIRE(kind == PMT_LSQ_DIAG || kind == PMT_LSQ_LINEAR, PMT_INVALID_ARGUMENT, w + ": only diagonal and linear terms take a column list");
        PMT_REQUIRE(term_ncols, PMT_INVALID_ARGUMENT, w + ": null column counts");
        const int64_t m = term_ncols[t];
        PMT_REQUIRE(m >= 0 && m <= n, PMT_DIMENSION_MISMATCH, w + ": column count outside 0 .. n");
        for (int64_t k = 0; k < m; ++k) {
            PMT_REQUIRE(list[k] >= 0 && list[k] < n, PMT_DIMENSION_MISMATCH, w + ": column position outside 0 .. n-1");
            PMT_REQUIRE(k == 0 || list[k] > list[k - 1], PMT_INVALID_ARGUMENT, w + ": column positions not strictly increasing");
        }
        PMT_REQUIRE(!fill || (term_pos && term_pos[t]), PMT_INVALID_ARGUMENT, w + ": null position table of a term with a column list");
    }
    PMT_REQUIRE(kb == nblocks, PMT_INVALID_ARGUMENT, w + ": the term list does not hold nblocks blocks");
    for (int b = 0; b < nblocks; ++b) {
        PMT_REQUIRE(nq[b] >= 0 && nlin[b] >= 0, PMT_INVALID_ARGUMENT, w + ": negative count");
        PMT_REQUIRE(nq[b] < (int64_t)SS_NONE && nlin[b] <= n, PMT_DIMENSION_MISMATCH, w + ": a block with 2^32 - 1 or more pairs, or more columns than n");
        PMT_REQUIRE((nq[b] == 0 || (pair_j[b] && pair_k[b])) && (nlin[b] == 0 || lin_col[b]), PMT_INVALID_ARGUMENT, w + ": null pointer");
        PMT_REQUIRE(!fill || (quad_at[b] && lin_at[b]), PMT_INVALID_ARGUMENT, w + ": null gather table");
        for (int64_t s = 0; s < nq[b]; ++s) {
            const uint32_t j = pair_j[b][s], k = pair_k[b][s];
            PMT_REQUIRE(j <= k && (int64_t)k < n, PMT_DIMENSION_MISMATCH, w + ": pair outside j <= k < n");
            PMT_REQUIRE(s == 0 || pair_j[b][s - 1] < j || (pair_j[b][s - 1] == j && pair_k[b][s - 1] < k), PMT_INVALID_ARGUMENT,
                        w + ": pairs not sorted by (j, k)");
        }
        for (int64_t l = 0; l < nlin[b]; ++l) {
            PMT_REQUIRE((int64_t)lin_col[b][l] < n, PMT_DIMENSION_MISMATCH, w + ": column position outside 0 .. n-1");
            PMT_REQUIRE(l == 0 || lin_col[b][l] > lin_col[b][l - 1], PMT_INVALID_ARGUMENT, w + ": columns not strictly increasing");
        }
    }
    // positions a diagonal term lists (their (j, j) pairs), and the columns with a linear contribution
    std::vector<uint8_t> diag((size_t)n, 0), col((size_t)n, 0);
    for (int t = 0; t < nterms; ++t) {
        const int kind = term_kind[t];
        if (kind != PMT_LSQ_DIAG && kind != PMT_LSQ_LINEAR) continue;
        const int64_t *list = term_cols ? term_cols[t] : nullptr;
        const int64_t m = list ? term_ncols[t] : n;
        const bool lin = kind == PMT_LSQ_LINEAR || term_has_vec[t];
        for (int64_t k = 0; k < m; ++k) {
            const int64_t j = list ? list[k] : k;
            if (kind == PMT_LSQ_DIAG) diag[(size_t)j] = 1;
            if (lin) col[(size_t)j] = 1;
        }
        if (fill && list) {
            int32_t *pos = term_pos[t];
            for (int64_t j = 0; j < n; ++j) pos[j] = -1;
            for (int64_t k = 0; k < m; ++k) pos[list[k]] = (int32_t)k;
        }
    }
    // the quadratic pairs: the blocks' sorted lists and the diagonal positions merged by (j, k) — each step looks at the K + 1 heads
    // (K <= 8: linear in the input), no comparison sort
    int64_t head[PMT_LSQ_MAX_BLOCKS] = {0};
    int64_t dj = 0, total = 0;
    const uint64_t END = ~(uint64_t)0;
    for (;;) {
        while (dj < n && !diag[(size_t)dj]) ++dj;
        uint64_t best = dj < n ? ((uint64_t)dj << 32 | (uint64_t)dj) : END;
        for (int b = 0; b < nblocks; ++b)
            if (head[b] < nq[b]) {
                const uint64_t key = (uint64_t)pair_j[b][head[b]] << 32 | pair_k[b][head[b]];
                if (key < best) best = key;
            }
        if (best == END) break;
        if (fill) {
            out_pair_j[total] = (uint32_t)(best >> 32);
            out_pair_k[total] = (uint32_t)(best & 0xFFFFFFFFu);
        }
        for (int b = 0; b < nblocks; ++b) {
            const bool has = head[b] < nq[b] && ((uint64_t)pair_j[b][head[b]] << 32 | pair_k[b][head[b]]) == best;
            if (fill) quad_at[b][total] = has ? (uint32_t)head[b] : SS_NONE;
            if (has) ++head[b];
        }
        if (dj < n && ((uint64_t)dj << 32 | (uint64_t)dj) == best) ++dj;
        ++total;
    }
    *out_nq = total;
    // the linear columns: one sweep over the positions
    for (int b = 0; b < nblocks; ++b) {
        head[b] = 0;
        for (int64_t l = 0; l < nlin[b]; ++l) col[lin_col[b][l]] = 1;
    }
    int64_t nl = 0;
    for (int64_t j = 0; j < n; ++j) {
        if (!col[(size_t)j]) continue;
        if (fill) out_lin_col[nl] = (uint32_t)j;
        for (int b = 0; b < nblocks; ++b) {
            const bool has = head[b] < nlin[b] && (int64_t)lin_col[b][head[b]] == j;
            if (fill) lin_at[b][nl] = has ? (uint32_t)head[b] : SS_NONE;
            if (has) ++head[b];
        }
        ++nl;
    }
    *out_nlin = nl;
    return PMT_OK;
} catch (const std::bad_alloc &) {
    return pmt::fail(PMT_OUT_OF_MEMORY, "sparse_gram_sum_merge: out of host memory");
}

extern "C" int pmt_sparse_gram_sum_f64(int64_t n, const pmt_sparse_lsq_term *terms, int nterms, const uint32_t *pair_j, const uint32_t *pair_k,
                                       int64_t nq, const uint32_t *lin_col, int64_t nlin, const int64_t *xvar, const int64_t *varmap,
                                       pmt_quadratic_term *out_quad, pmt_linear_term *out_lin, double *out_const, void *stream) {
    const std::string w("sparse_gram_sum");
    PMT_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), PMT_DIMENSION_MISMATCH, w + ": need 0 <= n < 2^31 columns");
    PMT_REQUIRE(nq >= 0 && nlin >= 0, PMT_INVALID_ARGUMENT, w + ": negative count");
    PMT_REQUIRE(nlin <= n, PMT_DIMENSION_MISMATCH, w + ": more linear terms than columns");
    PMT_REQUIRE(terms, PMT_INVALID_ARGUMENT, w + ": null term list");
    PMT_REQUIRE(nterms >= 1 && nterms <= PMT_LSQ_MAX_TERMS, PMT_INVALID_ARGUMENT, w + ": 1 .. 32 terms");
    PMT_REQUIRE(varmap, PMT_INVALID_ARGUMENT, w + ": the MOI form needs varmap");
    PMT_REQUIRE(out_const, PMT_INVALID_ARGUMENT, w + ": null pointer");
    PMT_REQUIRE(nq == 0 || (pair_j && pair_k && xvar && out_quad), PMT_INVALID_ARGUMENT, w + ": null pointer");
    PMT_REQUIRE(nlin == 0 || (lin_col && xvar && out_lin), PMT_INVALID_ARGUMENT, w + ": null pointer");
    PMT_REQUIRE(cdiv(nq, SS_NT) + cdiv(nlin, SS_NT) < ((int64_t)1 << 31) - 1, PMT_DIMENSION_MISMATCH, w + ": too many terms for one launch");
    SparseSumArgs g;
    g.nterms = nterms;
    int nblocks = 0;
    for (int i = 0; i < nterms; ++i) {
        const pmt_sparse_lsq_term &t = terms[i];
        switch (t.kind) {
        case PMT_LSQ_BLOCK:
            ++nblocks;
            PMT_REQUIRE(t.constant && (nq == 0 || (t.quad && t.quad_at)) && (nlin == 0 || (t.lin && t.lin_at)), PMT_INVALID_ARGUMENT,
                        w + ": null term list or gather table of a block");
            break;
        case PMT_LSQ_DIAG:
            PMT_REQUIRE(t.vec ? (t.sign == 1 || t.sign == -1) : t.sign == 0, PMT_INVALID_ARGUMENT,
                        w + ": diagonal term sign must be +1 or -1 with a vector, 0 without");
            PMT_REQUIRE(t.nvec >= 0 && t.nvec <= n && (t.pos || t.nvec == n), PMT_DIMENSION_MISMATCH,
                        w + ": vector length of a diagonal term outside 0 .. n, or not n without a position table");
            break;
        case PMT_LSQ_LINEAR:
            PMT_REQUIRE(t.vec, PMT_INVALID_ARGUMENT, w + ": null coefficient vector of a linear term");
            PMT_REQUIRE(t.nvec >= 0 && t.nvec <= n && (t.pos || t.nvec == n), PMT_DIMENSION_MISMATCH,
                        w + ": vector length of a linear term outside 0 .. n, or not n without a position table");
            break;
        case PMT_LSQ_CONSTANT:
            break;
        default:
            return fail(PMT_INVALID_ARGUMENT, w + ": unknown term kind");
        }
        g.t[i] = t;
    }
    for (int i = nterms; i < PMT_LSQ_MAX_TERMS; ++i) g.t[i] = pmt_sparse_lsq_term{};
    PMT_REQUIRE(nblocks >= 1 && nblocks <= PMT_LSQ_MAX_BLOCKS, PMT_INVALID_ARGUMENT, w + ": 1 .. 8 least-squares blocks");
    return dispatch(stream, [=](hipStream_t s) {
        PMT_LAUNCH(sparse_gram_sum_kernel, dim3((unsigned)(1 + cdiv(nq, SS_NT) + cdiv(nlin, SS_NT))), dim3(SS_NT), 0, s, g, pair_j, pair_k, nq, lin_col,
                   nlin, xvar, varmap, out_quad, out_lin, out_const);
        return check_launch("sparse_gram_sum_kernel");
    });
}
