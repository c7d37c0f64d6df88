// Weighted sums of least-squares terms as one canonical objective: the combine behind pmt_quad_gram_sum_f64.
//
// The reference builds such an objective with add! / mul! of quadratic functions (src/functions.jl:452-461 append the term lists, :578
// scales them) and canonicalize! (:381-386) merges the duplicates before the MOI copy (src/moi_interop.jl:45-62).  Here block 1 of the sum
// is already the canonical MOI function (pmt_quad_gram_f64, moi = 1); blocks 2..K are the CSC values of pmt_quad_gram_csc_f64 (the same
// coefficients bit for bit).  These kernels weight and add them in place, in the order the header fixes.
#include "streams.h"

namespace pmt {

constexpr int SUM_TILE = 64;

struct SumArgs {
    int64_t n;
    int nterms;
    int first;          // index of block 1 in t[]
    int has_d;          // at least one diagonal term
    pmt_lsq_term t[PMT_LSQ_MAX_TERMS];
};

// Which columns a term covers (pmt_quad_gram_sum_f64: all of them; pmt_quad_gram_sum_sub_f64: runs of positions).  find(t, j): the
// term's vector index of position j, or -1 when the term does not list j; len(t): the length of its vector.
struct AllCols {
    __device__ __forceinline__ int64_t find(int, int64_t j) const { return j; }
    __device__ __forceinline__ int64_t len(int, int64_t n) const { return n; }
};

struct SubCols {
    int32_t first[PMT_LSQ_MAX_TERMS];   // the term's first run
    int32_t count[PMT_LSQ_MAX_TERMS];   // its number of runs, -1: every column
    int32_t nvec[PMT_LSQ_MAX_TERMS];    // its vector length
    int32_t start[PMT_LSQ_MAX_RUNS];    // run r: positions start .. start + run_len - 1, vector indices base ..
    int32_t run_len[PMT_LSQ_MAX_RUNS];
    int32_t base[PMT_LSQ_MAX_RUNS];
    __device__ __forceinline__ int64_t find(int t, int64_t j) const {
        if (count[t] < 0) return j;
        for (int r = first[t]; r < first[t] + count[t]; ++r)
            if (j >= start[r] && j < (int64_t)start[r] + run_len[r]) return base[r] + (j - start[r]);
        return -1;
    }
    __device__ __forceinline__ int64_t len(int t, int64_t n) const { return count[t] < 0 ? n : nvec[t]; }
};

// W_t = scale_t * (*weight_t), or scale_t
__device__ __forceinline__ double sum_weight(const pmt_lsq_term &t) { return t.weight ? t.scale * *t.weight : t.scale; }

// D_j = ((2*W_d1) + (2*W_d2)) + ..  over the diagonal terms that list position j, in order; `any`: whether one does
template <class Cols>
__device__ __forceinline__ double sum_diag_shift_at(const SumArgs &g, const Cols &cs, int64_t j, bool &any) {
    double d = 0.0;
    any = false;
    for (int i = 0; i < g.nterms; ++i) {
        if (g.t[i].kind != PMT_LSQ_DIAG || cs.find(i, j) < 0) continue;
        const double w2 = 2 * sum_weight(g.t[i]);
        d = any ? d + w2 : w2;
        any = true;
    }
    return d;
}

// One 64 x 64 tile of the upper triangle per workgroup (row-major order of the tile pairs).  Block 1's coefficients are read from the
// term array (row-major), the CSC columns of blocks 2..K coalesced (a tile column is 64 consecutive doubles) and transposed through LDS;
// the combined coefficients go back through LDS so that each wave rewrites whole row segments of 24-byte terms with 16-byte stores.
template <class Cols>
__device__ __forceinline__ void gram_sum_tile(const SumArgs &g, const Cols &cs, QT *__restrict__ quad) {
    __shared__ double tile[SUM_TILE][SUM_TILE + 1];
    const int64_t n = g.n;
    const int64_t nt = (n + SUM_TILE - 1) / SUM_TILE;
    int64_t p = blockIdx.x, bj = 0;
    while (p >= nt - bj) { p -= nt - bj; ++bj; }
    const int64_t j0 = bj * SUM_TILE, k0 = (bj + p) * SUM_TILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t k = k0 + lane;
    double acc[16];
    const double w1 = sum_weight(g.t[g.first]);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int64_t j = j0 + wave + 4 * i;
        acc[i] = (k < n && j <= k) ? w1 * quad[tri_pos(n, j, k)].coeff : 0.0;
    }
    for (int b = g.first + 1; b < g.nterms; ++b) {
        if (g.t[b].kind != PMT_LSQ_BLOCK) continue;
        const double wb = sum_weight(g.t[b]);
        const double *__restrict__ v = g.t[b].values;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = wave + 4 * i;
            const int64_t kc = k0 + c, jr = j0 + lane;
            tile[c][lane] = (kc < n && jr <= kc) ? v[kc * (kc + 1) / 2 + jr] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = acc[i] + wb * tile[lane][wave + 4 * i];
    }
    if (g.has_d) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (j0 + wave + 4 * i != k) continue;
            bool any;
            const double d = sum_diag_shift_at(g, cs, k, any);
            if (any) acc[i] = acc[i] + d;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) tile[wave + 4 * i][lane] = acc[i];
    __syncthreads();
    typedef unsigned long long u64w;
    typedef u64w u64w2 __attribute__((ext_vector_type(2)));
    for (int r = 0; r < 16; ++r) {
        const int jj = wave * 16 + r;
        const int64_t j = j0 + jj;
        if (j >= n) break;
        const int64_t ks = k0 > j ? k0 : j, ke = (k0 + SUM_TILE < n) ? k0 + SUM_TILE : n;
        if (ke <= ks) continue;
        // the row's terms ks .. ke - 1 as 16-byte chunks (as wave_write_words, common.h): the coefficient words from LDS, the row / column
        // words as they are (read back through the same, non-restrict, pointer: each lane stores only the words it has read)
        u64w *seg = reinterpret_cast<u64w *>(quad + tri_pos(n, j, ks));
        const int off = (int)(ks - k0), nwords = 3 * (int)(ke - ks);
        const int lead = (int)((reinterpret_cast<uintptr_t>(seg) >> 3) & 1);
        auto word = [&](int q) -> u64w { return q % 3 == 0 ? (u64w)__double_as_longlong(tile[jj][off + q / 3]) : seg[q]; };
        if (lead && lane == 0) seg[0] = word(0);
        for (int c = lane; lead + 2 * c < nwords; c += 64) {
            const int q0 = lead + 2 * c;
            if (q0 + 1 < nwords) {
                u64w2 v;
                v.x = word(q0);
                v.y = word(q0 + 1);
                *reinterpret_cast<u64w2 *>(seg + q0) = v;
            } else {
                seg[q0] = word(q0);
            }
        }
    }
}

// lin[j] for one j per thread; with `diag` (block 1 alone, weight the constant +1: the off-diagonal coefficients stay as they are) the n
// diagonal coefficients too.
template <class Cols>
__device__ __forceinline__ void gram_sum_aux(const SumArgs &g, const Cols &cs, QT *__restrict__ quad, LT *__restrict__ lin, int diag) {
    const int64_t n = g.n;
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    LT t = lin[j];
    double c = sum_weight(g.t[g.first]) * t.coeff;
    for (int b = g.first + 1; b < g.nterms; ++b)
        if (g.t[b].kind == PMT_LSQ_BLOCK) c = c + sum_weight(g.t[b]) * g.t[b].lin[j].coeff;
    for (int i = 0; i < g.nterms; ++i) {
        if (g.t[i].kind != PMT_LSQ_DIAG || !g.t[i].vec) continue;
        const int64_t v = cs.find(i, j);
        if (v >= 0) c = c + sum_weight(g.t[i]) * (2 * signed_const(g.t[i].vec[v], g.t[i].sign));
    }
    for (int i = 0; i < g.nterms; ++i) {
        if (g.t[i].kind != PMT_LSQ_LINEAR) continue;
        const int64_t v = cs.find(i, j);
        if (v >= 0) c = c + sum_weight(g.t[i]) * g.t[i].vec[v];
    }
    t.coeff = c;
    lin[j] = t;
    if (diag && g.has_d) {
        bool any;
        const double d = sum_diag_shift_at(g, cs, j, any);
        double *q = &quad[tri_pos(n, j, j)].coeff;
        if (any) *q = sum_weight(g.t[g.first]) * *q + d;
    }
}

// The constant, one workgroup: sum_k W_k*cc_k, then W_d * (sum_j v_j^2) per diagonal term with v, then the scalar constants — each in
// expression order.  sum_j v_j^2: thread t adds j = t, t + 256, .. in order; the 256 partial sums in a halving tree (t + 128, .., t + 1).
template <class Cols>
__device__ __forceinline__ void gram_sum_const(const SumArgs &g, const Cols &cs, double *__restrict__ cst) {
    __shared__ double red[256];
    const int64_t n = g.n;
    const int tid = threadIdx.x;
    double s = sum_weight(g.t[g.first]) * *cst;
    for (int b = g.first + 1; b < g.nterms; ++b)
        if (g.t[b].kind == PMT_LSQ_BLOCK) s = s + sum_weight(g.t[b]) * *g.t[b].constant;
    for (int i = 0; i < g.nterms; ++i) {
        if (g.t[i].kind != PMT_LSQ_DIAG || !g.t[i].vec) continue;
        const double *__restrict__ v = g.t[i].vec;
        double part = 0.0;
        const int64_t nv = cs.len(i, n);
        for (int64_t jj = tid; jj < nv; jj += 256) part = part + v[jj] * v[jj];
        __syncthreads();
        red[tid] = part;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if (tid < h) red[tid] = red[tid] + red[tid + h];
            __syncthreads();
        }
        s = s + sum_weight(g.t[i]) * red[0];
    }
    for (int i = 0; i < g.nterms; ++i)
        if (g.t[i].kind == PMT_LSQ_CONSTANT) s = s + sum_weight(g.t[i]) * (g.t[i].vec ? *g.t[i].vec : 1.0);
    __syncthreads();                    // every thread has read *cst
    if (tid == 0) *cst = s;
}

__global__ __launch_bounds__(256) void gram_sum_tile_kernel(SumArgs g, QT *__restrict__ quad) { gram_sum_tile(g, AllCols{}, quad); }
__global__ __launch_bounds__(256) void gram_sum_aux_kernel(SumArgs g, QT *__restrict__ quad, LT *__restrict__ lin, int diag) {
    gram_sum_aux(g, AllCols{}, quad, lin, diag);
}
__global__ __launch_bounds__(256) void gram_sum_const_kernel(SumArgs g, double *__restrict__ cst) { gram_sum_const(g, AllCols{}, cst); }

// pmt_quad_gram_sum_sub_f64: the same kernels over the terms' runs of positions
__global__ __launch_bounds__(256) void gram_sum_sub_tile_kernel(SumArgs g, SubCols cs, QT *__restrict__ quad) { gram_sum_tile(g, cs, quad); }
__global__ __launch_bounds__(256) void gram_sum_sub_aux_kernel(SumArgs g, SubCols cs, QT *__restrict__ quad, LT *__restrict__ lin, int diag) {
    gram_sum_aux(g, cs, quad, lin, diag);
}
__global__ __launch_bounds__(256) void gram_sum_sub_const_kernel(SumArgs g, SubCols cs, double *__restrict__ cst) { gram_sum_const(g, cs, cst); }

}  // namespace pmt

using namespace pmt;

namespace {

// the checks and the kernel arguments shared by both entries; `diag`: block 1 alone with the constant weight +1
int sum_args(const char *who, int64_t cols, const pmt_lsq_term *terms, int nterms, pmt_quadratic_term *out_quad, pmt_linear_term *out_lin,
             double *out_const, SumArgs &g, int &diag) {
    const std::string w(who);
    PMT_REQUIRE(cols >= 0, PMT_DIMENSION_MISMATCH, w + ": negative column count");
    PMT_REQUIRE(terms, PMT_INVALID_ARGUMENT, w + ": null term list");
    PMT_REQUIRE(nterms >= 1 && nterms <= PMT_LSQ_MAX_TERMS, PMT_INVALID_ARGUMENT, w + ": 1 .. 32 terms");
    g.n = cols; g.nterms = nterms; g.first = -1; g.has_d = 0;
    int nblocks = 0;
    for (int i = 0; i < nterms; ++i) {
        const pmt_lsq_term &t = terms[i];
        switch (t.kind) {
        case PMT_LSQ_BLOCK:
            if (nblocks++ == 0) {
                g.first = i;
            } else {
                PMT_REQUIRE(t.values && t.lin && t.constant, PMT_INVALID_ARGUMENT, w + ": null value array of a block");
            }
            break;
        case PMT_LSQ_DIAG:
            PMT_REQUIRE(!t.vec || t.sign == 1 || t.sign == -1, PMT_INVALID_ARGUMENT, w + ": diagonal term sign must be +1 or -1");
            g.has_d = 1;
            break;
        case PMT_LSQ_LINEAR:
            PMT_REQUIRE(t.vec, PMT_INVALID_ARGUMENT, w + ": null coefficient vector of a linear term");
            break;
        case PMT_LSQ_CONSTANT:
            break;
        default:
            return fail(PMT_INVALID_ARGUMENT, w + ": unknown term kind");
        }
        g.t[i] = t;
    }
    PMT_REQUIRE(nblocks >= 1 && nblocks <= PMT_LSQ_MAX_BLOCKS, PMT_INVALID_ARGUMENT, w + ": 1 .. 8 least-squares blocks");
    PMT_REQUIRE(out_const && (cols == 0 || (out_quad && out_lin)), PMT_INVALID_ARGUMENT, w + ": null output");
    const pmt_lsq_term &b1 = terms[g.first];
    diag = nblocks == 1 && !b1.weight && b1.scale == 1.0;
    return PMT_OK;
}

}  // namespace

extern "C" int pmt_quad_gram_sum_f64(int64_t cols, const pmt_lsq_term *terms, int nterms, pmt_quadratic_term *out_quad,
                                     pmt_linear_term *out_lin, double *out_const, void *stream) {
    SumArgs g;
    int diag = 0;
    const int rc0 = sum_args("quad_gram_sum", cols, terms, nterms, out_quad, out_lin, out_const, g, diag);
    if (rc0 != PMT_OK) return rc0;
    return dispatch(stream, [=](hipStream_t s) {
        if (!diag && cols > 0) {
            const int64_t nt = cdiv(cols, SUM_TILE);
            PMT_LAUNCH(gram_sum_tile_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, s, g, out_quad);
            int rc = check_launch("gram_sum_tile_kernel");
            if (rc != PMT_OK) return rc;
        }
        if (cols > 0) {
            PMT_LAUNCH(gram_sum_aux_kernel, dim3((unsigned)cdiv(cols, 256)), dim3(256), 0, s, g, out_quad, out_lin, diag);
            int rc = check_launch("gram_sum_aux_kernel");
            if (rc != PMT_OK) return rc;
        }
        // the constant reads the blocks' c'c: inside a plan's replay the stream-K node writes it at the END of the replay (gram.hip,
        // const_part), so this launch queues behind it there
        return gram_after_deferred(s, [=]() -> int {
            PMT_LAUNCH(gram_sum_const_kernel, dim3(1), dim3(256), 0, s, g, out_const);
            return check_launch("gram_sum_const_kernel");
        });
    });
}

extern "C" int pmt_quad_gram_sum_sub_f64(int64_t cols, const pmt_lsq_term *terms, int nterms, const int64_t *const *term_cols,
                                         const int64_t *term_ncols, pmt_quadratic_term *out_quad, pmt_linear_term *out_lin, double *out_const,
                                         void *stream) {
    SumArgs g;
    int diag = 0;
    const int rc0 = sum_args("quad_gram_sum_sub", cols, terms, nterms, out_quad, out_lin, out_const, g, diag);
    if (rc0 != PMT_OK) return rc0;
    PMT_REQUIRE(cols <= INT32_MAX, PMT_DIMENSION_MISMATCH, "quad_gram_sum_sub: more than 2^31 - 1 columns");
    SubCols cs;
    int nruns = 0;
    for (int i = 0; i < nterms; ++i) {
        const int64_t *list = term_cols ? term_cols[i] : nullptr;
        cs.first[i] = nruns;
        cs.count[i] = -1;
        cs.nvec[i] = (int32_t)cols;
        if (!list) continue;
        const int kind = terms[i].kind;
        PMT_REQUIRE(kind == PMT_LSQ_DIAG || kind == PMT_LSQ_LINEAR, PMT_INVALID_ARGUMENT,
                    "quad_gram_sum_sub: only diagonal and linear terms take a column list");
        PMT_REQUIRE(term_ncols, PMT_INVALID_ARGUMENT, "quad_gram_sum_sub: null column counts");
        const int64_t m = term_ncols[i];
        PMT_REQUIRE(m >= 0 && m <= cols, PMT_DIMENSION_MISMATCH, "quad_gram_sum_sub: column count outside 0 .. cols");
        int count = 0;
        for (int64_t k = 0; k < m; ++k) {
            const int64_t j = list[k];
            PMT_REQUIRE(j >= 0 && j < cols, PMT_DIMENSION_MISMATCH, "quad_gram_sum_sub: column position outside 0 .. cols-1");
            PMT_REQUIRE(k == 0 || j > list[k - 1], PMT_INVALID_ARGUMENT, "quad_gram_sum_sub: column positions not strictly increasing");
            if (k > 0 && j == list[k - 1] + 1) {
                ++cs.run_len[nruns - 1];
                continue;
            }
            PMT_REQUIRE(nruns < PMT_LSQ_MAX_RUNS, PMT_INVALID_ARGUMENT, "quad_gram_sum_sub: more than 64 runs of positions");
            cs.start[nruns] = (int32_t)j;
            cs.run_len[nruns] = 1;
            cs.base[nruns] = (int32_t)k;
            ++nruns;
            ++count;
        }
        cs.count[i] = count;
        cs.nvec[i] = (int32_t)m;
    }
    for (int r = nruns; r < PMT_LSQ_MAX_RUNS; ++r) cs.start[r] = cs.run_len[r] = cs.base[r] = 0;
    for (int i = nterms; i < PMT_LSQ_MAX_TERMS; ++i) cs.first[i] = cs.count[i] = cs.nvec[i] = 0;
    return dispatch(stream, [=](hipStream_t s) {
        if (!diag && cols > 0) {
            const int64_t nt = cdiv(cols, SUM_TILE);
            PMT_LAUNCH(gram_sum_sub_tile_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, s, g, cs, out_quad);
            int rc = check_launch("gram_sum_sub_tile_kernel");
            if (rc != PMT_OK) return rc;
        }
        if (cols > 0) {
            PMT_LAUNCH(gram_sum_sub_aux_kernel, dim3((unsigned)cdiv(cols, 256)), dim3(256), 0, s, g, cs, out_quad, out_lin, diag);
            int rc = check_launch("gram_sum_sub_aux_kernel");
            if (rc != PMT_OK) return rc;
        }
        return gram_after_deferred(s, [=]() -> int {
            PMT_LAUNCH(gram_sum_sub_const_kernel, dim3(1), dim3(256), 0, s, g, cs, out_const);
            return check_launch("gram_sum_sub_const_kernel");
        });
    });
}
