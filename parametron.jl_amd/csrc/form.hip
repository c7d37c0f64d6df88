// transpose(x) * Q * x as its canonical function: the symmetrising node behind pmt_quad_form_f64.
//
// The reference builds this objective with bilinearmul! (src/functions.jl:840-858): all n^2 terms (Q[j,k], x_j, x_k); canonicalize!
// (:381-386) then sorts them and adds the two terms of every pair {j, k}, and the MOI copy (src/moi_interop.jl:45-62) doubles the diagonal.
// Every off-diagonal coefficient is the sum of exactly two numbers and IEEE addition commutes, so the canonical function is
// Q[j,k] + Q[k,j] (j < k), 2*Q[j,j] on the diagonal, on the row-major upper triangle — bit for bit, whatever order the sort combines in.
//
// A tiled transpose-add, bound by HBM: 8 n^2 bytes read, 24 (terms) / 8 (CSC values) bytes per upper-triangle entry written.  One
// workgroup per 64 x 64 tile (J, K), J <= K, of the upper triangle.  Both source tiles are read along their columns (a column of Q is
// contiguous): tile (K, J) arrives with k on the lanes, which is the layout the row-major term array wants; tile (J, K) arrives with j on
// the lanes and goes through LDS to be read transposed (pitch 65 doubles: a lane stride of 130 dwords covers the 64 banks of a b64 read
// once per 32 lanes).  A diagonal tile is its own partner and is loaded once.  The sums go back through the same LDS image so that each
// wave writes whole row segments of 24-byte terms as 16-byte stores (wave_write_words, common.h), and the CSC values column by column.
#include "common.h"

namespace pmt {

constexpr int FORM_TILE = 64;
constexpr int FORM_THREADS = 256;
constexpr int64_t FORM_MAX_N = (int64_t)1 << 21;          // 2^15 tiles a side: the grid of tile pairs stays below 2^31

struct FormArgs {
    const double *Q; int64_t ldq, n;
    const int64_t *xvar; const int64_t *varmap;           // varmap: NULL with moi == 0 (native indices)
    int moi; double alpha;
    QT *quad; double *values; LT *lin; double *cst;
};

__device__ __forceinline__ int64_t form_tri_pos(int64_t n, int64_t j, int64_t k) { return j * n - (j * (j - 1)) / 2 + (k - j); }

__global__ __launch_bounds__(FORM_THREADS) void quad_form_kernel(FormArgs g) {
    __shared__ double tile[FORM_TILE][FORM_TILE + 1];
    __shared__ int64_t colvar[FORM_TILE];
    const int64_t n = g.n, ldq = g.ldq;
    const int64_t nt = (n + FORM_TILE - 1) / FORM_TILE;
    int64_t p = blockIdx.x, bj = 0;
    while (p >= nt - bj) { p -= nt - bj; ++bj; }
    const bool diagonal = p == 0;
    const int64_t j0 = bj * FORM_TILE, k0 = (bj + p) * FORM_TILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *__restrict__ Q = g.Q;

    // lower[i] = Q[k0 + lane, j0 + wave + 4 i] (k on the lanes); upper[i] = Q[j0 + lane, k0 + wave + 4 i] (j on the lanes)
    double lower[16], upper[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int64_t r = k0 + lane, c = j0 + wave + 4 * i;
        lower[i] = (r < n && c < n) ? Q[r + c * ldq] : 0.0;
    }
    if (!diagonal) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t r = j0 + lane, c = k0 + wave + 4 * i;
            upper[i] = (r < n && c < n) ? Q[r + c * ldq] : 0.0;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) upper[i] = lower[i];
    }
    if (tid < FORM_TILE) {
        const int64_t k = k0 + tid;
        const int64_t v = k < n ? map_var(g.varmap, g.xvar[k]) : 0;
        colvar[tid] = v;
        // the zero affine part (a least-squares block's out_lin / out_const: the node stands where a block stands in a sum)
        if (diagonal && g.lin && k < n) {
            LT t;
            t.coeff = 0.0;
            t.var = v;
            g.lin[k] = t;
        }
    }
    if (blockIdx.x == 0 && tid == 0 && g.cst) *g.cst = 0.0;
    // tile[kk][jj] = Q[j0 + jj, k0 + kk]
#pragma unroll
    for (int i = 0; i < 16; ++i) tile[wave + 4 * i][lane] = upper[i];
    __syncthreads();
    // s(jj = wave + 4 i, kk = lane) = Q[j,k] + Q[k,j]; the diagonal keeps Q[j,j] (doubled where it is written)
    double s[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int jj = wave + 4 * i;
        const double a = tile[lane][jj];
        s[i] = (diagonal && jj == lane) ? a : a + lower[i];
    }
    __syncthreads();
    // tile[jj][kk] = s
#pragma unroll
    for (int i = 0; i < 16; ++i) tile[wave + 4 * i][lane] = s[i];
    __syncthreads();
    const int64_t ke = (k0 + FORM_TILE < n) ? k0 + FORM_TILE : n;
    if (g.quad) {
        typedef unsigned long long u64w;
        for (int r = 0; r < 16; ++r) {
            const int jj = wave * 16 + r;
            const int64_t j = j0 + jj;
            if (j >= n) break;
            const int64_t ks = k0 > j ? k0 : j;
            if (ke <= ks) continue;
            const int off = (int)(ks - k0);
            const u64w rowvar = (u64w)map_var(g.varmap, g.xvar[j]);
            const bool dbl = g.moi && diagonal;                         // the row's first term is its diagonal term
            wave_write_words<3>(reinterpret_cast<u64w *>(g.quad + form_tri_pos(n, j, ks)), (int)(ke - ks), lane, [&](int q) -> u64w {
                const int t = q / 3, f = q - 3 * t;
                if (f == 1) return rowvar;
                if (f == 2) return (u64w)colvar[off + t];
                const double v = tile[jj][off + t];
                return (u64w)__double_as_longlong((dbl && t == 0) ? 2 * v : v);
            });
        }
    }
    if (g.values) {
        // CSC: column k holds rows 0 .. k; this tile's part of it, rows j0 .. min(j0 + 63, k), is contiguous (j on the lanes)
        const double alpha = g.alpha;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int kk = wave + 4 * i;
            const int64_t k = k0 + kk, j = j0 + lane;
            if (k >= n || j > k) continue;
            const double v = tile[lane][kk];
            g.values[k * (k + 1) / 2 + j] = alpha * (j == k ? 2 * v : v);
        }
    }
}

}  // namespace pmt

using namespace pmt;

extern "C" int pmt_quad_form_f64(const double *Q, int64_t ldq, int64_t n, const int64_t *xvar, int moi, const int64_t *varmap, double alpha,
                                 pmt_quadratic_term *out_quad, double *out_P_values, pmt_linear_term *out_lin, double *out_const,
                                 void *stream) {
    PMT_REQUIRE(Q, PMT_INVALID_ARGUMENT, "quad_form: null matrix");
    PMT_REQUIRE(xvar, PMT_INVALID_ARGUMENT, "quad_form: null variable indices");
    PMT_REQUIRE(n >= 1, PMT_INVALID_ARGUMENT, "quad_form: n < 1");
    PMT_REQUIRE(n <= FORM_MAX_N, PMT_INVALID_ARGUMENT, "quad_form: more than 2^21 variables");
    PMT_REQUIRE(ldq >= n, PMT_INVALID_ARGUMENT, "quad_form: ldq < n");
    PMT_REQUIRE(moi == 0 || varmap, PMT_INVALID_ARGUMENT, "quad_form: MOI indices without a varmap");
    PMT_REQUIRE(out_quad || out_P_values, PMT_INVALID_ARGUMENT, "quad_form: neither term nor value output");
    FormArgs g;
    g.Q = Q; g.ldq = ldq; g.n = n;
    g.xvar = xvar; g.varmap = moi ? varmap : nullptr;
    g.moi = moi; g.alpha = alpha;
    g.quad = out_quad; g.values = out_P_values; g.lin = out_lin; g.cst = out_const;
    return dispatch(stream, [=](hipStream_t s) {
        const int64_t nt = cdiv(n, FORM_TILE);
        PMT_LAUNCH(quad_form_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(FORM_THREADS), 0, s, g);
        return check_launch("quad_form_kernel");
    });
}
