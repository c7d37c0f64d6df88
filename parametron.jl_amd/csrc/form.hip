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
//
// The shifted form transpose(x (+|-) v) * Q * (x (+|-) v) behind pmt_quad_form_shift_f64 — the reference's matvecmul! over the affine vector
// (src/functions.jl:800-822) and vecdot! (:702-709 over :548-576) in front of the same canonicalize! and MOI copy — is the same pass over Q:
// the quadratic part is the plain form's, and lin = (Q + Q')c, const = 0.5 c'lin come from the S a tile already holds in LDS (SHIFT below).
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
    const double *v; int sign; double *part;              // the shifted form (pmt_quad_form_shift_f64): x (+|-) v, the workspace P[nb + 1][n]
};

// SHIFT: the tile of the shifted form transpose(x (+|-) v) * Q * (x (+|-) v).  The quadratic part is the plain form's; the tile's S, in LDS
// after the transpose-add, also gives this tile's share of lin = S*c: one chain per row over the tile's columns (P[K][j], j in block J) and,
// off the diagonal, one per column over its rows (P[J][k], k in block K; S is bitwise symmetric).  Every (B, j) of the workspace is written
// by exactly one thread of the launch; quad_form_shift_lin_kernel adds the blocks.
template <bool SHIFT>
__device__ __forceinline__ void quad_form_tile(const FormArgs &g) {
    __shared__ double tile[FORM_TILE][FORM_TILE + 1];
    __shared__ int64_t colvar[FORM_TILE];
    __shared__ double cj[SHIFT ? FORM_TILE : 1], ck[SHIFT ? FORM_TILE : 1];
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
        if (SHIFT) ck[tid] = k < n ? signed_const(g.v[k], g.sign) : 0.0;
        // the zero affine part (a least-squares block's out_lin / out_const: the node stands where a block stands in a sum)
        if (!SHIFT && diagonal && g.lin && k < n) {
            LT t;
            t.coeff = 0.0;
            t.var = v;
            g.lin[k] = t;
        }
    }
    if (SHIFT && tid >= FORM_TILE && tid < 2 * FORM_TILE) {
        const int64_t j = j0 + tid - FORM_TILE;
        cj[tid - FORM_TILE] = j < n ? signed_const(g.v[j], g.sign) : 0.0;
    }
    if (!SHIFT && blockIdx.x == 0 && tid == 0 && g.cst) *g.cst = 0.0;
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
    if (SHIFT) {
        // tile[jj][kk] = S[j0 + jj, k0 + kk] (a diagonal tile: Q[j,j] at jj == kk, doubled here); plain multiplies and adds, ascending
        const int kw = (int)(ke - k0);
        const int jw = (int)(((j0 + FORM_TILE < n) ? j0 + FORM_TILE : n) - j0);
        if (wave == 0 && lane < jw) {
            auto S = [&](int kk) { const double a = tile[lane][kk]; return (diagonal && kk == lane) ? 2 * a : a; };
            double acc = S(0) * ck[0];
            for (int kk = 1; kk < kw; ++kk) acc = acc + S(kk) * ck[kk];
            g.part[(bj + p) * n + j0 + lane] = acc;
        } else if (wave == 1 && !diagonal && lane < kw) {
            double acc = tile[0][lane] * cj[0];
            for (int jj = 1; jj < jw; ++jj) acc = acc + tile[jj][lane] * cj[jj];
            g.part[bj * n + k0 + lane] = acc;
        }
    }
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
            wave_write_words<3>(reinterpret_cast<u64w *>(g.quad + tri_pos(n, j, ks)), (int)(ke - ks), lane, [&](int q) -> u64w {
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

__global__ __launch_bounds__(FORM_THREADS) void quad_form_kernel(FormArgs g) { quad_form_tile<false>(g); }
__global__ __launch_bounds__(FORM_THREADS) void quad_form_shift_kernel(FormArgs g) { quad_form_tile<true>(g); }

// lin_j = ((P[0][j] + P[1][j]) + ..) + P[nb-1][j]
__device__ __forceinline__ double form_shift_lin_at(const double *__restrict__ part, int64_t n, int64_t nb, int64_t j) {
    double s = part[j];
    int64_t b = 1;
    for (; b + 8 <= nb; b += 8) {                       // eight loads in flight, added in block order
        double a[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = part[(b + i) * n + j];
#pragma unroll
        for (int i = 0; i < 8; ++i) s = s + a[i];
    }
    for (; b < nb; ++b) s = s + part[b * n + j];
    return s;
}

// Behind quad_form_shift_kernel on the stream: one thread per j adds the blocks' partials, stores the linear term and, when a constant is
// wanted, leaves the product c_j*lin_j in the workspace's last row (row nb).  Workgroups of one wave: n / 64 of them share the n*nb loads.
__global__ __launch_bounds__(FORM_TILE) void quad_form_shift_lin_kernel(FormArgs g) {
    const int64_t n = g.n, nb = (n + FORM_TILE - 1) / FORM_TILE;
    const int64_t j = (int64_t)blockIdx.x * FORM_TILE + threadIdx.x;
    if (j >= n) return;
    const double lin = form_shift_lin_at(g.part, n, nb, j);
    if (g.lin) {
        LT t;
        t.coeff = lin;
        t.var = map_var(g.varmap, g.xvar[j]);
        g.lin[j] = t;
    }
    if (g.cst) g.part[nb * n + j] = signed_const(g.v[j], g.sign) * lin;
}

// Behind that: one workgroup adds the n products in S_d's order (gram_sum.hip: 256 chains onto 0.0, a halving tree) and halves the sum.
// Stream order alone puts the three launches behind each other: no workgroup waits for another.
__global__ __launch_bounds__(FORM_THREADS) void quad_form_shift_const_kernel(FormArgs g) {
    __shared__ double red[FORM_THREADS];
    const int64_t n = g.n, nb = (n + FORM_TILE - 1) / FORM_TILE;
    const int tid = threadIdx.x;
    const double *__restrict__ prod = g.part + nb * n;
    double s = 0.0;
    for (int64_t j = tid; j < n; j += FORM_THREADS) s = s + prod[j];
    red[tid] = s;
    __syncthreads();
    for (int h = FORM_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] = red[tid] + red[tid + h];
        __syncthreads();
    }
    if (tid == 0) *g.cst = 0.5 * red[0];
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
    g.v = nullptr; g.sign = 0; g.part = nullptr;
    return dispatch(stream, [=](hipStream_t s) {
        const int64_t nt = cdiv(n, FORM_TILE);
        PMT_LAUNCH(quad_form_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(FORM_THREADS), 0, s, g);
        return check_launch("quad_form_kernel");
    });
}

extern "C" int64_t pmt_quad_form_shift_workspace_bytes(int64_t n) { return n < 1 ? 0 : 8 * (cdiv(n, FORM_TILE) + 1) * n; }

extern "C" int pmt_quad_form_shift_f64(const double *Q, int64_t ldq, int64_t n, const int64_t *xvar, const double *v, int sign, int moi,
                                       const int64_t *varmap, double alpha, pmt_quadratic_term *out_quad, double *out_P_values,
                                       pmt_linear_term *out_lin, double *out_const, void *workspace, void *stream) {
    PMT_REQUIRE(Q, PMT_INVALID_ARGUMENT, "quad_form_shift: null matrix");
    PMT_REQUIRE(xvar, PMT_INVALID_ARGUMENT, "quad_form_shift: null variable indices");
    PMT_REQUIRE(v, PMT_INVALID_ARGUMENT, "quad_form_shift: null vector");
    PMT_REQUIRE(workspace, PMT_INVALID_ARGUMENT, "quad_form_shift: null workspace");
    PMT_REQUIRE(sign == 1 || sign == -1, PMT_INVALID_ARGUMENT, "quad_form_shift: sign must be +1 or -1");
    PMT_REQUIRE(n >= 1, PMT_INVALID_ARGUMENT, "quad_form_shift: n < 1");
    PMT_REQUIRE(n <= FORM_MAX_N, PMT_INVALID_ARGUMENT, "quad_form_shift: more than 2^21 variables");
    PMT_REQUIRE(ldq >= n, PMT_INVALID_ARGUMENT, "quad_form_shift: ldq < n");
    PMT_REQUIRE(moi == 0 || varmap, PMT_INVALID_ARGUMENT, "quad_form_shift: MOI indices without a varmap");
    PMT_REQUIRE(out_quad || out_P_values, PMT_INVALID_ARGUMENT, "quad_form_shift: neither term nor value output");
    FormArgs g;
    g.Q = Q; g.ldq = ldq; g.n = n;
    g.xvar = xvar; g.varmap = moi ? varmap : nullptr;
    g.moi = moi; g.alpha = alpha;
    g.quad = out_quad; g.values = out_P_values; g.lin = out_lin; g.cst = out_const;
    g.v = v; g.sign = sign; g.part = static_cast<double *>(workspace);
    return dispatch(stream, [=](hipStream_t s) {
        const int64_t nt = cdiv(n, FORM_TILE);
        PMT_LAUNCH(quad_form_shift_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(FORM_THREADS), 0, s, g);
        const int rc = check_launch("quad_form_shift_kernel");
        if (rc != PMT_OK) return rc;
        if (!g.lin && !g.cst) return rc;
        PMT_LAUNCH(quad_form_shift_lin_kernel, dim3((unsigned)nt), dim3(FORM_TILE), 0, s, g);
        const int rl = check_launch("quad_form_shift_lin_kernel");
        if (rl != PMT_OK || !g.cst) return rl;
        PMT_LAUNCH(quad_form_shift_const_kernel, dim3(1), dim3(FORM_THREADS), 0, s, g);
        return check_launch("quad_form_shift_const_kernel");
    });
}
