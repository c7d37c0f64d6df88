// Batched MPC horizons: B independent instances, each a whole horizon of stage costs
//     J_i = sum_{t<T} transpose(x_t (+|-) r_{i,t}) * Q_i * (x_t (+|-) r_{i,t}) + transpose(u_t (+|-) v_{i,t}) * R_i * (u_t (+|-) v_{i,t})
// over z = [x_0; u_0; x_1; u_1; ..] subject to C_i*z (+|-) d_i, one slab
//     [ SQ: nx(nx+1)/2 | SR: nu(nu+1)/2 | q: n | const: 1 | C: m*n row-major | d-consts: m ],   n = T*(nx + nu)
// per instance (pmt_batch_horizon_coeffs_f64).  In the reference a batch is many independent Models (src/model.jl:1-22); per instance this
// replaces, for every stage, matvecmul! over the affine vector (src/functions.jl:800-822) and vecdot! (:702-709 over :548-576), the add! of
// the stages (:244), canonicalize! (:381-386) and the MOI copies (src/moi_interop.jl:45-81), coefficients only.
//
// One workgroup of 256 threads per instance, persistent: workgroup g takes the instances g, g + G, ..  No workgroup waits for another, no
// atomics, no workspace.  The walk is horizon_tile.h's: Q_i's tiles formed once and kept in LDS, the SQ section written from them, the T
// stages x_t out of LDS; then the same for R_i and the stages u_t in the same LDS.  Here every stage is unweighted and has no linear
// vector (stages<NT, false>).  Then the stage constants (LDS, z order) in S_d's order, C_i transposed through tile 0 and the d-consts as
// batch_form_kernel does them.
// LDS: 33280 (tile) + 2048 (c) + 8192 (stage constants) + 2048 (tree) = 45568 bytes with one tile: three workgroups per CU;
// 99840 + 4096 + 2048 (the two waves' products) + 8192 + 2048 = 116224 bytes with three: one workgroup per CU.
//
// pmt_batch_horizon_expand_f64 rebuilds one instance's MOI buffers from its slab: a streaming writer, a wave per row of quadratic terms /
// per 64 linear or vector-affine terms through wave_write_words (common.h).
#include <algorithm>

#include "horizon_tile.h"

namespace pmt {

namespace {

// This file's own launch shape and bounds, the walk's (horizon_tile.h): tests/test_batch_horizon_host.py reads them here beside the header's
constexpr int BH_TILE = 64;
constexpr int BH_THREADS = 256;
constexpr int BH_WAVES = BH_THREADS / 64;
constexpr int BH_MAX_DIM = 128;
constexpr int BH_MAX_T = 512;
static_assert(BH_MAX_DIM == PMT_BATCH_HORIZON_MAX_DIM && BH_MAX_T == PMT_BATCH_HORIZON_MAX_T, "the header's bounds are the kernel's");
static_assert(BH_TILE == HT_TILE && BH_THREADS == HT_THREADS && BH_MAX_DIM == HT_MAX_DIM && BH_MAX_T == HT_MAX_T, "the walk's constants");

struct BatchHorizonArgs {
    const double *Q, *R, *r, *v, *C, *d;        // instance-major: Q[B][nx*nx], R[B][nu*nu] column-major, r[B][T*nx], v[B][T*nu], C[B][m*n], d[B][m]
    int64_t B, m;
    int T, nx, nu, sign_r, sign_v, sign_d;
    double *out; int64_t out_stride;
};

}  // namespace

template <int NT>
__global__ __launch_bounds__(BH_THREADS) void batch_horizon_kernel(BatchHorizonArgs g) {
    __shared__ Tiles<NT> tl;
    __shared__ double cw[BH_WAVES][NT * BH_TILE];
    __shared__ double pr[BH_WAVES][BH_TILE];
    __shared__ double sc[2 * BH_MAX_T];
    __shared__ double red[BH_THREADS];
    const int T = g.T, nx = g.nx, nu = g.nu, w = nx + nu, n = T * w;
    const int64_t m = g.m, nqx = (int64_t)nx * (nx + 1) / 2, nqu = (int64_t)nu * (nu + 1) / 2;
    const int tid = threadIdx.x;

    for (int64_t inst = blockIdx.x; inst < g.B; inst += gridDim.x) {
        double *__restrict__ out = g.out + inst * g.out_stride;
        double *__restrict__ oq = out + nqx + nqu;
        // d is asked for now and looked at at the end of the instance (every thread loads, thread t >= m the last entry again)
        double dv = 0.0;
        if (g.sign_d && m > 0) dv = g.d[inst * m + (tid < m ? tid : m - 1)];

        // Q_i and the stages x_t, then R_i and the stages u_t, through the same tiles (one copy of the code: the registers of one)
        for (int ph = 0; ph < (nu > 0 ? 2 : 1); ++ph) {
            const int nd = ph ? nu : nx, sign = ph ? g.sign_v : g.sign_r;
            const double *__restrict__ M = ph ? g.R + inst * nu * nu : g.Q + inst * nx * nx;
            const double *__restrict__ ref = !sign ? nullptr : (ph ? g.v + inst * T * nu : g.r + inst * T * nx);   // (sign == 0: not read)
            form<NT>(tl, M, nd, ph ? out + nqx : out, tid);
            stages<NT, false>(tl, cw, pr, sc, ref, sign, nullptr, nullptr, nd, T, ph ? oq + nx : oq, w, ph, nu > 0 ? 2 : 1, tid);
        }
        __syncthreads();

        // the stage constants in z order, added in S_d's order: 256 chains onto 0.0, then the halving tree
        // (batch_horizon_terms.hip and batch_horizon_tv.hip's tail hold this sum too: moved into a shared function it compiles to other device code)
        {
            const int nst = nu ? 2 * T : T;
            double s = 0.0;
            for (int t = tid; t < nst; t += BH_THREADS) s = s + sc[t];
            red[tid] = s;
            __syncthreads();
            for (int h = BH_THREADS / 2; h > 0; h >>= 1) {
                if (tid < h) red[tid] = red[tid] + red[tid + h];
                __syncthreads();
            }
            if (tid == 0) oq[n] = red[0];
        }

        // the constraint block: C_i column-major -> row-major through tile 0 (rows on the lanes in, columns on the lanes out)
        // (batch_horizon_terms.hip and batch_horizon_tv.hip's tail hold this block too: moved into a shared function it compiles to other device code)
        if (m > 0) {
            const double *__restrict__ Ci = g.C + inst * m * n;
            double *__restrict__ oc = oq + n + 1;
            double (&tile)[BH_TILE][BH_TILE + 1] = tl.t[0];
            for (int64_t r0 = 0; r0 < m; r0 += BH_TILE) {
                for (int c0 = 0; c0 < n; c0 += BH_TILE) {
                    int lane = tid & 63, wave = tid >> 6;
                    asm volatile("" : "+v"(lane), "+v"(wave));
                    double cin[16];
                    const int64_t r = r0 + lane, rc = r < m ? r : m - 1;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int c = c0 + wave + 4 * i;
                        cin[i] = Ci[(c < n ? c : n - 1) * m + rc];
                    }
                    landed(cin);
#pragma unroll
                    for (int i = 0; i < 16; ++i) tile[wave + 4 * i][lane] = cin[i];
                    __syncthreads();
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int64_t rr = r0 + wave + 4 * i;
                        const int c = c0 + lane;
                        if (rr < m && c < n) oc[rr * n + c] = tile[lane][wave + 4 * i];
                    }
                    __syncthreads();
                }
            }
            double *__restrict__ od = oc + m * n;
            if (tid < m) od[tid] = signed_const(dv, g.sign_d);
            for (int64_t r = tid + BH_THREADS; r < m; r += BH_THREADS) od[r] = g.sign_d ? signed_const(g.d[inst * m + r], g.sign_d) : 0.0;
        }
        __syncthreads();                                  // the next instance reuses the tiles, sc and red
    }
}

// One instance's MOI buffers from its slab.  A wave per unit, the units dealt out over the grid's waves: the n rows of quadratic terms
// (row j of a stage: its columns k >= j), then 64 linear terms each, 64 vector-affine terms each, 64 constants each.
__global__ __launch_bounds__(BH_THREADS) void batch_horizon_expand_kernel(const double *__restrict__ slab, int T, int nx, int nu, int64_t m,
                                                                           const int64_t *__restrict__ xvar, const int64_t *__restrict__ varmap,
                                                                           QT *__restrict__ oq, LT *__restrict__ ol, double *__restrict__ oc,
                                                                           VAT *__restrict__ ov, double *__restrict__ ovc) {
    const int lane = threadIdx.x & 63;
    const int64_t wv = (int64_t)blockIdx.x * BH_WAVES + (threadIdx.x >> 6), nwv = (int64_t)gridDim.x * BH_WAVES;
    const int w = nx + nu;
    const int64_t n = (int64_t)T * w, nqx = (int64_t)nx * (nx + 1) / 2, nqu = (int64_t)nu * (nu + 1) / 2;
    const double *__restrict__ sq = slab + nqx + nqu, *__restrict__ scn = sq + n + 1, *__restrict__ sd = scn + m * n;
    const int64_t nvat = m * n;
    const int64_t u1 = n, u2 = u1 + (n + 63) / 64, u3 = u2 + (nvat + 63) / 64, u4 = u3 + (m + 63) / 64;
    for (int64_t u = wv; u < u4; u += nwv) {
        if (u < u1) {
            const int t = (int)(u / w), wi = (int)(u - (int64_t)t * w);
            const bool isu = wi >= nx;
            const int nd = isu ? nu : nx, j = isu ? wi - nx : wi;
            const int64_t zb = u - j;                                            // the stage's first variable in z
            const double *__restrict__ sec = (isu ? slab + nqx : slab) + tri_pos(nd, j, j);
            QT *__restrict__ dst = oq + (int64_t)t * (nqx + nqu) + (isu ? nqx : 0) + tri_pos(nd, j, j);
            expand_quad_row(sec, dst, nullptr, nd - j, xvar + zb + j, varmap, lane);
        } else {
            expand_rest(u, u1, u2, u3, n, m, sq, scn, sd, xvar, varmap, ol, ov, ovc, lane);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *oc = sq[n];
}

}  // namespace pmt

using namespace pmt;

extern "C" int64_t pmt_batch_horizon_slab_doubles(int64_t T, int64_t nx, int64_t nu, int64_t m) {
    const int64_t n = T * (nx + nu);
    return nx * (nx + 1) / 2 + nu * (nu + 1) / 2 + n + 1 + m * n + m;
}

extern "C" int pmt_batch_horizon_coeffs_f64(const double *Q, const double *R, const double *r, const double *v, const double *Cm, const double *d,
                                            int64_t B, int64_t T, int64_t nx, int64_t nu, int64_t m, int sign_r, int sign_v, int sign_d,
                                            double *out, int64_t out_stride, void *stream) {
    PMT_REQUIRE(B >= 0, PMT_DIMENSION_MISMATCH, "batch_horizon: negative dimension");
    const int rc = check_dims("batch_horizon", T, nx, nu, 0, m);
    if (rc != PMT_OK) return rc;
    const int64_t L = pmt_batch_horizon_slab_doubles(T, nx, nu, m);
    PMT_REQUIRE(out_stride >= L, PMT_DIMENSION_MISMATCH, "batch_horizon: out_stride smaller than the slab");
    PMT_REQUIRE(sign_r >= -1 && sign_r <= 1 && sign_v >= -1 && sign_v <= 1 && sign_d >= -1 && sign_d <= 1, PMT_INVALID_ARGUMENT,
                "batch_horizon: signs must be -1, 0 or +1");
    if (B == 0) return PMT_OK;
    PMT_REQUIRE(out && Q && (nu == 0 || R) && (sign_r == 0 || r) && (nu == 0 || sign_v == 0 || v) && (m == 0 || (Cm && d)), PMT_INVALID_ARGUMENT,
                "batch_horizon: null pointer");
    BatchHorizonArgs g;
    g.Q = Q; g.R = R; g.r = r; g.v = v; g.C = Cm; g.d = d;
    g.B = B; g.m = m;
    g.T = (int)T; g.nx = (int)nx; g.nu = (int)nu; g.sign_r = sign_r; g.sign_v = sign_v; g.sign_d = sign_d;
    g.out = out; g.out_stride = out_stride;
    return dispatch(stream, [=](hipStream_t s) {
        // resident workgroups (LDS): three per CU with one tile, one with three; each walks the instances blockIdx.x, blockIdx.x + G, ..
        if (std::max(g.nx, g.nu) <= BH_TILE) {
            const dim3 grid((unsigned)std::min<int64_t>(B, (int64_t)3 * cu_count()));
            PMT_LAUNCH(batch_horizon_kernel<1>, grid, dim3(BH_THREADS), 0, s, g);
        } else {
            const dim3 grid((unsigned)std::min<int64_t>(B, (int64_t)cu_count()));
            PMT_LAUNCH(batch_horizon_kernel<2>, grid, dim3(BH_THREADS), 0, s, g);
        }
        return check_launch("batch_horizon_kernel");
    });
}

extern "C" int pmt_batch_horizon_expand_f64(const double *slab, int64_t T, int64_t nx, int64_t nu, int64_t m, const int64_t *xvar,
                                            const int64_t *varmap, pmt_quadratic_term *out_quad, pmt_linear_term *out_lin, double *out_const,
                                            pmt_vector_affine_term *out_vat, double *out_vconsts, void *stream) {
    const int rc = check_dims("batch_horizon_expand", T, nx, nu, 0, m);
    if (rc != PMT_OK) return rc;
    PMT_REQUIRE(slab && xvar && varmap && out_quad && out_lin && out_const && (m == 0 || (out_vat && out_vconsts)), PMT_INVALID_ARGUMENT,
                "batch_horizon_expand: null pointer");
    const int iT = (int)T, inx = (int)nx, inu = (int)nu;
    return dispatch(stream, [=](hipStream_t s) {
        PMT_LAUNCH(batch_horizon_expand_kernel, expand_grid((int64_t)iT * (inx + inu), m), dim3(BH_THREADS), 0, s, slab, iT, inx, inu, m, xvar, varmap,
                   out_quad, out_lin, out_const, out_vat, out_vconsts);
        return check_launch("batch_horizon_expand_kernel");
    });
}
