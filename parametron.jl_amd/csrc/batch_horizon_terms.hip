// Batched MPC horizons with a terminal cost, a weight per stage and linear stage terms: B independent instances,
//     J_i = sum_{t<T} wx_{i,t} * transpose(x_t (+|-) r_{i,t}) * Q_i * (x_t (+|-) r_{i,t}) + dot(gx_{i,t}, x_t)
//                   + wu_{i,t} * transpose(u_t (+|-) v_{i,t}) * R_i * (u_t (+|-) v_{i,t}) + dot(gu_{i,t}, u_t)
//           + wN_i * transpose(x_T (+|-) rN_i) * P_i * (x_T (+|-) rN_i) + dot(gN_i, x_T)
// over z = [x_0; u_0; ..; x_{T-1}; u_{T-1}; x_T] (x_T only with a P) subject to C_i*z (+|-) d_i, one slab
//     [ SQ | SR | SP: term*nx(nx+1)/2 | W: ns | q: n | const: 1 | C: m*n row-major | d-consts: m ],   n = T*(nx + nu) + term*nx
// per instance (pmt_batch_horizon_terms_coeffs_f64), ns = T*(1 + (nu > 0)) + term stages in z order.  Per stage the words are those of
// pmt_quad_stages_terms_f64 (quad_stages.hip) with scale = 1.0, weight = &W_s, lin_vec = g_s: in the reference mul! of the stage's function
// by the weight (src/functions.jl:244 for the add! of the stages) beside what batch_horizon.hip lists.
//
// The walk is horizon_tile.h's, as in batch_horizon.hip: one workgroup of 256 threads per instance, persistent; Q_i's tiles formed once and
// kept in LDS, the section written from them, the T stages out of LDS.  Then the same for R_i and — the third phase — for P_i with its one
// stage x_T, all through the same tiles.  Here every stage has its weight and may have a linear vector (stages<NT, true>).  The W section
// is copied behind the phases, the stage on the lanes.
// The ns <= 2 * 512 + 1 stage constants (LDS, z order) are added in S_d's order; C_i and the d-consts as the sibling does them.
// LDS: 33280 (tile) + 2048 (c) + 8208 (1025 stage constants, padded) + 2048 (tree) = 45584 bytes with one tile: three workgroups per CU;
// 99840 + 4096 + 2048 (the two waves' products) + 8208 + 2048 = 116240 bytes with three: one workgroup per CU.
//
// pmt_batch_horizon_terms_expand_f64 rebuilds one instance's MOI buffers from its slab: the sibling's streaming writer with one multiply
// per quadratic term, coeff = W_s * S[j,k].
#include <algorithm>

#include "horizon_tile.h"

namespace pmt {

namespace {

constexpr int BT_MAX_STAGES = 2 * HT_MAX_T + 1;      // x_t and u_t of every t, and x_T
static_assert(sizeof(pmt_batch_horizon_terms) == 128, "fourteen pointers and four signs, no padding");

struct BatchHorizonTermsArgs {
    pmt_batch_horizon_terms in;                 // instance-major device pointers and the signs (include/parametron_hip.h)
    int64_t B, m;
    int T, nx, nu, term;
    double *out; int64_t out_stride;
};

}  // namespace

template <int NT>
__global__ __launch_bounds__(HT_THREADS) void batch_horizon_terms_kernel(BatchHorizonTermsArgs g) {
    __shared__ Tiles<NT> tl;
    __shared__ double cw[HT_WAVES][NT * HT_TILE];
    __shared__ double pr[HT_WAVES][HT_TILE];
    __shared__ double sc[BT_MAX_STAGES];
    __shared__ double red[HT_THREADS];
    const int T = g.T, nx = g.nx, nu = g.nu, term = g.term, w = nx + nu, n = T * w + term * nx;
    const int xs = nu > 0 ? 2 : 1, ns = T * xs + term;             // stages per t; stages of the instance
    const int64_t m = g.m, nqx = (int64_t)nx * (nx + 1) / 2, nqu = (int64_t)nu * (nu + 1) / 2, nqp = term ? nqx : 0;
    const int tid = threadIdx.x;

    for (int64_t inst = blockIdx.x; inst < g.B; inst += gridDim.x) {
        double *__restrict__ out = g.out + inst * g.out_stride;
        double *__restrict__ ow = out + nqx + nqu + nqp;
        double *__restrict__ oq = ow + ns;
        // d is asked for now and looked at at the end of the instance (every thread loads, thread t >= m the last entry again)
        double dv = 0.0;
        if (g.in.sign_d && m > 0) dv = g.in.d[inst * m + (tid < m ? tid : m - 1)];

        // Q_i and the stages x_t, R_i and the stages u_t, P_i and the stage x_T through the same tiles (one copy of the code: the registers of one)
        for (int ph = 0; ph < 3; ++ph) {
            if ((ph == 1 && nu == 0) || (ph == 2 && !term)) continue;
            const int nd = ph == 1 ? nu : nx, Tp = ph == 2 ? 1 : T;
            const int sign = ph == 0 ? g.in.sign_r : (ph == 1 ? g.in.sign_v : g.in.sign_rN);
            const double *Mb = ph == 0 ? g.in.Q : (ph == 1 ? g.in.R : g.in.P);
            const double *rb = ph == 0 ? g.in.r : (ph == 1 ? g.in.v : g.in.rN);
            const double *wb = ph == 0 ? g.in.wx : (ph == 1 ? g.in.wu : g.in.wN);
            const double *gb = ph == 0 ? g.in.gx : (ph == 1 ? g.in.gu : g.in.gN);
            const double *__restrict__ M = Mb + inst * nd * nd;
            const double *__restrict__ ref = (sign && rb) ? rb + inst * Tp * nd : nullptr;                 // (sign == 0: not read)
            const double *__restrict__ wts = wb ? wb + inst * Tp : nullptr;
            const double *__restrict__ gv = gb ? gb + inst * Tp * nd : nullptr;
            double *__restrict__ osec = ph == 0 ? out : (ph == 1 ? out + nqx : out + nqx + nqu);
            double *__restrict__ qd = ph == 0 ? oq : (ph == 1 ? oq + nx : oq + (int64_t)T * w);
            form<NT>(tl, M, nd, osec, tid);
            stages<NT, true>(tl, cw, pr, sc, ref, sign, wts, gv, nd, Tp, qd, w, ph == 2 ? T * xs : ph, xs, tid);
        }
        __syncthreads();

        // the W section: the stages' weights in z order as read, the stage on the lanes
        for (int s = tid; s < ns; s += HT_THREADS) {
            const bool last = s >= T * xs;
            const int t = last ? 0 : s / xs;
            const bool isu = !last && s - t * xs != 0;
            const double *wb = last ? g.in.wN : (isu ? g.in.wu : g.in.wx);
            ow[s] = wb ? wb[inst * (last ? 1 : T) + t] : 1.0;
        }

        // the stage constants in z order, added in S_d's order: 256 chains onto 0.0, then the halving tree
        // (batch_horizon.hip and batch_horizon_tv.hip's tail hold this sum too: moved into a shared function it compiles to other device code)
        {
            double s = 0.0;
            for (int t = tid; t < ns; t += HT_THREADS) s = s + sc[t];
            red[tid] = s;
            __syncthreads();
            for (int h = HT_THREADS / 2; h > 0; h >>= 1) {
                if (tid < h) red[tid] = red[tid] + red[tid + h];
                __syncthreads();
            }
            if (tid == 0) oq[n] = red[0];
        }

        // the constraint block: C_i column-major -> row-major through tile 0 (rows on the lanes in, columns on the lanes out)
        // (batch_horizon.hip and batch_horizon_tv.hip's tail hold this block too: moved into a shared function it compiles to other device code)
        if (m > 0) {
            const double *__restrict__ Ci = g.in.C + inst * m * n;
            double *__restrict__ oc = oq + n + 1;
            double (&tile)[HT_TILE][HT_TILE + 1] = tl.t[0];
            for (int64_t r0 = 0; r0 < m; r0 += HT_TILE) {
                for (int c0 = 0; c0 < n; c0 += HT_TILE) {
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
            if (tid < m) od[tid] = signed_const(dv, g.in.sign_d);
            for (int64_t r = tid + HT_THREADS; r < m; r += HT_THREADS) od[r] = g.in.sign_d ? signed_const(g.in.d[inst * m + r], g.in.sign_d) : 0.0;
        }
        __syncthreads();                                  // the next instance reuses the tiles, sc and red
    }
}

// One instance's MOI buffers from its slab.  A wave per unit, the units dealt out over the grid's waves: the n rows of quadratic terms
// (row j of a stage: its columns k >= j, each times the stage's weight), then 64 linear terms each, 64 vector-affine terms each, 64
// constants each.
__global__ __launch_bounds__(HT_THREADS) void batch_horizon_terms_expand_kernel(const double *__restrict__ slab, int T, int nx, int nu, int term,
                                                                                 int64_t m, const int64_t *__restrict__ xvar,
                                                                                 const int64_t *__restrict__ varmap, QT *__restrict__ oq,
                                                                                 LT *__restrict__ ol, double *__restrict__ oc, VAT *__restrict__ ov,
                                                                                 double *__restrict__ ovc) {
    const int lane = threadIdx.x & 63;
    const int64_t wv = (int64_t)blockIdx.x * HT_WAVES + (threadIdx.x >> 6), nwv = (int64_t)gridDim.x * HT_WAVES;
    const int w = nx + nu, xs = nu > 0 ? 2 : 1, ns = T * xs + term;
    const int64_t nz = (int64_t)T * w, n = nz + (int64_t)term * nx;
    const int64_t nqx = (int64_t)nx * (nx + 1) / 2, nqu = (int64_t)nu * (nu + 1) / 2, nqp = term ? nqx : 0;
    const double *__restrict__ sw = slab + nqx + nqu + nqp, *__restrict__ sq = sw + ns, *__restrict__ scn = sq + n + 1, *__restrict__ sd = scn + m * n;
    const int64_t nvat = m * n;
    const int64_t u1 = n, u2 = u1 + (n + 63) / 64, u3 = u2 + (nvat + 63) / 64, u4 = u3 + (m + 63) / 64;
    for (int64_t u = wv; u < u4; u += nwv) {
        if (u < u1) {
            // row u of z: stage x_t or u_t of t = u / w, or the terminal stage behind the T pairs
            const bool last = u >= nz;
            const int t = last ? T : (int)(u / w), wi = (int)(u - (int64_t)t * w);
            const bool isu = !last && wi >= nx;
            const int nd = isu ? nu : nx, j = isu ? wi - nx : wi;
            const int64_t zb = u - j;                                            // the stage's first variable in z
            const double *__restrict__ sec = (last ? slab + nqx + nqu : (isu ? slab + nqx : slab)) + tri_pos(nd, j, j);
            QT *__restrict__ dst = oq + (int64_t)t * (nqx + nqu) + (isu ? nqx : 0) + tri_pos(nd, j, j);
            expand_quad_row(sec, dst, sw + (last ? T * xs : t * xs + (isu ? 1 : 0)), nd - j, xvar + zb + j, varmap, lane);
        } else {
            expand_rest(u, u1, u2, u3, n, m, sq, scn, sd, xvar, varmap, ol, ov, ovc, lane);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *oc = sq[n];
}

}  // namespace pmt

using namespace pmt;

extern "C" int64_t pmt_batch_horizon_terms_slab_doubles(int64_t T, int64_t nx, int64_t nu, int64_t term, int64_t m) {
    const int64_t n = T * (nx + nu) + term * nx, ns = T * (nu > 0 ? 2 : 1) + term;
    return nx * (nx + 1) / 2 + nu * (nu + 1) / 2 + term * (nx * (nx + 1) / 2) + ns + n + 1 + m * n + m;
}

extern "C" int pmt_batch_horizon_terms_coeffs_f64(const pmt_batch_horizon_terms *in, int64_t B, int64_t T, int64_t nx, int64_t nu, int64_t m,
                                                  double *out, int64_t out_stride, void *stream) {
    PMT_REQUIRE(in, PMT_INVALID_ARGUMENT, "batch_horizon_terms: null descriptor");
    PMT_REQUIRE(B >= 0, PMT_DIMENSION_MISMATCH, "batch_horizon_terms: negative dimension");
    const int term = in->P ? 1 : 0;
    const int rc = check_dims("batch_horizon_terms", T, nx, nu, term, m);
    if (rc != PMT_OK) return rc;
    const int64_t L = pmt_batch_horizon_terms_slab_doubles(T, nx, nu, term, m);
    PMT_REQUIRE(out_stride >= L, PMT_DIMENSION_MISMATCH, "batch_horizon_terms: out_stride smaller than the slab");
    const auto sign_ok = [](int s) { return s >= -1 && s <= 1; };
    PMT_REQUIRE(sign_ok(in->sign_r) && sign_ok(in->sign_v) && sign_ok(in->sign_rN) && sign_ok(in->sign_d), PMT_INVALID_ARGUMENT,
                "batch_horizon_terms: signs must be -1, 0 or +1");
    if (B == 0) return PMT_OK;
    PMT_REQUIRE(out && in->Q && (nu == 0 || in->R) && (in->sign_r == 0 || in->r) && (nu == 0 || in->sign_v == 0 || in->v) &&
                    (!term || in->sign_rN == 0 || in->rN) && (m == 0 || (in->C && in->d)),
                PMT_INVALID_ARGUMENT, "batch_horizon_terms: null pointer");
    BatchHorizonTermsArgs g;
    g.in = *in;
    if (nu == 0) { g.in.R = nullptr; g.in.v = nullptr; g.in.wu = nullptr; g.in.gu = nullptr; }          // (no u stages: never read)
    if (!term) { g.in.rN = nullptr; g.in.wN = nullptr; g.in.gN = nullptr; }
    g.B = B; g.m = m;
    g.T = (int)T; g.nx = (int)nx; g.nu = (int)nu; g.term = term;
    g.out = out; g.out_stride = out_stride;
    return dispatch(stream, [=](hipStream_t s) {
        // resident workgroups (LDS): three per CU with one tile, one with three; each walks the instances blockIdx.x, blockIdx.x + G, ..
        if (std::max(g.nx, g.nu) <= HT_TILE) {
            const dim3 grid((unsigned)std::min<int64_t>(B, (int64_t)3 * cu_count()));
            PMT_LAUNCH(batch_horizon_terms_kernel<1>, grid, dim3(HT_THREADS), 0, s, g);
        } else {
            const dim3 grid((unsigned)std::min<int64_t>(B, (int64_t)cu_count()));
            PMT_LAUNCH(batch_horizon_terms_kernel<2>, grid, dim3(HT_THREADS), 0, s, g);
        }
        return check_launch("batch_horizon_terms_kernel");
    });
}

extern "C" int pmt_batch_horizon_terms_expand_f64(const double *slab, int64_t T, int64_t nx, int64_t nu, int64_t term, int64_t m,
                                                  const int64_t *xvar, const int64_t *varmap, pmt_quadratic_term *out_quad,
                                                  pmt_linear_term *out_lin, double *out_const, pmt_vector_affine_term *out_vat,
                                                  double *out_vconsts, void *stream) {
    const int rc = check_dims("batch_horizon_terms_expand", T, nx, nu, term, m);
    if (rc != PMT_OK) return rc;
    PMT_REQUIRE(slab && xvar && varmap && out_quad && out_lin && out_const && (m == 0 || (out_vat && out_vconsts)), PMT_INVALID_ARGUMENT,
                "batch_horizon_terms_expand: null pointer");
    const int iT = (int)T, inx = (int)nx, inu = (int)nu, iterm = (int)term;
    return dispatch(stream, [=](hipStream_t s) {
        PMT_LAUNCH(batch_horizon_terms_expand_kernel, expand_grid((int64_t)iT * (inx + inu) + (int64_t)iterm * inx, m), dim3(HT_THREADS), 0, s, slab, iT, inx,
                   inu, iterm, m, xvar, varmap, out_quad, out_lin, out_const, out_vat, out_vconsts);
        return check_launch("batch_horizon_terms_expand_kernel");
    });
}
