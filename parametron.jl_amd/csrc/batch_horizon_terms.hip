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
// The walk is batch_horizon_kernel's (batch_horizon.hip): one workgroup of 256 threads per instance, persistent; S_Q's upper 64 x 64 tiles
// formed once and kept in LDS (one tile for dims <= 64, three for dims <= 128), the section written from them, the T matvecs out of LDS with
// one thread per row (a stage in 16, 32 or 64 lanes of a wave, or in two waves above 64 rows), the chains those of pmt_quad_form_shift_f64.
// Then the same for R_i and — the third phase — for P_i with its one stage x_T, all through the same tiles.  What is new sits where a
// stage's lin_j and constant are stored: q = W_s * lin_j (+ g_s[j]), constant = W_s * (0.5 * T_s); the chains stay unweighted, so they
// keep their order.  The W section is copied behind the phases, the stage on the lanes.  A stage's weight and its linear vector are fetched with its reference vector: unconditional on
// clamped indices, asked for a round ahead, in front of the chains.  A plain stage (sign 0) has no chain: W_s * +0.0 (+ g_s[j]).
// The ns <= 2 * 512 + 1 stage constants (LDS, z order) are added in S_d's order; C_i and the d-consts as the sibling does them.
// LDS: 33280 (tile) + 2048 (c) + 8208 (1025 stage constants, padded) + 2048 (tree) = 45584 bytes with one tile: three workgroups per CU;
// 99840 + 4096 + 2048 (the two waves' products) + 8208 + 2048 = 116240 bytes with three: one workgroup per CU.
//
// pmt_batch_horizon_terms_expand_f64 rebuilds one instance's MOI buffers from its slab: the sibling's streaming writer with one multiply
// per quadratic term, coeff = W_s * S[j,k].
#include <algorithm>

#include "common.h"

namespace pmt {

namespace {

constexpr int BT_TILE = 64;
constexpr int BT_THREADS = 256;
constexpr int BT_WAVES = BT_THREADS / 64;
constexpr int BT_MAX_DIM = 128;
constexpr int BT_MAX_T = 512;
constexpr int BT_MAX_STAGES = 2 * BT_MAX_T + 1;      // x_t and u_t of every t, and x_T
static_assert(BT_MAX_DIM == PMT_BATCH_HORIZON_MAX_DIM && BT_MAX_T == PMT_BATCH_HORIZON_MAX_T, "the header's bounds are the kernel's");
static_assert(BT_MAX_DIM <= 2 * BT_TILE, "at most two column blocks: three upper tiles");
static_assert(sizeof(pmt_batch_horizon_terms) == 128, "fourteen pointers and four signs, no padding");

struct BatchHorizonTermsArgs {
    pmt_batch_horizon_terms in;                 // instance-major device pointers and the signs (include/parametron_hip.h)
    int64_t B, m;
    int T, nx, nu, term;
    double *out; int64_t out_stride;
};

__device__ __forceinline__ int64_t bt_tri_pos(int64_t n, int64_t j, int64_t k) { return j * n - (j * (j - 1)) / 2 + (k - j); }

// ((s(0)*c(0) + s(1)*c(1)) + ..) + s(len-1)*c(len-1): the first product starts the chain.  The operands of eight steps are read from LDS
// together; the order of the additions is the chain's.
template <typename FS, typename FC>
__device__ __forceinline__ double bt_chain(int len, FS s, FC c) {
    double acc = s(0) * c(0);
    int k = 1;
    for (; k + 8 <= len; k += 8) {
        double a[8], b[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) { a[i] = s(k + i); b[i] = c(k + i); }
#pragma unroll
        for (int i = 0; i < 8; ++i) { const double pr = a[i] * b[i]; acc = acc + pr; }
    }
    for (; k < len; ++k) acc = acc + s(k) * c(k);
    return acc;
}

// Every element of v is in its register here: loads issued above this point are not moved below it or into a branch.
__device__ __forceinline__ void bt_landed(double (&v)[16]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) asm volatile("" : "+v"(v[i]));
}

template <int NT> struct BtTiles { double t[NT == 1 ? 1 : 3][BT_TILE][BT_TILE + 1]; };

// S = M + M' of one nd x nd matrix into the resident tiles — tile (bj, bk) at index bj + bk — and its section (tri(j,k), the diagonal
// doubled): batch_horizon.hip's bh_form
template <int NT>
__device__ __forceinline__ void bt_form(BtTiles<NT> &tl, const double *__restrict__ M, int nd, double *__restrict__ osec, int tid) {
    const int n = nd, nt = (n + BT_TILE - 1) / BT_TILE;
    __syncthreads();                                    // the matvecs of the matrix before are through with the tiles
    for (int bj = 0; bj < nt; ++bj) {
        for (int bk = bj; bk < nt; ++bk) {
            const bool diagonal = bk == bj;
            double (&tile)[BT_TILE][BT_TILE + 1] = tl.t[NT == 1 ? 0 : bj + bk];
            // (the lane's coordinates are made opaque per tile: derived from loop invariants, the compiler otherwise keeps every address
            // and predicate of the unrolled body below alive across the whole instance loop)
            int lane = tid & 63, wave = tid >> 6;
            asm volatile("" : "+v"(lane), "+v"(wave));
            const int j0 = bj * BT_TILE, k0 = bk * BT_TILE;
            // lower[i] = M[k0 + lane, j0 + wave + 4 i] (k on the lanes); upper[i] = M[j0 + lane, k0 + wave + 4 i] (j on the lanes)
            // Out-of-range entries are 0.0: the load goes to the matrix's last row / column instead and is dropped, so no load is
            // conditional.  All loads of a tile are issued before the first value is looked at (bt_landed).
            double lower[16], upper[16];
            const int rk = k0 + lane, rj = j0 + lane;
            const unsigned ork = (unsigned)(rk < n ? rk : n - 1), orj = (unsigned)(rj < n ? rj : n - 1);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int c = j0 + wave + 4 * i;
                lower[i] = M[ork + (unsigned)(c < n ? c : n - 1) * (unsigned)n];
            }
            if (!diagonal) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int c = k0 + wave + 4 * i;
                    upper[i] = M[orj + (unsigned)(c < n ? c : n - 1) * (unsigned)n];
                }
                bt_landed(upper);
#pragma unroll
                for (int i = 0; i < 16; ++i) upper[i] = (rj < n && k0 + wave + 4 * i < n) ? upper[i] : 0.0;
            }
            bt_landed(lower);
#pragma unroll
            for (int i = 0; i < 16; ++i) lower[i] = (rk < n && j0 + wave + 4 * i < n) ? lower[i] : 0.0;
            if (diagonal) {
#pragma unroll
                for (int i = 0; i < 16; ++i) upper[i] = lower[i];
            }
            // tile[kk][jj] = M[j0 + jj, k0 + kk]
#pragma unroll
            for (int i = 0; i < 16; ++i) tile[wave + 4 * i][lane] = upper[i];
            __syncthreads();
            // s(jj = wave + 4 i, kk = lane) = M[j,k] + M[k,j]; the diagonal keeps M[j,j] (doubled where it is used)
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
            // the section: row j holds its columns k >= j; this tile's piece of it, k on the lanes
#pragma unroll 4
            for (int r = 0; r < 16; ++r) {
                const int jj = wave * 16 + r, j = j0 + jj;
                const int k = k0 + lane;
                if (j < n && k < n && k >= j) {
                    const double v = tile[jj][lane];
                    osec[bt_tri_pos(n, j, k)] = (k == j) ? 2 * v : v;
                }
            }
        }
    }
}

// The T stages of one matrix out of the resident tiles.  Stage t is stage s = sc0 + t * scstride of the instance: q[t * zstride + j] =
// W_s * lin_j (+ g_s[j]), sc[s] = W_s * (0.5 * T_s).  `ref` holds the T reference vectors of nd numbers (not read with sign == 0), `wts`
// the T weights (NULL: 1.0), `gv` the T linear vectors of nd numbers (NULL: none).
template <int NT>
__device__ __forceinline__ void bt_stages(BtTiles<NT> &tl, double (&cw)[BT_WAVES][NT * BT_TILE], double (&pr)[BT_WAVES][BT_TILE], double *sc,
                                          const double *__restrict__ ref, int sign, const double *__restrict__ wts,
                                          const double *__restrict__ gv, int nd, int T, double *__restrict__ q, int zstride, int sc0,
                                          int scstride, int tid) {
    if (sign == 0) {
        // the plain stages: no chain, lin_j = +0.0 and T_s = +0.0 — W_s * +0.0 keeps the weight's sign and its NaN
        for (int i = tid; i < T * nd; i += BT_THREADS) {
            const int t = i / nd, j = i - t * nd;
            const double wv = wts ? wts[t] : 1.0;
            double ql = wv * 0.0;
            if (gv) ql = ql + gv[i];
            q[(int64_t)t * zstride + j] = ql;
        }
        for (int t = tid; t < T; t += BT_THREADS) {
            const double wv = wts ? wts[t] : 1.0;
            sc[sc0 + t * scstride] = wv * (0.5 * 0.0);
        }
        return;
    }
    int lane = tid & 63, wave = tid >> 6;
    asm volatile("" : "+v"(lane), "+v"(wave));
    const int nt = NT == 1 ? 1 : (nd + BT_TILE - 1) / BT_TILE;
    if (nt == 1) {
        // One column block: a stage lives in W = 16, 32 or 64 lanes of one wave, 64 / W stages side by side in a wave (lanes of different
        // stages read the same word of S: a broadcast).  The products never leave the wave: the tree's levels W/2 .. 1 are __shfl_down
        // inside the W lanes; the levels above add +0.0 to a chain that started from +0.0, which changes no bit.
        const int W = nd <= 16 ? 16 : (nd <= 32 ? 32 : 64), G = 64 / W;
        const int sub = lane / W, jl = lane - sub * W;
        const int per = BT_WAVES * G, rounds = (T + per - 1) / per;
        // the stage's reference word, weight and linear word of this lane (no load is conditional on the lane: a stage or a row past the
        // end loads the last one's again; `wts` and `gv` are the same for the whole launch)
        double cv = 0.0, wn = 1.0, gn = 0.0;
        auto ask = [&](int st) {
            const int64_t sl = st < T ? st : T - 1;
            const int64_t at = sl * nd + (jl < nd ? jl : nd - 1);
            cv = ref[at];
            if (wts) wn = wts[sl];
            if (gv) gn = gv[at];
        };
        ask(wave * G + sub);
        for (int rd = 0; rd < rounds; ++rd) {
            const int st = (rd * BT_WAVES + wave) * G + sub;
            const bool live = st < T && jl < nd;
            asm volatile("" : "+v"(cv), "+v"(wn), "+v"(gn));   // (looked at here; the next round's are asked for below, in front of the chains)
            cw[wave][lane] = signed_const(cv, sign);
            const double wv = wn, gj = gn;
            ask(st + per);
            __syncthreads();
            double prod = 0.0;
            if (live) {
                const double *cs = cw[wave] + sub * W;
                const double lin = bt_chain(nd, [&](int kk) { const double a = tl.t[0][jl][kk]; return kk == jl ? 2 * a : a; }, [&](int kk) { return cs[kk]; });
                double ql = wv * lin;
                if (gv) ql = ql + gj;
                q[(int64_t)st * zstride + jl] = ql;
                prod = cs[jl] * lin;
            }
            double t = 0.0 + prod;                      // chain j of the stage's tree: 0.0 + c_j*lin_j; a row past nd: 0.0
            for (int h = W >> 1; h > 0; h >>= 1) t = t + __shfl_down(t, h, W);
            if (live && jl == 0) {
                const double half = 0.5 * t;
                sc[sc0 + st * scstride] = wv * half;
            }
        }
        return;
    }
    const int units = T * nt, rounds = (units + BT_WAVES - 1) / BT_WAVES;
    const int kw0 = nd < BT_TILE ? nd : BT_TILE, kw1 = nd - BT_TILE;
    // the reference vector, the weight and this lane's linear word of the stage of unit u (a unit past the last loads the last stage's
    // again: no load is conditional on the lane)
    double ca, cb = 0.0, wn = 1.0, gn = 0.0;
    auto ask = [&](int u) {
        int st = nt == 2 ? u >> 1 : u;
        const int row = (nt == 2 ? (u & 1) * BT_TILE : 0) + lane;
        st = st < T ? st : T - 1;
        const double *__restrict__ rv = ref + (int64_t)st * nd;
        ca = rv[lane < nd ? lane : nd - 1];
        if (NT == 2) cb = rv[lane + BT_TILE < nd ? lane + BT_TILE : nd - 1];
        if (wts) wn = wts[st];
        if (gv) gn = gv[(int64_t)st * nd + (row < nd ? row : nd - 1)];
    };
    ask(wave);
    for (int rd = 0; rd < rounds; ++rd) {
        const int unit = rd * BT_WAVES + wave;
        const bool live = unit < units;
        const int st = nt == 2 ? unit >> 1 : unit, rb = nt == 2 ? unit & 1 : 0;
        asm volatile("" : "+v"(ca), "+v"(cb), "+v"(wn), "+v"(gn));   // (looked at here; the next round's are asked for below, in front of the chains)
        cw[wave][lane] = signed_const(ca, sign);
        if (NT == 2) cw[wave][BT_TILE + lane] = signed_const(cb, sign);
        const double wv = wn, gj = gn;
        ask(unit + BT_WAVES);
        __syncthreads();
        double prod = 0.0;
        const int j = rb * BT_TILE + lane;
        if (live && j < nd) {
            // plain multiplies and adds, ascending, the first product starting the chain; the blocks in order
            const double *cv = cw[wave];
            double lin;
            if (rb == 0) {
                lin = bt_chain(kw0, [&](int kk) { const double a = tl.t[0][lane][kk]; return kk == lane ? 2 * a : a; }, [&](int kk) { return cv[kk]; });
                if (NT == 2 && nt == 2) {
                    const double p1 = bt_chain(kw1, [&](int kk) { return tl.t[NT == 1 ? 0 : 1][lane][kk]; }, [&](int kk) { return cv[BT_TILE + kk]; });
                    lin = lin + p1;
                }
            } else {
                lin = bt_chain(kw0, [&](int kk) { return tl.t[NT == 1 ? 0 : 1][kk][lane]; }, [&](int kk) { return cv[kk]; });
                const double p1 = bt_chain(kw1, [&](int kk) { const double a = tl.t[NT == 1 ? 0 : 2][lane][kk]; return kk == lane ? 2 * a : a; },
                                           [&](int kk) { return cv[BT_TILE + kk]; });
                lin = lin + p1;
            }
            double ql = wv * lin;
            if (gv) ql = ql + gj;
            q[(int64_t)st * zstride + j] = ql;
            prod = cv[j] * lin;
        }
        pr[wave][lane] = 0.0 + prod;                    // chain j of the stage's tree: 0.0 + c_j*lin_j; a row past nd: 0.0
        __syncthreads();
        if (live && rb == 0) {
            double t = pr[wave][lane];
            if (nt == 2) t = t + pr[wave + 1][lane];    // (an even unit runs on an even wave, the stage's second half beside it)
            for (int h = 32; h > 0; h >>= 1) t = t + __shfl_down(t, h);
            if (lane == 0) {
                const double half = 0.5 * t;
                sc[sc0 + st * scstride] = wv * half;
            }
        }
    }
}

}  // namespace

template <int NT>
__global__ __launch_bounds__(BT_THREADS) void batch_horizon_terms_kernel(BatchHorizonTermsArgs g) {
    __shared__ BtTiles<NT> tl;
    __shared__ double cw[BT_WAVES][NT * BT_TILE];
    __shared__ double pr[BT_WAVES][BT_TILE];
    __shared__ double sc[BT_MAX_STAGES];
    __shared__ double red[BT_THREADS];
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
            bt_form<NT>(tl, M, nd, osec, tid);
            bt_stages<NT>(tl, cw, pr, sc, ref, sign, wts, gv, nd, Tp, qd, w, ph == 2 ? T * xs : ph, xs, tid);
        }
        __syncthreads();

        // the W section: the stages' weights in z order as read, the stage on the lanes
        for (int s = tid; s < ns; s += BT_THREADS) {
            const bool last = s >= T * xs;
            const int t = last ? 0 : s / xs;
            const bool isu = !last && s - t * xs != 0;
            const double *wb = last ? g.in.wN : (isu ? g.in.wu : g.in.wx);
            ow[s] = wb ? wb[inst * (last ? 1 : T) + t] : 1.0;
        }

        // the stage constants in z order, added in S_d's order: 256 chains onto 0.0, then the halving tree
        {
            double s = 0.0;
            for (int t = tid; t < ns; t += BT_THREADS) s = s + sc[t];
            red[tid] = s;
            __syncthreads();
            for (int h = BT_THREADS / 2; h > 0; h >>= 1) {
                if (tid < h) red[tid] = red[tid] + red[tid + h];
                __syncthreads();
            }
            if (tid == 0) oq[n] = red[0];
        }

        // the constraint block: C_i column-major -> row-major through tile 0 (rows on the lanes in, columns on the lanes out)
        if (m > 0) {
            const double *__restrict__ Ci = g.in.C + inst * m * n;
            double *__restrict__ oc = oq + n + 1;
            double (&tile)[BT_TILE][BT_TILE + 1] = tl.t[0];
            for (int64_t r0 = 0; r0 < m; r0 += BT_TILE) {
                for (int c0 = 0; c0 < n; c0 += BT_TILE) {
                    int lane = tid & 63, wave = tid >> 6;
                    asm volatile("" : "+v"(lane), "+v"(wave));
                    double cin[16];
                    const int64_t r = r0 + lane, rc = r < m ? r : m - 1;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int c = c0 + wave + 4 * i;
                        cin[i] = Ci[(c < n ? c : n - 1) * m + rc];
                    }
                    bt_landed(cin);
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
            for (int64_t r = tid + BT_THREADS; r < m; r += BT_THREADS) od[r] = g.in.sign_d ? signed_const(g.in.d[inst * m + r], g.in.sign_d) : 0.0;
        }
        __syncthreads();                                  // the next instance reuses the tiles, sc and red
    }
}

// One instance's MOI buffers from its slab.  A wave per unit, the units dealt out over the grid's waves: the n rows of quadratic terms
// (row j of a stage: its columns k >= j, each times the stage's weight), then 64 linear terms each, 64 vector-affine terms each, 64
// constants each.
__global__ __launch_bounds__(BT_THREADS) void batch_horizon_terms_expand_kernel(const double *__restrict__ slab, int T, int nx, int nu, int term,
                                                                                 int64_t m, const int64_t *__restrict__ xvar,
                                                                                 const int64_t *__restrict__ varmap, QT *__restrict__ oq,
                                                                                 LT *__restrict__ ol, double *__restrict__ oc, VAT *__restrict__ ov,
                                                                                 double *__restrict__ ovc) {
    typedef unsigned long long u64w;
    const int lane = threadIdx.x & 63;
    const int64_t wv = (int64_t)blockIdx.x * BT_WAVES + (threadIdx.x >> 6), nwv = (int64_t)gridDim.x * BT_WAVES;
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
            const double wt = sw[last ? T * xs : t * xs + (isu ? 1 : 0)];
            const double *__restrict__ sec = (last ? slab + nqx + nqu : (isu ? slab + nqx : slab)) + bt_tri_pos(nd, j, j);
            QT *__restrict__ dst = oq + (int64_t)t * (nqx + nqu) + (isu ? nqx : 0) + bt_tri_pos(nd, j, j);
            const u64w rowvar = (u64w)map_var(varmap, xvar[zb + j]);
            wave_write_words<3>(reinterpret_cast<u64w *>(dst), nd - j, lane, [&](int q) -> u64w {
                const int e = q / 3, f = q - 3 * e;
                if (f == 1) return rowvar;
                if (f == 2) return (u64w)map_var(varmap, xvar[zb + j + e]);
                return (u64w)__double_as_longlong(wt * sec[e]);
            });
        } else if (u < u2) {
            const int64_t e0 = (u - u1) * 64;
            const int cnt = (int)(n - e0 < 64 ? n - e0 : 64);
            wave_write_words<2>(reinterpret_cast<u64w *>(ol + e0), cnt, lane, [&](int q) -> u64w {
                const int64_t e = e0 + (q >> 1);
                return (q & 1) ? (u64w)map_var(varmap, xvar[e]) : (u64w)__double_as_longlong(sq[e]);
            });
        } else if (u < u3) {
            const int64_t e0 = (u - u2) * 64;
            const int cnt = (int)(nvat - e0 < 64 ? nvat - e0 : 64);
            wave_write_words<3>(reinterpret_cast<u64w *>(ov + e0), cnt, lane, [&](int q) -> u64w {
                const int k = q / 3, f = q - 3 * k;
                const int64_t e = e0 + k, row = e / n;
                if (f == 0) return (u64w)(row + 1);
                if (f == 2) return (u64w)map_var(varmap, xvar[e - row * n]);
                return (u64w)__double_as_longlong(scn[e]);
            });
        } else {
            const int64_t e = (u - u3) * 64 + lane;
            if (e < m) ovc[e] = sd[e];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *oc = sq[n];
}

static int bt_cu_count() {
    static int cus[16] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) { (void)hipGetLastError(); return 256; }
    if (!cus[dev]) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) { (void)hipGetLastError(); v = 256; }
        cus[dev] = v;
    }
    return cus[dev];
}

// the dimension checks both entry points share; `who` words the message
static int bt_check_dims(const char *who, int64_t T, int64_t nx, int64_t nu, int64_t term, int64_t m) {
    const std::string w(who);
    PMT_REQUIRE(T >= 0 && nx >= 0 && nu >= 0 && m >= 0, PMT_DIMENSION_MISMATCH, w + ": negative dimension");
    PMT_REQUIRE(nx >= 1, PMT_DIMENSION_MISMATCH, w + ": nx < 1");
    PMT_REQUIRE(nx <= BT_MAX_DIM && nu <= BT_MAX_DIM, PMT_DIMENSION_MISMATCH, w + ": nx or nu above 128");
    PMT_REQUIRE(T >= 1 && T <= BT_MAX_T, PMT_DIMENSION_MISMATCH, w + ": T outside 1 .. 512");
    PMT_REQUIRE(term == 0 || term == 1, PMT_DIMENSION_MISMATCH, w + ": term must be 0 or 1");
    PMT_REQUIRE(m <= (INT64_C(1) << 40), PMT_DIMENSION_MISMATCH, w + ": m beyond 2^40");
    return PMT_OK;
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
    const int rc = bt_check_dims("batch_horizon_terms", T, nx, nu, term, m);
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
        if (std::max(g.nx, g.nu) <= BT_TILE) {
            const dim3 grid((unsigned)std::min<int64_t>(B, (int64_t)3 * bt_cu_count()));
            PMT_LAUNCH(batch_horizon_terms_kernel<1>, grid, dim3(BT_THREADS), 0, s, g);
        } else {
            const dim3 grid((unsigned)std::min<int64_t>(B, (int64_t)bt_cu_count()));
            PMT_LAUNCH(batch_horizon_terms_kernel<2>, grid, dim3(BT_THREADS), 0, s, g);
        }
        return check_launch("batch_horizon_terms_kernel");
    });
}

extern "C" int pmt_batch_horizon_terms_expand_f64(const double *slab, int64_t T, int64_t nx, int64_t nu, int64_t term, int64_t m,
                                                  const int64_t *xvar, const int64_t *varmap, pmt_quadratic_term *out_quad,
                                                  pmt_linear_term *out_lin, double *out_const, pmt_vector_affine_term *out_vat,
                                                  double *out_vconsts, void *stream) {
    const int rc = bt_check_dims("batch_horizon_terms_expand", T, nx, nu, term, m);
    if (rc != PMT_OK) return rc;
    PMT_REQUIRE(slab && xvar && varmap && out_quad && out_lin && out_const && (m == 0 || (out_vat && out_vconsts)), PMT_INVALID_ARGUMENT,
                "batch_horizon_terms_expand: null pointer");
    const int iT = (int)T, inx = (int)nx, inu = (int)nu, iterm = (int)term;
    return dispatch(stream, [=](hipStream_t s) {
        const int64_t n = (int64_t)iT * (inx + inu) + (int64_t)iterm * inx;
        const int64_t units = n + cdiv(n, 64) + cdiv(m * n, 64) + cdiv(m, 64);
        PMT_LAUNCH(batch_horizon_terms_expand_kernel, dim3((unsigned)std::min<int64_t>(cdiv(units, BT_WAVES), 4096)), dim3(BT_THREADS), 0, s, slab,
                   iT, inx, inu, iterm, m, xvar, varmap, out_quad, out_lin, out_const, out_vat, out_vconsts);
        return check_launch("batch_horizon_terms_expand_kernel");
    });
}
