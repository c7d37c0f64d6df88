// Batched MPC horizons: B independent instances, each a whole horizon of stage costs
//     J_i = sum_{t<T} transpose(x_t (+|-) r_{i,t}) * Q_i * (x_t (+|-) r_{i,t}) + transpose(u_t (+|-) v_{i,t}) * R_i * (u_t (+|-) v_{i,t})
// over z = [x_0; u_0; x_1; u_1; ..] subject to C_i*z (+|-) d_i, one slab
//     [ SQ: nx(nx+1)/2 | SR: nu(nu+1)/2 | q: n | const: 1 | C: m*n row-major | d-consts: m ],   n = T*(nx + nu)
// per instance (pmt_batch_horizon_coeffs_f64).  In the reference a batch is many independent Models (src/model.jl:1-22); per instance this
// replaces, for every stage, matvecmul! over the affine vector (src/functions.jl:800-822) and vecdot! (:702-709 over :548-576), the add! of
// the stages (:244), canonicalize! (:381-386) and the MOI copies (src/moi_interop.jl:45-81), coefficients only.
//
// One workgroup of 256 threads per instance, persistent: workgroup g takes the instances g, g + G, ..  No workgroup waits for another, no
// atomics, no workspace.  Every stage of an instance shares S_Q = Q_i + Q_i' and S_R, so the workgroup forms S_Q's upper 64 x 64 tiles ONCE,
// as batch_form_kernel (batch_form.hip) forms an instance's — both source tiles read along their columns, every load of a tile issued before
// the first value is looked at, the transpose-add through the tile of pitch 65 doubles — and KEEPS them in LDS: one tile for dims <= 64,
// three (0,0), (0,1), (1,1) for dims <= 128 (the kernel is instantiated by that count).  It writes the SQ section from them and then runs
// the T matvecs S_Q * c_t out of LDS, one thread per row: with dims above 64 a wave per 64 rows of a stage, two waves a stage; up to 64 a
// stage in 16, 32 or 64 lanes of one wave, so 16, 8 or 4 stages run side by side (8192 x (32, 32, 16, 0): 323 us with a wave per stage,
// profiles/r20_batch_horizon.txt for the packed form).  The stage's c_t = 0.0 (+|-) r_t lies in a buffer of the wave's own, the next
// round's values are asked for before this round's chains run.  A
// row's chains are those include/parametron_hip.h fixes for pmt_quad_form_shift_f64 (64-column blocks, the first product starting the chain,
// the blocks in order; the lower tile (1,0) is tile (0,1) read along its columns), the stage's constant its 256-entry tree: with dims <= 128
// the levels 128 and — up to 64 rows — 64 add +0.0 to a chain that started from +0.0, which changes no bit, so the tree starts with the two
// waves' products added and ends in the wave (__shfl_down 32 .. 1).  Then the same for R_i in the same LDS, the stage constants (LDS, z
// order) in S_d's order, C_i transposed through tile 0 and the d-consts as batch_form_kernel does them.
// LDS: 33280 (tile) + 2048 (c) + 8192 (stage constants) + 2048 (tree) = 45568 bytes with one tile: three workgroups per CU;
// 99840 + 4096 + 2048 (the two waves' products) + 8192 + 2048 = 116224 bytes with three: one workgroup per CU.
//
// pmt_batch_horizon_expand_f64 rebuilds one instance's MOI buffers from its slab: a streaming writer, a wave per row of quadratic terms /
// per 64 linear or vector-affine terms through wave_write_words (common.h).
#include <algorithm>

#include "common.h"

namespace pmt {

namespace {

constexpr int BH_TILE = 64;
constexpr int BH_THREADS = 256;
constexpr int BH_WAVES = BH_THREADS / 64;
constexpr int BH_MAX_DIM = 128;
constexpr int BH_MAX_T = 512;
static_assert(BH_MAX_DIM == PMT_BATCH_HORIZON_MAX_DIM && BH_MAX_T == PMT_BATCH_HORIZON_MAX_T, "the header's bounds are the kernel's");
static_assert(BH_MAX_DIM <= 2 * BH_TILE, "at most two column blocks: three upper tiles");

struct BatchHorizonArgs {
    const double *Q, *R, *r, *v, *C, *d;        // instance-major: Q[B][nx*nx], R[B][nu*nu] column-major, r[B][T*nx], v[B][T*nu], C[B][m*n], d[B][m]
    int64_t B, m;
    int T, nx, nu, sign_r, sign_v, sign_d;
    double *out; int64_t out_stride;
};

__device__ __forceinline__ int64_t bh_tri_pos(int64_t n, int64_t j, int64_t k) { return j * n - (j * (j - 1)) / 2 + (k - j); }

// ((s(0)*c(0) + s(1)*c(1)) + ..) + s(len-1)*c(len-1): the first product starts the chain.  The operands of eight steps are read from LDS
// together; the order of the additions is the chain's.
template <typename FS, typename FC>
__device__ __forceinline__ double bh_chain(int len, FS s, FC c) {
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
__device__ __forceinline__ void bh_landed(double (&v)[16]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) asm volatile("" : "+v"(v[i]));
}

template <int NT> struct BhTiles { double t[NT == 1 ? 1 : 3][BH_TILE][BH_TILE + 1]; };

// S = M + M' of one nd x nd matrix into the resident tiles — tile (bj, bk) at index bj + bk — and its section (tri(j,k), the diagonal doubled)
template <int NT>
__device__ __forceinline__ void bh_form(BhTiles<NT> &tl, const double *__restrict__ M, int nd, double *__restrict__ osec, int tid) {
    const int n = nd, nt = (n + BH_TILE - 1) / BH_TILE;
    __syncthreads();                                    // the matvecs of the matrix before are through with the tiles
    for (int bj = 0; bj < nt; ++bj) {
        for (int bk = bj; bk < nt; ++bk) {
            const bool diagonal = bk == bj;
            double (&tile)[BH_TILE][BH_TILE + 1] = tl.t[NT == 1 ? 0 : bj + bk];
            // (the lane's coordinates are made opaque per tile: derived from loop invariants, the compiler otherwise keeps every address
            // and predicate of the unrolled body below alive across the whole instance loop)
            int lane = tid & 63, wave = tid >> 6;
            asm volatile("" : "+v"(lane), "+v"(wave));
            const int j0 = bj * BH_TILE, k0 = bk * BH_TILE;
            // lower[i] = M[k0 + lane, j0 + wave + 4 i] (k on the lanes); upper[i] = M[j0 + lane, k0 + wave + 4 i] (j on the lanes)
            // Out-of-range entries are 0.0: the load goes to the matrix's last row / column instead and is dropped, so no load is
            // conditional.  All loads of a tile are issued before the first value is looked at (bh_landed).
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
                bh_landed(upper);
#pragma unroll
                for (int i = 0; i < 16; ++i) upper[i] = (rj < n && k0 + wave + 4 * i < n) ? upper[i] : 0.0;
            }
            bh_landed(lower);
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
                    osec[bh_tri_pos(n, j, k)] = (k == j) ? 2 * v : v;
                }
            }
        }
    }
}

// The T stages of one matrix out of the resident tiles: q[t * zstride + j] = lin_j of stage t, sc[sc0 + t * scstride] = its constant.
// `ref` holds the instance's T reference vectors of nd numbers (not read with sign == 0: the plain stages, +0.0 throughout).
template <int NT>
__device__ __forceinline__ void bh_stages(BhTiles<NT> &tl, double (&cw)[BH_WAVES][NT * BH_TILE], double (&pr)[BH_WAVES][BH_TILE], double *sc,
                                          const double *__restrict__ ref, int sign, int nd, int T, double *__restrict__ q, int zstride, int sc0,
                                          int scstride, int tid) {
    if (sign == 0) {
        for (int i = tid; i < T * nd; i += BH_THREADS) {
            const int t = i / nd, j = i - t * nd;
            q[(int64_t)t * zstride + j] = 0.0;
        }
        for (int t = tid; t < T; t += BH_THREADS) sc[sc0 + t * scstride] = 0.0;
        return;
    }
    int lane = tid & 63, wave = tid >> 6;
    asm volatile("" : "+v"(lane), "+v"(wave));
    const int nt = NT == 1 ? 1 : (nd + BH_TILE - 1) / BH_TILE;
    if (nt == 1) {
        // One column block: a stage lives in W = 16, 32 or 64 lanes of one wave, 64 / W stages side by side in a wave (lanes of different
        // stages read the same word of S: a broadcast).  The products never leave the wave: the tree's levels W/2 .. 1 are __shfl_down
        // inside the W lanes; the levels above add +0.0 to a chain that started from +0.0, which changes no bit.
        const int W = nd <= 16 ? 16 : (nd <= 32 ? 32 : 64), G = 64 / W;
        const int sub = lane / W, jl = lane - sub * W;
        const int per = BH_WAVES * G, rounds = (T + per - 1) / per;
        double cv = 0.0;
        auto ask = [&](int st) { cv = ref[(int64_t)(st < T ? st : T - 1) * nd + (jl < nd ? jl : nd - 1)]; };      // (no load is conditional)
        ask(wave * G + sub);
        for (int rd = 0; rd < rounds; ++rd) {
            const int st = (rd * BH_WAVES + wave) * G + sub;
            const bool live = st < T && jl < nd;
            asm volatile("" : "+v"(cv));                // (looked at here; the next round's is asked for below, in front of the chains)
            cw[wave][lane] = signed_const(cv, sign);
            ask(st + per);
            __syncthreads();
            double prod = 0.0;
            if (live) {
                const double *cs = cw[wave] + sub * W;
                const double lin = bh_chain(nd, [&](int kk) { const double a = tl.t[0][jl][kk]; return kk == jl ? 2 * a : a; }, [&](int kk) { return cs[kk]; });
                q[(int64_t)st * zstride + jl] = lin;
                prod = cs[jl] * lin;
            }
            double t = 0.0 + prod;                      // chain j of the stage's tree: 0.0 + c_j*lin_j; a row past nd: 0.0
            for (int h = W >> 1; h > 0; h >>= 1) t = t + __shfl_down(t, h, W);
            if (live && jl == 0) sc[sc0 + st * scstride] = 0.5 * t;
        }
        return;
    }
    const int units = T * nt, rounds = (units + BH_WAVES - 1) / BH_WAVES;
    const int kw0 = nd < BH_TILE ? nd : BH_TILE, kw1 = nd - BH_TILE;
    // the reference vector of the stage of unit u (a unit past the last loads the last stage's again: no load is conditional)
    double ca, cb = 0.0;
    auto ask = [&](int u) {
        int st = nt == 2 ? u >> 1 : u;
        st = st < T ? st : T - 1;
        const double *__restrict__ rv = ref + (int64_t)st * nd;
        ca = rv[lane < nd ? lane : nd - 1];
        if (NT == 2) cb = rv[lane + BH_TILE < nd ? lane + BH_TILE : nd - 1];
    };
    ask(wave);
    for (int rd = 0; rd < rounds; ++rd) {
        const int unit = rd * BH_WAVES + wave;
        const bool live = unit < units;
        const int st = nt == 2 ? unit >> 1 : unit, rb = nt == 2 ? unit & 1 : 0;
        asm volatile("" : "+v"(ca), "+v"(cb));          // (looked at here; the next round's are asked for below, in front of the chains)
        cw[wave][lane] = signed_const(ca, sign);
        if (NT == 2) cw[wave][BH_TILE + lane] = signed_const(cb, sign);
        ask(unit + BH_WAVES);
        __syncthreads();
        double prod = 0.0;
        const int j = rb * BH_TILE + lane;
        if (live && j < nd) {
            // plain multiplies and adds, ascending, the first product starting the chain; the blocks in order
            const double *cv = cw[wave];
            double lin;
            if (rb == 0) {
                lin = bh_chain(kw0, [&](int kk) { const double a = tl.t[0][lane][kk]; return kk == lane ? 2 * a : a; }, [&](int kk) { return cv[kk]; });
                if (NT == 2 && nt == 2) {
                    const double p1 = bh_chain(kw1, [&](int kk) { return tl.t[NT == 1 ? 0 : 1][lane][kk]; }, [&](int kk) { return cv[BH_TILE + kk]; });
                    lin = lin + p1;
                }
            } else {
                lin = bh_chain(kw0, [&](int kk) { return tl.t[NT == 1 ? 0 : 1][kk][lane]; }, [&](int kk) { return cv[kk]; });
                const double p1 = bh_chain(kw1, [&](int kk) { const double a = tl.t[NT == 1 ? 0 : 2][lane][kk]; return kk == lane ? 2 * a : a; },
                                           [&](int kk) { return cv[BH_TILE + kk]; });
                lin = lin + p1;
            }
            q[(int64_t)st * zstride + j] = lin;
            prod = cv[j] * lin;
        }
        pr[wave][lane] = 0.0 + prod;                    // chain j of the stage's tree: 0.0 + c_j*lin_j; a row past nd: 0.0
        __syncthreads();
        if (live && rb == 0) {
            double t = pr[wave][lane];
            if (nt == 2) t = t + pr[wave + 1][lane];    // (an even unit runs on an even wave, the stage's second half beside it)
            for (int h = 32; h > 0; h >>= 1) t = t + __shfl_down(t, h);
            if (lane == 0) sc[sc0 + st * scstride] = 0.5 * t;
        }
    }
}

}  // namespace

template <int NT>
__global__ __launch_bounds__(BH_THREADS) void batch_horizon_kernel(BatchHorizonArgs g) {
    __shared__ BhTiles<NT> tl;
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
            bh_form<NT>(tl, M, nd, ph ? out + nqx : out, tid);
            bh_stages<NT>(tl, cw, pr, sc, ref, sign, nd, T, ph ? oq + nx : oq, w, ph, nu > 0 ? 2 : 1, tid);
        }
        __syncthreads();

        // the stage constants in z order, added in S_d's order: 256 chains onto 0.0, then the halving tree
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
                    bh_landed(cin);
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
    typedef unsigned long long u64w;
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
            const double *__restrict__ sec = (isu ? slab + nqx : slab) + bh_tri_pos(nd, j, j);
            QT *__restrict__ dst = oq + (int64_t)t * (nqx + nqu) + (isu ? nqx : 0) + bh_tri_pos(nd, j, j);
            const u64w rowvar = (u64w)map_var(varmap, xvar[zb + j]);
            wave_write_words<3>(reinterpret_cast<u64w *>(dst), nd - j, lane, [&](int q) -> u64w {
                const int e = q / 3, f = q - 3 * e;
                if (f == 1) return rowvar;
                if (f == 2) return (u64w)map_var(varmap, xvar[zb + j + e]);
                return (u64w)__double_as_longlong(sec[e]);
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

static int bh_cu_count() {
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
static int bh_check_dims(const char *who, int64_t T, int64_t nx, int64_t nu, int64_t m) {
    const std::string w(who);
    PMT_REQUIRE(T >= 0 && nx >= 0 && nu >= 0 && m >= 0, PMT_DIMENSION_MISMATCH, w + ": negative dimension");
    PMT_REQUIRE(nx >= 1, PMT_DIMENSION_MISMATCH, w + ": nx < 1");
    PMT_REQUIRE(nx <= BH_MAX_DIM && nu <= BH_MAX_DIM, PMT_DIMENSION_MISMATCH, w + ": nx or nu above 128");
    PMT_REQUIRE(T >= 1 && T <= BH_MAX_T, PMT_DIMENSION_MISMATCH, w + ": T outside 1 .. 512");
    PMT_REQUIRE(m <= (INT64_C(1) << 40), PMT_DIMENSION_MISMATCH, w + ": m beyond 2^40");
    return PMT_OK;
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
    const int rc = bh_check_dims("batch_horizon", T, nx, nu, m);
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
            const dim3 grid((unsigned)std::min<int64_t>(B, (int64_t)3 * bh_cu_count()));
            PMT_LAUNCH(batch_horizon_kernel<1>, grid, dim3(BH_THREADS), 0, s, g);
        } else {
            const dim3 grid((unsigned)std::min<int64_t>(B, (int64_t)bh_cu_count()));
            PMT_LAUNCH(batch_horizon_kernel<2>, grid, dim3(BH_THREADS), 0, s, g);
        }
        return check_launch("batch_horizon_kernel");
    });
}

extern "C" int pmt_batch_horizon_expand_f64(const double *slab, int64_t T, int64_t nx, int64_t nu, int64_t m, const int64_t *xvar,
                                            const int64_t *varmap, pmt_quadratic_term *out_quad, pmt_linear_term *out_lin, double *out_const,
                                            pmt_vector_affine_term *out_vat, double *out_vconsts, void *stream) {
    const int rc = bh_check_dims("batch_horizon_expand", T, nx, nu, m);
    if (rc != PMT_OK) return rc;
    PMT_REQUIRE(slab && xvar && varmap && out_quad && out_lin && out_const && (m == 0 || (out_vat && out_vconsts)), PMT_INVALID_ARGUMENT,
                "batch_horizon_expand: null pointer");
    const int iT = (int)T, inx = (int)nx, inu = (int)nu;
    return dispatch(stream, [=](hipStream_t s) {
        const int64_t n = (int64_t)iT * (inx + inu);
        const int64_t units = n + cdiv(n, 64) + cdiv(m * n, 64) + cdiv(m, 64);
        PMT_LAUNCH(batch_horizon_expand_kernel, dim3((unsigned)std::min<int64_t>(cdiv(units, BH_WAVES), 4096)), dim3(BH_THREADS), 0, s, slab, iT, inx,
                   inu, m, xvar, varmap, out_quad, out_lin, out_const, out_vat, out_vconsts);
        return check_launch("batch_horizon_expand_kernel");
    });
}
