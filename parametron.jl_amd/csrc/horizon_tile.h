// The tile walk of the batched horizon kernels (batch_horizon.hip, batch_horizon_terms.hip): what one workgroup of 256 threads does with one
// matrix of an instance and the stages that share it.
//
// Every stage of an instance shares S_Q = Q_i + Q_i' (and S_R, S_P), so the workgroup forms S's upper 64 x 64 tiles ONCE (form), as
// batch_form_kernel (batch_form.hip) forms an instance's — both source tiles read along their columns, every load of a tile issued before
// the first value is looked at, the transpose-add through the tile of pitch 65 doubles — and KEEPS them in LDS: one tile for dims <= 64,
// three (0,0), (0,1), (1,1) for dims <= 128 (the kernels are instantiated by that count, NT).  It writes the matrix's section from them and
// then runs the T matvecs S * c_t out of LDS (stages), one thread per row: with dims above 64 a wave per 64 rows of a stage, two waves a
// stage; up to 64 a stage in 16, 32 or 64 lanes of one wave, so 16, 8 or 4 stages run side by side (8192 x (32, 32, 16, 0): 323 us with a
// wave per stage, profiles/r20_batch_horizon.txt for the packed form).  The stage's c_t = 0.0 (+|-) r_t lies in a buffer of the wave's own,
// the next round's values are asked for before this round's chains run.  A row's chains are those include/parametron_hip.h fixes for
// pmt_quad_form_shift_f64 (64-column blocks, the first product starting the chain, the blocks in order; the lower tile (1,0) is tile (0,1)
// read along its columns), the stage's constant its 256-entry tree: with dims <= 128 the levels 128 and — up to 64 rows — 64 add +0.0 to a
// chain that started from +0.0, which changes no bit, so the tree starts with the two waves' products added and ends in the wave
// (__shfl_down 32 .. 1).
//
// TERMS (batch_horizon_terms.hip): a stage has a weight W_s and may have a linear vector g_s.  They sit where a stage's lin_j and constant
// are stored: q = W_s * lin_j (+ g_s[j]), constant = W_s * (0.5 * T_s); the chains stay unweighted, so they keep their order.  A stage's
// weight and its linear word are fetched with its reference word: unconditional on clamped indices, asked for a round ahead, in front of
// the chains.  A plain stage (sign 0) has no chain: W_s * +0.0 (+ g_s[j]).  Without TERMS the weight is the constant 1.0 and there is no
// linear vector: the multiplies and adds fold away and the device code is that of the unweighted walk.
//
// Beside the walk, what the horizon files share otherwise: the item walk of the kernels whose work item is a stage (HorizonItem), the
// pieces of the expand kernels (expand_quad_row, expand_rest, and their grid: expand_grid) and the objective entry points' dimension
// checks (check_dims).  What the two dynamics files share lies in dynamics_tile.h.
#pragma once
#include <algorithm>

#include "common.h"

namespace pmt {

constexpr int HT_TILE = 64;
constexpr int HT_THREADS = 256;
constexpr int HT_WAVES = HT_THREADS / 64;
constexpr int HT_MAX_DIM = 128;
constexpr int HT_MAX_T = 512;
static_assert(HT_MAX_DIM == PMT_BATCH_HORIZON_MAX_DIM && HT_MAX_T == PMT_BATCH_HORIZON_MAX_T, "the header's bounds are the kernel's");
static_assert(HT_MAX_DIM <= 2 * HT_TILE, "at most two column blocks: three upper tiles");

// Where the work item is a stage, not an instance (batch_horizon_ltv.hip, batch_horizon_tv.hip): an item's place (item = inst*per + s,
// `per` items an instance) and its walk in steps of `stride` items without a division per step — (inst, s) follows the item by adding
// (step_inst, step_s) = (stride / per, stride % per) with one carry
struct HorizonItem {
    int64_t item, inst;
    int s;
    __device__ __forceinline__ HorizonItem(unsigned first, int per) : item(first), inst(first / (unsigned)per), s((int)(first % (unsigned)per)) {}
    __device__ __forceinline__ void step(unsigned stride, int step_inst, int step_s, int per) {
        item += stride; inst += step_inst; s += step_s;
        if (s >= per) { s -= per; ++inst; }
    }
};

template <int NT> struct Tiles { double t[NT == 1 ? 1 : 3][HT_TILE][HT_TILE + 1]; };

// S = M + M' of one nd x nd matrix into the resident tiles — tile (bj, bk) at index bj + bk — and its section (tri(j,k), the diagonal doubled)
template <int NT>
__device__ __forceinline__ void form(Tiles<NT> &tl, const double *__restrict__ M, int nd, double *__restrict__ osec, int tid) {
    const int n = nd, nt = (n + HT_TILE - 1) / HT_TILE;
    __syncthreads();                                    // the matvecs of the matrix before are through with the tiles
    for (int bj = 0; bj < nt; ++bj) {
        for (int bk = bj; bk < nt; ++bk) {
            const bool diagonal = bk == bj;
            double (&tile)[HT_TILE][HT_TILE + 1] = tl.t[NT == 1 ? 0 : bj + bk];
            // (the lane's coordinates are made opaque per tile: derived from loop invariants, the compiler otherwise keeps every address
            // and predicate of the unrolled body below alive across the whole instance loop)
            int lane = tid & 63, wave = tid >> 6;
            asm volatile("" : "+v"(lane), "+v"(wave));
            const int j0 = bj * HT_TILE, k0 = bk * HT_TILE;
            // lower[i] = M[k0 + lane, j0 + wave + 4 i] (k on the lanes); upper[i] = M[j0 + lane, k0 + wave + 4 i] (j on the lanes)
            // Out-of-range entries are 0.0: the load goes to the matrix's last row / column instead and is dropped, so no load is
            // conditional.  All loads of a tile are issued before the first value is looked at (landed).
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
                landed(upper);
#pragma unroll
                for (int i = 0; i < 16; ++i) upper[i] = (rj < n && k0 + wave + 4 * i < n) ? upper[i] : 0.0;
            }
            landed(lower);
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
                    osec[tri_pos(n, j, k)] = (k == j) ? 2 * v : v;
                }
            }
        }
    }
}

// The T stages of one matrix out of the resident tiles.  Stage t is stage s = sc0 + t * scstride of the instance: q[t * zstride + j] =
// W_s * lin_j (+ g_s[j]), sc[s] = W_s * (0.5 * T_s).  `ref` holds the T reference vectors of nd numbers (not read with sign == 0: the
// plain stages, +0.0 throughout), `wts` the T weights (NULL: 1.0), `gv` the T linear vectors of nd numbers (NULL: none); without TERMS
// neither is looked at.
template <int NT, bool TERMS>
__device__ __forceinline__ void stages(Tiles<NT> &tl, double (&cw)[HT_WAVES][NT * HT_TILE], double (&pr)[HT_WAVES][HT_TILE], double *sc,
                                       const double *__restrict__ ref, int sign, const double *__restrict__ wts,
                                       const double *__restrict__ gv, int nd, int T, double *__restrict__ q, int zstride, int sc0,
                                       int scstride, int tid) {
    if constexpr (!TERMS) { wts = nullptr; gv = nullptr; }
    if (sign == 0) {
        // the plain stages: no chain, lin_j = +0.0 and T_s = +0.0 — W_s * +0.0 keeps the weight's sign and its NaN
        for (int i = tid; i < T * nd; i += HT_THREADS) {
            const int t = i / nd, j = i - t * nd;
            const double wv = wts ? wts[t] : 1.0;
            double ql = wv * 0.0;
            if (gv) ql = ql + gv[i];
            q[(int64_t)t * zstride + j] = ql;
        }
        for (int t = tid; t < T; t += HT_THREADS) {
            const double wv = wts ? wts[t] : 1.0;
            sc[sc0 + t * scstride] = wv * (0.5 * 0.0);
        }
        return;
    }
    int lane = tid & 63, wave = tid >> 6;
    asm volatile("" : "+v"(lane), "+v"(wave));
    const int nt = NT == 1 ? 1 : (nd + HT_TILE - 1) / HT_TILE;
    if (nt == 1) {
        // One column block: a stage lives in W = 16, 32 or 64 lanes of one wave, 64 / W stages side by side in a wave (lanes of different
        // stages read the same word of S: a broadcast).  The products never leave the wave: the tree's levels W/2 .. 1 are __shfl_down
        // inside the W lanes; the levels above add +0.0 to a chain that started from +0.0, which changes no bit.
        const int W = nd <= 16 ? 16 : (nd <= 32 ? 32 : 64), G = 64 / W;
        const int sub = lane / W, jl = lane - sub * W;
        const int per = HT_WAVES * G, rounds = (T + per - 1) / per;
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
            const int st = (rd * HT_WAVES + wave) * G + sub;
            const bool live = st < T && jl < nd;
            // (looked at here; the next round's are asked for below, in front of the chains)
            if constexpr (TERMS) asm volatile("" : "+v"(cv), "+v"(wn), "+v"(gn));
            else asm volatile("" : "+v"(cv));
            cw[wave][lane] = signed_const(cv, sign);
            const double wv = wn, gj = gn;
            ask(st + per);
            __syncthreads();
            double prod = 0.0;
            if (live) {
                const double *cs = cw[wave] + sub * W;
                const double lin = chain(nd, [&](int kk) { const double a = tl.t[0][jl][kk]; return kk == jl ? 2 * a : a; }, [&](int kk) { return cs[kk]; });
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
    const int units = T * nt, rounds = (units + HT_WAVES - 1) / HT_WAVES;
    const int kw0 = nd < HT_TILE ? nd : HT_TILE, kw1 = nd - HT_TILE;
    // the reference vector, the weight and this lane's linear word of the stage of unit u (a unit past the last loads the last stage's
    // again: no load is conditional on the lane)
    double ca, cb = 0.0, wn = 1.0, gn = 0.0;
    auto ask = [&](int u) {
        int st = nt == 2 ? u >> 1 : u;
        const int row = (nt == 2 ? (u & 1) * HT_TILE : 0) + lane;
        st = st < T ? st : T - 1;
        const double *__restrict__ rv = ref + (int64_t)st * nd;
        ca = rv[lane < nd ? lane : nd - 1];
        if (NT == 2) cb = rv[lane + HT_TILE < nd ? lane + HT_TILE : nd - 1];
        if (wts) wn = wts[st];
        if (gv) gn = gv[(int64_t)st * nd + (row < nd ? row : nd - 1)];
    };
    ask(wave);
    for (int rd = 0; rd < rounds; ++rd) {
        const int unit = rd * HT_WAVES + wave;
        const bool live = unit < units;
        const int st = nt == 2 ? unit >> 1 : unit, rb = nt == 2 ? unit & 1 : 0;
        // (looked at here; the next round's are asked for below, in front of the chains)
        if constexpr (TERMS) asm volatile("" : "+v"(ca), "+v"(cb), "+v"(wn), "+v"(gn));
        else asm volatile("" : "+v"(ca), "+v"(cb));
        cw[wave][lane] = signed_const(ca, sign);
        if (NT == 2) cw[wave][HT_TILE + lane] = signed_const(cb, sign);
        const double wv = wn, gj = gn;
        ask(unit + HT_WAVES);
        __syncthreads();
        double prod = 0.0;
        const int j = rb * HT_TILE + lane;
        if (live && j < nd) {
            // plain multiplies and adds, ascending, the first product starting the chain; the blocks in order
            const double *cv = cw[wave];
            double lin;
            if (rb == 0) {
                lin = chain(kw0, [&](int kk) { const double a = tl.t[0][lane][kk]; return kk == lane ? 2 * a : a; }, [&](int kk) { return cv[kk]; });
                if (NT == 2 && nt == 2) {
                    const double p1 = chain(kw1, [&](int kk) { return tl.t[NT == 1 ? 0 : 1][lane][kk]; }, [&](int kk) { return cv[HT_TILE + kk]; });
                    lin = lin + p1;
                }
            } else {
                lin = chain(kw0, [&](int kk) { return tl.t[NT == 1 ? 0 : 1][kk][lane]; }, [&](int kk) { return cv[kk]; });
                const double p1 = chain(kw1, [&](int kk) { const double a = tl.t[NT == 1 ? 0 : 2][lane][kk]; return kk == lane ? 2 * a : a; },
                                        [&](int kk) { return cv[HT_TILE + kk]; });
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

// The quadratic-row unit of an expand kernel: one wave writes row j of a stage, its cnt = nd - j columns k >= j, to `dst`.  Term e takes
// word e of `sec` (the row's words in the slab's section; times *wt where the stage has a weight, NULL: as it is), the row's variable xv[0]
// and the column's xv[e] — xv the row's place in xvar (a stage's variables are contiguous in z).  The kernels differ in where sec, dst and
// the weight lie; each keeps its unit split u1 .. u4 and its decode of row u into (t, isu, nd, j): written once for the three, those
// change the kernels' register counts.
__device__ __forceinline__ void expand_quad_row(const double *__restrict__ sec, QT *__restrict__ dst, const double *__restrict__ wt, int cnt,
                                                const int64_t *__restrict__ xv, const int64_t *__restrict__ varmap, int lane) {
    typedef unsigned long long u64w;
    const double wv = wt ? *wt : 1.0;
    const u64w rowvar = (u64w)map_var(varmap, xv[0]);
    wave_write_words<3>(reinterpret_cast<u64w *>(dst), cnt, lane, [&](int q) -> u64w {
        const int e = q / 3, f = q - 3 * e;
        if (f == 1) return rowvar;
        if (f == 2) return (u64w)map_var(varmap, xv[e]);
        return (u64w)__double_as_longlong(wt ? wv * sec[e] : sec[e]);
    });
}

// the grid of an expand kernel over n variables and m constraint rows: a wave per unit — the n rows of quadratic terms, then 64 linear
// terms, 64 vector-affine terms, 64 constants each —, at most 4096 workgroups
inline dim3 expand_grid(int64_t n, int64_t m) {
    const int64_t units = n + cdiv(n, 64) + cdiv(m * n, 64) + cdiv(m, 64);
    return dim3((unsigned)std::min<int64_t>(cdiv(units, HT_WAVES), 4096));
}

// The units of an expand kernel behind its n rows of quadratic terms, one wave per unit u in [u1, u4): 64 linear terms each up to u2 (q at
// `sq`), 64 vector-affine terms each up to u3 (the row-major C at `scn`), then 64 constants each (the d-consts at `sd`).
__device__ __forceinline__ void expand_rest(int64_t u, int64_t u1, int64_t u2, int64_t u3, int64_t n, int64_t m, const double *__restrict__ sq,
                                            const double *__restrict__ scn, const double *__restrict__ sd, const int64_t *__restrict__ xvar,
                                            const int64_t *__restrict__ varmap, LT *__restrict__ ol, VAT *__restrict__ ov,
                                            double *__restrict__ ovc, int lane) {
    typedef unsigned long long u64w;
    const int64_t nvat = m * n;
    if (u < u2) {
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

// the dimension checks the objective files' entry points share (batch_horizon.hip has no terminal stage: term = 0); `who` words the message
inline int check_dims(const char *who, int64_t T, int64_t nx, int64_t nu, int64_t term, int64_t m) {
    const std::string w(who);
    PMT_REQUIRE(T >= 0 && nx >= 0 && nu >= 0 && m >= 0, PMT_DIMENSION_MISMATCH, w + ": negative dimension");
    PMT_REQUIRE(nx >= 1, PMT_DIMENSION_MISMATCH, w + ": nx < 1");
    PMT_REQUIRE(nx <= HT_MAX_DIM && nu <= HT_MAX_DIM, PMT_DIMENSION_MISMATCH, w + ": nx or nu above 128");
    PMT_REQUIRE(T >= 1 && T <= HT_MAX_T, PMT_DIMENSION_MISMATCH, w + ": T outside 1 .. 512");
    PMT_REQUIRE(term == 0 || term == 1, PMT_DIMENSION_MISMATCH, w + ": term must be 0 or 1");
    PMT_REQUIRE(m <= (INT64_C(1) << 40), PMT_DIMENSION_MISMATCH, w + ": m beyond 2^40");
    return PMT_OK;
}

}  // namespace pmt
