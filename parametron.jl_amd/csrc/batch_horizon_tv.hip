// The batch of horizons with TIME-VARYING stage weights (pmt_batch_horizon_tv_coeffs_f64): B independent instances, each
//     J_i = sum_{t<T} transpose(x_t (+|-) r_{i,t}) * Q_{i,t} * (x_t (+|-) r_{i,t}) + transpose(u_t (+|-) v_{i,t}) * R_{i,t} * (u_t (+|-) v_{i,t})
//           [+ transpose(x_T (+|-) r_{i,T}) * Q_{i,T} * (x_T (+|-) r_{i,T})]
// over z = [x_0; u_0; x_1; u_1; ..; (x_T)] subject to C_i*z (+|-) d_i — the fleet that re-linearises its cost at every stage and solve, the
// objective sibling of batch_horizon_ltv.hip.  One slab
//     [ S: ns blocks in z order, nd(nd+1)/2 words each | q: n | sconst: ns | const: 1 | C: m*n row-major | d-consts: m ]
// per instance.  In the reference a batch is many independent Models (src/model.jl:1-22); per instance and stage this replaces matvecmul!
// over the affine vector (src/functions.jl:800-822), vecdot! (:702-709 over :548-576), the add! of the stages (:244), canonicalize!
// (:381-386) and the MOI copies (src/moi_interop.jl:45-81), coefficients only — the words of quad_stages.hip on the instance's own table,
// stage s's Q pointer at its own matrix.
//
// A streaming problem: every matrix is read once and about half its bytes are written; nothing is shared between two stages.  So the work
// item is one STAGE, not one instance.  The x stages of the batch are contiguous in Q (item = i*(T + term) + t at item*nx*nx) and the u
// stages in R (item = i*T + t at item*nu*nu): the call is one launch over the x items, one over the u items, and a short third launch per
// instance — all ordered by the stream alone, no workgroup waits for another, no atomics, no workspace.  Items are dealt over persistent
// workgroups of 256 threads; (i, t) follows the item by adding (stride / per, stride % per) with one carry — the only divisions are 32-bit,
// once per thread; all instance and stage offsets are 64-bit.
//   nd <= 64   batch_horizon_tv_packed_kernel<W, LPT>, W = 8, 16, 32 or 64 the stage's lane width (nd <= W), LPT = 8, 16, 16, 16 loads a thread:
//              a stage lives in W*W / LPT = 8, 16, 64 or 256 threads, so 32, 16, 4 or 1 consecutive items make a pass of a workgroup and every
//              thread's loads cover its stage's W x W tile — a 4 x 4 stage takes 8 threads, a 12 x 12 one 16.  The whole matrix is one
//              tile: one load gives M[j,k] and M[k,j] (the diagonal tile of batch_form.hip).  tile[c][r] = M[r,c] in LDS at pitch W + 1,
//              s = M[r,c] + M[c,r] from the thread's own registers and the transposed LDS word, S back into the tile.  Then the NEXT
//              pass's loads are issued — in flight under this pass's stores and chains, in the registers just freed — the block leaves row by
//              row with k on the lanes (8-byte stores: a block starts at any 8-byte address), one thread per row runs the chain of
//              pmt_quad_form_shift_f64 (one 64-column block: the first product starts the chain) and the tree's levels W/2 .. 1 are
//              __shfl_down inside the W lanes; the levels above add +0.0 to a chain that started from +0.0, which changes no bit
//              (horizon_tile.h).  LDS 33792 .. 36864 bytes: four workgroups per CU; 20480 bytes and 80 registers at W = 8: six.
//   nd <= 128  batch_horizon_tv_wide_kernel: one item per workgroup pass, batch_form.hip's walk over the three upper tiles (0,0), (0,1), (1,1)
//              with the two blocks' chains in LDS, lin_j = P[0][j] + P[1][j], the tree's level 64 across the two halves and the rest in
//              wave 0; one loop over (item, tile), the next tile's loads issued before the current tile's chains and stores.  LDS 37376
//              bytes: four workgroups per CU.
//   tail       batch_horizon_tv_tail_kernel, a workgroup per instance, persistent: const = the instance's ns sconst words (written by the
//              two launches before it on the stream) in S_d's order — 256 chains onto 0.0, chain c taking the stages c, c + 256, .., then the
//              halving tree — and C_i, d as batch_horizon.hip writes them.  Without a constraint block (m == 0) const is all that is left:
//              batch_horizon_tv_const_kernel, a wave per instance, the same additions without LDS or barriers.
// Why two stage launches and not one: a launch over one kind of stage has one nd, so one packing, one LDS layout and one register budget;
// a workgroup that took x and u stages in turn would run both at the resources of the larger.
//
// pmt_batch_horizon_tv_expand_f64 is batch_horizon.hip's streaming writer: the S blocks lie in the slab in the order of the quadratic terms,
// so term e of out_quad takes word e of S.
#include <algorithm>

#include "horizon_tile.h"

namespace pmt {

namespace {

constexpr int TV_THREADS = 256;
constexpr int TV_WAVES = TV_THREADS / 64;
constexpr int TV_TILE = 64;
constexpr int TV_MAX_DIM = PMT_BATCH_HORIZON_MAX_DIM, TV_MAX_T = PMT_BATCH_HORIZON_MAX_T;
constexpr int TV_WG_PER_CU = 4;              // resident workgroups per CU (LDS: at most 37376 bytes each; 116 .. 124 vector registers)
constexpr int TV_WG_PER_CU_8 = 6;            // ... of the packed kernel of 8 lanes a stage (80 vector registers, 20480 bytes of LDS)
static_assert(TV_MAX_DIM <= 2 * TV_TILE, "the wide kernel walks two column blocks: three upper tiles");
static_assert(TV_TILE == HT_TILE && TV_THREADS == HT_THREADS, "expand_rest (horizon_tile.h) takes a wave per unit of this launch shape");

// The stages of one kind (x or u) of the whole batch: item = inst*per + t
struct TvStageArgs {
    const double *M;                         // [items][nd*nd] column-major, leading dimension nd
    const double *ref;                       // [items][nd]; with sign == 0 any readable address (word 0 is loaded and dropped)
    int64_t items;                           // B * per
    int per, nd, sign;                       // stages of this kind per instance: T + term (x) or T (u)
    int64_t blk0, blk_step;                  // the slab offset of stage t's S block: blk0 + t*blk_step
    int64_t q0, sc0;                         // ... of its q words: q0 + t*q_step; of its sconst word: sc0 + t*sc_step
    int q_step, sc_step;
    double *out; int64_t out_stride;
};

struct TvTailArgs {
    const double *C, *d;                     // C[B][m*n] column-major, d[B][m]
    int64_t B, m, sc_at;                     // sc_at: the slab offset of sconst; const, C and the d-consts follow its ns words
    int n, ns, sign_d;
    double *out; int64_t out_stride;
};

// The W x W tile of item `item` (clamped by the caller) into v, thread tl of the item's 256 / P taking (row tl % W, columns tl / W + CSTEP*i);
// every load unconditional on a clamped index.  rv: the reference word of row tl (threads past the last row load the last again).
template <int W, int CSTEP, int LPT>
__device__ __forceinline__ void tv_packed_load(const TvStageArgs &g, int64_t item, int tl, double (&v)[LPT], double &rv) {
    const int nd = g.nd;
    const double *__restrict__ M = g.M + item * nd * nd;
    // (the thread's coordinates are made opaque per pass: derived from loop invariants, the compiler otherwise keeps every address of the
    // unrolled body alive across the whole item loop)
    int r = tl % W, c0 = tl / W;
    asm volatile("" : "+v"(r), "+v"(c0));
    const unsigned rc = (unsigned)(r < nd ? r : nd - 1);
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
        const int c = c0 + CSTEP * i;
        v[i] = M[rc + (unsigned)(c < nd ? c : nd - 1) * (unsigned)nd];
    }
    rv = g.ref[g.sign ? item * nd + (tl < nd ? tl : nd - 1) : 0];
}

}  // namespace

// Stages of at most W rows, LPT loads per thread: TPS = W*W / LPT threads per stage, P = 256 / TPS consecutive items per pass of a workgroup.
template <int W, int LPT>
__global__ __launch_bounds__(TV_THREADS) void batch_horizon_tv_packed_kernel(TvStageArgs g) {
    constexpr int TPS = W * W / LPT, P = TV_THREADS / TPS, PITCH = W + 1, CSTEP = TPS / W;
    static_assert(LPT * TPS == W * W && CSTEP * LPT == W && TPS >= W && P * TPS == TV_THREADS, "LPT loads per thread cover the item's W x W tile");
    __shared__ double tile[P][W * PITCH];
    __shared__ double cvec[P][W];
    const int nd = g.nd, per = g.per, sign = g.sign;
    const int tid = threadIdx.x, sub = tid / TPS, tl = tid - sub * TPS;
    const unsigned G = gridDim.x, stride = G * P;
    const int step_inst = (int)(stride / (unsigned)per), step_t = (int)(stride % (unsigned)per);
    const int64_t last = g.items - 1;

    // the workgroup's passes: the items pass*P .. pass*P + P - 1, this thread's the one of its sub; a sub past the last item loads the last
    // item again and writes nothing
    HorizonItem p(blockIdx.x * P + sub, per);
    int64_t pass0 = (int64_t)blockIdx.x * P;              // the pass's first item: the same for the whole workgroup
    if (pass0 > last) return;
    double v[LPT], rv;
    tv_packed_load<W, CSTEP, LPT>(g, p.item < last ? p.item : last, tl, v, rv);
    for (;;) {
        const bool live = p.item <= last;
        double *__restrict__ tl_ = tile[sub];
        landed(v);
        {
            int r = tl % W, c0 = tl / W;
            asm volatile("" : "+v"(r), "+v"(c0));
            // out-of-range entries are 0.0;  tile[c][r] = M[r,c]
#pragma unroll
            for (int i = 0; i < LPT; ++i) {
                const int c = c0 + CSTEP * i;
                v[i] = (r < nd && c < nd) ? v[i] : 0.0;
                tl_[c * PITCH + r] = v[i];
            }
            asm volatile("" : "+v"(rv));                  // (looked at here, not in front of the loads)
            if (tl < W) cvec[sub][tl] = signed_const(rv, sign);
            __syncthreads();
            // s(r, c) = M[r,c] + M[c,r]; the diagonal keeps M[j,j] (doubled where it is used)
            double s[LPT];
#pragma unroll
            for (int i = 0; i < LPT; ++i) {
                const int c = c0 + CSTEP * i;
                const double a = tl_[r * PITCH + c];
                s[i] = (c == r) ? v[i] : v[i] + a;
            }
            __syncthreads();
            // tile[c][r] = S[r,c] (= S[c,r], bit for bit: the sum of two numbers)
#pragma unroll
            for (int i = 0; i < LPT; ++i) tl_[(c0 + CSTEP * i) * PITCH + r] = s[i];
            __syncthreads();
        }
        // the next pass: its loads are in flight under this pass's stores and chains (past the last pass: the last item again, dropped)
        HorizonItem q = p;
        q.step(stride, step_inst, step_t, per);
        const bool more = pass0 + stride <= last;
        tv_packed_load<W, CSTEP, LPT>(g, q.item < last ? q.item : last, tl, v, rv);

        double *__restrict__ out = g.out + p.inst * g.out_stride;
        if (live) {
            // the block: row j holds its columns k >= j, k on the lanes, CSTEP rows at a time
            double *__restrict__ osec = out + g.blk0 + p.s * g.blk_step;
            const int k = tl % W, jr = tl / W;
            for (int j0 = 0; j0 < nd; j0 += CSTEP) {
                const int j = j0 + jr;
                if (j < nd && k < nd && k >= j) {
                    const double a = tl_[j * PITCH + k];
                    osec[tri_pos(nd, j, k)] = (k == j) ? 2 * a : a;
                }
            }
        }
        // one thread per row: lin_j, plain multiplies and adds, ascending, the first product starting the chain; then chain j of the
        // stage's tree, 0.0 + c_j*lin_j (a row past nd, a plain stage: 0.0), the levels W/2 .. 1 inside the W lanes
        double prod = 0.0;
        if (live && tl < nd) {
            double lin = 0.0;
            if (sign) {
                const double *cs = cvec[sub];
                lin = chain(nd, [&](int kk) { const double a = tl_[tl * PITCH + kk]; return kk == tl ? 2 * a : a; }, [&](int kk) { return cs[kk]; });
                prod = cs[tl] * lin;
            }
            out[g.q0 + (int64_t)p.s * g.q_step + tl] = lin;
        }
        double t = 0.0 + prod;
        for (int h = W >> 1; h > 0; h >>= 1) t = t + __shfl_down(t, h, W);
        if (live && tl == 0) out[g.sc0 + (int64_t)p.s * g.sc_step] = 0.5 * t;
        __syncthreads();                                  // the next pass reuses the LDS
        if (!more) break;
        p = q; pass0 += stride;
    }
}

// The upper tile ti = 0, 1, 2 -> (bj, bk) = (0,0), (0,1), (1,1) of a wide stage's matrix Q into registers: lower[i] = Q[k0 + lane, j0 + wave + 4 i]
// (k on the lanes) and, off the diagonal, upper[i] = Q[j0 + lane, k0 + wave + 4 i] (j on the lanes); no load depends on the lane, every index
// is clamped
__device__ __forceinline__ void tv_wide_load(const double *__restrict__ Q, int n, int ti, int tid, double (&lower)[16], double (&upper)[16]) {
    // (the lane's coordinates are made opaque per tile, as in batch_form.hip)
    int lane = tid & 63, wave = tid >> 6;
    asm volatile("" : "+v"(lane), "+v"(wave));
    const int j0 = (ti >> 1) * TV_TILE, k0 = ((ti + 1) >> 1) * TV_TILE;
    const int rk = k0 + lane, rj = j0 + lane;
    const unsigned ork = (unsigned)(rk < n ? rk : n - 1), orj = (unsigned)(rj < n ? rj : n - 1);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = j0 + wave + 4 * i;
        lower[i] = Q[ork + (unsigned)(c < n ? c : n - 1) * (unsigned)n];
    }
    if (ti == 1) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = k0 + wave + 4 * i;
            upper[i] = Q[orj + (unsigned)(c < n ? c : n - 1) * (unsigned)n];
        }
    }
}

// Stages of 65 .. 128 rows, one per pass of a workgroup: batch_form.hip's walk of the upper tiles, the chains of the two column blocks in LDS.
// One loop over (item, tile): the next tile's loads — the next item's first tile behind an item's last — are issued as soon as the current
// tile's S sits in LDS, in the registers that has freed, and are in flight under its chains and stores.
__global__ __launch_bounds__(TV_THREADS) void batch_horizon_tv_wide_kernel(TvStageArgs g) {
    __shared__ double tile[TV_TILE][TV_TILE + 1];
    __shared__ double part[2][TV_MAX_DIM];                // P[B][j]
    __shared__ double cvec[TV_MAX_DIM];
    __shared__ double pr[TV_MAX_DIM];
    const int n = g.nd, per = g.per;
    const int tid = threadIdx.x;
    const bool shift = g.sign != 0;
    const unsigned G = gridDim.x;
    const int step_inst = (int)(G / (unsigned)per), step_t = (int)(G % (unsigned)per);

    HorizonItem p(blockIdx.x, per);
    if (p.item >= g.items) return;
    int ti = 0;
    double lower[16], upper[16];
    tv_wide_load(g.M + p.item * n * n, n, ti, tid, lower, upper);
    // the reference is asked for with the item's first tile (every thread loads, thread t >= n the last entry again)
    double pv = g.ref[shift ? p.item * n + (tid < n ? tid : n - 1) : 0];
    for (;;) {
        const int bj = ti >> 1, bk = (ti + 1) >> 1;
        const bool diagonal = bk == bj;
        const int j0 = bj * TV_TILE, k0 = bk * TV_TILE;
        double *__restrict__ out = g.out + p.inst * g.out_stride;
        {
            int lane = tid & 63, wave = tid >> 6;
            asm volatile("" : "+v"(lane), "+v"(wave));
            const int rk = k0 + lane, rj = j0 + lane;
            if (!diagonal) {
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
            if (ti == 0 && shift) {                     // c = 0.0 (+|-) ref; read by the chains, behind this tile's barriers
                asm volatile("" : "+v"(pv));
                if (tid < n) cvec[tid] = signed_const(pv, g.sign);
            }
            // tile[kk][jj] = Q[j0 + jj, k0 + kk]
#pragma unroll
            for (int i = 0; i < 16; ++i) tile[wave + 4 * i][lane] = upper[i];
            __syncthreads();
            // s(jj = wave + 4 i, kk = lane) = Q[j,k] + Q[k,j]; the diagonal keeps Q[j,j] (doubled where it is used)
            double s[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int jj = wave + 4 * i;
                const double a = tile[lane][jj];
                s[i] = (diagonal && jj == lane) ? a : a + lower[i];
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 16; ++i) tile[wave + 4 * i][lane] = s[i];
            __syncthreads();
        }
        // the next tile: its loads are in flight under this tile's chains and stores (past the last tile: this tile again, dropped)
        HorizonItem q = p;
        int qi = ti + 1;
        if (qi == 3) { qi = 0; q.step(G, step_inst, step_t, per); }
        const bool more = q.item < g.items;
        if (!more) { q = p; qi = ti; }
        tv_wide_load(g.M + q.item * n * n, n, qi, tid, lower, upper);
        if (qi == 0) pv = g.ref[shift ? q.item * n + (tid < n ? tid : n - 1) : 0];
        {
            int lane = tid & 63, wave = tid >> 6;
            asm volatile("" : "+v"(lane), "+v"(wave));
            const int kw = n - k0 < TV_TILE ? n - k0 : TV_TILE, jw = n - j0 < TV_TILE ? n - j0 : TV_TILE;
            if (shift) {
                // plain multiplies and adds, ascending, the first product starting the chain
                if (wave == 0 && lane < jw) {
                    part[bk][j0 + lane] = chain(kw, [&](int kk) { const double a = tile[lane][kk]; return (diagonal && kk == lane) ? 2 * a : a; },
                                                   [&](int kk) { return cvec[k0 + kk]; });
                } else if (wave == 1 && !diagonal && lane < kw) {
                    part[bj][k0 + lane] = chain(jw, [&](int jj) { return tile[jj][lane]; }, [&](int jj) { return cvec[j0 + jj]; });
                }
            }
            // the block: row j holds its columns k >= j; this tile's piece of it, k on the lanes
            double *__restrict__ osec = out + g.blk0 + p.s * g.blk_step;
#pragma unroll 4
            for (int r = 0; r < 16; ++r) {
                const int jj = wave * 16 + r, j = j0 + jj;
                const int k = k0 + lane;
                if (j < n && k < n && k >= j) {
                    const double a = tile[jj][lane];
                    osec[tri_pos(n, j, k)] = (k == j) ? 2 * a : a;
                }
            }
        }
        __syncthreads();
        if (ti == 2) {
            // lin_j = P[0][j] + P[1][j]; chain j of the tree: 0.0 + c_j*lin_j (a row past n, a plain stage: 0.0); the levels 256 and 128 add
            // +0.0 to such a chain, which changes no bit: level 64 across the halves, then inside wave 0
            if (tid < TV_MAX_DIM) {
                double prod = 0.0;
                if (tid < n) {
                    double lin = 0.0;
                    if (shift) {
                        lin = part[0][tid] + part[1][tid];
                        prod = cvec[tid] * lin;
                    }
                    out[g.q0 + (int64_t)p.s * g.q_step + tid] = lin;
                }
                pr[tid] = 0.0 + prod;
            }
            __syncthreads();
            if (tid < 64) {
                double t = pr[tid] + pr[tid + 64];
                for (int h = 32; h > 0; h >>= 1) t = t + __shfl_down(t, h);
                if (tid == 0) out[g.sc0 + (int64_t)p.s * g.sc_step] = 0.5 * t;
            }
            // (no barrier here: part and cvec were last read in front of the barrier above, and the next item writes pr only behind its
            // tiles' barriers)
        }
        if (!more) break;
        p = q; ti = qi;
    }
}

// Per instance: const from the instance's stage constants, C_i transposed through the tile, the d-consts (batch_horizon.hip's tail)
__global__ __launch_bounds__(TV_THREADS) void batch_horizon_tv_tail_kernel(TvTailArgs g) {
    __shared__ double tile[TV_TILE][TV_TILE + 1];
    __shared__ double red[TV_THREADS];
    const int n = g.n, ns = g.ns;
    const int64_t m = g.m;
    const int tid = threadIdx.x;
    for (int64_t inst = blockIdx.x; inst < g.B; inst += gridDim.x) {
        double *__restrict__ osc = g.out + inst * g.out_stride + g.sc_at;
        double dv = 0.0;
        if (g.sign_d && m > 0) dv = g.d[inst * m + (tid < m ? tid : m - 1)];
        // the stage constants in z order, added in S_d's order: 256 chains onto 0.0, then the halving tree
        // (batch_horizon.hip and batch_horizon_terms.hip hold this sum too: moved into a shared function it compiles to other device code)
        {
            double s = 0.0;
            for (int t = tid; t < ns; t += TV_THREADS) s = s + osc[t];
            red[tid] = s;
            __syncthreads();
            for (int h = TV_THREADS / 2; h > 0; h >>= 1) {
                if (tid < h) red[tid] = red[tid] + red[tid + h];
                __syncthreads();
            }
            if (tid == 0) osc[ns] = red[0];
        }
        // the constraint block: C_i column-major -> row-major through the tile (rows on the lanes in, columns on the lanes out)
        // (batch_horizon.hip and batch_horizon_terms.hip hold this block too: moved into a shared function it compiles to other device code)
        if (m > 0) {
            const double *__restrict__ Ci = g.C + inst * m * n;
            double *__restrict__ oc = osc + ns + 1;
            for (int64_t r0 = 0; r0 < m; r0 += TV_TILE) {
                for (int c0 = 0; c0 < n; c0 += TV_TILE) {
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
            for (int64_t r = tid + TV_THREADS; r < m; r += TV_THREADS) od[r] = g.sign_d ? signed_const(g.d[inst * m + r], g.sign_d) : 0.0;
        }
        __syncthreads();                                  // the next instance reuses red and the tile
    }
}

// m == 0: const alone — a wave per instance, four to a workgroup, without LDS.  Lane l holds the chains l, l + 64, l + 128 and l + 192 of
// the 256; the tree's level 128 adds chain c + 128 to chain c, level 64 the two sums of a lane, the levels 32 .. 1 run in the wave: the
// additions of the tail kernel's tree, in its order.
__global__ __launch_bounds__(TV_THREADS) void batch_horizon_tv_const_kernel(TvTailArgs g) {
    const int lane = threadIdx.x & 63, ns = g.ns;
    const int64_t wv = (int64_t)blockIdx.x * TV_WAVES + (threadIdx.x >> 6), nwv = (int64_t)gridDim.x * TV_WAVES;
    for (int64_t inst = wv; inst < g.B; inst += nwv) {
        double *__restrict__ osc = g.out + inst * g.out_stride + g.sc_at;
        double c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double s = 0.0;
            for (int t = lane + 64 * k; t < ns; t += TV_THREADS) s = s + osc[t];
            c[k] = s;
        }
        const double lo = c[0] + c[2], hi = c[1] + c[3];
        double t = lo + hi;
        for (int h = 32; h > 0; h >>= 1) t = t + __shfl_down(t, h);
        if (lane == 0) osc[ns] = t;
    }
}

// One instance's MOI buffers from its slab.  A wave per unit, the units dealt out over the grid's waves: the n rows of quadratic terms
// (row j of a stage: its columns k >= j — term e of out_quad takes word e of S), then 64 linear terms each, 64 vector-affine terms each,
// 64 constants each.
__global__ __launch_bounds__(TV_THREADS) void batch_horizon_tv_expand_kernel(const double *__restrict__ slab, int T, int nx, int nu, int term, int64_t m,
                                                                              const int64_t *__restrict__ xvar, const int64_t *__restrict__ varmap,
                                                                              QT *__restrict__ oq, LT *__restrict__ ol, double *__restrict__ oc,
                                                                              VAT *__restrict__ ov, double *__restrict__ ovc) {
    const int lane = threadIdx.x & 63;
    const int64_t wv = (int64_t)blockIdx.x * TV_WAVES + (threadIdx.x >> 6), nwv = (int64_t)gridDim.x * TV_WAVES;
    const int w = nx + nu, ns = T * (nu ? 2 : 1) + term;
    const int64_t n = (int64_t)T * w + (int64_t)term * nx, nqx = (int64_t)nx * (nx + 1) / 2, nqu = (int64_t)nu * (nu + 1) / 2;
    const int64_t nS = T * (nqx + nqu) + term * nqx;
    const double *__restrict__ sq = slab + nS, *__restrict__ scn = sq + n + ns + 1, *__restrict__ sd = scn + m * n;
    const int64_t nvat = m * n;
    const int64_t u1 = n, u2 = u1 + (n + 63) / 64, u3 = u2 + (nvat + 63) / 64, u4 = u3 + (m + 63) / 64;
    for (int64_t u = wv; u < u4; u += nwv) {
        if (u < u1) {
            const int t = (int)(u / w), wi = (int)(u - (int64_t)t * w);          // (the terminal stage: t == T, wi < nx)
            const bool isu = wi >= nx;
            const int nd = isu ? nu : nx, j = isu ? wi - nx : wi;
            const int64_t zb = u - j;                                            // the stage's first variable in z
            const int64_t at = (int64_t)t * (nqx + nqu) + (isu ? nqx : 0) + tri_pos(nd, j, j);
            expand_quad_row(slab + at, oq + at, nullptr, nd - j, xvar + zb + j, varmap, lane);
        } else {
            expand_rest(u, u1, u2, u3, n, m, sq, scn, sd, xvar, varmap, ol, ov, ovc, lane);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *oc = sq[n + ns];
}

// a launch of the packed kernel: P items per pass of a workgroup
template <int W, int LPT>
static void tv_launch_packed(const TvStageArgs &a, hipStream_t s) {
    constexpr int P = TV_THREADS / (W * W / LPT), PER_CU = W == 8 ? TV_WG_PER_CU_8 : TV_WG_PER_CU;
    const dim3 grid((unsigned)std::min<int64_t>(cdiv(a.items, P), (int64_t)PER_CU * cu_count()));
    PMT_LAUNCH_NAMED("batch_horizon_tv_packed_kernel", (batch_horizon_tv_packed_kernel<W, LPT>), grid, dim3(TV_THREADS), 0, s, a);
}

static void tv_launch_stages(const TvStageArgs &a, hipStream_t s) {
    if (a.nd > TV_TILE) {
        PMT_LAUNCH(batch_horizon_tv_wide_kernel, dim3((unsigned)std::min<int64_t>(a.items, (int64_t)TV_WG_PER_CU * cu_count())), dim3(TV_THREADS), 0, s, a);
    } else if (a.nd > 32) {
        tv_launch_packed<64, 16>(a, s);
    } else if (a.nd > 16) {
        tv_launch_packed<32, 16>(a, s);
    } else if (a.nd > 8) {
        tv_launch_packed<16, 16>(a, s);
    } else {
        tv_launch_packed<8, 8>(a, s);
    }
}

}  // namespace pmt

using namespace pmt;

extern "C" int64_t pmt_batch_horizon_tv_slab_doubles(int64_t T, int64_t nx, int64_t nu, int64_t term, int64_t m) {
    const int64_t n = T * (nx + nu) + term * nx, ns = T * (nu > 0 ? 2 : 1) + term;
    return T * (nx * (nx + 1) / 2 + nu * (nu + 1) / 2) + term * (nx * (nx + 1) / 2) + n + ns + 1 + m * n + m;
}

extern "C" int pmt_batch_horizon_tv_coeffs_f64(const double *Q, const double *R, const double *r, const double *v, const double *Cm, const double *d,
                                               int64_t B, int64_t T, int64_t nx, int64_t nu, int64_t term, int64_t m, int sign_r, int sign_v,
                                               int sign_d, double *out, int64_t out_stride, void *stream) {
    PMT_REQUIRE(B >= 0, PMT_DIMENSION_MISMATCH, "batch_horizon_tv: negative dimension");
    const int rc = check_dims("batch_horizon_tv", T, nx, nu, term, m);
    if (rc != PMT_OK) return rc;
    const int64_t L = pmt_batch_horizon_tv_slab_doubles(T, nx, nu, term, m);
    PMT_REQUIRE(out_stride >= L, PMT_DIMENSION_MISMATCH, "batch_horizon_tv: out_stride smaller than the slab");
    PMT_REQUIRE(sign_r >= -1 && sign_r <= 1 && sign_v >= -1 && sign_v <= 1 && sign_d >= -1 && sign_d <= 1, PMT_INVALID_ARGUMENT,
                "batch_horizon_tv: signs must be -1, 0 or +1");
    if (B == 0) return PMT_OK;
    PMT_REQUIRE(out && Q && (nu == 0 || R) && (sign_r == 0 || r) && (nu == 0 || sign_v == 0 || v) && (m == 0 || (Cm && d)), PMT_INVALID_ARGUMENT,
                "batch_horizon_tv: null pointer");
    const int64_t nqx = nx * (nx + 1) / 2, nqu = nu * (nu + 1) / 2, w = nx + nu;
    const int64_t n = T * w + term * nx, ns = T * (nu > 0 ? 2 : 1) + term, nS = T * (nqx + nqu) + term * nqx;
    TvStageArgs x, u;
    x.M = Q; x.ref = sign_r ? r : Q; x.items = B * (T + term); x.per = (int)(T + term); x.nd = (int)nx; x.sign = sign_r;
    x.blk0 = 0; x.blk_step = nqx + nqu; x.q0 = nS; x.q_step = (int)w; x.sc0 = nS + n; x.sc_step = nu > 0 ? 2 : 1;
    x.out = out; x.out_stride = out_stride;
    u = x;
    u.M = R; u.ref = sign_v ? v : R; u.items = B * T; u.per = (int)T; u.nd = (int)nu; u.sign = sign_v;
    u.blk0 = nqx; u.q0 = nS + nx; u.sc0 = nS + n + 1;
    TvTailArgs tl;
    tl.C = Cm; tl.d = d; tl.B = B; tl.m = m; tl.sc_at = nS + n; tl.n = (int)n; tl.ns = (int)ns; tl.sign_d = sign_d;
    tl.out = out; tl.out_stride = out_stride;
    const bool has_u = nu > 0;
    return dispatch(stream, [=](hipStream_t s) {
        tv_launch_stages(x, s);
        int e = check_launch("batch_horizon_tv stages x");
        if (e != PMT_OK) return e;
        if (has_u) {
            tv_launch_stages(u, s);
            e = check_launch("batch_horizon_tv stages u");
            if (e != PMT_OK) return e;
        }
        if (tl.m == 0) {
            PMT_LAUNCH(batch_horizon_tv_const_kernel, dim3((unsigned)std::min<int64_t>(cdiv(B, TV_WAVES), (int64_t)8 * cu_count())), dim3(TV_THREADS), 0, s, tl);
            return check_launch("batch_horizon_tv_const_kernel");
        }
        PMT_LAUNCH(batch_horizon_tv_tail_kernel, dim3((unsigned)std::min<int64_t>(B, (int64_t)TV_WG_PER_CU * cu_count())), dim3(TV_THREADS), 0, s, tl);
        return check_launch("batch_horizon_tv_tail_kernel");
    });
}

extern "C" int pmt_batch_horizon_tv_expand_f64(const double *slab, int64_t T, int64_t nx, int64_t nu, int64_t term, int64_t m, const int64_t *xvar,
                                               const int64_t *varmap, pmt_quadratic_term *out_quad, pmt_linear_term *out_lin, double *out_const,
                                               pmt_vector_affine_term *out_vat, double *out_vconsts, void *stream) {
    const int rc = check_dims("batch_horizon_tv_expand", T, nx, nu, term, m);
    if (rc != PMT_OK) return rc;
    PMT_REQUIRE(slab && xvar && varmap && out_quad && out_lin && out_const && (m == 0 || (out_vat && out_vconsts)), PMT_INVALID_ARGUMENT,
                "batch_horizon_tv_expand: null pointer");
    const int iT = (int)T, inx = (int)nx, inu = (int)nu, iterm = (int)term;
    return dispatch(stream, [=](hipStream_t s) {
        PMT_LAUNCH(batch_horizon_tv_expand_kernel, expand_grid((int64_t)iT * (inx + inu) + (int64_t)iterm * inx, m), dim3(TV_THREADS), 0, s, slab, iT, inx,
                   inu, iterm, m, xvar, varmap, out_quad, out_lin, out_const, out_vat, out_vconsts);
        return check_launch("batch_horizon_tv_expand_kernel");
    });
}
