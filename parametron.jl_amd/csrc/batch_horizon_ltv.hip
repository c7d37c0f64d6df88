// The batch of horizons' TIME-VARYING dynamics rows as a compact section per instance (pmt_batch_horizon_dynamics_tv_f64): instance i's
// constraints
//     x_0 (+|-) h_{i,0},    (+|-)x_t (+|-) A_{i,t}*x_{t-1} (+|-) B_{i,t}*u_{t-1} (+|-) h_{i,t},  t = 1 .. T-1
// over z = [x_0; u_0; x_1; u_1; ..] — the fleet that re-linearises every stage at every solve.  The section
//     [ AB_1 | AB_2 | .. | AB_{T-1} | h-consts: T*nx ],   AB_t: nx*(nx + nu) row-major
// holds, block by block, the words batch_horizon_dyn.hip's AB holds for the pair (A_{i,t}, B_{i,t}).  In the reference a batch is many
// independent Models (src/model.jl:1-22); per instance and record this replaces matvecmul! (src/functions.jl:775-798), vecadd! /
// vecsubtract! (:751-764) and the MOI copy (src/moi_interop.jl:64-81) — the records of affine_stages.hip on the instance's own tables, stage
// t's matrix parts pointing at A_{i,t}, B_{i,t}.  Nothing is computed: copies, sign-bit flips and 0.0 (+|-) h, bound by loads and stores.
//
// The work item is one matrix pair (i, t), item = i*(T-1) + (t-1), not one instance: 64 instances of 100 stages fill the chip as 8192 of 8
// do.  Consecutive items are contiguous in A and Bm (offset item*nx*nx, item*nx*nu); the block goes to out + i*out_stride + (t-1)*nab.
// Persistent workgroups of 256 threads deal the items out, workgroup g taking g, g + G, ..; (i, t-1) follows the item by adding
// (G / (T-1), G % (T-1)) with one carry — the only divisions are 32-bit, once per workgroup.  No workgroup waits for another, no atomics,
// no workspace; all instance and stage offsets are 64-bit.
// h-consts: item (i, t-1) writes the nx constants of stage t, and the item of t = 1 those of stage 0 with them (2*nx contiguous words, one
// thread each) — every item carries the same few words, nothing serialises behind one item, and the load rides with the item's first
// tile.  T == 1 has no item: its section is the constants alone (batch_horizon_ltv_consts_kernel, 256 / nx instances per workgroup pass).
// Tiles are batch_horizon_dyn.hip's (the loads: dynamics_tile.h): 4096 words read along the columns (64 x 64, 32 x 128 up to 32 rows, 16 x 256 up to 16), every load
// unconditional on a clamped index and issued before the first value is looked at (landed), lane coordinates opaque per tile, transposed
// through an LDS tile of pitch columns + 1, rows leaving with the column on the lanes as 8-byte stores.  New here: an item is a few tiles
// at most (one at (32, 16)), so the walk over (item, row tile, column tile) is ONE loop and the next tile's loads are issued as soon as the
// current tile sits in LDS — they are in flight under its stores and the barrier, in the registers the LDS write has just freed.  And
// where 2048 words hold a whole row of the tile's rows (w <= 64 at 32 rows, <= 128 at 16) the tile is that half: at (32, 16) ten of the
// sixteen loads of a thread would fall on clamped columns, and with 16.5 KB of LDS eight workgroups are resident per CU instead of four —
// what a launch bound by the bytes it has in flight needs.
// Pairs of at most 512 AB words take a wave each, four to a workgroup, without LDS (batch_horizon_ltv_small_kernel).
//
// pmt_batch_horizon_dynamics_tv_expand_f64 is the streaming writer both dynamics files share (dynamics_expand<true>, dynamics_tile.h) with
// the row source at AB_t: each section word is read once.
#include "dynamics_tile.h"
#include "horizon_tile.h"

namespace pmt {

namespace {

constexpr int LT_LOADS = 16, LT_LOADS_HALF = 8;                // loads per thread of a tile: 4096 words, or 2048 where they hold a whole row
constexpr int LT_WG_PER_CU = 4, LT_WG_PER_CU_HALF = 8;         // resident workgroups per CU of the tile kernel (LDS: at most 33280 / 16640 bytes each)
static_assert(2 * 22 <= 64 && 23 * 23 > DY_SMALL_WORDS, "a wave's item has nx <= 22: one lane per constant of its two stages");

struct BatchLtvArgs {
    const u64 *A, *Bm;                       // instance-, then stage-major: A[B][T-1][nx*nx], Bm[B][T-1][nx*nu] column-major, leading dimension nx
    const double *h;                         // h[B][T*nx] stage-major; with sign_h == 0 any readable address (word 0 is loaded and dropped)
    int64_t items;                           // B * (T - 1)
    int T, nx, nu, sign_h;
    u64 flip_a, flip_b;                      // the sign bit where the sign is -1
    double *out; int64_t out_stride;
};

// the constants an item writes: the stage s + 1, and stage 0 with it where s == 0 — `cnt` contiguous words from `first`
__device__ __forceinline__ void ltv_const_range(int s, int nx, int &first, int &cnt) {
    first = s ? (s + 1) * nx : 0;
    cnt = s ? nx : 2 * nx;
}

// thread k's constant of the item, on a clamped index (the load is unconditional; sign_h == 0 reads word 0 of g.h and drops it)
__device__ __forceinline__ double ltv_const_load(const BatchLtvArgs &g, const HorizonItem &p, int k) {
    int first, cnt;
    ltv_const_range(p.s, g.nx, first, cnt);
    const int64_t at = p.inst * g.T * g.nx + first + (k < cnt ? k : cnt - 1);
    return g.h[g.sign_h ? at : 0];
}

__device__ __forceinline__ void ltv_const_store(const BatchLtvArgs &g, const HorizonItem &p, int k, double hv) {
    int first, cnt;
    ltv_const_range(p.s, g.nx, first, cnt);
    if (k < cnt) g.out[p.inst * g.out_stride + (int64_t)(g.T - 1) * g.nx * (g.nx + g.nu) + first + k] = signed_const(hv, g.sign_h);
}

// the tile (r0, c0) of item p's [A | B] into v (dynamics_tile.h), and the thread's constant of the item with it
template <int RL, int LPT>
__device__ __forceinline__ void ltv_tile_load(const BatchLtvArgs &g, const HorizonItem &p, int r0, int c0, int tid, u64 (&v)[LPT], double &hv) {
    const int nx = g.nx, nu = g.nu;
    const u64 *__restrict__ Ai = g.A + p.item * nx * nx;
    const u64 *__restrict__ Bi = nu ? g.Bm + p.item * nx * nu : Ai;              // (nu == 0: no column selects it)
    int lr, lc;
    dynamics_tile_load<RL, LPT>(Ai, Bi, nx, nx + nu, r0, c0, tid, v, lr, lc);
    hv = ltv_const_load(g, p, tid);
}

}  // namespace

// RL rows x CW = 256 * LPT / RL columns a tile.  One loop over the workgroup's tiles: (item, r0, c0), the column tile running fastest.
template <int RL, int LPT>
__global__ __launch_bounds__(DY_THREADS) void batch_horizon_ltv_kernel(BatchLtvArgs g) {
    constexpr int CW = DY_THREADS * LPT / RL, PITCH = CW + 1, CSTEP = DY_THREADS / RL;
    __shared__ u64 tile[RL * PITCH];
    const int nx = g.nx, w = nx + g.nu, per = g.T - 1;
    const int64_t nab = (int64_t)nx * w;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned G = gridDim.x;
    const int step_inst = (int)(G / (unsigned)per), step_s = (int)(G % (unsigned)per);
    const u64 flip_a = g.flip_a, flip_b = g.flip_b;

    HorizonItem p(blockIdx.x, per);
    if (p.item >= g.items) return;
    int r0 = 0, c0 = 0;
    u64 v[LPT];
    double hv;
    ltv_tile_load<RL, LPT>(g, p, r0, c0, tid, v, hv);
    for (;;) {
        landed(v);
        // tile[row][column], each word with its part's sign; the item's constants leave with its first tile
        // (batch_horizon_dyn.hip holds this store too: moved into a shared function it compiles to other device code)
        {
            int lr = tid % RL, lc = tid / RL;
            asm volatile("" : "+v"(lr), "+v"(lc));
#pragma unroll
            for (int i = 0; i < LPT; ++i) tile[lr * PITCH + lc + CSTEP * i] = v[i] ^ (c0 + lc + CSTEP * i < nx ? flip_a : flip_b);
        }
        if (r0 == 0 && c0 == 0) ltv_const_store(g, p, tid, hv);
        __syncthreads();
        // the next tile: its loads are in flight under this tile's stores (past the last tile: this tile again, dropped)
        HorizonItem q = p;
        int qr = r0, qc = c0 + CW;
        if (qc >= w) {
            qc = 0; qr += RL;
            if (qr >= nx) { qr = 0; q.step(G, step_inst, step_s, per); }
        }
        const bool more = q.item < g.items;
        if (!more) { q = p; qr = r0; qc = c0; }
        ltv_tile_load<RL, LPT>(g, q, qr, qc, tid, v, hv);
        // a wave per row, the column on the lanes
        // (batch_horizon_dyn.hip holds this write-out too: moved into a shared function it compiles to other device code)
        {
            u64 *__restrict__ ob = reinterpret_cast<u64 *>(g.out) + p.inst * g.out_stride + p.s * nab;
            const int nr = nx - r0 < RL ? nx - r0 : RL, nc = w - c0 < CW ? w - c0 : CW;
            for (int rr = wave; rr < nr; rr += DY_WAVES) {
                u64 *__restrict__ orow = ob + (int64_t)(r0 + rr) * w + c0;
                for (int c = lane; c < nc; c += 64) orow[c] = tile[rr * PITCH + c];
            }
        }
        __syncthreads();                                  // the next tile reuses the LDS
        if (!more) break;
        p = q; r0 = qr; c0 = qc;
    }
}

// A wave per matrix pair of at most DY_SMALL_WORDS AB words: lane l writes the words l, l + 64, .. of AB_t in output order
__global__ __launch_bounds__(DY_THREADS) void batch_horizon_ltv_small_kernel(BatchLtvArgs g) {
    const int nx = g.nx, nu = g.nu, w = nx + nu, nab = nx * w, per = g.T - 1;
    const int lane = threadIdx.x & 63;
    const unsigned wv = blockIdx.x * DY_WAVES + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), nwv = gridDim.x * DY_WAVES;
    const int step_inst = (int)(nwv / (unsigned)per), step_s = (int)(nwv % (unsigned)per);
    const u64 flip_a = g.flip_a, flip_b = g.flip_b;
    unsigned src[DY_SMALL_LOADS];
    bool from_a[DY_SMALL_LOADS];
#pragma unroll
    for (int k = 0; k < DY_SMALL_LOADS; ++k) src[k] = dynamics_small_source(lane + 64 * k, nx, w, nab, from_a[k]);
    for (HorizonItem p(wv, per); p.item < g.items; p.step(nwv, step_inst, step_s, per)) {
        const u64 *__restrict__ Ai = g.A + p.item * nx * nx;
        const u64 *__restrict__ Bi = nu ? g.Bm + p.item * nx * nu : Ai;          // (nu == 0: no word selects it)
        u64 *__restrict__ out = reinterpret_cast<u64 *>(g.out) + p.inst * g.out_stride + (int64_t)p.s * nab;
        // (batch_horizon_dyn.hip holds the load and the flip / store loop too: moved into shared functions they compile to other device code)
        u64 v[DY_SMALL_LOADS];
#pragma unroll
        for (int k = 0; k < DY_SMALL_LOADS; ++k) v[k] = (from_a[k] ? Ai : Bi)[src[k]];
        const double hv = ltv_const_load(g, p, lane);
        landed(v);
#pragma unroll
        for (int k = 0; k < DY_SMALL_LOADS; ++k) {
            const int e = lane + 64 * k;
            if (e < nab) out[e] = v[k] ^ (from_a[k] ? flip_a : flip_b);
        }
        ltv_const_store(g, p, lane, hv);
    }
}

// T == 1: the section is the nx constants of stage 0.  256 / nx instances per pass of a workgroup, a thread per word.
__global__ __launch_bounds__(DY_THREADS) void batch_horizon_ltv_consts_kernel(const double *__restrict__ h, int64_t B, int nx, int sign_h,
                                                                               double *__restrict__ out, int64_t out_stride) {
    const int each = DY_THREADS / nx, sub = (int)threadIdx.x / nx, r = (int)threadIdx.x - sub * nx;
    if (sub >= each) return;
    for (int64_t i = (int64_t)blockIdx.x * each + sub; i < B; i += (int64_t)gridDim.x * each)
        out[i * out_stride + r] = sign_h ? signed_const(h[i * nx + r], sign_h) : 0.0;
}

__global__ __launch_bounds__(DY_THREADS) void batch_horizon_ltv_expand_kernel(const double *__restrict__ section, int T, int nx, int nu, int sign_xp,
                                                                               const int64_t *__restrict__ xvar, const int64_t *__restrict__ varmap,
                                                                               u64 *__restrict__ terms, double *__restrict__ consts) {
    dynamics_expand<true>(section, T, nx, nu, sign_xp, xvar, varmap, terms, consts);
}

}  // namespace pmt

using namespace pmt;

extern "C" int64_t pmt_batch_horizon_dynamics_tv_doubles(int64_t T, int64_t nx, int64_t nu) { return (T - 1) * nx * (nx + nu) + T * nx; }

extern "C" int pmt_batch_horizon_dynamics_tv_f64(const double *A, const double *Bm, const double *h, int64_t B, int64_t T, int64_t nx, int64_t nu,
                                                 int sign_a, int sign_b, int sign_h, double *out, int64_t out_stride, void *stream) {
    PMT_REQUIRE(B >= 0, PMT_DIMENSION_MISMATCH, "batch_horizon_dynamics_tv: negative instance count");
    const int rc = dynamics_check_dims("batch_horizon_dynamics_tv", T, nx, nu);
    if (rc != PMT_OK) return rc;
    PMT_REQUIRE(out_stride >= pmt_batch_horizon_dynamics_tv_doubles(T, nx, nu), PMT_DIMENSION_MISMATCH,
                "batch_horizon_dynamics_tv: out_stride smaller than the section");
    PMT_REQUIRE((sign_a == 1 || sign_a == -1) && (sign_b == 1 || sign_b == -1), PMT_INVALID_ARGUMENT,
                "batch_horizon_dynamics_tv: sign_a and sign_b must be +1 or -1");
    PMT_REQUIRE(sign_h >= -1 && sign_h <= 1, PMT_INVALID_ARGUMENT, "batch_horizon_dynamics_tv: sign_h must be -1, 0 or +1");
    if (B == 0) return PMT_OK;
    PMT_REQUIRE(out && (T == 1 || (A && (nu == 0 || Bm))) && (sign_h == 0 || h), PMT_INVALID_ARGUMENT, "batch_horizon_dynamics_tv: null pointer");
    BatchLtvArgs g;
    g.A = reinterpret_cast<const u64 *>(A); g.Bm = reinterpret_cast<const u64 *>(Bm);
    g.h = sign_h ? h : reinterpret_cast<const double *>(A);
    g.items = B * (T - 1);
    g.T = (int)T; g.nx = (int)nx; g.nu = (int)nu; g.sign_h = sign_h;
    g.flip_a = sign_a < 0 ? DY_SIGN_BIT : 0; g.flip_b = sign_b < 0 ? DY_SIGN_BIT : 0;
    g.out = out; g.out_stride = out_stride;
    return dispatch(stream, [=](hipStream_t s) {
        if (g.T == 1) {
            const dim3 grid((unsigned)std::min<int64_t>(cdiv(B, DY_THREADS / g.nx), (int64_t)DY_SMALL_WG_PER_CU * cu_count()));
            PMT_LAUNCH(batch_horizon_ltv_consts_kernel, grid, dim3(DY_THREADS), 0, s, h, B, g.nx, g.sign_h, g.out, g.out_stride);
            return check_launch("batch_horizon_ltv_consts_kernel");
        }
        if (g.nx * (g.nx + g.nu) <= DY_SMALL_WORDS) {
            const dim3 grid((unsigned)std::min<int64_t>(cdiv(g.items, DY_WAVES), (int64_t)DY_SMALL_WG_PER_CU * cu_count()));
            PMT_LAUNCH(batch_horizon_ltv_small_kernel, grid, dim3(DY_THREADS), 0, s, g);
            return check_launch("batch_horizon_ltv_small_kernel");
        }
        // a tile of half the words where it still holds a whole row of [A | B]: half the loads of a narrow pair fall on clamped columns
        // otherwise, and twice the workgroups are resident
        const int w = g.nx + g.nu, rl = g.nx <= 16 ? 16 : (g.nx <= 32 ? 32 : 64);
        const bool half = w <= DY_THREADS * LT_LOADS_HALF / rl;
        const dim3 grid((unsigned)std::min<int64_t>(g.items, (int64_t)(half ? LT_WG_PER_CU_HALF : LT_WG_PER_CU) * cu_count()));
        if (rl == 16 && half) PMT_LAUNCH_NAMED("batch_horizon_ltv_kernel", (batch_horizon_ltv_kernel<16, LT_LOADS_HALF>), grid, dim3(DY_THREADS), 0, s, g);
        else if (rl == 16) PMT_LAUNCH_NAMED("batch_horizon_ltv_kernel", (batch_horizon_ltv_kernel<16, LT_LOADS>), grid, dim3(DY_THREADS), 0, s, g);
        else if (rl == 32 && half) PMT_LAUNCH_NAMED("batch_horizon_ltv_kernel", (batch_horizon_ltv_kernel<32, LT_LOADS_HALF>), grid, dim3(DY_THREADS), 0, s, g);
        else if (rl == 32) PMT_LAUNCH_NAMED("batch_horizon_ltv_kernel", (batch_horizon_ltv_kernel<32, LT_LOADS>), grid, dim3(DY_THREADS), 0, s, g);
        else PMT_LAUNCH_NAMED("batch_horizon_ltv_kernel", (batch_horizon_ltv_kernel<64, LT_LOADS>), grid, dim3(DY_THREADS), 0, s, g);
        return check_launch("batch_horizon_ltv_kernel");
    });
}

extern "C" int pmt_batch_horizon_dynamics_tv_expand_f64(const double *section, int64_t T, int64_t nx, int64_t nu, int sign_xp, const int64_t *xvar,
                                                        const int64_t *varmap, pmt_vector_affine_term *out_terms, double *out_consts, void *stream) {
    const int rc = dynamics_check_dims("batch_horizon_dynamics_tv_expand", T, nx, nu);
    if (rc != PMT_OK) return rc;
    PMT_REQUIRE(sign_xp == 1 || sign_xp == -1, PMT_INVALID_ARGUMENT, "batch_horizon_dynamics_tv_expand: sign_xp must be +1 or -1");
    PMT_REQUIRE(section && xvar && out_terms && out_consts, PMT_INVALID_ARGUMENT, "batch_horizon_dynamics_tv_expand: null pointer");
    const int iT = (int)T, inx = (int)nx, inu = (int)nu;
    return dispatch(stream, [=](hipStream_t s) {
        return dynamics_expand_launch("batch_horizon_ltv_expand_kernel", batch_horizon_ltv_expand_kernel, s, section, iT, inx, inu, sign_xp, xvar, varmap, out_terms,
                                      out_consts);
    });
}
