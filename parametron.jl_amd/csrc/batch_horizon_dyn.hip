// The batch of horizons' dynamics rows as a compact section per instance (pmt_batch_horizon_dynamics_f64): instance i's constraints
//     x_0 (+|-) h_{i,0},    (+|-)x_t (+|-) A_i*x_{t-1} (+|-) B_i*u_{t-1} (+|-) h_{i,t},  t = 1 .. T-1
// over z = [x_0; u_0; x_1; u_1; ..] are T vector-affine records whose coefficient words are T-1 copies of [A_i | B_i] and a +-1.0 per row;
// the section
//     [ AB: nx*(nx + nu) row-major | h-consts: T*nx ]
// holds what differs between instances once.  In the reference a batch is many independent Models (src/model.jl:1-22); per instance and
// record this replaces matvecmul! (src/functions.jl:775-798), vecadd! / vecsubtract! (:751-764) and the MOI copy
// (src/moi_interop.jl:64-81) — the records of affine_stages.hip on the instance's own tables.  Nothing is computed: copies, sign-bit flips
// and 0.0 (+|-) h, so the launch is bound by its loads and stores.
//
// Persistent workgroups of 256 threads, workgroup g taking the instances g, g + G, ..  No workgroup waits for another, no atomics, no
// workspace.  [A_i | B_i] (nx rows, nx + nu columns, both halves column-major with leading dimension nx) is walked in tiles of 4096 words:
// 64 rows x 64 columns, or 32 x 128 with nx <= 32, or 16 x 256 with nx <= 16 (the kernel is instantiated by the tile's rows), so that a
// column of a narrow instance does not leave three quarters of a wave's lanes idle.  A tile is read along its columns as batch_form_kernel
// reads its tiles — no load is conditional (an index past the edge goes to the last row / column and is dropped), all 16 loads of a thread
// are issued before the first value is looked at (landed), the lane's coordinates are made opaque per tile — and transposed through an
// LDS tile of pitch columns + 1 doubles: 16 consecutive lanes hold 16 rows of one column, a stride of 2 mod 32 dwords, which covers the 32
// banks of a b64 write once; rows leave with the column on the lanes as 8-byte stores, so a section starts at any 8-byte address.  The
// h-consts stream through registers, four clamped loads per thread in flight.  LDS: 33280 bytes, four workgroups per CU.
// Small instances: with nx*(nx + nu) <= 512 words — (nx, nu) = (12, 4): 192 words — a tile, its two barriers and 16 loads per thread would be
// spent on a fraction of one wave's worth of words.  Such instances take a WAVE each, four to a workgroup (batch_horizon_dyn_small_kernel):
// the lanes walk the AB words in output order and read the entry each needs (the whole matrix is at most 4 KB, the reads of a wave fall
// into its few cache lines), eight clamped loads per lane in flight; no LDS, no barrier.  The words are copies either way.
//
// pmt_batch_horizon_dynamics_expand_f64 rebuilds one instance's MOI buffers from its section: the streaming writer both dynamics files
// share (dynamics_expand<false>, dynamics_tile.h, where the tile's loads, the small path's word source, the constants of the launch
// shape and the dimension check lie too).
#include "dynamics_tile.h"

namespace pmt {

namespace {

constexpr int BD_LOADS = 16;                 // loads per thread of a tile: 4096 words
constexpr int BD_WG_PER_CU = 4;              // resident workgroups per CU of the tile kernel (LDS: 33280 bytes each)

struct BatchDynArgs {
    const u64 *A, *Bm;                       // instance-major: A[B][nx*nx], Bm[B][nx*nu] column-major, leading dimension nx
    const double *h;                         // h[B][T*nx] stage-major
    int64_t B;
    int T, nx, nu, sign_h;
    u64 flip_a, flip_b;                      // the sign bit where the sign is -1
    double *out; int64_t out_stride;
};

// h-consts[i] = 0.0 (+|-) h[i], i < cnt, the `width` threads of the caller striding together; four clamped loads per thread in flight
__device__ __forceinline__ void bd_consts(const double *__restrict__ h, int sign, int cnt, double *__restrict__ o, int first, int width) {
    if (sign == 0) {
        for (int i = first; i < cnt; i += width) o[i] = 0.0;
        return;
    }
    for (int i0 = first; i0 < cnt; i0 += 4 * width) {
        double hv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = i0 + k * width;
            hv[k] = h[i < cnt ? i : cnt - 1];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = i0 + k * width;
            if (i < cnt) o[i] = signed_const(hv[k], sign);
        }
    }
}

}  // namespace

// RL rows x CW = 4096 / RL columns a tile (dynamics_tile.h), one instance per pass of a workgroup
template <int RL>
__global__ __launch_bounds__(DY_THREADS) void batch_horizon_dyn_kernel(BatchDynArgs g) {
    constexpr int CW = DY_THREADS * BD_LOADS / RL, PITCH = CW + 1, CSTEP = DY_THREADS / RL;
    __shared__ u64 tile[RL * PITCH];
    const int T = g.T, nx = g.nx, nu = g.nu, w = nx + nu;
    const int tid = threadIdx.x;
    const u64 flip_a = g.flip_a, flip_b = g.flip_b;

    for (int64_t inst = blockIdx.x; inst < g.B; inst += gridDim.x) {
        const u64 *__restrict__ Ai = g.A + inst * nx * nx;
        const u64 *__restrict__ Bi = nu ? g.Bm + inst * nx * nu : Ai;            // (nu == 0: no column selects it)
        u64 *__restrict__ out = reinterpret_cast<u64 *>(g.out + inst * g.out_stride);
        bd_consts(g.sign_h ? g.h + inst * T * nx : nullptr, g.sign_h, T * nx, g.out + inst * g.out_stride + (int64_t)nx * w, tid, DY_THREADS);

        for (int r0 = 0; r0 < nx; r0 += RL) {
            for (int c0 = 0; c0 < w; c0 += CW) {
                int lr, lc;
                u64 v[BD_LOADS];
                dynamics_tile_load<RL, BD_LOADS>(Ai, Bi, nx, w, r0, c0, tid, v, lr, lc);
                landed(v);
                // tile[row][column], each word with its part's sign
                // (batch_horizon_ltv.hip holds this store too: moved into a shared function it compiles to other device code)
#pragma unroll
                for (int i = 0; i < BD_LOADS; ++i) tile[lr * PITCH + lc + CSTEP * i] = v[i] ^ (c0 + lc + CSTEP * i < nx ? flip_a : flip_b);
                __syncthreads();
                // a wave per row, the column on the lanes
                // (batch_horizon_ltv.hip holds this write-out too: moved into a shared function it compiles to other device code)
                const int lane = tid & 63, wave = tid >> 6;
                const int nr = nx - r0 < RL ? nx - r0 : RL, nc = w - c0 < CW ? w - c0 : CW;
                for (int rr = wave; rr < nr; rr += DY_WAVES) {
                    u64 *__restrict__ orow = out + (int64_t)(r0 + rr) * w + c0;
                    for (int c = lane; c < nc; c += 64) orow[c] = tile[rr * PITCH + c];
                }
                __syncthreads();                          // the next tile reuses the LDS
            }
        }
    }
}

// A wave per instance of at most DY_SMALL_WORDS AB words (dynamics_tile.h)
__global__ __launch_bounds__(DY_THREADS) void batch_horizon_dyn_small_kernel(BatchDynArgs g) {
    const int T = g.T, nx = g.nx, nu = g.nu, w = nx + nu, nab = nx * w;
    const int lane = threadIdx.x & 63;
    const int64_t wv = (int64_t)blockIdx.x * DY_WAVES + (threadIdx.x >> 6), nwv = (int64_t)gridDim.x * DY_WAVES;
    const u64 flip_a = g.flip_a, flip_b = g.flip_b;
    unsigned src[DY_SMALL_LOADS];
    bool from_a[DY_SMALL_LOADS];
#pragma unroll
    for (int k = 0; k < DY_SMALL_LOADS; ++k) src[k] = dynamics_small_source(lane + 64 * k, nx, w, nab, from_a[k]);
    for (int64_t inst = wv; inst < g.B; inst += nwv) {
        const u64 *__restrict__ Ai = g.A + inst * nx * nx;
        const u64 *__restrict__ Bi = nu ? g.Bm + inst * nx * nu : Ai;            // (nu == 0: no word selects it)
        u64 *__restrict__ out = reinterpret_cast<u64 *>(g.out + inst * g.out_stride);
        // (batch_horizon_ltv.hip holds the load and the flip / store loop too: moved into shared functions they compile to other device code)
        u64 v[DY_SMALL_LOADS];
#pragma unroll
        for (int k = 0; k < DY_SMALL_LOADS; ++k) v[k] = (from_a[k] ? Ai : Bi)[src[k]];
        landed(v);
#pragma unroll
        for (int k = 0; k < DY_SMALL_LOADS; ++k) {
            const int e = lane + 64 * k;
            if (e < nab) out[e] = v[k] ^ (from_a[k] ? flip_a : flip_b);
        }
        bd_consts(g.sign_h ? g.h + inst * T * nx : nullptr, g.sign_h, T * nx, g.out + inst * g.out_stride + nab, lane, 64);
    }
}

__global__ __launch_bounds__(DY_THREADS) void batch_horizon_dyn_expand_kernel(const double *__restrict__ section, int T, int nx, int nu, int sign_xp,
                                                                               const int64_t *__restrict__ xvar, const int64_t *__restrict__ varmap,
                                                                               u64 *__restrict__ terms, double *__restrict__ consts) {
    dynamics_expand<false>(section, T, nx, nu, sign_xp, xvar, varmap, terms, consts);
}

}  // namespace pmt

using namespace pmt;

extern "C" int64_t pmt_batch_horizon_dynamics_doubles(int64_t T, int64_t nx, int64_t nu) { return nx * (nx + nu) + T * nx; }

extern "C" int pmt_batch_horizon_dynamics_f64(const double *A, const double *Bm, const double *h, int64_t B, int64_t T, int64_t nx, int64_t nu,
                                              int sign_a, int sign_b, int sign_h, double *out, int64_t out_stride, void *stream) {
    PMT_REQUIRE(B >= 0, PMT_DIMENSION_MISMATCH, "batch_horizon_dynamics: negative instance count");
    const int rc = dynamics_check_dims("batch_horizon_dynamics", T, nx, nu);
    if (rc != PMT_OK) return rc;
    PMT_REQUIRE(out_stride >= pmt_batch_horizon_dynamics_doubles(T, nx, nu), PMT_DIMENSION_MISMATCH,
                "batch_horizon_dynamics: out_stride smaller than the section");
    PMT_REQUIRE((sign_a == 1 || sign_a == -1) && (sign_b == 1 || sign_b == -1), PMT_INVALID_ARGUMENT,
                "batch_horizon_dynamics: sign_a and sign_b must be +1 or -1");
    PMT_REQUIRE(sign_h >= -1 && sign_h <= 1, PMT_INVALID_ARGUMENT, "batch_horizon_dynamics: sign_h must be -1, 0 or +1");
    if (B == 0) return PMT_OK;
    PMT_REQUIRE(out && A && (nu == 0 || Bm) && (sign_h == 0 || h), PMT_INVALID_ARGUMENT, "batch_horizon_dynamics: null pointer");
    BatchDynArgs g;
    g.A = reinterpret_cast<const u64 *>(A); g.Bm = reinterpret_cast<const u64 *>(Bm); g.h = h;
    g.B = B;
    g.T = (int)T; g.nx = (int)nx; g.nu = (int)nu; g.sign_h = sign_h;
    g.flip_a = sign_a < 0 ? DY_SIGN_BIT : 0; g.flip_b = sign_b < 0 ? DY_SIGN_BIT : 0;
    g.out = out; g.out_stride = out_stride;
    return dispatch(stream, [=](hipStream_t s) {
        if (g.nx * (g.nx + g.nu) <= DY_SMALL_WORDS) {
            const dim3 grid((unsigned)std::min<int64_t>(cdiv(B, DY_WAVES), (int64_t)DY_SMALL_WG_PER_CU * cu_count()));
            PMT_LAUNCH(batch_horizon_dyn_small_kernel, grid, dim3(DY_THREADS), 0, s, g);
            return check_launch("batch_horizon_dyn_small_kernel");
        }
        const dim3 grid((unsigned)std::min<int64_t>(B, (int64_t)BD_WG_PER_CU * cu_count()));
        if (g.nx <= 16) PMT_LAUNCH(batch_horizon_dyn_kernel<16>, grid, dim3(DY_THREADS), 0, s, g);
        else if (g.nx <= 32) PMT_LAUNCH(batch_horizon_dyn_kernel<32>, grid, dim3(DY_THREADS), 0, s, g);
        else PMT_LAUNCH(batch_horizon_dyn_kernel<64>, grid, dim3(DY_THREADS), 0, s, g);
        return check_launch("batch_horizon_dyn_kernel");
    });
}

extern "C" int pmt_batch_horizon_dynamics_expand_f64(const double *section, int64_t T, int64_t nx, int64_t nu, int sign_xp, const int64_t *xvar,
                                                     const int64_t *varmap, pmt_vector_affine_term *out_terms, double *out_consts, void *stream) {
    const int rc = dynamics_check_dims("batch_horizon_dynamics_expand", T, nx, nu);
    if (rc != PMT_OK) return rc;
    PMT_REQUIRE(sign_xp == 1 || sign_xp == -1, PMT_INVALID_ARGUMENT, "batch_horizon_dynamics_expand: sign_xp must be +1 or -1");
    PMT_REQUIRE(section && xvar && out_terms && out_consts, PMT_INVALID_ARGUMENT, "batch_horizon_dynamics_expand: null pointer");
    const int iT = (int)T, inx = (int)nx, inu = (int)nu;
    return dispatch(stream, [=](hipStream_t s) {
        return dynamics_expand_launch("batch_horizon_dyn_expand_kernel", batch_horizon_dyn_expand_kernel, s, section, iT, inx, inu, sign_xp, xvar, varmap, out_terms, out_consts);
    });
}
