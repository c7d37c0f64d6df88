// Batched tracking-cost QPs: transpose(x (+|-) p_i) * Q_i * (x (+|-) p_i) subject to C_i*x (+|-) d_i for B independent instances, one slab
//     [ Q: n(n+1)/2 | q: n | const: 1 | C: m*n row-major | d-consts: m ]
// per instance (the layout of batch.hip, so pmt_batch_expand_f64 and the slab exchange take it as it is).  In the reference a batch is many
// independent Models (src/model.jl:1-22); per instance this replaces matvecmul! over the affine vector (src/functions.jl:800-822), vecdot!
// (:702-709 over :548-576), canonicalize! (:381-386) and the MOI copies (src/moi_interop.jl:45-81), coefficients only.
//
// One workgroup of 256 threads per instance, persistent: workgroup g takes the instances g, g + G, ..  No workgroup waits for another, no
// atomics, no workspace.  It walks the instance's 64 x 64 tile pairs (J <= K) exactly as quad_form_tile<true> (form.hip) does for one
// instance: both source tiles read along their columns, the transpose-add through an LDS tile of pitch 65 doubles (a lane stride of 130
// dwords covers the 64 banks of a b64 read once per 32 lanes), one thread per row adding the row chains and — off the diagonal — one per
// column the column chains.  Where the single-instance node keeps the chains P[nb][n] in a global workspace and adds them in two further
// launches, n <= 256 lets them stay in LDS (8 KB): after the last tile one thread per j adds the blocks in order and stores q[j], the
// 256-entry tree gives the constant, and the same workgroup transposes its C_i through the tile and writes the d-consts.  Summation order and
// operations are those include/parametron_hip.h fixes for pmt_quad_form_shift_f64, so a slab equals what that node writes for the instance
// alone, bit for bit.  The Q section leaves as 8-byte stores with k on the lanes: a slab starts at any 8-byte address.
// LDS: 33280 (tile) + 8192 (P) + 2048 (c) + 2048 (tree) = 45568 bytes: three workgroups per CU.
// What the time is made of (profiles/r18_batch_form.txt): round trips to HBM.  No load is conditional and all loads of a tile are issued
// before the first value is looked at (landed); p and d are asked for at the top of an instance.  8192 x (128, 16): 462 us, 0.51 of 8 TB/s
// on the algorithmic bytes, against 871 us with every load waited for in turn.
#include <algorithm>

#include "common.h"

namespace pmt {

namespace {

constexpr int BF_TILE = 64;
constexpr int BF_THREADS = 256;
constexpr int BF_MAX_N = 256;
constexpr int BF_MAX_NB = BF_MAX_N / BF_TILE;
constexpr int BF_WG_PER_CU = 3;
static_assert(BF_MAX_N == PMT_BATCH_FORM_MAX_N, "the header's bound is the kernel's");
static_assert(BF_MAX_N <= BF_THREADS, "one thread per j adds the blocks; the tree takes one product per thread");

struct BatchFormArgs {
    const double *Q, *p, *C, *d;        // instance-major: Q[B][n*n] column-major, p[B][n], C[B][m*n] column-major, d[B][m]
    int64_t B, m;
    int n, sign_p, sign_d;
    double *out; int64_t out_stride;
};

}  // namespace

__global__ __launch_bounds__(BF_THREADS) void batch_form_kernel(BatchFormArgs g) {
    __shared__ double tile[BF_TILE][BF_TILE + 1];
    __shared__ double part[BF_MAX_NB][BF_MAX_N];          // P[B][j]
    __shared__ double cvec[BF_MAX_N];
    __shared__ double red[BF_THREADS];
    const int n = g.n, nt = (n + BF_TILE - 1) / BF_TILE;
    const int64_t m = g.m, nq = (int64_t)n * (n + 1) / 2;
    const int tid = threadIdx.x;
    const bool shift = g.sign_p != 0;

    for (int64_t inst = blockIdx.x; inst < g.B; inst += gridDim.x) {
        const double *__restrict__ Q = g.Q + inst * n * n;
        double *__restrict__ out = g.out + inst * g.out_stride;
        // p and d are asked for now and looked at behind the first tile's loads / at the end of the instance: no round trip of their own
        // (every thread loads, thread t >= n the last entry again)
        double pv = 0.0, dv = 0.0;
        if (shift && n > 0) pv = g.p[inst * n + (tid < n ? tid : n - 1)];
        if (g.sign_d && m > 0) dv = g.d[inst * m + (tid < m ? tid : m - 1)];
        bool c_pending = shift;

        for (int bj = 0; bj < nt; ++bj) {
            for (int bk = bj; bk < nt; ++bk) {
                const bool diagonal = bk == bj;
                // (the lane's coordinates are made opaque per tile: derived from loop invariants, the compiler otherwise keeps every address
                // and predicate of the unrolled body below alive across the whole instance loop — 234 vector registers instead of 3 waves a SIMD)
                int lane = tid & 63, wave = tid >> 6;
                asm volatile("" : "+v"(lane), "+v"(wave));
                const int j0 = bj * BF_TILE, k0 = bk * BF_TILE;
                // lower[i] = Q[k0 + lane, j0 + wave + 4 i] (k on the lanes); upper[i] = Q[j0 + lane, k0 + wave + 4 i] (j on the lanes)
                // Out-of-range entries are 0.0: the load goes to the instance's last row / column instead and is dropped, so no load is
                // conditional and an address is the uniform base plus one 32-bit offset.  All loads of a tile are issued before the first
                // value is looked at (landed: left to itself the compiler sinks every load into its own branch and waits for each in turn).
                double lower[16], upper[16];
                const int rk = k0 + lane, rj = j0 + lane;
                const unsigned ork = (unsigned)(rk < n ? rk : n - 1), orj = (unsigned)(rj < n ? rj : n - 1);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int c = j0 + wave + 4 * i;
                    lower[i] = Q[ork + (unsigned)(c < n ? c : n - 1) * (unsigned)n];
                }
                if (!diagonal) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int c = k0 + wave + 4 * i;
                        upper[i] = Q[orj + (unsigned)(c < n ? c : n - 1) * (unsigned)n];
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
                if (c_pending) {                        // c = 0.0 (+|-) p; read by the chains, behind this tile's barriers
                    asm volatile("" : "+v"(pv));        // (looked at here, not in front of the loads)
                    if (tid < n) cvec[tid] = signed_const(pv, g.sign_p);
                    c_pending = false;
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
                // tile[jj][kk] = s
#pragma unroll
                for (int i = 0; i < 16; ++i) tile[wave + 4 * i][lane] = s[i];
                __syncthreads();
                const int kw = n - k0 < BF_TILE ? n - k0 : BF_TILE, jw = n - j0 < BF_TILE ? n - j0 : BF_TILE;
                if (shift) {
                    // plain multiplies and adds, ascending, the first product starting the chain
                    if (wave == 0 && lane < jw) {
                        part[bk][j0 + lane] = chain(kw, [&](int kk) { const double a = tile[lane][kk]; return (diagonal && kk == lane) ? 2 * a : a; },
                                                       [&](int kk) { return cvec[k0 + kk]; });
                    } else if (wave == 1 && !diagonal && lane < kw) {
                        part[bj][k0 + lane] = chain(jw, [&](int jj) { return tile[jj][lane]; }, [&](int jj) { return cvec[j0 + jj]; });
                    }
                }
                // the Q section: row j holds its columns k >= j; this tile's piece of it, k on the lanes
#pragma unroll 4
                for (int r = 0; r < 16; ++r) {
                    const int jj = wave * 16 + r, j = j0 + jj;
                    const int k = k0 + lane;
                    if (j < n && k < n && k >= j) {
                        const double v = tile[jj][lane];
                        out[tri_pos(n, j, k)] = (k == j) ? 2 * v : v;
                    }
                }
                __syncthreads();
            }
        }

        // lin_j = ((P[0][j] + P[1][j]) + ..) + P[nb-1][j]; T by 256 chains onto 0.0 (n <= 256: one product each), then the halving tree
        double prod = 0.0;
        if (tid < n) {
            double lin = 0.0;
            if (shift) {
                lin = part[0][tid];
                for (int b = 1; b < nt; ++b) lin = lin + part[b][tid];
                prod = cvec[tid] * lin;
            }
            out[nq + tid] = lin;
        }
        double chain = 0.0;
        if (shift && tid < n) chain = chain + prod;
        red[tid] = chain;
        __syncthreads();
        for (int h = BF_THREADS / 2; h > 0; h >>= 1) {
            if (tid < h) red[tid] = red[tid] + red[tid + h];
            __syncthreads();
        }
        if (tid == 0) out[nq + n] = shift ? 0.5 * red[0] : 0.0;

        // the constraint block: C_i column-major -> row-major through the tile (rows on the lanes in, columns on the lanes out)
        if (m > 0 && n > 0) {
            const double *__restrict__ Ci = g.C + inst * m * n;
            double *__restrict__ oc = out + nq + n + 1;
            for (int64_t r0 = 0; r0 < m; r0 += BF_TILE) {
                for (int c0 = 0; c0 < n; c0 += BF_TILE) {
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
                        const int64_t r = r0 + wave + 4 * i;
                        const int c = c0 + lane;
                        if (r < m && c < n) oc[r * n + c] = tile[lane][wave + 4 * i];
                    }
                    __syncthreads();
                }
            }
        }
        if (m > 0) {
            double *__restrict__ od = out + nq + n + 1 + m * n;
            if (tid < m) od[tid] = signed_const(dv, g.sign_d);
            for (int64_t r = tid + BF_THREADS; r < m; r += BF_THREADS) od[r] = g.sign_d ? signed_const(g.d[inst * m + r], g.sign_d) : 0.0;
        }
        __syncthreads();                                  // the next instance reuses cvec, part and red
    }
}

}  // namespace pmt

using namespace pmt;

extern "C" int pmt_batch_form_coeffs_f64(const double *Q, const double *p, const double *Cm, const double *d, int64_t B, int64_t n, int64_t m,
                                         int sign_p, int sign_d, double *out, int64_t out_stride, void *stream) {
    PMT_REQUIRE(B >= 0 && n >= 0 && m >= 0, PMT_DIMENSION_MISMATCH, "batch_form: negative dimension");
    PMT_REQUIRE(n <= BF_MAX_N, PMT_DIMENSION_MISMATCH, "batch_form: more than 256 variables per instance");
    const int64_t L = pmt_batch_lsq_slab_doubles(n, m);
    PMT_REQUIRE(out_stride >= L, PMT_DIMENSION_MISMATCH, "batch_form: out_stride smaller than the slab");
    PMT_REQUIRE(sign_p >= -1 && sign_p <= 1 && sign_d >= -1 && sign_d <= 1, PMT_INVALID_ARGUMENT, "batch_form: signs must be -1, 0 or +1");
    if (B == 0) return PMT_OK;
    PMT_REQUIRE(out && (n == 0 || Q) && (n == 0 || sign_p == 0 || p) && (m * n == 0 || Cm) && (m == 0 || d), PMT_INVALID_ARGUMENT,
                "batch_form: null pointer");
    BatchFormArgs g;
    g.Q = Q; g.p = p; g.C = Cm; g.d = d;
    g.B = B; g.m = m;
    g.n = (int)n; g.sign_p = sign_p; g.sign_d = sign_d;
    g.out = out; g.out_stride = out_stride;
    return dispatch(stream, [=](hipStream_t s) {
        // three workgroups per CU stay resident (LDS); each walks the instances blockIdx.x, blockIdx.x + G, ..
        const dim3 grid((unsigned)std::min<int64_t>(B, (int64_t)BF_WG_PER_CU * cu_count()));
        PMT_LAUNCH(batch_form_kernel, grid, dim3(BF_THREADS), 0, s, g);
        return check_launch("batch_form_kernel");
    });
}
