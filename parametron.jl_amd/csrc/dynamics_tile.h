// What the two dynamics files of the batched horizons share (batch_horizon_dyn.hip: one [A_i | B_i] per instance; batch_horizon_ltv.hip: one
// per instance and stage): the launch shape and bounds, the dimension check, the loads of a tile of [A | B], the source of a word of the
// small path, and the expansion of one instance's section with its launch.  The files keep what differs: where the pair and its block
// sit, the loop over the tiles (one instance per pass against one fused (item, r0, c0) loop with the next tile's loads issued early), the
// h-consts and the entry points.  They also keep, each its copy, the tile's signed LDS store and row write-out and the small path's load /
// flip / store loops: moved into functions of this header those compile to other device code in the coefficient kernels (operand order,
// scalar moves), which have to stay as they are.
//
// [A | B] (nx rows, w = nx + nu columns, both halves column-major with leading dimension nx) is walked in tiles of RL rows x CW columns,
// thread (lr = tid % RL, lc = tid / RL) loading the columns lc, lc + 256 / RL, ..: LPT loads per thread, so CW = 256 * LPT / RL.  No load is
// conditional (an index past the edge goes to the last row / column and is dropped); the tile is transposed through LDS at pitch CW + 1
// words — 16 consecutive lanes hold 16 rows of one column, a stride of 2 mod 32 dwords, which covers the 32 banks of a b64 write once — and
// rows leave with the column on the lanes as 8-byte stores, so a block starts at any 8-byte address.
#pragma once
#include <algorithm>

#include "common.h"

namespace pmt {

typedef unsigned long long u64;

constexpr int DY_THREADS = 256;
constexpr int DY_WAVES = DY_THREADS / 64;
constexpr int DY_SMALL_WORDS = 512;          // AB words up to which a matrix pair takes a wave: eight loads per lane
constexpr int DY_SMALL_LOADS = DY_SMALL_WORDS / 64;
constexpr int DY_SMALL_WG_PER_CU = 8;
constexpr int DY_EXPAND_ROWS = DY_WAVES;     // rows of a stage per work item of the expansion: one per wave
constexpr int DY_MAX_DIM = PMT_BATCH_HORIZON_MAX_DIM, DY_MAX_T = PMT_BATCH_HORIZON_MAX_T;
constexpr u64 DY_SIGN_BIT = 0x8000000000000000ull;
static_assert(2 * DY_MAX_DIM <= DY_THREADS, "one thread per index word of a stage, per constant of an item's two stages; a 16-row tile holds a whole row of [A | B]");

// the dimension checks all four entry points share; `who` words the message
inline int dynamics_check_dims(const char *who, int64_t T, int64_t nx, int64_t nu) {
    const std::string w(who);
    PMT_REQUIRE(nx >= 1 && nx <= DY_MAX_DIM, PMT_DIMENSION_MISMATCH, w + ": nx outside 1 .. 128");
    PMT_REQUIRE(nu >= 0 && nu <= DY_MAX_DIM, PMT_DIMENSION_MISMATCH, w + ": nu outside 0 .. 128");
    PMT_REQUIRE(T >= 1 && T <= DY_MAX_T, PMT_DIMENSION_MISMATCH, w + ": T outside 1 .. 512");
    return PMT_OK;
}

// The tile (r0, c0) of [Ai | Bi] into v; -> the thread's place (lr, lc) in the tile.  (The place is made opaque per tile: derived from
// loop invariants, the compiler otherwise keeps every address of the unrolled body alive across the whole loop over the tiles.)
template <int RL, int LPT>
__device__ __forceinline__ void dynamics_tile_load(const u64 *__restrict__ Ai, const u64 *__restrict__ Bi, int nx, int w, int r0, int c0, int tid,
                                                   u64 (&v)[LPT], int &lr, int &lc) {
    constexpr int CSTEP = DY_THREADS / RL;
    lr = tid % RL; lc = tid / RL;
    asm volatile("" : "+v"(lr), "+v"(lc));
    const int r = r0 + lr;
    const unsigned rc = (unsigned)(r < nx ? r : nx - 1);
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
        const int c = c0 + lc + CSTEP * i, cc = c < w ? c : w - 1;
        const u64 *__restrict__ col = cc < nx ? Ai + (unsigned)cc * (unsigned)nx : Bi + (unsigned)(cc - nx) * (unsigned)nx;
        v[i] = col[rc];
    }
}

// The small path, a wave per pair of at most DY_SMALL_WORDS AB words: lane l writes the words l, l + 64, .. of AB in output order.  The
// source of word e — row r = e / w, column j = e - r*w of [A | B] — is the same for every pair: -> its index in A (from_a) or in B.
__device__ __forceinline__ unsigned dynamics_small_source(int e, int nx, int w, int nab, bool &from_a) {
    const int ec = e < nab ? e : nab - 1;
    const int r = ec / w, j = ec - r * w;
    from_a = j < nx;
    return (unsigned)(r + (j < nx ? j : j - nx) * nx);
}

// One instance's records from its section: a streaming writer.  Items, dealt out over the workgroups: (stage t >= 1, four rows) — the
// stage's nx + nu index words vm[xvar[..]] are fetched once into LDS, then a wave per row writes its 1 + nx + nu terms through
// wave_write_words (common.h), each AB word read by the one lane that stores it —, then stage 0, then the constants 256 at a time.
// TV: stage t's rows come from its own block AB_t, (t-1)*nab words into the section, and the constants lie behind T-1 blocks, not one.
// (nab = nx*w is written out where it is used: as a 64-bit constant in front of the loop it changes the time-invariant kernel's registers.)
template <bool TV>
__device__ __forceinline__ void dynamics_expand(const double *__restrict__ section, int T, int nx, int nu, int sign_xp,
                                                const int64_t *__restrict__ xvar, const int64_t *__restrict__ varmap, u64 *__restrict__ terms,
                                                double *__restrict__ consts) {
    __shared__ u64 vmx[DY_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = nx + nu, row_len = 1 + w, bands = (nx + DY_EXPAND_ROWS - 1) / DY_EXPAND_ROWS, nconst = T * nx;
    const int64_t ndyn = (int64_t)(T - 1) * bands, nitems = ndyn + 1 + (nconst + DY_THREADS - 1) / DY_THREADS;
    const u64 *__restrict__ ab = reinterpret_cast<const u64 *>(section);
    const u64 one = (u64)__double_as_longlong(1.0) ^ (sign_xp < 0 ? DY_SIGN_BIT : 0);
    for (int64_t it = blockIdx.x; it < nitems; it += gridDim.x) {
        if (it < ndyn) {
            const int t = 1 + (int)(it / bands), r = (int)(it % bands) * DY_EXPAND_ROWS + wave;
            // the columns of the stage's rows: the contiguous slice xvar[(t-1)*w .. t*w)
            if (tid < w) vmx[tid] = (u64)map_var(varmap, xvar[(int64_t)(t - 1) * w + tid]);
            __syncthreads();
            if (r < nx) {
                const u64 rowidx = (u64)(r + 1), xp = (u64)map_var(varmap, xvar[(int64_t)t * w + r]);
                const u64 *__restrict__ row = TV ? ab + (t - 1) * ((int64_t)nx * w) + r * w : ab + r * w;
                wave_write_words<3>(terms + 3 * (nx + ((int64_t)(t - 1) * nx + r) * row_len), row_len, lane, [&](int q) -> u64 {
                    const int e = q / 3, f = q - 3 * e;
                    if (f == 0) return rowidx;
                    if (e == 0) return f == 1 ? one : xp;
                    return f == 1 ? row[e - 1] : vmx[e - 1];
                });
            }
            __syncthreads();                              // the next item reuses vmx
        } else if (it == ndyn) {
            // stage 0: row i holds (i + 1, +-1.0, vm[xvar[i]])
            for (int i0 = wave * 64; i0 < nx; i0 += DY_THREADS) {
                wave_write_words<3>(terms + 3 * i0, nx - i0 < 64 ? nx - i0 : 64, lane, [&](int q) -> u64 {
                    const int e = q / 3, f = q - 3 * e;
                    if (f == 0) return (u64)(i0 + e + 1);
                    return f == 1 ? one : (u64)map_var(varmap, xvar[i0 + e]);
                });
            }
        } else {
            const int i = (int)(it - ndyn - 1) * DY_THREADS + tid;
            if (i < nconst) consts[i] = TV ? section[(T - 1) * ((int64_t)nx * w) + i] : section[nx * w + i];
        }
    }
}

// the launch of the expansion under the kernel name `name` of the caller's file, its grid sized by the items
template <typename K>
inline int dynamics_expand_launch(const char *name, K kernel, hipStream_t s, const double *section, int T, int nx, int nu, int sign_xp, const int64_t *xvar,
                                  const int64_t *varmap, pmt_vector_affine_term *out_terms, double *out_consts) {
    const int64_t items = (int64_t)(T - 1) * cdiv(nx, DY_EXPAND_ROWS) + 1 + cdiv((int64_t)T * nx, DY_THREADS);
    PMT_LAUNCH_NAMED(name, kernel, dim3((unsigned)std::min<int64_t>(items, (int64_t)8 * cu_count())), dim3(DY_THREADS), 0, s, section, T,
                     nx, nu, sign_xp, xvar, varmap, reinterpret_cast<u64 *>(out_terms), out_consts);
    return check_launch(name);
}

}  // namespace pmt
