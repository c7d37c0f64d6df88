// One tile of the dense affine kernels: TR x 64 entries of the column-major matrix, transposed through LDS, written as row-major terms.
// affine.hip's affine_tile_kernel runs it as one workgroup per tile; the one-launch Gram node (gram_mid.hip) runs the same body for its
// RIDERS — constraint packs whose tiles the persistent workgroups draw once their Gram items have run out — so every stored word of a
// ridden pack is the expression the stand-alone launch stores.
#pragma once
#include "common.h"

namespace pmt {

constexpr int TILE = 64;
constexpr int PITCH = TILE + 1;

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u64 f2u(double x) { return (u64)__double_as_longlong(x); }

template <bool NT>
__device__ __forceinline__ void store16(u64x2 *p, u64x2 v) {
    if (NT) __builtin_nontemporal_store(v, p); else *p = v;
}
template <bool NT>
__device__ __forceinline__ void store8(u64 *p, u64 v) {
    if (NT) __builtin_nontemporal_store(v, p); else *p = v;
}

// A dense MOI vector pack (the arguments of pmt_affine_pack_vector_f64) as the one-launch Gram node carries it: the stand-alone launch's
// choices (launch_affine: load / store paths, tile height, nontemporal policies) are made on the host, once, by affine_rider
struct AffineRider {
    const double *A; int64_t lda, rows, cols;
    const int64_t *xvar; const double *b; const int64_t *varmap; int64_t row_offset;
    u64 *out; double *out_consts;
    int sign, vec_in, vec_out;
    int tr, nt, ntl;              // rows per tile (32 / 64); nontemporal stores; nontemporal loads of the matrix
    int tiles_x, first_tile;      // 64-column tiles per tile row; the pack's first tile in the launch's numbering
};

// MODE 0: LinearTerm output   MODE 1: VectorAffineTerm output.  Tile (bx, by) of the block; thread t of 256.  tile: TR * PITCH doubles
// and vmx: TILE words of LDS.  One workgroup barrier between the load and the store phase; the caller orders the LDS against its reuse.
template <int MODE, bool NT, int TR, bool NTL>
__device__ __forceinline__ void affine_tile_body(const double *__restrict__ A, int64_t lda, int64_t rows, int64_t cols,
                                                 const int64_t *__restrict__ xvar, const double *__restrict__ b, int sign,
                                                 const int64_t *__restrict__ varmap, int64_t row_offset, u64 *__restrict__ out,
                                                 double *__restrict__ out_consts, int vec_in, int vec_out, int bx, int by, int t,
                                                 double *tile, u64 *vmx) {
    const int lane = t & 63;
    const int wave = t >> 6;
    const int64_t c0 = (int64_t)bx * TILE;
    const int64_t r0 = (int64_t)by * TR;
    const int nr = (int)min((int64_t)TR, rows - r0);
    const int nc = (int)min((int64_t)TILE, cols - c0);
    const bool full = (nr == TR) && (nc == TILE);

    // ---- load phase: column-major A tile -> LDS tile[row][col]
    if (full && vec_in) {
        constexpr int TPC = TR / 2;        // threads per column (16-byte pieces of a column segment)
        constexpr int CPI = 256 / TPC;     // columns per iteration
        const int cg = t / TPC;            // column within the group
        const int lr = (t % TPC) * 2;      // row pair
        const double *base = A + (c0 + cg) * lda + r0 + lr;
#pragma unroll
        for (int it = 0; it < TILE / CPI; ++it) {
            const f64x2 *src = reinterpret_cast<const f64x2 *>(base + (int64_t)it * CPI * lda);
            f64x2 v = NTL ? __builtin_nontemporal_load(src) : *src;
            const int c = it * CPI + cg;
            tile[lr * PITCH + c] = v.x;
            tile[(lr + 1) * PITCH + c] = v.y;
        }
    } else {
        const int r = t & 63;
        for (int c = t >> 6; c < nc; c += 4)
            if (r < nr) tile[r * PITCH + c] = A[(c0 + c) * lda + r0 + r];
    }
    if (t < nc) {
        const int64_t v = xvar[c0 + t];
        vmx[t] = (u64)(MODE == 1 ? map_var(varmap, v) : v);
    }
    // constants: one column of blocks writes 0.0 (+|-) b[row]
    if (bx == 0 && t < nr && out_consts)
        out_consts[r0 + t] = signed_const(b ? b[r0 + t] : 0.0, b ? sign : 0);
    __syncthreads();

    // ---- store phase
    if (MODE == 0) {
        // 16 B per term: one wave store = 64 terms = 1 KiB contiguous
        if (lane < nc) {
            const u64 var = vmx[lane];
            for (int r = wave; r < nr; r += 4) {
                u64x2 v;
                v.x = f2u(tile[r * PITCH + lane]);
                v.y = var;
                store16<NT>(reinterpret_cast<u64x2 *>(out + ((r0 + r) * cols + c0 + lane) * 2), v);
            }
        }
    } else {
        if (full && vec_out) {
            // rows in pairs: 3 full-wave 16-byte stores per pair (row segment = 192 qwords = 96 chunks)
            for (int rp = wave * 2; rp < TR; rp += 8) {
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    int r, chunk;
                    if (s == 0) { r = rp; chunk = lane; }
                    else if (s == 1) { r = rp + (lane >> 5); chunk = 64 + (lane & 31); }
                    else { r = rp + 1; chunk = lane; }
                    const int q0 = chunk * 2;
                    const u64 rowidx = (u64)(row_offset + r0 + r + 1);
                    u64 w[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int q = q0 + h;
                        const int term = q / 3;
                        const int f = q - term * 3;
                        w[h] = (f == 0) ? rowidx : (f == 1 ? f2u(tile[r * PITCH + term]) : vmx[term]);
                    }
                    u64x2 v; v.x = w[0]; v.y = w[1];
                    store16<NT>(reinterpret_cast<u64x2 *>(out + ((r0 + r) * cols + c0) * 3 + q0), v);
                }
            }
        } else {
            if (lane < nc) {
                const u64 var = vmx[lane];
                for (int r = wave; r < nr; r += 4) {
                    u64 *p = out + ((r0 + r) * cols + c0 + lane) * 3;
                    store8<NT>(p, (u64)(row_offset + r0 + r + 1));
                    store8<NT>(p + 1, f2u(tile[r * PITCH + lane]));
                    store8<NT>(p + 2, var);
                }
            }
        }
    }
}

// The rider form of a recorded dense MOI pack (SmallNode of SOP_AFFINE_VAT), with the stand-alone launch's choices; false: not a pack
// that can ride (no rows or no columns).  affine_rider_tiles: its tile count alone, from the shape (a pure host function).
bool affine_rider(const SmallNode &nd, AffineRider *out);
int64_t affine_rider_tiles(int64_t rows, int64_t cols);

}  // namespace pmt
