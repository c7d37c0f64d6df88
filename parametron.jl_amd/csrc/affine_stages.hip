// Horizon dynamics constraints: the MOI.VectorAffineFunction buffers of MANY affine records from one launch (pmt_affine_stages_f64).  What a
// model-predictive controller writes beside its stage costs (quad_stages.hip): T records x_{t+1} == A*x_t + B*u_t (+ w_t), every one a sum of
// two or three dense products over the shared matrix Parameters A and B, a Variable vector and at most one number vector.  In the reference
// each record is matvecmul! (src/functions.jl:775-798) per product, vecadd! / vecsubtract! (:751-764) per + / -, and the MOI copy
// (src/moi_interop.jl:64-81); on the device that was two pmt_affine_assemble_f64, two pmt_affvec_combine_f64 and one
// pmt_pack_vector_affine_f64 per record.  The combine multiplies by an exact +1 / -1 and the pack copies, so the words of a record are
// copies of the matrices' entries with, at most, their sign bit flipped: nothing is computed, and the launch is bound by its stores.
//
// Two device tables, built, checked (pmt_affine_stages_check) and uploaded once by the host: a record (pmt_affine_stage) names its rows, its
// slice of the two outputs, its number vector and a run of PARTS (pmt_affine_part) — the leaves of its sum in expression order: a matrix
// over a Variable vector (cols terms per row) or a Variable vector alone (one term per row), with the leaf's effective sign.
// Persistent workgroups of 256 threads, eight resident per CU: workgroup (x, y) walks the records x, x + X, ..; a record's work items — per
// matrix part its 16-row x 64-column tiles, per Variable-vector part the part itself — are numbered in table order and item k belongs to
// the workgroup with y == k mod Y (Y = 1 .. 8, the more the fewer records there are), so a record of several tiles is shared by Y
// workgroups that never talk to each other.  A tile is read along its columns (16 lanes on consecutive rows of a column), transposed
// through an LDS tile of pitch 65 doubles as affine_tile.h does, and every row segment leaves as 16-byte stores through wave_write_words
// (common.h) — a segment starts at any 8-byte word.  The shared matrices are read once per record and come from L2 behind the first
// records.  Every output word is written exactly once; no atomics; no workgroup waits for another.  LDS: 8320 (tile) + 512 (index words)
// bytes.  Measured (tools/affine_stages_probe.py, profiles/r21_affine_stages.txt): items of 16 rows instead of 64 and eight workgroups
// per CU instead of two took 100 records of 64 x (64 + 32 + 1) from 18.5 to 9.6 us and 200 of 128 x (128 + 32 + 1) from 89.7 to 30.5 us.
#include <algorithm>
#include <vector>

#include "affine_tile.h"

namespace pmt {

namespace {

constexpr int AS_THREADS = 256;
constexpr int AS_BAND = 16;                  // rows of a work item
constexpr int AS_WG_PER_CU = 8;              // resident workgroups per CU the persistent grid is sized for (LDS: 9 KB each)
constexpr int AS_SPLIT = 8;                  // at most this many workgroups share a record's items when there are few records
static_assert(sizeof(pmt_affine_part) == 32, "pmt_affine_part: 32 bytes, no padding (the ctypes and Julia mirrors)");
static_assert(sizeof(pmt_affine_stage) == 48, "pmt_affine_stage: 48 bytes, no padding (the ctypes and Julia mirrors)");
static_assert(PMT_AFFINE_STAGES_MAX_PARTS == 8, "the header's bound is the check's");

struct AffineStagesArgs {
    const pmt_affine_stage *stages; int64_t T;
    const pmt_affine_part *parts;
    const int64_t *varmap;
    u64 *terms; double *consts;
};

constexpr u64 AS_SIGN_BIT = 0x8000000000000000ull;

}  // namespace

__global__ __launch_bounds__(AS_THREADS) void affine_stages_kernel(AffineStagesArgs g) {
    __shared__ double tile[AS_BAND * PITCH];
    __shared__ u64 vmx[TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t *__restrict__ varmap = g.varmap;
    const int by = blockIdx.y, ny = gridDim.y;

    for (int64_t s = blockIdx.x; s < g.T; s += gridDim.x) {
        const pmt_affine_stage d = g.stages[s];
        const int rows = d.rows;
        const int64_t row_len = d.row_len;
        u64 *__restrict__ out = g.terms + 3 * d.term_offset;
        if (by == 0) {
            // the constants: 0.0 (+|-) vec[i], 0.0 without a vector
            const double *__restrict__ vec = d.vec;
            for (int i = tid; i < rows; i += AS_THREADS)
                g.consts[d.const_offset + i] = signed_const(vec ? vec[i] : 0.0, vec ? d.vec_sign : 0);
        }
        int k = 0;                           // the record's items in table order
        int64_t o = 0;                       // the part's first term within a row
        for (int p = 0; p < d.nparts; ++p) {
            const pmt_affine_part pt = g.parts[d.first_part + p];
            const u64 flip = pt.sign < 0 ? AS_SIGN_BIT : 0;
            const int64_t *__restrict__ xvar = pt.xvar;
            if (!pt.mat) {
                // a Variable vector: row i holds (i + 1, +-1.0, vm[xvar[i]])
                if (k % ny == by) {
                    const u64 one = f2u(1.0) ^ flip;
                    for (int i = tid; i < rows; i += AS_THREADS) {
                        u64 *q = out + 3 * (i * row_len + o);
                        q[0] = (u64)(i + 1);
                        q[1] = one;
                        q[2] = (u64)map_var(varmap, xvar[i]);
                    }
                }
                ++k;
                o += 1;
                continue;
            }
            const double *__restrict__ A = pt.mat;
            const int64_t ld = pt.ld;
            const int cols = pt.cols;
            for (int r0 = 0; r0 < rows; r0 += AS_BAND) {
                const int nr = rows - r0 < AS_BAND ? rows - r0 : AS_BAND;
                for (int c0 = 0; c0 < cols; c0 += TILE, ++k) {
                    if (k % ny != by) continue;
                    const int nc = cols - c0 < TILE ? cols - c0 : TILE;
                    // column-major tile -> tile[row][col]: AS_BAND lanes on consecutive rows of one column
                    const int lr = tid % AS_BAND;
                    if (lr < nr)
                        for (int c = tid / AS_BAND; c < nc; c += AS_THREADS / AS_BAND) tile[lr * PITCH + c] = A[(int64_t)(c0 + c) * ld + r0 + lr];
                    if (tid < nc) vmx[tid] = (u64)map_var(varmap, xvar[c0 + tid]);
                    __syncthreads();
                    // a wave per row segment of nc terms
                    for (int r = wave; r < nr; r += 4) {
                        const u64 rowidx = (u64)(r0 + r + 1);
                        const double *trow = tile + r * PITCH;
                        wave_write_words<3>(out + 3 * ((int64_t)(r0 + r) * row_len + o + c0), nc, lane, [&](int q) -> u64 {
                            const int e = q / 3, f = q - 3 * e;
                            if (f == 0) return rowidx;
                            if (f == 2) return vmx[e];
                            return f2u(trow[e]) ^ flip;
                        });
                    }
                    __syncthreads();                      // the next item reuses tile and vmx
                }
            }
            o += cols;
        }
    }
}

// slices [at, at + len) sorted by their start tile [0, total): the first starts at 0, each starts where the one before ends, the last ends at total
static bool as_slices_tile(std::vector<std::pair<int64_t, int64_t>> &s, int64_t total) {
    std::sort(s.begin(), s.end());
    int64_t end = 0;
    for (const auto &p : s) {
        if (p.first != end || p.second > total - p.first) return false;
        end = p.first + p.second;
    }
    return end == total;
}

}  // namespace pmt

using namespace pmt;

extern "C" int pmt_affine_stages_check(const pmt_affine_stage *host_stages, int64_t T, const pmt_affine_part *host_parts, int64_t nparts,
                                       int64_t nterms, int64_t nconsts) {
    PMT_REQUIRE(T >= 0 && nparts >= 0, PMT_DIMENSION_MISMATCH, "affine_stages: negative stage or part count");
    PMT_REQUIRE(nterms >= 0 && nconsts >= 0, PMT_DIMENSION_MISMATCH, "affine_stages: negative term or constant count");
    if (T == 0) {
        PMT_REQUIRE(nterms == 0 && nconsts == 0, PMT_DIMENSION_MISMATCH, "affine_stages: no stage, but terms or constants to tile");
        return PMT_OK;
    }
    PMT_REQUIRE(host_stages && host_parts, PMT_INVALID_ARGUMENT, "affine_stages: null stage or part table");
    std::vector<std::pair<int64_t, int64_t>> terms, consts;
    terms.reserve((size_t)T);
    consts.reserve((size_t)T);
    for (int64_t t = 0; t < T; ++t) {
        const pmt_affine_stage &d = host_stages[t];
        const std::string at = " (stage " + std::to_string(t) + ")";
        PMT_REQUIRE(d.vec_sign >= -1 && d.vec_sign <= 1, PMT_INVALID_ARGUMENT, "affine_stages: vec_sign must be -1, 0 or +1" + at);
        PMT_REQUIRE((d.vec_sign != 0) == (d.vec != nullptr), PMT_INVALID_ARGUMENT, "affine_stages: a number vector needs a sign of +-1, no vector a sign of 0" + at);
        PMT_REQUIRE(d.rows >= 1, PMT_DIMENSION_MISMATCH, "affine_stages: rows below 1" + at);
        PMT_REQUIRE(d.nparts >= 1 && d.nparts <= PMT_AFFINE_STAGES_MAX_PARTS, PMT_DIMENSION_MISMATCH, "affine_stages: nparts outside 1 .. 8" + at);
        PMT_REQUIRE(d.first_part >= 0 && (int64_t)d.first_part <= nparts - d.nparts, PMT_DIMENSION_MISMATCH, "affine_stages: parts outside the part table" + at);
        PMT_REQUIRE(d.term_offset >= 0 && d.const_offset >= 0, PMT_DIMENSION_MISMATCH, "affine_stages: a slice starts below 0" + at);
        int64_t len = 0;
        for (int p = 0; p < d.nparts; ++p) {
            const pmt_affine_part &q = host_parts[d.first_part + p];
            const std::string pat = " (stage " + std::to_string(t) + ", part " + std::to_string(p) + ")";
            PMT_REQUIRE(q.xvar, PMT_INVALID_ARGUMENT, "affine_stages: null variable indices" + pat);
            PMT_REQUIRE(q.sign == 1 || q.sign == -1, PMT_INVALID_ARGUMENT, "affine_stages: a part's sign must be +1 or -1" + pat);
            PMT_REQUIRE(q.cols >= 1, PMT_DIMENSION_MISMATCH, "affine_stages: cols below 1" + pat);
            if (q.mat) PMT_REQUIRE(q.ld >= d.rows, PMT_DIMENSION_MISMATCH, "affine_stages: ld < rows" + pat);
            else PMT_REQUIRE(q.cols == 1, PMT_DIMENSION_MISMATCH, "affine_stages: a Variable-vector part has one term per row" + pat);
            len += q.cols;
        }
        PMT_REQUIRE(d.row_len == len, PMT_DIMENSION_MISMATCH, "affine_stages: row_len is not the sum of the parts' cols" + at);
        PMT_REQUIRE(len <= INT64_MAX / (3 * (int64_t)d.rows), PMT_DIMENSION_MISMATCH, "affine_stages: rows * row_len overflows" + at);
        terms.emplace_back(d.term_offset, (int64_t)d.rows * len);
        consts.emplace_back(d.const_offset, (int64_t)d.rows);
    }
    PMT_REQUIRE(as_slices_tile(terms, nterms), PMT_DIMENSION_MISMATCH, "affine_stages: the term slices overlap, leave a gap or do not end at nterms");
    PMT_REQUIRE(as_slices_tile(consts, nconsts), PMT_DIMENSION_MISMATCH, "affine_stages: the constant slices overlap, leave a gap or do not end at nconsts");
    return PMT_OK;
}

extern "C" int pmt_affine_stages_f64(const pmt_affine_stage *stages, int64_t T, const pmt_affine_part *parts, const int64_t *varmap,
                                     pmt_vector_affine_term *out_terms, double *out_consts, void *stream) {
    PMT_REQUIRE(T >= 0, PMT_DIMENSION_MISMATCH, "affine_stages: negative stage count");
    PMT_REQUIRE(T == 0 || (stages && parts && out_terms && out_consts), PMT_INVALID_ARGUMENT, "affine_stages: null pointer");
    if (T == 0) return PMT_OK;
    AffineStagesArgs g;
    g.stages = stages; g.T = T;
    g.parts = parts;
    g.varmap = varmap;
    g.terms = reinterpret_cast<u64 *>(out_terms); g.consts = out_consts;
    return dispatch(stream, [=](hipStream_t s) {
        // persistent in x over the records; fewer records than resident workgroups: up to AS_SPLIT workgroups share each record's items
        const int64_t resident = (int64_t)AS_WG_PER_CU * cu_count();
        const unsigned gy = (unsigned)std::max<int64_t>(1, std::min<int64_t>(AS_SPLIT, resident / T));
        const dim3 grid((unsigned)std::min<int64_t>(T, resident / gy), gy);
        PMT_LAUNCH(affine_stages_kernel, grid, dim3(AS_THREADS), 0, s, g);
        return check_launch("affine_stages_kernel");
    });
}
