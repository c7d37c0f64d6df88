// Geometry of the canonical least-squares contraction (gram_sk.hip), kept apart from the kernel bodies: argument block, tile geometry,
// work-unit numbering, the XCD-aware tile order, the accumulator lane map, the term store; and the host side of the node's forms.
#pragma once
#include "common.h"

namespace pmt {

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef unsigned long long u64;

constexpr int ST = 128;            // output tile edge
constexpr int SKC = 256;           // contraction depth per work unit (the most; SKArgs::skc)
constexpr int MAXG = 512;          // upper bound on persistent workgroups
constexpr int SLOT = ST * ST;      // doubles per partial-tile slot
constexpr int MAXGROUPS = 16;     // stages (band ranges) of a host delivery

struct SKArgs {
    const double *A; int64_t lda, rows, cols;
    const int64_t *xvar; const int64_t *varmap; int moi;
    QT *out_quad;     // MOI / native QuadraticTerms at the canonical row-major upper-triangular position, or null
    double *out_csc;  // solver form: alpha * (MOI coefficient) at k(k+1)/2 + j (CSC of the upper triangle, values only), or null
    double alpha;
    int ntiles, nchunk, G;
    int skc;          // rows per (tile, chunk) work unit: SKC, or less where SKC-row units would leave most of the chip idle (launch_gram_sk)
    int tfull;        // whole tiles per workgroup (phase A); tiles [tfull*G, T) are split along the contraction (phase B)
    int64_t U;        // number of (tile, chunk) units of phase B = (T - tfull*G) * nchunk
    int vec_in;
    double *ws;
    // Tile order: 0 = super-rows of 4 tile rows (sk_seq_unrank); w > 0 = super-columns of w tile columns (sk_colseq_unrank): the column
    // bands of the output complete in ascending order, which is what a solver hand-off in CSC order wants to ship first.
    int order_w;
    int seq_begin;    // this launch covers the tiles seq_begin, seq_begin + seq_step, .. (T' of them) of the sequence (a staged host delivery
                      // launches the contraction band range by band range; 0 and all tiles otherwise)
    int seq_step;     // +1, or -1: the sequence is walked from its end (column bands complete in DESCENDING order: the small ones last)
    unsigned *pair_flags; unsigned epoch;      // pair fold of a ranged launch (gram_sk.hip), or null
    unsigned flag_value;                       // what a first half stores into its tile's flag: `epoch` (anything else only under fault injection)
    int *error;                                // page-locked error word: a second half whose partner never showed up stores 2 here
    long long pair_timeout;                    // bound of the pair wait in 100 MHz ticks
    int strict;                                // ranged launches: the sequence enumerates the STRICTLY upper tiles (jb < kb) only — the diagonal
                                               // tiles of a wide tall matrix are computed by gram_tall.hip
};

// TN = 16-column MFMA tiles per wave along N.  One instance ships: TN = 2, 64x32 wave tiles, 8 waves.
template <int TN>
struct Cfg {
    static_assert(TN == 2, "the geometry below is the shipped one only");
    static constexpr int NW = 8;
    static constexpr int NT = NW * 64;
    static constexpr int WCOLS = 16 * TN;             // columns per wave
    static constexpr int NWC = ST / WCOLS;            // waves along N
    static constexpr int NACC = 4 * TN * 4;           // fp64 accumulators per lane
    static constexpr int NLD = (ST * 8) / NT;         // 16-byte pieces per thread per panel per 16 rows
};

__device__ __forceinline__ void sk_tri_unrank(int t, int nt, int &jb, int &kb) {
    int j = (int)((2.0 * nt + 1.0 - sqrt((2.0 * nt + 1.0) * (2.0 * nt + 1.0) - 8.0 * (double)t)) * 0.5);
    if (j < 0) j = 0;
    if (j > nt - 1) j = nt - 1;
    while (j > 0 && (j * nt - j * (j - 1) / 2) > t) --j;
    while (j + 1 < nt && ((j + 1) * nt - (j + 1) * j / 2) <= t) ++j;
    jb = j;
    kb = j + (t - (j * nt - j * (j - 1) / 2));
}

// L2-friendly enumeration of the upper-triangular tile grid: super-rows of 4 tile rows, each traversed column by column
// (kb-major), so 32 consecutive tiles form a ~4 x 8 block that needs only ~12 distinct column panels.  Workgroups round-robin
// over the 8 XCDs (bid % 8), each XCD with its own L2: at every time step the 32 workgroups of one XCD get 32 CONSECUTIVE tiles
// of this sequence, so most panel reads hit the XCD's L2 instead of going to the fabric.
__device__ __forceinline__ void sk_seq_unrank(int idx, int nt, int &jb, int &kb) {
    int base = 0;
    for (int R = 0; R * 4 < nt; ++R) {
        const int j0 = R * 4;
        const int h = min(4, nt - j0);                  // tile rows in this super-row
        const int W = nt - j0;                          // columns (kb = j0 .. nt-1)
        const int tri = h * (h + 1) / 2;                // the first h columns hold 1, 2, .., h tiles
        const int count = tri + (W - h) * h;
        if (idx < base + count) {
            int p = idx - base;
            if (p < tri) {
                int c = 0;
                while (p >= c + 1) { p -= c + 1; ++c; }
                kb = j0 + c; jb = j0 + p;
            } else {
                p -= tri;
                kb = j0 + h + p / h; jb = j0 + p % h;
            }
            return;
        }
        base += count;
    }
    jb = kb = nt - 1;
}

// Column-band-major enumeration: super-columns of w tile columns, each traversed row by row (jb-major), so 32 consecutive tiles form a
// (32/w) x w block and every column band kb is complete once the sequence has passed its super-column.
__device__ __forceinline__ void sk_colseq_unrank(int idx, int nt, int w, int &jb, int &kb) {
    int base = 0;
    for (int c0 = 0; c0 < nt; c0 += w) {
        const int h = min(w, nt - c0);                  // tile columns in this super-column
        const int rect = c0 * h;                        // rows 0 .. c0-1 hold h tiles each; rows c0 .. c0+h-1 hold h, h-1, .., 1
        const int count = rect + h * (h + 1) / 2;
        if (idx < base + count) {
            int p = idx - base;
            if (p < rect) {
                jb = p / h; kb = c0 + p % h;
            } else {
                p -= rect;
                int r = 0;
                while (p >= h - r) { p -= h - r; ++r; }
                jb = c0 + r; kb = c0 + r + p;
            }
            return;
        }
        base += count;
    }
    jb = kb = nt - 1;
}

// idx: position in the tile sequence (a ranged launch adds its seq_begin itself)
__device__ __forceinline__ void sk_tile_unrank(const SKArgs &g, int idx, int &jb, int &kb) {
    if (g.order_w > 0) sk_colseq_unrank(idx, g.ntiles, g.order_w, jb, kb);
    else sk_seq_unrank(idx, g.ntiles, jb, kb);
}

// strictly upper tiles of the nt x nt grid = the upper-inclusive triangle of size nt - 1 shifted one tile column to the right (the same
// L2-friendly super-row order)
__device__ __forceinline__ void sk_tile_unrank_strict(const SKArgs &g, int idx, int &jb, int &kb) {
    sk_seq_unrank(idx, g.ntiles - 1, jb, kb);
    kb += 1;
}

// sequence index of the t-th whole tile of workgroup bid (phase A)
__device__ __forceinline__ int sk_phase_a_index(const SKArgs &g, int bid, int t) {
    if ((g.G & 7) == 0) return (t * 8 + (bid & 7)) * (g.G >> 3) + (bid >> 3);
    return bid * g.tfull + t;
}

__device__ __forceinline__ int64_t sk_unit_begin(const SKArgs &g, int b) { return (int64_t)b * g.U / g.G; }

// the workgroup whose range of phase-B units holds unit u
__device__ __forceinline__ int sk_unit_owner(const SKArgs &g, int64_t u) {
    int b = (int)((u * g.G) / g.U);
    if (b >= g.G) b = g.G - 1;
    while (b + 1 < g.G && sk_unit_begin(g, b + 1) <= u) ++b;
    while (b > 0 && sk_unit_begin(g, b) > u) --b;
    return b;
}

// the workspace slot in which workgroup b left its partial of remainder tile rtile: its first slot if its range begins in that tile
__device__ __forceinline__ double *sk_partial_slot(const SKArgs &g, int b, int rtile) {
    const int64_t bu0 = sk_unit_begin(g, b);
    const int first_rtile = (int)(bu0 / g.nchunk);
    const int slot = 2 * b + (first_rtile == rtile ? 0 : 1);
    return g.ws + (int64_t)slot * SLOT;
}

// (row, col) inside the 128x128 tile of accumulator r = (tm*TN + tn)*4 + s of thread tid
template <int TN>
__device__ __forceinline__ void sk_acc_pos(int tid, int r, int &row, int &col) {
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave / Cfg<TN>::NWC, wc = wave % Cfg<TN>::NWC;
    const int tm = r / (4 * TN), tn = (r / 4) % TN, s = r & 3;
    const int i = lane >> 4, b = (lane >> 2) & 3, j = lane & 3;
    row = wr * 64 + tm * 16 + 4 * b + i;
    col = wc * Cfg<TN>::WCOLS + tn * 16 + 4 * ((b + s) & 3) + j;
}

// 2*acc -> QuadraticTerm at the canonical upper-triangular position
__device__ __forceinline__ void sk_store_term(const SKArgs &g, int jb, int kb, int row, int col, double v) {
    const int64_t n = g.cols;
    const int64_t j = (int64_t)jb * ST + row, k = (int64_t)kb * ST + col;
    if (k >= n || j >= n || j > k) return;
    double c = v;
    if (g.moi || j != k) c = 2 * c;          // off-diagonal: (j,k)+(k,j) combined; diagonal: MOI doubling (moi_interop.jl:58)
    if (g.out_csc) g.out_csc[k * (k + 1) / 2 + j] = g.alpha * c;
    if (!g.out_quad) return;
    const int64_t jv = g.xvar[j], kv = g.xvar[k];
    const int64_t pos = j * n - (j * (j - 1)) / 2 + (k - j);
    u64 *p = reinterpret_cast<u64 *>(g.out_quad) + pos * 3;
    p[0] = (u64)__double_as_longlong(c);
    p[1] = (u64)(g.moi ? map_var(g.varmap, jv) : jv);
    p[2] = (u64)(g.moi ? map_var(g.varmap, kv) : kv);
}


// ---- host side: the launchers of the node's forms, their size helpers and the predicates gram.hip's gram_form decides by; what else it calls
int launch_gram_sk(const double *A, int64_t lda, int64_t rows, int64_t cols, const int64_t *xvar, const int64_t *varmap, int moi,
                   pmt_quadratic_term *out_quad, double *out_csc, double alpha, void *workspace, int order_w, int64_t seq_begin, int64_t seq_count,
                   unsigned *pair_flags, unsigned epoch, int *error_word, hipStream_t s, int strict = 0);
size_t gram_sk_workspace_bytes(int64_t rows, int64_t cols);
bool gram_tiny(int64_t rows, int64_t cols);
bool gram_tall_applies(int64_t rows, int64_t cols);
bool gram_tall_diag_applies(int64_t rows, int64_t cols);
int gram_tall_groups(int64_t rows, int64_t cols);
int gram_tall_stage_rows(int64_t rows, int64_t cols);
int gram_tall_run_lanes(int64_t rows, int64_t cols);
size_t gram_tall_workspace_bytes(int64_t rows, int64_t cols);
int launch_gram_tall(const double *A, int64_t lda, int64_t rows, int64_t cols, const int64_t *xvar, const double *b, int sign, int moi,
                     const int64_t *varmap, pmt_quadratic_term *out_quad, double *out_csc, double alpha, pmt_linear_term *out_lin,
                     double *out_const, void *workspace, hipStream_t s);
size_t gram_mid_workspace_bytes(int64_t rows, int64_t cols);
int gram_mid_counters(int64_t cols);
bool gram_mid_defers(int64_t rows, int64_t cols, bool *whole_rounds);          // the shape's plan defers tiles (gram_mid.hip: MidWalk)
bool gram_mid_strips(int64_t rows, int64_t cols, int *strips, int *tiles_in_strips);          // the shape's plan runs its first body tiles as strips, a whole tile per wave (gram_mid.hip: mid_strips)
int launch_gram_mid(const double *A, int64_t lda, int64_t rows, int64_t cols, const int64_t *xvar, const double *b, int sign, int moi,
                    const int64_t *varmap, pmt_quadratic_term *out_quad, double *out_csc, double alpha, pmt_linear_term *out_lin,
                    double *out_const, void *workspace, unsigned *counters, const void *riders, int nriders, int rider_tiles, hipStream_t s);
bool gram_mid_persistent(int64_t rows, int64_t cols);          // the shape runs as PMT_MID_G persistent workgroups (the form that takes riders)
// What a recorded one-launch node that delivers nothing to the host tells its plan, which decides who rides in it (plan.hip): its operands;
// the plan derives the byte ranges the node reads (A, b, xvar, varmap) and writes (out_quad / out_csc, out_lin, out_const, workspace)
struct MidNote {
    const double *A; int64_t lda, rows, cols; const double *b; const int64_t *xvar, *varmap;
    const void *out_quad, *out_csc, *out_lin, *out_const, *workspace; size_t workspace_bytes;
};
int dispatch_mid(void *stream, Launch launch, const MidNote &note);
// the riders of one node: at most this many packs, of at most this many algorithmic bytes (32 per entry) in all — a persistent workgroup
// is one workgroup per CU where the stand-alone pack runs eight, so a pack much larger than the node's idle tail is faster alone
#ifndef PMT_MID_RIDER_MB
#define PMT_MID_RIDER_MB 256       // measured: profiles/r15_gram_riders.txt, section 5 (a measurement build raises it)
#endif
constexpr int MID_MAX_RIDERS = 8;
constexpr int64_t PMT_MID_RIDER_BYTES = (int64_t)PMT_MID_RIDER_MB << 20;
int launch_gram_mid_constant(const double *b, int sign, int64_t rows, double *out_const, hipStream_t s);
int check_strictly_increasing(const int64_t *xvar_dev, int64_t n, void *stream);
void mark_no_graph(void *stream);
int launch_blocked_dot(const double *a, int sign_a, const double *b, int sign_b, int64_t n, double *scratch, double *out, hipStream_t s, int chained);
size_t blocked_dot_scratch_doubles();
int launch_small_one(const SmallNode &nd, hipStream_t s);

}  // namespace pmt
