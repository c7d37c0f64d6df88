// Canonical least-squares objective: canonicalize!(residual . residual) for residual = A*x (+|-) b, fused with
// the MOI copy.  out_quad = upper triangle (row-major) of 2*A'A as QuadraticTerms, out_lin = 2*A'c, out_const = c'c
// (SURVEY.md Appendix A.3).  The only arithmetic-heavy node of the path: r*n*(n+1) fp64 FLOP -> f64 MFMA.
//
// Reference semantics replaced: _vecdot!/muladd! literal expansion (src/functions.jl:702-709,548-576) followed by
// canonicalize! (src/functions.jl:381-386, sort_and_combine! src/util.jl:9-26) and
// update!(::MOI.ScalarQuadraticFunction, ...) (src/moi_interop.jl:45-62).  The reference sums duplicates in
// QuickSort order; here the contraction index runs in row order inside v_mfma_f64_4x4x4_4b_f64 — coefficients
// agree to rounding (tests: <= 1e-12 relative), indices exactly.
//
// This file holds the node: validation, the choice of its form (gram_form: the contraction itself is gram_tall.hip's, gram_mid.hip's or
// gram_sk.hip's), the stream-K form's two small reductions (q = 2 A'c, c'c) on a side stream, the host delivery, the C-ABI entry points.
#include <algorithm>
#include <memory>
#include <vector>

#include "streams.h"

#ifndef PMT_GRAM_ABL_NO_LINEAR
#define PMT_GRAM_ABL_NO_LINEAR 0   // ablation (wrong q): the stream-K form without its affine part on the side stream — what folding q into the contraction could gain at most
#endif

namespace pmt {

constexpr size_t PAIR_FLAG_BYTES = 4096;      // 4 bytes per tile of a stage (at most 512 workgroups / 2 tiles)
// a CSC delivery computes the tiles column band by column band (super-columns of ONE tile column: a band's completion is never held back by
// its neighbour's, so the stages complete nearly equal byte counts — 1.73 vs 1.77 ms per solve with super-columns of two at n = 4096,
// profiles/r04_host_delivery.txt), walked from the LAST band to the first (order_w < 0): the column bands finish in descending order.  Band kb holds (kb + 1) tiles' worth of values, so the long bands leave while the contraction is
// still busy and what is left to ship when it ends — the tail nothing overlaps — is the short ones (ascending order, round 3, left 8.1 MB
// = 0.15 ms of PCIe behind the last stage at n = 4096; descending leaves 1 MB).
constexpr int DELIVER_ORDER_W = 1;

// out_lin[j] = (2 * sum_i c_i * A[i,j], vm[xvar[j]]),  c_i = 0.0 (+|-) b[i]; one wave per column (coalesced along i)
__global__ __launch_bounds__(256) void gram_linear_kernel(const double *__restrict__ A, int64_t lda, int64_t rows, int64_t cols,
                                                          const int64_t *__restrict__ xvar, const double *__restrict__ b, int sign,
                                                          int moi, const int64_t *__restrict__ varmap, LT *__restrict__ out_lin) {
    const int64_t col = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= cols) return;
    const int lane = threadIdx.x & 63;
    const double *a = A + col * lda;
    double acc = 0.0;
    if (b && sign)
        for (int64_t i = lane; i < rows; i += 64) acc += signed_const(b[i], sign) * a[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) {
        LT t;
        t.coeff = 2 * acc;
        const int64_t v = xvar[col];
        t.var = moi ? map_var(varmap, v) : v;
        out_lin[col] = t;
    }
}

// Tall matrices (rows >> cols): one wave per column leaves most of the chip idle (cols = 128: 128 waves read 1 GB) — the rows are cut
// into `nsplit` chunks, one wave per (column, chunk), and the chunk sums of a column are added in chunk order (deterministic).
__global__ __launch_bounds__(256) void gram_linear_split_kernel(const double *__restrict__ A, int64_t lda, int64_t rows, int64_t cols,
                                                                const double *__restrict__ b, int sign, int64_t chunk,
                                                                double *__restrict__ partial) {
    const int64_t col = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= cols) return;
    const int lane = threadIdx.x & 63;
    const int64_t i0 = (int64_t)blockIdx.y * chunk;
    const int len = (int)(min(rows, i0 + chunk) - i0);                   // 32-bit loop state: 16 VGPRs, co-resident with the contraction
    const double *a = A + col * lda + i0, *bb = b + i0;
    double acc = 0.0;
    for (int i = lane; i < len; i += 64) acc += signed_const(bb[i], sign) * a[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) partial[(int64_t)blockIdx.y * cols + col] = acc;
}

__global__ __launch_bounds__(256) void gram_linear_finish_kernel(const double *__restrict__ partial, int nsplit, int64_t cols,
                                                                 const int64_t *__restrict__ xvar, int moi, const int64_t *__restrict__ varmap,
                                                                 LT *__restrict__ out_lin) {
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= cols) return;
    double acc = 0.0;
    for (int k = 0; k < nsplit; ++k) acc += partial[(int64_t)k * cols + col];
    LT t;
    t.coeff = 2 * acc;
    const int64_t v = xvar[col];
    t.var = moi ? map_var(varmap, v) : v;
    out_lin[col] = t;
}

constexpr int64_t LIN_CHUNK_MIN = 4096;      // rows per (column, chunk) wave at least: 64 iterations of 64 lanes
constexpr int64_t LIN_WAVES = 8192;          // waves that fill the chip (256 CUs x 32)
// The constant c'c of the stream-K node: sequential (the reference's left-to-right sum, src/functions.jl:574, bit for bit) or 2048 chains.
// The sequential chain runs on one wave beside the contraction at ~0.07 us per row (0.287 ms at r = 4096, profiles/r04_c2_rocprofv3_kernel_stats.csv);
// the contraction takes T(r) = 0.096 + 0.276 r / 1024 ms at n = 4096 (528 tiles), in proportion to the tile count
// elsewhere.  The chain is kept where the contraction hides it (config 2: 0.29 of 1.19 ms); where it would be half of the node or more
// (few columns) the chained form takes over, as it always does above 8192 rows.  Bit-exactness of the constant is not part of the
// parity bar (1e-12 relative); the order is fixed either way and reported by pmt_quad_gram_constant_order.
static bool constant_chained(int64_t rows, int64_t cols) {
    if (rows > 8192) return true;
    if (rows < 2048) return false;
    const double nt = (double)cdiv(std::max<int64_t>(cols, 1), ST);
    const double contraction_ms = (0.096 + 0.276 * (double)rows / 1024.0) * (nt * (nt + 1) / 2) / 528.0;
    return 0.07e-3 * (double)rows > 0.5 * contraction_ms;
}

// WIDE shapes of up to 2048 columns that the one-launch form on 64 x 64 tiles takes (gram_mid.hip; round 6b/6c): the sizes the reference is
// used at with a few hundred variables, and most of what used to be the four launches tall + fix-up + strict stream-K + fix-up.  Same-box node
// times in us, four launches -> one (profiles/r06_gram_mid.txt): 300 x 300 35.7 -> 16, 40 x 520 46 -> 10, 1024 x 512 44 -> 21, 4096 x 512
// 62 -> 33.6, 4096 x 1024 128 -> 98, 8192 x 512 90 -> 50.5, 2048 x 1280 127 -> 71, 65536 x 512 411 -> 304, 65536 x 1024 1380 -> 1189,
// 262144 x 512 1387 -> 1282, 100000 x 129 188 -> 103.  Up to 128 columns the one-tile kernel of gram_tall.hip stays (three 64 x 64 tiles
// split 80 ways fold too much: 8192 x 128 18 -> 40 us).
#ifndef PMT_MID_MAXCOLS
#define PMT_MID_MAXCOLS 2048
#endif
#ifndef PMT_MID_BIGCOLS
#define PMT_MID_BIGCOLS 4096
#endif
#ifndef PMT_MID_BIGEL
#define PMT_MID_BIGEL ((int64_t)1 << 29)      // (the fast load path needs the matrix within 4 GiB)
#endif
// 2049 .. 4096 columns (config 2), round 6c: with the pinned instruction stream, the tiles in super-tile order and the partial round / the
// diagonal tiles split (gram_mid.hip: mid_plan) the one launch beats the stream-K node (contraction + fix-up, q and the constant on a side
// stream) at every row count measured — 4096 x 4096 1205 -> 1069-1092 us (0.73 -> 0.80-0.82 of the f64 matrix peak), 2048 x 4096 661 -> 573,
// 4096 x 3072 718 -> 630, 4096 x 2304 461 -> 373, 8192 x 2560 1065 -> 839, 1000 x 3000 246 -> 191, 8192 x 4096 2340 -> 2062, 16384 x 4096
// 4616 -> 4405, 32768 x 3072 5338 -> 4863, 131072 x 2560 17877 -> 15256, 20000 x 3500 4878 -> 3859; 65536 x 4096 18287 -> 18444 is a tie.  A
// STAGED host delivery of such a shape (config 2's host_csc hand-off: column bands leave while the contraction runs) keeps the stream-K
// kernel — run_quad_gram — with the constant in this form's order, so that pmt_quad_gram_constant_order holds for every call form.
static bool gram_mid_big(int64_t rows, int64_t cols) {
#ifdef PMT_NO_MID
    return false;
#endif
    return cols > 16 * 128 && cols <= PMT_MID_BIGCOLS && rows >= 1 && rows * cols < PMT_MID_BIGEL;
}
static bool gram_mid_applies(int64_t rows, int64_t cols) {
#ifdef PMT_NO_MID
    return false;
#endif
    if (gram_mid_big(rows, cols)) return true;
    if (!gram_tall_diag_applies(rows, cols) || cols > PMT_MID_MAXCOLS) return false;
    // Measured with the pinned instruction stream of round 6c (gram_mid.hip: mid_step), one launch against four, us (profiles/r06_gram_mid.txt):
    //   wins   200000 x 224 287 (330), 230000 x 256 354 (381), 150000 x 288 304 (459), 160000 x 320 326 (498), 131072 x 384 358 (460),
    //          100000 x 448 375 (554), 262144 x 512 1282 (1387), 524288 x 512 2527 (2680), 2^20 x 384 2991 (3188), 4096 x 2048 359 (381),
    //          16384 x 2048 1190 (1338), 131072 x 1024 2453 (2640), 262144 x 1024 4980 (5240)
    //   loses  380000 x 129 578 (505), 300000 x 160 462 (422), 250000 x 192 389 (366), 262144 x 256 407 (386), 786432 x 320 2317 (2224)
    // (every 64-column panel is read once per tile of its row and column: few, narrow panels out of HBM are the four launches' shapes).  The
    // fast load path needs the matrix within 4 GiB: below 2^29 elements.
    const int64_t el = rows * cols;
    if (cols <= 192) return el <= ((int64_t)1 << 25);
    if (cols < 320) return el < ((int64_t)1 << 26);
    if (cols < 384) return el <= ((int64_t)1 << 27);
    return el < ((int64_t)1 << 29);
}

static int linear_splits(int64_t rows, int64_t cols) {
    if (cols <= 0) return 1;
    return (int)std::max<int64_t>(1, std::min(cdiv(LIN_WAVES, cols), rows / LIN_CHUNK_MIN));
}

// The form of the node, decided here and nowhere else (the measured thresholds are at the predicates):
//   Tiny           a plain call (no CSC values, no delivery) of a tiny shape (gram_tiny): a node of the small-plan interpreter (small.hip)
//   Mid            2049 .. 4096 columns unless delivered (gram_mid_big), the wide shapes of gram_mid_applies: one launch (gram_mid.hip)
//   Fused          the rest of up to 2048 columns: gram_tall.hip's diagonal tiles, q and c'c in one pass, then the strict stream-K launch
//   StreamKStaged  a delivered call of any other shape: the stream-K contraction in stages, its column bands shipped while it runs
//   StreamK        everything else, cols == 0 included: the stream-K contraction (gram_sk.hip), q and c'c on a side stream
enum class GramForm { Tiny, Fused, Mid, StreamK, StreamKStaged };
static GramForm gram_form(int64_t rows, int64_t cols, bool csc, bool deliver) {
    if (!deliver && !csc && gram_tiny(rows, cols)) return GramForm::Tiny;
    const bool big = gram_mid_big(rows, cols);
    if ((big && !deliver) || (!big && gram_mid_applies(rows, cols))) return GramForm::Mid;
    if (gram_tall_applies(rows, cols) || gram_tall_diag_applies(rows, cols)) return GramForm::Fused;
    return deliver && cols > 0 ? GramForm::StreamKStaged : GramForm::StreamK;         // (no predicate holds for cols <= 0)
}

// the summation order of c'c a form gives (include/parametron_hip.h: pmt_quad_gram_constant_order; a tiny node's is row order, order 0)
struct ConstantOrder { int order, groups, stage_rows; };
static ConstantOrder constant_order(GramForm form, int64_t rows, int64_t cols) {
    if (form == GramForm::Fused) {
        const int lanes = gram_tall_run_lanes(rows, cols);
        return {lanes == 4 ? 4 : lanes == 16 ? 3 : 2, gram_tall_groups(rows, cols), gram_tall_stage_rows(rows, cols)};
    }
    // the one-launch form's 512 strided chains — also in the staged delivery of a shape that form takes otherwise: every call form agrees
    if (form == GramForm::Mid || (form == GramForm::StreamKStaged && gram_form(rows, cols, true, false) == GramForm::Mid)) return {5, 1, 512};
    return constant_chained(rows, cols) ? ConstantOrder{1, 2048, 0} : ConstantOrder{0, 1, 0};
}

// the signals of one recorded delivery: a dependency signal per band group (a one-thread kernel behind the stage that completes the group
// stores 0 into its value when the group is in memory) and one completion signal that counts the groups' transfers down; `engine`: this
// launch's transfers go through the copy engine (else through the courier kernel on the fetch stream)
struct DeliverSignals {
    dma::Engine *eng = nullptr;
    dma::Signal dep[MAXGROUPS], done;
    int n = 0;
    bool tried = false, pending = false, engine = false;
    ~DeliverSignals() {
        for (int i = 0; eng && i < n; ++i) dma::signal_destroy(eng, dep[i]);
        if (eng) dma::signal_destroy(eng, done);
    }
};

// Host delivery of the CSC values or the terms.  StreamKStaged: the contraction runs in STAGES, each a launch over a range of the tile sequence
// and its fix-up; a stage that completes bands ends with a one-thread kernel that releases their transfer.  Fused and Mid: ONE transfer of
// the whole array behind the node's last kernel — staging pays for hundreds of megabytes (config 2), not for the <= 50 MB of these shapes.
struct DeliverPlan {
    double *host = nullptr;                 // page-locked destination, same layout as the delivered array
    double *host_dev = nullptr;             // ... and its device-visible address
    const double *src = nullptr;            // the delivered array, as doubles: out_csc, or out_quad (three doubles per term)
    std::shared_ptr<DeliverSignals> sig;    // lives as long as the recorded call
    int order_w = 0, nstages = 0;           // the stages' tile order (launch_gram_sk) and count
    int64_t seq_begin[MAXGROUPS], seq_count[MAXGROUPS];
    int group_of[MAXGROUPS];                // index of the band group the stage completes, or -1
    int ngroups = 0;
    int64_t gbeg[MAXGROUPS], gend[MAXGROUPS];      // the groups' ranges of the delivered array (doubles)
};

// Stage size.  With the persistent grid all workgroups finish a round of whole tiles together, so one launch of everything delivers in two
// bursts (at n = r = 4096: nothing for 0.6 ms, half of P then, the rest at the end: 1.95 ms per solve).  Stages of HALF a grid's worth of
// tiles — every tile split in two along the contraction, stream-K over all workgroups, partial sums added by the fix-up launch — complete
// a quarter of P every 0.3 ms, which is also what PCIe takes to ship it: the copy engine stays busy from the first stage on.  The split
// costs ~15 % of contraction time (partial tiles through the workspace, 3 launches per stage; profiles/r03_host_delivery.txt) and changes
// the summation order of a split tile (two half sums added) — within the stated tolerance, deterministic, and the delivered host array is
// the device array of the same run bit for bit.  `nstages_hint` (the entry point's ngroups) > 0 overrides the number of stages.
// quad: the delivered array is out_quad (24-byte terms, ROW-major upper triangle): tile order 0 (super-rows of four tile rows, sk_seq_unrank), the
// groups are row bands and the offsets count doubles (three per term); else out_csc (column bands, super-columns of DELIVER_ORDER_W).
static DeliverPlan deliver_plan(int64_t rows, int64_t cols, bool staged, int nstages_hint, bool quad) {
    DeliverPlan d;
#ifdef PMT_TUNING
    static const int order_w = [] { const char *e = getenv("PMT_DELIVER_ORDER_W"); return e ? atoi(e) : DELIVER_ORDER_W; }();
#else
    constexpr int order_w = DELIVER_ORDER_W;
#endif
    d.order_w = quad ? 0 : -order_w;
    const int nt = (int)cdiv(cols, ST);
    const int64_t T = (int64_t)nt * (nt + 1) / 2;
    const int64_t nchunk = std::max<int64_t>(1, cdiv(rows, 256));
    const int64_t G = std::min<int64_t>(T * nchunk, 256);                  // as launch_gram_sk (gram_sk.hip)
    int64_t per = nchunk >= 2 ? std::max<int64_t>(1, G / 2) : G;           // tiles per stage: half a grid's worth (whole tiles if there is nothing to split)
    if (nstages_hint > 0) per = std::max<int64_t>(1, cdiv(T, std::min(nstages_hint, MAXGROUPS)));
    if (cdiv(T, per) > MAXGROUPS) per = cdiv(T, MAXGROUPS);
    if (!staged) per = T;               // (one stage that completes every band: one group, the whole array)
    // position in the walk after which each band is complete, and the band's range of the delivered array
    std::vector<int64_t> seq_end_of_band((size_t)nt), bandbeg((size_t)nt), bandend((size_t)nt);
    int64_t seq_end = 0;
    if (quad) {
        // row bands, ascending (row band jb holds nt - jb tiles: the short ones come last by themselves)
        for (int j0 = 0; j0 < nt; j0 += 4) {
            const int h = std::min(4, nt - j0), W = nt - j0;
            seq_end += (int64_t)h * (h + 1) / 2 + (int64_t)(W - h) * h;    // (sk_seq_unrank)
            for (int jb = j0; jb < j0 + h; ++jb) seq_end_of_band[(size_t)jb] = seq_end;
        }
        for (int jb = 0; jb < nt; ++jb) {
            const int64_t J0 = (int64_t)jb * ST, J = std::min<int64_t>(cols, (int64_t)(jb + 1) * ST);
            bandbeg[(size_t)jb] = 3 * (J0 * cols - J0 * (J0 - 1) / 2);      // rows 0 .. J-1 of the row-major upper triangle, 3 doubles per term
            bandend[(size_t)jb] = 3 * (J * cols - J * (J - 1) / 2);
        }
    } else {
        // column bands, DESCENDING: the walk starts at the end of the column-band-major sequence (sk_colseq_unrank, launch_gram_sk order_w < 0)
        std::vector<int64_t> start_of_super((size_t)nt);
        int64_t pos = 0;
        for (int c0 = 0; c0 < nt; c0 += order_w) {
            const int h = std::min(order_w, nt - c0);
            for (int kb = c0; kb < c0 + h; ++kb) start_of_super[(size_t)kb] = pos;
            pos += (int64_t)c0 * h + (int64_t)h * (h + 1) / 2;
        }
        for (int kb = 0; kb < nt; ++kb) {
            seq_end_of_band[(size_t)kb] = T - start_of_super[(size_t)kb];     // the walk has passed the band's whole super-column
            const int64_t c0 = (int64_t)kb * ST, cend = std::min<int64_t>(cols, (int64_t)(kb + 1) * ST);
            bandbeg[(size_t)kb] = c0 * (c0 + 1) / 2;
            bandend[(size_t)kb] = cend * (cend + 1) / 2;
        }
    }
    // bands in completion order: 0, 1, .. (quad) or nt-1, nt-2, .. (CSC)
    auto band_at = [&](int i) { return quad ? i : nt - 1 - i; };
    int done_bands = 0;
    for (int64_t t0 = 0; t0 < T; t0 += per) {
        const int st = d.nstages++;
        d.seq_begin[st] = t0;
        d.seq_count[st] = std::min<int64_t>(per, T - t0);
        int nb = done_bands;
        while (nb < nt && seq_end_of_band[(size_t)band_at(nb)] <= t0 + d.seq_count[st]) ++nb;
        d.group_of[st] = -1;
        if (nb > done_bands) {
            d.group_of[st] = d.ngroups;
            const int first = band_at(done_bands), last = band_at(nb - 1);
            d.gbeg[d.ngroups] = bandbeg[(size_t)std::min(first, last)];
            d.gend[d.ngroups] = bandend[(size_t)std::max(first, last)];
            ++d.ngroups;
            done_bands = nb;
        }
    }
    return d;
}

struct GramArgs {          // the operands of one node
    const double *A; int64_t lda, rows, cols; const int64_t *xvar; const double *b; int sign, moi; const int64_t *varmap;
    pmt_quadratic_term *out_quad; double *out_csc; double alpha; pmt_linear_term *out_lin; double *out_const; void *workspace;
};

// before the node's kernels: the previous delivery of this call has read its array, and this launch's transfers are armed
static int deliver_arm(const DeliverPlan &d, SideStream *side, hipStream_t s) {
    PMT_REQUIRE(side && side->counters, PMT_STATE_ERROR, "quad_gram_csc_deliver: no auxiliary streams for this stream");
    DeliverSignals *sig = d.sig.get();
    // Preferred: one copy-engine transfer per band group, each started by the signal set behind the group's stage (hsadma.hip)
    const int mode = dma::delivery_mode();
    // the previous delivery of this entry must have read its array before this contraction overwrites it (whichever way it went)
    if (sig->pending) { if (int rc = dma::wait(sig->eng, sig->done, 10.0)) return rc; sig->pending = false; }
    // an immediate (unrecorded) call owns fresh signals: what earlier calls on this stream handed to the engine is awaited here
    if (!side->in_replay) { if (int rc = wait_dma_pending(side)) return rc; }
    if (mode != 2 && !sig->tried) {
        sig->tried = true;
        dma::Engine *eng = dma::get(side->device);
        bool ok = eng && dma::signal_create(eng, 0, &sig->done) == PMT_OK;
        for (int i = 0; ok && i < d.ngroups; ++i) { ok = dma::signal_create(eng, 1, &sig->dep[i]) == PMT_OK; if (ok) sig->n = i + 1; }
        if (ok) sig->eng = eng;
    }
    sig->engine = mode != 2 && sig->eng != nullptr;
    PMT_REQUIRE(mode != 1 || sig->engine, PMT_STATE_ERROR, "host delivery: the copy engine was demanded (pmt_set_host_delivery(1)) but is not available");
    // (what went through the fetch stream before — a previous delivery by the courier, a recorded fetch — is ordered by its event)
    if (side->fetch_pending) { PMT_HIP_CHECK(hipStreamWaitEvent(s, side->fetch_done, 0)); side->fetch_pending = false; }
    if (!sig->engine) return ensure_fetch_stream(side);
    for (int i = 0; i < d.ngroups; ++i) dma::signal_set(sig->eng, sig->dep[i], 1);
    dma::signal_set(sig->eng, sig->done, d.ngroups);
    return PMT_OK;
}

// behind the kernel that completes band group `grp`, one thread stores 0 into the word the group's transfer waits for: the value of its
// dependency signal (copy engine, hsadma.hip) or the courier's flag (deliver.hip)
static int release_group(const DeliverPlan &d, SideStream *side, int grp, hipStream_t s) {
    const dma::Signal flag{0, reinterpret_cast<int64_t *>(static_cast<char *>(side->counters) + FLAGS_OFFSET) + grp};
    return dma::launch_signal_store(d.sig->engine ? d.sig->dep[grp] : flag, s);
}

// behind the node's kernels: hand the groups' transfers over
static int deliver_submit(const DeliverPlan &d, SideStream *side) {
    if (!d.sig->engine) {
        // fallback, fetch stream: ONE courier launch, queued now that the contraction's workgroups are on their way; it polls the
        // band groups' flags and stores each finished group straight into the host array (deliver.hip)
        char *cb = static_cast<char *>(side->counters);
        if (int rc = launch_courier(d.src, d.host_dev, reinterpret_cast<long long *>(cb + FLAGS_OFFSET), reinterpret_cast<unsigned *>(cb + DONE_OFFSET),
                                    side->err_dev, d.ngroups, d.gbeg, d.gend, side->fetch)) return rc;
        PMT_HIP_CHECK(hipEventRecord(side->fetch_done, side->fetch));
        side->fetch_pending = true;
        return PMT_OK;
    }
    // The engine works through its queue in submission order.  Inside a plan's replay the groups' transfers are therefore submitted at
    // the END of the replay, behind the recorded fetches of the tape (q, A's values, bounds: ready within the first tenth of the
    // contraction) — submitted here they would hold those back until the last band group has left.
    auto submit = [p = d]() -> int {
        for (int i = 0; i < p.ngroups; ++i)
            if (int rc = dma::copy_to_host(p.sig->eng, p.host + p.gbeg[i], p.src + p.gbeg[i], sizeof(double) * (size_t)(p.gend[i] - p.gbeg[i]),
                                           &p.sig->dep[i], p.sig->done, 1)) return rc;
        return PMT_OK;
    };
    d.sig->pending = true;
    side->dma_pending.emplace_back(d.sig->eng, d.sig->done);
    side->keepalive.push_back(d.sig);
    if (!side->in_replay) return submit();
    side->deferred.push_back(submit);
    return PMT_OK;
}

// the side stream waits for what `s` has queued so far — also for a plan's side-lane entries behind a fused or one-launch node, which may
// read its AFFINE part (the hand-off's q gather; plan.hip `replay`) as they would behind the stream-K form's gram_linear
static int fork_side(SideStream *side, hipStream_t s) {
    PMT_HIP_CHECK(hipEventRecord(side->fork, s));
    PMT_HIP_CHECK(hipStreamWaitEvent(side->stream, side->fork, 0));
    return PMT_OK;
}
// ... which a fused or one-launch node needs only in a replay that puts work on the side stream (SideStream::side_work).  In a tape of
// lane-0 entries alone (config 2: the node, then the constraint pack) the event behind the node orders nothing, and the runtime still
// holds the next launch on `s` back for it: 7.5 us between the node and the pack (profiles/r14_item_boundaries.txt)
static bool forks_in_replay(const SideStream *side) { return side && side->in_replay && side->side_work; }

// Fused: the diagonal tiles, q and c'c in ONE pass over A (gram_tall.hip), then the strictly upper tiles in ONE ranged launch of the stream-K
// kernel (SKArgs::strict; the partials of both share the workspace in stream order) — no side stream, no separate reductions
static int fused_node(const GramArgs &g, SideStream *side, hipStream_t s) {
    int rc = launch_gram_tall(g.A, g.lda, g.rows, g.cols, g.xvar, g.b, g.sign, g.moi, g.varmap, g.out_quad, g.out_csc, g.alpha, g.out_lin,
                              g.out_const, g.workspace, s);
    if (!rc && forks_in_replay(side)) rc = fork_side(side, s);          // (the strictly upper tiles then run beside those entries)
    const int64_t nt = cdiv(g.cols, ST);
    if (!rc && nt > 1)
        rc = launch_gram_sk(g.A, g.lda, g.rows, g.cols, g.xvar, g.varmap, g.moi, g.out_quad, g.out_csc, g.alpha, g.workspace, 0, 0, nt * (nt - 1) / 2,
                            nullptr, 0, nullptr, s, 1);
    return rc;
}

// Mid: every tile, q and c'c in ONE launch on 64 x 64 tiles (gram_mid.hip); the per-tile arrival counts are the calling stream's
static int mid_node(const GramArgs &g, SideStream *side, hipStream_t s) {
    PMT_REQUIRE(side && side->counters && (size_t)gram_mid_counters(g.cols) * sizeof(unsigned) <= MID_COUNTER_BYTES, PMT_STATE_ERROR,
                "quad_gram: no auxiliary state for this stream");
    int rc = launch_gram_mid(g.A, g.lda, g.rows, g.cols, g.xvar, g.b, g.sign, g.moi, g.varmap, g.out_quad, g.out_csc, g.alpha, g.out_lin,
                             g.out_const, g.workspace, reinterpret_cast<unsigned *>(static_cast<char *>(side->counters) + MID_OFFSET),
                             side->mid_riders, side->mid_nriders, side->mid_rider_tiles, s);
    return !rc && forks_in_replay(side) ? fork_side(side, s) : rc;
}

// StreamK: the contraction on `s`, q = 2 A'c and c'c on the side stream; staged: stage by stage (deliver_plan), releasing band groups
static int stream_k_node(const GramArgs &g, bool staged, const DeliverPlan &d, SideStream *side, hipStream_t s) {
    // fork: the two small reductions of this node (q = 2 A'c, HBM-bound; c'c, a serial chain) run on a side stream while
    // the MFMA-bound contraction owns the main stream; join before returning control of `s`.  Legal under stream capture.
    hipStream_t s2 = side ? side->stream : s;
    if (side) { if (int rc = fork_side(side, s)) return rc; }
    if (side && side->in_replay) side->side_work = true;          // (a fused or one-launch node later in the tape forks as before)
    const int64_t rows = g.rows, cols = g.cols;
    int rc = PMT_OK;
    double *scratch = g.workspace ? reinterpret_cast<double *>(static_cast<char *>(g.workspace) + gram_sk_workspace_bytes(rows, cols)) : nullptr;
    const int nsplit = (scratch && g.b && g.sign) ? linear_splits(rows, cols) : 1;
    if (PMT_GRAM_ABL_NO_LINEAR) {
    } else if (cols > 0 && nsplit > 1) {
        const int64_t chunk = 64 * cdiv(cdiv(rows, nsplit), 64);
        PMT_LAUNCH(gram_linear_split_kernel, dim3((unsigned)cdiv(cols, 4), (unsigned)nsplit), dim3(256), 0, s2, g.A, g.lda, rows, cols, g.b, g.sign, chunk, scratch);
        PMT_LAUNCH(gram_linear_finish_kernel, dim3((unsigned)cdiv(cols, 256)), dim3(256), 0, s2, scratch, nsplit, cols, g.xvar, g.moi, g.varmap, g.out_lin);
        rc = check_launch("gram_linear_split_kernel");
    } else if (cols > 0) {
        PMT_LAUNCH(gram_linear_kernel, dim3((unsigned)cdiv(cols, 4)), dim3(256), 0, s2, g.A, g.lda, rows, cols, g.xvar, g.b, g.sign, g.moi, g.varmap, g.out_lin);
        rc = check_launch("gram_linear_kernel");
    }
    // c'c: a serial chain of `rows` additions on ONE wave (bit for bit the reference's left-to-right sum) — ~50 us alone, ~0.3 ms beside
    // the contraction.  Inside a plan's replay it is queued at the END of the replay, i.e. behind the tape's side-lane entries on the
    // side stream (the MOI copies of the constraints, the hand-off gathers and their fetches), which used to wait for it.
    double *chains = scratch ? scratch + (size_t)linear_splits(rows, cols) * (size_t)cols : nullptr;
    const int order = constant_order(staged ? GramForm::StreamKStaged : GramForm::StreamK, rows, cols).order;
    auto const_part = [=]() -> int {
        int rc2 = PMT_OK;
        if (order == 5) rc2 = launch_gram_mid_constant(g.b, g.sign, rows, g.out_const, s2);      // (a staged delivery: the one-launch form's order)
        else if (g.b && g.sign && rows > 0) rc2 = launch_blocked_dot(g.b, g.sign, g.b, g.sign, rows, chains, g.out_const, s2, order);
        else if (hipMemsetAsync(g.out_const, 0, sizeof(double), s2) != hipSuccess) rc2 = fail(PMT_HIP_ERROR, "hipMemsetAsync(out_const)");
        if (side) { PMT_HIP_CHECK(hipEventRecord(side->join2, side->stream)); PMT_HIP_CHECK(hipStreamWaitEvent(s, side->join2, 0)); }
        return rc2;
    };
    const bool defer_const = side && side->in_replay;
    if (!rc && defer_const) side->deferred.push_back(const_part);
    if (side) PMT_HIP_CHECK(hipEventRecord(side->join, side->stream));          // the affine part: `s` joins it behind the contraction's launch
    if (!rc && cols > 0 && !staged) rc = launch_gram_sk(g.A, g.lda, rows, cols, g.xvar, g.varmap, g.moi, g.out_quad, g.out_csc, g.alpha, g.workspace, 0, 0, -1,
                                                        nullptr, 0, nullptr, s);
    else if (!rc && cols > 0) {
        // flags of the pair fold (gram_sk.hip): the tail of the partial-tile workspace, beyond the slots a grid of 256 uses; cleared
        // per delivery, stage st writes / waits for the value st + 1
        unsigned *pair_flags = g.workspace ? reinterpret_cast<unsigned *>(static_cast<char *>(g.workspace) + gram_sk_workspace_bytes(rows, cols) - PAIR_FLAG_BYTES) : nullptr;
        if (pair_flags) PMT_HIP_CHECK(hipMemsetAsync(pair_flags, 0, PAIR_FLAG_BYTES, s));
        for (int st = 0; !rc && st < d.nstages; ++st) {
            rc = launch_gram_sk(g.A, g.lda, rows, cols, g.xvar, g.varmap, g.moi, g.out_quad, g.out_csc, g.alpha, g.workspace, d.order_w, d.seq_begin[st],
                                d.seq_count[st], pair_flags, (unsigned)(st + 1), side->err_dev, s);
            if (!rc && d.group_of[st] >= 0) rc = release_group(d, side, d.group_of[st], s);
        }
        if (!rc) rc = deliver_submit(d, side);
    }
    if (side) PMT_HIP_CHECK(hipStreamWaitEvent(s, side->join, 0));
    if (!rc && !defer_const) rc = const_part();          // (behind the contraction's launch: its workgroups are placed first)
    return rc;
}

// the whole node, in the form gram_form picks.  out_quad (term structs) and out_csc (solver values, alpha-scaled) are independent optional
// outputs of the same contraction; host != null: out_csc, or out_quad where there is no out_csc, is also DELIVERED to this page-locked buffer.
static int gram_node(const GramArgs &g, void *stream, double *host = nullptr, int ngroups = 0) {
    const int64_t rows = g.rows, cols = g.cols;
    PMT_REQUIRE(rows >= 0 && cols >= 0, PMT_DIMENSION_MISMATCH, "quad_gram: negative dimension");
    PMT_REQUIRE(g.lda >= rows, PMT_DIMENSION_MISMATCH, "quad_gram: lda < rows");
    PMT_REQUIRE(g.sign >= -1 && g.sign <= 1, PMT_INVALID_ARGUMENT, "quad_gram: sign must be -1, 0 or +1");
    PMT_REQUIRE(g.out_const, PMT_INVALID_ARGUMENT, "quad_gram: null out_const");
    PMT_REQUIRE(g.sign == 0 || g.b || rows == 0, PMT_INVALID_ARGUMENT, "quad_gram: sign != 0 needs b");
    if (cols > 0) PMT_REQUIRE(g.xvar && (g.out_quad || g.out_csc) && g.out_lin && (g.A || rows == 0), PMT_INVALID_ARGUMENT, "quad_gram: null pointer");
    PMT_REQUIRE(cols < (int64_t)ST * 32000, PMT_DIMENSION_MISMATCH, "quad_gram: too many columns");
    const GramForm form = gram_form(rows, cols, g.out_csc != nullptr, host != nullptr);
    PMT_REQUIRE(g.workspace || (form != GramForm::Fused && form != GramForm::Mid), PMT_INVALID_ARGUMENT, "quad_gram: workspace required");
    if (int rc = check_strictly_increasing(g.xvar, cols, stream)) return rc;
    if (form == GramForm::Tiny) {
        // (README Example 1 with the canonical objective: 8 x 8) row-order sums by the interpreter kernel; by itself — an immediate call, or
        // a run of one — the node is ONE launch of the interpreter's body: the same bits as inside a run
        SmallNode nd;
        nd.op = SOP_GRAM; nd.sign = (g.b && g.sign) ? g.sign : 0; nd.moi = g.moi; nd.d[0] = g.lda; nd.d[1] = rows; nd.d[2] = cols;
        nd.in[0] = g.A; nd.in[1] = g.xvar; nd.in[2] = g.b; nd.in[3] = g.varmap; nd.out[0] = g.out_quad; nd.out[1] = g.out_lin; nd.out[2] = g.out_const;
        nd.work = rows * cols * (cols + 1) / 2 + 64 * rows;
        return dispatch(stream, [=](hipStream_t s) { return launch_small_one(nd, s); }, nd);
    }
    DeliverPlan dplan;
    if (host && cols > 0) {
        dplan = deliver_plan(rows, cols, form == GramForm::StreamKStaged, ngroups, !g.out_csc);
        dplan.host = host;
        dplan.src = g.out_csc ? g.out_csc : reinterpret_cast<const double *>(g.out_quad);
        dplan.host_dev = static_cast<double *>(host_device_pointer(host));
        PMT_REQUIRE(dplan.host_dev, PMT_INVALID_ARGUMENT, "quad_gram_csc_deliver: host_P_values must be page-locked host memory (pmt_host_alloc)");
        dplan.sig = std::make_shared<DeliverSignals>();
        mark_no_graph(stream);
    }
    Launch node = [=](hipStream_t s) -> int {
        SideStream *side = side_stream(s);
        const bool deliver = dplan.host != nullptr;
        if (deliver) { if (int rc = deliver_arm(dplan, side, s)) return rc; }
        if (form == GramForm::StreamK || form == GramForm::StreamKStaged) return stream_k_node(g, form == GramForm::StreamKStaged, dplan, side, s);
        int rc = form == GramForm::Fused ? fused_node(g, side, s) : mid_node(g, side, s);
        // the whole array is in memory behind the node's last kernel: release its one transfer
        if (!rc && deliver) rc = release_group(dplan, side, 0, s);
        if (!rc && deliver) rc = deliver_submit(dplan, side);
        return rc;
    };
    // a recorded one-launch node that delivers nothing: the plan may let constraint packs ride in it (plan.hip)
    if (form == GramForm::Mid && !host && cols > 0)
        return dispatch_mid(stream, std::move(node), MidNote{g.A, g.lda, rows, cols, (g.b && g.sign) ? g.b : nullptr, g.xvar, g.moi ? g.varmap : nullptr,
                                                              g.out_quad, g.out_csc, g.out_lin, g.out_const, g.workspace,
                                                              pmt_quad_gram_workspace_bytes(rows, cols)});
    return dispatch(stream, std::move(node));
}

}  // namespace pmt

using namespace pmt;

extern "C" int pmt_quad_gram_constant_order(int64_t rows, int64_t cols, int *order, int *groups, int *stage_rows) {
    PMT_REQUIRE(rows >= 0 && cols >= 0 && order, PMT_INVALID_ARGUMENT, "quad_gram_constant_order: bad argument");
    // the form of an undelivered CSC call, which is never a tiny node: a tiny node sums in row order, as the stream-K node does at its
    // <= 64 rows — except for one row of 129 .. 180 columns, the one-launch form here, where every order adds the same single square
    const ConstantOrder o = constant_order(gram_form(rows, cols, true, false), rows, cols);
    *order = o.order; if (groups) *groups = o.groups; if (stage_rows) *stage_rows = o.stage_rows;
    return PMT_OK;
}

extern "C" int pmt_quad_gram_mid_defers(int64_t rows, int64_t cols, int *plan, int *whole_rounds) {
    PMT_REQUIRE(rows >= 0 && cols >= 0 && plan, PMT_INVALID_ARGUMENT, "quad_gram_mid_defers: bad argument");
    bool whole = false;
    const bool can = gram_form(rows, cols, true, false) == GramForm::Mid && gram_mid_defers(rows, cols, &whole);
    *plan = can ? 1 : 0; if (whole_rounds) *whole_rounds = (can && whole) ? 1 : 0;
    return PMT_OK;
}

extern "C" int pmt_quad_gram_mid_strips(int64_t rows, int64_t cols, int *strips, int *tiles_in_strips) {
    PMT_REQUIRE(rows >= 0 && cols >= 0 && strips, PMT_INVALID_ARGUMENT, "quad_gram_mid_strips: bad argument");
    int ns = 0, nt = 0;
    if (gram_form(rows, cols, true, false) == GramForm::Mid) gram_mid_strips(rows, cols, &ns, &nt);
    *strips = ns; if (tiles_in_strips) *tiles_in_strips = nt;
    return PMT_OK;
}

extern "C" size_t pmt_quad_gram_workspace_bytes(int64_t rows, int64_t cols) {
    // The most that a form the shape takes across call kinds (plain or CSC, delivered; a tiny node none) needs, and never less than the
    // stream-K node's need — its partial tiles (which the fused form's strict launch shares), the chunk sums of q, the chains of c'c.
    size_t bytes = gram_sk_workspace_bytes(rows, cols) +
                   sizeof(double) * ((size_t)linear_splits(rows, cols) * (size_t)std::max<int64_t>(cols, 0) + blocked_dot_scratch_doubles());
    for (const bool deliver : {false, true}) {
        const GramForm form = gram_form(rows, cols, true, deliver);
        bytes = std::max(bytes, form == GramForm::Fused ? gram_tall_workspace_bytes(rows, cols) : form == GramForm::Mid ? gram_mid_workspace_bytes(rows, cols) : 0);
    }
    return bytes;
}

extern "C" int pmt_quad_gram_f64(const double *A, int64_t lda, int64_t rows, int64_t cols, const int64_t *xvar, const double *b, int sign,
                                 int moi, const int64_t *varmap, pmt_quadratic_term *out_quad, pmt_linear_term *out_lin, double *out_const,
                                 void *workspace, void *stream) {
    if (cols > 0) PMT_REQUIRE(out_quad, PMT_INVALID_ARGUMENT, "quad_gram: null out_quad");
    return gram_node({A, lda, rows, cols, xvar, b, sign, moi, varmap, out_quad, nullptr, 1.0, out_lin, out_const, workspace}, stream);
}

extern "C" int pmt_quad_gram_csc_f64(const double *A, int64_t lda, int64_t rows, int64_t cols, const int64_t *xvar, const double *b, int sign,
                                     const int64_t *varmap, double alpha, double *out_P_values, pmt_quadratic_term *out_quad,
                                     pmt_linear_term *out_lin, double *out_const, void *workspace, void *stream) {
    if (cols > 0) PMT_REQUIRE(out_P_values, PMT_INVALID_ARGUMENT, "quad_gram_csc: null out_P_values");
    return gram_node({A, lda, rows, cols, xvar, b, sign, 1, varmap, out_quad, out_P_values, alpha, out_lin, out_const, workspace}, stream);
}

extern "C" int pmt_quad_gram_deliver_f64(const double *A, int64_t lda, int64_t rows, int64_t cols, const int64_t *xvar, const double *b, int sign,
                                         int moi, const int64_t *varmap, pmt_quadratic_term *out_quad, pmt_quadratic_term *host_quad, int nstages,
                                         pmt_linear_term *out_lin, double *out_const, void *workspace, void *stream) {
    if (cols > 0) PMT_REQUIRE(out_quad && host_quad, PMT_INVALID_ARGUMENT, "quad_gram_deliver: null out_quad / host_quad");
    PMT_REQUIRE(nstages >= 0 && nstages <= MAXGROUPS, PMT_INVALID_ARGUMENT, "quad_gram_deliver: nstages must be 0 (default) .. 16");
    return gram_node({A, lda, rows, cols, xvar, b, sign, moi, varmap, out_quad, nullptr, 1.0, out_lin, out_const, workspace}, stream, reinterpret_cast<double *>(host_quad), nstages);
}

extern "C" int pmt_quad_gram_csc_deliver_f64(const double *A, int64_t lda, int64_t rows, int64_t cols, const int64_t *xvar, const double *b, int sign,
                                             const int64_t *varmap, double alpha, double *out_P_values, double *host_P_values, int ngroups,
                                             pmt_linear_term *out_lin, double *out_const, void *workspace, void *stream) {
    if (cols > 0) PMT_REQUIRE(out_P_values && host_P_values, PMT_INVALID_ARGUMENT, "quad_gram_csc_deliver: null P values pointer");
    PMT_REQUIRE(ngroups >= 0 && ngroups <= MAXGROUPS, PMT_INVALID_ARGUMENT, "quad_gram_csc_deliver: ngroups must be 0 (default) .. 16");
    return gram_node({A, lda, rows, cols, xvar, b, sign, 1, varmap, nullptr, out_P_values, alpha, out_lin, out_const, workspace}, stream, host_P_values, ngroups);
}
