// Canonical least-squares objective for WIDE shapes of 129 .. 4096 columns (from the sizes the reference is used at with a few hundred
// variables up to config 2, within what the fast load path reaches: gram.hip, gram_form) in ONE launch: upper triangle of A'A, q = 2 A'c, c'c.
//
// Reference semantics replaced: _vecdot!/muladd! literal expansion (src/functions.jl:702-709,548-576) + canonicalize!
// (src/functions.jl:381-386, src/util.jl:9-26) + update!(::MOI.ScalarQuadraticFunction) (src/moi_interop.jl:45-62): SURVEY Appendix A.3.
//
// Why a third form beside gram_sk.hip / gram_tall.hip (profiles/r06_gram_mid.txt): on 128 x 128 tiles a split tile's partial is 128 KB — as
// large as the 64 rows x 256 columns a work unit reads.  4096 x 512 wrote and re-read 84 MB of partials through a second (fix-up) launch:
// 54.8 us for 13.7 us of flops.  Here
//   * tiles are 64 x 64 (a partial is 32 KB); a workgroup takes one (tile, row chunk); its four waves split the chunk's 8-row groups among
//     themselves (a split of the contraction index: each wave holds the WHOLE tile, 16 blocks x 4 rotations = 64 accumulators, so a
//     k-step's 4 + 4 operand loads feed 64 MFMAs) and stream their rows straight from global memory (L2 / Infinity Cache) in the MFMA
//     operand layout — no barrier, no shared panel; the rotated B operands come out of the wave's private piece of LDS (gram_tall.hip:
//     gram_stream_kernel); an 8-row group and the loads of the group D further on are one pinned instruction stream (mid_step);
//   * diagonal tiles compute their 10 upper blocks and carry q = A'c on the matrix pipe (B operand = c in every lane of the slot); they are
//     split into fewer chunks than the off-diagonal ones (40 against 64 MFMAs per k-step);
//   * the waves' sums are added through LDS in a fixed order; a split tile's partials go to the workspace and the LAST workgroup of the tile
//     to arrive (one atomic counter per tile, release / acquire fences at agent scope — nobody spins, no co-residency needed) adds them in
//     CHUNK order, whatever the arrival order: deterministic sums; it then writes the tile's terms as row-contiguous 16-byte chunks;
//   * c'c is one more workgroup of the same launch, in the order pmt_quad_gram_constant_order reports as 5 (gram_sk.hip: sk_lin_role),
//     restated bit for bit by tests/gpu_util.py.
// Summation order of a coefficient (fixed by (rows, cols) alone): wave w of chunk c adds the 8-row groups c gpc + w, + 4, .. in MFMA k
// order (rows 2 k, 2 k + 1 of a group in contraction slot k); waves (0 + 2) + (1 + 3); chunks in ascending order.  The waves' sums are
// added in one of two places — by halving behind the item's loop (mid_tail), or, for a DEFERRED tile of the persistent walk, row by row
// inside the next item's loop from the four raw partials in LDS (mid_wo_op: (p0 + p2) + (p1 + p3)) — each level the same two operands,
// so the same bits; pmt_quad_gram_mid_defers tells which shapes defer (profiles/r20_deferred_tile.txt).
// A tile inside a STRIP (mid_strips; pmt_quad_gram_mid_strips tells which shapes have them and how many of their first body tiles they
// take — again (rows, cols) alone) is ONE wave's for the whole contraction: a coefficient is ONE chain, the 8-row groups 0, 1, 2, .. of
// the matrix in MFMA k order, with no wave level and no chunk level.  Every other tile of such a launch, q and c'c are summed as above.
#include "affine_tile.h"
#include "gram_common.h"

#ifndef PMT_MID_WPS
#define PMT_MID_WPS 1              // waves per SIMD the register budget aims at
#endif
#ifndef PMT_MID_G
#define PMT_MID_G 256              // workgroups per round (one per CU: 202 + 128 registers per lane)
#endif
#ifndef PMT_MID_MAXWG
#define PMT_MID_MAXWG 2304         // workgroups at most (several rounds where the tiles alone are more than half of the CUs)
#endif
#ifndef PMT_MID_D
#define PMT_MID_D 2                // iterations (8-row groups) in flight per wave (pinned stream, mid_step: 2 33.6 us at 4096 x 512, 3 34.0, 4 35.4; 4096 x 1024 97.7 / 100.3 / 103.7)
#endif
#ifndef PMT_MID_WO_RPS
#define PMT_MID_WO_RPS 2           // rows of a deferred tile that a wave writes out per 8-row group of the next item's loop (mid_wo_op: 1 and 2 the same step time at config 2, 1.0637 / 1.0645 ms against the parent's 1.0748; 4 spills 7 registers)
#endif
#ifndef PMT_MID_GROUP_US
#define PMT_MID_GROUP_US 1.15      // the cost model's time of one 8-row group per wave (mid_plan)
#endif
#ifndef PMT_MID_TAIL_US
#define PMT_MID_TAIL_US 0.95       // the same in the plan of unsplit tiles with split tails (mid_plan)
#endif
#ifndef PMT_MID_SB
#define PMT_MID_SB 8               // edge of a super-tile in tiles
#endif
#ifndef PMT_MID_FB
#define PMT_MID_FB 4               // chunks whose partials the last arriver loads together (64 loads per thread: a wave may have 63 outstanding; 8, or 16-byte loads: no faster)
#endif
// The hand-over of a partial to the tile's last arriver.  0 (ships): the partial goes out as agent-scope write-through stores (sc1),
// s_waitcnt vmcnt(0), then the relaxed agent-scope count; the last arriver reads the partials with agent-scope loads — per-access
// coherence, the same contract as the pair fold of gram_sk.hip (a property of gfx942 / gfx950, which is all this library is built for).
// 1: the memory model's form — release fence (buffer_wbl2 sc1: the XCD's whole L2) in every workgroup, acquire fence (buffer_inv sc1) in the
// last arriver; measured in profiles/r06_gram_mid.txt.
#ifndef PMT_MID_FORMAL
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__)
#define PMT_MID_FORMAL 1
#else
#define PMT_MID_FORMAL 0
#endif
#endif

#ifdef PMT_MID_TRACE
// debugging aid (tools/mid_trace.py): 100 MHz wall-clock stamps of the phases of every workgroup (of its LAST item where it walks several)
__device__ unsigned long long g_mid_trace[1024 * 8];
// ... and (tools/mid_walk_trace.py) per workgroup of the persistent walk, summed over its items in eight words of LDS behind the kernel's
// own (mid_walk_note) and written out when it leaves: [0] items, [1] main loops (a deferred tile's write-out inside), [2] stamp 1 -> 3 / 5 (the waves'
// sums, the count, a fold; of a deferring item: the hand-off), [3] epilogues (none of a deferring item),
// [4] from one item's last store to the next one's start, [5] the first item's start, [6] the last item's end, [7] the time it left
__device__ unsigned long long g_mid_walk[1024 * 8];
// ... and of its rider tiles: [0] how many it drew, [1] the time its last rider store had left
__device__ unsigned long long g_mid_riders[1024 * 2];
#define MID_TRACE_WORDS 8
__device__ __forceinline__ void mid_walk_note(unsigned long long *w, int k, unsigned long long t) {
    if (k == 0) { if (w[0]) w[4] += t - w[7]; else w[5] = t; w[0] += 1; }
    else if (k == 1) w[1] += t - w[7];
    else if (k == 3 || k == 5) { w[2] += t - w[7]; w[6] = t; }          // (3: a split tile's chunk that is not the last to arrive ends here)
    else if (k == 6) { w[3] += t - w[7]; w[6] = t; }
    else return;
    w[7] = t;
}
#define MID_STAMP(k) do { if (threadIdx.x == 0 && blockIdx.x < 1024) { const unsigned long long t_ = wall_clock64(); g_mid_trace[blockIdx.x * 8 + (k)] = t_; \
                          mid_walk_note(reinterpret_cast<unsigned long long *>(sh + MSH_AT), (k), t_); } } while (0)
// (the stamps are per translation unit: the strip build, gram_mid_strips.hip, has its own; the readers overlay the workgroups that
// build stamped — a traced process launches one shape)
#ifdef PMT_MID_STRIPS_TU
extern "C" int pmt_mid_strips_trace_read(int which, unsigned long long *host) {
    if (which == 0) return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_mid_trace), sizeof(unsigned long long) * 1024 * 8) == hipSuccess ? 0 : 1;
    if (which == 1) return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_mid_walk), sizeof(unsigned long long) * 1024 * 8) == hipSuccess ? 0 : 1;
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_mid_riders), sizeof(unsigned long long) * 1024 * 2) == hipSuccess ? 0 : 1;
}
#else
extern "C" int pmt_mid_strips_trace_read(int which, unsigned long long *host);
static int mid_trace_overlay(int which, unsigned long long *host, int words, int key) {
    static unsigned long long other[1024 * 8];
    if (pmt_mid_strips_trace_read(which, other)) return 1;
    for (int b = 0; b < 1024; ++b)
        if (other[b * words + key]) for (int i = 0; i < words; ++i) host[b * words + i] = other[b * words + i];
    return 0;
}
extern "C" int pmt_mid_trace_read(unsigned long long *host) {
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_mid_trace), sizeof(unsigned long long) * 1024 * 8) != hipSuccess) return 1;
    return mid_trace_overlay(0, host, 8, 0);
}
extern "C" int pmt_mid_walk_read(unsigned long long *host) {
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_mid_walk), sizeof(unsigned long long) * 1024 * 8) != hipSuccess) return 1;
    return mid_trace_overlay(1, host, 8, 0);
}
extern "C" int pmt_mid_riders_read(unsigned long long *host) {
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_mid_riders), sizeof(unsigned long long) * 1024 * 2) != hipSuccess) return 1;
    return mid_trace_overlay(2, host, 2, 1);
}
#endif
#else
#define MID_STAMP(k) do { } while (0)
#define MID_TRACE_WORDS 0
#endif

namespace pmt {

constexpr int MT = 64;                       // tile edge
constexpr int MACC = 64;                     // accumulators per lane: (block row tm, block column tn, rotation) = (a >> 4, (a >> 2) & 3, a & 3)
constexpr int MPART = MACC * 64;             // doubles of a tile partial, [a][lane]
constexpr int MSTRIDE = MPART + MT + 8;      // + q partial (diagonal tiles), padded to 64 bytes
constexpr int MPITCH = MT + 1;
constexpr int MFG = 8;                       // chunks per group of a two-level fold (mid_body)
constexpr int MCNT = 16;                     // counter words per tile: [0] the tile's, [1 + group] the groups' (at most 64 chunks)
constexpr int MQBUF = 4 * 2048;              // LDS (doubles): [0, 8192) rotation pieces / the waves' exchange pieces / the finished tile + q + row descriptors;
// A DEFERRED tile (mid_body: hand-off) waits in LDS while the next item's loop runs: the four waves' raw accumulators, [wave][a][lane]
// with a pitch of MDP doubles per a.  A row of the write-out (mid_wo_op) reads 16 different a, four neighbouring lanes each: a pitch of
// 68 = 4 (mod 32) puts the 8 a of a half-wave on 8 different groups of four 8-byte banks (64 dwords: the bank modulus of ds_read_b64).
// The region starts behind the rotation pieces (4 x 4 KB, which the next item's loop uses) and overlaps the exchange pieces and the
// finished tile of the immediate path, which never runs with a tile pending (MidWalk).
constexpr int MDP = 68;
constexpr int MDPART = MACC * MDP;           // doubles of a wave's deferred partial
constexpr int MDEF = 4 * 512;                // the deferred partials: behind the rotation pieces
constexpr int MAREA = 4 * MT;                // a map area of the deferring form: the tile's variable maps (2 x 64) and a deferred tile's row descriptors (64 x (address of the row's first term, row variable))
// The kernel is built twice on the fast load path (gram_mid_kernel<FAST, DF>).  DF = false is the kernel without deferred tiles, kept
// instruction for instruction what it was before there were any (tools/isa_diff.py against the commit before: whatever is new stands
// under `if constexpr (DF)`, the loop's text and the order of the declarations around it included — the register allocation of both
// builds follows them): the larger LDS allocation alone cost the single-round shapes 0.4 .. 0.7 us per launch, a changed decode and loop
// as much again (profiles/r20_deferred_tile.txt).  Only the launches that defer (launch_gram_mid) take the other one.
template <bool DF> struct MidLds {
    static constexpr int QW = DF ? MDEF + 4 * MDPART : MQBUF;      // the waves' q (4 x 64)
    static constexpr int FLAG = QW + 4 * MT;                        // the count's old value
    static constexpr int MAPS = FLAG + 8;                           // the tile's variable maps (2 x 64); DF: two areas, alternating from one deferred tile to the next (MidWalk::par)
    static constexpr int SH = MAPS + (DF ? 2 * MAREA : 2 * MT);
};
// 16 KB of rotation pieces + 4 x 64 x 68 x 8 B = 136 KB of partials + 2 KB (q) + 64 B + 2 x 2 KB = 158.1 KB of the CU's 160 KB (by its
// registers the kernel runs one workgroup per CU either way)
static_assert(MDEF + 4 * MDPART >= MQBUF, "the immediate path's exchange pieces and finished tile lie inside the rotation pieces + partials");
static_assert((MidLds<true>::SH + MID_TRACE_WORDS) * 8 + 16 <= 160 * 1024, "the kernel's LDS: one workgroup within the 160 KB of a gfx950 CU");

struct MidArgs {
    const double *A; int64_t lda, rows, cols;
    const double *b; int sign;               // c_i = 0.0 (+|-) b[i]; null / 0: c = 0
    const int64_t *xvar; const int64_t *varmap; int moi;
    QT *out_quad; double *out_csc; double alpha; LT *out_lin; double *out_const;
    int nb;                                  // 64-column panels
    int n_off, s_off, s_diag;                // strictly upper tiles, row chunks of one, row chunks of a diagonal tile
    int gpc_off, gpc_diag;                   // 8-row groups per chunk
    int n_tail, s_tail, gpc_tail;            // the LAST n_tail strictly upper tiles (in the order they are walked) in s_tail chunks instead (mid_plan)
    int n_strips;                            // the FIRST 4 n_strips body tiles of the walk as strips, a whole tile per wave (mid_strips; in the padding the nine ints left: the layout of the others is what it was)
    double *ws;                              // one MSTRIDE slot per workgroup
    unsigned *counters;                      // one per tile, zero between launches (the last arriver re-arms its tile's)
    int xcd;                                 // workgroup ids in the XCD-aware order (gram_mid_kernel)
    int persist, total;                      // PMT_MID_G persistent workgroups walk the `total` work items (gram_mid_kernel)
    unsigned *tickets;                       // 8 per-XCD tickets + the count of workgroups that have left + the riders' ticket; zero between launches
    const AffineRider *riders;               // constraint packs whose tiles the persistent workgroups draw once their items have run out
    int nriders, rider_tiles;                // (a plan's table, plan.hip; null / 0: nobody rides) ... and the tiles of all of them
};

struct MidPlan { int nb, n_off, s_off, s_diag, gpc_off, gpc_diag, n_tail, s_tail, gpc_tail, wgs; };

// Row chunks per tile, from (rows, cols) alone (the summation order depends on them).  s chunks per off-diagonal tile and ceil(5 s / 8) per
// diagonal one (88 against 128 MFMAs per 8-row group) make W workgroups that run one per CU in ceil(W / PMT_MID_G) rounds of
// ceil(groups per chunk / 4) iterations of ~1.15 us each + ~5 us per workgroup (first loads, the waves' sums; + 1 for a partial); a
// split tile's last arriver then reads s partials (mid_fold_us: 5.5 us measured at s = 7 .. 9, tools/mid_trace.py) — once in the
// launch's tail and, summed over the tiles, as work of the CUs.  The s with the smallest estimate, at most PMT_MID_MAXWG workgroups (33 KB of workspace each).
// what adding `count` partials costs the last arriver: one round of loads per PMT_MID_FB partials (~2.6 us each, tools/mid_trace.py)
static double mid_fold_us(int count) { return 0.5 + 2.6 * (double)cdiv(count, PMT_MID_FB); }

static MidPlan mid_plan(int64_t rows, int64_t cols) {
    MidPlan p;
    p.nb = (int)cdiv(cols, MT);
    p.n_off = p.nb * (p.nb - 1) / 2;
    const int ngroups = (int)std::max<int64_t>(1, cdiv(rows, 8));
    const int maxs = std::max(1, ngroups / 4);
    auto sd = [&](int s) { return std::min(maxs, std::max(1, (5 * s + 7) / 8)); };
    int best = 1;
    double best_t = 1e300;
    for (int s = 1; s <= std::min(maxs, 64); ++s) {
        const int64_t wgs = (int64_t)p.n_off * s + (int64_t)p.nb * sd(s);
        if (s > 1 && wgs > PMT_MID_MAXWG) break;
        const double it_off = (double)cdiv(cdiv(ngroups, s), 4), it_diag = 0.69 * (double)cdiv(cdiv(ngroups, sd(s)), 4);
        const double fold = s <= 1 ? 0.0 : s <= MFG ? mid_fold_us(s) : mid_fold_us(MFG) + 1.5 + mid_fold_us((int)cdiv(s, MFG));
        const double t = (double)cdiv(wgs, PMT_MID_G) * (PMT_MID_GROUP_US * (p.n_off ? std::max(it_off, it_diag) : it_diag) + 5.0 + (s > 1 ? 1.0 : 0.0)) +
                         fold * (1.0 + (double)(p.n_off + p.nb) / PMT_MID_G);
        if (t < best_t) { best_t = t; best = s; }
    }
    int s = best;
#ifdef PMT_TUNING
    if (const char *e = getenv("PMT_MID_S")) { const int v = atoi(e); if (v > 0) s = std::min(v, maxs); }      // (measurement builds only)
#endif
    // UNSPLIT off-diagonal tiles in several rounds of PMT_MID_G workgroups (config 2: 2016 of them + 64 diagonal ones = 8.1 rounds): what the
    // rounds do not divide is split instead of costing a whole tile time on a few CUs —
    //   * the LAST n_off % G off-diagonal tiles (the partial round) in s_tail chunks each (4096 x 3072: 1128 tiles = 4 rounds + 104 tiles,
    //     152 CUs idle for a tile time; in two chunks they are one round of half the length);
    //   * the diagonal tiles (last in the workgroup order) in chunks that fill the CUs the last round leaves free, the rest short rounds
    //     (config 2: instead of a ninth round of 0.69 tile times for 32 workgroups).
    // Both counts by the shortest estimated tail; compared with the best uniform split above.
    int sdiag = sd(s), ntail = 0, stail = 1;
    if (p.n_off + p.nb > PMT_MID_G) {
        // (0.95 us per 8-row group and wave: the pinned loop's time in these long workgroups, tools/mid_trace.py — config 2 1101 -> 1085 us
        // against the uniform model's 1.15, which stays where it decides the summation order of the single-round shapes)
        auto wg_us = [&](int c, double w) { return PMT_MID_TAIL_US * w * (double)cdiv(cdiv(ngroups, c), 4) + 5.0 + (c > 1 ? 1.0 : 0.0); };
        const int rem = p.n_off % PMT_MID_G;
        int ct = 1;
        double tail_off = 0.0;
        if (rem) {
            tail_off = 1e300;
            for (int c = 1; c <= std::min(maxs, MFG); ++c) {
                const double t = (double)cdiv((int64_t)rem * c, PMT_MID_G) * wg_us(c, 1.0) + (c > 1 ? mid_fold_us(c) : 0.0);
                if (t < tail_off) { tail_off = t; ct = c; }
            }
        }
        const int last = rem ? (int)(((int64_t)rem * ct) % PMT_MID_G) : 0, free_cus = last ? PMT_MID_G - last : 0;
        const double t_last = rem ? wg_us(ct, 1.0) : wg_us(1, 1.0);
        int cd = 1;
        double tail_diag = 1e300;
        for (int c = 1; c <= std::min(maxs, MFG); ++c) {
            const double t_d = wg_us(c, 0.69);
            const int64_t inside = (int64_t)free_cus * (int64_t)(t_last / t_d);       // chunks done beside the last off-diagonal round
            const int64_t left = std::max<int64_t>(0, (int64_t)p.nb * c - inside);
            const double t = (double)cdiv(left, PMT_MID_G) * t_d + (c > 1 ? mid_fold_us(c) : 0.0);
            if (t < tail_diag) { tail_diag = t; cd = c; }
        }
        const double t1 = (double)(p.n_off / PMT_MID_G) * wg_us(1, 1.0) + tail_off + tail_diag;
        // (the uniform model counts PMT_MID_GROUP_US per group)
        if (s == 1 || t1 * (PMT_MID_GROUP_US / PMT_MID_TAIL_US) < best_t) { s = 1; sdiag = cd; ntail = ct > 1 ? rem : 0; stail = ct > 1 ? ct : 1; }
    }
#ifdef PMT_TUNING
    if (const char *e = getenv("PMT_MID_TAIL")) { if (atoi(e) == 0) { ntail = 0; stail = 1; } }          // (measurement builds only)
#endif
    p.gpc_off = (int)cdiv(ngroups, s);
    p.s_off = (int)cdiv(ngroups, p.gpc_off);
    p.gpc_diag = (int)cdiv(ngroups, sdiag);
    p.s_diag = (int)cdiv(ngroups, p.gpc_diag);
    p.n_tail = ntail;
    p.gpc_tail = (int)cdiv(ngroups, stail);
    p.s_tail = ntail ? (int)cdiv(ngroups, p.gpc_tail) : 1;
    if (p.s_tail <= 1) { p.n_tail = 0; p.s_tail = 1; p.gpc_tail = ngroups; }
    p.wgs = (p.n_off - p.n_tail) * p.s_off + p.n_tail * p.s_tail + p.nb * p.s_diag + 1;
    return p;
}

// one 8-row group of one wave: buf[t] = rows (row0 + 2 lk, + 1) of column (t < 4 ? cj0 : ck0) + 16 (t & 3) + lm; cb = the same rows of b.
// FAST (A 16-byte aligned with an even pitch, b 16-byte aligned, the matrix within 4 GiB): scalar base + 32-bit lane offset, no mask (a
// column beyond the matrix reads the LAST column: its products land in entries nobody stores).  Otherwise 8-byte loads from clamped
// addresses, what lies outside replaced by 0.0 — no branch around a load (gram_tall.hip: stream_load).
template <bool DIAG, bool FAST>
__device__ __forceinline__ void mid_load(const MidArgs &g, int64_t row0, int lane, int64_t cj0, int64_t ck0, const unsigned (&voff)[DIAG ? 4 : 8],
                                         f64x2 (&buf)[DIAG ? 4 : 8], f64x2 &cb) {
    constexpr int NG = DIAG ? 4 : 8;
    const int lm = lane & 15, lk = lane >> 4;
    if (FAST) {
        const char *base = reinterpret_cast<const char *>(g.A + row0);
#pragma unroll
        for (int t = 0; t < NG; ++t) buf[t] = *reinterpret_cast<const f64x2 *>(base + voff[t]);
        cb.x = 0.0; cb.y = 0.0;
        if (DIAG && g.b) cb = *reinterpret_cast<const f64x2 *>(g.b + row0 + 2 * lk);
        return;
    }
    const int64_t row = row0 + 2 * lk;
    const bool r0 = row < g.rows, r1 = row + 1 < g.rows;
#pragma unroll
    for (int t = 0; t < NG; ++t) {
        const int64_t col = (t < 4 ? cj0 : ck0) + 16 * (t & 3) + lm;
        const bool cv = col < g.cols;
        const bool v0 = cv && r0, v1 = cv && r1;
        const double *p0 = g.A + (v0 ? col * g.lda + row : 0), *p1 = g.A + (v1 ? col * g.lda + row + 1 : 0);
        const double x = *p0, y = *p1;
        buf[t].x = v0 ? x : 0.0;
        buf[t].y = v1 ? y : 0.0;
    }
    cb.x = 0.0; cb.y = 0.0;
    if (DIAG && g.b) {
        const double x = g.b[r0 ? row : 0], y = g.b[r1 ? row + 1 : 0];
        cb.x = r0 ? x : 0.0;
        cb.y = r1 ? y : 0.0;
    }
}

// the MFMAs of one 8-row group.  The B operand of rotation r of a block column is the value the lane 4 r further up its 16-lane row holds:
// the wave stores its four B groups into its private piece of LDS and reads them back rotated (a wave's LDS operations execute in order).
template <bool DIAG>
__device__ __forceinline__ void mid_compute(double *__restrict__ rot, const f64x2 (&buf)[DIAG ? 4 : 8], const f64x2 &cb, int sign, int lane,
                                            double (&acc)[MACC], double (&qacc)[4]) {
    constexpr int BO = DIAG ? 0 : 4;
    const int lm = lane & 15, lrow = lane & 48;
#pragma unroll
    for (int t = 0; t < 4; ++t) *reinterpret_cast<f64x2 *>(rot + (t * 64 + lane) * 2) = buf[BO + t];
    // ALL rotated operands are asked for up front, and the MFMAs that need none of them (rotation 0: the loaded values themselves) go
    // first: the LDS round trip hides behind 32 MFMAs.  Read rotation by rotation in front of their first use, every wait for an LDS
    // read stood in the wave's one issue stream (one wave per SIMD): ~10 exposed waits per 8-row group, the loop at 0.55 of the pipe.
    f64x2 bv[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        bv[c][0] = buf[BO + c];
#pragma unroll
        for (int r = 1; r < 4; ++r) {
            bv[c][r] = *reinterpret_cast<const f64x2 *>(rot + (c * 64 + lrow + ((lm + 4 * r) & 15)) * 2);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    constexpr int NC = 4;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int tm = 0; tm < (DIAG ? c + 1 : 4); ++tm) {
            const int a = (tm * 4 + c) * 4;
            acc[a] = __builtin_amdgcn_mfma_f64_4x4x4f64(buf[tm].x, bv[c][0].x, acc[a], 0, 0, 0);
        }
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int tm = 0; tm < (DIAG ? c + 1 : 4); ++tm) {
            const int a = (tm * 4 + c) * 4;
            acc[a] = __builtin_amdgcn_mfma_f64_4x4x4f64(buf[tm].y, bv[c][0].y, acc[a], 0, 0, 0);
        }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
        for (int r = 1; r < 4; ++r)
#pragma unroll
            for (int tm = 0; tm < (DIAG ? c + 1 : 4); ++tm) {
                const int a = (tm * 4 + c) * 4 + r;
                acc[a] = __builtin_amdgcn_mfma_f64_4x4x4f64(buf[tm].x, bv[c][r].x, acc[a], 0, 0, 0);
            }
#pragma unroll
        for (int r = 1; r < 4; ++r)
#pragma unroll
            for (int tm = 0; tm < (DIAG ? c + 1 : 4); ++tm) {
                const int a = (tm * 4 + c) * 4 + r;
                acc[a] = __builtin_amdgcn_mfma_f64_4x4x4f64(buf[tm].y, bv[c][r].y, acc[a], 0, 0, 0);
            }
    }
    if (DIAG) {
        // q = A'c on the matrix pipe: the B operand is c in every lane of the contraction slot, so block b of the result holds q of the
        // columns 4 b .. 4 b + 3 of the group (four copies)
        const double c0 = signed_const(cb.x, sign), c1 = signed_const(cb.y, sign);
#pragma unroll
        for (int t = 0; t < 4; ++t) qacc[t] = __builtin_amdgcn_mfma_f64_4x4x4f64(buf[t].x, c0, qacc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t) qacc[t] = __builtin_amdgcn_mfma_f64_4x4x4f64(buf[t].y, c1, qacc[t], 0, 0, 0);
    }
}

// The write-out of a DEFERRED tile (mid_body: hand-off): an unsplit strictly upper tile of two whole panels, so every row is 64 doubled
// terms that start at the tile's first column.  Rows are dealt as in mid_epilogue — row 4 i + wave, a lane per term — and a wave's 16 rows
// are taken MWO_RPS per step (an 8-row group of the next item's loop), in the order i = 4 (step's rows) + b: the rows of one step share
// b = (row >> 2) & 3 and with it the lanes' offsets into the partials.  Per row: the row's descriptor (one broadcast read), the four
// waves' partials of the lane's entry, (p0 + p2) + (p1 + p3) — what the halving of mid_tail adds, level by level the same two operands —
// doubled, the column's variable, three 8-byte stores to scalar row base + 24 * lane.  Every operation is one mid_wo_op(n): the loop
// (mid_step<false, true>) puts each behind an MFMA of its own; mid_wo_run issues what is left of a tile without a loop around it.
// What is wave-uniform (step, wave, area, the row's address) is scalar; what depends on the lane comes from a fresh thread id.
constexpr int MWO_RPS = PMT_MID_WO_RPS;            // rows per step and wave
constexpr int MWO_STEPS = 16 / MWO_RPS;            // steps per tile
constexpr int MWO_ROW_OPS = 13;
constexpr int MWO_OPS = 2 + MWO_ROW_OPS * MWO_RPS;
static_assert(4 % MWO_RPS == 0, "the rows of a step share b");
static_assert(MWO_OPS <= 16 + 92, "a step's free places: 16 MFMAs of phase 0, 92 of phase 1");
struct MidWoAt { double *sh; int q, wave, pmo; };          // the pending tile's next step, this wave, the tile's map area: all scalar
struct MidWo { const double *rb; unsigned so; u64 dsc[2], m; double p[4]; u64 dst; };
__device__ __forceinline__ int mid_fresh_lane() {
    int t;
    asm volatile("v_mov_b32 %0, %1" : "=v"(t) : "v"((int)threadIdx.x));
    return t & 63;
}
__device__ __forceinline__ void mid_wo_op(int n, MidWo &r, const MidWoAt &at) {
    const int i0 = at.q * MWO_RPS, b = i0 >> 2, tm0 = i0 & 3;
    if (n == 0) {
        // entry (row, lane) of the tile is accumulator a = 16 tm + 4 (lane >> 4) + (((lane >> 2) - b) & 3) of lane 16 wave + 4 b + (lane & 3) (mid_pos)
        const int lane = mid_fresh_lane();
        r.rb = at.sh + MDEF + ((lane >> 4) * 4 + (((lane >> 2) - b) & 3)) * MDP + (lane & 3) + tm0 * 16 * MDP + at.wave * 16 + b * 4;
        return;
    }
    if (n == 1) { r.so = 24u * (unsigned)mid_fresh_lane(); return; }
    const int e = (n - 2) / MWO_ROW_OPS, o = (n - 2) % MWO_ROW_OPS;
    const int row = 16 * (tm0 + e) + 4 * b + at.wave;
    if (o == 0) {
        const u64 *d = reinterpret_cast<const u64 *>(at.sh + at.pmo + 2 * MT) + 2 * row;
        r.dsc[0] = d[0]; r.dsc[1] = d[1];
    } else if (o <= 4) r.p[o - 1] = r.rb[(o - 1) * MDPART + e * 16 * MDP];
    else if (o == 5) r.m = reinterpret_cast<const u64 *>(at.sh + at.pmo)[mid_fresh_lane()];
    else if (o == 6) {
        const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)r.dsc[0]), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(r.dsc[0] >> 32));
        r.dst = (u64)hi << 32 | lo;
    } else if (o == 7) r.p[0] = r.p[0] + r.p[2];
    else if (o == 8) r.p[1] = r.p[1] + r.p[3];
    else if (o == 9) r.p[0] = 2 * (r.p[0] + r.p[1]);
    else {
        // (an address built from two scalars: named global, or the stores are flat ones, which count as LDS traffic too and after which every wait is for everything)
        typedef __attribute__((address_space(1))) u64 gu64;
        gu64 *d = reinterpret_cast<gu64 *>(r.dst + r.so);
        if (o == 10) d[0] = (u64)__double_as_longlong(r.p[0]);
        else if (o == 11) d[1] = r.dsc[1];
        else d[2] = r.m;
    }
}
// what is left of the pending tile, at once (a flush, or the rest of an item with fewer rounds than the write-out needs)
__device__ __forceinline__ void mid_wo_run(double *sh, int &q, int wave, int pmo) {
    for (; q < MWO_STEPS; ++q) {
        MidWo r;
        const MidWoAt at = {sh, q, wave, pmo};
#pragma unroll
        for (int n = 0; n < MWO_OPS; ++n) mid_wo_op(n, r, at);
    }
}

// The write-out of a pending tile of a STRIP (mid_strips): the tile is ONE wave's — its 64 finished sums per lane lie in the wave's own
// [a][lane] region, its column variables and row descriptors in the wave's own map area — and the wave writes all 64 rows, MWO_RPS per
// step, in the order i = (step's rows) >> 4, b, tm: the rows 16 tm + 4 b + i of one step share i and b and with them the lanes' offsets.
// Per row: the descriptor, ONE partial, doubled, the column's variable, three 8-byte global stores — no sum: nothing was split.
constexpr int MSO_STEPS = MT / MWO_RPS;            // steps per tile and wave
constexpr int MSO_ROW_OPS = 8;
constexpr int MSO_OPS = 2 + MSO_ROW_OPS * MWO_RPS;
constexpr int MSA = 3 * MT;                        // a wave's map area (u64): the tile's column variables, then its 64 row descriptors (address of the row's first term, row variable)
static_assert(MSO_OPS <= 16 + 92, "a step's free places: 16 MFMAs of phase 0, 92 of phase 1");
__device__ __forceinline__ void mid_so_op(int n, MidWo &r, const MidWoAt &at) {          // (at.pmo: the wave's map area)
    const int i0 = at.q * MWO_RPS, i = i0 >> 4, b = (i0 >> 2) & 3, tm0 = i0 & 3;
    if (n == 0) {
        // entry (row, lane) of the tile is accumulator a = 16 tm + 4 (lane >> 4) + (((lane >> 2) - b) & 3) of lane 16 i + 4 b + (lane & 3) (mid_pos)
        const int lane = mid_fresh_lane();
        r.rb = at.sh + MDEF + at.wave * MDPART + ((lane >> 4) * 4 + (((lane >> 2) - b) & 3)) * MDP + (lane & 3) + tm0 * 16 * MDP + i * 16 + b * 4;
        return;
    }
    if (n == 1) { r.so = 24u * (unsigned)mid_fresh_lane(); return; }
    const int e = (n - 2) / MSO_ROW_OPS, o = (n - 2) % MSO_ROW_OPS;
    const int row = 16 * (tm0 + e) + 4 * b + i;
    const u64 *area = reinterpret_cast<const u64 *>(at.sh + at.pmo);
    if (o == 0) { r.dsc[0] = area[MT + 2 * row]; r.dsc[1] = area[MT + 2 * row + 1]; }
    else if (o == 1) r.p[0] = r.rb[e * 16 * MDP];
    else if (o == 2) r.m = area[mid_fresh_lane()];
    else if (o == 3) {
        const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)r.dsc[0]), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(r.dsc[0] >> 32));
        r.dst = (u64)hi << 32 | lo;
    } else if (o == 4) r.p[0] = 2 * r.p[0];
    else {
        typedef __attribute__((address_space(1))) u64 gu64;          // (global stores, not flat ones: mid_wo_op)
        gu64 *d = reinterpret_cast<gu64 *>(r.dst + r.so);
        if (o == 5) d[0] = (u64)__double_as_longlong(r.p[0]);
        else if (o == 6) d[1] = r.dsc[1];
        else d[2] = r.m;
    }
}
__device__ __forceinline__ void mid_so_run(double *sh, int &q, int wave, int pmo) {
    for (; q < MSO_STEPS; ++q) {
        MidWo r;
        const MidWoAt at = {sh, q, wave, pmo};
#pragma unroll
        for (int n = 0; n < MSO_OPS; ++n) mid_so_op(n, r, at);
    }
}

// One 8-row group AND the loads of the group D further on, as ONE pinned instruction stream (the FAST load path).  The
// workgroup has one wave per SIMD: whatever is not an MFMA stands in the wave's only issue stream.  mid_compute + mid_load put the 16 LDS
// operations of a group in one run in front of the MFMAs and its 8 loads (with a 64-bit vector add each: the compiler hoists the zero
// extension of the lane offsets out of the loop and loses the scalar-base form) in runs behind them: ~18.5 clocks per MFMA against 16.6 for
// bare MFMAs.  Here every LDS operation and every load stands alone behind an MFMA (the matrix pipe is busy for 16 clocks after an issue):
//   * the 32 (20 + 8 of q on a diagonal tile) MFMAs that need no rotation first, one LDS operation behind each of the first 16;
//   * the rotated MFMAs block ROW by block row: an A operand's registers are free after its row — its reload is issued there, the B
//     operands' reloads (free after the first phase) behind the first MFMAs of the second;
//   * loads in the scalar-base form (the lane offset passes through an empty asm: nothing to hoist).
// Every accumulator sees the same operations in the same order as in mid_compute (x before y of each group): the same bits.
#define MID_SB() __builtin_amdgcn_sched_barrier(0)
// The reloads take TWO scalar bases, one for the four A-side operands and one for the four B-side ones: both g.A + next_row0 inside an
// item; in the round that ends an item of the persistent walk, the bases of the NEXT item's tile (mid_body) — the lane offsets of two
// whole panels differ by a multiple of the pitch, so the redirect is a scalar select and the stream keeps its instructions.
// WO: the step also carries one step of a deferred tile's write-out (mid_wo_op), one operation behind each MFMA that has nothing behind it
// yet — the same 128 MFMAs, 16 LDS operations and 8 loads in the same places.  ST: the pending tile is a strip's (mid_so_op).
template <bool DIAG, bool WO = false, bool ST = false>
__device__ __forceinline__ void mid_step(const MidArgs &g, double *__restrict__ rot, int64_t next_row0, const char *base_a, const char *base_b,
                                         unsigned (&voff)[DIAG ? 4 : 8], f64x2 (&buf)[DIAG ? 4 : 8], f64x2 &cb, int sign, int lane,
                                         double (&acc)[MACC], double (&qacc)[4], const MidWoAt &wo = MidWoAt()) {
    static_assert(!(DIAG && WO), "only a strictly upper tile's loop carries a write-out");
    MidWo wr;
    int wn = 0;                                      // write-out operations issued
    constexpr int BO = DIAG ? 0 : 4;
    const int lm = lane & 15, lrow = lane & 48, lk = lane >> 4;
    auto reload = [&](int t) {
        asm volatile("" : "+v"(voff[t]));
        buf[t] = *reinterpret_cast<const f64x2 *>((t < 4 ? base_a : base_b) + voff[t]);
    };
    f64x2 bv[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) bv[c][0] = buf[BO + c];
    auto lds_op = [&](int i) {                       // 0..3: the B groups out; 4..15: the rotated reads
        if (i < 4) *reinterpret_cast<f64x2 *>(rot + (i * 64 + lane) * 2) = buf[BO + i];
        else {
            const int c = (i - 4) / 3, r = 1 + (i - 4) % 3;
            bv[c][r] = *reinterpret_cast<const f64x2 *>(rot + (c * 64 + lrow + ((lm + 4 * r) & 15)) * 2);
        }
    };
    MID_SB();
    // phase 0: rotation 0 (operands as loaded), x then y; an LDS operation behind each of the first 16
    int k = 0;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int tm = 0; tm < (DIAG ? c + 1 : 4); ++tm) {
                const int a = (tm * 4 + c) * 4;
                acc[a] = __builtin_amdgcn_mfma_f64_4x4x4f64(pass ? buf[tm].y : buf[tm].x, pass ? bv[c][0].y : bv[c][0].x, acc[a], 0, 0, 0);
                if (k < 16) { MID_SB(); lds_op(k); MID_SB(); }
                else if constexpr (WO) { if (wn < (ST ? MSO_OPS : MWO_OPS)) { MID_SB(); if constexpr (ST) mid_so_op(wn, wr, wo); else mid_wo_op(wn, wr, wo); MID_SB(); ++wn; } }
                ++k;
            }
    if (DIAG) {
        // q = A'c on the matrix pipe (mid_compute)
        const double c0 = signed_const(cb.x, sign), c1 = signed_const(cb.y, sign);
#pragma unroll
        for (int t = 0; t < 4; ++t) qacc[t] = __builtin_amdgcn_mfma_f64_4x4x4f64(buf[t].x, c0, qacc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t) qacc[t] = __builtin_amdgcn_mfma_f64_4x4x4f64(buf[t].y, c1, qacc[t], 0, 0, 0);
        MID_SB();
        // (no b: sign is 0 and signed_const ignores what is loaded — any valid address keeps the block free of branches)
        cb = *reinterpret_cast<const f64x2 *>((g.b ? g.b : g.A) + next_row0 + 2 * lk);
    }
    MID_SB();
    // phase 1: the rotated blocks, block row by block row
    int nb = 0;                                      // B reloads issued (off-diagonal tiles: buf[4..7])
#pragma unroll
    for (int tm = 0; tm < 4; ++tm) {
#pragma unroll
        for (int pass = 0; pass < 2; ++pass)
#pragma unroll
            for (int c = (DIAG ? tm : 0); c < 4; ++c)
#pragma unroll
                for (int r = 1; r < 4; ++r) {
                    const int a = (tm * 4 + c) * 4 + r;
                    acc[a] = __builtin_amdgcn_mfma_f64_4x4x4f64(pass ? buf[tm].y : buf[tm].x, pass ? bv[c][r].y : bv[c][r].x, acc[a], 0, 0, 0);
                    if (!DIAG && nb < 4) { MID_SB(); reload(4 + nb); MID_SB(); ++nb; }
                    else if constexpr (WO) { if (wn < (ST ? MSO_OPS : MWO_OPS)) { MID_SB(); if constexpr (ST) mid_so_op(wn, wr, wo); else mid_wo_op(wn, wr, wo); MID_SB(); ++wn; } }
                }
        MID_SB();
        reload(tm);
        MID_SB();
    }
}

__host__ __device__ constexpr bool mid_used(bool diag, int a) { return !diag || (a >> 4) <= ((a >> 2) & 3); }

// (row, col) inside the tile of accumulator a of a lane (gram_common.h: sk_acc_pos, on the 4 x 4 block grid of the tile)
__device__ __forceinline__ void mid_pos(int lane, int a, int &row, int &col) {
    const int i = lane >> 4, b = (lane >> 2) & 3, j = lane & 3;
    row = 16 * (a >> 4) + 4 * b + i;
    col = 16 * ((a >> 2) & 3) + 4 * ((b + (a & 3)) & 3) + j;
}

// the mapped variable indices of the tile's 64 columns / 64 rows, gathered at the TOP of the workgroup's life (two dependent loads that
// would otherwise stand in the tail of the tile's last arriver); the barriers of the wave sums order them before the epilogue
__device__ __forceinline__ void mid_maps(const MidArgs &g, double *sh, int tid, int jb, int kb, int mo) {
    u64 *cmap = reinterpret_cast<u64 *>(sh + mo);
    if (tid >= 2 * MT || (!g.out_quad && jb != kb)) return;
    const int64_t i = (tid < MT ? (int64_t)kb * MT + tid : (int64_t)jb * MT + tid - MT);
    const int64_t v = i < g.cols ? g.xvar[i] : 1;
    cmap[tid] = (u64)(g.moi ? map_var(g.varmap, v) : v);
}

// The finished tile (sh[row * MPITCH + col], q of a diagonal tile in sh[MT * MPITCH ..]) -> terms.  Row j of the tile's entries
// k = max(j, k0) .. are consecutive QuadraticTerms of the canonical upper triangle: one wave per row, 16-byte chunks.
__device__ __forceinline__ void mid_epilogue(const MidArgs &g, double *sh, int tid, int jb, int kb, int mo) {
    const int wave = tid >> 6, lane = tid & 63;
    const int64_t n = g.cols, j0 = (int64_t)jb * MT, k0 = (int64_t)kb * MT;
    double *tile = sh;
    const double *qfin = sh + MT * MPITCH;
    const u64 *cmap = reinterpret_cast<const u64 *>(sh + mo);             // (mid_maps, at the top of the item; mo: the item's map area)
    const u64 *rmap = cmap + MT;
    if (g.out_csc) {
        const int64_t j = j0 + lane;
#pragma unroll 4
        for (int col = wave; col < MT; col += 4) {
            const int64_t k = k0 + col;
            double c = tile[lane * MPITCH + col];
            if (g.moi || j != k) c = 2 * c;
            if (k < n && j <= k) g.out_csc[k * (k + 1) / 2 + j] = g.alpha * c;
        }
    }
    if (g.out_quad) {
        // One descriptor per tile row (first word of its segment in the term array, term count, first column, diagonal flag), then a
        // wave per row, a lane per TERM: two unconditional LDS reads and three 8-byte stores (scalar row base + 24 * lane + immediate).
        // The workgroup is alone with the tile (one wave per SIMD), so what counts is the instruction count: 16-byte chunks assembled
        // word by word took 15 us per tile as a wave per row with conditional reads, 6.9 us as a flat chunk list, (tools/mid_trace.py).
        u64 *out = reinterpret_cast<u64 *>(g.out_quad);
        u64 *desc = reinterpret_cast<u64 *>(sh + MT * MPITCH + MT);
        if (tid < MT) {
            const int64_t j = j0 + tid;
            const int64_t kstart = j > k0 ? j : k0;
            const int64_t kend = (k0 + MT < n) ? k0 + MT : n;
            const int64_t nterms = (j < n && kend > kstart) ? kend - kstart : 0;
            desc[2 * tid] = (u64)(j * n - (j * (j - 1)) / 2 + (kstart - j)) * 3;
            desc[2 * tid + 1] = (u64)nterms | (u64)(kstart - k0) << 16 | (u64)(kstart == j ? 1 : 0) << 24;
        }
        __syncthreads();
        const bool moi = g.moi != 0;
        const int uwave = __builtin_amdgcn_readfirstlane(wave);
#pragma unroll 4
        for (int i = 0; i < MT / 4; ++i) {
            const int row = 4 * i + uwave;
            const u64 w0 = desc[2 * row], info = desc[2 * row + 1];
            const int nterms = (int)(info & 0xffff), coff = (int)((info >> 16) & 0xff);
            const bool dg = ((info >> 24) & 1) != 0;          // the segment starts on the diagonal: its first term is not doubled in native mode
            double c = tile[row * MPITCH + coff + lane];
            const u64 m = cmap[(coff + lane) & (MT - 1)], rv = rmap[row];
            // off-diagonal: (j,k)+(k,j) combined; diagonal: MOI doubling (moi_interop.jl:58)
            if (moi || !(dg && lane == 0)) c = 2 * c;
            if (lane < nterms) {
                u64 *d = out + w0 + 3 * lane;
                d[0] = (u64)__double_as_longlong(c);
                d[1] = rv;
                d[2] = m;
            }
        }
    }
    if (jb == kb && tid < MT) {
        const int64_t j = j0 + tid;
        if (j < n) {
            LT t;
            t.coeff = 2 * qfin[tid];
            t.var = (int64_t)rmap[tid];
            g.out_lin[j] = t;
        }
    }
}

// c'c in order 5 (gram_sk.hip: sk_lin_role): virtual thread t of 512 adds rows t, t + 512, ..; a shuffle tree per virtual wave; the eight
// virtual waves in order.  Thread tid of this 256-thread workgroup is the virtual threads tid and tid + 256.
__device__ __forceinline__ void mid_constant(const MidArgs &g, double *sh, int tid) {
    const int wave = tid >> 6, lane = tid & 63;
    double s0 = 0.0, s1 = 0.0;
    if (g.b && g.sign) {
        for (int64_t i = tid; i < g.rows; i += 512) { const double c = signed_const(g.b[i], g.sign); s0 = s0 + c * c; }
        for (int64_t i = tid + 256; i < g.rows; i += 512) { const double c = signed_const(g.b[i], g.sign); s1 = s1 + c * c; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { s0 = s0 + __shfl_down(s0, off, 64); s1 = s1 + __shfl_down(s1, off, 64); }
    if (lane == 0) { sh[wave] = s0; sh[4 + wave] = s1; }
    __syncthreads();
    if (tid == 0) {
        double v = sh[0];
#pragma unroll
        for (int w = 1; w < 8; ++w) v = v + sh[w];
        *g.out_const = v;
    }
}

__device__ __forceinline__ void mid_put(double *p, double v) {
#if PMT_MID_FORMAL
    *p = v;
#else
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
__device__ __forceinline__ double mid_get(const double *p) {
#if PMT_MID_FORMAL
    return *p;
#else
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}

// Behind the main loop, as seen by wave W.  The four waves' sums, (0 + 2) + (1 + 3), by halving: wave W hands the half of its 64
// accumulators that its partner W ^ 2 keeps to that partner through LDS and adds the partner's other half to its own; then the same
// with quarters and the partner W ^ 1 — every wave ends up OWNING the finished sums of one block row (a = 16 W .. 16 W + 15), each
// the same bits whichever side added (a + b = b + a).  Two waves summing everything for the others took 2.5 us of the workgroup's tail
// (accumulator moves + adds in one issue stream, tools/mid_trace.py); here every wave moves 48 and adds 48.  The owned quarter then goes
// to the workspace (a split tile) or into the finished tile in LDS; q of a diagonal tile is added by wave 0 (lane = column).
template <bool DIAG, int W, bool DF>
__device__ __forceinline__ void mid_tail(const MidArgs &g, double *sh, int lane, double (&acc)[MACC], const double (&qacc)[4], int nchunk, double *w) {
    constexpr int KEEP1 = (W >> 1) * 32, GIVE1 = 32 - KEEP1, KEEP2 = KEEP1 + (W & 1) * 16, GIVE2 = KEEP1 + 16 - (W & 1) * 16;
    double *mine = sh + W * 2048;
    const double *half = sh + (W ^ 2) * 2048, *quarter = sh + (W ^ 1) * 2048;
    const bool qlane = (lane & 3) == 0;
    const int qcol = 4 * ((lane >> 2) & 3) + (lane >> 4);          // q of column 16 t + qcol sits in qacc[t] of the lanes with lane & 3 == 0
#pragma unroll
    for (int a = 0; a < 32; a += 2)
        if (mid_used(DIAG, GIVE1 + a)) { f64x2 v; v.x = acc[GIVE1 + a]; v.y = acc[GIVE1 + a + 1]; *reinterpret_cast<f64x2 *>(mine + (a * 32 + lane) * 2) = v; }
    if (DIAG && qlane) {
#pragma unroll
        for (int t = 0; t < 4; ++t) sh[MidLds<DF>::QW + W * MT + 16 * t + qcol] = qacc[t];
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 32; a += 2)
        if (mid_used(DIAG, KEEP1 + a)) {
            const f64x2 v = *reinterpret_cast<const f64x2 *>(half + (a * 32 + lane) * 2);
            acc[KEEP1 + a] = acc[KEEP1 + a] + v.x; acc[KEEP1 + a + 1] = acc[KEEP1 + a + 1] + v.y;
        }
    double qsum = 0.0;
    if (DIAG && W == 0) qsum = (sh[MidLds<DF>::QW + lane] + sh[MidLds<DF>::QW + 2 * MT + lane]) + (sh[MidLds<DF>::QW + MT + lane] + sh[MidLds<DF>::QW + 3 * MT + lane]);
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 16; a += 2)
        if (mid_used(DIAG, GIVE2 + a)) { f64x2 v; v.x = acc[GIVE2 + a]; v.y = acc[GIVE2 + a + 1]; *reinterpret_cast<f64x2 *>(mine + (a * 32 + lane) * 2) = v; }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 16; a += 2)
        if (mid_used(DIAG, KEEP2 + a)) {
            const f64x2 v = *reinterpret_cast<const f64x2 *>(quarter + (a * 32 + lane) * 2);
            acc[KEEP2 + a] = acc[KEEP2 + a] + v.x; acc[KEEP2 + a + 1] = acc[KEEP2 + a + 1] + v.y;
        }
    __syncthreads();                                               // (the finished tile overwrites the exchange pieces)
    if (nchunk == 1) {
#pragma unroll
        for (int a = KEEP2; a < KEEP2 + 16; ++a) {
            if (!mid_used(DIAG, a)) continue;
            int row, col;
            mid_pos(lane, a, row, col);
            sh[row * MPITCH + col] = acc[a];
        }
        if (DIAG && W == 0) sh[MT * MPITCH + lane] = qsum;
        return;
    }
#pragma unroll
    for (int a = KEEP2; a < KEEP2 + 16; ++a) if (mid_used(DIAG, a)) mid_put(&w[a * 64 + lane], acc[a]);
    if (DIAG && W == 0) mid_put(&w[MPART + lane], qsum);
    // the partial is visible device-wide before the tile's count goes up (mid_body: a barrier, then the count)
#if PMT_MID_FORMAL
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
#else
    __builtin_amdgcn_s_waitcnt(0);
#endif
}

// sum (in ascending order) of `count` partials `stride` doubles apart, LOADED PMT_MID_FB at a time (the sum is not a chain of round trips to
// the fabric); thread tid: the elements e = tid + 256 u of the [a][lane] layout, and q of column tid of a diagonal tile
template <bool DIAG>
__device__ __forceinline__ void mid_fold(const double *p, int count, int64_t stride, int tid, double (&sum)[16], double &qs) {
#pragma unroll
    for (int u = 0; u < 16; ++u) sum[u] = 0.0;
    qs = 0.0;
    for (int c0 = 0; c0 < count; c0 += PMT_MID_FB) {
        double v[PMT_MID_FB][16], qv[PMT_MID_FB];
#pragma unroll
        for (int cc = 0; cc < PMT_MID_FB; ++cc) {
            const double *pc = p + (int64_t)min(c0 + cc, count - 1) * stride;          // (beyond the last one: a repeated load that is not added)
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int a = (tid >> 6) + 4 * u;
                v[cc][u] = 0.0;
                if (mid_used(DIAG, a)) v[cc][u] = mid_get(pc + tid + 256 * u);
            }
            qv[cc] = 0.0;
            if (DIAG && tid < MT) qv[cc] = mid_get(pc + MPART + tid);
        }
#pragma unroll
        for (int cc = 0; cc < PMT_MID_FB; ++cc) {
            const bool live = c0 + cc < count;
#pragma unroll
            for (int u = 0; u < 16; ++u) { const double t = sum[u] + v[cc][u]; sum[u] = live ? t : sum[u]; }
            const double t = qs + qv[cc];
            qs = live ? t : qs;
        }
    }
}

// What the persistent walk (gram_mid_kernel) knows one item ahead while an item runs; wave-uniform, all false elsewhere.
struct MidWalk {
    bool early;                  // the item in hand belongs to the unsplit body: the ticket behind it is drawn under this item's tail
    unsigned *ticket; int id0;   // ... from this word: id = id0 + 8 * its old value
    int *slot;                   // ... and travels to the other waves through this word of LDS at the barrier in front of the epilogue
    int drawn;                   // out: that id
    bool next_full; int njb, nkb, nrank;      // the item in hand (an unsplit strictly upper tile): two whole panels; its tile and place in the walk
    bool pre;                    // in: this wave's first PMT_MID_D groups are in buf already (the previous item loaded them); out: the next item's are
    // The deferred tile.  An item that prefetches on every wave (mid_body: defer) does not add and write its tile behind its loop: the
    // waves leave their raw accumulators in LDS (the hand-off) and the tile is added and written inside the first rounds of the NEXT
    // item's loop.  INVARIANT: while a tile is pending (woq < MWO_STEPS) nothing but the rotation pieces, the other map area and the next
    // hand-off (behind its barrier) touches LDS.  The item behind a deferring one is the body tile it held in hand, so a tile is only
    // ever pending at the top of a strictly upper item: that item either defers too or writes the pending tile out before anything else
    // (mid_body: mid_wo_run).  A workgroup's last body item holds no body tile in hand and does not defer, so nothing is pending in front
    // of a diagonal chunk, the constant, a rider tile or the end of the kernel: no path leaves or reuses the partials or the areas.
    int woq;                     // the pending tile's next write-out step; MWO_STEPS: none pending
    int par;                     // the map area of the item that runs (0 / 1); a pending tile's is the other one
    bool deferred;               // out: the item left its tile pending (no barrier needed behind it)
};

// nothing of `buf` is needed from here on: the registers are free up to the next loads (an empty definition, no instruction) — on the
// paths that never carry loaded groups into the next item (split tiles, diagonal tiles) they do not count against the fold's budget
template <int N>
__device__ __forceinline__ void mid_forget(f64x2 (&buf)[PMT_MID_D][N]) {
#pragma unroll
    for (int d = 0; d < PMT_MID_D; ++d)
#pragma unroll
        for (int t = 0; t < N; ++t) asm volatile("" : "=v"(buf[d][t].x), "=v"(buf[d][t].y));
}

template <bool DIAG>
__device__ __forceinline__ auto &mid_buf(f64x2 (&own)[PMT_MID_D][4], f64x2 (&walk)[PMT_MID_D][8]) {
    if constexpr (DIAG) return own; else return walk;
}

// `pbuf`: the operand registers of the strictly upper tiles live in the kernel — in the persistent walk they carry the next item's first
// groups from one item into the next (wk.pre)
template <bool DIAG, bool FAST, bool DF>
__device__ __forceinline__ void mid_body(const MidArgs &g, double *sh, int tid, int jb, int kb, int chunk, int nchunk, int gpc, int first_wg, unsigned *counter,
                                         MidWalk &wk, f64x2 (&pbuf)[PMT_MID_D][8]) {
    constexpr int NG = DIAG ? 4 : 8;
    constexpr int D = PMT_MID_D;
    // (what depends on the thread alone is worked out again per item: kept across the walk's loop, with the operand registers now living
    // there too, these values no longer fit the register file)
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lm = lane & 15, lk = lane >> 4;
    const int64_t cj0 = (int64_t)jb * MT, ck0 = (int64_t)kb * MT;
    const int ngroups = (int)((g.rows + 7) >> 3);
    const int g0 = chunk * gpc + wave, g1 = min((chunk + 1) * gpc, ngroups);
    const int my = g1 > g0 ? (g1 - g0 + 3) / 4 : 0;                       // groups g0, g0 + 4, .. of this wave
    // the one ragged group (rows % 8 rows) is the last group of the matrix: loaded with masks, outside the pipelined loop
    const bool ragged = FAST && (g.rows & 7) && my > 0 && g0 + 4 * (my - 1) == ngroups - 1;
    const int nfast = ragged ? my - 1 : my;

    static_assert(FAST || !DF, "tiles are deferred on the fast load path only");
    constexpr int MSH_AT = MidLds<DF>::SH;
    (void)MSH_AT;                                                  // (read by the trace build only)
    MID_STAMP(0);
    const int mo = MidLds<DF>::MAPS + (DF ? wk.par * MAREA : 0), pmo = MidLds<DF>::MAPS + (wk.par ^ 1) * MAREA;
    mid_maps(g, sh, tid, jb, kb, mo);
    double acc[MACC], qacc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < MACC; ++a) acc[a] = 0.0;
    unsigned voff[NG];
#pragma unroll
    for (int t = 0; t < NG; ++t) voff[t] = (unsigned)((min((t < 4 ? cj0 : ck0) + 16 * (t & 3) + lm, g.cols - 1) * g.lda + 2 * lk) * 8);
    double *rot = sh + wave * 512;
    f64x2 dbuf[D][4], cb[D];
    auto &buf = mid_buf<DIAG>(dbuf, pbuf);
    auto row_of = [&](int s) { return (int64_t)(g0 + 4 * min(s, max(nfast - 1, 0))) * 8; };
    // The persistent walk: the last whole round of this item loads the first D groups of the item in hand instead of repeating the last
    // group.  Both items are unsplit strictly upper tiles of whole panels, so the next item gives this wave the same groups g0, g0 + 4, ..
    // (nfast of them: at least D), and its lane offsets are these plus (its first column - this one's) * pitch, per side: every address
    // is one the next item's own first loads would read.  No leftover group and no ragged one, which would need buf[] behind the loop.
    const bool pre = !DIAG && wk.pre;
    bool pf = false;
    if (!DIAG && FAST) pf = wk.early && wk.next_full && nchunk == 1 && !ragged && nfast > 0 && nfast % D == 0 && (int64_t)(kb + 1) * MT <= g.cols;
    // In the deferring build the item DEFERS its tile (MidWalk) where it prefetches.  The launch chose the build (launch_gram_mid) for
    // rows a multiple of 32 D, an unsplit body and a call that writes terms and nothing else: a body item then has whole rounds on all
    // four waves, none ragged — `pf` is the same on every wave, the choice is the workgroup's, and what is left of it at run time is the
    // item in hand (a body tile of a whole panel) and this item's own last panel.  An item that does not defer writes a pending tile out
    // before it touches LDS (its loop and the barrier behind it stand between that and its own tail's LDS writes).
    bool defer = false;
    if constexpr (DF) {
        // (the ticket in hand came through LDS: stated uniform here, the step counter and the loops that test it stay scalar)
        defer = __builtin_amdgcn_readfirstlane((int)pf) != 0;
        if (!defer) mid_wo_run(sh, wk.woq, wave, pmo);
    }
    bool late = false;                                             // the ticket was drawn in front of the loop's last round ...
    unsigned drawn_late = 0;                                       // ... this one
    const int ahead_at = __builtin_amdgcn_readfirstlane(pf ? nfast - D : -1);          // (a scalar: the loop compares it without a vector instruction)
    const int64_t shift_a = pf ? ((int64_t)wk.njb * MT - cj0) * g.lda * 8 : 0, shift_b = pf ? ((int64_t)wk.nkb * MT - ck0) * g.lda * 8 : 0;
    if (nfast > 0) {
        if (!pre) {
            // (group by group, as the loop issues them: the loop's vmcnt waits are the stricter of what this order and the loop's own
            // demand — with the groups' loads interleaved here, every round waited for all but one load of the group behind)
#pragma unroll
            for (int d = 0; d < D; ++d) {
                __builtin_amdgcn_sched_barrier(0);
                mid_load<DIAG, FAST>(g, row_of(d), lane, cj0, ck0, voff, buf[d], cb[d]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // FAST: the pinned stream; mid_compute + mid_load with scheduling barriers between the phases, which it replaced there (37.3 -> 34.3 us
        // at 4096 x 512, 1250 -> 1189 at 65536 x 1024 — profiles/r06_gram_mid.txt), still serve the bounds-checked path and the leftovers
        if (FAST) {
            // whole rounds of D groups as one branch-free block (a branch inside it and the compiler's vmcnt waits fall back to "all
            // loads": the number of loads in flight must not depend on the path); the loads beyond the last group repeat the last group
            int s0 = 0;
            if constexpr (!DIAG && DF) {
                // the first rounds of an item behind a deferred tile: the same rounds with the tile's write-out in them, a step per group
                // (loops of their own: the steady rounds below keep their instruction stream and their waits)
                static_assert(MWO_STEPS % D == 0, "whole rounds of write-out steps");
                for (; s0 + D <= nfast && wk.woq < MWO_STEPS; s0 += D, wk.woq += D) {
                    const bool ahead = s0 == ahead_at;
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        const int64_t row = ahead ? (int64_t)(g0 + 4 * d) * 8 : row_of(s0 + d + D);          // (ahead: at least D groups, row_of(d) without its clamp)
                        const char *base = reinterpret_cast<const char *>(g.A + row);
                        const MidWoAt at = {sh, wk.woq + d, wave, pmo};
                        mid_step<DIAG, true>(g, rot, row, base + (ahead ? shift_a : 0), base + (ahead ? shift_b : 0), voff, buf[d], cb[d], g.sign, lane, acc, qacc, at);
                    }
                }
            }
            // A deferring item draws the ticket behind the item in hand in front of its LAST round, where that is a steady one: the
            // hand-off is a few hundred clocks of LDS traffic, not the tail that hid the ticket's round trip, and the round is a copy
            // of its own behind the loop — straight-line, so its waits count the one more operation in flight, and the loop keeps its text.
            if constexpr (DF) late = defer && s0 + D <= nfast;
            for (; s0 + D <= nfast - (late ? D : 0); s0 += D) {
                const bool ahead = s0 == ahead_at;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    // (DF, ahead: at least D groups, row_of(d) without its clamp — with the clamp the deferring build's round held vector instructions)
                    const int64_t row = ahead ? (DF ? (int64_t)(g0 + 4 * d) * 8 : row_of(d)) : row_of(s0 + d + D);
                    const char *base = reinterpret_cast<const char *>(g.A + row);
                    mid_step<DIAG>(g, rot, row, base + (ahead ? shift_a : 0), base + (ahead ? shift_b : 0), voff, buf[d], cb[d], g.sign, lane, acc, qacc);
                }
            }
            if constexpr (DF) {
                if (late) {
                    // (as a wrapping increment: an atomic add the compiler turns into a wave reduction whose result it waits for on the spot)
                    if (tid == 0) drawn_late = __builtin_amdgcn_atomic_inc32(wk.ticket, ~0u, __ATOMIC_RELAXED, "agent");
#pragma unroll
                    for (int d = 0; d < D; ++d) {          // (the last round: ahead, the next item's first groups)
                        const char *base = reinterpret_cast<const char *>(g.A + (int64_t)(g0 + 4 * d) * 8);
                        mid_step<DIAG>(g, rot, (int64_t)(g0 + 4 * d) * 8, base + shift_a, base + shift_b, voff, buf[d], cb[d], g.sign, lane, acc, qacc);
                    }
                    s0 += D;
                }
            }
#pragma unroll
            for (int d = 0; d < D - 1; ++d)
                if (s0 + d < nfast) mid_compute<DIAG>(rot, buf[d], cb[d], g.sign, lane, acc, qacc);
        } else {
            for (int s0 = 0; s0 < nfast; s0 += D) {
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    if (s0 + d < nfast) mid_compute<DIAG>(rot, buf[d], cb[d], g.sign, lane, acc, qacc);
                    mid_load<DIAG, FAST>(g, row_of(s0 + d + D), lane, cj0, ck0, voff, buf[d], cb[d]);
                }
            }
        }
    }
    if (ragged) {
        mid_load<DIAG, false>(g, (int64_t)(ngroups - 1) * 8, lane, cj0, ck0, voff, buf[0], cb[0]);
        mid_compute<DIAG>(rot, buf[0], cb[0], g.sign, lane, acc, qacc);
    }

    if constexpr (DF) wk.deferred = false;
    if constexpr (!DIAG && DF) {
        if (defer) {
            // The HAND-OFF.  What the loop's rounds did not take of the tile before this one goes out first; then a barrier (every wave's
            // last read of the pending partials and descriptors), the raw accumulators and this tile's descriptors, a barrier — and the
            // next item's loop starts, its first groups in registers.  The ticket travels as it does in front of the epilogue.
            mid_wo_run(sh, wk.woq, wave, pmo);
            MID_STAMP(1);
            wk.pre = pf;
            unsigned drawn = drawn_late;
            if (!late && tid == 0) drawn = __hip_atomic_fetch_add(wk.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            double *mine = sh + MDEF + wave * MDPART + lane;
#pragma unroll
            for (int a = 0; a < MACC; ++a) mine[a * MDP] = acc[a];
            if (tid < MT) {
                const int64_t n = g.cols, j = cj0 + tid;
                u64 *desc = reinterpret_cast<u64 *>(sh + mo + 2 * MT);
                desc[2 * tid] = (u64)(reinterpret_cast<u64 *>(g.out_quad) + (u64)(j * n - (j * (j - 1)) / 2 + (ck0 - j)) * 3);
                desc[2 * tid + 1] = reinterpret_cast<const u64 *>(sh + mo)[MT + tid];
            }
            if (tid == 0) *wk.slot = wk.id0 + 8 * (int)drawn;
            __syncthreads();
            wk.drawn = *wk.slot;
            wk.woq = 0; wk.par ^= 1; wk.deferred = true;
            MID_STAMP(5);
            return;
        }
    }
    MID_STAMP(1);
    wk.pre = pf;
    // the ticket behind the item in hand: asked for here, where only the tail's LDS traffic and the epilogue's stores follow it (behind
    // this item's loads, the next item's included); looked at in front of the epilogue
    unsigned drawn = 0;
    if (!DIAG && wk.early && tid == 0) drawn = __hip_atomic_fetch_add(wk.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned *flag = reinterpret_cast<unsigned *>(sh + MidLds<DF>::FLAG);
    double *w = g.ws + (int64_t)(first_wg + chunk) * MSTRIDE;
    __syncthreads();                                               // every wave is done with its rotation piece
    if (wave == 0) mid_tail<DIAG, 0, DF>(g, sh, lane, acc, qacc, nchunk, w);
    else if (wave == 1) mid_tail<DIAG, 1, DF>(g, sh, lane, acc, qacc, nchunk, w);
    else if (wave == 2) mid_tail<DIAG, 2, DF>(g, sh, lane, acc, qacc, nchunk, w);
    else mid_tail<DIAG, 3, DF>(g, sh, lane, acc, qacc, nchunk, w);
    MID_STAMP(2);
    if (nchunk > 1) {
        // One level up to MFG chunks: the tile's last arriver adds them all.  Beyond (few tiles, tall: 65536 x 256 is 10 tiles of 29 chunks —
        // one CU reading 29 x 32 KB took 20 us of the node's 113), two levels: the last arriver of every GROUP of MFG consecutive chunks adds
        // its group and publishes the sum in the slot of the group's first chunk, the last of THOSE adds the groups' sums.  The order stays
        // fixed: chunks in order within a group, groups in order.
        const bool two = nchunk > MFG;
        const int gfirst = two ? (chunk / MFG) * MFG : 0;
        const int n1 = two ? min(MFG, nchunk - gfirst) : nchunk;
        unsigned *c1 = two ? counter + 1 + chunk / MFG : counter;
        __syncthreads();                                           // every wave's quarter of the partial has left (mid_tail waits for its stores)
        if (tid == 0) *flag = __hip_atomic_fetch_add(c1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        MID_STAMP(3);
        if (*flag != (unsigned)(n1 - 1)) { mid_forget(buf); return; }          // (workgroup-uniform) not the last one of this tile / group
#if PMT_MID_FORMAL
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#endif
        if (tid == 0) __hip_atomic_store(c1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);          // re-armed for the next launch
        double sum[16], qs;
        double *p = g.ws + (int64_t)(first_wg + gfirst) * MSTRIDE;
        mid_fold<DIAG>(p, n1, MSTRIDE, tid, sum, qs);
        if (two) {
#pragma unroll
            for (int u = 0; u < 16; ++u) if (mid_used(DIAG, (tid >> 6) + 4 * u)) mid_put(p + tid + 256 * u, sum[u]);
            if (DIAG && tid < MT) mid_put(p + MPART + tid, qs);
#if PMT_MID_FORMAL
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
#else
            __builtin_amdgcn_s_waitcnt(0);
#endif
            __syncthreads();                                       // (also: everyone has read the first count's old value)
            if (tid == 0) *flag = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            const int ng = (nchunk + MFG - 1) / MFG;
            if (*flag != (unsigned)(ng - 1)) { mid_forget(buf); return; }
#if PMT_MID_FORMAL
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#endif
            if (tid == 0) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            mid_fold<DIAG>(g.ws + (int64_t)first_wg * MSTRIDE, ng, (int64_t)MFG * MSTRIDE, tid, sum, qs);
        }
        __syncthreads();                                           // (the tile overwrites the exchange pieces)
        MID_STAMP(4);
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int a = (tid >> 6) + 4 * u;
            if (!mid_used(DIAG, a)) continue;
            int row, col;
            mid_pos(lane, a, row, col);
            sh[row * MPITCH + col] = sum[u];
        }
        if (DIAG && tid < MT) sh[MT * MPITCH + tid] = qs;
        mid_forget(buf);
    }
    if (!DIAG && wk.early && tid == 0) *wk.slot = wk.id0 + 8 * (int)drawn;
    __syncthreads();
    if (!DIAG && wk.early) wk.drawn = *wk.slot;
    MID_STAMP(5);
    mid_epilogue(g, sh, tid, jb, kb, mo);
#ifdef PMT_MID_TRACE
    __builtin_amdgcn_s_waitcnt(0);
    MID_STAMP(6);
#endif
}

// position of workgroup `id` in the XCD-major order of the ids [base, base + n): the ids of XCD 0 (id % 8 == 0) first, in ascending order,
// then XCD 1's, ..
__device__ __forceinline__ int mid_xcd_rank(int id, int base, int n) {
    const int x = id & 7, end = base + n;
    int start = 0;
    for (int y = 0; y < x; ++y) {
        const int fy = base + ((y - base) & 7);                    // the first id of the range on XCD y
        start += fy < end ? ((end - 1 - fy) >> 3) + 1 : 0;
    }
    return start + ((id - (base + ((x - base) & 7))) >> 3);
}

// Strictly upper tile number t -> (jb, kb) in SUPER-TILE order (round 6c): 8 x 8 blocks of tiles, column by column; inside a block row by
// row (on the diagonal: column by column).  32 consecutive tiles — what an XCD runs at a time — are then 4 row panels x 8 column panels
// (12 panels through its L2) instead of one column panel with 32 row panels (33): config 2 moved 4.39 GB per launch over the fabric.
// COLS (the deferring build only, where the decode stands alone between two items in the waves' one issue stream: 1.9 -> 1.2 us per item,
// profiles/r20_deferred_tile.txt): a column of blocks at a time, the same order; every other build keeps the walk block by block.
template <bool COLS>
__device__ __forceinline__ void mid_tile_of(int t, int nb, int &jb, int &kb) {
    constexpr int SB = PMT_MID_SB;
    const int nsb = (nb + SB - 1) / SB;
    if constexpr (!COLS) {
        for (int K = 0; K < nsb; ++K) {
            const int wK = min(SB, nb - SB * K);
            for (int J = 0; J <= K; ++J) {
                const int cnt = J < K ? SB * wK : wK * (wK - 1) / 2;
                if (t >= cnt) { t -= cnt; continue; }
                if (J < K) { jb = SB * J + t / wK; kb = SB * K + t % wK; return; }
                int kk = 1;
                while (t >= kk) { t -= kk; ++kk; }
                jb = SB * K + t; kb = SB * K + kk;
                return;
            }
        }
        jb = 0; kb = 1;
    } else {
        for (int K = 0; K < nsb; ++K) {
            const int wK = min(SB, nb - SB * K);
            const int above = K * SB * wK, cnt = above + wK * (wK - 1) / 2;          // the K blocks above the diagonal one, and the column
            if (t >= cnt) { t -= cnt; continue; }
            if (t < above) {
                if (wK == SB) { jb = t / SB; kb = SB * K + t % SB; }                  // (block J = t / SB^2, row t % SB^2 / SB of it: SB J + that row is t / SB)
                else { const int J = t / (SB * wK), u = t - J * SB * wK; jb = SB * J + u / wK; kb = SB * K + u % wK; }
                return;
            }
            t -= above;
            int kk = 1;
            while (t >= kk) { t -= kk; ++kk; }
            jb = SB * K + t; kb = SB * K + kk;
            return;
        }
        jb = 0; kb = 1;
    }
}

// one work item of the launch: (tile, chunk) number `id`, or the constant's (the last one)
struct MidItem { int kind, jb, kb, chunk, nch, gpc, first, rank; };          // kind: 0 a strictly upper tile, 1 a diagonal one, 2 the constant
// ST (the strip build, behind its strips): the ids 0 .. n_strips - 1 are the strips (mid_strips) and the first 4 n_strips ranks of the walk
// theirs; the body tiles behind them, the tails, the diagonal chunks and the constant follow in the order they always had, with the
// workspace slots and counters they always had.
template <bool COLS, bool ST = false>
__device__ __forceinline__ MidItem mid_decode(const MidArgs &g, int id) {
    // XCD-aware order: workgroup ids go round-robin over the 8 XCDs (id % 8), each with its own 4 MB L2.  The (chunk, tile) list is walked
    // CHUNK-major and cut into 8 contiguous pieces, one per XCD: the 32 workgroups an XCD runs at a time work on the same rows of A and
    // on neighbouring tiles (shared 64-column panels), so a matrix larger than one L2 is still read mostly out of L2 — numbered tile-major
    // (id = tile * S + chunk) every XCD touched every row chunk of every panel and 4096 x 1024 ran out of the Infinity Cache at 1.76 us per
    // 8-row group instead of 1.15 (profiles/r06_gram_mid.txt).
    MidItem it = {2, 0, 0, 0, 1, 0, 0, 0};
    const int sb = ST ? g.n_strips : 0;          // (ST: s_off = 1)
    const int nbody = g.n_off - g.n_tail - 4 * sb, wbody = sb + nbody * g.s_off, noff = wbody + g.n_tail * g.s_tail;
    if (id < noff) {
        // body tiles (ranks 0 .. nbody - 1 of the walk) in s_off chunks, then the tail tiles in s_tail chunks: chunk-major inside each part
        const bool tail = id >= wbody;
        const int base = tail ? wbody : sb, ntile = tail ? g.n_tail : nbody, nch = tail ? g.s_tail : g.s_off;
        const int k = g.xcd ? mid_xcd_rank(id, base, ntile * nch) : ((id - base) % nch) * ntile + (id - base) / nch;
        const int chunk = k / ntile;
        const int rank = 4 * sb + (tail ? nbody : 0) + (k - chunk * ntile);          // the tile's place in the walk: its workspace slots and its counters
        int t = rank, jb, kb;
        if (g.xcd || ST) mid_tile_of<COLS>(t, g.nb, jb, kb);          // (ST: ONE walk for the strips and the tiles behind them, whatever the order of the ids — mid_strips takes its ranks from mid_tile_of)
        else {
            kb = 1;
            while (t >= kb) { t -= kb; ++kb; }                     // strictly upper tiles, column by column: (0,1), (0,2), (1,2), (0,3), ..
            jb = t;
        }
        it.kind = 0; it.jb = jb; it.kb = kb; it.chunk = chunk; it.nch = nch; it.gpc = tail ? g.gpc_tail : g.gpc_off;
        it.first = tail ? wbody + 3 * sb + (rank - 4 * sb - nbody) * g.s_tail : rank * g.s_off;
        it.rank = rank;
        return it;
    }
    if (id < noff + g.nb * g.s_diag) {
        const int k = g.xcd ? mid_xcd_rank(id, noff, g.nb * g.s_diag) : ((id - noff) % g.s_diag) * g.nb + (id - noff) / g.s_diag;
        const int chunk = k / g.nb, jb = k - chunk * g.nb;
        it.kind = 1; it.jb = jb; it.kb = jb; it.chunk = chunk; it.nch = g.s_diag; it.gpc = g.gpc_diag; it.first = noff + 3 * sb + jb * g.s_diag; it.rank = g.n_off + jb;
    }
    return it;
}

template <bool FAST, bool DF>
__device__ __forceinline__ void mid_item(const MidArgs &g, double *sh, int tid, const MidItem &it, MidWalk &wk, f64x2 (&pbuf)[PMT_MID_D][8]) {
    if (it.kind == 0) {
        mid_body<false, FAST, DF>(g, sh, tid, it.jb, it.kb, it.chunk, it.nch, it.gpc, it.first, g.counters + it.rank * MCNT, wk, pbuf);
        return;
    }
    wk.pre = false;
    if constexpr (DF) wk.deferred = false;
    if (it.kind == 1) mid_body<true, FAST, DF>(g, sh, tid, it.jb, it.kb, it.chunk, it.nch, it.gpc, it.first, g.counters + it.rank * MCNT, wk, pbuf);
    else mid_constant(g, sh, tid);          // (nothing is pending: the item behind a deferring one is a body tile, MidWalk)
    mid_forget(pbuf);
}

// The STRIPS of the strip build (gram_mid_kernel<true, true, true>; launch_gram_mid: a shape of many body tiles, profiles/r25_gram_strips.txt).
// Strip i is the four consecutive ranks 4 i .. 4 i + 3 of the body walk; wave w of the workgroup that draws it owns rank 4 i + w for the
// WHOLE contraction: all 8-row groups 0, 1, 2, .. through mid_step with its own two scalar bases, its 64 accumulators the finished sums of
// its tile.  Between two strips of a workgroup no wave reads what another wrote but the ticket:
//   * the look-ahead of the walk, per wave: the workgroup holds one strip in hand; the last round of a wave's loop loads the first D groups
//     of ITS tile of that strip (the same lane offsets, both bases shifted); lane 0 of the workgroup draws the ticket behind it in front of
//     its last round and hands it over through one of two alternating words of LDS at the ONE barrier a strip ends with;
//   * the deferred write-out, per wave: behind its loop the wave leaves its accumulators in its own [a][lane] region (pitch MDP) and the
//     tile's column variables and row descriptors in its own map area, and writes the tile inside the first MSO_STEPS / D rounds of its
//     next loop (mid_so_op), the rest behind that loop where it is shorter — producer and consumer are the same wave, whose LDS operations
//     execute in order.  The area is written behind the loop, when nothing is pending any more: one area per wave is enough.
// A workgroup's last strip (the id in hand is no strip) writes its tiles at once: nothing is pending when the function returns, behind a
// barrier the LDS is the walk's (MidWalk).  Returns the id in hand, the workgroup's first item that is no strip.
__device__ __forceinline__ int mid_strips(const MidArgs &g, double *sh, int tid, int *slot, unsigned *ticket, int id0, f64x2 (&pbuf)[PMT_MID_D][8]) {
    constexpr int D = PMT_MID_D;
    constexpr int MSH_AT = MidLds<true>::SH;
    (void)MSH_AT;                                                  // (read by the trace build only)
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lm = lane & 15, lk = lane >> 4;
    // (stated uniform, as mid_body states its loop bounds: the loops and the rows' addresses stay scalar in every build, the traced one included)
    const int ns = __builtin_amdgcn_readfirstlane(g.n_strips), ngroups = __builtin_amdgcn_readfirstlane((int)(g.rows >> 3));      // (rows a multiple of 32 D: whole rounds, none ragged)
    double *rot = sh + wave * 512;
    const int pmo = MidLds<true>::QW + wave * MSA;
    static_assert(MidLds<true>::QW + 4 * MSA <= MidLds<true>::SH, "the four waves' map areas lie behind the partials");
    int id = blockIdx.x;                                           // (the launch has more strips than workgroups)
    if (tid == 0) slot[0] = id0 + 8 * (int)__hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    int hand = __builtin_amdgcn_readfirstlane(slot[0]), par = 1;
    int woq = MSO_STEPS;                                           // the pending tile's next write-out step; MSO_STEPS: none pending
    bool pre = false;                                              // the first D groups are in pbuf already
    int jb, kb;
    mid_tile_of<true>(4 * mid_xcd_rank(id, 0, ns) + wave, g.nb, jb, kb);
    for (;;) {
        MID_STAMP(0);
        const bool more = __builtin_amdgcn_readfirstlane((int)(hand < ns)) != 0;          // (the workgroup's: every wave sees the same ticket)
        woq = __builtin_amdgcn_readfirstlane(woq);
        int njb = jb, nkb = kb;
        if (more) mid_tile_of<true>(4 * mid_xcd_rank(hand, 0, ns) + wave, g.nb, njb, nkb);
        const int64_t cj0 = (int64_t)jb * MT, ck0 = (int64_t)kb * MT;
        double acc[MACC], qacc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < MACC; ++a) acc[a] = 0.0;
        unsigned voff[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) voff[t] = (unsigned)((((t < 4 ? cj0 : ck0) + 16 * (t & 3) + lm) * g.lda + 2 * lk) * 8);          // (whole panels)
        f64x2 cb[D];
        if (!pre) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                __builtin_amdgcn_sched_barrier(0);
                mid_load<false, true>(g, (int64_t)d * 8, lane, cj0, ck0, voff, pbuf[d], cb[d]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        const int ahead_at = more ? ngroups - D : -1;
        const int64_t shift_a = more ? ((int64_t)njb * MT - cj0) * g.lda * 8 : 0, shift_b = more ? ((int64_t)nkb * MT - ck0) * g.lda * 8 : 0;
        int s0 = 0;
        // the first rounds behind a strip: the same rounds with the wave's pending tile in them, a step per group
        static_assert(MSO_STEPS % D == 0, "whole rounds of write-out steps");
        for (; s0 + D <= ngroups && woq < MSO_STEPS; s0 += D, woq += D) {
            const bool ahead = s0 == ahead_at;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int64_t row = ahead ? (int64_t)d * 8 : (int64_t)min(s0 + d + D, ngroups - 1) * 8;
                const char *base = reinterpret_cast<const char *>(g.A + row);
                const MidWoAt at = {sh, woq + d, wave, pmo};
                mid_step<false, true, true>(g, rot, row, base + (ahead ? shift_a : 0), base + (ahead ? shift_b : 0), voff, pbuf[d], cb[d], g.sign, lane, acc, qacc, at);
            }
        }
        // the steady rounds; the last one of a strip with another in hand stands behind the loop, the ticket's draw in front of it (mid_body)
        const bool late = more && s0 + D <= ngroups;
        for (; s0 + D <= ngroups - (late ? D : 0); s0 += D) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int64_t row = (int64_t)min(s0 + d + D, ngroups - 1) * 8;
                const char *base = reinterpret_cast<const char *>(g.A + row);
                mid_step<false>(g, rot, row, base, base, voff, pbuf[d], cb[d], g.sign, lane, acc, qacc);
            }
        }
        unsigned drawn = 0;
        if (late) {
            if (tid == 0) drawn = __builtin_amdgcn_atomic_inc32(ticket, ~0u, __ATOMIC_RELAXED, "agent");
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const char *base = reinterpret_cast<const char *>(g.A + (int64_t)d * 8);
                mid_step<false>(g, rot, (int64_t)d * 8, base + shift_a, base + shift_b, voff, pbuf[d], cb[d], g.sign, lane, acc, qacc);
            }
        } else if (more && tid == 0) drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        MID_STAMP(1);
        // what the rounds did not take of the tile before this one goes out first; then this tile takes the region and the area
        mid_so_run(sh, woq, wave, pmo);
        double *mine = sh + MDEF + wave * MDPART + lane;
#pragma unroll
        for (int a = 0; a < MACC; ++a) mine[a * MDP] = acc[a];
        {
            u64 *area = reinterpret_cast<u64 *>(sh + pmo);
            const int64_t n = g.cols, j = cj0 + lane;
            const int64_t vc = g.xvar[ck0 + lane], vr = g.xvar[j];
            area[lane] = (u64)(g.moi ? map_var(g.varmap, vc) : vc);
            area[MT + 2 * lane] = (u64)(reinterpret_cast<u64 *>(g.out_quad) + (u64)(j * n - (j * (j - 1)) / 2 + (ck0 - j)) * 3);
            area[MT + 2 * lane + 1] = (u64)(g.moi ? map_var(g.varmap, vr) : vr);
        }
        // (the wave reads back what its other lanes wrote: its LDS operations execute in order; nothing moves across this point)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        woq = 0;
        if (!more) {
            mid_so_run(sh, woq, wave, pmo);
#ifdef PMT_MID_TRACE
            __builtin_amdgcn_s_waitcnt(0);
            MID_STAMP(6);
#endif
            return hand;
        }
        if (tid == 0) slot[par] = id0 + 8 * (int)drawn;
        __syncthreads();                                           // the strip's one barrier: the ticket
        id = hand; hand = __builtin_amdgcn_readfirstlane(slot[par]); par ^= 1;
        jb = njb; kb = nkb; pre = true;
        MID_STAMP(5);
    }
}

// One tile of a RIDER: a dense MOI constraint pack recorded beside the node (plan.hip) whose tiles the persistent workgroups draw from
// ticket word 9 once their XCD's Gram items have run out — a workgroup's last item ends 27 us (median, config 2) before the launch does,
// and nothing else can use its CU until it leaves.  The tile is affine_tile_kernel's own body (affine_tile.h) in the front of `sh`;
// what depends on the thread comes from a fresh thread id, so nothing of it is live across the Gram items.
__device__ __forceinline__ void mid_rider_tile(const AffineRider &r, int local, double *sh) {
    int t;
    asm volatile("v_mov_b32 %0, %1" : "=v"(t) : "v"((int)threadIdx.x));
    const int by = local / r.tiles_x, bx = local - by * r.tiles_x;
    double *tile = sh;
    u64 *vmx = reinterpret_cast<u64 *>(sh + TILE * PITCH);
#define MID_RIDE(NTV, TRV, NTLV)                                                                                                         \
    affine_tile_body<1, NTV, TRV, NTLV>(r.A, r.lda, r.rows, r.cols, r.xvar, r.b, r.sign, r.varmap, r.row_offset, r.out, r.out_consts,   \
                                        r.vec_in, r.vec_out, bx, by, t, tile, vmx)
    if (r.ntl) { if (r.tr == 32) MID_RIDE(true, 32, true); else MID_RIDE(true, 64, true); }
#ifdef PMT_TUNING
    else if (!r.nt) { if (r.tr == 32) MID_RIDE(false, 32, false); else MID_RIDE(false, 64, false); }
#endif
    else { if (r.tr == 32) MID_RIDE(true, 32, false); else MID_RIDE(true, 64, false); }
#undef MID_RIDE
}
static_assert(TILE * PITCH + TILE <= MQBUF, "a rider's tile and its variable-map row live in the front of the kernel's LDS");

// A launch of more than PMT_MID_G work items runs PERSISTENT (round 6c): PMT_MID_G workgroups, each walking items until none is left,
// instead of one workgroup per item — between two workgroups on a CU lay 2.5 us (the first one's stores drain, the dispatcher starts the
// next: tools/mid_trace.py, 8 times per CU at config 2); in a loop the next item's loads go out while the stores of the last drain.  The
// items keep their XCD: a workgroup with blockIdx % 8 = x takes the ids x, x + 8, x + 16, .. in order through ticket word x (what the
// hardware's round-robin over the XCDs gives a launch of one workgroup per item).  Nobody waits for anybody; the last workgroup to leave
// re-arms the tickets.  (Workgroups of an XCD that has run dry taking the other XCDs' items: measured, 7 us slower at config 2 —
// profiles/r14_item_boundaries.txt.)
// On the fast load path, in the unsplit body (s_off = 1: config 2's 2016 tiles) a workgroup holds ONE ticket in hand: the item after the
// one it runs is known while that one's main loop runs, so the loop's last round loads the next item's first groups (mid_body) and the
// ticket behind it is drawn under the tail — between two items stands one barrier instead of a ticket's round trip between two barriers
// and the first loads' latency.  The look-ahead stops with the body: from the first id in hand that lies in the split tails or the
// diagonal chunks on, a workgroup draws on demand, so nobody sits on a short item while others run dry.
// Round 20: such an item also DEFERS its tile (MidWalk, mid_body: hand-off) — the waves' sums, the doubling and the stores of a finished
// tile run inside the first rounds of the next item's loop instead of behind its own.
// A workgroup whose ticket has run dry then draws RIDER tiles (mid_rider_tile) until those are exhausted too, and leaves: Gram items
// always come first; the launch of one workgroup per item takes no riders.
// ST (with FAST and DF): the launch's first g.n_strips items are STRIPS (mid_strips); behind them the walk above, as the deferring build runs it.
template <bool FAST, bool DF, bool ST = false>
__global__ __launch_bounds__(256, PMT_MID_WPS) void gram_mid_kernel(MidArgs g) {
    static_assert(!ST || (FAST && DF), "strips: the fast load path, in the LDS of the deferring build");
    constexpr int MSH_AT = MidLds<DF>::SH;
    __shared__ double sh[MSH_AT + MID_TRACE_WORDS];
    __shared__ int next_id, ahead_id;
    const int tid = threadIdx.x;
    const int x = blockIdx.x & 7, per = gridDim.x >> 3;
#ifdef PMT_MID_TRACE
    if (tid == 0) for (int i = 0; i < MID_TRACE_WORDS; ++i) reinterpret_cast<unsigned long long *>(sh + MSH_AT)[i] = 0;
#endif
    f64x2 pbuf[PMT_MID_D][8];
    MidWalk wk = {};
    wk.ticket = g.tickets + x; wk.id0 = x + 8 * per; wk.slot = &ahead_id;
    if constexpr (DF) wk.woq = MWO_STEPS;
    const int wbody = ST ? g.n_off - g.n_tail - 3 * g.n_strips : (g.n_off - g.n_tail) * g.s_off;
    bool look = FAST && g.persist && g.s_off == 1;
    int id = blockIdx.x, hand = -1;                                // `hand`: the id behind `id`, once drawn
    if constexpr (ST) {
        // the strips first; behind them the workgroup draws on demand (few body tiles are left, if any: nothing to look ahead for)
        __shared__ int strip_slot[2];
        id = mid_strips(g, sh, tid, strip_slot, wk.ticket, wk.id0, pbuf);
        mid_forget(pbuf);
        look = false;
        __syncthreads();                                           // every wave has written its last tile: the LDS is the walk's
    }
    if (look) {
        if (tid == 0) next_id = wk.id0 + 8 * (int)__hip_atomic_fetch_add(wk.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        hand = next_id;
    }
    MidItem cur = mid_decode<DF, ST>(g, id);
    for (;;) {
        if constexpr (ST) { if (id >= g.total) break; }            // (a workgroup whose XCD has nothing behind its strips)
        wk.early = hand >= 0 && hand < wbody;                      // (ids ascend: id is a body item as well; s_off = 1: both are unsplit)
        wk.next_full = false;
        if (wk.early) {
            const MidItem nx = mid_decode<DF, ST>(g, hand);
            wk.next_full = (int64_t)(nx.kb + 1) * MT <= g.cols;
            wk.njb = nx.jb; wk.nkb = nx.kb; wk.nrank = nx.rank;
        }
        mid_item<FAST, DF>(g, sh, tid, cur, wk, pbuf);
        if (!g.persist) return;                                    // (one workgroup per item)
        if (!DF || !wk.deferred) __syncthreads();                         // the item's last LDS reads, and next_id's last readers (a deferred tile: the hand-off's barriers)
        if (wk.early) {
            id = hand; hand = wk.drawn;
            cur.jb = wk.njb; cur.kb = wk.nkb; cur.first = cur.rank = wk.nrank;          // (an unsplit body item like `cur`: kind, chunk, nch, gpc stay)
            continue;
        }
        if (hand >= 0) { id = hand; hand = -1; }
        else {
            if (tid == 0) next_id = wk.id0 + 8 * (int)__hip_atomic_fetch_add(wk.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            id = next_id;
        }
        if (id >= g.total) break;
        cur = mid_decode<DF, ST>(g, id);
    }
    // (nothing is pending here, MidWalk: a workgroup's last body item does not defer — the riders and the end of the walk need no write-out)
    if (g.rider_tiles > 0) {
        int mine = 0;
        for (;;) {
            __syncthreads();                                       // next_id's last readers; the last tile's LDS reads
            if (tid == 0) next_id = (int)__hip_atomic_fetch_add(g.tickets + 9, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            const int rt = __builtin_amdgcn_readfirstlane(next_id);
            if (rt >= g.rider_tiles) break;
            int k = 0;
            while (k + 1 < g.nriders && rt >= g.riders[k + 1].first_tile) ++k;
            mid_rider_tile(g.riders[k], rt - g.riders[k].first_tile, sh);
            ++mine;
        }
#ifdef PMT_MID_TRACE
        __builtin_amdgcn_s_waitcnt(0);
        if (tid == 0 && blockIdx.x < 1024) { g_mid_riders[blockIdx.x * 2] = (unsigned long long)mine; g_mid_riders[blockIdx.x * 2 + 1] = wall_clock64(); }
#endif
        (void)mine;                                                // (read by the trace build only)
    }
#ifdef PMT_MID_TRACE
    if (tid == 0 && blockIdx.x < 1024) {
        for (int i = 0; i < 7; ++i) g_mid_walk[blockIdx.x * 8 + i] = reinterpret_cast<unsigned long long *>(sh + MSH_AT)[i];
        g_mid_walk[blockIdx.x * 8 + 7] = wall_clock64();
    }
#endif
    if (tid == 0) {
        const unsigned gone = __hip_atomic_fetch_add(g.tickets + 8, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (gone == gridDim.x - 1) {
#pragma unroll
            for (int i = 0; i < 10; ++i) __hip_atomic_store(g.tickets + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// The STRIP build is instantiated in a translation unit of its own, gram_mid_strips.hip, which is this file without its host part: with
// the third build beside it the compiler re-associates address arithmetic in <true, true, false> (21 instructions more), and the builds
// without strips are to stay the kernels they were, instruction for instruction (tools/isa_diff.py; profiles/r25_gram_strips.txt).
int launch_gram_mid_strips(const MidArgs &g, unsigned grid, hipStream_t s);
#ifdef PMT_MID_STRIPS_TU
int launch_gram_mid_strips(const MidArgs &g, unsigned grid, hipStream_t s) {
    PMT_LAUNCH_NAMED("gram_mid_kernel", (gram_mid_kernel<true, true, true>), dim3(grid), dim3(256), 0, s, g);
    return check_launch("gram_mid_kernel");
}
#else
// c'c alone, in the same order 5 (the staged host delivery of a shape the one-launch form otherwise takes: gram.hip)
__global__ __launch_bounds__(256) void gram_mid_constant_kernel(MidArgs g) {
    __shared__ double sh[8];
    mid_constant(g, sh, threadIdx.x);
}
int launch_gram_mid_constant(const double *b, int sign, int64_t rows, double *out_const, hipStream_t s) {
    MidArgs g = {};
    g.rows = rows; g.b = (b && sign) ? b : nullptr; g.sign = g.b ? sign : 0; g.out_const = out_const;
    PMT_LAUNCH_NAMED("gram_mid_constant_kernel", gram_mid_constant_kernel, dim3(1), dim3(256), 0, s, g);
    return check_launch("gram_mid_constant_kernel");
}

size_t gram_mid_workspace_bytes(int64_t rows, int64_t cols) {
    if (cols <= 0) return 0;
    const MidPlan p = mid_plan(rows, cols);
    return sizeof(double) * (size_t)p.wgs * MSTRIDE;
}
bool gram_mid_persistent(int64_t rows, int64_t cols) { return cols > 0 && rows > 0 && mid_plan(rows, cols).wgs >= 2 * PMT_MID_G; }
// The shape's plan lets tiles be deferred (MidWalk): the persistent walk over an unsplit body.  *whole_rounds: the row count gives every
// wave whole rounds of 8-row groups (rows a multiple of 32 PMT_MID_D), so on the fast load path the launch takes the deferring build
// (gram_mid_kernel<true, true>) and every body tile of two whole panels but a workgroup's last is deferred; otherwise the launch is the
// build without deferred tiles and every item takes the immediate path.
static bool mid_plan_defers(const MidPlan &p) {          // (two body tiles per workgroup: with one, nothing is ever pending)
    return p.wgs >= 2 * PMT_MID_G && p.s_off == 1 && p.n_off - p.n_tail >= 2 * PMT_MID_G;
}
static bool mid_rows_defer(int64_t rows) { return rows % (32 * PMT_MID_D) == 0; }
bool gram_mid_defers(int64_t rows, int64_t cols, bool *whole_rounds) {
    if (whole_rounds) *whole_rounds = false;
    if (cols <= 0 || rows <= 0) return false;
    const bool can = mid_plan_defers(mid_plan(rows, cols));
    if (whole_rounds) *whole_rounds = can && mid_rows_defer(rows);
    return can;
}
// How many of the body tiles go in STRIPS (mid_strips), from (rows, cols) alone: 0, or all whole strips from the front of the walk — the
// tiles left over (at most three), the tails, the diagonal chunks and the constant stay the items they were, behind the strips in the
// ticket order, so the end of the launch keeps its fine-grained work.  A shape takes them where tiles would be deferred with whole rounds
// on every wave, every panel is whole, there are at least 1.5 strips per workgroup (with one nothing is ever pending; up to 4096 columns
// that leaves no room for a smaller count of whole rounds of strips: 2016 body tiles are 1.97 rounds) — and where the estimate says so,
// in the style of mid_plan: a strip is four tile times and ~2 us, a tile of its own a tile time and ~5 us (3.5 beside its loop, 1.5 in
// the write-out rounds: profiles/r20_deferred_tile.txt); strips run in rounds of PMT_MID_G, the rest fills the CUs evenly.  Config 2:
// 504 strips, 994 us against 1029 for single tiles by this estimate (measured: -22 us per step, profiles/r25_gram_strips.txt); 4096 x 3584
// (384 strips: half of the CUs idle for a whole strip) stays as it is.
static int mid_plan_strips(const MidPlan &p, int64_t rows, int64_t cols) {
    if (!mid_plan_defers(p) || !mid_rows_defer(rows) || cols % MT) return 0;
    const int nbody = p.n_off - p.n_tail, ns = nbody / 4;
    if (2 * ns < 3 * PMT_MID_G) return 0;
    const double tile_us = PMT_MID_TAIL_US * (double)cdiv(cdiv(rows, 8), 4);
    const double chunk_us = PMT_MID_TAIL_US * 0.69 * (double)cdiv(p.gpc_diag, 4) + 5.0 + (p.s_diag > 1 ? 1.0 : 0.0);
    const double rest_us = (double)p.n_tail * p.s_tail * (PMT_MID_TAIL_US * (double)cdiv(p.gpc_tail, 4) + 6.0) + (double)p.nb * p.s_diag * chunk_us;
    const double strip_us = 4.0 * tile_us + 2.0, item_us = tile_us + 5.0;
    const double t_strips = std::max((double)cdiv(ns, PMT_MID_G) * strip_us, ((double)ns * strip_us + (double)(nbody - 4 * ns) * item_us + rest_us) / PMT_MID_G);
    const double t_items = ((double)nbody * item_us + rest_us) / PMT_MID_G;
    return t_strips < t_items ? ns : 0;
}
bool gram_mid_strips(int64_t rows, int64_t cols, int *strips, int *tiles_in_strips) {
    const int ns = cols > 0 && rows > 0 ? mid_plan_strips(mid_plan(rows, cols), rows, cols) : 0;
    if (strips) *strips = ns;
    if (tiles_in_strips) *tiles_in_strips = 4 * ns;
    return ns > 0;
}
int gram_mid_counters(int64_t cols) { const int nb = (int)cdiv(cols, MT); return MCNT * (nb * (nb + 1) / 2) + 16; }      // (+ the tickets)

// the whole node in one launch; `counters`: gram_mid_counters(cols) zeroed words owned by the calling stream (streams.h: SideStream)
int launch_gram_mid(const double *A, int64_t lda, int64_t rows, int64_t cols, const int64_t *xvar, const double *b, int sign, int moi,
                    const int64_t *varmap, pmt_quadratic_term *out_quad, double *out_csc, double alpha, pmt_linear_term *out_lin,
                    double *out_const, void *workspace, unsigned *counters, const void *riders, int nriders, int rider_tiles, hipStream_t s) {
    if (!workspace || !counters) return fail(PMT_INVALID_ARGUMENT, "quad_gram: workspace required");
    const MidPlan p = mid_plan(rows, cols);
    MidArgs g;
    g.A = A; g.lda = lda; g.rows = rows; g.cols = cols; g.b = (b && sign) ? b : nullptr; g.sign = g.b ? sign : 0;
    g.xvar = xvar; g.varmap = varmap; g.moi = moi; g.out_quad = reinterpret_cast<QT *>(out_quad); g.out_csc = out_csc; g.alpha = alpha;
    g.out_lin = reinterpret_cast<LT *>(out_lin); g.out_const = out_const;
    g.nb = p.nb; g.n_off = p.n_off; g.s_off = p.s_off; g.s_diag = p.s_diag; g.gpc_off = p.gpc_off; g.gpc_diag = p.gpc_diag;
    g.n_tail = p.n_tail; g.s_tail = p.s_tail; g.gpc_tail = p.gpc_tail;
    g.ws = reinterpret_cast<double *>(workspace); g.counters = counters;
    g.xcd = rows * cols * 8 > ((int64_t)4 << 20);      // (a matrix that fits one L2 is all there on every XCD: 1024 x 512 23.0 against 25.6 us)
    const bool fast = (reinterpret_cast<uintptr_t>(A) & 15) == 0 && (lda & 1) == 0 && (reinterpret_cast<uintptr_t>(g.b) & 15) == 0 &&
                      (uint64_t)lda * (uint64_t)cols * 8 < (1ull << 32);
    g.total = p.wgs;
    g.persist = p.wgs >= 2 * PMT_MID_G;
    g.tickets = counters + gram_mid_counters(cols) - 16;
    // riders (a plan's table, gram.hip: mid_node) travel with the persistent form only: plan.hip lets nobody ride another
    const bool ride = g.persist && riders && nriders > 0 && rider_tiles > 0;
    g.riders = ride ? static_cast<const AffineRider *>(riders) : nullptr; g.nriders = ride ? nriders : 0; g.rider_tiles = ride ? rider_tiles : 0;
    const unsigned grid = g.persist ? (unsigned)PMT_MID_G : (unsigned)p.wgs;
    // the deferring form where tiles will be deferred (gram_mid_defers + what the call adds: the fast load path, terms and nothing else)
    const bool df = fast && mid_plan_defers(p) && mid_rows_defer(rows) && out_quad && !out_csc;
    // ... and the strip build where the shape's plan has strips (gram_mid_strips): its ids are the strips, then the items that are left
    g.n_strips = df ? mid_plan_strips(p, rows, cols) : 0;
    g.total = p.wgs - 3 * g.n_strips;
    // (instantiated in this order, the builds without deferred tiles are kernels 1 and 2 of the file as in the parent: tools/isa_diff.py)
    if (fast && !df) PMT_LAUNCH_NAMED("gram_mid_kernel", (gram_mid_kernel<true, false>), dim3(grid), dim3(256), 0, s, g);
    else if (!fast) PMT_LAUNCH_NAMED("gram_mid_kernel", (gram_mid_kernel<false, false>), dim3(grid), dim3(256), 0, s, g);
    else if (!g.n_strips) PMT_LAUNCH_NAMED("gram_mid_kernel", (gram_mid_kernel<true, true>), dim3(grid), dim3(256), 0, s, g);
    else return launch_gram_mid_strips(g, grid, s);
    return check_launch("gram_mid_kernel");
}
#endif          // PMT_MID_STRIPS_TU

}  // namespace pmt
