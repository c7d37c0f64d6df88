// Horizon stage costs: sum_t transpose(x_t (+|-) v_t) * Q_t * (x_t (+|-) v_t) over T pairwise disjoint Variable vectors as ONE canonical MOI
// function, from one launch (pmt_quad_stages_f64).  What a model-predictive controller writes: T = 10 .. a few hundred stages, two or three
// weight matrices shared by all of them, one reference vector per stage.  In the reference every stage is matvecmul! over the affine vector
// (src/functions.jl:800-822) and vecdot! (:702-709 over :548-576) — bilinearmul! (:840-858) for a plain stage —, the stages are added with
// add! (:244), and canonicalize! (:381-386) and the MOI copy (src/moi_interop.jl:45-62) follow; no pair (j, k) is shared between two stages.
//
// One workgroup of 256 threads per stage, persistent: workgroup g takes the stages g, g + G, .. of a device table of descriptors
// (pmt_quad_stage).  No workgroup waits for another, no atomics, no workspace.  A stage is walked exactly as batch_form_kernel
// (batch_form.hip) walks an instance: the 64 x 64 tile pairs (J <= K), both source tiles read along their columns with every load of a tile
// issued before the first value is looked at, the transpose-add through an LDS tile of pitch 65 doubles, one thread per row adding the row
// chains and — off the diagonal — one per column the column chains into P[B][j] in LDS (n <= 256); after the last tile one thread per j adds
// the blocks in order, the 256-entry tree gives the stage's constant.  Summation order and operations are those include/parametron_hip.h
// fixes for pmt_quad_form_shift_f64, so a stage's slice equals what that node writes for the stage alone, bit for bit.
// What is new against that kernel:
//   - Q is named by the descriptor (column-major, leading dimension ldq) and shared by many stages: behind the first stages it comes from L2
//     and the launch is bound by its writes;
//   - the stage's index words vm[xvar[j]] are fetched once into LDS (2 KB) — asked for at the top of the stage, looked up through the varmap
//     behind the first tile's loads, read by the epilogues;
//   - the epilogue writes 24-byte term structs row by row and 16-byte linear terms through wave_write_words (common.h), as quad_form_tile
//     (form.hip) and sparse_form_kernel do: a slice starts at any 8-byte address.
// The stages' constants go to stage_consts[t]; a second launch of one workgroup, ordered by the stream alone, adds them in S_d's order.
// pmt_quad_stages_terms_f64 is the same pair of launches with a weight and a linear term dot(c_t, x_t) per stage and scalar constants
// beside the stages, from two more device tables.  pmt_quad_stages_diag_f64 adds identity-weighted stage costs: a stage without a matrix
// (W_t * dot(x_t (+|-) v_t, x_t (+|-) v_t): n quadratic terms, no tile walk) and a diagonal term riding on a form stage, from a third
// table.  The kernels are templates on MODE; the instantiations QS_PLAIN and QS_TERMS are the device code of the two older entry points
// unchanged (tools/isa_diff.py).  pmt_quad_stages_csc_f64 (QS_CSC) is pmt_quad_stages_diag_f64 with another quadratic epilogue: a device-resident
// solver's CSC values of the block-diagonal upper-triangular P — 8 bytes per entry, no index words — instead of 24-byte term structs.
// LDS: 33280 (tile) + 8192 (P) + 2048 (c) + 2048 (tree) + 2048 (index words) + 2048 (lin) = 49664 bytes: three workgroups per CU.
#include <algorithm>
#include <type_traits>
#include <vector>

#include "common.h"

namespace pmt {

namespace {

constexpr int QS_TILE = 64;
constexpr int QS_THREADS = 256;
constexpr int QS_MAX_N = 256;
constexpr int QS_MAX_NB = QS_MAX_N / QS_TILE;
constexpr int QS_WG_PER_CU = 3;
static_assert(QS_MAX_N == PMT_QUAD_STAGES_MAX_N, "the header's bound is the kernel's");
static_assert(QS_MAX_N <= QS_THREADS, "one thread per j adds the blocks; the tree takes one product per thread");
static_assert(sizeof(pmt_quad_stage) == 56, "pmt_quad_stage: 56 bytes, no padding (the ctypes and Julia mirrors)");
static_assert(sizeof(pmt_quad_stage_terms) == 40 && sizeof(pmt_quad_stage_const) == 24, "pmt_quad_stage_terms / _const: 40 / 24 bytes, no padding");
static_assert(sizeof(pmt_quad_stage_diag) == 32, "pmt_quad_stage_diag: 32 bytes, no padding");

// the entry point an instantiation serves: pmt_quad_stages_f64, pmt_quad_stages_terms_f64, pmt_quad_stages_diag_f64, pmt_quad_stages_csc_f64
constexpr int QS_PLAIN = 0, QS_TERMS = 1, QS_DIAG = 2, QS_CSC = 3;

struct QuadStagesArgs {
    const pmt_quad_stage *stages; int64_t T;
    const int64_t *varmap;
    QT *quad; LT *lin;
    double *consts, *cst;
};

// pmt_quad_stages_terms_f64: the stages' weights and linear terms, and the table of scalar constants added behind the tree
struct QuadStagesTermsArgs : QuadStagesArgs {
    const pmt_quad_stage_terms *terms;
    const pmt_quad_stage_const *cterms; int64_t nconsts;
};
// pmt_quad_stages_diag_f64: the stages' riders (NULL: no stage has one)
struct QuadStagesDiagArgs : QuadStagesTermsArgs {
    const pmt_quad_stage_diag *diags;
};
// pmt_quad_stages_csc_f64: P's CSC values (quad is unused) and the sense they are multiplied by
struct QuadStagesCscArgs : QuadStagesDiagArgs {
    double *pvalues; double alpha;
};
template <int MODE> using QsArgs = std::conditional_t<MODE == QS_CSC, QuadStagesCscArgs, std::conditional_t<MODE == QS_DIAG, QuadStagesDiagArgs, std::conditional_t<MODE == QS_TERMS, QuadStagesTermsArgs, QuadStagesArgs>>>;

}  // namespace

// TERMS (pmt_quad_stages_terms_f64): stage t is weighted and may carry a linear term (g.terms[t], pmt_quad_stage_terms): W_t multiplies
// every value word, the linear coefficients and the constant as they are written, W_c * c_t[j] is added to the weighted linear
// coefficient; the chains (part, cvec, the tree) stay unweighted, so lin_j and cc_t keep the order of the unweighted stage.  No LDS of
// its own.  The instantiation without TERMS is the kernel of pmt_quad_stages_f64 as it was (tools/isa_diff.py).
// QS_DIAG (pmt_quad_stages_diag_f64) is TERMS with two more kinds of stage, in pmt_quad_gram_sum_f64's order for a PMT_LSQ_DIAG term
// (gram_sum.hip: sum_diag_shift_at, gram_sum_aux, gram_sum_const):
//   - an identity stage (Q == NULL) has no tiles: behind the prologue's loads it writes n terms (2*W_t, var_j, var_j), lin[j] =
//     W_t*(2*c_j) (+ W_c*c_t[j]) — W_c*c_t[j] alone without v, +0.0 with neither — and W_t*S, S = sum_j c_j*c_j from the 256-entry tree;
//   - a rider (g.diags[t].present) adds (2*W_d) to the stage's n diagonal coefficients as they are written, W_d*(2*c^d_j) to lin[j] between
//     W_t*lin_j and W_c*c_t[j], and W_d*S to the constant from one more pass of the tree over red[].
// QS_CSC (pmt_quad_stages_csc_f64) is QS_DIAG with the quadratic epilogue of a CSC hand-off: quad_at counts doubles of g.pvalues, and the
// coefficient c(j,k) QS_DIAG writes at tri(j,k) goes, times alpha, to k(k+1)/2 + j — column k's rows j0 .. min(j0 + jw - 1, k) of a tile are
// one contiguous run, a wave per column with the rows on the lanes, two to a lane for the 16-byte stores (tile[jj][kk] with jj = 2 lane,
// 2 lane + 1: a stride of 130 doubles, lanes l and l + 16 share a bank: two-way at the most); an identity stage writes alpha*(2*W_t) n times.  The index words var[] serve the linear terms alone.
template <int MODE>
__global__ __launch_bounds__(QS_THREADS, MODE >= QS_DIAG ? QS_WG_PER_CU : 1) void quad_stages_kernel(QsArgs<MODE> g) {
    constexpr bool TERMS = MODE != QS_PLAIN, DIAG = MODE >= QS_DIAG, CSC = MODE == QS_CSC;
    typedef unsigned long long u64w;
    __shared__ double tile[QS_TILE][QS_TILE + 1];
    __shared__ double part[QS_MAX_NB][QS_MAX_N];          // P[B][j]
    __shared__ double cvec[QS_MAX_N];
    __shared__ double red[QS_THREADS];
    __shared__ int64_t var[QS_MAX_N];                     // vm[xvar[j]]
    __shared__ double linv[QS_MAX_N];
    const int tid = threadIdx.x;
    const int64_t *__restrict__ varmap = g.varmap;

    for (int64_t t = blockIdx.x; t < g.T; t += gridDim.x) {
        const pmt_quad_stage d = g.stages[t];
        [[maybe_unused]] pmt_quad_stage_terms e;          // (asked for with the descriptor: one round trip for both)
        if constexpr (TERMS) e = g.terms[t];
        [[maybe_unused]] pmt_quad_stage_diag dg = {};     // (no table: no stage has a rider)
        if constexpr (DIAG) {
            if (g.diags) dg = g.diags[t];
        }
        const bool ident = DIAG && d.Q == nullptr, rider = DIAG && dg.present != 0, rider_vec = rider && dg.sign != 0;
        const int n = d.n, nt = ident ? 0 : (n + QS_TILE - 1) / QS_TILE;
        const int64_t ldq = d.ldq;
        const double *__restrict__ Q = d.Q;
        const bool shift = d.sign != 0;
        [[maybe_unused]] QT *__restrict__ oq = nullptr;
        [[maybe_unused]] double *__restrict__ op = nullptr;
        if constexpr (CSC) op = g.pvalues + d.quad_at;
        else oq = g.quad + d.quad_at;
        // v and the index words are asked for now and looked at behind the first tile's loads: no round trip of their own in front of the
        // tiles (every thread loads, thread t >= n the last entry again)
        const int ct = tid < n ? tid : n - 1;
        double pv = 0.0;
        if (shift) pv = d.vec[ct];
        int64_t xv = d.xvar[ct];
        bool pending = true;
        // the two weight Parameters and the thread's c_t[j] are asked for here too and looked at behind the first tile's loads.  No load is
        // conditional: a pointer the entry does not give is replaced by the address of the entry's own scale, and the value dropped
        double wt = 1.0, wc = 0.0, cl = 0.0, wv = 0.0, wcv = 0.0;
        if constexpr (TERMS) {
            const double *own = &g.terms[t].scale;
            wv = *(e.weight ? e.weight : own);
            wcv = *(e.lin_weight ? e.lin_weight : own);
            cl = *(e.lin_vec ? e.lin_vec + ct : own);
        }
        // a rider's weight Parameter likewise (its vector is asked for behind the tiles: the walk has no registers to spare for it)
        [[maybe_unused]] double wd = 0.0, cd = 0.0, wdv = 0.0;
        if constexpr (DIAG) wdv = *(rider && dg.weight ? dg.weight : &g.terms[t].scale);

        for (int bj = 0; bj < nt; ++bj) {
            for (int bk = bj; bk < nt; ++bk) {
                const bool diagonal = bk == bj;
                // (the lane's coordinates are made opaque per tile: derived from loop invariants, the compiler otherwise keeps every address
                // and predicate of the unrolled body below alive across the whole stage loop)
                int lane = tid & 63, wave = tid >> 6;
                asm volatile("" : "+v"(lane), "+v"(wave));
                const int j0 = bj * QS_TILE, k0 = bk * QS_TILE;
                // lower[i] = Q[k0 + lane, j0 + wave + 4 i] (k on the lanes); upper[i] = Q[j0 + lane, k0 + wave + 4 i] (j on the lanes)
                // Out-of-range entries are 0.0: the load goes to the stage's last row / column instead and is dropped, so no load is
                // conditional.  All loads of a tile are issued before the first value is looked at (landed).
                double lower[16], upper[16];
                const int rk = k0 + lane, rj = j0 + lane;
                const int ork = rk < n ? rk : n - 1, orj = rj < n ? rj : n - 1;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int c = j0 + wave + 4 * i;
                    lower[i] = Q[ork + (int64_t)(c < n ? c : n - 1) * ldq];
                }
                if (!diagonal) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int c = k0 + wave + 4 * i;
                        upper[i] = Q[orj + (int64_t)(c < n ? c : n - 1) * ldq];
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
                if (pending) {                          // c = 0.0 (+|-) v and the index words; read behind this tile's barriers
                    asm volatile("" : "+v"(pv), "+v"(xv));      // (looked at here, not in front of the loads)
                    if (tid < n) {
                        var[tid] = varmap[xv - 1];
                        if (shift) cvec[tid] = signed_const(pv, d.sign);
                    }
                    if constexpr (TERMS) {              // W_t = scale * (*weight) or scale, W_c likewise: one rounded product each
                        asm volatile("" : "+v"(wv), "+v"(wcv), "+v"(cl));
                        wt = e.weight ? e.scale * wv : e.scale;
                        wc = e.lin_weight ? e.lin_scale * wcv : e.lin_scale;
                    }
                    if constexpr (DIAG) {               // W_d likewise
                        asm volatile("" : "+v"(wdv));
                        wd = dg.weight ? dg.scale * wdv : dg.scale;
                    }
                    pending = false;
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
                const int kw = n - k0 < QS_TILE ? n - k0 : QS_TILE, jw = n - j0 < QS_TILE ? n - j0 : QS_TILE;
                if (shift) {
                    // plain multiplies and adds, ascending, the first product starting the chain
                    if (wave == 0 && lane < jw) {
                        part[bk][j0 + lane] = chain(kw, [&](int kk) { const double a = tile[lane][kk]; return (diagonal && kk == lane) ? 2 * a : a; },
                                                       [&](int kk) { return cvec[k0 + kk]; });
                    } else if (wave == 1 && !diagonal && lane < kw) {
                        part[bj][k0 + lane] = chain(jw, [&](int jj) { return tile[jj][lane]; }, [&](int jj) { return cvec[j0 + jj]; });
                    }
                }
                // the quadratic terms: row j holds its columns k >= j; this tile's piece of it, a wave per row segment, 16-byte stores
                [[maybe_unused]] const int ke = k0 + kw;
                if constexpr (CSC) {
                    // P's values: column k holds its rows j <= k; this tile's piece of it, a wave per column, 16-byte stores
                    for (int r = 0; r < 16; ++r) {
                        const int kk = wave * 16 + r, k = k0 + kk;
                        if (k >= n) break;
                        wave_write_words<1>(reinterpret_cast<u64w *>(op + ((int64_t)k * (k + 1) / 2 + j0)), diagonal ? kk + 1 : jw, lane, [&](int q) -> u64w {
                            const double v = tile[q][kk];
                            const bool dj = diagonal && q == kk;                                      // the column's last value is its diagonal one
                            double c = wt * (dj ? 2 * v : v);
                            if (rider && dj) c = c + 2 * wd;
                            return (u64w)__double_as_longlong(g.alpha * c);
                        });
                    }
                } else {
                    for (int r = 0; r < 16; ++r) {
                        const int jj = wave * 16 + r, j = j0 + jj;
                        if (j >= n) break;
                        const int ks = k0 > j ? k0 : j;
                        if (ke <= ks) continue;
                        const int off = ks - k0;
                        const u64w rowvar = (u64w)var[j];
                        wave_write_words<3>(reinterpret_cast<u64w *>(oq + tri_pos(n, j, ks)), ke - ks, lane, [&](int q) -> u64w {
                            const int e = q / 3, f = q - 3 * e;
                            if (f == 1) return rowvar;
                            if (f == 2) return (u64w)var[k0 + off + e];
                            const double v = tile[jj][off + e];
                            const double c = (diagonal && e == 0) ? 2 * v : v;                        // the row's first term is its diagonal term
                            if constexpr (DIAG) {
                                if (rider && diagonal && e == 0) return (u64w)__double_as_longlong(wt * c + 2 * wd);
                            }
                            return (u64w)__double_as_longlong(TERMS ? wt * c : c);
                        });
                    }
                }
                __syncthreads();
            }
        }

        // lin_j = ((P[0][j] + P[1][j]) + ..) + P[nb-1][j]; T_t by 256 chains onto 0.0 (n <= 256: one product each), then the halving tree
        if constexpr (DIAG) {
            if (rider_vec) cd = signed_const(dg.vec[ct], dg.sign);      // c^d = 0.0 (+|-) v^d
            if (ident) {                                  // no tile in front of which to look at the prologue's loads: here
                if (tid < n) {
                    var[tid] = varmap[xv - 1];
                    if (shift) cvec[tid] = signed_const(pv, d.sign);
                }
                wt = e.weight ? e.scale * wv : e.scale;
                wc = e.lin_weight ? e.lin_scale * wcv : e.lin_scale;
            }
        }
        double prod = 0.0;
        if (DIAG && ident) {
            if (tid < n) {
                double lin = 0.0;
                if (shift) {
                    const double c = cvec[tid];
                    lin = wt * (2 * c);
                    if (e.lin_vec) lin = lin + wc * cl;
                    prod = c * c;
                } else if (e.lin_vec) {
                    lin = wc * cl;                        // the first contributor starts the chain: a -0.0 survives
                }
                linv[tid] = lin;
            }
        } else if (tid < n) {
            double lin = 0.0;
            if (shift) {
                lin = part[0][tid];
                for (int b = 1; b < nt; ++b) lin = lin + part[b][tid];
                prod = cvec[tid] * lin;
            }
            if constexpr (TERMS) {                        // W_t * lin_j (a plain stage: W_t * +0.0), then + W_c * c_t[j]
                lin = wt * lin;
                if constexpr (DIAG) {
                    if (rider_vec) lin = lin + wd * (2 * cd);
                }
                if (e.lin_vec) lin = lin + wc * cl;
            }
            linv[tid] = lin;
        }
        double chain = 0.0;
        if (shift && tid < n) chain = chain + prod;
        red[tid] = chain;
        __syncthreads();
        {
            // the linear terms: wave w writes the terms 64 w .. of the stage's slice
            const int lane = tid & 63, w0 = (tid >> 6) * 64;
            if (w0 < n) {
                const int cnt = n - w0 < 64 ? n - w0 : 64;
                wave_write_words<2>(reinterpret_cast<u64w *>(g.lin + d.lin_at + w0), cnt, lane, [&](int q) -> u64w {
                    const int e = w0 + (q >> 1);
                    return (q & 1) ? (u64w)var[e] : (u64w)__double_as_longlong(linv[e]);
                });
                if (DIAG && ident) {                      // and the terms (2*W_t, var_j, var_j) 64 w .. of an identity stage
                    if constexpr (CSC) {                  // (P's values: alpha*(2*W_t) 64 w ..)
                        const u64w w2 = (u64w)__double_as_longlong(g.alpha * (2 * wt));
                        wave_write_words<1>(reinterpret_cast<u64w *>(op + w0), cnt, lane, [&](int) -> u64w { return w2; });
                    } else {
                        const u64w w2 = (u64w)__double_as_longlong(2 * wt);
                        wave_write_words<3>(reinterpret_cast<u64w *>(oq + w0), cnt, lane, [&](int q) -> u64w {
                            const int e = q / 3;
                            return q == 3 * e ? w2 : (u64w)var[w0 + e];
                        });
                    }
                }
            }
        }
        for (int h = QS_THREADS / 2; h > 0; h >>= 1) {
            if (tid < h) red[tid] = red[tid] + red[tid + h];
            __syncthreads();
        }
        if constexpr (DIAG) {
            // an identity stage: W_t * S, or +0.0 without v; a rider with v: W_t * cc_t, then + W_d * S from a second pass of the tree
            double sc = 0.0;
            if (ident) {
                if (shift) sc = wt * red[0];
            } else {
                sc = wt * (shift ? 0.5 * red[0] : 0.0);
            }
            if (rider_vec) {
                __syncthreads();                          // every thread has read red[0]
                double sq = 0.0;
                if (tid < n) sq = sq + cd * cd;
                red[tid] = sq;
                __syncthreads();
                for (int h = QS_THREADS / 2; h > 0; h >>= 1) {
                    if (tid < h) red[tid] = red[tid] + red[tid + h];
                    __syncthreads();
                }
                sc = sc + wd * red[0];
            }
            if (tid == 0) g.consts[t] = sc;
        } else if (tid == 0) {
            const double cc = shift ? 0.5 * red[0] : 0.0;
            g.consts[t] = TERMS ? wt * cc : cc;
        }
        __syncthreads();                                  // the next stage reuses cvec, part, red, var and linv
    }
}

// Behind quad_stages_kernel on the stream: one workgroup adds the T stage constants in S_d's order (gram_sum.hip: 256 chains onto 0.0,
// chain c taking the stages c, c + 256, .. in order, then the halving tree).  T == 0 gives 0.0.  TERMS: one thread then adds the scalar
// constants in table order, s = s + W_i * (value_i or 1.0).
template <bool TERMS>
__global__ __launch_bounds__(QS_THREADS) void quad_stages_const_kernel(QsArgs<TERMS ? QS_TERMS : QS_PLAIN> g) {
    __shared__ double red[QS_THREADS];
    const int tid = threadIdx.x;
    const double *__restrict__ c = g.consts;
    double s = 0.0;
    for (int64_t t = tid; t < g.T; t += QS_THREADS) s = s + c[t];
    red[tid] = s;
    __syncthreads();
    for (int h = QS_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] = red[tid] + red[tid + h];
        __syncthreads();
    }
    if constexpr (TERMS) {
        if (tid == 0) {
            s = red[0];
            for (int64_t i = 0; i < g.nconsts; ++i) {
                const pmt_quad_stage_const k = g.cterms[i];
                const double w = k.weight ? k.scale * *k.weight : k.scale;
                s = s + w * (k.value ? *k.value : 1.0);
            }
            *g.cst = s;
        }
    } else {
        if (tid == 0) *g.cst = red[0];
    }
}

// slices [at, at + len) of the stages, sorted by their start, stay inside [0, total) and do not overlap
static bool qs_slices_ok(std::vector<std::pair<int64_t, int64_t>> &s, int64_t total) {
    std::sort(s.begin(), s.end());
    int64_t end = 0;
    for (const auto &p : s) {
        if (p.first < end || p.second > total - p.first) return false;
        end = p.first + p.second;
    }
    return true;
}

// the stage launch (none for T == 0) and the constant's, behind each other on the stream
// (QS_DIAG adds its constants as QS_TERMS does: the same second kernel)
template <int MODE>
static int qs_launch(void *stream, const QsArgs<MODE> &g) {
    constexpr bool TERMS = MODE != QS_PLAIN;
    return dispatch(stream, [=](hipStream_t s) {
        if (g.T > 0) {
            // three workgroups per CU stay resident (LDS); each walks the stages blockIdx.x, blockIdx.x + G, ..
            const dim3 grid((unsigned)std::min<int64_t>(g.T, (int64_t)QS_WG_PER_CU * cu_count()));
            PMT_LAUNCH(quad_stages_kernel<MODE>, grid, dim3(QS_THREADS), 0, s, g);
            const int rc = check_launch("quad_stages_kernel");
            if (rc != PMT_OK) return rc;
        }
        const QsArgs<TERMS ? QS_TERMS : QS_PLAIN> gc = g;
        PMT_LAUNCH(quad_stages_const_kernel<TERMS>, dim3(1), dim3(QS_THREADS), 0, s, gc);
        return check_launch("quad_stages_const_kernel");
    });
}

}  // namespace pmt

using namespace pmt;

// The host side of the four entry points.  They share one check of the host tables (qs_check), the argument checks in front of the launch and
// the launch itself (qs_run over the most-derived argument struct, of which qs_launch<MODE> takes its slice); the MODE says what an entry has
// beyond the last:
//   QS_PLAIN  pmt_quad_stages_f64        the stage table
//   QS_TERMS  pmt_quad_stages_terms_f64  + the stages' terms and the table of constants
//   QS_DIAG   pmt_quad_stages_diag_f64   + the riders (the table may be NULL), and a stage without a matrix is an identity stage
//   QS_CSC    pmt_quad_stages_csc_f64    the same tables; P's CSC values times alpha instead of the quadratic terms
// A check's message keeps the prefix of the entry that introduced its table, whichever check is called; a launch's says the entry's own name.

// pmt_quad_stages_check .. pmt_quad_stages_csc_check: the counts, the stage table, the slices, the side tables, the riders, in this order.
// Tables a mode does not have are NULL / 0 and not looked at.  From QS_DIAG on a stage without a matrix is an identity stage of n quadratic
// terms (QS_CSC: n values; a form stage's n(n+1)/2 likewise count doubles there), its ldq not looked at
static int qs_check(int mode, const pmt_quad_stage *host_stages, const pmt_quad_stage_terms *host_terms, const pmt_quad_stage_diag *host_diags,
                    int64_t T, const pmt_quad_stage_const *host_consts, int64_t nconsts, int64_t nterms, int64_t nlin) {
    PMT_REQUIRE(T >= 0, PMT_DIMENSION_MISMATCH, "quad_stages: negative stage count");
    PMT_REQUIRE(nterms >= 0 && nlin >= 0, PMT_DIMENSION_MISMATCH, "quad_stages: negative term count");
    PMT_REQUIRE(T == 0 || host_stages, PMT_INVALID_ARGUMENT, "quad_stages: null stage table");
    std::vector<std::pair<int64_t, int64_t>> quad, lin;
    quad.reserve((size_t)T);
    lin.reserve((size_t)T);
    for (int64_t t = 0; t < T; ++t) {
        const pmt_quad_stage &d = host_stages[t];
        const std::string at = " (stage " + std::to_string(t) + ")";
        PMT_REQUIRE(d.Q || mode >= QS_DIAG, PMT_INVALID_ARGUMENT, "quad_stages: null matrix" + at);
        PMT_REQUIRE(d.xvar, PMT_INVALID_ARGUMENT, "quad_stages: null variable indices" + at);
        PMT_REQUIRE(d.sign >= -1 && d.sign <= 1, PMT_INVALID_ARGUMENT, "quad_stages: sign must be -1, 0 or +1" + at);
        PMT_REQUIRE(d.sign == 0 || d.vec, PMT_INVALID_ARGUMENT, "quad_stages: a shifted stage without its vector" + at);
        PMT_REQUIRE(d.n >= 1 && d.n <= QS_MAX_N, PMT_DIMENSION_MISMATCH, "quad_stages: n outside 1 .. 256" + at);
        PMT_REQUIRE(!d.Q || d.ldq >= d.n, PMT_DIMENSION_MISMATCH, "quad_stages: ldq < n" + at);
        PMT_REQUIRE(d.quad_at >= 0 && d.lin_at >= 0, PMT_DIMENSION_MISMATCH, "quad_stages: a slice starts below 0" + at);
        quad.emplace_back(d.quad_at, d.Q ? (int64_t)d.n * (d.n + 1) / 2 : (int64_t)d.n);
        lin.emplace_back(d.lin_at, (int64_t)d.n);
    }
    PMT_REQUIRE(qs_slices_ok(quad, nterms), PMT_DIMENSION_MISMATCH, "quad_stages: quadratic slices overlap or leave [0, nterms)");
    PMT_REQUIRE(qs_slices_ok(lin, nlin), PMT_DIMENSION_MISMATCH, "quad_stages: linear slices overlap or leave [0, nlin)");
    if (mode == QS_PLAIN) return PMT_OK;
    PMT_REQUIRE(T == 0 || host_terms, PMT_INVALID_ARGUMENT, "quad_stages_terms: null table of stage terms");
    PMT_REQUIRE(nconsts >= 0 && nconsts <= PMT_QUAD_STAGES_MAX_CONSTS, PMT_DIMENSION_MISMATCH, "quad_stages_terms: nconsts outside 0 .. 32");
    PMT_REQUIRE(nconsts == 0 || host_consts, PMT_INVALID_ARGUMENT, "quad_stages_terms: null table of constants");
    if (mode < QS_DIAG || !host_diags) return PMT_OK;
    for (int64_t t = 0; t < T; ++t) {
        const pmt_quad_stage_diag &r = host_diags[t];
        const std::string at = " (stage " + std::to_string(t) + ")";
        PMT_REQUIRE(r.present == 0 || r.present == 1, PMT_INVALID_ARGUMENT, "quad_stages_diag: present must be 0 or 1" + at);
        PMT_REQUIRE(host_stages[t].Q || !r.present, PMT_INVALID_ARGUMENT, "quad_stages_diag: a rider on an identity stage" + at);
        if (!r.present) continue;
        PMT_REQUIRE(r.sign >= -1 && r.sign <= 1, PMT_INVALID_ARGUMENT, "quad_stages_diag: sign must be -1, 0 or +1" + at);
        PMT_REQUIRE(r.sign == 0 || r.vec, PMT_INVALID_ARGUMENT, "quad_stages_diag: a shifted rider without its vector" + at);
    }
    return PMT_OK;
}

// An entry point's argument checks under its own `name`, then its launches.  `g` is filled as far as MODE reads it: {{{{stages, T, varmap,
// out_quad, out_lin, stage_consts, out_const}, terms, consts, nconsts}, diags}, out_P_values, alpha}
template <int MODE>
static int qs_run(const char *name, void *stream, const QuadStagesCscArgs &g) {
    constexpr bool TERMS = MODE != QS_PLAIN;
    const auto says = [name](const char *what) { return std::string(name) + ": " + what; };
    PMT_REQUIRE(g.T >= 0, PMT_DIMENSION_MISMATCH, says("negative stage count"));
    PMT_REQUIRE(!TERMS || (g.nconsts >= 0 && g.nconsts <= PMT_QUAD_STAGES_MAX_CONSTS), PMT_DIMENSION_MISMATCH, says("nconsts outside 0 .. 32"));
    PMT_REQUIRE(g.cst, PMT_INVALID_ARGUMENT, says("null constant"));
    PMT_REQUIRE(!TERMS || g.nconsts == 0 || g.cterms, PMT_INVALID_ARGUMENT, says("null table of constants"));
    const bool out = MODE == QS_CSC ? g.pvalues != nullptr : g.quad != nullptr;
    PMT_REQUIRE(g.T == 0 || (g.stages && (!TERMS || g.terms) && g.varmap && out && g.lin && g.consts), PMT_INVALID_ARGUMENT, says("null pointer"));
    return qs_launch<MODE>(stream, g);
}

extern "C" int pmt_quad_stages_check(const pmt_quad_stage *host_stages, int64_t T, int64_t nterms, int64_t nlin) {
    return qs_check(QS_PLAIN, host_stages, nullptr, nullptr, T, nullptr, 0, nterms, nlin);
}

extern "C" int pmt_quad_stages_f64(const pmt_quad_stage *stages, int64_t T, const int64_t *varmap, pmt_quadratic_term *out_quad,
                                   pmt_linear_term *out_lin, double *stage_consts, double *out_const, void *stream) {
    return qs_run<QS_PLAIN>("quad_stages", stream,
                            {{{{stages, T, varmap, out_quad, out_lin, stage_consts, out_const}, nullptr, nullptr, 0}, nullptr}, nullptr, 0.0});
}

extern "C" int pmt_quad_stages_terms_check(const pmt_quad_stage *host_stages, const pmt_quad_stage_terms *host_terms, int64_t T,
                                           const pmt_quad_stage_const *host_consts, int64_t nconsts, int64_t nterms, int64_t nlin) {
    return qs_check(QS_TERMS, host_stages, host_terms, nullptr, T, host_consts, nconsts, nterms, nlin);
}

extern "C" int pmt_quad_stages_terms_f64(const pmt_quad_stage *stages, const pmt_quad_stage_terms *terms, int64_t T,
                                         const pmt_quad_stage_const *consts, int64_t nconsts, const int64_t *varmap,
                                         pmt_quadratic_term *out_quad, pmt_linear_term *out_lin, double *stage_consts, double *out_const,
                                         void *stream) {
    return qs_run<QS_TERMS>("quad_stages_terms", stream,
                            {{{{stages, T, varmap, out_quad, out_lin, stage_consts, out_const}, terms, consts, nconsts}, nullptr}, nullptr, 0.0});
}

extern "C" int pmt_quad_stages_diag_check(const pmt_quad_stage *host_stages, const pmt_quad_stage_terms *host_terms,
                                          const pmt_quad_stage_diag *host_diags, int64_t T, const pmt_quad_stage_const *host_consts,
                                          int64_t nconsts, int64_t nterms, int64_t nlin) {
    return qs_check(QS_DIAG, host_stages, host_terms, host_diags, T, host_consts, nconsts, nterms, nlin);
}

extern "C" int pmt_quad_stages_diag_f64(const pmt_quad_stage *stages, const pmt_quad_stage_terms *terms, const pmt_quad_stage_diag *diags,
                                        int64_t T, const pmt_quad_stage_const *consts, int64_t nconsts, const int64_t *varmap,
                                        pmt_quadratic_term *out_quad, pmt_linear_term *out_lin, double *stage_consts, double *out_const,
                                        void *stream) {
    return qs_run<QS_DIAG>("quad_stages_diag", stream,
                           {{{{stages, T, varmap, out_quad, out_lin, stage_consts, out_const}, terms, consts, nconsts}, diags}, nullptr, 0.0});
}

extern "C" int pmt_quad_stages_csc_check(const pmt_quad_stage *host_stages, const pmt_quad_stage_terms *host_terms,
                                         const pmt_quad_stage_diag *host_diags, int64_t T, const pmt_quad_stage_const *host_consts,
                                         int64_t nconsts, int64_t nvalues, int64_t nlin) {
    return qs_check(QS_CSC, host_stages, host_terms, host_diags, T, host_consts, nconsts, nvalues, nlin);
}

extern "C" int pmt_quad_stages_csc_f64(const pmt_quad_stage *stages, const pmt_quad_stage_terms *terms, const pmt_quad_stage_diag *diags,
                                       int64_t T, const pmt_quad_stage_const *consts, int64_t nconsts, const int64_t *varmap, double alpha,
                                       double *out_P_values, pmt_linear_term *out_lin, double *stage_consts, double *out_const,
                                       void *stream) {
    return qs_run<QS_CSC>("quad_stages_csc", stream,
                          {{{{stages, T, varmap, nullptr, out_lin, stage_consts, out_const}, terms, consts, nconsts}, diags}, out_P_values, alpha});
}
