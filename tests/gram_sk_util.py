"""Host restatement of the stream-K Gram form's launch arithmetic (csrc/gram_sk.hip: launch_gram_sk; csrc/gram.hip: deliver_plan, gram_form), the
case tables of test_gpu_gram_sk.py, and exact ("dyadic") data for them.  No GPU, no library: test_gram_sk_plan_host.py pushes the tables
through these functions to prove which regime every case reaches, and compares the expected form with pmt_quad_gram_constant_order.

The restatement lives here and not behind an export of the device file on purpose: gram_sk.hip's schedule moves with unrelated source
edits (the file is FROZEN), so nothing is added to it for the tests' sake.

Exact data.  dyadic(shape, bits, rng) returns integers in (-2^bits, 2^bits) scaled by 2^-bits.  With 2 bits + ceil(log2(rows)) + 1 <= 52
every product a_ij a_ik is an integer multiple of 2^(-2 bits) below 1, and every partial sum of up to `rows` of them (A'A, A'c, c'c), in any
order, with or without FMA, is such a multiple below 2^(ceil(log2 rows)): it has at most 2 bits + ceil(log2 rows) + 1 <= 52 significant
bits and is exact.  The float64 results are therefore unique — whatever the split of the contraction, the order of the fix-up, the fold —
and their mantissas are filled down to the last bits (small-integer data would leave the low word of every double zero).  The factor 2 and
alpha in {-0.5, 2.0} are powers of two: exact too.  The reference is plain numpy (A.T @ A, A.T @ c, c @ c), exact for the same reason."""
import math
from collections import namedtuple

import numpy as np

ST = 128                 # output tile edge                                   (gram_common.h)
SKC = 256                # contraction depth per work unit at most
MAXG = 512               # upper bound on persistent workgroups
MAXGROUPS = 16           # stages of a host delivery
GWANT = 256              # one 8-wave workgroup per CU                        (launch_gram_sk)
NACC = 32                # fp64 accumulators per lane (Cfg<2>::NACC)
SK_APB1_BELOW = 64       # fix-up: one accumulator per workgroup below this   (gram_sk.hip)
SK_BK = 16               # rows per stage
TCOLS = 128              # columns of the one-tile kernel                     (gram_tall.hip)
MID_MAXCOLS, MID_BIGCOLS, MID_BIGEL = 2048, 4096, 1 << 29                   # (gram.hip)
SMALL_NODE_WORK_MAX = 32768                                                 # (common.h)
DELIVER_ORDER_W = 1      # super-columns of one tile column, walked from the end (gram.hip)


def cdiv(a, b):
    return -(-a // b)


def ntiles(cols):
    return cdiv(cols, ST)


def tri(nt):
    return nt * (nt + 1) // 2


# ---- launch_gram_sk -------------------------------------------------------------------------------------------------------------------------
LaunchPlan = namedtuple("LaunchPlan", "skc nchunk G tfull R U fold fixup units_min units_max max_partials")


def sk_launch_plan(rows, T, ranged, strict, pair_flags):
    """launch_gram_sk's host arithmetic for a launch over T tiles (ranged: seq_count >= 0; strict implies ranged).  fixup is one of
    "none", "apb4", "apb1", "sliced".  units_min / units_max: phase-B units of the emptiest / fullest workgroup (sk_unit_begin);
    max_partials: the most workgroups that share one split tile (what the fix-up kernels' loops run over)."""
    strict = bool(strict and ranged)
    skc = SKC
    if not ranged or strict:
        while skc > 64 and T * cdiv(rows, skc) < 256:
            skc >>= 1
    nchunk = max(1, cdiv(rows, skc))
    G = min(T * nchunk, min(GWANT, MAXG))
    if strict and 2 <= T <= 32 and T * nchunk >= 4 * GWANT:
        G = T * (GWANT // T)
    tfull = T // G
    R = T - tfull * G
    U = R * nchunk
    fold = bool(ranged and pair_flags and tfull == 0 and nchunk % 2 == 0 and 2 * R == G and U == G * (nchunk // 2) and G <= MAXG // 2)
    fixup = "none"
    if nchunk > 1 and R > 0 and not fold:
        if G >= 32 * R:
            fixup = "sliced"
        elif R * (NACC // 4) < SK_APB1_BELOW:
            fixup = "apb1"
        else:
            fixup = "apb4"
    begin = [b * U // G for b in range(G + 1)]
    units = [begin[b + 1] - begin[b] for b in range(G)]
    max_partials = 0
    if R > 0:
        owner = np.searchsorted(np.asarray(begin[1:]), np.arange(U), side="right")          # workgroup b holds units [begin[b], begin[b+1])
        for rt in range(R):
            max_partials = max(max_partials, int(owner[(rt + 1) * nchunk - 1] - owner[rt * nchunk]) + 1)
    return LaunchPlan(skc, nchunk, G, tfull, R, U, fold, fixup, min(units), max(units), max_partials)


def slots_per_workgroup(plan):
    """the most partial-tile slots one workgroup of the launch writes (a workgroup whose unit range ends one split tile and begins the next
    writes two: U > G)"""
    if plan.R == 0 or plan.fixup == "none":
        return 0
    most = 0
    for b in range(plan.G):
        u0, u1 = b * plan.U // plan.G, (b + 1) * plan.U // plan.G
        n, u = 0, u0
        while u < u1:
            rt = u // plan.nchunk
            c0 = u - rt * plan.nchunk
            c1 = min(plan.nchunk, c0 + (u1 - u))
            if not (c0 == 0 and c1 == plan.nchunk):
                n += 1
            u += c1 - c0
        most = max(most, n)
    return most


# ---- gram_form ------------------------------------------------------------------------------------------------------------------------------
def gram_tiny(rows, cols):
    t = rows * cols * (cols + 1) // 2
    return cols > 0 and rows <= 64 and t <= 16384 and t + 64 * rows <= SMALL_NODE_WORK_MAX


def gram_tall_applies(rows, cols):
    return 1 <= cols <= TCOLS and rows >= 1 and not gram_tiny(rows, cols)


def gram_tall_diag_applies(rows, cols):
    return TCOLS < cols <= 16 * TCOLS and rows >= 1


def gram_mid_big(rows, cols):
    return 16 * 128 < cols <= MID_BIGCOLS and rows >= 1 and rows * cols < MID_BIGEL


def gram_mid_applies(rows, cols):
    if gram_mid_big(rows, cols):
        return True
    if not gram_tall_diag_applies(rows, cols) or cols > MID_MAXCOLS:
        return False
    el = rows * cols
    if cols <= 192:
        return el <= 1 << 25
    if cols < 320:
        return el < 1 << 26
    if cols < 384:
        return el <= 1 << 27
    return el < 1 << 29


def gram_form(rows, cols, csc, deliver):
    """gram.hip: gram_form -> "tiny", "mid", "fused", "streamk_staged", "streamk" """
    if not deliver and not csc and gram_tiny(rows, cols):
        return "tiny"
    big = gram_mid_big(rows, cols)
    if (big and not deliver) or (not big and gram_mid_applies(rows, cols)):
        return "mid"
    if gram_tall_applies(rows, cols) or gram_tall_diag_applies(rows, cols):
        return "fused"
    return "streamk_staged" if deliver and cols > 0 else "streamk"


def constant_chained(rows, cols):
    if rows > 8192:
        return True
    if rows < 2048:
        return False
    nt = float(cdiv(max(cols, 1), ST))
    contraction_ms = (0.096 + 0.276 * rows / 1024.0) * (nt * (nt + 1) / 2) / 528.0
    return 0.07e-3 * rows > 0.5 * contraction_ms


def expected_constant_order(use, rows, cols):
    """what pmt_quad_gram_constant_order must report for a shape whose case expects stream-K use `use`: 0 / 1 for the stream-K node; 5 for a
    staged delivery of a shape whose plain call is the one-launch form; 2 (or 3, 4: the fused tall forms) for the strict launch"""
    if use == "strict":
        return (2, 3, 4)
    if use == "staged" and gram_form(rows, cols, True, False) == "mid":
        return (5,)
    return (1,) if constant_chained(rows, cols) else (0,)


def sk_use(rows, cols, csc, deliver):
    """which of the stream-K kernel's three jobs a call does: "plain" (GramForm::StreamK), "staged" (StreamKStaged), "strict" (the fused
    form's strictly upper tiles), or None (the kernel does not run)"""
    form = gram_form(rows, cols, csc, deliver)
    if form == "streamk":
        return "plain" if cols > 0 else None
    if form == "streamk_staged":
        return "staged"
    if form == "fused" and ntiles(cols) > 1:
        return "strict"
    return None


# ---- deliver_plan ---------------------------------------------------------------------------------------------------------------------------
Stage = namedtuple("Stage", "seq_begin seq_count")


def deliver_stages(rows, cols, ngroups, quad):
    """deliver_plan's stages of a STAGED delivery (the form is StreamKStaged): (order_w, [Stage]).  order_w is what launch_gram_sk gets:
    0 for the terms (row bands, forward walk), -DELIVER_ORDER_W for the CSC values (column bands, walked from the end)."""
    nt = ntiles(cols)
    T = tri(nt)
    nchunk = max(1, cdiv(rows, 256))
    G = min(T * nchunk, 256)
    per = max(1, G // 2) if nchunk >= 2 else G
    if ngroups > 0:
        per = max(1, cdiv(T, min(ngroups, MAXGROUPS)))
    if cdiv(T, per) > MAXGROUPS:
        per = cdiv(T, MAXGROUPS)
    stages = [Stage(t0, min(per, T - t0)) for t0 in range(0, T, per)]
    return (0 if quad else -DELIVER_ORDER_W), stages


def linear_splits(rows, cols):
    if cols <= 0:
        return 1
    return max(1, min(cdiv(8192, cols), rows // 4096))


def seq_unrank(idx, nt):
    """sk_seq_unrank: super-rows of four tile rows, column by column"""
    base = 0
    for j0 in range(0, nt, 4):
        h, W = min(4, nt - j0), nt - j0
        t3 = h * (h + 1) // 2
        count = t3 + (W - h) * h
        if idx < base + count:
            p = idx - base
            if p < t3:
                c = 0
                while p >= c + 1:
                    p -= c + 1
                    c += 1
                return j0 + p, j0 + c
            p -= t3
            return j0 + p % h, j0 + h + p // h
        base += count
    return nt - 1, nt - 1


def colseq_unrank(idx, nt, w):
    """sk_colseq_unrank: super-columns of w tile columns, row by row"""
    base = 0
    for c0 in range(0, nt, w):
        h = min(w, nt - c0)
        rect = c0 * h
        count = rect + h * (h + 1) // 2
        if idx < base + count:
            p = idx - base
            if p < rect:
                return p // h, c0 + p % h
            p -= rect
            r = 0
            while p >= h - r:
                p -= h - r
                r += 1
            return c0 + r, c0 + r + p
        base += count
    return nt - 1, nt - 1


def stage_tiles(cols, order_w, stage):
    """the (jb, kb) tiles a ranged launch covers, in launch order (launch_gram_sk: seq_begin / seq_step; a walk from the end for order_w < 0)"""
    nt = ntiles(cols)
    if order_w < 0:
        first, step, w = tri(nt) - 1 - stage.seq_begin, -1, -order_w
    else:
        first, step, w = stage.seq_begin, 1, order_w
    out = []
    for t in range(stage.seq_count):
        idx = first + step * t
        out.append(colseq_unrank(idx, nt, w) if w > 0 else seq_unrank(idx, nt))
    return out


def case_launches(case):
    """every stream-K launch a case makes, as (LaunchPlan, order_w, Stage or None)"""
    rows, cols = case.rows, case.cols
    use = case.use
    if use == "plain":
        return [(sk_launch_plan(rows, tri(ntiles(cols)), False, False, False), 0, None)]
    if use == "strict":
        nt = ntiles(cols)
        return [(sk_launch_plan(rows, nt * (nt - 1) // 2, True, True, False), 0, None)]
    order_w, stages = deliver_stages(rows, cols, case.ngroups, case.entry == "terms_deliver")
    return [(sk_launch_plan(rows, st.seq_count, True, False, True), order_w, st) for st in stages]


def load_path(case):
    """"vec" (16-byte loads: even pitch, 16-byte-aligned base) or "masked" (vec_in == 0: 8-byte loads, bounds-checked)"""
    return "vec" if (case.rows + case.pad) % 2 == 0 and case.shift == 0 else "masked"


# ---- exact data -----------------------------------------------------------------------------------------------------------------------------
def dyadic_bits(rows, most=20):
    """the largest bits <= most with 2 bits + ceil(log2(rows)) + 1 <= 52"""
    lg = max(1, math.ceil(math.log2(max(rows, 2))))
    return min(most, (52 - 1 - lg) // 2)


def dyadic_bound_holds(rows, bits):
    return 2 * bits + (math.ceil(math.log2(rows)) if rows > 1 else 0) + 1 <= 52


def dyadic(shape, bits, rng):
    """integers in (-2^bits, 2^bits) scaled by 2^-bits (see the module docstring)"""
    return rng.integers(-(1 << bits) + 1, 1 << bits, size=shape).astype(np.float64) / float(1 << bits)


def exact_dot(x, y, bits):
    """sum x_i y_i of dyadic vectors with Python integers, as the float64 it must round to WITHOUT rounding (asserted)"""
    xi = [int(v) for v in np.rint(np.asarray(x) * float(1 << bits)).astype(np.int64)]
    yi = [int(v) for v in np.rint(np.asarray(y) * float(1 << bits)).astype(np.int64)]
    s = sum(a * b for a, b in zip(xi, yi))
    assert abs(s) < 1 << 53, "the sum does not fit a double's mantissa"
    return float(s) / float(1 << (2 * bits))


def variables(cols, seed, gaps=True):
    """strictly increasing model variable indices with gaps, and a permuting varmap over 1 .. xvar[-1]"""
    rng = np.random.default_rng(seed)
    xv = np.cumsum(rng.integers(1, 4, size=cols)).astype(np.int64) if gaps else np.arange(1, cols + 1, dtype=np.int64)
    vm = rng.permutation(int(xv[-1])).astype(np.int64) + 1 + 5
    return xv, vm


# ---- the case tables ------------------------------------------------------------------------------------------------------------------------
# entry:  "plain"          pmt_quad_gram_f64              out_quad; moi 0 / 1
#         "csc"            pmt_quad_gram_csc_f64          alpha * values (+ out_quad where quad = True); moi = 1
#         "csc_deliver"    pmt_quad_gram_csc_deliver_f64  alpha * values, delivered to the host; ngroups
#         "terms_deliver"  pmt_quad_gram_deliver_f64      the terms, delivered to the host; ngroups = nstages; moi 0 / 1
# use:    which job of the stream-K kernel the case expects ("plain" and its non-RANGED instantiation, "staged" / "strict": RANGED)
# sign:   -1 / +1, or 0: b = NULL.   vm: moi = 1 goes through a permuting varmap and xvar has gaps (else varmap = NULL, xvar = 1 .. n)
# quad:   out_quad is given (always for "plain" / "terms_deliver", never for "csc_deliver")
Case = namedtuple("Case", "entry use rows cols pad shift ngroups sign moi vm alpha quad bits")


def _case(entry, use, rows, cols, pad, shift, ngroups=0, sign=-1, moi=1, vm=False, alpha=1.0, quad=None, bits=None):
    if quad is None:
        quad = entry in ("plain", "terms_deliver")
    return Case(entry, use, rows, cols, pad, shift, ngroups, sign, moi, vm, alpha, quad, dyadic_bits(rows) if bits is None else bits)


# more than 4096 columns: 33 tile columns, T = 561, G = 256, tfull = 2, R = 49 — the plain (not RANGED) instantiation
PLAIN = [
    _case("plain", "plain", 1, 4097, 0, 0, sign=-1, moi=1, vm=True),                    # one row, one column in the last tile, odd pitch
    _case("csc", "plain", 16, 4224, 0, 0, sign=+1, vm=True, alpha=2.0, quad=True),      # all-fast path, nchunk = 1
    _case("plain", "plain", 257, 4100, 0, 0, sign=0, moi=0),                            # second chunk of one row, U < G, masked
    _case("csc", "plain", 600, 4200, 2, 1, sign=-1, alpha=-0.5, quad=False),            # shifted base, three chunks
    _case("plain", "plain", 1030, 4224, 2, 0, sign=+1, moi=1, vm=True),                 # fast chunks plus a 6-row tail
    _case("csc", "plain", 1552, 4160, 0, 0, sign=0, alpha=2.0, quad=False),             # U > G: two slots per workgroup, half-filled last tile
]
# staged CSC deliveries: 17 tile columns, T = 153 (the last: 33, T = 561) — RANGED, walked from the end
CSC_DELIVER = [
    _case("csc_deliver", "staged", 5, 2049, 0, 0, 0, sign=-1, vm=True, alpha=2.0),      # one stage of whole tiles, reversed walk, masked
    _case("csc_deliver", "staged", 512, 2176, 0, 0, 0, sign=+1, alpha=-0.5),            # fold, stages of 128 and 25 tiles
    _case("csc_deliver", "staged", 500, 2100, 1, 0, 0, sign=0, alpha=2.0),              # fold on the masked path
    _case("csc_deliver", "staged", 600, 2100, 0, 0, 0, sign=-1, vm=True, alpha=-0.5),   # no fold, apb4
    _case("csc_deliver", "staged", 600, 2100, 0, 0, 16, sign=+1, alpha=2.0),            # stages of 10 tiles, last stage of 3: apb1
    _case("csc_deliver", "staged", 512, 2176, 0, 0, 16, sign=0, alpha=-0.5),            # fold on grids of 20 and 6
    _case("csc_deliver", "staged", 8200, 2100, 0, 0, 16, sign=-1, vm=True, alpha=2.0),  # last stage sliced, gram_linear_split_kernel
    _case("csc_deliver", "staged", 300, 4100, 0, 0, 0, sign=+1, alpha=-0.5),            # delivered beyond 4096 columns
]
# term deliveries: row bands, forward walk — RANGED
TERMS_DELIVER = [
    _case("terms_deliver", "staged", 600, 2100, 0, 0, 0, sign=-1, moi=0),
    _case("terms_deliver", "staged", 600, 2100, 0, 0, 16, sign=+1, moi=1, vm=True),
]
# the strict launch inside the fused form — RANGED, SKArgs::strict
STRICT = [
    _case("csc", "strict", 260113, 129, 0, 0, sign=-1, vm=True, alpha=2.0, quad=True, bits=16),      # one strict tile split 256 ways, masked, sliced
    _case("plain", "strict", 261128, 257, 0, 0, sign=+1, moi=0, bits=16),                              # three strict tiles on 255 workgroups
]
# beyond the issue's tables: every 16-byte-load case above has an even row count, so the scalar tail that sk_load_panel takes for the
# last row of an odd row count on the vec_in == 1 path (even pitch from an odd padding) would go unseen — one case per instantiation
EXTRA = [
    _case("csc", "plain", 257, 4100, 1, 0, sign=+1, alpha=-0.5, quad=False),
    _case("csc_deliver", "staged", 601, 2100, 1, 0, 0, sign=-1, alpha=2.0),
    # ... and the RANGED instantiation's phase A: one stage of all 561 tiles (tfull = 2), whose remainder leaves workgroups without a unit
    # between the owners of a split tile (U = 98 < G = 256), as plain (257, 4100) does on the other instantiation
    _case("csc_deliver", "staged", 300, 4100, 0, 0, 1, sign=0, alpha=2.0),
]
CASES = PLAIN + CSC_DELIVER + TERMS_DELIVER + STRICT + EXTRA
# the two cases that also run with rng.random() - 0.4 data against the project's own bar, 1e-12 * (2 |A|'|A|)
RANDOM = [PLAIN[3], CSC_DELIVER[4]]


def case_id(c):
    s = "%s-%dx%d" % (c.entry, c.rows, c.cols)
    if c.pad or c.shift:
        s += "-pad%d-shift%d" % (c.pad, c.shift)
    if c.entry.endswith("deliver"):
        s += "-g%d" % c.ngroups
    return s


# ---- the numpy reference --------------------------------------------------------------------------------------------------------------------
def reference(case, A, b, xv, vm):
    """what the node must write for A (rows x cols), b (or None), model variables xv and varmap vm (or None), bit for bit:
    {"quad": (nq, 3) int64 words or None, "csc": (nq,) float64 or None, "lin": (cols, 2) int64 words, "const": float}"""
    n = case.cols
    G = A.T @ A + 0.0                    # (+ 0.0: a sum of -0.0 products is +0.0 on the device, whose accumulators start at +0.0)
    c = None if (b is None or case.sign == 0) else (0.0 - b if case.sign < 0 else 0.0 + b)
    idx = (lambda v: v if vm is None else vm[v - 1]) if case.moi else (lambda v: v)
    iu = np.triu_indices(n)
    coeff = 2.0 * G[iu]
    if not case.moi:
        coeff = np.where(iu[0] == iu[1], G[iu], coeff)
    out = {"quad": None, "csc": None}
    if case.quad:
        q = np.empty((len(coeff), 3), dtype=np.int64)
        q[:, 0] = coeff.view(np.int64)
        q[:, 1] = idx(xv[iu[0]])
        q[:, 2] = idx(xv[iu[1]])
        out["quad"] = q
    if case.entry in ("csc", "csc_deliver"):
        csc = np.empty(len(coeff))
        csc[iu[1] * (iu[1] + 1) // 2 + iu[0]] = case.alpha * coeff
        out["csc"] = csc
    lin = np.empty((n, 2), dtype=np.int64)
    lin[:, 0] = (2.0 * (A.T @ c + 0.0) if c is not None else np.zeros(n)).view(np.int64)
    lin[:, 1] = idx(xv)
    out["lin"] = lin
    out["const"] = float(c @ c) if c is not None else 0.0
    return out
