// Per-calling-stream state (streams.h): created on first use, released with the last plan on the stream.
#include <cstring>
#include <mutex>
#include <unordered_map>

#include "streams.h"

namespace pmt {

static std::mutex g_side_mu;
static std::unordered_map<hipStream_t, SideStream> g_side;
static const long long ARMED[MAXGROUPS] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};     // the courier's flags, armed

// everything a calling stream's state holds goes (what is still queued on its streams and engines first)
static void destroy_side(SideStream &ss) {
    for (hipStream_t st : {ss.stream, ss.fetch}) if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    for (hipEvent_t e : {ss.fork, ss.join, ss.join2, ss.fetch_done}) if (e) (void)hipEventDestroy(e);
    (void)wait_dma_pending(&ss);
    if (ss.counters) (void)hipFree(ss.counters);
    if (ss.err_host) (void)hipHostFree(ss.err_host);
}

SideStream *side_stream(hipStream_t s) {
#ifdef PMT_TUNING
    static const bool enabled = [] { const char *e = getenv("PMT_GRAM_SIDE_STREAM"); return !(e && e[0] == '0'); }();
    if (!enabled) return nullptr;
#endif
    int dev = 0;
    if (hipStreamGetDevice(s, &dev) != hipSuccess) {
        (void)hipGetLastError();
        if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    }
    std::lock_guard<std::mutex> lock(g_side_mu);
    SideStream &ss = g_side[s];
    if (ss.stream && ss.device == dev) return &ss;
    int prev = 0;
    (void)hipGetDevice(&prev);
    if (prev != dev && hipSetDevice(dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    // LOWEST priority: (1) HIP multiplexes streams onto a few hardware queues per priority class, so a side stream of its own class
    // never shares a queue with the (normal-priority) stream it serves — sharing one makes the contraction queue up behind its own side
    // kernels (config 2 under torch.distributed, whose RCCL streams take queues too: 1.35 instead of 1.24 ms per step); (2) when both
    // have packets ready, the contraction's workgroups are placed first.
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    bool ok = hipStreamCreateWithPriority(&ss.stream, hipStreamNonBlocking, prio_least) == hipSuccess &&
              hipEventCreateWithFlags(&ss.fork, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&ss.join, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&ss.join2, hipEventDisableTiming) == hipSuccess &&
              hipMalloc(&ss.counters, COUNTER_BYTES) == hipSuccess &&
              hipHostMalloc(reinterpret_cast<void **>(&ss.err_host), 64, hipHostMallocDefault) == hipSuccess &&
              hipMemsetAsync(ss.counters, 0, COUNTER_BYTES, s) == hipSuccess;      // on the calling stream: ordered before its first kernel
    if (ok) {
        memset(ss.err_host, 0, 64);
        ss.err_dev = static_cast<int *>(host_device_pointer(ss.err_host));
        ok = ss.err_dev != nullptr &&
             hipMemcpyAsync(static_cast<char *>(ss.counters) + FLAGS_OFFSET, ARMED, sizeof ARMED, hipMemcpyHostToDevice, s) == hipSuccess;
    }
    if (prev != dev) (void)hipSetDevice(prev);
    if (!ok) {
        (void)hipGetLastError();
        destroy_side(ss);
        g_side.erase(s);
        return nullptr;
    }
    ss.device = dev;
    return &ss;
}

// the side stream of calling stream `s` for other users (the plan's side lane, plan.hip): work queued here lines up BEHIND the Gram
// node's two small reductions, i.e. it is dispatched once the contraction's workgroups are placed and runs as they drain
// a plan that goes away takes the side stream of its stream with it (pmt_plan_destroy): HIP multiplexes streams onto a handful of hardware
// queues, and a leaked side stream can end up sharing the queue of a later plan's stream — its contraction then queues BEHIND its own side
// kernels instead of running beside them (measured: config 3 1.27 -> 1.45 ms when run after another plan in the same process)
// Plans that share one external stream share its side stream: it is reference-counted by plan (pmt_plan_create retains, pmt_plan_destroy
// releases) and goes away with the LAST of them, not with the first.
static std::unordered_map<hipStream_t, int> g_side_refs;
void retain_side_stream(hipStream_t s) {
    std::lock_guard<std::mutex> lock(g_side_mu);
    ++g_side_refs[s];
}
void release_side_stream(hipStream_t s) {
    std::lock_guard<std::mutex> lock(g_side_mu);
    auto rc = g_side_refs.find(s);
    if (rc != g_side_refs.end()) {
        if (--rc->second > 0) return;
        g_side_refs.erase(rc);
    }
    auto it = g_side.find(s);
    if (it == g_side.end()) return;
    destroy_side(it->second);
    g_side.erase(it);
}

// the state of calling stream `s`, if it has any (it lives until the last plan on `s` releases it)
static SideStream *find_side(hipStream_t s) {
    std::lock_guard<std::mutex> lock(g_side_mu);
    auto it = g_side.find(s);
    return it == g_side.end() ? nullptr : &it->second;
}

// ---- the calling stream's device-to-host stream -----------------------------------------------------------------------------------
int ensure_fetch_stream(SideStream *ss) {
    if (ss->fetch) return PMT_OK;
    int prev = 0;
    (void)hipGetDevice(&prev);
    if (prev != ss->device) PMT_HIP_CHECK(hipSetDevice(ss->device));
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    hipError_t e = hipStreamCreateWithPriority(&ss->fetch, hipStreamNonBlocking, prio_greatest);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ss->fetch_done, hipEventDisableTiming);
    if (prev != ss->device) (void)hipSetDevice(prev);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(PMT_HIP_ERROR, std::string("fetch stream: ") + hipGetErrorString(e)); }
    return PMT_OK;
}

// D2H copy ordered behind everything enqueued on `after` (the plan's stream or its side stream) so far.  Preferred: the copy engine, started
// by a signal that a one-thread kernel on `after` sets (hsadma.hip) — nothing of it runs on a CU.  Otherwise a kernel copy / the runtime's
// copy on the fetch stream of `s`.  r.height > 0: a PITCHED copy of r.height rows of `bytes` bytes each (a matrix block whose device copy
// is padded, or that lands in a column range of a wider host matrix); the engine does those natively (hsa_amd_memory_async_copy_rect).
int fetch_async(hipStream_t s, hipStream_t after, hipEvent_t order_event, void *host_dst, const void *device_src, size_t bytes, FetchState *st, FetchRect r) {
    SideStream *ss = side_stream(s);
    if (!ss) return fail(PMT_STATE_ERROR, "fetch_async: no auxiliary streams for this stream");
    // A fetch behind the plan's OWN stream inside a replay (its producer finishes with the objective's kernels, e.g. the constant, whose
    // serial chain is itself queued at the end of the replay) is issued at the end of the replay, behind that chain's join and behind the
    // band groups of a delivery (the copy engine's queue is first in, first out).
    if (ss->in_replay && after == s) {
        ss->deferred.push_back([=]() -> int { return fetch_async(s, after, order_event, host_dst, device_src, bytes, st, r); });
        return PMT_OK;
    }
    const int mode = dma::delivery_mode();
    // whichever way this entry's previous copy went, it has read the device buffer (and left the host one) before the next one is queued
    if (st && st->pending) { if (int rc = dma::wait(st->eng, st->done, 10.0)) return rc; st->pending = false; }
    // the engine is handed physical pages: only page-locked, device-mapped destinations qualify (a pageable numpy / Julia array takes the
    // runtime's copy below, which stages it)
    if (st && st->pinned < 0) st->pinned = host_device_pointer(host_dst) ? 1 : 0;
    if (mode != 2 && st && st->pinned == 1 && !st->created && !st->tried) {
        st->tried = true;
        st->eng = dma::get(ss->device);
        if (st->eng) {
            if (dma::signal_create(st->eng, 1, &st->dep) == PMT_OK && dma::signal_create(st->eng, 0, &st->done) == PMT_OK) st->created = true;
            else st->eng = nullptr;
        }
    }
    const bool engine = mode != 2 && st && st->created;
    if (mode == 1 && !engine)
        return fail(PMT_STATE_ERROR, "host delivery: the copy engine was demanded (pmt_set_host_delivery(1)) but is not available for this transfer "
                                     "(no HSA agent match, or a pageable destination)");
    if (engine) {
        dma::signal_set(st->eng, st->dep, 1);
        dma::signal_set(st->eng, st->done, 1);
        if (int rc = dma::launch_signal_store(st->dep, after)) return rc;
        st->pending = true;
        ss->dma_pending.emplace_back(st->eng, st->done);
        if (r.height) return dma::copy_rect_to_host(st->eng, host_dst, r.dst_pitch, device_src, r.src_pitch, bytes, r.height, &st->dep, st->done);
        return dma::copy_to_host(st->eng, host_dst, device_src, bytes, &st->dep, st->done);
    }
    if (int rc = ensure_fetch_stream(ss)) return rc;
    PMT_HIP_CHECK(hipEventRecord(order_event, after));
    PMT_HIP_CHECK(hipStreamWaitEvent(ss->fetch, order_event, 0));
    // a <= 16-VGPR copy kernel that is co-resident with the contraction (deliver.hip) when the destination is page-locked, 8-byte words
    // and below 16 GiB; the runtime's copy otherwise
    const size_t total = r.height ? r.height * r.dst_pitch : bytes;
    const bool words = bytes % 8 == 0 && (!r.height || (r.dst_pitch % 8 == 0 && r.src_pitch % 8 == 0));
    void *dst_dev = (words && total / 8 < (size_t)1 << 31) ? host_device_pointer(host_dst) : nullptr;
    if (dst_dev && r.height) { if (int rc = launch_to_host_2d(device_src, r.src_pitch, dst_dev, r.dst_pitch, bytes, r.height, ss->fetch)) return rc; }
    else if (dst_dev) { if (int rc = launch_to_host(device_src, dst_dev, bytes, ss->fetch)) return rc; }
    else if (r.height) PMT_HIP_CHECK(hipMemcpy2DAsync(host_dst, r.dst_pitch, device_src, r.src_pitch, bytes, r.height, hipMemcpyDeviceToHost, ss->fetch));
    else PMT_HIP_CHECK(hipMemcpyAsync(host_dst, device_src, bytes, hipMemcpyDeviceToHost, ss->fetch));
    PMT_HIP_CHECK(hipEventRecord(ss->fetch_done, ss->fetch));
    ss->fetch_pending = true;
    return PMT_OK;
}

#ifdef PMT_TUNING
static double g_replay_t0 = 0;
static double host_us() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3; }
// debugging aid (PMT_DMA_DEBUG=2): poll every pending completion signal and the calling stream, print when each changes
static void trace_dma_pending(SideStream *ss, hipStream_t s) {
    std::vector<long> last(ss->dma_pending.size(), -100);
    bool stream_done = false;
    const double t0 = host_us();
    for (;;) {
        bool all = true;
        for (size_t i = 0; i < ss->dma_pending.size(); ++i) {
            const long v = (long)*ss->dma_pending[i].second.value;
            if (v != last[i]) { fprintf(stderr, "[trace +%.0f us] transfer set %zu: %ld left\n", host_us() - g_replay_t0, i, v); last[i] = v; }
            if (v > 0) all = false;
        }
        if (!stream_done && hipStreamQuery(s) == hipSuccess) { stream_done = true; fprintf(stderr, "[trace +%.0f us] the plan's stream is idle\n", host_us() - g_replay_t0); }
        if ((all && stream_done) || host_us() - t0 > 1e6) break;
    }
}
#endif

int wait_dma_pending(SideStream *ss) {
    int rc = PMT_OK;
    for (auto &p : ss->dma_pending) { const int r = dma::wait(p.first, p.second, 10.0); if (r && !rc) rc = r; }
    ss->dma_pending.clear();
    ss->keepalive.clear();
    return rc;
}

// `s` waits until the copies enqueued on its fetch stream so far have read their device buffers (start of the next re-evaluation)
int fetch_fence(hipStream_t s) {
    SideStream *ss = find_side(s);
    if (!ss) return PMT_OK;
    // copy-engine transfers are not stream work: the HOST waits for them (a no-op when the caller has synchronised, as solve! does)
    if (int rc = wait_dma_pending(ss)) return rc;
    if (ss->fetch_pending) { PMT_HIP_CHECK(hipStreamWaitEvent(s, ss->fetch_done, 0)); ss->fetch_pending = false; }
    return PMT_OK;
}

// a plan's replay brackets its tape with these: transfers that should queue up behind the tape's own are submitted by replay_end
void replay_begin(hipStream_t s, bool side_work) {
#ifdef PMT_TUNING
    g_replay_t0 = host_us();
#endif
    if (SideStream *ss = find_side(s)) { ss->in_replay = true; ss->side_work = side_work; }
}
int replay_end(hipStream_t s) {
    SideStream *ss = find_side(s);
    if (!ss) return PMT_OK;
    ss->in_replay = false;
    ss->side_work = false;
    int rc = PMT_OK;
    for (auto &f : ss->deferred) { const int r = f(); if (r && !rc) rc = r; }
    ss->deferred.clear();
    return rc;
}

// `f` (launches on `s`) behind what a plan's replay has queued at its end for `s` so far — the stream-K node's c'c (gram.hip: const_part):
// appended to that queue inside a replay that has one, run now otherwise.  A consumer of a Gram node's constant (gram_sum.hip) goes
// through this, so that it reads the constant after it has been written.
int gram_after_deferred(hipStream_t s, std::function<int()> f) {
    SideStream *ss = find_side(s);
    if (!ss || !ss->in_replay || ss->deferred.empty()) return f();
    ss->deferred.push_back(std::move(f));
    return PMT_OK;
}

// host: block until every copy enqueued on the fetch stream of `s` has landed
int fetch_synchronize(hipStream_t s) {
    SideStream *ss = find_side(s);
    if (!ss) return PMT_OK;
#ifdef PMT_TUNING
    { const char *e = getenv("PMT_DMA_DEBUG"); if (e && e[0] == '2') trace_dma_pending(ss, s); }
#endif
    int rc = wait_dma_pending(ss);
    if (!rc && ss->fetch) PMT_HIP_CHECK(hipStreamSynchronize(ss->fetch));
    // the kernels' error word (page-locked, written with system-scope stores before the data the transfers above carried)
    const int err = ss->err_host ? __atomic_exchange_n(ss->err_host, 0, __ATOMIC_ACQ_REL) : 0;
    if (err == ERR_COURIER) {
        // the courier left without re-arming: flags back to "in the making", completion count to zero
        PMT_HIP_CHECK(hipMemset(ss->counters, 0, COUNTER_BYTES));
        PMT_HIP_CHECK(hipMemcpy(static_cast<char *>(ss->counters) + FLAGS_OFFSET, ARMED, sizeof ARMED, hipMemcpyHostToDevice));
        return fail(PMT_HIP_ERROR, "host delivery: the courier saw no progress of the contraction for 2 s and gave up; the host arrays are incomplete");
    }
    if (err == ERR_PAIR_FOLD)
        return fail(PMT_HIP_ERROR, "host delivery: a split tile of the contraction never received its first half (pair fold); the tile was "
                                   "written as NaN and the delivered quadratic coefficients are invalid");
    if (err) return fail(PMT_HIP_ERROR, "host delivery: unknown device error " + std::to_string(err));
    return rc;
}

}  // namespace pmt

extern "C" int pmt_fetch_synchronize(void *stream) {
    PMT_REQUIRE(!pmt::is_recording_handle(stream), PMT_INVALID_ARGUMENT, "fetch_synchronize: `stream` is a plan's recording handle; use pmt_plan_fetch_synchronize");
    return pmt::fetch_synchronize(reinterpret_cast<hipStream_t>(stream));
}
