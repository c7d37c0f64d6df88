// Per-calling-stream state (streams.hip), internal: what the Gram node (gram.hip), gram_sum.hip and the plans (plan.hip) share about a stream.
#pragma once
#include <memory>
#include <vector>

#include "dma.h"
#include "gram_common.h"

namespace pmt {

// One non-blocking side stream + fork/join events PER CALLING STREAM (= per plan: a plan is one stream), created on first use on the
// calling stream's device.  Two plans driven from two host threads therefore never share an event (different plans are
// independent); calls on ONE stream must be serialised by the caller, as for any HIP stream.
// `counters` (library-owned device memory, zeroed once by side_stream, re-armed by the courier kernel): the courier's per-group flags of a host
// delivery (MAXGROUPS x i64) and its own completion count / error flag — calls on one stream are serialised, so one set per
// calling stream is enough.
// `fetch` is the calling stream's DEVICE-TO-HOST stream (created on first use, highest priority so that it has a hardware queue of its
// own class): recorded fetches (pmt_plan_record_fetch) and the band-wise delivery of pmt_quad_gram_csc_deliver_f64 travel on it while
// the kernels go on; `fetch_done` is recorded behind the last copy enqueued so far.
struct SideStream {
    hipStream_t stream = nullptr; hipEvent_t fork = nullptr, join = nullptr, join2 = nullptr; int device = -1;
    void *counters = nullptr;
    // error word of the kernels that wait on other workgroups with a bound (the courier, the pair fold of gram_sk.hip): page-locked host
    // memory the kernels store to (system scope) and the host reads without a copy in fetch_synchronize.  0 = fine, ERR_* otherwise
    int *err_host = nullptr, *err_dev = nullptr;
    hipStream_t fetch = nullptr; hipEvent_t fetch_done = nullptr; bool fetch_pending = false;
    std::vector<std::pair<dma::Engine *, dma::Signal>> dma_pending;     // completion signals of copy-engine transfers in flight
    std::vector<std::shared_ptr<void>> keepalive;                        // ... and the owners of their signals (an immediate call's go with the call)
    bool in_replay = false;                                              // a plan's tape is being replayed: P's transfers are submitted at its end
    bool side_work = false;                                              // ... and it puts work on `stream`: side-lane entries, or a stream-K node's reductions
    std::vector<std::function<int()>> deferred;
    // the riders of the NEXT one-launch Gram node on this stream: set and cleared around the node by its plan's exec entry (plan.hip), passed
    // on by mid_node (gram.hip); a device table of AffineRider (affine_tile.h), its length, the tiles of all of them
    const void *mid_riders = nullptr; int mid_nriders = 0, mid_rider_tiles = 0;
};
constexpr int ERR_COURIER = 1, ERR_PAIR_FOLD = 2;
// layout of `counters`: [MAXGROUPS x u64 unused][MAXGROUPS x i64 courier flags (armed = 1)][u32 courier done][u32 unused]
constexpr size_t PROGRESS_OFFSET = 0;
constexpr size_t FLAGS_OFFSET = PROGRESS_OFFSET + MAXGROUPS * sizeof(unsigned long long);
constexpr size_t DONE_OFFSET = FLAGS_OFFSET + MAXGROUPS * sizeof(long long);
constexpr size_t MID_OFFSET = DONE_OFFSET + 2 * sizeof(unsigned);                  // per-tile arrival counts of the one-launch mid-size node (gram_mid.hip)
constexpr size_t MID_COUNTER_BYTES = 135168;         // 16 words per tile, 2080 tiles at 4096 columns
constexpr size_t COUNTER_BYTES = MID_OFFSET + MID_COUNTER_BYTES;

SideStream *side_stream(hipStream_t s);            // created on first use; null when it cannot be
int ensure_fetch_stream(SideStream *ss);
int wait_dma_pending(SideStream *ss);               // host: the copy-engine transfers in flight have landed
inline hipStream_t side_stream_of(hipStream_t s) { SideStream *ss = side_stream(s); return ss ? ss->stream : nullptr; }
void retain_side_stream(hipStream_t s);
void release_side_stream(hipStream_t s);
int fetch_async(hipStream_t s, hipStream_t after, hipEvent_t order_event, void *host_dst, const void *device_src, size_t bytes, FetchState *st, FetchRect r);
int fetch_fence(hipStream_t s);
int fetch_synchronize(hipStream_t s);
void replay_begin(hipStream_t s, bool side_work);      // side_work: the tape has side-lane entries (plan.hip: replay)
int replay_end(hipStream_t s);
// at replay time: run `f` on `s` behind the work a plan's replay has deferred to its end on `s`, or now
int gram_after_deferred(hipStream_t s, std::function<int()> f);

// kernel copies into page-locked host memory (deliver.hip)
void *host_device_pointer(void *host);
int launch_courier(const double *src, double *dst_dev, long long *ready, unsigned *done, int *error, int ngroups, const int64_t *gbeg, const int64_t *gend, hipStream_t s);
int launch_to_host(const void *src, void *dst_dev, size_t bytes, hipStream_t s);
int launch_to_host_2d(const void *src, size_t src_pitch, void *dst_dev, size_t dst_pitch, size_t width_bytes, size_t height, hipStream_t s);

}  // namespace pmt
