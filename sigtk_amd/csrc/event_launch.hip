// event_launch.hip -- host side of `event`: the dispatch order, the segment plan, the side streams and the order of the
// launches.  It holds no kernel and includes no device header: every kernel is launched through the launch_k_* function
// its own unit exports (event_args.h).  The map of the event units is in event_device.h.
#include "event_args.h"
#include "side_stream.h"
#include "stat_args.h"
#include "sgk_common.h"

namespace sgk {

// Side streams (side_stream.h).  A batch with short AND longer reads runs two detector kernels: k_event (a wavefront per
// read) and k_event_multi (several short reads per wavefront).  In one stream the
// second would wait for the last wave of the first -- two tails instead of one, which costs what the packing gains
// (50 000 RNA-like reads, log-normal around 20 000 samples: 6.36 ms against 6.29 ms with a wavefront per read).
// k_event_multi therefore goes to a side stream of the library's own, forked off the caller's stream behind the dispatch
// order and joined in front of the fallback kernel; the long reads' chains (k_event_seg) overlap with it as well.
// (Tried in round 1: cutting the batch into read slices and running the builder of slice s on a side stream under the
// detector of slice s+1.  Both kernels contend for VALU issue and the detector needs >= 3072 reads in flight to fill its
// 12 waves/CU, so the overlapped step was 8.8 ms against 7.8 ms.)
int launch_event(const EvArgs &a, int rna, bool float_input, uint32_t n_fb_blocks, hipStream_t st, bool rt) {
    if (a.n_reads == 0) return SGK_OK;
    ProfScope whole("path:event", st);
    SGK_HIP_TRY(hipMemsetAsync(a.hdr, 0, sizeof(EvHeader), st));
    EvArgs ao = a;
    if (a.n_reads >= ORDER_MIN_READS && a.order) {
        const int rc = launch_order(a.lengths, a.n_reads, a.order, a.order + a.n_reads, st);
        if (rc != SGK_OK) return rc;
    } else ao.order = nullptr;
    int rc = SGK_OK;
    if (ao.max_segs) rc = launch_k_seg_plan(st, ao);
    // The segments' kernel.  Long reads' segments start FIRST: they stay on the caller's stream and k_event goes to a
    // side stream whose start waits for the fork event (the other way round k_event's workgroups -- ten thousand of them
    // -- take every slot and the chains start late: a ragged batch took 3.81 ms instead of 3.65; stat's long reads taught
    // the same, stat_launch.hip launch_beside_long).  The tail split's segments go LAST, behind k_event on the caller's
    // stream: small units for the slots the last whole reads leave empty.  (Tried for them: a stream of the LOWEST
    // priority, to be dispatched into the slots k_event's last waves leave empty -- 5.1 vs 3.8 ms on config 2.)
    const bool tail_only = ao.max_segs && ao.split_seg && !ao.has_long;
    // (no dispatch order and packing on: every read is under multi_max.  k_event would have nothing to do -- unless
    // the segments are test-sized and some of those reads are long: their segments are k_event_seg's)
    const bool all_short = ao.multi_lanes && !ao.order && !ao.max_segs;
    const bool side_multi = ao.multi_lanes && !all_short, side_whole = ao.max_segs && !tail_only && !all_short;
    SideFork side;
    side.open(st, (int)side_multi + (int)side_whole);
    const hipStream_t st_multi = side_multi ? side.stream(0) : st;
    const hipStream_t st_whole = side_whole ? side.stream(side_multi ? 1 : 0) : st;
    if (rc == SGK_OK && ao.max_segs && !tail_only) rc = launch_k_event_seg(rna, float_input, st, ao, rt);
    if (rc == SGK_OK && ao.multi_lanes) rc = launch_k_event_multi(rna, float_input, st_multi, ao, rt);
    if (rc == SGK_OK && !all_short) rc = launch_k_event(rna, float_input, st_whole, ao, rt);
    if (rc == SGK_OK && tail_only) rc = launch_k_event_seg(rna, float_input, st, ao, rt);
    // join: the fallback kernel (and whatever the caller enqueues next) waits for the side streams as well
    side.join();
    if (rc != SGK_OK) return rc;
    return launch_k_event_fallback(rna, float_input, n_fb_blocks, st, a, rt);
}

// The generic kernel for caller-supplied parameters: the header, the dispatch order, one persistent launch.
int launch_event_param(const EvArgs &a, const EvParamArgs &pa, bool float_input, uint32_t n_blocks, hipStream_t st) {
    if (a.n_reads == 0) return SGK_OK;
    ProfScope whole("path:event_param", st);
    SGK_HIP_TRY(hipMemsetAsync(a.hdr, 0, sizeof(EvHeader), st));
    EvArgs ao = a;
    if (a.n_reads >= ORDER_MIN_READS && a.order) {
        const int rc = launch_order(a.lengths, a.n_reads, a.order, a.order + a.n_reads, st);
        if (rc != SGK_OK) return rc;
    } else ao.order = nullptr;
    return launch_k_event_param(float_input, n_blocks, st, ao, pa);
}

}  // namespace sgk
