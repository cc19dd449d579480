// event_fallback.hip -- k_event_fallback: the reads that fail the exactness guard, redone on the reference's own
// sequentially rounded prefix arrays.  The prefix scan (seq_prefix), the generic detector on those arrays (detect_pass /
// detect_read, for reads the fast pass cannot take at all) and the builder on them (build_read_prefix) are
// event_generic.h's, shared with k_event_param.  The fast pass with its repair context (FLAGGED) is event_detect.h's.
// The map of the event units is in event_device.h.
#include "event_detect.h"
#include "event_generic.h"

namespace sgk {

using EventList = EventListT<REP_MAX_EVENTS>;

// RT: the preset's windows, thresholds from the arguments -- in the fast pass with its repair context and in the
// generic pass alike
template <int W1, typename T, bool RT = false>
__global__ __launch_bounds__(64) void k_event_fallback(EvArgs a) {
    __shared__ PrefixLds L;
    __shared__ LzLds Lz;
    __shared__ EventList events;
    double *P = a.scratch + (uint64_t)blockIdx.x * a.scratch_stride;
    double *P2 = P + a.scratch_stride / 2;
    const uint32_t nf = a.hdr->n_flagged;
    const Det<W1, RT> dt(a);
    const DetVals dv = RT ? DetVals{W1, 2 * W1, dt.thr1(), dt.thr2(), dt.ph()} : DetVals{};  // (RT = false: det_vals ignores it)
    for (;;) {
        uint32_t w = 0;
        if (lane_id() == 0) w = atomicAdd(&a.hdr->fb_next, 1u);
        w = __shfl(w, 0, 64);
        if (w >= nf) break;
        const uint32_t r = a.flag_list[w];
        ReadCtx<T> rc = make_ctx<T>(a, r);
        seq_prefix<T, REP_MAX_EVENTS>(rc, P, P2, &L, &events);
        rc.P = P;
        rc.P2 = P2;
        // fast pass + event-local repair; reads the fast pass cannot take (odd alignment, no room around
        // the read) go through the generic pass that takes every window sum from the prefix arrays
        RepairCtx rep;
        rep.P = P;
        rep.P2 = P2;
        rep.ev = events.ev;
        rep.nev = events.count < REP_MAX_EVENTS ? events.count : REP_MAX_EVENTS;
        rep.all_dirty = events.count > REP_MAX_EVENTS;
        const int rcode = detect_read_lazy<W1, T, true, RT>(rc, a.hdr, &Lz, &rep, dt);
        if (rcode) detect_read<W1, T, RT>(rc, dv, LEAD, a.hdr);
        __threadfence();
        __syncthreads();
        build_read_prefix<T>(a, rc, r);
        __syncthreads();
    }
}

int launch_k_event_fallback(int rna, bool float_input, uint32_t n_fb_blocks, hipStream_t st, const EvArgs &a, bool rt) {
    return event_instance(rna, float_input, rt, [&](auto w1, auto t, auto r) -> int {
        SGK_LAUNCH("k_event_fallback", (k_event_fallback<decltype(w1)::value, decltype(t), decltype(r)::value>), n_fb_blocks, 64, st, a);
        return SGK_OK;
    });
}

}  // namespace sgk
