// event_multi.hip -- k_event_multi: several short reads per wavefront.  The map of the event units is in event_device.h.
#include "event_build.h"

namespace sgk {

// Short reads, several per wavefront: `lanes` consecutive lanes share a read (detector: detect_span<MULTI>), then the
// wave builds its reads one after the other.  The short reads are the tail of the dispatch order (launch_order sorts by
// length class, longest first; multi_max is a class boundary) or, in a batch without an order, all reads.
template <int W1, typename T, bool RT = false>
__global__ __launch_bounds__(64, (W1 == 3 ? DET_WAVES_DNA : DET_WAVES_RNA)) void k_event_multi(EvArgs a) {
    __shared__ EventLds L;
    const int lanes = (int)a.multi_lanes, G = 64 / lanes;
    const int l = lane_id();
    const uint32_t first = a.order ? a.order[a.n_reads + len_bucket(a.multi_max)] : 0u;  // reads that are not short
    const uint32_t nshort = a.n_reads - first;
    const uint32_t w0 = blockIdx.x * (uint32_t)G;
    if (w0 >= nshort) return;
    const uint32_t gi = (uint32_t)l / (uint32_t)lanes;
    const bool has = w0 + gi < nshort;
    const uint32_t idx = first + (has ? w0 + gi : w0);
    const uint32_t r = a.order ? a.order[idx] : idx;
    ReadCtx<T> rc = make_ctx<T>(a, r);
    // (with segments shorter than multi_max -- tests -- a read can be short and long at once: the segments have it)
    const bool mine = has && !(a.max_segs && rc.n >= (int64_t)a.long_min);  // (no tail split in a batch with packed reads)
    if (!mine) rc.n = 0;
    constexpr bool MULTI_LEAD = W1 == 3 && ((SGK_EVENT_LEAD) & 4) != 0;  // (off in the shipped build, event_detect.h)
    const int rcode = detect_span<W1, T, false, true, MULTI_LEAD, RT>(rc, a.hdr, &L.lz, nullptr, 0, (int)rc.n, 0,
                                                                  a.lead_override, nullptr, lanes, Det<W1, RT>(a));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    constexpr bool MULTI_CARRY = ((SGK_BUILD_CARRY) & 2) != 0;  // (off in the shipped build, event_build.h)
    for (int g = 0; g < G; ++g) {
        if (w0 + (uint32_t)g >= nshort) break;
        const uint32_t rg = (uint32_t)__builtin_amdgcn_readlane((int)r, g * lanes);
        const int code = __builtin_amdgcn_readlane(rcode, g * lanes);
        if (!__builtin_amdgcn_readlane((int)mine, g * lanes)) continue;
        const ReadCtx<T> rcg = make_ctx<T>(a, rg);
        build_read<T, false, MULTI_CARRY>(a, rcg, rg, build_lds<MULTI_CARRY>(&L), code != 0);
        __syncthreads();
    }
}

int launch_k_event_multi(int rna, bool float_input, hipStream_t st, const EvArgs &a, bool rt) {
    const uint32_t per_wave = 64u / a.multi_lanes;
    const uint32_t grid = (a.n_reads + per_wave - 1) / per_wave;
    return event_instance(rna, float_input, rt, [&](auto w1, auto t, auto r) -> int {
        SGK_LAUNCH("k_event_multi", (k_event_multi<decltype(w1)::value, decltype(t), decltype(r)::value>), grid, 64, st, a);
        return SGK_OK;
    });
}

}  // namespace sgk
