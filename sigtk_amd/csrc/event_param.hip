// event_param.hip -- k_event_param: event detection with caller-supplied detector parameters (window lengths,
// thresholds, peak height: detector_param of src/events.c:35-41), exact for every set of the documented domain.  None of
// the presets' certificates holds for free parameters, so this is the generic path of event_generic.h as a kernel of
// its own: per read the reference's sequential prefix arrays, both t-statistics from differences of them with
// wf = (float)w at run time, the two automata stepped short-then-long at every index on speculative chunks that are
// re-run until the lanes' states agree, and the builder on the prefix arrays.
//
// A persistent grid: every workgroup (one wavefront) owns a scratch range for the longest read -- two prefix arrays of
// max_read_len + 1 doubles and the read's peak bitmap -- and takes reads from an atomic counter, longest first when the
// batch has a dispatch order.  The workspace therefore grows with the workgroups and the longest read, not with the
// batch's samples.  The map of the event units is in event_device.h.
#include "event_generic.h"

namespace sgk {

// tile of the prefix scan: 12 KB of LDS per workgroup, so that LDS does not bound the resident workgroups
// (PARAM_MAX_BLOCKS, event_args.h, does: by measurement)
constexpr int PARAM_SP_TILE = 512;

template <typename T>
__global__ __launch_bounds__(64) void k_event_param(EvArgs a, EvParamArgs pa) {
    __shared__ PrefixLdsT<PARAM_SP_TILE> L;
    double *P = a.scratch + (uint64_t)blockIdx.x * a.scratch_stride;
    double *P2 = P + ((uint64_t)pa.max_read_len + 1);
    unsigned long long *bm = reinterpret_cast<unsigned long long *>(P2 + ((uint64_t)pa.max_read_len + 1));
    DetVals dv;
    dv.w1 = (int)pa.w1;
    dv.w2 = (int)pa.w2;
    dv.thr1 = pa.thr1;
    dv.thr2 = pa.thr2;
    dv.ph = pa.ph;
    for (;;) {
        uint32_t w = 0;
        if (lane_id() == 0) w = atomicAdd(&a.hdr->fb_next, 1u);
        w = __shfl(w, 0, 64);
        if (w >= a.n_reads) break;
        const uint32_t r = a.order ? a.order[w] : w;
        ReadCtx<T> rc = make_ctx<T>(a, r);
        if (rc.n > (int64_t)pa.max_read_len) {
            // a read longer than the batch said its longest is: no room for its prefix arrays.  No events, and the
            // status reports a capacity overflow.
            if (lane_id() == 0) {
                a.n_events[r] = 0;
                atomicAdd(&a.hdr->n_overflow, 1u);
            }
            continue;
        }
        rc.bm = bm;
        seq_prefix<T, 1>(rc, P, P2, &L, static_cast<EventListT<1> *>(nullptr));
        rc.P = P;
        rc.P2 = P2;
        detect_read<0, T>(rc, dv, pa.lead, a.hdr);
        __threadfence();
        __syncthreads();
        build_read_prefix<T>(a, rc, r);
        __syncthreads();
    }
}

int launch_k_event_param(bool float_input, uint32_t n_blocks, hipStream_t st, const EvArgs &a, const EvParamArgs &pa) {
    if (float_input) SGK_LAUNCH("k_event_param", (k_event_param<float>), n_blocks, 64, st, a, pa);
    else SGK_LAUNCH("k_event_param", (k_event_param<int16_t>), n_blocks, 64, st, a, pa);
    return SGK_OK;
}

}  // namespace sgk
