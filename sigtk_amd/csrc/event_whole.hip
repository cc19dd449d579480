// event_whole.hip -- k_event: a whole read on one wavefront, detector and builder back to back.  The map of the event
// units is in event_device.h.
#include "event_build.h"

namespace sgk {

// (the DNA preset's instances take the leading-edge form of the fast pass: SGK_EVENT_LEAD, event_detect.h)
template <int W1>
constexpr bool EV_LEAD = ((SGK_EVENT_LEAD) & (W1 == 3 ? 1 : 2)) != 0;

// (and the carrying form of the builder: SGK_BUILD_CARRY, event_build.h)
template <int W1>
constexpr bool EV_CARRY = ((SGK_BUILD_CARRY) & (W1 == 3 ? 1 : 2)) != 0;

// RT: the thresholds come from the arguments (Det<W1, RT>, event_device.h)
template <int W1, typename T, bool RT = false>
__global__ __launch_bounds__(64, (W1 == 3 ? DET_WAVES_DNA : DET_WAVES_RNA)) void k_event(EvArgs a) {
    __shared__ EventLds L;
    // One read per workgroup, longest first (launch_order): a kernel cannot end before its longest read has, so that one
    // should start first, not wherever it sits in the batch.  Reads that several waves share -- long reads, the tail
    // split -- are k_event_seg's (round 5: a kernel of its own.  While one kernel held both paths the whole-read path --
    // 9 216 of config 2's 10 000 workgroups -- carried the chain's state: 33 spilled registers, 688 bytes of scratch per
    // lane; as a device function called from here the chain spilled in its own detector pass instead.)
    const uint32_t bi = blockIdx.x;
    const uint32_t r = a.order ? a.order[bi] : bi;
    const ReadCtx<T> rc = make_ctx<T>(a, r);
    if (seg_len_of(a, bi, (uint32_t)rc.n) != 0u) return;  // taken by its segments (k_event_seg)
    if (a.multi_lanes && rc.n < (int64_t)a.multi_max) return;  // taken by k_event_multi
#ifdef SGK_DEV  // development builds (tools/build_variant.sh): phases switched off / timestamps, see event_args.h
    unsigned long long t0 = 0ull, t1 = 0ull;
    if (a.dev & SGK_DEV_TRACE) t0 = wall_clock64();
    int rcode = 0;
    if (!(a.dev & SGK_DEV_NO_DETECT)) rcode = detect_span<W1, T, false, false, EV_LEAD<W1>, RT>(rc, a.hdr, &L.lz, nullptr, 0, (int)rc.n, 0, a.lead_override, nullptr, 64, Det<W1, RT>(a));
    if (a.dev & SGK_DEV_TRACE) t1 = wall_clock64();
#else
    const int rcode = detect_span<W1, T, false, false, EV_LEAD<W1>, RT>(rc, a.hdr, &L.lz, nullptr, 0, (int)rc.n, 0, a.lead_override, nullptr, 64, Det<W1, RT>(a));
#endif
    // the bitmap words of every lane (and the replay's atomics) are complete before any lane of this workgroup reads
    // them back.  Workgroup scope: the wave's own CU only -- an agent-scope release / acquire pair here writes back and
    // invalidates L2 once per read, which made 5 000-sample reads 1.7x slower than with two kernels.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#ifdef SGK_DEV
    if (!(a.dev & SGK_DEV_NO_BUILD)) build_read<T, false, EV_CARRY<W1>>(a, rc, r, build_lds<EV_CARRY<W1>>(&L), rcode != 0);
    if ((a.dev & SGK_DEV_TRACE) && lane_id() == 0) {
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        unsigned long long *tr = reinterpret_cast<unsigned long long *>(a.scratch) + 4ull * blockIdx.x;
        tr[0] = t0;
        tr[1] = t1;
        tr[2] = wall_clock64();
        tr[3] = ((unsigned long long)xcc << 32) | hw;
    }
#else
    build_read<T, false, EV_CARRY<W1>>(a, rc, r, build_lds<EV_CARRY<W1>>(&L), rcode != 0);
#endif
}

int launch_k_event(int rna, bool float_input, hipStream_t st, const EvArgs &a, bool rt) {
    return event_instance(rna, float_input, rt, [&](auto w1, auto t, auto r) -> int {
        SGK_LAUNCH("k_event", (k_event<decltype(w1)::value, decltype(t), decltype(r)::value>), a.n_reads, 64, st, a);
        return SGK_OK;
    });
}

}  // namespace sgk
