// event_seg.hip -- reads that several wavefronts share (long reads, the tail split): the list of their segments
// (k_seg_plan) and the chain that runs detector, seam check and builder of a segment in one wave (k_event_seg).  The map
// of the event units is in event_device.h.
#include "event_build.h"

namespace sgk {

// The list of their segments (one thread per dispatch position; the order of the list does not matter).
__global__ __launch_bounds__(256) void k_seg_plan(EvArgs a) {
    const uint32_t pos = blockIdx.x * 256u + threadIdx.x;
    if (pos >= a.n_reads) return;
    const uint32_t r = a.order ? a.order[pos] : pos;
    const uint32_t n = a.lengths[r];
    const uint32_t seg = seg_len_of(a, pos, n);
    if (seg == 0u) return;
    const uint32_t G = (uint32_t)(((uint64_t)n + seg - 1) / seg);
    const uint32_t s0 = atomicAdd(&a.hdr->n_segs, G), li = atomicAdd(&a.hdr->n_long, 1u);
    // The capacities cover every batch of non-overlapping reads with these totals (event_seg_capacity).  A read that
    // does not fit all the same (overlapping reads) is left to the exact fallback; what it took of the lists is marked
    // as nobody's.
    if ((uint64_t)s0 + G > a.max_segs || li >= a.max_long) {
        for (uint64_t k = s0; k < (uint64_t)s0 + G && k < a.max_segs; ++k) a.segs[k].read = SEG_NONE;
        if (li < a.max_long) {
            LongRead none;
            none.read = r; none.seg0 = 0; none.nseg = 0; none.seg_len = seg;
            none.ext_lo = 0; none.ext_hi = 0; none.flags = 0; none.built = 0;
            a.longs[li] = none;
        }
        a.flags[r] = 1;
        a.flag_list[atomicAdd(&a.hdr->n_flagged, 1u)] = r;
        return;
    }
    LongRead lr;
    lr.read = r; lr.seg0 = s0; lr.nseg = G; lr.seg_len = seg;
    lr.ext_lo = a.dig ? 32767u : 0xffffffffu;          // (int16 input: signed extremes; pA input: bit patterns)
    lr.ext_hi = a.dig ? (uint32_t)-32768 : 0u;
    lr.flags = 0; lr.built = 0;
    a.longs[li] = lr;
    for (uint32_t g = 0; g < G; ++g) {
        SegDesc d;
        d.read = r; d.g = g; d.lread = li; d.pad = 0;
        a.segs[s0 + g] = d;
        a.seg_state[s0 + g].stage = 0u;   // (the chain: nothing of this segment is published yet)
    }
}

// ---- the chain: detector, seam check and builder of one segment in one wave (round 4) -------------------------
// Round 3 ran the segments' detector passes in k_event and left the rest to four kernels behind it (seams, counts,
// builders, verdict): a cut read lost the fusion of detector and builder, and every kernel had a tail of its own.  Now
// the wave of segment g does everything itself and takes what it needs from segment g - 1 -- ALWAYS a lower workgroup
// index, so with workgroups started in index order (what the hardware does, per XCD; decoupled look-back scans rely on
// the same) the chain cannot deadlock; a wait that exceeds ~1 s all the same declines the read (exact fallback).
//   1. detect_span over the segment, speculative start (mode 1): bitmap words of ITS range only;
//   2. wait for segment g - 1's record {final end state, boundaries so far, the last of them, declined?} -- 40 bytes,
//      published with agent-scope atomic stores (write-through) behind an s_waitcnt, read back with agent-scope atomic
//      loads behind one agent acquire (MI355X_MICROARCH.md, inter-workgroup visibility: the XCDs' L2s are not coherent);
//   3. the seam: end(g - 1) != its own init0 -> the segment is run again from the true state (mode 2);
//   4. publish its own record (so the segments behind need not wait for its builder);
//   5. build the events that end at the boundaries it OWNS: those inside its range and the peaks that were pending at
//      the seam and emitted behind it (seg->pre: positions in front of the segment that no bitmap shows) -- from the
//      last boundary of the segments in front, at the rank their boundaries give;
//   6. extremes / flags into the read's record (atomics); the wave that finishes last gives the verdict (exactness
//      guard over the whole read, n_events, counters, fallback list).
// A hot long-detector run that crosses the seam is replayed for the part in front of it as well; a peak found there
// (none on nanopore-like signals) would belong to another wave's events: the read is declined.
__device__ __forceinline__ uint32_t ld_agent(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(uint32_t *p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// (ONE call site of detect_span for the speculative pass and the re-run from the true state: each inlined copy of the
// detector pass is ~25 KB of code.)
template <int W1, typename T, bool RT = false>
__device__ __forceinline__ void chain_segment(const EvArgs &a, uint32_t bx, EventLds *L) {
    if (bx >= a.hdr->n_segs) return;
    const SegDesc d = a.segs[bx];
    if (d.read == SEG_NONE) return;
    const uint32_t r = d.read, g = d.g, lread = d.lread;
    const ReadCtx<T> rc = make_ctx<T>(a, r);
    LongRead *lrp = a.longs + lread;
    const uint32_t seg_len = lrp->seg_len;
    int sa, sb;
    seg_span(seg_len, g, rc.n, sa, sb);
    SegState *st = a.seg_state + bx;
    const int l = lane_id();
    const Det<W1, RT> dt(a);
    const uint32_t nseg = lrp->nseg;
    bool declined = false;
    uint32_t prev_cum = 0u;
    int prev_last = -1;
    int mode = g == 0 ? 0 : 1;
#ifdef SGK_DEV
    unsigned long long tt0 = 0ull, tt1 = 0ull, tt2 = 0ull;
    if (a.dev & SGK_DEV_TRACE) tt0 = wall_clock64();
#endif
    for (int attempt = 0; attempt < 2; ++attempt) {
        const int rcode = detect_span<W1, T, false, false, false, RT>(rc, a.hdr, &L->lz, nullptr, sa, sb, mode, a.lead_override, st, 64, dt);
#ifdef SGK_DEV
        if ((a.dev & SGK_DEV_TRACE) && attempt == 0) tt1 = wall_clock64();
#endif
        if (l == 0) st->status = rcode;
        declined = rcode != 0;
        // (what detect_span's lanes stored -- st->end, cross runs, pre peaks -- is visible to the wave's other lanes)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (g == 0 || attempt == 1) break;
        SegState *ps = st - 1;
        int ok = 1;
        if (l == 0) {
            unsigned spins = 0;
            while (ld_agent(&ps->stage) == 0u) {
                __builtin_amdgcn_s_sleep(8);
                if (++spins > 4000000u) { ok = 0; break; }
            }
        }
        ok = __builtin_amdgcn_readfirstlane(ok);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        LzSnapState pe;
        pe.sp = (int)ld_agent(reinterpret_cast<const uint32_t *>(&ps->end.sp));
        pe.sv = __uint_as_float(ld_agent(reinterpret_cast<const uint32_t *>(&ps->end.sv)));
        pe.lm = (int)ld_agent(reinterpret_cast<const uint32_t *>(&ps->end.lm));
        pe.r0 = (int)ld_agent(reinterpret_cast<const uint32_t *>(&ps->end.r0));
        pe.bits = ld_agent(&ps->end.bits);
        prev_cum = ld_agent(&ps->cum_cnt);
        prev_last = (int)ld_agent(reinterpret_cast<const uint32_t *>(&ps->last_pos));
        if (!ok || (ld_agent(&ps->cflags) & 1u)) declined = true;
        if (declined) break;
        // the seam (st->init0 / st->end: this wave's own stores; the states are in LDS as well)
        const LzSnapState mine = L->lz.snap.init[0];
        if (lz_equal(pe, mine)) break;
        __syncthreads();
        if (l == 0) {
            L->lz.snap.st0[0] = pe;
            atomicAdd(&a.hdr->n_seam_rerun, 1u);
        }
        __syncthreads();
        mode = 2;   // once more, from the true state
    }
    if (g > 0 && !declined) {
        // hot runs that began in front of the seam: the part in front of it
        __syncthreads();
        const int nc = (int)st->n_cross;
        if (nc > 0) {
            const bool has = l < nc;
            const LzRun run = has ? st->cross[l] : LzRun{0, 0};
            int found = 0;
            replay_run<W1, T, false, true, RT>(rc, nullptr, has, run.a, run.b, 0, sa, a.hdr, &found, dt);
            if (__any(found != 0)) declined = true;
        }
    }
    // this wave's bitmap words (and the replay's atomics) are complete before any of its lanes reads them back
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // the boundaries the segment owns: the bits of its range + its pre peaks
    int cnt = 0, last = -1, n_pre = 0;
    if (!declined) {
        const int w0 = sa >> 6, w1 = (sb + 63) >> 6;
        for (int wb = w0; wb < w1; wb += 64) {
            const int w = wb + l;
            unsigned long long v = w < w1 ? rc.bm[w] : 0ull;
            const int rem = sb - (w << 6);
            if (rem < 64) v = rem <= 0 ? 0ull : (v & ((1ull << rem) - 1ull));
            if (v) {
                cnt += __popcll(v);
                last = (w << 6) + 63 - __clzll(v);
            }
        }
#pragma unroll
        for (int dd = 32; dd >= 1; dd >>= 1) {
            cnt += __shfl_xor(cnt, dd, 64);
            const int o = __shfl_xor(last, dd, 64);
            last = o > last ? o : last;
        }
        n_pre = (int)st->n_pre;
        if (last < 0) {
            for (int k = 0; k < n_pre; ++k) last = st->pre[k] > last ? st->pre[k] : last;
            if (last < 0) last = prev_last;
        }
    }
    const uint32_t my_cum = prev_cum + (uint32_t)(cnt + n_pre);
    // publish (the end state: what detect_span left in st->end -- lane 0's own store)
    if (l == 0) {
        const LzSnapState e = st->end;
        st_agent(reinterpret_cast<uint32_t *>(&st->end.sp), (uint32_t)e.sp);
        st_agent(reinterpret_cast<uint32_t *>(&st->end.sv), __float_as_uint(e.sv));
        st_agent(reinterpret_cast<uint32_t *>(&st->end.lm), (uint32_t)e.lm);
        st_agent(reinterpret_cast<uint32_t *>(&st->end.r0), (uint32_t)e.r0);
        st_agent(&st->end.bits, e.bits);
        st_agent(&st->cum_cnt, my_cum);
        st_agent(reinterpret_cast<uint32_t *>(&st->last_pos), (uint32_t)(declined ? prev_last : last));
        st_agent(&st->cflags, declined ? 1u : 0u);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        st_agent(&st->stage, 1u);
    }
    uint32_t fl = declined ? 1u : 0u;
#ifdef SGK_DEV
    if (a.dev & SGK_DEV_TRACE) tt2 = wall_clock64();
#endif
    if (!declined) {
        constexpr bool SEG_CARRY = ((SGK_BUILD_CARRY) & 2) != 0;  // (off in the shipped build, event_build.h)
        build_read<T, true, SEG_CARRY>(a, rc, r, build_lds<SEG_CARRY>(L), false, sa, sb, st, prev_cum, prev_last, st->pre, n_pre);
        __syncthreads();
#ifdef SGK_DEV
        if ((a.dev & SGK_DEV_TRACE) && l == 0) {   // (segments: start, detector end, seam + publish end | builder end in the top bits)
            unsigned long long *tr = reinterpret_cast<unsigned long long *>(a.scratch) + 4ull * (a.n_reads + blockIdx.x);
            tr[0] = tt0;
            tr[1] = tt1;
            tr[2] = wall_clock64();
            tr[3] = (1ull << 63) | ((tt2 - tt0) << 16) | (g & 0xffffu);
        }
#endif
        if (l == 0) {
            const uint32_t lo = st->ext_lo, hi = st->ext_hi;
            if constexpr (std::is_same<T, int16_t>::value) {
                atomicMin(reinterpret_cast<int *>(&lrp->ext_lo), (int)lo);
                atomicMax(reinterpret_cast<int *>(&lrp->ext_hi), (int)hi);
            } else {
                atomicMin(&lrp->ext_lo, lo);
                atomicMax(&lrp->ext_hi, hi);
            }
            fl = st->bflags;
        }
    }
    if (l != 0) return;
    if (fl) atomicOr(&lrp->flags, fl);
    // (everything the verdict reads was written with device-scope atomics, which complete in memory: this lane's have
    // before it counts itself done.  NO agent-scope fence: its write-back of the XCD's whole L2 -- megabytes of other
    // waves' event stores -- once per segment made the chain slower than no split at all, 3.95 vs 3.86 ms)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t done = atomicAdd(&lrp->built, 1u);
    if (done + 1u != nseg) return;
    // the verdict (every segment has published its record and added its extremes / flags)
    const uint32_t flags = atomicOr(&lrp->flags, 0u);
    const int64_t n = rc.n;
    bool flagged = (flags & 1u) != 0u;
    if (!flagged) {
        float mn, mx;
        bool known;
        if constexpr (std::is_same<T, int16_t>::value) {
            const int rmn = atomicMin(reinterpret_cast<int *>(&lrp->ext_lo), 32767);
            const int rmx = atomicMax(reinterpret_cast<int *>(&lrp->ext_hi), -32768);
            known = raw_extremes_to_pa(rmn, rmx, rc.sc, mn, mx);
        } else {
            const uint32_t mnb = atomicMin(&lrp->ext_lo, 0xffffffffu), mxb = atomicMax(&lrp->ext_hi, 0u);
            mn = (mnb == 0xffffffffu) ? FLT_MAX : __uint_as_float(mnb + 1u);
            mx = __uint_as_float(mxb);
            known = mxb < 0x7f800000u;
        }
        flagged = !known || !guard_ok(mn, mx, n);
    }
    a.flags[r] = flagged ? 1 : 0;
    if (flagged) {
        a.flag_list[atomicAdd(&a.hdr->n_flagged, 1u)] = r;
    } else {
        const uint32_t nev = ld_agent(&a.seg_state[lrp->seg0 + nseg - 1u].cum_cnt) + 1u;
        a.n_events[r] = nev;
        atomicAdd(&a.hdr->n_events_total, (unsigned long long)nev);
        if (flags & 2u) atomicAdd(&a.hdr->n_overflow, 1u);
    }
}

// The segments' kernel: a workgroup per entry of the segment list (usually much shorter than its capacity).
template <int W1, typename T, bool RT = false>
__global__ __launch_bounds__(64, (W1 == 3 ? DET_WAVES_DNA : DET_WAVES_RNA)) void k_event_seg(EvArgs a) {
    __shared__ EventLds L;
    chain_segment<W1, T, RT>(a, blockIdx.x, &L);
}

int launch_k_seg_plan(hipStream_t st, const EvArgs &a) {
    SGK_LAUNCH_UNTIMED(k_seg_plan, (a.n_reads + 255) / 256, 256, st, a);
    return SGK_OK;
}
int launch_k_event_seg(int rna, bool float_input, hipStream_t st, const EvArgs &a, bool rt) {
    return event_instance(rna, float_input, rt, [&](auto w1, auto t, auto r) -> int {
        SGK_LAUNCH("k_event_seg", (k_event_seg<decltype(w1)::value, decltype(t), decltype(r)::value>), a.max_segs, 64, st, a);
        return SGK_OK;
    });
}

}  // namespace sgk
