// event_fallback.hip -- k_event_fallback: the reads that fail the exactness guard, redone on the reference's own
// sequentially rounded prefix arrays, and everything only this kernel uses: the prefix scan (seq_prefix), the generic
// detector on those arrays (detect_pass / detect_read, for reads the fast pass cannot take at all) and the builder on
// them (build_read_prefix).  The fast pass with its repair context (FLAGGED) is event_detect.h's.  The map of the event
// units is in event_device.h.
#include "event_detect.h"

namespace sgk {

constexpr int LEAD = 64;   // speculative warm-up (samples) of the generic pass; multiple of 64
// chunk length of the generic pass: 64 lanes x K samples cover the read, K a multiple of 64 (its bitmap words are
// 64-bit)
__device__ inline uint32_t chunk_len(int64_t n) {
    const int64_t k = (n + 4095) / 4096;
    return (uint32_t)(k < 1 ? 64 : 64 * k);
}

// ---------------------------------------------------------------- detector state
struct DetState {
    int sp;      // short peak_pos (-1 none)
    float sv;    // short peak_value
    int svalid;
    int lp;      // long peak_pos
    float lv;
    int lvalid;
    int lmask;   // long masked_to, normalised to -1 when it no longer masks
};
__device__ inline DetState det_fresh(int masked_to) {
    DetState d;
    d.sp = -1; d.sv = FLT_MAX; d.svalid = 0;
    d.lp = -1; d.lv = FLT_MAX; d.lvalid = 0;
    d.lmask = masked_to;
    return d;
}
__device__ inline DetState det_norm(DetState d, int i) {
    if (d.lmask < i) d.lmask = -1;
    return d;
}
__device__ inline bool det_equal(const DetState &a, const DetState &b) {
    return a.sp == b.sp && __float_as_int(a.sv) == __float_as_int(b.sv) && a.svalid == b.svalid &&
           a.lp == b.lp && __float_as_int(a.lv) == __float_as_int(b.lv) && a.lvalid == b.lvalid &&
           a.lmask == b.lmask;
}
__device__ inline DetState det_shfl_up(const DetState &a) {
    DetState r;
    r.sp = __shfl_up(a.sp, 1, 64);
    r.sv = __shfl_up(a.sv, 1, 64);
    r.svalid = __shfl_up(a.svalid, 1, 64);
    r.lp = __shfl_up(a.lp, 1, 64);
    r.lv = __shfl_up(a.lv, 1, 64);
    r.lvalid = __shfl_up(a.lvalid, 1, 64);
    r.lmask = __shfl_up(a.lmask, 1, 64);
    return r;
}

// One index of short_long_peak_detector (src/events.c:383-440): short first, then long.
// emit_s / emit_l receive the emitted peak position of each detector, or -1.
template <int W1>
__device__ inline void det_step(DetState &d, int i, float v1, float v2, int &emit_s, int &emit_l) {
    constexpr int W2 = 2 * W1;
    constexpr float ph = DetParam<W1>::ph;
    emit_s = -1;
    emit_l = -1;
    // ---- short detector: its masked_to stays 0, so only index 0 is skipped (events.c:387)
    if (i > 0) {
        if (d.sp < 0) {
            if (v1 < d.sv) {
                d.sv = v1;
            } else if (v1 - d.sv > ph) {
                d.sv = v1;
                d.sp = i;
            }
        } else {
            if (v1 > d.sv) {
                d.sv = v1;
                d.sp = i;
            }
            if (d.sv > DetParam<W1>::thr1) {  // dominate the long detector (events.c:414-422)
                d.lmask = d.sp + W1;
                d.lp = -1;
                d.lv = FLT_MAX;
                d.lvalid = 0;
            }
            if (d.sv - v1 > ph && d.sv > DetParam<W1>::thr1) d.svalid = 1;
            if (d.svalid && (i - d.sp) > W1 / 2) {
                emit_s = d.sp;
                d.sp = -1;
                d.sv = v1;
                d.svalid = 0;
            }
        }
    }
    // ---- long detector
    if (!(d.lmask >= i)) {
        if (d.lp < 0) {
            if (v2 < d.lv) {
                d.lv = v2;
            } else if (v2 - d.lv > ph) {
                d.lv = v2;
                d.lp = i;
            }
        } else {
            if (v2 > d.lv) {
                d.lv = v2;
                d.lp = i;
            }
            if (d.lv - v2 > ph && d.lv > DetParam<W1>::thr2) d.lvalid = 1;
            if (d.lvalid && (i - d.lp) > W2 / 2) {
                emit_l = d.lp;
                d.lp = -1;
                d.lv = v2;
                d.lvalid = 0;
            }
        }
    }
}

// One pass of the GENERIC detector over the wave's chunks: every window sum is a difference of the reference's
// prefix arrays (rc.P / rc.P2), both detectors step on every index.  Slow (uncoalesced loads of the prefix arrays,
// library division and sqrt); only the fallback kernel uses it, for reads the fast pass cannot take.
//   lead   : samples each lane starts before its chunk start (LEAD: speculative pass, 0: re-run)
//   active : whether this lane runs in this pass
//   st     : state at the pass start (lead == 0 only; the speculative pass starts fresh)
//   at_s   : out, normalised state when the lane reaches its chunk start s (speculative pass)
//   at_e   : out, normalised state when the lane reaches its chunk end e (written only when reached)
template <int W1, typename T>
__device__ __attribute__((noinline)) void detect_pass(const ReadCtx<T> &rc, int lead, bool active, int64_t s,
                                                      int64_t e, uint32_t K, DetState st, DetState &at_s,
                                                      DetState &at_e) {
    constexpr int W2 = 2 * W1;
    const int64_t n = rc.n;
    const int64_t i_begin = s - lead;
    if (!__any(active)) return;
    DetState d = (lead > 0) ? det_fresh(i_begin <= 0 ? 0 : -1) : st;
    // bitmap register window: wcur = word of the current index, wprev = the word before it
    unsigned long long wcur = 0ull, wprev = 0ull;
    const int64_t wlo = s >> 6, whi = (e + 63) >> 6;
    bool done = !active;
    const int main_steps = lead + (int)K;
    const bool t1_ok = n >= 2 * W1, t2_ok = n >= 2 * W2;
    int j = 0;
    for (;; ++j) {
        if (j >= main_steps && !__any(!done)) break;
        const int64_t i = i_begin + j;
        if ((j & 63) == 0 && j > 0 && active) {
            // entering bitmap word (i>>6): retire the word two back
            const int64_t wr = (i >> 6) - 2;
            if (wr >= wlo && wr < whi) rc.bm[wr] = wprev;
            wprev = wcur;
            wcur = 0ull;
        }
        if (active && i >= 0) {
            if (i == s && lead > 0) at_s = det_norm(d, (int)i);
            if (i == e) at_e = det_norm(d, (int)i);
            if (i >= n) done = true;
            if (i >= e) {
                const bool pend = (d.sp >= 0 && d.sp < e) || (d.lp >= 0 && d.lp < e);
                if (!pend) done = true;
            }
            if (!done) {
                float v1 = 0.0f, v2 = 0.0f;
                if (t1_ok && i >= W1 && i <= n - W1) {
                    const double p0 = rc.P[i], q0 = rc.P2[i];
                    v1 = sgk_tstat_ref<W1>(p0 - rc.P[i - W1], q0 - rc.P2[i - W1], rc.P[i + W1] - p0,
                                           rc.P2[i + W1] - q0);
                }
                if (t2_ok && i >= W2 && i <= n - W2) {
                    const double p0 = rc.P[i], q0 = rc.P2[i];
                    v2 = sgk_tstat_ref<W2>(p0 - rc.P[i - W2], q0 - rc.P2[i - W2], rc.P[i + W2] - p0,
                                           rc.P2[i + W2] - q0);
                }
                int es, el;
                det_step<W1>(d, (int)i, v1, v2, es, el);
#pragma unroll
                for (int z = 0; z < 2; ++z) {
                    const int p = z ? el : es;
                    if (p >= s && p < e) {
                        const int64_t wi = (int64_t)p >> 6, wb = i >> 6;
                        const unsigned long long bit = 1ull << (p & 63);
                        if (wi == wb) wcur |= bit;
                        else if (wi == wb - 1) wprev |= bit;
                        else rc.bm[wi] |= bit;  // older word: already retired, owned by this lane only
                    }
                }
            }
        }
    }
    if (active) {
        // the last processed index is i_begin + j - 1; the register window holds its word and
        // the one before it
        const int64_t wb = (i_begin + (int64_t)j - 1) >> 6;
        if (wb - 1 >= wlo && wb - 1 < whi) rc.bm[wb - 1] = wprev;
        if (wb >= wlo && wb < whi) rc.bm[wb] = wcur;
    }
}

// Generic detector over one read by one wave (prefix arrays required).
template <int W1, typename T>
__device__ void detect_read(const ReadCtx<T> &rc, EvHeader *hdr) {
    const int64_t n = rc.n;
    if (n <= 0) return;
    const uint32_t K = chunk_len(n);
    const int c = lane_id();
    const int64_t s = (int64_t)c * K;
    const int64_t e = (s + K < n) ? s + K : n;
    const bool active = s < n;
    const DetState fresh = det_fresh(0);
    DetState at_s = fresh, at_e = fresh;
    detect_pass<W1, T>(rc, LEAD, active, s, e, K, fresh, at_s, at_e);
    DetState init = at_s;
    for (int iter = 0; iter < 64; ++iter) {
        const DetState pe = det_shfl_up(at_e);
        const bool bad = active && c > 0 && !det_equal(pe, init);
        const unsigned long long badmask = __ballot(bad);
        if (badmask == 0ull) break;
        if (bad) init = pe;
        DetState unused = fresh;
        detect_pass<W1, T>(rc, 0, bad, s, e, K, pe, unused, at_e);
        if (c == 0) atomicAdd(&hdr->n_rerun, (uint32_t)__popcll(badmask));
    }
}

// src/events.c:457-473 (create_event)
__device__ inline void store_event(const EvArgs &a, uint64_t slot0, uint64_t cap, uint64_t k, uint32_t ps,
                                   uint32_t pe, double dsum, double dsumsq, bool &overflow) {
    if (k >= cap) { overflow = true; return; }
    const float len = (float)(pe - ps);
    const float m = (float)dsum / len;
    const float dsq = (float)dsumsq;
    const float var = dsq / len - m * m;
    const float sd = sqrtf(fmaxf(var, 0.0f));
    sgk_event_rec_t e;
    e.start = ps;
    e.length = pe - ps;
    e.mean = m;
    e.stdv = sd;
    a.events[slot0 + k] = e;
}

// fallback builder: event sums are differences of the sequential prefix arrays, as in the reference
template <typename T>
__device__ void build_read_prefix(const EvArgs &a, const ReadCtx<T> &rc, uint32_t r) {
    const int64_t n = rc.n;
    const int l = lane_id();
    const uint64_t slot0 = a.ev_slots[r], cap = a.ev_slots[r + 1] - slot0;
    if (n <= 0) {
        if (l == 0) a.n_events[r] = 0;
        return;
    }
    const uint32_t *bm32 = reinterpret_cast<const uint32_t *>(rc.bm);
    bool overflow = false;
    uint32_t rank = 0, prevp = 0;
    const int64_t nwords = (n + 31) >> 5;
    for (int64_t w0 = 0; w0 < nwords; w0 += 64) {
        const int64_t w = w0 + l;
        const int64_t pos0 = w * 32;
        uint32_t bits = (w < nwords) ? bm32[w] : 0u;
        if (w < nwords && n - pos0 < 32) bits &= (1u << (int)(n - pos0)) - 1u;
        const int cnt = __popc(bits);
        const int incl = wave_incl_scan_i(cnt);
        const int excl = incl - cnt;
        const int total = __shfl(incl, 63, 64);
        const unsigned long long m = __ballot(cnt > 0);
        const uint32_t lastp = cnt > 0 ? (uint32_t)(pos0 + 31 - __clz((int)bits)) : 0u;
        const unsigned long long lower = m & ((1ull << l) - 1ull);
        const int src = lower ? 63 - __clzll((long long)lower) : 0;
        uint32_t pl = __shfl(lastp, src, 64);
        if (!lower) pl = prevp;
        int k = 0;
        while (bits) {
            const int b = __ffs((int)bits) - 1;
            bits &= bits - 1u;
            const uint32_t p = (uint32_t)(pos0 + b);
            store_event(a, slot0, cap, (uint64_t)rank + (uint64_t)(excl + k), pl, p, rc.P[p] - rc.P[pl],
                        rc.P2[p] - rc.P2[pl], overflow);
            pl = p;
            ++k;
        }
        if (m) {
            prevp = __shfl(lastp, 63 - __clzll((long long)m), 64);
            rank += (uint32_t)total;
        }
    }
    if (l == 0) {
        store_event(a, slot0, cap, (uint64_t)rank, prevp, (uint32_t)n, rc.P[n] - rc.P[prevp],
                    rc.P2[n] - rc.P2[prevp], overflow);
        a.n_events[r] = rank + 1;
        atomicAdd(&a.hdr->n_events_total, (unsigned long long)(rank + 1));
    }
    if (__any(overflow) && l == 0) atomicAdd(&a.hdr->n_overflow, 1u);
}

// Sequential double prefix sums, src/events.c:293-303: strictly in order.  Per 2048-sample tile the wave
// converts to pA (and float squares) in parallel into LDS; lane 0 runs the dependent chain of sums and
// lane 1 the chain of squares, writing the prefix values to LDS; then all lanes store the tile to the
// scratch arrays (coalesced) and test every addition for exactness (TwoSum residual): positions where
// the scan rounded are the "events" the repair logic needs.
constexpr int SP_TILE = 2048;
struct PrefixLds {
    float x[SP_TILE];
    float xq[SP_TILE];
    double ps[SP_TILE + 1];   // ps[0] = prefix before the tile, ps[k+1] = prefix after sample k
    double pq[SP_TILE + 1];
};
struct EventList {
    int ev[REP_MAX_EVENTS];
    int count;
};
template <typename T>
__device__ void seq_prefix(const ReadCtx<T> &rc, double *P, double *P2, PrefixLds *L, EventList *E) {
    const int l = lane_id();
    const int64_t n = rc.n;
    double acc = 0.0;
    if (l == 0) { P[0] = 0.0; P2[0] = 0.0; E->count = 0; }
    for (int64_t tb = 0; tb < n; tb += SP_TILE) {
        const int m = (n - tb) < SP_TILE ? (int)(n - tb) : SP_TILE;
        __syncthreads();
        for (int k = l; k < m; k += 64) {
            const float x = to_pa(rc.base[tb + k], rc.sc);
            L->x[k] = x;
            L->xq[k] = x * x;
        }
        __syncthreads();
        if (l < 2) {
            const float *src = (l == 0) ? L->x : L->xq;
            double *dst = (l == 0) ? L->ps : L->pq;
            dst[0] = acc;
            int k = 0;
            for (; k + 8 <= m; k += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = src[k + u];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    acc = acc + (double)v[u];
                    dst[k + u + 1] = acc;
                }
            }
            for (; k < m; ++k) {
                acc = acc + (double)src[k];
                dst[k + 1] = acc;
            }
        }
        __syncthreads();
        for (int k = l; k < m; k += 64) {
            const double s0 = L->ps[k], s1 = L->ps[k + 1], q0 = L->pq[k], q1 = L->pq[k + 1];
            P[tb + k + 1] = s1;
            P2[tb + k + 1] = q1;
            const double ys = (double)L->x[k], yq = (double)L->xq[k];
            const double bs = s1 - s0, bq = q1 - q0;
            const double es = (s0 - (s1 - bs)) + (ys - bs), eq = (q0 - (q1 - bq)) + (yq - bq);
            if (es != 0.0 || eq != 0.0) {
                const int idx = atomicAdd(&E->count, 1);
                if (idx < REP_MAX_EVENTS) E->ev[idx] = (int)(tb + k);
            }
        }
    }
    __threadfence();
    __syncthreads();
    if (l == 0) {  // sort the (few) event positions
        const int m = E->count < REP_MAX_EVENTS ? E->count : REP_MAX_EVENTS;
        for (int i = 1; i < m; ++i) {
            const int v = E->ev[i];
            int j = i - 1;
            while (j >= 0 && E->ev[j] > v) { E->ev[j + 1] = E->ev[j]; --j; }
            E->ev[j + 1] = v;
        }
    }
    __syncthreads();
}

template <int W1, typename T>
__global__ __launch_bounds__(64) void k_event_fallback(EvArgs a) {
    __shared__ PrefixLds L;
    __shared__ LzLds Lz;
    __shared__ EventList events;
    double *P = a.scratch + (uint64_t)blockIdx.x * a.scratch_stride;
    double *P2 = P + a.scratch_stride / 2;
    const uint32_t nf = a.hdr->n_flagged;
    for (;;) {
        uint32_t w = 0;
        if (lane_id() == 0) w = atomicAdd(&a.hdr->fb_next, 1u);
        w = __shfl(w, 0, 64);
        if (w >= nf) break;
        const uint32_t r = a.flag_list[w];
        ReadCtx<T> rc = make_ctx<T>(a, r);
        seq_prefix<T>(rc, P, P2, &L, &events);
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
        const int rcode = detect_read_lazy<W1, T, true>(rc, a.hdr, &Lz, &rep);
        if (rcode) detect_read<W1, T>(rc, a.hdr);
        __threadfence();
        __syncthreads();
        build_read_prefix<T>(a, rc, r);
        __syncthreads();
    }
}

int launch_k_event_fallback(int rna, bool float_input, uint32_t n_fb_blocks, hipStream_t st, const EvArgs &a) {
    if (rna && float_input) SGK_LAUNCH("k_event_fallback", (k_event_fallback<7, float>), n_fb_blocks, 64, st, a);
    else if (rna) SGK_LAUNCH("k_event_fallback", (k_event_fallback<7, int16_t>), n_fb_blocks, 64, st, a);
    else if (float_input) SGK_LAUNCH("k_event_fallback", (k_event_fallback<3, float>), n_fb_blocks, 64, st, a);
    else SGK_LAUNCH("k_event_fallback", (k_event_fallback<3, int16_t>), n_fb_blocks, 64, st, a);
    return SGK_OK;
}

}  // namespace sgk
