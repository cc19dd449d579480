// event_generic.h -- the exact generic event path on the reference's own sequentially rounded prefix arrays: the prefix
// scan (seq_prefix), the two-automaton detector stepped index by index on differences of those arrays (det_step,
// detect_pass, detect_read) and the builder on them (build_read_prefix).  Two kernels share it:
//   k_event_fallback  (event_fallback.hip)  a preset's reads the fast pass cannot take: <W1> is a template argument, the
//                                           windows and thresholds are DetParam<W1>'s constants (RT: the windows are,
//                                           the thresholds are DetVals' -- the presets' windows with the caller's
//                                           thresholds)
//   k_event_param     (event_param.hip)     caller-supplied detector parameters: <0>, everything in DetVals at run time
// The map of the event units is in event_device.h.
#pragma once
#include "event_device.h"

namespace sgk {

constexpr int LEAD = 64;   // speculative warm-up (samples) of the generic pass on a preset
// chunk length of the generic pass: 64 lanes x K samples cover the read, K a multiple of 64 (its bitmap words are
// 64-bit).  GENERIC_CHUNK_SAMPLES is the read length per step of K (sigtk_amd/api.py mirrors it for the tests).
constexpr int GENERIC_CHUNK_SAMPLES = 4096;
__device__ inline uint32_t chunk_len(int64_t n) {
    const int64_t k = (n + GENERIC_CHUNK_SAMPLES - 1) / GENERIC_CHUNK_SAMPLES;
    return (uint32_t)(k < 1 ? 64 : 64 * k);
}

// ---------------------------------------------------------------- detector parameters
// detector_param of src/events.c:35-41 as values.  With W1 > 0 (a preset) every user below takes the compile-time
// constants instead and the struct is dead; with RT as well only its windows are.
struct DetVals {
    int w1, w2;
    float thr1, thr2, ph;
};
template <int W1, bool RT = false>
__device__ __forceinline__ DetVals det_vals(const DetVals &dv) {
    if constexpr (W1 > 0) {
        DetVals p;
        p.w1 = W1;
        p.w2 = 2 * W1;
        p.thr1 = RT ? dv.thr1 : DetParam<W1>::thr1;
        p.thr2 = RT ? dv.thr2 : DetParam<W1>::thr2;
        p.ph = RT ? dv.ph : DetParam<W1>::ph;
        return p;
    } else {
        return dv;
    }
}

// the reference expression (sgk_tstat_ref<W>, tstat_math.h) with wf = (float)w at run time: one rounding per operator
__device__ inline __attribute__((noinline)) float sgk_tstat_ref_rt(float wf, double A, double A2, double B, double B2) {
    const float sum2 = (float)B;
    const float sumsq2 = (float)B2;
    const float mean1 = (float)(A / (double)wf);
    const float mean2 = sum2 / wf;
    const float m1sq = mean1 * mean1;
    const float m2sq = mean2 * mean2;
    const float q2 = sumsq2 / wf;
    double acc = A2 / (double)wf;
    acc = acc - (double)m1sq;
    acc = acc + (double)q2;
    acc = acc - (double)m2sq;
    float cv = (float)acc;
    cv = fmaxf(cv, 1.17549435e-38f);
    const float delta = mean2 - mean1;
    const float cvw = cv / wf;
    return (float)(fabs((double)delta) / sqrt((double)cvw));
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
template <int W1, bool RT = false>
__device__ inline void det_step(const DetVals &dv, DetState &d, int i, float v1, float v2, int &emit_s, int &emit_l) {
    const DetVals p = det_vals<W1, RT>(dv);
    emit_s = -1;
    emit_l = -1;
    // ---- short detector: its masked_to stays 0, so only index 0 is skipped (events.c:387)
    if (i > 0) {
        if (d.sp < 0) {
            if (v1 < d.sv) {
                d.sv = v1;
            } else if (v1 - d.sv > p.ph) {
                d.sv = v1;
                d.sp = i;
            }
        } else {
            if (v1 > d.sv) {
                d.sv = v1;
                d.sp = i;
            }
            if (d.sv > p.thr1) {  // dominate the long detector (events.c:414-422)
                d.lmask = d.sp + p.w1;
                d.lp = -1;
                d.lv = FLT_MAX;
                d.lvalid = 0;
            }
            if (d.sv - v1 > p.ph && d.sv > p.thr1) d.svalid = 1;
            if (d.svalid && (i - d.sp) > p.w1 / 2) {
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
            } else if (v2 - d.lv > p.ph) {
                d.lv = v2;
                d.lp = i;
            }
        } else {
            if (v2 > d.lv) {
                d.lv = v2;
                d.lp = i;
            }
            if (d.lv - v2 > p.ph && d.lv > p.thr2) d.lvalid = 1;
            if (d.lvalid && (i - d.lp) > p.w2 / 2) {
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
// library division and sqrt).
//   lead   : samples each lane starts before its chunk start (> 0: speculative pass, 0: re-run); any value >= 0 --
//            the result of detect_read does not depend on it, only the number of re-runs does
//   active : whether this lane runs in this pass
//   st     : state at the pass start (lead == 0 only; the speculative pass starts fresh)
//   at_s   : out, normalised state when the lane reaches its chunk start s (speculative pass)
//   at_e   : out, normalised state when the lane reaches its chunk end e (written only when reached)
template <int W1, typename T, bool RT = false>
__device__ __attribute__((noinline)) void detect_pass(const ReadCtx<T> &rc, const DetVals &dv, int lead, bool active,
                                                      int64_t s, int64_t e, uint32_t K, DetState st, DetState &at_s,
                                                      DetState &at_e) {
    const DetVals p = det_vals<W1, RT>(dv);
    const int w1 = p.w1, w2 = p.w2;
    const int64_t n = rc.n;
    const int64_t i_begin = s - lead;
    if (!__any(active)) return;
    DetState d = (lead > 0) ? det_fresh(i_begin <= 0 ? 0 : -1) : st;
    // bitmap register window: wcur = word of the current index, wprev = the word before it
    unsigned long long wcur = 0ull, wprev = 0ull;
    const int64_t wlo = s >> 6, whi = (e + 63) >> 6;
    bool done = !active;
    const int main_steps = lead + (int)K;
    const bool t1_ok = n >= 2 * (int64_t)w1, t2_ok = n >= 2 * (int64_t)w2;
    [[maybe_unused]] const float wf1 = (float)w1, wf2 = (float)w2;
    int j = 0;
    for (;; ++j) {
        if (j >= main_steps && !__any(!done)) break;
        const int64_t i = i_begin + j;
        if ((i & 63) == 0 && j > 0 && active) {
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
                if (t1_ok && i >= w1 && i <= n - w1) {
                    const double p0 = rc.P[i], q0 = rc.P2[i];
                    const double A = p0 - rc.P[i - w1], A2 = q0 - rc.P2[i - w1];
                    const double B = rc.P[i + w1] - p0, B2 = rc.P2[i + w1] - q0;
                    if constexpr (W1 > 0) v1 = sgk_tstat_ref<W1>(A, A2, B, B2);
                    else v1 = sgk_tstat_ref_rt(wf1, A, A2, B, B2);
                }
                if (t2_ok && i >= w2 && i <= n - w2) {
                    const double p0 = rc.P[i], q0 = rc.P2[i];
                    const double A = p0 - rc.P[i - w2], A2 = q0 - rc.P2[i - w2];
                    const double B = rc.P[i + w2] - p0, B2 = rc.P2[i + w2] - q0;
                    if constexpr (W1 > 0) v2 = sgk_tstat_ref<2 * W1>(A, A2, B, B2);
                    else v2 = sgk_tstat_ref_rt(wf2, A, A2, B, B2);
                }
                int es, el;
                det_step<W1, RT>(dv, d, (int)i, v1, v2, es, el);
#pragma unroll
                for (int z = 0; z < 2; ++z) {
                    const int pk = z ? el : es;
                    if (pk >= s && pk < e) {
                        const int64_t wi = (int64_t)pk >> 6, wb = i >> 6;
                        const unsigned long long bit = 1ull << (pk & 63);
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

// Generic detector over one read by one wave (prefix arrays required).  Lane 0 starts from the true state, so after
// the speculative pass its end state is final; every iteration of the loop below makes at least the first lane whose
// start state was wrong final.  63 iterations therefore always reach the sequential result whatever `lead` is; the loop
// allows 64.
template <int W1, typename T, bool RT = false>
__device__ void detect_read(const ReadCtx<T> &rc, const DetVals &dv, int lead, EvHeader *hdr) {
    const int64_t n = rc.n;
    if (n <= 0) return;
    const uint32_t K = chunk_len(n);
    const int c = lane_id();
    const int64_t s = (int64_t)c * K;
    const int64_t e = (s + K < n) ? s + K : n;
    const bool active = s < n;
    const DetState fresh = det_fresh(0);
    DetState at_s = fresh, at_e = fresh;
    detect_pass<W1, T, RT>(rc, dv, lead, active, s, e, K, fresh, at_s, at_e);
    DetState init = at_s;
    for (int iter = 0; iter < 64; ++iter) {
        const DetState pe = det_shfl_up(at_e);
        const bool bad = active && c > 0 && !det_equal(pe, init);
        const unsigned long long badmask = __ballot(bad);
        if (badmask == 0ull) break;
        if (bad) init = pe;
        DetState unused = fresh;
        detect_pass<W1, T, RT>(rc, dv, 0, bad, s, e, K, pe, unused, at_e);
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

// builder on the prefix arrays: event sums are differences of the sequential prefix arrays, as in the reference
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

// Sequential double prefix sums, src/events.c:293-303: strictly in order.  Per TILE-sample tile the wave
// converts to pA (and float squares) in parallel into LDS; lane 0 runs the dependent chain of sums and
// lane 1 the chain of squares, writing the prefix values to LDS; then all lanes store the tile to the
// scratch arrays (coalesced) and, when the caller wants them (E != null), test every addition for exactness
// (TwoSum residual): positions where the scan rounded are the "events" the fallback's repair logic needs.
// The tile only sets how much LDS a workgroup holds (24 bytes per sample), not the result: k_event_fallback keeps
// 2048 beside its detector's LDS, k_event_param takes 512 so that LDS does not bound its waves per CU.
constexpr int SP_TILE = 2048;
template <int TILE>
struct PrefixLdsT {
    float x[TILE];
    float xq[TILE];
    double ps[TILE + 1];   // ps[0] = prefix before the tile, ps[k+1] = prefix after sample k
    double pq[TILE + 1];
};
using PrefixLds = PrefixLdsT<SP_TILE>;
template <int CAP>
struct EventListT {
    int ev[CAP];
    int count;
};
template <typename T, int CAP, int TILE>
__device__ void seq_prefix(const ReadCtx<T> &rc, double *P, double *P2, PrefixLdsT<TILE> *L, EventListT<CAP> *E) {
    const int l = lane_id();
    const int64_t n = rc.n;
    double acc = 0.0;
    if (l == 0) {
        P[0] = 0.0;
        P2[0] = 0.0;
        if (E) E->count = 0;
    }
    for (int64_t tb = 0; tb < n; tb += TILE) {
        const int m = (n - tb) < TILE ? (int)(n - tb) : TILE;
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
            if (E) {
                const double ys = (double)L->x[k], yq = (double)L->xq[k];
                const double bs = s1 - s0, bq = q1 - q0;
                const double es = (s0 - (s1 - bs)) + (ys - bs), eq = (q0 - (q1 - bq)) + (yq - bq);
                if (es != 0.0 || eq != 0.0) {
                    const int idx = atomicAdd(&E->count, 1);
                    if (idx < CAP) E->ev[idx] = (int)(tb + k);
                }
            }
        }
    }
    __threadfence();
    __syncthreads();
    if (E) {
        if (l == 0) {  // sort the (few) event positions
            const int m = E->count < CAP ? E->count : CAP;
            for (int i = 1; i < m; ++i) {
                const int v = E->ev[i];
                int j = i - 1;
                while (j >= 0 && E->ev[j] > v) { E->ev[j + 1] = E->ev[j]; --j; }
                E->ev[j + 1] = v;
            }
        }
        __syncthreads();
    }
}

}  // namespace sgk
