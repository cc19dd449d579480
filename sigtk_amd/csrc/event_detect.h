// event_detect.h -- the lazy detector of the `event` path: one wave over a span of a read (or, MULTI, over several
// short reads), samples -> peak bitmap.  The map of the event units is in event_device.h.
#pragma once
#include <utility>

#include "event_device.h"

namespace sgk {

// ================================================================ fast detector pass (round 2: "LazyPass")
// Same semantics as detect_pass, restructured around what the instruction stream costs on gfx950
// (tools/valu_rate.hip, profiles/archive/r02_valu_rate.txt: plain f32 add/mul/fma, logic and int add issue in 2.3 cycles per
// wave64 instruction; everything f64, conversions, v_cmp, v_cndmask, v_max/min and packed f32 take 4.45):
//  * window sums are differences of a RUNNING double prefix sum kept in a register ring (P(i) .. P(i+W2+1)): one
//    conversion and one addition per sample for the sums and for the float squares, one subtraction per window;
//    exact under the read-level guard, like every sum of this path;
//  * the A side of a t-statistic (mean1, sumsq1/w - mean1^2) is what the B side's window sum yields W indices later:
//    it is evaluated once per window position and ringed (SgkARole), not re-derived from sums;
//  * the tail |delta| / sqrt(cv/w) is evaluated in f32 with error-free transformations and certified
//    (sgk_tail_f32); uncertified evaluations (2^-12) are redone with the reference expression;
//  * the SHORT detector (events.c:383-440, k = 0) runs on every index, written as lane-mask algebra: the
//    comparisons produce wave masks (scalar registers), the boolean state (in a peak / valid / strong) lives in
//    masks, only peak_value and peak_pos are selected in vector registers;
//  * the LONG detector (k = 1) is LAZY.  It is reset whenever the short detector sits in a strong peak
//    (events.c:414-422) and can only emit if, since that reset, some t-statistic it saw exceeded thr2.  Per index
//    the kernel proves from cheap f32 estimates that the long window's statistic cannot exceed thr2
//    (sgk_long_cold); a run (reset .. next reset) in which the proof fails is recorded (2e-4 of the indices on
//    nanopore data) and re-played with exact arithmetic after the pass (replay_long_runs);
//  * emitted peaks go to a per-lane 512-position bitmap ring in LDS and leave as whole words.
// Positions inside a pass are BLOCK-relative (the 16-step unrolled block's first index = 0), so every position the
// automaton writes is an inline constant; they are rebased once per block.
template <int W1>
struct LzCfg {
    static constexpr int W2 = 2 * W1;
    static constexpr int R = 16;                    // unroll (multiple of every ring length)
    static constexpr int NP = (W1 == 3) ? 8 : 16;   // prefix ring >= W2 + 2
    static constexpr int NA = (W1 == 3) ? 4 : 8;    // short A-side ring >= W1
    static constexpr int NL = (W1 == 3) ? 8 : 16;   // long side ring >= W2
    static constexpr int H1 = W1 / 2;
};
static_assert(LzCfg<3>::NP >= 8 && LzCfg<7>::NP >= 16, "prefix ring holds P(i) .. P(i+W2+1)");

// Which kernels take the leading-edge form of the fast pass (LazyPass<.., LEAD>), as bits: 1 k_event<3, *> (shipped),
// 2 k_event<7, *>, 4 k_event_multi<3, *>.  The others are switches for listings and A/B builds (tools/build_variant.sh
// <tag> -DSGK_EVENT_LEAD=<bits>; 0: the trailing form everywhere); profiles/event_leading_window.md has what they showed.
#ifndef SGK_EVENT_LEAD
#define SGK_EVENT_LEAD 1
#endif

// Which passes keep the lazy long detector's bookkeeping as a mask history (LazyPass::BOOK, below), as bits: 1 the passes
// on the leading-edge form (k_event<3, *>, shipped), 2 the other unflagged passes (k_event<7, *>, k_event_multi,
// k_event_seg), 4 the fallback's.  0 is the form with lm / r0 in vector registers and a compare per index
// (tools/build_variant.sh <tag> -DSGK_EVENT_BOOK=0); profiles/event_bookkeeping.md has the listings.
#ifndef SGK_EVENT_BOOK
#define SGK_EVENT_BOOK 1
#endif

// How the fast pass of k_event<3, *> (the leading-edge form with the mask history: LEAD and BOOK) keeps the emission's
// bookkeeping, as bits (tools/build_variant.sh <tag> -DSGK_EVENT_EMIT=<bits>; 0: a bit selected and ORed into the bitmap
// word and two rare tests per index); profiles/event_emission.md has the listings and what each part showed.
//   1  the bitmap word is built in REVERSED order, bw = bw + bw + carry(em): the emission mask is the carry-in of one
//      v_addc_co_u32 per index, and the word is bit-reversed once per 32 positions where it leaves for the ring
//   2  one test per index, (rare emission | recorded run) != 0, marked unlikely, with both rare blocks behind it
#ifndef SGK_EVENT_EMIT
#define SGK_EVENT_EMIT 3
#endif

constexpr int LZ_NONE = -(1 << 29);   // "no mask" / far in the past (block-relative positions drift by -16 per block)
constexpr int LZ_NREC = 8;            // hot long-detector runs a lane can record per pass (more: read -> exact fallback)
constexpr int LZ_RING_WORDS = 16;     // per-lane bitmap ring: 512 positions

// detector state at a block boundary: LzSnapState (event_args.h), what chunks hand over / compare
struct LzSnap {
    LzSnapState init[64];  // state a chunk's accepted run started from (at its chunk start)
    LzSnapState at_e[64];  // state at the chunk end
    LzSnapState st0[64];   // start state handed to a re-run
};
__device__ inline bool lz_equal(const LzSnapState &a, const LzSnapState &b) {
    return a.sp == b.sp && __float_as_int(a.sv) == __float_as_int(b.sv) && a.lm == b.lm && a.r0 == b.r0 &&
           a.bits == b.bits;
}
struct LzLds {
    uint32_t ring[64][LZ_RING_WORDS + 1];  // + one word: the lane's inherited emission (LZ_PRE, below)
    LzSnap snap;
    LzRun runs[64][LZ_NREC];
    int nrec[64];
};

// Exact (reference-expression) t-statistic at index i of a read, window sums formed directly from
// the samples in global memory.  Out of line: only reached when a fast evaluation's certificate
// fails (about 2^-12 of the evaluations) and in the long detector's replay.
template <typename T>
__device__ __attribute__((noinline)) float tstat_exact_at(const T *base, Scale sc, int i, int w) {
    double A = 0.0, A2 = 0.0, B = 0.0, B2 = 0.0;
    for (int k = 0; k < w; ++k) {
        const float xa = to_pa(base[i - w + k], sc);
        const float xb = to_pa(base[i + k], sc);
        A = A + (double)xa;
        A2 = A2 + (double)(xa * xa);
        B = B + (double)xb;
        B2 = B2 + (double)(xb * xb);
    }
    if (w == 3) return sgk_tstat_ref<3>(A, A2, B, B2);
    if (w == 6) return sgk_tstat_ref<6>(A, A2, B, B2);
    if (w == 7) return sgk_tstat_ref<7>(A, A2, B, B2);
    return sgk_tstat_ref<14>(A, A2, B, B2);
}

// 16 consecutive samples starting at an even sample offset, as they sit in memory.
template <typename T>
struct Lead16;
template <>
struct Lead16<int16_t> {
    uint32_t w[8];
    template <int U>
    __device__ __forceinline__ float get(const Scale &sc) const {
        const int v = (U & 1) ? ((int)w[U / 2] >> 16) : (int)(short)(w[U / 2] & 0xffffu);
        const float shifted = (float)v + sc.offf;
        return shifted * sc.unit;
    }
};
template <>
struct Lead16<float> {
    float w[16];
    template <int U>
    __device__ __forceinline__ float get(const Scale &) const { return w[U]; }
};
typedef uint32_t sgk_u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// Samples in front of a read (the speculative warm-up of its first chunks reaches there) are whatever the caller's
// buffer holds.  No t-statistic that sees them is used, but they pass through the RUNNING prefix sums, and a value
// far larger than the read's own samples (a neighbour scaled with this read's offset/range) would leave a rounding
// residue in those double sums for the rest of the chunk.  Every position before the read therefore takes the
// value of the read's first sample: inside the magnitude range the exactness guard checks.  Rare (first lanes of a
// read, first blocks only), kept out of line.
template <typename T>
__device__ __attribute__((noinline)) Lead16<T> lead_fix_head(Lead16<T> g, int pos, T first) {
    T tmp[16];
    __builtin_memcpy(tmp, g.w, sizeof(tmp));
#pragma unroll
    for (int k = 0; k < 16; ++k) tmp[k] = (pos + k < 0) ? first : tmp[k];
    __builtin_memcpy(g.w, tmp, sizeof(tmp));
    return g;
}

// ---- repair context of a read that failed the exactness guard (fallback kernel only) ----------
// The reference's window sums are differences of its sequentially rounded prefix arrays.  They equal
// the exact sums the fast pass forms EXCEPT where an inexact addition of the sequential scan ("event"
// at sample t: prefix[t+1] != prefix[t] + y_t exactly) lies inside the window, i.e. for the indices
// i in [t-w+1, t+w].  The fast pass therefore runs unchanged on such reads and only those indices
// (plus uncertified evaluations) are re-evaluated from the scratch prefix arrays; for the long window they
// count as "hot" (the run is re-played from the prefix arrays).
constexpr int REP_MAX_EVENTS = 32;
struct RepairCtx {
    const double *P, *P2;   // reference prefix arrays (n+1 entries each)
    const int *ev;          // sorted event positions (LDS)
    int nev;
    bool all_dirty;         // more events than REP_MAX_EVENTS: every index is evaluated from the prefix arrays
};

__device__ __attribute__((noinline)) float tstat_prefix_at(const double *P, const double *P2, int i, int w) {
    const double p0 = P[i], q0 = P2[i];
    const double A = p0 - P[i - w], A2 = q0 - P2[i - w], B = P[i + w] - p0, B2 = P2[i + w] - q0;
    if (w == 3) return sgk_tstat_ref<3>(A, A2, B, B2);
    if (w == 6) return sgk_tstat_ref<6>(A, A2, B, B2);
    if (w == 7) return sgk_tstat_ref<7>(A, A2, B, B2);
    return sgk_tstat_ref<14>(A, A2, B, B2);
}

// marks (as "redo exactly" / "hot") the indices q0..q0+3 that lie within a window length of an event
template <int W1>
__device__ __forceinline__ void repair_mark(const RepairCtx &rep, int &next_t, int q0, unsigned cnt1, unsigned cnt2,
                                            unsigned &bad1, unsigned &bad2) {
    constexpr int W2 = 2 * W1;
    if (rep.all_dirty) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if ((unsigned)(q0 + u - W1) < cnt1) bad1 |= 1u << u;
            if ((unsigned)(q0 + u - W2) < cnt2) bad2 |= 1u << u;
        }
        return;
    }
    if (next_t > q0 + 3 + W2 - 1) return;  // no event can reach this quad (the usual case)
    int nt = 0x7fffffff;
    for (int k = 0; k < rep.nev; ++k) {
        const int t = rep.ev[k];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = q0 + u;
            if ((unsigned)(i - t + W1 - 1) < (unsigned)(2 * W1) && (unsigned)(i - W1) < cnt1) bad1 |= 1u << u;
            if ((unsigned)(i - t + W2 - 1) < (unsigned)(2 * W2) && (unsigned)(i - W2) < cnt2) bad2 |= 1u << u;
        }
        if (t + W2 >= q0 + 4 && t < nt) nt = t;  // may still reach a later quad
    }
    next_t = nt;
}

// out of line (rare): a peak whose bitmap word may have left the lane's ring, or that lies in front of the lane's own
// range [s, e).  A lane stops at e even if a peak is still pending there: the lane behind starts (verified) from the
// same state and emits it -- a peak that lies in front of its own range.  If that happens inside its range (cur >=
// own_lo), the lane INHERITED the peak with its start state and leaves the position in its ring's extra word (LZ_PRE):
// detect_span sets the bit once the lane's start state is known to be the true one.  (At most one per pass: after the
// emission every peak position lies inside the range.)  If it happens during the warm-up, the owner has emitted it.
// (Round 2 let the OWNER run on until its pending peak was emitted; on a flat signal that is never, and every pass of
// every lane walked to the end of the read: 5 s for a constant read of 75 000 samples.)
constexpr int LZ_PRE = LZ_RING_WORDS;
__device__ __attribute__((noinline)) void lz_emit_slow(uint32_t *ring, unsigned long long *bm, int flushed,
                                                       int i_begin, int s, int e, int p, int cur) {
    const int own_lo = s - i_begin;
    if (p < own_lo) {
        if (cur >= own_lo) ring[LZ_PRE] = (uint32_t)(i_begin + p);
        return;
    }
    if (p >= flushed) {
        atomicOr(&ring[(p >> 5) & (LZ_RING_WORDS - 1)], 1u << (p & 31));
    } else {
        const int pa = i_begin + p;
        if (pa >= s && pa < e) atomicOr(reinterpret_cast<uint32_t *>(bm) + (pa >> 5), 1u << (pa & 31));
    }
}
// out of line (rare): a hot long-detector run [a, b) ended at the reset of index b (or at the read's end, b = n); the
// lane whose chunk holds index b (for b = n: index n-1) replays it.  Lane c+1 meets the reset at its first index
// with the state it shares with lane c, so exactly one lane records every run.
__device__ __attribute__((noinline)) int lz_record(LzRun *runs, int nrec, int a, int b, int s, int e, int n) {
    if ((b >= s && b < e) || (b == n && e == n && s < n)) {
        if (nrec < LZ_NREC) {
            runs[nrec].a = a;
            runs[nrec].b = b;
        }
        ++nrec;
    }
    return nrec;
}

// out of line (rare): the uncertified t-statistics of a quad, redone with the reference expression
struct Redo4 {
    float v[4];
};
template <int W1, typename T, bool FLAGGED>
__device__ __attribute__((noinline)) Redo4 redo_quad(const T *base, Scale sc, const double *P, const double *P2, int i0,
                                                     unsigned cnt1, unsigned bits, float t0, float t1, float t2,
                                                     float t3) {
    Redo4 r;
    r.v[0] = t0; r.v[1] = t1; r.v[2] = t2; r.v[3] = t3;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if ((bits >> k) & 1u) {
            const int i = i0 + k;
            float v = 0.0f;
            if ((unsigned)(i - W1) < cnt1) {
                if constexpr (FLAGGED) v = tstat_prefix_at(P, P2, i, W1);
                else v = tstat_exact_at<T>(base, sc, i, W1);
            }
            r.v[k] = v;
        }
    }
    return r;
}

typedef unsigned long long lmask_t;  // one bit per lane: lives in a scalar register pair, combined on the scalar unit
// mask -> per-lane predicate without vector work: selects become v_cndmask with the mask as its condition operand,
// branches become s_and_saveexec
__device__ __forceinline__ bool lane_of(lmask_t m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
// w + w + (the lane's bit of c): a lane mask shifted into a word as the carry-in of one add (the carry-out is dropped)
__device__ __forceinline__ uint32_t shift_in(uint32_t w, lmask_t c) {
    lmask_t co;
    asm("v_addc_co_u32_e64 %0, %1, %0, %0, %2" : "+v"(w), "=s"(co) : "s"(c));
    return w;
}

// State of one fast pass.  Every ring access uses a compile-time index (U is a template parameter and the pass
// starts on a multiple of the unroll length), so the rings live in registers; the 16 steps of one loop iteration
// are expanded with fold expressions, four at a time: t-statistics of 4 indices -> (rare, rolled, out of line)
// exact redo of uncertified ones -> the automaton on those 4 indices.
//
// Samples are NOT staged through LDS: each lane loads the 16 leading samples of the next block (x[i+W2], 32 bytes)
// straight from global memory one block ahead.  A wave touches 64 different 128-byte lines per load instruction;
// each line is consumed over 4 consecutive blocks and stays in L2 meanwhile, so HBM traffic remains one pass over
// the samples and there are no barriers or cooperative loads in the loop.
//
// LEAD (a template choice: k_event<3, *> takes it; it costs the other kernels registers they do not have): the short
// window is formed at the LEADING edge.  Step i forms the sums of window position p = i + W1, c = P(i+W2) - P(i+W1):
// their floats go into a ring (ss / sqs) and are the B side of index p, W1 steps later; the A side made of c goes into
// the A ring, twice as deep, and is the A side of index p + W1.  The long window of index i is the short windows i
// and i + W1: its estimates come from their four floats (sgk_lside_halves) -- two f64 subtractions and two conversions
// per index less than with b2 = P(i+W2) - P(i), and P(i) .. P(i+W1-1) need not stay in the prefix ring.  Every sum is
// exact and every float the same RN32 of it, so the short statistic is bit for bit what the trailing form computes.
template <int W1, typename T, bool FLAGGED, bool LEAD = false, bool RT = false>
struct LazyPass {
    static_assert(!(LEAD && FLAGGED), "the fallback keeps its domain checks and TwoSum form");
    using C = LzCfg<W1>;
    static constexpr int W2 = C::W2, R = C::R, NP = C::NP, NA = C::NA, NL = C::NL, H1 = C::H1;
    static constexpr int NA2 = LEAD ? 2 * NA : NA;   // LEAD: an A side waits 2 * W1 steps for its index
    static constexpr int NS = LEAD ? NA : 1;         // LEAD: ring of the short windows' f32 sums, > W1
    static_assert(NA2 > (LEAD ? 2 : 1) * W1 && (!LEAD || NS > W1) && R % NA2 == 0, "ring depths");
    // BOOK: the long detector's mask as a history of lane masks, its run start as one register (see moff / rs)
    static constexpr bool BOOK = ((SGK_EVENT_BOOK) & (FLAGGED ? 4 : (LEAD ? 1 : 2))) != 0;
    // EMIT: SGK_EVENT_EMIT, for the one pass it is written for
    static constexpr int EMIT = (LEAD && BOOK && W1 == 3) ? (SGK_EVENT_EMIT) : 0;
    static constexpr int NM = W1 - H1;   // an emission masks the long detector at its own index and at the NM - 1 behind it
    // rings
    double Ps[NP], Pq[NP];        // running prefix sums of x and of fl(x*x); slot of P(k) = k mod NP
    SgkARole ar[NA2];             // short A side of window position p at slot p mod NA2
    float ss[NS], sqs[NS];        // LEAD: RN32 of the short window sums of position p at slot p mod NS
    SgkLSide ls[NL];              // long-window estimates of window position p at slot p mod NL
    float t1[4];                  // t-statistics of the current quad
    lmask_t nk[4];                // lanes whose t-statistic of the quad's k-th index is not certified
    lmask_t hc[4];                // lanes whose long window may exceed thr2 at the quad's k-th index
    Lead16<T> cur;                // x[ib + W2 .. ib + W2 + 16)
    // short detector (block-relative positions); boolean state as lane masks
    float sv;
    int sp;
    lmask_t inpk, val, strong;
    lmask_t hist[H1 + 1];           // hist[k]: lanes whose peak_pos was set k+1 indices ago
    uint32_t bw;                  // bitmap word (32 positions) that holds position j - H1 - 1, the usual emitted peak
                                  // (EMIT & 1: the emissions of the last 32 indices, the latest in bit 0 -- the word of
                                  // the span in reversed order, right-aligned)
    // lazy long detector
    int lm, r0;                   // short peak position at the last reset (masked while i <= lm + W1); last reset
    // BOOK, instead of lm and r0.  An emission is the last reset of its peak and masks the long detector up to
    // peak_pos + W1.  The usual emission's peak lies exactly H1 + 1 indices back: it masks this index and the next
    // NM - 1, the same in every lane, so "masked" is a short history of emission masks on the scalar unit and the first
    // index behind reset and mask is the constant u + NM.  The rare emission (an older peak) sits behind a branch and
    // forms both from sp there; its mask ends at least one index earlier.
    lmask_t moff[NM - 1];         // moff[k]: lanes an earlier emission masks at the k-th index from the current one
    int rs;                       // max(r0, lm + W1 + 1): where the long detector's current run starts (block-relative)
    lmask_t hot;
    int nrec;
    // geometry
    uint32_t *ring;               // this lane's bitmap ring in LDS
    LzRun *runs;
    const T *base;
    int lo, hi;                   // legal read-relative load range
    Scale sc;
    int n, s, e, i_begin, ib, jb, flushed;
    unsigned cnt1, cnt2;
    lmask_t done;                 // lanes that have nothing left to do (past their chunk, no pending peak)
    bool slow;                    // wave-uniform: this block takes the predicated steps (read's ends, very old peak)
    bool oldpeak;                 // wave-uniform: some lane's peak may lie outside the bitmap ring
    unsigned long long *bm;       // read's bitmap (global)
    RepairCtx rep;                // FLAGGED only
    int next_t;                   // FLAGGED only
    [[no_unique_address]] Det<W1, RT> dt;   // the thresholds: the preset's constants (empty) or three wave-uniform floats
    int dirty;                    // FLAGGED only: block-relative index up to which this lane's own window sums are
                                  // not trusted (an addition of ITS running prefix was inexact, see tstep)

    // Unconditional 32-byte load of x[pos .. pos+16).  Positions outside the readable range are redirected to the
    // nearest readable group: whatever value a position yields is used consistently (it enters the prefix sum once),
    // and no t-statistic whose window reaches outside [0, n) is ever used (events.c:332-338).  Positions before the
    // read are replaced by the read's first sample (lead_fix_head).
    __device__ __forceinline__ void load_lead(Lead16<T> &dst, int pos) const {
        int p = pos > hi - 16 ? hi - 16 : pos;
        p = p < lo ? lo : p;
        constexpr int NV = 16 * (int)sizeof(T) / 16;
        const sgk_u32x4_a4 *src = reinterpret_cast<const sgk_u32x4_a4 *>(base + p);
        sgk_u32x4_a4 v[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = src[k];
        __builtin_memcpy(dst.w, v, sizeof(dst.w));
        if (pos < 0) dst = lead_fix_head<T>(dst, pos, base[0]);
    }

    // phase 1 of index ib+U: advance the prefix ring, form the window sums, the short window's t-statistic and the
    // long window's bound.  No predicates: what a block near the read's ends needs is patched per quad (slow_fix).
    template <int U>
    __device__ __forceinline__ void tstep() {
        const float xn = cur.template get<U>(sc);  // x[i + W2]
        const float xqn = xn * xn;
        // P(i+W2+1) = P(i+W2) + x[i+W2]; it replaces P(i-1)
        Ps[(U + W2 + 1) % NP] = Ps[(U + W2) % NP] + (double)xn;
        Pq[(U + W2 + 1) % NP] = Pq[(U + W2) % NP] + (double)xqn;
        if constexpr (LEAD) {
            // the short window at position p = i + W1
            const double c = Ps[(U + W2) % NP] - Ps[(U + W1) % NP], cq = Pq[(U + W2) % NP] - Pq[(U + W1) % NP];
            const float s_p = (float)c, sq_p = (float)cq;
            const float s_i = ss[U % NS], sq_i = sqs[U % NS];  // ... and at position i, formed W1 steps ago
            ss[(U + W1) % NS] = s_p;
            sqs[(U + W1) % NS] = sq_p;
            bool cv_ok, tail_ok;
            t1[U & 3] = sgk_tstat_try_ab<W1>(s_i, sq_i, ar[(U + NA2 - W1) % NA2], cv_ok, tail_ok);
            nk[U & 3] = ~(__ballot(cv_ok) & __ballot(tail_ok));
            ar[(U + W1) % NA2] = sgk_arole<W1, true>(c, cq);
            const SgkLSide lb = sgk_lside_halves<W2>(s_i, sq_i, s_p, sq_p);  // long window at position i: bound only
            hc[U & 3] = ~__ballot(sgk_long_cold<W2>(ls[(U + NL - W2) % NL], lb));
            ls[U % NL] = lb;
            return;
        }
        const double p0 = Ps[U % NP], q0 = Pq[U % NP];
        const double b1 = Ps[(U + W1) % NP] - p0, b1q = Pq[(U + W1) % NP] - q0;
        const double b2 = Ps[(U + W2) % NP] - p0, b2q = Pq[(U + W2) % NP] - q0;
        // short window: its A side was ringed W1 indices ago
        const SgkLSide lb = sgk_lside<W2>(b2, b2q);  // long window: bound only
        if constexpr (!FLAGGED) {
            // the certificate's two conditions are combined as lane masks, on the scalar unit (see sgk_tstat_try_ab)
            bool cv_ok, tail_ok;
            t1[U & 3] = sgk_tstat_try_ab<W1>(b1, b1q, ar[(U + NA - W1) % NA], cv_ok, tail_ok);
            nk[U & 3] = ~(__ballot(cv_ok) & __ballot(tail_ok));
            ar[U % NA] = sgk_arole<W1, true>(b1, b1q);
            hc[U & 3] = ~__ballot(sgk_long_cold<W2>(ls[(U + NL - W2) % NL], lb));
            ls[U % NL] = lb;
        } else {
            // (the fallback kernel keeps its conditions as bools: as masks they cost it registers and spills)
            bool ok;
            const float v = sgk_tstat_try_ab<W1>(b1, b1q, ar[(U + NA - W1) % NA], ok);
            ok = ok && sgk_try_domain<W1>(b1, b1q, ar[(U + NA - W1) % NA]);
            // A flagged read failed the magnitude guard: the lane's running prefix can round as well, and not where
            // the reference's sequential scan did (other origin, other magnitudes), so `rep` does not list those
            // places.  TwoSum residual of the two additions above; after an inexact one the window sums of the next
            // 2 * W2 indices (every window with x[i + W2] inside) are taken from the reference's prefix arrays.
            // (Found by the soak: a 2e-5 pA sample 22 indices in front of a plateau of two equal statistics.)
            const double a_s = Ps[(U + W2) % NP], b_s = (double)xn, r_s = Ps[(U + W2 + 1) % NP];
            const double a_q = Pq[(U + W2) % NP], b_q = (double)xqn, r_q = Pq[(U + W2 + 1) % NP];
            const double t_s = r_s - a_s, t_q = r_q - a_q;
            const double e_s = (a_s - (r_s - t_s)) + (b_s - t_s), e_q = (a_q - (r_q - t_q)) + (b_q - t_q);
            const bool clean = U > dirty;
            if (e_s != 0.0 || e_q != 0.0) dirty = dirty > U + 2 * W2 ? dirty : U + 2 * W2;
            ok = ok && clean;
            ar[U % NA] = sgk_arole<W1, false>(b1, b1q);
            bool cold = sgk_long_cold<W2>(ls[(U + NL - W2) % NL], lb);
            cold = cold && clean && sgk_lside_domain(ls[(U + NL - W2) % NL]) && sgk_lside_domain(lb);
            ls[U % NL] = lb;
            t1[U & 3] = v;
            nk[U & 3] = ~__ballot(ok);
            hc[U & 3] = ~__ballot(cold);
        }
    }

    // One step of the short detector (events.c:383-440, k = 0) and of the lazy long detector's bookkeeping, on lane
    // masks.  u: block-relative index (an inline constant in the fast form); live: lanes that take the step.
    template <bool SLOW>
    __device__ __forceinline__ void dstep_core(const int u, const float v, const lmask_t hck, const lmask_t live) {
        const float ph = dt.ph(), thr1 = dt.thr1();
        const float d1 = v - sv;
        const float ee = lane_of(inpk) ? d1 : -d1;   // in a peak: v - peak_value; before one: peak_value - v
        lmask_t P = __ballot(ee > 0.0f);             // v > peak_value (in a peak) / v < peak_value (before one)
        lmask_t Q = __ballot(ee < -ph);              // peak_value - v > ph (in a peak) / v - peak_value > ph
        const lmask_t Tt = __ballot(v > thr1);
        if constexpr (SLOW) {
            P &= live;
            Q &= live;
        }
        const lmask_t ent = Q & ~inpk;                      // a peak starts here: peak_pos = i
        const lmask_t pos = (inpk & P) | ent;               // peak_pos = i
        strong = (pos & Tt) | (strong & ~pos);              // peak_value > threshold
        lmask_t dom = inpk & strong;                        // events.c:414-422: the short detector dominates the long one
        if constexpr (SLOW) dom &= live;
        val = inpk & (val | (Q & strong));
        // (i - peak_pos) > w/2  <=>  peak_pos was not set during the last w/2 indices (nor at this one: ~P)
        lmask_t recent = hist[0];
#pragma unroll
        for (int k = 1; k < H1; ++k) recent |= hist[k];
        lmask_t em = val & ~P & ~recent;
        if constexpr (SLOW) em &= live;
        const lmask_t upd = P | ent | em;
        // Emission.  A strong peak stays strong and in a peak until it is emitted, so the emission step is the LAST
        // step at which this peak resets the long detector: masked_to and the reset index are taken here.
        // the usual emitted peak was set exactly H1+1 indices ago: its position is the same in every lane, and so
        // is its bit in the lane's current bitmap word
        const uint32_t bit = 1u << ((jb + u - H1 - 1) & 31);
        // BOOK: lanes whose long detector is masked at this index (off) and at the following ones (nx), see moff
        lmask_t off = 0ull, nx[NM - 1];
        if (SLOW && oldpeak) {
            // some lane holds a peak older than the bitmap ring reaches (or one from before the pass)
            if constexpr ((EMIT & 1) != 0) bw += bw;   // (the position belongs to u: every step shifts; these bits go to the ring)
            if (lane_of(em)) {
                lz_emit_slow(ring, bm, flushed, i_begin, s, e, jb + sp, jb + u);
                if constexpr (BOOK) {
                    rs = max(u, sp + W1 + 1);
                } else {
                    lm = sp;
                    r0 = u;
                }
            }
            if constexpr (BOOK) {
                off = moff[0];
#pragma unroll
                for (int k = 0; k < NM - 1; ++k) nx[k] = k + 1 < NM - 1 ? moff[k + 1] : 0ull;
                book_mask_from_sp<NM - 1>(em, u, off, nx);
            }
        } else {
            if constexpr (BOOK) {
                if constexpr ((EMIT & 1) != 0) bw = shift_in(bw, em);
                else if (lane_of(em)) bw |= bit;
                rs = lane_of(em) ? u + NM : rs;
                const lmask_t eusual = em & hist[H1];
                off = moff[0] | eusual;
#pragma unroll
                for (int k = 0; k < NM - 1; ++k) nx[k] = k + 1 < NM - 1 ? (moff[k + 1] | eusual) : eusual;
            } else {
                if (lane_of(em)) {
                    bw |= bit;
                    lm = sp;
                    r0 = u;
                }
            }
            const lmask_t erare = em & ~hist[H1];
            if constexpr ((EMIT & 2) != 0) {
                // both rare blocks behind one test that the usual step falls through (the emission's rs first: the
                // recorded run reads it)
                const lmask_t rec = dom & hot;
                if (__builtin_expect((erare | rec) != 0ull, 0)) {
                    if (erare != 0ull) emit_rare(erare, u, bit, off, nx);
                    if (rec != 0ull) record_run(rec, u);
                }
            } else {
                if (erare != 0ull) emit_rare(erare, u, bit, off, nx);
            }
        }
        sv = lane_of(upd) ? v : sv;
        sp = lane_of(pos) ? u : sp;
        inpk = (inpk & ~em) | ent;
        val = val & ~em;
        if constexpr (SLOW) {
            // a frozen lane's history does not age
#pragma unroll
            for (int k = H1; k >= 1; --k) hist[k] = (hist[k - 1] & live) | (hist[k] & ~live);
            hist[0] = pos | (hist[0] & ~live);
        } else {
#pragma unroll
            for (int k = H1; k >= 1; --k) hist[k] = hist[k - 1];
            hist[0] = pos;
        }
        // lazy long detector: the run that ends at this reset is recorded if it was hot; a new run starts at the
        // peak's last reset (its emission); resets in between leave nothing behind
        if ((EMIT & 2) == 0 || (SLOW && oldpeak)) {
            const lmask_t rec = dom & hot;
            if (rec != 0ull) record_run(rec, u);
        }
        lmask_t on;
        if constexpr (BOOK) {
            on = ~off;
#pragma unroll
            for (int k = 0; k < NM - 1; ++k) {
                // a frozen lane's mask does not age, like its hist[]
                if constexpr (SLOW) moff[k] = (nx[k] & live) | (moff[k] & ~live);
                else moff[k] = nx[k];
            }
        } else {
            on = __ballot(lm < u - W1);
        }
        if constexpr (SLOW) on &= live;
        hot = (hot & ~dom) | (on & hck & (~dom | em));
    }
    // the rare emission (lanes `erare`): an older peak.  Undo the usual bit, set the right one (its word is in the ring)
    __device__ __forceinline__ void emit_rare(const lmask_t erare, const int u, const uint32_t bit, lmask_t &off,
                                              lmask_t (&nx)[NM - 1]) {
        if (lane_of(erare)) {
            if constexpr ((EMIT & 1) != 0) bw &= ~1u;
            else bw &= ~bit;
            const int p = jb + sp, own = s - i_begin;
            if (p >= own) atomicOr(&ring[(p >> 5) & (LZ_RING_WORDS - 1)], 1u << (p & 31));
            else if (jb >= own) ring[LZ_PRE] = (uint32_t)(i_begin + p);  // inherited, see lz_emit_slow
            if constexpr (BOOK) rs = max(u, sp + W1 + 1);
        }
        // (sp <= u - H1 - 2: masked up to index u + NM - 2 at the most)
        if constexpr (BOOK) book_mask_from_sp<NM - 2>(erare, u, off, nx);
    }
    __device__ __forceinline__ void record_run(const lmask_t rec, const int u) {
        if (lane_of(rec)) nrec = lz_record(runs, nrec, ib + run_start(), ib + u, s, e, n);
    }
    // first index (block-relative) of the long detector's current run: behind its last reset and behind the mask
    __device__ __forceinline__ int run_start() const {
        if constexpr (BOOK) return rs;
        else return max(r0, lm + W1 + 1);
    }
    // BOOK: lanes `m` emitted a peak at sp that need not lie H1 + 1 indices back: their mask reaches up to sp + W1
    // (KN: how many of the following indices it can reach)
    template <int KN>
    __device__ __forceinline__ void book_mask_from_sp(const lmask_t m, const int u, lmask_t &off, lmask_t (&nx)[NM - 1]) const {
        off |= m & __ballot(sp + W1 >= u);
#pragma unroll
        for (int k = 0; k < KN; ++k) nx[k] |= m & __ballot(sp + W1 >= u + k + 1);
    }
    // the bitmap word moves on when position j - H1 - 1 enters the next 32-position span
    __device__ __forceinline__ void bw_advance() {
        const int p = jb - 1;  // last position of the span that is complete (jb is a multiple of 32 here)
        if constexpr ((EMIT & 1) != 0) {
            // the ring keeps the natural bit order.  (bw need not be zeroed, the span's 32 shifts push every older bit
            // out; it is, one v_mov per 32 indices: with the word live across the flush k_event<3, float> spills a VGPR)
            atomicOr(&ring[(p >> 5) & (LZ_RING_WORDS - 1)], __builtin_bitreverse32(bw));
            bw = 0u;
            return;
        }
        atomicOr(&ring[(p >> 5) & (LZ_RING_WORDS - 1)], bw);
        bw = 0u;
    }
    template <int U>
    __device__ __forceinline__ void dstep() {
        if constexpr (U == H1 + 1) {
            if ((jb & 16) == 0) bw_advance();
        }
        dstep_core<false>(U, t1[U & 3], hc[U & 3], ~0ull);
    }
    // a step of a block near the read's ends (or holding a very old peak): lanes that are done and indices behind
    // the read's end are frozen
    template <int U>
    __device__ __forceinline__ void dstep_edge() {
        if constexpr (U == H1 + 1) {
            if ((jb & 16) == 0) bw_advance();
        }
        const lmask_t live = ~done & __ballot((unsigned)(ib + U) < (unsigned)n);
        dstep_core<true>(U, t1[U & 3], hc[U & 3], live);
    }
    // the statistic is defined as 0 at the read's first / last W1 indices (events.c:332-338)
    // ... and so is the long window's at the last W2: it cannot exceed thr2 there.  (Its window sums reach behind the
    // read there -- whatever lies behind it made the long detector "hot" at the end of most short RNA reads, and each
    // of them paid for an exact replay of its last run.)
    __device__ __forceinline__ void slow_fix(const int u0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in1 = (unsigned)(ib + u0 + k - W1) < cnt1;
            t1[k] = in1 ? t1[k] : 0.0f;
            nk[k] &= __ballot(in1);
            hc[k] &= __ballot((unsigned)(ib + u0 + k - W2) < cnt2);
        }
    }

    // four indices U0..U0+3
    template <int U0>
    __device__ __forceinline__ void quad() {
        tstep<U0>();
        tstep<U0 + 1>();
        tstep<U0 + 2>();
        tstep<U0 + 3>();
        if (slow) slow_fix(U0);
        if constexpr (FLAGGED) {
            unsigned bad1 = 0u, bad2 = 0u;
            repair_mark<W1>(rep, next_t, ib + U0, cnt1, cnt2, bad1, bad2);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                nk[k] |= __ballot(((bad1 >> k) & 1u) != 0u);
                hc[k] |= __ballot(((bad2 >> k) & 1u) != 0u);
            }
        }
        // rare: evaluations whose certificate failed are redone with the reference expression
        const lmask_t anybad = (nk[0] | nk[1] | nk[2] | nk[3]) & ~done;
        if (anybad != 0ull) {
            if (lane_of(anybad)) {
                const unsigned bits = (lane_of(nk[0]) ? 1u : 0u) | (lane_of(nk[1]) ? 2u : 0u) |
                                      (lane_of(nk[2]) ? 4u : 0u) | (lane_of(nk[3]) ? 8u : 0u);
                const Redo4 r4 = redo_quad<W1, T, FLAGGED>(base, sc, rep.P, rep.P2, ib + U0, cnt1, bits, t1[0], t1[1],
                                                           t1[2], t1[3]);
                t1[0] = r4.v[0]; t1[1] = r4.v[1]; t1[2] = r4.v[2]; t1[3] = r4.v[3];
            }
        }
        if (slow) {
            dstep_edge<U0>();
            dstep_edge<U0 + 1>();
            dstep_edge<U0 + 2>();
            dstep_edge<U0 + 3>();
        } else {
            dstep<U0>();
            dstep<U0 + 1>();
            dstep<U0 + 2>();
            dstep<U0 + 3>();
        }
    }

    // ---- ring initialisation: prefix sums from the origin o = i_begin - W2 over w[k] = x[o + k], k < 2*W2;
    // A sides / long estimates of the window positions in front of the first index
    template <int K>
    __device__ __forceinline__ void init_step(double &ps, double &pq, const float (&w)[2 * W2], double (&hs)[W2 + 1],
                                              double (&hq)[W2 + 1]) {
        const float x = w[K];
        ps = ps + (double)x;
        pq = pq + (double)(x * x);
        constexpr int k1 = K + 1;  // now ps = P(o + k1)
        if constexpr (k1 <= W2) { hs[k1] = ps; hq[k1] = pq; }
        if constexpr (k1 >= W2) { Ps[(k1 - W2) % NP] = ps; Pq[(k1 - W2) % NP] = pq; }  // P(i_begin + k1 - W2)
        // short window position p = o + k1 - W1 in [i_begin - W1, i_begin): sums P(o + k1) - P(o + k1 - W1)
        if constexpr (k1 >= W2 && k1 < W2 + W1) {
            constexpr int pr = k1 - W1;
            ar[((k1 - W1 - W2) % NA + NA) % NA] = sgk_arole<W1, !FLAGGED>(ps - hs[pr], pq - hq[pr]);
        }
        // long window position p = o + k1 - W2 in [i_begin - W2, i_begin)
        if constexpr (k1 >= W2 && k1 < 2 * W2) {
            constexpr int pr = k1 - W2;
            ls[((k1 - 2 * W2) % NL + NL) % NL] = sgk_lside<W2>(ps - hs[pr], pq - hq[pr]);
        }
    }
    template <int... Ks>
    __device__ __forceinline__ void init_rings(const float (&w)[2 * W2], std::integer_sequence<int, Ks...>) {
        double ps = 0.0, pq = 0.0;
        double hs[W2 + 1], hq[W2 + 1];
        hs[0] = 0.0;
        hq[0] = 0.0;
        (init_step<Ks>(ps, pq, w, hs, hq), ...);
    }

    // LEAD: the same prefix sums; short windows at the positions [i_begin - W2, i_begin + W1): f32 sums of those from
    // i_begin on, A sides of those from i_begin - W1 on, and the long estimates of [i_begin - W2, i_begin) from pairs
    // of them, as every later step forms them (what a pass decides at an index does not depend on where it began)
    __device__ __forceinline__ void init_lead(const float (&w)[2 * W2]) {
        double hs[2 * W2 + 1], hq[2 * W2 + 1];  // P(o + k)
        hs[0] = 0.0;
        hq[0] = 0.0;
#pragma unroll
        for (int k = 0; k < 2 * W2; ++k) {
            hs[k + 1] = hs[k] + (double)w[k];
            hq[k + 1] = hq[k] + (double)(w[k] * w[k]);
        }
#pragma unroll
        for (int k = W2; k <= 2 * W2; ++k) { Ps[(k - W2) % NP] = hs[k]; Pq[(k - W2) % NP] = hq[k]; }  // P(i_begin + k - W2)
        float sf[W2 + W1], sqf[W2 + W1];  // short window position p = o + j
#pragma unroll
        for (int j = 0; j < W2 + W1; ++j) {
            const double c = hs[j + W1] - hs[j], cq = hq[j + W1] - hq[j];
            sf[j] = (float)c;
            sqf[j] = (float)cq;
            if (j >= W1) ar[(j - W2 + NA2) % NA2] = sgk_arole<W1, true>(c, cq);
            if (j >= W2) { ss[(j - W2) % NS] = sf[j]; sqs[(j - W2) % NS] = sqf[j]; }
        }
#pragma unroll
        for (int j = 0; j < W2; ++j) ls[(j - W2 + NL) % NL] = sgk_lside_halves<W2>(sf[j], sqf[j], sf[j + W1], sqf[j + W1]);
    }

    template <int... Qs>
    __device__ __forceinline__ void block(std::integer_sequence<int, Qs...>) {
        (quad<4 * Qs>(), ...);
    }
};

// flush 8 ring words (the 256 positions starting at pass-relative position p0, a multiple of 256) of this lane to
// the read's bitmap, in 16-bit units: i_begin is a multiple of 16, so pass-relative units are the bitmap's units, and
// only units inside the lane's own range [own_lo, own_hi) (pass-relative; multiples of 16, or the read's end) are
// written -- every owned unit is written exactly once per pass, zero or not
__device__ __forceinline__ void lz_flush(uint32_t *ring, unsigned long long *bm, int i_begin, int p0, int own_lo,
                                         int own_hi) {
    uint16_t *bm16 = reinterpret_cast<uint16_t *>(bm);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int p = p0 + 32 * k;
        const int wi = (p >> 5) & (LZ_RING_WORDS - 1);
        const uint32_t w = ring[wi];
        ring[wi] = 0u;
        if (p >= own_lo && p < own_hi) bm16[(i_begin + p) >> 4] = (uint16_t)(w & 0xffffu);
        if (p + 16 >= own_lo && p + 16 < own_hi) bm16[(i_begin + p + 16) >> 4] = (uint16_t)(w >> 16);
    }
}

// One pass of the lazy detector over the wave's chunks.
//   given  : (per lane) this lane starts from snap.st0 -- the true state at its first index: a re-run of a lane whose
//            speculation failed, or the first lane of a segment that is run from a known state; the other lanes
//            start from the fresh state (true for the first lane of a read, speculative elsewhere)
//   lead   : this lane's warm-up before its chunk start s (0 for a lane that starts from a true state)
//   steps  : indices every lane runs (wave-uniform: warm-up + chunk length)
//   active : whether this lane runs in this pass
// Writes the lane's bitmap words, its hot-run records and (speculative pass) snap.init / snap.at_e.
template <int W1, typename T, bool FLAGGED, bool LEAD = false, bool RT = false>
__device__ __forceinline__ void pass_lazy(const ReadCtx<T> &rc, bool given, int lead, int steps, bool active, int s,
                                          int e, LzLds *L, const RepairCtx *rep, bool by_progress = false,
                                          const Det<W1, RT> dt = Det<W1, RT>{}) {
    using LP = LazyPass<W1, T, FLAGGED, LEAD, RT>;
    constexpr int W2 = LP::W2, R = LP::R;
    if (!__any(active)) return;
    const int l = lane_id();
    LP f;
    f.dt = dt;
    f.n = (int)rc.n;
    // lanes that do not take part in the pass own nothing: nothing they emit or record can land anywhere
    f.s = active ? s : 0x7fffffff;
    f.e = active ? e : 0x7fffffff;
    f.bm = rc.bm;
    f.sc = rc.sc;
    f.base = rc.base;
    f.lo = (int)(rc.lo < -(1 << 30) ? -(1 << 30) : rc.lo);
    f.hi = (int)(rc.hi > 0x7fffffffLL ? 0x7fffffffLL : rc.hi);
    f.ring = L->ring[l];
    f.runs = L->runs[l];
    const int n = f.n;
    const int i_begin = s - lead;  // multiple of 16, never negative
    f.i_begin = i_begin;
#pragma unroll
    for (int k = 0; k < LZ_RING_WORDS; ++k) f.ring[k] = 0u;
    if (active) f.ring[LZ_PRE] = 0xffffffffu;  // no inherited emission in this pass yet
#pragma unroll
    for (int k = 0; k < 4; ++k) { f.t1[k] = 0.0f; f.nk[k] = 0ull; f.hc[k] = 0ull; }
    {
        // x[i_begin - W2 .. i_begin + W2): prefix sums from the origin i_begin - W2
        float w[2 * W2];
#pragma unroll
        for (int k = 0; k < 2 * W2; ++k) {
            int p = i_begin - W2 + k;
            p = p > f.hi - 1 ? f.hi - 1 : p;
            p = p < 0 ? 0 : p;  // lane 0: positions before the read (their window positions are marked below)
            w[k] = to_pa(f.base[p], f.sc);
        }
#pragma unroll
        for (int k = 0; k < LP::NP; ++k) { f.Ps[k] = 0.0; f.Pq[k] = 0.0; }
        if constexpr (LEAD) f.init_lead(w);
        else f.init_rings(w, std::make_integer_sequence<int, 2 * W2>{});
        // The statistic is defined as 0 at the read's first W1 indices (events.c:332-338): their A side is a window
        // position in front of the read.  Lane 0 marks those ring entries (NaN): the evaluation cannot be certified
        // and the exact path returns the 0.  (LEAD: the ring also holds the positions 0 .. W1-1, which are real.)
        if (i_begin == 0) {
            if constexpr (LEAD) {
#pragma unroll
                for (int k = 1; k <= W1; ++k) f.ar[LP::NA2 - k].va = __builtin_nan("");
            } else {
#pragma unroll
                for (int k = 0; k < LP::NA; ++k) f.ar[k].va = __builtin_nan("");
            }
        }
    }
    // leading samples of the first block: x[i_begin + W2 .. +16)
    f.load_lead(f.cur, i_begin + W2);

    // detector state
    f.sv = FLT_MAX;
    f.sp = 0;
    f.inpk = 0ull; f.val = 0ull; f.strong = 0ull; f.hot = 0ull;
#pragma unroll
    for (int k = 0; k <= LP::H1; ++k) f.hist[k] = 0ull;
    f.bw = 0u;
    f.lm = LZ_NONE;
    f.r0 = 0;  // the (pseudo) reset a speculative pass starts from; index 0 for lane 0
    f.rs = 0;
#pragma unroll
    for (int k = 0; k < LP::NM - 1; ++k) f.moff[k] = 0ull;
    if (__any(given)) {
        LzSnapState st = L->snap.st0[l];
        if (!given) { st.sp = -1; st.sv = FLT_MAX; st.lm = LZ_NONE; st.r0 = i_begin; st.bits = 0u; }  // fresh
        f.sv = st.sv;
        f.inpk = __ballot((st.bits & 1u) != 0u);
        f.val = __ballot((st.bits & 2u) != 0u);
        f.strong = __ballot((st.bits & 4u) != 0u);
        f.hot = __ballot((st.bits & 8u) != 0u);
        f.sp = (st.bits & 1u) ? st.sp - i_begin : 0;
        f.lm = st.lm == LZ_NONE ? LZ_NONE : st.lm - W1 - i_begin;  // handed over as masked_to; kept as the peak position
#pragma unroll
        for (int k = 0; k <= LP::H1; ++k) f.hist[k] = __ballot((st.bits & 1u) && st.sp == i_begin - 1 - k);
        f.r0 = st.r0 - i_begin;
        if constexpr (LP::BOOK) {
            const int mt = st.lm == LZ_NONE ? LZ_NONE : st.lm - i_begin;  // masked_to, below NM - 1: its emission lies behind
            f.rs = max(st.r0 - i_begin, mt + 1);
#pragma unroll
            for (int k = 0; k < LP::NM - 1; ++k) f.moff[k] = __ballot(mt >= k);
        }
    }
    f.nrec = 0;
    f.done = ~__ballot(active);
    f.flushed = 0;
    if constexpr (FLAGGED) {
        f.dirty = 2 * W2;  // the ring was filled by a handful of additions that were not checked
        f.rep = *rep;
        // first event whose influence [t-W2+1, t+W2] is not entirely before this pass' first index
        f.next_t = 0x7fffffff;
        for (int k = 0; k < f.rep.nev; ++k) {
            const int t = f.rep.ev[k];
            if (t + W2 >= i_begin && t < f.next_t) f.next_t = t;
        }
    }
    const int main_steps = steps;
    f.cnt1 = (n - 2 * W1 + 1) > 0 ? (unsigned)(n - 2 * W1 + 1) : 0u;
    f.cnt2 = (n - 2 * W2 + 1) > 0 ? (unsigned)(n - 2 * W2 + 1) : 0u;
    // pass-relative range of the positions this lane owns (its bitmap words)
    const int own_lo = lead, own_hi = active ? lead + (e - s) : lead;  // (lane 0: lead = 0)

    auto snapshot = [&](int ib) -> LzSnapState {
        // ib: absolute index of the block about to start (positions are relative to it)
        LzSnapState st;
        const bool ip = lane_of(f.inpk);
        st.sv = f.sv;
        st.sp = ip ? ib + f.sp : -1;
        // normalised when it no longer masks.  (BOOK: at a block's start every emission lies behind, so a run start in
        // front -- rs > 0 -- is the mask's end + 1, and one behind says that nothing masks)
        if constexpr (LP::BOOK) st.lm = (f.rs - 1 < 0) ? LZ_NONE : ib + f.rs - 1;
        else st.lm = (f.lm + W1 < 0) ? LZ_NONE : ib + f.lm + W1;
        // what the long detector's current run STARTS with: the first index behind the last reset that is not masked.
        // (The reset index alone is not enough once the mask is normalised away: a lane that takes this state over
        // would replay a hot run from the reset, through indices the mask hid from the reference's long detector --
        // found by the soak with a 16-sample warm-up, tests/golden/soak_seed41_*.npz.)
        st.r0 = ib + f.run_start();
        st.bits = (ip ? 1u : 0u) | ((ip && lane_of(f.val)) ? 2u : 0u) | ((ip && lane_of(f.strong)) ? 4u : 0u) |
                  (lane_of(f.hot) ? 8u : 0u);
        return st;
    };

    // (by_progress: the wave's first pass over its span, under a policy that ranks by what is left to do -- in steps, not
    // as a fraction of the span: a segment of a cut read starts where a whole read is when it has as much left)
    constexpr int PRIO_STEPS = 400;   // a quarter of the pass over a 100 000-sample read
    const int q1 = by_progress ? main_steps - 3 * PRIO_STEPS : -1, q2 = by_progress ? main_steps - 2 * PRIO_STEPS : -1,
              q3 = by_progress ? main_steps - PRIO_STEPS : -1;
    if (by_progress) {
        if (q1 > 0) __builtin_amdgcn_s_setprio(3);
        else if (q2 > 0) __builtin_amdgcn_s_setprio(2);
        else if (q3 > 0) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
    }
    int jb = 0;
    for (;;) {
        const int ib = i_begin + jb;
        if ((jb & 255) == 0 && jb >= 512) {
            lz_flush(f.ring, f.bm, i_begin, jb - 512, own_lo, own_hi);
            f.flushed = jb - 256;
        }
        // blocks that touch the read's last W2 indices (the statistics are defined as 0 there) or its end take the
        // predicated forms of the steps; so does a block in which some lane holds a peak older than the bitmap ring
        // or one from in front of its own range
        const bool lane_edge = ib + R - 1 > n - W2;
        // (... or a peak in front of the lane's own range in the range's first block: it may be emitted there within
        // w/2 indices, as a "usual" peak whose bit the fast steps would put into the bitmap word; in later blocks it is
        // an "older peak", which the fast steps hand to the ring or, in front of the range, to LZ_PRE)
        // (one ballot per compare, combined as masks: a bool OR / AND of compares reaches __ballot through a vector 0/1)
        const lmask_t old_peak = __ballot(f.sp < -(256 - 2 * R)) | (__ballot(f.sp + jb < own_lo) & __ballot(jb == own_lo));
        f.oldpeak = (old_peak & f.inpk & ~f.done) != 0ull;
        f.slow = f.oldpeak || (__ballot(lane_edge) & ~f.done) != 0ull;
        f.ib = ib;
        f.jb = jb;
        // issue the loads of the NEXT block's leading samples now; consumed one iteration later
        Lead16<T> nxt;
        f.load_lead(nxt, ib + R + W2);
        f.block(std::make_integer_sequence<int, R / 4>{});
        f.cur = nxt;
        // rebase the block-relative positions
        f.sp -= R;
        if constexpr (LP::BOOK) {
            f.rs -= R;
        } else {
            f.lm = f.lm < LZ_NONE ? LZ_NONE : f.lm - R;
            f.r0 -= R;
        }
        if constexpr (FLAGGED) f.dirty = f.dirty < -(1 << 20) ? f.dirty : f.dirty - R;
        jb += R;
        if (jb == q1) __builtin_amdgcn_s_setprio(2);
        else if (jb == q2) __builtin_amdgcn_s_setprio(1);
        else if (jb == q3) __builtin_amdgcn_s_setprio(0);
        {
            // state snapshots live in LDS (they are only needed after the pass)
            const int nb = i_begin + jb;  // first index of the next block
            if (active && lead > 0 && jb == lead) L->snap.init[l] = snapshot(nb);
            if (active && nb == e) L->snap.at_e[l] = snapshot(nb);
            // a lane stops at the end of its range; a peak still pending there is emitted by the lane behind
            // (lz_emit_slow), and dropped at the read's end as in the reference, whose loop ends at n-1
            const lmask_t reach = __ballot(nb >= e) & ~f.done;
            // the run still open at the end of the read is replayed by the lane that holds the read's last index --
            // recorded HERE: the lane may step on (other lanes of the wave have more to do, and in k_event_multi their
            // reads are longer) through whatever lies behind the read, and its run bookkeeping with it
            if ((reach & f.hot) != 0ull) {
                if (lane_of(reach & f.hot) && e == n) f.nrec = lz_record(f.runs, f.nrec, nb + f.run_start(), n, s, e, n);
            }
            f.done |= reach;
            // ... and it steps on without the exact redo of uncertified statistics: whatever it decides from here on
            // must not land in its own range.  Out of its peak, every position it can emit lies behind the range.
            f.inpk &= ~reach;
            f.val &= ~reach;
            f.strong &= ~reach;
        }
        if (jb >= main_steps && f.done == ~0ull) break;
    }
    // remaining ring words (the current bitmap word first)
    {
        const int p = jb - LP::H1 - 2 < 0 ? 0 : jb - LP::H1 - 2;  // a position inside the word bw stands for
        uint32_t w = f.bw;
        if constexpr ((LP::EMIT & 1) != 0) {
            // the word has seen m < 32 shifts since its span began (14 or 30: jb is a multiple of 16); its first position
            // sits in bit m - 1.  Reversed, the span's positions are the top m bits.
            const int m = (jb - LP::H1 - 1) & 31;
            w = __builtin_bitreverse32(w) >> (32 - m);
        }
        atomicOr(&f.ring[(p >> 5) & (LZ_RING_WORDS - 1)], w);
    }
    for (int p0 = f.flushed; p0 < jb; p0 += 256) lz_flush(f.ring, f.bm, i_begin, p0, own_lo, own_hi);
    if (active) L->nrec[l] = f.nrec;
}

// Exact replay of the long detector (events.c:383-440, k = 1) over one hot run per lane: from the fresh state a
// reset leaves, over the indices [i, b) of the run (inside a run masked_to does not change and every index is
// processed).  Peaks that lie in [bits_lo, bits_hi) are ORed into the read's bitmap.
// COLLECT: they are not set in the bitmap, *found is set instead (chain_segment: a peak in front of a seam lies in
// another wave's words).  A template argument, not a pointer test: what the other callers compile to must not depend
// on whether chain_segment is in the unit.
// (`inline`: pins the inlining of both instances into k_event_seg, as in the unit that held every kernel -- out of line
// they cost its int16 instances 80 bytes of scratch)
template <int W1, typename T, bool FLAGGED, bool COLLECT = false, bool RT = false>
__device__ inline void replay_run(const ReadCtx<T> &rc, const RepairCtx *rep, bool has, int i, int b, int bits_lo,
                           int bits_hi, EvHeader *hdr, int *found = nullptr, const Det<W1, RT> dt = Det<W1, RT>{}) {
    if (has && b > i) atomicAdd(&hdr->n_replay_idx, (unsigned long long)(b - i));
    constexpr int W2 = 2 * W1;
    const float ph = dt.ph(), thr2 = dt.thr2();
    const int n = (int)rc.n;
    const unsigned cnt2 = (n - 2 * W2 + 1) > 0 ? (unsigned)(n - 2 * W2 + 1) : 0u;
    uint32_t *bm32 = reinterpret_cast<uint32_t *>(rc.bm);
    int lp = -1;
    float lv = FLT_MAX;
    bool lvalid = false;
    while (__any(has && i < b)) {
        if (has && i < b) {
            float v2 = 0.0f;
            if ((unsigned)(i - W2) < cnt2) {
                if constexpr (FLAGGED) v2 = tstat_prefix_at(rep->P, rep->P2, i, W2);
                else v2 = tstat_exact_at<T>(rc.base, rc.sc, i, W2);
            }
            if (lp < 0) {
                if (v2 < lv) {
                    lv = v2;
                } else if (v2 - lv > ph) {
                    lv = v2;
                    lp = i;
                }
            } else {
                if (v2 > lv) {
                    lv = v2;
                    lp = i;
                }
                if (lv - v2 > ph && lv > thr2) lvalid = true;
                if (lvalid && (i - lp) > W2 / 2) {
                    if (lp > 0 && lp < n && lp >= bits_lo && lp < bits_hi) {
                        if constexpr (COLLECT) *found = 1;
                        else atomicOr(&bm32[lp >> 5], 1u << (lp & 31));
                    }
                    lp = -1;
                    lv = v2;
                    lvalid = false;
                }
            }
            ++i;
        }
    }
}
// ... over the recorded hot runs of the wave's lanes.  bits_lo: first index of the span this wave owns (a run that
// began in front of it leaves its peaks in front of the span to whoever replays the span's cross runs)
// (`inline`, as above: out of line -- where k_event<3, short> with the mask-history bookkeeping had it -- the read's
// context has to live in scratch for it)
template <int W1, typename T, bool FLAGGED, bool RT = false>
__device__ inline void replay_long_runs(const ReadCtx<T> &rc, LzLds *L, const RepairCtx *rep, bool active, int bits_lo,
                                        EvHeader *hdr, const Det<W1, RT> dt = Det<W1, RT>{}) {
    const int l = lane_id();
    const int nrec = active ? L->nrec[l] : 0;
    for (int k = 0; k < LZ_NREC; ++k) {
        const bool has = k < nrec;
        if (!__any(has)) break;
        const int i = has ? L->runs[l][k].a : 0;
        const int b = has ? L->runs[l][k].b : 0;
        replay_run<W1, T, FLAGGED, false, RT>(rc, rep, has, i, b, bits_lo, 0x7fffffff, hdr, nullptr, dt);
    }
}

// speculative pass + verification / re-run loop + replay of the hot long-detector runs over the span [a, b) of a read
// (a multiple of 16; the whole read: a = 0, b = n).
//   mode 0: the state at a is the fresh one (a = 0: the read's start)
//   mode 1: unknown: the first lane warms up in front of a like every other lane; the state it reached at a is
//           left in seg->init0, to be compared with the end state of the span in front (chain_segment)
//   mode 2: the state at a is L->snap.st0[0], put there by the caller
// seg (spans of a read that several waves share; null otherwise) receives the state at b and the hot runs that began
// in front of a.
// Returns 0 when the span is done, 1 when the fast pass cannot take the read (alignment / room around the read), 2
// when a lane met more hot runs than it can record (pathological signal: constant stretches, tiny variances).
//
// MULTI (k_event_multi): the wave holds 64 / lanes reads, `lanes` consecutive lanes each (rc, b and the return code are
// per lane; a = 0, mode 0, no seg): a short read on all 64 lanes spends more steps on warm-ups than on its samples.
// LEAD: the form of the fast pass (LazyPass).
template <int W1, typename T, bool FLAGGED, bool MULTI = false, bool LEAD = false, bool RT = false>
__device__ __forceinline__ int detect_span(const ReadCtx<T> &rc, EvHeader *hdr, LzLds *L, const RepairCtx *rep,
                                           const int a, const int b, const int mode, const int lead_override,
                                           SegState *seg, const int lanes = 64,
                                           const Det<W1, RT> dt = Det<W1, RT>{}) {
    const int n = (int)rc.n;
    if constexpr (!MULTI) {
        if (b <= a) return 0;
    }
    // speculative warm-up before every chunk.  RNA events are ~5x longer, so the automata converge later: with 64
    // samples ~1.4 % of the chunk boundaries need a re-run, with 256 about 0.002 %.  A re-run costs the wave one
    // more pass over a chunk (K samples), the warm-up costs `lead` samples per lane: short reads (small K) are
    // better off with a short warm-up and the occasional re-run, long reads with a long one.
    // (DNA, long reads: 32 samples were tried: 6 re-runs per 640 000 chunk boundaries of the benchmark, no gain.)
    const int len = b - a;
    int lead = len < 32768 ? LEAD_DNA_SHORT : LEAD_DNA;
    if (W1 == 7) lead = len <= 32768 ? LEAD_RNA_SHORT : LEAD_RNA;
    if constexpr (MULTI) {
        // the same rule for the same chunk length: what 64 lanes would see of a read 64 / lanes times as long
        const long long len64 = (long long)len * (64 / lanes);
        lead = len64 < 32768 ? LEAD_DNA_SHORT : LEAD_DNA;
        if (W1 == 7) lead = len64 <= 32768 ? LEAD_RNA_SHORT : LEAD_RNA;
    }
    if (lead_override > 0) lead = lead_override;
    // the fast pass uses unguarded 4-byte-aligned 32-byte vector loads: it needs 16 readable samples behind the
    // read; other reads take the exact fallback
    const bool no_fast = (reinterpret_cast<uintptr_t>(rc.base) & 3u) != 0 || rc.hi < (int64_t)n + 16;
    if constexpr (!MULTI) {
        if (no_fast) return 1;
    }
    const int c = MULTI ? (lane_id() & (lanes - 1)) : lane_id();  // lane within its read
    int K, s, e0, lead_c;
    if (mode == 1) {
        // every lane warms up: lane c owns [a + cK, a + (c+1)K)
        K = 16 * ((len + 1023) / 1024);
        s = a + c * K;
        e0 = s + K;
        lead_c = lead;
    } else {
        K = MULTI ? chunk_len_lanes(len, lead, lanes) : chunk_len_fast(len, lead);
        s = c == 0 ? a : a + c * K + lead;
        e0 = c == 0 ? a + lead + K : s + K;
        lead_c = c > 0 ? lead : 0;
    }
    int TT = lead + K;
    int Kmax = K;
    if constexpr (MULTI) {  // the passes' step counts are the wave's: the longest of its reads
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const int o = __shfl_xor(Kmax, d, 64), t = __shfl_xor(TT, d, 64);
            Kmax = o > Kmax ? o : Kmax;
            TT = t > TT ? t : TT;
        }
    }
    const int e = e0 < b ? e0 : b;
    const bool active = s < b && !(MULTI && no_fast);
    {
        LzSnapState z;
        z.sp = -1; z.sv = FLT_MAX; z.lm = LZ_NONE; z.r0 = 0; z.bits = 0u;
        L->snap.init[lane_id()] = z;
        L->snap.at_e[lane_id()] = z;
        L->nrec[lane_id()] = 0;
        L->ring[lane_id()][LZ_PRE] = 0xffffffffu;
    }
    bool run = active;
    bool first = true;
    const int l = lane_id();
    const uint32_t pol = FLAGGED ? 0u : prio_policy(rc.dev);
    for (int iter = 0; iter < 66; ++iter) {
        pass_lazy<W1, T, FLAGGED, LEAD, RT>(rc, first ? (mode == 2 && c == 0) : true, first ? lead_c : 0, first ? TT : Kmax, run,
                                            s, e, L, rep, first && (pol == 1u || pol == 2u), dt);
        __syncthreads();
        // chunk c is right iff it started (at s) from the state chunk c-1 ended with
        const LzSnapState pe = L->snap.at_e[c > 0 ? l - 1 : l];
        const LzSnapState mine = L->snap.init[l];
        const bool bad = active && c > 0 && !lz_equal(pe, mine);
        const unsigned long long badmask = __ballot(bad);
        if (badmask == 0ull) break;
        __syncthreads();
        if (bad) {
            L->snap.init[l] = pe;
            L->snap.st0[l] = pe;
        }
        run = bad;
        first = false;
        if (l == 0) atomicAdd(&hdr->n_rerun, (uint32_t)__popcll(badmask));
        __syncthreads();
    }
    int rcode = 0;
    if constexpr (MULTI) {
        // per read: the lanes of a read that cannot be taken here, or whose lanes met too many hot runs, stand aside
        const unsigned long long over = __ballot(active && L->nrec[l] > LZ_NREC);
        const unsigned long long grp = (lanes >= 64 ? ~0ull : ((1ull << lanes) - 1ull)) << (l & ~(lanes - 1));
        if (no_fast) rcode = 1;
        else if (over & grp) rcode = 2;
    } else {
        if (__any(active && L->nrec[l] > LZ_NREC)) return 2;
    }
    const bool mine_ok = active && rcode == 0;
    if (seg) {
        // what the neighbours need: the states at both ends, the runs that began in front of the span
        const int last = __popcll(__ballot(active)) - 1;
        if (l == 0) {
            seg->init0 = L->snap.init[0];
            seg->end = L->snap.at_e[last];
        }
        const int nrec = active ? L->nrec[l] : 0;
        int ncross = 0;
        for (int k = 0; k < nrec; ++k) ncross += (L->runs[l][k].a < a) ? 1 : 0;
        const int incl = wave_incl_scan_i(ncross);
        const int total = wave_last_i(incl);
        if (total > SEG_CROSS_MAX) rcode = 2;
        else {
            int at = incl - ncross;
            for (int k = 0; k < nrec; ++k) {
                if (L->runs[l][k].a < a) seg->cross[at++] = L->runs[l][k];
            }
        }
        if (l == 0) seg->n_cross = total > SEG_CROSS_MAX ? 0u : (uint32_t)total;
    }
    // inherited emissions (lz_emit_slow) of the lanes' accepted runs.  Inside the span the bit is set here; one in
    // front of it lies in another wave's words: it is left in seg->pre -- the segment OWNS that boundary (chain_segment
    // builds the event that ends there), the bitmap never shows it.
    const int pre = mine_ok ? (int)L->ring[l][LZ_PRE] : -1;
    const bool pre_out = pre >= 0 && pre < a;
    if (seg) {
        const int npre = pre_out ? 1 : 0;
        const int incl = wave_incl_scan_i(npre);
        const int total = wave_last_i(incl);
        if (total > SEG_PRE_MAX) rcode = 2;
        else if (npre) seg->pre[incl - 1] = pre;
        if (l == 0) seg->n_pre = total > SEG_PRE_MAX ? 0u : (uint32_t)total;
    }
    const unsigned long long hotm = __ballot(mine_ok && L->nrec[l] > 0);
    const bool anypre = __any(pre >= 0);
    if (hotm != 0ull || anypre) {
        if (l == 0 && hotm != 0ull) atomicAdd(&hdr->n_hot_runs, (uint32_t)__popcll(hotm));
        __threadfence_block();
        __syncthreads();  // every lane's bitmap words are in memory before anything is ORed into them
        if (pre >= 0 && !pre_out) atomicOr(reinterpret_cast<uint32_t *>(rc.bm) + (pre >> 5), 1u << (pre & 31));
        if (hotm != 0ull) replay_long_runs<W1, T, FLAGGED, RT>(rc, L, rep, mine_ok, a, hdr, dt);
    }
    return rcode;
}
// one wave, one read
template <int W1, typename T, bool FLAGGED, bool RT = false>
__device__ __forceinline__ int detect_read_lazy(const ReadCtx<T> &rc, EvHeader *hdr, LzLds *L, const RepairCtx *rep,
                                                const Det<W1, RT> dt = Det<W1, RT>{}) {
    const int n = (int)rc.n;
    if (n <= 0) return 0;
    return detect_span<W1, T, FLAGGED, false, false, RT>(rc, hdr, L, rep, 0, n, 0, 0, nullptr, 64, dt);
}

}  // namespace sgk
