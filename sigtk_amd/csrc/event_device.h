// event_device.h -- the `event` hot path (reference: src/events.c:293-573) for gfx950: what every path uses.
//
// The unit of work is a SPAN of a read on one wavefront (64 lanes):
//
//   detector         (detect_span, LazyPass)  window sums -> t-statistics -> short/long peak detector.
//                    Lane c owns chunk c of the span (K samples, K a multiple of 16).  Each lane slides a
//                    running double prefix sum through a register ring, evaluates the reference's mixed
//                    float/double t-statistic expression tree (events.c:338-361) for the short window in
//                    certified fast arithmetic, steps the short detector automaton (events.c:383-440) as
//                    lane-mask algebra, and runs the long detector lazily (exact only where a rigorous bound
//                    cannot exclude a peak).  The automaton is serial in the reference; here every chunk
//                    starts SPECULATIVELY from the fresh state `lead` samples before its chunk, and the
//                    speculation is verified: chunk c is accepted iff its state at its chunk start equals
//                    chunk c-1's state at that position; mismatching chunks are re-run from the true state
//                    until a fixed point (exact in the general case; re-runs are counted in the status
//                    block).  Output: one bit per sample (peak positions) in a workspace bitmap.
//
//   builder          (build_read)  bitmap + samples -> event table (events.c:457-504).  Lane-local double prefix
//                    sums, wave scan across lanes, boundary records compacted in LDS, then one event per lane per
//                    round with one 16-byte store of (start, length, mean, stdv).
//
// and the kernels differ in what a wave's span is:
//
//   k_event          a whole read: detector and builder back to back in the same wave (most reads)
//   k_event_seg      a SEGMENT of a read that several waves share -- long reads, the tail split (k_seg_plan lists them):
//                    the wave of a segment runs the detector over it, checks the seam against the segment in front and
//                    builds its own events (chain_segment, round 4; a kernel of its own since round 5)
//   k_event_multi    several short reads per wave, `lanes` lanes each, on a side stream beside k_event (round 3)
//   k_event_param    persistent kernel for caller-supplied detector parameters: the fallback's exact path with the
//                    windows and thresholds as run-time values (event_param.hip)
//   k_event_fallback persistent kernel over the reads that fail the exactness guard: lane 0 reproduces
//                    compute_sum_sumsq's sequential double prefix scan (events.c:293-303) into workspace
//                    scratch, then the same detector and builder run with window/event sums taken as
//                    differences of those arrays, exactly as the reference does.
//
// Exactness guard: the reference accumulates double prefix sums sequentially and uses their differences; the
// fast path forms window sums and event sums directly.  Both give the real-number sums (hence identical bits)
// whenever no prefix sum can round: every sample is a multiple of 2^g (g = lowest bit of the smallest non-zero
// |x|) and all partial sums are below 2^(g+53).  Per read we check  ilogb(n*max|x|) - ilogb(min|x|!=0) <= 29
// for x and for the float squares, and that every non-zero |x| lies in [2^-20, 2^20] (the range in which the
// certified fast arithmetic of tstat_math.h has no subnormal intermediate); reads failing the check take the
// fallback kernel.
//
// Where what lives.  One translation unit per kernel, so that a kernel's code depends on what it uses only:
//   event_device.h     (this file) what every path shares: the chunk rules and warm-up lengths, the detector's
//                      thresholds, the per-read context, the issue-priority policy, the exactness guard, the segments'
//                      geometry, the waves per SIMD.
//   event_detect.h     the lazy detector: LazyPass, pass_lazy, the exact replay of the long detector's hot runs,
//                      detect_span / detect_read_lazy -- and the repair context of flagged reads (the fallback's template
//                      argument of the same code).
//   event_build.h      the builder: build_read on BuildLds, and EventLds, the LDS detector and builder take turns in.
//   event_whole.hip    k_event.
//   event_seg.hip      k_seg_plan, chain_segment, k_event_seg.
//   event_multi.hip    k_event_multi.
//   event_generic.h    the exact generic path on the reference's sequentially rounded prefix arrays: the prefix scan, the
//                      two automata stepped on every index (detect_pass / detect_read), the builder on those arrays --
//                      for a preset (<W1>) or for parameters given at run time (<0>, DetVals).
//   event_fallback.hip k_event_fallback: a preset's reads that fail the exactness guard, on event_generic.h.
//   event_param.hip    k_event_param: caller-supplied detector parameters (sgk_event_param), on event_generic.h; a
//                      persistent grid with per-workgroup prefix arrays, launched by launch_event_param.
//   event_launch.hip   launch_event: order, plan, side streams, the launches; it holds no kernel and launches them through
//                      the launch_k_* functions of event_args.h, one per kernel, each defined next to its kernel.
//   event_plan.hip     host only, in front of launch_event: options -> configuration, the batch's plan (event_plan), both
//                      workspace layouts, the parameters' route, and run_event behind every entry point of api.hip.
#pragma once
#include "event_args.h"
#include "sgk_common.h"
#include "tstat_math.h"

namespace sgk {

// speculative warm-up (samples) of the fast pass in front of every chunk, by preset and span length (detect_span)
constexpr int LEAD_DNA = 64, LEAD_DNA_SHORT = 32, LEAD_RNA = 256, LEAD_RNA_SHORT = 128;

// Chunk layout of the fast pass.  Every lane runs T = lead + K indices: lane 0 runs [0, T) from the true initial
// state and owns all of it; lane c >= 1 warms up over [cK, cK + lead) and owns [cK + lead, cK + lead + K).  No lane
// ever runs in front of the read.  K is a multiple of 16 (a lane owns whole 16-bit units of the bitmap), so short
// reads stay on most of the 64 lanes: 5 000 samples with lead 32 are 62 chunks of 80.
__device__ inline int chunk_len_fast(int n, int lead) {
    const int m = n > lead ? n - lead : 1;
    const int k = (m + 1023) / 1024;
    return 16 * (k < 1 ? 1 : k);
}
// ... when `lanes` lanes (a power of two) share the read instead of 64
__device__ inline int chunk_len_lanes(int n, int lead, int lanes) {
    const int m = n > lead ? n - lead : 1;
    const int k = (m + 16 * lanes - 1) / (16 * lanes);
    return 16 * (k < 1 ? 1 : k);
}

template <int W1>
struct DetParam;
template <>
struct DetParam<3> {  // event_detection_defaults, src/events.c:43-47
    static constexpr float thr1 = 1.4f, thr2 = 9.0f, ph = 0.2f;
};
template <>
struct DetParam<7> {  // event_detection_rna, src/events.c:50-54
    static constexpr float thr1 = 2.5f, thr2 = 9.0f, ph = 1.0f;
};
// Where the fast kernels take the three thresholds from.  RT = false: the preset's constants, an empty object that costs
// nothing.  RT = true: three wave-uniform floats of the kernel's arguments (EvArgs::thr1 / thr2 / ph) -- the presets'
// windows with the caller's thresholds (SGK_EVENT_PARAMS_PRESET_KERNELS; domain and per-site argument: DESIGN.md 3.16).
template <int W1, bool RT>
struct Det;
template <int W1>
struct Det<W1, false> {
    Det() = default;
    __device__ __forceinline__ explicit Det(const EvArgs &) {}
    __device__ __forceinline__ constexpr float thr1() const { return DetParam<W1>::thr1; }
    __device__ __forceinline__ constexpr float thr2() const { return DetParam<W1>::thr2; }
    __device__ __forceinline__ constexpr float ph() const { return DetParam<W1>::ph; }
};
template <int W1>
struct Det<W1, true> {
    float t1, t2, h;
    Det() = default;
    __device__ __forceinline__ explicit Det(const EvArgs &a) : t1(a.thr1), t2(a.thr2), h(a.ph) {}
    __device__ __forceinline__ float thr1() const { return t1; }
    __device__ __forceinline__ float thr2() const { return t2; }
    __device__ __forceinline__ float ph() const { return h; }
};

// ---------------------------------------------------------------- per-read context
template <typename T>
struct ReadCtx {
    const T *base;            // read's first sample
    int64_t n;                // samples in the read
    int64_t lo, hi;           // legal read-relative load range
    Scale sc;
    bool vec_ok;
    unsigned long long *bm;   // bitmap words of this read
    const double *P, *P2;     // fallback prefix arrays (n+1 entries) or null
    uint32_t dev;             // EvArgs::dev (development builds; 0 otherwise)
};

template <typename T>
__device__ inline ReadCtx<T> make_ctx(const EvArgs &a, uint32_t r) {
    ReadCtx<T> rc;
    const uint64_t o0 = a.offsets[r];
    rc.base = reinterpret_cast<const T *>(a.samples) + o0;
    rc.n = (int64_t)a.lengths[r];
    rc.lo = -(int64_t)o0;
    rc.hi = (int64_t)(a.n_alloc - o0);
    if (a.dig) rc.sc = make_scale(a.dig[r], a.off[r], a.rng[r]);
    else { rc.sc.offf = 0.0f; rc.sc.unit = 1.0f; }
    rc.vec_ok = ((reinterpret_cast<uintptr_t>(rc.base) & 15u) == 0);
    rc.bm = a.bitmap + (o0 >> 6) + r;
    rc.P = nullptr;
    rc.P2 = nullptr;
    rc.dev = a.dev;
    return rc;
}

// Issue priority by REMAINING work (round 5).  A SIMD arbitrates oldest-first among waves of equal priority: of the three
// waves that start together on a SIMD the oldest finishes its detector pass in 0.50 ms, the second in 0.71, the youngest
// in 0.97 (per-wave timestamps, profiles/r05_event_first_round.md) -- and then runs on alone, on a SIMD one wave cannot
// saturate (an instruction per 4.5 - 6 cycles instead of 2.3 - 4.45).  That, not the instruction cache (0.003 % misses)
// or address translation (949 misses per launch), is the "slow first round" of rounds 3 and 4, and the same thing happens
// when a launch drains.  A wave therefore lowers its own priority as it gets on with its read -- 3 while more than 1 200
// steps of its pass are left, 2, 1, 0 for the last 400 and in the builder -- so that whichever wave of a SIMD has most
// left to do issues first and the waves of a SIMD end together.
#ifndef SGK_PRIO_POLICY
#define SGK_PRIO_POLICY 1   // 0: none; 1: by the steps left of the detector pass 3 / 2 / 1 / 0, builder 0; 2: ... builder 3; 3: builder 3 only
#endif
__device__ __forceinline__ uint32_t prio_policy(uint32_t dev) {
#ifdef SGK_DEV
    return ((dev >> 8) & 7u) ? ((dev >> 8) & 7u) - 1u : (uint32_t)SGK_PRIO_POLICY;   // dev bits 8..10: policy + 1
#else
    (void)dev;
    return (uint32_t)SGK_PRIO_POLICY;
#endif
}

__device__ inline bool guard_ok(float mn, float mx, int64_t n) {
    if (!(mx > 0.0f)) return true;  // all samples zero
    // range in which the certified arithmetic of tstat_math.h (sgk_tstat_try_ab) has no subnormal intermediates
    if (mn < 9.5367431640625e-07f || mx > 1048576.0f) return false;
    const int eb = ilogb((double)n * (double)mx), em = ilogb((double)mn);
    if (eb - em > 29) return false;
    const float mnq = mn * mn, mxq = mx * mx;
    if (mnq < FLT_MIN) return false;
    const int ebq = ilogb((double)n * (double)mxq), emq = ilogb((double)mnq);
    if (ebq - emq > 29) return false;
    // the A side's mean is formed with one multiply (tstat_math.h: sgk_arole<W, SHORT>): magnitudes within 2^16
    return ilogbf(mx) - ilogbf(mn) <= 16;
}

// min non-zero |x| / max |x| of a read from the extremes of its raw samples (x = (raw + off) * unit is monotone in
// raw); returns false when the read crosses or touches zero pA (the smallest non-zero magnitude is then not known
// from the extremes; such reads fail the guard anyway: it tolerates a ratio of ~64 between the magnitudes)
__device__ inline bool raw_extremes_to_pa(int rmin, int rmax, const Scale &sc, float &mn, float &mx) {
    const float a = ((float)rmin + sc.offf), b = ((float)rmax + sc.offf);
    const float xa = fabsf(a * sc.unit), xb = fabsf(b * sc.unit);
    mn = fminf(xa, xb);
    mx = fmaxf(xa, xb);
    const bool same_sign = (a > 0.0f && b > 0.0f) || (a < 0.0f && b < 0.0f);
    return same_sign && mn > 0.0f && mx < __builtin_inff();
}

// span of segment g of a read of n samples
__device__ __forceinline__ void seg_span(uint32_t seg_len, uint32_t g, int64_t n, int &sa, int &sb) {
    const int64_t lo = (int64_t)g * seg_len, hi = lo + seg_len;
    sa = (int)lo;
    sb = (int)(hi < n ? hi : n);
}

// Which reads several wavefronts share, and in segments of which length (0: the read has a wavefront of its own).
//  * long reads (>= long_min samples): a wave per read cannot end before its longest read has;
//  * the TAIL SPLIT (round 4): the reads at dispatch positions >= split_from.  n_reads equal waves over the GPU's
//    resident wave slots run in rounds; the last, partial round costs nearly a whole one (10 000 reads over 3 072 slots:
//    3.26 rounds of work took the time of 3.75).  The reads of that round are cut into split_seg-sample segments -- as
//    many units as fill a round, each a fraction of a read long -- and run FIRST; every other read keeps the fused
//    detector + builder of its own wave (cutting every read costs more than the balance returns: the builder of a
//    cut read is a kernel of its own, profiles/archive/r04_event_experiments.md).
__device__ __forceinline__ uint32_t seg_len_of(const EvArgs &a, uint32_t pos, uint32_t n) {
    if (a.max_segs == 0) return 0u;
    if (n >= a.long_min) return a.seg_len;
    if (pos >= a.split_from && n > a.split_seg) return a.split_seg;
    return 0u;
}

// waves per SIMD the detector kernels are compiled for.  DNA preset: 168 VGPRs -> 3; RNA preset (deeper rings): 242
// VGPRs -> 2
constexpr int DET_WAVES_DNA = 3, DET_WAVES_RNA = 2;

}  // namespace sgk
