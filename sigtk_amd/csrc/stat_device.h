// stat_device.h -- per-read statistics, the JNN segmenter and the adaptor/polyA finder: the device code every path uses.
//
// Reference semantics that shape these kernels:
//   * meanf/meani16/stdvf/stdvi16 (src/stat.h:17-54) accumulate into ONE float, strictly in sample order; at 100k
//     samples the result differs from the exact value by up to ~6e-5 relative, so the rounding sequence must be
//     reproduced.  Two implementations live here:
//       - round 2 (default): one WAVE per read.  seqsum.h evaluates the sequential sum exactly, 1024 terms at a time
//         (surrogate starts in the sum's binade, parity maps, binade crossings repaired natively): k_stat_wave,
//         k_adaptor_wave, k_jnn_wave, k_polya_wave, with the reads dispatched longest first (launch_order);
//       - round 1 (SGK_LANE_PER_READ=1, and find_polya on large uniform batches): one read per LANE, serial float
//         chain, the 64 reads of a wave streamed through the LDS row stager (row_stream.h): k_moments, k_jnn, k_adaptor,
//         k_polya.  Kept as the independent second implementation the tests compare against, bit for bit.
//   * medians are order statistics (rank n/2, src/stat.h:56-73 + ksort.h:233-259).  For the int16 median any exact
//     selection works -> a histogram with one bin per raw value over a window centred on the read's mean (k_stat_wave:
//     2048 bins per wave, fused into its second pass; k_median: 8192 bins per 256-thread workgroup), a two-level radix
//     select for regions and for reads whose order statistic falls outside the window.  The pA median is
//     pA(raw order statistic) because the int16 -> pA map is monotone (non-increasing when range/digitisation < 0) --
//     EXCEPT where pA values compare equal without being the same bits (+0 / -0: a unit of 0, products that underflow)
//     or do not order (NaN: a unit or offset that is not finite): there it is the element the reference's own
//     exchanges leave at n/2.  Such a median is a zero or comes with a non-finite scale; k_median_literal
//     (stat_literal.hip, median_literal.h) finds those records behind the other kernels and redoes them literally.
//   * jnn_core (src/jnn.c:190-278) and jnnv2 (src/jnn.c:99-179) are serial automata with thresholds derived from those
//     sequential float moments.  Their per-sample work is integer: in / out-of-range flags of the raw samples, integer
//     rolling totals with the exact constant division (tstat_math.h) and integer thresholds for jnnv2's run finder.
//     Wave-per-read forms: jnn_core in 64 chunks between data-determined sync points, from event to event on 32-bit
//     masks (jnn_chunks); jnnv2's run finder from threshold flip to flip (k_adaptor_wave).
//
// Where what lives.  Three paths, each in a translation unit of its own, selected per batch by stat_launch.hip:
//   stat_lane.hip   one read per LANE (round 1) on row_stream.h: k_moments, k_median, k_jnn, k_polya, k_adaptor.  It
//                   includes neither seqsum.h nor stat_wave.h: it is the independent second implementation.
//   stat_wave.hip   one read per WAVE on seqsum.h: k_stat_wave, k_jnn_wave, k_polya_wave, k_adaptor_wave, and the sort
//                   that hands them the reads longest first (k_order_*).
//   stat_long.hip   a long read on 64 waves: k_long_list, k_long_limit, k_long_chains and the long reads' workspace.
//   stat_literal.hip  k_median_literal, behind all three.
//   stat_wave.h     the wave-per-read building blocks, shared by stat_wave.hip and stat_long.hip (never by the lanes).
//   stat_device.h   (this file) what all three share: regions, the long reads' hand-over, the clamps and the automata
//                   and thresholds of the reference that both implementations must state the same way.  k_jnn_f32 of
//                   shims.hip uses its JnnAuto as well.
//   statf_kernels.hip, jnnf_kernels.hip  stat and jnn on batches of FLOAT reads (sgk_stat_f32, sgk_jnn_f32), one read per
//                   wave on float_reads.h; they use seqsum.h, the automata of this file and jnn_chunks_src / the merge of
//                   stat_wave.h, and have their own entry points: nothing of the int16 paths goes through them.  The
//                   float stat shims of shims.hip are a batch of one read on statf_kernels.hip.
//   stat_launch.hip the lane / wave rule and the launchers; it holds no kernel and launches them through the
//                   launch_k_* functions of stat_args.h, one per kernel, each defined next to its kernel.
#pragma once
#include "sgk_common.h"
#include "stat_args.h"
#include "tstat_math.h"

namespace sgk {

// region of read r a kernel works on (absolute sample index + length)
struct Region {
    int64_t start;
    int64_t len;
};
__device__ inline Region get_region(int mode, const sgk_batch_t &b, const sgk_prefix_rec_t *prec, uint32_t r) {
    Region g;
    g.start = (int64_t)b.offsets[r];
    g.len = (int64_t)b.lengths[r];
    if (mode == REG_ADAPT) {
        const sgk_prefix_rec_t p = prec[r];
        if (p.adapt_y > 0) { g.start += p.adapt_x; g.len = (int64_t)p.adapt_y - p.adapt_x; }
        else g.len = 0;
    } else if (mode == REG_POLYA) {
        const sgk_prefix_rec_t p = prec[r];
        if (p.adapt_y > 0 && p.polya_y > 0) { g.start += (int64_t)p.polya_x + p.adapt_y; g.len = (int64_t)p.polya_y - p.polya_x; }
        else g.len = 0;
    } else if (mode == REG_TAIL) {  // pA[adapt_y .. n), find_polya's input (cfunc.c:186-191)
        const sgk_prefix_rec_t p = prec[r];
        if (p.adapt_y > 0) { g.start += p.adapt_y; g.len -= p.adapt_y; }
        else g.len = 0;
    }
    if (g.len < 0) g.len = 0;
    return g;
}

// what the workgroups of a long read exchange is written and read with agent-scope atomics
__device__ __forceinline__ uint32_t lc_ld(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long lc_ld(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void lc_st(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void lc_st(unsigned long long *p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The record of read r if k_long_list listed it (wave-uniform; null: an ordinary read).  k_long_chains may run BESIDE the
// kernel that asks (stat, jnn: side stream), so who does a read is decided by what k_long_list wrote -- LongSums::rec_off,
// final before either kernel starts -- and never by LongSums::valid, which k_long_chains sets when it is done (prefix'
// k_adaptor_wave, launched behind it, reads the sums under valid).
__device__ inline const LongSums *find_long(const StatArgs &a, uint32_t r, int64_t len) {
    if (!a.longs || len < (int64_t)a.long_min) return nullptr;
    const uint32_t nl = a.long_hdr->n_long, n = nl < LC_CAP ? nl : LC_CAP;
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t i = i0 + (uint32_t)lane_id();
        const unsigned long long hit = __ballot(i < n && a.long_list[i] == r);
        if (hit) {
            return a.longs + i0 + (uint32_t)(__ffsll((long long)hit) - 1);
        }
    }
    return nullptr;
}

// The redo launch of a wave kernel (StatArgs::long_redo): wave widx looks at entry widx of the long list and takes its
// read iff k_long_chains declined it (a barrier of its workgroups timed out, lc_barrier).  Usually none: every wave
// returns at once.
__device__ inline bool long_redo_read(const StatArgs &a, uint32_t widx, uint32_t &r) {
    if (!a.longs) return false;
    const uint32_t nl = a.long_hdr->n_long, n = nl < LC_CAP ? nl : LC_CAP;
    if (widx >= n) return false;
    if (a.longs[widx].rec_off == LC_NO_REC || a.long_work[widx].failed == 0u) return false;
    r = a.long_list[widx];
    if (lane_id() == 0) atomicAdd(&a.long_hdr->n_declined, 1u);
    return true;
}

__device__ inline float clampf_raw(int16_t v) {  // rm_outlier, src/jnn.c:61-77
    return v > 1200 ? 1200.0f : (v < 0 ? 0.0f : (float)v);
}
__device__ inline int clampi_raw(int16_t v) {  // rm_outlier as an integer (the float it yields is that integer)
    return v > 1200 ? 1200 : (v < 0 ? 0 : (int)v);
}
__device__ inline float clampf_pa(float v) {     // rm_outlierf, src/jnn.c:79-95
    return v > 1200.0f ? 1200.0f : (v < 0.0f ? 0.0f : v);
}

// two samples per packed 16-bit instruction: the outlier clamp of rm_outlier (src/jnn.c:61-77)
typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ s16x2 clamp_raw2(uint32_t w) {
    s16x2 v = __builtin_bit_cast(s16x2, w);
    v = __builtin_elementwise_max(v, (s16x2){0, 0});
    return __builtin_elementwise_min(v, (s16x2){1200, 1200});
}

// (sgk_stat_rec_t::reserved / sgk_prefix_rec_t::reserved between kernels: reads whose median is still to be found)
constexpr uint32_t FLAG_MEDIAN_WHOLE = 1u, FLAG_MEDIAN_ADAPT = 1u, FLAG_MEDIAN_POLYA = 2u;
// (what a record KEEPS: a pA median that is a pick among equal-comparing values and could not be redone, median_literal.h)
constexpr uint32_t FLAG_MEDIAN_INEXACT = SGK_MEDIAN_INEXACT, FLAG_MEDIAN_INEXACT_POLYA = SGK_MEDIAN_INEXACT_POLYA;

// ---------------------------------------------------------------- jnn_core automaton (src/jnn.c:190-278)
struct JnnAuto {
    float top, bot, first_min;
    int window, error, seg_dist;
    int hi_i, lo_i;  // integer form of the thresholds for integer-valued samples: in  <=>  lo_i < iv < hi_i
    int first_min_i; // (float)c >= first_min  <=>  c >= first_min_i
    int keep_min;    // an ended segment is kept iff c >= keep_min
    int open_m;      // -1 while a segment is open, else 0 (all predicates are kept as 0 / -1 lane masks)
    int err, run_err, c, w, start, nseg, last_x, last_y;
    __device__ void init(float top_, float bot_, int corrector, int seg_dist_, int window_, float stall_len, int error_) {
        top = top_; bot = bot_; window = window_; error = error_; seg_dist = seg_dist_;
        first_min = (float)window_ * stall_len;
        first_min_i = (int)ceilf(first_min);
        keep_min = first_min_i < window_ ? first_min_i : window_;  // c >= window || (nseg == 0 && c >= first_min_i)
        // v < top <=> iv < ceil(top), v > bot <=> iv > floor(bot) for an integer iv in [0, 1200]; NaN thresholds
        // compare false with everything
        hi_i = (top_ != top_) ? -0x40000000 : (top_ > 4000.0f ? 4000 : (top_ < -4.0f ? -4 : (int)ceilf(top_)));
        lo_i = (bot_ != bot_) ? 0x40000000 : (bot_ > 4000.0f ? 4000 : (bot_ < -4.0f ? -4 : (int)floorf(bot_)));
        open_m = 0; err = 0; run_err = 0; c = 0; w = corrector; start = 0; nseg = 0; last_x = 0; last_y = 0;
    }
    // in-range test of a clamped raw sample as a lane mask (no compare -> scalar-mask -> select round trips)
    __device__ __forceinline__ int in_mask_raw(int iv) const { return ((iv - hi_i) & (lo_i - iv)) >> 31; }
    __device__ __forceinline__ int in_mask_f(float v) const { return ((v < top) & (v > bot)) ? -1 : 0; }

    // One sample of jnn_core (src/jnn.c:213-271).  emit(k, x, y) is called when segment k can no longer change.
    // The lanes of a wave run different reads, and a lone wave spends its time waiting on dependent
    // compare -> SGPR -> select chains, so the per-sample bookkeeping is integer mask algebra on the vector
    // unit (0 / -1 masks, "x - mask" adds one); one wave-level test guards the two rare events (the c % w
    // correction and the end of a segment).
    template <typename E>
    __device__ __forceinline__ void step(int i, int in, E emit) {
        const int opn = open_m;
        const int errlt = (err - error) >> 31;           // err < error
        const int tol = ~in & opn & errlt;               // tolerated out-of-range sample
        const int rest = ~in & opn & ~errlt;             // the segment ends (closed or abandoned)
        const int cnt = in | tol;
        const int opening = in & ~opn;
        start = (opening & i) | (~opening & start);
        const int c1 = c - cnt;
        const int w1 = w - in;
        int err1 = err - tol;
        run_err = (run_err - tol) & ~in;
        // "if (c >= window && c >= w && c % w == 0) err--" (jnn.c:228, 238): c >= w needs more tolerated
        // samples in the segment than in-range samples before it
        // cheap necessary conditions, evaluated on every sample: c1 >= w1 for the correction, and for keeping an
        // ended segment c >= keep_min (= window, or min(window, first_min_i) while no segment has been kept yet)
        const int fix = cnt & ((w1 - 1 - c1) >> 31);
        const int keep = rest & ((keep_min - 1 - c) >> 31);
        if (__any((fix | keep) != 0)) {
            if (fix && c1 >= window) {
                if ((c1 % w1) == 0) --err1;
            }
            if (keep) {
                const int end = i - run_err;
                if (nseg > 0 && start - last_y < seg_dist) {
                    last_y = end;
                } else {
                    if (nseg > 0) emit(nseg - 1, last_x, last_y);
                    last_x = start; last_y = end;
                    ++nseg;
                }
                keep_min = window;  // "first segment" rule (jnn.c:243) no longer applies
            }
        }
        open_m = (open_m | in) & ~rest;
        c = c1 & ~rest;
        err = err1 & ~rest;
        run_err &= ~rest;
        w = w1;
    }
    template <typename E>
    __device__ void finish(E emit) {
        if (nseg > 0) emit(nseg - 1, last_x, last_y);
    }
};

// integer form of jnn_core's range test for thresholds top / bot (JnnAuto::init above), on the UNCLAMPED sample:
// lo_i < clamp(v) < hi_i  <=>  lo_r < v < hi_r; keep_min: the shortest segment that can matter
struct JnnThr {
    int hi_r, lo_r, keep_min;
};
__device__ __forceinline__ JnnThr jnn_thresholds(float top, float bot, const JnnP &p) {
    const int hi_i = (top != top) ? -0x40000000 : (top > 4000.0f ? 4000 : (top < -4.0f ? -4 : (int)ceilf(top)));
    const int lo_i = (bot != bot) ? 0x40000000 : (bot > 4000.0f ? 4000 : (bot < -4.0f ? -4 : (int)floorf(bot)));
    JnnThr t;
    t.hi_r = hi_i <= 0 ? -40000 : (hi_i > 1200 ? 40000 : hi_i);
    t.lo_r = lo_i >= 1200 ? 40000 : (lo_i < 0 ? -40000 : lo_i);
    const int first_min_i = (int)ceilf((float)p.window * p.stall_len);  // (float)c >= window * stall_len
    t.keep_min = first_min_i < p.window ? first_min_i : p.window;
    return t;
}

// ---------------------------------------------------------------- find_adaptor / jnnv2 (src/jnn.c:99-188)
constexpr int ADW = 2000;  // jnnv2 window (both presets, src/jnn.h:84-98)

// rolling_window's t_i = tt / w (src/jnn.c:20-56).  tt is a float holding an exact integer (< 2000*1200 < 2^24),
// so it is carried as an int here; the division by the constant 2000 is the correctly rounded three-operation
// form of tstat_math.h (verified exhaustively for every float >= 2^-100 by oracle/verify_math.cpp).
__device__ __forceinline__ float roll_mean(int tot) { return sgk_div_f32<ADW>((float)tot); }

// smallest integer total whose rolling mean is >= x (resp. > x): roll_mean is non-decreasing in tot, so
// the run finder's float comparisons t < bot / t > bot (src/jnn.c:139-163) become integer comparisons
// tot < T_lt / tot >= T_gt.  Binary search over [0, 2000*1200].
// Where the window comes from (the window source of roll_threshold and adaptor_find): WinPreset is the constant 2000 of
// both presets with the constant division above; WinParam (k_adaptor_param, stat_param.hip) holds a caller's window, 2 ..
// 13 981, and divides at run time -- the library is built with -fhip-fp32-correctly-rounded-divide-sqrt, which makes
// the f32 `/` the correctly rounded IEEE quotient (tot <= 1200 * 13 981 <= 2^24 and the window are exact in f32, the
// quotient is 0 or a normal number); tests/test_gpu_segmenter_params.py runs it for every total of every tested window.
struct WinPreset {
    __device__ __forceinline__ int w() const { return ADW; }
    __device__ __forceinline__ float mean(int tot) const { return roll_mean(tot); }
};
struct WinParam {
    int win;
    float winf;
    __device__ __forceinline__ int w() const { return win; }
    __device__ __forceinline__ float mean(int tot) const { return (float)tot / winf; }
};
template <typename WS = WinPreset>
__device__ inline int roll_threshold(float x, bool strict, const WS ws = WS{}) {
    if (x != x) return strict ? 0x7fffffff : 0;  // NaN threshold: no t is < or > it
    int lo = 0, hi = ws.w() * 1200 + 1;  // answer in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const float t = ws.mean(mid);
        const bool ok = strict ? (t > x) : (t >= x);   // NaN x: never ok -> hi stays -> nothing is >= / > x
        if (ok) hi = mid; else lo = mid + 1;
    }
    return lo;
}

}  // namespace sgk
