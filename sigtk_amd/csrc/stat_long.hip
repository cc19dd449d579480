// stat_long.hip -- the long-read path: the sequential sums of a read of long_min samples or more on 64 wavefronts
// (k_long_chains), the list of such reads (k_long_list, k_long_limit) and their workspace (prepare_long).  It evaluates
// single tiles with the wave-per-read routines of stat_wave.h and hands reads over to / takes them from the kernels of
// stat_wave.hip through LongSums (find_long, long_redo_read in stat_device.h).  Must not include row_stream.h.
#include "stat_wave.h"

namespace sgk {

// ---------------------------------------------------------------- long reads: the sequential sums on 64 wavefronts
// A wave evaluates a sequential float sum at ~1 000 terms per microsecond; a read of 3 000 000 samples keeps its wave
// busy for milliseconds per sum while the rest of the batch is long done.  k_long_chains gives such a read LC_PARTS
// workgroups of four wavefronts (on LC_PARTS compute units: the sums are bound by vector-instruction issue, one compute
// unit's four SIMDs would not do).  What seqsum.h does with the 16 terms of a lane is done here once more with the 1 024
// terms of a TILE (tools/proto/seqsum_tiles_proto.py is the numpy model, seqsum_segments_proto.py the round-3 sketch it
// grew from):
//
//   level 1, all waves, no dependency between them: a wave owns a contiguous run of tiles.  It PREDICTS the accumulator
//     in front of each tile (sums of the terms in front of its run, pass A below, then tile by tile from its own
//     summaries), takes the binade E of the prediction, and summarises the tile for that binade: T0 / T1, the
//     increment of the accumulator's significand over the tile's 1 024 terms when it enters the tile even / odd (lanes'
//     surrogate walks, parity maps composed across the lanes, once per entering parity).  8 bytes per tile and sum in
//     the workspace.  Tiles the argument does not cover (surrogates left the binade, a negative term, tile 0 with its
//     native head) are marked instead.
//   level 2, one wave per sum, 64 tiles per step: the summaries are composed exactly as ss_fast composes lanes -- parity
//     maps by the segmented xor scan, increments by a sum scan, S + total <= 2^24 certifies that the true sum stayed in
//     the binade.  A tile whose binade was predicted wrongly (E differs from the true accumulator's), in which the sum
//     leaves its binade, or that is marked, is evaluated from the TRUE accumulator with the wave kernels' own tile
//     routine (ss_tile1 / roll_chain_tile): about log2(n / 256) + a few tiles per sum.
//
// Nothing is speculative in the result: a wrong prediction costs a tile evaluation, never a wrong bit.  The workgroups
// of a read meet at barriers on a counter in the workspace (three per stage); everything they exchange is written and
// read with agent-scope atomics (the L2s of the eight XCDs are not coherent for ordinary accesses).  A read's workgroups
// are neighbours in the grid and the grid is small enough to be resident at once, so nobody waits for a workgroup that
// cannot start.  The four (stat), two (jnn, prefix) sums of a read land in LongSums; k_stat_wave / k_jnn_wave /
// k_adaptor_wave pick them up (find_long) and walk the read only for the histogram / pA output, the automaton (already
// 64 chunks wide), the run finder.
constexpr uint32_t LC_VALID = 0x00800000u;

template <int C>
struct Ix {
    static constexpr int v = C;
};
__device__ __forceinline__ double wave_sum_d(double v) { return wave_last_d(wave_incl_scan_d(v)); }
__device__ __forceinline__ int wave_sum_i(int v) { return wave_last_i(wave_incl_scan_i(v)); }
struct LcCtx {
    LongWork *w;
    LongHdr *hdr;
    unsigned long long *rec[2];  // tile records of the two sums: T0 | (E << 24 | LC_VALID | (T1 - T0 + 0x8000) & 0xffff) << 32
    uint32_t phase;              // barriers passed
    int part;                    // this workgroup's index among the read's LC_PARTS
    uint32_t fault;              // StatArgs::long_fault
};
// All workgroups of the read; what they wrote with lc_st before is readable with lc_ld behind it.  Returns false when
// the read is DECLINED: this workgroup waited in vain (the bound -- seconds -- keeps a GPU that does not dispatch a
// grid's workgroups in order, or shares its slots with something that does not end, from hanging) or another one of the
// read did and said so in LongWork::failed.  Every workgroup then leaves the read without writing anything of the
// subtool's output (all of it is written behind a read's LAST barrier: whoever passes that one has seen all LC_PARTS
// arrive, so what it writes is right even if a late workgroup flagged the read meanwhile), and the redo launch of the
// wave kernel (StatArgs::long_redo, behind the join) takes the read on one wavefront -- the path of every read before
// round 4.  The event chain treats a timeout the same way (event_seg.hip, chain_segment).
// long_fault (tests only, sgk_stat_options_t::debug_fault): 1 | part << 8 | phase << 16: workgroup `part` never arrives
// at barrier `phase` (1-based) and the spin bound is 2^12; 2 | bound << 8: that spin bound, nobody withheld.
__device__ inline bool lc_barrier(LcCtx &cx) {
    __shared__ uint32_t s_fail;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    ++cx.phase;
    if (threadIdx.x == 0) {
        uint32_t fail = 0u, bound = 1u << 24;
        const uint32_t mode = cx.fault & 0xffu;
        if (mode == 1u) bound = 1u << 12;
        else if (mode == 2u) bound = (cx.fault >> 8) ? (cx.fault >> 8) : 1u;
        if (mode == 1u && (uint32_t)cx.part == ((cx.fault >> 8) & 0xffu) && cx.phase == ((cx.fault >> 16) & 0xffu)) {
            lc_st(&cx.w->failed, 1u);  // (the withheld workgroup: it leaves, the others find out)
            fail = 1u;
        } else {
            atomicAdd(&cx.w->arrive, 1u);
            const uint32_t target = cx.phase * (uint32_t)LC_PARTS;
            uint32_t spins = 0u;
            while (lc_ld(&cx.w->arrive) < target) {
                if (lc_ld(&cx.w->failed)) { fail = 1u; break; }
                __builtin_amdgcn_s_sleep(2);
                if (++spins >= bound) {
                    lc_st(&cx.w->failed, 1u);
                    atomicAdd(&cx.hdr->n_timeout, 1u);
                    fail = 1u;
                    break;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        s_fail = fail;
    }
    __syncthreads();
    return s_fail == 0u;  // (the next barrier's leading __syncthreads orders this read before the next write)
}

// level 1: the summary of one tile for the binade of the predicted accumulator mt; tsum: (about) the sum of its terms
template <typename TF>
__device__ __forceinline__ unsigned long long lc_summary(const TF &tf, double mt, bool force_mark, double &tsum) {
    const uint32_t mb = ss_bits(ss_uniform((float)mt));
    const uint32_t ex = (mb >> 23) & 0xffu;
    const bool ok = !(mb >> 31) && ex >= 27u && ex <= 227u && !force_mark;
    const uint32_t b0 = ((ok ? ex : 127u) << 23) | 0x400000u, b1 = b0 + 1u;
    SsWalk w = {ss_float(b0), ss_float(b1), 0u};
    ss_walk_terms<0, true>(w, tf);
    const uint32_t c0 = ss_bits(w.a0), c1 = ss_bits(w.a1);
    const uint32_t bad = (((c0 ^ b0) | (c1 ^ b1)) >> 23) | (w.neg >> 31);
    if (!ok || __any(bad != 0u)) {
        float v = 0.0f;
        ss_native_terms<0>(v, tf.with(ss_opaque_zero()));
        tsum = wave_sum_d((double)v);
        return 0ull;
    }
    const int f0 = (int)(c0 - b0), f1 = (int)(c1 - b1);
    int T0, T1;
    if (__any(f0 != f1)) {  // some lane met a tie: the tile's increment depends on the parity it is entered with
        const int s0 = __builtin_amdgcn_inverse_ballot_w64(ss_parity_in(f0, f1, 0)) ? f1 : f0;
        const int s1 = __builtin_amdgcn_inverse_ballot_w64(ss_parity_in(f0, f1, 1)) ? f1 : f0;
        T0 = wave_sum_i(s0);
        T1 = wave_sum_i(s1);
    } else T0 = T1 = wave_sum_i(f0);
    tsum = (double)T0 * (double)ss_float((ex - 23u) << 23);
    const uint32_t hi = (ex << 24) | LC_VALID | ((uint32_t)(T1 - T0 + 0x8000) & 0xffffu);
    return ((unsigned long long)hi << 32) | (uint32_t)T0;
}

// level 2: the accumulator m taken through tiles [0, nt) (records rec[0 .. nt)); eval(tile, m) evaluates one tile from
// the true accumulator.  One wave.
template <typename EVAL>
__device__ inline float lc_compose(float m, const unsigned long long *rec, int nt, uint32_t &n_true, EVAL eval) {
    const int lane = lane_id();
    for (int g0 = 0; g0 < nt; g0 += 64) {
        const int gn = nt - g0 < 64 ? nt - g0 : 64;
        const unsigned long long rc = lane < gn ? lc_ld(rec + g0 + lane) : 0ull;
        const uint32_t rhi = (uint32_t)(rc >> 32);
        const int t0 = (int)(uint32_t)rc, t1 = t0 + (int)(rhi & 0xffffu) - 0x8000;
        int skip = 0;
        while (skip < gn) {
            m = ss_uniform(m);
            const uint32_t mb = ss_bits(m);
            const uint32_t ex = (mb >> 23) & 0xffu;
            const bool live = lane >= skip && lane < gn;
            // (a record carries a binade in 27 .. 227 or is marked: a negative, tiny, huge or non-finite m matches none)
            const bool okl = live && !(mb >> 31) && (rhi & LC_VALID) && (rhi >> 24) == ex;
            const unsigned long long badm = __ballot(live && !okl);
            const int fb = badm ? (int)__builtin_amdgcn_readfirstlane(__ffsll((long long)badm) - 1) : gn;
            int fail = fb;
            if (fb > skip) {
                const int S = (int)((mb & 0x7fffffu) | 0x800000u);
                const bool in = lane >= skip && lane < fb;
                const int f0 = in ? t0 : 0, f1 = in ? t1 : 0;  // (other lanes: the identity map)
                int f = f0;
                if (__any(f0 != f1)) f = __builtin_amdgcn_inverse_ballot_w64(ss_parity_in(f0, f1, S)) ? f1 : f0;
                // a tile's increment is below 2^23 + 2^10, 64 of them overflow no int; the comparison is done in 64 bits
                const long long incl = (long long)wave_incl_scan_i(f);
                const unsigned long long cm = __ballot(in && (long long)S + incl > (1ll << 24));
                if (cm) fail = (int)__builtin_amdgcn_readfirstlane(__ffsll((long long)cm) - 1);
                if (fail > skip) {
                    const int tot = __builtin_amdgcn_readlane((int)incl, fail - 1);
                    m = (float)(S + tot) * ss_float((ex - 23u) << 23);
                }
            }
            if (fail >= gn) break;
            m = eval(g0 + fail, m);
            ++n_true;
            skip = fail + 1;
        }
    }
    return m;
}

// One stage (one or two sums over the same tiles) of a long read.  SRC supplies the tiles:
//   NCH                      sums per stage
//   seek(t) / ahead(t, te) / next()   streaming: position at tile t; issue the loads of tile t + 1 (< te); step
//   terms(t, f)              calls f(Ix<c>, term functor of sum c) for the current tile, c = 0 .. NCH - 1; the functors
//                            mask what lies outside the region and carry the sum's orientation
//   eval(c, t, m)            sum c's tile t from the true (oriented) accumulator m
//   flip(c) / negated(c)     from now on sum c runs on the negated terms / does it?
//   pass_a(t) / pass_b(t) / end_b()   what else the subtool does with the current tile in either pass, and once per
//                            workgroup behind pass B (stat: pA output; window histogram)
// Returns the SIGNED sums in out[]; false: the read is declined (lc_barrier), out[] means nothing.  Every wave of the
// read's LC_PARTS workgroups calls it (barriers inside).
template <typename SRC>
__device__ inline bool lc_stage(SRC &src, LcCtx &cx, int ntiles, float (&out)[2], uint32_t &n_true_out) {
    constexpr int N = SRC::NCH;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = lane_id();
    const int gw = cx.part * LC_WG_WAVES + wv;  // this wave among the read's LC_WAVES
    const int per = (ntiles + LC_WAVES - 1) / LC_WAVES;
    const int ta = gw * per < ntiles ? gw * per : ntiles, te = ta + per < ntiles ? ta + per : ntiles;
    // ---- pass A: the sum of the terms of this wave's tiles (a double per lane; the prediction needs no more)
    double acc[N];
#pragma unroll
    for (int c = 0; c < N; ++c) acc[c] = 0.0;
    if (ta < te) {
        src.seek(ta);
        for (int t = ta; t < te; ++t) {
            src.ahead(t, te);
            src.terms(t, [&](auto ix, const auto &tf) {
                constexpr int c = decltype(ix)::v;
                float v = 0.0f;
                ss_native_terms<0>(v, tf);
                acc[c] += (double)v;
            });
            src.pass_a(t);
            src.next();
        }
    }
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const double tot = wave_sum_d(acc[c]);
        if (lane == 0) lc_st(&cx.w->seg_tot[gw][c], (unsigned long long)__double_as_longlong(tot));
    }
    if (!lc_barrier(cx)) return false;
    // the sum is oriented by the sign of the read's total (as the wave kernels orient it by the sign of the
    // accumulator): non-negative terms are what the summaries cover
    double mt[N];
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const double v = __longlong_as_double((long long)lc_ld(&cx.w->seg_tot[lane][c]));  // (LC_WAVES == 64 lanes)
        const double before = wave_sum_d(lane < gw ? v : 0.0), all = wave_sum_d(v);
        if (all < 0.0) { src.flip(c); mt[c] = -before; }
        else mt[c] = before;
    }
    // ---- pass B: the tiles' summaries
    if (ta < te) {
        src.seek(ta);
        for (int t = ta; t < te; ++t) {
            src.ahead(t, te);
            src.terms(t, [&](auto ix, const auto &tf) {
                constexpr int c = decltype(ix)::v;
                double ts;
                const unsigned long long rc = lc_summary(tf, mt[c], t == 0, ts);
                if (lane == 0) lc_st(cx.rec[c] + t, rc);
                mt[c] += ts;
            });
            src.pass_b(t);
            src.next();
        }
    }
    src.end_b();
    if (!lc_barrier(cx)) return false;
    // ---- level 2: wave c of the read's first workgroup composes sum c
    if (cx.part == 0 && wv < N) {
        uint32_t n_true = 0u;
        const float m = lc_compose(0.0f, cx.rec[wv], ntiles, n_true, [&](int t, float mm) { return src.eval(wv, t, mm); });
        if (lane == 0) {
            lc_st(reinterpret_cast<uint32_t *>(&cx.w->m[wv]), ss_bits(m));
            atomicAdd(&cx.w->n_true, n_true);
        }
    }
    if (!lc_barrier(cx)) return false;
#pragma unroll
    for (int c = 0; c < N; ++c) out[c] = ss_signed(ss_float(lc_ld(reinterpret_cast<const uint32_t *>(&cx.w->m[c]))), src.negated(c));
    n_true_out = lc_ld(&cx.w->n_true);
    return true;
}

// ---- the tile sources
struct SrcTiles {  // streaming of the raw tiles of a region
    WaveRead wr;
    WaveTile cur, nxt;
    __device__ __forceinline__ void seek(int t) { wr.load(cur, t); }
    __device__ __forceinline__ void ahead(int t, int te) { if (t + 1 < te) wr.load(nxt, t + 1); }
    __device__ __forceinline__ void next() { cur = nxt; }
    __device__ __forceinline__ void pass_a(int) {}
    __device__ __forceinline__ void pass_b(int) {}
    __device__ __forceinline__ void end_b() {}
    template <typename F>
    __device__ __forceinline__ void bases(int t, F f) const {  // f(TermBase) for the current tile
        const int q0 = lane_id() * SS_SPL;
        int q_lo, q_hi;
        wr.range(t, 0, q_lo, q_hi);
        if (wr.interior(t)) f(TermBase<true>{cur, q0, q_lo, q_hi, 0u});
        else f(TermBase<false>{cur, q0, q_lo, q_hi, 0u});
    }
};
struct SrcStatSums : SrcTiles {  // stat, stage 1: raw and pA (src/stat.h:17-33)
    static constexpr int NCH = 2;
    Scale sc;
    int sraw;   // -1: the raw chain runs negated
    float sg;   // the pA chain's orientation times the sign of the unit (as in k_stat_wave)
    float *pa_dst;  // fused stat + pa: the pA array at the region's base (or null)
    __device__ void init(const sgk_batch_t &b, const Region &g, const Scale &s, float *pa_out) {
        wr.init(b, g); sc = s; sraw = 0; sg = s.unit < 0.0f ? -1.0f : 1.0f;
        pa_dst = pa_out ? pa_out + wr.rb : nullptr;
    }
    __device__ __forceinline__ void pass_a(int t) { if (pa_dst) pa_write_tile(wr, t, sc, pa_dst); }
    __device__ __forceinline__ void flip(int c) { if (c == 0) sraw = ~sraw; else sg = -sg; }
    __device__ __forceinline__ bool negated(int c) const { return c == 0 ? sraw != 0 : sg < 0.0f; }
    template <typename F>
    __device__ __forceinline__ void terms(int t, F f) const {
        const Scale so = {sc.offf, sc.unit * sg};
        bases(t, [&](auto b) {
            f(Ix<0>{}, TermRaw<decltype(b)::interior>{b, sraw});
            f(Ix<1>{}, TermPa<decltype(b)::interior>{b, so});
        });
    }
    __device__ __attribute__((noinline)) float eval(int c, int t, float m) const {
        WaveTile x;
        wr.load(x, t);
        const Scale so = {sc.offf, sc.unit * sg};
        if (c == 0) ss_tile1<true>(m, wr, x, t, [&](auto b) { return TermRaw<decltype(b)::interior>{b, sraw}; });
        else ss_tile1<true>(m, wr, x, t, [&](auto b) { return TermPa<decltype(b)::interior>{b, so}; });
        return m;
    }
};
struct SrcStatDevs : SrcTiles {  // stat, stage 2: squared deviations (src/stat.h:36-54)
    static constexpr int NCH = 2;
    Scale sc;
    float mraw, mpa;
    int lo;            // window histogram: first raw value
    uint32_t *hist;    // this workgroup's (LDS, zeroed)
    uint32_t *ghist;   // the read's (workspace, zeroed): the workgroups add theirs
    __device__ __forceinline__ void pass_b(int t) {
        int q_lo, q_hi;
        wr.range(t, 0, q_lo, q_hi);
        if (wr.interior(t)) hist_tile<true>(cur, q_lo, q_hi, lo, hist);
        else hist_tile<false>(cur, q_lo, q_hi, lo, hist);
    }
    __device__ __forceinline__ void end_b() {
        __syncthreads();
        for (int i = (int)threadIdx.x; i < WH_BINS; i += LC_WG_WAVES * 64) {
            const uint32_t h = hist[i];
            if (h) atomicAdd(&ghist[i], h);
        }
    }
    __device__ __forceinline__ void flip(int) {}
    __device__ __forceinline__ bool negated(int) const { return false; }
    template <typename F>
    __device__ __forceinline__ void terms(int t, F f) const {
        bases(t, [&](auto b) {
            f(Ix<0>{}, TermDevRaw<decltype(b)::interior>{b, mraw});
            f(Ix<1>{}, TermDevPa<decltype(b)::interior>{b, sc, mpa});
        });
    }
    __device__ __attribute__((noinline)) float eval(int c, int t, float m) const {
        WaveTile x;
        wr.load(x, t);
        if (c == 0) ss_tile1<false>(m, wr, x, t, [&](auto b) { return TermDevRaw<decltype(b)::interior>{b, mraw}; });
        else ss_tile1<false>(m, wr, x, t, [&](auto b) { return TermDevPa<decltype(b)::interior>{b, sc, mpa}; });
        return m;
    }
};
template <bool DEV>
struct SrcClamp : SrcTiles {  // jnn: rm_outlier(raw), then its squared deviations (src/jnn.c:195-199)
    static constexpr int NCH = 1;
    float mean;
    __device__ __forceinline__ void flip(int) {}
    __device__ __forceinline__ bool negated(int) const { return false; }
    template <typename B>
    __device__ __forceinline__ auto term(B b) const {
        if constexpr (DEV) return TermDevClamp<B::interior>{b, mean};
        else return TermClamp<B::interior>{b};
    }
    template <typename F>
    __device__ __forceinline__ void terms(int t, F f) const {
        bases(t, [&](auto b) { f(Ix<0>{}, term(b)); });
    }
    __device__ __attribute__((noinline)) float eval(int, int t, float m) const {
        WaveTile x;
        wr.load(x, t);
        ss_tile1<false>(m, wr, x, t, [&](auto b) { return term(b); });
        return m;
    }
};
template <bool DEV>
struct SrcRoll {  // jnnv2: the rolling means of ADW clamped samples, then their squared deviations (src/jnn.c:106-124)
    static constexpr int NCH = 1;
    WaveRead wr;  // region: the windows' first samples
    float mean;
    int T0;
    WaveTile tr, ld, trn, ldn;
    __device__ __forceinline__ void flip(int) {}
    __device__ __forceinline__ bool negated(int) const { return false; }
    __device__ __forceinline__ float term(int v) const {
        if constexpr (DEV) { const float d = roll_mean(v) - mean; return d * d; }
        else return roll_mean(v);
    }
    __device__ __forceinline__ void seek(int t) {
        T0 = window_total(wr, t, t == 0 ? wr.skip : 0);
        roll_load(wr, tr, ld, t);
    }
    __device__ __forceinline__ void ahead(int t, int te) { if (t + 1 < te) roll_load(wr, trn, ldn, t + 1); }
    __device__ __forceinline__ void next() { tr = trn; ld = ldn; }
    __device__ __forceinline__ void pass_a(int) {}
    __device__ __forceinline__ void pass_b(int) {}
    __device__ __forceinline__ void end_b() {}
    __device__ __forceinline__ void totals(const WaveTile &a, const WaveTile &b, int t, int &T, int (&tot)[SS_SPL]) const {
        if (t == 0 && wr.skip > 0) roll_tile<true>(a, b, wr.skip, T, tot);
        else roll_tile<false>(a, b, 0, T, tot);
    }
    template <typename F>
    __device__ __forceinline__ void terms(int t, F f) {
        int tot[SS_SPL];
        totals(tr, ld, t, T0, tot);
        const int q0 = lane_id() * SS_SPL;
        int q_lo, q_hi;
        wr.range(t, 0, q_lo, q_hi);
        float x[SS_SPL];
#pragma unroll
        for (int e = 0; e < SS_SPL; ++e) x[e] = (q0 + e >= q_lo && q0 + e < q_hi) ? term(tot[e]) : 0.0f;
        f(Ix<0>{}, TermArr{x});
    }
    __device__ __attribute__((noinline)) float eval(int, int t, float m) const {
        int T = window_total(wr, t, t == 0 ? wr.skip : 0);
        WaveTile a, b;
        roll_load(wr, a, b, t);
        int tot[SS_SPL];
        totals(a, b, t, T, tot);
        roll_chain_tile(m, wr, t, tot, [&](int v) { return term(v); });
        return m;
    }
};

// lists the reads of long_min samples or more (any order) and gives each its tile records
__global__ __launch_bounds__(256) void k_long_list(StatArgs a) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.b.n_reads) return;
    const uint32_t len = a.b.lengths[r];
    if (len < a.long_min) return;
    const uint32_t i = atomicAdd(&a.long_hdr->n_long, 1u);
    if (i >= LC_CAP) return;
    const uint32_t need = (len + 7u) / SS_TILE + 2u;  // tiles of the read from an 8-sample boundary in front of it
    const uint32_t off = atomicAdd(&a.long_hdr->pool_used, need);
    a.long_list[i] = r;
    LongSums *o = a.longs + i;
    o->read = r;
    o->valid = 0u;
    o->rec_off = off + need <= a.long_pool_tiles ? off : LC_NO_REC;  // (no room: the read runs on one wave as before)
    a.long_work[i].arrive = 0u;
    a.long_work[i].n_true = 0u;
    a.long_work[i].failed = 0u;
}
// A batch whose own threshold still lists more reads than two rounds of the long kernel's grid take is a batch of
// similar, long reads: one wave per read balances that by itself (1 000 reads of 500 000 samples: stat 1.4 ms) and
// the long kernel, built for a few outliers, does not (64 reads at a time).  The list is dropped.
__global__ void k_long_limit(LongHdr *hdr, uint32_t limit) {
    if (threadIdx.x == 0 && hdr->n_long > limit) hdr->n_long = 0u;
}
template <int KIND>
__global__ __launch_bounds__(LC_WG_WAVES * 64) void k_long_chains(StatArgs a, JnnP p, AdaptP ap) {
    __shared__ uint32_t hist[KIND == LC_STAT ? WH_BINS : 1];
    // these waves are the batch's critical path and share their SIMDs with the wave kernel's: they issue first
    __builtin_amdgcn_s_setprio(3);
    const uint32_t nl = a.long_hdr->n_long, n_long = nl < LC_CAP ? nl : LC_CAP;
    const uint32_t groups = gridDim.x / LC_PARTS;
    for (uint32_t i = blockIdx.x / LC_PARTS; i < n_long; i += groups) {
        LongSums *o = a.longs + i;
        if (o->rec_off == LC_NO_REC) continue;
        const uint32_t r = a.long_list[i];
        const Region g = get_region(REG_WHOLE, a.b, nullptr, r);
        LcCtx cx;
        cx.w = a.long_work + i;
        cx.hdr = a.long_hdr;
        cx.rec[0] = a.long_pool + o->rec_off;
        cx.rec[1] = a.long_pool + a.long_pool_tiles + o->rec_off;
        cx.phase = 0u;
        cx.part = (int)(blockIdx.x % LC_PARTS);
        cx.fault = a.long_fault;
        float s1[2] = {0.0f, 0.0f}, s2[2] = {0.0f, 0.0f};
        uint32_t tiles = 0u, n_true = 0u, done = 1u;  // done: 1 the sums, 2 the subtool's whole output for this read
        if (KIND == LC_STAT) {
            const Scale sc = make_scale(a.b.digitisation[r], a.b.offset[r], a.b.range[r]);
            const float nf = (float)(int)g.len;
            uint32_t *ghist = a.long_hist + (size_t)i * WH_BINS;
            for (int b = (int)threadIdx.x; b < WH_BINS / LC_PARTS; b += LC_WG_WAVES * 64) lc_st(&ghist[cx.part * (WH_BINS / LC_PARTS) + b], 0u);
            for (int b = (int)threadIdx.x; b < WH_BINS; b += LC_WG_WAVES * 64) hist[b] = 0u;
            SrcStatSums src1;
            src1.init(a.b, g, sc, a.pa_out);
            if (!lc_stage(src1, cx, src1.wr.ntiles, s1, n_true)) continue;  // declined: the redo launch has the read
            SrcStatDevs src2;
            src2.wr = src1.wr; src2.sc = sc; src2.mraw = s1[0] / nf; src2.mpa = s1[1] / nf;
            src2.lo = hist_window_lo(src2.mraw); src2.hist = hist; src2.ghist = ghist;
            if (!lc_stage(src2, cx, src2.wr.ntiles, s2, n_true)) continue;
            tiles = 4u * (uint32_t)src1.wr.ntiles;
            // the record: the read's histogram through this workgroup's LDS (everybody is behind the stage's last barrier)
            if (cx.part == 0 && threadIdx.x < 64) {
                constexpr int PER = WH_BINS / 64;
                const int lane = lane_id();
#pragma unroll
                for (int b = 0; b < PER; ++b) hist[lane * PER + b] = lc_ld(&ghist[lane * PER + b]);
                stat_finish<REG_WHOLE>(a, r, g, sc, src2.lo, hist, src2.mraw, src2.mpa, sqrtf(s2[0] / nf), sqrtf(s2[1] / nf));
            }
            __syncthreads();
            done = 2u;
        } else if (KIND == LC_JNN) {
            // (fixed thresholds: launch_jnn does not come here; slots too small for the chunks: k_jnn_wave keeps the read)
            if (p.std_scale > 0.0f && jnn_long_cap(a, r, (g.start & 7) + g.len) >= 4u) {
                const float nf = (float)(int)g.len;
                SrcClamp<false> src1;
                src1.wr.init(a.b, g); src1.mean = 0.0f;
                if (!lc_stage(src1, cx, src1.wr.ntiles, s1, n_true)) continue;
                SrcClamp<true> src2;
                src2.wr = src1.wr; src2.mean = s1[0] / nf;
                if (!lc_stage(src2, cx, src2.wr.ntiles, s2, n_true)) continue;
                tiles = 2u * (uint32_t)src1.wr.ntiles;
                // ---- the automaton on all waves: 64 chunks per wave (jnn_chunks), every chunk stages its first
                // candidate and its strong segments in its part of the upper half of the read's slots; one wave merges
                // them, 64 chunks per round
                const float mn = s1[0] / nf, band = sqrtf(s2[0] / nf) * p.std_scale;
                const JnnThr th = jnn_thresholds(mn + band, mn - band, p);
                const WaveRead &wr = src1.wr;
                const int C = jnn_long_chunks(wr.skip + g.len);
                const uint64_t slot0 = a.seg_slots[r], cap = a.seg_slots[r + 1] - slot0;
                const uint32_t half = (uint32_t)(cap / 2), capL = (uint32_t)((cap - half) / (uint32_t)C);
                {
                    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = lane_id();
                    const int gw = cx.part * LC_WG_WAVES + wv;
                    int32_t *up_x = a.seg_x + slot0 + half, *up_y = a.seg_y + slot0 + half;
                    if (gw * 64 < C) {
                        const int gc = gw * 64 + lane;
                        uint32_t *sx_ = reinterpret_cast<uint32_t *>(up_x + (uint64_t)(gc < C ? gc : 0) * capL);
                        uint32_t *sy_ = reinterpret_cast<uint32_t *>(up_y + (uint64_t)(gc < C ? gc : 0) * capL);
                        int fx = 0, fy = 0, fstrong = 0, has_first = 0;
                        uint32_t cnt = 0u;
                        auto candidate = [&](int sx, int sy, int c) {
                            const int strong = c >= p.window ? 1 : 0;
                            if (!has_first) { has_first = 1; fx = sx; fy = sy; fstrong = strong; }
                            else if (strong) {
                                if (cnt < capL - 2u) { lc_st(sx_ + 2 + cnt, (uint32_t)sx); lc_st(sy_ + 2 + cnt, (uint32_t)sy); }
                                ++cnt;
                            }
                        };
                        jnn_chunks(wr, g.len, th.hi_r, th.lo_r, p.error, th.keep_min, candidate, C, gw * 64);
                        if (gc < C) {  // the chunk's header: its first candidate, how many strong segments follow
                            lc_st(sx_, (uint32_t)fx); lc_st(sx_ + 1, (uint32_t)fy);
                            lc_st(sy_, (uint32_t)(has_first | (fstrong << 1))); lc_st(sy_ + 1, cnt);
                        }
                    }
                    if (!lc_barrier(cx)) continue;
                    if (cx.part == 0 && wv == 0) {
                        JnnCarry cy = {false, false, false, 0, 0u};
                        for (int j = 0; j < C; j += 64) {
                            const int gc = j + lane;
                            const int32_t *sx_ = up_x + (uint64_t)(gc < C ? gc : 0) * capL, *sy_ = up_y + (uint64_t)(gc < C ? gc : 0) * capL;
                            int fx = 0, fy = 0, fl = 0;
                            uint32_t cnt = 0u;
                            if (gc < C) { fx = jnn_ld<true>(sx_); fy = jnn_ld<true>(sx_ + 1); fl = jnn_ld<true>(sy_); cnt = (uint32_t)jnn_ld<true>(sy_ + 1); }
                            jnn_merge_round<true>(cy, fl & 1, fx, fy, (fl >> 1) & 1, cnt, capL - 2u, sx_ + 2, sy_ + 2, p.seg_dist,
                                                  a.seg_x + slot0, a.seg_y + slot0, half);
                        }
                        const uint32_t total = jnn_merge_flush(cy, a.seg_y + slot0, half);
                        if (lane == 0) a.n_segs[r] = total;  // (JNN_REDO_MARK: the lane-per-read kernel takes the read)
                    }
                    done = 2u;
                }
            }
        } else {
            if (g.len > ADW) {  // (always: long_min is far above the window)
                const int64_t m = g.len - ADW;
                const float mf = (float)(int)m;
                SrcRoll<false> src1;
                src1.wr.init(a.b, Region{g.start, m}); src1.mean = 0.0f;
                if (!lc_stage(src1, cx, src1.wr.ntiles, s1, n_true)) continue;
                SrcRoll<true> src2;
                src2.wr = src1.wr; src2.mean = s1[0] / mf;
                if (!lc_stage(src2, cx, src2.wr.ntiles, s2, n_true)) continue;
                tiles = 2u * (uint32_t)src1.wr.ntiles;
                // thresholds, run finder (it stops at the first adaptor candidate) and the record: one wave
                if (cx.part == 0 && threadIdx.x < 64) {
                    sgk_prefix_rec_t *rec = a.prefix + r;
                    if (threadIdx.x == 0) adaptor_init_rec(rec, g.len);
                    adaptor_find(src1.wr, window_total(src1.wr, 0, src1.wr.skip), s1[0], s2[0], mf, ap, rec);
                }
                done = 2u;
            }
        }
        if (cx.part == 0 && threadIdx.x == 0) {
            o->s1[0] = s1[0]; o->s1[1] = s1[1];
            o->s2[0] = s2[0]; o->s2[1] = s2[1];
            o->valid = done;
            atomicAdd(&a.long_hdr->n_tiles, tiles);
            atomicAdd(&a.long_hdr->n_true, n_true);
        }
    }
}
// the tile records: 8 bytes per tile and sum for the long reads of the batch, at most LC_POOL_TILES tiles
static uint32_t long_pool_tiles(uint64_t n_samples, uint32_t max_read_len) {
    if (max_read_len < LC_LONG_MIN_FLOOR) return 0u;
    const uint64_t most = n_samples / SS_TILE + 2ull * (n_samples / LC_LONG_MIN_FLOOR < LC_CAP ? n_samples / LC_LONG_MIN_FLOOR : LC_CAP) + 2ull;
    return (uint32_t)(most < LC_POOL_TILES ? most : LC_POOL_TILES);
}
size_t long_workspace_bytes(uint64_t n_samples, uint32_t max_read_len) {
    return sizeof(LongHdr) + (size_t)LC_CAP * (4 + sizeof(LongSums) + sizeof(LongWork) + LC_HIST_BINS * 4) +
           (size_t)long_pool_tiles(n_samples, max_read_len) * 16;
}
uint32_t long_threshold(uint64_t n_samples, int32_t opt_long_min, LongRule rule) {
    uint64_t lm64 = opt_long_min > 0 ? (uint64_t)opt_long_min : n_samples / rule.div;
    if (opt_long_min <= 0) {
        uint64_t fl = rule.floor_div ? n_samples / rule.floor_div : rule.floor_lo;
        fl = fl < rule.floor_lo ? rule.floor_lo : (fl > LC_LONG_MIN ? LC_LONG_MIN : fl);
        if (lm64 < fl) lm64 = fl;
    }
    if (lm64 < LC_LONG_MIN_FLOOR) lm64 = LC_LONG_MIN_FLOOR;
    return lm64 > 0xffffffffull ? 0xffffffffu : (uint32_t)lm64;
}
int prepare_long(StatArgs &a, void *ws, size_t ws_bytes, int32_t opt_long_min, LongRule auto_div, hipStream_t st) {
    a.long_hdr = nullptr;
    a.long_list = nullptr;
    a.longs = nullptr;
    a.long_work = nullptr;
    a.long_pool = nullptr;
    a.long_hist = nullptr;
    a.long_pool_tiles = 0u;
    a.long_min = 0u;
    // By default a read is long when one wavefront would still be busy with it after the rest of the batch is done:
    // a wave takes 2 - 4 ns per sample, the full GPU ~1.3 ps, and the batch's longest reads are dispatched first, so a
    // read of more than n_samples / 2048 samples (jnn, whose wave is slower on a long read: / 3072) decides when the
    // kernel ends (and one of less than 131 072 - 262 144 samples, by the size of the batch, costs less than the long
    // path's barriers: stat_args.h, LongRule).  Measured on 20 000
    // log-normal reads (1 081 of 262 144 samples or more): with all of those on the long path stat takes 6.8 ms
    // instead of 3.9 -- the wave kernels balance them.
    const uint32_t lm = long_threshold(a.b.n_samples, opt_long_min, auto_div);
    const size_t off = order_workspace_bytes(a.b.n_reads);
    if (!ws || ws_bytes < off + long_workspace_bytes(0, 0) || (reinterpret_cast<uintptr_t>(ws) & 7u)) return SGK_OK;
    char *base = static_cast<char *>(ws) + off;
    const uint32_t pool = long_pool_tiles(a.b.n_samples, a.b.max_read_len);
    if (opt_long_min < 0 || a.b.max_read_len < lm || pool == 0u || ws_bytes < off + long_workspace_bytes(a.b.n_samples, a.b.max_read_len)) {
        SGK_HIP_TRY(hipMemsetAsync(base, 0, sizeof(LongHdr), st));  // no long read in this call: sgk_stat_long_status says so
        return SGK_OK;
    }
    a.long_hdr = reinterpret_cast<LongHdr *>(base);
    base += sizeof(LongHdr);
    a.longs = reinterpret_cast<LongSums *>(base);
    base += (size_t)LC_CAP * sizeof(LongSums);
    a.long_work = reinterpret_cast<LongWork *>(base);
    base += (size_t)LC_CAP * sizeof(LongWork);
    a.long_pool = reinterpret_cast<unsigned long long *>(base);
    base += (size_t)pool * 16;
    a.long_hist = reinterpret_cast<uint32_t *>(base);
    base += (size_t)LC_CAP * LC_HIST_BINS * 4;
    a.long_list = reinterpret_cast<uint32_t *>(base);
    a.long_pool_tiles = pool;
    a.long_min = lm;
    SGK_HIP_TRY(hipMemsetAsync(a.long_hdr, 0, sizeof(LongHdr), st));
    SGK_LAUNCH_UNTIMED(k_long_list, (a.b.n_reads + 255) / 256, 256, st, a);
    if (opt_long_min == 0) SGK_LAUNCH_UNTIMED(k_long_limit, 1, 64, st, a.long_hdr, LC_AUTO_MAX_READS);
    return SGK_OK;
}
// workgroups of k_long_chains: LC_PARTS per long read the batch can hold, all resident at once (at most 64 reads at a
// time: 1 024 workgroups of 256 threads; further long reads follow in the same workgroups)
static uint32_t long_grid(const StatArgs &a) {
    const uint64_t most = a.b.n_samples / a.long_min;
    return (uint32_t)(most < 1 ? 1 : (most > 64 ? 64 : most)) * LC_PARTS;
}
int launch_k_long_chains(const char *name, int kind, hipStream_t st, const StatArgs &a, const JnnP &p, const AdaptP &ap) {
    const uint32_t grid = long_grid(a);
    if (kind == LC_STAT) SGK_LAUNCH(name, (k_long_chains<LC_STAT>), grid, LC_WG_WAVES * 64, st, a, p, ap);
    else if (kind == LC_JNN) SGK_LAUNCH(name, (k_long_chains<LC_JNN>), grid, LC_WG_WAVES * 64, st, a, p, ap);
    else if (kind == LC_ADAPT) SGK_LAUNCH(name, (k_long_chains<LC_ADAPT>), grid, LC_WG_WAVES * 64, st, a, p, ap);
    else return SGK_ERR_ARG;
    return SGK_OK;
}

}  // namespace sgk
