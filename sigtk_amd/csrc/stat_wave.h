// stat_wave.h -- the wave-per-read building blocks on seqsum.h: tiles of 64 x SS_SPL samples and their term functors,
// the tile steps of the sequential sums, the window histogram and the end of stat, jnn_core in chunks and its merge,
// the rolling totals of jnnv2 and its run finder from flip to flip.  Shared by the wave-per-read kernels
// (stat_wave.hip) and the long-read path (stat_long.hip), which evaluates single tiles with the same routines.  It must
// not include row_stream.h: the lane-per-read kernels (stat_lane.hip) are the independent implementation.
#pragma once
#include "seqsum.h"
#include "stat_device.h"

namespace sgk {

// ---------------------------------------------------------------- one WAVE per read (seqsum.h)
// The sequential float sums of a read (or of a region of it) by one wavefront: tiles of 64 x SS_SPL samples, every
// lane loads its 32 contiguous bytes with two 16-byte loads (tile t + 1 is in flight while tile t is consumed), the
// sums advance through the tile as seqsum.h describes.  Two passes over the samples:
//   1. sum of raw and of pA                                   -> the two means (src/stat.h:17-33)
//   2. sums of the squared deviations (src/stat.h:36-54), the histogram of the raw values over a window of WH_BINS codes
//      centred on the raw mean (median = order statistic of rank n/2, src/stat.h:56-73), and -- fused stat + pa,
//      BASELINE config 4 -- the pA value of every sample
// The second pass of a read follows its first on the same wave; reads whose order statistic falls outside the window
// are flagged (`reserved`) and taken by k_median.  Ragged batches cost what their samples cost: a wave is busy for the
// length of ITS read, not for the longest read among 64 neighbours as in the lane-per-read kernels above.
constexpr int WH_BINS = 2048;
static_assert(WH_BINS == (int)LC_HIST_BINS, "the long reads' histograms in the workspace");

struct WaveTile {
    uint32_t w[SS_SPL / 2];
    template <int E>
    __device__ __forceinline__ int16_t sample() const {
        return (E & 1) ? (int16_t)(w[E / 2] >> 16) : (int16_t)(w[E / 2] & 0xffffu);
    }
};
// This lane's 16 samples of the tile that starts at base-relative index `tile0` (wave-uniform, >= 0, a multiple of 8, as
// is n_total >= 8).  Both 16-byte loads are unconditional, so that the load of tile t + 1 stays in flight under tile t,
// and addressed as uniform base + 32-bit lane offset (scalar address arithmetic).  (Round 5: with the non-temporal hint
// on these loads every wave kernel is slower -- stat+pa 19.2 -> 20.5 ms, jnn 15.5 -> 16.7, jnnv2 13.1 -> 18.7: the
// second 16-byte load of a lane and jnnv2's trailing tile live on the line staying where the first load put it.)
// Near the end of the buffer the offsets are clamped to its last 16 bytes: such samples are outside the region and
// masked by the term functors.
__device__ __forceinline__ void wt_load(WaveTile &t, const int16_t *samples, int64_t n_total, int64_t tile0) {
    const int64_t last = n_total - 8;
    const int64_t t0 = tile0 < last ? tile0 : last;
    const int64_t room64 = (last - t0) * (int64_t)sizeof(int16_t);
    const uint32_t room = room64 > 4096 ? 4096u : (uint32_t)room64;  // largest legal byte offset, a multiple of 16
    const char *tb = reinterpret_cast<const char *>(samples + t0);
    const uint32_t lo = (uint32_t)lane_id() * (uint32_t)(SS_SPL * sizeof(int16_t));
    const uint32_t o0 = lo < room ? lo : room, o1 = lo + 16u < room ? lo + 16u : room;
    const uint4 q0 = *static_cast<const uint4 *>(__builtin_assume_aligned(tb + o0, 16));
    const uint4 q1 = *static_cast<const uint4 *>(__builtin_assume_aligned(tb + o1, 16));
    t.w[0] = q0.x; t.w[1] = q0.y; t.w[2] = q0.z; t.w[3] = q0.w;
    t.w[4] = q1.x; t.w[5] = q1.y; t.w[6] = q1.z; t.w[7] = q1.w;
}

// calls f.template operator()<E>(raw, valid) for this lane's 16 samples (tile-local indices q0 .. q0 + 15)
template <int E, bool INTERIOR, typename F>
__device__ __forceinline__ void wt_each_(const WaveTile &t, int q0, int q_lo, int q_hi, F &f) {
    if constexpr (E < SS_SPL) {
        f.template operator()<E>(t.sample<E>(), INTERIOR || (q0 + E >= q_lo && q0 + E < q_hi));
        wt_each_<E + 1, INTERIOR>(t, q0, q_lo, q_hi, f);
    }
}

struct WaveRead {  // wave-uniform description of the region a wave works on
    const int16_t *samples;
    int64_t n_total, rb, len;
    int skip, ntiles;
    __device__ void init(const sgk_batch_t &b, const Region &g) {
        samples = b.samples;
        n_total = (int64_t)b.n_samples;
        rb = g.start & ~(int64_t)7;
        skip = (int)(g.start - rb);
        len = g.len;
        ntiles = (int)((skip + len + SS_TILE - 1) / SS_TILE);
    }
    __device__ __forceinline__ void load(WaveTile &t, int tile) const {
        wt_load(t, samples, n_total, rb + (int64_t)tile * SS_TILE);
    }
    // a tile strictly inside the region (and not the first one, whose head is added natively): no predicates
    __device__ __forceinline__ bool interior(int tile) const {
        return tile > 0 && (int64_t)(tile + 1) * SS_TILE - skip <= len;
    }
    __device__ __forceinline__ int head() const { return (int)(len < SS_HEAD ? len : SS_HEAD); }
    // tile-local index range [q_lo, q_hi) of the region's samples in `tile`, without its first `drop` samples
    __device__ __forceinline__ void range(int tile, int drop, int &q_lo, int &q_hi) const {
        const int64_t lo = (int64_t)skip + drop - (int64_t)tile * SS_TILE, hi = (int64_t)skip + len - (int64_t)tile * SS_TILE;
        q_lo = lo < 0 ? 0 : (lo > SS_TILE ? SS_TILE : (int)lo);
        q_hi = hi < 0 ? 0 : (hi > SS_TILE ? SS_TILE : (int)hi);
    }
};

// term functors of the four sums (seqsum.h): INTERIOR tiles need no validity test.  `z` is 0; the rare paths of
// ss_finish pass an OPAQUE zero (SsOpaque) so that their term arithmetic stays inside those paths -- the compiler
// otherwise hoists all of it in front of the fast path and keeps 32 terms alive across it.
template <bool INTERIOR>
struct TermBase {
    static constexpr bool interior = INTERIOR;
    const WaveTile &t;
    int q0, q_lo, q_hi;  // q0: tile-local index of this lane's first sample
    uint32_t z;
    template <int E>
    __device__ __forceinline__ bool valid() const { return INTERIOR || (q0 + E >= q_lo && q0 + E < q_hi); }
    template <int E>
    __device__ __forceinline__ int16_t sample() const {
        const uint32_t w = t.w[E / 2] ^ z;
        return (E & 1) ? (int16_t)(w >> 16) : (int16_t)(w & 0xffffu);
    }
    template <int E>
    __device__ __forceinline__ float clamped() const {  // rm_outlier of the sample: the clamp is packed, two per dword
        const s16x2 c = clamp_raw2(t.w[E / 2] ^ z);
        return (float)((E & 1) ? c.y : c.x);
    }
};
template <bool INTERIOR>
struct TermRaw {  // (float)raw, src/stat.h:29-33
    TermBase<INTERIOR> b;
    int sm;  // -1 while the accumulator runs on the negated chain (orientation, as TermPa's unit), else 0
    __device__ __forceinline__ TermRaw with(uint32_t z) const { TermRaw r = *this; r.b.z = z; return r; }
    template <int E>
    __device__ __forceinline__ float get() const {
        // negated as an integer: a zero sample stays +0 (a -0.0 term would count as negative and end the fast walk)
        const int v = (int)b.template sample<E>();
        return b.template valid<E>() ? (float)((v ^ sm) - sm) : 0.0f;
    }
};
template <bool INTERIOR>
struct TermPa {   // pA, src/stat.h:17-27 on signal_in_picoamps' output
    TermBase<INTERIOR> b;
    Scale so;     // unit carries the orientation of the accumulator
    __device__ __forceinline__ TermPa with(uint32_t z) const { TermPa r = *this; r.b.z = z; return r; }
    template <int E>
    __device__ __forceinline__ float get() const {
        return b.template valid<E>() ? to_pa(b.template sample<E>(), so) : 0.0f;
    }
};
template <bool INTERIOR>
struct TermDevRaw {  // (raw - mean)^2, src/stat.h:46-54
    TermBase<INTERIOR> b;
    float mean;
    __device__ __forceinline__ TermDevRaw with(uint32_t z) const { TermDevRaw r = *this; r.b.z = z; return r; }
    template <int E>
    __device__ __forceinline__ float get() const {
        const float d = (float)b.template sample<E>() - mean;
        return b.template valid<E>() ? d * d : 0.0f;
    }
};
template <bool INTERIOR>
struct TermDevPa {   // (pA - mean)^2, src/stat.h:36-44
    TermBase<INTERIOR> b;
    Scale sc;
    float mean;
    __device__ __forceinline__ TermDevPa with(uint32_t z) const { TermDevPa r = *this; r.b.z = z; return r; }
    template <int E>
    __device__ __forceinline__ float get() const {
        const float d = to_pa(b.template sample<E>(), sc) - mean;
        return b.template valid<E>() ? d * d : 0.0f;
    }
};

__device__ __forceinline__ int ss_edge_zero() { return (int)ss_opaque_zero(); }
// the signed value of an oriented accumulator (a zero accumulator stands for +0)
__device__ __forceinline__ float ss_signed(float m, bool negated) { return m == 0.0f ? 0.0f : (negated ? -m : m); }

// one tile of two chains: both walks are issued before either chain's (branching) bookkeeping.  mka / mkb build the
// chains' term functors from a TermBase<INTERIOR>.
template <bool NEG, typename MA, typename MB>
__device__ __forceinline__ void ss_tile2(float &ma, float &mb, const WaveRead &wr, const WaveTile &cur, int t, MA mka, MB mkb) {
    const int q0 = lane_id() * SS_SPL;
    int q_lo, q_hi;
    if (t == 0) {  // the head of the read, natively (the functors mask what lies behind it)
        wr.range(0, 0, q_lo, q_hi);
        const int qh = q_lo + wr.head();
        if (qh > q_lo)
            ss_serial2(ma, mb, mka(TermBase<false>{cur, q0, q_lo, qh, 0u}), mkb(TermBase<false>{cur, q0, q_lo, qh, 0u}),
                       q_lo / SS_SPL, (qh - 1) / SS_SPL);
    }
    wr.range(t, t == 0 ? wr.head() : 0, q_lo, q_hi);
    SsWalk wa, wb;
    if (wr.interior(t)) {
        wa = ss_walk<NEG>(ma, mka(TermBase<true>{cur, q0, q_lo, q_hi, 0u}));
        wb = ss_walk<NEG>(mb, mkb(TermBase<true>{cur, q0, q_lo, q_hi, 0u}));
    } else {
        // (The 32 validity compares of an edge tile are evaluated in front of the branch, on every tile.  Round 5 kept
        // them inside it with an opaque copy of q0, as ss_tile1 does: two registers more, which k_stat_wave does not
        // have -- 127 and 2 spilled, 20.05 against 19.72 ms for stat+pa at 125 000 x 100 000; opaque copies of the
        // scalars q_lo / q_hi instead cost no register and are slower all the same, 19.7 against 19.4.)
        wa = ss_walk<NEG>(ma, mka(TermBase<false>{cur, q0, q_lo, q_hi, 0u}));
        wb = ss_walk<NEG>(mb, mkb(TermBase<false>{cur, q0, q_lo, q_hi, 0u}));
    }
    int ska, skb;
    if (ss_fast<NEG>(ma, wa, mka(TermBase<false>{cur, q0, q_lo, q_hi, 0u}), ska))
        ma = ss_finish<NEG>(ma, mka(TermBase<false>{cur, q0, q_lo, q_hi, 0u}), wa, ska);
    if (ss_fast<NEG>(mb, wb, mkb(TermBase<false>{cur, q0, q_lo, q_hi, 0u}), skb))
        mb = ss_finish<NEG>(mb, mkb(TermBase<false>{cur, q0, q_lo, q_hi, 0u}), wb, skb);
}

// pA of every sample of tile t, written as whole cache lines: the tile is read once more as 4 x 256 samples with 8 bytes
// per lane (L2 hits) so that a store instruction covers 1 KB contiguously (the sums' layout, 64 bytes per lane, would make
// every store instruction touch 32 lines partially).  pa_dst: the pA array at the region's 8-sample base (wr.rb).
__device__ __forceinline__ void pa_write_tile(const WaveRead &wr, int t, const Scale &sc, float *pa_dst) {
    const int lane = lane_id();
    int q_lo, q_hi;
    wr.range(t, 0, q_lo, q_hi);
    const bool pa_interior = q_lo == 0 && q_hi == SS_TILE;
#pragma unroll 1
    for (int sub = 0; sub < SS_TILE / 256; ++sub) {
        const int qs = sub * 256 + lane * 4;
        int64_t pp = wr.rb + (int64_t)t * SS_TILE + qs;
        const int64_t last = wr.n_total - 4;
        pp = pp < last ? pp : last;
        const uint2 rw = *reinterpret_cast<const uint2 *>(wr.samples + pp);
        const float4 o = make_float4(to_pa((int16_t)(rw.x & 0xffffu), sc), to_pa((int16_t)(rw.x >> 16), sc),
                                     to_pa((int16_t)(rw.y & 0xffffu), sc), to_pa((int16_t)(rw.y >> 16), sc));
        float *dst = pa_dst + (int64_t)t * SS_TILE + qs;
        // (a group of four inside the region is stored whole in an edge tile as well: dst is 16-byte aligned)
        if (pa_interior || (qs >= q_lo && qs + 4 <= q_hi)) *reinterpret_cast<float4 *>(dst) = o;
        else {
            if (qs >= q_lo && qs < q_hi) dst[0] = o.x;
            if (qs + 1 >= q_lo && qs + 1 < q_hi) dst[1] = o.y;
            if (qs + 2 >= q_lo && qs + 2 < q_hi) dst[2] = o.z;
            if (qs + 3 >= q_lo && qs + 3 < q_hi) dst[3] = o.w;
        }
    }
}
// The same from the tile the wave already holds (round 5): the re-read above missed the L2 on 60 % of its lines at
// 125 000 x 100 000 (15 of 65 GB fetched; the 50 GB of pA stores go through the same L2), so the wave turns its tile into
// the stores' layout through 2 KB of LDS instead -- `tl`, the wave's histogram, which pass 1 does not use yet.
__device__ __forceinline__ void pa_write_tile_lds(const WaveRead &wr, int t, const Scale &sc, float *pa_dst, const WaveTile &cur,
                                                  uint32_t *tl) {
    const int lane = lane_id();
    int q_lo, q_hi;
    wr.range(t, 0, q_lo, q_hi);
    const bool pa_interior = q_lo == 0 && q_hi == SS_TILE;
    uint4 *row = reinterpret_cast<uint4 *>(tl) + lane * 2;
    row[0] = make_uint4(cur.w[0], cur.w[1], cur.w[2], cur.w[3]);
    row[1] = make_uint4(cur.w[4], cur.w[5], cur.w[6], cur.w[7]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int sub = 0; sub < SS_TILE / 256; ++sub) {
        const int qs = sub * 256 + lane * 4;
        const uint2 rw = *reinterpret_cast<const uint2 *>(tl + sub * 128 + lane * 2);
        const float4 o = make_float4(to_pa((int16_t)(rw.x & 0xffffu), sc), to_pa((int16_t)(rw.x >> 16), sc),
                                     to_pa((int16_t)(rw.y & 0xffffu), sc), to_pa((int16_t)(rw.y >> 16), sc));
        float *dst = pa_dst + (int64_t)t * SS_TILE + qs;
        if (pa_interior || (qs >= q_lo && qs + 4 <= q_hi)) *reinterpret_cast<float4 *>(dst) = o;
        else {
            if (qs >= q_lo && qs < q_hi) dst[0] = o.x;
            if (qs + 1 >= q_lo && qs + 1 < q_hi) dst[1] = o.y;
            if (qs + 2 >= q_lo && qs + 2 < q_hi) dst[2] = o.z;
            if (qs + 3 >= q_lo && qs + 3 < q_hi) dst[3] = o.w;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the next tile's rows are written behind these reads
    __builtin_amdgcn_wave_barrier();
}
// the histogram window of a read: WH_BINS raw values around its mean
__device__ __forceinline__ int hist_window_lo(float mraw) {
    const int c = (mraw == mraw) ? (int)fminf(fmaxf(mraw, -32768.0f), 32767.0f) : 0;
    const int lo = c - WH_BINS / 2;
    return lo < -32768 ? -32768 : (lo > 32768 - WH_BINS ? 32768 - WH_BINS : lo);
}
// this lane's 16 samples of a tile into the window histogram (LDS)
template <bool INTERIOR>
__device__ __forceinline__ void hist_tile(const WaveTile &cur, int q_lo, int q_hi, int lo, uint32_t *hist) {
    auto each = [&]<int E>(int16_t v, bool valid) {
        if (valid) {
            int b = (int)v - lo;
            b = b < 0 ? 0 : (b > WH_BINS - 1 ? WH_BINS - 1 : b);
            atomicAdd(&hist[b], 1u);
        }
    };
    wt_each_<0, INTERIOR>(cur, lane_id() * SS_SPL, q_lo, q_hi, each);
}
// The end of stat for one region, by one wave: the order statistics of ranks k (raw median) and, for a negative unit,
// n-1-k (the pA median's raw value) from the window histogram `hist` (LDS, complete and visible to this wave), and the
// record.  A median outside the window leaves the read flagged for k_median.
template <int MODE>
__device__ inline void stat_finish(const StatArgs &a, uint32_t r, const Region &g, const Scale &sc, int lo, const uint32_t *hist,
                                   float mraw, float mpa, float sdraw, float sdpa) {
    const int lane = lane_id();
    const int64_t k = g.len / 2;
    const bool mirrored = sc.unit < 0.0f && g.len - 1 - k != k;  // pA order is the reverse of the raw order
    constexpr int PER = WH_BINS / 64;
    uint32_t cnt[PER], lsum = 0u;
#pragma unroll
    for (int i = 0; i < PER; ++i) { cnt[i] = hist[lane * PER + i]; lsum += cnt[i]; }
    const uint32_t incl = (uint32_t)wave_incl_scan_i((int)lsum), excl = incl - lsum;
    int found[2] = {0, 0};
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        const uint32_t rank = (uint32_t)(w ? (mirrored ? g.len - 1 - k : k) : k);
        int bin = 0;
        if (rank >= excl && rank < incl) {
            uint32_t acc = excl;
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                if (rank >= acc && rank < acc + cnt[i]) bin = lane * PER + i;
                acc += cnt[i];
            }
        }
        const unsigned long long own = __ballot(rank >= excl && rank < incl);
        found[w] = own ? __builtin_amdgcn_readlane(bin, __builtin_amdgcn_readfirstlane(__ffsll((long long)own) - 1)) : 0;
    }
    const bool trusted = g.len > 0 && found[0] > 0 && found[0] < WH_BINS - 1 && found[1] > 0 && found[1] < WH_BINS - 1;
    if (lane == 0) {
        const int med = lo + found[0];
        const float pm = to_pa((int16_t)(lo + found[1]), sc);
        const bool pending = g.len > 0 && !trusted;
        if (MODE == REG_WHOLE) {
            sgk_stat_rec_t *o = a.stat + r;
            o->raw_mean = mraw; o->pa_mean = mpa; o->raw_std = sdraw; o->pa_std = sdpa;
            o->raw_median = g.len > 0 ? med : 0;
            o->pa_median = g.len > 0 ? pm : 0.0f;
            o->n = (uint32_t)g.len;
            o->reserved = pending ? FLAG_MEDIAN_WHOLE : 0u;
        } else if (MODE == REG_ADAPT) {
            a.prefix[r].adapt_mean = mpa;
            a.prefix[r].adapt_std = sdpa;
            if (g.len > 0) a.prefix[r].adapt_median = pm;
            if (pending) a.prefix[r].reserved |= FLAG_MEDIAN_ADAPT;
        } else {
            a.prefix[r].polya_mean = mpa;
            a.prefix[r].polya_std = sdpa;
            if (g.len > 0) a.prefix[r].polya_median = pm;
            if (pending) a.prefix[r].reserved |= FLAG_MEDIAN_POLYA;
        }
    }
}

// ---------------------------------------------------------------- jnn_raw, one WAVE per read
// jnn_core's state (open / err / prev_err / c) is reset whenever a segment ends, and every open segment ends inside a
// streak of more than `error` consecutive out-of-range samples: behind such a streak the automaton is closed, whatever
// happened before it -- SYNC POINTS that depend on the data alone.  The read is cut into 64 chunks; lane c scans from
// the nominal start of chunk c to the first sync point at or behind it, runs the automaton from there (closed) to the
// first sync point at or behind the nominal start of chunk c + 1, where lane c + 1 has started: exact, no speculation,
// nothing to verify; reads without such streaks degenerate to fewer, longer lane runs.  (Valid while the `err--`
// correction of jnn.c:228,238 cannot fire, i.e. error < corrector as in every preset; other parameters use k_jnn.)
// Thresholds: the sequential float moments of the clamped signal through seqsum.h (two coalesced passes).  A lane
// stages its kept segments in its own part of the upper half of the read's slots; the merge (src/jnn.c:246-258) is a
// flag scan: a kept segment opens a new merged segment iff its start is seg_dist or more behind the previous end.
template <bool INTERIOR>
struct TermClamp {  // rm_outlier(raw), src/jnn.c:61-77
    TermBase<INTERIOR> b;
    __device__ __forceinline__ TermClamp with(uint32_t z) const { TermClamp r = *this; r.b.z = z; return r; }
    template <int E>
    __device__ __forceinline__ float get() const {
        return b.template valid<E>() ? b.template clamped<E>() : 0.0f;
    }
};
template <bool INTERIOR>
struct TermDevClamp {  // (rm_outlier(raw) - mean)^2
    TermBase<INTERIOR> b;
    float mean;
    __device__ __forceinline__ TermDevClamp with(uint32_t z) const { TermDevClamp r = *this; r.b.z = z; return r; }
    template <int E>
    __device__ __forceinline__ float get() const {
        const float d = b.template clamped<E>() - mean;
        return b.template valid<E>() ? d * d : 0.0f;
    }
};
// one tile of one chain (see ss_tile2)
template <bool NEG, typename MK>
__device__ __forceinline__ void ss_tile1(float &m, const WaveRead &wr, const WaveTile &cur, int t, MK mk) {
    const int q0 = lane_id() * SS_SPL;
    int q_lo, q_hi;
    if (t == 0) {
        wr.range(0, 0, q_lo, q_hi);
        const int qh = q_lo + wr.head();
        if (qh > q_lo) m = ss_serial(m, mk(TermBase<false>{cur, q0, q_lo, qh, 0u}), q_lo / SS_SPL, (qh - 1) / SS_SPL);
    }
    wr.range(t, t == 0 ? wr.head() : 0, q_lo, q_hi);
    // (q0 of the edge branch through an opaque copy made there: its 32 validity compares were otherwise evaluated in
    // front of the branch, on every tile -- a third of the vector time of an interior tile's walk, round 5)
    SsWalk w;
    if (wr.interior(t)) w = ss_walk<NEG>(m, mk(TermBase<true>{cur, q0, q_lo, q_hi, 0u}));
    else w = ss_walk<NEG>(m, mk(TermBase<false>{cur, q0 + ss_edge_zero(), q_lo, q_hi, 0u}));
    int sk;
    if (ss_fast<NEG>(m, w, mk(TermBase<false>{cur, q0, q_lo, q_hi, 0u}), sk))
        m = ss_finish<NEG>(m, mk(TermBase<false>{cur, q0, q_lo, q_hi, 0u}), w, sk);
}

constexpr int JW_BLOCK = 32;  // samples a lane takes per step of the chunked pass

// The chunked pass of jnn_core shared by k_jnn_wave and k_polya_wave: in <=> lo_r < raw < hi_r; `candidate(x, y, c)`
// is called, per lane in sample order, for every segment that ended after c >= keep_min samples.
__device__ __forceinline__ int jnn_chunk_lanes(int64_t nq) { return nq >= 512 ? (nq / 256 >= 64 ? 64 : (int)(nq / 256)) : 1; }
// (C chunks in all; this wave's lane l takes chunk gchunk0 + l: one wave per read has C <= 64 and gchunk0 = 0, the waves
// of a long read share its C = 64 x waves chunks)
// ... and of a long read on LC_WAVES waves: chunks of at least 512 samples, at most 64 per wave
__device__ __forceinline__ int jnn_long_chunks(int64_t nq) {
    const int64_t c = nq / 512;
    const int lanes = jnn_chunk_lanes(nq);
    return c > 64 * LC_WAVES ? 64 * LC_WAVES : (c > lanes ? (int)c : lanes);
}
// slots per chunk of a long read's staging area (the upper half of its slots); below 4 the read stays with k_jnn_wave
__device__ __forceinline__ uint32_t jnn_long_cap(const StatArgs &a, uint32_t r, int64_t nq) {
    const uint64_t cap = a.seg_slots[r + 1] - a.seg_slots[r];
    return (uint32_t)((cap - cap / 2) / (uint32_t)jnn_long_chunks(nq));
}
// Where the blocks' in-range masks come from is the SOURCE's business (`src`): JnnSrcRaw below forms them from int16 samples
// and integer thresholds; the float batch (jnnf_kernels.hip) reads masks it made from floats.  A source has
//   skew(q)        how far q lies behind the start of its line (the lane's first line is moved back by it)
//   load_line(q)   requests the line of JW_LINE positions at q (a multiple of JW_LINE behind skew) into the source
//   block_mask(h)  bit e: position e of block h of the loaded line is in range (positions outside the read: anything)
// `skip`: q of the read's sample 0.
template <typename SRC, typename CAND>
__device__ __forceinline__ void jnn_chunks_src(SRC &src, int skip, int64_t n, int error, int keep_min, CAND &candidate, int C,
                                               int gchunk0) {
    const int lane = lane_id();
    const int E1 = error + 1;
    // ---- chunks in q space (q = sample index + skip; chunk bounds are multiples of 8 -> 16-byte aligned loads)
    const int64_t nq = skip + n;
    const int64_t K = ((nq + C - 1) / C + 7) & ~(int64_t)7;
    const int LEAD = (E1 + 7) & ~7;
    const int gc = gchunk0 + lane;
    const bool active = gc < C;
    const int64_t cs = (int64_t)gc * K, ce = cs + K;             // nominal chunk of this lane
    int64_t qb = gc == 0 ? 0 : cs - LEAD;                        // where this lane starts reading
    int runm = (gc == 0) ? -1 : 0, srchm = (active && gc != 0) ? -1 : 0;  // -1 / 0 lane masks
    int opn = 0, err = 0, run = 0, start = 0, oc = 0;
    // A block of 32 samples as bit masks (bit e: sample e is in / out of range; samples outside the read are neither).
    // The automaton goes from EVENT to event -- a segment opens at the next set bit of `inm`; it ends at the
    // (error + 1 - err)-th set bit of `outm` behind that -- instead of sample by sample: a segment lives for ~13 samples
    // on nanopore data, so a block holds a handful of events.  Positions [lo, hi) of the block belong to this lane's run.
    auto run_block = [&](uint32_t inm, uint32_t outm, int i0, int lo, int hi) {
        const uint32_t range = (lo >= 32 ? 0u : (0xffffffffu >> lo) << lo) & (hi >= 32 ? 0xffffffffu : ((1u << hi) - 1u));
        inm &= range;
        outm &= range;
        int pos = lo;
        for (;;) {
            const uint32_t keep = pos >= 32 ? 0u : (0xffffffffu >> pos) << pos;  // bits at positions >= pos
            if (!opn) {
                const uint32_t m = inm & keep;
                if (!m) break;
                const int e = __ffs((int)m) - 1;
                start = i0 + e; opn = -1; err = 0; run = 0; pos = e + 1;
            } else {
                uint32_t mo = outm & keep;
                const int need = error - err + 1;
                const int pc = __popc(mo);
                if (pc < need) {
                    err += pc;
                    const uint32_t mi = inm & keep;
                    run = mi ? __clz((int)mi) - (32 - hi) : run + (hi - pos);
                    break;
                }
                for (int k = 1; k < need; ++k) mo &= mo - 1u;
                const int e = __ffs((int)mo) - 1;
                const uint32_t mi = inm & keep & ((1u << e) - 1u);  // in-range samples in [pos, e)
                const int perr = mi ? e - (32 - __clz((int)mi)) : run + (e - pos);
                const int i = i0 + e;
                if (i - start >= keep_min) candidate(start, i - perr, i - start);
                opn = 0; err = 0; run = 0; pos = e + 1;
            }
        }
    };
    // bit e set: sample e ends a streak of at least E1 out-of-range samples (oc_in of them in front of the block):
    // behind it the automaton is closed (E1 <= 32)
    auto sync_bits = [&](uint32_t outm, int oc_in) -> uint32_t {
        const uint32_t prev = oc_in >= 32 ? 0xffffffffu : ~(0xffffffffu >> oc_in);  // the oc_in samples in front
        unsigned long long x = ((unsigned long long)outm << 32) | prev;
        for (int k = 1; k < E1;) {
            const int st = k < E1 - k ? k : E1 - k;
            x &= x << st;
            k += st;
        }
        return (uint32_t)(x >> 32);
    };

    constexpr int JW_LINE = 2 * JW_BLOCK;  // positions per line
    qb -= src.skew(qb);  // (starting earlier only adds to what the sync search knows)
    // the automaton over the block of 32 samples at q
    auto step = [&](uint32_t inm, int64_t q) {
        const bool busy = active && (srchm | runm) && q < nq;
        if (!busy) return;
        uint32_t vmask = 0xffffffffu;
        if (q < skip || q + JW_BLOCK > nq) {  // a block on the read's edge
            const int64_t a0 = skip - q, a1 = nq - q;
            const int lo = a0 < 0 ? 0 : (a0 > 32 ? 32 : (int)a0), hi = a1 > 32 ? 32 : (a1 < 0 ? 0 : (int)a1);
            vmask = (lo >= 32 ? 0u : (0xffffffffu >> lo) << lo) & (hi >= 32 ? 0xffffffffu : ((1u << hi) - 1u));
        }
        inm &= vmask;
        const uint32_t outm = ~inm & vmask;
        int lo = 0, hi = 32;
        bool ends_here = false;
        if (srchm || q + JW_BLOCK >= ce) {  // the sync logic is in play (the block holds sample ce - 1 or lies behind it)
            const uint32_t sy = sync_bits(outm, oc);
            if (srchm) {  // the run starts behind the first sync sample at position >= cs - 1
                const int64_t f = cs - q - 1;
                const uint32_t m = f >= 32 ? 0u : (f <= 0 ? sy : (sy >> f) << f);
                if (m) {
                    lo = __ffs((int)m);  // position behind that sample
                    srchm = 0;
                    runm = q + lo >= ce ? 0 : -1;
                } else lo = 32;
            }
            if (runm && q + JW_BLOCK >= ce) {  // ... and ends with the first sync sample at position >= ce - 1
                int64_t f = ce - q - 1;
                if (f < lo) f = lo;
                const uint32_t m = f >= 32 ? 0u : (f <= 0 ? sy : (sy >> f) << f);
                if (m) { hi = __ffs((int)m); ends_here = true; }  // (hi can be 32: the sync sample is the block's last)
            }
        }
        if (runm && lo < hi) run_block(inm, outm, (int)(q - skip), lo, hi);
        if (ends_here) runm = 0;  // done
        const uint32_t stop = inm | ~vmask;  // samples that are not out of range
        oc = stop ? __clz((int)stop) : oc + 32;
    };
    src.load_line(qb);
    for (;;) {
        if (!__any(active && (srchm | runm) && qb < nq)) break;
        const uint32_t m0 = src.block_mask(0), m1 = src.block_mask(1);
        src.load_line(qb + JW_LINE);
        step(m0, qb);
        step(m1, qb + JW_BLOCK);
        qb += JW_LINE;
    }
}

// The source of the int16 kernels: in <=> lo_r < raw < hi_r on the samples of `wr`.
// Every lane streams its own chunk, a whole 128-byte line (two blocks) per step, from a line boundary: the masks of
// both blocks are formed first, the next line is requested into the registers that frees, and is in flight under
// the automaton's two blocks.  (Round 5.  Until then a lane took 64 bytes per step with the next 64 in flight: the
// two halves of a line were requested a whole step apart, 3.6 us during which 4 MB pass through an XCD's 4 MB L2,
// and 60 % of the lines were fetched twice -- 15 of the kernel's 90 GB at 125 000 x 100 000, in a kernel that runs
// at 5.8 TB/s.  Earlier attempts kept two whole lines per lane in registers: 115 registers instead of 89, four waves
// per SIMD instead of five, 16.4 ms against 15.6; the LDS row stager of the lane-per-read kernels lost to its
// barriers.)
struct JnnSrcRaw {
    static constexpr int JW_LINE = 2 * JW_BLOCK;  // samples per 128-byte line
    const WaveRead &wr;
    // lo_r < v < hi_r  <=>  lp1 <= v <= hm1 on int16 samples (thresholds beyond the int16 range: always / never)
    bool never;
    s16x2 hm1, lp1;
    uint32_t ln[JW_LINE / 2];
    __device__ __forceinline__ JnnSrcRaw(const WaveRead &wr_, int hi_r, int lo_r) : wr(wr_) {
        never = hi_r <= -32768 || lo_r >= 32767;
        const int hm1_i = hi_r - 1 > 32767 ? 32767 : hi_r - 1, lp1_i = lo_r + 1 < -32768 ? -32768 : lo_r + 1;
        hm1 = s16x2{(short)hm1_i, (short)hm1_i};
        lp1 = s16x2{(short)lp1_i, (short)lp1_i};
    }
    __device__ __forceinline__ int64_t skew(int64_t qb) const { return (wr.rb + qb) & (int64_t)(JW_LINE - 1); }
    __device__ __forceinline__ void load_line(int64_t q) {
        const int64_t last = wr.n_total - 8;
#pragma unroll
        for (int v = 0; v < JW_LINE / 8; ++v) {
            int64_t pp = wr.rb + q + 8 * v;
            pp = pp < last ? pp : last;
            pp = pp < 0 ? 0 : pp;
            const uint4 u = *reinterpret_cast<const uint4 *>(wr.samples + pp);
            ln[4 * v] = u.x; ln[4 * v + 1] = u.y; ln[4 * v + 2] = u.z; ln[4 * v + 3] = u.w;
        }
    }
    static __device__ __forceinline__ uint32_t spread16(uint32_t x) {  // bit k -> bit 2k
        x = (x | (x << 8)) & 0x00FF00FFu;
        x = (x | (x << 4)) & 0x0F0F0F0Fu;
        x = (x | (x << 2)) & 0x33333333u;
        x = (x | (x << 1)) & 0x55555555u;
        return x;
    }
    // bit e of the result: lo_r < sample e < hi_r of the block in ln[16 h ..].  Two samples per instruction (one by one
    // this was 18 issue cycles per sample): saturating packed subtractions leave the sign of (hi_r - 1) - v and of
    // v - (lo_r + 1) in bits 15 / 31 of a word -- either set: out of range --, the words' flags are collected by
    // shifting (even samples in the low half, odd ones in the high half) and the two halves interleaved at the end.
    __device__ __forceinline__ uint32_t block_mask(int h) const {
        uint32_t acc = 0u;
#pragma unroll
        for (int k = 0; k < JW_BLOCK / 2; ++k) {
            const s16x2 v = __builtin_bit_cast(s16x2, ln[h * (JW_BLOCK / 2) + k]);
            const uint32_t d = __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(hm1, v)) |
                               __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(v, lp1));
            acc = (d & 0x80008000u) | ((acc >> 1) & 0x7fff7fffu);
        }
        return never ? 0u : ~(spread16(acc & 0xffffu) | (spread16(acc >> 16) << 1));
    }
};
template <typename CAND>
__device__ __forceinline__ void jnn_chunks(const WaveRead &wr, int64_t n, int hi_r, int lo_r, int error, int keep_min,
                                           CAND &candidate, int C, int gchunk0) {
    JnnSrcRaw src(wr, hi_r, lo_r);
    jnn_chunks_src(src, wr.skip, n, error, keep_min, candidate, C, gchunk0);
}

// The merge of the kept segments (src/jnn.c:246-258), 64 chunks per round, in chunk order.  A chunk's kept segments are
// [its first candidate, if that is strong or the first candidate of the read] + its staged strong ones; a kept segment
// opens a new merged segment iff its start is seg_dist or more behind the previous kept segment's end.  Between rounds
// the carry holds the last kept segment (its end is written once the next kept segment turns out to open a new merged
// one, or by jnn_merge_flush) and the number of merged segments so far.
struct JnnCarry {
    bool has, seen, overflow;  // a kept segment so far; a candidate so far; some slot range was too small
    int y;                     // end of the last kept segment
    uint32_t idx;              // merged segments opened so far
};
template <bool AGENT>
__device__ __forceinline__ int jnn_ld(const int32_t *p) {
    if constexpr (AGENT) return (int)lc_ld(reinterpret_cast<const uint32_t *>(p));
    else return *p;
}
template <bool AGENT>  // AGENT: the staged segments were written by other workgroups (agent-scope atomics)
__device__ inline void jnn_merge_round(JnnCarry &cy, int has_first, int fx, int fy, int fstrong, uint32_t cnt, uint32_t cap_l,
                                       const int32_t *stage_x, const int32_t *stage_y, int seg_dist, int32_t *out_x,
                                       int32_t *out_y, uint32_t half) {
    const int lane = lane_id();
    const unsigned long long hasf = __ballot(has_first != 0);
    const int firstlane = (!cy.seen && hasf) ? __ffsll((long long)hasf) - 1 : -1;
    const bool keep_first = has_first && (fstrong || lane == firstlane);
    bool overflow = cnt > cap_l;
    if (cnt > cap_l) cnt = cap_l;
    const uint32_t kcnt = cnt + (keep_first ? 1u : 0u);
    // y of the last kept segment of the nearest lane in front that has one (or the carry's)
    int last_y_own = 0;
    if (kcnt) last_y_own = cnt ? jnn_ld<AGENT>(stage_y + cnt - 1) : fy;
    const unsigned long long nonempty = __ballot(kcnt != 0u);
    const unsigned long long before = nonempty & ((1ull << lane) - 1ull);
    const int src_prev = before ? 63 - __clzll((long long)before) : 0;
    int prev_y_in = __shfl(last_y_own, src_prev, 64);
    bool has_prev = before != 0ull;
    if (!has_prev) { prev_y_in = cy.y; has_prev = cy.has; }
    auto entry = [&](uint32_t k, int &x, int &y) {
        if (keep_first) {
            if (k == 0) { x = fx; y = fy; return; }
            --k;
        }
        x = jnn_ld<AGENT>(stage_x + k); y = jnn_ld<AGENT>(stage_y + k);
    };
    // pass 1: how many merged segments start in this lane; is this lane's first kept segment one of them?
    uint32_t nnew = 0u;
    bool first_is_new = false;
    {
        int py = prev_y_in;
        bool hp = has_prev;
        for (uint32_t k = 0; k < kcnt; ++k) {
            int x, y;
            entry(k, x, y);
            const bool nw = !hp || !(x - py < seg_dist);
            if (k == 0) first_is_new = nw;
            nnew += nw ? 1u : 0u;
            py = y; hp = true;
        }
    }
    const uint32_t incl = (uint32_t)wave_incl_scan_i((int)nnew), base = cy.idx + incl - nnew;
    const uint32_t total = (uint32_t)wave_last_i((int)incl);
    // the end of the last kept segment in front of this round, if this round's first kept segment opens a new merged one
    const int firstne = nonempty ? __ffsll((long long)nonempty) - 1 : -1;
    if (cy.has && lane == firstne && first_is_new && cy.idx - 1u < half) out_y[cy.idx - 1u] = cy.y;
    // is the kept segment behind this lane's last one the start of a new merged segment?  (the round's last kept
    // segment: decided by the next round or the flush)
    const unsigned long long after = lane == 63 ? 0ull : (nonempty & ~((2ull << lane) - 1ull));
    const int src_next = after ? __ffsll((long long)after) - 1 : 0;
    const bool next_new = __shfl(first_is_new ? 1 : 0, src_next, 64) != 0 && after != 0ull;
    // pass 2: x of every segment that starts a merged one, y of every segment that ends one
    {
        int py = prev_y_in;
        bool hp = has_prev;
        uint32_t idx = base;  // merged segments started so far (in front of and inside this lane)
        int x = 0, y = 0;
        if (kcnt) entry(0, x, y);
        for (uint32_t k = 0; k < kcnt; ++k) {
            const bool nw = !hp || !(x - py < seg_dist);
            if (nw) {
                if (idx < half) out_x[idx] = x; else overflow = true;
                ++idx;
            }
            int xn = 0, yn = 0;
            bool ends;
            if (k + 1 < kcnt) {
                entry(k + 1, xn, yn);
                ends = !(xn - y < seg_dist);
            } else ends = next_new;
            if (ends && idx - 1 < half) out_y[idx - 1] = y;
            py = y; hp = true;
            x = xn; y = yn;
        }
    }
    if (nonempty) {
        cy.y = __builtin_amdgcn_readlane(last_y_own, 63 - __clzll((long long)nonempty));
        cy.has = true;
    }
    cy.idx += total;
    cy.seen = cy.seen || hasf != 0ull;
    cy.overflow = cy.overflow || __any(overflow);
}
// the end of the read's last kept segment; returns the number of merged segments (JNN_REDO_MARK: the slots did not do)
__device__ inline uint32_t jnn_merge_flush(const JnnCarry &cy, int32_t *out_y, uint32_t half) {
    if (cy.has && lane_id() == 0 && cy.idx - 1u < half) out_y[cy.idx - 1u] = cy.y;
    return (cy.overflow || cy.idx > half) ? JNN_REDO_MARK : cy.idx;
}

// ---- tile masks: 1024 flags of a tile held as 16 bits per lane (k_polya_wave, adaptor_find)
// first set bit at tile-local position >= cur of the 1024-bit mask held as 16 bits per lane (-1: none)
__device__ __forceinline__ int mask_next(uint32_t m16, int cur) {
    const int lo = cur - lane_id() * SS_SPL;
    const uint32_t m = lo <= 0 ? m16 : (lo >= SS_SPL ? 0u : (m16 >> lo) << lo);
    const unsigned long long has = __ballot(m != 0u);
    if (!has) return -1;
    const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)has) - 1);
    return l * SS_SPL + __builtin_amdgcn_readlane(__ffs((int)m) - 1, l);
}
// last set bit at a tile-local position in [cur, hi) (-1: none)
__device__ __forceinline__ int mask_last(uint32_t m16, int cur, int hi) {
    const int lo = cur - lane_id() * SS_SPL, up = hi - lane_id() * SS_SPL;
    uint32_t m = lo <= 0 ? m16 : (lo >= SS_SPL ? 0u : (m16 >> lo) << lo);
    m = up >= SS_SPL ? m : (up <= 0 ? 0u : m & ((1u << up) - 1u));
    const unsigned long long has = __ballot(m != 0u);
    if (!has) return -1;
    const int l = __builtin_amdgcn_readfirstlane(63 - __clzll((long long)has));
    return l * SS_SPL + __builtin_amdgcn_readlane(31 - __clz((int)m), l);
}

// set bits of the tile mask (16 bits per lane) at tile-local positions >= cur
__device__ __forceinline__ uint32_t mask_from(uint32_t m16, int cur) {
    const int lo = cur - lane_id() * SS_SPL;
    return lo <= 0 ? m16 : (lo >= SS_SPL ? 0u : (m16 >> lo) << lo);
}
// position of the k-th (k >= 1) set bit at a position >= cur, given that there are at least k
__device__ __forceinline__ int mask_select(uint32_t m16, int cur, int k) {
    uint32_t m = mask_from(m16, cur);
    const int c = __popc(m), incl = wave_incl_scan_i(c), excl = incl - c;
    const unsigned long long own = __ballot(excl < k && incl >= k);
    const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)own) - 1);
    int kk = k - __builtin_amdgcn_readlane(excl, l);  // 1 .. 16, wave-uniform
    for (; kk > 1; --kk) m &= m - 1u;
    return l * SS_SPL + __builtin_amdgcn_readlane(__ffs((int)m) - 1, l);
}

__host__ __device__ inline JnnP jnn_polya_params() {  // JNNV1_R9_POLYA == JNNV1_RNA004_POLYA, src/jnn.h:52-72
    return JnnP{-1.0f, 50, 200, 250, 1.0f, 30, 0.0f, 0.0f};
}

// ---------------------------------------------------------------- find_polya, one WAVE per read
// jnn_pa on pA[adapt_y .. n) with the fixed thresholds of cfunc.c:191 and the polyA preset (src/jnn.h:52-72), first
// merged segment only.  x -> rm_outlierf(signal_in_picoamps(x)) is monotone in the raw value, so the in-range test
// bot < pA < top is an interval test on the raw sample (its bounds by bisection over the 65 536 raw values, with the
// float expression itself): no pA is formed.  With error = 30 the automaton has next to no sync points (31 out-of-range
// samples in a row), so instead of chunks the wave goes through the tail tile by tile (64 x 16 samples, coalesced) with
// the automaton's state in scalars and JUMPS: a segment opens at the next in-range sample and ends at the
// (error + 1 - err)-th out-of-range sample behind it, both found on the tile's 16-bit lane masks (next set bit; k-th set
// bit by a popcount scan).  It stops as soon as the first merged segment can no longer change -- usually after a few
// tiles, where the lane-per-read kernel waits for the slowest of 64 reads.
// (jnn_chunks was tried first for this: its chunks degenerate, 11.3 ms against the lane kernel's 5.8 ms on 50 000 reads.)
template <typename PRED>
__device__ inline int first_true_i16(PRED pred) {  // smallest v in [-32768, 32767] with pred(v), 32768 if none (pred monotone)
    int lo = -32768, hi = 32768;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pred(mid)) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// PARAM: the caller's set `q` (polya_wave_ok(q): stall_len 1, so that the first-segment rule is the window's, and error <
// corrector, so that the correction of jnn.c:228,238 cannot fire) in place of the preset and of 30 / 20
template <bool PARAM>
__global__ __launch_bounds__(256) void k_polya_wave_t(StatArgs a, PolyP q) {
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
    const uint32_t widx = blockIdx.x * 4 + wv;
    if (widx >= a.b.n_reads) return;
    const uint32_t r = a.order ? a.order[widx] : widx;
    const Region g = get_region(REG_TAIL, a.b, a.prefix, r);
    int px = -1, py = -1;
    if (g.len > 0) {
        const Scale sc = make_scale(a.b.digitisation[r], a.b.offset[r], a.b.range[r]);
        const float mid = a.prefix[r].adapt_mean + (PARAM ? q.shift : 30.0f);
        const float top = mid + (PARAM ? q.band : 20.0f), bot = mid - (PARAM ? q.band : 20.0f);
        const JnnP pp = PARAM ? q.p : jnn_polya_params();
        auto f = [&](int v) { return clampf_pa(to_pa((int16_t)v, sc)); };
        int vlo, vhi;  // in range <=> vlo <= raw <= vhi
        if (sc.unit >= 0.0f) {
            vlo = first_true_i16([&](int v) { return f(v) > bot; });
            vhi = first_true_i16([&](int v) { return !(f(v) < top); }) - 1;
        } else {
            vlo = first_true_i16([&](int v) { return f(v) < top; });
            vhi = first_true_i16([&](int v) { return !(f(v) > bot); }) - 1;
        }
        // a NaN anywhere (unit, offset, thresholds) makes every comparison of the reference false: nothing is in range
        if (!(sc.unit == sc.unit) || !(sc.offf == sc.offf) || !(top == top)) { vlo = 1; vhi = 0; }
        WaveRead wr;
        wr.init(a.b, g);
        const int hi_r = vhi + 1, lo_r = vlo - 1;  // in range <=> lo_r < raw < hi_r
        // automaton state (wave-uniform): open, errors so far, trailing tolerated errors, start; first merged segment
        int opn = 0, err = 0, run = 0, start = 0, last_y = 0;
        bool found = false, done = false;
        WaveTile cur_t, nxt_t;
        wr.load(cur_t, 0);
        for (int t = 0; t < wr.ntiles && !done; ++t) {
            if (t + 1 < wr.ntiles) wr.load(nxt_t, t + 1);
            int q_lo, q_hi;
            wr.range(t, 0, q_lo, q_hi);
            uint32_t inm = 0u;
#pragma unroll
            for (int e = 0; e < SS_SPL; ++e) {
                const int iv = (e & 1) ? (int)(int16_t)(cur_t.w[e / 2] >> 16) : (int)(int16_t)(cur_t.w[e / 2] & 0xffffu);
                inm |= ((uint32_t)((iv - hi_r) & (lo_r - iv)) >> 31) << e;
            }
            const int l0 = q_lo - lane * SS_SPL, l1 = q_hi - lane * SS_SPL;
            uint32_t vm = l0 <= 0 ? 0xffffu : (l0 >= SS_SPL ? 0u : (0xffffu >> l0) << l0);
            vm = l1 >= SS_SPL ? vm : (l1 <= 0 ? 0u : vm & ((1u << l1) - 1u));
            inm &= vm;
            const uint32_t outm = ~inm & vm;
            const int jbase = t * SS_TILE - wr.skip;  // sample index (in the tail) of tile-local position 0
            int cur = q_lo;
            for (;;) {
                if (!opn) {
                    const int ps = mask_next(inm, cur);
                    if (ps < 0) break;
                    start = jbase + ps; opn = 1; err = 0; run = 0; cur = ps + 1;
                } else {
                    const int need = pp.error + 1 - err;
                    const int pc = wave_last_i(wave_incl_scan_i(__popc(mask_from(outm, cur))));
                    if (pc < need) {  // the segment outlives the tile
                        err += pc;
                        const int li = mask_last(inm, cur, q_hi);
                        run = li >= 0 ? q_hi - 1 - li : run + (q_hi - cur);
                        break;
                    }
                    const int pe = mask_select(outm, cur, need);
                    const int li = mask_last(inm, cur, pe);
                    const int perr = li >= 0 ? pe - 1 - li : run + (pe - cur);
                    const int i = jbase + pe, end = i - perr;
                    if (i - start >= pp.window) {  // kept (stall_len = 1: the first-segment rule is the same)
                        if (!found) { px = start; py = end; found = true; }
                        else if (start - last_y < pp.seg_dist) py = end;
                        else { done = true; break; }  // the first merged segment is final
                        last_y = end;
                    }
                    opn = 0; err = 0; run = 0; cur = pe + 1;
                }
            }
            cur_t = nxt_t;
        }
    }
    if (lane == 0) {
        a.prefix[r].polya_x = px;
        a.prefix[r].polya_y = py;
    }
}
// ---------------------------------------------------------------- find_adaptor / jnnv2, one WAVE per read
// Same arithmetic as k_adaptor, laid out as k_stat_wave: tiles of 64 x SS_SPL window indices; a lane holds the trailing
// samples x[i..i+16) and the leading samples x[i+2000..i+2016) of its 16 indices, forms the 16 differences of the
// clamped values (packed 16-bit), a DPP scan of the lanes' difference sums gives every lane its first rolling total
// (integers: exact in any order), and the sequential float sums of the rolling means (src/jnn.c:106-107) advance through
// seqsum.h.  Three passes: sum of the means; sum of their squared deviations; the run finder (src/jnn.c:126-158), whose
// state only changes where the below / above-threshold flags flip: the wave jumps from flip to flip over 16-bit lane
// masks and stops at the first qualifying segment that can no longer change.
// rolling totals of this lane's 16 window indices.  T0: total of the tile's first index (wave-uniform), advanced to
// the next tile's.  d_lo: tile-local indices below it have no difference (they lie in front of the read).
// (CLAMPED: the tiles hold rm_outlier of the samples already, roll_sweep)
template <bool MASKED, bool CLAMPED = false>
__device__ __forceinline__ void roll_tile(const WaveTile &trail, const WaveTile &lead, int d_lo, int &T0, int (&tot)[SS_SPL]) {
    const int q0 = lane_id() * SS_SPL;
    int run = 0;
#pragma unroll
    for (int k = 0; k < SS_SPL / 2; ++k) {
        const s16x2 d = CLAMPED ? __builtin_bit_cast(s16x2, lead.w[k]) - __builtin_bit_cast(s16x2, trail.w[k])
                                : clamp_raw2(lead.w[k]) - clamp_raw2(trail.w[k]);
        int d0 = (int)d.x, d1 = (int)d.y;
        if (MASKED) {
            d0 = (q0 + 2 * k >= d_lo) ? d0 : 0;
            d1 = (q0 + 2 * k + 1 >= d_lo) ? d1 : 0;
        }
        tot[2 * k] = run;
        run += d0;
        tot[2 * k + 1] = run;
        run += d1;
    }
    const int incl = wave_incl_scan_i(run);
    const int base = T0 + incl - run;
#pragma unroll
    for (int e = 0; e < SS_SPL; ++e) tot[e] += base;
    T0 += wave_last_i(incl);
}

// total of the ADW clamped samples that start at tile-local position lo0 (< SS_TILE) of tile t: the rolling total of
// the window that starts there (tiles t and t + 1 hold all of it)
__device__ __forceinline__ int window_total(const WaveRead &wr, int t, int lo0) {
    const int q0 = lane_id() * SS_SPL;
    int part = 0;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        WaveTile w;
        wr.load(w, t + tt);
        const int lo = lo0 - tt * SS_TILE, hi = lo0 + ADW - tt * SS_TILE;
#pragma unroll
        for (int k = 0; k < SS_SPL / 2; ++k) {
            const s16x2 c = clamp_raw2(w.w[k]);
            part += (q0 + 2 * k >= lo && q0 + 2 * k < hi) ? (int)c.x : 0;
            part += (q0 + 2 * k + 1 >= lo && q0 + 2 * k + 1 < hi) ? (int)c.y : 0;
        }
    }
    return wave_last_i(wave_incl_scan_i(part));
}
// the trailing and the leading tile of window tile t
__device__ __forceinline__ void roll_load(const WaveRead &wr, WaveTile &x, WaveTile &y, int t) {
    const int64_t tile0 = wr.rb + (int64_t)t * SS_TILE;
    wt_load(x, wr.samples, wr.n_total, tile0);
    wt_load(y, wr.samples, wr.n_total, tile0 + ADW);
}
// one tile of a chain over the terms term(rolling total)
template <typename TERM>
__device__ __forceinline__ void roll_chain_tile(float &acc, const WaveRead &wr, int t, const int (&tot)[SS_SPL], TERM term) {
    const int q0 = lane_id() * SS_SPL;
    int q_lo, q_hi;
    float x[SS_SPL];
    if (t == 0) {  // head, natively
        wr.range(0, 0, q_lo, q_hi);
        const int qh = q_lo + wr.head();
#pragma unroll
        for (int e = 0; e < SS_SPL; ++e) x[e] = (q0 + e >= q_lo && q0 + e < qh) ? term(tot[e]) : 0.0f;
        if (qh > q_lo) acc = ss_serial(acc, TermArr{x}, q_lo / SS_SPL, (qh - 1) / SS_SPL);
    }
    wr.range(t, t == 0 ? wr.head() : 0, q_lo, q_hi);
    if (wr.interior(t)) {
#pragma unroll
        for (int e = 0; e < SS_SPL; ++e) x[e] = term(tot[e]);
    } else {
        const int q0e = q0 + ss_edge_zero();  // (keeps the compares inside this branch, see ss_tile1)
#pragma unroll
        for (int e = 0; e < SS_SPL; ++e) x[e] = (q0e + e >= q_lo && q0e + e < q_hi) ? term(tot[e]) : 0.0f;
    }
    const SsWalk w = ss_walk<false>(acc, TermArr{x});
    int sk;
    if (ss_fast<false>(acc, w, TermArr{x}, sk)) acc = ss_finish<false>(acc, TermArr{x}, w, sk);
}

// one sweep over the rolling totals of the windows of wr: f(t, tot) per tile; stops when f returns true.
// `ring` (round 5; nullptr: every trailing tile is loaded from memory): 3 x 2 KB of LDS of this wave's.  The trailing tile
// of window tile t + 1 is what the wave loaded as LEADING tiles t - 1 and t (ADW = 2 000 = 2 x 1 024 - 48 samples: lane l's
// 16 trailing samples are lane l + 3's of leading tile t - 1, the last three lanes' are lanes 0 .. 2's of tile t), so the
// leading tiles go through a ring and the trailing ones come out of it: at 125 000 x 100 000 the second read missed the L2
// for 36 % of its lines (67.9 GB fetched for two passes of 25 GB and a partial third).
constexpr int ROLL_RING_TILES = 3;
constexpr int ROLL_RING_BYTES = ROLL_RING_TILES * SS_TILE * (int)sizeof(int16_t);
static_assert(2 * SS_TILE - ADW == 3 * SS_SPL && ADW > SS_TILE, "the lane shift of the trailing tile");
template <typename F>
__device__ __forceinline__ void roll_sweep(const WaveRead &wr, int first_total, F f, uint4 *ring = nullptr) {
    int T0 = first_total;
    const int lane = lane_id();
    // the tiles are kept clamped (rm_outlier, two samples per instruction): a tile is clamped once, as a leading tile
    auto clamp_tile = [](WaveTile &x) {
#pragma unroll
        for (int k = 0; k < SS_SPL / 2; ++k) x.w[k] = __builtin_bit_cast(uint32_t, clamp_raw2(x.w[k]));
    };
    WaveTile tr, ld, trn, ldn;
    roll_load(wr, tr, ld, 0);
    clamp_tile(tr);
    clamp_tile(ld);
    for (int t = 0; t < wr.ntiles; ++t) {
        const bool more = t + 1 < wr.ntiles;
        const bool from_ring = ring != nullptr && t + 1 >= 2;
        if (ring) {
            uint4 *row = ring + (t % ROLL_RING_TILES) * (SS_TILE / 8) + lane * 2;
            row[0] = make_uint4(ld.w[0], ld.w[1], ld.w[2], ld.w[3]);
            row[1] = make_uint4(ld.w[4], ld.w[5], ld.w[6], ld.w[7]);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        if (more) {
            const int64_t tile0 = wr.rb + (int64_t)(t + 1) * SS_TILE;
            if (!from_ring) wt_load(trn, wr.samples, wr.n_total, tile0);
            wt_load(ldn, wr.samples, wr.n_total, tile0 + ADW);
        }
        int tot[SS_SPL];
        if (t == 0 && wr.skip > 0) roll_tile<true, true>(tr, ld, wr.skip, T0, tot);
        else roll_tile<false, true>(tr, ld, 0, T0, tot);
        if (f(t, tot)) break;
        if (more) {
            clamp_tile(ldn);
            if (!from_ring) clamp_tile(trn);
        }
        if (more && from_ring) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int src = lane + 3;
            const uint4 *row = src < 64 ? ring + ((t + 2) % ROLL_RING_TILES) * (SS_TILE / 8) + src * 2   // tile t - 1
                                        : ring + (t % ROLL_RING_TILES) * (SS_TILE / 8) + (src - 64) * 2;  // tile t
            const uint4 q0 = row[0], q1 = row[1];
            trn.w[0] = q0.x; trn.w[1] = q0.y; trn.w[2] = q0.z; trn.w[3] = q0.w;
            trn.w[4] = q1.x; trn.w[5] = q1.y; trn.w[6] = q1.z; trn.w[7] = q1.w;
        }
        tr = trn; ld = ldn;
    }
    if (ring) {  // the next sweep's rows are written behind this one's reads
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}
// what find_adaptor leaves in a read's record before anything is found (lane 0)
__device__ __forceinline__ void adaptor_init_rec(sgk_prefix_rec_t *o, int64_t n) {
    o->n = (uint32_t)n;
    o->reserved = 0;
    o->polya_x = -1; o->polya_y = -1;
    o->adapt_mean = 0.0f; o->adapt_std = 0.0f; o->adapt_median = 0.0f;
    o->polya_mean = 0.0f; o->polya_std = 0.0f; o->polya_median = 0.0f;
}
// jnnv2's thresholds from the two sums over the m rolling means (src/jnn.c:106-124) and its run finder (k_adaptor's RunFinder,
// src/jnn.c:126-167) from flip to flip, by one wave; writes adapt_x / adapt_y
// WS: the window source (stat_device.h); sweep(f): one sweep over the rolling totals of the windows of wr, as roll_sweep
template <typename WS, typename SWEEP>
__device__ __forceinline__ void adaptor_find_ws(const WaveRead &wr, float s, float q, float mf, const AdaptP &ap,
                                                sgk_prefix_rec_t *o, const WS ws, SWEEP sweep) {
    const int lane = lane_id(), q0 = lane * SS_SPL;
    const float mn = s / mf;
    const float sd = sqrtf(q / mf);
    const float bot = mn - sd * ap.std_scale;
    const int t_lt = roll_threshold(bot, false, ws), t_gt = roll_threshold(bot, true, ws);
    int in_run = 0, start = 0, end = 0, nseg = 0, last_x = 0, last_y = 0, ans_x = 0, ans_y = 0, found = 0;
    auto settle = [&]() {
        const int len = last_y - last_x;
        if (!found && !(len > ap.hi_thresh) && !(len < ap.lo_thresh)) { found = 1; ans_x = last_x; ans_y = last_y; }
    };
    sweep([&](int t, const int (&tot)[SS_SPL]) {
        int q_lo, q_hi;
        wr.range(t, 0, q_lo, q_hi);
        uint32_t bm = 0u, am = 0u;
#pragma unroll
        for (int e = 0; e < SS_SPL; ++e) {
            bm |= (uint32_t)((tot[e] - t_lt) >> 31) & (1u << e);       // tot < t_lt
            am |= ~(uint32_t)((tot[e] - t_gt) >> 31) & (1u << e);      // tot >= t_gt
        }
        const int lo = q_lo - q0, hi = q_hi - q0;
        uint32_t vm = lo <= 0 ? 0xffffu : (lo >= SS_SPL ? 0u : (0xffffu >> lo) << lo);
        vm = hi >= SS_SPL ? vm : (hi <= 0 ? 0u : vm & ((1u << hi) - 1u));
        bm &= vm; am &= vm;
        const int jbase = t * SS_TILE - wr.skip;  // window index of tile-local position 0
        int cur = 0;
        for (;;) {
            if (!in_run) {
                const int p = mask_next(bm, cur);
                if (p < 0) break;
                start = jbase + p; in_run = 1; cur = p + 1;
            } else {
                const int pa = mask_next(am, cur);
                const int pb = mask_last(bm, cur, pa < 0 ? SS_TILE : pa);
                if (pb >= 0) end = jbase + pb;
                if (pa < 0) break;
                if (nseg > 0 && start - last_y < ap.seg_dist) last_y = end;
                else {
                    if (nseg > 0) settle();
                    last_x = start; last_y = end; ++nseg;
                }
                start = 0; end = 0; in_run = 0; cur = pa + 1;
                if (found) break;
            }
        }
        return found != 0;
    });
    if (nseg > 0) settle();
    if (lane == 0) {
        if (found) { o->adapt_x = ans_x + ws.w() / 2 - 1; o->adapt_y = ans_y + ws.w() / 2 - 1; }
        else { o->adapt_x = 0; o->adapt_y = 0; }
    }
}
__device__ inline void adaptor_find(const WaveRead &wr, int first_total, float s, float q, float mf, const AdaptP &ap,
                                    sgk_prefix_rec_t *o, uint4 *ring = nullptr) {
    adaptor_find_ws(wr, s, q, mf, ap, o, WinPreset{}, [&](auto f) { roll_sweep(wr, first_total, f, ring); });
}

}  // namespace sgk
