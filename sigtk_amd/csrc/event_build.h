// event_build.h -- the builder of the `event` path: peak bitmap + samples -> event table (events.c:457-504), one wave
// per read or per segment of a read.  The map of the event units is in event_device.h.
#pragma once
#include <type_traits>

#include "event_detect.h"

namespace sgk {

constexpr int BT = 32;      // samples per lane per builder tile: 64 bytes of int16, one 32-bit bitmap word
// create_event (events.c:457-473) for the fast builder: the two divisions by the event length share one refined
// reciprocal (tstat_math.h: bit-identical to `/` inside the range guard); one 16-byte store per event.
struct EvOut {
    uint4 *ev;   // the read's first slot
    uint32_t cap;
#ifdef SGK_DEV
    bool raw;    // SGK_DEV_RAW_EVENTS
#endif
};
__device__ __forceinline__ void store_event_fast(const EvOut &o, uint32_t k, uint32_t ps, uint32_t pe, double dsum,
                                                 double dsumsq, bool &overflow) {
    if (k >= o.cap) { overflow = true; return; }
#ifdef SGK_DEV
    if (o.raw) {
        uint4 e;
        e.x = ps; e.y = pe - ps; e.z = __float_as_uint((float)dsum); e.w = __float_as_uint((float)dsumsq);
        o.ev[k] = e;
        return;
    }
#endif
    const float len = (float)(pe - ps);
    const float r1 = sgk_refined_rcp(len);
    const float m = sgk_div_with_rcp((float)dsum, len, r1);
    const float var = sgk_div_with_rcp((float)dsumsq, len, r1) - m * m;
    // certified square root (tstat_math.h); the two conditions meet as lane masks, the rare lane takes sqrtf
    const float v = fmaxf(var, 0.0f);
    bool dom_ok, cert_ok;
    float sd = sgk_sqrt_cert(v, dom_ok, cert_ok);
    const lmask_t sq_ok = __ballot(dom_ok) & __ballot(cert_ok);
    if (!lane_of(sq_ok)) {
        __asm__ volatile("" ::: "memory");  // a real branch: if-converted, every lane would evaluate both forms
        sd = sqrtf(v);
    }
    uint4 e;
    e.x = ps;
    e.y = pe - ps;
    e.z = __float_as_uint(m);
    e.w = __float_as_uint(sd);
    o.ev[k] = e;
}

// Boundary records per tile in LDS: {S, S2} as one 16-byte record + a 16-bit tile-relative position (10.6 KB per
// wave with the lane prefixes).  The detector can emit a boundary every 3 samples (683 per tile), but sizing LDS for
// that costs occupancy; a tile with more than BREC boundaries (events shorter than 3.6 samples on average over 2048
// samples: never seen on nanopore data, sp1 peaks at 425) sends its read to k_event_fallback instead.
constexpr int BREC = 576;
struct __attribute__((aligned(16))) BuildRec {
    double S, S2;
};
// NPT: lane prefixes kept.  The carrying builder (SGK_BUILD_CARRY below) keeps 128: the tile's 64 behind 64 zeros, the
// entries that the leftover records of the previous tile look up (their prefix is folded in already).
template <int NPT>
struct BuildLdsT {
    BuildRec rec[BREC];
    double pt[NPT];
    double pt2[NPT];
    uint16_t p[BREC];  // tile-relative sample index of the boundary (carrying builder: + 2048; a leftover's is below 2048)
};
typedef BuildLdsT<64> BuildLds;
typedef BuildLdsT<128> BuildLdsCarry;
static_assert(sizeof(BuildLds) <= 11776, "builder LDS budget: 13 waves per CU");
// 12 workgroups of k_event<3, *> (3 waves per SIMD) share the CU's 160 KB: 13 653 bytes each, 13 312 in whole 512-byte
// blocks.  (The kernels' LDS is the union with the detector's LzLds, 12 544 bytes: the zeros fit under it.)
static_assert(sizeof(BuildLdsCarry) <= 13312, "carrying builder LDS budget: 12 workgroups per CU");

// The builder's form per kernel (tools/build_variant.sh <tag> -DSGK_BUILD_CARRY=<bits>; 0: every tile runs
// ceil(records / 64) rounds and starts again): 1 k_event<3, *>, 2 the other unflagged kernels (k_event<7, *>,
// k_event_seg, k_event_multi).  In the carrying form a tile runs its full rounds only and leaves the records that remain
// in LDS for the next tile's; profiles/event_rounds.md has what each form showed.
#ifndef SGK_BUILD_CARRY
#define SGK_BUILD_CARRY 1
#endif

// value of lane l-1, lane 0 receives lane 63's (wave rotate right by one lane, DPP wave_ror:1; every lane has a source)
__device__ __forceinline__ int wave_ror1_i(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x13C, 0xf, 0xf, true); }
__device__ __forceinline__ double wave_ror1_d(double v) {
    return __hiloint2double(wave_ror1_i(__double2hiint(v)), wave_ror1_i(__double2loint(v)));
}

typedef short sgk_s2 __attribute__((ext_vector_type(2)));

// One lane's walk over its 32 samples of a tile: lane-relative double prefix sums, one record per boundary bit.
// FULL: every sample of the tile is inside the read (no per-sample validity select).
// A lane's 32 samples of a tile AS THEY SIT IN MEMORY (16 dwords of packed int16, or 32 floats).  Kept packed on purpose:
// as an array of 32 int16 elements the compiler gives every sample a register of its own and unpacks the high halves
// right behind the load -- an s_waitcnt vmcnt directly after the "prefetch" of the next tile, i.e. no prefetch at all
// (round 5: the whole memory latency was exposed once per tile).  The walk converts straight from the packed words
// (v_cvt_f32_i32_sdwa).
template <typename T>
struct TileRegs {
    static constexpr int NW = BT * (int)sizeof(T) / 4;
    uint32_t w[NW];
    __device__ __forceinline__ float pa(int k, const Scale &sc) const {   // k: a constant after unrolling
        if constexpr (std::is_same<T, int16_t>::value) {
            const int v = (k & 1) ? ((int)w[k / 2] >> 16) : (int)(short)(w[k / 2] & 0xffffu);
            return ((float)v + sc.offf) * sc.unit;
        } else {
            return __uint_as_float(w[k]);
        }
    }
};
template <typename T, bool FULL, typename LDS>
__device__ __forceinline__ void build_walk(const TileRegs<T> &buf, uint32_t bits, int nvalid, const Scale &sc, int l,
                                           int excl, LDS *L, double &S, double &S2, uint32_t &mnb,
                                           uint32_t &mxb) {
    // (LDS addresses as 32-bit offsets: what ds_write takes)
    typedef __attribute__((address_space(3))) char *LdsBytes;
    typedef __attribute__((address_space(3))) uint16_t *LdsU16;
    uint32_t rr32 = (uint32_t)(uintptr_t)(LdsBytes)(char *)L->rec + (uint32_t)excl * 16u;
    uint32_t rp32 = (uint32_t)(uintptr_t)(LdsBytes)(char *)L->p + (uint32_t)excl * 2u;
    // The boundary bits are taken from the top of the reversed word: doubling it hands the next bit out as the carry, a
    // lane mask in scalar registers from one add (v_add_co_u32) instead of v_and_b32 + v_cmp_ne_u32 per sample.
    uint32_t rbits = __builtin_bitreverse32(bits);
#pragma unroll
    for (int k = 0; k < BT; ++k) {
        float x = buf.pa(k, sc);
        if (!FULL && k >= nvalid) x = 0.0f;
        const float xq = x * x;
        if constexpr (std::is_same<T, float>::value) {
            // pA input: the guard's extremes are tracked on the bit patterns (non-negative floats order like
            // unsigned integers; zero - 1 wraps to the top, so it never wins the minimum; inf / nan end up above
            // every finite value and fail the guard)
            const uint32_t ab = __float_as_uint(x) & 0x7fffffffu;
            mxb = ab > mxb ? ab : mxb;
            mnb = (ab - 1u) < mnb ? (ab - 1u) : mnb;
        }
        lmask_t bnd;
        asm("v_add_co_u32 %0, %1, %0, %0" : "+v"(rbits), "=s"(bnd));
        if (lane_of(bnd)) {
            typedef double __attribute__((ext_vector_type(2))) sgk_d2;
            *(__attribute__((address_space(3))) sgk_d2 *)(uintptr_t)rr32 = sgk_d2{S, S2};   // BuildRec {S, S2}
            *(LdsU16)(uintptr_t)rp32 = (uint16_t)(l * BT + k);
            // (in place, under the lane mask: written as `rr += 16` the two pointers come out as an add into a new
            // register plus a move each -- four vector instructions per sample instead of two)
            asm volatile("v_add_u32 %0, 16, %0\n\tv_add_u32 %1, 2, %1" : "+v"(rr32), "+v"(rp32));
        }
        S = S + (double)x;
        S2 = S2 + (double)xq;
    }
}

// SEG: the wave builds the events of one segment [seg_a, seg_b) of a long read (several waves share the read): the
// events that END at a boundary inside the segment, and the read's last event if the segment is the read's last.
// It walks from the last boundary in front of the segment (prev_p; none: from the read's start), at the event rank the
// boundaries in front give (cnt_before); extremes and flags go to st, the read's verdict is chain_segment's.  In front
// of the segment the bitmap words are another wave's: the only boundaries the walk knows there are the one it starts
// at (prev_p) and the ones this segment owns (pre: peaks that were pending at the seam).
//
// CARRY (SGK_BUILD_CARRY): a round emits one event per lane, so the records of a tile that do not fill a round -- 19 of 64
// lanes on average on DNA reads -- wait in LDS for the next tile's instead of taking a round of their own.  They are
// moved to the front of the record arrays with their lane prefix folded in and rebased to the next tile's start (exact
// under the guard, like the carry), and their position falls below 2048, where the look-up of the lane prefix finds
// zeros.  The next tile's walk writes behind them.  Only a read's (a segment's) last tile runs a partial round -- and a
// tile that ends with fewer than 64 records, some of them leftovers already: a leftover is never older than one tile,
// which is what its 16-bit position and the 64 zeros can express.  With full rounds lane 0's previous boundary is lane
// 63's of the round before: a wave rotate by one lane, no v_readlane.
template <typename T, bool SEG = false, bool CARRY = false>
__device__ __forceinline__ void build_read(const EvArgs &a, const ReadCtx<T> &rc, uint32_t r,
                           BuildLdsT<CARRY ? 128 : 64> *L, bool declined,
                           int64_t seg_a = 0, int64_t seg_b = 0, SegState *st = nullptr, uint32_t cnt_before = 0,
                           int prev_p = -1, const int *pre = nullptr, int n_pre = 0) {
    const int64_t n = rc.n;
    const int l = lane_id();
    const uint64_t slot0 = a.ev_slots[r], cap = a.ev_slots[r + 1] - slot0;
    if (n <= 0) {
        if (l == 0) { a.n_events[r] = 0; a.flags[r] = 0; }
        return;
    }
    const uint32_t *bm32 = reinterpret_cast<const uint32_t *>(rc.bm);
    {
        const uint32_t pol = prio_policy(a.dev);
        if (pol == 2u || pol == 3u) __builtin_amdgcn_s_setprio(3);
        else if (pol == 1u) __builtin_amdgcn_s_setprio(0);
    }
    EvOut eo;
    eo.ev = reinterpret_cast<uint4 *>(a.events + slot0);
    eo.cap = cap > 0xffffffffull ? 0xffffffffu : (uint32_t)cap;
#ifdef SGK_DEV
    eo.raw = (a.dev & SGK_DEV_RAW_EVENTS) != 0u;
#endif
    bool overflow = false, dense = false;
    uint32_t rank = 0, prevp = 0;
    // SEG: bits in [bit_lo, bit_hi) count; the first of them (the boundary in front of the segment) ends no event of
    // this segment: its record only starts the next one
    int64_t bit_lo = 0, bit_hi = n, walk0 = 0;
    uint32_t skip_rank = 0xffffffffu;
    if constexpr (SEG) {
        bit_hi = seg_b;
        if (prev_p >= 0) {
            bit_lo = prev_p;
            walk0 = bit_lo & ~(int64_t)31;
            rank = cnt_before - 1u;
            skip_rank = rank;
        }
    }
    double Gprev = 0.0, G2prev = 0.0;  // prefix sums at the previous boundary, relative to the current tile start
    // CARRY: prevp / Gprev / G2prev are lane 0's (the only lane that takes them); m records wait in front of L->rec
    int m = 0;
    if constexpr (CARRY) {
        L->pt[l] = 0.0;
        L->pt2[l] = 0.0;
    }
    // exactness guard inputs: int16 reads track the extremes of the RAW samples (packed 16-bit min / max, two samples
    // per instruction); pA reads the extremes of the float bit patterns
    uint32_t mnb = 0xffffffffu, mxb = 0u;
    sgk_s2 rmin2 = {32767, 32767}, rmax2 = {-32768, -32768};
    constexpr int NV = BT * (int)sizeof(T) / 16;
    // tile loader: this lane's 32 samples and its 32 bitmap bits.  The next tile is fetched while the
    // current one is processed (register double buffer).
    // (bits of the tile = (raw & keep) | extra: the masks are formed WITHOUT touching the loaded word, so that nothing waits
    // for the load where it is issued -- one `bits &= mask` here put an s_waitcnt vmcnt(0) right behind the prefetch)
    auto load_tile = [&](int64_t tb, TileRegs<T> &buf, uint32_t &raw, uint32_t &keep, uint32_t &extra, int &nvalid) {
        const int64_t pos0 = tb + (int64_t)l * BT;
        raw = (pos0 < n) ? bm32[pos0 >> 5] : 0u;
        keep = 0xffffffffu;
        extra = 0u;
        const int64_t rem = n - pos0;
        nvalid = rem <= 0 ? 0 : (rem >= BT ? BT : (int)rem);
        if (nvalid < BT) keep = (nvalid == 0) ? 0u : ((1u << nvalid) - 1u);
        if constexpr (SEG) {
            if (pos0 < seg_a) {
                uint32_t sb = 0u;
                if (prev_p >= pos0 && prev_p < pos0 + BT) sb |= 1u << (int)(prev_p - pos0);
                for (int k = 0; k < n_pre; ++k) {
                    const int64_t q = pre[k];
                    if (q >= pos0 && q < pos0 + BT) sb |= 1u << (int)(q - pos0);
                }
                extra = sb & keep;
                keep = 0u;
            }
            const int64_t dl = bit_lo - pos0, dh = bit_hi - pos0;
            uint32_t m = 0xffffffffu;
            if (dl > 0) m = dl >= BT ? 0u : ~((1u << (int)dl) - 1u);
            if (dh < BT) m = dh <= 0 ? 0u : (m & ((1u << (int)dh) - 1u));
            keep &= m;
            extra &= m;
        }
        if (pos0 >= n) {
            // lanes behind the read's end (every read's last tile has some): nothing to load
#pragma unroll
            for (int k = 0; k < TileRegs<T>::NW; ++k) buf.w[k] = 0u;
        } else if (rc.vec_ok && pos0 + BT <= rc.hi) {
            const uint4 *src = reinterpret_cast<const uint4 *>(rc.base + pos0);
            uint4 v[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) v[k] = src[k];
            __builtin_memcpy(buf.w, v, sizeof(buf.w));
        } else {
            // (a read on an odd address / at the end of the buffer: element by element, packed by hand -- both branches
            // must define the same dwords, or the compiler unpacks the vector loads to match this one)
            if constexpr (std::is_same<T, int16_t>::value) {
#pragma unroll
                for (int k = 0; k < BT; k += 2) {
                    const uint32_t lo = (k < nvalid) ? (uint32_t)(uint16_t)rc.base[pos0 + k] : 0u;
                    const uint32_t hi = (k + 1 < nvalid) ? (uint32_t)(uint16_t)rc.base[pos0 + k + 1] : 0u;
                    buf.w[k / 2] = lo | (hi << 16);
                }
            } else {
#pragma unroll
                for (int k = 0; k < BT; ++k) buf.w[k] = (k < nvalid) ? __float_as_uint(rc.base[pos0 + k]) : 0u;
            }
        }
    };
    TileRegs<T> nbuf;
    uint32_t nraw, nkeep, nextra;
    int nnvalid;
    load_tile(walk0, nbuf, nraw, nkeep, nextra, nnvalid);
    for (int64_t tb = walk0; tb < bit_hi; tb += 64 * BT) {
        const TileRegs<T> buf = nbuf;
        const uint32_t bits = (nraw & nkeep) | nextra;
        const int nvalid = nnvalid;
        if (tb + 64 * BT < bit_hi) load_tile(tb + 64 * BT, nbuf, nraw, nkeep, nextra, nnvalid);
        const int cnt = __popc(bits);
        const int incl = wave_incl_scan_i(cnt);
        const int excl = incl - cnt;
        const int total = wave_last_i(incl);
        const bool full = tb + 64 * BT <= n;
        if constexpr (std::is_same<T, int16_t>::value) {
            // raw extremes (samples behind the read's end repeat a valid one)
            sgk_s2 w[BT / 2];
            __builtin_memcpy(w, buf.w, sizeof(w));
            if (!full) {
                const sgk_s2 first = {(short)rc.base[0], (short)rc.base[0]};
#pragma unroll
                for (int k = 0; k < BT / 2; ++k) {
                    if (2 * k + 1 >= nvalid) w[k] = (2 * k >= nvalid) ? first : sgk_s2{w[k].x, w[k].x};
                }
            }
#pragma unroll
            for (int k = 0; k < BT / 2; ++k) {
                rmin2 = __builtin_elementwise_min(rmin2, w[k]);
                rmax2 = __builtin_elementwise_max(rmax2, w[k]);
            }
        }
        // walk: lane-relative prefix sums, boundary records.  A tile with more than BREC boundaries is not recorded:
        // its read is redone by the fallback.
        double S = 0.0, S2 = 0.0;
        // (CARRY: the leftovers count: total + m; the records go behind them, positions and lane prefixes 64 lanes up)
        const bool toomany = CARRY ? total + m > BREC : total > BREC;
        if (toomany) dense = true;
        const uint32_t wbits = toomany ? 0u : bits;
        const int wl = CARRY ? l + 64 : l, wexcl = CARRY ? excl + m : excl;
        if (full) build_walk<T, true>(buf, wbits, nvalid, rc.sc, wl, wexcl, L, S, S2, mnb, mxb);
        else build_walk<T, false>(buf, wbits, nvalid, rc.sc, wl, wexcl, L, S, S2, mnb, mxb);
        const double inS = wave_incl_scan_d(S), inS2 = wave_incl_scan_d(S2);
        L->pt[wl] = inS - S;
        L->pt2[wl] = inS2 - S2;
        const double tileS = wave_last_d(inS), tileS2 = wave_last_d(inS2);
        __syncthreads();
        // The next tile's samples and bitmap word were requested before the walk and have long arrived: say so HERE,
        // in front of the rounds' event stores.  Left to the compiler the wait sits at their first use -- behind those
        // stores, and vmcnt counts loads and stores in one queue on gfx9: every tile would wait for its events to be
        // acknowledged by memory.  (vmcnt(0), expcnt / lgkmcnt untouched)
        __builtin_amdgcn_s_waitcnt(0x0F70);
#ifdef SGK_DEV
        const int tot = (toomany || (a.dev & SGK_DEV_NO_ROUNDS)) ? 0 : total + m;
#else
        const int tot = toomany ? 0 : total + m;
#endif
        // one event per lane per round.  Prefix sums are kept relative to the tile start (exact under the guard, so
        // no absolute base is needed); the previous boundary of lane l is lane l-1's record, lane 0 takes the
        // carry: the last record of the previous round / tile.
        // The LDS look-ups of a round are two dependent trips (position -> lane -> that lane's prefix); they run two
        // rounds ahead of the arithmetic (round 5: the rounds were 0.41 ms for 7.3 vector instructions per sample --
        // waits, profiles/r05_event_instruction_table.md): records of round i + 2 and lane prefixes of round i + 1 are
        // in flight while round i is evaluated.
        auto rec_at = [&](int k0, uint32_t &pr, double &S_, double &S2_) {
            const int k = k0 + l;
            const int kk = k < tot ? k : tot - 1;
            pr = L->p[kk];
            const BuildRec rcd = L->rec[kk];
            S_ = rcd.S;
            S2_ = rcd.S2;
        };
        uint32_t pr0 = 0u, pr1 = 0u, pr2 = 0u;
        double S0 = 0.0, S20 = 0.0, S1 = 0.0, S21 = 0.0, Sn = 0.0, S2n = 0.0, pt0 = 0.0, pt20 = 0.0, pt1 = 0.0, pt21 = 0.0;
        if (tot > 0) {
            rec_at(0, pr0, S0, S20);
            rec_at(64, pr1, S1, S21);
            pt0 = L->pt[pr0 / BT];
            pt20 = L->pt2[pr0 / BT];
        }
        if constexpr (CARRY) {
            // positions carry + 2048 (a leftover's, relative to the tile before, is below it)
            const uint32_t tbm = (uint32_t)tb - (uint32_t)(64 * BT);
            const bool partial = tb + 64 * BT >= bit_hi || (m > 0 && tot < 64);
            const int nfull = tot & ~63, mleft = tot - nfull;
            // A round leaves position and sums of the next one's records behind ({p, G, G2}: formed where the look-ups
            // it issued at its start have arrived), so the look-ups themselves are not handed from round to round.
            uint32_t p = tbm + pr0;
            double G = pt0 + S0, G2 = pt20 + S20;
            for (int k0 = 0; k0 < nfull; k0 += 64) {
                pt1 = L->pt[pr1 / BT];            // round k0 + 64
                pt21 = L->pt2[pr1 / BT];
                rec_at(k0 + 128, pr2, Sn, S2n);   // round k0 + 128
                const uint32_t k = (uint32_t)(k0 + l);
                const uint32_t pp = (uint32_t)wave_shr1_i((int)p, (int)prevp);
                const double Gp = wave_shr1_d(G, Gprev), G2p = wave_shr1_d(G2, G2prev);
                if (!SEG || rank + k != skip_rank) store_event_fast(eo, rank + k, pp, p, G - Gp, G2 - G2p, overflow);
                prevp = (uint32_t)wave_ror1_i((int)p);
                Gprev = wave_ror1_d(G);
                G2prev = wave_ror1_d(G2);
                p = tbm + pr1;
                G = pt1 + S1;
                G2 = pt21 + S21;
                pr1 = pr2; S1 = Sn; S21 = S2n;
            }
            // what is left (fewer than 64 records) is what the last round left behind
            if (partial) {
                if (mleft > 0) {
                    const uint32_t k = (uint32_t)(nfull + l);
                    const uint32_t pp = (uint32_t)wave_shr1_i((int)p, (int)prevp);
                    const double Gp = wave_shr1_d(G, Gprev), G2p = wave_shr1_d(G2, G2prev);
                    if (l < mleft && (!SEG || rank + k != skip_rank))
                        store_event_fast(eo, rank + k, pp, p, G - Gp, G2 - G2p, overflow);
                    prevp = (uint32_t)__builtin_amdgcn_readlane((int)p, mleft - 1);
                    Gprev = readlane_d(G, mleft - 1);
                    G2prev = readlane_d(G2, mleft - 1);
                }
                rank += (uint32_t)tot;
                m = 0;
            } else {
                if (l < mleft) {
                    BuildRec left;
                    left.S = G - tileS;
                    left.S2 = G2 - tileS2;
                    L->rec[l] = left;
                    L->p[l] = (uint16_t)(p - (uint32_t)tb);
                }
                rank += (uint32_t)nfull;
                m = mleft;
            }
            Gprev = Gprev - tileS;
            G2prev = G2prev - tileS2;
            __syncthreads();
            continue;
        }
        for (int k0 = 0; k0 < tot; k0 += 64) {
            pt1 = L->pt[pr1 / BT];            // round k0 + 64
            pt21 = L->pt2[pr1 / BT];
            rec_at(k0 + 128, pr2, Sn, S2n);   // round k0 + 128
            const int k = k0 + l;
            const bool act = k < tot;
            const uint32_t p = (uint32_t)tb + pr0;
            const double G = pt0 + S0;
            const double G2 = pt20 + S20;
            const uint32_t pp = (uint32_t)wave_shr1_i((int)p, (int)prevp);
            const double Gp = wave_shr1_d(G, Gprev), G2p = wave_shr1_d(G2, G2prev);
            if (act && (!SEG || rank + (uint32_t)k != skip_rank))
                store_event_fast(eo, rank + (uint32_t)k, pp, p, G - Gp, G2 - G2p, overflow);
            const int last = (tot - k0) < 64 ? (tot - k0 - 1) : 63;  // wave-uniform
            prevp = (uint32_t)__builtin_amdgcn_readlane((int)p, last);
            Gprev = readlane_d(G, last);
            G2prev = readlane_d(G2, last);
            pr0 = pr1; S0 = S1; S20 = S21; pt0 = pt1; pt20 = pt21;
            pr1 = pr2; S1 = Sn; S21 = S2n;
        }
        rank += (uint32_t)tot;
        // rebase the carry to the next tile's start
        Gprev = Gprev - tileS;
        G2prev = G2prev - tileS2;
        __syncthreads();
    }
    // exactness guard (see the file header): reads that fail it are redone by k_event_fallback
    float mn, mx;
    bool known = true;
    if constexpr (std::is_same<T, int16_t>::value) {
        int rmn = rmin2.x < rmin2.y ? rmin2.x : rmin2.y, rmxv = rmax2.x > rmax2.y ? rmax2.x : rmax2.y;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const int o1 = __shfl_xor(rmn, d, 64), o2 = __shfl_xor(rmxv, d, 64);
            rmn = o1 < rmn ? o1 : rmn;
            rmxv = o2 > rmxv ? o2 : rmxv;
        }
        if constexpr (SEG) { mnb = (uint32_t)rmn; mxb = (uint32_t)rmxv; }
        else known = raw_extremes_to_pa(rmn, rmxv, rc.sc, mn, mx);
    } else {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t o1 = (uint32_t)__shfl_xor((int)mnb, d, 64), o2 = (uint32_t)__shfl_xor((int)mxb, d, 64);
            mnb = o1 < mnb ? o1 : mnb;
            mxb = o2 > mxb ? o2 : mxb;
        }
        mn = (mnb == 0xffffffffu) ? FLT_MAX : __uint_as_float(mnb + 1u);
        mx = __uint_as_float(mxb);
        known = mxb < 0x7f800000u;
    }
    if constexpr (SEG) {
        // the read's last segment closes the read's last event; the verdict on the read is chain_segment's
        if (l == 0 && seg_b == n) store_event_fast(eo, rank, prevp, (uint32_t)n, 0.0 - Gprev, 0.0 - G2prev, overflow);
        const bool ovf = __any(overflow);
        if (l == 0) {
            st->ext_lo = mnb;
            st->ext_hi = mxb;
            st->bflags = (dense ? 1u : 0u) | (ovf ? 2u : 0u);
        }
        return;
    }
    const bool flagged = dense || !known || !guard_ok(mn, mx, n) || declined;
    if (l == 0) {
        a.flags[r] = flagged ? 1 : 0;
        if (flagged) {
            const uint32_t k = atomicAdd(&a.hdr->n_flagged, 1u);
            a.flag_list[k] = r;
        } else {
            store_event_fast(eo, rank, prevp, (uint32_t)n, 0.0 - Gprev, 0.0 - G2prev, overflow);
            a.n_events[r] = rank + 1;
            atomicAdd(&a.hdr->n_events_total, (unsigned long long)(rank + 1));
        }
    }
    if (!flagged && __any(overflow) && l == 0) atomicAdd(&a.hdr->n_overflow, 1u);
}

// Detector and builder of one read in one wave, back to back: the builder's phases
// that wait on memory (sample tiles, event stores) run under other waves' detector arithmetic instead of in a
// kernel of their own.  The bitmap goes through memory (L2) between the two phases of the same wave.
union EventLds {
    LzLds lz;
    BuildLds b;
    BuildLdsCarry bc;
};
template <bool CARRY>
__device__ __forceinline__ BuildLdsT<CARRY ? 128 : 64> *build_lds(EventLds *L) {
    if constexpr (CARRY) return &L->bc;
    else return &L->b;
}

}  // namespace sgk
