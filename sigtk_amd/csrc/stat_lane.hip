// stat_lane.hip -- the lane-per-read kernels (round 1): one read per lane, serial float chains, the 64 reads of a
// wave streamed through the LDS row stager (row_stream.h).  The independent second implementation the tests compare the
// wave-per-read kernels against, bit for bit: it must not include seqsum.h or stat_wave.h.  The map of the stat units and
// the reference semantics are in stat_device.h.
#include "row_stream.h"
#include "stat_device.h"

namespace sgk {

__device__ inline int wave_max_i(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// Lane-per-row sequential sweep: calls f(j, raw) for j = 0..len-1 in order.  All lanes of the wave
// must call it (cooperative tile loads); lanes with len == 0 just help loading.  Tile t+1 is in
// flight while tile t is consumed out of registers.
template <int K, typename F>
__device__ __forceinline__ void sweep_tile_elems(const uint32_t (&w)[32], int64_t j0, int64_t len, F &f) {
    if constexpr (K < TILE) {
        const int64_t j = j0 + K;
        if (j >= 0 && j < len) f(j, RowPrefetch::sample<K>(w));
        sweep_tile_elems<K + 1>(w, j0, len, f);
    }
}
template <int K, typename F>
__device__ __forceinline__ void sweep_tile_full(const uint32_t (&w)[32], int j0, F &f) {
    if constexpr (K < TILE) {
        f((int64_t)(j0 + K), RowPrefetch::sample<K>(w));
        sweep_tile_full<K + 1>(w, j0, f);
    }
}
template <typename F>
__device__ inline void sweep_rows(RowPrefetch &rs, int skip, int64_t len, F f) {
    const int maxq = wave_max_i((int)(len > 0 ? skip + len : 0));
    const int ntiles = (maxq + TILE - 1) / TILE;
    if (ntiles == 0) return;
    rs.issue(0);
    rs.commit(0);
    for (int t = 0; t < ntiles; ++t) {
        if (t + 1 < ntiles) rs.issue(t + 1);
        uint32_t w[32];
        rs.row(w);
        const int64_t j0 = (int64_t)t * TILE - skip;
        // common case: the whole tile lies inside the row of every lane that still has samples (lanes whose row
        // has ended, or has not begun, sit the tile out) -> no per-sample predicates
        const bool inside = j0 >= 0 && j0 + TILE <= len, outside = j0 + TILE <= 0 || j0 >= len;
        if (__all(inside || outside)) {
            if (inside) sweep_tile_full<0>(w, (int)j0, f);
        } else if (!outside) sweep_tile_elems<0>(w, j0, len, f);
        if (t + 1 < ntiles) rs.commit(t + 1);
    }
}

// Same contract as sweep_rows, but the tile is consumed in rolled parts of P samples (P/2 registers, a P-step
// unrolled body): for callbacks with a lot of code or state (the jnn automaton) this keeps the kernel small and
// out of scratch.
template <int K, int P, typename F>
__device__ __forceinline__ void sweep_part_elems(const uint32_t (&w)[P / 2], int64_t j0, int64_t len, F &f) {
    if constexpr (K < P) {
        const int64_t j = j0 + K;
        if (j >= 0 && j < len) f(j, RowPrefetch::sample_part<K>(w));
        sweep_part_elems<K + 1, P>(w, j0, len, f);
    }
}
template <int K, int P, typename F>
__device__ __forceinline__ void sweep_part_full(const uint32_t (&w)[P / 2], int j0, F &f) {
    if constexpr (K < P) {
        f((int64_t)(j0 + K), RowPrefetch::sample_part<K>(w));
        sweep_part_full<K + 1, P>(w, j0, f);
    }
}
template <int P, typename F>
__device__ inline void sweep_rows_parts(RowPrefetch &rs, int skip, int64_t len, F f) {
    const int maxq = wave_max_i((int)(len > 0 ? skip + len : 0));
    const int ntiles = (maxq + TILE - 1) / TILE;
    if (ntiles == 0) return;
    rs.issue(0);
    rs.commit(0);
    for (int t = 0; t < ntiles; ++t) {
        if (t + 1 < ntiles) rs.issue(t + 1);
#pragma unroll 1
        for (int h = 0; h < TILE / P; ++h) {
            uint32_t w[P / 2];
            rs.row_part<P>(h, w);
            const int64_t j0 = (int64_t)t * TILE + h * P - skip;
            const bool inside = j0 >= 0 && j0 + P <= len, outside = j0 + P <= 0 || j0 >= len;
            if (__all(inside || outside)) {  // see sweep_rows
                if (inside) sweep_part_full<0, P>(w, (int)j0, f);
            } else if (!outside) sweep_part_elems<0, P>(w, j0, len, f);
        }
        if (t + 1 < ntiles) rs.commit(t + 1);
    }
}

__device__ inline RowPrefetch make_stream(char *lds, const sgk_batch_t &b, int64_t start, bool wanted, int &skip) {
    RowPrefetch rs;
    const int64_t rb = start & ~(int64_t)7;
    skip = (int)(start - rb);
    rs.init(lds, b.samples, (int64_t)b.n_samples, rb, __ballot(wanted));
    return rs;
}

// ---------------------------------------------------------------- moments (src/stat.h:17-54)
// HIST (stat without the pA output): the deviation pass also counts, per lane, the samples in a window of MH_BINS raw
// values around the read's mean (a column of LDS words per lane: no other lane touches it) and those below it, and the
// read's median (rank n/2 and, for a negative unit, n-1-n/2: src/stat.h:56-73) is read off that: the third pass over
// the samples (k_median) is only needed for reads whose median lies outside the window (flagged for k_median; the sp1
// fixture's reads have their median -10 .. +21 raw values from their mean, 13 at the 99th percentile: a few per cent of
// real reads, whose k_median workgroups cost in proportion).  The lane kernels are bound by HBM and close to bound by
// instruction issue: 125 000 x 100 000 samples 13.0 (k_moments 9.0 + k_median 4.0) -> 10.0 ms with 32 bins (10.8 with a
// branch around the counting instead of the extra row); 64 bins
// (16 KB of LDS per wave) lose the occupancy the kernel streams with (16.5 ms), 64 16-bit counters packed two to a word
// cost more instructions than they save (12.6 ms).
constexpr int MH_BINS = 32;
constexpr int MOM_WAVES = 1;  // waves per SIMD the register allocation aims at (3: 168 registers + 42 spilled, 13.0 against 10.1 ms)
template <int MODE, bool HIST = false>
__global__ __launch_bounds__(64, MOM_WAVES) void k_moments(StatArgs a) {
    __shared__ __attribute__((aligned(16))) char lds[RowPrefetch::LDS_BYTES];
    __shared__ uint32_t mh[HIST ? (MH_BINS + 1) * 64 : 1];  // (+ a row nobody reads: samples outside the window)
    const int lane = lane_id();
    const uint32_t r = blockIdx.x * 64 + lane;
    const bool valid = r < a.b.n_reads;
    Region g = {0, 0};
    Scale sc = {0.0f, 1.0f};
    if (valid) {
        g = get_region(MODE, a.b, a.prefix, r);
        sc = make_scale(a.b.digitisation[r], a.b.offset[r], a.b.range[r]);
    }
    int skip;
    RowPrefetch rs = make_stream(lds, a.b, g.start, valid && g.len > 0, skip);
    const float nf = (float)(int)g.len;
    float sraw = 0.0f, spa = 0.0f;
    sweep_rows(rs, skip, g.len, [&](int64_t, int16_t v) {
        sraw = sraw + (float)v;
        spa = spa + to_pa(v, sc);
    });
    const float mraw = sraw / nf, mpa = spa / nf;
    float qraw = 0.0f, qpa = 0.0f;
    int lo = 0;
    uint32_t below = 0u;
    if (HIST) {
        const int c = (mraw == mraw) ? (int)fminf(fmaxf(mraw, -32768.0f), 32767.0f) : 0;
        lo = c - MH_BINS / 2;
#pragma unroll
        for (int b = 0; b < MH_BINS; ++b) mh[b * 64 + lane] = 0u;
    }
    sweep_rows(rs, skip, g.len, [&](int64_t, int16_t v) {
        const float d = (float)v - mraw;
        qraw = qraw + d * d;
        const float e = to_pa(v, sc) - mpa;
        qpa = qpa + e * e;
        if (HIST) {
            // (no branch: a sample outside the window goes to the extra row; this lane's column)
            const uint32_t b = (uint32_t)((int)v - lo);
            atomicAdd(&mh[(b < (uint32_t)MH_BINS ? b : (uint32_t)MH_BINS) * 64u + (uint32_t)lane], 1u);
            below += b >> 31;
        }
    });
    if (!valid) return;
    const float sdraw = sqrtf(qraw / nf), sdpa = sqrtf(qpa / nf);
    // HIST: the order statistics of ranks n/2 and (negative unit) n-1-n/2 from the window's counts
    int b1 = -1, b2 = -1;
    if (HIST && g.len > 0) {
        const uint32_t k = (uint32_t)(g.len / 2);
        const bool mirrored = sc.unit < 0.0f && g.len - 1 - (int64_t)k != (int64_t)k;  // pA order is the reverse of the raw order
        const uint32_t k2 = mirrored ? (uint32_t)(g.len - 1 - (int64_t)k) : k;
        uint32_t acc = below;
        for (int b = 0; b < MH_BINS; ++b) {
            const uint32_t h = mh[b * 64 + lane];
            if (b1 < 0 && k >= acc && k < acc + h) b1 = b;
            if (b2 < 0 && k2 >= acc && k2 < acc + h) b2 = b;
            acc += h;
        }
    }
    const bool have_median = b1 >= 0 && b2 >= 0;
    if (MODE == REG_WHOLE) {
        sgk_stat_rec_t *o = a.stat + r;
        o->raw_mean = mraw; o->pa_mean = mpa; o->raw_std = sdraw; o->pa_std = sdpa;
        o->n = (uint32_t)g.len;
        o->reserved = 0;
        if (HIST) {
            if (g.len <= 0) { o->raw_median = 0; o->pa_median = 0.0f; }
            else if (have_median) {
                o->raw_median = lo + b1;
                o->pa_median = to_pa((int16_t)(lo + b2), sc);
            } else o->reserved = FLAG_MEDIAN_WHOLE;  // outside the window: k_median (FLAGGED) takes the read
        }
    } else if (MODE == REG_ADAPT) {
        a.prefix[r].adapt_mean = mpa;
        a.prefix[r].adapt_std = sdpa;
        if (HIST && g.len > 0) {
            if (have_median) a.prefix[r].adapt_median = to_pa((int16_t)(lo + b2), sc);
            else a.prefix[r].reserved |= FLAG_MEDIAN_ADAPT;
        }
    } else {
        a.prefix[r].polya_mean = mpa;
        a.prefix[r].polya_std = sdpa;
        if (HIST && g.len > 0) {
            if (have_median) a.prefix[r].polya_median = to_pa((int16_t)(lo + b2), sc);
            else a.prefix[r].reserved |= FLAG_MEDIAN_POLYA;
        }
    }
}

// ---------------------------------------------------------------- median (src/stat.h:56-73)
// Visit every key of x[0..n) with a 256-thread workgroup: 16-byte vector loads over the aligned
// middle (four in flight per thread), scalar loads for the unaligned head and tail.  With PA, pa[i] =
// signal_in_picoamps(x[i]) is written on the way (two 16-byte stores per vector): the fused stat + pa of
// BASELINE config 4 costs no extra pass over the samples.
template <bool PA, typename F>
__device__ __forceinline__ void visit_keys(const int16_t *x, int64_t n, F f, float *pa = nullptr,
                                           Scale sc = Scale{0.0f, 1.0f}) {
    const int t = threadIdx.x;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(x);
    int64_t head = (int64_t)(((16 - (addr & 15)) & 15) / 2);
    if (head > n) head = n;
    const int64_t nvec = (n - head) / 8;
    const int64_t tail0 = head + nvec * 8;
    if (t < head) {
        f((uint32_t)((int)x[t] + 32768));
        if (PA) pa[t] = to_pa(x[t], sc);
    }
    if (tail0 + t < n && t < 8) {
        f((uint32_t)((int)x[tail0 + t] + 32768));
        if (PA) pa[tail0 + t] = to_pa(x[tail0 + t], sc);
    }
    const uint4 *v = reinterpret_cast<const uint4 *>(x + head);
    for (int64_t i = t; i < nvec; i += 256 * 4) {
        uint4 q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t k = i + (int64_t)u * 256;
            q[u] = (k < nvec) ? v[k] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t k = i + (int64_t)u * 256;
            if (k < nvec) {
                const uint32_t w[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
                float o[8];
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const int16_t s0 = (int16_t)(w[d] & 0xffffu), s1 = (int16_t)(w[d] >> 16);
                    f((uint32_t)((int)s0 + 32768));
                    f((uint32_t)((int)s1 + 32768));
                    if (PA) { o[2 * d] = to_pa(s0, sc); o[2 * d + 1] = to_pa(s1, sc); }
                }
                if (PA) {
                    float4 *dst = reinterpret_cast<float4 *>(pa + head + k * 8);  // x + head is 16-byte aligned
                    dst[0] = make_float4(o[0], o[1], o[2], o[3]);
                    dst[1] = make_float4(o[4], o[5], o[6], o[7]);
                }
            }
        }
    }
}

// exclusive prefix of one count per thread over a 256-thread workgroup (a DPP scan per wave + the four wave totals
// through part[260 .. 263]; a serial pass of one thread over 256 LDS words cost a short read more than counting its
// samples did)
__device__ __forceinline__ uint32_t block_excl_scan_256(uint32_t s, uint32_t *part /*264*/) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint32_t incl = (uint32_t)wave_incl_scan_i((int)s);
    if (lane == 63) part[260 + wv] = incl;
    __syncthreads();
    uint32_t before = incl - s;
#pragma unroll
    for (int w = 0; w < 3; ++w) before += w < wv ? part[260 + w] : 0u;
    __syncthreads();
    return before;
}

// rank-k order statistic of the int16 keys of a region, by a 256-thread workgroup
template <bool PA = false>
__device__ int block_select(const int16_t *x, int64_t n, int64_t rank, uint32_t *hist /*4096*/, uint32_t *part /*264*/,
                            float *pa = nullptr, Scale sc = Scale{0.0f, 1.0f}) {
    const int t = threadIdx.x;
    for (int i = t; i < 4096; i += 256) hist[i] = 0;
    __syncthreads();
    visit_keys<PA>(x, n, [&](uint32_t key) { atomicAdd(&hist[key >> 4], 1u); }, pa, sc);
    __syncthreads();
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += hist[t * 16 + k];
    const uint32_t before = block_excl_scan_256(s, part);
    if ((uint64_t)rank >= before && (uint64_t)rank < (uint64_t)before + s) {
        uint32_t acc = before;
        for (int k = 0; k < 16; ++k) {
            const uint32_t h = hist[t * 16 + k];
            if ((uint64_t)rank < (uint64_t)acc + h) { part[256] = (uint32_t)(t * 16 + k); part[257] = (uint32_t)(rank - acc); break; }
            acc += h;
        }
    }
    __syncthreads();
    const uint32_t bin = part[256], rank2 = part[257];
    __syncthreads();
    if (t < 16) hist[t] = 0;
    __syncthreads();
    visit_keys<false>(x, n, [&](uint32_t key) {
        if ((key >> 4) == bin) atomicAdd(&hist[key & 15u], 1u);
    });
    __syncthreads();
    if (t == 0) {
        uint32_t acc = 0, val = 0;
        for (int k = 0; k < 16; ++k) {
            if (rank2 < acc + hist[k]) { val = (uint32_t)k; break; }
            acc += hist[k];
        }
        part[256] = val;
    }
    __syncthreads();
    const int res = (int)((bin << 4) | part[256]) - 32768;
    __syncthreads();
    return res;
}

// Order statistics of ranks k1 and k2 from ONE pass: an LDS histogram with one bin per raw value over the window
// [lo, lo + RANGE_BINS) (centred on the read's mean, which k_moments has already written); values outside are
// clipped into the two edge bins.  A rank that lands in an edge bin is not trusted (ok = false -> the caller
// falls back to the two-level select).  Nanopore raw signals span a few hundred ADC codes, so this is the path taken.
constexpr int RANGE_BINS = 8192;
template <bool PA, int nb /* bins: RANGE_BINS or a narrower window */>
__device__ bool block_select_range(const int16_t *x, int64_t n, int64_t k1, int64_t k2, int lo,
                                   uint32_t *hist /*RANGE_BINS*/, uint32_t *part /*264*/, int &r1, int &r2,
                                   float *pa, Scale sc) {
    const int t = threadIdx.x;
    constexpr int per = nb / 256;
    for (int i = t; i < nb; i += 256) hist[i] = 0;
    __syncthreads();
    const int base = lo + 32768;
    visit_keys<PA>(x, n, [&](uint32_t key) {
        int b = (int)key - base;
        b = b < 0 ? 0 : (b > nb - 1 ? nb - 1 : b);
        atomicAdd(&hist[b], 1u);
    }, pa, sc);
    __syncthreads();
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < per; ++k) s += hist[t * per + k];
    const uint32_t before = block_excl_scan_256(s, part);
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        const int64_t rank = w ? k2 : k1;
        if ((uint64_t)rank >= before && (uint64_t)rank < (uint64_t)before + s) {
            uint32_t acc = before;
            for (int k = 0; k < per; ++k) {
                const uint32_t h = hist[t * per + k];
                if ((uint64_t)rank < (uint64_t)acc + h) { part[256 + w] = (uint32_t)(t * per + k); break; }
                acc += h;
            }
        }
    }
    __syncthreads();
    const int b1 = (int)part[256], b2 = (int)part[257];
    __syncthreads();
    r1 = lo + b1;
    r2 = lo + b2;
    return b1 > 0 && b1 < nb - 1 && b2 > 0 && b2 < nb - 1;
}

// FLAGGED: only the reads k_stat_wave could not settle (order statistic outside its window)
template <int MODE, bool PA = false, bool FLAGGED = false>
__global__ __launch_bounds__(256) void k_median(StatArgs a) {
    __shared__ uint32_t hist[MODE == REG_WHOLE ? RANGE_BINS : 4096];
    __shared__ uint32_t part[264];
    const uint32_t r = blockIdx.x;
    if (FLAGGED) {
        const uint32_t fl = MODE == REG_WHOLE ? a.stat[r].reserved : a.prefix[r].reserved;
        if (!(fl & (MODE == REG_POLYA ? 2u : 1u))) return;
    }
    const Region g = get_region(MODE, a.b, a.prefix, r);
    if (g.len <= 0) {
        if (threadIdx.x == 0 && MODE == REG_WHOLE) { a.stat[r].raw_median = 0; a.stat[r].pa_median = 0.0f; a.stat[r].reserved = 0; }
        return;
    }
    const Scale sc = make_scale(a.b.digitisation[r], a.b.offset[r], a.b.range[r]);
    const int16_t *x = a.b.samples + g.start;
    float *pa = PA ? a.pa_out + g.start : nullptr;
    const int64_t k = g.len / 2;
    const bool mirrored = sc.unit < 0.0f && g.len - 1 - k != k;  // pA order is the reverse of the raw order
    int med, med_for_pa;
    bool done = false;
    if (MODE == REG_WHOLE) {
        // window centred on the read's raw mean (written by k_moments, which runs before this kernel)
        // (a short read gets a narrower window: clearing and scanning 8192 bins costs a 5 000-sample read more than
        // counting its samples; +-1024 raw values around the mean still hold any nanopore read's median)
        const float m = a.stat[r].raw_mean;
        const int nb = g.len <= 65536 ? 2048 : RANGE_BINS;
        int c = (m == m) ? (int)fminf(fmaxf(m, -32768.0f), 32767.0f) : 0;
        int lo = c - nb / 2;
        lo = lo < -32768 ? -32768 : (lo > 32768 - nb ? 32768 - nb : lo);
        const int64_t k2 = mirrored ? g.len - 1 - k : k;
        done = nb == 2048 ? block_select_range<PA, 2048>(x, g.len, k, k2, lo, hist, part, med, med_for_pa, pa, sc)
                          : block_select_range<PA, RANGE_BINS>(x, g.len, k, k2, lo, hist, part, med, med_for_pa, pa, sc);
        pa = nullptr;  // already written
    }
    if (!done) {
        if (PA && pa) med = block_select<true>(x, g.len, k, hist, part, pa, sc);
        else med = block_select<false>(x, g.len, k, hist, part);
        med_for_pa = mirrored ? block_select<false>(x, g.len, g.len - 1 - k, hist, part) : med;
    }
    if (threadIdx.x == 0) {
        const float pm = to_pa((int16_t)med_for_pa, sc);
        if (MODE == REG_WHOLE) { a.stat[r].raw_median = med; a.stat[r].pa_median = pm; a.stat[r].reserved = 0; }
        else if (MODE == REG_ADAPT) a.prefix[r].adapt_median = pm;
        else a.prefix[r].polya_median = pm;
        if (FLAGGED && MODE != REG_WHOLE) a.prefix[r].reserved &= ~(MODE == REG_POLYA ? 2u : 1u);
    }
}

// jnn_raw (src/jnn.c:282-293): jnn_core over rm_outlier(raw) with any jnn_param_t
__global__ __launch_bounds__(64) void k_jnn(StatArgs a, JnnP p) {
    __shared__ __attribute__((aligned(16))) char lds[RowPrefetch::LDS_BYTES];
    const uint32_t r = blockIdx.x * 64 + lane_id();
    const bool valid = r < a.b.n_reads && (!a.jnn_redo || a.n_segs[r] == JNN_REDO_MARK);
    if (a.jnn_redo && !__any(valid)) return;
    Region g = {0, 0};
    if (valid) g = get_region(REG_WHOLE, a.b, nullptr, r);
    int skip;
    RowPrefetch rs = make_stream(lds, a.b, g.start, valid && g.len > 0, skip);
    float top = p.top, bot = p.bot;
    if (p.std_scale > 0.0f) {  // src/jnn.c:195-199
        const float nf = (float)(int)g.len;
        float s = 0.0f;
        sweep_rows(rs, skip, g.len, [&](int64_t, int16_t v) { s = s + clampf_raw(v); });
        const float mn = s / nf;
        float q = 0.0f;
        sweep_rows(rs, skip, g.len, [&](int64_t, int16_t v) {
            const float d = clampf_raw(v) - mn;
            q = q + d * d;
        });
        const float sd = sqrtf(q / nf);
        const float band = sd * p.std_scale;
        top = mn + band;
        bot = mn - band;
    }
    JnnAuto A;
    A.init(top, bot, p.corrector, p.seg_dist, p.window, p.stall_len, p.error);
    const uint64_t slot0 = valid ? a.seg_slots[r] : 0, cap = valid ? a.seg_slots[r + 1] - slot0 : 0;
    bool overflow = false;
    auto emit = [&](int k, int x, int y) {
        if ((uint64_t)k < cap) { a.seg_x[slot0 + k] = x; a.seg_y[slot0 + k] = y; }
        else overflow = true;
    };
    sweep_rows_parts<16>(rs, skip, g.len, [&](int64_t j, int16_t v) { A.step((int)j, A.in_mask_raw(clampi_raw(v)), emit); });
    A.finish(emit);
    if (valid) a.n_segs[r] = (uint32_t)A.nseg;
    if (overflow) atomicAdd(a.err_count, 1u);
}

// find_polya (src/jnn.c:352-374): first segment of jnn_pa on pA[adapt_y..n) with fixed thresholds
// top = (m_a+30)+20, bot = (m_a+30)-20 (src/cfunc.c:191); polyA preset src/jnn.h:52-72.
// PARAM: the caller's set `q` (any of the domain: JnnAuto is the whole automaton) in place of the preset and of 30 / 20
template <bool PARAM>
__device__ __forceinline__ void polya_lane(const StatArgs &a, const PolyP &q, char *lds) {
    const uint32_t r = blockIdx.x * 64 + lane_id();
    const bool valid = r < a.b.n_reads;
    Region g = {0, 0};
    Scale sc = {0.0f, 1.0f};
    float m_a = 0.0f;
    if (valid) {
        g = get_region(REG_TAIL, a.b, a.prefix, r);
        sc = make_scale(a.b.digitisation[r], a.b.offset[r], a.b.range[r]);
        m_a = a.prefix[r].adapt_mean;
    }
    int skip;
    RowPrefetch rs = make_stream(lds, a.b, g.start, valid && g.len > 0, skip);
    const float mid = m_a + (PARAM ? q.shift : 30.0f);
    JnnAuto A;
    const JnnP pp = PARAM ? q.p : JnnP{-1.0f, 50, 200, 250, 1.0f, 30, 0.0f, 0.0f};  // JNNV1_R9_POLYA, src/jnn.h:52-61
    A.init(mid + (PARAM ? q.band : 20.0f), mid - (PARAM ? q.band : 20.0f), pp.corrector, pp.seg_dist, pp.window, pp.stall_len, pp.error);
    int px = -1, py = -1;
    auto emit = [&](int k, int x, int y) {
        if (k == 0) { px = x; py = y; }
    };
    // (a lane whose first segment is final could stop; the sweep is wave-cooperative, so it just idles)
    sweep_rows_parts<16>(rs, skip, g.len, [&](int64_t j, int16_t v) {
        if (py < 0 || A.nseg < 2) A.step((int)j, A.in_mask_f(clampf_pa(to_pa(v, sc))), emit);
    });
    if (A.nseg == 1 || (A.nseg >= 2 && py < 0)) A.finish(emit);
    if (valid) {
        a.prefix[r].polya_x = px;
        a.prefix[r].polya_y = py;
    }
}
__global__ __launch_bounds__(64) void k_polya(StatArgs a) {
    __shared__ __attribute__((aligned(16))) char lds[RowPrefetch::LDS_BYTES];
    polya_lane<false>(a, PolyP{}, lds);
}
__global__ __launch_bounds__(64) void k_polya_param(StatArgs a, PolyP q) {
    __shared__ __attribute__((aligned(16))) char lds[RowPrefetch::LDS_BYTES];
    polya_lane<true>(a, q, lds);
}

// ---------------------------------------------------------------- find_adaptor / jnnv2 (src/jnn.c:99-188)
// rolling window mean (jnn.c:20-56) of the clamped raw signal, its sequential float mean/std,
// then the below-threshold run finder with merging; first run with lo <= length <= hi.
struct RunFinder {
    int t_lt, t_gt;  // tot < t_lt  <=>  t < bot;   tot >= t_gt  <=>  t > bot   (see roll_threshold)
    int seg_dist, lo, hi;
    int in_run, start, end, nseg, last_x, last_y, ans_x, ans_y, found;
    __device__ void init(int t_lt_, int t_gt_, int seg_dist_, int lo_, int hi_) {
        t_lt = t_lt_; t_gt = t_gt_; seg_dist = seg_dist_; lo = lo_; hi = hi_;
        in_run = 0; start = 0; end = 0; nseg = 0; last_x = 0; last_y = 0; ans_x = 0; ans_y = 0; found = 0;
    }
    __device__ void settle() {  // the last segment can no longer change
        const int len = last_y - last_x;
        if (!found && !(len > hi) && !(len < lo)) { found = 1; ans_x = last_x; ans_y = last_y; }
    }
    __device__ __forceinline__ void step(int j, int tot) {
        const bool below = tot < t_lt, above = tot >= t_gt;
        // selects for the per-sample updates; only the (rare) end of a run branches
        start = (below & !in_run) ? j : start;
        end = (below & (in_run != 0)) ? j : end;
        if (above & (in_run != 0)) {
            if (nseg > 0 && start - last_y < seg_dist) last_y = end;
            else {
                if (nseg > 0) settle();
                last_x = start; last_y = end; ++nseg;
            }
            start = 0; end = 0; in_run = 0;
        } else {
            in_run = below ? 1 : in_run;
        }
    }
    __device__ void finish() { if (nseg > 0) settle(); }
};

// One rolling-window sweep: calls f(i, tot_i) for i = 0..m-1 (m = n - ADW) in order, tot_i = sum of the clamped
// samples x[i .. i+ADW).  The trailing edge is a second row stream whose base is shifted by 16 samples, so that
// its tiles line up with the leading stream's: trail tile = lead tile - 31 (ADW = 2000 = 31*64 + 16).
constexpr int PART = 16;  // samples handled per (rolled) inner iteration: keeps the unrolled bodies and the
                          // register footprint small (two streams, three sweeps, each in a full and an edge form)
// f(i, tot_i) is called for the window indices i = 0..m-1 only (m = n - ADW, as rolling_window's output length,
// src/jnn.c:20-56); indices are 32-bit (reads are < 2^31 samples, misc.c:20).
template <int K, typename F>
__device__ __forceinline__ void rolling_elems(const uint32_t (&wl)[PART / 2], const uint32_t (&wt)[PART / 2],
                                              int64_t il0, int64_t n, int &tot, F &f) {
    if constexpr (K < PART) {
        const int64_t il = il0 + K;  // lead index
        if (il >= 0 && il < n) {
            const int cl = clampi_raw(RowPrefetch::sample_part<K>(wl));
            if (il < ADW) {
                tot = tot + cl;
                if (il == ADW - 1) f(0, tot);
            } else {
                const int ct = clampi_raw(RowPrefetch::sample_part<K>(wt));
                tot = tot - ct;
                tot = tot + cl;
                if (il < n - 1) f((int)(il - ADW + 1), tot);  // the total after the last sample has no window
            }
        }
        rolling_elems<K + 1>(wl, wt, il0, n, tot, f);
    }
}
// all PART lead indices are in [ADW, n-1): no predicates.  Two samples per packed 16-bit instruction for the outlier
// clamp and the lead - trail difference (|difference| <= 1200 fits int16).
template <int K, typename F>
__device__ __forceinline__ void rolling_full(const uint32_t (&wl)[PART / 2], const uint32_t (&wt)[PART / 2], int i0,
                                             int &tot, F &f) {
    if constexpr (K < PART) {
        static_assert(K % 2 == 0, "pairs");
        const s16x2 d = clamp_raw2(wl[K / 2]) - clamp_raw2(wt[K / 2]);
        tot += (int)d.x;
        f(i0 + K, tot);
        tot += (int)d.y;
        f(i0 + K + 1, tot);
        rolling_full<K + 2>(wl, wt, i0, tot, f);
    }
}
struct NeverStop {
    __device__ bool operator()() const { return false; }
};
// `stop` is asked once per tile (this lane has nothing more to learn); the sweep ends early when every lane says so
template <typename F, typename S = NeverStop>
__device__ inline void sweep_rolling(RowPrefetch &lead, RowPrefetch &trail, int skip, int64_t n, F f, S stop = S()) {
    const int maxq = wave_max_i((int)(n > ADW ? skip + n : 0));
    const int ntiles = (maxq + TILE - 1) / TILE;
    if (ntiles == 0) return;
    constexpr int LAG = 31;  // tiles between the two streams
    int tot = 0;
    const int n32 = (int)n;
    lead.issue(0);
    lead.commit(0);
    for (int t = 0; t < ntiles; ++t) {
        if (t + 1 < ntiles) lead.issue(t + 1);
        if (t + 1 >= LAG && t + 1 < ntiles) trail.issue(t + 1 - LAG);
#pragma unroll 1
        for (int h = 0; h < TILE / PART; ++h) {
            uint32_t wl[PART / 2], wt[PART / 2];
            lead.row_part<PART>(h, wl);
            if (t >= LAG) trail.row_part<PART>(h, wt);
            else {
#pragma unroll
                for (int k = 0; k < PART / 2; ++k) wt[k] = 0u;
            }
            const int il0 = t * TILE + h * PART - skip;
            // lanes whose read has ended (or is too short, or has not begun) sit the part out; the predicated form
            // is only needed while some lane crosses the start, the first full window or the end of its read
            const bool inside = il0 >= ADW && il0 + PART < n32;
            const bool outside = n32 <= ADW || il0 >= n32 || il0 + PART <= 0;
            if (__all(inside || outside)) {
                if (inside) rolling_full<0>(wl, wt, il0 - ADW + 1, tot, f);
            } else if (!outside) rolling_elems<0>(wl, wt, (int64_t)il0, n, tot, f);
        }
        if (__all(stop())) break;
        if (t + 1 < ntiles) lead.commit(t + 1);
        if (t + 1 >= LAG && t + 1 < ntiles) trail.commit(t + 1 - LAG);
    }
}

__global__ __launch_bounds__(64, 2) void k_adaptor(StatArgs a, AdaptP ap) {
    __shared__ __attribute__((aligned(16))) char lds[2 * RowPrefetch::LDS_BYTES];
    const uint32_t r = blockIdx.x * 64 + lane_id();
    const bool valid = r < a.b.n_reads;
    Region g = {0, 0};
    if (valid) g = get_region(REG_WHOLE, a.b, nullptr, r);
    const int64_t n = g.len;
    const bool run = valid && n > ADW;
    int skip;
    RowPrefetch lead = make_stream(lds, a.b, g.start, run, skip);
    RowPrefetch trail;
    // trail position = lead position - 2000 = (row base - 16) + (q - 31*64): the same rows, shifted
    trail = lead;
    trail.lds = lds + RowPrefetch::LDS_BYTES;
    trail.set_shift(-2);
    const int64_t m = n - ADW;
    const float mf = (float)(int)m;
    float s = 0.0f;
    sweep_rolling(lead, trail, skip, n, [&](int, int tot) { s = s + roll_mean(tot); });
    const float mn = s / mf;
    float q = 0.0f;
    sweep_rolling(lead, trail, skip, n, [&](int, int tot) {
        const float d = roll_mean(tot) - mn;
        q = q + d * d;
    });
    const float sd = sqrtf(q / mf);
    RunFinder F;
    const float bot = mn - sd * ap.std_scale;
    F.init(roll_threshold(bot, false), roll_threshold(bot, true), ap.seg_dist, ap.lo_thresh, ap.hi_thresh);
    // the answer is the first qualifying segment (the reference breaks out of its segment list, src/jnn.c:154-167),
    // and a segment is final once a later one has started without merging into it: nothing after that changes it
    sweep_rolling(lead, trail, skip, n, [&](int i, int tot) { F.step(i, tot); }, [&]() { return !run || F.found != 0; });
    F.finish();
    if (!valid) return;
    sgk_prefix_rec_t *o = a.prefix + r;
    o->n = (uint32_t)n;
    o->reserved = 0;
    o->polya_x = -1; o->polya_y = -1;
    o->adapt_mean = 0.0f; o->adapt_std = 0.0f; o->adapt_median = 0.0f;
    o->polya_mean = 0.0f; o->polya_std = 0.0f; o->polya_median = 0.0f;
    if (!run) { o->adapt_x = -1; o->adapt_y = -1; }
    else if (F.found) { o->adapt_x = F.ans_x + ADW / 2 - 1; o->adapt_y = F.ans_y + ADW / 2 - 1; }
    else { o->adapt_x = 0; o->adapt_y = 0; }
}

// ---------------------------------------------------------------- the launches (stat_args.h)
int launch_k_moments(const char *name, int region, bool hist, hipStream_t st, const StatArgs &a) {
    const uint32_t grid = (a.b.n_reads + 63) / 64;
    if (region == REG_WHOLE && !hist) SGK_LAUNCH(name, (k_moments<REG_WHOLE, false>), grid, 64, st, a);
    else if (region == REG_WHOLE) SGK_LAUNCH(name, (k_moments<REG_WHOLE, true>), grid, 64, st, a);
    else if (region == REG_ADAPT && !hist) SGK_LAUNCH(name, (k_moments<REG_ADAPT, false>), grid, 64, st, a);
    else if (region == REG_ADAPT) SGK_LAUNCH(name, (k_moments<REG_ADAPT, true>), grid, 64, st, a);
    else if (region == REG_POLYA && !hist) SGK_LAUNCH(name, (k_moments<REG_POLYA, false>), grid, 64, st, a);
    else if (region == REG_POLYA) SGK_LAUNCH(name, (k_moments<REG_POLYA, true>), grid, 64, st, a);
    else return SGK_ERR_ARG;
    return SGK_OK;
}
int launch_k_median(const char *name, int region, bool pa, bool flagged, hipStream_t st, const StatArgs &a) {
    const uint32_t grid = a.b.n_reads;
    if (pa) {  // fused stat + pa: whole reads, every read
        if (region != REG_WHOLE || flagged) return SGK_ERR_ARG;
        SGK_LAUNCH(name, (k_median<REG_WHOLE, true, false>), grid, 256, st, a);
    } else if (region == REG_WHOLE && !flagged) SGK_LAUNCH(name, (k_median<REG_WHOLE, false, false>), grid, 256, st, a);
    else if (region == REG_WHOLE) SGK_LAUNCH(name, (k_median<REG_WHOLE, false, true>), grid, 256, st, a);
    else if (region == REG_ADAPT && !flagged) SGK_LAUNCH(name, (k_median<REG_ADAPT, false, false>), grid, 256, st, a);
    else if (region == REG_ADAPT) SGK_LAUNCH(name, (k_median<REG_ADAPT, false, true>), grid, 256, st, a);
    else if (region == REG_POLYA && !flagged) SGK_LAUNCH(name, (k_median<REG_POLYA, false, false>), grid, 256, st, a);
    else if (region == REG_POLYA) SGK_LAUNCH(name, (k_median<REG_POLYA, false, true>), grid, 256, st, a);
    else return SGK_ERR_ARG;
    return SGK_OK;
}
int launch_k_jnn(const char *name, hipStream_t st, const StatArgs &a, const JnnP &p) {
    SGK_LAUNCH(name, k_jnn, (a.b.n_reads + 63) / 64, 64, st, a, p);
    return SGK_OK;
}
int launch_k_polya(hipStream_t st, const StatArgs &a) {
    SGK_LAUNCH("k_polya", k_polya, (a.b.n_reads + 63) / 64, 64, st, a);
    return SGK_OK;
}
int launch_k_polya_param(hipStream_t st, const StatArgs &a, const PolyP &q) {
    SGK_LAUNCH("k_polya_param", k_polya_param, (a.b.n_reads + 63) / 64, 64, st, a, q);
    return SGK_OK;
}
int launch_k_adaptor(hipStream_t st, const StatArgs &a, const AdaptP &p) {
    SGK_LAUNCH("k_adaptor", k_adaptor, (a.b.n_reads + 63) / 64, 64, st, a, p);
    return SGK_OK;
}

}  // namespace sgk
