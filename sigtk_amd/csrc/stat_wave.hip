// stat_wave.hip -- the wave-per-read kernels (round 2, the default): k_stat_wave, k_jnn_wave, k_polya_wave,
// k_adaptor_wave on the building blocks of stat_wave.h.  Long reads that k_long_chains (stat_long.hip) has taken are
// skipped here (find_long) or, when it declined them, redone (long_redo_read).  The sort that hands the reads to the
// waves longest first (k_order_*, launch_order; the event kernels use it too) is here as well.  Must not include
// row_stream.h.
#include "stat_wave.h"

namespace sgk {

constexpr int STAT_WAVES = 4;  // waves per SIMD the register allocation aims at (5: spills, measured slower)
template <int MODE, bool PA>
__global__ __launch_bounds__(256, STAT_WAVES) void k_stat_wave(StatArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t hist_all[4][WH_BINS];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
    const uint32_t widx = blockIdx.x * 4 + wv;  // wave-uniform, and known to be: everything derived from it is scalar
    uint32_t r;
    if (MODE == REG_WHOLE && a.long_redo) {
        if (!long_redo_read(a, widx, r)) return;
    } else {
        if (widx >= a.b.n_reads) return;  // (no workgroup barrier anywhere in this kernel)
        r = a.order ? a.order[widx] : widx;
    }
    uint32_t *hist = hist_all[wv];
    const Region g = get_region(MODE, a.b, a.prefix, r);
    const Scale sc = make_scale(a.b.digitisation[r], a.b.offset[r], a.b.range[r]);
    WaveRead wr;
    wr.init(a.b, g);
    const float nf = (float)(int)g.len;
    // a long read's record (and pA) is k_long_chains' work
    if (MODE == REG_WHOLE && !a.long_redo) {
        const LongSums *lg = find_long(a, r, g.len);
        if (lg && lg->rec_off != LC_NO_REC) return;
    }

    // ---- pass 1: sum of raw, sum of pA (oriented so that the running sum is non-negative); fused stat + pa: the pA of
    // every sample is written here, under the lighter arithmetic of the two passes
    // (both chains: a read whose running raw sum is negative -- signed ADC codes -- would otherwise fail the fast
    // walk's sign test on every tile and be added term by term)
    float m_raw = 0.0f, m_pa = 0.0f, sg = sc.unit < 0.0f ? -1.0f : 1.0f;
    int sraw = 0;
    {
        WaveTile cur, nxt;
        if (wr.ntiles > 0) wr.load(cur, 0);
        float *pa_dst = PA ? a.pa_out + wr.rb : nullptr;
        for (int t = 0; t < wr.ntiles; ++t) {
            if (t + 1 < wr.ntiles) wr.load(nxt, t + 1);
            const Scale so = {sc.offf, sc.unit * sg};
            if (PA) pa_write_tile_lds(wr, t, sc, pa_dst, cur, hist);
            ss_tile2<true>(
                m_raw, m_pa, wr, cur, t, [&](auto b) { return TermRaw<decltype(b)::interior>{b, sraw}; },
                [&](auto b) { return TermPa<decltype(b)::interior>{b, so}; });
            if (m_pa < 0.0f) { m_pa = -m_pa; sg = -sg; }
            if (m_raw < 0.0f) { m_raw = -m_raw; sraw = ~sraw; }
            cur = nxt;
        }
    }
    // (a zero accumulator stands for +0: the reference's sum starts at +0 and x + (-x), +0 + -0 are +0 under
    // round-to-nearest, whichever way the chain was oriented)
    const float mraw = ss_signed(m_raw, sraw != 0) / nf;
    const float mpa = ss_signed(m_pa, sg < 0.0f) / nf;

    // ---- pass 2: squared deviations, window histogram
    const int lo = hist_window_lo(mraw);
#pragma unroll
    for (int i = 0; i < WH_BINS / 64; ++i) hist[i * 64 + lane] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    float q_raw = 0.0f, q_pa = 0.0f;
    {
        WaveTile cur, nxt;
        if (wr.ntiles > 0) wr.load(cur, 0);
        for (int t = 0; t < wr.ntiles; ++t) {
            if (t + 1 < wr.ntiles) wr.load(nxt, t + 1);
            int q_lo, q_hi;
            wr.range(t, 0, q_lo, q_hi);
            if (wr.interior(t)) hist_tile<true>(cur, q_lo, q_hi, lo, hist);
            else hist_tile<false>(cur, q_lo, q_hi, lo, hist);
            ss_tile2<false>(
                q_raw, q_pa, wr, cur, t, [&](auto b) { return TermDevRaw<decltype(b)::interior>{b, mraw}; },
                [&](auto b) { return TermDevPa<decltype(b)::interior>{b, sc, mpa}; });
            cur = nxt;
        }
    }
    const float sdraw = sqrtf(q_raw / nf), sdpa = sqrtf(q_pa / nf);

    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    stat_finish<MODE>(a, r, g, sc, lo, hist, mraw, mpa, sdraw, sdpa);
}

__global__ __launch_bounds__(256) void k_jnn_wave(StatArgs a, JnnP p) {
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
    const uint32_t widx = blockIdx.x * 4 + wv;
    uint32_t r;
    if (a.long_redo) {
        if (!long_redo_read(a, widx, r)) return;
    } else {
        if (widx >= a.b.n_reads) return;
        r = a.order ? a.order[widx] : widx;
    }
    const Region g = get_region(REG_WHOLE, a.b, nullptr, r);
    const int64_t n = g.len;
    if (n <= 0) {
        if (lane == 0) a.n_segs[r] = 0u;
        return;
    }
    WaveRead wr;
    wr.init(a.b, g);
    float top = p.top, bot = p.bot;
    if (p.std_scale > 0.0f) {  // src/jnn.c:195-199
        const float nf = (float)(int)n;
        float s = 0.0f, q = 0.0f;
        // a long read is k_long_chains' (sums, automaton and merge) if its slots have room for 4 096 chunks' headers
        const LongSums *lg = a.long_redo ? nullptr : find_long(a, r, n);
        if (lg && lg->rec_off != LC_NO_REC && jnn_long_cap(a, r, wr.skip + n) >= 4u) return;
        {
            WaveTile cur, nxt;
            wr.load(cur, 0);
            for (int t = 0; t < wr.ntiles; ++t) {
                if (t + 1 < wr.ntiles) wr.load(nxt, t + 1);
                ss_tile1<false>(s, wr, cur, t, [&](auto b) { return TermClamp<decltype(b)::interior>{b}; });
                cur = nxt;
            }
        }
        const float mn = s / nf;
        {
            WaveTile cur, nxt;
            wr.load(cur, 0);
            for (int t = 0; t < wr.ntiles; ++t) {
                if (t + 1 < wr.ntiles) wr.load(nxt, t + 1);
                ss_tile1<false>(q, wr, cur, t, [&](auto b) { return TermDevClamp<decltype(b)::interior>{b, mn}; });
                cur = nxt;
            }
        }
        const float band = sqrtf(q / nf) * p.std_scale;
        top = mn + band;
        bot = mn - band;
    }
    const JnnThr th = jnn_thresholds(top, bot, p);

    // ---- the automaton, in chunks between sync points (jnn_chunks); kept segments are staged in the upper half of the
    // read's slots (a part per lane), the merged segments go to the lower half
    const int64_t nq = wr.skip + n;
    const int C = jnn_chunk_lanes(nq);
    const uint64_t slot0 = a.seg_slots[r], cap = a.seg_slots[r + 1] - slot0;
    const uint32_t half = (uint32_t)(cap / 2), capL = (uint32_t)((cap - half) / (uint32_t)C);
    int32_t *stage_x = a.seg_x + slot0 + half + (uint64_t)lane * capL, *stage_y = a.seg_y + slot0 + half + (uint64_t)lane * capL;

    int fx = 0, fy = 0, fstrong = 0, has_first = 0;
    uint32_t cnt = 0u;

    // a segment that ended with c >= keep_min samples: the lane's first one is kept in registers (whether it is kept
    // depends on the lanes in front), later ones only matter if c >= window
    auto candidate = [&](int sx, int sy, int c) {
        const int strong = c >= p.window ? 1 : 0;
        if (!has_first) { has_first = 1; fx = sx; fy = sy; fstrong = strong; }
        else if (strong) {
            if (cnt < capL) { stage_x[cnt] = sx; stage_y[cnt] = sy; }
            ++cnt;  // (more than capL: jnn_merge_round reports the overflow)
        }
    };
    jnn_chunks(wr, n, th.hi_r, th.lo_r, p.error, th.keep_min, candidate, C, 0);

    // A lane's staging part is sized for chunks that end where they should; a read with too few sync points (a lane ran
    // on through many chunks and kept more segments than its part holds) is handed to the lane-per-read kernel instead
    JnnCarry cy = {false, false, false, 0, 0u};
    jnn_merge_round<false>(cy, has_first, fx, fy, fstrong, cnt, capL, stage_x, stage_y, p.seg_dist, a.seg_x + slot0,
                           a.seg_y + slot0, half);
    const uint32_t total = jnn_merge_flush(cy, a.seg_y + slot0, half);
    if (lane == 0) a.n_segs[r] = total;
}

// ---------------------------------------------------------------- find_polya, one WAVE per read
// k_polya_wave is k_polya_wave_t<false> of stat_wave.h (the kernel is a template there so that stat_param.hip can
// instantiate it with a caller's set; as a device function called from two kernels the preset kernel took more registers)

__global__ __launch_bounds__(256) void k_adaptor_wave(StatArgs a, AdaptP ap) {
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
    const uint32_t widx = blockIdx.x * 4 + wv;
    uint32_t r;
    if (a.long_redo) {
        if (!long_redo_read(a, widx, r)) return;
    } else {
        if (widx >= a.b.n_reads) return;
        r = a.order ? a.order[widx] : widx;
    }
    __shared__ uint4 ring_all[4][ROLL_RING_BYTES / 16];
    uint4 *ring = ring_all[wv];
    const Region g = get_region(REG_WHOLE, a.b, nullptr, r);
    const int64_t n = g.len;
    // a long read is k_long_chains' (which runs beside this kernel): its sums, thresholds, run finder and record
    const LongSums *lg = a.long_redo ? nullptr : find_long(a, r, n);
    if (lg && lg->rec_off != LC_NO_REC) return;
    sgk_prefix_rec_t *o = a.prefix + r;
    if (lane == 0) adaptor_init_rec(o, n);
    if (n <= ADW) {  // "Not enough data to trim", src/jnn.c:173-177
        if (lane == 0) { o->adapt_x = -1; o->adapt_y = -1; }
        return;
    }
    const int64_t m = n - ADW;  // number of rolling means
    WaveRead wr;
    wr.init(a.b, Region{g.start, m});

    // total of the first window: clamped samples 0 .. 1999 (tile-local positions skip .. skip + 1999 of tiles 0 and 1)
    const int first_total = window_total(wr, 0, wr.skip);
    const float mf = (float)(int)m;
    float s = 0.0f;
    roll_sweep(wr, first_total, [&](int t, const int (&tot)[SS_SPL]) {
        roll_chain_tile(s, wr, t, tot, [](int v) { return roll_mean(v); });
        return false;
    }, ring);
    const float mn = s / mf;
    float q = 0.0f;
    roll_sweep(wr, first_total, [&](int t, const int (&tot)[SS_SPL]) {
        roll_chain_tile(q, wr, t, tot, [&](int v) { const float d = roll_mean(v) - mn; return d * d; });
        return false;
    }, ring);
    adaptor_find(wr, first_total, s, q, mf, ap, o, ring);
}

// ---------------------------------------------------------------- dispatch order of the wave-per-read kernels
// A wave-per-read kernel cannot finish before its longest read has: reads are handed to the waves longest first
// (workgroups start in index order), by a counting sort of the read lengths into 128 buckets (4 per octave).
// (per-workgroup LDS histograms first: a batch of equal-length reads would otherwise send every atomic to one word)
__global__ __launch_bounds__(256) void k_order_count(const uint32_t *lengths, uint32_t n, uint32_t *hist) {
    __shared__ uint32_t h[128];
    if (threadIdx.x < 128) h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r < n) atomicAdd(&h[len_bucket(lengths[r])], 1u);
    __syncthreads();
    if (threadIdx.x < 128 && h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}
__global__ void k_order_scan(uint32_t *hist /* 128 counts -> cursors, longest bucket first */) {
    if (threadIdx.x == 0) {
        uint32_t acc = 0u;
        for (int b = 127; b >= 0; --b) { const uint32_t c = hist[b]; hist[b] = acc; acc += c; }
    }
}
__global__ __launch_bounds__(256) void k_order_fill(const uint32_t *lengths, uint32_t n, uint32_t *cursor, uint32_t *order) {
    __shared__ uint32_t h[128], base[128];
    if (threadIdx.x < 128) h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    uint32_t b = 0u, local = 0u;
    if (r < n) { b = len_bucket(lengths[r]); local = atomicAdd(&h[b], 1u); }
    __syncthreads();
    if (threadIdx.x < 128 && h[threadIdx.x]) base[threadIdx.x] = atomicAdd(&cursor[threadIdx.x], h[threadIdx.x]);
    __syncthreads();
    if (r < n) order[base[b] + local] = r;
}
int launch_order(const uint32_t *lengths, uint32_t nr, uint32_t *order, uint32_t *hist, hipStream_t st) {
    SGK_HIP_TRY(hipMemsetAsync(hist, 0, 128 * 4, st));
    SGK_LAUNCH_UNTIMED(k_order_count, (nr + 255) / 256, 256, st, lengths, nr, hist);
    SGK_LAUNCH_UNTIMED(k_order_scan, 1, 64, st, hist);
    SGK_LAUNCH_UNTIMED(k_order_fill, (nr + 255) / 256, 256, st, lengths, nr, hist, order);
    return SGK_OK;
}

// ---------------------------------------------------------------- the launches (stat_args.h)
int launch_k_stat_wave(const char *name, int region, bool pa, uint32_t grid, hipStream_t st, const StatArgs &a) {
    if (pa) {  // fused stat + pa: whole reads
        if (region != REG_WHOLE) return SGK_ERR_ARG;
        SGK_LAUNCH(name, (k_stat_wave<REG_WHOLE, true>), grid, 256, st, a);
    } else if (region == REG_WHOLE) SGK_LAUNCH(name, (k_stat_wave<REG_WHOLE, false>), grid, 256, st, a);
    else if (region == REG_ADAPT) SGK_LAUNCH(name, (k_stat_wave<REG_ADAPT, false>), grid, 256, st, a);
    else if (region == REG_POLYA) SGK_LAUNCH(name, (k_stat_wave<REG_POLYA, false>), grid, 256, st, a);
    else return SGK_ERR_ARG;
    return SGK_OK;
}
int launch_k_jnn_wave(const char *name, uint32_t grid, hipStream_t st, const StatArgs &a, const JnnP &p) {
    SGK_LAUNCH(name, k_jnn_wave, grid, 256, st, a, p);
    return SGK_OK;
}
int launch_k_polya_wave(hipStream_t st, const StatArgs &a) {
    SGK_LAUNCH("k_polya_wave", k_polya_wave_t<false>, (a.b.n_reads + 3) / 4, 256, st, a, PolyP{});
    return SGK_OK;
}
int launch_k_adaptor_wave(const char *name, uint32_t grid, hipStream_t st, const StatArgs &a, const AdaptP &p) {
    SGK_LAUNCH(name, k_adaptor_wave, grid, 256, st, a, p);
    return SGK_OK;
}

}  // namespace sgk
