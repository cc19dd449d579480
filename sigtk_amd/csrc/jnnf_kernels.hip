// jnnf_kernels.hip -- sgk_jnn_f32: jnn_pa (src/jnn.c:295-306) of every read of a float batch, jnn_core over rm_outlierf(x)
// with any parameter set of sgk_jnn_params_check's domain, and per-read fixed thresholds for find_polya (src/jnn.c:352-374).
// What k_jnn_f32 (shims.hip) does for one array per launch with all 64 lanes walking it, in a batch shape:
//   * k_jnnf_wave, one WAVE per read (float_reads.h):
//       - the thresholds: given per read (top[r], bot[r]), fixed (p.top, p.bot), or mean -+ std_scale * deviation of the
//         clamped values from the two sequential sums (seqsum.h), one coalesced sweep each;
//       - one more coalesced sweep turns the read into in-range MASKS, a bit per value: bot < clamp(x) < top, compared in
//         float, strictly, as jnn_core does -- so -0.0, NaN samples (a NaN passes the clamp and is then out of range), NaN
//         thresholds and thresholds between representable values need no thought (the int16 kernels' integer
//         thresholds, jnn_thresholds, do not carry over).  The masks (1 / 32 of the read's bytes) stay in the wave's
//         LDS for reads of up to 16 384 positions and else go to a row of the workspace the wave takes from a bump
//         counter (200 000 short reads on one counter cost more than their sweeps);
//       - the automaton runs on those masks in chunks between sync points, lane per chunk: jnn_chunks_src of stat_wave.h,
//         the int16 kernels' own, with the masks as its source; staging in the upper half of the read's slots and the
//         merge (jnn_merge_round) are k_jnn_wave's.
//   * k_jnnf_literal behind it, one read per LANE, the literal loop (JnnAuto, the whole automaton) on the thresholds the
//     wave kernel left in the workspace.  It takes the reads the wave kernel marked: every read of a parameter set the
//     chunked form cannot run (error >= corrector: the `err--` correction of jnn.c:228,238 can fire; error > 31;
//     window < 128), and reads whose staging overflowed, whose slots are too small or whose mask row found no room.
// A read is never split over workgroups (float_reads.h).
#include "float_reads.h"
#include "stat_wave.h"

namespace sgk {

struct JnnfArgs {
    const float *top, *bot;       // per-read thresholds, or both null
    const uint64_t *seg_slots;
    int32_t *seg_x, *seg_y;
    uint32_t *n_segs;
    uint32_t *err_count;          // workspace word 0: reads whose segments overflowed their slots
    unsigned long long *mask_used;  // workspace: mask words handed out
    float2 *thr;                  // workspace: the thresholds of read r
    uint32_t *masks;
    unsigned long long mask_words;  // capacity of `masks`
    uint32_t literal_all;         // the set is not one the chunked form can run: thresholds only
};

struct JnnSrcBits {  // jnn_chunks_src on masks: bit q & 31 of row[q >> 5] is position q of the read
    const uint32_t *row;
    int64_t nw;
    uint32_t w[2];
    __device__ __forceinline__ int64_t skew(int64_t qb) const { return qb & 63; }
    __device__ __forceinline__ void load_line(int64_t q) {
        const int64_t i = q >> 5;  // even: the row is 8-byte aligned
        uint2 u = make_uint2(0u, 0u);
        if (i >= 0 && i + 1 < nw) u = *reinterpret_cast<const uint2 *>(row + i);
        w[0] = u.x; w[1] = u.y;
    }
    __device__ __forceinline__ uint32_t block_mask(int h) const { return w[h]; }
};

constexpr int JF_LDS_WORDS = 512;  // mask words a wave keeps in LDS: reads of up to 16 384 positions

__global__ __launch_bounds__(256) void k_jnnf_wave(FloatBatch b, JnnP p, JnnfArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t lds_rows[4][JF_LDS_WORDS];
    const int lane = lane_id();
    uint32_t r;
    if (!float_wave_read(b, r)) return;
    FloatRead fr;
    fr.init(b, r);
    const int n = fr.n;
    if (n == 0) {
        if (lane == 0) a.n_segs[r] = 0u;
        return;
    }
    float top = p.top, bot = p.bot;
    if (a.top) { top = a.top[r]; bot = a.bot[r]; }
    else if (p.std_scale > 0.0f) {  // src/jnn.c:195-199 on rm_outlierf's values
        auto none = [](int, const float (&)[SS_SPL], uint32_t) {};
        const float s = fr_chain(fr, [](float v) { return clampf_pa(v); }, none);
        const float mn = s / (float)n;
        const float q = fr_chain(fr, [&](float v) { const float d = clampf_pa(v) - mn; return d * d; }, none);
        const float band = sqrtf(q / (float)n) * p.std_scale;
        top = mn + band;
        bot = mn - band;
    }
    if (lane == 0) a.thr[r] = make_float2(top, bot);

    // ---- the masks' row: in the wave's LDS where it fits (reads of up to 32 * JF_LDS_WORDS positions: no counter, no
    // global round trip), else a row of the workspace from the bump counter
    if (a.literal_all) {
        if (lane == 0) a.n_segs[r] = JNN_REDO_MARK;
        return;
    }
    const int64_t nw = (fr.nq + 63) / 64 * 2;
    const bool in_lds = nw <= JF_LDS_WORDS;
    uint32_t *row = lds_rows[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
    if (!in_lds) {
        unsigned long long base = 0ull;
        if (lane == 0) base = atomicAdd(a.mask_used, (unsigned long long)nw);
        base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) |
               (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if (base + (unsigned long long)nw > a.mask_words) {
            if (lane == 0) a.n_segs[r] = JNN_REDO_MARK;
            return;
        }
        row = a.masks + base;
    }
    fr_sweep(fr, [&](int t, const float (&x)[SS_SPL], uint32_t vm) {
        uint32_t m = 0u;
#pragma unroll
        for (int e = 0; e < SS_SPL; ++e) {
            const float c = clampf_pa(x[e]);
            m |= (uint32_t)((c < top) & (c > bot)) << e;
        }
        m &= vm;
        const uint32_t hi = (uint32_t)__shfl_down((int)m, 1, 64);
        const int64_t wi = (int64_t)t * (SS_TILE / 32) + (lane >> 1);
        if (!(lane & 1) && wi < nw) row[wi] = m | (hi << 16);
    });
    // the row is read back by other lanes of this wave
    if (in_lds) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    else __threadfence();
    __builtin_amdgcn_wave_barrier();

    // ---- the automaton, in chunks between sync points; kept segments are staged in the upper half of the read's slots
    // (a part per lane), the merged segments go to the lower half (k_jnn_wave)
    const int C = jnn_chunk_lanes(fr.nq);
    const uint64_t slot0 = a.seg_slots[r], cap = a.seg_slots[r + 1] - slot0;
    const uint32_t half = (uint32_t)(cap / 2), capL = (uint32_t)((cap - half) / (uint32_t)C);
    int32_t *stage_x = a.seg_x + slot0 + half + (uint64_t)lane * capL, *stage_y = a.seg_y + slot0 + half + (uint64_t)lane * capL;
    const int first_min_i = (int)ceilf((float)p.window * p.stall_len);  // (float)c >= window * stall_len
    const int keep_min = first_min_i < p.window ? first_min_i : p.window;
    int fx = 0, fy = 0, fstrong = 0, has_first = 0;
    uint32_t cnt = 0u;
    auto candidate = [&](int sx, int sy, int c) {
        const int strong = c >= p.window ? 1 : 0;
        if (!has_first) { has_first = 1; fx = sx; fy = sy; fstrong = strong; }
        else if (strong) {
            if (cnt < capL) { stage_x[cnt] = sx; stage_y[cnt] = sy; }
            ++cnt;  // (more than capL: jnn_merge_round reports the overflow)
        }
    };
    JnnSrcBits src = {row, nw, {0u, 0u}};
    jnn_chunks_src(src, fr.skip, (int64_t)n, p.error, keep_min, candidate, C, 0);
    JnnCarry cy = {false, false, false, 0, 0u};
    jnn_merge_round<false>(cy, has_first, fx, fy, fstrong, cnt, capL, stage_x, stage_y, p.seg_dist, a.seg_x + slot0,
                           a.seg_y + slot0, half);
    const uint32_t total = jnn_merge_flush(cy, a.seg_y + slot0, half);
    if (lane == 0) a.n_segs[r] = total;
}

__global__ __launch_bounds__(64) void k_jnnf_literal(FloatBatch b, JnnP p, JnnfArgs a) {
    const uint32_t r = blockIdx.x * 64 + lane_id();
    const bool valid = r < b.n_reads && a.n_segs[r] == JNN_REDO_MARK;
    if (!__any(valid)) return;
    const float *x = valid ? b.x + b.offsets[r] : nullptr;
    const int n = valid ? (int)b.lengths[r] : 0;
    const float2 th = valid ? a.thr[r] : make_float2(0.0f, 0.0f);
    JnnAuto A;
    A.init(th.x, th.y, p.corrector, p.seg_dist, p.window, p.stall_len, p.error);
    const uint64_t slot0 = valid ? a.seg_slots[r] : 0, cap = valid ? a.seg_slots[r + 1] - slot0 : 0;
    bool overflow = false;
    auto emit = [&](int k, int sx, int sy) {
        if ((uint64_t)k < cap) { a.seg_x[slot0 + k] = sx; a.seg_y[slot0 + k] = sy; }
        else overflow = true;
    };
    for (int j = 0; j < n; ++j) A.step(j, A.in_mask_f(clampf_pa(x[j])), emit);
    A.finish(emit);
    if (valid) a.n_segs[r] = (uint32_t)A.nseg;
    if (overflow) atomicAdd(a.err_count, 1u);
}

// ---- the workspace: [0, 64) counters (word 0: reads that overflowed their slots, as sgk_jnn_param; bytes 8 .. 15: mask
// words handed out), the dispatch order, two floats per read, the mask rows (two words per 64 positions of a read, whose
// first position can lie up to 3 values in front of the read: n_values / 32 + 3 per read bounds them)
static size_t jnnf_thr_off(uint32_t n_reads) { return order_workspace_bytes(n_reads); }
static size_t jnnf_mask_off(uint32_t n_reads) { return jnnf_thr_off(n_reads) + round_up((uint64_t)n_reads * sizeof(float2), 64); }
static uint64_t jnnf_mask_words(uint32_t n_reads, uint64_t n_values) { return n_values / 32 + 3ull * n_reads + 64; }
static size_t jnnf_ws(uint32_t n_reads, uint64_t n_values) {
    return jnnf_mask_off(n_reads) + (size_t)jnnf_mask_words(n_reads, n_values) * sizeof(uint32_t);
}

}  // namespace sgk

using namespace sgk;

extern "C" {

size_t sgk_jnn_f32_workspace_bytes(uint32_t n_reads, uint64_t n_values, uint32_t max_read_len) {
    (void)max_read_len;
    return jnnf_ws(n_reads, n_values);
}

int sgk_jnn_f32(const float *x, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads, uint32_t max_read_len,
                uint64_t n_values, const sgk_jnn_param_t *p, const float *top, const float *bot, const uint64_t *seg_slots,
                int32_t *seg_x, int32_t *seg_y, uint32_t *n_segs, void *ws, size_t ws_bytes, void *stream) {
    if (sgk_jnn_params_check(p) != SGK_OK) return SGK_ERR_ARG;
    if ((top == nullptr) != (bot == nullptr) || (top && p->std_scale > 0.0f)) return SGK_ERR_ARG;
    SGK_TRY(float_batch_check(x, offsets, lengths, n_reads, max_read_len));
    if (n_reads == 0) return SGK_OK;
    if (!seg_slots || !seg_x || !seg_y || !n_segs || !ws || (reinterpret_cast<uintptr_t>(ws) & 15u)) return SGK_ERR_ARG;
    if (ws_bytes < jnnf_ws(n_reads, n_values)) return SGK_ERR_WORKSPACE;
    if (sgk_device_count() <= 0) return SGK_ERR_NODEVICE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const JnnP q = to_jnnp(*p);
    char *w = static_cast<char *>(ws);
    SGK_HIP_TRY(hipMemsetAsync(w, 0, 64, st));
    FloatBatch b = {x, offsets, lengths, n_reads, nullptr};
    SGK_TRY(float_batch_order(b, ws, st));
    JnnfArgs a;
    a.top = top; a.bot = bot;
    a.seg_slots = seg_slots; a.seg_x = seg_x; a.seg_y = seg_y; a.n_segs = n_segs;
    a.err_count = reinterpret_cast<uint32_t *>(w);
    a.mask_used = reinterpret_cast<unsigned long long *>(w + 8);
    a.thr = reinterpret_cast<float2 *>(w + jnnf_thr_off(n_reads));
    a.masks = reinterpret_cast<uint32_t *>(w + jnnf_mask_off(n_reads));
    a.mask_words = jnnf_mask_words(n_reads, n_values);
    // (the route of sgk_jnn_param, stat_launch.hip: launch_jnn)
    const bool wave_ok = q.error >= 0 && q.error < q.corrector && q.error <= 31 && q.window >= 128;
    a.literal_all = wave_ok ? 0u : 1u;
    SGK_LAUNCH("k_jnnf_wave", k_jnnf_wave, (n_reads + 3) / 4, 256, st, b, q, a);
    SGK_LAUNCH("k_jnnf_literal", k_jnnf_literal, (n_reads + 63) / 64, 64, st, b, q, a);
    return SGK_OK;
}

}  // extern "C"
