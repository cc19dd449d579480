// stat_param.hip -- k_adaptor_param: find_adaptor / jnnv2 (src/jnn.c:99-188) with a caller's window, 2 .. 13 981
// (sgk_prefix_param, sgk_jnnv2_param).  The preset kernels (k_adaptor, k_adaptor_wave, k_long_chains) have the window
// 2000 in their tile geometry and in the constant division; this one takes it at run time:
//   * one WAVEFRONT per read, of any length -- there is no long-read split, a read of 10^6 samples takes one wavefront
//     three sweeps of 10^6 windows;
//   * tiles of 64 x SS_SPL window indices, lane l owns 16 consecutive ones: the tot[SS_SPL] layout roll_tile,
//     roll_chain_tile and the run finder of adaptor_find_ws (stat_wave.h) work on, shared with the preset kernels
//     through their window source (WinParam, stat_device.h);
//   * the rolling totals are integers: the first window's total is a plain reduction, a lane's first total is the tile
//     carry plus a wave scan of the lanes' lead-minus-trail sums (roll_tile);
//   * the leading samples lie `window` samples behind the trailing ones, at any 2-byte residue, and the read itself
//     starts anywhere in the arena: load16 reads whole dwords where 16 samples and the dwords that hold them lie
//     inside the read, and sample by sample, each behind its own bounds test, everywhere else.  No byte outside the
//     read's [0, n) is touched;
//   * t = (float)tot / (float)window is the correctly rounded quotient (WinParam).
#include "stat_wave.h"

namespace sgk {

// samples c[i0 .. i0 + 16) of the read `s` of n samples, two per word; samples outside [0, n) read as 0 (their clamp)
__device__ __forceinline__ void load16(const int16_t *s, int64_t n, int64_t i0, uint32_t (&w)[SS_SPL / 2]) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(s + i0);
    if (i0 >= 0 && i0 + SS_SPL <= n && (addr & 3u) == 0u) {
        const uint32_t *p = reinterpret_cast<const uint32_t *>(s + i0);
#pragma unroll
        for (int k = 0; k < SS_SPL / 2; ++k) w[k] = p[k];
    } else if (i0 >= 1 && i0 + SS_SPL + 1 <= n && (addr & 3u) == 2u) {  // dwords from sample i0 - 1 to sample i0 + 16
        const uint32_t *p = reinterpret_cast<const uint32_t *>(s + i0 - 1);
        uint32_t prev = p[0];
#pragma unroll
        for (int k = 0; k < SS_SPL / 2; ++k) {
            const uint32_t nx = p[k + 1];
            w[k] = (prev >> 16) | (nx << 16);
            prev = nx;
        }
    } else {
#pragma unroll
        for (int k = 0; k < SS_SPL / 2; ++k) {
            const int64_t i = i0 + 2 * k;
            const uint32_t lo = (i >= 0 && i < n) ? (uint32_t)(uint16_t)s[i] : 0u;
            const uint32_t hi = (i + 1 >= 0 && i + 1 < n) ? (uint32_t)(uint16_t)s[i + 1] : 0u;
            w[k] = lo | (hi << 16);
        }
    }
}
__device__ __forceinline__ void load16_clamped(const int16_t *s, int64_t n, int64_t i0, WaveTile &x) {
    load16(s, n, i0, x.w);
#pragma unroll
    for (int k = 0; k < SS_SPL / 2; ++k) x.w[k] = __builtin_bit_cast(uint32_t, clamp_raw2(x.w[k]));
}

// total of the first window: clamped samples 0 .. win - 1 (win < n)
__device__ inline int param_first_total(const int16_t *s, int win) {
    int part = 0;
    for (int64_t i0 = (int64_t)lane_id() * SS_SPL; i0 < win; i0 += SS_TILE) {
        WaveTile x;
        load16_clamped(s, win, i0, x);  // (bound: the window -- what lies behind it reads as 0)
#pragma unroll
        for (int k = 0; k < SS_SPL / 2; ++k) {
            const s16x2 c = __builtin_bit_cast(s16x2, x.w[k]);
            part += (int)c.x + (int)c.y;
        }
    }
    return wave_last_i(wave_incl_scan_i(part));
}

// one sweep over the rolling totals of the read's windows: f(t, tot) per tile of SS_TILE window indices; stops when f
// returns true (wave-uniform).  Window indices at or behind n - win get totals nobody uses (the callers mask them).
template <typename F>
__device__ __forceinline__ void param_sweep(const int16_t *s, int64_t n, int win, int ntiles, int first_total, F f) {
    int T0 = first_total;
#pragma unroll 1
    for (int t = 0; t < ntiles; ++t) {
        const int64_t i0 = (int64_t)t * SS_TILE + (int64_t)lane_id() * SS_SPL;
        WaveTile tr, ld;
        load16_clamped(s, n, i0, tr);
        load16_clamped(s, n, i0 + win, ld);
        int tot[SS_SPL];
        roll_tile<false, true>(tr, ld, 0, T0, tot);
        if (f(t, tot)) break;
    }
}

__global__ __launch_bounds__(256) void k_adaptor_param(StatArgs a, AdaptP ap, int win) {
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
    const uint32_t widx = blockIdx.x * 4 + wv;
    if (widx >= a.b.n_reads) return;
    const uint32_t r = a.order ? a.order[widx] : widx;
    const Region g = get_region(REG_WHOLE, a.b, nullptr, r);
    const int64_t n = g.len;
    sgk_prefix_rec_t *o = a.prefix + r;
    if (lane == 0) adaptor_init_rec(o, n);
    if (n <= win) {  // "Not enough data to trim", src/jnn.c:173-177
        if (lane == 0) { o->adapt_x = -1; o->adapt_y = -1; }
        return;
    }
    const int16_t *s = a.b.samples + g.start;
    const int64_t m = n - win;  // number of rolling means
    const WinParam ws = {win, (float)win};
    // what roll_chain_tile and the run finder ask a WaveRead: which window indices of a tile exist (index 0 is
    // tile-local position 0: no skip)
    WaveRead wr;
    wr.samples = a.b.samples;
    wr.n_total = (int64_t)a.b.n_samples;
    wr.rb = g.start;
    wr.skip = 0;
    wr.len = m;
    wr.ntiles = (int)((m + SS_TILE - 1) / SS_TILE);

    const int first_total = param_first_total(s, win);
    const float mf = (float)(int)m;
    float sum = 0.0f;
    param_sweep(s, n, win, wr.ntiles, first_total, [&](int t, const int (&tot)[SS_SPL]) {
        roll_chain_tile(sum, wr, t, tot, [&](int v) { return ws.mean(v); });
        return false;
    });
    const float mn = sum / mf;
    float q = 0.0f;
    param_sweep(s, n, win, wr.ntiles, first_total, [&](int t, const int (&tot)[SS_SPL]) {
        roll_chain_tile(q, wr, t, tot, [&](int v) { const float d = ws.mean(v) - mn; return d * d; });
        return false;
    });
    adaptor_find_ws(wr, sum, q, mf, ap, o, ws, [&](auto f) { param_sweep(s, n, win, wr.ntiles, first_total, f); });
}

// the kernel's own quotient for the totals 0 .. n - 1 (tests: against IEEE division, every total of a window)
__global__ __launch_bounds__(256) void k_roll_means_param(int win, uint32_t n, float *out) {
    const WinParam ws = {win, (float)win};
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) out[i] = ws.mean((int)i);
}

int launch_k_adaptor_param(hipStream_t st, const StatArgs &a, const AdaptP &p, int window) {
    if (window < 2 || window > 13981) return SGK_ERR_ARG;
    SGK_LAUNCH("k_adaptor_param", k_adaptor_param, (a.b.n_reads + 3) / 4, 256, st, a, p, window);
    return SGK_OK;
}
int launch_k_polya_wave_param(hipStream_t st, const StatArgs &a, const PolyP &q) {
    if (!polya_wave_ok(q)) return SGK_ERR_ARG;
    SGK_LAUNCH("k_polya_wave_param", k_polya_wave_t<true>, (a.b.n_reads + 3) / 4, 256, st, a, q);
    return SGK_OK;
}
int launch_k_roll_means_param(hipStream_t st, int window, uint32_t n, float *out) {
    if (window < 2 || window > 13981 || !out) return SGK_ERR_ARG;
    if (n == 0) return SGK_OK;
    const uint32_t grid = (n + 255u) / 256u;
    SGK_LAUNCH_UNTIMED(k_roll_means_param, grid > 4096u ? 4096u : grid, 256, st, window, n, out);
    return SGK_OK;
}

}  // namespace sgk
