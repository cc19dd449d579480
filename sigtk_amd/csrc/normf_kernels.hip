// normf_kernels.hip -- sgk_normalise_f32 / sgk_normalise: every read of a float batch as y = (x - shift) / scale, in float32,
// one rounding per operation:
//   SGK_NORM_ZSCORE  shift = meanf(x),   scale = stdvf(x)
//   SGK_NORM_MEDMAD  shift = medianf(x), scale = medianf(|x - shift|) * 1.4826f
//   * launch_statf first (statf_kernels.hip): mean, deviation, median and flags of every read, bit for bit the reference's,
//     into a record array in the workspace.  The sign of a zero median decides the sign of x - shift for a zero x, so
//     shift comes from that path with its literal redo and not from a selection of this unit's own.
//   * k_normf_wave<method>, one WAVE per read (float_reads.h), longest reads first:
//       z-score   one write sweep;
//       med-MAD   three counting sweeps over the keys of fabsf(x - shift), 11 + 11 + 10 bits in the wave's 2 048-bin LDS
//                 histogram (statf_radix.h), then the write sweep.  The deviations hold no negative value and no -0, so
//                 the histogram's order statistic of rank n / 2 is bit for bit ks_ksmall's: no literal redo.
//     A read holding a NaN or an infinity has a mean that is not finite; only behind such a mean (which a sum that
//     overflowed has too) a sweep looks for the value itself.  If there is one, shift and scale are NaN and with them
//     every y of the read.
// The z-score kernel has no histogram and no LDS.  No workgroup barrier anywhere; a read is never split over workgroups.
#include "statf_radix.h"

namespace sgk {

template <int METHOD>
__global__ __launch_bounds__(256) void k_normf_wave(FloatBatch b, const sgk_statf_rec_t *stat, float *y, sgk_norm_rec_t *rec) {
    uint32_t r;
    if (!float_wave_read(b, r)) return;
    FloatRead fr;
    fr.init(b, r);
    const int n = fr.n;
    const float nan = __builtin_nanf("");
    if (n == 0) {  // nothing of y is written
        if (lane_id() == 0) rec[r] = sgk_norm_rec_t{nan, nan, 0u, 0u};
        return;
    }
    const sgk_statf_rec_t s = stat[r];
    uint32_t flags = s.flags & SGK_MEDIAN_INEXACT;
    float shift = METHOD == SGK_NORM_ZSCORE ? s.mean : s.median, scale = s.std;
    bool hostile = false;
    if (!(fabsf(s.mean) < __builtin_inff())) {  // (wave-uniform) a NaN or an infinity among the values, or a sum that overflowed
        uint32_t h = 0u;
        fr_sweep(fr, [&](int, const float (&x)[SS_SPL], uint32_t vm) {
#pragma unroll
            for (int e = 0; e < SS_SPL; ++e) h |= (uint32_t)(((vm >> e) & 1u) && !(fabsf(x[e]) < __builtin_inff()));
        });
        hostile = __ballot(h != 0u) != 0ull;
    }
    if (hostile) {
        shift = scale = nan;
        flags |= SGK_NORM_NONFINITE;
    } else if constexpr (METHOD == SGK_NORM_MEDMAD) {
        __shared__ __attribute__((aligned(16))) uint32_t hist_all[4][SF_BINS];
        uint32_t *hist = hist_all[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
        const float med = shift;
        const auto dev = [med](float v) { return fabsf(v - med); };
        uint32_t rank = (uint32_t)(n / 2);
        statf_clear(hist);
        fr_sweep(fr, [&](int, const float (&x)[SS_SPL], uint32_t vm) { statf_count(x, vm, 0u, 0u, 21, 0x7ffu, hist, dev); });
        uint32_t prefix = statf_pick(hist, rank) << 21;
        statf_clear(hist);
        fr_sweep(fr, [&](int, const float (&x)[SS_SPL], uint32_t vm) { statf_count(x, vm, 0xffe00000u, prefix, 10, 0x7ffu, hist, dev); });
        prefix |= statf_pick(hist, rank) << 10;
        statf_clear(hist);
        fr_sweep(fr, [&](int, const float (&x)[SS_SPL], uint32_t vm) { statf_count(x, vm, 0xfffffc00u, prefix, 0, 0x3ffu, hist, dev); });
        prefix |= statf_pick(hist, rank);
        scale = statf_unkey(prefix) * 1.4826f;
    }
    if (scale == 0.0f) flags |= SGK_NORM_ZERO_SCALE;
    // The write sweep.  y may be x itself: every sweep that reads the read is over by now, a position is written by the
    // lane that loaded it, and fr_sweep loads tile t + 1 before tile t is handed out and stored -- no value is read after
    // it was overwritten.  Each quotient is one subtraction and one correctly rounded division (build.py's flags),
    // subnormal results kept.
    float *yq = y + b.offsets[r] - fr.skip;
    const bool aligned = (reinterpret_cast<uintptr_t>(yq) & 15u) == 0u;
    fr_sweep(fr, [&](int t, const float (&x)[SS_SPL], uint32_t) {
        float v[SS_SPL];
#pragma unroll
        for (int e = 0; e < SS_SPL; ++e) v[e] = (x[e] - shift) / scale;
        fr.store(yq, aligned, v, t);
    });
    if (lane_id() == 0) rec[r] = sgk_norm_rec_t{shift, scale, (uint32_t)n, flags};
}

// ---- the workspace: that of sgk_stat_f32 (counters, dispatch order, literal rows), then the batch's sgk_statf_rec_t
static size_t normf_stat_bytes(uint32_t n_reads, uint64_t n_values, uint32_t max_read_len) {
    return (sgk_stat_f32_workspace_bytes(n_reads, n_values, max_read_len) + 15u) & ~(size_t)15u;
}
static size_t normf_ws(uint32_t n_reads, uint64_t n_values, uint32_t max_read_len) {
    return normf_stat_bytes(n_reads, n_values, max_read_len) + (size_t)n_reads * sizeof(sgk_statf_rec_t);
}
static bool norm_method_ok(int method) { return method == SGK_NORM_ZSCORE || method == SGK_NORM_MEDMAD; }

// x may be y (in place).  ws: 16-byte aligned, normf_ws bytes
static int launch_normf(FloatBatch b, uint32_t max_read_len, uint64_t n_values, int method, float *y, sgk_norm_rec_t *rec, void *ws,
                        hipStream_t st) {
    SGK_TRY(float_batch_order(b, ws, st));
    sgk_statf_rec_t *stat = reinterpret_cast<sgk_statf_rec_t *>(static_cast<char *>(ws) + normf_stat_bytes(b.n_reads, n_values, max_read_len));
    SGK_TRY(launch_statf_ordered(b, max_read_len, stat, ws, st));
    if (method == SGK_NORM_ZSCORE)
        SGK_LAUNCH("k_normf_wave_zscore", k_normf_wave<SGK_NORM_ZSCORE>, (b.n_reads + 3) / 4, 256, st, b, stat, y, rec);
    else
        SGK_LAUNCH("k_normf_wave_medmad", k_normf_wave<SGK_NORM_MEDMAD>, (b.n_reads + 3) / 4, 256, st, b, stat, y, rec);
    return SGK_OK;
}

}  // namespace sgk

using namespace sgk;

extern "C" {

size_t sgk_normalise_f32_workspace_bytes(uint32_t n_reads, uint64_t n_values, uint32_t max_read_len) {
    return normf_ws(n_reads, n_values, max_read_len);
}
size_t sgk_normalise_workspace_bytes(uint32_t n_reads, uint64_t n_samples, uint32_t max_read_len) {
    return normf_ws(n_reads, n_samples, max_read_len);
}

int sgk_normalise_f32(const float *x, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads, uint32_t max_read_len,
                      uint64_t n_values, int method, float *y, sgk_norm_rec_t *rec, void *ws, size_t ws_bytes, void *stream) {
    if (!norm_method_ok(method)) return SGK_ERR_ARG;
    SGK_TRY(float_batch_check(x, offsets, lengths, n_reads, max_read_len));
    if (n_reads == 0) return SGK_OK;
    if (!y || !rec || !ws || (reinterpret_cast<uintptr_t>(y) & 3u) || (reinterpret_cast<uintptr_t>(ws) & 15u)) return SGK_ERR_ARG;
    if (y != x && y < x + n_values && x < y + n_values) return SGK_ERR_ARG;  // in place or apart
    if (ws_bytes < normf_ws(n_reads, n_values, max_read_len)) return SGK_ERR_WORKSPACE;
    if (sgk_device_count() <= 0) return SGK_ERR_NODEVICE;
    return launch_normf(FloatBatch{x, offsets, lengths, n_reads, nullptr}, max_read_len, n_values, method, y, rec, ws,
                        static_cast<hipStream_t>(stream));
}

// x is sgk_pa of the batch: written into y, then normalised there in place
int sgk_normalise(const sgk_batch_t *batch, int method, float *y, sgk_norm_rec_t *rec, void *ws, size_t ws_bytes, void *stream) {
    if (!norm_method_ok(method)) return SGK_ERR_ARG;
    SGK_TRY(check_batch(batch));
    if (batch->n_reads == 0) return SGK_OK;
    if (!y || !rec || !ws || (reinterpret_cast<uintptr_t>(y) & 3u) || (reinterpret_cast<uintptr_t>(ws) & 15u)) return SGK_ERR_ARG;
    if (batch->max_read_len >= 0x80000000u) return SGK_ERR_ARG;
    if (ws_bytes < normf_ws(batch->n_reads, batch->n_samples, batch->max_read_len)) return SGK_ERR_WORKSPACE;
    if (sgk_device_count() <= 0) return SGK_ERR_NODEVICE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    SGK_TRY(launch_pa(batch, y, st));
    return launch_normf(FloatBatch{y, batch->offsets, batch->lengths, batch->n_reads, nullptr}, batch->max_read_len, batch->n_samples,
                        method, y, rec, ws, st);
}

}  // extern "C"
