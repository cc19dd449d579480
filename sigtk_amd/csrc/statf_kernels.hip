// statf_kernels.hip -- sgk_stat_f32: meanf / stdvf / medianf (src/stat.h:17-27, 36-44, 56-63) of every read of a float
// batch, bit for bit; sgk_meanf / sgk_stdvf / sgk_medianf (shims.hip) are a batch of one read on the same two kernels:
//   * k_statf_wave, one WAVE per read (float_reads.h), three sweeps over the read's values:
//       1. the sequential sum (seqsum.h)               + the counts of the keys' top 11 bits + "not finite" / "a NaN"
//       2. the sequential sum of squared deviations    + the counts of the next 11 bits among the keys that matched
//       3.                                               the counts of the last 10 bits
//     The order statistic of rank n / 2 is found level by level from a 2 048-bin histogram of the values' keys in the
//     wave's 8 KB of LDS (statf_radix.h, shared with k_normf_wave).
//   * k_statf_literal behind it (the scheme of k_median_literal, stat_literal.hip) looks at every record once and redoes
//     the hostile ones by one lane: a median that is a zero, or of an array holding a NaN, with the reference's own
//     selection on a scratch row of the workspace (median_literal.h); mean and deviation of an array holding a NaN or an
//     infinity with x86's NaN rules (x86_mean_std).  Between the two kernels the record's `flags` carries what is to do.
// A read is never split over workgroups (float_reads.h).
#include "median_literal.h"
#include "statf_radix.h"

namespace sgk {

constexpr uint32_t SF_NONFINITE = 1u, SF_PICK = 2u;  // sgk_statf_rec_t::flags between the two kernels
static_assert((SF_NONFINITE | SF_PICK) < SGK_MEDIAN_INEXACT, "the flag a record keeps");

__global__ __launch_bounds__(256) void k_statf_wave(FloatBatch b, sgk_statf_rec_t *out) {
    __shared__ __attribute__((aligned(16))) uint32_t hist_all[4][SF_BINS];
    uint32_t r;
    if (!float_wave_read(b, r)) return;  // (no workgroup barrier anywhere in this kernel)
    uint32_t *hist = hist_all[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
    FloatRead fr;
    fr.init(b, r);
    const int n = fr.n;
    if (n == 0) {  // 0 / 0 and a selection from nothing
        if (lane_id() == 0) out[r] = sgk_statf_rec_t{__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), 0u};
        return;
    }
    uint32_t rank = (uint32_t)(n / 2), hostile = 0u;
    const auto same = [](float v) { return v; };  // the keys are those of the values themselves
    statf_clear(hist);
    const float s = fr_chain(fr, [](float v) { return v; }, [&](int, const float (&x)[SS_SPL], uint32_t vm) {
#pragma unroll
        for (int e = 0; e < SS_SPL; ++e)
            if (((vm >> e) & 1u) && !(fabsf(x[e]) < __builtin_inff())) hostile |= x[e] != x[e] ? (SF_NONFINITE | SF_PICK) : SF_NONFINITE;
        statf_count(x, vm, 0u, 0u, 21, 0x7ffu, hist, same);
    });
    const float mn = s / n;
    uint32_t prefix = statf_pick(hist, rank) << 21;
    statf_clear(hist);
    const float q = fr_chain(fr, [&](float v) { return (v - mn) * (v - mn); }, [&](int, const float (&x)[SS_SPL], uint32_t vm) {
        statf_count(x, vm, 0xffe00000u, prefix, 10, 0x7ffu, hist, same);
    });
    prefix |= statf_pick(hist, rank) << 10;
    statf_clear(hist);
    fr_sweep(fr, [&](int, const float (&x)[SS_SPL], uint32_t vm) { statf_count(x, vm, 0xfffffc00u, prefix, 0, 0x3ffu, hist, same); });
    prefix |= statf_pick(hist, rank);
    const float med = statf_unkey(prefix);
    hostile = __ballot(hostile & SF_NONFINITE) ? SF_NONFINITE | (__ballot(hostile & SF_PICK) ? SF_PICK : 0u) : 0u;
    if (med == 0.0f) hostile |= SF_PICK;  // +0 and -0 compare equal: the reference's pick
    if (lane_id() == 0) out[r] = sgk_statf_rec_t{mn, sqrtf(q / n), med, hostile};
}

// (one wave per workgroup, a scratch row per workgroup; the reads are dealt round robin, as in k_median_literal)
__global__ __launch_bounds__(64) void k_statf_literal(FloatBatch b, sgk_statf_rec_t *out, float *scratch, uint32_t stride) {
    const int lane = lane_id();
    float *s = scratch ? scratch + (size_t)blockIdx.x * stride : nullptr;
    for (uint64_t r0 = blockIdx.x; r0 < b.n_reads; r0 += 64ull * gridDim.x) {
        const uint64_t r64 = r0 + (uint64_t)lane * gridDim.x;
        const uint32_t fl = r64 < b.n_reads ? out[r64].flags : 0u;
        unsigned long long todo = __ballot((fl & (SF_NONFINITE | SF_PICK)) != 0u);
        while (todo) {  // (wave-uniform)
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const uint32_t rr = (uint32_t)(r0 + (uint64_t)l * gridDim.x);
            const uint32_t f = (uint32_t)__shfl((int)fl, l, 64);
            const float *x = b.x + b.offsets[rr];
            const int64_t len = (int64_t)b.lengths[rr];
            uint32_t keep = 0u;
            if ((f & SF_NONFINITE) && lane == 0) x86_mean_std(len, [&](int64_t i) { return x[i]; }, out[rr].mean, out[rr].std);
            if (f & SF_PICK) {
                if (!s || len > (int64_t)stride) keep = SGK_MEDIAN_INEXACT;  // no room to redo it: the record says so
                else {
                    for (int64_t i = lane; i < len; i += 64) s[i] = x[i];
                    __syncthreads();
                    if (lane == 0) out[rr].median = literal_select(s, len, len / 2, [](float p, float q) { return p < q; });
                    __syncthreads();
                }
            }
            if (lane == 0) out[rr].flags = keep;
        }
    }
}

// ---- the workspace: [0, 64) unused counters, the dispatch order, the scratch rows of k_statf_literal (literal_rows,
// stat_args.h), each with room for the batch's longest read
static uint32_t statf_stride(uint32_t max_read_len) { return (max_read_len + 3u) & ~3u; }
static size_t statf_rows(uint32_t n_reads, uint32_t max_read_len) {
    return literal_rows(n_reads, (size_t)statf_stride(max_read_len) * sizeof(float));
}
static size_t statf_ws(uint32_t n_reads, uint32_t max_read_len) {
    return order_workspace_bytes(n_reads) + statf_rows(n_reads, max_read_len) * statf_stride(max_read_len) * sizeof(float);
}

int float_batch_check(const float *x, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads, uint32_t max_read_len) {
    if (n_reads == 0) return SGK_OK;
    if (!x || !offsets || !lengths || (reinterpret_cast<uintptr_t>(x) & 3u)) return SGK_ERR_ARG;
    if (max_read_len >= 0x80000000u) return SGK_ERR_ARG;  // the reference's n is an int
    return SGK_OK;
}
// the dispatch order of a float batch in the workspace at ws + 64 (batches of ORDER_MIN_READS reads or more)
int float_batch_order(FloatBatch &b, void *ws, hipStream_t st) {
    b.order = nullptr;
    if (b.n_reads < ORDER_MIN_READS) return SGK_OK;
    uint32_t *order = reinterpret_cast<uint32_t *>(static_cast<char *>(ws) + 64), *hist = order + b.n_reads;
    SGK_TRY(launch_order(b.lengths, b.n_reads, order, hist, st));
    b.order = order;
    return SGK_OK;
}

int launch_statf_ordered(const FloatBatch &b, uint32_t max_read_len, sgk_statf_rec_t *out, void *ws, hipStream_t st) {
    SGK_LAUNCH("k_statf_wave", k_statf_wave, (b.n_reads + 3) / 4, 256, st, b, out);
    float *scratch = reinterpret_cast<float *>(static_cast<char *>(ws) + order_workspace_bytes(b.n_reads));
    SGK_LAUNCH("k_statf_literal", k_statf_literal, (uint32_t)statf_rows(b.n_reads, max_read_len), 64, st, b, out, scratch,
               statf_stride(max_read_len));
    return SGK_OK;
}
int launch_statf(FloatBatch b, uint32_t max_read_len, sgk_statf_rec_t *out, void *ws, hipStream_t st) {
    SGK_TRY(float_batch_order(b, ws, st));
    return launch_statf_ordered(b, max_read_len, out, ws, st);
}

}  // namespace sgk

using namespace sgk;

extern "C" {

size_t sgk_stat_f32_workspace_bytes(uint32_t n_reads, uint64_t n_values, uint32_t max_read_len) {
    (void)n_values;
    return statf_ws(n_reads, max_read_len);
}

int sgk_stat_f32(const float *x, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads, uint32_t max_read_len,
                 uint64_t n_values, sgk_statf_rec_t *out, void *ws, size_t ws_bytes, void *stream) {
    (void)n_values;
    SGK_TRY(float_batch_check(x, offsets, lengths, n_reads, max_read_len));
    if (n_reads == 0) return SGK_OK;
    if (!out || !ws || (reinterpret_cast<uintptr_t>(ws) & 15u)) return SGK_ERR_ARG;
    if (ws_bytes < statf_ws(n_reads, max_read_len)) return SGK_ERR_WORKSPACE;
    if (sgk_device_count() <= 0) return SGK_ERR_NODEVICE;
    return launch_statf(FloatBatch{x, offsets, lengths, n_reads, nullptr}, max_read_len, out, ws, static_cast<hipStream_t>(stream));
}

}  // extern "C"
