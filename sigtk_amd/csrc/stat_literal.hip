// stat_literal.hip -- k_median_literal: the pA medians that are a PICK among equal-comparing or unordered values (a zero,
// or a unit / offset that is not finite: median_literal.h) redone with the reference's own selection.  It runs behind
// the kernels that wrote the medians (stat_launch.hip), looks at every record once -- 64 per wavefront, one compare on
// the median and two on the scale -- and redoes what it finds, one lane per read, on a scratch copy of the region's int16
// samples in the workspace: ordinary reads pay that one look.  What one lane costs: profiles/median_literal.md.
// The same lane redoes the pA mean and deviation of a read whose unit or offset is not finite, for the sign of their NaN
// (median_literal.h: x86_mean_std); that needs no scratch.
#include "median_literal.h"
#include "stat_device.h"

namespace sgk {

template <int MODE>
__global__ __launch_bounds__(64) void k_median_literal(StatArgs a) {
    const int lane = lane_id();
    int16_t *s = a.lit_scratch ? a.lit_scratch + (size_t)blockIdx.x * a.lit_stride : nullptr;
    constexpr uint32_t inexact = MODE == REG_POLYA ? FLAG_MEDIAN_INEXACT_POLYA : FLAG_MEDIAN_INEXACT;
    // the reads are dealt round robin: workgroup b looks at reads b, b + B, b + 2 B ..., 64 of them at a time, so that a
    // batch in which every read is to be redone keeps every workgroup busy
    for (uint64_t r0 = blockIdx.x; r0 < a.b.n_reads; r0 += 64ull * gridDim.x) {
        const uint64_t r64 = r0 + (uint64_t)lane * gridDim.x;
        const uint32_t r = r64 < a.b.n_reads ? (uint32_t)r64 : a.b.n_reads;
        Region g = {0, 0};
        Scale sc = {0.0f, 1.0f};
        bool pick = false, sums = false;
        if (r < a.b.n_reads) {
            g = get_region(MODE, a.b, a.prefix, r);
            sc = make_scale(a.b.digitisation[r], a.b.offset[r], a.b.range[r]);
            const float pm = MODE == REG_WHOLE ? a.stat[r].pa_median : (MODE == REG_ADAPT ? a.prefix[r].adapt_median : a.prefix[r].polya_median);
            pick = g.len >= 1 && median_is_a_pick(pm, sc);
            sums = g.len >= 1 && !scale_is_finite(sc);
        }
        const unsigned long long picks = __ballot(pick);
        unsigned long long todo = picks | __ballot(sums);
        while (todo) {  // (wave-uniform)
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const uint32_t rr = (uint32_t)(r0 + (uint64_t)l * gridDim.x);
            const int64_t start = (int64_t)__shfl((long long)g.start, l, 64), len = (int64_t)__shfl((long long)g.len, l, 64);
            const Scale q = {__shfl(sc.offf, l, 64), __shfl(sc.unit, l, 64)};
            if (lane == 0 && !scale_is_finite(q)) {
                float mean, sd;
                const int16_t *x = a.b.samples + start;
                x86_mean_std(len, [&](int64_t i) { return x86_to_pa(x[i], q); }, mean, sd);
                if (MODE == REG_WHOLE) { a.stat[rr].pa_mean = mean; a.stat[rr].pa_std = sd; }
                else if (MODE == REG_ADAPT) { a.prefix[rr].adapt_mean = mean; a.prefix[rr].adapt_std = sd; }
                else { a.prefix[rr].polya_mean = mean; a.prefix[rr].polya_std = sd; }
            }
            if (!((picks >> l) & 1ull)) continue;
            if (!s || len > (int64_t)a.lit_stride) {  // no room to redo it: the record says so
                if (lane == 0) {
                    if (MODE == REG_WHOLE) a.stat[rr].reserved |= inexact;
                    else a.prefix[rr].reserved |= inexact;
                    if (a.lit_hdr) atomicAdd(&a.lit_hdr->n_inexact, 1u);
                }
                continue;
            }
            for (int64_t i = lane; i < len; i += 64) s[i] = a.b.samples[start + i];
            __syncthreads();
            if (lane == 0) {
                const int16_t v = literal_select(s, len, len / 2, [&](int16_t x, int16_t y) { return to_pa(x, q) < to_pa(y, q); });
                const float pm = x86_to_pa(v, q);
                if (MODE == REG_WHOLE) a.stat[rr].pa_median = pm;
                else if (MODE == REG_ADAPT) a.prefix[rr].adapt_median = pm;
                else a.prefix[rr].polya_median = pm;
                if (a.lit_hdr) atomicAdd(&a.lit_hdr->n_literal, 1u);
            }
            __syncthreads();
        }
    }
}

// a workgroup per scratch row (literal_rows, stat_args.h), each row with room for the batch's longest read
static uint32_t literal_stride(uint32_t max_read_len) { return (max_read_len + 7u) & ~7u; }
size_t literal_workspace_bytes(uint32_t n_reads, uint32_t max_read_len) {
    const size_t per = (size_t)literal_stride(max_read_len) * sizeof(int16_t);
    return literal_rows(n_reads, per) * per;
}
void prepare_literal(StatArgs &a, void *ws, size_t ws_bytes) {
    a.lit_hdr = nullptr;
    a.lit_scratch = nullptr;
    a.lit_stride = 0u;
    a.lit_blocks = 0u;
    const size_t off = order_workspace_bytes(a.b.n_reads);
    // (the header prepare_long clears for every call whose workspace holds one)
    if (!ws || ws_bytes < off + long_workspace_bytes(0, 0) || (reinterpret_cast<uintptr_t>(ws) & 7u)) return;
    a.lit_hdr = reinterpret_cast<LongHdr *>(static_cast<char *>(ws) + off);
    const size_t soff = off + long_workspace_bytes(a.b.n_samples, a.b.max_read_len);
    const size_t per = (size_t)literal_stride(a.b.max_read_len) * sizeof(int16_t);
    if (per == 0 || ws_bytes < soff + per) return;
    a.lit_blocks = (uint32_t)literal_rows(a.b.n_reads, per, ws_bytes - soff);   // (a workspace with room for fewer: fewer workgroups)
    a.lit_stride = literal_stride(a.b.max_read_len);
    a.lit_scratch = reinterpret_cast<int16_t *>(static_cast<char *>(ws) + soff);
}
int launch_k_median_literal(const char *name, int region, hipStream_t st, const StatArgs &a) {
    // (without scratch the kernel only marks what it cannot redo)
    const uint32_t grid = a.lit_scratch ? a.lit_blocks : (a.b.n_reads < LIT_BLOCKS ? a.b.n_reads : LIT_BLOCKS);
    if (grid == 0) return SGK_OK;
    if (region == REG_WHOLE) SGK_LAUNCH(name, (k_median_literal<REG_WHOLE>), grid, 64, st, a);
    else if (region == REG_ADAPT) SGK_LAUNCH(name, (k_median_literal<REG_ADAPT>), grid, 64, st, a);
    else if (region == REG_POLYA) SGK_LAUNCH(name, (k_median_literal<REG_POLYA>), grid, 64, st, a);
    else return SGK_ERR_ARG;
    return SGK_OK;
}

}  // namespace sgk
