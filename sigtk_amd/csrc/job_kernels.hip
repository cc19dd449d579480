// job_kernels.hip -- the small kernels of the job runtime: dense layout of per-read counts (k_layout) and the gathers of
// capacity-sized arenas into that layout (k_gather, k_gather_events), behind the launchers of job_launch.h.
#include "job_launch.h"

extern "C" {   // (the kernels keep the plain names they have had in every profile)

// offs[r] = running sum of counts[0..r) with every count rounded up to `align` (a power of two); offs[n] = total.
// One 1024-thread workgroup: a contiguous slice of reads per thread, block scan of the slice sums in LDS.
// With `slots` (capacity arena, n+1 entries) a count is first clamped to its read's capacity.
__device__ inline uint64_t layout_item(const uint32_t *counts, const uint64_t *slots, uint32_t r, uint64_t m) {
    uint64_t c = counts[r];
    if (slots) {
        const uint64_t cap = slots[r + 1] - slots[r];
        c = c < cap ? c : cap;
    }
    return (c + m) & ~m;
}
__global__ __launch_bounds__(1024) void k_layout(const uint32_t *counts, const uint64_t *slots, uint32_t n, uint32_t align,
                                                 uint64_t *offs) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n + 1023u) / 1024u;
    const uint32_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    const uint64_t m = (uint64_t)align - 1;
    uint64_t sum = 0;
    for (uint32_t r = lo; r < hi; ++r) sum += layout_item(counts, slots, r, m);
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint64_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint64_t o = part[t] - sum;
    for (uint32_t r = lo; r < hi; ++r) {
        offs[r] = o;
        o += layout_item(counts, slots, r, m);
    }
    if (t == 1023) offs[n] = part[1023];
}

// items of read r: src[k][slots[r] .. +counts[r]) -> dst[k][doffs[r] ..), k < narr (4-byte items)
__global__ __launch_bounds__(256) void k_gather(sgk::GatherArgs g, int narr, const uint64_t *slots, const uint32_t *counts,
                                                const uint64_t *doffs) {
    const uint32_t r = blockIdx.x;
    const uint64_t s = slots[r], d = doffs[r], cap = slots[r + 1] - s;
    const uint32_t c = counts[r] < cap ? counts[r] : (uint32_t)cap;  // an overflowing read keeps what fitted
    for (int k = 0; k < narr; ++k)
        for (uint32_t i = threadIdx.x; i < c; i += 256) g.dst[k][d + i] = g.src[k][s + i];
}

// events of read r: records src[slots[r] .. +counts[r]) -> the four dense arrays dst[k][doffs[r] ..), k < narr
// (start, length, mean, stdv as 4-byte items; narr = 2 for SGK_JOB_EVENTS_COMPACT; narr = 1: the lengths alone)
__global__ __launch_bounds__(256) void k_gather_events(const sgk_event_rec_t *src, sgk::GatherArgs g, int narr,
                                                       const uint64_t *slots, const uint32_t *counts,
                                                       const uint64_t *doffs) {
    const uint32_t r = blockIdx.x;
    const uint64_t s = slots[r], d = doffs[r], cap = slots[r + 1] - s;
    const uint32_t c = counts[r] < cap ? counts[r] : (uint32_t)cap;  // an overflowing read keeps what fitted
    for (uint32_t i = threadIdx.x; i < c; i += 256) {
        const uint4 v = *reinterpret_cast<const uint4 *>(src + s + i);
        if (narr == 1) {
            g.dst[0][d + i] = v.y;
            continue;
        }
        g.dst[0][d + i] = v.x;
        g.dst[1][d + i] = v.y;
        if (narr > 2) {
            g.dst[2][d + i] = v.z;
            g.dst[3][d + i] = v.w;
        }
    }
}

}  // extern "C"

namespace sgk {

int launch_layout(const uint32_t *counts, const uint64_t *slots_or_null, uint32_t n, uint32_t align, uint64_t *offs, hipStream_t st) {
    SGK_LAUNCH_UNTIMED(k_layout, 1, 1024, st, counts, slots_or_null, n, align, offs);
    return SGK_OK;
}
int launch_gather(const GatherArgs &g, int narr, const uint64_t *slots, const uint32_t *counts, const uint64_t *doffs,
                  uint32_t n_reads, hipStream_t st) {
    SGK_LAUNCH_UNTIMED(k_gather, n_reads, 256, st, g, narr, slots, counts, doffs);
    return SGK_OK;
}
int launch_gather_events(const sgk_event_rec_t *src, const GatherArgs &g, int narr, const uint64_t *slots,
                         const uint32_t *counts, const uint64_t *doffs, uint32_t n_reads, hipStream_t st) {
    SGK_LAUNCH_UNTIMED(k_gather_events, n_reads, 256, st, src, g, narr, slots, counts, doffs);
    return SGK_OK;
}

}  // namespace sgk
