// statf_radix.h -- the order statistic of a float read by a three-level radix over the values' keys (11 + 11 + 10 bits) in
// a wave's 2 048-bin LDS histogram: what k_statf_wave (statf_kernels.hip, the median of x) and k_normf_wave
// (normf_kernels.hip, the median of |x - median|) share.  The key of a float is its order-preserving integer image.  A
// lane counts runs of equal bins among its 16 consecutive values and adds a run at a time: a nanopore read keeps to a few
// of the top-level bins, and 1 024 atomics on three LDS words per tile would otherwise cost more than the tile's HBM
// traffic.  Everything here is wave-local: fences and wave barriers, no workgroup barrier.
#pragma once
#include "float_reads.h"

namespace sgk {

constexpr int SF_BINS = 2048;

__device__ __forceinline__ uint32_t statf_key(float f) {  // a < b  <=>  key(a) < key(b) (zeros: -0 below +0)
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float statf_unkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// this lane's values whose key matches `prefix` on the bits `known` into hist[(key >> shift) & mask], a run at a time;
// the key is that of tf(x[e])
template <typename TF>
__device__ __forceinline__ void statf_count(const float (&x)[SS_SPL], uint32_t vm, uint32_t known, uint32_t prefix, int shift,
                                            uint32_t mask, uint32_t *hist, TF tf) {
    uint32_t cb = 0u, cc = 0u;
#pragma unroll
    for (int e = 0; e < SS_SPL; ++e) {
        const uint32_t k = statf_key(tf(x[e]));
        if (((vm >> e) & 1u) && (k & known) == prefix) {
            const uint32_t b = (k >> shift) & mask;
            if (cc && b != cb) { atomicAdd(&hist[cb], cc); cc = 0u; }
            cb = b;
            ++cc;
        }
    }
    if (cc) atomicAdd(&hist[cb], cc);
}
__device__ __forceinline__ void statf_clear(uint32_t *hist) {
#pragma unroll
    for (int i = 0; i < SF_BINS / 64; ++i) hist[i * 64 + lane_id()] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// the bin that holds rank `rank` of the complete histogram (wave-uniform); rank becomes the rank inside that bin
__device__ inline uint32_t statf_pick(const uint32_t *hist, uint32_t &rank) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int lane = lane_id();
    constexpr int PER = SF_BINS / 64;
    uint32_t cnt[PER], lsum = 0u;
#pragma unroll
    for (int i = 0; i < PER; ++i) { cnt[i] = hist[lane * PER + i]; lsum += cnt[i]; }
    const uint32_t incl = (uint32_t)wave_incl_scan_i((int)lsum), excl = incl - lsum;
    const bool mine = rank >= excl && rank < incl;
    uint32_t bin = 0u, below = 0u;
    if (mine) {
        uint32_t acc = excl;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            if (rank >= acc && rank < acc + cnt[i]) { bin = (uint32_t)(lane * PER + i); below = acc; }
            acc += cnt[i];
        }
    }
    const unsigned long long own = __ballot(mine);
    const int l = own ? __builtin_amdgcn_readfirstlane(__ffsll((long long)own) - 1) : 0;
    rank -= (uint32_t)__builtin_amdgcn_readlane((int)below, l);
    return (uint32_t)__builtin_amdgcn_readlane((int)bin, l);
}

}  // namespace sgk
