// float_reads.h -- a batch of float (pA) reads on the device, one WAVE per read: what sgk_stat_f32 (statf_kernels.hip) and
// sgk_jnn_f32 (jnnf_kernels.hip) share.  sgk_meanf / sgk_stdvf / sgk_medianf (shims.hip) are a batch of one read on
// launch_statf; sgk_jnn_pa keeps a single-array kernel of its own (shims.hip says why).
//
// A float batch is x, offsets, lengths: read r is x[offsets[r] .. offsets[r] + lengths[r]); x is 4-byte aligned and an
// offset is any element index.  The wave works in q space: q = i + skip, where skip (0 .. 3) is the number of elements
// between the 16-byte boundary at or below the read's first value and that value.  A tile is 64 x SS_SPL positions, lane l
// owns positions 16 l .. 16 l + 15 of it (the layout seqsum.h asks for) as four groups of four: a group that lies inside
// the read is one 16-byte load, a group that straddles an end of the read is loaded value by value, each behind its own
// test, and a group outside the read is not loaded at all.  So no byte outside the read -- let alone outside
// [x, x + n_values) -- is touched, whatever the residue of the offset, and what a read's neighbours or the gaps hold
// cannot matter.  Positions outside the read hold 0 and are masked by `vm` wherever a 0 could be seen.
//
// A read is never split over wavefronts: a read of 10^6 values takes one wavefront a thousand tiles per pass -- slow and
// right, like k_adaptor_param.  Float input does not go through k_long_chains.
#pragma once
#include "seqsum.h"
#include "stat_device.h"

namespace sgk {

struct FloatBatch {  // the device pointers of a float batch (kernel argument)
    const float *x;
    const uint64_t *offsets;
    const uint32_t *lengths;
    uint32_t n_reads;
    const uint32_t *order;  // wave i takes read order[i] (longest first), or null
};

struct FloatRead {  // wave-uniform
    const float *xb;  // the 16-byte boundary at or below the read's first value (never dereferenced below `skip`)
    int skip, n, ntiles;
    int64_t nq;       // skip + n
    __device__ __forceinline__ void init(const FloatBatch &b, uint32_t r) {
        const float *p = b.x + b.offsets[r];
        skip = (int)((reinterpret_cast<uintptr_t>(p) & 15u) >> 2);
        xb = p - skip;
        n = (int)b.lengths[r];
        nq = (int64_t)skip + n;
        ntiles = (int)((nq + SS_TILE - 1) / SS_TILE);
    }
    // bit e: position 16 lane + e of tile t is a value of the read
    __device__ __forceinline__ uint32_t valid16(int t) const {
        const int64_t q = (int64_t)t * SS_TILE + lane_id() * SS_SPL;
        const int64_t a0 = skip - q, a1 = nq - q;
        const int lo = a0 < 0 ? 0 : (a0 > SS_SPL ? SS_SPL : (int)a0), hi = a1 > SS_SPL ? SS_SPL : (a1 < 0 ? 0 : (int)a1);
        return lo >= hi ? 0u : ((0xffffu >> lo) << lo) & ((1u << hi) - 1u);
    }
    // this lane's 16 positions of tile t
    __device__ __forceinline__ void load(float (&v)[SS_SPL], int t) const {
        const int64_t q0 = (int64_t)t * SS_TILE + lane_id() * SS_SPL;
#pragma unroll
        for (int g = 0; g < SS_SPL / 4; ++g) {
            const int64_t q = q0 + 4 * g;
            if (q >= skip && q + 4 <= nq) {
                const float4 u = *static_cast<const float4 *>(__builtin_assume_aligned(xb + q, 16));
                v[4 * g] = u.x; v[4 * g + 1] = u.y; v[4 * g + 2] = u.z; v[4 * g + 3] = u.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[4 * g + k] = (q + k >= skip && q + k < nq) ? xb[q + k] : 0.0f;
            }
        }
    }
    // load's mirror: this lane's 16 positions of tile t into an array of x's layout.  yq + q is where position q goes (the
    // read's first value at yq + skip); `aligned`: yq is a 16-byte boundary, as xb is.  A group inside the read is one
    // 16-byte store, a group that straddles an end of the read is stored value by value, each behind its own test, and a
    // group outside the read is not stored at all: no byte outside the read is written -- not a gap, not a neighbour, not
    // the slack in front of an unaligned first value.  An array whose 16-byte phase differs from x's is stored value by
    // value throughout.
    __device__ __forceinline__ void store(float *yq, bool aligned, const float (&v)[SS_SPL], int t) const {
        const int64_t q0 = (int64_t)t * SS_TILE + lane_id() * SS_SPL;
#pragma unroll
        for (int g = 0; g < SS_SPL / 4; ++g) {
            const int64_t q = q0 + 4 * g;
            if (aligned && q >= skip && q + 4 <= nq) {
                *static_cast<float4 *>(__builtin_assume_aligned(yq + q, 16)) = float4{v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]};
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (q + k >= skip && q + k < nq) yq[q + k] = v[4 * g + k];
            }
        }
    }
};

// host side (statf_kernels.hip): the argument checks both entry points share, and the dispatch order of a batch of
// ORDER_MIN_READS reads or more, sorted into the workspace at ws + 64 (order_workspace_bytes)
int float_batch_check(const float *x, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads, uint32_t max_read_len);
int float_batch_order(FloatBatch &b, void *ws, hipStream_t st);
// What sgk_stat_f32 launches once its arguments are checked (b.order is the launcher's to fill; ws: 16-byte aligned, of
// the size sgk_stat_f32_workspace_bytes gives).  The float stat shims call it directly.
int launch_statf(FloatBatch b, uint32_t max_read_len, sgk_statf_rec_t *out, void *ws, hipStream_t st);
// ... for a batch whose b.order the caller has filled with float_batch_order on the same workspace (sgk_normalise_f32)
int launch_statf_ordered(const FloatBatch &b, uint32_t max_read_len, sgk_statf_rec_t *out, void *ws, hipStream_t st);

// the read a wave takes: four waves per workgroup, longest reads first where the batch has a dispatch order
__device__ __forceinline__ bool float_wave_read(const FloatBatch &b, uint32_t &r) {
    const uint32_t widx = blockIdx.x * 4 + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (widx >= b.n_reads) return false;
    r = b.order ? b.order[widx] : widx;
    return true;
}

// one sweep over the read: f(t, v, vm) per tile, with tile t + 1 in flight under it
template <typename F>
__device__ __forceinline__ void fr_sweep(const FloatRead &fr, F f) {
    float cur[SS_SPL], nxt[SS_SPL];
    if (fr.ntiles > 0) fr.load(cur, 0);
#pragma unroll 1
    for (int t = 0; t < fr.ntiles; ++t) {
        if (t + 1 < fr.ntiles) fr.load(nxt, t + 1);
        f(t, cur, fr.valid16(t));
#pragma unroll
        for (int e = 0; e < SS_SPL; ++e) cur[e] = nxt[e];
    }
}

// One sequential float sum of the reference over the read: term(x[i]) for i = 0 .. n - 1 in sample order (seqsum.h, on
// tiles that start at a 16-byte boundary).  Terms can have any sign: the chain is oriented by the sign of its
// accumulator, tiles holding a term of the other sign, a NaN or an infinity are added natively.  side(t, v, vm) sees
// every tile's values first (histograms, flags).
template <typename TERM, typename SIDE>
__device__ inline float fr_chain(const FloatRead &fr, TERM term, SIDE side) {
    const int q0 = lane_id() * SS_SPL;
    float m = 0.0f, sg = 1.0f;
    const int hq = fr.skip + (fr.n < SS_HEAD ? fr.n : SS_HEAD);  // the head: positions skip .. hq - 1 of tile 0
    fr_sweep(fr, [&](int t, const float (&x)[SS_SPL], uint32_t vm) {
        side(t, x, vm);
        float v[SS_SPL], y[SS_SPL];
#pragma unroll
        for (int e = 0; e < SS_SPL; ++e) v[e] = ((vm >> e) & 1u) ? term(x[e]) * sg : 0.0f;  // (* +-1: exact)
        if (t == 0) {  // the head natively; its terms are zeroed for the tile chain
#pragma unroll
            for (int e = 0; e < SS_SPL; ++e) y[e] = (q0 + e < hq) ? v[e] : 0.0f;
            if (hq > fr.skip) m = ss_serial(m, TermArr{y}, 0, (hq - 1) / SS_SPL);
#pragma unroll
            for (int e = 0; e < SS_SPL; ++e) v[e] = (q0 + e < hq) ? 0.0f : v[e];
        }
        const SsWalk w = ss_walk<true>(m, TermArr{v});
        int sk;
        if (ss_fast<true>(m, w, TermArr{v}, sk)) m = ss_finish<true>(m, TermArr{v}, w, sk);
        if (m < 0.0f) { m = -m; sg = -sg; }
    });
    return m == 0.0f ? 0.0f : m * sg;
}

}  // namespace sgk
