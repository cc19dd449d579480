// sigraw_kernels.hip -- k_sigraw_gather: the plain int16 signal of inflated BLOW5 records moved into the sample arena
// (sgk_sigraw_gather).
//
// A BLOW5 record whose signal is not compressed (signal_press 0: every file older than svb-zd, every `-s none` file)
// holds its samples as they are, little-endian int16, behind a head of 2 + id_len + 44 bytes (slow5lib/src/slow5.c:
// 2918-2935).  The record was inflated to a 16-byte aligned place, so the samples start at whatever byte the read id's
// length leaves them at: any residue of 16, the odd ones included.  The arena wants every read on a 16-byte boundary.
//
// The move is a byte-shifted copy.  Work is dealt out in units of SR_UNIT samples: workgroup (r, u) takes units u,
// u + gx, u + 2 gx, ... of read r, every thread SR_WPT 16-byte words of a unit.  A word of the destination is bytes
// [R, R + 16) of two neighbouring aligned words of the source, R the residue -- uniform over the read, so it is kept in
// an SGPR: its dword part picks the registers (a uniform branch over four straight-line bodies), its byte part is the
// shift of v_alignbyte_b32.  Both source words are loaded by the thread that needs them; the second is the first of the
// thread next to it and comes out of the cache.  No LDS, no shuffles; all loads of a unit are issued before its first
// store.  With R = 0 the second load is not made.
//
// Only aligned 16-byte words are loaded, and only words that hold a byte of the signal: the word behind the last one is
// touched when the read's last bytes lie in it, never otherwise.  Stores are whole 16-byte words except the read's last
// one when the length is no multiple of 8: that one goes out sample by sample, so that not one sample behind the read is
// written.
#include "sgk_common.h"

namespace sgk {

constexpr uint32_t SR_BLOCK = 256;                   // threads of a workgroup
constexpr uint32_t SR_WPT = 4;                       // 16-byte words per thread and unit
constexpr uint32_t SR_UNIT_WORDS = SR_BLOCK * SR_WPT;
constexpr uint32_t SR_UNIT = SR_UNIT_WORDS * 8;      // samples of a unit

struct SigrawArgs {
    const uint8_t *records;
    const uint64_t *rec_offsets;
    const uint32_t *rec_lengths;
    const uint32_t *sig_offsets;
    const uint32_t *rec_status;   // nullptr, or n_reads words: a record with a non-zero word is not read (status 2)
    int16_t *samples;
    const uint64_t *offsets;
    const uint32_t *lengths;
    uint32_t *status;
    uint32_t n_reads, gx;         // gx workgroups per read
};

// bytes [4 D + s, 4 D + s + 16) of the 32 bytes lo | hi (s < 4)
template <int D>
__device__ inline uint4 sr_shift(const uint4 lo, const uint4 hi, const uint32_t s) {
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return make_uint4(__builtin_amdgcn_alignbyte(w[D + 1], w[D], s), __builtin_amdgcn_alignbyte(w[D + 2], w[D + 1], s),
                      __builtin_amdgcn_alignbyte(w[D + 3], w[D + 2], s), __builtin_amdgcn_alignbyte(w[D + 4], w[D + 3], s));
}

__global__ __launch_bounds__(SR_BLOCK) void k_sigraw_gather(const SigrawArgs a) {
    const uint32_t r = blockIdx.x / a.gx, u0 = blockIdx.x - r * a.gx;
    const uint32_t n = a.lengths[r];
    uint32_t st = 0u;
    if (a.rec_status && a.rec_status[r] != 0u) st = 2u;   // (its length word may be garbage: not looked at)
    else if ((uint64_t)a.sig_offsets[r] + 2ull * n > a.rec_lengths[r]) st = 1u;
    if (u0 == 0u && threadIdx.x == 0u) a.status[r] = st;
    if (st != 0u) return;
    const uint64_t src = a.rec_offsets[r] + a.sig_offsets[r];
    const uint32_t res = __builtin_amdgcn_readfirstlane((uint32_t)src & 15u);
    const uint32_t d = res >> 2, s = res & 3u;
    const uint4 *in = reinterpret_cast<const uint4 *>(a.records) + (src >> 4);
    int16_t *out = a.samples + a.offsets[r];
    const uint32_t nw = n / 8u + ((n & 7u) != 0u);   // words of the destination, the last one perhaps partial
    const uint32_t units = nw / SR_UNIT_WORDS + ((nw % SR_UNIT_WORDS) != 0u);
    for (uint32_t u = u0; u < units; u += a.gx) {
        uint4 lo[SR_WPT], hi[SR_WPT];
        uint32_t left[SR_WPT];   // samples of the read from this word on (0: no such word)
#pragma unroll
        for (uint32_t k = 0; k < SR_WPT; ++k) {
            const uint32_t j = u * SR_UNIT_WORDS + k * SR_BLOCK + threadIdx.x;
            left[k] = j < nw ? n - 8u * j : 0u;
            lo[k] = make_uint4(0u, 0u, 0u, 0u);
            hi[k] = lo[k];
            if (left[k]) lo[k] = in[j];
            // the word behind: when bytes of this destination word lie in it (a partial word may end in front of it)
            if (left[k] && res + 2u * (left[k] < 8u ? left[k] : 8u) > 16u) hi[k] = in[j + 1u];
        }
#pragma unroll
        for (uint32_t k = 0; k < SR_WPT; ++k) {
            const uint32_t j = u * SR_UNIT_WORDS + k * SR_BLOCK + threadIdx.x;
            uint4 v;
            switch (d) {   // uniform
                case 0: v = sr_shift<0>(lo[k], hi[k], s); break;
                case 1: v = sr_shift<1>(lo[k], hi[k], s); break;
                case 2: v = sr_shift<2>(lo[k], hi[k], s); break;
                default: v = sr_shift<3>(lo[k], hi[k], s); break;
            }
            if (left[k] >= 8u) {
                *reinterpret_cast<uint4 *>(out + 8ull * j) = v;
            } else if (left[k]) {   // the read's last word, 1 - 7 samples of it
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (uint32_t i = 0; i < 7u; ++i)
                    if (i < left[k]) out[8ull * j + i] = (int16_t)(uint16_t)(w[i >> 1] >> (16u * (i & 1u)));
            }
        }
    }
}

}  // namespace sgk

extern "C" uint32_t sgk_sigraw_unit_samples(void) { return sgk::SR_UNIT; }

extern "C" int sgk_sigraw_gather(const uint8_t *records, const uint64_t *rec_offsets, const uint32_t *rec_lengths,
                                 const uint32_t *sig_offsets, const uint32_t *rec_status, uint32_t n_reads, int16_t *samples,
                                 const uint64_t *offsets, const uint32_t *lengths, uint32_t max_read_len, uint64_t n_samples,
                                 uint32_t *status, void *stream) {
    using namespace sgk;
    if (n_reads == 0) return SGK_OK;
    if (!records || !rec_offsets || !rec_lengths || !sig_offsets || !samples || !offsets || !lengths || !status) return SGK_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(records) & 15u) || (reinterpret_cast<uintptr_t>(samples) & 15u)) return SGK_ERR_ALIGN;
    // workgroups per read: as many as the longest read has units, but no more than twice what the average read has --
    // one long read among many short ones must not make every short one launch hundreds of workgroups that find nothing
    // to do.  A workgroup strides over its read's units, so any gx >= 1 moves every sample.
    uint64_t gx = ((uint64_t)max_read_len + SR_UNIT - 1u) / SR_UNIT;
    if (n_samples) {
        const uint64_t avg2 = (2u * n_samples + (uint64_t)SR_UNIT * n_reads - 1u) / ((uint64_t)SR_UNIT * n_reads);
        if (avg2 < gx) gx = avg2;
    }
    if (gx < 1u) gx = 1u;
    if (gx * n_reads > 0x7fffffffull) gx = 0x7fffffffull / n_reads;   // (n_reads < 2^32: gx >= 0 ...
    if (gx < 1u) return SGK_ERR_ARG;                                   // ... and 0 only with more than 2^31 reads)
    const SigrawArgs a = {records, rec_offsets, rec_lengths, sig_offsets, rec_status, samples, offsets, lengths, status,
                          n_reads, (uint32_t)gx};
    SGK_LAUNCH("k_sigraw_gather", k_sigraw_gather, (uint32_t)(gx * n_reads), SR_BLOCK, static_cast<hipStream_t>(stream), a);
    return SGK_OK;
}
