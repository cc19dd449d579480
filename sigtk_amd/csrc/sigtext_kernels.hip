// sigtext_kernels.hip -- GPU parse of the raw_signal column of text SLOW5 records.
//
// Format (slow5lib/src/slow5.c:2754-2778, slow5_misc.c:303-319): decimal int16 tokens separated by ','.  The reference walks
// the column with strsep + strtol, one record at a time on its one thread.  Here one wavefront parses one read: per tile
// of 64 lanes x 16 bytes every lane loads one aligned 16-byte word, counts its commas, and a wave scan of the counts
// gives every token its sample index.  A token belongs to the lane that holds its terminator (the ',' behind it, or the
// end of the text, which is treated as one more ','); it is at most 6 bytes long and may have started in the previous
// lane, so every lane also gets the previous lane's upper 8 bytes (one DPP wave shift; lane 0 takes them from the
// previous tile's lane 63, carried in two wave-uniform registers).  The lane then walks its 8 + 16 bytes with a small
// integer automaton and stores a value at every terminator of its own.  Integer arithmetic and vector stores only.
//
// Accepted tokens, and nothing else: 0 | -?[1-9][0-9]{0,4} with the value in [-32768, 32767].
// status: 2 if any token is malformed, else 1 if the number of tokens is not lengths[r], else 0.
// Memory: loads are aligned 16-byte words inside [text_offsets[r] & ~15, round_up(text_offsets[r] + text_lengths[r], 16));
// stores go to sample indices < lengths[r] only, whatever the text holds.
#include "sgk_common.h"

namespace sgk {

constexpr uint32_t SGT_PAD = 0x01010101u;  // bytes outside the text: they end a token's look-back and start nothing

struct SigTextArgs {
    const uint8_t *text;
    const uint64_t *text_offsets;  // n_reads
    const uint32_t *text_lengths;  // n_reads (bytes of the column)
    int16_t *samples;
    const uint64_t *offsets;       // n_reads (sample index of each read in `samples`)
    const uint32_t *lengths;       // n_reads (expected sample counts)
    uint32_t *status;              // n_reads: 0 ok, 1 token count mismatch, 2 malformed token
    uint32_t n_reads;
};

// 0x80 in every byte of w that equals c (exact: no carries between bytes)
__device__ inline uint32_t bytes_eq(uint32_t w, uint32_t c4) {
    const uint32_t x = w ^ c4;
    const uint32_t t = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;
    return ~(t | x | 0x7f7f7f7fu);
}

// the bytes of word w at stream position p .. p + 3 that lie outside [lo, hi) become pad bytes; position hi (the end of
// the text) becomes the terminator of the last token
__device__ inline uint32_t clip_word(uint32_t w, uint64_t p, uint64_t lo, uint64_t hi) {
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint64_t q = p + (uint64_t)j;
        uint32_t c = (w >> (8 * j)) & 0xffu;
        if (q < lo || q > hi) c = 0x01u;
        else if (q == hi) c = (uint32_t)',';
        else if (c == 0x01u) c = 0x02u;  // a pad byte's value inside the text is a byte like any other: malformed
        out |= c << (8 * j);
    }
    return out;
}

__global__ __launch_bounds__(64) void k_sigtext_decode(SigTextArgs a) {
    const uint32_t r = blockIdx.x;
    const int l = lane_id();
    const uint32_t tlen = a.text_lengths[r];
    const uint32_t count = a.lengths[r];
    if (tlen == 0) {  // no tokens at all
        if (l == 0) a.status[r] = count == 0 ? 0u : 1u;
        return;
    }
    const uint8_t *t0 = a.text + a.text_offsets[r];
    const uint64_t lead = (uint64_t)(reinterpret_cast<uintptr_t>(t0) & 15u);
    const uint4 *base = reinterpret_cast<const uint4 *>(t0 - lead);  // aligned; stream position p is byte p from here
    const uint64_t end = lead + (uint64_t)tlen;                      // position of the virtual last terminator
    const uint64_t nload = (end + 15u) >> 4;                         // 16-byte words that hold text
    const uint64_t ntiles = (end >> 10) + 1u;                        // tiles up to and including position `end`
    int16_t *out = a.samples + a.offsets[r];
    uint32_t cursor = 0;                    // tokens in front of this tile (wave-uniform)
    uint32_t cz = SGT_PAD, cw = SGT_PAD;    // upper 8 bytes of the previous tile's lane 63 (wave-uniform)
    uint32_t err = 0;
    for (uint64_t t = 0; t < ntiles; ++t) {
        const uint64_t wi = t * 64u + (uint64_t)l;  // this lane's 16-byte word
        const uint64_t p0 = wi << 4;
        uint4 w = make_uint4(SGT_PAD, SGT_PAD, SGT_PAD, SGT_PAD);
        if (wi < nload) w = base[wi];
        if (p0 < lead || p0 + 16u > end) {  // the first word, the last one and what lies behind it
            w.x = clip_word(w.x, p0, lead, end);
            w.y = clip_word(w.y, p0 + 4u, lead, end);
            w.z = clip_word(w.z, p0 + 8u, lead, end);
            w.w = clip_word(w.w, p0 + 12u, lead, end);
        } else if (bytes_eq(w.x, SGT_PAD) | bytes_eq(w.y, SGT_PAD) | bytes_eq(w.z, SGT_PAD) | bytes_eq(w.w, SGT_PAD)) {
            err = 1;  // (see clip_word)
        }
        const uint32_t cc = 0x2c2c2c2cu;
        const int ncomma = __popc(bytes_eq(w.x, cc)) + __popc(bytes_eq(w.y, cc)) + __popc(bytes_eq(w.z, cc)) +
                           __popc(bytes_eq(w.w, cc));
        const int incl = wave_incl_scan_i(ncomma);
        uint32_t idx = cursor + (uint32_t)(incl - ncomma);  // sample index of this lane's first terminator
        const uint32_t b[6] = {(uint32_t)wave_shr1_i((int)w.z, (int)cz), (uint32_t)wave_shr1_i((int)w.w, (int)cw),
                               w.x, w.y, w.z, w.w};
        // automaton over the 8 look-back bytes and the lane's own 16: `open` = the start of the current token was seen
        uint32_t open = 0, val = 0, ndig = 0, neg = 0, first = 0, bad = 0;
#pragma unroll
        for (int j = 0; j < 24; ++j) {
            const uint32_t c = (b[j >> 2] >> (8 * (j & 3))) & 0xffu;
            const uint32_t d = c - (uint32_t)'0';
            if (c == (uint32_t)',' || c == 0x01u) {
                if (j >= 8 && c == (uint32_t)',') {
                    const uint32_t ok = open & (bad == 0) & (ndig >= 1u) & (ndig <= 5u) & ((first != 0) | ((ndig == 1u) & (neg == 0))) &
                                        (val <= 32767u + neg);
                    if (!ok) err = 1;
                    const int32_t v = neg ? -(int32_t)val : (int32_t)val;
                    if (ok && idx < count) out[idx] = (int16_t)v;
                    ++idx;
                }
                open = 1; val = 0; ndig = 0; neg = 0; first = 0; bad = 0;
            } else if (d <= 9u) {
                if (ndig == 0) first = d;
                val = val * 10u + d;
                ndig = ndig < 15u ? ndig + 1u : ndig;
                if (ndig > 5u) val = 99999u;  // (no wrap-around into range)
            } else if (c == (uint32_t)'-') {
                if (ndig != 0 || neg) bad = 1;
                neg = 1;
            } else {
                bad = 1;
            }
        }
        cursor += (uint32_t)wave_last_i(incl);
        cz = (uint32_t)__builtin_amdgcn_readlane((int)w.z, 63);
        cw = (uint32_t)__builtin_amdgcn_readlane((int)w.w, 63);
    }
    const int any_err = __any((int)err);
    if (l == 0) a.status[r] = any_err ? 2u : (cursor != count ? 1u : 0u);
}

int launch_sigtext(const SigTextArgs &a, hipStream_t st) {
    if (a.n_reads == 0) return SGK_OK;
    SGK_LAUNCH("k_sigtext_decode", k_sigtext_decode, a.n_reads, 64, st, a);
    return SGK_OK;
}

}  // namespace sgk

extern "C" int sgk_sigtext_decode(const uint8_t *text, const uint64_t *text_offsets, const uint32_t *text_lengths,
                                  uint32_t n_reads, int16_t *samples, const uint64_t *offsets,
                                  const uint32_t *lengths, uint32_t *status, void *stream) {
    if (n_reads == 0) return SGK_OK;
    if (!text || !text_offsets || !text_lengths || !samples || !offsets || !lengths || !status) return SGK_ERR_ARG;
    sgk::SigTextArgs a = {text, text_offsets, text_lengths, samples, offsets, lengths, status, n_reads};
    return sgk::launch_sigtext(a, static_cast<hipStream_t>(stream));
}
