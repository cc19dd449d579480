// zstd_kernels.hip -- zstd frames (RFC 8878) decoded on the GPU, one wavefront per frame.
//
// Why: BLOW5 files with record compression 2 hold one zstd frame per record (slow5lib/src/slow5_press.c:1156-1200; what
// MinKNOW writes and `slow5tools -c zstd` recommends).  As with zlib records (inflate_kernels.hip) the records go to the
// GPU as they sit in the file, a wavefront decodes each into device memory, and the svb-zd decoder reads the signal blob
// from there.  The host decoder (host/zstd_dec.c) takes and refuses the same frames with the same statuses.
//
// One frame per wavefront, a grid that strides over the frames.  What is serial in the format runs on wave-uniform values
// (block and section headers, the FSE distribution, the sequence loop with its three states and its backward bitstream,
// read through a window of the input the lanes hold one dword each); the lanes work together where there is work to share:
//   * FSE tables: a lane per symbol -- the spread order of the cells by ballots, the cells of a symbol numbered by the lane
//     that owns it; the Huffman table: a lane per symbol, ranked within its weight by ballots;
//   * the four Huffman streams of a literals section are decoded by four lanes side by side (one lane for a single
//     stream), each with its own bit buffer, into the block's literals scratch in global memory (up to 128 KB: sized by
//     the resident wavefronts, not by the frames);
//   * literals and matches are copied up to 64 bytes per step into a 4 KB ring in LDS, lane i the byte at offset
//     - (i mod offset) (overlapping matches included), from the ring when the match reaches back less than 4 032 bytes,
//     else from the frame's own bytes in global memory; completed 1 KB chunks of the ring leave as 16-byte stores;
//   * the content checksum (XXH64), when the frame carries one: its four lanes of stripes on four lanes.
// Every loop is bounded by input bytes, output room or the declared sequence count: a hostile frame ends with a status.
#include "job_launch.h"
#include "sgk_common.h"

#include <map>
#include <mutex>
#include <utility>

namespace sgk {

constexpr int ZS_WIN = 4096;             // the output ring in LDS
constexpr int ZS_NEAR = ZS_WIN - 64;     // a step of up to 64 bytes at up to this offset reads the ring
constexpr int ZS_FLUSH = 1024;           // bytes per flush of the ring (64 lanes x 16)
constexpr uint32_t ZS_BLOCK_MAX = 128u << 10;
constexpr uint32_t ZS_LIT_STRIDE = ZS_BLOCK_MAX + 256u;   // literals scratch per resident wavefront
constexpr uint32_t ZS_LL_LOG = 9, ZS_OF_LOG = 8, ZS_ML_LOG = 9, ZS_HUF_LOG = 11, ZS_W_LOG = 6;

enum {
    ZS_OK = 0,
    ZS_ERR_HEADER = 1,
    ZS_ERR_BLOCK = 2,
    ZS_ERR_TABLE = 3,
    ZS_ERR_SECTION = 4,
    ZS_ERR_OFFSET = 5,
    ZS_ERR_TRUNCATED = 6,
    ZS_ERR_CHECKSUM = 7,
    ZS_ERR_SIZE = 8,
};

struct ZsArgs {
    const uint8_t *in;
    const uint64_t *in_offsets;
    const uint32_t *in_lengths;
    uint8_t *out;
    const uint64_t *out_offsets;
    const uint32_t *out_caps;
    uint32_t *out_lengths;
    uint32_t *status;
    uint8_t *scratch;   // gridDim.x * ZS_LIT_STRIDE bytes
    uint32_t n;
};

struct ZsLds {
    uint8_t win[ZS_WIN];
    uint32_t ll[1 << ZS_LL_LOG], of[1 << ZS_OF_LOG], ml[1 << ZS_ML_LOG];   // symbol | bits << 8 | baseline << 16
    uint32_t wt[1 << ZS_W_LOG];         // the table of FSE-compressed Huffman weights
    uint16_t huf[1 << ZS_HUF_LOG];      // symbol | code length << 8
    uint16_t order[1 << ZS_LL_LOG];     // FSE build: the cells in the order the spread visits them
    uint8_t sym[1 << ZS_LL_LOG];        // FSE build: the symbol of every cell
    int16_t counts[64];                 // an FSE distribution as read
    uint8_t w[256];                     // Huffman weights
};
static_assert(sizeof(ZsLds) <= 16384, "ten frames per compute unit");

__constant__ const int16_t ZS_LL_DEFAULT[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
__constant__ const int16_t ZS_ML_DEFAULT[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                                1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
__constant__ const int16_t ZS_OF_DEFAULT[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
__constant__ const uint32_t ZS_LL_BASE[36] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40,
                                              48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
__constant__ const uint8_t ZS_LL_BITS[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
__constant__ const uint32_t ZS_ML_BASE[53] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29,
                                              30, 31, 32, 33, 34, 35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
__constant__ const uint8_t ZS_ML_BITS[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                             0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};

__device__ __forceinline__ uint32_t zuni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t zhighbit(uint32_t v) { return 31u - (uint32_t)__clz((int)v); }   // v != 0
__device__ __forceinline__ uint32_t zmask(uint32_t nb) { return nb >= 32u ? 0xffffffffu : (1u << nb) - 1u; }

// ---- the input: wave-uniform reads through two 64-dword windows the lanes hold (the newest two chunks looked at: a
// stream read backwards crosses from a chunk into the one below it)
struct ZsIn {
    const uint32_t *base;   // 4-byte aligned start of the frame's dwords
    uint32_t n_dw;          // dwords that may be read
    uint32_t lead;          // the frame's first byte within base
    uint32_t len;           // the frame's bytes
    uint32_t wa, wb;        // per lane: dword (chunk * 64 + lane) of chunks ca and cb
    uint32_t ca, cb;

    __device__ __forceinline__ uint32_t dword(uint32_t k) {
        const uint32_t c = k >> 6;
        if (c != ca) {
            if (c == cb) {
                const uint32_t t = wa; wa = wb; wb = t;
                cb = ca;
            } else {
                wb = wa;
                cb = ca;
                const uint32_t i = c * 64u + (uint32_t)lane_id();
                wa = i < n_dw ? base[i] : 0u;
            }
            ca = c;
        }
        return (uint32_t)__builtin_amdgcn_readlane((int)wa, (int)(k & 63u));
    }
    // nb <= 32 bits from bit `bit` behind byte `byte` of the frame (the caller stays inside the frame)
    __device__ __forceinline__ uint32_t bits(uint32_t byte, uint32_t bit, uint32_t nb) {
        const uint32_t a = lead + byte + (bit >> 3), bb = (a & 3u) * 8u + (bit & 7u);
        const uint32_t k = a >> 2, w0 = dword(k), w1 = dword(k + 1u);
        return (uint32_t)(((((unsigned long long)w1) << 32) | w0) >> bb) & zmask(nb);
    }
    __device__ __forceinline__ uint32_t u8(uint32_t byte) { return bits(byte, 0u, 8u); }
};

// ---- a bitstream read backwards (4.1): bits [0, pos) behind byte `at` are unread; below bit 0 there are zeros and pos
// goes negative there
struct ZsRev {
    uint32_t at;
    int32_t pos;
};
__device__ __forceinline__ bool zs_rev_init(ZsIn &in, ZsRev &b, uint32_t at, uint32_t n) {
    if (n == 0u) return false;
    const uint32_t last = in.u8(at + n - 1u);
    if (last == 0u) return false;   // no end mark
    b.at = at;
    b.pos = (int32_t)((n - 1u) * 8u + zhighbit(last));
    return true;
}
__device__ __forceinline__ uint32_t zs_rev_get(ZsIn &in, ZsRev &b, uint32_t nb) {   // nb <= 32
    uint32_t v = 0u;
    if (nb != 0u) {
        const int32_t lo = b.pos - (int32_t)nb;
        if (lo >= 0) v = in.bits(b.at, (uint32_t)lo, nb);
        else if (b.pos > 0) v = (in.bits(b.at, 0u, (uint32_t)b.pos) << (uint32_t)(-lo)) & zmask(nb);
    }
    b.pos -= (int32_t)nb;
    return v;
}

// ---- FSE (4.1.1)
// the distribution at byte `at` (n bytes at most): counts into L.counts (lane 0 writes; the caller synchronises);
// returns the bytes it takes, or -status
__device__ int zs_fse_read_dist(ZsLds &L, ZsIn &in, uint32_t at, uint32_t n, uint32_t max_log, uint32_t max_sym, uint32_t &nsym, uint32_t &log) {
    const int l = lane_id();
    uint32_t bit = 0u;
    const uint32_t nbits = n * 8u;
    if (nbits < 4u) return -ZS_ERR_TRUNCATED;
    const uint32_t al = 5u + in.bits(at, 0u, 4u);
    bit = 4u;
    if (al > max_log) return -ZS_ERR_TABLE;
    int32_t remaining = 1 << al;
    uint32_t s = 0u;
    while (remaining > 0 && s <= max_sym) {
        const uint32_t nb = zhighbit((uint32_t)remaining + 1u) + 1u;
        if (bit + nb > nbits + 7u) return -ZS_ERR_TRUNCATED;
        uint32_t v = in.bits(at, bit, nb);
        const uint32_t lower = (1u << (nb - 1u)) - 1u, thresh = (1u << nb) - 1u - ((uint32_t)remaining + 1u);
        if ((v & lower) < thresh) {
            bit += nb - 1u;
            v &= lower;
        } else {
            bit += nb;
            if (v > lower) v -= thresh;
        }
        if (bit > nbits) return -ZS_ERR_TRUNCATED;
        const int32_t proba = (int32_t)v - 1;
        remaining -= proba < 0 ? 1 : proba;
        if (l == 0) L.counts[s] = (int16_t)proba;
        ++s;
        if (proba == 0) {
            for (;;) {   // runs of zeros, two bits each: bounded by the alphabet
                if (bit + 2u > nbits) return -ZS_ERR_TRUNCATED;
                const uint32_t r = in.bits(at, bit, 2u);
                bit += 2u;
                if (s + r > max_sym + 1u) return -ZS_ERR_TABLE;
                if (l < (int)r) L.counts[s + (uint32_t)l] = 0;
                s += r;
                if (r != 3u) break;
            }
        }
    }
    if (remaining != 0 || s > max_sym + 1u) return -ZS_ERR_TABLE;
    nsym = s;
    log = al;
    return (int)((bit + 7u) >> 3);
}

// the decoding table of a distribution: lane s holds the count of symbol s (s < nsym <= 64)
__device__ void zs_fse_build(ZsLds &L, uint32_t *t, int c, uint32_t nsym, uint32_t log) {
    const int l = lane_id();
    const uint32_t size = 1u << log, mask = size - 1u, step = (size >> 1) + (size >> 3) + 3u;
    if ((uint32_t)l >= nsym) c = 0;
    // the symbols of probability "less than one" take the cells from the top, lowest symbol highest
    const unsigned long long mh = __ballot(c == -1);
    const uint32_t nhigh = (uint32_t)__popcll(mh);
    if (c == -1) L.sym[size - 1u - (uint32_t)__popcll(mh & ((1ull << l) - 1ull))] = (uint8_t)l;
    const uint32_t high = size - 1u - nhigh;   // (nhigh < size: the counts sum to size, no more than 64 symbols of one cell)
    const int pc = c > 0 ? c : 0;
    const int incl = wave_incl_scan_i(pc);
    const uint32_t excl = (uint32_t)(incl - pc);
    // the cells at or below `high` in the order position = (position + step) & mask visits them
    uint32_t base = 0u;
    for (uint32_t j0 = 0u; j0 < size; j0 += 64u) {
        const uint32_t j = j0 + (uint32_t)l, p = (j * step) & mask;
        const bool valid = j < size && p <= high;
        const unsigned long long m = __ballot(valid);
        if (valid) L.order[base + (uint32_t)__popcll(m & ((1ull << l) - 1ull))] = (uint16_t)p;
        base += (uint32_t)__popcll(m);
    }
    __syncthreads();
    // (base == size - nhigh == the sum of the positive counts)
    int maxc = pc;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int o = __shfl_xor(maxc, d, 64);
        maxc = o > maxc ? o : maxc;
    }
    maxc = (int)zuni((uint32_t)maxc);
    for (int m = 0; m < maxc; ++m)
        if (m < pc) L.sym[L.order[excl + (uint32_t)m]] = (uint8_t)l;
    __syncthreads();
    // the cells of a symbol, by position, are its states count, count + 1, ...: the lane that owns the symbol numbers them
    uint32_t nx = c == -1 ? 1u : (uint32_t)pc;
    for (uint32_t i0 = 0u; i0 < size; i0 += 8u) {
        uint32_t cs[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) cs[k] = L.sym[i0 + (uint32_t)k];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (cs[k] == (uint32_t)l) {
                const uint32_t nb = log - zhighbit(nx);
                t[i0 + (uint32_t)k] = cs[k] | (nb << 8) | (((nx << nb) - size) << 16);
                ++nx;
            }
        }
    }
    __syncthreads();
}

// ---- Huffman (4.2.1): the tree description at `at` (n bytes at most) -> L.huf; returns the bytes it takes, or -status
__device__ int zs_huf_read(ZsLds &L, ZsIn &in, uint32_t at, uint32_t n, uint32_t &huf_log) {
    const int l = lane_id();
    if (n < 1u) return -ZS_ERR_TRUNCATED;
    uint32_t nw, used;
    const uint32_t h = in.u8(at);
    __syncthreads();   // (L.w and the build arrays are free: nothing of an earlier block reads them)
    if (h >= 128u) {
        nw = h - 127u;
        used = 1u + (nw + 1u) / 2u;
        if (used > n) return -ZS_ERR_TRUNCATED;
        for (uint32_t i0 = 0u; i0 < nw; i0 += 64u) {
            const uint32_t i = i0 + (uint32_t)l;
            // (uniform reads: a weight pair per step of the window would do; 128 weights at most)
            uint32_t v = 0u;
            for (uint32_t k = 0u; k < 64u && i0 + k < nw; k += 2u) {
                const uint32_t byte = in.u8(at + 1u + (i0 + k) / 2u);
                if ((uint32_t)l == k) v = byte >> 4;
                if ((uint32_t)l == k + 1u) v = byte & 15u;
            }
            if (i < nw) L.w[i] = (uint8_t)v;
        }
    } else {
        used = 1u + h;
        if (used > n) return -ZS_ERR_TRUNCATED;
        if (h < 2u) return -ZS_ERR_TABLE;
        uint32_t ns = 0u, log = 0u;
        const int hb = zs_fse_read_dist(L, in, at + 1u, h, ZS_W_LOG, 11u, ns, log);
        if (hb < 0) return -ZS_ERR_TABLE;
        __syncthreads();
        zs_fse_build(L, L.wt, (uint32_t)l < ns ? (int)L.counts[l] : 0, ns, log);
        ZsRev b;
        if ((uint32_t)hb >= h || !zs_rev_init(in, b, at + 1u + (uint32_t)hb, h - (uint32_t)hb)) return -ZS_ERR_TABLE;
        // two states take turns until one of them would read in front of the stream (4.2.1.2)
        uint32_t s1 = zs_rev_get(in, b, log), s2 = zs_rev_get(in, b, log);
        if (b.pos < 0) return -ZS_ERR_TABLE;
        nw = 0u;
        for (;;) {
            if (nw > 253u) return -ZS_ERR_TABLE;
            const uint32_t c1 = zuni(L.wt[s1]);
            if (l == 0) L.w[nw] = (uint8_t)c1;
            ++nw;
            s1 = (c1 >> 16) + zs_rev_get(in, b, (c1 >> 8) & 255u);
            const uint32_t c2 = zuni(L.wt[s2]);
            if (l == 0) L.w[nw] = (uint8_t)c2;   // (either way the other state's symbol comes next)
            ++nw;
            if (b.pos < 0) break;
            s2 = (c2 >> 16) + zs_rev_get(in, b, (c2 >> 8) & 255u);
            if (b.pos < 0) {
                const uint32_t c3 = zuni(L.wt[s1]);
                if (l == 0) L.w[nw] = (uint8_t)c3;
                ++nw;
                break;
            }
        }
    }
    __syncthreads();
    // the last weight completes the sum to a power of two; lanes: symbol l, l + 64, ...
    uint32_t sum = 0u, bad = 0u;
    uint32_t wv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t s = (uint32_t)(q * 64 + l);
        wv[q] = s < nw ? (uint32_t)L.w[s] : 0u;
        if (wv[q] > ZS_HUF_LOG) bad = 1u;
        if (wv[q]) sum += 1u << (wv[q] - 1u);
    }
    if (__ballot(bad != 0u)) return -ZS_ERR_TABLE;
    sum = (uint32_t)wave_last_i(wave_incl_scan_i((int)sum));
    if (sum == 0u) return -ZS_ERR_TABLE;
    const uint32_t log = zhighbit(sum) + 1u, left = (1u << log) - sum;
    if (log > ZS_HUF_LOG || (left & (left - 1u)) != 0u) return -ZS_ERR_TABLE;
    const uint32_t wlast = zhighbit(left) + 1u;
    if ((nw & 63u) == (uint32_t)l) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if ((nw >> 6) == (uint32_t)q) wv[q] = wlast;
    }
    ++nw;
    // symbols per weight, where each weight's cells start (weight 1, the longest codes, from cell 0), each symbol's rank
    uint32_t rank[ZS_HUF_LOG + 1];
#pragma unroll
    for (int k = 1; k <= (int)ZS_HUF_LOG; ++k) {
        rank[k] = 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) rank[k] += (uint32_t)__popcll(__ballot(wv[q] == (uint32_t)k));
    }
    if (rank[1] < 2u || (rank[1] & 1u)) return -ZS_ERR_TABLE;
    uint32_t start[ZS_HUF_LOG + 1], seen[ZS_HUF_LOG + 1], at_cell = 0u;
#pragma unroll
    for (int k = 1; k <= (int)ZS_HUF_LOG; ++k) {
        start[k] = at_cell;
        at_cell += rank[k] << (k - 1);
        seen[k] = 0u;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t first = 0u;
#pragma unroll
        for (int k = 1; k <= (int)ZS_HUF_LOG; ++k) {
            const unsigned long long m = __ballot(wv[q] == (uint32_t)k);
            if (wv[q] == (uint32_t)k) first = start[k] + ((seen[k] + (uint32_t)__popcll(m & ((1ull << l) - 1ull))) << (k - 1));
            seen[k] += (uint32_t)__popcll(m);
        }
        if (wv[q]) {
            const uint32_t span = 1u << (wv[q] - 1u);
            const uint16_t e = (uint16_t)((uint32_t)(q * 64 + l) | ((log + 1u - wv[q]) << 8));
            for (uint32_t k = 0u; k < span; ++k) L.huf[first + k] = e;   // (first + span <= 2^log: the weights sum to it)
        }
    }
    __syncthreads();
    huf_log = log;
    return (int)used;
}

// Huffman streams, one per lane (ns = 1 or 4 of them): lane k decodes cnt symbols of the stream at byte sb, sn bytes
// long, into dst[0 .. cnt).  All of a stream's bits and no more.  Returns whether every stream did.
__device__ bool zs_huf_streams(const ZsLds &L, const ZsIn &in, uint32_t ns, uint32_t sb, uint32_t sn, uint8_t *dst, uint32_t cnt, uint32_t log) {
    const int l = lane_id();
    const bool mine = (uint32_t)l < ns;
    bool ok = true;
    if (!mine) { cnt = 0u; sn = 1u; sb = 0u; }
    if (sn == 0u) { ok = false; cnt = 0u; sn = 1u; sb = 0u; }
    // (per-lane loads of aligned dwords of the frame; those behind its end are not read)
    const uint32_t a0 = in.lead + sb;
    const uint32_t *base = in.base;
    const uint32_t n_dw = in.n_dw;
    uint32_t last = 0u;
    {
        const uint32_t a = a0 + sn - 1u;
        last = (base[a >> 2] >> ((a & 3u) * 8u)) & 255u;   // (a byte of the frame: sb + sn <= in.len)
    }
    if (mine && last == 0u) { ok = false; cnt = 0u; last = 1u; }
    int32_t left = (int32_t)((sn - 1u) * 8u + zhighbit(last | (mine ? 0u : 1u)));   // unread bits of the stream
    int32_t lo = left;                        // bits not yet in the buffer
    unsigned long long buf = 0ull;            // the next bits, from the top
    uint32_t have = 0u;                       // valid bits in buf
    const uint32_t maxcnt = [&] {
        uint32_t m = cnt;
#pragma unroll
        for (int d = 2; d >= 1; d >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)m, d, 64);
            m = o > m ? o : m;
        }
        return zuni(m);
    }();
    for (uint32_t i = 0u; i < maxcnt; ++i) {
        if (have <= 32u) {
            // the 32 bits below `lo` (zeros below the stream's first bit)
            uint32_t w = 0u;
            if (lo > 0) {
                const uint32_t b = lo >= 32 ? (uint32_t)(lo - 32) : 0u;
                const uint32_t ab = (a0 & 3u) * 8u + b, k = (a0 >> 2) + (ab >> 5), sh = ab & 31u;
                const uint32_t w0 = k < n_dw ? base[k] : 0u, w1 = k + 1u < n_dw ? base[k + 1u] : 0u;
                w = (uint32_t)(((((unsigned long long)w1) << 32) | w0) >> sh);
                if (lo < 32) w <<= (uint32_t)(32 - lo);
            }
            lo -= 32;
            buf |= (unsigned long long)w << (32u - have);
            have += 32u;
        }
        if (i < cnt) {
            const uint32_t e = L.huf[(uint32_t)(buf >> (64u - log))];
            const uint32_t len = e >> 8;
            dst[i] = (uint8_t)e;
            buf <<= len;
            have -= len;
            left -= (int32_t)len;
        }
    }
    if (mine && left != 0) ok = false;
    return __ballot(!ok) == 0ull;
}

// ---- the output: a ring in LDS, flushed 1 KB at a time
struct ZsOut {
    uint8_t *dst;        // where the frame's bytes go (16-byte aligned)
    uint32_t cap;        // bytes kept (the declared content size: checked against out_caps[r] before anything is written)
    uint32_t pos;        // bytes produced
    uint32_t flushed;    // bytes that have left the ring (multiple of ZS_FLUSH)
};
__device__ __forceinline__ void zs_flush(ZsLds &L, ZsOut &o, uint32_t m) {
    const int l = lane_id();
    const uint32_t j0 = (uint32_t)l * 16u;
    const uint4 v = *reinterpret_cast<const uint4 *>(&L.win[(o.flushed + j0) & (ZS_WIN - 1)]);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    const uint32_t at = o.flushed + j0;
    if (at + 16u <= o.cap && j0 + 16u <= m) {
        *reinterpret_cast<uint4 *>(o.dst + at) = v;
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (at + (uint32_t)k < o.cap && j0 + (uint32_t)k < m) o.dst[at + k] = (uint8_t)((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
    }
    o.flushed += m;
}
// lane i < n (n <= 64) appends byte v
__device__ __forceinline__ void zs_put(ZsLds &L, ZsOut &o, uint32_t n, uint32_t v) {
    const int l = lane_id();
    if ((uint32_t)l < n) L.win[(o.pos + (uint32_t)l) & (ZS_WIN - 1)] = (uint8_t)v;
    __syncthreads();
    o.pos += n;
    while (o.pos - o.flushed >= (uint32_t)ZS_FLUSH) zs_flush(L, o, ZS_FLUSH);
}
// n bytes from src (global memory nobody writes while they are read), or n times the byte `rle` (src null)
__device__ void zs_copy_in(ZsLds &L, ZsOut &o, const uint8_t *src, uint32_t rle, uint32_t n) {
    const int l = lane_id();
    for (uint32_t i0 = 0u; i0 < n; i0 += 64u) {
        const uint32_t m = n - i0 < 64u ? n - i0 : 64u;
        uint32_t v = rle;
        if (src && (uint32_t)l < m) v = src[i0 + (uint32_t)l];
        zs_put(L, o, m, v);
    }
}
// a match: out[pos + i] = out[pos + i - off], off <= pos
__device__ void zs_copy_match(ZsLds &L, ZsOut &o, uint32_t off, uint32_t n) {
    const int l = lane_id();
    for (uint32_t i0 = 0u; i0 < n; i0 += 64u) {
        const uint32_t m = n - i0 < 64u ? n - i0 : 64u;
        uint32_t v = 0u;
        if (off <= (uint32_t)ZS_NEAR) {
            const uint32_t i = off >= m ? (uint32_t)l : (uint32_t)l % off;
            v = L.win[(o.pos - off + i) & (ZS_WIN - 1)];
        } else {
            // further back than the ring holds: those bytes left it at least ZS_NEAR - 1023 - 63 bytes ago.  Past the
            // vector L1, behind the wave's own stores.
            __builtin_amdgcn_s_waitcnt(0x0F70);
            if ((uint32_t)l < m) v = __hip_atomic_load(o.dst + (o.pos - off + (uint32_t)l), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        zs_put(L, o, m, v);
    }
}

// ---- XXH64, seed 0, of dst[0 .. n) (global memory; the caller has waited for its stores)
constexpr unsigned long long XP1 = 0x9E3779B185EBCA87ull, XP2 = 0xC2B2AE3D27D4EB4Full, XP3 = 0x165667B19E3779F9ull,
                             XP4 = 0x85EBCA77C2B2AE63ull, XP5 = 0x27D4EB2F165667C5ull;
__device__ __forceinline__ unsigned long long zrotl(unsigned long long v, int r) { return (v << r) | (v >> (64 - r)); }
__device__ __forceinline__ unsigned long long zxround(unsigned long long acc, unsigned long long v) { return zrotl(acc + v * XP2, 31) * XP1; }
__device__ __forceinline__ unsigned long long zxmerge(unsigned long long h, unsigned long long v) { return (h ^ zxround(0ull, v)) * XP1 + XP4; }
__device__ __forceinline__ unsigned long long zs_ld64(const uint8_t *p) {   // 8-byte aligned
    return __hip_atomic_load(reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t zs_ld8(const uint8_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long zreadlane64(unsigned long long v, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ unsigned long long zs_xxh64(const uint8_t *dst, uint32_t n) {
    const int l = lane_id();
    unsigned long long h;
    uint32_t at = 0u;
    if (n >= 32u) {
        // the four accumulators on lanes 0 .. 3, a stripe of 32 bytes per step
        unsigned long long acc = l == 0 ? XP1 + XP2 : (l == 1 ? XP2 : (l == 2 ? 0ull : 0ull - XP1));
        const uint32_t stripes = n / 32u;
        for (uint32_t s = 0u; s < stripes; ++s)
            if (l < 4) acc = zxround(acc, zs_ld64(dst + s * 32u + (uint32_t)l * 8u));
        const unsigned long long v1 = zreadlane64(acc, 0), v2 = zreadlane64(acc, 1), v3 = zreadlane64(acc, 2), v4 = zreadlane64(acc, 3);
        h = zrotl(v1, 1) + zrotl(v2, 7) + zrotl(v3, 12) + zrotl(v4, 18);
        h = zxmerge(h, v1); h = zxmerge(h, v2); h = zxmerge(h, v3); h = zxmerge(h, v4);
        at = stripes * 32u;
    } else h = XP5;
    h += (unsigned long long)n;
    for (; at + 8u <= n; at += 8u) h = zrotl(h ^ zxround(0ull, zs_ld64(dst + at)), 27) * XP1 + XP4;
    if (at + 4u <= n) {
        const uint32_t w = zs_ld8(dst + at) | (zs_ld8(dst + at + 1u) << 8) | (zs_ld8(dst + at + 2u) << 16) | (zs_ld8(dst + at + 3u) << 24);
        h = zrotl(h ^ (w * XP1), 23) * XP2 + XP3;
        at += 4u;
    }
    for (; at < n; ++at) h = zrotl(h ^ (zs_ld8(dst + at) * XP5), 11) * XP1;
    h ^= h >> 33; h *= XP2; h ^= h >> 29; h *= XP3; h ^= h >> 32;
    return zreadlane64(h, 0);
}

// ---- the state that lasts a frame
struct ZsFrame {
    uint32_t rep0, rep1, rep2;
    uint32_t huf_log, ll_log, of_log, ml_log;
    bool have_huf, have_ll, have_of, have_ml;
};

// one compressed block (3.1.1.3): bytes [p, p + n) of the frame; room: what the block may still produce
__device__ uint32_t zs_block(ZsLds &L, ZsIn &in, ZsOut &o, ZsFrame &f, uint8_t *lit_scratch, uint32_t p, uint32_t n, uint32_t room) {
    const int l = lane_id();
    // literals section
    if (n < 1u) return ZS_ERR_SECTION;
    const uint32_t b0 = in.u8(p), type = b0 & 3u, sf = (b0 >> 2) & 3u;
    uint32_t hl, regen, comp = 0u, streams = 1u;
    if (type < 2u) {
        if ((sf & 1u) == 0u) { hl = 1u; regen = b0 >> 3; }
        else if (sf == 1u) { hl = 2u; if (n < 2u) return ZS_ERR_SECTION; regen = (b0 >> 4) | (in.u8(p + 1u) << 4); }
        else { hl = 3u; if (n < 3u) return ZS_ERR_SECTION; regen = (b0 >> 4) | (in.u8(p + 1u) << 4) | (in.u8(p + 2u) << 12); }
    } else {
        hl = sf < 2u ? 3u : sf + 2u;
        if (n < hl) return ZS_ERR_SECTION;
        const uint32_t nb = sf < 2u ? 10u : (sf == 2u ? 14u : 18u);
        regen = in.bits(p, 4u, nb);
        comp = in.bits(p, 4u + nb, nb);
        streams = sf == 0u ? 1u : 4u;
    }
    if (regen > ZS_BLOCK_MAX) return ZS_ERR_SECTION;
    const uint8_t *frame = reinterpret_cast<const uint8_t *>(in.base) + in.lead;
    const uint8_t *lit = nullptr;   // null: the byte lit_rle repeated
    uint32_t lit_rle = 0u;
    uint32_t at = hl;
    if (type == 0u) {
        if (regen > n - at) return ZS_ERR_SECTION;
        lit = frame + p + at;
        at += regen;
    } else if (type == 1u) {
        if (n - at < 1u) return ZS_ERR_SECTION;
        lit_rle = in.u8(p + at);
        at += 1u;
    } else {
        if (comp > n - at) return ZS_ERR_SECTION;
        uint32_t q = p + at, qn = comp;
        at += comp;
        if (type == 2u) {
            const int used = zs_huf_read(L, in, q, qn, f.huf_log);
            if (used < 0) return used == -ZS_ERR_TRUNCATED ? ZS_ERR_SECTION : (uint32_t)-used;
            f.have_huf = true;
            q += (uint32_t)used;
            qn -= (uint32_t)used;
        } else if (!f.have_huf) return ZS_ERR_TABLE;
        bool ok;
        if (streams == 1u) {
            ok = zs_huf_streams(L, in, 1u, q, qn, lit_scratch, regen, f.huf_log);
        } else {
            if (qn < 6u) return ZS_ERR_SECTION;
            const uint32_t s1 = in.bits(q, 0u, 16u), s2 = in.bits(q, 16u, 16u), s3 = in.bits(q, 32u, 16u);
            if (s1 + s2 + s3 > qn - 6u) return ZS_ERR_SECTION;
            const uint32_t s4 = qn - 6u - s1 - s2 - s3, seg = (regen + 3u) / 4u;
            if (seg * 3u > regen) return ZS_ERR_SECTION;
            const uint32_t sb = q + 6u + (l >= 1 ? s1 : 0u) + (l >= 2 ? s2 : 0u) + (l >= 3 ? s3 : 0u);
            const uint32_t sn = l == 0 ? s1 : (l == 1 ? s2 : (l == 2 ? s3 : s4));
            const uint32_t cnt = l < 3 ? seg : regen - 3u * seg;
            ok = zs_huf_streams(L, in, 4u, sb, sn, lit_scratch + (uint32_t)(l < 4 ? l : 0) * seg, cnt, f.huf_log);
        }
        if (!ok) return ZS_ERR_SECTION;
        // the literals were written by up to four lanes and are read by all of them: out to L2, and nothing stale in L1
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        lit = lit_scratch;
    }
    // sequences section
    if (n - at < 1u) return ZS_ERR_SECTION;
    uint32_t nseq = in.u8(p + at);
    ++at;
    if (nseq >= 128u) {
        if (nseq == 255u) {
            if (n - at < 2u) return ZS_ERR_SECTION;
            nseq = in.bits(p + at, 0u, 16u) + 0x7f00u;
            at += 2u;
        } else {
            if (n - at < 1u) return ZS_ERR_SECTION;
            nseq = ((nseq - 128u) << 8) + in.u8(p + at);
            ++at;
        }
    }
    const uint32_t start = o.pos;
    uint32_t lit_at = 0u;
    if (nseq == 0u) {
        if (at != n) return ZS_ERR_SECTION;
    } else {
        if (n - at < 1u) return ZS_ERR_SECTION;
        const uint32_t modes = in.u8(p + at);
        ++at;
        if (modes & 3u) return ZS_ERR_SECTION;
        for (int k = 0; k < 3; ++k) {
            const uint32_t mode = (modes >> (6 - 2 * k)) & 3u;
            uint32_t *t = k == 0 ? L.ll : (k == 1 ? L.of : L.ml);
            uint32_t &log = k == 0 ? f.ll_log : (k == 1 ? f.of_log : f.ml_log);
            bool &have = k == 0 ? f.have_ll : (k == 1 ? f.have_of : f.have_ml);
            const uint32_t max_sym = k == 0 ? 35u : (k == 1 ? 31u : 52u), max_log = k == 0 ? ZS_LL_LOG : (k == 1 ? ZS_OF_LOG : ZS_ML_LOG);
            if (mode == 0u) {
                const uint32_t ns = k == 0 ? 36u : (k == 1 ? 29u : 53u);
                int c = 0;
                if ((uint32_t)l < ns) c = k == 0 ? ZS_LL_DEFAULT[l] : (k == 1 ? ZS_OF_DEFAULT[l] : ZS_ML_DEFAULT[l]);
                log = k == 1 ? 5u : 6u;
                __syncthreads();
                zs_fse_build(L, t, c, ns, log);
            } else if (mode == 1u) {
                if (n - at < 1u) return ZS_ERR_SECTION;
                const uint32_t s = in.u8(p + at);
                if (s > max_sym) return ZS_ERR_TABLE;
                ++at;
                __syncthreads();
                if (l == 0) t[0] = s;   // one state, no bits
                __syncthreads();
                log = 0u;
            } else if (mode == 2u) {
                uint32_t ns = 0u;
                __syncthreads();
                const int used = zs_fse_read_dist(L, in, p + at, n - at, max_log, max_sym, ns, log);
                if (used < 0) return used == -ZS_ERR_TRUNCATED ? ZS_ERR_SECTION : (uint32_t)-used;
                __syncthreads();
                zs_fse_build(L, t, (uint32_t)l < ns ? (int)L.counts[l] : 0, ns, log);
                at += (uint32_t)used;
            } else if (!have) return ZS_ERR_TABLE;
            have = true;
        }
        ZsRev b;
        if (at >= n || !zs_rev_init(in, b, p + at, n - at)) return ZS_ERR_SECTION;
        uint32_t sl = zs_rev_get(in, b, f.ll_log), so = zs_rev_get(in, b, f.of_log), sm = zs_rev_get(in, b, f.ml_log);
        if (b.pos < 0) return ZS_ERR_SECTION;
        for (uint32_t i = 0u; i < nseq; ++i) {
            const uint32_t cl = zuni(L.ll[sl]), co = zuni(L.of[so]), cm = zuni(L.ml[sm]);
            const uint32_t oc = co & 255u, mc = cm & 255u, lc = cl & 255u;
            if (lc > 35u || mc > 52u || oc > 31u) return ZS_ERR_SECTION;   // (never: the tables hold no such symbol)
            const unsigned long long ov = (1ull << oc) + zs_rev_get(in, b, oc);
            const uint32_t mlen = ZS_ML_BASE[mc] + zs_rev_get(in, b, ZS_ML_BITS[mc]);
            const uint32_t ll = ZS_LL_BASE[lc] + zs_rev_get(in, b, ZS_LL_BITS[lc]);
            if (i + 1u < nseq) {
                sl = (cl >> 16) + zs_rev_get(in, b, (cl >> 8) & 255u);
                sm = (cm >> 16) + zs_rev_get(in, b, (cm >> 8) & 255u);
                so = (co >> 16) + zs_rev_get(in, b, (co >> 8) & 255u);
            }
            if (b.pos < 0) return ZS_ERR_SECTION;
            unsigned long long off;
            if (ov > 3ull) {
                off = ov - 3ull;
                f.rep2 = f.rep1;
                f.rep1 = f.rep0;
            } else {
                const uint32_t idx = (uint32_t)ov - 1u + (ll == 0u ? 1u : 0u);   // 0 .. 3
                if (idx == 0u) off = f.rep0;
                else {
                    off = idx == 3u ? (unsigned long long)f.rep0 - 1ull : (idx == 1u ? f.rep1 : f.rep2);
                    if (idx != 1u) f.rep2 = f.rep1;
                    f.rep1 = f.rep0;
                }
            }
            if (off == 0ull || off > 0xffffffffull) return ZS_ERR_OFFSET;
            f.rep0 = (uint32_t)off;
            if (ll > regen - lit_at) return ZS_ERR_SECTION;
            if ((unsigned long long)ll + mlen > (unsigned long long)(room - (o.pos - start))) return ZS_ERR_SIZE;
            zs_copy_in(L, o, lit ? lit + lit_at : nullptr, lit_rle, ll);
            lit_at += ll;
            if (off > (unsigned long long)o.pos) return ZS_ERR_OFFSET;
            zs_copy_match(L, o, (uint32_t)off, mlen);
        }
        if (b.pos != 0) return ZS_ERR_SECTION;
    }
    const uint32_t rest = regen - lit_at;
    if (rest > room - (o.pos - start)) return ZS_ERR_SIZE;
    zs_copy_in(L, o, lit ? lit + lit_at : nullptr, lit_rle, rest);
    return ZS_OK;
}

__device__ uint32_t zs_frame(ZsLds &L, ZsIn &in, ZsOut &o, uint32_t out_cap, uint8_t *lit_scratch) {
    // the frame header (3.1.1.1)
    const uint32_t n = in.len;
    if (n < 4u) return ZS_ERR_TRUNCATED;
    if (in.bits(0u, 0u, 32u) != 0xFD2FB528u) return ZS_ERR_HEADER;   // (a skippable frame too)
    if (n < 5u) return ZS_ERR_TRUNCATED;
    const uint32_t d = in.u8(4u), fcs_flag = d >> 6, single = (d >> 5) & 1u, did_flag = d & 3u;
    if (d & 8u) return ZS_ERR_HEADER;
    const uint32_t did_len = did_flag == 3u ? 4u : did_flag, fcs_len = fcs_flag == 0u ? single : 1u << fcs_flag;
    if (fcs_len == 0u) return ZS_ERR_HEADER;   // no content size
    uint32_t at = 5u + (single ? 0u : 1u);
    if (n < at || n - at < did_len + fcs_len) return ZS_ERR_TRUNCATED;
    for (uint32_t k = 0u; k < did_len; ++k)
        if (in.u8(at + k)) return ZS_ERR_HEADER;
    at += did_len;
    unsigned long long size = in.bits(at, 0u, fcs_len >= 4u ? 32u : fcs_len * 8u);
    if (fcs_len == 8u) size |= (unsigned long long)in.bits(at + 4u, 0u, 32u) << 32;
    if (fcs_len == 2u) size += 256ull;
    at += fcs_len;
    const bool checksum = (d >> 2) & 1u;
    if (size > (unsigned long long)out_cap) return ZS_ERR_SIZE;
    o.cap = (uint32_t)size;
    ZsFrame f;
    f.rep0 = 1u; f.rep1 = 4u; f.rep2 = 8u;
    f.huf_log = f.ll_log = f.of_log = f.ml_log = 0u;
    f.have_huf = f.have_ll = f.have_of = f.have_ml = false;
    for (bool last = false; !last;) {
        if (n - at < 3u) return ZS_ERR_TRUNCATED;
        const uint32_t bh = in.bits(at, 0u, 24u);
        at += 3u;
        last = bh & 1u;
        const uint32_t type = (bh >> 1) & 3u, bsize = bh >> 3;
        if (type == 3u || bsize > ZS_BLOCK_MAX) return ZS_ERR_BLOCK;
        const uint32_t room = o.cap - o.pos < ZS_BLOCK_MAX ? o.cap - o.pos : ZS_BLOCK_MAX;
        if ((type == 1u ? 1u : bsize) > n - at) return ZS_ERR_TRUNCATED;
        if (type == 0u || type == 1u) {
            if (bsize > room) return ZS_ERR_SIZE;
            if (type == 0u) zs_copy_in(L, o, reinterpret_cast<const uint8_t *>(in.base) + in.lead + at, 0u, bsize);
            else zs_copy_in(L, o, nullptr, in.u8(at), bsize);
            at += type == 0u ? bsize : 1u;
        } else {
            const uint32_t rc = zs_block(L, in, o, f, lit_scratch, at, bsize, room);
            if (rc) return rc;
            at += bsize;
        }
    }
    if (o.pos != o.cap) return ZS_ERR_SIZE;
    __syncthreads();
    if (o.pos > o.flushed) zs_flush(L, o, o.pos - o.flushed);
    if (checksum) {
        if (n - at < 4u) return ZS_ERR_TRUNCATED;
        const uint32_t want = in.bits(at, 0u, 32u);
        at += 4u;
        __builtin_amdgcn_s_waitcnt(0x0F70);
        if ((uint32_t)zs_xxh64(o.dst, o.pos) != want) return ZS_ERR_CHECKSUM;
    }
    if (at != n) return ZS_ERR_HEADER;   // bytes behind the frame (another frame among them)
    return ZS_OK;
}

__global__ __launch_bounds__(64) void k_zstd(ZsArgs a) {
    __shared__ __attribute__((aligned(16))) ZsLds L;
    const int l = lane_id();
    uint8_t *lit_scratch = a.scratch + (size_t)blockIdx.x * ZS_LIT_STRIDE;
    for (uint32_t r = blockIdx.x; r < a.n; r += gridDim.x) {
        const uint8_t *src = a.in + a.in_offsets[r];
        const uint32_t in_len = a.in_lengths[r];
        ZsIn in;
        in.lead = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3u);
        in.base = reinterpret_cast<const uint32_t *>(src - in.lead);
        in.n_dw = (in.lead + in_len + 3u) / 4u;
        in.len = in_len;
        in.wa = in.wb = 0u;
        in.ca = in.cb = 0xfffffff0u;
        ZsOut o;
        o.dst = a.out + a.out_offsets[r];
        o.cap = 0u;
        o.pos = 0u;
        o.flushed = 0u;
        __syncthreads();   // (the ring and the tables are the previous frame's until here)
        const uint32_t st = zs_frame(L, in, o, a.out_caps[r], lit_scratch);
        if (l == 0) {
            a.status[r] = st;
            a.out_lengths[r] = st == ZS_OK ? o.pos : (o.flushed < o.cap ? o.flushed : o.cap);
        }
    }
}

// ---- the literals scratch: one allocation per device and stream, grown when a launch needs more; a job's is freed with
// the job, that of a stream the caller of sgk_zstd_decompress owns stays for the life of the process
struct ZsScratch {
    void *p = nullptr;
    size_t bytes = 0;
};
static std::mutex g_zs_mu;
static std::map<std::pair<int, hipStream_t>, ZsScratch> g_zs_scratch;
static int g_zs_waves[64];   // resident wavefronts of k_zstd per device (0: not asked yet)

int launch_zstd(ZsArgs a, hipStream_t st) {
    if (a.n == 0) return SGK_OK;
    int dev = 0;
    SGK_HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_zs_mu);
    if (dev < 0 || dev >= 64) return SGK_ERR_ARG;
    if (g_zs_waves[dev] == 0) {
        int cus = 0;
        SGK_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        const int per_cu = (int)(163840 / sizeof(ZsLds));   // LDS decides how many frames a compute unit holds
        g_zs_waves[dev] = (cus > 0 ? cus : 1) * (per_cu < 32 ? per_cu : 32);
    }
    const uint32_t grid = a.n < (uint32_t)g_zs_waves[dev] ? a.n : (uint32_t)g_zs_waves[dev];
    ZsScratch &s = g_zs_scratch[std::make_pair(dev, st)];
    const size_t need = (size_t)grid * ZS_LIT_STRIDE;
    if (s.bytes < need) {
        if (s.p) SGK_HIP_TRY(hipFree(s.p));   // (waits for the launches that use it)
        s.p = nullptr;
        s.bytes = 0;
        SGK_HIP_TRY(hipMalloc(&s.p, need));
        s.bytes = need;
    }
    a.scratch = static_cast<uint8_t *>(s.p);
    SGK_LAUNCH("k_zstd", k_zstd, grid, 64, st, a);
    return SGK_OK;
}

// what a stream's owner calls before it destroys the stream (sgk_job_destroy does), after the stream's work is done: the
// scratch kept for it is freed, and a later stream with the same handle value starts without one
void zstd_release_scratch(int dev, hipStream_t st) {
    std::lock_guard<std::mutex> lock(g_zs_mu);
    auto it = g_zs_scratch.find(std::make_pair(dev, st));
    if (it == g_zs_scratch.end()) return;
    if (it->second.p) (void)hipFree(it->second.p);
    g_zs_scratch.erase(it);
}

}  // namespace sgk

extern "C" int sgk_zstd_decompress(const uint8_t *in, const uint64_t *in_offsets, const uint32_t *in_lengths, uint32_t n,
                                   uint8_t *out, const uint64_t *out_offsets, const uint32_t *out_caps, uint32_t *out_lengths,
                                   uint32_t *status, void *stream) {
    if (n == 0) return SGK_OK;
    if (!in || !in_offsets || !in_lengths || !out || !out_offsets || !out_caps || !out_lengths || !status) return SGK_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(out) & 15u) return SGK_ERR_ALIGN;
    sgk::ZsArgs a;
    a.in = in; a.in_offsets = in_offsets; a.in_lengths = in_lengths; a.out = out; a.out_offsets = out_offsets;
    a.out_caps = out_caps; a.out_lengths = out_lengths; a.status = status; a.scratch = nullptr; a.n = n;
    return sgk::launch_zstd(a, static_cast<hipStream_t>(stream));
}
