// deflate_kernels.hip -- zlib (RFC 1950 / 1951) streams WRITTEN on the GPU, one wavefront per stream: the counterpart of
// inflate_kernels.hip and the last record-layer codec that had no device side.
//
// Why: `qts` quantises and re-encodes the signal on the GPU (k_qts, k_svbzd_size, k_svbzd_encode) and then handed every
// blob back to the host, which spliced it into its record and called compress2() on the thread pool -- that deflate was
// the tool's whole cost.  A rewritten record is svb-zd bytes: key bytes in runs, data bytes that are
// noise.  Dynamic Huffman codes plus matches of distance 1 are what zlib's Z_RLE strategy writes, and on this data that
// is never worse than the hash-chain search of level 6.  It needs no hash table and no window.
//
// The format is fixed so that tools/proto/deflate_proto.py writes the same bytes:
//   * header 78 9C, blocks of DEF_BLOCK input bytes, big-endian Adler-32;
//   * tokens: literals and matches of distance 1.  A maximal run of L equal bytes inside a block is one literal and then
//     matches over the other L - 1 bytes, 258 at a time; a rest of 1 or 2 bytes is literals.  Runs end with the block.
//     A token is written at the LAST byte it covers (a match of 258 at the run's 259th byte, the rest at the run's end),
//     which needs the distance to the run's start -- a max-scan of run starts across the lanes, carried from tile to
//     tile -- and one byte of look-ahead.  The order of tokens in the stream is that of their first bytes all the same.
//   * a block is dynamic-Huffman when that takes fewer bits than a stored block from the same bit position, else stored;
//   * code lengths: def_build below (Huffman by the two-queue method over the symbols sorted by (count, symbol), zlib's
//     overflow repair on the leaves-per-depth counts, lengths handed out over the sorted order); the literal/length code
//     is limited to 15 bits, the code length code to 7; the distance code is the single code 0 (one bit) when the block
//     has a match, else HDIST = 0 with one length of 0, as zlib writes it;
//   * the block header's code lengths are run-length coded with 16 / 17 / 18 (def_rle).
//
// Two passes over a block, both reading it from global memory (the second read hits the cache; keeping 16 KB of block in
// LDS would leave a compute unit 6 streams): pass 1 counts symbols with LDS atomics and sums Adler-32 per tile, pass 2
// looks the codes up and writes them.  Each lane computes the bits of its 16 bytes' tokens, a wave scan gives its bit
// offset, the bits are merged into a stage in LDS with atomicOr on dwords, and the stage leaves as whole aligned dwords
// (as k_svbzd_encode's does); the bits of the last, partial dword stay for the next tile.  The code builder's node arrays
// share the stage's LDS: 8.4 KB per stream, which would allow 19 streams per compute unit as k_inflate has; the kernel's 180
// vector registers allow two waves per SIMD, 8 streams per compute unit, and that is the limit in force.
#include "job_launch.h"
#include "sgk_common.h"

namespace sgk {

constexpr int DEF_BLOCK = 16384;   // input bytes per DEFLATE block (header ~100 bytes: well under 1 %)
constexpr int DEF_VPL = 16;        // bytes per lane and tile
constexpr int DEF_TILE = 64 * DEF_VPL;
constexpr int DEF_STAGE_DW = 1024; // a tile's bits: at most 30 per byte (two literals of 15 bits) + the 31 carried
constexpr int DEF_NSYM = 288;      // literal / length symbols (286 used), a multiple of 32
constexpr int DEF_NCL = 19;

struct DefArgs {
    const uint8_t *in;             // all streams
    const uint64_t *in_offsets;    // n: byte offset of stream r
    const uint32_t *in_lengths;    // n: its bytes (< 2^29)
    uint8_t *out;                  // the zlib streams
    const uint64_t *out_offsets;   // n: 16-byte aligned offsets into out
    const uint32_t *out_caps;      // n: room for stream r
    uint32_t *out_lengths;         // n: bytes written (0 with status 1)
    uint32_t *status;              // n: 0, or 1: the stream needs more than out_caps[r] bytes
    uint32_t n;
};

struct DefLds {
    union {
        uint32_t stage[DEF_STAGE_DW];         // bits on their way out (zero behind the valid ones)
        struct {                              // def_build: the Huffman tree
            uint32_t w[2 * DEF_NSYM];         //   weights: leaves in sorted order, then the internal nodes as they are made
            uint16_t par[2 * DEF_NSYM];       //   parent of every node
        } t;
    };
    uint32_t hist[DEF_NSYM];       // symbol counts of the block
    uint32_t code[DEF_NSYM];       // (bit-reversed code << 4) | length
    uint32_t clhist[32], clcode[32];
    uint16_t order[DEF_NSYM];      // symbol at every sorted rank
    uint16_t items[DEF_NSYM + 32]; // the run-length coded code lengths: symbol | extra value << 5
    uint8_t lens[DEF_NSYM + 32];   // literal / length code lengths, the distance length behind them
    uint8_t cllens[32];
    uint32_t cnt[16], first[16], rank0[16];   // per length: codes, first canonical code, first sorted rank
    uint32_t nitems;
};
static_assert(sizeof(DefLds) <= 8704, "the LDS is not what limits the streams per compute unit");

__constant__ const uint8_t DEF_CLORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ int def_uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int def_wave_sum(int v) { return wave_last_i(wave_incl_scan_i(v)); }
__device__ __forceinline__ int def_incl_max(int v, int l) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        if (l >= d) v = t > v ? t : v;
    }
    return v;
}

// ---- code lengths and codes of one alphabet, by the whole wave.  freq[0 .. nsym) in LDS (a lone used symbol gets a
// partner with count 1 there, as zlib forces two codes); lens[] and codes[] out.  nsym <= DEF_NSYM, maxbits <= 15.
__device__ void def_build(DefLds &L, uint32_t *freq, int nsym, int maxbits, uint8_t *lens, uint32_t *codes) {
    const int l = lane_id();
    constexpr int R = (DEF_NSYM + 63) / 64;
    int n = 0;
    for (int s0 = 0; s0 < nsym; s0 += 64) n += __popcll(__ballot(s0 + l < nsym && freq[s0 + l] != 0u));
    if (n < 2) {
        if (l == 0) {
            const int extra = freq[0] == 0u ? 0 : 1;
            freq[extra] = 1u;
            if (n == 0) freq[1 - extra] = 1u;
        }
        n = 2;
    }
    if (l < 16) L.cnt[l] = 0u;
    __syncthreads();
    // sorted rank of every used symbol by (count, symbol)
    uint32_t mine[R], rank[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int s = l + 64 * i;
        const uint32_t f = s < nsym ? freq[s] : 0u;
        mine[i] = f ? ((f << 9) | (uint32_t)s) : 0u;
        rank[i] = 0u;
    }
    for (int t = 0; t < nsym; ++t) {
        const uint32_t f = freq[t];
        if (f == 0u) continue;   // (wave-uniform: every lane reads the same word)
        const uint32_t kt = (f << 9) | (uint32_t)t;
#pragma unroll
        for (int i = 0; i < R; ++i) rank[i] += kt < mine[i] ? 1u : 0u;
    }
    __syncthreads();   // (the stage's last reader is behind us: its LDS becomes the tree)
#pragma unroll
    for (int i = 0; i < R; ++i) {
        if (mine[i]) {
            L.t.w[rank[i]] = mine[i] >> 9;
            L.order[rank[i]] = (uint16_t)(mine[i] & 511u);
        }
        const int s = l + 64 * i;
        if (s < nsym) lens[s] = 0;
    }
    __syncthreads();
    // the tree: two queues (sorted leaves, internal nodes in the order they are made); of equal weights the internal
    // node goes first.  Serial: 2 (n - 1) picks.
    if (l == 0) {
        int li = 0, ii = n;
        for (int node = n; node < 2 * n - 1; ++node) {
            uint32_t sum = 0u;
            for (int k = 0; k < 2; ++k) {
                int pick;
                if (li < n && (ii >= node || L.t.w[li] < L.t.w[ii])) pick = li++;
                else pick = ii++;
                sum += L.t.w[pick];
                L.t.par[pick] = (uint16_t)node;
            }
            L.t.w[node] = sum;
        }
    }
    __syncthreads();
    // leaves per depth (beyond the limit: at the limit)
    const int root = 2 * n - 2;
    for (int q = l; q < n; q += 64) {
        int d = 0, x = q;
        while (x != root && d < 2 * DEF_NSYM) {   // (a path is shorter than the tree has nodes)
            x = L.t.par[x];
            ++d;
        }
        atomicAdd(&L.cnt[d < maxbits ? d : maxbits], 1u);
    }
    __syncthreads();
    if (l == 0) {
        // over-subscribed by `excess` codes of the longest length: zlib's repair (gen_bitlen), 2^-maxbits per step
        int excess = -(1 << maxbits);
        for (int b = 1; b <= maxbits; ++b) excess += (int)L.cnt[b] << (maxbits - b);
        while (excess > 0) {
            int bits = maxbits - 1;
            while (bits > 0 && L.cnt[bits] == 0u) --bits;
            if (bits == 0) break;   // (never: fewer symbols than codes of the longest length)
            L.cnt[bits] -= 1u;
            L.cnt[bits + 1] += 2u;
            L.cnt[maxbits] -= 1u;
            --excess;
        }
        uint32_t code = 0u, q = 0u;
        L.cnt[0] = 0u;
        for (int b = 1; b <= maxbits; ++b) {
            code = (code + L.cnt[b - 1]) << 1;
            L.first[b] = code;
        }
        for (int b = maxbits; b >= 1; --b) {
            L.rank0[b] = q;
            q += L.cnt[b];
        }
    }
    __syncthreads();
    // lengths over the sorted order: the rarest symbols get the longest codes
    for (int q = l; q < n; q += 64) {
        int len = 0;
        for (int b = 1; b <= maxbits; ++b)
            if ((uint32_t)q >= L.rank0[b] && (uint32_t)q < L.rank0[b] + L.cnt[b]) len = b;
        lens[L.order[q]] = (uint8_t)len;
    }
    __syncthreads();
    // canonical codes: rank within the length in symbol order (as inf_build), bit-reversed for the LSB-first stream
    uint32_t seen[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) seen[k] = 0u;
    for (int s0 = 0; s0 < nsym; s0 += 64) {
        const int s = s0 + l;
        const int len = s < nsym ? (int)lens[s] : 0;
        uint32_t rk = 0u;
#pragma unroll
        for (int k = 1; k <= 15; ++k) {
            const unsigned long long m = __ballot(len == k);
            if (len == k) rk = seen[k] + (uint32_t)__popcll(m & ((1ull << l) - 1ull));
            seen[k] += (uint32_t)__popcll(m);
        }
        if (s < nsym) codes[s] = len ? (((__brev(L.first[len] + rk) >> (32 - len)) << 4) | (uint32_t)len) : 0u;
    }
    __syncthreads();
}

// ---- the code lengths lens[0 .. nseq) run-length coded into L.items / L.clhist (lane 0; at most nseq items)
__device__ void def_rle(DefLds &L, int nseq) {
    uint32_t ni = 0u;
    int i = 0;
    while (i < nseq) {
        const int v = L.lens[i];
        int r = 1;
        while (i + r < nseq && L.lens[i + r] == v) ++r;
        i += r;
        if (v == 0) {
            while (r >= 11) {
                const int t = r < 138 ? r : 138;
                L.items[ni++] = (uint16_t)(18 | ((t - 11) << 5));
                L.clhist[18] += 1u;
                r -= t;
            }
            if (r >= 3) {
                L.items[ni++] = (uint16_t)(17 | ((r - 3) << 5));
                L.clhist[17] += 1u;
                r = 0;
            }
        } else {
            L.items[ni++] = (uint16_t)v;
            L.clhist[v] += 1u;
            --r;
            while (r >= 3) {
                const int t = r < 6 ? r : 6;
                L.items[ni++] = (uint16_t)(16 | ((t - 3) << 5));
                L.clhist[16] += 1u;
                r -= t;
            }
        }
        for (; r > 0; --r) {
            L.items[ni++] = (uint16_t)v;
            L.clhist[v] += 1u;
        }
    }
    L.nitems = ni;
}

// ---- the writer: bits in the stage, whole dwords to global memory
struct DefOut {
    uint32_t *dst;      // stream r's bytes (16-byte aligned)
    uint32_t cap;       // bytes that may be written
    uint32_t dw;        // dwords that have left the stage
    uint32_t sbits;     // valid bits in the stage (< 32 after a flush)
    bool over;          // the stream needs more than cap
};
// bits [off, off + nb) of the stage |= val (nb <= 32; nb == 0: nothing)
__device__ __forceinline__ void def_put(DefLds &L, uint32_t off, uint32_t val, uint32_t nb) {
    if (nb == 0u) return;
    const uint32_t dw = off >> 5, sh = off & 31u;
    atomicOr(&L.stage[dw], val << sh);
    if (sh + nb > 32u) atomicOr(&L.stage[dw + 1u], val >> (32u - sh));
}
// every lane's (val, nb) behind each other in lane order
__device__ __forceinline__ void def_emit(DefLds &L, DefOut &o, uint32_t val, uint32_t nb) {
    const int incl = wave_incl_scan_i((int)nb);
    def_put(L, o.sbits + (uint32_t)incl - nb, val, nb);
    o.sbits += (uint32_t)wave_last_i(incl);
}
__device__ __forceinline__ void def_flush(DefLds &L, DefOut &o) {
    const int l = lane_id();
    __syncthreads();
    const uint32_t ndw = o.sbits >> 5;
    if ((o.dw + ndw) * 4u > o.cap) o.over = true;
    if (!o.over)
        for (uint32_t w = (uint32_t)l; w < ndw; w += 64u) o.dst[o.dw + w] = L.stage[w];
    const uint32_t carry = L.stage[ndw];
    __syncthreads();
    for (uint32_t w = (uint32_t)l; w <= ndw; w += 64u) L.stage[w] = w == 0u ? carry : 0u;
    __syncthreads();
    o.dw += ndw;
    o.sbits &= 31u;
}

// ---- a lane's 16 bytes of a tile
struct DefLane {
    uint32_t w[4];      // the bytes, zeros beyond nval
    int nval;           // 0 .. 16
    int p0;             // block-relative position of the first
    int prv, nxt;       // the byte in front of them / behind them, -1: the block's start / end
};
__device__ __forceinline__ void def_load(const uint8_t *blk, int blen, int t0, int l, DefLane &v) {
    v.p0 = t0 + l * DEF_VPL;
    const int left = blen - v.p0;
    v.nval = left <= 0 ? 0 : (left >= DEF_VPL ? DEF_VPL : left);
    v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0u;
    if (v.nval == DEF_VPL && (reinterpret_cast<uintptr_t>(blk + v.p0) & 15u) == 0) {
        const uint4 q = *reinterpret_cast<const uint4 *>(blk + v.p0);
        v.w[0] = q.x; v.w[1] = q.y; v.w[2] = q.z; v.w[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < DEF_VPL; ++k)
            if (k < v.nval) v.w[k >> 2] |= (uint32_t)blk[v.p0 + k] << (8 * (k & 3));
    }
    v.prv = (v.nval > 0 && v.p0 > 0) ? (int)blk[v.p0 - 1] : -1;
    v.nxt = (v.nval > 0 && v.p0 + v.nval < blen) ? (int)blk[v.p0 + v.nval] : -1;
}
__device__ __forceinline__ int def_byte(const DefLane &v, int k) { return (int)((v.w[k >> 2] >> (8 * (k & 3))) & 0xffu); }

// the block-relative position of the run start that governs this lane's first byte; `carry`: that of the tile's first
// byte when it continues a run (updated to the one behind the tile)
__device__ __forceinline__ int def_run_start(const DefLane &v, int l, int &carry) {
    int ls = -1, pc = v.prv;
#pragma unroll
    for (int k = 0; k < DEF_VPL; ++k) {
        if (k < v.nval) {
            const int c = def_byte(v, k);
            if (c != pc) ls = v.p0 + k;
            pc = c;
        }
    }
    if (l == 0 && carry > ls) ls = carry;
    const int incl = def_incl_max(ls, l);
    const int up = __shfl_up(incl, 1, 64);
    const int sin = l == 0 ? carry : up;
    carry = __builtin_amdgcn_readlane(incl, 63);
    return sin;
}

// match length 3 .. 258 -> symbol, extra bits, extra value (RFC 1951 3.2.5, by arithmetic)
__device__ __forceinline__ void def_length_symbol(int len, int &sym, int &xb, int &xv) {
    const int l3 = len - 3;
    if (l3 < 8) { sym = 257 + l3; xb = 0; xv = 0; }
    else if (len == 258) { sym = 285; xb = 0; xv = 0; }
    else {
        const int e = 29 - __clz(l3);   // floor(log2(l3)) - 2
        sym = 261 + 4 * e + ((l3 >> e) & 3);
        xb = e;
        xv = l3 & ((1 << e) - 1);
    }
}

// the tokens of the lane's bytes in stream order: f(k, symbol, extra bits, extra value, literals) -- literals: 0 for a
// match, else 1 or 2 times the literal `symbol`; nothing for a byte that ends no token
template <class F>
__device__ __forceinline__ void def_tokens(const DefLane &v, int start, F f) {
    int pc = v.prv;
#pragma unroll
    for (int k = 0; k < DEF_VPL; ++k) {
        if (k < v.nval) {
            const int c = def_byte(v, k);
            const int p = v.p0 + k;
            if (c != pc) start = p;
            pc = c;
            const int nc = k + 1 < v.nval ? def_byte(v, k + 1 < DEF_VPL ? k + 1 : k) : v.nxt;
            const int kk = p - start;
            if (kk == 0) f(k, c, 0, 0, 1);
            else {
                const int o = (kk - 1) % 258;
                if (o == 257) f(k, 285, 0, 0, 0);
                else if (nc != c) {
                    const int len = o + 1;
                    if (len >= 3) {
                        int sym, xb, xv;
                        def_length_symbol(len, sym, xb, xv);
                        f(k, sym, xb, xv, 0);
                    } else f(k, c, 0, 0, len);
                }
            }
        }
    }
}

__global__ __launch_bounds__(64) void k_deflate(DefArgs a) {
    __shared__ __attribute__((aligned(16))) DefLds L;
    const uint32_t r = blockIdx.x;
    if (r >= a.n) return;
    const int l = lane_id();
    const uint8_t *src = a.in + a.in_offsets[r];
    const uint32_t n = a.in_lengths[r];
    DefOut o;
    o.dst = reinterpret_cast<uint32_t *>(a.out + a.out_offsets[r]);
    o.cap = a.out_caps[r];
    o.dw = 0u;
    o.sbits = 0u;
    o.over = false;
    for (int w = l; w < DEF_STAGE_DW; w += 64) L.stage[w] = 0u;
    __syncthreads();
    def_emit(L, o, 0x78u | (0x9Cu << 8), l == 0 ? 16u : 0u);
    uint32_t ad_a = 1u, ad_b = 0u;
    const uint32_t nblocks = n ? (n + DEF_BLOCK - 1u) / DEF_BLOCK : 1u;
    for (uint32_t bi = 0; bi < nblocks && !o.over; ++bi) {
        const uint8_t *blk = src + (size_t)bi * DEF_BLOCK;
        const int blen = (int)(n - bi * DEF_BLOCK < (uint32_t)DEF_BLOCK ? n - bi * DEF_BLOCK : (uint32_t)DEF_BLOCK);
        const uint32_t fin = bi + 1u == nblocks ? 1u : 0u;
        // ---- pass 1: symbol counts, Adler-32
        for (int s = l; s < DEF_NSYM; s += 64) L.hist[s] = 0u;
        if (l < 32) L.clhist[l] = 0u;
        __syncthreads();
        int carry = -1;
        for (int t0 = 0; t0 < blen; t0 += DEF_TILE) {
            DefLane v;
            def_load(blk, blen, t0, l, v);
            const int m = blen - t0 < DEF_TILE ? blen - t0 : DEF_TILE;
            uint32_t s1 = 0u, s2 = 0u;
#pragma unroll
            for (int k = 0; k < DEF_VPL; ++k) {
                const uint32_t d = (uint32_t)def_byte(v, k);   // (zero beyond the block)
                const int j = l * DEF_VPL + k;
                s1 += d;
                s2 += j < m ? d * (uint32_t)(m - j) : 0u;
            }
            s1 = (uint32_t)def_wave_sum((int)s1);
            s2 = (uint32_t)def_wave_sum((int)s2);
            ad_b = (ad_b + (uint32_t)m * ad_a + s2) % 65521u;
            ad_a = (ad_a + s1) % 65521u;
            const int start = def_run_start(v, l, carry);
            def_tokens(v, start, [&](int, int sym, int, int, int lits) { atomicAdd(&L.hist[sym], lits ? (uint32_t)lits : 1u); });
        }
        if (l == 0) L.hist[256] = 1u;
        __syncthreads();
        // ---- the codes
        const uint32_t carry_dw = L.stage[0];   // (the stage's LDS is the builder's for a while)
        def_build(L, L.hist, 286, 15, L.lens, L.code);
        int hi = 256, nmatch = 0, body = 0;
        for (int s0 = 0; s0 < DEF_NSYM; s0 += 64) {
            const int s = s0 + l;
            const bool used = s < 286 && L.lens[s] != 0;
            const unsigned long long mk = __ballot(used);
            if (mk) hi = s0 + 63 - __clzll((long long)mk) > hi ? s0 + 63 - __clzll((long long)mk) : hi;
            if (used) {
                const int f = (int)L.hist[s];
                int xb = 0;
                if (s > 256) {
                    nmatch += f;
                    xb = 1 + ((s >= 265 && s < 285) ? ((s - 261) >> 2) : 0);   // the distance bit, the length's extra bits
                }
                body += f * ((int)L.lens[s] + xb);
            }
        }
        body = def_wave_sum(body);
        const bool has_match = def_wave_sum(nmatch) > 0;
        const int nlit = hi + 1;
        if (l == 0) L.lens[nlit] = has_match ? 1 : 0;
        __syncthreads();
        if (l == 0) def_rle(L, nlit + 1);
        __syncthreads();
        def_build(L, L.clhist, DEF_NCL, 7, L.cllens, L.clcode);
        int ncl = 19;
        while (ncl > 4 && L.cllens[DEF_CLORDER[ncl - 1]] == 0) --ncl;
        ncl = def_uni(ncl);
        int hdr = 0;
        if (l < DEF_NCL) hdr = (int)L.clhist[l] * ((int)L.cllens[l] + (l == 16 ? 2 : (l == 17 ? 3 : (l == 18 ? 7 : 0))));
        const uint32_t dyn_bits = (uint32_t)(3 + 14 + 3 * ncl + def_wave_sum(hdr) + body);
        const uint32_t pos = o.sbits & 7u;
        const uint32_t pad = (0u - (pos + 3u)) & 7u;
        const uint32_t stored_bits = 3u + pad + 32u + 8u * (uint32_t)blen;
        const bool dynamic = dyn_bits < stored_bits;
        // the stage again: zero but for the bits it carried
        __syncthreads();
        for (int w = l; w < DEF_STAGE_DW; w += 64) L.stage[w] = w == 0 ? carry_dw : 0u;
        __syncthreads();
        // ---- the block's header
        if (dynamic) {
            uint32_t val = 0u, nb = 0u;
            if (l == 0) {
                val = fin | (2u << 1) | ((uint32_t)(nlit - 257) << 3) | (0u << 8) | ((uint32_t)(ncl - 4) << 13);
                nb = 17u;
            } else if (l <= ncl) {
                val = L.cllens[DEF_CLORDER[l - 1]];
                nb = 3u;
            }
            def_emit(L, o, val, nb);
            const int ni = (int)L.nitems;
            for (int i0 = 0; i0 < ni; i0 += 64) {
                val = 0u;
                nb = 0u;
                if (i0 + l < ni) {
                    const uint32_t it = L.items[i0 + l], s = it & 31u, c = L.clcode[s];
                    val = (c >> 4) | ((it >> 5) << (c & 15u));
                    nb = (c & 15u) + (s == 16u ? 2u : (s == 17u ? 3u : (s == 18u ? 7u : 0u)));
                }
                def_emit(L, o, val, nb);
            }
        } else {
            def_emit(L, o, fin, l == 0 ? 3u + pad : 0u);
            def_emit(L, o, (uint32_t)blen | (((uint32_t)blen ^ 0xffffu) << 16), l == 0 ? 32u : 0u);
        }
        def_flush(L, o);
        // ---- pass 2: the tokens' bits
        carry = -1;
        for (int t0 = 0; t0 < blen && !o.over; t0 += DEF_TILE) {
            DefLane v;
            def_load(blk, blen, t0, l, v);
            uint32_t pv[DEF_VPL], pn[DEF_VPL];
#pragma unroll
            for (int k = 0; k < DEF_VPL; ++k) { pv[k] = 0u; pn[k] = 0u; }
            if (dynamic) {
                const int start = def_run_start(v, l, carry);
                def_tokens(v, start, [&](int k, int sym, int xb, int xv, int lits) {
                    const uint32_t c = L.code[sym], len = c & 15u, bits = c >> 4;
                    if (lits == 0) {   // length code, extra bits, the one-bit distance code 0
                        pv[k] = bits | ((uint32_t)xv << len);
                        pn[k] = len + (uint32_t)xb + 1u;
                    } else if (lits == 1) {
                        pv[k] = bits;
                        pn[k] = len;
                    } else {
                        pv[k] = bits | (bits << len);
                        pn[k] = 2u * len;
                    }
                });
            } else {
#pragma unroll
                for (int k = 0; k < DEF_VPL; ++k) {
                    if (k < v.nval) {
                        pv[k] = (uint32_t)def_byte(v, k);
                        pn[k] = 8u;
                    }
                }
            }
            uint32_t tot = 0u;
#pragma unroll
            for (int k = 0; k < DEF_VPL; ++k) tot += pn[k];
            const int incl = wave_incl_scan_i((int)tot);
            uint32_t off = o.sbits + (uint32_t)incl - tot;
#pragma unroll
            for (int k = 0; k < DEF_VPL; ++k) {
                def_put(L, off, pv[k], pn[k]);
                off += pn[k];
            }
            o.sbits += (uint32_t)wave_last_i(incl);
            def_flush(L, o);
        }
        if (dynamic) {
            const uint32_t c = L.code[256];
            def_emit(L, o, c >> 4, l == 0 ? (c & 15u) : 0u);
            def_flush(L, o);   // (fewer than 32 bits stay: the next block's builder keeps stage[0] alone)
        }
    }
    // ---- the check value on the next byte boundary, most significant byte first
    o.sbits = (o.sbits + 7u) & ~7u;
    const uint32_t ad = (ad_b << 16) | ad_a;
    def_emit(L, o, __builtin_bswap32(ad), l == 0 ? 32u : 0u);
    def_flush(L, o);
    const uint32_t rem = o.sbits >> 3;   // 0 .. 3 bytes that fill no dword
    const uint32_t total = o.dw * 4u + rem;
    if (total > o.cap) o.over = true;
    if (!o.over && (uint32_t)l < rem) reinterpret_cast<uint8_t *>(o.dst + o.dw)[l] = (uint8_t)(L.stage[0] >> (8 * l));
    if (l == 0) {
        a.status[r] = o.over ? 1u : 0u;
        a.out_lengths[r] = o.over ? 0u : total;
    }
}

// ---- qts record mode: head | u64 len_raw_signal | signal | tail of every read, behind each other in an arena
// Head and tail are two sources of their own (base, 64-bit offset, length per record): the frames the host staged, where
// the tail lies directly behind the head (k_qts_record_sizes), or the record as k_inflate / k_zstd left it in the job's
// arena, where the old signal lies between them (k_qts_zrec_sizes).
struct AsmArgs {
    const uint8_t *head_src;       // head r: head_lengths[r] bytes at head_src + head_offsets[r]
    const uint64_t *head_offsets;  // n
    const uint32_t *head_lengths;  // n
    const uint8_t *tail_src;       // tail r: tail_lengths[r] bytes at tail_src + tail_offsets[r]
    const uint64_t *tail_offsets;  // n
    const uint32_t *tail_lengths;  // n
    const uint32_t *skip;          // n or null: non-zero: record r is not assembled (nothing of it is read or written)
    const uint8_t *signal;         // svb-zd blobs or int16 samples (bytes)
    const uint64_t *sig_offsets;   // n: offsets into signal, in units of sig_unit bytes
    const uint32_t *sig_counts;    // n: blob bytes / samples: the value of len_raw_signal
    uint32_t sig_unit;             // 1: blobs, 2: samples
    uint8_t *arena;
    const uint64_t *rec_offsets;   // n: where record r goes
    uint32_t n;
};
__device__ __forceinline__ uint32_t qts_deflate_cap(uint32_t len) {   // what k_deflate may need for len bytes
    return len + 5u * (len ? (len + DEF_BLOCK - 1u) / DEF_BLOCK : 1u) + 6u;
}
// staged frames (frame r: head_lengths[r] bytes of head, then the tail, at frame_offsets[r]): the two sources,
// rec_lengths[r] = frame + 8 + signal bytes; caps[r] = what k_deflate may need for it
__global__ __launch_bounds__(256) void k_qts_record_sizes(const uint32_t *frame_offsets, const uint32_t *head_lengths,
                                                          const uint32_t *sig_counts, uint32_t sig_unit, uint32_t n,
                                                          uint64_t *head_offsets, uint64_t *tail_offsets, uint32_t *tail_lengths,
                                                          uint32_t *rec_lengths, uint32_t *caps) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const uint32_t f0 = frame_offsets[r], flen = frame_offsets[r + 1] - f0, head = head_lengths[r];
    head_offsets[r] = f0;
    tail_offsets[r] = (uint64_t)f0 + head;
    tail_lengths[r] = flen - head;
    const uint32_t len = flen + 8u + sig_counts[r] * sig_unit;
    rec_lengths[r] = len;
    caps[r] = qts_deflate_cap(len);
}
// The same for records inflated on the device (SGK_SIGNAL_ZREC): record r lies at rec_offsets[r] of the arena with room
// rec_caps[r], its old svb-zd blob at sig_offsets[r] (arena offset) with sig_lengths[r] bytes; inflated_lengths[r] is what
// it inflated to.  head = [0, blob - 8), tail = [blob end, inflated length).  A record whose inflate status or tail
// status (null: the batch has no column table) is non-zero has an inflated length nobody vouches for -- 0, short of the
// signal's end, or a word that lies behind the room: it gets length 0 everywhere and bad[r] = 2, as does one whose length
// does not hold its head and signal or exceeds its room.  new_counts[r]: the bytes of the new blob.
struct ZrecSizeArgs {
    const uint64_t *rec_offsets;
    const uint32_t *rec_caps, *inflated_lengths;
    const uint64_t *sig_offsets;
    const uint32_t *sig_lengths, *inflate_status, *tail_status, *new_counts;
    uint32_t n;
    uint64_t *head_offsets, *tail_offsets;
    uint32_t *head_lengths, *tail_lengths, *rec_lengths, *caps, *bad;
};
__global__ __launch_bounds__(256) void k_qts_zrec_sizes(ZrecSizeArgs a) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.n) return;
    const uint64_t ro = a.rec_offsets[r];
    const uint64_t so = a.sig_offsets[r] - ro, end = so + a.sig_lengths[r];   // relative to the record
    bool ok = a.inflate_status[r] == 0u && (!a.tail_status || a.tail_status[r] == 0u);
    uint32_t il = 0u;
    if (ok) {
        il = a.inflated_lengths[r];
        ok = so >= 8u && il <= a.rec_caps[r] && (uint64_t)il >= end;
    }
    const uint32_t head = ok ? (uint32_t)so - 8u : 0u, tail = ok ? il - (uint32_t)end : 0u;
    const uint32_t len = ok ? head + 8u + a.new_counts[r] + tail : 0u;
    a.head_offsets[r] = ro;
    a.head_lengths[r] = head;
    a.tail_offsets[r] = ok ? ro + end : ro;
    a.tail_lengths[r] = tail;
    a.rec_lengths[r] = len;
    a.caps[r] = qts_deflate_cap(len);
    a.bad[r] = ok ? 0u : 2u;
}
// after k_deflate: the records k_qts_zrec_sizes gave up on report their status and no stream (k_deflate made an empty one)
__global__ __launch_bounds__(256) void k_qts_zrec_mark(const uint32_t *bad, uint32_t n, uint32_t *out_lengths, uint32_t *status) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n || bad[r] == 0u) return;
    out_lengths[r] = 0u;
    status[r] = bad[r];
}
__global__ __launch_bounds__(256) void k_qts_assemble(AsmArgs a) {
    const uint32_t r = blockIdx.x;
    if (r >= a.n) return;
    if (a.skip && a.skip[r] != 0u) return;
    const uint32_t head = a.head_lengths[r], tail = a.tail_lengths[r];
    const uint32_t cnt = a.sig_counts[r], sbytes = cnt * a.sig_unit;
    const uint8_t *hs = a.head_src + a.head_offsets[r];
    const uint8_t *ts = a.tail_src + a.tail_offsets[r];
    const uint8_t *sg = a.signal + a.sig_offsets[r] * a.sig_unit;
    uint8_t *dst = a.arena + a.rec_offsets[r];
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < head; i += 256u) dst[i] = hs[i];
    if (t < 8u) dst[head + t] = t < 4u ? (uint8_t)(cnt >> (8u * t)) : (uint8_t)0;
    uint8_t *sd = dst + head + 8u;
    // the signal: whole aligned dwords of the destination where the source allows it
    const uint32_t lead = (uint32_t)((4u - (reinterpret_cast<uintptr_t>(sd) & 3u)) & 3u);
    if (sbytes >= 64u && ((reinterpret_cast<uintptr_t>(sg) + lead) & 3u) == 0) {
        for (uint32_t i = t; i < lead; i += 256u) sd[i] = sg[i];
        const uint32_t ndw = (sbytes - lead) >> 2;
        const uint32_t *s32 = reinterpret_cast<const uint32_t *>(sg + lead);
        uint32_t *d32 = reinterpret_cast<uint32_t *>(sd + lead);
        for (uint32_t i = t; i < ndw; i += 256u) d32[i] = s32[i];
        for (uint32_t i = lead + ndw * 4u + t; i < sbytes; i += 256u) sd[i] = sg[i];
    } else {
        for (uint32_t i = t; i < sbytes; i += 256u) sd[i] = sg[i];
    }
    uint8_t *td = sd + sbytes;
    for (uint32_t i = t; i < tail; i += 256u) td[i] = ts[i];
}
// bytes [src_offsets[r], + lengths[r]) of src -> dst + dst_offsets[r] (both 16-byte aligned offsets)
__global__ __launch_bounds__(256) void k_bytes_gather(const uint8_t *src, const uint64_t *src_offsets, const uint32_t *lengths,
                                                      uint32_t n, uint8_t *dst, const uint64_t *dst_offsets) {
    const uint32_t r = blockIdx.x;
    if (r >= n) return;
    const uint32_t len = lengths[r], nq = len >> 4;
    const uint8_t *s = src + src_offsets[r];
    uint8_t *d = dst + dst_offsets[r];
    for (uint32_t i = threadIdx.x; i < nq; i += 256u) reinterpret_cast<uint4 *>(d)[i] = reinterpret_cast<const uint4 *>(s)[i];
    for (uint32_t i = nq * 16u + threadIdx.x; i < len; i += 256u) d[i] = s[i];
}

int launch_qts_record_sizes(const uint32_t *frame_offsets, const uint32_t *head_lengths, const uint32_t *sig_counts,
                            uint32_t sig_unit, uint32_t n, uint64_t *head_offsets, uint64_t *tail_offsets,
                            uint32_t *tail_lengths, uint32_t *rec_lengths, uint32_t *caps, hipStream_t st) {
    if (n == 0) return SGK_OK;
    SGK_LAUNCH_UNTIMED(k_qts_record_sizes, (n + 255u) / 256u, 256, st, frame_offsets, head_lengths, sig_counts, sig_unit, n,
                       head_offsets, tail_offsets, tail_lengths, rec_lengths, caps);
    return SGK_OK;
}
int launch_qts_zrec_sizes(const uint64_t *rec_offsets, const uint32_t *rec_caps, const uint32_t *inflated_lengths,
                          const uint64_t *sig_offsets, const uint32_t *sig_lengths, const uint32_t *inflate_status,
                          const uint32_t *tail_status, const uint32_t *new_counts, uint32_t n, uint64_t *head_offsets,
                          uint32_t *head_lengths, uint64_t *tail_offsets, uint32_t *tail_lengths, uint32_t *rec_lengths,
                          uint32_t *caps, uint32_t *bad, hipStream_t st) {
    if (n == 0) return SGK_OK;
    ZrecSizeArgs a = {rec_offsets, rec_caps, inflated_lengths, sig_offsets, sig_lengths, inflate_status, tail_status, new_counts, n,
                      head_offsets, tail_offsets, head_lengths, tail_lengths, rec_lengths, caps, bad};
    SGK_LAUNCH_UNTIMED(k_qts_zrec_sizes, (n + 255u) / 256u, 256, st, a);
    return SGK_OK;
}
int launch_qts_zrec_mark(const uint32_t *bad, uint32_t n, uint32_t *out_lengths, uint32_t *status, hipStream_t st) {
    if (n == 0) return SGK_OK;
    SGK_LAUNCH_UNTIMED(k_qts_zrec_mark, (n + 255u) / 256u, 256, st, bad, n, out_lengths, status);
    return SGK_OK;
}
int launch_qts_assemble(const uint8_t *head_src, const uint64_t *head_offsets, const uint32_t *head_lengths,
                        const uint8_t *tail_src, const uint64_t *tail_offsets, const uint32_t *tail_lengths, const uint32_t *skip,
                        const uint8_t *signal, const uint64_t *sig_offsets, const uint32_t *sig_counts, uint32_t sig_unit,
                        uint8_t *arena, const uint64_t *rec_offsets, uint32_t n, hipStream_t st) {
    if (n == 0) return SGK_OK;
    AsmArgs a = {head_src, head_offsets, head_lengths, tail_src, tail_offsets, tail_lengths, skip,
                 signal, sig_offsets, sig_counts, sig_unit, arena, rec_offsets, n};
    SGK_LAUNCH("k_qts_assemble", k_qts_assemble, n, 256, st, a);
    return SGK_OK;
}
int launch_bytes_gather(const uint8_t *src, const uint64_t *src_offsets, const uint32_t *lengths, uint32_t n, uint8_t *dst,
                        const uint64_t *dst_offsets, hipStream_t st) {
    if (n == 0) return SGK_OK;
    SGK_LAUNCH("k_bytes_gather", k_bytes_gather, n, 256, st, src, src_offsets, lengths, n, dst, dst_offsets);
    return SGK_OK;
}

}  // namespace sgk

extern "C" uint32_t sgk_deflate_block_bytes(void) { return (uint32_t)sgk::DEF_BLOCK; }

extern "C" uint64_t sgk_deflate_bound(uint64_t n) {
    const uint64_t per = sgk::DEF_BLOCK < 65535 ? sgk::DEF_BLOCK : 65535;
    const uint64_t blocks = n ? (n + per - 1) / per : 1;
    return n + 5 * blocks + 6;
}

namespace sgk {
// status[0] |= 1 if a stream is too long for 32-bit bit positions
__global__ __launch_bounds__(256) void k_deflate_check(const uint32_t *in_lengths, uint32_t n, uint32_t *flag) {
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < n; r += gridDim.x * 256u)
        if (in_lengths[r] >= (1u << 29)) atomicOr(flag, 1u);
}
int launch_deflate(const DefArgs &a, hipStream_t st) {
    if (a.n == 0) return SGK_OK;
    SGK_LAUNCH("k_deflate", k_deflate, a.n, 64, st, a);
    return SGK_OK;
}
int launch_deflate_unchecked(const uint8_t *in, const uint64_t *in_offsets, const uint32_t *in_lengths, uint32_t n, uint8_t *out,
                             const uint64_t *out_offsets, const uint32_t *out_caps, uint32_t *out_lengths, uint32_t *status,
                             hipStream_t st) {   // (the job's records: their lengths are bounded on the host)
    DefArgs a;
    a.in = in; a.in_offsets = in_offsets; a.in_lengths = in_lengths; a.out = out; a.out_offsets = out_offsets;
    a.out_caps = out_caps; a.out_lengths = out_lengths; a.status = status; a.n = n;
    return launch_deflate(a, st);
}
}  // namespace sgk

extern "C" int sgk_deflate(const uint8_t *in, const uint64_t *in_offsets, const uint32_t *in_lengths, uint32_t n, uint8_t *out,
                           const uint64_t *out_offsets, const uint32_t *out_caps, uint32_t *out_lengths, uint32_t *status,
                           void *stream) {
    if (n == 0) return SGK_OK;
    if (!in || !in_offsets || !in_lengths || !out || !out_offsets || !out_caps || !out_lengths || !status) return SGK_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(out) & 15u) return SGK_ERR_ALIGN;
    sgk::DefArgs a;
    a.in = in; a.in_offsets = in_offsets; a.in_lengths = in_lengths; a.out = out; a.out_offsets = out_offsets;
    a.out_caps = out_caps; a.out_lengths = out_lengths; a.status = status; a.n = n;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // positions are 32-bit: a stream of 2^29 bytes or more is refused before anything is written (status[0] is the
    // flag's place until k_deflate writes the statuses)
    uint32_t flag = 0u;
    SGK_HIP_TRY(hipMemsetAsync(status, 0, 4, st));
    const uint32_t grid = (n + 255u) / 256u < 1024u ? (n + 255u) / 256u : 1024u;
    SGK_LAUNCH_UNTIMED(sgk::k_deflate_check, grid, 256, st, in_lengths, n, status);
    SGK_HIP_TRY(hipMemcpyAsync(&flag, status, 4, hipMemcpyDeviceToHost, st));
    SGK_HIP_TRY(hipStreamSynchronize(st));
    if (flag) return SGK_ERR_ARG;
    return sgk::launch_deflate(a, st);
}
