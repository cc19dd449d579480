// ss_kernels.hip -- `ss paf2tsv`: the ss:Z: strings of a resquiggle PAF to one TSV row per k-mer (sgk_ss_*; DESIGN 3.11;
// the reference: src/ss.c:124-197, one record at a time through atoi and printf).
//
// Decode (k_ss_decode): one wavefront per span of a record, in the shape of k_sigtext_decode.  Per tile of 64 lanes x 16
// bytes every lane loads one aligned 16-byte word.  A token <digits><op> belongs to the lane that holds its op; a valid
// token is at most 11 bytes long, so it began in this lane or the previous one: every lane also gets the previous
// lane's upper 12 bytes (three DPP wave shifts; lane 0 takes them from the previous tile's lane 63, carried in three
// wave-uniform registers).  Twelve bytes are enough to see an eleventh digit in front of an op, which is an error.
// The lane walks its 12 + 16 bytes with a small integer automaton and sums what its own ops add to i_raw and i_k; wave
// scans of the sums and a wave-uniform carry across tiles give every ',' its i_raw and i_k.  Only a tile whose k-mer
// range meets the span's walks a second time, to store.  No LDS, integer arithmetic and vector stores only.
//
// Sums cannot wrap: a number is held in 32 bits with an overflow flag, a lane's sum of at most 8 numbers in 64 bits,
// clamped to 2^31 before the scan; the scan runs on the clamped value's 16-bit halves (two int scans, at most 64 x 2^16
// each); the carry is clamped to 2^31 after every tile.  All addends are non-negative, so a clamp anywhere leaves the
// final total above INT32_MAX, which is status 5.
//
// Text (k_ss_measure / k_ss_write): the tile list, the scan and the staged 16-byte stores are text_tiles.h; a span is a
// row of the tile list, a k-mer an item, the numbers text_format.h.  A row repeats the read id, so a tile of 256 rows is
// 256 x (id + up to 35) bytes: the LDS image is 24 KiB, which holds ids of up to 61 bytes with the longest numbers (a
// 36-byte UUID gives at most 18 KiB) and lets six workgroups share a CU's 160 KiB.  A tile that does not fit (long ids)
// is written straight to global memory, every lane its own row.
#include "sgk_common.h"
#include "text_format.h"
#include "text_tiles.h"

namespace sgk {

constexpr uint32_t SS_PAD = 0x01010101u;  // bytes outside the string: they end a token's look-back and start nothing
constexpr uint32_t SS_NONE = 0xffffffffu;
constexpr int64_t SS_SAT = 0x80000000ll;  // INT32_MAX + 1: where sums are clamped
constexpr uint32_t SS_STAGE = 24576;      // bytes of a tile's LDS image

struct SsArgs : TileList {  // (n_rows = the batch's spans)
    const uint8_t *ss;
    uint64_t n_ss_bytes;
    const sgk_ss_record_t *records;
    const sgk_ss_span_t *spans;
    uint32_t n_records, n_spans;
    const uint64_t *out_offsets;
    int32_t *pairs;
    uint32_t *status;
    int32_t *ends;
    const uint8_t *id_bytes;
    const uint32_t *id_offs;
    uint64_t *row_offsets;  // n_spans + 1 (measure)
    uint8_t *text;          // (write)
    uint64_t text_cap;
};

// non-zero iff a byte of w is 0x01
__device__ inline uint32_t ss_has_pad(uint32_t w) {
    const uint32_t x = w ^ SS_PAD;
    return (x - 0x01010101u) & ~x & 0x80808080u;
}
// the bytes of word w at stream positions p .. p + 3 outside [lo, hi) become pad bytes; a pad byte's value inside the
// string becomes 0x02, a byte like any other: invalid
__device__ inline uint32_t ss_clip(uint32_t w, uint64_t p, uint64_t lo, uint64_t hi) {
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint64_t q = p + (uint64_t)j;
        uint32_t c = (w >> (8 * j)) & 0xffu;
        if (q < lo || q >= hi) c = 0x01u;
        else if (c == 0x01u) c = 0x02u;
        out |= c << (8 * j);
    }
    return out;
}
__device__ inline uint32_t wave_min_u(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}

struct SsLane {
    int64_t raw, k;       // what the lane's own ops add (or, when storing, the running i_raw / i_k)
    uint32_t e1, e2, rng; // lowest string position of a status 1 / status 2 byte; a number out of range
};

// The automaton over the 12 look-back bytes (b[0..2]) and the lane's own 16 (b[3..6]).  spos: string position of the
// lane's own byte 0 (modulo 2^32: only used for bytes inside the string).  STORE: L.raw / L.k come in as i_raw / i_k in
// front of the lane's first own op and every ',' whose k-mer lies in [base_k, base_k + count) stores its pair.
template <bool STORE>
__device__ inline void ss_walk(const uint32_t (&b)[7], uint32_t spos, SsLane &L, int64_t base_k, uint32_t count, int32_t *out) {
    uint32_t val = 0, ndig = 0, over = 0;
#pragma unroll
    for (int j = 0; j < 28; ++j) {
        const uint32_t c = (b[j >> 2] >> (8 * (j & 3))) & 0xffu;
        const uint32_t d = c - (uint32_t)'0';
        const bool own = j >= 12;
        if (d <= 9u) {
            over |= (uint32_t)((val > 214748364u) | ((val == 214748364u) & (d > 7u)));
            val = val * 10u + d;
            ++ndig;
        } else {
            if (c == (uint32_t)',' || c == (uint32_t)'I' || c == (uint32_t)'D') {
                if (own) {
                    const uint32_t pos = spos + (uint32_t)(j - 12);
                    if (!STORE) {
                        if (ndig == 0u) L.e1 = pos < L.e1 ? pos : L.e1;
                        if (ndig > 10u || over) L.rng = 1u;
                    }
                    const int64_t n = (int64_t)val;
                    if (c == (uint32_t)'I') {
                        L.raw += n;
                    } else if (c == (uint32_t)'D') {
                        L.k += n;
                    } else {
                        if (STORE) {
                            const int64_t jj = L.k - base_k;
                            if (jj >= 0 && jj < (int64_t)count)
                                *reinterpret_cast<int2 *>(out + 2 * jj) = make_int2((int32_t)L.raw, (int32_t)(L.raw + n));
                        }
                        L.raw += n;
                        L.k += 1;
                    }
                }
            } else if (!STORE && own && c != 0x01u) {
                const uint32_t pos = spos + (uint32_t)(j - 12);
                L.e2 = pos < L.e2 ? pos : L.e2;
            }
            val = 0;
            ndig = 0;
            over = 0;
        }
    }
}

__device__ inline int64_t ss_clamp(int64_t v) { return v < SS_SAT ? v : SS_SAT; }

__global__ __launch_bounds__(64) void k_ss_decode(SsArgs a) {
    const uint32_t s = blockIdx.x;
    const int l = lane_id();
    sgk_ss_span_t sp;
    if (a.spans) {
        sp = a.spans[s];
    } else {
        sp.record = s;
        sp.first = 0;
        sp.count = 0;
    }
    if (sp.record >= a.n_records) {  // not a record of this batch: nothing is read or stored
        if (l == 0) {
            a.status[s] = SS_NONE;
            a.ends[2 * (size_t)s] = -1;
            a.ends[2 * (size_t)s + 1] = -1;
        }
        return;
    }
    const sgk_ss_record_t rec = a.records[sp.record];
    const uint64_t lead = rec.ss_offset & 15u;  // stream position p is byte p from the aligned word in front of the string
    const uint64_t w0 = rec.ss_offset >> 4;
    const uint64_t nwords = (a.n_ss_bytes + 15u) >> 4;  // 16-byte words of the buffer
    const uint64_t end = lead + (uint64_t)rec.ss_len;
    const uint64_t ntiles = rec.ss_len ? (end + 1023u) >> 10 : 0u;
    const uint4 *base = reinterpret_cast<const uint4 *>(a.ss);
    const int64_t base_k = (int64_t)rec.st_k + (int64_t)sp.first;
    const int64_t lim_k = base_k + (int64_t)sp.count;
    int32_t *out = sp.count ? a.pairs + 2 * a.out_offsets[s] : nullptr;
    int64_t carry_raw = rec.start_raw, carry_k = rec.st_k;  // i_raw / i_k in front of this tile (wave-uniform)
    uint32_t cy = SS_PAD, cz = SS_PAD, cw = SS_PAD;         // upper 12 bytes of the previous tile's lane 63
    uint32_t e1 = SS_NONE, e2 = SS_NONE, rng = 0;
    for (uint64_t t = 0; t < ntiles; ++t) {
        const uint64_t wi = t * 64u + (uint64_t)l;  // this lane's word of the stream
        const uint64_t p0 = wi << 4;
        uint4 w = make_uint4(SS_PAD, SS_PAD, SS_PAD, SS_PAD);
        if (p0 < end && w0 + wi < nwords) w = base[w0 + wi];
        if (p0 < lead || p0 + 16u > end || (ss_has_pad(w.x) | ss_has_pad(w.y) | ss_has_pad(w.z) | ss_has_pad(w.w))) {
            w.x = ss_clip(w.x, p0, lead, end);
            w.y = ss_clip(w.y, p0 + 4u, lead, end);
            w.z = ss_clip(w.z, p0 + 8u, lead, end);
            w.w = ss_clip(w.w, p0 + 12u, lead, end);
        }
        const uint32_t b[7] = {(uint32_t)wave_shr1_i((int)w.y, (int)cy), (uint32_t)wave_shr1_i((int)w.z, (int)cz),
                               (uint32_t)wave_shr1_i((int)w.w, (int)cw), w.x, w.y, w.z, w.w};
        const uint32_t spos = (uint32_t)(p0 - lead);
        SsLane L = {0, 0, e1, e2, rng};
        ss_walk<false>(b, spos, L, 0, 0u, nullptr);
        e1 = L.e1;
        e2 = L.e2;
        rng = L.rng;
        const int64_t vr = ss_clamp(L.raw), vk = ss_clamp(L.k);  // <= 2^31: halves of at most 2^15 and 2^16 - 1
        const int r_lo = wave_incl_scan_i((int)(vr & 0xffff)), r_hi = wave_incl_scan_i((int)(vr >> 16));
        const int k_lo = wave_incl_scan_i((int)(vk & 0xffff)), k_hi = wave_incl_scan_i((int)(vk >> 16));
        const int64_t tot_r = ((int64_t)wave_last_i(r_hi) << 16) + (int64_t)wave_last_i(r_lo);
        const int64_t tot_k = ((int64_t)wave_last_i(k_hi) << 16) + (int64_t)wave_last_i(k_lo);
        if (sp.count && carry_k < lim_k && carry_k + tot_k > base_k) {  // (wave-uniform) a ',' of this tile may be the span's
            SsLane W = {carry_raw + (((int64_t)r_hi << 16) + (int64_t)r_lo - vr), carry_k + (((int64_t)k_hi << 16) + (int64_t)k_lo - vk),
                        0u, 0u, 0u};
            ss_walk<true>(b, spos, W, base_k, sp.count, out);
        }
        carry_raw = ss_clamp(carry_raw + tot_r);
        carry_k = ss_clamp(carry_k + tot_k);
        cy = (uint32_t)__builtin_amdgcn_readlane((int)w.y, 63);
        cz = (uint32_t)__builtin_amdgcn_readlane((int)w.z, 63);
        cw = (uint32_t)__builtin_amdgcn_readlane((int)w.w, 63);
    }
    e1 = wave_min_u(e1);
    e2 = wave_min_u(e2);
    const int any_rng = __any((int)rng);
    if (l == 0) {
        uint32_t st;
        if (e1 != SS_NONE || e2 != SS_NONE) st = e1 < e2 ? 1u : 2u;
        else if (any_rng || carry_raw > 0x7fffffffll || carry_k > 0x7fffffffll) st = 5u;
        else if (carry_raw != (int64_t)rec.end_raw) st = 3u;
        else if (carry_k != (int64_t)rec.end_k) st = 4u;
        else st = 0u;
        const bool no_ends = st == 1u || st == 2u || st == 5u;
        a.status[s] = st;
        a.ends[2 * (size_t)s] = no_ends ? -1 : (int32_t)carry_raw;
        a.ends[2 * (size_t)s + 1] = no_ends ? -1 : (int32_t)carry_k;
    }
}

// ---- text
__global__ __launch_bounds__(1024) void k_ss_tiles(SsArgs a) {
    text_tiles_body(a, [&](uint32_t s) { return a.spans[s].count; });
}
__global__ __launch_bounds__(1024) void k_ss_scan(SsArgs a) { text_scan_body(a, a.row_offsets); }

struct SsTile {
    uint32_t nt;        // the tile's k-mers
    uint32_t idl;
    const uint8_t *id;
    const int32_t *pr;  // the tile's first pair
    int64_t k0;         // its first k-mer
    int64_t tlen;
    bool rna;
};

__device__ inline SsTile ss_tile(const SsArgs &a, uint32_t t) {
    const uint32_t s = text_tile_row(a, t);
    const sgk_ss_span_t sp = a.spans[s];
    SsTile c;
    c.nt = 0;
    c.idl = 0;
    c.id = a.id_bytes;
    c.pr = a.pairs;
    c.k0 = 0;
    c.tlen = 0;
    c.rna = false;
    if (sp.record >= a.n_records) return c;
    const sgk_ss_record_t rec = a.records[sp.record];
    const uint32_t j0 = (t - a.tile_first[s]) * TEXT_TILE;
    c.nt = sp.count - j0 < (uint32_t)TEXT_TILE ? sp.count - j0 : (uint32_t)TEXT_TILE;
    c.idl = a.id_offs[rec.id + 1] - a.id_offs[rec.id];
    c.id = a.id_bytes + a.id_offs[rec.id];
    c.pr = a.pairs + 2 * (a.out_offsets[s] + j0);
    c.k0 = (int64_t)rec.st_k + (int64_t)sp.first + (int64_t)j0;
    c.tlen = rec.tlen;
    c.rna = rec.rna != 0;
    return c;
}

struct SsItem {
    int64_t idx;
    int32_t a, b;
    uint32_t len;
};
__device__ inline SsItem ss_item(const SsTile &c) {
    SsItem it = {0, -1, -1, 0u};
    if (threadIdx.x >= c.nt) return it;
    const int64_t i = c.k0 + (int64_t)threadIdx.x;
    it.idx = c.rna ? c.tlen - i - 1 : i;
    const int2 p = *reinterpret_cast<const int2 *>(c.pr + 2 * threadIdx.x);
    it.a = p.x;
    it.b = p.y;
    it.len = c.idl + 4u + (uint32_t)sgk_tf_i64_len(it.idx) +
             (it.a == -1 ? 2u : (uint32_t)(sgk_tf_i64_len(it.a) + sgk_tf_i64_len(it.b)));
    return it;
}
__device__ inline void ss_item_emit(const SsTile &c, const SsItem &it, char *p) {
    for (uint32_t k = 0; k < c.idl; ++k) p[k] = (char)c.id[k];
    p += c.idl;
    *p++ = '\t';
    p += sgk_tf_i64(p, it.idx);
    *p++ = '\t';
    if (it.a == -1) {
        *p++ = '.';
        *p++ = '\t';
        *p++ = '.';
    } else {
        p += sgk_tf_i64(p, it.a);
        *p++ = '\t';
        p += sgk_tf_i64(p, it.b);
    }
    *p = '\n';
}

__global__ __launch_bounds__(TEXT_TILE) void k_ss_measure(SsArgs a) {
    __shared__ uint32_t wave_tot[TEXT_TILE / 64];
    const uint32_t n_tiles = a.hdr->n_tiles;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const SsTile c = ss_tile(a, t);
        const SsItem it = ss_item(c);
        uint32_t my_off;
        const uint32_t total = text_lane_offsets(it.len, 0u, wave_tot, my_off);
        if (threadIdx.x == 0) a.tile_bytes[t] = total;
        __syncthreads();  // wave_tot is reused by the next tile
    }
}

__global__ __launch_bounds__(TEXT_TILE) void k_ss_write(SsArgs a) {
    __shared__ uint32_t wave_tot[TEXT_TILE / 64];
    __shared__ __attribute__((aligned(16))) char stage[SS_STAGE + 16];
    const uint32_t n_tiles = a.hdr->n_tiles;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const SsTile c = ss_tile(a, t);
        const SsItem it = ss_item(c);
        uint32_t my_off;
        const uint32_t total = text_lane_offsets(it.len, 0u, wave_tot, my_off);
        const uint64_t b0 = a.tile_off[t];
        if (b0 + total > a.text_cap) {  // (workgroup-uniform) nothing of this tile is written
            if (threadIdx.x == 0) atomicOr(&a.hdr->flags, TEXT_FLAG_OVERFLOW);
        } else if (total <= SS_STAGE) {
            uint8_t *dst = a.text + b0;
            char *img = stage + text_image_align(dst);
            if (it.len) ss_item_emit(c, it, img + my_off);
            __syncthreads();
            text_image_flush(dst, img, total);
        } else {  // long ids: every lane writes its own row straight to global memory
            if (it.len) ss_item_emit(c, it, reinterpret_cast<char *>(a.text + b0) + my_off);
        }
        __syncthreads();  // the image and wave_tot are reused by the next tile
    }
}

static int ss_batch_check(const sgk_ss_batch_t *b) {
    if (!b) return SGK_ERR_ARG;
    if (b->n_records && !b->records) return SGK_ERR_ARG;
    if (b->n_ss_bytes && !b->ss) return SGK_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(b->ss) & 15u) return SGK_ERR_ARG;
    return SGK_OK;
}

static void ss_fill(const sgk_ss_batch_t *b, SsArgs *a) {
    memset(a, 0, sizeof *a);
    a->ss = b->ss;
    a->n_ss_bytes = b->n_ss_bytes;
    a->records = b->records;
    a->spans = b->spans;
    a->n_records = b->n_records;
    a->n_spans = b->spans ? b->n_spans : b->n_records;
}

static int ss_text_args(const sgk_ss_batch_t *b, const uint64_t *out_offsets, const int32_t *pairs, const sgk_text_ids_t *ids,
                        void *ws, size_t ws_bytes, SsArgs *a) {
    const int rc = ss_batch_check(b);
    if (rc != SGK_OK) return rc;
    if (sgk_device_count() <= 0) return SGK_ERR_NODEVICE;
    SGK_TRY(text_ws_check(ws, ws_bytes, 0));
    if (b->n_spans && (!b->spans || !ids || !ids->bytes || !ids->offsets || !out_offsets || !pairs)) return SGK_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(pairs) & 7u) return SGK_ERR_ARG;
    ss_fill(b, a);
    a->n_spans = b->n_spans;
    if (!tile_list_carve(ws, ws_bytes, b->n_spans, a)) return SGK_ERR_WORKSPACE;
    a->out_offsets = out_offsets;
    a->pairs = const_cast<int32_t *>(pairs);
    a->id_bytes = ids ? ids->bytes : nullptr;
    a->id_offs = ids ? ids->offsets : nullptr;
    return SGK_OK;
}

}  // namespace sgk

using namespace sgk;

extern "C" {

int sgk_ss_decode(const sgk_ss_batch_t *b, const uint64_t *out_offsets, int32_t *pairs, uint32_t *status, int32_t *ends,
                  void *stream) {
    const int rc = ss_batch_check(b);
    if (rc != SGK_OK) return rc;
    if (sgk_device_count() <= 0) return SGK_ERR_NODEVICE;
    SsArgs a;
    ss_fill(b, &a);
    if (a.n_spans == 0) return SGK_OK;
    if (!status || !ends) return SGK_ERR_ARG;
    if (b->spans && (!out_offsets || !pairs)) return SGK_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(pairs) & 7u) return SGK_ERR_ARG;
    a.out_offsets = out_offsets;
    a.pairs = pairs;
    a.status = status;
    a.ends = ends;
    SGK_LAUNCH("k_ss_decode", k_ss_decode, a.n_spans, 64, static_cast<hipStream_t>(stream), a);
    return SGK_OK;
}

size_t sgk_ss_text_workspace_bytes(uint32_t n_spans, uint64_t n_rows_capacity) {
    return round_up(tile_list_bytes(n_spans, n_rows_capacity) + 64, 16);
}

int sgk_ss_text_measure(const sgk_ss_batch_t *b, const uint64_t *out_offsets, const int32_t *pairs, const sgk_text_ids_t *ids,
                        uint64_t *row_offsets, void *ws, size_t ws_bytes, void *stream) {
    SsArgs a;
    const int rc = ss_text_args(b, out_offsets, pairs, ids, ws, ws_bytes, &a);
    if (rc != SGK_OK) return rc;
    if (!row_offsets) return SGK_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    a.row_offsets = row_offsets;
    const uint32_t grid = text_grid(a);
    SGK_LAUNCH("k_ss_tiles", k_ss_tiles, 1, 1024, st, a);
    SGK_LAUNCH("k_ss_measure", k_ss_measure, grid, TEXT_TILE, st, a);
    SGK_LAUNCH("k_ss_scan", k_ss_scan, 1, 1024, st, a);
    return SGK_OK;
}

int sgk_ss_text_write(const sgk_ss_batch_t *b, const uint64_t *out_offsets, const int32_t *pairs, const sgk_text_ids_t *ids,
                      uint8_t *text, uint64_t text_capacity, void *ws, size_t ws_bytes, void *stream) {
    SsArgs a;
    const int rc = ss_text_args(b, out_offsets, pairs, ids, ws, ws_bytes, &a);
    if (rc != SGK_OK) return rc;
    if (!text && text_capacity) return SGK_ERR_ARG;
    a.text = text;
    a.text_cap = text_capacity;
    const uint32_t grid = text_grid(a);
    SGK_LAUNCH("k_ss_write", k_ss_write, grid, TEXT_TILE, static_cast<hipStream_t>(stream), a);
    return SGK_OK;
}

}  // extern "C"
