// text_kernels.hip -- the TSV rows of `pa`, `event` and `event -c` written on the device (sgk_text_*).
//
// The three subtools whose output is large print one number per sample (pa: ~10 bytes of text per 2-byte sample)
// or per event; formatting on the host means moving the binary results over PCIe and then turning them into
// characters on a handful of threads.  Here the batch's whole stdout body (header line excluded) is produced as one
// dense byte range in file order, byte for byte what the reference's printf calls give (src/cfunc.c:16-61, 85-102):
//
//   pa             id \t len \t v0,v1,...,v(len-1) \n                  (a read of 0 samples: id \t 0 \t \n)
//   event          id \t j \t start \t start+(int)length \t mean \t stdv \n  per event, then one empty line per read
//   event -c       id \t len \t start0 \t end \t n \t l0,l1,...  \n    (zero lengths are skipped, the comma only when
//                                                                       j < n-1; a read without events: .\t.\t.\t.)
//
// A byte's position depends on every byte in front of it, so there are two passes over the items with a scan between:
//
//   k_text_tiles    the items of every read (samples; events that fitted their slots) are cut into tiles of 256;
//                   a scan of the reads' tile counts maps tiles to reads (a read has at least one tile: its fixed
//                   parts -- id, length, the line end -- belong to its first and last tile)
//   k_text_measure  byte count of every tile; nothing is written but the count
//   k_text_scan     tile counts -> 64-bit byte offsets; row_offsets[r] is the offset of read r's first tile
//   k_text_write    every tile computes its items' characters again and stores them at its offset
//
// Work is divided by items, not by reads: a read of 1.6e6 samples among short ones is 6 250 tiles like any others.
// The number of events is known only on the device, so the grid is sized from the capacity the workspace was sized
// for and strides over the tile list the device built; there is no host round trip between the event kernels and
// these.  pa text is made from the int16 samples with to_pa() in both passes: the float array never exists.
//
// Inside a tile: one item per lane; per-lane byte counts (the length-only forms of text_format.h) -> inclusive wave
// scan with DPP -> the four waves' totals through LDS -> every lane writes its characters into an LDS image of the
// tile's byte range -> the image leaves as 16-byte stores.  The image is laid out at the same offset modulo 16 as
// its place in global memory, so both sides of the body are aligned; the up to 15 bytes in front of the first
// aligned word and behind the last one go out as byte stores.  Two tiles may share a 16-byte word of the output;
// neither ever reads or rewrites a byte of the other.  A tile that does not fit the image (ids of thousands of
// bytes in every `event` row) writes its characters straight to global memory, each lane its own bytes.
//
// The tile list, the scan and the staged stores do not depend on the grammar: they are text_tiles.h, which
// sref_kernels.hip uses for a fourth grammar.
//
// text_capacity is checked on the device (the call is asynchronous and the total is not known on the host): a tile
// that would end behind it writes nothing and raises TEXT_FLAG_OVERFLOW in the workspace's header.
#include "sgk_common.h"
#include "text_format.h"
#include "text_tiles.h"

namespace sgk {

int check_batch(const sgk_batch_t *b);

constexpr uint32_t TEXT_STAGE = 24576;  // bytes of a tile's LDS image (a pa tile needs at most 256 * 48)

struct TextArgs : TileList {  // (n_rows = the batch's reads)
    const int16_t *samples;
    const uint64_t *offsets;
    const uint32_t *lengths;
    const double *dig, *off, *rng;
    const uint8_t *id_bytes;
    const uint32_t *id_offs;
    const uint64_t *ev_slots;
    const sgk_event_rec_t *events;
    const uint32_t *n_events;
    uint64_t *row_offsets; // n_reads + 1 (measure)
    uint8_t *text;         // (write)
    uint64_t text_cap;
};

// items of read r: samples (pa), the events that fitted the read's slots (event kinds)
template <int KIND>
__device__ inline uint32_t text_items(const TextArgs &a, uint32_t r) {
    if (KIND == SGK_TEXT_PA) return a.lengths[r];
    const uint64_t cap = a.ev_slots[r + 1] - a.ev_slots[r];
    const uint32_t n = a.n_events[r];
    return n < cap ? n : (uint32_t)cap;  // an overflowing read is written with what fitted, as k_gather_events does
}

// ---- tiles of every read, one 1024-thread workgroup (the shape of k_layout in job_kernels.hip)
template <int KIND>
__global__ __launch_bounds__(1024) void k_text_tiles(TextArgs a) {
    text_tiles_body(a, [&](uint32_t r) { return text_items<KIND>(a, r); });
}

// ---- tile offsets and row offsets, one 1024-thread workgroup
__global__ __launch_bounds__(1024) void k_text_scan(TextArgs a) {
    text_scan_body(a, a.row_offsets);
}

// The sign of a NaN is printed ("nan" / "-nan"), and the reference runs on x86: there an invalid operation (0 * inf,
// 0 / 0, inf / inf) gives the NEGATIVE default NaN and a NaN operand goes through with its own sign (the first operand's
// when both are).  The values come from the library's to_pa(); for the rare NaN the sign is set by that rule, so the
// text does not depend on which NaN this GPU's arithmetic makes.
__device__ inline float nan_sign_as_x86(float res, float a, float b) {
    if (res == res) return res;
    const uint32_t s = (a != a) ? sgk_tf_bits(a) : (b != b) ? sgk_tf_bits(b) : 0x80000000u;
    return __uint_as_float((sgk_tf_bits(res) & 0x7fffffffu) | (s & 0x80000000u));
}
__device__ inline Scale text_scale(double digitisation, double offset, double range) {
    Scale s = make_scale(digitisation, offset, range);
    s.unit = nan_sign_as_x86(s.unit, (float)range, (float)digitisation);  // rangef / digf, src/misc.c:17-19
    return s;
}
__device__ inline float text_pa(int16_t raw, const Scale &sc) {
    const float v = to_pa(raw, sc);
    if (v == v) return v;
    const float shifted = nan_sign_as_x86((float)raw + sc.offf, (float)raw, sc.offf);
    return nan_sign_as_x86(v, shifted, sc.unit);
}

// ---- one tile
struct TileCtx {
    uint32_t r;        // the read
    uint32_t j0;       // its first item in this tile
    uint32_t n_items;  // items of the read
    uint32_t n;        // len_raw_signal
    uint32_t idl;
    const uint8_t *id;
    bool first, last;  // first / last tile of the read
    Scale sc;
    const int16_t *src;
    const sgk_event_rec_t *ev;
};

template <int KIND>
__device__ inline TileCtx tile_ctx(const TextArgs &a, uint32_t t) {
    const uint32_t lo = text_tile_row(a, t);
    TileCtx c;
    c.r = lo;
    c.j0 = (t - a.tile_first[lo]) * TEXT_TILE;
    c.first = c.j0 == 0;
    c.last = t + 1 == a.tile_first[lo + 1];
    c.n_items = text_items<KIND>(a, lo);
    c.n = a.lengths[lo];
    c.idl = a.id_offs[lo + 1] - a.id_offs[lo];
    c.id = a.id_bytes + a.id_offs[lo];
    c.src = nullptr;
    c.ev = nullptr;
    c.sc.offf = 0.f;
    c.sc.unit = 0.f;
    if (KIND == SGK_TEXT_PA) {
        c.sc = text_scale(a.dig[lo], a.off[lo], a.rng[lo]);
        c.src = a.samples + a.offsets[lo];
    } else {
        c.ev = a.events + a.ev_slots[lo];
    }
    return c;
}

__device__ inline sgk_event_rec_t load_event(const sgk_event_rec_t *p) {
    const uint4 v = *reinterpret_cast<const uint4 *>(p);
    sgk_event_rec_t e;
    e.start = v.x;
    e.length = v.y;
    e.mean = __uint_as_float(v.z);
    e.stdv = __uint_as_float(v.w);
    return e;
}

// bytes of item j (j < c.n_items)
template <int KIND>
__device__ inline uint32_t item_len(const TileCtx &c, uint32_t j) {
    if (KIND == SGK_TEXT_PA) return (uint32_t)sgk_tf_f32_len(text_pa(c.src[j], c.sc)) + (j != c.n - 1 ? 1u : 0u);
    const sgk_event_rec_t e = load_event(c.ev + j);
    if (KIND == SGK_TEXT_EVENT)
        return c.idl + 6u + (uint32_t)(sgk_tf_u32_len(j) + sgk_tf_u32_len(e.start) + sgk_tf_u64_len((uint64_t)e.start + e.length) +
                                       sgk_tf_f32_len(e.mean) + sgk_tf_f32_len(e.stdv));
    return e.length ? (uint32_t)sgk_tf_u32_len(e.length) + (j + 1 < c.n_items ? 1u : 0u) : 0u;
}

// the characters of item j at p (item_len bytes)
template <int KIND>
__device__ inline void item_emit(const TileCtx &c, uint32_t j, char *p) {
    if (KIND == SGK_TEXT_PA) {
        p += sgk_tf_f32(p, text_pa(c.src[j], c.sc));
        if (j != c.n - 1) *p = ',';
        return;
    }
    const sgk_event_rec_t e = load_event(c.ev + j);
    if (KIND == SGK_TEXT_EVENT) {
        for (uint32_t k = 0; k < c.idl; ++k) p[k] = (char)c.id[k];
        p += c.idl;
        *p++ = '\t';
        p += sgk_tf_u64(p, j);
        *p++ = '\t';
        p += sgk_tf_u64(p, e.start);
        *p++ = '\t';
        p += sgk_tf_u64(p, (uint64_t)e.start + e.length);
        *p++ = '\t';
        p += sgk_tf_f32(p, e.mean);
        *p++ = '\t';
        p += sgk_tf_f32(p, e.stdv);
        *p = '\n';
        return;
    }
    if (e.length) {
        p += sgk_tf_u64(p, e.length);
        if (j + 1 < c.n_items) *p = ',';
    }
}

// the read's fixed bytes in front of its first item (first tile) ...
template <int KIND>
__device__ inline uint32_t prefix_len(const TileCtx &c) {
    if (KIND == SGK_TEXT_EVENT || !c.first) return 0u;
    uint32_t n = c.idl + 2u + (uint32_t)sgk_tf_u32_len(c.n);
    if (KIND == SGK_TEXT_EVENT_COMPACT) {
        if (c.n_items) {
            const sgk_event_rec_t e0 = load_event(c.ev), e1 = load_event(c.ev + (c.n_items - 1));
            n += 3u + (uint32_t)(sgk_tf_u32_len(e0.start) + sgk_tf_u64_len((uint64_t)e1.start + e1.length) + sgk_tf_u32_len(c.n_items));
        } else {
            n += 7u;
        }
    }
    return n;
}
// ... written by the whole workgroup (the id) and its thread 0 (the numbers)
template <int KIND>
__device__ inline void prefix_emit(const TileCtx &c, char *p) {
    if (KIND == SGK_TEXT_EVENT || !c.first) return;
    for (uint32_t k = threadIdx.x; k < c.idl; k += TEXT_TILE) p[k] = (char)c.id[k];
    if (threadIdx.x != 0) return;
    p += c.idl;
    *p++ = '\t';
    p += sgk_tf_u64(p, c.n);
    *p++ = '\t';
    if (KIND == SGK_TEXT_EVENT_COMPACT) {
        if (c.n_items) {
            const sgk_event_rec_t e0 = load_event(c.ev), e1 = load_event(c.ev + (c.n_items - 1));
            p += sgk_tf_u64(p, e0.start);
            *p++ = '\t';
            p += sgk_tf_u64(p, (uint64_t)e1.start + e1.length);
            *p++ = '\t';
            p += sgk_tf_u64(p, c.n_items);
            *p++ = '\t';
        } else {
            p[0] = '.'; p[1] = '\t'; p[2] = '.'; p[3] = '\t'; p[4] = '.'; p[5] = '\t'; p[6] = '.';
        }
    }
}

// per-lane byte counts -> each lane's offset inside the tile and the tile's total (prefix and line end included)
template <int KIND>
__device__ inline uint32_t tile_offsets(const TileCtx &c, uint32_t *wave_tot, uint32_t &my_len, uint32_t &my_off) {
    const uint32_t j = c.j0 + threadIdx.x;
    my_len = j < c.n_items ? item_len<KIND>(c, j) : 0u;
    const uint32_t sum = text_lane_offsets(my_len, prefix_len<KIND>(c), wave_tot, my_off);
    return sum + (c.last ? 1u : 0u);  // every read ends with one '\n' (event: the empty line)
}

template <int KIND>
__global__ __launch_bounds__(TEXT_TILE) void k_text_measure(TextArgs a) {
    __shared__ uint32_t wave_tot[TEXT_TILE / 64];
    const uint32_t n_tiles = a.hdr->n_tiles;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const TileCtx c = tile_ctx<KIND>(a, t);
        uint32_t my_len, my_off;
        const uint32_t total = tile_offsets<KIND>(c, wave_tot, my_len, my_off);
        if (threadIdx.x == 0) a.tile_bytes[t] = total;
        __syncthreads();  // wave_tot is reused by the next tile
    }
}

template <int KIND>
__global__ __launch_bounds__(TEXT_TILE) void k_text_write(TextArgs a) {
    __shared__ uint32_t wave_tot[TEXT_TILE / 64];
    __shared__ __attribute__((aligned(16))) char stage[TEXT_STAGE + 16];
    const uint32_t n_tiles = a.hdr->n_tiles;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const TileCtx c = tile_ctx<KIND>(a, t);
        uint32_t my_len, my_off;
        const uint32_t total = tile_offsets<KIND>(c, wave_tot, my_len, my_off);
        const uint64_t b0 = a.tile_off[t];
        const uint32_t j = c.j0 + threadIdx.x;
        if (b0 + total > a.text_cap) {  // (workgroup-uniform) nothing of this tile is written
            if (threadIdx.x == 0) atomicOr(&a.hdr->flags, TEXT_FLAG_OVERFLOW);
        } else if (total <= TEXT_STAGE) {
            uint8_t *dst = a.text + b0;
            char *img = stage + text_image_align(dst);  // img + k and dst + k are congruent modulo 16
            prefix_emit<KIND>(c, img);
            if (my_len) item_emit<KIND>(c, j, img + my_off);
            if (c.last && threadIdx.x == 0) img[total - 1] = '\n';
            __syncthreads();
            text_image_flush(dst, img, total);
        } else {
            char *dst = reinterpret_cast<char *>(a.text + b0);
            prefix_emit<KIND>(c, dst);
            if (my_len) item_emit<KIND>(c, j, dst + my_off);
            if (c.last && threadIdx.x == 0) dst[total - 1] = '\n';
        }
        __syncthreads();  // the image and wave_tot are reused by the next tile
    }
}

// ---- test entries: every value into a 48-byte slot of its own; lengths[i] = 255 if the length-only form disagrees
__global__ __launch_bounds__(256) void k_text_numbers_f32(const float *v, uint64_t n, uint8_t *slots, uint8_t *lengths) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const int k = sgk_tf_f32(reinterpret_cast<char *>(slots + 48 * i), v[i]);
        lengths[i] = k == sgk_tf_f32_len(v[i]) ? (uint8_t)k : (uint8_t)255;
    }
}
__global__ __launch_bounds__(256) void k_text_numbers_i64(const int64_t *v, uint64_t n, uint8_t *slots, uint8_t *lengths) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const int k = sgk_tf_i64(reinterpret_cast<char *>(slots + 48 * i), v[i]);
        lengths[i] = k == sgk_tf_i64_len(v[i]) ? (uint8_t)k : (uint8_t)255;
    }
}

static int text_args(int kind, const sgk_batch_t *b, const sgk_text_ids_t *ids, const uint64_t *ev_slots,
                     const sgk_event_rec_t *events, const uint32_t *n_events, void *ws, size_t ws_bytes, TextArgs *a) {
    if (kind < SGK_TEXT_PA || kind > SGK_TEXT_EVENT_COMPACT) return SGK_ERR_ARG;
    const int rc = check_batch(b);
    if (rc != SGK_OK) return rc;
    SGK_TRY(text_ws_check(ws, ws_bytes, sizeof(TextHdr)));
    if (b->n_reads && (!ids || !ids->bytes || !ids->offsets)) return SGK_ERR_ARG;
    if (b->n_reads && kind != SGK_TEXT_PA && (!ev_slots || !events || !n_events)) return SGK_ERR_ARG;
    if (kind != SGK_TEXT_PA && (reinterpret_cast<uintptr_t>(events) & 15u)) return SGK_ERR_ALIGN;
    if (!tile_list_carve(ws, ws_bytes, b->n_reads, a)) return SGK_ERR_WORKSPACE;
    a->samples = b->samples;
    a->offsets = b->offsets;
    a->lengths = b->lengths;
    a->dig = b->digitisation;
    a->off = b->offset;
    a->rng = b->range;
    a->id_bytes = ids ? ids->bytes : nullptr;
    a->id_offs = ids ? ids->offsets : nullptr;
    a->ev_slots = ev_slots;
    a->events = events;
    a->n_events = n_events;
    a->row_offsets = nullptr;
    a->text = nullptr;
    a->text_cap = 0;
    return SGK_OK;
}

}  // namespace sgk

using namespace sgk;

extern "C" {

size_t sgk_text_workspace_bytes(int kind, uint32_t n_reads, uint64_t n_items_capacity) {
    (void)kind;
    return tile_list_bytes(n_reads, n_items_capacity) + 64;
}

int sgk_text_measure(int kind, const sgk_batch_t *b, const sgk_text_ids_t *ids, const uint64_t *ev_slots,
                     const sgk_event_rec_t *events, const uint32_t *n_events, uint64_t *row_offsets, void *ws,
                     size_t ws_bytes, void *stream) {
    TextArgs a;
    const int rc = text_args(kind, b, ids, ev_slots, events, n_events, ws, ws_bytes, &a);
    if (rc != SGK_OK) return rc;
    if (!row_offsets) return SGK_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    a.row_offsets = row_offsets;
    const uint32_t grid = text_grid(a);
    switch (kind) {
        case SGK_TEXT_PA:
            SGK_LAUNCH("k_text_tiles", k_text_tiles<SGK_TEXT_PA>, 1, 1024, st, a);
            SGK_LAUNCH("k_text_measure_pa", k_text_measure<SGK_TEXT_PA>, grid, TEXT_TILE, st, a);
            break;
        case SGK_TEXT_EVENT:
            SGK_LAUNCH("k_text_tiles", k_text_tiles<SGK_TEXT_EVENT>, 1, 1024, st, a);
            SGK_LAUNCH("k_text_measure_event", k_text_measure<SGK_TEXT_EVENT>, grid, TEXT_TILE, st, a);
            break;
        default:
            SGK_LAUNCH("k_text_tiles", k_text_tiles<SGK_TEXT_EVENT_COMPACT>, 1, 1024, st, a);
            SGK_LAUNCH("k_text_measure_event_c", k_text_measure<SGK_TEXT_EVENT_COMPACT>, grid, TEXT_TILE, st, a);
            break;
    }
    SGK_LAUNCH("k_text_scan", k_text_scan, 1, 1024, st, a);
    return SGK_OK;
}

int sgk_text_write(int kind, const sgk_batch_t *b, const sgk_text_ids_t *ids, const uint64_t *ev_slots,
                   const sgk_event_rec_t *events, const uint32_t *n_events, uint8_t *text, uint64_t text_capacity,
                   void *ws, size_t ws_bytes, void *stream) {
    TextArgs a;
    const int rc = text_args(kind, b, ids, ev_slots, events, n_events, ws, ws_bytes, &a);
    if (rc != SGK_OK) return rc;
    if (!text && text_capacity) return SGK_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    a.text = text;
    a.text_cap = text_capacity;
    const uint32_t grid = text_grid(a);
    switch (kind) {
        case SGK_TEXT_PA: SGK_LAUNCH("k_text_write_pa", k_text_write<SGK_TEXT_PA>, grid, TEXT_TILE, st, a); break;
        case SGK_TEXT_EVENT: SGK_LAUNCH("k_text_write_event", k_text_write<SGK_TEXT_EVENT>, grid, TEXT_TILE, st, a); break;
        default: SGK_LAUNCH("k_text_write_event_c", k_text_write<SGK_TEXT_EVENT_COMPACT>, grid, TEXT_TILE, st, a); break;
    }
    return SGK_OK;
}

int sgk_text_status(const void *ws, sgk_text_status_t *out) {
    if (!ws || !out) return SGK_ERR_ARG;
    TextHdr h;
    SGK_HIP_TRY(hipMemcpy(&h, ws, sizeof h, hipMemcpyDeviceToHost));
    out->overflow = (h.flags & TEXT_FLAG_OVERFLOW) ? 1u : 0u;
    out->n_tiles = h.n_tiles;
    out->n_bytes = h.n_bytes;
    if (h.flags & TEXT_FLAG_WORKSPACE) return SGK_ERR_WORKSPACE;
    return out->overflow ? SGK_ERR_CAPACITY : SGK_OK;
}

int sgk_text_numbers_f32(const float *v, uint64_t n, uint8_t *slots48, uint8_t *lengths, void *stream) {
    if (n == 0) return SGK_OK;
    if (!v || !slots48 || !lengths) return SGK_ERR_ARG;
    const uint64_t blocks = (n + 255) / 256;
    SGK_LAUNCH("k_text_numbers_f32", k_text_numbers_f32, (uint32_t)(blocks < 65536 ? blocks : 65536), 256,
               static_cast<hipStream_t>(stream), v, n, slots48, lengths);
    return SGK_OK;
}
int sgk_text_numbers_i64(const int64_t *v, uint64_t n, uint8_t *slots48, uint8_t *lengths, void *stream) {
    if (n == 0) return SGK_OK;
    if (!v || !slots48 || !lengths) return SGK_ERR_ARG;
    const uint64_t blocks = (n + 255) / 256;
    SGK_LAUNCH("k_text_numbers_i64", k_text_numbers_i64, (uint32_t)(blocks < 65536 ? blocks : 65536), 256,
               static_cast<hipStream_t>(stream), v, n, slots48, lengths);
    return SGK_OK;
}

}  // extern "C"
