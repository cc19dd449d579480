// text_tiles.h -- what the device-side text writers share whatever their grammar (text_kernels.hip: pa / event /
// event -c rows of a batch of reads; slow5_text_kernels.hip: the signal column of text SLOW5 records; sref_kernels.hip:
// spans of `sref` rows; ss_kernels.hip: spans of `ss paf2tsv` rows).  What the host pipes of the last two share is
// text_pipe.h.
//
// A writer's rows (reads, spans) have items (samples, events, signal positions).  The items of every row are cut into
// tiles of 256, one workgroup per tile and one item per lane; a row has at least one tile, which carries its fixed
// parts.  The workspace holds the tile list and carries it from the measure call to the write call:
//
//   TextHdr | tile_first[n_rows + 1] | tile_bytes[n_tiles_max] | tile_off[n_tiles_max + 1]
//
//   text_tiles_body   (one 1024-thread workgroup) tile counts of the rows -> tile_first
//   <measure kernel>  (the grammar's own)         tile_bytes
//   text_scan_body    (one 1024-thread workgroup) tile_bytes -> 64-bit tile_off; row_offsets[r] = tile_off[tile_first[r]]
//   <write kernel>    (the grammar's own)         lane offsets (text_lane_offsets), the tile's bytes into an LDS image
//                                                 laid out at the same offset modulo 16 as their place in global
//                                                 memory, the image out as 16-byte stores (text_image_flush)
#pragma once
#include "sgk_common.h"

namespace sgk {

constexpr int TEXT_TILE = 256;             // items per tile = threads per workgroup
constexpr uint32_t TEXT_GRID_MAX = 16384;  // workgroups stride over the tile list
constexpr uint32_t TEXT_FLAG_OVERFLOW = 1u, TEXT_FLAG_WORKSPACE = 2u;

struct TextHdr {  // first 64 bytes of the workspace
    uint32_t flags, n_tiles;
    uint64_t n_bytes;
    uint32_t reserved[12];
};

struct TileList {
    uint32_t n_rows, n_tiles_max;
    TextHdr *hdr;
    uint32_t *tile_first;  // n_rows + 1
    uint32_t *tile_bytes;  // n_tiles_max
    uint64_t *tile_off;    // n_tiles_max + 1
};

// bytes of a tile list for n_rows rows and n_items_capacity items in all
static inline size_t tile_list_bytes(uint32_t n_rows, uint64_t n_items_capacity) {
    const uint64_t nt0 = n_items_capacity / TEXT_TILE + (uint64_t)n_rows + 1;
    const size_t nt = nt0 < 0xfffffff0ull ? (size_t)nt0 : (size_t)0xfffffff0u;
    const size_t off_bytes = round_up(sizeof(TextHdr) + ((size_t)n_rows + 1) * 4, 16);
    const size_t off_off = round_up(off_bytes + nt * 4, 16);
    return off_off + (nt + 1) * 8;
}
// the tile list inside `bytes` bytes at w (16-byte aligned): the tile capacity is what the space holds,
// (bytes - header - tile_first) / (4 + 8 bytes per tile); false if it does not hold one tile
static inline bool tile_list_carve(void *w_, size_t bytes, uint32_t n_rows, TileList *l) {
    const size_t fixed = round_up(sizeof(TextHdr) + ((size_t)n_rows + 1) * 4, 16) + 16 + 8;
    if (bytes < fixed + 12) return false;
    uint64_t nt = (bytes - fixed) / 12;
    if (nt > 0xfffffff0ull) nt = 0xfffffff0ull;
    char *w = static_cast<char *>(w_);
    l->n_rows = n_rows;
    l->n_tiles_max = (uint32_t)nt;
    l->hdr = reinterpret_cast<TextHdr *>(w);
    l->tile_first = reinterpret_cast<uint32_t *>(w + sizeof(TextHdr));
    const size_t off_bytes = round_up(sizeof(TextHdr) + ((size_t)n_rows + 1) * 4, 16);
    l->tile_bytes = reinterpret_cast<uint32_t *>(w + off_bytes);
    l->tile_off = reinterpret_cast<uint64_t *>(w + round_up(off_bytes + (size_t)nt * 4, 16));
    return true;
}
// workgroups of a measure or write kernel: they stride over the tile list
static inline uint32_t text_grid(const TileList &l) { return l.n_tiles_max < TEXT_GRID_MAX ? l.n_tiles_max : TEXT_GRID_MAX; }
// a caller's workspace: missing or not 16-byte aligned is SGK_ERR_ARG, fewer than min_bytes SGK_ERR_WORKSPACE
static inline int text_ws_check(const void *ws, size_t ws_bytes, size_t min_bytes) {
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 15u)) return SGK_ERR_ARG;
    return ws_bytes < min_bytes ? SGK_ERR_WORKSPACE : SGK_OK;
}

#if defined(__HIPCC__)

// ---- tiles of every row, one 1024-thread workgroup (the shape of k_layout in job_kernels.hip); items(r) = items of row r
template <class Items>
__device__ inline void text_tiles_body(const TileList &a, Items items) {
    __shared__ uint32_t part[1024];
    const uint32_t t = threadIdx.x, n = a.n_rows;
    const uint32_t per = (n + 1023u) / 1024u;
    const uint32_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    uint32_t sum = 0;
    for (uint32_t r = lo; r < hi; ++r) {
        const uint32_t it = items(r);
        sum += it ? (it + TEXT_TILE - 1) / TEXT_TILE : 1u;
    }
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint32_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    // (the sum cannot wrap: it is at most n_items / 256 + n_rows, both below 2^32 / 2 for any batch that exists)
    const bool fits = part[1023] <= a.n_tiles_max;
    uint32_t o = part[t] - sum;
    for (uint32_t r = lo; r < hi; ++r) {
        a.tile_first[r] = fits ? o : 0u;
        const uint32_t it = items(r);
        o += it ? (it + TEXT_TILE - 1) / TEXT_TILE : 1u;
    }
    if (t == 1023) {
        a.tile_first[n] = fits ? part[1023] : 0u;
        a.hdr->flags = fits ? 0u : TEXT_FLAG_WORKSPACE;  // a workspace sized for a smaller batch: nothing is written
        a.hdr->n_tiles = fits ? part[1023] : 0u;
        a.hdr->n_bytes = 0;
    }
}

// ---- tile offsets and row offsets, one 1024-thread workgroup
__device__ inline void text_scan_body(const TileList &a, uint64_t *row_offsets) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x, n = a.hdr->n_tiles;
    const uint32_t per = (n + 1023u) / 1024u;
    const uint32_t lo = (uint64_t)t * per < n ? t * per : n, hi = (uint64_t)lo + per < n ? lo + per : n;
    uint64_t sum = 0;
    for (uint32_t k = lo; k < hi; ++k) sum += a.tile_bytes[k];
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint64_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint64_t o = part[t] - sum;
    for (uint32_t k = lo; k < hi; ++k) {
        a.tile_off[k] = o;
        o += a.tile_bytes[k];
    }
    if (t == 1023) {
        a.tile_off[n] = part[1023];
        a.hdr->n_bytes = part[1023];
    }
    __syncthreads();
    for (uint32_t r = t; r <= a.n_rows; r += 1024) row_offsets[r] = a.tile_off[a.tile_first[r]];
}

// the row of tile t: tile_first[r] <= t < tile_first[r + 1] (strictly increasing: every row has a tile)
__device__ inline uint32_t text_tile_row(const TileList &a, uint32_t t) {
    uint32_t lo = 0, hi = a.n_rows;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.tile_first[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

// per-lane byte counts -> each lane's offset inside the tile (behind `prefix` bytes of the row's fixed part) and the
// bytes of prefix + items; wave_tot: TEXT_TILE / 64 words of LDS, free again after the caller's next __syncthreads()
__device__ inline uint32_t text_lane_offsets(uint32_t my_len, uint32_t prefix, uint32_t *wave_tot, uint32_t &my_off) {
    const int incl = wave_incl_scan_i((int)my_len);
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 63u) wave_tot[w] = (uint32_t)incl;
    __syncthreads();
    uint32_t base = prefix, sum = prefix;
    for (uint32_t k = 0; k < TEXT_TILE / 64; ++k) {
        if (k < w) base += wave_tot[k];
        sum += wave_tot[k];
    }
    my_off = base + (uint32_t)incl - my_len;
    return sum;
}

// byte k of the image belongs at dst + k, and img + k and dst + k are congruent modulo 16 (img = stage + al below)
__device__ inline uint32_t text_image_align(const uint8_t *dst) { return (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u); }

// the image's `total` bytes to dst: 16-byte stores for the aligned body, byte stores for the up to 15 bytes in front
// of it and behind it.  Two tiles may share a 16-byte word of the output; neither reads or rewrites the other's bytes.
__device__ inline void text_image_flush(uint8_t *dst, const char *img, uint32_t total) {
    const uint32_t al = text_image_align(dst);
    const uint32_t head0 = (16u - al) & 15u, head = head0 < total ? head0 : total;
    const uint32_t nvec = (total - head) / 16u, tail0 = head + nvec * 16u;
    if (threadIdx.x < head) dst[threadIdx.x] = (uint8_t)img[threadIdx.x];
    for (uint32_t v = threadIdx.x; v < nvec; v += TEXT_TILE)
        *reinterpret_cast<uint4 *>(dst + head + 16u * v) = *reinterpret_cast<const uint4 *>(img + head + 16u * v);
    if (threadIdx.x < total - tail0) dst[tail0 + threadIdx.x] = (uint8_t)img[tail0 + threadIdx.x];
}

#endif  // __HIPCC__

}  // namespace sgk
