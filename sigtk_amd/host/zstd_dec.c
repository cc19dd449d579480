/* zstd_dec.c -- see zstd_dec.h.  Section numbers are RFC 8878's. */
#include "zstd_dec.h"

#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#define ZSD_BLOCK_MAX (128u << 10)
#define ZSD_LL_LOG 9
#define ZSD_OF_LOG 8
#define ZSD_ML_LOG 9
#define ZSD_HUF_LOG 11
#define ZSD_W_LOG 6

/* an FSE decoding cell: symbol | bits to read << 8 | baseline of the next state << 16 */
typedef uint32_t fse_cell_t;

typedef struct {
    const uint8_t *in;
    size_t in_len;
    uint8_t *out;
    size_t limit;        /* bytes wanted: the content size, or less (zsd_decode_head) */
    uint64_t pos;
    int head;            /* stop once `limit` bytes exist */
    uint32_t rep[3];
    int have_huf, have_ll, have_of, have_ml;
    uint32_t huf_log, ll_log, of_log, ml_log;
    uint16_t huf[1 << ZSD_HUF_LOG];   /* symbol | code length << 8, indexed by the next huf_log bits */
    fse_cell_t ll[1 << ZSD_LL_LOG], of[1 << ZSD_OF_LOG], ml[1 << ZSD_ML_LOG];
    fse_cell_t wt[1 << ZSD_W_LOG];    /* the table of FSE-compressed Huffman weights */
    uint8_t lit[ZSD_BLOCK_MAX];       /* the block's literals when they are Huffman coded */
} zsd_t;

static const int16_t LL_DEFAULT[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
static const int16_t ML_DEFAULT[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
static const int16_t OF_DEFAULT[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
static const uint32_t LL_BASE[36] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
static const uint8_t LL_BITS[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
static const uint32_t ML_BASE[53] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
static const uint8_t ML_BITS[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};

static inline uint32_t highbit(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }   /* v != 0 */

/* up to 8 bytes from p[at ..), zeros behind p[n) */
static inline uint64_t load64(const uint8_t *p, size_t n, size_t at) {
    uint64_t v = 0;
    if (at + 8 <= n) memcpy(&v, p + at, 8);
    else if (at < n) memcpy(&v, p + at, n - at);
    return v;
}

/* ---- a bitstream read backwards (4.1): bits [0, pos) of p[0 .. n) are unread, the next ones read are the highest.
 * Below bit 0 there are zeros; pos goes negative there and the caller looks at it when the stream should be over. */
typedef struct {
    const uint8_t *p;
    size_t n;
    int64_t pos;
} rbits_t;

static int rbits_init(rbits_t *b, const uint8_t *p, size_t n) {
    if (n == 0 || p[n - 1] == 0) return -1;   /* no end mark */
    b->p = p;
    b->n = n;
    b->pos = (int64_t)(n - 1) * 8 + highbit(p[n - 1]);
    return 0;
}
static inline uint32_t rbits_peek(const rbits_t *b, uint32_t nb) {   /* nb <= 32 */
    if (nb == 0) return 0;
    const int64_t lo = b->pos - (int64_t)nb;
    const uint64_t mask = (1ull << nb) - 1;
    if (lo >= 0) return (uint32_t)((load64(b->p, b->n, (size_t)(lo >> 3)) >> (lo & 7)) & mask);
    if (-lo >= (int64_t)nb) return 0;
    return (uint32_t)((load64(b->p, b->n, 0) << (-lo)) & mask);
}
static inline uint32_t rbits_get(rbits_t *b, uint32_t nb) {
    const uint32_t v = rbits_peek(b, nb);
    b->pos -= nb;
    return v;
}

/* ---- FSE (4.1.1) */
/* the distribution at p[0 .. n): counts[0 .. *nsym), *log; returns the bytes it takes, or -status */
static int fse_read_dist(const uint8_t *p, size_t n, uint32_t max_log, uint32_t max_sym, int16_t *counts, uint32_t *nsym, uint32_t *log) {
    size_t bit = 0;
    const size_t nbits = n * 8;
#define FWD(k) ((uint32_t)((load64(p, n, bit >> 3) >> (bit & 7)) & ((1u << (k)) - 1u)))
    if (nbits < 4) return -ZSD_ERR_TRUNCATED;
    const uint32_t al = 5 + FWD(4);
    bit += 4;
    if (al > max_log) return -ZSD_ERR_TABLE;
    int32_t remaining = 1 << al;
    uint32_t s = 0;
    while (remaining > 0 && s <= max_sym) {
        const uint32_t nb = highbit((uint32_t)remaining + 1) + 1;
        if (bit + nb > nbits + 7) return -ZSD_ERR_TRUNCATED;   /* (the low form may end up to a bit short of nb) */
        uint32_t v = FWD(nb);
        const uint32_t lower = (1u << (nb - 1)) - 1, thresh = (1u << nb) - 1 - ((uint32_t)remaining + 1);
        if ((v & lower) < thresh) {
            bit += nb - 1;
            v &= lower;
        } else {
            bit += nb;
            if (v > lower) v -= thresh;
        }
        if (bit > nbits) return -ZSD_ERR_TRUNCATED;
        const int32_t proba = (int32_t)v - 1;
        remaining -= proba < 0 ? 1 : proba;
        counts[s++] = (int16_t)proba;
        if (proba == 0) {
            for (;;) {   /* runs of zeros: two bits each, 3 means another two follow (bounded by the alphabet) */
                if (bit + 2 > nbits) return -ZSD_ERR_TRUNCATED;
                const uint32_t r = FWD(2);
                bit += 2;
                for (uint32_t k = 0; k < r; k++) {
                    if (s > max_sym) return -ZSD_ERR_TABLE;
                    counts[s++] = 0;
                }
                if (r != 3) break;
            }
        }
    }
#undef FWD
    if (remaining != 0 || s > max_sym + 1) return -ZSD_ERR_TABLE;   /* under- or over-filled */
    *nsym = s;
    *log = al;
    return (int)((bit + 7) >> 3);
}

static int fse_build(fse_cell_t *t, const int16_t *counts, uint32_t nsym, uint32_t log) {
    const uint32_t size = 1u << log, mask = size - 1, step = (size >> 1) + (size >> 3) + 3;
    uint16_t next[256];
    uint32_t high = size - 1;
    for (uint32_t s = 0; s < nsym; s++) {
        if (counts[s] == -1) {
            t[high--] = s;
            next[s] = 1;
        } else next[s] = (uint16_t)counts[s];
    }
    uint32_t pos = 0;
    for (uint32_t s = 0; s < nsym; s++)
        for (int32_t i = 0; i < counts[s]; i++) {
            t[pos] = s;
            do pos = (pos + step) & mask; while (pos > high);
        }
    if (pos != 0) return ZSD_ERR_TABLE;
    for (uint32_t i = 0; i < size; i++) {
        const uint32_t s = t[i], nx = next[s]++;
        const uint32_t nb = log - highbit(nx);
        t[i] = s | (nb << 8) | (((nx << nb) - size) << 16);
    }
    return 0;
}
static void fse_rle(fse_cell_t *t, uint32_t sym) { t[0] = sym; }   /* one state, no bits, log 0 */

/* ---- Huffman (4.2.1): the tree description at p -> the table; returns the bytes it takes, or -status */
static int huf_read(zsd_t *z, const uint8_t *p, size_t n) {
    if (n < 1) return -ZSD_ERR_TRUNCATED;
    uint8_t w[256];
    uint32_t nw;
    size_t used;
    const uint32_t h = p[0];
    if (h >= 128) {
        nw = h - 127;
        used = 1 + (nw + 1) / 2;
        if (used > n) return -ZSD_ERR_TRUNCATED;
        for (uint32_t i = 0; i < nw; i++) w[i] = (i & 1) ? (p[1 + i / 2] & 15) : (p[1 + i / 2] >> 4);
    } else {
        used = 1 + h;
        if (used > n) return -ZSD_ERR_TRUNCATED;
        if (h < 2) return -ZSD_ERR_TABLE;
        int16_t counts[12];
        uint32_t ns, log;
        const int hb = fse_read_dist(p + 1, h, ZSD_W_LOG, 11, counts, &ns, &log);
        if (hb < 0) return hb == -ZSD_ERR_TRUNCATED ? -ZSD_ERR_TABLE : hb;   /* (cut by its own size field, not by the input) */
        if (fse_build(z->wt, counts, ns, log)) return -ZSD_ERR_TABLE;
        rbits_t b;
        if ((size_t)hb >= h || rbits_init(&b, p + 1 + hb, h - (size_t)hb)) return -ZSD_ERR_TABLE;
        /* two states take turns until one of them would read in front of the stream (4.2.1.2) */
        uint32_t s1 = rbits_get(&b, log), s2 = rbits_get(&b, log);
        if (b.pos < 0) return -ZSD_ERR_TABLE;
        nw = 0;
        for (;;) {
            if (nw > 253) return -ZSD_ERR_TABLE;
            w[nw++] = (uint8_t)z->wt[s1];
            s1 = (z->wt[s1] >> 16) + rbits_get(&b, (z->wt[s1] >> 8) & 255);
            if (b.pos < 0) { w[nw++] = (uint8_t)z->wt[s2]; break; }
            w[nw++] = (uint8_t)z->wt[s2];
            s2 = (z->wt[s2] >> 16) + rbits_get(&b, (z->wt[s2] >> 8) & 255);
            if (b.pos < 0) { w[nw++] = (uint8_t)z->wt[s1]; break; }
        }
    }
    /* the last weight is what completes the sum to a power of two */
    uint32_t sum = 0, rank[ZSD_HUF_LOG + 2];
    memset(rank, 0, sizeof rank);
    for (uint32_t i = 0; i < nw; i++) {
        if (w[i] > ZSD_HUF_LOG) return -ZSD_ERR_TABLE;
        if (w[i]) sum += 1u << (w[i] - 1);
        rank[w[i]]++;
    }
    if (sum == 0) return -ZSD_ERR_TABLE;
    const uint32_t log = highbit(sum) + 1, left = (1u << log) - sum;
    if (log > ZSD_HUF_LOG || (left & (left - 1)) != 0) return -ZSD_ERR_TABLE;
    w[nw] = (uint8_t)(highbit(left) + 1);
    rank[w[nw]]++;
    nw++;
    if (rank[1] < 2 || (rank[1] & 1)) return -ZSD_ERR_TABLE;   /* (as libzstd: the two longest codes are siblings) */
    /* codes in order of weight, then of symbol: weight 1 (the longest codes) from index 0 */
    uint32_t start[ZSD_HUF_LOG + 2], at = 0;
    for (uint32_t k = 1; k <= log; k++) {
        start[k] = at;
        at += rank[k] << (k - 1);
    }
    for (uint32_t s = 0; s < nw; s++) {
        if (!w[s]) continue;
        const uint32_t span = 1u << (w[s] - 1);
        const uint16_t e = (uint16_t)(s | ((log + 1 - w[s]) << 8));
        for (uint32_t k = 0; k < span; k++) z->huf[start[w[s]] + k] = e;
        start[w[s]] += span;
    }
    z->huf_log = log;
    z->have_huf = 1;
    return (int)used;
}

/* one Huffman stream of nout symbols: all of its bits and no more; with `whole` 0 its first nout symbols, whatever follows */
static int huf_stream(const zsd_t *z, const uint8_t *p, size_t n, uint8_t *dst, size_t nout, int whole) {
    rbits_t b;
    if (rbits_init(&b, p, n)) return ZSD_ERR_SECTION;
    const uint32_t log = z->huf_log;
    for (size_t i = 0; i < nout; i++) {
        const uint16_t e = z->huf[rbits_peek(&b, log)];
        dst[i] = (uint8_t)e;
        b.pos -= e >> 8;
        if (b.pos < 0) return ZSD_ERR_SECTION;
    }
    return !whole || b.pos == 0 ? 0 : ZSD_ERR_SECTION;
}

/* ---- one compressed block (3.1.1.3): p[0 .. n) */
/* z->pos counts the frame's bytes as if all were kept; those at or behind z->limit are not written */
static void put_literals(zsd_t *z, const uint8_t *src, size_t n, int rle) {
    if (z->pos < z->limit) {
        const size_t k = n < z->limit - z->pos ? n : z->limit - z->pos;
        if (rle) memset(z->out + z->pos, src[0], k);
        else memcpy(z->out + z->pos, src, k);
    }
    z->pos += n;
}
static void put_match(zsd_t *z, size_t off, size_t n) {   /* off <= z->pos */
    if (z->pos < z->limit) {
        const size_t k = n < z->limit - z->pos ? n : z->limit - z->pos;
        uint8_t *d = z->out + z->pos;
        const uint8_t *s = d - off;
        if (off >= k) memcpy(d, s, k);
        else for (size_t j = 0; j < k; j++) d[j] = s[j];
    }
    z->pos += n;
}

static int block_compressed(zsd_t *z, const uint8_t *p, size_t n, uint64_t room) {
    /* literals section */
    if (n < 1) return ZSD_ERR_SECTION;
    const uint32_t type = p[0] & 3, sf = (p[0] >> 2) & 3;
    size_t hl, regen, comp = 0;
    uint32_t streams = 1;
    if (type < 2) {
        if ((sf & 1) == 0) { hl = 1; regen = p[0] >> 3; }
        else if (sf == 1) { hl = 2; if (n < 2) return ZSD_ERR_SECTION; regen = (p[0] >> 4) | ((size_t)p[1] << 4); }
        else { hl = 3; if (n < 3) return ZSD_ERR_SECTION; regen = (p[0] >> 4) | ((size_t)p[1] << 4) | ((size_t)p[2] << 12); }
    } else {
        hl = sf < 2 ? 3 : sf + 2;
        if (n < hl) return ZSD_ERR_SECTION;
        const uint64_t v = load64(p, n, 0) >> 4;
        const uint32_t nb = sf < 2 ? 10 : (sf == 2 ? 14 : 18);
        regen = (size_t)(v & ((1u << nb) - 1));
        comp = (size_t)((v >> nb) & ((1u << nb) - 1));
        streams = sf == 0 ? 1 : 4;
    }
    if (regen > ZSD_BLOCK_MAX) return ZSD_ERR_SECTION;
    const uint8_t *lit;
    int lit_rle = 0;
    size_t at = hl;
    if (type == 0) {
        if (regen > n - at) return ZSD_ERR_SECTION;
        lit = p + at;
        at += regen;
    } else if (type == 1) {
        if (n - at < 1) return ZSD_ERR_SECTION;
        lit = p + at;
        lit_rle = 1;
        at += 1;
    } else {
        if (comp > n - at) return ZSD_ERR_SECTION;
        const uint8_t *q = p + at;
        size_t qn = comp;
        at += comp;
        if (type == 2) {
            const int used = huf_read(z, q, qn);
            if (used < 0) return used == -ZSD_ERR_TRUNCATED ? ZSD_ERR_SECTION : -used;
            q += used;
            qn -= (size_t)used;
        } else if (!z->have_huf) return ZSD_ERR_TABLE;
        /* The head (zsd_decode_head) wants `need` more bytes.  A literal is copied only where it lands in front of the
         * limit, and literal k of a block lands at or behind the block's byte k: no literal from index `need` on is
         * ever read.  They all lie in the first stream when need <= its length, so only its first `need` symbols are
         * decoded; whether the streams end where they should is left to whoever decodes the whole frame. */
        const size_t need = z->head && z->pos < z->limit ? z->limit - (size_t)z->pos : regen;
        if (need < (streams == 1 ? regen : (regen + 3) / 4)) {
            size_t s1 = qn;
            if (streams == 4) {
                if (qn < 6) return ZSD_ERR_SECTION;
                s1 = q[0] | ((size_t)q[1] << 8);
                if (s1 > qn - 6) return ZSD_ERR_SECTION;
                q += 6;
            }
            const int rc = huf_stream(z, q, s1, z->lit, need, 0);
            if (rc) return rc;
        } else if (streams == 1) {
            const int rc = huf_stream(z, q, qn, z->lit, regen, 1);
            if (rc) return rc;
        } else {
            if (qn < 6) return ZSD_ERR_SECTION;
            const size_t s1 = q[0] | ((size_t)q[1] << 8), s2 = q[2] | ((size_t)q[3] << 8), s3 = q[4] | ((size_t)q[5] << 8);
            if (s1 + s2 + s3 > qn - 6) return ZSD_ERR_SECTION;
            const size_t s4 = qn - 6 - s1 - s2 - s3, seg = (regen + 3) / 4;
            if (seg * 3 > regen) return ZSD_ERR_SECTION;
            int rc = huf_stream(z, q + 6, s1, z->lit, seg, 1);
            if (!rc) rc = huf_stream(z, q + 6 + s1, s2, z->lit + seg, seg, 1);
            if (!rc) rc = huf_stream(z, q + 6 + s1 + s2, s3, z->lit + 2 * seg, seg, 1);
            if (!rc) rc = huf_stream(z, q + 6 + s1 + s2 + s3, s4, z->lit + 3 * seg, regen - 3 * seg, 1);
            if (rc) return rc;
        }
        lit = z->lit;
    }
    /* sequences section */
    if (n - at < 1) return ZSD_ERR_SECTION;
    uint32_t nseq = p[at++];
    if (nseq >= 128) {
        if (nseq == 255) {
            if (n - at < 2) return ZSD_ERR_SECTION;
            nseq = (p[at] | ((uint32_t)p[at + 1] << 8)) + 0x7f00;
            at += 2;
        } else {
            if (n - at < 1) return ZSD_ERR_SECTION;
            nseq = ((nseq - 128) << 8) + p[at++];
        }
    }
    const uint64_t start = z->pos;
    size_t lit_at = 0;
    if (nseq == 0) {
        if (at != n) return ZSD_ERR_SECTION;
    } else {
        if (n - at < 1) return ZSD_ERR_SECTION;
        const uint32_t modes = p[at++];
        if (modes & 3) return ZSD_ERR_SECTION;
        for (int k = 0; k < 3; k++) {
            const uint32_t mode = (modes >> (6 - 2 * k)) & 3;
            fse_cell_t *t = k == 0 ? z->ll : (k == 1 ? z->of : z->ml);
            uint32_t *log = k == 0 ? &z->ll_log : (k == 1 ? &z->of_log : &z->ml_log);
            int *have = k == 0 ? &z->have_ll : (k == 1 ? &z->have_of : &z->have_ml);
            const uint32_t max_sym = k == 0 ? 35 : (k == 1 ? 31 : 52), max_log = k == 0 ? ZSD_LL_LOG : (k == 1 ? ZSD_OF_LOG : ZSD_ML_LOG);
            if (mode == 0) {
                const int16_t *d = k == 0 ? LL_DEFAULT : (k == 1 ? OF_DEFAULT : ML_DEFAULT);
                *log = k == 1 ? 5 : 6;
                fse_build(t, d, k == 0 ? 36 : (k == 1 ? 29 : 53), *log);
            } else if (mode == 1) {
                if (n - at < 1) return ZSD_ERR_SECTION;
                if (p[at] > max_sym) return ZSD_ERR_TABLE;
                fse_rle(t, p[at++]);
                *log = 0;
            } else if (mode == 2) {
                int16_t counts[64];
                uint32_t ns;
                const int used = fse_read_dist(p + at, n - at, max_log, max_sym, counts, &ns, log);
                if (used < 0) return used == -ZSD_ERR_TRUNCATED ? ZSD_ERR_SECTION : -used;
                if (fse_build(t, counts, ns, *log)) return ZSD_ERR_TABLE;
                at += (size_t)used;
            } else if (!*have) return ZSD_ERR_TABLE;
            *have = 1;
        }
        rbits_t b;
        if (at >= n || rbits_init(&b, p + at, n - at)) return ZSD_ERR_SECTION;
        uint32_t sl = rbits_get(&b, z->ll_log), so = rbits_get(&b, z->of_log), sm = rbits_get(&b, z->ml_log);
        if (b.pos < 0) return ZSD_ERR_SECTION;
        for (uint32_t i = 0; i < nseq; i++) {
            const fse_cell_t cl = z->ll[sl], co = z->of[so], cm = z->ml[sm];
            const uint32_t oc = co & 255, mc = cm & 255, lc = cl & 255;
            if (lc > 35 || mc > 52 || oc > 31) return ZSD_ERR_SECTION;   /* (never: the tables hold no such symbol) */
            const uint64_t ov = (1ull << oc) + rbits_get(&b, oc);
            const uint32_t mlen = ML_BASE[mc] + rbits_get(&b, ML_BITS[mc]);
            const uint32_t ll = LL_BASE[lc] + rbits_get(&b, LL_BITS[lc]);
            if (i + 1 < nseq) {
                sl = (cl >> 16) + rbits_get(&b, (cl >> 8) & 255);
                sm = (cm >> 16) + rbits_get(&b, (cm >> 8) & 255);
                so = (co >> 16) + rbits_get(&b, (co >> 8) & 255);
            }
            if (b.pos < 0) return ZSD_ERR_SECTION;
            uint64_t off;
            if (ov > 3) {
                off = ov - 3;
                z->rep[2] = z->rep[1];
                z->rep[1] = z->rep[0];
            } else {
                const uint32_t idx = (uint32_t)ov - 1 + (ll == 0);   /* 0 .. 3 */
                if (idx == 0) off = z->rep[0];
                else {
                    off = idx == 3 ? (uint64_t)z->rep[0] - 1 : z->rep[idx];
                    if (idx != 1) z->rep[2] = z->rep[1];
                    z->rep[1] = z->rep[0];
                }
            }
            if (off == 0 || off > 0xffffffffull) return ZSD_ERR_OFFSET;
            z->rep[0] = (uint32_t)off;
            if (ll > regen - lit_at) return ZSD_ERR_SECTION;
            if ((uint64_t)ll + mlen > room - (z->pos - start)) return ZSD_ERR_SIZE;   /* past the block's 128 KB or the frame's size */
            put_literals(z, lit_rle ? lit : lit + lit_at, ll, lit_rle);
            lit_at += ll;
            if (off > z->pos) return ZSD_ERR_OFFSET;
            put_match(z, (size_t)off, mlen);
            if (z->head && z->pos >= z->limit) return 0;   /* the head is there */
        }
        if (b.pos != 0) return ZSD_ERR_SECTION;
    }
    const size_t rest = regen - lit_at;
    if (rest > room - (z->pos - start)) return ZSD_ERR_SIZE;
    put_literals(z, lit_rle ? lit : lit + lit_at, rest, lit_rle);
    return 0;
}

/* ---- XXH64, seed 0 (3.1.1: the checksum is its low 32 bits) */
#define XP1 0x9E3779B185EBCA87ull
#define XP2 0xC2B2AE3D27D4EB4Full
#define XP3 0x165667B19E3779F9ull
#define XP4 0x85EBCA77C2B2AE63ull
#define XP5 0x27D4EB2F165667C5ull
static inline uint64_t rotl64(uint64_t v, int r) { return (v << r) | (v >> (64 - r)); }
static inline uint64_t xround(uint64_t acc, uint64_t v) { return rotl64(acc + v * XP2, 31) * XP1; }
static inline uint64_t xmerge(uint64_t h, uint64_t v) { return (h ^ xround(0, v)) * XP1 + XP4; }
static uint64_t xxh64(const uint8_t *p, size_t n) {
    const uint8_t *end = p + n;
    uint64_t h;
    if (n >= 32) {
        uint64_t v1 = XP1 + XP2, v2 = XP2, v3 = 0, v4 = 0ull - XP1;
        do {
            uint64_t w[4];
            memcpy(w, p, 32);
            v1 = xround(v1, w[0]); v2 = xround(v2, w[1]); v3 = xround(v3, w[2]); v4 = xround(v4, w[3]);
            p += 32;
        } while (p + 32 <= end);
        h = rotl64(v1, 1) + rotl64(v2, 7) + rotl64(v3, 12) + rotl64(v4, 18);
        h = xmerge(h, v1); h = xmerge(h, v2); h = xmerge(h, v3); h = xmerge(h, v4);
    } else h = XP5;
    h += (uint64_t)n;
    while (p + 8 <= end) {
        uint64_t w;
        memcpy(&w, p, 8);
        h = rotl64(h ^ xround(0, w), 27) * XP1 + XP4;
        p += 8;
    }
    if (p + 4 <= end) {
        uint32_t w;
        memcpy(&w, p, 4);
        h = rotl64(h ^ (w * XP1), 23) * XP2 + XP3;
        p += 4;
    }
    while (p < end) h = rotl64(h ^ (*p++ * XP5), 11) * XP1;
    h ^= h >> 33; h *= XP2; h ^= h >> 29; h *= XP3; h ^= h >> 32;
    return h;
}

/* ---- the frame (3.1.1) */
typedef struct {
    uint64_t size;
    size_t hdr_len;
    int checksum;
} zsd_hdr_t;

static int read_header(const uint8_t *in, size_t n, zsd_hdr_t *h) {
    if (n < 4) return ZSD_ERR_TRUNCATED;
    if (!(in[0] == 0x28 && in[1] == 0xB5 && in[2] == 0x2F && in[3] == 0xFD)) return ZSD_ERR_HEADER;   /* (a skippable frame too) */
    if (n < 5) return ZSD_ERR_TRUNCATED;
    const uint32_t d = in[4], fcs_flag = d >> 6, single = (d >> 5) & 1, did_flag = d & 3;
    if (d & 8) return ZSD_ERR_HEADER;
    const size_t did_len = did_flag == 3 ? 4 : did_flag, fcs_len = fcs_flag == 0 ? single : (size_t)1 << fcs_flag;
    if (fcs_len == 0) return ZSD_ERR_HEADER;   /* no content size */
    size_t at = 5 + (single ? 0 : 1);
    if (n < at + did_len + fcs_len) return ZSD_ERR_TRUNCATED;
    for (size_t k = 0; k < did_len; k++)
        if (in[at + k]) return ZSD_ERR_HEADER;
    at += did_len;
    uint64_t v = 0;
    memcpy(&v, in + at, fcs_len);
    if (fcs_len == 2) v += 256;
    h->size = v;
    h->hdr_len = at + fcs_len;
    h->checksum = (d >> 2) & 1;
    return 0;
}

int zsd_content_size(const uint8_t *in, size_t in_len, uint64_t *size) {
    zsd_hdr_t h;
    const int rc = read_header(in, in_len, &h);
    if (!rc) *size = h.size;
    return rc;
}

static int decode(const uint8_t *in, size_t in_len, uint8_t *out, size_t cap, size_t *out_len, int head, zsd_t *z) {
    zsd_hdr_t h;
    *out_len = 0;
    int rc = read_header(in, in_len, &h);
    if (rc) return rc;
    if (!head && h.size > cap) return ZSD_ERR_SIZE;
    z->in = in;
    z->in_len = in_len;
    z->out = out;
    z->limit = h.size < cap ? (size_t)h.size : cap;
    z->pos = 0;
    z->rep[0] = 1; z->rep[1] = 4; z->rep[2] = 8;
    z->have_huf = z->have_ll = z->have_of = z->have_ml = 0;
    z->head = head && z->limit < h.size;
    size_t at = h.hdr_len;
    for (int last = 0; !last;) {
        if (z->head && z->pos >= z->limit) return ZSD_OK;
        if (in_len - at < 3) return ZSD_ERR_TRUNCATED;
        const uint32_t bh = in[at] | ((uint32_t)in[at + 1] << 8) | ((uint32_t)in[at + 2] << 16);
        at += 3;
        last = bh & 1;
        const uint32_t type = (bh >> 1) & 3, bsize = bh >> 3;
        if (type == 3 || bsize > ZSD_BLOCK_MAX) return ZSD_ERR_BLOCK;
        const uint64_t room = h.size - z->pos < ZSD_BLOCK_MAX ? h.size - z->pos : ZSD_BLOCK_MAX;
        if ((type == 1 ? 1u : bsize) > in_len - at) return ZSD_ERR_TRUNCATED;
        if (type == 0 || type == 1) {
            if (bsize > room) return ZSD_ERR_SIZE;
            put_literals(z, in + at, bsize, type == 1);
            at += type == 0 ? bsize : 1;
        } else {
            rc = block_compressed(z, in + at, bsize, room);
            at += bsize;
        }
        *out_len = z->pos < z->limit ? (size_t)z->pos : z->limit;
        if (rc) return rc;
    }
    if (z->head && z->pos >= z->limit) return ZSD_OK;
    if (z->pos != h.size) return ZSD_ERR_SIZE;
    if (h.checksum) {
        if (in_len - at < 4) return ZSD_ERR_TRUNCATED;
        const uint32_t want = in[at] | ((uint32_t)in[at + 1] << 8) | ((uint32_t)in[at + 2] << 16) | ((uint32_t)in[at + 3] << 24);
        at += 4;
        if ((uint32_t)xxh64(out, (size_t)z->pos) != want) return ZSD_ERR_CHECKSUM;
    }
    if (at != in_len) return ZSD_ERR_HEADER;   /* bytes behind the frame (another frame among them) */
    return ZSD_OK;
}

/* The tables and the literals buffer (about 150 KB) are kept per thread: one allocation for all the records a reader
 * thread decodes, released when the thread ends. */
static pthread_key_t state_key;
static pthread_once_t state_once = PTHREAD_ONCE_INIT;
static int state_key_ok;
static void state_make_key(void) { state_key_ok = pthread_key_create(&state_key, free) == 0; }
static zsd_t *state(void) {
    pthread_once(&state_once, state_make_key);
    if (!state_key_ok) return NULL;
    zsd_t *z = (zsd_t *)pthread_getspecific(state_key);
    if (!z) {
        z = (zsd_t *)malloc(sizeof *z);
        if (z && pthread_setspecific(state_key, z) != 0) {
            free(z);
            z = NULL;
        }
    }
    return z;
}

int zsd_decode(const uint8_t *in, size_t in_len, uint8_t *out, size_t cap, size_t *out_len) {
    zsd_t *z = state();
    size_t n = 0;
    const int rc = z ? decode(in, in_len, out, cap, &n, 0, z) : ZSD_ERR_MEM;
    if (out_len) *out_len = n;
    return rc;
}

int zsd_decode_head(const uint8_t *in, size_t in_len, uint8_t *out, size_t want, size_t *out_len) {
    zsd_t *z = state();
    size_t n = 0;
    const int rc = z ? decode(in, in_len, out, want, &n, 1, z) : ZSD_ERR_MEM;
    if (out_len) *out_len = n;
    return rc;
}

const char *zsd_status_name(int status) {
    static const char *const names[] = {"ok", "frame header refused", "bad block header", "bad table description",
                                        "bad literals or sequences section", "offset in front of the frame", "truncated",
                                        "checksum mismatch", "size differs from the declaration or exceeds the room", "out of memory"};
    return status >= 0 && status <= 9 ? names[status] : "unknown";
}
