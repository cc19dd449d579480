// text_pipe.h -- what a two-slot host text pipe is (text_pipes.hip: sgk_sref_pipe_*, sgk_ss_pipe_*), whatever its grammar.
//
// A pipe has two slots, so that one batch's download and the caller's fwrite overlap the next one's upload and kernels.
// A slot goes begin -> (the caller fills the pinned staging) -> submit -> wait.  It is busy from a submit that succeeded
// to the wait that follows; a submit that fails, for whatever reason, leaves it idle.  Its buffers are grow_buf.h's:
// they grow on demand, are kept from batch to batch and free themselves.
#pragma once
#include <new>

#include "grow_buf.h"
#include "text_tiles.h"

namespace sgk {
#pragma GCC visibility push(hidden)

// The sections of a staging blob, laid out front to back.  Every section starts 16-byte aligned; `slack` bytes stay
// free behind one that a kernel reads in 16-byte words.
struct StageCursor {
    size_t pos = 0;  // where the next section starts; after the last one, the bytes of the blob
    size_t take(size_t bytes, size_t slack = 0) {
        const size_t at = pos;
        pos = round_up(pos + bytes + slack, 16);
        return at;
    }
};

// the part of a slot every text pipe has
struct TextSlot {
    hipStream_t stream{};
    Pin<TextHdr> hdr;
    Dev<uint8_t> ws;
    Dev<uint64_t> rows;
    Pair<uint8_t> text;
    Pair<uint8_t> in;  // the staging blob, filled by the caller between begin and submit, and its device mirror
    size_t in_bytes{};
    uint64_t n_bytes{};
    int busy{};
    TextSlot() = default;
    TextSlot(const TextSlot &) = delete;
    TextSlot &operator=(const TextSlot &) = delete;
    int init() {
        SGK_HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        return hdr.ensure(1);
    }
    ~TextSlot() {
        if (stream) (void)hipStreamDestroy(stream);  // (drained by pipe_destroy)
    }
};

// a pipe (int device; struct Slot : TextSlot {...} slot[2]) on `device`, both streams made
template <class Pipe>
static inline int pipe_create(int device, Pipe **out) {
    *out = nullptr;
    const int ndev = sgk_device_count();
    if (ndev <= 0) return SGK_ERR_NODEVICE;
    if (device < 0 || device >= ndev) return SGK_ERR_ARG;
    SGK_HIP_TRY(hipSetDevice(device));
    Pipe *p = new (std::nothrow) Pipe();
    if (!p) return SGK_ERR_NOMEM;
    p->device = device;
    int rc = p->slot[0].init();
    if (rc == SGK_OK) rc = p->slot[1].init();
    if (rc != SGK_OK) {
        delete p;
        return rc;
    }
    *out = p;
    return SGK_OK;
}

// both streams drained before any buffer of either slot, a grammar's own included, is freed
template <class Pipe>
static inline void pipe_destroy(Pipe *p) {
    if (!p) return;
    for (TextSlot &S : p->slot) (void)hipStreamSynchronize(S.stream);
    delete p;
}

// what begin, submit and wait open with: the slot, which must be busy or idle as the call needs it, on the pipe's device
template <class Pipe>
static inline int pipe_slot(Pipe *p, int slot, bool busy, typename Pipe::Slot **out) {
    if (!p || slot < 0 || slot > 1 || (p->slot[slot].busy != 0) != busy) return SGK_ERR_ARG;
    SGK_HIP_TRY(hipSetDevice(p->device));
    *out = &p->slot[slot];
    return SGK_OK;
}

// submit: an idle slot that has had a begin; body(slot) uploads and enqueues the batch
template <class Pipe, class Body>
static inline int pipe_submit(Pipe *p, int slot, Body body) {
    typename Pipe::Slot *S;
    SGK_TRY(pipe_slot(p, slot, false, &S));
    if (!S->in.h.p) return SGK_ERR_ARG;
    S->n_bytes = 0;
    SGK_TRY(body(*S));
    S->busy = 1;
    return SGK_OK;
}

// measure -> size -> write -> download on the slot's stream; measure(), write(): the grammar's calls, bound to the batch,
// its workspace S.ws.p of ws_bytes, its row offsets S.rows.p and (write) its text S.text.d.p of S.n_bytes.
// Returns once the size is known; the text and the header with the write pass's flags are then on their way.
template <class Measure, class Write>
static inline int text_pipe_run(TextSlot &S, size_t ws_bytes, size_t n_rows, Measure measure, Write write) {
    SGK_TRY(S.ws.ensure_bytes(ws_bytes));
    SGK_TRY(S.rows.ensure(n_rows + 1));
    SGK_TRY(measure());
    SGK_HIP_TRY(hipMemcpyAsync(S.hdr.p, S.ws.p, sizeof(TextHdr), hipMemcpyDeviceToHost, S.stream));
    SGK_HIP_TRY(hipStreamSynchronize(S.stream));
    if (S.hdr.p->flags & TEXT_FLAG_WORKSPACE) return SGK_ERR_WORKSPACE;
    S.n_bytes = S.hdr.p->n_bytes;
    SGK_TRY(S.text.d.ensure_bytes(S.n_bytes + 16));  // (+ 16: wait hands out a pointer for an empty text too)
    SGK_TRY(S.text.h.ensure_bytes(S.n_bytes + 16));
    SGK_TRY(write());
    SGK_TRY(S.text.down(S.n_bytes, S.stream));
    SGK_HIP_TRY(hipMemcpyAsync(S.hdr.p, S.ws.p, sizeof(TextHdr), hipMemcpyDeviceToHost, S.stream));
    return SGK_OK;
}

// wait: the slot is idle again whatever became of its batch.  The header is looked at only if there is text: a submit
// that ended before its text pass (ss: no record, or none in front of the first bad one) left an earlier batch's header
// there, and a write pass over tiles of no bytes (n_bytes == 0 is their sum) cannot overflow, so nothing is missed.
static inline int text_pipe_finish(TextSlot &S, const uint8_t **text, uint64_t *n_bytes) {
    S.busy = 0;
    SGK_HIP_TRY(hipStreamSynchronize(S.stream));
    if (S.n_bytes && (S.hdr.p->flags & TEXT_FLAG_OVERFLOW)) return SGK_ERR_CAPACITY;
    *text = S.text.h.p;
    *n_bytes = S.n_bytes;
    return SGK_OK;
}

#pragma GCC visibility pop
}  // namespace sgk
