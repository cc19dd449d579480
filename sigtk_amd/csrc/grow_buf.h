// grow_buf.h -- the growing buffers of the host layer: device and pinned host memory that frees itself.  The job units
// (job.h) and the text pipes (text_pipe.h) keep every buffer they own in one of these.
#pragma once
#include "sgk_common.h"

namespace sgk {

enum class Mem { Dev, Pin };

// `count` elements of T in device or pinned host memory.  Only ever grows, with some slack (batches vary a little), so
// that a job recycled batch after batch stops allocating after the first few.
template <typename T, Mem M>
struct Grow {
    T *p = nullptr;
    size_t cap = 0;  // bytes
    Grow() = default;
    Grow(const Grow &) = delete;
    Grow &operator=(const Grow &) = delete;
    ~Grow() {
        if (p) (void)(M == Mem::Dev ? hipFree(p) : hipHostFree(p));
    }
    int ensure(size_t count) { return ensure_bytes(count * sizeof(T)); }
    int ensure_bytes(size_t bytes) {
        if (bytes <= cap) return SGK_OK;
        if (p) SGK_HIP_TRY(M == Mem::Dev ? hipFree(p) : hipHostFree(p));
        p = nullptr;
        cap = 0;
        const size_t want = round_up(bytes + bytes / 8, 4096);
        void *q = nullptr;
        SGK_HIP_TRY(M == Mem::Dev ? hipMalloc(&q, want) : hipHostMalloc(&q, want, hipHostMallocDefault));
        p = static_cast<T *>(q);
        cap = want;
        return SGK_OK;
    }
};
template <typename T> using Dev = Grow<T, Mem::Dev>;
template <typename T> using Pin = Grow<T, Mem::Pin>;

// a buffer that holds different element types under different result kinds
template <Mem M>
struct Bytes : Grow<uint8_t, M> {
    template <typename T>
    T *as() const {
        return reinterpret_cast<T *>(this->p);
    }
};

// room for `bytes` in dst (64 at least), then the copy -- none for an empty range
template <typename B>
static inline int grow_copy(B &dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t st) {
    SGK_TRY(dst.ensure_bytes(bytes ? bytes : 64));
    if (bytes) SGK_HIP_TRY(hipMemcpyAsync(dst.p, src, bytes, kind, st));
    return SGK_OK;
}
static inline int fetch(Grow<uint8_t, Mem::Pin> &h, const void *d, size_t bytes, hipStream_t st) {
    return grow_copy(h, d, bytes, hipMemcpyDeviceToHost, st);
}

// pinned staging `h` and its device mirror `d`: `count` elements up or down on the stream
template <typename T>
struct Pair {
    Pin<T> h;
    Dev<T> d;
    int up(size_t count, hipStream_t st) { return grow_copy(d, h.p, count * sizeof(T), hipMemcpyHostToDevice, st); }
    int down(size_t count, hipStream_t st) { return grow_copy(h, d.p, count * sizeof(T), hipMemcpyDeviceToHost, st); }
};

}  // namespace sgk
