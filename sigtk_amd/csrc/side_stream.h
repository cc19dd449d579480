// side_stream.h -- side streams for kernels that may run beside a launch's main kernel (the packed short reads and the
// whole reads of `event`, the long reads of `stat` / `jnn` / `prefix`): a small pool per device, one fork .. join per
// launch.
//
// Invariant: a thread holds at most one pool mutex, and only between one launcher's fork and join.  It never locks a
// pool mutex while it holds another (side_acquire tries the slots without blocking, then blocks on one holding
// nothing), so concurrent launchers of one process cannot deadlock.
#pragma once
#include <mutex>

#include "sgk_common.h"

namespace sgk {

// one slot of a device's pool: two non-blocking streams, the fork event (recorded on the caller's stream) and a join
// event per stream; its mutex is held while one launch enqueues its fork .. join (the events are the slot's)
struct SideSlot {
    static constexpr int N = 2;
    std::mutex mu;
    bool ok = false;  // (a slot whose creation failed stays unused)
    hipStream_t s[N] = {};
    hipEvent_t fork = nullptr, join[N] = {};
};
// returns a locked slot of the current device (unlock with x->mu.unlock()), or null (api.hip)
SideSlot *side_acquire();

// One fork .. join on up to two side streams: joins on every exit path (an error return in between must not leave the
// caller's stream unordered behind work that still writes the workspace).
struct SideFork {
    SideSlot *x = nullptr;
    hipStream_t main = nullptr;
    int n = 0;
    // records the fork on st and makes the first n_streams (<= 2) side streams wait for it; false: no fork, every
    // stream(i) is st.  (A stream that is being captured into a graph keeps everything in itself: the library's events
    // and streams are not part of the caller's capture.)
    bool open(hipStream_t st, int n_streams) {
        main = st;
        if (n_streams <= 0 || n_streams > SideSlot::N) return false;
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return false;
        x = side_acquire();
        if (!x) return false;
        bool ok = hipEventRecord(x->fork, st) == hipSuccess;
        for (int i = 0; ok && i < n_streams; ++i) ok = hipStreamWaitEvent(x->s[i], x->fork, 0) == hipSuccess;
        if (ok) {
            n = n_streams;
            return true;
        }
        x->mu.unlock();
        x = nullptr;
        return false;
    }
    hipStream_t stream(int i) const { return i < n ? x->s[i] : main; }
    void join() {
        if (!x) return;
        for (int i = 0; i < n; ++i) {
            const bool ok = hipEventRecord(x->join[i], x->s[i]) == hipSuccess &&
                            hipStreamWaitEvent(main, x->join[i], 0) == hipSuccess;
            if (!ok) (void)hipStreamSynchronize(x->s[i]);
        }
        x->mu.unlock();
        x = nullptr;
        n = 0;
    }
    ~SideFork() { join(); }
};

}  // namespace sgk
