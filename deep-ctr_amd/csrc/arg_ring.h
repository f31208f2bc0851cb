// arg_ring.h -- how the argument arrays of the group calls reach the device (fm_api.hip, fnn_api.hip, ipnn_api.hip).
//
// The per-model argument array of a group call (fm_train_online_multi, fm_train_step_multi, fnn_train_step_multi, and the
// evaluation calls fm_ / fnn_ / ipnn_predict_multi and fm_ / fnn_ / ipnn_eval_multi, the range flags' kernel of the last
// included) goes through a pinned host ring and its device image, both of the handle in front (hs[0]): a launch's
// array is written into the next free slots of the one and copied to the same slots of the other on hs[0]'s stream.  The copy is
// asynchronous, so a slot is the copy's to read until the copy has run: slots are handed out in order and never rewritten before
// the ring wraps, and a wrap first waits for the event recorded after the latest copy (all copies are on one stream, in order,
// so that covers every one of them).  The ring persists from call to call for the same reason.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace fnn {

struct ArgRing {
    size_t elem, cap;          // bytes per element, elements per ring
    void* host = nullptr; void* dev = nullptr; size_t cur = 0; hipEvent_t copied = nullptr;
    template <typename T> T* at_host(size_t slot) const { return static_cast<T*>(host) + slot; }
    template <typename T> const T* at_dev(size_t slot) const { return static_cast<const T*>(dev) + slot; }
    // (a ring whose element type is chosen per launch: by bytes, `elem` per slot)
    char* host_bytes(size_t slot) const { return static_cast<char*>(host) + slot * elem; }
    const char* dev_bytes(size_t slot) const { return static_cast<const char*>(dev) + slot * elem; }
};

// n elements of the ring, *slot the first of them.  Allocates on first use, every piece guarded, so that a call that failed half
// way can be made again; a wrap waits for the latest copy.
inline hipError_t ring_take(ArgRing& r, size_t n, size_t* slot)
{
    hipError_t e = hipSuccess;
    if (!r.copied && (e = hipEventCreateWithFlags(&r.copied, hipEventDisableTiming)) != hipSuccess) return e;
    if (!r.dev && (e = hipMalloc(&r.dev, r.cap * r.elem)) != hipSuccess) return e;
    if (!r.host && (e = hipHostMalloc(&r.host, r.cap * r.elem, hipHostMallocDefault)) != hipSuccess) return e;
    if (r.cur + n > r.cap) {
        if ((e = hipEventSynchronize(r.copied)) != hipSuccess) return e;
        r.cur = 0;
    }
    *slot = r.cur;
    r.cur += n;
    return hipSuccess;
}
// the n elements written at `slot` of the host ring, to the device image on stream `st` (hs[0]'s)
inline hipError_t ring_send(ArgRing& r, size_t slot, size_t n, hipStream_t st)
{
    const hipError_t e = hipMemcpyAsync(static_cast<char*>(r.dev) + slot * r.elem, r.host_bytes(slot), n * r.elem, hipMemcpyHostToDevice, st);
    return e != hipSuccess ? e : hipEventRecord(r.copied, st);
}
inline void ring_release(ArgRing& r)
{
    if (r.dev) hipFree(r.dev);
    if (r.host) hipHostFree(r.host);
    if (r.copied) hipEventDestroy(r.copied);
    r.dev = r.host = nullptr; r.copied = nullptr; r.cur = 0;
}

}  // namespace fnn
