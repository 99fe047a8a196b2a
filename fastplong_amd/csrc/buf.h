/*
 * buf.h -- what the host layer owns: device memory (DevBuf), page-locked host memory (PinBuf), events and streams (Event, Stream).
 *
 * A buffer is a pointer and the number of elements behind it.  It is freed exactly once (not copyable), its capacity is what
 * was allocated and never shrinks, and a grow empties it before it allocates, so a failed allocation leaves an empty buffer
 * and no dangling pointer.  A grow of device memory waits for the whole device first -- kernels and copies in flight may
 * still use the old block --, a grow of page-locked memory does not.  Callers say what they need and read .ptr.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace fpl {

struct DeviceMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static void release(void* p) { (void)hipFree(p); }
    static hipError_t before_grow() { return hipDeviceSynchronize(); }
};
struct PinnedMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void release(void* p) { (void)hipHostFree(p); }
    static hipError_t before_grow() { return hipSuccess; }
};

/* what a grow asks for: a quarter of headroom, so that a run whose batches differ a little in size does not reallocate on every
   batch, plus the call site's own constant; `limit` where the capacity goes on into a 32-bit field */
inline size_t grown(size_t need, size_t extra, size_t limit = SIZE_MAX) {
    const size_t want = need + need / 4 + extra;
    return want < limit ? want : limit;
}

template <class T, class Mem>
struct Buf {
    T* ptr = nullptr;
    size_t cap = 0; /* elements */
    struct Want {   /* one member of a regrow(): the buffer and the elements it is to hold */
        Buf& buf;
        size_t n;
        hipError_t before_grow() const { return Mem::before_grow(); }
    };
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { reset(); }
    void reset() {
        if (ptr) Mem::release(ptr);
        ptr = nullptr;
        cap = 0;
    }
    void swap(Buf& o) {
        T* const p = ptr;
        const size_t c = cap;
        ptr = o.ptr, cap = o.cap;
        o.ptr = p, o.cap = c;
    }
    bool holds(size_t need) const { return ptr && need <= cap; }
    Want want(size_t n) { return Want{*this, n}; }
    /* exactly n elements, at once: for what is made once and for fresh buffers nothing in flight can know */
    hipError_t alloc(size_t n) {
        reset();
        const hipError_t e = Mem::alloc((void**)&ptr, n * sizeof(T));
        if (e == hipSuccess)
            cap = n;
        else
            ptr = nullptr;
        return e;
    }
    /* room for `need` elements; when that takes a new block: need + need / 4 + extra */
    hipError_t grow(size_t need, size_t extra);
};
template <class T> using DevBuf = Buf<T, DeviceMem>;
template <class T> using PinBuf = Buf<T, PinnedMem>;

/* Buffers that are sized by one number grow together: ONE wait, every member emptied, then every member allocated in the order
   given.  A failure on the way empties them all, so the caller's holds() test on any member asks for the grow again. */
template <class W0, class... W>
hipError_t regrow(W0 w0, W... w) {
    hipError_t e = w0.before_grow();
    if (e != hipSuccess) return e;
    w0.buf.reset();
    (w.buf.reset(), ...);
    e = w0.buf.alloc(w0.n);
    ((e = e == hipSuccess ? w.buf.alloc(w.n) : e), ...);
    if (e != hipSuccess) {
        w0.buf.reset();
        (w.buf.reset(), ...);
    }
    return e;
}

template <class T, class Mem>
hipError_t Buf<T, Mem>::grow(size_t need, size_t extra) {
    return holds(need) ? hipSuccess : regrow(want(grown(need, extra)));
}

/* An event or a stream of the host layer: empty until create(), destroyed exactly once (not copyable) -- with its owner, so no list
   of handles has to be kept in step by hand.  It reads as the raw handle wherever a HIP call takes one; `.h` where a void* is made
   of it (BatchArgs). */
template <class H, hipError_t (*Destroy)(H)>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(const Handle&) = delete;
    Handle& operator=(const Handle&) = delete;
    ~Handle() { reset(); }
    void reset() {
        if (h) (void)Destroy(h);
        h = nullptr;
    }
    operator H() const { return h; }
};
struct Event : Handle<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDisableTiming) { return reset(), hipEventCreateWithFlags(&h, flags); }
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> {
    hipError_t create() { return reset(), hipStreamCreateWithFlags(&h, hipStreamNonBlocking); }
};

}  // namespace fpl
