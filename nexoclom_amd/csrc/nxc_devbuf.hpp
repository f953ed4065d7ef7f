// Host-only owner of one device allocation: DevBuf<T, Alloc> holds a pointer and the bytes it was
// asked for, grows only, and frees itself.  Plain C++ without a device call: the device comes in
// through Alloc, a policy of three static functions that return a status (0: done)
//     int alloc(void **ptr, size_t bytes);   int free(void *ptr);   int flush();
// nxc_api.hip supplies the HIP one.  The policy is there so that a stand-alone program can put a
// counting, failing fake in its place and run the error paths under the host sanitizers
// (tests/tools/devbuf_check.cpp); it is no extension point.
#pragma once

#include <cstddef>

template <typename T, class Alloc>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;                  // bytes the block was asked for (0 with a block: ensure(0))

    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            (void)release();
            p = o.p; cap = o.cap;
            o.p = nullptr; o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { (void)release(); }

    // Empty first, then the free: a free that fails is reported and can never be repeated.
    int release()
    {
        T *old = p;
        p = nullptr;
        cap = 0;
        return old ? Alloc::free(old) : 0;
    }

    // Room for `bytes`, grow-only: a block that is large enough stays (and keeps its contents), a
    // new one has none of the old contents.  A refused allocation is tried once more after
    // Alloc::flush(); on failure the buffer is empty.
    int ensure(size_t bytes)
    {
        if (cap >= bytes && p) return 0;
        if (int rc = release()) return rc;
        void *q = nullptr;
        int rc = Alloc::alloc(&q, bytes ? bytes : 8);
        if (rc) {
            (void)Alloc::flush();
            if ((rc = Alloc::alloc(&q, bytes ? bytes : 8))) return rc;
        }
        p = static_cast<T *>(q);
        cap = bytes;
        return 0;
    }

    T *get() const { return p; }
    operator T *() const { return p; }       // h->d_x + offset, if (h->d_x), a kernel's T * argument
};
