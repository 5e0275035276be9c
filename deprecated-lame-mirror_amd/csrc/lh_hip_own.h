/*
 * lh_hip_own.h -- move-only owners of the HIP resources the host layer holds (lh_api.cpp, lh_batch.cpp):
 * device memory, pinned host memory, events and streams.  Each releases what it holds in its destructor,
 * so a handle or a batch frees its resources by being deleted -- on its own device: the owner's
 * destructor runs wherever `delete' does, inside the caller's LhDeviceScope.
 *
 * Host only; no .hip file includes this.
 */
#ifndef LH_HIP_OWN_H
#define LH_HIP_OWN_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <utility>

/* (nothing of this may show up among the library's dynamic symbols) */
#pragma GCC visibility push(hidden)

/* memory of `cap()' elements, on the device or pinned on the host: what LhDevBuf and LhPinned are made of */
template < typename T, bool pinned > class LhBuf {
    T      *p_ = nullptr;
    size_t  cap_ = 0;
  public:
    LhBuf() = default;
    LhBuf(const LhBuf &) = delete;
    LhBuf & operator=(const LhBuf &) = delete;
    LhBuf(LhBuf && o) noexcept:p_(o.p_), cap_(o.cap_) {
        o.p_ = nullptr;
        o.cap_ = 0;
    }
    LhBuf & operator=(LhBuf && o) noexcept {
        if (this != &o) {
            release();
            p_ = o.p_;
            cap_ = o.cap_;
            o.p_ = nullptr;
            o.cap_ = 0;
        }
        return *this;
    }
    ~LhBuf() {
        release();
    }
    T      *get() const {
        return p_;
    }
    size_t  cap() const {
        return cap_;
    }
    /* n elements in place of whatever was held (released first: the caller wants its memory back before it asks) */
    hipError_t alloc(size_t n) {
        void   *p = nullptr;
        release();
        hipError_t const e = pinned ? hipHostMalloc(&p, n * sizeof(T), 0) : hipMalloc(&p, n * sizeof(T));
        if (e == hipSuccess && p) {
            p_ = (T *) p;
            cap_ = n;
        }
        return e;
    }
    /* Room for n elements.  Within the capacity nothing happens; beyond it n + slack elements are allocated FIRST -- a failed
     * allocation leaves the old buffer and its capacity in place --, then `drain', when given, is synchronised (work queued
     * on it may still be reading the old buffer), then the old buffer is freed.  Contents are not carried over.
     * *replaced says whether get() changed. */
    hipError_t reserve(size_t n, size_t slack = 0, hipStream_t drain = nullptr, bool *replaced = nullptr) {
        if (replaced)
            *replaced = false;
        if (n <= cap_)
            return hipSuccess;
        LhBuf   bigger;
        hipError_t e = bigger.alloc(n + slack);
        if (e == hipSuccess && drain)
            e = hipStreamSynchronize(drain);
        if (e != hipSuccess)
            return e;
        *this = std::move(bigger);
        if (replaced)
            *replaced = true;
        return hipSuccess;
    }
    void release() {
        if (p_)
            (void) (pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
    }
};

template < typename T > using LhDevBuf = LhBuf < T, false >;   /* hipMalloc / hipFree */
template < typename T > using LhPinned = LhBuf < T, true >;    /* hipHostMalloc / hipHostFree */

/* an event, made when first needed: create() on one that exists does nothing */
class LhEvent {
    hipEvent_t e_ = nullptr;
  public:
    LhEvent() = default;
    LhEvent(const LhEvent &) = delete;
    LhEvent & operator=(const LhEvent &) = delete;
    LhEvent(LhEvent && o) noexcept:e_(o.e_) {
        o.e_ = nullptr;
    }
    LhEvent & operator=(LhEvent && o) noexcept {
        if (this != &o) {
            release();
            e_ = o.e_;
            o.e_ = nullptr;
        }
        return *this;
    }
    ~LhEvent() {
        release();
    }
    operator  hipEvent_t() const {
        return e_;
    }
    hipError_t create(unsigned flags = hipEventDefault) {
        return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags);
    }
    void release() {
        if (e_)
            (void) hipEventDestroy(e_);
        e_ = nullptr;
    }
};

/* a stream, likewise */
class LhStream {
    hipStream_t s_ = nullptr;
  public:
    LhStream() = default;
    LhStream(const LhStream &) = delete;
    LhStream & operator=(const LhStream &) = delete;
    LhStream(LhStream && o) noexcept:s_(o.s_) {
        o.s_ = nullptr;
    }
    LhStream & operator=(LhStream && o) noexcept {
        if (this != &o) {
            release();
            s_ = o.s_;
            o.s_ = nullptr;
        }
        return *this;
    }
    ~LhStream() {
        release();
    }
    operator  hipStream_t() const {
        return s_;
    }
    hipError_t create(unsigned flags = hipStreamDefault) {
        return s_ ? hipSuccess : hipStreamCreateWithFlags(&s_, flags);
    }
    void release() {
        if (s_)
            (void) hipStreamDestroy(s_);
        s_ = nullptr;
    }
};

#pragma GCC visibility pop

#endif /* LH_HIP_OWN_H */
