// resources.hpp — the owning handles of the context's GPU resources: device memory, pinned host
// memory, events and streams.  Each is move-only, releases in its destructor, and converts to the raw
// handle it owns, so a HIP call takes it as it took the raw pointer.  The release calls of the HIP
// runtime appear in this header and nowhere else in csrc/.  Private to csrc/: not installed.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace rrte {

// One device allocation, untyped: what DeviceBuf<T> is made of and what the context's graveyard
// holds (a DeviceBuf<T> of any T moves into it).
class DeviceMem {
public:
    DeviceMem() = default;
    DeviceMem(DeviceMem&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    ~DeviceMem() { reset(); }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }

protected:
    void* p_ = nullptr;
    size_t cap_ = 0;  // elements of the typed view
};

// A device buffer of cap() elements of T.
template <typename T>
class DeviceBuf : public DeviceMem {
public:
    T* get() const { return static_cast<T*>(p_); }
    operator T*() const { return get(); }
    size_t cap() const { return cap_; }
    // Releases what it holds and allocates n elements (empty on failure).
    hipError_t alloc(size_t n) {
        reset();
        const hipError_t e = hipMalloc(&p_, n * sizeof(T));
        if (e == hipSuccess) cap_ = n;
        else p_ = nullptr;
        return e;
    }
};

// Page-locked host memory of cap() elements of T, allocated with `flags` (hipHostMalloc*), which it
// keeps for grow().
template <typename T>
class PinnedBuf {
public:
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { reset(); }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t cap() const { return cap_; }
    void reset() {
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    hipError_t alloc(size_t n, unsigned flags = hipHostMallocDefault) {
        reset();
        flags_ = flags;
        const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T), flags);
        if (e == hipSuccess) cap_ = n;
        else p_ = nullptr;
        return e;
    }
    // At least n elements: a smaller buffer is freed, then a larger one allocated (contents are not
    // kept).  The caller guarantees that no copy into or out of the old buffer is pending.
    hipError_t grow(size_t n) { return n <= cap_ && p_ ? hipSuccess : alloc(n, flags_); }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
    unsigned flags_ = hipHostMallocDefault;
};

// An event, created on demand: without timing unless asked (the frame timers ev0 / ev1 / ev2).
class Event {
public:
    Event() = default;
    Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        std::swap(e_, o.e_);
        return *this;
    }
    ~Event() {
        if (e_) (void)hipEventDestroy(e_);
    }
    hipEvent_t get() const { return e_; }
    operator hipEvent_t() const { return e_; }
    // Creates the event if there is none yet.
    hipError_t create(bool timing = false) {
        if (e_) return hipSuccess;
        return timing ? hipEventCreate(&e_) : hipEventCreateWithFlags(&e_, hipEventDisableTiming);
    }

private:
    hipEvent_t e_ = nullptr;
};

// A non-blocking stream the context owns (caller streams stay raw hipStream_t).
class Stream {
public:
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() {
        if (s_) (void)hipStreamDestroy(s_);
    }
    hipStream_t get() const { return s_; }
    operator hipStream_t() const { return s_; }
    // Creates the stream if there is none yet.
    hipError_t create() { return s_ ? hipSuccess : hipStreamCreateWithFlags(&s_, hipStreamNonBlocking); }
    hipError_t create(int priority) {
        return s_ ? hipSuccess : hipStreamCreateWithPriority(&s_, hipStreamNonBlocking, priority);
    }

private:
    hipStream_t s_ = nullptr;
};

}  // namespace rrte
