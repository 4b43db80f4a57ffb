// device_mem.h -- the one owner of device and pinned-host memory (host code only).  A context struct keeps raw pointers for its
// kernels and one Arena per lifetime that frees them: nothing is listed twice, and a buffer added to a context cannot be forgotten in
// its free path.  A function that can fail half way builds into a local Arena and hands it to the context's (adopt) once everything,
// launches included, has succeeded; a temporary is a local Arena that is never handed over.
//
// The allocate / free pair is the template parameter Mem (HipMem by default), so that the bookkeeping also runs on malloc / free where
// there is no device (tests/host/arena_check.cpp; define MGPT_DEVICE_MEM_NO_HIP to leave the HIP runtime out of the header).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <initializer_list>
#include <utility>
#include <vector>

#ifndef MGPT_DEVICE_MEM_NO_HIP
#include <hip/hip_runtime.h>
#endif

namespace mgpt {

// live allocations and bytes of every Arena of the process (mgpt_mem_debug); touched only where memory is allocated or freed
struct MemCounters {
    static inline std::atomic<int64_t> allocs{0}, bytes{0};
};

#ifndef MGPT_DEVICE_MEM_NO_HIP
struct HipMem {
    using Error = hipError_t;
    static constexpr Error ok = hipSuccess;
    static Error alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static Error alloc_host(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void free(void *p) { (void)hipFree(p); }               // (waits for the work that still uses p)
    static void free_host(void *p) { (void)hipHostFree(p); }
};
#else
struct HipMem;
#endif

template <class Mem = HipMem>
class Arena {
public:
    using Error = typename Mem::Error;

    Arena() = default;
    Arena(const Arena &) = delete;
    Arena &operator=(const Arena &) = delete;
    Arena(Arena &&o) noexcept : recs_(std::move(o.recs_)) { o.recs_.clear(); }
    Arena &operator=(Arena &&o) noexcept
    {
        if (this != &o) { release(); recs_ = std::move(o.recs_); o.recs_.clear(); }
        return *this;
    }
    ~Arena() { release(); }

    // *p = new device memory (nullptr on failure); owned by this arena from here on
    template <class T>
    Error alloc(T **p, size_t bytes) { return record(reinterpret_cast<void **>(p), bytes, false); }
    // ... pinned host memory
    template <class T>
    Error alloc_host(T **p, size_t bytes) { return record(reinterpret_cast<void **>(p), bytes, true); }

    // one request of alloc_all: where the pointer goes and how many bytes of device memory it gets
    struct Request {
        void **p;
        size_t bytes;
        template <class T>
        Request(T **p_, size_t bytes_) : p(reinterpret_cast<void **>(p_)), bytes(bytes_) {}
    };
    // the requests in order, up to the first failure, whose error it returns: the failed pointer and every later one are nullptr, what
    // was allocated before it is owned by this arena (a caller that gives up releases the arena, or lets a local one go out of scope)
    Error alloc_all(std::initializer_list<Request> requests)
    {
        for (const Request &r : requests) *r.p = nullptr;
        for (const Request &r : requests) {
            const Error e = record(r.p, r.bytes, false);
            if (e != Mem::ok) return e;
        }
        return Mem::ok;
    }

    // frees everything, latest first; the arena is empty and usable afterwards.  (The owner's pointers dangle: it resets itself as a whole.)
    void release()
    {
        for (size_t i = recs_.size(); i-- > 0;) {
            const Rec &r = recs_[i];
            if (r.host) Mem::free_host(r.p); else Mem::free(r.p);
            MemCounters::allocs.fetch_sub(1, std::memory_order_relaxed);
            MemCounters::bytes.fetch_sub((int64_t)r.bytes, std::memory_order_relaxed);
        }
        recs_.clear();
    }

    // takes over everything o owns (behind what this arena already has); o is left empty
    void adopt(Arena &&o)
    {
        recs_.insert(recs_.end(), o.recs_.begin(), o.recs_.end());
        o.recs_.clear();
    }

    bool empty() const { return recs_.empty(); }
    size_t count() const { return recs_.size(); }

private:
    struct Rec { void *p; size_t bytes; bool host; };
    std::vector<Rec> recs_;

    Error record(void **p, size_t bytes, bool host)
    {
        *p = nullptr;
        recs_.reserve(recs_.size() + 1);                           // (so that nothing can fail between the allocation and its record)
        const Error e = host ? Mem::alloc_host(p, bytes) : Mem::alloc(p, bytes);
        if (e != Mem::ok) { *p = nullptr; return e; }
        if (*p == nullptr) return e;                               // (zero bytes: nothing to own)
        recs_.push_back({*p, bytes, host});
        MemCounters::allocs.fetch_add(1, std::memory_order_relaxed);
        MemCounters::bytes.fetch_add((int64_t)bytes, std::memory_order_relaxed);
        return e;
    }
};

#ifndef MGPT_DEVICE_MEM_NO_HIP
using DeviceArena = Arena<>;
#endif

}  // namespace mgpt
