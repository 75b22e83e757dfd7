// mr_devmem.hpp — host only: where device memory, streams and events come from and
// the move-only owners that give them back (DESIGN.md "Who owns what").
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <unordered_map>
#include <utility>
#include <vector>

namespace mr {

// Plan buffers come from a cache of freed device blocks (size classes per device: powers
// of two up to 64 MiB, 64 MiB steps above): a plan for each fresh batch then costs no
// hipMalloc / hipFree (tens of microseconds each, milliseconds for large blocks).  A
// block returns to the cache when its plan is destroyed, after mr_plan_destroy has
// waited for the plan's work; the cache keeps up to 16 GiB and is emptied before a
// hipMalloc that would otherwise fail.
struct BlockCache {
    std::mutex mu;
    std::unordered_map<void *, std::pair<int, size_t>> live;  // block -> (device, class bytes)
    std::unordered_map<uint64_t, std::vector<void *>> free;   // (device, class) -> blocks
    size_t cached = 0;
};
inline BlockCache &block_cache() {
    static BlockCache *c = new BlockCache();  // never destroyed: plans may outlive static destructors
    return *c;
}
inline size_t size_class(size_t b) {
    constexpr size_t kBig = size_t(64) << 20;
    if (b > kBig) return (b + kBig - 1) / kBig * kBig;
    size_t c = 256;
    while (c < b) c <<= 1;
    return c;
}
inline uint64_t cache_key(int dev, size_t cls) { return (uint64_t(cls) << 8) | uint64_t(dev & 0xFF); }
// hipFree every cached block (dev >= 0: of that device only); the caller holds the lock
inline void trim_cache(int dev) {
    BlockCache &c = block_cache();
    for (auto &kv : c.free) {
        if (dev >= 0 && int(kv.first & 0xFF) != (dev & 0xFF)) continue;
        for (void *q : kv.second) {
            (void)hipFree(q);
            c.cached -= size_t(kv.first >> 8);
        }
        kv.second.clear();
    }
}
inline void trim_cache_all() {
    std::lock_guard<std::mutex> lk(block_cache().mu);
    trim_cache(-1);
}
inline hipError_t pmalloc(void **p, size_t bytes) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const size_t cls = size_class(std::max<size_t>(bytes, 1));
    BlockCache &c = block_cache();
    std::lock_guard<std::mutex> lk(c.mu);
    auto it = c.free.find(cache_key(dev, cls));
    if (it != c.free.end() && !it->second.empty()) {
        *p = it->second.back();
        it->second.pop_back();
        c.cached -= cls;
        c.live[*p] = {dev, cls};
        return hipSuccess;
    }
    hipError_t e = hipMalloc(p, cls);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        trim_cache(dev);
        e = hipMalloc(p, cls);
    }
    if (e == hipSuccess) c.live[*p] = {dev, cls};
    return e;
}
inline void pfree(void *p) {
    if (!p) return;
    BlockCache &c = block_cache();
    std::lock_guard<std::mutex> lk(c.mu);
    auto it = c.live.find(p);
    if (it == c.live.end()) {
        (void)hipFree(p);
        return;
    }
    const int dev = it->second.first;
    const size_t cls = it->second.second;
    c.live.erase(it);
    if (c.cached + cls > (size_t(16) << 30)) {
        (void)hipFree(p);
        return;
    }
    c.free[cache_key(dev, cls)].push_back(p);
    c.cached += cls;
}
// the cache-managed blocks that live objects hold: their count and class bytes
inline void cache_live(uint64_t *blocks, uint64_t *bytes) {
    BlockCache &c = block_cache();
    std::lock_guard<std::mutex> lk(c.mu);
    uint64_t b = 0;
    for (const auto &kv : c.live) b += kv.second.second;
    if (blocks) *blocks = c.live.size();
    if (bytes) *bytes = b;
}
// hipMalloc past the cache, for the grid's long-lived device tables (no size-class
// rounding): on out-of-memory the cache is trimmed and the allocation retried once
inline hipError_t dev_malloc(void **p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        trim_cache_all();
        e = hipMalloc(p, bytes);
    }
    return e;
}

// Plan streams come from a per-device pool as well: a destroyed plan (which waited for
// its work) returns its streams, and the next plan takes them without hipStreamCreate.
struct StreamPool {
    std::mutex mu;
    std::vector<std::pair<int, hipStream_t>> free;
};
inline StreamPool &stream_pool() {
    static StreamPool *p = new StreamPool();
    return *p;
}
inline hipError_t pstream_create(hipStream_t *s) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        StreamPool &p = stream_pool();
        std::lock_guard<std::mutex> lk(p.mu);
        for (size_t i = p.free.size(); i-- > 0;)
            if (p.free[i].first == dev) {
                *s = p.free[i].second;
                p.free.erase(p.free.begin() + long(i));
                return hipSuccess;
            }
    }
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}
inline void pstream_release(hipStream_t s) {
    if (!s) return;
    int dev = 0;
    (void)hipGetDevice(&dev);
    StreamPool &p = stream_pool();
    std::lock_guard<std::mutex> lk(p.mu);
    if (p.free.size() >= 64) {
        (void)hipStreamDestroy(s);
        return;
    }
    p.free.emplace_back(dev, s);
}

// `bytes` of device memory cleared to zero before this returns.  hipMemset on device memory
// only queues the fill on the null stream and returns (a 16 GiB fill: 4 us, then 2.8 ms of
// work), and the plans' streams are non-blocking: they do not wait for the null stream.  A
// kernel launched on one of them right afterwards could run before the fill, which then
// wipes what the kernel counted; with other host threads' copies queued on the null stream
// the fill can be milliseconds late.  So the fill is waited for here.
inline hipError_t zero_now(void *p, size_t bytes) {
    hipError_t e = hipMemsetAsync(p, 0, bytes, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    return e;
}

// ---- owners (move-only; an empty one holds nothing and releases nothing) ----
enum class DevMem { cache, direct };  // block cache (plans, temporaries) | plain hipMalloc (grid tables)

// `count` elements of T on the device; the way it was allocated is the way it is freed
template <class T>
class DevBuf {
    T *p_ = nullptr;
    size_t n_ = 0;
    DevMem how_ = DevMem::cache;

public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), n_(o.n_), how_(o.how_) { o.p_ = nullptr, o.n_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_, n_ = o.n_, how_ = o.how_;
            o.p_ = nullptr, o.n_ = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    // replaces what it held; on an error it is left empty
    hipError_t alloc(size_t count, DevMem how = DevMem::cache) {
        reset();
        void *p = nullptr;
        const hipError_t e = how == DevMem::cache ? pmalloc(&p, count * sizeof(T)) : dev_malloc(&p, count * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T *>(p), n_ = count, how_ = how;
        return hipSuccess;
    }
    // allocates and clears to zero bytes (the zeros are there when it returns: zero_now)
    hipError_t alloc_zero(size_t count, DevMem how = DevMem::cache) {
        hipError_t e = alloc(count, how);
        if (e == hipSuccess) e = zero_now(p_, count * sizeof(T));
        return e;
    }
    void reset() {
        if (p_ && how_ == DevMem::cache) pfree(p_);
        else if (p_) (void)hipFree(p_);
        p_ = nullptr, n_ = 0;
    }
    T *get() const { return p_; }
    size_t size() const { return n_; }
    explicit operator bool() const { return p_ != nullptr; }
};

// max(h.size(), 1) elements holding a copy of h
template <class T>
hipError_t upload(DevBuf<T> &d, const std::vector<T> &h, DevMem how = DevMem::cache) {
    hipError_t e = d.alloc(std::max<size_t>(h.size(), 1), how);
    if (e == hipSuccess && !h.empty()) e = hipMemcpy(d.get(), h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) d.reset();
    return e;
}

// a stream of the pool
class Stream {
    hipStream_t s_ = nullptr;

public:
    Stream() = default;
    Stream(Stream &&o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    Stream &operator=(Stream &&o) noexcept {
        std::swap(s_, o.s_);
        return *this;
    }
    ~Stream() { pstream_release(s_); }
    hipError_t create() { return s_ ? hipSuccess : pstream_create(&s_); }
    hipStream_t get() const { return s_; }
    explicit operator bool() const { return s_ != nullptr; }
};

class Event {
    hipEvent_t e_ = nullptr;

public:
    Event() = default;
    Event(Event &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event &operator=(Event &&o) noexcept {
        std::swap(e_, o.e_);
        return *this;
    }
    ~Event() {
        if (e_) (void)hipEventDestroy(e_);
    }
    hipError_t create(unsigned flags = hipEventDefault) {
        return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags);
    }
    hipEvent_t get() const { return e_; }
    explicit operator bool() const { return e_ != nullptr; }
};

}  // namespace mr
