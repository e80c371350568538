// dev_mem.h — ownership of device and pinned allocations (DESIGN.md §Memory ownership).
//
// dev_mem.cpp is the one unit in csrc/ that calls the runtime's allocation and free functions;
// everything else allocates through a dev_pool, which frees what it still holds when it dies.
// Ownership only: no reference counts, no sub-allocation, no caching — one get is one runtime
// allocation of exactly the bytes asked for.
//
// Standard headers only (a host test builds this with a plain C++ compiler against its own backend).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <string>
#include <utility>
#include <vector>

typedef struct ihipStream_t *hipStream_t;  // as <hip/hip_runtime.h> declares it

namespace ghip {

void set_error(const std::string &msg);

enum mem_kind { MEM_DEVICE, MEM_UNCACHED, MEM_PINNED };

struct mem_backend {
    void *(*alloc)(mem_kind k, size_t bytes);            // nullptr when the runtime refuses
    void (*free)(mem_kind k, void *p);
    int (*zero)(void *p, size_t bytes, hipStream_t s);   // stream-ordered memset to 0; 0 = queued
};
const mem_backend *hip_backend();  // dev_mem.cpp

// live allocations of every pool in the process (gemma_hip_mem_live)
inline std::atomic<int64_t> g_mem_live_allocs{0}, g_mem_live_bytes{0};

class dev_pool {
  public:
    explicit dev_pool(const mem_backend *b = hip_backend()) : be_(b) {}
    dev_pool(dev_pool &&o) noexcept : be_(o.be_), live_(std::move(o.live_)) { o.live_.clear(); }
    dev_pool(const dev_pool &) = delete;
    dev_pool &operator=(const dev_pool &) = delete;
    ~dev_pool() { clear(); }

    // 0, or -1 with the error set and *p = nullptr.  A zero-size request is no allocation: *p = nullptr, 0.
    template <class T> int get(T **p, size_t bytes, mem_kind k = MEM_DEVICE) {
        *p = (T *)take(bytes, k);
        return *p || !bytes ? 0 : -1;
    }
    // device memory zeroed on stream s, the stream of whatever fills it next (non-blocking streams do
    // not order against the null stream)
    template <class T> int get_zeroed(T **p, size_t bytes, hipStream_t s, mem_kind k = MEM_DEVICE) {
        if (get(p, bytes, k)) return -1;
        if (!bytes || be_->zero(*p, bytes, s) == 0) return 0;
        set_error("dev_pool: zeroing " + std::to_string(bytes) + " bytes failed");
        put(*p);
        return -1;
    }
    // frees one allocation of this pool and nulls the pointer; nullptr is a no-op.  A pointer the pool
    // does not hold sets the error and is left alone: nothing foreign ever reaches the runtime.
    template <class T> void put(T *&p) {
        if (!p) return;
        for (size_t i = live_.size(); i-- > 0;)
            if (live_[i].p == (void *)p) {
                release(live_[i]);
                live_.erase(live_.begin() + (ptrdiff_t)i);
                p = nullptr;
                return;
            }
        set_error("dev_pool: put of a pointer this pool does not own");
    }
    void clear() {
        for (size_t i = live_.size(); i-- > 0;) release(live_[i]);
        live_.clear();
    }
    size_t count() const { return live_.size(); }

  private:
    struct entry {
        void *p;
        size_t bytes;
        mem_kind k;
    };
    void *take(size_t bytes, mem_kind k) {
        if (!bytes) return nullptr;
        void *p = be_->alloc(k, bytes);
        if (!p) {
            set_error("dev_pool: allocation of " + std::to_string(bytes) + " bytes failed");
            return nullptr;
        }
        live_.push_back({p, bytes, k});
        g_mem_live_allocs += 1;
        g_mem_live_bytes += (int64_t)bytes;
        return p;
    }
    void release(const entry &en) {
        be_->free(en.k, en.p);
        g_mem_live_allocs -= 1;
        g_mem_live_bytes -= (int64_t)en.bytes;
    }
    const mem_backend *be_;
    std::vector<entry> live_;
};

}  // namespace ghip
