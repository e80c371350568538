// dev_mem_test.cpp — dev_pool (gemma.ggml_amd/csrc/dev_mem.h) on the host, over a malloc backend
// that fails its n-th call and poisons what it frees.  Stand-alone: plain C++, nothing from HIP.
//   g++ -std=c++17 -O1 -I gemma.ggml_amd/csrc tests/host/dev_mem_test.cpp -o dev_mem_test && ./dev_mem_test
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>

#include "dev_mem.h"

static std::string g_err;
namespace ghip {
void set_error(const std::string &msg) { g_err = msg; }
}  // namespace ghip
using namespace ghip;

static int g_fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);       \
            ++g_fails;                                                \
        }                                                             \
    } while (0)

// ---- the backend ----------------------------------------------------------------------------------
struct rec {
    size_t bytes;
    mem_kind k;
    int frees;
};
static std::map<void *, rec> g_recs;  // every allocation ever made (freed blocks are kept, poisoned)
static int g_calls = 0, g_fail_at = -1, g_bad_free = 0;
static bool fails_now() { return g_calls++ == g_fail_at; }

static void *t_alloc(mem_kind k, size_t bytes) {
    if (fails_now()) return nullptr;
    void *p = malloc(bytes);
    memset(p, 0xA5, bytes);
    g_recs[p] = {bytes, k, 0};
    return p;
}
static void t_free(mem_kind k, void *p) {
    auto it = g_recs.find(p);
    if (it == g_recs.end() || it->second.frees || it->second.k != k) {  // foreign, double, or wrong kind
        ++g_bad_free;
        return;
    }
    it->second.frees = 1;
    memset(p, 0xDD, it->second.bytes);  // poison; the block itself is released in backend_reset
}
static int t_zero(void *p, size_t bytes, hipStream_t) {
    if (fails_now()) return -1;
    memset(p, 0, bytes);
    return 0;
}
static const mem_backend g_be = {t_alloc, t_free, t_zero};

static int64_t backend_live(int64_t *bytes) {
    int64_t n = 0;
    *bytes = 0;
    for (auto &kv : g_recs)
        if (!kv.second.frees) {
            ++n;
            *bytes += (int64_t)kv.second.bytes;
        }
    return n;
}
static void backend_reset(int fail_at) {
    for (auto &kv : g_recs) free(kv.first);
    g_recs.clear();
    g_calls = 0;
    g_fail_at = fail_at;
    g_bad_free = 0;
}
static void counters_match() {
    int64_t b = 0;
    const int64_t n = backend_live(&b);
    CHECK(g_mem_live_allocs.load() == n);
    CHECK(g_mem_live_bytes.load() == b);
}

// ---- the script -------------------------------------------------------------------------------------
// every buffer the pool hands out is filled with its tag; a buffer that is still held must keep it
struct held {
    uint8_t *p = nullptr;
    size_t bytes = 0;
    uint8_t tag = 0;
};
static void fill(held &h, size_t bytes, uint8_t tag) {
    h.bytes = bytes;
    h.tag = tag;
    if (h.p) memset(h.p, tag, bytes);
}
static void intact(const held &h) {
    if (!h.p) return;
    auto it = g_recs.find(h.p);
    CHECK(it != g_recs.end() && it->second.frees == 0 && it->second.bytes == h.bytes);
    for (size_t i = 0; i < h.bytes; ++i)
        if (h.p[i] != h.tag) {
            CHECK(!"held buffer changed");
            break;
        }
}

// one fallible step: rc and pointer agree, a failure is the injected one, and nothing held is lost
static void after(int rc, const held &h, int calls_before, std::initializer_list<const held *> others) {
    const bool injected = g_fail_at >= calls_before && g_fail_at < g_calls;
    CHECK((rc == -1) == injected);
    if (rc) {
        CHECK(h.p == nullptr);
        CHECK(!g_err.empty());
    } else {
        CHECK(h.p != nullptr);
    }
    for (const held *o : others) intact(*o);
    counters_match();
}

static int run_script(int fail_at) {
    backend_reset(fail_at);
    g_err.clear();
    {
        dev_pool pool(&g_be);
        held a, b, c, d, e;
        int c0 = g_calls;
        int rc = pool.get(&a.p, 100);
        fill(a, 100, 1);
        after(rc, a, c0, {});

        c0 = g_calls;
        rc = pool.get_zeroed(&b.p, 64, nullptr);
        if (b.p)
            for (int i = 0; i < 64; ++i) CHECK(b.p[i] == 0);
        fill(b, 64, 2);
        after(rc, b, c0, {&a});

        c0 = g_calls;  // a zero-size request: no backend call, no failure, no pointer
        rc = pool.get(&c.p, 0);
        CHECK(rc == 0 && c.p == nullptr && g_calls == c0);
        rc = pool.get_zeroed(&c.p, 0, nullptr);
        CHECK(rc == 0 && c.p == nullptr && g_calls == c0);

        c0 = g_calls;
        rc = pool.get(&d.p, 32, MEM_PINNED);
        fill(d, 32, 3);
        after(rc, d, c0, {&a, &b});

        uint8_t *was_b = b.p;  // put: freed once, pointer nulled, the rest untouched
        pool.put(b.p);
        CHECK(b.p == nullptr);
        if (was_b) CHECK(g_recs[was_b].frees == 1 && was_b[0] == 0xDD);
        intact(a);
        intact(d);
        counters_match();

        pool.put(a.p);  // regrow: drop, then ask for more
        CHECK(a.p == nullptr);
        c0 = g_calls;
        rc = pool.get(&a.p, 200);
        fill(a, 200, 4);
        after(rc, a, c0, {&d});

        c0 = g_calls;
        rc = pool.get_zeroed(&e.p, 16, nullptr, MEM_UNCACHED);
        fill(e, 16, 5);
        after(rc, e, c0, {&a, &d});

        pool.clear();  // everything back, counters at zero, the pool usable again
        CHECK(pool.count() == 0);
        CHECK(g_mem_live_allocs.load() == 0 && g_mem_live_bytes.load() == 0);
        a = held{};
        c0 = g_calls;
        rc = pool.get(&a.p, 48);
        fill(a, 48, 6);
        after(rc, a, c0, {});
        c0 = g_calls;
        rc = pool.get_zeroed(&b.p, 8, nullptr);
        fill(b, 8, 7);
        after(rc, b, c0, {&a});
    }  // the pool dies holding a and b
    CHECK(g_mem_live_allocs.load() == 0);
    CHECK(g_mem_live_bytes.load() == 0);
    CHECK(g_bad_free == 0);
    for (auto &kv : g_recs) CHECK(kv.second.frees == 1);  // every allocation freed exactly once
    return g_calls;
}

static void misuse() {
    backend_reset(-1);
    dev_pool pool(&g_be), other(&g_be);
    int *p = nullptr, *q = nullptr;
    g_err.clear();
    pool.put(p);  // nullptr: nothing happens
    CHECK(g_err.empty() && g_bad_free == 0);

    CHECK(pool.get(&p, 40) == 0 && other.get(&q, 40) == 0);
    int on_stack = 0, *foreign = &on_stack;
    pool.put(foreign);  // never allocated: error, pointer kept, the backend not called
    CHECK(!g_err.empty() && foreign == &on_stack && g_bad_free == 0);
    g_err.clear();
    int *q2 = q;
    pool.put(q2);  // another pool's: the same
    CHECK(!g_err.empty() && q2 == q && g_recs[q].frees == 0);

    int *stale = p;
    g_err.clear();
    pool.put(p);
    CHECK(p == nullptr && g_err.empty() && g_recs[stale].frees == 1);
    pool.put(p);  // the nulled pointer again: a no-op
    CHECK(g_err.empty());
    pool.put(stale);  // a stale copy: refused, not freed twice
    CHECK(!g_err.empty() && stale != nullptr && g_bad_free == 0 && g_recs[stale].frees == 1);

    // moving hands the allocations over: the source frees nothing
    dev_pool moved(std::move(other));
    CHECK(other.count() == 0 && moved.count() == 1);
    other.clear();
    CHECK(g_recs[q].frees == 0);
    moved.put(q);
    CHECK(q == nullptr && g_bad_free == 0);
    CHECK(g_mem_live_allocs.load() == 0 && g_mem_live_bytes.load() == 0);
}

int main() {
    const int calls = run_script(-1);  // no failure: how many backend calls the script makes
    for (int n = 0; n <= calls + 1; ++n) {
        const int before = g_fails;
        run_script(n);
        if (g_fails != before) printf("  (failing call %d of %d)\n", n, calls);
    }
    misuse();
    backend_reset(-1);
    if (g_fails) {
        printf("dev_mem_test: %d checks failed\n", g_fails);
        return 1;
    }
    printf("dev_mem_test: ok (%d backend calls, each failed in turn)\n", calls);
    return 0;
}
