// arena_check.cpp -- the bookkeeping of mgpt::Arena (mapf_gpt_amd/csrc/device_mem.h) on malloc / free, for a sanitizer build on the CPU:
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/arena_check.cpp -o arena_check && ./arena_check
// Ends with exit status 0, the counters at 0 / 0 and nothing for LeakSanitizer to report (tests/test_abi_cpu.py builds and runs it).
#define MGPT_DEVICE_MEM_NO_HIP
#include "../../mapf_gpt_amd/csrc/device_mem.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace {

int g_failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failures++; } \
    } while (0)

// malloc / free with a budget: allocation number fail_at (counted from 1 since the last arm()) fails; host and device memory counted apart
struct TestMem {
    using Error = int;
    static constexpr Error ok = 0;
    static inline int calls = 0, fail_at = 0, live = 0, live_host = 0;
    static void arm(int n) { calls = 0; fail_at = n; }
    static Error get(void **p, size_t bytes, int *counter)
    {
        if (++calls == fail_at) return 2;                  // (leaves *p alone, as a failed runtime call would)
        *p = malloc(bytes);
        memset(*p, 0xA5, bytes);
        ++*counter;
        return ok;
    }
    static Error alloc(void **p, size_t bytes) { return get(p, bytes, &live); }
    static Error alloc_host(void **p, size_t bytes) { return get(p, bytes, &live_host); }
    static void free(void *p) { ::free(p); live--; }
    static void free_host(void *p) { ::free(p); live_host--; }
};
using A = mgpt::Arena<TestMem>;

int64_t live_allocs() { return mgpt::MemCounters::allocs.load(); }
int64_t live_bytes() { return mgpt::MemCounters::bytes.load(); }
bool all_free() { return live_allocs() == 0 && live_bytes() == 0 && TestMem::live == 0 && TestMem::live_host == 0; }

struct Ctx {                                               // a context in the library's style: raw pointers and their owner
    float *a = nullptr;
    int *b = nullptr;
    char *pinned = nullptr;
    double *c = nullptr;
    short *d = nullptr;
    A mem;
};

// the five-allocation sequence of a create function: builds into a local arena, commits only when everything has succeeded
int build(Ctx *c)
{
    A mem;
    Ctx n;
    int e = mem.alloc(&n.a, 100 * sizeof(float));
    if (e == TestMem::ok) e = mem.alloc(&n.b, 7 * sizeof(int));
    if (e == TestMem::ok) e = mem.alloc_host(&n.pinned, 33);
    if (e == TestMem::ok) e = mem.alloc(&n.c, 5 * sizeof(double));
    if (e == TestMem::ok) e = mem.alloc(&n.d, sizeof(short));
    if (e != TestMem::ok) return e;
    c->a = n.a; c->b = n.b; c->pinned = n.pinned; c->c = n.c; c->d = n.d;
    c->mem.adopt(std::move(mem));
    return TestMem::ok;
}

}  // namespace

int main()
{
    TestMem::arm(0);
    {   // alloc and release; release-then-reuse; the destructor releases
        A a;
        float *x = nullptr;
        char *h = nullptr;
        CHECK(a.alloc(&x, 64) == TestMem::ok && x != nullptr);
        CHECK(a.alloc_host(&h, 16) == TestMem::ok && h != nullptr);
        x[15] = 1.f; h[15] = 1;                                     // (the memory is ours: the sanitizer watches the bounds)
        CHECK(live_allocs() == 2 && live_bytes() == 80 && a.count() == 2 && TestMem::live == 1 && TestMem::live_host == 1);
        a.release();
        CHECK(a.empty() && all_free());
        a.release();                                                // (a second release is a no-op)
        CHECK(all_free());
        CHECK(a.alloc(&x, 32) == TestMem::ok);
        CHECK(live_allocs() == 1 && live_bytes() == 32);
    }
    CHECK(all_free());
    {   // move construction and move assignment: one owner at any time, the target's old memory is freed
        A a, c;
        int *p = nullptr, *q = nullptr;
        CHECK(a.alloc(&p, 40) == TestMem::ok);
        A b(std::move(a));
        CHECK(a.empty() && b.count() == 1 && live_allocs() == 1);
        CHECK(c.alloc(&q, 8) == TestMem::ok && live_bytes() == 48);
        c = std::move(b);
        CHECK(b.empty() && c.count() == 1 && live_allocs() == 1 && live_bytes() == 40);
        p[9] = 3;                                                   // still alive, owned by c
        A &self = c;
        c = std::move(self);                                        // (self-assignment keeps it)
        CHECK(c.count() == 1 && live_allocs() == 1);
    }
    CHECK(all_free());
    {   // adopt on success: the context's arena takes the local one's memory behind its own
        Ctx ctx;
        short *first = nullptr;
        CHECK(ctx.mem.alloc(&first, 2) == TestMem::ok);
        CHECK(build(&ctx) == TestMem::ok);
        CHECK(ctx.mem.count() == 6 && live_allocs() == 6 && ctx.a && ctx.b && ctx.pinned && ctx.c && ctx.d);
        ctx.a[99] = 1.f; ctx.pinned[32] = 1; ctx.d[0] = 0;
        CHECK(TestMem::live == 5 && TestMem::live_host == 1);
    }
    CHECK(all_free());
    // a failure at every allocation of the sequence: nothing is left behind, the context is untouched and usable
    for (int n = 1; n <= 5; n++) {
        Ctx ctx;
        TestMem::arm(n);
        CHECK(build(&ctx) != TestMem::ok);
        CHECK(ctx.mem.empty() && ctx.a == nullptr && ctx.d == nullptr && all_free());
        TestMem::arm(0);
        CHECK(build(&ctx) == TestMem::ok && live_allocs() == 5);    // the retry succeeds
        ctx.mem.release();
        CHECK(all_free());
    }
    {   // a failed allocation nulls the pointer it was given and records nothing
        A a;
        int *p = reinterpret_cast<int *>(0x10);
        TestMem::arm(1);
        CHECK(a.alloc(&p, 4) != TestMem::ok && p == nullptr && a.empty());
        TestMem::arm(0);
    }
    CHECK(all_free());
    {   // alloc_all: every request served, in order, and owned by the arena; nothing is live after release()
        A a;
        float *x = nullptr;
        int *y = nullptr;
        char *z = nullptr;
        CHECK(a.alloc_all({{&x, 64}, {&y, 12}, {&z, 3}}) == TestMem::ok && x && y && z);
        x[15] = 1.f; y[2] = 1; z[2] = 1;
        CHECK(a.count() == 3 && live_allocs() == 3 && live_bytes() == 79 && TestMem::live == 3 && TestMem::live_host == 0);
        a.release();
        CHECK(a.empty() && all_free());
    }
    // alloc_all with a failure at request k, for every k: the first error comes back, the pointers from k on are nullptr, the earlier
    // allocations are the arena's and go with it
    for (int k = 1; k <= 3; k++) {
        A a;
        void *const stale = reinterpret_cast<void *>(0x10);
        float *x = static_cast<float *>(stale);
        int *y = static_cast<int *>(stale);
        char *z = static_cast<char *>(stale);
        TestMem::arm(k);
        CHECK(a.alloc_all({{&x, 64}, {&y, 12}, {&z, 3}}) == 2);
        CHECK(TestMem::calls == k);                                 // it stopped at the failure
        TestMem::arm(0);
        CHECK((x != nullptr) == (k > 1) && (y != nullptr) == (k > 2) && z == nullptr);
        CHECK(x != stale && y != stale);
        CHECK(a.count() == (size_t)(k - 1) && live_allocs() == k - 1 && TestMem::live == k - 1);
        CHECK(live_bytes() == (k == 1 ? 0 : k == 2 ? 64 : 76));
        if (k > 1) x[15] = 1.f;
        if (k > 2) y[2] = 1;
        a.release();
        CHECK(a.empty() && all_free());
    }
    {   // a zero-byte request is no failure and stops nothing: the requests around it are served, the counters return to 0 / 0
        A a;
        float *x = nullptr;
        int *none = reinterpret_cast<int *>(0x10);
        char *z = nullptr;
        CHECK(a.alloc_all({{&x, 8}, {&none, 0}, {&z, 5}}) == TestMem::ok && x && z);
        CHECK(live_bytes() == 13 && a.count() == (none ? 3u : 2u));
        CHECK(a.alloc_all({}) == TestMem::ok);                      // (an empty list too)
        a.release();
        CHECK(a.empty() && all_free());
    }
    CHECK(all_free());
    if (g_failures == 0) printf("arena_check: ok (%lld allocations, %lld bytes live)\n", (long long)live_allocs(), (long long)live_bytes());
    return g_failures == 0 ? 0 : 1;
}
