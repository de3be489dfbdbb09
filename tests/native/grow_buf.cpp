// GrowBuf (gtsam-vslam_amd/csrc/grow_buf.hpp) with a counting allocator that can be told to fail: the six growth rules of the local-BA
// buffers, the failure path, release.  Stand-alone, built with -fsanitize=address,undefined by tests/test_grow_buf.py: a block
// freed twice or used after its free ends the program.
#include "grow_buf.hpp"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>

using namespace vslam;

static int g_allocs = 0, g_frees = 0, g_failAt = 0;      // g_failAt: the k-th call of alloc from now fails (0: none)
static size_t g_lastBytes = 0;
static std::set<void*> g_live;
static int g_bad = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); g_bad++; } } while (0)

struct FakeAlloc {
    static int alloc(void** p, size_t bytes) {
        if (g_failAt > 0 && --g_failAt == 0) return 2;      // (like hipErrorOutOfMemory: *p untouched)
        g_allocs++; g_lastBytes = bytes;
        *p = malloc(bytes ? bytes : 1);
        g_live.insert(*p);
        return 0;
    }
    static void free(void* p) {
        CHECK(g_live.count(p) == 1);      // nothing is freed twice, nothing that was never allocated
        g_live.erase(p);
        g_frees++;
        ::free(p);
    }
};

// one rule at requests of 0, 1, exactly the capacity and capacity + 1, on a fresh buffer and on a grown one
template <typename T, class Rule>
static void check_rule(const char* name, Rule rule, size_t first) {
    GrowBuf<T, FakeAlloc> b;
    int a0 = g_allocs, f0 = g_frees;
    CHECK(b.ensure(0, rule) == 0);
    CHECK(b.p == nullptr && b.n == 0 && g_allocs == a0);               // an empty request fits an empty buffer
    CHECK(b.ensure(1, rule) == 0);
    CHECK(b.p != nullptr && b.n == rule(1) && b.n >= 1 && g_allocs == a0 + 1 && g_lastBytes == rule(1) * sizeof(T));
    b.release();
    CHECK(g_frees == f0 + 1);
    a0 = g_allocs; f0 = g_frees;
    CHECK(b.ensure(first, rule) == 0);
    const size_t cap = b.n;
    T* const p = b.p;
    CHECK(cap == rule(first) && cap >= first && g_allocs == a0 + 1 && g_frees == f0 && g_lastBytes == cap * sizeof(T));
    for (size_t i = 0; i < cap; i++) b.p[i] = (T)i;                    // (the whole capacity is the buffer's: the sanitizer watches)
    for (size_t req : {(size_t)0, (size_t)1, first, cap}) {
        CHECK(b.ensure(req, rule) == 0);
        CHECK(b.p == p && b.n == cap && g_allocs == a0 + 1 && g_frees == f0);      // fits: no allocation, no free, same block
    }
    int before = 0;
    CHECK(b.ensure(cap + 1, rule, [&] { before++; CHECK(g_frees == f0); return 0; }) == 0);      // `before` runs ahead of the free
    CHECK(before == 1 && b.n == rule(cap + 1) && b.n >= cap + 1 && g_allocs == a0 + 2 && g_frees == f0 + 1 && g_lastBytes == b.n * sizeof(T));
    for (size_t i = 0; i < b.n; i++) b.p[i] = (T)i;
    // an error of `before` leaves the buffer as it was
    const size_t cap2 = b.n;
    T* const p2 = b.p;
    CHECK(b.ensure(cap2 + 1, rule, [] { return 7; }) == 7);
    CHECK(b.p == p2 && b.n == cap2 && g_allocs == a0 + 2 && g_frees == f0 + 1);
    b.release();
    CHECK(b.p == nullptr && b.n == 0 && g_frees == f0 + 2);
    b.release();                                                        // idempotent
    CHECK(g_frees == f0 + 2);
    printf("  %-14s %zu -> %zu, %zu -> %zu\n", name, first, cap, cap + 1, cap2);
}

// an allocator that fails on its k-th call: an empty buffer and the error, nothing freed twice, the next request allocates afresh
template <class Rule>
static void check_failure(Rule rule) {
    for (int k = 1; k <= 3; k++) {
        GrowBuf<uint8_t, FakeAlloc> b;
        const int a0 = g_allocs, f0 = g_frees;
        g_failAt = k;
        size_t req = 100;
        int grown = 0;
        for (int call = 1; call <= k; call++) {
            const int e = b.ensure(req, rule);
            if (call < k) { CHECK(e == 0 && b.p && b.n == rule(req)); grown++; req = b.n + 1; }
            else {
                CHECK(e == 2);
                CHECK(b.p == nullptr && b.n == 0);                     // empty: no freed address with a capacity beside it
                CHECK(g_allocs == a0 + grown && g_frees == f0 + grown);      // the old block went before the allocation was tried, once
            }
        }
        CHECK(g_failAt == 0);
        CHECK(b.ensure(0, rule) == 0 && b.p == nullptr);               // (nothing to do for an empty request)
        CHECK(b.ensure(req, rule) == 0);                                // the following request allocates afresh and succeeds
        CHECK(b.p != nullptr && b.n == rule(req) && g_allocs == a0 + grown + 1 && g_frees == f0 + grown);
        b.p[b.n - 1] = 1;
        b.release();
        b.release();
        CHECK(g_frees == f0 + grown + 1);
    }
}

int main() {
    check_rule<double>("dev double", grow_dev<double>(), 5000);         // below the 64 KB floor: 8192 doubles
    check_rule<double>("dev double", grow_dev<double>(), 100000);       // above it: twice the request
    check_rule<uint8_t>("dev bytes", grow_dev<uint8_t>(), 16);
    check_rule<uint8_t>("wrong", grow_wrong(), 3000);
    check_rule<uint8_t>("out", grow_out(), 3001);
    check_rule<uint8_t>("const / arena", grow_block(), 70000);
    check_rule<uint8_t>("ord scalars", grow_ord_scal(), 64 + 4 * 11);
    check_rule<uint8_t>("back", grow_back(), 12345);
    // the rules as the workspaces have always had them
    CHECK(grow_dev<double>()(5000) == 10000 && grow_dev<double>()(10) == 8192 && grow_dev<int>()(0) == 16384 && grow_dev<uint8_t>()(40000) == 80000);
    CHECK(grow_wrong()(1000) == 2 * 1000 + 4096);
    CHECK(grow_out()(1001) == 1001 + 500 + 4096);
    CHECK(grow_block()(1000) == 2 * 1000 + 65536);
    CHECK(grow_ord_scal()(108) == 108 + 1024);
    CHECK(grow_back()(1000) == 2 * 1000 + 4096);
    check_failure(grow_wrong());
    check_failure(grow_dev<uint8_t>());
    check_failure(grow_ord_scal());
    CHECK(g_allocs == g_frees && g_live.empty());                       // allocations equal frees at exit
    if (g_bad) { printf("FAILED: %d checks\n", g_bad); return 1; }
    printf("ok: %d allocations, %d frees\n", g_allocs, g_frees);
    return 0;
}
