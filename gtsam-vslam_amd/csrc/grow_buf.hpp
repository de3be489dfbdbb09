// Grow-only buffer of the local-BA workspaces (pure C++: also compiled on its own under AddressSanitizer + UBSan by
// tests/test_grow_buf.py).  A buffer keeps its block across calls and replaces it by a larger one when a request does not fit; how much
// larger is the caller's rule.  The failure path is the point: pointer and capacity change only after the new allocation has succeeded,
// so a failed growth leaves an EMPTY buffer (p == nullptr, n == 0) and an error - never a freed address with a capacity beside it - and
// the next request simply allocates afresh.
#pragma once
#include <algorithm>
#include <cstddef>

namespace vslam {

// Alloc: static E alloc(void** p, size_t bytes) (E{} = success, *p untouched or null on failure) and static void free(void* p).
template <typename T, typename Alloc>
struct GrowBuf {
    using Err = decltype(Alloc::alloc((void**)nullptr, (size_t)0));
    T* p = nullptr;
    size_t n = 0;        // capacity in elements of T
    // Room for `count` elements.  A request that fits allocates nothing; one that does not gets rule(count) elements.  `before` runs
    // ahead of the free (the site's stream synchronisation: the old block may still be in use); its error leaves the buffer as it was.
    template <class Rule, class Before>
    Err ensure(size_t count, Rule rule, Before before) {
        if (count <= n) return Err{};
        const Err b = before();
        if (b != Err{}) return b;
        release();       // (old block first: the peak is one block, not two)
        const size_t cap = rule(count);
        void* q = nullptr;
        const Err e = Alloc::alloc(&q, cap * sizeof(T));
        if (e != Err{}) return e;
        p = (T*)q; n = cap;
        return Err{};
    }
    template <class Rule>
    Err ensure(size_t count, Rule rule) { return ensure(count, rule, [] { return Err{}; }); }
    void release() {
        if (p) Alloc::free(p);
        p = nullptr; n = 0;
    }
    // (no destructor: the owners release explicitly - no HIP call from a thread_local destructor)
};

// ---- the growth rules of the local-BA buffers (capacity in elements for a request of c elements) ---------------------------------
struct GrowDouble { size_t add, floor; size_t operator()(size_t c) const { return std::max(2 * c + add, floor); } };      // 2 c + add, at least floor
struct GrowHalf { size_t add; size_t operator()(size_t c) const { return c + c / 2 + add; } };                            // c + c / 2 + add
struct GrowPlus { size_t add; size_t operator()(size_t c) const { return c + add; } };                                    // c + add
// device buffers: headroom of a factor two, floor of 64 KB in BYTES (a mapping thread's windows differ a little from call to call, and
// every new maximum costs a device-synchronising free + an allocation)
template <typename T> inline GrowDouble grow_dev() { return {0, ((size_t)64 << 10) / sizeof(T)}; }
inline GrowDouble grow_wrong() { return {4096, 0}; }                  // pinned chi2 flags
inline GrowHalf grow_out() { return {4096}; }                         // pinned landing area of the result
inline GrowDouble grow_block() { return {(size_t)64 << 10, 0}; }      // pinned constant block; the upload arena (host and device half)
inline GrowPlus grow_ord_scal() { return {1024}; }                    // pinned scalars of the device ordering
inline GrowDouble grow_back() { return {4096, 0}; }                   // pinned landing area of the batch

}  // namespace vslam
