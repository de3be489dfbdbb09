// Free list of the lockstep group's keyframe key slabs (pure C++: no HIP here - the allocator is handed in, so the accounting is
// compiled and tested on its own, tests/test_slab_pool.py).  A session carves fixed-size key slots from slabs (system.hip
// reserve_key_slot); a lane of a vslam_batch takes its slabs from this pool and hands them back when the lane restarts
// (vslam_batch_restart_lane) or the batch ends.  A slab that comes back is kept: the next session of any lane takes it before the
// allocator is asked again, so a lane that restarts for ever allocates nothing new and nothing is freed while other lanes' kernels
// run (a device free waits for the whole device).  destroy() frees what the list holds.
// Slot size is a session's own choice (from its first frame); a slab is just bytes: every slab is allocated with at least `unit`
// bytes, so that the slabs of sessions with different slot sizes are interchangeable.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <mutex>
#include <vector>

namespace vslam {

struct SlabPool {
    struct Slab { void* p; size_t bytes; bool used; };
    std::function<void*(size_t)> alloc;      // returns null when out of memory
    std::function<void(void*)> dealloc;
    size_t unit = (size_t)16 << 20;
    std::mutex mu;                           // (the lanes' host phases reserve key slots on the pool threads)
    std::vector<Slab> slabs;                 // every slab the pool has allocated and not yet freed

    // a slab of at least `bytes`: the smallest free one that is large enough, else a new one
    void* take(size_t bytes) {
        std::lock_guard<std::mutex> lk(mu);
        Slab* best = nullptr;
        for (Slab& s : slabs) if (!s.used && s.bytes >= bytes && (!best || s.bytes < best->bytes)) best = &s;
        if (best) { best->used = true; return best->p; }
        const size_t want = std::max(bytes, unit);
        void* p = alloc ? alloc(want) : nullptr;
        if (!p) return nullptr;
        slabs.push_back({p, want, true});
        return p;
    }
    // hands a slab back (false: not one of this pool's slabs in use - nothing is changed)
    bool give(void* p) {
        std::lock_guard<std::mutex> lk(mu);
        for (Slab& s : slabs) if (s.p == p && s.used) { s.used = false; return true; }
        return false;
    }
    void stats(int64_t* bytes, int32_t* inUse, int32_t* nFree) {
        std::lock_guard<std::mutex> lk(mu);
        int64_t b = 0; int32_t u = 0, f = 0;
        for (const Slab& s : slabs) { b += (int64_t)s.bytes; (s.used ? u : f)++; }
        if (bytes) *bytes = b;
        if (inUse) *inUse = u;
        if (nFree) *nFree = f;
    }
    // frees the free list; slabs still in use stay (their owners hand them back first).  Returns the number left in use.
    int destroy() {
        std::lock_guard<std::mutex> lk(mu);
        std::vector<Slab> keep;
        for (Slab& s : slabs) { if (s.used) keep.push_back(s); else if (dealloc) dealloc(s.p); }
        slabs.swap(keep);
        return (int)slabs.size();
    }
};

}  // namespace vslam
