// AddressSanitizer / UBSan check of the lockstep group's key-slab free list (gtsam-vslam_amd/csrc/slab_pool.hpp) with malloc / free as
// the allocator: sessions of several "lanes" take slabs on their own threads, write every byte of what they got, hand them back when the
// lane restarts; the pool must never hand one slab to two owners, must reuse what came back before it allocates, must free everything it
// allocated exactly once, and its accounting must add up at every restart.
#include "slab_pool.hpp"
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

static std::atomic<long long> g_allocs{0}, g_frees{0};

static int fail(const char* what) { printf("FAILED: %s\n", what); return 1; }

int main() {
    vslam::SlabPool P;
    P.unit = 1 << 16;
    P.alloc = [](size_t n) -> void* { g_allocs++; return malloc(n); };
    P.dealloc = [](void* p) { g_frees++; free(p); };

    // ---- one owner: reuse before allocation, sizes, refusals -------------------------------------------------------------------
    void* a = P.take(1000);              // (smaller than the unit: a unit-sized slab)
    void* b = P.take((1 << 16) + 1);     // (larger than the unit: its own size)
    if (!a || !b || a == b) return fail("take");
    memset(a, 1, 1 << 16); memset(b, 2, (1 << 16) + 1);
    int64_t bytes = 0; int32_t u = 0, f = 0;
    P.stats(&bytes, &u, &f);
    if (bytes != (1 << 16) + (1 << 16) + 1 || u != 2 || f != 0) return fail("stats after two takes");
    if (!P.give(a) || P.give(a)) return fail("give twice must be refused");
    int dummy = 0;
    if (P.give(&dummy)) return fail("give of a foreign pointer must be refused");
    P.stats(&bytes, &u, &f);
    if (u != 1 || f != 1) return fail("stats after give");
    if (P.take(1 << 16) != a) return fail("a free slab that fits is reused");
    if (!P.give(a) || !P.give(b)) return fail("give");
    if (P.take(100) != a) return fail("the smallest free slab that fits is taken");      // (not the larger b)
    void* c = P.take((1 << 16) + 1);
    if (c != b) return fail("a large request takes the large free slab");
    if (g_allocs != 2) return fail("nothing was allocated for the reuses");
    P.give(a); P.give(c);
    if (P.destroy() != 0 || g_frees != 2) return fail("destroy frees the free list");
    P.stats(&bytes, &u, &f);
    if (bytes != 0 || u != 0 || f != 0) return fail("stats after destroy");

    // ---- lanes restarting on their own threads ------------------------------------------------------------------------------------
    constexpr int LANES = 6, GENERATIONS = 200, MAXSLABS = 3;
    g_allocs = 0; g_frees = 0;
    std::atomic<int> bad{0};
    std::vector<std::thread> th;
    for (int l = 0; l < LANES; l++)
        th.emplace_back([&, l]() {
            for (int g = 0; g < GENERATIONS; g++) {
                const int n = 1 + (g + l) % MAXSLABS;
                const size_t sz = (size_t)(1 << 16) - 64 * ((g * 7 + l) % 5);      // (slot sizes differ between sessions: all fit a unit)
                unsigned char* s[MAXSLABS];
                for (int i = 0; i < n; i++) {
                    s[i] = (unsigned char*)P.take(sz);
                    if (!s[i]) { bad++; return; }
                    memset(s[i], l * 16 + i, sz);
                }
                std::this_thread::yield();
                for (int i = 0; i < n; i++) {
                    for (size_t k = 0; k < sz; k += 997) if (s[i][k] != (unsigned char)(l * 16 + i)) { bad++; break; }      // (nobody else wrote it)
                    if (!P.give(s[i])) bad++;
                }
            }
        });
    for (auto& t : th) t.join();
    if (bad) return fail("a slab was shared, lost or refused");
    P.stats(&bytes, &u, &f);
    if (u != 0 || f != g_allocs || bytes != (int64_t)g_allocs * (1 << 16)) return fail("accounting after the generations");
    if (g_allocs > LANES * MAXSLABS) return fail("bounded: never more slabs than the lanes hold at once");
    // a slab still in use survives destroy(); its owner hands it back, the next destroy() frees it
    void* keep = P.take(10);
    if (P.destroy() != 1) return fail("destroy keeps slabs in use");
    memset(keep, 3, 1 << 16);
    if (!P.give(keep) || P.destroy() != 0) return fail("second destroy");
    if (g_frees != g_allocs) return fail("every slab freed exactly once");
    printf("ok: %lld slabs served %d sessions\n", g_allocs.load(), LANES * GENERATIONS);
    return 0;
}
