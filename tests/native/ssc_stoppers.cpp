// The compact stopper array of k_ssc (gtsam-vslam_amd/csrc/ssc_stoppers.hpp), proven on the host: for every segment the capped
// one-array form of the parallel Hoare partition gives the cut, the number of exchanges and the permuted array of libstdc++'s
// sequential loop (std::__move_median_to_first + std::__unguarded_partition, restated below), no slot of the segment's slice is
// written twice, none is read unwritten, and no access leaves the slice.  The stopper array is a heap buffer of exactly one u16
// per element, so AddressSanitizer sees any slot outside it.  Every array is partitioned down to 16-element blocks the way
// introsort does, so segments of every length and offset down to 17 elements are covered, those past SSC_COOP_MIN included.
#include "ssc_stoppers.hpp"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static long long g_segments = 0, g_boundary = 0, g_capped = 0;

// key in the upper half, original index in the lower half, as in k_ssc
static inline uint32_t keyOf(uint32_t v) { return v >> 16; }

static void median_to_first(uint32_t* a, int f, int e) {
    const int ia = f + 1, ib = f + (e - f) / 2, ic = e - 1;
    const uint32_t ka = keyOf(a[ia]), kb = keyOf(a[ib]), kc = keyOf(a[ic]);
    int m;
    if (ka < kb) { if (kb < kc) m = ib; else if (ka < kc) m = ic; else m = ia; }
    else if (ka < kc) m = ia; else if (kb < kc) m = ic; else m = ib;
    const uint32_t t = a[f]; a[f] = a[m]; a[m] = t;
}

// std::__unguarded_partition(f + 1, e, f); returns the cut, *swaps = number of iter_swaps
static int sequential_partition(uint32_t* a, int f, int e, int* swaps) {
    int first = f + 1, last = e;
    const uint32_t pivot = keyOf(a[f]);
    *swaps = 0;
    for (;;) {
        while (keyOf(a[first]) < pivot) ++first;
        --last;
        while (pivot < keyOf(a[last])) --last;
        if (!(first < last)) return first;
        const uint32_t t = a[first]; a[first] = a[last]; a[last] = t;
        ++*swaps;
        ++first;
    }
}

// the slice of the stopper array with its bookkeeping: 0 = never written, 1 = written
struct Slice {
    uint16_t* s; uint8_t* state; int f, e; bool ok;
    void put(int slot, int x) {
        if (slot < f || slot >= e || state[slot]) { ok = false; return; }
        s[slot] = (uint16_t)x; state[slot] = 1;
    }
    int get(int slot) {
        if (slot < f || slot >= e || !state[slot]) { ok = false; return f; }
        return s[slot];
    }
};

// the capped parallel form, exactly as the kernels index it; returns the cut, *swaps = K
static int capped_partition(uint32_t* a, int f, int e, uint16_t* stop, uint8_t* state, int* swaps, bool* ok) {
    Slice S{stop, state, f, e, true};
    memset(state + f, 0, (size_t)(e - f));
    const uint32_t pk = keyOf(a[f]);
    const int cap = ssc_stop_cap(f, e);
    int nL = 0, nR = 0;
    for (int x = f + 1; x < e; x++)                      // left stoppers, ascending position
        if (keyOf(a[x]) >= pk) { if (nL < cap) S.put(ssc_stop_left(f, nL), x); nL++; }
    for (int x = e - 1; x > f; x--)                      // right stoppers, descending position
        if (keyOf(a[x]) <= pk) { if (nR < cap) S.put(ssc_stop_right(e, nR), x); nR++; }
    const int nPair = ssc_stop_pairs(nL, nR, cap);
    int K = 0;
    while (K < nPair && S.get(ssc_stop_left(f, K)) < S.get(ssc_stop_right(e, K))) K++;
    for (int k = 0; k < K; k++) {
        const int xl = S.get(ssc_stop_left(f, k)), xr = S.get(ssc_stop_right(e, k));
        const uint32_t t = a[xl]; a[xl] = a[xr]; a[xr] = t;
    }
    int cut = K >= 1 ? S.get(ssc_stop_right(e, K - 1)) : e;
    if (ssc_stop_has_left(K, nL, cap)) { const int l = S.get(ssc_stop_left(f, K)); if (l < cut) cut = l; }
    const int m = e - f - 1;
    if (nL > cap || nR > cap) g_capped++;
    if ((m & 1) == 0 && K == m / 2) g_boundary++;
    *swaps = K;
    *ok = S.ok;
    return cut;
}

#define CHECK(c, ...)                                                                     \
    do {                                                                                  \
        if (!(c)) { printf("FAILED %s (line %d): ", #c, __LINE__); printf(__VA_ARGS__); printf("\n"); return false; } \
    } while (0)

// introsort's partition tree of a[0, n) down to 16-element blocks, both forms side by side on their own copies
static bool run_array(const std::vector<uint32_t>& in, const char* what) {
    const int n = (int)in.size();
    uint32_t* a = (uint32_t*)malloc(sizeof(uint32_t) * n);      // sequential
    uint32_t* b = (uint32_t*)malloc(sizeof(uint32_t) * n);      // capped
    uint16_t* stop = (uint16_t*)malloc(sizeof(uint16_t) * n);
    uint8_t* state = (uint8_t*)malloc(n);
    memcpy(a, in.data(), sizeof(uint32_t) * n); memcpy(b, in.data(), sizeof(uint32_t) * n);
    std::vector<int> stack;
    if (n > 16) { stack.push_back(0); stack.push_back(n); }
    bool good = true;
    while (good && !stack.empty()) {
        const int e = stack.back(); stack.pop_back();
        const int f = stack.back(); stack.pop_back();
        median_to_first(a, f, e); median_to_first(b, f, e);
        int ks = 0, kc = 0;
        bool ok = true;
        const int cs = sequential_partition(a, f, e, &ks);
        const int cc = capped_partition(b, f, e, stop, state, &kc, &ok);
        g_segments++;
        good = [&] {
            CHECK(ok, "%s n %d segment [%d, %d): a slot written twice, read unwritten or outside the slice", what, n, f, e);
            CHECK(cs == cc, "%s n %d segment [%d, %d): cut %d, sequential %d", what, n, f, e, cc, cs);
            CHECK(ks == kc, "%s n %d segment [%d, %d): %d exchanges, sequential %d", what, n, f, e, kc, ks);
            CHECK(memcmp(a + f, b + f, sizeof(uint32_t) * (e - f)) == 0, "%s n %d segment [%d, %d): arrays differ", what, n, f, e);
            CHECK(cs > f && cs <= e, "%s n %d segment [%d, %d): cut %d", what, n, f, e, cs);
            return true;
        }();
        if (e - cs > 16) { stack.push_back(cs); stack.push_back(e); }
        if (cs - f > 16) { stack.push_back(f); stack.push_back(cs); }
    }
    free(a); free(b); free(stop); free(state);
    return good;
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }

static std::vector<uint32_t> pack(const std::vector<uint32_t>& keys) {
    std::vector<uint32_t> v(keys.size());
    for (size_t i = 0; i < keys.size(); i++) v[i] = (keys[i] << 16) | (uint32_t)i;
    return v;
}

int main() {
    // every 0 / 1 array of 17 .. 20 elements
    for (int n = 17; n <= 20; n++)
        for (uint32_t bits = 0; bits < (1u << n); bits++) {
            std::vector<uint32_t> k(n);
            for (int i = 0; i < n; i++) k[i] = (bits >> i) & 1u;
            if (!run_array(pack(k), "binary")) return 1;
        }
    // seeded random arrays up to 2 100 elements (past SSC_COOP_MIN = 2 048) over alphabets of 1, 2, 3, 17 and 256 values; as they
    // are, sorted and reversed
    const int alphabets[5] = {1, 2, 3, 17, 256};
    const int sizes[] = {17, 18, 31, 32, 33, 63, 64, 65, 66, 100, 127, 128, 129, 255, 256, 257, 1000, 2047, 2048, 2049, 2050, 2100};
    for (int al = 0; al < 5; al++)
        for (int rep = 0; rep < 40; rep++)
            for (int n : sizes) {
                std::vector<uint32_t> k(n);
                for (int i = 0; i < n; i++) k[i] = rnd() % alphabets[al];
                if (!run_array(pack(k), "random")) return 1;
                if (rep >= 4) continue;
                std::vector<uint32_t> s(k);
                for (int i = 1; i < n; i++) { uint32_t v = s[i]; int j = i; while (j > 0 && s[j - 1] > v) { s[j] = s[j - 1]; j--; } s[j] = v; }
                if (!run_array(pack(s), "sorted")) return 1;
                std::vector<uint32_t> r(s.rbegin(), s.rend());
                if (!run_array(pack(r), "reversed")) return 1;
                std::vector<uint32_t> o(n);                      // organ pipe: up, then down
                for (int i = 0; i < n; i++) o[i] = s[i < n / 2 ? 2 * i : 2 * (n - 1 - i) + 1 < n ? 2 * (n - 1 - i) + 1 : n - 1];
                if (!run_array(pack(o), "organ_pipe")) return 1;
            }
    if (g_boundary == 0 || g_capped == 0) { printf("FAILED: the boundary case (%lld) or a capped list (%lld) never occurred\n", g_boundary, g_capped); return 1; }
    printf("ok: %lld segments, %lld with a list longer than the cap, %lld at K = m / 2 with m even\n", g_segments, g_capped, g_boundary);
    return 0;
}
