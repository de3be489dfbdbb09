// The packed upper-block form of the reduced camera system (gtsam-vslam_amd/csrc/ba_packed.hpp), checked on the host for F = 1..10:
// the offsets of all (a <= b, i, j) and of the right-hand side are distinct and inside ba_packed_doubles(F); the row-major -> packed
// map and its inverse agree with them in both directions; entries below the block diagonal are absent; the slots of k_ba_reduce
// (packed offsets, then the absent entries) cover every row-major entry exactly once.
// The map is exercised through a heap buffer of exactly the stated size, so AddressSanitizer sees any offset outside it.
#include "ba_packed.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(c)                                                                      \
    do {                                                                              \
        if (!(c)) { printf("FAILED %s (line %d, F = %d)\n", #c, __LINE__, F); return 1; } \
    } while (0)

int main() {
    for (int F = 1; F <= 10; F++) {
        const int n = 6 * F, size = ba_packed_doubles(F), total = n * n + n;
        CHECK(ba_packed_blocks(F) == F * (F + 1) / 2);
        CHECK(size == ba_packed_blocks(F) * BA_PACKED_PITCH + n && BA_PACKED_PITCH >= 36);
        CHECK(size <= total || F == 1);      // (one block: 37 + 6 against 36 + 6)
        int* owner = (int*)malloc(sizeof(int) * size);      // row-major entry stored at each packed offset, -1: none
        for (int k = 0; k < size; k++) owner[k] = -1;
        int stored = 0, ordinal = 0;
        for (int a = 0; a < F; a++)
            for (int b = a; b < F; b++) {
                CHECK(ba_packed_block(F, a, b) == ordinal);      // rows of the block triangle, one after the other
                ordinal++;
                for (int i = 0; i < 6; i++)
                    for (int j = 0; j < 6; j++) {
                        const int off = ba_packed_off(F, a, b, i, j), e = (6 * a + i) * n + 6 * b + j;
                        CHECK(off >= 0 && off < ba_packed_rhs(F));
                        CHECK(owner[off] == -1);                 // injective
                        owner[off] = e;
                        stored++;
                        CHECK(ba_packed_from_rowmajor(F, e) == off);
                        CHECK(ba_packed_to_rowmajor(F, off) == e);
                        // a lane's base address + constant offsets: the entry is 6 i + j behind the block's first
                        CHECK(off == ba_packed_off(F, a, b, 0, 0) + 6 * i + j);
                    }
            }
        for (int k = 0; k < n; k++) {
            const int off = ba_packed_rhs(F) + k;
            CHECK(off < size && owner[off] == -1);
            owner[off] = n * n + k;
            stored++;
            CHECK(ba_packed_from_rowmajor(F, n * n + k) == off);
            CHECK(ba_packed_to_rowmajor(F, off) == n * n + k);
        }
        CHECK(stored == 36 * ba_packed_blocks(F) + n);
        // every row-major entry: in an upper block -> the offset that stores it; below the block diagonal -> absent
        int absent = 0;
        for (int e = 0; e < total; e++) {
            const int off = ba_packed_from_rowmajor(F, e);
            const bool lower = e < n * n && (e / n) / 6 > (e % n) / 6;
            if (lower) { CHECK(off == -1); absent++; continue; }
            CHECK(off >= 0 && off < size && owner[off] == e);
        }
        CHECK(absent == 36 * (F * (F - 1) / 2));
        // every packed offset: a stored entry, or block slack that maps to nothing
        for (int off = 0; off < size; off++) {
            const int e = ba_packed_to_rowmajor(F, off);
            CHECK(e == owner[off]);
            if (e >= 0) CHECK(ba_packed_from_rowmajor(F, e) == off);
        }
        // k_ba_reduce's slots: the packed offsets as they lie, then the entries below the block diagonal; every row-major entry once
        const int slots = ba_packed_reduce_slots(F);
        CHECK(slots == size + absent);
        std::vector<int> hits(total, 0);
        for (int t = 0; t < slots; t++) {
            const int e = ba_packed_reduce_entry(F, t);
            if (t < size) { CHECK(e == owner[t]); }
            else CHECK(e >= 0 && e < n * n && ba_packed_from_rowmajor(F, e) == -1);
            if (e >= 0) { CHECK(e < total); hits[e]++; }
        }
        for (int e = 0; e < total; e++) CHECK(hits[e] == 1);
        free(owner);
    }
    printf("ok: packed upper-block map, F = 1..10, pitch %d\n", BA_PACKED_PITCH);
    return 0;
}
