// Packed form of the reduced camera system of a tracker window (k_ba_schur2's LDS accumulator and the partials k_ba_reduce sums).
// Only the upper block triangle of S is ever written (a landmark's slots are sorted by free index) or read (the solves take the
// upper triangle), so the packed form keeps the 6x6 blocks (a <= b) of the F = n / 6 free keyframes, each block whole and row-major
// with row pitch 6, in row order of the block triangle, BA_PACKED_PITCH doubles apart; the right-hand side follows the blocks.
//   F = 10: 55 * 37 + 60 = 2 095 doubles against n * n + n = 3 660 row-major.
// The pitch is odd so that consecutive blocks start on different 8-byte LDS bank positions (a 36-double pitch puts every block
// of a landmark on 4 of the 16 positions); the slack double of a block is never written and stays zero.
#pragma once

#ifndef BA_PACKED_PITCH
#define BA_PACKED_PITCH 37
#endif

#ifndef BA_PACKED_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define BA_PACKED_HD __host__ __device__ inline
#else
#define BA_PACKED_HD inline
#endif
#endif

// number of blocks of the upper block triangle
BA_PACKED_HD int ba_packed_blocks(int F) { return F * (F + 1) / 2; }
// ordinal of block (a <= b): rows of the triangle one after the other
BA_PACKED_HD int ba_packed_block(int F, int a, int b) { return a * (2 * F - a + 1) / 2 + (b - a); }
// offset of entry (i, j) of block (a <= b)
BA_PACKED_HD int ba_packed_off(int F, int a, int b, int i, int j) { return ba_packed_block(F, a, b) * BA_PACKED_PITCH + 6 * i + j; }
// offset of the right-hand side (6 F entries, contiguous)
BA_PACKED_HD int ba_packed_rhs(int F) { return ba_packed_blocks(F) * BA_PACKED_PITCH; }
// doubles of the packed system: blocks, then the right-hand side
BA_PACKED_HD int ba_packed_doubles(int F) { return ba_packed_rhs(F) + 6 * F; }
// Row-major entry e of [S (n x n) | rhs (n)], n = 6 F  ->  packed offset; -1: the entry lies below the block diagonal (never stored).
BA_PACKED_HD int ba_packed_from_rowmajor(int F, int e) {
    const int n = 6 * F;
    if (e >= n * n) return ba_packed_rhs(F) + (e - n * n);
    const int r = e / n, c = e - r * n, a = r / 6, b = c / 6;
    if (a > b) return -1;
    return ba_packed_off(F, a, b, r - 6 * a, c - 6 * b);
}
// Packed offset -> row-major entry; -1: the slack of a block.
BA_PACKED_HD int ba_packed_to_rowmajor(int F, int off) {
    const int n = 6 * F, rhs = ba_packed_rhs(F);
    if (off >= rhs) return n * n + (off - rhs);
    const int blk = off / BA_PACKED_PITCH, in = off - blk * BA_PACKED_PITCH;
    if (in >= 36) return -1;
    int a = 0, first = 0;                    // block row a starts at ordinal `first` and holds F - a blocks
    while (blk >= first + F - a) { first += F - a; a++; }
    const int b = a + (blk - first), i = in / 6, j = in - 6 * i;
    return (6 * a + i) * n + 6 * b + j;
}
// k_ba_reduce over packed partials: slot t < ba_packed_doubles(F) sums packed offset t of every partial (consecutive threads read
// consecutive doubles) and owns the row-major entry that offset stores; the slots behind them own the entries below the block
// diagonal, which are in no partial (block (a > b) at ordinal a (a - 1) / 2 + b, 36 entries each).  Every row-major entry of
// [S | rhs] belongs to exactly one slot; -1: the slack of a block, no entry.
BA_PACKED_HD int ba_packed_reduce_slots(int F) { return ba_packed_doubles(F) + 36 * (F * (F - 1) / 2); }
BA_PACKED_HD int ba_packed_reduce_entry(int F, int t) {
    const int size = ba_packed_doubles(F);
    if (t < size) return ba_packed_to_rowmajor(F, t);
    const int k = t - size, lb = k / 36, in = k - 36 * lb;
    int a = 1;
    while (lb >= a * (a + 1) / 2) a++;       // blocks (a, 0 .. a - 1) start at ordinal a (a - 1) / 2
    const int b = lb - a * (a - 1) / 2, i = in / 6, j = in - 6 * i;
    return (6 * a + i) * (6 * F) + 6 * b + j;
}
