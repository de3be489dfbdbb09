// Index rule of the compact stopper array of k_ssc (the classes with SscCfg<M>::COMPACT; ssc.hip): the two stopper lists of a
// Hoare partition in ONE u16 array with one slot per element of the segment.
//
// Segment [f, e), pivot at f after median-of-3, m = e - f - 1 elements behind it.  The left stoppers (key >= pivot, ascending
// position) have ranks 0, 1, ... from the left, the right stoppers (key <= pivot, descending position) ranks 0, 1, ... from the
// right; exchange k swaps left rank k with right rank k while they have not crossed.  K exchanges touch 2 K distinct positions
// of the m, so K <= m / 2 and the partition only ever looks at ranks 0 .. K of either list.  Hence with the cap
//     C = (m + 1) >> 1 = (e - f) >> 1
// the slice [f, e) of the array holds both lists without collision (2 C <= e - f): left rank r < C at f + r, right rank r < C
// at e - 1 - r.  A rank >= C is never stored and reads as "crossed": the search for K stops at C, and L[K] enters the cut only
// if K < nL and K < C.  The one case that drops a rank the sequential loop looks at is m even, K = m / 2: every position has
// been exchanged, L[K] and R[K] lie behind the cap, and L[K] >= R[K - 1] there (the cut is R[K - 1] either way).
// The register walk (ssc_small_segment) applies the same rule to the hi - lo slots of every sub-segment [lo, hi).
// Host-includable: tests/native/ssc_stoppers.cpp proves the rule against the sequential loop of libstdc++.
#pragma once

#ifndef SSC_STOP_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define SSC_STOP_HD __host__ __device__ __forceinline__
#else
#define SSC_STOP_HD inline
#endif
#endif

// ranks stored per side of segment [f, e)
SSC_STOP_HD int ssc_stop_cap(int f, int e) { return (e - f) >> 1; }
// slot of the left / right stopper of rank r < ssc_stop_cap(f, e)
SSC_STOP_HD int ssc_stop_left(int f, int r) { return f + r; }
SSC_STOP_HD int ssc_stop_right(int e, int r) { return e - 1 - r; }
// pairs (left rank k, right rank k) the search for K may test: nL / nR stoppers exist, ranks >= cap read as crossed
SSC_STOP_HD int ssc_stop_pairs(int nL, int nR, int cap) { return nL < nR ? (nL < cap ? nL : cap) : (nR < cap ? nR : cap); }
// after K exchanges: does L[K] exist and is it stored (then the cut is min(R[K - 1], L[K]), else R[K - 1] or e)
SSC_STOP_HD bool ssc_stop_has_left(int K, int nL, int cap) { return K < nL && K < cap; }
