// Local BA, host side of ONE LM pass of one problem: validation, graph membership, the free set, the factor list ordered by
// (landmark, free index, pair, side), the slot table, the BetweenFactor chain, the second graph's statistics, report and result
// write-out.  Shared by the one-problem path (ba_run) and the batched one (ba_run_batch) of ba.hip.  Pure host code (no HIP calls,
// no streams, no set_error): tests/native/ba_host_order.cpp runs it on the CPU under ASan / UBSan.
#pragma once
#include "ba_types.hpp"
#include "ba_pool.hpp"
#include "../../include/vslam_hip.h"
#include <algorithm>
#include <cstring>
#include <functional>
#include <vector>

namespace vslam {

// Host side of a pinned upload arena: a bump allocator over [h, h + cap) with 256-byte aligned blocks.  take() past the end
// returns null (and keeps counting: `used` is then what the layout needs).
struct BaArenaView {
    uint8_t* h = nullptr;
    size_t cap = 0, used = 0;
    void reset() { used = 0; }
    template <class T> T* take(size_t count) {
        used = (used + 255) & ~(size_t)255;
        T* p = (T*)(h + used);
        used += std::max<size_t>(count, 1) * sizeof(T);
        return used <= cap ? p : nullptr;
    }
};
struct BaHostTmp {
    std::vector<uint8_t> kfPresent, lmPresent;
    std::vector<int> cnt, fidx, lpOf, order, fill, key, src, ns;
};
// When the host scans go to the pool: pair scans by landmark range from parPairs pairs on (ranges of >= parLmGrain landmarks),
// landmark chunks from chunkLm landmarks on (chunks of >= chunkGrain).  Tests lower them to reach the pooled forms with small problems.
struct BaHostTune { int parPairs = 200000, parLmGrain = 4096, chunkLm = 16384, chunkGrain = 2048; };
inline int ba_lm_chunks(const BaPool* pool, int Lp, const BaHostTune& tune) {
    return (pool && !pool->workers.empty() && Lp >= tune.chunkLm) ? std::max(1, std::min(32, Lp / tune.chunkGrain)) : 1;
}

// ---- validation of a problem: which rule failed (the callers word their own messages) -----------------------------------------
enum { BA_PROBLEM_OK = 0, BA_PROBLEM_INVALID = 1, BA_PROBLEM_PAIR_RANGE = 2 };
inline bool ba_check_args(const vslam_ba_problem* P, const vslam_ba_result* R) {
    return !(!P || !R || P->n_kf < 1 || P->n_lm < 0 || P->n_pairs < 0 || P->n_levels < 1 || P->n_levels > BA_MAX_LEVELS ||
             !P->kf_pose_wc || !P->kf_id || !P->kf_fixed || !P->kf_local || !P->sigma_factor || !P->inv_sigma_factor ||
             !R->kf_pose_wc || !R->lm_xyz || !R->pair_wrong || (P->n_lm > 0 && !P->lm_xyz) ||
             (P->n_pairs > 0 && (!P->pair_kf || !P->pair_lm || !P->pair_flags || !P->pair_uv || !P->pair_octave)));
}
// pair indices and octaves in range; with a pool the pairs are split over its workers and the caller (1.2 M pairs: ~1 ms on one core)
inline bool ba_check_pairs(const vslam_ba_problem* P, BaPool* pool = nullptr) {
    const int K = P->n_kf, L = P->n_lm, NP = P->n_pairs;
    auto in_range = [&](int p0, int p1) {
        for (int p = p0; p < p1; p++)
            if (P->pair_kf[p] < 0 || P->pair_kf[p] >= K || P->pair_lm[p] < 0 || P->pair_lm[p] >= L ||
                P->pair_octave[2 * p] < 0 || P->pair_octave[2 * p] >= P->n_levels || P->pair_octave[2 * p + 1] < 0 ||
                P->pair_octave[2 * p + 1] >= P->n_levels) return false;
        return true;
    };
    if (!pool) return in_range(0, NP);
    const int nr = (int)pool->workers.size() + 1;
    std::vector<uint8_t> ok(nr, 1);
    pool->run(nr, [&](int r) { ok[r] = in_range((int)((long long)NP * r / nr), (int)((long long)NP * (r + 1) / nr)) ? 1 : 0; });
    return std::find(ok.begin(), ok.end(), 0) == ok.end();
}
inline int ba_check_problem(const vslam_ba_problem* P, const vslam_ba_result* R, BaPool* pool = nullptr) {
    return !ba_check_args(P, R) ? BA_PROBLEM_INVALID : !ba_check_pairs(P, pool) ? BA_PROBLEM_PAIR_RANGE : BA_PROBLEM_OK;
}

// armed LM control block of pass ps (5 then 10 iterations)
inline void ba_init_ctl(double* h_ctl, int ps, int nAct) {
    for (int i = 0; i < CTL_DOUBLES; i++) h_ctl[i] = 0;
    h_ctl[CTL_LAMBDA] = 1e-5;
    int* ci = (int*)(h_ctl + CTL_INTS);
    ci[CI_STATE] = BA_LINEARIZE; ci[CI_SEL] = 0; ci[CI_ITER] = 0; ci[CI_INNER] = 0; ci[CI_MAXIT] = ps == 0 ? 5 : 10; ci[CI_FIRST] = 1;
    ci[CI_NACT] = nAct;
}

// the second graph (first-pass structure, pairs masked by the chi2 flags): BaPassHost::second_pass
struct BaSecondPass {
    long long NF2 = 0, Lp2 = 0, k2 = 0;       // factors; with `same` also landmarks and the sum of squared slot counts (this rank's shard)
    bool same = false;                        // same keyframes => same free set, same BetweenFactor chain; landmarks may only drop out
    std::vector<uint8_t> kfP2, lmP2;          // membership of the second graph
};

struct BaPassHost {
    int NF = 0, F = 0, n = 0, Lp = 0, NE = 0, maxSlots = 1, nSlotEntries = 0, maxFac = 1;
    long long sumK2 = 0;
    BaHostTune tune;
    double* h_ctl = nullptr; BaDev* h_D = nullptr;
    int *h_facKf = nullptr, *h_facFi = nullptr, *h_facLp = nullptr, *h_facLm = nullptr, *h_facPair = nullptr;
    double *h_facZ = nullptr, *h_facIs = nullptr; uint8_t* h_facRight = nullptr;
    int *h_lpStart = nullptr, *h_lpSlotStart = nullptr, *h_lpOrig = nullptr, *h_slotStart = nullptr, *h_slotFi = nullptr, *h_fidx = nullptr;
    BaEdge* h_edges = nullptr; uint8_t *h_kfPresent = nullptr, *h_lmPresent = nullptr;

    // Large problems (the C5 window: 1.2 M pairs) split the pair scans over the pool by LANDMARK RANGE: every worker reads all pairs
    // and handles those whose landmark falls in its range - no atomics, the pair order inside a landmark is kept.
    int par_ranges(const BaPool* pool, int NP, int L) const {
        return (pool && !pool->workers.empty() && NP >= tune.parPairs) ? std::min((int)pool->workers.size() + 1, std::max(1, L / tune.parLmGrain)) : 1;
    }
    // One scan of the unmasked pairs: keyframe / landmark membership (global) and this rank's factors per pair (`add(l, c)`, called
    // by the one worker that owns landmark l).  Returns the factor count of the shard.
    template <class Add>
    long long scan_pairs(const vslam_ba_problem* P, const uint8_t* wrong, int rank, int world, BaPool* pool, uint8_t* kfPres, uint8_t* lmPres, Add add) const {
        const int K = P->n_kf, L = P->n_lm, NP = P->n_pairs;
        const int nr = par_ranges(pool, NP, L);
        std::vector<long long> nfPart(nr, 0);
        std::vector<std::vector<uint8_t>> kfPart(nr > 1 ? nr : 0);
        auto scan = [&](int r) {
            const int l0 = (int)((long long)L * r / nr), l1 = (int)((long long)L * (r + 1) / nr);
            uint8_t* kfp = nr > 1 ? (kfPart[r].assign(K, 0), kfPart[r].data()) : kfPres;
            long long nf = 0;
            for (int p = 0; p < NP; p++) {
                const int l = P->pair_lm[p];
                if (l < l0 || l >= l1 || wrong[p]) continue;
                const int fl = P->pair_flags[p] & 3;
                if (!fl) continue;
                kfp[P->pair_kf[p]] = 1; lmPres[l] = 1;                    // graph membership is global
                if (world > 1 && l % world != rank) continue;              // landmark shard of this rank (no division for the one-rank case)
                const int c = (fl & 1) + (fl >> 1);
                add(l, c); nf += c;
            }
            nfPart[r] = nf;
        };
        if (nr > 1) pool->run(nr, scan); else scan(0);
        long long nf = 0;
        for (int r = 0; r < nr; r++) { nf += nfPart[r]; if (nr > 1) for (int k = 0; k < K; k++) kfPres[k] |= kfPart[r][k]; }
        return nf;
    }
    // membership, free set, landmark shard, factor counts
    void count(const vslam_ba_problem* P, const uint8_t* wrong, int rank, int world, BaHostTmp& T, BaPool* pool = nullptr) {
        const int K = P->n_kf, L = P->n_lm;
        T.kfPresent.assign(K, 0); T.lmPresent.assign(L, 0); T.cnt.assign((size_t)L + 1, 0);
        NF = (int)scan_pairs(P, wrong, rank, world, pool, T.kfPresent.data(), T.lmPresent.data(), [&](int l, int c) { T.cnt[l] += c; });
        T.lpOf.assign(L, -1);
        Lp = 0;
        for (int l = 0; l < L; l++) if (T.lmPresent[l] && l % world == rank) T.lpOf[l] = Lp++;
        free_set_and_edges(P, rank, T);
    }
    // free keyframes and the BetweenFactor chain from T.kfPresent (shared by the host and the device ordering)
    void free_set_and_edges(const vslam_ba_problem* P, int rank, BaHostTmp& T) {
        const int K = P->n_kf;
        T.fidx.assign(K, -1);
        F = 0;
        for (int k = 0; k < K; k++) if (T.kfPresent[k] && !P->kf_fixed[k]) T.fidx[k] = F++;
        n = 6 * F;
        // edges: id-consecutive keyframes of this pass's graph (src/OptimizationBA.cpp:750-768)
        T.order.clear();
        for (int k = 0; k < K; k++) if (T.kfPresent[k]) T.order.push_back(k);
        std::sort(T.order.begin(), T.order.end(), [&](int a, int b) { return P->kf_id[a] < P->kf_id[b]; });
        // the BetweenFactor chain is counted once (rank 0); S is summed over ranks
        NE = rank == 0 ? std::max((int)T.order.size() - 1, 0) : 0;
    }
    size_t arena_bytes(int K, int L, int edgeSlots) const {
        return 8192 + (size_t)NF * 56 + ((size_t)NF + Lp + 2) * 8 + ((size_t)Lp + 2) * 12 + (size_t)K * 8 + L +
               (size_t)edgeSlots * NE * sizeof(BaEdge) + 26 * 256 + sizeof(BaDev);
    }
    bool take(BaArenaView& A, int K, int L, int edgeSlots) {
        h_ctl = A.take<double>(CTL_DOUBLES);
        h_D = A.take<BaDev>(1);                     // the kernels' argument block (a one-entry lane table)
        h_facKf = A.take<int>(NF); h_facFi = A.take<int>(NF); h_facLp = A.take<int>(NF); h_facLm = A.take<int>(NF);
        h_facZ = A.take<double>((size_t)2 * NF); h_facIs = A.take<double>(NF);
        h_facRight = A.take<uint8_t>(NF);
        h_facPair = A.take<int>(NF);
        h_lpStart = A.take<int>(Lp + 1); h_lpSlotStart = A.take<int>(Lp + 1); h_lpOrig = A.take<int>(Lp);
        h_slotStart = A.take<int>((size_t)NF + Lp + 1); h_slotFi = A.take<int>((size_t)NF + Lp + 1);
        h_fidx = A.take<int>(K);
        h_edges = A.take<BaEdge>((size_t)edgeSlots * NE);
        h_kfPresent = A.take<uint8_t>(K); h_lmPresent = A.take<uint8_t>(L);
        return h_lmPresent != nullptr;
    }
    // bucket by landmark (counting sort, pair order preserved), order each short bucket by free index, emit the arrays
    void fill(const vslam_ba_problem* P, const uint8_t* wrong, int rank, int world, BaHostTmp& T, const DPose* pose0, BaPool* pool, int edgeSlots) {
        const int L = P->n_lm, NP = P->n_pairs;
        for (int l = 0; l < L; l++) if (T.lpOf[l] >= 0) { h_lpOrig[T.lpOf[l]] = l; }
        {
            int run = 0;
            for (int lp = 0; lp < Lp; lp++) { h_lpStart[lp] = run; run += T.cnt[h_lpOrig[lp]]; }
            h_lpStart[Lp] = run;
        }
        T.fill.assign(h_lpStart, h_lpStart + Lp);
        T.key.resize(NF); T.src.resize(NF);
        {
            const int nr = par_ranges(pool, NP, L);
            auto scatter = [&](int r) {
                const int l0 = (int)((long long)L * r / nr), l1 = (int)((long long)L * (r + 1) / nr);
                for (int p = 0; p < NP; p++) {
                    const int l = P->pair_lm[p];
                    if (l < l0 || l >= l1 || wrong[p] || l % world != rank) continue;
                    const int lp = T.lpOf[l];
                    const int fi = T.fidx[P->pair_kf[p]];
                    for (int side = 0; side < 2; side++) {
                        if (!((P->pair_flags[p] >> side) & 1)) continue;
                        const int pos = T.fill[lp]++;
                        T.key[pos] = fi; T.src[pos] = 2 * p + side;
                    }
                }
            };
            if (nr > 1) pool->run(nr, scatter); else scatter(0);
        }
        // landmark ranges in parallel: (1) order each bucket by free index and count its slots, (2) after the slot prefix,
        // write the factor arrays and the slot table.
        // Slot table: inside a landmark the factors of fixed keyframes (fi = -1) come first, then one
        // "slot" per free keyframe (its left and/or right factor).  Padded layout: per landmark the slot
        // starts followed by an end sentinel, so slot s spans [slotStart[s0+s], slotStart[s0+s+1]).
        T.ns.resize(Lp);
        const int nChunk = pool ? std::max(1, std::min(32, Lp / 64)) : 1;
        auto for_lps = [&](auto body) {       // body(lp) over the landmarks, chunks on the pool
            auto fn = [&](int c) { for (int lp = (int)((long long)Lp * c / nChunk), a1 = (int)((long long)Lp * (c + 1) / nChunk); lp < a1; lp++) body(lp); };
            if (pool && nChunk > 1) pool->run(nChunk, fn); else fn(0);
        };
        for_lps([&](int lp) {
            const int f0 = h_lpStart[lp], f1 = h_lpStart[lp + 1];
            for (int i = f0 + 1; i < f1; i++) {          // stable insertion sort by free index (buckets are ~10 long)
                const int k = T.key[i], v = T.src[i];
                int j = i - 1;
                while (j >= f0 && T.key[j] > k) { T.key[j + 1] = T.key[j]; T.src[j + 1] = T.src[j]; j--; }
                T.key[j + 1] = k; T.src[j + 1] = v;
            }
            int lastFi = -2, ns = 0;
            for (int f = f0; f < f1; f++) { const int fi = T.key[f]; if (fi >= 0 && fi != lastFi) { lastFi = fi; ns++; } }
            T.ns[lp] = ns;
        });
        maxSlots = 1; nSlotEntries = 0; sumK2 = 0; maxFac = 1;
        for (int lp = 0; lp < Lp; lp++) {
            h_lpSlotStart[lp] = nSlotEntries;
            maxFac = std::max(maxFac, h_lpStart[lp + 1] - h_lpStart[lp]);
            nSlotEntries += T.ns[lp] + 1;
            maxSlots = std::max(maxSlots, T.ns[lp]);
            sumK2 += (long long)T.ns[lp] * T.ns[lp];
        }
        for_lps([&](int lp) {
            const int f0 = h_lpStart[lp], f1 = h_lpStart[lp + 1];
            int se = h_lpSlotStart[lp], lastFi = -2;
            for (int f = f0; f < f1; f++) {
                const int fi = T.key[f], p = T.src[f] >> 1, side = T.src[f] & 1;
                if (fi >= 0 && fi != lastFi) { h_slotStart[se] = f; h_slotFi[se] = fi; se++; lastFi = fi; }
                h_facKf[f] = P->pair_kf[p]; h_facFi[f] = fi; h_facLp[f] = lp; h_facLm[f] = P->pair_lm[p];
                h_facZ[2 * (size_t)f] = P->pair_uv[4 * (size_t)p + 2 * side]; h_facZ[2 * (size_t)f + 1] = P->pair_uv[4 * (size_t)p + 2 * side + 1];
                h_facIs[f] = 1.0 / (1.0 / (double)P->inv_sigma_factor[P->pair_octave[2 * p + side]]);
                h_facRight[f] = (uint8_t)side;
                h_facPair[f] = p;
            }
            h_slotStart[se] = f1; h_slotFi[se] = -1;     // end sentinel
        });
        h_lpSlotStart[Lp] = nSlotEntries;
        for (int l = 0; l < L; l++) h_lmPresent[l] = T.lmPresent[l];
        fill_small(P, T, pose0, edgeSlots);
    }
    // the host-written small arrays: free index, membership of the keyframes, BetweenFactor edges
    void fill_small(const vslam_ba_problem* P, BaHostTmp& T, const DPose* pose0, int edgeSlots) {
        const int K = P->n_kf;
        for (int k = 0; k < K; k++) { h_fidx[k] = T.fidx[k]; h_kfPresent[k] = T.kfPresent[k]; }
        for (int i = 0; i < NE; i++) {
            BaEdge e{};
            e.a = T.order[i]; e.b = T.order[i + 1]; e.fa = T.fidx[e.a]; e.fb = T.fidx[e.b];
            DPose ai;
            pose_inverse(pose0[e.a], ai);
            pose_compose(ai, pose0[e.b], e.measured);
            for (int sl = 0; sl < edgeSlots; sl++) h_edges[(size_t)sl * NE + i] = e;
        }
    }
    // Membership / statistics of the second graph from the chi2 flags `wrong`, on the structure this pass filled (T as count() left
    // it): the same scan as count(); when the keyframes are the same also the landmarks left and the slot statistics of the
    // masked factor list (landmark chunks on the pool for large problems).  All sums are integers: pooled = serial.
    void second_pass(const vslam_ba_problem* P, const uint8_t* wrong, int rank, int world, const BaHostTmp& T, BaPool* pool, BaSecondPass& out) const {
        const int K = P->n_kf, L = P->n_lm;
        out = BaSecondPass{};
        out.kfP2.assign(K, 0); out.lmP2.assign(std::max(L, 1), 0);
        out.NF2 = scan_pairs(P, wrong, rank, world, pool, out.kfP2.data(), out.lmP2.data(), [](int, int) {});
        out.same = std::equal(out.kfP2.begin(), out.kfP2.end(), T.kfPresent.begin());
        if (!out.same) return;
        const int nc = ba_lm_chunks(pool, Lp, tune);
        std::vector<long long> k2Part(nc, 0), lpPart(nc, 0);
        auto part = [&](int c) {
            long long kk = 0, ll = 0;
            for (int l = (int)((long long)L * c / nc), l1 = (int)((long long)L * (c + 1) / nc); l < l1; l++) if (world == 1 || l % world == rank) ll += out.lmP2[l];
            for (int lp = (int)((long long)Lp * c / nc), lp1 = (int)((long long)Lp * (c + 1) / nc); lp < lp1; lp++) {
                int ns = 0, last = -2;
                for (int f = h_lpStart[lp]; f < h_lpStart[lp + 1]; f++) {
                    if (wrong[h_facPair[f]]) continue;
                    const int fi = h_facFi[f];
                    if (fi >= 0 && fi != last) { last = fi; ns++; }
                }
                kk += (long long)ns * ns;
            }
            k2Part[c] = kk; lpPart[c] = ll;
        };
        if (nc > 1) pool->run(nc, part); else part(0);
        for (int c = 0; c < nc; c++) { out.k2 += k2Part[c]; out.Lp2 += lpPart[c]; }
    }
};

// report of pass `pass` from a control block (as the device left it), with the pass's work figures
inline void ba_write_report(vslam_ba_result* R, int pass, const double* ctl, int F, long long nf, long long lp, long long k2) {
    const int* ci = (const int*)(ctl + CTL_INTS);
    R->report[pass].iterations = ci[CI_ITER];
    R->report[pass].inner_iterations = ci[CI_INNER];
    R->report[pass].initial_error = ctl[CTL_INIT_ERR];
    R->report[pass].final_error = ctl[CTL_ERROR];
    R->report[pass].lambda = ctl[CTL_LAMBDA];
    R->n_residuals = nf; R->n_landmarks = lp; R->n_free_kf = F; R->sum_k2 = k2;
    R->rounds = (pass == 0 ? 0 : R->rounds) + ci[CI_ROUNDS];
}
// final values and flags into the caller's arrays
inline void ba_write_result(vslam_ba_result* R, const DPose* poses, const double* lm, const uint8_t* wrong, int K, int L, int NP) {
    for (int k = 0; k < K; k++) pose_to_rm16(poses[k], R->kf_pose_wc + 16 * (size_t)k);
    if (L) memcpy(R->lm_xyz, lm, (size_t)3 * L * sizeof(double));
    if (NP) memcpy(R->pair_wrong, wrong, NP);
}

}  // namespace vslam
