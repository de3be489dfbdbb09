// Local BA: launch geometry as pure functions of a problem's (or a cohort's) shape - LDS sizes, waves per workgroup, grids, the
// solve kind, the window tiling and the host form of the window work lists.  No device calls; environment overrides arrive as
// knobs read in ba.hip.  tests/native/ba_host_order.cpp sweeps these on the CPU, tests/test_ba_plan.py the batch plan.
#pragma once
#include "ba_types.hpp"
#include "ba_order_host.hpp"
#include <initializer_list>

namespace vslam {

constexpr int BA_NCU = 256;
constexpr size_t BA_LDS_SOFT = 150 * 1024;      // what the wave choices aim for (the rest of the 160 KB: static LDS, slack)
constexpr int BA_SCHUR_LPW = 64 / BA_LPL_SCHUR, BA_BACK_LPW = 64 / BA_LPL_BACK;      // landmarks per wave
// k_ba_schur / k_ba_back: nw waves = nw * LPW landmark units per workgroup, W staging by slots; `copies` of the system next to it
inline size_t ba_stage_lds(int nw, int maxSlots) { return (size_t)nw * BA_SCHUR_LPW * 2 * maxSlots * 18 * sizeof(double) + (size_t)nw * BA_SCHUR_LPW * maxSlots * sizeof(int) + 16; }
inline size_t ba_schur_lds(int nw, int copies, size_t sysDoubles, int maxSlots) { return copies * sysDoubles * sizeof(double) + ba_stage_lds(nw, maxSlots); }
inline size_t ba_back_lds(int nw, int maxSlots) { return (size_t)nw * BA_BACK_LPW * maxSlots * 18 * sizeof(double) + (size_t)nw * BA_BACK_LPW * maxSlots * sizeof(int) + 16; }
// Waves per workgroup of k_ba_schur.  One workgroup for all NB candidates (sharedW: the W blocks are built once) when NB copies of
// the system fit LDS with a wave count of the menu (at most `cap`); else `start` waves, halved until one copy fits.
// A 16-wave workgroup with ~100 KB of LDS is the fastest form on an idle GPU, but it must find a whole CU's worth of free wave slots
// and LDS when the lockstep groups' wide kernels fill the chip; slimmer workgroups slot in between them (hence the caps).
inline int ba_schur_waves(int NB, bool allowShared, int cap, int start, size_t sysDoubles, int maxSlots, int& sharedW) {
    sharedW = 0;
    if (NB > 1 && allowShared)
        for (int nw : {16, 12, 8, 6, 4, 2})
            if (nw <= cap && ba_schur_lds(nw, NB, sysDoubles, maxSlots) <= BA_LDS_SOFT) { sharedW = 1; return nw; }
    while (start > 2 && ba_schur_lds(start, 1, sysDoubles, maxSlots) > BA_LDS_SOFT) start /= 2;
    return start;
}
inline int ba_back_waves(int cap, int maxSlots) {
    int nw = std::min(BA_SCHUR_WAVES / BA_BACK_LPW, cap);
    while (nw > 1 && ba_back_lds(nw, maxSlots) > BA_LDS_SOFT) nw /= 2;
    return nw;
}
inline size_t ba_mfma_lds() { return ((size_t)BA_MFMA_N * BA_MFMA_LD + 16 + BA_MFMA_N) * sizeof(double); }
// which reduced-camera solve takes a system of n unknowns: one wave with MFMA tiles, one wave row-per-lane, eight waves with MFMA
// tiles, else the block-column Cholesky / the row-per-thread LDS form (one-problem path only)
inline int ba_solve_kind(int n, bool useMfma) {
    return (n <= 64 && useMfma) ? BA_SOLVE_MFMA64 : n <= BA_WAVE_N ? BA_SOLVE_WAVE : (n <= BA_MFMA_N && useMfma) ? BA_SOLVE_MFMA : BA_SOLVE_LARGE;
}

// ---- one problem (ba_run) --------------------------------------------------------------------------------------------------------
// Windowed accumulation (F > BA_LDS_MAX_F): TB keyframes per block row - the largest tile whose NB copies leave room for >= 8 waves
// of staging; tbOverride > 0 sets it.  k_win_lists (device ordering) keeps a landmark's block rows in a 64-bit mask: at most 64 rows.
struct BaWinTile { int TB = 0, nBR = 0, nWin = 0, T = 0, TP = 0, tileDoubles = 0; size_t lds = 0; const char* why = nullptr; };
inline BaWinTile ba_window_tile(int F, int NB, bool devOrder, int tbOverride) {
    BaWinTile w;
    const size_t metaB = (size_t)BA_SCHUR_WAVES * BA_WIN_META * sizeof(int) + 16;
    w.TB = 4;
    for (int tb : {32, 24, 16, 12, 8, 6, 4}) {
        const size_t tileB = ((size_t)6 * tb * (6 * tb + 1) + 6 * tb) * sizeof(double) * NB;
        if (tileB + metaB <= BA_LDS_SOFT) { w.TB = tb; break; }
    }
    if (tbOverride > 0) w.TB = std::min(32, tbOverride);
    if (devOrder && (F + w.TB - 1) / w.TB > 64) w.TB = (F + 63) / 64;
    w.nBR = (F + w.TB - 1) / w.TB; w.nWin = w.nBR * (w.nBR + 1) / 2;
    w.T = 6 * w.TB; w.TP = w.T + 1; w.tileDoubles = w.T * w.TP + w.T;
    w.lds = (size_t)w.tileDoubles * sizeof(double) * NB + metaB;
    if (w.lds > (size_t)BA_LDS_BYTES) w.why = "local BA: window tile does not fit LDS";
    else if (devOrder && w.nBR > 64) w.why = "local BA: more than 64 block rows are not supported with the device ordering";
    return w;
}
struct BaSingleShape { int NF, Lp, F, NE, maxSlots, NB; bool useMfma, devOrder; };
struct BaSingleKnobs { int schurWavesCap = BA_SCHUR_WAVES, backWavesCap = 64, windowTB = 0; bool sharedW = true; };      // VSLAM_BA_SCHUR_WAVES / _BACK_WAVES / _WINDOW_TB / _NO_SHARED_W
struct BaSinglePlan {
    const char* why = nullptr;            // != null: the problem is refused (VSLAM_ERR_CAPACITY) with this message
    bool ldsS = false; BaWinTile win;     // the system in LDS (k_ba_schur), or windowed (k_ba_schur_win)
    int obsBlocks = 0, schurWaves = 0, sharedW = 0, lmBlocks = 0, backWaves = 0, backBlocks = 0, sharedBack = 0;
    size_t schurLds = 0, backLds = 0;
    int solveKind = 0, ldA = 0, cholN = 0; bool solveLds = false, useChol = false;
    size_t solveLdsBytes = 0, mfmaLds = 0, cholColLds = 0, cholBackLds = 0;
};
inline BaSinglePlan ba_single_plan(const BaSingleShape& s, const BaSingleKnobs& kn) {
    BaSinglePlan p;
    const int n = 6 * s.F, NB = s.NB;
    if (s.F > BA_MAX_FREE_KF) { p.why = "local BA: more than 170 free keyframes is not supported"; return p; }
    p.obsBlocks = std::max(1, std::min((s.NF + 255) / 256, 4 * BA_NCU));
    p.ldsS = s.F <= BA_LDS_MAX_F;
    const size_t sysDoubles = (size_t)n * n + n;
    if (p.ldsS) {
        p.schurWaves = ba_schur_waves(NB, kn.sharedW, kn.schurWavesCap, kn.schurWavesCap, sysDoubles, s.maxSlots, p.sharedW);
        p.schurLds = ba_schur_lds(p.schurWaves, p.sharedW ? NB : 1, sysDoubles, s.maxSlots);
    } else {
        p.win = ba_window_tile(s.F, NB, s.devOrder, kn.windowTB);
        if (p.win.why) { p.why = p.win.why; return p; }
        p.schurWaves = BA_SCHUR_WAVES;
        p.schurLds = p.win.lds;
    }
    const int schurUnits = p.schurWaves * BA_SCHUR_LPW;
    p.lmBlocks = std::max(1, std::min((s.Lp + schurUnits - 1) / schurUnits, BA_NCU));
    p.backWaves = ba_back_waves(kn.backWavesCap, s.maxSlots);
    p.backBlocks = std::max(1, std::min((s.Lp + p.backWaves * BA_BACK_LPW - 1) / (p.backWaves * BA_BACK_LPW), BA_NCU));
    p.backLds = ba_back_lds(p.backWaves, s.maxSlots);
    p.sharedBack = (NB > 1 && kn.sharedW) ? 1 : 0;
    p.ldA = ((n + 31) / 32) * 32 + 1;     // row stride = 1 (mod 32) doubles: conflict-free row-per-lane access
    p.solveLdsBytes = ((size_t)n * p.ldA + n + 8) * sizeof(double);
    p.solveLds = p.solveLdsBytes <= BA_LDS_SOFT;
    if (p.schurLds > (size_t)BA_LDS_BYTES) { p.why = "local BA: landmark with too many views for the LDS staging"; return p; }
    p.mfmaLds = ba_mfma_lds();
    p.solveKind = ba_solve_kind(n, s.useMfma);
    // larger systems: block-column MFMA Cholesky (k_ba_chol_col / k_ba_chol_back)
    p.useChol = n > BA_MFMA_N && s.useMfma;
    p.cholN = (std::max(n, 1) + CH_B - 1) / CH_B * CH_B;
    p.cholColLds = ((size_t)2 * CH_B * CH_LD + (size_t)CH_B * CH_PLD + 3 * CH_B) * sizeof(double);
    p.cholBackLds = ((size_t)CH_B * CH_LD + p.cholN + 4 * CH_B) * sizeof(double);
    return p;
}

// Host form of the window work lists.  Per landmark the distinct block rows of its slots (sorted by free index); every pair
// (i <= j) of them is one entry of window (row_i, row_j), a <= b at a * nBR - a (a - 1) / 2 + (b - a).  Landmark chunks run on the
// pool: each counts its entries per window, a prefix over (window, chunk) gives every chunk its own segment of every window's
// list - the same order as one sequential sweep.  A window's list is cut into workgroups of >= 256 entries, ~2 per CU overall.
// devWinCnt != null (device ordering: the [nWin + 1] list starts come from k_win_prefix): only the cuts; the lists are left out
// of `pack` (room for them is counted in nInts) and written in place by k_win_lists<1>.
struct BaWinLists {
    std::vector<int> pack;        // winA | winB | winFirst [nWin + 1] | wgWin | wgBegin | wgEnd [max(nWinWg, 1) each] (from oWg) | winLm
    size_t oWg = 0, nInts = 0;    // nInts: the device buffer (with max(total, 1) list entries)
    int nWinWg = 0, total = 0;
};
inline BaWinLists ba_window_lists_host(int Lp, const int* lpSlotStart, const int* slotFi, int TB, int nBR, BaPool* pool, int nCU,
                                       const int* devWinCnt = nullptr, const BaHostTune& tune = BaHostTune{}) {
    BaWinLists out;
    const int nWin = nBR * (nBR + 1) / 2;
    auto win_of = [nBR](int a, int b2) { return a * nBR - a * (a - 1) / 2 + (b2 - a); };     // a <= b2
    std::vector<int> winA(nWin), winB(nWin), winCnt((size_t)nWin + 1, 0);
    for (int a2 = 0; a2 < nBR; a2++) for (int b2 = a2; b2 < nBR; b2++) { winA[win_of(a2, b2)] = a2; winB[win_of(a2, b2)] = b2; }
    if (devWinCnt) winCnt.assign(devWinCnt, devWinCnt + nWin + 1);
    const int nCh = devWinCnt ? 0 : ba_lm_chunks(pool, Lp, tune);
    std::vector<int> chCnt((size_t)nCh * nWin, 0), chOff((size_t)nCh * nWin);
    // one sweep over a chunk's landmarks: fn(window) per entry
    auto sweep = [&](int c, auto fn) {
        std::vector<int> rows(nBR);
        for (int lp = (int)((long long)Lp * c / nCh), a1 = (int)((long long)Lp * (c + 1) / nCh); lp < a1; lp++) {
            int nr = 0, last = -1;
            for (int se = lpSlotStart[lp]; se < lpSlotStart[lp + 1] - 1; se++) {
                const int br = slotFi[se] / TB;
                if (br != last) { rows[nr++] = br; last = br; }
            }
            for (int i = 0; i < nr; i++) for (int j = i; j < nr; j++) fn(lp, win_of(rows[i], rows[j]));
        }
    };
    auto run = [&](const std::function<void(int)>& fn) { if (nCh > 1) pool->run(nCh, fn); else if (nCh == 1) fn(0); };
    run([&](int c) { int* cnt = &chCnt[(size_t)c * nWin]; sweep(c, [&](int, int w) { cnt[w]++; }); });
    if (!devWinCnt) {
        int at = 0;
        for (int w = 0; w < nWin; w++) {
            winCnt[w] = at;
            for (int c = 0; c < nCh; c++) { chOff[(size_t)c * nWin + w] = at; at += chCnt[(size_t)c * nWin + w]; }
        }
        winCnt[nWin] = at;
    }
    const int total = out.total = winCnt[nWin];
    std::vector<int> winLm(devWinCnt ? (size_t)0 : (size_t)std::max(total, 1));
    run([&](int c) { int* off = &chOff[(size_t)c * nWin]; sweep(c, [&](int lp, int w) { winLm[off[w]++] = lp; }); });
    const int chunk = std::max(256, (total + 2 * nCU - 1) / (2 * nCU));
    std::vector<int> wgWin, wgBegin, wgEnd, winFirst((size_t)nWin + 1, 0);
    for (int w = 0; w < nWin; w++) {
        winFirst[w] = (int)wgWin.size();
        for (int i0 = winCnt[w]; i0 < winCnt[w + 1]; i0 += chunk) { wgWin.push_back(w); wgBegin.push_back(i0); wgEnd.push_back(std::min(i0 + chunk, winCnt[w + 1])); }
    }
    winFirst[nWin] = (int)wgWin.size();
    const int nWg = out.nWinWg = (int)wgWin.size();
    out.nInts = (size_t)2 * nWin + (nWin + 1) + (size_t)3 * std::max(nWg, 1) + std::max(total, 1);
    std::vector<int>& pack = out.pack;
    pack.reserve(out.nInts);
    pack.insert(pack.end(), winA.begin(), winA.end()); pack.insert(pack.end(), winB.begin(), winB.end());
    pack.insert(pack.end(), winFirst.begin(), winFirst.end());
    out.oWg = pack.size();
    pack.insert(pack.end(), wgWin.begin(), wgWin.end()); pack.resize(out.oWg + std::max(nWg, 1));
    pack.insert(pack.end(), wgBegin.begin(), wgBegin.end()); pack.resize(out.oWg + 2 * (size_t)std::max(nWg, 1));
    pack.insert(pack.end(), wgEnd.begin(), wgEnd.end()); pack.resize(out.oWg + 3 * (size_t)std::max(nWg, 1));
    pack.insert(pack.end(), winLm.begin(), winLm.end());
    return out;
}

// ---- launch plan of the batch: a pure function of the cohort's shape (exported as vslam_local_ba_batch_plan) -----------------------
struct BaPlanKnobs { bool schur2, back2, sharedW; int s2Waves, b2Waves, schurWaves, lmBlocks, s2Layout; };
// problems outside the batched class (the LDS solve lives in the one-problem path; empty graphs; another rig)
inline bool ba_batch_single(const vslam_ba_lane_shape& s, bool useMfma) {
    return s.own_rig || s.n_free_kf > BA_LDS_MAX_F || s.n_free_kf <= 0 || s.n_factors <= 0 || s.n_pairs <= 0 || (!useMfma && 6 * s.n_free_kf > BA_WAVE_N);
}
inline void ba_batch_plan(const vslam_ba_batch_shape& S, const BaPlanKnobs& kn, vslam_ba_batch_plan& p) {
    p = vslam_ba_batch_plan{};
    const int NB = std::max(1, std::min((int)BA_MAX_NB, (int)S.lookahead));
    const bool useMfma = S.solver == 0;
    p.status = VSLAM_OK; p.lookahead = NB;
    int maxSlots = 1, maxFac = 1, fMax = 0, lpMax = 0, NL = 0;
    for (int i = 0; i < S.n_lanes; i++) {
        const vslam_ba_lane_shape& s = S.lanes[i];
        if (ba_batch_single(s, useMfma)) { p.n_single++; continue; }
        NL++;
        maxSlots = std::max(maxSlots, (int)s.max_slots); maxFac = std::max(maxFac, (int)s.max_factors);
        fMax = std::max(fMax, (int)s.n_free_kf); lpMax = std::max(lpMax, (int)s.n_points);
        p.solve_kinds |= 1 << ba_solve_kind(6 * s.n_free_kf, useMfma);
    }
    p.n_batch = NL; p.f_max = fMax; p.max_slots = maxSlots; p.max_factors = maxFac; p.lp_max = lpMax;
    if (NL == 0) { p.solve_kinds = 0; return; }
    const int nCU = BA_NCU, nMax = 6 * fMax;
    const size_t sysMax = (size_t)nMax * nMax + nMax;
    // k_ba_schur: a wave per landmark, W staging by slots; one workgroup for all lambda candidates (sharedW) when NB copies of the
    // system fit next to the staging
    int sharedW = 0;
    const int schurWaves = ba_schur_waves(NB, kn.sharedW, BA_SCHUR_WAVES, kn.schurWaves ? kn.schurWaves : BA_SCHUR_WAVES, sysMax, maxSlots, sharedW);
    const size_t schurLds = ba_schur_lds(schurWaves, sharedW ? NB : 1, sysMax, maxSlots);
    const int schurUnits = schurWaves * BA_SCHUR_LPW;
    int lmBlocks = std::max(1, std::min((lpMax + schurUnits - 1) / schurUnits, kn.lmBlocks ? kn.lmBlocks : std::max(16, 2 * nCU / NL)));
    // k_ba_schur2 (tracker windows): one LDS copy of the system + a staging region per landmark-wave
    const size_t s2StageB = (size_t)ba2_stage_doubles(maxFac, maxSlots) * sizeof(double);
    int s2Waves = std::max(2, std::min(16, kn.s2Waves));
    while (s2Waves > 2 && sysMax * sizeof(double) + s2Waves * s2StageB > 156 * 1024) s2Waves /= 2;
    const size_t s2Lds = sysMax * sizeof(double) + (size_t)s2Waves * s2StageB;
    const bool useSchur2 = kn.schur2 && fMax <= BA2_MAX_F && maxSlots <= BA2_MAX_F && s2Lds <= 156 * 1024;
    // (the kernel is a latency chain per landmark-wave: every workgroup of the cohort resident at once - one per CU at this LDS size -,
    //  each wave walks a few landmarks)
    if (useSchur2) lmBlocks = std::max(1, std::min((lpMax + 2 * s2Waves - 1) / (2 * s2Waves), kn.lmBlocks ? kn.lmBlocks : std::max(4, (16 / s2Waves) * nCU / NL)));
    // k_ba_back2 holds b2Waves staging regions and no system: that k_ba_schur2 fits does not make it fit (4 regions of a landmark with
    // ~120-200 stereo views exceed 160 KB where 2 regions + the system do not), so it halves its own waves until the launch fits
    int b2Waves = std::max(1, std::min(8, kn.b2Waves));
    while (b2Waves > 1 && (size_t)b2Waves * s2StageB > BA_DYN_LDS_MAX) b2Waves /= 2;
    const size_t b2Lds = (size_t)b2Waves * s2StageB;
    const bool useBack2 = useSchur2 && kn.back2 && b2Lds <= BA_DYN_LDS_MAX;
    const int backWaves = ba_back_waves(64, maxSlots);
    p.schur_kernel = useSchur2 ? VSLAM_BA_KERNEL_SCHUR2 : VSLAM_BA_KERNEL_SCHUR;
    p.schur_waves = useSchur2 ? s2Waves : schurWaves;
    p.schur_shared_w = useSchur2 ? 0 : sharedW;
    p.schur_blocks = lmBlocks;
    // (the rules above keep computing with the row-major size: the plans per shape stay; only the LDS asked for follows the layout)
    p.schur_lds = (int)(useSchur2 ? (size_t)ba2_sys_doubles(nMax, kn.s2Layout) * sizeof(double) + (size_t)s2Waves * s2StageB : schurLds);
    p.back_kernel = useBack2 ? VSLAM_BA_KERNEL_BACK2 : VSLAM_BA_KERNEL_BACK;
    if (useBack2) {
        p.back_waves = b2Waves; p.back_shared = 1; p.back_lds = (int)b2Lds;
        p.back_blocks = std::max(1, std::min((lpMax + 2 * b2Waves - 1) / (2 * b2Waves), std::max(8, (16 / b2Waves) * nCU / NL)));
    } else {
        p.back_waves = backWaves; p.back_shared = NB > 1 ? 1 : 0; p.back_lds = (int)ba_back_lds(backWaves, maxSlots);
        p.back_blocks = std::max(1, std::min((lpMax + backWaves * BA_BACK_LPW - 1) / (backWaves * BA_BACK_LPW), std::max(16, 2 * nCU / NL)));
    }
    p.solve_lds = (p.solve_kinds & (1 << BA_SOLVE_MFMA)) ? (int)ba_mfma_lds() : 0;
    if (p.schur_lds > BA_DYN_LDS_MAX || p.back_lds > BA_DYN_LDS_MAX || p.solve_lds > BA_DYN_LDS_MAX) p.status = VSLAM_ERR_CAPACITY;
}

}  // namespace vslam
