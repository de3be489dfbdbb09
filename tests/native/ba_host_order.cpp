// Host side of local BA (ba_order_host.hpp, ba_plan.hpp) against brute-force restatements, without a device: built with
// -fsanitize=address,undefined by tests/test_ba_host_order.py.  Prints "ok ..." and returns 0, or the first failed check.
#include "ba_order_host.hpp"
#include "ba_plan.hpp"
#include <cstdio>
#include <cstdlib>
#include <map>
#include <tuple>

using namespace vslam;

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s  [%s]\n", __FILE__, __LINE__, #c, g_case); return false; } } while (0)
static char g_case[256] = "";
static uint32_t g_seed = 12345;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }
static int rnd(int n) { return (int)(rnd() % (uint32_t)n); }

struct Prob {
    std::vector<float> sf, isf, uv; std::vector<double> pose, lm; std::vector<int64_t> id; std::vector<uint8_t> fixed, local, flags, wrong;
    std::vector<int32_t> pkf, plm, oct; std::vector<DPose> pose0;
    vslam_ba_problem P{};
};
// K keyframes (unsorted distinct ids; fixedMode 0 none / 1 some / 2 all), L landmarks each seen by a random set of keyframes, the pairs in
// random order with flags 0..3 (flagMode < 0) or all flagMode; random chi2 flags
static void make(Prob& q, int K, int L, int fixedMode, int flagMode, int wrongPct) {
    const int NL = 8;
    q = Prob{};
    for (int l = 0; l < NL; l++) { q.sf.push_back(1.f + 0.2f * l); q.isf.push_back(1.f / (1.f + 0.2f * l)); }
    q.pose0.resize(K);
    for (int k = 0; k < K; k++) {
        const double a = 0.1 * rnd(60), c = cos(a), s = sin(a);
        const double M[16] = {c, -s, 0, 0.5 * rnd(20), s, c, 0, 0.25 * rnd(20), 0, 0, 1, 0.125 * rnd(20), 0, 0, 0, 1};
        q.pose.insert(q.pose.end(), M, M + 16);
        pose_from_rm16(M, q.pose0[k]);
        q.id.push_back(1000 - 7 * k + (k % 3) * 40);       // distinct, not monotonic
        q.fixed.push_back(fixedMode == 2 ? 1 : fixedMode == 1 ? (uint8_t)(rnd(3) == 0) : 0);
        q.local.push_back(1);
    }
    for (int l = 0; l < 3 * L; l++) q.lm.push_back(0.01 * rnd(1000));
    std::vector<std::pair<int, int>> pr;
    for (int l = 0; l < L; l++) for (int k = 0; k < K; k++) if (rnd(3) != 0) pr.push_back({k, l});
    for (size_t i = pr.size(); i > 1; i--) std::swap(pr[i - 1], pr[rnd((int)i)]);
    for (auto& e : pr) {
        q.pkf.push_back(e.first); q.plm.push_back(e.second);
        q.flags.push_back((uint8_t)(flagMode < 0 ? rnd(4) : flagMode));
        q.wrong.push_back((uint8_t)(rnd(100) < wrongPct));
        for (int i = 0; i < 4; i++) q.uv.push_back(0.5f * rnd(1000));
        q.oct.push_back(rnd(NL)); q.oct.push_back(rnd(NL));
    }
    if (pr.empty()) q.wrong.push_back(0);
    vslam_ba_problem& P = q.P;
    P.n_levels = NL; P.sigma_factor = q.sf.data(); P.inv_sigma_factor = q.isf.data();
    P.n_kf = K; P.kf_pose_wc = q.pose.data(); P.kf_id = q.id.data(); P.kf_fixed = q.fixed.data(); P.kf_local = q.local.data();
    P.n_lm = L; P.lm_xyz = q.lm.data(); P.n_pairs = (int)pr.size();
    P.pair_kf = q.pkf.data(); P.pair_lm = q.plm.data(); P.pair_flags = q.flags.data(); P.pair_uv = q.uv.data(); P.pair_octave = q.oct.data();
}

// one pass of BaPassHost in an arena of exactly the stated size (malloc'ed: ASan sees an overrun), zero-filled so that runs compare bytewise
struct Pass {
    BaPassHost H; BaHostTmp T; BaArenaView A; std::vector<uint8_t> mem;
    bool run(const Prob& q, const uint8_t* wrong, int rank, int world, BaPool* pool, const BaHostTune& tune, int edgeSlots) {
        H = BaPassHost{}; H.tune = tune;
        H.count(&q.P, wrong, rank, world, T, pool);
        mem.assign(H.arena_bytes(q.P.n_kf, q.P.n_lm, edgeSlots), 0);
        A.h = mem.data(); A.cap = mem.size(); A.reset();
        CHECK(H.take(A, q.P.n_kf, q.P.n_lm, edgeSlots));
        CHECK(A.used <= A.cap && H.h_ctl && H.h_D && H.h_facKf && H.h_edges && H.h_kfPresent);
        H.fill(&q.P, wrong, rank, world, T, q.pose0.data(), pool, edgeSlots);
        return true;
    }
};
static const BaHostTune kSmallTune = {1, 8, 16, 16};      // pooled forms from 1 pair / 16 landmarks on

struct Fac { int l, fi, p, side; };
static bool check_order(const Prob& q, const uint8_t* wrong, int rank, int world, const Pass& S) {
    const vslam_ba_problem& P = q.P;
    const BaPassHost& H = S.H;
    const int K = P.n_kf, L = P.n_lm, NP = P.n_pairs;
    std::vector<uint8_t> kfP(K, 0), lmP(std::max(L, 1), 0);
    for (int p = 0; p < NP; p++) if (!wrong[p] && (P.pair_flags[p] & 3)) { kfP[P.pair_kf[p]] = 1; lmP[P.pair_lm[p]] = 1; }
    std::vector<int> fidx(K, -1), lpOf(L, -1), lpOrig;
    int F = 0;
    for (int k = 0; k < K; k++) if (kfP[k] && !P.kf_fixed[k]) fidx[k] = F++;
    for (int l = 0; l < L; l++) if (lmP[l] && l % world == rank) { lpOf[l] = (int)lpOrig.size(); lpOrig.push_back(l); }
    std::vector<Fac> f;
    for (int p = 0; p < NP; p++) for (int side = 0; side < 2; side++)
        if (!wrong[p] && ((P.pair_flags[p] >> side) & 1) && P.pair_lm[p] % world == rank) f.push_back({P.pair_lm[p], fidx[P.pair_kf[p]], p, side});
    std::stable_sort(f.begin(), f.end(), [](const Fac& a, const Fac& b) { return std::tie(a.l, a.fi, a.p, a.side) < std::tie(b.l, b.fi, b.p, b.side); });
    const int NF = (int)f.size(), Lp = (int)lpOrig.size();
    CHECK(H.NF == NF && H.Lp == Lp && H.F == F && H.n == 6 * F);
    for (int k = 0; k < K; k++) CHECK(H.h_fidx[k] == fidx[k] && H.h_kfPresent[k] == kfP[k]);
    for (int l = 0; l < L; l++) CHECK(H.h_lmPresent[l] == lmP[l]);
    int maxSlots = 1, maxFac = 1, se = 0, at = 0;
    long long k2 = 0;
    for (int lp = 0; lp < Lp; lp++) {
        CHECK(H.h_lpOrig[lp] == lpOrig[lp] && H.h_lpStart[lp] == at && H.h_lpSlotStart[lp] == se);
        int ns = 0, last = -2, nf = 0;
        for (; at < NF && f[at].l == lpOrig[lp]; at++, nf++) {
            const Fac& e = f[at];
            if (e.fi >= 0 && e.fi != last) { CHECK(H.h_slotStart[se] == at && H.h_slotFi[se] == e.fi); se++; ns++; last = e.fi; }
            CHECK(H.h_facKf[at] == P.pair_kf[e.p] && H.h_facFi[at] == e.fi && H.h_facLp[at] == lp && H.h_facLm[at] == e.l && H.h_facPair[at] == e.p);
            CHECK(H.h_facRight[at] == e.side && H.h_facZ[2 * at] == P.pair_uv[4 * e.p + 2 * e.side] && H.h_facZ[2 * at + 1] == P.pair_uv[4 * e.p + 2 * e.side + 1]);
            CHECK(H.h_facIs[at] == 1.0 / (1.0 / (double)P.inv_sigma_factor[P.pair_octave[2 * e.p + e.side]]));
        }
        CHECK(nf > 0 && H.h_slotStart[se] == at && H.h_slotFi[se] == -1);      // end sentinel
        se++;
        maxSlots = std::max(maxSlots, ns); maxFac = std::max(maxFac, nf); k2 += (long long)ns * ns;
    }
    CHECK(at == NF && H.h_lpStart[Lp] == NF && H.h_lpSlotStart[Lp] == se);
    CHECK(H.maxSlots == maxSlots && H.maxFac == maxFac && H.nSlotEntries == se && H.sumK2 == k2);
    // edges: id-consecutive present keyframes, measured = inverse(a) b, counted on rank 0 only
    std::vector<int> ord;
    for (int k = 0; k < K; k++) if (kfP[k]) ord.push_back(k);
    std::sort(ord.begin(), ord.end(), [&](int a, int b) { return P.kf_id[a] < P.kf_id[b]; });
    const int NE = rank == 0 ? std::max((int)ord.size() - 1, 0) : 0;
    CHECK(H.NE == NE);
    return true;
}
static bool check_edges(const Prob& q, const Pass& S, int edgeSlots) {
    const BaPassHost& H = S.H;
    for (int sl = 0; sl < edgeSlots; sl++) for (int i = 0; i < H.NE; i++) {
        const BaEdge& e = H.h_edges[(size_t)sl * H.NE + i];
        CHECK(e.a == S.T.order[i] && e.b == S.T.order[i + 1] && q.P.kf_id[e.a] < q.P.kf_id[e.b] && e.fa == H.h_fidx[e.a] && e.fb == H.h_fidx[e.b]);
        DPose ai, m;
        pose_inverse(q.pose0[e.a], ai); pose_compose(ai, q.pose0[e.b], m);
        CHECK(!memcmp(&m, &e.measured, sizeof(DPose)));
    }
    return true;
}
static bool check_second(const Prob& q, const Pass& S, const std::vector<uint8_t>& w2, int rank, int world, BaPool* pool) {
    const vslam_ba_problem& P = q.P;
    const int K = P.n_kf, L = P.n_lm, NP = P.n_pairs;
    BaSecondPass a, b;
    S.H.second_pass(&P, w2.data(), rank, world, S.T, nullptr, a);
    BaPassHost Hp = S.H; Hp.tune = kSmallTune;
    Hp.second_pass(&P, w2.data(), rank, world, S.T, pool, b);
    CHECK(a.NF2 == b.NF2 && a.Lp2 == b.Lp2 && a.k2 == b.k2 && a.same == b.same && a.kfP2 == b.kfP2 && a.lmP2 == b.lmP2);
    std::vector<uint8_t> kfP(K, 0), lmP(std::max(L, 1), 0);
    long long nf = 0, lp2 = 0, k2 = 0;
    std::map<int, std::vector<int>> seen;      // landmark -> free indices of its unmasked factors
    for (int p = 0; p < NP; p++) {
        const int fl = P.pair_flags[p] & 3, l = P.pair_lm[p];
        if (w2[p] || !fl) continue;
        kfP[P.pair_kf[p]] = 1; lmP[l] = 1;
        if (l % world != rank) continue;
        nf += (fl & 1) + (fl >> 1);
        if (S.H.h_fidx[P.pair_kf[p]] >= 0) seen[l].push_back(S.H.h_fidx[P.pair_kf[p]]);
    }
    CHECK(a.NF2 == nf && a.kfP2 == kfP && a.lmP2 == lmP && a.same == (kfP == S.T.kfPresent));
    if (!a.same) return true;
    for (int l = 0; l < L; l++) if (l % world == rank) lp2 += lmP[l];
    for (auto& e : seen) { std::sort(e.second.begin(), e.second.end()); const long long ns = std::unique(e.second.begin(), e.second.end()) - e.second.begin(); k2 += ns * ns; }
    CHECK(a.Lp2 == lp2 && a.k2 == k2);
    return true;
}

static bool test_problems(BaPool& pool) {
    int nSame = 0, nDiff = 0;
    for (int K : {1, 2, 3, 12}) for (int L : {0, 1, 5, 300}) for (int fixedMode = 0; fixedMode < 3; fixedMode++) for (int rw = 0; rw < 3; rw++) {
        const int rank = rw == 2 ? 1 : 0, world = rw == 0 ? 1 : 2;
        Prob q;
        make(q, K, L, fixedMode, -1, (K + L + rw) % 2 ? 10 : 0);
        snprintf(g_case, sizeof g_case, "K %d L %d fixed %d rank %d/%d NP %d", K, L, fixedMode, rank, world, q.P.n_pairs);
        vslam_ba_result R{};
        std::vector<double> rp(16 * K), rl(3 * L + 1); std::vector<uint8_t> rw2(q.P.n_pairs + 1);
        R.kf_pose_wc = rp.data(); R.lm_xyz = rl.data(); R.pair_wrong = rw2.data();
        CHECK(ba_check_problem(&q.P, &R) == BA_PROBLEM_OK && ba_check_problem(&q.P, &R, &pool) == BA_PROBLEM_OK);
        for (int es : {1, 5}) {
            Pass s, p;
            if (!s.run(q, q.wrong.data(), rank, world, nullptr, BaHostTune{}, es)) return false;
            if (!p.run(q, q.wrong.data(), rank, world, &pool, kSmallTune, es)) return false;
            if (!check_order(q, q.wrong.data(), rank, world, s) || !check_edges(q, s, es)) return false;
            // pooled against serial: identical bytes
            CHECK(s.A.used == p.A.used && !memcmp(s.mem.data(), p.mem.data(), s.A.used));
            CHECK(s.H.NF == p.H.NF && s.H.Lp == p.H.Lp && s.H.F == p.H.F && s.H.NE == p.H.NE && s.H.maxSlots == p.H.maxSlots && s.H.maxFac == p.H.maxFac &&
                  s.H.nSlotEntries == p.H.nSlotEntries && s.H.sumK2 == p.H.sumK2);
            if (es != 1) continue;
            for (int flip : {3, 30}) {      // second graph: more flags set
                std::vector<uint8_t> w2 = q.wrong;
                for (auto& w : w2) if (rnd(100) < flip) w = 1;
                if (!check_second(q, s, w2, rank, world, &pool)) return false;
                BaSecondPass t; s.H.second_pass(&q.P, w2.data(), rank, world, s.T, nullptr, t); (t.same ? nSame : nDiff)++;
            }
        }
        if (q.P.n_pairs > 0) {      // a pair index out of range is named, serial and pooled
            q.plm[rnd(q.P.n_pairs)] = L;
            CHECK(ba_check_problem(&q.P, &R) == BA_PROBLEM_PAIR_RANGE && ba_check_problem(&q.P, &R, &pool) == BA_PROBLEM_PAIR_RANGE);
        }
        q.P.kf_id = nullptr;
        CHECK(ba_check_problem(&q.P, &R) == BA_PROBLEM_INVALID && ba_check_problem(nullptr, &R) == BA_PROBLEM_INVALID);
    }
    CHECK(nSame > 10 && nDiff > 10);
    // crafted second graphs: every keyframe sees every landmark with both sides
    Prob q;
    g_seed = 99;
    do make(q, 3, 5, 0, 3, 0); while (q.P.n_pairs < 12);
    snprintf(g_case, sizeof g_case, "crafted second pass");
    Pass s;
    if (!s.run(q, q.wrong.data(), 0, 1, nullptr, BaHostTune{}, 1)) return false;
    int lmDrop = -1;      // a landmark whose keyframes all see another landmark too
    for (int l = 0; l < 5 && lmDrop < 0; l++) {
        bool ok = s.T.lmPresent[l] != 0;
        for (int k = 0; k < 3 && ok; k++) {
            int others = 0, mine = 0;
            for (int p = 0; p < q.P.n_pairs; p++) if (q.pkf[p] == k) (q.plm[p] == l ? mine : others)++;
            ok = !mine || others;
        }
        if (ok) lmDrop = l;
    }
    CHECK(lmDrop >= 0);
    std::vector<uint8_t> w2 = q.wrong;
    for (int p = 0; p < q.P.n_pairs; p++) if (q.plm[p] == lmDrop) w2[p] = 1;
    BaSecondPass t;
    s.H.second_pass(&q.P, w2.data(), 0, 1, s.T, nullptr, t);
    CHECK(t.same && t.Lp2 == s.H.Lp - 1 && t.NF2 < s.H.NF && t.k2 < s.H.sumK2);      // only a landmark drops out
    if (!check_second(q, s, w2, 0, 1, &pool)) return false;
    w2 = q.wrong;
    for (int p = 0; p < q.P.n_pairs; p++) if (q.pkf[p] == q.pkf[0]) w2[p] = 1;
    s.H.second_pass(&q.P, w2.data(), 0, 1, s.T, nullptr, t);
    CHECK(!t.same);                                                                   // a keyframe loses all its pairs
    if (!check_second(q, s, w2, 0, 1, &pool)) return false;
    // report / result write-out
    double ctl[CTL_DOUBLES] = {0};
    ctl[CTL_LAMBDA] = 0.5; ctl[CTL_ERROR] = 2.5; ctl[CTL_INIT_ERR] = 7.5;
    int* ci = (int*)(ctl + CTL_INTS); ci[CI_ITER] = 4; ci[CI_INNER] = 6; ci[CI_ROUNDS] = 3;
    vslam_ba_result R{};
    ba_write_report(&R, 0, ctl, 2, 11, 12, 13); ba_write_report(&R, 1, ctl, 2, 21, 22, 23);
    CHECK(R.report[0].iterations == 4 && R.report[1].inner_iterations == 6 && R.report[1].initial_error == 7.5 && R.report[0].final_error == 2.5 && R.report[1].lambda == 0.5);
    CHECK(R.n_residuals == 21 && R.n_landmarks == 22 && R.sum_k2 == 23 && R.n_free_kf == 2 && R.rounds == 6);
    std::vector<double> rp(16 * 3), rl(15); std::vector<uint8_t> rwr(q.P.n_pairs);
    R.kf_pose_wc = rp.data(); R.lm_xyz = rl.data(); R.pair_wrong = rwr.data();
    ba_write_result(&R, q.pose0.data(), q.lm.data(), w2.data(), 3, 5, q.P.n_pairs);
    for (int i = 0; i < 48; i++) CHECK(rp[i] == q.pose[i]);
    CHECK(!memcmp(rl.data(), q.lm.data(), 15 * 8) && !memcmp(rwr.data(), w2.data(), q.P.n_pairs));
    return true;
}

static bool test_windows(BaPool& pool) {
    for (int F : {21, 65, 170}) for (int TB : {1, 4, 8}) {
        snprintf(g_case, sizeof g_case, "windows F %d TB %d", F, TB);
        // slot tables: landmark 0 is seen by every free keyframe (nBR rows: 65 and more with TB = 1), the others by a few
        const int Lp = 700, nCU = 4;
        std::vector<int> lpSlotStart, slotFi;
        for (int lp = 0; lp < Lp; lp++) {
            lpSlotStart.push_back((int)slotFi.size());
            const int step = lp == 0 ? 1 : 1 + rnd(F);
            for (int fi = lp == 0 ? 0 : rnd(step); fi < F; fi += step) slotFi.push_back(fi);
            slotFi.push_back(-1);
        }
        lpSlotStart.push_back((int)slotFi.size());
        const int nBR = (F + TB - 1) / TB, nWin = nBR * (nBR + 1) / 2;
        const BaWinLists a = ba_window_lists_host(Lp, lpSlotStart.data(), slotFi.data(), TB, nBR, nullptr, nCU);
        const BaWinLists b = ba_window_lists_host(Lp, lpSlotStart.data(), slotFi.data(), TB, nBR, &pool, nCU, nullptr, kSmallTune);
        CHECK(a.pack == b.pack && a.oWg == b.oWg && a.nInts == b.nInts && a.nWinWg == b.nWinWg && a.total == b.total);
        std::vector<std::vector<int>> want(nWin);      // every (landmark, row pair i <= j) once, in its window's list, in landmark order
        std::vector<int> winOf((size_t)nBR * nBR, -1);
        for (int r = 0, w = 0; r < nBR; r++) for (int c = r; c < nBR; c++, w++) { winOf[(size_t)r * nBR + c] = w; CHECK(a.pack[w] == r && a.pack[nWin + w] == c); }
        for (int lp = 0; lp < Lp; lp++) {
            std::vector<int> rows;
            for (int se = lpSlotStart[lp]; se < lpSlotStart[lp + 1] - 1; se++) if (rows.empty() || rows.back() != slotFi[se] / TB) rows.push_back(slotFi[se] / TB);
            for (size_t i = 0; i < rows.size(); i++) for (size_t j = i; j < rows.size(); j++) want[winOf[(size_t)rows[i] * nBR + rows[j]]].push_back(lp);
        }
        const int nWg = a.nWinWg, wgs = std::max(nWg, 1);
        const int *winFirst = a.pack.data() + 2 * nWin, *wgWin = a.pack.data() + a.oWg, *wgBegin = wgWin + wgs, *wgEnd = wgBegin + wgs, *winLm = wgEnd + wgs;
        CHECK(a.oWg == (size_t)3 * nWin + 1 && a.nInts == a.oWg + 3 * (size_t)wgs + std::max(a.total, 1) && a.pack.size() == a.nInts);
        const int chunk = std::max(256, (a.total + 2 * nCU - 1) / (2 * nCU));
        int at = 0, wg = 0;
        std::vector<int> winCnt;
        for (int w = 0; w < nWin; w++) {      // the cuts tile each list without gap or overlap
            winCnt.push_back(at);
            CHECK(winFirst[w] == wg);
            for (size_t i = 0; i < want[w].size(); i++) CHECK(winLm[at + i] == want[w][i]);
            for (const int end = at + (int)want[w].size(); at < end; wg++) {
                CHECK(wg < nWg && wgWin[wg] == w && wgBegin[wg] == at && wgEnd[wg] == std::min(at + chunk, end));
                at = wgEnd[wg];
            }
        }
        winCnt.push_back(at);
        CHECK(at == a.total && wg == nWg && winFirst[nWin] == nWg);
        // device-supplied list starts: the same cuts, room for the lists but no lists
        const BaWinLists d = ba_window_lists_host(Lp, lpSlotStart.data(), slotFi.data(), TB, nBR, &pool, nCU, winCnt.data());
        CHECK(d.nInts == a.nInts && d.oWg == a.oWg && d.nWinWg == nWg && d.total == a.total && d.pack.size() == a.oWg + 3 * (size_t)wgs);
        CHECK(!memcmp(d.pack.data(), a.pack.data(), d.pack.size() * sizeof(int)));
    }
    snprintf(g_case, sizeof g_case, "window tiles");
    for (int F = 21; F <= BA_MAX_FREE_KF; F++) for (int NB = 1; NB <= 4; NB++) for (int tb : {0, 1, 2, 4, 8, 32}) for (int dev = 0; dev < 2; dev++) {
        const BaWinTile w = ba_window_tile(F, NB, dev != 0, tb);
        if (w.why) { CHECK(w.lds > (size_t)BA_LDS_BYTES || (dev && w.nBR > 64)); continue; }
        CHECK(w.TB >= 1 && w.nBR == (F + w.TB - 1) / w.TB && w.lds <= (size_t)BA_LDS_BYTES && (!dev || w.nBR <= 64) && (tb == 0 || dev || w.TB == tb));
        CHECK(w.T == 6 * w.TB && w.TP == w.T + 1 && w.tileDoubles == w.T * w.TP + w.T && w.nWin == w.nBR * (w.nBR + 1) / 2);
    }
    // 65 block rows of 8 keyframes: refused by the free-keyframe rule, nothing is sized
    BaSingleKnobs kn; kn.windowTB = 8;
    CHECK(ba_single_plan(BaSingleShape{1000, 100, 65 * 8, 0, 8, 4, true, false}, kn).why != nullptr);
    CHECK(ba_single_plan(BaSingleShape{1000, 100, BA_MAX_FREE_KF + 1, 0, 8, 4, true, true}, BaSingleKnobs{}).why != nullptr);
    CHECK(ba_single_plan(BaSingleShape{1000, 100, BA_MAX_FREE_KF, 0, 8, 4, true, true}, BaSingleKnobs{}).why == nullptr);
    return true;
}

static bool in(int v, std::initializer_list<int> s) { return std::find(s.begin(), s.end(), v) != s.end(); }
static bool test_plans() {
    const size_t cap = BA_LDS_BYTES;
    for (int F = 1; F <= BA_MAX_FREE_KF; F++) for (int ms = 1; ms <= std::min(F, 40); ms++) for (int NB = 1; NB <= 4; NB++) for (int mf = 0; mf < 2; mf++) {
        snprintf(g_case, sizeof g_case, "plan F %d maxSlots %d NB %d mfma %d", F, ms, NB, mf);
        const int n = 6 * F, Lp = 37 * F + ms;
        const BaSinglePlan p = ba_single_plan(BaSingleShape{13 * Lp, Lp, F, F, ms, NB, mf != 0, false}, BaSingleKnobs{});
        if (p.why) continue;      // (the capacity error ba_run raises)
        CHECK(p.schurLds <= cap && p.backLds <= cap && p.mfmaLds <= cap && p.cholColLds <= cap && p.cholBackLds <= cap && (!p.solveLds || p.solveLdsBytes <= cap));
        CHECK((size_t)BA_SCHUR_WAVES * ms * sizeof(int) <= cap);      // k_ba_lm_prep
        CHECK(p.ldsS == (F <= BA_LDS_MAX_F) && (p.ldsS ? in(p.schurWaves, {16, 12, 8, 6, 4, 2}) && (p.sharedW || in(p.schurWaves, {16, 8, 4, 2})) : p.schurWaves == BA_SCHUR_WAVES));
        CHECK(in(p.backWaves, {8, 4, 2, 1}) && p.sharedBack == (NB > 1) && (!p.sharedW || NB > 1));
        CHECK(p.lmBlocks >= 1 && p.lmBlocks <= BA_NCU && p.backBlocks >= 1 && p.backBlocks <= BA_NCU && p.obsBlocks >= 1 && p.obsBlocks <= 4 * BA_NCU);
        CHECK(p.lmBlocks * p.schurWaves * BA_SCHUR_LPW >= std::min(Lp, BA_NCU * p.schurWaves) && p.backBlocks * p.backWaves * BA_BACK_LPW >= std::min(Lp, BA_NCU * p.backWaves * BA_BACK_LPW));
        CHECK(p.ldA % 32 == 1 && p.ldA >= n && p.cholN % CH_B == 0 && p.cholN >= n && p.useChol == (mf && n > BA_MFMA_N));
        CHECK(p.solveKind == ba_solve_kind(n, mf != 0) && (p.solveKind != BA_SOLVE_LARGE || n > (mf ? BA_MFMA_N : BA_WAVE_N)));
        vslam_ba_lane_shape s{};
        s.n_free_kf = F; s.n_points = Lp; s.n_factors = 13 * Lp; s.n_pairs = 10 * Lp; s.max_slots = ms; s.max_factors = 2 * ms;
        if (!ba_batch_single(s, mf != 0))       // the batch's former three-kind table
            CHECK(p.solveKind == ((n <= 64 && mf) ? BA_SOLVE_MFMA64 : n <= BA_WAVE_N ? BA_SOLVE_WAVE : BA_SOLVE_MFMA));
    }
    return true;
}

int main() {
    BaPool pool;
    pool.start(3);
    if (!test_problems(pool) || !test_windows(pool) || !test_plans()) return 1;
    printf("ok: ordering, pooled = serial, edges, arena, second pass, window lists, plans\n");
    return 0;
}
