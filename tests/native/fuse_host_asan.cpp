// The commit of vslam_system_fuse_loop (gtsam-vslam_amd/csrc/fuse_host.hpp) on plain vectors, as a stand-alone program under
// AddressSanitizer + UBSan.  The map comes in on the command line's file (written by tests/test_fuse_host.py from
// tests/fuse_cases.py), the merged map goes out as text; the Python side compares it with tests/fuse_ref.py.
//   in:  nPoints nKf nLeft nRight
//        per point: kdx lastObsKF outlier inFrame nObs (kf l r)*
//        nActive active*      nPairs (a b)*
//   out: "ok", then the same records after the merge, the keyframes' four tables, the counts
#include "fuse_host.hpp"
#include <cstdio>
#include <cstdlib>

struct Obs { int kf, l, r; };
struct Point {
    std::vector<Obs> kfm;
    long long kdx = 0;
    int lastObsKF = -1;
    int find(int kf) const { for (size_t i = 0; i < kfm.size(); i++) if (kfm[i].kf == kf) return (int)i; return -1; }
};
struct Keyframe { std::vector<int> lmpL, lmpR, unF, unFR; };

static int rd(FILE* f) { int v = 0; if (fscanf(f, "%d", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); } return v; }
static void row(const char* name, const std::vector<int>& v) { printf("%s", name); for (int x : v) printf(" %d", x); printf("\n"); }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    const int nP = rd(f), nK = rd(f), nL = rd(f), nR = rd(f);
    std::vector<Point> pts(nP);
    std::vector<uint8_t> outlier(nP), inFrame(nP);
    std::vector<Keyframe> kfs(nK);
    for (auto& k : kfs) { k.lmpL.assign(nL, -1); k.unF.assign(nL, -1); k.lmpR.assign(nR, -1); k.unFR.assign(nR, -1); }
    for (int m = 0; m < nP; m++) {
        pts[m].kdx = rd(f); pts[m].lastObsKF = rd(f); outlier[m] = (uint8_t)rd(f); inFrame[m] = (uint8_t)rd(f);
        const int n = rd(f);
        for (int q = 0; q < n; q++) {
            Obs o; o.kf = rd(f); o.l = rd(f); o.r = rd(f);
            pts[m].kfm.push_back(o);
            if (o.l >= 0) { kfs[o.kf].lmpL[o.l] = m; kfs[o.kf].unF[o.l] = (int)pts[m].kdx; }
            if (o.r >= 0) { kfs[o.kf].lmpR[o.r] = m; kfs[o.kf].unFR[o.r] = (int)pts[m].kdx; }
        }
    }
    std::vector<int> active(rd(f));
    for (int& a : active) a = rd(f);
    std::vector<std::pair<int, int>> pairs(rd(f));
    for (auto& p : pairs) { p.first = rd(f); p.second = rd(f); }
    fclose(f);

    const vslam_fuse::CommitCounts c = vslam_fuse::merge_observations(pairs, pts, kfs, outlier, inFrame);
    if (!pairs.empty()) vslam_fuse::merge_active(pairs, pts.size(), active, inFrame);

    printf("ok\n");
    for (int m = 0; m < nP; m++) {
        printf("point %d %d %d %d", m, pts[m].lastObsKF, (int)outlier[m], (int)inFrame[m]);
        for (const Obs& o : pts[m].kfm) printf(" %d %d %d", o.kf, o.l, o.r);
        printf("\n");
    }
    for (int k = 0; k < nK; k++) { row("lmpL", kfs[k].lmpL); row("lmpR", kfs[k].lmpR); row("unF", kfs[k].unF); row("unFR", kfs[k].unFR); }
    row("active", active);
    row("touched", c.touched);
    row("refresh", c.refresh);
    printf("counts %d %d %d\n", c.nFused, c.nMoved, c.nDropped);
    return 0;
}
