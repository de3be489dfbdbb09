// The lane packing of vslam_global_ba_batch (gtsam-vslam_amd/csrc/gba_pack_host.hpp) as a stand-alone program under
// AddressSanitizer + UBSan.  The lanes' shapes come in on the command line's file (written by tests/test_gba_pack_host.py), the
// table goes out as text; the Python side compares it with running sums of its own.
//   in:  nLanes (K L P M nf b nBlk nInc nLmPairs nList)*
//   out: "status <s> <message>", then for status 0: "sums ..." and one "lane ..." line per lane
#include "gba_pack_host.hpp"
#include <cstdio>
#include <cstdlib>

static int rd(FILE* f) { int v = 0; if (fscanf(f, "%d", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); } return v; }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    const int n = rd(f);
    std::vector<vslam::GbaLaneShape> s(n > 0 ? n : 0);
    for (auto& q : s) {
        q.K = rd(f); q.L = rd(f); q.P = rd(f); q.M = rd(f); q.nf = rd(f); q.b = rd(f); q.nBlk = rd(f); q.nInc = rd(f); q.nLmPairs = rd(f); q.nList = rd(f);
        q.hasUnknowns = q.nf > 0 || q.L > 0;
        q.fx = 400.0 + q.K; q.fy = 410.0; q.cx = 320.0; q.cy = 240.0; q.bl = 0.12;
    }
    fclose(f);
    std::vector<vslam::GbaLane> tab;
    vslam::GbaPackSums S;
    std::string err;
    const int st = vslam::gba_pack(s.data(), n, tab, S, &err);
    printf("status %d %s\n", st, err.c_str());
    if (st) return 0;
    printf("sums %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", S.K, S.L, S.P, S.M, S.nf, S.inc, S.lp, S.band, S.blk, S.list);
    for (int l = 0; l < n; l++) {
        const vslam::GbaLane& T = tab[l];
        printf("lane %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %.1f\n", T.K, T.L, T.P, T.M, T.nf, T.b, T.nBlk, T.hasUnknowns, T.kf0, T.lm0,
               T.pair0, T.edge0, T.free0, T.inc0, T.lp0, T.band0, T.blk0, T.list0, T.lane, T.fx);
    }
    return 0;
}
