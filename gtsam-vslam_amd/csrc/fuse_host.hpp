// The commit of vslam_system_fuse_loop (vslam_hip.h; restated by tests/fuse_ref.py): the bookkeeping that
// makes one map point of two - the observation merge, the keyframes' tables, the active set.  No HIP include and no session type: the
// functions are written against the MEMBERS they touch, so the session hands them its own containers and a stand-alone program
// (tests/native/fuse_host_asan.cpp) hands them plain vectors of small structs.
//   Points     indexable; an element has  kfm (a std::vector of {kf, l, r}; find(kf) -> position or -1), kdx, lastObsKF
//   Keyframes  indexable; an element has  lmpL, lmpR, unF, unFR (std::vector<int>)
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace vslam_fuse {

struct CommitCounts {
    int nFused = 0, nMoved = 0, nDropped = 0;
    std::vector<int> touched;          // keyframes whose tables changed, ascending, each once
    std::vector<int> refresh;          // keyframes whose covisibility weights changed: the touched ones and every keyframe that
                                       // observes a kept point (its weight towards the keyframes the point was moved into grew)
};

// pairs: (absorbed a, kept b) in ascending a, every point at most once.  Observations of a go to b where b's keyframe has none yet
// and are erased from the keyframe otherwise; a ends as an outlier without observations.
template <class Points, class Keyframes>
CommitCounts merge_observations(const std::vector<std::pair<int, int>>& pairs, Points& pts, Keyframes& kfs, std::vector<uint8_t>& outlier,
                                std::vector<uint8_t>& inFrame) {
    CommitCounts c;
    for (const auto& pr : pairs) {
        auto& a = pts[pr.first];
        auto& b = pts[pr.second];
        for (const auto& o : a.kfm) {
            auto& kf = kfs[o.kf];
            if (b.find(o.kf) < 0) {
                b.kfm.push_back(o);
                if (o.l >= 0) { kf.lmpL[o.l] = pr.second; kf.unF[o.l] = (int)b.kdx; }
                if (o.r >= 0) { kf.lmpR[o.r] = pr.second; kf.unFR[o.r] = (int)b.kdx; }
                c.nMoved++;
            } else {
                if (o.l >= 0) { kf.lmpL[o.l] = -1; kf.unF[o.l] = -1; }
                if (o.r >= 0) { kf.lmpR[o.r] = -1; kf.unFR[o.r] = -1; }
                c.nDropped++;
            }
            c.touched.push_back(o.kf);
        }
        a.kfm.clear();
        outlier[pr.first] = 1; inFrame[pr.first] = 0;
        b.lastObsKF = std::max(b.lastObsKF, a.lastObsKF);
        c.nFused++;
    }
    std::sort(c.touched.begin(), c.touched.end());
    c.touched.erase(std::unique(c.touched.begin(), c.touched.end()), c.touched.end());
    c.refresh = c.touched;
    for (const auto& pr : pairs) for (const auto& o : pts[pr.second].kfm) c.refresh.push_back(o.kf);
    std::sort(c.refresh.begin(), c.refresh.end());
    c.refresh.erase(std::unique(c.refresh.begin(), c.refresh.end()), c.refresh.end());
    return c;
}

// the active set: the old list without the absorbed points, order kept, then the kept points not yet in it in ascending index; every
// kept point is in the frame.  nPoints: the size of the map.
inline void merge_active(const std::vector<std::pair<int, int>>& pairs, size_t nPoints, std::vector<int>& active, std::vector<uint8_t>& inFrame) {
    std::vector<uint8_t> mark(nPoints, 0);     // 1: absorbed, 2: already active
    for (const auto& pr : pairs) mark[pr.first] = 1;
    size_t n = 0;
    for (int m : active) if (mark[m] != 1) { active[n++] = m; mark[m] = 2; }
    active.resize(n);
    std::vector<int> kept;
    for (const auto& pr : pairs) { kept.push_back(pr.second); inFrame[pr.second] = 1; }
    std::sort(kept.begin(), kept.end());
    for (int b : kept) if (mark[b] != 2) active.push_back(b);
}

}  // namespace vslam_fuse
