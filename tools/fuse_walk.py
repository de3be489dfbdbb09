"""What vslam_system_fuse_loop does on the out-and-back corridor walk of tests/test_gpu_loop.py, measured (nothing here is asserted).

Per stride (source frames between two frames of the walk; 40 frames out, 39 back, local_mapping = 1, 1 500 features):
  * close_loop(min_kf_gap = 2) at the return, then the inliers of the next three frames (source frames 1, 2, 3) WITHOUT a fuse;
  * the same run WITH fuse_loop between close_loop and the next frame, the split at the turn-round (min_kf_gap = latestKF -
    (kf_out - 1)): its report, the inliers of the next three frames, then up to 20 frames until a keyframe is inserted (never fewer than
    three frames) and the first new keyframe's covisibility entries as they stand then;
  * from the taps before the fuse: the pair count of the search at every split (min_kf_gap = 1 .. latestKF), and at the turn-round
    split the histograms of n_gated and of d1 over the proposals at radius 2 / 4 / 8 (vslam_fuse_search on the taps).
usage: python tools/fuse_walk.py [out.json] [strides, e.g. 1,2,3]      (default profiles/fuse_walk.json)"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("gtsam-vslam_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np
import torch  # noqa: F401  (one HIP runtime per process: before the library)
import synth
import vslam_capi as vc

RIG = synth.RIGS["euroc"]
N_OUT = 40
K = (RIG["fx"], RIG["fy"], RIG["cx"], RIG["cy"])
SIZE = (RIG["w"], RIG["h"])


def affine_inv(T):
    """m4_affine_inv of csrc/system.hpp, operation for operation: camPoseInv from the camera pose"""
    a, b, c, d, e, f, g, h, i = (float(T[r][q]) for r in range(3) for q in range(3))
    A = e * i - f * h; B = -(d * i - f * g); Cc = d * h - e * g
    det = a * A + b * B + c * Cc
    inv = [A / det, -(b * i - c * h) / det, (b * f - c * e) / det,
           B / det, (a * i - c * g) / det, -(a * f - c * d) / det,
           Cc / det, -(a * h - b * g) / det, (a * e - b * d) / det]
    R = np.eye(4)
    t = [float(T[0][3]), float(T[1][3]), float(T[2][3])]
    for q in range(3):
        for p in range(3):
            R[q, p] = inv[3 * q + p]
        R[q, 3] = -(inv[3 * q] * t[0] + inv[3 * q + 1] * t[1] + inv[3 * q + 2] * t[2])
    return R


def sets(s, split_kf):
    """(idA, idB): non-outlier map points created after / up to keyframe split_kf, creation order"""
    _, outl = s.map_points()
    _, creator = s.map_point_keyframes()
    live = outl == 0
    return np.nonzero(live & (creator > split_kf))[0], np.nonzero(live & (creator <= split_kf))[0]


def walk_to_return(L, R, poses):
    s = vc.System(RIG, 1500, T0=poses[0], local_mapping=1)
    reps = []
    for n, j in enumerate(list(range(N_OUT)) + list(range(N_OUT - 2, -1, -1))):
        T, rep = s.track(L[j], R[j], n)
        reps.append(rep)
    return s, reps


def one_stride(stride):
    Ls, Rs, poses, _ = synth.corridor_sequence("euroc", N_OUT, "cuda", frame_step=stride)
    L, R = Ls.cpu().numpy(), Rs.cpu().numpy()
    out = dict(stride=stride)
    for fuse in (False, True):
        s, reps = walk_to_return(L, R, poses)
        n = len(reps)
        kf_out = max(r["n_keyframes"] for r in reps[:N_OUT])
        cl = s.close_loop(min_kf_gap=2)
        latest = s.counts()["keyframes"] - 1
        r = dict(kf_out=kf_out, latest_kf=latest, min_inliers_walk=min(q["n_inliers"] for q in reps[1:]), close_loop_corrected=cl["corrected"],
                 kf_loop=cl["kf_loop"], active_after_close=cl["n_active_after"])
        if fuse and cl["corrected"]:
            xyz, _ = s.map_points()
            desc = s.map_point_descriptors()
            T_cw = affine_inv(cl["T_wc"])
            per_split = {}
            for gap in range(1, latest + 1):
                idA, idB = sets(s, latest - gap)
                m, b, c = vc.fuse_search(T_cw, K, SIZE, xyz[idA], desc[idA], xyz[idB], desc[idB])
                per_split[gap] = dict(n_a=len(idA), n_b=len(idB), **c)
            r["pairs_by_min_kf_gap"] = per_split
            gap = latest - (kf_out - 1)
            idA, idB = sets(s, kf_out - 1)
            hist = {}
            for rad in (2.0, 4.0, 8.0):
                m, b, c = vc.fuse_search(T_cw, K, SIZE, xyz[idA], desc[idA], xyz[idB], desc[idB], radius=rad)
                prop = (b[:, 3] > 0) & (b[:, 0] <= 50)
                hist[str(rad)] = dict(counts=c, n_gated_hist_over_a=np.bincount(np.minimum(b[:, 3], 16), minlength=17).tolist(),
                                      d1_hist_over_proposals_by_10=np.bincount(b[prop, 0] // 10, minlength=6).tolist(),
                                      d1_hist_over_gated_by_10=np.bincount(b[b[:, 3] > 0, 0] // 10, minlength=26).tolist())
            r["histograms_at_turn_round_split"] = hist
            f = s.fuse_loop(min_kf_gap=gap)
            r["fuse_min_kf_gap"] = gap
            r["fuse_report"] = f
        after = []
        new_kf = None
        for q in range(20):
            T, rep = s.track(L[1 + q], R[1 + q], n + q)
            after.append(rep["n_inliers"])
            if rep["keyframe_inserted"] and new_kf is None:
                new_kf = rep["n_keyframes"] - 1
            if new_kf is not None and q >= 2:               # (at least the three frames after the correction)
                break
        r["inliers_after"] = after
        if new_kf is not None:
            cov = s.covisibility()
            rows = cov[cov[:, 0] == new_kf]
            r["new_keyframe"] = new_kf
            r["new_keyframe_covisibility"] = rows[:, 1:].tolist()
            r["new_keyframe_sees_way_out"] = bool((rows[:, 1] < kf_out).any())
        s.close()
        out["with_fuse" if fuse else "without_fuse"] = r
        print(json.dumps({("with_fuse" if fuse else "without_fuse"): r, "stride": stride}), flush=True)
    return out


def main(argv):
    out_path = argv[0] if len(argv) > 0 else os.path.join(ROOT, "profiles", "fuse_walk.json")
    strides = [int(x) for x in argv[1].split(",")] if len(argv) > 1 else [1, 2, 3]
    res = dict(protocol="corridor walk, 40 frames out and 39 back, local_mapping 1, 1500 features; close_loop(min_kf_gap=2) at the return; "
                        "one run without and one with fuse_loop (defaults, split at the turn-round) per stride", strides=[])
    for st in strides:
        res["strides"].append(one_stride(st))
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
