"""vslam_system_fuse_loop on the out-and-back corridor walk of tests/test_gpu_loop.py (its walk and run are imported): after the
loop correction at the return the map holds the landmarks of the corridor twice, and the call makes one map point of each pair.
The session's pairs are compared with the numpy restatement of the search (tests/fuse_ref.py) on the session's own taps, the map
after the call with the restatement's commit applied to the taps before it.

PAIRS_MEASURED: what the stride-1 walk yields at the turn-round split with the default parameters, measured on an MI355X with the
restatement (tools/fuse_walk.py -> profiles/fuse_walk.json); the test asserts at least half of it, and at least 10."""
import numpy as np
import pytest
import torch  # noqa: F401,E402  (one HIP runtime per process: before the library, as tests/test_gpu_loop.py explains)
import fuse_ref as fr
from test_gpu_loop import GAP, N_OUT, RIG, run, walk

pytestmark = pytest.mark.gpu

PAIRS_MEASURED = 101          # (7 keyframes out, 2 since the turn-round: 329 new points against 643 old ones, 113 proposals)
K = (RIG["fx"], RIG["fy"], RIG["cx"], RIG["cy"])
SIZE = (RIG["w"], RIG["h"])


def affine_inv(T):
    """the session's camPoseInv from its camera pose: m4_affine_inv of csrc/system.hpp, operation for operation (cofactors over the
    determinant, then -A^-1 t), so that the restatement projects with the very matrix the session hands to the search"""
    a, b, c, d, e, f, g, h, i = (float(T[r][q]) for r in range(3) for q in range(3))
    A = e * i - f * h; B = -(d * i - f * g); Cc = d * h - e * g
    det = a * A + b * B + c * Cc
    inv = [A / det, -(b * i - c * h) / det, (b * f - c * e) / det,
           B / det, (a * i - c * g) / det, -(a * f - c * d) / det,
           Cc / det, -(a * h - b * g) / det, (a * e - b * d) / det]
    t = [float(T[0][3]), float(T[1][3]), float(T[2][3])]
    R = np.eye(4)
    for q in range(3):
        for p in range(3):
            R[q, p] = inv[3 * q + p]
        R[q, 3] = -(inv[3 * q] * t[0] + inv[3 * q + 1] * t[1] + inv[3 * q + 2] * t[2])
    return R


def taps(s):
    """everything the taps show of the map, as plain containers"""
    xyz, outl = s.map_points()
    _, creator = s.map_point_keyframes()
    off, tr = s.map_point_observations()
    n_kf = s.counts()["keyframes"]
    rows = [tuple(r) for r in tr.tolist()]
    obs = [rows[off[m]:off[m + 1]] for m in range(len(xyz))]
    tables = []
    for k in range(n_kf):
        l, r = s.keyframe_points(k)
        tables.append(dict(lmpL=l.tolist(), lmpR=r.tolist(), unF=[-1] * len(l), unFR=[-1] * len(r)))       # (unF / unFR have no tap)
    return dict(xyz=xyz, outl=outl, creator=creator, desc=s.map_point_descriptors(), obs=obs, tables=tables, active=s.active_points().tolist(),
                cov=s.covisibility(), n_kf=n_kf)


def snapshot(s):
    """the taps as bytes: what a call that changes nothing must leave alone"""
    xyz, outl = s.map_points()
    first, creator = s.map_point_keyframes()
    off, tr = s.map_point_observations()
    kf_idx, kf_pose = s.keyframes()
    mt, ol = s.last_frame()
    tables = b"".join(a.tobytes() for k in range(len(kf_idx)) for a in s.keyframe_points(k))
    return (s.counts(), xyz.tobytes(), outl.tobytes(), first.tobytes(), creator.tobytes(), s.map_point_descriptors().tobytes(), off.tobytes(),
            tr.tobytes(), tables, s.active_points().tobytes(), s.covisibility().tobytes(), kf_idx.tobytes(), kf_pose.tobytes(), mt.tobytes(),
            ol.tobytes(), s.fused_pairs().tobytes())


def closed_session(capi):
    """the walk with local_mapping = 1 and the loop correction at the return, as test_close_loop_at_the_return; returns the session,
    the number of frames tracked, the keyframes of the way out, the fuse's min_kf_gap that puts the split at the turn-round, and the
    camera pose after the correction"""
    s, Ts, reps = run(capi, 1)
    kf_out = max(r["n_keyframes"] for r in reps[:N_OUT])
    rep = s.close_loop(min_kf_gap=GAP)
    assert rep["success"] == 1 and rep["corrected"] == 1
    latest = s.counts()["keyframes"] - 1
    return s, len(Ts), kf_out, latest - (kf_out - 1), rep["T_wc"]


def test_commit_against_the_restatement(capi):
    s, n, kf_out, gap, T_wc = closed_session(capi)
    before = taps(s)
    live = before["outl"] == 0
    idA = np.nonzero(live & (before["creator"] > kf_out - 1))[0]
    idB = np.nonzero(live & (before["creator"] <= kf_out - 1))[0]
    match, best, counts = fr.search(affine_inv(T_wc), K, SIZE, before["xyz"][idA], before["desc"][idA], before["xyz"][idB], before["desc"][idB])
    pairs = [(int(idA[j]), int(idB[match[j]])) for j in range(len(idA)) if match[j] >= 0]
    rep = s.fuse_loop(min_kf_gap=gap)
    print("fuse_loop:", rep, "| restatement:", counts, "| keyframes of the way out:", kf_out, "min_kf_gap", gap)
    # the session's pairs are the restatement's, index for index
    assert s.fused_pairs().tolist() == [list(p) for p in pairs]
    assert rep["busy"] == 0 and (rep["n_a"], rep["n_b"]) == (len(idA), len(idB)) and rep["search"] == counts
    assert len(pairs) >= max(10, PAIRS_MEASURED // 2)
    # the map after the call is the restatement's commit of the map before it
    kdx = before["creator"].tolist()
    w_obs, w_tab, w_outl, _, w_act, _, w_counts = fr.commit(pairs, before["obs"], before["tables"], kdx, before["outl"].tolist(),
                                                            [0] * len(kdx), before["active"], [0] * len(kdx))
    after = taps(s)
    assert after["obs"] == w_obs
    for k in range(before["n_kf"]):
        assert after["tables"][k]["lmpL"] == w_tab[k]["lmpL"] and after["tables"][k]["lmpR"] == w_tab[k]["lmpR"], k
    assert after["outl"].tolist() == w_outl
    assert after["active"] == w_act
    assert after["xyz"].tobytes() == before["xyz"].tobytes() and after["desc"].tobytes() == before["desc"].tobytes()
    assert after["creator"].tobytes() == before["creator"].tobytes() and after["n_kf"] == before["n_kf"]
    # every touched keyframe's covisibility list follows calcConnections' rule over the new observations; the others keep theirs
    # (recomputed: the touched keyframes and every keyframe that observes a kept point - fuse_ref.commit's `refresh`)
    touched, refresh = w_counts["touched"], w_counts["refresh"]
    assert len(touched) >= 1 and set(touched) <= set(refresh)
    for k in range(before["n_kf"]):
        got = [(int(w), int(o)) for kk, o, w in after["cov"] if kk == k]
        if k in refresh:
            assert got == fr.connections(k, w_tab, w_obs, before["n_kf"]), k
        else:
            assert got == [(int(w), int(o)) for kk, o, w in before["cov"] if kk == k], k
    print("touched keyframes:", touched, "| covisibility entries that tie a keyframe since the turn-round to one of the way out:",
          [(int(kk), int(o), int(w)) for kk, o, w in after["cov"] if kk >= kf_out and o < kf_out])
    assert (rep["n_fused"], rep["n_obs_moved"], rep["n_obs_dropped"], rep["n_keyframes_touched"], rep["n_active_after"]) == \
           (len(pairs), w_counts["n_obs_moved"], w_counts["n_obs_dropped"], len(touched), len(w_act))
    assert len(s.last_frame()[0]) == 0
    s.close()


def test_it_keeps_tracking(capi):
    """after the fuse the session tracks on past the return until a keyframe has been inserted (at most 20 frames): no lost frame.
    Measured: 277 - 418 inliers over the twenty frames (285 - 441 without the fuse), and no keyframe is inserted within them, so the
    covisibility line below is printed only if that changes; the covisibility entries between the keyframes since the turn-round
    and those of the way out, as they stand after the fuse, are printed by test_commit_against_the_restatement."""
    L, R, _ = walk()
    s, n, kf_out, gap, _ = closed_session(capi)
    rep = s.fuse_loop(min_kf_gap=gap)
    assert rep["n_fused"] >= 10
    for q in range(20):
        T, r = s.track(L[1 + q], R[1 + q], n + q)
        print("frame %d after the fuse: %d inliers%s" % (q, r["n_inliers"], ", keyframe" if r["keyframe_inserted"] else ""))
        assert r["n_inliers"] >= 50
        if r["keyframe_inserted"]:
            new = r["n_keyframes"] - 1
            rows = [(int(o), int(w)) for kk, o, w in s.covisibility() if kk == new]
            print("covisibility of keyframe %d (other, weight): %s; a keyframe of the way out among them: %s"
                  % (new, rows, any(o < kf_out for o, w in rows)))
            break
    s.close()


@pytest.mark.parametrize("searched", [False, True])
def test_it_leaves_alone_what_it_should(capi, searched):
    """local_mapping = 0, a call after every frame of the way out: nothing is fused, no tap changes, and the run equals a run without
    the calls, poses bitwise.
    searched = False: the default min_kf_gap = 20 leaves the old set empty, so the search is idle.
    searched = True: min_kf_gap = 1 puts every point the latest keyframe created against all older ones, so the kernels run on
    both sets, but with radius 1e-3 pixel and max_hamming 1 nothing can pair: two separately triangulated points do not project
    within a thousandth of a pixel of each other.  This is the path "the search ran and found nothing"."""
    prm = dict(min_kf_gap=1, radius=1e-3, max_hamming=1) if searched else {}
    reports = []

    def hook(s, n, j, T, rep):
        before = snapshot(s)
        f = s.fuse_loop(**prm)
        assert snapshot(s) == before, n
        reports.append(f)

    s, Tg, Rg = run(capi, 0, hook, upto=N_OUT)
    s.close()
    assert all(f["n_fused"] == 0 and f["busy"] == 0 for f in reports) and any(f["n_a"] > 0 for f in reports)
    if searched:
        assert any(f["n_a"] > 0 and f["n_b"] > 0 and f["search"]["n_visible_a"] > 0 and f["search"]["n_visible_b"] > 0 for f in reports)
    else:
        assert all(f["n_b"] == 0 for f in reports)
    plain, Tp, Rp = run(capi, 0, upto=N_OUT)
    plain.close()
    for n in range(N_OUT):
        assert Tg[n].tobytes() == Tp[n].tobytes(), n
        assert Rg[n] == Rp[n], n


def test_busy(capi):
    """local_mapping = 2: a call between the hand-over of a mapping pass and its landing reports busy and changes nothing"""
    reports = []

    def hook(s, n, j, T, rep):
        before = snapshot(s)
        f = s.fuse_loop()
        if f["busy"]:
            assert snapshot(s) == before, n
            assert f == dict(f, n_a=0, n_b=0, n_fused=0, n_active_after=0)
        reports.append(f)

    s, _, _ = run(capi, 2, hook, upto=N_OUT, mapping_delay=2)
    s.close()
    assert any(f["busy"] for f in reports) and not all(f["busy"] for f in reports)


def test_refusals(capi):
    L, R, truth = walk()
    s = capi.System(RIG, 1500, T0=truth[0], local_mapping=0)

    def refused(call):
        with pytest.raises(capi.VslamError) as ex:
            call()
        return ex.value.status == capi.ERR_INVALID

    assert refused(lambda: s.fuse_loop())                                  # no tracked frame yet
    s.track(L[0], R[0], 0)
    before = snapshot(s)
    for bad in (dict(min_kf_gap=-1), dict(radius=-1.0), dict(depth_ratio=-1.25), dict(max_hamming=-1), dict(depth_ratio=0.5),
                dict(radius=float("nan"))):
        assert refused(lambda: s.fuse_loop(**bad)), bad
    assert snapshot(s) == before
    rep = s.fuse_loop()                                                    # one keyframe: no old set
    assert rep["n_fused"] == 0 and rep["n_b"] == 0 and snapshot(s) == before
    s.close()
    imu = dict(gravity=(0.0, 9.81, 0.0), noise=(1.7e-4, 2e-5, 2e-3, 3e-3), T_bs=np.eye(4), hz=200)
    si = capi.System(RIG, 1500, T0=truth[0], imu=imu, local_mapping=0)
    si.track(L[0], R[0], 0)
    assert refused(lambda: si.fuse_loop())
    assert si.counts()["keyframes"] == 1
    si.close()
    sm = capi.MonoSystem(RIG, 1500, RIG["fps"], T0=truth[0], imu=imu)
    assert refused(lambda: sm.fuse_loop())
    sm.close()
