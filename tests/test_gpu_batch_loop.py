"""Loop closing of vslam_batch lanes (vslam_batch_close_loop / vslam_batch_correct_loop) on the corridor walk of
tests/test_gpu_loop.py (its rendering, helpers and bounds are imported): three lanes on the same rig -
  lane 0 walks out 40 frames and back;
  lane 1 walks out 32 frames and back, and is masked out of tracking once it has returned (fewer keyframes, a smaller graph);
  lane 2 walks out 40 frames and stops there: masked out of tracking afterwards, kept in the loop mask - nothing to close.
A masked lane must get what the single-session calls give a session, whatever the other lanes do; lanes outside the mask must
not be touched at all.  The corrections are checked against the numpy restatement of the pose-graph solve (tests/pgo_ref.py) on
graphs rebuilt here from the lanes' taps and the documented edge rules, and lane 0 against a session driven alone."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch  # noqa: F401,E402   (one HIP runtime per process: before libvslam_hip.so, as tests/test_gpu_loop.py explains)
import pgo_ref as pr
import test_gpu_loop as tl

pytestmark = pytest.mark.gpu

RIG = tl.RIG
GAP = tl.GAP
N_OUT = [40, 32, 40]
SCHEDS = [list(range(40)) + list(range(38, -1, -1)), list(range(32)) + list(range(30, -1, -1)), list(range(40))]
STEPS = len(SCHEDS[0])
SENTINEL = 0xA5
INT_FIELDS = ("kf_loop", "n_candidates", "n_nodes", "n_sequential", "n_covisibility", "n_edges", "points_moved", "n_active_after")
PGO_INT_FIELDS = ("accepted", "rejected", "n_free", "half_bandwidth")


def drive(capi, local_mapping=0, hook=None, scheds=SCHEDS, **kw):
    """tracks the three walks in lockstep (a lane is masked out once its schedule has ended); hook(batch, n, mask, T, reports)
    after every step.  Returns (batch, poses per step, reports per step)."""
    L, R, poses = tl.walk()
    bt = capi.Batch(RIG, 1500, 3, T0s=[poses[s[0]] for s in scheds], local_mapping=local_mapping, **kw)
    Ts, reps = [], []
    for n in range(max(len(s) for s in scheds)):
        mask = [n < len(s) for s in scheds]
        lefts = [L[s[n]] if m else None for s, m in zip(scheds, mask)]
        rights = [R[s[n]] if m else None for s, m in zip(scheds, mask)]
        T, rep = bt.track(lefts, rights, [n] * 3, mask=mask)
        Ts.append(T.copy()); reps.append(rep)
        if hook:
            hook(bt, n, mask, T, rep)
    return bt, Ts, reps


def snapshots(bt):
    return [tl.snapshot(bt.system(b)) for b in range(3)]


@functools.lru_cache(maxsize=None)
def plain_run():
    """the batch at the end of the walks without any loop call: (batch, poses, reports); only test (b) changes the batch"""
    import vslam_capi
    return drive(vslam_capi)


def raw_loop_call(capi, bt, mask, kf_loops=None, poses=None, **params):
    """the C call on report entries pre-filled with sentinel bytes: (status, [report dict, or None where the entry still holds them])"""
    reps = (capi.LoopReport * 3)()
    C.memset(reps, SENTINEL, C.sizeof(reps))
    mk = np.ascontiguousarray(mask, np.uint8)
    prm = capi.System._loop_params(params)
    if kf_loops is None:
        st = capi.lib().vslam_batch_close_loop(bt.h_b, mk.ctypes.data_as(C.c_void_p), C.byref(prm), reps)
    else:
        kf = np.ascontiguousarray(kf_loops, np.int32); T = np.ascontiguousarray(poses, np.float64)
        st = capi.lib().vslam_batch_correct_loop(bt.h_b, mk.ctypes.data_as(C.c_void_p), kf.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p),
                                                 C.byref(prm), reps)
    blank = bytes([SENTINEL]) * C.sizeof(capi.LoopReport)
    return st, [None if bytes(reps[b]) == blank else capi._loop_report_dict(reps[b]) for b in range(3)]


def taps(s):
    fidx, P = s.keyframes()
    X, outl = s.map_points()
    first_obs, _ = s.map_point_keyframes()
    return dict(fidx=fidx, P=P, X=X, outl=outl, first_obs=first_obs, cov=s.covisibility())


def check_correction(s, before, rep, T_cam, kf_loop, T_corr, name):
    """a lane's correction against the documented rules: the graph rebuilt from the taps taken before the call, solved by the
    restatement; fixed keyframes bit for bit; map points with their first observing keyframe; the active set"""
    P_old, cov = before["P"], before["cov"]
    K = len(P_old)
    latest = K - 1
    edges = [(k - 1, k, pr.rigid_inv(P_old[k - 1]) @ P_old[k], 1.0, 1.0) for k in range(1, K)]
    seen = set()
    for k, o, w in cov:
        a, b = min(k, o), max(k, o)
        if w >= 100 and k != o and (a, b) not in seen:
            seen.add((a, b))
            edges.append((a, b, pr.rigid_inv(P_old[a]) @ P_old[b], 1.0, 1.0))
    D = T_corr @ np.linalg.inv(T_cam)
    edges.append((kf_loop, latest, pr.rigid_inv(P_old[kf_loop]) @ D @ P_old[latest], 10.0, 10.0))
    assert rep["busy"] == 0 and rep["success"] == 1 and rep["corrected"] == 1 and rep["kf_loop"] == kf_loop
    assert (rep["n_nodes"], rep["n_sequential"], rep["n_covisibility"], rep["n_edges"]) == (K, K - 1, len(seen), len(edges))
    fixed = np.zeros(K, np.uint8); fixed[[0, kf_loop]] = 1
    want, wrep = pr.optimize(P_old, fixed, edges)
    _, P_new = s.keyframes()
    print(name, "pgo", rep["pgo"], "ref", wrep, "max diff", np.abs(P_new - want).max(), "drift", rep["drift_translation"], rep["drift_rotation"])
    assert np.abs(P_new - want).max() <= 1e-7
    assert (rep["pgo"]["accepted"], rep["pgo"]["rejected"]) == (wrep["accepted"], wrep["rejected"])
    assert P_new[0].tobytes() == P_old[0].tobytes() and P_new[kf_loop].tobytes() == P_old[kf_loop].tobytes()
    X_new, outl_new = s.map_points()
    assert np.array_equal(before["outl"], outl_new)
    X_want = pr.move_points(before["X"], before["first_obs"], P_old, P_new)
    assert np.abs(X_new - X_want).max() <= 1e-9 and rep["points_moved"] == int((before["first_obs"] >= 0).sum())
    T_now = P_new[latest] @ np.linalg.inv(P_old[latest]) @ T_cam         # the camera follows the latest keyframe
    assert np.abs(rep["T_wc"] - T_now).max() <= 1e-9
    inside, unsure = tl.in_frame(rep["T_wc"], X_new)
    act = s.active_points()
    assert np.all(np.diff(act) > 0) and rep["n_active_after"] == len(act)
    got = np.zeros(len(X_new), bool); got[act] = True
    wanted = inside & (outl_new == 0)
    assert np.array_equal(got[~unsure], wanted[~unsure]) and not got[outl_new != 0].any()
    assert len(s.last_frame()[0]) == 0
    return P_new


def test_detection_leaves_every_lane_alone(capi):
    """(a): close_loop with detect_only on all lanes after EVERY step.  No call changes anything the taps show of any lane
    (bitwise); no lane reports a loop on its way out; lanes 0 and 1 find one at their return, against a keyframe of their way
    out, at a pose within the single-session test's bound of the ground truth; lane 2, standing at the far end, never does; and
    the whole run tracks frame for frame as a run without the calls - poses bitwise, reports equal."""
    log = []

    def hook(bt, n, mask, T, rep):
        before = snapshots(bt)
        d = bt.close_loop(detect_only=1, min_kf_gap=GAP)
        assert snapshots(bt) == before, n
        for b in range(3):
            assert d[b]["corrected"] == 0 and d[b]["busy"] == 0
            if mask[b]:
                assert d[b]["T_wc"].tobytes() == T[b].tobytes()
        log.append((n, d, [before[b][0]["keyframes"] for b in range(3)]))

    bt, Tg, Rg = drive(capi, 0, hook)
    bt.close()
    _, Tp, Rp = plain_run()
    for n in range(STEPS):
        for b in range(3):
            if n < len(SCHEDS[b]):
                assert Tg[n][b].tobytes() == Tp[n][b].tobytes(), (n, b)
                assert Rg[n][b] == Rp[n][b], (n, b)
    _, _, truth = tl.walk()
    for n, d, kfs in log:
        print(n, [(x["success"], x["n_candidates"], x["kf_loop"], x["reloc"]["n_inliers"]) for x in d], kfs)
        for b in range(3):
            if n < N_OUT[b]:
                assert d[b]["success"] == 0, (n, b)        # nothing to close on the way out
        assert d[2]["success"] == 0                        # lane 2 never comes back
    for b in (0, 1):
        n_end = len(SCHEDS[b]) - 1
        kf_out = log[N_OUT[b] - 1][2][b]
        d = log[n_end][1][b]
        assert kf_out >= 5 and d["success"] == 1 and 0 <= d["kf_loop"] < kf_out, (b, kf_out, d["kf_loop"])
        err = np.abs(d["T_wc_corrected"] - truth[SCHEDS[b][n_end]]).max()
        print("lane %d: relocalised pose against the ground truth: %.3e" % (b, err))
        assert err <= 3 * 1.5e-3
    assert log[-1][2][0] != log[-1][2][1]                  # the lanes' graphs differ in size


def test_close_loop_at_lane_0_return(capi):
    """(b): the full call at the end of lane 0's walk with mask [1, 0, 1].  Lane 0 is corrected: by the documented rules (the
    restatement on the graph rebuilt from its taps) and as a session driven alone over the same walk is by
    vslam_system_close_loop - integer report fields equal, keyframe and camera poses within the lane-against-session bound of
    tests/test_gpu_batch_reloc.py (1e-9; lanes and sessions are not bit-equal in tracking).  Lane 1, outside the mask, is bitwise
    untouched and its report entry unwritten; lane 2 finds nothing and is bitwise untouched.
    Measured: lane 0 finds keyframe 0 (698 candidates, 180 inliers; 15 keyframes, 14 free poses, 3 trials), its keyframes are within
    3.0e-14 of the restatement, and against the session alone the difference in keyframe and camera poses is 0.0 - bit-equal on this
    walk, before and after the call; the three frames after the correction track with 314, 431 and 417 inliers."""
    L, R, truth = tl.walk()
    bt, Ts, reps = plain_run()
    before = snapshots(bt)
    s0 = bt.system(0)
    tap0 = taps(s0)
    T_cam = Ts[-1][0].copy()
    st, r = raw_loop_call(capi, bt, [1, 0, 1], min_kf_gap=GAP)
    assert st == capi.OK, capi.lib().vslam_last_error()
    after = snapshots(bt)
    assert r[1] is None and after[1] == before[1]
    assert r[2]["success"] == 0 and r[2]["corrected"] == 0 and r[2]["busy"] == 0 and after[2] == before[2]
    assert after[0] != before[0]
    P_new = check_correction(s0, tap0, r[0], T_cam, r[0]["kf_loop"], r[0]["T_wc_corrected"], "lane 0")
    # a session alone over lane 0's walk
    s, T1, R1 = tl.run(capi, 0)
    rs = s.close_loop(min_kf_gap=GAP)
    for k in INT_FIELDS:
        assert rs[k] == r[0][k], (k, rs[k], r[0][k])
    for k in PGO_INT_FIELDS:
        assert rs["pgo"][k] == r[0]["pgo"][k], (k, rs["pgo"][k], r[0]["pgo"][k])
    dk = np.abs(s.keyframes()[1] - P_new).max(); dc = np.abs(rs["T_wc"] - r[0]["T_wc"]).max()
    print("lane 0 against the session alone: keyframes %.3e, camera %.3e, before the call %.3e" % (dk, dc, np.abs(T1[-1] - T_cam).max()))
    assert dk <= 1e-9 and dc <= 1e-9
    s.close()
    # tracking goes on from the corrected pose
    for q, j in enumerate((1, 2, 3)):
        T, rr = bt.track([L[j], None, None], [R[j], None, None], [STEPS + q] * 3, mask=[1, 0, 0])
        print("lane 0, frame after the correction:", rr[0]["n_inliers"], "inliers")
        assert rr[0]["n_inliers"] >= 50
    bt.close()


def test_correct_loop_on_two_lanes_in_one_call(capi):
    """(c): lane 0 is said to be 0.3 m / 2 degrees from its true pose, anchored at its keyframe 1; lane 1 0.2 m / 1.5 degrees
    another way, anchored at its keyframe 2: two graphs of different size solved in the same launch, each against the
    restatement.  Lane 2, outside the mask, is untouched."""
    L, R, truth = tl.walk()
    bt, Ts, reps = drive(capi)
    before = snapshots(bt)
    tp = [taps(bt.system(b)) for b in (0, 1)]
    assert len(tp[0]["P"]) != len(tp[1]["P"])
    T_cam = [Ts[len(SCHEDS[b]) - 1][b].copy() for b in (0, 1)]
    drift = [pr.make_pose(pr.so3_exp(np.array([0.0, np.deg2rad(2.0), 0.0])), np.array([0.3, 0.0, 0.0])),
             pr.make_pose(pr.so3_exp(np.array([0.0, 0.0, np.deg2rad(1.5)])), np.array([0.0, 0.05, -0.2]))]
    T_corr = [truth[0] @ drift[0], truth[0] @ drift[1]]
    st, r = raw_loop_call(capi, bt, [1, 1, 0], kf_loops=[1, 2, 0], poses=np.array(T_corr + [np.eye(4)]))
    assert st == capi.OK, capi.lib().vslam_last_error()
    assert r[2] is None and snapshots(bt)[2] == before[2]
    for b in (0, 1):
        P_new = check_correction(bt.system(b), tp[b], r[b], T_cam[b], [1, 2][b], T_corr[b], "lane %d" % b)
        assert np.abs(P_new[-1] - tp[b]["P"][-1]).max() > 0.05          # the correction arrived
    for q, j in enumerate((1, 2)):
        T, rr = bt.track([L[j], L[j], None], [R[j], R[j], None], [STEPS + q] * 3, mask=[1, 1, 0])
        assert rr[0]["n_inliers"] >= 50 and rr[1]["n_inliers"] >= 50
    # the Python binding: same call shape, None for lanes outside the mask (the camera is said to be where it is: no drift left)
    d = bt.correct_loop([1, None, None], [T[0], None, None], mask=[1, 0, 0])
    assert d[1] is None and d[2] is None and d[0]["corrected"] == 1
    bt.close()


def test_refusals(capi):
    L, R, truth = tl.walk()
    bt = capi.Batch(RIG, 1500, 3, T0s=[truth[0]] * 3, local_mapping=0)
    T, _ = bt.track([L[0], L[0], None], [R[0], R[0], None], [0] * 3, mask=[1, 1, 0])        # lane 2 has no tracked frame

    def refused(mask, **kw):
        before = [tl.snapshot(bt.system(b)) for b in (0, 1)]
        st, r = raw_loop_call(capi, bt, mask, **kw)
        assert st == capi.ERR_INVALID, (st, capi.lib().vslam_last_error())
        assert all(x is None for x in r) and [tl.snapshot(bt.system(b)) for b in (0, 1)] == before
        return capi.lib().vslam_last_error().decode()

    assert "lane 2" in refused([1, 1, 1])                                          # a lane without a tracked frame in the mask
    assert "lane 2" in refused([0, 0, 1], kf_loops=[0, 0, 0], poses=np.array([T[0]] * 3))
    T2, _ = bt.track([L[1], L[1], None], [R[1], R[1], None], [1] * 3, mask=[1, 1, 0])
    K = bt.system(1).counts()["keyframes"]
    assert "lane 1" in refused([0, 1, 0], kf_loops=[0, K - 1, 0], poses=np.array([T2[0]] * 3))        # kf_loop = the latest keyframe
    assert "lane 1" in refused([0, 1, 0], kf_loops=[0, K, 0], poses=np.array([T2[0]] * 3))            # out of range
    bad = np.array([T2[0]] * 3); bad[1, 0, 3] = np.nan
    refused([1, 1, 0], kf_loops=[0, 0, 0], poses=bad)                                                 # a non-finite pose (or kf_loop: the latest)
    refused([1, 1, 0], min_kf_gap=-1)
    refused([1, 1, 0], loop_weight=-1.0)
    refused([1, 1, 0], mode=2)
    reps = (capi.LoopReport * 3)()
    assert capi.lib().vslam_batch_close_loop(bt.h_b, None, None, reps) == capi.ERR_INVALID          # a NULL mask
    mk = np.ones(3, np.uint8)
    assert capi.lib().vslam_batch_close_loop(bt.h_b, mk.ctypes.data_as(C.c_void_p), None, None) == capi.ERR_INVALID
    st, r = raw_loop_call(capi, bt, [1, 1, 0], min_kf_gap=GAP)                     # legal: too few keyframes for candidates
    assert st == capi.OK and r[2] is None and all(r[b]["success"] == 0 and r[b]["corrected"] == 0 for b in (0, 1))
    bt.close()
    imu = dict(gravity=(0.0, 9.81, 0.0), noise=(1.7e-4, 2e-5, 2e-3, 3e-3), T_bs=np.eye(4), hz=200)
    bi = capi.Batch(RIG, 1500, 3, T0s=[truth[0]] * 3, imu=imu, local_mapping=0)
    Ti, _ = bi.track([L[0]] * 3, [R[0]] * 3, [0] * 3)
    before = [tl.snapshot(bi.system(b)) for b in range(3)]
    for kw in (dict(), dict(kf_loops=[0, 0, 0], poses=Ti)):
        st, r = raw_loop_call(capi, bi, [1, 1, 1], **kw)
        assert st == capi.ERR_INVALID and all(x is None for x in r)
    assert [tl.snapshot(bi.system(b)) for b in range(3)] == before
    bi.close()


def test_busy_lane_beside_a_lane_that_detects(capi):
    """local_mapping = 2, mapping_delay = 2, detect_only calls on all lanes after every step: a lane between the hand-over of a
    local BA and its landing reports busy (success 0, no candidates, untouched) while another lane of the same call is not busy
    and runs its detection.  Lanes on identical walks insert their keyframes at the same steps and would be busy together, so
    lane 1 walks its shorter way from source frame 3 on: its keyframes fall on other steps.  Found by running it (the printed log):
    eighteen of the 79 calls are such calls - lanes 0 and 2 busy beside lane 1 at steps 12, 19, 20, 23, 24, 33, 34; lane 1 busy
    beside lanes 0 and 2 at steps 14, 21, 22, 28, 29, 53, 54; lane 0 busy beside lanes 1 and 2 at steps 67, 68, 74, 75."""
    scheds = [SCHEDS[0], list(range(3, 35)) + list(range(33, 2, -1)), SCHEDS[2]]
    log = []

    def hook(bt, n, mask, T, rep):
        before = snapshots(bt)
        d = bt.close_loop(detect_only=1, min_kf_gap=GAP)
        after = snapshots(bt)
        for b in range(3):
            if d[b]["busy"]:
                assert d[b]["success"] == 0 and d[b]["n_candidates"] == 0 and after[b] == before[b], (n, b)
        assert after == before, n
        log.append((n, d))

    bt, Ts, reps = drive(capi, 2, hook, scheds=scheds, mapping_delay=2)
    bt.close()
    mixed = []
    for n, d in log:
        print(n, [(x["busy"], x["success"], x["n_candidates"]) for x in d])
        busy = [b for b in range(3) if d[b]["busy"]]
        ran = [b for b in range(3) if not d[b]["busy"] and d[b]["n_candidates"] >= 50]       # (50: reloc.min_inliers, the stage ran)
        if busy and ran:
            mixed.append((n, busy, ran))
    print("calls with a busy lane beside a detecting lane:", mixed)
    assert mixed
