"""vslam_batch_fuse_loop and vslam_batch_global_ba on the three-lane corridor walk of tests/test_gpu_batch_loop.py (its drive,
schedules and GAP are imported): lanes 0 and 1 walk out and come back (40 and 32 frames out: maps and problems of different
size), lane 2 walks out and stops there.  After the walk close_loop corrects lanes 0 and 1; fuse_loop and global_ba then run on
them with mask [1, 1, 0], each as ONE batched device call.  A masked lane must get what the session calls give a session:
the fuse commit is the numpy restatement's (tests/fuse_ref.py) on the lane's own taps, as tests/test_gpu_fuse_loop.py checks a
session; the global BA is tests/gba_ref.py's result on the problem the lane's own tap shows before the call, with the bounds of
tests/test_gpu_gba_session.py; lane 0 also equals a session driven alone over the same walk.  Lanes outside the mask are not
touched at all, their report entries included.
Measured on an MI355X (local_mapping = 0): lane 0 has 15 keyframes, 1 037 points and 3 772 pairs, lane 1 12, 951 and 3 199; the
one fuse call (min_kf_gap 5, lane 0's turn-round) commits 159 and 97 pairs, each the restatement's index for index; the one
global BA call takes 7 and 8 trials (cost 1 447.0 -> 586.6 and 1 216.5 -> 510.3, half-bandwidths 13 and 10) and leaves poses
within 1.6e-15 and points within 1.8e-13 of the restatement; lane 0 against the session alone: 0.0 on keyframes and camera
(bit-equal on this walk); the three frames after it track with 264 - 426 inliers.  With local_mapping = 2 lane 0 is busy beside
the returned lane 1 at step 67: lane 1 fuses 24 pairs and is adjusted in 8 trials."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch  # noqa: F401,E402   (one HIP runtime per process: before libvslam_hip.so, as tests/test_gpu_loop.py explains)
import fuse_ref as fr
import gba_ref as gr
import test_gpu_loop as tl
import test_gpu_batch_loop as bl
import test_gpu_fuse_loop as fl
from test_gpu_gba_session import edge_list

pytestmark = pytest.mark.gpu

GAP = bl.GAP
STEPS = bl.STEPS
SENTINEL = 0xA5
EDGE_WEIGHT = 100.0
FUSE_INTS = ("busy", "n_a", "n_b", "n_fused", "n_obs_moved", "n_obs_dropped", "n_keyframes_touched", "n_active_after")
GBA_INTS = ("busy", "success", "n_keyframes", "n_landmarks", "n_pairs", "n_edges", "n_wrong", "n_outliers", "n_active_after")
GBA_SOLVE_INTS = ("iterations", "accepted", "rejected", "n_free", "n_isolated", "n_present", "n_thin", "n_factors", "half_bandwidth")


def raw_call(capi, bt, which, mask, params, lanes=3):
    """the C call on report entries pre-filled with sentinel bytes: (status, [report dict, or None where the entry still holds them])"""
    if which == "fuse":
        cls, fn, to_dict = capi.FuseLoopReport, capi.lib().vslam_batch_fuse_loop, capi._fuse_loop_report_dict
        prm = capi.System._fuse_loop_params(params)
    else:
        cls, fn, to_dict = capi.SystemGbaReport, capi.lib().vslam_batch_global_ba, capi._system_gba_report_dict
        prm = capi.SystemGbaParams(capi.GbaParams(int(params.get("max_iterations", 0)), float(params.get("lambda0", 0.0))), float(params.get("edge_weight", 0.0)))
    reps = (cls * lanes)()
    C.memset(reps, SENTINEL, C.sizeof(reps))
    mk = np.ascontiguousarray(mask, np.uint8)
    st = fn(bt.h_b, mk.ctypes.data_as(C.c_void_p), C.byref(prm), reps)
    blank = bytes([SENTINEL]) * C.sizeof(cls)
    return st, [None if bytes(reps[b]) == blank else to_dict(reps[b]) for b in range(lanes)]


def snapshots(bt, lanes=(0, 1, 2)):
    """the richer snapshot of tests/test_gpu_fuse_loop.py (observations, tables, descriptors, fused pairs too), per lane"""
    return [fl.snapshot(bt.system(b)) for b in lanes]


def check_fuse(before, after, fused_pairs, last_frame, rep, T_wc, gap, name):
    """a lane's fuse against the restatement, as tests/test_gpu_fuse_loop.py::test_commit_against_the_restatement checks a session:
    before / after are the lane's taps (fl.taps) around the call, fused_pairs and last_frame its taps of those names after it"""
    latest = before["n_kf"] - 1
    live = before["outl"] == 0
    idA = np.nonzero(live & (before["creator"] > latest - gap))[0]
    idB = np.nonzero(live & (before["creator"] <= latest - gap))[0]
    match, best, counts = fr.search(fl.affine_inv(T_wc), fl.K, fl.SIZE, before["xyz"][idA], before["desc"][idA], before["xyz"][idB], before["desc"][idB])
    pairs = [(int(idA[j]), int(idB[match[j]])) for j in range(len(idA)) if match[j] >= 0]
    print(name, "fuse_loop:", rep, "| restatement:", counts, "| split after keyframe", latest - gap, "of", latest)
    assert fused_pairs.tolist() == [list(p) for p in pairs]
    assert rep["busy"] == 0 and (rep["n_a"], rep["n_b"]) == (len(idA), len(idB)) and rep["search"] == counts
    assert len(pairs) >= 10 and rep["n_fused"] >= 10
    kdx = before["creator"].tolist()
    w_obs, w_tab, w_outl, _, w_act, _, w_counts = fr.commit(pairs, before["obs"], before["tables"], kdx, before["outl"].tolist(),
                                                            [0] * len(kdx), before["active"], [0] * len(kdx))
    assert after["obs"] == w_obs
    for k in range(before["n_kf"]):
        assert after["tables"][k]["lmpL"] == w_tab[k]["lmpL"] and after["tables"][k]["lmpR"] == w_tab[k]["lmpR"], k
    assert after["outl"].tolist() == w_outl and after["active"] == w_act
    assert after["xyz"].tobytes() == before["xyz"].tobytes() and after["desc"].tobytes() == before["desc"].tobytes()
    touched, refresh = w_counts["touched"], w_counts["refresh"]
    for k in range(before["n_kf"]):
        got = [(int(w), int(o)) for kk, o, w in after["cov"] if kk == k]
        if k in refresh:
            assert got == fr.connections(k, w_tab, w_obs, before["n_kf"]), k
        else:
            assert got == [(int(w), int(o)) for kk, o, w in before["cov"] if kk == k], k
    assert (rep["n_fused"], rep["n_obs_moved"], rep["n_obs_dropped"], rep["n_keyframes_touched"], rep["n_active_after"]) == \
           (len(pairs), w_counts["n_obs_moved"], w_counts["n_obs_dropped"], len(touched), len(w_act))
    assert len(last_frame[0]) == 0


def check_gba(s, prob, ed, obs_before, outl0, rep, name):
    """a lane's global BA against the restatement on the problem its tap showed before the call: the bounds of
    tests/test_gpu_gba_session.py::test_session_against_the_restatement"""
    edges = edge_list(ed)
    off, tr = obs_before
    ref = gr.optimize(prob, edges, sigma=prob["sigma_factor"], inv_sigma=prob["inv_sigma_factor"])
    g, rr = rep["gba"], ref["report"]
    _, poses = s.keyframes()
    xyz, outl = s.map_points()
    dp = np.abs(poses - ref["kf_pose"]).max()
    dl = np.abs(xyz[prob["lm_index"]] - ref["lm"]).max()
    print(name, "report", rep, "| restatement", rr, "| max pose diff", dp, "max point diff", dl, "margin", ref["margin"])
    assert rep["busy"] == 0 and rep["success"] == 1
    assert (rep["n_keyframes"], rep["n_landmarks"], rep["n_pairs"], rep["n_edges"]) == (len(prob["kf_pose"]), len(prob["lm"]), len(prob["pair_kf"]), len(edges))
    for k in ("n_free", "n_isolated", "n_present", "n_thin", "n_factors", "accepted", "rejected"):
        assert g[k] == rr[k], k
    assert abs(g["initial_cost"] - rr["initial_cost"]) <= 1e-9 * rr["initial_cost"]
    assert abs(g["final_cost"] - rr["final_cost"]) <= 1e-9 * rr["final_cost"]
    assert g["final_cost"] < g["initial_cost"]
    assert ref["margin"] > 1e-9
    assert dp <= 1e-7 and dl <= 1e-7
    wrong = np.flatnonzero(ref["pair_wrong"])
    assert rep["n_wrong"] == len(wrong)
    off2, tr2 = s.map_point_observations()
    for q in wrong:                                          # wrong pairs are gone from the observation and the table taps
        kf, mp = int(prob["pair_kf"][q]), int(prob["lm_index"][prob["pair_lm"][q]])
        was = [tuple(r) for r in tr[off[mp]:off[mp + 1]].tolist() if r[0] == kf]
        assert len(was) == 1
        assert all(r[0] != kf for r in tr2[off2[mp]:off2[mp + 1]].tolist())
        tL, tR = s.keyframe_points(kf)
        assert (was[0][1] < 0 or tL[was[0][1]] != mp) and (was[0][2] < 0 or tR[was[0][2]] != mp)
    assert len(tr2) == len(tr) - len(wrong)
    assert rep["n_outliers"] == int(outl.sum() - outl0.sum())


@functools.lru_cache(maxsize=None)
def sequence():
    """the walk, close_loop on all lanes, then fuse_loop and global_ba with mask [1, 1, 0]: everything the tests look at, taken
    once.  The batch stays open for test_tracking_goes_on, the only test that moves it on."""
    import vslam_capi as capi
    bt, Ts, reps = bl.drive(capi)
    kf_out = [max(reps[n][b]["n_keyframes"] for n in range(bl.N_OUT[b])) for b in (0, 1)]
    rc = bt.close_loop(min_kf_gap=GAP)
    latest0 = bt.system(0).counts()["keyframes"] - 1
    gap = latest0 - (kf_out[0] - 1)                          # lane 0's split is its turn-round; the call has ONE min_kf_gap for all lanes
    D = dict(bt=bt, rc=rc, gap=gap, kf_out=kf_out)
    D["snap2"] = [snapshots(bt, (2,))[0]]
    D["fuse_taps"] = [fl.taps(bt.system(b)) for b in (0, 1)]
    D["fuse"] = raw_call(capi, bt, "fuse", [1, 1, 0], dict(min_kf_gap=gap))
    D["fuse_after"] = [fl.taps(bt.system(b)) for b in (0, 1)]
    D["pairs"] = [bt.system(b).fused_pairs() for b in (0, 1)]
    D["last_frame"] = [bt.system(b).last_frame() for b in (0, 1)]
    D["snap2"].append(snapshots(bt, (2,))[0])
    D["problems"] = [bt.system(b).global_ba_problem(edge_weight=EDGE_WEIGHT) for b in (0, 1)]
    D["obs"] = [bt.system(b).map_point_observations() for b in (0, 1)]
    D["outl0"] = [bt.system(b).map_points()[1] for b in (0, 1)]
    D["gba"] = raw_call(capi, bt, "gba", [1, 1, 0], dict(edge_weight=EDGE_WEIGHT))
    D["snap2"].append(snapshots(bt, (2,))[0])
    D["poses"] = [bt.system(b).keyframes()[1] for b in (0, 1)]
    D["cam0"] = bt.close_loop(mask=[1, 0, 0], detect_only=1, min_kf_gap=GAP)[0]["T_wc"]
    return D


def test_full_sequence(capi):
    D = sequence()
    bt, rc, gap = D["bt"], D["rc"], D["gap"]
    assert rc[0]["corrected"] == 1 and rc[1]["corrected"] == 1 and rc[2]["success"] == 0
    st, rf = D["fuse"]
    assert st == capi.OK
    st, rg = D["gba"]
    assert st == capi.OK
    # lane 2, outside the mask: bitwise untouched by either call, its report entries still hold the sentinel
    assert rf[2] is None and rg[2] is None
    assert D["snap2"][0] == D["snap2"][1] == D["snap2"][2]
    # the lanes' problems differ in size
    p0, p1 = D["problems"][0][0], D["problems"][1][0]
    assert len(p0["kf_pose"]) != len(p1["kf_pose"]) and len(p0["pair_kf"]) != len(p1["pair_kf"])
    for b in (0, 1):
        s = bt.system(b)
        # the fuse on the taps taken right before and right after it (the lane has moved on since: the global BA ran)
        check_fuse(D["fuse_taps"][b], D["fuse_after"][b], D["pairs"][b], D["last_frame"][b], rf[b], rc[b]["T_wc"], gap, "lane %d" % b)
        prob, ed = D["problems"][b]
        check_gba(s, prob, ed, D["obs"][b], D["outl0"][b], rg[b], "lane %d" % b)
        assert D["fuse_taps"][b]["n_kf"] == len(prob["kf_pose"])
    # lane 0 against a session driven alone over the same walk through the three calls
    s, T1, R1 = tl.run(capi, 0)
    rs = s.close_loop(min_kf_gap=GAP)
    fs = s.fuse_loop(min_kf_gap=gap)
    gs = s.global_ba(edge_weight=EDGE_WEIGHT)
    assert rs["corrected"] == 1 and rs["kf_loop"] == rc[0]["kf_loop"]
    for k in FUSE_INTS:
        assert fs[k] == rf[0][k], (k, fs[k], rf[0][k])
    assert fs["search"] == rf[0]["search"] and s.fused_pairs().tolist() == D["pairs"][0].tolist()
    for k in GBA_INTS:
        assert gs[k] == rg[0][k], (k, gs[k], rg[0][k])
    for k in GBA_SOLVE_INTS:
        assert gs["gba"][k] == rg[0]["gba"][k], (k, gs["gba"][k], rg[0]["gba"][k])
    cam = s.close_loop(detect_only=1, min_kf_gap=GAP)["T_wc"]
    dk = np.abs(s.keyframes()[1] - D["poses"][0]).max(); dc = np.abs(cam - D["cam0"]).max()
    print("lane 0 against the session alone: keyframes %.3e, camera %.3e" % (dk, dc))
    assert dk <= 1e-9 and dc <= 1e-9
    s.close()


def test_tracking_goes_on(capi):
    """the next three frames of lanes 0 and 1 track with at least 50 inliers (the existing tests' bound)"""
    L, R, _ = tl.walk()
    bt = sequence()["bt"]
    for q, j in enumerate((1, 2, 3)):
        T, rr = bt.track([L[j], L[j], None], [R[j], R[j], None], [STEPS + q] * 3, mask=[1, 1, 0])
        print("frame %d after the global BA: %d and %d inliers" % (q, rr[0]["n_inliers"], rr[1]["n_inliers"]))
        assert rr[0]["n_inliers"] >= 50 and rr[1]["n_inliers"] >= 50
    bt.close()
    sequence.cache_clear()


def test_busy_lane_beside_a_lane_that_works(capi):
    """local_mapping = 2, mapping_delay = 2, the pattern of tests/test_gpu_batch_loop.py::test_busy_lane_beside_a_lane_that_detects
    (lane 1 walks a shorter way from source frame 3 on, so its keyframes fall on other steps).  Once lane 1 has come back, at the
    first step where lane 0 is between the hand-over of a local BA and its landing: lane 1's loop is closed, then fuse_loop and
    global_ba run with mask [1, 1, 0].  Lane 0 reports busy from both and is untouched; lane 1 is fused and adjusted."""
    scheds = [bl.SCHEDS[0], list(range(3, 35)) + list(range(33, 2, -1)), bl.SCHEDS[2]]
    done = []
    kf_out1 = []

    def hook(bt, n, mask, T, rep):
        if n == 31:
            kf_out1.append(rep[1]["n_keyframes"])            # lane 1's keyframes at its turn-round
        if done or n < len(scheds[1]):
            return
        d = bt.close_loop(detect_only=1, min_kf_gap=GAP)
        if not (d[0]["busy"] and not d[1]["busy"]):
            return
        rc = bt.close_loop(mask=[0, 1, 0], min_kf_gap=GAP)
        assert rc[1]["corrected"] == 1, rc[1]
        gap = (bt.system(1).counts()["keyframes"] - 1) - (kf_out1[0] - 1)
        before = snapshots(bt, (0, 2))
        st, rf = raw_call(capi, bt, "fuse", [1, 1, 0], dict(min_kf_gap=gap))
        assert st == capi.OK
        st, rg = raw_call(capi, bt, "gba", [1, 1, 0], dict(edge_weight=EDGE_WEIGHT))
        assert st == capi.OK
        assert snapshots(bt, (0, 2)) == before
        print("step", n, "fuse", rf, "gba", rg)
        assert rf[0] == dict(rf[0], busy=1, n_a=0, n_b=0, n_fused=0, n_active_after=0)
        assert rg[0]["busy"] == 1 and rg[0]["success"] == 0 and rg[0]["n_keyframes"] == 0
        assert rf[2] is None and rg[2] is None
        assert rf[1]["busy"] == 0 and rf[1]["n_fused"] >= 1 and len(bt.system(1).fused_pairs()) == rf[1]["n_fused"]
        assert rg[1]["busy"] == 0 and rg[1]["success"] == 1 and rg[1]["gba"]["final_cost"] < rg[1]["gba"]["initial_cost"]
        done.append(n)

    bt, Ts, reps = bl.drive(capi, 2, hook, scheds=scheds, mapping_delay=2)
    bt.close()
    print("lane 0 busy beside the returned lane 1 at step", done)
    assert done


def test_refusals(capi):
    L, R, truth = tl.walk()
    bt = capi.Batch(bl.RIG, 1500, 3, T0s=[truth[0]] * 3, local_mapping=0)
    bt.track([L[0], L[0], None], [R[0], R[0], None], [0] * 3, mask=[1, 1, 0])        # lane 2 has no tracked frame
    mk = np.ones(3, np.uint8)

    def refused(which, mask, **params):
        before = snapshots(bt, (0, 1))
        st, r = raw_call(capi, bt, which, mask, params)
        assert st == capi.ERR_INVALID, (st, capi.lib().vslam_last_error())
        assert all(x is None for x in r) and snapshots(bt, (0, 1)) == before
        return capi.lib().vslam_last_error().decode()

    for which in ("fuse", "gba"):
        assert "lane 2" in refused(which, [1, 1, 1])                                 # a lane without a tracked frame in the mask
        assert "lane 2" in refused(which, [0, 0, 1])
    for bad in (dict(min_kf_gap=-1), dict(radius=-1.0), dict(max_hamming=-1), dict(depth_ratio=0.5), dict(radius=float("nan"))):
        refused("fuse", [1, 1, 0], **bad)
    for bad in (dict(edge_weight=-1.0), dict(edge_weight=float("nan")), dict(max_iterations=-1), dict(lambda0=-1.0), dict(lambda0=float("inf"))):
        refused("gba", [1, 1, 0], **bad)
    lib = capi.lib()
    before = snapshots(bt, (0, 1))
    freps = (capi.FuseLoopReport * 3)(); greps = (capi.SystemGbaReport * 3)()
    assert lib.vslam_batch_fuse_loop(bt.h_b, None, None, freps) == capi.ERR_INVALID                   # a NULL mask
    assert lib.vslam_batch_fuse_loop(bt.h_b, mk.ctypes.data_as(C.c_void_p), None, None) == capi.ERR_INVALID
    assert lib.vslam_batch_global_ba(bt.h_b, None, None, greps) == capi.ERR_INVALID
    assert lib.vslam_batch_global_ba(bt.h_b, mk.ctypes.data_as(C.c_void_p), None, None) == capi.ERR_INVALID
    assert snapshots(bt, (0, 1)) == before
    # legal: one keyframe per lane - as the session calls report (no old set, nothing fused; success = 0), nothing changed
    st, r = raw_call(capi, bt, "fuse", [1, 1, 0], {})
    assert st == capi.OK and r[2] is None and all(r[b]["n_fused"] == 0 and r[b]["n_b"] == 0 and r[b]["busy"] == 0 for b in (0, 1))
    st, r = raw_call(capi, bt, "gba", [1, 1, 0], {})
    assert st == capi.OK and r[2] is None and all(r[b]["success"] == 0 and r[b]["busy"] == 0 for b in (0, 1))
    assert snapshots(bt, (0, 1)) == before
    # the Python binding: None for lanes outside the mask
    d = bt.fuse_loop(mask=[1, 0, 0])
    assert d[1] is None and d[2] is None and d[0]["n_fused"] == 0
    d = bt.global_ba(mask=[0, 1, 0], edge_weight=1.0)
    assert d[0] is None and d[2] is None and d[1]["success"] == 0
    bt.close()
    imu = dict(gravity=(0.0, 9.81, 0.0), noise=(1.7e-4, 2e-5, 2e-3, 3e-3), T_bs=np.eye(4), hz=200)
    bi = capi.Batch(bl.RIG, 1500, 3, T0s=[truth[0]] * 3, imu=imu, local_mapping=0)
    bi.track([L[0]] * 3, [R[0]] * 3, [0] * 3)
    before = [tl.snapshot(bi.system(b)) for b in range(3)]
    for which in ("fuse", "gba"):
        st, r = raw_call(capi, bi, which, [1, 1, 1], {})
        assert st == capi.ERR_INVALID and all(x is None for x in r)
    assert [tl.snapshot(bi.system(b)) for b in range(3)] == before
    bi.close()
