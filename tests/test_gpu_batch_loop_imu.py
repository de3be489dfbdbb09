"""Loop closing of the IMU lanes of a vslam_batch (vslam_batch_close_loop_imu / vslam_batch_correct_loop_imu) on the smooth corridor
out-and-back of tests/test_gpu_loop_imu.py, case (d) (its rendering, IMU buckets and helpers are imported): three IMU lanes -
  lane 0 walks frames 0 .. 80 of the walk;
  lane 1 walks frames 8 .. 80 (another start pose and velocity, fewer keyframes, a smaller graph) and is masked out of tracking after;
  lane 2 walks frames 0 .. 80 and is left OUT of the loop mask.
A masked lane must get what a session driven alone gets (poses within 1e-7, the same reports), the lane outside the mask must not
be touched by a bit, and the call makes ONE yaw-only solve for all lanes (the pose-graph measurement hook counts the solves)."""
import ctypes as C
import numpy as np
import pytest
import torch  # noqa: F401,E402   (one HIP runtime per process: before libvslam_hip.so)
import test_gpu_loop_imu as ti

pytestmark = pytest.mark.gpu

FIRST = [0, 8, 0]
INT_FIELDS = ("busy", "success", "corrected", "kf_loop", "n_candidates", "n_nodes", "n_sequential", "n_covisibility", "n_edges", "points_moved",
              "n_active_after")
PGO_FIELDS = ("accepted", "rejected", "n_free", "n_isolated", "half_bandwidth")
RELOC_INTS = ("success", "n_points", "n_pairs", "best_hypothesis", "best_count", "n_inliers", "n_stereo")
SENTINEL = 0xA5


def drive(capi):
    L, R, poses = ti.corridor_walk()
    bt = capi.Batch(ti.RIG, 1500, 3, T0s=[poses[f] for f in FIRST], imu=ti.IMU, velocities=[ti.walk_velocity(f) for f in FIRST], local_mapping=0)
    for step in range(ti.N_WALK + 1):
        fr = [f + step for f in FIRST]
        mask = [n <= ti.N_WALK for n in fr]
        lefts = [L[n] if m else None for n, m in zip(fr, mask)]
        rights = [R[n] if m else None for n, m in zip(fr, mask)]
        bks = [ti.walk_bucket(n) if (m and step > 0) else None for n, m in zip(fr, mask)]
        T, reps = bt.track(lefts, rights, [step] * 3, imu_buckets=bks, mask=mask)
        for b in range(3):
            assert not mask[b] or step == 0 or reps[b]["n_inliers"] >= 50, (step, b, reps[b]["n_inliers"])
    return bt


def lane_state(bt, b):
    return ti.snapshot(bt.system(b))


def test_lanes_equal_sessions_driven_alone(capi):
    bt = drive(capi)
    untouched = lane_state(bt, 2)
    P_old = [bt.system(b).keyframes()[1] for b in range(3)]
    st_old = [bt.system(b).imu_state() for b in range(3)]
    T_old = [None] * 3
    # refusals change nothing: the 6-DoF calls on an IMU batch, a bad parameter
    for call in (lambda: bt.close_loop(min_kf_gap=ti.GAP), lambda: bt.close_loop_imu(min_kf_gap=-1), lambda: bt.close_loop_imu(mode=2)):
        with pytest.raises(capi.VslamError) as ex:
            call()
        assert ex.value.status == capi.ERR_INVALID
    assert [lane_state(bt, b) for b in range(3)][2] == untouched
    # detection alone: reports and projections, nothing changed
    before = [lane_state(bt, b) for b in range(3)]
    det = bt.close_loop_imu(mask=[1, 1, 0], detect_only=1, min_kf_gap=ti.GAP)
    assert [lane_state(bt, b) for b in range(3)] == before and det[2] is None
    for b in (0, 1):
        T_old[b] = det[b][0]["T_wc"]
        assert det[b][0]["success"] == 1 and det[b][0]["corrected"] == 0
    # the call, on report entries pre-filled with sentinel bytes, with the solve counter on
    reps = (capi.LoopReport * 3)(); ireps = (capi.LoopImuReport * 3)()
    C.memset(reps, SENTINEL, C.sizeof(reps)); C.memset(ireps, SENTINEL, C.sizeof(ireps))
    mk = np.array([1, 1, 0], np.uint8)
    prm = capi.System._loop_params(dict(min_kf_gap=ti.GAP))
    capi.pose_graph_set_timing(True)
    status = capi.lib().vslam_batch_close_loop_imu(bt.h_b, mk.ctypes.data_as(C.c_void_p), C.byref(prm), reps, ireps)
    n_solves = capi.pose_graph_solve_count()
    groups = capi.pose_graph_timings()
    capi.pose_graph_set_timing(False)
    assert status == capi.OK, capi.lib().vslam_last_error()
    print("solves:", n_solves, "groups:", groups)
    assert n_solves == 1 and "pgoy_band_chol" in groups and not any(k.startswith("pgo_") for k in groups)      # ONE yaw solve for both lanes
    # the lane outside the mask: session and report entries untouched
    assert lane_state(bt, 2) == untouched
    assert bytes(reps[2]) == bytes([SENTINEL]) * C.sizeof(capi.LoopReport) and bytes(ireps[2]) == bytes([SENTINEL]) * C.sizeof(capi.LoopImuReport)
    for b in (0, 1):
        rep, irep = capi._loop_report_dict(reps[b]), capi._loop_imu_report_dict(ireps[b])
        want, iwant, Pw_old, Pw_new, stw = ti.alone(FIRST[b])
        P_new = bt.system(b).keyframes()[1]
        print("lane", b, {k: rep[k] for k in INT_FIELDS}, "pgo", rep["pgo"], "yaw", irep["yaw"], "alone", iwant["yaw"],
              "max pose diff", np.abs(P_new - Pw_new).max())
        assert rep["corrected"] == 1
        for k in INT_FIELDS:
            assert rep[k] == want[k], (b, k, rep[k], want[k])
        for k in PGO_FIELDS:
            assert rep["pgo"][k] == want["pgo"][k], (b, k)
        for k in RELOC_INTS:
            assert rep["reloc"][k] == want["reloc"][k], (b, k)
        assert np.abs(P_old[b] - Pw_old).max() <= 1e-7 and np.abs(P_new - Pw_new).max() <= 1e-7
        assert np.abs(rep["T_wc"] - want["T_wc"]).max() <= 1e-7 and np.abs(rep["T_wc_corrected"] - want["T_wc_corrected"]).max() <= 1e-7
        assert abs(irep["yaw"] - iwant["yaw"]) <= 1e-7 and abs(irep["tilt_dropped"] - iwant["tilt_dropped"]) <= 1e-7
        assert np.abs(irep["T_wc_projected"] - iwant["T_wc_projected"]).max() <= 1e-7
        # (a velocity is a difference of two poses at 1e-7 over a frame interval of 0.05 s: the bound of tests/test_gpu_reloc_imu.py)
        assert np.abs(irep["velocity"] - iwant["velocity"]).max() <= 2e-7 / 0.05 and np.abs(irep["velocity_before"] - iwant["velocity_before"]).max() <= 2e-7 / 0.05
        ti.check_correction(P_old[b], P_new, T_old[b], rep["T_wc"], st_old[b], bt.system(b).imu_state(), irep)
    assert capi._loop_imu_report_dict(ireps[0])["yaw"] != capi._loop_imu_report_dict(ireps[1])["yaw"]      # (two different corrections)
    # lane 0 tracks on
    L, R, _ = ti.corridor_walk()
    for q in (1, 2):
        n = ti.N_WALK + q
        T, rr = bt.track([L[n], None, None], [R[n], None, None], [n] * 3, imu_buckets=[ti.walk_bucket(n), None, None], mask=[True, False, False])
        assert rr[0]["n_inliers"] >= 50
    bt.close()


def test_correct_loop_imu_lanes_and_refusals(capi):
    """vslam_batch_correct_loop_imu with a pure-tilt claim on lane 0 and a yaw claim on lane 1: lane 0 changes by no bit, lane 1 equals
    what System.correct_loop_imu gives the same session state (its own invariants); a batch without IMU is refused"""
    import pgo_ref as pr
    bt = drive(capi)
    cam = bt.close_loop_imu(mask=[1, 1, 0], detect_only=1, min_kf_gap=ti.GAP)
    cams = [cam[0][0]["T_wc"], cam[1][0]["T_wc"], None]
    tilt = pr.make_pose(pr.so3_exp(np.deg2rad(2.0) * np.array([1.0, 0.0, 0.0])) @ cams[0][:3, :3], cams[0][:3, 3])
    yawc = pr.make_pose(pr.so3_exp(np.deg2rad(0.2) * ti.GHAT) @ cams[1][:3, :3], cams[1][:3, 3] + np.array([0.01, 0.0, 0.0]))
    P_old = [bt.system(b).keyframes()[1] for b in range(3)]
    X_old = bt.system(0).map_points()[0]
    st_old = [bt.system(b).imu_state() for b in range(3)]
    untouched = lane_state(bt, 2)
    capi.pose_graph_set_timing(True)
    out = bt.correct_loop_imu([0, 0, None], [tilt, yawc, None], mask=[1, 1, 0])
    assert capi.pose_graph_solve_count() == 1
    capi.pose_graph_set_timing(False)
    assert out[2] is None and lane_state(bt, 2) == untouched
    r0, i0 = out[0]
    assert r0["corrected"] == 1 and r0["pgo"]["iterations"] == 0 and abs(i0["yaw"]) <= 1e-12 and abs(i0["tilt_dropped"] - np.deg2rad(2.0)) <= 1e-9
    assert bt.system(0).keyframes()[1].tobytes() == P_old[0].tobytes() and bt.system(0).map_points()[0].tobytes() == X_old.tobytes()
    r1, i1 = out[1]
    assert r1["corrected"] == 1 and r1["pgo"]["accepted"] >= 1 and abs(i1["yaw"] - np.deg2rad(0.2)) <= 1e-9 and i1["tilt_dropped"] <= 1e-9
    ti.check_correction(P_old[1], bt.system(1).keyframes()[1], cams[1], r1["T_wc"], st_old[1], bt.system(1).imu_state(), i1)
    with pytest.raises(capi.VslamError) as ex:
        bt.correct_loop_imu([-1, 0, None], [tilt, yawc, None], mask=[1, 1, 0])
    assert ex.value.status == capi.ERR_INVALID and "lane 0" in str(ex.value)
    bt.close()
    plain = capi.Batch(ti.RIG, 1500, 2, local_mapping=0)
    with pytest.raises(capi.VslamError) as ex:
        plain.close_loop_imu()
    assert ex.value.status == capi.ERR_INVALID and "no IMU" in str(ex.value)
    plain.close()
