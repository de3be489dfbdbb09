"""vslam_system_fuse_loop_imu / vslam_system_global_ba_imu / vslam_system_global_ba_problem_imu on
the smooth corridor out-and-back of tests/test_gpu_loop_imu.py, after vslam_system_close_loop_imu at the return: the fuse pairs
what tests/fuse_ref.py pairs on the session's own taps and leaves the IMU state alone; the session's keyframes and map points
after the adjustment are the restatement's result (tests/gba_yaw_ref.py) on the problem the session's tap shows, every keyframe
and the camera keep gravity, the velocity turns with the camera, and the walk's two remaining frames track.
If the restatement's decision_margin on the session's problem is below 1e-12 an accept / reject decision of the pass hangs on the
last bit of the cost: poses, points and costs are still compared, trial counts are not, and the test says so."""
import numpy as np
import pytest
import synth
import torch  # noqa: F401,E402  (one HIP runtime per process: before the library, as tests/test_gpu_loop.py explains)
import fuse_ref as fr
import gba_yaw_ref as gy
import pgo_yaw_ref as py
from test_gpu_loop_imu import G, GAP, GHAT, IMU, N_WALK, RIG, check_correction, corridor_walk, drive_walk, walk_bucket, walk_velocity
from test_gpu_fuse_loop import affine_inv, taps
from test_gpu_gba_session import edge_list

pytestmark = pytest.mark.gpu
K = (RIG["fx"], RIG["fy"], RIG["cx"], RIG["cy"])
SIZE = (RIG["w"], RIG["h"])


def imu_bytes(s):
    st = s.imu_state()
    return st["velocity"].tobytes(), st["bias"].tobytes(), st["bias_good"].tobytes(), st["pending"]


def closed_walk(capi):
    """the walk and the yaw-only loop correction at the return; returns the session, the keyframes of the way out, the fuse's
    min_kf_gap that puts the split at the turn-round and the camera pose after the correction"""
    mark = {}

    def hook(s, n, T, rep):
        if n <= N_WALK // 2:
            mark["kf_out"] = s.counts()["keyframes"]

    s, Ts, reps = drive_walk(capi, 0, hook)
    rep, irep = s.close_loop_imu(min_kf_gap=GAP)
    assert rep["success"] == 1 and rep["corrected"] == 1
    latest = s.counts()["keyframes"] - 1
    return s, mark["kf_out"], latest - (mark["kf_out"] - 1), rep["T_wc"]


def test_fuse_pairs_the_restatements_pairs_and_leaves_the_imu_state(capi):
    s, kf_out, gap, T_wc = closed_walk(capi)
    before = taps(s)
    imu0 = imu_bytes(s)
    poses0 = s.keyframes()[1].tobytes()
    live = before["outl"] == 0
    idA = np.nonzero(live & (before["creator"] > kf_out - 1))[0]
    idB = np.nonzero(live & (before["creator"] <= kf_out - 1))[0]
    match, best, counts = fr.search(affine_inv(T_wc), K, SIZE, before["xyz"][idA], before["desc"][idA], before["xyz"][idB], before["desc"][idB])
    pairs = [(int(idA[j]), int(idB[match[j]])) for j in range(len(idA)) if match[j] >= 0]
    rep = s.fuse_loop_imu(min_kf_gap=gap)
    print("fuse_loop_imu:", rep, "| restatement:", counts, "| keyframes of the way out:", kf_out, "min_kf_gap", gap, "| pairs fused:", rep["n_fused"])
    assert rep["busy"] == 0 and (rep["n_a"], rep["n_b"]) == (len(idA), len(idB)) and rep["search"] == counts
    assert s.fused_pairs().tolist() == [list(p) for p in pairs]          # the session's pairs are the restatement's, index for index
    assert rep["n_fused"] == len(pairs) and rep["n_fused"] >= 1
    kdx = before["creator"].tolist()
    w_obs, w_tab, w_outl, _, w_act, _, w_counts = fr.commit(pairs, before["obs"], before["tables"], kdx, before["outl"].tolist(),
                                                            [0] * len(kdx), before["active"], [0] * len(kdx))
    after = taps(s)
    assert after["obs"] == w_obs and after["outl"].tolist() == w_outl and after["active"] == w_act
    assert after["xyz"].tobytes() == before["xyz"].tobytes()
    assert imu_bytes(s) == imu0 and s.keyframes()[1].tobytes() == poses0   # the IMU state and the keyframes: not a bit
    s.close()


@pytest.mark.parametrize("edge_weight", [0.0, 100.0])
def test_session_against_the_restatement(capi, edge_weight):
    L, R, _ = corridor_walk()
    s, kf_out, gap, T_old = closed_walk(capi)
    assert s.fuse_loop_imu(min_kf_gap=gap)["n_fused"] >= 1
    prob, ed = s.global_ba_problem_imu(edge_weight=edge_weight)
    edges = edge_list(ed)
    off, tr = s.map_point_observations()
    assert len(edges) == (0 if edge_weight == 0 else len(prob["kf_pose"]) - 1)
    assert prob["kf_fixed"][0] == 1 and prob["kf_local"].all()
    xyz0, outl0 = s.map_points()
    assert prob["lm_index"].tolist() == np.flatnonzero(outl0 == 0).tolist() and prob["lm"].tobytes() == xyz0[prob["lm_index"]].tobytes()
    ref = gy.optimize(prob, edges, G, sigma=prob["sigma_factor"], inv_sigma=prob["inv_sigma_factor"])
    P_old = s.keyframes()[1]
    st = s.imu_state()
    rep, irep = s.global_ba_imu(edge_weight=edge_weight)
    g, rr = rep["gba"], ref["report"]
    _, poses = s.keyframes()
    xyz, outl = s.map_points()
    dp = np.abs(poses - ref["kf_pose"]).max()
    dl = np.abs(xyz[prob["lm_index"]] - ref["lm"]).max()
    counted = ref["decision_margin"] >= 1e-12
    print("edge weight", edge_weight, "report", rep, "| restatement", rr, "| max pose diff", dp, "max point diff", dl, "chi2 margin", ref["margin"],
          "decision margin", ref["decision_margin"], "| keyframes moved by up to", np.abs(poses - prob["kf_pose"]).max(), "| yaw", irep["yaw"],
          "velocity", irep["velocity_before"], "->", irep["velocity"])
    if not counted:
        print("decision margin below 1e-12: a decision of this pass hangs on the last bit of the cost; trial counts are NOT compared")
    assert rep["busy"] == 0 and rep["success"] == 1
    assert (rep["n_keyframes"], rep["n_landmarks"], rep["n_pairs"], rep["n_edges"]) == (len(prob["kf_pose"]), len(prob["lm"]), len(prob["pair_kf"]), len(edges))
    for k in ("n_free", "n_isolated", "n_present", "n_thin", "n_factors") + (("accepted", "rejected") if counted else ()):
        assert g[k] == rr[k], k
    assert abs(g["initial_cost"] - rr["initial_cost"]) <= 1e-9 * rr["initial_cost"]
    assert abs(g["final_cost"] - rr["final_cost"]) <= 1e-9 * rr["final_cost"]
    assert g["final_cost"] < g["initial_cost"]
    assert ref["margin"] > 1e-9
    assert dp <= 1e-7 and dl <= 1e-7
    # wrong pairs are gone from the observation and the table taps
    wrong = np.flatnonzero(ref["pair_wrong"])
    assert rep["n_wrong"] == len(wrong)
    off2, tr2 = s.map_point_observations()
    for q in wrong:
        kf, mp = int(prob["pair_kf"][q]), int(prob["lm_index"][prob["pair_lm"][q]])
        was = [tuple(r) for r in tr[off[mp]:off[mp + 1]].tolist() if r[0] == kf]
        assert len(was) == 1
        assert all(r[0] != kf for r in tr2[off2[mp]:off2[mp + 1]].tolist())
        tl, tR = s.keyframe_points(kf)
        assert (was[0][1] < 0 or tl[was[0][1]] != mp) and (was[0][2] < 0 or tR[was[0][2]] != mp)
    assert len(tr2) == len(tr) - len(wrong)
    assert rep["n_outliers"] == int(outl.sum() - outl0.sum())
    # gravity kept on every keyframe and on the camera, the velocity turned by dR, its norm kept, bias untouched
    check_correction(P_old, poses, T_old, irep["T_wc"], st, s.imu_state(), irep)
    dR = irep["T_wc"][:3, :3] @ T_old[:3, :3].T
    assert abs(irep["yaw"] - py.twist(dR, GHAT)) <= 1e-12
    assert np.abs(poses - P_old).max() > 0 and np.linalg.norm(st["velocity"]) > 0.01
    for q in (1, 2):
        T, r = s.track(L[N_WALK + q], R[N_WALK + q], N_WALK + q, imu_bucket=walk_bucket(N_WALK + q))
        print("frame after the adjustment:", r["n_inliers"], "inliers")
        assert r["n_inliers"] >= 50
    s.close()


def test_busy_while_mapping_is_in_flight(capi):
    """local_mapping = 2: the calls between the hand-over of a mapping pass and its landing report busy and change nothing"""
    L, R, poses = corridor_walk()
    s = capi.System(RIG, 1500, T0=poses[0], imu=dict(IMU, velocity=walk_velocity(0)), local_mapping=2, mapping_delay=2)
    busy = 0
    for n in range(N_WALK // 2):
        s.track(L[n], R[n], n, imu_bucket=walk_bucket(n) if n else None)
        if s.counts()["keyframes"] < 2 or busy >= 3:
            continue
        P = s.keyframes()[1].tobytes()
        X = s.map_points()[0].tobytes()
        imu0 = imu_bytes(s)
        f = s.fuse_loop_imu(min_kf_gap=GAP)
        if not f["busy"]:
            continue                                        # (nothing in flight; the walk has not returned, so nothing is fused either)
        r, ir = s.global_ba_imu()
        assert r["busy"] == 1 and r["success"] == 0 and r["n_keyframes"] == 0 and ir["yaw"] == 0.0
        assert ir["velocity_before"].tobytes() == imu0[0] and ir["velocity"].tobytes() == imu0[0]
        assert s.keyframes()[1].tobytes() == P and s.map_points()[0].tobytes() == X and imu_bytes(s) == imu0
        with pytest.raises(capi.VslamError):
            s.global_ba_problem_imu()                       # (the tap refuses while a pass is in flight)
        busy += 1
    print("busy calls:", busy)
    assert busy >= 1
    s.close()


def test_who_is_served(capi):
    """the three new calls refuse a session without IMU and a mono session; the three old calls still refuse the IMU session"""
    def refused(call, word=None):
        with pytest.raises(capi.VslamError) as ex:
            call()
        return ex.value.status == capi.ERR_INVALID and (word is None or word in str(ex.value))

    L, R, poses = corridor_walk()
    plain = capi.System(RIG, 1500, T0=poses[0], local_mapping=0)
    assert refused(lambda: plain.global_ba_imu())           # (no IMU, and no frame yet)
    plain.track(L[0], R[0], 0)
    before = (plain.counts(), plain.keyframes()[1].tobytes(), plain.map_points()[0].tobytes())
    assert refused(lambda: plain.fuse_loop_imu(), "no IMU") and refused(lambda: plain.global_ba_imu(), "no IMU")
    assert refused(lambda: plain.global_ba_problem_imu(), "no IMU")
    assert (plain.counts(), plain.keyframes()[1].tobytes(), plain.map_points()[0].tobytes()) == before
    plain.close()
    mono = capi.MonoSystem(RIG, 1500, synth.MONO_FPS, imu=IMU)
    assert refused(lambda: mono.fuse_loop_imu(), "mono") and refused(lambda: mono.global_ba_imu(), "mono") and refused(lambda: mono.global_ba_problem_imu(), "mono")
    mono.close()
    si = capi.System(RIG, 1500, T0=poses[0], imu=dict(IMU, velocity=walk_velocity(0)), local_mapping=0)
    assert refused(lambda: si.global_ba_imu(), "no tracked frame")
    si.track(L[0], R[0], 0)
    imu0 = imu_bytes(si)
    before = (si.counts(), si.keyframes()[1].tobytes(), si.map_points()[0].tobytes())
    assert refused(lambda: si.fuse_loop(), "IMU") and refused(lambda: si.global_ba(), "IMU") and refused(lambda: si.global_ba_problem(), "IMU")
    for bad in (dict(edge_weight=-1.0), dict(edge_weight=float("nan")), dict(max_iterations=-1), dict(lambda0=-1.0)):
        assert refused(lambda: si.global_ba_imu(**bad)), bad
    assert refused(lambda: si.fuse_loop_imu(min_kf_gap=-1))
    rep, irep = si.global_ba_imu()                          # one keyframe: nothing to do
    assert rep["success"] == 0 and rep["busy"] == 0 and irep["yaw"] == 0.0 and irep["velocity"].tobytes() == imu0[0]
    assert (si.counts(), si.keyframes()[1].tobytes(), si.map_points()[0].tobytes()) == before and imu_bytes(si) == imu0
    si.close()
