"""vslam_system_global_ba on the out-and-back corridor walk, after the loop correction at the return and the fuse of the duplicate
map points (closed_session of tests/test_gpu_fuse_loop.py, walk and run of tests/test_gpu_loop.py): the session's keyframes and
map points after the call are the numpy restatement's result (tests/gba_ref.py) on the problem the session's own tap shows.
Measured on an MI355X: 9 keyframes, 871 points, 3 199 pairs, 700 present points after the parallax guard,
7 trials, cost 529.03 -> 504.01, poses within 1.5e-15 and points within 1.3e-13 of the restatement.  No pair of this walk is flagged
wrong, so the loop over the erased pairs runs over none; tests/test_gpu_gba.py pins the flags on a problem with gross outliers."""
import numpy as np
import pytest
import torch  # noqa: F401,E402  (one HIP runtime per process: before the library, as tests/test_gpu_loop.py explains)
import gba_ref as gr
from test_gpu_loop import N_OUT, RIG, run, walk
from test_gpu_fuse_loop import closed_session, snapshot

pytestmark = pytest.mark.gpu


def edge_list(arr):
    return [(int(e["i"]), int(e["j"]), np.array(e["Z"]).reshape(4, 4), float(e["w_rot"]), float(e["w_trans"])) for e in arr]


def fused_session(capi):
    s, n, kf_out, gap, _ = closed_session(capi)
    rep = s.fuse_loop(min_kf_gap=gap)
    assert rep["n_fused"] >= 10
    return s, n


@pytest.mark.parametrize("edge_weight", [0.0, 100.0])
def test_session_against_the_restatement(capi, edge_weight):
    s, n = fused_session(capi)
    prob, ed = s.global_ba_problem(edge_weight=edge_weight)
    edges = edge_list(ed)
    off, tr = s.map_point_observations()
    assert len(edges) == (0 if edge_weight == 0 else len(prob["kf_pose"]) - 1)
    assert prob["kf_fixed"][0] == 1 and prob["kf_local"].all()
    xyz0, outl0 = s.map_points()
    assert prob["lm_index"].tolist() == np.flatnonzero(outl0 == 0).tolist() and prob["lm"].tobytes() == xyz0[prob["lm_index"]].tobytes()
    ref = gr.optimize(prob, edges, sigma=prob["sigma_factor"], inv_sigma=prob["inv_sigma_factor"])
    rep = s.global_ba(edge_weight=edge_weight)
    g, rr = rep["gba"], ref["report"]
    _, poses = s.keyframes()
    xyz, outl = s.map_points()
    dp = np.abs(poses - ref["kf_pose"]).max()
    dl = np.abs(xyz[prob["lm_index"]] - ref["lm"]).max()
    print("edge weight", edge_weight, "report", rep, "| restatement", rr, "| max pose diff", dp, "max point diff", dl, "margin", ref["margin"],
          "| keyframes moved by up to", np.abs(poses - prob["kf_pose"]).max(), "points by up to", np.abs(ref["lm"] - prob["lm"]).max())
    assert rep["busy"] == 0 and rep["success"] == 1
    assert (rep["n_keyframes"], rep["n_landmarks"], rep["n_pairs"], rep["n_edges"]) == (len(prob["kf_pose"]), len(prob["lm"]), len(prob["pair_kf"]), len(edges))
    for k in ("n_free", "n_isolated", "n_present", "n_thin", "n_factors", "accepted", "rejected"):
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
    s.close()


def test_it_keeps_tracking(capi):
    """the bar of tests/test_gpu_fuse_loop.py::test_it_keeps_tracking: the next 20 frames track with at least 50 inliers each; the
    counts are printed beside those of the run without the call"""
    L, R, _ = walk()
    counts = {}
    for with_call in (False, True):
        s, n = fused_session(capi)
        if with_call:
            rep = s.global_ba(edge_weight=100.0)
            assert rep["success"] == 1 and rep["gba"]["final_cost"] < rep["gba"]["initial_cost"]
        counts[with_call] = [s.track(L[1 + q], R[1 + q], n + q)[1]["n_inliers"] for q in range(20)]
        s.close()
    for q in range(20):
        print("frame %d after the call: %d inliers (%d without it)" % (q, counts[True][q], counts[False][q]))
    assert min(counts[True]) >= 50


def test_busy(capi):
    """local_mapping = 2: a call between the hand-over of a mapping pass and its landing reports busy and changes nothing"""
    reports = []

    def hook(s, n, j, T, rep):
        if n < 12 or len([r for r in reports if r["busy"]]) >= 3:
            return
        before = snapshot(s)
        r = s.global_ba()
        if r["busy"]:
            assert snapshot(s) == before, n
            assert r["success"] == 0 and r["n_keyframes"] == 0
        reports.append(r)

    s, _, _ = run(capi, 2, hook, upto=N_OUT, mapping_delay=2)
    s.close()
    assert any(r["busy"] for r in reports)


def test_one_keyframe_and_refusals(capi):
    L, R, truth = walk()
    s = capi.System(RIG, 1500, T0=truth[0], local_mapping=0)

    def refused(call):
        with pytest.raises(capi.VslamError) as ex:
            call()
        return ex.value.status == capi.ERR_INVALID

    assert refused(lambda: s.global_ba())                                  # no tracked frame yet
    assert refused(lambda: s.global_ba_problem())
    s.track(L[0], R[0], 0)
    before = snapshot(s)
    for bad in (dict(edge_weight=-1.0), dict(edge_weight=float("nan")), dict(max_iterations=-1), dict(lambda0=-1.0), dict(lambda0=float("inf"))):
        assert refused(lambda: s.global_ba(**bad)), bad
    rep = s.global_ba()                                                    # one keyframe: nothing to do
    assert rep["success"] == 0 and rep["busy"] == 0 and snapshot(s) == before
    s.close()
    imu = dict(gravity=(0.0, 9.81, 0.0), noise=(1.7e-4, 2e-5, 2e-3, 3e-3), T_bs=np.eye(4), hz=200)
    si = capi.System(RIG, 1500, T0=truth[0], imu=imu, local_mapping=0)
    si.track(L[0], R[0], 0)
    assert refused(lambda: si.global_ba())
    si.close()
    sm = capi.MonoSystem(RIG, 1500, RIG["fps"], T0=truth[0], imu=imu)
    assert refused(lambda: sm.global_ba())
    sm.close()
