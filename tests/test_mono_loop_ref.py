"""The mono + IMU restatement (tests/mono_loop_ref.py) alone, on the sequence the GPU tests use (synth.MONO_CALLS): the conditions
that make the GPU parity test meaningful, and known answers of the movement gate."""
import numpy as np
import synth
import mono_loop_ref as ml


def _rot_y(deg):
    a = np.radians(deg)
    T = np.eye(4)
    T[0, 0] = T[2, 2] = np.cos(a); T[0, 2] = np.sin(a); T[2, 0] = -np.sin(a)
    return T


def test_gate_known_answers():
    """Both conditions are required and both are inclusive.  The reference's 0.1 m is the float literal 0.1f held in a double
    (0.100000001490116...): that value is the smallest accepted baseline, and the double 0.1 just below it is refused."""
    m01 = float(np.float32(0.1))
    assert ml.BASELINE_THRESHOLD == m01 and ml.ANGLE_THRESHOLD == 5.0
    assert not ml.gate_accepts(m01, 4.9)               # 0.1 m / 4.9 degrees
    assert not ml.gate_accepts(0.09, 10.0)             # 0.09 m / 10 degrees
    assert ml.gate_accepts(m01, 5.0)                   # 0.1 m / 5 degrees
    assert not ml.gate_accepts(0.1, 5.0)               # (double 0.1 < 0.1f)
    # the same through poses: a translation along x and a rotation about y
    for dist, deg, want in ((m01, 4.9, False), (0.09, 10.0, False), (0.11, 5.5, True), (0.11, 0.0, False), (0.0, 30.0, False)):
        T2 = _rot_y(deg); T2[0, 3] = dist
        b, a = ml.gate_inputs(np.eye(4), T2)
        assert abs(b - dist) < 1e-15 and abs(a - deg) < 1e-9
        assert ml.gate_accepts(b, a) == want
    # relative to a start pose that is not the identity
    T1 = _rot_y(40.0); T1[:3, 3] = (1.0, -2.0, 0.5)
    T2 = T1 @ _rot_y(6.0); T2[:3, 3] += (0.0, 0.2, 0.0)
    b, a = ml.gate_inputs(T1, T2)
    assert abs(b - 0.2) < 1e-12 and abs(a - 6.0) < 1e-9


def test_sequence_meets_the_conditions_of_the_gpu_test():
    lg = ml.reference_run().log
    assert len(lg) == len(synth.MONO_CALLS) == 17
    states = [l["state"] for l in lg]
    kf_calls = [i for i, s in enumerate(states) if s == ml.BOOTSTRAP]
    assert len(kf_calls) == 3
    # the gate refuses >= 1 call before the first bootstrap keyframe and >= 1 between two bootstrap keyframes
    before = [i for i in range(kf_calls[0]) if states[i] == ml.REFUSED]
    between = [i for i in range(kf_calls[0], kf_calls[-1]) if states[i] == ml.REFUSED]
    assert len(before) >= 1 and len(between) >= 1
    # one of them fails only the rotation test
    assert any(lg[i]["baseline"] >= ml.BASELINE_THRESHOLD and lg[i]["angle"] < ml.ANGLE_THRESHOLD for i in before + between)
    for i in before + between:
        assert not lg[i]["keyframe"] and lg[i]["n_keyframes"] == (0 if i < kf_calls[0] else lg[i - 1]["n_keyframes"])
    # refused calls leave the pose where it was
    assert np.array_equal(lg[before[0]]["pose"], synth.mono_arc_pose(0))
    assert np.array_equal(lg[between[0]]["pose"], lg[between[0] - 1]["pose"])
    # initialisation on the fourth accepted call
    accepted = [i for i, s in enumerate(states) if s != ml.REFUSED]
    init = accepted[3]
    assert states[init] == ml.INITIALISED and states.count(ml.INITIALISED) == 1 and lg[init]["n_keyframes"] == 4
    info = lg[init]["init"]
    assert lg[init]["new_points"] >= 200 and lg[init]["n_map_points"] == lg[init]["new_points"]
    targets = set()
    for mp in info["created"]:
        targets |= {kf.numb for kf in mp.kFMatches if kf.numb != 0}
        assert 0 in [kf.numb for kf in mp.kFMatches] and len(mp.kFMatches) >= 2
    assert len(targets) >= 2
    assert lg[init]["radius_matches"] == sum(info["per_target"]) and all(n > 0 for n in info["per_target"])
    # the claim-table rule is exercised: a target has more keys than the initialising frame
    kfs = ml.reference_run().keyFrames
    assert len(info["table"]) == max(len(k.keys["kpsL"]) for k in kfs[:4]) > len(kfs[3].keys["kpsL"])
    # >= 8 tracked calls follow, each with >= 50 inliers, each inserting a keyframe and creating nothing
    assert all(l["state"] == ml.TRACKED for l in lg[init + 1:])
    tracked, last = lg[init + 1:-1], lg[-1]
    assert len(tracked) == 10
    for n, l in enumerate(tracked):
        assert l["nIn"] >= 50 and l["keyframe"] and l["new_points"] == 0 and l["radius_matches"] == 0
        assert l["n_map_points"] == lg[init]["n_map_points"]
        assert l["n_keyframes"] == 5 + n
        assert l["n_active_after"] <= (tracked[n - 1]["n_active_after"] if n else lg[init]["n_active_after"])
    assert any(l["outliers"].any() for l in tracked)               # (the flags compared on the GPU are not all zero)
    # after them, one more tracked call from a view 0.01 degrees beside the first keyframe's: the solve loses the pose, every retry
    # round runs (radius 1200 -> 1230 -> ... and back), the call ends below 50 inliers and flags most of its points - the paths the
    # ten calls above never take.  It still inserts its keyframe and creates nothing.
    assert last["rounds"] == 5 and last["radius"] > 1200.0 and last["nIn"] < 50 and last["outliers"].sum() > 100
    assert last["keyframe"] and last["new_points"] == 0 and last["n_map_points"] == lg[init]["n_map_points"] and last["n_keyframes"] == 15
    # the track is where the camera was, up to the translation the first refused bucket held (the whole map is shifted by it)
    shift = synth.mono_arc_pose(synth.MONO_CALLS[0])[:3, 3] - synth.mono_arc_pose(0)[:3, 3]
    for l in lg[kf_calls[0]:-1]:
        T = synth.mono_arc_pose(l["frame"])
        assert np.abs(l["pose"][:3, :3] - T[:3, :3]).max() < 5e-3 and np.abs(l["pose"][:3, 3] + shift - T[:3, 3]).max() < 1e-2
