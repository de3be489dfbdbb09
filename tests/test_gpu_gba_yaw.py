"""vslam_global_ba_yaw / _batch against the numpy restatement (tests/gba_yaw_ref.py) on the shapes where the 4x4 kernels can go
wrong - one block alone in its wave, block counts of 1 and 2 modulo 3 without off-diagonal landmark blocks, a band as wide as the
matrix, a block list of 300, band and loop edge after the reordering, the mixed case, rejected trials, outliers - with an
unnormalised axis that is aligned with no coordinate axis.  Tolerances are those of test_gpu_gba.py: 1e-7 absolute per pose entry
and landmark coordinate, 1e-9 relative on the costs, final_lambda to 1e-12 relative, the same accepted and rejected trials, equal
flags (chi2 margin above 1e-9); R_new R_old^T g = g to 1e-12 on every keyframe; fixed, isolated and thin items bit for bit.
tests/test_gba_yaw_ref.py holds the condition under which trial counts may be compared (decision_margin >= 1e-12) on the CPU."""
import functools
import numpy as np
import pytest
import gba_ref as gr
import gba_yaw_ref as gy
import pgo_yaw_ref as py

pytestmark = pytest.mark.gpu
AXIS = gy.AXIS
CASES_A = ["one_free", "two_free", "no_shared4", "no_shared5", "dense12", "long_list", "chain40", "chain60_loop", "mixed", "rejected", "outliers"]


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, edges, parameters, the restatement's result): computed once, never modified"""
    prob, edges = gy.build(name)
    prm = gy.PARAMS.get(name, {})
    ref = gy.optimize(prob, edges, AXIS, **prm)
    for a in list(prob.values()) + [ref["kf_pose"], ref["lm"], ref["pair_wrong"]]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return prob, edges, prm, ref


def run(capi, prob, edges=None, axis=AXIS, **prm):
    return capi.global_ba_yaw(prob["rig"], gr.SIGMA, gr.INV_SIGMA, prob, axis, edges, **prm)


def same_bytes(a, b):
    return (a["kf_pose"].tobytes() == b["kf_pose"].tobytes() and a["lm"].tobytes() == b["lm"].tobytes() and
            a["pair_wrong"].tobytes() == b["pair_wrong"].tobytes() and a["report"] == b["report"])


@pytest.mark.parametrize("name", CASES_A)
def test_against_restatement(capi, name):
    prob, edges, prm, ref = case(name)
    assert ref["decision_margin"] >= 1e-12 and ref["margin"] > 1e-9
    got = run(capi, prob, edges, **prm)
    rep, rrep, S = got["report"], ref["report"], ref["structure"]
    dl = np.abs(got["lm"] - ref["lm"]).max() if len(ref["lm"]) else 0.0
    tilt = gy.gravity_error(got["kf_pose"], prob["kf_pose"], AXIS)
    print(name, rep, "ref", rrep, "max pose diff", np.abs(got["kf_pose"] - ref["kf_pose"]).max(), "max landmark diff", dl,
          "flags", int(got["pair_wrong"].sum()), "chi2 margin", ref["margin"], "decision margin", ref["decision_margin"], "gravity error", tilt)
    for k in ("n_free", "n_isolated", "n_present", "n_thin", "n_factors"):
        assert rep[k] == rrep[k], k
    assert rep["iterations"] == rep["accepted"] + rep["rejected"]
    assert (rep["accepted"], rep["rejected"]) == (rrep["accepted"], rrep["rejected"])        # the same trials as the restatement
    assert abs(rep["initial_cost"] - rrep["initial_cost"]) <= 1e-9 * rrep["initial_cost"]
    assert abs(rep["final_cost"] - rrep["final_cost"]) <= 1e-9 * rrep["final_cost"]
    assert rep["final_lambda"] == pytest.approx(rrep["final_lambda"], rel=1e-12)
    assert np.abs(got["kf_pose"] - ref["kf_pose"]).max() <= 1e-7
    assert dl <= 1e-7
    assert np.array_equal(got["pair_wrong"], ref["pair_wrong"])
    assert tilt <= 1e-12                                                              # roll and pitch about g: untouched
    start = np.asarray(prob["kf_pose"], np.float64)
    for k in range(len(start)):
        if S.col[k] < 0:
            assert got["kf_pose"][k].tobytes() == start[k].tobytes(), k          # fixed and isolated keyframes: not a bit
    lm0 = np.asarray(prob["lm"], np.float64)
    for l in np.flatnonzero(~S.present):
        assert got["lm"][l].tobytes() == lm0[l].tobytes(), l                       # thin landmarks: not a bit
    assert same_bytes(run(capi, prob, edges, **prm), got)                        # (e) the same input, the same bytes


def test_shapes_of_the_cases(capi):
    """what each case is there for"""
    rep = lambda name: run(capi, *case(name)[:2], **case(name)[2])["report"]
    r = rep("one_free")
    assert (r["n_free"], r["half_bandwidth"]) == (1, 0)            # one block alone in its wave
    for name, nf in (("two_free", 2), ("no_shared4", 4), ("no_shared5", 5)):
        r = rep(name)
        assert (r["n_free"], r["half_bandwidth"]) == (nf, 0)       # nf listed blocks, all diagonal: 2, 1 and 2 modulo 3
    r = rep("dense12")
    assert r["n_free"] == 12 and r["half_bandwidth"] == 11
    r = rep("long_list")
    assert r["n_free"] == 2 and r["half_bandwidth"] == 1 and r["n_present"] == 300
    r = rep("chain40")
    assert r["n_free"] == 40 and 1 <= r["half_bandwidth"] <= 3
    r = rep("chain60_loop")
    assert r["n_free"] == 60 and 1 <= r["half_bandwidth"] <= 8     # (the loop is absorbed by the reordering, as at 260)
    r = rep("mixed")
    assert (r["n_free"], r["n_isolated"], r["n_thin"]) == (6, 1, 1)
    r = rep("rejected")
    assert r["rejected"] >= 1 and r["accepted"] <= 2
    prob, _, _, ref = case("outliers")
    assert ref["pair_wrong"].sum() >= prob["n_bad"] // 2


def test_edges_only_is_the_yaw_pose_graph_solve(capi):
    """(b) without landmarks the call runs the edge bodies of vslam_pose_graph_optimize_yaw"""
    prob, edges, _, ref = case("edges_only")
    got = run(capi, prob, edges)
    out, rep = capi.pose_graph_optimize_yaw(prob["kf_pose"], prob["kf_fixed"], edges, AXIS)
    print("difference", np.abs(got["kf_pose"] - out).max(), got["report"], rep)
    assert np.abs(got["kf_pose"] - out).max() <= 1e-12
    assert (got["report"]["accepted"], got["report"]["rejected"]) == (rep["accepted"], rep["rejected"])
    assert gy.gravity_error(got["kf_pose"], prob["kf_pose"], AXIS) <= 1e-12
    assert np.abs(got["kf_pose"] - ref["kf_pose"]).max() <= 1e-7


def test_all_fixed_equals_the_six_dof_call(capi):
    """(c) no keyframe parameter is left: only bodies shared with vslam_global_ba run"""
    prob, edges, _, _ = case("structure_only")
    got = run(capi, prob, edges)
    six = capi.global_ba(prob["rig"], gr.SIGMA, gr.INV_SIGMA, prob, edges)
    assert got["report"]["n_free"] == 0 and got["report"]["accepted"] >= 1
    assert same_bytes(got, six)


def test_yaw_and_translation_noise_is_removed(capi):
    """(d) keyframes disturbed by a yaw about g and a translation: the distance to the truth falls"""
    prob, edges = gy.yaw_noise()
    truth = np.asarray(prob["kf_pose_true"])
    got = run(capi, prob, edges)
    six = capi.global_ba(prob["rig"], gr.SIGMA, gr.INV_SIGMA, prob, edges)
    err = lambda P: float(np.abs(np.asarray(P) - truth).max())
    tilt = lambda P: gy.gravity_error(P, prob["kf_pose"], AXIS)
    print("error to the truth: start", err(prob["kf_pose"]), "yaw-only", err(got["kf_pose"]), "6-DoF", err(six["kf_pose"]),
          "| gravity error: yaw-only", tilt(got["kf_pose"]), "6-DoF", tilt(six["kf_pose"]), "|", got["report"])
    assert got["report"]["final_cost"] < got["report"]["initial_cost"]
    assert err(got["kf_pose"]) < err(prob["kf_pose"])
    assert tilt(got["kf_pose"]) <= 1e-12


AXES = [AXIS, (0.0, -9.81, 0.0), (-2.0, 0.5, 1.5)]


def test_batch_lanes_equal_their_single_calls(capi):
    """(f) three lanes with three axes and an idle lane between them; the lane order reversed"""
    names = ["mixed", "chain40", "no_shared4"]
    lanes = []
    for name, ax in zip(names, AXES):
        prob, edges, _, _ = case(name)
        lanes.append(dict(rig=prob["rig"], sigma_factor=gr.SIGMA, inv_sigma_factor=gr.INV_SIGMA, prob=prob, edges=edges, axis=ax))
    lanes.insert(1, None)
    single = [None if ln is None else run(capi, ln["prob"], ln["edges"], ln["axis"]) for ln in lanes]
    got = capi.global_ba_yaw_batch(lanes)
    back = capi.global_ba_yaw_batch(lanes[::-1])[::-1]
    assert got[1] is None and back[1] is None
    for g, ln in enumerate(lanes):
        if ln is None:
            continue
        assert same_bytes(got[g], single[g]), g
        assert same_bytes(back[g], single[g]), g
        assert gy.gravity_error(got[g]["kf_pose"], ln["prob"]["kf_pose"], ln["axis"]) <= 1e-12
    assert len({single[g]["report"]["iterations"] for g in (0, 2, 3)}) > 1          # the lanes stop in different rounds
    # another axis, another result
    assert not same_bytes(run(capi, lanes[0]["prob"], lanes[0]["edges"], AXES[1]), single[0])


def test_timers(capi):
    """(h)"""
    prob, edges, _, _ = case("dense12")
    capi.global_ba_set_timing(True)
    try:
        run(capi, prob, edges)
        t = capi.global_ba_timings()
    finally:
        capi.global_ba_set_timing(False)
    assert set(t) == {"gba_linearize", "gba_landmarks", "gba_assemble", "gba_band_chol", "gba_back", "gba_cost", "gba_chi2"}
    assert all(v >= 0 for v in t.values())


def refused(capi, status, prob, edges=None, text=None, axis=AXIS, **prm):
    with pytest.raises(capi.VslamError) as e:
        run(capi, prob, edges, axis, **prm)
    assert e.value.status == status, str(e.value)
    if text:
        assert text in str(e.value), str(e.value)


def test_refusals(capi):
    """(g) those of test_gpu_gba.py, and the axis"""
    prob, _, _, _ = case("one_free")
    mod = lambda **kw: dict({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in prob.items()}, **kw)
    INV = capi.ERR_INVALID
    refused(capi, INV, prob, axis=(0.0, 0.0, 0.0), text="axis")
    refused(capi, INV, prob, axis=(0.0, float("nan"), 1.0), text="axis")
    refused(capi, INV, prob, axis=(float("inf"), 0.0, 1.0), text="axis")
    refused(capi, INV, prob, max_iterations=-1)
    refused(capi, INV, prob, lambda0=-1.0)
    refused(capi, INV, prob, lambda0=float("nan"))
    refused(capi, INV, mod(kf_fixed=np.zeros(2, np.uint8)), text="free gauge")
    pk = prob["pair_kf"].copy(); pk[3] = 2
    refused(capi, INV, mod(pair_kf=pk), text="pair 3")
    pl = prob["pair_lm"].copy(); pl[5] = -1
    refused(capi, INV, mod(pair_lm=pl), text="pair 5")
    po = prob["pair_oct"].copy(); po[4, 1] = 8
    refused(capi, INV, mod(pair_oct=po), text="pair 4")
    lm = prob["lm"].copy(); lm[2, 2] = -1.0                  # behind both cameras: its first pair is 4
    refused(capi, INV, mod(lm=lm), text="pair 4 (keyframe 0, landmark 2)")
    lm = prob["lm"].copy(); lm[0, 0] = np.inf
    refused(capi, INV, mod(lm=lm))
    E = np.eye(4)
    refused(capi, INV, prob, [(1, 1, E, 1.0, 1.0)], text="edge 0")
    refused(capi, INV, prob, [(0, 2, E, 1.0, 1.0)], text="edge 0")
    refused(capi, INV, prob, [(0, 1, E, -1.0, 1.0)], text="edge 0")
    refused(capi, INV, prob, [(0, 1, E * np.nan, 1.0, 1.0)], text="edge 0")
    prob3 = mod(kf_pose=np.concatenate([prob["kf_pose"], prob["kf_pose"][1:] @ gr.look_z(0.3), prob["kf_pose"][1:] @ gr.look_z(0.6)]),
                kf_fixed=np.array([1, 0, 0, 0], np.uint8), kf_local=np.ones(4, np.uint8))
    refused(capi, INV, prob3, [(2, 3, gr.look_z(0.3), 1.0, 1.0)], text="free gauge")
    assert run(capi, prob3, [(2, 3, gr.look_z(0.3), 1.0, 1.0), (3, 0, gr.look_z(-1.0), 1.0, 1.0)])["report"]["n_free"] == 3


def test_nothing_is_written_on_refusal(capi):
    """a batched call whose LAST lane has a zero axis: the caller's arrays of every lane keep their bytes"""
    lanes, outs = [], []
    for name, ax in (("one_free", AXIS), ("two_free", (0.0, 0.0, 0.0))):
        prob, edges, _, _ = case(name)
        out = dict(kf_pose=np.full((len(prob["kf_pose"]), 4, 4), 7.0), lm=np.full((len(prob["lm"]), 3), 7.0), pair_wrong=np.full(len(prob["pair_kf"]), 7, np.uint8))
        outs.append(out)
        lanes.append(dict(rig=prob["rig"], sigma_factor=gr.SIGMA, inv_sigma_factor=gr.INV_SIGMA, prob=prob, edges=edges, axis=ax, out=out))
    with pytest.raises(capi.VslamError) as e:
        capi.global_ba_yaw_batch(lanes)
    assert e.value.status == capi.ERR_INVALID and "lane 1" in str(e.value) and "axis" in str(e.value)
    for out in outs:
        assert (out["kf_pose"] == 7.0).all() and (out["lm"] == 7.0).all() and (out["pair_wrong"] == 7).all()
    with pytest.raises(capi.VslamError) as e:
        capi.global_ba_yaw_batch([None] * 1025)
    assert e.value.status == capi.ERR_CAPACITY


def big(n_kf, n_lm, pk, pl, fixed0=True):
    fixed = np.zeros(n_kf, np.uint8)
    fixed[0] = fixed0
    P = len(pk)
    return dict(rig=gr.RIG, kf_pose=np.tile(np.eye(4), (n_kf, 1, 1)), kf_fixed=fixed, kf_local=np.ones(n_kf, np.uint8), lm=np.tile([0.0, 0.0, 3.0], (n_lm, 1)),
                pair_kf=np.asarray(pk, np.int32), pair_lm=np.asarray(pl, np.int32), pair_flags=np.full(P, 3, np.uint8),
                pair_uv=np.zeros((P, 4), np.float32), pair_oct=np.zeros((P, 2), np.int32))


def test_limits(capi):
    """VSLAM_ERR_CAPACITY at the 6-DoF call's limits, decided on the host before anything is sized or launched"""
    CAP = capi.ERR_CAPACITY
    refused(capi, CAP, big(16385, 1, [0, 1], [0, 0]), text="keyframes")
    refused(capi, CAP, big(2, 1048577, [0, 1], [0, 0]), text="landmarks")
    refused(capi, CAP, big(2, 1, np.zeros(2097153, np.int32), np.zeros(2097153, np.int32)), text="pairs")
    edges = np.zeros(262145, capi.PGO_EDGE_DTYPE)
    refused(capi, CAP, big(2, 1, [0, 1], [0, 0]), edges, text="edges")
    refused(capi, CAP, big(4098, 1, np.arange(4098), np.zeros(4098, np.int32)), text="block lists")
    refused(capi, CAP, big(601, 1, np.arange(601), np.zeros(601, np.int32)), text="band")
