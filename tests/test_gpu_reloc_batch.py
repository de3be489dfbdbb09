"""GPU tests of the batched relocalisation stage (vslam_relocalize_batch): several matchers ("lanes") in one call, one launch per
stage for all of them.  A lane's result is DEFINED as what vslam_relocalize returns for that matcher, so the yardstick is the one of
tests/test_gpu_reloc.py - the CPU restatement (tests/reloc_ref.py) per lane, compared exactly as assert_steps_abc does there: d,
key_winner, pairs, counts, winner and flags bit for bit through the test tap, report integers equal, refined pose to 1e-7.  The
lanes' matchers sit on images 2b / 2b + 1 of ONE extractor, as the lanes of a vslam_batch do; the frames are crafted (set_keys +
vslam_stereo_finalize_arrays), so the extractor never runs."""
import numpy as np
import pytest
import synth
import reloc_cases as rc
import reloc_ref as rr
from test_gpu_reloc import matching_scene, load_frame, assert_steps_abc

pytestmark = pytest.mark.gpu
RIG = rc.RIG
# the second camera (tests/test_gpu_batch_lanes.py's): other focal length, principal point and baseline
RIG_B = dict(RIG, fx=458.0, fy=458.0, cx=360.0, cy=248.0, bl=0.16)
SENTINEL = 777.0


def make_lanes(capi, rigs):
    ge = capi.Extractor(RIG["w"], RIG["h"], 1500, batch=2 * len(rigs))
    return [capi.Matcher(rig, ge, 2 * b, ge, 2 * b + 1) for b, rig in enumerate(rigs)]


@pytest.fixture(scope="module")
def inv_sigma(oracle):
    return oracle.Extractor(1500).InvSigmaFactor


def load(m, g):
    return load_frame(m, g["kL"], g["dL"], g["kR"], g["dR"], g["best"], g["depth"], g["sad"])


def hypothesis_frame(oracle, inv_sigma, rig, C, mode="pose", **params):
    """tests/test_gpu_reloc.py's hypothesis_case for a given rig, without the call: a crafted frame whose restatement keeps every
    tested residual a relative 1e-6 away from the chi2 bound (the seed is advanced until that holds)"""
    for seed in range(100 * C, 100 * C + 20):
        g = rc.frame_for_records(C, 0.4, seed, rig=rig, mode=mode)
        st = oracle.stereo_finalize(g["best"], g["depth"], g["sad"], len(g["kR"]), rig)
        ref = rr.relocalize(oracle, rig, inv_sigma, g["points"], g["desc"], g["kL"], g["dL"], g["kR"], st, **params)
        if ref["hyp"]["margin"] > 1e-6:
            break
    assert ref["hyp"]["margin"] > 1e-6 and ref["n_pairs"] == C
    return g, st, ref


def assert_lane(m, rep, pairs, T_row, ref, counts=True):
    """one lane of a batched call against its restatement"""
    assert_steps_abc(m.relocalize_debug(), rep, pairs, ref, counts=counts)
    assert (rep["success"], rep["n_inliers"], rep["n_stereo"]) == (ref["success"], ref["n_inliers"], ref["n_stereo"])
    if "refined" in ref:
        assert rep["lm"]["iterations"] == ref["refined"]["iterations"]
    else:
        assert rep["lm"]["iterations"] == 0
    if ref["success"]:
        assert np.abs(T_row - ref["T_cw"]).max() < 1e-7
    else:
        assert (T_row == SENTINEL).all()                       # a failed lane's row is not written


def test_mixed_shapes_in_one_call(capi, oracle, inv_sigma):
    """no points, no keys, one of each, sizes on both sides of the 256-point workgroup and of the 2048-key tile, and an idle lane
    between them: every lane equals its restatement, the idle lane's matcher keeps its state"""
    shapes = [(0, 2049), (300, 0), (1, 1), None, (257, 2047), (300, 2049)]
    ms = make_lanes(capi, [RIG] * len(shapes))
    scenes, sts = [None] * len(shapes), [None] * len(shapes)
    for b, sh in enumerate(shapes):
        g = matching_scene(*(sh if sh else (40, 60)), 7000 + b)
        scenes[b] = g
        sts[b] = load(ms[b], g)
    idle = shapes.index(None)
    ms[idle].relocalize(scenes[idle]["points"], scenes[idle]["desc"], n_hypotheses=4)      # the state an idle lane must keep
    dbg0 = ms[idle].relocalize_debug()
    T = np.full((len(shapes), 4, 4), SENTINEL)
    _, reps, pairs = capi.relocalize_batch([m if sh else None for m, sh in zip(ms, shapes)], [g["points"] for g in scenes],
                                           [g["desc"] for g in scenes], T_out=T, n_hypotheses=4)
    for b, sh in enumerate(shapes):
        if sh is None:
            continue
        g = scenes[b]
        ref = rr.relocalize(oracle, RIG, inv_sigma, g["points"], g["desc"], g["kL"], g["dL"], g["kR"], sts[b], n_hypotheses=4)
        assert (reps[b]["n_points"], len(ms[b].relocalize_debug()["key_winner"])) == sh
        assert_lane(ms[b], reps[b], pairs[b], T[b], ref, counts=False)
        assert reps[b]["success"] == 0                          # random world points: nothing to recover
    assert reps[idle] is None and pairs[idle] is None and (T[idle] == SENTINEL).all()
    dbg1 = ms[idle].relocalize_debug()
    for k in dbg0:
        assert np.array_equal(dbg0[k], dbg1[k]), k
    st1 = ms[idle].stereo_fetch(len(scenes[idle]["kL"]), len(scenes[idle]["kR"]))
    for f in ("rightIdxs", "leftIdxs", "depth", "close"):
        assert np.array_equal(st1[f], sts[idle][f]), f


def test_mixed_outcomes_in_one_call(capi, oracle, inv_sigma):
    """one call whose lanes end in every way the stage can: never refined (C = 2), refined and refused (C = 3, C = 65 with the
    points behind the camera), every hypothesis void (collinear), recovered (C = 200); two cameras among the lanes"""
    cases = [(2, "pose", RIG), (3, "pose", RIG_B), (65, "mirror", RIG), (64, "collinear", RIG_B), (200, "pose", RIG_B)]
    ms = make_lanes(capi, [c[2] for c in cases])
    gs, refs = [], []
    for m, (C, mode, rig) in zip(ms, cases):
        g, st, ref = hypothesis_frame(oracle, inv_sigma, rig, C, mode)
        got = load(m, g)
        for f in ("rightIdxs", "leftIdxs", "depth", "close"):
            assert np.array_equal(got[f], st[f])
        gs.append(g); refs.append(ref)
    T = np.full((len(cases), 4, 4), SENTINEL)
    _, reps, pairs = capi.relocalize_batch(ms, [g["points"] for g in gs], [g["desc"] for g in gs], T_out=T)
    for b, (C, mode, rig) in enumerate(cases):
        assert_lane(ms[b], reps[b], pairs[b], T[b], refs[b])
    assert [r["success"] for r in reps] == [0, 0, 0, 0, 1]
    assert reps[0]["best_count"] == 0 and reps[0]["lm"]["iterations"] == 0          # C = 2: the failure report, no refinement
    assert "refined" in refs[1] and "refined" in refs[2]                            # C = 3 and the mirror lane were refined, and refused
    assert reps[2]["best_count"] == 39
    assert reps[3]["n_pairs"] == 64 and reps[3]["best_count"] == 0 and not ms[3].relocalize_debug()["counts"].any()
    assert np.abs(T[4] - gs[4]["T_cw"]).max() < 1e-3
    # the recovered lane against vslam_relocalize on the same matcher and frame (reloaded: step D may have cleared stereo pairs).
    # Same kernel bodies on the same problem, and the pose kernel's sums are a fixed tree: 1e-12.
    load(ms[4], gs[4])
    T1, rep1, pairs1 = ms[4].relocalize(gs[4]["points"], gs[4]["desc"])
    assert T1 is not None and np.abs(T[4] - T1).max() < 1e-12
    assert np.array_equal(pairs1, pairs[4])
    for k in ("success", "n_points", "n_pairs", "best_hypothesis", "best_count", "n_inliers", "n_stereo"):
        assert rep1[k] == reps[4][k], k
    for k in ("iterations", "inner"):
        assert rep1["lm"][k] == reps[4]["lm"][k], k
    for k in ("initialError", "finalError", "lam"):
        assert abs(rep1["lm"][k] - reps[4]["lm"][k]) <= 1e-12 * max(1.0, abs(rep1["lm"][k])), k


@pytest.mark.parametrize("H", [1, 1024])
def test_hypothesis_counts_two_lanes(capi, oracle, inv_sigma, H):
    rigs = [RIG, RIG_B]
    ms = make_lanes(capi, rigs)
    gs, refs = [], []
    for m, rig in zip(ms, rigs):
        g, st, ref = hypothesis_frame(oracle, inv_sigma, rig, 64, n_hypotheses=H)
        load(m, g)
        gs.append(g); refs.append(ref)
    T = np.full((2, 4, 4), SENTINEL)
    _, reps, pairs = capi.relocalize_batch(ms, [g["points"] for g in gs], [g["desc"] for g in gs], T_out=T, n_hypotheses=H)
    for b in range(2):
        assert len(ms[b].relocalize_debug()["counts"]) == H
        assert_lane(ms[b], reps[b], pairs[b], T[b], refs[b])


def test_argument_errors_leave_the_other_lanes_alone(capi):
    ms = make_lanes(capi, [RIG, RIG, RIG])
    gs = [matching_scene(20, 30, 9100 + b) for b in range(2)]
    for m, g in zip(ms, gs):
        load(m, g)
    capi.relocalize_batch(ms[:2], [g["points"] for g in gs], [g["desc"] for g in gs], n_hypotheses=4)
    before = [m.relocalize_debug() for m in ms[:2]]

    def unchanged():
        for m, d0 in zip(ms[:2], before):
            d1 = m.relocalize_debug()
            for k in d0:
                assert np.array_equal(d0[k], d1[k]), k

    with pytest.raises(capi.VslamError) as e:
        capi.relocalize_batch(ms[:2], [gs[0]["points"], np.zeros((65537, 3))], [gs[0]["desc"], np.zeros((65537, 32), np.uint8)])
    assert e.value.status == capi.ERR_CAPACITY and "lane 1" in str(e.value)
    unchanged()
    with pytest.raises(capi.VslamError) as e:      # ms[2]: no completed stereo match
        capi.relocalize_batch([ms[0], ms[2]], [g["points"] for g in gs], [g["desc"] for g in gs])
    assert e.value.status == capi.ERR_INVALID and "lane 1" in str(e.value)
    unchanged()
    with pytest.raises(capi.VslamError) as e:
        capi.relocalize_batch(ms[:2], [g["points"] for g in gs], [g["desc"] for g in gs], n_hypotheses=1025)
    assert e.value.status == capi.ERR_INVALID
    unchanged()
