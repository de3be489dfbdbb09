"""GPU tests of relocalisation mode 1 (vslam_reloc_params::mode = 1: hypotheses from 2D-3D correspondences) against its CPU
restatement (tests/reloc_p3p_ref.py), in the way tests/test_gpu_reloc.py pins mode 0: steps A - C' bit for bit through the test
tap, the refined pose to 1e-7.  Crafted frames go through set_keys + vslam_stereo_finalize_arrays; the stereo state is read back
and must equal the one the restatement was given.  Every crafted case advances its seed (at most 20) until the restatement keeps
every tested residual a relative 1e-6 from the chi2 bound and every discriminant of the solver a relative 1e-6 from zero
(reloc_p3p_cases.find_case; tests/test_reloc_p3p_ref.py checks without a GPU that every case has such a seed)."""
import numpy as np
import pytest
import synth
import reloc_cases as rc
import reloc_p3p_cases as pc
import reloc_p3p_ref as pp
import reloc_ref as rr
from test_gpu_reloc import load_frame, assert_steps_abc, rigid_inv

pytestmark = pytest.mark.gpu
RIG = rc.RIG
SENTINEL = 777.0
REL_INT = ("success", "n_points", "n_pairs", "best_hypothesis", "best_count", "n_inliers", "n_stereo")


@pytest.fixture(scope="module")
def inv_sigma(oracle):
    return oracle.Extractor(1500).InvSigmaFactor


@pytest.fixture(scope="module")
def crafted(capi):
    ge = capi.Extractor(RIG["w"], RIG["h"], 1500, batch=2)
    return capi.Matcher(RIG, ge, 0, ge, 1)


def load(m, g, st=None):
    got = load_frame(m, g["kL"], g["dL"], g["kR"], g["dR"], g["best"], g["depth"], g["sad"])
    if st is not None:
        for f in ("rightIdxs", "leftIdxs", "depth", "close"):
            assert np.array_equal(got[f], st[f]), f
    return got


def run_case(m, oracle, inv_sigma, **case):
    g, st, ref = pc.find_case(oracle, inv_sigma, **case)
    load(m, g, st)
    params = {k: v for k, v in case.items() if k not in ("C", "mode", "far")}
    T, rep, pairs = m.relocalize(g["points"], g["desc"], mode=1, **params)
    return g, st, ref, T, rep, pairs, m.relocalize_debug()


def assert_result(T, rep, ref):
    assert (rep["success"], rep["n_inliers"], rep["n_stereo"]) == (ref["success"], ref["n_inliers"], ref["n_stereo"])
    assert (T is None) == (ref["T_cw"] is None)
    if T is not None:
        assert np.abs(T - ref["T_cw"]).max() < 1e-7


@pytest.mark.parametrize("C", [2, 3, 4, 64, 65, 200])
def test_steps_equal_the_restatement(capi, oracle, inv_sigma, crafted, C):
    """40 % gross outliers, a quarter of the keys without a right match: every key is a correspondence"""
    g, st, ref, T, rep, pairs, dbg = run_case(crafted, oracle, inv_sigma, C=C)
    assert rep["n_pairs"] == C
    assert_steps_abc(dbg, rep, pairs, ref)
    assert_result(T, rep, ref)
    if C == 2:
        assert rep["success"] == 0 and rep["best_count"] == 0 and T is None and not dbg["counts"].any()
    if C >= 64:
        stereo = ref["rec"]["stereo"]
        assert stereo.any() and not stereo.all() and (st["rightIdxs"] < 0).sum() >= C // 8
        assert rep["best_count"] >= int(round(0.6 * C)) and dbg["flags"].sum() == rep["best_count"]
        assert dbg["flags"][~stereo].any()                   # correspondences without a right match are among the winner's inliers
    if C == 200:
        assert rep["success"] == 1 and np.abs(T - g["T_cw"]).max() < 1e-3
        assert 0 < rep["n_stereo"] < rep["n_inliers"]        # left-only factors went through the refinement


@pytest.mark.parametrize("H", [1, 1024])
def test_hypothesis_counts(capi, oracle, inv_sigma, crafted, H):
    g, st, ref, T, rep, pairs, dbg = run_case(crafted, oracle, inv_sigma, C=64, n_hypotheses=H)
    assert len(dbg["counts"]) == H
    assert_steps_abc(dbg, rep, pairs, ref)
    if H == 1024:
        assert (ref["hyp"]["slot"] >= 0).sum() > 512 and len(set(ref["hyp"]["slot"])) == 5      # void, and every slot wins somewhere


def test_collinear_points_void_every_hypothesis(capi, oracle, inv_sigma, crafted):
    g, st, ref, T, rep, pairs, dbg = run_case(crafted, oracle, inv_sigma, C=64, mode="collinear")
    assert_steps_abc(dbg, rep, pairs, ref)
    assert rep["n_pairs"] == 64 and not dbg["counts"].any() and rep["best_hypothesis"] == 0 and rep["best_count"] == 0
    assert rep["success"] == 0 and T is None and not dbg["flags"].any()


def test_points_behind_the_camera_do_not_count(capi, oracle, inv_sigma, crafted):
    """40 % of the pairs are points behind the camera whose every residual is zero under the true pose"""
    g, st, ref, T, rep, pairs, dbg = run_case(crafted, oracle, inv_sigma, C=65, mode="mirror")
    assert_steps_abc(dbg, rep, pairs, ref)
    rec = ref["rec"]
    R, t = g["T_cw"][:3, :3], g["T_cw"][:3, 3]
    behind = rec["Xw"] @ R[2] + t[2] < 0
    assert behind.sum() == 26 and rep["best_count"] == 39
    assert not dbg["flags"][behind].any() and dbg["flags"][~behind].all()
    _, val = pp.chi2_values(rec, R, t, RIG, inv_sigma)
    assert (val[behind] < 1e-3).all()


def test_far_scene_fails_in_mode_0_and_recovers_in_mode_1(capi, oracle, inv_sigma, crafted):
    """300 true pairs at 25 - 60 m, 0.25 px of noise on the right keys"""
    g, st, ref = pc.find_case(oracle, inv_sigma, far=True)
    load(crafted, g, st)
    T0, rep0, _ = crafted.relocalize(g["points"], g["desc"])
    ref0 = rr.relocalize(oracle, RIG, inv_sigma, g["points"], g["desc"], g["kL"], g["dL"], g["kR"], st)
    assert ref0["success"] == 0 and rep0["success"] == 0 and T0 is None and rep0["n_pairs"] == ref0["n_pairs"] == 297
    print("far scene, mode 0: best count %d of %d pairs (restatement %d)" % (rep0["best_count"], rep0["n_pairs"], ref0["best_count"]))
    load(crafted, g, st)
    T, rep, pairs = crafted.relocalize(g["points"], g["desc"], mode=1)
    assert_steps_abc(crafted.relocalize_debug(), rep, pairs, ref)
    assert rep["n_pairs"] == 300 and rep["best_count"] == 300
    assert rep["success"] == 1 and ref["success"] == 1 and np.abs(T - ref["T_cw"]).max() < 1e-7
    assert (rep["n_inliers"], rep["n_stereo"]) == (ref["n_inliers"], ref["n_stereo"])
    print("far scene, mode 1: %d inliers, %.3e from the true pose" % (rep["n_inliers"], np.abs(T - g["T_cw"]).max()))


def test_unknown_mode_is_refused(capi, crafted):
    g = pc.frame(8, 0.0, 1)
    load(crafted, g)
    for mode in (2, -1):
        with pytest.raises(capi.VslamError) as e:
            crafted.relocalize(g["points"], g["desc"], mode=mode)
        assert e.value.status == capi.ERR_INVALID
        with pytest.raises(capi.VslamError) as e:
            capi.relocalize_batch([crafted], [g["points"]], [g["desc"]], mode=mode)
        assert e.value.status == capi.ERR_INVALID


def test_batched_lanes_equal_their_single_calls(capi, oracle, inv_sigma):
    """vslam_relocalize_batch(mode = 1) over lanes of different C with an idle lane and a lane with fewer than three
    correspondences: every lane equals the restatement and its own single mode-1 call (same kernel bodies on the same problem,
    the pose kernel's sums are a fixed tree: 1e-12)"""
    cases = [dict(C=200), None, dict(C=2), dict(C=65, mode="mirror"), dict(C=64)]
    ge = capi.Extractor(RIG["w"], RIG["h"], 1500, batch=2 * len(cases))
    ms = [capi.Matcher(RIG, ge, 2 * b, ge, 2 * b + 1) for b in range(len(cases))]
    found = [pc.find_case(oracle, inv_sigma, **c) if c else None for c in cases]
    gs = [f[0] if f else pc.frame(8, 0.0, 1) for f in found]
    for m, g, f in zip(ms, gs, found):
        load(m, g, f[1] if f else None)
    T = np.full((len(cases), 4, 4), SENTINEL)
    _, reps, pairs = capi.relocalize_batch([m if c else None for m, c in zip(ms, cases)], [g["points"] for g in gs],
                                           [g["desc"] for g in gs], T_out=T, mode=1)
    assert reps[1] is None and pairs[1] is None and (T[1] == SENTINEL).all()
    assert [r["success"] if r else None for r in reps] == [1, None, 0, 0, 0]
    for b, c in enumerate(cases):
        if c is None:
            continue
        g, st, ref = found[b]
        dbg = ms[b].relocalize_debug()
        assert_steps_abc(dbg, reps[b], pairs[b], ref)
        assert (reps[b]["success"], reps[b]["n_inliers"], reps[b]["n_stereo"]) == (ref["success"], ref["n_inliers"], ref["n_stereo"])
        load(ms[b], g, st)                                   # (step D may have cleared stereo pairs)
        T1, rep1, pairs1 = ms[b].relocalize(g["points"], g["desc"], mode=1)
        for k in REL_INT:
            assert rep1[k] == reps[b][k], (b, k)
        assert rep1["lm"]["iterations"] == reps[b]["lm"]["iterations"]
        assert np.array_equal(pairs1, pairs[b])
        dbg1 = ms[b].relocalize_debug()
        for k in dbg:
            assert np.array_equal(dbg[k], dbg1[k]), (b, k)
        if rep1["success"]:
            assert np.abs(T1 - T[b]).max() < 1e-12 and np.abs(T[b] - ref["T_cw"]).max() < 1e-7
        else:
            assert T1 is None and (T[b] == SENTINEL).all()
    assert reps[2]["n_pairs"] == 2 and reps[2]["best_count"] == 0 and reps[2]["lm"]["iterations"] == 0


# ---- sessions ------------------------------------------------------------------------------------------------------------------
FRAMES = list(range(13))


def _foreign():
    return synth.stereo_frame(4, scene_seed=9, tex_seed=0xBEEF)[:2]


def test_session_relocalise_mode_1(capi, oracle):
    """tests/test_gpu_reloc.py::test_session_relocalise in mode 1: a refused call changes nothing, an accepted one commits as
    mode 0 does, tracking goes on"""
    import vo_system
    synth.prerender(FRAMES)
    T0 = synth.pose_at(0, RIG["fps"])
    ref = vo_system.System(RIG, 1500, T0=T0, local_mapping=True)
    got = capi.System(RIG, 1500, T0=T0, local_mapping=1)
    tracked = []
    for n in FRAMES:
        L, R, _ = synth.stereo_frame(n)
        ref.track(L, R, n)
        Pg, _ = got.track(L, R, n)
        tracked.append(Pg)
    before = got.counts()
    assert before["map_points"] == len(ref.mapPoints)
    Lf, Rf = _foreign()
    T, rrep = got.relocalize(Lf, Rf, 13, mode=1)
    assert rrep["success"] == 0 and np.array_equal(T, tracked[-1]) and got.counts() == before
    L, R, _ = synth.stereo_frame(3)
    T_wc, rrep = got.relocalize(L, R, 14, mode=1)
    mps = [mp for mp in ref.mapPoints if not mp.isOutlier]
    xyz = np.stack([mp.wp for mp in mps]); desc = np.stack([mp.desc for mp in mps])
    kL, dL = ref.exL.extract(L); kR, dR = ref.exR.extract(R)
    st = oracle.stereo_match(ref.exL, ref.exR, RIG, kL, dL, kR, dR)
    want = pp.relocalize(oracle, RIG, ref.invSigma, xyz, desc, kL, dL, kR, st, mode=1)
    want0 = rr.relocalize(oracle, RIG, ref.invSigma, xyz, desc, kL, dL, kR, st)
    assert want["success"] == 1 and rrep["success"] == 1
    assert want["n_pairs"] > want0["n_pairs"]                # the winners on keys without depth are correspondences now
    assert (rrep["n_points"], rrep["n_pairs"], rrep["n_inliers"], rrep["n_stereo"]) == (len(mps), want["n_pairs"], want["n_inliers"], want["n_stereo"])
    assert np.abs(T_wc - rigid_inv(want["T_cw"])).max() < 1e-7
    print("mode 1: %d pairs (mode 0: %d), %d inliers, %.3e from the tracked pose of frame 3"
          % (rrep["n_pairs"], want0["n_pairs"], rrep["n_inliers"], np.abs(T_wc - tracked[3]).max()))
    assert np.abs(T_wc - tracked[3]).max() < 0.02
    after = got.counts()
    assert after["keyframes"] == before["keyframes"] and after["map_points"] == before["map_points"] and after["frames"] == before["frames"] + 1
    assert len(got.last_frame()[0]) == 0
    for k, f in enumerate((4, 5)):
        L, R, T_true = synth.stereo_frame(f)
        P, rep = got.track(L, R, 15 + k)
        assert rep["n_inliers"] >= 50, (f, rep)
        assert np.abs(P - T_true).max() < 0.05
    got.close()


def test_batch_lanes_relocalise_mode_1(capi):
    """vslam_batch_relocalize(mode = 1): lane 0 on its own frame 3 (recovers), lane 1 on a foreign frame (refused, unchanged);
    each lane equals a session driven alone through the same calls, and tracks on"""
    synth.prerender(FRAMES)
    T0 = synth.pose_at(0, RIG["fps"])
    own = synth.stereo_frame(3)[:2]
    calls = [own, _foreign()]
    after = [4, 13]
    singles = []
    for b in range(2):
        s = capi.System(RIG, 1500, T0=T0, local_mapping=1)
        for n in FRAMES:
            L, R, _ = synth.stereo_frame(n)
            P, _ = s.track(L, R, n)
        T, rrep = s.relocalize(calls[b][0], calls[b][1], 13, mode=1)
        c, lf = s.counts(), s.last_frame()
        L, R, _ = synth.stereo_frame(after[b])
        P2, rep2 = s.track(L, R, 14)
        singles.append((T, rrep, c, lf, P, P2, rep2))
        s.close()
    bt = capi.Batch(RIG, 1500, 2, T0s=[T0, T0], local_mapping=1)
    for n in FRAMES:
        L, R, _ = synth.stereo_frame(n)
        Tt, _ = bt.track([L, L], [R, R], [n, n])
    last = Tt[1].copy()
    T, rreps = bt.relocalize([calls[0][0], calls[1][0]], [calls[0][1], calls[1][1]], [13, 13], mode=1)
    assert [r["success"] for r in rreps] == [1, 0]
    for b in range(2):
        T1, r1, c1, l1, P, P2, rep2 = singles[b]
        for k in REL_INT:
            assert r1[k] == rreps[b][k], (b, k)
        assert r1["lm"]["iterations"] == rreps[b]["lm"]["iterations"]
        assert np.abs(T1 - T[b]).max() <= 1e-9               # (the allowance of tests/test_gpu_batch_reloc.py: the local BA's summation order)
        assert bt.system(b).counts() == c1
        lf = bt.system(b).last_frame()
        assert np.array_equal(l1[0], lf[0]) and np.array_equal(l1[1], lf[1])
    assert np.array_equal(T[1], last)                        # the refused lane's row is its unchanged camera pose
    fr = [synth.stereo_frame(f) for f in after]
    T2, reps2 = bt.track([f[0] for f in fr], [f[1] for f in fr], [14, 14])
    for b in range(2):
        assert np.abs(T2[b] - singles[b][5]).max() <= 1e-9
        assert reps2[b]["n_inliers"] == singles[b][6]["n_inliers"] and reps2[b]["n_inliers"] >= 50
    bt.close()
