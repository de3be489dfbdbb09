"""The CPU restatement of relocalisation mode 1 (tests/reloc_p3p_ref.py) checked on its own, and the finding that motivates the
mode: with stereo depth of far points the stereo-triple hypotheses of mode 0 find a fraction of the
inliers the true pose has, the 2D-3D hypotheses find all of them."""
import numpy as np
import reloc_cases as rc
import reloc_p3p_cases as pc
import reloc_p3p_ref as pp
import reloc_ref as rr

RIG = rc.RIG
ONES = np.ones(8, np.float32)


def triple(rng, T, depth):
    R, t = T[:3, :3], T[:3, 3]
    u = rng.uniform(40, RIG["w"] - 40, 3); v = rng.uniform(40, RIG["h"] - 40, 3); z = rng.uniform(depth[0], depth[1], 3)
    Xc = np.stack([(u - RIG["cx"]) * z / RIG["fx"], (v - RIG["cy"]) * z / RIG["fy"], z], axis=1)
    return (Xc - t) @ R, Xc / np.linalg.norm(Xc, axis=1)[:, None]


def bearings_of(sol, Xw):
    Y = Xw @ sol[0].T + sol[1]
    return Y / np.linalg.norm(Y, axis=1)[:, None]


def test_solver_known_answers():
    rng = np.random.Generator(np.random.PCG64(1))
    counts = np.zeros(5, int)
    for T in (rc.true_pose(), rc.true_pose(11), np.eye(4)):
        for k in range(200):
            Xw, y = triple(rng, T, (25.0, 60.0) if k % 2 else (2.0, 8.0))
            sols, _ = pp.p3p(Xw, y)
            assert len(sols) == 4
            ok = [s for s in sols if s is not None]
            counts[len(ok)] += 1
            for s in ok:
                assert min(s[2]) > 0
                assert np.abs(bearings_of(s, Xw) - y).max() < 1e-9
                assert np.abs(s[0] @ s[0].T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(s[0]) - 1) < 1e-12
            assert min(max(np.abs(s[0] - T[:3, :3]).max(), np.abs(s[1] - T[:3, 3]).max()) for s in ok) < 1e-9
    assert counts[0] == 0 and counts[2:].sum() > 0          # (several solutions per triple do occur)


def test_void_triples():
    rng = np.random.Generator(np.random.PCG64(2))
    T = rc.true_pose()
    Xw, y = triple(rng, T, (2.0, 8.0))
    assert any(s is not None for s in pp.p3p(Xw, y)[0])
    line = np.outer([1.0, 2.0, 3.5], [0.3, -0.2, 0.9]) + np.array([0.5, 0.1, -0.4])
    assert pp.p3p(line, y)[0] == [None] * 4                                 # collinear world points
    assert pp.p3p(np.stack([Xw[0], Xw[0], Xw[2]]), y)[0] == [None] * 4      # coincident world points
    assert pp.p3p(Xw, np.stack([y[0], y[0], y[2]]))[0] == [None] * 4        # two equal bearings
    # A triple whose third point lies BEHIND the camera, on its key's ray extended backwards: the algebraic solutions (depths
    # of either sign) contain the planted one, no solution has three positive depths, so every slot is void.
    R, t = T[:3, :3], T[:3, 3]
    for seed in (0, 1, 4, 5, 7):
        g = np.random.Generator(np.random.PCG64(seed))
        u = g.uniform(40, RIG["w"] - 40, 3); v = g.uniform(40, RIG["h"] - 40, 3); z = g.uniform(2, 8, 3)
        y = np.stack([(u - RIG["cx"]) / RIG["fx"], (v - RIG["cy"]) / RIG["fy"], np.ones(3)], axis=1)
        y /= np.linalg.norm(y, axis=1)[:, None]
        lam = z / y[:, 2]; lam[2] = -lam[2]
        Xw = (lam[:, None] * y - t) @ R
        alg = [s for s in pp.p3p(Xw, y, keep_negative=True)[0] if s is not None]
        assert any(np.abs(np.abs(np.array(s[2], float)) - np.abs(lam)).max() < 1e-8 for s in alg)
        assert all(min(s[2]) < 0 for s in alg)
        assert pp.p3p(Xw, y)[0] == [None] * 4


def test_no_nan_reaches_a_count():
    """records of degenerate geometry - every world point on one line, or every key at one pixel - give void hypotheses and
    zero counts (a NaN pose would count every record: !(NaN > 7.815))"""
    f = pc.frame(64, 0.0, 5, mode="collinear")
    kw = np.arange(64, dtype=np.int32)
    rec = pp.pairs(kw, f["points"], f["kL"], f["kR"], f["depth"], f["best"], RIG)
    hyp = pp.hypotheses(rec, RIG, ONES, 64, 3)
    assert not hyp["counts"].any() and (hyp["slot"] == -1).all() and hyp["best"] == 0 and not hyp["flags"].any()
    f = pc.frame(64, 0.0, 6)
    f["kL"]["x"] = 300.0; f["kL"]["y"] = 200.0
    rec = pp.pairs(kw, f["points"], f["kL"], f["kR"], f["depth"], f["best"], RIG)
    hyp = pp.hypotheses(rec, RIG, ONES, 64, 3)
    assert not hyp["counts"].any() and (hyp["slot"] == -1).all()
    # and on an ordinary frame every stored pose is finite
    f = pc.frame(64, 0.4, 7)
    rec = pp.pairs(kw, f["points"], f["kL"], f["kR"], f["depth"], f["best"], RIG)
    for h in range(64):
        for s in pp.p3p(rec["Xw"][rr.sample(9, h, 64)], rec["y"][rr.sample(9, h, 64)])[0]:
            assert s is None or (np.isfinite(s[0]).all() and np.isfinite(s[1]).all())


def test_step_b_keeps_every_winning_pair():
    f = pc.frame(65, 0.4, 11)
    kw = np.arange(65, dtype=np.int32); kw[[3, 40]] = -1
    depth = f["depth"].copy(); depth[f["best"] < 0] = -1
    rec = pp.pairs(kw, f["points"], f["kL"], f["kR"], depth, f["best"], RIG)
    assert list(rec["i"]) == [i for i in range(65) if i not in (3, 40)]
    assert np.array_equal(rec["stereo"], f["best"][rec["i"]] >= 0) and rec["stereo"].any() and not rec["stereo"].all()
    assert (rec["kxr"][~rec["stereo"]] == 0).all() and np.array_equal(rec["kxr"][rec["stereo"]], f["kR"]["x"][f["best"][rec["i"]][rec["stereo"]]])
    assert np.abs(np.linalg.norm(rec["y"], axis=1) - 1).max() < 1e-15
    assert np.abs(rec["y"][:, 0] / rec["y"][:, 2] - (rec["kx"].astype(np.float64) - RIG["cx"]) / RIG["fx"]).max() < 1e-15
    # a record without the flag is scored on its two left rows: a wrong right key cannot push it out
    T = f["T_cw"]
    good = np.ones(63, bool); good[np.isin(rec["i"], f["bad"])] = False
    assert np.array_equal(pp.inliers(rec, T[:3, :3], T[:3, 3], RIG, ONES), good)


def test_far_scene_stereo_triples_fail_and_p3p_finds_every_inlier():
    """The finding: 300 true pairs at 25 - 60 m, 0.25 px of noise on the right keys, left keys exact."""
    g = pc.far_scene()
    T = g["T_cw"]
    assert len(g["rec0"]["i"]) == 300 and rr.inliers(g["rec0"], T[:3, :3], T[:3, 3], RIG, ONES).sum() == 300
    h0 = rr.hypotheses(g["rec0"], RIG, ONES, 256, rr.DEFAULTS["seed"])
    h1 = pp.hypotheses(g["rec1"], RIG, ONES, 256, rr.DEFAULTS["seed"])
    print("far scene: best count of mode 0 %d, of mode 1 %d (of 300)" % (h0["best_count"], h1["best_count"]))
    assert h0["best_count"] < 50
    assert h1["best_count"] == 300
    assert np.abs(h1["T_cw"] - T).max() < 1e-4          # (keys are floats: 3e-5 px at 25 - 60 m)


def test_far_scene_with_noise_on_the_left_keys_too():
    """0.25 px on the left keys as well (a key whose noisy disparity is not positive has no right match: one of the 300).
    The restatement gives 13 of 299 in mode 0 and 300 of 300 in mode 1; the winning hypothesis is 0.10 away from the true pose
    before the refinement."""
    g = pc.far_scene(sigma_l=0.25)
    h0 = rr.hypotheses(g["rec0"], RIG, ONES, 256, rr.DEFAULTS["seed"])
    h1 = pp.hypotheses(g["rec1"], RIG, ONES, 256, rr.DEFAULTS["seed"])
    print("far scene, noisy left keys: mode 0 %d of %d, mode 1 %d of 300" % (h0["best_count"], len(g["rec0"]["i"]), h1["best_count"]))
    assert (len(g["rec0"]["i"]), h0["best_count"]) == (299, 13)
    assert h1["best_count"] == 300


def test_frame_without_right_matches(oracle):
    g = pc.far_scene(right=False)
    st = oracle.stereo_finalize(g["best"], g["depth"], g["sad"], len(g["kR"]), RIG)
    assert (st["rightIdxs"] < 0).all()
    args = (oracle, RIG, ONES, g["points"], g["desc"], g["kL"], g["dL"], g["kR"], st)
    r0 = rr.relocalize(*args)
    assert r0["n_pairs"] == 0 and r0["success"] == 0 and r0["T_cw"] is None
    r1 = pp.relocalize(*args, mode=1)
    assert r1["n_pairs"] == 300 and r1["best_count"] == 300 and not r1["rec"]["stereo"].any()
    assert r1["success"] == 1 and r1["n_inliers"] == 300 and r1["n_stereo"] == 0
    print("no right matches: refined pose differs from the true one by %.3e" % np.abs(r1["T_cw"] - g["T_cw"]).max())
    assert np.abs(r1["T_cw"] - g["T_cw"]).max() < 1e-3      # (the bound of the crafted frames in tests/test_gpu_reloc.py)


def test_forty_percent_outliers():
    f = pc.frame(200, 0.4, 21)
    rec = pp.pairs(np.arange(200, dtype=np.int32), f["points"], f["kL"], f["kR"], f["depth"], f["best"], RIG)
    hyp = pp.hypotheses(rec, RIG, ONES, 256, rr.DEFAULTS["seed"])
    good = np.ones(200, bool); good[f["bad"]] = False
    assert hyp["best_count"] >= good.sum() and np.array_equal(hyp["flags"].astype(bool) & good, good)
    assert hyp["best"] == int(np.nonzero(hyp["counts"] == hyp["counts"].max())[0][0])
    assert hyp["slot"][hyp["best"]] >= 0 and (hyp["counts"][hyp["slot"] < 0] == 0).all()


def test_every_gpu_case_finds_its_seed(oracle):
    """the seed-advance rule of tests/test_gpu_reloc_p3p.py, checked without a GPU: every case has a seed among its 20"""
    inv_sigma = oracle.Extractor(1500).InvSigmaFactor
    for case in pc.GPU_CASES:
        g, st, ref = pc.find_case(oracle, inv_sigma, **case)
        assert ref["hyp"]["margin"] > pc.MARGIN
