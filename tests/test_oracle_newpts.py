"""CPU checks of the oracle's new-point restatement (no GPU): DLT triangulation against ground truth and the
rank / degenerate cases of gtsam::triangulatePoint3 (GTSAM 4.2 triangulation.cpp), calcDescriptor's median rule."""
import copy
import numpy as np
import pytest
import synth
import newpts_cases as nc


def _P(K, T_wc):
    Tcw = np.linalg.inv(T_wc)
    return K @ Tcw[:3, :]


def test_dlt_recovers_point_and_detects_degeneracy(oracle):
    rig = synth.RIGS["euroc"]
    K = np.array([[rig["fx"], 0, rig["cx"]], [0, rig["fy"], rig["cy"]], [0, 0, 1.0]])
    rng = np.random.default_rng(0)
    X = np.array([0.4, -0.2, 5.0])
    Ps, uv = [], []
    for i in range(5):
        T = np.eye(4); T[:3, 3] = [0.3 * i, 0.05 * i, 0.0]
        P = _P(K, T); x = P @ np.append(X, 1.0)
        Ps.append(P.ravel()); uv.append(x[:2] / x[2])
    ok, p = oracle.triangulate_dlt(Ps, uv)
    assert ok and np.abs(p - X).max() < 1e-9
    # noisy observations: the algebraic solution stays close
    uvn = [u + rng.normal(0, 0.3, 2) for u in uv]
    ok, p = oracle.triangulate_dlt(Ps, uvn)
    assert ok and np.abs(p - X).max() < 0.2
    # the same camera twice: rank 2 -> underconstrained
    ok, _ = oracle.triangulate_dlt([Ps[0], Ps[0]], [uv[0], uv[0]])
    assert not ok


def test_calc_descriptor_median_rule(oracle):
    rng = np.random.default_rng(1)
    d = rng.integers(0, 256, (7, 32), dtype=np.uint8)
    dist = np.array([[int(np.unpackbits(a ^ b).sum()) for b in d] for a in d])
    med = [sorted(row)[int(0.5 * (len(d) - 1))] for row in dist]
    assert oracle.calc_descriptor(d) == int(np.argmin(med))
    assert oracle.calc_descriptor(d[:1]) == 0


def test_mono_map_point_creation_quirks_and_sanity(oracle):
    """calculateMPFromMono + the mono checkReprojError (src/FeatureTracker.cpp:1580-1684) as restated: needs >= 2 views,
    rejects world z < 0.1, and its reprojection check multiplies with KeyFrame::pose.pose (camera-to-world), so with the
    centimetre baselines of mono initialisation it acts as a loose gate; accepted points sit near the truth."""
    import synth
    pr = synth.make_mono_points_problem()
    sf = np.array([1.2 ** (2 * i) for i in range(8)], np.float32)
    r = oracle.mono_new_points(pr["rig"], sf, pr["kf_pose"], pr["kf_id"], pr["n_views"], pr["view_kf"], pr["view_xy"], pr["view_oct"])
    acc = r["accepted"].astype(bool)
    assert 40 < acc.sum() < len(acc)
    assert not acc[pr["n_views"] < 2].any()                       # minNumberOfKFsForMp
    assert not acc[r["xyz"][:, 2] < 0.1].any()                    # the world-z test
    assert (r["nObs"][acc] >= 2).all() and (r["keep"][acc, 0] == 1).all()      # lastKF must survive the filter
    assert (r["keep"].sum(1)[acc] == r["nObs"][acc]).all()
    # triangulation quality of accepted points whose every view was an inlier: depth is weakly observed at these
    # baselines, the bearing is not
    ok = acc & (r["nObs"] == pr["n_views"])
    b_est = r["xyz"][ok] / np.linalg.norm(r["xyz"][ok], axis=1, keepdims=True)
    b_tru = pr["truth"][ok] / np.linalg.norm(pr["truth"][ok], axis=1, keepdims=True)
    assert np.median(np.arccos(np.clip((b_est * b_tru).sum(1), -1, 1))) < 2e-3
    # a single view or an empty row is never triangulated
    r1 = oracle.mono_new_points(pr["rig"], sf, pr["kf_pose"], pr["kf_id"], np.minimum(pr["n_views"], 1), pr["view_kf"], pr["view_xy"], pr["view_oct"])
    assert r1["accepted"].sum() == 0


def _kf_update_args(mod, pr):
    def kp(t):
        k = np.zeros(len(t[0]), mod.KP_DTYPE)
        k["x"], k["y"], k["octave"] = t
        return k
    isf = np.array([1.0 / 1.2 ** (2 * i) for i in range(8)], np.float32)
    return (pr["rig"], isf, pr["numb"], pr["key_pose"], pr["ref_pose"], pr["cur_pose_inv"], kp(pr["kL"]), kp(pr["kR"]),
            pr["slotL"], pr["slotR"], pr["lm"], pr["kdx"], pr["outlier"])


def test_keyframe_update_pose_semantics(oracle):
    """KeyFrame::updatePose (src/KeyFrame.cpp:6-76): own landmarks keep their camera-frame coordinates under the new
    pose, older ones are only gated, newer ones / outliers / empty slots are untouched; a zero correction drops nothing
    but noise outliers, a large one drops many."""
    import synth
    pr = synth.make_kf_update_problem()
    r = oracle.keyframe_update_pose(*_kf_update_args(oracle, pr))
    newPose = pr["key_pose"] @ pr["ref_pose"]
    assert np.abs(r["pose"] - newPose).max() < 1e-12
    own = np.zeros(len(pr["lm"]), bool)
    own[pr["slotL"][pr["slotL"] >= 0]] = True
    own &= (pr["kdx"] == pr["numb"]) & (pr["outlier"] == 0)
    h = lambda X: np.c_[X, np.ones(len(X))]
    before = (pr["cur_pose_inv"] @ h(pr["lm"][own]).T).T[:, :3]
    after = (np.linalg.inv(newPose) @ h(r["lm"][own]).T).T[:, :3]
    assert own.sum() > 100 and np.abs(before - after).max() < 1e-9
    assert np.array_equal(r["lm"][~own], pr["lm"][~own])
    older = lambda slot: (slot >= 0) & (pr["kdx"][np.maximum(slot, 0)] < pr["numb"]) & (pr["outlier"][np.maximum(slot, 0)] == 0)
    assert not r["dropL"][~older(pr["slotL"])].any() and not r["dropR"][~older(pr["slotR"])].any()
    assert 0 < r["dropL"].sum() < older(pr["slotL"]).sum() and 0 < r["dropR"].sum() < older(pr["slotR"]).sum()
    big = synth.make_kf_update_problem(shift=0.5)
    rb = oracle.keyframe_update_pose(*_kf_update_args(oracle, big))
    assert rb["dropL"].sum() > 2 * r["dropL"].sum()


# ---- crafted windows of the new-point search (tests/newpts_cases.py): every case is in the regime it is named after ------------
_SIDE = {"L": "left", "R": "right"}


def _check_probe(c, name):
    """the restatement's view of the probe's pair against what the case says it built"""
    p = c.probes[name]
    if p["kf"] is None:
        return
    pr, ex = c.pairs[p["cand"]][p["kf"]], p["expect"]
    assert pr["verdict"] == ex["verdict"], (c.name, name, pr["verdict"])
    for f in ("hasL", "hasR", "predScale", "out"):
        if f in ex:
            assert pr[f] == ex[f], (c.name, name, f, pr[f])
    if "q_le" in ex:
        assert pr["q"] <= ex["q_le"], (c.name, name, pr["q"])
    if "q_gt" in ex:
        assert pr["q"] > ex["q_gt"], (c.name, name, pr["q"])
    if "side" in ex:
        assert pr["side"] == _SIDE[ex["side"]], (c.name, name)
    if "side" in pr:
        S = pr[pr["side"]]
        if "best" in ex:
            assert S["best"] is not None and S["best"][3] == ex["best"], (c.name, name, S["best"])
        if "sec_level" in ex:
            assert S["sec"] is not None and S["sec"][1] == ex["sec_level"], (c.name, name, S["sec"])
        if "sec_dist" in ex:
            assert (S["sec"][0] if S["sec"] else None) == ex["sec_dist"], (c.name, name, S["sec"])
        if ex.get("clamped"):
            assert ex["best"] in S["clamped"], (c.name, name)
    if ex["verdict"].startswith("matched"):
        assert (p["kf"],) + pr["out"] in c.raw[p["cand"]]


def _check_oracle(oracle, c):
    """the oracle's candidates and raw matches are the restatement's; finals as constructed"""
    rig, kfs, last = c.g.rig, c.kfs, c.last
    ref = oracle.find_new_points(c.ex, rig, kfs, last)
    assert ref["n"] == len(c.cands)
    assert list(ref["candL"]) == [cd["key"] for cd in c.cands] and list(ref["candR"]) == [cd["keyR"] for cd in c.cands]
    for ci, raw in enumerate(c.raw):
        if len(raw) < 3:                                   # below minCount: untouched, the rows are the raw matches
            assert ref["nObs"][ci] == len(raw) and ref["accepted"][ci] == 0, (c.name, ci)
            assert ref["obs"][ci][:len(raw)].tolist() == [list(r) for r in raw], (c.name, ci)
    # the matches before the filter, keyframe by keyframe: a window of two keyframes never triangulates
    for k in range(1, len(kfs)):
        sub = oracle.find_new_points(c.ex, rig, [kfs[0], kfs[k]], last)
        assert sub["n"] == len(c.cands)
        for ci, raw in enumerate(c.raw):
            mine = [list(r[1:]) for r in raw if r[0] == k]
            got = [sub["obs"][ci][1][1:].tolist()] if sub["nObs"][ci] == 2 else []
            assert got == mine, (c.name, ci, k, got, mine)
    for name, f in c.finals.items():
        ci = c.probes[name]["cand"]
        assert ref["accepted"][ci] == f["accepted"] and ref["nObs"][ci] == f["nObs"], (c.name, name, ref["accepted"][ci], ref["nObs"][ci], ref["obs"][ci])
        assert ref["obs"][ci][:f["nObs"]].tolist() == nc.expected_final(c, name), (c.name, name, ref["obs"][ci])
        if "kfs" in f:
            assert [r[0] for r in ref["obs"][ci][:f["nObs"]].tolist()] == f["kfs"]
        if "rows" in f:
            assert 2 * sum((l >= 0) + (r >= 0) for _, l, r in c.raw[ci]) == f["rows"]
    assert int(ref["accepted"].sum()) >= c.min_accepted and int((ref["accepted"] == 0).sum()) >= c.min_rejected
    return ref


@pytest.mark.parametrize("rig_name", nc.RIG_NAMES)
@pytest.mark.parametrize("name", list(nc.ALL_CASES))
def test_crafted_window_is_in_its_regime(oracle, name, rig_name):
    c = nc.get(oracle, name, rig_name)
    for pn in c.probes:
        _check_probe(c, pn)
    _check_oracle(oracle, c)
    verdicts = {c.pairs[p["cand"]][p["kf"]]["verdict"] for p in c.probes.values() if p["kf"] is not None}
    if name in nc.MATCH_CASES:
        assert c.min_accepted == 10                              # the fillers triangulate
        assert len(verdicts) >= 2 or name == "pred_scale"        # both outcomes present
    if name == "pred_scale":
        assert {c.pairs[p["cand"]][1]["predScale"] for p in c.probes.values() if p["expect"]} == {0, 1, 3, 4, 7}
    # what the case is named after
    if name == "second_level_rule":
        assert sum(p["expect"]["verdict"] == "ratio" for p in c.probes.values() if p["expect"]) >= 6
        assert sum(p["expect"]["verdict"] == "matched-right" for p in c.probes.values() if p["expect"]) >= 8
    if name == "thresholds":
        rej = {pn: p["expect"]["verdict"] == "ratio" for pn, p in c.probes.items() if pn.startswith("ratio_")}
        assert any(rej.values()) and not all(rej.values())
    if name == "row_counts":
        assert sorted(f["rows"] for f in c.finals.values() if "rows" in f) == list(range(6, 65, 2))
        assert [c.probes["rows_%d" % r]["cand"] for r in range(6, 65, 2)] == list(range(30))     # neighbours in one 64-thread group
    if name.startswith("chunk_"):
        n_last, n_cand = (int(x) for x in name.split("_")[1:])
        assert len(c.kfs[0]["kpsL"]) == n_last and len(c.cands) == n_cand
        keys = [cd["key"] for cd in c.cands]
        assert keys[0] == 0 and keys[-1] == n_last - 1 and (n_last <= 1024 or 1024 in keys)
        kinds = [(int(c.last["hasMp"][i]), bool(c.last["depth"][i] > 0), bool(c.kfs[0]["unF"][i] >= 0)) for i in range(n_last)]
        assert {(0, True), (1, False)} <= {(h, d) for h, d, u in kinds if (h and not u) or (not h and d)}       # both kept kinds
        assert any(h == 0 and not d for h, d, u in kinds) and any(h == 1 and u for h, d, u in kinds)          # both rejected kinds
    if name == "skip_mid":
        assert c.kfs[2]["id"] == c.kfs[0]["id"] and all(c.pairs[ci][2]["verdict"] == "skip" for ci in range(len(c.cands)))
    if name == "single_kf":
        assert len(c.kfs) == 1 and len(c.cands) == 10
    if name == "no_candidates":
        assert len(c.kfs[0]["kpsL"]) > 0 and len(c.cands) == 0
    if name == "empty_last":
        assert len(c.kfs[0]["kpsL"]) == 0 and len(c.cands) == 0


def _dlt(oracle, c, ci):
    """oracle.triangulate_dlt on the candidate's raw observations -> (ok, point, depths in its cameras)"""
    rig = c.g.rig
    K = np.array([[rig["fx"], 0, rig["cx"]], [0, rig["fy"], rig["cy"]], [0, 0, 1.0]])
    Ps, uv, Ts = [], [], []
    for k, l, r in c.raw[ci]:
        for side, idx in ((0, l), (1, r)):
            if idx < 0:
                continue
            T = np.linalg.inv(c.kfs[k]["T_wc"])[:3, :].copy()
            if side:
                T[0, 3] -= c.g.b
            kp = (c.kfs[k]["kpsR"] if side else c.kfs[k]["kpsL"])[idx]
            Ps.append((K @ T).ravel()); uv.append([float(kp["x"]), float(kp["y"])]); Ts.append(T)
    ok, pt = oracle.triangulate_dlt(Ps, uv)
    return ok, pt, [float(T[2, :3] @ pt + T[2, 3]) for T in Ts]


@pytest.mark.parametrize("rig_name", nc.RIG_NAMES)
def test_rank_deficient_and_cheirality_are_reached(oracle, rig_name):
    c = nc.get(oracle, "rank_deficient", rig_name)
    for name, f in c.finals.items():
        if f.get("rank_deficient"):
            ci = c.probes[name]["cand"]
            assert len(c.raw[ci]) == f["nObs"] >= 3 and all(r < 0 for _, _, r in c.raw[ci][1:])
            assert len({c.kfs[k]["id"] for k, _, _ in c.raw[ci]}) == f["nObs"]                   # different keyframes ...
            assert all(np.array_equal(c.kfs[k]["T_wc"], c.kfs[0]["T_wc"]) for k, _, _ in c.raw[ci])      # ... one camera
            assert not _dlt(oracle, c, ci)[0]
    c = nc.get(oracle, "cheirality", rig_name)
    n = 0
    for name, f in c.finals.items():
        if f.get("behind"):
            ok, pt, depths = _dlt(oracle, c, c.probes[name]["cand"])
            assert ok and min(depths) < -0.05, (name, depths)
            n += 1
    assert n == 2


# probes of the high rows whose outcome the former 12-bit cell field (dist | 1, visit position cell & 4095) must change
_PORTRAIT_FLIPS = dict(thresholds={"d50": "dist>50", "d50_right": "dist>50", "ratio_30_50": "ratio"},
                       second_level_rule={"L_col_after": "matched-left", "L_row_after": "matched-left", "L_rowcol_after": "matched-left",
                                          "L_idx_after": "matched-left", "L_straddle_63_64": "matched-left"},
                       left_right_choice={"right_by_one_even": "ratio"})


@pytest.mark.parametrize("name", list(nc.PORTRAIT_CASES))
def test_portrait_cases_reach_grid_rows_beyond_64(oracle, name):
    """480 x 752: 101 grid rows, cell indices up to 6463 - more than 12 bits.  Every portrait case holds its probes twice,
    in grid rows >= 64 and (lo_) below; the restatement run with the former key layout changes the verdict of the named
    high-row probes and of no low-row probe, so a kernel with that layout cannot pass the GPU parity test of any case."""
    c = nc.get(oracle, name, "portrait")
    assert c.g.yGrids == 101 and c.g.xGrids * c.g.yGrids > 4096
    for pn in c.probes:
        _check_probe(c, pn)
    _check_oracle(oracle, c)

    def best_row(pr):
        return pr[pr["side"]]["best"][2][0] // 64 if "side" in pr and pr[pr["side"]]["best"] else None
    old = copy.copy(c.g)
    old.old_cell_field = True
    _, old_pairs, _ = nc.window(old, c.kfs, c.last)
    changed = {}
    for pn, p in c.probes.items():
        if p["kf"] is None:
            continue
        pr, po = c.pairs[p["cand"]][p["kf"]], old_pairs[p["cand"]][p["kf"]]
        row = best_row(pr)
        if pn.startswith("lo_"):
            twin = c.probes[pn[3:]]
            assert row is None or row < 60, (pn, row)
            assert p["expect"]["verdict"] == twin["expect"]["verdict"]             # the same probe, in a low row
        elif row is not None:
            assert row >= 63, (pn, row)
        if (po["verdict"], po["out"]) != (pr["verdict"], pr["out"]):
            changed[pn] = po["verdict"]
    assert not any(pn.startswith("lo_") for pn in changed)
    for pn, verdict in _PORTRAIT_FLIPS[name].items():
        assert changed.get(pn) == verdict, (name, pn, changed)
    if name == "second_level_rule":          # the straddle: best in grid row 63, second in row 64, equal distances either way
        pr = c.pairs[c.probes["L_straddle_63_64"]["cand"]][1]["left"]
        assert pr["best"][2][0] // 64 == 63 and pr["sec"][2][0] // 64 == 64 and pr["best"][0] % 2 == 1 and pr["sec"][0] % 2 == 1
