"""GPU tests of the relocalisation stage (vslam_relocalize, vslam_system_relocalize) against its CPU restatement
(tests/reloc_ref.py): the stage has no reference counterpart, the restatement is written from the rules in DESIGN.md section 6.
Steps A - C are compared bit for bit through the test tap (vslam_relocalize_debug), the refined pose to 1e-7 as in the
project's other pose tests.  Crafted frames go through set_keys + vslam_stereo_finalize_arrays (the finalize kernel's 1 %
nearest-depth cut applies: the tests read the stereo state back and hand exactly that to the restatement)."""
import hashlib
import os
import numpy as np
import pytest
import synth
import reloc_cases as rc
import reloc_ref as rr

pytestmark = pytest.mark.gpu
RIG = rc.RIG


def rigid_inv(T):
    Ti = np.eye(4)
    Rt = T[:3, :3].T.copy()
    Ti[:3, :3] = Rt
    for i in range(3):
        Ti[i, 3] = -(Rt[i, 0] * T[0, 3] + Rt[i, 1] * T[1, 3] + Rt[i, 2] * T[2, 3])
    return Ti


@pytest.fixture(scope="module")
def crafted(capi, oracle):
    """one extractor / matcher pair for every crafted frame (the extractor never runs: both key sets are overridden)"""
    ge = capi.Extractor(RIG["w"], RIG["h"], 1500, batch=2)
    m = capi.Matcher(RIG, ge, 0, ge, 1)
    return m, oracle.Extractor(1500).InvSigmaFactor


def load_frame(m, kL, dL, kR, dR, best, depth, sad):
    m.stereo_finalize_arrays(best, depth, sad, len(kR))
    m.set_keys(0, kL, dL)
    m.set_keys(1, kR, dR)
    return m.stereo_fetch(len(kL), len(kR))


def assert_steps_abc(dbg, rep, pairs, ref, counts=True):
    assert np.array_equal(dbg["d"], ref["d"])
    assert np.array_equal(dbg["key_winner"], ref["key_winner"])
    assert np.array_equal(pairs, ref["pairs"])
    assert rep["n_points"] == ref["n_points"] and rep["n_pairs"] == ref["n_pairs"]
    if counts:
        assert np.array_equal(dbg["counts"], ref["hyp"]["counts"])
        assert (rep["best_hypothesis"], rep["best_count"]) == (ref["best_hypothesis"], ref["best_count"])
        assert np.array_equal(dbg["flags"], ref["hyp"]["flags"])


# ---- step A / B: matching --------------------------------------------------------------------------------------------------
def matching_scene(N, nL, seed):
    """random keys with a duplicate pair across the tile edge, map points planted 0 .. 69 bits away from a random key (so
    that both sides of max_hamming and of the ratio test occur, and - with more points than keys - many points propose one
    key, with equal distances among them); some keys without an accepted stereo pair"""
    rng = np.random.Generator(np.random.PCG64(seed))
    dL = rng.integers(0, 256, (nL, 32), dtype=np.uint8)
    if nL >= 2:
        dL[nL - 1] = dL[0]
    desc = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    if nL:
        for p in range(N):
            if p % 5 != 4:
                desc[p], _ = rc.flip_bits(dL[int(rng.integers(0, nL))], int(rng.integers(0, 70)), rng)
    kL = np.zeros(nL, rc.KP_DTYPE); kR = np.zeros(nL, rc.KP_DTYPE)
    kL["x"] = rng.uniform(60, RIG["w"] - 40, nL); kL["y"] = rng.uniform(40, RIG["h"] - 40, nL); kL["octave"] = rng.integers(0, 8, nL)
    kR["x"] = kL["x"] - rng.uniform(5, 25, nL).astype(np.float32); kR["y"] = kL["y"]; kR["octave"] = kL["octave"]
    best = np.arange(nL, dtype=np.int32)
    best[rng.random(nL) < 0.2] = -1
    depth = rng.uniform(2, 8, nL).astype(np.float32)
    return dict(kL=kL, dL=dL, kR=kR, dR=rng.integers(0, 256, (nL, 32), dtype=np.uint8), best=best, depth=depth,
                sad=np.full(nL, 10, np.int32), points=rng.uniform(-5, 5, (N, 3)), desc=desc)


@pytest.mark.parametrize("nL", [0, 1, 2047, 2049])
@pytest.mark.parametrize("N", [0, 1, 63, 65, 257, 300])
def test_match_bit_for_bit(capi, oracle, crafted, N, nL):
    m, inv_sigma = crafted
    g = matching_scene(N, nL, 1000 * N + nL)
    st = load_frame(m, g["kL"], g["dL"], g["kR"], g["dR"], g["best"], g["depth"], g["sad"])
    T, rep, pairs = m.relocalize(g["points"], g["desc"], n_hypotheses=4)
    ref = rr.relocalize(oracle, RIG, inv_sigma, g["points"], g["desc"], g["kL"], g["dL"], g["kR"], st, n_hypotheses=4)
    assert_steps_abc(m.relocalize_debug(), rep, pairs, ref, counts=False)
    assert rep["success"] == 0 and T is None                    # random world points: nothing to recover
    if N >= 63 and nL >= 2047:
        d = ref["d"]
        assert (d[:, 0] <= 50).any() and (d[:, 0] > 50).any() and (ref["pairs"] >= 0).any()
        lost = ref["key_winner"][g["best"] < 0]
        lost = lost[lost >= 0]                                  # winners on keys without depth exist, and are dropped
        assert len(lost) and (ref["pairs"][lost] == -1).all()


def test_match_rules_at_the_tile_edge(capi, oracle, crafted):
    """every rule of step A with the keys concerned on both sides of the 2048-key LDS tile"""
    m, inv_sigma = crafted
    nL = 2049
    rng = np.random.Generator(np.random.PCG64(77))
    g = matching_scene(0, nL, 5)
    dL = rng.integers(0, 256, (nL, 32), dtype=np.uint8)
    K50, KTIE_A, KTIE_B, KTWO, KEQ, KND, KA, KB = 2047, 100, 2048, 2046, 1, 3, 7, 2045
    dL[KTIE_B] = dL[KTIE_A]
    pts = []
    pts.append(rc.flip_bits(dL[K50], 50, rng)[0])               # 0: accepted at the bound
    pts.append(rc.flip_bits(dL[K50], 51, rng)[0])               # 1: refused
    pts.append(rc.flip_bits(dL[KTIE_A], 3, rng)[0])             # 2: tie across the tile edge: lowest index, d2 == d1 refuses
    pts.append(rc.flip_bits(dL[KTWO], 7, rng)[0])               # 3: loses key KTWO ...
    pts.append(rc.flip_bits(dL[KTWO], 5, rng)[0])               # 4: ... to the smaller distance
    pts.append(rc.flip_bits(dL[KEQ], 9, rng)[0])                # 5: equal distances: the lower point index wins
    pts.append(rc.flip_bits(dL[KEQ], 9, rng)[0])                # 6
    pts.append(rc.flip_bits(dL[KND], 2, rng)[0])                # 7: wins a key without depth: dropped in step B ...
    pts.append(rc.flip_bits(dL[KND], 6, rng)[0])                # 8: ... and the key stays lost to the loser
    p9, bits = rc.flip_bits(dL[KA], 40, rng)                    # 9: ratio test, 100 * 40 against 80 * d2
    pts.append(p9)
    desc = np.stack(pts)
    best = np.arange(nL, dtype=np.int32); best[KND] = -1
    depth = np.full(nL, 5.0, np.float32)
    depth[200:221] = 1.0                                        # the 20 pairs the 1 % cut takes are none of the keys above
    pw = rng.uniform(-5, 5, (len(desc), 3))
    for d2 in (50, 51):
        dL[KB] = rc.flip_bits(dL[KA], d2 - 40, rng, avoid=bits)[0]
        st = load_frame(m, g["kL"], dL, g["kR"], g["dR"], best, depth, g["sad"])
        assert st["depth"][K50] > 0 and st["depth"][KND] < 0
        T, rep, pairs = m.relocalize(pw, desc, n_hypotheses=1)
        ref = rr.relocalize(oracle, RIG, inv_sigma, pw, desc, g["kL"], dL, g["kR"], st, n_hypotheses=1)
        dbg = m.relocalize_debug()
        assert_steps_abc(dbg, rep, pairs, ref, counts=False)
        d, kw = dbg["d"], dbg["key_winner"]
        assert list(d[0][:2]) == [50, K50] and list(d[1][:2]) == [51, K50] and kw[K50] == 0 and pairs[0] == K50 and pairs[1] == -1
        assert list(d[2]) == [3, KTIE_A, 3] and kw[KTIE_A] == -1 and kw[KTIE_B] == -1 and pairs[2] == -1
        assert kw[KTWO] == 4 and pairs[4] == KTWO and pairs[3] == -1
        assert kw[KEQ] == 5 and pairs[5] == KEQ and pairs[6] == -1
        assert kw[KND] == 7 and pairs[7] == -1 and pairs[8] == -1
        assert list(d[9]) == [40, KA, d2]
        assert (kw[KA], pairs[9]) == ((-1, -1) if d2 == 50 else (9, KA))       # 4000 < 4000 is refused, 4000 < 4080 accepted


def test_limits_and_arguments(capi, crafted):
    m, _ = crafted
    g = matching_scene(4, 8, 3)
    load_frame(m, g["kL"], g["dL"], g["kR"], g["dR"], g["best"], g["depth"], g["sad"])
    texts = []
    with pytest.raises(capi.VslamError) as e:
        m.relocalize(np.zeros((65537, 3)), np.zeros((65537, 32), np.uint8))
    assert e.value.status == capi.ERR_CAPACITY
    texts.append(str(e.value))
    with pytest.raises(capi.VslamError) as e:
        m.relocalize(g["points"], g["desc"], n_hypotheses=1025)
    assert e.value.status == capi.ERR_INVALID
    texts.append(str(e.value))
    ge = capi.Extractor(RIG["w"], RIG["h"], 1500, batch=2)
    fresh = capi.Matcher(RIG, ge, 0, ge, 1)                    # no completed stereo match
    with pytest.raises(capi.VslamError) as e:
        fresh.relocalize(g["points"], g["desc"])
    assert e.value.status == capi.ERR_INVALID
    texts.append(str(e.value))
    assert not any("lane" in t for t in texts), texts          # the single call is one lane of the batched driver and names none


# ---- step C: hypotheses ----------------------------------------------------------------------------------------------------
def hypothesis_case(m, oracle, inv_sigma, C, mode="pose", **params):
    """a crafted frame whose restatement keeps every tested residual a relative 1e-6 away from the chi2 bound (the seed is
    advanced until that holds, so that a last-bit difference cannot flip a count)"""
    for seed in range(100 * C, 100 * C + 20):
        g = rc.frame_for_records(C, 0.4, seed, mode=mode)
        st = oracle.stereo_finalize(g["best"], g["depth"], g["sad"], len(g["kR"]), RIG)
        ref = rr.relocalize(oracle, RIG, inv_sigma, g["points"], g["desc"], g["kL"], g["dL"], g["kR"], st, **params)
        if ref["hyp"]["margin"] > 1e-6:
            break
    assert ref["hyp"]["margin"] > 1e-6 and ref["n_pairs"] == C
    got_st = load_frame(m, g["kL"], g["dL"], g["kR"], g["dR"], g["best"], g["depth"], g["sad"])
    for f in ("rightIdxs", "leftIdxs", "depth", "close"):
        assert np.array_equal(got_st[f], st[f])
    T, rep, pairs = m.relocalize(g["points"], g["desc"], **params)
    return g, ref, T, rep, pairs, m.relocalize_debug()


@pytest.mark.parametrize("C", [2, 3, 64, 65, 200])
def test_hypotheses_equal_the_restatement(capi, oracle, crafted, C):
    m, inv_sigma = crafted
    g, ref, T, rep, pairs, dbg = hypothesis_case(m, oracle, inv_sigma, C)
    assert_steps_abc(dbg, rep, pairs, ref)
    assert (rep["success"], rep["n_inliers"], rep["n_stereo"]) == (ref["success"], ref["n_inliers"], ref["n_stereo"])
    if C == 2:
        assert rep["success"] == 0 and rep["n_pairs"] == 2 and rep["best_count"] == 0 and T is None      # the failure report
    if C >= 64:                                              # 60 % of the pairs fit one pose: found, refined, accepted at C = 200
        assert rep["best_count"] >= int(round(0.6 * C))
        assert np.abs(dbg["flags"].sum() - rep["best_count"]) == 0
    if C == 200:
        assert rep["success"] == 1 and np.abs(T - ref["T_cw"]).max() < 1e-7
        assert np.abs(T - g["T_cw"]).max() < 1e-3           # (depths and pixels are floats: the crafted pose comes back to ~1e-5)
    else:
        assert (T is None) == (ref["T_cw"] is None)
        if T is not None:
            assert np.abs(T - ref["T_cw"]).max() < 1e-7


@pytest.mark.parametrize("H", [1, 4, 1024])
def test_hypothesis_counts(capi, oracle, crafted, H):
    m, inv_sigma = crafted
    g, ref, T, rep, pairs, dbg = hypothesis_case(m, oracle, inv_sigma, 64, n_hypotheses=H)
    assert len(dbg["counts"]) == H
    assert_steps_abc(dbg, rep, pairs, ref)


def test_collinear_points_void_every_hypothesis(capi, oracle, crafted):
    m, inv_sigma = crafted
    g, ref, T, rep, pairs, dbg = hypothesis_case(m, oracle, inv_sigma, 64, mode="collinear")
    assert_steps_abc(dbg, rep, pairs, ref)
    assert rep["n_pairs"] == 64 and not dbg["counts"].any() and rep["best_hypothesis"] == 0 and rep["best_count"] == 0
    assert rep["success"] == 0 and T is None and not dbg["flags"].any()


def test_points_behind_the_camera_do_not_count(capi, oracle, crafted):
    """40 % of the pairs are points BEHIND the camera whose every residual is zero under the true pose: only the z > 0 test
    keeps them out.  (A frame whose correspondences ALL lie behind every hypothesis cannot be built through the stage: the
    three sampled pairs are reproduced at their own X_c, whose z is the key's positive depth; the restatement's test covers
    that case on records of its own, tests/test_reloc_ref.py.)"""
    m, inv_sigma = crafted
    g, ref, T, rep, pairs, dbg = hypothesis_case(m, oracle, inv_sigma, 65, mode="mirror")
    assert_steps_abc(dbg, rep, pairs, ref)
    rec = ref["rec"]
    R, t = g["T_cw"][:3, :3], g["T_cw"][:3, 3]
    z_true = rec["Xw"] @ R[2] + t[2]
    behind = z_true < 0
    assert behind.sum() == 26 and rep["best_count"] == 39
    assert not dbg["flags"][behind].any() and dbg["flags"][~behind].all()
    # without the z test they would all count: their weighted residual under the true pose is far below the bound
    _, val = rr.chi2_values(rec, R, t, RIG, inv_sigma)
    assert (val[behind] < 1e-3).all()


# ---- the single call against what it returned before it became the one-lane case of the batched driver ---------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reloc_single.npz")
# name -> (generator, its arguments): hypothesis_case in mode 0, reloc_p3p_cases.find_case in mode 1, matching_scene (N, nL)
RECORDED = {"pose_C2": ("pose", 2), "pose_C3": ("pose", 3), "mirror_C65": ("mirror", 65), "pose_C200": ("pose", 200),
            "p3p_C200": ("p3p", 200), "p3p_C2": ("p3p", 2),
            "match_0_2049": ("match", 0, 2049), "match_300_0": ("match", 300, 0), "match_1_1": ("match", 1, 1), "match_257_2047": ("match", 257, 2047)}
FRAME_ARRAYS = ("kL", "dL", "kR", "dR", "best", "depth", "sad", "points", "desc")
REPORT_INTS = ("success", "n_points", "n_pairs", "best_hypothesis", "best_count", "n_inliers", "n_stereo")


def recorded_case(name, m, oracle, inv_sigma):
    """one case of tests/golden/reloc_single.npz run on matcher m: what make_reloc_single.py stored and what the test compares.
    ints: the report's integer fields, lm.iterations, lm.inner, whether a pose was returned; f64: the pose (zeros without one),
    lm.initialError, lm.finalError, lm.lam; sha: a checksum of the frame and the map the generator built"""
    kind, args = RECORDED[name][0], RECORDED[name][1:]
    if kind == "match":
        N, nL = args
        g = matching_scene(N, nL, 1000 * N + nL)
        load_frame(m, g["kL"], g["dL"], g["kR"], g["dR"], g["best"], g["depth"], g["sad"])
        T, rep, pairs = m.relocalize(g["points"], g["desc"], n_hypotheses=4)
    elif kind == "p3p":
        import reloc_p3p_cases as pc
        g, st, _ = pc.find_case(oracle, inv_sigma, C=args[0])
        load_frame(m, g["kL"], g["dL"], g["kR"], g["dR"], g["best"], g["depth"], g["sad"])
        T, rep, pairs = m.relocalize(g["points"], g["desc"], mode=1)
    else:
        g, _, T, rep, pairs, _ = hypothesis_case(m, oracle, inv_sigma, args[0], mode=kind)
    dbg = m.relocalize_debug()
    sha = hashlib.sha256()
    for f in FRAME_ARRAYS:
        sha.update(np.ascontiguousarray(g[f]).tobytes())
    lm = rep["lm"]
    out = dict(ints=np.array([rep[f] for f in REPORT_INTS] + [lm["iterations"], lm["inner"], int(T is not None)], np.int32),
               f64=np.concatenate([(T if T is not None else np.zeros((4, 4))).ravel(), [lm["initialError"], lm["finalError"], lm["lam"]]]),
               pairs=pairs, sha=np.frombuffer(sha.digest(), np.uint8))
    out.update(dbg)
    return out


@pytest.mark.parametrize("name", list(RECORDED))
def test_single_call_returns_recorded_results(capi, oracle, crafted, name):
    """vslam_relocalize against tests/golden/reloc_single.npz: what the call returned on an MI355X at commit 85824ca, the last one
    where it had its own by-value kernels, its own host loop and the host-built refinement problem (make_reloc_single.py).
    Integers, pairs, the four tap arrays, the pose and the three LM doubles byte for byte: the bound between the two drivers was
    1e-12 max(1, |x|) (test_gpu_reloc_batch.py, test_gpu_reloc_p3p.py), the difference seen on every case here was zero
    (profiles/README.md), so the bytes are held."""
    m, inv_sigma = crafted
    got = recorded_case(name, m, oracle, inv_sigma)
    with np.load(GOLDEN) as z:
        want = {k: z[name + "/" + k] for k in got}
    assert np.array_equal(got["sha"], want["sha"]), "the seeded generator of this case no longer builds the recorded inputs"
    for k in ("ints", "pairs", "d", "key_winner", "counts", "flags", "f64"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), (k, np.abs(got[k].astype(np.float64) - want[k]).max() if got[k].size else 0)


# ---- the whole stage on rendered frames ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rendered(capi, oracle):
    """the map of frame 0 (initializeMap, as vslam_tracker_init_map builds it on the device: tests/test_gpu_track.py pins the
    two to each other) and an extractor / matcher pair for the frames to relocalise"""
    from test_gpu_track import oracle_init_map
    oL, oR = oracle.Extractor(1500), oracle.Extractor(1500)
    L, R, T0 = synth.stereo_frame(0)
    kL, dL = oL.extract(L); kR, dR = oR.extract(R)
    st = oracle.stereo_match(oL, oR, RIG, kL, dL, kR, dR)
    xyz, desc, _ = oracle_init_map(RIG, oL, kL, dL, st, T0)
    ge = capi.Extractor(RIG["w"], RIG["h"], 1500, batch=2)
    m = capi.Matcher(RIG, ge, 0, ge, 1)
    return dict(oL=oL, oR=oR, ge=ge, m=m, xyz=xyz, desc=desc)


def _stage(oracle, s, L, R):
    kL, dL = s["oL"].extract(L); kR, dR = s["oR"].extract(R)
    st = oracle.stereo_match(s["oL"], s["oR"], RIG, kL, dL, kR, dR)
    ref = rr.relocalize(oracle, RIG, s["oL"].InvSigmaFactor, s["xyz"], s["desc"], kL, dL, kR, st)
    s["ge"].extract([L, R]); s["m"].stereo_match()
    T, rep, pairs = s["m"].relocalize(s["xyz"], s["desc"])
    return ref, T, rep, pairs


@pytest.mark.parametrize("frame", [1, 4, 8])
def test_relocalise_rendered_frames(capi, oracle, rendered, frame):
    """No prior: the pose of frames 1, 4 and 8 from the map of frame 0.  Error of the restatement itself against the ground
    truth (max |T_wc - truth| over the 4 x 4 entries), measured on the CPU: 1.45e-3 (frame 1), 1.17e-3 (frame 4), 1.50e-3
    (frame 8); the stage is held to three times the restatement's error on the same frame."""
    L, R, T_true = synth.stereo_frame(frame)
    ref, T, rep, pairs = _stage(oracle, rendered, L, R)
    assert ref["success"] == 1 and rep["success"] == 1
    assert (rep["n_pairs"], rep["n_inliers"], rep["n_stereo"]) == (ref["n_pairs"], ref["n_inliers"], ref["n_stereo"])
    assert (rep["best_hypothesis"], rep["best_count"]) == (ref["best_hypothesis"], ref["best_count"])
    assert np.array_equal(pairs, ref["pairs"])
    assert np.abs(T - ref["T_cw"]).max() < 1e-7
    err_ref = np.abs(rigid_inv(ref["T_cw"]) - T_true).max()
    err = np.abs(rigid_inv(T) - T_true).max()
    print("frame %d: pose error %.3e (restatement %.3e), %d pairs, %d inliers" % (frame, err, err_ref, rep["n_pairs"], rep["n_inliers"]))
    assert err <= 3 * err_ref


def test_foreign_scene_is_refused(capi, oracle, rendered):
    """another scene under another texture (a scene of another seed under the SAME texture shares its background walls with
    the map, and the restatement recovers its pose from them: checked on the CPU when this case was chosen)"""
    L, R, _ = synth.stereo_frame(4, scene_seed=9, tex_seed=0xBEEF)
    ref, T, rep, pairs = _stage(oracle, rendered, L, R)
    assert ref["success"] == 0 and rep["success"] == 0 and T is None
    assert (rep["n_pairs"], rep["best_count"], rep["n_inliers"]) == (ref["n_pairs"], ref["best_count"], ref["n_inliers"])


# ---- the session -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("local_mapping", [0, 1])
def test_session_relocalise(capi, oracle, local_mapping):
    import vo_system
    frames = list(range(13))
    synth.prerender(frames)
    T0 = synth.pose_at(0, RIG["fps"])
    ref = vo_system.System(RIG, 1500, T0=T0, local_mapping=bool(local_mapping))
    got = capi.System(RIG, 1500, T0=T0, local_mapping=local_mapping)
    tracked = []
    for n in frames:
        L, R, _ = synth.stereo_frame(n)
        Pr = ref.track(L, R, n)
        Pg, rep = got.track(L, R, n)
        assert np.abs(Pg - Pr).max() < 1e-7                  # (the two hold the same map: tests/test_gpu_system.py)
        tracked.append(Pg)
    before = got.counts()
    assert before["map_points"] == len(ref.mapPoints)
    L, R, _ = synth.stereo_frame(3)
    T_wc, rrep = got.relocalize(L, R, 13)
    # the restatement on the same map: every map point that is not an outlier, in creation order
    mps = [mp for mp in ref.mapPoints if not mp.isOutlier]
    xyz = np.stack([mp.wp for mp in mps]); desc = np.stack([mp.desc for mp in mps])
    kL, dL = ref.exL.extract(L); kR, dR = ref.exR.extract(R)
    st = oracle.stereo_match(ref.exL, ref.exR, RIG, kL, dL, kR, dR)
    want = rr.relocalize(oracle, RIG, ref.invSigma, xyz, desc, kL, dL, kR, st)
    assert want["success"] == 1 and rrep["success"] == 1
    assert (rrep["n_points"], rrep["n_pairs"], rrep["n_inliers"], rrep["n_stereo"]) == (len(mps), want["n_pairs"], want["n_inliers"], want["n_stereo"])
    assert np.abs(T_wc - rigid_inv(want["T_cw"])).max() < 1e-7
    print("local_mapping %d: relocalised pose of frame 3 differs from the tracked one by %.3e" % (local_mapping, np.abs(T_wc - tracked[3]).max()))
    assert np.abs(T_wc - tracked[3]).max() < 0.02
    after = got.counts()
    assert after["keyframes"] == before["keyframes"] and after["map_points"] == before["map_points"] and after["frames"] == before["frames"] + 1
    assert len(got.last_frame()[0]) == 0
    for k, f in enumerate((4, 5)):
        L, R, T_true = synth.stereo_frame(f)
        P, rep = got.track(L, R, 14 + k)
        assert rep["n_inliers"] >= 50, (f, rep)
        assert np.abs(P - T_true).max() < 0.05


def test_failed_session_relocalisation_changes_nothing(capi):
    frames = list(range(6))
    synth.prerender(list(range(8)))
    T0 = synth.pose_at(0, RIG["fps"])
    a = capi.System(RIG, 1500, T0=T0, local_mapping=1)
    b = capi.System(RIG, 1500, T0=T0, local_mapping=1)
    for n in frames:
        L, R, _ = synth.stereo_frame(n)
        Pa, _ = a.track(L, R, n); Pb, _ = b.track(L, R, n)
    Lf, Rf, _ = synth.stereo_frame(4, scene_seed=9, tex_seed=0xBEEF)
    T, rep = a.relocalize(Lf, Rf, 6)
    assert rep["success"] == 0 and np.array_equal(T, Pa)
    assert a.counts() == b.counts()
    for n in (6, 7):
        L, R, _ = synth.stereo_frame(n)
        Pa, ra = a.track(L, R, n); Pb, rb = b.track(L, R, n)
        # (poses to 1e-9, not bitwise: a local BA sums with fp64 atomics, whose order varies from run to run)
        assert np.abs(Pa - Pb).max() < 1e-9
        for f in ("keyframe_inserted", "n_active", "n_inliers", "n_stereo", "rounds", "n_keyframes", "n_map_points", "n_active_after"):
            assert ra[f] == rb[f], (n, f)
        la, lb = a.last_frame(), b.last_frame()
        assert np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1])


def test_imu_and_mono_sessions_are_refused(capi):
    L, R, _ = synth.stereo_frame(0)
    imu = dict(gravity=(0.0, 9.81, 0.0), noise=(1.6968e-4, 1.9393e-5, 2.0e-3, 3.0e-3), T_bs=synth.T_BC1, hz=200)
    s = capi.System(RIG, 1500, imu=imu, local_mapping=0)
    with pytest.raises(capi.VslamError) as e:
        s.relocalize(L, R, 1)
    assert e.value.status == capi.ERR_INVALID and "IMU" in str(e.value)
    ms = capi.MonoSystem(RIG, 1500, synth.MONO_FPS, imu=imu)
    with pytest.raises(capi.VslamError) as e:
        capi.System.relocalize(ms, L, R, 1)
    assert e.value.status == capi.ERR_INVALID and "mono" in str(e.value)
