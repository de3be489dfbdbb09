"""CPU checks of the stereo oracle and of the crafted cases in tests/stereo_cases.py (no GPU).

1. The oracle's findStereoMatchesORB2R is split into its matching loop and stereoFinalize (the two cuts); the factored
   `stereo_finalize`, applied to the values the loop hands over, must give what the monolithic call gives.
2. Every crafted case proves here, with the oracle and numpy alone, that it is in the regime it is named after - before
   the GPU comparison of the same case in tests/test_gpu_stereo.py counts for anything.
All comparisons are exact.  The defined-domain rule of the cases is stated in tests/stereo_cases.py."""
import numpy as np
import pytest
import synth
import stereo_cases as sc

CASES = [(n, r) for r in sc.MATCH_RIGS for n in sc.MATCH_CASES]


def _same(a, b):
    for f in ("rightIdxs", "leftIdxs", "close"):
        assert np.array_equal(a[f], b[f]), f
    assert np.array_equal(a["depth"].view(np.uint32), b["depth"].view(np.uint32))


def _oracle_case(oracle, name, rig_name):
    images, kL, dL, kR, dR, c = sc.match_case(oracle, name, rig_name)
    ref = oracle.stereo_match(c.ctx.exL, c.ctx.exR, c.ctx.rig, kL, dL, kR, dR)
    return c, ref


# ---- 1. equivalence of the split -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rig_name", CASES)
def test_split_equals_monolithic_on_crafted(oracle, name, rig_name):
    c, ref = _oracle_case(oracle, name, rig_name)
    fin = oracle.stereo_finalize(ref["preBest"], ref["preDepth"], ref["preSad"], len(c.kR), c.ctx.rig)
    _same(ref, fin)


@pytest.mark.parametrize("frame,rig_name,nfeat", [(0, "euroc", 1500), (2, "kitti", 2000)])
def test_split_equals_monolithic_on_rendered(oracle, frame, rig_name, nfeat):
    L, R, _ = synth.stereo_frame(frame, rig_name)
    rig = synth.RIGS[rig_name]
    oL, oR = oracle.Extractor(nfeat), oracle.Extractor(nfeat)
    kL, dL = oL.extract(L)
    kR, dR = oR.extract(R)
    ref = oracle.stereo_match(oL, oR, rig, kL, dL, kR, dR)
    n = int((ref["preBest"] >= 0).sum())
    assert n > 200 and n > (ref["rightIdxs"] >= 0).sum() > 0          # the cuts dropped something
    _same(ref, oracle.stereo_finalize(ref["preBest"], ref["preDepth"], ref["preSad"], len(kR), rig))


def test_split_tiled_limit_case(oracle):
    """the full-path case at the left-key limit: ties straddle the depth cut and left keys share right keys"""
    images, kL, dL, kR, dR, c = sc.tiled_case(oracle, "euroc", sc.STEREO_MAX_L)
    ref = oracle.stereo_match(c.ctx.exL, c.ctx.exR, c.ctx.rig, kL, dL, kR, dR)
    _same(ref, oracle.stereo_finalize(ref["preBest"], ref["preDepth"], ref["preSad"], len(kR), c.ctx.rig))
    n, endDe, cut, less, equal, quota = sc.depth_cut(ref["preBest"], ref["preDepth"])
    print("tiled: n %d endDe %d cut %r less %d equal %d quota %d" % (n, endDe, cut, less, equal, quota))
    assert n > 4000 and endDe >= 40 and equal >= 2 and 0 < quota < equal
    share = np.bincount(ref["preBest"][ref["preBest"] >= 0])
    assert share.max() > 100
    kept, dropped = ref["rightIdxs"] >= 0, (ref["preBest"] >= 0) & (ref["rightIdxs"] < 0)
    assert kept.any() and dropped.any()
    assert np.intersect1d(ref["preBest"][kept], ref["preBest"][dropped]).size > 0


# ---- 2. regime checks, one per case ---------------------------------------------------------------------------------
def _common_regime(c, ref):
    """the counters and the set of accepted pairs are what the builder predicts"""
    got = dict(candidates=ref["candidates"], sad=ref["sad"], matches=ref["matches"])
    print(c.name, c.ctx.rig_name, "expect", c.expect, "oracle", got)
    assert got == c.expect
    assert np.array_equal(ref["preBest"], c.pre_best)
    for l, cur in c.curves.items():
        if c.pre_best[l] >= 0:
            assert ref["preSad"][l] == cur["bestDistW"], l
    # the filler pairs are ordinary: accepted at bestX 0 and kept
    for l in range(10):
        assert c.curves[l]["bestX"] == 0 and not c.curves[l]["skipped"].any() and ref["rightIdxs"][l] == c.pre_best[l] >= 0


def _case(oracle, name, rig_name):
    c, ref = _oracle_case(oracle, name, rig_name)
    _common_regime(c, ref)
    return c, ref


@pytest.mark.parametrize("rig_name", sc.MATCH_RIGS)
@pytest.mark.parametrize("name", ["skip_left", "skip_right"])
def test_regime_shift_skip(oracle, name, rig_name):
    """the accepted pair has bestX next to a skipped shift, so an allDists[] = 0 of a skipped shift enters the parabola"""
    c, ref = _case(oracle, name, rig_name)
    side = -1 if name == "skip_left" else 1
    for tag, bx in c.want_bestX.items():
        l = c.tags[tag]
        cur = c.curves[l]
        assert cur["bestX"] == bx and cur["skipped"].any() and not cur["skipped"].all()
        assert cur["skipped"][5 + bx + side] and cur["dists"][5 + bx + side] == 0      # the neighbour is a skipped shift
        assert not cur["skipped"][5 + bx - side] and cur["dists"][5 + bx - side] > cur["dists"][5 + bx]
        assert ref["preBest"][l] >= 0 and ref["rightIdxs"][l] >= 0 and ref["depth"][l] > 0
        print(tag, "bestX", bx, "dists", cur["dists"], "delta", cur["delta"], "depth", ref["depth"][l])


@pytest.mark.parametrize("rig_name", sc.MATCH_RIGS)
def test_regime_skip_all(oracle, rig_name):
    """every shift skipped: refined, counted as a match (delta = 0 / 0), not accepted"""
    c, ref = _case(oracle, "skip_all", rig_name)
    for tag in ("p0", "p1", "p2", "p3"):
        l = c.tags[tag]
        cur = c.curves[l]
        assert cur["skipped"].all() and cur["bestDistW"] == sc.INT_MAX and cur["bestX"] == 0 and np.isnan(cur["delta"])
        assert ref["preBest"][l] == -1 and ref["rightIdxs"][l] == -1
    # without the four probes the counters are the filler's alone: each probe added a candidate, a refinement, a match
    assert c.expect == dict(candidates=14, sad=14, matches=14)


@pytest.mark.parametrize("rig_name", sc.MATCH_RIGS)
def test_regime_octave(oracle, rig_name):
    c, ref = _case(oracle, "octave", rig_name)
    # admitted: 1 + 2 + 1 + 2 right keys; four more right keys two octaves away share the rows and add nothing
    assert c.expect["candidates"] == 10 + 6 and len(c.kR) == 10 + 6 + 4
    for tag, oL in (("o0", 0), ("o3", 3), ("o7", 7), ("o7s", 7)):
        l = c.tags[tag]
        assert l in c.curves and c.kL["octave"][l] == oL
        row = np.flatnonzero(c.kR["y"] == c.kL["y"][l])
        admitted = [r for r in row if abs(int(c.kR["octave"][r]) - oL) <= 1]
        excluded = [r for r in row if abs(int(c.kR["octave"][r]) - oL) == 2]
        assert len(admitted) + len(excluded) == len(row)
        # an excluded key has the identical descriptor: had it been admitted it would have won
        assert all(sc.hamming(c.dL[l], c.dR[r]) == 0 for r in excluded) and (excluded or tag == "o7s")
        assert min(sc.hamming(c.dL[l], c.dR[r]) for r in admitted) > 0 and c.best_of[l] in admitted


@pytest.mark.parametrize("rig_name", sc.MATCH_RIGS)
def test_regime_band(oracle, rig_name):
    c, ref = _case(oracle, "band", rig_name)
    assert c.expect["candidates"] == 10 + 3
    for tag in ("b0", "b1", "b7"):
        assert c.tags[tag + "_in"] in c.curves and c.tags[tag + "_out"] not in c.curves
        assert c.kL["y"][c.tags[tag + "_out"]] - c.kL["y"][c.tags[tag + "_in"]] == 1
    # the in-band keys reach the SAD stage, so the oracle's refinement count says the band edge was inside
    assert ref["sad"] == 13


@pytest.mark.parametrize("rig_name", sc.MATCH_RIGS)
def test_regime_uR(oracle, rig_name):
    c, ref = _case(oracle, "uR", rig_name)
    # uR == uL adds a candidate; the two keys one ulp above add none (three right keys, one candidate)
    assert c.expect["candidates"] == 11 and len(c.kR) == 13
    l = c.tags["eq"]
    assert ref["preBest"][l] == 10 and c.kR["y"][10] == c.kL["y"][l] and c.kR["y"][11] > c.kL["y"][l]
    assert np.float32(c.kR["y"][11]).view(np.uint32) - np.float32(c.kL["y"][l]).view(np.uint32) == 1
    assert sc.hamming(c.dL[l], c.dR[11]) == 0 and ref["preBest"][c.tags["ulp"]] == -1


@pytest.mark.parametrize("rig_name", sc.MATCH_RIGS)
def test_regime_threshold(oracle, rig_name):
    c, ref = _case(oracle, "threshold", rig_name)
    # the 76-bit key adds a candidate but no refinement
    assert c.expect == dict(candidates=10 + 4, sad=10 + 2, matches=c.expect["matches"])
    assert sc.hamming(c.dL[c.tags["d75"]], c.dR[10]) == 75 and sc.hamming(c.dL[c.tags["d76"]], c.dR[11]) == 76
    assert ref["preBest"][c.tags["d75"]] == 10 and ref["preBest"][c.tags["d76"]] == -1
    l = c.tags["tie75"]
    assert sc.hamming(c.dL[l], c.dR[12]) == sc.hamming(c.dL[l], c.dR[13]) == 75 and ref["preBest"][l] == 12


@pytest.mark.parametrize("rig_name", sc.MATCH_RIGS)
def test_regime_half(oracle, rig_name):
    c, ref = _case(oracle, "half", rig_name)
    assert c.expect["candidates"] == 10 + 2
    for tag in ("l_even", "l_odd"):
        assert c.kL["y"][c.tags[tag]] % 1 == 0.5
    assert c.kR["y"][12] % 1 == 0.5 and c.kR["y"][13] % 1 == 0.5
    assert ref["preBest"][c.tags["l_even"]] == 10 and ref["preBest"][c.tags["r_odd"]] == 13
    assert ref["preBest"][c.tags["l_odd"]] == -1 and ref["preBest"][c.tags["r_even"]] == -1


@pytest.mark.parametrize("rig_name", sc.MATCH_RIGS)
def test_regime_rows_outside(oracle, rig_name):
    c, ref = _case(oracle, "rows_outside", rig_name)
    H = c.ctx.rig["h"]
    rows = np.rint(c.kR["y"][10:]).astype(int)
    assert (rows < 0).sum() >= 3 and (rows >= H).sum() >= 3 and 0 in rows
    # eight candidates come from right keys whose y lies outside the image; none is refined
    assert c.expect == dict(candidates=10 + 8, sad=10, matches=10)
    assert (ref["preBest"][10:] == -1).all()
    assert c.kL["y"][c.tags["neg"]] < 0 and np.rint(c.kL["y"][c.tags["neg"]]) == 0
    assert np.signbit(c.kL["y"][c.tags["negzero"]]) and c.kL["y"][c.tags["negzero"]] == 0


@pytest.mark.parametrize("rig_name", sc.MATCH_RIGS)
def test_regime_many_to_one(oracle, rig_name):
    """a dropped left key and a kept left key share a right key, with the dropped one before and after the kept one"""
    c, ref = _case(oracle, "many_to_one", rig_name)
    seen = 0
    for g in range(2):
        t = c.tags["true_%d" % g]
        r = ref["preBest"][t]
        assert r >= 0 and ref["rightIdxs"][t] == r                      # the true pair is kept ...
        imps = [c.tags["imp_%d_%d" % (g, i)] for i in range(6)]
        shared = [l for l in imps if ref["preBest"][l] == r]
        assert shared and all(ref["rightIdxs"][l] == -1 for l in shared)  # ... impostors were accepted onto r and dropped
        assert all((l < t) == (g == 0) for l in imps)
        assert ref["leftIdxs"][r] == -1                                 # so r ends up unowned although t -> r stands
        print("group", g, "true", t, "right", r, "accepted impostors", shared, "SADs", ref["preSad"][shared], ref["preSad"][t])
        seen += len(shared)
    assert seen >= 2


# ---- the direct finalize cases ---------------------------------------------------------------------------------------
FIN = sc.finalize_cases()


@pytest.mark.parametrize("name", sorted(FIN))
def test_finalize_case_domain_and_naive(oracle, name):
    """the inputs stay in the domain the match kernel can emit, and the oracle's finalize agrees with a plain Python
    restatement (sorted tuples) of src/FeatureMatcher.cpp:655-705"""
    best, depth, sad, nR = FIN[name]
    acc = best >= 0
    assert (best < nR).all() and np.isfinite(depth[acc]).all() and (depth[acc] > 0).all()
    assert ((sad[acc] >= 0) & (sad[acc] <= sc.SAD_MAX)).all() and np.isin(sad[~acc], (0, sc.INT_MAX)).all()
    rig = synth.RIGS["euroc"]
    ref = oracle.stereo_finalize(best, depth, sad, nR, rig)
    _same(ref, sc.naive_finalize(best, depth, sad, nR, np.float32(rig["bl"]) * np.float32(40)))


@pytest.mark.parametrize("name", sc.TIE_CASES)
def test_regime_finalize_depth_ties(name):
    """at least two accepted pairs share the cut depth bit for bit and only some of them are dropped"""
    best, depth, sad, nR = FIN[name]
    n, endDe, cut, less, equal, quota = sc.depth_cut(best, depth)
    print(name, "n", n, "endDe", endDe, "cut", cut, "less", less, "equal", equal, "quota", quota)
    assert endDe >= 1 and equal >= 2 and 0 < quota < equal


def test_regime_finalize_counts():
    want = {"n1": 0, "n2": 0, "n99": 0, "n100": 1, "n101": 1, "n199": 1, "n200": 2, "n201": 2}
    for k, e in want.items():
        n, endDe = sc.depth_cut(FIN[k][0], FIN[k][1])[:2]
        assert (n, endDe) == (int(k[1:]), e)
    for k in ("max_l_ties", "max_l_all_equal", "max_l_distinct"):
        assert len(FIN[k][0]) == sc.STEREO_MAX_L and (FIN[k][0] >= 0).all()
    n, endDe, cut, less, equal, quota = sc.depth_cut(*FIN["tie_depth_whole_group"][:2])
    assert equal == 3 and quota == equal
    assert (FIN["holes"][0] < 0).sum() > 100 and (FIN["tie_depth_holes"][0] < 0).sum() > 100


def test_regime_finalize_sad_edges(oracle):
    rig = synth.RIGS["euroc"]
    edges = sc.sad_edge_medians()
    assert len(edges) >= 2
    for tag, (m, t) in (("lo", edges[0]), ("hi", edges[-1])):
        best, depth, sad, nR = FIN["sad_on_cut_%s" % tag]
        assert int(np.sort(sad)[len(sad) // 2]) == m
        cut = np.float32(m) * (np.float32(1.5) * np.float32(1.4))
        assert float(cut) == t and (sad == t).sum() == 10 and (sad == t - 1).sum() == 10
        ref = oracle.stereo_finalize(best, depth, sad, nR, rig)
        assert (ref["rightIdxs"][sad == t] == -1).all() and (ref["rightIdxs"][sad == t - 1] >= 0).all()
        print("median", m, "cut-off", cut)
    best, depth, sad, nR = FIN["sad_all_zero"]
    assert (oracle.stereo_finalize(best, depth, sad, nR, rig)["rightIdxs"] == -1).all()       # medDistD == 0 drops all
    best, depth, sad, nR = FIN["sad_all_equal"]
    assert (oracle.stereo_finalize(best, depth, sad, nR, rig)["rightIdxs"] >= 0).sum() == 149   # (one goes to the depth cut)
    for n in (100, 101):
        best, depth, sad, nR = FIN["sad_median_tie_%d" % n]
        s = np.sort(sad)
        assert s[n // 2] == 250 and s[n // 2 - 1] == 100
        ref = oracle.stereo_finalize(best, depth, sad, nR, rig)
        assert (ref["rightIdxs"][sad == 600] == -1).all() and (ref["rightIdxs"][sad == 250] >= 0).sum() >= (sad == 250).sum() - 1


def test_regime_finalize_many_to_one(oracle):
    best, depth, sad, nR = FIN["many_to_one"]
    ref = oracle.stereo_finalize(best, depth, sad, nR, synth.RIGS["euroc"])
    kept = ref["rightIdxs"] >= 0
    for r, (any_kept, owned) in enumerate([(True, False), (True, False), (True, False), (True, False), (False, False), (True, True)]):
        assert kept[best == r].any() == any_kept and (ref["leftIdxs"][r] >= 0) == owned, r
    # group 3 loses an EARLIER key only: the last writer is kept and the right key still ends up unowned
    g3 = np.flatnonzero(best == 3)
    assert kept[g3[-1]] and not kept[g3[0]] and ref["leftIdxs"][3] == -1
    assert ref["leftIdxs"][5] == np.flatnonzero(best == 5)[-1] and kept[best == 5].all()
