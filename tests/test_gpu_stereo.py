"""GPU parity: HIP findStereoMatchesORB2R (through the C ABI) vs the CPU oracle.
Bar: rightIdxs / leftIdxs / close identical, estimatedDepth bitwise identical (float), the three counters equal.

Besides rendered frames, the crafted cases of tests/stereo_cases.py run here: host-supplied keys on real pyramids
through the full path (k_stereo_rows, k_stereo_match, k_stereo_finalize), and host-supplied per-left (best, depth, SAD)
arrays straight into k_stereo_finalize (vslam_stereo_finalize_arrays) against the oracle's stereo_finalize.  Each case
is first shown to be in its regime by tests/test_oracle_stereo.py on the CPU.  Defined domain (see stereo_cases.py): no
left key that can reach the SAD stage is closer than 5 level-pixels to a border of its level - there the reference is
undefined behaviour, and the kernel's clamping of an out-of-image left window stays unpinned."""
import numpy as np
import pytest
import synth
import stereo_cases as sc

pytestmark = pytest.mark.gpu


def _run_pair(oracle, capi, L, R, rig_name, nfeat):
    rig = synth.RIGS[rig_name]
    oL, oR = oracle.Extractor(nfeat), oracle.Extractor(nfeat)
    kL, dL = oL.extract(L)
    kR, dR = oR.extract(R)
    ref = oracle.stereo_match(oL, oR, rig, kL, dL, kR, dR)
    ge = capi.Extractor(rig["w"], rig["h"], nfeat, batch=2)
    ge.extract([L, R])
    m = capi.Matcher(rig, ge, 0, ge, 1)
    m.stereo_match()
    got = m.stereo_fetch(len(kL), len(kR))
    return ref, got


def _assert_same(ref, got):
    assert np.array_equal(ref["rightIdxs"], got["rightIdxs"])
    assert np.array_equal(ref["leftIdxs"], got["leftIdxs"])
    assert np.array_equal(ref["close"], got["close"])
    assert np.array_equal(ref["depth"].view(np.uint32), got["depth"].view(np.uint32))
    assert (ref["candidates"], ref["sad"], ref["matches"]) == (got["candidates"], got["sad"], got["matches"])


@pytest.mark.parametrize("frame", [0, 5])
def test_stereo_parity_euroc(oracle, capi, frame):
    L, R, _ = synth.stereo_frame(frame)
    ref, got = _run_pair(oracle, capi, L, R, "euroc", 1500)
    _assert_same(ref, got)
    assert (ref["rightIdxs"] >= 0).sum() > 200


def test_stereo_parity_kitti(oracle, capi):
    L, R, _ = synth.stereo_frame(2, "kitti")
    ref, got = _run_pair(oracle, capi, L, R, "kitti", 2000)
    _assert_same(ref, got)


def test_stereo_identical_images_zero_disparity(oracle, capi):
    """Left == right: disparity 0 is rejected (0 < d), so nothing may match."""
    L = synth.random_image(752, 480, 77)
    ref, got = _run_pair(oracle, capi, L, L.copy(), "euroc", 1500)
    _assert_same(ref, got)


def test_stereo_crafted_keys_edge_cases(oracle, capi):
    """Host-supplied keys: empty sides, a single key, duplicated right keys (ties -> first index
    wins), reversed / permuted key order."""
    L, R, _ = synth.stereo_frame(1)
    rig = synth.RIGS["euroc"]
    oL, oR = oracle.Extractor(1500), oracle.Extractor(1500)
    kL, dL = oL.extract(L)
    kR, dR = oR.extract(R)
    ge = capi.Extractor(752, 480, 1500, batch=2)
    ge.extract([L, R])
    m = capi.Matcher(rig, ge, 0, ge, 1)
    cases = []
    cases.append((kL[:0], dL[:0], kR, dR))
    cases.append((kL, dL, kR[:0], dR[:0]))
    cases.append((kL[:1], dL[:1], kR, dR))
    dupK = np.concatenate([kR, kR[:200]]); dupD = np.concatenate([dR, dR[:200]])
    cases.append((kL, dL, dupK, dupD))
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(kR))
    cases.append((kL[::-1].copy(), dL[::-1].copy(), kR[perm], dR[perm]))
    for (a, b, c, d) in cases:
        ref = oracle.stereo_match(oL, oR, rig, a, b, c, d)
        m.set_keys(0, a, b)
        m.set_keys(1, c, d)
        m.stereo_match()
        got = m.stereo_fetch(len(a), len(c))
        _assert_same(ref, got)


# ---- crafted cases (tests/stereo_cases.py) ---------------------------------------------------------------------------
_GPU = {}


def _gpu_pair(capi, ctx):
    """extractor + matcher holding the image pair of ctx; the pyramids are the oracle's, level for level"""
    key = (ctx.rig_name, ctx.shift)
    if key not in _GPU:
        ge = capi.Extractor(ctx.rig["w"], ctx.rig["h"], 500, batch=2)
        ge.extract([ctx.L, ctx.R])
        for o in range(8):
            assert np.array_equal(ge.level(0, o), ctx.lvL[o]) and np.array_equal(ge.level(1, o), ctx.lvR[o]), o
        _GPU[key] = (ge, capi.Matcher(ctx.rig, ge, 0, ge, 1))
    return _GPU[key][1]


def _full_path(m, kL, dL, kR, dR):
    m.set_keys(0, kL, dL)
    m.set_keys(1, kR, dR)
    m.stereo_match()
    return m.stereo_fetch(len(kL), len(kR))


@pytest.mark.parametrize("rig_name", sc.MATCH_RIGS)
@pytest.mark.parametrize("name", sorted(sc.MATCH_CASES))
def test_stereo_crafted_matching(oracle, capi, name, rig_name):
    """shift skips at the left / right border and of all 11 shifts, the octave, band, uR, threshold, .5-rounding and
    y < 0 edges, right-key rows outside the image, several left keys on one right key - at 752 x 480 and 1920 x 1200"""
    images, kL, dL, kR, dR, c = sc.match_case(oracle, name, rig_name)
    ref = oracle.stereo_match(c.ctx.exL, c.ctx.exR, c.ctx.rig, kL, dL, kR, dR)
    assert (ref["candidates"], ref["sad"], ref["matches"]) == (c.expect["candidates"], c.expect["sad"], c.expect["matches"])
    assert np.array_equal(ref["preBest"], c.pre_best)           # in its regime (test_oracle_stereo.py has the details)
    got = _full_path(_gpu_pair(capi, c.ctx), kL, dL, kR, dR)
    print(name, rig_name, "oracle", ref["candidates"], ref["sad"], ref["matches"], "gpu", got["candidates"], got["sad"], got["matches"],
          "accepted", int((ref["rightIdxs"] >= 0).sum()), int((got["rightIdxs"] >= 0).sum()))
    _assert_same(ref, got)


FIN = sc.finalize_cases()


def _assert_same_finalize(ref, got):
    assert np.array_equal(ref["rightIdxs"], got["rightIdxs"])
    assert np.array_equal(ref["leftIdxs"], got["leftIdxs"])
    assert np.array_equal(ref["close"], got["close"])
    assert np.array_equal(ref["depth"].view(np.uint32), got["depth"].view(np.uint32))
    assert (got["candidates"], got["sad"], got["matches"]) == (0, 0, 0)


@pytest.mark.parametrize("name", sorted(FIN))
def test_stereo_finalize_direct(oracle, capi, name):
    """k_stereo_finalize alone: accepted-pair counts around the 1 % steps and the LDS limit, equal depths straddling the
    cut, the SAD cut at its edges, many-to-one with mixed drops, holes.  The compaction order inside the kernel is decided
    by LDS atomics, so each case is launched three times and must return identical bytes."""
    best, depth, sad, nR = FIN[name]
    ctx = sc.context(oracle, "euroc", 9)
    m = _gpu_pair(capi, ctx)
    ref = oracle.stereo_finalize(best, depth, sad, nR, ctx.rig)
    runs = []
    for _ in range(3):
        m.stereo_finalize_arrays(best, depth, sad, nR)
        got = m.stereo_fetch(len(best), nR)
        runs.append(b"".join(got[f].tobytes() for f in ("rightIdxs", "leftIdxs", "depth", "close")))
        _assert_same_finalize(ref, got)
    assert runs[0] == runs[1] == runs[2]
    print(name, "accepted", int((best >= 0).sum()), "kept", int((ref["rightIdxs"] >= 0).sum()))


def test_stereo_finalize_errors(oracle, capi):
    """capacity and argument errors of the direct entry; the matcher keeps working after each"""
    ctx = sc.context(oracle, "euroc", 9)
    m = _gpu_pair(capi, ctx)
    n = sc.STEREO_MAX_L + 1

    def status(best, depth, sad, nR, nL=None):
        with pytest.raises(capi.VslamError) as e:
            m.stereo_finalize_arrays(best, depth, sad, nR, nL)
        return e.value.status

    zeros = lambda k: (np.zeros(k, np.int32), np.ones(k, np.float32), np.zeros(k, np.int32))
    assert status(*zeros(n), 10) == capi.ERR_CAPACITY                      # one above the LDS limit
    assert status(*zeros(70000), 10) == capi.ERR_CAPACITY                  # above 65535 keys
    assert status(*zeros(10), 65536) == capi.ERR_CAPACITY                  # ... on the right side
    b, d, s = zeros(10)
    b[7] = 5
    assert status(b, d, s, 5) == capi.ERR_INVALID                          # best[i] >= nR
    assert status(b, d, s, 0) == capi.ERR_INVALID
    assert status(*zeros(1), 5, nL=-1) == capi.ERR_INVALID
    assert status(*zeros(1), -1) == capi.ERR_INVALID
    best, depth, sad, nR = FIN["tie_depth"]
    m.stereo_finalize_arrays(best, depth, sad, nR)
    _assert_same_finalize(oracle.stereo_finalize(best, depth, sad, nR, ctx.rig), m.stereo_fetch(len(best), nR))


def test_stereo_full_path_at_left_key_limit(oracle, capi):
    """7680 left keys (the dynamic-LDS limit) through the full path: tiled crafted keys, so that hundreds of left keys
    share each right key and equal depths straddle the 1 % cut.  One more key is a capacity error, and so are more
    than 65535 keys; the matcher works on afterwards."""
    images, kL, dL, kR, dR, c = sc.tiled_case(oracle, "euroc", sc.STEREO_MAX_L)
    assert len(kL) == sc.STEREO_MAX_L
    m = _gpu_pair(capi, c.ctx)
    ref = oracle.stereo_match(c.ctx.exL, c.ctx.exR, c.ctx.rig, kL, dL, kR, dR)
    n, endDe, cut, less, equal, quota = sc.depth_cut(ref["preBest"], ref["preDepth"])
    assert n > 4000 and 0 < quota < equal
    _assert_same(ref, _full_path(m, kL, dL, kR, dR))
    # the same keys as the RIGHT side of a small left set: 7680 right keys, every left key meets hundreds of candidates
    images, kL1, dL1, kR1, dR1, c1 = sc.match_case(oracle, "many_to_one", "euroc")
    kRt, dRt = np.tile(kR1, 640), np.tile(dR1, (640, 1))
    assert len(kRt) == sc.STEREO_MAX_L
    _assert_same(oracle.stereo_match(c.ctx.exL, c.ctx.exR, c.ctx.rig, kL1, dL1, kRt, dRt), _full_path(m, kL1, dL1, kRt, dRt))
    # one key more
    kL2, dL2 = np.concatenate([kL, kL[:1]]), np.concatenate([dL, dL[:1]])
    m.set_keys(0, kL2, dL2)
    with pytest.raises(capi.VslamError) as e:
        m.stereo_match()
    assert e.value.status == capi.ERR_CAPACITY
    # more than 65535 keys: refused when they are handed over
    reps = 65536 // len(kL) + 1
    with pytest.raises(capi.VslamError) as e:
        m.set_keys(0, np.tile(kL, reps)[:65536], np.tile(dL, (reps, 1))[:65536])
    assert e.value.status == capi.ERR_CAPACITY
    with pytest.raises(capi.VslamError) as e:
        m.stereo_match()
    assert e.value.status == capi.ERR_CAPACITY
    _assert_same(ref, _full_path(m, kL, dL, kR, dR))
