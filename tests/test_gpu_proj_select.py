"""GPU parity of the window scan's two selections (scan_side in csrc/proj_dev.hpp): a window of at most 64 entries keeps one
key per lane and ranks the lanes' keys, a larger window (and every window of an un-bucketed grid) keeps a sorted list per lane
and merges the lanes.  Every case runs matchByProjectionRPred, matchByProjectionMono and matchByRadius through the C ABI with
the sparse selection (default) and with VSLAM_PROJ_SELECT=0 (general path only); both must give the oracle's match pairs and
claim tables bit for bit.

The returned test count is the number of Hamming tests of k_proj_candidates: candidates of every unmatched, in-frame map point
that pass the cell, octave and radius filters, claims IGNORED (the oracle's own count skips keys claimed earlier in the walk,
so it can only be smaller).  The tests restate that count in numpy (Grid.counts) and require it exactly on both paths; where no
window holds a key that another map point could claim (one map point per isolated window) the oracle's count must equal it too.
Frames are crafted (set_keys + the finalize tap with no stereo pairs) unless a case needs an extracted one."""
import os
import numpy as np
import pytest
import synth
from test_gpu_proj import _frontend, _make_mps

pytestmark = pytest.mark.gpu
RIG = synth.RIGS["euroc"]
RAD = 10.0
LEVEL = 2                  # crafted map points: radius 1.44 * 10 px, a window of 4 - 5 cells a side
# entries per crafted window: nothing, one, the K = 8 boundary, a quarter wave, the wave (the switch between the two selections)
# and a window that needs three passes of the general path
COUNTS = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 130]
CENTRES = [(94.0 + 188.0 * (i % 4), 80.0 + 160.0 * (i // 4)) for i in range(12)]      # windows far apart: no shared cell


class Grid:
    """the matching grid of a rig and the window of a prediction, in the float32 arithmetic of assignKeysToGrids / getMatchIdxs"""

    def __init__(self, rig, scale_pyramid):
        w, h = np.float32(rig["w"]), np.float32(rig["h"])
        self.xG = 64
        self.yG = int(np.ceil(np.float32(64) / (w / h)))
        self.xM, self.yM = np.float32(64) / w, np.float32(self.yG) / h
        self.sp = np.asarray(scale_pyramid, np.float32)

    def cells(self, x, y):
        cx = np.clip(np.rint(np.asarray(x, np.float32) * self.xM).astype(np.int64), 0, self.xG - 1)
        cy = np.clip(np.rint(np.asarray(y, np.float32) * self.yM).astype(np.int64), 0, self.yG - 1)
        return cx, cy

    def window(self, px, py, level, rad):
        px, py = np.float32(px), np.float32(py)
        r = self.sp[level] * np.float32(rad)
        x0 = max(0, int(np.floor((px - r) * self.xM))); x1 = min(self.xG - 1, int(np.ceil((px + r) * self.xM)))
        y0 = max(0, int(np.floor((py - r) * self.yM))); y1 = min(self.yG - 1, int(np.ceil((py + r) * self.yM)))
        return x0, x1, y0, y1, r

    def counts(self, k, px, py, level, rad, parallax=False):
        """(entries of the window, Hamming tests) of one prediction against the keys k, claims ignored"""
        x0, x1, y0, y1, r = self.window(px, py, level, rad)
        if x0 >= self.xG or y0 >= self.yG or x1 < 0 or y1 < 0 or len(k) == 0:
            return 0, 0
        cx, cy = self.cells(k["x"], k["y"])
        inw = (cx >= x0) & (cx <= x1) & (cy >= y0) & (cy <= y1)
        dx, dy = k["x"] - np.float32(px), k["y"] - np.float32(py)
        t = inw & (k["octave"] <= level + 1) & (k["octave"] >= level - 1) & (np.abs(dx) < r) & (np.abs(dy) < r)
        if parallax:
            t &= np.sqrt(dx.astype(np.float64) ** 2 + dy.astype(np.float64) ** 2) > 10.0
        return int(inw.sum()), int(t.sum())


def _both(fn):
    """[fn() with the sparse selection, fn() with VSLAM_PROJ_SELECT=0]"""
    outs = []
    for sw in (None, "0"):
        if sw is not None:
            os.environ["VSLAM_PROJ_SELECT"] = sw
        try:
            outs.append(fn())
        finally:
            os.environ.pop("VSLAM_PROJ_SELECT", None)
    return outs


def _keys(capi, xy, octs):
    k = np.zeros(len(xy), capi.KP_DTYPE)
    if len(xy):
        k["x"], k["y"] = np.asarray(xy, np.float32).reshape(-1, 2).T
    k["octave"] = octs
    k["size"], k["response"], k["class_id"] = 31.0, 1.0, -1
    return k


def _flip(rng, base, nbits):
    d = base.copy()
    for b in rng.choice(256, nbits, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _cluster(g, rng, cx, cy, level, n, rad=RAD, spread=22.0):
    """n key positions whose cells all lie inside the window of (cx, cy, level): the window holds exactly n entries, some of them
    outside the radius (visited, not tested)"""
    x0, x1, y0, y1, _ = g.window(cx, cy, level, rad)
    out = []
    while len(out) < n:
        x, y = np.float32(cx + rng.uniform(-spread, spread)), np.float32(cy + rng.uniform(-spread, spread))
        c = g.cells([x], [y])
        if x0 <= c[0][0] <= x1 and y0 <= c[1][0] <= y1:
            out.append((x, y))
    return out


def _side(capi, g, rng, counts, bases, shift, max_flip=90, same=False):
    """one side's keys: cluster i of counts[i] keys around CENTRES[i] (+ shift in x), descriptors = bases[i] with up to max_flip
    flipped bits (same: one descriptor per cluster - every distance of the cluster is equal), octaves LEVEL - 2 .. LEVEL + 2"""
    xy, octs, desc = [], [], []
    for (cx, cy), n, base in zip(CENTRES, counts, bases):
        pts = _cluster(g, rng, cx + shift, cy, LEVEL, n)
        xy += pts
        octs += list(rng.integers(LEVEL - 2, LEVEL + 3, n))
        one = _flip(rng, base, 20)
        desc += [one if same else _flip(rng, base, int(rng.integers(0, max_flip))) for _ in range(n)]
    order = rng.permutation(len(xy))            # key index order unrelated to the clusters
    k = _keys(capi, np.array(xy, np.float32).reshape(-1, 2)[order], np.array(octs, np.int32)[order])
    return k, np.array(desc, np.uint8).reshape(-1, 32)[order]


def _mps_at(oracle, bases, shift, per=1):
    """`per` map points on every cluster centre (left prediction on the centre, right one `shift` px beside it)"""
    mps = np.zeros(len(CENTRES) * per, oracle.MPV_DTYPE)
    for i, ((cx, cy), base) in enumerate(zip(CENTRES, bases)):
        s = slice(i * per, (i + 1) * per)
        mps["desc"][s] = base
        mps["predLx"][s], mps["predLy"][s], mps["predRx"][s], mps["predRy"][s] = cx, cy, cx + shift, cy
    mps["scaleLevelL"] = mps["scaleLevelR"] = LEVEL
    mps["inFrame"] = mps["inFrameR"] = 1
    return mps


@pytest.fixture(scope="module")
def crafted(oracle, capi):
    """one extractor / matcher pair for every crafted frame (the extractor never runs: both key sets are overridden)"""
    ge = capi.Extractor(RIG["w"], RIG["h"], 1500, batch=2)
    m = capi.Matcher(RIG, ge, 0, ge, 1)
    oL = oracle.Extractor(1500)
    return m, oL, Grid(RIG, oL.scalePyramid)


@pytest.fixture(scope="module")
def extracted(oracle, capi):
    """one extracted euroc frame with its stereo pairs, shared by the cases that need real keys"""
    rig, oL, keys, st, ge, m = _frontend(oracle, capi)
    return rig, oL, keys, st, ge, m, Grid(rig, oL.scalePyramid)


def _load(m, kL, dL, kR, dR):
    """a crafted frame without stereo pairs"""
    nL = len(kL)
    m.stereo_finalize_arrays(np.full(nL, -1, np.int32), np.full(nL, -1, np.float32), np.zeros(nL, np.int32), len(kR))
    m.set_keys(0, kL, dL)
    m.set_keys(1, kR, dR)
    st = m.stereo_fetch(nL, len(kR))
    assert (st["rightIdxs"] == -1).all() and (st["leftIdxs"] == -1).all()
    return st


def _expected_tests(g, mps, mt0, kL, kR, rad):
    """Hamming tests of k_proj_candidates: (stereo call, mono call)"""
    tl = tr = 0
    for i, p in enumerate(mps):
        if mt0[i, 0] >= 0 or mt0[i, 1] >= 0:
            continue
        if p["inFrame"]:
            tl += g.counts(kL, p["predLx"], p["predLy"], int(p["scaleLevelL"]), rad)[1]
        if p["inFrameR"]:
            tr += g.counts(kR, p["predRx"], p["predRy"], int(p["scaleLevelR"]), rad)[1]
    return tl + tr, tl


def _check_all(oracle, capi, rig, m, oL, g, kL, dL, kR, dR, st, mps, rad, mL0=None, mR0=None, oracle_count=False, min_matches=1):
    """the three entry points on both selections against the oracle; oracle_count: the oracle's test count must equal the
    library's (no window holds a key that an earlier map point claims)"""
    M = len(mps)
    mL0 = np.full(len(kL), -1, np.int32) if mL0 is None else mL0
    mR0 = np.full(len(kR), -1, np.int32) if mR0 is None else mR0
    mt0 = np.full((M, 2), -1, np.int32)
    want_s, want_m = _expected_tests(g, mps, mt0, kL, kR, rad)
    # matchByProjectionRPred
    ref = oracle.match_projection(oL, rig, mps, kL, dL, kR, dR, st["rightIdxs"], st["leftIdxs"], mL0, mR0, mt0, rad)
    assert ref[0] >= min_matches
    assert ref[4] <= want_s and (not oracle_count or ref[4] == want_s)
    for n, mL, mR, mt, nc in _both(lambda: capi.match_projection(m, mps, rad, mL0, mR0, mt0)):
        assert n == ref[0] and np.array_equal(mt, ref[3]) and np.array_equal(mL, ref[1]) and np.array_equal(mR, ref[2])
        assert nc == want_s
    # matchByProjectionMono
    ref = oracle.match_projection_mono(oL, rig, mps, kL, dL, mL0, mt0, rad)
    assert ref[3] <= want_m and (not oracle_count or ref[3] == want_m)
    for n, mL, mt, nc in _both(lambda: capi.match_projection_mono(m, mps, rad, mL0, mt0)):
        assert n == ref[0] and np.array_equal(mt, ref[2]) and np.array_equal(mL, ref[1])
        assert nc == want_m
    # matchByRadius: the "last keyframe" = the map points' left predictions, levels and descriptors
    lk = _keys(capi, np.stack([mps["predLx"], mps["predLy"]], 1), mps["scaleLevelL"])
    ld = np.ascontiguousarray(mps["desc"])
    ref = oracle.match_by_radius(oL, rig, lk, ld, kL, dL, mL0, rad)
    for n, mL, out in _both(lambda: capi.match_by_radius(m, lk, ld, rad, mL0)):
        assert n == ref[0] and np.array_equal(out, ref[2]) and np.array_equal(mL, ref[1])


def test_crafted_window_sizes(oracle, capi, crafted):
    """Windows of exactly 0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65 and 130 entries on the left side and the same counts in reverse
    order on the right side, one map point per window."""
    m, oL, g = crafted
    rng = np.random.default_rng(11)
    bases = [rng.integers(0, 256, 32).astype(np.uint8) for _ in CENTRES]
    kL, dL = _side(capi, g, rng, COUNTS, bases, 0.0)
    kR, dR = _side(capi, g, rng, COUNTS[::-1], bases, -20.0)
    st = _load(m, kL, dL, kR, dR)
    mps = _mps_at(oracle, bases, -20.0)
    for i, p in enumerate(mps):
        assert g.counts(kL, p["predLx"], p["predLy"], LEVEL, RAD)[0] == COUNTS[i]
        assert g.counts(kR, p["predRx"], p["predRy"], LEVEL, RAD)[0] == COUNTS[::-1][i]
    _check_all(oracle, capi, RIG, m, oL, g, kL, dL, kR, dR, st, mps, RAD, oracle_count=True, min_matches=6)


def test_equal_distances_order_by_cell_and_index(oracle, capi, crafted):
    """Every key of a cluster carries one descriptor, so every candidate of a window has the same Hamming distance and the order
    of the K best comes from (cell, index) alone; three map points per window walk down that order through the claims."""
    m, oL, g = crafted
    rng = np.random.default_rng(12)
    bases = [rng.integers(0, 256, 32).astype(np.uint8) for _ in CENTRES]
    counts = [3, 12, 70, 8, 9, 64, 65, 2, 16, 17, 30, 100]
    kL, dL = _side(capi, g, rng, counts, bases, 0.0, same=True)
    kR, dR = _side(capi, g, rng, counts[::-1], bases, -20.0, same=True)
    st = _load(m, kL, dL, kR, dR)
    _check_all(oracle, capi, RIG, m, oL, g, kL, dL, kR, dR, st, _mps_at(oracle, bases, -20.0, per=3), RAD, min_matches=6)


def test_window_edges_and_image_borders(oracle, capi, crafted):
    """Keys in the first and the last cell of every window row (with the window's own slice bounds), and windows clipped at each
    of the four image borders and corners."""
    m, oL, g = crafted
    rng = np.random.default_rng(13)
    w, h = RIG["w"], RIG["h"]
    spots = [(3, 3), (w - 3, 3), (3, h - 3), (w - 3, h - 3), (376, 2), (376, h - 2), (2, 240), (w - 2, 240), (300, 200), (130, 120), (600, 330)]
    xy, octs, desc, bases = [], [], [], []
    for (px, py) in spots:
        base = rng.integers(0, 256, 32).astype(np.uint8)
        bases.append(base)
        x0, x1, y0, y1, r = g.window(px, py, LEVEL, RAD)
        pts = []
        for cy in range(y0, y1 + 1):              # the row's first and last cell, at the cell centres
            pts += [(x0 / g.xM, cy / g.yM), (x1 / g.xM, cy / g.yM)]
        e = float(r) - 0.5                        # just inside the radius on either side, and around the prediction
        pts += [(px - e, py), (px + e, py), (px, py - e), (px, py + e)] + [(px + rng.uniform(-5, 5), py + rng.uniform(-5, 5)) for _ in range(3)]
        pts = [(min(max(x, 0.0), w - 1.0), min(max(y, 0.0), h - 1.0)) for x, y in pts]
        xy += pts
        octs += list(rng.integers(LEVEL - 1, LEVEL + 2, len(pts)))
        desc += [_flip(rng, base, int(rng.integers(0, 90))) for _ in pts]
    order = rng.permutation(len(xy))
    kL = _keys(capi, np.array(xy, np.float32)[order], np.array(octs, np.int32)[order])
    dL = np.array(desc, np.uint8)[order]
    kR, dR = kL.copy(), dL.copy()
    kR["x"] = np.maximum(kR["x"] - np.float32(4.0), 0)
    st = _load(m, kL, dL, kR, dR)
    mps = np.zeros(len(spots), oracle.MPV_DTYPE)
    for i, ((px, py), base) in enumerate(zip(spots, bases)):
        mps["desc"][i] = base
        mps["predLx"][i], mps["predLy"][i], mps["predRx"][i], mps["predRy"][i] = px, py, max(px - 4.0, 0.0), py
        x0, x1, y0, y1, _ = g.window(px, py, LEVEL, RAD)
        cx, cy = g.cells(kL["x"], kL["y"])
        rows = set(cy[(cx == x0) & (cy >= y0) & (cy <= y1)]) & set(cy[(cx == x1) & (cy >= y0) & (cy <= y1)])
        assert len(rows) == y1 - y0 + 1           # every row of the window has a key in its first and in its last cell
    mps["scaleLevelL"] = mps["scaleLevelR"] = LEVEL
    mps["inFrame"] = mps["inFrameR"] = 1
    _check_all(oracle, capi, RIG, m, oL, g, kL, dL, kR, dR, st, mps, RAD, min_matches=6)


def test_exhausted_lists_rescan_small_windows(oracle, capi, crafted):
    """Twenty map points on one spot with one descriptor, windows of 12, 40 and 64 entries and part of the keys claimed before the
    call: the later points find their eight-key lists claimed and k_proj_resolve rescans the window under the claim tables
    (scan_side<2>) - on the sparse selection here, the windows being at most a wave wide."""
    m, oL, g = crafted
    rng = np.random.default_rng(14)
    bases = [rng.integers(0, 256, 32).astype(np.uint8) for _ in CENTRES]
    counts = [12, 40, 64, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    kL, dL = _side(capi, g, rng, counts, bases, 0.0, max_flip=60)
    kR, dR = _side(capi, g, rng, counts, bases, -20.0, max_flip=60)
    kL["octave"] = rng.integers(LEVEL - 1, LEVEL + 2, len(kL))      # every entry inside the radius is a candidate: long lists;
    kR["octave"] = rng.integers(LEVEL - 1, LEVEL + 2, len(kR))      # mixed levels: the ratio test seldom applies, claims go on
    st = _load(m, kL, dL, kR, dR)
    mps = _mps_at(oracle, bases, -20.0, per=20)[:60]
    mL0 = np.where(rng.random(len(kL)) < 0.3, 7, -1).astype(np.int32)
    mR0 = np.where(rng.random(len(kR)) < 0.3, 7, -1).astype(np.int32)
    # the case does what it is for: under the claims the oracle ends with, a full left list of the three spots has fewer than two
    # unclaimed keys among its eight best - the spot's last map points could not decide from their lists
    ref = oracle.match_projection(oL, RIG, mps, kL, dL, kR, dR, st["rightIdxs"], st["leftIdxs"], mL0, mR0, np.full((60, 2), -1, np.int32), RAD)
    exhausted = 0
    cxs, cys = g.cells(kL["x"], kL["y"])
    for (cx, cy), base in list(zip(CENTRES, bases))[:3]:
        x0, x1, y0, y1, r = g.window(cx, cy, LEVEL, RAD)
        cand = np.nonzero((cxs >= x0) & (cxs <= x1) & (cys >= y0) & (cys <= y1) & (np.abs(kL["x"] - np.float32(cx)) < r) &
                          (np.abs(kL["y"] - np.float32(cy)) < r))[0]
        dist = np.unpackbits(dL[cand] ^ base, axis=1).sum(1)
        best8 = cand[np.lexsort((cand, cys[cand] * g.xG + cxs[cand], dist))][:8]
        exhausted += len(best8) == 8 and (ref[1][best8] < 0).sum() < 2
    assert exhausted >= 1
    _check_all(oracle, capi, RIG, m, oL, g, kL, dL, kR, dR, st, mps, RAD, mL0=mL0, mR0=mR0, min_matches=10)


def test_claim_exhaustion_whole_image_window(oracle, capi, extracted):
    """test_projection_claim_exhaustion_forces_rescan's shape: sixty map points share one descriptor and one spot with a radius that
    covers the image, so the rescans under claims run on the general path (more than 64 entries) whatever the switch says."""
    rig, oL, (kL, dL, kR, dR), st, ge, m, g = extracted
    M = 60
    mps = np.zeros(M, oracle.MPV_DTYPE)
    s = int(np.argmax(st["rightIdxs"] >= 0))
    mps["desc"][:] = dL[s]
    mps["predLx"], mps["predLy"] = kL["x"][s], kL["y"][s]
    mps["predRx"], mps["predRy"] = kR["x"][st["rightIdxs"][s]], kR["y"][st["rightIdxs"][s]]
    mps["scaleLevelL"] = mps["scaleLevelR"] = kL["octave"][s]
    mps["inFrame"] = mps["inFrameR"] = 1
    _check_all(oracle, capi, rig, m, oL, g, kL, dL, kR, dR, st, mps, 400.0)


def test_many_jobs_on_an_extracted_frame(oracle, capi, extracted):
    """More than 1 024 map points in one call (1 100 and 131 duplicates: 2 462 jobs, so the last workgroup has two idle waves; the
    sequential walk of k_proj_resolve), the tracker's two radii."""
    rig, oL, (kL, dL, kR, dR), st, ge, m, g = extracted
    rng = np.random.default_rng(15)
    mps = _make_mps(oracle, kL, dL, kR, dR, st, rng, 1100, 6.0, dup=131)
    assert (2 * len(mps)) % 4 == 2
    for rad in (10.0, 4.0):
        _check_all(oracle, capi, rig, m, oL, g, kL, dL, kR, dR, st, mps, rad, min_matches=100)


def test_unbucketed_portrait_rig(oracle, capi):
    """480 x 752: 101 grid rows, more than the bucket tables hold, so every lane strides over all keys of the side and the
    selection is the general one on both settings of the switch (test_projection_parity_portrait_rig's frame)."""
    rig = dict(synth.RIGS["euroc"], w=480, h=752, cx=240.0, cy=376.0)
    L = synth.random_image(rig["w"], rig["h"], 91)
    speckle = np.random.default_rng(92).random(L.shape) < 0.25
    R = np.minimum(np.roll(L, -12, axis=1).astype(np.int32) + speckle, 255).astype(np.uint8)
    oL, oR = oracle.Extractor(1500), oracle.Extractor(1500)
    kL, dL = oL.extract(L)
    kR, dR = oR.extract(R)
    st = oracle.stereo_match(oL, oR, rig, kL, dL, kR, dR)
    ge = capi.Extractor(rig["w"], rig["h"], 1500, batch=2)
    ge.extract([L, R])
    m = capi.Matcher(rig, ge, 0, ge, 1)
    m.stereo_match()
    g = Grid(rig, oL.scalePyramid)
    assert g.yG == 101
    mps = _make_mps(oracle, kL, dL, kR, dR, st, np.random.default_rng(16), 500, 6.0, dup=80)
    _check_all(oracle, capi, rig, m, oL, g, kL, dL, kR, dR, st, mps, RAD, min_matches=100)
