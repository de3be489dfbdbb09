"""GPU parity of k_ssc at the limits of its LDS size classes (3 072 / 6 144 / SSC_NMAX_MID / 16 384 candidates) against the
oracle's restatement of FeatureExtractor::ssc, bit-exact kept list in order - with the classes on (the default) and with
VSLAM_SSC_CLASSES=0 (the two classes 6 144 / 16 384 only).  Candidate kinds: `ties` (the tie order decides), `one_value` (every
partition splits evenly: the segment lists are at their fullest), `sorted` and `organ_pipe` (median-of-3 worst-ish cases: the
depth limit).  The oracle's result of a case is computed once and shared by both settings."""
import os
import re
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = [1920, 1600, 1333, 1111, 926, 772, 643, 536]
ROWS = [1200, 1000, 833, 694, 579, 482, 402, 335]
KINDS = ("ties", "one_value", "sorted", "organ_pipe")


def _const(name):
    src = open(os.path.join(ROOT, "gtsam-vslam_amd", "csrc", "extract_kernels.hpp")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


TINY, SMALL, MID, LDS = (_const(k) for k in ("SSC_NMAX_TINY", "SSC_NMAX_SMALL", "SSC_NMAX_MID", "SSC_NMAX_LDS"))
SIZES = (TINY - 1, TINY, TINY + 1, SMALL, SMALL + 1, MID - 1, MID, MID + 1, LDS)


def _cands(oracle, rng, n, cols, rows, kind, box=None):
    k = np.zeros(n, oracle.KP_DTYPE)
    if box is None:
        k["x"] = rng.integers(16, cols - 16, n); k["y"] = rng.integers(16, rows - 16, n)
    else:                                      # every candidate inside a box x box block
        k["x"] = rng.integers(cols // 2, cols // 2 + box, n); k["y"] = rng.integers(rows // 2, rows // 2 + box, n)
    if kind == "ties":
        k["response"] = rng.choice([7, 8, 20, 21], n)
    elif kind == "one_value":
        k["response"] = 30
    elif kind == "sorted":
        r = np.sort(rng.integers(7, 256, n))
        k["response"] = np.concatenate([r[: n // 2], r[n // 2:][::-1]])
    elif kind == "organ_pipe":
        h = n // 2
        k["response"] = np.concatenate([np.arange(h) * 248 // max(h, 1) + 7, (np.arange(n - h)[::-1]) * 248 // max(n - h, 1) + 7])
    elif kind == "uniform":
        k["response"] = rng.integers(7, 120, n)
    k["octave"] = 0; k["size"] = 31; k["angle"] = -1; k["class_id"] = -1
    return k


_REF = {}


def _case(oracle, level, n, kind, box=None):
    """(candidates, the oracle's kept list) of a case, computed once"""
    key = (level, n, kind, box)
    if key not in _REF:
        rng = np.random.default_rng(1000 * level + n + 7 * KINDS.index(kind) if kind in KINDS else n)
        cand = _cands(oracle, rng, n, COLS[level], ROWS[level], kind, box)
        oe = oracle.Extractor(4000)
        assert n > oe.featurePerLevel[level]
        ref = oe.ssc(cand, int(oe.featurePerLevel[level]), 0.1, COLS[level], ROWS[level])
        for a in (cand, ref):
            a.flags.writeable = False
        _REF[key] = (cand, ref)
    return _REF[key]


_GE = {}


def _extractor(capi, classes):
    """one 1920x1200 / 4000-feature extractor per setting (the variable is read when an extractor is created)"""
    if classes not in _GE:
        os.environ["VSLAM_SSC_CLASSES"] = "3" if classes else "0"
        try:
            _GE[classes] = capi.Extractor(1920, 1200, 4000, batch=2)
        finally:
            os.environ.pop("VSLAM_SSC_CLASSES", None)
    return _GE[classes]


def _check(ge, level, cand, ref):
    got = ge.ssc_level(level, cand)
    assert len(got) == len(ref), (len(got), len(ref))
    for f in ("x", "y", "response"):
        assert np.array_equal(got[f], ref[f]), f
    assert ge.ssc_stats() == (1, 0)


@pytest.mark.parametrize("classes", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_ssc_parity_at_class_limits(oracle, capi, n, classes):
    ge = _extractor(capi, classes)
    for kind in KINDS:
        cand, ref = _case(oracle, 0, n, kind)
        _check(ge, 0, cand, ref)


@pytest.mark.parametrize("classes", [True, False])
@pytest.mark.parametrize("box", [100, 200])
def test_ssc_small_class_probes_beyond_a_slice(oracle, capi, box, classes):
    """Level 5 of the 1920x1200 rig (772x482, 349 kept of 3 000: the 3 072 class), every candidate inside a box x box block.  Two
    picks of a probe are more than two cells apart, so a probe of width w keeps at most (ceil((2 box / w + 2) / 3))^2 of them:
    for w >= 12 that is 36 (box 100) / 144 (box 200), below the 314 the search accepts.  Every probe it can end on is finer,
    and the bit grid of width 11 is already (2 * 482 / 11 + 1) x 5 = 440 words against the 416 a probing wave's 2 KB slice leaves
    beside its pick words: the search has to go through the solo probe on the whole arena (box 200: ends near width 6) and,
    for grids beyond the arena's 4 000 words (box 100: near width 3, 5 474 words), through the task's HBM grid."""
    w = 12
    assert (-(-(2 * box // w + 2) // 3)) ** 2 < 314
    assert (2 * ROWS[5] // 11 + 1) * ((2 * COLS[5] // 11 + 1 + 31) // 32) > 4096 // 8 - TINY // 32
    cand, ref = _case(oracle, 5, 3000, "uniform", box)
    assert 314 <= len(ref) <= 384              # the search ended on an accepted probe (349 -+ 10 %)
    _check(_extractor(capi, classes), 5, cand, ref)


@pytest.mark.parametrize("classes", [True, False])
def test_whole_frame_with_classes(oracle, capi, monkeypatch, classes):
    """One whole 752x480 frame (1 427 ... 356 candidates per level: every level in the 3 072 class, or in the 6 144 class with
    the classes off); identical keypoints and descriptors."""
    import synth
    img = synth.random_image(752, 480, 4321)
    monkeypatch.setenv("VSLAM_SSC_CLASSES", "3" if classes else "0")
    ge = capi.Extractor(752, 480, 1500)
    (gk, gd), = ge.extract([img])
    key = ("frame",)
    if key not in _REF:
        _REF[key] = oracle.Extractor(1500).extract(img)
    ok, od = _REF[key]
    assert len(gk) == len(ok) > 1000
    for f in ok.dtype.names:
        assert np.array_equal(ok[f], gk[f]), f
    assert np.array_equal(od, gd)
    assert ge.ssc_stats() == (1, 0)
    ge.close()


def test_ssc_class_bounds():
    """the header's limits are the ones these tests step across"""
    assert (TINY, SMALL, LDS) == (3072, 6144, 16384) and SMALL < MID < LDS and MID % 256 == 0
