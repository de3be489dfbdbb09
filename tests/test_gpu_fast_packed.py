"""k_fast's packed stages against the CPU oracle, bit-exact, on inputs chosen for what packed arithmetic can get wrong:
centres whose v - t / v + t leave the pixel range, every byte phase of a cell's first column and every row-length remainder,
both thresholds, the full-scan fallback, and a batch of 16 different images (the XCD image mapping of nimg >= 8).
The comparison is the one of tests/test_gpu_extract.py::_compare: per level the candidates (x, y, response, octave, size, order),
then the kept keypoints and the descriptors."""
import numpy as np
import pytest
import synth

SIZES = [(752, 480), (333, 257), (401, 263), (334, 258), (371, 300), (343, 260)]


def _compare(oracle, capi, img, nfeat):
    h, w = img.shape
    oe = oracle.Extractor(nfeat)
    ok, od = oe.extract(img)
    ge = capi.Extractor(w, h, nfeat)
    (gk, gd), = ge.extract([img])
    ncand = 0
    for l in range(8):
        assert np.array_equal(ge.level(0, l), oe.level(l)), "pyramid level %d" % l
        oc, gc = oe.fast_candidates(l), ge.candidates(0, l)
        assert len(oc) == len(gc), "level %d candidate count %d vs %d" % (l, len(oc), len(gc))
        for f in ("x", "y", "response", "octave", "size"):
            assert np.array_equal(oc[f], gc[f]), "level %d candidates field %s" % (l, f)
        ncand += len(oc)
    assert len(ok) == len(gk)
    for f in ok.dtype.names:
        assert np.array_equal(ok[f], gk[f]), "keypoint field %s" % f
    assert np.array_equal(od, gd)
    ge.close()
    return oe, ncand


def _cell_phases(w, h, nlevels=8, scale=1.2, edge=19):
    """(cStart & 3, detW & 3) of every cell k_fast processes, from the geometry of vslam_extractor::init and k_fast."""
    out = set()
    s = np.float32(1.0)
    for l in range(nlevels):
        if l:
            s = np.float32(s * np.float32(scale))
        inv = np.float32(1.0) / s
        wl, hl = int(np.rint(np.float32(w) * inv)), int(np.rint(np.float32(h) * inv))
        mn = edge - 3
        maxX, maxY = wl - mn, hl - mn
        wid, hig = maxX - mn, maxY - mn
        nC, nR = int(np.float32(wid) / np.float32(35.0)), int(np.float32(hig) / np.float32(35.0))
        gW, gH = int(np.ceil(np.float32(wid) / np.float32(nC))), int(np.ceil(np.float32(hig) / np.float32(nR)))
        for iR in range(nR):
            for iC in range(nC):
                rS, cS = mn + iR * gH, mn + iC * gW
                if rS >= maxY - 6 or cS >= maxX - 6:
                    continue
                detW, detH = min(cS + gW + 6, maxX) - cS - 6, min(rS + gH + 6, maxY) - rS - 6
                if detW > 0 and detH > 0:
                    out.add((cS & 3, detW & 3))
    return out


def test_sizes_cover_every_byte_phase_and_row_remainder():
    """CPU only: the cells of SIZES cover all 16 combinations of (first column & 3, detection width & 3)."""
    seen = set()
    for w, h in SIZES:
        seen |= _cell_phases(w, h)
    assert len(seen) == 16, sorted(seen)
    assert len(set().union(*[_cell_phases(w, h) for w, h in SIZES[:5]])) == 15


def _saturated(w, h, seed):
    r = synth.random_image(w, h, seed).astype(np.int32)
    return np.where(r > 128, 255 - r % 13, r % 13).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,seed", [(401, 263, 5), (371, 300, 6)])
def test_fast_saturated_centres(oracle, capi, w, h, seed):
    """Every corner centre is below 20 or above 235: v - 20 < 0 or v + 20 > 255 for each of them."""
    img = _saturated(w, h, seed)
    oe, ncand = _compare(oracle, capi, img, 600)
    c0 = oe.fast_candidates(0)
    v = img[c0["y"].astype(np.int64), c0["x"].astype(np.int64)].astype(np.int32)
    print("saturation %dx%d: %d candidates, level 0: %d below 20, %d above 235" % (w, h, ncand, (v < 20).sum(), (v > 235).sum()))
    assert (v < 20).sum() >= 200 and (v > 235).sum() >= 200


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_fast_alignment_and_row_remainders(oracle, capi, w, h):
    _compare(oracle, capi, synth.random_image(w, h, 17), 600)


def _low_contrast(w, h, k):
    img = synth.random_image(w, h, 33).astype(np.float32)
    return np.clip(128 + (img - 128) * k, 0, 255).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(752, 480), (401, 263)])
@pytest.mark.parametrize("k", [0.18, 0.10])
def test_fast_second_threshold_pass(oracle, capi, w, h, k):
    """Low contrast: the candidates come from the threshold-7 pass of cells that are empty at 20 (response below 20)."""
    oe, ncand = _compare(oracle, capi, _low_contrast(w, h, k), 1500)
    low = sum(int((oe.fast_candidates(l)["response"] < 20).sum()) for l in range(8))
    print("contrast %.2f %dx%d: %d candidates, %d with response below 20" % (k, w, h, ncand, low))
    assert low >= 100


@pytest.mark.gpu
def test_fast_full_scan_fallback_odd_rows(oracle, capi, monkeypatch):
    """VSLAM_FAST_LIST_CAP=4: the full-scan suppression on cells whose detection width is not a multiple of four."""
    assert any(d for _, d in _cell_phases(401, 263))
    monkeypatch.setenv("VSLAM_FAST_LIST_CAP", "4")
    _compare(oracle, capi, synth.random_image(401, 263, 55), 600)


@pytest.mark.gpu
def test_fast_batch_of_16_different_images(oracle, capi):
    imgs = [synth.random_image(401, 263, 200 + i) if i % 3 else _saturated(401, 263, 200 + i) for i in range(16)]
    ge = capi.Extractor(401, 263, 600, batch=16)
    res = ge.extract(imgs)
    oe = oracle.Extractor(600)
    for i, (img, (gk, gd)) in enumerate(zip(imgs, res)):
        ok, od = oe.extract(img)
        for l in range(8):
            oc, gc = oe.fast_candidates(l), ge.candidates(i, l)
            assert len(oc) == len(gc), "slot %d level %d candidate count %d vs %d" % (i, l, len(oc), len(gc))
            for f in ("x", "y", "response", "octave", "size"):
                assert np.array_equal(oc[f], gc[f]), "slot %d level %d candidates field %s" % (i, l, f)
        assert len(ok) == len(gk), "slot %d" % i
        for f in ok.dtype.names:
            assert np.array_equal(ok[f], gk[f]), "slot %d keypoint field %s" % (i, f)
        assert np.array_equal(od, gd), "slot %d" % i
    ge.close()
