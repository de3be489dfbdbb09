"""k_blur on crafted images: EVERY level of every case, the blurred level the extractor holds against the oracle's blur of the
unblurred level it holds (so the comparison does not depend on the resize, nor on a keypoint happening to lie on the level).

What the images pin: the REFLECT_101 byte-permute selectors of the left border and of the right border (m = w - x = 1 .. 7 of
the last thread column, which the level widths' w % 4 of 0, 1, 2, 3 select) on extreme values and on single impulses next to
each border; the (acc + 32768) >> 16 rounding at all-255; the byte tail of the store when x + 4 > w; a second 256-px tile that
holds one thread column; the row reflection at the top and at the bottom for tile heights that end on, just after and just
before a 16-row boundary."""
import numpy as np
import pytest
import synth
from test_gpu_fast_packed import _saturated

SIZES = [(640, 480), (401, 263), (334, 258), (343, 260)]


def _level_sizes(w, h, nlevels=8, scale=1.2):
    out, s = [], np.float32(1.0)
    for l in range(nlevels):
        if l:
            s = np.float32(s * np.float32(scale))
        inv = np.float32(1.0) / s
        out.append((int(np.rint(np.float32(w) * inv)), int(np.rint(np.float32(h) * inv))))
    return out


def test_blur_sizes_cover_the_kernel_paths():
    """CPU only."""
    assert sorted(w % 4 for w, _ in SIZES) == [0, 1, 2, 3]          # level 0, where the impulses are single pixels
    lv = [s for sz in SIZES for s in _level_sizes(*sz)]
    assert set(w % 4 for w, _ in lv) == {0, 1, 2, 3}
    assert any(257 <= w <= 260 for w, _ in lv)                       # a second 256-px tile of one thread column
    assert any(w % 64 == 0 for w, _ in lv)                           # pitch == w
    assert {0, 1, 15} <= set(h % 16 for _, h in lv)
    assert any(1 <= h % 64 <= 2 for _, h in lv)                      # a last tile row of one or two image rows


def _images(w, h, seed):
    """[(name, image, flat)]"""
    yy, xx = np.mgrid[0:h, 0:w]
    out = [("zeros", np.zeros((h, w), np.uint8), True), ("255", np.full((h, w), 255, np.uint8), True),
           ("checkerboard", (((xx + yy) & 1) * 255).astype(np.uint8), False),
           ("vertical stripes", ((xx & 1) * 255).astype(np.uint8), False),
           ("horizontal stripes", ((yy & 1) * 255).astype(np.uint8), False),
           ("saturated", _saturated(w, h, seed), False)]
    pos = [(x, h // 2) for x in list(range(8)) + list(range(w - 8, w))]
    pos += [(w // 2, y) for y in list(range(7)) + list(range(h - 7, h))]
    pos += [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]
    for x, y in pos:
        im = np.zeros((h, w), np.uint8)
        im[y, x] = 255
        out.append(("impulse at (%d, %d)" % (x, y), im, False))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_blur_every_level_on_crafted_images(oracle, capi, w, h):
    cases = _images(w, h, 11)
    ge = capi.Extractor(w, h, 600, batch=len(cases))
    res = ge.extract([im for _, im, _ in cases])
    sizes = _level_sizes(w, h)
    for i, (name, im, flat) in enumerate(cases):
        if flat:                                   # no corner anywhere: the frame is empty, the levels are there all the same
            assert len(res[i][0]) == 0 and res[i][1].shape == (0, 32), name
        for l in range(8):
            src, got = ge.level(i, l), ge.level(i, l, blurred=True)
            assert src.shape == (sizes[l][1], sizes[l][0])
            if l == 0:
                assert np.array_equal(src, im), name
            want = oracle.blur(src)
            bad = np.argwhere(got != want)
            assert len(bad) == 0, "%s, %dx%d level %d (%dx%d): %d pixels differ, first (x, y) = (%d, %d)" % (
                name, w, h, l, sizes[l][0], sizes[l][1], len(bad), bad[0][1], bad[0][0])
            if name == "255":
                assert src.min() == 255 and got.min() == 255, "level %d" % l
            if name == "zeros":
                assert got.max() == 0, "level %d" % l
    ge.close()
