"""k_orient_desc alone, through the describe tap (vslam_extractor_describe), on crafted patches - bit-exact against the oracle:
angle, x, y, size, response, octave and the 32 descriptor bytes.

  exact angles   tiles whose disc moments are set exactly: the origin, the axes, the diagonals (the ax >= ay tie of fastAtan2)
                 and the smallest angles next to each axis, among them the largest angle below 360 the moments allow (the
                 k == 4 edge of the kernel's range reduction);
  sweep          720 ramps half a degree apart: every 1-degree bin of the angle;
  flip cases     tests/golden/orient_flip_cases.json: the angles at which cosf / sinf of the host libm and float(cos(double))
                 rotate a pattern offset onto different pixels (tests/test_orient_census.py) - the kernel must follow the
                 double route (the CPU companion, test_flip_cases_separate_the_two_routes, shows that the two routes really give
                 different descriptors on these tiles);
  positions      the four extreme legal positions of every level and runs of 8 consecutive x at both ends (all byte phases
                 of the kernel's aligned patch staging), in the LAST image slot of a batch, under poisoned allocations;
  refusals       of the tap itself;  tap == pipeline on a noise image."""
import ctypes as C
import numpy as np
import pytest
import synth
import orient_tiles as ot

FLIP_SEED = 22         # of seeds 1..40 the one whose textures tell the two trig routes apart on the most tiles (28 of 84)
POS_SIZES = [(640, 480), (401, 263), (334, 258)]


def _level_sizes(w, h, nlevels=8, scale=1.2):
    out, s = [], np.float32(1.0)
    for l in range(nlevels):
        if l:
            s = np.float32(s * np.float32(scale))
        inv = np.float32(1.0) / s
        out.append((int(np.rint(np.float32(w) * inv)), int(np.rint(np.float32(h) * inv))))
    return out


def _describe_level0(oracle, capi, img, centres, nfeat=600):
    """describe the tile centres of `img` on level 0 -> (got, want, oracle extractor)"""
    h, w = img.shape
    oe = oracle.Extractor(nfeat)
    oe.extract(img)
    want = ot.oracle_keys(oracle, oe, oe.level(0), 0, centres)
    ge = capi.Extractor(w, h, nfeat)
    ge.extract([img])
    got = ge.describe(0, 0, ot.query(capi, centres))
    ge.close()
    return got, want, oe


# ---------------------------------------------------------------------------------------------------------------- exact angles
def _exact_cases(umax):
    rng = np.random.default_rng(7)
    probe = ot.sym_texture(rng)
    big = min(ot.capacity(probe, umax, sw, sg) for sw in (False, True) for sg in (1, -1)) * 3 // 4
    a = 1000
    cases = [(0, 0), (a, 0), (-a, 0), (0, a), (0, -a), (a, a), (a, -a), (-a, a), (-a, -a), (1, 1), (-1, -1),
             (big, -1), (big, 1), (-big, 1), (-big, -1), (1, big), (-1, big), (1, -big), (-1, -big)]
    return cases, big


def test_exact_angle_tiles_hit_their_moments(oracle):
    """CPU only: the construction of the tiles (what the GPU test relies on)."""
    oe = oracle.Extractor(600)
    umax = [int(v) for v in oe.umax]
    cases, big = _exact_cases(umax)
    assert big >= 50000
    rng = np.random.default_rng(7)
    for m10, m01 in cases:
        t = ot.set_moments(ot.sym_texture(rng), m10, m01, umax)
        assert ot.moments(t, umax) == (m10, m01)


@pytest.mark.gpu
def test_exact_angles(oracle, capi):
    oe0 = oracle.Extractor(600)
    umax = [int(v) for v in oe0.umax]
    cases, big = _exact_cases(umax)
    rng = np.random.default_rng(7)
    tiles = [ot.set_moments(ot.sym_texture(rng), m10, m01, umax) for m10, m01 in cases]
    for t, c in zip(tiles, cases):
        assert ot.moments(t, umax) == c
    img, centres = ot.mosaic(tiles, 5)
    got, want, oe = _describe_level0(oracle, capi, img, centres)
    ang = dict(zip(cases, want[0]["angle"]))
    for c in cases:                                      # each tile has its intended angle: the polynomial of its moments
        assert np.float32(oracle.fast_atan2(float(c[1]), float(c[0]))).view(np.uint32) == ang[c].view(np.uint32), c
    assert ang[(0, 0)] == 0.0 and ang[(1000, 0)] == 0.0 and ang[(0, 1000)] == 90.0 and ang[(-1000, 0)] == 180.0 and ang[(0, -1000)] == 270.0
    for c in [(1000, 1000), (1, 1)]:
        assert 44.9 < ang[c] < 45.1
    # the largest angle these moments allow: below 360, and the kernel's reduction takes k = rint(ang * 2 / pi) = 4 for it
    top = ang[(big, -1)]
    assert top == max(ang.values()) and 359.99 < top < 360.0
    rad = np.float32(top * np.float32(np.float32(np.pi) / np.float32(180.0)))
    assert np.rint(np.float64(rad) * 6.36619772367581382433e-01) == 4.0
    print("exact angles: big = %d, top angle %.6f, (big, +1) -> %.6g" % (big, top, ang[(big, 1)]))
    ot.assert_same(got, want, "exact angles")


# ----------------------------------------------------------------------------------------------------------------------- sweep
def _ramp_tiles(i0, i1):
    rng = np.random.default_rng(100 + i0)
    u = np.arange(ot.TILE) - ot.C
    uu, vv = np.meshgrid(u, u)
    tiles = []
    for i in range(i0, i1):
        th = np.deg2rad(0.5 * i)
        ramp = np.rint(2.0 * (uu * np.cos(th) + vv * np.sin(th))).astype(np.int64)
        tiles.append(128 + ramp + (ot.sym_texture(rng) - 120) // 2)
    return tiles


@pytest.mark.gpu
def test_angle_sweep(oracle, capi):
    bins = set()
    for i0 in range(0, 720, 120):
        img, centres = ot.mosaic(_ramp_tiles(i0, i0 + 120), 12)
        got, want, _ = _describe_level0(oracle, capi, img, centres)
        ot.assert_same(got, want, "sweep tiles %d.." % i0)
        bins |= set(int(a) % 360 for a in want[0]["angle"])
    assert bins == set(range(360)), sorted(set(range(360)) - bins)


# ------------------------------------------------------------------------------------------------------------------ flip cases
def _flip_setup(oracle):
    oe = oracle.Extractor(600)
    umax = [int(v) for v in oe.umax]
    cases, img, centres = ot.flip_image(FLIP_SEED, umax)
    oe.extract(img)
    return oe, cases, img, centres


def test_flip_cases_separate_the_two_routes(oracle):
    """CPU only: every tile has exactly the recorded angle, and on at least 20 of them the oracle's double route and the
    float route of the host libm give different descriptors - so the GPU test below can tell which one the kernel follows."""
    oe, cases, img, centres = _flip_setup(oracle)
    dbl = ot.oracle_keys(oracle, oe, oe.level(0), 0, centres)
    flt = ot.oracle_keys(oracle, oe, oe.level(0), 0, centres, trig="float")
    for c, a in zip(cases, dbl[0]["angle"]):
        assert int(a.view(np.uint32)) == int(c["angle_bits"], 16), c
    differ = int((dbl[1] != flt[1]).any(axis=1).sum())
    print("flip cases: %d tiles, descriptors differ between the routes on %d" % (len(cases), differ))
    assert differ >= 20


@pytest.mark.gpu
def test_flip_cases_follow_the_double_route(oracle, capi):
    oe, cases, img, centres = _flip_setup(oracle)
    assert len(cases) >= 20
    want = ot.oracle_keys(oracle, oe, oe.level(0), 0, centres)
    for c, a in zip(cases, want[0]["angle"]):
        assert int(a.view(np.uint32)) == int(c["angle_bits"], 16), c
    h, w = img.shape
    ge = capi.Extractor(w, h, 600)
    ge.extract([img])
    got = ge.describe(0, 0, ot.query(capi, centres))
    ge.close()
    ot.assert_same(got, want, "flip cases")


# ----------------------------------------------------------------------------------------------------- positions and byte phases
def _position_points(w, h):
    pts = [(19, 19), (w - 20, 19), (19, h - 20), (w - 20, h - 20)]
    for y in (19, h // 2, h - 20):
        pts += [(19 + i, y) for i in range(8)] + [(w - 27 + i, y) for i in range(8)]
    return pts


def test_position_sizes_cover_every_width_residue_and_pitch_equal_width():
    """CPU only."""
    assert POS_SIZES[0][0] % 64 == 0                     # level 0: pitch == w, the patch of x = w - 20 runs into the next row
    res = set(w % 4 for s in POS_SIZES for w, _ in _level_sizes(*s))
    assert res == {0, 1, 2, 3}
    for s in POS_SIZES:
        for w, h in _level_sizes(*s):
            xs = [x for x, _ in _position_points(w, h)]
            assert set((x - 19) & 3 for x in xs) == {0, 1, 2, 3} and set((x - 15) & 3 for x in xs) == {0, 1, 2, 3}
            assert min(xs) == 19 and max(xs) == w - 20


_pos_cache = {}


def _positions_oracle(oracle, w, h):
    if (w, h) not in _pos_cache:
        img = synth.random_image(w, h, 29)
        oe = oracle.Extractor(600)
        oe.extract(img)
        want = []
        for l, (wl, hl) in enumerate(_level_sizes(w, h)):
            lv = oe.level(l)
            assert lv.shape == (hl, wl)
            want.append(ot.oracle_keys(oracle, oe, lv, l, _position_points(wl, hl), response=l + 1))
        _pos_cache[(w, h)] = (img, want)
    return _pos_cache[(w, h)]


def _positions_gpu(capi, w, h, img):
    ge = capi.Extractor(w, h, 600, batch=2)             # slot 1: its last level ends the pyramid allocations
    ge.extract([synth.random_image(w, h, 30), img])
    got = []
    for l, (wl, hl) in enumerate(_level_sizes(w, h)):
        got.append(ge.describe(1, l, ot.query(capi, _position_points(wl, hl), response=l + 1)))
    ge.close()
    return got


@pytest.fixture
def poison(capi):
    L = capi.lib()
    L.vslam_debug_poison.restype = None

    def set_byte(b):
        L.vslam_debug_poison(C.c_int32(b))
    yield set_byte
    set_byte(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [0xA5, 0xFF])
@pytest.mark.parametrize("w,h", POS_SIZES)
def test_extreme_positions_and_byte_phases_under_poison(oracle, capi, poison, w, h, fill):
    img, want = _positions_oracle(oracle, w, h)
    plain = _positions_gpu(capi, w, h, img)
    poison(fill)
    got = _positions_gpu(capi, w, h, img)
    for l in range(8):
        ot.assert_same(got[l], want[l], "%dx%d level %d fill 0x%02x" % (w, h, l, fill))
        ot.assert_same(got[l], plain[l], "%dx%d level %d fill 0x%02x against the unpoisoned run" % (w, h, l, fill))


# -------------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.gpu
def test_describe_refusals(capi):
    w, h = 401, 263
    ge = capi.Extractor(w, h, 100)
    ok = ot.query(capi, [(30, 30), (40, 40), (50, 50), (60, 60)])
    with pytest.raises(capi.VslamError) as e:            # before run(): no pyramid yet
        ge.describe(0, 0, ok)
    assert e.value.status == capi.ERR_INVALID and "not run" in str(e.value)
    ge.extract([synth.random_image(w, h, 3)])
    sizes = _level_sizes(w, h)
    for l in (0, 3, 7):
        wl, hl = sizes[l]
        for bad in [(18, 30), (wl - 19, 30), (30, 18), (30, hl - 19), (-1, 30), (30, 4095)]:
            q = ok.copy()
            q[3]["x"], q[3]["y"] = bad
            with pytest.raises(capi.VslamError) as e:
                ge.describe(0, l, q)
            assert e.value.status == capi.ERR_INVALID and "keypoint 3" in str(e.value), str(e.value)
        for x, y in [(19, 19), (wl - 20, hl - 20)]:      # the bounds themselves are legal
            assert len(ge.describe(0, l, ot.query(capi, [(x, y)]))[0]) == 1
    for r in (-1, 256):
        q = ok.copy()
        q[2]["response"] = r
        with pytest.raises(capi.VslamError) as e:
            ge.describe(0, 0, q)
        assert e.value.status == capi.ERR_INVALID and "keypoint 2" in str(e.value) and "response" in str(e.value)
    with pytest.raises(capi.VslamError) as e:            # more than an image can keep
        ge.describe(0, 0, ot.query(capi, [(30, 30)] * 5000))
    assert e.value.status == capi.ERR_CAPACITY
    for bad_idx, bad_level in [(1, 0), (-1, 0), (0, 8), (0, -1)]:
        with pytest.raises(capi.VslamError) as e:
            ge.describe(bad_idx, bad_level, ok)
        assert e.value.status == capi.ERR_INVALID
    k, d = ge.describe(0, 0, ok[:0])
    assert k.shape == (0,) and d.shape == (0, 32)
    with pytest.raises(capi.VslamError):                 # the tap invalidates the frame's outputs, like ssc_level
        ge.fetch(0)
    ge.close()


# ------------------------------------------------------------------------------------------------------------- tap == pipeline
@pytest.mark.gpu
def test_describe_equals_pipeline(capi):
    img = synth.random_image(401, 263, 17)
    ge = capi.Extractor(401, 263, 600)
    (gk, gd), = ge.extract([img])
    assert len(gk) > 300
    seen = 0
    for l in range(8):
        sel = np.nonzero(gk["octave"] == l)[0]
        sc = np.float64(ge.scalePyramid[l])
        pts = [(int(np.rint(gk["x"][i] / sc)), int(np.rint(gk["y"][i] / sc))) for i in sel]
        q = ot.query(capi, pts)
        q["response"] = gk["response"][sel]
        ot.assert_same(ge.describe(0, l, q), (gk[sel], gd[sel]), "level %d" % l)
        seen += len(sel)
    assert seen == len(gk)
    ge.close()
