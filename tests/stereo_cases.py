"""Crafted inputs for the stereo matcher (findStereoMatchesORB2R, src/FeatureMatcher.cpp:528-708), shared by
tests/test_oracle_stereo.py (CPU: every case proves, with the oracle alone, that it is in the regime it is named after)
and tests/test_gpu_stereo.py (GPU: bit-exact parity on the same cases).  A plain module, not a conftest.

Pyramids: a textured image and a copy shifted left by a whole number of pixels (plus a sparse +1 speckle, so that the
SAD at the true shift is small but not zero), extracted by the oracle, so that both sides hold real pyramids.  Keys and
descriptors are host-supplied.  Every case is a few isolated probes (one image row each, rows further apart than the
widest row band) plus ten ordinary filler pairs that keep the median SAD ordinary.

DEFINED DOMAIN.  The reference reads its left 11x11 window with rowRange / colRange (which throw outside the image)
and the oracle's Image::at is unchecked, so a left key closer than 5 level-pixels to a border of its level octL is
undefined behaviour there and cannot be a parity target: the kernel's clamping of an out-of-image LEFT window stays
unpinned.  Every left key built here that can reach the SAD stage keeps 5 <= round(x * scaleInv[octL]) <= w - 6 and
5 <= round(y * scaleInv[octL]) <= h - 6 (asserted in _Builder.finish).  The only exceptions are left keys marked
no_sad, which provably never reach the SAD stage: y < 0 (rejected by `maxU < 0` before anything is read), or every right
key of the case further than 75 bits from their descriptor (asserted too).  "Border" cases therefore mean the RIGHT
key's x near the left / right border (the shift-skip rule `startW < 0 || endW >= cols`, fully defined) and right keys
whose rounded row is outside the image (defined by the oracle's skip of rows outside [0, H)).

Two edges named in the matching tests cannot be reached past the other tests and are only run, not told apart:
yKey == mn of a right key's band needs uL < uR, which the window test `uR <= uL` (the y-as-disparity quirk) rejects;
a right key below the image needs a left key with yKey >= H, which the oracle skips.
"""
import numpy as np
import synth

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
INT_MAX = 2 ** 31 - 1
STEREO_MAX_L = 7680            # left keys per pair the matcher accepts (20 B of dynamic LDS each)
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# pyramids
class Ctx:
    """One image pair with the oracle extractors that hold its pyramids."""

    def __init__(self, oracle, rig_name, shift, seed=91):
        self.rig_name, self.rig, self.shift = rig_name, synth.RIGS[rig_name], shift
        w, h = self.rig["w"], self.rig["h"]
        self.L = synth.random_image(w, h, seed)
        speckle = np.random.default_rng(seed + 1).random((h, w)) < 0.25
        self.R = np.minimum(np.roll(self.L, -shift, axis=1).astype(np.int32) + speckle, 255).astype(np.uint8)
        self.exL, self.exR = oracle.Extractor(500), oracle.Extractor(500)
        self.exL.extract(self.L)
        self.exR.extract(self.R)
        self.lvL = [self.exL.level(o) for o in range(8)]
        self.lvR = [self.exR.level(o) for o in range(8)]
        self.scale, self.scaleInv = self.exL.scalePyramid, self.exL.scaleInvPyramid


_CTX = {}


def context(oracle, rig_name, shift):
    key = (rig_name, shift)
    if key not in _CTX:
        _CTX[key] = Ctx(oracle, rig_name, shift)
    return _CTX[key]


# ---------------------------------------------------------------------------------------------------------------------
# the per-left rule restated in numpy on the oracle's pyramids (float as the reference: the regime checks use it to say
# which shifts are skipped and where the SAD minimum lands, independently of the oracle's own matcher code)
def c_round(v):
    v = float(v)
    return F32(np.sign(v) * np.floor(abs(v) + 0.5))       # std::round: halves away from zero


def sad_curve(ctx, kl, kr):
    """-> dict(dists[11] float32 with 0 at skipped shifts, skipped[11], bestX, bestDistW, scuL, scvL, scuR)"""
    o = int(kl["octave"])
    sc = F32(ctx.scaleInv[o])
    scuL, scvL, scuR = c_round(F32(kl["x"]) * sc), c_round(F32(kl["y"]) * sc), c_round(F32(kr["x"]) * sc)
    imL, imR = ctx.lvL[o], ctx.lvR[o]
    cols = imR.shape[1]
    ly0, lx0 = int(scvL - F32(5)), int(scuL - F32(5))
    assert 0 <= ly0 and ly0 + 11 <= imL.shape[0] and 0 <= lx0 and lx0 + 11 <= imL.shape[1], "left window outside the defined domain"
    winL = imL[ly0:ly0 + 11, lx0:lx0 + 11].astype(np.int64)
    dists, skipped = np.zeros(11, F32), np.ones(11, bool)
    bestX, bestW = 0, INT_MAX
    for xm in range(-5, 6):
        startW, endW = scuR + F32(xm) - F32(5), scuR + F32(xm) + F32(5) + F32(1)
        if startW < 0 or endW >= cols:
            continue
        rx0 = int(startW)
        sad = int(np.abs(winL - imR[ly0:ly0 + 11, rx0:rx0 + 11].astype(np.int64)).sum())
        if float(F32(bestW)) > sad:
            bestX, bestW = xm, sad
        dists[xm + 5], skipped[xm + 5] = F32(sad), False
    return dict(dists=dists, skipped=skipped, bestX=bestX, bestDistW=bestW, scuL=scuL, scvL=scvL, scuR=scuR)


def refine(ctx, kl, kr):
    """-> (counted as a match, accepted before the cuts, curve) for left key kl refined against right key kr"""
    c = sad_curve(ctx, kl, kr)
    bx = c["bestX"]
    if bx in (-5, 5):
        return False, False, c
    d1, d2, d3 = c["dists"][4 + bx], c["dists"][5 + bx], c["dists"][6 + bx]
    with np.errstate(all="ignore"):
        delta = (d1 - d3) / (F32(2) * (d1 + d3 - F32(2) * d2))
    if delta > 1 or delta < -1:
        return False, False, c
    newuR = F32(ctx.scale[int(kl["octave"])]) * (c["scuR"] + F32(bx) + delta)
    disparity = F32(kl["x"]) - newuR
    c["delta"] = delta
    return True, bool(disparity > 0 and float(disparity) < ctx.rig["fx"]), c


# ---------------------------------------------------------------------------------------------------------------------
def flip(desc, nbits, start=0):
    """desc with bits start .. start + nbits - 1 inverted (Hamming distance nbits to the original)"""
    d = desc.copy()
    for b in range(start, start + nbits):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


class Case:
    """kL, dL, kR, dR; expect = dict(candidates, sad, matches) as the builder predicts them; pre_best[nL] = the right
    index each left key is predicted to be accepted onto before the cuts (-1: none); curves[l] = the numpy SAD curve of a
    refined left key; tags = named left-key indices for the case's own regime check."""


class _Builder:
    def __init__(self, ctx, name, seed=5):
        self.ctx, self.name = ctx, name
        self.rng = np.random.default_rng(seed)
        h = ctx.rig["h"]
        self.step = max(20, (h - 60) // 22)
        self.next_row = 30
        self.lk, self.ld, self.rk, self.rd = [], [], [], []
        self.cand, self.best, self.no_sad = [], [], []
        self.tags = {}

    def row(self):
        y = self.next_row
        self.next_row += self.step
        assert self.next_row <= self.ctx.rig["h"] - 30, "out of rows"
        return float(y)

    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def right(self, x, y, o, d):
        k = np.zeros((), KP_DTYPE)
        k["x"], k["y"], k["octave"], k["size"], k["angle"] = x, y, o, 31.0, 0.0
        self.rk.append(k); self.rd.append(d)
        return len(self.rk) - 1

    def left(self, x, y, o, d, cand, best, no_sad=False, tag=None):
        """cand: Hamming candidates this key meets by construction; best: the right index that wins with <= 75 bits or None"""
        k = np.zeros((), KP_DTYPE)
        k["x"], k["y"], k["octave"], k["size"], k["angle"] = x, y, o, 31.0, 0.0
        self.lk.append(k); self.ld.append(d)
        self.cand.append(cand); self.best.append(best); self.no_sad.append(no_sad)
        if tag:
            self.tags[tag] = len(self.lk) - 1
        return len(self.lk) - 1

    def filler(self, n=10):
        """ordinary pairs at octave 0: the right key at the true shift, so bestX = 0"""
        w, S = self.ctx.rig["w"], self.ctx.shift
        for i in range(n):
            y = self.row()
            lx = float(60 + (i * 53) % (w - 140))
            d = self.desc()
            r = self.right(lx - S, y, 0, flip(d, i % 7))
            self.left(lx, y, 0, d, 1, r)

    def finish(self):
        ctx, c = self.ctx, Case()
        c.name, c.ctx = self.name, ctx
        c.kL, c.kR = np.array(self.lk, KP_DTYPE), np.array(self.rk, KP_DTYPE)
        c.dL = np.array(self.ld, np.uint8).reshape(-1, 32)
        c.dR = np.array(self.rd, np.uint8).reshape(-1, 32)
        c.tags = self.tags
        nL = len(c.kL)
        c.pre_best = np.full(nL, -1, np.int32)
        c.curves = {}
        matches = 0
        for l in range(nL):
            kl = c.kL[l]
            if self.no_sad[l]:
                # provably never refined: y < 0, or no right key within 75 bits
                assert kl["y"] < 0 or all(hamming(c.dL[l], dr) > 75 for dr in c.dR), (self.name, l)
                assert self.best[l] is None
                continue
            o = int(kl["octave"])
            su, sv = c_round(F32(kl["x"]) * F32(ctx.scaleInv[o])), c_round(F32(kl["y"]) * F32(ctx.scaleInv[o]))
            hl, wl = ctx.lvL[o].shape
            assert 5 <= su <= wl - 6 and 5 <= sv <= hl - 6, (self.name, l, "left key outside the defined domain")
            if self.best[l] is None:
                continue
            m, acc, cur = refine(ctx, kl, c.kR[self.best[l]])
            c.curves[l] = cur
            matches += int(m)
            if acc:
                c.pre_best[l] = self.best[l]
        c.best_of = list(self.best)
        c.expect = dict(candidates=int(sum(self.cand)), sad=sum(b is not None for b in self.best), matches=matches)
        return c


# ---------------------------------------------------------------------------------------------------------------------
# matching cases.  Each returns a Case; `shift_of` names the image pair it needs.
def case_skip_left(ctx):
    """right key near the LEFT border: shifts with startW < 0 are skipped, the SAD minimum sits next to the first
    shift that is not (bestX - 1 skipped: dist1 = 0 enters the parabola)"""
    b = _Builder(ctx, "skip_left"); b.filler()
    S = ctx.shift
    for tag, rx, bx in (("p0", 8.0, -3), ("p1", 6.0, -1), ("p2", 9.0, -4)):
        y, d = b.row(), b.desc()
        r = b.right(rx, y, 0, flip(d, 3))
        b.left(rx + bx + S, y, 0, d, 1, r, tag=tag)      # true match of the left window at right x = rx + bx
    c = b.finish(); c.want_bestX = {"p0": -3, "p1": -1, "p2": -4}
    return c


def case_skip_right(ctx):
    """right key near the RIGHT border (image pair shifted by one pixel, so that the true match can sit there): shifts
    with endW >= cols are skipped, the SAD minimum sits next to the last shift that is not (dist3 = 0)"""
    assert ctx.shift == 1
    b = _Builder(ctx, "skip_right"); b.filler()
    w = ctx.rig["w"]
    for tag, rx, bx in (("p0", w - 7.0, 0), ("p1", w - 5.0, -2), ("p2", w - 3.0, -4)):
        y, d = b.row(), b.desc()
        r = b.right(rx, y, 0, flip(d, 3))
        b.left(w - 6.0, y, 0, d, 1, r, tag=tag)           # true match at right x = w - 7 = rx + bx
    c = b.finish(); c.want_bestX = {"p0": 0, "p1": -2, "p2": -4}
    return c


def case_skip_all(ctx):
    """all 11 shifts skipped: bestDistW stays INT_MAX, bestX 0, every dist 0 -> delta = 0 / 0 passes both comparisons,
    the pair counts as a match and the NaN disparity rejects it"""
    b = _Builder(ctx, "skip_all"); b.filler()
    w = ctx.rig["w"]
    for tag, rx in (("p0", -1.0), ("p1", w - 1.0), ("p2", w + 3.0), ("p3", -0.6)):
        y, d = b.row(), b.desc()
        r = b.right(rx, y, 0, flip(d, 3))
        b.left(300.0, y, 0, d, 1, r, tag=tag)
    return b.finish()


def case_octave(ctx):
    """octR == octL +- 1 is a candidate, +- 2 is not, at octL 0, 3 and 7; the excluded keys carry the better
    descriptor, so admitting one changes the winner"""
    b = _Builder(ctx, "octave"); b.filler()
    S, w, h = ctx.shift, ctx.rig["w"], ctx.rig["h"]
    for tag, oL, ins, outs in (("o0", 0, (1,), (2,)), ("o3", 3, (2, 4), (1, 5)), ("o7", 7, (6,), (5,)), ("o7s", 7, (7, 6), ())):
        y, d = b.row(), b.desc()
        lx = w * 0.5
        first = None
        for k, oR in enumerate(ins):
            r = b.right(lx - S, y, oR, flip(d, 12 - 2 * k))     # the LAST admitted key is the best one
            first = r
        for oR in outs:
            b.right(lx - S, y, oR, d.copy())
        b.left(lx, y, oL, d, len(ins), first, tag=tag)
    return b.finish()


def case_band(ctx):
    """yKey == mx of the right key's row band is inside, one row beyond is outside (octave 0: +2, octave 1: +3, octave
    7, the largest band: +8); yKey == mn and one row beyond (never candidates: uL < uR)"""
    b = _Builder(ctx, "band"); b.filler()
    S, w = ctx.shift, ctx.rig["w"]
    for tag, oL, oR, mx in (("b0", 0, 0, 2), ("b1", 0, 1, 3), ("b7", 6, 7, 8)):
        yr, d = b.row(), b.desc()
        lx = w * 0.5
        r = b.right(lx - S, yr, oR, flip(d, 4))
        b.left(lx, yr + mx, oL, d, 1, r, tag=tag + "_in")
        b.left(lx, yr + mx + 1, oL, d, 0, None, tag=tag + "_out")
    yr, d = b.row(), b.desc()
    r = b.right(w * 0.5 - S, yr, 0, flip(d, 4))
    b.left(w * 0.5, yr - 2, 0, d, 0, None, tag="mn")
    b.left(w * 0.5, yr - 3, 0, d, 0, None, tag="mn_out")
    return b.finish()


def case_uR(ctx):
    """uR == uL is inside the window (uR <= maxU), one ulp above is outside; the excluded key has the better descriptor"""
    b = _Builder(ctx, "uR"); b.filler()
    S = ctx.shift
    y, d = b.row(), b.desc()
    r = b.right(300.0 - S, y, 0, flip(d, 9))
    b.right(300.0 - S, np.nextafter(F32(y), F32(np.inf)), 0, d.copy())
    b.left(300.0, y, 0, d, 1, r, tag="eq")
    y, d = b.row(), b.desc()
    b.right(300.0 - S, np.nextafter(F32(y), F32(np.inf)), 0, d.copy())
    b.left(300.0, y, 0, d, 0, None, tag="ulp")
    return b.finish()


def case_threshold(ctx):
    """descriptor distance 75 is refined, 76 is a candidate without refinement"""
    b = _Builder(ctx, "threshold"); b.filler()
    S = ctx.shift
    y, d = b.row(), b.desc()
    r = b.right(320.0 - S, y, 0, flip(d, 75))
    b.left(320.0, y, 0, d, 1, r, tag="d75")
    y, d = b.row(), b.desc()
    b.right(320.0 - S, y, 0, flip(d, 76))
    b.left(320.0, y, 0, d, 1, None, tag="d76")
    y, d = b.row(), b.desc()
    r = b.right(320.0 - S, y, 0, flip(d, 75, start=100))      # tie at 75 bits: the smaller index wins
    b.right(320.0 - S, y, 0, flip(d, 75, start=20))
    b.left(320.0, y, 0, d, 2, r, tag="tie75")
    return b.finish()


def case_half(ctx):
    """y at an exact .5: cvRound is round-half-to-even, on the left key's yKey and on the right key's band centre"""
    b = _Builder(ctx, "half"); b.filler()
    S = ctx.shift
    # left 100.5 -> 100 (half-up would give 101): right band [96, 100] holds it
    y0, d = b.row(), b.desc()
    y0 = float(int(y0) // 2 * 2)           # even
    r = b.right(310.0 - S, y0 - 2, 0, flip(d, 4))
    b.left(310.0, y0 + 0.5, 0, d, 1, r, tag="l_even")
    # left 101.5 -> 102 (truncation would give 101): right band [97, 101] does not hold it
    y0, d = b.row(), b.desc()
    y0 = float(int(y0) // 2 * 2)
    b.right(310.0 - S, y0 - 1, 0, flip(d, 4))
    b.left(310.0, y0 + 1.5, 0, d, 0, None, tag="l_odd")
    # right 98.5 -> 98, band [96, 100]: left 100.6 -> 101 is outside (half-up 99 -> [97, 101] would hold it)
    y0, d = b.row(), b.desc()
    y0 = float(int(y0) // 2 * 2)
    b.right(310.0 - S, y0 - 1.5, 0, flip(d, 4))
    b.left(310.0, y0 + 0.6, 0, d, 0, None, tag="r_even")
    # right 99.5 -> 100, band [98, 102]: left 102.4 -> 102 is inside (truncation 99 -> [97, 101] would not)
    y0, d = b.row(), b.desc()
    y0 = float(int(y0) // 2 * 2)
    r = b.right(310.0 - S, y0 - 0.5, 0, flip(d, 4))
    b.left(310.0, y0 + 2.4, 0, d, 1, r, tag="r_odd")
    return b.finish()


def case_rows_outside(ctx):
    """right keys whose rounded row is outside the image (the kernel keeps them in its border buckets, the oracle skips
    the rows outside [0, H)), left y < 0 with yKey == 0, left y == -0.0.  The left keys sit at the border, so none may
    reach the SAD stage: every right descriptor is 80 bits from every left one."""
    b = _Builder(ctx, "rows_outside"); b.filler()
    S, H = ctx.shift, ctx.rig["h"]
    d = b.desc()
    dr = flip(d, 80)
    b.right(200.0, -1.0, 0, dr)             # band [-3, 1]: rows 0 and 1
    b.right(200.0, -3.0, 0, dr)             # band [-5, -1]: no row
    b.right(200.0, -5.0, 7, dr)             # octave 7, band [-13, 3]: rows 0 .. 3
    b.right(200.0, -0.4, 0, dr)             # rounds to row 0 from outside: band [-2, 2]
    b.right(200.0, H + 1.0, 0, dr)          # band [H - 1, H + 3]: row H - 1, but uR > uL for every left key inside
    b.right(200.0, H - 0.4, 0, dr)          # rounds to row H
    b.right(200.0, H + 300.0, 3, dr)        # far outside
    ns = dict(no_sad=True)
    b.left(210.0, 0.0, 0, d, 2, None, tag="y0", **ns)        # (-1.0 and -0.4)
    b.left(210.0, 1.0, 0, d, 2, None, tag="y1", **ns)
    b.left(210.0, 2.0, 0, d, 1, None, tag="y2", **ns)        # (-0.4 only)
    b.left(210.0, 3.0, 0, d, 0, None, tag="y3", **ns)
    b.left(210.0, 3.0, 6, d, 1, None, tag="y3o6", **ns)      # the octave-7 key
    b.left(210.0, 4.0, 6, d, 0, None, tag="y4o6", **ns)
    b.left(210.0, -0.3, 0, d, 0, None, tag="neg", **ns)      # yKey 0, maxU < 0
    b.left(210.0, -0.0, 0, d, 2, None, tag="negzero", **ns)  # maxU = -0.0 is not < 0: like y0 (-1.0 and -0.4 are <= -0.0)
    b.left(210.0, H - 1.0, 0, d, 0, None, tag="bottom", **ns)
    b.left(210.0, H - 0.6, 0, d, 0, None, tag="bottom2", **ns)
    return b.finish()


def case_many_to_one(ctx):
    """several left keys accepted onto one right key: the true one (small SAD, kept) and impostors elsewhere on the row
    (large SAD, dropped by the median cut), before and after it in index order - last-writer leftIdxs, then the kill"""
    b = _Builder(ctx, "many_to_one"); b.filler()
    S = ctx.shift
    for g, order in enumerate(("before", "after")):
        y, d = b.row(), b.desc()
        rx = 150.0
        r = b.right(rx, y, 0, flip(d, 2))
        if order == "after":
            b.left(rx + S, y, 0, d, 1, r, tag="true_%d" % g)
        # impostor positions along the row: four whose SAD curve (numpy, on the pyramids) passes the parabola and the
        # disparity test, so that they are accepted and left to the median cut, and two that are rejected before it
        probe, want, xs = np.zeros((), KP_DTYPE), [True] * 4 + [False] * 2, []
        for k in range(1, 80):
            probe["x"], probe["y"], probe["octave"] = rx + S + 7.0 * k, y, 0
            acc = refine(ctx, probe, b.rk[r])[1]
            if acc in want:
                want.remove(acc); xs.append(float(probe["x"]))
        assert not want, "no impostor positions found"
        for i, x in enumerate(sorted(xs)):
            b.left(x, y, 0, flip(d, 5, start=40), 1, r, tag="imp_%d_%d" % (g, i))
        if order == "before":
            b.left(rx + S, y, 0, d, 1, r, tag="true_%d" % g)
    return b.finish()


# name -> (builder, shift of the image pair)
MATCH_CASES = {
    "skip_left": (case_skip_left, 9), "skip_right": (case_skip_right, 1), "skip_all": (case_skip_all, 9),
    "octave": (case_octave, 9), "band": (case_band, 9), "uR": (case_uR, 9), "threshold": (case_threshold, 9),
    "half": (case_half, 9), "rows_outside": (case_rows_outside, 9), "many_to_one": (case_many_to_one, 9),
}
MATCH_RIGS = ("euroc", "synthetic")        # 752 x 480 and 1920 x 1200 (two rows per thread in the row scan)


def match_case(oracle, name, rig_name):
    fn, shift = MATCH_CASES[name]
    c = fn(context(oracle, rig_name, shift))
    return (c.ctx.L, c.ctx.R), c.kL, c.dL, c.kR, c.dR, c


def tiled_case(oracle, rig_name, n_left):
    """the many_to_one case with its left keys tiled to n_left: every pair has many bit-identical copies, so equal depths
    straddle the nearest-1 % cut and hundreds of left keys share each right key"""
    images, kL, dL, kR, dR, c = match_case(oracle, "many_to_one", rig_name)
    reps = -(-n_left // len(kL))
    return images, np.tile(kL, reps)[:n_left].copy(), np.tile(dL, (reps, 1))[:n_left].copy(), kR, dR, c


# ---------------------------------------------------------------------------------------------------------------------
# direct cases of the finalize step: name -> (best[nL], depth[nL], sad[nL], nR).  Domain: depth finite > 0 and SAD in
# [0, 121 * 255] on accepted rows; best == -1 rows carry depth -1 and SAD 0 or INT_MAX (what the match kernel writes).
SAD_MAX = 121 * 255
SAD_FACTOR = F32(1.5) * F32(1.4)


def sad_edge_medians(limit=4000):
    """medians m whose cut-off (float)m * (1.5f * 1.4f) is a whole number: a SAD can sit exactly on it"""
    out = []
    for m in range(1, limit):
        t = F32(m) * SAD_FACTOR
        if float(t) == int(t) and int(t) <= SAD_MAX:
            out.append((m, int(t)))
    return out


def depth_cut(best, depth):
    """-> (n, endDe, cut depth, less, equal, quota) of the nearest-1 % cut, in numpy"""
    d = depth[best >= 0]
    n = len(d)
    endDe = int(np.floor(n * 0.01))
    if endDe == 0:
        return n, 0, None, 0, 0, 0
    cut = np.sort(d)[endDe - 1]
    less, equal = int((d < cut).sum()), int((d.view(np.uint32) == cut.view(np.uint32)).sum())
    return n, endDe, cut, less, equal, endDe - less


def naive_finalize(best, depth, sad, nR, close_depth):
    """src/FeatureMatcher.cpp:655-705 in plain Python (sorted tuples), for the direct cases"""
    nL = len(best)
    ri, li = np.full(nL, -1, np.int32), np.full(nR, -1, np.int32)
    dp, cl = np.full(nL, -1, np.float32), np.zeros(nL, np.uint8)
    acc = [i for i in range(nL) if best[i] >= 0]
    for i in acc:
        ri[i], li[best[i]], dp[i], cl[i] = best[i], i, depth[i], depth[i] < close_depth
    if not acc:
        return dict(rightIdxs=ri, leftIdxs=li, depth=dp, close=cl)
    byD = sorted((float(depth[i]), i) for i in acc)
    byS = sorted((int(sad[i]), i) for i in acc)
    med = F32(byS[len(byS) // 2][0]) * SAD_FACTOR

    def kill(i):
        if ri[i] >= 0:
            li[ri[i]] = -1
        ri[i], dp[i], cl[i] = -1, -1, 0
    for k in range(int(np.floor(len(acc) * 0.01))):
        kill(byD[k][1])
    for s, i in reversed(byS):
        if F32(s) < med:
            break
        kill(i)
    return dict(rightIdxs=ri, leftIdxs=li, depth=dp, close=cl)


def _fin(best, depth, sad, nR):
    return np.asarray(best, np.int32), np.asarray(depth, np.float32), np.asarray(sad, np.int32), int(nR)


def finalize_cases():
    rng = np.random.default_rng(17)
    cases = {}

    def plain(n, nL=None, nR=None):
        nL = n if nL is None else nL
        nR = max(n, 1) if nR is None else nR
        best, depth, sad = np.full(nL, -1, np.int32), np.full(nL, -1, np.float32), np.zeros(nL, np.int32)
        rows = np.sort(rng.choice(nL, n, replace=False))
        best[rows] = rng.permutation(nR)[:n] if n <= nR else rng.integers(0, nR, n)
        depth[rows] = rng.uniform(0.3, 40.0, n).astype(np.float32)
        sad[rows] = rng.integers(200, 1200, n)
        hole = best < 0
        sad[hole] = np.where(rng.random(hole.sum()) < 0.5, INT_MAX, 0)
        return best, depth, sad, nR

    for n in (1, 2, 99, 100, 101, 199, 200, 201):          # endDe 0 -> 1 -> 2
        cases["n%d" % n] = _fin(*plain(n))
    cases["holes"] = _fin(*plain(230, nL=700, nR=400))
    cases["none_accepted"] = _fin(*plain(0, nL=50, nR=20))
    cases["no_right"] = _fin(np.full(40, -1), np.full(40, -1.0), np.zeros(40), 0)

    # equal depths straddling the cut: n = 300 -> endDe 3; one nearer pair, then five at the same depth at interleaved
    # indices of which the two lowest indices go
    best, depth, sad, nR = plain(300)
    depth[:] = rng.uniform(2.0, 40.0, 300)
    depth[77] = 0.5
    for i in (250, 3, 142, 9, 299):
        depth[i] = 1.0
    cases["tie_depth"] = _fin(best, depth, sad, nR)
    # the tie group lies in the middle of a run of the same value that also spans holes
    best, depth, sad, nR = plain(400, nL=900, nR=500)
    acc = np.flatnonzero(best >= 0)
    depth[acc] = rng.uniform(2.0, 40.0, 400)
    depth[acc[::7]] = 1.25                                    # 58 pairs at the cut depth, endDe = 4
    cases["tie_depth_holes"] = _fin(best, depth, sad, nR)
    # all depths equal
    best, depth, sad, nR = plain(250)
    depth[:] = 3.5
    cases["depth_all_equal"] = _fin(best, depth, sad, nR)
    # quota == equal: the whole tie group goes (the rank loop must not run astray)
    best, depth, sad, nR = plain(300)
    depth[:] = rng.uniform(2.0, 40.0, 300)
    depth[[5, 150, 290]] = 0.75
    cases["tie_depth_whole_group"] = _fin(best, depth, sad, nR)

    # SAD edges
    best, depth, sad, nR = plain(150)
    sad[:] = 500
    cases["sad_all_equal"] = _fin(best, depth, sad, nR)
    best, depth, sad, nR = plain(150)
    sad[:] = 0
    cases["sad_all_zero"] = _fin(best, depth, sad, nR)
    best, depth, sad, nR = plain(150)
    sad[:] = SAD_MAX
    cases["sad_all_max"] = _fin(best, depth, sad, nR)
    edges = sad_edge_medians()
    for tag, (m, t) in (("lo", edges[0]), ("hi", edges[-1])):
        best, depth, sad, nR = plain(90)
        sad[:] = m
        sad[:10] = t - 1
        sad[10:20] = t                                        # exactly on the cut-off: dropped (not < medDistD)
        sad[20:30] = t + 1
        p = rng.permutation(90)
        cases["sad_on_cut_%s" % tag] = _fin(best, depth, sad[p], nR)
    # ties around rank n / 2: the median is the UPPER middle of an even count
    for n in (100, 101):
        best, depth, sad, nR = plain(n)
        sad[:] = 250
        sad[:50] = 100                                        # ranks 0..49 = 100, rank 50 = 250: cut-off 525, not 210
        sad[-5:] = 600
        p = rng.permutation(n)
        cases["sad_median_tie_%d" % n] = _fin(best, depth, sad[p], nR)

    # many-to-one with mixed drops: 6 right keys, 120 left keys; groups with one key in the depth cut / every other key /
    # only the owning key / only an earlier key / every key / no key dropped
    n = 120
    best = (np.arange(n) % 6).astype(np.int32)
    depth = rng.uniform(1.0, 30.0, n).astype(np.float32)
    sad = rng.integers(300, 500, n).astype(np.int32)
    sad[best == 1] = np.where(np.arange((best == 1).sum()) % 2 == 0, 5000, 400)
    sad[np.flatnonzero(best == 2)[-1]] = 5000                 # only the last writer dropped
    sad[np.flatnonzero(best == 3)[0]] = 5000                  # only an earlier key dropped
    sad[best == 4] = 9000
    depth[np.flatnonzero(best == 0)[3]] = 0.01                # the depth cut (endDe = 1) hits the clean group
    cases["many_to_one"] = _fin(best, depth, sad, 6)

    # the LDS limit: every one of 7680 left keys accepted, few distinct depths
    n = STEREO_MAX_L
    best = rng.integers(0, 5000, n).astype(np.int32)
    depth = (1.0 + rng.integers(0, 400, n) * 0.025).astype(np.float32)      # ~19 copies of each: less > 0 at the cut
    sad = rng.integers(100, 4000, n).astype(np.int32)
    cases["max_l_ties"] = _fin(best, depth, sad, 5000)
    cases["max_l_all_equal"] = _fin(best, np.full(n, 2.0), sad, 5000)
    best, depth, sad, nR = plain(n)
    cases["max_l_distinct"] = _fin(best, depth, sad, nR)
    return cases


# cases that must show equal depths straddling the cut (0 < quota < equal)
TIE_CASES = ("tie_depth", "tie_depth_holes", "depth_all_equal", "max_l_ties", "max_l_all_equal")
