"""vslam_match_by_radius_window (matchByRadius from one key set into several resident key blocks on ONE claim table, what
addMappointsMono does) against sequential CPU matchByRadius calls that share the table: match_out, n_matches and the final table
bit-exact, on crafted keys (every gate and the claim logic pinned one by one) and on real frames of the mono sequence."""
import numpy as np
import pytest
import synth

pytestmark = pytest.mark.gpu
RIG = synth.RIGS["euroc"]          # 752 x 480: 64 x 41 matching grid, cells of 11.75 x 11.7 px
RAD = 15.0                         # octave 0: a window of 15 px


@pytest.fixture(scope="module")
def ctx(oracle, capi):
    ge = capi.Extractor(RIG["w"], RIG["h"], 1500, batch=1)
    ge.extract([synth.random_image(RIG["w"], RIG["h"], 99)])      # (vslam_match_by_radius wants an extractor that has run)
    m = capi.Matcher(RIG, ge, 0, None, 0)
    return dict(oracle=oracle, capi=capi, ex=oracle.Extractor(1500), ge=ge, m=m)


def kps_of(oracle, rows):
    """rows: (x, y, octave)"""
    k = np.zeros(len(rows), oracle.KP_DTYPE)
    for i, (x, y, o) in enumerate(rows):
        k[i]["x"], k[i]["y"], k[i]["octave"] = np.float32(x), np.float32(y), o
        k[i]["size"], k[i]["angle"], k[i]["class_id"] = 31.0, 0.0, -1
    return k


def flipped(base, dist):
    """the descriptor at Hamming distance `dist` from base (its first `dist` bits flipped)"""
    d = base.copy()
    for b in range(dist):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def reference(c, qk, qd, targets, tab0, rad, fresh=False):
    """sequential matchByRadius calls, the table carried from target to target (or a fresh copy of tab0 for each)"""
    o = c["oracle"]
    tab = np.array(tab0, np.int32, copy=True)
    outs, ns = [], []
    for tk, td in targets:
        t = np.array(tab0, np.int32, copy=True) if fresh else tab
        n, sub, out = o.match_by_radius(c["ex"], RIG, qk, qd, tk, td, t[:len(tk)], rad)
        if not fresh:
            tab[:len(tk)] = sub
        outs.append(out); ns.append(n)
    return np.array(ns, np.int32), tab, (np.stack(outs) if outs else np.zeros((0, len(qk)), np.int32))


def run(c, qk, qd, targets, tab0, rad=RAD):
    """the window call, checked against the sequential reference; returns (n_matches, table, match_out)"""
    capi = c["capi"]
    last = capi.KeyBlock(qk, qd)
    blocks = [capi.KeyBlock(tk, td) for tk, td in targets]
    n, tab, out = capi.match_by_radius_window(c["m"], last, blocks, rad, tab0)
    rn, rtab, rout = reference(c, qk, qd, targets, tab0, rad)
    assert np.array_equal(out, rout), (out, rout)
    assert np.array_equal(n, rn) and np.array_equal(tab, rtab)
    for b in blocks + [last]:
        b.free()
    return n, tab, out


class Scene:
    """queries far apart (120 px), each with its own candidates placed relative to it; one target"""

    def __init__(self, oracle, seed=1):
        self.o, self.rng = oracle, np.random.default_rng(seed)
        self.q, self.qd, self.t, self.td, self.want = [], [], [], [], []

    def add(self, octave, cands, want):
        """cands: (dx, dy, octave, hamming distance); want: index into cands of the expected match, or None"""
        i = len(self.q)
        x, y = 60.0 + 120.0 * (i % 5), 50.0 + 110.0 * (i // 5)
        base = self.rng.integers(0, 256, 32, dtype=np.uint8)
        self.q.append((x, y, octave)); self.qd.append(base)
        self.want.append(None if want is None else len(self.t) + want)
        for dx, dy, o, dist in cands:
            self.t.append((np.float32(x) + np.float32(dx), np.float32(y) + np.float32(dy), o)); self.td.append(flipped(base, dist))
        return i

    def arrays(self):
        return kps_of(self.o, self.q), np.stack(self.qd), kps_of(self.o, self.t), np.stack(self.td)


def test_gates_one_by_one(ctx):
    o = ctx["oracle"]
    s = Scene(o)
    s.add(0, [(10.0, 0.0, 0, 20)], None)                       # parallax of exactly 10 px: rejected (> 10 is required)
    s.add(0, [(10.0 + 2.0 ** -10, 0.0, 0, 20)], 0)             # just above
    s.add(0, [(0.0, 10.0, 0, 20)], None)
    s.add(0, [(8.0, 6.0 + 2.0 ** -10, 0, 20)], 0)              # hypot(8, 6 + eps) > 10
    s.add(2, [(12.0, 0.0, 1, 20)], 0)                          # octave -1
    s.add(2, [(12.0, 0.0, 3, 20)], 0)                          # octave +1
    s.add(2, [(12.0, 0.0, 0, 20)], None)                       # octave -2
    s.add(2, [(12.0, 0.0, 4, 20)], None)                       # octave +2
    s.add(0, [(15.0, 0.0, 0, 20)], None)                       # |dx| == radius: outside (strict <)
    s.add(0, [(15.0 - 2.0 ** -10, 0.0, 0, 20)], 0)
    s.add(0, [(0.0, -15.0, 0, 20)], None)                      # |dy| == radius
    s.add(0, [(0.0, -15.0 + 2.0 ** -10, 0, 20)], 0)
    s.add(0, [(12.0, 0.0, 0, 40), (0.0, 12.0, 0, 50)], None)   # same level, 40 >= 0.8 * 50: rejected
    s.add(0, [(12.0, 0.0, 0, 39), (0.0, 12.0, 0, 50)], 0)      # 39 < 40
    s.add(0, [(12.0, 0.0, 0, 40), (0.0, 12.0, 1, 50)], 0)      # different levels: no ratio test
    s.add(0, [(0.0, 12.0, 0, 50), (12.0, 0.0, 0, 39)], 1)      # (the better one second in index order)
    s.add(0, [(12.0, 0.0, 0, 100)], 0)                         # matchDistProj: 100 accepted
    s.add(0, [(12.0, 0.0, 0, 101)], None)                      # 101 rejected
    s.add(0, [], None)                                         # no candidate at all
    qk, qd, tk, td = s.arrays()
    assert len(qk) <= 64 and len(tk) <= 64
    n, tab, out = run(ctx, qk, qd, [(tk, td)], np.full(len(tk), -1, np.int32))
    want = np.array([-1 if w is None else w for w in s.want], np.int32)
    assert np.array_equal(out[0], want), (out[0], want)
    assert n[0] == (want >= 0).sum()
    for i, w in enumerate(want):
        if w >= 0:
            assert tab[w] == i


def test_one_target_equals_match_by_radius_on_the_current_frame(ctx):
    o, capi = ctx["oracle"], ctx["capi"]
    rng = np.random.default_rng(5)
    s = Scene(o, seed=5)
    for i in range(20):
        cands = [(float(rng.uniform(-14, 14)), float(rng.uniform(-14, 14)), int(rng.integers(0, 2)), int(rng.integers(5, 110))) for _ in range(3)]
        s.add(int(rng.integers(0, 2)), cands, None)
    qk, qd, tk, td = s.arrays()
    tab0 = np.full(len(tk), -1, np.int32)
    n, tab, out = run(ctx, qk, qd, [(tk, td)], tab0)
    ctx["m"].set_keys(0, tk, td)
    n1, tab1, out1 = capi.match_by_radius(ctx["m"], qk, qd, RAD, tab0)
    ctx["m"].use_extractor_keys()
    assert n[0] == n1 and n1 >= 3 and np.array_equal(out[0], out1) and np.array_equal(tab, tab1)


def _shared_claim_case(o):
    """query 0 claims index 0 in target 0; index 0 is query 1's best candidate in targets 1 and 2"""
    rng = np.random.default_rng(11)
    b0, b1 = rng.integers(0, 256, 32, dtype=np.uint8), rng.integers(0, 256, 32, dtype=np.uint8)
    qk = kps_of(o, [(100.0, 100.0, 0), (400.0, 300.0, 0)]); qd = np.stack([b0, b1])
    far = rng.integers(0, 256, 32, dtype=np.uint8)
    t0 = (kps_of(o, [(112.0, 100.0, 0)]), np.stack([flipped(b0, 5)]))
    t1 = (kps_of(o, [(412.0, 300.0, 0), (400.0, 312.0, 1)]), np.stack([flipped(b1, 10), flipped(b1, 30)]))
    t2 = (kps_of(o, [(388.0, 300.0, 0), (700.0, 20.0, 0), (400.0, 288.0, 1)]), np.stack([flipped(b1, 8), far, flipped(b1, 25)]))
    return qk, qd, [t0, t1, t2]


def test_claims_carry_from_target_to_target(ctx):
    o = ctx["oracle"]
    qk, qd, targets = _shared_claim_case(o)
    tab0 = np.full(3, -1, np.int32)
    n, tab, out = run(ctx, qk, qd, targets, tab0)
    assert out.tolist() == [[0, -1], [-1, 1], [-1, 2]] and n.tolist() == [1, 1, 1]
    assert tab.tolist() == [0, 1, 1]
    # three calls with fresh tables give something else: the case cannot pass without the shared table
    fn, _, fout = reference(ctx, qk, qd, targets, tab0, RAD, fresh=True)
    assert fout.tolist() == [[0, -1], [-1, 0], [-1, 0]] and not np.array_equal(fout, out)


def test_entries_claimed_on_entry_are_respected(ctx):
    o = ctx["oracle"]
    qk, qd, targets = _shared_claim_case(o)
    tab0 = np.array([-1, 7, -1, 3], np.int32)        # index 1 taken before the call (and a 4th entry no target reaches)
    n, tab, out = run(ctx, qk, qd, targets, tab0)
    assert out.tolist() == [[0, -1], [-1, -1], [-1, 2]]
    assert tab.tolist() == [0, 7, 1, 3]


def test_exact_rescan_when_the_top_list_is_claimed_away(ctx):
    """10 candidates, the 8 best claimed on entry: the match is the 9th, found by the rescan with the claims applied"""
    o = ctx["oracle"]
    rng = np.random.default_rng(3)
    b = rng.integers(0, 256, 32, dtype=np.uint8)
    qk = kps_of(o, [(300.0, 200.0, 0)]); qd = b[None]
    ang = np.linspace(0, 2 * np.pi, 10, endpoint=False)
    dist = [10, 12, 14, 16, 18, 20, 22, 24, 40, 90]
    order = rng.permutation(10)
    rows, descs = [None] * 10, [None] * 10
    for r, k in enumerate(order):                    # index order unrelated to the distance order
        rows[k] = (300.0 + 12.0 * np.cos(ang[r]), 200.0 + 12.0 * np.sin(ang[r]), 0); descs[k] = flipped(b, dist[r])
    tk, td = kps_of(o, rows), np.stack(descs)
    tab0 = np.full(10, -1, np.int32)
    tab0[order[:8]] = 50
    n, tab, out = run(ctx, qk, qd, [(tk, td)], tab0)
    assert out[0, 0] == order[8] and n[0] == 1 and tab[order[8]] == 0
    # and with 9 claimed only the 90 is left: above nothing to compare with, 90 <= 100: accepted
    tab0[order[8]] = 50
    n, tab, out = run(ctx, qk, qd, [(tk, td)], tab0)
    assert out[0, 0] == order[9]


def test_target_sizes_0_1_64_and_table_length(ctx):
    o, capi = ctx["oracle"], ctx["capi"]
    rng = np.random.default_rng(8)
    bases = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    qrows = [(80.0 + 130.0 * i, 240.0, 0) for i in range(5)]
    qk, qd = kps_of(o, qrows), bases
    e = (kps_of(o, []), np.zeros((0, 32), np.uint8))
    one = (kps_of(o, [(92.0, 240.0, 0)]), flipped(bases[0], 9)[None])
    rows, descs = [], []
    for j in range(64):                              # 64 keys: each query has candidates among them
        i = j % 5
        rows.append((qrows[i][0] + float(rng.uniform(-14, 14)), 240.0 + float(rng.uniform(-14, 14)), int(rng.integers(0, 2))))
        descs.append(flipped(bases[i], int(rng.integers(5, 100))))
    big = (kps_of(o, rows), np.stack(descs))
    tab0 = np.full(100, -1, np.int32)
    tab0[[3, 70, 99]] = (4, 1, 2)
    n, tab, out = run(ctx, qk, qd, [e, one, big], tab0)
    assert out.shape == (3, 5) and (out[0] == -1).all() and n[0] == 0 and out[1, 0] == 0 and n[2] >= 3
    assert tab[70] == 1 and tab[99] == 2 and (tab[64:70] == -1).all()
    # a table shorter than a target is an error, nothing is written
    last = capi.KeyBlock(qk, qd); blocks = [capi.KeyBlock(*t) for t in (e, one, big)]
    with pytest.raises(capi.VslamError) as ei:
        capi.match_by_radius_window(ctx["m"], last, blocks, RAD, np.full(63, -1, np.int32))
    assert ei.value.status == capi.ERR_INVALID
    for b in blocks + [last]:
        b.free()


def test_no_queries_and_no_targets(ctx):
    o = ctx["oracle"]
    qk, qd, targets = _shared_claim_case(o)
    tab0 = np.array([-1, 5, -1], np.int32)
    n, tab, out = run(ctx, kps_of(o, []), np.zeros((0, 32), np.uint8), targets, tab0)
    assert out.shape == (3, 0) and n.tolist() == [0, 0, 0] and np.array_equal(tab, tab0)
    n, tab, out = run(ctx, qk, qd, [], tab0)
    assert out.shape == (0, 2) and len(n) == 0 and np.array_equal(tab, tab0)


def test_real_keys_first_frame_into_three_others(ctx):
    """four rendered frames of the mono sequence, 1500 features: the first keyframe's view into two wide views and the
    initialising keyframe's, rad 120 and rad 15"""
    o = ctx["oracle"]
    K = [ctx["ex"].extract(synth.mono_frame(f)[0]) for f in (22, 160, 178, 54)]
    tab0 = np.full(max(len(k[0]) for k in K), -1, np.int32)
    for rad in (120.0, 15.0):
        n, tab, out = run(ctx, K[0][0], K[0][1], K[1:], tab0, rad)
        assert (n > 20).all()
        if rad == 120.0:
            fn, _, fout = reference(ctx, K[0][0], K[0][1], K[1:], tab0, rad, fresh=True)
            assert fn[2] > 2 * n[2]                   # the shared table decides most of the last target
