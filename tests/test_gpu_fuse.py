"""vslam_fuse_search / vslam_fuse_search_batch (csrc/fuse.hip) against the numpy restatement tests/fuse_ref.py: every output array
and every report field compared as bytes, with the wave-uniform skip of k_fuse_match_b on and off (VSLAM_FUSE_SKIP, read per call).
Crafted inputs use the identity pose and unit intrinsics, so that the chosen (u, v, z) are exact in float (tests/fuse_cases.py);
the sizes cross the workgroup (256 A points) and the LDS tile (1024 B targets)."""
import ctypes as C
import functools
import numpy as np
import pytest
import fuse_cases as fc
import fuse_ref as fr

pytestmark = pytest.mark.gpu

SKIPS = ["1", "0"]
F32 = np.float32


def device(capi, T, K, size, A, dA, B, dB, **prm):
    m, b, rep = capi.fuse_search(T, K, size, A, dA, B, dB, **prm)
    return m, b, rep


def check(capi, monkeypatch, T, K, size, A, dA, B, dB, **prm):
    """device == restatement, byte for byte, on both settings of the skip; returns the restatement's answer"""
    want = fr.search(T, K, size, A, dA, B, dB, **prm)
    for skip in SKIPS:
        monkeypatch.setenv("VSLAM_FUSE_SKIP", skip)
        m, b, rep = device(capi, T, K, size, A, dA, B, dB, **prm)
        assert m.dtype == np.int32 and b.dtype == np.int32
        assert m.tobytes() == want[0].tobytes(), (skip, np.nonzero(m != want[0])[0][:8])
        assert b.tobytes() == want[1].tobytes(), (skip, np.nonzero((b != want[1]).any(axis=1))[0][:8])
        assert rep == want[2], skip
    return want


def scene(nA, nB, plants, seed=0):
    """nA / nB filler points that gate nothing (A on an 8-pixel grid left of u = 300, B on one right of u = 320, all at z = 2, random
    descriptors), then plants (a, b, bits): B point b moves onto A point a and takes its descriptor with `bits` bits flipped"""
    rng = np.random.default_rng(1000 * nA + nB + seed)
    a = np.arange(nA); b = np.arange(nB)
    A = np.stack([(a % 37) * 8.0, (a // 37) * 8.0, np.full(nA, 2.0)], axis=1)
    B = np.stack([320 + (b % 40) * 8.0, (b // 40) * 8.0, np.full(nB, 2.0)], axis=1)
    dA = fc.random_desc(rng, nA); dB = fc.random_desc(rng, nB)
    for (pa, pb, bits) in plants:
        B[pb] = A[pa]
        dB[pb] = fc.desc_with_bits(dA[pa], bits, 7)
    return fc.points(A), dA, fc.points(B), dB


@pytest.mark.parametrize("nB", [1, 1023, 1024, 1025, 2051])
@pytest.mark.parametrize("nA", [1, 255, 256, 257])
def test_sizes_across_workgroup_and_tile(capi, monkeypatch, nA, nB):
    """the winning target is the last of a tile, the first of the next, the last of a partial tile; the proposer the first or last
    thread of a workgroup, or the only thread of the second one"""
    bs = [x for x in dict.fromkeys([nB - 1, 1023, 1024, 0, 2047, 2048]) if 0 <= x < nB]
    as_ = [x for x in dict.fromkeys([nA - 1, 0, 255, 256, 128]) if 0 <= x < nA]
    plants = [(a, b, 3 + i) for i, (a, b) in enumerate(zip(as_, bs))]
    A, dA, B, dB = scene(nA, nB, plants)
    match, best, counts = check(capi, monkeypatch, fc.EYE, fc.K_UNIT, fc.SIZE, A, dA, B, dB, radius=5.0)
    for i, (a, b, bits) in enumerate(plants):
        assert match[a] == b and best[a].tolist() == [bits, b, 257, 1]
    assert counts == dict(n_visible_a=nA, n_visible_b=nB, n_proposals=len(plants), n_pairs=len(plants))


def test_gate_edges(capi, monkeypatch):
    base = np.zeros((1, 32), np.uint8)
    run = functools.partial(check, capi, monkeypatch, fc.EYE, fc.K_UNIT, fc.SIZE)
    # du, dv = 3, 4: 9 + 16 = 25 exactly
    A = fc.points([(10, 10, 2)]); B = fc.points([(13, 14, 2)])
    assert run(A, base, B, base, radius=5.0)[0].tolist() == [0]
    assert run(A, base, B, base, radius=float(np.nextafter(F32(5), F32(0))))[0].tolist() == [-1]
    # depths 4 and 5 at ratio 1.25, both ways; one float above 5 fails both ways
    P4 = fc.points([(0, 0, 4)]); P5 = fc.points([(0, 0, 5)]); P5u = fc.points([(0, 0, float(np.nextafter(F32(5), F32(6))))])
    assert run(P4, base, P5, base, depth_ratio=1.25)[0].tolist() == [0]
    assert run(P5, base, P4, base, depth_ratio=1.25)[0].tolist() == [0]
    assert run(P4, base, P5u, base, depth_ratio=1.25)[0].tolist() == [-1]
    assert run(P5u, base, P4, base, depth_ratio=1.25)[0].tolist() == [-1]
    # the image border and the camera plane, on either side: a twin at the same place would match if both were visible
    spots = np.array([(0, 0, 1), (640, 10, 1), (10, 480, 1), (639, 479, 1), (-1, 5, 1)], np.float64)
    P = np.vstack([fc.points(spots), [[3.0, 3.0, 0.0]], [[3.0, 3.0, -2.0]]])
    d = np.zeros((len(P), 32), np.uint8)
    match, best, counts = run(P, d, P, d, radius=0.5)
    assert match.tolist() == [0, -1, -1, 3, -1, -1, -1]
    assert counts == dict(n_visible_a=2, n_visible_b=2, n_proposals=2, n_pairs=2)
    # an invisible point on one side only
    vis = fc.points([(5, 5, 1)]); inv = np.array([[5.0, 5.0, -1.0]])
    assert run(vis, base, inv, base)[2] == dict(n_visible_a=1, n_visible_b=0, n_proposals=0, n_pairs=0)
    assert run(inv, base, vis, base)[2] == dict(n_visible_a=0, n_visible_b=1, n_proposals=0, n_pairs=0)


@pytest.mark.parametrize("ratio", [1.0, 1.25])
def test_invisible_points_gate_nothing_at_any_ratio(capi, monkeypatch, ratio):
    """depth_ratio = 1 is the one ratio at which two records with z = -1 would satisfy both depth compares; the NaN pixel of an
    invisible record keeps them apart.  Invisible points with EQUAL descriptors on both sides (behind the camera, z = 0, outside
    the image), among them the last targets of a partial group of the second tile (nB = 1029: 1029 % 8 = 5, so the group is padded
    with three more invisible records) and A points in both waves that the 70 A points fill; visible twins at equal depth pair."""
    nA, nB = 70, 1029
    plants = [(5, 1024, 2), (66, 7, 3)]
    A, dA, B, dB = scene(nA, nB, plants)
    hidden = np.array([[1.0, 1.0, -2.0], [2.0, 2.0, 0.0], [1400.0, 10.0, 2.0]])       # behind, on the camera plane, outside (u = 700)
    for i, a in enumerate((3, 64, 69)):
        A[a] = hidden[i]; dA[a] = 0
    for i, b in enumerate((0, 1027, 1028)):
        B[b] = hidden[i]; dB[b] = 0
    match, best, counts = check(capi, monkeypatch, fc.EYE, fc.K_UNIT, fc.SIZE, A, dA, B, dB, radius=5.0, depth_ratio=ratio)
    for a in (3, 64, 69):
        assert match[a] == -1 and best[a].tolist() == [257, -1, 257, 0]
    assert (best[:, 1] < nB).all() and (match < nB).all()
    assert match[5] == 1024 and match[66] == 7
    assert counts == dict(n_visible_a=nA - 3, n_visible_b=nB - 3, n_proposals=2, n_pairs=2)
    # nothing but invisible points on either side
    H = np.repeat(hidden, 3, axis=0); dH = np.zeros((9, 32), np.uint8)
    match, best, counts = check(capi, monkeypatch, fc.EYE, fc.K_UNIT, fc.SIZE, H, dH, H, dH, radius=5.0, depth_ratio=ratio)
    assert (match == -1).all() and counts == dict(n_visible_a=0, n_visible_b=0, n_proposals=0, n_pairs=0)


def test_descriptor_rules(capi, monkeypatch):
    run = functools.partial(check, capi, monkeypatch, fc.EYE, fc.K_UNIT, fc.SIZE)
    base = np.zeros(32, np.uint8)
    A = fc.points([(50, 50, 2), (100, 50, 2), (150, 50, 2), (200, 50, 2)])
    dA = np.stack([base] * 4)
    # A0: exactly max_hamming; A1: one more; A2: two gated targets at the same distance; A3: one gated target
    B = fc.points([(50, 50, 2), (100, 50, 2), (150, 51, 2), (150, 49, 2), (200, 50, 2)])
    dB = np.stack([fc.desc_with_bits(base, 50), fc.desc_with_bits(base, 51), fc.desc_with_bits(base, 9, 30), fc.desc_with_bits(base, 9, 90),
                   fc.desc_with_bits(base, 1)])
    match, best, counts = run(A, dA, B, dB, max_hamming=50)
    assert match.tolist() == [0, -1, 2, 4]
    assert best.tolist() == [[50, 0, 257, 1], [51, 1, 257, 1], [9, 2, 9, 2], [1, 4, 257, 1]]
    assert counts["n_proposals"] == 3 and counts["n_pairs"] == 3


def test_resolve_rules(capi, monkeypatch):
    run = functools.partial(check, capi, monkeypatch, fc.EYE, fc.K_UNIT, fc.SIZE)
    base = np.zeros(32, np.uint8)
    # two A points, two B points, all four gates pass; first each A point has a target of its own
    A = fc.points([(50, 50, 2), (51, 50, 2)])
    dA = np.stack([fc.desc_with_bits(base, 2, 0), fc.desc_with_bits(base, 2, 10)])
    B = fc.points([(50.5, 50, 2), (51, 51, 2)])
    dB = np.stack([fc.desc_with_bits(base, 2, 20), fc.desc_with_bits(base, 4, 10)])
    match, best, counts = run(A, dA, B, dB)
    # (worked: A0 = bits 0-1, A1 = bits 10-11, B0 = bits 20-21, B1 = bits 10-13.  A0: B0 4, B1 6.  A1: B0 4, B1 2 -> A1 prefers B1.)
    assert best.tolist() == [[4, 0, 6, 2], [2, 1, 4, 2]] and match.tolist() == [0, 1]
    # now B1 is as far from A1 as from A0: both propose B0 with d1 = 4.  The lower a wins; A1 stays unmatched although B1 (distance
    # 6) was gated too
    dB2 = np.stack([fc.desc_with_bits(base, 2, 20), fc.desc_with_bits(base, 4, 30)])
    match, best, counts = run(A, dA, B, dB2)
    assert best.tolist() == [[4, 0, 6, 2], [4, 0, 6, 2]] and match.tolist() == [0, -1]
    assert counts == dict(n_visible_a=2, n_visible_b=2, n_proposals=2, n_pairs=1)
    # different d1: the smaller wins whatever the order of the proposers
    for first in (0, 1):
        dA3 = np.stack([fc.desc_with_bits(base, 3 if first == 0 else 5, 0), fc.desc_with_bits(base, 5 if first == 0 else 3, 0)])
        B3 = fc.points([(50.5, 50, 2)]); dB3 = base[None, :]
        match, best, _ = run(A, dA3, B3, dB3)
        assert match.tolist() == ([0, -1] if first == 0 else [-1, 0])


def test_skip_cases(capi, monkeypatch):
    """a wave in which exactly one lane gates a target (lane 6 of wave 1), waves that gate nothing over whole tiles (wave 0 and the
    partial wave 2), a workgroup whose last wave lies wholly past nA (nA = 130: wave 3 of workgroup 0)"""
    A, dA, B, dB = scene(130, 2100, [(70, 1500, 4)])
    match, best, counts = check(capi, monkeypatch, fc.EYE, fc.K_UNIT, fc.SIZE, A, dA, B, dB, radius=5.0)
    assert np.nonzero(match >= 0)[0].tolist() == [70] and match[70] == 1500 and counts["n_pairs"] == 1
    # and one in which the lanes of one wave gate DIFFERENT targets of one tile, some of them two
    A, dA, B, dB = scene(64, 1024, [(i, 3 * i, i % 7) for i in range(0, 64, 5)] + [(i, 3 * i + 1, 9) for i in range(0, 64, 10)])
    match, best, counts = check(capi, monkeypatch, fc.EYE, fc.K_UNIT, fc.SIZE, A, dA, B, dB, radius=5.0)
    assert counts["n_pairs"] == 13 and best[10].tolist() == [3, 30, 9, 2]


@functools.lru_cache(maxsize=None)
def known_answer():
    """600 A points and 5 000 B points with random descriptors; 200 B points lie where an A point lies and carry its descriptor under
    0 .. 20 flipped bits; all seen from a random rigid pose.  Two random descriptors lie 128 +- 8 bits apart, so a chance distance
    <= 50 is a ten-sigma event: exactly the 200 planted pairs match."""
    rng = np.random.default_rng(77)
    K = (458.654, 457.296, 367.215, 248.375); size = (752, 480)
    R = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    if np.linalg.det(R) < 0:
        R[:, 0] = -R[:, 0]
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = rng.normal(size=3)

    def cloud(n):
        u = rng.uniform(5, size[0] - 5, n); v = rng.uniform(5, size[1] - 5, n); z = rng.uniform(2, 10, n)
        Xc = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1)
        return (Xc - T[:3, 3]) @ R                      # R^T (Xc - t)
    A = cloud(600); B = cloud(5000)
    dA = fc.random_desc(rng, 600); dB = fc.random_desc(rng, 5000)
    a_idx = rng.choice(600, 200, replace=False); b_idx = rng.choice(5000, 200, replace=False)
    for k, (a, b) in enumerate(zip(a_idx, b_idx)):
        B[b] = A[a]
        flip = rng.choice(256, k % 21, replace=False)
        d = dA[a].copy()
        for bit in flip:
            d[bit >> 3] ^= np.uint8(1 << (bit & 7))
        dB[b] = d
    want = np.full(600, -1, np.int32); want[a_idx] = b_idx
    for arr in (A, B, dA, dB, want, T):
        arr.setflags(write=False)
    return T, K, size, A, dA, B, dB, want


def test_known_answer(capi, monkeypatch):
    T, K, size, A, dA, B, dB, planted = known_answer()
    match, best, counts = check(capi, monkeypatch, T, K, size, A, dA, B, dB)
    assert np.array_equal(match, planted)               # the restatement's own answer: exactly the planted pairs
    assert counts["n_pairs"] == 200 and counts["n_proposals"] == 200 and counts["n_visible_a"] == 600


def lane_inputs():
    T, K, size, A, dA, B, dB, _ = known_answer()
    s1 = scene(257, 2051, [(256, 2050, 5), (0, 1023, 6), (255, 1024, 7)])
    s2 = scene(1, 1, [(0, 0, 2)])
    s3 = scene(256, 1024, [(255, 1023, 1)])
    s4 = scene(130, 1100, [(70, 5, 4)])
    e = np.zeros((0, 3)); ed = np.zeros((0, 32), np.uint8)
    unit = (fc.EYE, fc.K_UNIT, fc.SIZE)
    return [unit + s1, (T, K, size, A, dA, B, dB), None, unit + (s4[0], s4[1], e, ed), unit + s2, unit + s3, unit + s4]


def test_lanes_equal_their_single_calls(capi, monkeypatch):
    """seven lanes in one call - one idle, one with nB = 0 - then reversed: every lane's bytes are its single call's, and two
    identical calls return identical bytes"""
    lanes = lane_inputs()
    for skip in SKIPS:
        monkeypatch.setenv("VSLAM_FUSE_SKIP", skip)
        single = [None if ln is None else capi.fuse_search(*ln, radius=5.0) for ln in lanes]
        for order in (list(range(7)), list(range(6, -1, -1))):
            got = capi.fuse_search_batch([lanes[g] for g in order], radius=5.0, fill=-77)
            again = capi.fuse_search_batch([lanes[g] for g in order], radius=5.0, fill=-77)
            for q, g in enumerate(order):
                m, b, rep = got[q]
                assert m.tobytes() == again[q][0].tobytes() and b.tobytes() == again[q][1].tobytes() and rep == again[q][2]
                if lanes[g] is None:
                    assert rep == dict(n_visible_a=-77, n_visible_b=-77, n_proposals=-77, n_pairs=-77)      # not written at all
                    continue
                assert m.tobytes() == single[g][0].tobytes(), (skip, g)
                assert b.tobytes() == single[g][1].tobytes(), (skip, g)
                assert rep == single[g][2], (skip, g)
    # the single calls against the restatement (the lanes that the other tests do not already cover)
    for g in (0, 3, 6):
        ln = lanes[g]
        want = fr.search(*ln, radius=5.0)
        assert single[g][0].tobytes() == want[0].tobytes() and single[g][1].tobytes() == want[1].tobytes() and single[g][2] == want[2]
    assert single[3][2] == dict(n_visible_a=130, n_visible_b=0, n_proposals=0, n_pairs=0) and (single[3][0] == -1).all()
    # nA = 0: nothing to match, the report counts what is visible
    s = lanes[6]
    m, b, rep = capi.fuse_search(fc.EYE, fc.K_UNIT, fc.SIZE, np.zeros((0, 3)), np.zeros((0, 32), np.uint8), s[5], s[6])
    assert len(m) == 0 and rep == dict(n_visible_a=0, n_visible_b=1100, n_proposals=0, n_pairs=0)


SENT = 0x5A


def raw_batch(capi, lanes, n_lanes=None, prm=(0.0, 0.0, 0), reports=True, table=True):
    """vslam_fuse_search_batch with sentinel-filled outputs; lanes: dicts of FuseLane fields (arrays or None).
    Returns (status, message, every output buffer still holds the sentinel)"""
    L = capi.lib()
    B = len(lanes)
    tab = (capi.FuseLane * max(B, 1))()
    keep, outs = [], []
    for g, ln in enumerate(lanes):
        nA = ln["n_a"]
        match = np.full(max(nA, 1), SENT * 0x01010101, np.int32); best = np.full((max(nA, 1), 4), SENT * 0x01010101, np.int32)
        arrs = {k: (None if ln.get(k) is None else np.ascontiguousarray(ln[k])) for k in ("T_cw", "a_xyz", "a_desc", "b_xyz", "b_desc")}
        keep.append(arrs); outs += [match, best]
        ptr = lambda a: None if a is None else a.ctypes.data
        K = ln.get("K", fc.K_UNIT); size = ln.get("size", fc.SIZE)
        tab[g] = capi.FuseLane(ptr(arrs["T_cw"]), K[0], K[1], K[2], K[3], size[0], size[1], ptr(arrs["a_xyz"]), ptr(arrs["a_desc"]), nA,
                               ptr(arrs["b_xyz"]), ptr(arrs["b_desc"]), ln["n_b"],
                               None if ln.get("no_match") else match.ctypes.data, best.ctypes.data)
    reps = np.full(4 * max(B, 1), SENT * 0x01010101, np.int32)
    p = capi.FuseParams(*prm)
    st = L.vslam_fuse_search_batch(tab if table else None, B if n_lanes is None else n_lanes, C.byref(p), 0,
                                   reps.ctypes.data_as(C.c_void_p) if reports else None)
    msg = L.vslam_last_error().decode()
    clean = all((o == SENT * 0x01010101).all() for o in outs) and (reps == SENT * 0x01010101).all()
    return st, msg, clean


def raw_single(capi, ln, prm=(0.0, 0.0, 0), null_params=False, null_report=False):
    """vslam_fuse_search with sentinel-filled outputs; ln as for raw_batch.  Returns (status, message, outputs still hold the sentinel)"""
    L = capi.lib()
    nA = ln["n_a"]
    match = np.full(max(nA, 1), SENT * 0x01010101, np.int32); best = np.full((max(nA, 1), 4), SENT * 0x01010101, np.int32)
    rep = np.full(4, SENT * 0x01010101, np.int32)
    arrs = {k: (None if ln.get(k) is None else np.ascontiguousarray(ln[k])) for k in ("T_cw", "a_xyz", "a_desc", "b_xyz", "b_desc")}
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    K = ln.get("K", fc.K_UNIT); size = ln.get("size", fc.SIZE)
    p = capi.FuseParams(*prm)
    st = L.vslam_fuse_search(ptr(arrs["T_cw"]), C.c_double(K[0]), C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3]), int(size[0]), int(size[1]),
                             ptr(arrs["a_xyz"]), ptr(arrs["a_desc"]), nA, ptr(arrs["b_xyz"]), ptr(arrs["b_desc"]), ln["n_b"],
                             None if null_params else C.byref(p), 0, None if ln.get("no_match") else ptr(match), ptr(best),
                             None if null_report else ptr(rep))
    msg = L.vslam_last_error().decode()
    clean = all((o == SENT * 0x01010101).all() for o in (match, best, rep))
    return st, msg, clean


def good_lane(nA=3, nB=4):
    A, dA, B, dB = scene(nA, nB, [(0, 0, 1)])
    return dict(T_cw=fc.EYE.copy(), a_xyz=A, a_desc=dA, n_a=nA, b_xyz=B, b_desc=dB, n_b=nB)


def test_refusals(capi):
    ok = good_lane()
    st, msg, clean = raw_batch(capi, [ok, ok])
    assert st == capi.OK and not clean                           # (the helper itself: a good call writes)

    def refused(status, lanes, needle="lane 1", **kw):
        st, msg, clean = raw_batch(capi, lanes, **kw)
        assert st == status, (st, msg)
        assert clean, msg
        if needle:
            assert needle in msg, msg

    bad = lambda **kw: dict(ok, **kw)
    nan_pose = fc.EYE.copy(); nan_pose[1, 3] = np.nan
    inf_xyz = ok["b_xyz"].copy(); inf_xyz[2, 1] = np.inf
    INV, CAP = capi.ERR_INVALID, capi.ERR_CAPACITY
    # NULL arrays, lanes < 1
    for k in ("T_cw", "a_xyz", "a_desc", "b_xyz", "b_desc"):
        refused(INV, [ok, bad(**{k: None})])
    refused(INV, [ok, bad(no_match=True)])
    refused(INV, [ok], needle=None, n_lanes=0)
    refused(INV, [ok], needle=None, table=False)
    refused(INV, [ok], needle=None, reports=False)
    refused(INV, [ok, bad(n_a=-1)])
    # non-finite pose, coordinate, intrinsic, parameter
    refused(INV, [ok, bad(T_cw=nan_pose)])
    refused(INV, [ok, bad(b_xyz=inf_xyz)])
    refused(INV, [ok, bad(a_xyz=np.where(np.arange(9).reshape(3, 3) == 4, np.nan, ok["a_xyz"]))])
    refused(INV, [ok, bad(K=(1.0, np.inf, 0.0, 0.0))])
    refused(INV, [ok, ok], needle=None, prm=(float("nan"), 0.0, 0))
    refused(INV, [ok, ok], needle=None, prm=(0.0, float("inf"), 0))
    # image size, negative parameters, depth_ratio inside (0, 1)
    refused(INV, [ok, bad(size=(0, 480))])
    refused(INV, [ok, bad(size=(640, 0))])
    refused(INV, [ok, ok], needle=None, prm=(-1.0, 0.0, 0))
    refused(INV, [ok, ok], needle=None, prm=(0.0, -1.25, 0))
    refused(INV, [ok, ok], needle=None, prm=(0.0, 0.0, -1))
    refused(INV, [ok, ok], needle=None, prm=(0.0, 0.5, 0))
    # capacity: a set above 65 536, more than 256 lanes, more than 1 048 576 points in all
    big = np.zeros((65537, 3)); big[:, 2] = 1.0
    bigd = np.zeros((65537, 32), np.uint8)
    refused(CAP, [ok, bad(b_xyz=big, b_desc=bigd, n_b=65537)])
    refused(CAP, [ok, bad(a_xyz=big, a_desc=bigd, n_a=65537)])
    refused(CAP, [ok] * 257, needle=None)
    full = bad(b_xyz=big[:65536], b_desc=bigd[:65536], n_b=65536)
    refused(CAP, [full] * 17, needle="lane 15")                  # 16 x 65 539 points pass 1 048 576 at the sixteenth lane
    # the single call has its own argument checks: the same refusals, sentinel bytes intact, no lane in the text
    def single(status, lane=ok, prm=(0.0, 0.0, 0), **kw):
        st, msg, clean = raw_single(capi, lane, prm, **kw)
        assert st == status, (st, msg)
        assert clean == (status != capi.OK), msg
        assert status == capi.OK or ("vslam_fuse_search:" in msg and "lane" not in msg), msg      # (the text of a refusal)

    single(capi.OK)
    single(capi.OK, null_params=True)                            # NULL params: all defaults
    single(INV, null_report=True)
    single(INV, lane=bad(T_cw=None))
    for k in ("a_xyz", "a_desc", "b_xyz", "b_desc"):
        single(INV, lane=bad(**{k: None}))
    single(INV, lane=bad(no_match=True))
    single(INV, lane=bad(n_b=-1))
    single(INV, lane=bad(T_cw=nan_pose))
    single(INV, lane=bad(b_xyz=inf_xyz))
    single(INV, lane=bad(K=(np.nan, 1.0, 0.0, 0.0)))
    single(INV, lane=bad(size=(0, 480)))
    for prm in ((float("nan"), 0.0, 0), (-1.0, 0.0, 0), (0.0, -1.0, 0), (0.0, 0.0, -1), (0.0, 0.5, 0)):
        single(INV, prm=prm)
    single(CAP, lane=bad(b_xyz=big, b_desc=bigd, n_b=65537))
    single(CAP, lane=bad(a_xyz=big, a_desc=bigd, n_a=65537))
    with pytest.raises(capi.VslamError) as ex:
        capi.fuse_search(nan_pose, fc.K_UNIT, fc.SIZE, ok["a_xyz"], ok["a_desc"], ok["b_xyz"], ok["b_desc"])
    assert ex.value.status == INV and "lane" not in str(ex.value)
    with pytest.raises(capi.VslamError) as ex:
        capi.fuse_search(fc.EYE, fc.K_UNIT, fc.SIZE, ok["a_xyz"], ok["a_desc"], ok["b_xyz"], ok["b_desc"], depth_ratio=0.9)
    assert ex.value.status == INV
    with pytest.raises(capi.VslamError) as ex:
        capi.fuse_search(fc.EYE, fc.K_UNIT, fc.SIZE, ok["a_xyz"], ok["a_desc"], big, bigd)
    assert ex.value.status == CAP
