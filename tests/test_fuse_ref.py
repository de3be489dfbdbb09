"""The numpy restatement of the duplicate search and of the fuse commit (tests/fuse_ref.py) against answers worked by hand."""
import numpy as np
import fuse_cases as fc
import fuse_ref as fr


def test_search_by_hand():
    """Four A points, five B points, every step written out.
    records (u, v, z):   A0 (10, 10, 2)   A1 (10.5, 10, 2)   A2 (100, 100, 4)   A3 behind the camera
                         B0 (13, 14, 2)   B1 (10, 10, 2)     B2 (10, 11, 2)     B3 (100, 100, 8)   B4 (700, 10, 2): outside
    radius 5, depth_ratio 1.25, max_hamming 50.
    gates   A0: B0 (9 + 16 = 25 <= 25), B1 (0), B2 (1)            A1: B0 (6.25 + 16 = 22.25), B1 (0.25), B2 (1.25)
            A2: B3 is at the same pixel, but 8 > 1.25 * 4: nothing      A3: invisible, nothing
    descriptors   base = 32 zero bytes; A0 = base, A1 = base with bits 0..2 set, A2 = base
                  B0 = 60 bits set (from bit 100), B1 = 10 bits set (from bit 0), B2 = 10 bits set (from bit 20), B3 = base
    distances     A0: B0 60, B1 10, B2 10 -> d1 = 10 at B1 (the lower index), d2 = 10, 3 gated
                  A1: B0 63 (bits 0..2 and 100..159 differ), B1 7 (bits 3..9), B2 13 -> d1 = 7 at B1, d2 = 13, 3 gated
    one to one    B1: keys (10 << 32 | 0) and (7 << 32 | 1): A1 wins; A0 loses and stays unmatched although B2 was gated too."""
    A = fc.points([(10, 10, 2), (10.5, 10, 2), (100, 100, 4), (1, 1, -3)])
    B = fc.points([(13, 14, 2), (10, 10, 2), (10, 11, 2), (100, 100, 8), (700, 10, 2)])
    base = np.zeros(32, np.uint8)
    dA = np.stack([base, fc.desc_with_bits(base, 3), base, base])
    dB = np.stack([fc.desc_with_bits(base, 60, 100), fc.desc_with_bits(base, 10), fc.desc_with_bits(base, 10, 20), base, base])
    RA = fr.project(fc.EYE, fc.K_UNIT, fc.SIZE, A)
    RB = fr.project(fc.EYE, fc.K_UNIT, fc.SIZE, B)
    assert RA.dtype == np.float32
    assert RA[:3].tolist() == [[10, 10, 2, 0], [10.5, 10, 2, 0], [100, 100, 4, 0]]
    assert RB[:4].tolist() == [[13, 14, 2, 0], [10, 10, 2, 0], [10, 11, 2, 0], [100, 100, 8, 0]]
    for r in (RA[3], RB[4]):                            # invisible: (NaN, NaN, -1, 0)
        assert np.isnan(r[0]) and np.isnan(r[1]) and r[2:].tolist() == [-1, 0]
    match, best, counts = fr.search(fc.EYE, fc.K_UNIT, fc.SIZE, A, dA, B, dB, radius=5.0, depth_ratio=1.25, max_hamming=50)
    assert best.tolist() == [[10, 1, 10, 3], [7, 1, 13, 3], [257, -1, 257, 0], [257, -1, 257, 0]]
    assert match.tolist() == [-1, 1, -1, -1]
    assert counts == dict(n_visible_a=3, n_visible_b=4, n_proposals=2, n_pairs=1)
    # a smaller radius: B0 leaves both gates (25 and 22.25 > 16), the rest stands
    _, best, _ = fr.search(fc.EYE, fc.K_UNIT, fc.SIZE, A, dA, B, dB, radius=4.0, depth_ratio=1.25, max_hamming=50)
    assert best.tolist()[:2] == [[10, 1, 10, 2], [7, 1, 13, 2]]
    # max_hamming 9: A0 (10) no longer proposes, A1 (7) does
    match, _, counts = fr.search(fc.EYE, fc.K_UNIT, fc.SIZE, A, dA, B, dB, radius=5.0, depth_ratio=1.25, max_hamming=9)
    assert match.tolist() == [-1, 1, -1, -1] and counts["n_proposals"] == 1
    # depth_ratio 2: A2 and B3 (4 and 8: 8 <= 2 * 4) now pair at distance 0
    match, best, counts = fr.search(fc.EYE, fc.K_UNIT, fc.SIZE, A, dA, B, dB, radius=5.0, depth_ratio=2.0, max_hamming=50)
    assert best[2].tolist() == [0, 3, 257, 1] and match.tolist() == [-1, 1, 3, -1] and counts["n_pairs"] == 2
    # empty sets
    m, b, c = fr.search(fc.EYE, fc.K_UNIT, fc.SIZE, A, dA, B[:0], dB[:0])
    assert m.tolist() == [-1] * 4 and b.tolist() == [[257, -1, 257, 0]] * 4 and c == dict(n_visible_a=3, n_visible_b=0, n_proposals=0, n_pairs=0)


def test_projection_order_and_borders():
    """u = 0 is inside, u = w is not; z = 0 and z < 0 are outside; a general pose follows the written summation order"""
    P = fc.points([(0, 0, 1), (640, 0, 1), (639.5, 479.5, 1), (0, 480, 1)])
    P = np.vstack([P, [[1.0, 1.0, 0.0]], [[1.0, 1.0, -2.0]]])
    R = fr.project(fc.EYE, fc.K_UNIT, fc.SIZE, P)
    assert (R[:, 2] > 0).tolist() == [True, False, True, False, False, False]
    rng = np.random.default_rng(5)
    T = np.eye(4); T[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]; T[:3, 3] = rng.normal(size=3)
    X = rng.normal(size=(50, 3)) * 3 + [0, 0, 8]
    K = (458.654, 457.296, 367.215, 248.375)
    R = fr.project(T, K, (752, 480), X)
    for i in range(50):
        x, y, z = [(T[r, 0] * X[i, 0] + T[r, 1] * X[i, 1]) + T[r, 2] * X[i, 2] + T[r, 3] for r in range(3)]
        ok = z > 0
        if ok:
            iz = 1.0 / z
            u, v = K[0] * x * iz + K[2], K[1] * y * iz + K[3]
            ok = not (u < 0 or v < 0 or u >= 752 or v >= 480)
        if ok:
            assert R[i].tolist() == [float(np.float32(u)), float(np.float32(v)), float(np.float32(z)), 0.0]
        else:
            assert np.isnan(R[i, 0]) and np.isnan(R[i, 1]) and R[i, 2:].tolist() == [-1, 0]


def test_invisible_points_gate_nothing_at_any_ratio():
    """depth_ratio = 1 is the one ratio at which two records with z = -1 would satisfy both depth compares (-1 <= 1 * -1): the NaN
    pixel of an invisible record keeps them apart.  Points behind the camera, at z = 0 and outside the image on both sides, with
    equal descriptors, beside one visible twin pair at equal depth (2 <= 1 * 2 both ways)"""
    P = np.vstack([[[1.0, 1.0, -2.0]], [[1.0, 1.0, -2.0]], [[3.0, 3.0, 0.0]], fc.points([(700, 10, 2), (20, 30, 2)])])
    d = np.zeros((len(P), 32), np.uint8)
    for ratio in (1.0, 1.25, 4.0):
        match, best, counts = fr.search(fc.EYE, fc.K_UNIT, fc.SIZE, P, d, P, d, radius=5.0, depth_ratio=ratio, max_hamming=50)
        assert match.tolist() == [-1, -1, -1, -1, 4]
        assert best.tolist() == [[257, -1, 257, 0]] * 4 + [[0, 4, 257, 1]]
        assert counts == dict(n_visible_a=1, n_visible_b=1, n_proposals=1, n_pairs=1)


def test_commit_by_hand():
    """the six-point, three-keyframe map of tests/fuse_cases.py: an observation moved, one dropped because the kept point already
    sits in that keyframe, a right-only observation, an absorbed point that was active and one that was not, a kept point that
    was not active"""
    tables = fc.commit_tables()
    before = (repr(fc.COMMIT_OBS), repr(tables), list(fc.COMMIT_ACTIVE))
    obs, t, outl, inf, act, last, counts = fr.commit(fc.COMMIT_PAIRS, fc.COMMIT_OBS, tables, fc.COMMIT_KDX, fc.COMMIT_OUTLIER,
                                                     fc.COMMIT_IN_FRAME, fc.COMMIT_ACTIVE, fc.COMMIT_LAST_OBS)
    assert (repr(fc.COMMIT_OBS), repr(tables), list(fc.COMMIT_ACTIVE)) == before        # the inputs are left alone
    assert obs == [[(0, 0, 0), (1, 0, -1), (2, 0, 0)], [(0, 1, -1), (2, 3, -1), (1, -1, 2)], [(1, 2, 1)], [], [], [(2, 2, -1)]]
    assert t[0] == fc.commit_tables()[0]                                                # keyframe 0 saw neither absorbed point
    assert t[1] == dict(lmpL=[0, -1, 2, -1, -1, -1], lmpR=[-1, 2, 1, -1], unF=[0, -1, 1, -1, -1, -1], unFR=[-1, 1, 0, -1])
    assert t[2] == dict(lmpL=[0, -1, 5, 1, -1, -1], lmpR=[0, -1, -1, -1], unF=[0, -1, 2, 0, -1, -1], unFR=[0, -1, -1, -1])
    assert outl == [0, 0, 0, 1, 1, 0] and inf == [1, 1, 1, 0, 0, 1]
    assert act == [1, 2, 5, 0]
    assert last == [2, 2, 1, 2, 2, 2]
    # keyframe 0 observes both kept points and neither absorbed one: its tables stand, its covisibility weights do not
    assert counts == dict(n_fused=2, n_obs_moved=2, n_obs_dropped=2, touched=[1, 2], refresh=[0, 1, 2], n_active_after=4)
    # the tables after the merge are exactly those that belong to the merged observations
    assert t == fc.commit_tables(obs)
    # no pairs: nothing changes
    obs0, t0, outl0, inf0, act0, last0, c0 = fr.commit([], fc.COMMIT_OBS, tables, fc.COMMIT_KDX, fc.COMMIT_OUTLIER, fc.COMMIT_IN_FRAME,
                                                       fc.COMMIT_ACTIVE, fc.COMMIT_LAST_OBS)
    assert obs0 == [list(o) for o in fc.COMMIT_OBS] and t0 == tables and act0 == fc.COMMIT_ACTIVE and inf0 == fc.COMMIT_IN_FRAME
    assert c0["n_fused"] == 0 and c0["touched"] == []


def test_connections_rule():
    """weights over the observations; the right table counts right-only observations; the threshold is 15"""
    n = 20
    obs = [[(0, i, -1), (1, i, -1)] for i in range(n)] + [[(0, -1, 0), (2, -1, 0)]]
    t = [dict(lmpL=list(range(n)), lmpR=[n]), dict(lmpL=list(range(n)), lmpR=[-1]), dict(lmpL=[-1] * n, lmpR=[n])]
    assert fr.connections(0, t, obs, 3) == [(21, 0), (20, 1)]
    assert fr.connections(1, t, obs, 3) == [(20, 1), (20, 0)]
    assert fr.connections(2, t, obs, 3) == []
