"""The CPU restatement of the relocalisation stage (tests/reloc_ref.py) checked on its own: the stage has no reference
counterpart, so the restatement is what the kernels are pinned to (tests/test_gpu_reloc.py) and has to stand by itself."""
import numpy as np
import reloc_cases as rc
import reloc_ref as rr


def test_mix_known_values():
    # computed with a separate C program (uint32_t arithmetic) from the rule in DESIGN.md section 6
    known = {(0x00000000, 0, 0): 0x00000000, (0x52454C4F, 0, 0): 0x620C5C52, (0x52454C4F, 1, 0): 0xDB503E30,
             (0x52454C4F, 0, 1): 0xE3957C82, (0x52454C4F, 255, 15): 0x6F2CAD06, (0x00000001, 1023, 7): 0xDA3906DA,
             (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF): 0x533C4B30}
    for (s, h, j), v in known.items():
        assert rr.mix(s, h, j) == v, (s, h, j)


def test_sample_rule():
    for C in (3, 4, 64, 200):
        for h in range(64):
            idx = rr.sample(rr.DEFAULTS["seed"], h, C)
            if idx is None:
                continue
            assert len(set(idx)) == 3 and all(0 <= v < C for v in idx)
            draws = [(rr.mix(rr.DEFAULTS["seed"], h, j) * C) >> 32 for j in range(16)]
            first = []
            for v in draws:
                if v not in first:
                    first.append(v)
            assert idx == first[:3]
    assert rr.sample(1, 0, 2) is None


def test_triad_recovers_known_pose():
    T = rc.true_pose(11)
    R, t = T[:3, :3], T[:3, 3]
    rng = np.random.Generator(np.random.PCG64(5))
    for _ in range(20):
        A = rng.uniform(-4, 4, (3, 3))
        B = A @ R.T + t
        Rh, th = rr.triad(A, B)
        assert np.abs(Rh - R).max() < 1e-12 and np.abs(th - t).max() < 1e-12
    # degenerate triples are void: coincident points, collinear points
    A = np.array([[0.0, 0, 0], [0, 0, 0], [1, 2, 3]])
    assert rr.triad(A, A @ R.T + t) is None
    A = np.array([[0.0, 0, 0], [1, 1, 1], [2, 2, 2]])
    assert rr.triad(A, A @ R.T + t) is None


def test_match_rules_small():
    rng = np.random.Generator(np.random.PCG64(1))
    keys = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    keys[4] = keys[1]                                   # a tie for the best key
    p0, b0 = rc.flip_bits(keys[0], 50, rng)             # accepted at the bound
    p1, _ = rc.flip_bits(keys[0], 51, rng)              # refused
    p2, _ = rc.flip_bits(keys[1], 3, rng)               # d1 == d2: refused, lowest index reported
    p3, _ = rc.flip_bits(keys[2], 7, rng)
    p4, _ = rc.flip_bits(keys[2], 5, rng)               # wins key 2 against p3
    p5, _ = rc.flip_bits(keys[3], 9, rng)
    p6, _ = rc.flip_bits(keys[3], 9, rng)               # equal distance: the lower point index keeps key 3
    d, kw = rr.match(np.stack([p0, p1, p2, p3, p4, p5, p6]), keys, 50, 80)
    assert list(d[0][:2]) == [50, 0] and list(d[1][:2]) == [51, 0]
    assert list(d[2]) == [3, 1, 3]
    assert list(kw) == [0, -1, 4, 5, -1, -1]
    # a single key: d2 = 257
    d, kw = rr.match(np.stack([p0]), keys[:1], 50, 80)
    assert list(d[0]) == [50, 0, 257] and list(kw) == [0]
    # the ratio test at equality: 100 * 40 == 80 * 50 is refused, d2 = 51 accepted
    ka = keys[5]
    pt, bits = rc.flip_bits(ka, 40, rng)
    kb50, _ = rc.flip_bits(ka, 10, rng, avoid=bits)
    kb51, _ = rc.flip_bits(ka, 11, rng, avoid=bits)
    d, kw = rr.match(np.stack([pt]), np.stack([ka, kb50]), 50, 80)
    assert list(d[0]) == [40, 0, 50] and list(kw) == [-1, -1]
    d, kw = rr.match(np.stack([pt]), np.stack([ka, kb51]), 50, 80)
    assert list(d[0]) == [40, 0, 51] and list(kw) == [0, -1]


def test_winner_with_forty_percent_outliers():
    rec, T, good = rc.records(200, 0.4, seed=21)
    inv_sigma = np.float32(1.0) / (np.float32(1.2) ** (2 * np.arange(8, dtype=np.float32)))
    hyp = rr.hypotheses(rec, rc.RIG, inv_sigma, 256, rr.DEFAULTS["seed"])
    assert hyp["best_count"] >= int(good.sum())
    assert np.array_equal(hyp["flags"].astype(bool) & good, good)          # every noise-free inlier is kept
    assert np.abs(hyp["T_cw"] - T).max() < 1e-9
    # the winner is the lowest h among the largest counts
    assert hyp["best"] == int(np.nonzero(hyp["counts"] == hyp["counts"].max())[0][0])


def test_points_behind_the_camera_do_not_count():
    """records whose camera-frame points all lie behind the camera: every hypothesis reproduces them there, count 0"""
    rec, T, _ = rc.records(64, 0.0, seed=4)
    R, t = T[:3, :3], T[:3, 3]
    rec["Xc"] = -rec["Xc"]
    rec["Xw"] = (rec["Xc"] - t) @ R
    inv_sigma = np.ones(8, np.float32)
    hyp = rr.hypotheses(rec, rc.RIG, inv_sigma, 32, 7)
    assert hyp["counts"].max() == 0 and hyp["best"] == 0 and hyp["best_count"] == 0 and not hyp["flags"].any()


def test_fewer_than_three_records_is_a_failure(oracle):
    g = rc.frame_for_records(2, 0.0, seed=8)
    st = oracle.stereo_finalize(g["best"], g["depth"], g["sad"], len(g["kR"]), rc.RIG)
    ex = oracle.Extractor(1500)
    r = rr.relocalize(oracle, rc.RIG, ex.InvSigmaFactor, g["points"], g["desc"], g["kL"], g["dL"], g["kR"], st)
    assert r["n_pairs"] == 2 and r["success"] == 0 and r["T_cw"] is None and r["best_count"] == 0
