"""Time of one vslam_relocalize call on a resident frame: 1 500 left keys against 20 000 map points, 256 hypotheses.

The frame is crafted (keys at random pixels with stereo depth, through set_keys + vslam_stereo_finalize_arrays) and stays in
HBM; the map is 20 000 points of which 1 200 carry a key's descriptor with 0 .. 30 bits flipped - 60 % of those consistent
with one camera pose, the rest gross outliers - and 18 800 random descriptors.  Every call uploads the map (20 000 x 56 B),
runs the four kernels and the refinement, and downloads the result, as a caller's call does.
Reported: the wall-clock time of a call (host clock around the call, which ends in a device synchronise) and the device time
per kernel group from the matcher's HIP events (summed over a repetition's calls, divided by their number).  Five warm-up
calls, then `reps` repetitions of `calls` calls each; median and range over the repetitions.  Beside it, as context only, the
time of the numpy restatement (tests/reloc_ref.py, steps A - C and the CPU pose solve) on one core for the same input.
usage: python tools/reloc_rate.py [out.json] [calls] [reps]

--lanes: the batched call.  For L = 1, 4 and 16 lanes (L matchers on images 2b / 2b + 1 of one extractor, each with a frame and a
map of the shape above from its own seed) the wall-clock time of ONE vslam_relocalize_batch call against L sequential
vslam_relocalize calls on the same matchers, same build, same process.  Five warm-up calls of each form, then `reps` repetitions
that alternate the two forms (`calls` calls each); host clock around calls that end in a device synchronise.
usage: python tools/reloc_rate.py --lanes [out.json] [calls] [reps]

--mode 0 | 1 (with either form above): vslam_reloc_params::mode of every call (default 0).
--mode both: the two hypothesis modes against each other on the same resident frame and map, same build, same process - five warm-up
calls of each, then `reps` repetitions that alternate mode 0 and mode 1 (`calls` calls each): wall-clock time per call and device
time per kernel group of each mode; then the 16-lane vslam_relocalize_batch call of each mode, alternated in the same way.
usage: python tools/reloc_rate.py --mode both [out.json] [calls] [reps]

--imu: the two phases of vslam_batch_relocalize_imu against each other.  The phases belong to sessions, so the frame and the map here
are a session's own, not the crafted 1 500 x 20 000 shape above: L = 1 and 16 stereo + IMU lanes of a vslam_batch track the rendered
EuRoC source frames 0, 2, 4, 6 (1 500 features; a map of ~2 000 points each), then every lane is relocalised on source frame 4 (first
pose: the pose alone) and on source frame 6 with the bucket between them (second pose: + k_imu_preintegrate_b and k_reloc_velocity_b) -
the two calls alternate by construction, same build, same process.  Five warm-up pairs, then `reps` repetitions of `pairs` pairs: wall
clock per call of each phase (host clock around a call that ends in a device synchronise), timing off; then one repetition with the
batch's stage timing on for the device time of every stage of each phase.
usage: python tools/reloc_rate.py --imu [out.json] [pairs] [reps]"""
import json, os, sys, time
os.environ.setdefault("OMP_NUM_THREADS", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("gtsam-vslam_amd", "tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np
import synth
import vslam_capi as vc

N_KEYS, N_POINTS, N_TRUE = 1500, 20000, 1200
RIG = synth.RIGS["euroc"]
MODE = 0            # --mode


def flip(desc, k, rng):
    out = desc.copy()
    for b in rng.choice(256, size=k, replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def build(seed=1):
    rng = np.random.Generator(np.random.PCG64(seed))
    n = N_KEYS
    kL = np.zeros(n, vc.KP_DTYPE); kR = np.zeros(n, vc.KP_DTYPE)
    u = rng.uniform(60, RIG["w"] - 40, n).astype(np.float32); v = rng.uniform(40, RIG["h"] - 40, n).astype(np.float32)
    z = rng.uniform(2.0, 8.0, n).astype(np.float32)
    kL["x"], kL["y"], kL["octave"] = u, v, rng.integers(0, 8, n)
    kR["x"] = (u - RIG["fx"] * RIG["bl"] / z).astype(np.float32); kR["y"] = v; kR["octave"] = kL["octave"]
    dL = rng.integers(0, 256, (n, 32), dtype=np.uint8); dR = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    w = np.array([0.3, -0.4, 0.2]); th = np.linalg.norm(w); K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K); t = np.array([0.8, -0.3, 1.1])
    zp = z.astype(np.float64)
    Xc = np.stack([(u - RIG["cx"]) * zp / RIG["fx"], (v - RIG["cy"]) * zp / RIG["fy"], zp], axis=1)
    Xw_keys = (Xc - t) @ R
    points = rng.uniform(-8, 8, (N_POINTS, 3)); desc = rng.integers(0, 256, (N_POINTS, 32), dtype=np.uint8)
    where = rng.permutation(N_POINTS)[:N_TRUE]; keys = rng.permutation(n)[:N_TRUE]
    for j, (p, k) in enumerate(zip(where, keys)):
        desc[p] = flip(dL[k], int(rng.integers(0, 31)), rng)
        if j % 5 < 3:
            points[p] = Xw_keys[k]
    return dict(kL=kL, dL=dL, kR=kR, dR=dR, best=np.arange(n, dtype=np.int32), depth=z, sad=np.full(n, 10, np.int32),
                points=points, desc=desc)


def main_lanes(argv):
    out_path = argv[0] if len(argv) > 0 else os.path.join(ROOT, "profiles", "reloc_batch_rate.json")
    calls = int(argv[1]) if len(argv) > 1 else 30
    reps = int(argv[2]) if len(argv) > 2 else 3
    if vc.device_count() < 1:
        raise RuntimeError("reloc_rate needs a GPU: a time taken anywhere else says nothing about the stage")
    LMAX = 16
    ge = vc.Extractor(RIG["w"], RIG["h"], 1500, batch=2 * LMAX)
    ms, gs = [], []
    for b in range(LMAX):
        g = build(seed=1 + b)
        m = vc.Matcher(RIG, ge, 2 * b, ge, 2 * b + 1)
        m.stereo_finalize_arrays(g["best"], g["depth"], g["sad"], N_KEYS)
        m.set_keys(0, g["kL"], g["dL"]); m.set_keys(1, g["kR"], g["dR"])
        m.set_timing(False)
        ms.append(m); gs.append(g)
    pts = [g["points"] for g in gs]; dsc = [g["desc"] for g in gs]
    res = dict(keys=N_KEYS, map_points=N_POINTS, hypotheses=256, mode=MODE, calls_per_repetition=calls, repetitions=reps, lanes={})
    for L in (1, 4, 16):
        def batched():
            return vc.relocalize_batch(ms[:L], pts[:L], dsc[:L], mode=MODE)

        def sequential():
            return [ms[b].relocalize(pts[b], dsc[b], pairs=True, mode=MODE) for b in range(L)]

        for _ in range(5):
            Tb, repb, _ = batched()
            seq = sequential()
        same = all(repb[b][k] == seq[b][1][k] for b in range(L) for k in ("success", "n_pairs", "best_hypothesis", "best_count", "n_inliers", "n_stereo")) and \
            all(seq[b][0] is not None and float(np.abs(seq[b][0] - Tb[b]).max()) < 1e-12 for b in range(L))
        wb, ws = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(calls):
                batched()
            wb.append((time.perf_counter() - t0) / calls * 1e3)
            t0 = time.perf_counter()
            for _ in range(calls):
                sequential()
            ws.append((time.perf_counter() - t0) / calls * 1e3)
        stat = lambda v: dict(median=float(np.median(v)), min=min(v), max=max(v))
        res["lanes"][str(L)] = dict(batched_call_ms=stat(wb), sequential_calls_ms=stat(ws), batched_over_sequential=float(np.median(wb) / np.median(ws)),
                                    batched_ms_per_lane=float(np.median(wb)) / L, lanes_equal_the_single_calls=bool(same),
                                    inliers=[repb[b]["n_inliers"] for b in range(L)])
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main_modes(argv):
    out_path = argv[0] if len(argv) > 0 else os.path.join(ROOT, "profiles", "reloc_p3p_rate.json")
    calls = int(argv[1]) if len(argv) > 1 else 50
    reps = int(argv[2]) if len(argv) > 2 else 3
    if vc.device_count() < 1:
        raise RuntimeError("reloc_rate needs a GPU: a time taken anywhere else says nothing about the stage")
    stat = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    LMAX = 16
    ge = vc.Extractor(RIG["w"], RIG["h"], 1500, batch=2 * LMAX)
    ms, gs = [], []
    for b in range(LMAX):
        g = build(seed=1 + b)
        m = vc.Matcher(RIG, ge, 2 * b, ge, 2 * b + 1)
        m.stereo_finalize_arrays(g["best"], g["depth"], g["sad"], N_KEYS)
        m.set_keys(0, g["kL"], g["dL"]); m.set_keys(1, g["kR"], g["dR"])
        ms.append(m); gs.append(g)
    res = dict(keys=N_KEYS, map_points=N_POINTS, hypotheses=256, calls_per_repetition=calls, repetitions=reps, single_call={}, batched_16_lanes={})
    # ---- one call on one matcher, timing on: wall clock and kernel groups, the modes alternated
    m, g = ms[0], gs[0]
    st = m.stereo_fetch(N_KEYS, N_KEYS)
    last = {}
    for _ in range(5):
        for mode in (0, 1):
            last[mode] = m.relocalize(g["points"], g["desc"], pairs=False, mode=mode)
    m.timings()
    wall, groups = {0: [], 1: []}, {0: [], 1: []}
    for _ in range(reps):
        for mode in (0, 1):
            t0 = time.perf_counter()
            for _ in range(calls):
                m.relocalize(g["points"], g["desc"], pairs=False, mode=mode)
            wall[mode].append((time.perf_counter() - t0) / calls * 1e3)
            groups[mode].append({k: v / calls for k, v in m.timings().items()})
    import pyoracle, reloc_p3p_ref as pp
    ref = pp.relocalize(pyoracle, RIG, pyoracle.Extractor(1500).InvSigmaFactor, g["points"], g["desc"], g["kL"], g["dL"], g["kR"], st, mode=1)
    T1, rep1, _ = last[1]
    for mode in (0, 1):
        rep = last[mode][1]
        res["single_call"]["mode_%d" % mode] = dict(
            report={k: rep[k] for k in ("success", "n_pairs", "best_count", "n_inliers", "n_stereo")}, wall_ms_per_call=stat(wall[mode]),
            device_ms_per_call={k: stat([gr.get(k, 0.0) for gr in groups[mode]]) for k in sorted(groups[mode][0])})
    res["single_call"]["mode_1"]["same_result_as_restatement"] = bool(
        ref["n_pairs"] == rep1["n_pairs"] and ref["best_count"] == rep1["best_count"] and ref["n_inliers"] == rep1["n_inliers"] and
        ref["T_cw"] is not None and T1 is not None and float(np.abs(ref["T_cw"] - T1).max()) < 1e-7)
    # ---- the 16-lane batched call, timing off
    for m in ms:
        m.set_timing(False)
    pts = [g["points"] for g in gs]; dsc = [g["desc"] for g in gs]
    reps_b = {}
    for _ in range(5):
        for mode in (0, 1):
            reps_b[mode] = vc.relocalize_batch(ms, pts, dsc, mode=mode)[1]
    wb = {0: [], 1: []}
    for _ in range(reps):
        for mode in (0, 1):
            t0 = time.perf_counter()
            for _ in range(calls):
                vc.relocalize_batch(ms, pts, dsc, mode=mode)
            wb[mode].append((time.perf_counter() - t0) / calls * 1e3)
    for mode in (0, 1):
        res["batched_16_lanes"]["mode_%d" % mode] = dict(batched_call_ms=stat(wb[mode]), batched_ms_per_lane=float(np.median(wb[mode])) / LMAX,
                                                         inliers=[r["n_inliers"] for r in reps_b[mode]], pairs=[r["n_pairs"] for r in reps_b[mode]])
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main_imu(argv):
    out_path = argv[0] if len(argv) > 0 else os.path.join(ROOT, "profiles", "reloc_imu_rate.json")
    pairs = int(argv[1]) if len(argv) > 1 else 20
    reps = int(argv[2]) if len(argv) > 2 else 3
    if vc.device_count() < 1:
        raise RuntimeError("reloc_rate needs a GPU: a time taken anywhere else says nothing about the stage")
    fps = RIG["fps"]
    imu = dict(gravity=(0.0, 9.81, 0.0), noise=(1.6968e-4, 1.9393e-5, 2.0e-3, 3.0e-3), T_bs=synth.T_BC1, hz=200)
    stat = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))

    def velocity(f):
        h = 1e-4
        return (synth.pose_at(f + h * fps, fps)[:3, 3] - synth.pose_at(f - h * fps, fps)[:3, 3]) / (2 * h)

    def bucket(f0, f1):
        S, dts, _ = synth.imu_samples(f0, f1, fps, noise_seed=0x1A00 + f1)
        return (S[:, :3], S[:, 3:], np.arange(len(dts)) * 5e6)

    src = [0, 2, 4, 6]
    synth.prerender(src)
    frames = [synth.stereo_frame(f) for f in src]
    res = dict(features=1500, source_frames=src, mode=MODE, pairs_per_repetition=pairs, repetitions=reps, lanes={})
    for L in (1, 16):
        bt = vc.Batch(RIG, 1500, L, T0s=[synth.pose_at(0, fps)] * L, imu=imu, velocities=[velocity(0)] * L, local_mapping=1, host_threads=min(L, 8))
        for n, f in enumerate(src):
            bt.track([frames[n][0]] * L, [frames[n][1]] * L, [n] * L, imu_buckets=[bucket(src[n - 1], f)] * L if n else None)
        fn = [len(src)]
        bk = [bucket(4, 6)] * L

        def pair(wall=None):
            out = []
            for ph, (k, b) in enumerate(((2, None), (3, bk))):
                t0 = time.perf_counter()
                T, rr_, ir = bt.relocalize_imu([frames[k][0]] * L, [frames[k][1]] * L, [fn[0]] * L, imu_buckets=b, mode=MODE)
                if wall is not None:
                    wall[ph].append((time.perf_counter() - t0) * 1e3)
                fn[0] += 1
                out.append((rr_, ir))
            return out

        for _ in range(5):
            last = pair()
        ok = all(last[0][1][b]["phase"] == 1 and last[1][1][b]["phase"] == 2 for b in range(L))
        med = [[], []]
        for _ in range(reps):
            wall = [[], []]
            for _ in range(pairs):
                pair(wall)
            for ph in range(2):
                med[ph].append(float(np.mean(wall[ph])))
        bt.set_timing(True)
        pair()
        bt.timings()
        dev = [{}, {}]
        for _ in range(pairs):
            for ph, (k, b) in enumerate(((2, None), (3, bk))):
                bt.relocalize_imu([frames[k][0]] * L, [frames[k][1]] * L, [fn[0]] * L, imu_buckets=b, mode=MODE)
                fn[0] += 1
                for name, ms in bt.timings()[0].items():
                    if name.startswith("reloc_"):
                        dev[ph].setdefault(name, []).append(ms)
        bt.set_timing(False)
        res["lanes"][str(L)] = dict(
            phases_as_expected=bool(ok), map_points=last[1][0][0]["n_points"], pairs=last[1][0][0]["n_pairs"], inliers=last[1][0][0]["n_inliers"],
            dt=last[1][1][0]["dt"], rot_residual=last[1][1][0]["rot_residual"],
            first_pose_call_ms=stat(med[0]), second_pose_call_ms=stat(med[1]), second_minus_first_ms=float(np.median(med[1]) - np.median(med[0])),
            device_ms_per_call_first_pose={k: stat(v) for k, v in sorted(dev[0].items())},
            device_ms_per_call_second_pose={k: stat(v) for k, v in sorted(dev[1].items())})
        bt.close()
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main():
    global MODE
    if "--mode" in sys.argv:
        k = sys.argv.index("--mode")
        mode = sys.argv[k + 1]
        del sys.argv[k:k + 2]
        if mode == "both":
            return main_modes(sys.argv[1:])
        MODE = int(mode)
    if len(sys.argv) > 1 and sys.argv[1] == "--imu":
        return main_imu(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--lanes":
        return main_lanes(sys.argv[2:])
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "reloc_rate.json")
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    if vc.device_count() < 1:
        raise RuntimeError("reloc_rate needs a GPU: a time taken anywhere else says nothing about the stage")
    g = build()
    ge = vc.Extractor(RIG["w"], RIG["h"], 1500, batch=2)
    m = vc.Matcher(RIG, ge, 0, ge, 1)
    m.stereo_finalize_arrays(g["best"], g["depth"], g["sad"], N_KEYS)
    m.set_keys(0, g["kL"], g["dL"]); m.set_keys(1, g["kR"], g["dR"])
    st = m.stereo_fetch(N_KEYS, N_KEYS)
    for _ in range(5):
        T, rep, _ = m.relocalize(g["points"], g["desc"], pairs=False, mode=MODE)
    m.timings()
    wall, groups = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            m.relocalize(g["points"], g["desc"], pairs=False, mode=MODE)
        wall.append((time.perf_counter() - t0) / calls * 1e3)
        groups.append({k: v / calls for k, v in m.timings().items()})
    res = dict(keys=N_KEYS, map_points=N_POINTS, hypotheses=256, mode=MODE, calls_per_repetition=calls, repetitions=reps,
               report={k: rep[k] for k in ("success", "n_pairs", "best_count", "n_inliers", "n_stereo")},
               hamming_tests_per_call=N_KEYS * N_POINTS,
               wall_ms_per_call=dict(median=float(np.median(wall)), min=min(wall), max=max(wall)),
               device_ms_per_call={k: dict(median=float(np.median([gr.get(k, 0.0) for gr in groups])), min=min(gr.get(k, 0.0) for gr in groups),
                                           max=max(gr.get(k, 0.0) for gr in groups)) for k in sorted(groups[0])})
    mt = res["device_ms_per_call"].get("reloc_match", {}).get("median", 0.0)
    if mt > 0:
        res["hamming_tests_per_second_in_k_reloc_match"] = N_KEYS * N_POINTS / (mt * 1e-3)
    # context: the numpy restatement on one core (best of three)
    import pyoracle, reloc_ref as rr, reloc_p3p_ref as pp
    inv_sigma = pyoracle.Extractor(1500).InvSigmaFactor
    cpu = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref = (pp if MODE else rr).relocalize(pyoracle, RIG, inv_sigma, g["points"], g["desc"], g["kL"], g["dL"], g["kR"], st, **(dict(mode=1) if MODE else {}))
        cpu.append((time.perf_counter() - t0) * 1e3)
    res["numpy_restatement_one_core_ms"] = dict(best=min(cpu), all=cpu)
    res["same_result_as_restatement"] = bool(ref["n_pairs"] == rep["n_pairs"] and ref["best_count"] == rep["best_count"] and
                                             ref["n_inliers"] == rep["n_inliers"] and ref["T_cw"] is not None and T is not None and
                                             float(np.abs(ref["T_cw"] - T).max()) < 1e-7)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
