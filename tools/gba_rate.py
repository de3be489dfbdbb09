"""Time of one vslam_global_ba call on out-and-back corridors of 200, 1 000 and 2 000 keyframes at the bench workload's density.

The camera walks 0.3 m per keyframe along x, looking sideways (+z) at landmarks 2 - 5 m away, and returns beside its own track.
Every keyframe of the way out starts 50 landmarks that it and its next two keyframes see (about 100 landmarks per keyframe); the
first view of a landmark is a left + right pair, the others are left only, and every third landmark is seen again, the same way,
by the three keyframes of the way back that stand beside them: about 5 factors per landmark.  Keyframe 0 is fixed; measurements
carry 0.3 px of noise (times 1.2^octave), the start is the truth disturbed by 0.004 rad / 0.01 m per keyframe and 0.01 m per point.
Every call uploads the problem, runs the LM loop and downloads the result, as a caller's call does.
Reported per size: the wall-clock time of a call - two warm-up calls, then `reps` repetitions of `calls` calls, median and range
over the repetitions; the half-bandwidth b after the reordering, the trials, the costs; from one more call with the library's
HIP-event timing on, the device time per kernel group; microseconds of the factorisation group per block column and trial.
Then one problem both bundle adjustments can run, 150 free keyframes of the same corridor: vslam_local_ba (two passes, dense
reduced system) and vslam_global_ba side by side, with the time per LM trial of each.  Numbers only, no bar.
With --lanes N: N such corridors of unequal length (150 .. 250 free keyframes, evenly spread) as ONE vslam_global_ba_batch call
against the same problems as N vslam_global_ba calls one after the other: two warm-up calls, `reps` repetitions, the wall clock of
whole calls (upload, loop, download), the device time per kernel group of one more call of each kind, and whether every lane's
bytes equal its single call's.  Writes profiles/gba_batch_rate.json.
With --yaw: vslam_global_ba_yaw / _batch beside the 6-DoF calls in the same process, on the 2 000-keyframe corridor (single) and
on the sixteen corridors of --lanes 16 (batched), with the per-group timings of both.  Writes profiles/gba_yaw_rate.json.
usage: python tools/gba_rate.py [out.json] [calls] [reps]
       python tools/gba_rate.py --lanes N [out.json] [reps]
       python tools/gba_rate.py --yaw [out.json] [reps]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("gtsam-vslam_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np
import gba_ref as gr
import pgo_ref as pr
import vslam_capi as vc

SIZES = (200, 1000, 2000)
PER_KF = 50


def corridor(n_free, seed=1):
    rng = np.random.default_rng(seed)
    K = n_free + 1
    half = n_free // 2
    xs = np.array([0.3 * (k if k <= half else n_free - k) for k in range(K)])
    truth = np.array([gr.look_z(xs[k], 0.0 if k <= half else 0.06, 0.01 * np.cos(0.3 * k), 0.02 * np.sin(0.2 * k)) for k in range(K)])
    start_kf = np.repeat(np.arange(half - 1), PER_KF)
    L = len(start_kf)
    lm = np.stack([xs[start_kf] + rng.uniform(-0.8, 1.4, L), rng.uniform(-0.8, 0.8, L), rng.uniform(2.0, 5.0, L)], 1)
    pk, pl, pf = [], [], []
    for j in range(3):
        pk.append(start_kf + j); pl.append(np.arange(L)); pf.append(np.full(L, 3 if j == 0 else 1))
    again = np.flatnonzero(np.arange(L) % 3 == 0)
    for j in range(3):
        kb = n_free - (start_kf[again] + j)
        ok = (kb > half) & (kb < K)
        pk.append(kb[ok]); pl.append(again[ok]); pf.append(np.full(int(ok.sum()), 3 if j == 0 else 1))
    pk, pl, pf = np.concatenate(pk), np.concatenate(pl), np.concatenate(pf)
    order = np.lexsort((pk, pl))
    pk, pl, pf = pk[order], pl[order], pf[order]
    fx, fy, cx, cy, bl = gr.camera(gr.RIG)
    R, t = truth[pk, :3, :3], truth[pk, :3, 3]
    q = np.einsum("nji,nj->ni", R, lm[pl] - t)
    octv = np.clip(np.round(np.log(q[:, 2] / 2.0) / np.log(1.2)), 0, 7).astype(np.int32)
    uv = np.stack([fx * q[:, 0] / q[:, 2] + cx, fy * q[:, 1] / q[:, 2] + cy, fx * (q[:, 0] - bl) / q[:, 2] + cx, fy * q[:, 1] / q[:, 2] + cy], 1)
    uv += rng.normal(0, 0.3, uv.shape) * gr.SCALE[octv][:, None]
    start = truth.copy()
    for k in range(1, K):
        start[k] = truth[k] @ pr.random_pose(rng, 0.004, 0.01)
    fixed = np.zeros(K, np.uint8)
    fixed[0] = 1
    return dict(rig=gr.RIG, kf_pose=start, kf_id=np.arange(K, dtype=np.int64), kf_fixed=fixed, kf_local=np.ones(K, np.uint8),
                lm=lm + rng.normal(0, 0.01, lm.shape), pair_kf=pk.astype(np.int32), pair_lm=pl.astype(np.int32), pair_flags=pf.astype(np.uint8),
                pair_uv=uv.astype(np.float32), pair_oct=np.stack([octv, octv], 1).astype(np.int32))


def timed(fn, calls, reps):
    for _ in range(2):
        fn()
    per = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        per.append(1e3 * (time.perf_counter() - t0) / calls)
    return dict(median=float(np.median(per)), min=float(min(per)), max=float(max(per)))


def batch_main(n_lanes, argv):
    out_path = argv[0] if argv else os.path.join(ROOT, "profiles", "gba_batch_rate.json")
    reps = int(argv[1]) if len(argv) > 1 else 3
    sizes = [int(round(v)) for v in np.linspace(150, 250, n_lanes)] if n_lanes > 1 else [200]
    probs = [corridor(n, seed=10 + i) for i, n in enumerate(sizes)]
    lanes = [dict(rig=p["rig"], sigma_factor=gr.SIGMA, inv_sigma_factor=gr.INV_SIGMA, prob=p) for p in probs]
    single = lambda: [vc.global_ba(p["rig"], gr.SIGMA, gr.INV_SIGMA, p) for p in probs]
    batch = lambda: vc.global_ba_batch(lanes)
    a, b = single(), batch()
    same = all(x[k].tobytes() == y[k].tobytes() for x, y in zip(a, b) for k in ("kf_pose", "lm", "pair_wrong")) and \
        all(x["report"] == y["report"] for x, y in zip(a, b))
    ms_single, ms_batch = timed(single, 1, reps), timed(batch, 1, reps)
    longest = int(np.argmax([r["report"]["iterations"] * r["report"]["n_free"] for r in a]))
    p = probs[longest]
    ms_longest = timed(lambda: vc.global_ba(p["rig"], gr.SIGMA, gr.INV_SIGMA, p), 1, reps)
    vc.global_ba_set_timing(True)
    batch()
    g_batch = vc.global_ba_timings()
    g_single = {}
    for p in probs:
        vc.global_ba(p["rig"], gr.SIGMA, gr.INV_SIGMA, p)
        for k, v in vc.global_ba_timings().items():
            g_single[k] = g_single.get(k, 0.0) + v
    vc.global_ba_set_timing(False)
    res = dict(protocol="2 warm-up calls, %d repetitions, host clock around whole calls (upload, LM loop, download); kernel groups from HIP "
                        "events of one more call of each kind (the single calls' groups summed over the lanes)" % reps,
               lanes=n_lanes, free_keyframes=sizes, landmarks=[len(p["lm"]) for p in probs], pairs=[len(p["pair_kf"]) for p in probs],
               half_bandwidth=[r["report"]["half_bandwidth"] for r in a], lm_trials=[r["report"]["iterations"] for r in a],
               rounds=max(r["report"]["iterations"] for r in a), lanes_equal_single_calls_bitwise=bool(same),
               ms_batched_call=ms_batch, ms_single_calls_together=ms_single, ms_longest_lane_alone=dict(ms_longest, lane=longest),
               single_over_batched=ms_single["median"] / ms_batch["median"], batched_over_longest_lane=ms_batch["median"] / ms_longest["median"],
               kernel_group_ms_batched=g_batch, kernel_group_ms_single_calls_summed=g_single)
    print(json.dumps(res), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


YAW_AXIS = (0.3, 0.9, -0.2)


def yaw_main(argv):
    """vslam_global_ba_yaw beside vslam_global_ba in one process: the 2 000-keyframe corridor as single calls, the sixteen corridors
    of --lanes 16 as batched calls; wall clock of whole calls and the device time per kernel group of one more call of each kind"""
    out_path = argv[0] if argv else os.path.join(ROOT, "profiles", "gba_yaw_rate.json")
    reps = int(argv[1]) if len(argv) > 1 else 3
    groups_of = lambda fn: (vc.global_ba_set_timing(True), fn(), vc.global_ba_timings(), vc.global_ba_set_timing(False))[2]
    report = lambda r: {k: r["report"][k] for k in ("iterations", "accepted", "rejected", "n_free", "half_bandwidth", "initial_cost", "final_cost")}

    def tilt(out, prob):
        g = np.array(YAW_AXIS) / np.linalg.norm(YAW_AXIS)
        return float(max(np.abs(n[:3, :3] @ o[:3, :3].T @ g - g).max() for n, o in zip(out["kf_pose"], prob["kf_pose"])))

    res = dict(protocol="2 warm-up calls, %d repetitions, host clock around whole calls (upload, LM loop, download), both calls alternating "
                        "in one process; kernel groups from HIP events of one more call of each kind; axis (%g, %g, %g)" % ((reps,) + YAW_AXIS))
    prob = corridor(2000)
    six = lambda: vc.global_ba(prob["rig"], gr.SIGMA, gr.INV_SIGMA, prob)
    yaw = lambda: vc.global_ba_yaw(prob["rig"], gr.SIGMA, gr.INV_SIGMA, prob, YAW_AXIS)
    a, b = six(), yaw()
    row = dict(keyframes=2001, landmarks=len(prob["lm"]), pairs=len(prob["pair_kf"]), six_dof=report(a), yaw=report(b),
               gravity_error_six_dof=tilt(a, prob), gravity_error_yaw=tilt(b, prob))
    row["ms_per_call_six_dof"], row["ms_per_call_yaw"] = timed(six, 1, reps), timed(yaw, 1, reps)
    row["ms_per_trial_six_dof"] = row["ms_per_call_six_dof"]["median"] / max(a["report"]["iterations"], 1)
    row["ms_per_trial_yaw"] = row["ms_per_call_yaw"]["median"] / max(b["report"]["iterations"], 1)
    row["kernel_group_ms_six_dof"], row["kernel_group_ms_yaw"] = groups_of(six), groups_of(yaw)
    for name, r in (("six_dof", a), ("yaw", b)):
        row["us_band_chol_per_column_and_trial_" + name] = 1e3 * row["kernel_group_ms_" + name].get("gba_band_chol", 0.0) / (r["report"]["n_free"] * max(r["report"]["iterations"], 1))
    print("single", json.dumps(row), flush=True)
    res["single_2000_keyframes"] = row
    sizes = [int(round(v)) for v in np.linspace(150, 250, 16)]
    probs = [corridor(n, seed=10 + i) for i, n in enumerate(sizes)]
    lanes = [dict(rig=p["rig"], sigma_factor=gr.SIGMA, inv_sigma_factor=gr.INV_SIGMA, prob=p) for p in probs]
    yaw_lanes = [dict(ln, axis=YAW_AXIS) for ln in lanes]
    six_b = lambda: vc.global_ba_batch(lanes)
    yaw_b = lambda: vc.global_ba_yaw_batch(yaw_lanes)
    a, b = six_b(), yaw_b()
    alone = [vc.global_ba_yaw(p["rig"], gr.SIGMA, gr.INV_SIGMA, p, YAW_AXIS) for p in probs]
    same = all(x[k].tobytes() == y[k].tobytes() for x, y in zip(alone, b) for k in ("kf_pose", "lm", "pair_wrong")) and \
        all(x["report"] == y["report"] for x, y in zip(alone, b))
    row = dict(lanes=16, free_keyframes=sizes, lm_trials_six_dof=[r["report"]["iterations"] for r in a], lm_trials_yaw=[r["report"]["iterations"] for r in b],
               half_bandwidth=[r["report"]["half_bandwidth"] for r in b], yaw_lanes_equal_single_calls_bitwise=bool(same))
    row["ms_batched_call_six_dof"], row["ms_batched_call_yaw"] = timed(six_b, 1, reps), timed(yaw_b, 1, reps)
    row["ms_per_round_six_dof"] = row["ms_batched_call_six_dof"]["median"] / max(row["lm_trials_six_dof"])
    row["ms_per_round_yaw"] = row["ms_batched_call_yaw"]["median"] / max(row["lm_trials_yaw"])
    row["kernel_group_ms_six_dof"], row["kernel_group_ms_yaw"] = groups_of(six_b), groups_of(yaw_b)
    print("batched", json.dumps(row), flush=True)
    res["batched_16_corridors"] = row
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


def main():
    if "--yaw" in sys.argv:
        return yaw_main([a for a in sys.argv[1:] if a != "--yaw"])
    if "--lanes" in sys.argv:
        at = sys.argv.index("--lanes")
        return batch_main(int(sys.argv[at + 1]), sys.argv[1:at] + sys.argv[at + 2:])
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gba_rate.json")
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    res = dict(protocol="2 warm-up calls, %d repetitions of %d calls, host clock around calls that end in a device synchronise; kernel groups "
                        "from HIP events of one more call" % (reps, calls), sizes={})
    gba = lambda prob: vc.global_ba(prob["rig"], gr.SIGMA, gr.INV_SIGMA, prob)
    for n in SIZES:
        prob = corridor(n)
        got = gba(prob)
        rep = got["report"]
        ms = timed(lambda: gba(prob), calls, reps)
        vc.global_ba_set_timing(True)
        gba(prob)
        groups = vc.global_ba_timings()
        vc.global_ba_set_timing(False)
        row = dict(keyframes=n + 1, landmarks=len(prob["lm"]), pairs=len(prob["pair_kf"]), factors=rep["n_factors"],
                   landmarks_per_keyframe=len(prob["pair_kf"]) / (n + 1), factors_per_landmark=rep["n_factors"] / max(rep["n_present"], 1),
                   ms_per_call=ms, kernel_group_ms=groups, half_bandwidth=rep["half_bandwidth"], lm_trials=rep["iterations"],
                   accepted=rep["accepted"], rejected=rep["rejected"], initial_cost=rep["initial_cost"], final_cost=rep["final_cost"],
                   us_band_chol_per_column_and_trial=1e3 * groups.get("gba_band_chol", 0.0) / (rep["n_free"] * max(rep["iterations"], 1)))
        print(n, json.dumps(row), flush=True)
        res["sizes"][str(n)] = row
    # one problem both calls can run
    prob = corridor(150, seed=2)
    side = {}
    g = gba(prob)
    side["global_ba"] = dict(ms_per_call=timed(lambda: gba(prob), calls, reps), trials=g["report"]["iterations"], half_bandwidth=g["report"]["half_bandwidth"],
                             initial_cost=g["report"]["initial_cost"], final_cost=g["report"]["final_cost"])
    side["global_ba"]["ms_per_trial"] = side["global_ba"]["ms_per_call"]["median"] / max(g["report"]["iterations"], 1)
    try:
        lba = lambda: vc.local_ba(prob["rig"], gr.SIGMA, gr.INV_SIGMA, prob)
        l = lba()
        trials = sum(r["inner"] for r in l["reports"])
        side["local_ba"] = dict(ms_per_call=timed(lba, calls, reps), trials=trials, lm_iterations=[r["iterations"] for r in l["reports"]],
                                final_error_x2=[2 * r["finalError"] for r in l["reports"]], free_kf=int(l["free_kf"]),
                                max_pose_difference_to_global=float(np.abs(l["kf_pose"] - g["kf_pose"]).max()))
        side["local_ba"]["ms_per_trial"] = side["local_ba"]["ms_per_call"]["median"] / max(trials, 1)
    except vc.VslamError as e:
        side["local_ba"] = dict(error=str(e))
    res["side_by_side_150_free_keyframes"] = dict(keyframes=151, landmarks=len(prob["lm"]), pairs=len(prob["pair_kf"]), **side,
                                                  note="the local BA adds between factors along kf_id and runs two passes of 5 + 10 iterations at "
                                                       "tolerance 1e-5; the global BA runs one pass to a relative decrease of 1e-10: the results differ by design")
    print(json.dumps(res["side_by_side_150_free_keyframes"]), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
