"""Time of one vslam_pose_graph_optimize call on out-and-back keyframe chains of 200, 1 000 and 4 000 poses.

The chain walks 0.1 m per keyframe along a gently curving path and returns over it; every pose is tied to its next two
successors ((k, k + 1) and (k, k + 2): two sequential-range edges per pose) with measurement noise of up to 0.002 rad / 0.005 m,
and ONE loop edge ties the last pose to pose 5.  Pose 0 is fixed; the start is the chain of the (k, k + 1) measurements, so the
loop edge carries the accumulated drift.  Every call uploads the graph, runs the LM loop and downloads the poses, as a caller's
call does.
Reported per size: the wall-clock time of a call (host clock around the call, which ends in a device synchronise) - two warm-up
calls, then `reps` repetitions of `calls` calls, median and range over the repetitions; the half-bandwidth after the reordering,
the LM trials, the costs; then, from one more repetition with the library's HIP-event timing on, the device time per kernel
group of a call.  Beside it, as context only, the time of the numpy restatement (tests/pgo_ref.py, dense solve) for the sizes a
dense solve can hold (200 and 1 000 poses), with the thread count numpy ran with.
usage: python tools/pgo_rate.py [out.json] [calls] [reps]

python tools/pgo_rate.py --lanes G [out.json] [calls] [reps] times vslam_pose_graph_optimize_batch instead: per nominal size (200 and
1 000 poses) G such chains of DIFFERENT lengths, spread evenly over 0.7 .. 1.3 of the nominal size, each with its own noise, so that
the lanes stop in different rounds.  Same protocol; reported per nominal size: the batched call, the G single calls of the same
graphs one after another, the single call on the nominal chain alone (the figure profiles/pgo_rate.json holds for the single call),
the rounds of the batched call (its longest lane's trials) against every lane's trials, and whether every lane's poses equal its
single call's bytes.  Default output: profiles/pgo_batch_rate.json.

python tools/pgo_rate.py --yaw [out.json] [calls] [reps] times vslam_pose_graph_optimize_yaw (axis (0, 1, 0)) on the 1 000- and
4 000-pose chains, and vslam_pose_graph_optimize on the same graphs in the same process as the yardstick.  Same protocol; per size
and solve: the call's time, the trials, the costs, the device time per kernel group, and the walk's cost per block column
(the band_chol group over trials x free poses: the walk's dependency chain is what bounds it).  The two
solves run different numbers of trials on different problems, so the per-column and per-trial figures are the comparable ones.
Default output: profiles/pgo_yaw_rate.json."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("gtsam-vslam_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np
import pgo_ref as pr
import vslam_capi as vc

SIZES = (200, 1000, 4000)
REF_SIZES = (200, 1000)
BATCH_SIZES = (200, 1000)


def out_and_back(n, seed=1):
    rng = np.random.default_rng(seed)
    half = n // 2
    truth = []
    for k in range(n):
        s = k if k < half else n - 1 - k              # position along the path: out, then back over it
        truth.append(pr.make_pose(pr.so3_exp(np.array([0.0, 0.3 * np.sin(0.01 * s), 0.0])),
                                  np.array([0.5 * np.sin(0.02 * s), 0.0, 0.1 * s])))
    edges = [pr.noisy_edge(rng, truth, k, k + 1, 0.002, 0.005) for k in range(n - 1)]
    edges += [pr.noisy_edge(rng, truth, k, k + 2, 0.002, 0.005) for k in range(n - 2)]
    edges.append(pr.noisy_edge(rng, truth, n - 1, 5, 0.002, 0.005, 10.0, 10.0))
    poses = [truth[0]]
    for k in range(n - 1):
        poses.append(poses[-1] @ edges[k][2])
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return np.array(poses), fixed, edges


def timed(fn, calls, reps):
    for _ in range(2):
        fn()
    per = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        per.append((time.perf_counter() - t0) / calls * 1e3)
    return dict(median=float(np.median(per)), min=float(min(per)), max=float(max(per)))


def main_lanes(G, argv):
    out_path = argv[0] if len(argv) > 0 else os.path.join(ROOT, "profiles", "pgo_batch_rate.json")
    calls = int(argv[1]) if len(argv) > 1 else 3
    reps = int(argv[2]) if len(argv) > 2 else 3
    res = dict(protocol="2 warm-up calls, %d repetitions of %d calls, host clock around calls that end in a device synchronise" % (reps, calls),
               lanes=G, sizes={})
    for nominal in BATCH_SIZES:
        ns = [int(round(nominal * (0.7 + 0.6 * g / max(G - 1, 1)))) for g in range(G)]
        graphs = []
        for g, n in enumerate(ns):
            poses, fixed, edges = out_and_back(n, seed=1 + g)
            graphs.append((poses, fixed, vc.pgo_edges(edges)))
        nom = out_and_back(nominal)
        nom = (nom[0], nom[1], vc.pgo_edges(nom[2]))
        batched = vc.pose_graph_optimize_batch(graphs)
        singles = [vc.pose_graph_optimize(*g) for g in graphs]
        same = all(b[0].tobytes() == s[0].tobytes() and b[1] == s[1] for b, s in zip(batched, singles))
        t_batch = timed(lambda: vc.pose_graph_optimize_batch(graphs), calls, reps)
        t_singles = timed(lambda: [vc.pose_graph_optimize(*g) for g in graphs], calls, reps)
        t_longest = timed(lambda: vc.pose_graph_optimize(*graphs[-1]), calls, reps)
        t_nominal = timed(lambda: vc.pose_graph_optimize(*nom), calls, reps)
        trials = [r[1]["iterations"] for r in batched]
        r = dict(nominal_poses=nominal, lane_poses=ns, lane_trials=trials, rounds=max(trials), sum_of_trials=sum(trials),
                 half_bandwidth=[b[1]["half_bandwidth"] for b in batched], lanes_equal_single_calls_bitwise=bool(same),
                 ms_batched_call=t_batch, ms_single_calls_in_sequence=t_singles, ms_single_call_longest_lane=t_longest,
                 ms_single_call_nominal_chain=t_nominal)
        res["sizes"][str(nominal)] = r
        print(json.dumps(r), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


YAW_SIZES = (1000, 4000)


def main_yaw(argv):
    out_path = argv[0] if len(argv) > 0 else os.path.join(ROOT, "profiles", "pgo_yaw_rate.json")
    calls = int(argv[1]) if len(argv) > 1 else 3
    reps = int(argv[2]) if len(argv) > 2 else 3
    axis = (0.0, 1.0, 0.0)
    res = dict(protocol="2 warm-up calls, %d repetitions of %d calls, host clock around calls that end in a device synchronise; kernel "
                        "groups from HIP events of one more repetition; both solves in one process, the 6-DoF call first" % (reps, calls),
               axis=axis, sizes={})
    for n in YAW_SIZES:
        poses, fixed, edges = out_and_back(n)
        ea = vc.pgo_edges(edges)
        solves = (("six_dof", "pgo_band_chol", lambda: vc.pose_graph_optimize(poses, fixed, ea)),
                  ("yaw", "pgoy_band_chol", lambda: vc.pose_graph_optimize_yaw(poses, fixed, ea, axis)))
        r = dict(poses=n, edges=len(edges))
        for name, walk, fn in solves:
            t = timed(fn, calls, reps)
            out, rep = fn()
            vc.pose_graph_set_timing(True)
            groups = {}
            for _ in range(calls):
                fn()
                for k, v in vc.pose_graph_timings().items():
                    groups[k] = groups.get(k, 0.0) + v / calls
            vc.pose_graph_set_timing(False)
            cols = rep["iterations"] * rep["n_free"]
            r[name] = dict(ms_per_call=t, kernel_group_ms=groups, half_bandwidth=rep["half_bandwidth"], lm_trials=rep["iterations"],
                           accepted=rep["accepted"], rejected=rep["rejected"], initial_cost=rep["initial_cost"], final_cost=rep["final_cost"],
                           ms_per_trial=t["median"] / max(rep["iterations"], 1),
                           band_chol_us_per_column=1e3 * groups.get(walk, 0.0) / max(cols, 1))
        res["sizes"][str(n)] = r
        print(json.dumps(r), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main(argv):
    if "--yaw" in argv:
        return main_yaw([a for a in argv if a != "--yaw"])
    if "--lanes" in argv:
        k = argv.index("--lanes")
        return main_lanes(int(argv[k + 1]), argv[:k] + argv[k + 2:])
    out_path = argv[0] if len(argv) > 0 else os.path.join(ROOT, "profiles", "pgo_rate.json")
    calls = int(argv[1]) if len(argv) > 1 else 3
    reps = int(argv[2]) if len(argv) > 2 else 3
    res = dict(protocol="2 warm-up calls, %d repetitions of %d calls, host clock around calls that end in a device synchronise; "
                        "kernel groups from HIP events of one more repetition" % (reps, calls), sizes={})
    for n in SIZES:
        poses, fixed, edges = out_and_back(n)
        ea = vc.pgo_edges(edges)
        for _ in range(2):
            out, rep = vc.pose_graph_optimize(poses, fixed, ea)
        per = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(calls):
                vc.pose_graph_optimize(poses, fixed, ea)
            per.append((time.perf_counter() - t0) / calls * 1e3)
        vc.pose_graph_set_timing(True)
        groups = {}
        for _ in range(calls):
            vc.pose_graph_optimize(poses, fixed, ea)
            for k, v in vc.pose_graph_timings().items():
                groups[k] = groups.get(k, 0.0) + v / calls
        vc.pose_graph_set_timing(False)
        r = dict(poses=n, edges=len(edges), ms_per_call=dict(median=float(np.median(per)), min=float(min(per)), max=float(max(per))),
                 kernel_group_ms=groups, half_bandwidth=rep["half_bandwidth"], lm_trials=rep["iterations"], accepted=rep["accepted"],
                 rejected=rep["rejected"], initial_cost=rep["initial_cost"], final_cost=rep["final_cost"])
        if n in REF_SIZES:
            t0 = time.perf_counter()
            want, wrep = pr.optimize(poses, fixed, edges)
            r["restatement"] = dict(seconds=time.perf_counter() - t0, threads=os.environ.get("OMP_NUM_THREADS", "unset"),
                                    max_pose_difference=float(np.abs(want - out).max()), final_cost=wrep["final_cost"], trials=wrep["iterations"])
        res["sizes"][str(n)] = r
        print(json.dumps(r), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
