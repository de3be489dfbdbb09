"""Device time of the projection-matching kernels alone at the bench shape: ONE primed group of 128 lanes on the corridor
sequence of bench.py's default (C2), both passes of a frame (radius 10, then 4), by the batch's per-stage HIP events.
usage: python tools/proj_rate.py [--lib PATH] [--lanes 128] [--prime 160] [--steps 30] [--reps 3] [--hist]
  --lib   the library to measure (default: the tree's) - e.g. the parent commit's build, for an A/B in one GPU session
  --hist  the library was built with -DVSLAM_PROJ_HIST: also print how many keys a (map point, side) job walks over and how
          many it tests (vslam_debug_proj_hist), over every frame of the run
VSLAM_PROJ_SELECT=0 in the environment measures the general selection of the same build.
One JSON line: per repetition the microseconds per launch of k_proj_cells_b / k_proj_candidates_b / k_proj_resolve_b."""
import argparse, ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "gtsam-vslam_amd"))
ap = argparse.ArgumentParser()
ap.add_argument("--lib", default="")
ap.add_argument("--lanes", type=int, default=128)
ap.add_argument("--prime", type=int, default=160)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--hist", action="store_true")
args = ap.parse_args()
import numpy as np
import bench
import torch, synth
import vslam_capi as vc
if args.lib:
    vc.LIB_PATH = os.path.abspath(args.lib)
cfg = bench.CONFIGS["c2"]
dev = torch.device("cuda", 0)
nfr = 640
rig, Ls, Rs, poses, vel, fwd, bwd = bench.make_corridor_sequence(cfg, nfr, 1, 0.5, 0, dev)
torch.cuda.synchronize()
lp = [Ls[j].data_ptr() for j in range(nfr)]; rp = [Rs[j].data_ptr() for j in range(nfr)]
need = args.prime + 10 + args.steps * args.reps + 2
imu = dict(gravity=bench.GRAVITY, noise=bench.IMU_NOISE, T_bs=synth.T_BC1, hz=200)
scfg = vc.system_config(rig, cfg["nfeat"], imu=imu, local_mapping=2, device=0, mapping_delay=4, mapping_np_delay=2)
fl = vc.Fleet(scfg, args.lanes, lp, rp, rig["w"], True, poses=poses, velocities=vel, imu_forward=fwd, imu_backward=bwd, lanes=args.lanes,
              start_span=max(nfr - need, 0))
fl.run(args.prime)
fl.set_sampling(1)
fl.run(10)
fl.timings()                  # (the first sampled steps carry the timers' set-up: discarded)
out = {"lib": args.lib or "tree", "select": os.environ.get("VSLAM_PROJ_SELECT", "default"), "lanes": args.lanes, "steps_per_rep": args.steps, "us_per_launch": []}
for _ in range(args.reps):
    rep = fl.run(args.steps)
    tm, cnt = fl.timings()
    steps = max(cnt["frames"] / args.lanes, 1)
    out["us_per_launch"].append({"proj_cells": round(1e3 * tm.get("proj_cells", 0.0) / steps, 1),
                                 "proj_candidates": round(1e3 * tm.get("proj_candidates", 0.0) / (2 * steps), 1),
                                 "proj_resolve": round(1e3 * tm.get("proj_resolve", 0.0) / (2 * steps), 1), "sampled_steps": steps})
out["lost_frames"] = rep["lost_frames"]; out["min_inliers"] = rep["min_inliers"]
fl.set_sampling(0)
if args.hist:
    h = np.zeros((2, 66), np.uint64)
    vc._chk(vc.lib().vslam_debug_proj_hist(h.ctypes.data_as(ctypes.c_void_p)))
    jobs = int(h[0].sum())
    cum = lambda a, n: round(float(a[:n + 1].sum()) / max(jobs, 1), 4)
    out["hist"] = {"jobs": jobs, "visited": [int(v) for v in h[0]], "tested": [int(v) for v in h[1]],
                   "visited_le": {str(n): cum(h[0], n) for n in (0, 1, 2, 4, 8, 16, 32, 64)},
                   "tested_le": {str(n): cum(h[1], n) for n in (0, 1, 2, 4, 8, 16, 32, 64)},
                   "mean_visited_le64": round(float((h[0][:65] * np.arange(65)).sum()) / max(float(h[0][:65].sum()), 1), 2),
                   "mean_tested_le64": round(float((h[1][:65] * np.arange(65)).sum()) / max(float(h[1][:65].sum()), 1), 2)}
print(json.dumps(out), flush=True)
fl.close()
