"""A cohort of tracker-window local BAs alone on the GPU (vslam_local_ba_batch): wall time per cohort and device time per stage.
usage: bacohort.py [--max-views V] [lanes ...]
--max-views V: cap of views per landmark of the synthetic windows (default 12: 13.3 factors, 8.4 slots per landmark; 4 and 5 bracket
the headline run's local BAs at about 5 factors and 3 slots per landmark)"""
import sys, os, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gtsam-vslam_amd"))
import numpy as np, synth, vslam_capi as vc
rig = synth.RIGS["euroc"]
fe = vc.Extractor(752, 480, 1500)
args = sys.argv[1:]
max_views = 12
if "--max-views" in args:
    k = args.index("--max-views")
    max_views = int(args[k + 1])
    del args[k:k + 2]
sizes = [int(v) for v in args] or [1, 10, 20, 40]
allp = [synth.make_ba_problem(n_local=10, n_fixed=4, n_lm=1000 + 15 * (s % 11), seed=100 + s, max_views=max_views) for s in range(max(sizes))]
for n in sizes:
    probs = allp[:n]
    vc.local_ba_set_timing(False)
    for it in range(2):
        r = vc.local_ba_batch(rig, fe.sigmaFactor, fe.InvSigmaFactor, probs)
    t = time.perf_counter()
    for it in range(5):
        r = vc.local_ba_batch(rig, fe.sigmaFactor, fe.InvSigmaFactor, probs)
    wall = (time.perf_counter() - t) / 5
    vc.local_ba_set_timing(True)
    r = vc.local_ba_batch(rig, fe.sigmaFactor, fe.InvSigmaFactor, probs)
    tm = vc.local_ba_timings()
    rounds = [q["rounds"] for q in r]
    it = [q["reports"][0]["iterations"] + q["reports"][1]["iterations"] for q in r]
    print("%3d lanes: wall %.2f ms (incl. the ctypes marshalling of the problems) | device %.2f ms | residual blocks %d, landmarks %d | rounds per lane %.1f (max %d), "
          "iterations %.1f | stages ms: %s" % (n, 1e3 * wall, sum(v for k, v in tm.items() if not k.endswith("#n")), r[0]["residuals"], r[0]["landmarks"], np.mean(rounds), max(rounds), np.mean(it),
                                               {k: round(v, 3) for k, v in tm.items()}))
