"""Raw (unrectified) input: device time of the fused level-0 load (k_load_images_rect: rectification and gray conversion inside the
launch that fills pyramid level 0) against the two launches it replaces (k_remap_linear / k_remap_linear_gray<3> into scratch
images, then k_load_images), for the 512 images of 752x480 of one 256-lane vslam_batch step with the EuRoC cam0 / cam1
calibration; and frames/s of one 128-lane vslam_batch on the device-resident corridor sequence fed three ways, alternated in
one process, three repetitions each:
  (a) pre-rectified gray frames through track;
  (b) raw frames through the two-step path: Rectifier.remap_device into scratch images, then track(on_device=True);
  (c) raw frames through track(raw=True).
usage: python tools/raw_rate.py [steps]
The kernel times come from a child run of this script under `rocprofv3 --kernel-trace --stats` (argument --kernels); the
frames/s from wall-clock time of this process (no profiler attached).  Bytes per launch are computed from the shapes (source +
destination + the float maps, the maps counted once per image: what a launch asks of the memory system; the maps of a camera
are shared by its 256 images, so the HBM share is smaller - `GB_hbm_min`).  HBM peak for the fractions: 8.0 TB/s (MI355X spec)."""
import csv, glob, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gtsam-vslam_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import synth
import vslam_capi as vc
from color_rate import colourise

W, H = 752, 480
LOAD_LANES = 256
PEAK = 8.0e12
# EuRoC cam0 / cam1 (tests/test_gpu_rectify.py)
K0 = [[458.654, 0, 367.215], [0, 457.296, 248.375], [0, 0, 1]]; D0 = [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05]
K1 = [[457.587, 0, 379.999], [0, 456.134, 255.238], [0, 0, 1]]; D1 = [-0.28368365, 0.07451284, -0.00010473, -3.55590700e-05]
R0 = [[0.999966347530033, -0.001422739138722922, 0.008079580483432283], [0.001365741834644127, 0.9999741760894847, 0.007055629199258132],
      [-0.008089410156878961, -0.007044357138835809, 0.9999424675829176]]
R1 = [[0.9999633526194376, -0.003625811871560086, 0.007755443660172947], [0.003680398547259526, 0.9999684752771629, -0.007035845251224894],
      [-0.007729688520722713, 0.007064130529506649, 0.999945173484644]]
P = [[435.2046959714599, 0, 367.4517211914062], [0, 435.2046959714599, 252.2008514404297], [0, 0, 1]]


def kernels_child(steps):
    """the launches that the parent's profiler times: per channel count, `steps` fused steps, then `steps` two-step steps"""
    import torch
    dev = torch.device("cuda", 0)
    Ls, Rs, _, _ = synth.corridor_sequence("euroc", 8, dev, frame_step=2, first=0)
    rig = synth.RIGS["euroc"]
    B = LOAD_LANES
    # every lane has its own source images (frame b % 8 shifted by b columns), as the lanes of a real batch do: the sources
    # of a launch (185 MB gray, 554 MB BGR) do not fit the caches
    def per_lane(x):
        return torch.stack([torch.roll(x[b % 8], shifts=b, dims=1) for b in range(B)]).contiguous()
    imgs = {1: (per_lane(Ls), per_lane(Rs)), 3: (per_lane(colourise(Ls, 3, 1)), per_lane(colourise(Rs, 3, 2)))}
    scratch = torch.empty((2, B, H, W), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rl = vc.Rectifier(K0, D0, R0, P, (W, H), (W, H)); rr = vc.Rectifier(K1, D1, R1, P, (W, H), (W, H))
    bt = vc.Batch(rig, 1500, B, local_mapping=0)          # (extraction follows each load; local mapping off)
    bt.set_rectifiers(-1, rl, rr)
    sl = [scratch[0, b].data_ptr() for b in range(B)]; sr = [scratch[1, b].data_ptr() for b in range(B)]
    for cn in (1, 3):
        L, R = imgs[cn]
        lp = [L[b].data_ptr() for b in range(B)]; rp = [R[b].data_ptr() for b in range(B)]
        for s in range(steps):
            bt.track(lp, rp, [s] * B, on_device=True, stride=W * cn, channels=cn, raw=True)
        for s in range(steps):
            rl.remap_device(lp, W * cn, sl, W, channels=cn)
            rr.remap_device(rp, W * cn, sr, W, channels=cn)
            bt.track(sl, sr, [s] * B, on_device=True, stride=W)
    bt.close(); rl.close(); rr.close()


def kernel_table(steps):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "raw", "--",
               sys.executable, os.path.abspath(__file__), "--kernels", str(steps)]
        subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
        f = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)[0]
        rows = list(csv.DictReader(open(f)))
    px = W * H
    # (name in the trace, images per launch, source bytes per pixel, map bytes per pixel)
    want = [("k_load_images_rect<1>", 2 * LOAD_LANES, 1, 8, "fused gray"), ("k_load_images_rect<3>", 2 * LOAD_LANES, 3, 8, "fused BGR"),
            ("k_remap_linear(", LOAD_LANES, 1, 8, "remap gray"), ("k_remap_linear_gray<3>", LOAD_LANES, 3, 8, "remap BGR"),
            ("k_load_images(", 2 * LOAD_LANES, 1, 0, "load gray")]
    res = {}
    for key, nimg, cn, mp, tag in want:
        r = [x for x in rows if key in x["Name"]]
        if not r:
            continue
        us = float(r[0]["AverageNs"]) / 1e3
        nbytes = nimg * px * (cn + 1 + mp)
        cams = 2 if nimg > LOAD_LANES else 1
        hbm = nimg * px * (cn + 1) + (cams * px * mp if mp else 0)
        res[tag] = dict(images=nimg, us_per_launch=round(us, 1), calls=int(r[0]["Calls"]), GB=round(nbytes / 1e9, 3),
                        GB_per_s=round(nbytes / (us * 1e-6) / 1e9, 1), fraction_of_hbm_peak=round(nbytes / (us * 1e-6) / PEAK, 3),
                        GB_hbm_min=round(hbm / 1e9, 3), hbm_min_fraction_of_peak=round(hbm / (us * 1e-6) / PEAK, 3))
    # 512 images: the fused launch against two remap launches (one per camera, 256 images each) + the gray load
    if all(t in res for t in ("fused gray", "remap gray", "load gray")):
        res["two-step gray us (2 x remap + load)"] = round(2 * res["remap gray"]["us_per_launch"] + res["load gray"]["us_per_launch"], 1)
    if all(t in res for t in ("fused BGR", "remap BGR", "load gray")):
        res["two-step BGR us (2 x remap + load)"] = round(2 * res["remap BGR"]["us_per_launch"] + res["load gray"]["us_per_launch"], 1)
    return res


def batch_rate(steps, reps=3):
    import torch
    dev = torch.device("cuda", 0)
    rig = synth.RIGS["euroc"]
    B, nfr = 128, 40
    Ls, Rs, poses, _ = synth.corridor_sequence("euroc", nfr, dev, frame_step=2, first=0)
    # the corridor renders taken as raw frames of two mildly distorted cameras (K = P = the rig's intrinsics: the rectified
    # frames stay trackable; the cost of a tap does not depend on the calibration)
    K = [[rig["fx"], 0, rig["cx"]], [0, rig["fy"], rig["cy"]], [0, 0, 1]]
    rl = vc.Rectifier(K, [-0.02, 0.004, 0, 0], None, K, (W, H), (W, H)); rr = vc.Rectifier(K, [-0.021, 0.0045, 1e-4, -5e-5], None, K, (W, H), (W, H))
    rect = torch.empty((2, nfr, H, W), dtype=torch.uint8, device=dev)
    rl.remap_device([Ls[k].data_ptr() for k in range(nfr)], W, [rect[0, k].data_ptr() for k in range(nfr)], W)
    rr.remap_device([Rs[k].data_ptr() for k in range(nfr)], W, [rect[1, k].data_ptr() for k in range(nfr)], W)
    scratch = torch.empty((2, B, H, W), dtype=torch.uint8, device=dev)
    sl = [scratch[0, b].data_ptr() for b in range(B)]; sr = [scratch[1, b].data_ptr() for b in range(B)]
    torch.cuda.synchronize()
    runs = {"a_prerectified_gray": [], "b_two_step_raw": [], "c_fused_raw": []}
    for rep in range(reps):
        for mode in runs:
            bt = vc.Batch(rig, 1500, B, T0s=[poses[0]] * B, local_mapping=2, mapping_delay=2, mapping_np_delay=1)
            bt.set_rectifiers(-1, rl, rr)

            def step(k):
                if mode == "a_prerectified_gray":
                    bt.track([rect[0, k].data_ptr()] * B, [rect[1, k].data_ptr()] * B, [k] * B, on_device=True, stride=W)
                elif mode == "b_two_step_raw":
                    rl.remap_device([Ls[k].data_ptr()] * B, W, sl, W)
                    rr.remap_device([Rs[k].data_ptr()] * B, W, sr, W)
                    bt.track(sl, sr, [k] * B, on_device=True, stride=W)
                else:
                    bt.track([Ls[k].data_ptr()] * B, [Rs[k].data_ptr()] * B, [k] * B, on_device=True, stride=W, raw=True)

            for k in range(10):
                step(k)
            t0 = time.perf_counter()
            for k in range(10, 10 + steps):
                step(k)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            bt.wait_mapping()
            bt.close()
            runs[mode].append(round(B * steps / el, 1))
    rl.close(); rr.close()
    out = {m: dict(frames_per_s=v, median=float(np.median(v)), spread=round(max(v) - min(v), 1)) for m, v in runs.items()}
    b, c = out["b_two_step_raw"], out["c_fused_raw"]
    out["fused_not_slower_than_two_step"] = bool(c["median"] >= b["median"] - b["spread"])
    return out


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--kernels":
        kernels_child(int(sys.argv[2]))
        sys.exit(0)
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    res = dict(size=[W, H], hbm_peak_TBps=PEAK / 1e12, kernels=kernel_table(5))
    res["batch_128_lanes"] = batch_rate(min(steps, 29))
    print(json.dumps(res, indent=1))
