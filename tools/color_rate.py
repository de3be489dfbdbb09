"""Colour input: device time of the level-0 loads (512 images of 752x480 per launch: one 256-lane vslam_batch step, the largest
batch; the benchmark's 768 images per step are three launches of 256) and of the rectifier (768 images per launch), gray against
BGR / BGRA, and frames/s of one 128-lane vslam_batch on the device-resident corridor sequence fed gray,
then BGR.
usage: python tools/color_rate.py [steps]
The kernel times come from a child run of this script under `rocprofv3 --kernel-trace --stats` (argument --kernels); the
frames/s from wall-clock time of this process (no profiler attached).  HBM peak for the fraction: 8.0 TB/s (MI355X spec)."""
import csv, glob, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gtsam-vslam_amd"))
import numpy as np
import synth
import vslam_capi as vc

W, H, NIMG = 752, 480, 768
LOAD_LANES = 256
PEAK = 8.0e12


def colourise(g, cn, seed):
    """torch u8 gray images [n, h, w] on the device -> BGR / BGRA [n, h, w, cn] (the tests' rule: B = g + e, G = g + d,
    R = g - round((9617 d + 1868 e) / 4899), clipped; alpha random)"""
    import torch
    gen = torch.Generator(device=g.device).manual_seed(seed)
    gi = g.to(torch.int32)
    d = torch.randint(-30, 31, g.shape, generator=gen, device=g.device, dtype=torch.int32)
    e = torch.randint(-30, 31, g.shape, generator=gen, device=g.device, dtype=torch.int32)
    r = gi - torch.round((9617 * d + 1868 * e).to(torch.float64) / 4899).to(torch.int32)
    planes = [(gi + e).clamp(0, 255), (gi + d).clamp(0, 255), r.clamp(0, 255)]
    if cn == 4:
        planes.append(torch.randint(0, 256, g.shape, generator=gen, device=g.device, dtype=torch.int32))
    return torch.stack(planes, -1).to(torch.uint8).contiguous()


def kernels_child(steps):
    """the launches that the parent's profiler times"""
    import torch
    dev = torch.device("cuda", 0)
    Ls, Rs, _, _ = synth.corridor_sequence("euroc", 8, dev, frame_step=2, first=0)
    rig = synth.RIGS["euroc"]
    B = LOAD_LANES
    imgs = {1: (Ls, Rs), 3: (colourise(Ls, 3, 1), colourise(Rs, 3, 2)), 4: (colourise(Ls, 4, 3), colourise(Rs, 4, 4))}
    torch.cuda.synchronize()
    # level-0 loads: one launch for the 512 images of a 256-lane step (extraction follows; local mapping off)
    bt = vc.Batch(rig, 1500, B, local_mapping=0)
    for cn in (1, 3, 4):
        L, R = imgs[cn]
        for s in range(min(steps, 8)):
            lp = [L[s].data_ptr()] * B; rp = [R[s].data_ptr()] * B
            bt.track(lp, rp, [s] * B, on_device=True, stride=W * cn, channels=cn)
    bt.close()
    # rectifier: 768 images per launch, EuRoC cam0 calibration
    K0 = [[458.654, 0, 367.215], [0, 457.296, 248.375], [0, 0, 1]]; D0 = [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05]
    P = [[435.2046959714599, 0, 367.4517211914062], [0, 435.2046959714599, 252.2008514404297], [0, 0, 1]]
    r = vc.Rectifier(K0, D0, None, P, (W, H), (W, H))
    out = torch.empty((8, H, W), dtype=torch.uint8, device=dev)
    for cn in (1, 3):
        L = imgs[cn][0]
        for s in range(steps):
            r.remap_device([L[i % 8].data_ptr() for i in range(NIMG)], W * cn, [out[i % 8].data_ptr() for i in range(NIMG)], W, channels=cn)
    r.close()


def kernel_table(steps):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "color", "--",
               sys.executable, os.path.abspath(__file__), "--kernels", str(steps)]
        subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
        f = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)[0]
        rows = list(csv.DictReader(open(f)))
    want = [("k_load_images(", 1, "gray"), ("k_load_images_color<3>", 3, "BGR"), ("k_load_images_color<4>", 4, "BGRA"),
            ("k_remap_linear(", 1, "remap gray"), ("k_remap_linear_gray<3>", 3, "remap BGR")]
    res = {}
    for key, cn, tag in want:
        r = [x for x in rows if key in x["Name"]]
        if not r:
            continue
        us = float(r[0]["AverageNs"]) / 1e3
        px = W * H * (NIMG if "remap" in tag else 2 * LOAD_LANES)
        # algorithmic bytes: source (cn per pixel) + gray destination; the rectifier also reads its two float maps
        nbytes = px * (cn + 1 + (8 if "remap" in tag else 0))
        res[tag] = dict(images=px // (W * H), us_per_launch=round(us, 1), calls=int(r[0]["Calls"]), GB=round(nbytes / 1e9, 3),
                        GB_per_s=round(nbytes / (us * 1e-6) / 1e9, 1), fraction_of_hbm_peak=round(nbytes / (us * 1e-6) / PEAK, 3))
    return res


def batch_rate(steps):
    import torch
    dev = torch.device("cuda", 0)
    rig = synth.RIGS["euroc"]
    B, nfr = 128, 40
    Ls, Rs, poses, _ = synth.corridor_sequence("euroc", nfr, dev, frame_step=2, first=0)
    col = (colourise(Ls, 3, 5), colourise(Rs, 3, 6))
    torch.cuda.synchronize()
    out = {}
    for cn, (L, R) in ((1, (Ls, Rs)), (3, col)):
        bt = vc.Batch(rig, 1500, B, T0s=[poses[0]] * B, local_mapping=2, mapping_delay=2, mapping_np_delay=1)

        def step(k):
            lp = [L[k].data_ptr()] * B; rp = [R[k].data_ptr()] * B
            bt.track(lp, rp, [k] * B, on_device=True, stride=W * cn, channels=cn)

        for k in range(10):
            step(k)
        t0 = time.perf_counter()
        for k in range(10, 10 + steps):
            step(k)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        bt.wait_mapping()
        bt.close()
        out["gray" if cn == 1 else "BGR"] = dict(frames_per_s=round(B * steps / el, 1), ms_per_step=round(1e3 * el / steps, 3))
    return out


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--kernels":
        kernels_child(int(sys.argv[2]))
        sys.exit(0)
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    res = dict(size=[W, H], hbm_peak_TBps=PEAK / 1e12, kernels=kernel_table(5))
    res["batch_128_lanes"] = batch_rate(min(steps, 29))
    print(json.dumps(res, indent=1))
