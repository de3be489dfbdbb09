"""FAST candidate counts per pyramid level over the bench's corridor frames, and the k_ssc size class each level falls in.
usage: python tools/ssc_level_counts.py [frames]      (default 640: the default sequence of bench.py, both images of every pair)
Prints one JSON object: per level min / median / p90 / max of the counts and the share of the (image, level) tasks per class."""
import json, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'gtsam-vslam_amd'))
import numpy as np, torch, synth, vslam_capi as vc
nfr = int(sys.argv[1]) if len(sys.argv) > 1 else 640
hdr = open(os.path.join(ROOT, 'gtsam-vslam_amd', 'csrc', 'extract_kernels.hpp')).read()
lim = {k: int(re.search(r"constexpr int SSC_NMAX_%s = (\d+);" % k, hdr).group(1)) for k in ("TINY", "SMALL", "MID", "LDS")}
Ls, Rs, _, _ = synth.corridor_sequence("euroc", nfr, torch.device("cuda"), frame_step=1, speed=0.5, first=0)
fe = vc.Extractor(752, 480, 1500, batch=2)
numRet = [int(v) for v in fe.featurePerLevel]
cnt = np.zeros((nfr, 2, 8), np.int64)
for f in range(nfr):
    fe.extract([Ls[f].cpu().numpy(), Rs[f].cpu().numpy()])
    for i in range(2):
        for l in range(8):
            cnt[f, i, l] = len(fe.candidates(i, l))
out = {"frames": nfr, "limits": lim, "kept_per_level": numRet, "levels": [], "class_share_per_level": []}
for l in range(8):
    c = cnt[:, :, l].ravel()
    out["levels"].append({"level": l, "min": int(c.min()), "median": int(np.median(c)), "p90": int(np.percentile(c, 90)), "max": int(c.max())})
    sh = {"kept_whole": float((c <= numRet[l]).mean()), "tiny": float(((c > numRet[l]) & (c <= lim["TINY"])).mean()),
          "small": float(((c > max(numRet[l], lim["TINY"])) & (c <= lim["SMALL"])).mean()),
          "mid": float(((c > lim["SMALL"]) & (c <= lim["MID"])).mean()), "lds": float(((c > lim["MID"]) & (c <= lim["LDS"])).mean()),
          "hbm": float((c > lim["LDS"]).mean())}
    out["class_share_per_level"].append({k: round(v, 4) for k, v in sh.items()})
c0 = cnt[:, :, 0].ravel()
out["level0_above_small"] = int((c0 > lim["SMALL"]).sum())
out["level0_mid_share_of_those"] = round(float(((c0 > lim["SMALL"]) & (c0 <= lim["MID"])).sum()) / max(1, int((c0 > lim["SMALL"]).sum())), 4)
print(json.dumps(out))
