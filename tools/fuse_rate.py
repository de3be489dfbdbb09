"""Time of vslam_fuse_search at nA = 1 000, nB = 65 536: what the all-against-all gate scan costs, and what the wave-uniform skip of
k_fuse_match_b is worth.

Input: both sets seen from one random rigid pose over a 752 x 480 image at depths 2 .. 10 m, random descriptors, 300 B points placed
on an A point with its descriptor under 0 .. 20 flipped bits.  Sixteen lanes are sixteen such inputs with different seeds, each with
nB = 64 536: sixteen lanes of 1 000 + 65 536 points would pass the call's limit of 1 048 576 points over all lanes, which sixteen
lanes of 65 536 points meet exactly.
One STEP is one process: `python tools/fuse_rate.py step LANES SKIP [out.json]` times LANES lanes with VSLAM_FUSE_SKIP=SKIP - three
warm-up calls, then 5 repetitions of 10 calls: the wall-clock time of a call (host clock; a call ends in a device synchronise),
median and range over the repetitions, and from 10 more calls with the library's HIP-event timing on the device time of each
kernel, median over the calls - and merges its figures into the JSON.  `python tools/fuse_rate.py ref [out.json]` times the numpy
restatement (tests/fuse_ref.py) once on the one-lane input, on one core, and checks the device's bytes against it when a device is
there.  A full measurement chains the steps, each under its own time limit:
  timeout 120 python tools/fuse_rate.py step 1 1 && timeout 120 python tools/fuse_rate.py step 1 0 && \
  timeout 120 python tools/fuse_rate.py step 16 1 && timeout 120 python tools/fuse_rate.py step 16 0 && timeout 300 python tools/fuse_rate.py ref
Default output: profiles/fuse_rate.json."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("gtsam-vslam_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np

N_A, N_B, N_TWINS = 1000, 65536, 300
K = (458.654, 457.296, 367.215, 248.375)
SIZE = (752, 480)


def make_input(seed, N_B=N_B):
    rng = np.random.default_rng(seed)
    R = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    if np.linalg.det(R) < 0:
        R[:, 0] = -R[:, 0]
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = rng.normal(size=3)

    def cloud(n):
        u = rng.uniform(5, SIZE[0] - 5, n); v = rng.uniform(5, SIZE[1] - 5, n); z = rng.uniform(2, 10, n)
        Xc = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1)
        return (Xc - T[:3, 3]) @ R
    A = cloud(N_A); B = cloud(N_B)
    dA = rng.integers(0, 256, (N_A, 32), dtype=np.uint8); dB = rng.integers(0, 256, (N_B, 32), dtype=np.uint8)
    a_idx = rng.choice(N_A, N_TWINS, replace=False); b_idx = rng.choice(N_B, N_TWINS, replace=False)
    for k, (a, b) in enumerate(zip(a_idx, b_idx)):
        B[b] = A[a]
        d = dA[a].copy()
        for bit in rng.choice(256, k % 21, replace=False):
            d[bit >> 3] ^= np.uint8(1 << (bit & 7))
        dB[b] = d
    return T, K, SIZE, A, dA, B, dB


def load(path):
    if os.path.exists(path):
        with open(path) as f:
            return json.load(f)
    return dict(shape=dict(n_a=N_A, n_b=N_B, twins=N_TWINS), steps={})


def save(path, res):
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


def step(lanes, skip, path):
    os.environ["VSLAM_FUSE_SKIP"] = str(skip)
    import vslam_capi as vc
    n_b = N_B if lanes == 1 else min(N_B, 1048576 // lanes - N_A)
    ins = [make_input(100 + g, n_b) for g in range(lanes)]
    call = (lambda: vc.fuse_search(*ins[0])) if lanes == 1 else (lambda: vc.fuse_search_batch(ins))
    for _ in range(3):
        out = call()
    per = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(10):
            call()
        per.append((time.perf_counter() - t0) / 10 * 1e3)
    vc.fuse_set_timing(True)
    groups = {}
    for _ in range(10):
        call()
        for k, v in vc.fuse_timings().items():
            groups.setdefault(k, []).append(v)
    vc.fuse_set_timing(False)
    reps = [out[2]] if lanes == 1 else [o[2] for o in out]
    r = dict(lanes=lanes, skip=skip, n_a=N_A, n_b=n_b, ms_per_call=dict(median=float(np.median(per)), min=float(min(per)), max=float(max(per))),
             kernel_ms={k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in groups.items()},
             pairs_per_lane=[q["n_pairs"] for q in reps], proposals_per_lane=[q["n_proposals"] for q in reps])
    res = load(path)
    res["protocol"] = "3 warm-up calls; 5 repetitions of 10 calls (host clock, a call ends in a device synchronise); kernels: HIP events of 10 more calls"
    res["steps"]["lanes%d_skip%d" % (lanes, skip)] = r
    save(path, res)
    print(json.dumps(r), flush=True)


def ref(path):
    import fuse_ref as fr
    inp = make_input(100)
    t0 = time.perf_counter()
    want = fr.search(*inp)
    sec = time.perf_counter() - t0
    r = dict(seconds=sec, threads=os.environ.get("OMP_NUM_THREADS", "unset"), n_pairs=want[2]["n_pairs"])
    try:
        import vslam_capi as vc
        if vc.device_count() > 0:
            got = vc.fuse_search(*inp)
            r["device_equals_restatement_bitwise"] = bool(got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2])
    except Exception as e:      # (no library or no device: the timing stands alone)
        r["device"] = repr(e)
    res = load(path)
    res["restatement_one_lane"] = r
    save(path, res)
    print(json.dumps(r), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "step":
        step(int(a[1]), int(a[2]), a[3] if len(a) > 3 else os.path.join(ROOT, "profiles", "fuse_rate.json"))
    elif a and a[0] == "ref":
        ref(a[1] if len(a) > 1 else os.path.join(ROOT, "profiles", "fuse_rate.json"))
    else:
        print(__doc__)
