"""The host bookkeeping of vslam_system_fuse_loop (gtsam-vslam_amd/csrc/fuse_host.hpp), built without a device as a stand-alone
program under AddressSanitizer + UBSan (tests/native/fuse_host_asan.cpp) and compared with the restatement's commit
(tests/fuse_ref.py) on the map of tests/fuse_cases.py and on random maps."""
import os
import subprocess
import tempfile
import numpy as np
import pytest
import fuse_cases as fc
import fuse_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program():
    src = os.path.join(ROOT, "tests", "native", "fuse_host_asan.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "fuse_host_asan")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(ROOT, "gtsam-vslam_amd", "csrc"), src, "-o", exe], check=True)
        yield exe


def run_native(exe, pairs, obs, kdx, outlier, in_frame, active, last_obs, n_kf, n_left, n_right):
    words = [len(obs), n_kf, n_left, n_right]
    for m, lst in enumerate(obs):
        words += [kdx[m], last_obs[m], outlier[m], in_frame[m], len(lst)] + [x for o in lst for x in o]
    words += [len(active)] + list(active) + [len(pairs)] + [x for p in pairs for x in p]
    with tempfile.NamedTemporaryFile("w", suffix=".txt") as f:
        f.write(" ".join(str(int(w)) for w in words))
        f.flush()
        r = subprocess.run([exe, f.name], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok"), r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    out = dict(obs=[], last=[], outlier=[], in_frame=[], tables=[])
    for line in r.stdout.splitlines()[1:]:
        name, *v = line.split()
        v = [int(x) for x in v]
        if name == "point":
            out["last"].append(v[1]); out["outlier"].append(v[2]); out["in_frame"].append(v[3])
            out["obs"].append([tuple(v[4 + 3 * q: 7 + 3 * q]) for q in range((len(v) - 4) // 3)])
        elif name == "lmpL":
            out["tables"].append(dict(lmpL=v))
        elif name in ("lmpR", "unF", "unFR"):
            out["tables"][-1][name] = v
        else:
            out[name] = v
    return out


def compare(exe, pairs, obs, kdx, outlier, in_frame, active, last_obs, n_kf, n_left, n_right):
    tables = fc.commit_tables(obs, kdx, n_kf)
    got = run_native(exe, pairs, obs, kdx, outlier, in_frame, active, last_obs, n_kf, n_left, n_right)
    w_obs, w_t, w_outl, w_inf, w_act, w_last, w_counts = fr.commit(pairs, obs, tables, kdx, outlier, in_frame, active, last_obs)
    assert got["obs"] == w_obs
    assert got["tables"] == w_t
    assert got["outlier"] == w_outl and got["in_frame"] == w_inf and got["last"] == w_last
    assert got["active"] == w_act
    assert got["touched"] == w_counts["touched"] and got["refresh"] == w_counts["refresh"]
    assert got["counts"] == [w_counts["n_fused"], w_counts["n_obs_moved"], w_counts["n_obs_dropped"]]
    return got


def test_commit_case_through_the_header(program):
    got = compare(program, fc.COMMIT_PAIRS, fc.COMMIT_OBS, fc.COMMIT_KDX, fc.COMMIT_OUTLIER, fc.COMMIT_IN_FRAME, fc.COMMIT_ACTIVE,
                  fc.COMMIT_LAST_OBS, 3, fc.N_LEFT, fc.N_RIGHT)
    assert got["active"] == [1, 2, 5, 0] and got["counts"] == [2, 2, 2] and got["touched"] == [1, 2]      # (the hand-worked answer)
    got = compare(program, [], fc.COMMIT_OBS, fc.COMMIT_KDX, fc.COMMIT_OUTLIER, fc.COMMIT_IN_FRAME, fc.COMMIT_ACTIVE,
                  fc.COMMIT_LAST_OBS, 3, fc.N_LEFT, fc.N_RIGHT)
    assert got["active"] == fc.COMMIT_ACTIVE and got["counts"] == [0, 0, 0]


def test_random_maps_through_the_header(program):
    """random small maps with the tables' geometry of the hand-worked case: every key slot of a keyframe belongs to at most one
    point, pairs join a late point to an early one"""
    rng = np.random.default_rng(11)
    for _ in range(20):
        n_kf, n_pts = 3, 8
        free_l = [list(rng.permutation(fc.N_LEFT)) for _ in range(n_kf)]
        free_r = [list(rng.permutation(fc.N_RIGHT)) for _ in range(n_kf)]
        obs, kdx = [], []
        for m in range(n_pts):
            lst = []
            for kf in range(n_kf):
                if rng.random() < 0.5:
                    l = int(free_l[kf].pop()) if free_l[kf] and rng.random() < 0.8 else -1
                    r = int(free_r[kf].pop()) if free_r[kf] and (l < 0 or rng.random() < 0.4) else -1
                    if l >= 0 or r >= 0:
                        lst.append((kf, l, r))
            obs.append(lst)
            kdx.append(0 if m < 4 else 2)
        olds = list(rng.permutation(4)); news = sorted(int(x) for x in rng.choice(np.arange(4, 8), int(rng.integers(0, 4)), replace=False))
        pairs = [(a, int(olds[i])) for i, a in enumerate(news)]
        active = [int(m) for m in rng.permutation(n_pts) if rng.random() < 0.6]
        in_frame = [int(m in active) for m in range(n_pts)]
        last = [max([o[0] for o in lst], default=-1) for lst in obs]
        compare(program, pairs, obs, kdx, [0] * n_pts, in_frame, active, last, n_kf, fc.N_LEFT, fc.N_RIGHT)
