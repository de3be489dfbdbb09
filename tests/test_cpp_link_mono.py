"""The mono + IMU mode linked from C++: tests/native/adapter_mono_link.cpp holds VSlamSystem::InitializeMonocular's construction
sequence (src/System.cpp:27-34) and TrackMonoIMU (:82-85) on the classes of include/vslam_adapter.hpp and is built by g++ against
libvslam_hip.so.  CPU: it compiles and links (shared wrapper and stand-alone program), every undefined vslam_* symbol resolved by
the library.  GPU: adapter_mono_run() over the first 10 calls of the mono sequence equals the ctypes path call by call."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "adapter_mono_link.cpp")
LIBDIR = os.path.join(ROOT, "gtsam-vslam_amd")


def _build(tmp, shared):
    out = os.path.join(str(tmp), "libadapter_mono_link.so" if shared else "adapter_mono_link")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-o", out,
           "-L", LIBDIR, "-lvslam_hip", "-Wl,-rpath," + LIBDIR]
    cmd += ["-shared", "-fPIC"] if shared else ["-DVSLAM_LINK_MAIN"]
    cmd += ["-lpthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return out


def test_mono_adapter_compiles_and_links_against_the_library(capi, tmp_path):
    for shared in (True, False):
        out = _build(tmp_path, shared)
        nm = subprocess.run(["nm", "-D", "--undefined-only", out], stdout=subprocess.PIPE, text=True).stdout
        used = {l.split()[-1] for l in nm.splitlines() if " vslam_" in l or l.strip().startswith("U vslam_")}
        assert {"vslam_system_create_mono", "vslam_system_track_mono_imu", "vslam_system_counts"} <= used, sorted(used)
        lib = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libvslam_hip.so")], stdout=subprocess.PIPE, text=True).stdout
        defined = {l.split()[-1] for l in lib.splitlines()}
        assert used <= defined, sorted(used - defined)
        ldd = subprocess.run(["ldd", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
        assert "libvslam_hip.so" in ldd and "not found" not in ldd.split("libvslam_hip.so")[1].splitlines()[0], ldd


@pytest.mark.gpu
def test_mono_adapter_run_matches_ctypes_path(capi, tmp_path):
    import synth
    import mono_loop_ref as ml
    so = _build(tmp_path, True)
    L = C.CDLL(so)
    rig = synth.RIGS["euroc"]
    w, h = rig["w"], rig["h"]
    n = 10
    frames = np.stack([synth.mono_frame(f)[0] for f in synth.MONO_CALLS[:n]]).astype(np.uint8)
    buckets = [synth.mono_bucket(k) for k in range(n)]
    start = np.concatenate([[0], np.cumsum([len(b[1]) for b in buckets])]).astype(np.int32)
    acc = np.ascontiguousarray(np.concatenate([b[0][:, :3] for b in buckets])); gyr = np.ascontiguousarray(np.concatenate([b[0][:, 3:] for b in buckets]))
    ts = np.ascontiguousarray(np.concatenate([b[2] for b in buckets]), np.float64)
    T0 = np.ascontiguousarray(synth.mono_arc_pose(0))
    numb = np.array(synth.MONO_CALLS[:n], np.int32)
    g = np.array(ml.G); noise = np.array(ml.NOISE); Tbs = np.ascontiguousarray(synth.T_BC1)
    out = np.zeros((n, 20))
    crig = capi.make_rig(rig)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L.adapter_mono_run.restype = C.c_int
    kf = L.adapter_mono_run(p(frames), n, w, h, C.byref(crig), C.c_double(synth.MONO_FPS), p(T0), p(g), p(noise), p(Tbs), 200, p(numb),
                            p(start), p(acc), p(gyr), p(ts), p(out))
    assert kf >= 4, kf
    # the ctypes path with the extractor parameters of the reference's default FeatureExtractor() (2000 features)
    ms = capi.MonoSystem(rig, 2000, synth.MONO_FPS, T0=T0, imu=dict(gravity=ml.G, noise=ml.NOISE, T_bs=synth.T_BC1, hz=200))
    states = []
    for k in range(n):
        S, _, t = buckets[k]
        T, rep = ms.track(frames[k], synth.MONO_CALLS[k], (S[:, :3], S[:, 3:], t))
        assert np.abs(T.reshape(16) - out[k, :16]).max() <= 1e-9, k
        assert (rep["state"], rep["n_inliers"], rep["n_map_points"], rep["keyframe_inserted"]) == tuple(int(v) for v in out[k, 16:20]), k
        states.append(rep["state"])
    assert ms.counts()["keyframes"] == kf and states[:6] == [0, 1, 1, 0, 1, 2] and set(states[6:]) == {3}
    ms.close()
