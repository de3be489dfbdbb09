"""ctypes binding of libvslam_hip.so (the C ABI declared in include/vslam_hip.h).

This is plumbing for tests/ and bench.py only: every call goes straight to the
HIP library.  There is no Python or CPU fallback; if the library or a GPU is
missing the calls raise.
"""
import ctypes as C
import os
import subprocess
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvslam_hip.so")
_LIB = None

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_CAPACITY, ERR_COMM = range(6)


class FeParams(C.Structure):
    _fields_ = [("n_features", C.c_int32), ("n_levels", C.c_int32), ("scale", C.c_float),
                ("edge_threshold", C.c_int32), ("patch_size", C.c_int32),
                ("max_fast_threshold", C.c_int32), ("min_fast_threshold", C.c_int32)]


class VslamError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("vslam status %d: %s" % (status, msg))
        self.status = status


def build():
    """Compile libvslam_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(_HERE, "csrc")])


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libvslam_hip.so is not built (run __graft_entry__.build()); "
                               "there is no CPU fallback")
        _LIB = C.CDLL(LIB_PATH)
        _LIB.vslam_last_error.restype = C.c_char_p
    return _LIB


def _chk(status):
    if status != OK:
        raise VslamError(status, lib().vslam_last_error().decode())


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _image(a, h, w):
    """a host image (h, w) gray, (h, w, 3) BGR or (h, w, 4) BGRA -> (contiguous u8 array, channels, row stride in bytes)"""
    a = np.ascontiguousarray(a, np.uint8)
    if a.ndim == 2:         # (gray: what the callers passed before colour input existed, unchecked here)
        return a, 1, a.shape[1]
    if a.ndim == 3 and a.shape[2] in (3, 4) and a.shape[:2] == (h, w):
        return a, a.shape[2], a.strides[0]
    raise ValueError("image of shape %s: expected (%d, %d), (%d, %d, 3) BGR or (%d, %d, 4) BGRA" % (a.shape, h, w, h, w, h, w))


def device_count():
    return int(lib().vslam_device_count())


class Extractor:
    """FeatureExtractor (reference include/FeatureExtractor.h:53-98) on the GPU."""

    def __init__(self, width, height, nfeatures=2000, nlevels=8, scale=1.2, edge=19, patch=31,
                 max_fast=20, min_fast=7, batch=1, device=0):
        self.L = lib()
        self.width, self.height, self.batch, self.nlevels = width, height, batch, nlevels
        prm = FeParams(nfeatures, nlevels, scale, edge, patch, max_fast, min_fast)
        self.h = C.c_void_p()
        _chk(self.L.vslam_extractor_create(C.byref(prm), width, height, batch, device, C.byref(self.h)))
        f = lambda: np.zeros(nlevels, np.float32)
        i = lambda: np.zeros(nlevels, np.int32)
        self.scalePyramid, self.scaleInvPyramid, self.sigmaFactor, self.InvSigmaFactor = f(), f(), f(), f()
        self.scaledPatchSize, self.featurePerLevel = i(), i()
        _chk(self.L.vslam_extractor_tables(self.h, _p(self.scalePyramid), _p(self.scaleInvPyramid),
                                           _p(self.sigmaFactor), _p(self.InvSigmaFactor),
                                           _p(self.scaledPatchSize), _p(self.featurePerLevel)))

    def close(self):
        if self.h:
            self.L.vslam_extractor_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_image(self, idx, image):
        """image: (H, W) gray, (H, W, 3) BGR or (H, W, 4) BGRA u8 (colour: converted to gray on the device)"""
        img, ch, st = _image(image, self.height, self.width)
        assert img.shape[:2] == (self.height, self.width)
        if ch == 1:
            _chk(self.L.vslam_extractor_set_image_host(self.h, idx, _p(img), st))
        else:
            _chk(self.L.vslam_extractor_set_image_color(self.h, idx, _p(img), st, ch, 0))

    def set_image_device(self, idx, dptr, stride, channels=1):
        if channels == 1:
            _chk(self.L.vslam_extractor_set_image_device(self.h, idx, C.c_void_p(dptr), stride))
        else:
            _chk(self.L.vslam_extractor_set_image_color(self.h, idx, C.c_void_p(dptr), int(stride), int(channels), 1))

    def set_image_raw(self, idx, rectifier, image, stride=None, channels=1, on_device=False):
        """an UNRECTIFIED image through `rectifier` (a Rectifier whose output size is this extractor's) into level 0: host u8
        array (sh, sw) gray, (sh, sw, 3) BGR or (sh, sw, 4) BGRA, or a device pointer with `channels` (stride default sw x cn)"""
        if on_device:
            sp, ch, st = C.c_void_p(image), channels, stride or rectifier.sw * channels
        else:
            img, ch, st = _image(image, rectifier.sh, rectifier.sw)
            assert img.shape[:2] == (rectifier.sh, rectifier.sw)
            sp = _p(img)
        _chk(self.L.vslam_extractor_set_image_raw(self.h, idx, rectifier.h_r, sp, int(st), int(ch), int(on_device)))

    def run(self):
        _chk(self.L.vslam_extractor_run(self.h))

    def fetch(self, idx, cap=None):
        n = C.c_int32()
        _chk(self.L.vslam_extractor_count(self.h, idx, C.byref(n)))
        cap = max(n.value, 1) if cap is None else cap
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        _chk(self.L.vslam_extractor_fetch(self.h, idx, _p(kps), _p(desc), cap, C.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    def extract(self, images):
        """images: list of `batch` u8 arrays -> list of (keypoints, descriptors)."""
        assert len(images) == self.batch
        for i, im in enumerate(images):
            self.set_image(i, im)
        self.run()
        return [self.fetch(i) for i in range(self.batch)]

    def level(self, idx, level, blurred=False):
        w, h = C.c_int32(), C.c_int32()
        _chk(self.L.vslam_extractor_level_size(self.h, level, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        _chk(self.L.vslam_extractor_level_copy(self.h, idx, level, int(blurred), _p(out)))
        return out

    def candidates(self, idx, level, cap=400000):
        out = np.zeros(cap, KP_DTYPE)
        n = C.c_int32()
        _chk(self.L.vslam_extractor_candidates(self.h, idx, level, _p(out), cap, C.byref(n)))
        return out[:n.value].copy()

    def ssc_level(self, level, cand):
        """FeatureExtractor::ssc of one pyramid level on caller-supplied candidates (test tap)."""
        cand = np.ascontiguousarray(cand, KP_DTYPE)
        out = np.zeros(max(len(cand), 1), KP_DTYPE)
        n = C.c_int32()
        _chk(self.L.vslam_extractor_ssc_level(self.h, level, _p(cand), len(cand), _p(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def describe(self, idx, level, kps):
        """k_orient_desc alone on caller-supplied keypoints of one level of image `idx` (level coordinates in x / y, response
        0..255), after a run() on the current images (test tap) -> (keypoints, descriptors)."""
        kps = np.ascontiguousarray(kps, KP_DTYPE)
        out = np.zeros(max(len(kps), 1), KP_DTYPE)
        desc = np.zeros((max(len(kps), 1), 32), np.uint8)
        n = C.c_int32()
        _chk(self.L.vslam_extractor_describe(self.h, idx, level, _p(kps), len(kps), _p(out), _p(desc), len(out), C.byref(n)))
        return out[:n.value].copy(), desc[:n.value].copy()

    def timings(self):
        names = (C.c_char_p * 32)()
        ms = (C.c_float * 32)()
        n = C.c_int32()
        _chk(self.L.vslam_extractor_timings(self.h, names, ms, 32, C.byref(n)))
        return {names[i].decode(): float(ms[i]) for i in range(n.value)}

    def set_timing(self, on):
        _chk(self.L.vslam_extractor_set_timing(self.h, int(bool(on))))

    def ssc_stats(self):
        on, fb = C.c_int32(), C.c_int32()
        _chk(self.L.vslam_extractor_ssc_stats(self.h, C.byref(on), C.byref(fb)))
        return on.value, fb.value


class Rig(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("baseline", C.c_float), ("width", C.c_int32), ("height", C.c_int32)]


def make_rig(r):
    return Rig(r["fx"], r["fy"], r["cx"], r["cy"], r["bl"], r["w"], r["h"])


class Matcher:
    """FeatureMatcher (reference include/FeatureMatcher.h:22-63) on the GPU."""

    def __init__(self, rig, fe_left, left_image, fe_right, right_image):
        self.L = lib()
        self.fe = (fe_left, fe_right)   # keep the extractors alive
        self.rig = make_rig(rig)
        self.h = C.c_void_p()
        # fe_right = None -> mono matcher (left-only operations of the mono + IMU mode)
        _chk(self.L.vslam_matcher_create(C.byref(self.rig), fe_left.h, left_image,
                                         fe_right.h if fe_right is not None else None, right_image, C.byref(self.h)))

    def close(self):
        if self.h:
            self.L.vslam_matcher_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_keys(self, right, kps, desc):
        kps = np.ascontiguousarray(kps, KP_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        assert desc.shape == (len(kps), 32)
        _chk(self.L.vslam_matcher_set_keys(self.h, int(right), _p(kps), _p(desc), len(kps)))

    def use_extractor_keys(self):
        _chk(self.L.vslam_matcher_use_extractor_keys(self.h))

    def stereo_match(self):
        _chk(self.L.vslam_stereo_match(self.h))

    def stereo_finalize_arrays(self, best, depth, sad, nR, nL=None):
        """The finalize kernel alone on per-left (accepted right index or -1, depth, SAD) arrays (test tap);
        read the result with stereo_fetch(len(best), nR).  nL overrides the count passed down (error-path tests)."""
        best = np.ascontiguousarray(best, np.int32); depth = np.ascontiguousarray(depth, np.float32)
        sad = np.ascontiguousarray(sad, np.int32)
        assert len(best) == len(depth) == len(sad)
        _chk(self.L.vslam_stereo_finalize_arrays(self.h, _p(best), _p(depth), _p(sad), len(best) if nL is None else int(nL), int(nR)))

    def stereo_fetch(self, nL, nR):
        ri = np.full(max(nL, 1), -1, np.int32); li = np.full(max(nR, 1), -1, np.int32)
        dp = np.full(max(nL, 1), -1, np.float32); cl = np.zeros(max(nL, 1), np.uint8)
        st = np.zeros(3, np.int64)
        _chk(self.L.vslam_stereo_fetch(self.h, _p(ri), _p(li), _p(dp), _p(cl), max(nL, 1), max(nR, 1), _p(st)))
        return dict(rightIdxs=ri[:nL], leftIdxs=li[:nR], depth=dp[:nL], close=cl[:nL],
                    candidates=int(st[0]), sad=int(st[1]), matches=int(st[2]))

    def timings(self):
        names = (C.c_char_p * 32)()
        ms = (C.c_float * 32)()
        n = C.c_int32()
        _chk(self.L.vslam_matcher_timings(self.h, names, ms, 32, C.byref(n)))
        return {names[i].decode(): float(ms[i]) for i in range(n.value)}

    def set_timing(self, on):
        _chk(self.L.vslam_matcher_set_timing(self.h, int(bool(on))))

    def bind_extractors(self, feL, iL, feR, iR):
        _chk(self.L.vslam_matcher_bind_extractors(self.h, feL.h, iL, feR.h, iR))
        self.fe = (feL, feR)      # keep them alive

    def relocalize(self, points, desc, pairs=True, **params):
        """vslam_relocalize on the matcher's current frame: (T_cw or None, report dict, pairs or None).  params: the
        fields of RelocParams (max_hamming, ratio_pct, n_hypotheses, seed, min_inliers, mode; 0 / absent = default)."""
        points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        assert len(desc) == len(points)
        n = len(points)
        prm = RelocParams(**{k: int(v) for k, v in params.items()})
        T = np.zeros((4, 4))
        rep = RelocReport()
        po = np.full(max(n, 1), -1, np.int32) if pairs else None
        _chk(self.L.vslam_relocalize(self.h, _p(points), _p(desc), n, C.byref(prm), _p(T), _p(po) if pairs else None, C.byref(rep)))
        d = _reloc_report_dict(rep)
        return (T if d["success"] else None), d, (po[:n] if pairs else None)

    def relocalize_debug(self):
        """(d1, i1, d2) per map point, winning map point per left key, count per hypothesis and the winner's inlier flag
        per correspondence of the last relocalize call (test tap)"""
        return _reloc_debug(lambda *a: self.L.vslam_relocalize_debug(self.h, *a))


MPV_DTYPE = np.dtype([("desc", "u1", 32), ("predLx", "<f4"), ("predLy", "<f4"), ("predRx", "<f4"),
                      ("predRy", "<f4"), ("scaleLevelL", "<i4"), ("scaleLevelR", "<i4"),
                      ("inFrame", "u1"), ("inFrameR", "u1"), ("_pad", "u1", 2)])
assert MPV_DTYPE.itemsize == 60


class LmReport(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("inner_iterations", C.c_int32), ("initial_error", C.c_double),
                ("final_error", C.c_double), ("lam", C.c_double)]


class RelocParams(C.Structure):
    _fields_ = [("max_hamming", C.c_int32), ("ratio_pct", C.c_int32), ("n_hypotheses", C.c_int32), ("seed", C.c_uint32),
                ("min_inliers", C.c_int32), ("mode", C.c_int32)]


class RelocReport(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("success", "n_points", "n_pairs", "best_hypothesis", "best_count", "n_inliers", "n_stereo")] + \
               [("lm", LmReport)]


def _reloc_report_dict(rep):
    d = {f[0]: getattr(rep, f[0]) for f in RelocReport._fields_ if f[0] != "lm"}
    d["lm"] = dict(iterations=rep.lm.iterations, inner=rep.lm.inner_iterations, initialError=rep.lm.initial_error,
                   finalError=rep.lm.final_error, lam=rep.lm.lam)
    return d


class RelocImuReport(C.Structure):
    _fields_ = [("phase", C.c_int32), ("dt", C.c_double), ("velocity_prev", C.c_double * 3), ("velocity", C.c_double * 3),
                ("bias", C.c_double * 6), ("rot_residual", C.c_double)]


def _reloc_imu_report_dict(rep):
    return dict(phase=rep.phase, dt=rep.dt, velocity_prev=np.array(list(rep.velocity_prev)), velocity=np.array(list(rep.velocity)),
                bias=np.array(list(rep.bias)), rot_residual=rep.rot_residual)


def _reloc_debug(call):
    """the arrays of a relocalize_debug tap; call(d3, cap, kw, cap, hc, cap, fl, cap, sizes4) is the bound C function"""
    sz = np.zeros(4, np.int32)
    _chk(call(None, 0, None, 0, None, 0, None, 0, _p(sz)))
    n, nL, H, Cn = (int(v) for v in sz)
    d3 = np.zeros((max(n, 1), 3), np.int32); kw = np.zeros(max(nL, 1), np.int32)
    hc = np.zeros(max(H, 1), np.int32); fl = np.zeros(max(Cn, 1), np.uint8)
    _chk(call(_p(d3), n, _p(kw), nL, _p(hc), H, _p(fl), Cn, _p(sz)))
    return dict(d=d3[:n], key_winner=kw[:nL], counts=hc[:H], flags=fl[:Cn])


class PgoEdge(C.Structure):
    _fields_ = [("i", C.c_int32), ("j", C.c_int32), ("Z", C.c_double * 16), ("w_rot", C.c_double), ("w_trans", C.c_double)]


PGO_EDGE_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("Z", "<f8", 16), ("w_rot", "<f8"), ("w_trans", "<f8")])
assert PGO_EDGE_DTYPE.itemsize == C.sizeof(PgoEdge) == 152


class PgoParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("lambda0", C.c_double)]


class PgoReport(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("iterations", "accepted", "rejected", "n_free", "n_isolated", "half_bandwidth")] + \
               [(n, C.c_double) for n in ("initial_cost", "final_cost", "final_lambda")]


def _pgo_report_dict(rep):
    return {f[0]: getattr(rep, f[0]) for f in PgoReport._fields_}


def pgo_edges(edges):
    """[(i, j, Z (4, 4), w_rot, w_trans), ...] -> the vslam_pgo_edge array"""
    a = np.zeros(max(len(edges), 1), PGO_EDGE_DTYPE)
    for k, (i, j, Z, wr, wt) in enumerate(edges):
        a[k] = (i, j, np.asarray(Z, np.float64).reshape(16), wr, wt)
    return a


def pose_graph_optimize(poses, fixed, edges, max_iterations=0, lambda0=0.0, device=0):
    """vslam_pose_graph_optimize: poses (n, 4, 4) world <- camera, fixed (n), edges as pgo_edges takes them (or its array).
    Returns (new poses, report dict)."""
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 4, 4)
    fixed = np.ascontiguousarray(fixed, np.uint8)
    assert len(fixed) == len(poses)
    m = len(edges)
    ea = edges if isinstance(edges, np.ndarray) else pgo_edges(edges)
    prm = PgoParams(int(max_iterations), float(lambda0))
    rep = PgoReport()
    out = np.zeros_like(poses)
    _chk(lib().vslam_pose_graph_optimize(_p(poses), _p(fixed), len(poses), _p(ea), m, C.byref(prm), int(device), _p(out), C.byref(rep)))
    return out, _pgo_report_dict(rep)


class PgoGraph(C.Structure):
    _fields_ = [("T_wc", C.c_void_p), ("fixed", C.c_void_p), ("n", C.c_int32), ("edges", C.c_void_p), ("m", C.c_int32),
                ("T_wc_out", C.c_void_p)]


def pose_graph_optimize_batch(graphs, max_iterations=0, lambda0=0.0, device=0):
    """vslam_pose_graph_optimize_batch: graphs = [(poses, fixed, edges) or None (an idle lane), ...], one parameter set for all.
    Returns [(new poses, report dict) or None, ...]."""
    B = len(graphs)
    tab = (PgoGraph * max(B, 1))()
    reps = (PgoReport * max(B, 1))()
    keep, outs = [], [None] * B
    for g, gr in enumerate(graphs):
        if gr is None:
            continue
        poses = np.ascontiguousarray(gr[0], np.float64).reshape(-1, 4, 4)
        fixed = np.ascontiguousarray(gr[1], np.uint8)
        assert len(fixed) == len(poses)
        ea = gr[2] if isinstance(gr[2], np.ndarray) else pgo_edges(gr[2])
        outs[g] = np.zeros_like(poses)
        keep.append((poses, fixed, ea))
        tab[g] = PgoGraph(poses.ctypes.data, fixed.ctypes.data, len(poses), ea.ctypes.data, len(gr[2]), outs[g].ctypes.data)
    prm = PgoParams(int(max_iterations), float(lambda0))
    _chk(lib().vslam_pose_graph_optimize_batch(tab, B, C.byref(prm), int(device), reps))
    return [None if outs[g] is None else (outs[g], _pgo_report_dict(reps[g])) for g in range(B)]


class PgoYawGraph(C.Structure):
    _fields_ = [("graph", PgoGraph), ("axis", C.c_double * 3)]


def pose_graph_optimize_yaw(poses, fixed, edges, axis, max_iterations=0, lambda0=0.0, device=0):
    """vslam_pose_graph_optimize_yaw: pose_graph_optimize with rotations confined to `axis` (3, any non-zero length) and world
    translations.  Returns (new poses, report dict)."""
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 4, 4)
    fixed = np.ascontiguousarray(fixed, np.uint8)
    assert len(fixed) == len(poses)
    m = len(edges)
    ea = edges if isinstance(edges, np.ndarray) else pgo_edges(edges)
    ax = np.ascontiguousarray(axis, np.float64).reshape(3)
    prm = PgoParams(int(max_iterations), float(lambda0))
    rep = PgoReport()
    out = np.zeros_like(poses)
    _chk(lib().vslam_pose_graph_optimize_yaw(_p(poses), _p(fixed), len(poses), _p(ea), m, _p(ax), C.byref(prm), int(device), _p(out), C.byref(rep)))
    return out, _pgo_report_dict(rep)


def pose_graph_optimize_yaw_batch(graphs, max_iterations=0, lambda0=0.0, device=0):
    """vslam_pose_graph_optimize_yaw_batch: graphs = [(poses, fixed, edges, axis) or None (an idle lane), ...], one parameter set
    for all.  Returns [(new poses, report dict) or None, ...]."""
    B = len(graphs)
    tab = (PgoYawGraph * max(B, 1))()
    reps = (PgoReport * max(B, 1))()
    keep, outs = [], [None] * B
    for g, gr in enumerate(graphs):
        if gr is None:
            continue
        poses = np.ascontiguousarray(gr[0], np.float64).reshape(-1, 4, 4)
        fixed = np.ascontiguousarray(gr[1], np.uint8)
        assert len(fixed) == len(poses)
        ea = gr[2] if isinstance(gr[2], np.ndarray) else pgo_edges(gr[2])
        ax = np.ascontiguousarray(gr[3], np.float64).reshape(3)
        outs[g] = np.zeros_like(poses)
        keep.append((poses, fixed, ea))
        tab[g].graph = PgoGraph(poses.ctypes.data, fixed.ctypes.data, len(poses), ea.ctypes.data, len(gr[2]), outs[g].ctypes.data)
        tab[g].axis[:] = [float(v) for v in ax]
    prm = PgoParams(int(max_iterations), float(lambda0))
    _chk(lib().vslam_pose_graph_optimize_yaw_batch(tab, B, C.byref(prm), int(device), reps))
    return [None if outs[g] is None else (outs[g], _pgo_report_dict(reps[g])) for g in range(B)]


def pose_graph_move_points(points, ref_index, T_old, T_new, device=0):
    """vslam_pose_graph_move_points: T_new[ref] * T_old[ref]^-1 * X per point (ref < 0: unchanged)"""
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    ref = np.ascontiguousarray(ref_index, np.int32)
    A = np.ascontiguousarray(T_old, np.float64).reshape(-1, 4, 4)
    B = np.ascontiguousarray(T_new, np.float64).reshape(-1, 4, 4)
    assert len(ref) == len(points) and len(A) == len(B)
    out = np.zeros((max(len(points), 1), 3))
    _chk(lib().vslam_pose_graph_move_points(_p(points), _p(ref), _p(A), _p(B), len(points), len(A), int(device), _p(out)))
    return out[:len(points)]


def pose_graph_set_timing(on):
    _chk(lib().vslam_pose_graph_set_timing(int(bool(on))))


def pose_graph_timings():
    """kernel group -> device ms of this thread's last pose_graph_optimize or pose_graph_optimize_batch (after
    pose_graph_set_timing(True)); the timers sit in the loop both calls share, so a batched call's figures cover all its lanes"""
    names = (C.c_char_p * 8)(); ms = (C.c_float * 8)(); n = C.c_int32()
    _chk(lib().vslam_pose_graph_timings(names, ms, 8, C.byref(n)))
    return {names[i].decode(): float(ms[i]) for i in range(n.value)}


def pose_graph_solve_count():
    """solves (single or batched, 6-DoF or yaw-only) that reached the device on this thread since pose_graph_set_timing"""
    n = C.c_int64()
    _chk(lib().vslam_pose_graph_solve_count(C.byref(n)))
    return n.value


class FuseParams(C.Structure):
    _fields_ = [("radius", C.c_float), ("depth_ratio", C.c_float), ("max_hamming", C.c_int32)]


class FuseReport(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_visible_a", "n_visible_b", "n_proposals", "n_pairs")]


class FuseLane(C.Structure):
    _fields_ = [("T_cw", C.c_void_p), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("w", C.c_int32), ("h", C.c_int32), ("a_xyz", C.c_void_p), ("a_desc", C.c_void_p), ("n_a", C.c_int32),
                ("b_xyz", C.c_void_p), ("b_desc", C.c_void_p), ("n_b", C.c_int32), ("match", C.c_void_p), ("best", C.c_void_p)]


class FuseLoopParams(C.Structure):
    _fields_ = [("search", FuseParams), ("min_kf_gap", C.c_int32)]


class FuseLoopReport(C.Structure):
    _fields_ = [("busy", C.c_int32), ("n_a", C.c_int32), ("n_b", C.c_int32), ("search", FuseReport)] + \
               [(n, C.c_int32) for n in ("n_fused", "n_obs_moved", "n_obs_dropped", "n_keyframes_touched", "n_active_after")]


def _fuse_report_dict(rep):
    return {f[0]: getattr(rep, f[0]) for f in FuseReport._fields_}


def _fuse_arrays(T_cw, xyz_a, desc_a, xyz_b, desc_b):
    T = np.ascontiguousarray(T_cw, np.float64).reshape(4, 4)
    xa = np.ascontiguousarray(xyz_a, np.float64).reshape(-1, 3); da = np.ascontiguousarray(desc_a, np.uint8).reshape(-1, 32)
    xb = np.ascontiguousarray(xyz_b, np.float64).reshape(-1, 3); db = np.ascontiguousarray(desc_b, np.uint8).reshape(-1, 32)
    assert len(xa) == len(da) and len(xb) == len(db)
    return T, xa, da, xb, db


def fuse_search(T_cw, K, size, xyz_a, desc_a, xyz_b, desc_b, radius=0.0, depth_ratio=0.0, max_hamming=0, device=0, fill=None):
    """vslam_fuse_search: T_cw (4, 4) camera <- world, K = (fx, fy, cx, cy), size = (w, h), the two sets.  Returns (match (nA),
    best (nA, 4), report dict).  fill: an int32 value the outputs and the report are pre-filled with (a refused or idle call
    leaves it there; default -1 / 0 / 0)."""
    T, xa, da, xb, db = _fuse_arrays(T_cw, xyz_a, desc_a, xyz_b, desc_b)
    nA = len(xa)
    match = np.full(max(nA, 1), -1 if fill is None else fill, np.int32)
    best = np.full((max(nA, 1), 4), 0 if fill is None else fill, np.int32)
    rep = FuseReport(*([0 if fill is None else fill] * 4))
    prm = FuseParams(float(radius), float(depth_ratio), int(max_hamming))
    _chk(lib().vslam_fuse_search(_p(T), C.c_double(K[0]), C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3]), int(size[0]), int(size[1]),
                                 _p(xa), _p(da), nA, _p(xb), _p(db), len(xb), C.byref(prm), int(device), _p(match), _p(best), C.byref(rep)))
    return match[:nA], best[:nA], _fuse_report_dict(rep)


def fuse_search_batch(lanes, radius=0.0, depth_ratio=0.0, max_hamming=0, device=0, fill=None):
    """vslam_fuse_search_batch: lanes = [(T_cw, K, size, xyz_a, desc_a, xyz_b, desc_b) or None (an idle lane), ...], one parameter
    set for all.  Returns [(match, best, report dict), ...]; an idle lane's arrays are empty and its report holds the fill."""
    B = len(lanes)
    tab = (FuseLane * max(B, 1))()
    reps = (FuseReport * max(B, 1))()
    f = 0 if fill is None else fill
    for g in range(B):
        reps[g] = FuseReport(f, f, f, f)
    keep, outs = [], []
    for g, ln in enumerate(lanes):
        if ln is None:
            outs.append((np.zeros(0, np.int32), np.zeros((0, 4), np.int32)))
            continue
        T, xa, da, xb, db = _fuse_arrays(ln[0], *ln[3:7])
        nA = len(xa)
        match = np.full(max(nA, 1), -1 if fill is None else fill, np.int32)
        best = np.full((max(nA, 1), 4), f, np.int32)
        keep.append((T, xa, da, xb, db))
        outs.append((match[:nA], best[:nA]))
        K, size = ln[1], ln[2]
        tab[g] = FuseLane(T.ctypes.data, K[0], K[1], K[2], K[3], int(size[0]), int(size[1]), xa.ctypes.data, da.ctypes.data, nA,
                          xb.ctypes.data, db.ctypes.data, len(xb), match.ctypes.data, best.ctypes.data)
    prm = FuseParams(float(radius), float(depth_ratio), int(max_hamming))
    _chk(lib().vslam_fuse_search_batch(tab, B, C.byref(prm), int(device), reps))
    return [(outs[g][0], outs[g][1], _fuse_report_dict(reps[g])) for g in range(B)]


def fuse_set_timing(on):
    _chk(lib().vslam_fuse_set_timing(int(bool(on))))


def fuse_timings():
    """stage -> device ms of this thread's last fuse_search / fuse_search_batch (after fuse_set_timing(True))"""
    names = (C.c_char_p * 4)(); ms = (C.c_float * 4)(); n = C.c_int32()
    _chk(lib().vslam_fuse_timings(names, ms, 4, C.byref(n)))
    return {names[i].decode(): float(ms[i]) for i in range(n.value)}


class LoopParams(C.Structure):
    _fields_ = [("reloc", RelocParams), ("pgo", PgoParams), ("min_kf_gap", C.c_int32), ("covis_min", C.c_int32),
                ("loop_weight", C.c_double), ("detect_only", C.c_int32)]


class LoopReport(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("busy", "success", "corrected", "kf_loop", "n_candidates", "n_nodes", "n_sequential",
                                         "n_covisibility", "n_edges", "points_moved", "n_active_after")] + \
               [("drift_translation", C.c_double), ("drift_rotation", C.c_double), ("T_wc_corrected", C.c_double * 16),
                ("T_wc", C.c_double * 16), ("reloc", RelocReport), ("pgo", PgoReport)]


def _loop_report_dict(rep):
    d = {f[0]: getattr(rep, f[0]) for f in LoopReport._fields_ if f[0] not in ("T_wc_corrected", "T_wc", "reloc", "pgo")}
    d["T_wc_corrected"] = np.array(list(rep.T_wc_corrected)).reshape(4, 4)
    d["T_wc"] = np.array(list(rep.T_wc)).reshape(4, 4)
    d["reloc"] = _reloc_report_dict(rep.reloc)
    d["pgo"] = _pgo_report_dict(rep.pgo)
    return d


class LoopImuReport(C.Structure):
    _fields_ = [("yaw", C.c_double), ("tilt_dropped", C.c_double), ("T_wc_projected", C.c_double * 16),
                ("velocity_before", C.c_double * 3), ("velocity", C.c_double * 3)]


def _loop_imu_report_dict(rep):
    return dict(yaw=rep.yaw, tilt_dropped=rep.tilt_dropped, T_wc_projected=np.array(list(rep.T_wc_projected)).reshape(4, 4),
                velocity_before=np.array(list(rep.velocity_before)), velocity=np.array(list(rep.velocity)))


def relocalize_batch(matchers, points, descs, T_out=None, **params):
    """vslam_relocalize_batch: matchers / points / descs per lane (a None matcher: the lane is idle).  Returns (T [lanes, 4, 4],
    reports, pairs): a lane's T row is written only on its success (T_out: the array to write into, e.g. pre-filled), its
    report and pairs are None for an idle lane."""
    B = len(matchers)
    L = lib()
    mh = (C.c_void_p * B)(); pp = (C.c_void_p * B)(); dp = (C.c_void_p * B)(); qp = (C.c_void_p * B)()
    n = np.zeros(B, np.int32)
    keep, pairs = [], [None] * B
    for b, m in enumerate(matchers):
        if m is None:
            continue
        x = np.ascontiguousarray(points[b], np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(descs[b], np.uint8).reshape(-1, 32)
        assert len(x) == len(d)
        pairs[b] = np.full(max(len(x), 1), -1, np.int32)
        keep += [x, d]
        mh[b], pp[b], dp[b], qp[b], n[b] = m.h.value, x.ctypes.data, d.ctypes.data, pairs[b].ctypes.data, len(x)
    prm = RelocParams(**{k: int(v) for k, v in params.items()})
    T = np.zeros((B, 4, 4)) if T_out is None else T_out
    assert T.dtype == np.float64 and T.shape == (B, 4, 4) and T.flags.c_contiguous
    reps = (RelocReport * B)()
    _chk(L.vslam_relocalize_batch(mh, B, pp, dp, _p(n), C.byref(prm), _p(T), qp, reps))
    return (T, [_reloc_report_dict(reps[b]) if matchers[b] is not None else None for b in range(B)],
            [pairs[b][:n[b]] if matchers[b] is not None else None for b in range(B)])


def match_projection(matcher, mps, rad, matchedL, matchedR, matches):
    """matchByProjectionRPred through the C ABI; returns (n, matchedL, matchedR, matches, ncand)."""
    mps = np.ascontiguousarray(mps, MPV_DTYPE)
    mL = np.array(matchedL, np.int32, copy=True)
    mR = np.array(matchedR, np.int32, copy=True)
    mt = np.array(matches, np.int32, copy=True).reshape(-1, 2)
    if len(mL) == 0:
        mL = np.full(1, -1, np.int32)
    if len(mR) == 0:
        mR = np.full(1, -1, np.int32)
    n = C.c_int32()
    nc = C.c_int64()
    _chk(matcher.L.vslam_match_projection(matcher.h, _p(mps), len(mps), C.c_float(rad), _p(mL), _p(mR), _p(mt),
                                          C.byref(n), C.byref(nc)))
    return n.value, mL[:len(matchedL)], mR[:len(matchedR)], mt, nc.value


class PoseProblem(C.Structure):
    _fields_ = [("n_mps", C.c_int32), ("points_xyz", C.c_void_p), ("in_frame", C.c_void_p),
                ("in_frame_r", C.c_void_p), ("mp_is_outlier", C.c_void_p), ("matches", C.c_void_p),
                ("mps_outliers", C.c_void_p), ("T_cw", C.c_double * 16)]


def estimate_pose(matcher, points, in_frame, in_frame_r, mp_is_outlier, matches, mps_outliers, T_cw):
    """estimatePoseGTSAM (stereo-only) + findOutliersR on the matcher's current frame."""
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    M = len(points)
    inF = np.ascontiguousarray(in_frame, np.uint8); inFR = np.ascontiguousarray(in_frame_r, np.uint8)
    mpo = np.ascontiguousarray(mp_is_outlier, np.uint8)
    mt = np.array(matches, np.int32, copy=True).reshape(-1, 2)
    out = np.array(mps_outliers, np.uint8, copy=True)
    prob = PoseProblem()
    prob.n_mps = M
    prob.points_xyz, prob.in_frame, prob.in_frame_r = _p(points), _p(inF), _p(inFR)
    prob.mp_is_outlier, prob.matches, prob.mps_outliers = _p(mpo), _p(mt), _p(out)
    T = np.ascontiguousarray(T_cw, np.float64).reshape(16)
    for i in range(16):
        prob.T_cw[i] = T[i]
    nIn, nSt = C.c_int32(), C.c_int32()
    rep = LmReport()
    _chk(matcher.L.vslam_estimate_pose(matcher.h, C.byref(prob), C.byref(nIn), C.byref(nSt), C.byref(rep)))
    Tout = np.array([prob.T_cw[i] for i in range(16)], np.float64).reshape(4, 4)
    return dict(T_cw=Tout, nIn=nIn.value, nStereo=nSt.value, matches=mt, outliers=out, iterations=rep.iterations,
                inner=rep.inner_iterations, initialError=rep.initial_error, finalError=rep.final_error, lam=rep.lam)


def world_to_frame(matcher, T_cw, points, max_scale_dist, log_scale):
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    n = len(points)
    msd = np.ascontiguousarray(max_scale_dist, np.float32)
    T = np.ascontiguousarray(T_cw, np.float64)
    pl = np.zeros((n, 2), np.float32); pr = np.zeros((n, 2), np.float32)
    ll = np.zeros(n, np.int32); lr = np.zeros(n, np.int32)
    vf = np.zeros(n, np.uint8); vr = np.zeros(n, np.uint8)
    _chk(matcher.L.vslam_world_to_frame(matcher.h, _p(T), n, _p(points), _p(msd), C.c_float(log_scale), _p(pl), _p(pr),
                                        _p(ll), _p(lr), _p(vf), _p(vr)))
    return pl, pr, ll, lr, vf, vr


class BaProblem(C.Structure):
    _fields_ = [("rig", Rig), ("n_levels", C.c_int32), ("sigma_factor", C.c_void_p), ("inv_sigma_factor", C.c_void_p),
                ("n_kf", C.c_int32), ("kf_pose_wc", C.c_void_p), ("kf_id", C.c_void_p), ("kf_fixed", C.c_void_p),
                ("kf_local", C.c_void_p), ("n_lm", C.c_int32), ("lm_xyz", C.c_void_p), ("n_pairs", C.c_int32),
                ("pair_kf", C.c_void_p), ("pair_lm", C.c_void_p), ("pair_flags", C.c_void_p), ("pair_uv", C.c_void_p),
                ("pair_octave", C.c_void_p)]


class BaResult(C.Structure):
    _fields_ = [("kf_pose_wc", C.c_void_p), ("lm_xyz", C.c_void_p), ("pair_wrong", C.c_void_p),
                ("pair_wrong_pass1", C.c_void_p), ("report", LmReport * 2), ("n_residuals", C.c_int64),
                ("n_landmarks", C.c_int64), ("n_free_kf", C.c_int64), ("sum_k2", C.c_int64), ("rounds", C.c_int64)]


def ba_problem_structs(rig, sigma_factor, inv_sigma_factor, prob):
    """(vslam_ba_problem, vslam_ba_result, keep) for a flattened problem dict; keep["read"]() turns the filled result into the
    dict local_ba returns (keep also holds the arrays the structs point into)."""
    kfPose = np.ascontiguousarray(prob["kf_pose"], np.float64).reshape(-1, 16)
    kfId = np.ascontiguousarray(prob["kf_id"], np.int64)
    kfFixed = np.ascontiguousarray(prob["kf_fixed"], np.uint8); kfLocal = np.ascontiguousarray(prob["kf_local"], np.uint8)
    lm = np.ascontiguousarray(prob["lm"], np.float64).reshape(-1, 3)
    pk = np.ascontiguousarray(prob["pair_kf"], np.int32); pl = np.ascontiguousarray(prob["pair_lm"], np.int32)
    pf = np.ascontiguousarray(prob["pair_flags"], np.uint8)
    puv = np.ascontiguousarray(prob["pair_uv"], np.float32).reshape(-1, 4)
    poct = np.ascontiguousarray(prob["pair_oct"], np.int32).reshape(-1, 2)
    sf = np.ascontiguousarray(sigma_factor, np.float32); isf = np.ascontiguousarray(inv_sigma_factor, np.float32)
    P = BaProblem()
    P.rig = make_rig(rig)
    P.n_levels = len(sf); P.sigma_factor = _p(sf); P.inv_sigma_factor = _p(isf)
    P.n_kf = len(kfPose); P.kf_pose_wc = _p(kfPose); P.kf_id = _p(kfId); P.kf_fixed = _p(kfFixed); P.kf_local = _p(kfLocal)
    P.n_lm = len(lm); P.lm_xyz = _p(lm) if len(lm) else None
    P.n_pairs = len(pk)
    if len(pk):
        P.pair_kf, P.pair_lm, P.pair_flags, P.pair_uv, P.pair_octave = _p(pk), _p(pl), _p(pf), _p(puv), _p(poct)
    kfOut = np.zeros_like(kfPose); lmOut = np.zeros((max(len(lm), 1), 3))
    wrong = np.zeros(max(len(pk), 1), np.uint8); wrong1 = np.zeros(max(len(pk), 1), np.uint8)
    R = BaResult()
    R.kf_pose_wc, R.lm_xyz, R.pair_wrong, R.pair_wrong_pass1 = _p(kfOut), _p(lmOut), _p(wrong), _p(wrong1)

    def read():
        reps = [dict(iterations=R.report[s].iterations, inner=R.report[s].inner_iterations,
                     initialError=R.report[s].initial_error, finalError=R.report[s].final_error, lam=R.report[s].lam)
                for s in range(2)]
        return dict(kf_pose=kfOut.reshape(-1, 4, 4), lm=lmOut[:len(lm)], pair_wrong=wrong[:len(pk)],
                    pair_wrong1=wrong1[:len(pk)], reports=reps, residuals=R.n_residuals, landmarks=R.n_landmarks,
                    free_kf=R.n_free_kf, sum_k2=R.sum_k2, rounds=R.rounds)
    keep = dict(arrays=[kfPose, kfId, kfFixed, kfLocal, lm, pk, pl, pf, puv, poct, sf, isf, kfOut, lmOut, wrong, wrong1], read=read)
    return P, R, keep


def local_ba(rig, sigma_factor, inv_sigma_factor, prob, device=0, comm=None):
    """LocalMapper::localBA numerical core through the C ABI."""
    P, R, keep = ba_problem_structs(rig, sigma_factor, inv_sigma_factor, prob)
    _chk(lib().vslam_local_ba(C.byref(P), C.byref(R), device, comm.h if comm is not None else None))
    return keep["read"]()


def local_ba_batch(rig, sigma_factor, inv_sigma_factor, probs, device=0):
    """vslam_local_ba_batch: the problems optimised together, one launch per stage for all of them (rig: one dict for all
    problems, or a list with one rig per problem - the lanes of a cohort may have different cameras)"""
    n = len(probs)
    rigs = list(rig) if isinstance(rig, (list, tuple)) else [rig] * n
    built = [ba_problem_structs(rigs[i], sigma_factor, inv_sigma_factor, pr) for i, pr in enumerate(probs)]
    PP = (C.POINTER(BaProblem) * n)(*[C.pointer(b[0]) for b in built])
    RR = (C.POINTER(BaResult) * n)(*[C.pointer(b[1]) for b in built])
    _chk(lib().vslam_local_ba_batch(PP, RR, n, int(device)))
    return [b[2]["read"]() for b in built]


class GbaParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("lambda0", C.c_double)]


class GbaReport(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("iterations", "accepted", "rejected", "n_free", "n_isolated", "n_present", "n_thin",
                                          "n_factors", "half_bandwidth", "reserved")] + \
               [(n, C.c_double) for n in ("initial_cost", "final_cost", "final_lambda")]


class GbaResult(C.Structure):
    _fields_ = [("kf_pose_wc", C.c_void_p), ("lm_xyz", C.c_void_p), ("pair_wrong", C.c_void_p), ("report", GbaReport)]


class SystemGbaParams(C.Structure):
    _fields_ = [("gba", GbaParams), ("edge_weight", C.c_double)]


class SystemGbaReport(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("busy", "success", "n_keyframes", "n_landmarks", "n_pairs", "n_edges", "n_wrong", "n_outliers",
                                          "n_active_after", "reserved")] + [("gba", GbaReport)]


class GbaImuReport(C.Structure):
    _fields_ = [("yaw", C.c_double), ("velocity_before", C.c_double * 3), ("velocity", C.c_double * 3), ("T_wc", C.c_double * 16)]


def _gba_report_dict(rep):
    return {f[0]: getattr(rep, f[0]) for f in GbaReport._fields_ if f[0] != "reserved"}


def _system_gba_report_dict(rep):
    d = {f[0]: getattr(rep, f[0]) for f in SystemGbaReport._fields_ if f[0] not in ("gba", "reserved")}
    d["gba"] = _gba_report_dict(rep.gba)
    return d


def _fuse_loop_report_dict(rep):
    d = {f[0]: getattr(rep, f[0]) for f in FuseLoopReport._fields_ if f[0] != "search"}
    d["search"] = _fuse_report_dict(rep.search)
    return d


def global_ba(rig, sigma_factor, inv_sigma_factor, prob, edges=None, max_iterations=0, lambda0=0.0, device=0):
    """vslam_global_ba on a flattened problem dict (the keys local_ba takes; kf_id may be missing: it is not used) with optional
    relative-pose edges as pgo_edges takes them (or its array).  Returns dict(kf_pose, lm, pair_wrong, report)."""
    return _global_ba(None, rig, sigma_factor, inv_sigma_factor, prob, edges, max_iterations, lambda0, device)


def global_ba_yaw(rig, sigma_factor, inv_sigma_factor, prob, axis, edges=None, max_iterations=0, lambda0=0.0, device=0):
    """vslam_global_ba_yaw: global_ba with keyframes that move only by a rotation about `axis` (3 floats, any non-zero length) and
    a translation"""
    return _global_ba(np.ascontiguousarray(axis, np.float64).reshape(3), rig, sigma_factor, inv_sigma_factor, prob, edges, max_iterations, lambda0, device)


def _global_ba(axis, rig, sigma_factor, inv_sigma_factor, prob, edges, max_iterations, lambda0, device):
    if "kf_id" not in prob:
        prob = dict(prob, kf_id=np.arange(len(prob["kf_pose"]), dtype=np.int64))
    P, _, keep = ba_problem_structs(rig, sigma_factor, inv_sigma_factor, prob)
    m = 0 if edges is None else len(edges)
    ea = None if m == 0 else (edges if isinstance(edges, np.ndarray) else pgo_edges(edges))
    n_kf, n_lm, n_pairs = P.n_kf, P.n_lm, P.n_pairs
    kfOut = np.zeros((max(n_kf, 1), 4, 4)); lmOut = np.zeros((max(n_lm, 1), 3)); wrong = np.zeros(max(n_pairs, 1), np.uint8)
    R = GbaResult()
    R.kf_pose_wc, R.lm_xyz, R.pair_wrong = _p(kfOut), _p(lmOut), _p(wrong)
    prm = GbaParams(int(max_iterations), float(lambda0))
    if axis is None:
        _chk(lib().vslam_global_ba(C.byref(P), None if ea is None else _p(ea), m, C.byref(prm), int(device), C.byref(R)))
    else:
        _chk(lib().vslam_global_ba_yaw(C.byref(P), None if ea is None else _p(ea), m, _p(axis), C.byref(prm), int(device), C.byref(R)))
    del keep
    return dict(kf_pose=kfOut[:n_kf], lm=lmOut[:n_lm], pair_wrong=wrong[:n_pairs], report=_gba_report_dict(R.report))


class GbaLane(C.Structure):
    _fields_ = [("problem", C.POINTER(BaProblem)), ("edges", C.c_void_p), ("n_edges", C.c_int32), ("result", C.POINTER(GbaResult))]


def global_ba_batch(lanes, max_iterations=0, lambda0=0.0, device=0):
    """vslam_global_ba_batch: lanes = [None (an idle lane) or dict(rig, sigma_factor, inv_sigma_factor, prob, edges=None,
    out=None, in_place=False), ...], one parameter set for all.  prob and edges are what global_ba takes.  out: dict(kf_pose
    (K, 4, 4) float64, lm (L, 3) float64, pair_wrong (P) uint8) of the caller's own C-contiguous arrays for the call to write into
    (default: fresh arrays); in_place: the result arrays are the problem's own (its kf_pose and lm must be C-contiguous float64
    arrays, which are then overwritten).  Returns [None or dict(kf_pose, lm, pair_wrong, report), ...]."""
    return _global_ba_batch(False, lanes, max_iterations, lambda0, device)


class GbaYawLane(C.Structure):
    _fields_ = [("lane", GbaLane), ("axis", C.c_double * 3)]


def global_ba_yaw_batch(lanes, max_iterations=0, lambda0=0.0, device=0):
    """vslam_global_ba_yaw_batch: the lanes of global_ba_batch, each with its own `axis` (3 floats, any non-zero length)"""
    return _global_ba_batch(True, lanes, max_iterations, lambda0, device)


def _global_ba_batch(yaw, lanes, max_iterations, lambda0, device):
    B = len(lanes)
    tab = ((GbaYawLane if yaw else GbaLane) * max(B, 1))()
    keep, outs = [], [None] * B
    for g, ln in enumerate(lanes):
        if ln is None:
            continue
        prob = ln["prob"]
        if "kf_id" not in prob:
            prob = dict(prob, kf_id=np.arange(len(prob["kf_pose"]), dtype=np.int64))
        P, _, kp = ba_problem_structs(ln["rig"], ln["sigma_factor"], ln["inv_sigma_factor"], prob)
        edges = ln.get("edges")
        m = 0 if edges is None else len(edges)
        ea = None if m == 0 else (edges if isinstance(edges, np.ndarray) else pgo_edges(edges))
        n_kf, n_lm, n_pairs = P.n_kf, P.n_lm, P.n_pairs
        if ln.get("in_place"):
            kfOut, lmOut = kp["arrays"][0], kp["arrays"][4]
            assert kfOut.ctypes.data == np.asarray(prob["kf_pose"]).ctypes.data and (n_lm == 0 or lmOut.ctypes.data == np.asarray(prob["lm"]).ctypes.data)
            kfOut = kfOut.reshape(-1, 4, 4)
            wrong = np.zeros(max(n_pairs, 1), np.uint8)
        elif ln.get("out") is not None:
            kfOut, lmOut, wrong = ln["out"]["kf_pose"], ln["out"]["lm"], ln["out"]["pair_wrong"]
            for a, dt, n in ((kfOut, np.float64, n_kf * 16), (lmOut, np.float64, n_lm * 3), (wrong, np.uint8, n_pairs)):
                assert a.dtype == dt and a.flags["C_CONTIGUOUS"] and a.size >= n
        else:
            kfOut = np.zeros((max(n_kf, 1), 4, 4)); lmOut = np.zeros((max(n_lm, 1), 3)); wrong = np.zeros(max(n_pairs, 1), np.uint8)
        R = GbaResult()
        R.kf_pose_wc, R.lm_xyz, R.pair_wrong = _p(kfOut), _p(lmOut), _p(wrong)
        keep.append((P, R, kp, ea))
        outs[g] = (R, kfOut[:n_kf], lmOut[:n_lm], wrong[:n_pairs])
        entry = GbaLane(C.pointer(P), None if ea is None else ea.ctypes.data, m, C.pointer(R))
        tab[g] = GbaYawLane(entry, (C.c_double * 3)(*[float(v) for v in ln["axis"]])) if yaw else entry
    prm = GbaParams(int(max_iterations), float(lambda0))
    _chk((lib().vslam_global_ba_yaw_batch if yaw else lib().vslam_global_ba_batch)(tab, B, C.byref(prm), int(device)))
    return [None if o is None else dict(kf_pose=o[1], lm=o[2], pair_wrong=o[3], report=_gba_report_dict(o[0].report)) for o in outs]


def global_ba_set_timing(on):
    _chk(lib().vslam_global_ba_set_timing(int(bool(on))))


def global_ba_timings():
    """kernel group -> device ms of this thread's last global_ba or global_ba_batch (after global_ba_set_timing(True)); a batched
    call's figures cover all its lanes"""
    names = (C.c_char_p * 8)(); ms = (C.c_float * 8)(); n = C.c_int32()
    _chk(lib().vslam_global_ba_timings(names, ms, 8, C.byref(n)))
    return {names[i].decode(): float(ms[i]) for i in range(n.value)}


class BaLaneShape(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("n_free_kf", "n_points", "n_factors", "n_edges", "n_pairs", "max_slots", "max_factors", "own_rig")]


class BaBatchShape(C.Structure):
    _fields_ = [("n_lanes", C.c_int32), ("lanes", C.POINTER(BaLaneShape)), ("lookahead", C.c_int32), ("solver", C.c_int32)]


class BaBatchPlan(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("status", "n_batch", "n_single", "lookahead", "f_max", "max_slots", "max_factors", "lp_max",
                                         "schur_kernel", "schur_waves", "schur_shared_w", "schur_blocks", "schur_lds",
                                         "back_kernel", "back_waves", "back_shared", "back_blocks", "back_lds", "solve_kinds", "solve_lds")]


BA_KERNELS = {0: None, 1: "schur", 2: "schur2", 3: "back", 4: "back2"}
BA_SOLVES = {1: "mfma64", 2: "wave", 4: "mfma"}


def _plan_dict(p):
    d = {f: int(getattr(p, f)) for f, _ in BaBatchPlan._fields_}
    d["schur_kernel"] = BA_KERNELS[d["schur_kernel"]]
    d["back_kernel"] = BA_KERNELS[d["back_kernel"]]
    d["solves"] = {name for bit, name in BA_SOLVES.items() if d["solve_kinds"] & bit}
    return d


def local_ba_batch_plan(lanes, lookahead=4, solver=0):
    """vslam_local_ba_batch_plan (pure host function, no GPU): lanes = list of dicts with the vslam_ba_lane_shape fields
    (missing ones 0); returns the plan as a dict (kernels by name, `solves` the set of solve kinds)."""
    arr = (BaLaneShape * max(len(lanes), 1))()
    for i, ln in enumerate(lanes):
        for k, v in ln.items():
            setattr(arr[i], k, int(v))
    S = BaBatchShape(len(lanes), arr, int(lookahead), int(solver))
    P = BaBatchPlan()
    _chk(lib().vslam_local_ba_batch_plan(C.byref(S), C.byref(P)))
    return _plan_dict(P)


def local_ba_last_batch_plan():
    """the plan of this thread's last local_ba_batch call"""
    P = BaBatchPlan()
    _chk(lib().vslam_local_ba_last_batch_plan(C.byref(P)))
    return _plan_dict(P)


def local_ba_timings():
    names = (C.c_char_p * 32)()
    ms = (C.c_float * 32)()
    n = C.c_int32()
    _chk(lib().vslam_local_ba_timings(names, ms, 32, C.byref(n)))
    return {names[i].decode(): float(ms[i]) for i in range(n.value)}


def ba_refresh_depth(rig, kf_pose_wc, lm_xyz, lm_outlier, pair_kf, pair_lm, pair_wrong, cur_depth, device=0):
    """MapPoint::updatePos depth / close refresh after localBA (vslam_ba_refresh_depth); returns (depth, close, updated)."""
    T = np.ascontiguousarray(kf_pose_wc, np.float64).reshape(-1, 16)
    lm = np.ascontiguousarray(lm_xyz, np.float64).reshape(-1, 3); lo = np.ascontiguousarray(lm_outlier, np.uint8)
    pk = np.ascontiguousarray(pair_kf, np.int32); pl = np.ascontiguousarray(pair_lm, np.int32)
    pw = np.ascontiguousarray(pair_wrong, np.uint8); cd = np.ascontiguousarray(cur_depth, np.float32)
    n = len(pk)
    d = np.zeros(max(n, 1), np.float32); c = np.zeros(max(n, 1), np.uint8); u = np.zeros(max(n, 1), np.uint8)
    r = make_rig(rig)
    _chk(lib().vslam_ba_refresh_depth(C.byref(r), len(T), _p(T), len(lm), _p(lm), _p(lo), n, _p(pk), _p(pl), _p(pw), _p(cd), int(device),
                                      _p(d), _p(c), _p(u)))
    return d[:n], c[:n], u[:n]


def ba_refresh_depth_merged(rigs, n_kfs, kf_pose_wc, lm_xyz, lm_outlier, pair_kf, pair_lm, pair_wrong, cur_depth, device=0):
    """the same for requests of different cameras staged together (vslam_ba_refresh_depth_merged, the lockstep group's form):
    request r has n_kfs[r] keyframe poses and the rig rigs[r]; poses, landmarks and pairs are the concatenations."""
    T = np.ascontiguousarray(kf_pose_wc, np.float64).reshape(-1, 16)
    lm = np.ascontiguousarray(lm_xyz, np.float64).reshape(-1, 3); lo = np.ascontiguousarray(lm_outlier, np.uint8)
    pk = np.ascontiguousarray(pair_kf, np.int32); pl = np.ascontiguousarray(pair_lm, np.int32)
    pw = np.ascontiguousarray(pair_wrong, np.uint8); cd = np.ascontiguousarray(cur_depth, np.float32)
    n = len(pk)
    d = np.zeros(max(n, 1), np.float32); c = np.zeros(max(n, 1), np.uint8); u = np.zeros(max(n, 1), np.uint8)
    rg = (Rig * len(rigs))(*[make_rig(r) for r in rigs])
    nk = np.ascontiguousarray(n_kfs, np.int32)
    assert len(nk) == len(rigs) and int(nk.sum()) == len(T)
    _chk(lib().vslam_ba_refresh_depth_merged(rg, _p(nk), len(rigs), _p(T), len(lm), _p(lm), _p(lo), n, _p(pk), _p(pl), _p(pw), _p(cd),
                                             int(device), _p(d), _p(c), _p(u)))
    return d[:n], c[:n], u[:n]


def local_ba_set_timing(on):
    _chk(lib().vslam_local_ba_set_timing(int(bool(on))))


def local_ba_set_solver(kind=-1):
    """reduced-camera solve of the calling thread's local BAs: -1 default, 0 MFMA forms, 1 wave / LDS forms"""
    _chk(lib().vslam_local_ba_set_solver(int(kind)))


def local_ba_set_lookahead(candidates=0, speculative_linearize=-1, mask_second_pass=1):
    """Scheduling knobs only: lambda candidates per trial round (1..4, 0 = default), speculative linearisation
    (0 / 1, -1 = default), second pass by masking instead of a host rebuild (0 / 1)."""
    _chk(lib().vslam_local_ba_set_lookahead(int(candidates), int(speculative_linearize), int(mask_second_pass)))


class TrackReport(C.Structure):
    _fields_ = [("n_map_points", C.c_int32), ("n_active", C.c_int32), ("rounds", C.c_int32),
                ("n_inliers", C.c_int32), ("n_stereo", C.c_int32), ("lm_iterations", C.c_int32),
                ("last_radius", C.c_float)]


def tracker_init_map(matcher, T_wc):
    T = np.ascontiguousarray(T_wc, np.float64)
    _chk(matcher.L.vslam_tracker_init_map(matcher.h, _p(T)))


def tracker_track(matcher, T_wc_pred, frame_number):
    T = np.ascontiguousarray(T_wc_pred, np.float64)
    out = np.zeros((4, 4), np.float64)
    rep = TrackReport()
    _chk(matcher.L.vslam_tracker_track(matcher.h, _p(T), int(frame_number), _p(out), C.byref(rep)))
    return out, {f[0]: getattr(rep, f[0]) for f in TrackReport._fields_}


def tracker_fetch(matcher, cap=65536):
    mt = np.zeros((cap, 2), np.int32); out = np.zeros(cap, np.uint8); act = np.zeros(cap, np.int32)
    n = C.c_int32()
    _chk(matcher.L.vslam_tracker_fetch(matcher.h, _p(mt), _p(out), _p(act), cap, C.byref(n)))
    return mt[:n.value].copy(), out[:n.value].copy(), act[:n.value].copy()


# ---- communicators for the landmark-sharded BA ----------------------------------------------
class Comm:
    def __init__(self, handle):
        self.h = handle

    def close(self):
        if self.h:
            lib().vslam_comm_destroy(self.h)
            self.h = None


def comm_create_local(world):
    """`world` in-process ranks (host threads sharing one GPU)."""
    arr = (C.c_void_p * world)()
    _chk(lib().vslam_comm_create_local(world, arr))
    return [Comm(C.c_void_p(arr[r])) for r in range(world)]


def comm_create_rccl(rank, world, device, broadcast_bytes):
    """RCCL communicator.  broadcast_bytes(buf: bytes|None) -> bytes must return rank 0's 128-byte id on
    every rank (e.g. via torch.distributed.broadcast_object_list)."""
    idbuf = (C.c_uint8 * 128)()
    if rank == 0:
        _chk(lib().vslam_comm_unique_id(idbuf))
    uid = broadcast_bytes(bytes(idbuf) if rank == 0 else None)
    assert len(uid) == 128
    idbuf = (C.c_uint8 * 128).from_buffer_copy(uid)
    h = C.c_void_p()
    _chk(lib().vslam_comm_create_rccl(idbuf, rank, world, device, C.byref(h)))
    return Comm(h)


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_size_t)


def comm_create_callback(rank, world, device, allreduce):
    """Communicator over a caller-supplied collective: allreduce(array) must sum the float64 numpy array IN PLACE over the ranks
    (e.g. torch.distributed.all_reduce on torch.from_numpy(array) with a gloo group).  The library stages the reduced camera
    systems through the host around it, so the ranks may be separate processes sharing one GPU."""
    def _cb(ctx, buf, n):
        try:
            allreduce(np.ctypeslib.as_array(buf, shape=(n,)))
            return 0
        except Exception:      # noqa: BLE001  (the status crosses the C boundary; the library reports VSLAM_ERR_COMM)
            return 1
    fn = ALLREDUCE_FN(_cb)
    h = C.c_void_p()
    _chk(lib().vslam_comm_create_callback(int(rank), int(world), int(device), fn, None, C.byref(h)))
    c = Comm(h)
    c._keep = fn      # the C side holds the function pointer for the communicator's lifetime
    return c


def landmark_owner(landmark_index, world):
    """Shard rule of the multi-GPU BA: landmark l belongs to rank l % world."""
    return landmark_index % world


class ImuInput(C.Structure):
    _fields_ = [("gravity", C.c_double * 3), ("gyro_noise_density", C.c_double), ("gyro_random_walk", C.c_double),
                ("accel_noise_density", C.c_double), ("accel_random_walk", C.c_double), ("T_body_sensor", C.c_double * 16),
                ("T_wc_prev", C.c_double * 16), ("velocity_prev", C.c_double * 3), ("bias_prev", C.c_double * 6),
                ("n_samples", C.c_int32), ("hz", C.c_int32), ("acceleration", C.c_void_p), ("angular_velocity", C.c_void_p),
                ("timestamps_ns", C.c_void_p)]


class ImuOutput(C.Structure):
    _fields_ = [("velocity", C.c_double * 3), ("bias", C.c_double * 6)]


def estimate_pose_imu(matcher, points, in_frame, in_frame_r, mp_is_outlier, matches, mps_outliers, gravity, noise,
                      T_body_sensor, T_wc_prev, vel_prev, bias_prev, acc, gyro, timestamps_ns, hz):
    """estimatePoseGTSAM IMU branch + findOutliersR on the matcher's current frame.
    noise = (gyro_density, gyro_walk, acc_density, acc_walk)."""
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    M = len(points)
    inF = np.ascontiguousarray(in_frame, np.uint8); inFR = np.ascontiguousarray(in_frame_r, np.uint8)
    mpo = np.ascontiguousarray(mp_is_outlier, np.uint8)
    mt = np.array(matches, np.int32, copy=True).reshape(-1, 2); out = np.array(mps_outliers, np.uint8, copy=True)
    prob = PoseProblem()
    prob.n_mps = M
    prob.points_xyz, prob.in_frame, prob.in_frame_r = _p(points), _p(inF), _p(inFR)
    prob.mp_is_outlier, prob.matches, prob.mps_outliers = _p(mpo), _p(mt), _p(out)
    acc = np.ascontiguousarray(acc, np.float64).reshape(-1, 3); gyro = np.ascontiguousarray(gyro, np.float64).reshape(-1, 3)
    ts = np.ascontiguousarray(timestamps_ns, np.float64)
    imu = ImuInput()
    for i in range(3):
        imu.gravity[i] = gravity[i]; imu.velocity_prev[i] = vel_prev[i]
    imu.gyro_noise_density, imu.gyro_random_walk, imu.accel_noise_density, imu.accel_random_walk = noise
    Tb = np.asarray(T_body_sensor, np.float64).reshape(16); Tp = np.asarray(T_wc_prev, np.float64).reshape(16)
    for i in range(16):
        imu.T_body_sensor[i] = Tb[i]; imu.T_wc_prev[i] = Tp[i]
    for i in range(6):
        imu.bias_prev[i] = bias_prev[i]
    imu.n_samples, imu.hz = len(ts), int(hz)
    imu.acceleration, imu.angular_velocity, imu.timestamps_ns = _p(acc), _p(gyro), _p(ts)
    o = ImuOutput()
    nIn, nSt = C.c_int32(), C.c_int32()
    rep = LmReport()
    _chk(matcher.L.vslam_estimate_pose_imu(matcher.h, C.byref(prob), C.byref(imu), C.byref(o), C.byref(nIn), C.byref(nSt), C.byref(rep)))
    Tout = np.array([prob.T_cw[i] for i in range(16)], np.float64).reshape(4, 4)
    return dict(T_cw=Tout, vel=np.array(list(o.velocity)), bias=np.array(list(o.bias)), nIn=nIn.value, nStereo=nSt.value,
                matches=mt, outliers=out, iterations=rep.iterations, inner=rep.inner_iterations,
                initialError=rep.initial_error, finalError=rep.final_error, lam=rep.lam)


def _imu_input(gravity, noise, T_body_sensor, T_wc_prev, vel_prev, bias_prev, acc, gyro, timestamps_ns, hz):
    acc = np.ascontiguousarray(acc, np.float64).reshape(-1, 3); gyro = np.ascontiguousarray(gyro, np.float64).reshape(-1, 3)
    ts = np.ascontiguousarray(timestamps_ns, np.float64)
    imu = ImuInput()
    for i in range(3):
        imu.gravity[i] = gravity[i]; imu.velocity_prev[i] = vel_prev[i]
    imu.gyro_noise_density, imu.gyro_random_walk, imu.accel_noise_density, imu.accel_random_walk = noise
    Tb = np.asarray(T_body_sensor, np.float64).reshape(16); Tp = np.asarray(T_wc_prev, np.float64).reshape(16)
    for i in range(16):
        imu.T_body_sensor[i] = Tb[i]; imu.T_wc_prev[i] = Tp[i]
    for i in range(6):
        imu.bias_prev[i] = bias_prev[i]
    imu.n_samples, imu.hz = len(ts), int(hz)
    imu.acceleration, imu.angular_velocity, imu.timestamps_ns = _p(acc), _p(gyro), _p(ts)
    imu._keep = (acc, gyro, ts)      # keep the arrays alive while the struct is in use
    return imu


def tracker_track_imu(matcher, T_wc_pred, frame_number, gravity, noise, T_body_sensor, T_wc_prev, vel_prev, bias_prev,
                      acc, gyro, timestamps_ns, hz):
    T = np.ascontiguousarray(T_wc_pred, np.float64)
    imu = _imu_input(gravity, noise, T_body_sensor, T_wc_prev, vel_prev, bias_prev, acc, gyro, timestamps_ns, hz)
    out = np.zeros((4, 4), np.float64)
    o = ImuOutput()
    rep = TrackReport()
    _chk(matcher.L.vslam_tracker_track_imu(matcher.h, _p(T), int(frame_number), C.byref(imu), _p(out), C.byref(o), C.byref(rep)))
    return out, {f[0]: getattr(rep, f[0]) for f in TrackReport._fields_}, np.array(list(o.velocity)), np.array(list(o.bias))


# ---- mono + IMU mode (C4) -------------------------------------------------------------------------
def match_projection_mono(matcher, mps, rad, matchedL, matches):
    """matchByProjectionMono; returns (n, matchedL, matches, ncand)."""
    mps = np.ascontiguousarray(mps, MPV_DTYPE)
    mL = np.array(matchedL, np.int32, copy=True)
    if len(mL) == 0:
        mL = np.full(1, -1, np.int32)
    mt = np.array(matches, np.int32, copy=True).reshape(-1, 2)
    n, nc = C.c_int32(), C.c_int64()
    _chk(matcher.L.vslam_match_projection_mono(matcher.h, _p(mps), len(mps), C.c_float(rad), _p(mL), _p(mt), C.byref(n), C.byref(nc)))
    return n.value, mL[:len(matchedL)], mt, nc.value


def match_by_radius(matcher, last_kps, last_desc, rad, matchedL):
    """matchByRadius; returns (n, matchedL, match_out)."""
    lk = np.ascontiguousarray(last_kps, KP_DTYPE); ld = np.ascontiguousarray(last_desc, np.uint8).reshape(-1, 32)
    mL = np.array(matchedL, np.int32, copy=True)
    out = np.full(max(len(lk), 1), -1, np.int32)
    n = C.c_int32()
    _chk(matcher.L.vslam_match_by_radius(matcher.h, _p(lk), _p(ld), len(lk), C.c_float(rad), _p(mL), _p(out), C.byref(n)))
    return n.value, mL, out[:len(lk)]


def estimate_pose_mono(matcher, points, in_frame, mp_is_outlier, matches, mps_outliers, gravity, noise, T_body_sensor,
                       T_wc_prev, vel_prev, bias_prev, acc, gyro, timestamps_ns, hz):
    """estimatePoseGTSAMMono + findOutliersMono on the matcher's current (left) keypoints."""
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    M = len(points)
    inF = np.ascontiguousarray(in_frame, np.uint8); mpo = np.ascontiguousarray(mp_is_outlier, np.uint8)
    mt = np.array(matches, np.int32, copy=True).reshape(-1, 2); out = np.array(mps_outliers, np.uint8, copy=True)
    prob = PoseProblem()
    prob.n_mps = M
    prob.points_xyz, prob.in_frame, prob.in_frame_r = _p(points), _p(inF), None
    prob.mp_is_outlier, prob.matches, prob.mps_outliers = _p(mpo), _p(mt), _p(out)
    imu = _imu_input(gravity, noise, T_body_sensor, T_wc_prev, vel_prev, bias_prev, acc, gyro, timestamps_ns, hz)
    o = ImuOutput()
    nIn = C.c_int32()
    rep = LmReport()
    _chk(matcher.L.vslam_estimate_pose_mono(matcher.h, C.byref(prob), C.byref(imu), C.byref(o), C.byref(nIn), C.byref(rep)))
    Tout = np.array([prob.T_cw[i] for i in range(16)], np.float64).reshape(4, 4)
    return dict(T_cw=Tout, vel=np.array(list(o.velocity)), bias=np.array(list(o.bias)), nIn=nIn.value, outliers=out,
                iterations=rep.iterations, inner=rep.inner_iterations, initialError=rep.initial_error,
                finalError=rep.final_error, lam=rep.lam)


def imu_predict(matcher, gravity, noise, T_body_sensor, T_wc_prev, pred_velocity, bias_prev, acc, gyro, timestamps_ns, hz, last_dt):
    """PredictNextPoseIMU; returns (T_wc_pred, velocity_pred)."""
    imu = _imu_input(gravity, noise, T_body_sensor, T_wc_prev, pred_velocity, bias_prev, acc, gyro, timestamps_ns, hz)
    pv = np.ascontiguousarray(pred_velocity, np.float64)
    T = np.zeros((4, 4)); v = np.zeros(3)
    _chk(matcher.L.vslam_imu_predict(matcher.h, C.byref(imu), _p(pv), C.c_double(last_dt), _p(T), _p(v)))
    return T, v


def imu_preintegrate(matcher, gravity, noise, T_body_sensor, T_wc_prev, vel_prev, bias_prev, acc, gyro, timestamps_ns, hz):
    """Test tap: the pose solve's pre-integration of one bucket; returns (pim[295], Lam (15, 15), pred[15])."""
    imu = _imu_input(gravity, noise, T_body_sensor, T_wc_prev, vel_prev, bias_prev, acc, gyro, timestamps_ns, hz)
    pim, lam, pred = np.zeros(295), np.zeros(225), np.zeros(15)
    _chk(matcher.L.vslam_imu_preintegrate(matcher.h, C.byref(imu), _p(pim), _p(lam), _p(pred)))
    return pim, lam.reshape(15, 15), pred


def imu_preintegrate_batch(matcher, buckets, solve_io=None, fill=np.nan):
    """Test tap: one batched pre-integration launch.  buckets: per lane the argument tuple of imu_preintegrate after
    `matcher` (an empty bucket = idle lane); solve_io: None or per lane None / 9 doubles (velocity, bias of a solve).
    The outputs start at `fill`; returns (pim (B, 295), Lam (B, 15, 15), pred (B, 15))."""
    B = len(buckets)
    imus = (ImuInput * B)()
    keep = []
    for b, args in enumerate(buckets):
        one = _imu_input(*args)
        keep.append(one)                        # (its arrays stay alive while the copy in imus[b] points at them)
        imus[b] = one
    io = None
    if solve_io is not None:
        arrs = [None if v is None else np.ascontiguousarray(v, np.float64) for v in solve_io]
        keep.append(arrs)
        io = (C.c_void_p * B)(*[None if a is None else a.ctypes.data for a in arrs])
    pim, lam, pred = np.full((B, 295), fill), np.full((B, 225), fill), np.full((B, 15), fill)
    _chk(matcher.L.vslam_imu_preintegrate_batch(matcher.h, B, imus, io, _p(pim), _p(lam), _p(pred)))
    return pim, lam.reshape(B, 15, 15), pred


def imu_reinit_velocity(matcher, gravity, noise, T_body_sensor, T_wc_prev, bias_good, acc, gyro, timestamps_ns, hz, T_cw_new):
    """Test tap: the velocity rule of an IMU relocalisation's second pose (k_imu_preintegrate_b + k_reloc_velocity) on one
    bucket; returns dict(dt, velocity_prev, velocity, rot_residual)."""
    imu = _imu_input(gravity, noise, T_body_sensor, T_wc_prev, np.zeros(3), bias_good, acc, gyro, timestamps_ns, hz)
    T = np.ascontiguousarray(T_cw_new, np.float64).reshape(16)
    out = np.zeros(8)
    _chk(matcher.L.vslam_imu_reinit_velocity(matcher.h, C.byref(imu), _p(T), _p(out)))
    return dict(dt=out[0], velocity_prev=out[1:4].copy(), velocity=out[4:7].copy(), rot_residual=out[7])


def imu_reinit_velocity_batch(matcher, lanes, fill=np.nan):
    """Test tap: one launch of each kernel (k_imu_preintegrate_b, k_reloc_velocity_b) for several lanes.  lanes: per lane the
    argument tuple of imu_reinit_velocity after `matcher` (an empty bucket = idle lane).  The rows start at `fill`; returns
    out (B, 8): dt, velocity_prev[3], velocity[3], rot_residual."""
    B = len(lanes)
    imus = (ImuInput * B)()
    keep = []
    T = np.zeros((B, 16))
    for b, args in enumerate(lanes):
        one = _imu_input(args[0], args[1], args[2], args[3], np.zeros(3), *args[4:9])
        keep.append(one)
        imus[b] = one
        T[b] = np.asarray(args[9], np.float64).reshape(16)
    out = np.full((B, 8), fill)
    _chk(matcher.L.vslam_imu_reinit_velocity_batch(matcher.h, B, imus, _p(T), _p(out)))
    return out


def tracker_set_map(matcher, xyz, desc, max_scale_dist, is_outlier=None):
    xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    msd = np.ascontiguousarray(max_scale_dist, np.float32)
    ol = None if is_outlier is None else np.ascontiguousarray(is_outlier, np.uint8)
    _chk(matcher.L.vslam_tracker_set_map(matcher.h, _p(xyz), _p(desc), _p(msd), _p(ol) if ol is not None else None, len(xyz)))


def tracker_track_mono_imu(matcher, gravity, noise, T_body_sensor, T_wc_prev, vel_prev, bias_prev, pred_velocity, fps,
                           acc, gyro, timestamps_ns, hz):
    """Tracking block of TrackImageMonoIMU; returns (T_cw, report, velocity, bias, T_wc_pred, pred_velocity)."""
    imu = _imu_input(gravity, noise, T_body_sensor, T_wc_prev, vel_prev, bias_prev, acc, gyro, timestamps_ns, hz)
    pv = np.ascontiguousarray(pred_velocity, np.float64)
    out = np.zeros((4, 4)); Tp = np.zeros((4, 4)); pvo = np.zeros(3)
    o = ImuOutput()
    rep = TrackReport()
    _chk(matcher.L.vslam_tracker_track_mono_imu(matcher.h, C.byref(imu), _p(pv), C.c_double(fps), _p(out), C.byref(o), _p(Tp), _p(pvo),
                                                C.byref(rep)))
    return out, {f[0]: getattr(rep, f[0]) for f in TrackReport._fields_}, np.array(list(o.velocity)), np.array(list(o.bias)), Tp, pvo


# ---- new-point pipeline (LocalMapper::findNewPoints) / MapPoint::calcDescriptor ------------------------
class KfView(C.Structure):
    _fields_ = [("T_wc", C.c_void_p), ("id", C.c_int64), ("n_left", C.c_int32), ("n_right", C.c_int32),
                ("kps_l", C.c_void_p), ("desc_l", C.c_void_p), ("kps_r", C.c_void_p), ("desc_r", C.c_void_p),
                ("right_idxs", C.c_void_p), ("left_idxs", C.c_void_p), ("unmatched_f", C.c_void_p), ("unmatched_fr", C.c_void_p),
                ("device_keys", C.c_void_p), ("estimated_depth", C.c_void_p), ("close_flags", C.c_void_p)]


class NewPointsProblem(C.Structure):
    _fields_ = [("rig", Rig), ("n_levels", C.c_int32), ("scale_pyramid", C.c_void_p), ("sigma_factor", C.c_void_p),
                ("log_scale", C.c_float), ("n_kf", C.c_int32), ("kfs", C.c_void_p), ("estimated_depth", C.c_void_p),
                ("has_mp", C.c_void_p), ("mp_xyz", C.c_void_p), ("mp_desc", C.c_void_p)]


class NewPointsResult(C.Structure):
    _fields_ = [("capacity", C.c_int32), ("n_candidates", C.c_int32), ("cand_left", C.c_void_p), ("cand_right", C.c_void_p),
                ("accepted", C.c_void_p), ("xyz", C.c_void_p), ("n_obs", C.c_void_p), ("obs", C.c_void_p)]


def _kf_view(v, kf, ptr):
    v.T_wc = ptr(kf["T_wc"], np.float64); v.id = int(kf["id"]); v.n_left = len(kf["kpsL"]); v.n_right = len(kf["kpsR"])
    v.kps_l, v.desc_l = ptr(kf["kpsL"], KP_DTYPE), ptr(kf["descL"], np.uint8)
    v.kps_r, v.desc_r = ptr(kf["kpsR"], KP_DTYPE), ptr(kf["descR"], np.uint8)
    v.right_idxs, v.left_idxs = ptr(kf["rightIdxs"], np.int32), ptr(kf["leftIdxs"], np.int32)
    v.unmatched_f, v.unmatched_fr = ptr(kf["unF"], np.int32), ptr(kf["unFR"], np.int32)


def _np_call(rig, scale_pyramid, sigma_factor, kfs, last, keep, n_kf=None, capacity=None, device_keys=None):
    """problem and result structures of one window (their arrays stay alive in `keep`) -> (P, R, result arrays)"""
    n = len(kfs)

    def ptr(a, dt):
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return a.ctypes.data if a.size else None

    views = (KfView * max(n, 1))()
    for k, kf in enumerate(kfs):
        _kf_view(views[k], kf, ptr)
        if device_keys and k in device_keys:
            views[k].device_keys = int(device_keys[k])
    sp = np.ascontiguousarray(scale_pyramid, np.float32); sg = np.ascontiguousarray(sigma_factor, np.float32)
    keep.extend([views, sp, sg])
    P = NewPointsProblem()
    P.rig = make_rig(rig); P.n_levels = len(sp); P.scale_pyramid, P.sigma_factor = _p(sp), _p(sg)
    P.log_scale = float(np.float32(np.log(np.float64(sp[1])))); P.n_kf = n if n_kf is None else int(n_kf); P.kfs = C.cast(views, C.c_void_p)
    P.estimated_depth, P.has_mp = ptr(last["depth"], np.float32), ptr(last["hasMp"], np.uint8)
    P.mp_xyz, P.mp_desc = ptr(last["mpXyz"], np.float64), ptr(last["mpDesc"], np.uint8)
    n0 = max(len(kfs[0]["kpsL"]), 1)
    out = dict(cL=np.zeros(n0, np.int32), cR=np.zeros(n0, np.int32), acc=np.zeros(n0, np.uint8), xyz=np.zeros((n0, 3)),
               nObs=np.zeros(n0, np.int32), obs=np.full((n0, max(n, 1), 3), -1, np.int32))
    R = NewPointsResult()
    R.capacity = n0 if capacity is None else int(capacity)
    R.cand_left, R.cand_right, R.accepted, R.xyz, R.n_obs, R.obs = (_p(out[k]) for k in ("cL", "cR", "acc", "xyz", "nObs", "obs"))
    return P, R, out


def _np_out(R, o):
    nc = R.n_candidates
    return dict(n=nc, candL=o["cL"][:nc], candR=o["cR"][:nc], accepted=o["acc"][:nc], xyz=o["xyz"][:nc], nObs=o["nObs"][:nc], obs=o["obs"][:nc])


def find_new_points(rig, scale_pyramid, sigma_factor, kfs, last, device=0, n_kf=None, capacity=None, device_keys=None):
    """kfs: list of dicts (T_wc, id, kpsL, descL, kpsR, descR, rightIdxs, leftIdxs, unF, unFR), kfs[0] = lastKF;
    last: dict(depth, hasMp, mpXyz, mpDesc).  Test taps: n_kf / capacity override what the structures say (argument
    checks; a VslamError then carries n_candidates), device_keys = {k: device address of keyframe k's resident block}."""
    keep = []
    P, R, o = _np_call(rig, scale_pyramid, sigma_factor, kfs, last, keep, n_kf, capacity, device_keys)
    st = lib().vslam_find_new_points(C.byref(P), C.byref(R), int(device))
    if st != OK:
        e = VslamError(st, lib().vslam_last_error().decode())
        e.n_candidates = R.n_candidates
        raise e
    return _np_out(R, o)


def find_new_points_batch(rig, scale_pyramid, sigma_factor, windows, device=0):
    """vslam_find_new_points_batch: windows = list of (kfs, last); one result dict per window"""
    keep, calls = [], []
    for kfs, last in windows:
        calls.append(_np_call(rig, scale_pyramid, sigma_factor, kfs, last, keep))
    n = len(calls)
    Ps = (C.POINTER(NewPointsProblem) * n)(*[C.pointer(c[0]) for c in calls])
    Rs = (C.POINTER(NewPointsResult) * n)(*[C.pointer(c[1]) for c in calls])
    _chk(lib().vslam_find_new_points_batch(Ps, Rs, n, int(device)))
    return [_np_out(c[1], c[2]) for c in calls]


def kf_keys_bytes(n_left, n_right):
    lib().vslam_kf_keys_bytes.restype = C.c_size_t
    return int(lib().vslam_kf_keys_bytes(int(n_left), int(n_right)))


def kf_keys_upload(kf, device_block, device=0):
    """fills the device block at address device_block (kf_keys_bytes(...) bytes of device memory owned by the caller) from
    the keyframe dict's host arrays"""
    keep = []

    def ptr(a, dt):
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return a.ctypes.data if a.size else None

    v = KfView()
    _kf_view(v, kf, ptr)
    _chk(lib().vslam_kf_keys_upload(C.byref(v), int(device), C.c_void_p(int(device_block))))


class MonoPointsProblem(C.Structure):
    _fields_ = [("rig", Rig), ("n_levels", C.c_int32), ("sigma_factor", C.c_void_p), ("n_kf", C.c_int32),
                ("kf_pose_wc", C.c_void_p), ("kf_id", C.c_void_p), ("n_points", C.c_int32), ("n_views", C.c_void_p),
                ("view_kf", C.c_void_p), ("view_xy", C.c_void_p), ("view_octave", C.c_void_p)]


class MonoPointsResult(C.Structure):
    _fields_ = [("accepted", C.c_void_p), ("xyz", C.c_void_p), ("n_obs", C.c_void_p), ("keep", C.c_void_p)]


def mono_new_points(rig, sigma_factor, kf_pose_wc, kf_id, n_views, view_kf, view_xy, view_octave, device=0):
    """calculateMPFromMono + mono checkReprojError for every keypoint of lastKF (keyframe 0).
    view_*: (n_points, n_kf[, 2]) arrays, the first n_views[i] entries of row i are used."""
    T = np.ascontiguousarray(kf_pose_wc, np.float64).reshape(-1, 16)
    nK = len(T)
    ids = np.ascontiguousarray(kf_id, np.int32)
    sg = np.ascontiguousarray(sigma_factor, np.float32)
    nv = np.ascontiguousarray(n_views, np.int32); nP = len(nv)
    vk = np.ascontiguousarray(view_kf, np.int32).reshape(nP, nK)
    vxy = np.ascontiguousarray(view_xy, np.float32).reshape(nP, nK, 2)
    vo = np.ascontiguousarray(view_octave, np.int32).reshape(nP, nK)
    acc = np.zeros(max(nP, 1), np.uint8); xyz = np.zeros((max(nP, 1), 3)); nobs = np.zeros(max(nP, 1), np.int32)
    keep = np.zeros((max(nP, 1), nK), np.uint8)
    P = MonoPointsProblem()
    P.rig = make_rig(rig); P.n_levels = len(sg); P.sigma_factor = _p(sg); P.n_kf = nK; P.kf_pose_wc = _p(T); P.kf_id = _p(ids)
    P.n_points = nP; P.n_views, P.view_kf, P.view_xy, P.view_octave = _p(nv), _p(vk), _p(vxy), _p(vo)
    R = MonoPointsResult()
    R.accepted, R.xyz, R.n_obs, R.keep = _p(acc), _p(xyz), _p(nobs), _p(keep)
    _chk(lib().vslam_mono_new_points(C.byref(P), C.byref(R), int(device)))
    return dict(accepted=acc[:nP], xyz=xyz[:nP], nObs=nobs[:nP], keep=keep[:nP])


class KfUpdateProblem(C.Structure):
    _fields_ = [("rig", Rig), ("n_levels", C.c_int32), ("inv_sigma_factor", C.c_void_p), ("numb", C.c_int64),
                ("key_pose", C.c_void_p), ("ref_pose", C.c_void_p), ("cur_pose_inv", C.c_void_p),
                ("n_left", C.c_int32), ("n_right", C.c_int32), ("kps_left", C.c_void_p), ("kps_right", C.c_void_p),
                ("slot_lm_l", C.c_void_p), ("slot_lm_r", C.c_void_p), ("n_lm", C.c_int32), ("lm_xyz", C.c_void_p),
                ("lm_kdx", C.c_void_p), ("lm_outlier", C.c_void_p)]


def keyframe_update_pose(rig, inv_sigma_factor, numb, key_pose, ref_pose, cur_pose_inv, kpsL, kpsR, slotL, slotR,
                         lm_xyz, lm_kdx, lm_outlier, device=0):
    """KeyFrame::updatePose; returns dict(lm (updated copy), dropL, dropR, pose)."""
    isf = np.ascontiguousarray(inv_sigma_factor, np.float32)
    kp, rp, ci = (np.ascontiguousarray(a, np.float64).reshape(16) for a in (key_pose, ref_pose, cur_pose_inv))
    kl = np.ascontiguousarray(kpsL, KP_DTYPE); kr = np.ascontiguousarray(kpsR, KP_DTYPE)
    sl = np.ascontiguousarray(slotL, np.int32); sr = np.ascontiguousarray(slotR, np.int32)
    lm = np.array(lm_xyz, np.float64).reshape(-1, 3).copy()
    kd = np.ascontiguousarray(lm_kdx, np.int64); ol = np.ascontiguousarray(lm_outlier, np.uint8)
    dl = np.zeros(max(len(kl), 1), np.uint8); dr = np.zeros(max(len(kr), 1), np.uint8); pose = np.zeros(16)
    P = KfUpdateProblem()
    P.rig = make_rig(rig); P.n_levels = len(isf); P.inv_sigma_factor = _p(isf); P.numb = int(numb)
    P.key_pose, P.ref_pose, P.cur_pose_inv = _p(kp), _p(rp), _p(ci)
    P.n_left, P.n_right = len(kl), len(kr)
    P.kps_left, P.kps_right, P.slot_lm_l, P.slot_lm_r = _p(kl), _p(kr), _p(sl), _p(sr)
    P.n_lm = len(lm); P.lm_xyz, P.lm_kdx, P.lm_outlier = _p(lm), _p(kd), _p(ol)
    _chk(lib().vslam_keyframe_update_pose(C.byref(P), int(device), _p(dl), _p(dr), _p(pose)))
    return dict(lm=lm, dropL=dl[:len(kl)], dropR=dr[:len(kr)], pose=pose.reshape(4, 4))


def save_trajectory(path, path_positions, is_keyframe, pose_or_ref):
    """VSlamSystem::saveTrajectoryAndPosition: is_keyframe (n,), pose_or_ref (n,4,4): the pose of a keyframe, the
    refPose (relative to the closest previous keyframe) of any other frame."""
    kf = np.ascontiguousarray(is_keyframe, np.uint8); T = np.ascontiguousarray(pose_or_ref, np.float64).reshape(-1, 16)
    _chk(lib().vslam_save_trajectory(path.encode(), path_positions.encode() if path_positions else None, len(kf), _p(kf), _p(T)))


def calc_descriptors(desc_lists, device=0):
    """desc_lists: list of (n_i, 32) uint8 arrays; returns the chosen index per map point."""
    start = np.zeros(len(desc_lists) + 1, np.int32)
    for i, d in enumerate(desc_lists):
        start[i + 1] = start[i] + len(d)
    allv = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in desc_lists if len(d)]
    descs = np.concatenate(allv) if allv else np.zeros((1, 32), np.uint8)
    best = np.full(max(len(desc_lists), 1), -1, np.int32)
    _chk(lib().vslam_calc_descriptors(_p(descs), _p(start), len(desc_lists), int(device), _p(best)))
    return best[:len(desc_lists)]


# ---- closed loop: vslam_system (VSlamSystem::TrackStereo[IMU] + the optimizer thread) ---------------------------------
class SystemConfig(C.Structure):
    _fields_ = [("fe", FeParams), ("rig", Rig), ("device", C.c_int32), ("use_imu", C.c_int32), ("local_mapping", C.c_int32),
                ("window", C.c_int32), ("T_wc_init", C.c_double * 16), ("gravity", C.c_double * 3),
                ("gyro_noise_density", C.c_double), ("gyro_random_walk", C.c_double), ("accel_noise_density", C.c_double),
                ("accel_random_walk", C.c_double), ("T_body_sensor", C.c_double * 16), ("imu_hz", C.c_int32),
                ("velocity_init", C.c_double * 3), ("mapping_delay", C.c_int32), ("mapping_np_delay", C.c_int32)]


class ImuBucket(C.Structure):
    _fields_ = [("n", C.c_int32), ("acceleration", C.c_void_p), ("angular_velocity", C.c_void_p), ("timestamps_ns", C.c_void_p)]


class FrameReport(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("frame", "keyframe_inserted", "n_active", "n_inliers", "n_stereo", "rounds", "lm_iterations",
                                         "n_keyframes", "n_map_points", "n_active_after", "mapping_ran", "new_points", "ba_keyframes",
                                         "ba_local", "ba_landmarks", "ba_pairs", "ba_wrong", "ba_outliers", "ba_residuals", "ba_free_kf",
                                         "ba_sum_k2", "ba_trials", "ba_rounds")] + [("ba_report", LmReport * 2)]


class System:
    """vslam_system: one stereo (+ IMU) session with its map, tracker and local mapper."""

    def __init__(self, rig, nfeatures, T0=None, imu=None, local_mapping=1, window=10, device=0, nlevels=8, scale=1.2, mapping_delay=0,
                 mapping_np_delay=0):
        self.L = lib()
        cfg = SystemConfig()
        cfg.fe = FeParams(nfeatures, nlevels, scale, 19, 31, 20, 7)
        cfg.rig = make_rig(rig)
        cfg.device = device; cfg.local_mapping = local_mapping; cfg.window = window; cfg.mapping_delay = mapping_delay; cfg.mapping_np_delay = mapping_np_delay
        if T0 is not None:
            cfg.T_wc_init = (C.c_double * 16)(*np.asarray(T0, np.float64).reshape(16))
        if imu is not None:     # dict(gravity, noise=(gyro density, gyro walk, acc density, acc walk), T_bs, hz)
            cfg.use_imu = 1
            cfg.gravity = (C.c_double * 3)(*imu["gravity"])
            cfg.gyro_noise_density, cfg.gyro_random_walk, cfg.accel_noise_density, cfg.accel_random_walk = imu["noise"]
            cfg.T_body_sensor = (C.c_double * 16)(*np.asarray(imu["T_bs"], np.float64).reshape(16))
            cfg.imu_hz = int(imu["hz"])
            if "velocity" in imu:
                cfg.velocity_init = (C.c_double * 3)(*imu["velocity"])
        self.w, self.h = rig["w"], rig["h"]
        self.rig = dict(rig)
        self.h_sys = C.c_void_p()
        _chk(self.L.vslam_system_create(C.byref(cfg), C.byref(self.h_sys)))

    def close(self):
        if self.h_sys:
            self.L.vslam_system_destroy(self.h_sys)
            self.h_sys = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_rectifiers(self, left, right):
        """bind the cameras' Rectifier objects for track(raw=True) (None, None unbinds); they must outlive the session"""
        _chk(self.L.vslam_system_set_rectifiers(self.h_sys, left.h_r if left is not None else None, right.h_r if right is not None else None))
        self.src_size = (left.sw, left.sh) if left is not None else None

    def track(self, left, right, frame_number, imu_bucket=None, on_device=False, stride=None, channels=1, raw=False):
        """left / right: u8 arrays (host: (H, W) gray, (H, W, 3) BGR or (H, W, 4) BGRA) or device pointers (on_device, with
        `channels`).  imu_bucket: (acc (n,3), gyro (n,3), timestamps_ns (n)).  raw: unrectified frames of the bound
        rectifiers' source size (sh, sw[, cn]; stride default sw x cn), rectified on the way into the pyramid."""
        T = np.zeros((4, 4))
        rep = FrameReport()
        b = None
        keep = []
        if imu_bucket is not None:
            acc, gyr, ts = (np.ascontiguousarray(a, np.float64) for a in imu_bucket)
            keep = [acc, gyr, ts]
            b = ImuBucket(len(ts), _p(acc), _p(gyr), _p(ts))
        sw, sh = (getattr(self, "src_size", None) or (self.w, self.h)) if raw else (self.w, self.h)
        if on_device:
            lp, rp, st, ch = C.c_void_p(left), C.c_void_p(right), stride or sw * channels, channels
        else:
            left, ch, st = _image(left, sh, sw)
            right, chr_, _ = _image(right, sh, sw)
            if chr_ != ch or right.strides[0] != st:
                raise ValueError("left and right images differ in channels")
            keep += [left, right]
            lp, rp = _p(left), _p(right)
        if raw:
            _chk(self.L.vslam_system_track_stereo_raw(self.h_sys, lp, rp, int(st), int(ch), int(on_device), int(frame_number),
                                                      C.byref(b) if b is not None else None, _p(T), C.byref(rep)))
        elif ch == 1:
            _chk(self.L.vslam_system_track_stereo(self.h_sys, lp, rp, st, int(on_device), int(frame_number),
                                                  C.byref(b) if b is not None else None, _p(T), C.byref(rep)))
        else:
            _chk(self.L.vslam_system_track_stereo_color(self.h_sys, lp, rp, int(st), int(ch), int(on_device), int(frame_number),
                                                        C.byref(b) if b is not None else None, _p(T), C.byref(rep)))
        d = {f[0]: getattr(rep, f[0]) for f in FrameReport._fields_ if f[0] != "ba_report"}
        d["ba_report"] = [dict(iterations=r.iterations, inner=r.inner_iterations, initialError=r.initial_error,
                               finalError=r.final_error, lam=r.lam) for r in rep.ba_report]
        return T, d

    def relocalize(self, left, right, frame_number, on_device=False, stride=None, **params):
        """vslam_system_relocalize with gray frames: (T_wc, report dict); T_wc is the unchanged camera pose on failure"""
        T = np.zeros((4, 4))
        rep = RelocReport()
        prm = RelocParams(**{k: int(v) for k, v in params.items()})
        if on_device:
            lp, rp, st = C.c_void_p(left), C.c_void_p(right), stride or self.w
            keep = []
        else:
            left, ch, st = _image(left, self.h, self.w)
            right, chr_, _ = _image(right, self.h, self.w)
            if ch != 1 or chr_ != 1:
                raise ValueError("relocalize takes gray frames")
            keep = [left, right]
            lp, rp = _p(left), _p(right)
        _chk(self.L.vslam_system_relocalize(self.h_sys, lp, rp, int(st), int(on_device), int(frame_number), C.byref(prm), _p(T),
                                            C.byref(rep)))
        return T, _reloc_report_dict(rep)

    def relocalize_imu(self, left, right, frame_number, imu_bucket=None, on_device=False, stride=None, **params):
        """vslam_system_relocalize_imu with gray frames: (T_wc, report dict, IMU report dict).  The first successful call commits
        the pose (phase 1); the next one takes the bucket since it and re-initialises the velocity (phase 2)."""
        T = np.zeros((4, 4))
        rep = RelocReport(); irep = RelocImuReport()
        prm = RelocParams(**{k: int(v) for k, v in params.items()})
        b = None
        keep = []
        if imu_bucket is not None:
            acc, gyr, ts = (np.ascontiguousarray(a, np.float64) for a in imu_bucket)
            keep = [acc, gyr, ts]
            b = ImuBucket(len(ts), _p(acc), _p(gyr), _p(ts))
        if on_device:
            lp, rp, st = C.c_void_p(left), C.c_void_p(right), stride or self.w
        else:
            left, ch, st = _image(left, self.h, self.w)
            right, chr_, _ = _image(right, self.h, self.w)
            if ch != 1 or chr_ != 1:
                raise ValueError("relocalize takes gray frames")
            keep += [left, right]
            lp, rp = _p(left), _p(right)
        _chk(self.L.vslam_system_relocalize_imu(self.h_sys, lp, rp, int(st), int(on_device), int(frame_number),
                                                C.byref(b) if b is not None else None, C.byref(prm), _p(T), C.byref(rep), C.byref(irep)))
        return T, _reloc_report_dict(rep), _reloc_imu_report_dict(irep)

    @staticmethod
    def _loop_params(params):
        prm = LoopParams()
        for k, v in params.items():
            if k in ("max_iterations", "lambda0"):
                setattr(prm.pgo, k, v)
            elif k in ("min_kf_gap", "covis_min", "detect_only"):
                setattr(prm, k, int(v))
            elif k == "loop_weight":
                prm.loop_weight = float(v)
            else:
                setattr(prm.reloc, k, int(v))       # the fields of RelocParams
        return prm

    def correct_loop(self, kf_loop, T_wc_corrected, **params):
        """vslam_system_correct_loop: the current camera really is at T_wc_corrected, keyframe kf_loop anchors it.  params:
        covis_min, loop_weight, max_iterations, lambda0.  Returns the report dict (busy: nothing was done)."""
        T = np.ascontiguousarray(T_wc_corrected, np.float64).reshape(4, 4)
        rep = LoopReport()
        prm = self._loop_params(params)
        _chk(self.L.vslam_system_correct_loop(self.h_sys, int(kf_loop), _p(T), C.byref(prm), C.byref(rep)))
        return _loop_report_dict(rep)

    def close_loop(self, **params):
        """vslam_system_close_loop on the frame of the last track(): detection over the map points the tracker has left behind,
        then (unless detect_only=1) the correction.  params: min_kf_gap, covis_min, loop_weight, detect_only, max_iterations,
        lambda0 and the fields of RelocParams.  Returns the report dict."""
        rep = LoopReport()
        prm = self._loop_params(params)
        _chk(self.L.vslam_system_close_loop(self.h_sys, C.byref(prm), C.byref(rep)))
        return _loop_report_dict(rep)

    def correct_loop_imu(self, kf_loop, T_wc_corrected, **params):
        """vslam_system_correct_loop_imu (a stereo + IMU session): correct_loop with the claim projected to a rotation about gravity
        and a translation, the yaw-only solve, and the velocity rotated with the camera.  Returns (report dict, IMU report dict)."""
        T = np.ascontiguousarray(T_wc_corrected, np.float64).reshape(4, 4)
        rep = LoopReport(); irep = LoopImuReport()
        prm = self._loop_params(params)
        _chk(self.L.vslam_system_correct_loop_imu(self.h_sys, int(kf_loop), _p(T), C.byref(prm), C.byref(rep), C.byref(irep)))
        return _loop_report_dict(rep), _loop_imu_report_dict(irep)

    def close_loop_imu(self, **params):
        """vslam_system_close_loop_imu: close_loop's detection on the frame of the last track(), then (unless detect_only=1) the
        correction of correct_loop_imu.  Returns (report dict, IMU report dict)."""
        rep = LoopReport(); irep = LoopImuReport()
        prm = self._loop_params(params)
        _chk(self.L.vslam_system_close_loop_imu(self.h_sys, C.byref(prm), C.byref(rep), C.byref(irep)))
        return _loop_report_dict(rep), _loop_imu_report_dict(irep)

    def fuse_loop(self, **params):
        """vslam_system_fuse_loop: the duplicate map points of the place the camera sees become one.  params: radius, depth_ratio,
        max_hamming, min_kf_gap.  Returns the report dict (busy: nothing was done)."""
        prm = self._fuse_loop_params(params)
        rep = FuseLoopReport()
        _chk(self.L.vslam_system_fuse_loop(self.h_sys, C.byref(prm), C.byref(rep)))
        return _fuse_loop_report_dict(rep)

    @staticmethod
    def _fuse_loop_params(params):
        prm = FuseLoopParams()
        for k, v in params.items():
            if k == "min_kf_gap":
                prm.min_kf_gap = int(v)
            elif k == "max_hamming":
                prm.search.max_hamming = int(v)
            else:
                setattr(prm.search, k, float(v))     # radius, depth_ratio
        return prm

    def map_point_descriptors(self):
        """test tap: (n, 32) descriptor bytes of every map point, creation order"""
        n = C.c_int32(); d = np.zeros((max(self.counts()["map_points"], 1), 32), np.uint8)
        _chk(self.L.vslam_system_map_point_descriptors(self.h_sys, len(d), C.byref(n), _p(d)))
        return d[:n.value].copy()

    def map_point_observations(self):
        """test tap: (offsets (n + 1), triples (n_obs, 3) of (keyframe, left index, right index)) over every map point"""
        n = C.c_int32(); m = C.c_int32()
        _chk(self.L.vslam_system_map_point_observations(self.h_sys, 0, 0, C.byref(n), C.byref(m), None, None))
        off = np.zeros(n.value + 1, np.int32); tr = np.zeros((max(m.value, 1), 3), np.int32)
        _chk(self.L.vslam_system_map_point_observations(self.h_sys, n.value, len(tr), C.byref(n), C.byref(m), _p(off), _p(tr)))
        return off, tr[:m.value].copy()

    def keyframe_points(self, kf):
        """test tap: (localMapPoints, localMapPointsR) of keyframe kf as map-point indices, -1 for none"""
        nl = C.c_int32(); nr = C.c_int32()
        _chk(self.L.vslam_system_keyframe_points(self.h_sys, int(kf), 0, 0, C.byref(nl), C.byref(nr), None, None))
        a = np.zeros(max(nl.value, 1), np.int32); b = np.zeros(max(nr.value, 1), np.int32)
        _chk(self.L.vslam_system_keyframe_points(self.h_sys, int(kf), len(a), len(b), C.byref(nl), C.byref(nr), _p(a), _p(b)))
        return a[:nl.value].copy(), b[:nr.value].copy()

    def fused_pairs(self):
        """test tap: (n, 2) (absorbed, kept) map-point indices of the last fuse_loop call"""
        n = C.c_int32()
        self.L.vslam_system_fused_pairs(self.h_sys, 0, C.byref(n), None)
        pr = np.zeros((max(n.value, 1), 2), np.int32)
        _chk(self.L.vslam_system_fused_pairs(self.h_sys, len(pr), C.byref(n), _p(pr)))
        return pr[:n.value].copy()

    def global_ba(self, edge_weight=0.0, max_iterations=0, lambda0=0.0):
        """vslam_system_global_ba: one global bundle adjustment over the whole map.  Returns the report dict (busy: nothing was
        done; success 0: fewer than two keyframes)."""
        prm = SystemGbaParams(GbaParams(int(max_iterations), float(lambda0)), float(edge_weight))
        rep = SystemGbaReport()
        _chk(self.L.vslam_system_global_ba(self.h_sys, C.byref(prm), C.byref(rep)))
        return _system_gba_report_dict(rep)

    def fuse_loop_imu(self, **params):
        """vslam_system_fuse_loop_imu (a stereo + IMU session): fuse_loop; the IMU state is not touched"""
        prm = self._fuse_loop_params(params)
        rep = FuseLoopReport()
        _chk(self.L.vslam_system_fuse_loop_imu(self.h_sys, C.byref(prm), C.byref(rep)))
        return _fuse_loop_report_dict(rep)

    def global_ba_imu(self, edge_weight=0.0, max_iterations=0, lambda0=0.0):
        """vslam_system_global_ba_imu (a stereo + IMU session): global_ba with keyframes that move only by a rotation about gravity
        and a translation; the velocity turns with the camera.  Returns (report dict, dict(yaw, velocity_before, velocity, T_wc))."""
        prm = SystemGbaParams(GbaParams(int(max_iterations), float(lambda0)), float(edge_weight))
        rep = SystemGbaReport(); irep = GbaImuReport()
        _chk(self.L.vslam_system_global_ba_imu(self.h_sys, C.byref(prm), C.byref(rep), C.byref(irep)))
        return _system_gba_report_dict(rep), dict(yaw=irep.yaw, velocity_before=np.array(irep.velocity_before), velocity=np.array(irep.velocity),
                                                  T_wc=np.array(irep.T_wc).reshape(4, 4))

    def global_ba_problem_imu(self, edge_weight=0.0):
        """test tap: global_ba_problem on a stereo + IMU session (what global_ba_imu would build now)"""
        return self.global_ba_problem(edge_weight, call=self.L.vslam_system_global_ba_problem_imu)

    def global_ba_problem(self, edge_weight=0.0, call=None):
        """test tap: (problem dict as global_ba takes it, plus lm_index, sigma_factor and inv_sigma_factor; edges array) that
        Session.global_ba would build now"""
        sz = (C.c_int32 * 5)()
        call = call or self.L.vslam_system_global_ba_problem
        _chk(call(self.h_sys, C.c_double(edge_weight), 0, sz, *([None] * 13)))
        K, Lm, NP, M, nLev = (int(v) for v in sz)
        z = lambda shape, dt: np.zeros(shape, dt)
        kf, fx, lc = z((max(K, 1), 4, 4), np.float64), z(max(K, 1), np.uint8), z(max(K, 1), np.uint8)
        lm, li = z((max(Lm, 1), 3), np.float64), z(max(Lm, 1), np.int32)
        pk, pl, pf = z(max(NP, 1), np.int32), z(max(NP, 1), np.int32), z(max(NP, 1), np.uint8)
        uv, oc = z((max(NP, 1), 4), np.float32), z((max(NP, 1), 2), np.int32)
        ed, sf, isf = z(max(M, 1), PGO_EDGE_DTYPE), z(max(nLev, 1), np.float32), z(max(nLev, 1), np.float32)
        sz2 = (C.c_int32 * 5)()
        _chk(call(self.h_sys, C.c_double(edge_weight), 1, sz2, _p(kf), _p(fx), _p(lc), _p(lm), _p(li), _p(pk), _p(pl), _p(pf), _p(uv), _p(oc),
                  _p(ed), _p(sf), _p(isf)))
        assert list(sz2) == list(sz)
        prob = dict(rig=self.rig, kf_pose=kf[:K], kf_fixed=fx[:K], kf_local=lc[:K], lm=lm[:Lm], lm_index=li[:Lm], pair_kf=pk[:NP], pair_lm=pl[:NP],
                    pair_flags=pf[:NP], pair_uv=uv[:NP], pair_oct=oc[:NP], sigma_factor=sf[:nLev], inv_sigma_factor=isf[:nLev])
        return prob, ed[:M]

    def active_points(self):
        """test tap: activeMapPoints as map-point indices"""
        n = C.c_int32(); idx = np.zeros(max(self.counts()["active"], 1), np.int32)
        _chk(self.L.vslam_system_active_points(self.h_sys, len(idx), C.byref(n), _p(idx)))
        return idx[:n.value].copy()

    def covisibility(self):
        """test tap: every sortedKFWeights entry as rows (keyframe, other keyframe, weight)"""
        n = C.c_int32()
        self.L.vslam_system_covisibility(self.h_sys, 0, C.byref(n), None)
        tr = np.zeros((max(n.value, 1), 3), np.int32)
        _chk(self.L.vslam_system_covisibility(self.h_sys, len(tr), C.byref(n), _p(tr)))
        return tr[:n.value].copy()

    def map_point_keyframes(self):
        """test tap: per map point (first observing keyframe or -1, creating keyframe)"""
        n = C.c_int32(); cap = max(self.counts()["map_points"], 1)
        fo = np.zeros(cap, np.int32); cr = np.zeros(cap, np.int32)
        _chk(self.L.vslam_system_map_point_keyframes(self.h_sys, cap, C.byref(n), _p(fo), _p(cr)))
        return fo[:n.value].copy(), cr[:n.value].copy()

    def imu_state(self):
        """test tap: dict(velocity, bias, bias_good, pending) of the session"""
        v = np.zeros(3); b = np.zeros(6); g = np.zeros(6); p = C.c_int32()
        _chk(self.L.vslam_system_imu_state(self.h_sys, _p(v), _p(b), _p(g), C.byref(p)))
        return dict(velocity=v, bias=b, bias_good=g, pending=p.value)

    def wait_mapping(self):
        _chk(self.L.vslam_system_wait_mapping(self.h_sys))

    def counts(self):
        v = [C.c_int32() for _ in range(4)]
        _chk(self.L.vslam_system_counts(self.h_sys, *[C.byref(x) for x in v]))
        return dict(keyframes=v[0].value, map_points=v[1].value, active=v[2].value, frames=v[3].value)

    def keyframes(self, cap=4096):
        n = C.c_int32(); fi = np.zeros(cap, np.int32); P = np.zeros((cap, 4, 4))
        _chk(self.L.vslam_system_keyframes(self.h_sys, cap, C.byref(n), _p(fi), _p(P)))
        return fi[:n.value].copy(), P[:n.value].copy()

    def last_frame(self, cap=65536):
        n = C.c_int32(); mt = np.zeros((cap, 2), np.int32); ol = np.zeros(cap, np.uint8)
        _chk(self.L.vslam_system_last_frame(self.h_sys, cap, C.byref(n), _p(mt), _p(ol)))
        return mt[:n.value].copy(), ol[:n.value].copy()

    def save_trajectory(self, path, path_positions=None):
        _chk(self.L.vslam_system_save_trajectory(self.h_sys, path.encode(), path_positions.encode() if path_positions else None))

    def map_points(self):
        n = C.c_int32(self.counts()["map_points"])
        xyz = np.zeros((max(n.value, 1), 3)); ol = np.zeros(max(n.value, 1), np.uint8)
        _chk(self.L.vslam_system_map_points(self.h_sys, max(n.value, 1), C.byref(n), _p(xyz), _p(ol)))
        return xyz[:n.value].copy(), ol[:n.value].copy()


class MonoFrameReport(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("frame", "state", "keyframe_inserted", "n_active", "n_inliers", "rounds", "lm_iterations")] + \
               [("last_radius", C.c_float)] + \
               [(n, C.c_int32) for n in ("new_points", "radius_matches", "n_keyframes", "n_map_points", "n_active_after")]


MONO_REFUSED, MONO_BOOTSTRAP, MONO_INITIALISED, MONO_TRACKED = 0, 1, 2, 3


class MonoSystem(System):
    """vslam_system in mono + IMU mode (VSlamSystem::TrackMonoIMU): a batch-1 extractor, a mono matcher, no local mapper.
    imu: dict(gravity, noise=(gyro density, gyro walk, acc density, acc walk), T_bs, hz[, velocity]); fps = the camera's rate."""

    def __init__(self, rig, nfeatures, fps, T0=None, imu=None, device=0, nlevels=8, scale=1.2, local_mapping=0, window=10):
        self.L = lib()
        cfg = SystemConfig()
        cfg.fe = FeParams(nfeatures, nlevels, scale, 19, 31, 20, 7)
        cfg.rig = make_rig(rig)
        cfg.device = device; cfg.local_mapping = local_mapping; cfg.window = window
        if T0 is not None:
            cfg.T_wc_init = (C.c_double * 16)(*np.asarray(T0, np.float64).reshape(16))
        if imu is not None:
            cfg.use_imu = 1
            cfg.gravity = (C.c_double * 3)(*imu["gravity"])
            cfg.gyro_noise_density, cfg.gyro_random_walk, cfg.accel_noise_density, cfg.accel_random_walk = imu["noise"]
            cfg.T_body_sensor = (C.c_double * 16)(*np.asarray(imu["T_bs"], np.float64).reshape(16))
            cfg.imu_hz = int(imu["hz"])
            if "velocity" in imu:
                cfg.velocity_init = (C.c_double * 3)(*imu["velocity"])
        self.w, self.h = rig["w"], rig["h"]
        self.h_sys = C.c_void_p()
        _chk(self.L.vslam_system_create_mono(C.byref(cfg), C.c_double(fps), C.byref(self.h_sys)))

    def track(self, left, frame_number, imu_bucket, channels=1, on_device=False, stride=None):
        """left: u8 array ((H, W) gray, (H, W, 3) BGR, (H, W, 4) BGRA) or a device pointer (on_device, with `channels`);
        imu_bucket: (acc (n,3), gyro (n,3), timestamps_ns (n)) since the previous call, or None (an error)."""
        T = np.zeros((4, 4))
        rep = MonoFrameReport()
        b = None
        keep = []
        if imu_bucket is not None:
            acc, gyr, ts = (np.ascontiguousarray(a, np.float64) for a in imu_bucket)
            keep = [acc, gyr, ts]
            b = ImuBucket(len(ts), _p(acc), _p(gyr), _p(ts))
        if on_device:
            lp, st, ch = C.c_void_p(left), stride or self.w * channels, channels
        else:
            left, ch, st = _image(left, self.h, self.w)
            keep.append(left)
            lp = _p(left)
        _chk(self.L.vslam_system_track_mono_imu(self.h_sys, lp, int(st), int(ch), int(on_device), int(frame_number),
                                                C.byref(b) if b is not None else None, _p(T), C.byref(rep)))
        return T, {f[0]: getattr(rep, f[0]) for f in MonoFrameReport._fields_}

    def memory(self):
        n, b = C.c_int32(), C.c_int64()
        _chk(self.L.vslam_system_memory(self.h_sys, C.byref(n), C.byref(b)))
        return dict(key_slots_used=n.value, key_slab_bytes=b.value)


class KeyBlock:
    """a key set (keypoints + descriptors, no right keys) resident in a device block, as vslam_kf_keys_upload writes it"""

    def __init__(self, kps, desc, device=0):
        self.L = lib()
        self.L.vslam_device_alloc.argtypes = [C.c_int32, C.c_size_t, C.POINTER(C.c_void_p)]
        self.L.vslam_device_free.argtypes = [C.c_int32, C.c_void_p]
        self.L.vslam_device_free.restype = None
        self.device = device
        self.n = len(kps)
        p = C.c_void_p()
        _chk(self.L.vslam_device_alloc(device, kf_keys_bytes(self.n, 0), C.byref(p)))
        self.ptr = p.value
        e = np.zeros(0, np.int32)
        kf_keys_upload(dict(T_wc=np.eye(4), id=0, kpsL=kps, descL=np.ascontiguousarray(desc, np.uint8).reshape(-1, 32),
                            kpsR=np.zeros(0, KP_DTYPE), descR=np.zeros((0, 32), np.uint8), rightIdxs=np.full(self.n, -1, np.int32),
                            leftIdxs=e, unF=e, unFR=e), self.ptr, device)

    def free(self):
        if self.ptr:
            self.L.vslam_device_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def match_by_radius_window(matcher, last, targets, rad, matchedL):
    """matchByRadius from the KeyBlock `last` into the KeyBlocks `targets` in order on one claim table (addMappointsMono);
    returns (n_matches per target, matchedL, match_out [n_targets][n_last])."""
    nT = len(targets)
    ptrs = (C.c_void_p * max(nT, 1))(*[t.ptr for t in targets])
    nt = np.array([t.n for t in targets], np.int32)
    mL = np.array(matchedL, np.int32, copy=True)
    out_c = np.full(max(nT * last.n, 1), -1, np.int32)
    nm = np.zeros(max(nT, 1), np.int32)
    matcher.L.vslam_match_by_radius_window.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_float,
                                                       C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    _chk(matcher.L.vslam_match_by_radius_window(matcher.h, last.ptr, last.n, ptrs if nT else None, _p(nt) if nT else None, nT,
                                                C.c_float(rad), _p(mL) if len(mL) else None, len(mL), _p(out_c), _p(nm)))
    return nm[:nT].copy(), mL, out_c[:nT * last.n].reshape(nT, last.n).copy()


class DeviceImage:
    """a u8 image uploaded into a device buffer of the library's allocator (vslam_device_alloc); .ptr for the *_device calls"""

    def __init__(self, img, device=0):
        self.L = lib()
        self.L.vslam_device_alloc.argtypes = [C.c_int32, C.c_size_t, C.POINTER(C.c_void_p)]
        self.L.vslam_device_upload.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t]
        self.L.vslam_device_free.argtypes = [C.c_int32, C.c_void_p]
        self.L.vslam_device_free.restype = None
        a = np.ascontiguousarray(img, np.uint8)
        self.device = device
        p = C.c_void_p()
        _chk(self.L.vslam_device_alloc(device, a.nbytes, C.byref(p)))
        self.ptr = p.value
        _chk(self.L.vslam_device_upload(device, self.ptr, a.ctypes.data, a.nbytes))

    def free(self):
        if self.ptr:
            self.L.vslam_device_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- N3: rectification and dataset bookkeeping -----------------------------------------------------------------------
class Rectifier:
    """vslam_rectifier: initUndistortRectifyMap once, remap(INTER_LINEAR) per frame (device images)."""

    def __init__(self, K, D, R, Pnew, src_size, size, device=0):
        self.L = lib()
        K = np.ascontiguousarray(K, np.float64).reshape(9); Pn = np.ascontiguousarray(Pnew, np.float64).reshape(9)
        Dv = np.ascontiguousarray(D if D is not None else [], np.float64).ravel()
        Rv = np.ascontiguousarray(R, np.float64).reshape(9) if R is not None else None
        self.w, self.h = size
        self.sw, self.sh = src_size
        self.h_r = C.c_void_p()
        _chk(self.L.vslam_rectifier_create(_p(K), _p(Dv) if len(Dv) else None, len(Dv), _p(Rv) if Rv is not None else None, _p(Pn),
                                           self.sw, self.sh, self.w, self.h, device, C.byref(self.h_r)))

    def maps(self):
        mx = np.zeros((self.h, self.w), np.float32); my = np.zeros((self.h, self.w), np.float32)
        _chk(self.L.vslam_rectifier_maps(self.h_r, _p(mx), _p(my)))
        return mx, my

    def remap(self, images):
        """host u8 images (sh x sw gray, or sh x sw x 3 BGR / x 4 BGRA, all alike) -> list of rectified gray host images (h x w)"""
        n = len(images)
        src = [_image(i, self.sh, self.sw) for i in images]
        ch, st = src[0][1], src[0][2]
        if any(c != ch for _, c, _ in src):
            raise ValueError("remap: images differ in channels")
        dst = [np.zeros((self.h, self.w), np.uint8) for _ in range(n)]
        sp = (C.c_void_p * n)(*[a.ctypes.data for a, _, _ in src]); dp = (C.c_void_p * n)(*[a.ctypes.data for a in dst])
        if ch == 1:
            _chk(self.L.vslam_rectifier_remap_host(self.h_r, sp, self.sw, dp, self.w, n))
        else:
            _chk(self.L.vslam_rectifier_remap_gray_host(self.h_r, sp, int(st), int(ch), dp, self.w, n))
        return dst

    def remap_device(self, src_ptrs, src_stride, dst_ptrs, dst_stride, channels=1):
        """device images: sources gray (channels = 1) or BGR / BGRA, destinations gray"""
        n = len(src_ptrs)
        sp = (C.c_void_p * n)(*src_ptrs); dp = (C.c_void_p * n)(*dst_ptrs)
        if channels == 1:
            _chk(self.L.vslam_rectifier_remap(self.h_r, sp, int(src_stride), dp, int(dst_stride), n))
        else:
            _chk(self.L.vslam_rectifier_remap_gray(self.h_r, sp, int(src_stride), int(channels), dp, int(dst_stride), n))

    def close(self):
        if self.h_r:
            self.L.vslam_rectifier_destroy(self.h_r)
            self.h_r = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Dataset:
    """vslam_dataset: EuRoC (kind 0) / KITTI (kind 1) frame lists, IMU buckets per frame, gravity guess."""

    def __init__(self, kind, images_path, imu_path=None):
        self.L = lib()
        self.h_d = C.c_void_p()
        _chk(self.L.vslam_dataset_open(int(kind), images_path.encode(), imu_path.encode() if imu_path else None, C.byref(self.h_d)))

    def __len__(self):
        return self.L.vslam_dataset_frames(self.h_d)

    def frame(self, i):
        l = C.c_char_p(); r = C.c_char_p(); t = C.c_double()
        _chk(self.L.vslam_dataset_frame(self.h_d, i, C.byref(l), C.byref(r), C.byref(t)))
        return l.value.decode(), r.value.decode(), t.value

    def imu_bucket(self, i):
        b = ImuBucket()
        _chk(self.L.vslam_dataset_imu_bucket(self.h_d, i, C.byref(b)))
        n = b.n
        if n == 0:
            return np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0)
        acc = np.ctypeslib.as_array(C.cast(b.acceleration, C.POINTER(C.c_double)), (n, 3)).copy()
        gyr = np.ctypeslib.as_array(C.cast(b.angular_velocity, C.POINTER(C.c_double)), (n, 3)).copy()
        ts = np.ctypeslib.as_array(C.cast(b.timestamps_ns, C.POINTER(C.c_double)), (n,)).copy()
        return acc, gyr, ts

    def gravity(self):
        v = C.c_int32(); g = (C.c_double * 3)()
        _chk(self.L.vslam_dataset_gravity(self.h_d, C.byref(v), g))
        return bool(v.value), tuple(g)

    def close(self):
        if self.h_d:
            self.L.vslam_dataset_close(self.h_d)
            self.h_d = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- vslam_batch: B lanes in lockstep, one launch per stage for all lanes --------------------------------------------------
def _report_dict(rep):
    d = {f[0]: getattr(rep, f[0]) for f in FrameReport._fields_ if f[0] != "ba_report"}
    d["ba_report"] = [dict(iterations=r.iterations, inner=r.inner_iterations, initialError=r.initial_error,
                           finalError=r.final_error, lam=r.lam) for r in rep.ba_report]
    return d


class _BorrowedSystem(System):
    """a lane's vslam_system (owned by the batch): the read-out methods of System"""

    def __init__(self, L, handle, rig=None):      # noqa: super().__init__ creates a session; this one is borrowed
        self.L = L
        self.h_sys = C.c_void_p(handle)
        self.rig = rig                  # (global_ba_problem hands it on)

    def close(self):
        self.h_sys = C.c_void_p()


class Batch:
    """vslam_batch: `lanes` sessions tracked in lockstep.  T0s: per-lane initial poses (or None), velocities: per-lane (IMU).
    rig: the camera of every lane; rigs=[...]: one rig dict per lane (a lane per robot: fx, fy, cx, cy, bl may differ, the image
    size may not; `rig` may then be None)."""

    def __init__(self, rig, nfeatures, lanes, T0s=None, imu=None, velocities=None, local_mapping=1, window=10, device=0,
                 host_threads=-1, mapping_threads=0, mapping_delay=0, mapping_np_delay=0, rigs=None):
        self.L = lib()
        self.L.vslam_batch_system.restype = C.c_void_p
        self.lanes = lanes
        if rigs is not None and len(rigs) != lanes:
            raise ValueError("Batch: rigs needs one rig per lane")
        self.rigs = list(rigs) if rigs is not None else [rig] * lanes
        rig = self.rigs[0]
        self._cfg = dict(nfeatures=nfeatures, imu=imu, local_mapping=local_mapping, window=window, device=device, mapping_delay=mapping_delay,
                         mapping_np_delay=mapping_np_delay)
        cfgs = (SystemConfig * lanes)()
        for b in range(lanes):
            cfgs[b] = self._config(self.rigs[b], T0s[b] if T0s is not None else None, velocities[b] if velocities is not None else None)
        self.w, self.h = rig["w"], rig["h"]
        self.h_b = C.c_void_p()
        _chk(self.L.vslam_batch_create(cfgs, lanes, host_threads, mapping_threads, C.byref(self.h_b)))

    def _config(self, rig, T0, velocity, **over):
        """a lane's vslam_system_config (over: fields set after the defaults, e.g. mapping_delay)"""
        kw = dict(self._cfg)
        nfeatures = over.pop("nfeatures", kw.pop("nfeatures"))
        im = None
        if kw["imu"] is not None:
            im = dict(kw["imu"])
            if velocity is not None:
                im["velocity"] = velocity
        kw["imu"] = over.pop("imu", im)
        kw.update(over)
        c = system_config(rig, nfeatures, **kw)
        if T0 is not None:
            c.T_wc_init = (C.c_double * 16)(*np.asarray(T0, np.float64).reshape(16))
        return c

    def restart_lane(self, lane, rig=None, T0=None, velocity=None, **over):
        """ends lane `lane`'s session and starts a new one in its place (vslam_batch_restart_lane), between two track() calls.
        rig: the new session's camera (None: the lane's previous one); T0 / velocity: its initial pose / velocity.  over: other
        config fields (nfeatures, imu, local_mapping, mapping_delay, mapping_np_delay) - the batch refuses what differs from its
        shared settings.  The lane's next frame carries frame number 0; rectifiers must be bound again for raw frames.
        With no argument but the lane, the library restarts it on its previous configuration (config = NULL: same rig, same
        initial pose and velocity).  As soon as anything is given, a whole new config is built: T0 = None is then the identity
        and velocity = None zero, not the previous session's."""
        lane = int(lane)
        if rig is None and T0 is None and velocity is None and not over:
            _chk(self.L.vslam_batch_restart_lane(self.h_b, lane, None))
            return
        r = rig if rig is not None else (self.rigs[lane] if 0 <= lane < self.lanes else self.rigs[0])
        c = self._config(r, T0, velocity, **over)
        _chk(self.L.vslam_batch_restart_lane(self.h_b, lane, C.byref(c)))
        self.rigs[lane] = r

    def memory(self):
        """key slabs (HBM) the batch has allocated in total, and how many of them sessions hold / its free list holds"""
        nb = C.c_int64(); u = C.c_int32(); f = C.c_int32()
        _chk(self.L.vslam_batch_memory(self.h_b, C.byref(nb), C.byref(u), C.byref(f)))
        return dict(key_slab_bytes=nb.value, slabs_in_use=u.value, slabs_free=f.value)

    def close(self):
        if self.h_b:
            self.L.vslam_batch_destroy(self.h_b)
            self.h_b = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_rectifiers(self, lane, left, right):
        """bind lane `lane`'s (-1: every lane's) Rectifier objects for the raw=True calls (None, None unbinds); they must
        outlive the batch.  All lanes' sources share one size, stride and channel count per call."""
        _chk(self.L.vslam_batch_set_rectifiers(self.h_b, int(lane), left.h_r if left is not None else None,
                                               right.h_r if right is not None else None))
        self.src_size = (left.sw, left.sh) if left is not None else None

    def _images(self, lefts, rights, mask, on_device, stride, channels, keep, raw=False):
        """per-lane pointer tables, row stride and channels (host arrays: (H, W), (H, W, 3) BGR or (H, W, 4) BGRA, all alike;
        raw: of the rectifiers' source size)"""
        B = self.lanes
        lp = (C.c_void_p * B)(); rp = (C.c_void_p * B)()
        w, h = (getattr(self, "src_size", None) or (self.w, self.h)) if raw else (self.w, self.h)
        st, ch = stride or w * channels, channels
        seen = set()
        for b in range(B):
            if mask is not None and not mask[b]:
                continue
            if on_device:
                lp[b], rp[b] = lefts[b], rights[b]
            else:
                l, cl, sl = _image(lefts[b], h, w); r, cr, sr = _image(rights[b], h, w)
                seen |= {(cl, sl), (cr, sr)}
                keep += [l, r]
                lp[b], rp[b] = l.ctypes.data, r.ctypes.data
                ch, st = cl, sl
        if len(seen) > 1:
            raise ValueError("Batch.track: the lanes' images differ in channels")
        return lp, rp, st, ch

    def track(self, lefts, rights, frame_numbers, imu_buckets=None, mask=None, on_device=False, stride=None, channels=1, raw=False):
        """lefts / rights: per-lane u8 arrays (host: gray, BGR or BGRA) or device pointers (with `channels`); imu_buckets:
        per-lane (acc, gyro, ts) or None entries.  raw: unrectified frames through the lanes' bound rectifiers."""
        B = self.lanes
        T = np.zeros((B, 4, 4))
        reps = (FrameReport * B)()
        keep = []
        lp, rp, st, ch = self._images(lefts, rights, mask, on_device, stride, channels, keep, raw)
        bk = self._buckets(imu_buckets, keep)
        fr = np.ascontiguousarray(frame_numbers, np.int32)
        mk = np.ascontiguousarray(mask, np.uint8) if mask is not None else None
        if raw:
            _chk(self.L.vslam_batch_track_stereo_raw(self.h_b, lp, rp, int(st), int(ch), int(on_device), _p(fr), bk,
                                                     _p(mk) if mk is not None else None, _p(T), reps))
        elif ch == 1:
            _chk(self.L.vslam_batch_track_stereo(self.h_b, lp, rp, int(st), int(on_device), _p(fr), bk, _p(mk) if mk is not None else None,
                                                 _p(T), reps))
        else:
            _chk(self.L.vslam_batch_track_stereo_color(self.h_b, lp, rp, int(st), int(ch), int(on_device), _p(fr), bk,
                                                       _p(mk) if mk is not None else None, _p(T), reps))
        return T, [_report_dict(reps[b]) for b in range(B)]

    def track_prefetch(self, lefts, rights, frame_numbers, next_lefts=None, next_rights=None, imu_buckets=None, mask=None,
                       next_mask=None, stride=None, channels=1, raw=False):
        """device images of this step and (optionally) of the next one, whose extraction then starts under this step's host
        phases; the next call must pass exactly those pointers and channels (and raw) to use it"""
        B = self.lanes
        T = np.zeros((B, 4, 4))
        reps = (FrameReport * B)()
        keep = []
        lp, rp, st, ch = self._images(lefts, rights, mask, True, stride, channels, keep, raw)
        nl = nr = None
        if next_lefts is not None:
            nl, nr, _, _ = self._images(next_lefts, next_rights, next_mask, True, stride, channels, keep, raw)
        bk = self._buckets(imu_buckets, keep)
        fr = np.ascontiguousarray(frame_numbers, np.int32)
        mk = np.ascontiguousarray(mask, np.uint8) if mask is not None else None
        nmk = np.ascontiguousarray(next_mask, np.uint8) if next_mask is not None else None
        args = (_p(fr), bk, _p(mk) if mk is not None else None, _p(T), reps, nl, nr, _p(nmk) if nmk is not None else None)
        if raw:
            _chk(self.L.vslam_batch_track_stereo_prefetch_raw(self.h_b, lp, rp, int(st), int(ch), *args))
        elif ch == 1:
            _chk(self.L.vslam_batch_track_stereo_prefetch(self.h_b, lp, rp, int(st), *args))
        else:
            _chk(self.L.vslam_batch_track_stereo_prefetch_color(self.h_b, lp, rp, int(st), int(ch), *args))
        return T, [_report_dict(reps[b]) for b in range(B)]

    def relocalize(self, lefts, rights, frame_numbers, mask=None, on_device=False, stride=None, **params):
        """vslam_batch_relocalize with gray frames: (T_wc [lanes, 4, 4], reports).  A masked lane's T row is the recovered
        pose, or its unchanged camera pose on failure; the rows and reports (None) of lanes outside the mask are not written."""
        B = self.lanes
        T = np.zeros((B, 4, 4))
        reps = (RelocReport * B)()
        keep = []
        lp, rp, st, ch = self._images(lefts, rights, mask, on_device, stride, 1, keep)
        if ch != 1:
            raise ValueError("relocalize takes gray frames")
        fr = np.ascontiguousarray(frame_numbers, np.int32)
        mk = np.ascontiguousarray(mask, np.uint8) if mask is not None else None
        prm = RelocParams(**{k: int(v) for k, v in params.items()})
        _chk(self.L.vslam_batch_relocalize(self.h_b, lp, rp, int(st), int(on_device), _p(fr), _p(mk) if mk is not None else None,
                                           C.byref(prm), _p(T), reps))
        return T, [_reloc_report_dict(reps[b]) if mask is None or mask[b] else None for b in range(B)]

    def relocalize_imu(self, lefts, rights, frame_numbers, imu_buckets=None, mask=None, on_device=False, stride=None, **params):
        """vslam_batch_relocalize_imu with gray frames: (T_wc [lanes, 4, 4], reports, IMU reports).  imu_buckets: per-lane
        (acc, gyro, ts) for the lanes whose velocity is pending, None entries elsewhere (or None if no lane is)."""
        B = self.lanes
        T = np.zeros((B, 4, 4))
        reps = (RelocReport * B)(); ireps = (RelocImuReport * B)()
        keep = []
        lp, rp, st, ch = self._images(lefts, rights, mask, on_device, stride, 1, keep)
        if ch != 1:
            raise ValueError("relocalize takes gray frames")
        bk = self._buckets(imu_buckets, keep)
        fr = np.ascontiguousarray(frame_numbers, np.int32)
        mk = np.ascontiguousarray(mask, np.uint8) if mask is not None else None
        prm = RelocParams(**{k: int(v) for k, v in params.items()})
        _chk(self.L.vslam_batch_relocalize_imu(self.h_b, lp, rp, int(st), int(on_device), _p(fr), bk, _p(mk) if mk is not None else None,
                                               C.byref(prm), _p(T), reps, ireps))
        on = [mask is None or bool(mask[b]) for b in range(B)]
        return (T, [_reloc_report_dict(reps[b]) if on[b] else None for b in range(B)],
                [_reloc_imu_report_dict(ireps[b]) if on[b] else None for b in range(B)])

    def _loop_mask(self, mask):
        mk = np.ones(self.lanes, np.uint8) if mask is None else np.ascontiguousarray(mask, np.uint8)
        assert len(mk) == self.lanes
        return mk

    def close_loop(self, mask=None, **params):
        """vslam_batch_close_loop on the frames of the last track(): per masked lane (None: all) what System.close_loop does, the
        detection and the pose-graph solves batched.  Returns the per-lane report dicts (None for lanes outside the mask)."""
        mk = self._loop_mask(mask)
        reps = (LoopReport * self.lanes)()
        prm = System._loop_params(params)
        _chk(self.L.vslam_batch_close_loop(self.h_b, _p(mk), C.byref(prm), reps))
        return [_loop_report_dict(reps[b]) if mk[b] else None for b in range(self.lanes)]

    def correct_loop(self, kf_loops, poses, mask=None, **params):
        """vslam_batch_correct_loop: kf_loops [lanes], poses [lanes, 4, 4] (read for the masked lanes; None entries allowed
        elsewhere).  Returns the per-lane report dicts (None for lanes outside the mask)."""
        mk = self._loop_mask(mask)
        kf = np.array([int(k) if k is not None else 0 for k in kf_loops], np.int32)
        T = np.zeros((self.lanes, 4, 4))
        for b in range(self.lanes):
            if poses[b] is not None:
                T[b] = np.asarray(poses[b], np.float64).reshape(4, 4)
        reps = (LoopReport * self.lanes)()
        prm = System._loop_params(params)
        _chk(self.L.vslam_batch_correct_loop(self.h_b, _p(mk), _p(kf), _p(T), C.byref(prm), reps))
        return [_loop_report_dict(reps[b]) if mk[b] else None for b in range(self.lanes)]

    def close_loop_imu(self, mask=None, **params):
        """vslam_batch_close_loop_imu (an IMU batch): per masked lane what System.close_loop_imu does, the detection batched and ONE
        yaw-only solve for all lanes.  Returns [(report dict, IMU report dict) or None for lanes outside the mask]."""
        mk = self._loop_mask(mask)
        reps = (LoopReport * self.lanes)(); ireps = (LoopImuReport * self.lanes)()
        prm = System._loop_params(params)
        _chk(self.L.vslam_batch_close_loop_imu(self.h_b, _p(mk), C.byref(prm), reps, ireps))
        return [(_loop_report_dict(reps[b]), _loop_imu_report_dict(ireps[b])) if mk[b] else None for b in range(self.lanes)]

    def correct_loop_imu(self, kf_loops, poses, mask=None, **params):
        """vslam_batch_correct_loop_imu: kf_loops [lanes], poses [lanes, 4, 4] (read for the masked lanes; None entries allowed
        elsewhere).  Returns [(report dict, IMU report dict) or None for lanes outside the mask]."""
        mk = self._loop_mask(mask)
        kf = np.array([int(k) if k is not None else 0 for k in kf_loops], np.int32)
        T = np.zeros((self.lanes, 4, 4))
        for b in range(self.lanes):
            if poses[b] is not None:
                T[b] = np.asarray(poses[b], np.float64).reshape(4, 4)
        reps = (LoopReport * self.lanes)(); ireps = (LoopImuReport * self.lanes)()
        prm = System._loop_params(params)
        _chk(self.L.vslam_batch_correct_loop_imu(self.h_b, _p(mk), _p(kf), _p(T), C.byref(prm), reps, ireps))
        return [(_loop_report_dict(reps[b]), _loop_imu_report_dict(ireps[b])) if mk[b] else None for b in range(self.lanes)]

    def fuse_loop(self, mask=None, **params):
        """vslam_batch_fuse_loop: per masked lane (None: all) what System.fuse_loop does, the searches of all lanes in one batched
        call.  params as System.fuse_loop.  Returns the per-lane report dicts (None for lanes outside the mask)."""
        mk = self._loop_mask(mask)
        reps = (FuseLoopReport * self.lanes)()
        prm = System._fuse_loop_params(params)
        _chk(self.L.vslam_batch_fuse_loop(self.h_b, _p(mk), C.byref(prm), reps))
        return [_fuse_loop_report_dict(reps[b]) if mk[b] else None for b in range(self.lanes)]

    def global_ba(self, mask=None, edge_weight=0.0, max_iterations=0, lambda0=0.0):
        """vslam_batch_global_ba: per masked lane (None: all) what System.global_ba does, the solves of all lanes in one batched
        call.  Returns the per-lane report dicts (None for lanes outside the mask)."""
        mk = self._loop_mask(mask)
        reps = (SystemGbaReport * self.lanes)()
        prm = SystemGbaParams(GbaParams(int(max_iterations), float(lambda0)), float(edge_weight))
        _chk(self.L.vslam_batch_global_ba(self.h_b, _p(mk), C.byref(prm), reps))
        return [_system_gba_report_dict(reps[b]) if mk[b] else None for b in range(self.lanes)]

    def relocalize_debug(self, lane):
        """Matcher.relocalize_debug of lane `lane`: its part of the last relocalize call (test tap)"""
        return _reloc_debug(lambda *a: self.L.vslam_batch_relocalize_debug(self.h_b, int(lane), *a))

    def _buckets(self, imu_buckets, keep):
        B = self.lanes
        bk = None
        if imu_buckets is not None:
            bk = (ImuBucket * B)()
            for b in range(B):
                if imu_buckets[b] is None:
                    continue
                acc, gyr, ts = (np.ascontiguousarray(a, np.float64) for a in imu_buckets[b])
                keep += [acc, gyr, ts]
                bk[b] = ImuBucket(len(ts), acc.ctypes.data, gyr.ctypes.data, ts.ctypes.data)
        return bk

    def system(self, lane):
        return _BorrowedSystem(self.L, self.L.vslam_batch_system(self.h_b, lane), self.rigs[lane])

    def wait_mapping(self):
        _chk(self.L.vslam_batch_wait_mapping(self.h_b))

    def set_timing(self, on):
        _chk(self.L.vslam_batch_set_timing(self.h_b, int(on)))

    def timings(self):
        names = (C.c_char_p * 64)(); ms = (C.c_float * 64)(); n = C.c_int32(); ph = (C.c_double * 7)()
        _chk(self.L.vslam_batch_timings(self.h_b, names, ms, 64, C.byref(n), ph))
        out = {}
        for i in range(n.value):
            k = names[i].decode()
            out[k] = out.get(k, 0.0) + ms[i]
        return out, list(ph)


# ---- vslam_fleet: S sessions on S library threads ------------------------------------------------------------------------
class FleetSequence(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("left", C.c_void_p), ("right", C.c_void_p), ("stride", C.c_int32), ("on_device", C.c_int32),
                ("imu_forward", C.c_void_p), ("imu_backward", C.c_void_p), ("T_wc_true", C.c_void_p), ("velocity_true", C.c_void_p),
                ("start_span", C.c_int32)]


class FleetReport(C.Structure):
    _fields_ = [("n_sessions", C.c_int32)] + [(n, C.c_int64) for n in ("frames", "keyframes", "mappings", "new_points", "ba_landmarks",
                                                                      "ba_pairs", "ba_residuals", "ba_free_kf", "ba_sum_k2", "ba_trials", "ba_iterations", "ba_rounds",
                                                                      "sum_inliers", "sum_rounds", "lost_frames", "sum_active")] + \
               [("min_inliers", C.c_int32), ("seconds", C.c_double), ("max_session_seconds", C.c_double),
                ("max_position_error", C.c_double), ("sum_sq_position_error", C.c_double)]


def system_config(rig, nfeatures, imu=None, local_mapping=2, window=10, device=0, nlevels=8, scale=1.2, mapping_delay=0, mapping_np_delay=0):
    cfg = SystemConfig()
    cfg.mapping_delay = mapping_delay; cfg.mapping_np_delay = mapping_np_delay
    cfg.fe = FeParams(nfeatures, nlevels, scale, 19, 31, 20, 7)
    cfg.rig = make_rig(rig)
    cfg.device = device; cfg.local_mapping = local_mapping; cfg.window = window
    if imu is not None:
        cfg.use_imu = 1
        cfg.gravity = (C.c_double * 3)(*imu["gravity"])
        cfg.gyro_noise_density, cfg.gyro_random_walk, cfg.accel_noise_density, cfg.accel_random_walk = imu["noise"]
        cfg.T_body_sensor = (C.c_double * 16)(*np.asarray(imu["T_bs"], np.float64).reshape(16))
        cfg.imu_hz = int(imu["hz"])
        if "velocity" in imu:
            cfg.velocity_init = (C.c_double * 3)(*imu["velocity"])
    return cfg


class Fleet:
    """S independent sessions replaying one stereo sequence (device or pinned-host image pointers) as a ping-pong."""

    def __init__(self, cfg, n_sessions, left_ptrs, right_ptrs, stride, on_device, poses=None, velocities=None,
                 imu_forward=None, imu_backward=None, lanes=0, start_span=0):
        """lanes > 0: the sessions are the lanes of ceil(n_sessions / lanes) lockstep groups (vslam_batch)"""
        self.L = lib()
        n = len(left_ptrs)
        self._keep = []
        seq = FleetSequence()
        seq.n_frames = n; seq.stride = stride; seq.on_device = int(on_device); seq.start_span = int(start_span)
        la = (C.c_void_p * n)(*left_ptrs); ra = (C.c_void_p * n)(*right_ptrs)
        self._keep += [la, ra]
        seq.left = C.cast(la, C.c_void_p); seq.right = C.cast(ra, C.c_void_p)

        def buckets(lst):
            arr = (ImuBucket * n)()
            for i, b in enumerate(lst):
                if b is None:
                    continue
                acc, gyr, ts = (np.ascontiguousarray(a, np.float64) for a in b)
                self._keep += [acc, gyr, ts]
                arr[i] = ImuBucket(len(ts), _p(acc), _p(gyr), _p(ts))
            self._keep.append(arr)
            return C.cast(arr, C.c_void_p)

        if imu_forward is not None:
            seq.imu_forward = buckets(imu_forward); seq.imu_backward = buckets(imu_backward)
        if poses is not None:
            P = np.ascontiguousarray(poses, np.float64).reshape(n, 16); self._keep.append(P); seq.T_wc_true = _p(P)
        if velocities is not None:
            V = np.ascontiguousarray(velocities, np.float64).reshape(n, 3); self._keep.append(V); seq.velocity_true = _p(V)
        self.h = C.c_void_p()
        if lanes > 0:
            _chk(self.L.vslam_fleet_create_batched(C.byref(cfg), int(n_sessions), C.byref(seq), int(lanes), C.byref(self.h)))
        else:
            _chk(self.L.vslam_fleet_create(C.byref(cfg), int(n_sessions), C.byref(seq), C.byref(self.h)))
        self.n_sessions = n_sessions

    def run(self, n_steps):
        rep = FleetReport()
        _chk(self.L.vslam_fleet_run(self.h, int(n_steps), C.byref(rep)))
        return {f[0]: getattr(rep, f[0]) for f in FleetReport._fields_}

    def set_sampling(self, every):
        _chk(self.L.vslam_fleet_set_sampling(self.h, int(every)))

    def timings(self):
        names = (C.c_char_p * 64)(); ms = (C.c_float * 64)(); n = C.c_int32(); cnt = (C.c_int64 * 4)()
        _chk(self.L.vslam_fleet_timings(self.h, names, ms, 64, C.byref(n), cnt))
        return {names[i].decode(): float(ms[i]) for i in range(n.value)}, dict(frames=cnt[0], solves=cnt[1], ba=cnt[2], ba_cohorts=cnt[3])

    def close(self):
        if self.h:
            self.L.vslam_fleet_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
